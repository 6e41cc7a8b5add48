"""The 8-byte register-resident leaves on the array's 16-byte grid: leaf17_kernel and regpart_kernel read a segment as
16-byte vectors of two elements from the 16-byte boundary at or below its start, and write whole vectors with single
elements at both ends.  msd_sort_u64_segments and msd_sort_pairs_u64_segments on a segment list that pins the edges of
that grid (the u64 counterpart of test_gpu_leaf16_pipeline.py):

  * segment starts are even and odd;
  * (start % 2) + count = 17406, 17407, 17408 (the last vectors of the 17408-element grid) and 17409 (one above the
    capacity: left to the other leaves), each at an even and at an odd start;
  * a segment of 2 and one of 3 elements at an odd start;
  * the array's last segment ends on an odd index, and the array with it.

Every list runs three times: leaf17 on and regpart 0, leaf17 0 and regpart 1, the defaults.  Which kernel that means
depends on the type (csrc/msd_radix.hip, rounds() and lds_leaves()): u64 keys of up to 17408 elements are leaves, taken
by leaf17_kernel<NoVal> when leaf17 is on and by the LDS leaf otherwise -- the register partition never sees them;
tuples of 3073 .. 17407 elements take a register-resident pass when regpart is on and at least 64 segments qualify:
leaf17_kernel with leaf17 on, regpart_kernel without.  So, of the edge cases:
  * u64 keys: every segment of up to 17408 keys reaches leaf17_kernel<NoVal> when it is on.  The one of 17408 keys at an
    odd start (17409 grid elements) is rejected on the device and finished by the LDS leaf; the one of 17409 keys is no
    leaf at all and takes a general round.  With leaf17 0 ("regpart" mode) neither kernel under test runs for keys: that
    run pins the paths that take over.  No counter says how many segments leaf17_kernel<NoVal> handed on
    (`leaf17_rejected` counts the tuple pass only), so the over-capacity cases are checked by their result.
  * tuples: the host sends a segment to the register-resident pass if its count is at most 17407, whatever its start: of
    the list, (even, 17406), (odd, 17405), (even, 17407), (odd, 17406) and (odd, 17407: all 17408 grid elements); the
    segments of 17408 and 17409 tuples take a general round.
  * the segments of 2 and 3 elements reach neither kernel in any mode (leaf17_kernel<NoVal> leaves segments below 4096
    keys to the LDS leaf, the tuple pass starts at 3073): they pin that an odd start next to the kernels' segments is
    left alone by them.

The expectation is numpy's sort per segment; for tuples the row ids follow a stable argsort (the keys are distinct by
construction: the passes are not stable).  One-element spacers between the segments, the elements in front of the first
one and the guard bands around the arrays (tests/guardband.py) must stay as they are.
"""
import functools

import numpy as np
import pytest
import torch

from gpu_support import DEFAULTS
from guardband import Arena, guard_elems

pytestmark = pytest.mark.gpu

CAP = 17408       # kL17Cap (csrc/msd_leaf17.hpp) = kRpCap (csrc/msd_regpart.hpp): elements on the 16-byte grid
END_BIT = 56
LEAD = 7          # elements in front of the first segment: they belong to no segment
MODES = {"leaf17": {"leaf17": 1, "regpart": 0}, "regpart": {"leaf17": 0, "regpart": 1}, "defaults": {}}


@functools.lru_cache(None)
def case(typ):
    """(keys, offsets, expected keys, expected row ids) of ``typ``'s list, built once"""
    # fillers keep the list in the regime of the kernels under test: u64 keys need an average segment of >= 8192 keys for
    # leaf17_kernel to be launched, tuples at least 64 segments that fit a workgroup's registers
    fill = [16000 + 2 * i for i in range(12)] if typ == "u64" else [3100 + 2 * i for i in range(64)]
    sizes, at, starts = [], LEAD, {}

    def seg(count, parity):
        nonlocal at
        if at % 2 != parity:                       # a one-element spacer (never moved) turns the start's parity
            sizes.append(1)
            at += 1
        starts[(count, parity)] = at
        sizes.append(count)
        at += count

    f = iter(fill)
    for tot in (CAP - 2, CAP - 1, CAP, CAP + 1):
        for parity in (0, 1):
            seg(tot - parity, parity)
            seg(next(f), at % 2)                   # an ordinary segment between two of the edge cases
    seg(2, 1)
    seg(3, 1)
    for c in f:
        seg(c, at % 2)
    seg(9001 if at % 2 == 0 else 9000, at % 2)     # the last segment, and the array, end on an odd index
    assert at % 2 == 1 and all(starts[(t - p, p)] % 2 == p for t in (CAP - 2, CAP - 1, CAP, CAP + 1) for p in (0, 1))
    offs = np.concatenate(([LEAD], LEAD + np.cumsum(sizes))).astype(np.uint64)
    n = int(offs[-1])
    rng = np.random.default_rng(17 + len(typ))
    # distinct keys: 36 random bits above the element's index
    k = (rng.integers(0, 1 << 36, n, dtype=np.uint64) << np.uint64(20)) | np.arange(n, dtype=np.uint64)
    for i in range(len(sizes)):
        a, b = int(offs[i]), int(offs[i + 1])
        k[a:b] |= np.uint64((7 * i + 1) % 256) << np.uint64(END_BIT)
    want, rid = k.copy(), np.arange(n, dtype=np.uint64)
    for i in range(len(sizes)):
        a, b = int(offs[i]), int(offs[i + 1])
        o = np.argsort(k[a:b], kind="stable")
        want[a:b] = k[a:b][o]
        rid[a:b] = a + o
    assert (want[:LEAD] == k[:LEAD]).all()
    for arr in (k, offs, want, rid):
        arr.setflags(write=False)
    return k, offs, want, rid


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("typ", ["u64", "pairs"])
def test_grid_edges(ctx, typ, mode):
    k, offs, want, want_rid = case(typ)
    n, nseg = k.size, offs.size - 1
    guard = guard_elems(8, CAP)
    ka = Arena(torch.int64, n, lead_bytes=16, guard=guard, neighbours="low").fill(k.copy())
    ra = Arena(torch.int64, n, lead_bytes=48, guard=guard, neighbours="high").fill(np.arange(n, dtype=np.uint64)) if typ == "pairs" else None
    for name, v in MODES[mode].items():
        ctx.set_option(name, v)
    try:
        if typ == "pairs":
            ctx._ok(ctx._L.msd_sort_pairs_u64_segments(ctx._h, ka.ptr, ra.ptr, n, ctx._u64arr([int(o) for o in offs]), nseg, END_BIT))
        else:
            ctx._ok(ctx._L.msd_sort_u64_segments(ctx._h, ka.ptr, n, ctx._u64arr([int(o) for o in offs]), nseg, END_BIT))
        st = ctx.stats()
    finally:
        for name in MODES[mode]:
            ctx.set_option(name, DEFAULTS[name])
    print(f"{typ} {mode}: n={n} segments={nseg} stats={ {s: st.get(s, 0) for s in ('leaf17_launches', 'leaf17_segments', 'leaf17_rejected', 'regpart_rounds', 'rounds', 'small_segments')} }")
    ka.check(f"{typ} keys, {mode}")
    out = ka.host(np.uint64)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{bad.size} keys differ, first at {bad[:8]} (segments {np.searchsorted(offs, bad[:8], side='right') - 1})"
    if typ == "pairs":
        ra.check(f"row ids, {mode}")
        bad = np.flatnonzero(ra.host(np.uint64) != want_rid)
        assert bad.size == 0, f"{bad.size} row ids differ, first at {bad[:8]}"
    # the intended kernel ran
    leaf17 = MODES[mode].get("leaf17", DEFAULTS["leaf17"])
    regpart = MODES[mode].get("regpart", DEFAULTS["regpart"])
    if typ == "u64":
        assert st.get("leaf17_launches", 0) == (1 if leaf17 else 0) and st.get("regpart_rounds", 0) == 0, st
    elif not regpart:
        assert st.get("leaf17_segments", 0) == 0 and st.get("regpart_rounds", 0) == 0, st
    elif leaf17:
        assert st.get("leaf17_segments", 0) >= 64 and st.get("regpart_rounds", 0) == 0, st
    else:
        assert st.get("regpart_rounds", 0) >= 1 and st.get("leaf17_segments", 0) == 0, st
