"""count_place16_kernel with two key register sets: the next segment's keys are requested while the current one is
still placed, and the store phase leaves the counters clear.  msd_sort_u32_segments with ``count16 = 2`` (every
counting-leaf segment goes through the kernel first) on the lists where that order of events matters, against np.sort:

  * taken and rejected segments alternate -- the early request runs next to a segment that is not read, and the
    counters of a rejected segment are cleared by another path than those of a sorted one;
  * segment starts 0-3 modulo 4, counts that end on and around the kernel's capacity of 17408 grid elements;
  * 9-16 open bits; a value with 255 and with 256 copies (the byte counter's limit);
  * the array's last segment ending 1-3 elements short of a 16-byte vector;
  * one segment, and 2 * CUs + 1 segments (every workgroup of the persistent grid but one sorts exactly one).

Keys outside the segments (one-element spacers, the gaps at both ends) are random and must stay where they are.
"""
import numpy as np
import pytest
import torch

from gpu_support import DEFAULTS

pytestmark = pytest.mark.gpu

CAP = 17408             # kC16Cap (csrc/msd_count16.hpp): elements on the 16-byte grid
KCOUNTMEDMAX = 1 << 17  # kCountMedMax (csrc/msd_device.hpp): longest segment of the counting-leaf list


@pytest.fixture(autouse=True)
def count16_always(ctx):
    ctx.set_option("count16", 2)
    yield
    ctx.set_option("count16", DEFAULTS["count16"])


def run_segments(ctx, segs, end_bit, lead=0, trail=0, seed=0):
    """``segs``: list of (size, kind).  Segment i lies behind segment i - 1 (sizes of 1 serve as spacers: never moved);
    ``lead`` / ``trail`` elements in front of the first / behind the last belong to no segment.  Kinds: "u" uniform
    values, "c255" / "c256" uniform values of the upper half plus one value with that many copies, "crowd" 300 keys on
    the first 128 values (more than 255 keys for one thread's counters), "same" one value."""
    rng = np.random.default_rng(seed * 1000 + end_bit)
    offs = [lead]
    for sz, _ in segs:
        offs.append(offs[-1] + sz)
    n = offs[-1] + trail
    k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    nv = 1 << end_bit
    for i, (sz, kind) in enumerate(segs):
        a = offs[i]
        if sz < 2:
            continue
        if kind == "u":
            v = rng.integers(0, nv, sz, dtype=np.uint32)
        elif kind in ("c255", "c256"):
            c = int(kind[1:])
            v = rng.integers(nv // 2, nv, sz, dtype=np.uint32)
            v[rng.permutation(sz)[:c]] = 5
        elif kind == "crowd":
            v = rng.integers(nv // 2, nv, sz, dtype=np.uint32)
            v[rng.permutation(sz)[:300]] = rng.integers(0, min(128, nv // 2), 300, dtype=np.uint32)
        else:
            v = np.full(sz, 3, dtype=np.uint32)
        k[a:a + sz] = v | np.uint32(((i * 37 + 1) % 200) << end_bit)
    want = k.copy()
    for i, (sz, _) in enumerate(segs):
        want[offs[i]:offs[i + 1]] = np.sort(k[offs[i]:offs[i + 1]])
    t = torch.from_numpy(k.view(np.int32)).cuda()
    ctx.sort_segments(t, offs, end_bit)
    st = ctx.stats()
    out = t.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(out != want)
    seg_of = np.searchsorted(offs, bad[:8], side="right") - 1
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[:8]} (segments {seg_of}, offsets {[offs[s] for s in seg_of if 0 <= s < len(offs)]})"
    assert st.get("count_segments", 0) == sum(64 <= sz <= KCOUNTMEDMAX for sz, _ in segs), st
    return offs


@pytest.mark.parametrize("end_bit", list(range(9, 17)))
def test_taken_and_rejected_alternate(ctx, end_bit):
    """Every second segment is one the kernel leaves alone: too long, a value with 256 copies, a crowded thread."""
    rej = [(CAP + 1, "u"), (16001, "c256"), (30011, "u"), (15003, "crowd"), (CAP + 601, "u"), (4001, "same")]
    segs = []
    for i in range(24):
        segs.append((16384 - 7 * i, "u"))          # taken (starts drift over 0-3 modulo 4)
        segs.append(rej[i % len(rej)])
    segs.append((9000, "u"))
    offs = run_segments(ctx, segs, end_bit, lead=5, trail=9, seed=1)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}


@pytest.mark.parametrize("start_mod", [0, 1, 2, 3])
@pytest.mark.parametrize("end_bit", [16, 12])
def test_counts_around_the_capacity(ctx, start_mod, end_bit):
    """start % 4 = start_mod; (start % 4) + count = 17405 .. 17408 (the last vectors of the grid, taken) and 17409 (one
    above the capacity, rejected), each between ordinary segments and with a one-element spacer to restore the start."""
    segs = []
    lead = 4 + start_mod
    for tot in (CAP - 3, CAP - 2, CAP - 1, CAP, CAP + 1, CAP, CAP - 3):
        cnt = tot - start_mod
        pad = (-cnt) % 4                               # spacers bring the next start back to start_mod modulo 4
        segs.append((cnt, "u"))
        segs.extend([(1, "u")] * pad)
        segs.append((16000, "u"))                      # (a multiple of 4)
    offs = run_segments(ctx, segs, end_bit, lead=lead, trail=3, seed=2 + start_mod)
    big = [offs[i] % 4 for i, (sz, _) in enumerate(segs) if sz > 16000]
    assert big == [start_mod] * len(big)


@pytest.mark.parametrize("end_bit", [16, 13, 9])
def test_byte_counter_limit(ctx, end_bit):
    """255 copies of one value fill a byte counter (taken when the thread's other counters are empty: the copies sit in
    the otherwise unused lower half of the values), 256 overflow it (rejected); either way the result is the sorted one."""
    segs = [(12000, "c255"), (12000, "c256"), (12001, "c255"), (12003, "c256"), (12000, "u"), (12002, "c256"), (12000, "c255")]
    run_segments(ctx, segs, end_bit, lead=0, trail=0, seed=3)


@pytest.mark.parametrize("short", [1, 2, 3])
@pytest.mark.parametrize("last", [CAP - 8, 16384, 100])
def test_last_segment_short_of_a_vector(ctx, short, last):
    """The array ends ``short`` elements behind a multiple of 4 and its last segment ends with it: that segment's last
    vector would reach behind the array, so the kernel must not take it (and must not read it early either)."""
    lead = 8
    body = [(16384, "u"), (16380, "u"), (16384, "u")]
    used = lead + sum(s for s, _ in body)
    fill = (short - (used + last)) % 4                  # (used + fill + last) % 4 == short
    segs = body + [(1, "u")] * fill + [(last, "u")]
    offs = run_segments(ctx, segs, 16, lead=lead, trail=0, seed=4 + short)
    assert offs[-1] % 4 == short


@pytest.mark.parametrize("nseg", ["one", "2cu+1"])
def test_one_and_a_grid_of_segments(ctx, nseg):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = 1 if nseg == "one" else 2 * cus + 1
    segs = [(16384 - (i % 5), "u") for i in range(m)]
    run_segments(ctx, segs, 16, lead=2, trail=1, seed=5)
    run_segments(ctx, segs, 11, lead=0, trail=0, seed=6)
