"""Guard-band tests: no entry point writes outside the buffers it was given.

Every buffer a call gets -- in-place arrays, outputs, read-only inputs -- is the payload of a ``guardband.Arena``: one
tensor ``[front guard | lead | payload | back guard]`` whose guards hold a pseudo-random pattern.  Every case compares
the RESULT with the plain reference of the operation (numpy: np.sort, np.bincount, np.cumsum, np.searchsorted; the CPU
oracle for the generators, the sample and the delimiters; tuples by the suite's rule: the sorted key sequence,
``k[rid] == key``, rids a permutation) and then checks the guards of EVERY buffer; a read-only input's content is
compared too.  Where a counter exists for the path a case is meant to take, ``ctx.stats()`` is asserted: a bounds test
that silently took another path proves nothing.

Guards are at least 64 KiB and at least twice the largest unit a workgroup of the path handles at once: the classify
tile, the leaf capacities (from ``msd_plan_first_round``), kRpCap = kL17Cap = 17408 elements, kGatherChunk = 2048, one
hist2 record (``msd_hist2_record_bytes``).  One case per family has guards as long as the payload: a block placed through
a wrong base lands far away, not next door.  ``lead_bytes`` 0 / 16 / 48 / 240 / 272 puts the payload on and off the
256-byte block grid; ``neighbours`` "low" / "high" (see guardband.Arena) alternate.

Entry point (include/msd_radix_hip.h, every one with a non-const device pointer) -> test:
  msd_sort_u32 / _u64 / _pairs_u64, msd_sort_*_bits ......... test_sort_default_options (the plain forms for full-width keys),
                                                              test_sort_paths_*, test_sort_option_*, test_sort_long_guards
  msd_sort_*_top ........................................... test_sort_top
  msd_partition_* .......................................... test_partition_pass
  msd_partition_by_splitters_* ............................. test_partition_by_splitters
  msd_sort_*_segments ...................................... test_segments_*
  msd_pack_low16_u32 ....................................... test_pack_low16
  msd_order_low16_u32, _counts_u32, _scatter_u32 ........... test_order_low16
  msd_gather_runs_u32 / _u64 ............................... test_gather_runs_alignments_u32 / _u64, test_gather_runs_mixed_and_long_guards
  msd_merge_buckets_u32 / _low16 ........................... test_merge_buckets, test_merge_buckets_rejected
  msd_hist2_pack_u32 / _low16, msd_merge_buckets_u32_hist2,
  msd_bounds_from_counts16 ................................. test_hist2_pack_and_merge, test_hist2_from_low_halves, test_hist2_overflow_flag
  msd_bucket_bounds_* ...................................... test_bucket_bounds
  msd_histogram_* .......................................... test_histogram
  msd_exclusive_scan_u64 ................................... test_exclusive_scan
  msd_sample_*, msd_splitters_* ............................ test_sample_and_splitters
  msd_gen_* ................................................ test_generators, test_generators_mt19937_64
  msd_topk_u32 / _u64 / _pairs_u64, msd_topk_keys .......... test_topk, test_topk_long_guards_and_large_k

Out of scope: the host-pointer reference API (sort() / check() on numpy arrays) and the entry points that return
through host pointers (msd_select_*, msd_check_*); the RCCL entry points of msd_sharded.hip; the library's own workspace
(not reachable from a test); reads outside a buffer (a read cannot be observed without provoking a fault, which is not
to be done).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guardband
from gpu_support import DEFAULTS   # the options' defaults; other GPU test files share the session's context
from guardband import Arena
from oracle import oracle as O
from sort_rows_expect import np_encode

pytestmark = pytest.mark.gpu

LEADS = [0, 16, 48, 240, 272]
NEIGH = ["low", "high"]
KRPCAP = 17408          # kRpCap (csrc/msd_regpart.hpp) = kL17Cap (csrc/msd_leaf17.hpp): no binding exposes them
KCOUNTMEDMAX = 1 << 17  # kCountMedMax (csrc/msd_device.hpp, MSD_COUNT_MED_LOG)
KGATHERCHUNK = 2048     # kGatherChunk (csrc/msd_device.hpp, MSD_GATHER_CHUNK)
KSCANTILE = 2048        # kScanTile (csrc/msd_device.hpp: 256 threads x 8 items)
TDT = {2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}
UDT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
KEYB = {"u32": 4, "u64": 8, "pairs": 8}


@pytest.fixture(autouse=True)
def default_options(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    yield
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


@functools.lru_cache(None)
def plan(typ):
    from inplacemsdradixsort_amd.api import plan_first_round
    return plan_first_round(1 << 20, KEYB[typ], 8 if typ == "pairs" else 0)


@functools.lru_cache(None)
def sort_guard(typ):
    """guard elements for the sorts of ``typ``: tile, LDS-leaf capacity, the register-resident leaves, the counting leaves"""
    p = plan(typ)
    return guardband.guard_elems(KEYB[typ], p["tile_elems"], p["leaf_capacity"], KRPCAP, p["block_elems"])


def call(ctx, name, *args):
    ctx._ok(getattr(ctx._L, name)(ctx._h, *args))


def arena_of(a, lead=0, neighbours="random", guard=None):
    a = np.ascontiguousarray(a)
    return Arena(TDT[a.itemsize], a.size, lead_bytes=lead, guard=guard, neighbours=neighbours).fill(a)


def unchanged(ar, a, what):
    """a read-only input: guards and content"""
    ar.check(what)
    assert (ar.host(UDT[ar.es]) == np.ascontiguousarray(a).view(UDT[ar.es])).all(), f"{what}: the input was modified"


# ------------------------------------------------------------------ A. in-place sorts

def make_keys(kind, n, bits, rng):
    """(keys, end_bit) of one distribution"""
    dt = np.uint32 if bits == 32 else np.uint64
    full = (1 << bits) - 1
    uni = lambda: rng.integers(0, full, n, dtype=np.uint64, endpoint=True).astype(dt)  # noqa: E731
    if kind == "uniform":
        return uni(), bits
    if kind == "const":
        return np.full(n, 0xDEADBEEFCAFEF00D & full, dt), bits
    if kind == "low16":      # <= 16 open bits under a constant prefix: the counting leaves
        return (rng.integers(0, 1 << 16, n, dtype=np.uint64) | np.uint64((0xABCD1234 << (bits - 32)) & full & ~0xFFFF)).astype(dt), bits
    if kind == "low12":      # <= 12 open bits: the LDS leaf counts them all, its plain write-back (no groups to put in order)
        return (rng.integers(0, 1 << 12, n, dtype=np.uint64) | np.uint64((0xABCD1234 << (bits - 32)) & full & ~0xFFF)).astype(dt), bits
    if kind == "heavy":      # one value on 40 % of the keys, noise around it
        k = uni()
        k[rng.random(n) < 0.4] = dt(0x5A5A5A5A5A5A5A5A & full)
        return k, bits
    if kind == "sorted":
        return np.sort(uni()), bits
    if kind == "endbit":     # end_bit below the key width, the bits above it constant
        eb = 20 if bits == 32 else 58
        return ((uni() & dt((1 << eb) - 1)) | dt((0xABC << (bits - 12)) & full & ~((1 << eb) - 1))), eb
    raise ValueError(kind)


DISTS = ["uniform", "const", "low16", "heavy", "sorted", "endbit", "low12"]
SMALL_ROLES = ["1", "2", "3", "5", "B-1", "B", "B+1", "T-1", "T", "T+1", "leaf-1", "leaf", "leaf+1"]
RP_ROLES = ["rp-1", "rp", "rp+1"]
BIG_ROLES = ["2^20+3", "2^20+5", "2^20+7", "2^22+3", "2^22+5", "2^22+7"]


def role_n(typ, role):
    p = plan(typ)
    if role[0].isdigit():                            # "5", "2^20+3"
        head, _, add = role.partition("+")
        b, _, e = head.partition("^")
        return (int(b) ** int(e) if e else int(b)) + (int(add) if add else 0)
    base = {"B": p["block_elems"], "T": p["tile_elems"], "leaf": p["leaf_capacity"], "rp": KRPCAP, "med": KCOUNTMEDMAX}
    for name, v in base.items():
        if role == name:
            return v
        if role.startswith(name) and role[len(name)] in "+-":
            return v + int(role[len(name):])
    raise ValueError(role)


def default_cases():
    """Every size role once with a lead, a distribution and a neighbour mode in rotation; the cheap sizes (up to the leaves'
    capacities, every threshold with its +-1) additionally with every lead and every distribution."""
    out = []
    for typ in ("u32", "u64", "pairs"):
        small = SMALL_ROLES + (RP_ROLES if typ != "u32" else [])
        roles = small + BIG_ROLES
        cases = [(role, LEADS[i % 5], DISTS[i % 7], NEIGH[i % 2]) for i, role in enumerate(roles)]
        for role in small:
            cases += [(role, lead, "uniform", "low") for lead in LEADS]
            cases += [(role, 48, d, "high") for d in DISTS]
        seen = set()
        for cse in cases:
            if cse not in seen:
                seen.add(cse)
                out.append(pytest.param(typ, *cse, id=f"{typ}-{cse[0]}-lead{cse[1]}-{cse[2]}-{cse[3]}"))
    return out


def run_sort(ctx, typ, k, end_bit, lead=0, neighbours="random", guard=None, what="", rid_lead=None):
    """Sorts k (and positions as rids for tuples) in arenas; checks guards, then the result; returns ctx.stats()."""
    n, bits = k.size, 8 * KEYB[typ]
    g = sort_guard(typ) if guard is None else guard
    ka = arena_of(k, lead, neighbours, g)
    if typ == "pairs":
        ra = arena_of(np.arange(n, dtype=np.uint64), lead if rid_lead is None else rid_lead, neighbours, g)
        if end_bit == bits:
            call(ctx, "msd_sort_pairs_u64", ka.ptr, ra.ptr, n)
        else:
            call(ctx, "msd_sort_pairs_u64_bits", ka.ptr, ra.ptr, n, end_bit)
    elif end_bit == bits:
        call(ctx, "msd_sort_u32" if typ == "u32" else "msd_sort_u64", ka.ptr, n)
    else:
        call(ctx, "msd_sort_u32_bits" if typ == "u32" else "msd_sort_u64_bits", ka.ptr, n, end_bit)
    st = ctx.stats()
    ka.check(f"{what} keys")
    out = ka.host(k.dtype)
    assert (out == np.sort(k)).all(), f"{what}: not the sorted keys"
    if typ == "pairs":
        ra.check(f"{what} rids")
        rid = ra.host(np.uint64)
        assert (np.sort(rid) == np.arange(n, dtype=np.uint64)).all(), f"{what}: the rids are no permutation"
        assert (k[rid.astype(np.int64)] == out).all(), f"{what}: a rid left its key"
    return st


@pytest.mark.parametrize("typ,role,lead,dist,neighbours", default_cases())
def test_sort_default_options(ctx, typ, role, lead, dist, neighbours):
    n = role_n(typ, role)
    rng = np.random.default_rng(n * 7 + lead + len(dist))
    k, end_bit = make_keys(dist, n, 8 * KEYB[typ], rng)
    st = run_sort(ctx, typ, k, end_bit, lead, neighbours, what=f"{typ} n={n} lead={lead} {dist}", rid_lead=LEADS[(LEADS.index(lead) + 2) % 5])
    small_max = plan(typ)["leaf_capacity"]
    if n <= small_max and n > 1 and dist != "const":
        assert st.get("small_segments", 0) == 1 and st.get("rounds", 0) == 0, st        # one LDS leaf, no round
    if typ == "u32" and dist in ("low16", "low12") and n > small_max:
        assert st.get("big_count_segments", 0) == 1 and st.get("rounds", 0) == 0, st    # the multi-workgroup counting sort
    if dist == "uniform" and n > (1 << 20):
        assert st.get("rounds", 0) >= 1, st


@pytest.mark.parametrize("role,lead", [("leaf+1", 16), ("med-1", 48), ("med", 240), ("med+1", 272), ("2^21+3", 0)])
def test_sort_paths_u32_whole_input_counting_sort(ctx, role, lead):
    """u32 keys with <= 16 open bits above the LDS leaf's capacity: one `big` counting segment, whatever the size."""
    n = role_n("u32", role)
    rng = np.random.default_rng(n)
    for kind in ("low16", "twelve"):
        k = make_keys("low16", n, 32, rng)[0] if kind == "low16" else rng.integers(0, 1 << 12, n, dtype=np.uint32)
        st = run_sort(ctx, "u32", k, 32, lead, "low", what=f"{kind} n={n}")
        assert st.get("big_count_segments", 0) == 1, st


@pytest.mark.parametrize("lead,neighbours", [(0, "low"), (272, "high")])
def test_sort_paths_u32_counting_leaves_around_kcountmedmax(ctx, lead, neighbours):
    """24 open bits: one 8-bit round, children with 16 open bits.  Three children have kCountMedMax - 1, kCountMedMax and
    kCountMedMax + 1 keys (the last one is a `big` segment, the others take the single-workgroup counting leaves), the rest
    is spread evenly."""
    rng = np.random.default_rng(lead + 1)
    n = (1 << 21) + 7
    sizes = {3: KCOUNTMEDMAX - 1, 100: KCOUNTMEDMAX, 200: KCOUNTMEDMAX + 1}
    rest = n - sum(sizes.values())
    others = np.array([d for d in range(256) if d not in sizes], dtype=np.uint32)
    top = np.concatenate([np.full(c, d, np.uint32) for d, c in sizes.items()] + [others[rng.integers(0, len(others), rest)]])
    k = (rng.permutation(top) << np.uint32(16)) | rng.integers(0, 1 << 16, n, dtype=np.uint32)
    st = run_sort(ctx, "u32", k, 24, lead, neighbours, what="children around kCountMedMax")
    assert st.get("rounds", 0) == 1 and st.get("count_segments", 0) >= 250 and st.get("big_count_segments", 0) == 1, st


@pytest.mark.parametrize("mid_leaf,hot_share,lead", [(1, 0.3, 16), (0, 0.3, 48), (1, 0.9, 240)])
def test_sort_option_mid_leaf_and_escalation(ctx, mid_leaf, hot_share, lead):
    """A child of about 100 K keys whose hot value overflows the byte counters of the register-resident counting leaves:
    the 16-bit-counter leaf finishes it, or (switched off, or the value has more copies than 16 bits count) it escalates
    to the multi-workgroup counting sort.  The input of test_counting_leaf_overflow_escalates."""
    rng = np.random.default_rng(42)
    n = (1 << 22) + 5
    k = rng.integers(0, 1 << 21, n, dtype=np.uint32)
    hot = rng.random(n) < 0.025
    k[hot] = (np.uint32(0x55) << np.uint32(13)) | rng.integers(0, 1 << 13, int(hot.sum()), dtype=np.uint32)
    hotter = hot & (rng.random(n) < hot_share)
    k[hotter] = (np.uint32(0x55) << np.uint32(13)) | np.uint32(77)
    ctx.set_option("mid_leaf", mid_leaf)
    try:
        st = run_sort(ctx, "u32", k, 32, lead, "low", what=f"mid_leaf={mid_leaf} hot={hot_share}")
    finally:
        ctx.set_option("mid_leaf", DEFAULTS["mid_leaf"])
    assert st.get("count_segments", 0) >= 1, st
    if mid_leaf == 0 or hot_share > 0.8:
        assert st.get("big_count_segments", 0) >= 1, st
    else:
        assert st.get("big_count_segments", 0) == 0, st


@pytest.mark.parametrize("count16", [0, 1, 2])
@pytest.mark.parametrize("role,lead", [("2^20+3", 16), ("2^22+5", 272)])
def test_sort_option_count16(ctx, count16, role, lead):
    """u32 keys with 24 varying bits: one 8-bit round leaves children of 2^12 / 2^14 keys with 16 open bits.  They go through
    count_place_kernel alone (0), through count_place16_kernel at 2^14 keys per segment (1) or at any size (2)."""
    n = role_n("u32", role)
    k = O.gen_uniform_u32(n, seed=41 + n) & np.uint32(0x00FFFFFF)
    ctx.set_option("count16", count16)
    try:
        st = run_sort(ctx, "u32", k, 32, lead, NEIGH[count16 % 2], what=f"count16={count16} n={n}")
    finally:
        ctx.set_option("count16", DEFAULTS["count16"])
    assert st.get("rounds", 0) == 1 and st.get("count_segments", 0) >= 250 and st.get("skipped_bits", 0) == 8, st


@pytest.mark.parametrize("typ,lead", [("u32", 16), ("u32", 240), ("u64", 48), ("pairs", 272)])
def test_sort_option_direct_placement_forced(ctx, typ, lead):
    """direct_mode 2 with the thresholds of tests/test_gpu_direct.py: a direct-placement round runs at 2^22 elements."""
    n = (1 << 22) + 5
    rng = np.random.default_rng(lead)
    k = make_keys("uniform", n, 8 * KEYB[typ], rng)[0]
    ctx.set_option("direct_mode", 2)
    ctx.set_option("direct_min", 1 << 16)
    ctx.set_option("direct_min_parent", 1 << 12)
    try:
        st = run_sort(ctx, typ, k, 8 * KEYB[typ], lead, "high", what=f"direct {typ}")
    finally:
        for name in ("direct_mode", "direct_min", "direct_min_parent"):
            ctx.set_option(name, DEFAULTS[name])
    assert st.get("direct_rounds", 0) >= 1, st


def test_sort_option_direct_off(ctx):
    n = (1 << 22) + 3
    k = O.gen_uniform_u32(n, seed=6)
    ctx.set_option("direct_mode", 0)
    try:
        st = run_sort(ctx, "u32", k, 32, 48, "low", what="direct_mode=0")
    finally:
        ctx.set_option("direct_mode", DEFAULTS["direct_mode"])
    assert st.get("direct_rounds", 0) == 0 and st.get("rounds", 0) >= 1, st


def test_sort_paths_u32_default_direct_round(ctx):
    """the default options place the first round of 2^22 evenly spread keys directly"""
    st = run_sort(ctx, "u32", O.gen_uniform_u32((1 << 22) + 7, seed=8), 32, 240, "high", what="default direct")
    assert st.get("direct_rounds", 0) >= 1, st


@pytest.mark.parametrize("outlier", [False, True])
def test_sort_paths_sampled_bit_skip_and_restart(ctx, outlier):
    """2^24 + 7 u32 keys with 8 constant leading bits: the skip is decided on a sample and checked exactly later; one
    key that differs in a skipped bit makes the sort start over (test_sampled_bit_skip_is_verified)."""
    n = (1 << 24) + 7
    k = O.gen_uniform_u32(n, seed=n) & np.uint32(0x00FFFFFF)
    if outlier:
        k[12345] |= np.uint32(1 << 29)
    ctx.set_option("direct_min", 1 << 20)
    try:
        st = run_sort(ctx, "u32", k, 32, 272 if outlier else 16, "low", what=f"bit skip outlier={outlier}")
    finally:
        ctx.set_option("direct_min", DEFAULTS["direct_min"])
    assert st.get("direct_rounds", 0) >= 1, st
    if outlier:
        assert st.get("bit_skip_restarts", 0) == 1 and st.get("skipped_bits", 0) == 2, st
    else:
        assert st.get("bit_skip_restarts", 0) == 0 and st.get("skipped_bits", 0) == 8, st


@pytest.mark.parametrize("typ", ["u64", "pairs"])
@pytest.mark.parametrize("regpart,leaf17,lead", [(1, 1, 16), (0, 1, 48), (1, 0, 272)])
def test_sort_option_regpart_and_leaf17(ctx, typ, regpart, leaf17, lead):
    """4 000 001 elements: the first round leaves 256 parents of about 15.6 Ki elements, which fit the register-resident
    kernels (kRpCap = kL17Cap = 17408): leaf17_kernel, the register partition, or (regpart 0) a general round."""
    n = 4_000_001
    k = O.gen_uniform_u64(n, seed=51 + lead)
    ctx.set_option("regpart", regpart)
    ctx.set_option("leaf17", leaf17)
    try:
        st = run_sort(ctx, typ, k, 64, lead, NEIGH[regpart], what=f"{typ} regpart={regpart} leaf17={leaf17}")
    finally:
        ctx.set_option("regpart", DEFAULTS["regpart"])
        ctx.set_option("leaf17", DEFAULTS["leaf17"])
    if typ == "pairs":
        if regpart == 0:
            assert st.get("regpart_rounds", 0) == 0 and st.get("leaf17_segments", 0) == 0, st
        elif leaf17:
            assert st.get("leaf17_segments", 0) >= 1 and st.get("regpart_rounds", 0) == 0, st
        else:
            assert st.get("regpart_rounds", 0) >= 1 and st.get("leaf17_segments", 0) == 0, st
    else:
        assert st.get("leaf17_launches", 0) == (1 if leaf17 else 0), st
        if regpart == 0:
            assert st.get("regpart_rounds", 0) == 0, st


def test_sort_paths_leaf17_rejects(ctx):
    """Tuples: duplicates inside the segments and one top-byte bucket whose counted bits take only 8 values (groups longer
    than the fix-up follows): leaf17_kernel rejects it, the register partition and the small leaves finish it.  The input
    of test_leaf17_duplicates_and_rejected_segments."""
    rng = np.random.default_rng(77)
    n = 4_000_001
    k = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    k[5::5] = k[4::5][: k[5::5].size]
    sel = (k >> np.uint64(56)) == np.uint64(9)
    c = (k[sel] >> np.uint64(20)) & np.uint64(7)
    k[sel] = (np.uint64(9) << np.uint64(56)) | ((c * np.uint64(0x1249)) & np.uint64(0x1FFF)) << np.uint64(7) | (k[sel] & np.uint64(127))
    st = run_sort(ctx, "pairs", k, 64, 240, "low", what="leaf17 rejects", rid_lead=16)
    assert st.get("leaf17_segments", 0) >= 1 and st.get("leaf17_rejected", 0) >= 1, st


@pytest.mark.parametrize("typ", ["u32", "u64", "pairs"])
def test_sort_long_guards(ctx, typ):
    """guards as long as the payload (2^22 + 3 elements at most: u32; 2^21 + 3 for the 8-byte types)"""
    n = ((1 << 22) if typ == "u32" else (1 << 21)) + 3
    k = make_keys("uniform", n, 8 * KEYB[typ], np.random.default_rng(n))[0]
    st = run_sort(ctx, typ, k, 8 * KEYB[typ], 48, "low", guard=n, what=f"{typ} long guards")
    assert st.get("rounds", 0) >= 1, st


@pytest.mark.parametrize("typ,begin_bit", [("u32", 16), ("u32", 8), ("u64", 40), ("pairs", 48)])
@pytest.mark.parametrize("role,lead", [("5", 16), ("leaf+1", 48), ("2^20+5", 240), ("2^22+3", 272)])
def test_sort_top(ctx, typ, begin_bit, role, lead):
    """msd_sort_*_top: ordered by key >> begin_bit, the same multiset, rids with their keys"""
    n, bits = role_n(typ, role), 8 * KEYB[typ]
    k = make_keys("uniform", n, bits, np.random.default_rng(n + begin_bit))[0]
    ka = arena_of(k, lead, "high", sort_guard(typ))
    if typ == "pairs":
        r = k ^ np.uint64(0x1234)
        ra = arena_of(r, lead, "high", sort_guard(typ))
        call(ctx, "msd_sort_pairs_u64_top", ka.ptr, ra.ptr, n, bits, begin_bit)
    else:
        call(ctx, f"msd_sort_{typ}_top", ka.ptr, n, bits, begin_bit)
    ka.check("top keys")
    out = ka.host(k.dtype)
    top = (out.astype(np.uint64) >> np.uint64(begin_bit))
    assert (top[1:] >= top[:-1]).all() and (np.sort(out) == np.sort(k)).all()
    if typ == "pairs":
        ra.check("top rids")
        assert (ra.host(np.uint64) == (out ^ np.uint64(0x1234))).all()


@pytest.mark.parametrize("typ,shift,rb", [("u32", 24, 8), ("u32", 0, 8), ("u32", 27, 5), ("u32", 16, 3), ("u32", 31, 1), ("u64", 56, 8), ("u64", 13, 7), ("pairs", 56, 8), ("pairs", 40, 4)])
@pytest.mark.parametrize("role,lead,with_count", [("5", 16, True), ("B+1", 48, True), ("T+1", 240, True), ("leaf+1", 272, False), ("2^20+7", 16, True), ("2^22+3", 272, True)])
def test_partition_pass(ctx, typ, shift, rb, role, lead, with_count):
    """One in-place digit pass: digits ascending, the same multiset per bucket, bucket sizes = np.bincount in an arena of
    exactly 2^radix_bits counters (or no counter array at all)."""
    n, bits = role_n(typ, role), 8 * KEYB[typ]
    k = make_keys("uniform", n, bits, np.random.default_rng(n + shift))[0]
    ka = arena_of(k, lead, "low", sort_guard(typ))
    ca = Arena(torch.int64, 1 << rb, lead_bytes=LEADS[rb % 5], neighbours="high") if with_count else None
    cp = ca.ptr if ca else None
    if typ == "pairs":
        ra = arena_of(np.arange(n, dtype=np.uint64), lead, "low", sort_guard(typ))
        call(ctx, "msd_partition_pairs_u64", ka.ptr, ra.ptr, n, shift, rb, cp)
    else:
        call(ctx, f"msd_partition_{typ}", ka.ptr, n, shift, rb, cp)
    ka.check("partition keys")
    out = ka.host(k.dtype)
    dig = lambda a: ((a.astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << rb) - 1)).astype(np.int64)  # noqa: E731
    want = np.bincount(dig(k), minlength=1 << rb)
    if ca:
        ca.check("partition counts")
        assert (ca.host(np.uint64) == want.astype(np.uint64)).all()
    d = dig(out)
    assert (np.diff(d) >= 0).all(), "digits not ascending"
    order = np.argsort(dig(k), kind="stable")
    start = 0
    for c in want.tolist():      # bucket by bucket: the same multiset
        assert (np.sort(out[start:start + c]) == np.sort(k[order[start:start + c]])).all()
        start += c
    if typ == "pairs":
        ra.check("partition rids")
        rid = ra.host(np.uint64).astype(np.int64)
        assert (np.sort(rid) == np.arange(n)).all() and (k[rid] == out).all()


@pytest.mark.parametrize("typ", ["u32", "u64", "pairs"])
@pytest.mark.parametrize("parts", [1, 2, 8, 256])
@pytest.mark.parametrize("role,lead", [("5", 16), ("leaf+1", 48), ("2^20+3", 240), ("2^21+5", 272)])
def test_partition_by_splitters(ctx, typ, parts, role, lead):
    """Range p = keys in (delim[p-1], delim[p]]: np.searchsorted(delims, key, "left"); ranges contiguous and ascending,
    sizes in an arena of exactly `parts` counters, the delimiters unchanged."""
    n, bits = role_n(typ, role), 8 * KEYB[typ]
    rng = np.random.default_rng(n + parts)
    k = make_keys("uniform", n, bits, rng)[0]
    d = np.sort(rng.integers(0, (1 << bits) - 1, parts - 1, dtype=np.uint64, endpoint=True).astype(k.dtype))
    if parts > 2:
        d[1] = d[0]              # a duplicate delimiter: an empty range
    ka = arena_of(k, lead, "high", sort_guard(typ))
    da = arena_of(d, LEADS[parts % 5]) if parts > 1 else None
    ca = Arena(torch.int64, parts, lead_bytes=LEADS[(parts + 1) % 5], neighbours="low")
    dp = da.ptr if da else None
    if typ == "pairs":
        ra = arena_of(np.arange(n, dtype=np.uint64), lead, "high", sort_guard(typ))
        call(ctx, "msd_partition_by_splitters_pairs_u64", ka.ptr, ra.ptr, n, dp, parts, ca.ptr)
    else:
        call(ctx, f"msd_partition_by_splitters_{typ}", ka.ptr, n, dp, parts, ca.ptr)
    ka.check("splitter keys")
    ca.check("splitter counts")
    if da:
        unchanged(da, d, "delimiters")
    rng_of = lambda a: np.searchsorted(d, a, side="left")  # noqa: E731
    want = np.bincount(rng_of(k), minlength=parts)
    assert (ca.host(np.uint64) == want.astype(np.uint64)).all()
    out = ka.host(k.dtype)
    ro = rng_of(out)
    assert (np.diff(ro) >= 0).all(), "ranges not ascending"
    order = np.argsort(rng_of(k), kind="stable")
    assert (np.sort(out) == np.sort(k)).all()
    start = 0
    for c in want.tolist():
        assert (np.sort(out[start:start + c]) == np.sort(k[order[start:start + c]])).all()
        start += c
    if typ == "pairs":
        ra.check("splitter rids")
        rid = ra.host(np.uint64).astype(np.int64)
        assert (np.sort(rid) == np.arange(n)).all() and (k[rid] == out).all()


# ------------------------------------------------------------------ B. segmented sort

@pytest.mark.parametrize("lead,neighbours", [(16, "low"), (272, "high")])
@pytest.mark.parametrize("end_bit", [16, 24])
def test_segments_u32_every_list(ctx, end_bit, lead, neighbours):
    """msd_sort_u32_segments.  All segments of a call share end_bit, so route_to_leaves fills l_small + l_count + l_big
    with 16 open bits (sizes below 64, 64 .. kCountMedMax, above it) and l_small + parents with 24 (up to the LDS leaf's
    capacity, above it): the two settings together fill every list.  The offsets ascend and touch (segment i =
    [seg_off[i], seg_off[i + 1])), so a gap BETWEEN two segments is a one-element segment (never moved) or an empty one;
    the gaps in front of the first and behind the last segment (7 and 11 elements; the offsets are odd and even, on and off multiples of 4)
    belong to no segment.  All of them hold random values and must stay as they are."""
    rng = np.random.default_rng(end_bit + lead)
    S = plan("u32")["leaf_capacity"]
    sizes = [5, 1, 0, 63, 1, 64, 1, 1, S - 1, 1, S, S + 1, 3, 1, KCOUNTMEDMAX - 1, 0, KCOUNTMEDMAX, 1, KCOUNTMEDMAX + 1, 2, 1, 300_001, 65, 1]
    offs = [7]
    for sz in sizes:
        offs.append(offs[-1] + sz)
    total = offs[-1] + 11
    k = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)          # the gaps: anything
    want = k.copy()
    for i, sz in enumerate(sizes):                                                  # a segment's keys agree above end_bit
        a, b = offs[i], offs[i + 1]
        if sz > 1:
            k[a:b] = rng.integers(0, 1 << end_bit, sz, dtype=np.uint32) | np.uint32(((i * 37 + 1) % 200) << end_bit)
            want[a:b] = np.sort(k[a:b])
    assert any(o % 4 == 3 for o in offs) and any(o % 4 == 1 for o in offs)
    ka = arena_of(k, lead, neighbours, sort_guard("u32"))
    call(ctx, "msd_sort_u32_segments", ka.ptr, total, ctx._u64arr(offs), len(sizes), end_bit)
    st = ctx.stats()
    ka.check("segments u32")
    out = ka.host(np.uint32)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"differs at {bad[:8]} (offsets {offs})"
    if end_bit == 16:
        assert st.get("count_segments", 0) == sum(64 <= sz <= KCOUNTMEDMAX for sz in sizes), st
        assert st.get("big_count_segments", 0) == sum(sz > KCOUNTMEDMAX for sz in sizes), st
        assert st.get("small_segments", 0) >= sum(2 <= sz < 64 for sz in sizes) and st.get("rounds", 0) == 0, st
    else:
        assert st.get("rounds", 0) >= 1 and st.get("small_segments", 0) >= sum(2 <= sz <= S for sz in sizes), st


@pytest.mark.parametrize("lead,neighbours", [(48, "low"), (240, "high")])
def test_segments_u32_unlisted_gaps(ctx, lead, neighbours):
    """Gaps that belong to NO segment: seg_off[0] > 0, seg_off[nseg] < n, and between two listed segments lies a third,
    empty by its offsets' order -- the random keys in front, behind and inside stay where they are."""
    rng = np.random.default_rng(lead)
    n = 500_011
    k = rng.integers(0, 1 << 20, n, dtype=np.uint32)
    offs = [1001, 200_003, 200_003, 449_999]               # [0, 1001) and [449999, n) belong to no segment
    ka = arena_of(k, lead, neighbours, guard=n)             # (this family's case with guards as long as the payload)
    call(ctx, "msd_sort_u32_segments", ka.ptr, n, ctx._u64arr(offs), 3, 20)
    ka.check("segments with unlisted gaps")
    out = ka.host(np.uint32)
    assert (out[:1001] == k[:1001]).all() and (out[449_999:] == k[449_999:]).all()
    assert (out[1001:200_003] == np.sort(k[1001:200_003])).all() and (out[200_003:449_999] == np.sort(k[200_003:449_999])).all()


@pytest.mark.parametrize("typ", ["u64", "pairs"])
@pytest.mark.parametrize("lead,neighbours", [(16, "low"), (272, "high")])
def test_segments_u64_and_tuples(ctx, typ, lead, neighbours):
    """msd_sort_u64_segments / msd_sort_pairs_u64_segments: small segments, segments the register-resident kernels take
    (above the LDS leaf's capacity, up to kRpCap), parents; odd offsets; the first and last elements belong to no segment."""
    rng = np.random.default_rng(lead + len(typ))
    S = plan(typ)["leaf_capacity"]
    sizes = [5, 0, 1, S - 1, S, S + 1, 3, KRPCAP - 1, KRPCAP, KRPCAP + 1, 0, 2, 300_001] + [KRPCAP - 7 * i for i in range(1, 70)]
    offs = [7]
    for s in sizes:
        offs.append(offs[-1] + s)
    n = offs[-1] + 13
    end_bit = 56
    k = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    for i in range(len(sizes)):
        a, b = offs[i], offs[i + 1]
        k[a:b] = (k[a:b] & np.uint64((1 << 56) - 1)) | (np.uint64((7 * i + 1) % 256) << np.uint64(56))
    ka = arena_of(k, lead, neighbours, sort_guard(typ))
    if typ == "pairs":
        ra = arena_of(np.arange(n, dtype=np.uint64), lead, neighbours, sort_guard(typ))
        call(ctx, "msd_sort_pairs_u64_segments", ka.ptr, ra.ptr, n, ctx._u64arr(offs), len(sizes), end_bit)
    else:
        call(ctx, "msd_sort_u64_segments", ka.ptr, n, ctx._u64arr(offs), len(sizes), end_bit)
    st = ctx.stats()
    ka.check(f"segments {typ} keys")
    out = ka.host(np.uint64)
    want = k.copy()
    for i in range(len(sizes)):
        want[offs[i]:offs[i + 1]] = np.sort(k[offs[i]:offs[i + 1]])
    assert (out == want).all()
    if typ == "pairs":
        ra.check("segments rids")
        rid = ra.host(np.uint64).astype(np.int64)
        assert (np.sort(rid) == np.arange(n)).all() and (k[rid] == out).all()
        assert (rid[:7] == np.arange(7)).all() and (rid[offs[-1]:] == np.arange(offs[-1], n)).all()
        assert st.get("leaf17_segments", 0) + st.get("regpart_rounds", 0) >= 1, st
    assert st.get("rounds", 0) >= 1 and st.get("small_segments", 0) >= 3, st


# ------------------------------------------------------------------ C. out-of-place writers of the exchange path

@pytest.mark.parametrize("base", [0, 64, (1 << 20) + 8])
@pytest.mark.parametrize("r", range(8))
def test_pack_low16(ctx, base, r):
    """n >> 3 vectors + n & 7 scalars: every n mod 8, output arena of exactly n uint16"""
    n = base + r
    k = O.gen_uniform_u32(n, seed=n + 1) if n else np.zeros(0, np.uint32)
    ka = arena_of(k, LEADS[r % 5])
    oa = Arena(torch.int16, n, lead_bytes=LEADS[(r + 2) % 5], neighbours=NEIGH[r % 2])
    call(ctx, "msd_pack_low16_u32", ka.ptr, n, oa.ptr)
    oa.check(f"pack_low16 n={n}")
    unchanged(ka, k, "pack_low16 keys")
    assert (oa.host(np.uint16) == (k & np.uint32(0xFFFF)).astype(np.uint16)).all()


def _order_keys(kind, n, rng):
    if kind == "uniform":
        return O.gen_uniform_u32(n, seed=n)
    if kind == "narrow":         # a few top bytes occupied: empty parents
        return rng.integers(0, 1 << 26, n, dtype=np.uint32)
    return O.gen_zipf_u32(n, seed=5)  # skewed: one bucket holds a quarter of the keys


@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("kind", ["uniform", "narrow", "skewed"])
@pytest.mark.parametrize("n,lead", [(5, 16), (70_001, 48), ((1 << 20) + 3, 240), ((1 << 22) + 5, 272)])
def test_order_low16(ctx, n, lead, kind, halves):
    """msd_order_low16_u32 and its two halves: d_out (n uint16) and d_counts (65536 uint64) in arenas; n never a multiple
    of 4; the keys are only reordered, by their top 8 bits."""
    rng = np.random.default_rng(n)
    k = _order_keys(kind, n, rng)
    ka = arena_of(k, lead, "low", sort_guard("u32"))
    oa = Arena(torch.int16, n, lead_bytes=LEADS[(LEADS.index(lead) + 1) % 5], neighbours="high", guard=sort_guard("u32") * 2)
    ca = Arena(torch.int64, 65536, lead_bytes=lead, neighbours="low")
    if halves:
        call(ctx, "msd_order_low16_counts_u32", ka.ptr, n, ca.ptr)
        call(ctx, "msd_order_low16_scatter_u32", ka.ptr, n, oa.ptr)
    else:
        call(ctx, "msd_order_low16_u32", ka.ptr, n, oa.ptr, ca.ptr)
    for a, w in ((ka, "keys"), (oa, "low halves"), (ca, "counts")):
        a.check(f"order_low16 {w}")
    want = np.bincount(k >> np.uint32(16), minlength=65536)
    assert (ca.host(np.uint64) == want.astype(np.uint64)).all()
    got = oa.host(np.uint16)             # bucket after bucket (bucket = upper half), in any order inside a bucket
    rebuilt = (np.repeat(np.arange(65536, dtype=np.uint32), want) << np.uint32(16)) | got.astype(np.uint32)
    ks = np.sort(k)
    assert (np.sort(rebuilt) == ks).all(), "bucket b does not hold exactly the low halves of bucket b's keys"
    out = ka.host(np.uint32)
    assert (np.sort(out) == ks).all() and (np.diff((out >> np.uint32(24)).astype(np.int64)) >= 0).all()


GATHER_LENS = [0, 1, 3, 4, 5, KGATHERCHUNK - 1, KGATHERCHUNK, KGATHERCHUNK + 1, 3 * KGATHERCHUNK + 5, 7 * KGATHERCHUNK + 1023, 2, 9]


def _gather_case(ctx, dt, lens, dmis, smis, lead, rng, guard=None, shuffle=True):
    """Runs with the given destination / source misalignment (in elements against the 16-byte grid: callable run -> value),
    gaps between them in the destination, the last run flush with its end; the whole destination is compared (gaps keep their random fill), the source is
    unchanged."""
    vec = 16 // np.dtype(dt).itemsize
    src_off, dst_off, sa, da = [], [], 0, 0
    for i, ln in enumerate(lens):
        sa += (smis(i) - sa) % vec + vec * int(rng.integers(0, 3))
        da += (dmis(i) - da) % vec + vec * int(rng.integers(1, 4))
        src_off.append(sa)
        dst_off.append(da)
        sa += ln
        da += ln
    ns, nd = sa + 5, da          # the last run ends where the destination ends: the cell behind it is the back guard
    src = rng.integers(0, 1 << 63, ns, dtype=np.uint64).astype(dt)
    fill = rng.integers(0, 1 << 63, nd, dtype=np.uint64).astype(dt)
    order = rng.permutation(len(lens)) if shuffle else np.arange(len(lens))
    g = guardband.guard_elems(np.dtype(dt).itemsize, KGATHERCHUNK) if guard is None else guard
    s_ar = arena_of(src, lead, guard=g)
    d_ar = arena_of(fill, LEADS[(LEADS.index(lead) + 3) % 5], "low", guard=g)
    call(ctx, "msd_gather_runs_u32" if dt == np.uint32 else "msd_gather_runs_u64", d_ar.ptr, s_ar.ptr,
         ctx._u64arr([src_off[i] for i in order]), ctx._u64arr([dst_off[i] for i in order]), ctx._u64arr([lens[i] for i in order]), len(lens))
    d_ar.check(f"gather_runs dst (dst mis {dmis(0)}, src mis {smis(0)})")
    unchanged(s_ar, src, "gather_runs src")
    want = fill.copy()
    for so, do, ln in zip(src_off, dst_off, lens):
        want[do:do + ln] = src[so:so + ln]
    got = d_ar.host(dt)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"destination differs at {bad[:8]} (run starts {dst_off}, lengths {lens})"


@pytest.mark.parametrize("smis", range(4))
@pytest.mark.parametrize("dmis", range(4))
def test_gather_runs_alignments_u32(ctx, dmis, smis):
    rng = np.random.default_rng(dmis * 4 + smis)
    _gather_case(ctx, np.uint32, GATHER_LENS, lambda i: dmis, lambda i: smis, LEADS[(dmis + smis) % 5], rng)


@pytest.mark.parametrize("smis", range(2))
@pytest.mark.parametrize("dmis", range(2))
def test_gather_runs_alignments_u64(ctx, dmis, smis):
    rng = np.random.default_rng(100 + dmis * 2 + smis)
    _gather_case(ctx, np.uint64, GATHER_LENS, lambda i: dmis, lambda i: smis, LEADS[(dmis + 2 * smis) % 5], rng)


@pytest.mark.parametrize("dt", [np.uint32, np.uint64])
def test_gather_runs_mixed_and_long_guards(ctx, dt):
    """every run with its own misalignment, one long run; guards as long as the destination"""
    rng = np.random.default_rng(7)
    lens = GATHER_LENS + [300_001] + [int(x) for x in rng.integers(0, 5000, 40)]
    vec = 16 // np.dtype(dt).itemsize
    _gather_case(ctx, dt, lens, lambda i: (i * 3 + 1) % vec, lambda i: (i * 5 + 2) % vec, 48, rng, guard=sum(lens) + 4096)


def _arrivals(rng, nsrc, nb, first, open_bits, per_bucket, edit=None):
    """What a rank holds after a fine-grained exchange: per source its buckets first .. first + nb - 1 in order (unsorted
    inside a bucket), a few junk elements in front of every source and behind the last: (src, counts, base, all keys)."""
    counts = np.zeros((nsrc, nb), dtype=np.int64)
    parts, rows, base, at = [], [], [], 0
    for x in range(nsrc):
        c = rng.poisson(per_bucket / nsrc, nb).astype(np.int64)
        c[nb // 2] = 0                                                    # an empty bucket in the middle
        if edit is not None:
            c = edit(x, c)
        counts[x] = c
        pre = np.repeat(np.arange(first, first + nb, dtype=np.uint64), c)
        keys = ((pre << np.uint64(open_bits)) | rng.integers(0, 1 << open_bits, int(c.sum()), dtype=np.uint64)).astype(np.uint32)
        gap = int(rng.integers(0, 7))
        parts.append(rng.integers(0, 1 << 32, gap, dtype=np.uint64).astype(np.uint32))
        at += gap
        base.append(at)
        parts.append(keys)
        rows.append(keys)
        at += keys.size
    parts.append(rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32))
    return np.concatenate(parts), counts, base, rows


def _merge(ctx, form, src, counts, base, nb, open_bits, first, n, lead, surplus, rng):
    """runs msd_merge_buckets_u32 / _low16 with every buffer in an arena; returns the destination's host copy and the fill"""
    nsrc = counts.shape[0]
    s = src if form == "u32" else (src & np.uint32(0xFFFF)).astype(np.uint16)
    sa = arena_of(s, lead, guard=sort_guard("u32"))
    ca = arena_of(counts.reshape(-1), LEADS[(nsrc + 1) % 5])
    fill = rng.integers(0, 1 << 32, n + surplus, dtype=np.uint64).astype(np.uint32)
    da = arena_of(fill, LEADS[(LEADS.index(lead) + 2) % 5], "low", guard=sort_guard("u32") * 2)
    if form == "u32":
        call(ctx, "msd_merge_buckets_u32", sa.ptr, s.size, ca.ptr, ctx._u64arr(base), nsrc, nb, open_bits, first, da.ptr, n + surplus, n)
    else:
        call(ctx, "msd_merge_buckets_u32_low16", sa.ptr, s.size, ca.ptr, ctx._u64arr(base), nsrc, nb, first, da.ptr, n + surplus, n)
    st = ctx.stats()
    da.check(f"merge_buckets {form} dst")
    unchanged(sa, s, "merge_buckets src")
    unchanged(ca, counts.reshape(-1), "merge_buckets counts")
    return da.host(np.uint32), fill, st


@pytest.mark.parametrize("form,leaf", [("u32", 0), ("u32", 1), ("u32", 2), ("low16", 0)])   # (merge_leaf selects among the u32 form's leaves only)
@pytest.mark.parametrize("nsrc,nb,per_bucket,open_bits,lead", [(2, 64, 16000, 16, 16), (8, 300, 700, 16, 48), (3, 7, 40000, 16, 240), (5, 200, 3000, 12, 272), (1, 3, 5, 16, 0)])
def test_merge_buckets(ctx, form, leaf, nsrc, nb, per_bucket, open_bits, lead):
    """dst_cap > n_expected: the surplus keeps its fill; both leaves forced and the choice by bucket size"""
    if form == "low16" and open_bits != 16:
        open_bits = 16
    rng = np.random.default_rng(nsrc * 1000 + nb + leaf)
    first = 3 * nb
    src, counts, base, rows = _arrivals(rng, nsrc, nb, first, open_bits, per_bucket)
    n = int(counts.sum())
    ctx.set_option("merge_leaf", leaf)
    try:
        out, fill, st = _merge(ctx, form, src, counts, base, nb, open_bits, first, n, lead, 37, rng)
    finally:
        ctx.set_option("merge_leaf", DEFAULTS["merge_leaf"])
    assert (out[:n] == np.sort(np.concatenate(rows))).all()
    assert (out[n:] == fill[n:]).all(), "the surplus of the destination was written"


@pytest.mark.parametrize("form,leaf", [("u32", 1), ("u32", 2), ("low16", 0)])
def test_merge_buckets_rejected(ctx, form, leaf):
    """Buckets the leaves do not take (one key with 120000 copies, a crowded 256-value group; for the register-resident
    leaf also every bucket above its capacity) are finished by the general leaves in the destination."""
    rng = np.random.default_rng(4 + leaf)
    nsrc, nb = 4, 6
    src, counts, base, rows = _arrivals(rng, nsrc, nb, 0, 16, 120000, edit=lambda x, c: np.where(np.arange(nb) == nb // 2, 0, 30000))
    for x in range(nsrc):
        def sl(j):
            a = base[x] + int(counts[x, :j].sum())
            return slice(a, a + int(counts[x, j]))
        src[sl(2)] = np.uint32((2 << 16) | 77)
        src[sl(4)] &= np.uint32(0xFFFF00FF)
    allk = np.concatenate([src[base[x]:base[x] + int(counts[x].sum())] for x in range(nsrc)])
    n = int(counts.sum())
    ctx.set_option("merge_leaf", leaf)
    try:
        out, fill, st = _merge(ctx, form, src, counts, base, nb, 16, 0, n, 48, 5, rng)
    finally:
        ctx.set_option("merge_leaf", DEFAULTS["merge_leaf"])
    assert (out[:n] == np.sort(allk)).all() and (out[n:] == fill[n:]).all()
    assert st.get("merge_rejected", 0) >= 2, st


def _rb(ctx):
    return int(ctx._L.msd_hist2_record_bytes())


def _hist2_shard(rng, nb, first, per_bucket):
    c = rng.poisson(per_bucket, nb).astype(np.int64)
    pre = np.repeat(np.arange(first, first + nb, dtype=np.uint64), c)
    return ((pre << np.uint64(16)) | rng.integers(0, 1 << 16, int(c.sum()), dtype=np.uint64)).astype(np.uint32), c


@pytest.mark.parametrize("nsrc,nb,per_bucket,extra,lead", [(2, 24, 16384, 0, 16), (3, 50, 3000, 1000, 48), (1, 7, 17000, 0, 272), (8, 16, 12, 17408, 240)])
def test_hist2_pack_and_merge(ctx, nsrc, nb, per_bucket, extra, lead):
    """msd_bucket_bounds_u32 -> msd_hist2_pack_u32 -> msd_merge_buckets_u32_hist2, everything in arenas.  Source x packs its
    records to d_rec + x * nb * record bytes with rec_bytes = exactly its nb records (the next source's records, written
    before, must stay as they are) or `extra` bytes more (the surplus keeps its fill); the flag is a 4-byte arena.  The sum
    of the records, written out, is np.sort of all keys."""
    RB = _rb(ctx)
    rng = np.random.default_rng(nsrc * 131 + nb)
    first = 3 * nb
    fill = rng.integers(0, 256, nsrc * nb * RB + extra, dtype=np.uint8)
    rec = arena_of(fill, lead, guard=guardband.guard_elems(1, RB))
    counts = np.zeros((nsrc, nb), np.int64)
    allk = []
    for x in reversed(range(nsrc)):
        keys, c = _hist2_shard(rng, nb, first, per_bucket)
        counts[x] = c
        allk.append(keys)
        ka = arena_of(keys, LEADS[x % 5])
        ba = Arena(torch.int64, nb + 1, lead_bytes=LEADS[(x + 1) % 5], neighbours="high")
        fa = arena_of(np.array([0xDEAD], np.uint32), LEADS[(x + 2) % 5], "high")
        call(ctx, "msd_bucket_bounds_u32", ka.ptr, keys.size, 16, first, nb, ba.ptr)
        before = rec.host(np.uint8).copy()
        last = x == nsrc - 1
        call(ctx, "msd_hist2_pack_u32", ka.ptr, keys.size, ba.ptr, nb, rec.ptr + x * nb * RB, nb * RB + (extra if last else 0), fa.ptr)
        for a, w in ((rec, "records"), (ba, "bounds"), (fa, "flag")):
            a.check(f"hist2_pack {w} (source {x})")
        unchanged(ka, keys, "hist2_pack keys")
        assert (ba.host(np.uint64) == np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)).all()
        assert int(fa.host(np.uint32)[0]) == 0
        after = rec.host(np.uint8)
        lo, hi = x * nb * RB, (x + 1) * nb * RB
        assert (after[:lo] == before[:lo]).all() and (after[hi:] == before[hi:]).all(), f"source {x}: bytes outside its {nb} records changed"
    n = int(counts.sum())
    recs = rec.host(np.uint8).copy()
    ca = arena_of(counts.reshape(-1), 16)
    dfill = rng.integers(0, 1 << 32, n + 21, dtype=np.uint64).astype(np.uint32)
    da = arena_of(dfill, LEADS[(LEADS.index(lead) + 1) % 5], "low", guard=sort_guard("u32") * 2)
    call(ctx, "msd_merge_buckets_u32_hist2", rec.ptr, nsrc * nb * RB + extra, ca.ptr, nsrc, nb, first, da.ptr, n + 21, n)
    da.check("merge hist2 dst")
    unchanged(rec, recs, "merge hist2 records")
    unchanged(ca, counts.reshape(-1), "merge hist2 counts")
    out = da.host(np.uint32)
    assert (out[:n] == np.sort(np.concatenate(allk))).all() and (out[n:] == dfill[n:]).all()


def test_hist2_from_low_halves(ctx):
    """msd_order_low16_u32 -> msd_bounds_from_counts16 (65537 bounds in an arena) -> msd_hist2_pack_u32_low16 (256 records of
    exactly their size) -> msd_merge_buckets_u32_hist2 = np.sort of the keys."""
    RB = _rb(ctx)
    n = (1 << 22) + 5
    k = O.gen_uniform_u32(n, seed=123) & np.uint32(0x00FFFFFF)        # 256 buckets of about 2^14 keys
    ka = arena_of(k, 16)
    la = Arena(torch.int16, n, lead_bytes=48, neighbours="low")
    ca = Arena(torch.int64, 65536, lead_bytes=240)
    ba = Arena(torch.int64, 65537, lead_bytes=272, neighbours="high")
    call(ctx, "msd_order_low16_u32", ka.ptr, n, la.ptr, ca.ptr)
    counts = ca.host(np.uint64).copy()
    call(ctx, "msd_bounds_from_counts16", ca.ptr, ba.ptr)
    ba.check("bounds_from_counts16 bounds")
    unchanged(ca, counts, "bounds_from_counts16 counts")
    want = np.bincount(k >> np.uint32(16), minlength=65536)
    assert (counts == want.astype(np.uint64)).all()
    assert (ba.host(np.uint64) == np.concatenate([[0], np.cumsum(want)]).astype(np.uint64)).all()
    low = la.host(np.uint16).copy()
    bounds = ba.host(np.uint64).copy()
    fill = np.random.default_rng(1).integers(0, 256, 256 * RB, dtype=np.uint8)
    rec = arena_of(fill, 48, guard=guardband.guard_elems(1, RB))
    fa = arena_of(np.array([7], np.uint32), 16, "high")
    call(ctx, "msd_hist2_pack_u32_low16", la.ptr, n, ba.ptr, 256, rec.ptr, 256 * RB, fa.ptr)
    for a, w in ((rec, "records"), (fa, "flag")):
        a.check(f"hist2_pack_low16 {w}")
    unchanged(la, low, "hist2_pack_low16 low halves")
    unchanged(ba, bounds, "hist2_pack_low16 bounds")
    assert int(fa.host(np.uint32)[0]) == 0
    c256 = arena_of(want[:256].astype(np.int64), 0)
    da = Arena(torch.int32, n, lead_bytes=240, neighbours="low", guard=sort_guard("u32") * 2)
    call(ctx, "msd_merge_buckets_u32_hist2", rec.ptr, 256 * RB, c256.ptr, 1, 256, 0, da.ptr, n, n)
    da.check("merge hist2 dst")
    assert (da.host(np.uint32) == np.sort(k)).all()


@pytest.mark.parametrize("low16", [False, True])
@pytest.mark.parametrize("kind,flag", [("fits", 0), ("too many keys", 1), ("256 copies", 1), ("3000 listed values", 1)])
def test_hist2_overflow_flag(ctx, low16, kind, flag):
    """the 4-byte *d_overflow: set / cleared, nothing around it; the one record stays inside its 17408 bytes either way"""
    RB = _rb(ctx)
    rng = np.random.default_rng(17)
    k = {"fits": lambda: rng.permutation(60000).astype(np.uint32),
         "too many keys": lambda: rng.integers(0, 1 << 16, 70000, dtype=np.uint32),
         "256 copies": lambda: np.concatenate([rng.permutation(30000).astype(np.uint32), np.full(256, 31000, np.uint32)]),
         "3000 listed values": lambda: np.sort(rng.integers(0, 1 << 16, 3000, dtype=np.uint32).repeat(3))}[kind]()
    src = (k & np.uint32(0xFFFF)).astype(np.uint16) if low16 else k
    ka = arena_of(src, 48)
    ba = arena_of(np.array([0, k.size], np.uint64), 16)
    rec = arena_of(rng.integers(0, 256, RB, dtype=np.uint8), 272, guard=guardband.guard_elems(1, RB))
    fa = arena_of(np.array([0xDEAD], np.uint32), 240, "low")
    call(ctx, "msd_hist2_pack_u32_low16" if low16 else "msd_hist2_pack_u32", ka.ptr, k.size, ba.ptr, 1, rec.ptr, RB, fa.ptr)
    for a, w in ((rec, "record"), (fa, "flag")):
        a.check(f"hist2 overflow {w}")
    unchanged(ka, src, "hist2 keys")
    unchanged(ba, np.array([0, k.size], np.uint64), "hist2 bounds")
    assert (int(fa.host(np.uint32)[0]) != 0) == bool(flag)


@pytest.mark.parametrize("typ", ["u32", "u64"])
@pytest.mark.parametrize("shift_from_top,nb,first,lead", [(16, 1 << 16, 0, 16), (8, 256, 0, 48), (16, 8191, 8192 * 3, 240), (12, 100, 4000, 272), (16, 1, 5, 0)])
def test_bucket_bounds(ctx, typ, shift_from_top, nb, first, lead):
    bits = 8 * KEYB[typ]
    shift = bits - shift_from_top
    rng = np.random.default_rng(shift + nb)
    for n in (0, 1, 500_003):
        k = np.sort(make_keys("uniform", n, bits, rng)[0])
        ka = arena_of(k, lead)
        ba = Arena(torch.int64, nb + 1, lead_bytes=LEADS[(LEADS.index(lead) + 1) % 5], neighbours=NEIGH[nb % 2])
        call(ctx, f"msd_bucket_bounds_{typ}", ka.ptr, n, shift, first, nb, ba.ptr)
        ba.check(f"bucket_bounds n={n}")
        unchanged(ka, k, "bucket_bounds keys")
        want = np.searchsorted(k.astype(np.uint64) >> np.uint64(shift), np.arange(first, first + nb + 1, dtype=np.uint64), side="left")
        assert (ba.host(np.uint64) == want.astype(np.uint64)).all()


@pytest.mark.parametrize("typ", ["u32", "u64"])
@pytest.mark.parametrize("rb", [1, 5, 8, 12])
@pytest.mark.parametrize("n,lead", [(0, 0), (1, 16), (1001, 48), ((1 << 20) + 3, 272)])
def test_histogram(ctx, typ, rb, n, lead):
    bits = 8 * KEYB[typ]
    shift = bits - rb - (3 if rb < 12 else 0)
    k = make_keys("heavy", n, bits, np.random.default_rng(n + rb))[0] if n else np.zeros(0, UDT[KEYB[typ]])
    ka = arena_of(k, lead)
    ha = Arena(torch.int64, 1 << rb, lead_bytes=LEADS[rb % 5], neighbours=NEIGH[rb % 2])
    call(ctx, f"msd_histogram_{typ}", ka.ptr, n, shift, rb, ha.ptr)
    ha.check(f"histogram rb={rb}")
    unchanged(ka, k, "histogram keys")
    want = np.bincount(((k.astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << rb) - 1)).astype(np.int64), minlength=1 << rb)
    assert (ha.host(np.uint64) == want.astype(np.uint64)).all()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,lead", [(1, 16), (255, 48), (KSCANTILE - 1, 240), (KSCANTILE, 272), (KSCANTILE + 1, 0), (2 * KSCANTILE + 1, 16), (100_003, 48)])
def test_exclusive_scan(ctx, in_place, n, lead):
    x = O.gen_uniform_u64(n, seed=n) >> np.uint64(40)
    xa = arena_of(x, lead, "high")
    oa = xa if in_place else Arena(torch.int64, n, lead_bytes=LEADS[(LEADS.index(lead) + 1) % 5], neighbours="low")
    call(ctx, "msd_exclusive_scan_u64", xa.ptr, oa.ptr, n)
    oa.check("scan out")
    if not in_place:
        unchanged(xa, x, "scan in")
    want = np.concatenate([np.zeros(1, np.uint64), np.cumsum(x, dtype=np.uint64)[:-1]])
    assert (oa.host(np.uint64) == want).all()


@pytest.mark.parametrize("typ", ["u32", "u64"])
@pytest.mark.parametrize("parts", [1, 2, 256])
def test_sample_and_splitters(ctx, typ, parts):
    """msd_sample_*: m keys in an arena of exactly m (the CPU oracle draws the same positions); msd_splitters_*: parts - 1
    delimiters in an arena of exactly that many (none for one part: nothing is written at all)."""
    es = KEYB[typ]
    n = 300_001
    k = make_keys("heavy", n, 8 * es, np.random.default_rng(parts))[0]
    ka = arena_of(k, 16)
    for m in (1, 63, 20_001):
        sa = Arena(TDT[es], m, lead_bytes=LEADS[m % 5], neighbours=NEIGH[m % 2])
        call(ctx, f"msd_sample_{typ}", ka.ptr, n, m, 0xABCDEF, sa.ptr)
        sa.check(f"sample m={m}")
        want = (O.sample_u32 if typ == "u32" else O.sample_u64)(k, m, seed=0xABCDEF)
        assert (sa.host(UDT[es]) == want).all()
    unchanged(ka, k, "sample keys")
    s = np.sort(want)
    ssa = arena_of(s, 48)
    da = Arena(TDT[es], parts - 1, lead_bytes=272, neighbours="low")
    call(ctx, f"msd_splitters_{typ}", ssa.ptr, s.size, parts, da.ptr)
    da.check(f"splitters parts={parts}")
    unchanged(ssa, s, "sorted sample")
    assert (da.host(UDT[es]).astype(np.uint64) == O.extract_delimiters(s.astype(np.uint64), parts)).all()


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("base,lead", [(0, 16), (1024, 48), (1 << 20, 272)])
def test_generators(ctx, base, r, lead):
    """msd_gen_*: n mod 4 = 1, 2, 3; the output arena holds exactly n elements"""
    n = base + r
    a32 = lambda: Arena(torch.int32, n, lead_bytes=lead, neighbours=NEIGH[r % 2])  # noqa: E731
    a64 = lambda: Arena(torch.int64, n, lead_bytes=lead, neighbours=NEIGH[r % 2])  # noqa: E731
    a = a32()
    call(ctx, "msd_gen_uniform_u32", a.ptr, n, 0x5EED0001, 12345)
    a.check("gen_uniform_u32")
    assert (a.host(np.uint32) == O.gen_uniform_u32(n, seed=0x5EED0001, first=12345)).all()
    a = a64()
    call(ctx, "msd_gen_uniform_u64", a.ptr, n, 0x5EED0005, 7, 32)
    a.check("gen_uniform_u64")
    assert (a.host(np.uint64) == O.gen_uniform_u64(n, seed=0x5EED0005, first=7) >> np.uint64(32)).all()
    a = a32()
    call(ctx, "msd_gen_zipf_u32", a.ptr, n, 0x5EED0003, 0)
    a.check("gen_zipf_u32")
    z, ez = a.host(np.uint32).astype(np.int64), O.gen_zipf_u32(n, seed=0x5EED0003).astype(np.int64)
    # (the device's pow may differ from the host's in the last ulp: the tolerance of test_device_generators_match_oracle)
    assert (np.abs(z - ez) <= np.maximum(1, ez >> 40)).all() and (z != ez).mean() < max(1e-3, 1.5 / n)
    a = a32()
    call(ctx, "msd_gen_dup_u32", a.ptr, n, 77, 5, 1000)
    a.check("gen_dup_u32")
    assert (a.host(np.uint32) == O.gen_dup_u32(n, 1000, seed=77, first=5)).all()
    a = a64()
    call(ctx, "msd_gen_iota_u64", a.ptr, n, 1 << 40)
    a.check("gen_iota_u64")
    assert (a.host(np.uint64) == np.arange(n, dtype=np.uint64) + np.uint64(1 << 40)).all()


@pytest.mark.parametrize("n", [1, 311, 312, 313, 623, 624, 625, 5003])
def test_generators_mt19937_64(ctx, n):
    """one workgroup walks the stream in steps of its 312-word state"""
    a = Arena(torch.int64, n, lead_bytes=LEADS[n % 5], neighbours=NEIGH[n % 2])
    call(ctx, "msd_gen_mt19937_64", a.ptr, n, 5489, 0)
    a.check("gen_mt19937_64")
    assert (a.host(np.uint64) == O.mt19937_64(n, 5489)).all()


# ------------------------------------------------------------------ D. top-k and select

U32, I32, F32, U64, I64, F64 = range(6)
KT_BYTES = {U32: 4, I32: 4, F32: 4, U64: 8, I64: 8, F64: 8}


def topk_input(kt, kind, n, rng):
    """bit patterns of n keys of key type kt"""
    ut = UDT[KT_BYTES[kt]]
    if kind == "const":
        return np.full(n, np.array([-1.5], np.float32 if KT_BYTES[kt] == 4 else np.float64).view(ut)[0], ut)
    if kind == "dup":            # 200 values only: the bits run out on heavy values
        vals = rng.integers(0, np.iinfo(ut).max, 200, dtype=ut, endpoint=True)
        return vals[rng.integers(0, 200, n)]
    if kt % 3 == 2:              # floats: normal scores and a few special values (NaNs of both signs, zeros, infinities)
        ft = np.float32 if KT_BYTES[kt] == 4 else np.float64
        a = rng.standard_normal(n).astype(ft)
        sp = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf], ft)
        a[rng.integers(0, n, min(n, 12))] = sp[rng.integers(0, 6, min(n, 12))]
        return a.view(ut).copy()
    return rng.integers(0, np.iinfo(ut).max, n, dtype=ut, endpoint=True)


# (entry point, key type, with indices)
TOPK_VARIANTS = [("msd_topk_u32", U32, False), ("msd_topk_u64", U64, False), ("msd_topk_pairs_u64", U64, True)] + \
                [("msd_topk_keys", kt, idx) for kt in range(6) for idx in (False, True)]
N_TOPK = 70_001


@pytest.mark.parametrize("cap", [1 << 20, 4096, 1])
@pytest.mark.parametrize("kind", ["spread", "dup", "const"])
@pytest.mark.parametrize("entry,kt,idx", TOPK_VARIANTS, ids=[f"{e}-kt{k}-{'idx' if i else 'noidx'}" for e, k, i in TOPK_VARIANTS])
def test_topk(ctx, entry, kt, idx, kind, cap):
    """Output arenas of exactly k elements: out[k:] IS the back guard.  k = 0, 1, 2, 3, 5, a rank with keys straight to the
    output and candidates both present, n - 1, n; both directions; the one-pass path (default select_cap) and the deep
    path (select_cap 4096 and 1: more histogram passes, bits that run out).  With indices on a 32-bit key type the
    index arena is the buffer the filter writes its packed 8-byte elements to.  Keys (and rids) are arenas too."""
    es = KT_BYTES[kt]
    ut = UDT[es]
    n = N_TOPK
    rng = np.random.default_rng(kt * 10 + len(kind))
    bits = topk_input(kt, kind, n, rng)
    codes = np_encode(bits, kt)
    order = np.argsort(codes, kind="stable")
    S = bits[order]
    ka = arena_of(bits, LEADS[kt % 5], guard=sort_guard("u64" if es == 8 else "u32"))
    pairs = entry == "msd_topk_pairs_u64"
    rids = rng.permutation(n).astype(np.uint64) + np.uint64(1 << 33)
    ra = arena_of(rids, 48, guard=sort_guard("pairs")) if pairs else None
    typ = "pairs" if (pairs or (idx and es == 8)) else ("u64" if es == 8 or idx else "u32")   # what sorts the output
    ctx.set_option("select_cap", cap)
    try:
        for kk in (0, 1, 2, 3, 5, n // 3, n - 1, n):
            for which in (0, 1):
                oa = Arena(TDT[es], kk, lead_bytes=LEADS[(kk + which) % 5], neighbours=NEIGH[which], guard=sort_guard(typ))
                ia = Arena(torch.int64, kk, lead_bytes=LEADS[(kk + which + 2) % 5], neighbours=NEIGH[1 - which], guard=sort_guard(typ)) if idx else None
                if pairs:
                    call(ctx, entry, ka.ptr, ra.ptr, n, kk, which, oa.ptr, ia.ptr)
                elif entry == "msd_topk_keys":
                    call(ctx, entry, ka.ptr, kt, n, kk, which, oa.ptr, ia.ptr if idx else None)
                else:
                    call(ctx, entry, ka.ptr, n, kk, which, oa.ptr)
                st = ctx.stats()
                what = f"{entry} kt={kt} k={kk} which={which} cap={cap} {kind}"
                oa.check(what + " out")
                want = S[n - kk:] if which else S[:kk]
                got = oa.host(ut)
                assert (got == want).all(), what
                if idx:
                    ia.check(what + (" out rids" if pairs else " out indices"))
                    pos = ia.host(np.uint64)
                    if pairs:            # every (key, rid) written is a tuple of the input, none twice
                        pos = pos - np.uint64(1 << 33)
                        assert (pos < n).all()
                        where = np.empty(n, np.int64)
                        where[(rids - np.uint64(1 << 33)).astype(np.int64)] = np.arange(n)
                        pos = where[pos.astype(np.int64)]
                    assert (pos.astype(np.int64) < n).all() and len(np.unique(pos)) == kk, what
                    assert (bits[pos.astype(np.int64)] == got).all(), what
                if kk == n // 3 and kind == "spread" and cap == 4096:
                    assert st["select_below"] > 0 and st["select_candidates"] > 0 and st["select_below"] < kk <= st["select_below"] + st["select_candidates"], st
                if kk == n // 3 and kind == "spread" and cap == 1 and es == 4 and kt % 3 != 2:
                    assert st["select_hist_passes"] >= 2, st
    finally:
        ctx.set_option("select_cap", DEFAULTS["select_cap"])
    unchanged(ka, bits, "top-k keys")
    if pairs:
        unchanged(ra, rids, "top-k rids")


@pytest.mark.parametrize("entry,kt,idx", [("msd_topk_u32", U32, False), ("msd_topk_keys", F32, True), ("msd_topk_pairs_u64", U64, True)])
def test_topk_long_guards_and_large_k(ctx, entry, kt, idx):
    """2^21 + 3 keys, k around a third and all but one of them (the dense filter path: long runs per reservation); guards
    as long as the outputs"""
    es, n = KT_BYTES[kt], (1 << 21) + 3
    rng = np.random.default_rng(kt)
    bits = topk_input(kt, "spread", n, rng)
    S = bits[np.argsort(np_encode(bits, kt), kind="stable")]
    ka = arena_of(bits, 16)
    pairs = entry == "msd_topk_pairs_u64"
    ra = arena_of(np.arange(n, dtype=np.uint64), 48) if pairs else None
    for kk, which in ((n // 3, 0), (n - 1, 1), (n // 40, 1)):
        oa = Arena(TDT[es], kk, lead_bytes=240, neighbours=NEIGH[which], guard=kk)
        ia = Arena(torch.int64, kk, lead_bytes=272, neighbours=NEIGH[1 - which], guard=kk) if idx else None
        if pairs:
            call(ctx, entry, ka.ptr, ra.ptr, n, kk, which, oa.ptr, ia.ptr)
        elif idx:
            call(ctx, entry, ka.ptr, kt, n, kk, which, oa.ptr, ia.ptr)
        else:
            call(ctx, entry, ka.ptr, n, kk, which, oa.ptr)
        oa.check(f"{entry} k={kk} out")
        got = oa.host(UDT[es])
        assert (got == (S[n - kk:] if which else S[:kk])).all()
        if idx:
            ia.check(f"{entry} k={kk} indices")
            pos = ia.host(np.uint64).astype(np.int64)
            assert ((pos >= 0) & (pos < n)).all() and len(np.unique(pos)) == kk and (bits[pos] == got).all()
    unchanged(ka, bits, "top-k keys")
    if pairs:
        unchanged(ra, np.arange(n, dtype=np.uint64), "top-k rids")
