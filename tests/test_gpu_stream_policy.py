"""The two big stream kernels where a changed load or store can go wrong: masks, partial vectors and the array's end.

classify_direct2_kernel (csrc/msd_direct.hpp) and count_place16_kernel (csrc/msd_count16.hpp) take the cache policy of
their 16-byte loads and stores from compile-time knobs (MSD_D2_NT, MSD_C16_NT), and both exist twice: the host launches
the instantiation with the policy for arrays of at least 256 MiB (kStreamMinBytes, csrc/msd_device.hpp), the plain one
below.  Whatever the setting, the result is the sorted array, bit for bit; these cases aim at the accesses the knobs
touch, in both instantiations ("small": the array is the test's keys; "big": the same keys at the END of an array of
just over 256 MiB whose other keys belong to no segment and must stay where they are).

Leaf (``ctx.sort_segments`` with ``count16 = 2``: every counting-leaf segment goes through count_place16_kernel first),
against numpy's sort, keys outside the segments must stay where they are:
  * segment starts 0-3 modulo 4 (the elements in front of the segment inside its first 16-byte vector are masked);
  * counts 1, 3, 4, 5 and, with the start's offset, CAP - 3, CAP (the last vectors of the grid: taken) and CAP + 1
    (rejected, left untouched for count_place_kernel);
  * 9, 12 and 16 open bits;
  * a last segment that ends 1-3 elements short of a vector at the very end of a guarded allocation;
  * a value with 256 copies (rejected; the counters must still be clear for the next segment);
  * 3 * (workgroups resident) + 1 segments: every workgroup runs both copies of the loop body.

Direct round, u32 / u64 / tuples at 2^22 + 5 keys (the smallest size at which a direct round is planned) and at the first
size of 256 MiB (2^26 + 5 u32 keys, 2^25 + 5 u64 keys, 2^24 + 5 tuples), whole tensors and views that start at element 4
of a larger one (head and tail keys exist, the first slot is not slot 0), against torch.sort; u32 at 5 * 2^25 keys on
the front-count path, by the exact verdict of tests/exact_verdict.py.
"""
import numpy as np
import pytest
import torch

import exact_verdict as V
from guardband import Arena
from gpu_support import DEFAULTS, restore_defaults

pytestmark = pytest.mark.gpu

CAP = 17408             # kC16Cap (csrc/msd_count16.hpp): elements on the 16-byte grid
STREAM_MIN = 256 << 20  # kStreamMinBytes (csrc/msd_device.hpp)
BASE = STREAM_MIN // 4  # u32 keys in front of a "big" case's own keys (a multiple of 4: starts keep their offset)
SIZES = ["small", "big"]


@pytest.fixture()
def leaf_ctx(ctx):
    ctx.set_option("count16", 2)
    yield ctx
    ctx.set_option("count16", DEFAULTS["count16"])


@pytest.fixture(scope="module")
def filler(ctx):
    """BASE uniform keys that belong to no segment, generated once and left unchanged"""
    t = torch.empty(BASE, dtype=torch.int32, device="cuda")
    ctx.gen_uniform_u32(t, seed=0x5EED0009)
    return t


def make_segments(sizes, end_bit, lead, trail, seed, copies256=()):
    """keys, segment offsets and the expected array.  Segment i lies behind segment i - 1 and has its own prefix above
    `end_bit`; `lead` / `trail` random keys belong to no segment; segments listed in `copies256` get one value 256 times."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[lead], lead + np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1]) + trail
    k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for i, sz in enumerate(sizes):
        if sz < 2:
            continue                                                  # (a spacer: never moved, keeps its random key)
        v = rng.integers(0, 1 << end_bit, sz, dtype=np.uint32)
        if i in copies256:
            v = rng.integers(1 << (end_bit - 1), 1 << end_bit, sz, dtype=np.uint32)
            v[rng.permutation(sz)[:256]] = 5
        k[offs[i]:offs[i + 1]] = v | np.uint32(((i * 37 + 1) % 200) << end_bit)
    want = k.copy()
    for i in range(len(sizes)):
        want[offs[i]:offs[i + 1]] = np.sort(k[offs[i]:offs[i + 1]])
    return k, [int(o) for o in offs], want


def run_leaf(ctx, filler, size, k, offs, want, end_bit, guarded=False):
    """sorts the segments of `k` -- alone, or as the last keys of an array of BASE + len(k) -- and compares; returns the stats"""
    base = BASE if size == "big" else 0
    n = base + k.size
    ar = None
    if guarded:
        ar = Arena(torch.int32, n, guard=2 * CAP)
        t = ar.payload
    else:
        t = torch.empty(n, dtype=torch.int32, device="cuda")
    t[:base] = filler[:base]
    t[base:] = torch.from_numpy(k.view(np.int32)).cuda()
    ctx.sort_segments(t, [base + o for o in offs], end_bit)
    st = ctx.stats()
    if ar is not None:
        ar.check("count_place16_kernel at the array's end")
    out = t[base:].cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(out != want)
    seg_of = np.searchsorted(offs, bad[:8], side="right") - 1
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[:8]} (segments {seg_of})"
    assert torch.equal(t[:base], filler[:base]), "keys in front of the segments moved"
    return st


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("end_bit", [9, 12, 16])
@pytest.mark.parametrize("start_mod", [0, 1, 2, 3])
def test_leaf_starts_and_counts(leaf_ctx, filler, start_mod, end_bit, size):
    """every count of the list at a start of `start_mod` modulo 4, a one-element spacer run behind each to restore it"""
    counts = [1, 3, 4, 5, CAP - 3 - start_mod, CAP - start_mod, CAP - start_mod + 1, 4, CAP - start_mod, 3, 16384]
    sizes, big = [], []
    for c in counts:
        big.append(len(sizes))
        sizes.append(c)
        sizes.extend([1] * ((-c) % 4))
    k, offs, want = make_segments(sizes, end_bit, lead=4 + start_mod, trail=7, seed=100 + 4 * end_bit + start_mod)
    assert [offs[i] % 4 for i in big] == [start_mod] * len(big)
    st = run_leaf(leaf_ctx, filler, size, k, offs, want, end_bit)
    assert st.get("count_segments", 0) == sum(sz >= 64 for sz in sizes), st


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("short", [1, 2, 3])
@pytest.mark.parametrize("last", [CAP - 8, 100])
def test_leaf_last_segment_ends_with_the_allocation(leaf_ctx, filler, short, last, size):
    """The array ends `short` elements behind a multiple of 4 and its last segment ends with it, directly in front of
    the back guard: the segment's last vector would reach into the guard, so the kernel may neither take the segment nor
    request it early (the n_total test of prefetch); the guards are what they were."""
    body = [16384, 16380, 16384]
    lead = 8
    fill = (short - (lead + sum(body) + last)) % 4
    sizes = body + [1] * fill + [last]
    k, offs, want = make_segments(sizes, 16, lead=lead, trail=0, seed=200 + short)
    assert offs[-1] % 4 == short and offs[-1] == k.size
    run_leaf(leaf_ctx, filler, size, k, offs, want, 16, guarded=True)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("end_bit", [9, 16])
def test_leaf_rejected_overflow_leaves_counters_clear(leaf_ctx, filler, end_bit, size):
    """segments with a value of 256 copies (byte overflow: rejected, cleared by clear_all) in front of ordinary ones, which
    find the counters as the rejected ones left them"""
    sizes = [12000, 12001, 12000, 12003, 12002, 12000, 12001, 12000]
    k, offs, want = make_segments(sizes, end_bit, lead=1, trail=2, seed=300 + end_bit, copies256=(0, 2, 3, 6))
    run_leaf(leaf_ctx, filler, size, k, offs, want, end_bit)


@pytest.mark.parametrize("size", SIZES)
def test_leaf_three_segments_per_workgroup_and_one(leaf_ctx, filler, size):
    """3 * (workgroups resident: two per CU) + 1 segments of 1025-1029 keys (starts drift over 0-3 modulo 4)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [1025 + (i % 5) for i in range(3 * 2 * cus + 1)]
    k, offs, want = make_segments(sizes, 12, lead=3, trail=1, seed=400)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    st = run_leaf(leaf_ctx, filler, size, k, offs, want, 12)
    assert st.get("count_segments", 0) == len(sizes), st


# ---------------------------------------------------------------------------------------------- direct rounds

N_DIRECT = {("u32", "small"): (1 << 22) + 5, ("u64", "small"): (1 << 22) + 5, ("tuples", "small"): (1 << 22) + 5,
            ("u32", "big"): (1 << 26) + 5, ("u64", "big"): (1 << 25) + 5, ("tuples", "big"): (1 << 24) + 5}


@pytest.fixture()
def dctx(ctx):
    names = ("direct_mode", "direct_min", "direct_min_parent", "front_count", "front_min", "count16")
    restore_defaults(ctx, *names)
    yield ctx
    restore_defaults(ctx, *names)


@pytest.fixture(scope="module")
def inputs():
    """what direct_input has made so far; given back behind the module's last test"""
    made = {}
    yield made
    made.clear()


def direct_input(_inputs, ctx, kind, size):
    """uniform keys and their torch.sort (unsigned order), computed once per shape and left unchanged"""
    if (kind, size) not in _inputs:
        n = N_DIRECT[kind, size]
        if kind == "u32":
            k = torch.empty(n, dtype=torch.int32, device="cuda")
            ctx.gen_uniform_u32(k, seed=0x5EED0001)
            flip = -(1 << 31)
        else:
            k = torch.empty(n, dtype=torch.int64, device="cuda")
            ctx.gen_uniform_u64(k, seed=0x5EED0005)
            flip = -(1 << 63)
        _inputs[kind, size] = (k, torch.sort(k ^ flip).values ^ flip)
    return _inputs[kind, size]


def placed(keys, view):
    """`keys` as a whole tensor, or as a view that starts at element 4 of a larger zeroed one (with that tensor)"""
    if not view:
        return keys.clone(), None
    whole = torch.zeros(keys.numel() + 8, dtype=keys.dtype, device="cuda")
    v = whole[4:4 + keys.numel()]
    v.copy_(keys)
    return v, whole


def rim_untouched(whole, n):
    return whole is None or (int(whole[:4].abs().sum()) == 0 and int(whole[4 + n:].abs().sum()) == 0)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("view", [False, True])
def test_direct_round_u32(dctx, inputs, view, size):
    k, ref = direct_input(inputs, dctx, "u32", size)
    t, whole = placed(k, view)
    dctx.sort_u32(t)
    st = dctx.stats()
    assert st.get("direct_rounds", 0) >= 1, st
    assert torch.equal(t, ref)
    assert rim_untouched(whole, k.numel())


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("view", [False, True])
def test_direct_round_u64(dctx, inputs, view, size):
    k, ref = direct_input(inputs, dctx, "u64", size)
    t, whole = placed(k, view)
    dctx.sort_u64(t)
    st = dctx.stats()
    assert st.get("direct_rounds", 0) >= 1, st
    assert torch.equal(t, ref)
    assert rim_untouched(whole, k.numel())


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("view", [False, True])
def test_direct_round_tuples(dctx, inputs, view, size):
    """the rids are the keys' positions: behind the sort rid i must sit next to the key that was at position i"""
    k, ref = direct_input(inputs, dctx, "tuples", size)
    n = k.numel()
    t, whole = placed(k, view)
    r, rwhole = placed(torch.arange(n, dtype=torch.int64, device="cuda"), view)
    dctx.sort_pairs_u64(t, r)
    st = dctx.stats()
    assert st.get("direct_rounds", 0) >= 1, st
    assert torch.equal(t, ref)
    assert torch.equal(k[r], t), "a rid left its key"
    assert int(torch.sort(r).values.ne(torch.arange(n, dtype=torch.int64, device="cuda")).sum()) == 0, "rids are no permutation"
    assert rim_untouched(whole, n) and rim_untouched(rwhole, n)


def test_front_count_path_u32(dctx):
    """5 * 2^25 uniform keys with the front pass allowed from 2^27 on: the top 16 bits are counted once, both direct rounds
    are placed from that count, the counting leaf finishes -- all three stream kernels at a size where every workgroup
    runs many tiles and segments"""
    n = 5 << 25
    dctx.set_option("front_min", 1 << 27)
    t = torch.empty(n, dtype=torch.int32, device="cuda")
    dctx.gen_uniform_u32(t, seed=0x5EED0001)
    fp = V.fingerprint(t)
    dctx.sort_u32(t)
    st = dctx.stats()
    assert st.get("front_count_sorts", 0) == 1 and st.get("direct_rounds", 0) == 2, st
    V.assert_sorted_permutation(fp, t)
