"""GPU tests of radix select / top-k (msd_topk_*, msd_select_*): the output is a slice of the sorted input, bit-exact,
the input is untouched; both the one-pass and the deep (several histogram passes, bits exhausted) paths are taken;
bad arguments are refused without touching anything.  Expected values come from np.sort and the CPU oracle's sorts."""
import numpy as np
import pytest

from oracle import oracle as O
from gpu_support import DEFAULTS, host_bits as host

pytestmark = pytest.mark.gpu

DEFAULT_CAP = DEFAULTS["select_cap"]  # the library's default "select_cap" (include/msd_radix_hip.h)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    assert a.dtype == np.uint64
    return torch.from_numpy(a.view(np.int64)).cuda()


# (the generators of tests/test_gpu_parity.py)
def make_u32(n, kind, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return O.gen_uniform_u32(n, seed=0x5EED0001 + seed)
    if kind == "zipf":
        return O.gen_zipf_u32(n, seed=0x5EED0003 + seed)
    if kind == "dup256":
        return rng.integers(0, 256, n, dtype=np.uint32) * np.uint32(0x01010101)
    if kind == "const":
        return np.full(n, 0xDEADBEEF, np.uint32)
    if kind == "sorted":
        return np.sort(O.gen_uniform_u32(n, seed=seed))
    if kind == "reverse":
        return np.sort(O.gen_uniform_u32(n, seed=seed))[::-1].copy()
    if kind == "skew8":
        return (rng.random(n) ** 8 * 2**32).astype(np.uint32)
    if kind == "lowbits":
        return rng.integers(0, 1 << 12, n, dtype=np.uint32)
    raise ValueError(kind)


def make_u64(n, kind, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return O.gen_uniform_u64(n, seed=0x5EED0005 + seed)
    if kind == "upper_zero":
        return O.gen_uniform_u64(n, seed=0x5EED0005 + seed) >> np.uint64(32)
    if kind == "dup256":
        return rng.integers(0, 256, n, dtype=np.uint64) * np.uint64(0x0101010101010101)
    if kind == "const":
        return np.full(n, 0xDEADBEEFCAFEF00D, np.uint64)
    raise ValueError(kind)


def k_list(n):
    return sorted({k for k in (0, 1, 2, n // 1000 + 1, n // 2, n - 1, n) if 0 <= k <= n})


def check_keys(ctx, k, S=None):
    """top-k and select of the key array k for every k of the list and both directions, against the sorted array S."""
    n = len(k)
    if S is None:
        S = np.sort(k)
    t = dev(k)
    for kk in k_list(n):
        for largest in (False, True):
            out = ctx.topk(t, kk, largest=largest)
            assert out.numel() == kk
            want = S[n - kk:] if largest else S[:kk]
            assert (host(out) == want).all(), (n, kk, largest)
            if kk < n:
                assert ctx.select(t, kk, largest=largest) == int(S[n - 1 - kk] if largest else S[kk]), (n, kk, largest)
    assert (host(t) == k).all(), "the input was modified"


SIZES = [1, 2, 64, 65, 4097, 70001, 1 << 20, (1 << 21) + 77]
KINDS = ["uniform", "zipf", "dup256", "const", "sorted", "reverse", "skew8", "lowbits"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_topk_select_u32_equal_sorted_slice(ctx, n, kind):
    k = make_u32(n, kind, seed=n % 97 + 1)
    S = np.sort(k)
    assert (S == O.sort_u32(k)).all()
    check_keys(ctx, k, S)


SIZES64 = [1, 65, 70001, (1 << 20) + 7]
KINDS64 = ["uniform", "upper_zero", "dup256", "const"]


@pytest.mark.parametrize("n", SIZES64)
@pytest.mark.parametrize("kind", KINDS64)
def test_topk_select_u64_equal_sorted_slice(ctx, n, kind):
    k = make_u64(n, kind, seed=n % 97 + 1)
    S = np.sort(k)
    assert (S == O.sort_u64(k)).all()
    check_keys(ctx, k, S)


@pytest.mark.parametrize("n", SIZES64)
@pytest.mark.parametrize("kind", KINDS64)
def test_topk_pairs_u64(ctx, n, kind):
    import torch
    k = make_u64(n, kind, seed=n % 97 + 2)
    S = np.sort(k)
    tk = dev(k)
    tr = torch.arange(n, dtype=torch.int64, device="cuda")
    for kk in k_list(n):
        for largest in (False, True):
            ok, orr = ctx.topk(tk, kk, largest=largest, rids=tr)
            assert ok.numel() == kk and orr.numel() == kk
            hk, hr = host(ok), orr.cpu().numpy()
            assert (hk == (S[n - kk:] if largest else S[:kk])).all(), (n, kk, largest)
            assert ((hr >= 0) & (hr < n)).all()
            assert (k[hr] == hk).all(), "a (key, rid) written is not a tuple of the input"
            assert len(np.unique(hr)) == kk, "an input position was used twice"
    assert (host(tk) == k).all() and (tr.cpu().numpy() == np.arange(n)).all(), "the input was modified"


# ---- both paths are really taken

N_DEEP = (1 << 21) + 77


def _topk_with_stats(ctx, k, kk):
    t = dev(k)
    S = np.sort(k)
    n = len(k)
    res = {}
    for largest in (False, True):
        out = ctx.topk(t, kk, largest=largest)
        st = ctx.stats()
        assert (host(out) == (S[n - kk:] if largest else S[:kk])).all()
        assert ctx.select(t, kk, largest=largest) == int(S[n - 1 - kk] if largest else S[kk])
        sst = ctx.stats()
        for name in ("select_hist_passes", "select_skipped_bits", "select_candidates", "select_below"):
            assert name in st and name in sst, name
        assert st["select_below"] < kk <= st["select_below"] + st["select_candidates"], st
        res[largest] = st
    assert (host(t) == k).all()
    return res


def test_stats_small_cap_takes_both_paths(ctx):
    try:
        ctx.set_option("select_cap", 4096)
        kk = N_DEEP // 3
        for largest, st in _topk_with_stats(ctx, make_u32(N_DEEP, "uniform", seed=1), kk).items():
            assert st["select_hist_passes"] == 1 and st["select_candidates"] <= 4096, st
            assert st["select_below"] + st["select_candidates"] >= kk > st["select_below"], st
        # (from the small end rank n/3 lies in the crowded low buckets of both; from the large end of skew8 the keys
        # are thin there and one pass may do, so only the result is checked)
        for kind in ("skew8", "zipf"):
            st = _topk_with_stats(ctx, make_u32(N_DEEP, kind, seed=1), kk)
            assert st[False]["select_hist_passes"] >= 2, (kind, st)
            assert st[False]["select_candidates"] <= 4096 or st[False]["select_hist_passes"] == 3, (kind, st)
        for largest, st in _topk_with_stats(ctx, make_u32(N_DEEP, "const", seed=1), kk).items():
            assert st["select_candidates"] == N_DEEP and st["select_below"] == 0, st
        k64 = O.gen_uniform_u64(1 << 20, seed=5) >> np.uint64(32)
        for largest, st in _topk_with_stats(ctx, k64, len(k64) // 3).items():
            assert st["select_skipped_bits"] >= 32 and st["select_hist_passes"] <= 2, st
    finally:
        ctx.set_option("select_cap", DEFAULT_CAP)


def test_stats_default_cap_same_inputs(ctx):
    ctx.set_option("select_cap", DEFAULT_CAP)
    kk = N_DEEP // 3
    for kind in ("uniform", "skew8", "zipf", "const"):
        _topk_with_stats(ctx, make_u32(N_DEEP, kind, seed=1), kk)
    k64 = O.gen_uniform_u64(1 << 20, seed=5) >> np.uint64(32)
    for largest, st in _topk_with_stats(ctx, k64, len(k64) // 3).items():
        assert st["select_skipped_bits"] >= 32, st


def test_tiny_cap_forces_every_pass(ctx):
    """select_cap = 1: the search runs until the pivot bucket holds one key or the bits are used up."""
    try:
        ctx.set_option("select_cap", 1)
        check_keys(ctx, make_u32(70001, "uniform", seed=3))
        check_keys(ctx, make_u32(70001, "dup256", seed=3))
        check_keys(ctx, make_u64(70001, "uniform", seed=3))
        check_keys(ctx, make_u64(70001, "upper_zero", seed=3))
    finally:
        ctx.set_option("select_cap", DEFAULT_CAP)


def test_phases_with_profiling(ctx):
    t = dev(make_u32(1 << 20, "uniform", seed=2))
    try:
        ctx.set_profiling(True)
        ctx.topk(t, 1000)
        names = [p[0] for p in ctx.phases()]
    finally:
        ctx.set_profiling(False)
    assert "select_hist" in names and "select_filter" in names, names


# ---- arguments

def test_bad_arguments_are_refused_and_touch_nothing(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdError
    n = 5000
    k = make_u32(n, "uniform", seed=9)
    t = dev(k)
    out = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out0 = out.clone()

    def refused(f):
        with pytest.raises(MsdError) as e:
            f()
        assert "error -1" in str(e.value), str(e.value)  # MSD_EINVAL and its message
        assert len(str(e.value)) > len("error -1: ")
        assert (host(t) == k).all() and torch.equal(out, out0)

    big = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    refused(lambda: ctx._ok(ctx._L.msd_topk_u32(ctx._h, ctx._ptr(t, 4), n, n + 1, 0, ctx._ptr(big, 4))))  # k > n
    assert torch.equal(big, out0)
    refused(lambda: ctx.select(t, n))                       # k >= n
    refused(lambda: ctx.select(t, n + 5, largest=True))
    refused(lambda: ctx.topk(t, 100, out=out[1:]))          # misaligned output: a view offset by one element
    refused(lambda: ctx.topk(t, 100, out=t[:100]))          # the output aliases the input
    refused(lambda: ctx.topk(t, 100, out=t[n - 100:]))
    refused(lambda: ctx._ok(ctx._L.msd_topk_u32(ctx._h, ctx._ptr(t, 4), n, 100, 2, ctx._ptr(out, 4))))   # which = 2
    v = __import__("ctypes").c_uint32(77)
    refused(lambda: ctx._ok(ctx._L.msd_select_u32(ctx._h, ctx._ptr(t, 4), n, 1, 2, v)))
    assert v.value == 77
    refused(lambda: ctx._ok(ctx._L.msd_topk_u32(ctx._h, ctx._ptr(t, 4), n, 100, 0, None)))               # null output
    # tuples: rids checked the same way
    k64 = make_u64(n, "uniform", seed=9)
    tk, tr = dev(k64), torch.arange(n, dtype=torch.int64, device="cuda")
    o64 = torch.zeros(200, dtype=torch.int64, device="cuda")
    with pytest.raises(MsdError):
        ctx.topk(tk, 100, rids=tr, out=o64[:100], out_rids=tr[:100])
    with pytest.raises(MsdError):
        ctx.topk(tk, 100, rids=tr, out=o64[:100], out_rids=o64[50:150])
    assert (host(tk) == k64).all() and (tr.cpu().numpy() == np.arange(n)).all() and not o64.any()
    # k == 0: an empty result, nothing touched
    e = ctx.topk(t, 0)
    assert e.numel() == 0
    ctx.topk(t, 0, out=out)
    assert torch.equal(out, out0)
    ek, er = ctx.topk(tk, 0, rids=tr)
    assert ek.numel() == 0 and er.numel() == 0
    z = torch.empty(0, dtype=torch.int32, device="cuda")
    assert ctx.topk(z, 0).numel() == 0  # n == 0 && k == 0


# ---- larger than any leaf, once

def test_topk_2_28_uniform_against_full_sort(ctx):
    import torch
    n, kk = 1 << 28, 1 << 16
    t = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform_u32(t, seed=0x5EED0011)
    before = ctx.check(t)
    lo = ctx.topk(t, kk)
    hi = ctx.topk(t, kk, largest=True)
    v_lo, v_hi = ctx.select(t, kk), ctx.select(t, kk, largest=True)
    after = ctx.check(t)
    assert before[1:] == after[1:], "the input was modified"
    s = t.clone()
    ctx.sort_u32(s)
    assert torch.equal(lo, s[:kk]) and torch.equal(hi, s[n - kk:])
    assert v_lo == int(s[kk].item()) & 0xFFFFFFFF and v_hi == int(s[n - 1 - kk].item()) & 0xFFFFFFFF
    assert ctx.check(t)[1:] == before[1:]
