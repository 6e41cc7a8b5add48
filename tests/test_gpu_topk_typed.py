"""GPU tests of typed top-k / select (msd_topk_keys, msd_select_key; MsdContext.topk_typed / select_typed): signed and
float keys in their own order, with and without the positions of the keys.

The expected result is defined HERE: the keys' bit patterns are turned into order-preserving unsigned codes with the numpy
expressions of tests/sort_rows_expect.py (unsigned: the pattern; signed: value + 2^(W-1); float: positive -> sign bit set,
negative -> all bits inverted, i.e. IEEE-754 totalOrder), np.sort orders the codes, and the inverse map gives the sorted
bit patterns.  Inputs without NaN and without -0 are also compared with np.sort of the typed array itself.  Values are
compared BITWISE (integer views).  Indices are never compared with expected indices (ties make them unspecified), only
checked: in range, pointing at a key bit-equal to the value, no position twice."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEFAULTS, dev
from sort_rows_expect import F32, F64, I32, I64, U32, U64, VIEWS, make_float, make_int, np_decode, np_encode

pytestmark = pytest.mark.gpu

DEFAULT_CAP = DEFAULTS["select_cap"]  # the library's default "select_cap" (include/msd_radix_hip.h)


# ---- the expectation

def sorted_bits(a, kt):
    """the bit patterns of the typed array a in the ascending order of key type kt"""
    bits = np.ascontiguousarray(a).view(VIEWS[kt][0])
    S = np_decode(np.sort(np_encode(bits, kt)), kt)
    f = a if kt % 3 == 2 else None
    if f is None or not (np.isnan(f).any() or (np.signbit(f) & (f == 0)).any()):
        assert (S == np.sort(a).view(VIEWS[kt][0])).all(), "the codes' order is not numpy's order of the typed array"
    return S


def k_list(n):  # (as tests/test_gpu_topk.py)
    return sorted({k for k in (0, 1, 2, n // 1000 + 1, n // 2, n - 1, n) if 0 <= k <= n})


# ---- the check

def host_bits(t, kt):
    return t.cpu().numpy().view(VIEWS[kt][0])


def select_bits(ctx, t, kt, kk, largest):
    """msd_select_key itself: the value's bit pattern"""
    v = (C.c_uint32 if t.element_size() == 4 else C.c_uint64)()
    ctx._ok(ctx._L.msd_select_key(ctx._h, ctx._ptr(t, t.element_size()), kt, t.numel(), kk, 1 if largest else 0, C.byref(v)))
    return int(v.value)


def check_indices(bits, idx, vals_bits, kk):
    n = len(bits)
    assert idx.dtype == np.int64 and len(idx) == kk
    assert ((idx >= 0) & (idx < n)).all()
    assert (bits[idx] == vals_bits).all(), "a position does not hold the value written next to it"
    assert len(np.unique(idx)) == kk, "an input position was used twice"


def check_typed(ctx, a, kt, ks=None):
    """top-k (with and without indices) and select of the typed array a for every k of the list and both directions"""
    import math
    ut, tt = VIEWS[kt]
    n = len(a)
    bits = np.ascontiguousarray(a).view(ut)
    S = sorted_bits(a, kt)
    t = dev(a)
    for kk in (k_list(n) if ks is None else ks):
        for largest in (False, True):
            want = S[n - kk:] if largest else S[:kk]
            out = ctx.topk_typed(t, kk, largest=largest)
            assert out.dtype == t.dtype and out.numel() == kk
            assert (host_bits(out, kt) == want).all(), (n, kk, largest, "values")
            vals, idx = ctx.topk_typed(t, kk, largest=largest, indices=True)
            assert vals.dtype == t.dtype and vals.numel() == kk
            hv = host_bits(vals, kt)
            assert (hv == want).all(), (n, kk, largest, "values with indices")
            check_indices(bits, idx.cpu().numpy(), hv, kk)
            if kk < n:
                wb = S[n - 1 - kk] if largest else S[kk]
                assert select_bits(ctx, t, kt, kk, largest) == int(wb), (n, kk, largest, "select")
                v = ctx.select_typed(t, kk, largest=largest)
                we = np.array([wb], ut).view(tt)[0]
                if kt % 3 == 2:
                    assert isinstance(v, float)
                    if np.isnan(we):
                        assert math.isnan(v) and (math.copysign(1.0, v) < 0) == bool(np.signbit(we))
                    else:
                        assert np.array([v], tt).view(ut)[0] == wb, (v, we)
                else:
                    assert isinstance(v, int) and v == int(we)
    assert (host_bits(t, kt) == bits).all(), "the input was modified"


SIZES = [1, 2, 64, 65, 4097, 70001, 1 << 20, (1 << 21) + 77]
SIZES64 = [1, 65, 70001, (1 << 20) + 7]
FLOAT_KINDS = ["normal", "bits", "specials", "const", "negative", "sorted", "reverse", "coarse"]
INT_KINDS = ["bits", "small", "const", "extremes", "sorted", "reverse"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", FLOAT_KINDS)
def test_f32(ctx, n, kind):
    check_typed(ctx, make_float(n, kind, np.float32, seed=n % 97 + 1), F32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", INT_KINDS)
def test_i32(ctx, n, kind):
    check_typed(ctx, make_int(n, kind, np.int32, seed=n % 97 + 1), I32)


@pytest.mark.parametrize("n", SIZES64)
@pytest.mark.parametrize("kind", FLOAT_KINDS)
def test_f64(ctx, n, kind):
    check_typed(ctx, make_float(n, kind, np.float64, seed=n % 97 + 2), F64)


@pytest.mark.parametrize("n", SIZES64)
@pytest.mark.parametrize("kind", INT_KINDS)
def test_i64(ctx, n, kind):
    check_typed(ctx, make_int(n, kind, np.int64, seed=n % 97 + 2), I64)


def test_specials_really_contain_the_special_values():
    for tt in (np.float32, np.float64):
        a = make_float(70001, "specials", tt, seed=3)
        assert np.isnan(a).sum() >= 50 and np.isinf(a).sum() >= 10 and ((a == 0) & np.signbit(a)).sum() >= 5
    assert np.isnan(make_float(70001, "bits", np.float32, seed=3)).any()  # (a random f32 pattern is a NaN once in 128)


# ---- the deep paths with typed keys

N_DEEP = (1 << 21) + 77


@pytest.mark.parametrize("cap", [4096, 1])
@pytest.mark.parametrize("n", [70001, N_DEEP])
@pytest.mark.parametrize("kind", ["normal", "coarse", "const", "bits"])
def test_deep_paths_f32(ctx, cap, n, kind):
    try:
        ctx.set_option("select_cap", cap)
        check_typed(ctx, make_float(n, kind, np.float32, seed=5), F32)
    finally:
        ctx.set_option("select_cap", DEFAULT_CAP)


@pytest.mark.parametrize("cap", [4096, 1])
@pytest.mark.parametrize("kt", [I32, F64, I64])
def test_deep_paths_other_types(ctx, cap, kt):
    tt = VIEWS[kt][1]
    try:
        ctx.set_option("select_cap", cap)
        for kind in ("bits", "const") + (("normal", "coarse") if kt == F64 else ("small",)):
            a = make_float(70001, kind, tt, seed=6) if kt == F64 else make_int(70001, kind, tt, seed=6)
            check_typed(ctx, a, kt)
    finally:
        ctx.set_option("select_cap", DEFAULT_CAP)


def test_stats_normal_scores_need_a_second_histogram_pass(ctx):
    """N(0,1) float32 at rank n/4 (|x| about 0.67): the pivot's 12-bit bucket (sign, exponent, 3 mantissa bits) holds about
    2 % of the keys, ten times a cap of 4096.  const: the bits run out (exhausted path), every key is a candidate."""
    a = make_float(N_DEEP, "normal", np.float32, seed=1)
    S = sorted_bits(a, F32)
    t = dev(a)
    kk = N_DEEP // 4
    try:
        ctx.set_option("select_cap", 4096)
        for largest in (False, True):
            out = ctx.topk_typed(t, kk, largest=largest)
            st = ctx.stats()
            assert (host_bits(out, F32) == (S[N_DEEP - kk:] if largest else S[:kk])).all()
            assert st["select_hist_passes"] >= 2, (largest, st)
            assert st["select_below"] < kk <= st["select_below"] + st["select_candidates"], st
            vals, idx = ctx.topk_typed(t, kk, largest=largest, indices=True)
            assert ctx.stats()["select_hist_passes"] >= 2
            check_indices(a.view(np.uint32), idx.cpu().numpy(), host_bits(vals, F32), kk)
        c = make_float(N_DEEP, "const", np.float32, seed=1)
        tc = dev(c)
        for largest in (False, True):
            for with_idx in (False, True):
                r = ctx.topk_typed(tc, kk, largest=largest, indices=with_idx)
                st = ctx.stats()
                assert st["select_candidates"] == N_DEEP and st["select_below"] == 0, st
                vals = r[0] if with_idx else r
                assert (host_bits(vals, F32) == c.view(np.uint32)[:kk]).all()
                if with_idx:
                    check_indices(c.view(np.uint32), r[1].cpu().numpy(), host_bits(vals, F32), kk)
    finally:
        ctx.set_option("select_cap", DEFAULT_CAP)


def test_finish_phase_is_reported(ctx):
    t = dev(make_float(1 << 20, "normal", np.float32, seed=2))
    try:
        ctx.set_profiling(True)
        ctx.topk_typed(t, 1000, indices=True)
        names = [p[0] for p in ctx.phases()]
    finally:
        ctx.set_profiling(False)
    assert "select_hist" in names and "select_filter" in names and "select_finish" in names, names


# ---- unsigned key types through the new entry point

def _topk_keys(ctx, t, kt, kk, largest, with_idx):
    import torch
    es = t.element_size()
    out = torch.empty(kk, dtype=t.dtype, device="cuda")
    idx = torch.empty(kk, dtype=torch.int64, device="cuda") if with_idx else None
    ctx._ok(ctx._L.msd_topk_keys(ctx._h, ctx._ptr(t, es), kt, t.numel(), kk, 1 if largest else 0, ctx._ptr(out, es),
                                 ctx._ptr(idx, 8) if with_idx else None))
    return out, idx


@pytest.mark.parametrize("kt,n", [(U32, 70001), (U32, (1 << 21) + 77), (U64, 70001), (U64, (1 << 20) + 7)])
def test_unsigned_key_types_equal_topk(ctx, kt, n):
    import torch
    ut = VIEWS[kt][0]
    rng = np.random.default_rng(n)
    bits = rng.integers(0, np.iinfo(ut).max, n, dtype=ut, endpoint=True)
    bits[::7] = bits[0]  # (duplicates)
    t = dev(bits.view(np.int32 if kt == U32 else np.int64))  # (an int tensor carries the unsigned bits, as for ctx.topk)
    S = np.sort(bits)
    for kk in k_list(n):
        for largest in (False, True):
            ref = ctx.topk(t, kk, largest=largest)
            out, _ = _topk_keys(ctx, t, kt, kk, largest, False)
            assert torch.equal(out, ref)
            assert (host_bits(out, kt) == (S[n - kk:] if largest else S[:kk])).all()
            out, idx = _topk_keys(ctx, t, kt, kk, largest, True)
            assert torch.equal(out, ref)
            check_indices(bits, idx.cpu().numpy(), host_bits(out, kt), kk)
            if kk < n:
                assert select_bits(ctx, t, kt, kk, largest) == ctx.select(t, kk, largest=largest)
    assert (host_bits(t, kt) == bits).all()
    name = "uint32" if kt == U32 else "uint64"
    if hasattr(torch, name):  # this torch has the unsigned dtype: the dtype dispatch takes it
        tu = t.view(getattr(torch, name))
        kk = n // 3
        vals, idx = ctx.topk_typed(tu, kk, largest=True, indices=True)
        assert vals.dtype == tu.dtype
        assert (vals.cpu().numpy().view(ut) == S[n - kk:]).all()
        check_indices(bits, idx.cpu().numpy(), vals.cpu().numpy().view(ut), kk)
        assert ctx.select_typed(tu, kk) == int(S[kk])


# ---- arguments

def test_bad_arguments_are_refused_and_touch_nothing(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdError
    n = 5000
    a = make_float(n, "normal", np.float32, seed=9)
    t = dev(a)
    out = torch.full((n + 8,), 1.5, dtype=torch.float32, device="cuda")
    idx = torch.full((n + 8,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    out0, idx0 = out.clone(), idx.clone()
    L, h, p = ctx._L, ctx._h, ctx._ptr

    def refused(f):
        with pytest.raises(MsdError) as e:
            f()
        assert "error -1" in str(e.value), str(e.value)  # MSD_EINVAL and its message
        assert len(str(e.value)) > len("error -1: ")
        assert (host_bits(t, F32) == a.view(np.uint32)).all() and torch.equal(out, out0) and torch.equal(idx, idx0)

    def topk(keys=None, kt=F32, nn=n, kk=100, which=0, o=None, i=None):
        keys = p(t, 4) if keys is None else keys
        return lambda: ctx._ok(L.msd_topk_keys(h, keys, kt, nn, kk, which, p(out, 4) if o is None else o, i))

    assert L.msd_topk_keys(None, p(t, 4), F32, n, 100, 0, p(out, 4), p(idx, 8)) == -1   # null context
    v = C.c_uint32(77)
    assert L.msd_select_key(None, p(t, 4), F32, n, 1, 0, C.byref(v)) == -1 and v.value == 77
    assert torch.equal(out, out0) and torch.equal(idx, idx0)
    refused(topk(keys=C.c_void_p(0)))                                  # null input
    refused(topk(o=C.c_void_p(0)))                                     # null output
    refused(topk(o=C.c_void_p(0), i=p(idx, 8)))
    refused(topk(kk=n + 1))                                            # k > n
    refused(topk(kk=n + 1, i=p(idx, 8)))
    refused(lambda: ctx.select_typed(t, n))                            # k >= n
    refused(lambda: ctx.select_typed(t, n + 5, largest=True))
    refused(topk(which=2))                                             # unknown which
    refused(topk(which=-1, i=p(idx, 8)))
    refused(lambda: ctx._ok(L.msd_select_key(h, p(t, 4), F32, n, 1, 2, C.byref(v))))
    refused(topk(kt=6))                                                # unknown key type
    refused(topk(kt=-1, i=p(idx, 8)))
    refused(lambda: ctx._ok(L.msd_select_key(h, p(t, 4), 6, n, 1, 0, C.byref(v))))
    refused(lambda: ctx._ok(L.msd_select_key(h, p(t, 4), F32, n, 1, 0, None)))     # null result pointer
    assert v.value == 77
    refused(lambda: ctx.topk_typed(t[1:], 100))                        # misaligned input (a view offset by one element)
    refused(lambda: ctx.topk_typed(t, 100, out=out[1:]))               # misaligned output
    refused(lambda: ctx.topk_typed(t, 100, out=out, out_indices=idx[1:]))   # misaligned indices (8 bytes off)
    refused(lambda: ctx.topk_typed(t, 100, out=out[1:], out_indices=idx))
    refused(lambda: ctx.topk_typed(t, 100, out=t[:100]))               # the values alias the input
    refused(lambda: ctx.topk_typed(t, 100, out=t[n - 100:n]))
    refused(lambda: ctx.topk_typed(t, 100, out=t[:100], out_indices=idx))
    refused(lambda: ctx.topk_typed(t, 100, out=out, out_indices=t.view(torch.int64)[:100]))      # the indices alias the input
    refused(lambda: ctx.topk_typed(t, 100, out=idx.view(torch.float32)[:100], out_indices=idx))  # the two outputs overlap
    refused(lambda: ctx.topk_typed(t, 100, out=idx.view(torch.float32)[100:200], out_indices=idx))
    # 64-bit key types: the same rules
    a64 = make_float(n, "normal", np.float64, seed=9)
    t64 = dev(a64)
    o64 = torch.full((n + 8,), 2.5, dtype=torch.float64, device="cuda")
    o64_0 = o64.clone()
    for f in (lambda: ctx.topk_typed(t64, 100, out=o64[:100], out_indices=o64.view(torch.int64)[50:150]),
              lambda: ctx.topk_typed(t64, 100, out=t64[:100], out_indices=idx),
              lambda: ctx.topk_typed(t64, 100, out=o64, out_indices=t64.view(torch.int64)[200:300]),
              lambda: ctx.topk_typed(t64, 100, out=o64[1:], out_indices=idx),
              lambda: ctx.topk_typed(t64, n + 1, out=o64, out_indices=idx),
              lambda: ctx.select_typed(t64, n)):
        refused(f)
        assert (host_bits(t64, F64) == a64.view(np.uint64)).all() and torch.equal(o64, o64_0)
    # a dtype without a key order never reaches the library
    with pytest.raises(MsdError):
        ctx.topk_typed(t.to(torch.float16), 10)
    # k == 0 and n == 0: success, nothing touched
    assert ctx.topk_typed(t, 0).numel() == 0
    ctx.topk_typed(t, 0, out=out, out_indices=idx)
    e, ei = ctx.topk_typed(t, 0, indices=True)
    assert e.numel() == 0 and ei.numel() == 0 and ei.dtype == torch.int64
    z = torch.empty(0, dtype=torch.float32, device="cuda")
    assert ctx.topk_typed(z, 0).numel() == 0
    zv, zi = ctx.topk_typed(z, 0, indices=True)
    assert zv.numel() == 0 and zi.numel() == 0
    assert ctx.topk_typed(torch.empty(0, dtype=torch.int64, device="cuda"), 0, indices=True)[0].numel() == 0
    assert torch.equal(out, out0) and torch.equal(idx, idx0) and (host_bits(t, F32) == a.view(np.uint32)).all()


def test_indices_of_32_bit_keys_need_n_up_to_2_32(ctx):
    """n = 2^32 + 16 float32 keys (17 GB, not initialised; the buffer really has that size), indices requested: refused
    before any launch.  Without indices the same n is a valid call (not made here: 17 GB of noise to order)."""
    import torch
    from inplacemsdradixsort_amd import MsdError
    n, kk = 2**32 + 16, 16
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    assert t.numel() == n
    out = torch.full((kk,), 1.5, dtype=torch.float32, device="cuda")
    idx = torch.full((kk,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(MsdError) as e:
        ctx.topk_typed(t, kk, largest=True, out=out, out_indices=idx)
    assert "error -1" in str(e.value) and len(str(e.value)) > len("error -1: ")
    assert (out == 1.5).all() and (idx == -7).all()
    with pytest.raises(MsdError) as e:
        ctx.topk_typed(t.view(torch.int32), kk, out=out.view(torch.int32), out_indices=idx)
    assert "error -1" in str(e.value)
    assert (out == 1.5).all() and (idx == -7).all()
    del t
    torch.cuda.empty_cache()


# ---- larger than any leaf, once

def test_topk_2_28_normal_scores_against_torch_sort(ctx):
    import torch
    n, kk = 1 << 28, 1 << 16
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    t = torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    before = t.clone()
    s = torch.sort(t).values
    for largest in (False, True):
        vals, idx = ctx.topk_typed(t, kk, largest=largest, indices=True)
        torch.cuda.synchronize()
        assert torch.equal(vals, s[n - kk:] if largest else s[:kk])
        assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < n
        assert torch.equal(t[idx], vals)
        assert idx.unique().numel() == kk
        plain = ctx.topk_typed(t, kk, largest=largest)
        assert torch.equal(plain, vals)
    assert torch.equal(t, before), "the input was modified"
