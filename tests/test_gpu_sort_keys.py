"""GPU tests of the typed, two-way sort (msd_sort_keys, msd_sort_pairs_keys, msd_reverse of include/msd_sort_keys_hip.h;
MsdContext.sort_typed / reverse).

The expected order is defined HERE with numpy: bit patterns -> order-preserving unsigned codes (np_encode of
tests/sort_rows_expect.py), np.sort, decode; descending is that array reversed.  Results are compared BITWISE through
integer views; inputs without NaN and -0 are also compared with np.sort of the typed array.  The two counters are compared
with the table of the header, computed here from the input's sign bits alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import guardband
from gpu_support import dev
from sort_rows_expect import NAMES, VIEWS, float_specials, make_float, make_int, np_decode, np_encode

pytestmark = pytest.mark.gpu

U32, I32, F32, U64, I64, F64 = range(6)
KEY_TYPES = [U32, I32, F32, U64, I64, F64]
TILE = {4: 4092, 8: 2046}   # elements a workgroup of reverse_ranges_kernel takes from each end (RevCfg<E>::TILE)
EINVAL = -1


def test_tile_constant_is_the_bindings(ctx):
    assert ctx.REVERSE_TILE == TILE


# ---- the expectation

def expected_bits(bits, kt, descending):
    a = bits.view(VIEWS[kt][1])
    S = np_decode(np.sort(np_encode(bits, kt)), kt)
    f = a if kt % 3 == 2 else None
    if f is None or not (np.isnan(f).any() or (np.signbit(f) & (f == 0)).any()):
        assert (S == np.sort(a).view(bits.dtype)).all(), "the codes' order is not numpy's order of the typed array"
    return S[::-1].copy() if descending else S


def expected_counters(bits, kt, descending):
    """(sort_keys_split, sort_keys_reversed): the table of include/msd_sort_keys_hip.h"""
    n = len(bits)
    top = bits.dtype.type(1 << (bits.itemsize * 8 - 1))
    kind = kt % 3
    P = n if kind == 0 else int(np.count_nonzero((bits & top) == 0))
    N = n - P
    R = lambda a, b: b - a if b - a >= 2 else 0  # noqa: E731
    if kind == 0:
        rev = R(0, n) if descending else 0
    elif kind == 1:
        rev = R(0, P) + R(P, n) if descending else (0 if N == 0 or P == 0 else R(0, n) + R(0, N) + R(N, n))
    else:
        rev = R(0, P) if descending else (0 if N == 0 else R(0, n) if P == 0 else R(0, n) + R(N, n))
    return P, rev


def stat(ctx, name):
    v = C.c_uint64()
    assert ctx._L.msd_stat(ctx._h, name.encode(), C.byref(v)) == 0, name
    return int(v.value)


def up(bits):
    """bit patterns (unsigned numpy array) -> a device tensor of the signed integer type of that width"""
    return dev(bits.view(np.int32 if bits.itemsize == 4 else np.int64))


def sort_keys(ctx, t, kt, order):
    return ctx._L.msd_sort_keys(ctx._h, C.c_void_p(t.data_ptr()), kt, t.numel(), order)


def check_sort(ctx, bits, kt, what=""):
    """both directions of one input (bit patterns, unsigned numpy array): the order and the two counters"""
    asc = expected_bits(bits, kt, False)
    for descending in (False, True):
        t = up(bits)
        assert sort_keys(ctx, t, kt, int(descending)) == 0, ctx._L.msd_last_error(ctx._h)
        got = t.cpu().numpy().view(bits.dtype)
        exp = asc[::-1] if descending else asc
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"{what} {NAMES[kt]} descending={descending}: {bad.size} keys differ, first at {bad[0]}: {got[bad[0]]:#x} != {exp[bad[0]]:#x}"
        P, rev = expected_counters(bits, kt, descending)
        assert (stat(ctx, "sort_keys_split"), stat(ctx, "sort_keys_reversed")) == (P, rev), f"{what} {NAMES[kt]} descending={descending}"


# ---- inputs: random bit patterns with exactly s keys that have the sign bit

@functools.lru_cache(maxsize=None)
def base_bits(width, n):
    rng = np.random.default_rng(1000 * width + n % 997)
    ut = np.uint32 if width == 4 else np.uint64
    b = rng.integers(0, np.iinfo(ut).max, n, dtype=ut, endpoint=True)
    where = rng.permutation(n)
    b.setflags(write=False)
    where.setflags(write=False)
    return b, where


def bits_with_signs(width, n, s):
    b, where = base_bits(width, n)
    top = b.dtype.type(1 << (width * 8 - 1))
    out = b & ~top
    out[where[:s]] |= top
    if n >= 16:           # duplicates at both ends of the list of positions: equal low bits, each key keeps its sign
        for dup, src in ((where[n - 4:], where[n - 5]), (where[1:3], where[0])):
            out[dup] = (out[dup] & top) | (out[src] & ~top)
    return out


SIZES = [0, 1, 2, 3, 5, 64, 65, 257, 1025, 4099, (1 << 16) + 1, (1 << 20) + 7, (1 << 22) + 13]   # (the last reaches the sort's direct rounds)


def sign_counts(n):
    return sorted({s for s in (0, 1, 2, 3, n // 2, n - 3, n - 1, n) if 0 <= s <= n})


LARGE_FROM = 1 << 20   # from here on one test case per sign count (test_every_split_large)


@pytest.mark.parametrize("n", [n for n in SIZES if n < LARGE_FROM])
@pytest.mark.parametrize("kt", KEY_TYPES, ids=[NAMES[k] for k in KEY_TYPES])
def test_every_split_small(ctx, kt, n):
    width = 4 if kt < U64 else 8
    for s in sign_counts(n):
        bits = bits_with_signs(width, n, s)
        top = bits.dtype.type(1 << (width * 8 - 1))
        assert np.count_nonzero(bits & top) == s
        check_sort(ctx, bits, kt, f"n={n} signs={s}")


LARGE = [(n, i) for n in SIZES if n >= LARGE_FROM for i in range(8)]


@pytest.mark.parametrize("n,which", LARGE, ids=[f"{n}-s{i}" for n, i in LARGE])
@pytest.mark.parametrize("kt", KEY_TYPES, ids=[NAMES[k] for k in KEY_TYPES])
def test_every_split_large(ctx, kt, n, which):
    width = 4 if kt < U64 else 8
    s = sign_counts(n)[which]
    check_sort(ctx, bits_with_signs(width, n, s), kt, f"n={n} signs={s}")


FLOAT_KINDS = ["bits", "normal", "specials", "const", "sorted", "reverse"]
INT_KINDS = ["bits", "small", "const", "sorted", "reverse"]


@pytest.mark.parametrize("n", [5, 1025, (1 << 16) + 1])
@pytest.mark.parametrize("kt", KEY_TYPES, ids=[NAMES[k] for k in KEY_TYPES])
def test_input_kinds(ctx, kt, n):
    ut, tt = VIEWS[kt]
    for i, kind in enumerate(FLOAT_KINDS if kt % 3 == 2 else INT_KINDS):
        if kt % 3 == 2:
            a = make_float(n, kind, tt, 77 + i)
        else:   # (unsigned key types get the signed generators' bit patterns)
            a = make_int(n, kind, np.int32 if ut == np.uint32 else np.int64, 77 + i)
        check_sort(ctx, np.ascontiguousarray(a).view(ut).copy(), kt, f"{kind} n={n}")


def test_all_float_specials(ctx):
    for kt, tt in ((F32, np.float32), (F64, np.float64)):
        a = np.tile(float_specials(tt), 3)
        check_sort(ctx, np.random.default_rng(5).permutation(a).view(VIEWS[kt][0]).copy(), kt, "specials")


def test_nothing_moves_where_the_table_says_nothing(ctx):
    rng = np.random.default_rng(11)
    n = 3 * TILE[4] + 17
    for kt, bits in ((F32, rng.random(n, dtype=np.float32).view(np.uint32)), (I32, rng.integers(0, 1 << 31, n, dtype=np.int32).view(np.uint32)),
                     (F64, rng.random(n).view(np.uint64)), (I64, rng.integers(0, 1 << 62, n, dtype=np.int64).view(np.uint64)),
                     (U32, rng.integers(0, 1 << 32, n, dtype=np.uint32)), (U64, rng.integers(0, 1 << 64, n, dtype=np.uint64))):
        t = up(bits)
        assert sort_keys(ctx, t, kt, 0) == 0
        assert stat(ctx, "sort_keys_reversed") == 0 and stat(ctx, "sort_keys_split") == n
        assert (t.cpu().numpy().view(bits.dtype) == np.sort(bits)).all()
        if kt % 3 == 2:   # floats descending: exactly the non-negative block
            t = up(bits)
            assert sort_keys(ctx, t, kt, 1) == 0
            assert stat(ctx, "sort_keys_reversed") == n and stat(ctx, "sort_keys_split") == n


# ---- msd_reverse alone

def _counts(es):
    T = TILE[es]
    return [0, 1, 2, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 4 * T + 3, (1 << 22) + 13]


REVERSE_CASES = [(es, c) for es in (4, 8) for c in _counts(es)]


@pytest.mark.parametrize("es,count", REVERSE_CASES, ids=[f"{es}B-{c}" for es, c in REVERSE_CASES])
def test_reverse(ctx, es, count):
    import torch
    dt = torch.int32 if es == 4 else torch.int64
    for first in (0, 1, 2, 3, 5):
        total = first + count + 7
        t = torch.arange(total, dtype=dt, device="cuda")
        assert ctx._L.msd_reverse(ctx._h, C.c_void_p(t.data_ptr()), es, first, count) == 0
        exp = torch.arange(total, dtype=dt, device="cuda")
        exp[first:first + count] = torch.arange(first + count - 1, first - 1, -1, dtype=dt, device="cuda")
        bad = torch.nonzero(t != exp).flatten()
        assert bad.numel() == 0, f"first={first} count={count}: {bad.numel()} wrong, first at {int(bad[0])}: holds {int(t[bad[0]])}"


def test_reverse_of_an_element_aligned_view(ctx):
    import torch
    for dt in (torch.int32, torch.float32, torch.int64, torch.float64):
        base = torch.arange(3 * 4092 + 50, device="cuda").to(dt)
        for off in (1, 2, 3):
            t = base.clone()
            v = t[off:]                         # its address is only element aligned
            ctx.reverse(v, 1, v.numel() - 2)
            exp = base.clone()
            exp[off + 1:off + v.numel() - 1] = base[off + 1:off + v.numel() - 1].flip(0)
            assert torch.equal(t, exp), (dt, off)
            ctx.reverse(v)                      # defaults: the whole tensor
            exp[off:] = exp[off:].flip(0)
            assert torch.equal(t, exp), (dt, off)


# ---- tuples

@pytest.mark.parametrize("n", [0, 1, 2, 5, 4099, (1 << 16) + 1, (1 << 20) + 7])
@pytest.mark.parametrize("kt", [U64, I64, F64], ids=["u64", "i64", "f64"])
def test_pairs(ctx, kt, n):
    import torch
    rng = np.random.default_rng(n + kt)
    inputs = [bits_with_signs(8, n, n // 2)]
    if n >= 5:   # many equal keys around zero: ties on both sides of the sign
        small = rng.integers(-3, 4, n).astype(np.int64)
        inputs.append((small.astype(np.float64) if kt == F64 else small).view(np.uint64).copy())
    for bits in inputs:
        for descending in (False, True):
            keys = dev(bits.view(np.int64))
            rids = torch.arange(n, dtype=torch.int64, device="cuda")
            rc = ctx._L.msd_sort_pairs_keys(ctx._h, C.c_void_p(keys.data_ptr()), kt, C.c_void_p(rids.data_ptr()), n, int(descending))
            assert rc == 0, ctx._L.msd_last_error(ctx._h)
            got, r = keys.cpu().numpy().view(np.uint64), rids.cpu().numpy()
            assert (got == expected_bits(bits, kt, descending)).all(), (NAMES[kt], n, descending)
            assert (np.sort(r) == np.arange(n)).all(), "the rids are not a permutation"
            assert (bits[r] == got).all(), "a rid did not move with its key"
            assert (stat(ctx, "sort_keys_split"), stat(ctx, "sort_keys_reversed")) == expected_counters(bits, kt, descending)


# ---- guard bands: nothing outside the buffers is written

@pytest.mark.parametrize("lead", [0, 16])
@pytest.mark.parametrize("neighbours", ["low", "high"])
def test_guard_bands_keys(ctx, neighbours, lead):
    import torch
    for kt, dt in ((I32, torch.int32), (F32, torch.float32), (U32, torch.int32), (I64, torch.int64), (F64, torch.float64)):
        es = 4 if kt < U64 else 8
        for n in (1, 3, 2 * TILE[es] + 5, 5 * TILE[es] + 1):
            for descending in (False, True):
                bits = bits_with_signs(es, n, n // 3)
                A = guardband.Arena(dt, n, lead_bytes=lead, guard=2 * TILE[es], neighbours=neighbours).fill(bits)
                assert ctx._L.msd_sort_keys(ctx._h, C.c_void_p(A.ptr), kt, n, int(descending)) == 0
                A.check(f"msd_sort_keys {NAMES[kt]} n={n} descending={descending}")
                assert (A.host(bits.dtype) == expected_bits(bits, kt, descending)).all()


@pytest.mark.parametrize("lead", [0, 16])
@pytest.mark.parametrize("neighbours", ["low", "high"])
def test_guard_bands_pairs(ctx, neighbours, lead):
    import torch
    for kt in (I64, F64, U64):
        for n in (3, 2 * TILE[8] + 5):
            for descending in (False, True):
                bits = bits_with_signs(8, n, n // 3)
                K = guardband.Arena(torch.int64, n, lead_bytes=lead, guard=2 * TILE[8], neighbours=neighbours).fill(bits)
                R = guardband.Arena(torch.int64, n, lead_bytes=lead, guard=2 * TILE[8], neighbours=neighbours).fill(np.arange(n, dtype=np.int64))
                assert ctx._L.msd_sort_pairs_keys(ctx._h, C.c_void_p(K.ptr), kt, C.c_void_p(R.ptr), n, int(descending)) == 0
                K.check(f"keys {NAMES[kt]} n={n}")
                R.check(f"rids {NAMES[kt]} n={n}")
                assert (K.host(np.uint64) == expected_bits(bits, kt, descending)).all()
                assert (bits[R.host(np.int64)] == K.host(np.uint64)).all()


@pytest.mark.parametrize("lead", [0, 16])
@pytest.mark.parametrize("neighbours", ["low", "high"])
def test_guard_bands_reverse(ctx, neighbours, lead):
    import torch
    for es, dt in ((4, torch.int32), (8, torch.int64)):
        T = TILE[es]
        for n in (2, 5, T + 1, 2 * T, 4 * T + 3):
            for first, count in ((0, n), (0, max(n - 3, 0)), (min(3, n), n - min(3, n))):   # first = 0; first + count = n
                a = np.arange(n, dtype=np.int32 if es == 4 else np.int64)
                A = guardband.Arena(dt, n, lead_bytes=lead, guard=2 * T, neighbours=neighbours).fill(a)
                assert ctx._L.msd_reverse(ctx._h, C.c_void_p(A.ptr), es, first, count) == 0
                A.check(f"msd_reverse {es}B n={n} [{first},{first + count})")
                a[first:first + count] = a[first:first + count][::-1].copy()
                assert (A.host(a.dtype) == a).all()


# ---- refusals: MSD_EINVAL, nothing touched

def test_refusals(ctx):
    import torch
    L, h = ctx._L, ctx._h
    n = 1000
    src = torch.arange(n + 8, dtype=torch.int64, device="cuda").flip(0).contiguous()
    keys, rids = src.clone(), src.clone()
    kp, rp = keys.data_ptr(), rids.data_ptr()
    p = C.c_void_p
    refused = [
        L.msd_sort_keys(h, None, F32, n, 0),                              # null pointer
        L.msd_sort_keys(h, p(kp), 6, n, 0), L.msd_sort_keys(h, p(kp), -1, n, 0),       # unknown key type
        L.msd_sort_keys(h, p(kp), F32, n, 2), L.msd_sort_keys(h, p(kp), F32, n, -1),   # unknown order
        L.msd_sort_keys(h, p(kp + 4), F32, n, 0), L.msd_sort_keys(h, p(kp + 8), F64, n, 1),   # not 16-byte aligned
        L.msd_sort_pairs_keys(h, None, I64, p(rp), n, 0), L.msd_sort_pairs_keys(h, p(kp), I64, None, n, 0),
        L.msd_sort_pairs_keys(h, p(kp), 7, p(rp), n, 0), L.msd_sort_pairs_keys(h, p(kp), I64, p(rp), n, 3),
        L.msd_sort_pairs_keys(h, p(kp), U32, p(rp), n, 0), L.msd_sort_pairs_keys(h, p(kp), I32, p(rp), n, 0),
        L.msd_sort_pairs_keys(h, p(kp), F32, p(rp), n, 1),                # a 32-bit key type
        L.msd_sort_pairs_keys(h, p(kp + 8), F64, p(rp), n, 0), L.msd_sort_pairs_keys(h, p(kp), F64, p(rp + 8), n, 0),
        L.msd_sort_pairs_keys(h, p(kp), I64, p(kp), n, 0),                # overlap: the same array
        L.msd_sort_pairs_keys(h, p(kp), I64, p(kp + 16), n // 2, 0),      # overlap: shifted
        L.msd_reverse(h, None, 4, 0, 10),
        L.msd_reverse(h, p(kp), 2, 0, 10), L.msd_reverse(h, p(kp), 16, 0, 10), L.msd_reverse(h, p(kp), 0, 0, 10),
        L.msd_reverse(h, p(kp + 4), 8, 0, 10),                            # not element aligned
        L.msd_reverse(h, p(kp), 4, (1 << 64) - 5, 10),                    # first + count overflows
        L.msd_reverse(h, p(kp), 8, 1 << 62, 1 << 62),                     # ... as a byte offset
    ]
    assert refused == [EINVAL] * len(refused), refused
    assert ctx._L.msd_last_error(h)
    torch.cuda.synchronize()
    assert torch.equal(keys, src) and torch.equal(rids, src)
    # successful no-ops
    assert L.msd_sort_keys(h, None, F32, 0, 0) == 0 and L.msd_sort_keys(h, p(kp), I64, 1, 1) == 0
    assert L.msd_sort_pairs_keys(h, None, F64, None, 0, 1) == 0 and L.msd_sort_pairs_keys(h, p(kp), F64, p(rp), 1, 1) == 0
    assert L.msd_reverse(h, None, 4, 0, 0) == 0 and L.msd_reverse(h, p(kp), 8, 7, 1) == 0 and L.msd_reverse(h, p(kp), 4, 7, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(keys, src) and torch.equal(rids, src)


def test_null_context_is_refused_first():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    assert L.msd_sort_keys(None, None, 99, 10, 99) == EINVAL
    assert L.msd_sort_pairs_keys(None, None, 99, None, 10, 99) == EINVAL
    assert L.msd_reverse(None, None, 3, 1, 10) == EINVAL


# ---- phases and the Python wrapper

def test_phase_sort_fixup(ctx):
    bits = bits_with_signs(4, 4099, 2000)
    ctx.set_profiling(True)
    try:
        t = dev(bits.view(np.float32))
        ctx.sort_typed(t)
        names = [p for p, _ in ctx.phases()]
        assert "sort_fixup" in names and len(names) > 1, names
        u = up(bits)
        ctx.sort_u32(u)
        assert "sort_fixup" not in [p for p, _ in ctx.phases()]
    finally:
        ctx.set_profiling(False)
    assert (t.cpu().numpy().view(np.uint32) == expected_bits(bits, F32, False)).all()


@pytest.mark.parametrize("n", [3, 4099, (1 << 18) + 5])
def test_wrapper_against_torch_sort(ctx, n):
    import torch
    g = torch.Generator().manual_seed(n)
    for dt in (torch.float32, torch.int64, torch.float64):
        if dt.is_floating_point:
            x = torch.randn(n, generator=g, dtype=dt)
            x[x == 0] = 1.0                                          # (no -0, no NaN: torch.sort's order is then totalOrder)
        else:
            x = torch.randint(-(1 << 40), 1 << 40, (n,), generator=g, dtype=dt)
        for descending in (False, True):
            t = x.cuda()
            assert ctx.sort_typed(t, descending=descending) is None
            assert torch.equal(t.cpu(), torch.sort(x, descending=descending).values), (dt, descending)
            s = ctx.stats()
            assert "sort_keys_split" in s and "sort_keys_reversed" in s
        if dt != torch.float32:
            k, r = x.cuda(), torch.arange(n, dtype=torch.int64, device="cuda")
            ctx.sort_typed(k, descending=True, rids=r)
            assert torch.equal(k.cpu(), torch.sort(x, descending=True).values)
            assert torch.equal(x[r.cpu()], k.cpu())
