"""GPU tests of per-row top-k (msd_topk_rows; MsdContext.topk_rows): the k smallest / largest keys of EVERY row of a matrix,
for all six key types, with and without the positions of the keys, through the one-launch row kernel and through the loop
over msd_topk_keys.

The expected result is defined HERE, as in tests/test_gpu_topk_typed.py: the keys' bit patterns are turned into
order-preserving unsigned codes with the numpy expressions of tests/sort_rows_expect.py, np.sort orders the codes along
axis 1, and the inverse map gives the sorted bit patterns.  Values are compared BITWISE, all rows and all k elements.
Indices are never compared with expected indices (ties make them unspecified), only checked: in [0, row_len), pointing at a
key of their own row that is bit-equal to the value beside them, no position twice within a row.  After every case the
input is compared with what was uploaded.

The calls go through the C ABI on integer tensors that carry the bit patterns (so that the unsigned key types, padded rows
and arbitrary alignment need nothing of torch); the Python wrapper has tests of its own at the end."""
import ctypes as C

import numpy as np
import pytest

import guardband
from gpu_support import DEFAULTS, int_dtype_of_key as int_dtype
from sort_rows_expect import F32, F64, I32, I64, NAMES, U32, U64, UT, float_specials, np_decode, np_encode, row_bits, row_normal

pytestmark = pytest.mark.gpu


SHAPES_IN = [(1, 1), (1, 70001), (3, 64), (1000, 65), (4096, 128), (100000, 8), (257, 4097), (64, 131072), (300, 50257), (3, 1 << 20)]
SHAPES_BEYOND = [(5, (1 << 20) + 77), (2, 1 << 22)]
SHAPES = SHAPES_IN + SHAPES_BEYOND
SMALL_ROWS = 300   # "small" shapes: the loop is affordable, and k = row_len is tried


# ---- the expectation

def sorted_rows(bits, kt):
    """every row of the bit patterns (rows x row_len) in the ascending order of key type kt"""
    codes = np_encode(bits, kt)
    codes.sort(axis=1)
    return np_decode(codes, kt)


def test_the_expectation_orders_like_numpy_where_numpy_has_an_order():
    rng = np.random.default_rng(1)
    f = rng.standard_normal((5, 999)).astype(np.float32)
    assert (sorted_rows(f.view(np.uint32), F32) == np.sort(f, axis=1).view(np.uint32)).all()
    i = rng.integers(-2**63, 2**63 - 1, (5, 999), dtype=np.int64)
    assert (sorted_rows(i.view(np.uint64), I64) == np.sort(i, axis=1).view(np.uint64)).all()
    u = i.view(np.uint64)
    assert (sorted_rows(u, U64) == np.sort(u, axis=1)).all()


# ---- inputs: row r is a function of (seed + r, column) and of a scale of its own

FLOAT_KINDS = ["normal", "bits", "specials", "const", "coarse", "sorted", "reverse", "rotated"]
INT_KINDS = ["bits", "small", "const", "extremes", "sorted", "reverse", "rotated"]


def make_rows(rows, n, kind, kt, seed):
    """rows x n bit patterns (unsigned view) of key type kt"""
    ut = UT[kt]
    W = 32 if ut == np.uint32 else 64
    if kind == "rotated":   # row r = row 0 rotated by r: a wrong row base or a mix-up between rows shows
        base = make_rows(1, n, "normal" if kt % 3 == 2 else "bits", kt, seed)[0]
        idx = (np.arange(n)[None, :] + np.arange(rows)[:, None]) % n
        return base[idx]
    if kt % 3 == 2:
        tt = np.float32 if W == 32 else np.float64
        if kind == "bits":
            return (row_bits(rows, n, seed) >> np.uint64(64 - W)).astype(ut)
        if kind == "const":   # every key of a row ties (another value in every row)
            return np.repeat((-1.5 * np.exp2(np.arange(rows) % 9)).astype(tt)[:, None], n, axis=1).view(ut)
        a = row_normal(rows, n, seed, tt)
        if kind == "specials":
            b = row_bits(rows, n, seed + 12345)
            sp = float_specials(tt)
            plant = (b % np.uint64(5)) == 0
            a = np.where(plant, sp[((b >> np.uint64(8)) % np.uint64(len(sp))).astype(np.int64)], a)
        elif kind == "coarse":
            a = (np.round(a * 16) / 16).astype(tt)
        elif kind == "sorted":
            a = np.sort(a, axis=1)
        elif kind == "reverse":
            a = np.sort(a, axis=1)[:, ::-1]
        elif kind != "normal":
            raise ValueError(kind)
        return np.ascontiguousarray(a).view(ut)
    b = (row_bits(rows, n, seed) >> np.uint64(64 - W)).astype(ut)
    signed = kt % 3 == 1
    if kind == "bits":
        return b
    if kind == "small":     # many ties, around zero
        v = (b % ut(4096)).astype(np.int64) - (2048 if signed else 0) + (np.arange(rows) % 9)[:, None]
        return v.astype(np.int64).astype(ut) if not signed else v.astype(np.int32 if W == 32 else np.int64).view(ut)
    if kind == "const":
        return np.repeat((ut(123456789) * (np.arange(rows, dtype=ut) + ut(1)))[:, None], n, axis=1)
    if kind == "extremes":
        top = 1 << (W - 1)
        table = np.array([top, top - 1, (1 << W) - 1, 0] if signed else [0, (1 << W) - 1, 1, top], dtype=ut)
        return table[(b % ut(4)).astype(np.int64)]
    st = np.sort(b.view(np.int32 if W == 32 else np.int64), axis=1).view(ut) if signed else np.sort(b, axis=1)
    if kind == "sorted":
        return st
    if kind == "reverse":
        return np.ascontiguousarray(st[:, ::-1])
    raise ValueError(kind)


def test_generated_rows_differ_and_specials_are_planted():
    a = make_rows(6, 999, "normal", F32, 1).view(np.float32)
    assert len({a[r].tobytes() for r in range(6)}) == 6
    assert a[0].std() < a[4].std() / 8                      # a scale per row
    s = make_rows(3, 5000, "specials", F64, 1).view(np.float64)
    assert np.isnan(s).sum() > 100 and np.isinf(s).sum() > 20 and ((s == 0) & np.signbit(s)).sum() > 10
    r = make_rows(5, 77, "rotated", I32, 1)
    assert (r[3] == np.roll(r[0], -3)).all()
    c = make_rows(4, 9, "const", U64, 1)
    assert (c == c[:, :1]).all() and len(set(c[:, 0].tolist())) == 4


# ---- the call and the checks

def limits(ctx, kt, with_idx):
    a, b = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_topk_rows_limits(kt, int(with_idx), C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def k_list(rows, row_len, max_k):
    ks = {0, 1, 2, row_len // 1000 + 1, min(row_len, max_k), max_k + 1}
    if rows <= SMALL_ROWS:
        ks.add(row_len)
    return sorted(k for k in ks if 0 <= k <= row_len)


def raw_call(ctx, in_ptr, kt, rows, row_len, stride, k, largest, out_ptr, idx_ptr):
    return ctx._L.msd_topk_rows(ctx._h, C.c_void_p(in_ptr), kt, rows, row_len, stride, k, 1 if largest else 0, C.c_void_p(out_ptr),
                                C.c_void_p(idx_ptr) if idx_ptr else None)


class Uploaded:
    """rows x row_len bit patterns on the device, `pad` elements of padding behind every row and `lead` in front of the
    first: the padding holds the two patterns that would win if they were read (the largest and the smallest key of the
    key type, alternating)."""

    def __init__(self, bits, kt, pad=0, lead=0):
        import torch
        self.bits, self.kt = bits, kt
        self.rows, self.row_len = bits.shape
        self.stride = self.row_len + pad
        ut = UT[kt]
        win = np_decode(np.array([np.iinfo(ut).max, 0], dtype=ut), kt)
        flat = np.empty(lead + self.rows * self.stride, ut)
        flat[0::2] = win[0]
        flat[1::2] = win[1]
        body = flat[lead:].reshape(self.rows, self.stride)
        body[:, :self.row_len] = bits
        self.flat = flat
        self.es = flat.itemsize
        self.t = torch.from_numpy(flat.view(np.int32 if self.es == 4 else np.int64)).cuda()
        self.ptr = self.t.data_ptr() + lead * self.es

    def unchanged(self):
        return (self.t.cpu().numpy().view(UT[self.kt]) == self.flat).all()


def check_result(up, S, k, largest, hv, hi):
    """hv: rows x k value bits from the device, hi: rows x k int64 positions or None"""
    rows, n = up.rows, up.row_len
    want = S[:, n - k:] if largest else S[:, :k]
    assert hv.shape == want.shape
    bad = np.nonzero((hv != want).any(axis=1))[0]
    assert bad.size == 0, (NAMES[up.kt], rows, n, k, largest, "values differ in %d rows, first %d" % (bad.size, bad[0] if bad.size else -1))
    if hi is None:
        return
    assert hi.dtype == np.int64 and hi.shape == want.shape
    assert ((hi >= 0) & (hi < n)).all(), "a position outside its row"
    assert (np.take_along_axis(up.bits, hi, axis=1) == hv).all(), "a position does not hold the value written next to it"
    flat = (hi + (np.arange(rows, dtype=np.int64) * n)[:, None]).ravel()
    assert np.bincount(flat, minlength=rows * n).max() <= 1, "an input position was used twice within a row"


def run_case(ctx, bits, kt, pad=0, lead=0, ks=None, modes=None):
    """every k of the list, both directions, with and without indices; modes: inside the envelope 2 (asserting that the
    kernel produced it), on small shapes 1 as well (asserting the loop, and equal values), and 0 always."""
    import torch
    up = Uploaded(bits, kt, pad, lead)
    rows, n = up.rows, up.row_len
    S = sorted_rows(bits, kt)
    it = int_dtype(kt)
    try:
        for with_idx in (False, True):
            max_len, max_k = limits(ctx, kt, with_idx)
            assert max_len >= 1 << 20 and max_k >= 1024
            for k in (k_list(rows, n, max_k) if ks is None else ks):
                inside = n <= max_len and k <= max_k
                todo = modes if modes is not None else ([2] if inside else []) + ([1] if inside and rows <= SMALL_ROWS else []) + [0]
                for largest in (False, True):
                    first = None
                    for mode in todo:
                        ctx.set_option("topk_rows_mode", mode)
                        out = torch.full((rows * k,), 0x5A5A5A5A, dtype=it, device="cuda")
                        idx = torch.full((rows * k,), -7, dtype=torch.int64, device="cuda") if with_idx else None
                        ctx._ok(raw_call(ctx, up.ptr, kt, rows, n, up.stride, k, largest, out.data_ptr(), idx.data_ptr() if with_idx else 0))
                        hv = out.cpu().numpy().view(UT[kt]).reshape(rows, k)
                        hi = idx.cpu().numpy().reshape(rows, k) if with_idx else None
                        if k:
                            check_result(up, S, k, largest, hv, hi)
                            st = ctx.stats()
                            assert st["topk_rows_kernel_rows"] + st["topk_rows_looped_rows"] == rows, st
                            if mode == 2:
                                assert st["topk_rows_kernel_rows"] == rows, (mode, st)
                            if mode == 1:
                                assert st["topk_rows_looped_rows"] == rows, (mode, st)
                        else:
                            assert hv.size == 0
                        if first is None:
                            first = hv
                        assert np.array_equal(first, hv), "the row kernel and the loop disagree"
    finally:
        ctx.set_option("topk_rows_mode", DEFAULTS["topk_rows_mode"])
    assert up.unchanged(), "the input (or its padding) was modified"


def seed_of(*xs):
    s = 17
    for x in xs:
        s = (s * 1000003 + int(x)) % (1 << 31)
    return s


# ---- every key type on every shape, two kinds each

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kt", range(6), ids=lambda k: NAMES[k])
def test_every_key_type_on_every_shape(ctx, kt, shape):
    rows, n = shape
    for kind in (("normal", "specials") if kt % 3 == 2 else ("bits", "small")):
        run_case(ctx, make_rows(rows, n, kind, kt, seed_of(kt, rows, n)), kt)


# ---- every kind on one shape per lanes-per-row variant

KIND_SHAPES = [(1000, 65), (257, 4097), (64, 131072)]


@pytest.mark.parametrize("shape", KIND_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", FLOAT_KINDS)
def test_every_float_kind(ctx, kind, shape):
    run_case(ctx, make_rows(shape[0], shape[1], kind, F32, seed_of(1, *shape)), F32)


@pytest.mark.parametrize("shape", KIND_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", INT_KINDS)
def test_every_int_kind(ctx, kind, shape):
    run_case(ctx, make_rows(shape[0], shape[1], kind, I64, seed_of(2, *shape)), I64)
    if kind in ("extremes", "const", "rotated"):
        run_case(ctx, make_rows(shape[0], shape[1], kind, U32, seed_of(3, *shape)), U32)


@pytest.mark.parametrize("kt", [F64, I32])
def test_all_ties_and_specials_for_the_other_widths(ctx, kt):
    for shape in KIND_SHAPES:
        for kind in (("const", "specials", "rotated") if kt == F64 else ("const", "extremes", "rotated")):
            run_case(ctx, make_rows(shape[0], shape[1], kind, kt, seed_of(4, *shape)), kt)


# ---- padded rows: the padding must never be read

@pytest.mark.parametrize("pad", [1, 3, 37])
@pytest.mark.parametrize("kt", [F32, I64, U32, F64])
def test_padded_rows(ctx, kt, pad):
    for rows, n in ((3, 64), (1000, 65), (257, 4097), (20, 50257), (5, (1 << 20) + 77)):
        kind = "normal" if kt % 3 == 2 else "bits"
        run_case(ctx, make_rows(rows, n, kind, kt, seed_of(5, rows, n, pad)), kt, pad=pad, lead=pad % 2)


def test_the_padding_patterns_would_win():
    for kt in range(6):
        ut = UT[kt]
        win = np_decode(np.array([np.iinfo(ut).max, 0], dtype=ut), kt)
        b = make_rows(2, 500, "normal" if kt % 3 == 2 else "bits", kt, 3)
        e = np_encode(np.concatenate([b.ravel(), win]), kt)
        assert e[-2] == e.max() and e[-1] == e.min()
    assert np.isnan(np_decode(np.array([0xFFFFFFFF], np.uint32), F32).view(np.float32)[0])


# ---- guard bands

@pytest.mark.parametrize("lead", [0, 16])
@pytest.mark.parametrize("shape,k", [((1000, 65), 7), ((257, 4097), 300), ((6, (1 << 20) + 77), 1000)], ids=["short", "medium", "looped"])
def test_guard_bands(ctx, shape, k, lead):
    import torch
    rows, n = shape
    pad = 3
    for kt in (F32, I64):
        bits = make_rows(rows, n, "normal" if kt == F32 else "bits", kt, seed_of(6, rows, n))
        S = sorted_rows(bits, kt)
        it = int_dtype(kt)
        for stride in (n, n + pad):
            extent = (rows - 1) * stride + n        # exactly the input's extent: no padding behind the last row
            flat = np.zeros(extent, UT[kt])
            for r in range(rows):
                flat[r * stride:r * stride + n] = bits[r]
            a_in = guardband.Arena(it, extent, lead_bytes=lead).fill(flat)
            a_out = guardband.Arena(it, rows * k, lead_bytes=lead)
            a_idx = guardband.Arena(torch.int64, rows * k, lead_bytes=lead)
            up = Uploaded.__new__(Uploaded)
            up.bits, up.kt, up.rows, up.row_len = bits, kt, rows, n
            for largest in (False, True):
                for with_idx in (False, True):
                    ctx._ok(raw_call(ctx, a_in.ptr, kt, rows, n, stride, k, largest, a_out.ptr, a_idx.ptr if with_idx else 0))
                    for a in (a_in, a_out, a_idx):
                        a.check("%s %s stride %d" % (NAMES[kt], shape, stride))
                    check_result(up, S, k, largest, a_out.host(UT[kt]).reshape(rows, k), a_idx.host(np.int64).reshape(rows, k) if with_idx else None)
            assert (a_in.host(UT[kt]) == flat).all()


# ---- arguments

def test_bad_arguments_are_refused_and_touch_nothing(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdError
    rows, n, k = 50, 300, 10
    bits = make_rows(rows, n, "normal", F32, 9)
    t = torch.from_numpy(bits.view(np.int32)).cuda()
    out = torch.full((rows * n + 8,), 0x3FC00000, dtype=torch.int32, device="cuda")
    idx = torch.full((rows * n + 8,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    t0, out0, idx0 = t.clone(), out.clone(), idx.clone()
    ip, op, xp = t.data_ptr(), out.data_ptr(), idx.data_ptr()

    def refused(**kw):
        a = dict(in_ptr=ip, kt=F32, rows=rows, row_len=n, stride=n, k=k, largest=0, out_ptr=op, idx_ptr=xp)
        a.update(kw)
        with pytest.raises(MsdError) as e:
            ctx._ok(ctx._L.msd_topk_rows(ctx._h, C.c_void_p(a["in_ptr"]), a["kt"], a["rows"], a["row_len"], a["stride"], a["k"], a["largest"],
                                         C.c_void_p(a["out_ptr"]), C.c_void_p(a["idx_ptr"]) if a["idx_ptr"] else None))
        assert "error -1" in str(e.value) and len(str(e.value)) > len("error -1: "), str(e.value)
        assert torch.equal(t, t0) and torch.equal(out, out0) and torch.equal(idx, idx0)

    assert raw_call(ctx, ip, F32, rows, n, n, k, False, op, xp) == 0      # (the call itself is fine)
    out.copy_(out0)
    idx.copy_(idx0)
    assert ctx._L.msd_topk_rows(None, C.c_void_p(ip), F32, rows, n, n, k, 0, C.c_void_p(op), C.c_void_p(xp)) == -1   # null context
    assert torch.equal(out, out0) and torch.equal(idx, idx0)
    refused(in_ptr=0)                                   # null input
    refused(out_ptr=0)                                  # null output
    refused(largest=2)                                  # unknown which
    refused(largest=-1, idx_ptr=0)
    refused(kt=6)                                       # unknown key type
    refused(kt=-1)
    refused(k=n + 1)                                    # k > row_len
    refused(stride=n - 1)                               # row_stride < row_len
    refused(in_ptr=ip + 2)                              # not aligned to the element
    refused(out_ptr=op + 1)
    refused(idx_ptr=xp + 4)
    refused(kt=F64, in_ptr=ip + 4, row_len=n // 2, stride=n // 2)     # 8-byte keys on a 4-byte boundary
    refused(rows=1 << 62, stride=1 << 40)               # rows * row_stride overflows
    refused(rows=1 << 60, row_len=2, stride=2, k=2)     # rows * k overflows (as bytes of the indices)
    refused(out_ptr=ip)                                 # the values alias the input
    refused(out_ptr=ip + (rows - 1) * n * 4)            # ... its last row
    refused(idx_ptr=ip)                                 # the indices alias the input
    refused(out_ptr=xp + 8)                             # the two outputs overlap
    refused(out_ptr=op, idx_ptr=op + 16)
    # the padding behind the last row is not part of the input's extent: an output may start there
    assert raw_call(ctx, ip, F32, rows - 1, n - 16, n, 4, False, ip + ((rows - 2) * n + n - 16) * 4, 0) == 0
    t.copy_(t0)
    # mode 2 outside the envelope
    max_len, max_k = limits(ctx, F32, True)
    big = torch.zeros(max_len + 16, dtype=torch.int32, device="cuda")
    try:
        ctx.set_option("topk_rows_mode", 2)
        refused(in_ptr=big.data_ptr(), rows=1, row_len=max_len + 16, stride=max_len + 16)
        refused(in_ptr=big.data_ptr(), rows=1, row_len=max_len, stride=max_len, k=max_k + 1)
        with pytest.raises(MsdError):
            ctx.set_option("topk_rows_mode", 3)
    finally:
        ctx.set_option("topk_rows_mode", DEFAULTS["topk_rows_mode"])
    # k == 0 and rows == 0: success, nothing touched
    assert raw_call(ctx, ip, F32, rows, n, n, 0, False, op, xp) == 0
    assert raw_call(ctx, ip, F32, 0, n, n, k, True, op, xp) == 0
    assert raw_call(ctx, 0, F32, 0, n, n, k, True, 0, 0) == 0
    assert torch.equal(t, t0) and torch.equal(out, out0) and torch.equal(idx, idx0)


def test_indices_of_32_bit_keys_need_rows_up_to_2_32(ctx):
    """row_len = 2^32 + 16 with indices on a 32-bit key type: refused before any launch (the buffer really has that size)."""
    import torch
    from inplacemsdradixsort_amd import MsdError
    n = 2**32 + 16
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    out = torch.full((16,), 1.5, dtype=torch.float32, device="cuda")
    idx = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(MsdError) as e:
        ctx._ok(raw_call(ctx, t.data_ptr(), F32, 1, n, n, 16, True, out.data_ptr(), idx.data_ptr()))
    assert "error -1" in str(e.value) and len(str(e.value)) > len("error -1: ")
    assert (out == 1.5).all() and (idx == -7).all()
    del t
    torch.cuda.empty_cache()


# ---- the Python wrapper

def test_python_wrapper_shapes_views_and_outputs(ctx):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    x = torch.randn(6, 5, 1031, device="cuda", generator=g)
    s = torch.sort(x, dim=-1).values
    v, i = ctx.topk_rows(x, 9, largest=True, indices=True)
    assert v.shape == (6, 5, 9) and i.shape == (6, 5, 9) and i.dtype == torch.int64
    assert torch.equal(v, s[..., -9:]) and torch.equal(torch.gather(x, -1, i), v)
    assert torch.equal(ctx.topk_rows(x, 9), s[..., :9])
    m = torch.randn(300, 1000, device="cuda", generator=g)
    for view in (m[:, :-3], m[:, 1:], m[5:200, 7:77], m[::2]):           # padded rows, rows off the 16-byte grid, a window
        sv = torch.sort(view, dim=1).values
        v, i = ctx.topk_rows(view, 5, indices=True)
        assert torch.equal(v, sv[:, :5]) and torch.equal(torch.gather(view, 1, i), v)
        assert torch.equal(ctx.topk_rows(view, 5, largest=True), sv[:, -5:])
    one = torch.randn(50257, device="cuda", generator=g)                  # 1-D: one row
    assert torch.equal(ctx.topk_rows(one, 3, largest=True), torch.sort(one).values[-3:])
    d = torch.randn(40, 777, dtype=torch.float64, device="cuda", generator=g)
    ov, oi = torch.empty(40, 4, dtype=torch.float64, device="cuda"), torch.empty(40, 4, dtype=torch.int64, device="cuda")
    rv, ri = ctx.topk_rows(d, 4, out=ov, out_indices=oi)
    assert rv is ov and ri is oi and torch.equal(ov, torch.sort(d, dim=1).values[:, :4]) and torch.equal(torch.gather(d, 1, oi), ov)
    li = torch.randint(-2**62, 2**62, (33, 129), device="cuda", generator=g)
    assert torch.equal(ctx.topk_rows(li, 129), torch.sort(li, dim=1).values)
    assert ctx.topk_rows(m, 0).shape == (300, 0)
    e, ei = ctx.topk_rows(torch.empty(0, 9, device="cuda"), 3, indices=True)
    assert e.shape == (0, 3) and ei.shape == (0, 3)


def test_python_wrapper_refuses_layouts_it_would_have_to_copy(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdError
    x = torch.randn(64, 48, device="cuda")
    before = x.clone()
    for bad in (x.t(), x[:, ::2], torch.empty(3, 6, 16, device="cuda")[:, :4, :], x.to(torch.float16)):
        with pytest.raises(MsdError):
            ctx.topk_rows(bad, 2)
    with pytest.raises(MsdError):
        ctx.topk_rows(x, 2, out=torch.empty(64, 3, device="cuda"))       # wrong shape
    with pytest.raises(MsdError):
        ctx.topk_rows(x, 2, out=torch.empty(64, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(MsdError):
        ctx.topk_rows(x, 2, out_indices=torch.empty(64, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(MsdError):
        ctx.topk_rows(x.cpu(), 2)
    with pytest.raises(MsdError) as e:
        ctx.topk_rows(x, 49)
    assert "error -1" in str(e.value)
    assert torch.equal(x, before)


def test_phase_is_reported(ctx):
    import torch
    x = torch.randn(512, 4096, device="cuda")
    try:
        ctx.set_profiling(True)
        ctx.topk_rows(x, 8, indices=True)
        names = [p[0] for p in ctx.phases()]
    finally:
        ctx.set_profiling(False)
    assert names == ["select_rows"], names
    assert ctx.stats()["topk_rows_kernel_rows"] == 512


# ---- the shape the feature is for, once

def test_4096_rows_of_131072_normal_scores_against_torch_sort(ctx):
    import torch
    rows, n, k = 4096, 131072, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    x = torch.randn(rows, n, dtype=torch.float32, device="cuda", generator=g)
    before = x.clone()
    s = torch.sort(x, dim=1).values
    for largest in (False, True):
        vals, idx = ctx.topk_rows(x, k, largest=largest, indices=True)
        st = ctx.stats()
        assert st["topk_rows_kernel_rows"] == rows and st["topk_rows_looped_rows"] == 0, st   # mode 0 took the row kernel
        torch.cuda.synchronize()
        assert torch.equal(vals, s[:, n - k:] if largest else s[:, :k])
        assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < n
        assert torch.equal(torch.gather(x, 1, idx), vals)
        assert bool((torch.sort(idx, dim=1).values.diff(dim=1) > 0).all()), "a position twice within a row"
        assert torch.equal(ctx.topk_rows(x, k, largest=largest), vals)
    assert torch.equal(x, before), "the input was modified"
