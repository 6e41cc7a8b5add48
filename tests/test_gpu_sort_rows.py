"""GPU tests of the per-row sort (msd_sort_rows; MsdContext.sort_rows): EVERY row of a matrix in the order of its key type,
ascending or descending, for all six key types, with and without the positions of the keys, through the one-launch row
kernel (its three group shapes) and through the segment path.

The expected result is defined in tests/sort_rows_expect.py.  Values are compared BITWISE, all rows and all elements.
Positions are never compared with expected positions (ties make them unspecified), only checked: every row's positions are
a permutation of [0, row_len), and the input holds at each of them a key that is bit-equal to the value beside it.  After
every case the input is compared with what was uploaded, except in the in-place cases.

The calls go through the C ABI on integer tensors that carry the bit patterns (so that the unsigned key types, padded rows
and arbitrary alignment need nothing of torch); the Python wrapper has tests of its own at the end."""
import ctypes as C

import numpy as np
import pytest

import guardband
import sort_rows_expect as E
from gpu_support import DEFAULTS, int_dtype_of_key as int_dtype
from sort_rows_expect import F32, F64, I32, I64, NAMES, U32, U64, UT, make_rows, seed_of

pytestmark = pytest.mark.gpu

W = 512     # the longest row of the wave shape
B = 4096    # the host rule: 256 lanes up to here, 1024 lanes beyond
ASC, DESC = 0, 1
FILL = 0x5A5A5A5A


def limit(ctx, kt, with_idx):
    v = C.c_uint64()
    assert ctx._L.msd_sort_rows_limits(kt, int(with_idx), C.byref(v)) == 0
    return int(v.value)


def np_int(kt):
    return np.int32 if UT[kt] == np.uint32 else np.int64


def raw_call(ctx, in_ptr, kt, rows, n, stride, desc, out_ptr, idx_ptr):
    return ctx._L.msd_sort_rows(ctx._h, C.c_void_p(in_ptr), kt, rows, n, stride, DESC if desc else ASC, C.c_void_p(out_ptr),
                                C.c_void_p(idx_ptr) if idx_ptr else None)


def lanes_for(n):
    return 64 if n <= W else 256 if n <= B else 1024


def takes_kernel(ctx, kt, with_idx, n, aligned=True):
    """the host rule under mode 0 (include/msd_sort_rows_hip.h): beyond the envelope the segment path; inside it the row
    kernel, but for the longer rows of 64-bit keys whose outputs the segment path can take"""
    if n > limit(ctx, kt, with_idx):
        return False
    if kt < U64 or not aligned:
        return True
    return n <= 512 if with_idx else n < 4096


class Uploaded:
    """rows x row_len bit patterns on the device, `pad` elements of padding behind every row and `lead` in front of the
    first: the padding holds the two patterns that would sort first / last if they were read (the largest and the smallest
    key of the key type, alternating)."""

    def __init__(self, bits, kt, pad=0, lead=0):
        import torch
        self.bits, self.kt = bits, kt
        self.rows, self.row_len = bits.shape
        self.stride = self.row_len + pad
        ut = UT[kt]
        win = E.np_decode(np.array([np.iinfo(ut).max, 0], dtype=ut), kt)
        flat = np.empty(lead + self.rows * self.stride, ut)
        flat[0::2] = win[0]
        flat[1::2] = win[1]
        body = flat[lead:].reshape(self.rows, self.stride)
        body[:, :self.row_len] = bits
        self.flat = flat
        self.es = flat.itemsize
        self.t = torch.from_numpy(flat.view(np_int(kt))).cuda()
        self.ptr = self.t.data_ptr() + lead * self.es

    def unchanged(self):
        return (self.t.cpu().numpy().view(UT[self.kt]) == self.flat).all()


def check_values(kt, bits, desc, hv, what=""):
    want = E.expected(bits, kt, desc)
    assert hv.shape == want.shape
    bad = np.nonzero((hv != want).any(axis=1))[0]
    assert bad.size == 0, (NAMES[kt], bits.shape, desc, what, "values differ in %d rows, first %d" % (bad.size, bad[0] if bad.size else -1))


def run_case(ctx, bits, kt, pad=0, lead=0, out_lead=0, dirs=(False, True), idxs=(False, True), check_path=True):
    """both directions, with and without positions; under mode 0 and, inside the envelope, under mode 2 as well (mode 0 sends
    the longer rows of 64-bit keys to the segment path: the kernel is to be tested on them all the same).  out_lead: the
    outputs start that many elements off the 16-byte grid (inside the envelope only: the segment path refuses it).
    check_path (the caller has set no option): the counters name the path and the group shape the row length should take."""
    try:
        for with_idx in idxs:
            for mode in ((None,) if not check_path else (0, 2) if n_inside(ctx, kt, with_idx, bits.shape[1]) else (0,)):
                if mode is not None:
                    ctx.set_option("sort_rows_mode", mode)
                _run_case(ctx, bits, kt, pad, lead, out_lead, dirs, with_idx, check_path, mode == 2)
    finally:
        if check_path:
            ctx.set_option("sort_rows_mode", DEFAULTS["sort_rows_mode"])


def n_inside(ctx, kt, with_idx, n):
    return n <= limit(ctx, kt, with_idx)


def _run_case(ctx, bits, kt, pad, lead, out_lead, dirs, with_idx, check_path, forced_kernel):
    import torch
    up = Uploaded(bits, kt, pad, lead)
    rows, n = up.rows, up.row_len
    it = int_dtype(kt)
    inside = n_inside(ctx, kt, with_idx, n)
    ol = out_lead if inside else 0
    for desc in dirs:
        out = torch.full((rows * n + ol,), FILL, dtype=it, device="cuda")
        idx = torch.full((rows * n + ol,), -7, dtype=torch.int64, device="cuda") if with_idx else None
        rc = raw_call(ctx, up.ptr, kt, rows, n, up.stride, desc, out.data_ptr() + ol * up.es, idx.data_ptr() + ol * 8 if with_idx else 0)
        ctx._ok(rc)
        ho = out.cpu().numpy().view(UT[kt])
        assert (ho[:ol] == UT[kt](FILL)).all()
        hv = ho[ol:].reshape(rows, n)
        check_values(kt, bits, desc, hv, (with_idx, pad, lead, ol))
        if with_idx:
            hx = idx.cpu().numpy()
            assert (hx[:ol] == -7).all()
            E.check_positions(bits, hv, hx[ol:].reshape(rows, n))
        st = ctx.stats()
        assert st["sort_rows_kernel_rows"] + st["sort_rows_segment_rows"] == rows, st
        if check_path:
            kernel = forced_kernel or takes_kernel(ctx, kt, with_idx, n, aligned=(ol * up.es) % 16 == 0)
            assert st["sort_rows_kernel_rows"] == (rows if kernel else 0), (n, with_idx, st)
            assert st["sort_rows_lanes"] == (lanes_for(n) if kernel else 0), (n, with_idx, st)
    assert up.unchanged(), "the input (or its padding) was modified"


# ---- shapes: every key type, both directions, with and without positions

LEN_SPECS = ["1", "2", "3", "63", "64", "65", "W-1", "W", "W+1", "B-1", "B", "B+1", "M-1", "M", "M+1", "M+77", "70001"]


def resolve(spec, M):
    return int(eval(spec, {"W": W, "B": B, "M": M}))


@pytest.mark.parametrize("spec", LEN_SPECS)
@pytest.mark.parametrize("kt", range(6), ids=lambda k: NAMES[k])
def test_every_key_type_on_every_row_length(ctx, kt, spec):
    for with_idx in (False, True):
        n = resolve(spec, limit(ctx, kt, with_idx))
        for rows in (1, 3, 7):
            run_case(ctx, make_rows(rows, n, E.default_kind(kt), kt, seed_of(kt, rows, n)), kt, idxs=(with_idx,))


# groups loop over more rows than the grid holds, and a wave's read-ahead crosses workgroups
@pytest.mark.parametrize("shape", [(100000, 8), (20000, 65), (1000, 513), (1500, 513)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kt", range(6), ids=lambda k: NAMES[k])
def test_many_rows(ctx, kt, shape):
    rows, n = shape
    run_case(ctx, make_rows(rows, n, E.default_kind(kt), kt, seed_of(7, kt, rows, n)), kt)


@pytest.mark.parametrize("kt", range(6), ids=lambda k: NAMES[k])
def test_segment_path_with_partition_rounds(ctx, kt):
    n = (1 << 18) + 5
    run_case(ctx, make_rows(2, n, E.default_kind(kt), kt, seed_of(8, kt)), kt)


# ---- every input kind on one shape per group shape

KIND_SHAPES = [(37, 300), (9, 3001), (3, 9001)]


def test_the_kind_shapes_take_the_three_group_shapes():
    assert [lanes_for(n) for _, n in KIND_SHAPES] == [64, 256, 1024]


@pytest.mark.parametrize("kind", E.FLOAT_KINDS)
@pytest.mark.parametrize("kt", [F32, F64], ids=lambda k: NAMES[k])
def test_every_float_kind(ctx, kt, kind):
    for rows, n in KIND_SHAPES:
        run_case(ctx, make_rows(rows, n, kind, kt, seed_of(1, kt, n)), kt)


@pytest.mark.parametrize("kind", E.INT_KINDS)
@pytest.mark.parametrize("kt", [U32, I32, U64, I64], ids=lambda k: NAMES[k])
def test_every_int_kind(ctx, kt, kind):
    for rows, n in KIND_SHAPES:
        run_case(ctx, make_rows(rows, n, kind, kt, seed_of(2, kt, n)), kt)


# ---- forced group shapes

@pytest.mark.parametrize("lanes", [64, 256, 1024])
@pytest.mark.parametrize("kt", [F32, I64], ids=lambda k: NAMES[k])
def test_forced_lanes(ctx, kt, lanes):
    bits = make_rows(50, 300, E.default_kind(kt), kt, seed_of(3, kt))
    try:
        ctx.set_option("sort_rows_lanes", lanes)
        run_case(ctx, bits, kt, check_path=False)
        assert ctx.stats()["sort_rows_lanes"] == lanes
        if lanes == 64:     # a row that does not fit the forced shape takes the shape of its length
            run_case(ctx, make_rows(3, W + 1, E.default_kind(kt), kt, seed_of(4, kt)), kt)
    finally:
        ctx.set_option("sort_rows_lanes", DEFAULTS["sort_rows_lanes"])


# ---- modes

@pytest.mark.parametrize("kt", [F32, I64, U32, F64], ids=lambda k: NAMES[k])
def test_kernel_and_segment_path_agree_inside_the_envelope(ctx, kt):
    import torch
    it = int_dtype(kt)
    try:
        for with_idx in (False, True):
            for rows, n in ((7, 300), (5, 5000), (3, limit(ctx, kt, with_idx)), (40, 1)):
                bits = make_rows(rows, n, E.default_kind(kt), kt, seed_of(5, kt, n))
                up = Uploaded(bits, kt)
                for desc in (False, True):
                    got = {}
                    for mode in (2, 1):
                        ctx.set_option("sort_rows_mode", mode)
                        out = torch.full((rows * n,), FILL, dtype=it, device="cuda")
                        idx = torch.full((rows * n,), -7, dtype=torch.int64, device="cuda") if with_idx else None
                        ctx._ok(raw_call(ctx, up.ptr, kt, rows, n, n, desc, out.data_ptr(), idx.data_ptr() if with_idx else 0))
                        got[mode] = out.cpu().numpy().view(UT[kt]).reshape(rows, n)
                        check_values(kt, bits, desc, got[mode], mode)
                        if with_idx:
                            E.check_positions(bits, got[mode], idx.cpu().numpy().reshape(rows, n))
                        st = ctx.stats()
                        assert st["sort_rows_kernel_rows"] == (rows if mode == 2 else 0) and st["sort_rows_segment_rows"] == (rows if mode == 1 else 0), st
                    assert np.array_equal(got[1], got[2])
                assert up.unchanged()
    finally:
        ctx.set_option("sort_rows_mode", DEFAULTS["sort_rows_mode"])


class Buffers:
    """an input, an output and positions with known contents, to show that a refused call touched nothing"""

    def __init__(self, kt, rows, n, stride=None):
        import torch
        self.kt, self.rows, self.n, self.stride = kt, rows, n, stride or n
        self.bits = make_rows(rows, self.stride, "bits", kt, seed_of(6, kt, n))
        self.inp = torch.from_numpy(self.bits.view(np_int(kt)).ravel().copy()).cuda()
        self.out = torch.full((rows * n + 8,), FILL, dtype=int_dtype(kt), device="cuda")
        self.idx = torch.full((rows * n + 8,), -7, dtype=torch.int64, device="cuda")
        self.es = self.bits.itemsize

    def untouched(self):
        return ((self.inp.cpu().numpy().view(UT[self.kt]) == self.bits.ravel()).all() and (self.out.cpu().numpy().view(UT[self.kt]) == UT[self.kt](FILL)).all()
                and (self.idx.cpu().numpy() == -7).all())


@pytest.mark.parametrize("kt", [F32, I64], ids=lambda k: NAMES[k])
def test_mode_2_beyond_the_envelope_is_refused(ctx, kt):
    try:
        ctx.set_option("sort_rows_mode", 2)
        for with_idx in (False, True):
            n = limit(ctx, kt, with_idx) + 1
            b = Buffers(kt, 2, n)
            assert raw_call(ctx, b.inp.data_ptr(), kt, 2, n, n, False, b.out.data_ptr(), b.idx.data_ptr() if with_idx else 0) == -1
            assert "sort_rows_mode 2" in ctx._L.msd_last_error(ctx._h).decode()
            assert b.untouched()
    finally:
        ctx.set_option("sort_rows_mode", DEFAULTS["sort_rows_mode"])


# ---- padded and misaligned rows: the padding must never be read, and no base needs more than its element's alignment

@pytest.mark.parametrize("pad", [1, 3, 37])
@pytest.mark.parametrize("kt", [F32, I64, U32, F64], ids=lambda k: NAMES[k])
def test_padded_and_misaligned_rows(ctx, kt, pad):
    M = limit(ctx, kt, True)
    for rows, n in ((3, 64), (1000, 65), (9, 4097), (3, M), (3, M + 77)):
        run_case(ctx, make_rows(rows, n, E.default_kind(kt), kt, seed_of(9, rows, n, pad)), kt, pad=pad, lead=1, out_lead=1)
    run_case(ctx, make_rows(5, 300, E.default_kind(kt), kt, seed_of(10, pad)), kt, pad=pad, lead=0, out_lead=0)


def test_the_padding_patterns_would_sort_first_and_last():
    for kt in range(6):
        ut = UT[kt]
        win = E.np_decode(np.array([np.iinfo(ut).max, 0], dtype=ut), kt)
        b = make_rows(2, 500, E.default_kind(kt), kt, 3)
        e = E.np_encode(np.concatenate([b.ravel(), win]), kt)
        assert e[-2] == e.max() and e[-1] == e.min()


# ---- in place

@pytest.mark.parametrize("kt", range(6), ids=lambda k: NAMES[k])
def test_in_place(ctx, kt):
    import torch
    for with_idx in (False, True):
        M = limit(ctx, kt, with_idx)
        for rows, n in ((1000, 65), (9, 3001), (3, M), (3, M + 77)):
            bits = make_rows(rows, n, E.default_kind(kt), kt, seed_of(11, kt, n))
            for desc, mode in ((False, 0), (True, 0)) + (((False, 2), (True, 2)) if n <= M else ()):
                t = torch.from_numpy(bits.view(np_int(kt)).ravel().copy()).cuda()
                idx = torch.full((rows * n,), -7, dtype=torch.int64, device="cuda") if with_idx else None
                try:
                    ctx.set_option("sort_rows_mode", mode)
                    ctx._ok(raw_call(ctx, t.data_ptr(), kt, rows, n, n, desc, t.data_ptr(), idx.data_ptr() if with_idx else 0))
                finally:
                    ctx.set_option("sort_rows_mode", DEFAULTS["sort_rows_mode"])
                hv = t.cpu().numpy().view(UT[kt]).reshape(rows, n)
                check_values(kt, bits, desc, hv, "in place")
                if with_idx:
                    E.check_positions(bits, hv, idx.cpu().numpy().reshape(rows, n))
                st = ctx.stats()
                assert st["sort_rows_kernel_rows"] == (rows if mode == 2 or takes_kernel(ctx, kt, with_idx, n) else 0), st


# ---- guard bands around the input, the output and the positions

@pytest.mark.parametrize("case", ["wave", "full", "segments", "lead16"])
def test_guard_bands(ctx, case):
    import torch
    for kt in (F32, I64):
        M = limit(ctx, kt, True)
        rows, n, pad, lead = {"wave": (1000, 65, 3, 0), "full": (3, M, 0, 0), "segments": (3, M + 77, 3, 0), "lead16": (9, 3001, 1, 16)}[case]
        bits = make_rows(rows, n, E.default_kind(kt), kt, seed_of(12, rows, n))
        stride = n + pad
        extent = (rows - 1) * stride + n          # exactly the input's extent: no padding behind the last row
        flat = np.zeros(extent, UT[kt])
        for r in range(rows):
            flat[r * stride:r * stride + n] = bits[r]
        it = int_dtype(kt)
        for desc, neighbours in ((False, "low"), (True, "high")):
            a_in = guardband.Arena(it, extent, lead_bytes=lead, neighbours=neighbours).fill(flat)
            a_out = guardband.Arena(it, rows * n, lead_bytes=lead, neighbours=neighbours)
            a_idx = guardband.Arena(torch.int64, rows * n, lead_bytes=lead, neighbours=neighbours)
            a_out.payload.fill_(FILL)
            a_idx.payload.fill_(-7)
            try:
                ctx.set_option("sort_rows_mode", 2 if n <= M else 0)      # (the cases inside the envelope are the kernel's)
                ctx._ok(raw_call(ctx, a_in.ptr, kt, rows, n, stride, desc, a_out.ptr, a_idx.ptr))
            finally:
                ctx.set_option("sort_rows_mode", DEFAULTS["sort_rows_mode"])
            for a, what in ((a_in, "input"), (a_out, "output"), (a_idx, "positions")):
                a.check("%s %s %s" % (case, NAMES[kt], what))
            hv = a_out.host(UT[kt]).reshape(rows, n)
            check_values(kt, bits, desc, hv, case)
            E.check_positions(bits, hv, a_idx.host(np.int64).reshape(rows, n))
            assert (a_in.host(UT[kt]) == flat).all()
            st = ctx.stats()
            assert st["sort_rows_kernel_rows"] == (rows if n <= M else 0), st


# ---- refusals: MSD_EINVAL before any launch, every buffer untouched

def test_refusals_leave_every_buffer_untouched(ctx):
    L, h = ctx._L, ctx._h
    for kt in (F32, I64):
        es = 4 if kt == F32 else 8
        M = limit(ctx, kt, True)
        rows, n = 4, 100
        b = Buffers(kt, rows, n)
        inp, out, idx = b.inp.data_ptr(), b.out.data_ptr(), b.idx.data_ptr()
        p = C.c_void_p
        bad = [
            ("null input", (p(0), kt, rows, n, n, ASC, p(out), p(idx))),
            ("null output", (p(inp), kt, rows, n, n, ASC, p(0), p(idx))),
            ("key type", (p(inp), 6, rows, n, n, ASC, p(out), p(idx))),
            ("key type", (p(inp), -1, rows, n, n, ASC, p(out), None)),
            ("order", (p(inp), kt, rows, n, n, 2, p(out), p(idx))),
            ("order", (p(inp), kt, rows, n, n, -1, p(out), None)),
            ("stride < len", (p(inp), kt, rows, n, n - 1, ASC, p(out), p(idx))),
            ("misaligned input", (p(inp + 1), kt, rows, n, n, ASC, p(out), p(idx))),
            ("misaligned output", (p(inp), kt, rows, n, n, ASC, p(out + es // 2), p(idx))),
            ("misaligned positions", (p(inp), kt, rows, n, n, ASC, p(out), p(idx + 4))),
            ("rows * stride overflows", (p(inp), kt, 1 << 40, n, 1 << 40, ASC, p(out), p(idx))),
            ("rows * len overflows", (p(inp), kt, 1 << 62, 8, 8, ASC, p(out), None)),
            ("in place with padding", (p(inp), kt, rows, n - 4, n, ASC, p(inp), None)),
            ("out inside the input", (p(inp), kt, rows, n, n, ASC, p(inp + 4 * es), None)),
            ("out overlaps the input's end", (p(inp), kt, rows, n, n, ASC, p(inp + (rows * n - 1) * es), None)),
            ("positions on the input", (p(inp), kt, rows, n // 2, n // 2, ASC, p(out), p(inp))),
            ("positions on the output", (p(inp), kt, rows, n // 2, n // 2, ASC, p(out), p(out))),
            ("positions overlap the output's end", (p(inp), kt, rows, n // 2, n // 2, ASC, p(idx), p(idx + (rows * (n // 2) * es) // 8 * 8 - 8))),
        ]
        for what, args in bad:
            assert L.msd_sort_rows(h, *args) == -1, (NAMES[kt], what)
            assert L.msd_last_error(h), what
            assert b.untouched(), (NAMES[kt], what)
        # beyond the envelope the outputs follow the segment sort's own rule: 16-byte aligned, and the message says so
        n2 = M + 77
        b2 = Buffers(kt, 2, n2)
        for what, o, x in (("output", b2.out.data_ptr() + es, b2.idx.data_ptr()), ("positions", b2.out.data_ptr(), b2.idx.data_ptr() + 8)):
            assert L.msd_sort_rows(h, C.c_void_p(b2.inp.data_ptr()), kt, 2, n2, n2, ASC, C.c_void_p(o), C.c_void_p(x)) == -1, what
            assert "16-byte" in L.msd_last_error(h).decode() and "segment sort" in L.msd_last_error(h).decode()
            assert b2.untouched(), what
        # ... and the padding behind the LAST row is not part of the input: an output right behind the extent is fine
        b3 = Buffers(kt, 3, 60, stride=64)
        flat = torch_cat_with_room(b3)
        ctx._ok(L.msd_sort_rows(h, C.c_void_p(flat.data_ptr()), kt, 3, 60, 64, ASC, C.c_void_p(flat.data_ptr() + (2 * 64 + 60) * es), None))
        hv = flat.cpu().numpy().view(UT[kt])[2 * 64 + 60:2 * 64 + 60 + 180].reshape(3, 60)
        check_values(kt, b3.bits[:, :60], False, hv, "output behind the extent")


def torch_cat_with_room(b):
    """the input of `b` with room for an output behind it, in one tensor"""
    import torch
    return torch.cat([b.inp, torch.zeros(b.rows * b.n + 8, dtype=b.inp.dtype, device="cuda")])


def test_no_ops(ctx):
    for kt in (F32, I64):
        b = Buffers(kt, 4, 100)
        inp, out, idx = b.inp.data_ptr(), b.out.data_ptr(), b.idx.data_ptr()
        assert raw_call(ctx, inp, kt, 0, 100, 100, False, out, idx) == 0
        assert raw_call(ctx, inp, kt, 4, 0, 100, False, out, idx) == 0
        assert raw_call(ctx, 0, kt, 0, 0, 0, True, 0, 0) == 0
        assert b.untouched()


# ---- the Python wrapper

def test_wrapper_against_torch(ctx):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    for shape in ((1000, 65), (4, 6, 513), (3, 9001), (2, 30000)):
        x = torch.randn(shape, device="cuda", generator=g)                                   # (no NaN, and -0 is improbable: torch's order)
        y = torch.randint(-2**62, 2**62, shape, device="cuda", generator=g, dtype=torch.int64)
        for t in (x, y):
            for desc in (False, True):
                want = torch.sort(t, dim=-1, descending=desc).values
                v = ctx.sort_rows(t, descending=desc)
                assert v.shape == t.shape and torch.equal(v, want)
                v2, idx = ctx.sort_rows(t, descending=desc, indices=True)
                assert idx.dtype == torch.int64 and idx.shape == t.shape
                assert torch.equal(v2, want) and torch.equal(torch.gather(t, -1, idx), v2)
    st = ctx.stats()
    assert st["sort_rows_segment_rows"] == 2 and st["sort_rows_kernel_rows"] == 0


def test_wrapper_views_and_out(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdError
    g = torch.Generator(device="cuda").manual_seed(6)
    big = torch.randn(50, 400, device="cuda", generator=g)
    view = big[:, :300]                                      # padded rows: stride 400
    keep = big.clone()
    out = torch.empty(50, 300, device="cuda")
    oi = torch.empty(50, 300, dtype=torch.int64, device="cuda")
    r = ctx.sort_rows(view, out=out, out_indices=oi)
    assert r[0] is out and r[1] is oi
    assert torch.equal(out, torch.sort(view, dim=-1).values) and torch.equal(torch.gather(view, -1, oi), out)
    assert torch.equal(big, keep)
    with pytest.raises(MsdError):                            # in place needs row_stride == row_len
        ctx.sort_rows(view, out=big[:, :300])
    with pytest.raises(MsdError):                            # no hidden copy
        ctx.sort_rows(big.t())
    c = keep.clone()
    assert ctx.sort_rows(c, descending=True, out=c) is c     # in place, contiguous
    assert torch.equal(c, torch.sort(keep, dim=-1, descending=True).values)
    one = torch.randn(777, device="cuda", generator=g)       # one dimension: one row
    assert torch.equal(ctx.sort_rows(one), torch.sort(one).values)
    i32 = torch.randint(-2**31, 2**31 - 1, (33, 129), device="cuda", generator=g, dtype=torch.int32)
    f64 = torch.randn(33, 129, device="cuda", generator=g, dtype=torch.float64)
    for t in (i32, f64):
        assert torch.equal(ctx.sort_rows(t), torch.sort(t, dim=-1).values)
    assert ctx.sort_rows_limits(big) == limit(ctx, F32, False) and ctx.sort_rows_limits(f64, indices=True) == limit(ctx, F64, True)


# ---- phase report

def test_phase_is_reported(ctx):
    import torch
    x = torch.randn(100, 300, device="cuda")
    try:
        ctx.set_profiling(True)
        ctx.sort_rows(x)
        ph = ctx.phases()
        assert [p[0] for p in ph] == ["sort_rows"] and ph[0][1] > 0, ph
        ctx.sort_rows(torch.randn(2, 30000, device="cuda"), indices=True)
        assert "sort_rows" in [p[0] for p in ctx.phases()]
    finally:
        ctx.set_profiling(False)
