"""GPU tests of run-length encode (msd_run_encode; MsdContext.run_encode / unique): the distinct values of every run, where each
run starts, the terminator, the inverse map (plain, through the identity and through real sort positions) and the true
number of runs, for 4- and 8-byte elements.

The expected result is defined in tests/runs_expect.py; everything is compared BITWISE, all elements.  The calls go through
the C ABI on integer tensors that carry the bit patterns, with EVERY buffer -- input, values, starts, inverse, num_runs --
inside a guardband.Arena whose payload is pre-filled with a known pattern: a case checks what was written, that the rest of
each payload is what it was, that no guard was touched and that the input is what was uploaded.  The Python wrappers have
tests of their own at the end."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gpu_support as D
import guardband
import runs_expect as R
import sort_rows_expect as E
from guardband import Buf

pytestmark = pytest.mark.gpu

WIDTHS = E.WIDTHS


def limits(ctx, es):
    tile, scan_tile = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_run_encode_limits(es, C.byref(tile), C.byref(scan_tile)) == 0
    return int(tile.value), int(scan_tile.value)


def raw_call(ctx, data_ptr, es, n, cap, values_ptr, starts_ptr, positions_ptr, inverse_ptr, num_ptr):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_run_encode(ctx._h, vp(data_ptr), es, n, cap, vp(values_ptr), vp(starts_ptr), vp(positions_ptr), vp(inverse_ptr), vp(num_ptr))


def run_case(ctx, a, cap=None, values=True, starts=True, inverse=True, positions=None, in_off=0, in_lead=0, val_off=0, what=""):
    """one call on the unsigned array `a`, everything checked; returns the device buffers' host copies (values, starts, inverse)"""
    es, n = a.itemsize, a.size
    cap = n if cap is None else cap
    what = (what, es, n, cap, values, starts, inverse, positions is not None, in_off, in_lead, val_off)
    din = Buf(es, n, in_off, in_lead, a)
    dval = Buf(es, cap, val_off) if values else None
    dst = Buf(8, cap + 1) if starts else None
    dinv = Buf(8, n) if inverse else None
    dpos = Buf(8, n, a=positions.astype(np.uint64)) if positions is not None else None
    dnum = Buf(8, 1)
    rc = raw_call(ctx, din.ptr, es, n, cap, dval and dval.ptr, dst and dst.ptr, dpos and dpos.ptr, dinv and dinv.ptr, dnum.ptr)
    ctx._ok(rc)
    m, ev, es_, einv = R.expected_capped(a, cap, positions)
    k = min(m, cap)
    assert int(dnum.host()[0]) == m, (what, "num_runs", int(dnum.host()[0]), m)
    out = [None, None, None]
    if values:
        hv = dval.host()
        assert (hv[:k] == ev).all(), (what, "values differ", int(np.argmax(hv[:k] != ev)))
        assert dval.untouched_from(k), (what, "values written beyond min(m, cap)")
        out[0] = hv[:k]
    if starts:
        hs = dst.host()
        assert (hs[:k + 1].view(np.int64) == es_).all(), (what, "starts differ", int(np.argmax(hs[:k + 1].view(np.int64) != es_)))
        assert dst.untouched_from(k + 1), (what, "starts written beyond min(m, cap) + 1")
        out[1] = hs[:k + 1].view(np.int64)
    if inverse:
        hi = dinv.host().view(np.int64)
        assert (hi == einv).all(), (what, "inverse differs", int(np.argmax(hi != einv)))
        out[2] = hi
    assert din.unchanged(), (what, "the input changed")
    if dpos is not None:
        assert dpos.unchanged(), (what, "the positions changed")
    for name, b in (("input", din), ("values", dval), ("starts", dst), ("inverse", dinv), ("positions", dpos), ("num_runs", dnum)):
        if b is not None:
            b.check("%s of %s" % (name, what))
    return out


# ---- sizes x run patterns, both widths

@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("size", R.SIZE_NAMES)
@pytest.mark.parametrize("es", WIDTHS)
def test_sizes_and_patterns(ctx, es, size, pattern):
    tile, scan_tile = limits(ctx, es)
    n = R.sizes(tile, scan_tile)[size]
    a = R.make(pattern, n, es, tile, seed=E.seed_of(es, n))
    run_case(ctx, a, what=pattern)


# ---- values

@pytest.mark.parametrize("es", WIDTHS)
def test_keys_that_differ_in_one_bit(ctx, es):
    tile, _ = limits(ctx, es)
    n = 2 * tile + 1
    base = 0x12345678 if es == 4 else 0x123456789ABCDEF0
    bits = [8 * es - 1, 0] + ([32, 31] if es == 8 else [])   # the top bit and the lowest one; of both words of an 8-byte element
    for bit in bits:
        a = R.two_values(n, es, base, base ^ (1 << bit), seed=bit)
        v, _, _ = run_case(ctx, a, what="bit %d" % bit)
        assert v.size > n // 6 and set(np.unique(v).tolist()) == {base, base ^ (1 << bit)}


def test_float_specials_through_integer_views(ctx):
    for ft, ut in ((np.float32, np.uint32), (np.float64, np.uint64)):
        W = 8 * np.dtype(ut).itemsize
        qnan = (0x7FC00000 if W == 32 else 0x7FF8 << 48)
        sign = 1 << (W - 1)
        zeros = np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0], ft).view(ut)
        v, s, _ = run_case(ctx, zeros, what="zeros")
        assert v.tolist() == [0, sign, 0, sign] and s.tolist() == [0, 2, 4, 5, 6]          # +0 and -0 are two values
        nans = np.array([qnan, qnan, qnan, qnan | 1, qnan | 1, qnan | sign, qnan | sign, qnan], ut)
        assert np.isnan(nans.view(ft)).all()
        v, s, i = run_case(ctx, nans, what="nans")
        assert v.tolist() == [qnan, qnan | 1, qnan | sign, qnan]                            # equal NaNs are one run, other payloads not
        assert s.tolist() == [0, 3, 5, 7, 8] and i.tolist() == [0, 0, 0, 1, 1, 2, 2, 3]
        mixed = np.tile(np.r_[zeros, nans, np.array([1.5, 1.5, np.inf, -np.inf], ft).view(ut)], 700)
        run_case(ctx, mixed, what="specials")


# ---- capacity

@pytest.mark.parametrize("pattern", ["distinct", "geo40", "equal"])
@pytest.mark.parametrize("es", WIDTHS)
def test_capacity(ctx, es, pattern):
    tile, _ = limits(ctx, es)
    n = 2 * tile + 1
    a = R.make(pattern, n, es, tile, seed=5)
    m = R.expected(a)[0]
    for cap in sorted({0, m - 1, m, m + 1, n}):
        run_case(ctx, a, cap=cap, what="cap")
        run_case(ctx, a, cap=cap, inverse=False, what="cap")


# ---- alignment

@pytest.mark.parametrize("es", WIDTHS)
def test_alignment_of_input_and_values(ctx, es):
    tile, _ = limits(ctx, es)
    per16 = 16 // es
    page = guardband.PAGE // es
    a_full = R.make("geo1.5", 3 * tile, es, tile, seed=9)
    for off in range(1, per16):                                  # 4, 8, 12 bytes (4-byte elements) / 8 bytes off a 16-byte boundary
        for n in (1, 2, 3, per16 - off, per16 - off + 1, 65, tile - off, tile, tile + 1, 2 * tile + 1):
            run_case(ctx, a_full[:n], in_off=off, val_off=off, what="off")
            run_case(ctx, a_full[:n], in_off=off, val_off=0, inverse=False, what="off")
            run_case(ctx, a_full[:n], in_off=0, val_off=off, what="off")
    # the input's first element is the first / the last element of a page; its last element the last / the first of a page
    for in_lead, off, n in ((0, 0, page), (0, 0, page + 1), (guardband.PAGE - 16, per16 - 1, 1), (guardband.PAGE - 16, per16 - 1, page),
                            (guardband.PAGE - 16, per16 - 1, page + 1), (0, 1, page - 1), (0, 1, 2 * page)):
        run_case(ctx, a_full[:n], in_off=off, in_lead=in_lead, val_off=off, what="page")


# ---- the inverse

@pytest.mark.parametrize("es", WIDTHS)
def test_inverse_through_positions(ctx, es):
    import torch
    tile, _ = limits(ctx, es)
    rng = np.random.default_rng(3)
    for n in (1, 2, 65, tile + 1, 3 * tile - 1, 100003):
        x = R.geometric(n, es, 3.0, seed=n)[rng.permutation(n)] & R.UT[es](0xFFFF if n > 65 else 0x7)   # unsorted, many duplicates
        run_case(ctx, x, positions=np.arange(n, dtype=np.int64), what="identity")
        run_case(ctx, x, positions=rng.permutation(n).astype(np.int64), what="permutation")
        t = torch.from_numpy(x.view(R.IT[es])).cuda()
        if es == 4:
            s, pos = ctx.sort_rows(t, indices=True)
        else:
            s, pos = t.clone(), torch.arange(n, dtype=torch.int64, device="cuda")
            ctx.sort_typed(s, rids=pos)
        hs, hp = s.cpu().numpy().view(R.UT[es]), pos.cpu().numpy()
        assert (x[hp] == hs).all()
        v, _, inv = run_case(ctx, hs, positions=hp, what="sorted")
        assert (v[inv] == x).all()                               # torch's return_inverse: values[inverse] is the ORIGINAL array
        assert v.size == np.unique(x).size


# ---- optional outputs

@pytest.mark.parametrize("es", WIDTHS)
def test_optional_outputs_in_every_combination(ctx, es):
    tile, _ = limits(ctx, es)
    n = 2 * tile + 77
    a = R.make("geo40", n, es, tile, seed=11)
    pos = np.random.default_rng(4).permutation(n).astype(np.int64)
    for values, starts, inverse in itertools.product((False, True), repeat=3):
        run_case(ctx, a, values=values, starts=starts, inverse=inverse, what="optional")
        run_case(ctx, a, cap=7, values=values, starts=starts, inverse=inverse, what="optional")
        if inverse:
            run_case(ctx, a, values=values, starts=starts, inverse=True, positions=pos, what="optional")


def test_an_empty_array(ctx):
    for es in WIDTHS:
        a = np.zeros(0, R.UT[es])
        for cap in (0, 5):
            _, s, _ = run_case(ctx, a, cap=cap, what="empty")
            assert s.tolist() == [0]
            run_case(ctx, a, cap=cap, values=False, starts=False, inverse=False, what="empty")
        dnum, dst = Buf(8, 1), Buf(8, 3)
        ctx._ok(raw_call(ctx, 0, es, 0, 2, 0, dst.ptr, 0, 0, dnum.ptr))           # a null d_data with n == 0 is fine
        assert int(dnum.host()[0]) == 0 and int(dst.host()[0]) == 0 and dst.untouched_from(1)
        dnum.check("num_runs")
        dst.check("starts")


# ---- refusals through the C ABI

def test_refusals_touch_nothing(ctx):
    n = 1000
    for es in WIDTHS:
        a = R.make("geo1.5", n, es, 64, seed=2)
        din, dval, dst, dinv, dnum = Buf(es, n, a=a), Buf(es, n), Buf(8, n + 1), Buf(8, n), Buf(8, 1)
        dpos = Buf(8, n, a=np.arange(n, dtype=np.uint64))
        bufs = (din, dval, dst, dinv, dpos, dnum)
        good = dict(data=din.ptr, es=es, n=n, cap=n, values=dval.ptr, starts=dst.ptr, positions=dpos.ptr, inverse=dinv.ptr, num=dnum.ptr)

        def refused(message, **change):
            k = dict(good, **change)
            rc = raw_call(ctx, k["data"], k["es"], k["n"], k["cap"], k["values"], k["starts"], k["positions"], k["inverse"], k["num"])
            err = ctx._L.msd_last_error(ctx._h).decode()
            assert rc == -1 and message in err, (change, rc, err)
            for b in bufs:
                assert b.unchanged(), change
                b.check(str(change))

        for bad in (0, 2, 3, 16, -4):
            refused("elem_bytes", es=bad)
        refused("d_num_runs", num=0)
        refused("null data", data=0)
        for name, ptr in good.items():
            if name in ("data", "values"):
                for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                    refused("aligned", **{name: ptr + d})
            elif name in ("starts", "positions", "inverse", "num"):
                for d in (1, 4):
                    refused("aligned", **{name: ptr + d})
        refused("2^36", n=1 << 36)
        refused("2^36", n=(1 << 64) - 1)
        refused("d_positions without d_inverse", inverse=0)
        # every output against the input, the positions and the other outputs
        w = 8 // es   # elements of the input per word
        refused("overlap", values=din.ptr)
        refused("overlap", values=din.ptr + (n - 1) * es)
        refused("overlap", starts=din.ptr + 8 * (n // 2 // w))
        refused("overlap", inverse=din.ptr + 8 * (n // w - 1))
        refused("overlap", num=din.ptr)
        refused("overlap", num=din.ptr + (n * es - 8))
        refused("overlap", values=dpos.ptr)
        refused("overlap", starts=dpos.ptr + 8 * (n - 1))
        refused("overlap", inverse=dpos.ptr)
        refused("overlap", num=dpos.ptr + 8)
        refused("overlap", values=dst.ptr + 8 * n)               # the last word of the starts
        refused("overlap", values=dinv.ptr)
        refused("overlap", starts=dinv.ptr + 8 * (n - 1))
        refused("overlap", num=dval.ptr)
        refused("overlap", num=dst.ptr + 8 * n)
        refused("overlap", num=dinv.ptr + 8 * 5)
        refused("overlap", inverse=dst.ptr, positions=0)
        # and the call that all of these were changes of is fine
        ctx._ok(raw_call(ctx, *[good[k] for k in ("data", "es", "n", "cap", "values", "starts", "positions", "inverse", "num")]))
        m, ev, es_, einv = R.expected(a, np.arange(n))
        assert int(dnum.host()[0]) == m and (dval.host()[:m] == ev).all() and (dinv.host().view(np.int64) == einv).all()


def test_capacity_bounds_the_extents_that_must_not_overlap(ctx):
    """d_values and d_starts are taken as min(cap, n) and min(cap, n) + 1 elements: a cap beyond n claims no more memory"""
    es, n = 4, 100
    a = R.make("distinct", n, es, 64)
    din, dval, dst, dnum = Buf(es, n, a=a), Buf(es, n), Buf(8, n + 1), Buf(8, 1)
    ctx._ok(raw_call(ctx, din.ptr, es, n, (1 << 64) - 1, dval.ptr, dst.ptr, 0, 0, dnum.ptr))
    assert int(dnum.host()[0]) == n and (dval.host() == a).all() and dst.host().view(np.int64).tolist() == list(range(n + 1))
    for b in (din, dval, dst, dnum):
        b.check("huge cap")


# ---- asynchrony

@pytest.mark.parametrize("es", WIDTHS)
def test_two_calls_back_to_back_before_any_synchronise(ctx, es):
    """the second call reuses the first one's workspace: only stream order keeps them apart"""
    import torch
    tile, scan_tile = limits(ctx, es)
    n1, n2 = (scan_tile + 1) * tile + 5, 3 * tile - 1
    a1, a2 = R.make("geo1.5", n1, es, tile, seed=21), R.make("alternating", n2, es, tile)
    t1, t2 = torch.from_numpy(a1.view(R.IT[es])).cuda(), torch.from_numpy(a2.view(R.IT[es])).cuda()
    ctx.run_encode(t2)                      # (the workspace has its size: no reallocation, which would synchronise)
    ctx.run_encode(t1)
    torch.cuda.synchronize()
    r1 = ctx.run_encode(t1, inverse=True)
    r2 = ctx.run_encode(t2, inverse=True)
    r3 = ctx.run_encode(t1, cap=10, inverse=True)
    torch.cuda.synchronize()
    for (num, vals, st, inv), a, cap in ((r1, a1, n1), (r2, a2, n2), (r3, a1, 10)):
        m, ev, es_, einv = R.expected_capped(a, cap)
        k = min(m, cap)
        assert int(num.item()) == m and num.dtype == torch.int64 and num.numel() == 1
        assert vals.dtype == t1.dtype and vals.numel() == cap and st.numel() == cap + 1 and inv.numel() == a.size
        assert (vals.cpu().numpy().view(R.UT[es])[:k] == ev).all()
        assert (st.cpu().numpy()[:k + 1] == es_).all()
        assert (inv.cpu().numpy() == einv).all()


# ---- the Python wrappers

def test_run_encode_wrapper_outputs_and_phase(ctx):
    import torch
    t = torch.tensor([1.0, 1.0, -0.0, 0.0, 0.0, 2.0], device="cuda")
    num, vals, st, inv = ctx.run_encode(t, values=False, starts=False)
    assert int(num.item()) == 4 and vals is None and st is None and inv is None
    before = ctx.workspace_bytes
    assert before > 0
    ctx.set_profiling(True)
    try:
        num, vals, st, inv = ctx.run_encode(t, inverse=True)
        assert [p[0] for p in ctx.phases()] == ["run_encode"]
    finally:
        ctx.set_profiling(False)
    assert vals.dtype == torch.float32 and vals[:4].tolist() == [1.0, 0.0, 0.0, 2.0] and torch.signbit(vals[1]).item()
    assert st[:5].tolist() == [0, 2, 3, 5, 6] and inv.tolist() == [0, 0, 1, 2, 2, 3]
    assert ctx.run_encode_limits(4) == limits(ctx, 4) and ctx.run_encode_limits(8) == limits(ctx, 8)
    s = t[1:4]                                                   # a slice: 4 bytes off the 16-byte grid
    num, vals, st, _ = ctx.run_encode(s)
    assert int(num.item()) == 3 and st.tolist() == [0, 1, 2, 3]


UNIQUE_TYPES = [E.U32, E.I32, E.F32, E.U64, E.I64, E.F64]


def _unique_input(kt, n, kind):
    ut = E.UT[kt]
    W = 8 * np.dtype(ut).itemsize
    rng = np.random.default_rng(E.seed_of(kt, n))
    if kind == "distinct":
        return R.distinct(n, W // 8, seed=kt)[rng.permutation(n)]
    z = np.minimum(rng.zipf(1.3, n), 5000).astype(np.int64)      # Zipf-like: a few values hold most of the elements
    if kt % 3 == 2:
        ft = np.float32 if W == 32 else np.float64
        table = np.r_[np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], ft), rng.standard_normal(5000).astype(ft)].view(ut)
    else:
        table = np.r_[np.array([0, 1, (1 << W) - 1, 1 << (W - 1), (1 << (W - 1)) - 1], dtype=ut), rng.integers(0, 1 << W, 5000, dtype=ut)]
    return table[z]


@pytest.mark.parametrize("kind", ["zipf", "distinct"])
@pytest.mark.parametrize("n", [0, 1, 100003])
@pytest.mark.parametrize("kt", UNIQUE_TYPES, ids=[E.NAMES[k] for k in UNIQUE_TYPES])
def test_unique(ctx, kt, n, kind):
    import torch
    ut = E.UT[kt]
    es = np.dtype(ut).itemsize
    bits = _unique_input(kt, n, kind)
    dt = {E.I32: torch.int32, E.F32: torch.float32, E.I64: torch.int64, E.F64: torch.float64}.get(kt)
    t = torch.from_numpy(bits.view(R.IT[es])).cuda()
    if dt is None:
        name = "uint32" if kt == E.U32 else "uint64"
        assert hasattr(torch, name), "this torch has no %s" % name
        dt = getattr(torch, name)
    t = t.view(dt)
    codes, inv, counts = np.unique(E.np_encode(bits, kt), return_inverse=True, return_counts=True)
    want = E.np_decode(codes, kt)
    host = D.bits
    v = ctx.unique(t)
    assert v.dtype == dt and (host(v) == want).all() and host(v).size == want.size
    v, c = ctx.unique(t, return_counts=True)
    assert (host(v) == want).all() and c.dtype == torch.int64 and (c.cpu().numpy() == counts).all()
    v, i = ctx.unique(t, return_inverse=True)
    assert (host(v) == want).all() and i.dtype == torch.int64 and (i.cpu().numpy() == inv.reshape(-1)).all()
    v, i, c = ctx.unique(t, return_inverse=True, return_counts=True)
    assert (host(v) == want).all() and (i.cpu().numpy() == inv.reshape(-1)).all() and (c.cpu().numpy() == counts).all()
    assert (host(t) == bits).all()                               # the input is what it was
