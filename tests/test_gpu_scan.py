"""GPU tests of scan-by-key over runs (msd_scan_runs; MsdContext.scan_runs): per element the running sum, minimum, maximum
or count inside its run of equal keys, inclusive or exclusive, for 4- and 8-byte keys and the six value types.  d_positions
and MSD_SCAN_SCATTER are in the signature and not offered yet: every call that passes positions must be refused.

The expected result is defined in tests/scan_expect.py.  Integer sums, counts, float sums of small integers (the EXACT part:
values from [-2^20, 2^20] and n <= 2^24, so every partial sum in any order stays below 2^44 and is exact in a double) and
every minimum and maximum are compared exactly -- min / max BITWISE --, float sums of N(0,1) values against the sequential
float64 cumsum within the bound that holds for every order of summation.  The calls go through the C ABI on integer tensors
that carry the bit patterns, with EVERY buffer -- keys, values, d_out -- inside a guardband.Arena whose payload is
pre-filled with a known pattern and is larger than the buffer: a case checks the n results, that the payload in front of
and behind them is what it was, that no guard was touched and that the inputs are what was uploaded.  The buffers are
guardband.Buf; the key patterns and the value columns are those of tests/test_gpu_reduce.py.  The Python wrapper has tests of its own at the end."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_support as D
import guardband
import reduce_expect as X
import runs_expect as R
import scan_expect as S
import sort_rows_expect as E
import test_gpu_reduce as G                                         # (Inputs, make_keys, make_values, specials: the family's helpers, no fixtures)
from guardband import Buf

pytestmark = pytest.mark.gpu

WIDTHS = E.WIDTHS
OPS = ("sum", "min", "max", "count")
VT_IDS = [E.NAMES[v] for v in X.VAL_TYPES]
BIG_PATTERNS = ["equal", "distinct", "geo5000"] + G.CARRY_PATTERNS
JUNK_VT = 77                                                        # what a count passes for val_type


def limits(ctx, kb):
    tile, scan_tile = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_scan_runs_limits(kb, C.byref(tile), C.byref(scan_tile)) == 0
    return int(tile.value), int(scan_tile.value)


def obytes(vt, op):
    return 8 if op in ("sum", "count") else G.vbytes(vt)


def raw_call(ctx, keys_ptr, kb, n, vals_ptr, vt, positions_ptr, op, flags, out_ptr):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_scan_runs(ctx._h, vp(keys_ptr), kb, n, vp(vals_ptr), vt, vp(positions_ptr), op, flags, vp(out_ptr))


def compare(got, want, vt, op, what):
    """exact: integer sums, counts and min / max bitwise, float sums numerically (a zero of either sign is a zero)"""
    if op == "sum" and vt in X.FLOAT:
        g = got.view(np.float64)
        assert np.array_equal(g, want, equal_nan=True), (what, "float sums differ", int(np.argmax(~((g == want) | (np.isnan(g) & np.isnan(want))))))
    else:
        w = want.view(got.dtype)
        assert (got == w).all(), (what, "results differ", int(np.argmax(got != w)), int(got[np.argmax(got != w)]), int(w[np.argmax(got != w)]))


EXTRA = 3                                                           # elements of d_out's payload behind the n results


def scan_case(ctx, inp, vbits, vt, op, flags=0, val_off=0, val_lead=0, out_off=0, out_lead=0, what="", exact=True):
    """one call, everything checked; returns the n results as unsigned words.  d_out's payload has `out_off` elements in
    front of the results and EXTRA behind them, which must stay what they were.  A count gets no values: a null pointer
    and a junk val_type."""
    n = inp.n
    count = op == "count"
    ob = obytes(vt, op)
    what = (what, inp.where, "count" if count else E.NAMES[vt], op, flags, val_off, val_lead, out_off, out_lead)
    dval = None if count else Buf(G.vbytes(vt), n, val_off, val_lead, vbits)
    dout = Buf(ob, n + EXTRA, out_off, out_lead)
    ctx._ok(raw_call(ctx, inp.dkeys.ptr, inp.kb, n, dval and dval.ptr, JUNK_VT if count else vt, inp.dpos and inp.dpos.ptr, S.OPS[op], flags, dout.ptr))
    got = dout.host()[:n]
    if exact:
        want = S.expected(inp.keys, vbits, vt, op, exclusive=bool(flags & S.EXCLUSIVE), positions=inp.positions, scatter=bool(flags & S.SCATTER))
        compare(got, want, vt, op, what)
    assert dout.untouched_from(n), (what, "d_out written beyond its n elements")
    assert inp.dkeys.unchanged(), (what, "the keys changed")
    assert dval is None or dval.unchanged(), (what, "the values changed")
    if inp.dpos is not None:
        assert inp.dpos.unchanged(), (what, "the positions changed")
    for name, b in (("keys", inp.dkeys), ("values", dval), ("positions", inp.dpos), ("d_out", dout)):
        if b is not None:
            b.check("%s of %s" % (name, what))
    return got


# ---- geometry: sizes x run patterns, both key widths

GEOMETRY = [(size, p) for size in R.SIZE_NAMES for p in R.PATTERNS + G.CARRY_PATTERNS if size != "big" or p in BIG_PATTERNS]


@pytest.mark.parametrize("size,pattern", GEOMETRY, ids=["%s-%s" % sp for sp in GEOMETRY])
@pytest.mark.parametrize("kb", WIDTHS)
def test_sizes_and_patterns(ctx, kb, size, pattern):
    tile, scan_tile = limits(ctx, kb)
    n = R.sizes(tile, scan_tile)[size]
    keys = G.make_keys(pattern, n, kb, tile, seed=E.seed_of(kb, n))
    inp = G.Inputs(keys)
    # the reductions of the carry: u64 and double sums, 4- and 8-byte codes, and the count; inclusive and exclusive in turn
    calls = ((E.U32, "sum"), (E.F64, "sum"), (E.F32 if kb == 4 else E.I64, "min"), (E.I64 if kb == 4 else E.F32, "max"), (E.U32, "count"))
    turn = R.SIZE_NAMES.index(size) + len(pattern)
    for j, (vt, op) in enumerate(calls):
        vbits = None if op == "count" else G.make_values(vt, op, keys, 1)
        scan_case(ctx, inp, vbits, vt, op, flags=(turn + j) % 2, what=pattern)


def test_the_geometry_cases_are_what_the_list_says():
    assert len(GEOMETRY) == 12 * 11 + 5 and len(R.SIZE_NAMES) == 13 and len(R.PATTERNS) == 9


# ---- types: every value type x op x inclusive / exclusive, exact (float sums: the exact part)

def refused_case(ctx, inp, vt, op, flags, message):
    """the call is refused with `message`, and neither d_out nor an input is touched"""
    dout = Buf(obytes(vt, op), inp.n + EXTRA)
    rc = raw_call(ctx, inp.dkeys.ptr, inp.kb, inp.n, 0, JUNK_VT if op == "count" else vt, inp.dpos and inp.dpos.ptr, S.OPS[op], flags, dout.ptr)
    err = ctx._L.msd_last_error(ctx._h).decode()
    assert rc == -1 and message in err, (rc, err)
    for b in (dout, inp.dkeys, inp.dpos):
        if b is not None:
            assert b.unchanged()
            b.check(message)


@pytest.mark.parametrize("flags", [0, S.EXCLUSIVE], ids=["incl", "excl"])
@pytest.mark.parametrize("pattern", ["geo40", "geo5000", "equal"])
@pytest.mark.parametrize("size", ["T+1", "3T-1", "big"])
@pytest.mark.parametrize("vt", X.VAL_TYPES, ids=VT_IDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_types_ops_and_flags(ctx, kb, vt, size, pattern, flags):
    """every value type x every op x inclusive and exclusive at every size (MSD_SCAN_SCATTER needs positions, which are
    not offered yet: test_positions_are_refused)"""
    tile, scan_tile = limits(ctx, kb)
    n = R.sizes(tile, scan_tile)[size]
    assert n <= 1 << 24                                             # (what keeps the float sums of small integers exact)
    keys = G.make_keys(pattern, n, kb, tile, seed=E.seed_of(kb, n, vt))
    inp = G.Inputs(keys)
    for op in OPS:
        vbits = None if op == "count" else G.make_values(vt, op, keys, 2)
        got = scan_case(ctx, inp, vbits, vt, op, flags=flags, what=pattern)
        if vt in X.FLOAT and op in ("min", "max") and flags == 0 and pattern == "geo40":
            # the planted specials ARE running extremes: a zero, and a NaN of the sign that wins
            sign = E.UT[vt](1 << (8 * G.vbytes(vt) - 1))
            assert ((got == 0) | (got == sign)).any(), (pattern, op)
            assert (np.isnan(got.view(X.FLOAT[vt])) & (((got & sign) != 0) == (op == "min"))).any(), (pattern, op)


# ---- float sums, rounded part

@pytest.mark.parametrize("pattern", ["geo5000", "equal"])
@pytest.mark.parametrize("vt", [E.F32, E.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kb", WIDTHS)
def test_float_sums_within_the_bound_of_any_order_and_reproducible(ctx, kb, vt, pattern):
    """|got_i - ref_i| <= 2 * L_i * 2^-53 * sum_{j <= i} |x_j| with ref the sequential float64 cumsum of the run and L_i
    the length of the prefix: both sides are within L u sum|x| of the exact value in any order of L - 1 double additions
    (L^2 < 2^53; a float32 converts exactly and the identity's additions are exact).  The exclusive result is held to the
    same bound of the prefix in front of the element."""
    tile, scan_tile = limits(ctx, kb)
    n = R.sizes(tile, scan_tile)["big"]
    keys = G.make_keys(pattern, n, kb, tile, seed=7)
    vals = np.random.default_rng(E.seed_of(kb, vt, 99)).standard_normal(n).astype(X.FLOAT[vt])
    vbits = vals.view(E.UT[vt])
    inp = G.Inputs(keys)
    got = scan_case(ctx, inp, vbits, vt, "sum", what=pattern, exact=False)
    again = scan_case(ctx, inp, vbits, vt, "sum", what=pattern, exact=False)
    assert (got == again).all(), "the same call gave other bits"
    excl = scan_case(ctx, inp, vbits, vt, "sum", flags=S.EXCLUSIVE, what=pattern, exact=False).view(np.float64)
    _, _, starts, _ = R.expected(keys)
    ref = S.inclusive(starts, vbits, vt, "sum")
    sabs = S.seg_accumulate(np.add, np.abs(vals.astype(np.longdouble)), starts)   # (64-bit significands: 2^-11 of the bound's unit)
    length = np.arange(n) - np.repeat(starts[:-1], np.diff(starts)) + 1
    bound = np.longdouble(2.0) * length * np.longdouble(2.0) ** -53 * sabs
    err = np.abs(got.view(np.float64).astype(np.longdouble) - ref)
    worst = float(np.max(err / bound))
    print("worst error / bound: %.3g over %d elements in %d runs" % (worst, n, starts.size - 1))
    assert (err <= bound).all(), (pattern, int(np.argmax(err > bound)), worst)
    inner = np.ones(n, bool)
    inner[starts[:-1]] = False
    assert (excl[~inner] == 0.0).all() and not np.signbit(excl[~inner]).any()       # the identity at the heads: +0.0
    at = np.flatnonzero(inner)
    assert (np.abs(excl[at].astype(np.longdouble) - ref[at - 1]) <= bound[at - 1]).all()


@pytest.mark.parametrize("vt", [E.F32, E.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kb", WIDTHS)
def test_float_sums_of_infinities_and_nans(ctx, kb, vt):
    """an infinity or a NaN reaches every later element of its run and no other run"""
    tile, _ = limits(ctx, kb)
    n = 4 * tile - 1
    ft = X.FLOAT[vt]
    lengths = [5, tile // 2, 7, 2 * tile, 9, 1, 1, 1]               # run 3 spans three tiles, the last run two
    lengths += [n - sum(lengths)]
    keys = R.from_runs(lengths, kb, seed=3)
    starts = np.r_[0, np.cumsum(lengths)]
    vals = np.random.default_rng(5).standard_normal(n).astype(ft)
    vals[starts[0] + 2] = np.inf                                    # run 0: +inf
    vals[starts[1] + 1] = np.nan                                    # run 1: a NaN
    vals[starts[2]], vals[starts[2] + 6] = np.inf, -np.inf          # run 2: both infinities: a NaN at its last element only
    vals[starts[3] + 3], vals[starts[4] - 2] = -np.inf, np.inf      # run 3: both infinities, two tiles apart
    vals[starts[4] + 8] = -np.inf                                   # run 4: -inf at its last element
    vals[starts[5]], vals[starts[6]], vals[starts[7]] = np.inf, np.nan, -0.0
    vals[n - 1] = np.inf                                            # run 8: +inf in its second tile
    for flags in (0, S.EXCLUSIVE):
        g = scan_case(ctx, G.Inputs(keys), vals.view(E.UT[vt]), vt, "sum", flags=flags, exact=False).view(np.float64)
        ref = S.expected(keys, vals.view(E.UT[vt]), vt, "sum", exclusive=bool(flags))
        special = ~np.isfinite(ref)
        assert (np.isnan(g) == np.isnan(ref)).all() and (np.isinf(g) == np.isinf(ref)).all() and (g[np.isinf(ref)] == ref[np.isinf(ref)]).all()
        assert np.allclose(g[~special], ref[~special], rtol=0, atol=1e-9 * tile)
        k = 0 if flags else 1                                       # (exclusive: the element itself is not part of its result)
        assert special[starts[0] + 3 - k:starts[1]].all() and not special[starts[0]:starts[0] + 2].any()
        assert np.isnan(g[starts[1] + 2 - k:starts[2]]).all() and np.isfinite(g[starts[1]])
        assert (g[starts[3] + 4 - k:starts[4] - 2] == -np.inf).all() and np.isnan(g[starts[4] - 1])
        assert np.isfinite(g[starts[4]:starts[4] + 8]).all() and np.isfinite(g[starts[8]:n - 1]).all()
        if not flags:
            assert g[n - 1] == np.inf and g[starts[7]] == 0.0 and np.isnan(g[starts[6]]) and g[starts[5]] == np.inf


# ---- relations between the results, and to reduce_runs and run_encode

@pytest.mark.parametrize("kb", WIDTHS)
def test_relations(ctx, kb):
    import torch
    tile, scan_tile = limits(ctx, kb)
    host = D.bits
    for n, pattern in ((3 * tile - 1, "geo40"), ((scan_tile + 1) * tile + 5, "geo5000"), (2 * tile + 1, "tile_runs_half")):
        keys = G.make_keys(pattern, n, kb, tile, seed=12)
        t = torch.from_numpy(keys.view(R.IT[kb])).cuda()
        num, _, st, _ = ctx.run_encode(t)
        m = int(num.item())
        starts = st.cpu().numpy()[:m + 1]
        last = starts[1:] - 1
        inner = np.ones(n, bool)
        inner[starts[:-1]] = False
        at = np.flatnonzero(inner)
        for vt, op in ((E.I64, "sum"), (E.U32, "sum"), (E.F32, "min"), (E.F64, "max"), (E.I32, "max"), (E.U64, "min")):
            vbits = G.make_values(vt, op, keys, 14)
            dt = {E.I64: torch.int64, E.F32: torch.float32, E.F64: torch.float64, E.I32: torch.int32}.get(vt)
            v = torch.from_numpy(vbits.view(R.IT[vbits.itemsize])).cuda()
            if dt is None:
                name = "uint32" if vt == E.U32 else "uint64"
                assert hasattr(torch, name), "this torch has no %s" % name
                dt = getattr(torch, name)
            v = v.view(dt)
            incl, excl = host(ctx.scan_runs(t, v, op=op)), host(ctx.scan_runs(t, v, op=op, exclusive=True))
            assert (excl[at] == incl[at - 1]).all(), (pattern, op, "exclusive is not the inclusive result of the element in front")
            num_r, red = ctx.reduce_runs(t, v, op=op)
            assert int(num_r.item()) == m and (incl[last] == host(red)[:m]).all(), (pattern, op, "the last element of a run is not reduce_runs' result")
        incl, excl = host(ctx.scan_runs(t, None, op="count")), host(ctx.scan_runs(t, None, op="count", exclusive=True))
        assert (excl[at] == incl[at - 1]).all() and (excl[starts[:-1]] == 0).all()
        assert (incl[last] == np.diff(starts)).all(), (pattern, "the count at a run's last element is not its length")


# ---- positions: not offered yet; the caller gathers

@pytest.mark.parametrize("kb", WIDTHS)
def test_positions_are_refused_and_a_gathered_column_does_their_work(ctx, kb):
    """every call with d_positions is refused, with and without MSD_SCAN_SCATTER, and touches nothing; what positions are
    for -- the window function on a table sorted with positions -- is done with the value column gathered through them"""
    import torch
    tile, _ = limits(ctx, kb)
    rng = np.random.default_rng(3)
    for n in (1, 2, 65, tile + 1, 3 * tile - 1, 100003):
        x = R.geometric(n, kb, 3.0, seed=n)[rng.permutation(n)] & R.UT[kb](0xFFFF if n > 65 else 0x7)   # unsorted, many duplicates
        t = torch.from_numpy(x.view(R.IT[kb])).cuda()
        if kb == 4:
            s, pos = ctx.sort_rows(t, indices=True)
        else:
            s, pos = t.clone(), torch.arange(n, dtype=torch.int64, device="cuda")
            ctx.sort_typed(s, rids=pos)
        hs, hp = s.cpu().numpy().view(R.UT[kb]), pos.cpu().numpy()
        assert (x[hp] == hs).all()
        with_pos = G.Inputs(hs, hp)
        for j, (vt, op) in enumerate(((E.I64, "sum"), (E.F32, "max"), (E.U32, "min"), (E.F64, "sum"), (E.U32, "count"))):
            for flags in (0, S.EXCLUSIVE, S.SCATTER, S.SCATTER | S.EXCLUSIVE):
                refused_case(ctx, with_pos, vt, op, flags, "d_positions is not offered yet")
            vbits = None if op == "count" else G.make_values(vt, op, hs, 5)   # the column where the UNSORTED keys lie
            gathered = None if vbits is None else vbits[hp]
            got = scan_case(ctx, G.Inputs(hs), gathered, vt, op, flags=j % 2, what="gathered")
            compare(got, S.expected(hs, vbits, vt, op, exclusive=bool(j % 2), positions=hp), vt, op, "through positions, on the host")


# ---- alignment

@pytest.mark.parametrize("vb", WIDTHS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_alignment_of_keys_values_and_output(ctx, kb, vb):
    """the keys 4, 8 and 12 bytes off the 16-byte grid, the values at ANOTHER phase of it and the output at a third one
    (where its width leaves one), both widths against both"""
    tile, _ = limits(ctx, kb)
    full = R.make("geo1.5", 3 * tile, kb, tile, seed=9)
    sum_vt, mm_vt = (E.I32, E.F32) if vb == 4 else (E.F64, E.I64)
    turn = 0
    for koff in range(16 // kb):
        for voff in range(16 // vb):
            if koff * kb == voff * vb:
                continue
            for n in (1, 2, 3, 16 // kb - koff, 16 // kb - koff + 1, 65, tile - koff, tile + 1, 2 * tile + 1):
                keys = full[:n]
                vt, op = ((sum_vt, "sum"), (mm_vt, "min"), (mm_vt, "max"), (sum_vt, "count"))[turn % 4]
                ob = obytes(vt, op)
                third = [o for o in range(16 // ob) if o * ob not in (koff * kb, voff * vb)]
                turn += 1
                scan_case(ctx, G.Inputs(keys, key_off=koff), None if op == "count" else G.make_values(vt, op, keys, 8), vt, op, flags=turn // 4 % 2,
                          val_off=voff, out_off=third[turn % len(third)] if third else turn % (16 // ob), what="off")
    # all at the SAME phase too, for completeness
    keys = full[:tile + 3]
    scan_case(ctx, G.Inputs(keys, key_off=1), G.make_values(sum_vt, "sum", keys, 8), sum_vt, "sum", flags=S.EXCLUSIVE,
              val_off=kb // vb if kb >= vb else 0, out_off=kb // obytes(sum_vt, "sum"), what="same phase")


@pytest.mark.parametrize("vb", WIDTHS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_first_and_last_elements_of_a_page(ctx, kb, vb):
    """the first element of the keys / the values / the output is the first or the last element of a page, and so is the last one"""
    tile, _ = limits(ctx, kb)
    PAGE = guardband.PAGE
    full = R.make("geo1.5", 2 * PAGE, kb, tile, seed=10)
    vt = E.U32 if vb == 4 else E.F64
    # (lead, off) in elements of es bytes: the first element at the page's start / in the page's last element
    first = lambda es: (0, 0)
    last = lambda es: (PAGE - 16, 16 // es - 1)
    turn = 0
    for kplace, vplace, oplace in ((first, last, last), (last, first, first), (last, last, last), (first, first, first), (first, first, last)):
        (klead, koff), (vlead, voff) = kplace(kb), vplace(vb)
        ends = lambda lead, off, es: {(PAGE - (lead + off * es) % PAGE) // es, (PAGE - (lead + off * es) % PAGE) // es + 1}
        # n: the last element of the keys, of the values or of the output is the last / the first element of a page
        for op in ("sum", "max", "count"):
            ob = obytes(vt, op)
            olead, ooff = oplace(ob)
            for n in sorted({1, (2 * PAGE - (klead + koff * kb) % PAGE) // kb + 1} | ends(klead, koff, kb) | ends(vlead, voff, vb) | ends(olead, ooff, ob)):
                keys = full[:n]
                turn += 1
                scan_case(ctx, G.Inputs(keys, key_off=koff, key_lead=klead), None if op == "count" else G.make_values(vt, op, keys, 11), vt, op,
                          flags=turn % 2, val_off=voff, val_lead=vlead, out_off=ooff, out_lead=olead, what="page")


# ---- refusals through the C ABI

def test_refusals_in_order_touch_nothing(ctx):
    n = 1000
    for kb in WIDTHS:
        for vt, op in ((E.F32, 0), (E.I64, 1), (E.U32, 2), (E.F64, 0), (E.U32, 3)):
            vb, ob = G.vbytes(vt), 8 if op in (0, 3) else G.vbytes(vt)
            keys = R.make("geo1.5", n, kb, 64, seed=2)
            vbits = G.make_values(vt, OPS[op], keys, 3) if op != 3 else G.make_values(vt, "sum", keys, 3)
            din, dval, dout = Buf(kb, n, a=keys), Buf(vb, n, a=vbits), Buf(ob, n + EXTRA)
            dpos = Buf(8, n, a=np.arange(n, dtype=np.uint64))
            bufs = (din, dval, dout, dpos)
            count = op == 3
            good = dict(keys=din.ptr, kb=kb, n=n, vals=dval.ptr, vt=vt, positions=0, op=op, flags=(kb // 4 + op) % 2, out=dout.ptr)
            order = ("keys", "kb", "n", "vals", "vt", "positions", "op", "flags", "out")

            def refused(message, **change):
                k = dict(good, **change)
                rc = raw_call(ctx, *[k[a] for a in order])
                err = ctx._L.msd_last_error(ctx._h).decode()
                assert rc == -1 and message in err, (change, rc, err)
                for b in bufs:
                    assert b.unchanged(), change
                    b.check(str(change))

            # every refusal on its own
            for bad in (0, 2, 3, 16, -4):
                refused("key_bytes", kb=bad)
            for bad in (-1, 4, 100):
                refused("unknown op", op=bad)
            if not count:
                for bad in (-1, 6, 7, 100):
                    refused("val_type", vt=bad)
            for bad in (4, 8, 7, -1, 1 << 30):
                refused("unknown flags", flags=bad)
            for fl in (S.SCATTER, S.SCATTER | S.EXCLUSIVE):
                refused("without d_positions", flags=fl)
                refused("d_positions is not offered yet", positions=dpos.ptr, flags=fl)
            for fl in (0, S.EXCLUSIVE):
                refused("d_positions is not offered yet", positions=dpos.ptr, flags=fl)
                refused("d_positions is not offered yet", positions=dpos.ptr + 4, flags=fl)   # (whatever they are)
            refused("null keys", keys=0)
            if not count:
                refused("null values", vals=0)
            refused("null d_out", out=0)
            for name, es in (("keys", kb), ("vals", vb), ("out", ob)):
                if name == "vals" and count:
                    continue
                for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                    refused("aligned", **{name: good[name] + d})
            refused("2^36", n=1 << 36)
            refused("2^36", n=(1 << 64) - 1)
            refused("overlap", out=din.ptr)
            refused("overlap", out=din.ptr + (n * kb - ob))
            if not count:
                refused("overlap", out=dval.ptr + (n * vb - ob))
                refused("overlap", out=dval.ptr, vals=dval.ptr)
            # the order: of two faults the earlier one is reported
            refused("key_bytes", kb=5, op=9)
            refused("unknown op", op=9, vt=9)
            if not count:
                refused("val_type", vt=9, flags=4)
                refused("null keys", keys=0, vals=0)
                refused("null values", vals=0, out=0)
            refused("unknown flags", flags=6)
            refused("unknown flags", flags=4, positions=dpos.ptr)
            refused("without d_positions", flags=S.SCATTER, keys=0)
            refused("d_positions is not offered yet", positions=dpos.ptr, keys=0)
            refused("null keys", keys=0, out=0)
            refused("null d_out", out=0, keys=din.ptr + 1)
            refused("aligned", keys=din.ptr + 2, n=1 << 36)
            refused("2^36", n=1 << 36, out=din.ptr)
            # what is no fault: null pointers with n == 0; a count with a null d_vals, a misaligned one and a junk val_type
            ctx._ok(raw_call(ctx, 0, kb, 0, 0, vt, 0, op, 0, 0))
            ctx._ok(raw_call(ctx, 0, kb, 0, 0, vt, 0, op, S.EXCLUSIVE, 0))
            for b in bufs:
                assert b.unchanged()
            want = S.expected(keys, vbits, vt, OPS[op], exclusive=bool(good["flags"]))
            if count:
                for vals, junk in ((0, JUNK_VT), (dval.ptr + 1, -5), (dout.ptr, 6)):
                    ctx._ok(raw_call(ctx, din.ptr, kb, n, vals, junk, 0, op, good["flags"], dout.ptr))
                    compare(dout.host()[:n], want, vt, "count", "count without values")
                    dout.arena.fill(dout.fill)
            # and the call that all of these were changes of is fine
            ctx._ok(raw_call(ctx, *[good[a] for a in order]))
            compare(dout.host()[:n], want, vt, OPS[op], "good")
            assert dout.untouched_from(n) and din.unchanged() and dval.unchanged() and dpos.unchanged()
            for b in bufs:
                b.check("good")


def test_an_empty_array(ctx):
    for kb in WIDTHS:
        keys = np.zeros(0, R.UT[kb])
        for flags in (0, S.EXCLUSIVE):
            for vt, op in ((E.F32, "sum"), (E.I64, "min"), (E.U32, "count")):
                assert scan_case(ctx, G.Inputs(keys), None if op == "count" else np.zeros(0, E.UT[vt]), vt, op, flags=flags, what="empty").size == 0
        refused_case(ctx, G.Inputs(keys), E.U32, "max", S.SCATTER, "without d_positions")   # (refusals come before n == 0)


# ---- asynchrony and the workspace

@pytest.mark.parametrize("kb", WIDTHS)
def test_two_calls_back_to_back_with_a_run_encode_and_a_reduce_between(ctx, kb):
    """the calls share the slab: only stream order keeps them apart"""
    import torch
    tile, scan_tile = limits(ctx, kb)
    n1, n2 = (scan_tile + 1) * tile + 5, 3 * tile - 1
    k1, k2 = G.make_keys("tile_runs_half", n1, kb, tile, seed=21), G.make_keys("geo40", n2, kb, tile, seed=22)
    v1 = np.random.default_rng(1).integers(-(1 << 20), 1 << 20, n1).astype(np.float32)
    v2 = np.random.default_rng(2).integers(-(1 << 40), 1 << 40, n2)
    t1, t2 = torch.from_numpy(k1.view(R.IT[kb])).cuda(), torch.from_numpy(k2.view(R.IT[kb])).cuda()
    tv1, tv2 = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    ctx.reduce_runs(t1, tv1)                 # (the workspace has its size: no reallocation, which would synchronise)
    ctx.scan_runs(t1, tv1)
    torch.cuda.synchronize()
    r1 = ctx.scan_runs(t1, tv1)
    e = ctx.run_encode(t2, inverse=True)
    r2 = ctx.scan_runs(t2, tv2, op="min", exclusive=True)
    d = ctx.reduce_runs(t1, tv1, op="max")
    r3 = ctx.scan_runs(t1, tv1, op="max")
    r4 = ctx.scan_runs(t2, None, op="count")
    torch.cuda.synchronize()
    assert r1.dtype == torch.float64 and (r1.cpu().numpy() == S.expected(k1, v1.view(np.uint32), E.F32, "sum")).all()
    m2, ev, _, einv = R.expected(k2)
    assert int(e[0].item()) == m2 and (e[1].cpu().numpy().view(R.UT[kb])[:m2] == ev).all() and (e[3].cpu().numpy() == einv).all()
    assert r2.dtype == torch.int64 and (r2.cpu().numpy() == S.expected(k2, v2.view(np.uint64), E.I64, "min", exclusive=True).view(np.int64)).all()
    m1, _, w = X.expected(k1, v1.view(np.uint32), E.F32, "max")
    assert int(d[0].item()) == m1 and (d[1].cpu().numpy().view(np.uint32)[:m1] == w).all()
    assert r3.dtype == torch.float32 and (r3.cpu().numpy().view(np.uint32) == S.expected(k1, v1.view(np.uint32), E.F32, "max")).all()
    assert r4.dtype == torch.int64 and (r4.cpu().numpy().view(np.uint64) == S.expected(k2, None, 0, "count")).all()


def test_workspace_grows_by_no_more_than_the_records(ctx):
    """per tile and per scan piece one 8-byte tail and one 4-byte flag (256-byte aligned arrays), and nothing of what
    run_encode takes; the slab grows in steps of 1 MiB with an eighth on top"""
    import torch
    from inplacemsdradixsort_amd import MsdContext
    kb = 4
    tile, scan_tile = limits(ctx, kb)
    n = (scan_tile + 1) * tile + 5
    t = torch.from_numpy(G.make_keys("geo40", n, kb, tile).view(np.int32)).cuda()
    v = torch.ones(n, dtype=torch.float32, device="cuda")
    tiles = -(-n // tile)
    pieces = -(-tiles // scan_tile)
    records = 12 * (tiles + pieces) + 4 * 256 + 4096
    step = 1 << 20
    own = MsdContext(0)
    try:
        before = own.workspace_bytes
        out = own.scan_runs(t, v)
        after = own.workspace_bytes
        assert 0 <= after - before <= -(-(records + records // 8) // step) * step, (before, after, records)
        own.run_encode(t)                                         # (run_encode's words need no more room than the records)
        own.scan_runs(t, v, op="max", exclusive=True)
        assert own.workspace_bytes == after
        assert (out.cpu().numpy() == S.expected(t.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32), E.F32, "sum")).all()
    finally:
        own.close()


# ---- the Python wrapper

def test_scan_runs_wrapper_outputs_and_phase(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdError
    k = torch.tensor([1.0, 1.0, -0.0, 0.0, 0.0, 2.0], device="cuda")                  # runs: [0, 2) [2, 3) [3, 5) [5, 6): the zeros differ
    v = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int32, device="cuda")
    ctx.set_profiling(True)
    try:
        out = ctx.scan_runs(k, v)
        assert [p[0] for p in ctx.phases()] == ["scan_runs"]
    finally:
        ctx.set_profiling(False)
    assert out.dtype == torch.int64 and out.tolist() == [1, 3, 3, 4, 9, 6]
    assert ctx.scan_runs(k, v, exclusive=True).tolist() == [0, 1, 0, 0, 4, 0]
    out = ctx.scan_runs(k, v, op="max")
    assert out.dtype == torch.int32 and out.tolist() == [1, 2, 3, 4, 5, 6]
    assert ctx.scan_runs(k, v, op="max", exclusive=True).tolist() == [-(1 << 31), 1, -(1 << 31), -(1 << 31), 4, -(1 << 31)]
    assert ctx.scan_runs(k, v, op="min", exclusive=True).tolist() == [(1 << 31) - 1, 1, (1 << 31) - 1, (1 << 31) - 1, 4, (1 << 31) - 1]
    for vals in (None, v, k):
        out = ctx.scan_runs(k, vals, op="count")
        assert out.dtype == torch.int64 and out.tolist() == [1, 2, 1, 1, 2, 1]
    assert ctx.scan_runs(k, None, op="count", exclusive=True).tolist() == [0, 1, 0, 0, 1, 0]
    pos = torch.tensor([5, 4, 3, 2, 1, 0], device="cuda")
    out = ctx.scan_runs(k, v.double()[pos])                           # the column gathered through positions
    assert out.dtype == torch.float64 and out.tolist() == [6.0, 11.0, 4.0, 3.0, 5.0, 1.0]
    for kw in ({}, {"scatter": True}, {"op": "count"}, {"op": "max", "exclusive": True}):
        with pytest.raises(MsdError, match="not offered yet"):
            ctx.scan_runs(k, v, positions=pos, **kw)
    assert ctx.scan_runs(k.double(), v.long(), op="sum").dtype == torch.int64 and ctx.scan_runs(k, v.float(), op="min").dtype == torch.float32
    if hasattr(torch, "uint32") and hasattr(torch, "uint64"):
        out = ctx.scan_runs(k, v.view(torch.uint32))
        assert out.dtype == torch.uint64 and out.view(torch.int64).tolist() == [1, 3, 3, 4, 9, 6]
    # a small worked example with both zeros and a NaN: a running maximum takes the NaN and keeps it, torch.cummax-like
    # only in that; the minimum is not touched by it, and -0.0 is below +0.0
    one = torch.ones(6, dtype=torch.int32, device="cuda")
    f = torch.tensor([1.0, float("nan"), 0.0, -0.0, float("-inf"), 7.0], device="cuda")
    mx, mn = ctx.scan_runs(one, f, op="max"), ctx.scan_runs(one, f, op="min")
    assert mx[0].item() == 1.0 and all(math.isnan(x) for x in mx[1:].tolist())
    assert mn[:2].tolist() == [1.0, 1.0] and mn[2].item() == 0.0 and not torch.signbit(mn[2]).item()
    assert mn[3].item() == 0.0 and torch.signbit(mn[3]).item() and mn[4:].tolist() == [float("-inf")] * 2
    ex = ctx.scan_runs(one, f, op="max", exclusive=True)
    assert ex.view(torch.int32)[0].item() == -1 and ex[1].item() == 1.0 and math.isnan(ex[2].item())   # the identity: the -NaN of all ones
    ex = ctx.scan_runs(one, f, op="min", exclusive=True)
    assert ex.view(torch.int32)[0].item() == 0x7FFFFFFF and ex[1:3].tolist() == [1.0, 1.0]
    assert ctx.scan_runs_limits(4) == limits(ctx, 4) and ctx.scan_runs_limits(8) == limits(ctx, 8)
    s, sv = k[1:4], v[2:5]                                            # slices: 4 and 8 bytes off the 16-byte grid
    assert ctx.scan_runs(s, sv).tolist() == [3, 4, 5] and ctx.scan_runs(s, sv, op="count").tolist() == [1, 1, 1]
    s, sv = k[3:6], v[1:4]                                            # 12 and 4 bytes off
    assert ctx.scan_runs(s, sv, exclusive=True).tolist() == [0, 2, 0] and ctx.scan_runs(s, sv, op="max").tolist() == [2, 3, 4]
    assert ctx.scan_runs(k[:0], v[:0]).numel() == 0 and ctx.scan_runs(k[:0], None, op="count").dtype == torch.int64
