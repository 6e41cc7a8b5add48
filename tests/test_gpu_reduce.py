"""GPU tests of reduce-by-key over runs (msd_reduce_runs; MsdContext.reduce_runs / group_reduce): per run of equal keys the
sum, the minimum or the maximum of a value column, directly or through positions, and the true number of runs, for 4- and
8-byte keys and the six value types.

The expected result is defined in tests/reduce_expect.py.  Integer sums, float sums of small integers (the EXACT part: values
from [-2^20, 2^20] and n <= 2^24, so every partial sum in any order stays below 2^44 and is exact in a double) and every
minimum and maximum are compared exactly -- min / max BITWISE --, float sums of N(0,1) values against math.fsum within the
bound that holds for every order of summation.  The calls go through the C ABI on integer tensors that carry the bit
patterns, with EVERY buffer -- keys, values, positions, d_out, num_runs -- inside a guardband.Arena whose payload is
pre-filled with a known pattern: a case checks what was written, that the rest of d_out is what it was, that no guard was
touched and that the inputs are what was uploaded.  The Python wrappers have tests of their own at the end."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_support as D
import guardband
import reduce_expect as X
import runs_expect as R
import sort_rows_expect as E
from guardband import Buf

pytestmark = pytest.mark.gpu

WIDTHS = E.WIDTHS
OPS = ("sum", "min", "max")
VT_IDS = [E.NAMES[v] for v in X.VAL_TYPES]


def limits(ctx, kb):
    tile, scan_tile = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_reduce_runs_limits(kb, C.byref(tile), C.byref(scan_tile)) == 0
    return int(tile.value), int(scan_tile.value)


def vbytes(vt):
    return 4 if vt < E.U64 else 8


def obytes(vt, op):
    return 8 if op == "sum" else vbytes(vt)


def raw_call(ctx, keys_ptr, kb, n, vals_ptr, vt, positions_ptr, op, cap, out_ptr, num_ptr):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_reduce_runs(ctx._h, vp(keys_ptr), kb, n, vp(vals_ptr), vt, vp(positions_ptr), op, cap, vp(out_ptr), vp(num_ptr))


class Inputs:
    """the keys (and the positions) of a case on the device, shared by the calls of the case"""

    def __init__(self, keys, positions=None, key_off=0, key_lead=0):
        self.keys, self.positions = keys, positions
        self.kb, self.n = keys.itemsize, keys.size
        self.dkeys = Buf(self.kb, self.n, key_off, key_lead, keys)
        self.dpos = Buf(8, self.n, a=positions.astype(np.uint64)) if positions is not None else None
        self.where = (self.kb, self.n, key_off, key_lead, positions is not None)


def compare(got, want, vt, op, what):
    """exact: integer sums and min / max bitwise, float sums numerically (a zero of either sign is a zero)"""
    if op == "sum" and vt in X.FLOAT:
        g = got.view(np.float64)
        assert np.array_equal(g, want, equal_nan=True), (what, "float sums differ", int(np.argmax(~((g == want) | (np.isnan(g) & np.isnan(want))))))
    else:
        w = want.view(got.dtype)
        assert (got == w).all(), (what, "results differ", int(np.argmax(got != w)))


def reduce_case(ctx, inp, vbits, vt, op, cap=None, val_off=0, val_lead=0, out_off=0, what="", exact=True):
    """one call, everything checked; returns (m, the first min(m, cap) elements of d_out as unsigned words).  Without a
    `cap` d_out has room for every run and three elements more, which must stay what they were."""
    n = inp.n
    m, _, want = X.expected(inp.keys, vbits, vt, op, inp.positions)
    cap = min(n, m + 3) if cap is None else cap
    ob = obytes(vt, op)
    what = (what, inp.where, E.NAMES[vt], op, cap, val_off, val_lead, out_off)
    dval = Buf(vbytes(vt), n, val_off, val_lead, vbits)
    dout = Buf(ob, cap, out_off)
    dnum = Buf(8, 1)
    ctx._ok(raw_call(ctx, inp.dkeys.ptr, inp.kb, n, dval.ptr, vt, inp.dpos and inp.dpos.ptr, X.OPS[op], cap, dout.ptr, dnum.ptr))
    k = min(m, cap)
    assert int(dnum.host()[0]) == m, (what, "num_runs", int(dnum.host()[0]), m)
    got = dout.host()[:k]
    if exact:
        compare(got, want[:k], vt, op, what)
    assert dout.untouched_from(k), (what, "d_out written beyond min(m, cap)")
    assert inp.dkeys.unchanged(), (what, "the keys changed")
    assert dval.unchanged(), (what, "the values changed")
    if inp.dpos is not None:
        assert inp.dpos.unchanged(), (what, "the positions changed")
    for name, b in (("keys", inp.dkeys), ("values", dval), ("positions", inp.dpos), ("d_out", dout), ("num_runs", dnum)):
        if b is not None:
            b.check("%s of %s" % (name, what))
    return m, got


# ---- inputs

def make_keys(pattern, n, kb, tile, seed=1):
    """runs_expect's patterns and two that stress the carry across tiles"""
    if pattern == "long_middle":       # ONE run from the middle of tile 0 to the middle of the last tile, heads on both sides of it
        a = R.distinct(n, kb, seed)
        c = R.UT[kb](0x00C0FFEE)
        a[a == c] = c + R.UT[kb](1)
        last = (n - 1) // tile * tile if n else 0
        first = min(tile, n) // 2
        a[first:max(last + (n - last) // 2, first)] = c
        return a
    if pattern == "tile_runs_half":    # runs of exactly `tile` elements, offset by half a tile: every tile has ONE head and an open lead
        lengths = np.r_[tile // 2, np.full(n // tile + 2, tile)]
        return R.from_runs(lengths, kb, seed)[:n]
    return R.make(pattern, n, kb, tile, seed)


CARRY_PATTERNS = ["long_middle", "tile_runs_half"]


def specials(vt):
    """bit patterns: +-0, +-inf, the smallest and largest denormals of both signs, +-NaN with two payloads each"""
    if vt == E.F32:
        sign, inf, q, dmax = 0x80000000, 0x7F800000, 0x7FC00000, 0x007FFFFF
    else:
        sign, inf, q, dmax = 1 << 63, 0x7FF << 52, 0x7FF8 << 48, (1 << 52) - 1
    pos = [0, inf, 1, dmax, q, q | 0x1234]
    return np.array(pos + [p | sign for p in pos], E.UT[vt])


def make_values(vt, op, keys, seed):
    """values of type vt (unsigned bit patterns) for the keys' runs: wrapping integers, small integers as floats for a sum,
    float specials planted so that each is the extreme of some run for min / max"""
    n = keys.size
    ut = E.UT[vt]
    W = 8 * np.dtype(ut).itemsize
    rng = np.random.default_rng(E.seed_of(vt, n, seed))
    if vt not in X.FLOAT:
        v = rng.integers(0, 1 << W, n, dtype=ut)
        near = np.array([1 << (W - 1), (1 << (W - 1)) - 1, (1 << W) - 1, (1 << W) - 2, 1 << 32 if W == 64 else 1 << 31, (1 << 32) - 1, 0, 1], dtype=ut)
        at = rng.random(n) < 0.25                                  # values near 2^63 (2^31) and 2^32: the sums wrap
        v[at] = near[rng.integers(0, near.size, int(at.sum()))]
        return v
    ft = X.FLOAT[vt]
    if op == "sum":
        return rng.integers(-(1 << 20), (1 << 20) + 1, n).astype(ft).view(ut)
    # min / max: run j holds values in [1, 2) (j % 3 == 0), in (-2, -1] (j % 3 == 1) or of both signs; one special is planted
    # in it (with the other payload of the same NaN beside it in every 4th run): +-0 and the denormals are the minimum of a
    # positive run and the maximum of a negative one, the infinities and NaNs the extreme of any run
    m, _, starts, _ = R.expected(keys)
    run = np.repeat(np.arange(m), np.diff(starts))
    mag = 1.0 + rng.random(n)
    v = np.where(run % 3 == 0, mag, np.where(run % 3 == 1, -mag, (mag - 1.5) * 100.0)).astype(ft).view(ut)
    sp = specials(vt)
    j = np.arange(m)
    at = starts[:-1] + rng.integers(0, 1 << 62, m) % np.diff(starts)
    v[at] = sp[(j // 3) % sp.size]
    two = np.flatnonzero((np.diff(starts) >= 2) & (j % 4 == 0))
    nan = np.flatnonzero(np.isnan(sp.view(ft)))
    other = starts[two] + (at[two] - starts[two] + 1) % np.diff(starts)[two]
    pick = nan[np.arange(two.size) % nan.size]
    v[at[two]] = sp[pick]
    v[other] = sp[pick ^ 1]                                       # (the payloads of one sign are neighbours in the table)
    return v


# ---- geometry: sizes x run patterns, both key widths

@pytest.mark.parametrize("pattern", R.PATTERNS + CARRY_PATTERNS)
@pytest.mark.parametrize("size", R.SIZE_NAMES)
@pytest.mark.parametrize("kb", WIDTHS)
def test_sizes_and_patterns(ctx, kb, size, pattern):
    tile, scan_tile = limits(ctx, kb)
    n = R.sizes(tile, scan_tile)[size]
    keys = make_keys(pattern, n, kb, tile, seed=E.seed_of(kb, n))
    inp = Inputs(keys)
    # the four reductions of the carry: u64 and double sums, 4- and 8-byte codes
    for vt, op in ((E.U32, "sum"), (E.F64, "sum"), (E.F32 if kb == 4 else E.I64, "min"), (E.I64 if kb == 4 else E.F32, "max")):
        reduce_case(ctx, inp, make_values(vt, op, keys, 1), vt, op, what=pattern)


def test_the_carry_patterns_are_what_they_say():
    T = 64
    for kb in WIDTHS:
        n = 33 * T + 5
        m, _, starts, _ = R.expected(make_keys("long_middle", n, kb, T))
        lens = np.diff(starts)
        assert lens.max() == 33 * T + 2 - T // 2 and starts[np.argmax(lens)] == T // 2 and (np.delete(lens, np.argmax(lens)) == 1).all()
        m, _, starts, _ = R.expected(make_keys("tile_runs_half", n, kb, T))
        assert starts[:-1].tolist() == [0] + list(range(T // 2, n, T))
        for p in CARRY_PATTERNS:
            for small in (0, 1, 2, 3, T - 1):
                assert make_keys(p, small, kb, T).size == small


# ---- types: every value type x op, exact (float sums: the exact part)

@pytest.mark.parametrize("pattern", ["geo40", "geo5000", "equal"])
@pytest.mark.parametrize("size", ["T+1", "3T-1", "big"])
@pytest.mark.parametrize("vt", X.VAL_TYPES, ids=VT_IDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_types_and_ops(ctx, kb, vt, size, pattern):
    tile, scan_tile = limits(ctx, kb)
    n = R.sizes(tile, scan_tile)[size]
    assert n <= 1 << 24                                             # (what keeps the float sums of small integers exact)
    keys = make_keys(pattern, n, kb, tile, seed=E.seed_of(kb, n, vt))
    inp = Inputs(keys)
    for op in OPS:
        vbits = make_values(vt, op, keys, 2)
        m, got = reduce_case(ctx, inp, vbits, vt, op, what=pattern)
        if vt in X.FLOAT and op != "sum" and m >= 40:               # the planted specials ARE extremes: a zero, and a NaN of the sign that wins
            ft = X.FLOAT[vt]
            sign = E.UT[vt](1 << (8 * vbytes(vt) - 1))
            assert ((got == 0) | (got == sign)).any(), (pattern, op)
            assert (np.isnan(got.view(ft)) & (((got & sign) != 0) == (op == "min"))).any(), (pattern, op)


# ---- float sums, rounded part

@pytest.mark.parametrize("pattern", ["geo5000", "equal"])
@pytest.mark.parametrize("vt", [E.F32, E.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kb", WIDTHS)
def test_float_sums_within_the_bound_of_any_order_and_reproducible(ctx, kb, vt, pattern):
    """|sum - fsum| <= L * 2^-53 * sum|x| for a run of L elements: every order of L - 1 double additions stays within it
    (L^2 < 2^53), a float32 converts exactly and the identity's additions are exact"""
    tile, scan_tile = limits(ctx, kb)
    n = R.sizes(tile, scan_tile)["big"]
    keys = make_keys(pattern, n, kb, tile, seed=7)
    ft = X.FLOAT[vt]
    vals = np.random.default_rng(E.seed_of(kb, vt, 99)).standard_normal(n).astype(ft)
    inp = Inputs(keys)
    m, got = reduce_case(ctx, inp, vals.view(E.UT[vt]), vt, "sum", what=pattern, exact=False)
    m2, again = reduce_case(ctx, inp, vals.view(E.UT[vt]), vt, "sum", what=pattern, exact=False)
    assert m2 == m and (got == again).all(), "the same call gave other bits"
    _, starts, _ = X.expected(keys, vals.view(E.UT[vt]), vt, "sum")
    wide = vals.astype(np.float64)
    sabs = np.add.reduceat(np.abs(wide), starts[:-1])
    worst = 0.0
    for j in range(m):
        lo, hi = int(starts[j]), int(starts[j + 1])
        ref = math.fsum(wide[lo:hi].tolist())
        bound = (hi - lo) * 2.0 ** -53 * float(sabs[j]) * (1 + 2.0 ** -20)   # (sabs itself is a rounded sum: far less than 2^-20 off)
        err = abs(float(got.view(np.float64)[j]) - ref)
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (pattern, j, hi - lo, err, bound)
    print("worst error / bound: %.3g over %d runs" % (worst, m))


@pytest.mark.parametrize("vt", [E.F32, E.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kb", WIDTHS)
def test_float_sums_of_infinities_and_nans(ctx, kb, vt):
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
    vals[starts[2]], vals[starts[2] + 6] = np.inf, -np.inf          # run 2: both infinities
    vals[starts[3] + 3], vals[starts[4] - 2] = -np.inf, np.inf      # run 3: both infinities, two tiles apart
    vals[starts[4] + 8] = -np.inf                                   # run 4: -inf
    vals[starts[5]], vals[starts[6]], vals[starts[7]] = np.inf, np.nan, -0.0
    vals[n - 1] = np.inf                                            # run 8: +inf in its second tile
    m, got = reduce_case(ctx, Inputs(keys), vals.view(E.UT[vt]), vt, "sum", exact=False)
    g = got.view(np.float64)
    assert m == 9 and g[0] == np.inf and np.isnan(g[1]) and np.isnan(g[2]) and np.isnan(g[3]) and g[4] == -np.inf
    assert g[5] == np.inf and np.isnan(g[6]) and g[7] == 0.0 and g[8] == np.inf


# ---- positions

@pytest.mark.parametrize("kb", WIDTHS)
def test_values_through_positions(ctx, kb):
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
        uniq, inv = np.unique(x, return_inverse=True)
        for vt, op in ((E.I64, "sum"), (E.F32, "max"), (E.U32, "min"), (E.F64, "sum")):
            for positions, what in ((np.arange(n, dtype=np.int64), "identity"), (rng.permutation(n).astype(np.int64), "permutation")):
                keys = np.sort(x)
                reduce_case(ctx, Inputs(keys, positions), make_values(vt, op, keys, 4), vt, op, what=what)
            # real positions: the value column lies where the UNSORTED keys lie; the expectation takes the gathered values
            vbits = make_values(vt, op, hs, 5)
            m, got = reduce_case(ctx, Inputs(hs, hp), vbits, vt, op, what="sorted")
            assert m == uniq.size
            if op == "sum":                                         # ... and is the group-by of the unsorted arrays
                tot = np.zeros(m, X.out_dtype(vt, op))
                np.add.at(tot, inv.reshape(-1), X.widen(vbits, vt))
                compare(got, tot, vt, op, "group-by")


# ---- capacity

@pytest.mark.parametrize("pattern", ["distinct", "geo40", "equal"])
@pytest.mark.parametrize("kb", WIDTHS)
def test_capacity(ctx, kb, pattern):
    tile, _ = limits(ctx, kb)
    n = 2 * tile + 1
    keys = make_keys(pattern, n, kb, tile, seed=5)
    m = R.expected(keys)[0]
    inp = Inputs(keys)
    for cap in sorted({0, m - 1, m, m + 1, n}):
        for vt, op in ((E.F32, "sum"), (E.I32, "min"), (E.U64, "max")):
            assert reduce_case(ctx, inp, make_values(vt, op, keys, 6), vt, op, cap=cap, what="cap")[0] == m


def test_capacity_bounds_the_extent_that_must_not_overlap(ctx):
    """d_out is taken as min(cap, n) elements: a cap beyond n claims no more memory"""
    n = 100
    keys = R.make("distinct", n, 4, 64)
    v = make_values(E.U32, "sum", keys, 1)
    din, dval, dout, dnum = Buf(4, n, a=keys), Buf(4, n, a=v), Buf(8, n), Buf(8, 1)
    ctx._ok(raw_call(ctx, din.ptr, 4, n, dval.ptr, E.U32, 0, 0, (1 << 64) - 1, dout.ptr, dnum.ptr))
    assert int(dnum.host()[0]) == n and (dout.host() == v).all()
    for b in (din, dval, dout, dnum):
        b.check("huge cap")


# ---- alignment

@pytest.mark.parametrize("vb", WIDTHS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_alignment_of_keys_values_and_output(ctx, kb, vb):
    """the keys 4, 8 and 12 bytes off the 16-byte grid, the values at ANOTHER phase of it, both widths against both"""
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
                vt, op = ((sum_vt, "sum"), (mm_vt, "min"), (mm_vt, "max"))[turn % 3]
                turn += 1
                reduce_case(ctx, Inputs(keys, key_off=koff), make_values(vt, op, keys, 8), vt, op, val_off=voff,
                            out_off=(turn % (16 // obytes(vt, op))), what="off")
    # both at the SAME phase too, for completeness, through positions
    keys = full[:tile + 3]
    reduce_case(ctx, Inputs(keys, np.arange(keys.size, dtype=np.int64)[::-1].copy(), key_off=1), make_values(sum_vt, "sum", keys, 8), sum_vt, "sum",
                val_off=kb // vb if kb >= vb else 0, what="same phase")


@pytest.mark.parametrize("vb", WIDTHS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_first_and_last_elements_of_a_page(ctx, kb, vb):
    """the first element of the keys / the values is the first or the last element of a page, and so is the last one"""
    tile, _ = limits(ctx, kb)
    PAGE = guardband.PAGE
    full = R.make("geo1.5", 2 * PAGE, kb, tile, seed=10)
    vt = E.U32 if vb == 4 else E.F64
    # (lead, off) in elements of es bytes: the first element at the page's start / in the page's last element
    first = lambda es: (0, 0)
    last = lambda es: (PAGE - 16, 16 // es - 1)
    for kplace, vplace in ((first, last), (last, first), (last, last), (first, first)):
        (klead, koff), (vlead, voff) = kplace(kb), vplace(vb)
        # n: the keys' last element is the last / the first element of a page; then the values' last element
        for n in sorted({1, (PAGE - (klead + koff * kb) % PAGE) // kb, (PAGE - (klead + koff * kb) % PAGE) // kb + 1,
                         (PAGE - (vlead + voff * vb) % PAGE) // vb, (PAGE - (vlead + voff * vb) % PAGE) // vb + 1,
                         (2 * PAGE - (klead + koff * kb) % PAGE) // kb + 1}):
            keys = full[:n]
            for op in ("sum", "max"):
                reduce_case(ctx, Inputs(keys, key_off=koff, key_lead=klead), make_values(vt, op, keys, 11), vt, op, val_off=voff, val_lead=vlead, what="page")


# ---- the runs are run_encode's

@pytest.mark.parametrize("kb", WIDTHS)
def test_run_j_is_run_j_of_run_encode(ctx, kb):
    import torch
    tile, scan_tile = limits(ctx, kb)
    for n, pattern in ((3 * tile - 1, "geo40"), ((scan_tile + 1) * tile + 5, "geo5000"), (2 * tile + 1, "alternating")):
        keys = make_keys(pattern, n, kb, tile, seed=12)
        t = torch.from_numpy(keys.view(R.IT[kb])).cuda()
        v = np.random.default_rng(n).integers(-1000, 1000, n)
        tv = torch.from_numpy(v).cuda()
        num_e, vals_e, starts, _ = ctx.run_encode(t)
        num_r, out = ctx.reduce_runs(t, tv)
        m = int(num_e.item())
        assert int(num_r.item()) == m and out.dtype == torch.int64 and out.numel() == n
        st = starts.cpu().numpy()
        assert st[m] == n and (keys[st[:m]] == vals_e.cpu().numpy().view(R.UT[kb])[:m]).all()
        assert (out.cpu().numpy()[:m] == np.add.reduceat(v, st[:m])).all()   # starts from the one call, sums from the other
        _, mx = ctx.reduce_runs(t, tv, op="max")
        assert (mx.cpu().numpy()[:m] == np.maximum.reduceat(v, st[:m])).all()


# ---- refusals through the C ABI

def test_refusals_in_order_touch_nothing(ctx):
    n = 1000
    for kb in WIDTHS:
        for vt, op in ((E.F32, 0), (E.I64, 1), (E.U32, 2), (E.F64, 0)):
            vb, ob = vbytes(vt), 8 if op == 0 else vbytes(vt)
            keys = R.make("geo1.5", n, kb, 64, seed=2)
            vbits = make_values(vt, OPS[op], keys, 3)
            din, dval, dout, dnum = Buf(kb, n, a=keys), Buf(vb, n, a=vbits), Buf(ob, n), Buf(8, 1)
            dpos = Buf(8, n, a=np.arange(n, dtype=np.uint64))
            bufs = (din, dval, dout, dpos, dnum)
            good = dict(keys=din.ptr, kb=kb, n=n, vals=dval.ptr, vt=vt, positions=dpos.ptr, op=op, cap=n, out=dout.ptr, num=dnum.ptr)
            order = ("keys", "kb", "n", "vals", "vt", "positions", "op", "cap", "out", "num")

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
            for bad in (-1, 6, 7, 100):
                refused("val_type", vt=bad)
            for bad in (-1, 3, 100):
                refused("unknown op", op=bad)
            refused("d_num_runs is required", num=0)
            refused("null keys or values", keys=0)
            refused("null keys or values", vals=0)
            refused("null d_out", out=0)
            for name, es in (("keys", kb), ("vals", vb), ("out", ob), ("positions", 8), ("num", 8)):
                for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                    refused("aligned", **{name: good[name] + d})
            refused("2^36", n=1 << 36)
            refused("2^36", n=(1 << 64) - 1)
            refused("overlap", out=din.ptr)
            refused("overlap", out=din.ptr + (n * kb - ob))
            refused("overlap", out=dval.ptr + (n * vb - ob))
            refused("overlap", out=dpos.ptr + 8 * (n - 1))
            refused("overlap", num=din.ptr)
            refused("overlap", num=dval.ptr + (n * vb - 8))
            refused("overlap", num=dpos.ptr + 8)
            refused("overlap", num=dout.ptr)
            refused("overlap", num=dout.ptr + (n * ob - 8))
            # the order: of two faults the earlier one is reported
            refused("key_bytes", kb=5, vt=9)
            refused("val_type", vt=9, op=9)
            refused("unknown op", op=9, num=0)
            refused("d_num_runs is required", num=0, keys=0)
            refused("null keys or values", vals=0, out=0)
            refused("null d_out", out=0, keys=din.ptr + 1)
            refused("aligned", positions=dpos.ptr + 4, n=1 << 36)
            refused("2^36", n=1 << 36, out=din.ptr)
            # what is no fault: null pointers with n == 0, a null d_out that only counts
            ctx._ok(raw_call(ctx, 0, kb, 0, 0, vt, 0, op, 5, 0, dnum.ptr))
            assert int(dnum.host()[0]) == 0
            ctx._ok(raw_call(ctx, din.ptr, kb, n, dval.ptr, vt, 0, op, 0, 0, dnum.ptr))
            m, _, want = X.expected(keys, vbits, vt, OPS[op], np.arange(n))
            assert int(dnum.host()[0]) == m and dout.unchanged()
            # and the call that all of these were changes of is fine
            ctx._ok(raw_call(ctx, *[good[a] for a in order]))
            assert int(dnum.host()[0]) == m
            compare(dout.host()[:m], want, vt, OPS[op], "good")
            assert dout.untouched_from(m)
            for b in bufs:
                b.check("good")


def test_an_empty_array(ctx):
    for kb in WIDTHS:
        keys = np.zeros(0, R.UT[kb])
        for cap in (0, 5):
            for vt, op in ((E.F32, "sum"), (E.I64, "min")):
                assert reduce_case(ctx, Inputs(keys), np.zeros(0, E.UT[vt]), vt, op, cap=cap, what="empty")[0] == 0
        assert reduce_case(ctx, Inputs(keys, np.zeros(0, np.int64)), np.zeros(0, np.uint32), E.U32, "max", cap=3, what="empty")[0] == 0


# ---- asynchrony and the workspace

@pytest.mark.parametrize("kb", WIDTHS)
def test_two_calls_back_to_back_with_a_run_encode_between(ctx, kb):
    """the calls share the slab: only stream order keeps them apart"""
    import torch
    tile, scan_tile = limits(ctx, kb)
    n1, n2 = (scan_tile + 1) * tile + 5, 3 * tile - 1
    k1, k2 = make_keys("tile_runs_half", n1, kb, tile, seed=21), make_keys("geo40", n2, kb, tile, seed=22)
    v1 = np.random.default_rng(1).integers(-(1 << 20), 1 << 20, n1).astype(np.float32)
    v2 = np.random.default_rng(2).integers(-(1 << 40), 1 << 40, n2)
    t1, t2 = torch.from_numpy(k1.view(R.IT[kb])).cuda(), torch.from_numpy(k2.view(R.IT[kb])).cuda()
    tv1, tv2 = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    ctx.reduce_runs(t1, tv1)                 # (the workspace has its size: no reallocation, which would synchronise)
    torch.cuda.synchronize()
    r1 = ctx.reduce_runs(t1, tv1)
    e = ctx.run_encode(t2, inverse=True)
    r2 = ctx.reduce_runs(t2, tv2, op="min", cap=10)
    r3 = ctx.reduce_runs(t1, tv1, op="max")
    torch.cuda.synchronize()
    m1, _, w1 = X.expected(k1, v1.view(np.uint32), E.F32, "sum")
    assert int(r1[0].item()) == m1 and r1[1].dtype == torch.float64 and (r1[1].cpu().numpy()[:m1] == w1).all()
    m2, ev, es_, einv = R.expected(k2)
    assert int(e[0].item()) == m2 and (e[1].cpu().numpy().view(R.UT[kb])[:m2] == ev).all() and (e[3].cpu().numpy() == einv).all()
    _, _, w2 = X.expected(k2, v2.view(np.uint64), E.I64, "min")
    assert int(r2[0].item()) == m2 and r2[1].numel() == 10 and (r2[1].cpu().numpy() == w2[:10].view(np.int64)).all()
    _, _, w3 = X.expected(k1, v1.view(np.uint32), E.F32, "max")
    assert r3[1].dtype == torch.float32 and (r3[1].cpu().numpy().view(np.uint32)[:m1] == w3).all()


def test_workspace_grows_by_no_more_than_the_records(ctx):
    """per tile and per scan piece one 8-byte lead and one 4-byte head count on top of what run_encode takes (256-byte
    aligned arrays); the slab grows in steps of 1 MiB with an eighth on top"""
    import torch
    from inplacemsdradixsort_amd import MsdContext
    kb = 4
    tile, scan_tile = limits(ctx, kb)
    n = (scan_tile + 1) * tile + 5
    t = torch.from_numpy(make_keys("geo40", n, kb, tile).view(np.int32)).cuda()
    v = torch.ones(n, dtype=torch.float32, device="cuda")
    own = MsdContext(0)
    try:
        own.run_encode(t)
        before = own.workspace_bytes
        num, out = own.reduce_runs(t, v)
        after = own.workspace_bytes
        tiles = -(-n // tile)
        pieces = -(-tiles // scan_tile)
        records = 12 * (tiles + pieces) + 4 * 256
        step = 1 << 20
        assert before > 0 and 0 <= after - before <= -(-(records + records // 8) // step) * step, (before, after, records)
        m = R.expected(t.cpu().numpy().view(np.uint32))[0]
        assert int(num.item()) == m
    finally:
        own.close()


# ---- the Python wrappers

def test_reduce_runs_wrapper_outputs_and_phase(ctx):
    import torch
    k = torch.tensor([1.0, 1.0, -0.0, 0.0, 0.0, 2.0], device="cuda")
    v = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int32, device="cuda")
    ctx.set_profiling(True)
    try:
        num, out = ctx.reduce_runs(k, v)
        assert [p[0] for p in ctx.phases()] == ["reduce_runs"]
    finally:
        ctx.set_profiling(False)
    assert num.dtype == torch.int64 and num.numel() == 1 and int(num.item()) == 4
    assert out.dtype == torch.int64 and out.numel() == 6 and out[:4].tolist() == [3, 3, 9, 6]
    num, out = ctx.reduce_runs(k, v, op="max", cap=2)
    assert int(num.item()) == 4 and out.dtype == torch.int32 and out.tolist() == [2, 3]
    num, out = ctx.reduce_runs(k, v.double(), op="sum", positions=torch.tensor([5, 4, 3, 2, 1, 0], device="cuda"))
    assert out.dtype == torch.float64 and out[:4].tolist() == [11.0, 4.0, 5.0, 1.0]
    if hasattr(torch, "uint32") and hasattr(torch, "uint64"):
        num, out = ctx.reduce_runs(k, v.view(torch.uint32))
        assert out.dtype == torch.uint64 and out.view(torch.int64)[:4].tolist() == [3, 3, 9, 6]
    f = torch.tensor([float("nan"), 1.0, -0.0, 0.0, float("-inf"), 7.0], device="cuda")
    _, mx = ctx.reduce_runs(k, f, op="max")
    _, mn = ctx.reduce_runs(k, f, op="min")
    assert math.isnan(mx[0].item()) and mn[0].item() == 1.0           # a +NaN is the maximum of its run, and no more than that
    assert mn[1].item() == 0.0 and torch.signbit(mn[1]).item() and mx[2].item() == 0.0 and not torch.signbit(mx[2]).item()
    assert mn[2].item() == float("-inf")
    assert ctx.reduce_runs_limits(4) == limits(ctx, 4) and ctx.reduce_runs_limits(8) == limits(ctx, 8)
    s, sv = k[1:4], v[2:5]                                            # slices: 4 and 8 bytes off the 16-byte grid
    num, out = ctx.reduce_runs(s, sv)
    assert int(num.item()) == 3 and out.tolist() == [3, 4, 5]


GROUP_TYPES = [E.U32, E.I32, E.F32, E.U64, E.I64, E.F64]


def _group_keys(kt, n):
    ut = E.UT[kt]
    W = 8 * np.dtype(ut).itemsize
    rng = np.random.default_rng(E.seed_of(kt, n))
    z = np.minimum(rng.zipf(1.3, n), 3000).astype(np.int64)          # Zipf-like: a few keys hold most of the elements
    if kt % 3 == 2:
        ft = np.float32 if W == 32 else np.float64
        table = np.r_[np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], ft), rng.standard_normal(3000).astype(ft)].view(ut)
    else:
        table = np.r_[np.array([0, 1, (1 << W) - 1, 1 << (W - 1), (1 << (W - 1)) - 1], dtype=ut), rng.integers(0, 1 << W, 3000, dtype=ut)]
    return table[z]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", [0, 1, 100003])
@pytest.mark.parametrize("kt", GROUP_TYPES, ids=[E.NAMES[k] for k in GROUP_TYPES])
def test_group_reduce(ctx, kt, n, op):
    import torch
    ut = E.UT[kt]
    kb = np.dtype(ut).itemsize
    bits = _group_keys(kt, n)
    vt = X.VAL_TYPES[(kt + 1 + OPS.index(op)) % 6]                    # (every value type meets some key type and op)
    if vt in X.FLOAT and op != "sum":
        vbits = np.random.default_rng(n + kt).standard_normal(n).astype(X.FLOAT[vt]).view(E.UT[vt])
    else:                                                             # wrapping integers; small integers as floats: exact in any order
        vbits = make_values(vt, "sum", bits, 13)

    def tensor(b, t):
        dt = {E.I32: torch.int32, E.F32: torch.float32, E.I64: torch.int64, E.F64: torch.float64}.get(t)
        x = torch.from_numpy(b.view(R.IT[b.itemsize])).cuda()
        if dt is None:
            name = "uint32" if t == E.U32 else "uint64"
            assert hasattr(torch, name), "this torch has no %s" % name
            dt = getattr(torch, name)
        return x.view(dt)

    tk, tv = tensor(bits, kt), tensor(vbits, vt)
    # numpy's group-by on the codes
    codes, inv = np.unique(E.np_encode(bits, kt), return_inverse=True)
    inv = inv.reshape(-1)
    want_keys = E.np_decode(codes, kt)
    if op == "sum":
        want = np.zeros(codes.size, X.out_dtype(vt, op))
        with np.errstate(over="ignore"):
            np.add.at(want, inv, X.widen(vbits, vt))
    else:
        vc = E.np_encode(vbits, vt)
        red = np.full(codes.size, 0 if op == "max" else np.iinfo(vc.dtype).max, vc.dtype)
        (np.maximum if op == "max" else np.minimum).at(red, inv, vc)
        want = E.np_decode(red, vt)
    host = D.bits
    gk, ga = ctx.group_reduce(tk, tv, op=op)
    assert gk.dtype == tk.dtype and gk.numel() == codes.size and (host(gk) == want_keys).all()
    assert ga.numel() == codes.size and ga.dtype == (tv.dtype if op != "sum" else
                                                     torch.float64 if vt in X.FLOAT else torch.int64 if vt in X.SIGNED else torch.uint64)
    compare(host(ga), want, vt, op, "group_reduce")
    assert (host(tk) == bits).all() and (host(tv) == vbits).all()     # the inputs are what they were
