"""GPU tests of the merge of two sorted arrays (msd_merge_sorted; MsdContext.merge_sorted): the stable merge of two arrays that
are ascending in the library's key order -- keys alone, with 8-byte values, with the origin (the argsort of the concatenation)
and with both, for the six key types.

The expected result is defined in tests/merge_expect.py and every result is compared exactly.  The calls go through the C ABI
on integer tensors that carry the bit patterns, with EVERY buffer -- both key arrays, both value arrays and the three outputs
-- inside a guardband.Arena whose payload is pre-filled with a known pattern: a case checks the n + m outputs, that no guard
was touched, that the inputs are what was uploaded, that the payload in front of an offset buffer is what it was and that no
output word beyond n + m changed (every output buffer is TAIL elements longer than n + m).  The shapes are the smallest at
which a kernel can go wrong, taken from msd_merge_sorted_limits (T = the tile).  Unsorted inputs: test_gpu_untrusted_order.py.
The Python wrapper has tests of its own at the end."""
import ctypes as C

import numpy as np
import pytest

import gpu_support as D
import merge_expect as M
import search_expect as S
import sort_rows_expect as E
from guardband import Buf
from gpu_support import TAIL
from sort_rows_expect import UKT, WIDTHS, special_bits, top, uniform

pytestmark = pytest.mark.gpu

VARIANTS = ((False, False), (True, False), (False, True), (True, True))   # (values, origin)


def limits(ctx, kb):
    tile = C.c_uint64()
    assert ctx._L.msd_merge_sorted_limits(kb, C.byref(tile)) == 0
    return int(tile.value)


def raw_call(ctx, a, n, b, m, kt, va, vb, out, ov, oo):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_merge_sorted(ctx._h, vp(a), n, vp(b), m, kt, vp(va), vp(vb), vp(out), vp(ov), vp(oo))


def values_for(count, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, count, dtype=np.uint64)


class Case:
    """A and B (unsigned bit patterns of key type kt, ascending by code) and their values on the device, shared by the calls
    of the case.  offs: the element offsets of d_a, d_b, d_vals_a, d_vals_b, d_out, d_out_vals, d_out_origin."""

    def __init__(self, a, b, kt, offs=(0,) * 7, what=""):
        self.a, self.b, self.kt = a, b, kt
        self.kb, self.n, self.m = a.itemsize, a.size, b.size
        self.total = self.n + self.m
        self.va, self.vb = values_for(self.n, 11), values_for(self.m, 12)
        self.da, self.db = Buf(self.kb, self.n, offs[0], a=a), Buf(self.kb, self.m, offs[1], a=b)
        self.dva, self.dvb = Buf(8, self.n, offs[2], a=self.va), Buf(8, self.m, offs[3], a=self.vb)
        self.dout = Buf(self.kb, self.total + TAIL, offs[4])
        self.dov, self.doo = Buf(8, self.total + TAIL, offs[5]), Buf(8, self.total + TAIL, offs[6])
        self.want, self.origin = M.expected(a, b, kt)
        self.want_vals = np.concatenate([self.va, self.vb])[self.origin.astype(np.int64)]
        self.what = (what, E.NAMES[kt], self.n, self.m, offs)

    def bufs(self):
        return (("d_a", self.da), ("d_b", self.db), ("d_vals_a", self.dva), ("d_vals_b", self.dvb), ("d_out", self.dout), ("d_out_vals", self.dov),
                ("d_out_origin", self.doo))

    def launch(self, ctx, vals, origin):
        return raw_call(ctx, self.da.ptr, self.n, self.db.ptr, self.m, self.kt, vals and self.dva.ptr, vals and self.dvb.ptr, self.dout.ptr,
                        vals and self.dov.ptr, origin and self.doo.ptr)

    def verify(self, vals, origin, what=""):
        what = (self.what, "values" if vals else "", "origin" if origin else "", what)
        got = self.dout.written(self.total)
        bad = got != self.want
        assert not bad.any(), (what, "keys differ", int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), self.want[bad][:4].tolist())
        if origin:
            got = self.doo.written(self.total)
            bad = got != self.origin
            assert not bad.any(), (what, "origins differ", int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), self.origin[bad][:4].tolist())
        else:
            assert self.doo.unchanged(), (what, "d_out_origin was not given and changed")
        if vals:
            got = self.dov.written(self.total)
            bad = got != self.want_vals
            assert not bad.any(), (what, "values differ", int(bad.sum()), int(np.argmax(bad)))
        else:
            assert self.dov.unchanged(), (what, "d_out_vals was not given and changed")
        for name, b in self.bufs()[:4]:
            assert b.unchanged(), (what, "%s changed" % name)
        for name, b in self.bufs():
            b.check("%s of %s" % (name, what))

    def run(self, ctx, vals, origin):
        """one call, everything checked"""
        for b in (self.dout, self.dov, self.doo):
            b.reset()
        ctx._ok(self.launch(ctx, vals, origin))
        self.verify(vals, origin)

    def run_all(self, ctx):
        for vals, origin in VARIANTS:
            self.run(ctx, vals, origin)


# ---- inputs, as codes of an unsigned type (code == bits)

KINDS = ["distinct", "five", "all_equal", "a_below", "a_above", "a_equal_in_distinct_b"]


def inputs(kind, n, m, kb, seed):
    """A and B, both ascending"""
    rng = np.random.default_rng(E.seed_of(n, m, kb, seed, 8))
    ut = E.UW[kb]
    half = top(kb) >> 1
    five = np.array([0, 1 << 9, 77777, half, top(kb)], ut)
    if kind == "distinct":                                          # distinct keys, interleaved at random
        pool = np.unique(uniform(rng, n + m + 64, kb))[:n + m]
        assert pool.size == n + m
        pool = rng.permutation(pool)
        a, b = pool[:n], pool[n:]
    elif kind == "five":                                            # ties lie across every tile edge
        a, b = five[rng.integers(0, 5, n)], five[rng.integers(0, 5, m)]
    elif kind == "all_equal":                                       # stability shows in origin only; tiles of A only, then of B only
        a, b = np.full(n, 77777, ut), np.full(m, 77777, ut)
    elif kind == "a_below":
        a, b = uniform(rng, n, kb, 0, half), uniform(rng, m, kb, half + 1)
    elif kind == "a_above":
        a, b = uniform(rng, n, kb, half + 1), uniform(rng, m, kb, 0, half)
    else:                                                           # "a_equal_in_distinct_b"
        b = np.sort(np.unique(uniform(rng, m + 64, kb))[:m])
        assert b.size == m
        a = np.full(n, b[m // 2] if m else 77777, ut)
    return np.sort(a), np.sort(b)


def test_the_inputs_are_what_they_say():
    T = 64
    for kb in WIDTHS:
        for kind in KINDS:
            a, b = inputs(kind, 2 * T + 3, 2 * T + 3, kb, 3)
            assert (a[1:] >= a[:-1]).all() and (b[1:] >= b[:-1]).all() and a.size == b.size == 2 * T + 3
            merged, origin = M.tiles(a, b, T)                       # the model of the kernels gives the expectation on them
            want, want_origin = M.expected(a, b, UKT[kb])
            assert (merged == want).all() and (origin == want_origin).all()
        a, b = inputs("distinct", 2 * T + 3, 2 * T + 3, kb, 3)
        assert np.unique(np.r_[a, b]).size == 4 * T + 6
        a, b = inputs("all_equal", 2 * T + 3, 2 * T + 3, kb, 3)
        sa, sb, _ = S.splits(a, b, T, True)                         # tiles of A only, then tiles of B only
        assert sa[1] == T and sb[1] == 0 and sa[-2] == a.size and sb[-1] - sb[-2] > 0
        a, b = inputs("five", 5 * T, 5 * T, kb, 3)
        sa, sb, _ = S.splits(a, b, T, True)                         # ties across the tile edges
        assert any(0 < sa[i] < a.size and 0 < sb[i] < b.size and a[sa[i] - 1] == b[sb[i]] for i in range(1, len(sa) - 1))
        a, b = inputs("a_equal_in_distinct_b", T, 2 * T, kb, 3)
        assert (a == b[T]).all() and M.expected(a, b, UKT[kb])[1][T:2 * T + 1].tolist() == list(range(T)) + [2 * T]


# ---- the grid of sizes

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_sizes_around_the_tile(ctx, kb, kind):
    """n and m around the tile, every cell plain, with values, with origin and with both"""
    T = limits(ctx, kb)
    edge = (0, 1, 2, T - 1, T, T + 1, 2 * T + 3)
    for n, m in [(n, m) for n in edge for m in edge] + [(5 * T + 17, 3), (3, 5 * T + 17)]:
        a, b = inputs(kind, n, m, kb, 3)
        Case(a, b, UKT[kb], what=kind).run_all(ctx)


@pytest.mark.parametrize("kb", WIDTHS)
def test_a_larger_case(ctx, kb):
    """the split kernel has more than one workgroup"""
    n, m = (1 << 20) + 5, (1 << 19) + 3
    T = limits(ctx, kb)
    assert (n + m) // T + 1 > 256
    rng = np.random.default_rng(kb)
    a = np.sort(uniform(rng, n, kb, 0, 1 << 20))                    # (most keys have an equal one on the other side)
    b = np.sort(uniform(rng, m, kb, 0, 1 << 20))
    Case(a, b, UKT[kb], what="larger").run(ctx, True, True)


# ---- all six key types

@pytest.mark.parametrize("kt", M.KEY_TYPES, ids=[E.NAMES[k] for k in M.KEY_TYPES])
def test_every_key_type_with_special_values(ctx, kt):
    ut = E.UT[kt]
    kb = np.dtype(ut).itemsize
    T = limits(ctx, kb)
    rng = np.random.default_rng(kt)
    sp = special_bits(kt)

    def draw(count, first):
        x = uniform(rng, count, kb)
        at = rng.random(count) < 0.5
        x[at] = sp[rng.integers(0, sp.size, int(at.sum()))]
        x[:first.size] = first                                      # every special is on one side at least, most on both
        return S.sort_by_code(x, kt)

    for n, m in ((T + 1, T - 1), (2 * T + 3, T + 1)):
        case = Case(draw(n, sp[0::2]), draw(m, sp[1::2]), kt, what="specials")
        assert set(sp.tolist()) <= set(case.want.tolist())
        case.run_all(ctx)
    if kt % 3 == 2:                                                 # totalOrder: -0.0 from B lands in front of +0.0 from A, the NaNs lie outside
        sign = ut(1 << (8 * kb - 1))
        nan = sp[4]
        a = np.array([nan | sign, 0, 0, nan], ut)
        b = np.array([sign, sign, 0, nan, nan | ut(1)], ut)
        case = Case(a, b, kt, what="zeros and NaNs")
        case.run(ctx, True, True)
        assert case.dout.written(9).tolist() == [nan | sign, sign, sign, 0, 0, 0, nan, nan, nan | ut(1)]
        assert case.doo.written(9).tolist() == [0, 4, 5, 1, 2, 6, 3, 7, 8]


# ---- alignment

def test_four_byte_buffers_off_the_16_byte_grid(ctx):
    """d_a, d_b and d_out 4, 8 and 12 bytes behind a 16-byte boundary, each at another phase; values and origin 8 bytes off"""
    T = limits(ctx, 4)
    for turn, (oa, ob, oo) in enumerate([(1, 2, 3), (2, 3, 1), (3, 1, 2), (0, 1, 2), (3, 0, 1), (2, 1, 0)]):
        for n, m in ((2 * T + 3, T + 1), (T - 1, 3), (3, 2), (1, T + 1 - oo)):
            a, b = inputs("distinct" if turn % 2 else "five", n, m, 4, turn)
            Case(a, b, E.U32, offs=(oa, ob, 1, 1, oo, 1, 1), what="off").run_all(ctx)


def test_eight_byte_buffers_off_the_16_byte_grid(ctx):
    """8-byte keys have one phase off the grid: every buffer 8 bytes off, and every one of the key buffers alone on the grid"""
    T = limits(ctx, 8)
    for turn, (oa, ob, oo) in enumerate([(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0)]):
        for n, m in ((2 * T + 3, T + 1), (T - 1, 3), (1, 1), (2, T - oo)):
            a, b = inputs("distinct" if turn % 2 else "five", n, m, 8, turn)
            Case(a, b, E.U64, offs=(oa, ob, 1, 1, oo, 1, 1), what="off").run_all(ctx)


# ---- values and origin

@pytest.mark.parametrize("kb", WIDTHS)
def test_values_follow_their_keys_and_origin_is_a_permutation(ctx, kb):
    T = limits(ctx, kb)
    n, m = 3 * T + 5, 2 * T - 7
    a, b = inputs("five", n, m, kb, 5)
    case = Case(a, b, UKT[kb], what="values")
    case.run(ctx, True, True)
    origin = case.doo.written(n + m).astype(np.int64)
    assert (np.sort(origin) == np.arange(n + m)).all()             # a permutation of [0, n + m)
    assert (case.dov.written(n + m) == np.concatenate([case.va, case.vb])[origin]).all()
    assert (case.dout.written(n + m) == np.concatenate([a, b])[origin]).all()
    eq = case.want[1:] == case.want[:-1]
    assert (origin[1:][eq] > origin[:-1][eq]).all()                 # stable: among equal keys the concatenation's order, A before B


# ---- degenerate sizes

def test_empty_sides_and_null_pointers(ctx):
    for kb in WIDTHS:
        x = np.sort(uniform(np.random.default_rng(1), 1000, kb))
        Case(x[:0], x, UKT[kb], what="n = 0").run_all(ctx)          # copies the other side
        Case(x, x[:0], UKT[kb], what="m = 0").run_all(ctx)
        none = Case(x[:0], x[:0], UKT[kb], what="n + m = 0")
        none.run_all(ctx)
        # null pointers where nothing is read or written
        case = Case(x, x[:0], UKT[kb], what="null d_b")
        ctx._ok(raw_call(ctx, case.da.ptr, 1000, 0, 0, case.kt, case.dva.ptr, 0, case.dout.ptr, case.dov.ptr, case.doo.ptr))
        case.verify(True, True, "null d_b and d_vals_b")
        case = Case(x[:0], x, UKT[kb], what="null d_a")
        ctx._ok(raw_call(ctx, 0, 0, case.db.ptr, 1000, case.kt, 0, case.dvb.ptr, case.dout.ptr, case.dov.ptr, case.doo.ptr))
        case.verify(True, True, "null d_a and d_vals_a")
        ctx._ok(raw_call(ctx, 0, 0, 0, 0, UKT[kb], 0, 0, 0, 0, 0))  # nothing at all
        ctx._ok(raw_call(ctx, 0, 0, 0, 0, UKT[kb], 0, 0, none.dout.ptr, none.dov.ptr, none.doo.ptr))
        none.verify(False, False, "nothing to write")


# ---- refusals through the C ABI

def test_refusals_in_order_touch_nothing(ctx):
    n, m = 1000, 300
    for kb in WIDTHS:
        for kt in (UKT[kb], UKT[kb] + 2):
            a, b = inputs("distinct", n, m, kb, 4)
            case = Case(S.sort_by_code(a, kt), S.sort_by_code(b, kt), kt, what="refusals")
            bufs = [b for _, b in case.bufs()]
            da, db, dva, dvb, dout, dov, doo = bufs
            good = dict(a=da.ptr, n=n, b=db.ptr, m=m, kt=kt, va=dva.ptr, vb=dvb.ptr, out=dout.ptr, ov=dov.ptr, oo=doo.ptr)
            order = ("a", "n", "b", "m", "kt", "va", "vb", "out", "ov", "oo")

            def refused(message, **change):
                k = dict(good, **change)
                rc = raw_call(ctx, *[k[x] for x in order])
                err = ctx._L.msd_last_error(ctx._h).decode()
                assert rc == -1 and message in err, (change, rc, err)
                for buf in bufs:
                    assert buf.unchanged(), change
                    buf.check(str(change))

            # every refusal on its own, in the header's order
            for bad in (-1, 6, 7, 100):
                refused("key_type", kt=bad)
            refused("null d_out", out=0)
            refused("null d_a", a=0)
            refused("null d_b", b=0)
            refused("d_out_vals without", va=0)
            refused("d_out_vals without", vb=0)
            refused("d_out_vals without", va=0, vb=0)
            refused("without d_out_vals", ov=0)
            refused("without d_out_vals", ov=0, va=0)
            refused("without d_out_vals", ov=0, vb=0)
            for name, es in (("a", kb), ("b", kb), ("out", kb), ("va", 8), ("vb", 8), ("ov", 8), ("oo", 8)):
                for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                    refused("aligned", **{name: good[name] + d})
            for big in (1 << 36, (1 << 64) - 1):
                refused("2^36", n=big)
                refused("2^36", m=big)
            last = n + m - 1
            refused("must not overlap", out=da.ptr)
            refused("must not overlap", out=da.ptr + (n - 1) * kb)
            refused("must not overlap", a=dout.ptr + last * kb)
            refused("must not overlap", out=db.ptr)
            refused("must not overlap", b=dout.ptr + last * kb)
            refused("must not overlap", out=dva.ptr + 8 * (n - 1))
            refused("must not overlap", out=dvb.ptr)
            refused("must not overlap", ov=dva.ptr)
            refused("must not overlap", ov=dvb.ptr + 8 * (m - 1))
            refused("must not overlap", ov=da.ptr)
            refused("must not overlap", oo=dvb.ptr)
            refused("must not overlap", oo=db.ptr)
            refused("must not overlap", oo=da.ptr, va=0, vb=0, ov=0)
            refused("must not overlap", ov=dout.ptr + 8)            # the outputs among each other
            refused("must not overlap", oo=dout.ptr)
            refused("must not overlap", oo=dov.ptr + 8 * last)
            refused("must not overlap", ov=doo.ptr + 8 * last)
            # the order: of two faults the earlier one is reported
            refused("key_type", kt=9, out=0)
            refused("null d_out", out=0, a=0)
            refused("null d_a", a=0, b=0)
            refused("null d_b", b=0, va=0)
            refused("d_out_vals without", vb=0, a=da.ptr + 1)
            refused("without d_out_vals", ov=0, oo=doo.ptr + 4)
            refused("aligned", oo=doo.ptr + 4, n=1 << 36)
            refused("2^36", m=1 << 36, out=da.ptr)
            # and the call that all of these were changes of is fine
            ctx._ok(raw_call(ctx, *[good[x] for x in order]))
            case.verify(True, True, "good")


# ---- asynchrony, the workspace and the phase

@pytest.mark.parametrize("kb", WIDTHS)
def test_two_calls_back_to_back_with_a_search_between(ctx, kb):
    """the calls share the slab: only stream order keeps them apart"""
    import torch
    T = limits(ctx, kb)
    a1, b1 = inputs("five", 7 * T + 5, 5 * T + 1, kb, 21)
    a2, b2 = inputs("distinct", 2 * T + 3, 9 * T - 1, kb, 22)
    c1, c2 = Case(a1, b1, UKT[kb], what="first"), Case(a2, b2, UKT[kb], what="second")
    found = Buf(8, b1.size)
    c1.run(ctx, True, True)                                         # (the workspace has its size: no reallocation, which would synchronise)
    for b in (c1.dout, c1.dov, c1.doo):
        b.reset()
    torch.cuda.synchronize()
    ctx.set_option("search_mode", 2)
    try:
        ctx._ok(c1.launch(ctx, True, True))
        ctx._ok(ctx._L.msd_search_sorted(ctx._h, C.c_void_p(c1.da.ptr), UKT[kb], a1.size, C.c_void_p(c1.db.ptr), b1.size, 1, 1, None, C.c_void_p(found.ptr)))
        ctx._ok(c2.launch(ctx, False, True))
    finally:
        ctx.set_option("search_mode", D.DEFAULTS["search_mode"])
    torch.cuda.synchronize()
    c1.verify(True, True, "in front of the search")
    c2.verify(False, True, "behind the search")
    assert (found.host() == S.expected(a1, b1, UKT[kb], True)).all()
    found.check("d_out of the search")


def test_workspace_grows_by_the_splits(ctx):
    """one 8-byte split per tile plus one (a 256-byte aligned array, 4 KiB of slack); the slab grows in steps of 1 MiB with
    an eighth on top, and a second call of the same size finds it there"""
    from inplacemsdradixsort_amd import MsdContext
    kb = 4
    T = limits(ctx, kb)
    a, b = inputs("distinct", 40 * T + 5, 9 * T, kb, 23)
    case = Case(a, b, UKT[kb], what="workspace")
    own = MsdContext(0)
    try:
        before = own.workspace_bytes
        own._ok(case.launch(own, True, True))
        after = own.workspace_bytes
        case.verify(True, True, "first")
        need = 8 * (-(-(a.size + b.size) // T) + 1) + 4096
        step = 1 << 20
        assert 0 < after - before <= -(-(need + need // 8) // step) * step, (before, after, need)
        own._ok(case.launch(own, False, False))
        assert own.workspace_bytes == after
    finally:
        own.close()


def test_the_phase_is_named(ctx):
    a, b = inputs("distinct", 1000, 100, 4, 9)
    case = Case(a, b, E.U32, what="phase")
    ctx.set_profiling(True)
    try:
        case.run(ctx, True, False)
        assert [p[0] for p in ctx.phases()] == ["merge_sorted"]
    finally:
        ctx.set_profiling(False)


# ---- the Python wrapper

def test_merge_sorted_wrapper_for_every_dtype(ctx):
    import torch
    dts = D.dtypes()
    assert len(dts) == 6
    for dt, kt in dts:
        kb = np.dtype(E.UT[kt]).itemsize
        T = limits(ctx, kb)
        assert ctx.merge_sorted_limits(kb) == T
        rng = np.random.default_rng(kt)
        sp = special_bits(kt)
        n, m = T + 7, 2 * T - 3
        a_bits, b_bits = [S.sort_by_code(np.r_[sp, uniform(rng, c - sp.size, kb, 0, 1 << 12), ], kt) for c in (n, m)]
        want, want_origin = M.expected(a_bits, b_bits, kt)
        a, b = D.to_gpu(a_bits, dt), D.to_gpu(b_bits, dt)
        va, vb = torch.arange(n, dtype=torch.float64, device="cuda"), -torch.arange(m, dtype=torch.float64, device="cuda")
        before = [x.view(D.int_dtype(x.element_size())).clone() for x in (a, b, va, vb)]
        merged = ctx.merge_sorted(a, b)
        assert merged.dtype == dt and merged.shape == (n + m,) and (D.bits(merged) == want).all()
        merged, origin = ctx.merge_sorted(a, b, origin=True)
        assert origin.dtype == torch.int64 and (D.bits(merged) == want).all() and (origin.cpu().numpy() == want_origin.astype(np.int64)).all()
        merged, vals = ctx.merge_sorted(a, b, values_a=va, values_b=vb)
        assert vals.dtype == torch.float64 and torch.equal(vals, torch.cat([va, vb])[origin]) and (D.bits(merged) == want).all()
        out = torch.empty(n + m, dtype=dt, device="cuda")
        ov, oo = torch.empty(n + m, dtype=torch.float64, device="cuda"), torch.empty(n + m, dtype=torch.int64, device="cuda")
        r = ctx.merge_sorted(a, b, values_a=va, values_b=vb, out=out, out_values=ov, out_origin=oo)
        assert r[0] is out and r[1] is ov and r[2] is oo and len(r) == 3
        assert (D.bits(out) == want).all() and torch.equal(ov, vals) and torch.equal(oo, origin)
        for x, y in zip((a, b, va, vb), before):                    # the inputs are what they were
            assert torch.equal(x.view(D.int_dtype(x.element_size())), y)
        # empty sides
        assert (D.bits(ctx.merge_sorted(a[:0], b)) == b_bits).all() and (D.bits(ctx.merge_sorted(a, b[:0])) == a_bits).all()
        e, eo = ctx.merge_sorted(a[:0], b[:0], origin=True)
        assert e.shape == (0,) and eo.shape == (0,) and e.dtype == dt


def test_merge_sorted_is_the_sort_of_the_concatenation_where_the_orders_agree(ctx):
    import torch
    g = torch.Generator(device="cpu").manual_seed(5)
    for dt in (torch.int32, torch.int64, torch.float32, torch.float64):
        a = (torch.randn(5000, generator=g) * 50).to(dt).cuda()
        b = (torch.randn(3000, generator=g) * 50).to(dt).cuda()
        if dt.is_floating_point:
            a[a == 0] = 1.0                                         # (no zeros of two signs, no NaNs: the two orders agree)
            b[b == 0] = 1.0
        ctx.sort_typed(a)
        ctx.sort_typed(b)
        merged, origin = ctx.merge_sorted(a, b, origin=True)
        cat = torch.cat([a, b])
        want, want_origin = torch.sort(cat, stable=True)
        assert torch.equal(merged, want) and torch.equal(origin, want_origin)


def test_the_merge_feeds_run_encode_and_reduce_runs(ctx):
    """two sorted batches united, then a group-by over value columns that stay where they are"""
    import torch
    rng = np.random.default_rng(6)
    for dt, kdt in ((torch.int32, np.int32), (torch.int64, np.int64)):
        n, m = 30011, 12007
        ka, kb_ = np.sort(rng.integers(-300, 300, n).astype(kdt)), np.sort(rng.integers(-350, 250, m).astype(kdt))
        cat = np.concatenate([ka, kb_])
        col_i = rng.integers(-(1 << 40), 1 << 40, n + m)
        col_f = rng.standard_normal(n + m).astype(np.float32)
        merged, origin = ctx.merge_sorted(torch.from_numpy(ka).cuda(), torch.from_numpy(kb_).cuda(), origin=True)
        num, distinct, _, _ = ctx.run_encode(merged, starts=False)
        uniq, inv = np.unique(cat, return_inverse=True)
        g = int(num.item())
        assert g == uniq.size and (distinct[:g].cpu().numpy() == uniq).all()
        num_i, sums = ctx.reduce_runs(merged, torch.from_numpy(col_i).cuda(), op="sum", positions=origin)
        want = np.zeros(uniq.size, np.int64)
        np.add.at(want, inv, col_i)
        assert int(num_i.item()) == g and (sums[:g].cpu().numpy() == want).all()
        num_f, mins = ctx.reduce_runs(merged, torch.from_numpy(col_f).cuda(), op="min", positions=origin)
        wmin = np.full(uniq.size, np.inf, np.float32)
        np.minimum.at(wmin, inv, col_f)
        assert int(num_f.item()) == g and (mins[:g].cpu().numpy() == wmin).all()
