"""GPU tests of the set operations on two sorted arrays (msd_set_sorted; MsdContext.set_sorted, intersect1d, union1d, setdiff1d,
setxor1d): intersection, union, difference and symmetric difference of two arrays that are ascending in the library's key
order, as sets, with and without the origin, for the six key types.

The expected result is defined in tests/set_expect.py and every result is compared exactly.  The calls go through the C ABI
on integer tensors that carry the bit patterns, with EVERY buffer -- both inputs, d_out, d_out_origin and, in an arena of its
own, d_num_out -- inside a guardband.Arena whose payload is pre-filled with a known pattern: a case checks *d_num_out, the
min(count, cap) results, that no guard was touched, that the inputs are what was uploaded, that the payload in front of an
offset buffer is what it was, that no output word beyond min(count, cap) changed and that an output that was not given did
not change.  The shapes are the smallest at which a kernel can go wrong, taken from msd_set_sorted_limits (T = the tile).
The buffers are guardband.Buf, the special values those of sort_rows_expect.py and the six kinds of input of the merge come
from test_gpu_merge_sorted.py.  Unsorted inputs: test_gpu_untrusted_order.py.  The Python wrappers have tests of their own at the end."""
import ctypes as C

import numpy as np
import pytest

import gpu_support as D
import search_expect as S
import set_expect as X
import sort_rows_expect as E
from gpu_support import TAIL
from guardband import Buf
from sort_rows_expect import UKT, WIDTHS, special_bits, top, uniform
from test_gpu_merge_sorted import KINDS as MERGE_KINDS
from test_gpu_merge_sorted import inputs as merge_inputs

gpu = pytest.mark.gpu                                                 # (every test but the one of the inputs)

KINDS = MERGE_KINDS + ["half_shared"]
VARIANTS = [(op, origin) for op in X.OPS for origin in (False, True)]


def limits(ctx, kb):
    tile, scan = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_set_sorted_limits(kb, C.byref(tile), C.byref(scan)) == 0
    return int(tile.value), int(scan.value)


def raw_call(ctx, op, a, n, b, m, kt, cap, out, oo, num):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_set_sorted(ctx._h, op, vp(a), n, vp(b), m, kt, cap, vp(out), vp(oo), vp(num))


def distinct_pool(rng, count, kb):
    """`count` distinct values, ascending"""
    step = max(1, min(top(kb) // (count + 1), 1 << 20))
    return np.cumsum(rng.integers(1, step, count, dtype=np.uint64, endpoint=True)).astype(E.UW[kb])


def inputs(kind, n, m, kb, seed):
    """A and B, both ascending"""
    if kind != "half_shared":
        return merge_inputs(kind, n, m, kb, seed)
    rng = np.random.default_rng(E.seed_of(n, m, kb, seed, 9))
    shared = min(n, m) // 2                                         # A and B: random subsets of a pool of distinct values that share about half
    pool = rng.permutation(distinct_pool(rng, n + m - shared, kb))
    return np.sort(pool[:n]), np.sort(pool[n - shared:])


class Case:
    """A and B (unsigned bit patterns of key type kt, ascending by code) on the device, shared by the calls of the case.
    offs: the element offsets of d_a, d_b, d_out, d_out_origin.  The outputs hold n + m + TAIL elements."""

    def __init__(self, a, b, kt, offs=(0,) * 4, what=""):
        self.a, self.b, self.kt = a, b, kt
        self.kb, self.n, self.m = a.itemsize, a.size, b.size
        self.da, self.db = Buf(self.kb, self.n, offs[0], a=a), Buf(self.kb, self.m, offs[1], a=b)
        self.dout, self.doo = Buf(self.kb, self.n + self.m + TAIL, offs[2]), Buf(8, self.n + self.m + TAIL, offs[3])
        self.dnum = Buf(8, 1)
        self._want = {}
        self.what = (what, E.NAMES[kt], self.n, self.m, offs)

    def bufs(self):
        return (("d_a", self.da), ("d_b", self.db), ("d_out", self.dout), ("d_out_origin", self.doo), ("d_num_out", self.dnum))

    def want(self, op):
        """(keys, origin) of the operation, computed once"""
        if op not in self._want:
            self._want[op] = X.expected(self.a, self.b, self.kt, op)
        return self._want[op]

    def count(self, op):
        return self.want(op)[0].size

    def bound(self, op):
        return X.bound(op, self.n, self.m)

    def launch(self, ctx, op, origin=True, out=True, cap=None):
        return raw_call(ctx, op, self.da.ptr, self.n, self.db.ptr, self.m, self.kt, self.bound(op) if cap is None else cap, out and self.dout.ptr,
                        origin and self.doo.ptr, self.dnum.ptr)

    def verify(self, op, origin=True, out=True, cap=None, what=""):
        what = (self.what, X.OP_NAMES[op], "origin" if origin else "", "out" if out else "", cap, what)
        want, want_origin = self.want(op)
        stored = min(want.size, self.bound(op) if cap is None else cap)
        num = self.dnum.host()
        assert int(num[0]) == want.size, (what, "*d_num_out", int(num[0]), want.size)
        if out:
            got = self.dout.written(stored)
            bad = got != want[:stored]
            assert not bad.any(), (what, "keys differ", int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), want[:stored][bad][:4].tolist())
        else:
            assert self.dout.unchanged(), (what, "d_out was not given and changed")
        if origin:
            got = self.doo.written(stored)
            bad = got != want_origin[:stored]
            assert not bad.any(), (what, "origins differ", int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), want_origin[:stored][bad][:4].tolist())
        else:
            assert self.doo.unchanged(), (what, "d_out_origin was not given and changed")
        for name, b in self.bufs()[:2]:
            assert b.unchanged(), (what, "%s changed" % name)
        for name, b in self.bufs():
            b.check("%s of %s" % (name, what))

    def reset(self):
        for b in (self.dout, self.doo, self.dnum):
            b.reset()

    def run(self, ctx, op, origin=True, out=True, cap=None):
        """one call, everything checked"""
        self.reset()
        ctx._ok(self.launch(ctx, op, origin, out, cap))
        self.verify(op, origin, out, cap)

    def run_all(self, ctx):
        for op, origin in VARIANTS:
            self.run(ctx, op, origin)


# ---- the inputs, without a GPU

def test_the_inputs_are_what_they_say():
    T = 64
    for kb in WIDTHS:
        for kind in KINDS:
            a, b = inputs(kind, 2 * T + 3, 2 * T + 3, kb, 3)
            assert (a[1:] >= a[:-1]).all() and (b[1:] >= b[:-1]).all() and a.size == b.size == 2 * T + 3
            for op in X.OPS:                                        # the model of the kernels gives the expectation on them
                keys, origin = X.tiles(a, b, T, op)
                want, want_origin = X.expected(a, b, UKT[kb], op)
                assert keys.tolist() == want.tolist() and origin.tolist() == want_origin.tolist(), (kind, kb, op)
        a, b = inputs("five", 5 * T, 5 * T, kb, 3)
        sa, sb, _ = S.splits(a, b, T, True)                         # a match across a tile edge: the A element closes a tile, its B opens the next
        assert any(0 < sa[i] < a.size and sb[i] < b.size and a[sa[i] - 1] == b[sb[i]] for i in range(1, len(sa) - 1))
        a, b = inputs("all_equal", 2 * T + 3, 2 * T + 3, kb, 3)
        sa, sb, _ = S.splits(a, b, T, True)                         # tiles whose A run began in an earlier tile
        assert sa[1] == T and sa[2] == 2 * T and a[sa[1] - 1] == a[sa[1]]
        assert [X.expected(a, b, UKT[kb], op)[0].size for op in X.OPS] == [1, 1, 0, 0]
        a, b = inputs("half_shared", 2 * T + 3, 2 * T + 3, kb, 3)
        sizes = [X.expected(a, b, UKT[kb], op)[0].size for op in X.OPS]
        assert sizes == [T + 1, 3 * T + 5, T + 2, 2 * T + 4]        # a non-empty result for every op: half of each side is shared
        assert np.unique(a).size == a.size and np.unique(b).size == b.size


# ---- the grid of sizes

@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_sizes_around_the_tile(ctx, kb, kind):
    """n and m around the tile, every cell for the four operations, each with and without origin"""
    T, _ = limits(ctx, kb)
    edge = (0, 1, 2, T - 1, T, T + 1, 2 * T + 3)
    for n, m in [(n, m) for n in edge for m in edge] + [(5 * T + 17, 3), (3, 5 * T + 17)]:
        a, b = inputs(kind, n, m, kb, 3)
        Case(a, b, UKT[kb], what=kind).run_all(ctx)


@gpu
@pytest.mark.parametrize("kb", WIDTHS)
def test_the_scan_with_more_than_one_piece(ctx, kb):
    """more tile counts than one workgroup of the scan takes: the bases come from two pieces"""
    T, scan = limits(ctx, kb)
    total = (scan + 3) * T + 5
    n = total // 2 + 7
    a, b = inputs("half_shared", n, total - n, kb, 5)
    assert -(-total // T) > scan
    Case(a, b, UKT[kb], what="two pieces").run(ctx, X.UNION, True)


# ---- all six key types

@gpu
@pytest.mark.parametrize("kt", X.KEY_TYPES, ids=[E.NAMES[k] for k in X.KEY_TYPES])
def test_every_key_type_with_special_values(ctx, kt):
    ut = E.UT[kt]
    kb = np.dtype(ut).itemsize
    T, _ = limits(ctx, kb)
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
        assert set(sp.tolist()) <= set(case.want(X.UNION)[0].tolist())
        case.run_all(ctx)
    if kt % 3 == 2:                                                 # equality of bits: the zeros stay apart, equal NaNs are one value
        sign = ut(1 << (8 * kb - 1))
        nan = sp[4]
        a = np.array([nan | sign, 0, 0, nan, nan | ut(2)], ut)
        b = np.array([sign, sign, nan, nan, nan | ut(1)], ut)
        case = Case(a, b, kt, what="zeros and NaNs")
        case.run_all(ctx)
        assert case.want(X.INTERSECTION)[0].tolist() == [nan] and case.want(X.INTERSECTION)[1].tolist() == [3]
        assert case.want(X.UNION)[0].tolist() == [nan | sign, sign, 0, nan, nan | ut(1), nan | ut(2)]
        assert case.want(X.UNION)[1].tolist() == [0, 5, 1, 3, 9, 4]


# ---- alignment

def _alignment(ctx, kb, phases, sizes):
    for turn, (oa, ob, oo) in enumerate(phases):
        for n, m in sizes(oo):
            a, b = inputs("half_shared" if turn % 2 else "five", n, m, kb, turn)
            case = Case(a, b, UKT[kb], offs=(oa, ob, oo, 1), what="off")
            case.run_all(ctx)
            for op in (X.UNION, X.INTERSECTION):                    # the clipped last store ends at every phase of the 16-byte grid,
                for cut in range(1, 16 // kb + 1):                  # one element in front of a boundary among them
                    if case.count(op) >= cut:
                        case.run(ctx, op, True, True, case.count(op) - cut)


@gpu
def test_four_byte_buffers_off_the_16_byte_grid(ctx):
    """d_a, d_b and d_out 4, 8 and 12 bytes behind a 16-byte boundary, each at another phase; the origin 8 bytes off"""
    T, _ = limits(ctx, 4)
    _alignment(ctx, 4, [(1, 2, 3), (2, 3, 1), (3, 1, 2), (0, 1, 2), (3, 0, 1), (2, 1, 0)], lambda oo: ((2 * T + 3, T + 1), (T - 1, 3), (3, 2), (1, T + 1 - oo)))


@gpu
def test_eight_byte_buffers_off_the_16_byte_grid(ctx):
    """8-byte keys have one phase off the grid: every buffer 8 bytes off, and every one of the key buffers alone on the grid"""
    T, _ = limits(ctx, 8)
    _alignment(ctx, 8, [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0)], lambda oo: ((2 * T + 3, T + 1), (T - 1, 3), (1, 1), (2, T - oo)))


# ---- cap and null outputs

@gpu
@pytest.mark.parametrize("kb", WIDTHS)
def test_cap_clips_the_stores_and_never_the_count(ctx, kb):
    T, _ = limits(ctx, kb)
    for kind in ("five", "half_shared"):
        a, b = inputs(kind, 2 * T + 3, T + 9, kb, 7)
        case = Case(a, b, UKT[kb], what="cap")
        for op in X.OPS:
            count = case.count(op)
            assert count < case.bound(op) and (count > 0 or (kind == "five" and op in (X.DIFFERENCE, X.SYMMETRIC_DIFFERENCE)))
            for cap in sorted({0, max(count - 1, 0), count, count + 1, case.bound(op)}):   # (both sides hold all of the five values: nothing is left of a difference)
                case.run(ctx, op, True, True, cap)
            case.run(ctx, op, False, True, max(count - 1, 0))
            case.run(ctx, op, True, False, max(count - 1, 0))


@gpu
@pytest.mark.parametrize("kb", WIDTHS)
def test_null_outputs(ctx, kb):
    """a null d_out with the origin given, a null d_out_origin, and both null: the count alone"""
    T, _ = limits(ctx, kb)
    a, b = inputs("half_shared", 2 * T + 3, T + 1, kb, 8)
    case = Case(a, b, UKT[kb], what="null outputs")
    for op in X.OPS:
        case.run(ctx, op, True, False)
        case.run(ctx, op, False, True)
        case.run(ctx, op, False, False)
        case.run(ctx, op, False, False, 0)


# ---- degenerate sizes

@gpu
def test_empty_sides_and_null_pointers(ctx):
    for kb in WIDTHS:
        x = np.sort(uniform(np.random.default_rng(1), 1000, kb, 0, 500))   # (with duplicates)
        Case(x[:0], x, UKT[kb], what="n = 0").run_all(ctx)          # the empty result, or the distinct values of the other side
        Case(x, x[:0], UKT[kb], what="m = 0").run_all(ctx)
        none = Case(x[:0], x[:0], UKT[kb], what="n + m = 0")
        none.run_all(ctx)
        # null pointers where nothing is read
        case = Case(x, x[:0], UKT[kb], what="null d_b")
        for op in X.OPS:
            case.reset()
            ctx._ok(raw_call(ctx, op, case.da.ptr, 1000, 0, 0, case.kt, 1000, case.dout.ptr, case.doo.ptr, case.dnum.ptr))
            case.verify(op, cap=1000, what="null d_b")
        case = Case(x[:0], x, UKT[kb], what="null d_a")
        for op in X.OPS:
            case.reset()
            ctx._ok(raw_call(ctx, op, 0, 0, case.db.ptr, 1000, case.kt, 1000, case.dout.ptr, case.doo.ptr, case.dnum.ptr))
            case.verify(op, cap=1000, what="null d_a")
        for op in X.OPS:                                            # nothing at all: *d_num_out = 0 is still written
            for out, oo, cap in ((0, 0, 0), (0, 0, 5), (none.dout.ptr, none.doo.ptr, 5)):
                none.reset()
                assert int(none.dnum.host()[0]) != 0
                ctx._ok(raw_call(ctx, op, 0, 0, 0, 0, UKT[kb], cap, out, oo, none.dnum.ptr))
                none.verify(op, bool(oo), bool(out), cap, "nothing to write")


# ---- refusals through the C ABI

@gpu
def test_refusals_in_order_touch_nothing(ctx):
    n, m = 1000, 300
    for kb in WIDTHS:
        for kt in (UKT[kb], UKT[kb] + 2):
            a, b = inputs("half_shared", n, m, kb, 4)
            case = Case(S.sort_by_code(a, kt), S.sort_by_code(b, kt), kt, what="refusals")
            bufs = [b for _, b in case.bufs()]
            da, db, dout, doo, dnum = bufs
            good = dict(op=X.UNION, a=da.ptr, n=n, b=db.ptr, m=m, kt=kt, cap=n + m, out=dout.ptr, oo=doo.ptr, num=dnum.ptr)
            order = ("op", "a", "n", "b", "m", "kt", "cap", "out", "oo", "num")

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
            for bad in (-1, 4, 5, 100):
                refused("unknown op", op=bad)
            refused("d_num_out is required", num=0)
            refused("null d_a", a=0)
            refused("null d_b", b=0)
            for name, es in (("a", kb), ("b", kb), ("out", kb), ("oo", 8), ("num", 8)):
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
            refused("must not overlap", oo=da.ptr)
            refused("must not overlap", oo=db.ptr, out=0)
            refused("must not overlap", b=doo.ptr + last * 8)
            refused("must not overlap", num=da.ptr)
            refused("must not overlap", num=db.ptr + (m - 1) * kb - (m - 1) * kb % 8)
            refused("must not overlap", oo=dout.ptr)                # the outputs among each other
            refused("must not overlap", out=doo.ptr + last * 8)
            refused("must not overlap", num=dout.ptr + 8)
            refused("must not overlap", num=doo.ptr + last * 8)
            # the outputs are taken as min(cap, bound) elements long: the last element of that extent still counts
            refused("must not overlap", a=dout.ptr + 9 * kb, cap=10)
            refused("must not overlap", op=X.INTERSECTION, a=dout.ptr + (m - 1) * kb)
            refused("must not overlap", op=X.DIFFERENCE, b=doo.ptr + (n - 1) * 8)
            # the order: of two faults the earlier one is reported
            refused("key_type", kt=9, op=9)
            refused("unknown op", op=9, num=0)
            refused("d_num_out is required", num=0, a=0)
            refused("null d_a", a=0, b=0)
            refused("null d_b", b=0, out=dout.ptr + 1)
            refused("aligned", oo=doo.ptr + 4, n=1 << 36)
            refused("2^36", m=1 << 36, out=da.ptr)
            # and the call that all of these were changes of is fine
            ctx._ok(raw_call(ctx, *[good[x] for x in order]))
            case.verify(X.UNION, what="good")


# ---- asynchrony, the workspace and the phase

@gpu
@pytest.mark.parametrize("kb", WIDTHS)
def test_two_calls_back_to_back_with_a_merge_between(ctx, kb):
    """the calls share the slab: only stream order keeps them apart"""
    import torch
    T, _ = limits(ctx, kb)
    a1, b1 = inputs("five", 7 * T + 5, 5 * T + 1, kb, 21)
    a2, b2 = inputs("half_shared", 2 * T + 3, 9 * T - 1, kb, 22)
    c1, c2 = Case(a1, b1, UKT[kb], what="first"), Case(a2, b2, UKT[kb], what="second")
    merged = Buf(kb, a1.size + b1.size)
    c1.run(ctx, X.UNION)                                            # (the workspace has its size: no reallocation, which would synchronise)
    c1.reset()
    torch.cuda.synchronize()
    ctx._ok(c1.launch(ctx, X.SYMMETRIC_DIFFERENCE))
    ctx._ok(ctx._L.msd_merge_sorted(ctx._h, C.c_void_p(c1.da.ptr), a1.size, C.c_void_p(c1.db.ptr), b1.size, UKT[kb], None, None, C.c_void_p(merged.ptr), None, None))
    ctx._ok(c2.launch(ctx, X.INTERSECTION))
    torch.cuda.synchronize()
    c1.verify(X.SYMMETRIC_DIFFERENCE, what="in front of the merge")
    c2.verify(X.INTERSECTION, what="behind the merge")
    assert (merged.host() == np.sort(np.r_[a1, b1])).all()
    merged.check("d_out of the merge")


@gpu
def test_workspace_grows_by_the_splits_and_the_counts(ctx):
    """one 8-byte split per tile plus one, one 8-byte count per tile, one 8-byte sum per scan piece (256-byte aligned arrays,
    4 KiB of slack); the slab grows in steps of 1 MiB with an eighth on top, and a second call of the same size finds it there"""
    from inplacemsdradixsort_amd import MsdContext
    kb = 4
    T, scan = limits(ctx, kb)
    a, b = inputs("half_shared", 40 * T + 5, 9 * T, kb, 23)
    case = Case(a, b, UKT[kb], what="workspace")
    own = MsdContext(0)
    try:
        before = own.workspace_bytes
        own._ok(case.launch(own, X.UNION))
        after = own.workspace_bytes
        case.verify(X.UNION, what="first")
        tiles = -(-(a.size + b.size) // T)
        up = lambda x: -(-x // 256) * 256
        need = up(8 * (tiles + 1)) + up(8 * tiles) + 8 * -(-tiles // scan) + 4096
        step = 1 << 20
        assert 0 < after - before <= -(-(need + need // 8) // step) * step, (before, after, need)
        case.reset()
        own._ok(case.launch(own, X.DIFFERENCE, False))
        assert own.workspace_bytes == after
        case.verify(X.DIFFERENCE, False, what="second")
    finally:
        own.close()


@gpu
def test_the_phase_is_named(ctx):
    a, b = inputs("half_shared", 1000, 100, 4, 9)
    case = Case(a, b, E.U32, what="phase")
    ctx.set_profiling(True)
    try:
        case.run(ctx, X.UNION)
        assert [p[0] for p in ctx.phases()] == ["set_sorted"]
    finally:
        ctx.set_profiling(False)


# ---- the Python wrappers

@gpu
def test_set_sorted_wrapper_for_every_dtype(ctx):
    import torch
    dts = D.dtypes()
    assert len(dts) == 6
    for dt, kt in dts:
        kb = np.dtype(E.UT[kt]).itemsize
        T, scan = limits(ctx, kb)
        assert ctx.set_sorted_limits(kb) == (T, scan)
        rng = np.random.default_rng(kt)
        sp = special_bits(kt)
        n, m = T + 7, 2 * T - 3
        a_bits, b_bits = [S.sort_by_code(np.r_[sp, uniform(rng, c - sp.size, kb, 0, 1 << 12), ], kt) for c in (n, m)]
        a, b = D.to_gpu(a_bits, dt), D.to_gpu(b_bits, dt)
        before = [x.view(D.int_dtype(kb)).clone() for x in (a, b)]
        for op in X.OPS:
            name = X.OP_NAMES[op]
            want, want_origin = X.expected(a_bits, b_bits, kt, op)
            bound = X.bound(op, n, m)
            num, out = ctx.set_sorted(a, b, name)
            assert num.dtype == torch.int64 and num.shape == (1,) and num.is_cuda and int(num.item()) == want.size
            assert out.dtype == dt and out.shape == (bound,) and (D.bits(out[:want.size]) == want).all()
            num, out, origin = ctx.set_sorted(a, b, name, origin=True)
            assert origin.dtype == torch.int64 and origin.shape == (bound,) and int(num.item()) == want.size
            assert (D.bits(out[:want.size]) == want).all() and (origin[:want.size].cpu().numpy() == want_origin.astype(np.int64)).all()
            cap = want.size // 2
            o, oo = torch.zeros(cap, dtype=dt, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
            r = ctx.set_sorted(a, b, name, cap=cap, out=o, out_origin=oo)
            assert len(r) == 3 and r[1] is o and r[2] is oo and int(r[0].item()) == want.size
            assert (D.bits(o) == want[:cap]).all() and (oo.cpu().numpy() == want_origin[:cap].astype(np.int64)).all()
            num, none = ctx.set_sorted(a, b, name, cap=0)
            assert none.shape == (0,) and int(num.item()) == want.size
        for x, y in zip((a, b), before):                            # the inputs are what they were
            assert torch.equal(x.view(D.int_dtype(kb)), y)
        # empty sides
        distinct = np.unique(E.np_encode(b_bits, kt)).size
        assert int(ctx.set_sorted(a[:0], b, "union")[0].item()) == distinct and int(ctx.set_sorted(a[:0], b, "intersection")[0].item()) == 0
        num, e, eo = ctx.set_sorted(a[:0], b[:0], "union", origin=True)
        assert int(num.item()) == 0 and e.shape == (0,) and eo.shape == (0,) and e.dtype == dt


@gpu
def test_the_1d_conveniences_against_numpy(ctx):
    import torch
    g = torch.Generator(device="cpu").manual_seed(5)
    for dt in (torch.int32, torch.int64, torch.float32, torch.float64):
        a = (torch.randn(5000, generator=g) * 50).to(dt)
        b = (torch.randn(3000, generator=g) * 50 + 20).to(dt)
        if dt.is_floating_point:
            a, b = (a * 8).round() / 8, (b * 8).round() / 8         # (values that meet on both sides)
            a[a == 0] = 1.0                                         # (no zeros of two signs, no NaNs: bitwise and numeric equality agree)
            b[b == 0] = 1.0
        before = (a.clone(), b.clone())
        ga, gb = a.cuda(), b.cuda()
        for f, ref in ((ctx.intersect1d, np.intersect1d), (ctx.union1d, np.union1d), (ctx.setdiff1d, np.setdiff1d), (ctx.setxor1d, np.setxor1d)):
            got, want = f(ga, gb), ref(a.numpy(), b.numpy())
            assert got.dtype == dt and want.size > 0 and got.shape == (want.size,) and (got.cpu().numpy() == want).all(), (dt, ref.__name__)
        assert torch.equal(ga.cpu(), before[0]) and torch.equal(gb.cpu(), before[1])   # unsorted as they were


@gpu
def test_union_is_run_encode_of_the_merge_and_origin_leads_back_to_the_keys(ctx):
    import torch
    rng = np.random.default_rng(6)
    for dt, kdt in ((torch.int32, np.int32), (torch.int64, np.int64)):
        n, m = 30011, 12007
        a = torch.from_numpy(np.sort(rng.integers(-3000, 3000, n).astype(kdt))).cuda()
        b = torch.from_numpy(np.sort(rng.integers(-3500, 2500, m).astype(kdt))).cuda()
        runs, distinct, _, _ = ctx.run_encode(ctx.merge_sorted(a, b), starts=False)
        num, out = ctx.set_sorted(a, b, "union")
        g = int(num.item())
        assert g == int(runs.item()) and torch.equal(out[:g], distinct[:g])
        cat = torch.cat([a, b])
        for op in X.OPS:
            num, out, origin = ctx.set_sorted(a, b, X.OP_NAMES[op], origin=True)
            g = int(num.item())
            assert g > 0 and torch.equal(cat[origin[:g]], out[:g])
            if op in (X.INTERSECTION, X.DIFFERENCE):
                assert int(origin[:g].max().item()) < n             # a value that both sides hold is taken from A
