"""GPU tests of the sort-merge join of two sorted arrays (msd_join_groups, msd_join_pairs; MsdContext.join_groups, join_pairs,
join): the matched groups of two arrays that are ascending in the library's key order, and their expansion into index pairs.

The expected results are defined in tests/join_expect.py and every result is compared exactly.  The calls go through the C
ABI on integer tensors that carry the bit patterns, with EVERY buffer inside a guardband.Arena whose payload is pre-filled
with a known pattern: a case checks the count word, the min(count, cap) results, that no guard was touched, that the inputs
are what was uploaded, that the payload in front of an offset buffer is what it was, that no output word beyond min(count,
cap) changed and that an output that was not given did not change.  The shapes are the smallest at which a kernel can go
wrong, taken from msd_join_limits (T = the tile of the groups call, P = the pair ranks of one workgroup of the expansion).
The buffers are guardband.Buf, the special values those of sort_rows_expect.py and the input kinds come from
test_gpu_set_sorted.py.  Unsorted inputs and made-up groups: test_gpu_untrusted_order.py.  The Python wrappers have a test of their own at the end."""
import ctypes as C

import numpy as np
import pytest

import gpu_support as D
import join_expect as J
import search_expect as S
import set_expect as X
import sort_rows_expect as E
from gpu_support import TAIL
from guardband import Buf
from sort_rows_expect import UKT, WIDTHS, special_bits, uniform
from test_gpu_set_sorted import KINDS, inputs

pytestmark = pytest.mark.gpu

ALL5 = (True,) * 5
NAMES5 = ("d_keys", "d_a_first", "d_a_count", "d_b_first", "d_b_count")
JUNK = 0xDEADBEEFDEADBEEF                                             # in a group word behind the last group: never looked at


def limits(ctx, kb):
    t, s, p = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_join_limits(kb, C.byref(t), C.byref(s), C.byref(p)) == 0
    return int(t.value), int(s.value), int(p.value)


def vp(p):
    return C.c_void_p(p) if p else None


def raw_groups(ctx, a, n, b, m, kt, cap, keys, af, ac, bf, bc, num):
    return ctx._L.msd_join_groups(ctx._h, vp(a), n, vp(b), m, kt, cap, vp(keys), vp(af), vp(ac), vp(bf), vp(bc), vp(num))


def raw_pairs(ctx, gcap, ng, af, ac, bf, bc, n, m, pa, pb, cap, oa, ob, num):
    return ctx._L.msd_join_pairs(ctx._h, gcap, vp(ng), vp(af), vp(ac), vp(bf), vp(bc), n, m, vp(pa), vp(pb), cap, vp(oa), vp(ob), vp(num))


class Groups:
    """A and B (unsigned bit patterns of key type kt, ascending by code) on the device, shared by the calls of the case; every
    buffer `off` elements into its arena.  The five outputs hold min(n, m) + TAIL elements."""

    def __init__(self, a, b, kt, off=0, what=""):
        self.a, self.b, self.kt = a, b, kt
        self.kb, self.n, self.m = a.itemsize, a.size, b.size
        self.bound = min(self.n, self.m)
        self.da, self.db = Buf(self.kb, self.n, off, a=a), Buf(self.kb, self.m, off, a=b)
        self.outs = [Buf(self.kb, self.bound + TAIL, off)] + [Buf(8, self.bound + TAIL, off) for _ in range(4)]
        self.dnum = Buf(8, 1, off)
        self.want = J.groups(a, b, kt)
        self.count = self.want[0].size
        self.what = (what, E.NAMES[kt], self.n, self.m, off)

    def bufs(self):
        return [("d_a", self.da), ("d_b", self.db)] + list(zip(NAMES5, self.outs)) + [("d_num_groups", self.dnum)]

    def launch(self, ctx, cap=None, given=ALL5):
        return raw_groups(ctx, self.da.ptr, self.n, self.db.ptr, self.m, self.kt, self.bound if cap is None else cap,
                          *[g and o.ptr for g, o in zip(given, self.outs)], self.dnum.ptr)

    def verify(self, cap=None, given=ALL5, what=""):
        what = (self.what, cap, given, what)
        stored = min(self.count, self.bound if cap is None else cap)
        num = self.dnum.host()
        assert int(num[0]) == self.count, (what, "*d_num_groups", int(num[0]), self.count)
        for name, g, o, want in zip(NAMES5, given, self.outs, self.want):
            if g:
                got = o.written(stored)
                bad = got != want[:stored]
                assert not bad.any(), (what, name, int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), want[:stored][bad][:4].tolist())
            else:
                assert o.unchanged(), (what, "%s was not given and changed" % name)
        for name, b in self.bufs()[:2]:
            assert b.unchanged(), (what, "%s changed" % name)
        for name, b in self.bufs():
            b.check("%s of %s" % (name, what))

    def reset(self):
        for b in self.outs + [self.dnum]:
            b.reset()

    def run(self, ctx, cap=None, given=ALL5):
        """one call, everything checked"""
        self.reset()
        ctx._ok(self.launch(ctx, cap, given))
        self.verify(cap, given)
        return self


class Pairs:
    """Groups (the four uint64 arrays of join_expect.groups, or made by hand) on the device: `stated` is the word at
    d_num_groups (default: their number), `gcap` the groups_cap of the call (default: their number; beyond the groups the
    arrays hold junk).  pos: random permutations at d_pos_a and d_pos_b.  The outputs hold room + TAIL words."""

    def __init__(self, g, n, m, room, off=0, stated=None, gcap=None, pos=False, what=""):
        four = [np.asarray(x, np.uint64) for x in g[-4:]]
        G = four[0].size
        self.stated, self.gcap = G if stated is None else stated, G if gcap is None else gcap
        pad = np.full(max(self.gcap - G, 0), JUNK, np.uint64)
        self.dng = Buf(8, 1, off, a=np.array([self.stated], np.uint64))
        self.dg = [Buf(8, x.size + pad.size, off, a=np.r_[x, pad]) for x in four]
        used = min(self.stated, self.gcap, G)
        self.g = (None,) + tuple(x[:used] for x in four)
        self.total = J.total(self.g)
        self.n, self.m, self.room = n, m, room
        rng = np.random.default_rng(n + 3 * m)
        self.pa = rng.permutation(n).astype(np.uint64) if pos else None
        self.pb = rng.permutation(m).astype(np.uint64) if pos else None
        self.dpa = Buf(8, n, off, a=self.pa) if pos else None
        self.dpb = Buf(8, m, off, a=self.pb) if pos else None
        self.oa, self.ob = Buf(8, room + TAIL, off), Buf(8, room + TAIL, off)
        self.dnum = Buf(8, 1, off)
        self.what = (what, G, self.stated, self.gcap, n, m, off, pos)

    def inputs(self):
        return [self.dng] + self.dg + ([self.dpa, self.dpb] if self.dpa else [])

    def launch(self, ctx, cap, give_a=True, give_b=True):
        assert cap <= self.room
        return raw_pairs(ctx, self.gcap, self.dng.ptr, *[b.ptr for b in self.dg], self.n, self.m, self.dpa and self.dpa.ptr, self.dpb and self.dpb.ptr, cap,
                         give_a and self.oa.ptr, give_b and self.ob.ptr, self.dnum.ptr)

    def verify(self, cap, give_a=True, give_b=True, what=""):
        what = (self.what, cap, give_a, give_b, what)
        num = self.dnum.host()
        assert int(num[0]) == self.total, (what, "*d_num_pairs", int(num[0]), self.total)
        stored = min(self.total, cap)
        ia, ib = J.pairs(self.g, 0, stored)
        if self.pa is not None:
            ia, ib = self.pa[ia.astype(np.int64)], self.pb[ib.astype(np.int64)]
        for name, given, o, want in (("d_out_a", give_a, self.oa, ia), ("d_out_b", give_b, self.ob, ib)):
            if given:
                got = o.written(stored)
                bad = got != want
                assert not bad.any(), (what, name, int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), want[bad][:4].tolist())
            else:
                assert o.unchanged(), (what, "%s was not given and changed" % name)
        for b in self.inputs():
            assert b.unchanged(), (what, "an input changed")
        for b in self.inputs() + [self.oa, self.ob, self.dnum]:
            b.check(str(what))

    def run(self, ctx, cap, give_a=True, give_b=True):
        for b in (self.oa, self.ob, self.dnum):
            b.reset()
        ctx._ok(self.launch(ctx, cap, give_a, give_b))
        self.verify(cap, give_a, give_b)
        return self


def join_both(ctx, a, b, kt, off=0, what="", pair_cap=None):
    """the groups call, then the pairs of the expected groups (all of them unless pair_cap says less)"""
    gr = Groups(a, b, kt, off, what).run(ctx)
    total = J.total(gr.want)
    cap = total if pair_cap is None else pair_cap
    Pairs(gr.want, a.size, b.size, cap, off, what=what).run(ctx, cap)
    return gr


# ---- the grid of sizes

@pytest.mark.parametrize("kt", J.KEY_TYPES, ids=[E.NAMES[k] for k in J.KEY_TYPES])
def test_sizes_around_the_tile(ctx, kt):
    """n and m around the tile for every kind of input; the pairs of every cell whose product stays small"""
    kb = np.dtype(E.UT[kt]).itemsize
    T, _, P = limits(ctx, kb)
    cells = [(0, 0), (0, 5), (5, 0), (1, 1), (1, T), (T - 1, T + 1), (T, T - 1), (T + 1, 1), (3 * T + 5, T), (T - 1, 3 * T + 5), (0, 3 * T + 5), (3 * T + 5, 0)]
    for kind in KINDS:
        for n, m in cells:
            a, b = inputs(kind, n, m, kb, 3)
            a, b = S.sort_by_code(a, kt), S.sort_by_code(b, kt)
            gr = Groups(a, b, kt, what=kind).run(ctx)
            total = J.total(gr.want)
            cap = min(total, 3 * P + 5)
            Pairs(gr.want, n, m, cap, what=kind).run(ctx, cap)


def test_the_scan_with_more_than_one_piece(ctx):
    """more tile counts, and more groups, than one workgroup of the scan takes: the bases come from two pieces"""
    kb = 8
    T, scan, P = limits(ctx, kb)
    total = (scan + 3) * T + 5
    n = total // 2 + 7
    a, b = inputs("half_shared", n, total - n, kb, 5)
    assert -(-total // T) > scan
    gr = Groups(a, b, UKT[kb], what="two pieces").run(ctx)
    assert gr.count > scan                                           # the products of the pairs call have two pieces too
    Pairs(gr.want, n, total - n, gr.count, what="two pieces").run(ctx, gr.count)


def test_the_offsets_with_one_group_behind_the_first_piece(ctx):
    """scan + 1 groups of one pair each: the offsets' second piece holds a single group, and every offset is its index"""
    _, scan, _ = limits(ctx, 4)
    G = scan + 1
    idx, one = np.arange(G, dtype=np.uint64), np.ones(G, np.uint64)
    Pairs((idx, one, idx, one), G, G, G, what="one pair each").run(ctx, G)
    Pairs((idx, one, idx, one), G, G, G, gcap=G + scan + 7, what="one pair each, pieces behind the last group").run(ctx, scan)


# ---- alignment

@pytest.mark.parametrize("kt", [E.U32, E.I64], ids=["u32", "i64"])
def test_buffers_off_the_16_byte_grid(ctx, kt):
    kb = np.dtype(E.UT[kt]).itemsize
    T, _, P = limits(ctx, kb)
    for off in (1, 3):
        for kind, n, m in (("five", T + 1, T - 1), ("half_shared", 2 * T + 3, T + 1), ("half_shared", 3, 2)):
            a, b = inputs(kind, n, m, kb, off)
            a, b = S.sort_by_code(a, kt), S.sort_by_code(b, kt)
            gr = Groups(a, b, kt, off, "off").run(ctx)
            for cut in (1, 2, 3):
                if gr.count >= cut:
                    gr.run(ctx, gr.count - cut)
            total = J.total(gr.want)
            pr = Pairs(gr.want, n, m, min(total, 2 * P + 3), off, pos=True, what="off")
            for cap in sorted({min(total, 2 * P + 3), min(total, P + 1), max(min(total, P) - 1, 0)}):
                pr.run(ctx, cap)


# ---- runs that leave their tile

def _straddling(T, ut):
    v, lo, hi = ut(1000), np.arange(10, 17, dtype=ut), np.arange(2000, 2009, dtype=ut)
    rep = lambda x, k: np.full(k, x, ut)
    return {
        "long in A": (np.r_[lo[:3], rep(v, 2 * T + 5), hi[:2]], np.r_[lo, rep(v, 3), hi]),
        "long in B": (np.r_[lo, rep(v, 1), hi], np.r_[lo[:3], rep(v, 2 * T + 5), hi[:2]]),
        "both long": (rep(v, T + 3), rep(v, T + 3)),
        "the A run closes a tile, its b's open the next": (rep(v, T), np.r_[rep(v, 5), hi]),
        "... with smaller b's in front": (rep(v, T - 3), np.r_[lo[:3], rep(v, 5), hi]),
        "two matched values meet at a tile edge": (np.r_[rep(v, T - 2), rep(v + ut(1), 4)], np.r_[rep(v, 2), rep(v + ut(1), 3)]),
        "a matched value ends a tile, the next one is in B only": (np.r_[rep(v, T - 2), hi], np.r_[rep(v, 2), rep(v + ut(1), 3), hi[3:]]),
        "disjoint ranges": (np.sort(np.r_[lo, lo]), hi),
        "interleaved, nothing shared": (np.arange(0, 2 * T, 2, dtype=ut), np.arange(1, 2 * T, 2, dtype=ut)),
    }


@pytest.mark.parametrize("kb", WIDTHS)
def test_runs_that_straddle_tiles(ctx, kb):
    T, _, P = limits(ctx, kb)
    for what, (a, b) in _straddling(T, E.UW[kb]).items():
        gr = Groups(a, b, UKT[kb], what=what)
        model = J.tiles(a, b, T)                                     # the model of the kernel agrees with the expectation on these
        assert all((x == y).all() for x, y in zip(model, gr.want)), what
        gr.run(ctx)
        total = J.total(gr.want)
        if what == "both long":
            assert gr.count == 1 and total == (T + 3) ** 2
        if "disjoint" in what or "nothing shared" in what:
            assert gr.count == 0 and total == 0
        cap = min(total, 2 * P + 7)                                  # the true total, and the first cap pairs
        Pairs(gr.want, a.size, b.size, cap, what=what).run(ctx, cap)


# ---- float specials

@pytest.mark.parametrize("kt", [E.F32, E.F64], ids=["f32", "f64"])
def test_float_specials_join_by_their_bits(ctx, kt):
    ut = E.UT[kt]
    kb = np.dtype(ut).itemsize
    T, _, P = limits(ctx, kb)
    rng = np.random.default_rng(kt)
    sp = special_bits(kt)                                            # zeros, denormals, infinities, NaNs of both signs and two payloads

    def draw(count, first):
        x = uniform(rng, count, kb)
        at = rng.random(count) < 0.5
        x[at] = sp[rng.integers(0, sp.size, int(at.sum()))]
        x[:first.size] = first
        return S.sort_by_code(x, kt)

    a, b = draw(T + 1, sp), draw(T - 1, sp)
    gr = join_both(ctx, a, b, kt, what="specials", pair_cap=2 * P + 1)
    assert set(sp.tolist()) <= set(gr.want[0].tolist())
    sign, nan = ut(1 << (8 * kb - 1)), sp[4]
    a = np.array([nan | sign, 0, 0, nan, nan | ut(2)], ut)           # -NaN +0 +0 +NaN +NaN''
    b = np.array([sign, sign, nan, nan, nan | ut(1)], ut)            # -0 -0 +NaN +NaN +NaN'
    gr = join_both(ctx, a, b, kt, what="zeros and NaNs")
    assert [x.tolist() for x in gr.want] == [[nan], [3], [1], [2], [2]]


# ---- caps and outputs that are not given

@pytest.mark.parametrize("kb", WIDTHS)
def test_caps_of_the_groups_call(ctx, kb):
    T, _, _ = limits(ctx, kb)
    for kind in ("five", "half_shared"):
        a, b = inputs(kind, 2 * T + 3, T + 9, kb, 7)
        gr = Groups(a, b, UKT[kb], what="cap")
        count = gr.count
        assert 0 < count < gr.bound
        for cap in sorted({0, 1, count - 1, count, count + 5}):
            gr.run(ctx, cap)
        for out in range(5):                                         # each output omitted in turn, and given alone
            gr.run(ctx, None, tuple(i != out for i in range(5)))
            gr.run(ctx, count - 1, tuple(i == out for i in range(5)))
        gr.run(ctx, None, (False,) * 5)                              # the count alone


def _shapes(P):
    """groups made by hand: (a_first, a_count, b_first, b_count), n, m"""
    ones = np.arange(4 * P, dtype=np.uint64)
    u = lambda *x: np.array(x, np.uint64)
    return {
        "4P groups of one pair": ((ones, np.ones_like(ones), ones + np.uint64(7), np.ones_like(ones)), 4 * P, 4 * P + 7),
        "a row, a column and a block": ((u(2, 5, P + 9), u(1, P + 1, 7), u(0, 2 * P + 3, 2 * P + 10), u(2 * P + 3, 1, 5)), P + 20, 2 * P + 15),
    }


def test_caps_of_the_pairs_call_and_pair_shapes(ctx):
    _, _, P = limits(ctx, 4)
    for what, (g, n, m) in _shapes(P).items():
        pr = Pairs(g, n, m, 0, what=what)
        total = pr.total
        assert total > 3 * P
        pr = Pairs(g, n, m, total, what=what)
        for cap in (0, 1, P - 1, P, P + 1, total - 1, total):
            pr.run(ctx, cap)
        pr.run(ctx, total, True, False)
        pr.run(ctx, P + 1, False, True)
        pr.run(ctx, total, False, False)
        G = g[0].size
        Pairs(g, n, m, total, stated=G, gcap=G - 1, what="groups_cap below *d_num_groups").run(ctx, total)
        Pairs(g, n, m, total, stated=G - 1, gcap=G + 3, what="junk behind the groups").run(ctx, total)
        Pairs(g, n, m, total, stated=0, gcap=G, what="no group").run(ctx, total)
    none = [np.zeros(0, np.uint64)] * 4
    Pairs(none, 5, 5, 9, what="groups_cap == 0").run(ctx, 9)


def test_pairs_through_positions(ctx):
    kb = 4
    T, _, P = limits(ctx, kb)
    a, b = inputs("five", T + 1, T - 1, kb, 11)
    g = J.groups(a, b, UKT[kb])
    cap = 2 * P + 5
    assert J.total(g) > cap
    Pairs(g, a.size, b.size, cap, pos=True, what="positions").run(ctx, cap)
    a, b = inputs("half_shared", 2 * T + 3, T + 1, kb, 12)
    g = J.groups(a, b, UKT[kb])
    Pairs(g, a.size, b.size, J.total(g), pos=True, what="positions").run(ctx, J.total(g))


# ---- consistency with the intersection

@pytest.mark.parametrize("kb", WIDTHS)
def test_keys_and_a_first_are_the_intersection_with_origin(ctx, kb):
    T, _, _ = limits(ctx, kb)
    for kind in ("five", "half_shared", "a_equal_in_distinct_b"):
        a, b = inputs(kind, 2 * T + 3, T + 9, kb, 13)
        gr = Groups(a, b, UKT[kb], what="consistency").run(ctx)
        out, origin, num = Buf(kb, gr.bound + TAIL), Buf(8, gr.bound + TAIL), Buf(8, 1)
        ctx._ok(ctx._L.msd_set_sorted(ctx._h, X.INTERSECTION, vp(gr.da.ptr), gr.n, vp(gr.db.ptr), gr.m, gr.kt, gr.bound, vp(out.ptr), vp(origin.ptr), vp(num.ptr)))
        assert int(num.host()[0]) == int(gr.dnum.host()[0]) == gr.count
        assert (out.host() == gr.outs[0].host()).all() and (origin.host() == gr.outs[1].host()).all()   # (the untouched tails hold one pattern)


# ---- refusals through the C ABI

def test_refusals_in_order_touch_nothing(ctx):
    n, m = 1000, 300
    for kt in (E.U32, E.F32, E.I64):
        kb = np.dtype(E.UT[kt]).itemsize
        a, b = inputs("half_shared", n, m, kb, 4)
        gr = Groups(S.sort_by_code(a, kt), S.sort_by_code(b, kt), kt, what="refusals")
        bufs = [b for _, b in gr.bufs()]
        da, db, dk, daf, dac, dbf, dbc, dnum = bufs
        good = dict(a=da.ptr, n=n, b=db.ptr, m=m, kt=kt, cap=m, keys=dk.ptr, af=daf.ptr, ac=dac.ptr, bf=dbf.ptr, bc=dbc.ptr, num=dnum.ptr)
        order = ("a", "n", "b", "m", "kt", "cap", "keys", "af", "ac", "bf", "bc", "num")

        def refused(message, **change):
            k = dict(good, **change)
            rc = raw_groups(ctx, *[k[x] for x in order])
            err = ctx._L.msd_last_error(ctx._h).decode()
            assert rc == -1 and message in err, (change, rc, err)
            for buf in bufs:
                assert buf.unchanged(), change
                buf.check(str(change))

        for bad in (-1, 6, 7, 100):
            refused("key_type", kt=bad)
        refused("d_num_groups is required", num=0)
        refused("null d_a", a=0)
        refused("null d_b", b=0)
        for name, es in (("a", kb), ("b", kb), ("keys", kb), ("af", 8), ("ac", 8), ("bf", 8), ("bc", 8), ("num", 8)):
            for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                refused("aligned", **{name: good[name] + d})
        for big in (1 << 32, 1 << 36, (1 << 64) - 1):
            refused("2^32", n=big)
            refused("2^32", m=big)
        last = m - 1                                                 # the outputs are taken as min(cap, n, m) elements long
        for name in ("keys", "af", "ac", "bf", "bc", "num"):
            refused("must not overlap", **{name: da.ptr})
            refused("must not overlap", **{name: db.ptr + (m - 1) * kb - (m - 1) * kb % 8})
        refused("must not overlap", a=dk.ptr + last * kb)
        refused("must not overlap", b=dbc.ptr + last * 8)
        refused("must not overlap", af=dk.ptr, keys=dk.ptr)          # the outputs among each other
        refused("must not overlap", ac=daf.ptr + last * 8)
        refused("must not overlap", bc=dbf.ptr)
        refused("must not overlap", num=dac.ptr + 8)
        refused("must not overlap", a=dk.ptr + 9 * kb, cap=10)
        # the order: of two faults the earlier one is reported
        refused("key_type", kt=9, num=0)
        refused("d_num_groups is required", num=0, a=0)
        refused("null d_a", a=0, b=0)
        refused("null d_b", b=0, keys=dk.ptr + 1)
        refused("aligned", af=daf.ptr + 4, n=1 << 32)
        refused("2^32", m=1 << 32, keys=da.ptr)
        # and the call that all of these were changes of is fine
        ctx._ok(raw_groups(ctx, *[good[x] for x in order]))
        gr.verify(m, what="good")

        # the pairs call on these groups
        pr = Pairs(gr.want, n, m, J.total(gr.want), pos=True, what="refusals")
        pb = pr.inputs() + [pr.oa, pr.ob, pr.dnum]
        dng, gaf, gac, gbf, gbc, dpa, dpb, oa, ob, dnp = pb
        G = gr.count
        pgood = dict(gcap=G, ng=dng.ptr, af=gaf.ptr, ac=gac.ptr, bf=gbf.ptr, bc=gbc.ptr, n=n, m=m, pa=dpa.ptr, pb=dpb.ptr, cap=pr.total, oa=oa.ptr, ob=ob.ptr, num=dnp.ptr)
        porder = ("gcap", "ng", "af", "ac", "bf", "bc", "n", "m", "pa", "pb", "cap", "oa", "ob", "num")

        def prefused(message, **change):
            k = dict(pgood, **change)
            rc = raw_pairs(ctx, *[k[x] for x in porder])
            err = ctx._L.msd_last_error(ctx._h).decode()
            assert rc == -1 and message in err, (change, rc, err)
            for buf in pb:
                assert buf.unchanged(), change
                buf.check(str(change))

        prefused("d_num_pairs is required", num=0)
        prefused("null d_num_groups", ng=0)
        for name in ("af", "ac", "bf", "bc"):
            prefused("null group array", **{name: 0})
        for name in ("ng", "af", "ac", "bf", "bc", "pa", "pb", "oa", "ob", "num"):
            for d in (1, 2, 4, 7):
                prefused("aligned", **{name: pgood[name] + d})
        for big in (1 << 32, (1 << 64) - 1):
            prefused("2^32", n=big)
            prefused("2^32", m=big)
            prefused("2^32", gcap=big)
        prefused("2^40", n=(1 << 32) - 1, m=(1 << 32) - 1, cap=1 << 40, pa=0, pb=0)
        for name in ("oa", "ob", "num"):
            for inp in (dng, gaf, gac, gbf, gbc, dpa, dpb):
                prefused("must not overlap", **{name: inp.ptr})
        prefused("must not overlap", ob=oa.ptr + 8 * (pr.total - 1))
        prefused("must not overlap", num=ob.ptr)
        prefused("must not overlap", pa=oa.ptr + 8 * 9, cap=10)
        # the order
        prefused("d_num_pairs is required", num=0, ng=0)
        prefused("null d_num_groups", ng=0, af=0)
        prefused("null group array", bc=0, oa=oa.ptr + 4)
        prefused("aligned", oa=oa.ptr + 4, n=1 << 32)
        prefused("2^32", m=1 << 32, oa=gaf.ptr)
        ctx._ok(raw_pairs(ctx, *[pgood[x] for x in porder]))
        pr.verify(pr.total, what="good")


# ---- asynchrony and the phases

def test_the_phases_are_named_and_the_calls_share_the_stream(ctx):
    import torch
    T, _, P = limits(ctx, 4)
    a, b = inputs("five", 2 * T + 3, T + 1, 4, 9)
    gr = Groups(a, b, E.U32, what="phase")
    pr = Pairs(gr.want, a.size, b.size, 3 * P, what="phase")
    ctx.set_profiling(True)
    try:
        gr.run(ctx)
        assert [p[0] for p in ctx.phases()] == ["join_groups"]
        pr.run(ctx, 3 * P)
        assert [p[0] for p in ctx.phases()] == ["join_pairs"]
    finally:
        ctx.set_profiling(False)
    # the pairs call reads what the groups call wrote, with nothing but stream order between them
    gr.reset()
    torch.cuda.synchronize()
    oa, ob, num = Buf(8, 3 * P + TAIL), Buf(8, 3 * P + TAIL), Buf(8, 1)
    ctx._ok(gr.launch(ctx))
    ctx._ok(raw_pairs(ctx, gr.bound, gr.dnum.ptr, *[o.ptr for o in gr.outs[1:]], a.size, b.size, 0, 0, 3 * P, oa.ptr, ob.ptr, num.ptr))
    torch.cuda.synchronize()
    gr.verify(what="in front of the pairs")
    ia, ib = J.pairs(gr.want, 0, 3 * P)
    assert int(num.host()[0]) == J.total(gr.want) and (oa.written(3 * P) == ia).all() and (ob.written(3 * P) == ib).all()


# ---- the Python wrappers

def test_join_of_unsorted_tensors(ctx):
    import torch
    rng = np.random.default_rng(17)
    for dt, npdt in ((torch.int32, np.int32), (torch.float32, np.float32), (torch.int64, np.int64)):
        kb = np.dtype(npdt).itemsize
        pool = rng.integers(-100000, 100000, 300)
        av, bv = pool[rng.integers(0, 260, 5000)].astype(npdt), pool[rng.integers(40, 300, 4000)].astype(npdt)
        if dt.is_floating_point:
            av, bv = av / npdt(8), bv / npdt(8)
        a, b = torch.from_numpy(av).cuda(), torch.from_numpy(bv).cuda()
        ia, ib = ctx.join(a, b)
        assert ia.dtype == ib.dtype == torch.int64 and ia.shape == ib.shape and ia.dim() == 1
        abits, bbits = av.view(E.UW[kb]), bv.view(E.UW[kb])
        wi, wj = np.nonzero(abits[:, None] == bbits[None, :])       # the brute-force join on the bits
        got = np.stack([ia.cpu().numpy(), ib.cpu().numpy()], 1)
        assert got.shape[0] == wi.size > 10000
        assert (abits[got[:, 0]] == bbits[got[:, 1]]).all()
        key = lambda i, j: np.sort(i.astype(np.int64) * bv.size + j)
        assert (key(got[:, 0], got[:, 1]) == key(wi, wj)).all()     # the same set of pairs, none twice
        assert torch.equal(a.cpu(), torch.from_numpy(av)) and torch.equal(b.cpu(), torch.from_numpy(bv))   # unsorted as they were
        # the wrappers of the two calls on the sorted copies
        sa, sb = np.sort(av), np.sort(bv)
        kt = {torch.int32: E.I32, torch.float32: E.F32, torch.int64: E.I64}[dt]
        want = J.groups(sa.view(E.UW[kb]), sb.view(E.UW[kb]), kt)
        ga, gb = D.to_gpu(sa.view(E.UW[kb]), dt), D.to_gpu(sb.view(E.UW[kb]), dt)
        groups = ctx.join_groups(ga, gb)
        G = int(groups[0].item())
        assert G == want[0].size and groups[1].dtype == dt and all(t.dtype == torch.int64 and t.shape == (4000,) for t in groups[2:])
        assert (D.bits(groups[1][:G]) == want[0]).all() and all((t[:G].cpu().numpy() == w.astype(np.int64)).all() for t, w in zip(groups[2:], want[1:]))
        assert ctx.join_groups(ga[:0], gb)[0].item() == 0 and ctx.join_groups(ga, gb, keys=False)[1] is None
        num, _, _ = ctx.join_pairs(groups, 5000, 4000, 0)
        assert int(num.item()) == wi.size
        out_a = torch.zeros(1000, dtype=torch.int64, device="cuda")
        num, ra, rb = ctx.join_pairs(groups, 5000, 4000, 1000, out_a=out_a)
        wa, wb = J.pairs(want, 0, 1000)
        assert ra is out_a and int(num.item()) == wi.size and (ra.cpu().numpy() == wa.astype(np.int64)).all() and (rb.cpu().numpy() == wb.astype(np.int64)).all()
        e = ctx.join(a[:0], b)
        assert e[0].shape == (0,) and e[1].shape == (0,) and e[0].dtype == torch.int64
    assert ctx.join_limits(4) == limits(ctx, 4) and ctx.join_limits(8) == limits(ctx, 8)
