"""GPU tests of the calls that TRUST their inputs to be ascending -- msd_search_sorted under the merge path, msd_merge_sorted,
msd_set_sorted, msd_join_groups -- on inputs that are NOT, and of msd_join_pairs on groups this library did not write: the
third of the three layers of DESIGN.md 10.13.  The headers promise unspecified values and counts, but every load inside its
input array and every store inside the stated range of its output.

LOADS are checked on the CPU (tests/test_clamps_host.py, tests/test_clamp_models.py).  Here every buffer, inputs included,
sits in a guardband.Arena whose payload is pre-filled with a known pattern, and every case checks the STORES, the COUNTS and
where the VALUES came from: the return code; that no guard was touched; that the inputs are bit-identical afterwards; that no
output cell beyond the promised range changed; that an output that was not given did not change; that a count word holds
what the clamped model (search_expect.stored_clamped, set_expect.count_np, join_expect.expand_clamped at the kernels' real
tile) says; and that a stored value is one the model allows, an index below n + m, or one of the distinct tags that only the
right value array holds -- a load outside it would bring a cell of the guard pattern.  After each family the same entry
point runs on the same context with sorted inputs of the same shape and is compared exactly with the usual expectation."""
import ctypes as C

import numpy as np
import pytest

import join_expect as J
import merge_expect as M
import search_expect as S
import set_expect as X
import sort_rows_expect as E
import test_gpu_join as GJ
import test_gpu_merge_sorted as GM
import test_gpu_search as GS
import test_gpu_set_sorted as GX
from gpu_support import TAIL
from guardband import Buf
from sort_rows_expect import UKT, WIDTHS, top

gpu = pytest.mark.gpu                                               # (test_the_inputs_are_what_they_say needs none)

KINDS = ["reversed", "shuffled", "a_sorted_b_reversed", "a_reversed_b_sorted", "alternating", "sawtooth", "block_in_front", "float_torch_order"]
TAG = 0x7A60 << 48                                                  # tags: TAG + an index below 2^32
PAIR_TH, PAIR_PER = 256, 8                                          # kJoinPairTh, kJoinPairPer of csrc/msd_join.hpp


def _lib():
    from inplacemsdradixsort_amd import _lib as L
    return L.load()


def tile_of(kb):
    """T: the elements of one workgroup of the four tile kernels (the four *_limits calls agree; host only)"""
    t, x, y = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L = _lib()
    assert L.msd_merge_sorted_limits(kb, C.byref(t)) == 0
    tiles = [int(t.value)]
    assert L.msd_search_sorted_limits(kb, C.byref(t), C.byref(x)) == 0
    tiles.append(int(t.value))
    assert L.msd_set_sorted_limits(kb, C.byref(t), C.byref(x)) == 0
    tiles.append(int(t.value))
    assert L.msd_join_limits(kb, C.byref(t), C.byref(x), C.byref(y)) == 0
    tiles.append(int(t.value))
    assert len(set(tiles)) == 1, tiles
    return tiles[0]


def join_limits(kb):
    t, s, p = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert _lib().msd_join_limits(kb, C.byref(t), C.byref(s), C.byref(p)) == 0
    assert int(p.value) == PAIR_TH * PAIR_PER
    return int(t.value), int(s.value), int(p.value)


def shapes(T):
    return [(3 * T - 1, 2 * T + 5), (T + 1, T - 1), (3 * T + 5, 7), (7, 3 * T + 5), (1, 2 * T), (2 * T, 0)]


def torch_sort_order(rng, count, kb):
    """the bits of floats as torch.sort leaves them: ascending by VALUE, so +0.0 and -0.0 in the order they came in (here
    +0.0 first), and the NaNs of both signs last, in the order they came in -- by totalOrder a -NaN belongs in front"""
    ft = np.float32 if kb == 4 else np.float64
    x = np.sort(rng.integers(-6, 7, count).astype(ft) / 2)
    zeros = np.flatnonzero(x == 0)
    x[zeros[1::2]] = -0.0
    bits = x.view(E.UW[kb]).copy()
    sign = E.UW[kb](1 << (8 * kb - 1))
    nan = E.UW[kb](0x7FC00000 if kb == 4 else 0x7FF8 << 48)
    k = min(count, 5)
    bits[count - k:] = np.array([nan, nan | sign, nan | E.UW[kb](5), nan | sign | E.UW[kb](5), nan], E.UW[kb])[:k]
    return bits


def inputs(kind, n, m, kb, T):
    """``(a_bits, b_bits, key_type)``: A and B, NOT ascending in the order of the type (a side of 0 or 1 elements is)"""
    rng = np.random.default_rng([n, m, kb, KINDS.index(kind)])
    ut, kt = E.UW[kb], UKT[kb]
    span = max((n + m) // 2, 2)                                     # few enough values that the two sides share many
    draw = lambda count: rng.integers(0, span, count).astype(ut)
    up = np.sort
    down = lambda x: np.sort(x)[::-1].copy()
    if kind == "reversed":
        a, b = down(draw(n)), down(draw(m))
    elif kind == "shuffled":
        a, b = draw(n), draw(m)
    elif kind == "a_sorted_b_reversed":
        a, b = up(draw(n)), down(draw(m))
    elif kind == "a_reversed_b_sorted":
        a, b = down(draw(n)), up(draw(m))
    elif kind == "alternating":                                     # 0 and all ones, the two sides in opposite phase
        a = np.where(np.arange(n) % 2, top(kb), 0).astype(ut)
        b = np.where(np.arange(m) % 2, 0, top(kb)).astype(ut)
    elif kind == "sawtooth":                                        # periods of T + 1 against T - 1
        a, b = (np.arange(n) % (T + 1)).astype(ut), (np.arange(m) % (T - 1)).astype(ut)
    elif kind == "block_in_front":                                  # one block of large keys in front of an otherwise sorted A
        a, b = up(draw(n)), up(draw(m))
        k = min(n, T // 2 + 3)
        a[:k] = ut(top(kb)) - np.arange(k, dtype=ut)[::-1] // ut(2)
    else:                                                           # "float_torch_order"
        kt = E.F32 if kb == 4 else E.F64
        a, b = torch_sort_order(rng, n, kb), torch_sort_order(rng, m, kb)
    return a, b, kt


def codes_of(a, b, kt):
    return E.np_encode(a, kt), E.np_encode(b, kt)


def test_the_inputs_are_what_they_say():
    """The kinds are not ascending, the float kind is what torch.sort leaves, and -- with the clamped models at the real T --
    together they hit every clamp the GPU tests are there for.  The extents and the search's stores of every kind come from
    the vectorised models; the places with two elements and with none, and the write tiles that compact too few, from the
    statement-by-statement models of two kinds at the smaller tile."""
    hit = S.Stats()
    for kb in WIDTHS:
        T = tile_of(kb)
        n, m = shapes(T)[0]
        for kind in KINDS:
            a, b, kt = inputs(kind, n, m, kb, T)
            ca, cb = codes_of(a, b, kt)
            assert a.size == n and b.size == m and ((ca[1:] < ca[:-1]).any() or (cb[1:] < cb[:-1]).any()), kind
            for right in (False, True):
                S.extents(ca, cb, T, right, hit)
                index, _ = S.stored_clamped(ca, cb, T, right)
                hit.hit("covered_twice", index.size - np.unique(index).size)
            if kb == 8 and kind in ("shuffled", "float_torch_order"):
                M.tiles_clamped(ca, cb, T, stats=hit)
                X.tiles_clamped(ca, cb, T, X.UNION, stats=hit)
                J.tiles_clamped(ca, cb, T, stats=hit)
        for kind in ("float_torch_order",):
            a, b, kt = inputs(kind, n, m, kb, T)
            for x in (a, b):
                f = x.view(np.float32 if kb == 4 else np.float64)
                sign = x >> E.UW[kb](8 * kb - 1)
                finite = f[~np.isnan(f)]
                assert (finite[1:] >= finite[:-1]).all() and np.isnan(f[finite.size:]).all()       # torch.sort's order
                zeros = np.flatnonzero(f == 0)
                assert zeros.size >= 2 and sign[zeros[0]] == 0 and sign[zeros[1]] == 1              # +0.0 before -0.0
                assert set(sign[np.isnan(f)].tolist()) == {0, 1}                                    # NaNs of both signs
    for what in ("a_descends", "b_descends", "na_over_tile", "nb_clipped", "collision", "hole", "covered_twice", "unplaced"):
        assert hit.get(what), (what, dict(hit))


# ---- what every case checks

def unchanged(bufs, what):
    for name, b in bufs:
        assert b.unchanged(), (what, "%s changed" % name)


def guards(bufs, what):
    for name, b in bufs:
        b.check("%s of %s" % (name, what))


def assert_no_tags(*bufs):
    """the tags occur in no guard of an 8-byte buffer and in no pre-filled payload (a payload of tags starts with one)"""
    is_tag = lambda x: ((x >= TAG) & (x < TAG + (1 << 32))).any()
    for b in bufs:
        if b.es == 8:
            assert b.count and is_tag(b.fill[b.off:b.off + 1]) or not is_tag(b.fill)
            for side in ("front", "back"):
                assert not is_tag(b.arena._expected(side).cpu().numpy().view(np.uint64)), side


def tagged(x, count):
    """are all of x tags of an array of `count` elements?"""
    return ((x >= TAG) & (x < TAG + count)).all()


# ---- the search

@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_search_with_unsorted_needles_keys_and_both(ctx, kb, kind):
    """every cell of d_out is its pre-fill or a value the clamped model says some tile stores there, all <= n"""
    T = tile_of(kb)
    turn = 0
    for n, m in shapes(T):
        a, b, kt = inputs(kind, n, m, kb, T)
        for vary in ("needles", "keys", "both"):
            keys = a if vary != "needles" else S.sort_by_code(a, kt)
            needles = b if vary != "keys" else S.sort_by_code(b, kt)
            ck, cn = codes_of(keys, needles, kt)
            perm = np.random.default_rng(m).permutation(m).astype(np.uint64)
            dkeys, dneedles, dpos, dout = Buf(kb, n, a=keys), Buf(kb, m, a=needles), Buf(8, m, a=perm), Buf(8, m + TAIL)
            bufs = (("d_sorted", dkeys), ("d_needles", dneedles), ("d_positions", dpos), ("d_out", dout))
            for right, positions in ((False, False), (True, True)) if turn % 2 else ((True, False), (False, True)):
                what = (kind, E.NAMES[kt], n, m, vary, "right" if right else "left", positions)
                dout.reset()
                with GS.Mode(ctx, GS.MERGE):
                    ctx._ok(GS.raw_call(ctx, dkeys.ptr, kt, n, dneedles.ptr, m, 1, int(right), positions and dpos.ptr, dout.ptr))
                got = dout.written(m)                               # (nothing behind the m words changed)
                index, value = S.stored_clamped(ck, cn, T, right, perm.astype(np.int64) if positions else None)
                assert index.size == 0 or (0 <= index.min() and index.max() < m and 0 <= value.min() and value.max() <= n), what
                stored = np.zeros(m, bool)
                stored[index] = True
                assert (got[~stored] == dout.fill[:m][~stored]).all(), (what, "a cell no tile stores to changed")
                small = got[stored]
                assert (small <= n).all(), (what, "a result above n", small[small > n][:4].tolist())
                allowed = np.unique(index * (n + 1) + value)
                bad = ~np.isin(np.flatnonzero(stored) * (n + 1) + small.astype(np.int64), allowed)
                assert not bad.any(), (what, "a value no tile stores there", int(bad.sum()), np.flatnonzero(stored)[bad][:4].tolist(), small[bad][:4].tolist())
                unchanged(bufs[:3], what)
                guards(bufs, what)
            turn += 1
        # the same entry point on the same context with sorted inputs of the same shape
        case = GS.Case(S.sort_by_code(a, kt), S.sort_by_code(b, kt), kt, what="sorted behind " + kind)
        case.run(ctx, GS.MERGE, True)
        case.run(ctx, GS.MERGE, False)


# ---- the merge

@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_merge_of_unsorted_inputs(ctx, kb, kind):
    """keys only, and with values and origin: every origin below n + m, every value a tag of vals_a / vals_b, nothing
    behind n + m"""
    T = tile_of(kb)
    for n, m in shapes(T):
        a, b, kt = inputs(kind, n, m, kb, T)
        total = n + m
        va, vb = TAG + np.arange(n, dtype=np.uint64), TAG + n + np.arange(m, dtype=np.uint64)
        da, db, dva, dvb = Buf(kb, n, a=a), Buf(kb, m, a=b), Buf(8, n, a=va), Buf(8, m, a=vb)
        dout, dov, doo = Buf(kb, total + TAIL), Buf(8, total + TAIL), Buf(8, total + TAIL)
        bufs = (("d_a", da), ("d_b", db), ("d_vals_a", dva), ("d_vals_b", dvb), ("d_out", dout), ("d_out_vals", dov), ("d_out_origin", doo))
        assert_no_tags(*[x for _, x in bufs])
        for with_values in (False, True):
            what = (kind, E.NAMES[kt], n, m, with_values)
            for x in (dout, dov, doo):
                x.reset()
            ctx._ok(GM.raw_call(ctx, da.ptr, n, db.ptr, m, kt, with_values and dva.ptr, with_values and dvb.ptr, dout.ptr, with_values and dov.ptr,
                                with_values and doo.ptr))
            dout.written(total)                                     # (the TAIL is what it was; a position no element was ranked to holds whatever the LDS held)
            if with_values:
                origin, vals = doo.written(total), dov.written(total)
                assert (origin < total).all(), (what, "an origin beyond n + m", origin[origin >= total][:4].tolist())
                assert tagged(vals, total), (what, "a value from outside vals_a and vals_b", vals[(vals < TAG) | (vals >= TAG + total)][:4].tolist())
            else:
                assert dov.unchanged() and doo.unchanged(), (what, "an output that was not given changed")
            unchanged(bufs[:4], what)
            guards(bufs, what)
        GM.Case(S.sort_by_code(a, kt), S.sort_by_code(b, kt), kt, what="sorted behind " + kind).run_all(ctx)


# ---- the set operations

def caps_of(count):
    """no cap (TAIL // 2 above the count: the buffers hold TAIL more), count - 1, 1 and 0; and which outputs are given"""
    caps = [(count + TAIL // 2, True, True), (count - 1, True, False), (1, False, True), (0, True, True)]
    return [c for c in caps if c[0] >= 0]


def set_case(ctx, a, b, kt, T, ops, what, all_caps=True):
    n, m, kb = a.size, b.size, a.itemsize
    ca, cb = codes_of(a, b, kt)
    counts = {op: sum(X.count_np(ca, cb, T, op)) for op in ops}
    room = max(counts.values()) + TAIL
    da, db, dout, doo, dnum = Buf(kb, n, a=a), Buf(kb, m, a=b), Buf(kb, room), Buf(8, room), Buf(8, 1)
    bufs = (("d_a", da), ("d_b", db), ("d_out", dout), ("d_out_origin", doo), ("d_num_out", dnum))
    for op in ops:
        count = counts[op]
        for cap, give_out, give_origin in caps_of(count)[:None if all_caps else 2]:
            w = (what, X.OP_NAMES[op], cap, give_out, give_origin)
            for x in (dout, doo, dnum):
                x.reset()
            ctx._ok(GX.raw_call(ctx, op, da.ptr, n, db.ptr, m, kt, cap, give_out and dout.ptr, give_origin and doo.ptr, dnum.ptr))
            num = int(dnum.host()[0])
            assert num == count, (w, "*d_num_out", num, count)      # the count kernel has no race: the model's number
            stored = min(count, cap)
            if give_out:
                dout.written(stored)                                # (nothing behind min(count, cap) changed)
            else:
                assert dout.unchanged(), (w, "d_out was not given and changed")
            if give_origin:
                origin = doo.written(stored)
                assert (origin < n + m).all(), (w, "an origin beyond n + m", origin[origin >= n + m][:4].tolist())
            else:
                assert doo.unchanged(), (w, "d_out_origin was not given and changed")
            unchanged(bufs[:2], w)
            guards(bufs, w)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_set_operations_on_unsorted_inputs(ctx, kb, kind):
    """*d_num_out is the clamped model's count; nothing behind min(count, cap); origins below n + m"""
    T = tile_of(kb)
    for n, m in shapes(T):
        a, b, kt = inputs(kind, n, m, kb, T)
        set_case(ctx, a, b, kt, T, X.OPS, (kind, E.NAMES[kt], n, m))
        GX.Case(S.sort_by_code(a, kt), S.sort_by_code(b, kt), kt, what="sorted behind " + kind).run_all(ctx)


def reversed_over_a_scan_piece(kb):
    """more tiles than one scan piece: (scan_tile + 1) * T + 5 elements, both sides descending"""
    T, scan, _ = join_limits(kb)
    total = (scan + 1) * T + 5
    n = total * 3 // 5
    rng = np.random.default_rng(kb)
    draw = lambda count: np.sort(rng.integers(0, total // 2, count).astype(E.UW[kb]))[::-1].copy()
    return draw(n), draw(total - n), T


@gpu
@pytest.mark.parametrize("kb", WIDTHS)
def test_a_union_of_reversed_inputs_with_more_than_one_scan_piece(ctx, kb):
    a, b, T = reversed_over_a_scan_piece(kb)
    set_case(ctx, a, b, UKT[kb], T, (X.UNION,), ("reversed, scan pieces", kb), all_caps=False)


# ---- the groups and their pairs

def pairs_case(ctx, g, stated, gcap, n, m, caps, positions, what):
    """msd_join_pairs on the four columns g (gcap words each) against join_expect.expand_clamped, exactly: the expansion has
    no race and reads no cell nothing wrote.  With positions every stored word is a tag of pos_a / pos_b."""
    P = PAIR_TH * PAIR_PER
    cols = [np.asarray(x, np.uint64) for x in g]
    room = max(caps)
    dng = Buf(8, 1, a=np.array([stated], np.uint64))
    dg = [Buf(8, gcap, a=x) for x in cols]
    pa, pb = TAG + np.arange(n, dtype=np.uint64), TAG + (1 << 31) + np.arange(m, dtype=np.uint64)
    dpa, dpb = Buf(8, n, a=pa), Buf(8, m, a=pb)
    oa, ob, dnum = Buf(8, room + TAIL), Buf(8, room + TAIL), Buf(8, 1)
    ins = [("d_num_groups", dng)] + list(zip(GJ.NAMES5[1:], dg)) + [("d_pos_a", dpa), ("d_pos_b", dpb)]
    bufs = ins + [("d_out_a", oa), ("d_out_b", ob), ("d_num_pairs", dnum)]
    assert_no_tags(*[x for _, x in bufs])
    lists = [x.tolist() for x in cols]
    for turn, cap in enumerate(caps):
        give_a, give_b = turn % 3 != 1, turn % 3 != 2
        w = (what, stated, gcap, n, m, cap, positions, give_a, give_b)
        want = J.expand_clamped(stated, gcap, *lists, n, m, pa.tolist() if positions else None, pb.tolist() if positions else None, cap, PAIR_TH, PAIR_PER)
        for x in (oa, ob, dnum):
            x.reset()
        ctx._ok(GJ.raw_pairs(ctx, gcap, dng.ptr, *[x.ptr for x in dg], n, m, positions and dpa.ptr, positions and dpb.ptr, cap, give_a and oa.ptr, give_b and ob.ptr,
                             dnum.ptr))
        num = int(dnum.host()[0])
        assert num == want.total, (w, "*d_num_pairs", num, want.total)     # the wrapping sum of the first G products
        assert want.out_a.indices() <= set(range(min(want.total, cap))), w
        for name, given, o, stores, count, first in (("d_out_a", give_a, oa, want.out_a, n, TAG), ("d_out_b", give_b, ob, want.out_b, m, TAG + (1 << 31))):
            if not given:
                assert o.unchanged(), (w, "%s was not given and changed" % name)
                continue
            got = o.host()
            expect = o.fill[o.off:].copy()
            at = np.fromiter(stores.at.keys(), np.int64, len(stores.at))
            expect[at] = np.array([v[0] for v in stores.at.values()], np.uint64)
            bad = got != expect
            assert not bad.any(), (w, name, int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), expect[bad][:4].tolist())
            if positions:
                assert ((got[at] >= first) & (got[at] < first + count)).all(), (w, name, "a word from outside the positions")
        unchanged(ins, w)
        guards(bufs, w)
    return P


def groups_case(ctx, a, b, kt, T, what, all_caps=True, pairs=True):
    n, m, kb = a.size, b.size, a.itemsize
    ca, cb = codes_of(a, b, kt)
    count = sum(X.count_np(ca, cb, T, X.INTERSECTION))
    room = count + TAIL
    da, db = Buf(kb, n, a=a), Buf(kb, m, a=b)
    outs = [Buf(kb, room)] + [Buf(8, room) for _ in range(4)]
    dnum = Buf(8, 1)
    bufs = [("d_a", da), ("d_b", db)] + list(zip(GJ.NAMES5, outs)) + [("d_num_groups", dnum)]
    columns = None
    for turn, (cap, _, _) in enumerate(reversed(caps_of(count)[:None if all_caps else 2])):      # (the call without a cap last: its groups feed the pairs)
        given = [True] * 5 if cap >= count else [(turn + k) % 2 == 0 for k in range(5)]
        w = (what, cap, given)
        for x in outs + [dnum]:
            x.reset()
        ctx._ok(GJ.raw_groups(ctx, da.ptr, n, db.ptr, m, kt, cap, *[g and o.ptr for g, o in zip(given, outs)], dnum.ptr))
        num = int(dnum.host()[0])
        assert num == count, (w, "*d_num_groups", num, count)
        stored = min(count, cap)
        got = [o.written(stored) if g else None for g, o in zip(given, outs)]                      # (nothing behind min(count, cap) changed)
        for name, g, o in zip(GJ.NAMES5, given, outs):
            assert g or o.unchanged(), (w, "%s was not given and changed" % name)
        keys, af, ac, bf, bc = got
        assert keys is None or np.isin(keys, a).all(), (w, "a key that A does not hold")
        # what include/msd_join_hip.h promises of the groups of inputs in any order
        assert ac is None or (ac >= 1).all(), (w, "a_count of 0")
        assert af is None or ac is None or ((af < n) & (ac <= n) & (af + ac <= n)).all(), (w, "a run of A beyond n")
        assert bf is None or bc is None or ((bf <= m) & (bc <= m) & (bf + bc <= m)).all(), (w, "a run of B beyond m")
        unchanged(bufs[:2], w)
        guards(bufs, w)
        if cap >= count:
            columns = [x.copy() for x in got[1:]]
    if pairs and count and n * m:
        P = PAIR_TH * PAIR_PER
        for positions in (False, True):
            pairs_case(ctx, columns, count, count, n, m, (P - 1, P, P + 1, 2 * P + 3) if positions else (P + 1, 0, 3 * P), positions, (what, "pairs"))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_groups_of_unsorted_inputs_and_their_pairs(ctx, kb, kind):
    """*d_num_groups is the clamped model's count, every stored group lies inside A and B; the pairs of those groups are the
    clamped model's, exactly"""
    T = tile_of(kb)
    for n, m in shapes(T):
        a, b, kt = inputs(kind, n, m, kb, T)
        groups_case(ctx, a, b, kt, T, (kind, E.NAMES[kt], n, m))
        sa, sb = S.sort_by_code(a, kt), S.sort_by_code(b, kt)
        gr = GJ.Groups(sa, sb, kt, what="sorted behind " + kind).run(ctx)
        cap = min(J.total(gr.want), 2 * PAIR_TH * PAIR_PER + 5)
        GJ.Pairs(gr.want, n, m, cap, what="sorted behind " + kind).run(ctx, cap)


@gpu
@pytest.mark.parametrize("kb", WIDTHS)
def test_groups_of_reversed_inputs_with_more_than_one_scan_piece(ctx, kb):
    a, b, T = reversed_over_a_scan_piece(kb)
    groups_case(ctx, a, b, UKT[kb], T, ("reversed, scan pieces", kb), all_caps=False, pairs=False)


@gpu
@pytest.mark.parametrize("positions", [False, True], ids=["indices", "positions"])
def test_pairs_of_made_up_groups(ctx, positions):
    """groups this library did not write: counts of 0 and up to 2^63 (the products wrap), firsts beyond n and m,
    *d_num_groups below and above groups_cap, caps around pair_tile"""
    import test_clamp_models as CM
    P = PAIR_TH * PAIR_PER
    rng = np.random.default_rng(11)
    for trial in range(8):
        n, m = (300, 200) if trial % 2 else (4 * P, 3)
        gcap = (150, 3, 1, 700)[trial % 4]
        stated = (gcap // 2, gcap, gcap + 3, 1 << 40, 0)[trial % 5]
        g = list(CM.made_up_groups(rng, gcap, n, m))
        if trial % 4 < 2:                                           # small products: a total around the caps
            g[1], g[3] = [x % 40 for x in g[1]], [x % 30 for x in g[3]]
        pairs_case(ctx, g, stated, gcap, n, m, (P - 1, P, P + 1, 3 * P + 1), positions, ("made up", trial))
    gr = GJ.Groups(np.arange(300, dtype=np.uint32) // 3, np.arange(200, dtype=np.uint32) // 2, E.U32, what="sorted behind made-up groups").run(ctx)
    GJ.Pairs(gr.want, 300, 200, 2 * P, pos=positions, what="sorted behind made-up groups").run(ctx, 2 * P)
