"""GPU tests of the sorted search (msd_search_sorted; MsdContext.searchsorted / bucketize): per needle the number of keys of a
sorted array that are smaller (left) or not larger (right) in the library's key order, by the direct path (any needles) and
by the merge path (ascending needles), straight or through positions, for the six key types.

The expected result is defined in tests/search_expect.py and every result is compared exactly.  The calls go through the C ABI
on integer tensors that carry the bit patterns, with EVERY buffer -- keys, needles, positions, d_out -- inside a
guardband.Arena whose payload is pre-filled with a known pattern: a case checks the m outputs, that no guard was touched, that
the inputs are what was uploaded and that the payload in front of an offset buffer is what it was.  The shapes are the smallest
at which a kernel can go wrong, taken from msd_search_sorted_limits (T = the merge tile, D = the direct tile).  Unsorted
needles under the merge path: test_gpu_untrusted_order.py.  The Python wrappers have tests of their own at the end."""
import ctypes as C

import numpy as np
import pytest

import search_expect as S
import sort_rows_expect as E
from gpu_support import DEFAULTS
from guardband import Buf
from sort_rows_expect import UKT, WIDTHS, special_bits, top, uniform

pytestmark = pytest.mark.gpu

DIRECT, MERGE = 1, 2                # values of the option search_mode


def limits(ctx, kb):
    tile, direct = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_search_sorted_limits(kb, C.byref(tile), C.byref(direct)) == 0
    return int(tile.value), int(direct.value)


def raw_call(ctx, sorted_ptr, kt, n, needles_ptr, m, needles_sorted, side, positions_ptr, out_ptr):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_search_sorted(ctx._h, vp(sorted_ptr), kt, n, vp(needles_ptr), m, needles_sorted, side, vp(positions_ptr), vp(out_ptr))


class Mode:
    """the option search_mode for the calls inside; the session's context gets its default back"""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        self.ctx.set_option("search_mode", self.mode)

    def __exit__(self, *exc):
        self.ctx.set_option("search_mode", DEFAULTS["search_mode"])


class Case:
    """keys and needles (unsigned bit patterns of key type kt) on the device, shared by the calls of the case"""

    def __init__(self, keys, needles, kt, positions=None, offs=(0, 0, 0, 0), what=""):
        self.keys, self.needles, self.kt, self.positions = keys, needles, kt, positions
        self.kb, self.n, self.m = keys.itemsize, keys.size, needles.size
        self.dkeys = Buf(self.kb, self.n, offs[0], a=keys)
        self.dneedles = Buf(self.kb, self.m, offs[1], a=needles)
        self.dpos = Buf(8, self.m, offs[2], a=positions.astype(np.uint64)) if positions is not None else None
        self.dout = Buf(8, self.m, offs[3])
        self.want = {right: S.expected(keys, needles, kt, right) for right in (False, True)}
        self.what = (what, E.NAMES[kt], self.n, self.m, offs, positions is not None)

    def run(self, ctx, mode, right, needles_sorted=None):
        """one call, everything checked; returns the m results in the order of the needles"""
        needles_sorted = (mode == MERGE) if needles_sorted is None else needles_sorted
        what = (self.what, "merge" if mode == MERGE else "direct", "right" if right else "left")
        self.dout.reset()
        with Mode(ctx, mode):
            ctx._ok(raw_call(ctx, self.dkeys.ptr, self.kt, self.n, self.dneedles.ptr, self.m, int(needles_sorted), int(right),
                             self.dpos and self.dpos.ptr, self.dout.ptr))
        got = self.dout.host()
        if self.positions is not None:
            got = got[self.positions]                                # d_out[positions[j]] = r_j
        bad = got != self.want[right]
        assert not bad.any(), (what, "results differ", int(bad.sum()), int(np.argmax(bad)), got[bad][:4].tolist(), self.want[right][bad][:4].tolist())
        assert self.dkeys.unchanged(), (what, "the keys changed")
        assert self.dneedles.unchanged(), (what, "the needles changed")
        if self.dpos is not None:
            assert self.dpos.unchanged(), (what, "the positions changed")
        for name, b in (("keys", self.dkeys), ("needles", self.dneedles), ("positions", self.dpos), ("d_out", self.dout)):
            if b is not None:
                b.check("%s of %s" % (name, what))
        return got


# ---- inputs, as codes of an unsigned type (code == bits)

def direct_inputs(kind, n, m, kb, seed):
    """keys (ascending) and UNSORTED needles: below the first key, above the last one, code 0 and code all-ones among them"""
    rng = np.random.default_rng(E.seed_of(n, m, kb, seed))
    ut = E.UW[kb]
    if kind == "distinct":
        keys = np.unique(uniform(rng, n + 64, kb, 1 << 8, top(kb) - (1 << 8)))[:n]
        assert keys.size == n
    elif kind == "five":
        keys = np.sort(np.array([1 << 8, 1 << 9, 77777, top(kb) >> 1, top(kb) - 999], ut)[rng.integers(0, 5, n)])
    else:                                                           # "equal": needles below, equal and above
        keys = np.full(n, 123456789, ut)
    first, last = (int(keys[0]), int(keys[-1])) if n else (1 << 8, 1 << 9)
    special = np.array([0, top(kb), first - 1, last + 1, first, last], ut)
    pool = np.r_[special, keys[rng.integers(0, n, m)] if n else special[:0], uniform(rng, m, kb), keys[rng.integers(0, n, m)] + ut(1) if n else special[:0]]
    needles = np.r_[special, rng.permutation(pool)][:m] if m >= special.size else rng.permutation(pool)[:m]
    return keys, rng.permutation(needles)


MERGE_KINDS = ["distinct", "five", "needles_equal", "above", "below", "keys_equal"]


def merge_inputs(kind, n, m, kb, seed):
    """keys and needles, both ascending"""
    rng = np.random.default_rng(E.seed_of(n, m, kb, seed, 7))
    ut = E.UW[kb]
    half = top(kb) >> 1
    five = np.array([0, 1 << 9, 77777, half, top(kb)], ut)
    if kind == "distinct":
        keys = np.sort(uniform(rng, n, kb))
        needles = np.r_[keys[rng.integers(0, n, m // 2)] if n else keys[:0], uniform(rng, m - (m // 2 if n else 0), kb)]
    elif kind == "five":                                            # ties lie across every tile edge
        keys, needles = five[rng.integers(0, 5, n)], five[rng.integers(0, 5, m)]
    elif kind == "needles_equal":                                   # all needles equal to one key value: tiles of needles only
        keys = five[rng.integers(0, 5, n)]
        needles = np.full(m, np.sort(keys)[n // 2] if n else 77777, ut)
    elif kind == "above":                                           # tiles of keys only first
        keys, needles = uniform(rng, n, kb, 0, half), uniform(rng, m, kb, half + 1)
    elif kind == "below":
        keys, needles = uniform(rng, n, kb, half + 1), uniform(rng, m, kb, 0, half)
    else:                                                           # "keys_equal"
        keys = np.full(n, 77777, ut)
        needles = np.array([0, 77776, 77777, 77777, 77778, top(kb)], ut)[rng.integers(0, 6, m)]
    return np.sort(keys), np.sort(needles)


# ---- direct

@pytest.mark.parametrize("kind", ["distinct", "five", "equal"])
@pytest.mark.parametrize("kb", WIDTHS)
def test_direct_sizes(ctx, kb, kind):
    """n at the trip-count edges of the search, m around the direct tile"""
    _, D = limits(ctx, kb)
    for n in (0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097):
        for m in (1, D - 1, D, D + 1, 3 * D + 7):
            keys, needles = direct_inputs(kind, n, m, kb, 1)
            if m >= 6:
                assert 0 in needles and top(kb) in needles
            case = Case(keys, needles, UKT[kb], what=kind)
            for right in (False, True):
                case.run(ctx, DIRECT, right)


def test_direct_runs_when_the_needles_are_not_promised_sorted_whatever_the_mode(ctx):
    """needles_sorted = 0 with search_mode 2 still runs direct: unsorted needles come out right"""
    for kb in WIDTHS:
        T, D = limits(ctx, kb)
        keys, needles = direct_inputs("distinct", 2 * T + 3, 3 * D + 7, kb, 2)
        assert (needles[1:] < needles[:-1]).any()
        case = Case(keys, needles, UKT[kb], what="unsorted, mode 2")
        for right in (False, True):
            case.run(ctx, MERGE, right, needles_sorted=False)


# ---- merge, and its agreement with direct

@pytest.mark.parametrize("kind", MERGE_KINDS)
@pytest.mark.parametrize("kb", WIDTHS)
def test_merge_sizes(ctx, kb, kind):
    """n and m around the merge tile; the direct path on the same buffers gives the same"""
    T, _ = limits(ctx, kb)
    sizes = [(n, m) for n in (0, 1, 2, T - 1, T, T + 1, 2 * T + 3) for m in (1, 2, T - 1, T, T + 1, 2 * T + 3)] + [(5 * T + 17, 3)]
    for n, m in sizes:
        keys, needles = merge_inputs(kind, n, m, kb, 3)
        case = Case(keys, needles, UKT[kb], what=kind)
        for right in (False, True):
            merged = case.run(ctx, MERGE, right)
            direct = case.run(ctx, DIRECT, right, needles_sorted=True)
            assert (merged == direct).all()


def test_the_merge_inputs_are_what_they_say():
    T = 64
    for kb in WIDTHS:
        for kind in MERGE_KINDS:
            keys, needles = merge_inputs(kind, 2 * T + 3, 2 * T + 3, kb, 3)
            assert (keys[1:] >= keys[:-1]).all() and (needles[1:] >= needles[:-1]).all() and keys.size == needles.size == 2 * T + 3
        keys, needles = merge_inputs("needles_equal", 2 * T + 3, 2 * T + 3, kb, 3)
        for right in (False, True):                                 # tiles of needles only, in the model of the decomposition
            a, b, got = S.splits(keys, needles, T, right)
            assert any(a[i + 1] == a[i] and b[i + 1] - b[i] == T for i in range(len(a) - 1))
            assert (got.astype(np.uint64) == S.expected(keys, needles, UKT[kb], right)).all()
        keys, needles = merge_inputs("above", 2 * T + 3, T, kb, 3)
        a, b, _ = S.splits(keys, needles, T, False)                 # tiles of keys only first
        assert b[1] == 0 and b[2] == 0 and a[2] == 2 * T
        keys, needles = merge_inputs("five", 5 * T, 5 * T, kb, 3)
        a, b, _ = S.splits(keys, needles, T, False)                 # ties across the tile edges
        assert any(0 < a[i] < keys.size and 0 < b[i] < needles.size and keys[a[i]] == needles[b[i] - 1] for i in range(1, len(a) - 1))


@pytest.mark.parametrize("kb", WIDTHS)
def test_both_paths_on_a_larger_case(ctx, kb):
    """the split kernel has more than one workgroup"""
    n, m = (1 << 21) + 5, (1 << 20) + 3
    T, _ = limits(ctx, kb)
    assert (n + m) // T + 1 > 256
    rng = np.random.default_rng(kb)
    keys = np.sort(uniform(rng, n, kb, 0, 1 << 22))                 # (about half of the needles find an equal key)
    needles = np.sort(uniform(rng, m, kb, 0, 1 << 22))
    case = Case(keys, needles, UKT[kb], what="larger")
    for right in (False, True):
        merged = case.run(ctx, MERGE, right)
        direct = case.run(ctx, DIRECT, right, needles_sorted=True)
        assert (merged == direct).all()


@pytest.mark.parametrize("kb", WIDTHS)
def test_buffers_off_the_16_byte_grid(ctx, kb):
    """keys, needles, positions and d_out 1, 2 and 3 elements behind a 16-byte boundary, in every combination of two"""
    T, D = limits(ctx, kb)
    turn = 0
    for koff in range(4):
        for noff in range(4):
            turn += 1
            for n, m in ((2 * T + 3, T + 1), (16 // kb - 1, 3), (T - koff, D + 1)):
                keys, needles = merge_inputs("distinct" if turn % 2 else "five", n, m, kb, turn)
                pos = np.random.default_rng(turn).permutation(m) if turn % 3 == 0 else None
                case = Case(keys, needles, UKT[kb], positions=pos, offs=(koff, noff, turn % 2, (turn // 2) % 2), what="off")
                for right in (False, True):
                    case.run(ctx, MERGE, right)
                    case.run(ctx, DIRECT, right)


# ---- all six key types

@pytest.mark.parametrize("kt", S.KEY_TYPES, ids=[E.NAMES[k] for k in S.KEY_TYPES])
def test_every_key_type_with_special_values(ctx, kt):
    ut = E.UT[kt]
    kb = np.dtype(ut).itemsize
    T, _ = limits(ctx, kb)
    rng = np.random.default_rng(kt)
    sp = special_bits(kt)

    def draw(count):
        x = uniform(rng, count, kb)
        at = rng.random(count) < 0.5
        x[at] = sp[rng.integers(0, sp.size, int(at.sum()))]
        return x

    keys = S.sort_by_code(draw(T + 1), kt)
    needles = draw(T + 1)
    needles[:sp.size] = sp                                          # every special is a needle
    unsorted, ascending = Case(keys, needles, kt, what="specials"), Case(keys, S.sort_by_code(needles, kt), kt, what="specials, ascending")
    for right in (False, True):
        unsorted.run(ctx, DIRECT, right)
        ascending.run(ctx, MERGE, right)
        ascending.run(ctx, DIRECT, right)
    if kt % 3 == 2:                                                 # the order is totalOrder: the zeros are told apart, the NaNs lie outside
        sign = ut(1 << (8 * kb - 1))
        z = Case(np.array([sign, sign, 0, 0, 0], ut), np.array([0, sign], ut), kt, what="zeros")
        assert z.run(ctx, DIRECT, False).tolist() == [2, 0] and z.run(ctx, DIRECT, True).tolist() == [5, 2]
        nan = sp[4]
        nn = Case(S.sort_by_code(np.array([nan | sign, nan, 0, 5, 9], ut), kt), S.sort_by_code(np.array([nan | sign, nan], ut), kt), kt, what="nans")
        for mode in (DIRECT, MERGE):
            assert nn.run(ctx, mode, False, needles_sorted=True).tolist() == [0, 4] and nn.run(ctx, mode, True, needles_sorted=True).tolist() == [1, 5]


# ---- positions

@pytest.mark.parametrize("kb", WIDTHS)
def test_results_through_positions(ctx, kb):
    T, D = limits(ctx, kb)
    for m in (T + 1, 3 * D + 7):
        keys, needles = merge_inputs("distinct", 2 * T + 3, m, kb, 5)
        pos = np.random.default_rng(m).permutation(m)
        case = Case(keys, needles, UKT[kb], positions=pos, what="positions")
        for right in (False, True):
            case.run(ctx, MERGE, right)
            case.run(ctx, DIRECT, right)


# ---- options and the phase

def test_the_modes_agree_and_bad_options_are_refused(ctx):
    from inplacemsdradixsort_amd import MsdError
    for kb in WIDTHS:
        T, D = limits(ctx, kb)
        for n, m in ((2 * T + 3, T + 1), (5 * T + 17, 3), (3, 3 * D + 7)):   # (the library's choice is merge, direct, merge)
            keys, needles = merge_inputs("five", n, m, kb, 6)
            case = Case(keys, needles, UKT[kb], what="modes")
            for right in (False, True):
                a, b, c = case.run(ctx, 0, right, needles_sorted=True), case.run(ctx, DIRECT, right, needles_sorted=True), case.run(ctx, MERGE, right)
                assert (a == b).all() and (b == c).all()
    try:
        for name, bad in (("search_mode", 3), ("search_mode", -1), ("search_merge_ratio", 0), ("search_merge_ratio", -5)):
            with pytest.raises(MsdError, match=name):
                ctx.set_option(name, bad)
        ctx.set_option("search_merge_ratio", 1)                     # the library's choice under another R: same results
        keys, needles = merge_inputs("distinct", 3 * 4096, 4096, 4, 8)
        case = Case(keys, needles, E.U32, what="R = 1")
        case.run(ctx, 0, False, needles_sorted=True)
        ctx.set_option("search_merge_ratio", 1 << 20)
        case.run(ctx, 0, True, needles_sorted=True)
    finally:
        ctx.set_option("search_mode", DEFAULTS["search_mode"])
        ctx.set_option("search_merge_ratio", DEFAULTS["search_merge_ratio"])


def test_the_phase_is_named(ctx):
    keys, needles = merge_inputs("distinct", 1000, 100, 4, 9)
    case = Case(keys, needles, E.U32, what="phase")
    ctx.set_profiling(True)
    try:
        for mode in (DIRECT, MERGE):
            case.run(ctx, mode, False, needles_sorted=True)
            assert [p[0] for p in ctx.phases()] == ["search_sorted"]
    finally:
        ctx.set_profiling(False)


# ---- degenerate sizes

def test_no_keys_and_no_needles(ctx):
    for kb in WIDTHS:
        for mode in (DIRECT, MERGE):
            empty = Case(np.zeros(0, E.UW[kb]), np.sort(uniform(np.random.default_rng(1), 1000, kb)), UKT[kb], what="n = 0")
            for right in (False, True):
                assert (empty.run(ctx, mode, right) == 0).all()
            none = Case(np.arange(100, dtype=E.UW[kb]), np.zeros(0, E.UW[kb]), UKT[kb], what="m = 0")
            none.run(ctx, mode, False)
        # null pointers where nothing is read or written
        dn, dout = Buf(kb, 5, a=np.arange(5, dtype=E.UW[kb])), Buf(8, 5)
        ctx._ok(raw_call(ctx, 0, UKT[kb], 0, dn.ptr, 5, 1, 0, 0, dout.ptr))
        assert (dout.host() == 0).all()
        dout.reset()
        ctx._ok(raw_call(ctx, 0, UKT[kb], 7, 0, 0, 0, 1, 0, 0))
        ctx._ok(raw_call(ctx, dn.ptr, UKT[kb], 5, 0, 0, 0, 1, 0, dout.ptr))
        assert dout.unchanged() and dn.unchanged()
        dn.check("m = 0")
        dout.check("m = 0")


# ---- refusals through the C ABI

def test_refusals_in_order_touch_nothing(ctx):
    n, m = 1000, 300
    for kb in WIDTHS:
        for kt in (UKT[kb], UKT[kb] + 2):
            keys, needles = merge_inputs("distinct", n, m, kb, 4)
            keys, needles = S.sort_by_code(keys, kt), S.sort_by_code(needles, kt)
            dk, dn, dpos, dout = Buf(kb, n, a=keys), Buf(kb, m, a=needles), Buf(8, m, a=np.arange(m, dtype=np.uint64)), Buf(8, m)
            bufs = (dk, dn, dpos, dout)
            good = dict(keys=dk.ptr, kt=kt, n=n, needles=dn.ptr, m=m, ns=1, side=0, positions=dpos.ptr, out=dout.ptr)
            order = ("keys", "kt", "n", "needles", "m", "ns", "side", "positions", "out")

            def refused(message, **change):
                k = dict(good, **change)
                rc = raw_call(ctx, *[k[a] for a in order])
                err = ctx._L.msd_last_error(ctx._h).decode()
                assert rc == -1 and message in err, (change, rc, err)
                for b in bufs:
                    assert b.unchanged(), change
                    b.check(str(change))

            # every refusal on its own, in the header's order
            for bad in (-1, 6, 7, 100):
                refused("key_type", kt=bad)
            for bad in (-1, 2, 100):
                refused("side", side=bad)
                refused("needles_sorted", ns=bad)
            refused("null d_out", out=0)
            refused("null d_needles", needles=0)
            refused("null d_sorted", keys=0)
            for name, es in (("keys", kb), ("needles", kb), ("positions", 8), ("out", 8)):
                for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                    refused("aligned", **{name: good[name] + d})
            for big in (1 << 36, (1 << 64) - 1):
                refused("2^36", n=big)
                refused("2^36", m=big)
            refused("overlap d_sorted", out=dk.ptr)
            refused("overlap d_sorted", out=dk.ptr + (n * kb - 8))
            refused("overlap d_sorted", keys=dout.ptr + 8 * (m - 1))
            refused("overlap d_sorted", out=dn.ptr)
            refused("overlap d_sorted", out=dn.ptr + (m * kb - 8))
            refused("overlap d_sorted", out=dpos.ptr + 8 * (m - 1))
            refused("overlap d_sorted", positions=dout.ptr + 8 * (m - 1))
            # the order: of two faults the earlier one is reported
            refused("key_type", kt=9, side=5)
            refused("side", side=5, ns=5)
            refused("needles_sorted", ns=5, out=0)
            refused("null d_out", out=0, needles=0)
            refused("null d_needles", needles=0, keys=0)
            refused("null d_sorted", keys=0, positions=dpos.ptr + 4)
            refused("aligned", positions=dpos.ptr + 4, n=1 << 36)
            refused("2^36", m=1 << 36, out=dk.ptr)
            # and the call that all of these were changes of is fine
            ctx._ok(raw_call(ctx, *[good[a] for a in order]))
            assert (dout.host() == S.expected(keys, needles, kt, False)).all()
            for b in bufs:
                b.check("good")


# ---- the Python wrappers

def test_searchsorted_is_torch_searchsorted_where_the_orders_agree(ctx):
    import torch
    g = torch.Generator(device="cpu").manual_seed(1)
    for dt in (torch.int32, torch.int64, torch.float32):
        if dt.is_floating_point:
            keys = torch.randn(5000, generator=g).to(dt)
            needles = torch.cat([keys[torch.randint(0, 5000, (1500,), generator=g)], torch.randn(1500, generator=g).to(dt)]).reshape(3, 1000)
            keys[keys == 0] = 1.0                                   # (no zeros of two signs, no NaNs: the two orders agree)
            needles[needles == 0] = 1.0
        else:
            keys = torch.randint(-3000, 3000, (5000,), generator=g).to(dt)
            needles = torch.randint(-3100, 3100, (3, 1000), generator=g).to(dt)
        s = keys.cuda()
        ctx.sort_typed(s)
        x = needles.cuda()
        before = (s.clone(), x.clone())
        for right in (False, True):
            want = torch.searchsorted(s, x, right=right)
            got = ctx.searchsorted(s, x, right=right)
            assert got.dtype == torch.int64 and got.shape == x.shape and torch.equal(got, want)
            assert torch.equal(ctx.searchsorted(s, x, right=right, sort_needles=True), want)
            xs = x.reshape(-1).clone()
            ctx.sort_typed(xs)
            assert torch.equal(ctx.searchsorted(s, xs, right=right, needles_sorted=True), torch.searchsorted(s, xs, right=right))
        assert torch.equal(s, before[0]) and torch.equal(x, before[1])   # the inputs are what they were


def test_sort_needles_equals_the_default_and_keeps_the_shape(ctx):
    import torch
    for dt in (torch.float32, torch.float64, torch.int32, torch.int64):
        g = torch.Generator(device="cpu").manual_seed(2)
        s = (torch.randn(4000, generator=g) * 100).to(dt).cuda()
        ctx.sort_typed(s)
        x = s[torch.randperm(2100, generator=g).cuda()].reshape(7, 300).contiguous()
        for right in (False, True):
            a, b = ctx.searchsorted(s, x, right=right), ctx.searchsorted(s, x, right=right, sort_needles=True)
            assert a.shape == b.shape == (7, 300) and torch.equal(a, b)
    assert ctx.searchsorted(s, s[:0]).shape == (0,) and ctx.searchsorted(s, s[:0].reshape(0, 3), sort_needles=True).shape == (0, 3)


def test_bucketize_is_torch_bucketize(ctx):
    import torch
    g = torch.Generator(device="cpu").manual_seed(3)
    edges = torch.sort(torch.randn(257, generator=g)).values.cuda()
    v = torch.cat([torch.randn(10000, generator=g), edges.cpu()[::3]]).cuda().reshape(-1, 2)
    for right in (False, True):
        got = ctx.bucketize(v, edges, right=right)
        assert got.shape == v.shape and torch.equal(got, torch.bucketize(v, edges, right=right))


def test_the_lookup_of_keys_in_the_distinct_keys_of_a_group_reduce(ctx):
    import torch
    g = torch.Generator(device="cpu").manual_seed(4)
    for dt in (torch.int32, torch.int64, torch.float32, torch.float64):
        keys = torch.randint(-500, 500, (100003,), generator=g).to(dt).cuda()
        v = torch.ones(100003, device="cuda")
        vals, sums = ctx.group_reduce(keys, v)
        at = ctx.searchsorted(vals, keys)
        assert int(at.max().item()) < vals.numel() and torch.equal(vals[at], keys)
        count = ctx.searchsorted(vals, keys, right=True) - at       # every key is there exactly once ...
        assert (count == 1).all()
        assert torch.equal(sums[at], torch.bincount((keys.long() + 500))[keys.long() + 500].double())   # ... and finds its group's sum


def test_out_and_positions_are_honoured(ctx):
    import torch
    s = torch.arange(0, 2000, 2, dtype=torch.int32, device="cuda")
    x = torch.randint(-5, 2005, (5, 100), dtype=torch.int32, device="cuda")
    out = torch.full((5, 100), -7, dtype=torch.int64, device="cuda")
    r = ctx.searchsorted(s, x, out=out)
    assert r is out and torch.equal(out, torch.searchsorted(s, x))
    xs, pos = ctx.sort_rows(x.reshape(-1), indices=True)
    r2 = ctx.searchsorted(s, xs, right=True, needles_sorted=True, positions=pos)
    assert r2.shape == (500,) and torch.equal(r2.reshape(5, 100), torch.searchsorted(s, x, right=True))
    assert ctx.search_sorted_limits(4) == limits(ctx, 4) and ctx.search_sorted_limits(8) == limits(ctx, 8)
