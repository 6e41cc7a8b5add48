"""GPU tests of stream compaction and stable partition (msd_compact; MsdContext.compact / masked_select / nonzero /
filter_range): the kept keys, values and positions in their original order, the rejected ones behind them with
MSD_COMPACT_REST, and the true count, for every key type, masks and typed ranges.

The expected result is defined in tests/compact_expect.py; everything is compared BITWISE, all elements.  The calls go
through the C ABI on integer tensors that carry the bit patterns, with EVERY buffer -- keys, mask (1-byte cells), values,
each output and the count word -- inside a guardband.Arena whose payload is pre-filled with a known pattern: a case checks
what was written, that the rest of each payload is what it was, that no guard was touched and that the inputs are what was
uploaded.  The Python wrappers have tests of their own at the end."""
import ctypes as C
import itertools

import numpy as np
import pytest

import compact_expect as X
import guardband
import runs_expect as R
import sort_rows_expect as E
from guardband import Buf

pytestmark = pytest.mark.gpu

WIDTHS, UKT = E.WIDTHS, E.UKT
KEY_TYPES = [E.U32, E.I32, E.F32, E.U64, E.I64, E.F64]
PAGE = guardband.PAGE


def limits(ctx, es):
    tile, scan_tile = C.c_uint64(), C.c_uint64()
    assert ctx._L.msd_compact_limits(es, C.byref(tile), C.byref(scan_tile)) == 0
    return int(tile.value), int(scan_tile.value)


def at_page_start(es, n):
    return dict(off=0, lead_bytes=0)


def at_page_end(es, n):
    """the buffer's last element is the last element of a page"""
    start = (-n * es) % PAGE
    return dict(off=(start % 16) // es, lead_bytes=start - start % 16)


def raw_call(ctx, keys, kt, n, mask, lo, hi, flags, vals, vb, cap, okeys, ovals, oidx, count):
    vp = lambda p: C.c_void_p(p) if p else None
    return ctx._L.msd_compact(ctx._h, vp(keys), kt, n, vp(mask), lo, hi, flags, vp(vals), vb, cap, vp(okeys), vp(ovals), vp(oidx), vp(count))


def run_case(ctx, n, keys=None, kt=0, mask=None, lo=None, hi=None, invert=False, rest=False, vals=None, want_keys=True, want_idx=True, cap=None,
             place=None, what=""):
    """one call, everything checked.  keys / vals: unsigned arrays of bit patterns, mask: uint8; lo / hi: bit patterns (both or
    neither).  place: name -> dict(off=, lead_bytes=) for "keys", "mask", "vals", "okeys", "ovals", "oidx", "count".  Returns
    (m, kept keys, kept values, indices) as read back."""
    place = place or {}
    want_keys = want_keys and keys is not None
    cap = n if cap is None else cap
    es = keys.itemsize if keys is not None else 4
    vb = vals.itemsize if vals is not None else 0
    what = (what, n, es, kt, mask is not None, lo, hi, invert, rest, vb, want_keys, want_idx, cap, place)
    room = n if rest else min(cap, n + 3)                                   # (a little more than can be written)
    dkeys = Buf(es, n, a=keys, **place.get("keys", {})) if keys is not None else None
    dmask = Buf(1, n, a=mask, **place.get("mask", {})) if mask is not None else None
    dvals = Buf(vb, n, a=vals, **place.get("vals", {})) if vals is not None else None
    dok = Buf(es, room, **place.get("okeys", {})) if want_keys else None
    dov = Buf(vb, room, **place.get("ovals", {})) if vals is not None else None
    doi = Buf(8, room, **place.get("oidx", {})) if want_idx else None
    dcount = Buf(8, 1, **place.get("count", {}))
    flags = (X.RANGE if lo is not None else 0) | (X.INVERT if invert else 0) | (X.REST if rest else 0)
    rc = raw_call(ctx, dkeys and dkeys.ptr, kt, n, dmask and dmask.ptr, lo or 0, hi or 0, flags, dvals and dvals.ptr, vb, cap, dok and dok.ptr, dov and dov.ptr,
                  doi and doi.ptr, dcount.ptr)
    ctx._ok(rc)
    k = X.keep(n, keys, kt, mask, lo, hi, invert)
    m, ek, ev, ei = X.expected(k, keys, vals, rest=rest, cap=cap)
    w = ei.size                                                             # elements written: min(m, cap), n with rest
    assert w == (n if rest else min(m, cap))
    got = int(dcount.host()[0])
    assert got == m, (what, "count", got, m)
    out = [m, None, None, None]
    for i, (b, e, name) in enumerate(((dok, ek, "keys"), (dov, ev, "values"), (doi, ei, "indices")), 1):
        if b is None:
            continue
        h = b.host()
        e = e.view(E.UW[e.itemsize])
        assert (h[:w] == e).all(), (what, name + " differ", int(np.argmax(h[:w] != e)))
        assert b.untouched_from(w), (what, name + " written beyond what the call may write")
        out[i] = h[:w]
    for name, b in (("keys", dkeys), ("mask", dmask), ("values", dvals)):
        if b is not None:
            assert b.unchanged(), (what, "the input %s changed" % name)
    for name, b in (("keys", dkeys), ("mask", dmask), ("values", dvals), ("out keys", dok), ("out values", dov), ("out indices", doi), ("count", dcount)):
        if b is not None:
            b.check("%s of %s" % (name, what))
    return out


# ---- sizes x keep patterns x (mask | range), both widths

def _size_pattern_cases():
    for es in WIDTHS:
        for size in R.SIZE_NAMES:
            for p in (X.BIG_PATTERNS if size == "big" else X.PATTERNS):
                yield es, size, p


@pytest.mark.parametrize("es,size,pattern", list(_size_pattern_cases()))
def test_sizes_and_patterns(ctx, es, size, pattern):
    tile, scan_tile = limits(ctx, es)
    n = R.sizes(tile, scan_tile)[size]
    k = X.pattern(pattern, n, tile, seed=E.seed_of(es, n))
    vals = X.values_for(n, 12 - es)                                          # 8-byte values beside 4-byte keys and the reverse
    m1 = run_case(ctx, n, R.distinct(n, es, seed=7), UKT[es], mask=X.mask_of(k), vals=vals, what=pattern)[0]
    keys, lo, hi = X.keys_for_range(k, es)
    m2 = run_case(ctx, n, keys, UKT[es], lo=lo, hi=hi, vals=vals, what=pattern)[0]
    assert m1 == m2 == int(k.sum())


# ---- typed ranges

def _typed_keys(kt, n):
    """random keys of the type with the specials planted, and the planted values by name"""
    ut = E.UT[kt]
    W = 8 * np.dtype(ut).itemsize
    rng = np.random.default_rng(E.seed_of(kt, n))
    if kt % 3 == 2:
        ft = np.float32 if W == 32 else np.float64
        S = X.float_specials(ft)
        bits = rng.standard_normal(n).astype(ft).view(ut).copy()
        bits[rng.random(n) < 0.02] |= ut(0x7F800000 if W == 32 else 0x7FF << 52)   # infinities and NaNs of any payload, both signs
    else:
        top = 1 << (W - 1)
        S = {"min": top if kt % 3 == 1 else 0, "max": top - 1 if kt % 3 == 1 else (1 << W) - 1, "0": 0, "-1": (1 << W) - 1, "1": 1, "top": top, "top-1": top - 1}
        bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(ut) if W == 32 else rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
        bits[rng.random(n) < 0.3] &= ut(0xFFFF)
    planted = np.array(list(S.values()), dtype=ut)
    at = 1 + rng.choice(n - 2, size=8 * planted.size, replace=False)      # (not the two ends, which are planted last)
    bits[at] = np.tile(planted, 8)
    bits[[0, n - 1]] = planted[:2]
    return bits, S


@pytest.mark.parametrize("which", ["T+1", "3T-1"])
@pytest.mark.parametrize("kt", KEY_TYPES, ids=[E.NAMES[k] for k in KEY_TYPES])
def test_typed_ranges_with_planted_specials(ctx, kt, which):
    ut = E.UT[kt]
    es = np.dtype(ut).itemsize
    W = 8 * es
    tile, _ = limits(ctx, es)
    n = tile + 1 if which == "T+1" else 3 * tile - 1
    keys, S = _typed_keys(kt, n)
    full = tuple(int(x) for x in E.np_decode(np.array([0, (1 << W) - 1], dtype=ut), kt))
    if kt % 3 == 2:
        bounds = [full, (S["-den"], S["-den"]), (S["+inf"], S["-inf"]), (S["-0"], S["-0"]), (S["+0"], S["+inf"]), (S["+inf"], S["+nanmax"]),
                  (S["-0"], S["+0"]), (S["-nanmax"], S["-inf"]), (S["-inf"], S["+inf"])]
    else:
        bounds = [full, (S["-1"], S["-1"]), (S["1"], S["0"]), (S["0"], S["0"]), (S["0"], S["max"]), (S["min"], S["0"]), (S["top-1"], S["top-1"]),
                  (S["top"], S["top"])]
        if kt % 3 == 1:
            bounds += [(S["-1"], S["1"]), (S["min"], S["-1"])]               # across zero; the negatives
    seen = []
    for lo, hi in bounds:
        m = run_case(ctx, n, keys, kt, lo=lo, hi=hi, what="typed")[0]
        mi = run_case(ctx, n, keys, kt, lo=lo, hi=hi, invert=True, what="typed inverted")[0]
        assert m + mi == n
        seen.append(m)
    assert seen[0] == n and seen[2] == 0 and all(m >= 8 for m in seen[:2] + seen[3:])   # the full range; lo > hi; the planted values are found
    if kt % 3 == 2:
        assert seen[3] == 8                                                             # [-0.0, -0.0] is the -0.0s alone
    if es == 4:
        dk, dc = Buf(4, n, a=keys), Buf(8, 1)
        for lo, hi in ((1 << 32, 5), (5, 1 << 32), (1 << 63, 1 << 63)):
            assert raw_call(ctx, dk.ptr, kt, n, 0, lo, hi, X.RANGE, 0, 0, n, 0, 0, 0, dc.ptr) == -1
            assert "2^32" in ctx._L.msd_last_error(ctx._h).decode()
        ctx._ok(raw_call(ctx, dk.ptr, kt, n, 0, 1 << 32, 5, 0, 0, 0, n, 0, 0, 0, dc.ptr))   # (without MSD_COMPACT_RANGE the bounds are not looked at)
        assert int(dc.host()[0]) == n
        dc.check("count")


# ---- outputs, capacity

@pytest.mark.parametrize("es", WIDTHS)
def test_outputs_in_every_combination(ctx, es):
    tile, _ = limits(ctx, es)
    n = 2 * tile + 1
    k = X.pattern("rand50", n, tile, seed=5)
    keys, lo, hi = X.keys_for_range(k, es)
    mask = X.mask_of(k)
    for want_keys, vb, want_idx in itertools.product((False, True), (0, 4, 8), (False, True)):
        vals = X.values_for(n, vb) if vb else None
        kw = dict(vals=vals, want_keys=want_keys, want_idx=want_idx, what="outputs")
        run_case(ctx, n, keys, UKT[es], mask=mask, **kw)
        run_case(ctx, n, keys, UKT[es], lo=lo, hi=hi, **kw)
        run_case(ctx, n, keys, UKT[es], mask=mask, rest=True, **kw)
        run_case(ctx, n, keys, UKT[es], lo=lo, hi=hi, cap=7, **kw)


@pytest.mark.parametrize("pattern", ["rand50", "rand1", "all"])
@pytest.mark.parametrize("es", WIDTHS)
def test_capacity(ctx, es, pattern):
    tile, _ = limits(ctx, es)
    n = 2 * tile + 1
    k = X.pattern(pattern, n, tile, seed=6)
    m = int(k.sum())
    keys, lo, hi = X.keys_for_range(k, es)
    vals = X.values_for(n, 8)
    for cap in sorted({0, m - 1, m, m + 1, n}):
        assert run_case(ctx, n, keys, UKT[es], mask=X.mask_of(k), vals=vals, cap=cap, what="cap")[0] == m
        assert run_case(ctx, n, keys, UKT[es], lo=lo, hi=hi, cap=cap, what="cap")[0] == m
    assert run_case(ctx, n, keys, UKT[es], lo=lo, hi=hi, cap=(1 << 64) - 1, what="huge cap")[0] == m   # (a cap beyond n claims no more memory)


# ---- stable partition

@pytest.mark.parametrize("pattern", ["rand50", "all", "none"])
@pytest.mark.parametrize("size", R.SIZE_NAMES)
@pytest.mark.parametrize("es", WIDTHS)
def test_rest_is_a_stable_partition(ctx, es, size, pattern):
    tile, scan_tile = limits(ctx, es)
    n = R.sizes(tile, scan_tile)[size]
    k = X.pattern(pattern, n, tile, seed=8)
    keys, lo, hi = X.keys_for_range(k, es)
    vals = X.values_for(n, 4 if pattern == "rand50" else 8)
    m, ok, ov, oi = run_case(ctx, n, keys, UKT[es], mask=X.mask_of(k), vals=vals, rest=True, what="rest")
    oi = oi.view(np.int64)
    assert (np.sort(oi) == np.arange(n)).all() and (oi == np.argsort(~k, kind="stable")).all()
    assert k[oi[:m]].all() and not k[oi[m:]].any() and (np.diff(oi[:m]) > 0).all() and (np.diff(oi[m:]) > 0).all()
    run_case(ctx, n, keys, UKT[es], lo=lo, hi=hi, rest=True, cap=n + 5, what="rest")
    if n and pattern == "rand50":
        dk, dok, dc = Buf(es, n, a=keys), Buf(es, n), Buf(8, 1)
        assert raw_call(ctx, dk.ptr, UKT[es], n, 0, 0, 0, X.REST, 0, 0, n - 1, dok.ptr, 0, 0, dc.ptr) == -1
        assert "cap >= n" in ctx._L.msd_last_error(ctx._h).decode()
        assert dok.unchanged() and dc.unchanged()


# ---- both predicates at once

@pytest.mark.parametrize("es", WIDTHS)
def test_mask_and_range_together(ctx, es):
    tile, _ = limits(ctx, es)
    n = 3 * tile - 1
    keys, lo, hi = X.keys_for_range(X.pattern("rand50", n, tile, seed=9), es)
    mask = X.mask_of(X.pattern("rand50", n, tile, seed=10))
    vals = X.values_for(n, 8)
    counts = [run_case(ctx, n, keys, UKT[es], mask=mask, lo=lo, hi=hi, invert=inv, rest=rest, vals=vals, what="both")[0] for inv in (False, True) for rest in (False, True)]
    assert counts[0] == counts[1] and counts[2] == counts[3] and counts[0] + counts[2] == n and n // 8 < counts[0] < n // 2


# ---- the mask-only form

@pytest.mark.parametrize("size", R.SIZE_NAMES)
def test_mask_only_is_nonzero(ctx, size):
    tile, scan_tile = limits(ctx, 4)
    n = R.sizes(tile, scan_tile)[size]
    for pattern in ("rand50", "rand1", "tile_last"):
        mask = X.mask_of(X.pattern(pattern, n, tile, seed=11))
        m, _, _, oi = run_case(ctx, n, mask=mask, kt=99, what="nonzero")     # (without keys the key type is not looked at)
        assert (oi.view(np.int64) == np.flatnonzero(mask)).all()
    run_case(ctx, n, mask=X.mask_of(X.pattern("rand50", n, tile, seed=12)), invert=True, vals=X.values_for(n, 8), rest=True, what="mask and values")
    run_case(ctx, n, mask=X.mask_of(X.pattern("rand99", n, tile, seed=13)), want_idx=False, what="mask, count only")


# ---- alignment

def _alignment_inputs(ctx, es):
    tile, _ = limits(ctx, es)
    full = 2 * tile + 1
    keys_full, lo, hi = X.keys_for_range(X.pattern("rand50", full, tile, seed=14), es)
    mask_full = X.mask_of(X.pattern("rand50", full, tile, seed=15))
    return tile, keys_full, lo, hi, mask_full, X.values_for(full, 4), X.values_for(full, 8)


ALIGN_SIZES = lambda tile: (1, 2, 3, 65, tile - 1, tile, tile + 1, 2 * tile + 1)
MASK_OFFS = (1, 2, 3, 5, 15)


@pytest.mark.parametrize("es,koff", [(4, 1), (4, 2), (4, 3), (8, 1)])
def test_alignment_of_every_buffer(ctx, es, koff):
    """keys 4, 8, 12 bytes (4-byte keys) / 8 bytes (8-byte keys) off the 16-byte grid, the mask at odd bytes, values and
    outputs at other phases"""
    tile, keys_full, lo, hi, mask_full, v4, v8 = _alignment_inputs(ctx, es)
    per16 = 16 // es
    for i, moff in enumerate(MASK_OFFS):
        for n in ALIGN_SIZES(tile):
            vals = (v4, v8)[(i + n) % 2][:n]
            place = dict(keys=dict(off=koff), mask=dict(off=moff), vals=dict(off=(i + 1) % 4), okeys=dict(off=(koff + 1) % per16), ovals=dict(off=(i + 2) % 3),
                         oidx=dict(off=i % 2), count=dict(off=(i + 1) % 2))
            run_case(ctx, n, keys_full[:n], UKT[es], mask=mask_full[:n], lo=lo, hi=hi, vals=vals, rest=bool(n % 2), place=place, what="off")


@pytest.mark.parametrize("moff", MASK_OFFS)
@pytest.mark.parametrize("es", WIDTHS)
def test_alignment_of_the_mask_alone(ctx, es, moff):
    """the mask-only form, whose grid is the mask's, and a mask off the grid of aligned keys"""
    tile, keys_full, lo, hi, mask_full, v4, v8 = _alignment_inputs(ctx, es)
    for n in ALIGN_SIZES(tile):
        if es == 4:
            run_case(ctx, n, mask=mask_full[:n], vals=v8[:n], place=dict(mask=dict(off=moff), vals=dict(off=1)), what="mask off")
        run_case(ctx, n, keys_full[:n], UKT[es], mask=mask_full[:n], vals=v4[:n], place=dict(mask=dict(off=moff)), what="aligned keys, mask off")


@pytest.mark.parametrize("where", [at_page_start, at_page_end], ids=["start", "end"])
@pytest.mark.parametrize("es", WIDTHS)
def test_buffers_at_the_edges_of_pages(ctx, es, where):
    """every buffer begins at the first element of a page; every buffer ends at the last element of a page"""
    tile, keys_full, lo, hi, mask_full, v4, v8 = _alignment_inputs(ctx, es)
    for n in (1, 3, 65, tile - 1, tile + 1, PAGE // es, PAGE + 1):
        for rest in (False, True):
            w = n if rest else int(X.keep(n, keys_full[:n], UKT[es], mask_full[:n], lo, hi).sum())
            place = dict(keys=where(es, n), mask=where(1, n), vals=where(8, n), okeys=where(es, w), ovals=where(8, w), oidx=where(8, w), count=where(8, 1))
            run_case(ctx, n, keys_full[:n], UKT[es], mask=mask_full[:n], lo=lo, hi=hi, vals=v8[:n], rest=rest, cap=w, place=place, what=where.__name__)
            run_case(ctx, n, mask=mask_full[:n], cap=n, place=dict(mask=where(1, n), oidx=where(8, int((mask_full[:n] != 0).sum()))), what="mask " + where.__name__)


# ---- refusals through the C ABI

ARGS = ("keys", "kt", "n", "mask", "lo", "hi", "flags", "vals", "vb", "cap", "okeys", "ovals", "oidx", "count")


def test_refusals_touch_nothing_and_come_in_the_stated_order(ctx):
    n = 1000
    for es in WIDTHS:
        k = X.pattern("rand50", n, 64, seed=16)
        keys, lo, hi = X.keys_for_range(k, es)
        dkeys, dmask, dvals = Buf(es, n, a=keys), Buf(1, n, a=X.mask_of(k)), Buf(8, n, a=X.values_for(n, 8))
        dok, dov, doi, dcount = Buf(es, n), Buf(8, n), Buf(8, n), Buf(8, 1)
        bufs = (dkeys, dmask, dvals, dok, dov, doi, dcount)
        good = dict(keys=dkeys.ptr, kt=UKT[es], n=n, mask=dmask.ptr, lo=lo, hi=hi, flags=X.RANGE, vals=dvals.ptr, vb=8, cap=n, okeys=dok.ptr, ovals=dov.ptr,
                    oidx=doi.ptr, count=dcount.ptr)

        def refused(message, **change):
            kw = dict(good, **change)
            rc = raw_call(ctx, *[kw[a] for a in ARGS])
            err = ctx._L.msd_last_error(ctx._h).decode()
            assert rc == -1 and message in err, (change, rc, err)
            for b in bufs:
                assert b.unchanged(), change
                b.check(str(change))

        # the refusals in the order of the header: each alone, and each together with the one that comes after it
        ladder = [("unknown key_type", dict(kt=6)),
                  ("unknown flags", dict(flags=8 | X.RANGE)),
                  ("d_count is required", dict(count=0)),
                  ("without d_keys", dict(keys=0)),
                  ("2^32", dict(lo=1 << 32)) if es == 4 else None,
                  ("go together", dict(vals=0)),
                  ("val_bytes", dict(vb=3)),
                  ("nothing to take", dict(keys=0, mask=0, flags=0, okeys=0)),
                  ("aligned", dict(oidx=doi.ptr + 4)),
                  ("2^36", dict(n=1 << 36)),
                  ("cap >= n", dict(flags=X.RANGE | X.REST, cap=n - 1)),
                  ("overlap", dict(ovals=dvals.ptr))]
        ladder = [r for r in ladder if r]
        for i, (message, change) in enumerate(ladder):
            refused(message, **change)
            if i + 1 < len(ladder):
                refused(message, **dict(ladder[i + 1][1], **change))
        # more of each kind
        for bad in (-1, 7, 99):
            refused("unknown key_type", kt=bad)
        for bad in (8, 16, -1, 1 << 30):
            refused("unknown flags", flags=bad)
        refused("without d_keys", keys=0, flags=0)                           # d_out_keys alone asks for them
        refused("go together", ovals=0)
        for bad in (0, 1, 2, 16, -8):
            refused("val_bytes", vb=bad)
        refused("nothing to take", keys=0, mask=0, flags=0, okeys=0, oidx=0)
        for name in ("keys", "okeys"):
            for d in ((1, 2, 3) if es == 4 else (1, 2, 4, 7)):
                refused("aligned", **{name: good[name] + d})
        for name in ("vals", "ovals", "oidx", "count"):
            for d in (1, 4):
                refused("aligned", **{name: good[name] + d})
        refused("aligned", vals=dvals.ptr + 2, vb=4)
        refused("2^36", n=(1 << 64) - 1)
        refused("cap >= n", flags=X.REST, cap=0)
        # every output against every input and the other outputs
        refused("overlap", okeys=dkeys.ptr)
        refused("overlap", okeys=dkeys.ptr + (n - 1) * es)
        refused("overlap", okeys=dmask.ptr + 16)
        refused("overlap", oidx=dmask.ptr + 992)
        refused("overlap", okeys=dvals.ptr + 8 * (n - 1))
        refused("overlap", ovals=dkeys.ptr)
        refused("overlap", oidx=dvals.ptr)
        refused("overlap", count=dkeys.ptr)
        refused("overlap", count=dmask.ptr + 8)
        refused("overlap", count=dvals.ptr + 8 * (n - 1))
        refused("overlap", ovals=dok.ptr)
        refused("overlap", oidx=dok.ptr)
        refused("overlap", oidx=dov.ptr + 8 * (n - 1))
        refused("overlap", count=dok.ptr)
        refused("overlap", count=dov.ptr + 8)
        refused("overlap", count=doi.ptr + 8 * (n - 1))
        # a cap bounds the extents: outputs of cap elements may lie closer than n
        ctx._ok(raw_call(ctx, *[dict(good, cap=10, ovals=dok.ptr + 16 * es)[a] for a in ARGS]))
        # and the call that all of these were changes of is fine
        for b in (dok, dov, doi):
            b.arena.fill(b.fill)
        ctx._ok(raw_call(ctx, *[good[a] for a in ARGS]))
        m, ek, ev, ei = X.expected(X.keep(n, keys, UKT[es], dmask.fill, lo, hi), keys, dvals.fill)
        assert int(dcount.host()[0]) == m and (dok.host()[:m] == ek).all() and (dov.host()[:m] == ev).all() and (doi.host()[:m].view(np.int64) == ei).all()
        # 64-bit bounds use all their bits
        if es == 8:
            ctx._ok(raw_call(ctx, *[dict(good, lo=1 << 40, hi=(1 << 64) - 1)[a] for a in ARGS]))


def test_the_legal_corners(ctx):
    for es in WIDTHS:
        tile, _ = limits(ctx, es)
        n = tile + 5
        keys = R.distinct(n, es, seed=3)
        # n == 0: the count is written, nothing else; null inputs are fine
        for kw in (dict(), dict(rest=True), dict(mask=np.zeros(0, np.uint8)), dict(lo=1, hi=2)):
            assert run_case(ctx, 0, keys[:0], UKT[es], vals=X.values_for(0, 8), what="empty", **kw)[0] == 0
        dc, doi = Buf(8, 1), Buf(8, 4)
        ctx._ok(raw_call(ctx, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, doi.ptr, dc.ptr))
        assert int(dc.host()[0]) == 0 and doi.unchanged()
        # no predicate keeps everything, inverted nothing
        assert run_case(ctx, n, keys, UKT[es], vals=X.values_for(n, 4), what="no predicate")[0] == n
        assert run_case(ctx, n, keys, UKT[es], invert=True, what="no predicate")[0] == 0
        assert run_case(ctx, n, keys, UKT[es], invert=True, rest=True, what="no predicate")[0] == 0
        # neither keys nor a mask: the positions alone stand
        dc, doi = Buf(8, 1), Buf(8, n)
        ctx._ok(raw_call(ctx, 0, 0, n, 0, 0, 0, 0, 0, 0, n, 0, 0, doi.ptr, dc.ptr))
        assert int(dc.host()[0]) == n and (doi.host() == np.arange(n)).all()
        # count only, and cap == 0
        k = X.pattern("rand50", n, tile, seed=17)
        kr, lo, hi = X.keys_for_range(k, es)
        assert run_case(ctx, n, kr, UKT[es], lo=lo, hi=hi, want_keys=False, want_idx=False, what="count only")[0] == int(k.sum())
        assert run_case(ctx, n, kr, UKT[es], mask=X.mask_of(k), cap=0, what="cap 0")[0] == int(k.sum())


# ---- asynchrony and the workspace

@pytest.mark.parametrize("es", WIDTHS)
def test_two_calls_back_to_back_with_a_run_encode_between_them(ctx, es):
    """the calls share the context's scratch: only stream order keeps them apart"""
    import torch
    tile, scan_tile = limits(ctx, es)
    n1, n2 = (scan_tile + 1) * tile + 5, 3 * tile - 1
    k1, k2 = X.pattern("rand50", n1, tile, seed=18), X.pattern("rand1", n2, tile, seed=19)
    (a1, lo, hi), m2 = X.keys_for_range(k1, es), X.mask_of(k2)
    a2 = R.distinct(n2, es, seed=5)
    t1, t2 = torch.from_numpy(a1.view(R.IT[es])).cuda(), torch.from_numpy(a2.view(R.IT[es])).cuda()
    tm2 = torch.from_numpy(m2).cuda()
    kw1 = dict(lo=lo, hi=hi)
    assert 0 <= lo <= hi < 1 << (8 * es - 1)     # (signed tensors carry the bit patterns: the keys beyond hi are negative there, outside as well)
    ctx.compact(t1, indices=True, **kw1)                                     # (the workspace has its size: no reallocation, which would synchronise)
    torch.cuda.synchronize()
    r1 = ctx.compact(t1, indices=True, rest=True, **kw1)
    enc = ctx.run_encode(t1, inverse=True)
    r2 = ctx.compact(t2, mask=tm2, indices=True)
    r3 = ctx.compact(t1, cap=10, **kw1)
    torch.cuda.synchronize()
    host = lambda x: x.cpu().numpy().view(R.UT[es])
    ke = X.keep(n1, a1, E.I32 if es == 4 else E.I64, lo=lo, hi=hi)
    assert (ke == k1).all()
    m, ek, _, ei = X.expected(k1, a1, rest=True)
    assert int(r1[3].item()) == m and (host(r1[0]) == ek).all() and (r1[2].cpu().numpy() == ei).all()
    m, ek, _, ei = X.expected(k2, a2)
    assert int(r2[3].item()) == m and (host(r2[0])[:m] == ek).all() and (r2[2].cpu().numpy()[:m] == ei).all()
    m, ek, _, _ = X.expected(k1, a1, cap=10)
    assert int(r3[3].item()) == m and r3[0].numel() == 10 and (host(r3[0]) == ek).all() and r3[2] is None and r3[1] is None
    rm, rv, _, rinv = R.expected(a1)
    assert int(enc[0].item()) == rm and (enc[3].cpu().numpy() == rinv).all()


def test_the_workspace_is_a_word_per_tile_and_per_scan_piece(ctx):
    import torch
    from inplacemsdradixsort_amd import MsdContext
    tile, scan_tile = limits(ctx, 4)
    n = (scan_tile + 1) * tile + 5
    k = X.pattern("rand50", n, tile, seed=20)
    t = torch.from_numpy(R.distinct(n, 4).view(np.int32)).cuda()
    mask = torch.from_numpy(X.mask_of(k)).cuda()
    tiles = -(-n // tile)
    pieces = -(-tiles // scan_tile)
    need = -(-8 * tiles // 256) * 256 + 8 * pieces + 4096
    step = 1 << 20
    own = MsdContext(0)
    try:
        before = own.workspace_bytes
        out = own.compact(t, mask=mask, values=t, indices=True, rest=True)
        after = own.workspace_bytes
        assert 0 <= after - before <= -(-(need + need // 8) // step) * step, (before, after, need)
        own.run_encode(t)                                                    # (the same words)
        own.compact(t, mask=mask)
        assert own.workspace_bytes == after
        assert int(out[3].item()) == int(k.sum()) and (out[2].cpu().numpy() == np.argsort(~k, kind="stable")).all()
    finally:
        own.close()


# ---- relations

@pytest.mark.parametrize("es", WIDTHS)
def test_relations_with_torch_and_with_reduce_runs(ctx, es):
    import torch
    tile, _ = limits(ctx, es)
    n = 5 * tile + 123
    rng = np.random.default_rng(21)
    dt = torch.int32 if es == 4 else torch.int64
    keys = torch.from_numpy(rng.integers(0, 50, n).astype(R.IT[es])).cuda()          # few distinct keys: long groups
    vals = torch.from_numpy(rng.integers(-1000, 1000, n).astype(np.int64)).cuda()
    mask = torch.from_numpy(rng.random(n) < 0.4).cuda()
    # the count is torch's count of the keep mask; the positions gather the kept keys
    ok, ov, oi, count = ctx.compact(keys, mask=mask, lo=10, hi=39, values=vals, indices=True)
    keep = mask & (keys >= 10) & (keys <= 39)
    m = int(count.item())
    assert count.dtype == torch.int64 and m == int(torch.count_nonzero(keep).item())
    assert torch.equal(ok[:m], keys[oi[:m]]) and torch.equal(ov[:m], vals[oi[:m]]) and torch.equal(oi[:m], torch.nonzero(keep).flatten())
    assert ok.dtype == dt and ok.numel() == n
    # filter, then group by, on a table that is sorted by key: the partition's positions are what reduce_runs reads the value
    # column through; the kept keys' groups come first (the first rejected key, 0, differs from the last kept one)
    skeys, order = torch.sort(keys, stable=True)
    svals, smask = vals[order].contiguous(), mask[order].contiguous()
    pk, pv, pi, pcount = ctx.compact(skeys, mask=smask, lo=10, hi=39, values=svals, rest=True, indices=True)
    assert int(pcount.item()) == m and torch.equal(torch.sort(pi).values, torch.arange(n, device="cuda"))
    num_a, out_a = ctx.reduce_runs(pk, svals, op="sum", positions=pi)
    num_b, out_b = ctx.reduce_runs(pk[:m], pv[:m], op="sum")                 # the compacted column, reduced directly
    g = int(num_b.item())
    assert g == 30 and int(num_a.item()) > g and torch.equal(out_a[:g], out_b[:g])
    want = torch.zeros(50, dtype=torch.int64, device="cuda").index_add_(0, keys[keep].long(), vals[keep])[10:40]
    assert torch.equal(out_b[:g], want)


# ---- the Python wrappers

def test_wrappers_against_torch(ctx):
    import torch
    rng = np.random.default_rng(22)
    for dt, n in ((torch.float32, 100003), (torch.int64, 50001), (torch.float64, 4097), (torch.int32, 0), (torch.int32, 1)):
        if dt.is_floating_point:
            t = torch.from_numpy(rng.standard_normal(n)).to(dt).cuda()       # (no NaNs, no negative zeros)
        else:
            t = torch.from_numpy(rng.integers(-1000, 1000, n)).to(dt).cuda()
        mask = torch.from_numpy(rng.random(n) < 0.3).cuda()
        got = ctx.masked_select(t, mask)
        assert got.dtype == dt and torch.equal(got, torch.masked_select(t, mask))
        assert torch.equal(ctx.masked_select(t, mask.to(torch.uint8)), t[mask])
        assert torch.equal(ctx.nonzero(mask), torch.nonzero(mask).flatten()) and ctx.nonzero(mask).dtype == torch.int64
        assert torch.equal(ctx.nonzero(mask.to(torch.int8) * -3), torch.nonzero(mask).flatten())
        lo, hi = (-0.5, 1.25) if dt.is_floating_point else (-100, 250)
        want = (t >= lo) & (t <= hi)
        assert torch.equal(ctx.filter_range(t, lo, hi), t[want])
        v = torch.arange(n, device="cuda", dtype=torch.float64)
        fk, fv = ctx.filter_range(t, lo, hi, values=v)
        assert torch.equal(fk, t[want]) and torch.equal(fv, v[want])
        assert torch.equal(ctx.filter_range(t, lo, None), t[t >= lo]) and torch.equal(ctx.filter_range(t, None, hi), t[t <= hi])
    t2 = torch.from_numpy(rng.standard_normal((37, 113))).float().cuda()
    m2 = t2 > 0.5
    assert torch.equal(ctx.masked_select(t2, m2), torch.masked_select(t2, m2))


def test_where_the_range_differs_from_torch_and_the_phase(ctx):
    import torch
    nan = float("nan")
    host = np.array([-0.0, 0.0, nan, 1.0, -1.0, np.inf, nan, -np.inf], np.float32)
    host.view(np.uint32)[[2, 6]] = (0x7FC00000, 0xFFC00000)                  # a +NaN, and a NaN with the sign bit set
    t = torch.from_numpy(host).cuda()
    sign = torch.signbit(t).tolist()
    assert sign == [True, False, False, False, True, False, True, True]
    # torch: -0.0 >= 0.0 is true, a NaN compares false with everything
    assert (t >= 0.0).tolist() == [True, True, False, True, False, True, False, False]
    got = ctx.filter_range(t, 0.0, None)                                     # here: +0.0 and what lies above it, the +NaN included
    assert torch.equal(got.view(torch.int32), t[[1, 2, 3, 5]].view(torch.int32))
    assert [i for i in ctx.compact(t, lo=0.0, indices=True)[2][:4].tolist()] == [1, 2, 3, 5]
    assert ctx.compact(t, lo=-0.0, hi=-0.0, indices=True)[2][:1].tolist() == [0]
    assert ctx.compact(t, lo=float("-inf"), hi=float("inf"), indices=True, invert=True)[2][:2].tolist() == [2, 6]   # only the NaNs lie outside
    assert int(ctx.compact(t, hi=float("-inf"))[3].item()) == 2                # -inf and the -NaN below it
    assert int(ctx.compact(t, lo=1.0, hi=-1.0)[3].item()) == 0
    ok, _, oi, count = ctx.compact(t, lo=None, hi=None, mask=torch.ones(8, dtype=torch.bool, device="cuda"), indices=True)
    assert int(count.item()) == 8 and torch.equal(ok.view(torch.int32), t.view(torch.int32))   # bit-exact: payloads and signs of zero survive
    ctx.set_profiling(True)
    try:
        ctx.compact(t, lo=0.0, indices=True)
        assert [p[0] for p in ctx.phases()] == ["compact"]
    finally:
        ctx.set_profiling(False)
    assert ctx.compact_limits(4) == limits(ctx, 4) and ctx.compact_limits(8) == limits(ctx, 8)
    s = t[1:6]                                                               # a slice: 4 bytes off the 16-byte grid
    m = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1], dtype=torch.uint8, device="cuda")[3:8]   # and a mask 3 bytes off
    ok, _, oi, count = ctx.compact(s, mask=m, indices=True)
    assert int(count.item()) == 4 and oi[:4].tolist() == [0, 2, 3, 4] and ok[:4].tolist()[2:] == [-1.0, float("inf")]
