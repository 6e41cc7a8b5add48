"""GPU tests of what the typed entry points refuse, and in which order: msd_sort_keys, msd_sort_pairs_keys, msd_reverse,
msd_topk_rows and msd_sort_rows (msd_run_encode, msd_reduce_runs and msd_search_sorted have the same test next to their own).

Every refusal is provoked on its own and identified by words of its message; pairs of faults pin which of two is reported;
the edge cases that must be ACCEPTED are called too.  The calls go through the C ABI with every buffer inside a
guardband.Arena whose payload holds a known pattern: after a refusal every payload and every guard is what it was.  The
shapes are tiny (65 elements; 3 rows of 65 with stride 80): a refusal launches nothing."""
import ctypes as C

import numpy as np
import pytest

import sort_rows_expect as E
from gpu_support import DEFAULTS
from guardband import Buf

pytestmark = pytest.mark.gpu

U32, I32, F32, U64, I64, F64 = range(6)      # MSD_KEY_*
UKT = E.UKT                                   # the unsigned key type of a width: the order of the bit patterns
N = 65
ROWS, LEN, STRIDE = 3, 65, 80
EXTENT = (ROWS - 1) * STRIDE + LEN            # elements of a strided input: the padding behind the last row is not part of it


def keys_for(es, count, seed):
    return np.random.default_rng(seed).integers(0, 1 << (8 * es - 1), count, dtype=np.uint64).astype(E.UW[es])


def refuser(ctx, fn, order, good, bufs):
    """refused(words, **change): the good call with `change` answers MSD_EINVAL, its message holds every one of `words` (one
    string or several), and no buffer and no guard changed"""

    def refused(words, **change):
        k = dict(good, **change)
        rc = fn(ctx._h, *[k[a] for a in order])
        err = ctx._L.msd_last_error(ctx._h).decode()
        for w in ((words,) if isinstance(words, str) else words):
            assert rc == -1 and w in err, (change, rc, err)
        for b in bufs:
            assert b.unchanged(), change
            b.check(str(change))

    return refused


def off_grid(es):
    return (1, 2, 3) if es == 4 else (1, 2, 4, 7)


# ---- msd_sort_keys, msd_sort_pairs_keys

@pytest.mark.parametrize("es", (4, 8))
def test_sort_keys_refusals_in_order_touch_nothing(ctx, es):
    a = keys_for(es, N, 1)
    dk = Buf(es, N, a=a)
    order = ("keys", "kt", "n", "order")
    good = dict(keys=dk.ptr, kt=UKT[es], n=N, order=0)
    refused = refuser(ctx, ctx._L.msd_sort_keys, order, good, (dk,))
    # every refusal on its own, in the order of the code
    for bad in (-1, 6, 7, 100):
        refused("unknown key type", kt=bad)
    for bad in (-1, 2, 100):
        refused("order must be", order=bad)
    refused("null data pointer", keys=0)
    for d in range(es, 16, es):
        refused("16-byte aligned", keys=dk.ptr + d)
    for big in (1 << 36, (1 << 64) - 1):
        refused("n too large", n=big)
    # the order: of two faults the earlier one is reported
    refused("unknown key type", kt=9, order=5)
    refused("order must be", order=5, keys=0)
    refused("null data pointer", keys=0, n=1 << 36)
    refused("16-byte aligned", keys=dk.ptr + es, n=1 << 36)
    # accepted: nothing to sort (null or not, aligned or not a question that is asked of a null pointer)
    ctx._ok(ctx._L.msd_sort_keys(ctx._h, 0, UKT[es], 0, 0))
    ctx._ok(ctx._L.msd_sort_keys(ctx._h, dk.ptr, UKT[es], 0, 1))
    assert dk.unchanged()
    # and the call that all of these were changes of is fine
    ctx._ok(ctx._L.msd_sort_keys(ctx._h, *[good[k] for k in order]))
    assert (dk.host() == np.sort(a)).all()
    dk.check("good")


def test_sort_pairs_keys_refusals_in_order_touch_nothing(ctx):
    a = keys_for(8, N, 2)
    dk, dr = Buf(8, N, a=a), Buf(8, N, a=np.arange(N))
    order = ("keys", "kt", "rids", "n", "order")
    good = dict(keys=dk.ptr, kt=U64, rids=dr.ptr, n=N, order=0)
    refused = refuser(ctx, ctx._L.msd_sort_pairs_keys, order, good, (dk, dr))
    for bad in (-1, 6, 100):
        refused("unknown key type", kt=bad)
    for bad in (-1, 2):
        refused("order must be", order=bad)
    for kt32 in (U32, I32, F32):
        refused("tuples have 64-bit keys", kt=kt32)
    refused("null data pointer", keys=0)
    refused("null data pointer", rids=0)
    refused("16-byte aligned", keys=dk.ptr + 8)
    refused("16-byte aligned", rids=dr.ptr + 8)
    for big in (1 << 36, (1 << 64) - 1):
        refused("n too large", n=big)
    refused("keys and rids overlap", rids=dk.ptr)
    refused("keys and rids overlap", rids=dk.ptr + 16 * 8, n=N // 2)              # shifted by 16 elements: 16 shared
    refused("keys and rids overlap", keys=dr.ptr + 16 * 8, n=N // 2)
    refused("keys and rids overlap", rids=dk.ptr + 8 * (N - 1))                    # one element shared
    # the order
    refused("unknown key type", kt=9, order=5)
    refused("order must be", order=5, kt=F32)
    refused("tuples have 64-bit keys", kt=F32, keys=0)
    refused("null data pointer", keys=0, rids=dr.ptr + 8)
    refused("16-byte aligned", rids=dr.ptr + 8, n=1 << 36)
    refused("n too large", n=1 << 36, rids=dk.ptr)
    refused("n too large", n=(1 << 64) - 1, rids=dk.ptr)
    # accepted: nothing to sort; buffers that touch without sharing a byte
    ctx._ok(ctx._L.msd_sort_pairs_keys(ctx._h, 0, F64, 0, 0, 1))
    ctx._ok(ctx._L.msd_sort_pairs_keys(ctx._h, dk.ptr, U64, dk.ptr, 0, 0))
    assert dk.unchanged() and dr.unchanged()
    both = Buf(8, 64, a=np.concatenate([keys_for(8, 32, 3), np.arange(32, dtype=np.uint64)]))
    ctx._ok(ctx._L.msd_sort_pairs_keys(ctx._h, both.ptr, U64, both.ptr + 8 * 32, 32, 0))
    h = both.host()
    assert (h[:32] == np.sort(both.fill[:32])).all() and (both.fill[:32][h[32:]] == h[:32]).all()
    both.check("adjacent")
    # and the good call
    ctx._ok(ctx._L.msd_sort_pairs_keys(ctx._h, *[good[k] for k in order]))
    assert (dk.host() == np.sort(a)).all() and (a[dr.host()] == dk.host()).all()
    dk.check("good")
    dr.check("good")


# ---- msd_reverse

@pytest.mark.parametrize("es", (4, 8))
def test_reverse_refusals_in_order_touch_nothing(ctx, es):
    dd = Buf(es, N)
    order = ("data", "es", "first", "count")
    good = dict(data=dd.ptr, es=es, first=3, count=50)
    refused = refuser(ctx, ctx._L.msd_reverse, order, good, (dd,))
    for bad in (0, 2, 3, 16, -4):
        refused("elem_bytes", es=bad)
    refused("null data pointer", data=0)
    for d in off_grid(es):
        refused("aligned to its element size", data=dd.ptr + d)
        refused("aligned to its element size", data=dd.ptr + d, count=0)      # (asked whatever the count)
    refused("first + count overflows", first=(1 << 64) - 5, count=10)
    refused("first + count overflows", first=1 << 62, count=1 << 62)          # ... as a byte offset
    # the order
    refused("elem_bytes", es=3, data=0)
    refused("null data pointer", data=0, first=(1 << 64) - 5)
    refused("aligned to its element size", data=dd.ptr + 1, first=(1 << 64) - 5)
    # accepted: fewer than two elements, a null pointer among them
    for first, count, data in ((0, 0, 0), (7, 0, dd.ptr), (7, 1, dd.ptr), (N - 1, 1, dd.ptr)):
        ctx._ok(ctx._L.msd_reverse(ctx._h, data, es, first, count))
    assert dd.unchanged()
    dd.check("count < 2")
    # and the good call
    ctx._ok(ctx._L.msd_reverse(ctx._h, *[good[k] for k in order]))
    want = dd.fill.copy()
    want[3:53] = want[3:53][::-1]
    assert (dd.host() == want).all()
    dd.check("good")


# ---- msd_topk_rows

def strided(es, seed):
    """3 rows of 65 keys with stride 80, as the flat array of the whole buffer (3 * 80 elements) and as the rows"""
    flat = keys_for(es, ROWS * STRIDE, seed)
    return flat, flat.reshape(ROWS, STRIDE)[:, :LEN]


@pytest.mark.parametrize("es", (4, 8))
def test_topk_rows_refusals_in_order_touch_nothing(ctx, es):
    K = 5
    flat, rows = strided(es, 4)
    di, do, dx = Buf(es, ROWS * STRIDE, a=flat), Buf(es, ROWS * K), Buf(8, ROWS * K)
    order = ("inp", "kt", "rows", "len", "stride", "k", "which", "out", "idx")
    good = dict(inp=di.ptr, kt=UKT[es], rows=ROWS, len=LEN, stride=STRIDE, k=K, which=0, out=do.ptr, idx=dx.ptr)
    fn = ctx._L.msd_topk_rows
    refused = refuser(ctx, fn, order, good, (di, do, dx))
    for bad in (-1, 6, 100):
        refused("unknown key type", kt=bad)
    for bad in (-1, 2):
        refused("which must be", which=bad)
    refused("k must not exceed row_len", k=LEN + 1)
    refused("row_stride must not be smaller", stride=LEN - 1)
    refused("rows * row_stride overflows", rows=1 << 40, stride=1 << 40)
    refused("rows * row_stride overflows", rows=1 << 57)                       # ... as a byte count only
    if es == 4:   # (8-byte keys: k <= row_stride, so the input's byte count overflows first)
        refused("rows * k overflows", rows=1 << 55, len=64, stride=64, k=64)
    refused("null data pointer", inp=0)
    refused("null data pointer", out=0)
    for d in off_grid(es):
        refused("aligned to their element size", inp=di.ptr + d)
        refused("aligned to their element size", out=do.ptr + d)
    for d in (1, 2, 4, 7):
        refused("aligned to their element size", idx=dx.ptr + d)
    if es == 4:
        refused("indices of a 32-bit key type", rows=1, len=(1 << 32) + 1, stride=(1 << 32) + 1, k=1)
    refused("must not overlap", out=di.ptr)
    refused("must not overlap", out=di.ptr + (EXTENT - 1) * es)                # the last key of the last row
    refused("must not overlap", inp=do.ptr + (ROWS * K - 1) * es)
    refused("must not overlap", idx=di.ptr)
    refused("must not overlap", idx=di.ptr + (EXTENT * es - 8) // 8 * 8)
    refused("must not overlap", idx=do.ptr + (ROWS * K * es - 8) // 8 * 8)
    refused("must not overlap", out=dx.ptr + 8 * (ROWS * K - 1))
    # the order
    refused("unknown key type", kt=9, which=5)
    refused("unknown key type", kt=9, rows=0)
    refused("which must be", which=5, k=LEN + 1)
    refused("which must be", which=5, k=0)
    refused("k must not exceed row_len", k=LEN + 1, stride=LEN - 1)
    refused("row_stride must not be smaller", stride=LEN - 1, rows=1 << 62)
    refused("rows * row_stride overflows", rows=1 << 40, stride=1 << 40, inp=0)
    refused("null data pointer", inp=0, out=do.ptr + 1)
    refused("aligned to their element size", idx=dx.ptr + 4, out=di.ptr)
    if es == 4:
        refused("rows * k overflows", rows=1 << 55, len=64, stride=64, k=64, out=0)
        refused("aligned to their element size", inp=di.ptr + 2, rows=1, len=(1 << 32) + 1, stride=(1 << 32) + 1, k=1)
    # accepted: no rows or k == 0 before any pointer is looked at; without indices; an output right behind the input's extent
    ctx._ok(fn(ctx._h, 0, UKT[es], 0, LEN, STRIDE, K, 0, 0, 0))
    ctx._ok(fn(ctx._h, 0, UKT[es], ROWS, LEN, STRIDE, 0, 1, 0, 0))
    ctx._ok(fn(ctx._h, di.ptr + 1, UKT[es], 0, LEN, STRIDE, K, 0, do.ptr + 1, dx.ptr + 1))
    ctx._ok(fn(ctx._h, di.ptr, UKT[es], ROWS, LEN, STRIDE, 0, 0, di.ptr, di.ptr))
    for b in (di, do, dx):
        assert b.unchanged()
        b.check("nothing to do")
    want = np.sort(rows, axis=1)[:, :K]
    ctx._ok(fn(ctx._h, di.ptr, UKT[es], ROWS, LEN, STRIDE, K, 0, di.ptr + EXTENT * es, 0))   # (the padding holds 15 = 3 * 5 elements)
    h = di.host()
    assert (h[:EXTENT] == flat[:EXTENT]).all() and (h[EXTENT:].reshape(ROWS, K) == want).all()
    di.check("output behind the extent")
    di.reset()
    # and the good call
    ctx._ok(fn(ctx._h, *[good[k] for k in order]))
    got, pos = do.host().reshape(ROWS, K), dx.host().reshape(ROWS, K).astype(np.int64)
    assert (got == want).all() and (np.take_along_axis(rows, pos, 1) == got).all() and di.unchanged()
    for b in (di, do, dx):
        b.check("good")


# ---- msd_sort_rows

@pytest.mark.parametrize("es", (4, 8))
def test_sort_rows_refusals_in_order_touch_nothing(ctx, es):
    flat, rows = strided(es, 5)
    di, do, dx = Buf(es, ROWS * STRIDE, a=flat), Buf(es, ROWS * LEN), Buf(8, ROWS * LEN)
    order = ("inp", "kt", "rows", "len", "stride", "order", "out", "idx")
    good = dict(inp=di.ptr, kt=UKT[es], rows=ROWS, len=LEN, stride=STRIDE, order=0, out=do.ptr, idx=dx.ptr)
    fn = ctx._L.msd_sort_rows
    refused = refuser(ctx, fn, order, good, (di, do, dx))
    for bad in (-1, 6, 100):
        refused("unknown key type", kt=bad)
    for bad in (-1, 2):
        refused("order must be", order=bad)
    refused("row_stride must not be smaller", stride=LEN - 1)
    refused("rows * row_stride overflows", rows=1 << 40, stride=1 << 40)
    refused("rows * row_stride overflows", rows=1 << 57)                       # ... as a byte count only
    if es == 4:   # (8-byte keys: row_len <= row_stride, so the input's byte count overflows first)
        refused("rows * row_len overflows", rows=1 << 55, len=64, stride=64)
    refused("null data pointer", inp=0)
    refused("null data pointer", out=0)
    for d in off_grid(es):
        refused("aligned to their element size", inp=di.ptr + d)
        refused("aligned to their element size", out=do.ptr + d)
    for d in (1, 2, 4, 7):
        refused("aligned to their element size", idx=dx.ptr + d)
    refused("must not overlap", out=di.ptr)                                    # in place, but the rows are padded
    refused("must not overlap", out=di.ptr + 4 * es)
    refused("must not overlap", out=di.ptr + (EXTENT - 1) * es)
    refused("must not overlap", inp=do.ptr + (ROWS * LEN - 1) * es)
    refused("must not overlap", idx=di.ptr)
    refused("must not overlap", idx=di.ptr + (EXTENT * es - 8) // 8 * 8)
    refused("must not overlap", idx=do.ptr)
    refused("must not overlap", idx=do.ptr + (ROWS * LEN * es - 8) // 8 * 8)
    refused("must not overlap", out=dx.ptr + 8 * (ROWS * LEN - 1))
    refused("must not overlap", inp=do.ptr, out=do.ptr, stride=LEN, len=LEN, idx=do.ptr)   # in place is for the keys only
    # the segment path's own rule comes last
    ctx.set_option("sort_rows_mode", 1)
    try:
        if es == 4:
            refused(("16-byte", "segment sort"), out=do.ptr + 4)
            refused("must not overlap", out=di.ptr + 4)
        refused(("16-byte", "segment sort"), idx=dx.ptr + 8)
        refused("aligned to their element size", idx=dx.ptr + 4)
    finally:
        ctx.set_option("sort_rows_mode", DEFAULTS["sort_rows_mode"])
    # the order
    refused("unknown key type", kt=9, order=5)
    refused("unknown key type", kt=9, rows=0)
    refused("order must be", order=5, stride=LEN - 1)
    refused("order must be", order=5, len=0)
    refused("row_stride must not be smaller", stride=LEN - 1, rows=1 << 62)
    refused("rows * row_stride overflows", rows=1 << 40, stride=1 << 40, inp=0)
    refused("null data pointer", inp=0, out=do.ptr + 1)
    refused("aligned to their element size", idx=dx.ptr + 4, out=di.ptr)
    if es == 4:
        refused("rows * row_len overflows", rows=1 << 55, len=64, stride=64, out=0)
    # accepted: no rows or empty rows before any pointer is looked at
    ctx._ok(fn(ctx._h, 0, UKT[es], 0, LEN, STRIDE, 0, 0, 0))
    ctx._ok(fn(ctx._h, 0, UKT[es], ROWS, 0, STRIDE, 1, 0, 0))
    ctx._ok(fn(ctx._h, di.ptr + 1, UKT[es], 0, LEN, STRIDE, 0, do.ptr + 1, dx.ptr + 1))
    ctx._ok(fn(ctx._h, di.ptr, UKT[es], ROWS, 0, 0, 0, di.ptr, di.ptr))
    for b in (di, do, dx):
        assert b.unchanged()
        b.check("nothing to do")
    # accepted: in place, d_out_keys == d_keys with row_stride == row_len, with positions elsewhere
    dense = Buf(es, ROWS * LEN, a=np.ascontiguousarray(rows).reshape(-1))
    ctx._ok(fn(ctx._h, dense.ptr, UKT[es], ROWS, LEN, LEN, 0, dense.ptr, dx.ptr))
    got, pos = dense.host().reshape(ROWS, LEN), dx.host().reshape(ROWS, LEN).astype(np.int64)
    assert (got == np.sort(rows, axis=1)).all() and (np.take_along_axis(rows, pos, 1) == got).all()
    dense.check("in place")
    dx.check("in place")
    dx.reset()
    # and the good call
    ctx._ok(fn(ctx._h, *[good[k] for k in order]))
    got, pos = do.host().reshape(ROWS, LEN), dx.host().reshape(ROWS, LEN).astype(np.int64)
    assert (got == np.sort(rows, axis=1)).all() and (np.take_along_axis(rows, pos, 1) == got).all() and di.unchanged()
    for b in (di, do, dx):
        b.check("good")
