"""Stream compaction and stable partition (include/msd_compact_hip.h: msd_compact, msd_compact_limits; MsdContext.compact /
compact_limits / masked_select / nonzero / filter_range) without a GPU: the header declares the two functions with the agreed
argument lists and the three flags, the library exports them, the binding lists them apart from the other surfaces, a null
context is refused first, the limits call answers on the host, the Python wrapper refuses what never needs a device to be
refused, and the numpy expectation of tests/compact_expect.py is what its docstring says."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
import compact_expect as X
import sort_rows_expect as E

SIGNATURES = {
    "msd_compact": ["msd_ctx *ctx", "const void *d_keys", "int key_type", "uint64_t n", "const uint8_t *d_mask", "uint64_t lo_bits", "uint64_t hi_bits",
                    "int flags", "const void *d_vals", "int val_bytes", "uint64_t cap", "void *d_out_keys", "void *d_out_vals", "uint64_t *d_out_idx",
                    "uint64_t *d_count"],
    "msd_compact_limits": ["int key_bytes", "uint64_t *tile", "uint64_t *scan_tile"],
}


def test_header_declares_the_two_functions_and_the_flags():
    text, flat = A.header("msd_compact_hip.h")
    assert '#include "msd_radix_hip.h"' in flat and flat.count("#include") == 1
    A.check_signatures(flat, SIGNATURES)
    assert re.search(r"enum \{ MSD_COMPACT_RANGE = 1, MSD_COMPACT_INVERT = 2, MSD_COMPACT_REST = 4 \};", flat)
    assert (X.RANGE, X.INVERT, X.REST) == (1, 2, 4)
    for word in ("stable", "totalOrder", "-0.0", "NaN", "checked in this order", "true count", "torch"):
        assert word in text, word
    # the names other ABI tests keep out of every header but their own
    for word in ("msd_scan", "msd_join", "msd_search", "msd_set_sorted", "msd_merge_sorted", "msd_reduce"):
        assert word not in text, word


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_compact_hip.h", "msd_compact")


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("COMPACT_EXPORTS", SIGNATURES, "msd_compact_hip.h", "msd_compact.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_compact.argtypes[1:]]
    assert L.msd_compact(None, *zeros) == -1
    p = C.c_void_p(64)
    assert L.msd_compact(None, p, 0, 10, p, 1, 5, 1, p, 8, 10, p, p, p, p) == -1
    assert L.msd_compact(None, C.c_void_p(3), 77, 1 << 63, None, 1 << 40, 0, 64, p, 3, 0, None, None, C.c_void_p(4), None) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_are_those_of_run_encode():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile, scan_tile, t2, s2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert L.msd_compact_limits(kb, C.byref(tile), C.byref(scan_tile)) == 0
        assert L.msd_run_encode_limits(kb, C.byref(t2), C.byref(s2)) == 0
        assert (tile.value, scan_tile.value) == (t2.value, s2.value) and tile.value >= 64 and scan_tile.value >= 64
    A.check_limits_refusals(L.msd_compact_limits, 2, bad_widths=(0, 2, 16, -4, 5))


def test_limits_wrapper_and_flags():
    from inplacemsdradixsort_amd import MsdContext, MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        assert ctx.compact_limits(kb) == ctx.run_encode_limits(kb)
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.compact_limits(kb)
    assert (MsdContext.COMPACT_RANGE, MsdContext.COMPACT_INVERT, MsdContext.COMPACT_REST) == (X.RANGE, X.INVERT, X.REST)


def test_compact_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    m8 = torch.ones(8, dtype=torch.bool)
    for kdt in (torch.float32, torch.int32, torch.float64, torch.int64):
        k = torch.zeros(8, dtype=kdt)
        for kw in ({"mask": m8}, {"lo": 0}, {"lo": 0, "hi": 1, "invert": True}, {"mask": m8, "rest": True, "indices": True}, {"values": torch.zeros(8)}, {}):
            with pytest.raises(MsdError, match="GPU"):              # CPU tensors
                ctx.compact(k, **kw)
    with pytest.raises(MsdError, match="GPU"):
        ctx.compact(mask=m8, indices=True)
    with pytest.raises(MsdError, match="GPU"):
        ctx.nonzero(m8)
    with pytest.raises(MsdError, match="GPU"):
        ctx.masked_select(torch.zeros(2, 4), torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(MsdError, match="GPU"):
        ctx.filter_range(torch.zeros(8), 0.0, 1.0)
    k, v = torch.zeros(8, dtype=torch.int32), torch.zeros(8)
    with pytest.raises(MsdError, match="keys or a mask"):
        ctx.compact()
    with pytest.raises(MsdError, match="keys or a mask"):
        ctx.compact(values=v)
    with pytest.raises(MsdError, match="1-D"):                      # not 1-D
        ctx.compact(torch.zeros(2, 4))
    with pytest.raises(MsdError, match="1-D"):
        ctx.compact(k, mask=torch.ones(1, 8, dtype=torch.bool))
    with pytest.raises(MsdError, match="1-D"):
        ctx.compact(torch.zeros(()))
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.compact(torch.zeros(16)[::2])
    with pytest.raises(MsdError, match="contiguous"):
        ctx.compact(k, mask=torch.ones(16, dtype=torch.bool)[::2])
    with pytest.raises(MsdError, match="contiguous"):
        ctx.compact(k, values=torch.zeros(16)[::2])
    for other in (0, 7, 9):
        with pytest.raises(MsdError, match="differ in length"):     # differing lengths
            ctx.compact(k, mask=torch.ones(other, dtype=torch.bool))
        with pytest.raises(MsdError, match="differ in length"):
            ctx.compact(k, values=torch.zeros(other))
        with pytest.raises(MsdError, match="differ in length"):
            ctx.compact(mask=m8, values=torch.zeros(other))
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):         # keys: a dtype the library has no order for
            ctx.compact(torch.zeros(8).to(dt))
    for dt in (torch.float16, torch.int16, torch.uint8):
        with pytest.raises(MsdError, match="4- or 8-byte"):         # values: an element size other than 4 or 8
            ctx.compact(k, values=torch.zeros(8).to(dt))
    for dt in (torch.float32, torch.int32, torch.int16, torch.int64):
        with pytest.raises(MsdError, match="one-byte"):             # the mask: one byte per element
            ctx.compact(k, mask=torch.ones(8, dtype=dt))
    with pytest.raises(MsdError, match="without keys"):
        ctx.compact(mask=m8, lo=3)
    with pytest.raises(MsdError, match="without keys"):
        ctx.compact(mask=m8, out=torch.zeros(8))
    with pytest.raises(MsdError, match="without values"):
        ctx.compact(k, out_values=torch.zeros(8))
    with pytest.raises(MsdError, match="negative"):
        ctx.compact(k, cap=-1)
    with pytest.raises(MsdError, match="rest needs cap"):
        ctx.compact(k, rest=True, cap=7)
    for bad in (torch.zeros(8), torch.zeros(7, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(16, dtype=torch.int32)[::2]):
        with pytest.raises(MsdError, match="out must be"):          # outputs of the wrong dtype, length or layout
            ctx.compact(k, out=bad)
    with pytest.raises(MsdError, match="out_values must be"):
        ctx.compact(k, values=v, out_values=torch.zeros(8, dtype=torch.float64))
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.int64)):
        with pytest.raises(MsdError, match="out_indices must be"):
            ctx.compact(k, out_indices=bad)
    with pytest.raises(MsdError, match="one shape"):
        ctx.masked_select(torch.zeros(8), torch.ones(7, dtype=torch.bool))
    with pytest.raises(MsdError, match="takes a bound"):
        ctx.filter_range(k, None, None)


def test_bounds_become_bit_patterns_of_the_keys_dtype():
    import torch
    from inplacemsdradixsort_amd import MsdContext, MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    f32, f64, i32, i64 = (torch.zeros(1, dtype=d) for d in (torch.float32, torch.float64, torch.int32, torch.int64))
    K = MsdContext
    assert ctx._bound_bits(f32, K.KEY_F32, -0.0, True) == 0x80000000 and ctx._bound_bits(f32, K.KEY_F32, 0.0, True) == 0
    assert ctx._bound_bits(f32, K.KEY_F32, 1.0, True) == 0x3F800000 and ctx._bound_bits(f32, K.KEY_F32, float("inf"), False) == 0x7F800000
    assert ctx._bound_bits(f64, K.KEY_F64, -0.0, True) == 1 << 63 and ctx._bound_bits(f64, K.KEY_F64, 1, False) == 0x3FF << 52
    assert ctx._bound_bits(i32, K.KEY_I32, -1, True) == 0xFFFFFFFF and ctx._bound_bits(i64, K.KEY_I64, -2, True) == (1 << 64) - 2
    # None: the key with the lowest / highest code
    assert ctx._bound_bits(f32, K.KEY_F32, None, True) == 0xFFFFFFFF and ctx._bound_bits(f32, K.KEY_F32, None, False) == 0x7FFFFFFF
    assert ctx._bound_bits(i32, K.KEY_I32, None, True) == 0x80000000 and ctx._bound_bits(i32, K.KEY_I32, None, False) == 0x7FFFFFFF
    assert ctx._bound_bits(i64, K.KEY_I64, None, True) == 1 << 63 and ctx._bound_bits(f64, K.KEY_F64, None, False) == (1 << 63) - 1
    for bad in (1 << 31, -(1 << 31) - 1, 1.5, "x"):
        with pytest.raises(MsdError, match="is not a value"):
            ctx._bound_bits(i32, K.KEY_I32, bad, True)


def test_the_docstrings_say_what_the_filter_promises():
    from inplacemsdradixsort_amd import MsdContext
    d = MsdContext.compact.__doc__
    for word in ("stable", "bit-exact", "totalOrder", "-0.0", "NaN", "not modified", "Nothing waits on the host"):
        assert word in d, word
    for f in (MsdContext.masked_select, MsdContext.nonzero, MsdContext.filter_range):
        assert "ONE host wait" in f.__doc__, f.__name__
    assert "radix" in MsdContext.partition.__doc__.lower() or "digit" in MsdContext.partition.__doc__.lower()   # (that name stays the radix partition's)


# ---- the expectation

def test_the_expectation_on_worked_examples():
    keys = np.array([5, 9, 7, 5, 1, 8, 7], np.uint32)
    vals = np.array([10, 11, 12, 13, 14, 15, 16], np.uint64)
    mask = np.array([1, 0, 0x80, 0xFF, 0, 2, 0], np.uint8)
    k = X.keep(7, mask=mask)
    assert k.tolist() == [True, False, True, True, False, True, False]
    m, ek, ev, ei = X.expected(k, keys, vals)
    assert m == 4 and ek.tolist() == [5, 7, 5, 8] and ev.tolist() == [10, 12, 13, 15] and ei.tolist() == [0, 2, 3, 5] and ei.dtype == np.int64
    m, ek, ev, ei = X.expected(k, keys, vals, rest=True)
    assert m == 4 and ek.tolist() == [5, 7, 5, 8, 9, 1, 7] and ei.tolist() == [0, 2, 3, 5, 1, 4, 6] and ev.tolist() == [10, 12, 13, 15, 11, 14, 16]
    assert (ei == np.argsort(~k, kind="stable")).all()
    m, ek, ev, ei = X.expected(k, keys, None, cap=3)
    assert m == 4 and ek.tolist() == [5, 7, 5] and ev is None and ei.tolist() == [0, 2, 3]
    assert X.expected(k, cap=0)[0] == 4 and X.expected(k, cap=0)[3].size == 0 and X.expected(k)[1] is None
    # a range, both bounds inclusive; with the mask; inverted
    assert X.keep(7, keys, E.U32, lo=5, hi=7).tolist() == [True, False, True, True, False, False, True]
    assert X.keep(7, keys, E.U32, lo=7, hi=7).tolist() == [False, False, True, False, False, False, True]
    assert not X.keep(7, keys, E.U32, lo=7, hi=5).any() and X.keep(7, keys, E.U32, lo=7, hi=5, invert=True).all()
    assert X.keep(7, keys, E.U32, mask=mask, lo=5, hi=7).tolist() == [True, False, True, True, False, False, False]
    assert X.keep(7, keys, E.U32, mask=mask, lo=5, hi=7, invert=True).tolist() == [False, True, False, False, True, True, True]
    assert X.keep(3).all() and not X.keep(3, invert=True).any()
    # signed: the bit pattern of -1 lies below 0
    s = np.array([-3, -1, 0, 2, 5], np.int32).view(np.uint32)
    assert X.keep(5, s, E.I32, lo=0xFFFFFFFF, hi=2).tolist() == [False, True, True, True, False]
    assert not X.keep(5, s, E.U32, lo=0xFFFFFFFF, hi=2).any()
    # floats in totalOrder: -NaN < -inf < -1 < -0.0 < +0.0 < 1 < +inf < +NaN
    for ft, ut, kt in ((np.float32, np.uint32, E.F32), (np.float64, np.uint64, E.F64)):
        S = X.float_specials(ft)
        one = int(np.array([1.0], ft).view(ut)[0])
        f = np.array([S["-0"], S["+0"], S["-nan"], S["+nan"], one, S["-inf"], S["+inf"]], ut)
        assert X.keep(7, f, kt, lo=S["-0"], hi=S["+0"]).tolist() == [True, True, False, False, False, False, False]
        assert X.keep(7, f, kt, lo=S["+0"], hi=S["+0"]).tolist() == [False, True, False, False, False, False, False]   # a bound of +0.0 excludes -0.0
        assert X.keep(7, f, kt, lo=S["-0"], hi=S["-0"]).tolist() == [True, False, False, False, False, False, False]
        assert X.keep(7, f, kt, lo=S["+0"], hi=S["+inf"]).tolist() == [False, True, False, False, True, False, True]
        assert X.keep(7, f, kt, lo=S["+inf"], hi=S["+nanmax"]).tolist() == [False, False, False, True, False, False, True]
        assert X.keep(7, f, kt, lo=S["-nanmax"], hi=S["-inf"]).tolist() == [False, False, True, False, False, True, False]
        assert X.keep(7, f, kt, lo=S["-inf"], hi=S["+inf"]).tolist() == [True, True, False, False, True, True, True]   # the NaNs lie outside
        assert X.keep(7, f, kt, lo=S["-nanmax"], hi=S["+nanmax"]).all()
    # nothing at all
    m, ek, ev, ei = X.expected(X.keep(0), keys[:0], vals[:0], rest=True)
    assert m == 0 and ek.size == 0 and ev.size == 0 and ei.size == 0


def test_the_patterns_and_the_inputs_built_from_them():
    T = 64
    n = 3 * T - 1
    assert X.pattern("all", n, T).all() and not X.pattern("none", n, T).any()
    assert np.flatnonzero(X.pattern("tile_last", n, T)).tolist() == [63, 127] and np.flatnonzero(X.pattern("tile_first", n, T)).tolist() == [0, 64, 128]
    assert np.flatnonzero(X.pattern("first", n, T)).tolist() == [0] and np.flatnonzero(X.pattern("last", n, T)).tolist() == [n - 1]
    b = np.flatnonzero(X.pattern("block", n, T))
    assert b.size == T and b[0] % T != 0 and (np.diff(b) == 1).all()
    assert np.flatnonzero(X.pattern("every65", n, T)).tolist() == [0, 65, 130]
    assert not X.pattern("first", 0, T).any() and X.pattern("last", 1, T).tolist() == [True]
    for name in X.PATTERNS:
        k = X.pattern(name, n, T)
        assert k.dtype == bool and k.size == n
        mask = X.mask_of(k)
        assert ((mask != 0) == k).all() and set(np.unique(mask).tolist()) <= {0, 1, 2, 0x80, 0xFF}
        for es in (4, 8):
            keys, lo, hi = X.keys_for_range(k, es)
            assert keys.dtype == X.UT[es] and (X.keep(n, keys, E.U32 if es == 4 else E.U64, lo=lo, hi=hi) == k).all()
    assert 0.3 < X.pattern("rand50", 10000, T).mean() < 0.7 and X.pattern("rand1", 10000, T).mean() < 0.03 < 0.9 < X.pattern("rand99", 10000, T).mean()
    for vb in (4, 8):
        v = X.values_for(100, vb)
        assert v.dtype == X.UT[vb] and np.unique(v).size == 100


def test_the_vectorised_expectation_is_the_plain_loop():
    """200 random cases: every key type, with and without mask and range, inverted, rest, capped"""
    rng = np.random.default_rng(2025)
    for case in range(200):
        n = int(rng.integers(0, 300))
        kt = case % 6
        ut = E.UT[kt]
        W = 8 * np.dtype(ut).itemsize
        keys = rng.integers(0, 1 << W, n, dtype=ut, endpoint=False) if W == 32 else rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
        keys[rng.random(n) < 0.3] &= ut(0xFF)
        keys[rng.random(n) < 0.2] |= ut(1 << (W - 1))
        use_mask, use_range = case % 3 != 0, case % 4 != 1
        mask = X.mask_of(rng.random(n) < 0.6, seed=case) if use_mask else None
        lo = hi = None
        if use_range:
            lo, hi = (int(x) for x in rng.integers(0, 1 << W, 2, dtype=ut)) if W == 32 else (int(x) for x in rng.integers(0, (1 << 64) - 1, 2, dtype=np.uint64))
            if case % 7 == 0 and n:
                lo = hi = int(keys[n // 2])
        vals = X.values_for(n, (4, 8)[case % 2], seed=case) if case % 5 else None
        kw = dict(keys=keys, kt=kt, mask=mask, lo=lo, hi=hi, invert=bool(case % 2))
        rest = case % 8 == 3
        cap = None if rest or case % 3 else int(rng.integers(0, n + 2))
        got = X.expected(X.keep(n, **kw), keys, vals, rest=rest, cap=cap)
        want = X.naive(n, vals=vals, rest=rest, cap=cap, **kw)
        assert got[0] == want[0], case
        for g, w in zip(got[1:], want[1:]):
            assert (g is None) == (w is None) and (g is None or (g.dtype == w.dtype and g.tolist() == w.tolist())), case
