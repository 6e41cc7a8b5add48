"""Scan-by-key over runs (include/msd_scan_hip.h: msd_scan_runs, msd_scan_runs_limits; MsdContext.scan_runs /
scan_runs_limits) without a GPU: the header declares the two functions with the agreed argument lists, the four ops and the
two flags, the library exports them, the binding lists them apart from the other surfaces, a null context is refused first,
the limits call answers on the host, the Python wrapper refuses what never needs a device to be refused, and the numpy
expectation of tests/scan_expect.py is what its docstring says."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
import reduce_expect as X
import runs_expect as R
import scan_expect as S
import sort_rows_expect as E

SIGNATURES = {
    "msd_scan_runs": ["msd_ctx *ctx", "const void *d_keys", "int key_bytes", "uint64_t n", "const void *d_vals", "int val_type",
                      "const uint64_t *d_positions", "int op", "int flags", "void *d_out"],
    "msd_scan_runs_limits": ["int key_bytes", "uint64_t *tile", "uint64_t *scan_tile"],
}


def test_header_declares_the_two_functions_the_ops_and_the_flags():
    text, flat = A.header("msd_scan_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    assert re.search(r"enum \{ MSD_SCAN_SUM = 0, MSD_SCAN_MIN = 1, MSD_SCAN_MAX = 2, MSD_SCAN_COUNT = 3 \};", flat)
    assert re.search(r"enum \{ MSD_SCAN_EXCLUSIVE = 1, MSD_SCAN_SCATTER = 2 \};", flat)
    # the header says where the float order differs from torch, that sums are reproducible but not sequential and never
    # formed by subtraction, and states the identities
    for word in ("torch.cummax", "NaN", "-0.0", "totalOrder", "atomics", "same bits", "subtraction", "INT32_MAX", "INT64_MIN", "0x7FFFFFFF",
                 "NOT OFFERED"):                                    # (d_positions and MSD_SCAN_SCATTER: in the signature, refused)
        assert word in text, word
    # the names other ABI tests keep out of every header but their own
    for word in ("msd_set_sorted", "msd_merge_sorted", "msd_join", "msd_search"):
        assert word not in text, word


def test_the_scan_ops_are_the_reduce_ops():
    reduce_h, _ = A.header("msd_reduce_hip.h")
    for name, value in (("SUM", 0), ("MIN", 1), ("MAX", 2)):
        assert "MSD_REDUCE_%s = %d" % (name, value) in reduce_h and S.OPS[name.lower()] == X.OPS[name.lower()] == value
    assert S.OPS["count"] == 3 and (S.EXCLUSIVE, S.SCATTER) == (1, 2)


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_scan_hip.h", "msd_scan")


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("SCAN_EXPORTS", SIGNATURES, "msd_scan_hip.h", "msd_scan.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_scan_runs.argtypes[1:]]
    assert L.msd_scan_runs(None, *zeros) == -1
    assert L.msd_scan_runs(None, None, 4, 0, None, 0, None, 0, 0, None) == -1
    assert L.msd_scan_runs(None, None, 3, 10, None, 9, C.c_void_p(4), 7, 12, None) == -1
    p = C.c_void_p(64)
    assert L.msd_scan_runs(None, p, 8, 1 << 63, p, 5, p, 3, 3, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_are_those_of_run_encode():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile, scan_tile, t2, s2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert L.msd_scan_runs_limits(kb, C.byref(tile), C.byref(scan_tile)) == 0
        assert L.msd_run_encode_limits(kb, C.byref(t2), C.byref(s2)) == 0
        assert (tile.value, scan_tile.value) == (t2.value, s2.value) and tile.value >= 64 and scan_tile.value >= 64
    A.check_limits_refusals(L.msd_scan_runs_limits, 2, bad_widths=(0, 2, 16, -4, 5))


def test_limits_wrapper_and_ops_table():
    from inplacemsdradixsort_amd import MsdContext, MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        assert ctx.scan_runs_limits(kb) == ctx.run_encode_limits(kb)
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.scan_runs_limits(kb)
    assert MsdContext.SCAN_OPS == S.OPS
    assert {k: v for k, v in MsdContext.SCAN_OPS.items() if k != "count"} == MsdContext.REDUCE_OPS


def test_scan_runs_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    for kdt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for vdt in (torch.float32, torch.int64):
            for kw in ({}, {"op": "min"}, {"op": "max", "exclusive": True}, {"op": "count"}):
                with pytest.raises(MsdError, match="GPU"):          # CPU tensors
                    ctx.scan_runs(torch.zeros(8, dtype=kdt), torch.zeros(8, dtype=vdt), **kw)
        with pytest.raises(MsdError, match="GPU"):
            ctx.scan_runs(torch.zeros(8, dtype=kdt), None, op="count")
    k, v = torch.zeros(8, dtype=torch.int32), torch.zeros(8)
    for op in ("mean", "SUM", "cumsum", "", None, 0):
        with pytest.raises(MsdError, match="op must be"):           # a bad op name
            ctx.scan_runs(k, v, op=op)
    for op in ("sum", "min", "max"):
        with pytest.raises(MsdError, match="vals may be None"):     # missing values for an op that reads them
            ctx.scan_runs(k, None, op=op)
    with pytest.raises(MsdError, match="1-D"):                      # not 1-D
        ctx.scan_runs(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(MsdError, match="1-D"):
        ctx.scan_runs(k, torch.zeros(1, 8))
    with pytest.raises(MsdError, match="1-D"):
        ctx.scan_runs(torch.zeros(()), torch.zeros(()))
    with pytest.raises(MsdError, match="1-D"):
        ctx.scan_runs(torch.zeros(2, 4), None, op="count")
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.scan_runs(torch.zeros(16)[::2], v)
    with pytest.raises(MsdError, match="contiguous"):
        ctx.scan_runs(k, torch.zeros(16)[::2])
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="4- or 8-byte"):         # keys: an element size other than 4 or 8
            ctx.scan_runs(torch.zeros(8).to(dt), v)
        with pytest.raises(MsdError, match="4- or 8-byte"):
            ctx.scan_runs(torch.zeros(8).to(dt), None, op="count")
        with pytest.raises(MsdError, match="no key order"):         # values: a dtype the library has no order for
            ctx.scan_runs(k, torch.zeros(8).to(dt))
    for m in (0, 7, 9):
        with pytest.raises(MsdError, match="differ in length"):     # differing lengths
            ctx.scan_runs(k, torch.zeros(m))
    for pos in (torch.zeros(8, dtype=torch.int32), torch.zeros(8), torch.zeros(7, dtype=torch.int64), torch.zeros(9, dtype=torch.int64),
                torch.zeros(2, 4, dtype=torch.int64)):
        with pytest.raises(MsdError, match="positions must be"):    # positions of the wrong dtype or length
            ctx.scan_runs(k, v, positions=pos)
        with pytest.raises(MsdError, match="positions must be"):
            ctx.scan_runs(k, None, op="count", positions=pos)
    for kw in ({}, {"op": "count"}, {"op": "max", "exclusive": True}):
        with pytest.raises(MsdError, match="scatter without positions"):
            ctx.scan_runs(k, v, scatter=True, **kw)
        for scatter in (False, True):                               # positions are in the signature and not offered yet
            with pytest.raises(MsdError, match="not offered yet"):
                ctx.scan_runs(k, v, positions=torch.arange(8), scatter=scatter, **kw)


def test_the_docstring_says_where_the_results_differ_from_torch_and_why_there_is_no_group_scan():
    from inplacemsdradixsort_amd import MsdContext
    d = MsdContext.scan_runs.__doc__
    for word in ("torch.cummax", "torch.cummin", "NaN", "-0.0", "totalOrder", "atomics", "reproducible", "subtraction", "unstable", "composite"):
        assert word in d, word
    assert not hasattr(MsdContext, "group_scan")


# ---- the expectation

def test_the_expectation_on_worked_examples():
    keys = np.array([5, 5, 7, 5, 5, 5, 9], np.uint32)                                   # runs: [0, 2) [2, 3) [3, 6) [6, 7)
    v = np.array([1, 2, 3, 4, 5, 6, 0xFFFFFFFF], np.uint32)
    # unsigned and signed sums, 32-bit values widened to 64 bits
    out = S.expected(keys, v, E.U32, "sum")
    assert out.dtype == np.uint64 and out.tolist() == [1, 3, 3, 4, 9, 15, 0xFFFFFFFF]
    out = S.expected(keys, v, E.I32, "sum")
    assert out.dtype == np.int64 and out.tolist() == [1, 3, 3, 4, 9, 15, -1]
    assert S.expected(keys, v, E.U32, "sum", exclusive=True).tolist() == [0, 1, 0, 0, 4, 9, 0]
    assert S.expected(keys, v, E.I32, "sum", exclusive=True).tolist() == [0, 1, 0, 0, 4, 9, 0]
    # 64-bit sums wrap modulo 2^64
    big = np.array([1 << 63, 1 << 63, 1, (1 << 64) - 1, 2, 0, 7], np.uint64)
    assert S.expected(keys, big, E.U64, "sum").tolist() == [1 << 63, 0, 1, (1 << 64) - 1, 1, 1, 7]
    assert S.expected(keys, big, E.I64, "sum").tolist() == [-(1 << 63), 0, 1, -1, 1, 1, 7]
    assert S.expected(keys, big, E.U64, "sum", exclusive=True).tolist() == [0, 1 << 63, 0, 0, (1 << 64) - 1, 1, 0]
    i64 = np.array([(1 << 63) - 1, 1, -5, -1, -1, -1, 0], np.int64).view(np.uint64)
    assert S.expected(keys, i64, E.I64, "sum").tolist() == [(1 << 63) - 1, -(1 << 63), -5, -1, -2, -3, 0]
    # count: the row number, 1-based and 0-based; the values are not looked at
    assert S.expected(keys, None, 99, "count").dtype == np.uint64
    assert S.expected(keys, None, 99, "count").tolist() == [1, 2, 1, 1, 2, 3, 1]
    assert S.expected(keys, v, E.U32, "count", exclusive=True).tolist() == [0, 1, 0, 0, 1, 2, 0]
    # through positions: element i takes vals[positions[i]]; with scatter its result goes to positions[i]
    pos = np.array([6, 5, 4, 3, 2, 1, 0])
    assert S.expected(keys, v, E.U32, "sum", positions=pos).tolist() == [0xFFFFFFFF, 0xFFFFFFFF + 6, 5, 4, 7, 9, 1]
    assert S.expected(keys, v, E.U32, "sum", positions=pos, scatter=True).tolist() == [1, 9, 7, 4, 5, 0xFFFFFFFF + 6, 0xFFFFFFFF]
    assert S.expected(keys, v, E.U32, "sum", exclusive=True, positions=pos, scatter=True).tolist() == [0, 7, 4, 0, 0, 0xFFFFFFFF, 0]
    pos2 = np.array([2, 0, 1, 6, 3, 5, 4])
    assert S.expected(keys, None, 0, "count", positions=pos2).tolist() == [1, 2, 1, 1, 2, 3, 1]   # a count reads nothing through them
    assert S.expected(keys, None, 0, "count", positions=pos2, scatter=True).tolist() == [2, 1, 1, 2, 1, 3, 1]
    # min / max in the order of the type, and their identities
    s = np.array([3, -2, 7, -1, 0, 1, -9], np.int32).view(np.uint32)
    assert S.expected(keys, s, E.I32, "min").view(np.int32).tolist() == [3, -2, 7, -1, -1, -1, -9]
    assert S.expected(keys, s, E.I32, "max").view(np.int32).tolist() == [3, 3, 7, -1, 0, 1, -9]
    assert S.expected(keys, s, E.U32, "min").view(np.int32).tolist() == [3, 3, 7, -1, 0, 0, -9]          # as unsigned: negatives are large
    assert S.expected(keys, s, E.U32, "max").view(np.int32).tolist() == [3, -2, 7, -1, -1, -1, -9]
    imax, imin = (1 << 31) - 1, -(1 << 31)
    assert S.expected(keys, s, E.I32, "min", exclusive=True).view(np.int32).tolist() == [imax, 3, imax, imax, -1, -1, imax]
    assert S.expected(keys, s, E.I32, "max", exclusive=True).view(np.int32).tolist() == [imin, 3, imin, imin, -1, 0, imin]
    assert S.expected(keys, s, E.U32, "min", exclusive=True).tolist() == [0xFFFFFFFF, 3, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    assert S.expected(keys, s, E.U32, "max", exclusive=True).tolist() == [0, 3, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    # floats: sums in double, min / max in totalOrder on the bits
    f = np.array([0.5, 0.25, -1.0, 1.5, -0.5, 2.0, np.inf], np.float32)
    out = S.expected(keys, f.view(np.uint32), E.F32, "sum")
    assert out.dtype == np.float64 and out.tolist() == [0.5, 0.75, -1.0, 1.5, 1.0, 3.0, np.inf]
    out = S.expected(keys, f.view(np.uint32), E.F32, "sum", exclusive=True)
    assert out.tolist() == [0.0, 0.5, 0.0, 0.0, 1.5, 1.0, 0.0] and not np.signbit(out).any()
    qnan, sign, one = 0x7FC00000, 0x80000000, 0x3F800000
    z = np.array([0, sign, one, sign, qnan, 0x7F800000, qnan | sign | 1], np.uint32)                    # +0 -0 | 1 | -0 NaN inf | -NaN
    assert S.expected(keys, z, E.F32, "min").tolist() == [0, sign, one, sign, sign, sign, qnan | sign | 1]   # -0.0 is below +0.0
    assert S.expected(keys, z, E.F32, "max").tolist() == [0, 0, one, sign, qnan, qnan, qnan | sign | 1]      # a +NaN is the maximum, and stays it
    assert S.expected(keys, z, E.F32, "min", exclusive=True).tolist() == [0x7FFFFFFF, 0, 0x7FFFFFFF, 0x7FFFFFFF, sign, sign, 0x7FFFFFFF]
    assert S.expected(keys, z, E.F32, "max", exclusive=True).tolist() == [0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, sign, qnan, 0xFFFFFFFF]
    k2 = np.array([1, 1, 1, 1], np.uint64)
    z2 = np.array([0xFF800000, 0xFFC00000, 0x7FC00001, 0x7F800000], np.uint32)                            # -inf, -NaN, +NaN, +inf: 8-byte keys, 4-byte values
    assert S.expected(k2, z2, E.F32, "min").tolist() == [0xFF800000, 0xFFC00000, 0xFFC00000, 0xFFC00000]  # a -NaN is below -inf
    assert S.expected(k2, z2, E.F32, "max").tolist() == [0xFF800000, 0xFF800000, 0x7FC00001, 0x7FC00001]
    d = np.array([0.0, -0.0, np.nan, -np.inf], np.float64).view(np.uint64)
    assert S.expected(k2, d, E.F64, "min", exclusive=True).tolist() == [0x7FFFFFFFFFFFFFFF, 0, 1 << 63, 1 << 63]
    assert S.expected(k2, d, E.F64, "max", exclusive=True).tolist() == [0xFFFFFFFFFFFFFFFF, 0, 0, d[2]]
    # nothing at all
    for op in S.OPS:
        for kw in ({}, {"exclusive": True}, {"positions": np.zeros(0, np.int64), "scatter": True}):
            out = S.expected(keys[:0], v[:0], E.U32, op, **kw)
            assert out.size == 0 and out.dtype == S.out_dtype(E.U32, op)
    for vt in X.VAL_TYPES:
        assert S.out_dtype(vt, "sum").__name__ in ("uint64", "int64", "float64") and S.out_dtype(vt, "count") is np.uint64
        assert np.dtype(S.out_dtype(vt, "min")).itemsize == (4 if vt < 3 else 8)
    assert S.identity(E.I64, "min") == (1 << 63) - 1 and S.identity(E.I64, "max") == 1 << 63      # (bit patterns: INT64_MAX, INT64_MIN)
    assert S.identity(E.F64, "sum") == 0.0 and not np.signbit(S.identity(E.F64, "sum")) and S.identity(E.U32, "count") == 0


def test_the_vectorised_expectation_is_the_plain_loop():
    """200 random cases: short and long runs on both sides of scan_expect.LONG, every op and value type, both flags"""
    rng = np.random.default_rng(2024)
    for case in range(200):
        n = int(rng.integers(1, 400))
        kb = (4, 8)[case % 2]
        mean = (1.2, 3.0, 30.0, 150.0)[case % 4]
        keys = R.geometric(n, kb, mean, seed=case)
        vt = X.VAL_TYPES[case % 6]
        op = ("sum", "min", "max", "count")[(case // 6) % 4]
        ut = E.UT[vt]
        if vt in X.FLOAT and op == "sum":
            vbits = rng.standard_normal(n).astype(X.FLOAT[vt]).view(ut)
        else:
            vbits = rng.integers(0, 1 << (8 * np.dtype(ut).itemsize), n, dtype=ut)
            vbits[rng.random(n) < 0.3] &= ut(0xFF)                                     # (ties and small values among them)
        positions = rng.permutation(n).astype(np.int64) if case % 3 else None
        kw = dict(exclusive=bool(case % 2), positions=positions, scatter=positions is not None and case % 5 < 2)
        got, want = S.expected(keys, vbits, vt, op, **kw), S.naive(keys, vbits, vt, op, **kw)
        assert got.dtype == want.dtype
        assert (got.view(np.dtype("u%d" % got.itemsize)) == want.view(np.dtype("u%d" % want.itemsize))).all(), (case, op, vt, kw)
    assert R.expected(R.geometric(399, 4, 150.0, seed=3))[2].size < 399 // S.LONG + 20   # (there were runs beyond LONG)
