"""Reduce-by-key over runs (include/msd_reduce_hip.h: msd_reduce_runs, msd_reduce_runs_limits; MsdContext.reduce_runs /
reduce_runs_limits / group_reduce) without a GPU: the header declares the two functions with the agreed argument lists and the
three ops, the library exports them, the binding lists them apart from the other surfaces, a null context is refused first,
the limits call answers on the host, the Python wrappers refuse what never needs a device to be refused, and the numpy
expectation of tests/reduce_expect.py is what its docstring says."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
import reduce_expect as X
import sort_rows_expect as E

SIGNATURES = {
    "msd_reduce_runs": ["msd_ctx *ctx", "const void *d_keys", "int key_bytes", "uint64_t n", "const void *d_vals", "int val_type",
                        "const uint64_t *d_positions", "int op", "uint64_t cap", "void *d_out", "uint64_t *d_num_runs"],
    "msd_reduce_runs_limits": ["int key_bytes", "uint64_t *tile", "uint64_t *scan_tile"],
}


def test_header_declares_the_two_functions_and_the_ops():
    text, flat = A.header("msd_reduce_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    assert re.search(r"enum \{ MSD_REDUCE_SUM = 0, MSD_REDUCE_MIN = 1, MSD_REDUCE_MAX = 2 \};", flat)
    # the header says where the float order differs from torch, and that sums are reproducible but not sequential
    assert "torch.amax" in text and "torch.amin" in text and "NaN" in text and "-0.0" in text and "totalOrder" in text
    assert "atomics" in text and "same bits" in text


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_reduce_hip.h", "msd_reduce", headers=("msd_runs_hip.h", "msd_radix_hip.h"))


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("REDUCE_EXPORTS", SIGNATURES, "msd_reduce_hip.h", "msd_reduce.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_reduce_runs.argtypes[1:]]
    assert L.msd_reduce_runs(None, *zeros) == -1
    assert L.msd_reduce_runs(None, None, 4, 0, None, 0, None, 0, 0, None, None) == -1
    assert L.msd_reduce_runs(None, None, 3, 10, None, 9, C.c_void_p(4), 7, 10, None, None) == -1
    p = C.c_void_p(64)
    assert L.msd_reduce_runs(None, p, 8, 1 << 63, p, 5, p, 2, 1 << 63, p, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_are_those_of_run_encode():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile, scan_tile, t2, s2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert L.msd_reduce_runs_limits(kb, C.byref(tile), C.byref(scan_tile)) == 0
        assert L.msd_run_encode_limits(kb, C.byref(t2), C.byref(s2)) == 0
        assert (tile.value, scan_tile.value) == (t2.value, s2.value) and tile.value >= 64 and scan_tile.value >= 64
    A.check_limits_refusals(L.msd_reduce_runs_limits, 2, bad_widths=(0, 2, 16, -4, 5))


def test_limits_wrapper():
    from inplacemsdradixsort_amd import MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        assert ctx.reduce_runs_limits(kb) == ctx.run_encode_limits(kb)
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.reduce_runs_limits(kb)


def test_reduce_runs_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    for kdt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for vdt in (torch.float32, torch.int64):
            for kw in ({}, {"op": "min"}, {"op": "max", "cap": 3}, {"positions": torch.arange(8)}):
                with pytest.raises(MsdError, match="GPU"):          # CPU tensors
                    ctx.reduce_runs(torch.zeros(8, dtype=kdt), torch.zeros(8, dtype=vdt), **kw)
    k, v = torch.zeros(8, dtype=torch.int32), torch.zeros(8)
    for op in ("mean", "SUM", "", None, 0):
        with pytest.raises(MsdError, match="op must be"):           # a bad op name
            ctx.reduce_runs(k, v, op=op)
    with pytest.raises(MsdError, match="1-D"):                      # not 1-D
        ctx.reduce_runs(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(MsdError, match="1-D"):
        ctx.reduce_runs(k, torch.zeros(1, 8))
    with pytest.raises(MsdError, match="1-D"):
        ctx.reduce_runs(torch.zeros(()), torch.zeros(()))
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.reduce_runs(torch.zeros(16)[::2], v)
    with pytest.raises(MsdError, match="contiguous"):
        ctx.reduce_runs(k, torch.zeros(16)[::2])
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="4- or 8-byte"):         # keys: an element size other than 4 or 8
            ctx.reduce_runs(torch.zeros(8).to(dt), v)
        with pytest.raises(MsdError, match="no key order"):         # values: a dtype the library has no order for
            ctx.reduce_runs(k, torch.zeros(8).to(dt))
    for m in (0, 7, 9):
        with pytest.raises(MsdError, match="differ in length"):     # differing lengths
            ctx.reduce_runs(k, torch.zeros(m))
    for pos in (torch.zeros(8, dtype=torch.int32), torch.zeros(8), torch.zeros(7, dtype=torch.int64), torch.zeros(9, dtype=torch.int64),
                torch.zeros(2, 4, dtype=torch.int64)):
        with pytest.raises(MsdError, match="positions must be"):    # positions of the wrong dtype or length
            ctx.reduce_runs(k, v, positions=pos)
    with pytest.raises(MsdError, match="cap"):
        ctx.reduce_runs(k, v, cap=-1)


def test_group_reduce_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()
    for kdt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for op in ("sum", "min", "max"):
            with pytest.raises(MsdError, match="GPU"):
                ctx.group_reduce(torch.zeros(8, dtype=kdt), torch.zeros(8), op=op)
    k, v = torch.zeros(8, dtype=torch.int32), torch.zeros(8)
    with pytest.raises(MsdError, match="op must be"):
        ctx.group_reduce(k, v, op="mean")
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):
            ctx.group_reduce(torch.zeros(8).to(dt), v)
        with pytest.raises(MsdError, match="no key order"):
            ctx.group_reduce(k, torch.zeros(8).to(dt))
    with pytest.raises(MsdError, match="1-D"):
        ctx.group_reduce(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(MsdError, match="contiguous"):
        ctx.group_reduce(torch.zeros(16)[::2], v)
    with pytest.raises(MsdError, match="differ in length"):
        ctx.group_reduce(k, torch.zeros(9))


def test_the_docstrings_say_where_the_results_differ_from_torch():
    from inplacemsdradixsort_amd import MsdContext
    d = MsdContext.reduce_runs.__doc__
    assert "torch.amax" in d and "torch.amin" in d and "NaN" in d and "-0.0" in d and "atomics" in d
    assert "not modified" in MsdContext.group_reduce.__doc__


def test_the_expectation_on_worked_examples():
    keys = np.array([5, 5, 7, 5, 5, 5, 9], np.uint32)
    # unsigned and signed sums, 32-bit values widened to 64 bits
    v = np.array([1, 2, 3, 4, 5, 6, 0xFFFFFFFF], np.uint32)
    m, starts, out = X.expected(keys, v, E.U32, "sum")
    assert m == 4 and starts.tolist() == [0, 2, 3, 6, 7] and out.dtype == np.uint64 and out.tolist() == [3, 3, 15, 0xFFFFFFFF]
    m, _, out = X.expected(keys, v, E.I32, "sum")
    assert out.dtype == np.int64 and out.tolist() == [3, 3, 15, -1]
    # 64-bit sums wrap modulo 2^64
    big = np.array([1 << 63, 1 << 63, 1, (1 << 64) - 1, 2, 0, 7], np.uint64)
    assert X.expected(keys, big, E.U64, "sum")[2].tolist() == [0, 1, 1, 7]
    assert X.expected(keys, big, E.I64, "sum")[2].tolist() == [0, 1, 1, 7]
    i64 = np.array([(1 << 63) - 1, 1, -5, -1, -1, -1, 0], np.int64).view(np.uint64)
    assert X.expected(keys, i64, E.I64, "sum")[2].tolist() == [-(1 << 63), -5, -3, 0]
    # through positions: element i takes vals[positions[i]]
    pos = np.array([6, 5, 4, 3, 2, 1, 0])
    assert X.expected(keys, v, E.U32, "sum", pos)[2].tolist() == [0xFFFFFFFF + 6, 5, 4 + 3 + 2, 1]
    # min / max in the order of the type
    s = np.array([3, -2, 7, -1, 0, 1, -9], np.int32).view(np.uint32)
    assert X.expected(keys, s, E.I32, "min")[2].view(np.int32).tolist() == [-2, 7, -1, -9]
    assert X.expected(keys, s, E.I32, "max")[2].view(np.int32).tolist() == [3, 7, 1, -9]
    assert X.expected(keys, s, E.U32, "min")[2].view(np.int32).tolist() == [3, 7, 0, -9]          # as unsigned: negatives are large
    assert X.expected(keys, s, E.U32, "max")[2].view(np.int32).tolist() == [-2, 7, -1, -9]
    # floats: sums in double, min / max in totalOrder on the bits
    f = np.array([0.5, 0.25, -1.0, 1.5, -0.5, 2.0, np.inf], np.float32)
    out = X.expected(keys, f.view(np.uint32), E.F32, "sum")[2]
    assert out.dtype == np.float64 and out.tolist() == [0.75, -1.0, 3.0, np.inf]
    qnan, sign = 0x7FC00000, 0x80000000
    z = np.array([0, sign, 0x3F800000, sign, qnan, 0x7F800000, qnan | sign | 1], np.uint32)            # +0 -0 | 1 | -0 NaN inf | -NaN
    assert X.expected(keys, z, E.F32, "min")[2].tolist() == [sign, 0x3F800000, sign, qnan | sign | 1]   # -0.0 is below +0.0
    assert X.expected(keys, z, E.F32, "max")[2].tolist() == [0, 0x3F800000, qnan, qnan | sign | 1]      # a +NaN is the maximum
    k2 = np.array([1, 1, 1], np.uint64)
    z2 = np.array([0xFFC00000, 0xFF800000, 0x7FC00001], np.uint32)                                      # -NaN, -inf, +NaN: 8-byte keys, 4-byte values
    assert X.expected(k2, z2, E.F32, "min")[2].tolist() == [0xFFC00000] and X.expected(k2, z2, E.F32, "max")[2].tolist() == [0x7FC00001]
    # nothing at all
    m, starts, out = X.expected(keys[:0], v[:0], E.U32, "sum")
    assert m == 0 and starts.tolist() == [0] and out.size == 0
    for vt in X.VAL_TYPES:
        assert X.out_dtype(vt, "sum").__name__ in ("uint64", "int64", "float64") and np.dtype(X.out_dtype(vt, "min")).itemsize == (4 if vt < 3 else 8)
