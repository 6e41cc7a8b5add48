"""Merge of two sorted arrays (include/msd_merge_hip.h: msd_merge_sorted, msd_merge_sorted_limits; MsdContext.merge_sorted /
merge_sorted_limits) without a GPU: the header declares the two functions with the agreed argument lists, the library
exports them, the binding lists them apart from the other surfaces, a null context is refused first, the limits call answers
on the host, the Python wrapper refuses what never needs a device to be refused, and the numpy expectation and the model of
the two kernels in tests/merge_expect.py are what their docstrings say."""
import ctypes as C

import numpy as np
import pytest

import abi_support as A
import merge_expect as M
import sort_rows_expect as E

SIGNATURES = {
    "msd_merge_sorted": ["msd_ctx *ctx", "const void *d_a", "uint64_t n", "const void *d_b", "uint64_t m", "int key_type",
                         "const uint64_t *d_vals_a", "const uint64_t *d_vals_b", "void *d_out", "uint64_t *d_out_vals", "uint64_t *d_out_origin"],
    "msd_merge_sorted_limits": ["int key_bytes", "uint64_t *tile"],
}


def test_header_declares_the_two_functions():
    text, flat = A.header("msd_merge_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    # the header says what is promised about ties and floats, and what is taken on trust
    for word in ("stable", "TRUSTED", "totalOrder", "-0.0", "NaN"):
        assert word in text, word


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_merge_hip.h", "msd_merge_sorted")


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("MERGE_EXPORTS", SIGNATURES, "msd_merge_hip.h", "msd_merge2.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_merge_sorted.argtypes[1:]]
    assert L.msd_merge_sorted(None, *zeros) == -1
    assert L.msd_merge_sorted(None, None, 0, None, 0, 0, None, None, None, None, None) == -1
    assert L.msd_merge_sorted(None, None, 10, None, 10, 9, C.c_void_p(4), None, None, C.c_void_p(4), None) == -1
    p = C.c_void_p(64)
    assert L.msd_merge_sorted(None, p, 1 << 63, p, 1 << 63, 5, p, p, p, p, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_answer_on_the_host():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile = C.c_uint64(0)
        assert L.msd_merge_sorted_limits(kb, C.byref(tile)) == 0
        assert 64 <= tile.value <= 1 << 16                          # (the kernels keep a local index in 16 bits)
    A.check_limits_refusals(L.msd_merge_sorted_limits, 1)


def test_limits_wrapper():
    from inplacemsdradixsort_amd import MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        tile = C.c_uint64(0)
        assert ctx._L.msd_merge_sorted_limits(kb, C.byref(tile)) == 0
        assert ctx.merge_sorted_limits(kb) == tile.value
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.merge_sorted_limits(kb)


def test_merge_sorted_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    v5, v3 = torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        a, b = torch.zeros(5, dtype=dt), torch.zeros(3, dtype=dt)
        for kw in ({}, {"origin": True}, {"values_a": v5, "values_b": v3}, {"values_a": v5, "values_b": v3, "origin": True},
                   {"out": torch.zeros(8, dtype=dt)}, {"out_origin": torch.zeros(8, dtype=torch.int64)},
                   {"values_a": v5.double(), "values_b": v3.double(), "out_values": torch.zeros(8, dtype=torch.float64)}):
            with pytest.raises(MsdError, match="GPU"):              # CPU tensors
                ctx.merge_sorted(a, b, **kw)
    a, b = torch.zeros(5), torch.zeros(3)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):         # a dtype the library has no order for
            ctx.merge_sorted(a.to(dt), b.to(dt))
    for dt in (torch.float64, torch.int32, torch.int64):
        with pytest.raises(MsdError, match="differ in dtype"):      # differing dtypes
            ctx.merge_sorted(a, b.to(dt))
        with pytest.raises(MsdError, match="differ in dtype"):
            ctx.merge_sorted(a.to(dt), b)
    for bad in (torch.zeros(2, 4), torch.zeros(()), torch.zeros(1, 8)):
        with pytest.raises(MsdError, match="1-D"):                  # not 1-D
            ctx.merge_sorted(bad, b)
        with pytest.raises(MsdError, match="1-D"):
            ctx.merge_sorted(a, bad)
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.merge_sorted(torch.zeros(10)[::2], b)
    with pytest.raises(MsdError, match="contiguous"):
        ctx.merge_sorted(a, torch.zeros(6)[::2])
    with pytest.raises(MsdError, match="contiguous"):
        ctx.merge_sorted(a, b, values_a=torch.zeros(10, dtype=torch.int64)[::2], values_b=v3)
    for kw in ({"values_a": v5}, {"values_b": v3}):
        with pytest.raises(MsdError, match="both or neither"):      # one value tensor without the other
            ctx.merge_sorted(a, b, **kw)
    for va, vb in ((v3, v3), (v5, v5), (torch.zeros(6, dtype=torch.int64), v3)):
        with pytest.raises(MsdError, match="as long as their keys"):   # wrong value lengths
            ctx.merge_sorted(a, b, values_a=va, values_b=vb)
    for va, vb in ((v5.int(), v3.int()), (v5.float(), v3.float()), (v5, v3.double()), (v5.double(), v3),
                   (v5.to(torch.complex64), v3.to(torch.complex64))):
        with pytest.raises(MsdError, match="8-byte elements of one dtype"):   # wrong value widths, differing value dtypes
            ctx.merge_sorted(a, b, values_a=va, values_b=vb)
    with pytest.raises(MsdError, match="1-D"):
        ctx.merge_sorted(a, b, values_a=v5.reshape(5, 1), values_b=v3)
    for out in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32), torch.zeros(7), torch.zeros(9), torch.zeros(2, 4), torch.zeros(16)[::2]):
        with pytest.raises(MsdError, match="out must be"):          # out of the wrong dtype or shape, or not contiguous
            ctx.merge_sorted(a, b, out=out)
    for ov in (torch.zeros(8), torch.zeros(8, dtype=torch.float64), torch.zeros(7, dtype=torch.int64), torch.zeros(16, dtype=torch.int64)[::2]):
        with pytest.raises(MsdError, match="out_values must be"):
            ctx.merge_sorted(a, b, values_a=v5, values_b=v3, out_values=ov)
    with pytest.raises(MsdError, match="out_values without"):
        ctx.merge_sorted(a, b, out_values=torch.zeros(8, dtype=torch.int64))
    for oo in (torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(9, dtype=torch.int64), torch.zeros(4, 2, dtype=torch.int64)):
        with pytest.raises(MsdError, match="out_origin must be"):
            ctx.merge_sorted(a, b, out_origin=oo)
        with pytest.raises(MsdError, match="out_origin must be"):
            ctx.merge_sorted(a, b, origin=True, out_origin=oo)


def test_the_docstring_says_what_is_promised():
    from inplacemsdradixsort_amd import MsdContext
    d = MsdContext.merge_sorted.__doc__
    for word in ("stable", "A's come before all of B's", "bit-exact", "totalOrder", "-0.0", "NaN", "not modified", "Nothing waits on the host"):
        assert word in d, word
    assert "tile" in MsdContext.merge_sorted_limits.__doc__


def test_the_expectation_on_worked_examples():
    # duplicates across both sides: A before B among equals, each side in its own order
    a = np.array([1, 3, 3, 7, 9], np.uint32)
    b = np.array([0, 3, 3, 9, 9, 10], np.uint32)
    merged, origin = M.expected(a, b, E.U32)
    assert merged.tolist() == [0, 1, 3, 3, 3, 3, 7, 9, 9, 9, 10]
    assert origin.tolist() == [5, 0, 1, 2, 6, 7, 3, 4, 8, 9, 10]
    assert origin.dtype == np.uint64 and merged.dtype == np.uint32
    # signed keys across zero: the bits of a negative number are large unsigned numbers
    sa = np.array([-5, -1, 0, 2], np.int32).view(np.uint32)
    sb = np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1], np.int32).view(np.uint32)
    merged, origin = M.expected(sa, sb, E.I32)
    assert merged.view(np.int32).tolist() == [-(1 << 31), -5, -1, -1, 0, 0, 1, 2, (1 << 31) - 1]
    assert origin.tolist() == [4, 0, 1, 5, 2, 6, 7, 3, 8]
    s64 = np.array([-5, 0], np.int64).view(np.uint64)
    merged, origin = M.expected(s64, np.array([-7, 0, 3], np.int64).view(np.uint64), E.I64)
    assert merged.view(np.int64).tolist() == [-7, -5, 0, 0, 3] and origin.tolist() == [2, 0, 1, 3, 4]
    # float32 in totalOrder: -NaN, -inf, -0.0, +0.0, +inf, +NaN; -0.0 from B lands in front of +0.0 from A
    sign, inf, qnan = 0x80000000, 0x7F800000, 0x7FC00000
    fa = np.array([qnan | sign, 0, 0, inf, qnan], np.uint32)              # -NaN +0 +0 +inf +NaN
    fb = np.array([inf | sign, sign, 0, qnan, qnan | 1], np.uint32)       # -inf -0 +0 +NaN +NaN'
    merged, origin = M.expected(fa, fb, E.F32)
    assert merged.tolist() == [qnan | sign, inf | sign, sign, 0, 0, 0, inf, qnan, qnan, qnan | 1]
    assert origin.tolist() == [0, 5, 6, 1, 2, 7, 3, 4, 8, 9]
    # n = 0 and m = 0
    for kt in M.KEY_TYPES:
        ut = E.UT[kt]
        x = np.array([0, 5, 9], ut)
        for a, b in ((x[:0], x), (x, x[:0])):
            merged, origin = M.expected(a, b, kt)
            assert merged.tolist() == [0, 5, 9] and origin.tolist() == [0, 1, 2]
        merged, origin = M.expected(x[:0], x[:0], kt)
        assert merged.size == 0 and origin.size == 0 and merged.dtype == ut
    for a, b in ((np.array([2, 1], np.uint32), np.array([1, 2], np.uint32)), (np.array([1, 2], np.uint32), np.array([2, 1], np.uint32))):
        with pytest.raises(AssertionError):
            M.expected(a, b, E.U32)                                 # inputs that are not ascending are no expectation
    with pytest.raises(AssertionError):
        M.expected(np.array([0, 0x80000000], np.uint32), a[:0], E.I32)   # ... in the order of the TYPE


@pytest.mark.parametrize("distinct", [1, 2, 5, 50])
def test_the_tile_model_writes_every_position_once_and_gives_the_expectation(distinct):
    rng = np.random.default_rng(distinct)
    for trial in range(150):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        a = np.sort(rng.integers(0, distinct, n).astype(np.uint32))
        b = np.sort(rng.integers(0, distinct, m).astype(np.uint32))
        want, want_origin = M.expected(a, b, E.U32)
        for tile in (1, 3, 8, 16):
            merged, origin = M.tiles(a, b, tile)                    # (every position exactly once: the model asserts it)
            assert (merged == want).all() and (origin == want_origin).all(), (n, m, tile)


def test_the_tile_model_with_tiles_of_one_side_only():
    a = np.array([3] * 10, np.uint32)
    b = np.array([3] * 20, np.uint32)
    merged, origin = M.tiles(a, b, 4)
    assert (merged == 3).all() and origin.tolist() == list(range(30))   # all of A, then all of B: stability shows in origin only
