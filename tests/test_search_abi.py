"""Sorted search (include/msd_search_hip.h: msd_search_sorted, msd_search_sorted_limits; MsdContext.searchsorted / bucketize /
search_sorted_limits) without a GPU: the header declares the two functions with the agreed argument lists and the two sides,
the library exports them, the binding lists them apart from the other surfaces, a null context is refused first, the limits
call answers on the host, the Python wrappers refuse what never needs a device to be refused, and the numpy expectation and
the model of the merge path's decomposition in tests/search_expect.py are what their docstrings say."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
import search_expect as S
import sort_rows_expect as E

SIGNATURES = {
    "msd_search_sorted": ["msd_ctx *ctx", "const void *d_sorted", "int key_type", "uint64_t n", "const void *d_needles", "uint64_t m",
                          "int needles_sorted", "int side", "const uint64_t *d_positions", "uint64_t *d_out"],
    "msd_search_sorted_limits": ["int key_bytes", "uint64_t *tile", "uint64_t *direct_tile"],
}


def test_header_declares_the_two_functions_and_the_sides():
    text, flat = A.header("msd_search_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    assert re.search(r"enum \{ MSD_SEARCH_LEFT = 0, MSD_SEARCH_RIGHT = 1 \};", flat)
    # the header says where the order differs from torch, and what is taken on trust
    for word in ("torch.searchsorted", "-0.0", "NaN", "totalOrder", "TRUSTED"):
        assert word in text, word


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_search_hip.h", "msd_search", headers=("msd_radix_hip.h", "msd_runs_hip.h", "msd_reduce_hip.h"))


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("SEARCH_EXPORTS", SIGNATURES, "msd_search_hip.h", "msd_search.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_search_sorted.argtypes[1:]]
    assert L.msd_search_sorted(None, *zeros) == -1
    assert L.msd_search_sorted(None, None, 0, 0, None, 0, 0, 0, None, None) == -1
    assert L.msd_search_sorted(None, None, 9, 10, None, 10, 7, 3, C.c_void_p(4), None) == -1
    p = C.c_void_p(64)
    assert L.msd_search_sorted(None, p, 5, 1 << 63, p, 1 << 63, 1, 1, p, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_answer_on_the_host():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile, direct = C.c_uint64(0), C.c_uint64(0)
        assert L.msd_search_sorted_limits(kb, C.byref(tile), C.byref(direct)) == 0
        assert tile.value >= 64 and direct.value >= 64
    A.check_limits_refusals(L.msd_search_sorted_limits, 2, bad_widths=(0, 2, 16, -4, 5))


def test_limits_wrapper():
    from inplacemsdradixsort_amd import MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        tile, direct = C.c_uint64(0), C.c_uint64(0)
        assert ctx._L.msd_search_sorted_limits(kb, C.byref(tile), C.byref(direct)) == 0
        assert ctx.search_sorted_limits(kb) == (tile.value, direct.value)
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.search_sorted_limits(kb)


def test_searchsorted_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for kw in ({}, {"right": True}, {"needles_sorted": True}, {"sort_needles": True}, {"positions": torch.arange(6)},
                   {"out": torch.zeros(2, 3, dtype=torch.int64)}):
            with pytest.raises(MsdError, match="GPU"):              # CPU tensors
                ctx.searchsorted(torch.zeros(8, dtype=dt), torch.zeros(2, 3, dtype=dt), **kw)
        with pytest.raises(MsdError, match="GPU"):
            ctx.bucketize(torch.zeros(2, 3, dtype=dt), torch.zeros(8, dtype=dt))
    k, x = torch.zeros(8), torch.zeros(2, 3)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):         # a dtype the library has no order for
            ctx.searchsorted(k.to(dt), x.to(dt))
    for dt in (torch.float64, torch.int32, torch.int64):
        with pytest.raises(MsdError, match="differ in dtype"):      # differing dtypes
            ctx.searchsorted(k, x.to(dt))
        with pytest.raises(MsdError, match="differ in dtype"):
            ctx.bucketize(x.to(dt), k)
    for bad in (torch.zeros(2, 4), torch.zeros(()), torch.zeros(1, 8)):
        with pytest.raises(MsdError, match="1-D"):                  # sorted_keys that is not 1-D
            ctx.searchsorted(bad, x)
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.searchsorted(torch.zeros(16)[::2], x)
    with pytest.raises(MsdError, match="contiguous"):
        ctx.searchsorted(k, torch.zeros(3, 2).t())
    for pos in (torch.zeros(6, dtype=torch.int32), torch.zeros(6), torch.zeros(5, dtype=torch.int64), torch.zeros(7, dtype=torch.int64),
                torch.zeros(2, 3, dtype=torch.int64), torch.zeros(12, dtype=torch.int64)[::2]):
        with pytest.raises(MsdError, match="positions must be"):    # positions of the wrong dtype, length or shape
            ctx.searchsorted(k, x, positions=pos)
    with pytest.raises(MsdError, match="positions together with sort_needles"):
        ctx.searchsorted(k, x, positions=torch.arange(6), sort_needles=True)
    for out in (torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), torch.zeros(6, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64),
                torch.zeros(3, 2, dtype=torch.int64).t()):
        with pytest.raises(MsdError, match="out must be"):          # out of the wrong dtype or shape, or not contiguous
            ctx.searchsorted(k, x, out=out)


def test_the_docstrings_say_where_the_results_differ_from_torch():
    from inplacemsdradixsort_amd import MsdContext
    d = MsdContext.searchsorted.__doc__
    for word in ("torch.searchsorted", "-0.0", "NaN", "totalOrder", "not modified", "sort_needles"):
        assert word in d, word
    b = MsdContext.bucketize.__doc__
    assert "torch.bucketize" in b and "-0.0" in b and "NaN" in b
    o = MsdContext.set_option.__doc__
    assert "search_mode" in o and "search_merge_ratio" in o


def test_the_expectation_on_worked_examples():
    # LEFT and RIGHT on duplicates
    keys = np.array([1, 3, 3, 3, 7, 9, 9], np.uint32)
    x = np.array([0, 1, 2, 3, 4, 7, 8, 9, 10, 0xFFFFFFFF], np.uint32)
    assert S.expected(keys, x, E.U32, False).tolist() == [0, 0, 1, 1, 4, 4, 5, 5, 7, 7]
    assert S.expected(keys, x, E.U32, True).tolist() == [0, 1, 1, 4, 4, 5, 5, 7, 7, 7]
    assert S.expected(keys, x, E.U32, True).dtype == np.uint64
    # signed keys across zero: the bits of a negative number are large unsigned numbers
    sk = np.array([-5, -1, 0, 0, 2], np.int32).view(np.uint32)
    sx = np.array([-6, -5, -1, 0, 1, 2, 3, -(1 << 31), (1 << 31) - 1], np.int32).view(np.uint32)
    assert S.expected(sk, sx, E.I32, False).tolist() == [0, 0, 1, 2, 4, 4, 5, 0, 5]
    assert S.expected(sk, sx, E.I32, True).tolist() == [0, 1, 2, 4, 4, 5, 5, 0, 5]
    s64 = np.array([-5, -1, 0, 0, 2], np.int64).view(np.uint64)
    assert S.expected(s64, np.array([-1, 0], np.int64).view(np.uint64), E.I64, True).tolist() == [2, 4]
    # float32 in totalOrder: -NaN, -inf, -0.0, +0.0, +inf, +NaN
    sign, inf, qnan = 0x80000000, 0x7F800000, 0x7FC00000
    fk = np.array([qnan | sign, inf | sign, sign, sign, 0, 0x3F800000, inf, qnan], np.uint32)
    assert (S.sort_by_code(fk[::-1].copy(), E.F32) == fk).all()
    fx = np.array([0, sign, qnan, qnan | sign, inf, inf | sign, qnan | 1, qnan | sign | 1, 0x3F800000], np.uint32)
    #                +0  -0   +NaN  -NaN       +inf  -inf       +NaN'     -NaN'           1.0
    assert S.expected(fk, fx, E.F32, False).tolist() == [4, 2, 7, 0, 6, 1, 8, 0, 5]   # LEFT of +0.0 points behind the -0.0s
    assert S.expected(fk, fx, E.F32, True).tolist() == [5, 4, 8, 1, 7, 2, 8, 0, 6]    # a NaN with a larger payload lies further out
    # n = 0 and m = 0
    for kt in S.KEY_TYPES:
        ut = E.UT[kt]
        assert S.expected(np.zeros(0, ut), np.array([0, 5, (1 << 31)], ut), kt, False).tolist() == [0, 0, 0]
        assert S.expected(np.zeros(0, ut), np.array([0, 5, (1 << 31)], ut), kt, True).tolist() == [0, 0, 0]
        assert S.expected(np.array([1, 2], ut), np.zeros(0, ut), kt, True).size == 0
    with pytest.raises(AssertionError):
        S.expected(np.array([2, 1], np.uint32), x, E.U32, False)    # keys that are not ascending are no expectation


@pytest.mark.parametrize("distinct", [1, 2, 5, 50])
def test_the_split_model_partitions_the_needles_and_gives_the_expectation(distinct):
    rng = np.random.default_rng(distinct)
    for trial in range(120):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        a = np.sort(rng.integers(0, distinct, n).astype(np.uint32))
        b = np.sort(rng.integers(0, distinct, m).astype(np.uint32))
        for tile in (1, 3, 8, 16):
            for right in (False, True):
                sa, sb, got = S.splits(a, b, tile, right)
                tiles = -(-(n + m) // tile)
                assert len(sa) == len(sb) == tiles + 1 and sa[0] == sb[0] == 0 and sa[-1] == n and sb[-1] == m
                for i in range(tiles):
                    na, nb = sa[i + 1] - sa[i], sb[i + 1] - sb[i]
                    assert na >= 0 and nb >= 0 and na + nb <= tile, (n, m, tile, right, i)
                assert (got >= 0).all(), "a needle no tile wrote"          # (none twice: the model asserts it)
                assert (got.astype(np.uint64) == S.expected(a, b, E.U32, right)).all(), (n, m, tile, right)


def test_the_split_model_with_tiles_of_needles_only_and_of_keys_only():
    a = np.array([3] * 10, np.uint32)
    b = np.array([3] * 20, np.uint32)
    for right in (False, True):
        sa, sb, got = S.splits(a, b, 4, right)
        assert any(sa[i + 1] == sa[i] and sb[i + 1] - sb[i] == 4 for i in range(len(sa) - 1))     # needles only
        assert any(sb[i + 1] == sb[i] and sa[i + 1] - sa[i] == 4 for i in range(len(sa) - 1))     # keys only
        assert (got == (10 if right else 0)).all()
