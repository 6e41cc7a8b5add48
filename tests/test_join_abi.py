"""Sort-merge join of two sorted arrays (include/msd_join_hip.h: msd_join_groups, msd_join_pairs, msd_join_limits;
MsdContext.join_groups / join_pairs / join / join_limits) without a GPU: the header declares the three functions with the
agreed argument lists, the other headers declare none of it, the library exports them, the binding lists them apart from the
other surfaces, a null context is refused first, the limits call answers on the host, the Python wrappers refuse what never
needs a device to be refused, and the numpy expectation and the model of the write kernel in tests/join_expect.py are what
their docstrings say."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
import join_expect as J
import sort_rows_expect as E

SIGNATURES = {
    "msd_join_groups": ["msd_ctx *ctx", "const void *d_a", "uint64_t n", "const void *d_b", "uint64_t m", "int key_type", "uint64_t cap", "void *d_keys",
                        "uint64_t *d_a_first", "uint64_t *d_a_count", "uint64_t *d_b_first", "uint64_t *d_b_count", "uint64_t *d_num_groups"],
    "msd_join_pairs": ["msd_ctx *ctx", "uint64_t groups_cap", "const uint64_t *d_num_groups", "const uint64_t *d_a_first", "const uint64_t *d_a_count",
                       "const uint64_t *d_b_first", "const uint64_t *d_b_count", "uint64_t n", "uint64_t m", "const uint64_t *d_pos_a", "const uint64_t *d_pos_b",
                       "uint64_t cap", "uint64_t *d_out_a", "uint64_t *d_out_b", "uint64_t *d_num_pairs"],
    "msd_join_limits": ["int key_bytes", "uint64_t *tile", "uint64_t *scan_tile", "uint64_t *pair_tile"],
}


def test_header_declares_the_three_functions():
    text, flat = A.header("msd_join_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    # the header says what is promised about equality and floats, what is taken on trust, the order of the pairs, what a
    # truncated groups call means, and the order of the refusals
    for word in ("TRUSTED", "totalOrder", "-0.0", "NaN", "first occurrence", "lexicographic", "TRUNCATED", "checked in this order", "2^32", "join_groups", "join_pairs"):
        assert word in text, word
    # ... and names the other surfaces by their header files only (their ABI tests look for these strings in include/)
    for word in ("msd_set_sorted", "msd_merge_sorted", "msd_search", "msd_reduce"):
        assert word not in text, word


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_join_hip.h", "msd_join")


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("JOIN_EXPORTS", SIGNATURES, "msd_join_hip.h", "msd_join.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    p = C.c_void_p(64)
    for f in (L.msd_join_groups, L.msd_join_pairs):
        zeros = [t() for t in f.argtypes[1:]]
        assert f(None, *zeros) == -1
    assert L.msd_join_groups(None, None, 10, None, 10, 9, 5, C.c_void_p(4), None, None, None, None, None) == -1
    assert L.msd_join_groups(None, p, 1 << 63, p, 1 << 63, 5, 1 << 63, p, p, p, p, p, p) == -1
    assert L.msd_join_pairs(None, 7, None, None, None, None, None, 1 << 40, 1 << 40, C.c_void_p(4), None, 9, None, None, None) == -1
    assert L.msd_join_pairs(None, 1 << 63, p, p, p, p, p, 1 << 63, 1 << 63, p, p, 1 << 63, p, p, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_answer_on_the_host():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile, scan, pair, set_tile, set_scan = (C.c_uint64(0) for _ in range(5))
        assert L.msd_join_limits(kb, C.byref(tile), C.byref(scan), C.byref(pair)) == 0
        assert 64 <= tile.value < 0xFFFF                            # (the kernels keep a local index in 16 bits, all ones apart)
        assert scan.value >= 64 and pair.value >= 64
        assert L.msd_set_sorted_limits(kb, C.byref(set_tile), C.byref(set_scan)) == 0
        assert (set_tile.value, set_scan.value) == (tile.value, scan.value)   # the tiles and the scan of the set operations
    A.check_limits_refusals(L.msd_join_limits, 3)


def test_limits_wrapper():
    from inplacemsdradixsort_amd import MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        t, s, p = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert ctx._L.msd_join_limits(kb, C.byref(t), C.byref(s), C.byref(p)) == 0
        assert ctx.join_limits(kb) == (t.value, s.value, p.value)
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.join_limits(kb)


def test_the_wrappers_refuse_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        a, b = torch.zeros(5, dtype=dt), torch.zeros(3, dtype=dt)
        for kw in ({}, {"cap": 2}, {"cap": 0}, {"keys": False}):
            with pytest.raises(MsdError, match="GPU"):              # CPU tensors
                ctx.join_groups(a, b, **kw)
        with pytest.raises(MsdError, match="GPU"):
            ctx.join(a, b)
    a, b = torch.zeros(5), torch.zeros(3)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        for f in (ctx.join_groups, ctx.join):
            with pytest.raises(MsdError, match="no key order"):     # a dtype the library has no order for
                f(a.to(dt), b.to(dt))
    for dt in (torch.float64, torch.int32, torch.int64):
        for f in (ctx.join_groups, ctx.join):
            with pytest.raises(MsdError, match="differ in dtype"):  # differing dtypes
                f(a, b.to(dt))
            with pytest.raises(MsdError, match="differ in dtype"):
                f(a.to(dt), b)
    for bad in (torch.zeros(2, 4), torch.zeros(()), torch.zeros(1, 8)):
        for f in (ctx.join_groups, ctx.join):
            with pytest.raises(MsdError, match="1-D"):              # not 1-D
                f(bad, b)
            with pytest.raises(MsdError, match="1-D"):
                f(a, bad)
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.join_groups(torch.zeros(10)[::2], b)
    with pytest.raises(MsdError, match="contiguous"):
        ctx.join_groups(a, torch.zeros(6)[::2])
    for cap in (-1, -100):
        with pytest.raises(MsdError, match="cap must not be negative"):
            ctx.join_groups(a, b, cap=cap)
    # join_pairs: the groups, the positions and the outputs
    i64 = lambda count: torch.zeros(count, dtype=torch.int64)
    good = (i64(1), None, i64(3), i64(3), i64(3), i64(3))
    with pytest.raises(MsdError, match="GPU"):
        ctx.join_pairs(good, 5, 3, 4)
    for at in (2, 3, 4, 5):
        for bad in (i64(4), torch.zeros(3, dtype=torch.int32), torch.zeros(3), i64(6)[::2], torch.zeros(3, 1, dtype=torch.int64)):
            g = list(good)
            g[at] = bad
            with pytest.raises(MsdError, match="groups must be"):
                ctx.join_pairs(tuple(g), 5, 3, 4)
    for bad in (i64(2), torch.zeros(1, dtype=torch.int32)):
        with pytest.raises(MsdError, match="num_groups must be"):
            ctx.join_pairs((bad,) + good[1:], 5, 3, 4)
    for kw in ({"n": -1}, {"m": -1}, {"cap": -1}):
        with pytest.raises(MsdError, match="must not be negative"):
            ctx.join_pairs(good, **dict(dict(n=5, m=3, cap=4), **kw))
    for bad in (i64(4), i64(6), torch.zeros(5, dtype=torch.int32), i64(10)[::2], torch.zeros(5, 1, dtype=torch.int64)):
        with pytest.raises(MsdError, match="positions_a must be"):
            ctx.join_pairs(good, 5, 3, 4, positions_a=bad)
    for bad in (i64(2), i64(5), torch.zeros(3), i64(6)[::2]):
        with pytest.raises(MsdError, match="positions_b must be"):
            ctx.join_pairs(good, 5, 3, 4, positions_b=bad)
    for bad in (i64(3), i64(5), torch.zeros(4, dtype=torch.int32), torch.zeros(4), i64(8)[::2], torch.zeros(4, 1, dtype=torch.int64)):
        with pytest.raises(MsdError, match="out_a must be"):        # out of the wrong dtype or length, or not contiguous
            ctx.join_pairs(good, 5, 3, 4, out_a=bad)
        with pytest.raises(MsdError, match="out_b must be"):
            ctx.join_pairs(good, 5, 3, 4, out_b=bad)
    with pytest.raises(MsdError, match="GPU"):
        ctx.join_pairs(good, 5, 3, 4, positions_a=i64(5), positions_b=i64(3), out_a=i64(4), out_b=i64(4))


def test_the_docstrings_say_what_is_promised():
    from inplacemsdradixsort_amd import MsdContext
    flat = lambda f: re.sub(r"\s+", " ", f.__doc__)
    d = flat(MsdContext.join_groups)
    for word in ("trusted", "bit-exact", "totalOrder", "-0.0", "NaN", "first occurrence", "not modified", "Nothing waits on the host", "intersection"):
        assert word in d, word
    d = flat(MsdContext.join_pairs)
    for word in ("lexicographic", "truncated", "positions_a", "only counts", "Nothing waits on the host"):
        assert word in d, word
    d = flat(MsdContext.join)
    for word in ("UNSORTED", "-0.0", "NaN", "not modified", "One host wait"):
        assert word in d, word
    assert "pair" in MsdContext.join_limits.__doc__


def _lists(g):
    return [x.tolist() for x in g]


def test_the_expectation_on_worked_examples():
    a = np.array([1, 3, 3, 7, 9], np.uint32)
    b = np.array([0, 3, 3, 3, 9, 9, 10], np.uint32)
    g = J.groups(a, b, E.U32)
    assert _lists(g) == [[3, 9], [1, 4], [2, 1], [1, 4], [3, 2]]
    assert g[0].dtype == np.uint32 and all(x.dtype == np.uint64 for x in g[1:])
    assert J.total(g) == 8
    ia, ib = J.pairs(g, 0, 100)
    assert ia.tolist() == [1, 1, 1, 2, 2, 2, 4, 4] and ib.tolist() == [1, 2, 3, 1, 2, 3, 4, 5]
    assert [x.tolist() for x in J.pairs(g, 2, 7)] == [[1, 2, 2, 2, 4], [3, 1, 2, 3, 4]]
    assert [x.tolist() for x in J.pairs(g, 8, 9)] == [[], []] and [x.tolist() for x in J.pairs(g, 3, 3)] == [[], []]
    # signed keys across zero: the bits of a negative number are large unsigned numbers
    sa = np.array([-5, -1, -1, 0, 2], np.int32).view(np.uint32)
    sb = np.array([-(1 << 31), -1, 0, 0, (1 << 31) - 1], np.int32).view(np.uint32)
    g = J.groups(sa, sb, E.I32)
    assert g[0].view(np.int32).tolist() == [-1, 0] and _lists(g[1:]) == [[1, 3], [2, 1], [1, 2], [1, 2]]
    # float32: the zeros do not join; equal NaNs do, NaNs of different payload or sign do not
    sign, inf, qnan = 0x80000000, 0x7F800000, 0x7FC00000
    fa = np.array([qnan | sign, 0, 0, inf, qnan, qnan | 5], np.uint32)   # -NaN +0 +0 +inf +NaN +NaN'
    fb = np.array([sign, sign, inf, qnan, qnan, qnan | 6], np.uint32)    # -0 -0 +inf +NaN +NaN +NaN''
    g = J.groups(fa, fb, E.F32)
    assert _lists(g) == [[inf, qnan], [3, 4], [1, 1], [2, 3], [1, 2]]
    # an empty side, and inputs that are no expectation
    for kt in J.KEY_TYPES:
        x = np.array([0, 5, 5, 9], E.UT[kt])
        for p, q in ((x[:0], x), (x, x[:0]), (x[:0], x[:0])):
            g = J.groups(p, q, kt)
            assert _lists(g) == [[]] * 5 and g[0].dtype == E.UT[kt] and J.total(g) == 0
            assert [y.tolist() for y in J.pairs(g, 0, 5)] == [[], []]
        assert _lists(J.groups(x, x, kt)) == [[0, 5, 9], [0, 1, 3], [1, 2, 1], [0, 1, 3], [1, 2, 1]]
    with pytest.raises(AssertionError):
        J.groups(np.array([2, 1], np.uint32), np.array([1, 2], np.uint32), E.U32)
    with pytest.raises(AssertionError):
        J.groups(np.array([1, 2], np.uint32), np.array([0, 0x80000000], np.uint32), E.I32)   # ... in the order of the TYPE


@pytest.mark.parametrize("distinct", [1, 2, 5, 50])
def test_the_tile_model_reads_tile_and_halo_only_and_gives_the_groups(distinct):
    rng = np.random.default_rng(distinct)
    for trial in range(150):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        a = np.sort(rng.integers(0, distinct, n).astype(np.uint32))
        b = np.sort(rng.integers(0, distinct, m).astype(np.uint32))
        want = _lists(J.groups(a, b, E.U32))
        for tile in (1, 3, 8, 16):
            got = J.tiles(a, b, tile)                               # (every read inside the tile or its halo, one search per side: the model asserts it)
            assert _lists(got) == want, (n, m, tile)


def test_the_tile_model_with_runs_across_tile_edges():
    a = np.array([3] * 10 + [4] * 3 + [6], np.uint32)
    b = np.array([3] * 20 + [4] + [5] + [6] * 9, np.uint32)
    for tile in (1, 4, 7, 64):
        assert _lists(J.tiles(a, b, tile)) == [[3, 4, 6], [0, 10, 13], [10, 3, 1], [0, 20, 22], [20, 1, 9]]


def test_pairs_against_a_double_loop():
    rng = np.random.default_rng(12)
    for trial in range(200):
        n, m = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        distinct = int(rng.integers(1, 6))
        a = np.sort(rng.integers(0, distinct, n).astype(np.uint64))
        b = np.sort(rng.integers(0, distinct, m).astype(np.uint64))
        brute = [(i, j) for i in range(n) for j in range(m) if a[i] == b[j]]   # (lexicographic by construction)
        g = J.groups(a, b, E.U64)
        assert J.total(g) == len(brute)
        ia, ib = J.pairs(g, 0, len(brute) + 3)
        assert list(zip(ia.tolist(), ib.tolist())) == brute
        for lo, hi in ((0, 1), (1, 4), (len(brute) // 2, len(brute)), (len(brute), len(brute) + 2)):
            ia, ib = J.pairs(g, lo, hi)
            assert list(zip(ia.tolist(), ib.tolist())) == brute[lo:hi], (lo, hi)
