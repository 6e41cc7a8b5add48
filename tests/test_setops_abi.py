"""Set operations on two sorted arrays (include/msd_setops_hip.h: msd_set_sorted, msd_set_sorted_limits; MsdContext.set_sorted /
set_sorted_limits / intersect1d / union1d / setdiff1d / setxor1d) without a GPU: the header declares the two functions with
the agreed argument lists, the library exports them, the binding lists them apart from the other surfaces, a null context is
refused first, the limits call answers on the host, the Python wrapper refuses what never needs a device to be refused, and
the numpy expectation and the model of the kernels in tests/set_expect.py are what their docstrings say."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
import set_expect as X
import sort_rows_expect as E

SIGNATURES = {
    "msd_set_sorted": ["msd_ctx *ctx", "int op", "const void *d_a", "uint64_t n", "const void *d_b", "uint64_t m", "int key_type", "uint64_t cap", "void *d_out",
                       "uint64_t *d_out_origin", "uint64_t *d_num_out"],
    "msd_set_sorted_limits": ["int key_bytes", "uint64_t *tile", "uint64_t *scan_tile"],
}
OPS = ("intersection", "union", "difference", "symmetric_difference")


def test_header_declares_the_two_functions():
    text, flat = A.header("msd_setops_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    for name, value in (("MSD_SET_INTERSECTION", 0), ("MSD_SET_UNION", 1), ("MSD_SET_DIFFERENCE", 2), ("MSD_SET_SYMMETRIC_DIFFERENCE", 3)):
        assert re.search(r"#define %s %d\b" % (name, value), flat), name
        assert getattr(X, name[len("MSD_SET_"):]) == value
    # the header says what is promised about equality and floats, what is taken on trust, and what the origin names
    for word in ("TRUSTED", "totalOrder", "-0.0", "NaN", "first occurrence"):
        assert word in text, word
    # ... and names the other surfaces by their header files only (their ABI tests look for these strings in include/)
    for word in ("msd_merge_sorted", "msd_search", "msd_reduce"):
        assert word not in text, word


def test_the_other_headers_declare_none_of_it():
    A.check_no_other_header_has("msd_setops_hip.h", "msd_set_sorted")


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("SETOPS_EXPORTS", SIGNATURES, "msd_setops_hip.h", "msd_setops.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_set_sorted.argtypes[1:]]
    assert L.msd_set_sorted(None, *zeros) == -1
    assert L.msd_set_sorted(None, 0, None, 0, None, 0, 0, 0, None, None, None) == -1
    assert L.msd_set_sorted(None, 9, None, 10, None, 10, 9, 5, C.c_void_p(4), None, None) == -1
    p = C.c_void_p(64)
    assert L.msd_set_sorted(None, 3, p, 1 << 63, p, 1 << 63, 5, 1 << 63, p, p, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits_answer_on_the_host():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kb in (4, 8):
        tile, scan, merge_tile = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert L.msd_set_sorted_limits(kb, C.byref(tile), C.byref(scan)) == 0
        assert 64 <= tile.value < 0xFFFF                            # (the kernels keep a local index in 16 bits, all ones apart)
        assert scan.value >= 64
        assert L.msd_merge_sorted_limits(kb, C.byref(merge_tile)) == 0 and merge_tile.value == tile.value   # the merge's splits
    A.check_limits_refusals(L.msd_set_sorted_limits, 2, bad_widths=(0, 2, 5, 16, -4))


def test_limits_wrapper():
    from inplacemsdradixsort_amd import MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for kb in (4, 8):
        tile, scan = C.c_uint64(0), C.c_uint64(0)
        assert ctx._L.msd_set_sorted_limits(kb, C.byref(tile), C.byref(scan)) == 0
        assert ctx.set_sorted_limits(kb) == (tile.value, scan.value)
    for kb in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.set_sorted_limits(kb)


def test_set_sorted_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        a, b = torch.zeros(5, dtype=dt), torch.zeros(3, dtype=dt)
        for op in OPS:
            for kw in ({}, {"origin": True}, {"cap": 2}, {"cap": 0, "origin": True}, {"cap": 4, "out": torch.zeros(4, dtype=dt)},
                       {"cap": 4, "out_origin": torch.zeros(4, dtype=torch.int64)}):
                with pytest.raises(MsdError, match="GPU"):          # CPU tensors
                    ctx.set_sorted(a, b, op, **kw)
        for f in (ctx.intersect1d, ctx.union1d, ctx.setdiff1d, ctx.setxor1d):
            with pytest.raises(MsdError, match="GPU"):
                f(a, b)
    a, b = torch.zeros(5), torch.zeros(3)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):         # a dtype the library has no order for
            ctx.set_sorted(a.to(dt), b.to(dt), "union")
        with pytest.raises(MsdError, match="no key order"):
            ctx.union1d(a.to(dt), b.to(dt))
    for dt in (torch.float64, torch.int32, torch.int64):
        with pytest.raises(MsdError, match="differ in dtype"):      # differing dtypes
            ctx.set_sorted(a, b.to(dt), "union")
        with pytest.raises(MsdError, match="differ in dtype"):
            ctx.set_sorted(a.to(dt), b, "intersection")
        with pytest.raises(MsdError, match="differ in dtype"):
            ctx.setdiff1d(a.to(dt), b)
    for bad in (torch.zeros(2, 4), torch.zeros(()), torch.zeros(1, 8)):
        with pytest.raises(MsdError, match="1-D"):                  # not 1-D
            ctx.set_sorted(bad, b, "union")
        with pytest.raises(MsdError, match="1-D"):
            ctx.set_sorted(a, bad, "difference")
        with pytest.raises(MsdError, match="1-D"):
            ctx.setxor1d(a, bad)
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.set_sorted(torch.zeros(10)[::2], b, "union")
    with pytest.raises(MsdError, match="contiguous"):
        ctx.set_sorted(a, torch.zeros(6)[::2], "union")
    for op in ("", "xor", "Union", "intersect", 1, None):
        with pytest.raises(MsdError, match="op must be one of"):    # an unknown op
            ctx.set_sorted(a, b, op)
    for cap in (-1, -100):
        with pytest.raises(MsdError, match="cap must not be negative"):
            ctx.set_sorted(a, b, "union", cap=cap)
    # out has cap elements: by default the bound of the operation (min(n, m), n + m, n, n + m)
    for op, bound in zip(OPS, (3, 8, 5, 8)):
        for out in (torch.zeros(bound, dtype=torch.float64), torch.zeros(bound, dtype=torch.int32), torch.zeros(bound - 1), torch.zeros(bound + 1),
                    torch.zeros(bound, 1), torch.zeros(2 * bound)[::2]):
            with pytest.raises(MsdError, match="out must be"):      # out of the wrong dtype or shape, or not contiguous
                ctx.set_sorted(a, b, op, out=out)
        with pytest.raises(MsdError, match="GPU"):
            ctx.set_sorted(a, b, op, out=torch.zeros(bound))
        with pytest.raises(MsdError, match="out must be"):
            ctx.set_sorted(a, b, op, cap=2, out=torch.zeros(bound))
        for oo in (torch.zeros(bound), torch.zeros(bound, dtype=torch.int32), torch.zeros(bound + 1, dtype=torch.int64), torch.zeros(bound, 1, dtype=torch.int64)):
            with pytest.raises(MsdError, match="out_origin must be"):
                ctx.set_sorted(a, b, op, out_origin=oo)
            with pytest.raises(MsdError, match="out_origin must be"):
                ctx.set_sorted(a, b, op, origin=True, out_origin=oo)


def test_the_docstrings_say_what_is_promised():
    from inplacemsdradixsort_amd import MsdContext
    d = MsdContext.set_sorted.__doc__
    for word in ("trusted", "bit-exact", "totalOrder", "-0.0", "NaN", "first occurrence", "not modified", "Nothing waits on the host"):
        assert word in d, word
    assert "tile" in MsdContext.set_sorted_limits.__doc__
    for f in (MsdContext.intersect1d, MsdContext.union1d, MsdContext.setdiff1d, MsdContext.setxor1d):
        for word in ("UNSORTED", "-0.0", "NaN", "numpy"):           # where the bitwise equality differs from numpy's
            assert word in f.__doc__, (f.__name__, word)
    assert sorted(MsdContext.SET_OPS) == sorted(OPS)
    assert [MsdContext.SET_OPS[X.OP_NAMES[op]] for op in X.OPS] == list(X.OPS)


def _all(a, b, kt):
    return [[r.tolist() for r in X.expected(a, b, kt, op)] for op in X.OPS]    # intersection, union, difference, symmetric difference


def test_the_expectation_on_worked_examples():
    # duplicates on both sides: every value once, the origin names its first occurrence, in A where A holds it
    a = np.array([1, 3, 3, 7, 9], np.uint32)
    b = np.array([0, 3, 3, 9, 9, 10], np.uint32)
    inter, union, diff, xor = _all(a, b, E.U32)
    assert inter == [[3, 9], [1, 4]]
    assert union == [[0, 1, 3, 7, 9, 10], [5, 0, 1, 3, 4, 10]]
    assert diff == [[1, 7], [0, 3]]
    assert xor == [[0, 1, 7, 10], [5, 0, 3, 10]]
    keys, origin = X.expected(a, b, E.U32, X.UNION)
    assert origin.dtype == np.uint64 and keys.dtype == np.uint32
    # signed keys across zero: the bits of a negative number are large unsigned numbers
    sa = np.array([-5, -1, -1, 0, 2], np.int32).view(np.uint32)
    sb = np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1], np.int32).view(np.uint32)
    signed = lambda r: np.array(r[0], np.uint32).view(np.int32).tolist()
    inter, union, diff, xor = _all(sa, sb, E.I32)
    assert signed(inter) == [-1, 0] and inter[1] == [1, 3]
    assert signed(union) == [-(1 << 31), -5, -1, 0, 1, 2, (1 << 31) - 1] and union[1] == [5, 0, 1, 3, 8, 4, 9]
    assert signed(diff) == [-5, 2] and diff[1] == [0, 4]
    assert signed(xor) == [-(1 << 31), -5, 1, 2, (1 << 31) - 1] and xor[1] == [5, 0, 8, 4, 9]
    s64a, s64b = np.array([-5, 0], np.int64).view(np.uint64), np.array([-7, 0, 3], np.int64).view(np.uint64)
    keys, origin = X.expected(s64a, s64b, E.I64, X.UNION)
    assert keys.view(np.int64).tolist() == [-7, -5, 0, 3] and origin.tolist() == [2, 0, 1, 4]
    # float32: -0.0 only in B, +0.0 only in A: both survive a union and neither an intersection
    sign, inf, qnan = 0x80000000, 0x7F800000, 0x7FC00000
    fa = np.array([0, 0, inf], np.uint32)                           # +0 +0 +inf
    fb = np.array([inf | sign, sign, inf], np.uint32)               # -inf -0 +inf
    inter, union, diff, xor = _all(fa, fb, E.F32)
    assert inter == [[inf], [2]]
    assert union == [[inf | sign, sign, 0, inf], [3, 4, 0, 2]]
    assert diff == [[0], [0]]
    assert xor == [[inf | sign, sign, 0], [3, 4, 0]]
    # equal NaNs intersect; NaNs of different payload or sign do not
    na = np.array([qnan | sign, 1, qnan, qnan | 5], np.uint32)      # -NaN 1e-45 +NaN +NaN'
    nb = np.array([1, qnan, qnan, qnan | 6], np.uint32)             #      1e-45 +NaN +NaN +NaN''
    inter, union, diff, xor = _all(na, nb, E.F32)
    assert inter == [[1, qnan], [1, 2]]
    assert union == [[qnan | sign, 1, qnan, qnan | 5, qnan | 6], [0, 1, 2, 3, 7]]
    assert diff == [[qnan | sign, qnan | 5], [0, 3]]
    assert xor == [[qnan | sign, qnan | 5, qnan | 6], [0, 3, 7]]
    # n = 0 and m = 0
    for kt in X.KEY_TYPES:
        ut = E.UT[kt]
        x = np.array([0, 5, 5, 9], ut)
        distinct = [[0, 5, 9], [0, 1, 3]]
        none = [[], []]
        assert _all(x[:0], x, kt) == [none, distinct, none, distinct]
        assert _all(x, x[:0], kt) == [none, distinct, distinct, distinct]
        assert _all(x[:0], x[:0], kt) == [none] * 4
        assert X.expected(x[:0], x[:0], kt, X.UNION)[0].dtype == ut
    for a, b in ((np.array([2, 1], np.uint32), np.array([1, 2], np.uint32)), (np.array([1, 2], np.uint32), np.array([2, 1], np.uint32))):
        with pytest.raises(AssertionError):
            X.expected(a, b, E.U32, X.UNION)                        # inputs that are not ascending are no expectation
    with pytest.raises(AssertionError):
        X.expected(np.array([0, 0x80000000], np.uint32), a[:0], E.I32, X.UNION)   # ... in the order of the TYPE
    assert [X.bound(op, 5, 3) for op in X.OPS] == [3, 8, 5, 8] and [X.bound(op, 2, 7) for op in X.OPS] == [2, 9, 2, 9]


@pytest.mark.parametrize("distinct", [1, 2, 5, 50])
def test_the_tile_model_reads_tile_and_halo_only_and_gives_the_expectation(distinct):
    rng = np.random.default_rng(distinct)
    for trial in range(150):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        a = np.sort(rng.integers(0, distinct, n).astype(np.uint32))
        b = np.sort(rng.integers(0, distinct, m).astype(np.uint32))
        for op in X.OPS:
            want, want_origin = X.expected(a, b, E.U32, op)
            for tile in (1, 3, 8, 16):
                keys, origin = X.tiles(a, b, tile, op)              # (every read inside the tile or its halo: the model asserts it)
                assert keys.tolist() == want.tolist() and origin.tolist() == want_origin.tolist(), (n, m, tile, op)


def test_the_tile_model_with_runs_and_matches_across_tile_edges():
    a = np.array([3] * 10 + [4], np.uint32)
    b = np.array([3] * 20 + [5], np.uint32)
    for tile in (1, 4, 7):
        assert [X.tiles(a, b, tile, op)[0].tolist() for op in X.OPS] == [[3], [3, 4, 5], [4], [4, 5]]
        assert [X.tiles(a, b, tile, op)[1].tolist() for op in X.OPS] == [[0], [0, 10, 31], [10], [10, 31]]
