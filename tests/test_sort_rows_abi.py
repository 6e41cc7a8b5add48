"""The per-row sort (include/msd_sort_rows_hip.h: msd_sort_rows, msd_sort_rows_limits; MsdContext.sort_rows / sort_rows_limits)
without a GPU: the header declares the two functions with the agreed argument lists, the library exports them, the binding
lists them apart from the other surfaces, a null context is refused first, the limits call answers on the host, and the
Python wrapper refuses what never needs a device to be refused."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi_support as A
import sort_rows_expect as E

SIGNATURES = {
    "msd_sort_rows": ["msd_ctx *ctx", "const void *d_keys", "int key_type", "uint64_t rows", "uint64_t row_len", "uint64_t row_stride",
                      "int order", "void *d_out_keys", "uint64_t *d_out_idx"],
    "msd_sort_rows_limits": ["int key_type", "int with_idx", "uint64_t *max_row_len"],
}
# floors on max_row_len, derived from the hardware (key bytes, with positions) -> keys
FLOORS = {(4, False): 24576, (8, False): 17408, (4, True): 16384, (8, True): 8192}


def test_header_declares_the_two_functions():
    _, flat = A.header("msd_sort_rows_hip.h")
    assert '#include "msd_sort_keys_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("SORT_ROWS_EXPORTS", SIGNATURES, "msd_sort_rows_hip.h", "msd_sort_rows.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_sort_rows.argtypes[1:]]
    assert L.msd_sort_rows(None, *zeros) == -1                                   # (would be a no-op: rows == 0)
    assert L.msd_sort_rows(None, None, 2, 0, 0, 0, 0, None, None) == -1
    assert L.msd_sort_rows(None, None, 99, 10, 10, 5, 99, None, None) == -1
    assert L.msd_sort_rows(None, C.c_void_p(64), 0, 1 << 63, 1 << 63, 1 << 63, 1, C.c_void_p(64), None) == -1


def test_limits():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kt in range(6):
        got = {}
        for with_idx in (False, True):
            v = C.c_uint64(0)
            assert L.msd_sort_rows_limits(kt, int(with_idx), C.byref(v)) == 0
            got[with_idx] = int(v.value)
            assert got[with_idx] >= FLOORS[(4 if kt < 3 else 8, with_idx)], (kt, with_idx, got)
        assert got[True] <= got[False], (kt, got)
    v = C.c_uint64(77)
    for kt in (-1, 6, 99):
        assert L.msd_sort_rows_limits(kt, 0, C.byref(v)) == -1 and v.value == 77
    for kt in range(6):
        assert L.msd_sort_rows_limits(kt, 1, None) == -1


def test_stat_names_are_unknown_to_a_null_context():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    v = C.c_uint64(77)
    for name in (b"sort_rows_kernel_rows", b"sort_rows_segment_rows"):
        assert L.msd_stat(None, name, C.byref(v)) == -1 and v.value == 77


def test_sort_rows_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for kw in ({}, {"descending": True}, {"indices": True}):
            with pytest.raises(MsdError):                       # a CPU tensor
                ctx.sort_rows(torch.zeros(4, 8, dtype=dt), **kw)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):     # a dtype without a key order
            ctx.sort_rows(torch.zeros(4, 8).to(dt))
    with pytest.raises(MsdError, match="stride 1"):             # the last dimension is not stride 1
        ctx.sort_rows(torch.zeros(8, 4).t())
    with pytest.raises(MsdError, match="stride 1"):
        ctx.sort_rows(torch.zeros(4, 16)[:, ::2])
    with pytest.raises(MsdError, match="collapse"):             # leading dimensions that do not collapse
        ctx.sort_rows(torch.zeros(4, 6, 8)[:, :3, :])
    x = torch.zeros(4, 8)
    for out in (torch.zeros(4, 7), torch.zeros(8, 4), torch.zeros(32), torch.zeros(8, 4).t()):
        with pytest.raises(MsdError, match="shape"):            # an out of the wrong shape (or not contiguous)
            ctx.sort_rows(x, out=out)
    with pytest.raises(MsdError, match="dtype"):                # ... or dtype
        ctx.sort_rows(x, out=torch.zeros(4, 8, dtype=torch.float64))
    for oi in (torch.zeros(4, 8, dtype=torch.int32), torch.zeros(4, 8)):
        with pytest.raises(MsdError, match="int64"):            # out_indices that is not int64
            ctx.sort_rows(x, out_indices=oi)
    with pytest.raises(MsdError, match="shape"):
        ctx.sort_rows(x, out_indices=torch.zeros(4, 9, dtype=torch.int64))
    with pytest.raises(MsdError, match="GPU"):                  # everything else in order: still a CPU tensor
        ctx.sort_rows(x, out=torch.zeros(4, 8), out_indices=torch.zeros(4, 8, dtype=torch.int64))


def test_limits_wrapper_and_stats_names():
    from inplacemsdradixsort_amd import MsdContext, MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    assert ctx.sort_rows_limits(MsdContext.KEY_F32) >= FLOORS[(4, False)]
    assert ctx.sort_rows_limits(MsdContext.KEY_I64, indices=True) >= FLOORS[(8, True)]
    with pytest.raises(MsdError):
        ctx.sort_rows_limits(17)
    from inplacemsdradixsort_amd import api
    assert "sort_rows_kernel_rows" in api.STAT_NAMES and "sort_rows_segment_rows" in api.STAT_NAMES
    assert "in STAT_NAMES" in inspect.getsource(MsdContext.stats)   # (stats() asks for every name of that tuple)
    doc = MsdContext.set_option.__doc__
    assert "sort_rows_mode" in doc and "sort_rows_lanes" in doc


def test_the_expectation_orders_like_numpy_where_numpy_has_an_order():
    rng = np.random.default_rng(1)
    f = rng.standard_normal((5, 999)).astype(np.float32)
    i = rng.integers(-2**63, 2**63 - 1, (5, 999), dtype=np.int64)
    u = i.view(np.uint64)
    for desc in (False, True):
        flip = (lambda a: np.ascontiguousarray(a[:, ::-1])) if desc else (lambda a: a)
        assert (E.expected(f.view(np.uint32), E.F32, desc) == flip(np.sort(f, axis=1)).view(np.uint32)).all()
        assert (E.expected(i.view(np.uint64), E.I64, desc) == flip(np.sort(i, axis=1)).view(np.uint64)).all()
        assert (E.expected(u, E.U64, desc) == flip(np.sort(u, axis=1))).all()


def test_generated_rows_differ_and_kinds_are_what_they_say():
    a = E.make_rows(6, 999, "normal", E.F32, 1).view(np.float32)
    assert len({a[r].tobytes() for r in range(6)}) == 6
    assert a[0].std() < a[4].std() / 8                      # a scale per row
    s = E.make_rows(3, 5000, "specials", E.F64, 1).view(np.float64)
    assert np.isnan(s).sum() > 100 and np.isinf(s).sum() > 20 and ((s == 0) & np.signbit(s)).sum() > 10
    for kt in range(6):
        W = 32 if kt < 3 else 64
        for kind in (E.FLOAT_KINDS if kt % 3 == 2 else E.INT_KINDS):
            b = E.make_rows(4, 777, kind, kt, 5)
            assert b.dtype == E.UT[kt] and b.shape == (4, 777), (kt, kind)
            assert len({b[r].tobytes() for r in range(4)}) == 4, (kt, kind)     # every row has contents of its own
        c = E.make_rows(4, 777, "const", kt, 5)
        assert (c == c[:, :1]).all()
        t = E.make_rows(4, 777, "two", kt, 5)
        assert all(len(np.unique(t[r])) == 2 for r in range(4))
        lo = E.make_rows(4, 777, "lowbyte", kt, 5)
        assert ((lo ^ lo[:, :1]) >> E.UT[kt](8) == 0).all() and len(np.unique(lo[0])) > 100
        hi = E.make_rows(4, 777, "topbyte", kt, 5)
        assert ((hi ^ hi[:, :1]) << E.UT[kt](8) == 0).all() and len(np.unique(hi[0])) > 100
        st = E.make_rows(4, 777, "sorted", kt, 5)
        assert (st == E.expected(st, kt)).all()
        rv = E.make_rows(4, 777, "reverse", kt, 5)
        assert (rv == E.expected(rv, kt, True)).all()
    E.check_positions(np.array([[5, 3, 5]], np.uint32), np.array([[3, 5, 5]], np.uint32), np.array([[1, 2, 0]], np.int64))
    with pytest.raises(AssertionError):
        E.check_positions(np.array([[5, 3, 5]], np.uint32), np.array([[3, 5, 5]], np.uint32), np.array([[1, 0, 0]], np.int64))
