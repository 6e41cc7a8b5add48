"""Per-row top-k (msd_topk_rows, msd_topk_rows_limits; MsdContext.topk_rows) without a GPU: the header declares the two
functions with the agreed argument lists, the library exports them and the binding carries them, arguments are refused
before anything touches a device, the envelope is reported, and the layout rule of the Python wrapper -- which needs no
device -- accepts and refuses what it should on CPU tensors."""
import ctypes as C

import pytest

import abi_support as A

NEW = ["msd_topk_rows", "msd_topk_rows_limits"]
ARGS = {
    "msd_topk_rows": ["msd_ctx *ctx", "const void *d_keys", "int key_type", "uint64_t rows", "uint64_t row_len", "uint64_t row_stride",
                      "uint64_t k", "int which", "void *d_out_keys", "uint64_t *d_out_idx"],
    "msd_topk_rows_limits": ["int key_type", "int with_idx", "uint64_t *max_row_len", "uint64_t *max_k"],
}


@pytest.mark.parametrize("f", NEW)
def test_header_declares_the_function_with_its_argument_list(f):
    A.check_signatures(A.header("msd_radix_hip.h")[1], {f: ARGS[f]}, exactly=False)


def test_library_exports_and_binding_lists_them():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for f in NEW:
        assert f in _lib.EXPORTS, f
        assert hasattr(L, f), f
        assert getattr(L, f).argtypes is not None and len(getattr(L, f).argtypes) == len(ARGS[f]), f


def test_null_context_is_refused():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    assert L.msd_topk_rows(None, None, 2, 4, 10, 10, 1, 0, None, None) == -1
    assert L.msd_topk_rows(None, None, 2, 0, 10, 10, 0, 0, None, None) == -1     # (even where the call would be a no-op)


def test_limits_for_every_key_type():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for kt in range(6):
        for with_idx in (0, 1):
            a, b = C.c_uint64(7), C.c_uint64(7)
            assert L.msd_topk_rows_limits(kt, with_idx, C.byref(a), C.byref(b)) == 0
            assert a.value >= 1 << 20 and b.value >= 1024, (kt, with_idx, a.value, b.value)
            assert a.value < 1 << 32, "positions within a row travel in 32 bits"


def test_limits_refuses_bad_arguments_and_leaves_the_outputs():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    a, b = C.c_uint64(77), C.c_uint64(78)
    for bad in (6, -1, 100):
        assert L.msd_topk_rows_limits(bad, 0, C.byref(a), C.byref(b)) == -1
        assert L.msd_topk_rows_limits(bad, 1, C.byref(a), C.byref(b)) == -1
    assert L.msd_topk_rows_limits(2, 0, None, C.byref(b)) == -1
    assert L.msd_topk_rows_limits(2, 0, C.byref(a), None) == -1
    assert L.msd_topk_rows_limits(2, 1, None, None) == -1
    assert a.value == 77 and b.value == 78


# ---- the layout rule of MsdContext.topk_rows: no device needed

def test_layouts_that_are_taken():
    import torch
    lay = A.bare_ctx()._rows_layout
    assert lay(torch.empty(50257)) == (1, 50257, 50257)                       # 1-D: one row
    assert lay(torch.empty(7, 131)) == (7, 131, 131)
    assert lay(torch.empty(3, 5, 131)) == (15, 131, 131)                      # contiguous: the leading dimensions collapse
    assert lay(torch.empty(2, 3, 5, 8, dtype=torch.int64)) == (30, 8, 8)
    x = torch.empty(7, 131)
    assert lay(x[:, :-3]) == (7, 128, 131)                                    # padded rows
    assert lay(x[:, 1:]) == (7, 130, 131)                                     # rows that start off the 16-byte grid
    assert lay(x[2:5, 3:40]) == (3, 37, 131)
    assert lay(x[::2]) == (4, 131, 262)                                       # every other row: still one row stride
    assert lay(torch.empty(1, 9)) == (1, 9, 9)
    assert lay(torch.empty(4, 1, 9)) == (4, 9, 9)                             # a dimension of size 1 has no say
    assert lay(torch.empty(0, 9)) == (0, 9, 9)
    assert lay(torch.empty(4, 0))[:2] == (4, 0)
    y = torch.empty(3, 5, 140)[:, :, :131]                                    # 3-D, padded in the last dimension only
    assert lay(y) == (15, 131, 140)


def test_layouts_that_are_refused():
    import torch
    from inplacemsdradixsort_amd import MsdError
    lay = A.bare_ctx()._rows_layout
    x = torch.empty(64, 48)
    for bad in (x.t(),                                  # a transposed matrix: the last dimension has stride 48
                x[:, ::2],                              # every other column
                torch.empty(3, 6, 16)[:, :4, :],        # 3-D: the leading dimensions do not collapse (stride 96 != 4 * 16)
                torch.empty(6, 3, 16).transpose(0, 1),
                torch.empty(16).expand(4, 16),          # row stride 0 < row length
                torch.empty(())):                       # no dimension
        with pytest.raises(MsdError):
            lay(bad)


def test_dtype_without_a_key_order_is_refused_before_the_layout():
    import torch
    from inplacemsdradixsort_amd import MsdContext, MsdError
    ctx = A.bare_ctx()
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError):
            ctx.topk_rows(torch.zeros(4, 8).to(dt), 2)
    with pytest.raises(MsdError):                       # a CPU tensor never reaches the library
        ctx.topk_rows(torch.zeros(4, 8), 2)
    assert callable(MsdContext.topk_rows) and callable(MsdContext.topk_rows_limits)


def test_stats_names_are_listed():
    import inspect
    from inplacemsdradixsort_amd import MsdContext
    from inplacemsdradixsort_amd import api
    assert "topk_rows_kernel_rows" in api.STAT_NAMES and "topk_rows_looped_rows" in api.STAT_NAMES
    assert "in STAT_NAMES" in inspect.getsource(MsdContext.stats)   # (stats() asks for every name of that tuple)
