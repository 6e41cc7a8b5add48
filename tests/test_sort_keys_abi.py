"""The typed, two-way sort (include/msd_sort_keys_hip.h: msd_sort_keys, msd_sort_pairs_keys, msd_reverse; MsdContext.sort_typed
/ reverse) without a GPU: the header declares the three functions with the agreed argument lists, the library exports
them, the binding lists them apart from the surface of msd_radix_hip.h, a null context is refused first, and the Python
wrapper refuses what never needs a device to be refused."""
import ctypes as C
import inspect
import re

import pytest

import abi_support as A

SIGNATURES = {
    "msd_sort_keys": ["msd_ctx *ctx", "void *d_keys", "int key_type", "uint64_t n", "int order"],
    "msd_sort_pairs_keys": ["msd_ctx *ctx", "void *d_keys", "int key_type", "uint64_t *d_rids", "uint64_t n", "int order"],
    "msd_reverse": ["msd_ctx *ctx", "void *d_data", "int elem_bytes", "uint64_t first", "uint64_t count"],
}


def test_header_declares_the_three_functions():
    _, flat = A.header("msd_sort_keys_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    for name, value in (("MSD_ASCENDING", 0), ("MSD_DESCENDING", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), flat), name
    A.check_signatures(flat, SIGNATURES)


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("SORT_KEYS_EXPORTS", SIGNATURES, "msd_sort_keys_hip.h", "msd_reverse.hpp")


def test_null_context_is_refused_with_every_other_argument_zero():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for f in SIGNATURES:
        fn = getattr(L, f)
        zeros = [t() for t in fn.argtypes[1:]]      # the zero value of each argtype
        assert fn(None, *zeros) == -1, f
    # ... and whatever the other arguments are: the context is looked at first
    assert L.msd_sort_keys(None, None, 99, 10, 99) == -1
    assert L.msd_sort_pairs_keys(None, None, 0, None, 10, 0) == -1
    assert L.msd_reverse(None, None, 3, 1 << 63, 1 << 63) == -1


def test_stat_names_are_unknown_to_a_null_context():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    v = C.c_uint64(77)
    for name in (b"sort_keys_split", b"sort_keys_reversed"):
        assert L.msd_stat(None, name, C.byref(v)) == -1 and v.value == 77


def test_sort_typed_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        with pytest.raises(MsdError):                   # a CPU tensor
            ctx.sort_typed(torch.zeros(8, dtype=dt))
        with pytest.raises(MsdError):
            ctx.sort_typed(torch.zeros(8, dtype=dt), descending=True)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError):                   # a dtype without a key order
            ctx.sort_typed(torch.zeros(8).to(dt))
    rids = torch.arange(8, dtype=torch.int64)
    for dt in (torch.float32, torch.int32):
        with pytest.raises(MsdError, match="64-bit"):   # 32-bit keys with rids
            ctx.sort_typed(torch.zeros(8, dtype=dt), rids=rids)
    with pytest.raises(MsdError):                       # rids of another type or length
        ctx.sort_typed(torch.zeros(8, dtype=torch.int64), rids=rids.to(torch.int32))
    with pytest.raises(MsdError):
        ctx.sort_typed(torch.zeros(8, dtype=torch.float64), rids=rids[:7])
    with pytest.raises(MsdError):                       # not 1-D
        ctx.sort_typed(torch.zeros(4, 2))


def test_reverse_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()
    for t, args in ((torch.zeros(8), ()),                                       # a CPU tensor
                    (torch.zeros(8, dtype=torch.int16), ()), (torch.zeros(4, 2), ()),
                    (torch.zeros(8), (5, 4)), (torch.zeros(8), (-1, 2)), (torch.zeros(8), (9,))):
        with pytest.raises(MsdError):
            ctx.reverse(t, *args)


def test_stats_names_are_listed():
    from inplacemsdradixsort_amd import MsdContext, api
    assert "sort_keys_split" in api.STAT_NAMES and "sort_keys_reversed" in api.STAT_NAMES
    assert "in STAT_NAMES" in inspect.getsource(MsdContext.stats)   # (stats() asks for every name of that tuple)
    assert MsdContext.REVERSE_TILE == {4: 4092, 8: 2046}
