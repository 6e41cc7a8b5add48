"""Run-length encode (include/msd_runs_hip.h: msd_run_encode, msd_run_encode_limits; MsdContext.run_encode / run_encode_limits /
unique) without a GPU: the header declares the two functions with the agreed argument lists, the library exports them, the
binding lists them apart from the other surfaces, a null context is refused first, the limits call answers on the host, the
Python wrappers refuse what never needs a device to be refused, and the numpy expectation of tests/runs_expect.py is what
its docstring says."""
import ctypes as C

import numpy as np
import pytest

import abi_support as A
import runs_expect as R

SIGNATURES = {
    "msd_run_encode": ["msd_ctx *ctx", "const void *d_data", "int elem_bytes", "uint64_t n", "uint64_t cap", "void *d_values",
                       "uint64_t *d_starts", "const uint64_t *d_positions", "uint64_t *d_inverse", "uint64_t *d_num_runs"],
    "msd_run_encode_limits": ["int elem_bytes", "uint64_t *tile", "uint64_t *scan_tile"],
}


def test_header_declares_the_two_functions():
    text, flat = A.header("msd_runs_hip.h")
    assert '#include "msd_radix_hip.h"' in flat
    A.check_signatures(flat, SIGNATURES)
    assert "torch.unique" in text and "NaN" in text and "-0.0" in text   # the header says where bitwise equality differs


def test_library_exports_and_binding_lists_them_apart():
    A.check_exports("RUNS_EXPORTS", SIGNATURES, "msd_runs_hip.h", "msd_runs.hpp")


def test_null_context_is_refused_whatever_the_other_arguments_are():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    zeros = [t() for t in L.msd_run_encode.argtypes[1:]]
    assert L.msd_run_encode(None, *zeros) == -1
    assert L.msd_run_encode(None, None, 4, 0, 0, None, None, None, None, None) == -1
    assert L.msd_run_encode(None, None, 3, 10, 10, None, None, C.c_void_p(8), None, None) == -1
    p = C.c_void_p(64)
    assert L.msd_run_encode(None, p, 8, 1 << 63, 1 << 63, p, p, p, p, p) == -1
    assert L.msd_last_error(None) == b"null context"


def test_limits():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for es in (4, 8):
        tile, scan_tile = C.c_uint64(0), C.c_uint64(0)
        assert L.msd_run_encode_limits(es, C.byref(tile), C.byref(scan_tile)) == 0
        assert tile.value >= 64 and scan_tile.value >= 64, (es, tile.value, scan_tile.value)
    A.check_limits_refusals(L.msd_run_encode_limits, 2, bad_widths=(0, 2, 16, -4, 5))


def test_limits_wrapper():
    from inplacemsdradixsort_amd import MsdError, _lib
    ctx = A.bare_ctx()
    ctx._L = _lib.load()
    for es in (4, 8):
        tile, scan_tile = ctx.run_encode_limits(es)
        assert tile >= 64 and scan_tile >= 64
    for es in (0, 2, 16):
        with pytest.raises(MsdError):
            ctx.run_encode_limits(es)


def test_run_encode_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()                                             # (no _L, no _h: touching the library would raise AttributeError)
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for kw in ({}, {"cap": 3}, {"inverse": True}, {"values": False, "starts": False}):
            with pytest.raises(MsdError, match="GPU"):              # a CPU tensor
                ctx.run_encode(torch.zeros(8, dtype=dt), **kw)
    with pytest.raises(MsdError, match="1-D"):                      # not 1-D
        ctx.run_encode(torch.zeros(4, 8))
    with pytest.raises(MsdError, match="1-D"):
        ctx.run_encode(torch.zeros(()))
    with pytest.raises(MsdError, match="contiguous"):               # not contiguous
        ctx.run_encode(torch.zeros(16)[::2])
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="4- or 8-byte"):         # an element size other than 4 or 8
            ctx.run_encode(torch.zeros(8).to(dt))
    x = torch.zeros(8)
    for pos in (torch.zeros(8, dtype=torch.int32), torch.zeros(8), torch.zeros(7, dtype=torch.int64), torch.zeros(9, dtype=torch.int64),
                torch.zeros(2, 4, dtype=torch.int64)):
        with pytest.raises(MsdError, match="positions must be"):    # positions of the wrong dtype or length
            ctx.run_encode(x, inverse=True, positions=pos)
    with pytest.raises(MsdError, match="positions without inverse"):
        ctx.run_encode(x, positions=torch.arange(8))
    with pytest.raises(MsdError, match="GPU"):                      # everything else in order: still a CPU tensor
        ctx.run_encode(x, inverse=True, positions=torch.arange(8))


def test_unique_refuses_before_the_library_is_touched():
    import torch
    from inplacemsdradixsort_amd import MsdError
    ctx = A.bare_ctx()
    for dt in (torch.float32, torch.int32, torch.float64, torch.int64):
        for kw in ({}, {"return_inverse": True}, {"return_counts": True}):
            with pytest.raises(MsdError, match="GPU"):
                ctx.unique(torch.zeros(8, dtype=dt), **kw)
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError, match="no key order"):
            ctx.unique(torch.zeros(8).to(dt))
    with pytest.raises(MsdError, match="1-D"):
        ctx.unique(torch.zeros(4, 8))
    with pytest.raises(MsdError, match="contiguous"):
        ctx.unique(torch.zeros(16)[::2])


def test_the_docstrings_say_where_bitwise_equality_differs_from_torch():
    from inplacemsdradixsort_amd import MsdContext
    for f in (MsdContext.run_encode, MsdContext.unique):
        assert "torch.unique" in f.__doc__ and "NaN" in f.__doc__ and "-0.0" in f.__doc__, f.__name__


def test_the_expectation_on_a_worked_example():
    a = np.array([5, 5, 7, 5, 5, 5, 9], np.uint32)
    m, values, starts, inverse = R.expected(a)
    assert m == 4 and values.tolist() == [5, 7, 5, 9] and starts.tolist() == [0, 2, 3, 6, 7] and inverse.tolist() == [0, 0, 1, 2, 2, 2, 3]
    pos = np.array([6, 5, 4, 3, 2, 1, 0])
    assert R.expected(a, pos)[3].tolist() == [3, 2, 2, 2, 1, 0, 0]
    m2, v2, s2, _ = R.expected_capped(a, 2)
    assert m2 == 4 and v2.tolist() == [5, 7] and s2.tolist() == [0, 2, 3]      # the terminator: the start of run `cap`
    m3, v3, s3, _ = R.expected_capped(a, 9)
    assert v3.tolist() == values.tolist() and s3.tolist() == starts.tolist()    # ... or the array's length
    m0, v0, s0, i0 = R.expected(a[:0])
    assert m0 == 0 and v0.size == 0 and s0.tolist() == [0] and i0.size == 0
    # floats through integer views: the two zeros are two runs, equal NaNs one run, other payloads another run
    f = np.array([0.0, -0.0, -0.0, 1.0], np.float32).view(np.uint32)
    assert R.expected(f)[0] == 3
    nan = np.array([0x7FC00000, 0x7FC00000, 0x7FC00001, 0xFFC00000], np.uint32)
    assert R.expected(nan)[0] == 3


def test_generated_patterns_are_what_they_say():
    T = 64
    for es in (4, 8):
        d = R.make("distinct", 5 * T, es, T)
        assert d.dtype == R.UT[es] and np.unique(d).size == d.size
        assert R.expected(R.make("equal", 5 * T, es, T))[0] == 1
        assert R.expected(R.make("alternating", 5 * T, es, T))[0] == 5 * T
        m, _, starts, _ = R.expected(R.make("starts_at_tile", 5 * T, es, T))
        assert T in starts and m == 5 * T - 16
        m, _, starts, _ = R.expected(R.make("ends_at_tile", 5 * T, es, T))
        assert T in starts and T - 9 in starts and m == 5 * T - 8
        m, _, starts, _ = R.expected(R.make("three_tiles", 5 * T, es, T))
        assert T in starts and 4 * T in starts and m == 2 * T + 1
        for mean in (1.5, 40, 5000):
            g = R.make("geo%g" % mean, 200000, es, T)
            assert g.size == 200000 and 0.5 * mean < 200000 / R.expected(g)[0] < 2 * mean, mean   # (mean 5000: some 40 runs)
        for n in (0, 1, 2, 3):
            for p in R.PATTERNS:
                assert R.make(p, n, es, T).size == n
        top = R.UT[es](1 << (8 * es - 1))
        t = R.two_values(1000, es, 5, 5 | int(top), 3)
        assert set(np.unique(t).tolist()) == {5, 5 | int(top)} and 200 < R.expected(t)[0] < 500
    assert list(R.sizes(4096, 2048).values())[-1] == 2049 * 4096 + 5 and R.SIZE_NAMES[-1] == "big"
