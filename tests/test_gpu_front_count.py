"""The front pass of a u32 sort (csrc/msd_front16.hpp, option `front_count`): the top 16 key bits counted once, both direct
rounds placed from that count, one readback.

The path is taken where the plan is two direct 8-bit rounds followed by counting leaves of 16 open bits.  The planner
(pick_width) gives round 1 an 8-bit digit only if its children keep 2048 keys or more, that is from n = 2^27 evenly
spread keys on (at 2^20 .. 2^26 it plans a 7- or 8-bit round and narrower ones behind it, whatever `direct_min` and
`direct_min_parent` are set to), and the front pass is tried only where parents an eighth below the mean still get one:
from 1.15 * 2^27 keys on.  By default it is tried from 2^29 keys on (`front_min`, by measurement); the fixture
lowers that to 2^27, and every case runs at N = 5 * 2^25 = 1.25 * 2^27 keys with the other switches at their defaults;
below that size neither statistic is set.  One base array and its numpy sorts are shared by the cases that can use them.

Every case compares the sorted array with numpy.sort for exact equality, asserts through the stats `front_count_sorts` /
`front_count_declined` which way the sort went, and that `front_count = 0` gives the same array.
"""
import numpy as np
import pytest
import torch

import guardband
from gpu_support import DEFAULTS, dev_bits as dev, host_bits as host, restore_defaults
from inplacemsdradixsort_amd import MsdError

pytestmark = pytest.mark.gpu

N = 5 << 25
_cache = {}


def base(ctx):
    """N + 5 uniform keys (generated on the device), as a numpy array"""
    if "base" not in _cache:
        t = torch.empty(N + 5, dtype=torch.int32, device="cuda")
        ctx.gen_uniform_u32(t, seed=0x5EED0F16)
        _cache["base"] = host(t)
    return _cache["base"]


def base_sorted(ctx, n):
    """numpy's sort of the first n keys of the base array"""
    if n not in _cache:
        _cache[n] = np.sort(base(ctx)[:n])
    return _cache[n]


@pytest.fixture()
def fctx(ctx):
    """the library's defaults, whatever an earlier test of the session left, and `front_min` lowered to sizes numpy sorts in a moment"""
    names = ("front_count", "front_min", "direct_mode", "direct_min", "direct_min_parent")
    restore_defaults(ctx, *names)
    ctx.set_option("front_min", 1 << 27)
    yield ctx
    restore_defaults(ctx, *names)


def way(ctx):
    st = ctx.stats()
    return st.get("front_count_sorts", 0), st.get("front_count_declined", 0)


def sort_both(ctx, k, ref, expect):
    """sorts k with the front pass and without it; expect: "taken", "declined" or "either"."""
    t = dev(k)
    ctx.set_option("front_count", 1)
    ctx.sort_u32(t)
    got = way(ctx)
    assert (host(t) == ref).all(), "front_count = 1: not numpy's sort"
    if expect == "either":
        assert got in ((1, 0), (0, 1)), got
    else:
        assert got == ((1, 0) if expect == "taken" else (0, 1)), (expect, got, ctx.stats())
    t0 = dev(k)
    ctx.set_option("front_count", 0)
    ctx.sort_u32(t0)
    assert way(ctx) == (0, 0), ctx.stats()
    assert torch.equal(t, t0), "front_count = 0 gives another array"
    ctx.set_option("front_count", DEFAULTS["front_count"])
    return got


@pytest.mark.parametrize("n", [N, N + 5, N - 3])
def test_uniform_taken(fctx, n):
    """(the odd lengths: keys behind the last whole 16-byte vector, and a last chunk that is not full)"""
    sort_both(fctx, base(fctx)[:n], base_sorted(fctx, n), "taken")
    st = fctx.stats()
    assert st.get("direct_rounds", 0) == 2 and st.get("count_segments", 0) == 65536, st


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 5, (1 << 21) - 3])
def test_small_shapes_are_not_tried(fctx, n):
    """with the small-shape switches of the direct tests the plan at these sizes is still not two 8-bit rounds (a 7- or
    8-bit round, then 1-bit rounds): the front pass does not run, the sort is what it was"""
    fctx.set_option("direct_min", 1 << 16)
    fctx.set_option("direct_min_parent", 1 << 12)
    try:
        k = base(fctx)[:n]
        ref = np.sort(k)
        for opt in (1, 0):
            fctx.set_option("front_count", opt)
            t = dev(k)
            fctx.sort_u32(t)
            assert way(fctx) == (0, 0), fctx.stats()
            assert (host(t) == ref).all()
    finally:
        restore_defaults(fctx, "direct_min", "direct_min_parent")


def test_view_off_the_block_grid(fctx):
    """a view that starts 16 bytes into an allocation: off the 256-byte block grid, on the 16-byte grid the library asks for"""
    k, ref = base(fctx)[:N], base_sorted(fctx, N)
    whole = torch.zeros(N + 8, dtype=torch.int32, device="cuda")
    v = whole[4:4 + N]
    v.copy_(dev(k))
    fctx.sort_u32(v)
    assert way(fctx) == (1, 0), fctx.stats()
    assert (host(v) == ref).all()
    assert int(whole[:4].abs().sum()) == 0 and int(whole[4 + N:].abs().sum()) == 0


@pytest.mark.parametrize("off", [1, 3])
def test_view_off_the_16_byte_grid_is_refused_as_before(fctx, off):
    """the library takes 16-byte aligned keys only (include/msd_radix_hip.h); the front pass reads 16-byte vectors from the
    array's start and relies on it: such a view is refused before anything is read or written, with or without the option"""
    k = base(fctx)[:N + 4]
    for opt in (1, 0):
        fctx.set_option("front_count", opt)
        whole = dev(k)
        with pytest.raises(MsdError):
            fctx.sort_u32(whole[off:off + N])
        assert (host(whole) == k).all()
    fctx.set_option("front_count", DEFAULTS["front_count"])


def test_top_byte_zero_declined(fctx):
    k = base(fctx)[:N] >> np.uint32(8)
    sort_both(fctx, k, np.sort(k), "declined")


def test_all_equal_declined(fctx):
    k = np.full(N, 0xDEADBEEF, dtype=np.uint32)
    sort_both(fctx, k, k, "declined")


def probed(n):
    """positions front_probe_kernel samples (csrc/msd_front16.hpp: 32 runs of 1024 consecutive keys, evenly spread)"""
    stride = n // 1024 // 32 * 1024
    m = np.zeros(n, dtype=bool)
    for r in range(32):
        m[r * stride:r * stride + 1024] = True
    return m


def test_counter_overflow_declined(fctx):
    """half the keys share one 16-bit prefix: every workgroup's counter for it passes 65535.  Where the probe looks the
    keys stay evenly spread, so that the count is made and it is the overflow flag (or the exact verdict) that declines."""
    k = base(fctx)[:N].copy()
    crowd = ~probed(N)
    crowd[1::2] = False
    k[crowd] = (k[crowd] & np.uint32(0xFFFF)) | np.uint32(0x12340000)
    sort_both(fctx, k, np.sort(k), "declined")


def test_skew_seen_by_the_probe_declined(fctx):
    """the same crowd everywhere: the sample shows it and the read is not made"""
    k = base(fctx)[:N].copy()
    k[::2] = (k[::2] & np.uint32(0xFFFF)) | np.uint32(0x12340000)
    sort_both(fctx, k, np.sort(k), "declined")


@pytest.mark.parametrize("order", ["sorted", "reversed"])
def test_runs_declined(fctx, order):
    ref = base_sorted(fctx, N)
    k = ref if order == "sorted" else ref[::-1].copy()
    sort_both(fctx, k, ref, "declined")


def test_zipf_declined(fctx):
    t = torch.empty(N, dtype=torch.int32, device="cuda")
    fctx.gen_zipf_u32(t, seed=0x5EED0003)
    k = host(t)
    sort_both(fctx, k, np.sort(k), "declined")


def test_one_empty_second_byte_bucket(fctx):
    """exactly one child of one parent of round 1 is empty (prefix 0x4242 moved into 0x4243): zero counts in the plan and
    in the segment lists; whether the path is taken follows direct_plan_kernel's rule"""
    k = base(fctx)[:N].copy()
    k[(k >> np.uint32(16)) == 0x4242] |= np.uint32(0x10000)
    assert ((k >> np.uint32(16)) == 0x4242).sum() == 0
    sort_both(fctx, k, np.sort(k), "either")


def test_guarded_buffer(fctx):
    """no write outside the array (the front pass writes its partials, counts and summary into the workspace only)"""
    k, ref = base(fctx)[:N], base_sorted(fctx, N)
    a = guardband.Arena(torch.int32, N, lead_bytes=16).fill(k)
    fctx.sort_u32(a.payload)
    a.check("front_count sort")
    assert way(fctx) == (1, 0), fctx.stats()
    assert (a.host(np.uint32) == ref).all()


def test_two_sorts_back_to_back(fctx):
    """different lengths, one context, path taken in both: nothing of the first sort's counts may reach the second"""
    for n in (N + 5, N - 3, N + 5):
        t = dev(base(fctx)[:n])
        fctx.sort_u32(t)
        assert way(fctx) == (1, 0), (n, fctx.stats())
        assert (host(t) == base_sorted(fctx, n)).all(), n
