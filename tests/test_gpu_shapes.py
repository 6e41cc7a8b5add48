"""Structured inputs (sorted, reversed, long runs of one top digit, locally sorted blocks) at 2^26 keys: exact
result and no pathological slowdown.  Such inputs leave about one empty slot per stripe -- a handful of very
long chains for the block permutation unless it parks blocks to create more (`kMinChains`), and lists that
are consumed in lockstep at addresses a whole number of bucket regions apart unless each list starts at its
own entry; both cost a factor of 20-100 before they were handled.  The reference has no such test; the
oracle is torch.sort of the same keys (bit-exact), the time bound is relative to uniform keys in the same run."""
import time

import pytest

from gpu_support import DEFAULTS

pytestmark = pytest.mark.gpu

LOGN = 26


def _shapes(torch, ctx, n):
    base = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform_u32(base, seed=4242)
    srt = base.clone()
    ctx.sort_u32(srt)
    idx = torch.arange(n, device="cuda", dtype=torch.int64)
    return {
        "uniform": base,
        "sorted": srt,
        "reversed": torch.flip(srt, dims=[0]).contiguous(),
        "runs64k": (base & 0x00FFFFFF) | (((idx >> 16) & 0xFF) << 24).to(torch.int32),
        "blocksorted": base.view(-1, 1 << 20).sort(dim=1).values.contiguous().view(-1),
        "sawtooth": ((idx * 2654435761) & 0xFFFFFFFF).to(torch.int32),
    }


def _as_u32(torch, t):
    return t.to(torch.int64) & 0xFFFFFFFF


def test_structured_inputs_sort_exactly_and_in_reasonable_time(ctx):
    import torch
    n = 1 << LOGN
    shapes = _shapes(torch, ctx, n)
    times = {}
    for name, src in shapes.items():
        expect = torch.sort(_as_u32(torch, src)).values
        best = None
        for _ in range(2):
            t = src.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.sort_u32(t)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert bool((_as_u32(torch, t) == expect).all()), name
        times[name] = best
        del expect
    for name, dt in times.items():
        assert dt < 6.0 * times["uniform"] + 2e-3, (name, times)


@pytest.mark.parametrize("direct", [0, 2])
def test_structured_inputs_with_direct_placement_off_and_forced(ctx, direct):
    """The same shapes through both classify kernels (forced direct placement is slow on runs, never wrong)."""
    import torch
    n = 1 << 24
    ctx.set_option("direct_mode", direct)
    ctx.set_option("direct_min", 1 << 16)
    try:
        for name, src in _shapes(torch, ctx, n).items():
            t = src.clone()
            ctx.sort_u32(t)
            assert bool((_as_u32(torch, t) == torch.sort(_as_u32(torch, src)).values).all()), (name, direct)
    finally:
        ctx.set_option("direct_mode", DEFAULTS["direct_mode"])
        ctx.set_option("direct_min", DEFAULTS["direct_min"])
