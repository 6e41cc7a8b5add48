"""The calls whose ``MsdContext.stats()`` tests/golden/stats_by_call.json records, and the values that
tests/golden/option_outcomes.json probes every option with (a helper module like gpu_support.py, not a test).  Both files
were recorded once with the library as it stood before the context's tables and are replayed by
tests/test_gpu_options.py; they are never written again from the code under test.

Every case runs on a context of its own, so that ``workspace_bytes`` is that call's alone, and takes its input from the
library's generators with a fixed seed."""
import numpy as np
import torch

# (the edges of every rule of csrc/msd_options.hpp and a value on either side of each)
PROBES = (-1, 0, 1, 2, 3, 63, 64, 65, 256, 1024, 1 << 28, (1 << 28) + 1, 1 << 40)
UNKNOWN_OPTION = "no_such_option"


def _u32(ctx, n, seed):
    t = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform_u32(t, seed=seed)
    return t


def _u64(ctx, n, seed):
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.gen_uniform_u64(t, seed=seed)
    return t


def _sort_u32_direct(ctx):
    ctx.set_option("direct_mode", 2)
    ctx.sort_u32(_u32(ctx, 1 << 22, 102))


def _merge_buckets(ctx):
    """the smallest shape of tests/test_gpu_merge.py (8 sources, 4096 buckets of about 3 keys, 9 open bits): per source its
    share of 12288 uniform 21-bit keys in the order of their buckets, unsorted inside a bucket"""
    nsrc, nb, open_bits, n = 8, 4096, 9, 12288
    k = _u32(ctx, n, 110).cpu().numpy().view(np.uint32) & np.uint32((nb << open_bits) - 1)
    rows = [r[np.argsort(r >> np.uint32(open_bits), kind="stable")] for r in np.split(k, nsrc)]
    counts = np.stack([np.bincount(r >> np.uint32(open_bits), minlength=nb) for r in rows]).astype(np.int64)
    base = [x * (n // nsrc) for x in range(nsrc)]
    src = torch.from_numpy(np.concatenate(rows).view(np.int32)).cuda()
    dst = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.merge_buckets(src, torch.from_numpy(counts).cuda(), base, open_bits, 0, dst, n)
    assert (dst.cpu().numpy().view(np.uint32) == np.sort(k)).all()


CASES = {
    "sort_u32_2^16+3": lambda ctx: ctx.sort_u32(_u32(ctx, (1 << 16) + 3, 101)),
    "sort_u32_2^22_direct_mode_2": _sort_u32_direct,
    "sort_u64_2^18": lambda ctx: ctx.sort_u64(_u64(ctx, 1 << 18, 103)),
    "sort_pairs_u64_2^18": lambda ctx: ctx.sort_pairs_u64(_u64(ctx, 1 << 18, 104), torch.arange(1 << 18, dtype=torch.int64, device="cuda")),
    "sort_typed_2^16_f32_descending": lambda ctx: ctx.sort_typed(_u32(ctx, 1 << 16, 105).view(torch.float32), descending=True),
    "topk_100_of_2^16": lambda ctx: ctx.topk(_u32(ctx, 1 << 16, 106), 100),
    "topk_rows_4x4096_k8": lambda ctx: ctx.topk_rows(_u32(ctx, 4 * 4096, 107).view(torch.float32).view(4, 4096), 8),
    "sort_rows_64x512_indices": lambda ctx: ctx.sort_rows(_u32(ctx, 64 * 512, 108).view(torch.float32).view(64, 512), indices=True),
    "partition_2^16_8_bits": lambda ctx: ctx.partition(_u32(ctx, 1 << 16, 109), 24, 8),
    "merge_buckets_8x4096x3": _merge_buckets,
}


def stats_after(name):
    """``stats()`` of a fresh context after the named case"""
    from inplacemsdradixsort_amd import MsdContext
    ctx = MsdContext(0)
    try:
        CASES[name](ctx)
        torch.cuda.synchronize()
        return ctx.stats()
    finally:
        ctx.close()


def option_outcomes(names):
    """``[name, value, return code, msd_last_error]`` of msd_set_option on a fresh context: every name with every probe in
    turn, then the unknown name (the error text of an accepted call is the last refusal's, so the order is part of it)"""
    from inplacemsdradixsort_amd import MsdContext
    ctx = MsdContext(0)
    try:
        out = []
        for name, v in [(n, v) for n in names for v in PROBES] + [(UNKNOWN_OPTION, 1)]:
            rc = ctx._L.msd_set_option(ctx._h, name.encode(), v)
            out.append([name, v, rc, ctx._L.msd_last_error(ctx._h).decode()])
        return out
    finally:
        ctx.close()
