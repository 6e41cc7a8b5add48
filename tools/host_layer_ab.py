#!/usr/bin/env python3
"""Does a change of the host layer (msd_radix.hip outside the kernels) cost time?  Parent build against this one.

    python tools/host_layer_ab.py [runs [rows.jsonl [case-prefix ...]]]   (needs libinpmsdradix_hip_parent.so: _build.build_variant("parent") on the parent's tree)

Alternates the two builds in one job, `runs` (default 5: three underestimate the spread between processes) fresh processes
each; the rows are appended to rows.jsonl (default profiles/host_layer_ab.jsonl; the tile layer's job, DESIGN.md 1.1, was
`python tools/host_layer_ab.py 5 profiles/tile_layer_ab.jsonl`).  With case prefixes only the cases whose name starts with
one of them are measured.  A process measures, on one GPU:
  sort_u32_2^16, sort_u32_2^20   msd_sort_u32 on fresh uniform keys: median over 200 calls of the host clock around call + synchronise
  topk_rows_4x4096_f32_k8        msd_topk_rows, 4 rows of 4096 float32, k = 8: the same
  sort_rows_64x512_f32_idx       msd_sort_rows, 64 rows of 512 float32 with positions: the same, as all of the following
  run_encode_2^16_i32            msd_run_encode on 2^16 sorted int32 (values, starts)
  reduce_runs_sum_2^16_i64       msd_reduce_runs, the sum of int64 values over the runs of the same keys
  searchsorted_2^16_in_2^20_i32  msd_search_sorted, 2^16 unsorted needles in 2^20 sorted int32
  sort_typed_2^16_f32            msd_sort_keys on 2^16 float32 (a fresh copy of the same keys before every call)
  bench_2^30_u32                 bench.py's default line (ms_per_step of --steps 10 --warmup 2)
and, per entry point of the tile algorithms, at 2^16 elements (host time dominates; 200 calls) and at 2^26 (the tile kernels
dominate; 50 calls), sorted int32 keys with about 16 elements per run, N = the size:
  run_encode_N, reduce_runs_sum_f32_N, reduce_runs_min_i32_N (and _keys64_N: int64 keys), scan_runs_sum_f32_N, compact_range_N (the middle half of the key range, with values)
  searchsorted_merge_N (N ascending needles in N keys), merge_sorted_N, set_union_N, join_groups_N (N / 2 keys a side),
  join_pairs_N (all pairs of those groups)
and the leaves of the multi-GPU exchange at about 2^26 keys (50 calls):
  merge_buckets_{2,4,8}src_2^26 (msd_merge_buckets_u32: merge_place16_kernel) and merge_buckets_low16_2^26 (4 sources of low
  halves: merge_count_kernel): 4096 buckets of about 2^14 keys with 16 open bits, the sources' extents back to back behind
  gaps of 0 .. 6 elements (the bucket shapes of tests/test_gpu_merge.py);
  hist2_pack_2^26 (msd_hist2_pack_u32): 2^26 sorted uniform keys, 65536 buckets of about 1024 keys
and prints one JSON line per case; the driver appends them to profiles/host_layer_ab.jsonl and prints the comparison:
per case the parent's min-max over its runs against the median of this build's runs.  The small cases are the ones where
host time dominates (a sort of 2^16 keys is a dozen launches and two synchronisations)."""
import io
import json
import os
import runpy
import statistics
import subprocess
import sys
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "host_layer_ab.jsonl")
CALLS = 200


def child():
    sys.path.insert(0, ROOT)
    import torch
    if os.environ.get("MSD_VARIANT"):  # an experimental build (inplacemsdradixsort_amd._build.build_variant)
        from inplacemsdradixsort_amd import _build
        _build.LIB = os.path.join(_build.HERE, f"libinpmsdradix_hip_{os.environ['MSD_VARIANT']}.so")
        _build.stale = lambda: False
    from inplacemsdradixsort_amd import MsdContext
    ctx = MsdContext(0)
    ctx.use_torch_stream()

    def timed(call, before=None, calls=CALLS):
        ms = []
        for i in range(calls + 20):
            if before:
                before(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms[20:])                      # (the first 20 calls warm up)

    rows = {}
    only = [p for p in os.environ.get("MSD_AB_CASES", "").split(",") if p]

    def case(name, call, before=None, calls=CALLS):
        if not only or any(name.startswith(p) for p in only):
            rows[name] = timed(call, before, calls)

    for logn in (16, 20):
        t = torch.empty(1 << logn, dtype=torch.int32, device="cuda")
        case(f"sort_u32_2^{logn}", lambda: ctx.sort_u32(t), lambda i: ctx.gen_uniform_u32(t, seed=i))
        assert f"sort_u32_2^{logn}" not in rows or ctx.check(t)[0] == 0
    x = torch.randn(4, 4096, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    o = torch.empty(4, 8, device="cuda")
    case("topk_rows_4x4096_f32_k8", lambda: ctx.topk_rows(x, 8, out=o))
    # the typed entry points: one to four launches and no synchronisation of their own, so the call's time is host time
    g = torch.Generator("cuda").manual_seed(2)
    m = torch.randn(64, 512, device="cuda", generator=g)
    mo, mi = torch.empty_like(m), torch.empty(64, 512, dtype=torch.int64, device="cuda")
    case("sort_rows_64x512_f32_idx", lambda: ctx.sort_rows(m, out=mo, out_indices=mi))
    sk = torch.randint(0, 1 << 12, (1 << 16,), dtype=torch.int32, device="cuda", generator=g).sort().values
    sv = torch.arange(1 << 16, dtype=torch.int64, device="cuda")
    case("run_encode_2^16_i32", lambda: ctx.run_encode(sk))
    case("reduce_runs_sum_2^16_i64", lambda: ctx.reduce_runs(sk, sv))
    hay = torch.randint(-(1 << 30), 1 << 30, (1 << 20,), dtype=torch.int32, device="cuda", generator=g).sort().values
    needles = torch.randint(-(1 << 30), 1 << 30, (1 << 16,), dtype=torch.int32, device="cuda", generator=g)
    found = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    case("searchsorted_2^16_in_2^20_i32", lambda: ctx.searchsorted(hay, needles, out=found))
    f = torch.randn(1 << 16, device="cuda", generator=g)
    ft = torch.empty_like(f)
    case("sort_typed_2^16_f32", lambda: ctx.sort_typed(ft), lambda i: ft.copy_(f))
    del hay, needles, found, t, m, mo, mi
    for logn, calls in ((16, 200), (26, 50)):
        N, tag = 1 << logn, "2^%d" % logn
        gg = torch.Generator("cuda").manual_seed(logn)
        keys = torch.randint(0, N // 16, (N,), dtype=torch.int32, device="cuda", generator=gg).sort().values
        fv = torch.randn(N, device="cuda", generator=gg)
        case(f"run_encode_{tag}", lambda: ctx.run_encode(keys), calls=calls)
        case(f"reduce_runs_sum_f32_{tag}", lambda: ctx.reduce_runs(keys, fv), calls=calls)
        k64 = keys.to(torch.int64)
        case(f"reduce_runs_min_i32_{tag}", lambda: ctx.reduce_runs(keys, keys, op="min"), calls=calls)
        case(f"reduce_runs_min_i32_keys64_{tag}", lambda: ctx.reduce_runs(k64, keys, op="min"), calls=calls)
        del k64
        case(f"scan_runs_sum_f32_{tag}", lambda: ctx.scan_runs(keys, fv), calls=calls)
        case(f"compact_range_{tag}", lambda: ctx.compact(keys=keys, lo=N // 64, hi=3 * N // 64, values=fv), calls=calls)
        other = torch.randint(0, N // 16, (N,), dtype=torch.int32, device="cuda", generator=gg).sort().values
        case(f"searchsorted_merge_{tag}", lambda: ctx.searchsorted(keys, other, needles_sorted=True), calls=calls)
        a, b = keys[: N // 2].contiguous(), other[N // 2 :].contiguous()
        case(f"merge_sorted_{tag}", lambda: ctx.merge_sorted(a, b), calls=calls)
        case(f"set_union_{tag}", lambda: ctx.set_sorted(a, b, "union"), calls=calls)
        au = torch.randint(0, 4 * N, (N // 2,), dtype=torch.int32, device="cuda", generator=gg).sort().values   # few matches: about N / 16 pairs
        bu = torch.randint(0, 4 * N, (N // 2,), dtype=torch.int32, device="cuda", generator=gg).sort().values
        case(f"join_groups_{tag}", lambda: ctx.join_groups(au, bu), calls=calls)
        groups = ctx.join_groups(au, bu)
        case(f"join_pairs_{tag}", lambda: ctx.join_pairs(groups, N // 2, N // 2, N), calls=calls)
        del keys, fv, other, a, b, au, bu, groups
    exchange = [f"merge_buckets_{x}src_2^26" for x in (2, 4, 8)] + ["merge_buckets_low16_2^26", "hist2_pack_2^26"]
    if not only or any(c.startswith(p) for p in only for c in exchange):
        nb, first, gg = 4096, 5 * 4096, torch.Generator("cuda").manual_seed(26)

        def arrivals(nsrc):  # per source: its buckets first .. first + nb - 1 in order, unsorted inside a bucket
            counts = torch.poisson(torch.full((nsrc, nb), 16384.0 / nsrc, device="cuda"), generator=gg).to(torch.int64)
            parts, base, at = [], [], 0
            for x in range(nsrc):
                pre = torch.repeat_interleave(torch.arange(first, first + nb, device="cuda"), counts[x])
                low = torch.randint(0, 1 << 16, (pre.numel(),), device="cuda", generator=gg)
                parts += [torch.full((x % 7,), -1, dtype=torch.int32, device="cuda"), ((pre << 16) | low).to(torch.int32)]
                base.append(at + x % 7)
                at += x % 7 + pre.numel()
            parts.append(torch.full((8,), -1, dtype=torch.int32, device="cuda"))
            return torch.cat(parts), counts, base, int(counts.sum())

        for nsrc in (2, 4, 8):
            src, counts, base, n = arrivals(nsrc)
            dst = torch.empty(n + 5, dtype=torch.int32, device="cuda")
            case(f"merge_buckets_{nsrc}src_2^26", lambda: ctx.merge_buckets(src, counts, base, 16, first, dst, n), calls=50)
            if nsrc == 4:
                low = src.to(torch.int16)
                case("merge_buckets_low16_2^26", lambda: ctx.merge_buckets(low, counts, base, 16, first, dst, n), calls=50)
                del low
            del src, counts, dst
        keys = torch.randint(-(1 << 31), 1 << 31, (1 << 26,), dtype=torch.int64, device="cuda", generator=gg).to(torch.int32)
        ctx.sort_u32(keys)
        bounds = ctx.bucket_bounds(keys, 16, 65536)
        rec = torch.empty(65536 * ctx.HIST2_RECORD_BYTES, dtype=torch.uint8, device="cuda")
        case("hist2_pack_2^26", lambda: ctx.hist2_pack(keys, bounds, rec), calls=50)
        del keys, bounds, rec
    ctx.close()
    if not only or any("bench_2^30_u32".startswith(p) for p in only):
        buf = io.StringIO()
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"]
        with redirect_stdout(buf):
            runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
        rows["bench_2^30_u32"] = json.loads(buf.getvalue().strip().splitlines()[-1])["ms_per_step"]
    for case, ms in rows.items():
        print(json.dumps({"case": case, "ms": round(ms, 5)}), flush=True)


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    got = {}
    with open(sys.argv[2] if len(sys.argv) > 2 else OUT, "a") as f:
        for run in range(runs):
            for build in ("parent", "this"):
                env = dict(os.environ, MSD_VARIANT="parent") if build == "parent" else {k: v for k, v in os.environ.items() if k != "MSD_VARIANT"}
                env["MSD_AB_CASES"] = ",".join(sys.argv[3:])
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=420)
                if p.returncode != 0:   # a failed process ends the job: nothing more is started on the GPU
                    sys.exit(f"{build} run {run}: exit code {p.returncode}\n{p.stderr[-2000:]}")
                print(f"{build} run {run} done", file=sys.stderr, flush=True)
                for line in p.stdout.splitlines():
                    if line.startswith("{"):
                        row = dict(json.loads(line), build=build, run=run)
                        got.setdefault(row["case"], {}).setdefault(build, []).append(row["ms"])
                        f.write(json.dumps(row) + "\n")
                        f.flush()
    for case, g in got.items():
        lo, hi, med = min(g["parent"]), max(g["parent"]), statistics.median(g["this"])
        where = "inside" if lo <= med <= hi else "inside the range widened by its spread" if lo - (hi - lo) <= med <= hi + (hi - lo) else "OUTSIDE"
        print(json.dumps({"case": case, "parent_ms": g["parent"], "this_ms": g["this"], "parent_range": [lo, hi], "this_median": med, "verdict": where}))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
