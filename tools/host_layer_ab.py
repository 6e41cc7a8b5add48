#!/usr/bin/env python3
"""Does a change of the host layer (msd_radix.hip outside the kernels) cost time?  Parent build against this one.

    python tools/host_layer_ab.py [runs [rows.jsonl]]          (needs libinpmsdradix_hip_parent.so: _build.build_variant("parent") on the parent's tree)

Alternates the two builds in one job, `runs` (default 3) fresh processes each.  A process measures, on one GPU:
  sort_u32_2^16, sort_u32_2^20   msd_sort_u32 on fresh uniform keys: median over 200 calls of the host clock around call + synchronise
  topk_rows_4x4096_f32_k8        msd_topk_rows, 4 rows of 4096 float32, k = 8: the same
  sort_rows_64x512_f32_idx       msd_sort_rows, 64 rows of 512 float32 with positions: the same, as all of the following
  run_encode_2^16_i32            msd_run_encode on 2^16 sorted int32 (values, starts)
  reduce_runs_sum_2^16_i64       msd_reduce_runs, the sum of int64 values over the runs of the same keys
  searchsorted_2^16_in_2^20_i32  msd_search_sorted, 2^16 unsorted needles in 2^20 sorted int32
  sort_typed_2^16_f32            msd_sort_keys on 2^16 float32 (a fresh copy of the same keys before every call)
  bench_2^30_u32                 bench.py's default line (ms_per_step of --steps 10 --warmup 2)
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

    def timed(call, before=None):
        ms = []
        for i in range(CALLS + 20):
            if before:
                before(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms[20:])                      # (the first 20 calls warm up)

    rows = {}
    for logn in (16, 20):
        t = torch.empty(1 << logn, dtype=torch.int32, device="cuda")
        rows[f"sort_u32_2^{logn}"] = timed(lambda: ctx.sort_u32(t), lambda i: ctx.gen_uniform_u32(t, seed=i))
        assert ctx.check(t)[0] == 0
    x = torch.randn(4, 4096, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    o = torch.empty(4, 8, device="cuda")
    rows["topk_rows_4x4096_f32_k8"] = timed(lambda: ctx.topk_rows(x, 8, out=o))
    # the typed entry points: one to four launches and no synchronisation of their own, so the call's time is host time
    g = torch.Generator("cuda").manual_seed(2)
    m = torch.randn(64, 512, device="cuda", generator=g)
    mo, mi = torch.empty_like(m), torch.empty(64, 512, dtype=torch.int64, device="cuda")
    rows["sort_rows_64x512_f32_idx"] = timed(lambda: ctx.sort_rows(m, out=mo, out_indices=mi))
    sk = torch.randint(0, 1 << 12, (1 << 16,), dtype=torch.int32, device="cuda", generator=g).sort().values
    sv = torch.arange(1 << 16, dtype=torch.int64, device="cuda")
    rows["run_encode_2^16_i32"] = timed(lambda: ctx.run_encode(sk))
    rows["reduce_runs_sum_2^16_i64"] = timed(lambda: ctx.reduce_runs(sk, sv))
    hay = torch.randint(-(1 << 30), 1 << 30, (1 << 20,), dtype=torch.int32, device="cuda", generator=g).sort().values
    needles = torch.randint(-(1 << 30), 1 << 30, (1 << 16,), dtype=torch.int32, device="cuda", generator=g)
    found = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    rows["searchsorted_2^16_in_2^20_i32"] = timed(lambda: ctx.searchsorted(hay, needles, out=found))
    f = torch.randn(1 << 16, device="cuda", generator=g)
    ft = torch.empty_like(f)
    rows["sort_typed_2^16_f32"] = timed(lambda: ctx.sort_typed(ft), lambda i: ft.copy_(f))
    ctx.close()
    buf = io.StringIO()
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"]
    with redirect_stdout(buf):
        runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
    rows["bench_2^30_u32"] = json.loads(buf.getvalue().strip().splitlines()[-1])["ms_per_step"]
    for case, ms in rows.items():
        print(json.dumps({"case": case, "ms": round(ms, 5)}), flush=True)


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    got = {}
    with open(sys.argv[2] if len(sys.argv) > 2 else OUT, "a") as f:
        for run in range(runs):
            for build in ("parent", "this"):
                env = dict(os.environ, MSD_VARIANT="parent") if build == "parent" else {k: v for k, v in os.environ.items() if k != "MSD_VARIANT"}
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
