#!/usr/bin/env python3
"""Scan-by-key over runs (msd_scan_runs) on large sorted key arrays, against msd_reduce_runs and torch.

    python tools/scan_runs_sweep.py [--cells u32:28:uniform u32:28:zipf u32:28:equal u32:30:uniform u32:30:zipf u32:30:equal u64:30:uniform]
                                    [--out profiles/scan_runs_sweep.jsonl] [--append] [--step-timeout 900]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

Per cell (key width : log2 n : distribution) the keys are generated on the device (msd_gen_uniform_* / msd_gen_zipf_u32, or
one value for `equal`) and sorted with the library's own sort; the value columns are float32 N(0,1) and int64 from
[-2^40, 2^40).  Every way is timed with HIP events around the call: 3 warm-up calls, then the median of 10 timed calls with
the min-max spread.  For each value column `f32` / `i64` and each op `sum` / `max`, and once for `count` (no values):
    <val>_<op>              msd_scan_runs, inclusive, the values in the order of the keys
    <val>_<op>_gather       ... on top of `values[positions]` (a random permutation) made by torch first: what a caller pays
                            today for a value column that did not move with the keys (msd_scan_runs does not offer positions yet)
    <val>_<op>_reduce       (a) msd_reduce_runs on the same tensors: the floor -- the same reads, m outputs instead of n
    <val>_sum_torch         (b) torch's route to a segmented sum: c = cumsum(values); c - (c[starts] - values[starts])[inverse]
                            on the starts and the inverse of a run_encode made beforehand
    <val>_max_cummax        (c) torch.cummax(values), UNSEGMENTED: it computes something else and is a floor only
`*_bytes` = the keys twice, the values twice and n outputs (the call alone: none for the `_gather` rows); `*_TBps` = bytes / median time, to be set against the copy ceiling of
profiles/r02_stream_ceiling.jsonl.  Once per cell the int64 sums are compared with torch's route (exact), the float32 maxima
with a segmented maximum built from the reduce (at every run's last element) and the counts with the starts."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = ["u32:28:uniform", "u32:28:zipf", "u32:28:equal", "u32:30:uniform", "u32:30:zipf", "u32:30:equal", "u64:30:uniform"]
WARMUP, REPS = 3, 10


def measure(fn, warmup=WARMUP, reps=REPS):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t), [min(t), max(t)]


def cell(spec):
    import torch
    from inplacemsdradixsort_amd import MsdContext
    width, logn, dist = spec.split(":")
    kb, n = (4 if width == "u32" else 8), 1 << int(logn)
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    s = torch.empty(n, dtype=torch.int32 if kb == 4 else torch.int64, device="cuda")
    if dist == "equal":
        s.fill_(7)
    elif kb == 8:
        ctx.gen_uniform_u64(s)
    elif dist == "zipf":
        ctx.gen_zipf_u32(s)
    else:
        ctx.gen_uniform_u32(s)
    if dist != "equal":
        (ctx.sort_u32 if kb == 4 else ctx.sort_u64)(s)
    pos = torch.randperm(n, device="cuda")
    num, _, st, inv = ctx.run_encode(s, values=False, inverse=True)
    m = int(num.item())
    starts = st[:m].contiguous()
    last = (st[1:m + 1] - 1).contiguous()
    del st
    vals = {"f32": torch.randn(n, device="cuda"), "i64": torch.randint(-(1 << 40), 1 << 40, (n,), device="cuda")}
    row = {"width": width, "log2_n": int(logn), "dist": dist, "n": n, "runs": m, "warmup": WARMUP, "reps": REPS}

    def torch_sum(v):
        c = torch.cumsum(v, 0)
        return c - (c[starts] - v[starts])[inv]

    # the results once: exact against torch where the orders agree
    ours = ctx.scan_runs(s, vals["i64"])
    assert torch.equal(ours, torch_sum(vals["i64"])), spec
    assert torch.equal(ctx.scan_runs(s, vals["i64"], exclusive=True) + vals["i64"], ours), spec
    ours = ctx.scan_runs(s, vals["f32"], op="max")
    assert torch.equal(ours[last], ctx.reduce_runs(s, vals["f32"], op="max", cap=m)[1]) and bool((ours >= vals["f32"]).all()), spec
    ours = ctx.scan_runs(s, None, op="count")
    assert torch.equal(ours[last], last - starts + 1) and bool((ours[starts] == 1).all()), spec
    del ours
    torch.cuda.empty_cache()

    def timed(name, fn, nbytes=None):
        med, spread = measure(fn)
        row[name + "_ms"] = round(med, 4)
        row[name + "_ms_min_max"] = [round(x, 4) for x in spread]
        if nbytes is not None:
            row[name + "_bytes"] = nbytes
            row[name + "_TBps"] = round(nbytes / med / 1e9, 3)
        torch.cuda.empty_cache()

    def ours_three(name, v, op, vb, ob):
        moved = 2 * n * kb + 2 * n * vb + n * ob
        timed(name, lambda: ctx.scan_runs(s, v, op=op), moved)
        if v is not None:
            timed(name + "_gather", lambda: ctx.scan_runs(s, v[pos], op=op))

    for vname, v in vals.items():
        vb = v.element_size()
        for op in ("sum", "max"):
            name = "%s_%s" % (vname, op)
            ours_three(name, v, op, vb, 8 if op == "sum" else vb)
            timed(name + "_reduce", lambda: ctx.reduce_runs(s, v, op=op, cap=m), 2 * n * kb + n * vb + m * (8 if op == "sum" else vb))
        timed(vname + "_sum_torch", lambda: torch_sum(v))
        timed(vname + "_max_cummax", lambda: torch.cummax(v, 0))
    ours_three("count", None, "count", 0, 8)
    ctx.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=CELLS)
    ap.add_argument("--cell", default=None, help="measure this one cell in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_runs_sweep.jsonl"))
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of starting it anew")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one cell may take")
    a = ap.parse_args()
    if a.cell:
        cell(a.cell)
        return 0
    with open(a.out, "a" if a.append else "w") as out:
        for spec in a.cells:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cell", spec], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                   timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print("cell %s ran into its time limit of %d s: stopping" % (spec, a.step_timeout), flush=True)
                return 1
            rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
            if p.returncode != 0 or len(rows) != 1:
                print(p.stdout[-4000:])
                print("cell %s failed with status %d: stopping" % (spec, p.returncode), flush=True)
                return 1
            print(rows[0], flush=True)
            out.write(rows[0] + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
