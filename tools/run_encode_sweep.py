#!/usr/bin/env python3
"""Run-length encode (msd_run_encode) and MsdContext.unique on large sorted arrays, against torch.

    python tools/run_encode_sweep.py [--cells u32:28:uniform u32:28:zipf u32:30:uniform u32:30:zipf u64:30:uniform]
                                     [--out profiles/run_encode_sweep.jsonl] [--step-timeout 600]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

Per cell (key width : log2 n : distribution) the keys are generated on the device (msd_gen_uniform_* / msd_gen_zipf_u32), a
sorted copy is made with the library's own sort, and every way is timed with HIP events around the call: 5 warm-up calls,
then the median of 20 timed calls with the min-max spread.
    count        msd_run_encode with no optional output: steps 1 and 2 alone (one read of the input)
    encode       ... with values and starts
    encode_inv   ... with values, starts and the inverse
    encode_pos   ... with values, starts and the inverse through positions (a random permutation: the scattered stores)
    torch_uc     torch.unique_consecutive(sorted, return_counts=True)
    unique       MsdContext.unique(unsorted, return_counts=True): clone, sort, run_encode, one host read of the count
    torch_unique torch.unique(unsorted, return_counts=True)
`*_bytes` = two reads of the input plus the outputs written (encode: m values and m + 1 starts; the inverse: n words, with
positions n more words read); `*_TBps` = bytes / median time, to be set against the streaming ceiling of
profiles/r02_stream_ceiling.jsonl.  The result of `encode_inv` is checked against torch.unique_consecutive once per cell.
Tensors are int32 / int64 (torch has no unique for unsigned types): the typed sort inside `unique` pays its sign fix-up."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = ["u32:28:uniform", "u32:28:zipf", "u32:30:uniform", "u32:30:zipf", "u64:30:uniform"]
WARMUP, REPS = 5, 20


def measure(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
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
    es, n = (4 if width == "u32" else 8), 1 << int(logn)
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    x = torch.empty(n, dtype=torch.int32 if es == 4 else torch.int64, device="cuda")
    if es == 8:
        ctx.gen_uniform_u64(x)
    elif dist == "zipf":
        ctx.gen_zipf_u32(x)
    else:
        ctx.gen_uniform_u32(x)
    s = x.clone()
    (ctx.sort_u32 if es == 4 else ctx.sort_u64)(s)
    pos = torch.randperm(n, device="cuda")
    num, vals, st, inv = ctx.run_encode(s, inverse=True)
    m = int(num.item())
    tv, ti, tc = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    assert tv.numel() == m and torch.equal(tv, vals[:m]) and torch.equal(tc, st[1:m + 1] - st[:m]) and torch.equal(ti, inv), spec
    del tv, ti, tc, num, vals, st, inv
    torch.cuda.empty_cache()
    row = {"width": width, "log2_n": int(logn), "dist": dist, "n": n, "runs": m, "warmup": WARMUP, "reps": REPS}
    read2 = 2 * n * es
    ways = {
        "count": (lambda: ctx.run_encode(s, values=False, starts=False), n * es),
        "encode": (lambda: ctx.run_encode(s), read2 + m * (es + 8) + 8),
        "encode_inv": (lambda: ctx.run_encode(s, inverse=True), read2 + m * (es + 8) + 8 + 8 * n),
        "encode_pos": (lambda: ctx.run_encode(s, inverse=True, positions=pos), read2 + m * (es + 8) + 8 + 16 * n),
        "torch_uc": (lambda: torch.unique_consecutive(s, return_counts=True), None),
        "unique": (lambda: ctx.unique(x, return_counts=True), None),
        "torch_unique": (lambda: torch.unique(x, return_counts=True), None),
    }
    for name, (fn, nbytes) in ways.items():
        med, spread = measure(fn)
        row[name + "_ms"] = round(med, 4)
        row[name + "_ms_min_max"] = [round(v, 4) for v in spread]
        if nbytes is not None:
            row[name + "_bytes"] = nbytes
            row[name + "_TBps"] = round(nbytes / med / 1e9, 3)
        torch.cuda.empty_cache()
    ctx.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=CELLS)
    ap.add_argument("--cell", default=None, help="measure this one cell in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "run_encode_sweep.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one cell may take")
    a = ap.parse_args()
    if a.cell:
        cell(a.cell)
        return 0
    with open(a.out, "w") as out:
        for spec in a.cells:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cell", spec], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                   text=True, timeout=a.step_timeout)
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
