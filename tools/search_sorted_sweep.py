#!/usr/bin/env python3
"""Sorted search (msd_search_sorted) into large sorted key arrays, against torch.searchsorted.

    python tools/search_sorted_sweep.py [--cells u32:30:10 u32:30:16 ... u32:30:n u64:29:10 ... u64:29:n]
                                        [--right-cells u32:30:24] [--out profiles/search_sorted_sweep.jsonl] [--append]
                                        [--step-timeout 600]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

A cell is key width : log2 n : log2 m (or `n` for m = n).  The keys are generated on the device (msd_gen_uniform_*), shifted
right by one bit -- non-negative as int32 / int64, so that torch's order and the library's agree and torch.searchsorted is a
fair opponent on the same tensors -- and sorted with the library's own sort; the needles are m more of the same, unsorted,
and a sorted copy of them.  Every way is timed with HIP events around the call: 3 warm-up calls, then the median of 10 timed
calls with the min-max spread.  A torch way whose first call takes more than 0.3 s gets that call as its only warm-up and 3
timed calls; every row says what each way was made with (`*_warmup`, `*_reps`).  The ways, all LEFT:
    direct_unsorted        MsdContext.searchsorted on the unsorted needles: the direct path
    sortneedles_unsorted   ... with sort_needles=True, end to end: the sort with positions, then the merge path through them
    direct_sorted          the sorted needles, needles_sorted=True, search_mode 1: the direct path
    merge_sorted           ... search_mode 2: the merge path
    merge_sorted_right     ... right=True (only in --right-cells: it costs the same)
    auto_sorted            ... search_mode 0: the library's choice, with the R it was built with
    torch_unsorted / torch_sorted    torch.searchsorted on the same tensors
`merge_sorted_bytes` = (n + m) keys once and 8 m bytes of results; `merge_sorted_TBps` = bytes / median time, to be set against
the copy ceiling of profiles/r02_stream_ceiling.jsonl.  Once per cell every way of the library is compared with torch's
result (exact).  The tool reads nothing but what it generates.  (The committed file also holds the rows of
`--cells u32:30:25 u32:30:26 u64:29:25 u64:29:26 --right-cells --append`: they pin the crossover between the two paths.)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = ["10", "16", "20", "24", "28", "n"]
CELLS = ["u32:30:" + m for m in MS] + ["u64:29:" + m for m in MS]
RIGHT_CELLS = ["u32:30:24"]
WARMUP, REPS = 3, 10
SLOW_MS, SLOW_REPS = 300.0, 3


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, adaptive=False):
    """(median ms, [min, max], warm-up calls, timed calls)"""
    import torch
    first = timed(fn)
    warmup, reps = (1, SLOW_REPS) if adaptive and first > SLOW_MS else (WARMUP, REPS)
    for _ in range(warmup - 1):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn) for _ in range(reps)]
    return statistics.median(t), [min(t), max(t)], warmup, reps


def cell(spec, right):
    import torch
    from inplacemsdradixsort_amd import MsdContext
    width, logn, logm = spec.split(":")
    kb, n = (4 if width == "u32" else 8), 1 << int(logn)
    m = n if logm == "n" else 1 << int(logm)
    dt = torch.int32 if kb == 4 else torch.int64
    ctx = MsdContext(0)
    ctx.use_torch_stream()

    def generate(count, seed):
        t = torch.empty(count, dtype=dt, device="cuda")
        if kb == 4:
            ctx.gen_uniform_u32(t, seed=seed)
            t.bitwise_right_shift_(1).bitwise_and_(0x7FFFFFFF)
        else:
            ctx.gen_uniform_u64(t, seed=seed, shift_right=1)
        return t

    s = generate(n, 0x5EED0001)
    ctx.sort_typed(s)
    x = generate(m, 0x5EED0777)
    xs = x.clone()
    ctx.sort_typed(xs)
    row = {"width": width, "log2_n": int(logn), "n": n, "m": m, "log2_m": int(logn) if logm == "n" else int(logm), "side": "left"}

    def ours(needles, mode, **kw):
        ctx.set_option("search_mode", mode)
        return ctx.searchsorted(s, needles, **kw)

    ways = {
        "direct_unsorted": lambda: ours(x, 0),
        "sortneedles_unsorted": lambda: ours(x, 0, sort_needles=True),
        "direct_sorted": lambda: ours(xs, 1, needles_sorted=True),
        "merge_sorted": lambda: ours(xs, 2, needles_sorted=True),
        "auto_sorted": lambda: ours(xs, 0, needles_sorted=True),
    }
    if right:
        ways["merge_sorted_right"] = lambda: ours(xs, 2, needles_sorted=True, right=True)
    torch_ways = {"torch_unsorted": lambda: torch.searchsorted(s, x), "torch_sorted": lambda: torch.searchsorted(s, xs)}

    # the results once: exact against torch (the orders agree on these keys)
    want_u, want_s = torch_ways["torch_unsorted"](), torch_ways["torch_sorted"]()
    for name, fn in ways.items():
        want = torch.searchsorted(s, xs, right=True) if name.endswith("_right") else want_u if name.endswith("_unsorted") else want_s
        assert torch.equal(fn(), want), (spec, name)
    del want_u, want_s, want
    torch.cuda.empty_cache()

    for name, fn in list(ways.items()) + list(torch_ways.items()):
        med, spread, warmup, reps = measure(fn, adaptive=name.startswith("torch"))
        row[name + "_ms"] = round(med, 4)
        row[name + "_ms_min_max"] = [round(v, 4) for v in spread]
        row[name + "_warmup"], row[name + "_reps"] = warmup, reps
        if name.startswith("merge_sorted"):
            row[name + "_bytes"] = (n + m) * kb + 8 * m
            row[name + "_TBps"] = round(row[name + "_bytes"] / med / 1e9, 3)
        torch.cuda.empty_cache()
    ctx.set_option("search_mode", 0)
    ctx.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=CELLS)
    ap.add_argument("--right-cells", nargs="*", default=RIGHT_CELLS, help="cells that also time the merge path with right=True")
    ap.add_argument("--cell", default=None, help="measure this one cell in this process (what the driver starts)")
    ap.add_argument("--right", action="store_true", help="with --cell: also time right=True")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_sorted_sweep.jsonl"))
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of starting it anew")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one cell may take")
    a = ap.parse_args()
    if a.cell:
        cell(a.cell, a.right)
        return 0
    with open(a.out, "a" if a.append else "w") as out:
        for spec in a.cells:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", spec] + (["--right"] if spec in a.right_cells else [])
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.step_timeout)
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
