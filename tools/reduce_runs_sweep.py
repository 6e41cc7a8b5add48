#!/usr/bin/env python3
"""Reduce-by-key over runs (msd_reduce_runs) on large sorted key arrays, against torch.

    python tools/reduce_runs_sweep.py [--cells u32:28:uniform u32:28:zipf u32:28:equal u32:30:uniform u32:30:zipf u32:30:equal u64:30:uniform]
                                      [--out profiles/reduce_runs_sweep.jsonl] [--append] [--step-timeout 900]
                                      [--torch-warmup 2] [--torch-reps 5] [--skip scat ...]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

Per cell (key width : log2 n : distribution) the keys are generated on the device (msd_gen_uniform_* / msd_gen_zipf_u32, or
one value for `equal`) and sorted with the library's own sort; the value columns are float32 N(0,1) and int64 from
[-2^40, 2^40).  Every way is timed with HIP events around the call: 3 warm-up calls, then the median of 10 timed calls with
the min-max spread.  torch's ways get --torch-warmup and --torch-reps calls (2 and 5) and can be left out by a part of their
name (--skip): on keys with few distinct values their atomics take seconds per call.  Every row says what it was made with.
For each value column `f32` / `i64` and each op `sum` / `min` / `max`:
    <val>_<op>          msd_reduce_runs, the values in the order of the keys
    <val>_<op>_pos      ... read through positions (a random permutation: the gather)
    <val>_<op>_seg      torch.segment_reduce(values, op, lengths=...) on the lengths of a run_encode made beforehand
    <val>_<op>_scat     zeros(m).index_add_(0, inverse, values) for a sum, else empty(m).scatter_reduce_(0, inverse, values,
                        "amin" / "amax", include_self=False), on the inverse of a run_encode made beforehand
    <val>_<op>_scat_pos ... on the inverse through the positions, the values where they lie (the group-by without a gather)
A way torch refuses (a dtype an op does not take, a launch that is too large) is recorded as `<way>_error`.  `*_bytes` =
the keys twice, the values once, the positions once where they are used, and m outputs; `*_TBps` = bytes / median time, to
be set against the streaming ceiling of profiles/r02_stream_ceiling.jsonl.  Once per cell the int64 sums are compared with index_add_ (exact) and the
float32 minima and maxima with scatter_reduce_ (no NaNs in the values: the orders agree)."""
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
OPS = ("sum", "min", "max")


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


def cell(spec, torch_warmup, torch_reps, skip):
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
    lengths = (st[1:m + 1] - st[:m]).contiguous()
    del st
    _, _, _, inv_pos = ctx.run_encode(s, values=False, starts=False, inverse=True, positions=pos)
    vals = {"f32": torch.randn(n, device="cuda"), "i64": torch.randint(-(1 << 40), 1 << 40, (n,), device="cuda")}
    row = {"width": width, "log2_n": int(logn), "dist": dist, "n": n, "runs": m, "warmup": WARMUP, "reps": REPS, "torch_warmup": torch_warmup,
           "torch_reps": torch_reps, "skipped": list(skip)}

    # the results once: exact against torch where the orders agree
    _, ours = ctx.reduce_runs(s, vals["i64"])
    assert torch.equal(ours[:m], torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, inv, vals["i64"])), spec
    _, ours = ctx.reduce_runs(s, vals["i64"], positions=pos)
    assert torch.equal(ours[:m], torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, inv_pos, vals["i64"])), spec
    for op, name in (("min", "amin"), ("max", "amax")):
        _, ours = ctx.reduce_runs(s, vals["f32"], op=op, positions=pos)
        want = torch.empty(m, device="cuda").scatter_reduce_(0, inv_pos, vals["f32"], name, include_self=False)
        assert torch.equal(ours[:m], want), (spec, op)
    del ours, want
    torch.cuda.empty_cache()

    def scatter(v, op, index):
        if op == "sum":
            return torch.zeros(m, dtype=v.dtype, device="cuda").index_add_(0, index, v)
        return torch.empty(m, dtype=v.dtype, device="cuda").scatter_reduce_(0, index, v, "amin" if op == "min" else "amax", include_self=False)

    for vname, v in vals.items():
        vb = v.element_size()
        for op in OPS:
            ob = 8 if op == "sum" else vb
            moved = 2 * n * kb + n * vb + m * ob
            ways = {
                "": (lambda: ctx.reduce_runs(s, v, op=op, cap=m), moved),
                "_pos": (lambda: ctx.reduce_runs(s, v, op=op, positions=pos, cap=m), moved + 8 * n),
                "_seg": (lambda: torch.segment_reduce(v, op, lengths=lengths), None),
                "_scat": (lambda: scatter(v, op, inv), None),
                "_scat_pos": (lambda: scatter(v, op, inv_pos), None),
            }
            for suffix, (fn, nbytes) in ways.items():
                name = "%s_%s%s" % (vname, op, suffix)
                if nbytes is None and any(part in name for part in skip):
                    continue
                if nbytes is not None:
                    med, spread = measure(fn)
                else:
                    try:
                        med, spread = measure(fn, torch_warmup, torch_reps)
                    except (RuntimeError, NotImplementedError, TypeError) as e:
                        text = str(e).splitlines()[0][:160]
                        if not any(w in text for w in ("not implemented", "not supported", "xpected", "dtype", "only support", "invalid configuration")):
                            raise                                       # (anything but a refusal -- of the dtype, the op, or of the launch: a
                                                                        # grid torch sizes by the segments can be too large -- ends the cell)
                        row[name + "_error"] = text
                        continue
                row[name + "_ms"] = round(med, 4)
                row[name + "_ms_min_max"] = [round(x, 4) for x in spread]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_runs_sweep.jsonl"))
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of starting it anew")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one cell may take")
    ap.add_argument("--torch-warmup", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[], help="leave out torch's ways whose name holds one of these (scat, f32_min_scat, ...)")
    a = ap.parse_args()
    if a.cell:
        cell(a.cell, a.torch_warmup, a.torch_reps, a.skip)
        return 0
    with open(a.out, "a" if a.append else "w") as out:
        for spec in a.cells:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cell", spec, "--torch-warmup", str(a.torch_warmup), "--torch-reps",
                                    str(a.torch_reps), "--skip", *a.skip], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
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
