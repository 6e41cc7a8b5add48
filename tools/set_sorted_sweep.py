#!/usr/bin/env python3
"""Set operations on two sorted arrays (msd_set_sorted) on large inputs, against the routes a caller had before.

    python tools/set_sorted_sweep.py [--cells u32:30:20:uniform u32:30:28:half ... u64:29:n:d10]
                                     [--out profiles/set_sorted_sweep.jsonl] [--append] [--step-timeout 600]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

A cell is key width : log2 n : log2 m (or `n` for m = n) : keys.  `uniform` and `d10` (2^10 distinct values) are the cells of
tools/merge_sorted_sweep.py: generated on the device (msd_gen_uniform_*), shifted right by one bit -- non-negative as int32 /
int64, so that torch's order and the library's agree -- and sorted with the library's own sort.  `half` (half_shared): A is
uniform, and half of B's elements are taken from A at equal strides, the other half uniform from another seed.

The ways of one cell are timed INTERLEAVED on the same tensors: every way is warmed up (2 calls; a way whose first call takes
more than 0.3 s: that call alone), then ROUNDS rounds run every way once, one after the other, each call between two HIP
events; a row holds the median and the min-max spread per way and what it was made with (`*_warmup`, `*_reps`).  The ways:
    union / intersection / difference            MsdContext.set_sorted(a, b, op, out=...)
    union_origin / ...                           ... with the origin output
    former_union                                 merge_sorted(a, b) then run_encode: the library's own route before
    former_intersection / former_difference      searchsorted(b, a) left and right (needles_sorted) and a torch mask over the
                                                 heads of A's runs; the boolean index waits on the host
    torch_union                                  torch.unique(torch.cat([a, b]))
    torch_intersection / torch_difference        torch.unique_consecutive of both and a torch.isin(..., assume_unique=True) mask
`*_bytes` of a set_sorted way = what it really moves: both inputs twice, the results once (8 bytes more per result with the
origin) -- an UPPER bound: a tile of the write pass that has nothing to store reads nothing, so where few results come out
(2^10 distinct values) the inputs are read little more than once and the figure is up to twice the real traffic; `*_TBps` =
bytes / median time, to be set against the copy ceiling of profiles/r02_stream_ceiling.jsonl.  A way that
raises (torch refuses more than 2^31 - 1 elements in a sort, or runs out of memory) is listed in `not_measured` with its
message.  Once per cell every result of set_sorted is compared exactly with the former route's.  The tool reads nothing but
what it generates."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = ["20", "28", "n"]
CELLS = [w + ":" + m + ":" + d for w in ("u32:30", "u64:29") for d in ("uniform", "d10", "half") for m in MS]
OPS = ("union", "intersection", "difference")
WARMUP, ROUNDS = 2, 7
SLOW_MS, SLOW_ROUNDS = 300.0, 3


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def cell(spec):
    import torch
    from inplacemsdradixsort_amd import MsdContext
    width, logn, logm, keys = spec.split(":")
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
        if keys == "d10":
            t.bitwise_and_(0x3FF)
        return t

    a = generate(n, 0x5EED0001)
    ctx.sort_typed(a)
    b = generate(m, 0x5EED0777)
    if keys == "half":
        b[:m // 2] = a[torch.arange(m // 2, device="cuda") * (n // (m // 2))]
    ctx.sort_typed(b)
    total = n + m
    row = {"width": width, "log2_n": int(logn), "n": n, "m": m, "log2_m": int(logn) if logm == "n" else int(logm), "keys": keys, "not_measured": {}}
    out = torch.empty(total, dtype=dt, device="cuda")
    oo = torch.empty(total, dtype=torch.int64, device="cuda")
    bound = {"union": total, "intersection": min(n, m), "difference": n}

    def former_union():
        num, values, _, _ = ctx.run_encode(ctx.merge_sorted(a, b), starts=False)
        return num, values

    def former_mask(keep_in_b):
        left = ctx.searchsorted(b, a, right=False, needles_sorted=True)
        right = ctx.searchsorted(b, a, right=True, needles_sorted=True)
        in_b = right > left
        del left, right
        head = torch.ones(n, dtype=torch.bool, device="cuda")
        head[1:] = a[1:] != a[:-1]
        return a[head & (in_b if keep_in_b else ~in_b)]

    def torch_mask(invert):
        ua, ub = torch.unique_consecutive(a), torch.unique_consecutive(b)
        return ua[torch.isin(ua, ub, assume_unique=True, invert=invert)]

    # the results once, exactly, against the former routes
    counts = {}
    for op in OPS:
        num, _, _ = ctx.set_sorted(a, b, op, cap=bound[op], out=out[:bound[op]], out_origin=oo[:bound[op]])
        g = counts[op] = int(num.item())
        if op == "union":
            fnum, want = former_union()
            assert int(fnum.item()) == g, (spec, op, "count", g, int(fnum.item()))
            want = want[:g]
        else:
            want = former_mask(op == "intersection")
        assert want.numel() == g and torch.equal(out[:g], want), (spec, op, "differs from the former route")
        origin = oo[:g]
        assert bool((torch.where(origin < n, a[origin.clamp(max=n - 1)], b[(origin - n).clamp(min=0)]) == out[:g]).all()), (spec, op, "origin does not lead to the keys")
        del want, origin
        torch.cuda.empty_cache()
        row[op + "_count"] = g

    ways = []
    for op in OPS:
        ways.append((op, lambda op=op: ctx.set_sorted(a, b, op, cap=bound[op], out=out[:bound[op]]), 2 * total * kb + counts[op] * kb))
        ways.append((op + "_origin", lambda op=op: ctx.set_sorted(a, b, op, cap=bound[op], out=out[:bound[op]], out_origin=oo[:bound[op]]),
                     2 * total * kb + counts[op] * (kb + 8)))
    ways += [("former_union", former_union, None), ("former_intersection", lambda: former_mask(True), None), ("former_difference", lambda: former_mask(False), None),
             ("torch_union", lambda: torch.unique(torch.cat([a, b])), None), ("torch_intersection", lambda: torch_mask(False), None),
             ("torch_difference", lambda: torch_mask(True), None)]

    live, times, made = [], {}, {}
    for name, fn, nbytes in ways:                                   # warm-up, every way
        try:
            first = timed(fn)
            slow = first > SLOW_MS
            for _ in range(0 if slow else WARMUP - 1):
                fn()
            torch.cuda.synchronize()
        except Exception as e:                                      # (torch: too many elements for its sort, or out of memory)
            row["not_measured"][name] = (type(e).__name__ + ": " + str(e).splitlines()[0])[:200]
            torch.cuda.synchronize()                                # (a fault of the device is no refusal: it raises again here and ends the cell)
            torch.cuda.empty_cache()
            continue
        live.append((name, fn, nbytes))
        times[name], made[name] = [], (1 if slow else WARMUP, SLOW_ROUNDS if slow else ROUNDS)
        torch.cuda.empty_cache()
    for r in range(ROUNDS):                                         # the timed calls, interleaved
        for name, fn, _ in live:
            if r < made[name][1]:
                times[name].append(timed(fn))
                torch.cuda.empty_cache()
    for name, _, nbytes in live:
        t = times[name]
        med = statistics.median(t)
        row[name + "_ms"] = round(med, 4)
        row[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        row[name + "_warmup"], row[name + "_reps"] = made[name][0], len(t)
        if nbytes:
            row[name + "_bytes"] = nbytes
            row[name + "_bytes_per_elem"] = round(nbytes / total, 3)
            row[name + "_TBps"] = round(nbytes / med / 1e9, 3)
    ctx.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=CELLS)
    ap.add_argument("--cell", default=None, help="measure this one cell in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_sorted_sweep.jsonl"))
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of starting it anew")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one cell may take")
    a = ap.parse_args()
    if a.cell:
        cell(a.cell)
        return 0
    with open(a.out, "a" if a.append else "w") as out:
        for spec in a.cells:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", spec]
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
