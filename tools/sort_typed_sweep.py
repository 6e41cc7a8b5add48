#!/usr/bin/env python3
"""The typed, two-way sort (msd_sort_keys) against the unsigned sort on the same bit patterns, and the reversal kernel alone.

    python tools/sort_typed_sweep.py [--logn 28 30] [--reps 5] [--out profiles/sort_typed_sweep.jsonl]
                                     [--stream-copy FILE]      # the output of tools/microbench/stream_copy, same job
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sort_typed_sweep.py --trace-pass --cells DIR/cells.json
    python tools/sort_typed_sweep.py --ingest DIR --cells DIR/cells.json --out profiles/sort_typed_sweep.jsonl --append

Cells: float32 N(0,1), float32 uniform [0,1), int32 random bits, int32 non-negative, float64 N(0,1) (one power of two fewer
elements: the same bytes), each ascending and descending.  Per cell: HIP events around the call, one warm-up, the median of
--reps runs with min-max, the ways alternating in one process, every way on a fresh copy of the same input:
    typed     msd_sort_keys
    unsigned  msd_sort_u32 / msd_sort_u64 on the same bit patterns: what the library could do before, the yardstick
    torch     torch.sort, for orientation
`table`: the ranges the header's table gives this input (from the counters), `reversed`: their summed length.
`nothing_inside`: for a cell whose table row is "nothing", does the typed median lie inside the min-max of the unsigned
runs?  The warm-up run of `typed` is compared with torch.sort's values.

Rows {"what": "reverse"}: msd_reverse on R[0,n) -- 16-byte aligned ends -- and on R[1,n-2), both ends off the 16-byte grid
in different ways; rate = 2 x bytes of the range / time.  {"what": "stream_copy"}: the best `copy` line of --stream-copy.

--trace-pass runs every cell's typed sort once (after one warm-up on a small array) and writes the cells' order; --ingest
reads rocprofv3's kernel trace of that run: a sign_split_kernel dispatch opens a cell's fix-up, the reverse_ranges_kernel
dispatches up to the next one are its reversals.  Rows {"what": "reverse_kernels"}: their summed time and rate."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CELLS = [("float32", "normal"), ("float32", "uniform"), ("int32", "bits"), ("int32", "nonneg"), ("float64", "normal")]


def make(torch, dtype, dist, n):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0051)
    dt = getattr(torch, dtype)
    if dist == "normal":
        return torch.randn(n, dtype=dt, device="cuda", generator=g)
    if dist == "uniform":
        return torch.rand(n, dtype=dt, device="cuda", generator=g)
    lo = 0 if dist == "nonneg" else -2**31
    return torch.randint(lo, 2**31, (n,), dtype=dt, device="cuda", generator=g)


def cells(logns):
    for logn in logns:
        for dtype, dist in CELLS:
            for descending in (False, True):
                yield {"dtype": dtype, "dist": dist, "log2n": logn - (dtype == "float64"), "descending": descending}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def med(row, name, t):
    row[name + "_ms"] = round(statistics.median(t), 4)
    row[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]


def ingest(a):
    order = json.load(open(a.cells))
    paths = glob.glob(os.path.join(a.ingest, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        sys.exit(f"expected one kernel trace under {a.ingest}, found {paths}")
    groups = []
    with open(paths[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        if "sign_split_kernel" in name:
            groups.append([])
        elif "reverse_ranges_kernel" in name and groups:
            groups[-1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    groups = groups[1:]   # (the warm-up's)
    if len(groups) != len(order):
        sys.exit(f"{len(groups)} fix-ups in the trace, {len(order)} cells")
    with open(a.out, "a" if a.append else "w") as out:
        for cell, ms in zip(order, groups):
            row = dict(cell, what="reverse_kernels", launches=len(ms), reverse_kernels_ms=round(sum(ms), 4), each_ms=[round(x, 4) for x in ms])
            if cell["reversed"]:
                row["rate_TBps"] = round(2 * cell["reversed"] * cell["elem_bytes"] / sum(ms) / 1e9, 3)
            print(json.dumps(row))
            out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="+", default=[28, 30])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--stream-copy", default=None)
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--cells", default=None)
    ap.add_argument("--ingest", default=None)
    a = ap.parse_args()
    if a.ingest:
        return ingest(a)
    import torch
    from inplacemsdradixsort_amd import MsdContext
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    out = open(a.out, "a" if a.append else "w") if a.out and not a.trace_pass else None

    def emit(row):
        print(json.dumps(row), flush=True)
        if out:
            out.write(json.dumps(row) + "\n")
            out.flush()

    if a.trace_pass:
        ctx.sort_typed(torch.randn(1 << 20, device="cuda"))
        order = []
    for cell in cells(a.logn):
        n = 1 << cell["log2n"]
        src = make(torch, cell["dtype"], cell["dist"], n)
        es = src.element_size()
        ctx.reserve(n, es)
        work = torch.empty_like(src)
        desc = cell["descending"]

        def typed():
            ctx.sort_typed(work, descending=desc)

        def unsigned():
            (ctx.sort_u32 if es == 4 else ctx.sort_u64)(work.view(torch.int32 if es == 4 else torch.int64))

        if a.trace_pass:
            work.copy_(src)
            typed()
            st = ctx.stats()
            order.append(dict(cell, elem_bytes=es, split=st["sort_keys_split"], reversed=st["sort_keys_reversed"]))
            del src, work
            torch.cuda.empty_cache()
            continue
        ways = {"typed": typed, "unsigned": unsigned}
        if not a.no_torch:
            ways["torch"] = lambda: torch.sort(src, descending=desc)
        for name, fn in ways.items():     # warm-up, and the check
            work.copy_(src)
            fn()
            if name == "typed":
                st = ctx.stats()
                if not a.no_torch:
                    ref = torch.sort(src, descending=desc).values
                    assert torch.equal(work, ref), cell
                    del ref
        t = {name: [] for name in ways}
        for _ in range(a.reps):
            for name, fn in ways.items():
                work.copy_(src)
                torch.cuda.synchronize()
                t[name].append(timed(torch, fn))
        row = dict(cell, what="sort", n=n, elem_bytes=es, reps=a.reps, split=st["sort_keys_split"], reversed=st["sort_keys_reversed"])
        for name in ways:
            med(row, name, t[name])
        row["typed_minus_unsigned_ms"] = round(row["typed_ms"] - row["unsigned_ms"], 4)
        if st["sort_keys_reversed"] == 0:
            lo, hi = row["unsigned_ms_min_max"]
            row["nothing_inside"] = bool(lo <= row["typed_ms"] <= hi)
        emit(row)
        del src, work
        torch.cuda.empty_cache()
    if a.trace_pass:
        json.dump(order, open(a.cells, "w"))
        ctx.close()
        return
    # ---- the reversal kernel alone
    for logn, dt in ((max(a.logn), torch.int32), (max(a.logn) - 1, torch.int64)):
        n = 1 << logn
        x = torch.arange(n, dtype=dt, device="cuda")
        es = x.element_size()
        for label, first, count in (("aligned", 0, n), ("misaligned", 1, n - 3)):
            ctx.reverse(x, first, count)
            t = [timed(torch, lambda: ctx.reverse(x, first, count)) for _ in range(a.reps)]
            row = {"what": "reverse", "elem_bytes": es, "n": n, "ends": label, "first": first, "count": count, "reps": a.reps}
            med(row, "reverse", t)
            row["rate_TBps"] = round(2 * count * es / row["reverse_ms"] / 1e9, 3)
            emit(row)
        del x
        torch.cuda.empty_cache()
    if a.stream_copy:
        best = None
        for line in open(a.stream_copy):
            try:
                r = json.loads(line)
            except ValueError:
                continue
            if r.get("kernel") == "copy" and (best is None or r["best_TBps"] > best["best_TBps"]):
                best = r
        if best:
            emit(dict(best, what="stream_copy"))
    ctx.close()


if __name__ == "__main__":
    main()
