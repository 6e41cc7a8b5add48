#!/usr/bin/env python3
"""Per-row top-k (msd_topk_rows): the row kernel against the loop over msd_topk_keys, and what mode 0 makes of it.

    python tools/topk_rows_sweep.py [--shapes 8388608x64 4096x131072 ...] [--k 1 8 64 1024] [--dist normal uniform]
                                    [--dtype float32 int64] [--idx 0 1] [--out profiles/topk_rows_sweep.jsonl]

Per cell (shape, dtype, distribution, k, with / without indices): HIP events around the call, one warm-up, the median of
--reps runs with the min-max spread, the ways alternating in one process (a way that is one kernel launch runs twice in
its turn and the second run is timed: right behind the loop's many small launches and host waits the same launch measured
up to twice as long):
    mode0   msd_topk_rows as shipped ("topk_rows_mode" 0), and which way it took (the msd_stat counters)
    mode2   always the row kernel (inside its envelope)
    mode1   always the loop over msd_topk_keys: what the library could do for this call before msd_topk_rows existed.
            Timed on the first --loop-rows rows where the matrix has more (`loop_rows_timed`; `mode1_ms` is then that time
            scaled by rows / loop_rows_timed -- the loop's cost is per row -- and `mode1_scaled` says so)
    torch   torch.topk(x, k, dim=1), for orientation (its output order differs for "largest")
    lanesN  (--lanes) mode 2 with N lanes per row forced ("topk_rows_lanes"): what the thresholds between the kernel's three
            shapes are fitted to
`rate2_TBps` = rows * row_len * element bytes * 2 / mode2 time: the row kernel's rate if it reads every row twice (one
counting pass and the filter; evenly spread inputs.  The kernel does not report its passes).  The mode 2 result is checked
against torch.sort once per cell.  `mode0_ok`: mode 0 is not slower than the faster of mode 1 and mode 2 by more than its
own min-max spread."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from inplacemsdradixsort_amd import MsdContext, MsdError  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make(rows, n, dtype, dist):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0041)
    if dtype == "int64":
        return torch.randint(-2**62, 2**62, (rows, n), dtype=torch.int64, device="cuda", generator=g)
    if dist == "normal":
        return torch.randn(rows, n, dtype=torch.float32, device="cuda", generator=g)
    return torch.rand(rows, n, dtype=torch.float32, device="cuda", generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["8388608x64", "131072x4096", "4096x131072", "512x1048576", "8x67108864",
                                                    "262144x64", "4096x4096", "128x131072", "16x1048576"])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 8, 64, 1024])
    ap.add_argument("--dist", nargs="+", default=["normal", "uniform"])
    ap.add_argument("--dtype", nargs="+", default=["float32"], choices=["float32", "int64"])
    ap.add_argument("--idx", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--largest", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-rows", type=int, default=4096, help="mode 1 is timed on at most this many rows")
    ap.add_argument("--lanes", type=int, nargs="*", default=[], help="also time mode 2 with these lanes per row forced (64, 256, 1024)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    out = open(a.out, "a" if a.append else "w") if a.out else None
    largest = bool(a.largest)
    for shape in a.shapes:
        rows, n = (int(v) for v in shape.split("x"))
        for dtype in a.dtype:
            for dist in (a.dist if dtype == "float32" else ["bits"]):
                x = make(rows, n, dtype, dist)
                es = x.element_size()
                s = torch.sort(x[:min(rows, 64)], dim=1).values      # (the check: the first rows)
                for k in a.k:
                    if k > n:
                        continue
                    for idx in a.idx:
                        max_len, max_k = ctx.topk_rows_limits(x, bool(idx))
                        inside = n <= max_len and k <= max_k
                        lr = min(rows, a.loop_rows)
                        ov = torch.empty(rows, k, dtype=x.dtype, device="cuda")
                        oi = torch.empty(rows, k, dtype=torch.int64, device="cuda") if idx else None

                        def call(mode, r=rows, lanes=0):
                            ctx.set_option("topk_rows_mode", mode)
                            ctx.set_option("topk_rows_lanes", lanes)
                            ctx.topk_rows(x[:r], k, largest=largest, out=ov[:r], out_indices=oi[:r] if idx else None)

                        ways = {"mode0": lambda: call(0), "mode1": lambda: call(1, lr)}
                        if inside:
                            ways["mode2"] = lambda: call(2)
                            for ln in a.lanes:
                                if ln != 64 or n <= 512:
                                    ways["lanes%d" % ln] = lambda ln=ln: call(2, rows, ln)
                        if not a.no_torch and k <= n:
                            ways["torch"] = lambda: torch.topk(x, k, dim=1, largest=largest, sorted=True)
                        try:
                            for name, fn in ways.items():   # warm-up, and the check of the kernel's result
                                fn()
                                if name == ("mode2" if inside else "mode0"):
                                    got = ov[:s.shape[0]]
                                    assert torch.equal(got, s[:, n - k:] if largest else s[:, :k]), (shape, k, idx)
                                    if idx:
                                        assert torch.equal(torch.gather(x[:s.shape[0]], 1, oi[:s.shape[0]]), got), (shape, k, idx)
                                if name == "mode0":
                                    st = ctx.stats()
                                    took = "kernel" if st.get("topk_rows_kernel_rows") else "loop"
                            t = {name: [] for name in ways}
                            for _ in range(a.reps):             # alternating, same process
                                for name, fn in ways.items():
                                    if name != "mode1" and name != "torch" and not (name == "mode0" and took == "loop"):
                                        fn()                    # (behind the host-blocking loop the clocks have dropped: a kernel way runs twice, the second run counts)
                                    t[name].append(timed(fn))
                        finally:
                            ctx.set_option("topk_rows_mode", 0)
                            ctx.set_option("topk_rows_lanes", 0)
                        row = {"rows": rows, "row_len": n, "dtype": dtype, "dist": dist, "k": k, "idx": bool(idx), "largest": largest,
                               "mode0_took": took, "loop_rows_timed": lr, "mode1_scaled": lr < rows, "reps": a.reps}
                        for name in ways:
                            m = statistics.median(t[name])
                            scale = rows / lr if name == "mode1" else 1.0
                            row[name + "_ms"] = round(m * scale, 4)
                            row[name + "_ms_min_max"] = [round(min(t[name]) * scale, 4), round(max(t[name]) * scale, 4)]
                        if inside:
                            row["rate2_TBps"] = round(rows * n * es * 2 / row["mode2_ms"] / 1e9, 3)
                        best = min(row["mode1_ms"], row.get("mode2_ms", float("inf")))
                        spread = row["mode0_ms_min_max"][1] - row["mode0_ms_min_max"][0]
                        row["mode0_ok"] = bool(row["mode0_ms"] <= best + spread)
                        line = json.dumps(row)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
                        del ov, oi
                del x, s
                torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    try:
        main()
    except MsdError as e:
        sys.exit(str(e))
