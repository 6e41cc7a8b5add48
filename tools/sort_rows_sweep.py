#!/usr/bin/env python3
"""Per-row sort (msd_sort_rows): the row kernel against the segment path, what mode 0 makes of it, and what the library could
do for the same matrix before msd_sort_rows existed.

    python tools/sort_rows_sweep.py [--shapes 8388608x64 1048576x512 ...] [--dtype float32 int64] [--idx 0 1] [--desc 0 1]
                                    [--lanes 64 256 1024] [--out profiles/sort_rows_sweep.jsonl]

Per cell (shape, dtype, direction, with / without positions): HIP events around the call, one warm-up, the median of --reps
runs with the min-max spread, the ways alternating in one process (a msd_sort_rows way runs twice in its turn and the second
run is timed: right behind a host-blocking way the same launch measured up to 5 % longer):
    mode0     msd_sort_rows as shipped ("sort_rows_mode" 0), and which way it took (the msd_stat counters)
    mode2     always the row kernel (inside its envelope)
    mode1     always the segment path (it needs 16-byte aligned outputs, which these are)
    segments  msd_sort_u32_segments / msd_sort_u64_segments on the same bit patterns, in place on a copy (the copy is not
              timed): what one call could do before -- unsigned order only, ascending only, no positions
    loop      a loop over msd_sort_keys, one host-blocking typed sort per row, in place on a copy: timed on the first
              --loop-rows rows (`loop_rows_timed`) and scaled by rows / loop_rows_timed (`loop_scaled`)
    torch     torch.sort(x, dim=-1), for orientation
    lanesN    (--lanes) mode 2 with N lanes per row forced ("sort_rows_lanes"): what the rule between the kernel's three
              shapes is fitted to
`rate_TBps` = rows * row_len * (2 * key bytes + 8 with positions) / time of the fastest of mode 2 and mode 1: every key read
once and written once, every position written once.  The result of the first way that runs is checked against torch.sort on
the first rows once per cell.  `mode0_ok`: mode 0 is not slower than the faster of mode 1 and mode 2 by more than its own
min-max spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from inplacemsdradixsort_amd import MsdContext, MsdError  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make(rows, n, dtype):
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0051)
    if dtype == "int64":
        return torch.randint(-2**63, 2**63 - 1, (rows, n), dtype=torch.int64, device="cuda", generator=g)
    return torch.randn(rows, n, dtype=torch.float32, device="cuda", generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["8388608x64", "1048576x512", "131072x4096", "32768x16384", "4096x131072",
                                                    "262144x64", "32768x512", "4096x4096", "1024x16384"])
    ap.add_argument("--dtype", nargs="+", default=["float32", "int64"], choices=["float32", "int64"])
    ap.add_argument("--idx", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--desc", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-rows", type=int, default=256, help="the loop over msd_sort_keys is timed on at most this many rows")
    ap.add_argument("--lanes", type=int, nargs="*", default=[], help="also time mode 2 with these lanes per row forced (64, 256, 1024)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    out = open(a.out, "a" if a.append else "w") if a.out else None
    for shape in a.shapes:
        rows, n = (int(v) for v in shape.split("x"))
        for dtype in a.dtype:
            r_eff = rows // 2 if dtype == "int64" else rows         # int64 at half the rows: the same bytes
            x = make(r_eff, n, dtype)
            es = x.element_size()
            nchk = min(r_eff, 64)
            ov = torch.empty_like(x)
            oi = torch.empty(r_eff, n, dtype=torch.int64, device="cuda")
            work = torch.empty_like(x)
            offs = np.arange(r_eff + 1, dtype=np.uint64) * np.uint64(n)     # (handed to the library as they are: no list of 2^23 ints per call)
            offs_p = offs.ctypes.data_as(C.POINTER(C.c_uint64))
            seg_fn = ctx._L.msd_sort_u32_segments if es == 4 else ctx._L.msd_sort_u64_segments
            lr = min(r_eff, a.loop_rows)
            for desc in a.desc:
                s = torch.sort(x[:nchk], dim=1, descending=bool(desc)).values      # (the check: the first rows)
                for idx in a.idx:
                    inside = n <= ctx.sort_rows_limits(x, bool(idx))

                    def call(mode, lanes=0):
                        ctx.set_option("sort_rows_mode", mode)
                        ctx.set_option("sort_rows_lanes", lanes)
                        ctx.sort_rows(x, descending=bool(desc), out=ov, out_indices=oi if idx else None)

                    def segments():
                        ctx._ok(seg_fn(ctx._h, C.c_void_p(work.data_ptr()), r_eff * n, offs_p, r_eff, es * 8))

                    def loop():
                        for r in range(lr):
                            ctx.sort_typed(work[r], descending=bool(desc))

                    ways = {"mode0": lambda: call(0), "mode1": lambda: call(1)}
                    if inside:
                        ways["mode2"] = lambda: call(2)
                        for ln in a.lanes:
                            if (ln != 64 or n <= 512) and (ln != 256 or n <= 4096):
                                ways["lanes%d" % ln] = lambda ln=ln: call(2, ln)
                    ways["segments"] = segments
                    if not a.no_loop and (n * es) % 16 == 0:
                        ways["loop"] = loop
                    if not a.no_torch:
                        ways["torch"] = lambda: torch.sort(x, dim=-1, descending=bool(desc))
                    in_place = ("segments", "loop")
                    try:
                        took = "?"
                        for name, fn in ways.items():   # warm-up, and the check of the result
                            if name in in_place:
                                work.copy_(x)
                            fn()
                            if name in ("mode0", "mode1", "mode2"):
                                assert torch.equal(ov[:nchk], s), (shape, dtype, desc, idx, name)
                                if idx:
                                    assert torch.equal(torch.gather(x[:nchk], 1, oi[:nchk]), s), (shape, dtype, desc, idx, name)
                            if name == "mode0":
                                st = ctx.stats()
                                took = "kernel" if st.get("sort_rows_kernel_rows") else "segments"
                        t = {name: [] for name in ways}
                        for _ in range(a.reps):             # alternating, same process
                            for name, fn in ways.items():
                                if name in in_place:
                                    work.copy_(x)
                                    torch.cuda.synchronize()
                                elif name != "torch":
                                    fn()                    # (behind the host-blocking ways the clocks have dropped: a msd_sort_rows way runs twice, the second run counts)
                                t[name].append(timed(fn))
                    finally:
                        ctx.set_option("sort_rows_mode", 0)
                        ctx.set_option("sort_rows_lanes", 0)
                    row = {"rows": r_eff, "row_len": n, "dtype": dtype, "desc": bool(desc), "idx": bool(idx), "inside": inside,
                           "mode0_took": took, "loop_rows_timed": lr, "loop_scaled": lr < r_eff, "reps": a.reps}
                    for name in ways:
                        m = statistics.median(t[name])
                        scale = r_eff / lr if name == "loop" else 1.0
                        row[name + "_ms"] = round(m * scale, 4)
                        row[name + "_ms_min_max"] = [round(min(t[name]) * scale, 4), round(max(t[name]) * scale, 4)]
                    best = min(row["mode1_ms"], row.get("mode2_ms", float("inf")))
                    row["rate_TBps"] = round(r_eff * n * (2 * es + (8 if idx else 0)) / best / 1e9, 3)
                    spread = row["mode0_ms_min_max"][1] - row["mode0_ms_min_max"][0]
                    row["mode0_ok"] = bool(row["mode0_ms"] <= best + spread)
                    line = json.dumps(row)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            del x, ov, oi, work
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    try:
        main()
    except MsdError as e:
        sys.exit(str(e))
