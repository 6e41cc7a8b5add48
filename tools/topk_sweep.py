#!/usr/bin/env python3
"""Top-k against the only way to get it without msd_topk_*: clone() + msd_sort_* of the clone (+ a slice).

    python tools/topk_sweep.py [--logn 26 28 30] [--kinds u32 zipf u64 pairs pairs_hi0] [--out profiles/topk_sweep.jsonl]

Per (n, kind, k): HIP events around the call, one warm-up, the median of --reps runs, both ways in the same process, alternating.
Neither way changes its input (top-k reads it, the sort works on the clone made inside the clock), so the inputs are generated
once per (n, kind), outside the clock.  Every top-k result is compared with the slice of the sorted clone.  One JSON line per
case: both times, the ratio, the search's counters, the per-phase times of one extra profiled run, and `read_bytes_per_key`
= (select_hist_passes + 1) reads of the key array; what the filter writes and the finishing sort moves depends on k, not on n,
and is not in that figure.  MSD_VARIANT=<name> loads an experimental build."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
if os.environ.get("MSD_VARIANT"):  # an experimental build (inplacemsdradixsort_amd._build.build_variant)
    from inplacemsdradixsort_amd import _build
    _build.LIB = os.path.join(_build.HERE, f"libinpmsdradix_hip_{os.environ['MSD_VARIANT']}.so")
    _build.stale = lambda: False
from inplacemsdradixsort_amd import MsdContext  # noqa: E402

KINDS = {
    "u32": "uniform u32 keys", "zipf": "Zipf(theta=1) u32 keys", "u64": "uniform u64 keys",
    "pairs": "(u64 key, u64 rid) tuples, full-width keys", "pairs_hi0": "(u64 key, u64 rid) tuples, upper 32 key bits zero",
}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="+", default=[26, 28, 30])
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--logk", type=int, nargs="+", default=[0, 10, 16, 20, 24, -2], help="log2 k; -2 = n / 4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--select-cap", type=int, default=None)
    ap.add_argument("--largest", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    if a.select_cap:
        ctx.set_option("select_cap", a.select_cap)
    out = open(a.out, "w") if a.out else None
    for logn in a.logn:
        n = 1 << logn
        for kind in a.kinds:
            wide = kind not in ("u32", "zipf")
            keys = torch.empty(n, dtype=torch.int64 if wide else torch.int32, device="cuda")
            rids = None
            if kind == "u32":
                ctx.gen_uniform_u32(keys, seed=0x5EED0021)
            elif kind == "zipf":
                ctx.gen_zipf_u32(keys, seed=0x5EED0023)
            else:
                ctx.gen_uniform_u64(keys, seed=0x5EED0025, shift_right=32 if kind == "pairs_hi0" else 0)
            if kind.startswith("pairs"):
                rids = torch.empty(n, dtype=torch.int64, device="cuda")
                ctx.gen_iota_u64(rids)
            ctx.reserve(n, 8 if wide else 4, 8 if rids is not None else 0)
            torch.cuda.synchronize()
            before = ctx.check(keys)
            res = {}

            def clone_sort():
                c = keys.clone()
                if rids is not None:
                    r = rids.clone()
                    ctx.sort_pairs_u64(c, r)
                elif wide:
                    ctx.sort_u64(c)
                else:
                    ctx.sort_u32(c)
                res["sorted"] = c

            for lk in a.logk:
                k = n // 4 if lk == -2 else 1 << lk
                if k > n:
                    continue
                ok = torch.empty(k, dtype=keys.dtype, device="cuda")
                orr = torch.empty(k, dtype=torch.int64, device="cuda") if rids is not None else None

                def topk():
                    ctx.topk(keys, k, largest=a.largest, rids=rids, out=ok, out_rids=orr)

                ctx.set_profiling(True)   # one run with per-phase events (not one of the timed runs)
                topk()
                phases = {name: round(us, 1) for name, us in ctx.phases()}
                ctx.set_profiling(False)
                topk()
                stats = ctx.stats()
                clone_sort()
                want = res["sorted"][n - k:] if a.largest else res["sorted"][:k]
                assert torch.equal(ok, want), (kind, logn, k)
                t_top, t_ref = [], []
                for _ in range(a.reps):  # alternating, same process
                    t_top.append(timed(topk))
                    t_ref.append(timed(clone_sort))
                res.clear()
                m_top, m_ref = statistics.median(t_top), statistics.median(t_ref)
                kb = 8 if wide else 4
                row = {"logn": logn, "kind": kind, "k": k, "largest": a.largest, "topk_ms": round(m_top, 4), "clone_sort_ms": round(m_ref, 4),
                       "clone_sort_over_topk": round(m_ref / m_top, 2), "topk_ms_min_max": [round(min(t_top), 4), round(max(t_top), 4)],
                       "clone_sort_ms_min_max": [round(min(t_ref), 4), round(max(t_ref), 4)],
                       "select_hist_passes": stats["select_hist_passes"], "select_skipped_bits": stats["select_skipped_bits"],
                       "select_candidates": stats["select_candidates"], "select_below": stats["select_below"],
                       "read_bytes_per_key": (stats["select_hist_passes"] + 1) * kb,
                       "phases_us": phases, "topk_read_TBps": round((stats["select_hist_passes"] + 1) * kb * n / m_top / 1e9, 3)}
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            assert ctx.check(keys)[1:] == before[1:], "the input was modified"
            del keys, rids
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
