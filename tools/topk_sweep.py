#!/usr/bin/env python3
"""Top-k against the only way to get it without msd_topk_*: clone() + msd_sort_* of the clone (+ a slice).

    python tools/topk_sweep.py [--logn 26 28 30] [--kinds u32 zipf u64 pairs pairs_hi0] [--out profiles/topk_sweep.jsonl]

Per (n, kind, k): HIP events around the call, one warm-up, the median of --reps runs, both ways in the same process, alternating.
Neither way changes its input (top-k reads it, the sort works on the clone made inside the clock), so the inputs are generated
once per (n, kind), outside the clock.  Every top-k result is compared with the slice of the sorted clone.  One JSON line per
case: both times, the ratio, the search's counters, the per-phase times of one extra profiled run, and `read_bytes_per_key`
= (select_hist_passes + 1) reads of the key array; what the filter writes and the finishing sort moves depends on k, not on n,
and is not in that figure.  MSD_VARIANT=<name> loads an experimental build.

    python tools/topk_sweep.py --typed [--logn 28 30] [--kinds f32_bits ...] [--out profiles/topk_typed_sweep.jsonl]

Typed keys and indices (msd_topk_keys), each kind against the call it is to be judged by, same method:
    f32_bits, i32_bits   uniform random bit patterns as float32 / int32, no indices   vs  msd_topk_u32 on the same array
    f32_bits_idx         the same with indices                                        vs  float32 without indices
    f64_bits_idx         uniform 64-bit patterns as float64 with indices              vs  msd_topk_pairs_u64 fed an arange rid array
    f32_normal[_idx]     N(0,1) float32 scores, without / with indices                vs  torch.topk (k <= 2^20; orientation only)
Every typed result is checked: against the unsigned top-k of the keys' codes (computed with torch integer operations), or
torch.sort for the scores; indices must point at keys bit-equal to the values, no position twice."""
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


TYPED_KINDS = ["f32_bits", "i32_bits", "f32_bits_idx", "f64_bits_idx", "f32_normal", "f32_normal_idx"]


def codes_of(t):
    """the order-preserving unsigned codes of a float / int tensor's bit patterns, as an int tensor of the same width
    (include/msd_radix_hip.h: float: positive -> sign bit set, negative -> all bits inverted; signed: sign bit flipped)"""
    it = torch.int32 if t.element_size() == 4 else torch.int64
    b = t.view(it)
    top = torch.iinfo(it).min
    return torch.where(b < 0, ~b, b ^ top) if t.is_floating_point() else b ^ top


def typed_main(a, ctx, out):
    for logn in a.logn:
        n = 1 << logn
        for kind in a.kinds:
            base, idx = kind.replace("_idx", ""), kind.endswith("_idx")
            wide = base.startswith("f64")
            raw = torch.empty(n, dtype=torch.int64 if wide else torch.int32, device="cuda")
            if base == "f32_normal":
                g = torch.Generator(device="cuda")
                g.manual_seed(0x5EED0031)
                keys = torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
                raw = keys.view(torch.int32)
            elif wide:
                ctx.gen_uniform_u64(raw, seed=0x5EED0025)
                keys = raw.view(torch.float64)
            else:
                ctx.gen_uniform_u32(raw, seed=0x5EED0021)
                keys = raw.view(torch.float32) if base == "f32_bits" else raw
            rids = None
            if kind == "f64_bits_idx":  # what the reference call needs and the typed one does not
                rids = torch.empty(n, dtype=torch.int64, device="cuda")
                ctx.gen_iota_u64(rids)
            ctx.reserve(n, 8, 8 if wide else 0)  # (32-bit keys with indices are sorted as 64-bit elements)
            torch.cuda.synchronize()
            before = ctx.check(raw)
            codes = None if base == "f32_normal" else codes_of(keys)
            ref_name = {"f32_bits": "msd_topk_u32", "i32_bits": "msd_topk_u32", "f32_bits_idx": "msd_topk_keys F32 without indices",
                        "f64_bits_idx": "msd_topk_pairs_u64 + arange rids", "f32_normal": "torch.topk", "f32_normal_idx": "torch.topk"}[kind]
            for lk in a.logk:
                k = n // 4 if lk == -2 else 1 << lk
                if k > n:
                    continue
                ov = torch.empty(k, dtype=keys.dtype, device="cuda")
                oi = torch.empty(k, dtype=torch.int64, device="cuda") if idx else None
                rv = torch.empty(k, dtype=raw.dtype, device="cuda")
                rr = torch.empty(k, dtype=torch.int64, device="cuda") if rids is not None else None
                rf = torch.empty(k, dtype=keys.dtype, device="cuda")

                def topk():
                    ctx.topk_typed(keys, k, largest=a.largest, out=ov, out_indices=oi)

                ref = None
                if kind in ("f32_bits", "i32_bits"):
                    ref = lambda: ctx.topk(raw, k, largest=a.largest, out=rv)  # noqa: E731
                elif kind == "f32_bits_idx":
                    ref = lambda: ctx.topk_typed(keys, k, largest=a.largest, out=rf)  # noqa: E731
                elif kind == "f64_bits_idx":
                    ref = lambda: ctx.topk(raw, k, largest=a.largest, rids=rids, out=rv, out_rids=rr)  # noqa: E731
                elif k <= 1 << 20:   # torch.topk always returns the largest / smallest first and its indices
                    ref = lambda: torch.topk(keys, k, largest=a.largest, sorted=True)  # noqa: E731

                ctx.set_profiling(True)   # one run with per-phase events (not one of the timed runs)
                topk()
                phases = {name: round(us, 1) for name, us in ctx.phases()}
                ctx.set_profiling(False)
                topk()
                stats = ctx.stats()
                # ---- the result
                if codes is not None:
                    want = ctx.topk(codes, k, largest=a.largest)
                    assert torch.equal(codes_of(ov), want), (kind, logn, k)
                    del want
                else:
                    s = torch.sort(keys).values
                    assert torch.equal(ov, s[n - k:] if a.largest else s[:k]), (kind, logn, k)
                    del s
                if idx:
                    assert int(oi.min()) >= 0 and int(oi.max()) < n and torch.equal(raw[oi], ov.view(raw.dtype)), (kind, logn, k)
                    assert oi.unique().numel() == k, (kind, logn, k)
                torch.cuda.empty_cache()
                t_top, t_ref = [], []
                if ref is not None:
                    ref()
                for _ in range(a.reps):  # alternating, same process
                    t_top.append(timed(topk))
                    if ref is not None:
                        t_ref.append(timed(ref))
                m_top = statistics.median(t_top)
                kb = 8 if wide else 4
                row = {"logn": logn, "kind": kind, "k": k, "largest": a.largest, "topk_ms": round(m_top, 4),
                       "topk_ms_min_max": [round(min(t_top), 4), round(max(t_top), 4)], "ref": ref_name if ref is not None else None,
                       "select_hist_passes": stats["select_hist_passes"], "select_skipped_bits": stats["select_skipped_bits"],
                       "select_candidates": stats["select_candidates"], "select_below": stats["select_below"],
                       "read_bytes_per_key": (stats["select_hist_passes"] + 1) * kb, "phases_us": phases,
                       "topk_read_TBps": round((stats["select_hist_passes"] + 1) * kb * n / m_top / 1e9, 3),
                       "rid_array_bytes": 0, "ref_rid_array_bytes": 8 * n if rids is not None else 0,
                       "workspace_bytes": ctx.workspace_bytes}
                if ref is not None:
                    m_ref = statistics.median(t_ref)
                    row.update({"ref_ms": round(m_ref, 4), "ref_ms_min_max": [round(min(t_ref), 4), round(max(t_ref), 4)],
                                "topk_over_ref": round(m_top / m_ref, 3), "within_ref_spread": bool(min(t_ref) <= m_top <= max(t_ref))})
                if os.environ.get("MSD_VARIANT"):
                    row["variant"] = os.environ["MSD_VARIANT"]
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            assert ctx.check(raw)[1:] == before[1:], "the input was modified"
            del keys, raw, rids, codes
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="+", default=[26, 28, 30])
    ap.add_argument("--typed", action="store_true", help="typed keys and indices (msd_topk_keys): the kinds of TYPED_KINDS")
    ap.add_argument("--kinds", nargs="+", default=None, choices=list(KINDS) + TYPED_KINDS)
    ap.add_argument("--logk", type=int, nargs="+", default=[0, 10, 16, 20, 24, -2], help="log2 k; -2 = n / 4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--select-cap", type=int, default=None)
    ap.add_argument("--largest", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    if a.select_cap:
        ctx.set_option("select_cap", a.select_cap)
    out = open(a.out, "a" if a.append else "w") if a.out else None
    if a.typed:
        a.kinds = a.kinds or TYPED_KINDS
        typed_main(a, ctx, out)
        ctx.close()
        return
    a.kinds = a.kinds or list(KINDS)
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
