#!/usr/bin/env python3
"""Cache policy of the two big stream kernels, measured: classify_direct2_kernel (MSD_D2_NT) and count_place16_kernel
(MSD_C16_NT), bit 0 = nontemporal loads, bit 1 = nontemporal stores (csrc/msd_direct.hpp, csrc/msd_count16.hpp).

    python tools/nt_variants.py --build                       # the seven libraries (needs no GPU)
    python tools/nt_variants.py [--logn 30] [--rounds 4] [--kinds u32,u64,pairs] > profiles/nt_variants.jsonl

All builds are loaded into ONE process and run alternating: in every round each build sorts the same seeded input once
with phase timing off (the whole sort, events around the call) and once with the library's phase timing on (the launch
times of "A classify direct" -- both direct rounds together -- and of "count sort", the counting leaf).  The plain build
runs at both ends of every round; the range of its runs is the spread a variant has to beat.  The first round is a
warm-up and is dropped.  Every output is verified with ctx.check against the input's count and checksum.  One JSON line
per (kind, build), then one summary line per kind.  (The policy applies to arrays of at least kStreamMinBytes, csrc/
msd_device.hpp: keep --logn at 26 or above for u32 keys.)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from inplacemsdradixsort_amd import _build, _lib  # noqa: E402

VARIANTS = [("plain0", ["-DMSD_D2_NT=0", "-DMSD_C16_NT=0"])] + \
    [(f"d2nt{p}", [f"-DMSD_D2_NT={p}", "-DMSD_C16_NT=0"]) for p in (1, 2, 3)] + \
    [(f"c16nt{p}", ["-DMSD_D2_NT=0", f"-DMSD_C16_NT={p}"]) for p in (1, 2, 3)]
PHASES = ("A classify direct", "count sort")


def lib_path(name):
    return os.path.join(_build.HERE, f"libinpmsdradix_hip_{name}.so")


def build_all():
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:  # (hipcc runs in child processes)
        for out in ex.map(lambda v: _build.build_variant(v[0], v[1]), VARIANTS):
            print(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--logn", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--kinds", default="u32,u64,pairs")
    a = ap.parse_args()
    if a.build:
        return build_all()
    import torch
    from inplacemsdradixsort_amd import MsdContext
    _build.stale = lambda: False
    ctxs = {}
    for name, _ in VARIANTS:  # one context per library
        assert os.path.exists(lib_path(name)), f"{lib_path(name)}: run with --build first"
        _build.LIB, _lib._lib = lib_path(name), None
        ctxs[name] = MsdContext(0)
        ctxs[name].use_torch_stream()
    n = 1 << a.logn
    for kind in a.kinds.split(","):
        t = torch.empty(n, dtype=torch.int32 if kind == "u32" else torch.int64, device="cuda")
        r = torch.empty(n, dtype=torch.int64, device="cuda") if kind == "pairs" else None
        names = [v for v, _ in VARIANTS if kind == "u32" or not v.startswith("c16")]  # (the counting leaf takes u32 keys only)
        order = names + ["plain0"]
        res = {v: {"sort_ms": [], **{p: [] for p in PHASES}} for v in names}
        spread = {"sort_ms": [], **{p: [] for p in PHASES}}
        for rnd in range(a.rounds):
            seen = {}
            for v in order:
                ctx = ctxs[v]
                row = {}
                for profiling in (False, True):
                    if kind == "u32":
                        ctx.gen_uniform_u32(t, seed=0x5EED0001 + rnd)
                    else:
                        ctx.gen_uniform_u64(t, seed=0x5EED0005 + rnd)
                    if r is not None:
                        ctx.gen_iota_u64(r)
                    c0 = ctx.check(t)
                    ctx.set_profiling(profiling)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if kind == "u32":
                        ctx.sort_u32(t)
                    elif kind == "u64":
                        ctx.sort_u64(t)
                    else:
                        ctx.sort_pairs_u64(t, r)
                    e1.record()
                    torch.cuda.synchronize()
                    c1 = ctx.check(t)
                    assert c1[0] == 0 and c1[1:] == c0[1:], (kind, v, c0, c1)
                    if profiling:
                        ph = dict(ctx.phases())
                        for p in PHASES:
                            row[p] = round(ph.get(p, 0.0), 1)
                    else:
                        row["sort_ms"] = round(e0.elapsed_time(e1), 4)
                ctx.set_profiling(False)
                if rnd == 0:
                    continue  # warm-up round: first launches, workspace allocation
                for k, x in row.items():
                    res[v][k].append(x)
                if v == "plain0" and "plain0" in seen:
                    for k, x in row.items():
                        spread[k].append(round(abs(x - seen["plain0"][k]), 4))
                seen[v] = row
        for v in names:
            print(json.dumps({"kind": kind, "logn": a.logn, "build": v, "flags": dict(VARIANTS)[v], "verified": True,
                              "sort_ms": res[v]["sort_ms"], **{p + " us": res[v][p] for p in PHASES}}))
        med = {v: {k: statistics.median(x) for k, x in res[v].items()} for v in names}
        rng = {k: round(max(res["plain0"][k]) - min(res["plain0"][k]), 4) for k in spread}
        print(json.dumps({"kind": kind, "summary": "median minus plain0's median (negative: faster); plain0_range: max - min over all plain runs",
                          "plain0_median": med["plain0"], "plain0_range": rng, "plain0_same_round_differences": spread,
                          "delta": {v: {k: round(med[v][k] - med["plain0"][k], 4) for k in med[v]} for v in names if v != "plain0"}}), flush=True)
        del t, r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
