#!/usr/bin/env python3
"""Stream compaction and stable partition (msd_compact, MsdContext.compact) on large arrays, against torch.

    python tools/compact_sweep.py [--sizes i32:30 i32:28 i64:29] [--out profiles/compact_sweep.jsonl] [--step-timeout 900]

The driver (no --size) runs one child process per size, one at a time, each under its own time limit, and stops at the first
one that fails; a child (--size) measures every cell of one size and prints one JSON row per cell, which the driver appends to
--out.

Per size (key dtype : log2 n) the keys are uniform random (msd_gen_uniform_*), the value column is int64, and the cells are
every combination of
    share      about 1 %, 50 % and 99 % of the elements kept
    predicate  mask  a torch.bool mask that keeps the share
               range lo <= key <= hi with bounds that keep the share of the uniform keys
               both  mask AND range, each keeping the square root of the share
    outputs    keys, keys+idx (the int64 positions too), keys+vals (the 8-byte value column too), rest (keys and positions,
               the rejected elements behind the kept ones)
Every call is timed with HIP events around it: 3 warm-up calls, then the median of 10 timed calls with the min-max spread.
`bytes` = what the two passes read (the count: the keys with a range, the mask with a mask; the write: the keys, the mask,
the values) plus what is written (per stored element the key, 8 bytes of position, 8 bytes of value, as asked for; the count
word); `TBps` = bytes / median time, to be set against the copy ceiling of profiles/r02_stream_ceiling.jsonl.  `encode_ms` is
msd_run_encode without an inverse on the same keys, the cost one expects from the byte counts alone.

The opponents run once per share and predicate on the same tensors, their host synchronisation included (torch sizes the
result on the host): torch.masked_select(keys, mask), keys[mask] and torch.nonzero(mask) for the mask,
keys[(keys >= lo) & (keys <= hi)] for the range, keys[mask & (keys >= lo) & (keys <= hi)] for both.  The result of every
predicate is checked against torch once per share (keys, positions and count)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ["i32:30", "i32:28", "i64:29"]
SHARES = [0.01, 0.5, 0.99]
PREDICATES = ["mask", "range", "both"]
OUTPUTS = ["keys", "keys+idx", "keys+vals", "rest"]
WARMUP, REPS = 3, 10


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
    return round(statistics.median(t), 4), [round(min(t), 4), round(max(t), 4)]


def bounds(share, bits):
    """[lo, hi] that keeps `share` of uniform signed keys of that width, away from both ends of the type"""
    span = 1 << bits
    lo = -(span >> 1) + (span >> 8)
    return lo, lo + int(share * span) - 1


def size(spec):
    import torch
    from inplacemsdradixsort_amd import MsdContext
    dtype, logn = spec.split(":")
    es, n = (4 if dtype == "i32" else 8), 1 << int(logn)
    ctx = MsdContext(0)
    ctx.use_torch_stream()
    keys = torch.empty(n, dtype=torch.int32 if es == 4 else torch.int64, device="cuda")
    (ctx.gen_uniform_u32 if es == 4 else ctx.gen_uniform_u64)(keys)
    vals = torch.arange(n, dtype=torch.int64, device="cuda")
    encode_ms, _ = measure(lambda: ctx.run_encode(keys))
    for share in SHARES:
        for pred in PREDICATES:
            part = math.sqrt(share) if pred == "both" else share
            mask = (torch.rand(n, device="cuda") < part) if pred != "range" else None
            lo, hi = bounds(part, 8 * es) if pred != "mask" else (None, None)
            kw = dict(mask=mask, lo=lo, hi=hi)
            keep = torch.ones(n, dtype=torch.bool, device="cuda") if mask is None else mask.clone()
            if lo is not None:
                keep &= (keys >= lo) & (keys <= hi)
            ok, _, oi, count = ctx.compact(keys, indices=True, **kw)
            m = int(count.item())
            assert m == int(keep.sum().item()) and torch.equal(ok[:m], keys[keep]) and torch.equal(oi[:m], torch.nonzero(keep).flatten()), (spec, share, pred)
            del ok, oi, keep
            torch.cuda.empty_cache()
            if pred == "mask":
                opponents = {"torch_masked_select": lambda: torch.masked_select(keys, mask), "torch_index": lambda: keys[mask], "torch_nonzero": lambda: torch.nonzero(mask)}
            elif pred == "range":
                opponents = {"torch_index": lambda: keys[(keys >= lo) & (keys <= hi)]}
            else:
                opponents = {"torch_index": lambda: keys[mask & (keys >= lo) & (keys <= hi)]}
            their = {}
            for name, fn in opponents.items():
                med, spread = measure(lambda: (fn(), torch.cuda.synchronize()))
                their[name + "_ms"], their[name + "_ms_min_max"] = med, spread
                torch.cuda.empty_cache()
            reads = (es * n if lo is not None else 0) + (n if mask is not None else 0) + es * n + (n if mask is not None else 0)
            for outputs in OUTPUTS:
                rest, idx, with_vals = outputs == "rest", outputs in ("keys+idx", "rest"), outputs == "keys+vals"
                out = torch.empty(n, dtype=keys.dtype, device="cuda")
                out_i = torch.empty(n, dtype=torch.int64, device="cuda") if idx else None
                out_v = torch.empty(n, dtype=torch.int64, device="cuda") if with_vals else None
                fn = lambda: ctx.compact(keys, rest=rest, values=vals if with_vals else None, out=out, out_indices=out_i, out_values=out_v, **kw)
                med, spread = measure(fn)
                stored = n if rest else m
                nbytes = reads + (8 * n if with_vals else 0) + stored * (es + (8 if idx else 0) + (8 if with_vals else 0)) + 8
                row = {"dtype": dtype, "log2_n": int(logn), "n": n, "share": share, "kept": m, "predicate": pred, "outputs": outputs, "warmup": WARMUP, "reps": REPS,
                       "ms": med, "ms_min_max": spread, "bytes": nbytes, "TBps": round(nbytes / med / 1e9, 3), "encode_ms": encode_ms}
                row.update(their)
                print("ROW " + json.dumps(row), flush=True)
                del out, out_i, out_v
                torch.cuda.empty_cache()
            del mask
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=SIZES)
    ap.add_argument("--size", default=None, help="measure every cell of this one size in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_sweep.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one size may take")
    a = ap.parse_args()
    if a.size:
        size(a.size)
        return 0
    want = len(SHARES) * len(PREDICATES) * len(OUTPUTS)
    with open(a.out, "w") as out:
        for spec in a.sizes:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", spec], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                   timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print("size %s ran into its time limit of %d s: stopping" % (spec, a.step_timeout), flush=True)
                return 1
            rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
            for r in rows:
                out.write(r + "\n")
            out.flush()
            if p.returncode != 0 or len(rows) != want:
                print(p.stdout[-4000:])
                print("size %s failed with status %d after %d of %d cells: stopping" % (spec, p.returncode, len(rows), want), flush=True)
                return 1
            print("size %s: %d cells" % (spec, len(rows)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
