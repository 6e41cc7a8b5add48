#!/usr/bin/env python3
"""Merge of two sorted arrays (msd_merge_sorted) on large inputs, against sorting the concatenation again.

    python tools/merge_sorted_sweep.py [--cells u32:30:20:uniform u32:30:24:uniform ... u64:29:n:d10]
                                       [--out profiles/merge_sorted_sweep.jsonl] [--append] [--step-timeout 600]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

A cell is key width : log2 n : log2 m (or `n` for m = n) : keys (`uniform`, or `d10` for 2^10 distinct values).  The keys are
generated on the device (msd_gen_uniform_*), shifted right by one bit -- non-negative as int32 / int64, so that torch's order
and the library's agree -- and each side is sorted with the library's own sort.  Every way is timed with HIP events around the
call: 3 warm-up calls, then the median of 10 timed calls with the min-max spread.  A torch way whose first call takes more
than 0.3 s gets that call as its only warm-up and 3 timed calls; every row says what each way was made with (`*_warmup`,
`*_reps`).  The ways, all into outputs allocated once:
    merge_plain      MsdContext.merge_sorted(a, b, out=...)
    merge_values     ... with int64 values (the element's index in the concatenation) on both sides
    merge_origin     ... with the origin output
    sort_typed_cat   torch.cat([a, b]) and MsdContext.sort_typed on it: what a caller does without the merge
    torch_sort_cat   torch.sort(torch.cat([a, b]))
`*_bytes` = 2 (n + m) keys, plus 16 bytes per element with values, plus 8 with origin; `*_TBps` = bytes / median time, to be
set against the copy ceiling of profiles/r02_stream_ceiling.jsonl.  Once per cell every result of the library is checked
exactly: against torch.sort(cat, stable=True) -- the stable argsort of the concatenation; torch.sort refuses more than 2^31 - 1
elements, so the cell with n + m = 2^31 has neither this comparison nor the torch opponent (`torch_sort_cat_skipped`) -- and,
in every cell, by the four properties that define it: origin is a permutation, merged is cat[origin], merged ascends, and origin ascends wherever two neighbours of
merged are equal; the values must equal the origin.  Every timed series of a merge starts from zeroed outputs and what its
last call left is compared with that expectation again.  The tool reads nothing but what it generates."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = ["20", "24", "28", "n"]
CELLS = [w + ":" + m + ":" + d for w in ("u32:30", "u64:29") for d in ("uniform", "d10") for m in MS]
WARMUP, REPS = 3, 10
SLOW_MS, SLOW_REPS = 300.0, 3
TORCH_SORT_MAX = (1 << 31) - 1      # "The dimension being sorted can not have more than INT_MAX elements"


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
        ctx.sort_typed(t)
        return t

    a, b = generate(n, 0x5EED0001), generate(m, 0x5EED0777)
    total = n + m
    row = {"width": width, "log2_n": int(logn), "n": n, "m": m, "log2_m": int(logn) if logm == "n" else int(logm), "keys": keys}
    out = torch.empty(total, dtype=dt, device="cuda")

    # the results once, exactly
    va, vb = torch.arange(n, dtype=torch.int64, device="cuda"), torch.arange(n, total, dtype=torch.int64, device="cuda")
    ov, oo = torch.empty(total, dtype=torch.int64, device="cuda"), torch.empty(total, dtype=torch.int64, device="cuda")
    ctx.merge_sorted(a, b, values_a=va, values_b=vb, out=out, out_values=ov, out_origin=oo)
    plain = ctx.merge_sorted(a, b)
    assert torch.equal(plain, out), (spec, "plain and with values and origin differ")
    del plain
    assert torch.equal(ov, oo), (spec, "the values are not those of the origin")
    seen = torch.zeros(total, dtype=torch.bool, device="cuda")
    seen[oo] = True
    assert bool(seen.all()), (spec, "origin is no permutation")
    del seen
    cat = torch.cat([a, b])
    assert torch.equal(cat[oo], out), (spec, "merged is not cat[origin]")
    assert bool((out[1:] >= out[:-1]).all()), (spec, "merged does not ascend")
    assert bool(((out[1:] != out[:-1]) | (oo[1:] > oo[:-1])).all()), (spec, "not stable")
    torch_sorts = total <= TORCH_SORT_MAX
    if torch_sorts:
        want, want_origin = torch.sort(cat, stable=True)
        assert torch.equal(out, want) and torch.equal(oo, want_origin), (spec, "differs from torch.sort(cat, stable=True)")
    else:                                                           # the properties above define the same result
        want, want_origin = out.clone(), oo.clone()
        row["torch_sort_cat_skipped"] = "torch.sort takes at most 2^31 - 1 elements"
    del cat
    torch.cuda.empty_cache()

    def sort_typed_cat():
        c = torch.cat([a, b])
        ctx.sort_typed(c)
        return c

    ways = [
        ("merge_plain", lambda: ctx.merge_sorted(a, b, out=out), 2 * kb),
        ("merge_values", lambda: ctx.merge_sorted(a, b, values_a=va, values_b=vb, out=out, out_values=ov), 2 * kb + 16),
        ("merge_origin", lambda: ctx.merge_sorted(a, b, out=out, out_origin=oo), 2 * kb + 8),
        ("sort_typed_cat", sort_typed_cat, None),
        ("torch_sort_cat", lambda: torch.sort(torch.cat([a, b])), None),
    ]
    for name, fn, per_elem in ways:
        if name.startswith("torch") and not torch_sorts:
            continue
        if per_elem:                                                # a merge: the timed calls write into zeroed outputs ...
            out.zero_(), ov.zero_(), oo.zero_()
        med, spread, warmup, reps = measure(fn, adaptive=name.startswith("torch"))
        if per_elem:                                                # ... and what the last of them left is the expectation again
            assert torch.equal(out, want), (spec, name, "keys after the timed calls")
            got = ov if name == "merge_values" else oo if name == "merge_origin" else None
            assert got is None or torch.equal(got, want_origin), (spec, name, "values / origin after the timed calls")
        row[name + "_ms"] = round(med, 4)
        row[name + "_ms_min_max"] = [round(v, 4) for v in spread]
        row[name + "_warmup"], row[name + "_reps"] = warmup, reps
        if per_elem:
            row[name + "_bytes"] = total * per_elem
            row[name + "_TBps"] = round(row[name + "_bytes"] / med / 1e9, 3)
        torch.cuda.empty_cache()
    ctx.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=CELLS)
    ap.add_argument("--cell", default=None, help="measure this one cell in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_sorted_sweep.jsonl"))
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
