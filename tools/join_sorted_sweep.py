#!/usr/bin/env python3
"""Sort-merge join of two sorted arrays (msd_join_groups, msd_join_pairs) on large inputs, against the routes a caller had before.

    python tools/join_sorted_sweep.py [--cells u32:28:20:uniform u32:28:n:half ... u64:28:n:d10]
                                      [--out profiles/join_sorted_sweep.jsonl] [--append] [--step-timeout 300]

The driver (no --cell) runs one child process per cell, one at a time, each under its own time limit, and stops at the first
cell that fails; a child (--cell) measures one cell and prints one JSON row, which the driver appends to --out.

A cell is key width : log2 n : log2 m (or `n` for m = n) : keys, generated as in tools/set_sorted_sweep.py: `uniform` and
`d10` (2^10 distinct values) on the device, shifted right by one bit -- non-negative as int32 / int64, so that torch's order
and the library's agree -- and sorted with the library's own sort; `half` (half_shared): A is uniform, and half of B's
elements are taken from A at equal strides, the other half uniform from another seed.  At most PAIR_CAP = 2^30 pairs are
stored by any way of a cell (`d10` has up to 2^46).

The ways of one cell are timed INTERLEAVED on the same tensors, as in tools/set_sorted_sweep.py: every way is warmed up (2
calls; a way whose first call takes more than 0.3 s: that call alone), then ROUNDS rounds run every way once, each call
between two HIP events; a row holds the median and the min-max spread per way and what it was made with.  The ways:
    groups                msd_join_groups into preallocated arrays (all five outputs)
    set_intersection      MsdContext.set_sorted(a, b, "intersection") with the origin: the call that `groups` does strictly
                          more than; `groups_over_set` is the ratio of the medians
    pairs_count           msd_join_pairs with cap = 0: the products and their scan
    pairs                 msd_join_pairs of the first min(total, PAIR_CAP) pairs; `pairs_TBps` = 16 bytes per stored pair /
                          median, to be set against the copy ceiling of profiles/r02_stream_ceiling.jsonl
    join                  groups, then pairs: the two calls one behind the other (the total is known: no host read)
    former                the library's route before: two searchsorted(b, a, needles_sorted=True), the counts clipped to
                          PAIR_CAP pairs, torch.cumsum, one host read of the total, torch.repeat_interleave, arange, subtraction
    torch                 the same with torch.searchsorted
`loses_to_former` says whether `join` is slower than `former`.  A way that raises (out of memory) is listed in
`not_measured` with its message.  Once per cell the pairs of the join are compared exactly with those of the former route (both
are in lexicographic order).  The tool reads nothing but what it generates."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = [w + ":28:" + m + ":" + d for w in ("u32", "u64") for d in ("uniform", "d10", "half") for m in ("20", "n")]
PAIR_CAP = 1 << 30
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
    row = {"width": width, "log2_n": int(logn), "n": n, "m": m, "log2_m": int(logn) if logm == "n" else int(logm), "keys": keys, "pair_cap": PAIR_CAP,
           "not_measured": {}}
    gcap = min(n, m)
    i64 = lambda count: torch.empty(count, dtype=torch.int64, device="cuda")
    gkeys, gnum, pnum = torch.empty(gcap, dtype=dt, device="cuda"), i64(1), i64(1)
    four = [i64(gcap) for _ in range(4)]
    sout, sorigin = torch.empty(gcap, dtype=dt, device="cuda"), i64(gcap)
    kt = ctx._key_type(a)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

    def groups():
        ctx._ok(ctx._L.msd_join_groups(ctx._h, p(a), n, p(b), m, kt, gcap, p(gkeys), *[p(t) for t in four], p(gnum)))

    def pairs(cap, oa, ob):
        ctx._ok(ctx._L.msd_join_pairs(ctx._h, gcap, p(gnum), *[p(t) for t in four], n, m, None, None, cap, p(oa), p(ob), p(pnum)))

    groups()
    pairs(0, None, None)
    G, total = int(gnum.item()), int(pnum.item())
    stored = min(total, PAIR_CAP)
    row["groups"], row["pairs"], row["pairs_stored"] = G, total, stored
    oa, ob = i64(stored), i64(stored)

    def former(search):
        left, right = search(False), search(True)
        ends = torch.cumsum(right - left, 0)
        del right
        cnt = ends.clamp(max=PAIR_CAP)
        cnt[1:] -= ends[:-1].clamp(max=PAIR_CAP)                    # the counts, clipped to the first PAIR_CAP pairs
        tot = min(int(ends[-1].item()), PAIR_CAP)                   # (the host read)
        starts = ends.clamp_(max=PAIR_CAP).sub_(cnt)
        ia = torch.repeat_interleave(torch.arange(n, device="cuda"), cnt, output_size=tot)
        del cnt
        ib = torch.arange(tot, device="cuda").sub_(starts[ia]).add_(left[ia])
        return ia, ib

    lib_search = lambda right: ctx.searchsorted(b, a, right=right, needles_sorted=True)
    torch_search = lambda right: torch.searchsorted(b, a, right=right)

    # the pairs once, exactly, against the former route; the groups against the intersection
    pairs(stored, oa, ob)
    fa, fb = former(lib_search)
    assert fa.numel() == stored and torch.equal(fa, oa) and torch.equal(fb, ob), (spec, "the pairs differ from the former route's")
    del fa, fb
    snum, _, _ = ctx.set_sorted(a, b, "intersection", cap=gcap, out=sout, out_origin=sorigin)
    assert int(snum.item()) == G and torch.equal(sout[:G], gkeys[:G]) and torch.equal(sorigin[:G], four[0][:G]), (spec, "the groups differ from the intersection")
    torch.cuda.empty_cache()

    def join():
        groups()
        pairs(stored, oa, ob)

    total_elems = n + m
    ways = [("groups", groups, 2 * total_elems * kb + G * (kb + 32)),
            ("set_intersection", lambda: ctx.set_sorted(a, b, "intersection", cap=gcap, out=sout, out_origin=sorigin), 2 * total_elems * kb + G * (kb + 8)),
            ("pairs_count", lambda: pairs(0, None, None), None), ("pairs", lambda: pairs(stored, oa, ob), 16 * stored), ("join", join, None),
            ("former", lambda: former(lib_search), None), ("torch", lambda: former(torch_search), None)]

    live, times, made = [], {}, {}
    for name, fn, nbytes in ways:                                   # warm-up, every way
        try:
            first = timed(fn)
            slow = first > SLOW_MS
            for _ in range(0 if slow else WARMUP - 1):
                fn()
            torch.cuda.synchronize()
        except Exception as e:                                      # (out of memory)
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
    med = {}
    for name, _, nbytes in live:
        t = times[name]
        med[name] = statistics.median(t)
        row[name + "_ms"] = round(med[name], 4)
        row[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        row[name + "_warmup"], row[name + "_reps"] = made[name][0], len(t)
        if nbytes:
            row[name + "_bytes"] = nbytes
            row[name + "_TBps"] = round(nbytes / med[name] / 1e9, 3)
    if "groups" in med and "set_intersection" in med:
        row["groups_over_set"] = round(med["groups"] / med["set_intersection"], 3)
    for other in ("former", "torch"):
        if "join" in med and other in med:
            row[other + "_over_join"] = round(med[other] / med["join"], 3)
            row["loses_to_" + other] = med["join"] > med[other]
    ctx.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=CELLS)
    ap.add_argument("--cell", default=None, help="measure this one cell in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_sorted_sweep.jsonl"))
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of starting it anew")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one cell may take")
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
