#!/usr/bin/env python3
"""Per-sort table of what runs between the big kernels, from a rocprofv3 kernel trace of bench.py.

    python tools/fixup_gaps.py <..._kernel_trace.csv> [--skip W] > profiles/fixup_gaps_<tag>.txt

A sort is the run of kernels from one bit-skip sample (vary_kernel) or one front pass (front_probe_kernel, where the sort
tries that path: csrc/msd_front16.hpp; a declined one goes on with the bit-skip sample) to the last kernel before the next one, or before the first kernel that is not the
library's sort (input generation, checks).  The first W sorts (bench.py's warm-up)
are dropped; the rest are averaged position by position, so they must all launch the same kernels -- they do for the
seeded inputs of one config.  Printed: the big four, every other kernel with its duration, every interval of at least
--gap microseconds in which no kernel runs with the kernels on either side and the host call it sits behind, and the
totals.  Needs no GPU."""
import argparse
import csv
import re

BIG = ("classify_direct2_kernel", "count_place16_kernel", "direct_hist_kernel", "front_count16_kernel")
# the host synchronisation behind which the GPU waits, by the kernel that ran last before it
# (a round ends with collect_kernel, or with cleanup_kernel where collect_kernel runs behind the child scan)
HOST_CALL = {"vary_kernel": "run_vary (skip_leading_bits)", "front_top_kernel": "the front pass's readback (front_count)", "cleanup_kernel": "round_summary",
             "collect_kernel": "round_summary, or (collect_kernel behind the child scan) the early copy of the counters",
             "count_walk_kernel": "read_counters (count_leaves)"}
STARTS = ("vary_kernel", "front_probe_kernel")
OUTSIDE = ("gen_", "check_", "at::", "elementwise")
FILLS = "__amd_rocclr"  # the runtime's own fills and copies (hipMemsetAsync, hipMemcpyAsync of a few words): left out, their time counts as idle


def short(name):
    name = re.sub(r"^void\s+", "", name)
    name = re.sub(r"\(anonymous namespace\)::|\bmsd::", "", name)
    m = re.match(r"([A-Za-z_0-9]+)(<[^(]*>)?", name)
    if not m:
        return name[:60]
    args = m.group(2) or ""
    args = args.replace("unsigned int", "u32").replace("unsigned long", "u64")
    return m.group(1) + args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=2, help="sorts to drop at the start (warm-up)")
    ap.add_argument("--gap", type=float, default=4.0, help="list idle intervals of at least this many microseconds")
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.trace)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    sorts, cur = [], None
    for s, e, nm in rows:
        if nm.startswith(FILLS):
            continue
        inside = not nm.startswith(OUTSIDE)
        declined = bool(cur) and nm.startswith("vary_kernel") and all(k[2].startswith("front_") for k in cur)
        if nm.startswith(STARTS) and not declined and (cur is None or not cur or not cur[-1][2].startswith("vary_kernel")):
            if cur:
                sorts.append(cur)
            cur = []
        if cur is not None:
            if inside:
                cur.append((s, e, nm))
            else:
                if cur:
                    sorts.append(cur)
                cur = None
    if cur:
        sorts.append(cur)
    sorts = sorts[a.skip:]
    shape = [k[2] for k in sorts[0]]
    same = [s for s in sorts if [k[2] for k in s] == shape]
    print(f"# {len(sorts)} sorts behind {a.skip} dropped; {len(same)} launch the same {len(shape)} kernels and are averaged")
    n = len(same)
    dur = [sum(s[i][1] - s[i][0] for s in same) / n / 1e3 for i in range(len(shape))]
    gap = [0.0] + [sum(s[i][0] - s[i - 1][1] for s in same) / n / 1e3 for i in range(1, len(shape))]
    span = [(s[-1][1] - s[0][0]) / 1e3 for s in same]
    big = sum(d for d, nm in zip(dur, shape) if nm.startswith(BIG))
    print(f"# per sort, first kernel's start to last kernel's end: mean {sum(span) / n:.1f} us (min {min(span):.1f}, max {max(span):.1f})")
    print(f"# big four {big:.1f} us | other kernels {sum(dur) - big:.1f} us in {sum(not nm.startswith(BIG) for nm in shape)} launches | "
          f"no kernel running {sum(gap):.1f} us")
    print()
    print("## kernels in launch order (us)")
    print(f"{'#':>3} {'idle before':>11} {'duration':>9}  kernel")
    for i, nm in enumerate(shape):
        print(f"{i:3d} {gap[i]:11.1f} {dur[i]:9.1f}  {nm}{'   <-- big four' if nm.startswith(BIG) else ''}")
    print()
    print(f"## idle intervals of at least {a.gap} us")
    for i in range(1, len(shape)):
        if gap[i] >= a.gap:
            key = re.match(r"[A-Za-z_0-9]+", shape[i - 1]).group(0)
            print(f"{gap[i]:8.1f}  behind {shape[i - 1]}, before {shape[i]}: {HOST_CALL.get(key, 'launch boundary / host enqueue')}")
    small = sum(g for g in gap if g < a.gap)
    print(f"{small:8.1f}  all {sum(g < a.gap for g in gap[1:])} shorter boundaries together")
    print()
    print("## kernels outside the big four, by name (us per sort)")
    by = {}
    for d, nm in zip(dur, shape):
        if not nm.startswith(BIG):
            by.setdefault(nm, []).append(d)
    for nm, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{sum(v):8.1f}  {len(v):2d} x  {nm}  ({', '.join(f'{x:.1f}' for x in v)})")


if __name__ == "__main__":
    main()
