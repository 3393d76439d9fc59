#!/usr/bin/env python3
"""Per-step timeline of a rocprofv3 kernel trace of bench.py: for the last timed step, every
dispatch with its stream, start offset and duration, plus the step's busy / idle time.
    python3 tools/trace_timeline.py bench_out/trace_c2_kernels.csv [marker_kernel]
With --steady N: a summary over the last N whole steps instead -- per kernel the median / min / max
of its duration (summed over a step's dispatches), the step span, and for every kernel of another
queue that starts inside a fused gate kernel's span its median / max duration there.
    python3 tools/trace_timeline.py bench_out/trace_c2_kernels.csv --steady 20"""
import csv
import statistics
import sys
from collections import defaultdict

argv = sys.argv[1:]
steady = 0
if "--steady" in argv:
    i = argv.index("--steady")
    steady = int(argv[i + 1])
    del argv[i:i + 2]
rows = list(csv.DictReader(open(argv[0])))
marker = argv[1] if len(argv) > 1 else None
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
rows.sort(key=lambda r: r["s"])
if marker is None:  # the step's first kernel: the fused prologue (round 3) or the sampler before it
    marker = next((m for m in ("step_prologue_kernel", "sample_negatives_kernel")
                   if any(m in r["Kernel_Name"] for r in rows)), "step_prologue_kernel")
starts = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
if len(starts) < 3:
    sys.exit(f"marker {marker} found {len(starts)} times")


def short(r):
    return r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("ttamm::", "").split("(")[0][:70]


def steady_summary(n):
    if len(starts) < n + 2:
        sys.exit(f"marker {marker} found {len(starts)} times: fewer than {n} whole steps before the last")
    bounds = starts[-(n + 2):-1]  # n whole steps, the last (possibly cut) one left out
    spans, per_kernel, inside = [], defaultdict(list), defaultdict(list)
    for i0, i1 in zip(bounds, bounds[1:]):
        step = rows[i0:i1]
        spans.append((rows[i1]["s"] - step[0]["s"]) / 1e3)
        agg = defaultdict(float)
        for r in step:
            agg[short(r)] += (r["e"] - r["s"]) / 1e3
        for k, v in agg.items():
            per_kernel[k].append(v)
        for g in step:
            if "gate_fwd_kernel" not in g["Kernel_Name"] and "gate_bwd_kernel" not in g["Kernel_Name"]:
                continue
            gname = short(g).split("<")[0]
            for r in step:
                if r["Queue_Id"] != g["Queue_Id"] and g["s"] <= r["s"] < g["e"]:
                    inside[gname, short(r)].append((r["e"] - r["s"]) / 1e3)
    print(f"{n} steps: span median {statistics.median(spans):.1f} us, min {min(spans):.1f}, max {max(spans):.1f}")
    print("by kernel, us per step (median  min  max  steps seen):")
    for k, v in sorted(per_kernel.items(), key=lambda kv: -statistics.median(kv[1])):
        print(f"  {statistics.median(v):8.1f} {min(v):8.1f} {max(v):8.1f} {len(v):4d}  {k}")
    print("dispatches of another queue that start inside a gate kernel's span, us (median  max  count):")
    for (g, k), v in sorted(inside.items()):
        print(f"  {statistics.median(v):8.1f} {max(v):8.1f} {len(v):4d}  in {g}: {k}")


if steady:
    steady_summary(steady)
    sys.exit(0)
i0, i1 = starts[-3], starts[-2]  # a full step in the timed region
step = rows[i0:i1]
t0 = step[0]["s"]
t1 = rows[i1]["s"]
print(f"step span {(t1 - t0) / 1e3:.1f} us, {len(step)} dispatches")
busy = 0
cur_s = cur_e = None
for r in step:
    if cur_e is None or r["s"] > cur_e:
        if cur_e is not None:
            busy += cur_e - cur_s
        cur_s, cur_e = r["s"], r["e"]
    else:
        cur_e = max(cur_e, r["e"])
busy += cur_e - cur_s
print(f"GPU busy (union) {busy / 1e3:.1f} us, idle {(t1 - t0 - busy) / 1e3:.1f} us")
agg = defaultdict(float)
for r in step:
    name = short(r)
    print(f"  q{r['Queue_Id']:>2} +{(r['s'] - t0) / 1e3:8.1f} {(r['e'] - r['s']) / 1e3:8.1f} us  {name}  grid={r['Grid_Size_X']}")
    agg[name] += (r["e"] - r["s"]) / 1e3
print("by kernel (sum of durations, us):")
for k, v in sorted(agg.items(), key=lambda kv: -kv[1]):
    print(f"  {v:8.1f}  {k}")
