#!/usr/bin/env python
"""How long the frame-MLP kernel lasts inside the pipeline, by what runs beside it: digest of
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps 60 --warmup 20
(a run of its own, no counters).  Every steady-state launch of frame_mlps_wr_kernel (the first quarter of the launches is
dropped) is grouped by the number of recurrences (control_gru*) resident when it starts and overlapping it at all; per group:
launches, median / mean / min / max duration from the start and end stamps, and how many oscillator kernels overlap it on
average - a launch that overlaps one mostly WAITS for its CUs, so its duration says little about the kernel.
    python tools/frame_mlps_trace_digest.py DIR          (profiles/frame_mlps_12wave_ab.txt)"""
import csv
import glob
import os
import statistics as st
import sys

root = sys.argv[1]
path = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))[0]
rows = list(csv.DictReader(open(path)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
span = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
mlp = [r for r in rows if "frame_mlps_wr_kernel" in r["Kernel_Name"]]
gru = [span(r) for r in rows if "control_gru" in r["Kernel_Name"]]
osc = [span(r) for r in rows if "exciter_newt" in r["Kernel_Name"]]
print(f"# {len(rows)} kernels, {len(mlp)} frame-MLP launches, {len(gru)} recurrences")
for n in sorted({(r["Kernel_Name"][:90], r.get("Workgroup_Size", r.get("Workgroup_Size_X", "?")), r.get("Grid_Size", r.get("Grid_Size_X", "?")))
                 for r in mlp}):
    print("#  ", n)
groups = {}
for r in mlp[len(mlp) // 4:]:
    a, b = span(r)
    at_start = sum(1 for ga, gb in gru if ga <= a < gb)
    at_all = sum(1 for ga, gb in gru if ga < b and gb > a)
    groups.setdefault((at_start, at_all), []).append(((b - a) / 1e3, sum(1 for oa, ob in osc if oa < b and ob > a)))
print("recurrences resident at start | overlapping at all | launches | median us | mean us | min | max | mean oscillator kernels overlapping")
for k in sorted(groups):
    d = [x[0] for x in groups[k]]
    print(f"{k[0]:3d} {k[1]:3d} {len(d):5d} {st.median(d):8.1f} {st.mean(d):8.1f} {min(d):8.1f} {max(d):8.1f} {st.mean(x[1] for x in groups[k]):.2f}")
d = [x[0] for g in groups.values() for x in g]
print(f"all: {len(d)} launches, median {st.median(d):.1f} us, mean {st.mean(d):.1f} us")
gd = [(b - a) / 1e3 for a, b in gru[len(gru) // 4:]]
print(f"recurrence: {len(gd)} launches, median {st.median(gd):.1f} us, mean {st.mean(gd):.1f} us")
