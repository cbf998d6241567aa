#!/usr/bin/env python3
"""One steady-state step of bench.py from a rocprofv3 kernel trace: every kernel's start and end on its queue, how long k_octree
runs beside k_fast_cells or k_orient_desc, and the idle time of the GPU inside the step.
usage: python3 tools/orb_lanes_trace.py <dir with *_kernel_trace.csv> [steps back from the last, default 5]

A step ends with the matcher (k_hamming_*), which waits for everything of its step and is waited for by everything of the next."""
import csv
import glob
import sys

d = sys.argv[1]
back = int(sys.argv[2]) if len(sys.argv) > 2 else 5
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = []
for r in csv.DictReader(open(f)):
    name = r["Kernel_Name"].split("(")[0].replace("void ", "")
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Queue_Id", "?")))
rows.sort()
ends = [i for i, r in enumerate(rows) if r[2].startswith("k_hamming")]
last, prev = ends[-back], ends[-back - 1]
step = rows[prev + 1:last + 1]
t0 = rows[prev][1]                       # the previous step's matcher ends
print("step of %d kernels, %.1f us from the previous matcher's end to this one's" % (len(step), (step[-1][1] - t0) / 1e3))
print("%-22s %-6s %9s %9s %9s" % ("kernel", "queue", "start us", "end us", "us"))
for s, e, n, q in step:
    print("%-22s %-6s %9.1f %9.1f %9.1f" % (n[:22], q, (s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3))


def overlap(a, b):
    return sum(max(0, min(e1, e2) - max(s1, s2)) for s1, e1 in a for s2, e2 in b)


iv = lambda p: [(s, e) for s, e, n, q in step if n.startswith(p)]
octs = iv("k_octree")
for k, (s, e) in enumerate(octs):
    beside = overlap([(s, e)], iv("k_fast_cells") + iv("k_orient_desc"))
    print("k_octree %d: %.1f us, %.1f us of them beside k_fast_cells or k_orient_desc" % (k, (e - s) / 1e3, beside / 1e3))
# idle: the part of [t0, end of the step] no kernel covers
idle, end = 0, t0
for s, e, n, q in step:
    if s > end:
        idle += s - end
    end = max(end, e)
busy = sum(e - s for s, e, n, q in step)
print("idle gaps %.1f us; kernel time summed %.1f us over a span of %.1f us" % (idle / 1e3, busy / 1e3, (end - t0) / 1e3))
