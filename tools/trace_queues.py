#!/usr/bin/env python3
"""Reads a rocprofv3 --kernel-trace output directory: which kernels ran on which hardware queue and stream (middle half of the
run), the (queue, stream) pairs -- two streams on one queue serialise --, and what the stream-wait kernels stood in front of.

    python tools/trace_queues.py <dir>
"""
import csv, glob, os, sys

d = sys.argv[1]
rows = []
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    rows += list(csv.DictReader(open(f)))
if not rows:
    print("no trace"); sys.exit(0)
print("columns:", list(rows[0].keys()))


def short(n):
    return n.replace("void ", "").replace("vrt::", "").split("(")[0][:40]


render = [r for r in rows if "k_render" in r["Kernel_Name"]]
t_lo = int(render[len(render) // 4]["Start_Timestamp"]); t_hi = int(render[-len(render) // 4]["End_Timestamp"])
mid = [r for r in rows if int(r["Start_Timestamp"]) >= t_lo and int(r["End_Timestamp"]) <= t_hi]
for key in ("Queue_Id", "Stream_Id"):
    if key not in rows[0]:
        continue
    by = {}
    for r in mid:
        by.setdefault(r[key], {}).setdefault(short(r["Kernel_Name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"-- by {key} (middle half of the run)")
    for q, kinds in sorted(by.items()):
        for k, v in sorted(kinds.items()):
            print(f"  {key}={q:>4s} {k:42s} n={len(v):4d} total {sum(v) / 1e3:8.2f} ms mean {sum(v) / len(v):8.1f} us max {max(v):8.1f}")
# stream x queue pairs
if "Queue_Id" in rows[0] and "Stream_Id" in rows[0]:
    pairs = {}
    for r in mid:
        pairs.setdefault((r["Queue_Id"], r["Stream_Id"]), 0)
        pairs[(r["Queue_Id"], r["Stream_Id"])] += 1
    print("-- (queue, stream): kernels", sorted(pairs.items()))
# wait kernels: what comes next on the same queue, and how long after the wait began did it start
if "Queue_Id" in rows[0]:
    byq = {}
    for r in mid:
        byq.setdefault(r["Queue_Id"], []).append(r)
    held = {}
    for q, v in byq.items():
        v.sort(key=lambda r: int(r["Start_Timestamp"]))
        for a, b in zip(v, v[1:]):
            if "streamOpsWait" in a["Kernel_Name"]:
                k = (q, short(b["Kernel_Name"]), a.get("Stream_Id") == b.get("Stream_Id"))
                held.setdefault(k, []).append((int(a["End_Timestamp"]) - int(a["Start_Timestamp"])) / 1e3)
    print("-- wait kernel followed on its queue by (queue, kernel, same stream): n, total ms, mean us")
    for k, v in sorted(held.items()):
        print("  ", k, len(v), round(sum(v) / 1e3, 2), round(sum(v) / len(v), 1))
span = (t_hi - t_lo) / 1e6
nr = len([r for r in mid if "k_render" in r["Kernel_Name"]])
print(f"middle half: {span:.1f} ms, {nr} render launches, one every {span * 1e3 / max(nr, 1):.1f} us")
