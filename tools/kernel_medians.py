"""Per-kernel device time from a rocprofv3 kernel trace (dev tool; needs no GPU):
python tools/kernel_medians.py KERNEL_TRACE.csv [substring of the kernel names] [N]
For every kernel whose name holds the substring: the number of launches in the trace, and median, minimum and maximum of
End_Timestamp - Start_Timestamp over its last N launches in start order (all of them without N), in microseconds.  The
trace comes from `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- COMMAND` (DIR/*/*kernel_trace.csv)."""
import collections
import csv
import statistics
import sys

path = sys.argv[1]
pattern = sys.argv[2] if len(sys.argv) > 2 else ""
last = int(sys.argv[3]) if len(sys.argv) > 3 else 0
runs = collections.defaultdict(list)
with open(path, newline="") as f:
    for r in csv.DictReader(f):
        if pattern in r["Kernel_Name"]:
            runs[r["Kernel_Name"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
total = 0.0
for name, ts in sorted(runs.items(), key=lambda kv: min(kv[1])):       # in the order of their first launch
    ts.sort()
    us = [(e - s) / 1e3 for s, e in (ts[-last:] if last else ts)]
    short = name.replace("(anonymous namespace)::", "").removeprefix("void ").split("(")[0]
    total += statistics.median(us)
    print(f"{short:<24} launches {len(ts)} taken {len(us)} median {statistics.median(us):.2f} min {min(us):.2f} "
          f"max {max(us):.2f}")
print(f"sum of medians {total:.2f}")
