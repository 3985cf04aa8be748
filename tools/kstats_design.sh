#!/bin/bash
# tools/design_probe.py under rocprofv3 --kernel-trace --stats, each leg in a run of its own.  usage: tools/kstats_design.sh <outdir>  (a git-ignored
# place such as build/design_stats)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${1:?usage: tools/kstats_design.sh <outdir>}" && OUT=$(cd "$1" && pwd) || exit 1
python3 $ROOT/__graft_entry__.py || exit 1    # build OUTSIDE the profiler: the profiled process only loads the library
cd $OUT
for name in sample_score design; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$name -- python3 $ROOT/tools/design_probe.py $name 50 > $OUT/$name.log 2>&1 || { tail -20 $OUT/$name.log; exit 1; }
    cat $OUT/$name.log | grep -v "^W2\|^E2\|rocprof" | tail -20
    python3 - <<PY
import csv, glob
f = sorted(glob.glob("$OUT/$name/*/*kernel_stats.csv"))[-1]
rows = list(csv.DictReader(open(f)))
print(f"-- $name: {len(rows)} kernel names, {sum(float(r['TotalDurationNs']) for r in rows) / 1e6:.2f} ms of kernel time")
for r in rows[:8]:
    print(f"{r['Name'][:72]:72s} n {int(r['Calls']):5d} avg {float(r['AverageNs'])/1e3:8.2f} us min {float(r['MinNs'])/1e3:8.2f} max {float(r['MaxNs'])/1e3:8.2f} {float(r['Percentage']):5.1f}%")
# k_design by leg of the probe: launches in time order, 55 without constraints, then 55 + 1 with them
t = sorted(glob.glob("$OUT/$name/*/*kernel_trace.csv"))[-1]
d = sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])) for r in csv.DictReader(open(t)) if 'k_design' in r['Kernel_Name']))
for label, part in (("no constraints", d[:55]), ("hairpin pairs + GNRA + bias", d[55:])):
    if part:
        v = sorted(x[1] / 1e3 for x in part)
        print(f"k_design, {label}: {len(v)} launches, mean {sum(v) / len(v):.2f} us ({v[0]:.2f} .. {v[-1]:.2f}, median {v[len(v) // 2]:.2f})")
PY
done
