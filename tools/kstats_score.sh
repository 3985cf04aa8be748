#!/bin/bash
# tools/score_probe.py under rocprofv3 --kernel-trace --stats, each leg in a run of its own.  usage: tools/kstats_score.sh <outdir>  (a git-ignored
# place such as build/score_stats)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${1:?usage: tools/kstats_score.sh <outdir>}" && OUT=$(cd "$1" && pwd) || exit 1
python3 $ROOT/__graft_entry__.py || exit 1    # build OUTSIDE the profiler: the profiled process only loads the library
cd $OUT
for leg in "kernel 50" "validate 2"; do
    name=${leg%% *}
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$name -- python3 $ROOT/tools/score_probe.py $leg > $OUT/$name.log 2>&1 || { tail -20 $OUT/$name.log; exit 1; }
    cat $OUT/$name.log | grep -v "^W2\|^E2\|rocprof" | tail -20
    python3 - <<PY
import csv, glob
f = sorted(glob.glob("$OUT/$name/*/*kernel_stats.csv"))[-1]
rows = list(csv.DictReader(open(f)))
tot = sum(float(r['TotalDurationNs']) for r in rows)
print(f"-- $name: {len(rows)} kernel names, {tot / 1e6:.2f} ms of kernel time")
for r in rows:
    if rows.index(r) < 12 or 'k_score' in r['Name'] or 'argmax' in r['Name']:
        print(f"{r['Name'][:72]:72s} n {int(r['Calls']):5d} avg {float(r['AverageNs'])/1e3:8.2f} us min {float(r['MinNs'])/1e3:8.2f} max {float(r['MaxNs'])/1e3:8.2f} {float(r['Percentage']):5.1f}%")
PY
done
