#!/bin/bash
# tools/design_probe.py under rocprofv3 --kernel-trace --stats, each leg in a run of its own.  usage: tools/kstats_design.sh <outdir> [leg ...]
# (outdir: a git-ignored place such as build/design_stats; legs: sample_score design tied gc distinct count avoid profile dfa dfa_profile nested chain long, the first four by default)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${1:?usage: tools/kstats_design.sh <outdir> [leg ...]}" && OUT=$(cd "$1" && pwd) || exit 1
shift
LEGS=${*:-sample_score design tied gc}
python3 $ROOT/__graft_entry__.py || exit 1    # build OUTSIDE the profiler: the profiled process only loads the library
cd $OUT
for name in $LEGS; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$name -- python3 $ROOT/tools/design_probe.py $name 50 > $OUT/$name.log 2>&1 || { tail -20 $OUT/$name.log; exit 1; }
    cat $OUT/$name.log | grep -v "^W2\|^E2\|rocprof" | tail -20
    python3 - <<PY
import csv, glob
f = sorted(glob.glob("$OUT/$name/*/*kernel_stats.csv"))[-1]
rows = list(csv.DictReader(open(f)))
print(f"-- $name: {len(rows)} kernel names, {sum(float(r['TotalDurationNs']) for r in rows) / 1e6:.2f} ms of kernel time")
for r in rows[:16 if "$name" == "long" else 8]:
    print(f"{r['Name'][:72]:72s} n {int(r['Calls']):5d} avg {float(r['AverageNs'])/1e3:8.2f} us min {float(r['MinNs'])/1e3:8.2f} max {float(r['MaxNs'])/1e3:8.2f} {float(r['Percentage']):5.1f}%")
# k_design by leg of the probe: launches in time order, 55 without constraints, then 55 + 1 with them
t = sorted(glob.glob("$OUT/$name/*/*kernel_trace.csv"))[-1]
# the "tied" leg adds, after those, 55 + 55 + 1 + 55 + 1 launches of k_design_tied: one state per group free / with the hairpins, 64 groups x 4 states
def launches(match):
    return sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])) for r in csv.DictReader(open(t)) if match(r['Kernel_Name'])))
# the "gc" leg adds, after those of k_design, 55 + 55 + 1 launches of k_design_gc: the window 40..60 % free / with the hairpins
# the "distinct" leg adds 8 x 55 launches of k_design_distinct (+ 1 after every fourth): S = 8 then 64, sample then best, free then hairpins
d = launches(lambda n: 'k_design' in n and 'k_design_tied' not in n and 'k_design_gc' not in n and 'k_design_distinct' not in n and 'k_design_count' not in n and 'k_design_avoid' not in n and 'k_design_dfa' not in n and 'k_design_nested' not in n)
g = launches(lambda n: 'k_design_distinct' in n)
e = launches(lambda n: 'k_design_tied' in n)
f = launches(lambda n: 'k_design_gc' in n)
# the "count" leg: after 3 warm launches per variant, 5 alternating rounds of 10 launches per variant - k_design_gc free / hairpins (2 variants
# of its launches) and k_design_count (a) free / (a) hairpins / (b) / (c) (4 variants of its launches); per variant the mean of every round
c = launches(lambda n: 'k_design_count' in n and '_profile' not in n)
# the "avoid" leg: the same rounds - k_design_count (b) (1 variant of its launches: the yardstick of the same run) and k_design_avoid
# S = 8 max_run 3 / S = 8 64-state set / S = 64 max_run 3 (3 variants of its launches)
av = launches(lambda n: 'k_design_avoid' in n and '_profile' not in n)
# the "profile" leg: the same rounds - k_design_count (b) and k_design_avoid max_run 3 (1 variant each: the yardsticks of the same run),
# k_design_count_profile G+C cap T / 0..8 mutations cap 8 / plain under the hairpins (3 variants), k_design_avoid_profile max_run 3 /
# 64-state set (2 variants)
cp = launches(lambda n: 'k_design_count_profile' in n)
ap = launches(lambda n: 'k_design_avoid_profile' in n)
# the "dfa" leg: the same rounds - k_design_avoid max_run 3 (1 variant: the yardstick of the same run) and k_design_dfa on the same automaton
# with every live state accepting / require GGAGG + max_run 3 / require GGAGG and CUUCG + max_run 3 (3 variants of its launches)
dfa = launches(lambda n: 'k_design_dfa' in n and 'k_design_dfa_count' not in n and 'k_design_dfa_profile' not in n)
# the "dfa_profile" leg: the same rounds - k_design_dfa at three automata (3 variants) and k_design_avoid_profile max_run 3 (1 variant): the
# yardsticks of the same run; k_design_dfa_profile at the three automata (3 variants), then 3 + 10 launches on one RNA of 4,498 nt
dp = launches(lambda n: 'k_design_dfa_profile' in n)
# the "nested" leg: the same rounds - k_design_dfa max_run 3 with every live state accepting (1 variant: the yardstick of the same run) and
# k_design_nested on the same automaton without pairs / under the hairpin-rich structure / require GNRA + max_run 3 under it (3 variants)
ns = launches(lambda n: 'k_design_nested' in n)
# the "chain" leg: the same rounds - k_design_dfa max_run 3 with every live state accepting (1 variant) and k_design_count under the G+C
# window 45..60 % / under 0..8 mutations (2 variants): the yardsticks of the same run; k_design_dfa_count on the same automaton with nothing
# counted / under that window / under that budget (3 variants of its launches)
ch = launches(lambda n: 'k_design_dfa_count' in n)
# the "long" leg: every call of a long entry starts with a k_ct_long_leaves launch, so the trace splits into calls; the probe's log names the
# chunks of calls in order.  Per chunk name: the mean per call of the inside pass (level 1 + the level launches), of the walk
# (k_design_count_long) or of the outside pass and the leaves (k_pf_long_*), and their number of launches; the LDS entries by name.
if "$name" == "long":
    rows_t = sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(t))))
    calls, lds = [], {}
    for _, dur, kname in rows_t:
        if 'k_ct_long_leaves' in kname:
            calls.append(dict(inside=0.0, walk=0.0, outside=0.0, leaves=0.0, n=0))
        part = ('inside' if 'k_ct_long' in kname else 'walk' if 'k_design_count_long' in kname else 'leaves' if 'k_pf_long_leaves' in kname
                else 'outside' if 'k_pf_long' in kname else None)
        if part and calls:
            calls[-1][part] += dur / 1e3
            calls[-1]['n'] += 1
        for short in ('k_design_gc', 'k_design_count_profile', 'k_design_count'):
            if part is None and short in kname:
                lds.setdefault(short, []).append(dur / 1e3)
                break
    chunks = [line.strip().split('|')[1:] for line in open("$OUT/$name.log") if line.startswith('long-calls|')]
    at, by_name, order = 0, {}, []
    for cname, n in chunks:
        n = int(n)
        if ', lds' in cname:
            continue                                                # an LDS entry: one launch, reported by kernel name below
        if cname not in by_name:
            by_name[cname] = []
            order.append(cname)
        by_name[cname] += calls[at:at + n]
        at += n
    print(f"long: {len(calls)} calls of a long entry in the trace, {at} in the probe's log")
    for cname in order:
        if '(warm)' in cname or '(check)' in cname:
            continue
        cs = by_name[cname]
        mean = lambda k: sum(c[k] for c in cs) / len(cs)
        tail = (f"walk {mean('walk'):9.2f} us" if mean('walk') else f"root + outside pass {mean('outside'):9.2f} us, leaves {mean('leaves'):9.2f} us")
        print(f"long, {cname}: {len(cs)} calls x {cs[0]['n']} launches, inside pass {mean('inside'):9.2f} us, {tail}, kernel time per call "
              f"{mean('inside') + mean('walk') + mean('outside') + mean('leaves'):9.2f} us")
    for short, v in lds.items():
        body = sorted(v[3:])
        print(f"{short} (the LDS entry of the same run, C2, 3 warm launches dropped): {len(body)} launches, mean {sum(body) / len(body):.2f} us "
              f"({body[0]:.2f} .. {body[-1]:.2f}, median {body[len(body) // 2]:.2f})")
    raise SystemExit(0)
def by_round(seq, variants, v):
    body = seq[3 * variants:]
    return [[x[1] / 1e3 for x in body[10 * (variants * r + v):10 * (variants * r + v) + 10]] for r in range(5)]
def report(table):
    for kernel, label, rs in table:
        means = [sum(r) / len(r) for r in rs]
        flat = sorted(x for r in rs for x in r)
        print(f"{kernel}, {label}: 5 rounds x 10 launches, mean {sum(flat) / len(flat):.2f} us ({flat[0]:.2f} .. {flat[-1]:.2f}, median {flat[len(flat) // 2]:.2f}); "
              f"round means {' '.join(f'{v:.2f}' for v in means)} (spread {max(means) - min(means):.2f})")
if dp:
    autos = ("max_run 3, every live state accepting (13 live states)", "require GGAGG and CUUCG, max_run 3 (89 states, 73 live)",
             "require a 26-mer and a 39-mer (256 states, all live)")
    report(tuple(("k_design_dfa", f"{a}, S = 8", by_round(dfa, 3, v)) for v, a in enumerate(autos)) +
           (("k_design_avoid_profile", "max_run 3 (13 live states)", by_round(ap, 1, 0)),) +
           tuple(("k_design_dfa_profile", a, by_round(dp, 3, v)) for v, a in enumerate(autos)))
    m = [sum(x for r in by_round(s, k, v) for x in r) / 50 for s, k, v in ((dfa, 3, 0), (dfa, 3, 1), (dfa, 3, 2), (ap, 1, 0), (dp, 3, 0), (dp, 3, 1), (dp, 3, 2))]
    print(f"k_design_dfa_profile / k_design_dfa (S = 8) on the same automaton: {m[4] / m[0]:.3f} at 13 live states, {m[5] / m[1]:.3f} at 73, "
          f"{m[6] / m[2]:.3f} at 256; k_design_dfa_profile / k_design_avoid_profile at 13 live states: {m[4] / m[3]:.3f}; "
          f"k_design_dfa_profile / (k_design_dfa + k_design_avoid_profile) at 13 live states: {m[4] / (m[0] + m[3]):.3f}")
    one = sorted(x[1] / 1e3 for x in dp[3 * 3 + 150 + 3:3 * 3 + 150 + 13])
    print(f"k_design_dfa_profile, one RNA of 4,498 nt, max_run 3 (13 live states): {len(one)} launches, mean {sum(one) / len(one):.2f} us "
          f"({one[0]:.2f} .. {one[-1]:.2f}, median {one[len(one) // 2]:.2f})")
elif ch:
    report((("k_design_dfa", "max_run 3, every live state accepting (13 live states), S = 8", by_round(dfa, 1, 0)),
            ("k_design_count", "C|G counted, cap T, window 45..60 %, S = 8", by_round(c, 2, 0)),
            ("k_design_count", "random reference, 0..8 mutations, cap 8, S = 8", by_round(c, 2, 1)),
            ("k_design_dfa_count", "max_run 3 (13 live states), nothing counted, cap 0, S = 8", by_round(ch, 3, 0)),
            ("k_design_dfa_count", "max_run 3 (13 live states), G+C window 45..60 %, cap T, S = 8", by_round(ch, 3, 1)),
            ("k_design_dfa_count", "max_run 3 (13 live states), 0..8 mutations, cap 8, S = 8", by_round(ch, 3, 2))))
    m = [sum(x for r in by_round(s, k, v) for x in r) / 50 for s, k, v in ((dfa, 1, 0), (ch, 3, 0), (ch, 3, 1), (ch, 3, 2), (c, 2, 0), (c, 2, 1))]
    print(f"k_design_dfa_count / k_design_dfa, nothing counted: {m[1] / m[0]:.3f}; G+C window: {m[2] / m[0]:.3f} of k_design_dfa, {m[2] / m[4]:.3f} of "
          f"k_design_count; budget of 8: {m[3] / m[0]:.3f} of k_design_dfa, {m[3] / m[5]:.3f} of k_design_count")
elif ns:
    report((("k_design_dfa", "max_run 3, every live state accepting (13 live states), no pairs, S = 8", by_round(dfa, 1, 0)),
            ("k_design_nested", "max_run 3 (13 live states), no pairs, S = 8", by_round(ns, 3, 0)),
            ("k_design_nested", "max_run 3 (13 live states), hairpin-rich nested structure, S = 8", by_round(ns, 3, 1)),
            ("k_design_nested", "require GNRA, max_run 3 (61 states, 53 live), the same structure, S = 8", by_round(ns, 3, 2))))
    m = [sum(x for r in by_round(s, k, v) for x in r) / 50 for s, k, v in ((dfa, 1, 0), (ns, 3, 0))]
    print(f"k_design_nested / k_design_dfa on the same automaton without pairs: {m[1] / m[0]:.3f}")
elif dfa:
    report((("k_design_avoid", "max_run 3 (13 live states), S = 8, no constraints", by_round(av, 1, 0)),
            ("k_design_dfa", "max_run 3, every live state accepting (13 live states), S = 8", by_round(dfa, 3, 0)),
            ("k_design_dfa", "require GGAGG, max_run 3 (38 states, 30 live), S = 8", by_round(dfa, 3, 1)),
            ("k_design_dfa", "require GGAGG and CUUCG, max_run 3 (89 states, 73 live), S = 8", by_round(dfa, 3, 2))))
    m = [sum(x for r in by_round(s, k, v) for x in r) / 50 for s, k, v in ((av, 1, 0), (dfa, 3, 0))]
    print(f"k_design_dfa / k_design_avoid on the same automaton: {m[1] / m[0]:.3f} (the price of the global table)")
elif cp:
    report((("k_design_count", "(b) random reference, 0..8 mutations, cap 8, S = 8, no constraints", by_round(c, 1, 0)),
            ("k_design_avoid", "max_run 3 (13 live states), S = 8, no constraints", by_round(av, 1, 0)),
            ("k_design_count_profile", "G+C window 40..60 %, cap T, no constraints", by_round(cp, 3, 0)),
            ("k_design_count_profile", "0..8 mutations, cap 8, no constraints", by_round(cp, 3, 1)),
            ("k_design_count_profile", "plain, cap 0, hairpin pairs + GNRA + bias", by_round(cp, 3, 2)),
            ("k_design_avoid_profile", "max_run 3 (13 live states), no constraints", by_round(ap, 2, 0)),
            ("k_design_avoid_profile", "64-state set (57 live states), no constraints", by_round(ap, 2, 1))))
elif av:
    report((("k_design_count", "(b) random reference, 0..8 mutations, cap 8, S = 8, no constraints", by_round(c, 1, 0)),
            ("k_design_avoid", "max_run 3 (13 live states), S = 8, no constraints", by_round(av, 3, 0)),
            ("k_design_avoid", "64-state set (57 live states), S = 8, no constraints", by_round(av, 3, 1)),
            ("k_design_avoid", "max_run 3 (13 live states), S = 64, no constraints", by_round(av, 3, 2))))
elif c:
    report((("k_design_gc", "window 40..60 %, no constraints", by_round(f, 2, 0)),
                              ("k_design_count", "(a) C|G counted, cap T, window 40..60 %, no constraints", by_round(c, 4, 0)),
                              ("k_design_gc", "window 40..60 %, hairpin pairs + GNRA + bias", by_round(f, 2, 1)),
                              ("k_design_count", "(a) C|G counted, cap T, window 40..60 %, hairpin pairs + GNRA + bias", by_round(c, 4, 1)),
                              ("k_design_count", "(b) random reference, 0..8 mutations, cap 8, no constraints", by_round(c, 4, 2)),
                              ("k_design_count", "(c) compatible reference, 0..8 mutations, cap 8, hairpins", by_round(c, 4, 3))))
    f = []                                                          # (its k_design_gc launches are reported above, by round)
for kernel, label, part in (("k_design", "no constraints", d[:55]), ("k_design", "hairpin pairs + GNRA + bias", d[55:111]),
                            ("k_design_tied", "one state per group, no constraints", e[:55]),
                            ("k_design_tied", "one state per group, hairpin pairs + GNRA + bias", e[55:111]),
                            ("k_design_tied", "64 groups x 4 states, one 3-node chain per group", e[111:]),
                            ("k_design_gc", "window 40..60 %, no constraints", f[:55]),
                            ("k_design_gc", "window 40..60 %, hairpin pairs + GNRA + bias", f[55:])) + tuple(
        ("k_design_distinct", f"S = {S}, {mode}, {leg}", g[221 * i + 110 * j + 55 * k:221 * i + 110 * j + 55 * k + 55])
        for i, S in enumerate((8, 64)) for j, mode in enumerate(("sample", "best"))
        for k, leg in enumerate(("no constraints", "hairpin pairs + GNRA + bias"))):
    if part:
        v = sorted(x[1] / 1e3 for x in part)
        print(f"{kernel}, {label}: {len(v)} launches, mean {sum(v) / len(v):.2f} us ({v[0]:.2f} .. {v[-1]:.2f}, median {v[len(v) // 2]:.2f})")
PY
done
