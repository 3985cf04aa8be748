#!/usr/bin/env python3
"""LRU model of the Infinity Cache under the fused ResMPNN launches of a C2 forward (docs/experiments.md, sweep direction).

The stream, in units of 64 KiB: e (30,559 blocks x 8 KiB = 239 MiB) is read and written in place by every launch; the eight XCD-contiguous
eighths advance together; the node tables a launch gathers (~66 MB) enter in proportion to the position; the node update between two launches
moves ~62 MB.  Two treatments of that other traffic bracket the truth: "same lines" - the tables are the same lines in every launch and the
node update rewrites exactly them (they take their room once); "fresh lines" - every byte of it is a line never used again (it takes room
every time).  Assumptions: LRU replacement, allocation on stores, a read after a write hits.  Prints the share of e reads that hit, launches 2 - 10, for the ascending sweep and for the
alternating one, at several effective capacities.

    python tools/lru_sweep_model.py [--blocks 30559] [--launches 10]
"""
import argparse
from collections import OrderedDict

UNIT = 64 * 1024


def simulate(n_units, cap_units, launches, alternate, table_units, node_units, fresh_lines):
    cache, fresh = OrderedDict(), [0]

    def touch(key):
        hit = key in cache
        if hit:
            cache.move_to_end(key)
        else:
            cache[key] = None
            if len(cache) > cap_units:
                cache.popitem(last=False)
        return hit

    def pollute(n):
        for _ in range(n):
            fresh[0] += 1
            touch(("x", fresh[0]))

    chunk = (n_units + 7) // 8
    hits = reads = 0
    for l in range(launches):
        rev = alternate and (l & 1)
        done_tab = 0
        for t in range(chunk):
            pos = chunk - 1 - t if rev else t
            for x in range(8):
                u = x * chunk + pos
                if u >= n_units:
                    continue
                h = touch(("e", u))              # the read ...
                if l > 0:
                    hits += h
                    reads += 1
                touch(("e", u))                  # ... and the write back in place
            want = table_units * (t + 1) // chunk
            if fresh_lines:
                pollute(want - done_tab)
            else:
                for i in range(done_tab, want):
                    touch(("t", i))
            done_tab = want
        if fresh_lines:
            pollute(node_units)
        else:
            for i in range(table_units):
                touch(("t", i))
            pollute(max(0, node_units - table_units))
    return hits / max(reads, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=30559, help="residues of the batch (8 KiB of e each)")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--table-mb", type=float, default=66.0)
    ap.add_argument("--node-mb", type=float, default=62.0)
    a = ap.parse_args()
    n_units = (a.blocks * 8192 + UNIT - 1) // UNIT
    tab, node = int(a.table_mb * 1e6 / UNIT), int(a.node_mb * 1e6 / UNIT)
    print(f"e: {a.blocks} blocks = {n_units * UNIT / 2 ** 20:.0f} MiB; tables {a.table_mb:.0f} MB per launch, node update {a.node_mb:.0f} MB between launches")
    for cap_mib in (256, 224, 192, 160):
        cap = cap_mib * 2 ** 20 // UNIT
        r = [simulate(n_units, cap, a.launches, alt, tab, node, fresh) for fresh in (False, True) for alt in (False, True)]
        print(f"capacity {cap_mib:3d} MiB: e-read hits, same lines: ascending {r[0]:6.1%}, alternating {r[1]:6.1%};  fresh lines: ascending {r[2]:6.1%}, "
              f"alternating {r[3]:6.1%}")


if __name__ == "__main__":
    main()
