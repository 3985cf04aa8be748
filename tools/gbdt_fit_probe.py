#!/usr/bin/env python3
"""Wall time of the device-side tree fit (`GBDTReadout.fit`, csrc/gbdt_fit.hip) on a seeded learnable task.

    python tools/gbdt_fit_probe.py --rows 30559 --rounds 150              # the reference's model shape on one C2 batch of embeddings
    python tools/gbdt_fit_probe.py --rows 1200000 --rounds 10             # the size of the config-3 training set (time per round)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gbdt_fit_probe.py --rows 30559 --rounds 20 --repeats 1

The last form gives the per-kernel split (`*kernel_stats.csv`: k_hist is the histogram build); run it on its own, never together with
counter collection.  The library must be built beforehand (`python __graft_entry__.py`): this script never compiles."""
import argparse, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "rna-mpnn_amd"))
import __graft_entry__ as g
g.load_only()
from rnampnn.model.xgb import GBDTReadout

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=30559)
ap.add_argument("--features", type=int, default=256)
ap.add_argument("--rounds", type=int, default=150)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
gen = torch.Generator(device="cuda").manual_seed(1)
X = torch.randn(args.rows, args.features, device="cuda", generator=gen)
noise = torch.randn(args.rows, 2, device="cuda", generator=gen)
y = ((X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.4 * noise[:, 0] > 0).long() + 2 * (X[:, 3] - 0.7 * X[:, 5] + 0.4 * noise[:, 1] > 0.3).long())
kw = dict(n_estimators=args.rounds, max_depth=args.depth, subsample=0.8, colsample_bytree=0.8, seed=42)
GBDTReadout.fit(X[:2048], y[:2048], n_estimators=1, max_depth=2)          # runtime warm-up
times = []
for _ in range(args.repeats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model = GBDTReadout.fit(X, y, **kw)
    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
# integer adds of the histogram build: sampled rows x sampled features x (g, h) per level and tree
adds = 0.8 * args.rows * int(0.8 * args.features) * 2 * args.depth * args.rounds * 4
print(json.dumps(dict(metric="gbdt_fit_seconds", value=min(times), all=times, rows=args.rows, features=args.features, rounds=args.rounds,
                      depth=args.depth, nodes=int(model.arrays["tree_offsets"][-1]), train_score=model.score(X, y),
                      hist_adds_upper_bound=adds)))
