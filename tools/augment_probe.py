#!/usr/bin/env python3
"""The two measurements behind DESIGN.md section 9 "Training-set augmentations" (profiles/augment_kernel_stats.txt).
usage: python tools/augment_probe.py kernel [calls=50]        rnampnn_augment_coords at a C2-sized batch, HIP events around the loop; run it
                                                               under `rocprofv3 --kernel-trace --stats -- python ...` for the kernel's own time
       python tools/augment_probe.py epoch noise|plain [epochs=3]
                                                               config-3-shaped epochs of the main trainer over the 2,083 training lengths +
                                                               2,083 drawn copies: `noise` = AugmentedItems (device noise), `plain` = the same
                                                               copies as plain list entries (the form a commit without the module can run)"""
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
import numpy as np
import torch
from rnampnn.utils import synth
from rnampnn.utils.augment import AugmentedItems, augment_coords

what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
if what == "kernel":
    n_calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    coords, mask, _ = synth.synth_batch(synth.synth_lengths(256, 100, 140, seed=0))
    B, T = mask.shape
    c, m = torch.from_numpy(coords).cuda(), torch.from_numpy(mask).cuda()
    sg = torch.full((B,), 1e-2, device="cuda")
    key = torch.arange(1, B + 1, dtype=torch.int64, device="cuda") * 0x9E3779B97F4A7C1
    off = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.empty_like(c)
    for _ in range(5):
        augment_coords(c, m, sg, key, off, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_calls):
        augment_coords(c, m, sg, key, off, out=out)
    e1.record()
    torch.cuda.synchronize()
    nbytes, us = 2 * c.numel() * 4, e0.elapsed_time(e1) * 1e3 / n_calls
    print(f"B {B} T {T} values {c.numel()} nt {int(mask.sum())} traffic {nbytes / 1e6:.2f} MB: {us:.2f} us per call (events, back to back)")
else:
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils.train import Trainer
    mode = sys.argv[2] if len(sys.argv) > 2 else "noise"
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    lens0 = [int(n) for n in np.load(os.path.join(REPO, "tests", "data", "c3_train_lengths.npy"), allow_pickle=False)]
    items0 = [(synth.synth_rna(n, 100000 + i, seed=3), synth.synth_labels(n, 100000 + i, seed=3)) for i, n in enumerate(lens0)]
    items = AugmentedItems(items0, noise=len(items0), seed=0)
    lens = [int(n) for n in items.lengths]
    if mode == "plain":
        items = [items0[int(s)] for s in items.source]
    model = RNAMPNN(precision="bf16", num_res_neighbours=30, padding_len=4500).to("cuda:0")
    sd = synth.closed_form_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train_precision = "bf16"
    (opt,), (sched,) = model.configure_optimizers(fused=True)
    tr = Trainer(model, opt, sched, world=1, rank=0, seed=0)
    for e in range(epochs):
        print(json.dumps(dict(mode=mode, epoch=e, n=len(lens), **tr.run_epoch(items, lens, e, 512, 32768))), flush=True)
