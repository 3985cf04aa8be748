#!/usr/bin/env python3
"""The two measurements behind DESIGN.md section 9 "RNAMPNN epoch pipeline" (profiles/rnampnn_score_kernel_stats.txt).
usage: python tools/score_probe.py kernel [calls=50]     rnampnn_score at the C2 batch (256 RNAs x 100..140 nt): the validation outputs
                                                          (S = 0) and the same plus 8 sampled sequences, HIP events around each loop
       python tools/score_probe.py validate [reps=3]     a config-3-shaped validation pass (every 10th of the 2,083 training lengths: 209
                                                          RNAs, 1 .. 4,417 nt): Trainer.validate (forward + rnampnn_argmax_recovery, the
                                                          parent commit's pass) and Trainer.validate_metrics (forward + rnampnn_score),
                                                          alternated in one process, wall time between two synchronisations
Run either under `rocprofv3 --kernel-trace --stats -- python ...` (a run of its own) for the kernels' own times."""
import json
import os
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
import numpy as np
import torch
from rnampnn.model.rnampnn import RNAMPNN, sample_from_logits, score_logits
from rnampnn.utils import synth

what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
if what == "kernel":
    n_calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    lens = synth.synth_lengths(256, 100, 140, seed=0)
    _, mask, labels = synth.synth_batch(lens)
    B, T = mask.shape
    g = torch.Generator().manual_seed(0)
    m = torch.from_numpy(mask).cuda()
    logits = (3.0 * torch.randn(B, T, 4, generator=g)).cuda() * m[..., None]
    lab = torch.from_numpy(np.asarray(labels)).to(torch.int32).cuda()
    lab = lab.argmax(-1).to(torch.int32) if lab.dim() == 3 else lab
    seqs = sample_from_logits(logits, m, 1.0, 8, seed=1)
    legs = (("validation outputs, S = 0", dict(labels=lab, want=("correct", "valid", "label_loss", "label_nll"))),
            ("all outputs, S = 8", dict(labels=lab, seqs=seqs, want=("correct", "valid", "pred", "label_loss", "label_nll", "seq_nll", "seq_match"))))
    for name, kw in legs:
        for _ in range(5):
            score_logits(logits, mask=m, **kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_calls):
            score_logits(logits, mask=m, **kw)
        e1.record()
        torch.cuda.synchronize()
        print(f"B {B} T {T} nt {int(mask.sum())} {name}: {e0.elapsed_time(e1) * 1e3 / n_calls:.2f} us per call (events, back to back, "
              f"output allocation included)")
else:
    from rnampnn.utils.train import Trainer
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    lens = [int(n) for n in np.load(os.path.join(REPO, "tests", "data", "c3_train_lengths.npy"), allow_pickle=False)][::10]
    items = [(synth.synth_rna(n, 200000 + i, seed=3), synth.synth_labels(n, 200000 + i, seed=3)) for i, n in enumerate(lens)]
    for prec in ("bf16", "f32"):
        model = RNAMPNN(precision=prec, num_res_neighbours=30, padding_len=4500).to("cuda:0")
        sd = synth.closed_form_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        tr = Trainer(model, None)
        passes = (("validate", lambda: tr.validate(items, lens, 512, 32768)), ("validate_metrics", lambda: tr.validate_metrics(items, lens, 512, 32768)))
        for _, fn in passes:
            fn()                                                    # warm: workspace, allocator
        for r in range(reps):
            for name, fn in passes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                print(json.dumps(dict(precision=prec, rep=r, what=name, rnas=len(lens), nt=sum(lens), ms=round((time.perf_counter() - t0) * 1e3, 2),
                                      out=out)), flush=True)
