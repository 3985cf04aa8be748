#!/usr/bin/env python3
"""Throughput of the rdesign forward (row F3) on a C2-shaped batch (64 RNAs x 100..500 nt): tools/rdesign_probe.py [precision] [steps].
Prints one JSON line (nt/s, ms/step).  Run under tools/kstats_rdesign.sh for the per-kernel breakdown.

tools/rdesign_probe.py --train [steps] [--train-precision {f32,bf16}] [--no-trace] [--out DIR]: the TRAINING step (exact f32 by default, or the
bf16-mixed one) of a precision="f32" model at the same shape (dropout 0.1): HIP events around
>= 20 warmed steps of loss_and_grad + FlatAdam.step, the f32 forward of the same run next to it, workspace / tape bytes; before that (and
before this process touches the GPU) one traced run of three steps in a child process under `rocprofv3 --kernel-trace --stats`, whose
per-kernel table is printed and kept under DIR (default build/rdesign_train)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_precision(argv):
    tp = argv[argv.index("--train-precision") + 1] if "--train-precision" in argv else "f32"
    if tp not in ("f32", "bf16"):
        raise SystemExit("--train-precision takes f32 or bf16")
    return tp


def _trace(out_dir, train_precision):
    """One `rocprofv3 --kernel-trace --stats` run of a fresh child (this process has not opened the GPU yet) -> per-kernel table."""
    import csv
    import glob
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--train", "3", "--no-trace", "--train-precision", train_precision]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=420, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"))
    open(os.path.join(out_dir, "prof.log"), "wb").write(r.stdout)
    if r.returncode != 0:
        raise SystemExit(f"traced run failed with status {r.returncode}: see {out_dir}/prof.log")
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"rocprofv3 wrote no kernel_stats.csv under {out_dir}")
    rows = list(csv.DictReader(open(files[-1])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    lines = [f"{r['Name'][:72]:72s} n {int(r['Calls']):6d} avg {float(r['AverageNs']) / 1e3:9.1f} us  total {float(r['TotalDurationNs']) / 1e6:9.2f} ms "
             f"{float(r['Percentage']):5.1f}%" for r in rows[:24]]
    lines.append(f"all kernels of the traced child (3 warm-up + 3 timed steps, 3 + 3 f32 forwards, optimiser): {tot / 1e6:.1f} ms")
    open(os.path.join(out_dir, "kernel_stats.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def _out_dir(argv):
    return os.path.abspath(argv[argv.index("--out") + 1]) if "--out" in argv else os.path.join(ROOT, "build", "rdesign_train")


if "--train" in sys.argv and "--no-trace" not in sys.argv:      # first, while this process has loaded nothing of the GPU stack
    _trace(_out_dir(sys.argv), _train_precision(sys.argv))

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "rna-mpnn_amd"))
import __graft_entry__ as g  # noqa: E402

g.load_only()
from rdesign.model.rdesign import RNAModel  # noqa: E402
from rnampnn.utils import synth  # noqa: E402



def _batch():
    lens = [int(v) for v in synth.synth_lengths(64, 100, 500, seed=0)]
    T = max(lens)
    X = np.zeros((64, T, 6, 3), np.float32); mask = np.zeros((64, T), np.float32)
    for i, n in enumerate(lens):
        X[i, :n] = synth.synth_rna(n, i)[:, :6]; mask[i, :n] = 1
    S = np.concatenate([np.pad(synth.synth_labels(n, i), (0, T - n)) for i, n in enumerate(lens)]).reshape(64, T)
    return torch.from_numpy(X).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(S).cuda(), int(mask.sum())


def _train(argv):
    steps = max(int(next((a for a in argv if a.isdigit()), 20)), 1)      # (--out takes a path, not a number)
    from rdesign import _native
    torch.manual_seed(0)
    tp = _train_precision(argv)
    m = RNAModel(precision="f32", train_precision=tp).cuda().train()
    Xd, md, Sd, n_valid = _batch()
    opt = m.configure_optimizers(fused=True)[0][0]

    def timed(fn, n):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def step():
        m.loss_and_grad(Xd, Sd, md)
        opt.step()

    ms_step = timed(step, steps)
    m.eval()
    ms_fwd = timed(lambda: m._run(Xd, md, want=("logits",), n_valid=n_valid), steps)
    B, T = md.shape
    lib = _native.lib()
    flags = _native.TRAIN_BF16_MIXED if tp == "bf16" else _native.TRAIN_F32
    print(json.dumps(dict(metric="rdesign_train_step_nt_per_s", value=n_valid / (ms_step * 1e-3), ms_per_step=ms_step, ms_f32_forward=ms_fwd,
                          step_over_f32_forward=ms_step / ms_fwd, nt=n_valid, steps=steps, precision="f32", train_precision=tp, dropout=m.hparams["dropout"],
                          workspace_bytes=int(lib.rdesign_train_workspace_bytes_ex(m._handle.ptr, B, T, flags)),
                          tape_bytes=int(lib.rdesign_train_tape_bytes_ex(m._handle.ptr, B, T, flags)),
                          config="RNAModel defaults (k=25, 9 layers, dense 256), 64 RNAs x 100..500 nt synthetic; loss_and_grad + FlatAdam.step")))


if "--train" in sys.argv:
    _train(sys.argv[1:])
    sys.exit(0)
prec = sys.argv[1] if len(sys.argv) > 1 else "bf16"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
lens = [int(v) for v in synth.synth_lengths(64, 100, 500, seed=0)]
T = max(lens)
X = np.zeros((64, T, 6, 3), np.float32); mask = np.zeros((64, T), np.float32)
for i, n in enumerate(lens):
    X[i, :n] = synth.synth_rna(n, i)[:, :6]; mask[i, :n] = 1
torch.manual_seed(0)
m = RNAModel(precision=prec).cuda().eval()
Xd, md = torch.from_numpy(X).cuda(), torch.from_numpy(mask).cuda()
n_valid = int(mask.sum())
for _ in range(3):
    m._run(Xd, md, want=("logits",), n_valid=n_valid)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    m._run(Xd, md, want=("logits",), n_valid=n_valid)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
print(json.dumps(dict(metric="rdesign_forward_nt_per_s", value=n_valid / dt, ms_per_step=dt * 1e3, nt=n_valid, precision=prec,
                      config="RNAModel defaults (k=25, 9 layers, dense 256), 64 RNAs x 100..500 nt synthetic")))
