"""CPU test of bench.py's own N > 1 launcher: ``--gpus 2`` without RANK spawns two ranks (torch.distributed.run
children, gloo), which shard the config-4 workload, reduce time (MAX) and units (SUM) and all-reduce the flat gradient
buffer of the training leg.  ``--dry-run`` launches no kernel (there is no GPU here); what is checked is the plumbing the
driver relies on: n_gpus, the workload named in config, the JSON contract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


def _run(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env, cwd=REPO,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_spawns_its_own_ranks_and_reports_n_gpus():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run", "--batch", "64", "--no-build", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["parallelism"] == "dp2" and out["config"]["workload"].startswith("C4: 64 RNAs x 200 nt")
    assert out["config"]["nucleotides_per_step_per_gpu"] == 32 * 200          # whole RNAs, balanced
    assert out["scaling"] == "strong" and out["unit"] == "nucleotides/s" and out["higher_is_better"] is True
    assert out["vs_baseline"] is None and "cpu_baseline" not in out
    assert out["train"]["allreduce_bytes"] == 3536900 * 4 and out["train"]["steps"] == 5
    assert "allreduce_exposed_ms" in out["train"] and sum(out["train"]["allreduce_chunks_floats"]) == 3536900
    # the weak-scaling leg: the N = 1 workload (C2, 256 RNAs) on every rank, comparable with the N = 1 line
    w = out["weak_c2"]
    assert w["scaling"] == "weak" and w["workload"].startswith("C2: batch=256 RNAs") and w["steps"] == 2
    assert w["nucleotides_per_step_all_ranks"] > 2 * 256 * 100 and w["value"] > 0 and w["unit"] == "nucleotides/s"
    for key in ("metric", "value", "ms_per_step", "dtype", "data", "roofline"):
        assert key in out


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    r = _run(["--gpus", "2", "--dry-run", "--no-build"], env_extra={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_bench_plain_run_reports_the_headline_only():
    """Without --full a run times the forward and reports it: no training, weak-scaling, roofline or recovery leg."""
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "0", "--dry-run", "--batch", "64", "--no-build"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 0 and out["ms_per_step"] > 0
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    for key in ("train", "weak_c2", "roofline", "mfma", "recovery", "cpu_baseline", "train_epoch"):
        assert key not in out


def test_bench_refuses_zero_steps():
    r = _run(["--gpus", "1", "--steps", "0", "--dry-run", "--no-build"])
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_keeps_to_its_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    """A dump larger than the budget becomes the same seeded sample of RNAs on every run, with its row numbers beside it."""
    import bench
    outs = [torch.arange(6 * 5 * 4, dtype=torch.float32).reshape(6, 5, 4) + 1000 * i for i in range(2)]   # two micro-batches
    bench.dump_outputs(outs, str(tmp_path / "whole"), 0, 1)
    whole = np.load(tmp_path / "whole" / "logits.npy")
    assert whole.dtype == np.float32 and whole.shape == (12, 5, 4)
    assert np.array_equal(whole, torch.cat(outs).numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * 5 * 4 * 4)
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d), 0, 1)
    a, rows = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "a" / "logits_rows.npy")
    assert a.shape == (3, 5, 4) and a.nbytes <= bench.DUMP_MAX_BYTES and rows.dtype == np.float64
    assert np.array_equal(a, whole[rows.astype(np.int64)])
    assert np.array_equal(a, np.load(tmp_path / "b" / "logits.npy"))


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_logits_of_its_last_step(tmp_path):
    """--dump-outputs on the default N = 1 workload: the float32 logits of the 256 C2 RNAs, zero on padded rows, the same on a second run."""
    dumps = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and "roofline" not in out and "cpu_baseline" not in out
        dumps.append(np.load(tmp_path / d / "logits.npy"))
    lg = dumps[0]
    assert lg.dtype == np.float32 and lg.shape == (256, out["config"]["max_len"], 4) and np.isfinite(lg).all()
    sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
    from rnampnn.utils import synth
    lens = synth.synth_lengths(256, 100, 140, seed=0, first_index=0)
    assert all(not lg[i, n:].any() and lg[i, :n].any() for i, n in enumerate(lens))
    assert np.array_equal(dumps[0], dumps[1])
