"""Host side of the RNAMPNN pipeline (``rnampnn_score``'s ABI entry, rnampnn/utils/train.py checkpoints, train.py / predict.py flags,
the checkpoint family dispatch): no GPU needed."""
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))

SMALL = dict(num_res_neighbours=6, num_res_mpnn_layers=2, padding_len=128, dropout=0.25, n_estimators=5, xgb_max_depth=3)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    return _native


def test_header_declares_and_library_exports_rnampnn_score(native):
    text = open(os.path.join(REPO, "include", "rnampnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+rnampnn_score\s*\(([^;]*)\)\s*;", text)
    assert m, "include/rnampnn_hip.h does not declare rnampnn_score"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert "rnampnn_score" in native.SYMBOLS and len(native.SYMBOLS["rnampnn_score"][1]) == n_params == 17
    assert hasattr(native.lib(), "rnampnn_score")
    import __graft_entry__ as g
    assert "score.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "score.hip"))


def test_score_refuses_host_logits(native):
    from rnampnn.model.rnampnn import score_logits
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        score_logits(torch.zeros(1, 4, 4), mask=torch.ones(1, 4))


def test_checkpoint_round_trips_bit_for_bit_with_weights_only(native, tmp_path):
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils.train import load_checkpoint, save_checkpoint
    torch.manual_seed(3)
    m = RNAMPNN(precision="f32", train_precision="bf16", **SMALL)
    m.name, m.version = "RNAMPNN-T", 7
    (opt,), (sched,) = m.configure_optimizers()                      # torch.optim.Adam + StepLR on a CPU-constructed model
    for step in range(2):
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    sched.step()
    path = str(tmp_path / "last.pt")
    save_checkpoint(path, m, opt, sched, epoch=4, val_recovery_rate=0.5)
    raw = torch.load(path, map_location="cpu", weights_only=True)    # tensors and plain types only
    assert raw["model"] == "rnampnn" and raw["name"] == "RNAMPNN-T" and raw["version"] == 7 and raw["epoch"] == 4
    assert raw["val_recovery_rate"] == 0.5
    m2, ck = load_checkpoint(path)
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) and all(sd[k].shape == sd2[k].shape and torch.equal(sd[k], sd2[k]) for k in sd)
    kw = m.init_kwargs
    assert m2.init_kwargs == kw and kw["precision"] == "f32" and kw["train_precision"] == "bf16"
    assert all(kw[k] == v for k, v in SMALL.items()) and all(type(v) in (int, float, str, bool) for v in kw.values())
    assert (m2.name, m2.version, m2.train_precision) == ("RNAMPNN-T", 7, "bf16")
    (opt2,), (sched2,) = m2.configure_optimizers()
    opt2.load_state_dict(ck["optimizer"])
    sched2.load_state_dict(ck["scheduler"])
    a, b = opt.state_dict(), opt2.state_dict()
    assert a["param_groups"] == b["param_groups"] and list(a["state"]) == list(b["state"]) and len(a["state"]) == len(list(m.parameters()))
    for i in a["state"]:
        assert set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in a["state"][i]:
            assert torch.equal(torch.as_tensor(a["state"][i][k]), torch.as_tensor(b["state"][i][k])), (i, k)
    assert sched.state_dict() == sched2.state_dict() and sched2.last_epoch == 1
    # a clash with the checkpoint's own keys, or an object in the extras, is refused at save time
    with pytest.raises(ValueError):
        save_checkpoint(path, m, state_dict=1)
    with pytest.raises(TypeError):
        save_checkpoint(path, m, when=object())


class _Payload:
    pass


def test_a_file_with_a_pickled_object_is_refused(native, tmp_path):
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils.train import load_checkpoint, save_checkpoint
    m = RNAMPNN(precision="f32", **SMALL)
    good = str(tmp_path / "good.pt")
    save_checkpoint(good, m)
    ck = torch.load(good, map_location="cpu", weights_only=True)
    ck["hook"] = _Payload()
    bad = str(tmp_path / "bad.pt")
    torch.save(ck, bad)
    with pytest.raises(pickle.UnpicklingError):
        load_checkpoint(bad)
    # ... and so is a file of another family
    del ck["hook"], ck["model"]
    other = str(tmp_path / "other.pt")
    torch.save(ck, other)
    with pytest.raises(ValueError, match="not an RNAMPNN checkpoint"):
        load_checkpoint(other)


def test_command_lines_parse_the_new_flags(tmp_path):
    import predict
    import train
    a = train.parse([])
    assert a.model == "rnampnn" and a.out is None and a.resume is None
    d = str(tmp_path / "run")
    a = train.parse(["--out", d, "--resume", os.path.join(d, "last.pt"), "--fit-xgb"])
    assert a.model == "rnampnn" and a.out == d and a.resume == os.path.join(d, "last.pt") and a.fit_xgb
    p = predict.parse(["--ckpt", "x.pt", "--data", "d"])
    assert (p.samples, p.temperature, p.seed, p.designs_out) == (0, 0.1, 0, None)
    p = predict.parse(["--ckpt", "x.pt", "--data", "d", "--samples", "4", "--temperature", "0.5", "--seed", "9", "--designs-out", "z.csv"])
    assert (p.samples, p.temperature, p.seed, p.designs_out) == (4, 0.5, 9, "z.csv")
    with pytest.raises(ValueError, match="--resume"):
        train.run(train.parse(["--model", "rdesign", "--resume", "x.pt"]))


def test_checkpoint_family_dispatch(native, tmp_path):
    import predict
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils.train import save_checkpoint
    from rdesign.model.rdesign import RNAModel
    from rdesign.utils.train import save_checkpoint as save_rdesign
    mine = str(tmp_path / "rnampnn.pt")
    save_checkpoint(mine, RNAMPNN(precision="f32", **SMALL))
    assert predict.checkpoint_family(mine) == "rnampnn"
    theirs = str(tmp_path / "rdesign.pt")                            # today's rdesign files carry no 'model' key
    save_rdesign(theirs, RNAModel(num_mpnn_layers=1))
    assert "model" not in torch.load(theirs, map_location="cpu", weights_only=True)
    assert predict.checkpoint_family(theirs) == "rdesign"
    odd = str(tmp_path / "odd.pt")
    torch.save(dict(model="other"), odd)
    with pytest.raises(ValueError, match="unknown model family"):
        predict.checkpoint_family(odd)


def test_validation_metrics_are_loss_monitors_formulas():
    from rnampnn.utils.train import validation_metrics
    rng = np.random.RandomState(5)
    valid = rng.randint(1, 400, 29)
    correct = (valid * rng.rand(29)).astype(np.int64)
    loss = (valid * (0.8 + rng.rand(29))).astype(np.float32)
    got = validation_metrics(torch.from_numpy(correct).to(torch.int32), torch.from_numpy(valid).to(torch.int32), torch.from_numpy(loss))
    # LossMonitor.on_validation_epoch_end in float64: sum(loss * n) / sum(n), sum(correct) / sum(n), mean of the per-RNA rates
    want = dict(val_loss=loss.astype(np.float64).sum() / valid.sum(), weighted_val_recovery_rate=correct.sum() / valid.sum(),
                val_recovery_rate=np.mean(correct.astype(np.float64) / valid))
    assert set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k


def test_load_structures_keeps_every_structure(tmp_path):
    from rnampnn.utils import synth
    from rnampnn.utils.data import fill_nan_deterministic
    from rnampnn.utils.predict import load_structures
    os.makedirs(tmp_path / "coords"); os.makedirs(tmp_path / "seqs")
    want = {}
    for i, (rid, n) in enumerate([("b2", 21), ("a1", 30), ("c3", 25)]):
        c = synth.synth_rna(n, i, seed=2)
        if rid == "c3":
            c[4, 2] = np.nan
        np.save(tmp_path / "coords" / f"{rid}.npy", c)
        want[rid] = c
        if rid != "a1":
            (tmp_path / "seqs" / f"{rid}.fasta").write_text(">" + rid + "\n" + "".join("AUCG"[v] for v in synth.synth_labels(n, i, seed=2)) + "\n")
    np.save(tmp_path / "coords" / "bad.npy", np.zeros((3, 6, 3), np.float32))        # another atom count: no row
    items = load_structures(str(tmp_path))
    assert [r for r, _, _ in items] == ["a1", "b2", "c3"]
    assert items[0][2] is None and items[1][2].tolist() == synth.synth_labels(21, 0, seed=2).tolist()
    assert np.array_equal(items[1][1], want["b2"].astype(np.float32))
    assert not np.isnan(items[2][1]).any() and np.array_equal(items[2][1], fill_nan_deterministic(want["c3"], "c3"))
