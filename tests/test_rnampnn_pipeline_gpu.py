"""GPU checks of the RNAMPNN pipeline: ``Trainer.validate_metrics`` against the existing ``validation_step`` loop (no host round trip
inside the pass), ``design`` / ``score_sequences``, checkpoint + ``--resume`` (bit-identical continuation), ``train.py --out`` ->
``Final.pt`` -> ``predict.py``.  A small model throughout: 2 ResMPNN layers, k = 6, 16 synthetic RNAs of 20-90 nt."""
import csv
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rna-mpnn_amd")
sys.path.insert(0, PKG)

LENGTHS = [20 + (70 * ((7 * i) % 16)) // 15 for i in range(16)]      # 20 ... 90, not sorted
SMALL = dict(num_res_neighbours=6, num_res_mpnn_layers=2, padding_len=128)
CLI_SMALL = ["--layers", "2", "--neighbours", "6", "--max-len", "128", "--batch-size", "4", "--max-nt", "512"]


def _nll_bound(sum64, n):
    """tests/test_rdesign_trainer_gpu.py: _nll_bound."""
    return 1e-5 * abs(sum64) + 1e-6 * n


def _items(lengths=LENGTHS, seed=1):
    from rnampnn.utils import synth
    return [(synth.synth_rna(int(n), i, seed=seed), synth.synth_labels(int(n), i, seed=seed)) for i, n in enumerate(lengths)]


def _model(precision, seed=0, **kw):
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.rnampnn import RNAMPNN
    torch.manual_seed(seed)
    return RNAMPNN(precision=precision, **dict(SMALL, **kw)).cuda().eval()


def _batch(items, idx):
    from rnampnn.utils.data import pad_batch
    y, c, m, lens = pad_batch([items[i] for i in idx], pin=False)
    return y.cuda(), c.cuda(), m.cuda(), lens


# ------------------------------------------------------------------------------------------------------------------ validate_metrics
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_validate_metrics_equal_the_validation_step_accumulators(precision):
    from rnampnn.utils.data import PaddedLoader, bucket_batches
    from rnampnn.utils.train import Trainer
    items = _items()
    m = _model(precision)
    tr = Trainer(m, None)
    got = tr.validate_metrics(items, LENGTHS, 4, 512)
    micro, macro = tr.validate(items, LENGTHS, 4, 512)
    assert got["weighted_val_recovery_rate"] == micro and got["val_recovery_rate"] == macro
    m.val_step_outputs = {'val_loss': [], 'correct': [], 'len': [], 'recovery_rates': []}
    order = []
    for y, c, mask, lens, _ in PaddedLoader(items, bucket_batches(LENGTHS, 4, 512, seed=0), device="cuda"):
        m.validation_step((F.one_hot(y.long(), 4).float(), c, mask, None))          # the EXISTING per-batch torch / .tolist() path
        order += lens
    acc = m.val_step_outputs
    lv = tr.last_validation
    c, v = lv["correct"].cpu().numpy(), lv["valid"].cpu().numpy()
    assert v.tolist() == order and sorted(order) == sorted(LENGTHS) and lv["loss"].shape == lv["nll"].shape == (16,)
    assert int(c.sum()) == int(sum(acc["correct"])) and int(v.sum()) == int(sum(acc["len"])) == sum(LENGTHS)
    assert [int(round(r * n)) for r, n in zip(acc["recovery_rates"], order)] == c.tolist()     # n <= 90: round(rate * n) recovers the count
    # LossMonitor.on_validation_epoch_end, in float64
    n_tot = float(sum(acc["len"]))
    sum_loss = float(sum(float(t) for t in acc["val_loss"]))
    want = dict(val_loss=sum_loss / n_tot, weighted_val_recovery_rate=float(sum(acc["correct"])) / n_tot,
                val_recovery_rate=float(np.mean(np.array(acc["recovery_rates"], np.float64))))
    print(precision, "validate_metrics", got, "accumulators", want, "bound", _nll_bound(sum_loss, n_tot) / n_tot)
    assert set(got) == {"val_loss", "weighted_val_recovery_rate", "val_recovery_rate"}
    assert got["weighted_val_recovery_rate"] == want["weighted_val_recovery_rate"]
    assert abs(got["val_recovery_rate"] - want["val_recovery_rate"]) <= 2.0 ** -23      # the accumulators hold each rate as an f32 quotient
    assert abs(got["val_loss"] - want["val_loss"]) <= _nll_bound(sum_loss, n_tot) / n_tot
    assert abs(float(lv["loss"].cpu().numpy().astype(np.float64).sum()) / n_tot - got["val_loss"]) < 1e-12
    # the likelihood next to it: mix_loss of a 4-class softmax lies in [log(3 + e) - 1, log(3 + e)], the NLL is unbounded above
    assert 0.7436 * n_tot <= float(lv["loss"].sum()) <= 1.7437 * n_tot and float(lv["nll"].min()) > 0


class _SyncCounter:
    """Counts calls of the ways a host round trip is spelt in this code base (as tests/test_rdesign_trainer_gpu.py does)."""

    def __init__(self, monkeypatch):
        self.n, self.armed = 0, False
        for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "cpu"), (torch.cuda, "synchronize"),
                            (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")):
            monkeypatch.setattr(owner, name, self._wrap(getattr(owner, name)))

    def _wrap(self, fn):
        def counted(*a, **k):
            if self.armed:
                self.n += 1
            return fn(*a, **k)
        return counted

    def window(self, owner, name, calls, monkeypatch):
        """Arm at the start of the first call of ``owner.name`` and disarm at the end of call number ``calls``."""
        fn, state = getattr(owner, name), dict(i=0)

        def wrapped(*a, **k):
            if state["i"] == 0:
                self.armed = True
            out = fn(*a, **k)
            state["i"] += 1
            if state["i"] == calls:
                self.armed = False
            return out
        monkeypatch.setattr(owner, name, wrapped)
        return state


def test_no_host_round_trip_inside_a_validation_pass(monkeypatch):
    from rnampnn.utils.data import bucket_batches
    from rnampnn.utils.train import Trainer
    items = _items()
    m = _model("bf16")
    tr = Trainer(m, None)
    tr.validate_metrics(items, LENGTHS, 4, 512)                           # warm: workspace, allocator
    cnt = _SyncCounter(monkeypatch)
    nb = len(bucket_batches(LENGTHS, 4, 512, seed=0))
    st = cnt.window(m, "score_batch", nb, monkeypatch)
    tr.validate_metrics(items, LENGTHS, 4, 512)
    assert st["i"] == nb >= 4 and not cnt.armed
    assert cnt.n == 0, f"{cnt.n} host round trips between the first and the last batch of validate_metrics"
    # what the counter catches: the per-batch validation_step
    y, c, mask, _ = _batch(items, [0, 1, 2, 3])
    cnt.armed = True
    m.validation_step((F.one_hot(y.long(), 4).float(), c, mask, None))
    cnt.armed = False
    print("host round trips of one validation_step on 4 RNAs:", cnt.n)
    assert cnt.n > 0


def test_score_batch_with_the_tree_read_out():
    from rnampnn.model.rnampnn import letters_padded
    from rnampnn.model.xgb import GBDTReadout
    items = _items()
    m = _model("bf16")
    y, c, mask, lens = _batch(items, [0, 5, 9, 12])
    with pytest.raises(RuntimeError, match="needs a tree read-out"):
        m.score_batch(y, c, mask, use_trees=True)
    emb = m.embedding(c, mask)
    valid = mask == 1
    m.xgb_readout = GBDTReadout.fit(emb[valid], y[valid].long(), n_estimators=3, max_depth=3, seed=1)
    correct, nvalid, loss, nll = m.score_batch(y, c, mask, use_trees=True)
    assert loss is None and nll is None and nvalid.tolist() == lens
    ids = m.xgb_readout.predict(emb)
    assert correct.tolist() == [int(((ids[b] == y[b]) & valid[b]).sum()) for b in range(4)]
    assert m.predict_sequences(c, mask) == letters_padded(m._predict_ids(c, mask))


# ------------------------------------------------------------------------------------------------------------------ design / score_sequences
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_design_scores_its_own_samples_and_the_cold_draw_is_the_argmax(precision):
    from rnampnn.model.rnampnn import argmax_recovery
    items = _items()
    m = _model(precision)
    with torch.no_grad():       # a freshly initialised model is all but uniform (top-2 gaps of 1e-4 and less): spread its logits, so that
        for key in ("readout.readout_layers.3.weight", "readout.readout_layers.3.bias"):      # "temperature 1e-4" below is a cold draw
            m.get_parameter(key).mul_(500.0)
    y, c, mask, lens = _batch(items, [1, 4, 8, 15])
    seqs, nll = m.design(c, mask, n_samples=5, temperature=1.0, seed=3)
    assert seqs.shape == (5, 4, max(lens)) and seqs.dtype == torch.int8 and nll.shape == (5, 4)
    assert torch.equal(seqs, m.sample(c, mask, temperature=1.0, n_samples=5, seed=3))
    nll2, match, valid = m.score_sequences(c, mask, seqs, labels=y)
    assert nll.cpu().numpy().tobytes() == nll2.cpu().numpy().tobytes() and valid.tolist() == lens
    assert match.tolist() == [[int(((seqs[s, b] == y[b]) & (mask[b] == 1)).sum()) for b in range(4)] for s in range(5)]
    nll3, none, _ = m.score_sequences(c, mask, seqs[2])                   # one (B, T) sequence, no labels
    assert none is None and torch.equal(nll3[0], nll[2])
    # against float64 torch on the model's own logits
    x = m(c, mask).double()
    ref = ((torch.logsumexp(x, -1)[None] - torch.gather(x[None].expand(5, -1, -1, -1), 3, seqs.long().clamp(min=0)[..., None])[..., 0])
           * mask.double()[None]).sum(-1)
    for s in range(5):
        for b, n in enumerate(lens):
            assert abs(float(nll[s, b]) - float(ref[s, b])) <= _nll_bound(float(ref[s, b]), n), (s, b)
    # temperature 1e-4: the argmax sequence, whose NLL no other sequence undercuts
    pred, _, _ = argmax_recovery(m(c, mask), mask, None)
    top2 = torch.topk(x, 2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1])[mask == 1].min())
    print(precision, "smallest top-2 gap of the test logits:", gap, "largest |logit|:", float(x.abs().max()))
    assert gap >= 1e-2                                                    # 100 temperatures: a runner-up is drawn with probability e^-100
    cold, cold_nll = m.design(c, mask, n_samples=2, temperature=1e-4, seed=4)
    assert torch.equal(cold, pred[None].expand(2, -1, -1))
    assert torch.equal(cold_nll[0], cold_nll[1]) and bool((cold_nll[0][None] <= nll).all())
    t = m.test_step((F.one_hot(y.long(), 4).float(), c, mask, None))
    out = m.test_step_outputs
    assert set(out) == {"test_loss", "correct", "len", "recovery_rates"} and out["len"] == [sum(lens)] and len(out["recovery_rates"]) == 4
    correct, _, loss, _ = m.score_batch(y, c, mask)
    assert out["correct"] == [int(correct.sum())] and float(out["test_loss"][0]) == float(loss.sum()) and t["recovery_rates"] == out["recovery_rates"]


# ------------------------------------------------------------------------------------------------------------------ train.py --out / --resume
def _train(argv):
    import train as T
    torch.manual_seed(0)                                                  # the initial weights come from torch's generator
    return T.run(T.parse(["--synthetic", "16", "--seed", "2"] + CLI_SMALL + argv), log=lambda *a: None)


def test_resume_continues_the_same_trajectory_bit_for_bit(tmp_path):
    a, b = str(tmp_path / "straight"), str(tmp_path / "resumed")
    common = ["--train-precision", "f32"]
    _train(common + ["--epochs", "2", "--out", a])
    first = _train(common + ["--epochs", "1", "--out", b])
    assert len(first["epochs"]) == 1
    second = _train(common + ["--epochs", "2", "--out", b, "--resume", os.path.join(b, "last.pt")])
    assert len(second["epochs"]) == 1                                     # the epoch counter went on at 1
    ca = torch.load(os.path.join(a, "last.pt"), map_location="cpu", weights_only=True)
    cb = torch.load(os.path.join(b, "last.pt"), map_location="cpu", weights_only=True)
    assert ca["epoch"] == cb["epoch"] == 1 and ca["init_kwargs"] == cb["init_kwargs"] and ca["init_kwargs"]["train_precision"] == "f32"
    assert list(ca["state_dict"]) == list(cb["state_dict"])
    for k in ca["state_dict"]:
        assert torch.equal(ca["state_dict"][k], cb["state_dict"][k]), k
    fa, fb = ca["optimizer"]["flat_adam"], cb["optimizer"]["flat_adam"]
    assert fa["t"] == fb["t"] > 0 and float(fa["exp_avg"].abs().sum()) > 0
    assert torch.equal(fa["exp_avg"], fb["exp_avg"]) and torch.equal(fa["exp_avg_sq"], fb["exp_avg_sq"])
    assert ca["optimizer"]["param_groups"] == cb["optimizer"]["param_groups"] and ca["scheduler"] == cb["scheduler"]
    assert ca["scheduler"]["last_epoch"] == 2


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """``train.py --synthetic 16 --epochs 3 --out DIR`` (small model), run once."""
    out = str(tmp_path_factory.mktemp("run"))
    return out, _train(["--epochs", "3", "--out", out])


def test_final_pt_holds_the_best_epoch(trained):
    from rnampnn.utils.train import load_checkpoint
    out, res = trained
    recs = res["epochs"]
    assert len(recs) == 3 and sorted(os.listdir(out)) == ["Final.pt", "last.pt"]
    for r in recs:
        assert {"val_loss", "weighted_val_recovery_rate", "val_recovery_rate", "val_micro", "val_macro", "train_loss"} <= set(r)
        assert r["val_micro"] == r["weighted_val_recovery_rate"] and r["val_macro"] == r["val_recovery_rate"] and np.isfinite(r["val_loss"])
    model, ck = load_checkpoint(os.path.join(out, "Final.pt"))
    rates = [r["val_recovery_rate"] for r in recs]
    print("val_recovery_rate per epoch", rates, "stored", ck["val_recovery_rate"], "epoch", ck["epoch"])
    assert ck["val_recovery_rate"] == max(rates) and ck["epoch"] == rates.index(max(rates)) == res["best_epoch"]
    assert "optimizer" not in ck and ck["model"] == "rnampnn"
    last = torch.load(os.path.join(out, "last.pt"), map_location="cpu", weights_only=True)
    assert last["epoch"] == 2 and "optimizer" in last and "scheduler" in last and last["best_epoch"] == ck["epoch"]


def test_predict_cli_on_a_written_directory(trained, tmp_path):
    import predict as P
    from rnampnn.utils import synth
    from rnampnn.utils.data import bucket_batches, fill_nan_deterministic, pad_batch
    from rnampnn.utils.train import load_checkpoint
    out, _ = trained
    data = tmp_path / "data"
    os.makedirs(data / "coords"); os.makedirs(data / "seqs")
    ids, lens = ["r3", "r0", "r4", "r1", "r2"], [33, 20, 57, 41, 26]
    for i, (rid, n) in enumerate(zip(ids, lens)):
        c = synth.synth_rna(n, 40 + i, seed=3)
        if rid == "r4":
            c[5, 1] = np.nan                                              # a missing atom
        np.save(data / "coords" / f"{rid}.npy", c)
        if rid != "r1":                                                   # r1 has no fasta
            (data / "seqs" / f"{rid}.fasta").write_text(f">{rid}\n" + "".join("AUCG"[v] for v in synth.synth_labels(n, 40 + i, seed=3)) + "\n")
    sub, des = str(tmp_path / "submit.csv"), str(tmp_path / "designs.csv")
    rows = P.run(P.parse(["--ckpt", os.path.join(out, "Final.pt"), "--data", str(data), "--out", sub, "--samples", "2", "--designs-out", des,
                          "--batch-size", "2"]), log=lambda *a: None)
    got = list(csv.reader(open(sub)))
    assert got[0] == ["pdb_id", "seq"] and [r[0] for r in got[1:]] == sorted(ids) and [tuple(r) for r in got[1:]] == rows
    # the same batches through predict_sequences (padded forward) on the reloaded model
    model, _ = load_checkpoint(os.path.join(out, "Final.pt"), device="cuda")
    model.eval()
    order = sorted(range(5), key=lambda i: ids[i])
    coords = []
    for i in order:
        c = np.load(data / "coords" / f"{ids[i]}.npy")
        coords.append(fill_nan_deterministic(c, ids[i]) if np.isnan(c).any() else c.astype(np.float32))
    want = {}
    for b in bucket_batches([lens[i] for i in order], 2, 32768, seed=0):
        _, c, m, _ = pad_batch([(coords[j], np.zeros(coords[j].shape[0], np.int64)) for j in b], pin=False)
        for j, s in zip(b, model.predict_sequences(c, m)):
            want[ids[order[j]]] = s
    assert {r[0]: r[1] for r in got[1:]} == want and all(len(want[rid]) == n for rid, n in zip(ids, lens))
    d = list(csv.reader(open(des)))
    assert d[0] == ["pdb_id", "sample", "seq", "nll_per_nt", "recovery"] and len(d) == 1 + 2 * 5
    assert [(r[0], r[1]) for r in d[1:]] == [(rid, str(s)) for rid in sorted(ids) for s in range(2)]
    for r in d[1:]:
        n = lens[ids.index(r[0])]
        assert len(r[2]) == n and set(r[2]) <= set("AUCG") and float(r[3]) > 0
        assert (r[4] == "") == (r[0] == "r1") and (r[4] == "" or 0.0 <= float(r[4]) <= 1.0)
