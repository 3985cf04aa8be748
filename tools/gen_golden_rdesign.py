#!/usr/bin/env python3
"""Generate tests/golden/rdesign_*.npz from the REFERENCE's own `rdesign` modules (sibling of tools/gen_golden.py).

Runs only in the build container (needs the reference checkout; never on the GPU box, never from a test).  It imports
`rdesign.model.{feature,mpnn,functional}` and `rdesign.utils.data.featurize` from the reference and composes `RNAFeatures`,
`ModuleList[MPNNLayer]` and `Readout` as `rdesign/model/rdesign.py:53-65,82-88,100-102` does, with the default feature-type lists.
The LightningModule itself adds no arithmetic and needs xgboost, which is absent.

`rdesign/utils/data.py` imports BioPython, pytorch_lightning and seaborn at the top; none is touched by the arithmetic.  Each
import is tried for real first; only a name that fails gets an inert placeholder module, the names are printed, and after
every forward / backward the generator asserts that no placeholder object was called or instantiated.

`.eval()` throughout: dropout masks cannot be matched to torch's RNG.  `seeding()` of the reference is not called.
The fixtures store seeds and hyper-parameters, not weights: tests/_rdesign_cases.py regenerates them (asserted bit-identical here).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rdesign.py [--check]

`--check` regenerates into memory and compares every array with the committed fixture instead of writing.
"""
from __future__ import annotations

import importlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RDESIGN_REFERENCE", "/root/reference")
MAX_FIXTURE_BYTES = 1_000_000
MAX_SET_BYTES = 4_000_000

# ----------------------------------------------------------------------------- placeholders for the absent imports
STUB_USES = []                       # (module, attribute) of every placeholder object that was called or instantiated


class _StubModule(types.ModuleType):
    """Inert stand-in for an absent package: any public attribute is a dummy class (usable as a base class or, called with one
    function, as a decorator); dunder lookups raise AttributeError, so the import machinery sees an ordinary, path-less module."""

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        mod = self.__name__

        class Dummy:
            def __init__(self, *a, **k):
                STUB_USES.append((mod, name))

            def __call__(self, *a, **k):
                STUB_USES.append((mod, name))
                return a[0] if len(a) == 1 and callable(a[0]) else None

        Dummy.__name__ = Dummy.__qualname__ = name
        setattr(self, name, Dummy)
        return Dummy


def import_reference():
    """-> (RNAFeatures, MPNNLayer, Readout, featurize, stubbed names).  Real imports first; placeholders only for what fails."""
    sys.path.insert(0, REF)
    stubbed = []
    while True:
        try:
            feature = importlib.import_module("rdesign.model.feature")
            mpnn = importlib.import_module("rdesign.model.mpnn")
            functional = importlib.import_module("rdesign.model.functional")
            data = importlib.import_module("rdesign.utils.data")
            break
        except ModuleNotFoundError as exc:
            top = exc.name.split(".")[0]
            if top in stubbed or top in ("rdesign", "torch", "numpy"):
                raise
            stubbed.append(top)
            sys.modules[top] = _StubModule(top)
            for k in [k for k in sys.modules if k == "rdesign" or k.startswith("rdesign.")]:
                del sys.modules[k]                  # a half-imported reference module is imported afresh
    assert os.path.realpath(feature.__file__).startswith(os.path.realpath(REF)), feature.__file__
    del STUB_USES[:]                                # import-time uses (base classes, decorators) are not uses by the arithmetic
    # from here on `rnampnn` / `oracle` mean this repository's packages (the reference has an `rnampnn` of its own)
    sys.path.remove(REF)
    for k in [k for k in sys.modules if k == "rnampnn" or k.startswith("rnampnn.")]:
        del sys.modules[k]
    sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "rna-mpnn_amd"), REPO]
    return feature.RNAFeatures, mpnn.MPNNLayer, functional.Readout, data.featurize, stubbed


RNAFeatures, MPNNLayer, Readout, featurize, STUBBED = import_reference()
import _rdesign_cases as T                      # noqa: E402  (the test-side rules: _batch, _weights, _labels, golden_weights)
from oracle import rdesign_oracle as O          # noqa: E402
from rnampnn.utils import synth                 # noqa: E402


class RefComposite(torch.nn.Module):
    """The three reference modules wired as `RNAModel.__init__` / `forward` / `training_step` wire them."""

    def __init__(self, cfg: O.RDesignConfig):
        super().__init__()
        H = cfg.hidden_dim
        self.features = RNAFeatures(H, H, top_k=cfg.k_neighbors, dropout=0.1, node_feat_types=["angle", "distance", "direction"],
                                    edge_feat_types=["orientation", "distance", "direction"])
        self.mpnn_layers = torch.nn.ModuleList([
            MPNNLayer(H, H * 2, cfg.num_message_layers, cfg.num_dense_layers, cfg.dim_dense_layers, dropout=0.1)
            for _ in range(cfg.num_mpnn_layers)])
        self.readout = Readout(H, cfg.readout_hidden_dim, cfg.num_readout_layers, dropout=0.1)
        self.loss_fn = torch.nn.CrossEntropyLoss()

    def run(self, X, S, mask):
        taps = {}
        hooks = [self.features.node_embedding.register_forward_pre_hook(lambda m, a: taps.__setitem__("node_raw", a[0].detach().clone())),
                 self.features.edge_embedding.register_forward_pre_hook(lambda m, a: taps.__setitem__("edge_raw", a[0].detach().clone()))]
        _, S_p, h_V, h_E, E_idx, _ = self.features(X, S, mask)
        taps.update(E_idx=E_idx, h_V0=h_V.detach().clone())
        for l, layer in enumerate(self.mpnn_layers):
            h_EV = torch.cat([h_E, h_V[E_idx[0]], h_V[E_idx[1]]], dim=-1)
            h_V = layer(h_V, h_EV, E_idx)
            if l == 0:
                taps["h_V1"] = h_V.detach().clone()
        logits = self.readout(h_V)
        taps.update(h_V=h_V.detach(), logits=logits.detach(), loss=self.loss_fn(logits, S_p))
        for h in hooks:
            h.remove()
        return taps


def build(meta, dtype, leg=1):
    cfg, sd = T.golden_weights(meta, leg)
    model = RefComposite(cfg).eval()
    assert list(model.state_dict()) == list(O.state_dict_shapes(cfg)), "state_dict keys / order differ from the oracle's table"
    model.load_state_dict(sd)
    _, again = T.golden_weights(meta, leg)                               # the test-side rule regenerates the same bits
    for k, v in model.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v, again[k]), k
    return model.to(dtype), cfg


F64_ROW_STRIDE = 4                   # float64 h_V taps: rows ::4 (logits_f64 in full)
S2_ROW_STRIDE = 4                    # second-seed leg: logits in full, h_V rows ::4
S2_GRAD_STRIDE = 128                 # second-seed leg: 1-D gradients in full, matrix rows ::128 (+ norms and the projection)


def grad_arrays(model64, cfg, loss, grad_stride, probe_seed, prefix=""):
    keys = [k for k, _ in model64.named_parameters()]
    assert keys == list(O.state_dict_shapes(cfg))
    grads = torch.autograd.grad(loss, [p for _, p in model64.named_parameters()])
    assert not STUB_USES, f"a placeholder import was used by the backward: {STUB_USES}"
    out = {prefix + "loss_f64": np.float64(loss.detach())}
    for k, g in zip(keys, grads):
        out[prefix + "grad." + k] = g.numpy() if (g.dim() == 1 or grad_stride is None) else g.numpy()[::grad_stride]
    flat = torch.cat([g.reshape(-1) for g in grads])
    out.update({prefix + "grad_norm": np.array([float(g.norm()) for g in grads]), prefix + "grad_flat_norm": np.float64(flat.norm()),
                prefix + "grad_probe_dot": np.float64(flat @ T.probe_vector(probe_seed, flat.numel()))})
    return out


def run_legs(meta, X, S, mask, want_grad, leg=1):
    """-> (f32 taps, f64 taps, f64 model) of the reference at the weights `meta` names for `leg`."""
    with torch.no_grad():
        model, cfg = build(meta, torch.float32, leg)
        t32 = model.run(X, S, mask)
    model64, _ = build(meta, torch.float64, leg)
    with torch.set_grad_enabled(want_grad):
        t64 = model64.run(X.double(), S, mask.double())
    assert not STUB_USES, f"a placeholder import was used by the arithmetic: {STUB_USES}"
    assert torch.equal(t32["E_idx"], t64["E_idx"]), "f32 and f64 runs of the reference disagree on the graph"
    return t32, t64, model64, cfg


def scale_for_std(meta, leg, X, S, mask, min_std):
    """The read-out scale of the separated-logit case, from the reference alone: the smallest multiple of 0.1 that lifts the std of its
    f32 logits at this leg's weights to `min_std`."""
    tag = "" if leg == 1 else "2"
    with torch.no_grad():
        std = float(build({**meta, "readout_scale" + tag: 1.0}, torch.float32, leg)[0].run(X, S, mask)["logits"].std())
    return float(np.ceil(10.0 * min_std / std) / 10.0)


def run_case(name, cfg_kw, X, mask, *, weight_seed=0, full=True, e_nodes=4, row_stride=1,
             label_seed=None, grad_stride=None, min_logit_std=None):
    """f32 run = the golden, f64 run = the noise-floor reference (+ loss and autograd gradients when `label_seed` is given); then the
    same inputs at a second weight seed, stored compactly under `s2.` (no fixture should pass by accident of one weight draw)."""
    cfg_all = {**O.RDesignConfig().__dict__, **cfg_kw}
    del cfg_all["scale"]                     # MPNNLayer's own default (mpnn.py:6), not a hyper-parameter: the fixture must not supply it
    meta = dict(cfg=cfg_all, weight_seed=weight_seed, readout_scale=1.0, readout_scale2=1.0, stubbed=STUBBED, e_nodes=e_nodes,
                row_stride=row_stride, f64_row_stride=F64_ROW_STRIDE, weight_seed2=weight_seed + 1, s2_row_stride=S2_ROW_STRIDE)
    X = X.float().contiguous()
    mask = mask.float().contiguous()
    S = T._labels(mask, label_seed) if label_seed is not None else torch.zeros(mask.shape, dtype=torch.long)
    res = dict(X=X.numpy(), mask=mask.numpy())
    if min_logit_std is not None:
        meta["readout_scale"] = scale_for_std(meta, 1, X, S, mask, min_logit_std)
        meta["readout_scale2"] = scale_for_std(meta, 2, X, S, mask, min_logit_std)
    t32, t64, model64, cfg = run_legs(meta, X, S, mask, label_seed is not None)
    E_idx = t32["E_idx"]
    n_edge_rows = int((E_idx[0] < e_nodes).sum())                      # dst ascending: the edges of the first e_nodes packed nodes lead
    assert bool((E_idx[0, :n_edge_rows] < e_nodes).all())
    res.update(E_idx=E_idx.numpy().astype(np.int32), node_raw=t32["node_raw"].numpy()[::row_stride],
               edge_raw=t32["edge_raw"].numpy()[:n_edge_rows], h_V=t32["h_V"].numpy(), logits=t32["logits"].numpy(),
               h_V_f64=t64["h_V"].numpy()[::F64_ROW_STRIDE], logits_f64=t64["logits"].numpy())
    if full:
        res.update(h_V0=t32["h_V0"].numpy()[::row_stride], h_V1=t32["h_V1"].numpy()[::row_stride],
                   h_V0_f64=t64["h_V0"].numpy()[::F64_ROW_STRIDE])
    lg = t32["logits"]                                                 # the golden the device is compared with
    top2 = lg.topk(2, dim=-1).values
    meta["logit_std"] = float(lg.std())
    meta["excluded_share"] = float(((top2[:, 0] - top2[:, 1]) <= 0.1).double().mean())
    if min_logit_std is not None:
        assert meta["logit_std"] >= min_logit_std, f"{name}: reference logit std {meta['logit_std']:.3f} < {min_logit_std}"
        assert meta["excluded_share"] <= 0.10, f"{name}: {meta['excluded_share']:.3f} of rows have a top-2 margin <= 0.1"
    if label_seed is not None:
        meta.update(label_seed=label_seed, grad_stride=grad_stride, s2_grad_stride=S2_GRAD_STRIDE)
        probe_seed = 1000 + label_seed
        res.update(S=S.numpy(), grad_probe_seed=np.int64(probe_seed))
        res.update(grad_arrays(model64, cfg, t64["loss"], grad_stride, probe_seed))
    # second weight seed
    u32, u64, model64b, _ = run_legs(meta, X, S, mask, label_seed is not None, leg=2)
    assert torch.equal(u32["E_idx"], E_idx)
    top2 = u32["logits"].topk(2, dim=-1).values
    meta["logit_std2"] = float(u32["logits"].std())
    meta["excluded_share2"] = float(((top2[:, 0] - top2[:, 1]) <= 0.1).double().mean())
    if min_logit_std is not None:
        assert meta["logit_std2"] >= min_logit_std and meta["excluded_share2"] <= 0.10, (meta["logit_std2"], meta["excluded_share2"])
    res.update({"s2.h_V": u32["h_V"].numpy()[::S2_ROW_STRIDE], "s2.logits": u32["logits"].numpy(),
                "s2.logits_f64": u64["logits"].numpy()})
    if label_seed is not None:
        res.update(grad_arrays(model64b, cfg, u64["loss"], S2_GRAD_STRIDE, probe_seed, prefix="s2."))
    res["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    d_h = float((t32["h_V"].double() - t64["h_V"]).abs().max())
    d_l = float((t32["logits"].double() - t64["logits"]).abs().max())
    print(f"{name}: stubbed={STUBBED} B,T={tuple(mask.shape)} N={int(mask.sum())} E={E_idx.shape[1]} k={cfg.k_neighbors} "
          f"|f32-f64| h_V {d_h:.2e} logits {d_l:.2e} read-out scale {meta['readout_scale']}/{meta['readout_scale2']} logit std "
          f"{meta['logit_std']:.3f}/{meta['logit_std2']:.3f} margin<=0.1 share {meta['excluded_share']:.3f}/{meta['excluded_share2']:.3f}"
          + (f" loss {float(res['loss_f64']):.6f} |grad| {float(res['grad_flat_norm']):.4e}" if label_seed is not None else ""))
    return res


def emit(name, res, check):
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    if check:
        old = np.load(path)
        assert sorted(old.files) == sorted(res), f"{name}: keys differ"
        for k in res:
            a, b = np.asarray(res[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name}: array {k} is not byte-identical"
        size = os.path.getsize(path)
        print(f"  {name}: {len(res)} arrays byte-identical to the committed fixture ({size / 1024:.0f} KB)")
    else:
        buf = io.BytesIO()
        np.savez_compressed(buf, **res)
        size = buf.getbuffer().nbytes
        assert size <= MAX_FIXTURE_BYTES, f"{name}: {size} bytes > {MAX_FIXTURE_BYTES}"
        with open(path, "wb") as f:
            f.write(buf.getvalue())
        print(f"  -> {path[len(REPO) + 1:]} {size / 1024:.0f} KB")
    return size


def real_rna(pdb_id):
    """One record of the reference's dataset in the form `RNADataset.__getitem__` hands to `featurize` (rdesign/utils/data.py:64-82)."""
    coords = np.load(os.path.join(REF, "data", "coords", pdb_id + ".npy"))
    seq = "".join(l.strip() for l in open(os.path.join(REF, "data", "seqs", pdb_id + ".fasta")) if not l.startswith(">"))
    assert len(seq) == coords.shape[0]
    atoms = ["P", "O5'", "C5'", "C4'", "C3'", "O3'"]
    return {"name": pdb_id, "seq": seq, "coords": {a: coords[:, i, :] for i, a in enumerate(atoms)}}


def main():
    check = "--check" in sys.argv
    torch.manual_seed(0)
    torch.set_num_threads(8)
    total = 0

    def case(name, *a, **k):
        nonlocal total
        total += emit(name, run_case(name, *a, **k), check)

    # the three CASES of tests/test_rdesign_gpu.py
    short_k6 = dict(k_neighbors=6, num_mpnn_layers=2)
    readout2 = dict(k_neighbors=30, num_mpnn_layers=3, dim_dense_layers=512, num_readout_layers=2, readout_hidden_dim=128,
                    num_message_layers=2, num_dense_layers=1)
    case("rdesign_short_k6", short_k6, *T._batch([12, 4, 9], seed=5))
    case("rdesign_defaults", dict(), *T._batch([40, 33, 25, 7], seed=5), label_seed=3, grad_stride=128)    # + gradients, see below
    case("rdesign_readout2", readout2, *T._batch([64, 1, 31], seed=5), full=False)
    # T < k: the tensor itself is shorter than k, K' = min(top_k, N) = 4
    case("rdesign_T_lt_k", dict(k_neighbors=6, num_mpnn_layers=2), *T._batch([4, 3], seed=5))
    # n = k, k + 1, k - 1 in one batch
    case("rdesign_n_eq_k25", dict(num_mpnn_layers=3), *T._batch([26, 25, 24], seed=5), full=False)
    # the real 66-nt RNA 1B23_1_R (input of the committed fixture c1_1b23_k16_P66), alone and padded into a batch
    real = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "c1_1b23_k16_P66.npz"))["coords"][:, :, :6].astype(np.float32))
    n = real.shape[1]
    case("rdesign_1b23", dict(), real, torch.ones(1, n))
    X = torch.zeros(2, n, 6, 3)
    m = torch.zeros(2, n)
    X[0], m[0] = real[0], 1
    X[1, :40], m[1, :40] = torch.from_numpy(synth.synth_rna(40, 1, seed=11)[:, :6]), 1
    case("rdesign_1b23_batch", dict(), X, m, full=False)
    # real RNAs whose first residue lacks its P (NaN in the data set), through the reference's own featurize
    Xn, _, mn, lengths, names = featurize([real_rna("1A9N_1_Q"), real_rna("1AQ3_1_S")])
    assert not STUB_USES and Xn.dtype == torch.float32 and lengths.tolist() == [24, 12]
    case("rdesign_nan_featurize", dict(k_neighbors=8, num_mpnn_layers=2), Xn, mn)
    # C2-shaped miniature: 4 RNAs of 100-140 nt at the defaults
    lens = [int(v) for v in synth.synth_lengths(4, 100, 140, seed=0)]
    case("rdesign_c2_mini", dict(), *T._batch(lens, seed=7), full=False, e_nodes=2, row_stride=4)
    # separated logits: the defaults with the read-out scaled so that argmax is a meaningful check of the bf16 path
    case("rdesign_separated", dict(), *T._batch([40, 33, 25, 7], seed=5), full=False, e_nodes=2, min_logit_std=2.0)
    # gradients (f64 autograd, eval mode): a small model in full; the default model (rdesign_defaults above) on every 1-D tensor,
    # rows ::128 of every matrix, per-tensor and flat norms and one seeded projection
    case("rdesign_grad_small", dict(k_neighbors=6, num_mpnn_layers=1, num_message_layers=2, num_dense_layers=1, dim_dense_layers=16),
         *T._batch([12, 4, 9], seed=5), full=False, e_nodes=2, label_seed=3)
    case("rdesign_grad_T_lt_k", dict(k_neighbors=6, num_mpnn_layers=1, num_message_layers=2, num_dense_layers=1, dim_dense_layers=16),
         *T._batch([4, 3], seed=5), full=False, e_nodes=2, label_seed=4, grad_stride=16)
    print(f"{'checked' if check else 'wrote'} the set: {total / 1024:.0f} KB")
    assert total <= MAX_SET_BYTES, f"the set is {total} bytes > {MAX_SET_BYTES}"


if __name__ == "__main__":
    main()
