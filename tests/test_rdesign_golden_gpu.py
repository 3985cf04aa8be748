"""The rdesign HIP path against the REFERENCE's own modules: `rdesign_forward` (f32 and bf16) and both training steps (`rdesign_loss_and_grad_ex`,
p = 0) compared with tests/golden/rdesign_*.npz (tools/gen_golden_rdesign.py; keys: tests/_rdesign_cases.py), not with the restatement
oracle/rdesign_oracle.py.  Every case runs at the fixture's weight seed (leg 1: every stored tap) and at its second one (leg 2: logits in full,
h_V and gradient rows on a stride), so no fixture passes by accident of one weight draw.  The bounds are the ones the oracle-based files use,
imported where they are importable; measured values: DESIGN.md section 9."""
import numpy as np
import pytest
import torch

from _rdesign_cases import GRAD_GOLDEN, RDESIGN_GOLDEN, golden_weights, load_rdesign_golden, probe_vector
from test_hip_parity import BF16_GRAD_REL, bf16_tol
from test_rdesign_train_gpu import F32_COS, GRAD_REL_CAP, LOGIT_TOL, LOSS_TOL, MEASURED_GRAD_REL
from test_train_parity_gpu import BF16_COS, BF16_LOSS_TOL

pytestmark = pytest.mark.gpu

LEGS = [1, 2]
F32_TOL = 2e-4                       # tests/test_rdesign_gpu.py::test_forward_f32_matches_oracle
BF16_TOL = 5e-2                      # tests/test_rdesign_gpu.py::test_forward_bf16_within_tolerance
MARGIN = 0.1                         # 2 x BF16_TOL: the smallest top-2 logit margin that a 5e-2 error on each logit cannot flip
# Per-tensor bound of the f32 step: 4 x the worst-tensor error tests/test_rdesign_train_gpu.py measured (its convention).  rdesign_defaults is
# that file's "defaults" shape.  The two small gradient models have no entry there: they take the file's largest p = 0 bound - they are
# shallower (1 layer against 9) and narrower than the shape that bound was measured on, so f32 rounding accumulates over fewer sums.
F32_GRAD_REL = {"rdesign_defaults": 4 * MEASURED_GRAD_REL[("defaults", 0.0)]}
F32_GRAD_REL_OTHER = 4 * max(v for (_, p), v in MEASURED_GRAD_REL.items() if p == 0.0)


def _load(name, leg):
    a, meta = load_rdesign_golden(name)
    cfg, sd = golden_weights(meta, leg)
    return a, meta, cfg, sd, torch.from_numpy(a["X"]), torch.from_numpy(a["mask"])


def _model(meta, sd, precision, train_precision=None):
    from rdesign.model.rdesign import RNAModel
    kw = {k: v for k, v in meta["cfg"].items() if k != "num_rbf"}
    m = RNAModel(precision=precision, train_precision=train_precision, dropout=0.1, **kw)
    m.load_state_dict(sd)
    return m.cuda().eval()


def _golden_h_logits(a, meta, leg):
    """-> (row stride of the stored f32 h_V, h_V, logits) of one leg."""
    if leg == 1:
        return 1, torch.from_numpy(a["h_V"]), torch.from_numpy(a["logits"])
    return meta["s2_row_stride"], torch.from_numpy(a["s2.h_V"]), torch.from_numpy(a["s2.logits"])


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", RDESIGN_GOLDEN)
def test_forward_f32_matches_reference(name, leg):
    """Neighbour lists bit-exact against the reference's E_idx (count, order, dst and src), raw features within the column-group tolerances
    of test_features_and_graph_match_oracle, h_V and logits within 2e-4 of the reference's f32 run."""
    a, meta, cfg, sd, X, mask = _load(name, leg)
    m = _model(meta, sd, "f32")
    out = {k: v.cpu() for k, v in m._run(X, mask, want=("edge_index", "node_raw", "edge_raw", "h_V", "logits")).items()}
    mb = mask == 1
    n, K = int(mb.sum()), cfg.k_neighbors
    idx = out["edge_index"][mb]                                                   # (n, K), -1 = not attended
    valid = idx >= 0
    shift = (mask.sum(1).cumsum(0) - mask.sum(1)).long().view(-1, 1).expand(mask.shape)[mb]
    dst = torch.arange(n).view(n, 1).expand(n, K)[valid]
    src = (shift.view(n, 1) + idx)[valid]
    ref_E = torch.from_numpy(a["E_idx"]).long()
    assert dst.shape[0] == ref_E.shape[1], f"edge count {dst.shape[0]} != reference {ref_E.shape[1]}"
    assert torch.equal(torch.stack([dst, src]), ref_E)
    assert (out["edge_index"][~mb] < 0).all()
    d = (out["node_raw"][::meta["row_stride"]] - torch.from_numpy(a["node_raw"])).abs()
    got_e = out["edge_raw"].view(n, K, 115)
    ref_e = torch.from_numpy(a["edge_raw"])
    de = (got_e[valid][:ref_e.shape[0]] - ref_e).abs()
    rs, ref_h, ref_l = _golden_h_logits(a, meta, leg)
    dh = float((out["h_V"][::rs] - ref_h).abs().max())
    dl = float((out["logits"] - ref_l).abs().max())
    print(f"\n{name} leg {leg} f32: node rbf+dir {float(d[:, 12:].max()):.2e} dihedral {float(d[:, :12].max()):.2e}, edge rbf+dir "
          f"{float(de[:, 4:].max()):.2e} quaternion {float(de[:, :4].max()):.2e}, h_V {dh:.2e}, logits {dl:.2e}")
    assert d[:, 12:].max() < 2e-5 and d[:, :12].max() < 5e-4
    assert de[:, 4:].max() < 5e-5 and de[:, :4].max() < 2e-3
    assert got_e[~valid].abs().max() == 0 if (~valid).any() else True
    assert out["h_V"].shape == (n, 128) and dh < F32_TOL and dl < F32_TOL
    h_V, _ = m(X, torch.zeros(mask.shape, dtype=torch.long), mask)                # the public surface: forward + readout
    assert float((m.readout(h_V).cpu() - ref_l).abs().max()) < F32_TOL


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", RDESIGN_GOLDEN)
def test_forward_bf16_matches_reference(name, leg):
    """h_V and logits within 5e-2 of the reference's f32 run; on the separated-logit case the argmax equals the reference's on every row
    whose reference top-2 margin exceeds 0.1 (at least 90 % of the rows: asserted by the generator on the reference alone, stored)."""
    a, meta, cfg, sd, X, mask = _load(name, leg)
    m = _model(meta, sd, "bf16")
    out = {k: v.cpu() for k, v in m._run(X, mask, want=("h_V", "logits")).items()}
    rs, ref_h, ref_l = _golden_h_logits(a, meta, leg)
    dh = float((out["h_V"][::rs] - ref_h).abs().max())
    dl = float((out["logits"] - ref_l).abs().max())
    top2 = ref_l.topk(2, dim=-1).values
    keep = (top2[:, 0] - top2[:, 1]) > MARGIN
    agree = out["logits"].argmax(-1)[keep] == ref_l.argmax(-1)[keep]
    print(f"\n{name} leg {leg} bf16: h_V {dh:.2e}, logits {dl:.2e}, reference logit std {float(ref_l.std()):.3f} range "
          f"{float(ref_l.max() - ref_l.min()):.2f}: max|dlogit| / std {dl / float(ref_l.std()):.2e}, / range "
          f"{dl / float(ref_l.max() - ref_l.min()):.2e}; argmax agrees on {int(agree.sum())} of {int(keep.sum())} rows with margin > {MARGIN} "
          f"({int((~keep).sum())} of {keep.numel()} left out)")
    assert dh < BF16_TOL and dl < BF16_TOL
    if name == "rdesign_separated":
        share = float((~keep).double().mean())
        assert float(ref_l.std()) >= 2.0 and share <= 0.10 and abs(share - meta["excluded_share" + ("" if leg == 1 else "2")]) < 1e-12
        assert bool(agree.all())


def _grad_check(name, leg, a, meta, cfg, g, per_tensor, cos_min):
    """Device gradient `g` ({key: tensor}) against one leg of the stored float64 autograd gradient.  Whole gradient stored: the definition of
    `_rdesign_train_ref.grad_errors` (per tensor max|g - r| / max|r|, flat cosine).  Rows ::stride stored: the same per tensor on the stored
    rows, and in place of the cosine what cos > 1 - c allows at equal norms, |g - r| < sqrt(2c) |r|: every per-tensor norm and the flat norm
    within sqrt(2c) relative, and the projection <g - r, v> on the stored standard-normal v (standard deviation |g - r|) within 4 sigma."""
    from oracle import rdesign_oracle as O
    pre = "" if leg == 1 else "s2."
    gs = meta["grad_stride"] if leg == 1 else meta["s2_grad_stride"]
    keys = list(O.state_dict_shapes(cfg))
    rel = {}
    for k in keys:
        r = torch.from_numpy(a[pre + "grad." + k])
        got = g[k].double() if (g[k].dim() == 1 or gs is None) else g[k].double()[::gs]
        assert got.shape == r.shape and float(r.abs().max()) > 0, k
        rel[k] = float((got - r).abs().max() / r.abs().max())
    worst = max(rel, key=rel.get)
    flat = torch.cat([g[k].double().reshape(-1) for k in keys])
    slack = (2 * (1 - cos_min)) ** 0.5
    ref_norms = torch.from_numpy(a[pre + "grad_norm"])
    norms = torch.tensor([float(g[k].double().norm()) for k in keys], dtype=torch.float64)
    ref_flat = float(a[pre + "grad_flat_norm"])
    d_norm = float(((norms - ref_norms).abs() / ref_flat).max())
    d_flat = abs(float(flat.norm()) - ref_flat) / ref_flat
    d_probe = abs(float(flat @ probe_vector(int(a["grad_probe_seed"]), flat.numel())) - float(a[pre + "grad_probe_dot"])) / ref_flat
    msg = (f"worst per-tensor {rel[worst]:.3e} ({worst}), median {np.median(list(rel.values())):.2e}, bound {per_tensor:.1e}; tensor norms "
           f"{d_norm:.2e} and flat norm {d_flat:.2e} of |r| (allowed {slack:.2e}), projection {d_probe:.2e} of |r| (allowed {4 * slack:.2e})")
    cos = None
    if gs is None:
        ref_full = torch.cat([torch.from_numpy(a[pre + "grad." + k]).reshape(-1) for k in keys])
        cos = float(flat @ ref_full) / float(flat.norm() * ref_full.norm())
        msg += f", cos 1-{1 - cos:.1e}"
    print(f"   {name} leg {leg}: " + msg)
    assert rel[worst] < per_tensor, f"{worst}: {rel[worst]:.2e}"
    assert d_norm < slack and d_flat < slack and d_probe < 4 * slack
    if cos is not None:
        assert cos > cos_min
    return rel


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", GRAD_GOLDEN)
def test_f32_training_step_matches_reference_autograd(name, leg):
    """`loss_and_grad` at p = 0 against the reference's float64 loss, logits and autograd gradients: logits 2e-4, loss 4e-4, per-tensor bound
    of tests/test_rdesign_train_gpu.py (F32_GRAD_REL above), cosine > 1 - 1e-6.  Unlike that file, nothing of the device enters the reference
    side: the device's own f32 features are part of what is compared."""
    a, meta, cfg, sd, X, mask = _load(name, leg)
    pre = "" if leg == 1 else "s2."
    m = _model(meta, sd, "f32")
    S = torch.from_numpy(a["S"])
    loss, logits = m.loss_and_grad(X, S, mask, dropout=0.0, seed=1, return_logits=True)
    dlogit = float((logits.cpu().double() - torch.from_numpy(a[pre + "logits_f64"])).abs().max())
    dloss = abs(float(loss) - float(a[pre + "loss_f64"]))
    bound = F32_GRAD_REL.get(name, F32_GRAD_REL_OTHER)
    print(f"\n{name} leg {leg} f32 step: |dloss| {dloss:.2e}, max|dlogit| {dlogit:.2e}")
    assert bound <= GRAD_REL_CAP
    assert dlogit < LOGIT_TOL and dloss < LOSS_TOL
    _grad_check(name, leg, a, meta, cfg, _grads(m), bound, F32_COS)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", GRAD_GOLDEN)
def test_bf16_mixed_training_step_matches_reference_autograd(name, leg):
    """`train_precision="bf16"` at p = 0 against the same goldens with the bounds of tests/test_rdesign_train_bf16_gpu.py, unchanged:
    BF16_LOSS_TOL, bf16_tol(reference logits), BF16_GRAD_REL per tensor, BF16_COS."""
    a, meta, cfg, sd, X, mask = _load(name, leg)
    pre = "" if leg == 1 else "s2."
    m = _model(meta, sd, "f32", train_precision="bf16")
    S = torch.from_numpy(a["S"])
    loss, logits = m.loss_and_grad(X, S, mask, dropout=0.0, seed=1, return_logits=True)
    ref_logits = torch.from_numpy(a[pre + "logits_f64"])
    dlogit = float((logits.cpu().double() - ref_logits).abs().max())
    dloss = abs(float(loss) - float(a[pre + "loss_f64"]))
    tol = bf16_tol(ref_logits)
    print(f"\n{name} leg {leg} bf16-mixed step: |dloss| {dloss:.2e}, max|dlogit| {dlogit:.2e} (tol {tol:.1e})")
    assert torch.isfinite(m.flat_grad).all()
    assert dloss < BF16_LOSS_TOL and dlogit < tol
    _grad_check(name, leg, a, meta, cfg, _grads(m), BF16_GRAD_REL, BF16_COS)


@pytest.mark.parametrize("name", ["rdesign_short_k6", "rdesign_defaults"])
def test_wrong_weight_seed_misses_the_golden(name):
    """The fixtures are read and the seed matters: the same comparison with the weights of another seed misses the f32 bound by orders of
    magnitude, on the forward and on the gradient."""
    a, meta = load_rdesign_golden(name)
    cfg, sd = golden_weights(meta, seed=meta["weight_seed"] + 7)
    X, mask = torch.from_numpy(a["X"]), torch.from_numpy(a["mask"])
    m = _model(meta, sd, "f32")
    out = m._run(X, mask, want=("h_V", "logits"))
    assert float((out["logits"].cpu() - torch.from_numpy(a["logits"])).abs().max()) > 100 * F32_TOL
    assert float((out["h_V"].cpu() - torch.from_numpy(a["h_V"])).abs().max()) > 100 * F32_TOL
    if name in GRAD_GOLDEN:
        m.loss_and_grad(X, torch.from_numpy(a["S"]), mask, dropout=0.0, seed=1)
        with pytest.raises(AssertionError):
            _grad_check(name, 1, a, meta, cfg, _grads(m), F32_GRAD_REL[name], F32_COS)
