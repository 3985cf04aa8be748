"""GPU checks of the rdesign bf16-MIXED training step (`rdesign_loss_and_grad_ex` with RDESIGN_TRAIN_BF16_MIXED, `RNAModel(train_precision=
"bf16")`) against the fp64 restatement tests/_rdesign_train_ref.py differentiated by torch autograd - the checker of the f32 step
(tests/test_rdesign_train_gpu.py), fed the DEVICE's raw features in the same way, with the same dropout masks.  The bounds are the ones the
project uses for its bf16-mixed trainer (imported, not copied): BF16_LOSS_TOL, bf16_tol, BF16_GRAD_REL, BF16_COS.
The checker is a restatement; at p = 0 it is pinned to the reference's own autograd (tests/test_rdesign_golden_cpu.py), and
tests/test_rdesign_golden_gpu.py compares this step with the reference directly.  The dropout masks have no reference counterpart."""
import numpy as np
import pytest
import torch

from test_hip_parity import BF16_GRAD_REL, bf16_tol
from test_rdesign_cpu import _batch
from test_rdesign_train_gpu import SEED, SHAPES, TRAIN_KW, TRAIN_LENGTHS, _grads, _labels, _model, _reference_curve
from test_train_parity_gpu import BF16_COS, BF16_LOSS_TOL
import _rdesign_train_ref as R

pytestmark = pytest.mark.gpu

CASES = [(name, p) for name in SHAPES for p in (0.0, 0.1)]
# Worst per case as MEASURED on an MI355X (printed by test_loss_logits_and_gradients_match_fp64_autograd):
# (|dloss|, max|dlogit|, worst per-tensor gradient error relative to the tensor's largest reference entry, 1 - flat cosine, median per-tensor
# error with every label shifted by one class).  A CPU fp64 emulation of the bf16 roundings alone gave 3.7e-2 for the worst tensor (defaults,
# p = 0.1), <= 1.0e-2 on the other shapes, 1 - cos <= 6.4e-5, max|dlogit| <= 1.5e-2, |dloss| <= 3.3e-4.
MEASURED = {
    ("short_k6", 0.0): (5.5e-4, 5.6e-3, 8.4e-3, 8.1e-6, 1.47), ("short_k6", 0.1): (3.4e-4, 7.1e-3, 1.08e-2, 1.2e-5, 1.52),
    ("defaults", 0.0): (1.3e-4, 1.47e-2, 3.35e-2, 5.7e-5, 1.59), ("defaults", 0.1): (4.5e-4, 1.40e-2, 2.89e-2, 6.0e-5, 1.62),
    ("readout2", 0.0): (1.4e-4, 1.13e-2, 7.3e-3, 1.4e-5, 1.28), ("readout2", 0.1): (1.9e-4, 1.05e-2, 7.6e-3, 1.6e-5, 1.32),
    ("edges_75k", 0.0): (1.6e-4, 1.08e-2, 5.6e-3, 3.7e-6, 0.187), ("edges_75k", 0.1): (1.0e-4, 1.07e-2, 5.4e-3, 3.2e-6, 0.228),
}
# It trains: largest |HIP loss - fp64 loss| over the 40 Adam steps as MEASURED on an MI355X (printed by the test; the mixed curve falls from
# 1.5259 to 0.000477 next to fp64's 1.5262 to 0.000478), asserted at 10x
MEASURED_CURVE_DEV = {"adam": 5.58e-3, "flat": 5.81e-3}


def _mixed(kw, precision="f32", seed=0, dropout=0.1):
    m, cfg, sd = _model(kw, precision=precision, seed=seed, dropout=dropout)
    m.train_precision = "bf16"
    return m, cfg, sd


_cache = {}


def _case(name, p):
    """One f32-precision model with train_precision="bf16", batch and fp64 reference per (shape, dropout)."""
    if (name, p) not in _cache:
        kw, lengths = SHAPES[name]
        m, cfg, sd = _mixed(kw)
        X, mask = _batch(lengths, seed=5)
        S = _labels(mask)
        feats = R.device_features(m.eval(), X, mask)
        m.train()
        loss, logits, grads = R.loss_and_grads(feats, mask, S, sd, cfg, p, SEED)
        _cache[(name, p)] = dict(m=m, cfg=cfg, sd=sd, X=X, mask=mask, S=S, loss=loss, logits=logits, grads=grads)
    return _cache[(name, p)]


@pytest.mark.parametrize("name,p", CASES)
def test_loss_logits_and_gradients_match_fp64_autograd(name, p):
    """|dloss| < BF16_LOSS_TOL, max|dlogit| < bf16_tol(reference logits), every parameter gradient within BF16_GRAD_REL of its largest
    reference entry, flat cosine > BF16_COS, with and without dropout (same masks as the reference: a function of seed, site, element).
    Negative control: the device gradient with ALL labels shifted by one class misses the unshifted reference by more than BF16_GRAD_REL
    in the MEDIAN tensor.  Measured values: MEASURED above."""
    c = _case(name, p)
    m = c["m"]
    assert m.train_precision == "bf16" and (name, p) in MEASURED
    loss, logits = m.loss_and_grad(c["X"], c["S"], c["mask"], dropout=p, seed=SEED, return_logits=True)
    rel, cos = R.grad_errors(_grads(m), c["grads"])
    worst = max(rel, key=rel.get)
    dlogit = float((logits.cpu().double() - c["logits"]).abs().max())
    dloss = abs(float(loss) - c["loss"])
    tol = bf16_tol(c["logits"])
    m.loss_and_grad(c["X"], (c["S"] + 1) % 4, c["mask"], dropout=p, seed=SEED)
    rel2, _ = R.grad_errors(_grads(m), c["grads"])
    med2 = float(np.median(list(rel2.values())))
    print(f"\n{name} p={p}: |dloss| {dloss:.2e}, max|dlogit| {dlogit:.2e} (tol {tol:.1e}), worst per-tensor {rel[worst]:.3e} ({worst}), median "
          f"{np.median(list(rel.values())):.2e}, cos 1-{1 - cos:.1e}; all labels shifted: median {med2:.2e}")
    assert torch.isfinite(m.flat_grad).all()
    assert dloss < BF16_LOSS_TOL
    assert dlogit < tol
    assert cos > BF16_COS
    assert rel[worst] < BF16_GRAD_REL, f"{worst}: {rel[worst]:.2e}"
    assert med2 > BF16_GRAD_REL, f"negative control: shifting every label moves the median tensor by only {med2:.2e}"


def test_determinism_and_dropout_plumbing():
    c = _case("short_k6", 0.1)
    m, X, S, mask = c["m"], c["X"], c["S"], c["mask"]
    m.train()
    l1 = m.loss_and_grad(X, S, mask, seed=SEED).clone()
    g1 = m.flat_grad.clone()
    l2 = m.loss_and_grad(X, S, mask, seed=SEED).clone()
    assert torch.equal(l1, l2) and torch.equal(g1, m.flat_grad)                      # bit-reproducible
    m.loss_and_grad(X, S, mask, seed=SEED + 1)
    assert not torch.equal(g1, m.flat_grad)                                          # another seed, another mask
    m.manual_seed(SEED)
    m.loss_and_grad(X, S, mask)                                                      # the module's counter: SEED, then SEED + 1
    assert torch.equal(g1, m.flat_grad)
    m.loss_and_grad(X, S, mask)
    assert not torch.equal(g1, m.flat_grad)
    m.eval()                                                                         # eval mode = dropout 0 = independent of the seed
    le = m.loss_and_grad(X, S, mask, seed=1).clone()
    ge = m.flat_grad.clone()
    l0 = m.loss_and_grad(X, S, mask, dropout=0.0, seed=2)
    assert torch.equal(le, l0) and torch.equal(ge, m.flat_grad) and not torch.equal(ge, g1)
    # layout: every p.grad is a view of flat_grad at the arena offset, the padding floats are zero
    live = torch.zeros_like(m.flat_grad, dtype=torch.bool)
    base = m.flat_grad.data_ptr()
    for key, numel, off in m._handle.weight_schema():
        p = dict(m.named_parameters())[key]
        assert p.grad.data_ptr() == base + 4 * off and p.grad.numel() == numel
        live[off: off + numel] = True
    if (~live).any():
        assert float(m.flat_grad[~live].abs().max()) == 0.0
    assert torch.isfinite(m.flat_grad).all() and float(m.flat_grad.abs().max()) > 0
    m.train()


@pytest.mark.parametrize("kw,lengths", [SHAPES["short_k6"], SHAPES["readout2"]], ids=["M3", "M2_readout2"])
def test_either_handle_gives_the_same_bits(kw, lengths):
    """A precision="f32" and a precision="bf16" model with the same weights run the same kernels on the same nn.Linear-layout weights."""
    ma, _, _ = _mixed(kw, precision="f32")
    mb, _, _ = _mixed(kw, precision="bf16")
    X, mask = _batch(lengths, seed=5)
    S = _labels(mask)
    ma.train(); mb.train()
    for p in (0.0, 0.1):
        la = ma.loss_and_grad(X, S, mask, dropout=p, seed=SEED)
        lb = mb.loss_and_grad(X, S, mask, dropout=p, seed=SEED)
        assert torch.equal(la, lb) and torch.equal(ma.flat_grad, mb.flat_grad) and float(ma.flat_grad.abs().max()) > 0
    # and train_precision="f32" on the same model is still the exact-f32 step: other bits, the same loss within the bf16 bound
    ma.train_precision = "f32"
    lf = ma.loss_and_grad(X, S, mask, dropout=0.1, seed=SEED)
    assert not torch.equal(ma.flat_grad, mb.flat_grad) and abs(float(lf) - float(lb)) < BF16_LOSS_TOL


def test_autograd_surface():
    c = _case("short_k6", 0.1)
    m, X, S, mask = c["m"], c["X"], c["S"], c["mask"]
    m.train()
    batch = (X, S, mask, SHAPES["short_k6"][1], None)
    m.manual_seed(5)
    m.loss_and_grad(X, S, mask)
    g = m.flat_grad.clone()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    m.manual_seed(5)
    loss = m.training_step(batch)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    assert torch.equal(m.flat_grad, g)                                               # bit for bit the gradient of loss_and_grad
    m.manual_seed(5)
    m.training_step(batch).backward()                                                # no zero_grad: accumulates
    assert torch.equal(m.flat_grad, 2 * g)
    opt.zero_grad(set_to_none=True)
    m.manual_seed(5)
    (2.0 * m.training_step(batch)).backward()                                        # scaled by the incoming gradient
    assert torch.equal(m.flat_grad, 2 * g)
    with torch.no_grad():
        out = m.training_step(batch)
        assert not out.requires_grad and out.grad_fn is None


@pytest.mark.parametrize("which", ["adam", "flat"])
def test_it_trains(which):
    """The 8-RNA, 40-step Adam(lr 2e-3) setting of the f32 test at dropout 0: the mixed loss falls below 10 % of its start (the fp64 curve
    falls from 1.5262 to 0.000478 - the condition catches a sign error or a dead tensor) and follows the fp64 curve within 10x the deviation
    measured on an MI355X."""
    m, cfg, sd = _mixed(TRAIN_KW, dropout=0.0)
    X, mask = _batch(TRAIN_LENGTHS, seed=9)
    S = _labels(mask)
    feats = R.device_features(m.eval(), X, mask)
    ref = _reference_curve(feats, mask, S, sd, cfg)
    m.train()
    batch = (X, S, mask, TRAIN_LENGTHS, None)
    opt = m.configure_optimizers(fused=which == "flat")[0][0]
    curve = []
    for _ in range(41):
        opt.zero_grad()
        loss = m.training_step(batch)
        curve.append(float(loss.detach()))
        loss.backward()
        opt.step()
    dev = max(abs(a - b) for a, b in zip(curve, ref))
    print(f"\n{which}: bf16-mixed loss {curve[0]:.4f} -> {curve[40]:.6f}, fp64 {ref[0]:.4f} -> {ref[40]:.6f}, largest deviation over 40 steps {dev:.3e}")
    assert ref[40] < 0.01 * ref[0]
    assert curve[40] < 0.1 * curve[0]
    assert dev < 10 * MEASURED_CURVE_DEV[which]


def test_flat_adam_tracks_torch_adam():
    """Two models with equal weights and bit-equal bf16-mixed gradients, three steps of each optimiser on that ONE gradient (the f32 file's
    form: recomputing the gradient would compare bf16 rounding noise through Adam's normalisation, not the optimisers): every parameter
    within 2e-6, the bound of test_hip_parity's fused-Adam test."""
    X, mask = _batch(TRAIN_LENGTHS, seed=9)
    S = _labels(mask)
    ma, _, _ = _mixed(TRAIN_KW, dropout=0.0)
    mb, _, _ = _mixed(TRAIN_KW, dropout=0.0)
    ma.train(); mb.train()
    ma.loss_and_grad(X, S, mask)
    mb.loss_and_grad(X, S, mask)
    assert torch.equal(ma.flat_grad, mb.flat_grad) and float(ma.flat_grad.abs().max()) > 0
    start = mb._flat.clone()
    oa = ma.configure_optimizers()[0][0]
    ob = mb.configure_optimizers(fused=True)[0][0]
    for _ in range(3):
        oa.step(); ob.step()
    worst = max(float((pa.detach() - pb.detach()).abs().max()) for pa, pb in zip(ma.parameters(), mb.parameters()))
    print(f"\nFlatAdam vs torch Adam after 3 steps on one bf16-mixed gradient: max |dparam| {worst:.2e}")
    assert float((mb._flat - start).abs().max()) > 1e-3
    assert worst < 2e-6


def test_inference_sees_the_trained_weights():
    """Three FlatAdam steps on a precision="bf16" model: its eval() forward (MFMA path with cached weight images) changes and equals, bit for
    bit, a fresh model loaded from the trained state_dict."""
    from rdesign.model.rdesign import RNAModel
    X, mask = _batch(TRAIN_LENGTHS, seed=9)
    S = _labels(mask)
    m, _, _ = _mixed(TRAIN_KW, precision="bf16", dropout=0.0)
    before = m.eval().forward_logits(X, mask).clone()
    m.train()
    opt = m.configure_optimizers(fused=True)[0][0]
    for _ in range(3):
        m.loss_and_grad(X, S, mask)
        opt.step()
    after = m.eval().forward_logits(X, mask).clone()
    assert float((after - before).abs().max()) > 1e-3
    fresh = RNAModel(precision="bf16", dropout=0.0, **TRAIN_KW)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    assert torch.equal(fresh.cuda().eval().forward_logits(X, mask), after)
    # the same with torch's optimiser (the parameters' version counters instead of FlatAdam's notification)
    m.train()
    opt2 = torch.optim.Adam(m.parameters(), lr=2e-3)
    m.loss_and_grad(X, S, mask)
    opt2.step()
    again = m.eval().forward_logits(X, mask)
    assert float((again - after).abs().max()) > 1e-4


def test_refusals():
    from rdesign.model.rdesign import RNAModel
    with pytest.raises(ValueError, match="train_precision"):
        RNAModel(train_precision="int8")
    kw = dict(k_neighbors=6, num_mpnn_layers=1, num_message_layers=4)
    m = RNAModel(precision="f32", train_precision="bf16", **kw).cuda().train()
    X, mask = _batch([12, 4, 9], seed=5)
    S = _labels(mask)
    with pytest.raises(NotImplementedError, match="num_message_layers"):             # RDESIGN_ERR_UNSUPPORTED of the library
        m.loss_and_grad(X, S, mask)
    with pytest.raises(NotImplementedError, match="num_message_layers"):
        m.training_step((X, S, mask, [12, 4, 9], None))
    m.train_precision = "f32"                                                        # the f32 step takes any depth
    assert torch.isfinite(m.loss_and_grad(X, S, mask))
