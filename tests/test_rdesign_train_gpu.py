"""GPU checks of the rdesign f32 training step (`rdesign_loss_and_grad`, `RNAModel.loss_and_grad` / `training_step`, `FlatAdam`)
against the fp64 restatement tests/_rdesign_train_ref.py differentiated by torch autograd.  The reference is fed the DEVICE's raw
features (taps of `rdesign_forward`, parent-commit code with its own test), so the comparison sees only the training code.
The checker is a restatement; at p = 0 it is pinned to the reference's own autograd (tests/test_rdesign_golden_cpu.py), and
tests/test_rdesign_golden_gpu.py compares this step with the reference directly.  The dropout masks have no reference counterpart."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import rdesign_oracle as O
from test_rdesign_cpu import _batch, _weights
from test_rdesign_gpu import CASES as FWD_CASES
import _rdesign_train_ref as R

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-4             # the bound test_forward_f32_matches_oracle uses for this path
LOSS_TOL = 4e-4              # cross-entropy moves by at most 2 max|dlogit|
F32_COS = 0.999999           # tests/test_train_parity_gpu.py
GRAD_REL_CAP = 2e-3          # no per-tensor bound of the f32 trainer may exceed it
SEED = 71
# Per-tensor error of the HIP gradient vs fp64 autograd, worst tensor of each case as MEASURED on an MI355X (printed by
# test_loss_logits_and_gradients_match_fp64_autograd); the bound asserted is 4x the measurement (the convention of F32_GRAD_REL in
# tests/test_train_parity_gpu.py).  Orientation: torch's own fp32 autograd differs from fp64 by 1.0e-6 / 1.3e-6 / 4.6e-6 on the
# first three shapes.
MEASURED_GRAD_REL = {
    ("short_k6", 0.0): 1.04e-6, ("short_k6", 0.1): 8.6e-7,
    ("defaults", 0.0): 2.05e-6, ("defaults", 0.1): 2.82e-6,
    ("readout2", 0.0): 1.14e-6, ("readout2", 0.1): 1.28e-6,
    ("edges_75k", 0.1): 9.5e-7,
}
BIG_LENGTHS = [110 + (7 * i) % 31 for i in range(24)]                    # 24 RNAs of 110..140 nt: > 65,536 edge rows at k = 25
SHAPES = {"short_k6": FWD_CASES[0], "defaults": FWD_CASES[1], "readout2": FWD_CASES[2],
          "edges_75k": (dict(k_neighbors=25, num_mpnn_layers=2), BIG_LENGTHS)}
CASES = list(MEASURED_GRAD_REL)
# It trains: largest |HIP loss - fp64 loss| over the 40 Adam steps as MEASURED on an MI355X (printed by the test; both optimisers
# gave 2.308e-7 on a curve that falls from 1.5262 to 0.000478), asserted at 10x
MEASURED_CURVE_DEV = {"adam": 2.31e-7, "flat": 2.31e-7}


def _model(kw, precision="f32", seed=0, dropout=0.1):
    from rdesign.model.rdesign import RNAModel
    m = RNAModel(precision=precision, dropout=dropout, **kw)
    cfg = O.RDesignConfig(**kw)
    sd = _weights(cfg, seed)
    m.load_state_dict(sd)
    return m.cuda(), cfg, sd


def _labels(mask, seed=3):
    return torch.randint(0, 4, tuple(mask.shape), generator=torch.Generator().manual_seed(seed))


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


_cache = {}


def _case(name, p):
    """One model, batch and fp64 reference per (shape, dropout)."""
    if (name, p) not in _cache:
        kw, lengths = SHAPES[name]
        m, cfg, sd = _model(kw)
        X, mask = _batch(lengths, seed=5)
        S = _labels(mask)
        feats = R.device_features(m.eval(), X, mask)
        m.train()
        loss, logits, grads = R.loss_and_grads(feats, mask, S, sd, cfg, p, SEED)
        _cache[(name, p)] = dict(m=m, cfg=cfg, sd=sd, X=X, mask=mask, S=S, feats=feats, loss=loss, logits=logits, grads=grads)
    return _cache[(name, p)]


@pytest.mark.parametrize("name,p", CASES)
def test_loss_logits_and_gradients_match_fp64_autograd(name, p):
    """Loss within 4e-4, logits within 2e-4, every parameter gradient within 4x the measured worst-tensor error of the case (never
    above 2e-3), flat cosine > 1 - 1e-6; with dropout on as well - the masks are the same function of (seed, site, element).
    Negative control: the HIP gradient with ONE label flipped misses the unflipped reference by more than that bound in the
    MEDIAN tensor."""
    c = _case(name, p)
    m = c["m"]
    assert (sum(SHAPES[name][1]) * m.hparams["k_neighbors"] > 65536) == (name == "edges_75k")
    loss, logits = m.loss_and_grad(c["X"], c["S"], c["mask"], dropout=p, seed=SEED, return_logits=True)
    g = _grads(m)
    rel, cos = R.grad_errors(g, c["grads"])
    worst = max(rel, key=rel.get)
    dlogit = float((logits.cpu().double() - c["logits"]).abs().max())
    dloss = abs(float(loss) - c["loss"])
    bound = 4 * MEASURED_GRAD_REL[(name, p)]
    S2 = c["S"].clone()
    S2[0, 0] = (S2[0, 0] + 1) % 4
    m.loss_and_grad(c["X"], S2, c["mask"], dropout=p, seed=SEED)
    rel2, _ = R.grad_errors(_grads(m), c["grads"])
    med2 = float(np.median(list(rel2.values())))
    print(f"\n{name} p={p}: |dloss| {dloss:.2e}, max|dlogit| {dlogit:.2e}, worst per-tensor {rel[worst]:.3e} ({worst}), median "
          f"{np.median(list(rel.values())):.2e}, cos 1-{1 - cos:.1e}; bound {bound:.1e}; one label flipped: median {med2:.2e}")
    assert bound <= GRAD_REL_CAP
    assert dlogit < LOGIT_TOL
    assert dloss < LOSS_TOL
    assert cos > F32_COS
    assert rel[worst] < bound, f"{worst}: {rel[worst]:.2e}"
    assert med2 > bound, f"negative control: one flipped label moves the median tensor by only {med2:.2e}"


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
    S_p = S[mask == 1].cuda()
    assert abs(float(le) - float(m.loss_fn(m.forward_logits(X, mask), S_p))) < LOSS_TOL   # the inference path's loss
    # layout: every p.grad is a view of flat_grad at the arena offset, the padding floats are zero
    live = torch.zeros_like(m.flat_grad, dtype=torch.bool)
    base = m.flat_grad.data_ptr()
    for key, numel, off in m._handle.weight_schema():
        p = dict(m.named_parameters())[key]
        assert p.grad.data_ptr() == base + 4 * off and p.grad.numel() == numel
        live[off: off + numel] = True
    if (~live).any():                                # (every tensor of the configurations built so far is a multiple of 4 floats)
        assert float(m.flat_grad[~live].abs().max()) == 0.0
    assert torch.isfinite(m.flat_grad).all()
    m.train()


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
    assert all(p.grad is None for p in m.parameters())
    m.manual_seed(5)
    loss = m.training_step(batch)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    assert all(p.grad is not None and p.grad.data_ptr() >= m.flat_grad.data_ptr() for p in m.parameters())   # views re-bound
    assert torch.equal(m.flat_grad, g)                                               # bit for bit the gradient of loss_and_grad
    m.manual_seed(5)
    m.training_step(batch).backward()                                                # no zero_grad: accumulates
    assert torch.equal(m.flat_grad, 2 * g)
    opt.zero_grad(set_to_none=True)
    m.manual_seed(5)
    (2.0 * m.training_step(batch)).backward()                                        # scaled by the incoming gradient
    assert torch.equal(m.flat_grad, 2 * g)
    opt.zero_grad(set_to_none=True)
    m.manual_seed(5)
    la, lb = m.training_step(batch), m.training_step(batch)                          # seeds 5 and 6
    (la + lb).backward()
    ga = m.flat_grad.clone()
    m.loss_and_grad(X, S, mask, seed=5)
    g5 = m.flat_grad.clone()
    m.loss_and_grad(X, S, mask, seed=6)
    assert torch.equal(ga, g5 + m.flat_grad) and not torch.equal(g5, m.flat_grad)
    with torch.no_grad():
        assert not m.training_step(batch).requires_grad


def test_bf16_model_refuses_the_training_step():
    m, cfg, sd = _model(dict(k_neighbors=6, num_mpnn_layers=2), precision="bf16")
    X, mask = _batch([12, 4, 9], seed=5)
    S = _labels(mask)
    with pytest.raises(NotImplementedError, match="f32"):
        m.loss_and_grad(X, S, mask)
    with pytest.raises(NotImplementedError, match="f32"):
        m.training_step((X, S, mask, [12, 4, 9], None))
    lib = __import__("rdesign._native", fromlist=["lib"]).lib()
    assert lib.rdesign_train_workspace_bytes(m._handle.ptr, 3, 12) == 0              # the C ABI refuses as well


TRAIN_LENGTHS = [24, 17, 30, 9, 21, 28, 13, 26]
TRAIN_KW = dict(k_neighbors=8, num_mpnn_layers=3)


def _reference_curve(feats, mask, S, sd, cfg, steps=40, lr=2e-3):
    leaf = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(leaf.values()), lr=lr)
    node, edge, E_idx, attend = feats
    tgt = S[mask == 1].long()
    curve = []
    for _ in range(steps + 1):
        opt.zero_grad()
        _, logits = R.forward_train(node, edge, E_idx, attend, mask, leaf, cfg)
        loss = torch.nn.functional.cross_entropy(logits, tgt)
        curve.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return curve


@pytest.mark.parametrize("which", ["adam", "flat"])
def test_it_trains_as_the_fp64_reference_does(which):
    """40 steps of Adam(lr 2e-3) at dropout 0 on 8 small RNAs: the HIP loss falls below 10 % of its start (the fp64 reference
    falls to 0.04 % of it) and follows the fp64 curve within 10x the deviation measured on an MI355X."""
    m, cfg, sd = _model(TRAIN_KW, dropout=0.0)
    X, mask = _batch(TRAIN_LENGTHS, seed=9)
    S = _labels(mask)
    feats = R.device_features(m.eval(), X, mask)
    ref = _reference_curve(feats, mask, S, sd, cfg)
    m.train()
    batch = (X, S, mask, TRAIN_LENGTHS, None)
    if which == "flat":
        from rnampnn.model.rnampnn import FlatAdam
        opt = m.configure_optimizers(fused=True)[0][0]
        assert isinstance(opt, FlatAdam)
    else:
        opt = m.configure_optimizers()[0][0]
        assert type(opt) is torch.optim.Adam
    assert opt.param_groups[0]["lr"] == 2e-3
    curve = []
    for _ in range(41):
        opt.zero_grad()
        loss = m.training_step(batch)
        curve.append(float(loss.detach()))
        loss.backward()
        opt.step()
    dev = max(abs(a - b) for a, b in zip(curve, ref))
    print(f"\n{which}: HIP loss {curve[0]:.4f} -> {curve[40]:.6f}, fp64 {ref[0]:.4f} -> {ref[40]:.6f}, largest deviation over 40 steps {dev:.3e}")
    assert ref[40] < 0.01 * ref[0]                                                   # the reference itself trains (to 0.04 % in 40 steps)
    assert curve[40] < 0.1 * curve[0]
    assert dev < 10 * MEASURED_CURVE_DEV[which]


def test_flat_adam_matches_torch_adam_and_reaches_the_inference_path():
    """Two models with equal weights and bit-equal flat gradients, three steps of each optimiser on that ONE gradient: every
    parameter within 2e-6 (the bound of test_hip_parity's fused-Adam test); then the fused model's inference path sees the update."""
    X, mask = _batch(TRAIN_LENGTHS, seed=9)
    S = _labels(mask)
    ma, _, _ = _model(TRAIN_KW, dropout=0.0)
    mb, _, _ = _model(TRAIN_KW, dropout=0.0)
    before = mb.eval().forward_logits(X, mask).clone()
    ma.train(); mb.train()
    ma.loss_and_grad(X, S, mask)
    mb.loss_and_grad(X, S, mask)
    assert torch.equal(ma.flat_grad, mb.flat_grad) and float(ma.flat_grad.abs().max()) > 0
    oa = ma.configure_optimizers()[0][0]
    ob = mb.configure_optimizers(fused=True)[0][0]
    for _ in range(3):
        oa.step(); ob.step()
    worst = max(float((pa - pb).abs().max()) for pa, pb in zip(ma.parameters(), mb.parameters()))
    print(f"\nFlatAdam vs torch Adam after 3 steps: max |dparam| {worst:.2e}")
    assert worst < 2e-6
    la, lb = ma.eval().forward_logits(X, mask), mb.eval().forward_logits(X, mask)
    assert float((la - lb).abs().max()) < LOGIT_TOL
    assert float((lb - before).abs().max()) > 1e-3                                   # the in-place update reached the kernels' weight copies


def test_production_shape_is_finite_reproducible_and_sized_exactly():
    """64 RNAs x 100..500 nt at the defaults, dropout 0.1, train mode; the workspace query is exactly sufficient."""
    from rnampnn.utils import synth
    from rdesign import _native
    m, cfg, sd = _model(dict())
    m.train()
    lens = [int(v) for v in synth.synth_lengths(64, 100, 500, seed=3)]
    X, mask = _batch(lens, seed=7)
    S = _labels(mask)
    l1 = m.loss_and_grad(X, S, mask, seed=SEED).clone()
    g1 = m.flat_grad.clone()
    l2 = m.loss_and_grad(X, S, mask, seed=SEED)
    assert torch.isfinite(l1) and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(l1, l2) and torch.equal(g1, m.flat_grad)
    lib = _native.lib()
    B, T = mask.shape
    need = int(lib.rdesign_train_workspace_bytes(m._handle.ptr, B, T))
    tape = int(lib.rdesign_train_tape_bytes(m._handle.ptr, B, T))
    print(f"\nproduction shape: {sum(lens)} nt, loss {float(l1):.4f}, workspace {need / 2 ** 30:.2f} GiB, tape {tape / 2 ** 30:.2f} GiB")
    assert 0 < tape < need
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    base = (ws.data_ptr() + 255) // 256 * 256
    Xd, md, lab = X.cuda().contiguous(), mask.cuda().contiguous(), S.to(torch.int32).cuda().contiguous()
    loss, grad = torch.zeros((), device="cuda"), torch.zeros_like(g1)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(ws_bytes):
        return lib.rdesign_loss_and_grad(m._handle.ptr, ptr(Xd), ptr(md), ptr(lab), B, T, C.c_float(0.1), C.c_uint64(SEED), ptr(loss), None,
                                         ptr(grad), C.c_void_p(base), C.c_size_t(ws_bytes), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(need - 1) == 5                                                       # RDESIGN_ERR_WORKSPACE
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad, g1) and torch.equal(loss, l1)
