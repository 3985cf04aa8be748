"""Off-default node-side shapes on the device: heads 2, 4 and 16, FFN / read-out widths 32, 96, 160, 544 and 2048, chains with no fused
instance, against the oracle in float64 (``_node_shape_cases`` holds the table; test_node_shapes_cpu.py pins the oracle's attention to
torch at every head count and shows that the bounds used here see a wrong head count and a dropped K or N tail).

Reference: ``oracle.rnampnn_oracle`` in float64 on the k-NN graph of the f32 oracle, one forward with taps and one forward + backward per
case (and one more per dropout case), cached per module and shared by the f32 and the bf16 tests.  Every bound is imported from the test
that already asserts it for the same quantity at the default shape.

What ran: profiles/node_shapes_kernel_stats.txt is the kernel listing of this file (``rocprofv3 --kernel-trace --stats``), with the
kernel instances and fallbacks that only these shapes reach marked.
"""
import numpy as np
import pytest
import torch

import _node_shape_cases as NS
import test_hip_parity as P
from _tap_oracle import oracle_runs
from test_hip_parity import BF16_GRAD_REL, F32_LOGIT_TOL, bf16_tol
from test_mpnn_taps_gpu import F32_TAP_TOL
from test_mpnn_taps_gpu import _check as _check_tap
from test_mpnn_taps_gpu import _model as _model_with
from test_train_parity_gpu import (BF16_COS, BF16_LOSS_TOL, DEAD_ABS, F32_COS, F32_LOSS_TOL, grad_dict, grad_errors,
                                   oracle_loss_and_grad)

pytestmark = pytest.mark.gpu

# the per-tensor rule of test_loss_and_gradients_match_oracle_autograd and of
# test_gradients_with_dropout_match_oracle_autograd_and_are_bit_reproducible, and the latter's logit bound under dropout
F32_GRAD_REL, F32_GRAD_ABS = 2e-3, 1e-7
F32_DROPOUT_LOGIT_TOL = 2e-4
BF16_STAGE_TOL = 3e-2            # the bf16 node bound of test_standalone_stage_modules_match_oracle

_cache = {}


def _setup(case):
    """-> dict(hp, sd, coords, mask, labels, runs = {"f32", "f64", "autocast"}: oracle taps) of one case at its forward weights."""
    if ("fwd", case) not in _cache:
        hp, sd = NS.state_dict(case)
        coords, mask, labels = NS.batch()
        _cache["fwd", case] = dict(hp=hp, sd=sd, coords=coords, mask=mask, labels=labels,
                                   runs=oracle_runs(hp, sd, coords, mask))
    return _cache["fwd", case]


def _reference(case, dropout):
    """-> dict(hp, sd, coords, mask, labels, loss, logits, grads) of one case at its trainer weights: fp64 oracle autograd, with the
    library's dropout masks when ``dropout`` > 0."""
    if ("bwd", case, dropout) not in _cache:
        hp, sd = NS.state_dict(case, train=True)
        coords, mask, labels = NS.batch()
        loss, logits, grads = oracle_loss_and_grad(hp, sd, coords, mask, labels, dropout, NS.DROPOUT_SEED)
        _cache["bwd", case, dropout] = dict(hp=hp, sd=sd, coords=coords, mask=mask, labels=labels, loss=loss, logits=logits, grads=grads)
    return _cache["bwd", case, dropout]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case", NS.CASES)
def test_forward_matches_f64_oracle(case, precision):
    """Logits, ``embedding`` and the ``h_post`` / ``raw_emb`` taps of every case: f32 within F32_LOGIT_TOL (logits) and 2e-4 (taps); bf16
    within ``bf16_tol`` on the logits, and the two taps within M_BF16 x the error of the f32 oracle under bf16 autocast (``_check`` of
    test_mpnn_taps_gpu.py, unchanged).  The kernel's graph is the f32 oracle's; padded rows are exactly 0; two calls are bit-identical;
    ``forward_packed`` on the packed batch gives the valid rows of the padded call bit for bit."""
    from rnampnn.utils.data import pack_batch
    s = _setup(case)
    mask, ref = s["mask"], s["runs"]["f64"]
    c, m = torch.from_numpy(s["coords"]), torch.from_numpy(mask)
    model = _model_with(s["hp"], s["sd"], precision)
    taps = {k: v.cpu() for k, v in model.forward_taps(c, m, ["edge_index", "h_post", "raw_emb"]).items()}
    assert torch.equal(taps["edge_index"], s["runs"]["f32"]["edge_index"]), "the kernel's graph is not the f32 oracle's"
    logits = model(c, m).cpu()
    emb = model.embedding(c, m).cpu()
    valid = m.bool()
    err = {k: float((taps[k].double() - ref[k]).abs().max()) for k in ("logits", "h_post", "raw_emb", "embedding")}
    tol = F32_LOGIT_TOL if precision == "f32" else bf16_tol(ref["logits"], mask)
    print(f"\n{case} {precision}: max |dlogit| {err['logits']:.3e} (bound {tol:.1e}; logit std {float(ref['logits'][valid].std()):.3f}), "
          f"h_post {err['h_post']:.3e}, raw_emb {err['raw_emb']:.3e}, embedding {err['embedding']:.3e}")
    for key in ("logits", "h_post", "raw_emb", "embedding"):
        assert torch.isfinite(taps[key]).all(), key
        assert (taps[key][~valid] == 0).all(), f"{key}: a padded row is not 0"
    assert torch.equal(logits, taps["logits"]) and torch.equal(model(c, m).cpu(), logits)
    assert torch.equal(emb, taps["embedding"])
    assert torch.equal(emb, torch.cat([taps["h_post"], taps["raw_emb"]], -1))
    assert err["logits"] < tol
    if precision == "f32":
        for key in ("h_post", "raw_emb", "embedding"):
            assert err[key] < F32_TAP_TOL, f"{key}: {err[key]:.3e}"
    else:
        failures = []
        for key in ("h_post", "raw_emb"):
            _check_tap(case, precision, taps[key], s["runs"], key, mask, None, failures)
        assert not failures, failures
    packed, cu, max_len = pack_batch([c[b, :n] for b, n in enumerate(NS.LENS)])
    assert max_len == max(NS.LENS)
    lp, ep = model.forward_packed(packed.cuda(), cu.cuda(), max_len, want_embedding=True)
    assert torch.equal(lp.cpu(), logits[valid]) and torch.equal(ep.cpu(), emb[valid])


@pytest.mark.parametrize("case", list(NS.GOLDEN_NAMES))
def test_reference_goldens_stage_taps_f32_and_logits_bf16(golden, case):
    """The two reference-made fixtures of these shapes (plain closed-form weights): the f32 stage taps through the body of
    test_f32_stage_taps_match_reference_golden (``FULL_CASES`` lives in conftest.py and does not name them), and the bf16 logits within
    ``bf16_tol`` of the reference's."""
    name = NS.GOLDEN_NAMES[case]
    P.test_f32_stage_taps_match_reference_golden(golden, name)
    arrs, hp, shapes = golden(name)
    model, _ = P._model(hp, shapes, "bf16")
    logits = model(torch.from_numpy(arrs["coords"]), torch.from_numpy(arrs["mask"])).cpu().numpy()
    err = float(np.abs(logits - arrs["logits"]).max())
    print(f"\n{name} bf16: max |dlogit| vs the reference {err:.3e} (bound {bf16_tol(arrs['logits'], arrs['mask']):.1e})")
    assert np.isfinite(logits).all() and (logits[arrs["mask"] == 0] == 0).all()
    assert err < bf16_tol(arrs["logits"], arrs["mask"])


STAGES = ["RNABert_heads16_w160", "RNABert_heads2_w96", "RawFFN_w96", "Readout_w96"]


@pytest.mark.parametrize("stage", STAGES)
def test_standalone_bf16_stage_module_matches_oracle(stage):
    """``RNABert`` (heads 16 at width 160, heads 2 at width 96), ``RawFFN`` and ``Readout`` with precision="bf16" at S1's shapes and
    forward weights, on the f64 oracle's own stage inputs, against the oracle's stage functions in float64: within 3e-2, the bf16 bound
    of a node tensor in test_standalone_stage_modules_match_oracle (the read-out: ``bf16_tol`` of its logits).  Padded rows are exactly 0.

    ``RawFFN_w96`` is the case that found something.  The chain 28 -> 96 -> 96 -> 128 has no fused instance and runs as three
    ``k_gemm_bf16`` launches; with bf16 operands it was off by 4.27e-2 (max |raw_emb| 4.32), which the same chain in float64 with the
    operands of every Linear rounded to bf16 reproduces (4.274e-2): rounding that the GraphNormalization behind the chain amplifies.  The
    non-fused raw chain now takes f16 operands (``Lin::h16``, api.cpp); the float64 model with f16-rounded operands gives 6.45e-3 and
    the kernel measures 6.45e-3 on an MI355X."""
    from oracle import rnampnn_oracle as O
    from rnampnn.model.functional import RNABert, RawFFN, Readout
    s = _setup("h2_h16_w96")
    hp, ref, mask = s["hp"], s["runs"]["f64"], s["mask"]
    mt, m64 = torch.from_numpy(mask), torch.from_numpy(mask).double()
    sd64 = O.state_dict_from_numpy(s["sd"], torch.float64)
    cfg = O.OracleConfig(**{k: v for k, v in hp.items() if k in O.OracleConfig.__dataclass_fields__})
    L, P_len = hp["num_res_mpnn_layers"], hp["padding_len"]

    def load(mod, prefix):
        mod.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in s["sd"].items() if k.startswith(prefix)})
        return mod.to("cuda:0").eval()

    tol = BF16_STAGE_TOL
    with torch.no_grad():
        if stage.startswith("RNABert"):
            which, pre = ("post_fusion", "post_fusion.") if "heads16" in stage else ("embedding", "res_feature.res_embedding.")
            n_attn, heads, width, n_ffn = (hp[f"num_{which}_attn_layers"], hp[f"num_{which}_heads"], hp[f"{which}_ffn_dim"],
                                           hp[f"num_{which}_ffn_layers"])
            assert (heads, width) == ((16, 160) if "heads16" in stage else (2, 96))
            x = ref[f"h{L}"].float()
            got = load(RNABert(P_len, 128, n_attn, heads, width, n_ffn, precision="bf16"), pre)(x, mt)
            sd_stage = {"post_fusion." + k[len(pre):]: v for k, v in sd64.items() if k.startswith(pre)}
            want = O.rnabert(x.double(), m64, sd_stage, "post_fusion", n_attn, heads, n_ffn, P_len)
        elif stage == "RawFFN_w96":
            x = ref["raw"].float()
            got = load(RawFFN(28, hp["num_raw_ffn_dim"], hp["num_raw_ffn_layers"], 128, precision="bf16"), "raw_embedding.")(x, mt)
            want = O.raw_ffn(x.double(), m64, sd64, cfg)
        else:
            x = ref["embedding"].float()
            got = load(Readout(256, hp["readout_hidden_dim"], hp["num_readout_layers"], precision="bf16"), "readout.")(x, mt)
            want = O.readout(x.double(), m64, sd64, cfg)
            tol = bf16_tol(want, mask)
    got = got.cpu()
    err = float((got.double() - want).abs().max())
    print(f"\n{stage}: max |d| {err:.3e} (bound {tol:.1e}, max |value| {float(want.abs().max()):.2f})")
    assert torch.isfinite(got).all() and (got[mask == 0] == 0).all()
    assert err < tol


def _step(model, s, dropout, seed):
    loss, logits = model.loss_and_grad(torch.from_numpy(s["labels"]), torch.from_numpy(s["coords"]), torch.from_numpy(s["mask"]),
                                       return_logits=True, dropout=dropout, seed=seed)
    return float(loss), logits.cpu().double(), grad_dict(model)


TRAIN_RUNS = [(case, 0.0) for case in NS.CASES] + [(case, NS.DROPOUT) for case in NS.DROPOUT_CASES]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case, dropout", TRAIN_RUNS)
def test_trainer_matches_f64_oracle_autograd(case, dropout, precision):
    """``loss_and_grad`` of both trainers against fp64 oracle autograd, without dropout on every case and with dropout 0.4 (the oracle
    restating the library's masks; attention element = ((query row * heads + head) << 13) + key, so heads enters the index) on S1 and S2.
      f32         loss within F32_LOSS_TOL, logits within F32_LOGIT_TOL (2e-4 under dropout), every tensor within 2e-3 of its largest
                  reference entry or 1e-7 absolute, flat cosine > F32_COS, dead tensors below DEAD_ABS
      bf16-mixed  BF16_LOSS_TOL, ``bf16_tol``, BF16_GRAD_REL per tensor, BF16_COS, DEAD_ABS
    Under dropout two calls give bit-identical gradients and another seed another loss."""
    ref = s = _reference(case, dropout)
    model = _model_with(s["hp"], s["sd"], precision)
    assert model.train_precision == precision
    loss, logits, g = _step(model, s, dropout, NS.DROPOUT_SEED)
    valid = torch.from_numpy(s["mask"]).bool()
    dlogit = float((logits - ref["logits"])[valid].abs().max())
    rel, dead, cos = grad_errors(g, ref["grads"])
    absd = {k: float((g[k] - ref["grads"][k]).abs().max()) for k in rel}
    worst = max(rel, key=rel.get)
    print(f"\n{case} p={dropout} {precision}: |dloss| {abs(loss - ref['loss']):.2e}, max|dlogit| {dlogit:.2e}, worst per-tensor {rel[worst]:.2e} "
          f"({worst}, absolute {absd[worst]:.1e}), median {np.median(list(rel.values())):.2e}, cos 1-{1 - cos:.1e}, dead {dead:.1e}")
    assert all(torch.isfinite(v).all() for v in g.values())
    if precision == "f32":
        assert abs(loss - ref["loss"]) < F32_LOSS_TOL
        assert dlogit < (F32_DROPOUT_LOGIT_TOL if dropout > 0 else F32_LOGIT_TOL)
        bad = {k: (v, absd[k]) for k, v in rel.items() if not (v < F32_GRAD_REL or absd[k] < F32_GRAD_ABS)}
        assert not bad, bad
        assert cos > F32_COS
    else:
        assert abs(loss - ref["loss"]) < BF16_LOSS_TOL
        assert dlogit < bf16_tol(ref["logits"], s["mask"])
        assert cos > BF16_COS
    assert dead < DEAD_ABS
    if dropout > 0:
        loss2, _, g2 = _step(model, s, dropout, NS.DROPOUT_SEED)
        assert loss2 == loss and all(torch.equal(g2[k], g[k]) for k in g)
        loss3, _, _ = _step(model, s, dropout, NS.DROPOUT_SEED + 1)
        assert loss3 != loss
        eval_logits = _reference(case, 0.0)["logits"]
        assert float((ref["logits"] - eval_logits)[valid].abs().max()) > 1e-3            # the masks really act
    if precision == "bf16":
        over = sorted(((v, k) for k, v in rel.items() if v >= BF16_GRAD_REL), reverse=True)
        assert not over, over               # (no case needs test_train_parity_gpu's BF16_PER_TENSOR_OPEN convention: measured worst 8.7e-2)
