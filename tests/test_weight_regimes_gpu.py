"""The forward held to the oracle away from the closed-form weights: the bounds of test_mpnn_taps_gpu.py (``_check``, ``M_BF16``,
``F32_TAP_TOL``) and of test_hip_parity.py (``bf16_tol``), unchanged, at the regimes of ``_weight_regimes.REGIMES`` - GELU pre-activations
at and beyond the knee of the packed-f16 Phi forms, attention that picks keys (the running maximum of the online softmax moves between
key blocks), biases that are not small under the kGA / kGAn folding, separated logits - and the f16 range contract of DESIGN.md section 3.
test_weight_regimes_cpu.py pins, from the oracle alone, that each regime is where its name says and that the autocast yardstick is
conditioned (max ch, max row <= 0.1) on every tap asserted here.

Reference: the f64 oracle on the graph of the f32 oracle, which must equal the kernel's ``edge_index``.  Cases: ``_weight_regimes.CASES``."""
import numpy as np
import pytest
import torch

import _weight_regimes as W
from _tap_metrics import tap_error_padded
from _tap_oracle import swapped
from test_hip_parity import bf16_tol
from test_mpnn_taps_gpu import CONTROL_FACTOR, M_BF16, TAP_NAMES, _check, _model, _zero_outside

pytestmark = pytest.mark.gpu

NODE_TAPS = ["h_post", "raw_emb"]
F32_LOGIT_FLOOR = 2e-4


def _tensors(s):
    return torch.from_numpy(s["coords"]), torch.from_numpy(s["mask"])


def _check_node_outputs(label, precision, taps, runs, mask, failures):
    for key in NODE_TAPS:
        _check(label, precision, taps[key].cpu(), runs, key, mask, None, failures)


def _check_logits(label, precision, logits, runs, mask, argmax, failures):
    """f32: max(2e-4, 4 x |f32 oracle - f64 oracle|); bf16: ``bf16_tol`` of the f64 reference, and with ``argmax`` the same argmax on
    every valid row whose reference top-2 margin exceeds 2 x that tolerance."""
    ref = runs["f64"]["logits"]
    valid = torch.from_numpy(mask) > 0
    err = float((logits.double() - ref)[valid].abs().max())
    if precision == "f32":
        tol = max(F32_LOGIT_FLOOR, 4.0 * float((runs["f32"]["logits"].double() - ref)[valid].abs().max()))
    else:
        tol = bf16_tol(ref, mask)
    print(f"{label} logits {precision}: max |d| {err:.3e}  bound {tol:.3e}  (std of the reference {float(ref[valid].std()):.3f})")
    if not err <= tol:
        failures.append((label, "logits", "absmax", err, tol))
    if argmax and precision == "bf16":
        share, clear = W.left_out_share(ref, mask, tol)
        flips = int((logits.argmax(-1) != ref.argmax(-1))[clear].sum())
        print(f"{label} argmax: {flips} of {int(clear.sum())} rows with a clear margin differ ({share:.1%} of the valid rows left out)")
        assert share <= W.MAX_LEFT_OUT
        if flips:
            failures.append((label, "logits", "argmax flips", flips, 0))


def _run_pair(label, s, precision, fine, argmax, tap_names=None):
    """Every assertion of one (case, weights) setup at one precision -> list of misses."""
    hp, mask, runs = s["hp"], s["mask"], s["runs"]
    idx = runs["f32"]["edge_index"]
    c, m = _tensors(s)
    model = _model(hp, s["sd"], precision)
    failures = []
    pad = mask == 0
    print(f"\n{label}: k = {hp['num_res_neighbours']}, L = {hp['num_res_mpnn_layers']}, lens {s['lens']}, T = {mask.shape[1]}")
    for i, l in enumerate(s["layers"] if fine else (0,)):
        taps = model.forward_taps(c, m, (TAP_NAMES if fine else ["edge_index"]) + NODE_TAPS, tap_layer=l)
        assert torch.equal(taps["edge_index"].cpu(), idx), f"{label}: the kernel's graph is not the f32 oracle's"
        for key in NODE_TAPS + ["logits"]:
            v = taps[key].cpu().numpy()
            assert np.isfinite(v).all() and (v[pad] == 0).all(), f"{label}: {key} is not finite, or not 0 on a padded row"
        if fine:
            _zero_outside(taps, mask, idx)
            if i == 0:
                _check(label, precision, taps["h0"].cpu(), runs, "h0", mask, None, failures)
                _check(label, precision, taps["e0"].cpu(), runs, "e0", mask, idx, failures)
            runs_l = {p: {"h": r[f"h{l}"], "e": r[f"e{l}"]} for p, r in runs.items()}
            print(f"  layer {l}")
            _check(label, precision, taps["h_layer"].cpu(), runs_l, "h", mask, None, failures)
            _check(label, precision, taps["e_layer"].cpu(), runs_l, "e", mask, idx, failures)
        if i == 0:
            _check_node_outputs(label, precision, taps, runs, mask, failures)
    logits = model(c, m).cpu()                                   # the production launches, no tap
    assert bool(torch.isfinite(logits).all()) and bool((logits[torch.from_numpy(pad)] == 0).all())
    _check_logits(label, precision, logits, runs, mask, argmax, failures)
    return failures


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case,regime", W.PAIRS)
def test_regime_taps_and_logits_match_f64_oracle(case, regime, precision):
    s = W.setup(case, regime)
    failures = _run_pair(f"{case}_{regime}", s, precision, fine=regime != "all_mild", argmax=regime in W.ARGMAX_REGIMES)
    assert not failures, failures


def test_swapped_channels_fail_the_tap_bound_in_the_saturated_regime():
    """Negative control: case P x edge_saturated, a bf16 model with output channels 5 and 77 of layer 4's edge update exchanged
    (``_tap_oracle.swapped``) against the UNSWAPPED f64 oracle.  ``max ch`` of e4 must miss the bound 5-fold or more: saturation does not
    blunt the metric.  The model with the right weights passes it."""
    s = W.setup("P", "edge_saturated")
    hp, mask, runs = s["hp"], s["mask"], s["runs"]
    idx = runs["f32"]["edge_index"]
    c, m = _tensors(s)
    A = tap_error_padded(runs["autocast"]["e4"], runs["f64"]["e4"], mask, idx)
    bad = _model(hp, swapped(s["sd"], hp), "bf16").forward_taps(c, m, ["e_layer"], tap_layer=4)
    K = tap_error_padded(bad["e_layer"].cpu(), runs["f64"]["e4"], mask, idx)
    good = _model(hp, s["sd"], "bf16").forward_taps(c, m, ["e_layer"], tap_layer=4)
    G = tap_error_padded(good["e_layer"].cpu(), runs["f64"]["e4"], mask, idx)
    print(f"\ne4 swapped : {K}\ne4 right   : {G}\ne4 autocast: {A}\nswapped / bound: {K.max_ch / (M_BF16 * A.max_ch):.1f}")
    assert K.ch_ok and K.worst_ch in (5, 77)
    assert K.max_ch >= CONTROL_FACTOR * M_BF16 * A.max_ch
    assert G.max_ch <= M_BF16 * A.max_ch


# ------------------------------------------------------------------------------------------------ the f16 range contract
def _per_rna_finite_and_right_or_not_finite(label, logits, ref, mask, tol):
    """bf16 beyond the f16 range: per RNA, every valid row within ``tol`` of the reference, or a non-finite value among its valid rows.
    -> the list of RNAs that came out non-finite."""
    out = []
    for b in range(mask.shape[0]):
        rows = torch.from_numpy(mask[b]) > 0
        got = logits[b][rows].double()
        if not bool(torch.isfinite(got).all()):
            out.append(b)
            continue
        err = float((got - ref[b][rows]).abs().max())
        print(f"{label} RNA {b}: finite, max |d| {err:.3e} (bound {tol:.3e})")
        assert err <= tol, f"{label}: RNA {b} is finite and wrong by {err:.3e} (bound {tol:.3e})"
    print(f"{label}: non-finite RNAs {out}")
    return out


def test_range_contract_weights_driven_f32():
    """Case Q at L = 10, edge gain 8: |e| passes 65504 / a within three layers and reaches 1e11.  The f32 path holds its usual bounds, which are
    relative to the f32 oracle's own distance to the f64 oracle."""
    s = W.setup("Q_L10", "edge_overflow", modes=("f32", "f64"))
    failures = _run_pair("Q_L10_edge_overflow", s, "f32", fine=True, argmax=False)
    assert not failures, failures


def test_range_contract_weights_driven_bf16():
    """The same batch through the bf16 path, whose e is f16 of a e: per RNA right within ``bf16_tol`` or visibly non-finite, never finite
    and wrong; the call returns without an error and padded logits stay exactly 0."""
    s = W.setup("Q_L10", "edge_overflow", modes=("f32", "f64"))
    c, m = _tensors(s)
    logits = _model(s["hp"], s["sd"], "bf16")(c, m).cpu()
    assert bool((logits[torch.from_numpy(s["mask"] == 0)] == 0).all())
    ref = s["runs"]["f64"]["logits"]
    _per_rna_finite_and_right_or_not_finite("\nQ_L10_edge_overflow bf16", logits, ref, s["mask"], bf16_tol(ref, s["mask"]))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_range_contract_coordinates_of_one_rna(precision):
    """Case P at the closed-form weights with the coordinates of RNA 1 x 1e5: its cross distances - MFMA operands of the bf16 edge embedding,
    in f16 - exceed 65504 (``_weight_regimes.scaled_graph_note`` for the graph).  bf16: RNAs 0, 2 and 3 are bit-identical to the batch with
    RNA 1 unscaled (the isolation form of test_isolation_gpu.py) and RNA 1 is right or non-finite.  f32: the usual bounds on all four."""
    s = W.setup("P", "closed_form", scale_rna=(1, 1e5))
    base = W.setup("P", "closed_form", modes=("f32",))
    mask = s["mask"]
    c, m = _tensors(s)
    model = _model(s["hp"], s["sd"], precision)
    out = model.forward_taps(c, m, ["edge_index"])
    assert torch.equal(out["edge_index"].cpu(), s["runs"]["f32"]["edge_index"]), "the kernel's graph is not that of the unscaled batch"
    logits = out["logits"].cpu()
    assert bool((logits[torch.from_numpy(mask == 0)] == 0).all())
    ref = s["runs"]["f64"]["logits"]
    if precision == "f32":
        failures = _run_pair("P_rna1_x1e5", s, "f32", fine=True, argmax=False)
        assert not failures, failures
        return
    clean = model(torch.from_numpy(base["coords"]), m).cpu()
    for b in (0, 2, 3):
        assert logits[b].numpy().tobytes() == clean[b].numpy().tobytes(), f"RNA {b} moved with the coordinates of RNA 1"
    bad = _per_rna_finite_and_right_or_not_finite("\nP_rna1_x1e5 bf16", logits, ref, mask, bf16_tol(ref, mask))
    assert set(bad) <= {1}
