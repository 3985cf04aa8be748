"""Every regime of ``_weight_regimes.REGIMES`` pinned to what its name claims, from the oracle alone (no GPU), so that a later edit of
the gains cannot quietly return test_weight_regimes_gpu.py to the closed-form corner - and the conditions that file relies on: f16
headroom of a e, a conditioned autocast yardstick on every tap it asserts, and enough rows with a clear top-2 margin for its argmax check.

"Site" = one GELU of the oracle, named by the Linear in front of it; shares are over valid rows (node sites) / valid slots (edge sites)
of pre-activations with |x| > sqrt(9.5), the knee of the packed-f16 Phi forms of csrc/bf16_dev.h."""
import numpy as np
import pytest
import torch

import _weight_regimes as W
from _tap_metrics import tap_error_padded
from _tap_oracle import closed_form_sd
from test_hip_parity import bf16_tol


def _shares(sites):
    return np.array([v[0] for v in sites.values()])


def test_closed_form_control_sits_in_the_corner():
    st = W.stats_of("P", "closed_form")
    second = W.edge_sites(st, 3)
    assert len(second) == 20 and len(W.edge_sites(st, 0)) == 20
    print("\nclosed form: first Linears", _shares(W.edge_sites(st, 0)).round(4), "attention", st["attention"])
    assert (_shares(second) == 0.0).all()
    assert len(st["attention"]) == 2 and max(st["attention"]) <= 0.1
    assert max(W.stats_of("R", "closed_form")["attention"]) <= 0.1
    assert float(st["logits"][torch.from_numpy(W.setup("P", "closed_form", modes=("f32",))["mask"]) > 0].std()) < 0.2


def test_edge_knee_has_every_edge_site_between_2_and_40_per_cent():
    sh = _shares(W.edge_sites(W.stats_of("P", "edge_knee"), None))
    print(f"\nedge_knee: {sh.min():.4f} .. {sh.max():.4f} over {sh.size} sites")
    assert sh.size == 40 and sh.min() >= 0.02 and sh.max() <= 0.40


@pytest.mark.parametrize("case,least", [("P", 0.25), ("Q", 0.20)])
def test_edge_saturated_has_every_edge_site_at_25_per_cent_or_more(case, least):
    """The regime's claim is stated on case P.  Case Q (k = 16, three layers: |e| has grown less) carries it to k_mpnn_bf16 and is held to
    20 %, two orders of magnitude above the closed-form control (<= 0.7 % in a first Linear, 0 in a second)."""
    sh = _shares(W.edge_sites(W.stats_of(case, "edge_saturated"), None))
    print(f"\n{case} edge_saturated: {sh.min():.4f} .. {sh.max():.4f} over {sh.size} sites")
    assert sh.size == 4 * W.CASES[case][1] and sh.min() >= least


@pytest.mark.parametrize("case", ["P", "R"])
def test_attention_peaked_has_a_mean_largest_probability_of_0_3_or_more(case):
    att = W.stats_of(case, "attention_peaked")["attention"]
    print(f"\n{case} attention_peaked: {att}")
    assert len(att) == 2 and min(att) >= 0.3


@pytest.mark.parametrize("case", ["P", "R"])
def test_node_chains_saturate_the_post_fusion_ffn_and_the_read_out_and_separate_the_logits(case):
    st = W.stats_of(case, "node_chains")
    sites = {k: v for k, v in st["gelu"].items() if k.startswith("post_fusion.ffn_layers") or k == "readout.readout_layers.0"}
    print(f"\n{case} node_chains:", {k: round(v[0], 3) for k, v in sites.items()})
    assert len(sites) == 4 and min(v[0] for v in sites.values()) >= 0.05
    assert float(st["logits"][torch.from_numpy(W.setup(case, "node_chains")["mask"]) > 0].std()) >= 2.0


@pytest.mark.parametrize("case,regime", W.PAIRS)
def test_f16_headroom_of_the_scaled_edge_tensor(case, regime):
    assert regime in W.IN_ENVELOPE
    st = W.stats_of(case, regime)
    print(f"\n{case} x {regime}: max |a e_l| = {max(st['ae_max']):.1f} (bound {W.F16_MAX / 64:.0f})")
    assert st["finite"] and max(st["ae_max"]) <= W.F16_MAX / 64


@pytest.mark.parametrize("case,regime", W.PAIRS)
def test_autocast_yardstick_is_conditioned_on_every_asserted_tap(case, regime):
    s = W.setup(case, regime)
    runs, mask = s["runs"], s["mask"]
    idx = runs["f32"]["edge_index"]
    worst = 0.0
    for name, is_edge in W.asserted_taps(case, regime):
        A = tap_error_padded(runs["autocast"][name], runs["f64"][name], mask, idx if is_edge else None)
        worst = max(worst, A.max_ch, A.max_row)
        assert A.max_ch <= 0.1 and A.max_row <= 0.1, (name, A.max_ch, A.max_row)
    print(f"\n{case} x {regime}: worst yardstick figure {worst:.3e}")


@pytest.mark.parametrize("case,regime", [p for p in W.PAIRS if p[1] in W.ARGMAX_REGIMES])
def test_argmax_check_leaves_out_a_quarter_of_the_rows_at_most(case, regime):
    s = W.setup(case, regime)
    ref = s["runs"]["f64"]["logits"]
    tol = bf16_tol(ref, s["mask"])
    share, _ = W.left_out_share(ref, s["mask"], tol)
    print(f"\n{case} x {regime}: bf16_tol {tol:.3f}, {share:.1%} of the valid rows have a top-2 margin <= 2 tol")
    assert share <= W.MAX_LEFT_OUT


def test_scaled_sd_identity_and_unknown_substring():
    from rnampnn.model._schema import DEFAULT_HPARAMS
    sd, _ = closed_form_sd(dict(DEFAULT_HPARAMS, num_res_neighbours=16, num_res_mpnn_layers=2, padding_len=40))
    one = W.scaled_sd(sd, {k: 1.0 for g in W.REGIMES.values() for k in g})
    assert list(one) == list(sd)
    for k in sd:
        assert one[k].dtype == np.float32 and one[k].tobytes() == np.asarray(sd[k], np.float32).tobytes(), k
    two = W.scaled_sd(sd, {"in_proj": 3.0})
    moved = [k for k in sd if two[k].tobytes() != one[k].tobytes()]
    assert moved and all("in_proj_weight" in k or "in_proj_bias" in k for k in moved) and len(moved) == 4
    gn = W.scaled_sd(sd, {"res_mpnn_layers": 2.0})            # the substring matches the layers' GraphNorm keys too
    assert all(gn[k].tobytes() == one[k].tobytes() for k in sd if k.endswith("scale") or k.endswith("shift"))
    with pytest.raises(KeyError):
        W.scaled_sd(sd, {"no_such_layer": 2.0})
    with pytest.raises(KeyError):
        W.scaled_sd(sd, {"graph_norm": 2.0})                  # only scale / shift carry it: never touched, so nothing matches


# ------------------------------------------------------------------------------------------------ the f16 range contract, oracle side
def test_overflow_regime_is_finite_in_f32_and_far_beyond_the_f16_range():
    """Case Q at L = 10 with the edge gain at 8: the f32 oracle stays finite while |a e| passes 65504 a thousandfold."""
    st = W.stats_of("Q_L10", "edge_overflow")
    print("\nmax |a e_l|:", ["%.3g" % v for v in st["ae_max"]])
    assert st["finite"]
    assert max(st["ae_max"]) >= 1e3 * W.F16_MAX
    assert sum(v > W.F16_MAX for v in st["ae_max"][:-1]) >= 3          # e_L is never read: several READ layers are beyond the range


def test_scaled_coordinates_put_every_distance_of_that_rna_beyond_the_f16_range():
    """Case P, closed form, RNA 1 x 1e5, on the graph of the unscaled batch (``_weight_regimes.scaled_graph_note``): 48 or all of the 49
    cross distances of each of its edges exceed 65504, the f32 oracle stays finite and the other RNAs do not move.  The oracle's OWN search differs on
    RNA 1 there and nowhere else: the reference's mask value of 1e6 ranks in front of real residues."""
    from oracle import rnampnn_oracle as O
    base = W.setup("P", "closed_form", modes=("f32",))
    s = W.setup("P", "closed_form", scale_rna=(1, 1e5), modes=("f32",))
    idx = s["runs"]["f32"]["edge_index"]
    assert torch.equal(idx, base["runs"]["f32"]["edge_index"])
    c, m = torch.from_numpy(s["coords"]), torch.from_numpy(s["mask"])
    own = O.knn_graph(c, m, 30)
    assert [bool(torch.equal(own[b], idx[b])) for b in range(4)] == [True, False, True, True]
    d = O.edge_raw_features(c, m, idx)[1, ..., :49]
    ok = (m[1] > 0).unsqueeze(-1) & (idx[1] != -1) & (idx[1] < int(m[1].sum()))           # the phantom neighbour sits at the origin
    beyond = d[ok] > W.F16_MAX                 # all but 2 of 54,390 (two atom pairs 0.46 A apart): every edge has 48 or 49 of its 49 out of range
    assert int(beyond.sum(-1).min()) >= 48 and float(beyond.float().mean()) > 0.9999
    lg = s["runs"]["f32"]["logits"]
    assert bool(torch.isfinite(lg).all())
    for b in (0, 2, 3):
        assert torch.equal(lg[b], base["runs"]["f32"]["logits"][b])
