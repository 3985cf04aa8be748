"""The k-NN tie class on the device (tests/golden/rnampnn_ties/; the class and its logit gap: test_knn_ties_cpu.py, ``O.knn_graph``).

The full model names the phantom neighbour in slot n - 1 of every row of an RNA with n - 1 < k and T > n, where the reference's tie-break
leaves -1 in part of the rows when 1 <= T - n <= 2.  So (a) its ``edge_index`` tap is in the class of the reference's graph and its logits
match the oracle on the kernel's own graph, and (b) everything behind the graph is held to the reference's golden logits all the same:
the pipeline composed from the stand-alone stage modules, with slot n - 1 of the graph overwritten with the reference's value between
``ResFeature`` and the first ``ResMPNN`` (a caller's -1 means "no edge" to every stage), must reproduce them."""
import numpy as np
import pytest
import torch

from _tap_metrics import tap_error_padded
from _tap_oracle import TIE_FIXTURES, load_fixture, oracle_config, run_oracle
from test_hip_parity import F32_LOGIT_TOL, bf16_tol
from test_mpnn_taps_gpu import M_BF16

pytestmark = pytest.mark.gpu


def _load(mod, sd, prefix):
    mod.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(prefix)})
    return mod.to("cuda:0").eval()


def _staged(hp, sd, coords, mask, ref_idx, precision):
    """ResFeature -> slot n - 1 of the graph from the reference -> L x ResMPNN -> RNABert -> RawFFN -> Readout, the weights of the one
    state dict split by prefix -> (logits, hL, the graph the layers ran on)."""
    from rnampnn.model.feature import ResFeature
    from rnampnn.model.functional import RNABert, RawFFN, Readout
    from rnampnn.model.mpnn import ResMPNN
    k, L, P = int(hp["num_res_neighbours"]), int(hp["num_res_mpnn_layers"]), int(hp["padding_len"])
    feat = _load(ResFeature(num_neighbours=k, padding_len=P, num_attn_layers=hp["num_embedding_attn_layers"],
                            num_heads=hp["num_embedding_heads"], ffn_dim=hp["embedding_ffn_dim"], num_ffn_layers=hp["num_embedding_ffn_layers"],
                            num_edge_layers=hp["depth_res_edge_feature"], precision=precision), sd, "res_feature.")
    raw, h, e, idx = feat(coords, mask)
    idx = idx.clone()
    n = mask.sum(-1).long()
    for b in range(mask.shape[0]):
        nb = int(n[b])
        if 1 <= nb < mask.shape[1] and nb - 1 < k:
            idx[b, :nb, nb - 1] = ref_idx[b, :nb, nb - 1].to(idx.device)
    for l in range(L):
        layer = _load(ResMPNN(128, 128, hp["depth_res_mpnn"], hp["num_mpnn_edge_layers"], 0.4, precision=precision), sd, f"res_mpnn_layers.{l}.")
        h, e = layer(h, e, idx, mask)
    bert = _load(RNABert(padding_len=P, res_embedding_dim=128, num_attn_layers=hp["num_post_fusion_attn_layers"],
                         num_heads=hp["num_post_fusion_heads"], ffn_dim=hp["post_fusion_ffn_dim"],
                         num_ffn_layers=hp["num_post_fusion_ffn_layers"], precision=precision), sd, "post_fusion.")
    rawffn = _load(RawFFN(28, hp["num_raw_ffn_dim"], hp["num_raw_ffn_layers"], hp["raw_embedding_dim"], precision=precision), sd, "raw_embedding.")
    ro = _load(Readout(256, hp["readout_hidden_dim"], hp["num_readout_layers"], precision=precision), sd, "readout.")
    logits = ro(torch.cat([bert(h, mask), rawffn(raw, mask)], -1), mask)
    return logits.cpu(), h.cpu(), idx.cpu()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_tie_fixture(name, precision):
    from oracle import rnampnn_oracle as O
    from rnampnn.utils import synth
    from test_hip_parity import _model
    arrs, hp, shapes = load_fixture("rnampnn_ties", name)
    k, L = int(hp["num_res_neighbours"]), int(hp["num_res_mpnn_layers"])
    coords, mask = torch.from_numpy(arrs["coords"]), torch.from_numpy(arrs["mask"])
    ref_idx = torch.from_numpy(arrs["edge_index"]).long()
    valid = mask.bool()

    # (a) the full model: its graph is in the class, its logits are the oracle's on that graph
    model, sd = _model(hp, shapes, precision)
    out = model.forward_taps(coords, mask, ["edge_index"])
    own_idx, logits = out["edge_index"].cpu(), out["logits"].cpu()
    assert O.edge_index_in_class(ref_idx, own_idx, mask, k)
    assert torch.equal(own_idx, O.knn_graph(coords, mask, k))
    assert int(((own_idx != O.canonical_edge_index(ref_idx, mask)).sum())) > 0          # the fixture exercises the regime
    on_own = run_oracle(hp, sd, coords, mask, "f32", edge_index=own_idx)["logits"]
    tol = F32_LOGIT_TOL if precision == "f32" else bf16_tol(arrs["logits"], arrs["mask"])
    err_own = float((logits - on_own).abs().max())
    gap = float((logits - torch.from_numpy(arrs["logits"])).abs().max())
    print(f"\n{name} {precision}: full model vs oracle on its own graph {err_own:.2e} (bound {tol:.1e}); vs the reference's logits {gap:.2e} (the class gap)")
    assert err_own < tol

    # (b) the stages on the reference's graph against the reference's golden logits
    s_logits, s_hL, s_idx = _staged(hp, sd, coords, mask, ref_idx, precision)
    assert torch.equal(O.canonical_edge_index(s_idx, mask), O.canonical_edge_index(ref_idx, mask))
    err = float((s_logits - torch.from_numpy(arrs["logits"])).abs().max())
    K = tap_error_padded(s_hL, arrs["hL"], arrs["mask"])
    print(f"{name} {precision}: stages on the reference's graph vs reference: max |dlogit| {err:.2e} (bound {tol:.1e}); hL {K}")
    assert (s_logits[~valid] == 0).all() and (s_hL[~valid] == 0).all()
    assert err < tol
    if precision == "f32":
        assert K.absmax < 2e-4
    else:
        auto = run_oracle(hp, sd, coords, mask, "autocast", edge_index=O.canonical_edge_index(ref_idx, mask))[f"h{L}"]
        A = tap_error_padded(auto, arrs["hL"], arrs["mask"])
        print(f"{name} bf16: hL autocast {A}; kernel / autocast: row {K.max_row / A.max_row:.2f} absmax {K.absmax / A.absmax:.2f}")
        assert K.max_row <= M_BF16 * A.max_row and K.absmax <= M_BF16 * A.absmax
