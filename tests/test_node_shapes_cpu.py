"""The yardstick of test_node_shapes_gpu.py, checked without a device: the oracle's attention at every head count against torch's own
``nn.MultiheadAttention``, the schema of the four cases of ``_node_shape_cases``, and controls that show, oracle against oracle in
float64, that the bounds the device tests import are fine enough to see a wrong head count or a dropped K / N tail at these shapes."""
import numpy as np
import pytest
import torch

import _node_shape_cases as NS
from oracle import rnampnn_oracle as O
from test_hip_parity import F32_LOGIT_TOL, bf16_tol
from test_train_parity_gpu import grad_errors, oracle_loss_and_grad

F32_GRAD_REL, F32_GRAD_ABS = 2e-3, 1e-7          # the per-tensor rule of test_loss_and_gradients_match_oracle_autograd
CONTROL_FACTOR = 5.0


@pytest.mark.parametrize("heads", [2, 4, 8, 16])
def test_oracle_attention_matches_torch_multihead_attention(heads):
    """``O.rnabert`` with one attention layer, float64, lengths [37, 5, 1, 70] padded to T = 70 at padding_len = 80, against the same
    stage composed of torch's modules the way the reference's RNABert.forward composes them (functional.py:161-172): zero-pad to
    padding_len, x += MultiheadAttention(x, x, x, key_padding_mask = ~mask), GraphNormalization over the padded axis, the FFN, mask, cut
    back to T.  ``nn.MultiheadAttention(128, heads, batch_first=True)`` carries the same weights, so the head split, the 1 / sqrt(head dim)
    and the key mask of the oracle are pinned to torch at head dims 64, 32, 16 and 8.  Valid rows agree to 1e-12."""
    from rnampnn.model._schema import D, _bert
    from rnampnn.utils import synth
    lens, P, n_ffn, ffn = NS.LENS, 80, 2, 96
    T = max(lens)
    shapes = {}
    _bert(shapes, "post_fusion", 1, ffn, n_ffn)
    sd = O.state_dict_from_numpy(synth.closed_form_state_dict(shapes), torch.float64)
    sd["post_fusion.bi_attention_layers.0.in_proj_weight"] *= 3.0           # away from a uniform attention
    g = torch.Generator().manual_seed(heads)
    mask = torch.zeros(len(lens), T, dtype=torch.float64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    h = torch.randn(len(lens), T, D, generator=g, dtype=torch.float64) * mask.unsqueeze(-1)
    with torch.no_grad():
        got = O.rnabert(h, mask, sd, "post_fusion", 1, heads, n_ffn, P)

    mha = torch.nn.MultiheadAttention(D, heads, batch_first=True).double()
    p = "post_fusion.bi_attention_layers.0."
    mha.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
    ffn_mod = torch.nn.Sequential(*[torch.nn.Linear(D if i == 0 else ffn, ffn) if j == 0 else torch.nn.GELU() if j == 1 else torch.nn.Identity()
                                    for i in range(n_ffn) for j in range(3)], torch.nn.Linear(ffn, D)).double()
    ffn_mod.load_state_dict({k[len("post_fusion.ffn_layers."):]: v for k, v in sd.items() if k.startswith("post_fusion.ffn_layers.")})
    with torch.no_grad():
        x = torch.cat([h, torch.zeros(len(lens), P - T, D, dtype=torch.float64)], 1)
        pm = torch.cat([mask, torch.zeros(len(lens), P - T, dtype=torch.float64)], 1)
        x = x + mha(query=x, key=x, value=x, key_padding_mask=~pm.bool())[0]
        x = O.graph_norm(x, pm, sd["post_fusion.graph_norm_layers.0.scale"], sd["post_fusion.graph_norm_layers.0.shift"])
        want = (ffn_mod(x) * pm.unsqueeze(-1))[:, :T]
    valid = mask.bool()
    err = float((got - want)[valid].abs().max())
    other = float((got - O.rnabert(h, mask, sd, "post_fusion", 1, 8 if heads != 8 else 4, n_ffn, P))[valid].abs().max())
    print(f"heads {heads}: max |oracle - torch| on valid rows {err:.2e} (max |value| {float(want[valid].abs().max()):.2f}); another head count moves it by {other:.2e}")
    assert err < 1e-12
    assert (got[~valid] == 0).all()
    assert other > 1e-6                                 # the comparison depends on the head count


@pytest.mark.parametrize("case", NS.CASES)
def test_schema_matches_the_module(case):
    """``state_dict_shapes(hp)`` - what the closed-form weights of every case are made from - names the keys, the order and the shapes of
    ``RNAMPNN(**hp).state_dict()``, in both precisions, and the C library registers the same list."""
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    from rnampnn.model._schema import DEFAULT_HPARAMS, state_dict_shapes
    from rnampnn.model.rnampnn import RNAMPNN
    hp = NS.hparams(case)
    shapes = state_dict_shapes(hp)
    for precision in ("f32", "bf16"):
        model = RNAMPNN(precision=precision, **{k: v for k, v in hp.items() if k in DEFAULT_HPARAMS})
        mine = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        assert list(mine) == list(shapes) and mine == {k: tuple(v) for k, v in shapes.items()}, precision
    h = _native.Handle(hp, _native.PREC_BF16)
    assert [(k, n) for k, n in h.weight_schema()] == [(k, int(np.prod(s))) for k, s in shapes.items()]
    h.close()


@pytest.mark.parametrize("case", list(NS.GOLDEN_NAMES))
def test_reference_fixture_is_the_case_of_the_table(golden, case):
    """The two reference-made fixtures hold the hyper-parameters, the batch and the state-dict schema of cases S1 and S2."""
    from rnampnn.model._schema import state_dict_shapes
    arrs, hp, shapes = golden(NS.GOLDEN_NAMES[case])
    mine = NS.hparams(case)
    assert all(mine[k] == v for k, v in hp.items())
    assert {k: tuple(v) for k, v in state_dict_shapes(mine).items()} == shapes and list(state_dict_shapes(mine)) == list(shapes)
    coords, mask, labels = NS.batch()
    assert np.array_equal(arrs["coords"], coords) and np.array_equal(arrs["mask"], mask) and np.array_equal(arrs["labels"], labels)
    assert mask.shape == (4, 70) and mask.sum(1).tolist() == NS.LENS
    for key in ("raw", "h0", "h1", "hL", "h_post", "raw_emb", "e0", "e1", "edge_raw", "logits", "logits_f64"):      # full=True
        assert key in arrs, key


CONTROL_LINEAR = "raw_embedding.raw_ffn.3"          # S1: Linear(96 -> 96), the second hidden Linear of the raw chain


def _controls(hp, sd):
    """-> {name: (hp, sd)} of the three wrong models of S1."""
    w, b = sd[CONTROL_LINEAR + ".weight"], sd[CONTROL_LINEAR + ".bias"]
    assert w.shape == (96, 96)
    k_tail, n_tail, n_bias = w.copy(), w.copy(), b.copy()
    k_tail[:, 64:] = 0.0                                # the last, half-empty K tile never accumulated
    n_tail[64:] = 0.0                                   # the output columns past the last full 64-wide tile never written
    n_bias[64:] = 0.0
    return {"heads_swapped": (dict(hp, num_embedding_heads=hp["num_post_fusion_heads"], num_post_fusion_heads=hp["num_embedding_heads"]), sd),
            "k_tail_dropped": (hp, dict(sd, **{CONTROL_LINEAR + ".weight": k_tail})),
            "n_tail_dropped": (hp, dict(sd, **{CONTROL_LINEAR + ".weight": n_tail, CONTROL_LINEAR + ".bias": n_bias}))}


def test_bounds_resolve_the_faults():
    """Oracle against oracle in float64 on case S1: the model with (a) the two head counts exchanged, (b) input columns 64..95 of
    ``raw_embedding.raw_ffn.3`` (96 -> 96) zeroed - a dropped K tail - and (c) its output columns 64..95 zeroed, against the right one,
    each bound at the weights the device tests assert it at.  At the forward weights (``NS.GAINS``) each must miss F32_LOGIT_TOL by more
    than 5 x, and (a) and (b) must miss ``bf16_tol`` on the logits.  At the trainer weights (plain closed form) each must miss
    F32_LOGIT_TOL by more than 5 x and, in at least one parameter, the f32 per-tensor gradient rule (2e-3 of the tensor's largest entry
    and 1e-7 absolute) by more than 5 x; the share of BF16_GRAD_REL is printed.

    Measured                   forward weights                       trainer weights
                       / F32_LOGIT_TOL  / bf16_tol    / F32_LOGIT_TOL   gradient: / 2e-3, / 1e-7, / BF16_GRAD_REL   (tensor)
      heads_swapped      1155 x          3.85 x         19 x             394 x   8.4e2 x   9.8 x    (res_feature.res_embedding.bi_attention_layers.0.out_proj.weight)
      k_tail_dropped     16579 x         55.3 x         3777 x           514 x   2.0e4 x   8.6 x    (raw_embedding.raw_ffn.6.bias)
      n_tail_dropped     12037 x         40.1 x         2473 x           921 x   3.6e4 x   15.3 x   (raw_embedding.raw_ffn.6.bias)
    (the gradient columns: the tensor that misses both halves of the f32 rule by most; / BF16_GRAD_REL: the worst tensor)
    (a) at the plain closed-form weights moves the logits by 1.9e-3 = 0.06 x bf16_tol: the attention there is nearly uniform, which is
    why the forward tests of S1 carry gains on the attention projections and the read-out."""
    from test_hip_parity import BF16_GRAD_REL
    coords, mask, labels = NS.batch()
    valid = torch.from_numpy(mask).bool()
    for train in (False, True):
        hp, sd = NS.state_dict("h2_h16_w96", train=train)
        _, logits, grads = oracle_loss_and_grad(hp, sd, coords, mask, labels)
        tol16 = bf16_tol(logits, mask)
        for name, (hp2, sd2) in _controls(hp, sd).items():
            _, z, g = oracle_loss_and_grad(hp2, sd2, coords, mask, labels)
            dlogit = float((z - logits)[valid].abs().max())
            print(f"{'trainer' if train else 'forward'} weights, {name}: max |dlogit| {dlogit:.3e} = {dlogit / F32_LOGIT_TOL:.0f} x F32_LOGIT_TOL, "
                  f"{dlogit / tol16:.2f} x bf16_tol ({tol16:.2e})")
            assert dlogit > CONTROL_FACTOR * F32_LOGIT_TOL, name
            if not train:
                if name != "n_tail_dropped":
                    assert dlogit > tol16, name
                continue
            rel, _, _ = grad_errors(g, grads)
            moved = {k: (v, float((g[k] - grads[k]).abs().max())) for k, v in rel.items()}
            key = max(moved, key=lambda k: min(moved[k][0] / F32_GRAD_REL, moved[k][1] / F32_GRAD_ABS))
            print(f"    gradient of {key}: {moved[key][0]:.3e} of its largest entry = {moved[key][0] / F32_GRAD_REL:.0f} x the f32 rule, absolute "
                  f"{moved[key][1]:.2e} = {moved[key][1] / F32_GRAD_ABS:.1e} x; worst tensor {max(rel.values()) / BF16_GRAD_REL:.1f} x BF16_GRAD_REL")
            assert moved[key][0] > CONTROL_FACTOR * F32_GRAD_REL and moved[key][1] > CONTROL_FACTOR * F32_GRAD_ABS, name
