"""Off-default node-side shapes: one table for tools/gen_golden.py (group ``shapes``), test_node_shapes_cpu.py and
test_node_shapes_gpu.py.

Every case runs k = 6, two ResMPNN layers, depth-2 edge / message MLPs (the bf16 library needs them) on the lengths
[37, 5, 1, 70] at padding_len = 80: T = 70 > 64 gives the attention kernels a second, ragged 64-key chunk and a second query block,
n = 1 has no edge at all and n = 5 < k the phantom neighbour.  Weights: the closed-form state dict (S1's forward tests: x ``GAINS``).

  S1 h2_h16_w96    heads 2 (embedding) and 16 (post-fusion); widths 96 / 160 / 96 / 96: K = 32 (mod 64) in every GEMM behind a hidden layer
                   and N no multiple of 64 in the ones in front of it
  S2 h16_h4_w32    heads 16 and 4, two post-fusion attention layers; every width 32, one hidden Linear each, a one-Linear read-out
  S3 w2048_deep    no embedding attention; a 5-Linear chain at width 2048 (above the fused limit), a 512-wide chain of 3 Linears and a
                   2-Linear raw chain at K0 = 32 (the right form, no fused instance), a 3-Linear read-out at width 544 (= 32 mod 64, no
                   multiple of 128)
  S4 no_attention  no attention layer at all, which makes head counts 3 and 5 legal; width 64, FFN depths 1 / 3 / 3

This module imports nothing of the package at import time: tools/gen_golden.py loads it by path next to the reference's ``rnampnn``.
"""
LENS = [37, 5, 1, 70]
FIRST_INDEX = 1300
COMMON = dict(num_res_neighbours=6, num_res_mpnn_layers=2, depth_res_edge_feature=2, depth_res_mpnn=2, num_mpnn_edge_layers=2, padding_len=80)


def _case(emb_attn, emb_heads, post_attn, post_heads, widths, depths):
    (w_emb, w_post, w_raw, w_ro), (n_emb, n_post, n_raw, n_ro) = widths, depths
    return dict(COMMON, num_embedding_attn_layers=emb_attn, num_embedding_heads=emb_heads, num_post_fusion_attn_layers=post_attn,
                num_post_fusion_heads=post_heads, embedding_ffn_dim=w_emb, post_fusion_ffn_dim=w_post, num_raw_ffn_dim=w_raw,
                readout_hidden_dim=w_ro, num_embedding_ffn_layers=n_emb, num_post_fusion_ffn_layers=n_post, num_raw_ffn_layers=n_raw,
                num_readout_layers=n_ro)


# name -> the hyper-parameters that differ from the defaults
OVERRIDES = {
    "h2_h16_w96": _case(1, 2, 1, 16, (96, 160, 96, 96), (2, 2, 2, 2)),
    "h16_h4_w32": _case(1, 16, 2, 4, (32, 32, 32, 32), (1, 1, 1, 1)),
    "w2048_deep": _case(0, 8, 2, 8, (2048, 512, 512, 544), (4, 2, 1, 3)),
    "no_attention": _case(0, 3, 0, 5, (64, 64, 64, 64), (1, 3, 3, 2)),
}
CASES = list(OVERRIDES)
GOLDEN_NAMES = {"h2_h16_w96": "shapes_h2_h16_w96", "h16_h4_w32": "shapes_h16_h4_w32"}       # the fixtures made from the reference's modules
# Forward tests of S1: gains on the closed-form weights AND biases of the keys that contain the substring (``_weight_regimes.scaled_sd``).
# At the plain closed-form weights the attention is nearly uniform: S1 with its two head counts exchanged moves the fp64 logits by
# 1.9e-3, 0.06 x the bf16 logit bound, so no bf16 logit test could tell the head counts apart; with these gains it moves them by 3.9 x
# that bound.  The trainer tests keep the plain closed form: the gradient tells the head counts apart there (a tensor moves by 1.2 of its
# largest entry), while under the gains it is too ill-conditioned to be a yardstick of a bf16 trainer - rounding the WEIGHTS alone to
# bf16 moves the fp64 gradient to a flat cosine of 1 - 2.6e-3, past BF16_COS, and 35 tensors by more than BF16_GRAD_REL (plain: 1 - 2.5e-5,
# worst tensor 0.099).  test_node_shapes_cpu.py::test_bounds_resolve_the_faults holds each bound to the weights it is asserted at.  The
# reference-made fixture of S1 is at the plain closed form.
GAINS = {"h2_h16_w96": {"in_proj": 3.0, "out_proj": 3.0, "readout": 2.0}}
DROPOUT_CASES = ["h2_h16_w96", "h16_h4_w32"]
DROPOUT, DROPOUT_SEED = 0.4, 20240607


def hparams(name):
    """-> the full hyper-parameter dict of one case."""
    from rnampnn.model._schema import DEFAULT_HPARAMS
    return dict(DEFAULT_HPARAMS, **OVERRIDES[name])


def batch():
    """-> (coords (4, 70, 7, 3) f32, mask (4, 70) f32, labels (4, 70) i64) of the shared ragged batch."""
    from rnampnn.utils import synth
    return synth.synth_batch(LENS, first_index=FIRST_INDEX)


def state_dict(name, train=False):
    """-> (hp, the case's state dict as numpy arrays): closed form x ``GAINS`` for the forward tests, the plain closed form for the
    trainer tests (``train``)."""
    from rnampnn.model._schema import state_dict_shapes
    from rnampnn.utils import synth
    from _weight_regimes import scaled_sd
    hp = hparams(name)
    return hp, scaled_sd(synth.closed_form_state_dict(state_dict_shapes(hp)), {} if train else GAINS.get(name, {}))
