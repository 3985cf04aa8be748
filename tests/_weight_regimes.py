"""Weight regimes away from the closed-form corner, shared by test_weight_regimes_cpu.py and test_weight_regimes_gpu.py (CPU only).

At ``synth.closed_form_state_dict`` - U(+-1/sqrt(fan_in)) - hardly a GELU pre-activation of the per-edge MLPs passes the knee of the
packed-f16 Phi forms (|x| = sqrt(9.5) = 3.08: there ``clamp01(y^2)`` saturates), the attention is nearly uniform and the logits have a
standard deviation of 0.12.  ``scaled_sd`` multiplies the weights AND biases of one stage by a gain, which moves the f32 / f64 / autocast
oracles of ``_tap_oracle`` into the regimes of ``REGIMES``; ``regime_stats`` measures, on the f32 oracle alone, where a set of weights
sits (test_weight_regimes_cpu.py pins every regime to what its name claims).  One stage is scaled at a time so that the bf16-autocast
yardstick stays conditioned; ``all_mild`` scales all of them and is used for ``h_post``, ``raw_emb`` and the logits only.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import rnampnn_oracle as O
from _tap_oracle import closed_form_sd, oracle_config, oracle_runs, run_oracle

KGA = 0.324442842                      # csrc/bf16_dev.h kGA: the bf16 path stores e as f16 of KGA * e
KNEE = 9.5 ** 0.5                      # |x| beyond which clamp01((KGA x)^2) of phi4s / phi2s is saturated
F16_MAX = 65504.0
EDGE_KEYS = ("res_edge_embedding_layers", "message_layers", "edge_layers")

# edge_knee: x 1.45, not 1.5.  Counted over valid slots only, x 1.5 puts 45.9 % of the pre-activations of one first Linear beyond the knee,
# outside the 2 .. 40 % window test_weight_regimes_cpu.py holds this regime to; x 1.45 gives 2.4 .. 38.9 % over the 40 sites of case P.
REGIMES = {
    "closed_form": {},
    "edge_knee": {k: 1.45 for k in EDGE_KEYS},
    "edge_saturated": {k: 2.0 for k in EDGE_KEYS},
    "attention_peaked": {"in_proj": 3.0},
    "node_chains": {"ffn_layers": 3.0, "raw_ffn": 2.0, "readout": 4.0},
    "all_mild": dict({k: 1.5 for k in EDGE_KEYS}, in_proj=2.0, ffn_layers=2.0, readout=4.0),
    # outside the envelope on purpose (the f16 range contract): |KGA e| passes 65504 within a few layers
    "edge_overflow": {k: 8.0 for k in EDGE_KEYS},
}
IN_ENVELOPE = ("edge_knee", "edge_saturated", "attention_peaked", "node_chains", "all_mild")

# name -> (k, L, lens, T, first_index, tap layers)
CASES = {
    # k_resmpnn with its EMBED first launch, XCD ranges (122 blocks), an RNA with n - 1 < k, the fused k_attn_layer_rna over two key
    # blocks, k_node_update_rna, the three k_ffn_chain instantiations
    "P": (30, 10, [40, 37, 33, 12], 40, 700, (1, 5, 10)),
    # k_mpnn_bf16 / k_edge_embed_*
    "Q": (16, 3, [23, 40, 9], 40, 50, (1, 3)),
    # T > AL_NR = 144: the stand-alone k_attention_bf16_hd16 (five key blocks), the 64-key chunks of the f32 attention kernel
    "R": (16, 2, [150, 33], 150, 760, (2,)),
    # case Q at the production depth: the weights-driven leg of the range contract
    "Q_L10": (16, 10, [23, 40, 9], 40, 50, (10,)),
}
PAIRS = [("P", "edge_knee"), ("P", "edge_saturated"), ("P", "attention_peaked"), ("P", "node_chains"), ("P", "all_mild"),
         ("Q", "edge_saturated"), ("R", "attention_peaked"), ("R", "node_chains")]
ARGMAX_REGIMES = ("node_chains", "all_mild")
MAX_LEFT_OUT = 0.25


def asserted_taps(case, regime):
    """The oracle taps the device test asserts for a pair, as (name, is an edge tap); ``all_mild``: nothing finer than the node outputs."""
    fine = [] if regime == "all_mild" else [("h0", False), ("e0", True)] + [(f"{x}{l}", x == "e") for l in CASES[case][5] for x in "he"]
    return fine + [("h_post", False), ("raw_emb", False)]


def scaled_sd(sd_np, gains):
    """-> {key: float32 array}: every ``*weight`` / ``*bias`` tensor (``in_proj_weight`` / ``in_proj_bias`` included) whose key contains a
    substring of ``gains`` multiplied by that gain (by the product, where several match); GraphNorm ``scale`` / ``shift`` never.  A
    substring that matches no such key is an error."""
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in sd_np.items()}
    for sub, g in gains.items():
        keys = [k for k in out if sub in k and (k.endswith("weight") or k.endswith("bias"))]
        if not keys:
            raise KeyError(f"scaled_sd: no weight or bias key contains {sub!r}")
        for k in keys:
            out[k] = out[k] * np.float32(g)
    return out


class _TorchWithSoftmax:
    """Stands for ``torch`` inside the oracle module while ``regime_stats`` runs: ``softmax`` is wrapped, the rest passes through."""

    def __init__(self, on_softmax):
        self._on = on_softmax

    def __getattr__(self, name):
        return getattr(torch, name)

    def softmax(self, *a, **kw):
        p = torch.softmax(*a, **kw)
        self._on(p)
        return p


def regime_stats(hp, sd, coords, mask):
    """One f32 oracle run with ``_gelu`` (named by the ``_linear`` in front of it) and the softmax of ``rnabert`` wrapped ->
    dict(gelu = {Linear prefix: (share of |x| > KNEE, max |x|)} over valid rows / valid slots,
         attention = [mean over valid queries and heads of the largest probability, per attention layer in call order],
         ae_max = [max |KGA e_l| over valid slots, l = 0 .. L],  logits, finite = every tap of the run is finite on its valid part)."""
    m = torch.as_tensor(mask).float()
    c = torch.as_tensor(coords).float()
    sdt = O.state_dict_from_numpy(sd, torch.float32)
    cfg = oracle_config(hp)
    idx = O.knn_graph(c, m, cfg.num_res_neighbours)
    ok_node = m > 0
    ok_edge = ok_node.unsqueeze(-1) & (idx != -1)
    gelu, attention, last = {}, [], [None]
    orig = (O._linear, O._gelu, O.torch)

    def linear(x, sd_, prefix):
        last[0] = prefix
        return orig[0](x, sd_, prefix)

    def gelu_(x):
        v = x[ok_edge if x.dim() == 4 else ok_node].abs()
        assert last[0] is not None and last[0] not in gelu, last[0]
        gelu[last[0]] = (float((v > KNEE).float().mean()), float(v.max()))
        last[0] = None
        return orig[1](x)

    def on_softmax(p):                                      # (B, H, T, T)
        top = p.max(-1).values                              # (B, H, T)
        attention.append(float(top.transpose(1, 2)[ok_node].mean()))

    taps = {}
    O._linear, O._gelu, O.torch = linear, gelu_, _TorchWithSoftmax(on_softmax)
    try:
        with torch.no_grad():
            O.forward(c, m, sdt, cfg, taps=taps, edge_index=idx)
    finally:
        O._linear, O._gelu, O.torch = orig
    L = cfg.num_res_mpnn_layers
    e_max = [float(taps[f"e{l}"][ok_edge].abs().max()) for l in range(L + 1)]
    finite = all(bool(torch.isfinite(taps[f"e{l}"][ok_edge]).all()) for l in range(L + 1)) and bool(torch.isfinite(taps["logits"]).all())
    return dict(gelu=gelu, attention=attention, ae_max=[KGA * v for v in e_max], logits=taps["logits"], finite=finite)


def edge_sites(stats, which):
    """The message / edge-update GELU sites of ``regime_stats``: ``which`` = 0 (first Linears), 3 (second Linears) or None (both)."""
    return {k: v for k, v in stats["gelu"].items()
            if ("message_layers" in k or ".edge_layers" in k) and (which is None or k.endswith(f".{which}"))}


def left_out_share(logits_ref, mask, tol):
    """-> (share of valid rows whose top-2 margin of ``logits_ref`` is <= 2 tol, bool (B, T) of the rows that are kept)."""
    r = torch.as_tensor(logits_ref).double()
    top2 = torch.sort(r, -1).values
    valid = torch.as_tensor(mask) > 0
    clear = ((top2[..., -1] - top2[..., -2]) > 2.0 * tol) & valid
    return 1.0 - float(clear.sum()) / float(valid.sum()), clear


_cache = {}


def setup(case, regime, scale_rna=None, modes=("f32", "f64", "autocast")):
    """-> dict(hp, sd, lens, coords, mask, layers, runs) of ``CASES[case]`` at the weights of ``REGIMES[regime]``, computed once per process.
    ``scale_rna`` = (b, factor): the coordinates of RNA b multiplied by ``factor``, and every run on the graph of the UNSCALED batch
    (``scaled_graph_note``)."""
    key = (case, regime, scale_rna, tuple(modes))
    if key not in _cache:
        from rnampnn.model._schema import DEFAULT_HPARAMS
        from rnampnn.utils import synth
        k, L, lens, T, first, layers = CASES[case]
        hp = dict(DEFAULT_HPARAMS, num_res_neighbours=k, num_res_mpnn_layers=L, padding_len=T)
        sd = scaled_sd(closed_form_sd(hp)[0], REGIMES[regime])
        coords, mask, _ = synth.synth_batch(lens, first_index=first, max_len=T)
        if scale_rna is None:
            runs = oracle_runs(hp, sd, coords, mask, modes)
        else:
            idx = setup(case, regime, modes=("f32",))["runs"]["f32"]["edge_index"]
            coords = coords.copy()
            coords[scale_rna[0]] *= np.float32(scale_rna[1])
            runs = {m: run_oracle(hp, sd, coords, mask, m, edge_index=idx) for m in modes}
        _cache[key] = dict(hp=hp, sd=sd, lens=lens, coords=coords, mask=mask, layers=layers, runs=runs)
    return _cache[key]


scaled_graph_note = """The reference masks its distance matrix with the VALUE 1e6 (self and padded residues; feature.py:223-227), so its k-NN
graph is the nearest-neighbour graph only while every centroid distance stays below 1e6.  The kernels select among the real residues
(k_knn: "self and padded residues ... are never real neighbours") and share that domain.  Coordinates x 1e5 leave it - the oracle's own
search then ranks padding in front of real residues farther than 1e6 - so the scaled runs take the graph of the unscaled batch, which is
what a uniform scale of one RNA leaves of its neighbour order, and the device test asserts that the kernel's graph is that one."""


def stats_of(case, regime):
    key = ("stats", case, regime)
    if key not in _cache:
        s = setup(case, regime, modes=("f32",)) if (case, regime) not in PAIRS else setup(case, regime)
        _cache[key] = regime_stats(s["hp"], s["sd"], s["coords"], s["mask"])
    return _cache[key]
