"""Oracle runs of the rdesign forward with the h_V tap of every layer, shared by test_rdesign_taps_cpu.py and test_rdesign_taps_gpu.py
(CPU only; the conventions of ``_tap_oracle.py``).

Three runs of ``oracle.rdesign_oracle.forward`` on the same inputs and weights:
  "f64"       float64 weights, coordinates and arithmetic: the reference of the device tests.
  "f32"       plain float32: its distance to "f64" is the f32 noise floor of a tap.
  "autocast"  float32 weights under ``torch.autocast("cpu", dtype=torch.bfloat16)``: every matmul takes bf16 operands.  Its distance to
              "f64" is the yardstick of the bf16 forward (``RDESIGN_PREC_BF16``).
``O.forward`` takes no graph override, so the three runs build their own k-NN lists; ``oracle_runs`` asserts that the attended slots are
the same in all three, and the cases below are ones where they are.

Taps without a tap entry in the ABI: ``h_E`` is never updated in this model, so ``h_V`` of a model built with ``num_mpnn_layers = l`` and
loaded with ``truncated(sd, l)`` IS the tap after layer ``l`` of the full model (test_rdesign_taps_cpu.py holds the oracle to that, bit
for bit).
"""
from __future__ import annotations

import dataclasses

import torch

from oracle import rdesign_oracle as O
from _rdesign_cases import _batch, _weights

COORD_SEED = 5
WEIGHT_SEEDS = (0, 1)
SWAP_BLOCKS = {"edge": 0, "centre": 128, "neighbour": 256}       # column offset in message_layers.0.weight [128][384] = [W_e | W_centre | W_neighbour]

# name -> (constructor keywords other than the defaults, lengths, tap depths); the last depth is num_mpnn_layers
CASES = {
    # the production stack (k 25, L 9, msg 3, dense 3 x 256); n = 1 and n < k; 320 residues, 8,000 edge rows
    "A_defaults": (dict(), [120, 97, 64, 31, 7, 1], (1, 2, 5, 9)),
    # RD_KMAX: 1,120 residues x 64 = 71,680 live edge rows = 560 tiles of 128 > the 512-workgroup cap of te_gemm / te_mlp2_fwd, host bound
    # B * T * k = 115,200 (900 tiles): the grid-stride loops do live work on their second pass, over a heavily padded tail
    "B_k64_stride": (dict(k_neighbors=64, num_mpnn_layers=2), [300, 280, 260, 200, 70, 10], (1, 2)),
    # smallest k (the self edge only); 257 residues = 256 + 1: a one-row last tile on the node side
    "C_k1": (dict(k_neighbors=1, num_mpnn_layers=2), [200, 56, 1], (1, 2)),
    # depth-1 message branch: te_gemm with the P/Q epilogue, no te_mlp2_fwd; 257 residues
    "D_msg1_dense2": (dict(k_neighbors=30, num_mpnn_layers=3, num_message_layers=1, num_dense_layers=2, dim_dense_layers=128),
                      [150, 64, 31, 11, 1], (1, 3)),
    # two chained actA te_gemm after te_mlp2_fwd; hidden read-out layers; exactly 256 residues and 2,048 edge rows: no partial tile anywhere
    "E_msg4_dense1_ro3": (dict(k_neighbors=8, num_mpnn_layers=3, num_message_layers=4, num_dense_layers=1, dim_dense_layers=512,
                               num_readout_layers=3, readout_hidden_dim=128), [128, 100, 27, 1], (1, 3)),
    # te_mlp2_fwd alone; odd k; n = k + 1, k, k - 1
    "F_msg2_k33": (dict(k_neighbors=33, num_mpnn_layers=3, num_message_layers=2), [128, 60, 34, 33, 32, 2], (1, 3)),
}


def case_inputs(name, seed):
    """-> (constructor keywords, RDesignConfig, state dict of f32 tensors, X, mask, tap depths) of one case at one weight seed."""
    kw, lens, depths = CASES[name]
    cfg = O.RDesignConfig(**kw)
    assert depths[-1] == cfg.num_mpnn_layers
    X, mask = _batch(lens, seed=COORD_SEED)
    return kw, cfg, _weights(cfg, seed), X, mask, depths


def run_oracle(cfg, sd, X, mask, mode):
    """-> taps dict of one oracle run (``h_V0 .. h_VL``, ``logits``, ``E_idx``, ``attend``, ...); float tensors cast to f64."""
    dt = torch.float64 if mode == "f64" else torch.float32
    sdt = {k: v.to(dt) for k, v in sd.items()}
    taps = {}
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=mode == "autocast"):
        _, logits = O.forward(X.to(dt), mask.to(dt), sdt, cfg, taps=taps)
    taps["logits"] = logits
    return {k: (v.to(torch.float64) if v.is_floating_point() else v) for k, v in taps.items()}


def oracle_runs(cfg, sd, X, mask):
    """-> {"f64", "f32", "autocast"}: tap dicts; the attended neighbour lists of the three runs must be equal."""
    runs = {m: run_oracle(cfg, sd, X, mask, m) for m in ("f64", "f32", "autocast")}
    att, idx = runs["f32"]["attend"], runs["f32"]["E_idx"]
    for m in ("f64", "autocast"):
        assert torch.equal(runs[m]["attend"], att), f"the {m} oracle attends other slots than the f32 oracle"
        assert torch.equal(runs[m]["E_idx"][att], idx[att]), f"the {m} oracle's k-NN lists differ from the f32 oracle's"
    return runs


def truncated(sd, l):
    """The state dict of the first ``l`` layers: ``sd`` without ``mpnn_layers.j.*`` for j >= l."""
    return {k: v for k, v in sd.items() if not (k.startswith("mpnn_layers.") and int(k.split(".")[1]) >= l)}


def truncated_config(cfg, l):
    return dataclasses.replace(cfg, num_mpnn_layers=l)


def swapped_inputs(sd, layer, block, a=5, b=77):
    """The negative control: INPUT columns ``a`` and ``b`` of one 128-wide block (``SWAP_BLOCKS``) of the first message Linear of layer
    ``layer`` exchanged - correct code on other weights.  At layer 1 / "neighbour" it moves the final h_V and the logits by less than the
    flat 5e-2 of the final-tensor tests and ``max ch`` of h_V2 by several times the autocast figure (test_rdesign_taps_cpu.py)."""
    key, off = f"mpnn_layers.{layer}.message_layers.0.weight", SWAP_BLOCKS[block]
    out = dict(sd)
    w = sd[key].clone()
    w[:, [off + a, off + b]] = w[:, [off + b, off + a]]
    out[key] = w
    return out
