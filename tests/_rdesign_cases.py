"""Shared inputs of the rdesign tests and of tools/gen_golden_rdesign.py: the seeded batch and weight rules, and the loader of the
reference-made fixtures tests/golden/rdesign_*.npz.

The fixtures hold no weights: they store the seed and the hyper-parameters, and `_weights` regenerates the tensors (the generator
asserts that what it loaded into the reference's modules is bit-identical to what this file produces).

Keys of a fixture (f32 run of the reference's own `RNAFeatures` / `MPNNLayer` / `Readout` in eval mode unless tagged `_f64`):
  X (B,T,6,3) f32, mask (B,T) f32            the inputs
  meta                                       JSON: cfg (hyper-parameters), weight_seed, readout_scale (+ weight_seed2, readout_scale2: the second leg), stubbed (import placeholders the
                                             generator needed), e_nodes, row_stride, logit_std, excluded_share (share of rows whose top-2
                                             logit margin is <= 0.1) (+ label_seed, grad_stride on gradient cases)
  E_idx (2,E) int32                          the reference's packed edge list, row 0 = dst (the centre), row 1 = src (the neighbour)
  node_raw (N',101)                          input of features.node_embedding (forward pre-hook); N' = packed rows ::row_stride
  edge_raw (E',115)                          input of features.edge_embedding, the edges of the first `e_nodes` packed nodes only
  h_V (N,128), logits (N,4)                  final node state and read-out, every row
  h_V_f64 (N'',128), logits_f64 (N,4)        the float64 run; N'' = packed rows ::f64_row_stride
  h_V0, h_V1 (N',128), h_V0_f64 (N'',128)    after the feature stage / after layer 1: the FULL fixtures only (the rest stay small)
  s2.h_V (N/s2_row_stride,128), s2.logits (N,4), s2.logits_f64   the same inputs at the weights of meta["weight_seed2"]
and on gradient cases (meta has label_seed; float64 autograd of CrossEntropyLoss(readout(h_V), S), eval mode):
  S (B,T) int64, loss_f64 ()
  grad.<key>                                 the whole gradient (small model), or every 1-D tensor in full and rows ::grad_stride of every matrix
  grad_norm (n_tensors,), grad_flat_norm (), grad_probe_seed, grad_probe_dot ()   per-tensor L2, flat L2, <flat gradient, seeded normal vector>
  s2.loss_f64, s2.grad.<key>, s2.grad_norm, s2.grad_flat_norm, s2.grad_probe_dot  the second weight seed, matrix rows ::s2_grad_stride
"""
import json
import os

import numpy as np
import torch

from oracle import rdesign_oracle as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RDESIGN_GOLDEN = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("rdesign_") and f.endswith(".npz"))
FORWARD_KEYS = ("X", "mask", "E_idx", "node_raw", "edge_raw", "h_V", "logits", "h_V_f64", "logits_f64", "s2.h_V", "s2.logits", "s2.logits_f64")
FULL_KEYS = ("h_V0", "h_V1", "h_V0_f64")
META_KEYS = ("cfg", "weight_seed", "weight_seed2", "readout_scale", "readout_scale2", "stubbed", "e_nodes", "row_stride", "f64_row_stride", "s2_row_stride", "logit_std",
             "excluded_share")
GRAD_KEYS = ("S", "loss_f64", "grad_norm", "grad_flat_norm", "grad_probe_seed", "grad_probe_dot", "s2.loss_f64", "s2.grad_norm",
             "s2.grad_flat_norm", "s2.grad_probe_dot")
GRAD_META_KEYS = ("label_seed", "grad_stride", "s2_grad_stride")


def _batch(lengths, seed=0):
    from rnampnn.utils import synth
    T = max(lengths)
    X = np.zeros((len(lengths), T, 6, 3), np.float32)
    mask = np.zeros((len(lengths), T), np.float32)
    for i, n in enumerate(lengths):
        X[i, :n] = synth.synth_rna(n, i, seed=seed)[:, :6]
        mask[i, :n] = 1
    return torch.from_numpy(X), torch.from_numpy(mask)


def _weights(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in O.state_dict_shapes(cfg).items():
        if k.endswith("gain") or (("norm1" in k or "norm2" in k) and k.endswith("weight")):
            sd[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif len(shp) == 2:
            sd[k] = torch.randn(shp, generator=g) / shp[1] ** 0.5
        else:
            sd[k] = 0.1 * torch.randn(shp, generator=g)
    return sd


def _labels(mask, seed=3):
    return torch.randint(0, 4, tuple(mask.shape), generator=torch.Generator().manual_seed(seed))


def golden_weights(meta, leg=1, seed=None):
    """The state dict one leg of a fixture was made with (leg 1: weight_seed / readout_scale, leg 2: weight_seed2 / readout_scale2), or
    the rule of that leg at another `seed`: `_weights`, then the read-out's last Linear scaled (1 except on the separated-logit case)."""
    cfg = O.RDesignConfig(**meta["cfg"])
    tag = "" if leg == 1 else "2"
    sd = _weights(cfg, meta["weight_seed" + tag] if seed is None else seed)
    s = float(meta["readout_scale" + tag])
    if s != 1.0:
        last = 3 * max(cfg.num_readout_layers - 1, 0)
        for t in ("weight", "bias"):
            sd[f"readout.readout_layers.{last}.{t}"] = sd[f"readout.readout_layers.{last}.{t}"] * s
    return cfg, sd


def load_rdesign_golden(name):
    """-> (arrays dict, meta dict) of tests/golden/<name>.npz."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    arrs = {k: z[k] for k in z.files if k != "meta"}
    return arrs, json.loads(bytes(z["meta"]).decode())


def oracle_edge_list(E_idx, attend, mask):
    """The (2,E) dst/src list of feature.py:228-233 from the oracle's padded neighbour lists."""
    B, N, K = E_idx.shape
    shift = (mask.sum(1).cumsum(0) - mask.sum(1)).long()
    src = (shift.view(B, 1, 1) + E_idx)[attend]
    dst = (shift.view(B, 1, 1) + torch.arange(N).view(1, N, 1).expand(B, N, K))[attend]
    return torch.stack([dst, src])


def probe_vector(seed, numel):
    """The seeded normal vector of `grad_probe_dot` (float64, state-dict order, tensors flattened row-major)."""
    return torch.randn(numel, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64)


GRAD_GOLDEN = [n for n in RDESIGN_GOLDEN if "label_seed" in load_rdesign_golden(n)[1]]
