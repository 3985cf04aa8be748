"""fp64 reference of the rdesign TRAINING step (test helper; imported by test_rdesign_train_cpu.py / test_rdesign_train_gpu.py).

`oracle.rdesign_oracle.forward` has no dropout and computes its own features; this module restates
its layer loop from that module's own pieces (`_custom_norm`, `_gelu`, `F.layer_norm`, the `src` / `dst` construction) with
`oracle.rnampnn_oracle.dropout_multiplier` at the sites `csrc/rdesign_train.hip` documents, takes the raw features as ARGUMENTS
(so a GPU test can feed the device's own taps and compare only the training code), runs in float64 and is differentiated by torch
autograd with `F.cross_entropy`.  At p = 0 its loss and gradients are PINNED to float64 autograd through the reference's own modules
(tests/golden/rdesign_*.npz, tests/test_rdesign_golden_cpu.py: per tensor within 1e-10); the dropout masks have no reference counterpart.

Dropout addressing: site = index of the Dropout module in forward order from 1 (layer l, message Linear i: 1 + l (M + D) + i;
layer l, hidden dense Linear i: 1 + l (M + D) + M + i; hidden read-out Linear j: 1 + L (M + D) + j); element = row * width +
channel with row = packed node row p, or packed edge row p * k_neighbors + slot.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rdesign_oracle as O
from oracle.rnampnn_oracle import dropout_multiplier


def site_msg(cfg, l, i):
    return 1 + l * (cfg.num_message_layers + cfg.num_dense_layers) + i


def site_dense(cfg, l, i):
    return 1 + l * (cfg.num_message_layers + cfg.num_dense_layers) + cfg.num_message_layers + i


def site_readout(cfg, j):
    return 1 + cfg.num_mpnn_layers * (cfg.num_message_layers + cfg.num_dense_layers) + j


def drop_mask(seed, site, rows, width, p):
    """-> float64 (len(rows), width) tensor of 0 | 1/(1-p): the multipliers of elements rows[r] * width + c."""
    idx = np.asarray(rows, dtype=np.int64)[:, None] * int(width) + np.arange(int(width), dtype=np.int64)[None, :]
    return torch.from_numpy(dropout_multiplier(seed, site, idx, p).astype(np.float64))


def forward_train(node, edge, E_idx, attend, mask, sd, cfg, p=0.0, seed=0, taps=None):
    """The layer loop of `O.forward` with dropout: raw features in the padded layout of `O.raw_features` (node (B,N,101), edge
    (B,N,K',115), E_idx (B,N,K'), attend (B,N,K') bool) -> (h_V (N_valid,128), logits (N_valid,4)) in the dtype of `sd`."""
    B, N, Kp = E_idx.shape
    K = cfg.k_neighbors
    mb = mask == 1
    dt = sd["features.node_embedding.weight"].dtype
    node, edge = node.to(dt), edge.to(dt)
    h_V = O._custom_norm(node[mb] @ sd["features.node_embedding.weight"].T + sd["features.node_embedding.bias"],
                         sd["features.norm_nodes.gain"], sd["features.norm_nodes.bias"])
    h_E = O._custom_norm(edge[attend] @ sd["features.edge_embedding.weight"].T + sd["features.edge_embedding.bias"],
                         sd["features.norm_edges.gain"], sd["features.norm_edges.bias"])
    shift = (mask.sum(1).cumsum(0) - mask.sum(1)).long()
    src = (shift.view(B, 1, 1) + E_idx)[attend]
    dst = (shift.view(B, 1, 1) + torch.arange(N).view(1, N, 1).expand(B, N, Kp))[attend]
    slot = torch.arange(Kp).view(1, 1, Kp).expand(B, N, Kp)[attend]
    n_nodes = h_V.shape[0]
    node_rows = np.arange(n_nodes, dtype=np.int64)
    edge_rows = (dst * K + slot).numpy().astype(np.int64)

    def drop(x, site, rows):
        if p <= 0.0:
            return x
        m = drop_mask(seed, site, rows, x.shape[1], p).to(x.dtype)
        if taps is not None:
            taps.setdefault("masks", {})[site] = m
        return x * m

    for l in range(cfg.num_mpnn_layers):
        q = f"mpnn_layers.{l}"
        x = torch.cat([h_E, h_V[dst], h_V[src]], -1)
        for i in range(cfg.num_message_layers):
            x = O._gelu(x @ sd[f"{q}.message_layers.{3 * i}.weight"].T + sd[f"{q}.message_layers.{3 * i}.bias"])
            x = drop(x, site_msg(cfg, l, i), edge_rows)
        dh = torch.zeros(n_nodes, x.shape[1], dtype=x.dtype).index_add(0, dst, x) / cfg.scale
        h_V = F.layer_norm(h_V + dh, (cfg.hidden_dim,), sd[q + ".norm1.weight"], sd[q + ".norm1.bias"])
        y = h_V
        for i in range(cfg.num_dense_layers):
            y = O._gelu(y @ sd[f"{q}.dense.{3 * i}.weight"].T + sd[f"{q}.dense.{3 * i}.bias"])
            y = drop(y, site_dense(cfg, l, i), node_rows)
        y = y @ sd[f"{q}.dense.{3 * cfg.num_dense_layers}.weight"].T + sd[f"{q}.dense.{3 * cfg.num_dense_layers}.bias"]
        h_V = F.layer_norm(h_V + y, (cfg.hidden_dim,), sd[q + ".norm2.weight"], sd[q + ".norm2.bias"])
    x = h_V
    for j in range(max(cfg.num_readout_layers - 1, 0)):
        x = O._gelu(x @ sd[f"readout.readout_layers.{3 * j}.weight"].T + sd[f"readout.readout_layers.{3 * j}.bias"])
        x = drop(x, site_readout(cfg, j), node_rows)
    last = 3 * max(cfg.num_readout_layers - 1, 0)
    logits = x @ sd[f"readout.readout_layers.{last}.weight"].T + sd[f"readout.readout_layers.{last}.bias"]
    return h_V, logits


def loss_and_grads(feats, mask, S, sd, cfg, p=0.0, seed=0):
    """float64 training step: -> (loss float, logits (N_valid,4) f64, {key: gradient f64}).  `feats` = (node, edge, E_idx, attend)."""
    leaf = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    node, edge, E_idx, attend = feats
    _, logits = forward_train(node.double(), edge.double(), E_idx, attend, mask, leaf, cfg, p, seed)
    loss = F.cross_entropy(logits, S[mask == 1].long())
    keys = list(leaf)
    grads = torch.autograd.grad(loss, [leaf[k] for k in keys])
    return float(loss.detach()), logits.detach(), dict(zip(keys, grads))


def device_features(model, X, mask):
    """The device's own raw features (taps of `rdesign_forward`, parent-commit code with its own test) in the padded layout
    `forward_train` takes: the comparison then sees only the training code, not the f32 rounding of the features."""
    out = model._run(X, mask, want=("edge_index", "node_raw", "edge_raw"))
    B, T = mask.shape
    K = model.hparams["k_neighbors"]
    mb = mask == 1
    node = torch.zeros(B, T, 101, dtype=torch.float64)
    edge = torch.zeros(B, T, K, 115, dtype=torch.float64)
    node[mb] = out["node_raw"].cpu().double()
    edge[mb] = out["edge_raw"].cpu().double().view(-1, K, 115)
    eidx = out["edge_index"].cpu()
    return node, edge, eidx.clamp(min=0), eidx >= 0


def grad_errors(g, r):
    """-> ({key: max|g - r| / max|r|}, flat cosine): the definition of tests/test_train_parity_gpu.py (every reference tensor of this
    model is non-zero: asserted)."""
    rel, dot, n1, n2 = {}, 0.0, 0.0, 0.0
    for key, rv in r.items():
        gv = g[key].double().reshape(rv.shape)
        dot += float((gv * rv).sum()); n1 += float((gv * gv).sum()); n2 += float((rv * rv).sum())
        scale = float(rv.abs().max())
        assert scale > 0.0, f"reference gradient of {key} is exactly zero"
        rel[key] = float((gv - rv).abs().max()) / scale
    return rel, dot / max((n1 * n2) ** 0.5, 1e-300)
