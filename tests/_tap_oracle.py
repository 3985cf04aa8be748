"""Oracle runs with every h / e tap, shared by test_tap_metrics_cpu.py, test_mpnn_taps_gpu.py and test_knn_ties_*.py (CPU only).

Three runs of ``oracle.rnampnn_oracle.forward`` on the same inputs and weights:
  "f64"       float64 weights, coordinates and arithmetic on the graph of the f32 run: the reference of the device tests.  The neighbour
              set and the slot order are a discrete function of the f32 coordinates, and f64 distances could reorder a near-tie.
  "f32"       plain float32: its distance to "f64" is the f32 noise floor of a tap.
  "autocast"  float32 under ``torch.autocast("cpu", dtype=torch.bfloat16)``: every matmul takes bf16 operands, the precision the reference
              trains in (bf16-mixed).  Its distance to "f32" is the yardstick of the bf16 fast path, which claims to be finer (f16 operands).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import rnampnn_oracle as O
from rnampnn.utils import synth

SWAP_KEY, SWAP_ROWS = "res_mpnn_layers.3.edge_layers.{}.weight", (5, 77)


def oracle_config(hp) -> O.OracleConfig:
    return O.OracleConfig(**{k: v for k, v in hp.items() if k in O.OracleConfig.__dataclass_fields__})


def closed_form_sd(hp):
    """-> (state dict of numpy arrays, shapes) of the closed-form weights for the hyper-parameters ``hp``."""
    from rnampnn.model._schema import DEFAULT_HPARAMS, state_dict_shapes
    shapes = state_dict_shapes(dict(DEFAULT_HPARAMS, **{k: v for k, v in hp.items() if k in DEFAULT_HPARAMS}))
    return synth.closed_form_state_dict(shapes), shapes


def swapped(sd_np, hp):
    """The negative control: output channels 5 and 77 of the LAST Linear of layer 4's edge update exchanged (rows of its weight).  It moves
    two channels of e4 by a few per cent of |e| and the logits by less than any logit test can see."""
    key = SWAP_KEY.format(3 * (int(hp.get("num_mpnn_edge_layers", 2)) - 1))
    out = dict(sd_np)
    w = np.array(sd_np[key], copy=True)
    a, b = SWAP_ROWS
    w[[a, b]] = w[[b, a]]
    out[key] = w
    return out


def run_oracle(hp, sd_np, coords, mask, mode, edge_index=None):
    """-> taps dict of CPU tensors (h0, e0, h1, e1, ..., edge_index, logits, ...) of one oracle run; ``mode`` as in the module docstring."""
    dtype = torch.float64 if mode == "f64" else torch.float32
    sd = O.state_dict_from_numpy(sd_np, dtype)
    c, m = torch.as_tensor(coords).to(dtype), torch.as_tensor(mask).to(dtype)
    taps = {}
    with torch.no_grad():
        if mode == "autocast":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                O.forward(c, m, sd, oracle_config(hp), taps=taps, edge_index=edge_index)
        else:
            O.forward(c, m, sd, oracle_config(hp), taps=taps, edge_index=edge_index)
    return {k: (v if k == "edge_index" else v.to(torch.float64 if mode == "f64" else torch.float32)) for k, v in taps.items()}


def oracle_runs(hp, sd_np, coords, mask, modes=("f32", "f64", "autocast")):
    """-> {mode: taps}; the f64 run takes the f32 run's graph, and the graph under autocast must equal it."""
    runs = {"f32": run_oracle(hp, sd_np, coords, mask, "f32")}
    idx = runs["f32"]["edge_index"]
    if "f64" in modes:
        runs["f64"] = run_oracle(hp, sd_np, coords, mask, "f64", edge_index=idx)
    if "autocast" in modes:
        runs["autocast"] = run_oracle(hp, sd_np, coords, mask, "autocast")
        assert torch.equal(runs["autocast"]["edge_index"], idx), "bf16 autocast changed the k-NN graph"
    return runs


def load_fixture(subdir, name):
    """-> (arrays, hparams, state-dict shapes) of tests/golden/<subdir>/<name>.npz (``conftest.load_golden`` reads the top level only)."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", subdir, name + ".npz"))
    arrs = {k: z[k] for k in z.files if k not in ("hparams", "state_keys")}
    hp = json.loads(bytes(z["hparams"]).decode())
    shapes = {k: tuple(v) for k, v in json.loads(bytes(z["state_keys"]).decode()).items()}
    return arrs, hp, shapes


TIE_FIXTURES = ("k30_20_21", "k30_20_22", "k30_27_28_25", "k5_L2_5_6")
