"""CPU checks of the rdesign training step: the fp64 reference helper (tests/_rdesign_train_ref.py) agrees with the oracle it restates
and draws the documented dropout masks; the C ABI of the step is declared, bound and exported; the new translation unit keeps the
code base's rules (no runtime fill / copy calls, no float atomics); there is no CPU fallback."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import rdesign_oracle as O
from test_rdesign_cpu import _batch, _weights
import _rdesign_train_ref as R

NEW = ("rdesign_train_workspace_bytes", "rdesign_loss_and_grad")
TU = os.path.join(REPO, "rna-mpnn_amd", "csrc", "rdesign_train.hip")


@pytest.mark.parametrize("kw,lengths", [(dict(k_neighbors=6, num_mpnn_layers=2), [12, 4, 9]),
                                        (dict(k_neighbors=30, num_mpnn_layers=2, num_readout_layers=2, readout_hidden_dim=64,
                                              num_message_layers=2, num_dense_layers=1), [20, 1, 7])])
def test_helper_without_dropout_equals_the_oracle(kw, lengths):
    cfg = O.RDesignConfig(**kw)
    X, mask = _batch(lengths, seed=5)
    sd = {k: v.double() for k, v in _weights(cfg).items()}
    feats = O.raw_features(X.double(), mask.double(), cfg)
    h_ref, l_ref = O.forward(X.double(), mask.double(), sd, cfg)
    h, l = R.forward_train(*feats, mask, sd, cfg, p=0.0)
    assert (h - h_ref).abs().max() < 1e-12 and (l - l_ref).abs().max() < 1e-12        # same operations in fp64: rounding only
    loss, logits, grads = R.loss_and_grads(feats, mask, torch.zeros(mask.shape, dtype=torch.long), sd, cfg)
    assert set(grads) == set(sd) and all(float(g.abs().max()) > 0 for g in grads.values())   # no dead tensor in this model
    assert abs(loss - float(torch.nn.functional.cross_entropy(l_ref, torch.zeros(l_ref.shape[0], dtype=torch.long)))) < 1e-12


def test_helper_masks_drop_the_requested_share_and_differ_between_sites_and_seeds():
    cfg = O.RDesignConfig(k_neighbors=6, num_mpnn_layers=2)
    p, rows, width = 0.1, np.arange(400), 128
    n = rows.size * width
    sigma = (n * p * (1 - p)) ** 0.5
    masks = {}
    for seed in (71, 72):
        for site in (R.site_msg(cfg, 0, 0), R.site_msg(cfg, 1, 2), R.site_dense(cfg, 0, 1)):
            m = R.drop_mask(seed, site, rows, width, p)
            dropped = int((m == 0).sum())
            assert abs(dropped - n * p) < 3 * sigma, (seed, site, dropped)
            kept = m[m != 0]
            assert torch.all(kept == float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))))
            masks[(seed, site)] = m
    keys = list(masks)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            assert not torch.equal(masks[keys[i]], masks[keys[j]])
    # sites count the Dropout modules in forward order from 1
    assert [R.site_msg(cfg, 0, i) for i in range(3)] + [R.site_dense(cfg, 0, i) for i in range(3)] == [1, 2, 3, 4, 5, 6]
    assert R.site_msg(cfg, 1, 0) == 7 and R.site_readout(cfg, 0) == 13
    # and dropout moves the result
    X, mask = _batch([12, 4, 9], seed=5)
    sd = {k: v.double() for k, v in _weights(cfg).items()}
    feats = O.raw_features(X.double(), mask.double(), cfg)
    S = torch.randint(0, 4, mask.shape, generator=torch.Generator().manual_seed(1))
    _, _, g0 = R.loss_and_grads(feats, mask, S, sd, cfg, p=0.0)
    _, _, g1 = R.loss_and_grads(feats, mask, S, sd, cfg, p=0.1, seed=71)
    rel, _ = R.grad_errors(g1, g0)
    assert np.median(list(rel.values())) > 0.05


def test_training_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from rdesign import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rdesign_hip.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in rdesign_hip.h"
        assert name in _native.SYMBOLS
        assert hasattr(lib, name)
    assert "rdesign_train.hip" in g.SOURCES


def test_new_translation_unit_keeps_the_rules():
    src = open(TU).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for call in ("hipMemset", "hipMemcpy", "memset(", "memcpy("):
        assert call not in code, f"{call} in rdesign_train.hip: use launch_zero_bytes / launch_copy_bytes"
    assert "atomic" not in code, "no atomics in rdesign_train.hip: cross-workgroup sums go through the ordered reductions"
    assert "getenv" not in code and "ab_switch" not in code
    for fn in ("red_begin", "red_end", "launch_zero_bytes"):
        assert fn in code


def test_no_cpu_fallback_and_f32_only():
    from rdesign.model.rdesign import RNAModel
    X, mask = _batch([5])
    S = torch.zeros(1, 5, dtype=torch.long)
    m = RNAModel(num_mpnn_layers=1, precision="f32")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss_and_grad(X, S, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.training_step((X, S, mask, [5], None))
    b = RNAModel(num_mpnn_layers=1, precision="bf16")
    with pytest.raises(NotImplementedError, match="f32"):
        b.loss_and_grad(X, S, mask)
    with pytest.raises(NotImplementedError, match="f32"):
        b.training_step((X, S, mask, [5], None))
    with pytest.raises(NotImplementedError, match="training_step"):
        m.train()(X, S, mask)
