"""``RNAModel`` of the reference's ``rdesign`` package (``rdesign/model/rdesign.py:18-209``) on the MI355X path.

The module tree (``features.node_embedding`` ... ``mpnn_layers.{i}.message_layers.{0,3,6}`` ... ``readout.readout_layers.{j}``)
reproduces the reference's ``state_dict`` keys and shapes, so a reference checkpoint's ``state_dict`` loads with
``load_state_dict``; the sub-modules are parameter holders, the arithmetic is ``rdesign_forward`` of ``librnampnn_hip.so``.
Inference surface (``forward``, ``readout``, ``validation_step`` / ``test_step`` metrics, ``predict``) in f32 or bf16, and the
exact-f32 TRAINING STEP: ``loss_and_grad`` (``rdesign_loss_and_grad``: taped forward with dropout, cross-entropy, HIP backward into ONE
flat gradient buffer), ``training_step`` (the same behind an autograd node) and ``configure_optimizers(fused=True)`` (the main model's
``FlatAdam`` on this model's flat buffers).  f32 is the reference arithmetic of this model (its trainer sets no ``precision``,
``rdesign/utils/train.py:107-115``) and the default of the step; ``train_precision="bf16"`` opts into the bf16-mixed step
(``rdesign_loss_and_grad_ex``: bf16 per-edge tensors, MFMA GEMMs) on a model of either ``precision``.  ``augment_eps > 0`` is the
reference's ``RNAFeatures(augment_eps)`` (``feature.py:157-158``): train-mode steps see ``X + eps * N(0, 1)``, added on the device as a
function of the step's seed (``rnampnn_augment_coords``); eval-mode paths never look at it.  A differentiable
``forward`` / ``readout`` pair is not built.
Epoch-level surface: ``score_batch`` (one forward + ``rdesign_score``: per-RNA correct / valid / NLL as device tensors, no host round
trip when the loader's host ``lengths`` are passed), ``reserve_training``, ``allreduce_gradients`` (one flat all-reduce) - what
``rdesign.utils.train.Trainer`` drives.  The XGBoost head: ``xgb_readout`` is None until ``fit_xgb_readout`` / ``load_xgb_readout`` attach
the main model's device tree read-out (``rnampnn/model/xgb.py``, parity with XGBoost unpinned) to the packed 128-wide ``h_V``
(``rdesign/utils/train.py:58-89``, ``rdesign.py:151-153``); without one ``predict`` takes the reference's ``NotFittedError`` branch,
argmax of ``Readout`` (``rdesign.py:152-155``).
Parity: eval-mode forward, graph, features and p = 0 gradients are pinned to the reference's own modules (``tests/golden/rdesign_*.npz``);
dropout masks, the XGBoost branch of ``predict`` and the Lightning plumbing are not.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native
from rnampnn.model._base import _prep, _stream
from rnampnn.model.decode import (check_avoid, check_chain, check_distinct, check_mutations, check_nested, check_require, check_state_lengths, check_profile_tree, check_tree, design_by_mode, design_distinct_from_logits,  # noqa: F401
                                  design_from_logits, design_gc_from_logits, design_mode, design_mutations_from_logits, design_profile_from_logits, resolve_design, resolve_profile,
                                  letters_packed,
                                  score_logits)

_PREC = {"f32": _native.PREC_F32, "bf16": _native.PREC_BF16}
_TRAIN = {"f32": _native.TRAIN_F32, "bf16": _native.TRAIN_BF16_MIXED}


class _Holder(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError("this sub-module only holds parameters: call RNAModel.forward (HIP path, no CPU fallback)")


class Normalize(_Holder):
    """``functional.Normalize`` (rdesign/model/functional.py:79-96)."""

    def __init__(self, features: int):
        super().__init__()
        self.gain = nn.Parameter(torch.ones(features))
        self.bias = nn.Parameter(torch.zeros(features))


class RNAFeatures(_Holder):
    """Parameters of ``feature.RNAFeatures`` (rdesign/model/feature.py:8-27)."""

    def __init__(self, hidden: int):
        super().__init__()
        self.node_embedding = nn.Linear(101, hidden)
        self.edge_embedding = nn.Linear(115, hidden)
        self.norm_nodes = Normalize(hidden)
        self.norm_edges = Normalize(hidden)


def _mlp(sizes, act_last: bool, dropout: float) -> nn.Sequential:
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if act_last or i + 2 < len(sizes):
            layers += [nn.GELU(), nn.Dropout(dropout)]
    return nn.Sequential(*layers)


class MPNNLayer(_Holder):
    """Parameters of ``mpnn.MPNNLayer`` (rdesign/model/mpnn.py:5-29)."""

    def __init__(self, hidden, num_in, num_message_layers, num_dense_layers, dim_dense_layers, dropout=0.1, scale=30):
        super().__init__()
        self.scale = scale
        self.norm1 = nn.LayerNorm(hidden)
        self.norm2 = nn.LayerNorm(hidden)
        self.message_layers = _mlp([hidden + num_in] + [hidden] * num_message_layers, True, dropout)
        self.dense = _mlp([hidden] + [dim_dense_layers] * num_dense_layers + [hidden], False, dropout)


class Readout(nn.Module):
    """``functional.Readout`` (rdesign/model/functional.py:98-126); ``forward`` runs ``rdesign_readout``."""

    def __init__(self, owner: "RNAModel", hidden: int, readout_hidden_dim: int, num_layers: int, dropout: float):
        super().__init__()
        self.readout_layers = _mlp([hidden] + [readout_hidden_dim] * max(num_layers - 1, 0) + [4], False, dropout)
        object.__setattr__(self, "_owner", owner)          # not a sub-module: no cycle in the module tree

    def forward(self, res_embedding: torch.Tensor) -> torch.Tensor:
        return self._owner._readout_native(res_embedding)


class _TrainStep(torch.autograd.Function):
    """The loss of one ``rdesign_loss_and_grad`` call as an autograd leaf-maker: forward runs the native step into a private
    gradient buffer, backward ACCUMULATES ``incoming * gradient`` into the module's ``flat_grad`` (torch semantics: ``p.grad`` grows
    until ``zero_grad``).  The parameters are inputs only so that the node is part of the graph; they get no gradient through
    autograd's own return values (None) - ``p.grad`` are views of ``flat_grad``."""

    @staticmethod
    def forward(ctx, model, X, S, mask, p, seed, *params):
        g = torch.empty_like(model._flat)
        loss = model._step_native(X, S, mask, p, seed, g)[0]
        ctx.model, ctx.g = model, g
        return loss

    @staticmethod
    def backward(ctx, dloss):
        m, g = ctx.model, ctx.g
        if g is None:
            raise RuntimeError("the gradient of this training_step was already consumed (backward ran twice on one step)")
        ctx.g = None
        dev = g.device
        fresh = m._bind_flat_grad(dev)
        if fresh:                                   # the views were dropped (zero_grad(set_to_none=True)): gradients restart from zero
            m.flat_grad.zero_()
        m.flat_grad.add_(g * dloss.to(dev))
        return (None,) * (6 + len(m._slices))


class RNAModel(nn.Module):
    def __init__(self, hidden_dim: int = 128, vocab_size: int = 4, k_neighbors: int = 25, dropout: float = 0.1,
                 node_feat_types=None, edge_feat_types=None, num_message_layers: int = 3, num_dense_layers: int = 3,
                 dim_dense_layers: int = 256, num_mpnn_layers: int = 9, readout_hidden_dim: int = 256,
                 num_readout_layers: int = 0, lr: float = 0.002, n_estimators: int = 100, xgb_max_depth: int = 6,
                 xgb_learning_rate: float = 0.1, xgb_subsample: float = 0.8, xgb_colsample_bytree: float = 0.8,
                 precision: str = "bf16", train_precision: Optional[str] = None, augment_eps: float = 0.0):
        super().__init__()
        if node_feat_types not in (None, ["angle", "distance", "direction"]) or \
                edge_feat_types not in (None, ["orientation", "distance", "direction"]):
            raise NotImplementedError("the HIP path builds the reference's default feature set (101 node / 115 edge features)")
        if vocab_size != 4:
            raise NotImplementedError("vocab_size must be 4 (AUCG)")
        if precision not in _PREC:
            raise ValueError(f"precision must be one of {sorted(_PREC)}")
        self.name, self.version, self.precision = "RDesign-X", 0, precision
        self.train_precision = "f32" if train_precision is None else train_precision      # not a hyper-parameter of the handle, not in the state dict
        if not float(augment_eps) >= 0.0:
            raise ValueError("augment_eps must be >= 0")
        self.augment_eps = float(augment_eps)          # RNAFeatures(augment_eps), feature.py:157-158: train-mode steps only, not the handle's business
        self.hparams = dict(hidden_dim=hidden_dim, vocab_size=vocab_size, k_neighbors=k_neighbors, dropout=dropout,
                            num_message_layers=num_message_layers, num_dense_layers=num_dense_layers,
                            dim_dense_layers=dim_dense_layers, num_mpnn_layers=num_mpnn_layers,
                            readout_hidden_dim=readout_hidden_dim, num_readout_layers=num_readout_layers, lr=lr)
        self.xgb_hparams = dict(n_estimators=n_estimators, xgb_max_depth=xgb_max_depth, xgb_learning_rate=xgb_learning_rate,
                                xgb_subsample=xgb_subsample, xgb_colsample_bytree=xgb_colsample_bytree)      # not the handle's business
        self.xgb_readout = None                        # a ``GBDTReadout`` once fitted / loaded: ``predict`` then takes the tree route
        self.hidden_dim, self.vocab = hidden_dim, vocab_size
        self._handle = _native.Handle(self.hparams, _PREC[precision])      # validates like the reference constructor would fail later
        self.features = RNAFeatures(hidden_dim)
        self.mpnn_layers = nn.ModuleList([
            MPNNLayer(hidden_dim, hidden_dim * 2, num_message_layers, num_dense_layers, dim_dense_layers, dropout=dropout)
            for _ in range(num_mpnn_layers)])
        self.readout = Readout(self, hidden_dim, readout_hidden_dim, num_readout_layers, dropout)
        self.loss_fn = nn.CrossEntropyLoss()
        self.val_step_outputs = {"val_loss": [], "correct": [], "len": [], "recovery_rates": []}
        self.test_step_outputs = {"test_loss": [], "correct": [], "len": [], "recovery_rates": []}
        schema = self._handle.weight_schema()
        named = dict(self.named_parameters())
        assert [k for k, _, _ in schema] == list(named), "parameter table of the library != module tree"
        assert all(named[k].numel() == n for k, n, _ in schema)
        self._slices = [(named[k], off, n) for k, n, off in schema]
        self._flat: Optional[torch.Tensor] = None
        self._sig = None
        self._ws: Optional[torch.Tensor] = None
        self._ext_version = 0
        self._seed_base, self._seed_ctr = 0, 0
        self.flat_grad: Optional[torch.Tensor] = None
        self._tws: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ native state
    @property
    def train_precision(self) -> str:
        """Arithmetic of the training step: ``"f32"`` (exact f32, ``precision="f32"`` models only) or ``"bf16"`` (bf16-mixed, any model)."""
        return self._train_precision

    @train_precision.setter
    def train_precision(self, value: str) -> None:
        if value not in _TRAIN:
            raise ValueError(f"train_precision must be one of {sorted(_TRAIN)}")
        object.__setattr__(self, "_train_precision", value)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @property
    def init_kwargs(self) -> dict:
        """Constructor arguments that rebuild this module (plain types: what a checkpoint stores next to the ``state_dict``)."""
        return dict(self.hparams, **self.xgb_hparams, precision=self.precision, train_precision=self.train_precision, augment_eps=self.augment_eps)

    def _device(self) -> torch.device:
        """The CUDA device of the parameters (the name the main model's helpers use); raises on a CPU module."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("the rdesign HIP path runs on an MI355X: move the module to 'cuda' first (there is no CPU fallback)")
        return dev

    def _ensure(self, for_mixed_training: bool = False) -> torch.device:
        """Parameters aliased to the flat arena, kernel-side weight copies current.  ``for_mixed_training`` is accepted for
        ``FlatAdam`` (the main model skips its finalize with it); this model always finalizes: both training steps read the K-major
        copies of the embedding Linears, and finalize is what tells a bf16 model's inference path to rebuild its weight images."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("the rdesign HIP path runs on an MI355X: move the module to 'cuda' first (there is no CPU fallback)")
        lib = _native.lib()
        flat = self._flat
        if flat is None or flat.device != dev or any(p.data_ptr() != flat.data_ptr() + 4 * off for p, off, _ in self._slices):
            flat = torch.zeros(int(lib.rdesign_param_numel(self._handle.ptr)), dtype=torch.float32, device=dev)
            with torch.no_grad():
                for p, off, n in self._slices:
                    flat[off: off + n].copy_(p.data.reshape(-1))
                    p.data = flat[off: off + n].view(p.shape)
            with torch.cuda.device(dev):
                _native.check(lib.rdesign_use_weight_arena(self._handle.ptr, C.c_void_p(flat.data_ptr()), _stream(dev)))
            self._flat, self._sig = flat, None
        sig = (self._ext_version,) + tuple(p._version for p, _, _ in self._slices)
        if sig != self._sig:
            with torch.cuda.device(dev):
                _native.check(lib.rdesign_finalize_weights(self._handle.ptr, _stream(dev)))
            self._sig = sig
        return dev

    # what ``rnampnn.model.rnampnn.FlatAdam`` reads of a model
    @property
    def _flat_param(self) -> torch.Tensor:
        return self._flat

    @property
    def _param_slices(self):
        return self._slices

    def _weights_touched(self) -> None:
        """An in-place update of the flat buffer (``FlatAdam.step``) bypasses the parameters' version counters."""
        self._ext_version += 1

    def _bind_flat_grad(self, device) -> bool:
        """(Re-)bind every ``p.grad`` to its slice of ONE flat buffer laid out like the weight arena; True when a view had to be
        (re)made, i.e. ``zero_grad(set_to_none=True)`` dropped the gradients since the last backward."""
        if self.flat_grad is None or self.flat_grad.device != device:
            self.flat_grad = torch.zeros(int(_native.lib().rdesign_param_numel(self._handle.ptr)), dtype=torch.float32, device=device)
        base = self.flat_grad.data_ptr()
        fresh = False
        for p, off, n in self._slices:
            if p.grad is None or p.grad.data_ptr() != base + 4 * off:
                p.grad = self.flat_grad[off: off + n].view(p.shape)
                fresh = True
        return fresh

    def manual_seed(self, seed: int) -> None:
        """Seed of the dropout masks: call ``i`` after this draws its masks from ``seed + i``."""
        self._seed_base, self._seed_ctr = int(seed), 0

    def _next_seed(self) -> int:
        sd = self._seed_base + self._seed_ctr
        self._seed_ctr += 1
        return sd

    def _ws_args(self, B: int, T: int, dev, readout_rows: int = 0):
        lib = _native.lib()
        need = int(lib.rdesign_readout_workspace_bytes(self._handle.ptr, readout_rows) if readout_rows
                   else lib.rdesign_workspace_bytes(self._handle.ptr, B, T))
        if self._ws is None or self._ws.numel() < need + 256 or self._ws.device != dev:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        return C.c_void_p(aligned), C.c_size_t(self._ws.numel() - (aligned - base))

    @staticmethod
    def _check_mask(mask: torch.Tensor) -> None:
        m = mask.detach().cpu()
        if not bool((((m == 0) | (m == 1)).all()) and bool((m[:, 1:] <= m[:, :-1]).all())):
            raise ValueError("mask must be a 0/1 prefix mask per RNA (rdesign/utils/data.py:104-115 compacts valid residues)")

    def _run(self, X, mask, want=("h_V", "logits"), n_valid: Optional[int] = None):
        dev = self._ensure()
        if X.dim() != 4 or X.shape[2:] != (6, 3) or mask.shape != X.shape[:2]:
            raise ValueError(f"X must be (B, T, 6, 3) and mask (B, T); got {tuple(X.shape)}, {tuple(mask.shape)}")
        B, T = int(X.shape[0]), int(X.shape[1])
        if B == 0 or T == 0:
            raise ValueError("empty batch")
        if n_valid is None:                      # a caller that passes n_valid vouches for the mask (no host sync on the hot path)
            self._check_mask(mask)
        n = int(mask.sum().item()) if n_valid is None else n_valid
        Xd, md = _prep(X, dev), _prep(mask, dev)
        K = self.hparams["k_neighbors"]
        out = {}
        alloc = dict(h_V=lambda: torch.zeros(B * T, 128, device=dev), logits=lambda: torch.zeros(B * T, 4, device=dev),
                     edge_index=lambda: torch.full((B, T, K), -1, dtype=torch.int64, device=dev),
                     node_raw=lambda: torch.zeros(B * T, 101, device=dev), edge_raw=lambda: torch.zeros(B * T * K, 115, device=dev))
        for k in want:
            out[k] = alloc[k]()
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None
        ws, ws_bytes = self._ws_args(B, T, dev)
        with torch.cuda.device(dev):
            _native.check(_native.lib().rdesign_forward(self._handle.ptr, C.c_void_p(Xd.data_ptr()), C.c_void_p(md.data_ptr()), B, T,
                                                        ptr("h_V"), ptr("logits"), ptr("edge_index"), ptr("node_raw"), ptr("edge_raw"),
                                                        ws, ws_bytes, _stream(dev)))
        for k in ("h_V", "logits", "node_raw"):
            if k in out:
                out[k] = out[k][:n]
        if "edge_raw" in out:
            out["edge_raw"] = out["edge_raw"][:n * K]
        return out

    def _readout_native(self, h_V: torch.Tensor) -> torch.Tensor:
        dev = self._ensure()
        x = _prep(h_V, dev)
        if x.dim() != 2 or x.shape[1] != 128 or x.shape[0] == 0:
            raise ValueError(f"res_embedding must be (N, 128), N > 0; got {tuple(x.shape)}")
        n = int(x.shape[0])
        logits = torch.empty(n, 4, device=dev)
        ws, ws_bytes = self._ws_args(1, n, dev, readout_rows=n)
        with torch.cuda.device(dev):
            _native.check(_native.lib().rdesign_readout(self._handle.ptr, C.c_void_p(x.data_ptr()), n, C.c_void_p(logits.data_ptr()),
                                                        ws, ws_bytes, _stream(dev)))
        return logits

    # ------------------------------------------------------------------ reference surface
    def forward(self, X, S, mask, is_predict: bool = False):
        """-> (h_V (N, 128), S (N,)): packed over the valid residues (``rdesign.py:82-88``, ``feature.py:187-189``)."""
        if self.training:
            raise NotImplementedError("forward() of the rdesign HIP path is not differentiable: train with training_step(batch) or "
                                      "loss_and_grad(X, S, mask) (one native call: forward, loss and backward); call .eval() for inference")
        out = self._run(X, mask, want=("h_V",))
        S_packed = torch.masked_select(S.to(out["h_V"].device), mask.to(out["h_V"].device) == 1)
        return out["h_V"], S_packed

    def forward_logits(self, X, mask) -> torch.Tensor:
        """``readout(forward(...)[0])`` in one call (no second launch sequence)."""
        return self._run(X, mask, want=("logits",))["logits"]

    def configure_optimizers(self, fused: bool = False):
        """``rdesign.py:90-93``: Adam(lr) + StepLR(40, 0.8).  ``fused=True``: the main model's ``FlatAdam`` (one launch per step on
        the flat parameter / gradient buffers, weight decay 0) instead of ``torch.optim.Adam``."""
        if fused:
            from rnampnn.model.rnampnn import FlatAdam
            self._ensure()
            optimizer = FlatAdam(self, lr=self.hparams["lr"], weight_decay=0.0)
        else:
            optimizer = torch.optim.Adam(self.parameters(), lr=self.hparams["lr"])
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=40, gamma=0.8)
        return [optimizer], [scheduler]

    # ------------------------------------------------------------------ epoch-level surface (rdesign.utils.train.Trainer)
    def reserve_training(self, shapes) -> None:
        """Size the training workspace for the largest of ``shapes`` = iterable of (B, T) BEFORE a timed loop (``RNAMPNN.reserve_training``):
        growing a multi-gigabyte tape in the middle of an epoch costs a free + allocate + the allocator's synchronisation."""
        dev = self._ensure()
        lib, flags = _native.lib(), _TRAIN[self.train_precision]
        need = max((int(lib.rdesign_train_workspace_bytes_ex(self._handle.ptr, int(B), int(T), flags)) for B, T in shapes), default=0)
        if need and (self._tws is None or self._tws.numel() < need + 256 or self._tws.device != dev):
            self._tws = None
            self._tws = torch.empty(int(need * 1.05) + 256, dtype=torch.uint8, device=dev)

    def allreduce_gradients(self, force: bool = False) -> None:
        """Average ``flat_grad`` over the ranks of the default process group: ONE ``all_reduce`` of the flat buffer on the caller's stream,
        then a scale by 1 / world.  A no-op without a process group or at world size 1 unless ``force`` (tests drive the RCCL path on one
        GPU with it).  No chunks, no side stream."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or force)):
            return
        dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM)
        world = dist.get_world_size()
        if world > 1:
            self.flat_grad.mul_(1.0 / world)

    def _score_native(self, logits, pred, mask, S, want_nll: bool = True, want_pred: bool = False):
        """``rdesign_score`` on packed ``logits`` (n, 4) f32 XOR packed ``pred`` (n,) int32 -> (correct (B,) i32, valid (B,) i32,
        nll (B,) f32 or None, pred_out (n,) i32 or None), all on the device, nothing synchronised."""
        dev = self._device()
        if mask.dim() != 2 or tuple(S.shape) != tuple(mask.shape):
            raise ValueError(f"mask and S must be (B, T); got {tuple(mask.shape)}, {tuple(S.shape)}")
        B, T = int(mask.shape[0]), int(mask.shape[1])
        md, lab = _prep(mask, dev), _prep(S, dev, torch.int32)
        lg = None if logits is None else _prep(logits, dev)
        pr = None if pred is None else _prep(pred, dev, torch.int32)
        src = lg if lg is not None else pr
        n = 0 if src is None else int(src.shape[0])
        correct = torch.empty(B, dtype=torch.int32, device=dev)
        valid = torch.empty(B, dtype=torch.int32, device=dev)
        nll = torch.empty(B, dtype=torch.float32, device=dev) if want_nll else None
        pred_out = torch.empty(n, dtype=torch.int32, device=dev) if want_pred else None
        lib = _native.lib()
        ws = torch.empty(max(int(lib.rdesign_score_workspace_bytes(B)), 16), dtype=torch.uint8, device=dev)
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            _native.check(lib.rdesign_score(vp(lg), vp(pr), n, vp(md), vp(lab), B, T, vp(correct), vp(valid), vp(nll), vp(pred_out),
                                            vp(ws), C.c_size_t(ws.numel()), _stream(dev)))
        return correct, valid, nll, pred_out

    @staticmethod
    def _n_valid(lengths) -> Optional[int]:
        return None if lengths is None else int(sum(int(v) for v in lengths))

    @torch.no_grad()
    def score_batch(self, X, S, mask, lengths=None, use_trees: bool = False):
        """What ``validation_step`` accumulates, per RNA and on the device: one forward + ``rdesign_score`` ->
        (correct (B,) int32, valid (B,) int32, nll (B,) f32 = per-RNA SUM of the cross-entropy; None on the tree route).  ``lengths``:
        the host-side lengths the loader already has - with them nothing here touches the host (the caller vouches for the prefix mask);
        without them ``_run`` checks the mask and counts its ones on the host.  ``use_trees``: score ``xgb_readout.predict(h_V)``."""
        n = self._n_valid(lengths)
        if use_trees:
            if self.xgb_readout is None:
                raise RuntimeError("score_batch(use_trees=True) needs a tree read-out: call fit_xgb_readout or load_xgb_readout first")
            h_V = self._run(X, mask, want=("h_V",), n_valid=n)["h_V"]
            return self._score_native(None, self.xgb_readout.predict(h_V), mask, S, want_nll=False)[:3]
        logits = self._run(X, mask, want=("logits",), n_valid=n)["logits"]
        return self._score_native(logits, None, mask, S)[:3]

    # ------------------------------------------------------------------ constrained design on the packed logits (rnampnn_design / rnampnn_score)
    def _packed_logits(self, X, mask, lengths):
        """-> (packed logits (n, 4), cu_seqlens (B+1,) int32 built on the device from the mask's row sums, T): nothing here waits for the
        device when the loader's host ``lengths`` are passed (``score_batch``)."""
        logits = self._run(X, mask, want=("logits",), n_valid=self._n_valid(lengths))["logits"]
        md = _prep(mask, logits.device)
        cu = torch.zeros(md.shape[0] + 1, dtype=torch.int32, device=logits.device)
        cu[1:] = torch.cumsum(md.sum(dim=1), 0).to(torch.int32)
        return logits, cu, int(md.shape[1])

    @torch.no_grad()
    def design(self, X, mask, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None, lengths=None, states=None,
               state_weights=None, gc_content=None, distinct=None, mutations=None, avoid=None, require=None,
               pairs=None, tree: str = "lds", combine=None):
        """``n_samples`` sequences per RNA drawn from this model's read-out at ``temperature`` and scored, in one launch of the design
        family on the PACKED logits (``design_by_mode`` with ``cu_seqlens`` built on the device from the mask; ``X``, ``mask`` as
        ``score_batch`` takes them, ``lengths`` as there).  The return, by mode (S = ``n_samples``):
        "plain" (``constraints`` or free) and "states" -> (seqs int8 (S,B,T), -1 on padding; seq_nll (S,B) f32, the model's own
        temperature-1 NLL of each draw; infeasible (B,) int32);
        and in every other mode that triple plus - "gc_content": gc_count (S,B) int32, gc_miss (B,) int32; "distinct": logp (S,B) f32,
        n_distinct (B,) int32; "mutations": n_mut (S,B) int32, mut_miss (B,) int32; "avoid": hits (S,B) int32, avoid_miss (B,) int32;
        "require": hits, accepted (S,B) int32, dfa_miss (B,) int32; ``pairs="nested"``: hits, accepted, dfa_miss, nest_miss (B,) int32;
        ``combine="chain"``: hits, accepted, count (S,B) int32, dfa_miss, count_miss (B,) int32, log_z (B,) f64.
        What each argument means, which pairings are built and what is refused - the refusals are ``RNAMPNN.design``'s, each a
        ``ValueError`` before the forward pass - stands once, on ``rnampnn.model.decode.resolve_design``."""
        mode, mutations, avoid, require = resolve_design(constraints, states, lengths, gc_content, distinct, mutations, avoid, require, pairs,
                                                         combine, tree)
        logits, cu, T = self._packed_logits(X, mask, lengths)
        return design_by_mode(mode, logits, cu_seqlens=cu, max_len=T, n_samples=n_samples, temperature=temperature, seed=seed,
                              constraints=constraints, states=states, state_weights=state_weights, gc_content=gc_content, distinct=distinct,
                              mutations=mutations, avoid=avoid, require=require, tree=tree)

    @torch.no_grad()
    def design_profile(self, X, mask, temperature: float = 0.1, constraints=None, lengths=None, gc_content=None, mutations=None, avoid=None,
                       tree: str = "lds", require=None, max_run=None, table: str = "lds"):
        """What ``design`` draws FROM under the same arguments, with one eval-mode forward and one launch on the packed logits: the exact
        per-position marginals, log partition sums and entropy of the constrained, tempered distribution (``design_profile_from_logits``)
        -> a ``DesignProfile``.  ``constraints``, ``lengths``, ``gc_content``, ``mutations`` and ``avoid`` as in ``design``; the pairings
        ``design`` refuses are refused here with the same messages, before the forward pass.  No profile is built for ``states`` or
        ``distinct``.  ``tree`` as in ``design``, for every profile but ``avoid``'s.  ``table="global"`` (``check_table``; "lds" is everything above,
        unchanged): the profile of ``require`` and / or ``avoid`` / ``max_run`` on the 256-state automaton
        (``rnampnn_design_dfa_profile``), ``miss`` = ``dfa_miss``; ``require`` without it and what it is not built with are refused
        before the forward pass."""
        resolved = resolve_profile(constraints, gc_content, mutations, avoid, tree, require, table, max_run)
        was_training = self.training
        self.eval()
        try:
            logits, cu, T = self._packed_logits(X, mask, lengths)
        finally:
            self.train(was_training)
        return design_profile_from_logits(logits, cu_seqlens=cu, max_len=T, temperature=temperature, constraints=constraints,
                                          gc_content=gc_content, tree=tree, resolved=resolved)

    @torch.no_grad()
    def score_sequences(self, X, mask, seqs, labels=None, lengths=None):
        """Likelihood of given sequences under this model: ``seqs`` (S,B,T) or (B,T) class ids (``design``'s int8 output; entries on
        padding are never read) -> (seq_nll (S,B) f32, seq_match (S,B) int32 = #(seq == label) or None without ``labels`` (B,T) class
        ids, valid (B,) int32).  One forward + one ``rnampnn_score`` on the packed logits."""
        logits, cu, T = self._packed_logits(X, mask, lengths)
        want = ("seq_nll", "valid") + (("seq_match",) if labels is not None else ())
        out = score_logits(logits, cu_seqlens=cu, labels=labels, seqs=seqs if seqs.dim() == 3 else seqs.unsqueeze(0), want=want, max_len=T)
        return out["seq_nll"], out.get("seq_match"), out["valid"]

    # ------------------------------------------------------------------ tree head (rdesign/utils/train.py:51-89, rdesign.py:151-153)
    def load_xgb_readout(self, model_json) -> None:
        """Attach a fitted multi:softmax model in XGBoost's JSON schema (path or dict) over this model's 128 ``h_V`` features.  The
        reference unpickles ``XGB-V*.pkl``; pickles are never loaded here."""
        from rnampnn.model.xgb import GBDTReadout
        self.xgb_readout = GBDTReadout.from_xgboost_json(model_json)

    @torch.no_grad()
    def embed_valid(self, batches):
        """``XGBTrainer._generate_embedding`` (rdesign/utils/train.py:75-89) without leaving the device: ``batches`` yields the loader's
        (S, X, mask, lengths, ...) -> (h_V (N, 128) f32, labels (N,) int64) packed over the valid residues."""
        dev = self._device()
        xs, ys = [], []
        for batch in batches:
            S, X, mask = batch[0], batch[1], batch[2]
            n = self._n_valid(batch[3]) if len(batch) > 3 else None
            xs.append(self._run(X, mask, want=("h_V",), n_valid=n)["h_V"])
            ys.append(S.to(dev)[mask.to(dev) == 1].to(torch.int64))
        if not xs:
            raise ValueError("embed_valid: no batches")
        return torch.cat(xs), torch.cat(ys)

    @torch.no_grad()
    def fit_xgb_readout(self, batches, seed: int = 0) -> float:
        """``XGBTrainer.on_fit_end``: embed every valid nucleotide of ``batches``, fit the tree read-out on those rows ON THE DEVICE
        (``GBDTReadout.fit``) with the five constructor hyper-parameters (``xgb_hparams``; the reference's defaults: 100 rounds, depth 6,
        0.1 / 0.8 / 0.8) and attach it.  Returns the score on the rows it was fitted on."""
        from rnampnn.model.xgb import GBDTReadout
        X, y = self.embed_valid(batches)
        hp = self.xgb_hparams
        self.xgb_readout = GBDTReadout.fit(X, y, num_class=4, n_estimators=int(hp["n_estimators"]), max_depth=int(hp["xgb_max_depth"]),
                                           learning_rate=float(hp["xgb_learning_rate"]), subsample=float(hp["xgb_subsample"]),
                                           colsample_bytree=float(hp["xgb_colsample_bytree"]), seed=int(seed))
        return self.xgb_readout.score(X, y)

    @torch.no_grad()
    def _predict_packed(self, X, mask, lengths=None) -> torch.Tensor:
        """Packed class ids (N,) on the device: ``xgb_readout.predict(h_V)`` when a tree model is attached (``rdesign.py:151-153``), else
        the argmax of the read-out from ``rdesign_score`` (ties to the lowest class)."""
        n = self._n_valid(lengths)
        if self.xgb_readout is not None:
            return self.xgb_readout.predict(self._run(X, mask, want=("h_V",), n_valid=n)["h_V"])
        logits = self._run(X, mask, want=("logits",), n_valid=n)["logits"]
        zeros = torch.zeros(mask.shape, dtype=torch.int32, device=logits.device)
        return self._score_native(logits, None, mask, zeros, want_nll=False, want_pred=True)[3]

    @torch.no_grad()
    def predict_sequences(self, X, mask, lengths=None):
        """The sequences ``predict`` writes, one string per RNA of the batch (one device-to-host copy of the packed class ids)."""
        if lengths is None:
            lengths = mask.sum(dim=1).to(torch.int64).tolist()
        return letters_packed(self._predict_packed(X, mask, lengths), lengths)

    # ------------------------------------------------------------------ training step (exact f32, or bf16-mixed by train_precision)
    def _train_args(self, dropout, seed):
        if self.train_precision == "f32" and self.precision != "f32":
            raise NotImplementedError("the exact-f32 rdesign training step (train_precision='f32', the default) is built for precision='f32' "
                                      "models only (the reference trains this model in f32); set train_precision='bf16' for the bf16-mixed step")
        p = float((self.hparams["dropout"] if self.training else 0.0) if dropout is None else dropout)
        return p, (self._next_seed() if seed is None else int(seed))

    def _augmented(self, X, mask, seed: int):
        """``X + augment_eps * randn_like(X)`` of the reference's training forward (``feature.py:157-158``) on the device: every row with
        sigma = ``augment_eps``, no keys, ``seed`` = the step's dropout seed, so the noise is fresh each step and a function of that seed
        (``rnampnn_augment_coords``).  Eval-mode calls return ``X`` untouched without looking at ``augment_eps``."""
        if not self.training or self.augment_eps <= 0.0:
            return X
        from rnampnn.utils.augment import augment_coords
        dev = self._device()
        Xd, md = _prep(X, dev), _prep(mask, dev)
        sigma = torch.full((int(Xd.shape[0]),), self.augment_eps, dtype=torch.float32, device=dev)
        return augment_coords(Xd, md, sigma, seed=seed)

    def _step_native(self, X, S, mask, p: float, seed: int, grad: torch.Tensor, return_logits: bool = False):
        """One ``rdesign_loss_and_grad_ex`` call in the arithmetic of ``train_precision``; the gradient of every parameter OVERWRITES ``grad`` (laid out like the weight arena)."""
        dev = self._ensure()
        if X.dim() != 4 or X.shape[2:] != (6, 3) or tuple(mask.shape) != tuple(X.shape[:2]) or tuple(S.shape) != tuple(mask.shape):
            raise ValueError(f"X must be (B, T, 6, 3), S and mask (B, T); got {tuple(X.shape)}, {tuple(S.shape)}, {tuple(mask.shape)}")
        B, T = int(X.shape[0]), int(X.shape[1])
        if B == 0 or T == 0:
            raise ValueError("empty batch")
        Xd, md, lab = _prep(X, dev), _prep(mask, dev), _prep(S, dev, torch.int32)
        lib = _native.lib()
        flags = _TRAIN[self.train_precision]
        need = int(lib.rdesign_train_workspace_bytes_ex(self._handle.ptr, B, T, flags))
        if need == 0:
            # refused (rows beyond the dropout hash's index range, a message depth the mixed step lacks): the step itself, asked with no
            # buffers, returns the code that goes with the text the library has set
            _native.check(lib.rdesign_loss_and_grad_ex(self._handle.ptr, None, None, None, B, T, C.c_float(p), C.c_uint64(0), flags,
                                                       None, None, None, None, C.c_size_t(0), None))
            _native.check(_native.ERR_BAD_ARG)
        if self._tws is None or self._tws.numel() < need + 256 or self._tws.device != dev:
            self._tws = None
            self._tws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = self._tws.data_ptr()
        aligned = (base + 255) // 256 * 256
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        logits = torch.zeros(B * T, 4, dtype=torch.float32, device=dev) if return_logits else None
        with torch.cuda.device(dev):
            _native.check(lib.rdesign_loss_and_grad_ex(self._handle.ptr, C.c_void_p(Xd.data_ptr()), C.c_void_p(md.data_ptr()),
                                                       C.c_void_p(lab.data_ptr()), B, T, C.c_float(p), C.c_uint64(seed & (2 ** 64 - 1)), flags,
                                                       C.c_void_p(loss.data_ptr()), C.c_void_p(logits.data_ptr()) if return_logits else None,
                                                       C.c_void_p(grad.data_ptr()), C.c_void_p(aligned),
                                                       C.c_size_t(self._tws.numel() - (aligned - base)), _stream(dev)))
        return loss, logits

    def loss_and_grad(self, X, S, mask, dropout: Optional[float] = None, seed: Optional[int] = None, return_logits: bool = False):
        """``training_step`` + ``loss.backward()`` of the reference (``rdesign.py:95-104``) in one native call (HIP kernels in the
        arithmetic of ``train_precision``, bit-reproducible): -> loss (device scalar) [, logits (N, 4) packed over the valid residues].  ``dropout``: None = the module's
        hyper-parameter in train mode and 0 in eval mode; the masks are a function of ``seed`` (None = the module's running counter,
        ``manual_seed``).  In train mode with ``augment_eps > 0`` the step sees ``X`` + N(0, augment_eps^2) noise drawn from the same seed.  Afterwards every ``p.grad`` is a view of ONE flat buffer ``self.flat_grad`` (OVERWRITTEN), so a
        data-parallel job averages gradients with one ``dist.all_reduce(model.flat_grad)``."""
        p, sd = self._train_args(dropout, seed)
        dev = self._ensure()
        self._bind_flat_grad(dev)
        loss, logits = self._step_native(self._augmented(X, mask, sd), S, mask, p, sd, self.flat_grad, return_logits)
        if return_logits:
            self._check_mask(mask)
            return loss, logits[:int(mask.sum().item())]
        return loss

    def training_step(self, batch):
        """``rdesign.py:95-104``: -> scalar loss carrying an autograd node; ``loss.backward()`` ACCUMULATES the HIP gradient, scaled by
        the incoming gradient, into ``p.grad`` (views of ``flat_grad``) until ``zero_grad``."""
        X, S, mask, lengths, _ = batch
        p, sd = self._train_args(None, None)
        self._ensure()
        X = self._augmented(X, mask, sd)
        if not torch.is_grad_enabled():
            return self._step_native(X, S, mask, p, sd, torch.empty_like(self._flat))[0]
        return _TrainStep.apply(self, X, S, mask, p, sd, *[q for q, _, _ in self._slices])

    def _eval_step(self, batch, store, loss_key):
        X, S, mask, lengths, _ = batch
        out = self._run(X, mask, want=("logits",))
        logits = out["logits"]
        S_p = torch.masked_select(S.to(logits.device), mask.to(logits.device) == 1)
        loss = self.loss_fn(logits, S_p)
        correct = (logits.argmax(dim=-1) == S_p).to(torch.float32)
        rates, start = [], 0
        for n in [int(v) for v in lengths]:
            rates.append(float(correct[start:start + n].sum() / n)); start += n
        store[loss_key].append(loss * correct.shape[0])
        store["correct"].append(correct.sum(dim=-1).item())
        store["len"].append(correct.shape[0])
        store["recovery_rates"] += rates
        return loss, rates

    def validation_step(self, batch):
        loss, rates = self._eval_step(batch, self.val_step_outputs, "val_loss")
        return {"validation loss": loss, "recovery_rates": rates}

    def test_step(self, batch):
        loss, rates = self._eval_step(batch, self.test_step_outputs, "test_loss")
        return {"test loss": loss, "recovery_rates": rates}

    def predict(self, batch, batch_id, output_dir, filename):
        """``rdesign.py:143-173``: the classes of the attached tree read-out, or - the reference's branch for an unfitted XGBoost head -
        the argmax of the read-out; one CSV row per RNA."""
        self.eval()
        X, S, mask, lengths, pdb_ids = batch
        if self.xgb_readout is not None:
            samples = self._predict_packed(X, mask).tolist()
        else:
            samples = self._run(X, mask, want=("logits",))["logits"].argmax(dim=-1).tolist()
        os.makedirs(output_dir, exist_ok=True)
        start = 0
        with open(os.path.join(output_dir, filename), "a") as f:
            if batch_id == 0:
                f.write("pdb_id,seq\n")
            for length, pdb_id in zip(lengths, pdb_ids):
                n = int(length)
                f.write(f"{pdb_id},{''.join('AUCG'[i] for i in samples[start:start + n])}\n")
                start += n
