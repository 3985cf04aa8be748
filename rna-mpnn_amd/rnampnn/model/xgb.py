"""Device-side gradient-boosted-tree read-out: stands in for the reference's fitted
``xgb.XGBClassifier`` (``rnampnn/model/rnampnn.py:136-145``; ``self.xgb_readout.predict(embedding)``, ``:297-298``).

PARITY UNPINNED: xgboost (``requirements.txt``: ``xgboost~=2.1.1``) is not installed in the build image and the reference ships no
fitted model (its ``XGB-V*.pkl`` is a pickle, which this project never loads), so no XGBoost-produced vector backs this path.  What is
implemented is XGBoost's published prediction rule for ``gbtree`` / ``multi:softmax`` models, read from XGBoost's JSON model format
(``Booster.save_model("model.json")`` - a maintainer converts the pickle once with xgboost installed):

    learner.learner_model_param.{num_class, num_feature, base_score}
    learner.gradient_booster.model.tree_info[t]                      class of tree t
    learner.gradient_booster.model.trees[t].{left_children, right_children, split_indices, split_conditions, default_left}

(left child -1 = leaf, whose value sits in ``split_conditions``; go left iff ``x[f] < split_condition``, NaN follows ``default_left``).

``GBDTReadout.fit`` grows such a model on the device (``rnampnn_gbdt_fit``, csrc/gbdt_fit.hip): a histogram-method
trainer that restates XGBoost's published multi:softmax gradients, split gain and leaf weights with this project's own cuts, binning and
sampling - equally unpinned against XGBoost, and exact against its numpy restatement.  ``to_xgboost_json`` / ``save_json`` write the
schema above, so a fitted model round-trips through ``parse_xgboost_json``.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Sequence, Union

import numpy as np
import torch

from .. import _native
from ._base import _stream


def parse_xgboost_json(model: Union[str, dict]) -> dict:
    """XGBoost JSON model (path or parsed dict) -> flat arrays (see the module docstring for the fields read)."""
    if isinstance(model, str):
        with open(model) as f:
            model = json.load(f)
    learner = model["learner"]
    lp = learner["learner_model_param"]
    gb = learner["gradient_booster"]
    if gb.get("name", "gbtree") != "gbtree":
        raise NotImplementedError(f"booster '{gb.get('name')}' is not supported (gbtree only)")
    m = gb["model"]
    trees = m["trees"]
    num_class = max(int(lp.get("num_class", "0")), 1)
    for t in trees:
        if t.get("categories_nodes"):
            raise NotImplementedError("categorical splits are not supported")
    offs = np.zeros(len(trees) + 1, np.int32)
    offs[1:] = np.cumsum([len(t["left_children"]) for t in trees])
    cat = lambda key, dt: np.concatenate([np.asarray(t[key], dtype=dt) for t in trees])
    return dict(num_class=num_class, num_feature=int(lp["num_feature"]), base_score=float(lp.get("base_score", "0.5")),
                tree_offsets=offs, tree_class=np.asarray(m["tree_info"], np.int32),
                left_children=cat("left_children", np.int32), right_children=cat("right_children", np.int32),
                split_indices=cat("split_indices", np.int32), split_conditions=cat("split_conditions", np.float32),
                default_left=cat("default_left", np.uint8))


_ARRAY_KEYS = ("tree_offsets", "tree_class", "left_children", "right_children", "split_indices", "split_conditions", "default_left")
N_CUTS_MAX = 255


def to_xgboost_json(arrays: dict) -> dict:
    """Flat arrays -> a dict in XGBoost's JSON model schema (the fields ``parse_xgboost_json`` reads; floats are written through
    ``float(np.float32)``, whose shortest repr parses back to the same float32)."""
    off = np.asarray(arrays["tree_offsets"])
    trees = []
    for t in range(len(off) - 1):
        sl = slice(int(off[t]), int(off[t + 1]))
        trees.append(dict(left_children=[int(v) for v in arrays["left_children"][sl]], right_children=[int(v) for v in arrays["right_children"][sl]],
                          split_indices=[int(v) for v in arrays["split_indices"][sl]],
                          split_conditions=[float(np.float32(v)) for v in arrays["split_conditions"][sl]],
                          default_left=[int(v) for v in arrays["default_left"][sl]], categories_nodes=[]))
    return {"learner": {"learner_model_param": {"num_class": str(int(arrays["num_class"])), "num_feature": str(int(arrays["num_feature"])),
                                                "base_score": repr(float(np.float32(arrays["base_score"])))},
                        "objective": {"name": "multi:softmax"},
                        "gradient_booster": {"name": "gbtree", "model": {"tree_info": [int(v) for v in arrays["tree_class"]], "trees": trees}}}}


def quantile_cuts(X: torch.Tensor, max_bin: int = 256):
    """The fit's cuts, with torch on X's device: per feature the ascending distinct values
    ``v[floor(i * N / max_bin)]``, i = 1 .. max_bin - 1, of the sorted column ``v``, without any equal to ``v[0]``.
    -> cuts (F, 255) f32 (unused entries 0), n_cuts (F) i32."""
    N, F = X.shape
    v = torch.sort(X, dim=0).values
    idx = (torch.arange(1, max_bin, dtype=torch.int64, device=X.device) * N) // max_bin
    cand = v[idx] + 0.0                                               # (max_bin - 1, F); a zero cut is stored as +0.0
    keep = cand != v[0:1]
    keep[1:] &= cand[1:] != cand[:-1]
    order = torch.sort((~keep).to(torch.int8), dim=0, stable=True).indices      # kept candidates first, in their order
    n_cuts = keep.sum(0).to(torch.int32)
    packed = torch.gather(cand, 0, order)
    packed = torch.where(torch.arange(max_bin - 1, device=X.device)[:, None] < n_cuts[None, :], packed, torch.zeros_like(packed))
    cuts = torch.zeros(F, N_CUTS_MAX, dtype=torch.float32, device=X.device)
    cuts[:, :max_bin - 1] = packed.t()
    return cuts.contiguous(), n_cuts.contiguous()


def _gbdt_check(rc: int) -> None:
    if rc != 0:
        msg = _native.lib().rnampnn_gbdt_last_error().decode()
        raise {_native.ERR_BAD_ARG: ValueError, _native.ERR_UNSUPPORTED: NotImplementedError}.get(rc, RuntimeError)(msg)


def _export(handle) -> dict:
    """``rnampnn_gbdt_export``: sizes, then the seven arrays."""
    L = _native.lib()
    nt, nn, nc, nf, bs = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
    _gbdt_check(L.rnampnn_gbdt_export(handle, C.byref(nt), C.byref(nn), C.byref(nc), C.byref(nf), C.byref(bs), *([None] * 7)))
    a = dict(tree_offsets=np.zeros(nt.value + 1, np.int32), tree_class=np.zeros(nt.value, np.int32), left_children=np.zeros(nn.value, np.int32),
             right_children=np.zeros(nn.value, np.int32), split_indices=np.zeros(nn.value, np.int32),
             split_conditions=np.zeros(nn.value, np.float32), default_left=np.zeros(nn.value, np.uint8))
    _gbdt_check(L.rnampnn_gbdt_export(handle, None, None, None, None, None, *[a[k].ctypes.data_as(C.c_void_p) for k in _ARRAY_KEYS]))
    a.update(num_class=nc.value, num_feature=nf.value, base_score=float(bs.value))
    return a


class GBDTReadout:
    """``predict(embedding)`` of a fitted multi:softmax XGBoost model on the MI355X (``rnampnn_gbdt_*``, csrc/gbdt.hip), and ``fit``,
    which grows one there (csrc/gbdt_fit.hip)."""

    def __init__(self, arrays: dict, _handle=None):
        if _handle is not None:                 # a model the device just fitted: the handle is the model, the arrays are its export
            self._h = _handle
            self.arrays = arrays
            self.num_class, self.num_feature = int(arrays["num_class"]), int(arrays["num_feature"])
            return
        self.arrays = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}
        a = self.arrays
        self.num_class, self.num_feature = int(a["num_class"]), int(a["num_feature"])
        self._h = C.c_void_p()
        p = lambda k: a[k].ctypes.data_as(C.c_void_p)
        rc = _native.lib().rnampnn_gbdt_create(len(a["tree_class"]), self.num_class, self.num_feature, float(a["base_score"]),
                                               p("tree_offsets"), p("tree_class"), p("left_children"), p("right_children"),
                                               p("split_indices"), p("split_conditions"), p("default_left"), C.byref(self._h))
        if rc != 0:
            msg = _native.lib().rnampnn_gbdt_last_error().decode()
            raise (ValueError if rc == _native.ERR_BAD_ARG else RuntimeError)(msg)

    @classmethod
    def from_xgboost_json(cls, model: Union[str, dict]) -> "GBDTReadout":
        return cls(parse_xgboost_json(model))

    @classmethod
    def fit(cls, X: torch.Tensor, y: torch.Tensor, *, num_class: int = 4, n_estimators: int = 150, max_depth: int = 8,
            learning_rate: float = 0.1, subsample: float = 0.8, colsample_bytree: float = 0.8, reg_lambda: float = 1.0, gamma: float = 0.0,
            min_child_weight: float = 1.0, max_bin: int = 256, base_score: float = 0.5, seed: int = 0) -> "GBDTReadout":
        """``XGBClassifier(objective='multi:softmax', ...).fit(X, y)`` restated on the device (parity unpinned).
        X (N, F) float CUDA tensor, all finite; y (N) integer CUDA tensor in [0, num_class).  Bit-reproducible for one seed."""
        if X.device.type != "cuda" or y.device.type != "cuda":
            raise RuntimeError("the GBDT fit runs on an MI355X: pass CUDA tensors (there is no CPU fallback)")
        if X.dim() != 2 or y.dim() != 1 or y.shape[0] != X.shape[0] or X.shape[0] < 1:
            raise ValueError(f"X must be (N, F) and y (N), got {tuple(X.shape)} and {tuple(y.shape)}")
        if not 2 <= int(max_bin) <= 256:
            raise ValueError("max_bin must be 2..256 (a bin is one byte)")
        X = X.detach().to(torch.float32)
        if X.stride(1) != 1:
            X = X.contiguous()
        if not bool(torch.isfinite(X).all()):
            raise ValueError("X holds a non-finite value (the fit has no missing-value handling)")
        y32 = y.detach().to(torch.int32).contiguous()
        n, f = int(X.shape[0]), int(X.shape[1])
        params = _native.GbdtParams(num_class=int(num_class), n_estimators=int(n_estimators), max_depth=int(max_depth), max_bin=int(max_bin),
                                    learning_rate=float(learning_rate), subsample=float(subsample), colsample_bytree=float(colsample_bytree),
                                    reg_lambda=float(reg_lambda), gamma=float(gamma), min_child_weight=float(min_child_weight),
                                    base_score=float(base_score), seed=int(seed) & (2 ** 64 - 1))
        handle = C.c_void_p()
        with torch.cuda.device(X.device):
            cuts, n_cuts = quantile_cuts(X, int(max_bin))
            _gbdt_check(_native.lib().rnampnn_gbdt_fit(C.byref(params), C.c_void_p(X.data_ptr()), n, int(X.stride(0)), f,
                                                       C.c_void_p(y32.data_ptr()), C.c_void_p(cuts.data_ptr()), C.c_void_p(n_cuts.data_ptr()),
                                                       _stream(X.device), C.byref(handle)))
        try:
            arrays = _export(handle)
        except Exception:
            _native.lib().rnampnn_gbdt_destroy(handle)
            raise
        return cls(arrays, _handle=handle)

    def to_xgboost_json(self) -> dict:
        return to_xgboost_json(self.arrays)

    def save_json(self, path: str) -> None:
        with open(path, "w") as fh:
            json.dump(self.to_xgboost_json(), fh)

    def score(self, X: torch.Tensor, y: torch.Tensor) -> float:
        """``XGBClassifier.score``: the fraction of rows whose predicted class equals ``y``."""
        pred = self.predict(X).reshape(-1)
        return int((pred == y.reshape(-1).to(pred.device, torch.int64)).sum()) / max(int(pred.numel()), 1)

    def _run(self, x: torch.Tensor, want_margin: bool):
        if x.device.type != "cuda":
            raise RuntimeError("the GBDT read-out runs on an MI355X: pass a CUDA tensor (there is no CPU fallback)")
        x = x.detach().to(torch.float32)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        if x2.shape[1] < self.num_feature:
            raise ValueError(f"model expects {self.num_feature} features, got {x2.shape[1]}")
        n = int(x2.shape[0])
        pred = torch.empty(n, dtype=torch.int32, device=x.device)
        margin = torch.empty(n, self.num_class, dtype=torch.float32, device=x.device) if want_margin else None
        with torch.cuda.device(x.device):
            rc = _native.lib().rnampnn_gbdt_predict(self._h, C.c_void_p(x2.data_ptr()), n, int(x2.shape[1]),
                                                    C.c_void_p(margin.data_ptr()) if want_margin else None,
                                                    C.c_void_p(pred.data_ptr()), _stream(x.device))
        if rc != 0:
            raise RuntimeError(_native.lib().rnampnn_gbdt_last_error().decode())
        return pred.reshape(x.shape[:-1]).to(torch.int64), (margin.reshape(*x.shape[:-1], self.num_class) if want_margin else None)

    def predict(self, embedding: torch.Tensor) -> torch.Tensor:
        """``XGBClassifier.predict``: class ids, shape ``embedding.shape[:-1]``."""
        return self._run(embedding, False)[0]

    def margins(self, embedding: torch.Tensor) -> torch.Tensor:
        """``predict(output_margin=True)``: per-class sums of the leaf values (+ base_score)."""
        return self._run(embedding, True)[1]

    def close(self):
        if self._h:
            _native.lib().rnampnn_gbdt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
