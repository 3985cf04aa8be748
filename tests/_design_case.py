"""What the GPU tests of the five design entries (``test_design*_gpu.py``) share: byte views, uploads, the raw call of a C entry, and the
small models, constraint specs, data directory and checkpoints of their end-to-end tests.  A plain module like ``_design_ref.py``; the
float64 restatements (``_design_*_ref.py``) are the yardsticks and hold none of this."""
import ctypes as C
import os

import numpy as np
import torch

SMALL = dict(num_res_neighbours=6, num_res_mpnn_layers=2, padding_len=128)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x, dtype=dtype).contiguous().cuda()


def design_outputs(further, S, B, T):
    """The outputs of a design entry: seqs, seq_nll, infeasible and ``further`` = its own ((name, dtype, per sample ?), ...), in ABI order."""
    out = dict(seqs=torch.empty(S, B, T, dtype=torch.int8, device="cuda"), seq_nll=torch.empty(S, B, dtype=torch.float32, device="cuda"),
               infeasible=torch.empty(B, dtype=torch.int32, device="cuda"))
    for name, dtype, per_sample in further:
        out[name] = torch.empty(*((S, B) if per_sample else (B,)), dtype=dtype, device="cuda")
    return out


def raw_design(entry, own, further, logits, mask=None, cu=None, T=None, temperature=1.0, S=8, seed=0, allowed=None, partner=None, wobble=True,
               bias=None, seed_dev=None, out=None):
    """The C entry ``entry`` on device tensors (numpy arrays are uploaded) -> dict of its outputs.  ``own``: the entry's own arguments
    between the bias and the outputs, device tensors or scalars; ``further``: its outputs past ``infeasible`` (``design_outputs``)."""
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    lg, m, c = _dev(logits, torch.float32), _dev(mask, torch.float32), _dev(cu, torch.int32)
    B = int(m.shape[0]) if m is not None else int(c.numel()) - 1
    T = int(m.shape[1]) if m is not None else int(T)
    al, pa, bi = _dev(allowed, torch.uint8), _dev(partner, torch.int32), _dev(bias, torch.float32)
    out = design_outputs(further, S, B, T) if out is None else out
    _native.check(getattr(_native.lib(), entry)(
        _ptr(lg), int(lg.numel()) // 4, _ptr(m), _ptr(c), B, T, float(temperature), S, C.c_uint64(seed), _ptr(seed_dev), _ptr(al), _ptr(pa),
        int(wobble), _ptr(bi), int(bi is not None and bi.dim() == 3), *[_ptr(v) if torch.is_tensor(v) else v for v in own],
        *[_ptr(out[k]) for k in ("seqs", "seq_nll", "infeasible") + tuple(f[0] for f in further)], _stream(lg.device)))
    return out


def _specs():
    return [("GNRA" + "." * 29, "((((....))))" + "." * 21), (None, "(((..[[[)))....]]].."), ("." * 40 + "U", None)]


def _write_data(root, ids, lens):
    from rnampnn.utils import synth
    os.makedirs(root / "coords"); os.makedirs(root / "seqs")
    for i, (rid, n) in enumerate(zip(ids, lens)):
        np.save(root / "coords" / f"{rid}.npy", synth.synth_rna(n, 40 + i, seed=3))
        (root / "seqs" / f"{rid}.fasta").write_text(f">{rid}\n" + "".join("AUCG"[v] for v in synth.synth_labels(n, 40 + i, seed=3)) + "\n")


def _checkpoint(family, path):
    torch.manual_seed(0)
    if family == "rnampnn":
        from rnampnn.model.rnampnn import RNAMPNN
        from rnampnn.utils.train import save_checkpoint
        save_checkpoint(path, RNAMPNN(precision="f32", **SMALL))
    else:
        from rdesign.model.rdesign import RNAModel
        from rdesign.utils.train import save_checkpoint
        save_checkpoint(path, RNAModel(num_mpnn_layers=1))
