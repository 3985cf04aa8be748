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


PROFILE_OUTPUTS = ("marginals", "log_z", "log_z_free", "entropy", "infeasible", "miss")
PROFILE_SCALARS = ("log_z", "log_z_free", "entropy")


def profile_outputs(B, T):
    """The six outputs of a profile entry, in ABI order."""
    out = dict(marginals=torch.empty(B, T, 4, dtype=torch.float64, device="cuda"))
    for k in PROFILE_SCALARS:
        out[k] = torch.empty(B, dtype=torch.float64, device="cuda")
    out["infeasible"], out["miss"] = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
    return out


def raw_profile(entry, own, logits, mask=None, cu=None, T=None, temperature=1.0, allowed=None, partner=None, wobble=True, bias=None, out=None):
    """The C profile entry ``entry`` on device tensors (numpy arrays are uploaded) -> dict of its six outputs.  ``own``: the entry's own
    arguments between the bias and the outputs, tensors (on the device, or on the host where the ABI reads them there) or scalars."""
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    lg, m, c = _dev(logits, torch.float32), _dev(mask, torch.float32), _dev(cu, torch.int32)
    B = int(m.shape[0]) if m is not None else int(c.numel()) - 1
    T = int(m.shape[1]) if m is not None else int(T)
    al, pa, bi = _dev(allowed, torch.uint8), _dev(partner, torch.int32), _dev(bias, torch.float32)
    out = profile_outputs(B, T) if out is None else out
    _native.check(getattr(_native.lib(), entry)(
        _ptr(lg), int(lg.numel()) // 4, _ptr(m), _ptr(c), B, T, float(temperature), _ptr(al), _ptr(pa), int(wobble), _ptr(bi),
        int(bi is not None and bi.dim() == 3), *[_ptr(v) if torch.is_tensor(v) else v for v in own], *[_ptr(out[k]) for k in PROFILE_OUTPUTS],
        _stream(lg.device)))
    return out


def agree_profile(out, ref, what, rows=None, flags=True, tol=1e-8):
    """Device outputs within ``tol`` of the reference's (a restatement's dict or another entry's outputs): the marginals absolutely, the
    scalars relative to max(1, |value|); with ``flags`` the two int outputs exactly.  Prints and returns the observed maxima."""
    ref = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in ref.items() if k in PROFILE_OUTPUTS}
    rows = list(range(len(ref["log_z"]))) if rows is None else rows
    got = {k: out[k].cpu().numpy() for k in PROFILE_OUTPUTS}
    dm = float(np.abs(got["marginals"][rows] - ref["marginals"][rows]).max())
    ds = {k: float((np.abs(got[k][rows] - ref[k][rows]) / np.maximum(1.0, np.abs(ref[k][rows]))).max()) for k in PROFILE_SCALARS}
    print(f"{what}: max |dP| = {dm:.3e}, scalars relative to max(1, |value|): " + ", ".join(f"{k} {v:.3e}" for k, v in ds.items()))
    assert dm <= tol, what
    assert all(v <= tol for v in ds.values()), (what, ds)
    if flags:
        assert got["infeasible"][rows].tolist() == ref["infeasible"][rows].tolist() and got["miss"][rows].tolist() == ref["miss"][rows].tolist()
    return dm, ds


def same_profile(a, b, rows=None):
    """The six outputs of two profiles (dicts or ``DesignProfile``s as dicts), byte for byte, on ``rows`` or everywhere."""
    return all(_bytes(a[k] if rows is None else a[k][rows]) == _bytes(b[k] if rows is None else b[k][rows]) for k in PROFILE_OUTPUTS)


def one_rna(n, seed):
    """(logits (1,n,4) f32, mask (1,n)) of one RNA of n nucleotides, on the host."""
    rng = np.random.RandomState(seed)
    return (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32), np.ones((1, n), dtype=np.float32)


def dfa_workspace(symbol, B, T, live, *sizes, fill=None, need=None):
    """The workspace of an entry of the dfa family: ``symbol``(B, T, live, *sizes) bytes, which must be ``need`` - the formula
    include/rnampnn_hip.h gives, 8 B T live for the one table of rnampnn_design_dfa and its profile; ``fill``: a byte to fill it with."""
    from rnampnn import _native
    got = int(getattr(_native.lib(), symbol)(B, T, live, *sizes))
    assert got == (8 * B * T * live if need is None else need)
    ws = torch.empty(got, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


DFA_FURTHER = (("hits", torch.int32, True), ("accepted", torch.int32, True), ("dfa_miss", torch.int32, False))


def design_dfa(logits, delta, kind, seed, S, ws=None, **kw):
    """``rnampnn_design_dfa`` on device tensors (numpy arrays are uploaded; ``kind`` stays on the host) -> dict of its six outputs."""
    kind = torch.as_tensor(np.ascontiguousarray(kind), dtype=torch.uint8).contiguous()
    m, cu = kw.get("mask"), kw.get("cu")
    B = int(m.shape[0]) if m is not None else int(cu.shape[0]) - 1
    T = int(m.shape[1]) if m is not None else int(kw["T"])
    ws = dfa_workspace("rnampnn_design_dfa_workspace_bytes", B, T, int(((kind & 1) == 0).sum())) if ws is None else ws
    return raw_design("rnampnn_design_dfa", (_dev(delta, torch.uint8), kind, int(kind.numel()), ws, C.c_size_t(ws.numel())), DFA_FURTHER, logits,
                      seed=seed, S=S, **kw)


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
