"""Decoding from logits, as free functions over the C ABI's decode family: argmax + recovery (``rnampnn_argmax_recovery``), free draws
(``rnampnn_sample``), scores (``rnampnn_score``), constrained and multi-state design (``rnampnn_design``, ``rnampnn_design_tied``), design
under a G+C content window (``rnampnn_design_gc``), distinct designs (``rnampnn_design_distinct``) and the letters of class ids.  Needs the library and ``_base`` only, so both model
packages import it at module level."""
from __future__ import annotations

import ctypes as C
import itertools
from typing import Dict, List, Optional, Tuple

import torch

from .. import _native
from ..config.glob import REVERSE_VOCAB
from ._base import _prep, _ptr, _stream


def _seed64(seed: int) -> C.c_uint64:
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


def _layout(logits, mask, cu_seqlens, shaped, max_len):
    """The padded (``mask``) or packed (``cu_seqlens``) layout of f32 logits -> (logits, mask, cu, B, T) as the library takes them.
    (B, T) is the mask's shape; without a mask T is ``max_len`` when given, else the last extent of the first tensor in ``shaped``."""
    device = logits.device
    lg = _prep(logits, device)
    m = None if mask is None else _prep(mask, device)
    cu = None if cu_seqlens is None else _prep(cu_seqlens, device, torch.int32)
    if m is not None:
        return lg, m, cu, int(m.shape[0]), int(m.shape[1])
    T = int(max_len) if max_len is not None else next((int(t.shape[-1]) for t in shaped if t is not None), 0)
    return lg, m, cu, (int(cu.numel()) - 1) if cu is not None else int(lg.shape[0]), T


def _check_logits(lg, m, B: int, T: int) -> None:
    if lg.shape[-1] != 4 or lg.numel() < (4 * B * T if m is not None else 0):
        raise ValueError(f"logits must be (B, T, 4) with the mask or (N, 4) with cu_seqlens, got {tuple(lg.shape)}")


def _state_counts(states, B: int) -> List[int]:
    counts = [int(v) for v in states]
    if any(v < 0 for v in counts) or sum(counts) != B:
        raise ValueError(f"states must be non-negative row counts that sum to B = {B}, got {counts}")
    return counts


def argmax_recovery(logits: torch.Tensor, mask: torch.Tensor, labels: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """HIP decode kernel: (pred int8 (B,T) with -1 on padding, correct int32 (B,), valid int32 (B,))."""
    device = logits.device
    B, T = int(logits.shape[0]), int(logits.shape[1])
    lg, m = _prep(logits, device), _prep(mask, device)
    lab = None if labels is None else _prep(labels, device, torch.int32)
    pred = torch.empty(B, T, dtype=torch.int8, device=device)
    correct = torch.zeros(B, dtype=torch.int32, device=device)
    nvalid = torch.zeros(B, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _native.check(_native.lib().rnampnn_argmax_recovery(_ptr(lg), _ptr(m), _ptr(lab), B, T, _ptr(pred),
                                                            _ptr(correct), _ptr(nvalid), _stream(device)))
    return pred, correct, nvalid


def sample_from_logits(logits: torch.Tensor, mask: torch.Tensor, temperature: float, n_samples: int, seed: int = 0) -> torch.Tensor:
    device = logits.device
    B, T = int(logits.shape[0]), int(logits.shape[1])
    lg, m = _prep(logits, device), _prep(mask, device)
    out = torch.empty(n_samples, B, T, dtype=torch.int8, device=device)
    with torch.cuda.device(device):
        _native.check(_native.lib().rnampnn_sample(_ptr(lg), _ptr(m), B, T, float(temperature), int(n_samples), _seed64(seed), _ptr(out),
                                                   _stream(device)))
    return out


def check_state_lengths(states, lengths) -> None:
    """Multi-state design: the states of a group are conformers of ONE RNA.  ``ValueError`` naming the group when ``states`` does not
    partition the rows or a group's rows differ in length."""
    lo = 0
    for g, k in enumerate(_state_counts(states, len(lengths))):
        if len({int(n) for n in lengths[lo:lo + k]}) > 1:
            raise ValueError(f"group {g} (rows {lo}..{lo + k - 1}): its states differ in length {[int(n) for n in lengths[lo:lo + k]]}")
        lo += k


def design_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                       max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                       states=None, state_weights=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rnampnn_design`` (include/rnampnn_hip.h): ``n_samples`` constrained draws per RNA from f32 logits and their scores in one launch
    -> (seqs int8 (S,B,T), -1 on padding; seq_nll (S,B) f32 = ``score_logits``' ``seq_nll`` of the draws; infeasible (B,) int32).  Padded
    layout: logits (B,T,4) + ``mask`` (B,T); packed layout: logits (N,4) + ``cu_seqlens`` (B+1), the padded extent T from the constraints'
    tensors or ``max_len``.  ``constraints``: a ``DesignConstraints`` (padded (B,T) tensors in both layouts) or None for a free draw.
    ``states``: multi-state design (``rnampnn_design_tied``) - a sequence of row counts, one per group, that sums to B; the consecutive rows
    of a group are the states (conformers, the backbones of a switch) of ONE design: they receive the same sequence, drawn exactly from the
    product of their distributions under the union of their base-pair tables; ``seq_nll`` stays per row, ``infeasible`` is the group's count
    on each of its rows.  ``state_weights`` (B,) per row (default 1; negative = design against that state).  ``None`` keeps ``rnampnn_design``.
    CUDA logits only (there is no CPU fallback); no host synchronisation."""
    device = logits.device
    if device.type != "cuda":
        raise RuntimeError("rnampnn_design runs on an MI355X: pass CUDA logits (there is no CPU fallback)")
    c = constraints
    al = None if c is None or c.allowed is None else _prep(c.allowed, device, torch.uint8)
    pa = None if c is None or c.partner is None else _prep(c.partner, device, torch.int32)
    bi = None if c is None or c.bias is None else _prep(c.bias, device)
    lg, m, cu, B, T = _layout(logits, mask, cu_seqlens, (al, pa), max_len)
    for name, t in (("allowed", al), ("partner", pa)):
        if t is not None and tuple(t.shape) != (B, T):
            raise ValueError(f"constraints.{name} must be padded to (B, T) = {(B, T)}, got {tuple(t.shape)}")
    per_position = int(bi is not None and tuple(bi.shape) == (B, T, 4))
    if bi is not None and not per_position and tuple(bi.shape) != (4,):
        raise ValueError(f"constraints.bias must be (4,) or (B, T, 4) = {(B, T, 4)}, got {tuple(bi.shape)}")
    _check_logits(lg, m, B, T)
    S = int(n_samples)
    seqs = torch.empty(max(S, 0), max(B, 0), max(T, 0), dtype=torch.int8, device=device)
    nll = torch.empty(max(S, 0), max(B, 0), dtype=torch.float32, device=device)
    bad = torch.empty(max(B, 0), dtype=torch.int32, device=device)
    rows = (_ptr(lg), int(lg.numel()) // 4, _ptr(m), _ptr(cu), B, T)
    draw = (float(temperature), S, _seed64(seed), None, _ptr(al), _ptr(pa), int(bool(c.wobble)) if c is not None else 1, _ptr(bi),
            per_position, _ptr(seqs), _ptr(nll), _ptr(bad), _stream(device))
    if states is None and state_weights is not None:
        raise ValueError("state_weights belong to multi-state design: pass states as well")
    if states is None:
        with torch.cuda.device(device):
            _native.check(_native.lib().rnampnn_design(*rows, *draw))
        return seqs, nll, bad
    counts = _state_counts(states, B)
    gcu = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32).to(device, non_blocking=True)
    sw = None if state_weights is None else _prep(torch.as_tensor(state_weights, dtype=torch.float32), device)
    if sw is not None and tuple(sw.shape) != (B,):
        raise ValueError(f"state_weights must be (B,) = {(B,)}, got {tuple(sw.shape)}")
    with torch.cuda.device(device):
        _native.check(_native.lib().rnampnn_design_tied(*rows, _ptr(gcu), len(counts), _ptr(sw), *draw))
    return seqs, nll, bad


def gc_fractions(gc_content, B: int) -> torch.Tensor:
    """``gc_content`` - a pair of fractions for every RNA, or a (B,2) tensor - -> (B,2) f64 on its own device.  ``ValueError`` for another
    shape; a host value is also checked for fractions outside [0, 1] and lo > hi (a device tensor is not read here: the kernel clamps)."""
    fr = gc_content if torch.is_tensor(gc_content) else torch.as_tensor([float(v) for v in gc_content], dtype=torch.float64)
    fr = fr.to(torch.float64)
    if tuple(fr.shape) == (2,):
        fr = fr.expand(B, 2)
    if tuple(fr.shape) != (B, 2):
        raise ValueError(f"gc_content must be a pair (lo, hi) of fractions or a (B, 2) = {(B, 2)} tensor, got {tuple(fr.shape)}")
    if fr.device.type == "cpu":
        if not bool(((fr >= 0) & (fr <= 1)).all()):
            raise ValueError(f"gc_content holds fractions of the length: they must lie in [0, 1]")
        if bool((fr[:, 0] > fr[:, 1]).any()):
            raise ValueError("gc_content: lo > hi")
    return fr


def gc_counts(fractions: torch.Tensor, lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(B,2) fractions and (B,) lengths on one device -> the window in absolute counts, int32: lo = ceil(f_lo n - 1e-6),
    hi = floor(f_hi n + 1e-6) (the slack keeps 0.5 * 12 = 6 whatever the rounding of the product)."""
    n = lengths.to(torch.float64)
    lo = torch.ceil(fractions[:, 0].to(torch.float64) * n - 1e-6)
    hi = torch.floor(fractions[:, 1].to(torch.float64) * n + 1e-6)
    return lo.to(torch.int32).contiguous(), hi.to(torch.int32).contiguous()


def design_gc_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                          max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                          gc_content=(0.0, 1.0)) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rnampnn_design_gc`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` conditioned exactly on the G+C content of every
    RNA lying in a window, in one launch -> (seqs, seq_nll, infeasible, gc_count (S,B) int32 = C or G ids written, gc_miss (B,) int32 = 0
    when the window is reachable under the constraints, else its distance to the nearest reachable count, which the draws then hold).
    Layouts and ``constraints`` as in ``design_from_logits``.  ``gc_content``: a pair of fractions (lo, hi) in [0, 1] for every RNA, or a
    (B,2) tensor of them (float64: a float32 fraction carries its rounding into f * n); the counts are formed on the device from the mask
    or ``cu_seqlens`` (``gc_counts``), without a host synchronisation.  Fractions outside [0, 1] or lo > hi raise ``ValueError`` (a device
    tensor is not read back for that: the kernel clamps it).  CUDA logits only (there is no CPU fallback)."""
    device = logits.device
    if device.type != "cuda":
        raise RuntimeError("rnampnn_design_gc runs on an MI355X: pass CUDA logits (there is no CPU fallback)")
    c = constraints
    al = None if c is None or c.allowed is None else _prep(c.allowed, device, torch.uint8)
    pa = None if c is None or c.partner is None else _prep(c.partner, device, torch.int32)
    bi = None if c is None or c.bias is None else _prep(c.bias, device)
    lg, m, cu, B, T = _layout(logits, mask, cu_seqlens, (al, pa), max_len)
    for name, t in (("allowed", al), ("partner", pa)):
        if t is not None and tuple(t.shape) != (B, T):
            raise ValueError(f"constraints.{name} must be padded to (B, T) = {(B, T)}, got {tuple(t.shape)}")
    per_position = int(bi is not None and tuple(bi.shape) == (B, T, 4))
    if bi is not None and not per_position and tuple(bi.shape) != (4,):
        raise ValueError(f"constraints.bias must be (4,) or (B, T, 4) = {(B, T, 4)}, got {tuple(bi.shape)}")
    _check_logits(lg, m, B, T)
    fr = gc_fractions(gc_content, max(B, 0)).to(device, non_blocking=True)
    lengths = (m.sum(dim=1) + 0.5).floor() if m is not None else (cu[1:] - cu[:-1]).clamp(0, max(T, 0))
    lo, hi = gc_counts(fr, lengths)
    S = int(n_samples)
    seqs = torch.empty(max(S, 0), max(B, 0), max(T, 0), dtype=torch.int8, device=device)
    nll = torch.empty(max(S, 0), max(B, 0), dtype=torch.float32, device=device)
    bad = torch.empty(max(B, 0), dtype=torch.int32, device=device)
    count = torch.empty(max(S, 0), max(B, 0), dtype=torch.int32, device=device)
    miss = torch.empty(max(B, 0), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _native.check(_native.lib().rnampnn_design_gc(
            _ptr(lg), int(lg.numel()) // 4, _ptr(m), _ptr(cu), B, T, float(temperature), S, _seed64(seed), None, _ptr(al), _ptr(pa),
            int(bool(c.wobble)) if c is not None else 1, _ptr(bi), per_position, _ptr(lo), _ptr(hi), _ptr(seqs), _ptr(nll), _ptr(bad),
            _ptr(count), _ptr(miss), _stream(device)))
    return seqs, nll, bad, count, miss


DISTINCT_MODES = {"sample": 1, "best": 0}


def design_distinct_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                                max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                                mode: str = "sample") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rnampnn_design_distinct`` (include/rnampnn_hip.h): ``n_samples`` (at most 256) pairwise DIFFERENT sequences per RNA under the
    constraints of ``design_from_logits``, in one launch -> (seqs, seq_nll, infeasible, logp (S,B) f32 = the log-probability of each
    sequence under the constrained, tempered distribution, n_distinct (B,) int32 = slots filled = min(S, admitted sequences)).
    ``mode="sample"``: an exact sample without replacement, in sampling order (slot 0 is one exact draw); ``mode="best"``: the most probable
    admitted sequences, in descending order.  A slot s >= n_distinct[b] holds -1 everywhere, seq_nll +inf and logp -inf.  The slots do
    not depend on the batch or the layout, and the first S' of S slots are the call with S'.  Layouts and ``constraints`` as in
    ``design_from_logits``.  CUDA logits only (there is no CPU fallback); no host synchronisation."""
    if mode not in DISTINCT_MODES:
        raise ValueError(f"mode must be one of {sorted(DISTINCT_MODES)}, got {mode!r}")
    device = logits.device
    if device.type != "cuda":
        raise RuntimeError("rnampnn_design_distinct runs on an MI355X: pass CUDA logits (there is no CPU fallback)")
    c = constraints
    al = None if c is None or c.allowed is None else _prep(c.allowed, device, torch.uint8)
    pa = None if c is None or c.partner is None else _prep(c.partner, device, torch.int32)
    bi = None if c is None or c.bias is None else _prep(c.bias, device)
    lg, m, cu, B, T = _layout(logits, mask, cu_seqlens, (al, pa), max_len)
    for name, t in (("allowed", al), ("partner", pa)):
        if t is not None and tuple(t.shape) != (B, T):
            raise ValueError(f"constraints.{name} must be padded to (B, T) = {(B, T)}, got {tuple(t.shape)}")
    per_position = int(bi is not None and tuple(bi.shape) == (B, T, 4))
    if bi is not None and not per_position and tuple(bi.shape) != (4,):
        raise ValueError(f"constraints.bias must be (4,) or (B, T, 4) = {(B, T, 4)}, got {tuple(bi.shape)}")
    _check_logits(lg, m, B, T)
    S = int(n_samples)
    seqs = torch.empty(max(S, 0), max(B, 0), max(T, 0), dtype=torch.int8, device=device)
    nll = torch.empty(max(S, 0), max(B, 0), dtype=torch.float32, device=device)
    bad = torch.empty(max(B, 0), dtype=torch.int32, device=device)
    logp = torch.empty(max(S, 0), max(B, 0), dtype=torch.float32, device=device)
    filled = torch.empty(max(B, 0), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _native.check(_native.lib().rnampnn_design_distinct(
            _ptr(lg), int(lg.numel()) // 4, _ptr(m), _ptr(cu), B, T, float(temperature), S, _seed64(seed), None, _ptr(al), _ptr(pa),
            int(bool(c.wobble)) if c is not None else 1, _ptr(bi), per_position, DISTINCT_MODES[mode], _ptr(seqs), _ptr(nll), _ptr(bad),
            _ptr(logp), _ptr(filled), _stream(device)))
    return seqs, nll, bad, logp, filled


def check_distinct(distinct, states=None, gc_content=None) -> None:
    """``design(..., distinct=...)``: ``ValueError`` for an unknown mode or a combination that is not built; touches no device."""
    if distinct is None:
        return
    if distinct not in DISTINCT_MODES:
        raise ValueError(f"distinct must be None or one of {sorted(DISTINCT_MODES)}, got {distinct!r}")
    for name, value in (("states", states), ("gc_content", gc_content)):
        if value is not None:
            raise ValueError(f"distinct together with {name} is not built: the beam runs over the units of rnampnn_design only")


SCORE_OUTPUTS = {"valid": torch.int32, "pred": torch.int8, "correct": torch.int32, "label_nll": torch.float32, "label_loss": torch.float32,
                 "seq_nll": torch.float32, "seq_match": torch.int32}


def score_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                 labels: Optional[torch.Tensor] = None, seqs: Optional[torch.Tensor] = None,
                 want=("valid", "correct", "label_nll", "label_loss"), max_len: Optional[int] = None, out: Optional[Dict] = None,
                 n_seqs: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """``rnampnn_score`` (include/rnampnn_hip.h): per-RNA scores of f32 logits in one launch -> dict of the outputs named in ``want``
    (``SCORE_OUTPUTS``).  Padded layout: logits (B,T,4) + ``mask`` (B,T); packed layout: logits (N,4) + ``cu_seqlens`` (B+1), with the
    padded extent T taken from ``labels`` / ``seqs`` / ``max_len``.  ``labels`` (B,T) class ids and ``seqs`` (S,B,T) are padded in both.
    ``out``: caller-owned tensors to write into (by name); ``n_seqs``: S when it is not ``seqs.shape[0]``.  No host synchronisation."""
    device = logits.device
    if device.type != "cuda":
        raise RuntimeError("rnampnn_score runs on an MI355X: pass CUDA logits (there is no CPU fallback)")
    unknown = set(want) - set(SCORE_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}; choose from {sorted(SCORE_OUTPUTS)}")
    lab = None if labels is None else _prep(labels, device, torch.int32)
    sq = None if seqs is None else _prep(seqs, device, torch.int8)
    lg, m, cu, B, T = _layout(logits, mask, cu_seqlens, (lab, sq), max_len)
    S = int(n_seqs) if n_seqs is not None else (0 if sq is None else int(sq.shape[0]))
    for name, t in (("labels", lab), ("seqs", sq)):
        if t is not None and (tuple(t.shape[-2:]) != (B, T) or (name == "seqs" and (t.dim() != 3 or t.shape[0] < S))):
            raise ValueError(f"{name} must be padded to (..., B, T) = {(B, T)}, got {tuple(t.shape)}")
    _check_logits(lg, m, B, T)
    shapes = {"valid": (B,), "pred": (B, T), "correct": (B,), "label_nll": (B,), "label_loss": (B,), "seq_nll": (max(S, 0), B),
              "seq_match": (max(S, 0), B)}
    res, ptrs = {}, {}
    for name in want:
        t = None if out is None else out.get(name)
        if t is None:
            # (an output asked for is a non-null pointer even where S = 0 leaves it empty: the library decides what that means)
            numel = int(torch.Size(shapes[name]).numel())
            buf = torch.empty(max(numel, 1), dtype=SCORE_OUTPUTS[name], device=device)
            t, ptrs[name] = buf[:numel].view(shapes[name]), C.c_void_p(buf.data_ptr())
        elif t.dtype != SCORE_OUTPUTS[name] or tuple(t.shape) != shapes[name] or not t.is_contiguous() or t.device != device:
            raise ValueError(f"out[{name!r}] must be a contiguous {SCORE_OUTPUTS[name]} tensor of shape {shapes[name]} on {device}")
        else:
            ptrs[name] = _ptr(t)
        res[name] = t
    with torch.cuda.device(device):
        _native.check(_native.lib().rnampnn_score(_ptr(lg), int(lg.numel()) // 4, _ptr(m), _ptr(cu), _ptr(lab), _ptr(sq), S, B, T,
                                                  *[ptrs.get(name) for name in SCORE_OUTPUTS], _stream(device)))
    return res


_LETTERS = b"\0" + "".join(REVERSE_VOCAB[i] for i in range(len(REVERSE_VOCAB))).encode()


def letters_padded(pred: torch.Tensor) -> List[str]:
    """(B,T) class ids with -1 on padding (``rnampnn_score``'s ``pred``) -> one string per RNA: one lookup on the device, one copy."""
    lut = torch.frombuffer(bytearray(_LETTERS), dtype=torch.uint8).to(pred.device)
    rows = lut[pred.to(torch.int64) + 1].cpu().numpy()
    return [row.tobytes().split(b"\0", 1)[0].decode() for row in rows]


def letters_packed(ids: torch.Tensor, lengths) -> List[str]:
    """Packed class ids (N,) + host-side lengths -> one string per RNA: one lookup on the device, one copy."""
    lut = torch.frombuffer(bytearray(_LETTERS[1:]), dtype=torch.uint8).to(ids.device)
    flat = lut[ids.to(torch.int64)].cpu().numpy().tobytes().decode()
    res, start = [], 0
    for n in (int(v) for v in lengths):
        res.append(flat[start:start + n])
        start += n
    return res
