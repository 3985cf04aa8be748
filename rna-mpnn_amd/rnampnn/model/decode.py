"""Decoding from logits, as free functions over the C ABI's decode family: argmax + recovery (``rnampnn_argmax_recovery``), free draws
(``rnampnn_sample``), scores (``rnampnn_score``), constrained and multi-state design (``rnampnn_design``, ``rnampnn_design_tied``), design
under a G+C content window (``rnampnn_design_gc``), design within a count window / a mutation budget (``rnampnn_design_count``), distinct
designs (``rnampnn_design_distinct``), design that avoids forbidden motifs (``rnampnn_design_avoid``), design with required motifs (``rnampnn_design_dfa``), motifs under a nested structure (``rnampnn_design_nested``), motifs under a count window (``combine="chain"``: ``rnampnn_design_dfa_count``), the distribution those draws come from (``rnampnn_design_count_profile``, ``rnampnn_design_avoid_profile``), the count tree in global memory for long RNAs (``tree=``: ``rnampnn_design_count_long``, ``rnampnn_design_count_profile_long``), the choice between them (``design_mode``, ``design_by_mode``) and the letters of class ids.  Needs the library and ``_base`` only, so both model packages import
it at module level."""
from __future__ import annotations

import ctypes as C
import itertools
from typing import Dict, List, NamedTuple, Optional, Tuple

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


def _design_inputs(name, logits, mask, cu_seqlens, max_len, constraints, padded=()):
    """What every entry of the design family does to its inputs, once: the device check (it speaks of ``name``), the constraints'
    tensors, the layout and the shape checks -> (lg, m, cu, B, T, own, al, pa, bi, per_position, wobble); ``own``: the prepared
    ``padded`` inputs - further (label, tensor, dtype) inputs padded to (B,T), shape-checked ahead of the constraints'."""
    device = logits.device
    if device.type != "cuda":
        raise RuntimeError(f"{name} runs on an MI355X: pass CUDA logits (there is no CPU fallback)")
    c = constraints
    own = [(label, _prep(t, device, dtype)) for label, t, dtype in padded]
    al = None if c is None or c.allowed is None else _prep(c.allowed, device, torch.uint8)
    pa = None if c is None or c.partner is None else _prep(c.partner, device, torch.int32)
    bi = None if c is None or c.bias is None else _prep(c.bias, device)
    lg, m, cu, B, T = _layout(logits, mask, cu_seqlens, tuple(t for _, t in own) + (al, pa), max_len)
    for label, t in own + [("constraints.allowed", al), ("constraints.partner", pa)]:
        if t is not None and tuple(t.shape) != (B, T):
            raise ValueError(f"{label} must be padded to (B, T) = {(B, T)}, got {tuple(t.shape)}")
    per_position = int(bi is not None and tuple(bi.shape) == (B, T, 4))
    if bi is not None and not per_position and tuple(bi.shape) != (4,):
        raise ValueError(f"constraints.bias must be (4,) or (B, T, 4) = {(B, T, 4)}, got {tuple(bi.shape)}")
    _check_logits(lg, m, B, T)
    return lg, m, cu, B, T, [t for _, t in own], al, pa, bi, per_position, int(bool(c.wobble)) if c is not None else 1


def _entry_call(name, args, device) -> None:
    """Entry ``name`` of the C ABI on ``args`` - tensors go as their device pointers, scalars as they are - and the stream of ``device``;
    raises what ``_native.check`` makes of the return code."""
    with torch.cuda.device(device):
        _native.check(getattr(_native.lib(), name)(*[_ptr(v) if torch.is_tensor(v) else v for v in args], _stream(device)))


def _design_call(name, logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints, padded=(), head=None, tail=None,
                 outputs=(), entry=None):
    """One call of a design entry of the C ABI -> (seqs, seq_nll, infeasible, *the entry's further outputs).  What the entries share
    is done here, once: the inputs (``_design_inputs``), the outputs and the common positional arguments.  What is an entry's own comes
    in: ``padded`` - further inputs padded to (B,T), as ``_design_inputs`` takes them; ``head`` / ``tail`` - callables (B, T, mask, cu, *the padded inputs) ->
    the entry's own arguments, tensors or scalars, placed where the ABI has them: after the rows / after the bias; ``outputs`` -
    (dtype, per sample ?) of the outputs past ``infeasible``: (S,B) or (B,); ``entry`` - the symbol when it is not ``name``."""
    device = logits.device
    lg, m, cu, B, T, own, al, pa, bi, per_position, wobble = _design_inputs(name, logits, mask, cu_seqlens, max_len, constraints, padded)
    its = [() if f is None else tuple(f(B, T, m, cu, *own)) for f in (head, tail)]
    S = int(n_samples)
    seqs = torch.empty(max(S, 0), max(B, 0), max(T, 0), dtype=torch.int8, device=device)
    nll = torch.empty(max(S, 0), max(B, 0), dtype=torch.float32, device=device)
    bad = torch.empty(max(B, 0), dtype=torch.int32, device=device)
    more = [torch.empty(*((max(S, 0),) if per_sample else ()), max(B, 0), dtype=dtype, device=device) for dtype, per_sample in outputs]
    args = [lg, int(lg.numel()) // 4, m, cu, B, T, *its[0], float(temperature), S, _seed64(seed), None, al, pa, wobble, bi, per_position,
            *its[1], seqs, nll, bad, *more]
    _entry_call(entry or name, args, device)
    return (seqs, nll, bad, *more)


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
    def tied(B, T, m, cu):
        if states is None:
            if state_weights is not None:
                raise ValueError("state_weights belong to multi-state design: pass states as well")
            return ()
        counts = _state_counts(states, B)
        gcu = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32).to(logits.device, non_blocking=True)
        sw = None if state_weights is None else _prep(torch.as_tensor(state_weights, dtype=torch.float32), logits.device)
        if sw is not None and tuple(sw.shape) != (B,):
            raise ValueError(f"state_weights must be (B,) = {(B,)}, got {tuple(sw.shape)}")
        return gcu, len(counts), sw
    return _design_call("rnampnn_design", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints, head=tied,
                        entry="rnampnn_design" if states is None else "rnampnn_design_tied")


TREES = ("lds", "global", "auto")
TREE_MODES = ("gc_content", "mutations")
NO_TREE = {"nested": "pairs"}


def check_tree(tree: str, mode: Optional[str] = None) -> str:
    """``tree`` - where the count tree of a G+C window or a mutation budget lives: "lds" (the default: one launch, the tree in the LDS of
    the workgroup, ``NotImplementedError`` past what 160 KiB hold), "global" (``rnampnn_design_count_long`` /
    ``rnampnn_design_count_profile_long``: a workspace in global memory, built once per RNA) or "auto" ("lds" where the library accepts it,
    "global" otherwise; the two return the same bytes) -> ``tree``.  ``ValueError`` for another value and, with a ``design_mode`` given, for
    "global" / "auto" together with a mode that has no count tree; touches no device, so a caller refuses before its forward pass."""
    if tree not in TREES:
        raise ValueError(f"tree must be one of {list(TREES)}, got {tree!r}")
    if tree != "lds" and mode is not None and mode not in TREE_MODES:
        what = "a draw without a count window" if mode == "plain" else NO_TREE.get(mode, mode)
        raise ValueError(f"tree={tree!r} together with {what} is not built: only the count tree of gc_content and of mutations has a home in "
                         "global memory")
    return tree


def check_profile_tree(tree: str, mode: str) -> str:
    """``check_tree`` for ``design_profile_from_logits``, whose "plain" mode is a count profile as well: ``ValueError`` for anything but
    "lds" together with ``avoid``."""
    if check_tree(tree) != "lds" and mode == "avoid":
        raise ValueError(f"tree={tree!r} together with avoid is not built: only the count trees of the plain, gc_content and mutations "
                         "profiles have a home in global memory")
    return tree


def _by_tree(tree: str, call):
    """``call(long)`` -> its result, with ``long`` as ``tree`` decides: "lds" False, "global" True, "auto" False first and True when the
    library refuses the LDS entry (``NotImplementedError``: its size check, which fires before anything is launched)."""
    if check_tree(tree) != "auto":
        return call(tree == "global")
    try:
        return call(False)
    except NotImplementedError:
        return call(True)


def _workspace(symbol: str, device, *sizes):
    """The workspace of an entry: (a ``torch.empty`` of ``symbol``(*sizes) bytes, that size as the ABI takes it)."""
    need = int(getattr(_native.lib(), symbol)(*sizes))
    return torch.empty(max(need, 8), dtype=torch.uint8, device=device), C.c_size_t(need)


def _tree_workspace(symbol: str, B: int, T: int, cap: int, device):
    """The workspace of a long entry: ``symbol``(B, T, max(cap, 1)) bytes."""
    return _workspace(symbol, device, max(B, 0), max(T, 0), max(int(cap), 1))


def _automaton_tail(symbol: str, auto, device, B: int, T: int, *sizes, own=()):
    """The own arguments of an entry on a ``DesignAutomaton`` (dfa, nested, chain), between the bias and the outputs: the automaton,
    ``own`` (the chain's count side) and the workspace of ``symbol``(B, T, live states, *sizes) bytes."""
    return (auto.delta_on(device), auto.kind, auto.n_states, *own, *_workspace(symbol, device, max(B, 0), max(T, 0), auto.n_live, *sizes))


def _lengths(m, cu, T: int) -> torch.Tensor:
    """(B,) lengths on the device, from the mask's row sums or from ``cu_seqlens``; no host synchronisation."""
    return (m.sum(dim=1) + 0.5).floor() if m is not None else (cu[1:] - cu[:-1]).clamp(0, max(T, 0))


def _count_side(mode: str, B: int, T: int, device, m=None, cu=None, gc_content=None, reference=None, budget=None, lengths=None):
    """What a count entry counts under ``mode`` -> (counted (B,T) uint8, lo (B,), hi (B,) int32, cap), on ``device``: "gc_content" - C|G
    count everywhere, the window of ``gc_counts`` over the lengths (``lengths``, or from the mask / ``cu_seqlens``), cap T; "mutations" -
    ``mutation_sets(reference)``, the budget (lo, hi) as window and hi as cap.  No host synchronisation."""
    B, T = max(B, 0), max(T, 0)
    if mode == "gc_content":
        fr = gc_fractions(gc_content, B).to(device, non_blocking=True)
        lo, hi = gc_counts(fr, _lengths(m, cu, T) if lengths is None else lengths)
        return torch.full((B, T), 12, dtype=torch.uint8, device=device), lo, hi, T
    w, cap = count_window(budget, budget[1], B)
    w = w.to(device, non_blocking=True)
    return mutation_sets(reference), w[:, 0].contiguous(), w[:, 1].contiguous(), cap


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
                          gc_content=(0.0, 1.0), tree: str = "lds") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rnampnn_design_gc`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` conditioned exactly on the G+C content of every
    RNA lying in a window, in one launch -> (seqs, seq_nll, infeasible, gc_count (S,B) int32 = C or G ids written, gc_miss (B,) int32 = 0
    when the window is reachable under the constraints, else its distance to the nearest reachable count, which the draws then hold).
    Layouts and ``constraints`` as in ``design_from_logits``.  ``gc_content``: a pair of fractions (lo, hi) in [0, 1] for every RNA, or a
    (B,2) tensor of them (float64: a float32 fraction carries its rounding into f * n); the counts are formed on the device from the mask
    or ``cu_seqlens`` (``gc_counts``), without a host synchronisation.  Fractions outside [0, 1] or lo > hi raise ``ValueError`` (a device
    tensor is not read back for that: the kernel clamps it).  ``tree`` (``check_tree``): "lds" - this entry, T <= 1017; "global" -
    ``rnampnn_design_count_long`` with C|G counted everywhere and a cap of T, formed on the device, which returns the same bytes at every
    length; "auto" - "lds" where it fits.  CUDA logits only (there is no CPU fallback)."""
    def window(long):
        def tail(B, T, m, cu):
            side = _count_side("gc_content", B, T, logits.device, m, cu, gc_content=gc_content)
            return (*side, *_tree_workspace("rnampnn_design_count_long_workspace_bytes", B, T, T, logits.device)) if long else side[1:3]
        return tail
    return _by_tree(tree, lambda long: _design_call(
        "rnampnn_design_gc", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints, tail=window(long),
        outputs=((torch.int32, True), (torch.int32, False)), entry="rnampnn_design_count_long" if long else None))


def mutation_sets(reference: torch.Tensor) -> torch.Tensor:
    """(B,T) class ids of a reference sequence -> the ``counted`` tensor of ``design_count_from_logits`` that counts MUTATIONS against it:
    15 ^ (1 << id) (every class but the reference's), 0 where the id is outside 0..3 (padding, unknown letters: such a position never
    counts).  uint8 on the reference's own device; no host synchronisation."""
    ref = reference.to(torch.int64)
    known = (ref >= 0) & (ref <= 3)
    return torch.where(known, 15 ^ (1 << ref.clamp(0, 3)), torch.zeros_like(ref)).to(torch.uint8)


def count_window(window, cap: Optional[int], B: int) -> Tuple[torch.Tensor, int]:
    """``window`` - a pair of ints (lo, hi) for every RNA, or a (B,2) int tensor - and ``cap`` -> ((B,2) int32 on the window's own device,
    the cap).  ``cap`` defaults to the largest hi of a HOST window; ``ValueError`` for another shape, a negative cap, a device window
    without ``cap`` (it is not read back here) and a host hi above ``cap`` (the kernel would clamp it silently)."""
    w = window if torch.is_tensor(window) else torch.as_tensor([int(v) for v in window], dtype=torch.int32)
    if w.dtype.is_floating_point or w.dtype == torch.bool:
        raise ValueError(f"window holds absolute counts: pass ints, got {w.dtype}")
    if tuple(w.shape) == (2,):
        w = w.expand(B, 2)
    if tuple(w.shape) != (B, 2):
        raise ValueError(f"window must be a pair (lo, hi) of counts or a (B, 2) = {(B, 2)} int tensor, got {tuple(w.shape)}")
    if cap is not None and int(cap) < 0:
        raise ValueError(f"cap = {cap} is negative")
    if w.device.type != "cpu":
        if cap is None:
            raise ValueError("a window on the device needs cap: it sizes the count tree and is not read back from the device")
        return w.to(torch.int32), int(cap)
    top = int(w[:, 1].max()) if B > 0 else 0
    if cap is None:
        return w.to(torch.int32), max(top, 0)
    if top > int(cap):
        raise ValueError(f"window: hi = {top} lies above cap = {int(cap)}")
    return w.to(torch.int32), int(cap)


def design_count_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                             max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                             counted: Optional[torch.Tensor] = None, window=(0, 0),
                             cap: Optional[int] = None,
                             tree: str = "lds") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rnampnn_design_count`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` conditioned exactly on a count lying in a
    window, in one launch -> (seqs, seq_nll, infeasible, count (S,B) int32, count_miss (B,) int32 = 0 when the window is reachable under
    the constraints, else its distance to the count the draws then hold).  ``counted`` (B,T) uint8, padded in both layouts: bits 0..3 mark
    the classes (AUCG) that count 1 at that position (``mutation_sets(reference)``: the count is the number of mutations).  ``window``: a
    pair of ints (lo, hi) for every RNA or a (B,2) int tensor, absolute counts.  ``cap``: no count above it is ever drawn; it sizes the
    tree in LDS (T <= 2867 at cap 8, 1017 without a cap).  It defaults to the largest hi of a host-side window; a device window without
    ``cap`` or a host hi above ``cap`` is a ``ValueError``.  ``tree`` (``check_tree``): "lds" - this entry and its limits; "global" -
    ``rnampnn_design_count_long``, the tree in a workspace in global memory (``torch.empty`` here, 8 B doubles(T, cap) bytes, built once per
    RNA for all samples), T <= 32744 at every cap, the same bytes wherever both run; "auto" - "lds" where it fits.  Layouts and
    ``constraints`` as in ``design_from_logits``.  CUDA logits only (there is no CPU fallback); no host synchronisation."""
    if counted is None:
        raise ValueError("counted is required: the (B, T) sets of classes that count (mutation_sets(reference) for a mutation budget)")

    def sets_and_window(B, T, m, cu, cs):
        w, top = count_window(window, cap, max(B, 0))
        w = w.to(logits.device, non_blocking=True)
        return cs, w[:, 0].contiguous(), w[:, 1].contiguous(), top

    def long_sets_and_window(B, T, m, cu, cs):
        its = sets_and_window(B, T, m, cu, cs)
        return (*its, *_tree_workspace("rnampnn_design_count_long_workspace_bytes", B, T, its[3], logits.device))
    return _by_tree(tree, lambda long: _design_call(
        "rnampnn_design_count", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints,
        padded=(("counted", counted, torch.uint8),), tail=long_sets_and_window if long else sets_and_window,
        outputs=((torch.int32, True), (torch.int32, False)), entry="rnampnn_design_count_long" if long else None))


def check_budget(lo: int, hi: int, states=None, gc_content=None, distinct=None) -> Tuple[int, int]:
    """A mutation budget of between ``lo`` and ``hi`` positions -> (lo, hi).  ``ValueError`` for a negative or inverted budget and for
    a combination that is not built; touches no device."""
    design_mode(states, gc_content, distinct, mutations=(lo, hi))
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi < lo:
        raise ValueError(f"mutations: the budget needs 0 <= min <= max, got min = {lo}, max = {hi}")
    return lo, hi


def check_mutations(mutations, states=None, gc_content=None, distinct=None):
    """``design(..., mutations=(reference, max))`` or ``(reference, min, max)`` -> (reference, (min, max)), or None for None.
    ``ValueError`` for another form and for what ``check_budget`` refuses; touches no device."""
    if mutations is None:
        return None
    if not isinstance(mutations, (tuple, list)) or len(mutations) not in (2, 3) or not torch.is_tensor(mutations[0]):
        check_budget(0, 0, states, gc_content, distinct)               # (a combination that is not built is the more useful message)
        raise ValueError("mutations must be (reference, max) or (reference, min, max) with reference a (B, T) tensor of class ids")
    lo, hi = (0, mutations[1]) if len(mutations) == 2 else (mutations[1], mutations[2])
    return mutations[0], check_budget(lo, hi, states, gc_content, distinct)


def design_mutations_from_logits(logits: torch.Tensor, mutations, **kw):
    """``design_count_from_logits`` as a mutation budget: ``mutations`` as ``check_mutations`` returns it -> (seqs, seq_nll, infeasible,
    n_mut (S,B) int32 = the Hamming distance of each draw to the reference, mut_miss (B,) int32).  ``kw``: the layout, the draw and
    ``tree``, as ``design_count_from_logits`` takes them."""
    reference, window = mutations
    return design_count_from_logits(logits, counted=mutation_sets(reference.to(logits.device)), window=window, cap=window[1], **kw)


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
    return _design_call("rnampnn_design_distinct", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints,
                        tail=lambda B, T, m, cu: (DISTINCT_MODES[mode],), outputs=((torch.float32, True), (torch.int32, False)))


def check_avoid(avoid, constraints=None, max_run=None):
    """``design(..., avoid=...)`` -> the ``MotifAutomaton`` (``as_automaton``), or None for None.  ``ValueError`` when the constraints carry
    base pairs: a pair couples two distant positions, which the exact chain over (position, automaton state) does not carry.  Touches no
    device, so a caller refuses before its forward pass."""
    from ..utils.motifs import as_automaton
    auto = as_automaton(avoid, max_run)
    if auto is not None and constraints is not None and constraints.partner is not None:
        raise ValueError("avoid together with base pairs is not built: a pair couples two distant positions, so an exact draw would carry the "
                         "class of every open pair in the automaton's state; drop `structure` from the constraints (fixed nucleotides, IUPAC "
                         "sets, omit and bias all combine with avoid)")
    return auto


def design_avoid_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                             max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                             avoid=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``rnampnn_design_avoid`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` conditioned exactly on the sequence containing
    none of a set of forbidden motifs, in one launch -> (seqs, seq_nll, infeasible, hits (S,B) int32 = positions of the draw at which a
    motif ends: 0 on every RNA that can avoid them, avoid_miss (B,) int32 = 1 when no admitted sequence of the RNA avoids the motifs: it is
    then drawn as ``design_from_logits`` draws it and ``hits`` reports what it holds).  ``avoid``: a ``MotifAutomaton``
    (``rnampnn.utils.motifs``), a motif string or an iterable of them.  Fixed / IUPAC sets and either bias of ``constraints`` combine with
    it; base pairs are a ``ValueError`` (``check_avoid``).  The table of partition sums lives in LDS: T <= 1064 for ``max_run=3`` (13 live
    states), 290 at 64 live states; beyond it the library raises ``NotImplementedError`` naming the limit.  Layouts as in
    ``design_from_logits``.  CUDA logits only (there is no CPU fallback); no host synchronisation."""
    auto = check_avoid(avoid, constraints)
    if auto is None:
        raise ValueError("avoid is required: a MotifAutomaton or motif strings (MotifAutomaton.from_motifs(['GGGG'], max_run=3))")
    return _design_call("rnampnn_design_avoid", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints,
                        tail=lambda B, T, m, cu: (auto.delta_on(logits.device), auto.n_states, C.c_uint64(auto.terminal)),
                        outputs=((torch.int32, True), (torch.int32, False)))


def check_require(require, avoid=None, constraints=None, max_run=None):
    """``design(..., require=..., avoid=...)`` -> the ``DesignAutomaton`` (``as_design_automaton``: every motif of ``require`` occurs, none
    of ``avoid`` does), or None when ``require`` is None.  ``ValueError`` when the constraints carry base pairs, for the reason
    ``check_avoid`` gives, and for what ``DesignAutomaton.from_motifs`` refuses.  Touches no device, so a caller refuses before its forward
    pass."""
    from ..utils.motifs import as_design_automaton
    auto = as_design_automaton(require, avoid, max_run)
    if auto is not None and constraints is not None and constraints.partner is not None:
        raise ValueError("require together with base pairs is not built: a pair couples two distant positions, so an exact draw would carry the "
                         "class of every open pair in the automaton's state; drop `structure` from the constraints (fixed nucleotides, IUPAC "
                         "sets, omit and bias all combine with require)")
    return auto


def design_dfa_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                           max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                           require=None, avoid=None, max_run=None):
    """``rnampnn_design_dfa`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` conditioned exactly on the sequence containing
    EVERY motif of ``require`` somewhere and none of ``avoid`` (nor, with ``max_run=r``, a run longer than r), in one launch -> (seqs,
    seq_nll, infeasible, hits (S,B) int32 = positions of the draw at which an avoided word ends, accepted (S,B) int32 = 1 when the draw
    holds every required motif, dfa_miss (B,) int32 = 1 when no admitted sequence of the RNA is accepted - too short, or its fixed positions
    rule a required motif out: it is then drawn as ``design_from_logits`` draws it and ``hits`` / ``accepted`` report what it holds).
    ``require``: a ``DesignAutomaton`` (``rnampnn.utils.motifs``; ``avoid`` and ``max_run`` are then not read) or motif strings.  Fixed /
    IUPAC sets and either bias of ``constraints`` combine with it; base pairs are a ``ValueError`` (``check_require``).  The table of
    partition sums lives in a workspace in global memory (``torch.empty`` here, 8 B T L bytes at L live states), so neither the automaton
    (up to 256 states) nor T x L is bound by LDS: T <= 1587 for every automaton; beyond it the library raises ``NotImplementedError``
    naming the limit.  Layouts as in ``design_from_logits``.  CUDA logits only (there is no CPU fallback); no host synchronisation."""
    auto = check_require(require, avoid, constraints, max_run)
    if auto is None:
        raise ValueError("require is required: a DesignAutomaton or motif strings (DesignAutomaton.from_motifs(['GGAGG'], max_run=3))")

    return _design_call("rnampnn_design_dfa", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints,
                        tail=lambda B, T, m, cu: _automaton_tail("rnampnn_design_dfa_workspace_bytes", auto, logits.device, B, T),
                        outputs=((torch.int32, True), (torch.int32, True), (torch.int32, False)))


def check_nested(require=None, avoid=None, constraints=None, max_run=None):
    """``design(..., pairs="nested", require=..., avoid=...)`` -> the ``DesignAutomaton`` of ``rnampnn_design_nested``
    (``as_nested_automaton``: ``require`` with ``avoid`` absorbed, or ``avoid`` / ``max_run`` alone with every live state accepting), or
    None when none of them is given.  Base pairs are what this mode is for; ``ValueError`` naming the rows when HOST-side constraints hold
    a structure whose pairs cross (a pseudoknot is not a tree; a device-side ``partner`` is not read back: the kernel's ``nest_miss``
    reports it), and for what the automaton's constructors refuse.  Touches no device, so a caller refuses before its forward pass."""
    from ..utils.constraints import crossing_pairs
    from ..utils.motifs import as_nested_automaton
    auto = as_nested_automaton(require, avoid, max_run)
    partner = None if auto is None or constraints is None else constraints.partner
    if partner is not None and partner.device.type == "cpu":
        knotted = [b for b, row in enumerate(partner) if crossing_pairs(row)]
        if knotted:
            raise ValueError(f"pairs='nested': the structure of row(s) {knotted} holds a pseudoknot (two of its pairs cross); the exact draw "
                             "under motifs walks a nested structure: drop the crossing pairs from `structure`")
    return auto


def design_nested_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                              max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                              require=None, avoid=None, max_run=None):
    """``rnampnn_design_nested`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` under the base pairs of a NESTED target
    structure, conditioned exactly on the sequence containing EVERY motif of ``require`` somewhere and none of ``avoid`` (nor, with
    ``max_run=r``, a run longer than r), in one launch -> (seqs, seq_nll, infeasible, hits (S,B) int32, accepted (S,B) int32, dfa_miss (B,)
    int32 = 1 when no admitted sequence of the RNA is accepted, nest_miss (B,) int32 = 1 when two of its pairs cross; either way the RNA
    is then drawn as ``design_from_logits`` draws it and ``hits`` / ``accepted`` report what it holds).  ``require``: a ``DesignAutomaton``
    (``avoid`` and ``max_run`` are then not read), motif strings, or None for ``avoid`` / ``max_run`` alone.  Every field of
    ``constraints`` combines with it, the structure included; without pairs the outputs are ``design_dfa_from_logits``' byte for byte.
    The tables live in a workspace in global memory (``torch.empty`` here, about 8 B T L^2 bytes at L live states); at most 64 live states
    and T <= 1616, beyond which the library raises ``NotImplementedError`` naming the limit.  Layouts as in ``design_from_logits``.  CUDA
    logits only (there is no CPU fallback); no host synchronisation."""
    auto = check_nested(require, avoid, constraints, max_run)
    if auto is None:
        raise ValueError("require or avoid is required: a DesignAutomaton or motif strings (require=['GNRA'], avoid=['GGGG'], max_run=3)")

    return _design_call("rnampnn_design_nested", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints,
                        tail=lambda B, T, m, cu: _automaton_tail("rnampnn_design_nested_workspace_bytes", auto, logits.device, B, T),
                        outputs=((torch.int32, True), (torch.int32, True), (torch.int32, False), (torch.int32, False)))


def check_distinct(distinct, states=None, gc_content=None) -> None:
    """``design(..., distinct=...)``: ``ValueError`` for an unknown mode or a combination that is not built; touches no device."""
    if distinct is not None:
        design_mode(states, gc_content, distinct)


# What conditions the draws, in the order in which it decides the mode: (the argument that selects the mode, the arguments it is not built
# together with, why).  A mode further down is excluded by the ones above it, so every pair is named once.
DESIGN_MODES = (("avoid", ("states", "gc_content", "distinct", "mutations"),
                 "the automaton conditions the draws of rnampnn_design on the motifs alone"),
                ("mutations", ("states", "gc_content", "distinct"), "the budget conditions the draws of rnampnn_design on one count"),
                ("distinct", ("states", "gc_content"), "the beam runs over the units of rnampnn_design only"),
                ("gc_content", ("states",), "the G+C window conditions the draws of rnampnn_design only"),
                ("states", (), ""))


def check_chain(constraints=None, require=None, avoid=None, max_run=None):
    """``design(..., combine="chain", require=..., avoid=..., max_run=...)`` -> the ``DesignAutomaton`` of ``rnampnn_design_dfa_count``
    (``as_nested_automaton``: ``require`` with ``avoid`` absorbed, or ``avoid`` / ``max_run`` alone with every live state accepting).
    ``ValueError`` when the constraints carry base pairs - the one ``check_require`` raises with a ``require``, else ``check_avoid``'s -
    and for what the automaton's constructors refuse.  Touches no device, so a caller refuses before its forward pass."""
    from ..utils.motifs import as_nested_automaton
    if require is not None:
        return check_require(require, avoid, constraints, max_run)
    if avoid is None and max_run is None:
        return None
    check_avoid(avoid if avoid is not None else (), constraints, max_run)
    return as_nested_automaton(None, avoid, max_run)


def design_dfa_count_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                                 max_len: Optional[int] = None, n_samples: int = 8, temperature: float = 0.1, seed: int = 0, constraints=None,
                                 require=None, avoid=None, max_run=None, gc_content=None, mutations=None):
    """``rnampnn_design_dfa_count`` (include/rnampnn_hip.h): the draws of ``design_from_logits`` conditioned exactly on BOTH the motifs
    (every motif of ``require`` occurs, none of ``avoid`` does, no run longer than ``max_run``) AND one count - the G+C window
    ``gc_content`` (as ``design_gc_from_logits`` takes it) or the budget ``mutations`` (as ``check_mutations`` returns it: (reference,
    (min, max))) - in one launch -> (seqs, seq_nll, infeasible, hits (S,B) int32, accepted (S,B) int32, count (S,B) int32 = the C or G
    ids / the mutations of each draw, dfa_miss (B,) int32 = 1 when no admitted sequence holds the motifs at any count the cap allows: the
    RNA is then drawn as ``design_from_logits`` draws it, count_miss (B,) int32 = 0 when the window is reachable together with the motifs,
    else its distance to the nearest reachable count, which the draws then hold, log_z (B,) f64 = the log partition sum of what the draws
    come from).  The automaton is ``check_chain``'s (up to 256 states); the count side is what ``design_gc_from_logits`` /
    ``design_mutations_from_logits`` pass: C|G counted everywhere with a cap of T, or ``mutation_sets(reference)`` with the budget as
    window and cap.  Base pairs are a ``ValueError``.  The table lives in a workspace in global memory (``torch.empty`` here,
    8 B T L (cap + 1) bytes at L live states: it grows with the cap, the price of a draw that is exact in both conditions); T <= 1616 for
    every automaton and cap, beyond which the library raises ``NotImplementedError`` naming the limit.  Layouts as in
    ``design_from_logits``.  CUDA logits only (there is no CPU fallback); no host synchronisation."""
    if (gc_content is None) == (mutations is None):
        raise ValueError("exactly one of gc_content and mutations conditions the count (two counts at once are not built)")
    auto = check_chain(constraints, require, avoid, max_run)
    if auto is None:
        raise ValueError("require, avoid or max_run is required: a DesignAutomaton or motif strings (require=['GNRA'], avoid=['GGGG'], max_run=3)")
    device = logits.device
    padded = () if mutations is None else (("the reference of mutations", mutations[0], torch.int32),)

    def chain(B, T, m, cu, *ref):
        if mutations is None:
            side = _count_side("gc_content", B, T, device, m, cu, gc_content=gc_content)
        else:
            side = _count_side("mutations", B, T, device, reference=ref[0], budget=mutations[1])
        return _automaton_tail("rnampnn_design_dfa_count_workspace_bytes", auto, device, B, T, max(int(side[3]), 1), own=(*side[:3], int(side[3])))
    return _design_call("rnampnn_design_dfa_count", logits, mask, cu_seqlens, max_len, n_samples, temperature, seed, constraints,
                        padded=padded, tail=chain,
                        outputs=((torch.int32, True), (torch.int32, True), (torch.int32, True), (torch.int32, False), (torch.int32, False),
                                 (torch.float64, False)))


COMBINE = ("chain",)


def _chain_mode(given: dict, require, pairs, tree: str) -> str:
    """``design_mode`` with ``combine="chain"``: "chain", or the ``ValueError`` of a combination that is not built."""
    if given["avoid"] is None and require is None and given["max_run"] is None:
        raise ValueError("combine='chain' needs avoid, require or max_run: a plain G+C window or mutation budget needs no chain (drop combine=)")
    if (given["gc_content"] is None) == (given["mutations"] is None):
        raise ValueError("combine='chain' conditions on ONE count: pass exactly one of gc_content and mutations (two counts at once are "
                         "not built)")
    for name in ("states", "distinct"):
        if given[name] is not None:
            raise ValueError(f"combine='chain' together with {name} is not built: the chain over (position, automaton state, count) "
                             "conditions the draws of rnampnn_design on the motifs and one count alone")
    if pairs is not None:
        raise ValueError("combine='chain' together with pairs is not built: base pairs under motifs and a count at once would carry the "
                         "count through every transfer table of rnampnn_design_nested")
    if tree != "lds":
        raise ValueError(f"combine='chain' together with tree={tree!r} is not built: the chain's table lives in its own workspace and has "
                         "no count tree")
    return "chain"


def design_mode(states=None, gc_content=None, distinct=None, mutations=None, avoid=None, require=None, pairs=None, combine=None,
                max_run=None, tree: str = "lds") -> str:
    """Which entry ``design(...)`` draws from: "require", "avoid", "mutations", "distinct", "gc_content", "states", or "plain" when none of
    them is given.  ``require`` decides first and absorbs ``avoid`` (one automaton holds both lists).  ``ValueError`` for a combination
    that is not built (``DESIGN_MODES``; ``require`` with anything but ``avoid``) and an unknown ``distinct``; touches no device, so a
    caller refuses before its forward pass.  ``pairs="nested"`` opts in to "nested" (``rnampnn_design_nested``: ``avoid`` and / or
    ``require`` under the base pairs of a nested structure); it is a ``ValueError`` with another value, with a mode the automaton is not
    built together with, and with neither ``avoid`` nor ``require``.  With ``pairs=None`` nothing differs.  ``combine="chain"`` opts in
    to "chain" (``rnampnn_design_dfa_count``: ``avoid`` / ``require`` / ``max_run`` TOGETHER with ``gc_content`` or ``mutations``, exact in
    both); it is a ``ValueError`` with another value, without a motif argument, with both counts or neither, with ``states``,
    ``distinct`` or ``pairs``, and with a ``tree`` other than "lds".  With ``combine=None`` nothing differs (``max_run`` and ``tree`` are
    read by the chain alone)."""
    given = {"states": states, "gc_content": gc_content, "distinct": distinct, "mutations": mutations, "avoid": avoid}
    if combine is not None:
        if combine not in COMBINE:
            raise ValueError(f"combine must be None or 'chain', got {combine!r}")
        return _chain_mode(dict(given, max_run=max_run), require, pairs, tree)
    if pairs is not None:
        if pairs != "nested":
            raise ValueError(f"pairs must be None or 'nested', got {pairs!r}")
        for name in DESIGN_MODES[0][1]:
            if given[name] is not None:
                raise ValueError(f"pairs='nested' together with {name} is not built: the automaton conditions the draws of rnampnn_design on "
                                 "the motifs and the base pairs alone")
        if avoid is None and require is None:
            raise ValueError("pairs='nested' needs avoid and / or require: plain constraints already honour base pairs (drop pairs=)")
        return "nested"
    if require is not None:
        for name in DESIGN_MODES[0][1]:
            if given[name] is not None:
                raise ValueError(f"require together with {name} is not built: the automaton conditions the draws of rnampnn_design on the "
                                 "motifs alone")
        return "require"
    for mode, excluded, why in DESIGN_MODES:
        if given[mode] is None:
            continue
        if mode == "distinct" and distinct not in DISTINCT_MODES:
            raise ValueError(f"distinct must be None or one of {sorted(DISTINCT_MODES)}, got {distinct!r}")
        for name in excluded:
            if given[name] is not None:
                raise ValueError(f"{mode} together with {name} is not built: {why}")
        return mode
    return "plain"


def resolve_design(constraints=None, states=None, lengths=None, gc_content=None, distinct=None, mutations=None, avoid=None, require=None,
                   pairs=None, combine=None, tree: str = "lds", run=None):
    """What every ``design(...)`` - both models' and both command-line ``predict`` - does with its arguments before its forward pass ->
    (mode, mutations, avoid, require) as ``design_by_mode`` takes them.  Touches no device; what is not built is a ``ValueError`` here, in
    one order: ``design_mode``, ``check_tree``, ``check_mutations``, the automaton of the mode (``check_chain`` / ``check_nested`` /
    ``check_require``, else ``check_avoid``), ``check_state_lengths``.  ``run(tree, mode)``: the command line's hook - it makes its own
    checks of the tree and returns its forms of the four automaton checks, (chain, nested, require)(require, avoid) and avoid(avoid),
    which know ``samples`` and a constraints TABLE (``rnampnn.utils.predict.resolve_run``); ``mutations`` then passes through unread.

    The arguments, for every caller (the return tuple of each mode stands with ``RNAMPNN.design`` / ``RNAModel.design``):
    ``constraints`` (``rnampnn.utils.constraints.DesignConstraints``: fixed nucleotides, base pairs of a target structure, bias): the
    draws come from ``rnampnn_design``, which honours them and scores in the same launch; ``infeasible`` counts the positions whose
    constraint could not be honoured.  ``states`` / ``state_weights``: multi-state design (``design_from_logits``) - the consecutive rows
    of a group are states of ONE design and receive the same sequence.  ``lengths``: the loader's host-side lengths; with them a group
    whose states differ in length is refused naming the group (nothing reads the mask on the host; without them such a group is designed
    over its common prefix).  ``gc_content`` (a pair of fractions, or (B,2)): the draws, under ``constraints`` or free, are conditioned
    exactly on the G+C content of every RNA lying in that window (``design_gc_from_logits``); not built together with ``states``.
    ``distinct`` ("sample" or "best"): ``n_samples`` pairwise DIFFERENT sequences per RNA (``design_distinct_from_logits``), an exact
    sample without replacement or the most probable admitted sequences in descending order; not built together with ``states`` or
    ``gc_content``.  ``mutations`` (``(reference, max)`` or ``(reference, min, max)``, reference (B,T) class ids, e.g. the native
    sequence): the draws differ from the reference at between min (default 0) and max positions, drawn exactly from the model's
    distribution conditioned on that (``design_count_from_logits``); ``mut_miss`` = how far the structure and the fixed positions alone
    push the count out of the budget, 0 when it is reachable; not built together with ``states``, ``gc_content`` or ``distinct``.
    ``avoid`` (a ``rnampnn.utils.motifs.MotifAutomaton`` or motif strings such as ``["GGGG", "GAAUUC"]``): no draw contains one of the
    motifs, drawn exactly from the model's distribution conditioned on that, under the fixed positions and the bias of ``constraints`` or
    free (``design_avoid_from_logits``); ``avoid_miss`` = 1 for an RNA whose fixed positions spell a motif; not built together with the
    modes above or with constraints that carry base pairs.  ``require`` (a ``rnampnn.utils.motifs.DesignAutomaton`` or motif strings such
    as ``["GGAGG", "GNRA"]``): every draw contains EVERY one of the motifs somewhere and none of ``avoid``, which it absorbs
    (``design_dfa_from_logits``); ``dfa_miss`` = 1 for an RNA that cannot hold the motifs; not built together with the modes above or with
    base pairs.  ``pairs="nested"`` (``None``: everything above, unchanged): ``avoid`` and / or ``require`` UNDER the base pairs of
    ``constraints`` (``design_nested_from_logits``) - the structure is honoured and the draws are exact as long as it is nested;
    ``nest_miss`` = 1 for an RNA whose pairs cross: it is drawn as plain ``constraints`` draw it; host-side constraints whose structure
    crosses, another mode, another value, or neither ``avoid`` nor ``require`` are refused.  ``tree`` ("lds", the default: everything
    above, unchanged; "global"; "auto"): where the count tree of ``gc_content`` and ``mutations`` lives (``check_tree``) - in global
    memory RNAs of up to 32,744 nt are drawn under a G+C window, with the same bytes wherever both homes run; anything but "lds" with
    another mode is refused.  ``combine="chain"`` (``None``: everything above, unchanged): ``avoid`` and / or ``require`` TOGETHER with
    ``gc_content`` or ``mutations`` (``design_dfa_count_from_logits``), exact in both conditions at once; ``count`` = the C or G ids / the
    mutations of each draw; another value, no motif argument, both counts or neither, ``states``, ``distinct``, ``pairs``, a ``tree``
    other than "lds" and constraints that carry base pairs are refused."""
    mode = design_mode(states, gc_content, distinct, mutations, avoid, require=require, pairs=pairs, combine=combine, tree=tree)
    if run is None:
        check_tree(tree, mode)
        mutations = check_mutations(mutations)
    chain, nested, required, avoided = run(tree, mode) if run is not None else (
        lambda r, a: check_chain(constraints, r, a), lambda r, a: check_nested(r, a, constraints), lambda r, a: check_require(r, a, constraints),
        lambda a: check_avoid(a, constraints))
    if mode == "chain":
        require, avoid = chain(require, avoid), None
    elif mode == "nested":
        require, avoid = nested(require, avoid), None
    else:
        require = required(require, avoid)
        avoid = avoided(avoid) if require is None else None
    if run is None and states is not None and lengths is not None:
        check_state_lengths(states, lengths)
    return mode, mutations, avoid, require


TABLES = ("lds", "global")


def check_table(table: str, constraints=None, gc_content=None, mutations=None, avoid=None, require=None, max_run=None, tree: str = "lds"):
    """``table`` - where the backward table of a profile under motifs lives: "lds" (the default: ``rnampnn_design_avoid_profile``,
    forbidden motifs alone, at most 64 states, the table in the LDS of the workgroup) or "global" (``rnampnn_design_dfa_profile``:
    ``require`` and / or ``avoid`` on the automaton of up to 256 states, the table in a workspace in global memory) -> the
    ``DesignAutomaton`` of "global" (``check_require``, or ``DesignAutomaton.from_avoid`` for ``avoid`` alone), None for "lds".  There is
    no "auto": the two homes of the forbidden-motif profile add in different orders and agree to rounding, not to the byte, and that byte
    equality is what made ``tree="auto"`` invisible.  ``ValueError`` for another value, for ``require`` without "global", and for "global"
    without ``avoid`` / ``require``, with ``gc_content``, ``mutations``, a ``tree`` other than "lds" or base pairs in the constraints;
    touches no device, so a caller refuses before its forward pass."""
    if table not in TABLES:
        raise ValueError(f"table must be one of {list(TABLES)}, got {table!r}")
    if table == "lds":
        if require is not None:
            raise ValueError("a design profile together with require needs table=\"global\": the profile whose table lives in LDS knows "
                             "forbidden motifs only (rnampnn_design_dfa_profile keeps the table of the 256-state automaton in global memory)")
        return None
    if avoid is None and require is None:
        raise ValueError("table=\"global\" needs avoid and / or require: it is the home of the table of a profile under motifs (the count "
                         "profiles have tree=)")
    for name, value in (("gc_content", gc_content), ("mutations", mutations)):
        if value is not None:
            raise ValueError(f"table=\"global\" together with {name} is not built: the automaton conditions the profile on the motifs alone")
    if tree != "lds":
        raise ValueError(f"table=\"global\" together with tree={tree!r} is not built: a profile under motifs has no count tree")
    if require is not None:
        return check_require(require, avoid, constraints, max_run)
    from ..utils.motifs import DesignAutomaton
    return DesignAutomaton.from_avoid(check_avoid(avoid, constraints, max_run))


def resolve_profile(constraints=None, gc_content=None, mutations=None, avoid=None, tree: str = "lds", require=None, table: str = "lds",
                    max_run=None) -> tuple:
    """What both models' ``design_profile`` check before their forward pass, and ``design_profile_from_logits`` when it is called without
    the result -> (mode, mutations as ``check_mutations`` returns it, the ``MotifAutomaton`` of "avoid" or the ``DesignAutomaton`` of
    ``table="global"``, or None), as ``design_profile_from_logits`` takes it; the automaton is built once: the home of the table of a profile under motifs (``check_table``), the
    pairings ``design`` refuses, the home of the tree (``check_profile_tree``), the form of ``mutations`` and ``avoid`` together with
    base pairs.  Touches no device."""
    dfa = check_table(table, constraints, gc_content, mutations, avoid, require, max_run, tree)
    if dfa is not None:
        return "require" if require is not None else "avoid", None, dfa
    mode = design_mode(gc_content=gc_content, mutations=mutations, avoid=avoid)
    check_profile_tree(tree, mode)
    return mode, check_mutations(mutations), check_avoid(avoid, constraints, max_run)


def design_by_mode(mode: str, logits: torch.Tensor, states=None, state_weights=None, gc_content=None, distinct=None, mutations=None,
                   avoid=None, require=None, tree: str = "lds", **kw):
    """The ``*_from_logits`` call of ``mode`` (``design_mode``) -> what that function returns.  ``mutations`` as ``check_mutations``
    returns it, ``avoid`` as ``check_avoid`` does, ``require`` as ``check_require`` does (it holds ``avoid``); ``kw``: the layout and the
    draw (mask / cu_seqlens / max_len, n_samples, temperature, seed, constraints).  "nested": ``require`` as ``check_nested`` returns it
    (it holds ``avoid``).  ``tree`` (``check_tree``): the home of the count tree of "gc_content" and "mutations"; anything but "lds" with
    another mode is a ``ValueError``.  "chain": ``require`` as ``check_chain`` returns it (it holds ``avoid``) with ``gc_content`` or
    ``mutations``."""
    check_tree(tree, mode)
    if mode == "chain":
        return design_dfa_count_from_logits(logits, require=require, gc_content=gc_content, mutations=mutations, **kw)
    if mode == "nested":
        return design_nested_from_logits(logits, require=require, **kw)
    if mode == "require":
        return design_dfa_from_logits(logits, require=require, **kw)
    if mode == "avoid":
        return design_avoid_from_logits(logits, avoid=avoid, **kw)
    if mode == "mutations":
        return design_mutations_from_logits(logits, mutations, tree=tree, **kw)
    if mode == "distinct":
        return design_distinct_from_logits(logits, mode=distinct, **kw)
    if mode == "gc_content":
        return design_gc_from_logits(logits, gc_content=gc_content, tree=tree, **kw)
    return design_from_logits(logits, states=states, state_weights=state_weights, **kw)


class DesignProfile(NamedTuple):
    """What ``design_profile_from_logits`` returns: marginals (B,T,4) f64 - P(x_t = c) under the distribution the draws of ``mode`` come
    from, 0 on padding; log_z, log_z_free, entropy (B,) f64; infeasible (B,) int32 and miss (B,) int32 - the draw entry's own ``infeasible``
    and ``gc_miss`` / ``mut_miss`` / ``avoid_miss``; mode - the ``design_mode``."""
    marginals: torch.Tensor
    log_z: torch.Tensor
    log_z_free: torch.Tensor
    entropy: torch.Tensor
    infeasible: torch.Tensor
    miss: torch.Tensor
    mode: str

    @property
    def log_mass(self) -> torch.Tensor:
        """(B,) f64, <= 0: the log of the share of the model's mass that the constraints keep."""
        return self.log_z - self.log_z_free


PROFILE_ENTRIES = {"plain": "rnampnn_design_count_profile", "gc_content": "rnampnn_design_count_profile",
                   "mutations": "rnampnn_design_count_profile", "avoid": "rnampnn_design_avoid_profile",
                   "require": "rnampnn_design_dfa_profile"}


def profile_entry(mode: str, auto=None) -> str:
    """The profile entry of ``mode`` (None for a mode without one): ``PROFILE_ENTRIES``; "avoid" on a ``DesignAutomaton`` is "require"'s."""
    from ..utils.motifs import DesignAutomaton
    return PROFILE_ENTRIES.get("require" if isinstance(auto, DesignAutomaton) else mode)


def profile_mode_args(mode: str, B: int, T: int, device, lengths=None, gc_content=None, reference=None, budget=None, auto=None) -> tuple:
    """The own arguments of the profile entry of ``mode`` (``profile_entry``), between the bias and the outputs, on ``device``
    (``lengths`` (B,), read by "gc_content" alone, lives there): "plain" - nothing counts, window (0, 0), cap 0: the tree degenerates and the distribution is ``rnampnn_design``'s;
    "gc_content" - C|G count everywhere, the window of ``gc_counts``, cap T; "mutations" - ``mutation_sets(reference)``, the budget
    (lo, hi) as window and hi as cap; "avoid" - the automaton's tables; "require", and "avoid" on a ``DesignAutomaton`` - the automaton and
    the workspace of its backward table (``_automaton_tail``).  No host synchronisation."""
    if profile_entry(mode, auto) == PROFILE_ENTRIES["require"]:
        return _automaton_tail("rnampnn_design_dfa_profile_workspace_bytes", auto, device, B, T)
    if mode == "avoid":
        return auto.delta_on(device), auto.n_states, C.c_uint64(auto.terminal)
    if mode in ("gc_content", "mutations"):
        return _count_side(mode, B, T, device, gc_content=gc_content, reference=reference, budget=budget, lengths=lengths)
    if mode != "plain":
        raise ValueError(f"no profile is built for the mode {mode!r}")
    zero = torch.zeros(B, dtype=torch.int32, device=device)
    return torch.zeros(B, T, dtype=torch.uint8, device=device), zero, zero, 0


def design_profile_from_logits(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, cu_seqlens: Optional[torch.Tensor] = None,
                               max_len: Optional[int] = None, temperature: float = 0.1, constraints=None, gc_content=None, mutations=None,
                               avoid=None, tree: str = "lds", require=None, max_run=None, table: str = "lds",
                               resolved: Optional[tuple] = None) -> DesignProfile:
    """``rnampnn_design_count_profile`` / ``rnampnn_design_avoid_profile`` (include/rnampnn_hip.h): the exact distribution that the draws
    of ``design_by_mode`` come from under the same arguments - per-position marginals, log partition sums and entropy, fp64, in one launch ->
    ``DesignProfile``.  The mode is ``design_mode(gc_content=, mutations=, avoid=)``, so the pairings that are not built keep their messages:
    "plain" (constraints alone: the count entry with nothing counted, the distribution of ``design_from_logits``), "gc_content" (a pair of
    fractions or (B,2), as in ``design_gc_from_logits``), "mutations" (``(reference, max)`` or ``(reference, min, max)``, as ``design``
    takes it) and "avoid" (a ``MotifAutomaton`` or motif strings; base pairs are the ``ValueError`` of ``check_avoid``).  The trees live in
    LDS: T <= 535 for a G+C window, 1457 for a budget of 8, 1168 for ``max_run=3``; beyond it the library raises ``NotImplementedError``
    naming the limit.  ``tree`` (``check_tree``), for the three count modes: "global" - ``rnampnn_design_count_profile_long``, the inside
    and the outside tree in a workspace in global memory (``torch.empty`` here), T <= 65536, the same bytes wherever both run; "auto" -
    "lds" where it fits; anything but "lds" with ``avoid`` is a ``ValueError``.  ``table`` (``check_table``): "lds" - everything above,
    unchanged; "global" - ``rnampnn_design_dfa_profile``: the profile of what ``design_dfa_from_logits`` draws under ``require`` (a
    ``DesignAutomaton`` or motif strings, with ``avoid`` and ``max_run`` absorbed), or of ``avoid`` / ``max_run`` alone
    (``DesignAutomaton.from_avoid``), on automata of up to 256 states with the backward table in a workspace in global memory
    (``torch.empty`` here, 8 B T L bytes at L live states), T <= 4498 at every automaton; ``mode`` is "require" or "avoid" and ``miss``
    is ``dfa_miss``.  ``require`` without it, and "global" without ``avoid`` / ``require`` or with ``gc_content``, ``mutations``, another
    ``tree`` or base pairs, are a ``ValueError`` before any device work.  There is no "auto" table: the two homes of the forbidden-motif
    profile add in different orders and agree to rounding, not to the byte - and that byte equality is what made ``tree="auto"``
    invisible.  ``resolved``: ``resolve_profile``'s result from a caller that has run it already; ``mutations``, ``avoid``, ``require``,
    ``max_run`` and ``table`` are then not read.  Layouts and ``constraints`` as in ``design_from_logits``.  CUDA logits only (there is no CPU fallback); no host synchronisation."""
    if resolved is None:
        resolved = resolve_profile(constraints, gc_content, mutations, avoid, tree, require, table, max_run)
    mode, mutations, auto = resolved
    name = profile_entry(mode, auto)
    padded = (("the reference of mutations", mutations[0], torch.int32),) if mode == "mutations" else ()
    lg, m, cu, B, T, own, al, pa, bi, per_position, wobble = _design_inputs(name, logits, mask, cu_seqlens, max_len, constraints, padded)
    device, Bn, Tn = lg.device, max(B, 0), max(T, 0)
    lengths = _lengths(m, cu, Tn) if mode == "gc_content" else None
    its = profile_mode_args(mode, Bn, Tn, device, lengths, gc_content=gc_content, reference=own[0] if own else None,
                            budget=None if mutations is None else mutations[1], auto=auto)
    marg = torch.empty(Bn, Tn, 4, dtype=torch.float64, device=device)
    log_z, free, ent = (torch.empty(Bn, dtype=torch.float64, device=device) for _ in range(3))
    bad, miss = (torch.empty(Bn, dtype=torch.int32, device=device) for _ in range(2))

    def call(long):
        ws = _tree_workspace("rnampnn_design_count_profile_long_workspace_bytes", B, T, its[3], device) if long else ()
        args = [lg, int(lg.numel()) // 4, m, cu, B, T, float(temperature), al, pa, wobble, bi, per_position, *its, *ws, marg, log_z, free, ent, bad,
                miss]
        _entry_call(name + ("_long" if long else ""), args, device)
    _by_tree(tree, call)
    return DesignProfile(marg, log_z, free, ent, bad, miss, mode)


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
