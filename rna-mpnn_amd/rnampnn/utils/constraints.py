"""Design constraints for ``rnampnn_design`` (include/rnampnn_hip.h), built on the host: a sequence pattern -> the 4-bit ``allowed`` set of
every position, a dot-bracket secondary structure -> the ``partner`` table, a per-class or per-position ``bias``.  Nothing here touches a
device until ``DesignConstraints.to_device``."""
from __future__ import annotations

import csv
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..config.glob import VOCAB

FREE = 0xF
_BRACKETS = {"(": ")", "[": "]", "{": "}", "<": ">"}
_CLOSERS = {v: k for k, v in _BRACKETS.items()}


def _bits(letters: str) -> int:
    return sum(1 << VOCAB[ch] for ch in letters)


# IUPAC nucleotide codes (T is read as U); '.' and '-' leave the position free
IUPAC = {"A": _bits("A"), "U": _bits("U"), "T": _bits("U"), "C": _bits("C"), "G": _bits("G"),
         "R": _bits("AG"), "Y": _bits("CU"), "S": _bits("CG"), "W": _bits("AU"), "K": _bits("GU"), "M": _bits("AC"),
         "B": _bits("CGU"), "D": _bits("AGU"), "H": _bits("ACU"), "V": _bits("ACG"), "N": FREE, ".": FREE, "-": FREE}


def parse_dot_bracket(text: str) -> np.ndarray:
    """Dot-bracket string -> int32 partner array (-1 = unpaired).  ``()``, ``[]``, ``{}`` and ``<>`` nest independently of each other
    (pseudoknots); ``.`` is unpaired.  ``ValueError`` on an unbalanced string or an unknown character."""
    partner = np.full(len(text), -1, dtype=np.int32)
    stacks = {k: [] for k in _BRACKETS}
    for i, ch in enumerate(text):
        if ch == ".":
            continue
        if ch in _BRACKETS:
            stacks[ch].append(i)
        elif ch in _CLOSERS:
            st = stacks[_CLOSERS[ch]]
            if not st:
                raise ValueError(f"dot-bracket: {ch!r} at position {i} closes nothing")
            j = st.pop()
            partner[i], partner[j] = j, i
        else:
            raise ValueError(f"dot-bracket: unknown character {ch!r} at position {i}")
    for k, st in stacks.items():
        if st:
            raise ValueError(f"dot-bracket: {k!r} at position {st[-1]} is never closed")
    return partner


def crossing_pairs(partner_row) -> bool:
    """Does the structure of ONE RNA hold a pseudoknot?  ``partner_row``: its partner array (``parse_dot_bracket``; a tensor or a
    sequence, -1 = unpaired).  True when two of its pairs cross, i < k < j < l.  An entry that is not symmetric or points outside the row is
    no pair, as in ``rnampnn_design``.  Host side: one pass with a stack."""
    row = [int(v) for v in (partner_row.tolist() if hasattr(partner_row, "tolist") else partner_row)]
    n, open_ = len(row), []
    for t, j in enumerate(row):
        if not (0 <= j < n and j != t and row[j] == t):
            continue
        if j > t:
            open_.append(t)
        elif open_.pop() != j:                                     # a closer must close the innermost open pair
            return True
    return False


def parse_pattern(text: str) -> np.ndarray:
    """Sequence pattern -> uint8 ``allowed`` array: AUCG (and T = U) fix a nucleotide, the IUPAC codes R Y S W K M B D H V N admit their
    sets, ``.`` and ``-`` leave the position free; case is ignored.  ``ValueError`` on any other character."""
    out = np.empty(len(text), dtype=np.uint8)
    for i, ch in enumerate(text.upper()):
        if ch not in IUPAC:
            raise ValueError(f"pattern: unknown character {text[i]!r} at position {i}")
        out[i] = IUPAC[ch]
    return out


def parse_bias(text: str) -> np.ndarray:
    """``A=..,U=..,C=..,G=..`` (any subset, T = U) -> float32 (4,) in class order; classes not named get 0."""
    out = np.zeros(4, dtype=np.float32)
    for item in filter(None, (s.strip() for s in text.split(","))):
        key, sep, val = item.partition("=")
        key = key.strip().upper().replace("T", "U")
        if not sep or key not in VOCAB:
            raise ValueError(f"bias: expected LETTER=VALUE with a letter of AUCG, got {item!r}")
        out[VOCAB[key]] = float(val)
    return out


def parse_gc_content(text: str) -> Tuple[float, float]:
    """``LO:HI`` - the G+C content window as fractions of the length, 0 <= LO <= HI <= 1 - -> (lo, hi).  ``ValueError`` otherwise."""
    lo, sep, hi = text.partition(":")
    try:
        window = (float(lo), float(hi))
    except ValueError:
        window = None
    if not sep or window is None or not 0.0 <= window[0] <= window[1] <= 1.0:
        raise ValueError(f"gc-content: expected LO:HI with fractions 0 <= LO <= HI <= 1, got {text!r}")
    return window


def read_reference_fasta(path: str) -> Dict[str, str]:
    """A FASTA file with one record per structure (``>pdb_id`` and what follows up to the first blank) -> {pdb_id: sequence}: the
    references of a mutation budget (``--mutate-from``).  ``ValueError`` for sequence lines before the first header."""
    refs: Dict[str, str] = {}
    rid = None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            rid = line[1:].split()[0] if line[1:].split() else ""
            refs[rid] = ""
        elif line:
            if rid is None:
                raise ValueError(f"{path}: sequence before the first '>' header")
            refs[rid] += line
    return refs


def mutation_references(references: Optional[Dict[str, str]], ids: Sequence[str], lengths: Sequence[int], natives) -> List[np.ndarray]:
    """The reference sequence of every structure as int32 class ids (-1 for a letter outside AUCG, which never counts as a mutation;
    T = U): ``references[pdb_id]`` when a table is given, else ``natives[i]`` (the structure's own sequence as class ids, or None).
    ``ValueError`` naming the id for a structure without a reference and for a reference of another length."""
    out = []
    for i, (rid, n) in enumerate(zip(ids, lengths)):
        if references is not None:
            if rid not in references:
                raise ValueError(f"mutations: the reference file has no sequence for {rid!r}")
            ref = np.array([VOCAB.get(ch, -1) for ch in references[rid].upper().replace("T", "U")], dtype=np.int32)
        elif natives[i] is None:
            raise ValueError(f"mutations: structure {rid!r} has no reference sequence (no usable seqs/{rid}.fasta); pass a reference file")
        else:
            ref = np.asarray(natives[i], dtype=np.int32)
        if len(ref) != int(n):
            raise ValueError(f"mutations: the reference of {rid!r} has {len(ref)} letters, the structure {int(n)} nucleotides")
        out.append(ref)
    return out


def padded_references(refs: Sequence[np.ndarray], idx: Sequence[int], max_len: int) -> torch.Tensor:
    """The references of one batch -> (B, max_len) int32, -1 on padding."""
    out = torch.full((len(idx), max_len), -1, dtype=torch.int32)
    for r, i in enumerate(idx):
        out[r, :len(refs[i])] = torch.from_numpy(refs[i])
    return out


def omit_mask(letters: str) -> int:
    """``--omit`` letters -> the ``allowed`` set without them."""
    m = FREE
    for ch in letters.upper().replace("T", "U"):
        if ch not in VOCAB:
            raise ValueError(f"omit: {ch!r} is not one of AUCG")
        m &= ~(1 << VOCAB[ch])
    return m


@dataclass
class DesignConstraints:
    """Per-batch padded tensors: ``allowed`` (B,T) uint8, ``partner`` (B,T) int32, ``bias`` (4,) or (B,T,4) float32; each may be None."""
    allowed: Optional[torch.Tensor] = None
    partner: Optional[torch.Tensor] = None
    bias: Optional[torch.Tensor] = None
    wobble: bool = True

    @classmethod
    def from_specs(cls, specs: Sequence[Tuple[Optional[str], Optional[str]]], lengths: Sequence[int], T: int, bias=None,
                   wobble: bool = True, omit: str = "") -> "DesignConstraints":
        """One ``(pattern or None, structure or None)`` per RNA -> padded host tensors (free / unpaired where nothing is given and on
        padding).  ``omit``: letters no position may draw.  ``ValueError`` when a pattern or structure is not as long as its RNA."""
        B = len(specs)
        if len(lengths) != B:
            raise ValueError(f"{B} specs for {len(lengths)} lengths")
        keep = omit_mask(omit)
        allowed = np.full((B, T), FREE, dtype=np.uint8)
        partner = np.full((B, T), -1, dtype=np.int32)
        for b, ((pattern, structure), n) in enumerate(zip(specs, lengths)):
            n = int(n)
            if n > T:
                raise ValueError(f"RNA {b}: length {n} exceeds T = {T}")
            if pattern:
                if len(pattern) != n:
                    raise ValueError(f"RNA {b}: pattern of length {len(pattern)} for an RNA of length {n}")
                allowed[b, :n] = parse_pattern(pattern)
            if structure:
                if len(structure) != n:
                    raise ValueError(f"RNA {b}: structure of length {len(structure)} for an RNA of length {n}")
                partner[b, :n] = parse_dot_bracket(structure)
        allowed &= np.uint8(keep)
        have_allowed = keep != FREE or any(p for p, _ in specs)
        have_partner = any(s for _, s in specs)
        return cls(allowed=torch.from_numpy(allowed) if have_allowed else None,
                   partner=torch.from_numpy(partner) if have_partner else None,
                   bias=None if bias is None else torch.as_tensor(np.asarray(bias, dtype=np.float32)), wobble=wobble)

    def to_device(self, device) -> "DesignConstraints":
        mv = lambda t, dt: None if t is None else t.to(device=device, dtype=dt).contiguous()
        return DesignConstraints(mv(self.allowed, torch.uint8), mv(self.partner, torch.int32), mv(self.bias, torch.float32), self.wobble)


def read_constraints_csv(path: str) -> Dict[str, Tuple[str, str]]:
    """CSV with the columns ``pdb_id,fixed,structure`` -> {pdb_id: (pattern, structure)}; either field may be empty."""
    out = {}
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        missing = {"pdb_id", "fixed", "structure"} - set(rd.fieldnames or ())
        if missing:
            raise ValueError(f"{path}: missing column(s) {sorted(missing)} (expected pdb_id,fixed,structure)")
        for row in rd:
            out[row["pdb_id"].strip()] = ((row["fixed"] or "").strip(), (row["structure"] or "").strip())
    return out


def batch_constraints(table: Optional[Dict[str, Tuple[str, str]]], ids: Sequence[str], lengths: Sequence[int], T: int, bias=None,
                      wobble: bool = True, omit: str = "") -> DesignConstraints:
    """The constraints of one batch from a ``read_constraints_csv`` table: ids not in it are unconstrained; a row whose pattern or structure
    is not as long as its structure file is an error that names the id."""
    specs = []
    for rid, n in zip(ids, lengths):
        pattern, structure = (table or {}).get(rid, ("", ""))
        for what, text in (("fixed", pattern), ("structure", structure)):
            if text and len(text) != int(n):
                raise ValueError(f"constraints for {rid}: {what} has {len(text)} characters, the structure has {int(n)} nucleotides")
        try:                                                      # a malformed row names its id too
            parse_pattern(pattern), parse_dot_bracket(structure)
        except ValueError as exc:
            raise ValueError(f"constraints for {rid}: {exc}") from None
        specs.append((pattern or None, structure or None))
    return DesignConstraints.from_specs(specs, lengths, T, bias=bias, wobble=wobble, omit=omit)


def read_states_csv(path: str) -> Dict[str, List[Tuple[str, float]]]:
    """Multi-state design: CSV with the columns ``design_id,pdb_id,weight`` -> {design_id: [(pdb_id, weight), ...]}, designs and their states
    in file order.  The structures listed under one ``design_id`` are the states of ONE design; an empty ``weight`` is 1 (a negative one
    designs against that state).  ``ValueError`` naming a missing column or a ``pdb_id`` listed twice."""
    out: Dict[str, List[Tuple[str, float]]] = {}
    seen = set()
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        missing = {"design_id", "pdb_id", "weight"} - set(rd.fieldnames or ())
        if missing:
            raise ValueError(f"{path}: missing column(s) {sorted(missing)} (expected design_id,pdb_id,weight)")
        for row in rd:
            did, rid, w = (row["design_id"] or "").strip(), (row["pdb_id"] or "").strip(), (row["weight"] or "").strip()
            if rid in seen:
                raise ValueError(f"{path}: pdb_id {rid!r} is listed twice (a structure is a state of one design)")
            seen.add(rid)
            try:
                out.setdefault(did, []).append((rid, float(w) if w else 1.0))
            except ValueError:
                raise ValueError(f"{path}: weight {w!r} of pdb_id {rid!r} is not a number") from None
    return out
