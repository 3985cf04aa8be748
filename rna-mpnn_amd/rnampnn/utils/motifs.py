"""Forbidden motifs for ``rnampnn_design_avoid`` (include/rnampnn_hip.h), built on the host: a set of substrings over AUCG (IUPAC codes
expand to their sets, ``max_run`` adds the homopolymers) -> an Aho-Corasick automaton with the failure links compiled out, as the table
``delta`` (A,4) of next states and the bit set ``terminal`` of the states in which a motif has just ended.  ``hits`` follows the table over
given sequences (torch only, CPU or device): the user-facing "does this sequence contain a motif" check."""
from __future__ import annotations

import itertools
from collections import deque
from typing import Iterable, List, Optional, Tuple

import torch

from ..config.glob import REVERSE_VOCAB
from .constraints import IUPAC

MAX_STATES = 64                                                    # RNAMPNN_DESIGN_AVOID_MAX_STATES: one lane of a wave per state
_CODES = {ch: m for ch, m in IUPAC.items() if ch.isalpha()}


def expand_motif(motif: str) -> List[Tuple[int, ...]]:
    """One motif - AUCG, T read as U, IUPAC codes as their sets, any case - -> the class-id tuples it stands for.  ``ValueError`` for an
    empty motif or an unknown letter."""
    text = str(motif).strip().upper()
    if not text:
        raise ValueError("motifs: an empty motif")
    sets = []
    for i, ch in enumerate(text):
        if ch not in _CODES:
            raise ValueError(f"motifs: unknown letter {str(motif).strip()[i]!r} in {motif!r} (AUCG, T, or an IUPAC code)")
        sets.append([c for c in range(4) if (_CODES[ch] >> c) & 1])
    return list(itertools.product(*sets))


class MotifAutomaton:
    """``delta`` (A,4) uint8 host tensor: the state after reading class c (the order of ``REVERSE_VOCAB``) in state a; ``terminal``: a
    Python int whose bit a is set iff a motif ends in state a or in a state on its suffix-link chain; state 0 is the start and never
    terminal; the states are numbered breadth-first with the classes in order, so the table is a function of the motif SET alone.
    ``words``: the expanded motifs as sorted class-id tuples."""

    def __init__(self, delta: torch.Tensor, terminal: int, words=()):
        self.delta, self.terminal, self.words = delta, int(terminal), tuple(words)
        self._dev = {}

    @property
    def n_states(self) -> int:
        return int(self.delta.shape[0])

    @property
    def n_live(self) -> int:
        """The states that are not terminal: the columns of the kernel's table."""
        return self.n_states - bin(self.terminal).count("1")

    @classmethod
    def from_motifs(cls, motifs: Iterable[str], max_run: Optional[int] = None) -> "MotifAutomaton":
        """``motifs``: strings over AUCG (T = U, IUPAC codes expand); ``max_run=r`` adds the four homopolymers of length r + 1.  Duplicates
        and the order do not matter.  ``ValueError`` for an empty motif, an unknown letter, no motif at all, ``max_run < 1`` and a set
        whose automaton has more than 64 states (the message names the count)."""
        if isinstance(motifs, str):
            motifs = [motifs]
        words = set()
        for m in motifs:
            words.update(expand_motif(m))
        if max_run is not None:
            if int(max_run) < 1:
                raise ValueError(f"motifs: max_run = {max_run} must be at least 1")
            words.update((c,) * (int(max_run) + 1) for c in range(4))
        if not words:
            raise ValueError("motifs: no motif given (pass at least one motif or max_run)")
        # the trie, then breadth-first numbering with the classes in order
        children, ends = [[-1] * 4], [False]
        for w in sorted(words):
            node = 0
            for c in w:
                if children[node][c] < 0:
                    children[node][c] = len(children)
                    children.append([-1] * 4)
                    ends.append(False)
                node = children[node][c]
            ends[node] = True
        A = len(children)
        if A > MAX_STATES:
            raise ValueError(f"motifs: the automaton of these {len(words)} motifs has {A} states, the limit is {MAX_STATES} "
                             "(one lane of a wave per state): forbid fewer or shorter motifs")
        order, queue = [], deque([0])
        while queue:
            node = queue.popleft()
            order.append(node)
            queue.extend(k for k in children[node] if k >= 0)
        number = {node: i for i, node in enumerate(order)}
        # failure links compiled out, in breadth-first order: a missing edge of a state is the edge of its suffix state
        delta = [[0] * 4 for _ in range(A)]
        fail = [0] * A
        terminal = 0
        for i, node in enumerate(order):
            if ends[node] or (terminal >> fail[i]) & 1:
                terminal |= 1 << i
            for c in range(4):
                k = children[node][c]
                if k >= 0:
                    delta[i][c] = number[k]
                    fail[number[k]] = delta[fail[i]][c] if i else 0
                else:
                    delta[i][c] = delta[fail[i]][c] if i else 0
        return cls(torch.tensor(delta, dtype=torch.uint8), terminal, sorted(words))

    def letters(self) -> List[str]:
        """The expanded motifs as strings over AUCG."""
        return ["".join(REVERSE_VOCAB[c] for c in w) for w in self.words]

    def delta_on(self, device) -> torch.Tensor:
        """``delta`` on ``device``, uploaded once per device."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.delta.to(device).contiguous()
        return self._dev[key]

    def hits(self, seqs: torch.Tensor) -> torch.Tensor:
        """(..., T) class ids with -1 on padding -> (...) int32: the positions after which the automaton, following ``delta`` from the
        start, is in a terminal state - for an automaton built from motifs the positions at which a motif ends; 0 = the sequence holds
        none.  An id outside 0..3 is padding: it neither moves the automaton nor counts.  Torch only, on the device of ``seqs``."""
        ids = seqs.to(torch.int64)
        flat = ids.reshape(-1, ids.shape[-1]) if ids.dim() else ids.reshape(1, 1)
        table = self.delta_on(flat.device).to(torch.int64).reshape(-1)
        term = torch.tensor([(self.terminal >> a) & 1 for a in range(self.n_states)], dtype=torch.int32, device=flat.device)
        state = torch.zeros(flat.shape[0], dtype=torch.int64, device=flat.device)
        count = torch.zeros(flat.shape[0], dtype=torch.int32, device=flat.device)
        for t in range(flat.shape[1]):
            c = flat[:, t]
            valid = (c >= 0) & (c <= 3)
            state = torch.where(valid, table[state * 4 + c.clamp(0, 3)], state)
            count = count + torch.where(valid, term[state], torch.zeros_like(count))
        return count.reshape(ids.shape[:-1])


def as_automaton(avoid, max_run: Optional[int] = None) -> Optional[MotifAutomaton]:
    """``design(..., avoid=...)``: a ``MotifAutomaton``, a motif string or an iterable of motif strings -> the automaton; None for None."""
    if avoid is None or isinstance(avoid, MotifAutomaton):
        return avoid
    return MotifAutomaton.from_motifs(avoid, max_run=max_run)
