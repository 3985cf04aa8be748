"""Forbidden motifs for ``rnampnn_design_avoid`` (include/rnampnn_hip.h), built on the host: a set of substrings over AUCG (IUPAC codes
expand to their sets, ``max_run`` adds the homopolymers) -> an Aho-Corasick automaton with the failure links compiled out, as the table
``delta`` (A,4) of next states and the bit set ``terminal`` of the states in which a motif has just ended.  ``hits`` follows the table over
given sequences (torch only, CPU or device): the user-facing "does this sequence contain a motif" check.  ``DesignAutomaton`` is the
automaton of ``rnampnn_design_dfa``: motifs that MUST occur somewhere together with motifs that must not - the same trie times the set of
required motifs seen so far, up to 256 states, with ``kind`` (dead / accepting per state) in place of ``terminal`` and ``scan`` for ``hits``."""
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


DFA_MAX_STATES = 256                                               # RNAMPNN_DESIGN_DFA_MAX_STATES: one thread of the workgroup per state
DFA_MAX_REQUIRED = 6
KIND_DEAD, KIND_ACCEPTING = 1, 2


class DesignAutomaton:
    """The automaton of ``rnampnn_design_dfa`` (include/rnampnn_hip.h): motifs that MUST occur and motifs that must NOT.  ``delta`` (A,4)
    uint8 host tensor, as ``MotifAutomaton``'s; ``kind`` (A,) uint8 host tensor: bit 0 = dead (an avoided word ends in this state or on
    its suffix chain), bit 1 = accepting (not dead and every required motif seen).  A state is (node of the Aho-Corasick trie over the
    words of both lists, set of required motifs seen so far); only the states reachable from (root, none) exist, numbered breadth-first
    with the classes in order, so the tables are a function of the two motif SETS; nothing is minimised.  ``words``: the expanded avoided
    words as sorted class-id tuples; ``required``: per required motif the sorted tuple of its expansions."""

    def __init__(self, delta: torch.Tensor, kind: torch.Tensor, words=(), required=()):
        self.delta, self.kind, self.words, self.required = delta, kind, tuple(words), tuple(required)
        self._dev = {}

    @property
    def n_states(self) -> int:
        return int(self.delta.shape[0])

    @property
    def n_live(self) -> int:
        """The states that are not dead: the columns of the kernel's table."""
        return int(((self.kind & KIND_DEAD) == 0).sum())

    @classmethod
    def from_motifs(cls, require: Iterable[str] = (), avoid: Iterable[str] = (), max_run: Optional[int] = None) -> "DesignAutomaton":
        """``require``: motifs (AUCG, T = U, IUPAC codes expand) that must EVERY ONE occur at least once, any expansion of a motif
        counting as that motif; ``avoid`` / ``max_run``: as ``MotifAutomaton.from_motifs`` takes them.  Duplicates and the order do not
        matter.  ``ValueError`` for an empty or unknown motif, ``max_run < 1``, an empty ``require`` (``MotifAutomaton`` serves avoid
        alone), more than 6 required motifs and an automaton of more than 256 states (the message names the count)."""
        require = [require] if isinstance(require, str) else list(require if require is not None else ())
        avoid = [avoid] if isinstance(avoid, str) else list(avoid if avoid is not None else ())
        required = sorted({tuple(sorted(set(expand_motif(m)))) for m in require})
        if not required:
            raise ValueError("motifs: require is empty (MotifAutomaton and design(..., avoid=...) serve forbidden motifs alone)")
        if len(required) > DFA_MAX_REQUIRED:
            raise ValueError(f"motifs: {len(required)} required motifs, the limit is {DFA_MAX_REQUIRED} (the seen flags multiply the states)")
        banned = set()
        for m in avoid:
            banned.update(expand_motif(m))
        if max_run is not None:
            if int(max_run) < 1:
                raise ValueError(f"motifs: max_run = {max_run} must be at least 1")
            banned.update((c,) * (int(max_run) + 1) for c in range(4))
        # one trie over the words of both lists; per node the required motifs and whether an avoided word ends there
        children, seen_here, dead_here = [[-1] * 4], [0], [False]

        def insert(w):
            node = 0
            for c in w:
                if children[node][c] < 0:
                    children[node][c] = len(children)
                    children.append([-1] * 4)
                    seen_here.append(0)
                    dead_here.append(False)
                node = children[node][c]
            return node
        for i, group in enumerate(required):
            for w in group:
                seen_here[insert(w)] |= 1 << i
        for w in sorted(banned):
            dead_here[insert(w)] = True
        # failure links compiled out, breadth-first: a missing edge of a node is the edge of its suffix node; the marks follow the chain
        N = len(children)
        step, fail_of, order, queue = [[0] * 4 for _ in range(N)], [0] * N, [], deque([0])
        while queue:
            node = queue.popleft()
            order.append(node)
            if node:
                seen_here[node] |= seen_here[fail_of[node]]
                dead_here[node] = dead_here[node] or dead_here[fail_of[node]]
            for c in range(4):
                k = children[node][c]
                if k >= 0:
                    step[node][c] = k
                    fail_of[k] = step[fail_of[node]][c] if node else 0
                    queue.append(k)
                else:
                    step[node][c] = step[fail_of[node]][c] if node else 0
        # the product with the seen set: reachable states only, breadth-first from (root, none) with the classes in order
        number, states, queue = {(0, 0): 0}, [(0, 0)], deque([(0, 0)])
        delta = []
        while queue:
            node, seen = queue.popleft()
            row = []
            for c in range(4):
                k = step[node][c]
                nxt = (k, seen | seen_here[k])
                if nxt not in number:
                    number[nxt] = len(states)
                    states.append(nxt)
                    queue.append(nxt)
                row.append(number[nxt])
            delta.append(row)
        A = len(states)
        if A > DFA_MAX_STATES:
            raise ValueError(f"motifs: the automaton of these {len(required)} required motifs and {len(banned)} avoided words has {A} states, "
                             f"the limit is {DFA_MAX_STATES} (one thread of a workgroup per state): require or avoid fewer or shorter motifs")
        full = (1 << len(required)) - 1
        kind = [KIND_DEAD if dead_here[node] else (KIND_ACCEPTING if seen == full else 0) for node, seen in states]
        return cls(torch.tensor(delta, dtype=torch.uint8), torch.tensor(kind, dtype=torch.uint8), sorted(banned), required)

    @classmethod
    def from_avoid(cls, avoid=(), max_run: Optional[int] = None) -> "DesignAutomaton":
        """Forbidden motifs ALONE in the form ``rnampnn_design_nested`` takes them: ``MotifAutomaton``'s table (``avoid``: one, or motif
        strings with ``max_run``, as its ``from_motifs`` takes them) with ``kind`` = dead where a motif ends and accepting everywhere
        else.  ``from_motifs`` keeps refusing an empty ``require``; this is the separate door for avoid alone."""
        auto = as_automaton(avoid if avoid is not None else (), max_run)
        kind = [KIND_DEAD if (auto.terminal >> a) & 1 else KIND_ACCEPTING for a in range(auto.n_states)]
        return cls(auto.delta, torch.tensor(kind, dtype=torch.uint8), auto.words, ())

    def letters(self) -> List[str]:
        """The expanded avoided words as strings over AUCG."""
        return ["".join(REVERSE_VOCAB[c] for c in w) for w in self.words]

    def delta_on(self, device) -> torch.Tensor:
        """``delta`` on ``device``, uploaded once per device."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.delta.to(device).contiguous()
        return self._dev[key]

    def scan(self, seqs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(..., T) class ids with -1 on padding -> (hits, accepted), both (...) int32: the dead states entered following ``delta`` from
        the start (the positions at which an avoided word ends), and 1 where the state after the last nucleotide is accepting.  An id
        outside 0..3 is padding: it neither moves the automaton nor counts.  Torch only, on the device of ``seqs``."""
        ids = seqs.to(torch.int64)
        flat = ids.reshape(-1, ids.shape[-1]) if ids.dim() else ids.reshape(1, 1)
        table = self.delta_on(flat.device).to(torch.int64).reshape(-1)
        kind = self.kind.to(flat.device).to(torch.int32)
        state = torch.zeros(flat.shape[0], dtype=torch.int64, device=flat.device)
        count = torch.zeros(flat.shape[0], dtype=torch.int32, device=flat.device)
        for t in range(flat.shape[1]):
            c = flat[:, t]
            valid = (c >= 0) & (c <= 3)
            state = torch.where(valid, table[state * 4 + c.clamp(0, 3)], state)
            count = count + torch.where(valid, kind[state] & KIND_DEAD, torch.zeros_like(count))
        accepted = ((kind[state] & 3) == KIND_ACCEPTING).to(torch.int32)
        return count.reshape(ids.shape[:-1]), accepted.reshape(ids.shape[:-1])


def as_design_automaton(require, avoid=None, max_run: Optional[int] = None) -> Optional[DesignAutomaton]:
    """``design(..., require=..., avoid=...)``: a ``DesignAutomaton`` or motif strings (``avoid``: motif strings or a ``MotifAutomaton``,
    whose words are taken) -> the automaton; None when ``require`` is None."""
    if require is None or isinstance(require, DesignAutomaton):
        return require
    if isinstance(avoid, MotifAutomaton):
        avoid = avoid.letters()
    return DesignAutomaton.from_motifs(require, avoid if avoid is not None else (), max_run=max_run)


def as_nested_automaton(require=None, avoid=None, max_run: Optional[int] = None) -> Optional[DesignAutomaton]:
    """``design(..., pairs="nested", require=..., avoid=...)`` -> the ``DesignAutomaton`` of ``rnampnn_design_nested``: ``require`` with
    ``avoid`` absorbed (``as_design_automaton``), or ``avoid`` / ``max_run`` alone with every live state accepting
    (``DesignAutomaton.from_avoid``); None when none of the three is given."""
    if require is not None:
        return as_design_automaton(require, avoid, max_run)
    if avoid is None and max_run is None:
        return None
    return DesignAutomaton.from_avoid(avoid, max_run)


def as_automaton(avoid, max_run: Optional[int] = None) -> Optional[MotifAutomaton]:
    """``design(..., avoid=...)``: a ``MotifAutomaton``, a motif string or an iterable of motif strings -> the automaton; None for None."""
    if avoid is None or isinstance(avoid, MotifAutomaton):
        return avoid
    return MotifAutomaton.from_motifs(avoid, max_run=max_run)
