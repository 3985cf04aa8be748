"""Float64 numpy restatement of the draw ``rnampnn_design_nested`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_nested_*.py.  Per RNA a ``NestedPlan`` holds what does not depend on the sample - z, the masks, the validated and
feasible pairs, ``nest_miss``, the transfer tables R_t(a, g) over the live states (one per unpaired position and per opener; L x L inside
a pair, L x 1 at the top level, where the one goal is "accepted"), ``dfa_miss`` - and walks forward per sample with the hash of
``_design_ref``, a goal and a stack of goals; ``lse`` and ``Selection`` are ``_design_gc_ref``'s, ``follow`` / ``naive_hits`` the sibling
restatements'.  Besides the ids a draw returns the smallest margin of the selections on its path (see ``_design_gc_ref``).
``path_logprob`` multiplies the conditionals along the path of a GIVEN sequence (the exactness check against a brute-force joint).  The
automaton's tables (``delta``, ``kind``: bit 0 dead, bit 1 accepting) are an INPUT here, as they are for the kernel."""
import numpy as np

from _design_ref import COMPAT, u24
from _design_gc_ref import NEG, Selection, lse
from _design_avoid_ref import expand, naive_hits  # noqa: F401  (the tests' substring scans)
from _design_dfa_ref import DEAD, ACCEPTING, contains_all, follow, required_sets  # noqa: F401

ACCEPTED = 0                                                       # the one goal of the top level: column 0 of an (L,1) table


def crossing(mate):
    """Do two pairs of ``mate`` (partner per position, -1 = unpaired) cross: i < k < j < l?  By the definition, pair against pair."""
    pairs = [(t, int(j)) for t, j in enumerate(mate) if int(j) > t]
    return int(any(i < k < j < l for i, j in pairs for k, l in pairs))


class NestedPlan:
    def __init__(self, logits, n, temperature, delta, kind, allowed=None, partner=None, wobble=True, bias=None):
        n = int(n)
        self.n, self.wobble = n, bool(wobble)
        wob = self.wobble
        self.delta = delta = np.asarray(delta).astype(np.int64).reshape(-1, 4)
        self.kind = kind = np.asarray(kind).astype(np.int64)
        self.A = A = delta.shape[0]
        dead = (kind & DEAD) != 0
        self._sel, self._known = {}, {}                            # the selections and the candidate lists met so far
        z = np.asarray(logits)[:n].astype(np.float64)
        if bias is not None:
            bias = np.asarray(bias)
            z = z + (bias if bias.ndim == 1 else bias[:n]).astype(np.float64)
        self.z = z = z / float(np.float32(temperature))
        mask = np.full(n, 15, dtype=np.int64) if allowed is None else (np.asarray(allowed)[:n].astype(np.int64) & 15)
        self.infeasible = int((mask == 0).sum())
        self.mask = mask = np.where(mask == 0, 15, mask)
        # the pairs: validated as rnampnn_design validates them; one without an admitted compatible cell becomes two single positions
        self.mate = mate = np.full(n, -1, dtype=np.int64)
        self.cells = {}                                            # opener -> its admitted compatible cells (c, c'), a-major
        for t in range(n):
            j = -1 if partner is None else int(partner[t])
            if t < j < n and int(partner[j]) == t:
                cells = [(a, c) for a in range(4) for c in range(4) if (mask[t] >> a) & 1 and (mask[j] >> c) & 1 and (COMPAT[wob][a] >> c) & 1]
                if cells:
                    mate[t], mate[j] = j, t
                    self.cells[t] = cells
                else:
                    self.infeasible += 2
        self.nest_miss = crossing(mate)
        # the automaton over its live states: column k is the k-th live state; col[a, c] = the column of delta(a, c), -1 when it is dead
        self.states = states = np.nonzero(~dead)[0]
        self.L = L = len(states)
        number = np.full(A, -1, dtype=np.int64)
        number[states] = np.arange(L)
        inside = delta[states] < A
        self.col = col = np.where(inside, number[np.where(inside, delta[states], 0)], -1)      # (L,4)
        self.accepting = accepting = (kind[states] & ACCEPTING) != 0
        self.final = np.where(accepting, 0.0, NEG)[:, None]                                    # behind position n-1, (L,1)
        self.identity = np.where(np.eye(L, dtype=bool), 0.0, NEG)                              # behind an inner loop's last element
        self.R, self.top = {}, np.ones(n, dtype=bool)
        self.miss = 0
        if self.nest_miss:
            return
        depth = 0
        for t in range(n):
            if 0 <= mate[t] < t:
                depth -= 1
            self.top[t] = depth == 0
            if mate[t] > t:
                depth += 1
        with np.errstate(invalid="ignore"):
            for t in range(n - 1, -1, -1):
                j = int(mate[t])
                if 0 <= j < t:
                    continue
                if j < 0:
                    N = self.table(t + 1, self.top[t])
                    terms = np.full((L, 4, N.shape[1]), NEG)
                    for c in range(4):
                        ok = (col[:, c] >= 0) & bool((mask[t] >> c) & 1)
                        terms[ok, c] = z[t, c] + N[col[ok, c]]
                    self.R[t] = lse(terms, axis=1)
                    continue
                Rin, N = self.table(t + 1, False), self.table(j + 1, self.top[t])
                # P_t(a, b): per goal b the terms (cell, b') with delta(b', c') = b, cells a-major, b' ascending
                blocks, goals = [], []
                for c, c2 in self.cells[t]:
                    block = np.full((L, L), NEG)
                    ok = col[:, c] >= 0
                    block[ok] = (z[t, c] + z[j, c2]) + Rin[col[ok, c]]
                    blocks.append(block)
                    goals.append(col[:, c2])
                blocks, goals = np.concatenate(blocks, axis=1), np.concatenate(goals)
                P = np.full((L, L), NEG)
                for b in range(L):
                    pick = np.nonzero(goals == b)[0]
                    if pick.size:
                        P[:, b] = lse(blocks[:, pick], axis=1)
                self.R[t] = lse(P[:, :, None] + N[None, :, :], axis=1)
        self.miss = int(not self.table(0, True)[0, ACCEPTED] > NEG)

    def table(self, x, top):
        """The table of the element that starts at x in a loop: behind position n-1, behind a loop's last element, or R_x."""
        if x >= self.n:
            return self.final
        if 0 <= self.mate[x] < x:
            return self.identity
        return self.R[x]

    # ---- the candidates of one selection and their log-weights
    def _free(self, t):
        j = int(self.mate[t])                                      # (never a closer)
        if j < 0:
            cs = [c for c in range(4) if (self.mask[t] >> c) & 1]
            return cs, np.array([self.z[t, c] for c in cs])
        return self.cells[t], np.array([self.z[t, a] + self.z[j, c] for a, c in self.cells[t]])

    def _single(self, t, a, g):
        N = self.table(t + 1, self.top[t])
        cs = [c for c in range(4) if (self.mask[t] >> c) & 1 and self.col[a, c] >= 0 and N[self.col[a, c], g] > NEG]
        return cs, np.array([self.z[t, c] + N[self.col[a, c], g] for c in cs])

    def _pair(self, t, a, g):
        j = int(self.mate[t])
        Rin, N = self.table(t + 1, False), self.table(j + 1, self.top[t])
        cands, terms = [], []
        for c, c2 in self.cells[t]:
            k = self.col[a, c]
            if k < 0:
                continue
            for b2 in range(self.L):
                k2 = self.col[b2, c2]
                if k2 >= 0 and Rin[k, b2] > NEG and N[k2, g] > NEG:
                    cands.append((c, c2, b2))
                    terms.append(self.z[t, c] + self.z[j, c2] + Rin[k, b2] + N[k2, g])
        return cands, np.array(terms)

    def _cands(self, key, make):
        if key not in self._known:
            self._known[key] = make()
        return self._known[key]

    def _pick(self, key, make, u_bits, margins):
        if key not in self._sel:
            cands, terms = make()
            self._sel[key] = (cands, Selection(terms, leaf=True))
        cands, sel = self._sel[key]
        k, m = sel.pick(u_bits, margins)
        return cands[k], m

    def draw(self, seed, s, b, margins=True):
        """-> (ids (n,) int8, the smallest margin on the path)."""
        seq = np.full(self.n, -1, dtype=np.int8)
        margin, a, g, stack = np.inf, 0, ACCEPTED, []
        plain = self.miss or self.nest_miss
        for t in range(self.n):
            j = int(self.mate[t])
            if 0 <= j < t:                                         # a closer: its class came with the opener's
                if not plain:
                    a, g = int(self.col[a, seq[t]]), stack.pop()
                continue
            if plain:
                got, m = self._pick(("free", t), lambda: self._free(t), u24(seed, s, b, t), margins)
                if j < 0:
                    seq[t] = got
                else:
                    seq[t], seq[j] = got
            elif j < 0:
                got, m = self._pick((t, a, g), lambda: self._single(t, a, g), u24(seed, s, b, t), margins)
                seq[t], a = got, int(self.col[a, got])
            else:
                (c, c2, b2), m = self._pick((t, a, g), lambda: self._pair(t, a, g), u24(seed, s, b, t), margins)
                seq[t], seq[j] = c, c2
                stack.append(g)
                a, g = int(self.col[a, c]), b2
            margin = min(margin, m)
        return seq, margin

    def path_logprob(self, seq):
        """log of the product of the conditionals the draw multiplies along the path that ends in ``seq`` (-inf when it cannot be drawn)."""
        lp, a, g, stack = 0.0, 0, ACCEPTED, []
        plain = self.miss or self.nest_miss
        for t in range(self.n):
            j = int(self.mate[t])
            if 0 <= j < t:
                if not plain:
                    a, g = int(self.col[a, int(seq[t])]), stack.pop()
                continue
            if plain:
                cands, terms = self._cands(("free", t), lambda: self._free(t))
                want = int(seq[t]) if j < 0 else (int(seq[t]), int(seq[j]))
            elif j < 0:
                cands, terms = self._cands((t, a, g), lambda: self._single(t, a, g))
                want = int(seq[t])
            else:
                inner = int(self.col[a, int(seq[t])])               # the state before the closer, following the sequence inside the pair
                for x in range(t + 1, j):
                    inner = -1 if inner < 0 else int(self.col[inner, int(seq[x])])
                cands, terms = self._cands((t, a, g), lambda: self._pair(t, a, g))
                want = (int(seq[t]), int(seq[j]), inner)
            if want not in cands:
                return NEG
            lp += terms[cands.index(want)] - lse(terms)
            if not plain:
                if j >= 0:
                    stack.append(g)
                    g = want[2]
                a = int(self.col[a, int(seq[t])])
        return float(lp)


def design_nested_ref(logits, lengths, temperature, S, seed, delta, kind, allowed=None, partner=None, wobble=True, bias=None):
    """Padded (B,T,4) logits -> dict: seqs (S,B,T) int8, margin (S,B) f64, infeasible, dfa_miss, nest_miss (B,), hits, accepted (S,B), plans."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    margin = np.full((S, B), np.inf)
    hits, accepted = np.zeros((S, B), dtype=np.int32), np.zeros((S, B), dtype=np.int32)
    bad, miss, nest, plans = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plan = NestedPlan(logits[b], lengths[b], temperature, delta, kind, None if allowed is None else allowed[b],
                          None if partner is None else partner[b], wobble, bi)
        plans.append(plan)
        bad[b], miss[b], nest[b] = plan.infeasible, plan.miss, plan.nest_miss
        for s in range(S):
            seqs[s, b, :plan.n], margin[s, b] = plan.draw(int(seed), s, b)
            hits[s, b], accepted[s, b] = follow(seqs[s, b], delta, kind)
    return dict(seqs=seqs, margin=margin, infeasible=bad, dfa_miss=miss, nest_miss=nest, hits=hits, accepted=accepted, plans=plans)


def brute_force(plan):
    """Every sequence of a short RNA -> (4^n,) log-weights of the joint the entry conditions: the sum of z over the positions when the masks
    admit it, every feasible pair is compatible and the automaton, never leaving its live states, accepts it; -inf otherwise.  Knows no
    table: pairs are compared end against end and the automaton is followed letter by letter."""
    import itertools
    out = []
    for seq in itertools.product(range(4), repeat=plan.n):
        ok = all((plan.mask[t] >> c) & 1 for t, c in enumerate(seq))
        ok = ok and all((COMPAT[plan.wobble][seq[t]] >> seq[int(j)]) & 1 for t, j in enumerate(plan.mate) if j > t)
        a = 0
        for c in seq:
            nxt = int(plan.delta[a, c])
            ok = ok and nxt < plan.A and not plan.kind[nxt] & DEAD
            a = nxt if ok else 0
        ok = ok and (plan.kind[a] & 3) == ACCEPTING
        out.append(sum(plan.z[t, c] for t, c in enumerate(seq)) if ok else NEG)
    return np.array(out, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# The siblings' lengths, T = 300, S = 4, logits 3 * randn, a seed above 2^32, wobble pairs allowed.
#   b  n    what it is there for
#   0  0    the empty RNA: feasible iff state 0 accepts
#   1  1    one unpaired position: shorter than every required motif
#   2  2    "()": a pair of adjacent positions that closes at n-1; its interior is the identity
#   3  3    "(.)" with allowed[1] = 0 inside the pair: drawn as free, counts 1 in `infeasible`
#   4  63   a stem whose ends cannot avoid a run: 10..12 fixed to A, 13 admits A or C but pairs with 30, fixed to U, which rules C out, so
#           the stem spells AAAA: dfa_miss = 1 under every automaton with max_run = 3; two more stems and a hairpin around it
#   5  64   G + 6; 18..27 open a 10-pair stem and 20..26 are fixed to GGAGGAA, which spells GGAGG and GNRA (GGAA) inside it; 30 (IUPAC Y)
#           opens a hairpin in its loop; 40 omits G; 2 and 60, both fixed to A, are a pair that cannot pair: two single positions, counts 2
#   6  65   a pseudoknot ([ ] crosses ( )): nest_miss = 1, drawn as rnampnn_design draws it; allowed[5] = 0 counts 1
#   7  257  a per-position bias (the other rows' bias is zero), G + 6; an 8-deep stem, a multiloop of two hairpins, an adjacent pair
#   8  300  G + 6; the outermost pair closes at n-1 = 299, inside it a 7-deep stem, a multiloop, "()" and a 5-deep stem: depth 8
CASE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 257, 300]
CASE_T, CASE_S = 300, 4
CASE_SEED = 0x0123_4567_89AB_CDEB                                  # above 2^32: the 64-bit seed arithmetic is exercised
CASE_INFEASIBLE = [0, 0, 0, 1, 0, 2, 1, 0, 0]
CASE_NEST = [0, 0, 0, 0, 0, 0, 1, 0, 0]
CASE_G_RAISED = (5, 7, 8)
# The automata: (require, avoid, max_run).  No run longer than 3 alone (17 states, 13 live, every live state accepting); an IUPAC tetraloop
# with no run longer than 3 (61 states, 53 live); one required 5-mer (11 states).
CASE_AUTOMATA = {"max_run3": ((), (), 3), "gnra_run3": (("GNRA",), (), 3), "ggagg": (("GGAGG",), (), None)}
# dfa_miss per automaton: RNA 4 under max_run = 3; the short RNAs under a required motif longer than they are (RNA 6 is not built: 0)
CASE_MISS = {"max_run3": [0, 0, 0, 0, 1, 0, 0, 0, 0], "gnra_run3": [1, 1, 1, 1, 1, 0, 0, 0, 0], "ggagg": [1, 1, 1, 1, 0, 0, 0, 0, 0]}


def _hairpin(k, loop):
    return "(" * k + "." * loop + ")" * k


def _pad(text, n, left=2):
    assert len(text) + left <= n, (len(text), n)
    return "." * left + text + "." * (n - left - len(text))


def case_structures():
    """One dot-bracket string per RNA ([ ] marks the crossing stem of RNA 6)."""
    s4 = list("." * 63)
    for i, j in ((10, 33), (11, 32), (12, 31), (13, 30), (2, 50), (3, 49), (4, 48), (16, 26), (17, 25), (40, 46), (41, 45)):
        s4[i], s4[j] = "(", ")"
    s5 = list("." * 64)
    for k in range(10):
        s5[18 + k], s5[50 - k] = "(", ")"
    for i, j in ((30, 36), (31, 35), (2, 60), (5, 57)):
        s5[i], s5[j] = "(", ")"
    s6 = _pad("((((...[[[...))))...]]]" + "..." + _hairpin(3, 4), 65, left=8)
    s7 = _pad(_hairpin(8, 3) + "." + "(((" + _hairpin(2, 3) + _hairpin(2, 4) + ")))" + "..()..." + _hairpin(4, 6), 257, left=30)
    inner = _pad(".." + _hairpin(7, 4) + "..." + "((" + _hairpin(3, 3) + ".." + _hairpin(4, 5) + "." + "))" + "()" + "...." + _hairpin(5, 3), 298, left=100)
    return ["", ".", "()", "(.)", "".join(s4), "".join(s5), s6, s7, "(" + inner + ")"]


def parse_structure(text):
    """Dot-bracket -> partner array; ( ) and [ ] nest independently of each other."""
    mate, stacks = np.full(len(text), -1, dtype=np.int32), {"(": [], "[": []}
    for i, ch in enumerate(text):
        if ch in stacks:
            stacks[ch].append(i)
        elif ch in ")]":
            j = stacks["(" if ch == ")" else "["].pop()
            mate[i], mate[j] = j, i
    assert not any(stacks.values())
    return mate


def case_arrays():
    """-> dict of numpy arrays: logits (B,T,4) f32 (zero on padding), mask, allowed, partner, bias (B,T,4), packed, cu."""
    B, T = len(CASE_LENGTHS), CASE_T
    rng = np.random.RandomState(20241121)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    for b in CASE_G_RAISED:
        logits[b, :, 3] += 6.0
    mask = np.zeros((B, T), dtype=np.float32)
    for b, n in enumerate(CASE_LENGTHS):
        mask[b, :n] = 1
    logits *= mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    allowed[3, 1] = 0
    allowed[4, 10:13], allowed[4, 13], allowed[4, 30] = 1, 5, 2
    allowed[5, 20:27] = (8, 8, 1, 8, 8, 1, 1)
    allowed[5, 30], allowed[5, 40] = 6, 7
    allowed[5, 2], allowed[5, 60] = 1, 1
    allowed[6, 5] = 0
    partner = np.full((B, T), -1, dtype=np.int32)
    for b, text in enumerate(case_structures()):
        assert len(text) == CASE_LENGTHS[b]
        partner[b, :len(text)] = parse_structure(text)
    bias = np.zeros((B, T, 4), dtype=np.float32)
    bias[7, :CASE_LENGTHS[7]] = rng.standard_normal((CASE_LENGTHS[7], 4)).astype(np.float32)
    return dict(B=B, logits=logits, mask=mask, allowed=allowed, partner=partner, bias=bias, packed=np.ascontiguousarray(logits[mask != 0]),
                cu=np.concatenate([[0], np.cumsum(CASE_LENGTHS)]).astype(np.int32))


_CASE_REF = {}


def case_ref(name, delta, kind, temperature, S=CASE_S, seed=CASE_SEED):
    """The restatement's draws of the batch under automaton ``name`` (its tables passed in), once per process and never written to."""
    key = (name, float(temperature), S, seed)
    if key not in _CASE_REF:
        h = case_arrays()
        _CASE_REF[key] = design_nested_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, delta, kind, h["allowed"], h["partner"], True, h["bias"])
    return _CASE_REF[key]
