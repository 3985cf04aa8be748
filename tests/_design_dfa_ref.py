"""Float64 numpy restatement of the draw ``rnampnn_design_dfa`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_dfa_*.py.  Per RNA a ``DfaPlan`` holds what does not depend on the sample - z, the masks, the table l_t(a) of log
partition sums over (position, automaton state) that ENDS in the acceptance set, ``dfa_miss`` - and walks forward per sample with the
hash of ``_design_ref``; ``lse`` and ``Selection`` are ``_design_gc_ref``'s.  Besides the ids a draw returns the smallest margin of the
selections on its path (see ``_design_gc_ref``).  ``path_logprob`` multiplies the conditionals along the path of a GIVEN sequence (the
exactness check against a brute-force joint).  The automaton's tables (``delta``, ``kind``: bit 0 dead, bit 1 accepting) are an INPUT
here, as they are for the kernel; ``contains_all`` / ``naive_hits`` compare substrings and know no automaton, so they check both."""
import numpy as np

from _design_ref import u24
from _design_gc_ref import NEG, Selection, lse
from _design_avoid_ref import expand, naive_hits

DEAD, ACCEPTING = 1, 2


def required_sets(require):
    """Motif strings -> one set of class-id tuples per motif (its expansions), by plain enumeration."""
    return [expand([m]) for m in require]


def contains_all(seq, groups):
    """Does ``seq`` (class ids; it ends at the first id outside 0..3) hold, for every group, at least one of its words as a substring?"""
    seq = [int(v) for v in seq]
    n = next((i for i, v in enumerate(seq) if not 0 <= v <= 3), len(seq))
    seq = tuple(seq[:n])
    return all(any(seq[i:i + len(w)] == w for w in g for i in range(n - len(w) + 1)) for g in groups)


def follow(seq, delta, kind):
    """-> (dead states entered, 1 iff the end state is live and accepting), following ``delta`` from state 0 as the entry documents."""
    delta = np.asarray(delta).astype(np.int64).reshape(-1, 4)
    kind = np.asarray(kind).astype(np.int64)
    a, hits = 0, 0
    for v in seq:
        v = int(v)
        if not 0 <= v <= 3:
            break
        nxt = int(delta[a, v])
        out = nxt >= len(kind)
        hits += int(out or bool(kind[nxt] & DEAD))
        a = 0 if out else nxt
    return hits, int((kind[a] & 3) == ACCEPTING)


class DfaPlan:
    def __init__(self, logits, n, temperature, delta, kind, allowed=None, bias=None):
        n = int(n)
        self.n = n
        self.delta = delta = np.asarray(delta).astype(np.int64).reshape(-1, 4)
        self.kind = kind = np.asarray(kind).astype(np.int64)
        self.A = A = delta.shape[0]
        self.dead = dead = (kind & DEAD) != 0
        self._sel = {}
        z = np.asarray(logits)[:n].astype(np.float64)
        if bias is not None:
            bias = np.asarray(bias)
            z = z + (bias if bias.ndim == 1 else bias[:n]).astype(np.float64)
        self.z = z = z / float(np.float32(temperature))
        mask = np.full(n, 15, dtype=np.int64) if allowed is None else (np.asarray(allowed)[:n].astype(np.int64) & 15)
        self.infeasible = int((mask == 0).sum())
        self.mask = mask = np.where(mask == 0, 15, mask)
        # l[t, a]: -inf for a dead state; l[n, a] = 0 for a live ACCEPTING one, -inf for every other
        self.l = l = np.full((n + 1, A), NEG)
        l[n, (~dead) & ((kind & ACCEPTING) != 0)] = 0.0
        inside = delta < A
        target = np.where(inside, delta, 0)
        self.live_cell = live_cell = inside & ~dead[target]         # (A,4): delta(a,c) is a live state
        for t in range(n - 1, -1, -1):
            has = ((mask[t] >> np.arange(4)) & 1).astype(bool)
            with np.errstate(invalid="ignore"):
                terms = np.where(live_cell & has[None, :], z[t][None, :] + l[t + 1][target], NEG)
            l[t] = np.where(dead, NEG, lse(terms, axis=1))
        self.miss = int(not l[0, 0] > NEG)

    def _cells(self, t, a):
        """The classes the draw of position t in state a selects among, and their log-weights."""
        if self.miss:
            cs = [c for c in range(4) if (self.mask[t] >> c) & 1]
            return cs, np.array([self.z[t, c] for c in cs])
        cs = [c for c in range(4) if (self.mask[t] >> c) & 1 and self.live_cell[a, c] and self.l[t + 1, self.delta[a, c]] > NEG]
        return cs, np.array([self.z[t, c] + self.l[t + 1, self.delta[a, c]] for c in cs])

    def draw(self, seed, s, b, margins=True):
        """-> (ids (n,) int8, the smallest margin on the path)."""
        seq = np.full(self.n, -1, dtype=np.int8)
        margin, a = np.inf, 0
        for t in range(self.n):
            key = (t, 0 if self.miss else a)
            if key not in self._sel:
                cs, terms = self._cells(t, a)
                self._sel[key] = (cs, Selection(terms, leaf=True))
            cs, sel = self._sel[key]
            k, m = sel.pick(u24(seed, s, b, t), margins)
            margin = min(margin, m)
            seq[t] = cs[k]
            nxt = int(self.delta[a, cs[k]])
            a = 0 if nxt >= self.A else nxt
        return seq, margin

    def path_logprob(self, seq):
        """log of the product of the conditionals the draw multiplies along the path that ends in ``seq`` (-inf when it cannot be drawn)."""
        lp, a = 0.0, 0
        for t in range(self.n):
            cs, terms = self._cells(t, a)
            if int(seq[t]) not in cs:
                return NEG
            lp += terms[cs.index(int(seq[t]))] - lse(terms)
            nxt = int(self.delta[a, int(seq[t])])
            a = 0 if nxt >= self.A else nxt
        return float(lp)


def design_dfa_ref(logits, lengths, temperature, S, seed, delta, kind, allowed=None, bias=None):
    """Padded (B,T,4) logits -> dict: seqs (S,B,T) int8, margin (S,B) f64, infeasible (B,), dfa_miss (B,), hits (S,B), accepted (S,B), plans."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    margin = np.full((S, B), np.inf)
    hits, accepted = np.zeros((S, B), dtype=np.int32), np.zeros((S, B), dtype=np.int32)
    bad, miss, plans = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plan = DfaPlan(logits[b], lengths[b], temperature, delta, kind, None if allowed is None else allowed[b], bi)
        plans.append(plan)
        bad[b], miss[b] = plan.infeasible, plan.miss
        for s in range(S):
            seqs[s, b, :plan.n], margin[s, b] = plan.draw(int(seed), s, b)
            hits[s, b], accepted[s, b] = follow(seqs[s, b], delta, kind)
    return dict(seqs=seqs, margin=margin, infeasible=bad, dfa_miss=miss, hits=hits, accepted=accepted, plans=plans)


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# The siblings' lengths, T = 300, S = 4, logits 3 * randn, a seed above 2^32.  No base pairs (the entry refuses them).
#   b  n    what it is there for
#   0  0    the empty RNA: state 0 does not accept, so dfa_miss = 1 and nothing is drawn
#   1  1    one position: shorter than every required motif, dfa_miss = 1, rnampnn_design's draws
#   2  2    the same
#   3  3    the same, and allowed[1] = 0: drawn as free, counts 1 in `infeasible`
#   4  63   fixed to A everywhere but 10..14, which omit G: every required motif below holds a G, so it is impossible; dfa_miss = 1, and
#           under max_run = 3 the fixed As enter dead states: hits > 0, accepted = 0
#   5  64   G + 6; 20..26 fixed to GGAGGAA, which spells GGAGG and GNRA (GGAA); 30 is IUPAC Y, 40 omits G
#   6  65   20..22 fixed to GGG with 19 and 23 free (max_run = 3 forces both neighbours off G); allowed[5] = 0 counts 1 in `infeasible`
#   7  257  a per-position bias (the other rows' bias is zero), G + 6
#   8  300  G + 6 over the full extent
CASE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 257, 300]
CASE_T, CASE_S = 300, 4
CASE_SEED = 0x0123_4567_89AB_CDE9                                  # above 2^32: the 64-bit seed arithmetic is exercised
CASE_INFEASIBLE = [0, 0, 0, 1, 0, 0, 1, 0, 0]
CASE_MISS = [1, 1, 1, 1, 1, 0, 0, 0, 0]
CASE_G_RAISED = (5, 7, 8)
# The automata: (require, avoid, max_run).  One required 5-mer (11 states); an IUPAC tetraloop with no run longer than 3 (61 states, 53
# live); two required 5-mers with no run longer than 3: 89 states, 73 live - past one wave's lanes and past rnampnn_design_avoid's 64.
CASE_AUTOMATA = {"ggagg": (("GGAGG",), (), None), "gnra_run3": (("GNRA",), (), 3), "two_run3": (("GGAGG", "CUUCG"), (), 3)}


def case_arrays():
    """-> dict of numpy arrays: logits (B,T,4) f32 (zero on padding), mask, allowed, bias (B,T,4), packed, cu."""
    B, T = len(CASE_LENGTHS), CASE_T
    rng = np.random.RandomState(20241103)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    for b in CASE_G_RAISED:
        logits[b, :, 3] += 6.0
    mask = np.zeros((B, T), dtype=np.float32)
    for b, n in enumerate(CASE_LENGTHS):
        mask[b, :n] = 1
    logits *= mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    allowed[3, 1] = 0
    allowed[4, :CASE_LENGTHS[4]] = 1
    allowed[4, 10:15] = 7
    allowed[5, 20:27] = (8, 8, 1, 8, 8, 1, 1)
    allowed[5, 30], allowed[5, 40] = 6, 7
    allowed[6, 20:23] = 8
    allowed[6, 5] = 0
    bias = np.zeros((B, T, 4), dtype=np.float32)
    bias[7, :CASE_LENGTHS[7]] = rng.standard_normal((CASE_LENGTHS[7], 4)).astype(np.float32)
    return dict(B=B, logits=logits, mask=mask, allowed=allowed, bias=bias, packed=np.ascontiguousarray(logits[mask != 0]),
                cu=np.concatenate([[0], np.cumsum(CASE_LENGTHS)]).astype(np.int32))


_CASE_REF = {}


def case_ref(name, delta, kind, temperature, S=CASE_S, seed=CASE_SEED):
    """The restatement's draws of the batch under automaton ``name`` (its tables passed in), once per process and never written to."""
    key = (name, float(temperature), S, seed)
    if key not in _CASE_REF:
        h = case_arrays()
        _CASE_REF[key] = design_dfa_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, delta, kind, h["allowed"], h["bias"])
    return _CASE_REF[key]
