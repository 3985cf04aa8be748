"""Float64 numpy restatement of the draw ``rnampnn_design_avoid`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_avoid_*.py.  Per RNA an ``AvoidPlan`` holds what does not depend on the sample - z, the masks, the table l_t(a) of log
partition sums over (position, live automaton state), ``avoid_miss`` - and walks forward per sample with the hash of ``_design_ref``;
``lse`` and ``Selection`` are ``_design_gc_ref``'s.  Besides the ids a draw returns the smallest margin of the selections on its path (see
``_design_gc_ref``).  ``path_logprob`` multiplies the conditionals along the path of a GIVEN sequence (the exactness check against a
brute-force joint).  The automaton's tables are an INPUT here, as they are for the kernel; ``naive_hits`` counts motif ends by comparing
substrings and knows no automaton, so it checks both."""
import numpy as np

from _design_ref import u24
from _design_gc_ref import NEG, Selection, lse

LETTERS = "AUCG"
CODES = {"A": "A", "U": "U", "T": "U", "C": "C", "G": "G", "R": "AG", "Y": "CU", "S": "CG", "W": "AU", "K": "GU", "M": "AC", "B": "CGU",
         "D": "AGU", "H": "ACU", "V": "ACG", "N": "AUCG"}


def expand(motifs, max_run=None):
    """Motif strings (T = U, IUPAC codes) and ``max_run`` -> the set of class-id tuples, by plain enumeration."""
    words = set()
    for m in motifs:
        cur = [()]
        for ch in m.upper():
            cur = [w + (LETTERS.index(x),) for w in cur for x in CODES[ch]]
        words.update(cur)
    if max_run is not None:
        words.update((c,) * (max_run + 1) for c in range(4))
    return words


def naive_hits(seq, words):
    """The positions t of ``seq`` (class ids; it ends at the first id outside 0..3) at which some word ends: a substring comparison."""
    seq = [int(v) for v in seq]
    n = next((i for i, v in enumerate(seq) if not 0 <= v <= 3), len(seq))
    return sum(any(len(w) <= t + 1 and tuple(seq[t + 1 - len(w):t + 1]) == w for w in words) for t in range(n))


class AvoidPlan:
    def __init__(self, logits, n, temperature, delta, terminal, allowed=None, bias=None):
        n = int(n)
        self.n = n
        self.delta = delta = np.asarray(delta).astype(np.int64).reshape(-1, 4)
        self.A = A = delta.shape[0]
        self.dead = dead = [bool((int(terminal) >> a) & 1) for a in range(A)]
        self._sel = {}
        z = np.asarray(logits)[:n].astype(np.float64)
        if bias is not None:
            bias = np.asarray(bias)
            z = z + (bias if bias.ndim == 1 else bias[:n]).astype(np.float64)
        self.z = z = z / float(np.float32(temperature))
        mask = np.full(n, 15, dtype=np.int64) if allowed is None else (np.asarray(allowed)[:n].astype(np.int64) & 15)
        self.infeasible = int((mask == 0).sum())
        self.mask = mask = np.where(mask == 0, 15, mask)
        # l[t, a]: -inf for a dead state; l[n, a] = 0 for a live one
        self.l = l = np.full((n + 1, A), NEG)
        l[n, [a for a in range(A) if not dead[a]]] = 0.0
        for t in range(n - 1, -1, -1):
            for a in range(A):
                if not dead[a]:
                    l[t, a] = lse(np.array([z[t, c] + l[t + 1, delta[a, c]] for c in range(4) if self._live_cell(t, a, c)]))
        self.miss = int(not l[0, 0] > NEG)

    def _live_cell(self, t, a, c):
        nxt = self.delta[a, c]
        return bool((self.mask[t] >> c) & 1) and nxt < self.A and not self.dead[nxt]

    def _cells(self, t, a):
        """The classes the draw of position t in state a selects among, and their log-weights."""
        if self.miss:
            cs = [c for c in range(4) if (self.mask[t] >> c) & 1]
            return cs, np.array([self.z[t, c] for c in cs])
        cs = [c for c in range(4) if self._live_cell(t, a, c) and self.l[t + 1, self.delta[a, c]] > NEG]
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
            a = int(self.delta[a, cs[k]])
        return seq, margin

    def path_logprob(self, seq):
        """log of the product of the conditionals the draw multiplies along the path that ends in ``seq`` (-inf when it cannot be drawn)."""
        lp, a = 0.0, 0
        for t in range(self.n):
            cs, terms = self._cells(t, a)
            if int(seq[t]) not in cs:
                return NEG
            lp += terms[cs.index(int(seq[t]))] - lse(terms)
            a = int(self.delta[a, int(seq[t])])
        return float(lp)


def design_avoid_ref(logits, lengths, temperature, S, seed, delta, terminal, words, allowed=None, bias=None):
    """Padded (B,T,4) logits -> (seqs (S,B,T) int8, margin (S,B) f64, infeasible (B,), avoid_miss (B,), hits (S,B), plans)."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    margin = np.full((S, B), np.inf)
    hits = np.zeros((S, B), dtype=np.int32)
    bad, miss, plans = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plan = AvoidPlan(logits[b], lengths[b], temperature, delta, terminal, None if allowed is None else allowed[b], bi)
        plans.append(plan)
        bad[b], miss[b] = plan.infeasible, plan.miss
        for s in range(S):
            seqs[s, b, :plan.n], margin[s, b] = plan.draw(int(seed), s, b)
            hits[s, b] = naive_hits(seqs[s, b], words)
    return seqs, margin, bad, miss, hits, plans


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# The siblings' lengths, T = 300, S = 4, logits 3 * randn, a seed above 2^32.  No base pairs (the entry refuses them).
#   b  n    what it is there for
#   0  0    the empty RNA: feasible, nothing drawn
#   1  1    one position
#   2  2    shorter than every motif
#   3  3    allowed[1] = 0: drawn as free, counts 1 in `infeasible`
#   4  63   10..14 fixed to GGGGA, which ends a motif of every automaton below: infeasible, avoid_miss = 1, hits > 0, rnampnn_design's draws
#   5  64   G + 6: free draws would hold GGGG nearly everywhere; 30 is IUPAC Y, 40 omits G
#   6  65   20..22 fixed to GGG with 19 and 23 free: under max_run = 3 both neighbours are forced off G
#   7  257  a per-position bias (the other rows' bias is zero), G + 6
#   8  300  G + 6 over the full extent
CASE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 257, 300]
CASE_T, CASE_S = 300, 4
CASE_SEED = 0x0123_4567_89AB_CDE9                                  # above 2^32: the 64-bit seed arithmetic is exercised
CASE_INFEASIBLE = [0, 0, 0, 1, 0, 0, 0, 0, 0]
CASE_MISS = [0, 0, 0, 0, 1, 0, 0, 0, 0]
CASE_G_RAISED = (5, 7, 8)
# The automata: no run longer than 3 (17 states, 13 live); motifs that overlap, with one a suffix of another (UGGA / GGA share their end,
# GGA -> GAC -> ACGU chain through the suffix links); and a set of 7 motifs whose automaton has exactly 64 states, 57 of them live.
CASE_AUTOMATA = {"max_run3": ((), 3), "overlap": (("UGGA", "GGA", "GAC", "ACGU"), None),
                 "states64": (("GGGG", "GAAUUCAAGC", "CUGCAGUCGA", "AAGCUUGCAU", "UCUAGAGGCC", "CCCGGGAUAU", "AUCGAUCGGUAC"), None)}


def case_arrays():
    """-> dict of numpy arrays: logits (B,T,4) f32 (zero on padding), mask, allowed, bias (B,T,4), packed, cu."""
    B, T = len(CASE_LENGTHS), CASE_T
    rng = np.random.RandomState(20241021)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    for b in CASE_G_RAISED:
        logits[b, :, 3] += 6.0
    mask = np.zeros((B, T), dtype=np.float32)
    for b, n in enumerate(CASE_LENGTHS):
        mask[b, :n] = 1
    logits *= mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    allowed[3, 1] = 0
    allowed[4, 10:15] = (8, 8, 8, 8, 1)
    allowed[5, 30], allowed[5, 40] = 6, 7
    allowed[6, 20:23] = 8
    bias = np.zeros((B, T, 4), dtype=np.float32)
    bias[7, :CASE_LENGTHS[7]] = rng.standard_normal((CASE_LENGTHS[7], 4)).astype(np.float32)
    return dict(B=B, logits=logits, mask=mask, allowed=allowed, bias=bias, packed=np.ascontiguousarray(logits[mask != 0]),
                cu=np.concatenate([[0], np.cumsum(CASE_LENGTHS)]).astype(np.int32))


_CASE_REF = {}


def case_ref(name, delta, terminal, temperature, S=CASE_S, seed=CASE_SEED):
    """The restatement's draws of the batch under automaton ``name`` (its tables passed in), once per process and never written to."""
    key = (name, float(temperature), S, seed)
    if key not in _CASE_REF:
        h = case_arrays()
        motifs, max_run = CASE_AUTOMATA[name]
        _CASE_REF[key] = design_avoid_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, delta, terminal, expand(motifs, max_run), h["allowed"],
                                          h["bias"])
    return _CASE_REF[key]
