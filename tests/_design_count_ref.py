"""Float64 numpy restatement of the draw ``rnampnn_design_count`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_count_*.py.  Per RNA a ``CountPlan`` holds what does not depend on the sample - the units (single positions, feasible
pairs), their leaf polynomials under the per-position counted sets, the product tree of count polynomials truncated at the cap, the
window's target, ``k_min`` and ``count_miss`` - and draws top down with the hash of ``_design_ref``.  ``lse``, ``Selection`` and
``convolve`` are ``_design_gc_ref``'s.  Besides the ids a draw returns the smallest margin of the selections on its path (see
``_design_gc_ref``).  ``path_logprob`` multiplies the conditionals along the path of a GIVEN sequence (the exactness check against a
brute-force joint)."""
import numpy as np

from _design_ref import COMPAT, u24
import _design_gc_ref as G
from _design_gc_ref import NEG, SALT, Selection, convolve, lse


def bit(m, c):
    return (int(m) >> int(c)) & 1


def mutation_sets(reference):
    """Class ids -> counted sets 15 ^ (1 << id); 0 where the id is outside 0..3."""
    ref = np.asarray(reference).astype(np.int64)
    ok = (ref >= 0) & (ref <= 3)
    return np.where(ok, 15 ^ (1 << np.clip(ref, 0, 3)), 0).astype(np.uint8)


class CountPlan:
    def __init__(self, logits, n, temperature, lo, hi, counted, cap, allowed=None, partner=None, wobble=True, bias=None):
        n = int(n)
        self.n, wob = n, bool(wobble)
        self._sel = {}                                             # the running sums of every selection met so far
        z = np.asarray(logits)[:n].astype(np.float64)
        if bias is not None:
            bias = np.asarray(bias)
            z = z + (bias if bias.ndim == 1 else bias[:n]).astype(np.float64)
        self.z = z = z / float(np.float32(temperature))
        self.counted = cs = np.asarray(counted)[:n].astype(np.int64) & 15
        mask = np.full(n, 15, dtype=np.int64) if allowed is None else (np.asarray(allowed)[:n].astype(np.int64) & 15)
        self.infeasible = int((mask == 0).sum())
        self.mask = mask = np.where(mask == 0, 15, mask)
        mate = np.full(n, -1, dtype=np.int64)
        for t in range(n):
            j = -1 if partner is None else int(partner[t])
            if 0 <= j < n and j != t and int(partner[j]) == t:
                mate[t] = j
        self.kind = np.zeros(n, dtype=np.int64)                    # 0 single, 1 the lower end of a feasible pair, 2 its upper end
        self.cands = [None] * n                                    # per leaf: [(ids, z, what it counts)] of its candidates, in order
        self.mate = np.full(n, -1, dtype=np.int64)                 # the partner of a FEASIBLE pair
        for t in range(n):
            j = int(mate[t])
            if j > t:
                cells = [(a, c) for a in range(4) for c in range(4) if (mask[t] >> a) & 1 and (mask[j] >> c) & 1 and (COMPAT[wob][a] >> c) & 1]
                if cells:
                    self.kind[t], self.kind[j] = 1, 2
                    self.mate[t], self.mate[j] = j, t
                    self.cands[t] = [(cell, z[t, cell[0]] + z[j, cell[1]], bit(cs[t], cell[0]) + bit(cs[j], cell[1])) for cell in cells]
                else:
                    self.infeasible += 2
        for t in range(n):
            if self.kind[t] == 0:
                self.cands[t] = [(c, z[t, c], bit(cs[t], c)) for c in range(4) if (mask[t] >> c) & 1]
        leaf = np.full((n, 3), NEG)
        for t in range(n):
            if self.kind[t] == 2:
                leaf[t, 0] = 0.0
            else:
                for d in range(3):
                    leaf[t, d] = lse(np.array([zz for _, zz, g in self.cands[t] if g == d]))
        fin = np.isfinite(leaf)
        self.min_d = np.where(fin.any(axis=1), fin.argmax(axis=1), 0) if n else np.zeros(0, dtype=np.int64)
        self.k_min = int(self.min_d.sum())
        self.top = top = min(n, max(int(cap), 0))
        # levels[l][i] = the coefficients of node (l, i), degree min(2 * positions covered, n, cap)
        self.levels = [[leaf[t, :min(2, top) + 1] for t in range(n)]]
        while len(self.levels[-1]) > 1:
            prev, l = self.levels[-1], len(self.levels)
            cur = []
            for i in range((len(prev) + 1) // 2):
                deg = min(2 * (min((i + 1) << l, n) - (i << l)), top)
                if 2 * i + 1 < len(prev):
                    cur.append(convolve(prev[2 * i], prev[2 * i + 1], deg))
                else:
                    left = prev[2 * i]
                    cur.append(np.concatenate([left, np.full(max(deg + 1 - len(left), 0), NEG)])[:deg + 1])
            self.levels.append(cur)
        self.root = self.levels[-1][0] if n else np.zeros(1)
        lo = min(max(int(lo), 0), top)
        hi = max(min(max(int(hi), 0), top), lo)
        self.lo, self.hi, self.miss, self.target, self.at_min = lo, hi, 0, None, False
        fin = np.isfinite(self.root)
        if n and not fin[lo:hi + 1].any():
            for d in range(1, top + 1):
                if lo - d >= 0 and fin[lo - d]:
                    self.target, self.miss = lo - d, d
                    break
                if hi + d <= top and fin[hi + d]:
                    self.target, self.miss = hi + d, d
                    break
            if self.target is None:                                # no count of 0 .. min(n, cap) is reachable: every leaf at its minimum
                k = self.k_min
                self.target, self.at_min = k, True
                self.miss = lo - k if k < lo else k - hi if k > hi else 0

    def count(self, seq):
        return int(sum(bit(self.counted[t], seq[t]) for t in range(self.n)))

    def _leaf_set(self, t, d):
        c = [x for x in self.cands[t] if x[2] == d]
        return c if c else self.cands[t]

    def _selection(self, key, terms, leaf=False):
        if key not in self._sel:
            self._sel[key] = Selection(terms(), leaf)
        return self._sel[key]

    def draw(self, seed, s, b, margins=True):
        """-> (ids (n,) int8, the smallest margin on the path; inf with ``margins=False``, which skips that arithmetic)."""
        n = self.n
        seq = np.full(n, -1, dtype=np.int8)
        if n == 0:
            return seq, np.inf
        margin = np.inf
        if self.at_min:
            counts = [int(d) for d in self.min_d]
        else:
            if self.target is not None:
                K = self.target
            else:
                k, margin = self._selection("root", lambda: self.root[self.lo:self.hi + 1]).pick(u24(seed ^ SALT, s, b, 0), margins)
                K = self.lo + k
            counts = [K]
            for l in range(len(self.levels) - 1, 0, -1):
                child, nxt = self.levels[l - 1], []
                for i, k in enumerate(counts):
                    L = child[2 * i]
                    if 2 * i + 1 >= len(child):
                        nxt.append(min(k, len(L) - 1))
                        continue
                    R = child[2 * i + 1]
                    k = min(max(k, 0), len(self.levels[l][i]) - 1)
                    a0, a1 = max(0, k - (len(R) - 1)), min(k, len(L) - 1)

                    def terms():
                        with np.errstate(invalid="ignore"):
                            return L[a0:a1 + 1] + R[k - a0:(k - a1 - 1) if k - a1 - 1 >= 0 else None:-1]
                    a, m = self._selection((l, i, k), terms).pick(u24(seed ^ SALT, s, b, (2 * i + 1) << (l - 1)), margins)
                    margin = min(margin, m)
                    nxt += [a0 + a, k - a0 - a]
                counts = nxt
        for t, d in enumerate(counts):
            if self.kind[t] == 2:
                continue
            c = self._leaf_set(t, min(max(d, 0), 2))
            pick, m = self._selection((0, t, d), lambda: np.array([x[1] for x in c]), leaf=True).pick(u24(seed, s, b, t), margins)
            margin = min(margin, m)
            pick = c[pick][0]
            if self.kind[t] == 1:
                seq[t], seq[self.mate[t]] = pick
            else:
                seq[t] = pick
        return seq, margin

    def path_logprob(self, seq):
        """log of the product of the conditionals the draw multiplies along the path that ends in ``seq`` (-inf when it cannot be drawn)."""
        n = self.n
        unit = np.zeros(n, dtype=np.int64)                         # what a leaf counts
        lp = 0.0
        for t in range(n):
            if self.kind[t] == 2:
                continue
            ident = (int(seq[t]), int(seq[self.mate[t]])) if self.kind[t] == 1 else int(seq[t])
            hit = [x for x in self.cands[t] if x[0] == ident]
            if not hit:
                return NEG
            unit[t] = hit[0][2]
            lp += hit[0][1] - lse(np.array([x[1] for x in self.cands[t] if x[2] == unit[t]]))
        K = int(unit.sum())
        if self.at_min:
            return float(lp) if np.array_equal(unit, self.min_d) else NEG
        if self.target is not None:
            if K != self.target:
                return NEG
        elif not self.lo <= K <= self.hi:
            return NEG
        else:
            lp += self.root[K] - lse(self.root[self.lo:self.hi + 1])
        for l in range(len(self.levels) - 1, 0, -1):
            child = self.levels[l - 1]
            for i in range(len(self.levels[l])):
                if 2 * i + 1 >= len(child):
                    continue
                mid, end = (2 * i + 1) << (l - 1), min((i + 1) << l, n)
                a, r = int(unit[i << l:mid].sum()), int(unit[mid:end].sum())
                lp += child[2 * i][a] + child[2 * i + 1][r] - self.levels[l][i][a + r]
        return float(lp)


def design_count_ref(logits, lengths, temperature, S, seed, counted, lo, hi, cap, allowed=None, partner=None, wobble=True, bias=None):
    """Padded (B,T,4) logits -> (seqs (S,B,T) int8, margin (S,B) f64, infeasible (B,), count_miss (B,), count (S,B), plans)."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    margin = np.full((S, B), np.inf)
    count = np.zeros((S, B), dtype=np.int32)
    bad, miss, plans = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plan = CountPlan(logits[b], lengths[b], temperature, lo[b], hi[b], counted[b], min(int(cap), T), None if allowed is None else allowed[b],
                         None if partner is None else partner[b], wobble, bi)
        plans.append(plan)
        bad[b], miss[b] = plan.infeasible, plan.miss
        for s in range(S):
            seqs[s, b, :plan.n], margin[s, b] = plan.draw(int(seed), s, b)
            count[s, b] = plan.count(seqs[s, b])
    return seqs, margin, bad, miss, count, plans


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# The batch of _design_gc_ref (lengths, logits, masks, pair tables, the malformed table of the 64-mer, T = 300, S = 4, the seed above
# 2^32), with WOBBLE OFF, no bias, and a reference per RNA whose mutation sets are the counted sets.  The reference is random; where the
# table holds a pair (i, j) it is made complementary (ref_j pairs with ref_i), so that the structure alone forces no mutation, except:
#   b  n    the reference                                                                    window (lo, hi)
#   0  0    -                                                                                (0, 0)
#   1  1    random                                                                           (0, 0)      no mutation: the reference itself
#   2  2    A, G under the infeasible pair fixed to A, A: the count is 1 whatever is drawn    (2, 2)      unreachable: count_miss = 1, below
#   3  3    random                                                                           (2, 1)      lo > hi: read as (2, 2)
#   4  63   (0, 62) = G.U - incompatible with wobble off - and (1, 61) = A.A; 5 is fixed to   (0, 3)      k_min = 2 or more of the budget is
#           G, 57 is IUPAC Y; ids -1, 4 and 9 at 30..32 (never count)                                    spent by the structure
#   5  64   complementary over the pseudoknot                                                (-5, 100000) out of range: free up to the cap
#   6  65   random, 7 at 64 (never counts)                                                   (2, 2)      exactly two
#   7  257  complementary over the pairs across the node boundaries                          (0, 257)    free (cap 8: at most 8)
#   8  300  random over the 100-pair hairpin: the structure forces k_min >> 8 mutations       (0, 3)      below k_min: at cap 8 no count of
#                                                                                                        0..8 is reachable (the k_min rule),
#                                                                                                        at cap T the search finds k_min
CASE_LENGTHS, CASE_T, CASE_S, CASE_SEED, CASE_PAIRS = G.CASE_LENGTHS, G.CASE_T, G.CASE_S, G.CASE_SEED, G.CASE_PAIRS
CASE_LO = [0, 0, 2, 2, 0, -5, 2, 0, 0]
CASE_HI = [0, 0, 2, 1, 3, 100000, 2, 257, 3]
CASE_INFEASIBLE = G.CASE_INFEASIBLE
CASE_WOBBLE = False
CASE_CAPS = (8, CASE_T)
COMPLEMENT = (1, 0, 3, 2)                                          # A-U, U-A, C-G, G-C


def case_arrays():
    """``_design_gc_ref.case_arrays()`` plus reference (B,T) int32 (-1 on padding), counted (B,T) uint8, lo, hi."""
    h = dict(G.case_arrays())
    B, T = h["B"], CASE_T
    rng = np.random.RandomState(20241020)
    ref = rng.randint(0, 4, size=(B, T)).astype(np.int32)
    for b, i, j in CASE_PAIRS:
        if b not in (2, 8):
            ref[b, j] = COMPLEMENT[ref[b, i]]
    ref[2, :2] = (0, 3)
    ref[4, 0], ref[4, 62], ref[4, 1], ref[4, 61] = 3, 1, 0, 0
    ref[4, 30:33] = (-1, 4, 9)
    ref[6, 64] = 7
    for b, n in enumerate(CASE_LENGTHS):
        ref[b, n:] = -1
    h.update(reference=ref, counted=mutation_sets(ref), lo=np.array(CASE_LO, dtype=np.int32), hi=np.array(CASE_HI, dtype=np.int32))
    return h


_CASE_REF = {}


def case_ref(temperature, cap, S=CASE_S, seed=CASE_SEED):
    """The restatement's draws of the batch at ``temperature`` and ``cap``, computed once per process and never written to."""
    key = (float(temperature), int(cap), S, seed)
    if key not in _CASE_REF:
        h = case_arrays()
        _CASE_REF[key] = design_count_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, h["counted"], h["lo"], h["hi"], cap, h["allowed"],
                                          h["partner"], CASE_WOBBLE)
    return _CASE_REF[key]
