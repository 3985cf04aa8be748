"""Float64 numpy restatement of the draw ``rnampnn_design_gc`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_gc_*.py.  Per RNA a ``GcPlan`` holds what does not depend on the sample - the units (single positions, feasible pairs),
their leaf polynomials, the product tree of count polynomials in the log domain, the window's target and ``gc_miss`` - and draws top down
with the hash of ``_design_ref``.  Besides the ids a draw returns the smallest margin of the selections on its path (how far the uniform
lies from the nearest cumulative boundary, relative to the total): the device differs from this file by last-bit exp / log and by the
summation order inside a node, so a draw whose path passes closer than that to a boundary may legitimately land on the other side.
``maxplus=True`` builds the same tree over (max, +): its root holds the constrained optimum per count (the cold limit of the draw).
``path_logprob`` multiplies the conditionals along the path of a GIVEN sequence (the exactness check against a brute-force joint)."""
import numpy as np

from _design_ref import COMPAT, u24

SALT = 0xA0761D6478BD642F
GC = (0, 0, 1, 1)                      # AUCG = 0..3
NEG = -np.inf


def lse(x, axis=None, maxplus=False):
    """max + log(sum exp(x - max)), NaN ignored in the maximum; -inf where the maximum is not above -inf."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return NEG if axis is None else np.full(np.delete(x.shape, axis), NEG)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = np.fmax.reduce(x, axis=axis, initial=NEG)
        if maxplus:
            return mx
        ok = mx > NEG
        safe = np.where(ok, mx, 0.0)
        out = safe + np.log(np.sum(np.exp(x - (safe if axis is None else np.expand_dims(safe, axis))), axis=axis))
        return np.where(ok, out, NEG)[()]


class Selection:
    """The family's rule over candidates in order with log-weights ``terms``: weights exp(terms - max), the first candidate whose running
    sum exceeds u24 * 2^-24 * total; else the last candidate with a finite log-weight (``leaf=True``: the last candidate, the rule of a
    position or a pair in rnampnn_design); else the first.  The running sums are formed once; ``pick`` -> (index, margin)."""

    def __init__(self, terms, leaf=False):
        terms = np.asarray(terms, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            self.cum = np.cumsum(np.exp(terms - np.fmax.reduce(terms, initial=NEG)))
        self.tot = float(self.cum[-1])
        fin = np.nonzero(np.isfinite(terms))[0]
        self.fallback = len(terms) - 1 if leaf else (int(fin[-1]) if fin.size else 0)

    def pick(self, u_bits, want_margin=True):
        u = u_bits * 2.0 ** -24 * self.tot
        if self.tot != self.tot:
            return self.fallback, 0.0
        k = int(np.searchsorted(self.cum, u, side="right"))        # the first index with cum > u
        if k >= len(self.cum):
            k = self.fallback
        if len(self.cum) == 1 or not want_margin:
            return k, np.inf
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = float(np.min(np.abs(self.cum - u)) / self.tot)
        return k, (margin if margin == margin else 0.0)


def convolve(L, R, deg, maxplus=False):
    """c(k) = LSE over a = max(0, k - deg_R) .. min(k, deg_L) of L(a) + R(k - a), k = 0..deg."""
    dL, dR = len(L) - 1, len(R) - 1
    k = np.arange(deg + 1)[None, :]
    a = np.arange(dL + 1)[:, None]
    idx = k - a
    ok = (idx >= 0) & (idx <= dR)
    with np.errstate(invalid="ignore"):
        terms = np.where(ok, L[:, None] + R[np.clip(idx, 0, dR)], NEG)
    return lse(terms, axis=0, maxplus=maxplus)


class GcPlan:
    def __init__(self, logits, n, temperature, lo, hi, allowed=None, partner=None, wobble=True, bias=None, maxplus=False):
        n = int(n)
        self.n, self.maxplus, wob = n, maxplus, bool(wobble)
        self._sel = {}                                             # the running sums of every selection met so far
        z = np.asarray(logits)[:n].astype(np.float64)
        if bias is not None:
            bias = np.asarray(bias)
            z = z + (bias if bias.ndim == 1 else bias[:n]).astype(np.float64)
        self.z = z = z / float(np.float32(temperature))
        mask = np.full(n, 15, dtype=np.int64) if allowed is None else (np.asarray(allowed)[:n].astype(np.int64) & 15)
        self.infeasible = int((mask == 0).sum())
        self.mask = mask = np.where(mask == 0, 15, mask)
        mate = np.full(n, -1, dtype=np.int64)
        for t in range(n):
            j = -1 if partner is None else int(partner[t])
            if 0 <= j < n and j != t and int(partner[j]) == t:
                mate[t] = j
        self.kind = np.zeros(n, dtype=np.int64)                    # 0 single, 1 the lower end of a feasible pair, 2 its upper end
        self.cands = [None] * n                                    # per leaf: [(ids, z, G+C)] of its candidates, in order
        self.mate = np.full(n, -1, dtype=np.int64)                 # the partner of a FEASIBLE pair
        for t in range(n):
            j = int(mate[t])
            if j > t:
                cells = [(a, c) for a in range(4) for c in range(4) if (mask[t] >> a) & 1 and (mask[j] >> c) & 1 and (COMPAT[wob][a] >> c) & 1]
                if cells:
                    self.kind[t], self.kind[j] = 1, 2
                    self.mate[t], self.mate[j] = j, t
                    self.cands[t] = [(cell, z[t, cell[0]] + z[j, cell[1]], GC[cell[0]] + GC[cell[1]]) for cell in cells]
                else:
                    self.infeasible += 2
        for t in range(n):
            if self.kind[t] == 0:
                self.cands[t] = [(c, z[t, c], GC[c]) for c in range(4) if (mask[t] >> c) & 1]
        leaf = np.full((n, 3), NEG)
        for t in range(n):
            if self.kind[t] == 2:
                leaf[t, 0] = 0.0
            else:
                for d in range(3):
                    leaf[t, d] = lse(np.array([zz for _, zz, g in self.cands[t] if g == d]), maxplus=maxplus)
        # levels[l][i] = the coefficients of node (l, i), degree min(2 * positions covered, n)
        self.levels = [[leaf[t, :min(2, n) + 1] for t in range(n)]]
        while len(self.levels[-1]) > 1:
            prev, l = self.levels[-1], len(self.levels)
            cur = []
            for i in range((len(prev) + 1) // 2):
                deg = min(2 * (min((i + 1) << l, n) - (i << l)), n)
                if 2 * i + 1 < len(prev):
                    cur.append(convolve(prev[2 * i], prev[2 * i + 1], deg, maxplus))
                else:
                    left = prev[2 * i]
                    cur.append(np.concatenate([left, np.full(max(deg + 1 - len(left), 0), NEG)])[:deg + 1])
            self.levels.append(cur)
        self.root = self.levels[-1][0] if n else np.zeros(1)
        lo = min(max(int(lo), 0), n)
        hi = max(min(max(int(hi), 0), n), lo)
        self.lo, self.hi, self.miss, self.target = lo, hi, 0, None
        fin = np.isfinite(self.root)
        if n and not fin[lo:hi + 1].any():
            self.target = lo
            for d in range(1, n + 1):
                if lo - d >= 0 and fin[lo - d]:
                    self.target, self.miss = lo - d, d
                    break
                if hi + d <= n and fin[hi + d]:
                    self.target, self.miss = hi + d, d
                    break

    def optimum(self):
        """maxplus only: the largest sum of z over the sequences the constraints and the window (or its target) admit."""
        return float(self.root[self.target]) if self.target is not None else float(np.max(self.root[self.lo:self.hi + 1]))

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
        unit = np.zeros(n, dtype=np.int64)                         # the G+C a leaf carries
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


def design_gc_ref(logits, lengths, temperature, S, seed, gc_lo, gc_hi, allowed=None, partner=None, wobble=True, bias=None, rows=None):
    """Padded (B,T,4) logits -> (seqs (S,B,T) int8, margin (S,B) f64, infeasible (B,), gc_miss (B,), plans)."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    margin = np.full((S, B), np.inf)
    bad, miss, plans = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plan = GcPlan(logits[b], lengths[b], temperature, gc_lo[b], gc_hi[b], None if allowed is None else allowed[b],
                      None if partner is None else partner[b], wobble, bi)
        plans.append(plan)
        bad[b], miss[b] = plan.infeasible, plan.miss
        for s in range(S):
            if rows is None or b in rows:
                seqs[s, b, :plan.n], margin[s, b] = plan.draw(int(seed), s, b)
    return seqs, margin, bad, miss, plans


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# One padded batch under the global bias -4 on C and G (every window below sits in the tail of the biased distribution), T = 300, S = 4.
#   b  n    constraints                                                                     window (lo, hi)
#   0  0    -                                                                               (0, 0)
#   1  1    free                                                                            (1, 1)      a single count
#   2  2    both fixed to A and paired: an infeasible pair (counts 2)                       (1, 2)      unreachable: gc_miss = 1
#   3  3    allowed[1] = 0: drawn as free, counts 1                                         (2, 1)      lo > hi: read as (2, 2)
#   4  63   a hairpin (i, 62 - i), i < 25; 5 is fixed to G, 57 is IUPAC Y                    (31, 31)    a single count
#   5  64   a pseudoknot (i, 30 - i) and (10 + i, 50 - i), i < 5; a malformed table          (-5, 100000) out of range: free
#           (20 -> 21 one-sided, 22 -> 22, 23 -> 1000, 24 -> -7, 25 -> 70 in the padding, which points back)
#   6  65   free                                                                            (52, 65)    >= 80 % G+C: the far tail
#   7  257  a pair across a node boundary of every level 1..9: (10,11) (13,14) (19,20)       (100, 140)
#           (23,24) (47,48) (95,96) (63,64) (127,128) (255,256), the last one and (3, 200)
#           across the 256-stride
#   8  300  a long hairpin (i, 299 - i), i < 100, whose ends lie in different 256-strides    (0, 300)    the free window
CASE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 257, 300]
CASE_T, CASE_S = 300, 4
CASE_SEED = 0x0123_4567_89AB_CDE7                                  # above 2^32: the 64-bit seed arithmetic and the salt's XOR are exercised
CASE_LO = [0, 1, 1, 2, 31, -5, 52, 100, 0]
CASE_HI = [0, 1, 2, 1, 31, 100000, 65, 140, 300]
CASE_MISS = [0, 0, 1, 0, 0, 0, 0, 0, 0]
CASE_INFEASIBLE = [0, 0, 2, 1, 0, 0, 0, 0, 0]
CASE_PAIRS = ([(2, 0, 1)] + [(4, i, 62 - i) for i in range(25)] + [(5, i, 30 - i) for i in range(5)] + [(5, 10 + i, 50 - i) for i in range(5)]
              + [(7, a, a + 1) for a in (10, 13, 19, 23, 47, 95, 63, 127, 255)] + [(7, 3, 200)] + [(8, i, 299 - i) for i in range(100)])
CASE_BIAS = np.array([0.0, 0.0, -4.0, -4.0], dtype=np.float32)


def case_arrays():
    """-> dict of numpy arrays: logits (B,T,4) f32 = 3 * randn (zero on padding), mask, allowed, partner, packed, cu, lo, hi."""
    B, T = len(CASE_LENGTHS), CASE_T
    rng = np.random.RandomState(20241019)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    mask = np.zeros((B, T), dtype=np.float32)
    for b, n in enumerate(CASE_LENGTHS):
        mask[b, :n] = 1
    logits *= mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    partner = np.full((B, T), -1, dtype=np.int32)
    for b, i, j in CASE_PAIRS:
        partner[b, i], partner[b, j] = j, i
    allowed[2, 0] = allowed[2, 1] = 1
    allowed[3, 1] = 0
    allowed[4, 5], allowed[4, 57] = 8, 6
    partner[5, 20] = 21; partner[5, 22] = 22; partner[5, 23] = 1000; partner[5, 24] = -7; partner[5, 25] = 70; partner[5, 70] = 25
    return dict(B=B, logits=logits, mask=mask, allowed=allowed, partner=partner, packed=np.ascontiguousarray(logits[mask != 0]),
                cu=np.concatenate([[0], np.cumsum(CASE_LENGTHS)]).astype(np.int32), lo=np.array(CASE_LO, dtype=np.int32),
                hi=np.array(CASE_HI, dtype=np.int32))


_CASE_REF = {}


def case_ref(temperature, S=CASE_S, seed=CASE_SEED):
    """The restatement's draws of the batch at ``temperature``, computed once per process and never written to."""
    key = (float(temperature), S, seed)
    if key not in _CASE_REF:
        h = case_arrays()
        _CASE_REF[key] = design_gc_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, h["lo"], h["hi"], h["allowed"], h["partner"], True,
                                       CASE_BIAS)
    return _CASE_REF[key]
