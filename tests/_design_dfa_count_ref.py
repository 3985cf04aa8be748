"""Float64 numpy restatement of the draw ``rnampnn_design_dfa_count`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_dfa_count_*.py.  Per RNA a ``DfaCountPlan`` holds what does not depend on the sample - z, the masks, the counted sets,
the table l_t(a, k) of log partition sums over (position, automaton state, count still to come), formed vectorised over (state, count),
the window, the target, both miss flags and ``log_z`` - and walks forward per sample with (state, remaining count) and the hash of
``_design_ref``; ``lse`` and ``Selection`` are ``_design_gc_ref``'s, ``follow`` is ``_design_dfa_ref``'s.  Besides the ids a draw returns
the smallest margin of the selections on its path, the total's included (see ``_design_gc_ref``).  ``path_logprob`` multiplies the
conditionals along the path of a GIVEN sequence (the exactness check against a brute-force joint).  The automaton's tables are an INPUT
here, as they are for the kernel."""
import numpy as np

from _design_ref import u24
from _design_gc_ref import NEG, SALT, Selection, lse
from _design_count_ref import bit
from _design_dfa_ref import ACCEPTING, DEAD, follow


def gc_window(lengths, lo=0.45, hi=0.60):
    """The window of ``rnampnn.model.decode.gc_counts`` in absolute counts: ceil(f_lo n - 1e-6), floor(f_hi n + 1e-6)."""
    n = np.asarray(lengths, dtype=np.float64)
    return np.ceil(lo * n - 1e-6).astype(np.int32), np.floor(hi * n + 1e-6).astype(np.int32)


def recount(seq, counted):
    """The sum over the ids of ``seq`` (it ends at the first id outside 0..3) of bit(counted_t, id_t)."""
    total = 0
    for t, v in enumerate(seq):
        if not 0 <= int(v) <= 3:
            break
        total += bit(int(counted[t]), int(v))
    return total


class DfaCountPlan:
    def __init__(self, logits, n, temperature, delta, kind, counted, lo, hi, cap, allowed=None, bias=None):
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
        self.counted = cs = np.asarray(counted)[:n].astype(np.int64) & 15
        self.K = K = min(max(int(cap), 0), n)
        # l[t, a, k]: -inf for a dead state; l[n, a, 0] = 0 for a live ACCEPTING state, -inf for every other entry
        self.l = l = np.full((n + 1, A, K + 1), NEG)
        l[n, (~dead) & ((kind & ACCEPTING) != 0), 0] = 0.0
        inside = delta < A
        target = np.where(inside, delta, 0)
        self.live_cell = live_cell = inside & ~dead[target]         # (A,4): delta(a,c) is a live state
        for t in range(n - 1, -1, -1):
            terms = np.full((A, K + 1, 4), NEG)
            for c in range(4):
                if not (mask[t] >> c) & 1:
                    continue
                d = bit(int(cs[t]), c)
                nxt = l[t + 1][target[:, c]]                         # (A, K+1): l_{t+1}(delta(a,c), .)
                with np.errstate(invalid="ignore"):
                    terms[:, d:, c] = np.where(live_cell[:, c][:, None], z[t, c] + nxt[:, :K + 1 - d], NEG)
            l[t] = np.where(dead[:, None], NEG, lse(terms, axis=2))
        self.root = root = l[0, 0] if n > 0 else np.array([0.0 if (kind[0] & 3) == ACCEPTING else NEG])
        self.lo = lo = min(max(int(lo), 0), K)
        self.hi = hi = max(min(max(int(hi), 0), K), lo)
        finite = np.isfinite(root)
        self.any = bool(finite[lo:hi + 1].any())
        self.target, self.count_miss, self.dfa_miss = lo, 0, 0
        if self.any:
            self.log_z = float(lse(root[lo:hi + 1]))
        elif finite.any():                                          # the nearest reachable count, the lower one on a tie
            for d in range(1, K + 1):
                if lo - d >= 0 and finite[lo - d]:
                    self.target, self.count_miss = lo - d, d
                    break
                if hi + d <= K and finite[hi + d]:
                    self.target, self.count_miss = hi + d, d
                    break
            self.log_z = float(root[self.target])
        else:
            self.dfa_miss, self.log_z = 1, NEG

    def _cells(self, t, a, r):
        """The classes the draw of position t in state a with r still to count selects among, and their log-weights."""
        if self.dfa_miss:
            cs = [c for c in range(4) if (self.mask[t] >> c) & 1]
            return cs, np.array([self.z[t, c] for c in cs])
        cs, terms = [], []
        for c in range(4):
            k = r - bit(int(self.counted[t]), c)
            if (self.mask[t] >> c) & 1 and self.live_cell[a, c] and k >= 0 and self.l[t + 1, self.delta[a, c], k] > NEG:
                cs.append(c)
                terms.append(self.z[t, c] + self.l[t + 1, self.delta[a, c], k])
        return cs, np.array(terms)

    def _step(self, t, a, r):
        key = (t, 0, 0) if self.dfa_miss else (t, a, r)
        if key not in self._sel:
            cs, terms = self._cells(t, a, r)
            self._sel[key] = (cs, Selection(terms, leaf=True))
        return self._sel[key]

    def draw(self, seed, s, b, margins=True):
        """-> (ids (n,) int8, the smallest margin on the path, the total's selection included)."""
        seq = np.full(self.n, -1, dtype=np.int8)
        margin, a, r = np.inf, 0, self.target
        if self.any and self.n > 0:
            if "total" not in self._sel:
                self._sel["total"] = Selection(self.root[self.lo:self.hi + 1])
            k, margin = self._sel["total"].pick(u24(int(seed) ^ SALT, s, b, 0), margins)
            r = self.lo + k
        for t in range(self.n):
            cs, sel = self._step(t, a, r)
            k, m = sel.pick(u24(seed, s, b, t), margins)
            margin = min(margin, m)
            seq[t] = cs[k]
            nxt = int(self.delta[a, cs[k]])
            a = 0 if nxt >= self.A else nxt
            r = max(r - bit(int(self.counted[t]), cs[k]), 0)
        return seq, margin

    def path_logprob(self, seq):
        """log of the probability with which the draw ends in ``seq``: the total's conditional times those along the path (-inf when it
        cannot be drawn)."""
        k = recount(seq, self.counted)
        lp, r = 0.0, k
        if not self.dfa_miss:
            if self.any:
                if not self.lo <= k <= self.hi or not self.root[k] > NEG:
                    return NEG
                lp = float(self.root[k] - lse(self.root[self.lo:self.hi + 1]))
            elif k != self.target:
                return NEG
        a = 0
        for t in range(self.n):
            cs, terms = self._cells(t, a, r)
            if int(seq[t]) not in cs:
                return NEG
            lp += terms[cs.index(int(seq[t]))] - lse(terms)
            nxt = int(self.delta[a, int(seq[t])])
            a = 0 if nxt >= self.A else nxt
            r = max(r - bit(int(self.counted[t]), int(seq[t])), 0)
        return float(lp)


def design_dfa_count_ref(logits, lengths, temperature, S, seed, delta, kind, counted, lo, hi, cap, allowed=None, bias=None):
    """Padded (B,T,4) logits -> dict: seqs (S,B,T) int8, margin (S,B) f64, infeasible, dfa_miss, count_miss (B,), hits, accepted, count
    (S,B), log_z (B,) f64, plans.  ``cap`` = the call's count_cap (clamped to T here, as the entry clamps it)."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    cap = min(int(cap), T)
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    margin = np.full((S, B), np.inf)
    hits, accepted, count = (np.zeros((S, B), dtype=np.int32) for _ in range(3))
    bad, dmiss, cmiss, plans = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    log_z = np.full(B, NEG)
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plan = DfaCountPlan(logits[b], lengths[b], temperature, delta, kind, counted[b], lo[b], hi[b], cap,
                            None if allowed is None else allowed[b], bi)
        plans.append(plan)
        bad[b], dmiss[b], cmiss[b], log_z[b] = plan.infeasible, plan.dfa_miss, plan.count_miss, plan.log_z
        for s in range(S):
            seqs[s, b, :plan.n], margin[s, b] = plan.draw(int(seed), s, b)
            hits[s, b], accepted[s, b] = follow(seqs[s, b], delta, kind)
            count[s, b] = recount(seqs[s, b], counted[b])
    return dict(seqs=seqs, margin=margin, infeasible=bad, dfa_miss=dmiss, count_miss=cmiss, hits=hits, accepted=accepted, count=count,
                log_z=log_z, plans=plans)


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# T = 72, S = 4, logits 3 * randn, a seed above 2^32.  No base pairs (the entry refuses them).
#   b  n    what it is there for
#   0  0    the empty RNA: feasible iff state 0 accepts (max_run alone), else dfa_miss = 1
#   1  1    one position: shorter than every required motif (dfa_miss = 1 under the two automata that require one)
#   2  2    the same
#   3  3    the same, and allowed[1] = 0: drawn as free, counts 1 in `infeasible`
#   4  16   fixed and IUPAC positions: 2..5 fixed to GAAA (a GNRA), 8 is Y, 9 is R, 12 omits G
#   5  17   0..5 and 11..16 fixed to AUAUAU: at most 5 of 17 can be C or G, so the G+C window 8..10 is unreachable - target 5,
#           count_miss = 3; the five free positions hold a GNRA but not two 5-mers (dfa_miss = 1 under the third automaton).  The mutation
#           reference equals the fixed letters there, so the budgets stay reachable
#   6  33   a per-position bias (the other rows' bias is zero)
#   7  64   free over 64 positions: L (K + 1) runs into the thousands under the G+C window
CASE_LENGTHS = [0, 1, 2, 3, 16, 17, 33, 64]
CASE_T, CASE_S = 72, 4
CASE_SEED = 0x0123_4567_89AB_CDF1                                  # above 2^32: the 64-bit seed arithmetic is exercised
CASE_INFEASIBLE = [0, 0, 0, 1, 0, 0, 0, 0]
# The automata: (require, avoid, max_run) as ``as_nested_automaton`` takes them, with their live states
CASE_AUTOMATA = {"run3": (None, None, 3), "gnra_run3": (("GNRA",), None, 3), "two_run3": (("GGAGG", "CUUCG"), None, 3)}
CASE_LIVE = {"run3": 13, "gnra_run3": 53, "two_run3": 73}
# The count sides: name -> (what counts, the window, count_cap)
CASE_SIDES = ("gc", "mut4", "mut2_6")


def case_arrays():
    """-> dict of numpy arrays: logits (B,T,4) f32 (zero on padding), mask, allowed, bias (B,T,4), reference (B,T) int8, packed, cu."""
    B, T = len(CASE_LENGTHS), CASE_T
    rng = np.random.RandomState(20250607)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    mask = np.zeros((B, T), dtype=np.float32)
    for b, n in enumerate(CASE_LENGTHS):
        mask[b, :n] = 1
    logits *= mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    allowed[3, 1] = 0
    allowed[4, 2:6] = (8, 1, 1, 1)
    allowed[4, 8], allowed[4, 9], allowed[4, 12] = 6, 9, 7
    fixed5 = np.array([1, 2, 1, 2, 1, 2], dtype=np.uint8)         # AUAUAU as masks
    allowed[5, 0:6], allowed[5, 11:17] = fixed5, fixed5
    bias = np.zeros((B, T, 4), dtype=np.float32)
    bias[6, :CASE_LENGTHS[6]] = rng.standard_normal((CASE_LENGTHS[6], 4)).astype(np.float32)
    reference = rng.randint(0, 4, size=(B, T)).astype(np.int8)
    reference[5, 0:6] = reference[5, 11:17] = (0, 1, 0, 1, 0, 1)
    reference[mask == 0] = -1
    return dict(B=B, logits=logits, mask=mask, allowed=allowed, bias=bias, reference=reference,
                packed=np.ascontiguousarray(logits[mask != 0]), cu=np.concatenate([[0], np.cumsum(CASE_LENGTHS)]).astype(np.int32))


def case_side(side, h=None):
    """-> (counted (B,T) u8, lo (B,) i32, hi (B,) i32, count_cap) of a count side, as ``design_dfa_count_from_logits`` passes them."""
    h = case_arrays() if h is None else h
    B, T = h["mask"].shape
    if side == "gc":
        lo, hi = gc_window(CASE_LENGTHS)
        return np.full((B, T), 12, dtype=np.uint8), lo, hi, T
    ref = h["reference"].astype(np.int64)
    counted = np.where((ref >= 0) & (ref <= 3), 15 ^ (1 << np.clip(ref, 0, 3)), 0).astype(np.uint8)
    lo, hi = {"mut4": (0, 4), "mut2_6": (2, 6)}[side]
    return counted, np.full(B, lo, dtype=np.int32), np.full(B, hi, dtype=np.int32), hi


_CASE_REF = {}


def case_ref(name, side, delta, kind, temperature, S=CASE_S, seed=CASE_SEED):
    """The restatement's draws of the batch under automaton ``name`` (its tables passed in) and count side ``side``, once per process
    and never written to."""
    key = (name, side, float(temperature), S, seed)
    if key not in _CASE_REF:
        h = case_arrays()
        counted, lo, hi, cap = case_side(side, h)
        _CASE_REF[key] = design_dfa_count_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, delta, kind, counted, lo, hi, cap,
                                              h["allowed"], h["bias"])
    return _CASE_REF[key]
