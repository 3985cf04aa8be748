"""Float64 numpy restatement of the design profiles ``rnampnn_design_count_profile`` and ``rnampnn_design_avoid_profile`` document
(include/rnampnn_hip.h): the yardstick of tests/test_design_profile_*.py.  The inside tree, the window, the target and the k_min rule are
``_design_count_ref.CountPlan``'s, the backward table is ``_design_avoid_ref.AvoidPlan``'s - the plans the draws' restatements walk - so a
profile and the draws it describes read the same tables; the outside pass over the tree and the forward pass over the automaton are written
out here, plainly.  ``enumerate_profile`` knows neither: it sums ``exp(plan.path_logprob(seq))`` - the product of the draw's own
conditionals - over every sequence."""
import itertools
from collections import namedtuple

import numpy as np

from _design_avoid_ref import AvoidPlan
from _design_count_ref import CountPlan
from _design_gc_ref import NEG, lse

Profile = namedtuple("Profile", "marginals log_z log_z_free entropy")           # (n,4), and three floats, of ONE RNA


def _finish(plan, P, log_z):
    """(marginals, log_z) -> Profile: the free sum and the entropy log_z - sum of P z over the cells with P > 0."""
    z = plan.z
    free = float(sum(lse(z[t]) for t in range(plan.n)))
    if plan.n == 0:
        return Profile(P, 0.0, 0.0, 0.0)
    with np.errstate(invalid="ignore"):
        pz = float(sum(P[t, c] * z[t, c] for t in range(plan.n) for c in range(4) if P[t, c] != 0))      # (a NaN probability is kept: NaN)
    return Profile(P, float(log_z), free, float(log_z) - pz)


def _spread(plan, t, probs, P):
    """The probabilities of leaf t's candidates (``plan.cands[t]`` order) onto the positions: a pair's cell (a, b) adds to P_i(a), P_j(b)."""
    for (ident, _, _), p in zip(plan.cands[t], probs):
        if plan.kind[t] == 1:
            P[t, ident[0]] += p
            P[plan.mate[t], ident[1]] += p
        else:
            P[t, ident] += p


def count_profile(plan):
    """The distribution ``CountPlan.draw`` samples from -> Profile."""
    n = plan.n
    P = np.zeros((n, 4))
    if n == 0:
        return _finish(plan, P, 0.0)
    owners = [t for t in range(n) if plan.kind[t] != 2]
    if plan.at_min:                                                 # every leaf over the cells of its own smallest d, normalised
        log_z = 0.0
        for t in owners:
            d = int(plan.min_d[t])
            zz = np.array([x[1] if x[2] == d else NEG for x in plan.cands[t]])
            l = lse(zz)
            log_z += l
            with np.errstate(invalid="ignore"):
                _spread(plan, t, np.exp(zz - l), P)
        return _finish(plan, P, log_z)
    root = plan.root
    ks = [plan.target] if plan.target is not None else [k for k in range(plan.lo, plan.hi + 1) if np.isfinite(root[k])]
    log_z = lse(root[ks])
    out = [[None] * len(level) for level in plan.levels]
    top = np.full(len(root), NEG)
    top[ks] = 0.0
    out[-1][0] = top
    for l in range(len(plan.levels) - 1, 0, -1):                    # node (l, i) hands its halves at level l - 1 their outsides
        child = plan.levels[l - 1]
        for i, O in enumerate(out[l]):
            L = child[2 * i]
            if 2 * i + 1 >= len(child):                             # an empty right half: the left half is the node
                out[l - 1][2 * i] = np.array([O[a] if a < len(O) else NEG for a in range(len(L))])
                continue
            R = child[2 * i + 1]
            with np.errstate(invalid="ignore"):                      # O_L(a) = LSE over k of O(k) + R(k - a), k - a among R's, k among O's
                out[l - 1][2 * i] = np.array([lse(O[a:a + len(R)] + R[:len(O[a:a + len(R)])]) for a in range(len(L))])
                out[l - 1][2 * i + 1] = np.array([lse(O[c:c + len(L)] + L[:len(O[c:c + len(L)])]) for c in range(len(R))])
    for t in owners:
        O = out[0][t]
        with np.errstate(invalid="ignore"):
            _spread(plan, t, [np.exp(zz + O[g] - log_z) if g < len(O) else 0.0 for _, zz, g in plan.cands[t]], P)
    return _finish(plan, P, log_z)


def avoid_profile(plan):
    """The distribution ``AvoidPlan.draw`` samples from -> Profile."""
    n, A, z, l = plan.n, plan.A, plan.z, plan.l
    P = np.zeros((n, 4))
    if n == 0:
        return _finish(plan, P, 0.0)
    if plan.miss:                                                   # what the draw falls back to: the softmax over the admitted classes
        log_z = 0.0
        for t in range(n):
            zz = np.array([z[t, c] if (plan.mask[t] >> c) & 1 else NEG for c in range(4)])
            log_z += lse(zz)
            with np.errstate(invalid="ignore"):
                P[t] = np.exp(zz - lse(zz))
        return _finish(plan, P, log_z)
    log_z = l[0, 0]
    alpha = np.full(A, NEG)
    alpha[0] = 0.0
    for t in range(n):
        into = [[] for _ in range(A)]
        for a in range(A):
            if plan.dead[a]:
                continue
            for c in range(4):
                if plan._live_cell(t, a, c):
                    nxt = plan.delta[a, c]
                    with np.errstate(invalid="ignore"):
                        P[t, c] += np.exp(alpha[a] + z[t, c] + l[t + 1, nxt] - log_z)
                    into[nxt].append(alpha[a] + z[t, c])
        alpha = np.array([lse(np.array(v)) for v in into])
    return _finish(plan, P, log_z)


def enumerate_profile(plan):
    """-> (marginals (n,4), entropy, total, log_z) over every sequence of the plan's length with p = exp(path_logprob(seq)) > 0: the
    marginals are the sums of p, the entropy - sum p log p, total the sum of p (1 for a draw that is a distribution) and log_z the LSE
    of sum_t z_t(x_t) over those sequences - the set drawn from."""
    n = plan.n
    P, H, total, terms = np.zeros((n, 4)), 0.0, 0.0, []
    for seq in itertools.product(range(4), repeat=n):
        lp = plan.path_logprob(seq)
        if lp > NEG:
            p = np.exp(lp)
            total += p
            H -= p * lp
            terms.append(sum(plan.z[t, c] for t, c in enumerate(seq)))
            for t, c in enumerate(seq):
                P[t, c] += p
    return P, H, total, float(lse(np.array(terms, dtype=np.float64)))


def _pad(profiles, T):
    B = len(profiles)
    marg = np.zeros((B, T, 4))
    for b, p in enumerate(profiles):
        marg[b, :p.marginals.shape[0]] = p.marginals
    return dict(marginals=marg, log_z=np.array([p.log_z for p in profiles]), log_z_free=np.array([p.log_z_free for p in profiles]),
                entropy=np.array([p.entropy for p in profiles]))


def design_count_profile_ref(logits, lengths, temperature, counted, lo, hi, cap, allowed=None, partner=None, wobble=True, bias=None):
    """Padded (B,T,4) logits -> dict: marginals (B,T,4), log_z, log_z_free, entropy (B,) f64, infeasible, miss (B,) int32, plans."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    plans = []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plans.append(CountPlan(logits[b], lengths[b], temperature, lo[b], hi[b], counted[b], min(int(cap), T), None if allowed is None else allowed[b],
                               None if partner is None else partner[b], wobble, bi))
    res = _pad([count_profile(p) for p in plans], T)
    res.update(infeasible=np.array([p.infeasible for p in plans], dtype=np.int32), miss=np.array([p.miss for p in plans], dtype=np.int32), plans=plans)
    return res


def design_avoid_profile_ref(logits, lengths, temperature, delta, terminal, allowed=None, bias=None):
    """Padded (B,T,4) logits -> the dict of ``design_count_profile_ref``."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    plans = []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plans.append(AvoidPlan(logits[b], lengths[b], temperature, delta, terminal, None if allowed is None else allowed[b], bi))
    res = _pad([avoid_profile(p) for p in plans], T)
    res.update(infeasible=np.array([p.infeasible for p in plans], dtype=np.int32), miss=np.array([p.miss for p in plans], dtype=np.int32), plans=plans)
    return res


_CACHE = {}


def cached(key, make):
    """A reference computed once per process and never written to."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- the entropy, conditioned
# The contract's entropy, log_z - sum of P z, is a difference of two numbers of the size of log_z: in float64 it carries roundings of
# 2^-53 |log_z| however small the entropy is, and so does an enumerated - sum p log p whose log p are sums of z - LSE(z).  The
# distribution does not change when every position's z is shifted by a constant, so the CENTRED twin of a plan - z'_t(c) = z_t(c) minus
# the z of the position's most probable class, formed in float64 (exactly 0 for that class; the rounding of the others is scaled by their
# small probability) - describes the same distribution with log_z' and every conditional of the size of the entropy itself.  On the twin
# the same two formulas resolve the entropy to 1e-12 RELATIVE; tests/test_design_profile_cpu.py holds them to that.
def centred_z(plan, marginals):
    n = plan.n
    return plan.z - plan.z[np.arange(n), np.asarray(marginals).argmax(axis=1)][:, None] if n else plan.z


def centred_count_plan(plan, marginals, wobble):
    """The CountPlan of the same units, counted sets, window, cap and pairs on ``centred_z`` (temperature 1, no bias: z' is used as it is)."""
    return CountPlan(centred_z(plan, marginals), plan.n, 1.0, plan.lo, plan.hi, plan.counted, plan.top, plan.mask, plan.mate, wobble)


def centred_avoid_plan(plan, marginals):
    terminal = sum(1 << a for a in range(plan.A) if plan.dead[a])
    return AvoidPlan(centred_z(plan, marginals), plan.n, 1.0, plan.delta, terminal, plan.mask)


# ---------------------------------------------------------------------------------------------------------------- the link to the draws
# Three RNAs of 40 nt at temperature 1, S = 4096 draws each: the class frequencies f of the draws must lie within
# 6 sqrt(P (1 - P) / S) + 1 / S of the profile's P on every cell, and be 0 wherever P is 0.  RNA 0 is free but for two fixed positions, RNA
# 1 carries a hairpin of 8 pairs (the count modes only; wobble on), RNA 2 has G raised by 3 and an IUPAC position.
LINK_LENGTHS, LINK_T, LINK_S, LINK_SEED, LINK_TEMPERATURE = [40, 40, 40], 40, 4096, 0x5DEECE66D0123, 1.0
LINK_GC = ([18, 8, 24], [22, 12, 40])                              # G+C windows in counts
LINK_BUDGET = (2, 5)
LINK_AVOID = ((), 2)                                               # no run longer than 2


def link_arrays():
    B, T = 3, LINK_T
    rng = np.random.RandomState(20241101)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    logits[2, :, 3] += 3.0
    allowed = np.full((B, T), 15, dtype=np.uint8)
    allowed[0, 7], allowed[0, 21], allowed[2, 30] = 1, 8, 6
    partner = np.full((B, T), -1, dtype=np.int32)
    for i in range(8):
        partner[1, 3 + i], partner[1, 36 - i] = 36 - i, 3 + i
    ref = rng.randint(0, 4, size=(B, T)).astype(np.int32)
    for i in range(8):
        ref[1, 36 - i] = (1, 0, 3, 2)[ref[1, 3 + i]]
    return dict(B=B, logits=logits, mask=np.ones((B, T), dtype=np.float32), allowed=allowed, partner=partner, reference=ref)


def link_plans(mode):
    """The plans of the three RNAs in ``mode`` ("gc_content", "mutations", "avoid"), whose ``draw`` and profile the link test compares."""
    h = link_arrays()
    if mode == "avoid":
        from rnampnn.utils.motifs import MotifAutomaton
        auto = MotifAutomaton.from_motifs(list(LINK_AVOID[0]), max_run=LINK_AVOID[1])
        return [AvoidPlan(h["logits"][b], LINK_T, LINK_TEMPERATURE, auto.delta.numpy(), auto.terminal, h["allowed"][b]) for b in range(3)]
    if mode == "gc_content":
        return [CountPlan(h["logits"][b], LINK_T, LINK_TEMPERATURE, LINK_GC[0][b], LINK_GC[1][b], np.full(LINK_T, 12), LINK_T, h["allowed"][b],
                          h["partner"][b], True) for b in range(3)]
    from _design_count_ref import mutation_sets
    return [CountPlan(h["logits"][b], LINK_T, LINK_TEMPERATURE, LINK_BUDGET[0], LINK_BUDGET[1], mutation_sets(h["reference"][b]), LINK_BUDGET[1],
                      h["allowed"][b], h["partner"][b], True) for b in range(3)]


def frequencies(seqs):
    """(S, ..., T) class ids -> (..., T, 4): the share of the S draws that hold class c at a position."""
    seqs = np.asarray(seqs)
    return np.stack([(seqs == c).mean(axis=0) for c in range(4)], axis=-1)


def link_bound(P, S=LINK_S):
    """6 sqrt(P (1 - P) / S) + 1 / S; a fixed position's P = 1 + one rounding has the variance 0."""
    return 6.0 * np.sqrt(np.clip(P * (1.0 - P), 0.0, None) / S) + 1.0 / S
