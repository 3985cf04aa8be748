"""Float64 numpy restatement of the profile ``rnampnn_design_dfa_profile`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_dfa_profile_*.py.  The backward table, the masks, z and ``dfa_miss`` are ``_design_dfa_ref.DfaPlan``'s - the plan the
draws' restatement walks - so the profile and the draws it describes read the same table; the forward pass over the automaton is written
out here in the log domain, as the header states it: alpha_0(0) = 0, alpha_{t+1}(a') = LSE over the admitted cells (a, c) that lead to a'
of alpha_t(a) + z_t(c), P_t(c) = the sum over the admitted cells with a finite l_{t+1} of exp(alpha_t(a) + z_t(c) + l_{t+1}(delta(a,c)) -
log_z).  ``enumerate_dfa_profile`` knows no automaton pass at all: it sums exp(sum of z) over every sequence that the masks admit and that
``follow`` accepts without entering a dead state."""
import itertools

import numpy as np

from _design_dfa_ref import DfaPlan, follow
from _design_gc_ref import NEG, lse
from _design_profile_ref import Profile, _finish, _pad


def dfa_profile(plan):
    """The distribution ``DfaPlan.draw`` samples from -> Profile."""
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
    target = np.where(plan.live_cell, plan.delta, 0)
    source_live = ~plan.dead
    alpha = np.full(A, NEG)
    alpha[0] = 0.0
    for t in range(n):
        has = ((plan.mask[t] >> np.arange(4)) & 1).astype(bool)
        admitted = plan.live_cell & has[None, :] & source_live[:, None]                      # (A,4)
        with np.errstate(invalid="ignore"):
            cand = np.where(admitted, alpha[:, None] + z[t][None, :], NEG)
            term = np.where(admitted & (l[t + 1][target] > NEG), cand + l[t + 1][target] - log_z, NEG)
            P[t] = np.exp(term).sum(axis=0)
            top = np.full(A, NEG)
            np.maximum.at(top, target[admitted], cand[admitted])
            acc = np.zeros(A)
            shift = np.where(top > NEG, top, 0.0)
            np.add.at(acc, target[admitted], np.exp(cand[admitted] - shift[target[admitted]]))
            alpha = np.where(top > NEG, shift + np.log(np.where(acc > 0, acc, 1.0)), NEG)
    return _finish(plan, P, log_z)


def enumerate_dfa_profile(plan):
    """-> (marginals (n,4), entropy, log_z, count) over every sequence of the plan's length that the masks admit and the automaton
    accepts without entering a dead state: p = exp(sum of z - log_z), the marginals the sums of p, the entropy - sum of p log p; count =
    how many there are.  For a plan with ``miss`` (count 0) the set is every admitted sequence, as the draw falls back to."""
    n = plan.n
    seqs, terms = [], []
    for seq in itertools.product(*[[c for c in range(4) if (plan.mask[t] >> c) & 1] for t in range(n)]):
        hits, accepted = follow(seq, plan.delta, plan.kind)
        if plan.miss or (hits == 0 and accepted):
            seqs.append(seq)
            terms.append(sum(plan.z[t, c] for t, c in enumerate(seq)))
    terms = np.array(terms, dtype=np.float64)
    log_z = float(lse(terms))
    p = np.exp(terms - log_z)
    P = np.zeros((n, 4))
    for seq, w in zip(seqs, p):
        for t, c in enumerate(seq):
            P[t, c] += w
    H = float(-(p * (terms - log_z)).sum())
    return P, H, log_z, 0 if plan.miss else len(seqs)


def design_dfa_profile_ref(logits, lengths, temperature, delta, kind, allowed=None, bias=None):
    """Padded (B,T,4) logits -> dict: marginals (B,T,4), log_z, log_z_free, entropy (B,) f64, infeasible, miss (B,) int32, plans.  The
    scalars of an RNA of length 0 are 0 and its miss is !(state 0 accepts), as ``DfaPlan`` has it."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    plans = []
    for b in range(B):
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        plans.append(DfaPlan(logits[b], lengths[b], temperature, delta, kind, None if allowed is None else allowed[b], bi))
    res = _pad([dfa_profile(p) for p in plans], T)
    res.update(infeasible=np.array([p.infeasible for p in plans], dtype=np.int32), miss=np.array([p.miss for p in plans], dtype=np.int32), plans=plans)
    return res
