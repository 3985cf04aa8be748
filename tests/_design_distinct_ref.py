"""Float64 numpy restatement of the beam ``rnampnn_design_distinct`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_distinct_*.py.  The units of an RNA (single positions, feasible pairs, their cells in order and z) come from
``_design_gc_ref.GcPlan``, which restates the masks, the validation of the partner table and the infeasible count of the family;
l = z - LSE, the prefix hash, the conditioned Gumbel keys, the selection order and the single-cell rule are restated here.  Besides the
slots a run returns its MARGIN: the smallest relative gap |k1 - k2| / max(|k1|, |k2|) between two keys that were neighbours in a selection's
order down to the first loser - the decisions the result rests on.  The device differs from this file by last-bit exp / log / log1p, so a
run whose margin is within that rounding may legitimately come out in another order.  ``brute_force`` enumerates a short RNA outright."""
import itertools

import numpy as np

from _design_gc_ref import GcPlan, lse
from _design_ref import M64, PAIRS, mix64

SALT = 0xE7037ED1A0B428DB
MAX_S = 256
NEG = -np.inf
_K_B, _K_T = np.uint64(0xD6E8FEB86659FD93), np.uint64(0xBF58476D1CE4E5B9)


def mix64_np(x):
    """``mix64`` on uint64 arrays (the products wrap modulo 2^64)."""
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def root_hash(seed, b):
    return mix64(mix64((int(seed) ^ SALT) & M64) ^ ((0xD6E8FEB86659FD93 * (b + 1)) & M64))


def child_hash(h, t, cell):
    """H(child) of the parents ``h`` (uint64 array) at the unit of position ``t`` for the cell ids ``cell`` (broadcast against h)."""
    return mix64_np(h ^ (_K_T * (np.uint64(16 * (t + 1)) + np.asarray(cell, dtype=np.uint64))))


def lds_bytes(S, T):
    """The header's formula for the kernel's dynamic LDS."""
    return 144 * S + 16 * ((S + 7) // 8) + 6752 + 16 * (((S + (S + 1) // 2) * T + 15) // 16)


def units_of(logits, n, temperature, allowed=None, partner=None, wobble=True, bias=None):
    """-> ([(t, j or -1, cell ids, l (k,) f64)] in unit order, infeasible).  A cell id is c for a position and 4 a + b for a pair."""
    plan = GcPlan(logits, n, temperature, 0, n, allowed, partner, wobble, bias)
    units = []
    for t in range(plan.n):
        if plan.kind[t] == 2:
            continue
        z = np.array([x[1] for x in plan.cands[t]], dtype=np.float64)
        ids = [4 * x[0][0] + x[0][1] if plan.kind[t] == 1 else x[0] for x in plan.cands[t]]
        with np.errstate(invalid="ignore"):
            ell = z - lse(z)
        units.append((t, int(plan.mate[t]) if plan.kind[t] == 1 else -1, ids, ell))
    return units, plan.infeasible


def _no_nan(x):
    return np.where(np.isnan(x), NEG, x)


def beam(units, n, S, noise, seed=0, b=0):
    """-> (seqs (live, n) int8, logp (live,) f64, margin).  ``live`` = the slots filled."""
    phi, G = np.zeros(1), np.zeros(1)
    H = np.array([root_hash(seed, b)], dtype=np.uint64)
    back, margin = [], np.inf
    with np.errstate(all="ignore"):
        for t, j, ids, ell in units:
            nc, live = len(ids), len(phi)
            if nc == 1:                                            # no selection: every slot keeps its place
                phi = phi + ell[0]
                if noise:
                    H = child_hash(H, t, ids[0])
                else:
                    G = _no_nan(phi)
                back.append((t, j, np.arange(live), np.full(live, ids[0])))
                continue
            f = phi[:, None] + ell[None, :]
            Hc = None
            if noise:
                Hc = child_hash(H[:, None], t, np.array(ids)[None, :])
                u = ((Hc >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
                g = f - np.log(-np.log(u))
                Z = np.fmax.reduce(g, axis=1, initial=NEG)[:, None]
                v = G[:, None] - g + np.log1p(-np.exp(g - Z))
                kap = G[:, None] - np.maximum(0.0, v) - np.log1p(np.exp(-np.abs(v)))
                kap = np.where(g == Z, G[:, None], kap)
            else:
                kap = f
            key = _no_nan(kap).ravel()                             # candidate index = parent slot * nc + cell: the tie order
            order = np.argsort(-key, kind="stable")
            top = key[order[:S + 1]]
            if len(top) > 1:
                gap = np.abs(top[:-1] - top[1:]) / np.maximum(np.maximum(np.abs(top[:-1]), np.abs(top[1:])), 1e-300)
                margin = min(margin, float(np.min(np.where(np.isnan(gap), 0.0, gap))))
            keep = order[:S]
            p, k = keep // nc, keep % nc
            phi, G = f.ravel()[keep], key[keep]
            if noise:
                H = Hc.ravel()[keep]
            back.append((t, j, p, np.array(ids)[k]))
    live = len(phi)
    seqs = np.full((live, n), -1, dtype=np.int8)
    at = np.arange(live)
    for t, j, p, cell in reversed(back):
        if j >= 0:
            seqs[:, t], seqs[:, j] = cell[at] >> 2, cell[at] & 3
        else:
            seqs[:, t] = cell[at]
        at = p[at]
    return seqs, phi, margin


def design_distinct_ref(logits, lengths, temperature, S, seed, noise, allowed=None, partner=None, wobble=True, bias=None, rows=None):
    """Padded (B,T,4) logits -> (seqs (S,B,T) int8, logp (S,B) f64, n_distinct (B,), infeasible (B,), margin (B,) f64).  Empty slots hold -1
    and -inf.  ``rows``: the batch rows to run (the others stay empty)."""
    logits = np.asarray(logits)
    B, T = logits.shape[:2]
    seqs = np.full((S, B, T), -1, dtype=np.int8)
    logp = np.full((S, B), NEG)
    nd, bad, margin = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.full(B, np.inf)
    for b in range(B):
        if rows is not None and b not in rows:
            continue
        n = int(lengths[b])
        bi = None if bias is None else (np.asarray(bias) if np.asarray(bias).ndim == 1 else np.asarray(bias)[b])
        units, bad[b] = units_of(logits[b], n, temperature, None if allowed is None else allowed[b], None if partner is None else partner[b],
                                 wobble, bi)
        sq, lp, margin[b] = beam(units, n, S, noise, seed, b)
        nd[b] = len(lp)
        seqs[:len(lp), b, :n], logp[:len(lp), b] = sq, lp
    return seqs, logp, nd, bad, margin


def brute_force(z, mask, partner, wobble):
    """Every sequence the constraints admit, by enumeration (n <= 7), written independently of the units: an empty mask is free, a pair
    without an admitted compatible cell is two single positions.  z (n,4) f64 -> [(sequence, log-probability)], most probable first."""
    n = len(mask)
    assert n <= 7
    mask = [int(m) & 15 or 15 for m in mask]
    pairs = []
    for t in range(n):
        j = int(partner[t])
        if t < j < n and int(partner[j]) == t and any((mask[t] >> a) & 1 and (mask[j] >> c) & 1 for a, c in PAIRS[bool(wobble)]):
            pairs.append((t, j))
    rows = []
    for seq in itertools.product(range(4), repeat=n):
        if all((mask[t] >> seq[t]) & 1 for t in range(n)) and all((seq[i], seq[j]) in PAIRS[bool(wobble)] for i, j in pairs):
            rows.append((seq, float(sum(z[t, seq[t]] for t in range(n)))))
    total = lse(np.array([w for _, w in rows]))
    return sorted(((s, w - total) for s, w in rows), key=lambda r: -r[1])


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
# One padded batch, T = 300, logits = 2 * randn:
#   b  n    constraints
#   0  1    free
#   1  2    both fixed to A and paired: an infeasible pair (counts 2, two single positions with one cell each: ONE admitted sequence)
#   2  7    a pair (0, 6), position 2 fixed to G, position 3 IUPAC Y, allowed[4] = 0 (drawn free, counts 1): brute force applies
#   3  33   nested pairs (i, 32 - i), i < 12; 5 fixed to G (its partner is then C or U), 20 IUPAC R
#   4  64   a pseudoknot (i, 30 - i) and (10 + i, 50 - i), i < 5; a malformed table (20 -> 21 one-sided, 22 -> 22, 23 -> 1000, 24 -> -7,
#           25 -> 70 in the padding, which points back)
#   5  300  a long hairpin (i, 299 - i), i < 100, whose ends lie in different 256-strides; 150 fixed to A, 151 omits G
CASE_LENGTHS = [1, 2, 7, 33, 64, 300]
CASE_T = 300
CASE_SEED = 0x0123_4567_89AB_CDF1                                  # above 2^32: the 64-bit seed arithmetic and the salt's XOR are exercised
CASE_INFEASIBLE = [0, 2, 1, 0, 0, 0]
CASE_PAIRS = ([(1, 0, 1), (2, 0, 6)] + [(3, i, 32 - i) for i in range(12)] + [(4, i, 30 - i) for i in range(5)]
              + [(4, 10 + i, 50 - i) for i in range(5)] + [(5, i, 299 - i) for i in range(100)])
CASE_RUNS = [(S, temperature, noise) for S in (1, 8, 256) for temperature in (1.0, 0.3) for noise in (1, 0)]
MARGIN = 1e-9


def case_arrays():
    """-> dict of numpy arrays: logits (B,T,4) f32 = 2 * randn (zero on padding), mask, allowed, partner, packed, cu."""
    B, T = len(CASE_LENGTHS), CASE_T
    rng = np.random.RandomState(20261019)
    logits = (2.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    mask = np.zeros((B, T), dtype=np.float32)
    for b, n in enumerate(CASE_LENGTHS):
        mask[b, :n] = 1
    logits *= mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    partner = np.full((B, T), -1, dtype=np.int32)
    for b, i, j in CASE_PAIRS:
        partner[b, i], partner[b, j] = j, i
    allowed[1, 0] = allowed[1, 1] = 1
    allowed[2, 2], allowed[2, 3], allowed[2, 4] = 8, 6, 0
    allowed[3, 5], allowed[3, 20] = 8, 9
    partner[4, 20] = 21; partner[4, 22] = 22; partner[4, 23] = 1000; partner[4, 24] = -7; partner[4, 25] = 70; partner[4, 70] = 25
    allowed[5, 150], allowed[5, 151] = 1, 7
    return dict(B=B, logits=logits, mask=mask, allowed=allowed, partner=partner, packed=np.ascontiguousarray(logits[mask != 0]),
                cu=np.concatenate([[0], np.cumsum(CASE_LENGTHS)]).astype(np.int32))


_CASE_REF = {}


def case_ref(S, temperature, noise, seed=CASE_SEED):
    """The restatement's slots of the batch, computed once per process and never written to."""
    key = (int(S), float(temperature), int(bool(noise)), seed)
    if key not in _CASE_REF:
        h = case_arrays()
        _CASE_REF[key] = design_distinct_ref(h["logits"], CASE_LENGTHS, temperature, S, seed, noise, h["allowed"], h["partner"], True)
    return _CASE_REF[key]
