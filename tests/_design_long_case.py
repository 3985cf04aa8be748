"""The long RNAs of the count tree in global memory (``rnampnn_design_count_long`` / ``rnampnn_design_count_profile_long``), shared by
tests/test_design_long_cpu.py and tests/test_design_long_gpu.py: lengths the LDS entries refuse, each with a hairpin whose pairs straddle the
root's boundary (position 2^(levels - 1)) and a stripe of IUPAC sets, and their float64 restatements (``_design_gc_ref``,
``_design_count_ref``, ``_design_profile_ref``), computed once per process and never written to.  A plain module like ``_design_case.py``.

  name      lengths                 counted, window, cap                                      why this length
  gc1018    1018                    C|G, 45-60 % of the length, uncapped                      the first length rnampnn_design_gc refuses
  gc1025    1025                    the same                                                  an eleventh level whose last node is one position
  gc2049    2049                    the same                                                  a twelfth level of that kind
  mut2868   2868, 2868              mutation sets, the budget (0, 8), cap 8                   the first length rnampnn_design_count refuses at cap 8;
                                                                                              RNA 1's random reference over the hairpin forces more than
                                                                                              8 mutations: count_miss and the k_min rule
  mixed     1, 2, 3, 700, 1300      C|G, 45-60 %, uncapped, T = 1300                          one padded batch, trees of 0, 1, 2, 10 and 11 levels
  pf1025    1025                    C|G, 45-60 %, uncapped                                    the profile: LDS stops at 535
  pf1458    1458                    mutation sets, the budget (2, 8), cap 8                   the profile: LDS stops at 1457 at cap 8
"""
import numpy as np

import _design_count_ref as R
import _design_gc_ref as G
import _design_profile_ref as PR

NEAR = 1e-8
S, SEED = 2, 0x0123_4567_89AB_CDE7
GC = (0.45, 0.60)
STRIPE = (6, 9, 3, 12, 5, 10, 7, 14)                               # IUPAC sets over AUCG = bits 0..3: Y, ., W, S, M, K, H, B

SPECS = {"gc1018": ([1018], "gc", None, 1), "gc1025": ([1025], "gc", None, 1), "gc2049": ([2049], "gc", None, 1),
         "mut2868": ([2868, 2868], "mut", 8, 1), "mixed": ([1, 2, 3, 700, 1300], "gc", None, 1),
         "pf1025": ([1025], "gc", None, 1), "pf1458": ([1458], "mut", 8, 1)}


def hairpin(n):
    """Pairs (i, j) of an RNA of n >= 64 nucleotides that straddle the root's boundary, position mid = 2^(levels - 1): a stem around mid
    where the right half holds one, else the pair (mid - 40, n - 1) and a stem around mid / 2 (the boundary one level down)."""
    mid = 1 << ((n - 1).bit_length() - 1)
    stem = [(mid - 30 - i, mid + 30 + i) for i in range(150) if mid + 30 + i < n and mid - 30 - i >= 0]
    if stem:
        return stem
    half = mid // 2
    return [(mid - 40, n - 1)] + [(half - 30 - i, half + 30 + i) for i in range(150)]


def gc_window(n):
    """``gc_counts`` of the fractions GC on the host."""
    return int(np.ceil(GC[0] * n - 1e-6)), int(np.floor(GC[1] * n + 1e-6))


_CASES, _REFS = {}, {}


def case(name):
    """-> dict: lengths, B, T, logits (B,T,4) f32 = 3 * randn (zero on padding), mask, allowed, partner, counted, lo, hi, cap, wobble,
    reference (mutation cases), packed, cu."""
    if name in _CASES:
        return _CASES[name]
    lengths, kind, cap, seed = SPECS[name]
    B, T = len(lengths), max(lengths)
    rng = np.random.RandomState(seed)
    logits = (3.0 * rng.standard_normal((B, T, 4))).astype(np.float32)
    mask = np.zeros((B, T), dtype=np.float32)
    allowed = np.full((B, T), 15, dtype=np.uint8)
    partner = np.full((B, T), -1, dtype=np.int32)
    ref = rng.randint(0, 4, size=(B, T)).astype(np.int32)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
        ref[b, n:] = -1
        if n < 64:
            continue
        for i, j in hairpin(n):
            partner[b, i], partner[b, j] = j, i
            if not (name == "mut2868" and b == 1):
                ref[b, j] = R.COMPLEMENT[ref[b, i]]
        allowed[b, 8:48] = np.resize(np.array(STRIPE, dtype=np.uint8), 40)      # the stripe; the stems lie beyond position 64
        ref[b, 8:48] = [(int(m) & -int(m)).bit_length() - 1 for m in allowed[b, 8:48]]  # a reference the stripe admits: it forces no mutation
    logits *= mask[..., None]
    if kind == "gc":
        counted = np.where(mask != 0, 12, 0).astype(np.uint8)
        lo, hi = (np.array(v, dtype=np.int32) for v in zip(*[gc_window(n) for n in lengths]))
        cap = T
    else:
        counted = R.mutation_sets(ref)
        lo = np.full(B, 2 if name == "pf1458" else 0, dtype=np.int32)
        hi = np.full(B, 8, dtype=np.int32)
    d = dict(lengths=lengths, B=B, T=T, logits=logits, mask=mask, allowed=allowed, partner=partner, counted=counted, lo=lo, hi=hi, cap=int(cap),
             wobble=kind == "gc", reference=ref, packed=np.ascontiguousarray(logits[mask != 0]),
             cu=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), kind=kind)
    _CASES[name] = d
    return d


def draw_ref(name):
    """The restatement's S draws of ``case(name)`` at temperature 1 -> (seqs (S,B,T) int8, margin (S,B), infeasible (B,), miss (B,), plans):
    ``_design_gc_ref`` for gc1018 and gc1025 (what rnampnn_design_gc draws), ``_design_count_ref`` for the others."""
    if name not in _REFS:
        c = case(name)
        if name in ("gc1018", "gc1025"):
            _REFS[name] = G.design_gc_ref(c["logits"], c["lengths"], 1.0, S, SEED, c["lo"], c["hi"], c["allowed"], c["partner"], True)
        else:
            seqs, margin, bad, miss, _, plans = R.design_count_ref(c["logits"], c["lengths"], 1.0, S, SEED, c["counted"], c["lo"], c["hi"], c["cap"],
                                                                   c["allowed"], c["partner"], c["wobble"])
            _REFS[name] = (seqs, margin, bad, miss, plans)
    return _REFS[name]


def profile_ref(name):
    """The restatement's profile of ``case(name)`` at temperature 1 (``_design_profile_ref.design_count_profile_ref``)."""
    c = case(name)
    return PR.cached(("long", name), lambda: PR.design_count_profile_ref(c["logits"], c["lengths"], 1.0, c["counted"], c["lo"], c["hi"], c["cap"],
                                                                         c["allowed"], c["partner"], c["wobble"]))


def count_of(seqs, counted):
    """The count of written bytes: the sum over t of bit(counted[b,t], id) (0 on padding)."""
    ids = np.clip(seqs.astype(np.int64), 0, 3)
    return (((counted.astype(np.int64)[None] >> ids) & 1) * (seqs >= 0)).sum(axis=2)


def tree_doubles(T, cap):
    """doubles(T, cap) of include/rnampnn_hip.h on the host: the sum over the nodes of the levels 1 .. ceil(log2 T) of
    min(2 * (extent within T), T, cap) + 1."""
    cap, doubles, l = min(cap, T), 0, 1
    while (1 << (l - 1)) < T:
        size = 1 << l
        nodes = (T + size - 1) // size
        doubles += (nodes - 1) * (min(2 * size, T, cap) + 1) + min(2 * (T - (nodes - 1) * size), T, cap) + 1
        l += 1
    return doubles
