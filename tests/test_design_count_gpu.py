"""``rnampnn_design_count`` (csrc/design_count.hip) on the device, against the float64 restatement of its contract in
tests/_design_count_ref.py, against ``rnampnn_design_gc`` (counted = C|G everywhere is the same draw, byte for byte) and against an
enumerated joint.

The batch is the one ``_design_count_ref`` describes next to ``CASE_LO`` (the batch of the G+C tests - lengths 0, 1, 2, 3, 63, 64, 65, 257,
300; T = 300, S = 4, logits 3 * randn, a seed above 2^32, a hairpin, pairs across node boundaries, a pseudoknot, a fixed end inside a pair,
an infeasible pair, ``allowed = 0``, a malformed partner table - with wobble off and a reference per RNA whose mutation sets are counted):
the free window, (0, 0), (0, 3), (2, 2), a window below k_min, lo > hi and out-of-range windows, at cap 8 and at cap T.

Device and restatement differ by last-bit exp / log and the summation order inside a node (about 1e-12 relative), so a draw whose path has
a selection within 1e-8 of a cumulative boundary is left out of the equality check; tests/test_design_count_cpu.py bounds the share of such
draws by 1 % for the restatement alone, and the same bound is asserted here."""
import csv
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rna-mpnn_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_count_ref as R  # noqa: E402
import _design_gc_ref as G  # noqa: E402
from _design_ref import PAIRS  # noqa: E402
from _design_case import SMALL, design_outputs, raw_design, _bytes, _dev, _specs, _write_data, _checkpoint  # noqa: E402

LENGTHS, T, S, SEED = R.CASE_LENGTHS, R.CASE_T, R.CASE_S, R.CASE_SEED
NEAR = 1e-8
T_MAX_CAP8 = 2867                                                  # the largest padded extent whose tree fits 160 KiB of LDS at cap 8
OUTPUTS = ("seqs", "seq_nll", "infeasible", "count", "count_miss")


FURTHER = (("count", torch.int32, True), ("count_miss", torch.int32, False))


def _outputs(S, B, T):
    return design_outputs(FURTHER, S, B, T)


def design_count(logits, counted, lo, hi, cap, seed=SEED, S=S, wobble=R.CASE_WOBBLE, **kw):
    """The C entry on device tensors (numpy arrays are uploaded) -> dict of its five outputs."""
    return raw_design("rnampnn_design_count", (_dev(counted, torch.uint8), _dev(lo, torch.int32), _dev(hi, torch.int32), int(cap)), FURTHER,
                      logits, seed=seed, S=S, wobble=wobble, **kw)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = R.case_arrays()
    d = dict(h=h, run={})
    for k in ("logits", "mask", "allowed", "partner", "packed", "cu", "lo", "hi", "counted"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _run(case, temperature=1.0, cap=8, layout="padded"):
    """The batch through the kernel, once per (temperature, cap, layout)."""
    key = (float(temperature), int(cap), layout)
    if key not in case["run"]:
        kw = dict(temperature=temperature, allowed=case["allowed"], partner=case["partner"])
        if layout == "padded":
            case["run"][key] = design_count(case["logits"], case["counted"], case["lo"], case["hi"], cap, mask=case["mask"], **kw)
        else:
            case["run"][key] = design_count(case["packed"], case["counted"], case["lo"], case["hi"], cap, cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _count_of(seqs, counted):
    """The count of written bytes: the sum over t of bit(counted[b,t], id) (0 on padding)."""
    ids = np.clip(seqs.astype(np.int64), 0, 3)
    return (((counted.astype(np.int64)[None] >> ids) & 1) * (seqs >= 0)).sum(axis=2)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("cap", R.CASE_CAPS)
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_restatement(case, temperature, cap):
    out = _run(case, temperature, cap)
    want, margin, bad, miss, count, plans = R.case_ref(temperature, cap)
    got = out["seqs"].cpu().numpy()
    near = margin <= NEAR
    print(f"temperature {temperature}, cap {cap}: {near.mean():.4%} of the {near.size} (sample, RNA) draws left out (a selection within {NEAR} "
          f"of a boundary)")
    assert near.mean() <= 0.01
    assert out["count_miss"].tolist() == miss.tolist() and miss[8] == plans[8].k_min - 3 > 0 and plans[8].at_min == (cap == 8)
    assert out["infeasible"].tolist() == bad.tolist() == R.CASE_INFEASIBLE
    differ = [(s, b) for s in range(S) for b in range(len(LENGTHS)) if not near[s, b] and not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"
    keep = ~near
    assert np.array_equal(out["count"].cpu().numpy()[keep], count[keep])
    assert np.array_equal(out["count"].cpu().numpy(), _count_of(got, case["h"]["counted"]))


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_counting_c_and_g_everywhere_is_rnampnn_design_gc_byte_for_byte(case, temperature):
    """The G+C tests' own batch with counted = 12 everywhere and cap = T: every RNA whose window is reachable gets the bytes of
    rnampnn_design_gc - no draw is left out."""
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    h = G.case_arrays()
    B = h["B"]
    lg, m, al, pa = (_dev(h[k]) for k in ("logits", "mask", "allowed", "partner"))
    lo, hi, bi = _dev(h["lo"]), _dev(h["hi"]), _dev(G.CASE_BIAS)
    gc = _outputs(S, B, T)
    _native.check(_native.lib().rnampnn_design_gc(
        _ptr(lg), B * T, _ptr(m), None, B, T, float(temperature), S, C.c_uint64(SEED), None, _ptr(al), _ptr(pa), 1, _ptr(bi), 0, _ptr(lo),
        _ptr(hi), *[_ptr(gc[k]) for k in OUTPUTS], _stream(lg.device)))
    out = design_count(lg, np.full((B, T), 12, dtype=np.uint8), lo, hi, T, mask=m, temperature=temperature, allowed=al, partner=pa, wobble=True,
                       bias=bi)
    rows = [b for b in range(B) if G.CASE_MISS[b] == 0]
    assert len(rows) == B - 1
    for k in ("seqs", "seq_nll", "count"):
        assert _bytes(out[k][:, rows]) == _bytes(gc[k][:, rows]), k
    assert _bytes(out["infeasible"][rows]) == _bytes(gc["infeasible"][rows]) and out["count_miss"].tolist() == gc["count_miss"].tolist()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_the_cap_does_not_change_the_bytes(case):
    """Windows with hi <= 3 at cap 3, 8 and T: every output of an RNA whose target lies within the smallest cap has identical bytes.  The
    two RNAs whose structure forces more than 3 mutations (4 and 8) hold k_min at every cap, with the same count_miss."""
    hi = torch.clamp(case["hi"], max=3)
    lo = torch.minimum(case["lo"].clamp(min=0), hi)
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], partner=case["partner"])
    runs = [design_count(case["logits"], case["counted"], lo, hi, cap, **kw) for cap in (3, 8, T)]
    k_min = [p.k_min for p in R.case_ref(1.0, 8)[5]]
    rows = [b for b in range(len(LENGTHS)) if k_min[b] <= 3]
    assert rows == [0, 1, 2, 3, 5, 6, 7]
    for other in runs[1:]:
        for k in ("seqs", "seq_nll", "count"):
            assert _bytes(runs[0][k][:, rows]) == _bytes(other[k][:, rows]), k
        assert _bytes(runs[0]["infeasible"]) == _bytes(other["infeasible"]) and _bytes(runs[0]["count_miss"]) == _bytes(other["count_miss"])
        assert _bytes(runs[0]["count"]) == _bytes(other["count"])
    # (RNA 2 is fixed to one mutation under the window (2, 2): the search finds 1, within every cap)
    assert runs[0]["count_miss"].tolist() == [0, 0, 1, 0, k_min[4] - 3, 0, 0, 0, k_min[8] - 3]
    assert _bytes(runs[0]["seqs"][:, 8]) == _bytes(runs[1]["seqs"][:, 8])       # k_min > 8 as well: every leaf at its minimum at both caps


# ---------------------------------------------------------------------------------------------------------------- 4
def test_count_is_the_count_of_the_bytes_and_lies_in_the_window(case):
    counted = case["h"]["counted"]
    for cap in R.CASE_CAPS:
        miss = R.case_ref(1.0, cap)[3]
        for temperature in (1.0, 0.3, 1e-3):
            out = _run(case, temperature, cap)
            got, count = out["seqs"].cpu().numpy(), out["count"].cpu().numpy()
            assert np.array_equal(count, _count_of(got, counted))
            for b, n in enumerate(LENGTHS):
                assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
                top = min(n, cap)
                lo = min(max(R.CASE_LO[b], 0), top)
                hi = max(min(max(R.CASE_HI[b], 0), top), lo)
                if miss[b] == 0:
                    assert ((count[:, b] >= lo) & (count[:, b] <= hi)).all(), (temperature, cap, b, count[:, b])
            ref = case["h"]["reference"]
            known = (ref >= 0) & (ref <= 3)
            assert np.array_equal(count, ((got != ref[None]) & known[None] & (got >= 0)).sum(axis=2))    # the Hamming distance to the reference


def test_masks_and_pair_compatibility_hold_in_every_draw(case):
    h = case["h"]
    for cap in R.CASE_CAPS:
        for temperature in (1.0, 1e-3):
            got = _run(case, temperature, cap)["seqs"].cpu().numpy()
            for b, n in enumerate(LENGTHS):
                m = h["allowed"][b, :n].astype(np.int64) & 15
                m = np.where(m == 0, 15, m)
                assert ((m[None] >> got[:, b, :n]) & 1).all(), b
            for b, i, j in R.CASE_PAIRS:
                if b != 2:                                         # (2; 0,1) is the infeasible pair
                    assert all((int(got[s, b, i]), int(got[s, b, j])) in PAIRS[R.CASE_WOBBLE] for s in range(S)), (b, i, j)
            assert (got[:, 4, 5] == 3).all() and (got[:, 4, 57] == 2).all()     # G fixed inside a pair, wobble off: its partner is C


def test_seq_nll_is_rnampnn_scores_byte_for_byte(case):
    from rnampnn.model.decode import score_logits
    for layout in ("padded", "packed"):
        out = _run(case, 0.3, 8, layout)
        if layout == "padded":
            sc = score_logits(case["logits"], mask=case["mask"], seqs=out["seqs"], want=("seq_nll",))
        else:
            sc = score_logits(case["packed"], cu_seqlens=case["cu"], seqs=out["seqs"], want=("seq_nll",))
        assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"]), layout
        assert float(out["seq_nll"][:, 0].abs().max()) == 0.0 and bool((out["seq_nll"][:, 1:] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- 5
def test_layout_batch_seed_dev_and_a_second_call_do_not_change_the_bytes(case):
    h = case["h"]
    base = _run(case, 0.3, 8)
    kw = dict(temperature=0.3, allowed=case["allowed"], partner=case["partner"])
    seed_dev = torch.tensor([SEED], dtype=torch.int64, device="cuda")          # (the bits of a seed below 2^63)
    for other in (_run(case, 0.3, 8, "packed"),
                  design_count(case["logits"], case["counted"], case["lo"], case["hi"], 8, mask=case["mask"], **kw),
                  design_count(case["logits"], case["counted"], case["lo"], case["hi"], 8, mask=case["mask"], seed=0, seed_dev=seed_dev, **kw)):
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in OUTPUTS)
    # RNA 4 alone at its row, in a batch of another B and T whose other rows are empty and hold garbage
    B2, T2, n = 5, 80, LENGTHS[4]
    rng = np.random.RandomState(5)
    logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    partner = rng.randint(-3, 100, size=(B2, T2)).astype(np.int32)
    counted = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    mask = np.zeros((B2, T2), dtype=np.float32)
    logits[4, :n], allowed[4, :n], partner[4, :n], counted[4, :n], mask[4, :n] = (h["logits"][4, :n], h["allowed"][4, :n], h["partner"][4, :n],
                                                                                 h["counted"][4, :n], 1)
    lo, hi = np.full(B2, R.CASE_LO[4], dtype=np.int32), np.full(B2, R.CASE_HI[4], dtype=np.int32)
    one = design_count(logits, counted, lo, hi, 8, mask=mask, temperature=0.3, allowed=allowed, partner=partner)
    assert _bytes(one["seqs"][:, 4, :n]) == _bytes(base["seqs"][:, 4, :n]) and bool((one["seqs"][:, 4, n:] == -1).all())
    assert all(_bytes(one[k][:, 4]) == _bytes(base[k][:, 4]) for k in ("seq_nll", "count"))
    assert all(int(one[k][4]) == int(base[k][4]) for k in ("infeasible", "count_miss"))
    assert bool((one["seqs"][:, :4] == -1).all()) and one["count"][:, :4].abs().sum().item() == 0
    # S = 1 against S = 4
    first = design_count(case["logits"], case["counted"], case["lo"], case["hi"], 8, mask=case["mask"], S=1, **kw)
    assert _bytes(first["seqs"][0]) == _bytes(base["seqs"][0]) and _bytes(first["count_miss"]) == _bytes(base["count_miss"])


def test_the_call_replays_from_a_captured_graph_with_the_same_bytes(case):
    base = _run(case, 0.3, 8)
    out = _outputs(S, len(LENGTHS), T)
    args = (case["logits"], case["counted"], case["lo"], case["hi"], 8)
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], partner=case["partner"], out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        design_count(*args, **kw)                                   # (what a first call sets up happens outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        design_count(*args, **kw)
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_draw_frequencies_follow_the_enumerated_conditioned_joint():
    """A 5-mer with the pair (0, 4) and a reference, the budget [1, 2], temperature 1, 20,000 draws in one launch under a fixed seed: the
    frequency f of every admitted sequence lies within 5 sqrt(p (1 - p) / S) of its probability p under the enumerated joint conditioned
    on the budget (a binomial bound: f is the mean of S independent indicators), and nothing else is drawn."""
    import __graft_entry__ as g
    g.build()
    n, S6 = 5, 20000
    rng = np.random.RandomState(17)
    logits = rng.standard_normal((1, n, 4)).astype(np.float32)
    partner = np.array([[4, -1, -1, -1, 0]], dtype=np.int32)
    ref = np.array([[3, 0, 1, 2, 1]], dtype=np.int32)              # G.U at the pair: with wobble it costs no mutation
    counted = R.mutation_sets(ref)
    out = design_count(logits, counted, [1], [2], 2, mask=np.ones((1, n), dtype=np.float32), S=S6, seed=2024, partner=partner, wobble=True)
    z = logits[0].astype(np.float64)
    joint = {}
    for seq in itertools.product(range(4), repeat=n):
        if (seq[0], seq[4]) in PAIRS[True] and 1 <= sum(int(seq[t] != ref[0, t]) for t in range(n)) <= 2:
            joint[seq] = float(np.exp(sum(z[t, seq[t]] for t in range(n))))
    tot = sum(joint.values())
    got = out["seqs"].cpu().numpy()[:, 0]
    keys, freq = np.unique(got, axis=0, return_counts=True)
    seen = {tuple(int(v) for v in k): c / S6 for k, c in zip(keys, freq)}
    assert set(seen) <= set(joint), "a sequence outside the budget or the structure was drawn"
    assert out["count_miss"].tolist() == [0] and int(out["count"].min()) >= 1 and int(out["count"].max()) <= 2
    worst = 0.0
    for seq, w in joint.items():
        p = w / tot
        sd = np.sqrt(p * (1 - p) / S6)
        worst = max(worst, abs(seen.get(seq, 0.0) - p) / sd)
        assert abs(seen.get(seq, 0.0) - p) <= 5 * sd, (seq, seen.get(seq, 0.0), p)
    print(f"{len(joint)} admitted sequences, the largest deviation {worst:.2f} sd")


# ---------------------------------------------------------------------------------------------------------------- 7
def test_a_budget_below_what_the_structure_forces_holds_k_min():
    """A 24-mer hairpin whose reference violates three of its pairs (A.A, C.C, G.U with wobble off), the budget [0, 1] at cap 1: no count of
    0..1 is reachable, so every draw holds exactly k_min = 3 mutations - one per violated pair - count_miss = k_min - 1 = 2 and the
    structure is satisfied."""
    import __graft_entry__ as g
    g.build()
    n, pairs = 24, [(i, 23 - i) for i in range(8)]
    rng = np.random.RandomState(23)
    logits = (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32)
    partner = np.full((1, n), -1, dtype=np.int32)
    ref = rng.randint(0, 4, size=(1, n)).astype(np.int32)
    for i, j in pairs:
        partner[0, i], partner[0, j] = j, i
        ref[0, j] = R.COMPLEMENT[ref[0, i]]
    ref[0, 1], ref[0, 22] = 0, 0
    ref[0, 3], ref[0, 20] = 2, 2
    ref[0, 6], ref[0, 17] = 3, 1
    counted = R.mutation_sets(ref)
    for temperature in (1.0, 0.1):
        out = design_count(logits, counted, [0], [1], 1, mask=np.ones((1, n), dtype=np.float32), S=8, temperature=temperature, partner=partner,
                           wobble=False)
        plan = R.CountPlan(logits[0], n, temperature, 0, 1, counted[0], 1, None, partner[0], False)
        assert plan.k_min == 3 and plan.at_min
        got = out["seqs"].cpu().numpy()[:, 0]
        assert out["count_miss"].tolist() == [2] and out["count"].tolist() == [[3]] * 8 and out["infeasible"].tolist() == [0]
        assert ((got != ref) .sum(axis=1) == 3).all()
        assert all((int(got[s, i]), int(got[s, j])) in PAIRS[False] for s in range(8) for i, j in pairs)
        free = [t for t in range(n) if partner[0, t] < 0] + [t for i, j in pairs if (i, j) not in ((1, 22), (3, 20), (6, 17)) for t in (i, j)]
        assert (got[:, free] == ref[0, free]).all()                 # every other position keeps the reference
        for s in range(8):                                          # (leaf draws only: rnampnn_design's rule, no split is selected)
            want, margin = plan.draw(SEED, s, 0)
            assert margin <= NEAR or np.array_equal(got[s], want), s


# ---------------------------------------------------------------------------------------------------------------- 8
def test_the_largest_extent_that_fits_at_cap_8_and_one_past_it():
    """One RNA of T_MAX_CAP8 nucleotides at cap 8 (the truncated tree fills the LDS a workgroup may ask for), the budget [0, 8]: the count
    lies in the budget, the draw equals the restatement and the NLL bytes are rnampnn_score's.  One more nucleotide is NotImplementedError
    naming the limit, before any launch."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import design_count_from_logits, mutation_sets, score_logits
    n = T_MAX_CAP8
    rng = np.random.RandomState(11)
    logits = (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32)
    mask = np.ones((1, n), dtype=np.float32)
    partner = np.full((1, n), -1, dtype=np.int32)
    ref = rng.randint(0, 4, size=(1, n)).astype(np.int32)
    for i in range(150):                                           # a long hairpin whose pairs cross the root's boundary
        partner[0, 1900 + i], partner[0, 2300 - i] = 2300 - i, 1900 + i
        ref[0, 2300 - i] = R.COMPLEMENT[ref[0, 1900 + i]]
    ref[0, 1900], ref[0, 2300] = 0, 0                              # one pair the reference violates
    counted = R.mutation_sets(ref)
    lo, hi = np.array([0], dtype=np.int32), np.array([8], dtype=np.int32)
    out = design_count(logits, counted, lo, hi, 8, mask=mask, S=1, partner=partner)
    want, margin, bad, miss, count, _ = R.design_count_ref(logits, [n], 1.0, 1, SEED, counted, lo, hi, 8, None, partner, R.CASE_WOBBLE)
    got = out["seqs"].cpu().numpy()
    assert out["count_miss"].tolist() == miss.tolist() == [0] and out["infeasible"].tolist() == bad.tolist() == [0]
    assert np.array_equal(out["count"].cpu().numpy(), (got != ref[None]).sum(axis=2)) and 1 <= int(out["count"][0, 0]) <= 8
    print(f"T = {n}: margin {margin[0, 0]}, count {int(out['count'][0, 0])}")
    assert margin[0, 0] <= NEAR or np.array_equal(got[0, 0], want[0, 0])
    assert all((int(got[0, 0, 1900 + i]), int(got[0, 0, 2300 - i])) in PAIRS[R.CASE_WOBBLE] for i in range(150))
    sc = score_logits(torch.from_numpy(logits).cuda(), mask=torch.from_numpy(mask).cuda(), seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])
    with pytest.raises(NotImplementedError, match=rf"the limit is 163840 \(T <= {T_MAX_CAP8} at that cap\)"):
        design_count_from_logits(torch.zeros(1, n + 1, 4, device="cuda"), mask=torch.ones(1, n + 1, device="cuda"), n_samples=1, temperature=1.0,
                                 counted=mutation_sets(torch.zeros(1, n + 1, dtype=torch.int64, device="cuda")), window=(0, 8))


# ---------------------------------------------------------------------------------------------------------------- 10
def test_non_finite_logits_and_a_nan_bias_still_give_ids(case):
    """Row 7 (the 257-mer) gets NaN, +inf and -inf logits: ids in 0..3, count = the count of the bytes; every other row keeps its bytes.
    A NaN bias on every row: ids in 0..3 and -1 on padding.  Values only: the kernel raises no error."""
    counted = case["h"]["counted"]
    base = _run(case, 1.0, 8)
    logits = case["logits"].clone()
    logits[7, 40] = float("nan")
    logits[7, 41, 2] = float("inf")
    logits[7, 42, 1] = float("-inf")
    logits[7, 128:140] = float("nan")
    kw = dict(mask=case["mask"], allowed=case["allowed"], partner=case["partner"])
    out = design_count(logits, case["counted"], case["lo"], case["hi"], 8, **kw)
    got = out["seqs"].cpu().numpy()
    assert ((got[:, 7, :257] >= 0) & (got[:, 7, :257] <= 3)).all() and (got[:, 7, 257:] == -1).all()
    assert np.array_equal(out["count"].cpu().numpy(), _count_of(got, counted))
    rows = [b for b in range(len(LENGTHS)) if b != 7]
    assert _bytes(out["seqs"][:, rows]) == _bytes(base["seqs"][:, rows]) and _bytes(out["count"][:, rows]) == _bytes(base["count"][:, rows])
    assert out["infeasible"].tolist() == R.CASE_INFEASIBLE
    for cap in R.CASE_CAPS:
        nan_bias = design_count(case["logits"], case["counted"], case["lo"], case["hi"], cap, bias=torch.full((4,), float("nan")), **kw)
        torch.cuda.synchronize()
        got = nan_bias["seqs"].cpu().numpy()
        assert all(((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all() and (got[:, b, n:] == -1).all() for b, n in enumerate(LENGTHS))
        assert np.array_equal(nan_bias["count"].cpu().numpy(), _count_of(got, counted))


# ---------------------------------------------------------------------------------------------------------------- 9: the Python surface
def test_design_count_from_logits_in_both_layouts_and_with_a_device_window(case):
    from rnampnn.model.decode import design_count_from_logits, mutation_sets
    from rnampnn.utils.constraints import DesignConstraints
    cons = DesignConstraints(case["allowed"], case["partner"], None, R.CASE_WOBBLE)
    counted = mutation_sets(torch.from_numpy(case["h"]["reference"]).cuda())
    assert _bytes(counted) == _bytes(case["counted"])
    lo, hi = np.full(len(LENGTHS), 1, dtype=np.int32), np.full(len(LENGTHS), 5, dtype=np.int32)
    want = design_count(case["logits"], case["counted"], lo, hi, 5, mask=case["mask"], temperature=0.5, seed=77, allowed=case["allowed"],
                        partner=case["partner"])
    kw = dict(n_samples=S, temperature=0.5, seed=77, constraints=cons, counted=counted)
    window = torch.tensor([[1, 5]] * len(LENGTHS), dtype=torch.int32, device="cuda")
    for name, got in (("padded", design_count_from_logits(case["logits"], mask=case["mask"], window=(1, 5), **kw)),
                      ("packed", design_count_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, window=(1, 5), **kw)),
                      ("tensor", design_count_from_logits(case["logits"], mask=case["mask"], window=window, cap=5, **kw))):
        assert len(got) == 5 and [t.dtype for t in got] == [torch.int8, torch.float32, torch.int32, torch.int32, torch.int32]
        for a, k in zip(got, OUTPUTS):
            assert _bytes(a) == _bytes(want[k]), (name, k)
    with pytest.raises(ValueError, match="needs cap"):
        design_count_from_logits(case["logits"], mask=case["mask"], window=window, **kw)


MODEL_LENGTHS = [33, 20, 41]


def _check_budget(out, native, lengths, budget, fixed=None):
    seqs, n_mut, miss = out[0].cpu().numpy(), out[3].cpu().numpy(), out[4].tolist()
    native = native.cpu().numpy()
    for b, n in enumerate(lengths):
        dist = (seqs[:, b, :n] != native[b, :n][None]).sum(axis=1)
        assert np.array_equal(dist, n_mut[:, b]) and (dist <= budget + miss[b]).all(), b
        if miss[b] == 0:
            assert (dist <= budget).all(), b
    for b, t, c in fixed or ():
        assert (seqs[:, b, t] == c).all(), (b, t)


def test_both_models_design_within_a_mutation_budget():
    import __graft_entry__ as g
    g.build()
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.data import pad_batch
    torch.manual_seed(0)
    m = RNAMPNN(precision="f32", **SMALL).cuda().eval()
    items = [(synth.synth_rna(n, i, seed=1), synth.synth_labels(n, i, seed=1)) for i, n in enumerate(MODEL_LENGTHS)]
    native, c, mask, lens = pad_batch(items, pin=False)             # the labels are the native sequence (0 on padding, never read)
    native, c, mask = native.cuda(), c.cuda(), mask.cuda()
    assert len(m.design(c, mask, n_samples=3, temperature=1.0, seed=3)) == 2          # None keeps today's paths and return values
    out = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, mutations=(native, 4))
    assert len(out) == 5 and out[0].shape == (3, 3, max(lens)) and out[2].tolist() == [0, 0, 0] and out[4].tolist() == [0, 0, 0]
    _check_budget(out, native, lens, 4)
    assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    exact = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, mutations=(native, 2, 2))
    assert exact[3].tolist() == [[2, 2, 2]] * 3
    cons = DesignConstraints.from_specs(_specs(), lens, int(mask.shape[1]))
    out = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=cons, mutations=(native, 4))
    # G at 0 and A at 3 of RNA 0 (GNRA), U at 40 of RNA 2: the fixed positions hold whatever they cost
    _check_budget(out, native, lens, 4, fixed=[(0, 0, 3), (0, 3, 0), (2, 40, 1)])
    for (i, j) in ((0, 11), (1, 10), (2, 9), (3, 8)):
        assert all((int(out[0][s, 0, i]), int(out[0][s, 0, j])) in PAIRS[True] for s in range(3))
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    out = r.design(X, mask, n_samples=3, temperature=1.0, seed=5, lengths=MODEL_LENGTHS, mutations=(native, 4))
    assert len(out) == 5 and out[0].shape == (3, 3, max(lens)) and out[4].tolist() == [0, 0, 0]
    _check_budget(out, native, lens, 4)
    assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    out = r.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS, mutations=(native, 1, 4))
    _check_budget(out, native, lens, 4, fixed=[(0, 0, 3), (0, 3, 0), (2, 40, 1)])
    assert len(r.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS)) == 3


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_a_mutation_budget(family, tmp_path):
    """--max-mutations adds the columns mutations and mut_miss and holds every draw to the budget against the structure's own sequence, and
    against --mutate-from; the designs file written without the flag is byte for byte the same before and after."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    own = {rid: open(tmp_path / "data" / "seqs" / f"{rid}.fasta").read().split("\n")[1] for rid in ids}
    parents = {rid: "".join("AUCG"[(("AUCG".index(ch)) + 1) % 4] if k % 5 == 0 else ch for k, ch in enumerate(seq)) for rid, seq in own.items()}
    parents["r0"] = "N" + parents["r0"][1:]                        # an unknown letter never counts
    (tmp_path / "parents.fasta").write_text("".join(f">{rid}\n{seq}\n" for rid, seq in parents.items()))
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--samples", "2", "--temperature", "1.0",
              "--batch-size", "2"]
    quiet = dict(log=lambda *a: None)
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "before.csv")]), **quiet)
    for name, flags, refs, lo in (("own", ["--max-mutations", "3"], own, 0),
                                  ("from", ["--max-mutations", "3", "--min-mutations", "2", "--mutate-from", str(tmp_path / "parents.fasta")], parents, 2)):
        des = str(tmp_path / f"{name}.csv")
        P.run(P.parse(common + ["--designs-out", des] + flags), **quiet)
        d = list(csv.reader(open(des)))
        base = ["pdb_id", "sample", "seq", "nll_per_nt", "recovery"] + (["infeasible"] if family == "rdesign" else [])
        assert d[0] == base + ["mutations", "mut_miss"] and len(d) == 1 + 3 * 2
        for r in d[1:]:
            k = sum(a != b and b in "AUCG" for a, b in zip(r[2], refs[r[0]]))
            assert len(r[2]) == len(refs[r[0]]) and r[-1] == "0" and r[-2] == str(k) and lo <= k <= 3, r
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "after.csv")]), **quiet)
    assert open(tmp_path / "before.csv", "rb").read() == open(tmp_path / "after.csv", "rb").read()
    os.remove(tmp_path / "data" / "seqs" / "r1.fasta")
    if family == "rnampnn":                                        # (the rdesign loader drops a structure without a fasta)
        with pytest.raises(ValueError, match="'r1' has no reference sequence"):
            P.run(P.parse(common + ["--max-mutations", "3"]), **quiet)
