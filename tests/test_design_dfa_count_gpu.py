"""``rnampnn_design_dfa_count`` (csrc/design_dfa_count.hip) on the device: against ``rnampnn_design_dfa`` byte for byte where nothing
counts (the anchor), against the float64 restatement of its contract in tests/_design_dfa_count_ref.py, against a substring scan and a
recount of the written bytes, against the count family's profile where the automaton has one accepting state, against enumerated
probabilities, and for the independence the header states: layout, batch, S, workspace contents, second call, cap.

The batch is the one ``_design_dfa_count_ref`` describes next to ``CASE_LENGTHS``: T = 72, S = 4.  Device and restatement differ by
last-bit exp / log, so a draw whose path has a selection within 1e-8 of a cumulative boundary is left out of the equality check; the share
left out is printed and capped at 5 %, the cap tests/test_design_dfa_count_cpu.py holds the restatement alone to.  ``log_z`` is held to
1e-8 max(1, |value|), the profile tests' tolerance for fp64 sums formed in another order."""
import csv
import ctypes as C
import functools
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

import _design_avoid_ref as AV  # noqa: E402
import _design_dfa_ref as DR  # noqa: E402
import _design_dfa_count_ref as R  # noqa: E402
from _design_case import SMALL, design_outputs, dfa_workspace, raw_design, _bytes, _dev, _write_data, _checkpoint  # noqa: E402
from _design_case import design_dfa as _case_design_dfa  # noqa: E402

LENGTHS, T, S, SEED = R.CASE_LENGTHS, R.CASE_T, R.CASE_S, R.CASE_SEED
B = len(LENGTHS)
NEAR = 1e-8
DFA_OUTPUTS = ("seqs", "seq_nll", "infeasible", "hits", "accepted", "dfa_miss")
OUTPUTS = ("seqs", "seq_nll", "infeasible", "hits", "accepted", "count", "dfa_miss", "count_miss", "log_z")
FURTHER = (("hits", torch.int32, True), ("accepted", torch.int32, True), ("count", torch.int32, True), ("dfa_miss", torch.int32, False),
           ("count_miss", torch.int32, False), ("log_z", torch.float64, False))


def _automaton(name):
    from rnampnn.utils.motifs import as_nested_automaton
    return as_nested_automaton(*R.CASE_AUTOMATA[name])


def _lds_bytes(t):
    return 32 * t + 32 * ((t + 15) // 16) + 1024 * (((t + 15) // 16) | 1) + 4192


def workspace(Bn, Tn, live, cap, fill=None):
    return dfa_workspace("rnampnn_design_dfa_count_workspace_bytes", Bn, Tn, live, max(cap, 1), fill=fill,
                         need=8 * Bn * Tn * live * (min(max(cap, 1), Tn) + 1))


def design_chain(logits, delta, kind, counted, lo, hi, cap, seed=SEED, S=S, ws=None, **kw):
    """The C entry on device tensors (numpy arrays are uploaded; ``kind`` stays on the host) -> dict of its nine outputs."""
    kind = torch.as_tensor(np.ascontiguousarray(kind), dtype=torch.uint8).contiguous()
    live = int(((kind & 1) == 0).sum())
    m, cu = kw.get("mask"), kw.get("cu")
    Bn = int(m.shape[0]) if m is not None else int(cu.shape[0]) - 1
    Tp = int(m.shape[1]) if m is not None else int(kw["T"])
    ws = workspace(Bn, Tp, live, cap) if ws is None else ws
    own = (_dev(delta, torch.uint8), kind, int(kind.numel()), _dev(counted, torch.uint8), _dev(lo, torch.int32), _dev(hi, torch.int32), int(cap),
           ws, C.c_size_t(ws.numel()))
    return raw_design("rnampnn_design_dfa_count", own, FURTHER, logits, seed=seed, S=S, **kw)


design_dfa = functools.partial(_case_design_dfa, seed=SEED, S=S)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = R.case_arrays()
    d = dict(h=h, run={}, auto={name: _automaton(name) for name in R.CASE_AUTOMATA}, side={s: R.case_side(s, h) for s in R.CASE_SIDES})
    for k in ("logits", "mask", "allowed", "bias", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _run(case, name, side, temperature=1.0, layout="padded"):
    """The batch through the kernel, once per (automaton, count side, temperature, layout)."""
    key = (name, side, float(temperature), layout)
    if key not in case["run"]:
        a = case["auto"][name]
        kw = dict(temperature=temperature, allowed=case["allowed"], bias=case["bias"])
        where = dict(mask=case["mask"]) if layout == "padded" else dict(cu=case["cu"], T=T)
        case["run"][key] = design_chain(case["logits"] if layout == "padded" else case["packed"], a.delta, a.kind, *case["side"][side], **where, **kw)
    return case["run"][key]


def _ref(case, name, side, temperature):
    a = case["auto"][name]
    return R.case_ref(name, side, a.delta.numpy(), a.kind.numpy(), temperature)


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    return np.array_equal(inf, np.isinf(got)) and np.array_equal(got[inf], want[inf]) and \
        bool((np.abs(got[~inf] - want[~inf]) <= 1e-8 * np.maximum(1.0, np.abs(want[~inf]))).all())


def _compare(out, ref, label):
    """Draws equal the restatement wherever every margin exceeds NEAR; the flags match exactly; log_z within tolerance."""
    got, want, near = out["seqs"].cpu().numpy(), ref["seqs"], ref["margin"] <= NEAR
    print(f"{label}: {near.mean():.4%} of the {near.size} (sample, RNA) draws left out (a selection within {NEAR} of a boundary)")
    assert near.mean() <= 0.05
    for k in ("infeasible", "dfa_miss", "count_miss"):
        assert out[k].tolist() == ref[k].tolist(), k
    differ = [(s, b) for s in range(near.shape[0]) for b in range(near.shape[1]) if not near[s, b] and not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"
    keep = ~near
    for k in ("hits", "accepted", "count"):
        assert np.array_equal(out[k].cpu().numpy()[keep], ref[k][keep]), k
    print(f"{label}: log_z device {out['log_z'].tolist()} restatement {ref['log_z'].tolist()}")
    assert _close(out["log_z"].cpu().numpy(), ref["log_z"])


# ---------------------------------------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_nothing_counted_is_rnampnn_design_dfa_byte_for_byte(case, name, layout):
    """counted = 0 everywhere, at a cap of T and at count_cap = 0 (one slab per position), each with the window (0, 0): seqs, seq_nll,
    infeasible, hits, accepted and dfa_miss are the bytes of ``rnampnn_design_dfa``; count and count_miss are 0."""
    a = case["auto"][name]
    zero = np.zeros(B, dtype=np.int32)
    where = dict(mask=case["mask"]) if layout == "padded" else dict(cu=case["cu"], T=T)
    lg = case["logits"] if layout == "padded" else case["packed"]
    for temperature in (1.0, 0.3):
        kw = dict(temperature=temperature, allowed=case["allowed"], bias=case["bias"], **where)
        want = design_dfa(lg, a.delta, a.kind, **kw)
        for cap in (T, 0):
            out = design_chain(lg, a.delta, a.kind, np.zeros((B, T), dtype=np.uint8), zero, zero, cap, **kw)
            for k in DFA_OUTPUTS:
                assert _bytes(out[k]) == _bytes(want[k]), (name, layout, temperature, cap, k)
            assert int(out["count_miss"].abs().sum()) == 0 and int(out["count"].abs().sum()) == 0
        assert int(out["dfa_miss"].sum()) < B


# ---------------------------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("side", ["gc", "mut4", "mut2_6"])
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_restatement_and_hold_both_conditions(case, name, side, temperature):
    out, ref = _run(case, name, side, temperature), _ref(case, name, side, temperature)
    _compare(out, ref, f"{name}, {side}, temperature {temperature}")
    assert out["infeasible"].tolist() == R.CASE_INFEASIBLE
    got = out["seqs"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
    # what was written holds the conditions: a substring scan and a recount that know neither the automaton nor the table
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    groups, banned = DR.required_sets(require or ()), AV.expand(avoid or (), max_run)
    counted, lo, hi, cap = case["side"][side]
    hits, accepted, count = (out[k].cpu().numpy() for k in ("hits", "accepted", "count"))
    dmiss, cmiss = out["dfa_miss"].tolist(), out["count_miss"].tolist()
    scan_hits, scan_accepted = case["auto"][name].scan(out["seqs"])
    assert _bytes(scan_hits) == _bytes(out["hits"]) and _bytes(scan_accepted) == _bytes(out["accepted"])
    for b, n in enumerate(LENGTHS):
        K = min(cap, n)
        wl = min(max(int(lo[b]), 0), K)
        wh = max(min(max(int(hi[b]), 0), K), wl)
        for s in range(S):
            assert count[s, b] == R.recount(got[s, b], counted[b]) and hits[s, b] == AV.naive_hits(got[s, b], banned), (s, b)
            if side == "gc":
                assert count[s, b] == int(((got[s, b, :n] == 2) | (got[s, b, :n] == 3)).sum())
            else:
                assert count[s, b] == int((got[s, b, :n] != case["h"]["reference"][b, :n]).sum())
            if dmiss[b]:
                continue
            assert DR.contains_all(got[s, b], groups) and hits[s, b] == 0 and accepted[s, b] == 1, (s, b)
            if cmiss[b] == 0:
                assert wl <= count[s, b] <= wh, (s, b, count[s, b], wl, wh)
            else:
                assert min(abs(count[s, b] - wl), abs(count[s, b] - wh)) == cmiss[b] and not wl <= count[s, b] <= wh
    if side == "gc":
        assert dmiss[5] == int(name == "two_run3") and cmiss[5] == (0 if name == "two_run3" else 3)
        assert name == "two_run3" or (count[:, 5] == 5).all()
    assert dmiss[1:4] == ([0, 0, 0] if name == "run3" else [1, 1, 1])


def test_seq_nll_is_rnampnn_scores_byte_for_byte(case):
    from rnampnn.model.decode import score_logits
    out = _run(case, "two_run3", "gc", 0.3)
    sc = score_logits(case["logits"], mask=case["mask"], seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])


# ---------------------------------------------------------------------------------------------------------------- the count family
def test_one_accepting_state_is_the_count_familys_profile_and_miss(case):
    """An automaton of one live accepting state conditions on nothing: log_z equals ``design_profile_from_logits(...).log_z`` in the G+C
    and the mutation mode within 1e-8 max(1, |value|), and count_miss is ``rnampnn_design_count``'s exactly."""
    from rnampnn.model.decode import design_count_from_logits, design_gc_from_logits, design_profile_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    delta, kind = np.zeros((1, 4), dtype=np.uint8), np.array([2], dtype=np.uint8)
    cons = DesignConstraints(case["allowed"], None, case["bias"], True)
    ref = torch.from_numpy(case["h"]["reference"].astype(np.int32)).cuda()
    kw = dict(mask=case["mask"], temperature=0.7, constraints=cons)
    for side, profile_kw in (("gc", dict(gc_content=(0.45, 0.60))), ("mut4", dict(mutations=(ref, 0, 4))), ("mut2_6", dict(mutations=(ref, 2, 6)))):
        counted, lo, hi, cap = case["side"][side]
        out = design_chain(case["logits"], delta, kind, counted, lo, hi, cap, mask=case["mask"], temperature=0.7, allowed=case["allowed"],
                           bias=case["bias"])
        prof = design_profile_from_logits(case["logits"], **kw, **profile_kw)
        print(f"{side}: log_z chain {out['log_z'].tolist()} profile {prof.log_z.tolist()}")
        assert _close(out["log_z"].cpu().numpy(), prof.log_z.cpu().numpy()), side
        if side == "gc":
            miss = design_gc_from_logits(case["logits"], n_samples=1, seed=SEED, gc_content=(0.45, 0.60), **kw)[4]
        else:
            w = (int(lo[0]), int(hi[0]))
            miss = design_count_from_logits(case["logits"], n_samples=1, seed=SEED, counted=torch.from_numpy(counted).cuda(), window=w, cap=cap, **kw)[4]
        assert out["count_miss"].tolist() == miss.tolist() == prof.miss.tolist() and int(out["dfa_miss"].sum()) == 0, side
    assert out["count_miss"].tolist()[1] == 0


# ---------------------------------------------------------------------------------------------------------------- frequencies
@pytest.mark.parametrize("side", ["gc", "mut"])
def test_4096_draws_of_a_5_mer_follow_the_enumerated_probabilities(side):
    """Require GA, avoid CC, no run longer than 2, T = n = 5, temperature 1, G+C in 2..3 or 1..3 mutations: every admitted sequence's
    frequency lies within 5 binomial standard deviations of its brute-force probability (the joint over the sequences that hold both
    conditions by substring scan and recount, renormalised); no sequence outside the conditions is ever drawn.  S = 4096 also walks
    sixteen chunks of 256 samples."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.motifs import DesignAutomaton
    auto = DesignAutomaton.from_motifs(["GA"], ["CC"], 2)
    N, n = 4096, 5
    rng = np.random.RandomState(8)
    logits = (0.25 * rng.standard_normal((1, n, 4))).astype(np.float32)
    reference = rng.randint(0, 4, size=(1, n))
    counted = np.full((1, n), 12, dtype=np.uint8) if side == "gc" else (15 ^ (1 << reference)).astype(np.uint8)
    lo, hi = ((2, 3) if side == "gc" else (1, 3))
    out = design_chain(logits, auto.delta, auto.kind, counted, np.array([lo], dtype=np.int32), np.array([hi], dtype=np.int32), n if side == "gc" else hi,
                       S=N, seed=91, mask=np.ones((1, n), dtype=np.float32))
    assert out["dfa_miss"].tolist() == [0] and out["count_miss"].tolist() == [0] and int(out["accepted"].sum()) == N
    groups, banned = DR.required_sets(["GA"]), AV.expand(["CC"], 2)
    z = logits[0].astype(np.float64)
    logp = np.full(4 ** n, -np.inf)
    for i, seq in enumerate(itertools.product(range(4), repeat=n)):
        if DR.contains_all(seq, groups) and AV.naive_hits(seq, banned) == 0 and lo <= R.recount(seq, counted[0]) <= hi:
            logp[i] = sum(z[t, seq[t]] for t in range(n))
    total = R.lse(logp[np.isfinite(logp)])
    assert abs(float(out["log_z"][0]) - total) <= 1e-8 * max(1.0, abs(total))
    p = np.exp(logp - total)
    got = out["seqs"].cpu().numpy()[:, 0].astype(np.int64)
    counts = np.bincount((got * 4 ** np.arange(n - 1, -1, -1)).sum(axis=1), minlength=4 ** n)
    assert (counts[p == 0] == 0).all()
    sd = np.sqrt(N * p * (1 - p))
    dev = np.abs(counts - N * p)[p > 0] / sd[p > 0]
    print(f"{side}: {int((p > 0).sum())} admitted sequences, N p from {N * p[p > 0].min():.2f} to {N * p.max():.2f}; largest deviation {dev.max():.2f} sd")
    assert dev.max() <= 5.0


# ---------------------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("side", ["gc", "mut2_6"])
def test_layout_second_call_workspace_padding_and_graph_replay_give_identical_bytes(case, side):
    a = case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", side, 0.3)
    counted, lo, hi, cap = case["side"][side]
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
    rng = np.random.RandomState(3)
    pad = case["h"]["mask"] == 0
    g_logits, g_allowed, g_bias, g_counted = (x.copy() for x in (case["h"]["logits"], case["h"]["allowed"], case["h"]["bias"], counted))
    g_logits[pad], g_bias[pad] = np.nan, 1e30
    g_allowed[pad], g_counted[pad] = rng.randint(0, 256, size=int(pad.sum())), rng.randint(0, 256, size=int(pad.sum()))
    seed_dev = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    others = dict(packed=_run(case, "gnra_run3", side, 0.3, "packed"), second=design_chain(case["logits"], a.delta, a.kind, counted, lo, hi, cap, **kw),
                  seed_dev=design_chain(case["logits"], a.delta, a.kind, counted, lo, hi, cap, seed=0, seed_dev=seed_dev, **kw),
                  ws_ff=design_chain(case["logits"], a.delta, a.kind, counted, lo, hi, cap, ws=workspace(B, T, a.n_live, cap, fill=0xFF), **kw),
                  ws_larger=design_chain(case["logits"], a.delta, a.kind, counted, lo, hi, cap, ws=workspace(B + 1, T, a.n_live, cap, fill=0x7F), **kw),
                  garbage=design_chain(g_logits, a.delta, a.kind, g_counted, lo, hi, cap, mask=case["mask"], temperature=0.3, allowed=g_allowed,
                                       bias=g_bias))
    for label, other in others.items():
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in OUTPUTS), label
    out = design_outputs(FURTHER, S, B, T)
    ws = workspace(B, T, a.n_live, cap, fill=0xFF)
    dev = [_dev(a.delta, torch.uint8), _dev(counted, torch.uint8), _dev(lo, torch.int32), _dev(hi, torch.int32)]    # (nothing is uploaded while the stream captures)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        design_chain(case["logits"], dev[0], a.kind, dev[1], dev[2], dev[3], cap, ws=ws, out=out, **kw)
    for t in out.values():
        t.fill_(-7)
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS)


def test_an_rna_alone_equals_its_row_in_the_batch(case):
    """RNA 4 (fixed and IUPAC positions) and RNA 7 (64 nt) alone at their row, in a batch of another B and T whose other rows are empty
    and hold garbage."""
    h, a = case["h"], case["auto"]["two_run3"]
    B2, T2 = 9, 80
    rng = np.random.RandomState(5)
    for side in ("gc", "mut4"):
        base = _run(case, "two_run3", side, 0.3)
        counted, lo, hi, cap = case["side"][side]
        for b in (4, 7):
            n = LENGTHS[b]
            logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
            allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
            cs = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
            bias = rng.standard_normal((B2, T2, 4)).astype(np.float32)
            mask = np.zeros((B2, T2), dtype=np.float32)
            lo2, hi2 = rng.randint(-5, 50, size=B2).astype(np.int32), rng.randint(-5, 50, size=B2).astype(np.int32)
            logits[b, :n], allowed[b, :n], bias[b, :n], cs[b, :n], mask[b, :n] = h["logits"][b, :n], h["allowed"][b, :n], h["bias"][b, :n], counted[b, :n], 1
            lo2[b], hi2[b] = lo[b], hi[b]
            one = design_chain(logits, a.delta, a.kind, cs, lo2, hi2, T2 if side == "gc" else cap, mask=mask, allowed=allowed, bias=bias, temperature=0.3)
            assert _bytes(one["seqs"][:, b, :n]) == _bytes(base["seqs"][:, b, :n]) and bool((one["seqs"][:, b, n:] == -1).all()), (side, b)
            for k in ("seq_nll", "hits", "accepted", "count"):
                assert _bytes(one[k][:, b]) == _bytes(base[k][:, b]), (side, b, k)
            for k in ("infeasible", "dfa_miss", "count_miss", "log_z"):
                assert _bytes(one[k][b]) == _bytes(base[k][b]), (side, b, k)
            assert bool((one["seqs"][:, [x for x in range(B2) if x != b]] == -1).all())


def test_4_samples_are_a_prefix_of_7(case):
    a = case["auto"]["gnra_run3"]
    for side in ("gc", "mut2_6"):
        base = _run(case, "gnra_run3", side, 1.0)
        out = design_chain(case["logits"], a.delta, a.kind, *case["side"][side], S=7, mask=case["mask"], temperature=1.0, allowed=case["allowed"],
                           bias=case["bias"])
        for k in ("seqs", "seq_nll", "hits", "accepted", "count"):
            assert _bytes(out[k][:4]) == _bytes(base[k]), (side, k)
        for k in ("infeasible", "dfa_miss", "count_miss", "log_z"):
            assert _bytes(out[k]) == _bytes(base[k]), (side, k)


def test_the_outputs_do_not_depend_on_the_cap(case):
    """Budgets whose window lies within the cap and is reachable: cap = hi, hi + 3 and T give the same bytes (the rows whose window is not
    reachable, or that miss the motifs, are left out: their target may move with the cap)."""
    a = case["auto"]["gnra_run3"]
    for side in ("mut4", "mut2_6"):
        counted, lo, hi, cap = case["side"][side]
        base = _run(case, "gnra_run3", side, 0.3)
        keep = [b for b in range(B) if not int(base["dfa_miss"][b]) and not int(base["count_miss"][b])]
        assert len(keep) >= 4
        for other in (cap + 3, T, 100000):
            out = design_chain(case["logits"], a.delta, a.kind, counted, lo, hi, other, mask=case["mask"], temperature=0.3, allowed=case["allowed"],
                               bias=case["bias"])
            for k in ("seqs", "seq_nll", "hits", "accepted", "count"):
                assert _bytes(out[k][:, keep]) == _bytes(base[k][:, keep]), (side, other, k)
            for k in ("infeasible", "dfa_miss", "count_miss", "log_z"):
                assert _bytes(out[k][keep]) == _bytes(base[k][keep]), (side, other, k)


def test_256_states_read_the_slab_from_the_workspace(case):
    """An automaton of 256 live states under a G+C window at T = 72: 16 L (cap + 1) bytes = 299,008 do not fit LDS, so the slab of t + 1 is
    read from the workspace; the draws equal the restatement and hold both long motifs inside the window."""
    from rnampnn.utils.motifs import DesignAutomaton
    long = "GGAGGCUUCGAAUUCGCAUGCCAUGGUACCUAGCUAGGAUCCGAUAUCAAGCUUGCGGCCGCUCGAGACGUCUGCAGCCCGGGAGAUCUGUCGACACUAGUUCUAGA"
    auto = DesignAutomaton.from_motifs([long[:26], long[50:89]])
    assert auto.n_live == 256 and 16 * 256 * (T + 1) + _lds_bytes(T) > 163840
    n = 70
    logits = (3.0 * np.random.RandomState(12).standard_normal((1, T, 4))).astype(np.float32)
    mask = np.zeros((1, T), dtype=np.float32)
    mask[0, :n] = 1
    counted = np.full((1, T), 12, dtype=np.uint8)
    lo, hi = R.gc_window([n])
    out = design_chain(logits, auto.delta, auto.kind, counted, lo, hi, T, S=2, mask=mask, temperature=0.3)
    ref = R.design_dfa_count_ref(logits, [n], 0.3, 2, SEED, auto.delta.numpy(), auto.kind.numpy(), counted, lo, hi, T)
    _compare(out, ref, "256 states, G+C window")
    got = out["seqs"].cpu().numpy()
    assert out["dfa_miss"].tolist() == [0] and out["accepted"].tolist() == [[1], [1]]
    assert all(DR.contains_all(got[s, 0], DR.required_sets((long[:26], long[50:89]))) and int(lo[0]) <= R.recount(got[s, 0], counted[0]) <= int(hi[0])
               for s in range(2))


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_partner_workspace_and_the_lds_limit_are_refused_before_any_launch(case):
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    a = case["auto"]["gnra_run3"]
    lg, m = case["logits"], case["mask"]
    counted, lo, hi, cap = (_dev(x) if isinstance(x, np.ndarray) else x for x in case["side"]["mut4"])
    delta, kind = a.delta.cuda(), a.kind.clone()
    ws = workspace(B, T, a.n_live, cap)
    out = design_outputs(FURTHER, S, B, T)
    partner = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    for t in out.values():
        t.fill_(-7)
    keep = {k: t.clone() for k, t in out.items()}

    def call(logits=lg, mask=m, Bn=B, Tn=T, delta=delta, kind=kind, n_states=a.n_states, counted=counted, lo=lo, cap=cap, partner=None, ws=ws,
             ws_bytes=None, outs=True):
        return _native.lib().rnampnn_design_dfa_count(_ptr(logits), Bn * Tn, _ptr(mask), None, Bn, Tn, 1.0, S, C.c_uint64(SEED), None,
                                                      None, _ptr(partner), 1, None, 0, _ptr(delta), _ptr(kind), n_states, _ptr(counted), _ptr(lo),
                                                      _ptr(hi), cap, _ptr(ws), C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes),
                                                      *[_ptr(out[k]) if outs else None for k in OUTPUTS], _stream(lg.device))
    BAD, UNSUPPORTED = 1, 2
    bad = dict(null_delta=call(delta=None), null_kind=call(kind=None), states257=call(n_states=257), null_counted=call(counted=None),
               null_lo=call(lo=None), negative_cap=call(cap=-1), null_workspace=call(ws=None, ws_bytes=ws.numel()),
               small_workspace=call(ws_bytes=ws.numel() - 1))
    assert bad == {k: BAD for k in bad}, bad
    assert call(partner=partner) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match="base pairs .* are not built together with an automaton.*4\\^depth"):
        _native.check(call(partner=partner))
    with pytest.raises(ValueError, match=rf"the workspace is too small \({ws.numel() - 1} bytes\).*needs {ws.numel()}"):
        _native.check(call(ws_bytes=ws.numel() - 1))
    with pytest.raises(ValueError, match="null counted, count_lo or count_hi"):
        _native.check(call(counted=None))
    n = 1617
    assert _lds_bytes(1616) == 162560 and _lds_bytes(n) == 164672
    big_l, big_m = torch.zeros(1, n, 4, device="cuda"), torch.ones(1, n, device="cuda")
    big_c, big_ws = torch.zeros(1, n, dtype=torch.uint8, device="cuda"), workspace(1, n, a.n_live, cap)
    with pytest.raises(NotImplementedError, match=rf"T = {n} needs 164672 bytes of LDS.*the limit is 163840 \(T <= 1616;"):
        _native.check(call(logits=big_l, mask=big_m, Bn=1, Tn=n, counted=big_c, ws=big_ws))
    assert call(outs=False) == 0                                    # nothing asked for: no launch
    torch.cuda.synchronize()
    assert all(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)                 # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
MODEL_LENGTHS = [33, 20, 41]


def test_design_dfa_count_from_logits_in_both_layouts(case):
    from rnampnn.model.decode import check_mutations, design_dfa_count_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    a = case["auto"]["gnra_run3"]
    cons = DesignConstraints(case["allowed"], None, case["bias"], True)
    ref = torch.from_numpy(case["h"]["reference"].astype(np.int32)).cuda()
    kw = dict(n_samples=S, temperature=0.3, seed=SEED, constraints=cons)
    for side, count_kw in (("gc", dict(gc_content=(0.45, 0.60))), ("mut2_6", dict(mutations=check_mutations((ref, 2, 6))))):
        want = _run(case, "gnra_run3", side, 0.3)
        for name, got in (("padded", design_dfa_count_from_logits(case["logits"], mask=case["mask"], require=a, **count_kw, **kw)),
                          ("packed", design_dfa_count_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, require=a, **count_kw, **kw)),
                          ("strings", design_dfa_count_from_logits(case["logits"], mask=case["mask"], require=["GNRA"], max_run=3, **count_kw, **kw))):
            assert len(got) == 9 and [t.dtype for t in got] == [torch.int8, torch.float32] + [torch.int32] * 6 + [torch.float64]
            for t, k in zip(got, OUTPUTS):
                assert _bytes(t) == _bytes(want[k]), (side, name, k)
    run3 = design_dfa_count_from_logits(case["logits"], mask=case["mask"], max_run=3, gc_content=(0.45, 0.60), **kw)
    assert all(_bytes(t) == _bytes(_run(case, "run3", "gc", 0.3)[k]) for t, k in zip(run3, OUTPUTS))


def _scan_rows(seqs, lens, groups, banned):
    return all(DR.contains_all(row[:n], groups) and AV.naive_hits(row[:n], banned) == 0 for plane in seqs for row, n in zip(plane, lens))


def test_both_models_design_with_combine_chain():
    import __graft_entry__ as g
    g.build()
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    from rnampnn.utils.data import pad_batch
    torch.manual_seed(0)
    m = RNAMPNN(precision="f32", **SMALL).cuda().eval()
    items = [(synth.synth_rna(n, i, seed=1), synth.synth_labels(n, i, seed=1)) for i, n in enumerate(MODEL_LENGTHS)]
    _, c, mask, lens = pad_batch(items, pin=False)
    c, mask = c.cuda(), mask.cuda()
    groups, banned = DR.required_sets(["GNRA"]), AV.expand(["GAAUUC", "AAAA", "UUUU", "CCCC", "GGGG"])
    kw = dict(n_samples=4, temperature=1.0, seed=3)
    words = dict(require=["GNRA"], avoid=["GAAUUC", "AAAA", "UUUU", "CCCC", "GGGG"])
    assert len(m.design(c, mask, **kw)) == 2                       # None keeps today's paths and return values
    out = m.design(c, mask, gc_content=(0.4, 0.6), combine="chain", **words, **kw)
    assert len(out) == 9 and out[0].shape == (4, 3, max(lens)) and out[6].tolist() == [0, 0, 0] and out[7].tolist() == [0, 0, 0]
    got = out[0].cpu().numpy()
    assert _scan_rows(got, lens, groups, banned) and int(out[3].abs().sum()) == 0 and int(out[4].sum()) == 12
    for b, n in enumerate(lens):
        gc = ((got[:, b, :n] == 2) | (got[:, b, :n] == 3)).sum(axis=1)
        assert gc.tolist() == out[5][:, b].tolist() and (gc >= np.ceil(0.4 * n - 1e-6)).all() and (gc <= np.floor(0.6 * n + 1e-6)).all()
    assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    native = torch.full((3, max(lens)), -1, dtype=torch.int32)
    for i, (_, lab) in enumerate(items):
        native[i, :lens[i]] = torch.as_tensor(lab)
    out = m.design(c, mask, mutations=(native.cuda(), 6), combine="chain", avoid=["GAAUUC"], **kw)
    got = out[0].cpu().numpy()
    for b, n in enumerate(lens):
        mut = (got[:, b, :n] != native[b, :n].numpy()).sum(axis=1)
        assert mut.tolist() == out[5][:, b].tolist() and (mut <= 6).all()
    assert _scan_rows(got, lens, [], AV.expand(["GAAUUC"])) and out[6].tolist() == [0, 0, 0] and out[7].tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="avoid together with gc_content is not built"):
        m.design(c, mask, gc_content=(0.4, 0.6), avoid=["GGGG"], **kw)
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    out = r.design(X, mask, n_samples=4, temperature=1.0, seed=5, lengths=MODEL_LENGTHS, gc_content=(0.4, 0.6), combine="chain", **words)
    got = out[0].cpu().numpy()
    assert len(out) == 9 and _scan_rows(got, lens, groups, banned) and out[6].tolist() == [0, 0, 0] and out[7].tolist() == [0, 0, 0]
    for b, n in enumerate(lens):
        gc = ((got[:, b, :n] == 2) | (got[:, b, :n] == 3)).sum(axis=1)
        assert gc.tolist() == out[5][:, b].tolist() and (gc >= np.ceil(0.4 * n - 1e-6)).all() and (gc <= np.floor(0.6 * n + 1e-6)).all()
    assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    assert len(r.design(X, mask, n_samples=2, temperature=1.0, seed=5, lengths=MODEL_LENGTHS)) == 3


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_combine_chain(family, tmp_path):
    """--combine chain --max-run 3 --require GNRA --gc-content 0.4:0.6 adds the columns motif_hits, required_found, require_miss, gc_count
    and gc_miss; every written design holds a GNRA, no run longer than 3 and a G+C count inside the window, by a scan of the text."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    des = str(tmp_path / "chain.csv")
    P.run(P.parse(["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--samples", "3", "--temperature", "1.0",
                   "--batch-size", "2", "--designs-out", des, "--combine", "chain", "--max-run", "3", "--require", "GNRA", "--gc-content", "0.4:0.6"]),
          log=lambda *a: None)
    d = list(csv.reader(open(des)))
    head = ["pdb_id", "sample", "seq", "nll_per_nt", "recovery"] + (["infeasible"] if family == "rdesign" else [])
    assert d[0] == head + ["motif_hits", "required_found", "require_miss", "gc_count", "gc_miss"] and len(d) == 1 + 3 * 3
    for r in d[1:]:
        n = lens[ids.index(r[0])]
        gc = sum(ch in "CG" for ch in r[2])
        assert len(r[2]) == n and r[-5:] == ["0", "1", "0", str(gc), "0"], r
        assert np.ceil(0.4 * n - 1e-6) <= gc <= np.floor(0.6 * n + 1e-6), r
        assert any(w in r[2] for w in ("GAAA", "GUAA", "GCAA", "GGAA", "GAGA", "GUGA", "GCGA", "GGGA")), r
        assert not any(w in r[2] for w in ("AAAA", "UUUU", "CCCC", "GGGG")), r
