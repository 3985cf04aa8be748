"""``rnampnn_design_dfa`` (csrc/design_dfa.hip) on the device: against ``rnampnn_design_avoid`` byte for byte where every live state
accepts (the anchor), against the float64 restatement of its contract in tests/_design_dfa_ref.py, against a substring scan of the written
bytes, against enumerated probabilities, and on the ground the LDS-table entries do not reach (T = 1200 above 64 live states, 256 states).

The batch is the one ``_design_dfa_ref`` describes next to ``CASE_LENGTHS``.  Device and restatement differ by last-bit exp / log, so a
draw whose path has a selection within 1e-8 of a cumulative boundary is left out of the equality check; the share left out is printed and
capped at 5 %, the cap tests/test_design_dfa_cpu.py holds the restatement alone to."""
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
import _design_dfa_ref as R  # noqa: E402
from _design_case import SMALL, design_outputs, dfa_workspace, raw_design, _bytes, _dev, _write_data, _checkpoint  # noqa: E402
from _design_case import design_dfa as _case_design_dfa  # noqa: E402

LENGTHS, T, S, SEED = R.CASE_LENGTHS, R.CASE_T, R.CASE_S, R.CASE_SEED
NEAR = 1e-8
SHARED = ("seqs", "seq_nll", "infeasible", "hits")
OUTPUTS = ("seqs", "seq_nll", "infeasible", "hits", "accepted", "dfa_miss")
FURTHER = (("hits", torch.int32, True), ("accepted", torch.int32, True), ("dfa_miss", torch.int32, False))
FEASIBLE = [b for b in range(len(LENGTHS)) if not R.CASE_MISS[b]]
LONG = "GGAGGCUUCGAAUUCGCAUGCCAUGGUACCUAGCUAGGAUCCGAUAUCAAGCUUGCGGCCGCUCGAGACGUCUGCAGCCCGGGAGAUCUGUCGACACUAGUUCUAGA"
T_EDGE = 1587                                                      # the largest padded extent: 163,840 of 163,840 bytes of LDS


def _automaton(name):
    from rnampnn.utils.motifs import DesignAutomaton
    return DesignAutomaton.from_motifs(*R.CASE_AUTOMATA[name])


def _lds_bytes(t):
    return 32 * t + 16 * ((t + 15) // 16) + 1024 * (((t + 15) // 16) | 1) + 8032


def workspace(B, T, live, fill=None):
    return dfa_workspace("rnampnn_design_dfa_workspace_bytes", B, T, live, fill=fill)


design_dfa = functools.partial(_case_design_dfa, seed=SEED, S=S)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = R.case_arrays()
    d = dict(h=h, run={}, auto={name: _automaton(name) for name in R.CASE_AUTOMATA})
    for k in ("logits", "mask", "allowed", "bias", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _run(case, name, temperature=1.0, layout="padded"):
    """The batch through the kernel, once per (automaton, temperature, layout)."""
    key = (name, float(temperature), layout)
    if key not in case["run"]:
        a = case["auto"][name]
        kw = dict(temperature=temperature, allowed=case["allowed"], bias=case["bias"])
        if layout == "padded":
            case["run"][key] = design_dfa(case["logits"], a.delta, a.kind, mask=case["mask"], **kw)
        else:
            case["run"][key] = design_dfa(case["packed"], a.delta, a.kind, cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _ref(case, name, temperature):
    a = case["auto"][name]
    return R.case_ref(name, a.delta.numpy(), a.kind.numpy(), temperature)


def _compare(out, ref, label):
    """Draws equal the restatement wherever every margin exceeds NEAR; the flags match exactly.  -> the share left out."""
    got, want, near = out["seqs"].cpu().numpy(), ref["seqs"], ref["margin"] <= NEAR
    print(f"{label}: {near.mean():.4%} of the {near.size} (sample, RNA) draws left out (a selection within {NEAR} of a boundary)")
    assert near.mean() <= 0.05
    assert out["dfa_miss"].tolist() == ref["dfa_miss"].tolist() and out["infeasible"].tolist() == ref["infeasible"].tolist()
    Sn, Bn = near.shape
    differ = [(s, b) for s in range(Sn) for b in range(Bn) if not near[s, b] and not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"
    keep = ~near
    assert np.array_equal(out["hits"].cpu().numpy()[keep], ref["hits"][keep]) and np.array_equal(out["accepted"].cpu().numpy()[keep], ref["accepted"][keep])
    return near.mean()


# ---------------------------------------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("name", sorted(AV.CASE_AUTOMATA))
def test_every_live_state_accepting_is_rnampnn_design_avoid_byte_for_byte(name):
    """The avoid entry's own batch and automata (17, 9 and 64 states), kind = "every live state accepts": seqs, seq_nll, infeasible, hits
    and the miss flag are the bytes of ``design_avoid_from_logits``; accepted is 1 wherever the draw entered no dead state's end."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import design_avoid_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.motifs import MotifAutomaton
    h = AV.case_arrays()
    motifs, max_run = AV.CASE_AUTOMATA[name]
    auto = MotifAutomaton.from_motifs(motifs, max_run=max_run)
    kind = np.array([1 if (auto.terminal >> a) & 1 else 2 for a in range(auto.n_states)], dtype=np.uint8)
    dev = {k: torch.from_numpy(h[k]).cuda() for k in ("logits", "mask", "allowed", "bias")}
    cons = DesignConstraints(dev["allowed"], None, dev["bias"], True)
    for temperature in (1.0, 0.3):
        want = design_avoid_from_logits(dev["logits"], mask=dev["mask"], n_samples=AV.CASE_S, temperature=temperature, seed=AV.CASE_SEED,
                                        constraints=cons, avoid=auto)
        out = design_dfa(dev["logits"], auto.delta, kind, seed=AV.CASE_SEED, S=AV.CASE_S, mask=dev["mask"], temperature=temperature,
                         allowed=dev["allowed"], bias=dev["bias"])
        for k, t in zip(SHARED + ("dfa_miss",), want):
            assert _bytes(out[k]) == _bytes(t), (name, temperature, k)
        assert out["dfa_miss"].tolist() == AV.CASE_MISS and bool((out["hits"][:, 4] > 0).all())
        feasible = [b for b in range(len(AV.CASE_MISS)) if not AV.CASE_MISS[b]]
        assert bool((out["accepted"][:, feasible] == 1).all())


# ---------------------------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_restatement_and_hold_every_required_motif(case, name, temperature):
    out, ref = _run(case, name, temperature), _ref(case, name, temperature)
    _compare(out, ref, f"{name}, temperature {temperature}")
    assert out["dfa_miss"].tolist() == R.CASE_MISS and out["infeasible"].tolist() == R.CASE_INFEASIBLE
    got = out["seqs"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
    # the flags are the recount of the written bytes: the user-facing scan on the device, and a substring comparison on the host
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    groups, banned = R.required_sets(require), R.expand(avoid, max_run)
    hits, accepted = case["auto"][name].scan(out["seqs"])
    assert _bytes(hits) == _bytes(out["hits"]) and _bytes(accepted) == _bytes(out["accepted"])
    count = out["hits"].cpu().numpy()
    assert np.array_equal(count, np.array([[AV.naive_hits(row, banned) for row in plane] for plane in got], dtype=np.int32))
    assert (count[:, FEASIBLE] == 0).all() and bool((out["accepted"][:, FEASIBLE] == 1).all())
    assert all(R.contains_all(got[s, b], groups) for s in range(S) for b in FEASIBLE)
    assert not bool(out["accepted"][:, [b for b in range(len(LENGTHS)) if R.CASE_MISS[b]]].any())
    if max_run == 3:
        assert (count[:, 4] > 0).all()                              # the RNA fixed to A: its free draws run through dead states


def test_seq_nll_is_rnampnn_scores_byte_for_byte_in_both_layouts(case):
    from rnampnn.model.decode import score_logits
    padded, packed = _run(case, "two_run3", 0.3), _run(case, "two_run3", 0.3, "packed")
    assert all(_bytes(padded[k]) == _bytes(packed[k]) for k in OUTPUTS)
    sc = score_logits(case["logits"], mask=case["mask"], seqs=padded["seqs"], want=("seq_nll",))
    assert _bytes(padded["seq_nll"]) == _bytes(sc["seq_nll"])
    sc = score_logits(case["packed"], cu_seqlens=case["cu"], seqs=packed["seqs"], want=("seq_nll",))
    assert _bytes(packed["seq_nll"]) == _bytes(sc["seq_nll"])


# ---------------------------------------------------------------------------------------------------------------- frequencies
def test_20000_draws_of_a_6_mer_follow_the_enumerated_probabilities():
    """Require GA, no run longer than 2, T = n = 6, temperature 1: every admitted sequence's count lies within 5 binomial standard
    deviations of N p, p from the restatement's ``path_logprob`` (which the CPU test pins to the enumerated joint); no draw lies outside
    the language.  Logits 0.25 * randn keep every p within a small factor of the mean, so N p stays where the bound means something."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.motifs import DesignAutomaton
    auto = DesignAutomaton.from_motifs(["GA"], max_run=2)
    N, n = 20000, 6
    logits = (0.25 * np.random.RandomState(4).standard_normal((1, n, 4))).astype(np.float32)
    out = design_dfa(logits, auto.delta, auto.kind, S=N, seed=77, mask=np.ones((1, n), dtype=np.float32))
    assert out["dfa_miss"].tolist() == [0] and int(out["hits"].abs().sum()) == 0 and int(out["accepted"].sum()) == N
    got = out["seqs"].cpu().numpy()[:, 0].astype(np.int64)
    counts = np.bincount((got * 4 ** np.arange(n - 1, -1, -1)).sum(axis=1), minlength=4 ** n)
    plan = R.DfaPlan(logits[0], n, 1.0, auto.delta.numpy(), auto.kind.numpy())
    p = np.array([np.exp(plan.path_logprob(seq)) for seq in itertools.product(range(4), repeat=n)])
    assert abs(p.sum() - 1.0) < 1e-12 and (counts[p == 0] == 0).all()
    sd = np.sqrt(N * p * (1 - p))
    dev = np.abs(counts - N * p)[p > 0] / sd[p > 0]
    print(f"{int((p > 0).sum())} admitted sequences, N p from {N * p[p > 0].min():.2f} to {N * p.max():.2f}; largest deviation {dev.max():.2f} sd")
    assert dev.max() <= 5.0


# ---------------------------------------------------------------------------------------------------------------- new ground
def _single(n, name_or_auto, S=2, temperature=1.0, seed=11, raise_g=0.0):
    auto = _automaton(name_or_auto) if isinstance(name_or_auto, str) else name_or_auto
    rng = np.random.RandomState(seed)
    logits = (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32)
    logits[0, :, 3] += raise_g
    out = design_dfa(logits, auto.delta, auto.kind, S=S, mask=np.ones((1, n), dtype=np.float32), temperature=temperature)
    ref = R.design_dfa_ref(logits, [n], temperature, S, SEED, auto.delta.numpy(), auto.kind.numpy())
    return auto, logits, out, ref


def test_t_1200_with_73_live_states():
    """Far past the LDS-table entry's reach (T <= 290 at 64 live states): one RNA of 1200 nucleotides with G raised under two required
    5-mers and no run longer than 3; the draws equal the restatement, hold both motifs and no run, and the NLL bytes are rnampnn_score's."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import score_logits
    auto, logits, out, ref = _single(1200, "two_run3", raise_g=6.0)
    assert auto.n_live == 73 and out["dfa_miss"].tolist() == [0]
    _compare(out, ref, "T = 1200, 73 live states")
    got = out["seqs"].cpu().numpy()
    groups, banned = R.required_sets(("GGAGG", "CUUCG")), R.expand((), 3)
    assert all(R.contains_all(got[s, 0], groups) and AV.naive_hits(got[s, 0], banned) == 0 for s in range(2))
    assert out["hits"].tolist() == [[0], [0]] and out["accepted"].tolist() == [[1], [1]]
    sc = score_logits(torch.from_numpy(logits).cuda(), mask=torch.ones(1, 1200, device="cuda"), seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])


def test_an_automaton_of_256_states_at_t_300():
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.motifs import DesignAutomaton
    auto = DesignAutomaton.from_motifs([LONG[:26], LONG[50:89]])
    assert auto.n_states == 256 and auto.n_live == 256
    _, _, out, ref = _single(300, auto, temperature=0.3)
    _compare(out, ref, "256 states, T = 300")
    got = out["seqs"].cpu().numpy()
    assert out["accepted"].tolist() == [[1], [1]] and all(R.contains_all(got[s, 0], R.required_sets((LONG[:26], LONG[50:89]))) for s in range(2))


def test_the_lds_edge_is_accepted_on_one_side_and_refused_on_the_other():
    """bytes(T) = 32 T + 16 ceil(T / 16) + 1024 (ceil(T / 16) | 1) + 8032 for every automaton: T = 1587 fills the 163,840 bytes, 1588 is
    NotImplementedError naming the bytes, the limit and the largest T, before any launch."""
    import __graft_entry__ as g
    g.build()
    assert _lds_bytes(T_EDGE) == 163840 and _lds_bytes(T_EDGE + 1) == 163872
    auto, _, out, ref = _single(T_EDGE, "ggagg", S=1)
    _compare(out, ref, f"T = {T_EDGE}")
    assert out["accepted"].tolist() == [[1]] and out["hits"].tolist() == [[0]]
    n = T_EDGE + 1
    with pytest.raises(NotImplementedError, match=rf"T = {n} needs 163872 bytes of LDS.*the limit is 163840 \(T <= {T_EDGE};"):
        design_dfa(np.zeros((1, n, 4), dtype=np.float32), auto.delta, auto.kind, S=1, mask=np.ones((1, n), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- invariance
def test_layout_second_call_seed_dev_workspace_and_graph_replay_give_identical_bytes(case):
    a = case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", 0.3)
    B = len(LENGTHS)
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
    seed_dev = torch.tensor([SEED], dtype=torch.int64, device="cuda")          # (the bits of a seed below 2^63)
    others = dict(packed=_run(case, "gnra_run3", 0.3, "packed"), second=design_dfa(case["logits"], a.delta, a.kind, **kw),
                  seed_dev=design_dfa(case["logits"], a.delta, a.kind, seed=0, seed_dev=seed_dev, **kw),
                  ws_ff=design_dfa(case["logits"], a.delta, a.kind, ws=workspace(B, T, a.n_live, fill=0xFF), **kw),
                  ws_larger=design_dfa(case["logits"], a.delta, a.kind, ws=workspace(B + 1, T, a.n_live, fill=0x7F), **kw))
    for label, other in others.items():
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in OUTPUTS), label
    # stale outputs are fully overwritten, and the call replays from a captured graph
    out = design_outputs(FURTHER, S, B, T)
    ws = workspace(B, T, a.n_live, fill=0xFF)
    delta = a.delta.cuda()                                         # (nothing is uploaded while the stream captures)
    for fill in (-7, 99):
        for t in out.values():
            t.fill_(fill)
        design_dfa(case["logits"], delta, a.kind, ws=ws, out=out, **kw)
        assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS), fill
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        design_dfa(case["logits"], delta, a.kind, ws=ws, out=out, **kw)
    for t in out.values():
        t.fill_(-7)
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS)


def test_an_rna_alone_equals_the_rna_inside_the_batch(case):
    """RNA 5 (the fixed stretch that spells the motifs) alone at its row, in a batch of another B and T whose other rows are empty and
    hold garbage."""
    h, a = case["h"], case["auto"]["two_run3"]
    base = _run(case, "two_run3", 0.3)
    B2, T2, n = 8, 80, LENGTHS[5]
    rng = np.random.RandomState(5)
    logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    bias = rng.standard_normal((B2, T2, 4)).astype(np.float32)
    mask = np.zeros((B2, T2), dtype=np.float32)
    logits[5, :n], allowed[5, :n], bias[5, :n], mask[5, :n] = h["logits"][5, :n], h["allowed"][5, :n], h["bias"][5, :n], 1
    one = design_dfa(logits, a.delta, a.kind, mask=mask, allowed=allowed, bias=bias, temperature=0.3)
    assert _bytes(one["seqs"][:, 5, :n]) == _bytes(base["seqs"][:, 5, :n]) and bool((one["seqs"][:, 5, n:] == -1).all())
    assert all(_bytes(one[k][:, 5]) == _bytes(base[k][:, 5]) for k in ("seq_nll", "hits", "accepted"))
    assert one["dfa_miss"].tolist() == [1, 1, 1, 1, 1, 0, 1, 1] and bool((one["seqs"][:, [0, 1, 2, 3, 4, 6, 7]] == -1).all())


def test_300_samples_cover_two_chunks_and_the_first_4_are_the_call_with_4(case):
    a = case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", 1.0)
    rows = slice(6, 7)
    mask = torch.zeros_like(case["mask"])
    mask[6] = case["mask"][6]
    out = design_dfa(case["logits"], a.delta, a.kind, S=300, mask=mask, temperature=1.0, allowed=case["allowed"], bias=case["bias"])
    for k in ("seqs", "seq_nll", "hits", "accepted"):
        assert _bytes(out[k][:4, rows]) == _bytes(base[k][:, rows]), k
    got = out["seqs"].cpu().numpy()[:, 6]
    assert int(out["hits"][:, 6].abs().sum()) == 0 and int(out["accepted"][:, 6].sum()) == 300 and (got[:, 65:] == -1).all()
    assert len(np.unique(got[:, :65], axis=0)) > 290              # the slots are independent draws, not copies of a chunk
    plan = _ref(case, "gnra_run3", 1.0)["plans"][6]
    for s in (4, 63, 64, 255, 256, 257, 299):
        want, margin = plan.draw(SEED, s, 6)
        assert margin <= NEAR or np.array_equal(got[s, :65], want), s


def test_a_nan_row_changes_no_other_rnas_bytes(case):
    a = case["auto"]["two_run3"]
    base = _run(case, "two_run3", 1.0)
    logits = case["logits"].clone()
    logits[7, 100] = float("nan")
    out = design_dfa(logits, a.delta, a.kind, mask=case["mask"], temperature=1.0, allowed=case["allowed"], bias=case["bias"])
    others = [b for b in range(len(LENGTHS)) if b != 7]
    for k in ("seqs", "seq_nll", "hits", "accepted"):
        assert _bytes(out[k][:, others]) == _bytes(base[k][:, others]), k
    assert _bytes(out["dfa_miss"][others]) == _bytes(base["dfa_miss"][others]) and _bytes(out["infeasible"][others]) == _bytes(base["infeasible"][others])


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_every_bad_argument_the_workspace_and_the_partner_are_refused(case):
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    a = case["auto"]["gnra_run3"]
    lg, m = case["logits"], case["mask"]
    B = len(LENGTHS)
    delta, kind = a.delta.cuda(), a.kind.clone()
    dead0 = kind.clone()
    dead0[0] = 1
    ws = workspace(B, T, a.n_live)
    out = design_outputs(FURTHER, S, B, T)
    partner = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    for t in out.values():
        t.fill_(-7)
    keep = {k: t.clone() for k, t in out.items()}

    def call(logits=lg, mask=m, cu=None, B=B, T=T, temperature=1.0, S=S, delta=delta, kind=kind, n_states=a.n_states, partner=None, ws=ws,
             ws_bytes=None, outs=True):
        return _native.lib().rnampnn_design_dfa(_ptr(logits), B * T, _ptr(mask), _ptr(cu), B, T, float(temperature), S, C.c_uint64(SEED), None,
                                                None, _ptr(partner), 1, None, 0, _ptr(delta), _ptr(kind), n_states, _ptr(ws),
                                                C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes),
                                                *[_ptr(out[k]) if outs else None for k in OUTPUTS], _stream(lg.device))
    BAD, UNSUPPORTED = 1, 2
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)
    for t in out.values():
        t.fill_(-7)
    bad = dict(null_logits=call(logits=None), B0=call(B=0), T0=call(T=0), S0=call(S=0), S_big=call(S=65535), no_layout=call(mask=None),
               both_layouts=call(cu=case["cu"]), temperature0=call(temperature=0.0), temperature_nan=call(temperature=float("nan")),
               null_delta=call(delta=None), null_kind=call(kind=None), states0=call(n_states=0), states257=call(n_states=257),
               states_negative=call(n_states=-1), start_dead=call(kind=dead0), null_workspace=call(ws=None, ws_bytes=ws.numel()),
               small_workspace=call(ws_bytes=ws.numel() - 1), empty_workspace=call(ws_bytes=0))
    assert bad == {k: BAD for k in bad}, bad
    assert call(partner=partner) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match="base pairs .* are not built together with an automaton.*4\\^depth"):
        _native.check(call(partner=partner))
    with pytest.raises(ValueError, match="state 0, the start, is marked dead"):
        _native.check(call(kind=dead0))
    with pytest.raises(ValueError, match=rf"the workspace is too small \({ws.numel() - 1} bytes\).*needs {ws.numel()}"):
        _native.check(call(ws_bytes=ws.numel() - 1))
    with pytest.raises(ValueError, match="the workspace is null"):
        _native.check(call(ws=None, ws_bytes=ws.numel()))
    assert call(outs=False) == 0                                    # nothing asked for: no launch
    assert int(_native.lib().rnampnn_design_dfa_workspace_bytes(0, T, 5)) == 0
    torch.cuda.synchronize()
    assert all(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)                 # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the Python surface
MODEL_LENGTHS = [33, 20, 41]


def test_design_dfa_from_logits_in_both_layouts(case):
    from rnampnn.model.decode import design_dfa_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    a = case["auto"]["gnra_run3"]
    cons = DesignConstraints(case["allowed"], None, case["bias"], True)
    want = _run(case, "gnra_run3", 0.3)
    kw = dict(n_samples=S, temperature=0.3, seed=SEED, constraints=cons)
    for name, got in (("padded", design_dfa_from_logits(case["logits"], mask=case["mask"], require=a, **kw)),
                      ("packed", design_dfa_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, require=a, **kw)),
                      ("strings", design_dfa_from_logits(case["logits"], mask=case["mask"], require=["GNRA"], max_run=3, **kw))):
        assert len(got) == 6 and [t.dtype for t in got] == [torch.int8, torch.float32] + [torch.int32] * 4
        for t, k in zip(got, OUTPUTS):
            assert _bytes(t) == _bytes(want[k]), (name, k)


def test_both_models_design_with_a_required_motif():
    import __graft_entry__ as g
    g.build()
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.data import pad_batch
    from rnampnn.utils.motifs import DesignAutomaton
    torch.manual_seed(0)
    m = RNAMPNN(precision="f32", **SMALL).cuda().eval()
    items = [(synth.synth_rna(n, i, seed=1), synth.synth_labels(n, i, seed=1)) for i, n in enumerate(MODEL_LENGTHS)]
    _, c, mask, lens = pad_batch(items, pin=False)
    c, mask = c.cuda(), mask.cuda()
    groups, banned = R.required_sets(["GGAGG", "GNRA"]), R.expand(["GAAUUC"], 3)
    kw = dict(n_samples=4, temperature=1.0, seed=3)
    assert len(m.design(c, mask, **kw)) == 2                       # None keeps today's paths and return values
    auto = DesignAutomaton.from_motifs(["GGAGG", "GNRA"], ["GAAUUC"], 3)
    out = m.design(c, mask, require=auto, **kw)
    assert len(out) == 6 and out[0].shape == (4, 3, max(lens)) and int(out[3].abs().sum()) == 0 and int(out[4].sum()) == 12 and out[5].tolist() == [0, 0, 0]
    got = out[0].cpu().numpy()
    assert all(R.contains_all(row, groups) and AV.naive_hits(row, banned) == 0 for plane in got for row in plane)
    assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    hits, accepted = auto.scan(out[0])
    assert _bytes(hits) == _bytes(out[3]) and _bytes(accepted) == _bytes(out[4])
    strings = m.design(c, mask, require=["GNRA", "GGAGG"], avoid=["GAAUUC", "AAAA", "UUUU", "CCCC", "GGGG"], **kw)
    assert all(_bytes(x) == _bytes(y) for x, y in zip(strings, out))
    fixed = DesignConstraints.from_specs([("A" * 33, None), (None, None), (None, None)], lens, int(mask.shape[1]))
    out = m.design(c, mask, require=["GGAGG"], constraints=fixed, **kw)
    assert out[5].tolist() == [1, 0, 0] and int(out[4][:, 0].sum()) == 0 and int(out[4][:, 1:].sum()) == 8
    paired = DesignConstraints.from_specs([(None, "((((....))))" + "." * 21), (None, None), (None, None)], lens, int(mask.shape[1]))
    with pytest.raises(ValueError, match="drop `structure`"):
        m.design(c, mask, require=["GGAGG"], constraints=paired, **kw)
    with pytest.raises(ValueError, match="require together with gc_content is not built"):
        m.design(c, mask, gc_content=(0.4, 0.6), require=["GGAGG"], **kw)
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    out = r.design(X, mask, n_samples=4, temperature=1.0, seed=5, lengths=MODEL_LENGTHS, require=auto)
    assert len(out) == 6 and out[0].shape == (4, 3, max(lens)) and int(out[3].abs().sum()) == 0 and int(out[4].sum()) == 12 and out[5].tolist() == [0, 0, 0]
    assert all(R.contains_all(row, groups) and AV.naive_hits(row, banned) == 0 for plane in out[0].cpu().numpy() for row in plane)
    assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    assert len(r.design(X, mask, n_samples=2, temperature=1.0, seed=5, lengths=MODEL_LENGTHS)) == 3


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_required_motifs(family, tmp_path, monkeypatch):
    """--require with --avoid / --max-run adds the columns motif_hits, required_found and require_miss; the CSV is read back against the
    tensors the entry returned (recorded on their way through ``design_dfa_from_logits``); every written design holds both motifs and
    no avoided word; the designs file written without the flags is byte for byte the same before and after."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    from rnampnn.model import decode as D
    from rnampnn.model.decode import letters_padded
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--samples", "3", "--temperature", "1.0",
              "--batch-size", "2"]
    quiet = dict(log=lambda *a: None)
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "before.csv")]), **quiet)
    calls, inner = [], D.design_dfa_from_logits

    def recording(*a, **kw):
        res = inner(*a, **kw)
        calls.append(res)
        return res
    monkeypatch.setattr(D, "design_dfa_from_logits", recording)
    des = str(tmp_path / "require.csv")
    P.run(P.parse(common + ["--designs-out", des, "--require", "GGAGG,GNRA", "--avoid", "GAATTC", "--max-run", "3"]), **quiet)
    monkeypatch.undo()
    d = list(csv.reader(open(des)))
    head = ["pdb_id", "sample", "seq", "nll_per_nt", "recovery"] + (["infeasible"] if family == "rdesign" else [])
    assert d[0] == head + ["motif_hits", "required_found", "require_miss"] and len(d) == 1 + 3 * 3
    for r in d[1:]:
        assert len(r[2]) == lens[ids.index(r[0])] and r[-3:] == ["0", "1", "0"], r
        assert "GGAGG" in r[2] and any(w in r[2] for w in ("GAAA", "GUAA", "GCAA", "GGAA", "GAGA", "GUGA", "GCGA", "GGGA")), r
        assert not any(w in r[2] for w in ("GAAUUC", "AAAA", "UUUU", "CCCC", "GGGG")), r
    # the rows against the tensors: every (sequence, hits, accepted, miss) the entry returned is a row of the file, and there are no others
    rows = sorted((r[2], r[-3], r[-2], r[-1]) for r in d[1:])
    want = []
    for seqs, _, _, hits, accepted, miss in calls:
        for s in range(seqs.shape[0]):
            for b, text in enumerate(letters_padded(seqs[s])):
                want.append((text, str(int(hits[s, b])), str(int(accepted[s, b])), str(int(miss[b]))))
    assert len(calls) == 2 and sorted(want) == rows
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "after.csv")]), **quiet)
    assert open(tmp_path / "before.csv", "rb").read() == open(tmp_path / "after.csv", "rb").read()
    (tmp_path / "cons.csv").write_text("pdb_id,fixed,structure\nr2," + "." * 33 + ",((((....))))" + "." * 21 + "\n")
    with pytest.raises(ValueError, match="drop `structure` from the constraints of \\['r2'\\]"):
        P.run(P.parse(common + ["--require", "GGAGG", "--constraints", str(tmp_path / "cons.csv")]), **quiet)
