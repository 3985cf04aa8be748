"""``rnampnn_design_nested`` (csrc/design_nested.hip) on the device: against the float64 restatement of its contract in
tests/_design_nested_ref.py, against ``rnampnn_design_dfa`` byte for byte where no pair is valid (the anchor), against a substring scan and a
pair-by-pair comparison of the written bytes, against enumerated probabilities, and at its edges (T = 1000 with a stem 120 pairs deep, the
LDS edge, the live-state limit, every refused argument).

The batch is the one ``_design_nested_ref`` describes next to ``CASE_LENGTHS``.  Device and restatement differ by last-bit exp / log, so a
draw whose path has a selection within 1e-8 of a cumulative boundary is left out of the equality check; the share left out is printed and
capped at 5 %, the cap tests/test_design_nested_cpu.py holds the restatement alone to."""
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

import _design_dfa_ref as DF  # noqa: E402
import _design_nested_ref as R  # noqa: E402
from _design_case import SMALL, design_outputs, dfa_workspace, raw_design, _bytes, _dev, _write_data, _checkpoint  # noqa: E402
from _design_case import design_dfa as _case_design_dfa  # noqa: E402
from _design_ref import PAIRS  # noqa: E402

LENGTHS, T, S, SEED = R.CASE_LENGTHS, R.CASE_T, R.CASE_S, R.CASE_SEED
NEAR = 1e-8
OUTPUTS = ("seqs", "seq_nll", "infeasible", "hits", "accepted", "dfa_miss", "nest_miss")
FURTHER = (("hits", torch.int32, True), ("accepted", torch.int32, True), ("dfa_miss", torch.int32, False), ("nest_miss", torch.int32, False))
T_EDGE = 1616                                                      # the largest padded extent: 163,552 of 163,840 bytes of LDS


def _automaton(name):
    from rnampnn.utils.motifs import as_nested_automaton
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    return as_nested_automaton(require or None, avoid or None, max_run)


def _lds_bytes(t, live):
    return 36 * t + max(16 * live * live, 1024 * (((t + 15) // 16) | 1)) + 1952


def workspace(B, T, live, fill=None):
    return dfa_workspace("rnampnn_design_nested_workspace_bytes", B, T, live, fill=fill, need=8 * B * T * live * live + 256 * B * (T // 2 + 1))


def design_nested(logits, delta, kind, seed=SEED, S=S, ws=None, **kw):
    """The C entry on device tensors (numpy arrays are uploaded; ``kind`` stays on the host) -> dict of its seven outputs."""
    kind = torch.as_tensor(np.ascontiguousarray(kind), dtype=torch.uint8).contiguous()
    live = int(((kind & 1) == 0).sum())
    m, cu = kw.get("mask"), kw.get("cu")
    B = int(m.shape[0]) if m is not None else int(cu.shape[0]) - 1
    Tp = int(m.shape[1]) if m is not None else int(kw["T"])
    ws = workspace(B, Tp, live) if ws is None else ws
    return raw_design("rnampnn_design_nested", (_dev(delta, torch.uint8), kind, int(kind.numel()), ws, C.c_size_t(ws.numel())), FURTHER, logits,
                      seed=seed, S=S, **kw)


design_dfa = functools.partial(_case_design_dfa, seed=SEED, S=S)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = R.case_arrays()
    d = dict(h=h, run={}, auto={name: _automaton(name) for name in R.CASE_AUTOMATA})
    for k in ("logits", "mask", "allowed", "partner", "bias", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _kw(case, temperature):
    return dict(temperature=temperature, allowed=case["allowed"], partner=case["partner"], bias=case["bias"])


def _run(case, name, temperature=1.0, layout="padded"):
    """The batch through the kernel, once per (automaton, temperature, layout)."""
    key = (name, float(temperature), layout)
    if key not in case["run"]:
        a = case["auto"][name]
        if layout == "padded":
            case["run"][key] = design_nested(case["logits"], a.delta, a.kind, mask=case["mask"], **_kw(case, temperature))
        else:
            case["run"][key] = design_nested(case["packed"], a.delta, a.kind, cu=case["cu"], T=T, **_kw(case, temperature))
    return case["run"][key]


def _ref(case, name, temperature):
    a = case["auto"][name]
    return R.case_ref(name, a.delta.numpy(), a.kind.numpy(), temperature)


def _compare(out, ref, label):
    """Draws equal the restatement wherever every margin exceeds NEAR; the flags match exactly.  -> the share left out."""
    got, want, near = out["seqs"].cpu().numpy(), ref["seqs"], ref["margin"] <= NEAR
    print(f"{label}: {int(near.sum())} of the {near.size} (sample, RNA) draws left out ({near.mean():.4%}: a selection within {NEAR} of a boundary)")
    assert near.mean() <= 0.05
    for k in ("dfa_miss", "nest_miss", "infeasible"):
        assert out[k].tolist() == ref[k].tolist(), k
    Sn, Bn = near.shape
    differ = [(s, b) for s in range(Sn) for b in range(Bn) if not near[s, b] and not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"
    keep = ~near
    assert np.array_equal(out["hits"].cpu().numpy()[keep], ref["hits"][keep]) and np.array_equal(out["accepted"].cpu().numpy()[keep], ref["accepted"][keep])
    return near.mean()


def _pairs_hold(seq, mate, wobble=True):
    return all((int(seq[t]), int(seq[j])) in PAIRS[wobble] for t, j in enumerate(mate) if j > t)


# ---------------------------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_restatement_pair_and_hold_the_motifs(case, name, temperature):
    from rnampnn.model.decode import score_logits
    out, ref = _run(case, name, temperature), _ref(case, name, temperature)
    _compare(out, ref, f"{name}, temperature {temperature}")
    assert out["infeasible"].tolist() == R.CASE_INFEASIBLE and out["nest_miss"].tolist() == R.CASE_NEST
    assert out["dfa_miss"].tolist() == R.CASE_MISS[name]
    got = out["seqs"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
    # the flags are the recount of the written bytes: the user-facing scan on the device, and a substring comparison on the host
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    groups, banned = R.required_sets(require), R.expand(avoid, max_run)
    hits, accepted = case["auto"][name].scan(out["seqs"])
    assert _bytes(hits) == _bytes(out["hits"]) and _bytes(accepted) == _bytes(out["accepted"])
    count = out["hits"].cpu().numpy()
    assert np.array_equal(count, np.array([[R.naive_hits(row, banned) for row in plane] for plane in got], dtype=np.int32))
    for b, plan in enumerate(ref["plans"]):
        for s in range(S):
            assert _pairs_hold(got[s, b], plan.mate), (s, b)        # every feasible pair is compatible, on a miss too
            if not (plan.miss or plan.nest_miss):
                assert count[s, b] == 0 and int(out["accepted"][s, b]) == 1
                assert R.contains_all(got[s, b], groups) and R.naive_hits(got[s, b], banned) == 0, (s, b)
    assert (got[:, 5, 20:27] == np.array([3, 3, 0, 3, 3, 0, 0])).all() and (got[:, 5, 2] == 0).all() and (got[:, 5, 60] == 0).all()
    if max_run == 3:
        assert (count[:, 4] > 0).all()                              # the stem that cannot avoid AAAA: drawn free, the run is reported
    sc = score_logits(case["logits"], mask=case["mask"], seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])


# ---------------------------------------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("name", ["ggagg", "gnra_run3"])
def test_without_a_valid_pair_every_output_is_rnampnn_design_dfas_byte_for_byte(name):
    """The DFA entry's own batch and automata (11 and 61 states): a null partner table and one of -1 everywhere give its bytes, at both
    temperatures; nest_miss is 0."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.motifs import DesignAutomaton
    h = DF.case_arrays()
    auto = DesignAutomaton.from_motifs(*DF.CASE_AUTOMATA[name])
    dev = {k: torch.from_numpy(h[k]).cuda() for k in ("logits", "mask", "allowed", "bias")}
    none = torch.full((len(DF.CASE_LENGTHS), DF.CASE_T), -1, dtype=torch.int32, device="cuda")
    broken = none.clone()
    broken[5, 3], broken[5, 9], broken[7, 4], broken[8, 299] = 9, 4, 4, 300       # not symmetric, itself, outside the RNA: no pair
    for temperature in (1.0, 0.3):
        kw = dict(seed=DF.CASE_SEED, S=DF.CASE_S, mask=dev["mask"], temperature=temperature, allowed=dev["allowed"], bias=dev["bias"])
        want = design_dfa(dev["logits"], auto.delta, auto.kind, **kw)
        for label, partner in (("null", None), ("unpaired", none), ("broken", broken)):
            out = design_nested(dev["logits"], auto.delta, auto.kind, partner=partner, **kw)
            for k in OUTPUTS[:6]:
                assert _bytes(out[k]) == _bytes(want[k]), (name, temperature, label, k)
            assert out["nest_miss"].tolist() == [0] * len(DF.CASE_LENGTHS) and out["dfa_miss"].tolist() == DF.CASE_MISS


# ---------------------------------------------------------------------------------------------------------------- frequencies
def test_20000_draws_of_a_hairpin_follow_the_enumerated_probabilities():
    """((..)) under require GA and no run longer than 2, temperature 1: every admitted sequence's count lies within 5 binomial standard
    deviations of N p, p from the restatement's ``path_logprob`` (which the CPU test pins to the enumerated joint); no draw lies outside
    the language or breaks a pair.  Logits 0.25 * randn keep every p within a small factor of the mean."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.motifs import DesignAutomaton
    auto = DesignAutomaton.from_motifs(["GA"], max_run=2)
    N, n = 20000, 6
    mate = R.parse_structure("((..))")
    logits = (0.25 * np.random.RandomState(4).standard_normal((1, n, 4))).astype(np.float32)
    out = design_nested(logits, auto.delta, auto.kind, S=N, seed=77, mask=np.ones((1, n), dtype=np.float32), partner=mate[None])
    assert out["dfa_miss"].tolist() == [0] and out["nest_miss"].tolist() == [0]
    assert int(out["hits"].abs().sum()) == 0 and int(out["accepted"].sum()) == N
    got = out["seqs"].cpu().numpy()[:, 0].astype(np.int64)
    counts = np.bincount((got * 4 ** np.arange(n - 1, -1, -1)).sum(axis=1), minlength=4 ** n)
    plan = R.NestedPlan(logits[0], n, 1.0, auto.delta.numpy(), auto.kind.numpy(), None, mate)
    p = np.array([np.exp(plan.path_logprob(seq)) for seq in itertools.product(range(4), repeat=n)])
    assert abs(p.sum() - 1.0) < 1e-12 and (counts[p == 0] == 0).all()
    sd = np.sqrt(N * p * (1 - p))
    dev = np.abs(counts - N * p)[p > 0] / sd[p > 0]
    print(f"{int((p > 0).sum())} admitted sequences, N p from {N * p[p > 0].min():.2f} to {N * p.max():.2f}; largest deviation {dev.max():.2f} sd")
    assert dev.max() <= 5.0


# ---------------------------------------------------------------------------------------------------------------- invariance
def test_layout_second_call_seed_dev_workspace_and_graph_replay_give_identical_bytes(case):
    a = case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", 0.3)
    B = len(LENGTHS)
    kw = dict(mask=case["mask"], **_kw(case, 0.3))
    seed_dev = torch.tensor([SEED], dtype=torch.int64, device="cuda")          # (the bits of a seed below 2^63)
    others = dict(packed=_run(case, "gnra_run3", 0.3, "packed"), second=design_nested(case["logits"], a.delta, a.kind, **kw),
                  seed_dev=design_nested(case["logits"], a.delta, a.kind, seed=0, seed_dev=seed_dev, **kw),
                  ws_ff=design_nested(case["logits"], a.delta, a.kind, ws=workspace(B, T, a.n_live, fill=0xFF), **kw),
                  ws_larger=design_nested(case["logits"], a.delta, a.kind, ws=workspace(B + 1, T, a.n_live, fill=0x7F), **kw))
    for label, other in others.items():
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in OUTPUTS), label
    # stale outputs are fully overwritten, and the call replays from a captured graph
    out = design_outputs(FURTHER, S, B, T)
    ws = workspace(B, T, a.n_live, fill=0xFF)
    delta = a.delta.cuda()                                         # (nothing is uploaded while the stream captures)
    for fill in (-7, 99):
        for t in out.values():
            t.fill_(fill)
        design_nested(case["logits"], delta, a.kind, ws=ws, out=out, **kw)
        assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS), fill
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        design_nested(case["logits"], delta, a.kind, ws=ws, out=out, **kw)
    for t in out.values():
        t.fill_(-7)
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS)


def test_an_rna_alone_equals_the_rna_inside_the_batch(case):
    """RNA 5 (the stem with the fixed stretch, the hairpin in its loop, the pair that cannot pair) alone at its row, in a batch of another
    B and T whose other rows are empty and hold garbage."""
    h, a = case["h"], case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", 0.3)
    B2, T2, n = 8, 80, LENGTHS[5]
    rng = np.random.RandomState(5)
    logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    partner = rng.randint(-5, T2 + 5, size=(B2, T2)).astype(np.int32)
    bias = rng.standard_normal((B2, T2, 4)).astype(np.float32)
    mask = np.zeros((B2, T2), dtype=np.float32)
    logits[5, :n], allowed[5, :n], partner[5, :n], bias[5, :n], mask[5, :n] = h["logits"][5, :n], h["allowed"][5, :n], h["partner"][5, :n], h["bias"][5, :n], 1
    one = design_nested(logits, a.delta, a.kind, mask=mask, allowed=allowed, partner=partner, bias=bias, temperature=0.3)
    assert _bytes(one["seqs"][:, 5, :n]) == _bytes(base["seqs"][:, 5, :n]) and bool((one["seqs"][:, 5, n:] == -1).all())
    assert all(_bytes(one[k][:, 5]) == _bytes(base[k][:, 5]) for k in ("seq_nll", "hits", "accepted"))
    assert one["dfa_miss"].tolist() == [1, 1, 1, 1, 1, 0, 1, 1] and one["nest_miss"].tolist() == [0] * 8 and int(one["infeasible"][5]) == 2
    assert bool((one["seqs"][:, [0, 1, 2, 3, 4, 6, 7]] == -1).all())


def test_300_samples_cover_two_chunks_and_the_first_4_are_the_call_with_4(case):
    a = case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", 1.0)
    b, n = 5, LENGTHS[5]
    mask = torch.zeros_like(case["mask"])
    mask[b] = case["mask"][b]
    out = design_nested(case["logits"], a.delta, a.kind, S=300, mask=mask, **_kw(case, 1.0))
    for k in ("seqs", "seq_nll", "hits", "accepted"):
        assert _bytes(out[k][:4, b:b + 1]) == _bytes(base[k][:, b:b + 1]), k
    got = out["seqs"].cpu().numpy()[:, b]
    assert int(out["hits"][:, b].abs().sum()) == 0 and int(out["accepted"][:, b].sum()) == 300 and (got[:, n:] == -1).all()
    assert len(np.unique(got[:, :n], axis=0)) > 250               # the slots are independent draws, not copies of a chunk
    plan = _ref(case, "gnra_run3", 1.0)["plans"][b]
    assert all(_pairs_hold(row, plan.mate) for row in got)
    for s in (4, 63, 64, 255, 256, 257, 299):
        want, margin = plan.draw(SEED, s, b)
        assert margin <= NEAR or np.array_equal(got[s, :n], want), s


def test_a_nan_row_changes_no_other_rnas_bytes(case):
    a = case["auto"]["gnra_run3"]
    base = _run(case, "gnra_run3", 1.0)
    logits = case["logits"].clone()
    logits[7, 100] = float("nan")
    out = design_nested(logits, a.delta, a.kind, mask=case["mask"], **_kw(case, 1.0))
    others = [b for b in range(len(LENGTHS)) if b != 7]
    for k in ("seqs", "seq_nll", "hits", "accepted"):
        assert _bytes(out[k][:, others]) == _bytes(base[k][:, others]), k
    for k in ("dfa_miss", "nest_miss", "infeasible"):
        assert _bytes(out[k][others]) == _bytes(base[k][others]), k


# ---------------------------------------------------------------------------------------------------------------- edges
def _single(n, name, structure, S=2, temperature=1.0, seed=11, raise_g=0.0):
    auto = _automaton(name)
    rng = np.random.RandomState(seed)
    logits = (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32)
    logits[0, :, 3] += raise_g
    mate = R.parse_structure(structure)
    assert len(mate) == n
    out = design_nested(logits, auto.delta, auto.kind, S=S, mask=np.ones((1, n), dtype=np.float32), temperature=temperature, partner=mate[None])
    ref = R.design_nested_ref(logits, [n], temperature, S, SEED, auto.delta.numpy(), auto.kind.numpy(), None, mate[None])
    return auto, logits, mate, out, ref


def test_t_1000_with_a_stem_120_pairs_deep():
    """One RNA of 1000 nucleotides under no run longer than 3 (13 live states): a stem of 120 stacked pairs (the goal stack runs 120
    deep), hairpins before and after it; the draws equal the restatement, pair everywhere and hold no run; the NLL bytes are rnampnn_score's."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import score_logits
    structure = R._pad(R._hairpin(5, 4) + "..." + R._hairpin(120, 6) + ".." + "((" + R._hairpin(6, 3) + "." + R._hairpin(3, 7) + "))" + "()", 1000, left=300)
    auto, logits, mate, out, ref = _single(1000, "max_run3", structure, raise_g=6.0)
    assert auto.n_live == 13 and out["dfa_miss"].tolist() == [0] and out["nest_miss"].tolist() == [0]
    _compare(out, ref, "T = 1000, 13 live states, depth 120")
    got = out["seqs"].cpu().numpy()
    assert all(_pairs_hold(got[s, 0], mate) and R.naive_hits(got[s, 0], R.expand((), 3)) == 0 for s in range(2))
    assert out["hits"].tolist() == [[0], [0]] and out["accepted"].tolist() == [[1], [1]]
    sc = score_logits(torch.from_numpy(logits).cuda(), mask=torch.ones(1, 1000, device="cuda"), seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])


def test_the_lds_edge_is_accepted_on_one_side_and_refused_on_the_other():
    """bytes(T, L) = 36 T + max(16 L^2, 1024 (ceil(T / 16) | 1)) + 1952: T = 1616 takes 163,552 of the 163,840 bytes and runs, 1617 is
    NotImplementedError naming the bytes, the limit and the largest T, before any launch - at 11 live states and at 53 alike."""
    import __graft_entry__ as g
    g.build()
    assert _lds_bytes(T_EDGE, 11) == _lds_bytes(T_EDGE, 64) == 163552 and _lds_bytes(T_EDGE + 1, 11) == 165636 and _lds_bytes(1000, 64) == 103488
    structure = R._pad(R._hairpin(9, 5) + "." + R._hairpin(4, 3), T_EDGE - 2, left=700)
    auto, _, mate, out, ref = _single(T_EDGE, "ggagg", "(" + structure + ")", S=1)
    _compare(out, ref, f"T = {T_EDGE}")
    assert out["accepted"].tolist() == [[1]] and out["hits"].tolist() == [[0]] and _pairs_hold(out["seqs"].cpu().numpy()[0, 0], mate)
    n = T_EDGE + 1
    for name in ("ggagg", "gnra_run3"):
        auto = _automaton(name)
        with pytest.raises(NotImplementedError, match=rf"T = {n} needs 165636 bytes of LDS.*the limit is 163840 \(T <= {T_EDGE} at {auto.n_live} live"):
            design_nested(np.zeros((1, n, 4), dtype=np.float32), auto.delta, auto.kind, S=1, mask=np.ones((1, n), dtype=np.float32))


def test_every_bad_argument_and_73_live_states_are_refused_and_launch_nothing(case):
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    from rnampnn.utils.motifs import DesignAutomaton
    a = case["auto"]["gnra_run3"]
    lg, m = case["logits"], case["mask"]
    B = len(LENGTHS)
    delta, kind = a.delta.cuda(), a.kind.clone()
    dead0 = kind.clone()
    dead0[0] = 1
    ws = workspace(B, T, a.n_live)
    out = design_outputs(FURTHER, S, B, T)
    for t in out.values():
        t.fill_(-7)
    keep = {k: t.clone() for k, t in out.items()}

    def call(logits=lg, mask=m, cu=None, B=B, T=T, temperature=1.0, S=S, delta=delta, kind=kind, n_states=a.n_states, partner=case["partner"], ws=ws,
             ws_bytes=None, outs=True):
        return _native.lib().rnampnn_design_nested(_ptr(logits), B * T, _ptr(mask), _ptr(cu), B, T, float(temperature), S, C.c_uint64(SEED), None,
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
    with pytest.raises(ValueError, match="state 0, the start, is marked dead"):
        _native.check(call(kind=dead0))
    with pytest.raises(ValueError, match=rf"the workspace is too small \({ws.numel() - 1} bytes\).*need {ws.numel()}"):
        _native.check(call(ws_bytes=ws.numel() - 1))
    with pytest.raises(ValueError, match="the workspace is null"):
        _native.check(call(ws=None, ws_bytes=ws.numel()))
    # two required 5-mers with no run longer than 3: 89 states, 73 live - the DFA entry's ground, past this entry's limit
    two = DesignAutomaton.from_motifs(("GGAGG", "CUUCG"), (), 3)
    assert two.n_live == 73
    big = workspace(B, T, 73)
    assert call(delta=two.delta.cuda(), kind=two.kind, n_states=two.n_states, ws=big) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match="the automaton has 73 live states, the limit is 64"):
        _native.check(call(delta=two.delta.cuda(), kind=two.kind, n_states=two.n_states, ws=big))
    assert call(outs=False) == 0                                    # nothing asked for: no launch
    assert int(_native.lib().rnampnn_design_nested_workspace_bytes(0, T, 5)) == 0
    torch.cuda.synchronize()
    assert all(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)                 # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the Python surface
MODEL_LENGTHS = [33, 20, 41]
MODEL_STRUCTURES = ["((((....))))" + "." * 5 + "(((...)))" + "." * 7, "(((..(...)..))).....", "." * 41]


def test_design_nested_from_logits_in_both_layouts(case):
    from rnampnn.model.decode import design_by_mode, design_nested_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    a = case["auto"]["gnra_run3"]
    cons = DesignConstraints(case["allowed"], case["partner"], case["bias"], True)
    want = _run(case, "gnra_run3", 0.3)
    kw = dict(n_samples=S, temperature=0.3, seed=SEED, constraints=cons)
    for name, got in (("padded", design_nested_from_logits(case["logits"], mask=case["mask"], require=a, **kw)),
                      ("packed", design_nested_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, require=a, **kw)),
                      ("strings", design_nested_from_logits(case["logits"], mask=case["mask"], require=["GNRA"], max_run=3, **kw)),
                      ("by mode", design_by_mode("nested", case["logits"], mask=case["mask"], require=a, **kw))):
        assert len(got) == 7 and [t.dtype for t in got] == [torch.int8, torch.float32] + [torch.int32] * 5
        for t, k in zip(got, OUTPUTS):
            assert _bytes(t) == _bytes(want[k]), (name, k)
    alone = design_nested_from_logits(case["logits"], mask=case["mask"], avoid=[], max_run=3, **kw)
    for t, k in zip(alone, OUTPUTS):
        assert _bytes(t) == _bytes(_run(case, "max_run3", 0.3)[k]), k


def test_both_models_design_with_motifs_under_a_structure():
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
    _, c, mask, lens = pad_batch(items, pin=False)
    c, mask = c.cuda(), mask.cuda()
    Tm = int(mask.shape[1])
    cons = DesignConstraints.from_specs([(None, s) for s in MODEL_STRUCTURES], lens, Tm)
    mates = [R.parse_structure(s) for s in MODEL_STRUCTURES]
    groups, banned = R.required_sets(["GNRA"]), R.expand(["GGGG"])
    kw = dict(n_samples=4, temperature=1.0, seed=3)

    def check(out):
        assert len(out) == 7 and out[0].shape == (4, 3, Tm) and int(out[3].abs().sum()) == 0 and int(out[4].sum()) == 12
        assert out[5].tolist() == [0, 0, 0] and out[6].tolist() == [0, 0, 0] and out[2].tolist() == [0, 0, 0]
        got = out[0].cpu().numpy()
        for plane in got:
            for b, row in enumerate(plane):
                assert R.contains_all(row, groups) and R.naive_hits(row, banned) == 0 and _pairs_hold(row, mates[b]), (b, row)
    out = m.design(c, mask, require=["GNRA"], avoid=["GGGG"], constraints=cons, pairs="nested", **{**kw, "n_samples": 4})
    check(out)
    assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    plain = m.design(c, mask, constraints=cons, **kw)
    assert len(plain) == 3                                          # without the switch: today's paths and return values
    only = m.design(c, mask, avoid=["GGGG"], constraints=cons.to_device("cuda"), pairs="nested", **kw)
    assert len(only) == 7 and int(only[3].abs().sum()) == 0 and all(_pairs_hold(row, mates[b]) for plane in only[0].cpu().numpy() for b, row in enumerate(plane))
    knot = DesignConstraints.from_specs([(None, "((..[[..))..]]" + "." * 19), (None, None), (None, None)], lens, Tm)
    with pytest.raises(ValueError, match=r"row\(s\) \[0\] holds a pseudoknot"):
        m.design(c, mask, avoid=["GGGG"], constraints=knot, pairs="nested", **kw)
    dev = m.design(c, mask, avoid=["GGGG"], constraints=knot.to_device("cuda"), pairs="nested", **kw)      # device side: the kernel reports it
    assert dev[6].tolist() == [1, 0, 0] and dev[5].tolist() == [0, 0, 0]
    # the same calls without pairs raise what they raised
    with pytest.raises(ValueError, match="avoid together with base pairs is not built.*drop `structure`"):
        m.design(c, mask, avoid=["GGGG"], constraints=cons, **kw)
    with pytest.raises(ValueError, match="require together with base pairs is not built.*drop `structure`"):
        m.design(c, mask, require=["GNRA"], constraints=cons, **kw)
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    out = r.design(X, mask, n_samples=4, temperature=1.0, seed=5, lengths=MODEL_LENGTHS, require=["GNRA"], avoid=["GGGG"], constraints=cons, pairs="nested")
    check(out)
    assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    with pytest.raises(ValueError, match="require together with base pairs is not built"):
        r.design(X, mask, n_samples=2, lengths=MODEL_LENGTHS, require=["GNRA"], constraints=cons)


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_pairs_nested(family, tmp_path, monkeypatch):
    """--pairs nested with --require / --avoid / --max-run and a structure in --constraints adds the columns motif_hits, required_found,
    require_miss and nest_miss; the CSV is read back against the tensors the entry returned (recorded on their way through
    ``design_nested_from_logits``); every written design pairs as its structure says, holds the motif and no avoided word; without the
    switch the same command is refused in today's words."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    from rnampnn.model import decode as D
    from rnampnn.model.decode import letters_padded
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    structure = dict(zip(ids, MODEL_STRUCTURES))
    (tmp_path / "cons.csv").write_text("pdb_id,fixed,structure\n" + "".join(f"{rid},,{structure[rid]}\n" for rid in ids))
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--samples", "3", "--temperature", "1.0",
              "--batch-size", "2", "--constraints", str(tmp_path / "cons.csv")]
    quiet = dict(log=lambda *a: None)
    calls, inner = [], D.design_nested_from_logits

    def recording(*a, **kw):
        res = inner(*a, **kw)
        calls.append(res)
        return res
    monkeypatch.setattr(D, "design_nested_from_logits", recording)
    des = str(tmp_path / "nested.csv")
    P.run(P.parse(common + ["--designs-out", des, "--pairs", "nested", "--require", "GNRA", "--avoid", "GAATTC", "--max-run", "3"]), **quiet)
    monkeypatch.undo()
    d = list(csv.reader(open(des)))
    assert d[0] == ["pdb_id", "sample", "seq", "nll_per_nt", "recovery", "infeasible", "motif_hits", "required_found", "require_miss", "nest_miss"]
    assert len(d) == 1 + 3 * 3
    tetraloops = ("GAAA", "GUAA", "GCAA", "GGAA", "GAGA", "GUGA", "GCGA", "GGGA")
    for r in d[1:]:
        assert len(r[2]) == lens[ids.index(r[0])] and r[-5:] == ["0", "0", "1", "0", "0"], r
        assert any(w in r[2] for w in tetraloops) and not any(w in r[2] for w in ("GAAUUC", "AAAA", "UUUU", "CCCC", "GGGG")), r
        assert _pairs_hold(["AUCG".index(ch) for ch in r[2]], R.parse_structure(structure[r[0]])), r
    rows = sorted((r[2],) + tuple(r[-4:]) for r in d[1:])
    want = []
    for seqs, _, _, hits, accepted, miss, nest in calls:
        for s in range(seqs.shape[0]):
            for b, text in enumerate(letters_padded(seqs[s])):
                want.append((text, str(int(hits[s, b])), str(int(accepted[s, b])), str(int(miss[b])), str(int(nest[b]))))
    assert len(calls) == 2 and sorted(want) == rows
    with pytest.raises(ValueError, match="drop `structure` from the constraints of \\['r0', 'r1', 'r2'\\]"):
        P.run(P.parse(common + ["--require", "GNRA"]), **quiet)
    (tmp_path / "knot.csv").write_text("pdb_id,fixed,structure\nr2,,((..[[..))..]]" + "." * 19 + "\n")
    with pytest.raises(ValueError, match=r"\['r2'\] holds a pseudoknot"):
        P.run(P.parse(common[:-1] + [str(tmp_path / "knot.csv"), "--pairs", "nested", "--max-run", "3"]), **quiet)
