"""``rnampnn_design_dfa_profile`` (csrc/design_dfa_profile.hip) on the device, against the float64 restatement of its contract in
tests/_design_dfa_profile_ref.py, against the entries next to it (``rnampnn_design_dfa``: the flags byte for byte and the class frequencies
of 4096 draws; ``rnampnn_design_avoid_profile`` on an avoid-only automaton; the ``log_z`` of ``rnampnn_design_dfa_count`` with nothing
counted) and against itself (layouts, a second call, a stale workspace and stale outputs, an RNA alone, a captured graph, a NaN row).

The batch is ``_design_dfa_ref.case_arrays()``: lengths 0, 1, 2, 3, 63, 64, 65, 257, 300 at T = 300, rows 0 .. 4 misses, under the three
``CASE_AUTOMATA`` (11, 53 and 73 live states: one wave and past one wave) at temperatures 1.0 and 0.3.

Tolerances: the profile family's (include/rnampnn_hip.h) - marginals within 1e-8 absolute, log_z, log_z_free and entropy within
1e-8 * max(1, |value|); tests/test_design_dfa_profile_cpu.py shows the restatement's own rows summing to 1 within 1.5e-11 on this batch.
Each test prints the maxima it observed."""
import csv
import ctypes as C
import functools
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

import _design_avoid_ref as AR  # noqa: E402
import _design_dfa_profile_ref as PR  # noqa: E402
import _design_dfa_ref as R  # noqa: E402
import _design_profile_ref as FR  # noqa: E402
from _design_case import (SMALL, PROFILE_OUTPUTS as OUTPUTS, PROFILE_SCALARS as SCALARS, agree_profile, dfa_workspace, one_rna, profile_outputs, raw_design, raw_profile,  # noqa: E402
                          same_profile, _bytes, _dev, _write_data, _checkpoint)
from _design_case import design_dfa as _case_design_dfa  # noqa: E402

LENGTHS, T, B = R.CASE_LENGTHS, R.CASE_T, len(R.CASE_LENGTHS)
TOL = 1e-8
T_MAX = 4498                                                       # the largest T in 160 KiB of LDS (include/rnampnn_hip.h)
LONG = "GGAGGCUUCGAAUUCGCAUGCCAUGGUACCUAGCUAGGAUCCGAUAUCAAGCUUGCGGCCGCUCGAGACGUCUGCAGCCCGGGAGAUCUGUCGACACUAGUUCUAGA"
STATES_256 = ((LONG[:26], LONG[50:89]), (), None)                  # two long required words: exactly 256 states, all of them live


def _lds_bytes(t):
    return 32 * t + 16 * ((t + 15) // 16) + 15392


def _automaton(spec):
    from rnampnn.utils.motifs import DesignAutomaton
    return DesignAutomaton.from_motifs(*spec)


def workspace(Bn, Tn, live, fill=None):
    from rnampnn import _native
    ws = dfa_workspace("rnampnn_design_dfa_profile_workspace_bytes", Bn, Tn, live, fill=fill)
    assert ws.numel() == int(_native.lib().rnampnn_design_dfa_workspace_bytes(Bn, Tn, live))
    return ws


def dfa_profile(logits, delta, kind, ws=None, **kw):
    """The C entry on device tensors (numpy arrays are uploaded; ``kind`` stays on the host) -> dict of its six outputs."""
    kind = torch.as_tensor(np.ascontiguousarray(kind), dtype=torch.uint8).contiguous()
    m, cu = kw.get("mask"), kw.get("cu")
    Bn = int(m.shape[0]) if m is not None else int(cu.shape[0]) - 1
    Tn = int(m.shape[1]) if m is not None else int(kw["T"])
    ws = workspace(Bn, Tn, int(((kind & 1) == 0).sum())) if ws is None else ws
    return raw_profile("rnampnn_design_dfa_profile", (_dev(delta, torch.uint8), kind, int(kind.numel()), ws, C.c_size_t(ws.numel())), logits, **kw)


design_dfa = functools.partial(_case_design_dfa, seed=R.CASE_SEED, S=1)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = R.case_arrays()
    d = dict(h=h, run={}, auto={name: _automaton(spec) for name, spec in R.CASE_AUTOMATA.items()})
    for k in ("logits", "mask", "allowed", "bias", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _run(case, name, temperature, layout="padded"):
    key = (name, float(temperature), layout)
    if key not in case["run"]:
        a = case["auto"][name]
        kw = dict(temperature=temperature, allowed=case["allowed"], bias=case["bias"])
        if layout == "padded":
            case["run"][key] = dfa_profile(case["logits"], a.delta, a.kind, mask=case["mask"], **kw)
        else:
            case["run"][key] = dfa_profile(case["packed"], a.delta, a.kind, cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _ref(case, name, temperature):
    h, a = case["h"], case["auto"][name]
    return FR.cached(("dfa", name, float(temperature)), lambda: PR.design_dfa_profile_ref(
        h["logits"], LENGTHS, temperature, a.delta.numpy(), a.kind.numpy(), h["allowed"], h["bias"]))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_the_profile_equals_the_float64_restatement_and_the_draw_entrys_flags(case, name, temperature):
    out = _run(case, name, temperature)
    ref = _ref(case, name, temperature)
    agree_profile(out, ref, f"{name}, temperature {temperature}", tol=TOL)
    assert ref["miss"].tolist() == R.CASE_MISS and ref["infeasible"].tolist() == R.CASE_INFEASIBLE
    P = out["marginals"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert not P[b, n:].any() and (n == 0 or np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL)
    assert [float(out[k][0]) for k in SCALARS] == [0.0, 0.0, 0.0]                           # the empty RNA: a miss, state 0 does not accept
    assert bool((out["log_z"] - out["log_z_free"] <= 1e-9 * out["log_z_free"].abs().clamp(min=1)).all())
    assert np.abs(P[5, 20:27][np.arange(7), [3, 3, 0, 3, 3, 0, 0]] - 1.0).max() <= TOL     # the fixed GGAGGAA of RNA 5
    a = case["auto"][name]
    draw = design_dfa(case["logits"], a.delta, a.kind, mask=case["mask"], temperature=temperature, allowed=case["allowed"], bias=case["bias"])
    assert _bytes(out["infeasible"]) == _bytes(draw["infeasible"]) and _bytes(out["miss"]) == _bytes(draw["dfa_miss"])


@pytest.mark.parametrize("name", sorted(AR.CASE_AUTOMATA))
def test_an_avoid_only_automaton_agrees_with_rnampnn_design_avoid_profile(name):
    """The anchor: the avoid entry's own batch and automata (at most 64 states), kind = "every live state accepts"."""
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    from rnampnn.utils.motifs import MotifAutomaton
    motifs, max_run = AR.CASE_AUTOMATA[name]
    auto = MotifAutomaton.from_motifs(motifs, max_run=max_run)
    kind = np.array([1 if (auto.terminal >> a) & 1 else 2 for a in range(auto.n_states)], dtype=np.uint8)
    h = AR.case_arrays()
    dev = {k: _dev(h[k]) for k in ("logits", "mask", "allowed", "bias")}
    Bn, Tn = h["mask"].shape
    for temperature in (1.0, 0.3):
        want = profile_outputs(Bn, Tn)
        _native.check(_native.lib().rnampnn_design_avoid_profile(
            _ptr(dev["logits"]), Bn * Tn, _ptr(dev["mask"]), None, Bn, Tn, float(temperature), _ptr(dev["allowed"]), None, 1, _ptr(dev["bias"]), 1,
            _ptr(auto.delta.cuda()), auto.n_states, C.c_uint64(auto.terminal), *[_ptr(want[k]) for k in OUTPUTS], _stream(dev["logits"].device)))
        out = dfa_profile(dev["logits"], auto.delta, kind, mask=dev["mask"], temperature=temperature, allowed=dev["allowed"], bias=dev["bias"])
        agree_profile(out, want, f"anchor {name}, temperature {temperature}", flags=False, tol=TOL)
        assert _bytes(out["infeasible"]) == _bytes(want["infeasible"]) and _bytes(out["miss"]) == _bytes(want["miss"])


@pytest.mark.parametrize("name", ["gnra_run3", "two_run3"])
def test_log_z_is_the_chains_with_nothing_counted(case, name):
    """``rnampnn_design_dfa_count`` with nothing counted and the window (0, 0) reports the log partition sum of the same chain."""
    a = case["auto"][name]
    from rnampnn import _native
    ws = torch.empty(int(_native.lib().rnampnn_design_dfa_count_workspace_bytes(B, T, a.n_live, 1)), dtype=torch.uint8, device="cuda")
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    further = (("hits", torch.int32, True), ("accepted", torch.int32, True), ("count", torch.int32, True), ("dfa_miss", torch.int32, False),
               ("count_miss", torch.int32, False), ("log_z", torch.float64, False))
    chain = raw_design("rnampnn_design_dfa_count", (a.delta.cuda(), a.kind, a.n_states, torch.zeros(B, T, dtype=torch.uint8, device="cuda"), zero, zero, 0,
                                                    ws, C.c_size_t(ws.numel())), further, case["logits"], mask=case["mask"], temperature=0.3, S=1,
                       allowed=case["allowed"], bias=case["bias"])
    out = _run(case, name, 0.3)
    rows = [b for b in range(B) if not R.CASE_MISS[b]]               # on a miss the chain reports -inf, the profile the fallback's sum
    got, want = out["log_z"].cpu().numpy()[rows], chain["log_z"].cpu().numpy()[rows]
    print(f"{name}: max relative |d log_z| = {(np.abs(got - want) / np.maximum(1, np.abs(want))).max():.3e}")
    assert (np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))).all()
    assert _bytes(out["miss"]) == _bytes(chain["dfa_miss"])


def test_the_frequencies_of_4096_draws_lie_within_six_sigma_of_the_profile(case):
    """One feasible RNA of 40 nt under "GA required, no run longer than 2": ``rnampnn_design_dfa`` with S = 4096 and the profile on the
    same inputs; |f - P| <= 6 sqrt(P (1 - P) / S) + 1 / S on every cell and f = 0 wherever P = 0."""
    h = FR.link_arrays()
    auto = _automaton((("GA",), (), 2))
    lg, m, al = h["logits"][2:3], h["mask"][2:3], h["allowed"][2:3]
    prof = dfa_profile(lg, auto.delta, auto.kind, mask=m, temperature=FR.LINK_TEMPERATURE, allowed=al)
    draw = design_dfa(lg, auto.delta, auto.kind, seed=FR.LINK_SEED, S=FR.LINK_S, mask=m, temperature=FR.LINK_TEMPERATURE, allowed=al)
    P = prof["marginals"].cpu().numpy()
    f = FR.frequencies(draw["seqs"].cpu().numpy())
    ref = PR.dfa_profile(R.DfaPlan(lg[0], FR.LINK_T, FR.LINK_TEMPERATURE, auto.delta.numpy(), auto.kind.numpy(), al[0])).marginals
    print(f"max |f - P| = {np.abs(f - P).max():.4f}, max |P - restatement| = {np.abs(P[0] - ref).max():.3e}")
    assert prof["miss"].tolist() == [0] and np.abs(P[0] - ref).max() <= TOL and bool((draw["accepted"] == 1).all())
    assert (np.abs(f - P) <= FR.link_bound(P)).all() and not f[P == 0].any()


# ---------------------------------------------------------------------------------------------------------------- bytes
def test_bytes_do_not_depend_on_the_layout_a_second_call_stale_memory_or_a_graph(case):
    a = case["auto"]["two_run3"]
    delta = a.delta.cuda()                                          # (nothing is uploaded inside the capture)
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
    padded = _run(case, "two_run3", 0.3)
    assert same_profile(padded, _run(case, "two_run3", 0.3, "packed"))
    assert same_profile(padded, dfa_profile(case["logits"], delta, a.kind, **kw))
    out, ws = profile_outputs(B, T), workspace(B, T, a.n_live)
    for t in list(out.values()) + [ws]:                             # a workspace and outputs of 0xFF bytes (NaN as doubles)
        t.view(torch.uint8).fill_(0xFF)
    dfa_profile(case["logits"], delta, a.kind, ws=ws, out=out, **kw)
    assert same_profile(padded, out)
    assert same_profile(padded, dfa_profile(case["logits"], delta, a.kind, ws=workspace(B + 1, T, a.n_live, fill=0x7F), **kw))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dfa_profile(case["logits"], delta, a.kind, ws=ws, out=out, **kw)
    for t in list(out.values()) + [ws]:
        t.view(torch.uint8).fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert same_profile(padded, out)


def test_an_rna_alone_in_another_batch_and_a_nan_row_leave_the_bytes_unchanged(case):
    """RNA 6 alone at its row of a batch with B = 8 and T = 80 whose other rows are empty and hold garbage; then the full batch with RNA 7
    turned into NaN: every other RNA keeps its bytes."""
    B2, T2, b = 8, 80, 6
    rng = np.random.RandomState(5)
    h, n, a = case["h"], LENGTHS[6], case["auto"]["gnra_run3"]
    logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    bias = rng.standard_normal((B2, T2, 4)).astype(np.float32)
    mask = np.zeros((B2, T2), dtype=np.float32)
    logits[b, :n], allowed[b, :n], mask[b, :n], bias[b, :n] = h["logits"][b, :n], h["allowed"][b, :n], 1, h["bias"][b, :n]
    base = _run(case, "gnra_run3", 0.3)
    one = dfa_profile(logits, a.delta, a.kind, mask=mask, temperature=0.3, allowed=allowed, bias=bias)
    assert _bytes(one["marginals"][b, :n]) == _bytes(base["marginals"][b, :n]) and not bool(one["marginals"][b, n:].any())
    assert all(_bytes(one[k][b]) == _bytes(base[k][b]) for k in OUTPUTS[1:])
    others = [r for r in range(B2) if r != b]
    assert not bool(one["marginals"][others].any()) and all(float(one[k][others].abs().max()) == 0.0 for k in SCALARS)
    assert one["miss"][others].tolist() == [1] * 7                  # empty RNAs: state 0 does not accept
    nan = case["logits"].clone()
    nan[7, 5] = float("nan")
    nan[7, 100, 2] = float("inf")
    out = dfa_profile(nan, a.delta, a.kind, mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
    torch.cuda.synchronize()
    assert same_profile(out, base, [r for r in range(B) if r != 7])
    assert not bool(out["marginals"][7, LENGTHS[7]:].any())         # the padding of the NaN row is still written as 0


# ---------------------------------------------------------------------------------------------------------------- extent
def test_an_automaton_of_256_states_runs_and_257_are_refused():
    import __graft_entry__ as g
    g.build()
    auto = _automaton(STATES_256)
    assert auto.n_states == 256 and auto.n_live == 256
    n = 120
    logits, mask = one_rna(n, 21)
    seq = [["AUCG".index(ch) for ch in w] for w in STATES_256[0]]   # both words fixed into the RNA, so that it is feasible
    allowed = np.full((1, n), 15, dtype=np.uint8)
    allowed[0, 5:5 + len(seq[0])] = [1 << c for c in seq[0]]
    allowed[0, 60:60 + len(seq[1])] = [1 << c for c in seq[1]]
    out = dfa_profile(logits, auto.delta, auto.kind, mask=mask, allowed=allowed)
    ref = PR.design_dfa_profile_ref(logits, [n], 1.0, auto.delta.numpy(), auto.kind.numpy(), allowed)
    assert ref["miss"].tolist() == [0]
    agree_profile(out, ref, "256 states, T = 120", tol=TOL)
    kind257 = np.zeros(257, dtype=np.uint8)
    with pytest.raises(ValueError, match="n_states = 257, an automaton has 1 .. 256 states"):
        dfa_profile(logits, np.zeros((257, 4), dtype=np.uint8), kind257, mask=mask, ws=workspace(1, n, 256))


def test_the_largest_extent_and_one_past_it_and_t_1616_at_73_live_states():
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.motifs import DesignAutomaton
    auto = DesignAutomaton.from_avoid((), 3)                       # 17 states, 13 live
    assert auto.n_live == 13 and _lds_bytes(T_MAX) <= 163840 < _lds_bytes(T_MAX + 1)
    logits, mask = one_rna(T_MAX, 14)
    logits[0, :, 3] += 6.0
    out = dfa_profile(logits, auto.delta, auto.kind, mask=mask)
    ref = PR.design_dfa_profile_ref(logits, [T_MAX], 1.0, auto.delta.numpy(), auto.kind.numpy())
    agree_profile(out, ref, f"T = {T_MAX}, 13 live states", tol=TOL)
    n = T_MAX + 1
    with pytest.raises(NotImplementedError, match=rf"rnampnn_design_dfa_profile: T = {n} needs {_lds_bytes(n)} bytes of LDS.*the limit is 163840 "
                                                  rf"\(T <= {T_MAX}; the table of partition sums is in the workspace"):
        dfa_profile(np.zeros((1, n, 4), dtype=np.float32), auto.delta, auto.kind, mask=np.ones((1, n), dtype=np.float32))
    auto = _automaton(R.CASE_AUTOMATA["two_run3"])
    logits, mask = one_rna(1616, 15)
    logits[0, :, 3] += 6.0
    out = dfa_profile(logits, auto.delta, auto.kind, mask=mask, temperature=0.5)
    ref = PR.design_dfa_profile_ref(logits, [1616], 0.5, auto.delta.numpy(), auto.kind.numpy())
    assert auto.n_live == 73 and ref["miss"].tolist() == [0]
    agree_profile(out, ref, "T = 1616, 73 live states", tol=TOL)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_every_bad_argument_the_partner_and_the_all_null_call_launch_nothing(case):
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    lg, m, cu = case["logits"], case["mask"], case["cu"]
    a = case["auto"]["ggagg"]
    delta, kind = a.delta.cuda(), a.kind.clone()
    dead0 = kind.clone()
    dead0[0] = 1
    ws = workspace(B, T, a.n_live)
    partner = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    out = profile_outputs(B, T)
    BAD, UNSUPPORTED = 1, 2

    def ptr(v):
        return _ptr(v) if v is None or torch.is_tensor(v) else v

    def call(logits=lg, mask=m, cu=None, B=B, T=T, temperature=1.0, delta=delta, kind=kind, n_states=a.n_states, partner=None, ws=ws, ws_bytes=None,
             bias=None, per_position=0, marginals=out["marginals"], outputs=None, n_rows=None):
        outs = [ptr(marginals)] + [_ptr(out[k]) for k in OUTPUTS[1:]] if outputs is None else outputs
        return _native.lib().rnampnn_design_dfa_profile(
            _ptr(logits), B * T if n_rows is None else n_rows, _ptr(mask), _ptr(cu), B, T, float(temperature), None, _ptr(partner), 1, ptr(bias),
            per_position, _ptr(delta), _ptr(kind), n_states, ptr(ws), C.c_size_t(ws.numel() if ws_bytes is None else ws_bytes), *outs,
            _stream(lg.device))
    for t in out.values():
        t.fill_(-7)
    keep = {k: t.clone() for k, t in out.items()}
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)
    for t in out.values():
        t.fill_(-7)
    odd = C.c_void_p(out["marginals"].data_ptr() + 8)
    bad = dict(null_logits=call(logits=None), B0=call(B=0), T0=call(T=0), no_layout=call(mask=None), both_layouts=call(cu=cu),
               temperature0=call(temperature=0.0), temperature_nan=call(temperature=float("nan")),
               bias_unaligned=call(bias=C.c_void_p(lg.data_ptr() + 4), per_position=1), null_delta=call(delta=None), null_kind=call(kind=None),
               states0=call(n_states=0), states257=call(n_states=257), states_negative=call(n_states=-1), start_dead=call(kind=dead0),
               null_workspace=call(ws=None, ws_bytes=ws.numel()), small_workspace=call(ws_bytes=ws.numel() - 1), empty_workspace=call(ws_bytes=0),
               workspace_unaligned=call(ws=C.c_void_p(ws.data_ptr() + 4), ws_bytes=ws.numel()), marginals_unaligned=call(marginals=odd))
    assert bad == {k: BAD for k in bad}, bad
    assert call(partner=partner) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match=r"rnampnn_design_dfa_profile: base pairs \(a non-null partner\) are not built together with an "
                                                  r"automaton.*4\^depth"):
        _native.check(call(partner=partner))
    with pytest.raises(ValueError, match="rnampnn_design_dfa_profile: marginals must be 16-byte aligned"):
        _native.check(call(marginals=odd))
    with pytest.raises(ValueError, match=rf"the workspace is too small \({ws.numel() - 1} bytes\).*needs {ws.numel()} "
                                         r"\(rnampnn_design_dfa_profile_workspace_bytes\)"):
        _native.check(call(ws_bytes=ws.numel() - 1))
    with pytest.raises(ValueError, match="state 0, the start, is marked dead"):
        _native.check(call(kind=dead0))
    nothing = [None] * 6
    assert call(outputs=nothing) == 0                               # every output null: RNAMPNN_OK without a launch ...
    big = 100000                                                    # ... whatever T is; with one output asked for, the LDS check
    assert call(B=1, T=big, n_rows=big, outputs=nothing, ws_bytes=8 * big * a.n_live) == 0
    assert call(B=1, T=big, n_rows=big, outputs=nothing[:4] + [_ptr(out["infeasible"]), None], ws_bytes=8 * big * a.n_live) == UNSUPPORTED
    assert call(B=1, T=big, n_rows=big, partner=partner, outputs=nothing, ws_bytes=8 * big * a.n_live) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)  # nothing was launched
    assert int(_native.lib().rnampnn_design_dfa_profile_workspace_bytes(0, T, 3)) == 0


# ---------------------------------------------------------------------------------------------------------------- the Python surface
MODEL_LENGTHS = [33, 20, 41]
RESOLVED_MODES = [dict(require=["GA"], max_run=2, table="global"), dict(avoid=["GAC"], max_run=2, table="lds"),
                  dict(gc_content=(0.4, 0.6), tree="lds"), dict(gc_content=(0.4, 0.6), tree="global")]


@pytest.mark.parametrize("own", RESOLVED_MODES, ids=["require-global", "avoid-lds", "gc-lds", "gc-global"])
def test_the_resolved_call_path_returns_the_bytes_of_the_raw_arguments(own):
    """``design_profile_from_logits`` on raw arguments and on ``resolve_profile``'s result (the path both models and the command line
    take): the same bytes in all six outputs, B = 2, T = 12, lengths (12, 5), temperatures 1.0 and 0.3, both layouts."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import design_profile_from_logits, resolve_profile
    Tn, lengths = 12, (12, 5)
    rng = np.random.RandomState(5)
    logits = torch.from_numpy((3.0 * rng.standard_normal((2, Tn, 4))).astype(np.float32)).cuda()
    mask = torch.tensor([[1.0] * n + [0.0] * (Tn - n) for n in lengths], device="cuda")
    packed = torch.cat([logits[b, :n] for b, n in enumerate(lengths)])
    cu = torch.tensor([0, 12, 17], dtype=torch.int32, device="cuda")
    tree = own.get("tree", "lds")
    resolved = resolve_profile(None, own.get("gc_content"), None, own.get("avoid"), tree, own.get("require"), own.get("table", "lds"),
                               own.get("max_run"))
    for temperature in (1.0, 0.3):
        for lg, where in ((logits, dict(mask=mask)), (packed, dict(cu_seqlens=cu, max_len=Tn))):
            raw = design_profile_from_logits(lg, temperature=temperature, **where, **own)
            got = design_profile_from_logits(lg, temperature=temperature, gc_content=own.get("gc_content"), tree=tree, resolved=resolved, **where)
            assert got.mode == raw.mode == resolved[0]
            assert all(_bytes(getattr(got, k)) == _bytes(getattr(raw, k)) for k in OUTPUTS), (own, temperature, sorted(where))
            assert bool((raw.marginals[1, 5:] == 0).all()) and abs(float(raw.marginals[0].sum()) - Tn) <= TOL * Tn


def test_design_profile_from_logits_in_both_layouts_and_both_modes(case):
    from rnampnn.model.decode import DesignProfile, design_profile_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.motifs import DesignAutomaton, MotifAutomaton
    cons = DesignConstraints(case["allowed"], None, case["bias"], True)
    want = _run(case, "gnra_run3", 0.3)
    spec = R.CASE_AUTOMATA["gnra_run3"]
    for got in (design_profile_from_logits(case["logits"], mask=case["mask"], temperature=0.3, constraints=cons, require=list(spec[0]),
                                           max_run=spec[2], table="global"),
                design_profile_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, temperature=0.3, constraints=cons,
                                           require=case["auto"]["gnra_run3"], table="global")):
        assert isinstance(got, DesignProfile) and got.mode == "require" and got.marginals.dtype == torch.float64
        assert all(_bytes(getattr(got, k)) == _bytes(want[k]) for k in OUTPUTS)
        assert _bytes(got.log_mass) == _bytes(want["log_z"] - want["log_z_free"])
    auto = DesignAutomaton.from_avoid(["GGGG", "GAAUUC"], 3)
    want = dfa_profile(case["logits"], auto.delta, auto.kind, mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
    for got in (design_profile_from_logits(case["logits"], mask=case["mask"], temperature=0.3, constraints=cons, avoid=["GGGG", "GAAUUC"],
                                           max_run=3, table="global"),
                design_profile_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, temperature=0.3, constraints=cons,
                                           avoid=MotifAutomaton.from_motifs(["GGGG", "GAAUUC"], max_run=3), table="global")):
        assert got.mode == "avoid" and all(_bytes(getattr(got, k)) == _bytes(want[k]) for k in OUTPUTS)
    lds = design_profile_from_logits(case["logits"], mask=case["mask"], temperature=0.3, constraints=cons,
                                     avoid=MotifAutomaton.from_motifs(["GGGG", "GAAUUC"], max_run=3))
    agree_profile(want, {k: getattr(lds, k) for k in OUTPUTS}, "table=global against table=lds, avoid alone", tol=TOL)      # to rounding, not to the byte
    with pytest.raises(NotImplementedError, match=rf"T = {T_MAX + 1} needs \d+ bytes of LDS.*\(T <= {T_MAX};"):
        design_profile_from_logits(torch.zeros(1, T_MAX + 1, 4, device="cuda"), mask=torch.ones(1, T_MAX + 1, device="cuda"), require=["GGAGG"],
                                   table="global")


def test_both_models_design_profile(case):
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.decode import design_profile_from_logits
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
    cons = DesignConstraints.from_specs([("GNRA" + "." * 29, None), (None, None), (None, None)], lens, Tm)
    logits = m(c, mask)
    kw = dict(require=["GGAGG", "GNRA"], avoid=["GGGG"], max_run=3, table="global")
    got = m.design_profile(c, mask, temperature=0.5, constraints=cons, **kw)
    want = design_profile_from_logits(logits, mask=mask, temperature=0.5, constraints=cons, **kw)
    assert got.mode == "require" and all(_bytes(x) == _bytes(y) for x, y in zip(got[:6], want[:6]))
    P = got.marginals.cpu().numpy()
    assert got.miss.tolist() == [0, 0, 0] and bool((got.log_mass < 0).all()) and bool((got.entropy > 0).all())
    assert all(np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL and not P[b, n:].any() for b, n in enumerate(lens))
    assert abs(P[0, 0, 3] - 1.0) <= TOL                             # the fixed G of GNRA
    got = m.design_profile(c, mask, temperature=0.5, avoid=["GGGG"], table="global")
    assert got.mode == "avoid" and got.miss.tolist() == [0, 0, 0]
    assert m.training is False
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    packed, cu, Tr = r._packed_logits(X, mask, MODEL_LENGTHS)
    got = r.design_profile(X, mask, temperature=0.5, lengths=MODEL_LENGTHS, constraints=cons, **kw)
    want = design_profile_from_logits(packed, cu_seqlens=cu, max_len=Tr, temperature=0.5, constraints=cons, **kw)
    assert got.mode == "require" and all(_bytes(x) == _bytes(y) for x, y in zip(got[:6], want[:6]))
    P = got.marginals.cpu().numpy()
    assert all(np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL and not P[b, n:].any() for b, n in enumerate(MODEL_LENGTHS))


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_writes_the_profile_of_both_families(family, tmp_path, monkeypatch):
    """--profile-out --table global --require GNRA --max-run 3, without and with --samples: the two CSVs hold, value for value, the tensors
    ``design_profile_from_logits`` returned for the batches; with --samples the designs file is the one written without the profile."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    import rnampnn.utils.predict as U
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    seen = []
    real = U.design_profile_from_logits

    def recorder(*a, **kw):
        prof = real(*a, **kw)
        seen.append((prof, kw))
        return prof
    monkeypatch.setattr(U, "design_profile_from_logits", recorder)
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--temperature", "0.7", "--batch-size", "2",
              "--bias", "G=1", "--require", "GNRA", "--max-run", "3"]
    quiet = dict(log=lambda *a: None)
    prefix = str(tmp_path / "prof")
    P.run(P.parse(common + ["--profile-out", prefix, "--table", "global"]), **quiet)                 # without --samples
    pos = list(csv.reader(open(prefix + ".positions.csv")))
    rna = list(csv.reader(open(prefix + ".rnas.csv")))
    assert pos[0] == ["pdb_id", "position", "pA", "pU", "pC", "pG"] and rna[0] == ["pdb_id", "length", "log_mass", "entropy", "infeasible", "miss"]
    order = sorted(ids)
    assert [r[0] for r in rna[1:]] == order and [int(r[1]) for r in rna[1:]] == [lens[ids.index(i)] for i in order]
    assert len(pos) == 1 + sum(lens) and len(seen) == 2 and all(p.mode == "require" and kw["resolved"][0] == "require" for p, kw in seen)
    from rnampnn.utils.motifs import DesignAutomaton                # the global table's automaton, built once for the run's batches
    assert isinstance(seen[0][1]["resolved"][2], DesignAutomaton) and seen[0][1]["resolved"][2] is seen[1][1]["resolved"][2]
    rows = {}
    for prof, _ in seen:
        lm, marg = prof.log_mass.cpu().tolist(), prof.marginals.cpu().numpy()
        for b in range(len(lm)):
            n = int(np.count_nonzero(marg[b].sum(axis=1)))
            rows[(n, lm[b])] = (marg[b, :n], float(prof.entropy[b]), int(prof.infeasible[b]), int(prof.miss[b]))
    assert len(rows) == 3
    at = 1
    for r in rna[1:]:
        n = int(r[1])
        marg, ent, bad, miss = rows[(n, float(r[2]))]
        assert float(r[3]) == ent and int(r[4]) == bad and int(r[5]) == miss == 0 and float(r[2]) < 0
        block = pos[at:at + n]
        assert np.array_equal(np.array([[float(v) for v in x[2:]] for x in block]), marg)
        at += n
    flags = ["--samples", "3", "--seed", "4"]
    P.run(P.parse(common + flags + ["--designs-out", str(tmp_path / "a.csv")]), **quiet)
    P.run(P.parse(common + flags + ["--designs-out", str(tmp_path / "b.csv"), "--profile-out", str(tmp_path / "both"), "--table", "global"]), **quiet)
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    for ext in (".positions.csv", ".rnas.csv"):
        assert open(str(tmp_path / "both") + ext, "rb").read() == open(prefix + ext, "rb").read()
