"""``rnampnn_design_count_profile`` / ``rnampnn_design_avoid_profile`` (csrc/design_profile.hip) on the device, against the float64
restatement of their contract in tests/_design_profile_ref.py, against the draw entries of the same mode (``infeasible`` / ``*_miss`` byte
for byte; the class frequencies of 4096 draws) and against themselves (layouts, batches, a captured graph, stale outputs, a NaN row).

The batches are the siblings': lengths 0, 1, 2, 3, 63, 64, 65, 257, 300 at T = 300, the count tests' inputs (``_design_count_ref.case_arrays``:
hairpin, pseudoknot, infeasible pair, fixed ends, windows that are reachable, unreachable and below k_min) with and without their
constraints, and the avoid tests' (``_design_avoid_ref.case_arrays``) under the automata max_run3, overlap and states64.

Tolerances.  Device and restatement form the same sums in another order with last-bit exp / log: marginals within 1e-8 absolute, log_z,
log_z_free and entropy within 1e-8 * max(1, |value|) - the family's own selection margin; the draw tests already rest on device and
restatement tables agreeing more closely than that.  Each test prints the maxima it observed."""
import csv
import ctypes as C
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
import _design_count_ref as CR  # noqa: E402
import _design_profile_ref as PR  # noqa: E402
from _design_case import (SMALL, PROFILE_OUTPUTS as OUTPUTS, PROFILE_SCALARS as SCALARS, agree_profile, one_rna, profile_outputs, raw_design,  # noqa: E402
                          raw_profile, same_profile, _bytes, _dev, _write_data, _checkpoint)

LENGTHS, T = CR.CASE_LENGTHS, CR.CASE_T
TOL = 1e-8
T_MAX_CAP8, T_MAX_UNCAPPED, T_MAX_RUN3, T_MAX_64 = 1457, 535, 1168, 293      # the largest T in 160 KiB of LDS (include/rnampnn_hip.h)


def count_profile(logits, counted, lo, hi, cap, wobble=CR.CASE_WOBBLE, **kw):
    return raw_profile("rnampnn_design_count_profile", (_dev(counted, torch.uint8), _dev(lo, torch.int32), _dev(hi, torch.int32), int(cap)), logits,
                    wobble=wobble, **kw)


def avoid_profile(logits, delta, n_states, terminal, **kw):
    return raw_profile("rnampnn_design_avoid_profile", (_dev(delta, torch.uint8), int(n_states), C.c_uint64(int(terminal))), logits, **kw)


def _automaton(name):
    from rnampnn.utils.motifs import MotifAutomaton
    motifs, max_run = AR.CASE_AUTOMATA[name]
    return MotifAutomaton.from_motifs(motifs, max_run=max_run)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def count_case(built):
    h = CR.case_arrays()
    d = dict(h=h, run={})
    for k in ("logits", "mask", "allowed", "partner", "packed", "cu", "lo", "hi", "counted"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


@pytest.fixture(scope="module")
def avoid_case(built):
    h = AR.case_arrays()
    d = dict(h=h, run={}, auto={name: _automaton(name) for name in AR.CASE_AUTOMATA})
    for k in ("logits", "mask", "allowed", "bias", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _count_run(case, temperature, cap, variant="hairpin", layout="padded"):
    key = (float(temperature), int(cap), variant, layout)
    if key not in case["run"]:
        kw = dict(temperature=temperature)
        if variant == "hairpin":
            kw.update(allowed=case["allowed"], partner=case["partner"])
        if layout == "padded":
            case["run"][key] = count_profile(case["logits"], case["counted"], case["lo"], case["hi"], cap, mask=case["mask"], **kw)
        else:
            case["run"][key] = count_profile(case["packed"], case["counted"], case["lo"], case["hi"], cap, cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _count_ref(temperature, cap, variant):
    h = CR.case_arrays()
    con = dict(allowed=h["allowed"], partner=h["partner"]) if variant == "hairpin" else {}
    return PR.cached(("count", float(temperature), int(cap), variant), lambda: PR.design_count_profile_ref(
        h["logits"], LENGTHS, temperature, h["counted"], h["lo"], h["hi"], cap, wobble=CR.CASE_WOBBLE, **con))


def _avoid_run(case, name, temperature, layout="padded"):
    key = (name, float(temperature), layout)
    if key not in case["run"]:
        a = case["auto"][name]
        kw = dict(temperature=temperature, allowed=case["allowed"], bias=case["bias"])
        if layout == "padded":
            case["run"][key] = avoid_profile(case["logits"], a.delta, a.n_states, a.terminal, mask=case["mask"], **kw)
        else:
            case["run"][key] = avoid_profile(case["packed"], a.delta, a.n_states, a.terminal, cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _avoid_ref(case, name, temperature):
    h, a = case["h"], case["auto"][name]
    return PR.cached(("avoid", name, float(temperature)), lambda: PR.design_avoid_profile_ref(
        h["logits"], LENGTHS, temperature, a.delta.numpy(), a.terminal, h["allowed"], h["bias"]))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("variant", ["hairpin", "free"])
@pytest.mark.parametrize("cap", CR.CASE_CAPS)
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_count_profile_equals_the_float64_restatement_and_the_draw_entrys_flags(count_case, temperature, cap, variant):
    out = _count_run(count_case, temperature, cap, variant)
    ref = _count_ref(temperature, cap, variant)
    agree_profile(out, ref, f"count, temperature {temperature}, cap {cap}, {variant}", tol=TOL)
    P = out["marginals"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert not P[b, n:].any() and (n == 0 or np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL)
    assert [float(out[k][0]) for k in SCALARS] == [0.0, 0.0, 0.0]                           # the empty RNA
    assert bool((out["log_z"] - out["log_z_free"] <= 1e-9 * out["log_z_free"].abs().clamp(min=1)).all())
    if variant == "hairpin":
        assert ref["plans"][8].at_min == (cap == 8) and ref["miss"][8] > 0 and ref["infeasible"].tolist() == CR.CASE_INFEASIBLE
    kw = dict(allowed=count_case["allowed"], partner=count_case["partner"]) if variant == "hairpin" else {}
    draw = raw_design("rnampnn_design_count", (count_case["counted"], count_case["lo"], count_case["hi"], int(cap)),
                      (("count", torch.int32, True), ("count_miss", torch.int32, False)), count_case["logits"], mask=count_case["mask"],
                      temperature=temperature, S=1, seed=1, wobble=CR.CASE_WOBBLE, **kw)
    assert _bytes(out["infeasible"]) == _bytes(draw["infeasible"]) and _bytes(out["miss"]) == _bytes(draw["count_miss"])


@pytest.mark.parametrize("name", sorted(AR.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_avoid_profile_equals_the_float64_restatement_and_the_draw_entrys_flags(avoid_case, name, temperature):
    out = _avoid_run(avoid_case, name, temperature)
    ref = _avoid_ref(avoid_case, name, temperature)
    agree_profile(out, ref, f"avoid, {name}, temperature {temperature}", tol=TOL)
    assert ref["miss"].tolist() == AR.CASE_MISS and ref["infeasible"].tolist() == AR.CASE_INFEASIBLE
    P = out["marginals"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert not P[b, n:].any() and (n == 0 or np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL)
    if name == "max_run3":                                         # both neighbours of the fixed GGG of RNA 6 are forced off G
        assert P[6, 19, 3] == 0.0 and P[6, 23, 3] == 0.0 and np.abs(P[6, 20:23, 3] - 1.0).max() <= TOL
    a = avoid_case["auto"][name]
    draw = raw_design("rnampnn_design_avoid", (a.delta.cuda(), a.n_states, C.c_uint64(a.terminal)),
                      (("hits", torch.int32, True), ("avoid_miss", torch.int32, False)), avoid_case["logits"], mask=avoid_case["mask"],
                      temperature=temperature, S=1, seed=1, allowed=avoid_case["allowed"], bias=avoid_case["bias"])
    assert _bytes(out["infeasible"]) == _bytes(draw["infeasible"]) and _bytes(out["miss"]) == _bytes(draw["avoid_miss"])


# ---------------------------------------------------------------------------------------------------------------- the link to the draws
@pytest.mark.parametrize("mode", ["gc_content", "mutations", "avoid"])
def test_the_frequencies_of_4096_draws_lie_within_six_sigma_of_the_profile(built, mode):
    """Three RNAs of 40 nt: the draw entry with S = 4096 and the profile entry on the same inputs; |f - P| <= 6 sqrt(P (1 - P) / S) + 1 / S
    on every cell and f = 0 wherever P = 0 (tests/test_design_profile_cpu.py holds the restatement's own draws to the same bound)."""
    h = PR.link_arrays()
    S, B, T = PR.LINK_S, 3, PR.LINK_T
    kw = dict(mask=h["mask"], temperature=PR.LINK_TEMPERATURE, allowed=h["allowed"])
    if mode == "avoid":
        from rnampnn.utils.motifs import MotifAutomaton
        a = MotifAutomaton.from_motifs(list(PR.LINK_AVOID[0]), max_run=PR.LINK_AVOID[1])
        own = (a.delta.cuda(), a.n_states, C.c_uint64(a.terminal))
        prof = raw_profile("rnampnn_design_avoid_profile", own, h["logits"], **kw)
        draw = raw_design("rnampnn_design_avoid", own, (("hits", torch.int32, True), ("avoid_miss", torch.int32, False)), h["logits"], S=S,
                          seed=PR.LINK_SEED, **kw)
    else:
        if mode == "gc_content":
            own = (_dev(np.full((B, T), 12, dtype=np.uint8)), _dev(np.array(PR.LINK_GC[0], dtype=np.int32)),
                   _dev(np.array(PR.LINK_GC[1], dtype=np.int32)), T)
        else:
            own = (_dev(CR.mutation_sets(h["reference"])), _dev(np.full(B, PR.LINK_BUDGET[0], dtype=np.int32)),
                   _dev(np.full(B, PR.LINK_BUDGET[1], dtype=np.int32)), PR.LINK_BUDGET[1])
        kw.update(partner=h["partner"])
        prof = raw_profile("rnampnn_design_count_profile", own, h["logits"], **kw)
        draw = raw_design("rnampnn_design_count", own, (("count", torch.int32, True), ("count_miss", torch.int32, False)), h["logits"], S=S,
                          seed=PR.LINK_SEED, **kw)
    P = prof["marginals"].cpu().numpy()
    f = PR.frequencies(draw["seqs"].cpu().numpy())
    plans = PR.link_plans(mode)
    ref = np.stack([(PR.avoid_profile if mode == "avoid" else PR.count_profile)(p).marginals for p in plans])
    print(f"{mode}: max |f - P| = {np.abs(f - P).max():.4f}, max |P - restatement| = {np.abs(P - ref).max():.3e}")
    assert prof["miss"].tolist() == [0, 0, 0] and np.abs(P - ref).max() <= TOL
    assert (np.abs(f - P) <= PR.link_bound(P)).all() and not f[P == 0].any()


# ---------------------------------------------------------------------------------------------------------------- bytes
def test_bytes_do_not_depend_on_the_layout_the_batch_a_second_call_stale_outputs_or_a_graph(count_case, avoid_case):
    a = avoid_case["auto"]["overlap"]
    delta = a.delta.cuda()                                          # (nothing is uploaded inside the capture)
    runs = [
        ("count", lambda **kw: count_profile(count_case["logits"], count_case["counted"], count_case["lo"], count_case["hi"], 8, mask=count_case["mask"],
                                             temperature=0.3, allowed=count_case["allowed"], partner=count_case["partner"], **kw),
         _count_run(count_case, 0.3, 8), _count_run(count_case, 0.3, 8, layout="packed")),
        ("avoid", lambda **kw: avoid_profile(avoid_case["logits"], delta, a.n_states, a.terminal, mask=avoid_case["mask"], temperature=0.3,
                                             allowed=avoid_case["allowed"], bias=avoid_case["bias"], **kw),
         _avoid_run(avoid_case, "overlap", 0.3), _avoid_run(avoid_case, "overlap", 0.3, "packed"))]
    for what, call, padded, packed in runs:
        assert same_profile(padded, packed), what                          # the packed layout
        out = profile_outputs(len(LENGTHS), T)
        for fill in (-7, 99):                                       # a second call, stale outputs overwritten (padding rows included)
            for t in out.values():
                t.fill_(fill)
            call(out=out)
            assert same_profile(padded, out), (what, fill)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call(out=out)
        for t in out.values():
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert same_profile(padded, out), what


def test_an_rna_alone_in_another_batch_and_a_nan_row_leave_the_bytes_unchanged(count_case, avoid_case):
    """RNA 4 of the count batch (hairpin, k_min rule at cap 8) and RNA 6 of the avoid batch alone at their row of a batch with B = 8 and
    T = 80 whose other rows are empty and hold garbage; then the full batches with RNA 7 turned into NaN: every other RNA keeps its bytes."""
    B2, T2 = 8, 80
    rng = np.random.RandomState(5)
    for what, b in (("count", 4), ("avoid", 6)):
        case = count_case if what == "count" else avoid_case
        h, n = case["h"], LENGTHS[b]
        logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
        allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
        mask = np.zeros((B2, T2), dtype=np.float32)
        logits[b, :n], allowed[b, :n], mask[b, :n] = h["logits"][b, :n], h["allowed"][b, :n], 1
        if what == "count":
            partner = rng.randint(-3, T2 + 3, size=(B2, T2)).astype(np.int32)
            counted = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
            partner[b, :n], counted[b, :n] = h["partner"][b, :n], h["counted"][b, :n]
            base = _count_run(count_case, 0.3, 8)
            one = count_profile(logits, counted, np.full(B2, h["lo"][b], dtype=np.int32), np.full(B2, h["hi"][b], dtype=np.int32), 8, mask=mask,
                                temperature=0.3, allowed=allowed, partner=partner)
        else:
            bias = rng.standard_normal((B2, T2, 4)).astype(np.float32)
            bias[b, :n] = h["bias"][b, :n]
            a = avoid_case["auto"]["max_run3"]
            base = _avoid_run(avoid_case, "max_run3", 0.3)
            one = avoid_profile(logits, a.delta, a.n_states, a.terminal, mask=mask, temperature=0.3, allowed=allowed, bias=bias)
        assert _bytes(one["marginals"][b, :n]) == _bytes(base["marginals"][b, :n]) and not bool(one["marginals"][b, n:].any()), what
        assert all(_bytes(one[k][b]) == _bytes(base[k][b]) for k in OUTPUTS[1:]), what
        others = [r for r in range(B2) if r != b]
        assert not bool(one["marginals"][others].any()) and all(float(one[k][others].abs().max()) == 0.0 for k in SCALARS), what
        # a NaN row inside the full batch
        nan = case["logits"].clone()
        nan[7, 5] = float("nan")
        nan[7, 100, 2] = float("inf")
        rows = [r for r in range(len(LENGTHS)) if r != 7]
        if what == "count":
            out = count_profile(nan, case["counted"], case["lo"], case["hi"], 8, mask=case["mask"], temperature=0.3, allowed=case["allowed"],
                                partner=case["partner"])
        else:
            out = avoid_profile(nan, a.delta, a.n_states, a.terminal, mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
        torch.cuda.synchronize()
        assert same_profile(out, base, rows), what
        assert not bool(out["marginals"][7, LENGTHS[7]:].any())      # the padding of the NaN row is still written as 0


def test_the_plain_mode_equals_the_gc_mode_with_the_window_0_1(built):
    """``design_profile_from_logits`` without a mode (nothing counted, window (0, 0), cap 0) and with ``gc_content=(0, 1)`` (C|G counted,
    every count admitted, cap T) describe the same distribution: marginals, log_z, log_z_free and entropy within 1e-12, absolute."""
    from rnampnn.model.decode import design_profile_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    h = PR.link_arrays()
    lg, m = _dev(h["logits"]), _dev(h["mask"])
    m[0, 33:], m[2, 1:] = 0, 0                                      # lengths 33, 40, 1
    cons = DesignConstraints(_dev(h["allowed"]), _dev(h["partner"]), None, True)
    plain = design_profile_from_logits(lg, mask=m, temperature=1.0, constraints=cons)
    gc = design_profile_from_logits(lg, mask=m, temperature=1.0, constraints=cons, gc_content=(0.0, 1.0))
    assert plain.mode == "plain" and gc.mode == "gc_content" and gc.miss.tolist() == plain.miss.tolist() == [0, 0, 0]
    dm = float((plain.marginals - gc.marginals).abs().max())
    ds = [float((getattr(plain, k) - getattr(gc, k)).abs().max()) for k in SCALARS]
    print(f"plain vs G+C (0, 1): max |dP| = {dm:.3e}, absolute differences of the scalars {ds}, entropies {gc.entropy.tolist()}")
    assert dm <= 1e-12 and max(ds) <= 1e-12 and _bytes(plain.infeasible) == _bytes(gc.infeasible)
    assert bool((plain.log_mass <= 0).all()) and float(plain.log_mass[2]) == 0.0       # the 1-mer is unconstrained


# ---------------------------------------------------------------------------------------------------------------- the LDS edges
@pytest.mark.parametrize("cap, n", [(8, T_MAX_CAP8), (1 << 20, T_MAX_UNCAPPED)])
def test_the_largest_extent_of_the_count_profile_and_one_past_it(built, cap, n):
    logits, mask = one_rna(n, 12)
    ref_seq = np.random.RandomState(13).randint(0, 4, size=(1, n))
    counted = CR.mutation_sets(ref_seq) if cap == 8 else np.full((1, n), 12, dtype=np.uint8)
    lo, hi = ([2], [8]) if cap == 8 else ([n // 2 - 5], [n // 2 + 5])
    out = count_profile(logits, counted, np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), cap, mask=mask)
    ref = PR.design_count_profile_ref(logits, [n], 1.0, counted, lo, hi, min(cap, n), wobble=CR.CASE_WOBBLE)
    agree_profile(out, ref, f"count, T = {n}, cap {cap}", tol=TOL)
    with pytest.raises(NotImplementedError, match=rf"T = {n + 1} at count_cap = {cap} needs \d+ bytes of LDS.*the limit is 163840 \(T <= {n} at that cap\)"):
        count_profile(np.zeros((1, n + 1, 4), dtype=np.float32), np.zeros((1, n + 1), dtype=np.uint8), [0], [0], cap,
                      mask=np.ones((1, n + 1), dtype=np.float32))


@pytest.mark.parametrize("live, n", [(13, T_MAX_RUN3), (64, T_MAX_64)])
def test_the_largest_extent_of_the_avoid_profile_and_one_past_it(built, live, n):
    if live == 13:
        a = _automaton("max_run3")
        delta, n_states, terminal = a.delta.numpy(), a.n_states, a.terminal
    else:                                                          # 64 live states: a counter of the position modulo 64 that also reads the class
        delta = np.array([[(s + 1 + c) % 64 for c in range(4)] for s in range(64)], dtype=np.uint8)
        n_states, terminal = 64, 0
    logits, mask = one_rna(n, 14)
    logits[0, :, 3] += 6.0
    out = avoid_profile(logits, delta, n_states, terminal, mask=mask)
    ref = PR.design_avoid_profile_ref(logits, [n], 1.0, delta, terminal)
    agree_profile(out, ref, f"avoid, T = {n}, {live} live states", tol=TOL)
    with pytest.raises(NotImplementedError, match=rf"T = {n + 1} with {live} live states needs \d+ bytes of LDS.*the limit is 163840 \(T <= {n} at this automaton\)"):
        avoid_profile(np.zeros((1, n + 1, 4), dtype=np.float32), delta, n_states, terminal, mask=np.ones((1, n + 1), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_every_bad_argument_and_the_partner_of_the_avoid_profile_launch_nothing(count_case, avoid_case):
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    B = len(LENGTHS)
    lg, m, cu = count_case["logits"], count_case["mask"], count_case["cu"]
    a = avoid_case["auto"]["max_run3"]
    delta = a.delta.cuda()
    partner = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    out = profile_outputs(B, T)
    BAD, UNSUPPORTED = 1, 2

    def ptr(v):
        return _ptr(v) if v is None or torch.is_tensor(v) else v

    def count(logits=lg, mask=m, cu=None, B=B, T=T, temperature=1.0, counted=count_case["counted"], lo=count_case["lo"], hi=count_case["hi"], cap=8,
              bias=None, per_position=0, marginals=out["marginals"]):
        return _native.lib().rnampnn_design_count_profile(
            _ptr(logits), B * T, _ptr(mask), _ptr(cu), B, T, float(temperature), None, None, 0, ptr(bias), per_position, _ptr(counted), _ptr(lo),
            _ptr(hi), cap, ptr(marginals), *[_ptr(out[k]) for k in OUTPUTS[1:]], _stream(lg.device))

    def avoid(logits=lg, mask=m, cu=None, B=B, T=T, temperature=1.0, delta=delta, n_states=a.n_states, terminal=a.terminal, partner=None,
              marginals=out["marginals"]):
        return _native.lib().rnampnn_design_avoid_profile(
            _ptr(logits), B * T, _ptr(mask), _ptr(cu), B, T, float(temperature), None, _ptr(partner), 1, None, 0, _ptr(delta), n_states,
            C.c_uint64(terminal), ptr(marginals), *[_ptr(out[k]) for k in OUTPUTS[1:]],
            _stream(lg.device))
    for call in (count, avoid):
        for t in out.values():
            t.fill_(-7)
        keep = {k: t.clone() for k, t in out.items()}
        assert call() == 0
        torch.cuda.synchronize()
        assert not any(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)
    for t in out.values():
        t.fill_(-7)
    keep = {k: t.clone() for k, t in out.items()}
    odd = C.c_void_p(out["marginals"].data_ptr() + 8)
    bad = dict(null_logits=count(logits=None), B0=count(B=0), T0=count(T=0), no_layout=count(mask=None), both_layouts=count(cu=cu),
               temperature0=count(temperature=0.0), temperature_nan=count(temperature=float("nan")), null_counted=count(counted=None),
               null_lo=count(lo=None), null_hi=count(hi=None), cap_negative=count(cap=-1), marginals_unaligned=count(marginals=odd),
               bias_unaligned=count(bias=C.c_void_p(lg.data_ptr() + 4), per_position=1),
               a_null_logits=avoid(logits=None), a_B0=avoid(B=0), a_T0=avoid(T=0), a_no_layout=avoid(mask=None), a_both_layouts=avoid(cu=cu),
               a_temperature0=avoid(temperature=0.0), a_null_delta=avoid(delta=None), a_states0=avoid(n_states=0), a_states65=avoid(n_states=65),
               a_states_negative=avoid(n_states=-1), a_start_terminal=avoid(terminal=a.terminal | 1), a_marginals_unaligned=avoid(marginals=odd))
    assert bad == {k: BAD for k in bad}, bad
    assert avoid(partner=partner) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match="base pairs .* are not built together with forbidden motifs.*4\\^depth"):
        _native.check(avoid(partner=partner))
    with pytest.raises(ValueError, match="rnampnn_design_count_profile: count_cap = -1 is negative"):
        _native.check(count(cap=-1))
    torch.cuda.synchronize()
    assert all(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)                 # nothing was launched
    # every output null: RNAMPNN_OK without a launch
    lib = _native.lib()
    assert lib.rnampnn_design_count_profile(_ptr(lg), B * T, _ptr(m), None, B, T, 1.0, None, None, 0, None, 0, _ptr(count_case["counted"]),
                                            _ptr(count_case["lo"]), _ptr(count_case["hi"]), 8, None, None, None, None, None, None,
                                            _stream(lg.device)) == 0
    assert lib.rnampnn_design_avoid_profile(_ptr(lg), B * T, _ptr(m), None, B, T, 1.0, None, None, 1, None, 0, _ptr(delta), a.n_states,
                                            C.c_uint64(a.terminal), None, None, None, None, None, None, _stream(lg.device)) == 0
    # ... in both entries alike before the LDS check: an extent no tree or table fits is still RNAMPNN_OK when nothing is asked for
    big = 100000
    assert lib.rnampnn_design_count_profile(_ptr(lg), big, _ptr(m), None, 1, big, 1.0, None, None, 0, None, 0, _ptr(count_case["counted"]),
                                            _ptr(count_case["lo"]), _ptr(count_case["hi"]), big, None, None, None, None, None, None,
                                            _stream(lg.device)) == 0
    assert lib.rnampnn_design_avoid_profile(_ptr(lg), big, _ptr(m), None, 1, big, 1.0, None, None, 1, None, 0, _ptr(delta), a.n_states,
                                            C.c_uint64(a.terminal), None, None, None, None, None, None, _stream(lg.device)) == 0
    assert lib.rnampnn_design_avoid_profile(_ptr(lg), big, _ptr(m), None, 1, big, 1.0, None, _ptr(partner), 1, None, 0, _ptr(delta), a.n_states,
                                            C.c_uint64(a.terminal), None, None, None, None, None, None, _stream(lg.device)) == UNSUPPORTED
    assert lib.rnampnn_design_avoid_profile(_ptr(lg), big, _ptr(m), None, 1, big, 1.0, None, None, 1, None, 0, _ptr(delta), a.n_states,
                                            C.c_uint64(a.terminal), None, None, None, None, _ptr(out["infeasible"]), None,
                                            _stream(lg.device)) == UNSUPPORTED      # one output asked for: the LDS check


# ---------------------------------------------------------------------------------------------------------------- the Python surface
MODEL_LENGTHS = [33, 20, 41]


def test_design_profile_from_logits_in_both_layouts_and_every_mode(count_case, avoid_case):
    from rnampnn.model.decode import DesignProfile, design_profile_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    h = count_case["h"]
    cons = DesignConstraints(count_case["allowed"], count_case["partner"], None, CR.CASE_WOBBLE)
    ref = torch.from_numpy(h["reference"]).cuda()
    want = count_profile(count_case["logits"], count_case["counted"], np.zeros(len(LENGTHS), dtype=np.int32), np.full(len(LENGTHS), 3, dtype=np.int32), 3,
                         mask=count_case["mask"], temperature=0.3, allowed=count_case["allowed"], partner=count_case["partner"])
    for got in (design_profile_from_logits(count_case["logits"], mask=count_case["mask"], temperature=0.3, constraints=cons, mutations=(ref, 3)),
                design_profile_from_logits(count_case["packed"], cu_seqlens=count_case["cu"], max_len=T, temperature=0.3, constraints=cons,
                                           mutations=(ref, 0, 3))):
        assert isinstance(got, DesignProfile) and got.mode == "mutations" and got.marginals.dtype == torch.float64
        assert all(_bytes(getattr(got, k)) == _bytes(want[k]) for k in OUTPUTS)
        assert _bytes(got.log_mass) == _bytes(want["log_z"] - want["log_z_free"])
    a = avoid_case["auto"]["overlap"]
    cons = DesignConstraints(avoid_case["allowed"], None, avoid_case["bias"], True)
    want = _avoid_run(avoid_case, "overlap", 0.3)
    for got in (design_profile_from_logits(avoid_case["logits"], mask=avoid_case["mask"], temperature=0.3, constraints=cons, avoid=a),
                design_profile_from_logits(avoid_case["packed"], cu_seqlens=avoid_case["cu"], max_len=T, temperature=0.3, constraints=cons,
                                           avoid=AR.CASE_AUTOMATA["overlap"][0])):
        assert got.mode == "avoid" and all(_bytes(getattr(got, k)) == _bytes(want[k]) for k in OUTPUTS)
    with pytest.raises(NotImplementedError, match=r"T = 536 at count_cap = 536 needs \d+ bytes of LDS.*\(T <= 535 at that cap\)"):
        design_profile_from_logits(torch.zeros(1, 536, 4, device="cuda"), mask=torch.ones(1, 536, device="cuda"), gc_content=(0.4, 0.6))


def test_both_models_design_profile(built):
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
    cons = DesignConstraints.from_specs([("GNRA" + "." * 29, "((((....))))" + "." * 21), (None, None), (None, None)], lens, Tm)
    logits = m(c, mask)
    ref = torch.from_numpy(np.stack([np.pad(y, (0, Tm - len(y)), constant_values=-1) for _, y in items])).cuda()
    for kw in (dict(), dict(gc_content=(0.45, 0.6)), dict(mutations=(ref, 4))):
        got = m.design_profile(c, mask, temperature=0.5, constraints=cons, **kw)
        want = design_profile_from_logits(logits, mask=mask, temperature=0.5, constraints=cons, **kw)
        assert got.mode == want.mode and all(_bytes(x) == _bytes(y) for x, y in zip(got[:6], want[:6])), kw
        P = got.marginals.cpu().numpy()
        assert all(np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL and not P[b, n:].any() for b, n in enumerate(lens))
        assert bool((got.log_mass <= 0).all())
        assert abs(P[0, 0, 3] - 1.0) <= TOL and bool((got.entropy > 0).all())              # the fixed G of GNRA
    free = m.design_profile(c, mask, temperature=0.5)
    assert free.mode == "plain" and float(free.log_mass.abs().max()) <= 1e-9 * float(free.log_z.abs().max())
    got = m.design_profile(c, mask, temperature=0.5, avoid=["GGGG"])
    assert got.mode == "avoid" and got.miss.tolist() == [0, 0, 0] and bool((got.log_mass <= 0).all())
    with pytest.raises(ValueError, match="drop `structure`"):
        m.design_profile(c, mask, constraints=cons, avoid=["GGGG"])
    assert m.training is False
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    packed, cu, Tr = r._packed_logits(X, mask, MODEL_LENGTHS)
    for kw in (dict(constraints=cons), dict(constraints=cons, gc_content=(0.45, 0.6)), dict(avoid=["GGGG"], constraints=None)):
        got = r.design_profile(X, mask, temperature=0.5, lengths=MODEL_LENGTHS, **kw)
        want = design_profile_from_logits(packed, cu_seqlens=cu, max_len=Tr, temperature=0.5, **kw)
        assert got.mode == want.mode and all(_bytes(x) == _bytes(y) for x, y in zip(got[:6], want[:6])), kw
        P = got.marginals.cpu().numpy()
        assert all(np.abs(P[b, :n].sum(axis=1) - 1.0).max() <= TOL and not P[b, n:].any() for b, n in enumerate(MODEL_LENGTHS))


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_writes_the_profile_of_both_families(family, tmp_path, monkeypatch):
    """--profile-out with and without --samples, in the plain, G+C, mutation and avoid modes: the two CSVs hold, value for value, the
    tensors ``design_profile_from_logits`` returned for the batches, one row per nucleotide and per structure, in id order; the designs
    file is byte for byte the one written without the flag."""
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
        seen.append(prof)
        return prof
    monkeypatch.setattr(U, "design_profile_from_logits", recorder)
    (tmp_path / "cons.csv").write_text("pdb_id,fixed,structure\nr2,GNRA" + "." * 29 + ",\n")
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--temperature", "0.7", "--batch-size", "2",
              "--bias", "G=1", "--constraints", str(tmp_path / "cons.csv")]
    quiet = dict(log=lambda *a: None)
    modes = {"plain": [], "gc": ["--gc-content", "0.4:0.6"], "mut": ["--max-mutations", "5", "--min-mutations", "1"],
             "avoid": ["--avoid", "GAAUUC", "--max-run", "2", "--omit", "", "--no-wobble"]}
    for name, flags in modes.items():
        seen.clear()
        prefix = str(tmp_path / f"prof_{name}")
        P.run(P.parse(common + flags + ["--profile-out", prefix]), **quiet)             # without --samples
        pos = list(csv.reader(open(prefix + ".positions.csv")))
        rna = list(csv.reader(open(prefix + ".rnas.csv")))
        assert pos[0] == ["pdb_id", "position", "pA", "pU", "pC", "pG"] and rna[0] == ["pdb_id", "length", "log_mass", "entropy", "infeasible", "miss"]
        order = sorted(ids)
        assert [r[0] for r in rna[1:]] == order and [int(r[1]) for r in rna[1:]] == [lens[ids.index(i)] for i in order]
        assert len(pos) == 1 + sum(lens) and [r[0] for r in pos[1:]] == [i for i in order for _ in range(lens[ids.index(i)])]
        rows = {}                                                   # (length, log_mass) -> the tensors of that structure
        for prof in seen:
            lm, marg = prof.log_mass.cpu().tolist(), prof.marginals.cpu().numpy()
            for b in range(len(lm)):
                n = int(np.count_nonzero(marg[b].sum(axis=1)))
                rows[(n, lm[b])] = (marg[b, :n], float(prof.entropy[b]), int(prof.infeasible[b]), int(prof.miss[b]))
        assert len(rows) == 3 and len(seen) == 2                    # two batches of at most two structures
        at = 1
        for r in rna[1:]:
            n = int(r[1])
            marg, ent, bad, miss = rows[(n, float(r[2]))]
            assert float(r[3]) == ent and int(r[4]) == bad and int(r[5]) == miss
            assert float(r[2]) <= 1e-10                              # <= 0 but for the rounding of two sums of n <= 41 terms below 4000, added in different orders
            block = pos[at:at + n]
            assert [int(x[1]) for x in block] == list(range(1, n + 1))
            assert np.array_equal(np.array([[float(v) for v in x[2:]] for x in block]), marg)
            at += n
        if name == "plain":
            g_row = [x for x in pos[1:] if x[0] == "r2" and x[1] == "1"][0]
            assert abs(float(g_row[5]) - 1.0) <= TOL                # the fixed G of GNRA
    # with --samples: the designs file is what it is without --profile-out, and the profile what it is without --samples
    flags = modes["avoid"] + ["--samples", "3", "--seed", "4"]
    P.run(P.parse(common + flags + ["--designs-out", str(tmp_path / "a.csv")]), **quiet)
    P.run(P.parse(common + flags + ["--designs-out", str(tmp_path / "b.csv"), "--profile-out", str(tmp_path / "both")]), **quiet)
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    for ext in (".positions.csv", ".rnas.csv"):
        assert open(str(tmp_path / "both") + ext, "rb").read() == open(str(tmp_path / "prof_avoid") + ext, "rb").read()
