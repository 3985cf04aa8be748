"""Design profiles without a GPU: the float64 restatement of ``rnampnn_design_count_profile`` / ``rnampnn_design_avoid_profile``
(tests/_design_profile_ref.py) against an ENUMERATED joint - the marginals as sums of ``exp(path_logprob(seq))`` over every sequence, with
the draws' own restatements' ``path_logprob``, so the profile is tied to the conditionals the draws multiply - its exact properties, the
mode mapping and every new ``ValueError`` of the Python surface, and the CLI's refusals before a checkpoint is opened.

Tolerances.  Enumeration and restatement sum the same 4^n <= 65,536 terms of magnitude <= 1 in different orders: 1e-12 absolute on the
marginals.  log_z and the entropy are held to 1e-12 RELATIVE to the enumerated values.  The entropy is checked on the CENTRED twin of
every case (``_design_profile_ref.centred_*_plan``: the same distribution - its marginals equal the case's within 1e-12 - with every
position's z shifted so that its most probable class sits at 0): log_z - sum of P z and the enumerated - sum p log p are differences of
numbers of the size of log_z, which float64 cannot resolve to 1e-12 of an entropy of 0.004 next to log_z = 74 on either side; on the
twin log_z is of the size of the entropy and both sides agree to about 1e-15 relative.

What fails on the parent commit: the tests of the Python surface (the mode mapping, the refusals of ``design_profile_from_logits``, of
the models, of ``predict`` and of the CLI) - those names do not exist there.  The 43 tests that hold the NEW numpy restatement to
enumeration and to its properties run no product code and pass on any commit: they pin the yardstick of tests/test_design_profile_gpu.py,
every test of which fails on the parent."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_avoid_ref as AR  # noqa: E402
import _design_count_ref as CR  # noqa: E402
import _design_profile_ref as PR  # noqa: E402
from _design_gc_ref import lse  # noqa: E402
from rnampnn.model import decode as D  # noqa: E402
from rnampnn.utils.motifs import MotifAutomaton  # noqa: E402

TOL = 1e-12
A_, U_, C_, G_ = 0, 1, 2, 3


def _rows(n, seed):
    return (3.0 * np.random.RandomState(seed).standard_normal((n, 4))).astype(np.float32)


def _close(got, want):
    """Within 1e-12 relative (absolute below 1)."""
    return abs(got - want) <= TOL * max(1.0, abs(want))


def _relative(got, want):
    """Within 1e-12 of |want|: no floor."""
    return abs(got - want) <= TOL * abs(want)


def _hairpin(n):
    """Pairs (0, n-1), (1, n-2), (2, n-3) of an n-mer; -1 elsewhere."""
    p = np.full(n, -1, dtype=np.int32)
    for i in range(3):
        p[i], p[n - 1 - i] = n - 1 - i, i
    return p


def _count_cases():
    """(name, CountPlan arguments) of the enumerated cases: plain, G+C window, mutation budget reachable / unreachable / k_min > cap."""
    cases = []
    gc = np.full(8, 12, dtype=np.uint8)
    none = np.zeros(8, dtype=np.uint8)
    allowed = np.array([15, 0, 8, 6, 15, 3, 15, 15], dtype=np.uint8)           # an empty mask, a fixed G, IUPAC sets
    bias = np.random.RandomState(7).standard_normal((8, 4)).astype(np.float32)
    ref = np.array([0, 3, 2, 1, 1, 0, 3, 2])
    for temperature in (1.0, 0.3):
        tag = f"T{temperature}"
        cases += [
            (f"plain-free-{tag}", dict(n=5, seed=1, temperature=temperature, lo=0, hi=0, counted=none, cap=0)),
            (f"plain-masks-bias-{tag}", dict(n=6, seed=2, temperature=temperature, lo=0, hi=0, counted=none, cap=0, allowed=allowed, bias=bias)),
            (f"gc-window-{tag}", dict(n=6, seed=3, temperature=temperature, lo=2, hi=3, counted=gc, cap=6, allowed=allowed, bias=bias)),
            (f"gc-window-odd-{tag}", dict(n=5, seed=4, temperature=temperature, lo=1, hi=4, counted=gc, cap=5)),
            (f"gc-unreachable-{tag}", dict(n=4, seed=5, temperature=temperature, lo=0, hi=0, counted=gc, cap=4,
                                           allowed=np.array([8, 4, 15, 12], dtype=np.uint8))),
            (f"budget-reachable-{tag}", dict(n=6, seed=6, temperature=temperature, lo=1, hi=2, counted=CR.mutation_sets(ref), cap=2, allowed=allowed)),
            (f"budget-unreachable-{tag}", dict(n=5, seed=7, temperature=temperature, lo=0, hi=0, counted=CR.mutation_sets(ref), cap=3,
                                               allowed=np.array([2, 15, 15, 1, 15], dtype=np.uint8))),     # two fixed positions mutate: target 2
            (f"budget-kmin-above-cap-{tag}", dict(n=5, seed=8, temperature=temperature, lo=0, hi=1, counted=CR.mutation_sets(ref), cap=1,
                                                  allowed=np.array([2, 1, 15, 1, 15], dtype=np.uint8))),   # k_min = 3 > cap = 1
        ]
        for wobble in (True, False):
            cases += [
                (f"hairpin-gc-wobble{int(wobble)}-{tag}", dict(n=8, seed=9, temperature=temperature, lo=3, hi=5, counted=gc, cap=8,
                                                               partner=_hairpin(8), wobble=wobble)),
                (f"hairpin-no-cell-budget-wobble{int(wobble)}-{tag}", dict(          # the pair (0, 7) has no compatible cell: two single positions
                    n=8, seed=10, temperature=temperature, lo=0, hi=3, counted=CR.mutation_sets(ref), cap=3, partner=_hairpin(8), wobble=wobble,
                    allowed=np.array([1, 15, 15, 15, 15, 15, 15, 1], dtype=np.uint8), bias=bias)),
            ]
    return cases


COUNT_CASES = _count_cases()


def _count_plan(n, seed, temperature, lo, hi, counted, cap, allowed=None, partner=None, wobble=True, bias=None):
    return CR.CountPlan(_rows(n, seed), n, temperature, lo, hi, counted[:n], cap, None if allowed is None else allowed[:n], partner, wobble,
                        None if bias is None else bias[:n])


def _avoid_cases():
    cases = []
    bias = np.random.RandomState(11).standard_normal((6, 4)).astype(np.float32)
    for temperature in (1.0, 0.3):
        tag = f"T{temperature}"
        cases += [
            (f"max_run2-{tag}", dict(n=6, seed=21, temperature=temperature, motifs=(), max_run=2)),
            (f"overlap-{tag}", dict(n=6, seed=22, temperature=temperature, motifs=AR.CASE_AUTOMATA["overlap"][0], max_run=None, bias=bias,
                                    allowed=np.array([15, 0, 15, 9, 15, 7], dtype=np.uint8))),
            (f"fixed-stretch-spells-a-motif-{tag}", dict(n=6, seed=23, temperature=temperature, motifs=("GGA",), max_run=None,
                                                         allowed=np.array([15, 8, 8, 1, 15, 15], dtype=np.uint8))),
            (f"fixed-run-forces-neighbours-{tag}", dict(n=6, seed=24, temperature=temperature, motifs=(), max_run=2,
                                                        allowed=np.array([15, 15, 8, 8, 15, 15], dtype=np.uint8))),
        ]
    return cases


AVOID_CASES = _avoid_cases()


def _avoid_plan(n, seed, temperature, motifs, max_run, allowed=None, bias=None):
    auto = MotifAutomaton.from_motifs(list(motifs), max_run=max_run)
    logits = _rows(n, seed)
    if max_run is not None:
        logits[:, G_] += 3.0                                       # runs of G are what the free model would write
    return AR.AvoidPlan(logits, n, temperature, auto.delta.numpy(), auto.terminal, allowed, bias)


def _check_against_enumeration(plan, prof, twin, twin_prof):
    P, H, total, log_z = PR.enumerate_profile(plan)
    assert abs(total - 1.0) <= TOL                                 # the draw's conditionals form a distribution
    assert np.abs(prof.marginals - P).max() <= TOL
    assert _relative(prof.log_z, log_z), (prof.log_z, log_z)
    free = sum(lse(plan.z[t]) for t in range(plan.n))
    assert prof.log_z_free == free and prof.log_z - prof.log_z_free <= TOL * max(1.0, abs(free))       # the set drawn from is a subset
    # the entropy, on the centred twin: the same distribution, and both formulas within 1e-12 of the enumerated value, relative
    Pt, Ht, total_t, _ = PR.enumerate_profile(twin)
    assert abs(total_t - 1.0) <= TOL and np.abs(Pt - P).max() <= TOL and np.abs(twin_prof.marginals - prof.marginals).max() <= TOL
    assert twin.miss == plan.miss
    assert _relative(twin_prof.entropy, Ht), (twin_prof.entropy, Ht)


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name, kw", COUNT_CASES, ids=[c[0] for c in COUNT_CASES])
def test_count_profile_equals_the_enumerated_joint(name, kw):
    plan = _count_plan(**kw)
    if "unreachable" in name:
        assert plan.miss > 0 and plan.target is not None and not plan.at_min
    if "kmin-above-cap" in name:
        assert plan.at_min and plan.k_min > kw["cap"]
    if "no-cell" in name:
        assert plan.infeasible == 2
    prof = PR.count_profile(plan)
    twin = PR.centred_count_plan(plan, prof.marginals, kw.get("wobble", True))
    assert twin.at_min == plan.at_min and twin.target == plan.target
    _check_against_enumeration(plan, prof, twin, PR.count_profile(twin))


@pytest.mark.parametrize("name, kw", AVOID_CASES, ids=[c[0] for c in AVOID_CASES])
def test_avoid_profile_equals_the_enumerated_joint(name, kw):
    plan = _avoid_plan(**kw)
    assert plan.miss == int("spells-a-motif" in name)
    prof = PR.avoid_profile(plan)
    twin = PR.centred_avoid_plan(plan, prof.marginals)
    _check_against_enumeration(plan, prof, twin, PR.avoid_profile(twin))


# ---------------------------------------------------------------------------------------------------------------- properties
N = 41


def _big(seed=31):
    return (3.0 * np.random.RandomState(seed).standard_normal((N, 4))).astype(np.float32)


def _stem(n=N):
    p = np.full(n, -1, dtype=np.int32)
    for i in range(12):
        p[i], p[n - 2 - i] = n - 2 - i, i
    return p


@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_rows_sum_to_one_a_fixed_position_has_probability_one_and_padding_is_zero(temperature):
    allowed = np.full((1, 48), 15, dtype=np.uint8)
    allowed[0, 5], allowed[0, 17] = 1 << U_, 1 << G_
    logits = np.zeros((1, 48, 4), dtype=np.float32)
    logits[0, :N] = _big()
    counted = np.full((1, 48), 12, dtype=np.uint8)
    res = PR.design_count_profile_ref(logits, [N], temperature, counted, [18], [22], 48, allowed)
    P = res["marginals"][0]
    assert np.abs(P[:N].sum(axis=1) - 1.0).max() <= TOL and not P[N:].any()
    assert abs(P[5, U_] - 1.0) <= TOL and abs(P[17, G_] - 1.0) <= TOL and P[5, [A_, C_, G_]].max() == 0.0
    expected = (P[:N] * np.array([0, 0, 1, 1])).sum()
    assert 18 - TOL * N <= expected <= 22 + TOL * N                # the expected count lies in the reachable window
    assert res["log_z"][0] - res["log_z_free"][0] <= 0.0 and res["miss"].tolist() == [0]


@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_without_wobble_the_ends_of_a_pair_mirror_each_other(temperature):
    partner = _stem()
    ref = np.random.RandomState(5).randint(0, 4, size=N)
    for i in range(12):
        ref[partner[i]] = CR.COMPLEMENT[ref[i]]                    # the structure alone forces no mutation: the window is reachable
    plan = CR.CountPlan(_big(32), N, temperature, 2, 6, CR.mutation_sets(ref), 6, None, partner, False)
    P = PR.count_profile(plan).marginals
    assert plan.miss == 0 and plan.infeasible == 0 and np.abs(P.sum(axis=1) - 1.0).max() <= TOL
    for i in range(12):
        j = partner[i]
        assert abs(P[i, A_] - P[j, U_]) <= TOL and abs(P[i, U_] - P[j, A_]) <= TOL
        assert abs(P[i, C_] - P[j, G_]) <= TOL and abs(P[i, G_] - P[j, C_]) <= TOL
    expected = sum(P[t, c] * CR.bit(plan.counted[t], c) for t in range(N) for c in range(4))
    assert 2 - TOL * N <= expected <= 6 + TOL * N


def test_under_max_run_3_both_neighbours_of_a_fixed_ggg_have_no_g():
    auto = MotifAutomaton.from_motifs([], max_run=3)
    allowed = np.full(N, 15, dtype=np.uint8)
    allowed[20:23] = 1 << G_
    logits = _big(33)
    logits[:, G_] += 6.0
    prof = PR.avoid_profile(AR.AvoidPlan(logits, N, 1.0, auto.delta.numpy(), auto.terminal, allowed))
    P = prof.marginals
    assert P[19, G_] == 0.0 and P[23, G_] == 0.0 and np.abs(P[20:23, G_] - 1.0).max() <= TOL
    assert np.abs(P.sum(axis=1) - 1.0).max() <= TOL and prof.log_z < prof.log_z_free and prof.entropy > 0.0


@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_the_plain_mode_is_the_per_unit_closed_form_and_keeps_all_mass_without_constraints(temperature):
    logits = _big(34)
    none = np.zeros(N, dtype=np.uint8)
    free = PR.count_profile(CR.CountPlan(logits, N, temperature, 0, 0, none, 0))
    z = logits.astype(np.float64) / float(np.float32(temperature))
    soft = np.exp(z - np.array([lse(r) for r in z])[:, None])
    assert np.abs(free.marginals - soft).max() <= TOL
    assert _close(free.log_z, free.log_z_free)
    centred = PR.count_profile(PR.centred_count_plan(CR.CountPlan(logits, N, temperature, 0, 0, none, 0), free.marginals, True))
    assert np.abs(centred.marginals - soft).max() <= TOL and _relative(centred.entropy, -(soft * np.log(soft)).sum())      # (on the centred twin)
    # under masks and pairs: a single position is the softmax over its mask, a pair the softmax over its admitted compatible cells
    partner, allowed = _stem(), np.full(N, 15, dtype=np.uint8)
    allowed[0], allowed[30] = 8 | 4, 2 | 1
    plan = CR.CountPlan(logits, N, temperature, 0, 0, none, 0, allowed, partner, True)
    prof = PR.count_profile(plan)
    want, log_z = np.zeros((N, 4)), 0.0
    for t in range(N):
        if plan.kind[t] == 2:
            continue
        zz = np.array([x[1] for x in plan.cands[t]])
        log_z += lse(zz)
        PR._spread(plan, t, np.exp(zz - lse(zz)), want)
    assert np.abs(prof.marginals - want).max() <= TOL and _close(prof.log_z, log_z) and prof.log_z < prof.log_z_free
    # an avoid automaton that forbids nothing reachable (one state, no terminal) is the same free distribution
    one = PR.avoid_profile(AR.AvoidPlan(logits, N, temperature, np.zeros((1, 4), dtype=np.uint8), 0))
    assert np.abs(one.marginals - soft).max() <= TOL and _close(one.log_z, one.log_z_free)


def test_an_empty_rna_has_zero_scalars():
    for prof in (PR.count_profile(CR.CountPlan(np.zeros((0, 4), dtype=np.float32), 0, 1.0, 0, 3, np.zeros(0, dtype=np.uint8), 3)),
                 PR.avoid_profile(AR.AvoidPlan(np.zeros((0, 4), dtype=np.float32), 0, 1.0, np.zeros((1, 4), dtype=np.uint8), 0))):
        assert prof.marginals.shape == (0, 4) and (prof.log_z, prof.log_z_free, prof.entropy) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("mode", ["gc_content", "mutations", "avoid"])
def test_the_restatements_own_draws_stay_inside_the_bound_of_the_link_test(mode):
    """tests/test_design_profile_gpu.py holds the class frequencies of 4096 device draws to the device profile within
    6 sqrt(P (1 - P) / S) + 1 / S; the seed it uses keeps the restatement's own draws inside that bound of the restatement's profile."""
    for b, plan in enumerate(PR.link_plans(mode)):
        P = (PR.avoid_profile if mode == "avoid" else PR.count_profile)(plan).marginals
        seqs = np.stack([plan.draw(PR.LINK_SEED, s, b, margins=False)[0] for s in range(PR.LINK_S)])
        f = PR.frequencies(seqs)
        assert plan.miss == 0 and np.abs(P.sum(axis=1) - 1.0).max() <= TOL
        assert (np.abs(f - P) <= PR.link_bound(P)).all() and not f[P == 0].any(), (mode, b, np.abs(f - P).max())


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_the_mode_mapping():
    B, T = 3, 10
    lengths = torch.tensor([10.0, 4.0, 7.0])
    counted, lo, hi, cap = D.profile_mode_args("plain", B, T, "cpu")
    assert counted.dtype == torch.uint8 and tuple(counted.shape) == (B, T) and not counted.any() and lo.tolist() == hi.tolist() == [0] * B
    assert cap == 0 and lo.dtype == torch.int32
    counted, lo, hi, cap = D.profile_mode_args("gc_content", B, T, "cpu", lengths, gc_content=(0.4, 0.6))
    assert bool((counted == 12).all()) and cap == T and lo.tolist() == [4, 2, 3] and hi.tolist() == [6, 2, 4]
    ref = torch.tensor([[0, 1, 2, 3, -1, 4, 0, 0, 0, 0]] * B)
    counted, lo, hi, cap = D.profile_mode_args("mutations", B, T, "cpu", reference=ref, budget=(1, 3))
    assert counted[0].tolist() == [14, 13, 11, 7, 0, 0, 14, 14, 14, 14] and lo.tolist() == [1] * B and hi.tolist() == [3] * B and cap == 3
    auto = MotifAutomaton.from_motifs(["GGGG"])
    delta, n_states, terminal = D.profile_mode_args("avoid", B, T, "cpu", auto=auto)
    assert delta.tolist() == auto.delta.tolist() and n_states == 5 and terminal.value == 1 << 4
    assert set(D.PROFILE_ENTRIES) == {"plain", "gc_content", "mutations", "avoid", "require"}
    assert D.PROFILE_ENTRIES["require"] == "rnampnn_design_dfa_profile" and D.profile_entry("avoid", auto) == "rnampnn_design_avoid_profile"
    assert D.PROFILE_ENTRIES["avoid"] == "rnampnn_design_avoid_profile" and D.PROFILE_ENTRIES["gc_content"] == "rnampnn_design_count_profile"
    with pytest.raises(ValueError, match="no profile is built for the mode 'distinct'"):
        D.profile_mode_args("distinct", B, T, "cpu")
    p = D.DesignProfile(torch.zeros(1, 2, 4), torch.tensor([-3.0]), torch.tensor([-1.0]), torch.zeros(1), torch.zeros(1), torch.zeros(1), "plain")
    assert p.log_mass.tolist() == [-2.0] and p.mode == "plain" and len(p) == 7


def test_refusals_of_design_profile_from_logits_come_before_the_device():
    from rnampnn.utils.constraints import DesignConstraints
    logits, mask = torch.zeros(1, 6, 4), torch.ones(1, 6)
    ref = torch.zeros(1, 6, dtype=torch.int64)
    with pytest.raises(ValueError, match="avoid together with gc_content is not built"):
        D.design_profile_from_logits(logits, mask=mask, gc_content=(0.4, 0.6), avoid=["GGGG"])
    with pytest.raises(ValueError, match="avoid together with mutations is not built"):
        D.design_profile_from_logits(logits, mask=mask, mutations=(ref, 2), avoid=["GGGG"])
    with pytest.raises(ValueError, match="mutations together with gc_content is not built"):
        D.design_profile_from_logits(logits, mask=mask, mutations=(ref, 2), gc_content=(0.4, 0.6))
    with pytest.raises(ValueError, match="0 <= min <= max"):
        D.design_profile_from_logits(logits, mask=mask, mutations=(ref, 3, 2))
    with pytest.raises(ValueError, match=r"mutations must be \(reference, max\)"):
        D.design_profile_from_logits(logits, mask=mask, mutations=(2,))
    paired = DesignConstraints(None, torch.full((1, 6), -1, dtype=torch.int32), None, True)
    with pytest.raises(ValueError, match="drop `structure`"):
        D.design_profile_from_logits(logits, mask=mask, constraints=paired, avoid=["GGGG"])
    with pytest.raises(ValueError, match="unknown letter"):
        D.design_profile_from_logits(logits, mask=mask, avoid=["GGXG"])
    for kw in (dict(), dict(gc_content=(0.4, 0.6)), dict(mutations=(ref, 2)), dict(avoid=["GGGG"])):
        with pytest.raises(RuntimeError, match="_profile runs on an MI355X: pass CUDA logits \\(there is no CPU fallback\\)"):
            D.design_profile_from_logits(logits, mask=mask, **kw)


def test_the_models_refuse_before_their_forward():
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    m = RNAMPNN(precision="f32", num_res_neighbours=6, num_res_mpnn_layers=1)
    with pytest.raises(ValueError, match="avoid together with gc_content is not built"):
        m.design_profile(torch.zeros(1, 6, 7, 3), torch.ones(1, 6), gc_content=(0.4, 0.6), avoid=["GGGG"])
    r = RNAModel(num_mpnn_layers=1)
    with pytest.raises(ValueError, match="mutations together with gc_content is not built"):
        r.design_profile(torch.zeros(1, 6, 6, 3), torch.ones(1, 6), gc_content=(0.4, 0.6), mutations=(torch.zeros(1, 6, dtype=torch.int64), 1))


def test_predict_refuses_before_it_loads_a_model():
    from rnampnn.utils.predict import check_profile, predict
    check_profile(None, states={}, distinct="best")
    check_profile("p")
    for kw in (dict(states={}), dict(distinct="sample")):
        with pytest.raises(ValueError, match="a design profile together with states or distinct is not built"):
            predict(None, "/nonexistent", "/nonexistent/out.csv", samples=2, profile_prefix="p", **kw)


def test_cli_refusals_without_a_checkpoint(tmp_path):
    import predict as P
    base = ["--ckpt", str(tmp_path / "missing.pt"), "--data", str(tmp_path), "--profile-out", str(tmp_path / "prof")]
    (tmp_path / "states.csv").write_text("design_id,pdb_id,weight\nd,a,\n")
    quiet = dict(log=lambda *a: None)
    with pytest.raises(ValueError, match="--profile-out together with --states is not built"):
        P.run(P.parse(base + ["--samples", "2", "--states", str(tmp_path / "states.csv")]), **quiet)
    with pytest.raises(ValueError, match="--profile-out together with --distinct is not built"):
        P.run(P.parse(base + ["--samples", "2", "--distinct", "best"]), **quiet)
    with pytest.raises(ValueError, match="--avoid / --max-run together with --gc-content is not built"):
        P.run(P.parse(base + ["--avoid", "GGGG", "--gc-content", "0.4:0.6"]), **quiet)
    with pytest.raises(ValueError, match="--max-mutations together with --gc-content is not built"):
        P.run(P.parse(base + ["--max-mutations", "3", "--gc-content", "0.4:0.6"]), **quiet)
    with pytest.raises(ValueError, match="has 65 states, the limit is 64"):
        P.run(P.parse(base + ["--avoid", ",".join(list(AR.CASE_AUTOMATA["states64"][0][:-1]) + [AR.CASE_AUTOMATA["states64"][0][-1] + "A"])]), **quiet)
    # without --profile-out the modes still need --samples, with it they do not: the next failure is the missing checkpoint
    with pytest.raises(ValueError, match="--gc-content needs --samples N > 0"):
        P.run(P.parse(base[:4] + ["--gc-content", "0.4:0.6"]), **quiet)
    for flags in (["--gc-content", "0.4:0.6"], ["--max-mutations", "2"], ["--avoid", "GGGG", "--max-run", "3"], []):
        with pytest.raises(FileNotFoundError):
            P.run(P.parse(base + flags), **quiet)
    assert isinstance(P.profile_option(types.SimpleNamespace(profile_out=None, states=None, distinct=None)), dict)
