"""The host side of design profiles under required motifs, without a GPU: the float64 restatement of ``rnampnn_design_dfa_profile``
(tests/_design_dfa_profile_ref.py) against an enumeration over all 4^n sequences, its row sums on the device tests' batch, and the
Python surface of ``table=``: every new ``ValueError`` of ``design_profile_from_logits``, of the two models (before their forward pass)
and of the CLI (before a checkpoint is opened) - and every refusal that stands without ``table``, word for word."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_dfa_profile_ref as PR  # noqa: E402
import _design_dfa_ref as R  # noqa: E402
from rnampnn.model import decode as D  # noqa: E402
from rnampnn.utils import motifs as M  # noqa: E402

ENUM_TOL = 1e-12            # the restatement against the enumeration: two float64 sums of at most 4^8 terms of size <= 1


def _auto(require, avoid=(), max_run=None):
    return M.DesignAutomaton.from_motifs(require, avoid, max_run)


def _logits(n, seed=0):
    rng = np.random.RandomState(20250301 + seed)
    return (3.0 * rng.standard_normal((max(n, 1), 4))).astype(np.float32)


# (the automaton, n, temperature, allowed or None): two case automata, two short required words that fit n = 7 together, a fixed and an
# IUPAC position, an RNA that cannot hold the motif
ENUM_CASES = [(R.CASE_AUTOMATA["ggagg"], 7, 1.0, None),
              (R.CASE_AUTOMATA["ggagg"], 5, 0.3, None),
              (R.CASE_AUTOMATA["gnra_run3"], 7, 1.0, None),
              (R.CASE_AUTOMATA["gnra_run3"], 8, 0.3, None),
              ((("GGA", "CU"), (), None), 7, 1.0, None),
              ((("GGA", "CU"), ("AA",), 2), 8, 0.5, None),
              ((("GGA",), (), None), 7, 1.0, {2: 8, 4: 5, 5: 0}),        # position 2 fixed to G, 4 is IUPAC M (A|C), 5 empty: drawn free
              ((("GGAGG",), (), None), 7, 1.0, {3: 7}),                  # no G at 3: GGAGG fits nowhere in 7 nt - a miss
              ((("GGAGG",), (), None), 4, 1.0, None)]                    # shorter than the motif - a miss


@pytest.mark.parametrize("spec, n, temperature, fixed", ENUM_CASES)
def test_the_restatement_is_the_enumeration_over_all_sequences(spec, n, temperature, fixed):
    auto = _auto(*spec)
    allowed = np.full(n, 15, dtype=np.uint8)
    for t, m in (fixed or {}).items():
        allowed[t] = m
    plan = R.DfaPlan(_logits(n, n), n, temperature, auto.delta.numpy(), auto.kind.numpy(), allowed)
    prof = PR.dfa_profile(plan)
    P, H, log_z, count = PR.enumerate_dfa_profile(plan)
    assert (count == 0) == bool(plan.miss)
    assert np.abs(prof.marginals - P).max() <= ENUM_TOL
    assert abs(prof.log_z - log_z) <= ENUM_TOL * max(1.0, abs(log_z))
    assert abs(prof.entropy - H) <= 1e-10 * max(1.0, abs(log_z))   # log_z - sum P z carries the rounding of numbers of the size of log_z
    assert np.abs(prof.marginals.sum(axis=1) - 1.0).max() <= ENUM_TOL
    assert prof.log_z <= prof.log_z_free + 1e-12
    if plan.miss:
        assert np.array_equal(prof.marginals == 0, ((plan.mask[:, None] >> np.arange(4)) & 1) == 0)


@pytest.mark.parametrize("accepts", [True, False])
def test_length_0(accepts):
    """log_z = log_z_free = entropy = 0; miss = !(state 0 accepts): an avoid-only automaton accepts the empty sequence, a required motif
    does not."""
    auto = M.DesignAutomaton.from_avoid((), 3) if accepts else _auto(("GGAGG",))
    res = PR.design_dfa_profile_ref(np.zeros((1, 4, 4), dtype=np.float32), [0], 1.0, auto.delta.numpy(), auto.kind.numpy())
    assert int(res["miss"][0]) == (0 if accepts else 1)
    assert res["log_z"][0] == 0 and res["log_z_free"][0] == 0 and res["entropy"][0] == 0 and not res["marginals"].any()


@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_every_row_of_the_case_batch_sums_to_one(name, temperature):
    """The margin of the device tests' 1e-8: on their batch (up to 300 nt) every marginal row of the restatement sums to 1 within 16
    roundings of a number of the size of log_z (a row's terms are exp(alpha + z + l - log_z): sums of three numbers of that size, each
    of which carries the roundings of its own recursion) - 1.5e-11 at the largest |log_z| here, 7,000: three decades below 1e-8."""
    auto = _auto(*R.CASE_AUTOMATA[name])
    h = R.case_arrays()
    res = PR.design_dfa_profile_ref(h["logits"], R.CASE_LENGTHS, temperature, auto.delta.numpy(), auto.kind.numpy(), h["allowed"], h["bias"])
    assert list(res["miss"]) == R.CASE_MISS and list(res["infeasible"]) == R.CASE_INFEASIBLE
    for b, n in enumerate(R.CASE_LENGTHS):
        assert np.abs(res["marginals"][b, :n].sum(axis=1) - 1.0).max(initial=0.0) <= 16 * np.spacing(max(1.0, abs(res["log_z"][b])))
        assert 16 * np.spacing(max(1.0, abs(res["log_z"][b]))) < 2e-11
        assert not res["marginals"][b, n:].any()
    assert np.all(res["log_z"] <= res["log_z_free"] + 1e-9)


def test_an_avoid_only_automaton_is_the_avoid_restatement():
    """The anchor of the device test, on the host: with every live state accepting the profile is ``_design_profile_ref.avoid_profile``."""
    import _design_avoid_ref as AV
    import _design_profile_ref as P
    mot = M.MotifAutomaton.from_motifs(["GGGG", "GAAUUC"], max_run=3)
    auto = M.DesignAutomaton.from_avoid(mot)
    lg = _logits(40, 3)
    want = P.avoid_profile(AV.AvoidPlan(lg, 40, 0.5, mot.delta.numpy(), mot.terminal))
    got = PR.dfa_profile(R.DfaPlan(lg, 40, 0.5, auto.delta.numpy(), auto.kind.numpy()))
    assert np.abs(got.marginals - want.marginals).max() <= 1e-12
    assert abs(got.log_z - want.log_z) <= 1e-12 * abs(want.log_z) and abs(got.entropy - want.entropy) <= 1e-10 * abs(want.log_z)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def _paired():
    from rnampnn.utils.constraints import DesignConstraints
    return DesignConstraints.from_specs([("GNRA....", "((....))")], [8], 8)


NEW_ERRORS = [(dict(require=["GGAGG"]), r'a design profile together with require needs table="global"'),
              (dict(require=["GGAGG"], table="lds"), r'needs table="global"'),
              (dict(table="global"), r'table="global" needs avoid and / or require'),
              (dict(table="global", max_run=3), r'table="global" needs avoid and / or require'),
              (dict(table="global", require=["GGAGG"], gc_content=(0.4, 0.6)), r'table="global" together with gc_content is not built'),
              (dict(table="global", avoid=["GGGG"], gc_content=(0.4, 0.6)), r'table="global" together with gc_content is not built'),
              (dict(table="global", require=["GGAGG"], mutations=(torch.zeros(1, 8, dtype=torch.int32), 2)),
               r'table="global" together with mutations is not built'),
              (dict(table="global", require=["GGAGG"], tree="global"), r"table=\"global\" together with tree='global' is not built"),
              (dict(table="global", avoid=["GGGG"], tree="auto"), r"table=\"global\" together with tree='auto' is not built"),
              (dict(table="global", require=["GGAGG"], constraints="paired"), r"require together with base pairs is not built"),
              (dict(table="global", avoid=["GGGG"], constraints="paired"), r"avoid together with base pairs is not built"),
              (dict(table="auto", avoid=["GGGG"]), r"table must be one of \['lds', 'global'\], got 'auto'"),
              (dict(table="hbm", require=["GGAGG"]), r"table must be one of"),
              (dict(table="global", require=[]), r"require is empty"),
              (dict(table="global", require=["GXA"]), r"unknown letter 'X'")]


@pytest.mark.parametrize("kw, match", NEW_ERRORS)
def test_design_profile_from_logits_refuses_before_any_device_work(monkeypatch, kw, match):
    from rnampnn import _native
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the library was loaded"))
    kw = dict(kw)
    if kw.get("constraints") == "paired":
        kw["constraints"] = _paired()
    with pytest.raises(ValueError, match=match):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), **kw)
    with pytest.raises(ValueError, match=match):
        D.resolve_profile(kw.get("constraints"), kw.get("gc_content"), kw.get("mutations"), kw.get("avoid"), kw.get("tree", "lds"),
                          kw.get("require"), kw.get("table", "lds"), kw.get("max_run"))


def test_table_global_reaches_the_device_check_with_the_automaton_it_documents(monkeypatch):
    """What is built passes every host check and stops at "CUDA logits only"; the automaton is ``check_require``'s with ``require`` and
    ``DesignAutomaton.from_avoid``'s without."""
    for kw in (dict(require=["GGAGG", "GNRA"], avoid=["GGGG"], max_run=3), dict(avoid=["GGGG"], max_run=3),
               dict(avoid=M.MotifAutomaton.from_motifs(["GGGG"])), dict(require=_auto(("GGAGG",)))):
        with pytest.raises(RuntimeError, match="rnampnn_design_dfa_profile runs on an MI355X"):
            D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), table="global", **kw)
    auto = D.check_table("global", None, None, None, ["GGGG"], None, 3)
    assert isinstance(auto, M.DesignAutomaton) and auto.n_states == 17 and auto.n_live == 13 and auto.required == ()
    assert bool(((auto.kind == M.KIND_DEAD) | (auto.kind == M.KIND_ACCEPTING)).all())
    auto = D.check_table("global", None, None, None, ["GGGG"], ["GGAGG"], 3)
    assert len(auto.required) == 1 and auto.letters() == ["AAAA", "UUUU", "CCCC", "GGGG"]
    assert D.check_table("lds", None, (0.4, 0.6), None, ["GGGG"]) is None
    assert D.resolve_profile(None, None, None, ["GGGG"], "lds", ["GGAGG"], "global")[0] == "require"
    assert D.resolve_profile(None, None, None, ["GGGG"], "lds", None, "global")[0] == "avoid"
    assert D.TABLES == ("lds", "global")


def test_the_resolved_call_path_builds_the_automaton_once(monkeypatch):
    """``resolve_profile`` returns what ``design_profile_from_logits`` consumes: with its result passed on as ``resolved`` the subset
    construction runs once per call (twice before the resolver returned it), and the call gets as far as the device check."""
    built = []
    for name in ("from_motifs", "from_avoid"):
        real = getattr(M.DesignAutomaton, name).__func__
        monkeypatch.setattr(M.DesignAutomaton, name, classmethod(lambda cls, *a, _real=real, _name=name, **k: built.append(_name) or _real(cls, *a, **k)))
    resolved = D.resolve_profile(require=["GA"], max_run=2, table="global")
    assert resolved[0] == "require" and isinstance(resolved[2], M.DesignAutomaton) and resolved[1] is None
    with pytest.raises(RuntimeError, match="rnampnn_design_dfa_profile runs on an MI355X"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), resolved=resolved)
    assert built == ["from_motifs"]
    del built[:]
    resolved = D.resolve_profile(avoid=["GGGG"], max_run=2, table="global")
    with pytest.raises(RuntimeError, match="rnampnn_design_dfa_profile runs on an MI355X"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), resolved=resolved)
    assert built == ["from_avoid"] and resolved[0] == "avoid" and isinstance(resolved[2], M.DesignAutomaton)


def test_without_table_every_refusal_stands_word_for_word():
    with pytest.raises(ValueError, match="tree='auto' together with avoid is not built: only the count trees of the plain, gc_content and "
                                         "mutations profiles have a home in global memory"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), avoid=["GGGG"], tree="auto")
    with pytest.raises(ValueError, match="avoid together with gc_content is not built"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), avoid=["GGGG"], gc_content=(0.4, 0.6))
    with pytest.raises(ValueError, match="avoid together with base pairs is not built"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), avoid=["GGGG"], constraints=_paired())
    with pytest.raises(RuntimeError, match="rnampnn_design_avoid_profile runs on an MI355X"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), avoid=["GGGG"])
    with pytest.raises(RuntimeError, match="rnampnn_design_count_profile runs on an MI355X"):
        D.design_profile_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), table="lds")


def test_the_models_refuse_before_their_forward_pass(monkeypatch):
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    for cls in (RNAMPNN, RNAModel):
        ran = []
        for name in ("_run", "_packed_logits"):
            if hasattr(cls, name):
                monkeypatch.setattr(cls, name, lambda *a, **k: ran.append(1) or pytest.fail("the forward pass ran"))
        model = cls.__new__(cls)
        x, mask = torch.zeros(1, 8, 7, 3), torch.ones(1, 8)
        for kw, match in NEW_ERRORS:
            kw = dict(kw)
            if kw.get("constraints") == "paired":
                kw["constraints"] = _paired()
            with pytest.raises(ValueError, match=match):
                cls.design_profile(model, x, mask, **kw)
        assert not ran


def test_predict_refuses_before_the_first_forward_pass():
    """``resolve_run``, which both families' ``predict`` call first: ``table="global"`` lifts the refusal of a profile under ``require`` and
    of ``require`` without samples, and nothing else."""
    from rnampnn.utils.predict import resolve_run
    mode, avoid, require = resolve_run(0, "prefix", None, require=["GGAGG"], avoid=["GGGG"], table="global")
    assert mode == "require" and avoid is None and isinstance(require, M.DesignAutomaton)
    mode, avoid, require = resolve_run(4, "prefix", None, avoid=["GGGG"], table="global")
    assert mode == "avoid" and isinstance(avoid, M.MotifAutomaton) and require is None
    with pytest.raises(ValueError, match="a design profile together with require is not built: the profile entries know forbidden motifs only"):
        resolve_run(4, "prefix", None, require=["GGAGG"])
    with pytest.raises(ValueError, match="a design profile together with require is not built"):
        resolve_run(4, "prefix", None, require=["GGAGG"], table="lds")
    with pytest.raises(ValueError, match="required motifs need samples > 0"):
        resolve_run(0, None, None, require=["GGAGG"])
    for kw, match in ((dict(require=["GGAGG"]), "table='global' is the home of the table of a design profile"),          # no profile
                      (dict(), 'table="global" needs avoid and / or require'),
                      (dict(gc_content=(0.4, 0.6)), 'table="global" needs avoid and / or require'),
                      (dict(avoid=["GGGG"], gc_content=(0.4, 0.6)), "avoid together with gc_content is not built"),
                      (dict(require=["GGAGG"], pairs="nested"), "table='global' is the home of the table of a design profile"),
                      (dict(require=["GGAGG"], distinct="best"), "require together with distinct is not built")):
        with pytest.raises(ValueError, match=match):
            resolve_run(4, None if kw == dict(require=["GGAGG"]) else "prefix", None, table="global", **kw)
    with pytest.raises(ValueError, match="table must be one of"):
        resolve_run(4, "prefix", None, avoid=["GGGG"], table="auto")
    with pytest.raises(ValueError, match="require together with base pairs is not built"):
        resolve_run(0, "prefix", {"1abc": ("GNRA....", "((....))")}, require=["GGAGG"], table="global")


def test_the_cli_refuses_before_a_checkpoint_is_opened():
    sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
    import predict as P
    base = ["--ckpt", "none.pt", "--data", "none"]
    # what stands without --table, word for word
    with pytest.raises(ValueError, match="--require needs --samples N > 0"):
        P.run(P.parse(base + ["--require", "GGAGG"]))
    with pytest.raises(ValueError, match="--require together with --profile-out is not built: the automaton conditions plain single-state "
                                         "designs only, and no profile is built for it"):
        P.run(P.parse(base + ["--samples", "2", "--require", "GGAGG", "--profile-out", "prefix"]))
    with pytest.raises(ValueError, match="--require together with --profile-out is not built"):
        P.run(P.parse(base + ["--samples", "2", "--require", "GGAGG", "--profile-out", "prefix", "--table", "lds"]))
    with pytest.raises(ValueError, match="--tree auto together with --avoid is not built"):
        P.run(P.parse(base + ["--profile-out", "prefix", "--avoid", "GGGG", "--tree", "auto"]))
    # the new flag
    with pytest.raises(ValueError, match="--table global needs --profile-out PREFIX"):
        P.run(P.parse(base + ["--samples", "2", "--require", "GGAGG", "--table", "global"]))
    with pytest.raises(ValueError, match="--table global needs --require, --avoid or --max-run"):
        P.run(P.parse(base + ["--profile-out", "prefix", "--table", "global"]))
    for flag, value in (("--gc-content", "0.4:0.6"), ("--max-mutations", "3"), ("--distinct", "sample"), ("--states", "states.csv")):
        with pytest.raises(ValueError, match=f"(--require|--table global|--profile-out) together with {flag} is not built"):
            P.run(P.parse(base + ["--samples", "2", "--profile-out", "prefix", "--table", "global", "--require", "GGAGG", flag, value]))
    with pytest.raises(ValueError, match="--tree global together with --require is not built"):
        P.run(P.parse(base + ["--profile-out", "prefix", "--table", "global", "--require", "GGAGG", "--tree", "global"]))
    with pytest.raises(SystemExit):
        P.parse(base + ["--table", "auto"])
    # what is built gets as far as the checkpoint, with or without --samples
    for more in ([], ["--samples", "2"]):
        args = P.parse(base + ["--profile-out", "prefix", "--table", "global", "--require", "GGAGG,GNRA", "--max-run", "3"] + more)
        assert len(P.require_option(args)["require"].required) == 2 and P.table_option(args) == dict(table="global")
        with pytest.raises(FileNotFoundError):
            P.run(args)
    args = P.parse(base + ["--profile-out", "prefix", "--table", "global", "--max-run", "3"])
    assert "avoid" in P.avoid_option(args) and P.table_option(args) == dict(table="global") and P.table_option(P.parse(base)) == {}


def test_the_build_and_the_binding_know_the_new_unit():
    import __graft_entry__ as g
    from rnampnn import _native
    assert "design_dfa_profile.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_dfa_profile.hip"))
    assert {"rnampnn_design_dfa_profile", "rnampnn_design_dfa_profile_workspace_bytes"} <= set(_native.SYMBOLS)
    assert len(_native.SYMBOLS["rnampnn_design_dfa_profile"][1]) == 24
