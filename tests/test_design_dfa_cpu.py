"""The host side of design with required motifs, without a GPU: the automaton ``rnampnn.utils.motifs.DesignAutomaton`` builds against a
brute-force substring scan, the float64 restatement of ``rnampnn_design_dfa`` (tests/_design_dfa_ref.py) against an enumerated joint, the
share of the device tests' draws that pass close to a cumulative boundary, and the Python surface: every ``ValueError``, the refusals of
``design_mode`` and of base pairs, and the CLI's refusals before a checkpoint is opened."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_dfa_ref as R  # noqa: E402
from _design_gc_ref import NEG, lse  # noqa: E402
from rnampnn.model import decode as D  # noqa: E402
from rnampnn.utils import motifs as M  # noqa: E402

NEAR = 1e-8
LONG = "GGAGGCUUCGAAUUCGCAUGCCAUGGUACCUAGCUAGGAUCCGAUAUCAAGCUUGCGGCCGCUCGAGACGUCUGCAGCCCGGGAGAUCUGUCGACACUAGUUCUAGA"
STATES_256 = ((LONG[:26], LONG[50:89]), (), None)                  # two long required words: exactly 256 states
STATES_257 = ((LONG[:13], LONG[50:89]), (), 3)                     # ... and one too many


def _auto(require, avoid=(), max_run=None):
    return M.DesignAutomaton.from_motifs(require, avoid, max_run)


# ---------------------------------------------------------------------------------------------------------------- the automaton
SETS = [(("GA",), (), 2),                                          # the frequency test's automaton
        (("GGA", "GAC"), (), None),                                # overlapping required motifs: GGAC holds both
        (("UGGA", "GGA"), (), None),                               # one required motif is a suffix of another
        (("GGA",), ("GAC", "ACG"), None),                          # a required word runs into an avoided one
        (("GNR", "TT"), ("CC",), 3),                               # IUPAC, T = U
        (("GG", "GG", "AU"), ("GGG",), None),                      # a duplicate; GG is a prefix of the avoided GGG
        (("ACG",), ("ACG",), None)]                                # required and avoided at once: nothing is accepted


@pytest.mark.parametrize("require, avoid, max_run", SETS)
def test_the_automaton_equals_a_substring_scan_on_every_sequence_up_to_length_7(require, avoid, max_run):
    """"The end state accepts and no dead state was entered" is "holds every required motif and no avoided word", for all 21,845
    sequences; ``scan`` (torch) and ``follow`` (the restatement) agree on the counts."""
    auto = _auto(require, avoid, max_run)
    groups, banned = R.required_sets(require), R.expand(avoid, max_run)
    assert {tuple(w) for w in auto.words} == banned and auto.kind.dtype == torch.uint8 and auto.delta.dtype == torch.uint8
    assert tuple(auto.delta.shape) == (auto.n_states, 4) and auto.n_live == int(((auto.kind & 1) == 0).sum()) and int(auto.kind[0]) == 0
    assert not bool(((auto.kind & 3) == 3).any())                  # dead states never accept
    seqs = np.full((sum(4 ** n for n in range(8)), 7), -1, dtype=np.int8)
    i = 0
    for n in range(8):
        for w in itertools.product(range(4), repeat=n):
            seqs[i, :n] = w
            i += 1
    hits, accepted = (t.numpy() for t in auto.scan(torch.from_numpy(seqs)))
    want_hits = np.array([R.naive_hits(row, banned) for row in seqs])
    want_all = np.array([R.contains_all(row, groups) for row in seqs])
    assert np.array_equal(hits, want_hits)
    assert np.array_equal((accepted == 1) & (hits == 0), want_all & (want_hits == 0))
    for i in range(0, len(seqs), 97):
        assert R.follow(seqs[i], auto.delta.numpy(), auto.kind.numpy()) == (int(hits[i]), int(accepted[i]))


def test_order_duplicates_case_and_t_make_no_difference():
    x = _auto(["GGAGG", "GNRA"], ["GAAUUC", "ACGU"], 3)
    y = _auto(["gnra", "GGAGG", "GGAGG"], ["ACGT", "GAATTC", "ACGU"], 3)
    assert x.delta.tolist() == y.delta.tolist() and x.kind.tolist() == y.kind.tolist() and x.required == y.required
    z = _auto(["GARA", "GBRA"])                                     # not another spelling of GNRA: BOTH must occur, two seen flags
    assert len(z.required) == 2 and len(_auto(["GNRA"]).required) == 1 and z.n_states > _auto(["GNRA"]).n_states
    assert M.as_design_automaton(None) is None and M.as_design_automaton(x) is x
    av = M.MotifAutomaton.from_motifs(["GAAUUC", "ACGU"], max_run=3)
    assert M.as_design_automaton(["GGAGG", "GNRA"], av).delta.tolist() == x.delta.tolist()
    assert _auto("GGAGG").delta.tolist() == _auto(["GGAGG"]).delta.tolist()


def test_the_case_automata_have_the_sizes_the_tests_name():
    sizes = {name: (_auto(*spec).n_states, _auto(*spec).n_live) for name, spec in R.CASE_AUTOMATA.items()}
    assert sizes == {"ggagg": (11, 11), "gnra_run3": (61, 53), "two_run3": (89, 73)}


def test_256_states_are_accepted_and_257_refused():
    a = _auto(*STATES_256)
    assert a.n_states == M.DFA_MAX_STATES == 256 and int(a.delta.max()) == 255 and a.n_live == 256
    with pytest.raises(ValueError, match=r"has 257 states, the limit is 256"):
        _auto(*STATES_257)
    assert M.MAX_STATES == 64                                      # the avoid entry's limit stays


@pytest.mark.parametrize("require, avoid, max_run, match", [
    ((), (), None, "require is empty"), ((), ("GGGG",), 3, "require is empty"), (None, (), None, "require is empty"),
    (("GG", ""), (), None, "empty motif"), (("GGXA",), (), None, "unknown letter 'X'"), (("GG",), ("G.A",), None, "unknown letter"),
    (("GG",), (), 0, "max_run = 0"),
    (("AA", "AU", "AC", "AG", "UA", "UU", "UC"), (), None, "7 required motifs, the limit is 6")])
def test_value_errors(require, avoid, max_run, match):
    with pytest.raises(ValueError, match=match):
        M.DesignAutomaton.from_motifs(require, avoid, max_run)


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("spec, n", [(SETS[0], 6), (SETS[1], 6), (SETS[3], 6), (SETS[4], 5), (SETS[1], 2), (SETS[6], 4)])
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_path_logprob_is_the_enumerated_joint_over_the_language(spec, n, temperature):
    """Every one of the 4^n sequences: the product of the walk's conditionals equals the tempered, biased joint restricted to the admitted
    sequences of the language (every required motif, no avoided word, by substring comparison) and renormalised, to 1e-12; it is -inf
    outside; the probabilities sum to 1.  An RNA with no such sequence is dfa_miss and falls back to the free draw."""
    require, avoid, max_run = spec
    auto = _auto(require, avoid, max_run)
    groups, banned = R.required_sets(require), R.expand(avoid, max_run)
    rng = np.random.RandomState(17 + n)
    logits = (2.0 * rng.standard_normal((n, 4))).astype(np.float32)
    bias = rng.standard_normal((n, 4)).astype(np.float32)
    allowed = np.full(n, 15, dtype=np.uint8)
    if n >= 5:
        allowed[0], allowed[2] = 0, 15 ^ 4                           # empty: free; no C
    plan = R.DfaPlan(logits, n, temperature, auto.delta.numpy(), auto.kind.numpy(), allowed, bias)
    z = (logits.astype(np.float64) + bias.astype(np.float64)) / float(np.float32(temperature))
    mask = np.where(allowed == 0, 15, allowed)
    joint = {}
    for seq in itertools.product(range(4), repeat=n):
        if all((mask[t] >> seq[t]) & 1 for t in range(n)) and R.contains_all(seq, groups) and R.naive_hits(seq, banned) == 0:
            joint[seq] = sum(z[t, seq[t]] for t in range(n))
    assert plan.infeasible == int(n >= 5) and plan.miss == int(not joint)
    if not joint:                                                   # too short, or required and avoided at once
        free = R.DfaPlan(logits, n, temperature, np.zeros((1, 4), dtype=np.uint8), np.array([2], dtype=np.uint8), allowed, bias)
        assert free.miss == 0 and all(np.array_equal(plan.draw(5, s, 0)[0], free.draw(5, s, 0)[0]) for s in range(8))
        return
    total = lse(np.array(list(joint.values())))
    assert 0 < len(joint) < 4 ** n and abs(plan.l[0, 0] - total) <= 1e-12 * max(1.0, abs(total))
    mass = 0.0
    for seq in itertools.product(range(4), repeat=n):
        lp = plan.path_logprob(seq)
        if seq in joint:
            assert abs(lp - (joint[seq] - total)) <= 1e-12 * max(1.0, abs(lp)), seq
            mass += np.exp(lp)
        else:
            assert lp == NEG, seq
    assert abs(mass - 1.0) <= 1e-12


def test_every_live_state_accepting_is_the_avoid_restatement():
    """The anchor on the host: an automaton in which every live state accepts draws what ``_design_avoid_ref`` draws."""
    import _design_avoid_ref as AV
    auto = M.MotifAutomaton.from_motifs(["UGGA", "GGA"], max_run=3)
    kind = np.array([1 if (auto.terminal >> a) & 1 else 2 for a in range(auto.n_states)], dtype=np.uint8)
    rng = np.random.RandomState(2)
    logits = (3.0 * rng.standard_normal((40, 4))).astype(np.float32)
    logits[:, 3] += 4.0
    a = AV.AvoidPlan(logits, 40, 0.5, auto.delta.numpy(), auto.terminal)
    d = R.DfaPlan(logits, 40, 0.5, auto.delta.numpy(), kind)
    assert np.array_equal(a.l, d.l) and a.miss == d.miss == 0
    assert all(np.array_equal(a.draw(9, s, 3)[0], d.draw(9, s, 3)[0]) for s in range(16))


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_the_case_batch_keeps_clear_of_the_boundaries_and_holds_the_motifs(name, temperature):
    """The restatement alone: at most 5 % of the batch's (sample, RNA) draws pass within 1e-8 of a cumulative boundary - the cap the
    device comparison may leave out; every feasible RNA's draws hold every required motif and no avoided word, by substring scan."""
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    auto = _auto(require, avoid, max_run)
    ref = R.case_ref(name, auto.delta.numpy(), auto.kind.numpy(), temperature)
    near = ref["margin"] <= NEAR
    print(f"{name}, temperature {temperature}: {near.mean():.4%} of the {near.size} draws within {NEAR} of a boundary")
    assert near.mean() <= 0.05
    assert ref["infeasible"].tolist() == R.CASE_INFEASIBLE and ref["dfa_miss"].tolist() == R.CASE_MISS
    groups, banned = R.required_sets(require), R.expand(avoid, max_run)
    seqs = ref["seqs"]
    for b, miss in enumerate(R.CASE_MISS):
        for s in range(R.CASE_S):
            if not miss:
                assert R.contains_all(seqs[s, b], groups) and R.naive_hits(seqs[s, b], banned) == 0, (s, b)
                assert ref["hits"][s, b] == 0 and ref["accepted"][s, b] == 1
            else:
                assert ref["accepted"][s, b] == 0 and ref["hits"][s, b] == R.naive_hits(seqs[s, b], banned)
    hits, accepted = auto.scan(torch.from_numpy(seqs))
    assert np.array_equal(hits.numpy(), ref["hits"]) and np.array_equal(accepted.numpy(), ref["accepted"])
    assert (seqs[:, 5, 20:27] == np.array([3, 3, 0, 3, 3, 0, 0])).all() and (seqs[:, 6, 20:23] == 3).all() and (seqs[:, 4, :10] == 0).all()
    if max_run == 3:
        assert (ref["hits"][:, 4] > 0).all() and (seqs[:, 6, 19] != 3).all() and (seqs[:, 6, 23] != 3).all()


# ---------------------------------------------------------------------------------------------------------------- the mode and its refusals
def test_design_mode_selects_require_first_and_absorbs_avoid():
    auto = _auto(["GGAGG"])
    assert D.DESIGN_MODES[0][0] == "avoid" and D.design_mode(require=auto) == "require" and D.design_mode() == "plain"
    assert D.design_mode(avoid=["GGGG"], require=["GGAGG"]) == "require" and D.design_mode(avoid=["GGGG"]) == "avoid"
    assert D.design_mode(None, (0.4, 0.6)) == "gc_content" and D.design_mode([2], None, None, None, None) == "states"  # existing callers
    for name, value in (("states", [1]), ("gc_content", (0.4, 0.6)), ("distinct", "sample"), ("mutations", (torch.zeros(1, 4), 2))):
        with pytest.raises(ValueError, match=f"require together with {name} is not built"):
            D.design_mode(require=auto, **{name: value})
        with pytest.raises(ValueError, match=f"avoid together with {name} is not built"):      # every existing message stays
            D.design_mode(avoid=["GGGG"], **{name: value})


def test_base_pairs_are_refused_without_touching_a_device(monkeypatch):
    """The refusals come from ``check_require``, which the models call before their forward pass: no library is loaded, no tensor moved."""
    from rnampnn import _native
    from rnampnn.utils.constraints import DesignConstraints
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the library was loaded"))
    paired = DesignConstraints.from_specs([("GNRA....", "((....))")], [8], 8)
    with pytest.raises(ValueError, match="require together with base pairs is not built.*drop `structure`"):
        D.check_require(["GGAGG"], None, paired)
    with pytest.raises(ValueError, match="drop `structure`"):
        D.design_dfa_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), constraints=paired, require=["GGAGG"])
    fixed = DesignConstraints.from_specs([("GNRA....", None)], [8], 8, bias=[0, 0, 0, 1.0], omit="C")
    auto = D.check_require(["GGAGG"], ["GAAUUC"], fixed, max_run=3)
    assert isinstance(auto, M.DesignAutomaton) and auto.letters() == ["AAAA", "UUUU", "CCCC", "GAAUUC", "GGGG"]
    assert D.check_require(None, ["GGGG"], paired) is None
    with pytest.raises(ValueError, match="require is required"):
        D.design_dfa_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), avoid=["GGGG"])
    with pytest.raises(ValueError, match="7 required motifs"):
        D.design_dfa_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), require=["AA", "AU", "AC", "AG", "UA", "UU", "UC"])
    with pytest.raises(RuntimeError, match="rnampnn_design_dfa runs on an MI355X"):
        D.design_dfa_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), constraints=fixed, require=["GGAGG"], max_run=3)


def test_the_models_refuse_before_their_forward_pass(monkeypatch):
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils.constraints import DesignConstraints
    paired = DesignConstraints.from_specs([("GNRA....", "((....))")], [8], 8)
    for cls in (RNAMPNN, RNAModel):
        def forward_ran(*a, **k):
            pytest.fail("the forward pass ran")
        for name in ("_run", "_packed_logits"):
            if hasattr(cls, name):
                monkeypatch.setattr(cls, name, forward_ran)
        model = cls.__new__(cls)
        x, mask = torch.zeros(1, 8, 7, 3), torch.ones(1, 8)
        with pytest.raises(ValueError, match="require together with gc_content is not built"):
            cls.design(model, x, mask, require=["GGAGG"], gc_content=(0.4, 0.6))
        with pytest.raises(ValueError, match="require together with base pairs is not built"):
            cls.design(model, x, mask, require=["GGAGG"], avoid=["GGGG"], constraints=paired)
        with pytest.raises(ValueError, match="require is empty"):
            cls.design(model, x, mask, require=[])


def test_the_cli_refuses_before_a_checkpoint_is_opened():
    sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
    import predict as P
    base = ["--ckpt", "none.pt", "--data", "none"]
    with pytest.raises(ValueError, match="--require needs --samples"):
        P.run(P.parse(base + ["--require", "GGAGG"]))
    for flag, value in (("--profile-out", "prefix"), ("--states", "states.csv"), ("--gc-content", "0.4:0.6"), ("--distinct", "sample"),
                        ("--max-mutations", "3")):
        with pytest.raises(ValueError, match=f"--require together with {flag} is not built"):
            P.run(P.parse(base + ["--samples", "2", "--require", "GGAGG", "--avoid", "GGGG", flag, value]))
    with pytest.raises(ValueError, match="unknown letter 'X'"):
        P.run(P.parse(base + ["--samples", "2", "--require", "GGAGG,GXA"]))
    with pytest.raises(ValueError, match=r"has 257 states, the limit is 256"):
        P.run(P.parse(base + ["--samples", "2", "--require", ",".join(STATES_257[0]), "--max-run", "3"]))
    args = P.parse(base + ["--samples", "2", "--require", "GGAGG, GNRA", "--avoid", "GAATTC", "--max-run", "3"])
    opt = P.require_option(args)
    assert opt["require"].letters() == ["AAAA", "UUUU", "CCCC", "GAAUUC", "GGGG"] and len(opt["require"].required) == 2
    assert P.avoid_option(args) == {} and P.require_option(P.parse(base)) == {}             # --require takes --avoid / --max-run with it
    assert "avoid" in P.avoid_option(P.parse(base + ["--samples", "2", "--avoid", "GGGG"]))


def test_the_designs_csv_gains_three_columns():
    from rnampnn.utils.predict import design_columns
    header, cells, filled = design_columns("require", (torch.tensor([[0, 2]]), torch.tensor([[1, 0]]), torch.tensor([0, 1])), [5, 5])
    assert header == ",motif_hits,required_found,require_miss" and filled is None and cells(0, 0) == (0, 1, 0) and cells(0, 1) == (2, 0, 1)
    assert design_columns("avoid")[0] == ",motif_hits,avoid_miss"


def test_the_build_and_the_binding_know_the_new_unit():
    import __graft_entry__ as g
    from rnampnn import _native
    assert "design_dfa.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_dfa.hip"))
    assert {"rnampnn_design_dfa", "rnampnn_design_dfa_workspace_bytes"} <= set(_native.SYMBOLS)
