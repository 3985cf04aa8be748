"""The host side of design with motifs under base pairs, without a GPU: the float64 restatement of ``rnampnn_design_nested``
(tests/_design_nested_ref.py) against a brute-force enumeration of short RNAs, against ``_design_gc_ref`` (pairs, no automaton) and
``_design_dfa_ref`` (automaton, no pairs), the share of the device tests' draws that pass close to a cumulative boundary, and the Python
surface: ``crossing_pairs``, the avoid-alone automaton, every ``ValueError`` of ``pairs="nested"``, the refusals that ``pairs=None``
keeps word for word, and the CLI's refusals before a checkpoint is opened."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_dfa_ref as DF  # noqa: E402
import _design_gc_ref as GC  # noqa: E402
import _design_nested_ref as R  # noqa: E402
from _design_gc_ref import NEG, lse  # noqa: E402
from rnampnn.model import decode as D  # noqa: E402
from rnampnn.utils import motifs as M  # noqa: E402
from rnampnn.utils.constraints import DesignConstraints, crossing_pairs, parse_dot_bracket  # noqa: E402

NEAR = 1e-8
STRUCTURES = ["()", "(())..", "((.)(.))", ".(.).(.)", "(...)", "((..))", ".()()..", "(()).()", "((()))", "..(.)..", "(.(.).)", "(.)(())"]
AUTOMATA = {"ga_run2": (("GA",), (), 2), "gc_not_aa": (("GC",), ("AA",), None)}


def _auto(name):
    require, avoid, max_run = R.CASE_AUTOMATA[name] if name in R.CASE_AUTOMATA else AUTOMATA[name]
    return M.as_nested_automaton(require or None, avoid or None, max_run)


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("name", sorted(AUTOMATA))
def test_path_logprob_is_the_enumerated_joint_under_pairs_and_automaton(structure, name):
    """Every one of the 4^n sequences (n <= 8), free and under random masks, at both temperatures: the product of the walk's conditionals
    equals the tempered joint restricted to the sequences the masks admit, whose pairs are compatible and that the automaton accepts
    (``brute_force``: cell against cell, letter by letter), renormalised, to 1e-12; it is -inf outside; the probabilities sum to 1; and
    ``dfa_miss`` says exactly whether the enumeration found a sequence."""
    auto, n = _auto(name), len(structure)
    mate = R.parse_structure(structure)
    rng = np.random.RandomState(len(structure) * 31 + sorted(AUTOMATA).index(name))
    met = 0
    for temperature, masked in itertools.product((1.0, 0.3), (False, True)):
        logits = (3.0 * rng.standard_normal((n, 4))).astype(np.float32)
        allowed = rng.choice([15, 15, 15, 7, 9, 3, 12, 0, 8], size=n).astype(np.uint8) if masked else None
        plan = R.NestedPlan(logits, n, temperature, auto.delta.numpy(), auto.kind.numpy(), allowed, mate)
        assert plan.nest_miss == 0
        joint = R.brute_force(plan)
        assert plan.miss == int(not np.isfinite(joint).any()), (temperature, masked)
        if plan.miss:
            continue
        met += 1
        want = joint - lse(joint)
        got = np.array([plan.path_logprob(seq) for seq in itertools.product(range(4), repeat=n)])
        inside = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), inside) and (got[~inside] == NEG).all()
        assert np.abs(got[inside] - want[inside]).max() <= 1e-12
        assert abs(np.exp(got[inside]).sum() - 1.0) <= 1e-12
        assert abs(plan.table(0, True)[0, 0] - lse(joint)) <= 1e-12 * max(1.0, abs(lse(joint)))
    assert met >= 1 or n < 3                                        # (the free cases of every structure long enough are feasible)


def test_a_one_state_automaton_is_the_count_trees_full_window_and_rnampnn_designs_draws():
    """No motif at all (one live accepting state): pairs and masks alone.  ``_design_gc_ref`` with the window 0 .. n is that distribution
    too, but it selects the count first and the classes of a count after it, so its SELECTIONS differ from a plain draw's sample by
    sample; what the two share is the distribution: every sequence's ``path_logprob`` agrees to 1e-12.  The draws themselves are held
    to ``_design_ref`` - rnampnn_design's rule in float64, the pair one joint selection with its lower index - wherever the margin
    exceeds 1e-8, on the whole device batch."""
    import _design_ref as DR
    delta, kind = np.zeros((1, 4), dtype=np.uint8), np.array([2], dtype=np.uint8)
    rng = np.random.RandomState(11)
    for structure in ("()", "(())..", "((.)(.))", ".(.).(.)", "(.)(())"):
        n, mate = len(structure), R.parse_structure(structure)
        logits = (3.0 * rng.standard_normal((n, 4))).astype(np.float32)
        allowed = rng.choice([15, 15, 7, 9, 3, 12, 0], size=n).astype(np.uint8)
        plan = R.NestedPlan(logits, n, 0.3, delta, kind, allowed, mate)
        gc = GC.GcPlan(logits, n, 0.3, 0, n, allowed, mate, True)
        assert plan.miss == 0 and plan.infeasible == gc.infeasible
        for seq in itertools.product(range(4), repeat=n):
            got, want = plan.path_logprob(seq), gc.path_logprob(np.array(seq))
            assert (got == NEG and want == NEG) or abs(got - want) <= 1e-12, (structure, seq)
    h = R.case_arrays()
    seqs, margin, bad, _ = DR.design_ref(h["logits"], R.CASE_LENGTHS, 0.3, 4, R.CASE_SEED, h["allowed"], h["partner"], True, h["bias"])
    assert bad.tolist() == R.CASE_INFEASIBLE
    checked = 0
    for b, n in enumerate(R.CASE_LENGTHS):                          # (RNA 6 crosses: drawn as rnampnn_design draws it, so it is held too)
        plan = R.NestedPlan(h["logits"][b], n, 0.3, delta, kind, h["allowed"][b], h["partner"][b], True, h["bias"][b])
        assert plan.miss == 0 and plan.infeasible == R.CASE_INFEASIBLE[b] and plan.nest_miss == R.CASE_NEST[b]
        for s in range(4):
            got, m = plan.draw(R.CASE_SEED, s, b)
            if min(m, margin[s, b, :n].min(initial=np.inf)) > NEAR:
                assert np.array_equal(got, seqs[s, b, :n]), (b, s)
                checked += 1
    assert checked >= 30


@pytest.mark.parametrize("name", sorted(DF.CASE_AUTOMATA))
def test_without_pairs_the_draws_are_the_dfa_restatements(name):
    """The anchor on the host: the DFA entry's own batch and automata, no partner table - tables, flags and draws are ``_design_dfa_ref``'s."""
    h = DF.case_arrays()
    auto = M.DesignAutomaton.from_motifs(*DF.CASE_AUTOMATA[name])
    for b, n in enumerate(DF.CASE_LENGTHS):
        d = DF.DfaPlan(h["logits"][b], n, 0.3, auto.delta.numpy(), auto.kind.numpy(), h["allowed"][b], h["bias"][b])
        for partner in (None, np.full(DF.CASE_T, -1, dtype=np.int32)):
            p = R.NestedPlan(h["logits"][b], n, 0.3, auto.delta.numpy(), auto.kind.numpy(), h["allowed"][b], partner, True, h["bias"][b])
            assert (p.miss, p.infeasible, p.nest_miss) == (d.miss, d.infeasible, 0)
            live = np.nonzero((auto.kind.numpy() & 1) == 0)[0]
            assert all(np.array_equal(p.R[t][:, 0], d.l[t, live]) for t in range(n))
            for s in range(4):
                assert np.array_equal(p.draw(DF.CASE_SEED, s, b)[0], d.draw(DF.CASE_SEED, s, b)[0]), (b, s)


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_the_case_batch_keeps_clear_of_the_boundaries_pairs_and_holds_the_motifs(name, temperature):
    """The restatement alone: at most 5 % of the batch's (sample, RNA) draws pass within 1e-8 of a cumulative boundary - the cap the
    device comparison may leave out; the flags are the ones the batch was built for; every feasible RNA's draws pair compatibly at every
    feasible pair, hold every required motif and no avoided word (substring scan); the structures are as deep as the batch promises."""
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    auto = _auto(name)
    ref = R.case_ref(name, auto.delta.numpy(), auto.kind.numpy(), temperature)
    near = ref["margin"] <= NEAR
    print(f"{name}, temperature {temperature}: {near.mean():.4%} of the {near.size} draws within {NEAR} of a boundary")
    assert near.mean() <= 0.05
    assert ref["infeasible"].tolist() == R.CASE_INFEASIBLE and ref["nest_miss"].tolist() == R.CASE_NEST
    assert ref["dfa_miss"].tolist() == R.CASE_MISS[name]
    groups, banned = R.required_sets(require), R.expand(avoid, max_run)
    seqs, pairs = ref["seqs"], {(0, 1), (1, 0), (2, 3), (3, 2), (1, 3), (3, 1)}                    # AU, UA, CG, GC and the wobble UG, GU
    for b, plan in enumerate(ref["plans"]):
        for s in range(R.CASE_S):
            assert all((int(seqs[s, b, t]), int(seqs[s, b, j])) in pairs for t, j in enumerate(plan.mate) if j > t), (s, b)
            if not (plan.miss or plan.nest_miss):
                assert R.contains_all(seqs[s, b], groups) and R.naive_hits(seqs[s, b], banned) == 0, (s, b)
                assert ref["hits"][s, b] == 0 and ref["accepted"][s, b] == 1
            else:
                assert ref["hits"][s, b] == R.naive_hits(seqs[s, b], banned)
    hits, accepted = auto.scan(torch.from_numpy(seqs))
    assert np.array_equal(hits.numpy(), ref["hits"]) and np.array_equal(accepted.numpy(), ref["accepted"])
    assert (seqs[:, 5, 20:27] == np.array([3, 3, 0, 3, 3, 0, 0])).all() and (seqs[:, 4, 10:14] == 0).all() and (seqs[:, 4, 30:34] == 1).all()
    if max_run == 3:
        assert (ref["hits"][:, 4] > 0).all()                        # the stem that spells AAAA and pairs with UUUU


def test_the_case_structures_are_what_the_batch_promises():
    texts = R.case_structures()
    assert [len(t) for t in texts] == R.CASE_LENGTHS
    depth = [max(itertools.accumulate([(c in "([") - (c in ")]") for c in t]), default=0) for t in texts]
    assert depth[7] >= 6 and depth[8] >= 6 and "()" in texts[7] and "()" in texts[8] and texts[8][-1] == ")" and texts[2] == "()"
    h = R.case_arrays()
    assert [int(crossing_pairs(h["partner"][b, :n])) for b, n in enumerate(R.CASE_LENGTHS)] == R.CASE_NEST
    assert [R.crossing(h["partner"][b, :n]) for b, n in enumerate(R.CASE_LENGTHS)] == R.CASE_NEST
    assert sum(int((h["partner"][b] >= 0).sum()) // 2 for b in range(len(texts))) >= 60


# ---------------------------------------------------------------------------------------------------------------- the host helpers
def test_crossing_pairs_is_the_pairwise_definition():
    for text, want in (("", False), ("....", False), ("((..))", False), ("(())()", False), ("((..[[..))..]]", True), ("([)]", True),
                       ("(.[.).]", True), ("([])", False), ("{<>}[]", False), ("(((...)))[[[...]]]", False), ("<(>)", True)):
        mate = parse_dot_bracket(text)
        assert crossing_pairs(mate) is want and crossing_pairs(torch.from_numpy(mate)) is want and bool(R.crossing(mate)) is want, text
    rng = np.random.RandomState(3)
    for _ in range(200):                                            # random symmetric tables, entries that are no pair included
        n = int(rng.randint(2, 12))
        mate = np.full(n, -1, dtype=np.int64)
        free = list(rng.permutation(n))
        while len(free) >= 2 and rng.rand() < 0.7:
            i, j = free.pop(), free.pop()
            mate[i], mate[j] = j, i
        valid = mate.copy()
        if rng.rand() < 0.3:
            mate[int(rng.randint(n))] = int(rng.randint(-3, n + 3))  # a broken entry: it and its former partner are no pair
            valid = np.array([j if 0 <= j < n and j != t and mate[j] == t else -1 for t, j in enumerate(mate)])
        assert crossing_pairs(list(mate)) == bool(R.crossing(valid))
    assert crossing_pairs([5, -1, 9, 2]) is False                    # entries outside the row


def test_the_avoid_alone_automaton_accepts_in_every_live_state():
    auto = M.DesignAutomaton.from_avoid(["GGGG"], max_run=3)
    plain = M.MotifAutomaton.from_motifs(["GGGG"], max_run=3)
    assert torch.equal(auto.delta, plain.delta) and auto.n_states == 17 and auto.n_live == plain.n_live == 13
    assert auto.kind.tolist() == [1 if (plain.terminal >> a) & 1 else 2 for a in range(17)] and auto.required == ()
    assert M.as_nested_automaton(None, plain).kind.tolist() == auto.kind.tolist()
    assert M.as_nested_automaton(None, None, 3).n_live == 13 and M.as_nested_automaton() is None
    both = M.as_nested_automaton(["GNRA"], None, 3)
    assert (both.n_states, both.n_live) == (61, 53) and M.as_nested_automaton(both) is both
    seqs = torch.tensor([[3, 3, 3, 3, 0], [3, 3, 3, 0, 3]], dtype=torch.int8)
    hits, accepted = auto.scan(seqs)
    assert hits.tolist() == plain.hits(seqs).tolist() == [1, 0] and accepted.tolist() == [1, 1]
    with pytest.raises(ValueError, match="require is empty"):       # the refusal of from_motifs stays
        M.DesignAutomaton.from_motifs([], ["GGGG"])
    with pytest.raises(ValueError, match="no motif given"):
        M.DesignAutomaton.from_avoid([])


# ---------------------------------------------------------------------------------------------------------------- the mode and its refusals
def test_design_mode_nested_is_opt_in_and_refuses_what_is_not_built():
    assert D.design_mode(avoid=["GGGG"], pairs="nested") == "nested" and D.design_mode(require=["GNRA"], pairs="nested") == "nested"
    assert D.design_mode(avoid=["GGGG"], require=["GNRA"], pairs="nested") == "nested"
    for name, value in (("states", [1]), ("gc_content", (0.4, 0.6)), ("distinct", "sample"), ("mutations", (torch.zeros(1, 4), 2))):
        with pytest.raises(ValueError, match=f"pairs='nested' together with {name} is not built"):
            D.design_mode(avoid=["GGGG"], pairs="nested", **{name: value})
    with pytest.raises(ValueError, match="pairs='nested' needs avoid and / or require: plain constraints already honour base pairs"):
        D.design_mode(pairs="nested")
    for other in ("crossing", "", True, 1):
        with pytest.raises(ValueError, match="pairs must be None or 'nested'"):
            D.design_mode(avoid=["GGGG"], pairs=other)
    # pairs=None: every path, message and table is what it was
    assert D.DESIGN_MODES[0] == ("avoid", ("states", "gc_content", "distinct", "mutations"),
                                 "the automaton conditions the draws of rnampnn_design on the motifs alone")
    assert [m[0] for m in D.DESIGN_MODES] == ["avoid", "mutations", "distinct", "gc_content", "states"]
    assert D.design_mode(avoid=["GGGG"]) == "avoid" and D.design_mode(require=["GNRA"], pairs=None) == "require" and D.design_mode() == "plain"
    with pytest.raises(ValueError, match="require together with gc_content is not built"):
        D.design_mode(require=["GNRA"], gc_content=(0.4, 0.6))


def test_check_nested_names_crossing_rows_and_touches_no_device(monkeypatch):
    from rnampnn import _native
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the library was loaded"))
    nested = DesignConstraints.from_specs([("GNRA....", "((....))"), (None, "(())..()")], [8, 8], 8)
    auto = D.check_nested(["GNRA"], ["GGGG"], nested, max_run=3)
    assert isinstance(auto, M.DesignAutomaton) and auto.n_live == 53
    assert D.check_nested(None, None, nested) is None and D.check_nested(None, ["GGGG"], nested).n_live == 4
    knotted = DesignConstraints.from_specs([(None, "((....))"), (None, "(.[.).]."), (None, "........"), (None, "([)]....")], [8] * 4, 8)
    with pytest.raises(ValueError, match=r"pairs='nested': the structure of row\(s\) \[1, 3\] holds a pseudoknot"):
        D.check_nested(None, ["GGGG"], knotted)
    with pytest.raises(ValueError, match=r"row\(s\) \[1, 3\]"):
        D.design_nested_from_logits(torch.zeros(4, 8, 4), mask=torch.ones(4, 8), constraints=knotted, require=["GNRA"])
    with pytest.raises(ValueError, match="require or avoid is required"):
        D.design_nested_from_logits(torch.zeros(2, 8, 4), mask=torch.ones(2, 8), constraints=nested)
    with pytest.raises(RuntimeError, match="rnampnn_design_nested runs on an MI355X"):
        D.design_nested_from_logits(torch.zeros(2, 8, 4), mask=torch.ones(2, 8), constraints=nested, avoid=["GGGG"], max_run=3)
    # without the switch the refusals of base pairs keep their words
    with pytest.raises(ValueError, match="require together with base pairs is not built.*drop `structure`"):
        D.check_require(["GGAGG"], None, nested)
    with pytest.raises(ValueError, match="avoid together with base pairs is not built.*drop `structure`"):
        D.check_avoid(["GGGG"], nested)


def test_the_models_take_pairs_and_refuse_before_their_forward_pass(monkeypatch):
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    nested = DesignConstraints.from_specs([("GNRA....", "((....))")], [8], 8)
    knotted = DesignConstraints.from_specs([(None, "([..)]..")], [8], 8)
    for cls in (RNAMPNN, RNAModel):
        def forward_ran(*a, **k):
            pytest.fail("the forward pass ran")
        for name in ("_run", "_packed_logits"):
            if hasattr(cls, name):
                monkeypatch.setattr(cls, name, forward_ran)
        model = cls.__new__(cls)
        x, mask = torch.zeros(1, 8, 7, 3), torch.ones(1, 8)
        with pytest.raises(ValueError, match=r"row\(s\) \[0\] holds a pseudoknot"):
            cls.design(model, x, mask, avoid=["GGGG"], constraints=knotted, pairs="nested")
        with pytest.raises(ValueError, match="pairs='nested' together with gc_content is not built"):
            cls.design(model, x, mask, avoid=["GGGG"], constraints=nested, pairs="nested", gc_content=(0.4, 0.6))
        with pytest.raises(ValueError, match="pairs='nested' needs avoid and / or require"):
            cls.design(model, x, mask, constraints=nested, pairs="nested")
        with pytest.raises(ValueError, match="pairs must be None or 'nested'"):
            cls.design(model, x, mask, avoid=["GGGG"], constraints=nested, pairs="knots")
        # the same calls without the switch raise what they raised
        with pytest.raises(ValueError, match="avoid together with base pairs is not built"):
            cls.design(model, x, mask, avoid=["GGGG"], constraints=nested)
        with pytest.raises(ValueError, match="require together with base pairs is not built"):
            cls.design(model, x, mask, require=["GNRA"], constraints=nested)


def test_the_cli_refuses_before_a_checkpoint_is_opened(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
    import predict as P
    base = ["--ckpt", "none.pt", "--data", "none"]
    cons = tmp_path / "cons.csv"
    cons.write_text("pdb_id,fixed,structure\nr2,,((((....))))\nr0,,((..[[..))..]]\nr1,,........\nr3,,([)]\n")
    with pytest.raises(ValueError, match="--pairs nested needs --samples"):
        P.run(P.parse(base + ["--pairs", "nested", "--avoid", "GGGG"]))
    with pytest.raises(ValueError, match="--pairs nested needs --avoid, --max-run or --require"):
        P.run(P.parse(base + ["--pairs", "nested", "--samples", "2", "--constraints", str(cons)]))
    for flag, value in (("--profile-out", "prefix"), ("--states", "states.csv"), ("--gc-content", "0.4:0.6"), ("--distinct", "sample"),
                        ("--max-mutations", "3")):
        with pytest.raises(ValueError, match=f"--pairs nested together with {flag} is not built"):
            P.run(P.parse(base + ["--samples", "2", "--pairs", "nested", "--avoid", "GGGG", flag, value]))
    for motif in (["--avoid", "GGGG"], ["--max-run", "3"], ["--require", "GNRA", "--max-run", "3"]):
        with pytest.raises(ValueError, match=r"pairs='nested': the structure of \['r0', 'r3'\] holds a pseudoknot"):
            P.run(P.parse(base + ["--samples", "2", "--pairs", "nested", "--constraints", str(cons)] + motif))
    with pytest.raises(SystemExit):
        P.parse(base + ["--pairs", "knots"])
    with pytest.raises(ValueError, match="unknown letter 'X'"):
        P.run(P.parse(base + ["--samples", "2", "--pairs", "nested", "--require", "GXA"]))
    ok = tmp_path / "ok.csv"
    ok.write_text("pdb_id,fixed,structure\nr2,,((((....))))\n")
    args = P.parse(base + ["--samples", "2", "--pairs", "nested", "--require", "GNRA", "--avoid", "GAATTC", "--max-run", "3", "--constraints", str(ok)])
    opt = P.nested_option(args)
    assert opt["pairs"] == "nested" and opt["require"].letters() == ["AAAA", "UUUU", "CCCC", "GAAUUC", "GGGG"] and len(opt["require"].required) == 1
    alone = P.nested_option(P.parse(base + ["--samples", "2", "--pairs", "nested", "--max-run", "3"]))
    assert alone["require"].n_live == 13 and alone["require"].required == () and P.nested_option(P.parse(base)) == {}
    # without --pairs the structure is refused in today's words (the table is read after the checkpoint, so the library call is direct)
    from rnampnn.utils.constraints import read_constraints_csv
    from rnampnn.utils.predict import check_require_run
    with pytest.raises(ValueError, match="require together with base pairs is not built .*drop `structure` from the constraints of \\['r2'\\]"):
        check_require_run(["GNRA"], None, 2, None, read_constraints_csv(str(ok)))


def test_predict_refuses_a_profile_and_knots_in_both_families():
    from rnampnn.utils.predict import check_nested_run
    table = {"a": ("", "((..))"), "b": ("", "([)]"), "c": ("", "")}
    with pytest.raises(ValueError, match="a design profile together with pairs='nested' is not built"):
        check_nested_run(None, ["GGGG"], 2, "prefix", {})
    with pytest.raises(ValueError, match="need samples > 0"):
        check_nested_run(None, ["GGGG"], 0, None, {})
    with pytest.raises(ValueError, match=r"\['b'\] holds a pseudoknot"):
        check_nested_run(["GNRA"], None, 2, None, table)
    auto = check_nested_run(["GNRA"], None, 2, None, {"a": table["a"]})
    assert isinstance(auto, M.DesignAutomaton) and len(auto.required) == 1 and check_nested_run(None, ["GGGG"], 2, None, None).n_live == 4
    import rdesign.utils.predict as RP
    import rnampnn.utils.predict as NP
    for module in (NP, RP):
        with pytest.raises(ValueError, match=r"\['b'\] holds a pseudoknot"):
            module.predict(None, "none", "none.csv", samples=2, constraints=table, avoid=["GGGG"], pairs="nested")
        with pytest.raises(ValueError, match="avoid together with base pairs is not built"):
            module.predict(None, "none", "none.csv", samples=2, constraints=table, avoid=["GGGG"])


def test_the_designs_csv_gains_four_columns():
    from rnampnn.utils.predict import design_columns
    extras = (torch.tensor([[0, 2]]), torch.tensor([[1, 0]]), torch.tensor([0, 1]), torch.tensor([0, 1]))
    header, cells, filled = design_columns("nested", extras, [5, 5])
    assert header == ",motif_hits,required_found,require_miss,nest_miss" and filled is None
    assert cells(0, 0) == (0, 1, 0, 0) and cells(0, 1) == (2, 0, 1, 1)
    assert design_columns("require")[0] == ",motif_hits,required_found,require_miss" and design_columns("avoid")[0] == ",motif_hits,avoid_miss"


def test_the_build_and_the_binding_know_the_new_unit():
    import __graft_entry__ as g
    from rnampnn import _native
    assert "design_nested.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_nested.hip"))
    assert {"rnampnn_design_nested", "rnampnn_design_nested_workspace_bytes"} <= set(_native.SYMBOLS)
    header = open(os.path.join(REPO, "include", "rnampnn_hip.h")).read()
    assert "#define RNAMPNN_DESIGN_NESTED_MAX_LIVE 64" in header and "int rnampnn_design_nested(" in header
