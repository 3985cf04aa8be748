"""The host side of design that avoids forbidden motifs, without a GPU: the automaton ``rnampnn.utils.motifs`` builds, ``hits`` against a
substring scan, the float64 restatement of ``rnampnn_design_avoid`` (tests/_design_avoid_ref.py) against an enumerated joint, the
refusals of ``design_mode`` and of base pairs, and the share of the device tests' draws that pass close to a cumulative boundary."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_avoid_ref as R  # noqa: E402
from _design_gc_ref import NEG, lse  # noqa: E402
from rnampnn.model import decode as D  # noqa: E402
from rnampnn.utils.motifs import MAX_STATES, MotifAutomaton, as_automaton  # noqa: E402

NEAR = 1e-8
A_, U_, C_, G_ = 0, 1, 2, 3


def _words_of(auto):
    """The strings the automaton accepts the end of, read off its tables alone: every word up to length 6 whose walk ends terminal."""
    delta, out = auto.delta.tolist(), set()
    for n in range(1, 7):
        for w in itertools.product(range(4), repeat=n):
            a = 0
            for c in w:
                a = delta[a][c]
            if (auto.terminal >> a) & 1:
                out.add(w)
    return out


# ---------------------------------------------------------------------------------------------------------------- the automaton
def test_tables_for_gggg():
    a = MotifAutomaton.from_motifs(["GGGG"])
    assert a.delta.dtype == torch.uint8 and a.delta.tolist() == [[0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3], [0, 0, 0, 4], [0, 0, 0, 4]]
    assert a.terminal == 1 << 4 and a.n_states == 5 and a.n_live == 4 and a.letters() == ["GGGG"]


def test_max_run_3_has_13_live_states():
    """No run longer than 3: the trie of AAAA, UUUU, CCCC, GGGG has the root, 4 x 3 live states - the 13 columns of the kernel's table -
    and the four terminal ones, numbered last (breadth-first)."""
    a = MotifAutomaton.from_motifs([], max_run=3)
    assert a.n_live == 13 and a.n_states == 17 and a.terminal == 0b1111 << 13
    assert a.delta[0].tolist() == [1, 2, 3, 4] and a.delta[4].tolist() == [1, 2, 3, 8] and a.delta[12].tolist() == [1, 2, 3, 16]
    assert a.delta[16].tolist() == [1, 2, 3, 16]                  # GGGG + G ends GGGG again
    assert MotifAutomaton.from_motifs(["AAAA", "UUUU", "CCCC", "GGGG"]).delta.tolist() == a.delta.tolist()


def test_a_motif_that_is_a_suffix_of_another_marks_both_states():
    a = MotifAutomaton.from_motifs(["UGGA", "GGA"])
    # 0 root, 1 U, 2 G, 3 UG, 4 GG, 5 UGG, 6 GGA, 7 UGGA
    assert a.delta.tolist() == [[0, 1, 0, 2], [0, 1, 0, 3], [0, 1, 0, 4], [0, 1, 0, 5], [6, 1, 0, 4], [7, 1, 0, 4], [0, 1, 0, 2], [0, 1, 0, 2]]
    assert a.terminal == 0b11000000
    b = MotifAutomaton.from_motifs(["UGGAC", "GGA"])              # GGA ends inside UGGAC: the state UGGA is terminal through its suffix link
    words = _words_of(b)
    assert (U_, G_, G_, A_) in words and (G_, G_, A_) in words and (U_, G_, G_, A_, C_) in words and (U_, G_, G_) not in words


def test_overlapping_motifs_follow_their_suffix_links():
    a = MotifAutomaton.from_motifs(["GGA", "GAC", "ACGU"])
    seq = torch.tensor([[G_, G_, A_, C_, G_, U_, -1, -1]])         # GGA at 2, GAC at 3, ACGU at 5: each starts inside the one before
    assert a.hits(seq).tolist() == [3] and a.hits(torch.tensor([G_, G_, C_, A_, C_, G_, G_])).item() == 0
    assert R.naive_hits(seq[0].tolist(), R.expand(["GGA", "GAC", "ACGU"])) == 3


def test_iupac_t_order_and_duplicates():
    a = MotifAutomaton.from_motifs(["GGWCC"])
    assert a.letters() == ["GGACC", "GGUCC"] and a.delta.tolist() == MotifAutomaton.from_motifs(["GGUCC", "GGACC"]).delta.tolist()
    assert MotifAutomaton.from_motifs(["GGTCC"]).delta.tolist() == MotifAutomaton.from_motifs(["ggucc"]).delta.tolist()
    x = MotifAutomaton.from_motifs(["GGA", "ACGU", "GAC", "UGGA"], max_run=4)
    y = MotifAutomaton.from_motifs(["UGGA", "GAC", "GGA", "GGA", "ACGT", "GAC"], max_run=4)
    assert x.delta.tolist() == y.delta.tolist() and x.terminal == y.terminal and not x.terminal & 1
    assert len(MotifAutomaton.from_motifs(["NN"]).words) == 16 and as_automaton(None) is None and as_automaton(x) is x
    assert as_automaton("GGGG").delta.tolist() == MotifAutomaton.from_motifs(["GGGG"]).delta.tolist()


def test_64_states_are_accepted_and_65_refused():
    motifs, _ = R.CASE_AUTOMATA["states64"]
    a = MotifAutomaton.from_motifs(motifs)
    assert a.n_states == MAX_STATES == 64 and a.n_live == 57 and int(a.delta.max()) == 63
    with pytest.raises(ValueError, match=r"has 65 states, the limit is 64"):
        MotifAutomaton.from_motifs(list(motifs[:-1]) + [motifs[-1] + "A"])


@pytest.mark.parametrize("motifs, max_run, match", [([""], None, "empty motif"), (["GG", " "], None, "empty motif"), (["GGXA"], None, "unknown letter 'X'"),
                                                    (["GG.A"], None, "unknown letter"), ([], None, "no motif given"), ([], 0, "max_run = 0")])
def test_value_errors(motifs, max_run, match):
    with pytest.raises(ValueError, match=match):
        MotifAutomaton.from_motifs(motifs, max_run=max_run)


@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
def test_hits_equal_a_substring_scan(name):
    motifs, max_run = R.CASE_AUTOMATA[name]
    auto, words = MotifAutomaton.from_motifs(motifs, max_run=max_run), R.expand(motifs, max_run)
    assert {tuple(w) for w in auto.words} == words
    rng = np.random.RandomState(3)
    seqs = rng.choice(4, size=(3, 40, 48), p=[0.2, 0.2, 0.1, 0.5]).astype(np.int8)
    seqs[0, 0, 4:14] = [LETTER for LETTER in (G_, A_, A_, U_, U_, C_, A_, A_, G_, C_)]
    for i in range(40):
        seqs[:, i, 48 - i:] = -1                                    # lengths 48 .. 9, a row of every length in between
    got = auto.hits(torch.from_numpy(seqs))
    want = np.array([[R.naive_hits(row, words) for row in plane] for plane in seqs])
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 40) and np.array_equal(got.numpy(), want) and want.sum() > 0


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name, n", [("max_run3", 6), ("overlap", 6), ("overlap", 5), ("max_run3", 1)])
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_path_logprob_is_the_enumerated_joint_over_motif_free_sequences(name, n, temperature):
    """Every one of the 4^n sequences: the product of the walk's conditionals equals the tempered, biased joint restricted to the admitted
    sequences without a motif (by substring comparison) and renormalised, to 1e-12; it is -inf for the rest."""
    motifs, max_run = R.CASE_AUTOMATA[name]
    auto, words = MotifAutomaton.from_motifs(motifs, max_run=max_run), R.expand(motifs, max_run)
    rng = np.random.RandomState(7 + n)
    logits = (2.0 * rng.standard_normal((n, 4))).astype(np.float32)
    logits[:, 3] += 2.0
    bias = rng.standard_normal((n, 4)).astype(np.float32)
    allowed = np.full(n, 15, dtype=np.uint8)
    if n >= 5:
        allowed[1], allowed[3], allowed[4] = 8 | 1, 0, 15 ^ 4       # G or A; empty: free; no C
    plan = R.AvoidPlan(logits, n, temperature, auto.delta.numpy(), auto.terminal, allowed, bias)
    assert plan.miss == 0 and plan.infeasible == int(n >= 5)
    z = (logits.astype(np.float64) + bias.astype(np.float64)) / float(np.float32(temperature))
    mask = np.where(allowed == 0, 15, allowed)
    joint = {}
    for seq in itertools.product(range(4), repeat=n):
        if all((mask[t] >> seq[t]) & 1 for t in range(n)) and R.naive_hits(seq, words) == 0:
            joint[seq] = sum(z[t, seq[t]] for t in range(n))
    total = lse(np.array(list(joint.values())))
    assert 0 < len(joint) < 4 ** n or n == 1
    assert abs(plan.l[0, 0] - total) <= 1e-12 * max(1.0, abs(total))
    for seq in itertools.product(range(4), repeat=n):
        lp = plan.path_logprob(seq)
        if seq in joint:
            assert abs(lp - (joint[seq] - total)) <= 1e-12 * max(1.0, abs(lp)), seq
        else:
            assert lp == NEG, seq


def test_an_rna_whose_fixed_positions_spell_a_motif_falls_back_to_the_free_draw():
    auto = MotifAutomaton.from_motifs(["GGA"])
    logits = np.random.RandomState(1).standard_normal((5, 4)).astype(np.float32)
    allowed = np.array([15, 8, 8, 1, 15], dtype=np.uint8)
    plan = R.AvoidPlan(logits, 5, 1.0, auto.delta.numpy(), auto.terminal, allowed)
    assert plan.miss == 1 and not plan.l[0, 0] > NEG
    free = R.AvoidPlan(logits, 5, 1.0, np.zeros((1, 4), dtype=np.uint8), 0, allowed)      # the one-state automaton: no motif
    assert free.miss == 0
    for s in range(8):
        seq, _ = plan.draw(11, s, 0)
        assert np.array_equal(seq, free.draw(11, s, 0)[0]) and seq[1:4].tolist() == [G_, G_, A_] and R.naive_hits(seq, R.expand(["GGA"])) == 1


# ---------------------------------------------------------------------------------------------------------------- the mode and its refusals
def test_design_mode_names_every_new_pair():
    auto = MotifAutomaton.from_motifs(["GGGG"])
    assert D.DESIGN_MODES[0][0] == "avoid" and D.design_mode(avoid=auto) == "avoid" and D.design_mode() == "plain"
    assert D.design_mode(None, (0.4, 0.6)) == "gc_content" and D.design_mode([2], None, None, None) == "states"     # existing callers
    for name, value in (("states", [1]), ("gc_content", (0.4, 0.6)), ("distinct", "sample"), ("mutations", (torch.zeros(1, 4), 2))):
        with pytest.raises(ValueError, match=f"avoid together with {name} is not built"):
            D.design_mode(avoid=auto, **{name: value})


def test_base_pairs_are_refused_without_touching_a_device(monkeypatch):
    """The refusal comes from ``check_avoid``, which the models call before their forward pass: no library is loaded and no tensor moved."""
    from rnampnn import _native
    from rnampnn.utils.constraints import DesignConstraints
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the library was loaded"))
    paired = DesignConstraints.from_specs([("GNRA....", "((....))")], [8], 8)
    with pytest.raises(ValueError, match="avoid together with base pairs is not built.*drop `structure`"):
        D.check_avoid(["GGGG"], paired)
    with pytest.raises(ValueError, match="drop `structure`"):
        D.design_avoid_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), constraints=paired, avoid=["GGGG"])
    fixed = DesignConstraints.from_specs([("GNRA....", None)], [8], 8, bias=[0, 0, 0, 1.0], omit="C")
    assert fixed.partner is None and D.check_avoid(["GGGG"], fixed).n_states == 5 and D.check_avoid(None, paired) is None
    with pytest.raises(ValueError, match="avoid is required"):
        D.design_avoid_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8))
    with pytest.raises(RuntimeError, match="rnampnn_design_avoid runs on an MI355X"):
        D.design_avoid_from_logits(torch.zeros(1, 8, 4), mask=torch.ones(1, 8), constraints=fixed, avoid=["GGGG"])


def test_the_cli_refuses_before_a_model_is_loaded():
    sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
    import predict as P
    base = ["--ckpt", "none.pt", "--data", "none"]
    with pytest.raises(ValueError, match="need --samples"):
        P.run(P.parse(base + ["--avoid", "GGGG"]))
    with pytest.raises(ValueError, match="--avoid / --max-run together with --gc-content is not built"):
        P.run(P.parse(base + ["--samples", "2", "--max-run", "3", "--gc-content", "0.4:0.6"]))
    with pytest.raises(ValueError, match="unknown letter 'X'"):
        P.run(P.parse(base + ["--samples", "2", "--avoid", "GGGG,GXA"]))
    opt = P.avoid_option(P.parse(base + ["--samples", "2", "--avoid", "GGGG, GAATTC", "--max-run", "3"]))
    assert opt["avoid"].letters() == ["AAAA", "UUUU", "CCCC", "GAAUUC", "GGGG"] and P.avoid_option(P.parse(base)) == {}


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_the_case_batch_keeps_clear_of_the_boundaries_and_holds_no_motif(name, temperature):
    """The restatement alone: at most 1 % of the batch's (sample, RNA) draws pass within 1e-8 of a cumulative boundary (the device test
    leaves those out and asserts the same cap); every feasible RNA's draws hold no motif, the infeasible one's do."""
    motifs, max_run = R.CASE_AUTOMATA[name]
    auto = MotifAutomaton.from_motifs(motifs, max_run=max_run)
    seqs, margin, bad, miss, hits, plans = R.case_ref(name, auto.delta.numpy(), auto.terminal, temperature)
    near = margin <= NEAR
    print(f"{name}, temperature {temperature}: {near.mean():.4%} of the {near.size} draws within {NEAR} of a boundary")
    assert near.mean() <= 0.01
    assert bad.tolist() == R.CASE_INFEASIBLE and miss.tolist() == R.CASE_MISS
    assert (hits[:, [b for b in range(len(miss)) if not miss[b]]] == 0).all() and (hits[:, 4] > 0).all()
    assert np.array_equal(auto.hits(torch.from_numpy(seqs)).numpy(), hits)
    assert (seqs[:, 4, 10:15] == np.array([G_, G_, G_, G_, A_])).all() and (seqs[:, 6, 20:23] == G_).all()
    if name == "max_run3":
        assert (seqs[:, 6, 19] != G_).all() and (seqs[:, 6, 23] != G_).all()        # the only escapes are forced
    # what the motifs cost: with G raised by 6 a free draw of the 300-mer is full of GGGG
    free = R.AvoidPlan(R.case_arrays()["logits"][8], 300, temperature, np.zeros((1, 4), dtype=np.uint8), 0).draw(R.CASE_SEED, 0, 8)[0]
    assert R.naive_hits(free, R.expand(["GGGG"])) > 50
