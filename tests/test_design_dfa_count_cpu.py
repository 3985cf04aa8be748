"""The host side of design with motifs under a count window, without a GPU: the float64 restatement of ``rnampnn_design_dfa_count``
(tests/_design_dfa_count_ref.py) against an enumerated joint, against ``_design_dfa_ref`` where nothing counts and across caps; the share
of the device tests' draws that pass close to a cumulative boundary; and the Python surface: ``design_mode(combine=...)`` with every
accepted and refused combination, the refusal of base pairs, the CLI's refusals before a checkpoint is opened, the CSV's columns and the
workspace arithmetic of the binding."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_avoid_ref as AV  # noqa: E402
import _design_dfa_ref as DR  # noqa: E402
import _design_dfa_count_ref as R  # noqa: E402
from _design_gc_ref import NEG, lse  # noqa: E402
from rnampnn.model import decode as D  # noqa: E402
from rnampnn.utils import motifs as M  # noqa: E402

NEAR = 1e-8
AUTOMATA = [(("GA",), ("CC",), 2), (None, ("UGG", "GAC"), 3)]    # a required word beside avoided ones; forbidden motifs alone


def _auto(require, avoid=None, max_run=None):
    return M.as_nested_automaton(require, avoid, max_run)


def _brute(n, z, mask, groups, banned, counted, lo, hi):
    """{admitted sequence holding the motifs: (its log-weight, its count)}, by substring scan and recount."""
    joint = {}
    for seq in itertools.product(range(4), repeat=n):
        if all((mask[t] >> seq[t]) & 1 for t in range(n)) and DR.contains_all(seq, groups) and AV.naive_hits(seq, banned) == 0:
            joint[seq] = (sum(z[t, seq[t]] for t in range(n)), R.recount(seq, counted))
    return joint


# ---------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("spec", AUTOMATA)
@pytest.mark.parametrize("side", ["gc", "mut"])
def test_log_z_and_path_logprob_are_the_enumerated_joint_for_every_sequence_up_to_length_7(spec, side):
    """Every length 0..7 and every one of its 4^n sequences: log_z equals the brute-force sum over the sequences that hold the motifs
    (substring scan) with a count (recount) in the window within 1e-12; the product of the draw's conditionals equals the renormalised
    joint within 1e-12; it is -inf outside the conditions.  An unreachable window falls on the nearest reachable count."""
    require, avoid, max_run = spec
    auto = _auto(require, avoid, max_run)
    groups, banned = DR.required_sets(require or ()), AV.expand(avoid or (), max_run)
    for n in range(8):
        rng = np.random.RandomState(31 + n)
        logits = (2.0 * rng.standard_normal((n, 4))).astype(np.float32)
        bias = rng.standard_normal((n, 4)).astype(np.float32)
        allowed = np.full(n, 15, dtype=np.uint8)
        if n >= 5:
            allowed[0], allowed[2] = 0, 15 ^ 4                       # empty: free; no C
        if side == "gc":
            counted, (lo, hi), cap = np.full(n, 12, dtype=np.uint8), (2, 4), n
        else:
            counted, (lo, hi), cap = (15 ^ (1 << rng.randint(0, 4, size=n))).astype(np.uint8), (1, 3), 3
        temperature = 1.0 if n % 2 else 0.3
        plan = R.DfaCountPlan(logits, n, temperature, auto.delta.numpy(), auto.kind.numpy(), counted, lo, hi, cap, allowed, bias)
        z = (logits.astype(np.float64) + bias.astype(np.float64)) / float(np.float32(temperature))
        mask = np.where(allowed == 0, 15, allowed)
        joint = _brute(n, z, mask, groups, banned, counted, lo, hi)
        K = min(cap, n)
        wl = min(max(lo, 0), K)
        wh = max(min(max(hi, 0), K), wl)
        reachable = sorted({k for _, k in joint.values() if k <= K})
        if not reachable:
            assert plan.dfa_miss == 1 and plan.count_miss == 0 and plan.log_z == NEG
            continue
        inside = [k for k in reachable if wl <= k <= wh]
        if inside:
            keep, miss = set(inside), 0
        else:
            miss = min(min(abs(k - wl), abs(k - wh)) for k in reachable)
            keep = {min(k for k in reachable if min(abs(k - wl), abs(k - wh)) == miss)}     # the lower one on a tie
        assert plan.dfa_miss == 0 and plan.count_miss == miss, (n, plan.count_miss, miss)
        total = lse(np.array([w for w, k in joint.values() if k in keep]))
        assert abs(plan.log_z - total) <= 1e-12 * max(1.0, abs(total)), (n, plan.log_z, total)
        mass = 0.0
        for seq in itertools.product(range(4), repeat=n):
            lp = plan.path_logprob(seq)
            if seq in joint and joint[seq][1] in keep:
                assert abs(lp - (joint[seq][0] - total)) <= 1e-12 * max(1.0, abs(lp)), (n, seq)
                mass += np.exp(lp)
            else:
                assert lp == NEG, (n, seq)
        assert abs(mass - 1.0) <= 1e-12


def test_the_prototypes_partition_sum():
    """Require GA, avoid CC, no run longer than 2, G+C in 2..4 of 7: 3,156 admitted sequences; log Z by the chain equals the sum."""
    auto = _auto(("GA",), ("CC",), 2)
    rng = np.random.RandomState(0)
    logits = rng.standard_normal((7, 4)).astype(np.float32)
    plan = R.DfaCountPlan(logits, 7, 1.0, auto.delta.numpy(), auto.kind.numpy(), np.full(7, 12, dtype=np.uint8), 2, 4, 7)
    joint = _brute(7, logits.astype(np.float64), np.full(7, 15), DR.required_sets(("GA",)), AV.expand(("CC",), 2), np.full(7, 12), 2, 4)
    kept = [w for w, k in joint.values() if 2 <= k <= 4]
    assert len(kept) == 3156 and abs(plan.log_z - lse(np.array(kept))) <= 1e-12 * abs(plan.log_z)


# ---------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
def test_nothing_counted_reproduces_the_dfa_restatement_exactly(name):
    auto = _auto(*R.CASE_AUTOMATA[name])
    h = R.case_arrays()
    B, T = h["mask"].shape
    zero = np.zeros(B, dtype=np.int32)
    want = DR.design_dfa_ref(h["logits"], R.CASE_LENGTHS, 0.3, R.CASE_S, R.CASE_SEED, auto.delta.numpy(), auto.kind.numpy(), h["allowed"], h["bias"])
    for cap in (T, 0):
        got = R.design_dfa_count_ref(h["logits"], R.CASE_LENGTHS, 0.3, R.CASE_S, R.CASE_SEED, auto.delta.numpy(), auto.kind.numpy(),
                                     np.zeros((B, T), dtype=np.uint8), zero, zero, cap, h["allowed"], h["bias"])
        for k in ("seqs", "infeasible", "dfa_miss", "hits", "accepted"):
            assert np.array_equal(got[k], want[k]), (cap, k)
        assert not got["count"].any() and not got["count_miss"].any()
        assert all(np.array_equal(p.l[:, :, 0], q.l) for p, q in zip(got["plans"], want["plans"]))
        assert np.array_equal(got["log_z"], np.array([q.l[0, 0] if q.n else (0.0 if not q.miss else NEG) for q in want["plans"]]))


def test_the_draws_do_not_depend_on_the_cap():
    auto = _auto(*R.CASE_AUTOMATA["gnra_run3"])
    h = R.case_arrays()
    for side in ("mut4", "mut2_6"):
        counted, lo, hi, cap = R.case_side(side, h)
        base = R.case_ref("gnra_run3", side, auto.delta.numpy(), auto.kind.numpy(), 0.3)
        keep = [b for b in range(len(R.CASE_LENGTHS)) if not base["dfa_miss"][b] and not base["count_miss"][b]]
        assert len(keep) >= 4
        for other in (cap + 3, R.CASE_T, 100000):
            out = R.design_dfa_count_ref(h["logits"], R.CASE_LENGTHS, 0.3, R.CASE_S, R.CASE_SEED, auto.delta.numpy(), auto.kind.numpy(), counted, lo,
                                         hi, other, h["allowed"], h["bias"])
            assert np.array_equal(out["seqs"][:, keep], base["seqs"][:, keep]) and np.array_equal(out["log_z"][keep], base["log_z"][keep])
            assert np.array_equal(out["count"][:, keep], base["count"][:, keep])


# ---------------------------------------------------------------------------------------------------------------- the device tests' batch
def test_the_case_automata_have_the_sizes_the_tests_name():
    assert {name: _auto(*spec).n_live for name, spec in R.CASE_AUTOMATA.items()} == R.CASE_LIVE


@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("side", R.CASE_SIDES)
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_the_case_batch_keeps_clear_of_the_boundaries_and_holds_both_conditions(name, side, temperature):
    """The restatement alone: at most 5 % of the batch's (sample, RNA) draws pass within 1e-8 of a cumulative boundary - the cap the
    device comparison may leave out; every feasible RNA's draws hold the motifs and a count inside the window (or on the target)."""
    require, avoid, max_run = R.CASE_AUTOMATA[name]
    auto = _auto(require, avoid, max_run)
    ref = R.case_ref(name, side, auto.delta.numpy(), auto.kind.numpy(), temperature)
    near = ref["margin"] <= NEAR
    print(f"{name}, {side}, temperature {temperature}: {near.mean():.4%} of the {near.size} draws within {NEAR} of a boundary")
    assert near.mean() <= 0.05
    assert ref["infeasible"].tolist() == R.CASE_INFEASIBLE
    groups, banned = DR.required_sets(require or ()), AV.expand(avoid or (), max_run)
    counted, lo, hi, cap = R.case_side(side)
    for b, plan in enumerate(ref["plans"]):
        for s in range(R.CASE_S):
            seq = ref["seqs"][s, b]
            assert ref["count"][s, b] == R.recount(seq, counted[b])
            if plan.dfa_miss:
                continue
            assert DR.contains_all(seq, groups) and AV.naive_hits(seq, banned) == 0 and ref["hits"][s, b] == 0 and ref["accepted"][s, b] == 1
            assert (plan.lo <= ref["count"][s, b] <= plan.hi) if plan.any else (ref["count"][s, b] == plan.target), (s, b)
    assert ref["dfa_miss"][1:4].tolist() == ([0, 0, 0] if name == "run3" else [1, 1, 1]) and ref["dfa_miss"][7] == 0
    if side == "gc":                                                # the row whose fixed positions keep G+C below the window
        assert ref["dfa_miss"][5] == int(name == "two_run3") and ref["count_miss"][5] == (0 if name == "two_run3" else 3)
        assert name == "two_run3" or (ref["plans"][5].target == 5 and (ref["count"][:, 5] == 5).all())
    hits, accepted = auto.scan(torch.from_numpy(ref["seqs"]))
    assert np.array_equal(hits.numpy(), ref["hits"]) and np.array_equal(accepted.numpy(), ref["accepted"])


# ---------------------------------------------------------------------------------------------------------------- the mode and its refusals
def test_design_mode_combine_accepts_and_refuses():
    ref = (torch.zeros(1, 4), 2)
    for motif in (dict(avoid=["GGGG"]), dict(require=["GNRA"]), dict(max_run=3), dict(avoid=["GGGG"], require=["GNRA"], max_run=3)):
        assert D.design_mode(gc_content=(0.4, 0.6), combine="chain", **motif) == "chain"
        assert D.design_mode(mutations=ref, combine="chain", **motif) == "chain"
    assert D.design_mode(gc_content=(0.4, 0.6), avoid=["GGGG"], combine="chain", tree="lds") == "chain"
    with pytest.raises(ValueError, match="combine must be None or 'chain', got 'tree'"):
        D.design_mode(gc_content=(0.4, 0.6), avoid=["GGGG"], combine="tree")
    with pytest.raises(ValueError, match="combine='chain' needs avoid, require or max_run.*drop combine="):
        D.design_mode(gc_content=(0.4, 0.6), combine="chain")
    with pytest.raises(ValueError, match="exactly one of gc_content and mutations \\(two counts at once are not built\\)"):
        D.design_mode(gc_content=(0.4, 0.6), mutations=ref, avoid=["GGGG"], combine="chain")
    with pytest.raises(ValueError, match="exactly one of gc_content and mutations"):
        D.design_mode(avoid=["GGGG"], combine="chain")
    for name, value in (("states", [1]), ("distinct", "sample")):
        with pytest.raises(ValueError, match=f"combine='chain' together with {name} is not built"):
            D.design_mode(gc_content=(0.4, 0.6), avoid=["GGGG"], combine="chain", **{name: value})
    with pytest.raises(ValueError, match="combine='chain' together with pairs is not built"):
        D.design_mode(gc_content=(0.4, 0.6), avoid=["GGGG"], combine="chain", pairs="nested")
    for tree in ("global", "auto"):
        with pytest.raises(ValueError, match=f"combine='chain' together with tree='{tree}' is not built"):
            D.design_mode(gc_content=(0.4, 0.6), avoid=["GGGG"], combine="chain", tree=tree)


def test_with_combine_none_every_existing_message_is_unchanged():
    assert D.DESIGN_MODES[0] == ("avoid", ("states", "gc_content", "distinct", "mutations"),
                                 "the automaton conditions the draws of rnampnn_design on the motifs alone")
    ref = (torch.zeros(1, 4), 2)
    for name, value in (("states", [1]), ("gc_content", (0.4, 0.6)), ("distinct", "sample"), ("mutations", ref)):
        for combine in ({}, dict(combine=None)):
            with pytest.raises(ValueError, match=f"avoid together with {name} is not built: the automaton conditions the draws of rnampnn_design "
                                                 "on the motifs alone"):
                D.design_mode(avoid=["GGGG"], **{name: value}, **combine)
            with pytest.raises(ValueError, match=f"require together with {name} is not built: the automaton conditions"):
                D.design_mode(require=["GNRA"], **{name: value}, **combine)
            with pytest.raises(ValueError, match=f"pairs='nested' together with {name} is not built"):
                D.design_mode(avoid=["GGGG"], pairs="nested", **{name: value}, **combine)
    with pytest.raises(ValueError, match="mutations together with gc_content is not built: the budget conditions"):
        D.design_mode(gc_content=(0.4, 0.6), mutations=ref)
    assert D.design_mode(gc_content=(0.4, 0.6), max_run=3, tree="global") == "gc_content"      # read by the chain alone
    assert D.design_mode() == "plain" and D.design_mode(avoid=["GGGG"]) == "avoid" and D.design_mode(require=["GNRA"], avoid=["GG"]) == "require"


def test_base_pairs_and_bad_arguments_are_refused_without_touching_a_device(monkeypatch):
    from rnampnn import _native
    from rnampnn.utils.constraints import DesignConstraints
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the library was loaded"))
    paired = DesignConstraints.from_specs([("GNRA....", "((....))")], [8], 8)
    lg, mask = torch.zeros(1, 8, 4), torch.ones(1, 8)
    with pytest.raises(ValueError, match="require together with base pairs is not built.*drop `structure`"):
        D.design_dfa_count_from_logits(lg, mask=mask, constraints=paired, require=["GGAGG"], gc_content=(0.4, 0.6))
    with pytest.raises(ValueError, match="avoid together with base pairs is not built.*drop `structure`"):
        D.design_dfa_count_from_logits(lg, mask=mask, constraints=paired, max_run=3, gc_content=(0.4, 0.6))
    with pytest.raises(ValueError, match="require, avoid or max_run is required"):
        D.design_dfa_count_from_logits(lg, mask=mask, gc_content=(0.4, 0.6))
    with pytest.raises(ValueError, match="exactly one of gc_content and mutations"):
        D.design_dfa_count_from_logits(lg, mask=mask, avoid=["GGGG"])
    with pytest.raises(ValueError, match="exactly one of gc_content and mutations"):
        D.design_dfa_count_from_logits(lg, mask=mask, avoid=["GGGG"], gc_content=(0.4, 0.6), mutations=(torch.zeros(1, 8), (0, 2)))
    with pytest.raises(RuntimeError, match="rnampnn_design_dfa_count runs on an MI355X"):
        D.design_dfa_count_from_logits(lg, mask=mask, avoid=["GGGG"], gc_content=(0.4, 0.6))
    a = D.check_chain(None, None, ["GGGG"], 3)
    assert isinstance(a, M.DesignAutomaton) and a.n_live == 13 and D.check_chain(None, None, None, None) is None
    assert len(D.check_chain(None, ["GNRA"], ["GGGG"], 3).required) == 1


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
        with pytest.raises(ValueError, match="combine must be None or 'chain'"):
            cls.design(model, x, mask, require=["GGAGG"], gc_content=(0.4, 0.6), combine="both")
        with pytest.raises(ValueError, match="drop combine="):
            cls.design(model, x, mask, gc_content=(0.4, 0.6), combine="chain")
        with pytest.raises(ValueError, match="combine='chain' together with tree='global' is not built"):
            cls.design(model, x, mask, avoid=["GGGG"], gc_content=(0.4, 0.6), combine="chain", tree="global")
        with pytest.raises(ValueError, match="require together with base pairs is not built"):
            cls.design(model, x, mask, require=["GGAGG"], gc_content=(0.4, 0.6), combine="chain", constraints=paired)
        with pytest.raises(ValueError, match="require together with gc_content is not built"):      # without combine: today's message
            cls.design(model, x, mask, require=["GGAGG"], gc_content=(0.4, 0.6))


def test_the_cli_refuses_before_a_checkpoint_is_opened(tmp_path):
    import predict as P
    base = ["--ckpt", "none.pt", "--data", "none", "--samples", "2", "--combine", "chain"]
    motif, gc = ["--max-run", "3", "--require", "GNRA"], ["--gc-content", "0.4:0.6"]
    for flag, value in (("--profile-out", "prefix"), ("--states", "states.csv"), ("--distinct", "sample"), ("--pairs", "nested"), ("--tree", "global")):
        with pytest.raises(ValueError, match=f"--combine chain together with {flag} is not built"):
            P.run(P.parse(base + motif + gc + [flag, value]))
    with pytest.raises(ValueError, match="--combine chain needs --avoid, --max-run or --require"):
        P.run(P.parse(base + gc))
    with pytest.raises(ValueError, match="--combine chain needs exactly one of --gc-content and --max-mutations"):
        P.run(P.parse(base + motif))
    with pytest.raises(ValueError, match="--combine chain needs exactly one of --gc-content and --max-mutations"):
        P.run(P.parse(base + motif + gc + ["--max-mutations", "3"]))
    with pytest.raises(ValueError, match="--combine chain needs --samples"):
        P.run(P.parse(["--ckpt", "none.pt", "--data", "none", "--combine", "chain"] + motif + gc))
    with pytest.raises(ValueError, match="unknown letter 'X'"):
        P.run(P.parse(base + gc + ["--avoid", "GXA"]))
    (tmp_path / "cons.csv").write_text("pdb_id,fixed,structure\nr2," + "." * 12 + ",((((....))))\n")
    with pytest.raises(ValueError, match="combine='chain' together with base pairs is not built.*of \\['r2'\\]"):
        P.run(P.parse(base + motif + gc + ["--constraints", str(tmp_path / "cons.csv")]))
    with pytest.raises(ValueError, match="--avoid / --max-run together with --gc-content is not built"):      # without the flag: today's refusal
        P.run(P.parse(["--ckpt", "none.pt", "--data", "none", "--samples", "2", "--max-run", "3"] + gc))
    opt = P.chain_option(P.parse(base + motif + gc + ["--avoid", "GAATTC"]))
    assert opt["combine"] == "chain" and opt["require"].letters() == ["AAAA", "UUUU", "CCCC", "GAAUUC", "GGGG"] and len(opt["require"].required) == 1
    assert P.chain_option(P.parse(["--ckpt", "none.pt", "--data", "none"])) == {}
    with pytest.raises((FileNotFoundError, OSError)):              # every refusal passed: the next thing is the checkpoint
        P.run(P.parse(base + motif + gc))
    with pytest.raises((FileNotFoundError, OSError)):
        P.run(P.parse(base + ["--avoid", "GAAUUC", "--max-mutations", "6", "--min-mutations", "2"]))


def test_the_designs_csv_gains_five_columns():
    from rnampnn.utils.predict import design_columns
    extras = (torch.tensor([[0, 2]]), torch.tensor([[1, 0]]), torch.tensor([[3, 4]]), torch.tensor([0, 1]), torch.tensor([0, 2]),
              torch.tensor([-1.5, 0.0], dtype=torch.float64))
    header, cells, filled = design_columns("chain", extras, [5, 5], "gc_content")
    assert header == ",motif_hits,required_found,require_miss,gc_count,gc_miss" and filled is None
    assert cells(0, 0) == (0, 1, 0, 3, 0) and cells(0, 1) == (2, 0, 1, 4, 2)
    assert design_columns("chain", count="mutations")[0] == ",motif_hits,required_found,require_miss,mutations,mut_miss"
    assert design_columns("require")[0] == ",motif_hits,required_found,require_miss" and design_columns("gc_content")[0] == ",gc,gc_miss"


def test_the_build_and_the_binding_know_the_new_unit():
    import __graft_entry__ as g
    from rnampnn import _native
    assert "design_dfa_count.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_dfa_count.hip"))
    assert {"rnampnn_design_dfa_count", "rnampnn_design_dfa_count_workspace_bytes"} <= set(_native.SYMBOLS)
    assert len(_native.SYMBOLS["rnampnn_design_dfa_count"][1]) == 34 and len(_native.SYMBOLS["rnampnn_design_dfa"][1]) == 27
    if not os.path.exists(g.LIB):
        return                                                      # the arithmetic below needs the built library
    import ctypes as C
    lib = C.CDLL(g.LIB)
    fn = lib.rnampnn_design_dfa_count_workspace_bytes
    fn.restype, fn.argtypes = _native.SYMBOLS["rnampnn_design_dfa_count_workspace_bytes"]
    assert fn(256, 140, 13, 8) == 8 * 256 * 140 * 13 * 9 == 33546240 and fn(256, 140, 13, 140) == 525557760
    assert fn(8, 72, 73, 100000) == 8 * 8 * 72 * 73 * 73 and fn(8, 72, 73, 1) == 2 * 8 * 8 * 72 * 73
    assert fn(0, 72, 73, 8) == 0 and fn(8, 0, 73, 8) == 0 and fn(8, 72, 0, 8) == 0 and fn(8, 72, 73, 0) == 0
    assert fn(65536, 65536, 256, 65536) == 8 * 65536 * 65536 * 256 * 65537
