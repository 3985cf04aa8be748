"""Host side of constrained design (``rnampnn_design``): the constraint parsers, ``DesignConstraints.from_specs``, the ABI entry and its
argument errors (no launch happens, so no GPU is needed), predict.py's flags, and the statistics of the float64 reference sampler the GPU
tests compare against."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    return _native


# ---------------------------------------------------------------------------------------------------------------- parsers
def test_dot_bracket_nested_and_pseudoknotted():
    from rnampnn.utils.constraints import parse_dot_bracket
    p = parse_dot_bracket("((..)).")
    assert p.dtype == np.int32 and p.tolist() == [5, 4, -1, -1, 1, 0, -1]
    # an H-type pseudoknot: the square brackets cross the round ones and nest on their own level
    p = parse_dot_bracket("(([[.))]]")
    assert p.tolist() == [6, 5, 8, 7, -1, 1, 0, 3, 2]
    p = parse_dot_bracket("({<[.)}>]")
    assert p.tolist() == [5, 6, 7, 8, -1, 0, 1, 2, 3]
    assert parse_dot_bracket("").tolist() == [] and parse_dot_bracket("...").tolist() == [-1, -1, -1]
    assert all(p[p[i]] == i for i in range(len(p)) if p[i] >= 0)


@pytest.mark.parametrize("text", ["(", ")", "(()", "())", "([)", "(]", "<<>", "{"])
def test_dot_bracket_unbalanced_raises(text):
    from rnampnn.utils.constraints import parse_dot_bracket
    with pytest.raises(ValueError, match="dot-bracket"):
        parse_dot_bracket(text)


@pytest.mark.parametrize("text", ["(.x.)", "..A", "(|)", " ()"])
def test_dot_bracket_unknown_character_raises(text):
    from rnampnn.utils.constraints import parse_dot_bracket
    with pytest.raises(ValueError, match="unknown character"):
        parse_dot_bracket(text)


def test_pattern_every_iupac_code_and_t():
    from rnampnn.config.glob import VOCAB
    from rnampnn.utils.constraints import parse_pattern
    sets = dict(A="A", U="U", C="C", G="G", T="U", R="AG", Y="CU", S="CG", W="AU", K="GU", M="AC", B="CGU", D="AGU", H="ACU", V="ACG",
                N="ACGU")
    sets.update({".": "ACGU", "-": "ACGU"})
    for code, letters in sets.items():
        want = sum(1 << VOCAB[ch] for ch in letters)
        for text in (code, code.lower()):
            got = parse_pattern(text)
            assert got.dtype == np.uint8 and got.tolist() == [want], code
    assert parse_pattern("gNRa.t-").tolist() == [8, 15, 9, 1, 15, 2, 15]
    for bad in ("AXG", "A G", "A*"):
        with pytest.raises(ValueError, match="unknown character"):
            parse_pattern(bad)


def test_from_specs_checks_lengths_and_pads():
    from rnampnn.utils.constraints import DesignConstraints
    specs = [("GNRA", "(..)"), (None, "([)]."), ("uu", None), (None, None)]
    c = DesignConstraints.from_specs(specs, [4, 5, 2, 3], 6)
    assert c.allowed.dtype == torch.uint8 and c.partner.dtype == torch.int32 and c.bias is None and c.wobble is True
    assert c.allowed.device.type == "cpu" and c.partner.device.type == "cpu"
    assert c.allowed.tolist() == [[8, 15, 9, 1, 15, 15], [15] * 6, [2, 2, 15, 15, 15, 15], [15] * 6]
    assert c.partner.tolist() == [[3, -1, -1, 0, -1, -1], [2, 3, 0, 1, -1, -1], [-1] * 6, [-1] * 6]
    for bad in ([("GNR", None)], [(None, "(.)")], [("GNRAA", "(..)")]):
        with pytest.raises(ValueError, match="length"):
            DesignConstraints.from_specs(bad, [4], 6)
    with pytest.raises(ValueError):
        DesignConstraints.from_specs([("A", None)], [7], 6)          # an RNA longer than the padded extent
    # nothing given: no tensors at all (the call passes null pointers); a global bias and an omitted letter
    c = DesignConstraints.from_specs([(None, None)], [3], 4, bias=[0, 0, 0, -1.5], wobble=False, omit="g")
    assert c.partner is None and c.allowed.tolist() == [[7, 7, 7, 7]] and c.bias.tolist() == [0, 0, 0, -1.5] and c.wobble is False
    assert DesignConstraints.from_specs([(None, None)], [3], 4).allowed is None


def test_constraints_csv_and_batch_errors_name_the_id(tmp_path):
    from rnampnn.utils.constraints import batch_constraints, parse_bias, read_constraints_csv
    path = tmp_path / "c.csv"
    path.write_text("pdb_id,fixed,structure\nr1,GNRA,(..)\nr2,,((.))\nr3,AU,\n")
    table = read_constraints_csv(str(path))
    assert table == {"r1": ("GNRA", "(..)"), "r2": ("", "((.))"), "r3": ("AU", "")}
    c = batch_constraints(table, ["r2", "zz", "r1"], [5, 3, 4], 5)
    assert c.partner.tolist() == [[4, 3, -1, 1, 0], [-1] * 5, [3, -1, -1, 0, -1]]
    assert c.allowed.tolist() == [[15] * 5, [15] * 5, [8, 15, 9, 1, 15]]
    with pytest.raises(ValueError, match="r2"):
        batch_constraints(table, ["r2"], [6], 6)
    with pytest.raises(ValueError, match="r3"):
        batch_constraints({"r3": ("AX", "")}, ["r3"], [2], 2)
    (tmp_path / "bad.csv").write_text("pdb_id,structure\nr1,()\n")
    with pytest.raises(ValueError, match="fixed"):
        read_constraints_csv(str(tmp_path / "bad.csv"))
    assert parse_bias("G=-0.5, u=1,T=2").tolist() == [0.0, 2.0, 0.0, -0.5]
    with pytest.raises(ValueError):
        parse_bias("X=1")


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_rnampnn_design(native):
    text = open(os.path.join(REPO, "include", "rnampnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+rnampnn_design\s*\(([^;]*)\)\s*;", text)
    assert m, "include/rnampnn_hip.h does not declare rnampnn_design"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert "rnampnn_design" in native.SYMBOLS and len(native.SYMBOLS["rnampnn_design"][1]) == n_params == 19
    assert hasattr(native.lib(), "rnampnn_design")
    import __graft_entry__ as g
    assert "design.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design.hip"))


def _call(native, **kw):
    """rnampnn_design with made-up (never dereferenced) addresses: every case below must return before a launch."""
    a = dict(logits=0x1000, n_rows=64, mask=0x2000, cu=None, B=2, T=8, temperature=1.0, S=4, seed=1, seed_dev=None, allowed=None, partner=None,
             wobble=1, bias=None, per_position=0, seqs=0x3000, seq_nll=0x4000, infeasible=0x5000)
    a.update(kw)
    vp = lambda v: None if v is None else C.c_void_p(v)
    return native.lib().rnampnn_design(vp(a["logits"]), a["n_rows"], vp(a["mask"]), vp(a["cu"]), a["B"], a["T"], a["temperature"], a["S"],
                                       C.c_uint64(a["seed"]), vp(a["seed_dev"]), vp(a["allowed"]), vp(a["partner"]), a["wobble"],
                                       vp(a["bias"]), a["per_position"], vp(a["seqs"]), vp(a["seq_nll"]), vp(a["infeasible"]), None)


@pytest.mark.parametrize("kw, text", [
    (dict(logits=None), "null logits"),
    (dict(B=0), "empty batch"), (dict(B=-3), "empty batch"), (dict(T=0), "empty batch"),
    (dict(S=0), "S = 0"), (dict(S=-1), "S = -1"),
    (dict(S=65535), "at most 65534"),
    (dict(mask=None, cu=None), "exactly one of mask"), (dict(cu=0x6000), "exactly one of mask"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("inf")), "temperature"), (dict(temperature=float("nan")), "temperature"),
    (dict(logits=0x1004), "16-byte aligned"),
])
def test_argument_errors_are_value_errors_before_any_launch(native, kw, text):
    rc = _call(native, **kw)
    assert rc == native.ERR_BAD_ARG
    with pytest.raises(ValueError, match=text):
        native.check(rc)


def test_a_call_with_every_output_null_returns_ok_without_a_launch(native):
    assert _call(native, seqs=None, seq_nll=None, infeasible=None) == 0
    assert _call(native, S=65534, seqs=None, seq_nll=None, infeasible=None) == 0


def test_design_refuses_host_logits(native):
    from rnampnn.model.rnampnn import design_from_logits
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        design_from_logits(torch.zeros(1, 4, 4), mask=torch.ones(1, 4), n_samples=1, temperature=1.0, seed=0)


def test_predict_parses_the_constraint_flags(tmp_path):
    import predict
    p = predict.parse(["--ckpt", "x.pt", "--data", "d"])
    assert (p.constraints, p.bias, p.omit, p.no_wobble) == (None, None, "", False) and predict.design_options(p) == {}
    csv = tmp_path / "c.csv"
    csv.write_text("pdb_id,fixed,structure\nr1,GNRA,(..)\n")
    p = predict.parse(["--ckpt", "x.pt", "--data", "d", "--samples", "2", "--constraints", str(csv), "--bias", "A=0.5,G=-1", "--omit", "U",
                       "--no-wobble"])
    assert (p.constraints, p.bias, p.omit, p.no_wobble) == (str(csv), "A=0.5,G=-1", "U", True)
    o = predict.design_options(p)
    assert o["constraints"] == {"r1": ("GNRA", "(..)")} and o["bias"].tolist() == [0.5, 0.0, 0.0, -1.0] and o["omit"] == "U" and o["wobble"] is False
    o = predict.design_options(predict.parse(["--ckpt", "x.pt", "--data", "d", "--omit", "G"]))
    assert o["constraints"] is None and o["bias"] is None and o["wobble"] is True
    with pytest.raises(ValueError, match="omit"):
        predict.design_options(predict.parse(["--ckpt", "x.pt", "--data", "d", "--omit", "X"]))


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_mix64_is_the_splitmix64_finaliser():
    # the published splitmix64 stream from state 0: output k = mix64((k + 1) * golden)
    golden = 0x9E3779B97F4A7C15
    assert [R.mix64(golden * (k + 1)) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert R.u24(7, 0, 0, 0) == R.u24(7, 0, 0, 0) < (1 << 24) and len({R.u24(7, s, b, t) for s in range(3) for b in range(3) for t in range(3)}) == 27


def test_reference_pair_frequencies_follow_the_analytic_joint():
    """One 2-nt RNA that is one pair, 20,000 samples: every compatible cell within 5 binomial standard deviations of
    softmax(z_0(a) + z_1(b)) over the 6 compatible cells, every other cell never drawn."""
    S = 20000
    logits = np.array([[[0.3, -0.4, 1.1, 0.2], [-0.7, 0.9, 0.1, 0.5]]], dtype=np.float32)
    partner = np.array([[1, 0]], dtype=np.int32)
    seqs, margin, bad, _ = R.design_ref(logits, [2], 0.8, S, 1234, partner=partner, wobble=True)
    assert bad.tolist() == [0] and seqs.shape == (S, 1, 2) and np.isfinite(margin).all()
    temp = float(np.float32(0.8))
    joint = {(a, b): np.exp((float(logits[0, 0, a]) + float(logits[0, 1, b])) / temp) for (a, b) in R.PAIRS[True]}
    tot = sum(joint.values())
    assert len(joint) == 6
    counts = np.zeros((4, 4), dtype=np.int64)
    np.add.at(counts, (seqs[:, 0, 0].astype(np.int64), seqs[:, 0, 1].astype(np.int64)), 1)
    for a in range(4):
        for b in range(4):
            if (a, b) in joint:
                p = joint[(a, b)] / tot
                sd = np.sqrt(p * (1 - p) / S)
                print(f"cell {'AUCG'[a]}{'AUCG'[b]}: frequency {counts[a, b] / S:.5f} analytic {p:.5f} ({abs(counts[a, b] / S - p) / sd:.2f} sd)")
                assert abs(counts[a, b] / S - p) <= 5 * sd, (a, b)
            else:
                assert counts[a, b] == 0, (a, b)
    # without wobble GU / UG are gone too
    seqs4, _, _, _ = R.design_ref(logits, [2], 0.8, 2000, 99, partner=partner, wobble=False)
    assert {(int(a), int(b)) for a, b in seqs4[:, 0, :]} <= R.PAIRS[False] and len(R.PAIRS[False]) == 4
