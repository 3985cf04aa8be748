"""``rnampnn_design_distinct`` (csrc/design_distinct.hip) on the device, against the float64 restatement of its contract in
tests/_design_distinct_ref.py.

The batch is the one ``_design_distinct_ref`` describes next to ``CASE_LENGTHS`` (lengths 1, 2, 7, 33, 64, 300; T = 300, logits 2 * randn, a
seed above 2^32): fixed and empty masks, nested pairs, a pseudoknot, a pair with incompatible fixed ends, a malformed partner table and a
hairpin whose ends lie in different 256-strides.  It runs at S = 1, 8 and 256, at temperatures 1.0 and 0.3, with and without noise, in both
layouts (``CASE_RUNS``).

Device and restatement differ by last-bit exp / log / log1p (about 1e-14 relative on a key), so an RNA of a run whose margin - the smallest
relative gap between two keys that a selection ordered - is below 1e-9 is left out of the equality check; tests/test_design_distinct_cpu.py
bounds the share of such (run, RNA) pairs by 2 % for the restatement alone, and the same bound is asserted here."""
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

import _design_distinct_ref as D  # noqa: E402
from _design_ref import PAIRS  # noqa: E402
from _design_case import SMALL, raw_design, _bytes, _dev, _specs, _write_data, _checkpoint  # noqa: E402

LENGTHS, T, SEED = D.CASE_LENGTHS, D.CASE_T, D.CASE_SEED
OUTPUTS = ("seqs", "seq_nll", "infeasible", "logp", "n_distinct")


def design_distinct(logits, seed=SEED, noise=1, **kw):
    """The C entry on device tensors (numpy arrays are uploaded) -> dict of its five outputs."""
    return raw_design("rnampnn_design_distinct", (int(noise),), (("logp", torch.float32, True), ("n_distinct", torch.int32, False)), logits,
                      seed=seed, **kw)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = D.case_arrays()
    d = dict(h=h, run={})
    for k in ("logits", "mask", "allowed", "partner", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _run(case, S, temperature, noise, layout="padded"):
    """The batch through the kernel, once per (S, temperature, noise, layout); the outputs as numpy arrays, never written to."""
    key = (S, float(temperature), int(noise), layout)
    if key not in case["run"]:
        kw = dict(temperature=temperature, S=S, noise=noise, allowed=case["allowed"], partner=case["partner"])
        out = (design_distinct(case["logits"], mask=case["mask"], **kw) if layout == "padded"
               else design_distinct(case["packed"], cu=case["cu"], T=T, **kw))
        case["run"][key] = {k: v.cpu().numpy() for k, v in out.items()}
    return case["run"][key]


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("S, temperature, noise", D.CASE_RUNS)
def test_slots_equal_the_float64_restatement_in_both_layouts(case, S, temperature, noise):
    """seqs, n_distinct and infeasible equal the restatement on every RNA whose margin is at least 1e-9; logp agrees within 1e-5 relative
    (the f32 rounding of an fp64 sum, 6e-8, with room for libm differences)."""
    seqs, logp, nd, bad, margin = D.case_ref(S, temperature, noise)
    for layout in ("padded", "packed"):
        got = _run(case, S, temperature, noise, layout)
        assert np.array_equal(got["infeasible"], bad) and np.array_equal(got["n_distinct"], nd)
        for b in range(len(LENGTHS)):
            if margin[b] < D.MARGIN:
                continue
            assert np.array_equal(got["seqs"][:, b], seqs[:, b]), (layout, b)
            k = int(nd[b])
            err = np.abs(got["logp"][:k, b].astype(np.float64) - logp[:k, b])
            print(f"{layout} RNA {b}: margin {margin[b]:.2e}, largest |logp - restatement| / |restatement| "
                  f"{float(np.max(err / np.maximum(np.abs(logp[:k, b]), 1e-300))):.2e}")
            assert np.all(err <= 1e-5 * np.abs(logp[:k, b])), (layout, b)


def test_at_most_2_percent_of_the_batch_is_below_the_margin():
    margins = np.concatenate([D.case_ref(*run)[4] for run in D.CASE_RUNS])
    assert (margins < D.MARGIN).sum() <= 0.02 * margins.size


@pytest.mark.parametrize("temperature", [1.0, 0.3])
@pytest.mark.parametrize("noise", [1, 0])
def test_filled_slots_are_distinct_and_honour_the_constraints_and_empty_slots_are_empty(case, temperature, noise):
    h, got = case["h"], _run(case, 256, temperature, noise)
    assert got["n_distinct"].tolist() == [4, 1, 256, 256, 256, 256]
    for b, n in enumerate(LENGTHS):
        k = int(got["n_distinct"][b])
        rows = got["seqs"][:k, b]
        assert (rows[:, :n] >= 0).all() and (rows[:, :n] <= 3).all() and (rows[:, n:] == -1).all()
        assert len({r.tobytes() for r in rows}) == k, b
        assert (got["seqs"][k:, b] == -1).all() and np.isposinf(got["seq_nll"][k:, b]).all() and np.isneginf(got["logp"][k:, b]).all()
        assert np.isfinite(got["seq_nll"][:k, b]).all() and (got["logp"][:k, b] <= 0).all()
        if b == 1:
            continue                                               # the infeasible pair: both ends fixed to A, drawn as single positions
        mask = np.where(h["allowed"][b, :n] & 15, h["allowed"][b, :n] & 15, 15)
        assert ((mask[None, :] >> rows[:, :n]) & 1).all(), b
        for bb, i, j in D.CASE_PAIRS:
            if bb == b:
                assert all((int(r[i]), int(r[j])) in PAIRS[True] for r in rows), (b, i, j)
    if noise == 0:                                                 # the S best, in descending order
        for b in range(len(LENGTHS)):
            k = int(got["n_distinct"][b])
            assert (np.diff(got["logp"][:k, b].astype(np.float64)) <= 0).all(), b


@pytest.mark.parametrize("S, temperature, noise", [(256, 1.0, 1), (8, 0.3, 0), (256, 0.3, 0)])
def test_seq_nll_is_rnampnn_scores_byte_for_byte(case, S, temperature, noise):
    from rnampnn.model.decode import score_logits
    got = _run(case, S, temperature, noise)
    seqs = torch.from_numpy(got["seqs"]).cuda()
    for kw in (dict(logits=case["logits"], mask=case["mask"]), dict(logits=case["packed"], cu_seqlens=case["cu"])):
        want = score_logits(seqs=seqs, want=("seq_nll",), **kw)["seq_nll"].cpu().numpy()
        filled = np.arange(S)[:, None] < got["n_distinct"][None, :]
        assert got["seq_nll"][filled].tobytes() == want[filled].tobytes()


@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_best_equals_brute_force_on_the_devices_own_logits(case, temperature):
    h, got = case["h"], _run(case, 256, temperature, 0)
    for b in (0, 1, 2):
        n = LENGTHS[b]
        z = h["logits"][b, :n].astype(np.float64) / float(np.float32(temperature))
        want = D.brute_force(z, h["allowed"][b, :n], h["partner"][b, :n], True)
        k = min(256, len(want))
        assert int(got["n_distinct"][b]) == k
        assert [tuple(int(v) for v in r[:n]) for r in got["seqs"][:k, b]] == [s for s, _ in want[:k]], b
        ref = np.array([w for _, w in want[:k]])
        assert np.all(np.abs(got["logp"][:k, b] - ref) <= 1e-5 * np.abs(ref)), b


def test_best_slot_0_without_constraints_is_rnampnn_scores_pred(case):
    from rnampnn.model.decode import score_logits
    got = design_distinct(case["logits"], mask=case["mask"], temperature=0.7, S=3, noise=0)
    pred = score_logits(case["logits"], mask=case["mask"], want=("pred",))["pred"]
    assert _bytes(got["seqs"][0]) == _bytes(pred)
    assert got["infeasible"].tolist() == [0] * len(LENGTHS) and got["n_distinct"].tolist() == [3] * len(LENGTHS)


@pytest.mark.parametrize("temperature", [1.0, 0.3])
@pytest.mark.parametrize("noise", [1, 0])
def test_the_first_slots_of_a_wide_beam_are_the_narrow_beam(case, temperature, noise):
    wide = _run(case, 256, temperature, noise)
    for S in (8, 1):
        narrow = _run(case, S, temperature, noise)
        assert np.array_equal(narrow["n_distinct"], np.minimum(wide["n_distinct"], S))
        for k in ("seqs", "seq_nll", "logp"):
            assert narrow[k].tobytes() == np.ascontiguousarray(wide[k][:S]).tobytes(), (S, k)


@pytest.mark.parametrize("noise", [1, 0])
def test_padding_batch_layout_junk_and_a_second_call_do_not_change_the_bytes(case, noise):
    h, S, temp = case["h"], 8, 0.3
    base = _run(case, S, temp, noise)
    assert _same(base, _run(case, S, temp, noise, "packed"))                                   # layout
    kw = dict(temperature=temp, S=S, noise=noise)
    again = design_distinct(case["logits"], mask=case["mask"], allowed=case["allowed"], partner=case["partner"], **kw)
    assert _same(base, {k: v.cpu().numpy() for k, v in again.items()})                        # a second call
    # a wider padding, junk (NaN logits, wild masks and partners) beyond n_b, and two more RNAs behind the batch
    B, T2 = len(LENGTHS) + 2, T + 23
    rng = np.random.RandomState(1)
    logits = np.full((B, T2, 4), np.nan, dtype=np.float32)
    mask = np.zeros((B, T2), dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B, T2)).astype(np.uint8)
    partner = rng.randint(-5, T2 + 5, size=(B, T2)).astype(np.int32)
    for b, n in enumerate(LENGTHS):
        logits[b, :n], mask[b, :n] = h["logits"][b, :n], 1
        allowed[b, :n], partner[b, :n] = h["allowed"][b, :n], h["partner"][b, :n]
    logits[len(LENGTHS):, :40], mask[len(LENGTHS):, :40] = rng.standard_normal((2, 40, 4)), 1
    partner[len(LENGTHS):] = -1
    got = {k: v.cpu().numpy() for k, v in design_distinct(logits, mask=mask, allowed=allowed, partner=partner, **kw).items()}
    nb = len(LENGTHS)
    assert np.array_equal(got["seqs"][:, :nb, :T], base["seqs"]) and (got["seqs"][:, :nb, T:] == -1).all()
    for k in ("seq_nll", "logp"):
        assert np.ascontiguousarray(got[k][:, :nb]).tobytes() == base[k].tobytes(), k
    for k in ("infeasible", "n_distinct"):
        assert np.array_equal(got[k][:nb], base[k]), k


def test_nan_and_inf_logits_still_give_ids_and_an_in_range_count(case):
    h = case["h"]
    logits = h["logits"].copy()
    rng = np.random.RandomState(4)
    for b, n in enumerate(LENGTHS):
        for t in rng.choice(n, size=max(1, n // 5), replace=False):
            logits[b, t, rng.randint(4)] = rng.choice([np.nan, np.inf, -np.inf])
    logits[3, 7], logits[4, 3] = np.nan, -np.inf
    for noise in (1, 0):
        got = design_distinct(logits, mask=case["mask"], temperature=0.5, S=16, noise=noise, allowed=case["allowed"], partner=case["partner"])
        seqs, nd = got["seqs"].cpu().numpy(), got["n_distinct"].cpu().numpy()
        assert ((nd >= 1) & (nd <= 16)).all() and got["infeasible"].cpu().tolist() == D.CASE_INFEASIBLE
        for b, n in enumerate(LENGTHS):
            assert (seqs[:nd[b], b, :n] >= 0).all() and (seqs[:nd[b], b, :n] <= 3).all() and (seqs[nd[b]:, b] == -1).all()
            assert (seqs[:, b, n:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- Python surface
MODEL_LENGTHS = [33, 20, 41]


def _check_designs(out, cons, lens, S):
    seqs, nll, bad, logp, nd = out
    assert seqs.shape == (S, len(lens), max(lens)) and nd.tolist() == [S] * len(lens) and bad.tolist() == [0] * len(lens)
    got, allowed, partner = seqs.cpu().numpy(), cons.allowed.cpu().numpy(), cons.partner.cpu().numpy()
    for b, n in enumerate(lens):
        assert len({r[:n].tobytes() for r in got[:, b]}) == S
        assert ((allowed[b, :n][None, :] >> got[:, b, :n]) & 1).all()
        for t in range(n):
            j = int(partner[b, t])
            if j > t:
                assert all((int(r[t]), int(r[j])) in PAIRS[True] for r in got[:, b])
    assert torch.isfinite(nll).all() and (logp <= 0).all()


def test_both_models_design_distinct_sequences():
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
    cons = DesignConstraints.from_specs(_specs(), lens, int(mask.shape[1]))
    before = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=cons)
    assert len(before) == 3                                         # None keeps today's path and today's return value
    for mode in ("sample", "best"):
        out = m.design(c, mask, n_samples=5, temperature=0.1, seed=3, constraints=cons, distinct=mode)
        assert len(out) == 5
        _check_designs(out, cons, lens, 5)
        assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    free = m.design(c, mask, n_samples=5, temperature=0.1, seed=3, distinct="best")
    assert _bytes(free[0][0]) == _bytes(m.design(c, mask, n_samples=1, temperature=1.0, distinct="best")[0][0])   # the mode, at any temperature
    after = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=cons)
    assert all(_bytes(a) == _bytes(b) for a, b in zip(before, after))
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    for mode in ("sample", "best"):
        out = r.design(X, mask, n_samples=5, temperature=0.1, seed=5, constraints=cons, lengths=MODEL_LENGTHS, distinct=mode)
        assert len(out) == 5
        _check_designs(out, cons, lens, 5)
        assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    assert len(r.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS)) == 3


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_distinct_designs(family, tmp_path):
    """--distinct adds the last column logp and makes the designs of a structure pairwise different, alone and next to the constraint
    flags; a structure that admits fewer sequences than --samples has fewer rows; the designs file written without the flag is byte for
    byte the same before and after."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    specs = dict(zip(ids, _specs()))
    _write_data(tmp_path / "data", ids, lens)
    with open(tmp_path / "cons.csv", "w") as f:
        f.write("pdb_id,fixed,structure\n")
        for rid in ids:
            f.write(f"{rid},{specs[rid][0] or ''},{specs[rid][1] or ''}\n")
    with open(tmp_path / "fixed.csv", "w") as f:                    # r0 admits 4 sequences: everything but its last nucleotide is fixed
        f.write("pdb_id,fixed,structure\n" + f"r0,{'A' * (lens[1] - 1)}.,\n")
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    sub = str(tmp_path / "submit.csv")
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", sub, "--samples", "6", "--temperature", "0.1", "--batch-size", "2"]
    quiet = dict(log=lambda *a: None)
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "before.csv")]), **quiet)
    length = dict(zip(ids, lens))
    for mode in ("sample", "best"):
        for name, flags in (("free", []), ("cons", ["--constraints", str(tmp_path / "cons.csv"), "--bias", "G=-0.25", "--omit", "", "--no-wobble"])):
            des = str(tmp_path / f"{mode}_{name}.csv")
            P.run(P.parse(common + ["--designs-out", des, "--distinct", mode] + flags), **quiet)
            d = list(csv.reader(open(des)))
            base = ["pdb_id", "sample", "seq", "nll_per_nt", "recovery"] + (["infeasible"] if flags or family == "rdesign" else [])
            assert d[0] == base + ["logp"] and len(d) == 1 + 3 * 6
            assert len({(r[0], r[2]) for r in d[1:]}) == 3 * 6
            for r in d[1:]:
                assert len(r[2]) == length[r[0]] and float(r[-1]) <= 0
            if mode == "best":
                for rid in ids:
                    lp = [float(r[-1]) for r in d[1:] if r[0] == rid]
                    assert lp == sorted(lp, reverse=True)
    des = str(tmp_path / "fixed_out.csv")
    P.run(P.parse(common + ["--designs-out", des, "--distinct", "sample", "--constraints", str(tmp_path / "fixed.csv")]), **quiet)
    d = list(csv.reader(open(des)))
    assert len(d) == 1 + 6 + 4 + 6 and sorted(r[1] for r in d[1:] if r[0] == "r0") == ["0", "1", "2", "3"]
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "after.csv")]), **quiet)
    assert open(tmp_path / "before.csv", "rb").read() == open(tmp_path / "after.csv", "rb").read()
    assert list(csv.reader(open(tmp_path / "before.csv")))[0][-1] in ("recovery", "infeasible")
    with pytest.raises(ValueError, match="--distinct.*--gc-content"):
        P.run(P.parse(common + ["--distinct", "best", "--gc-content", "0.5:0.6"]), **quiet)
