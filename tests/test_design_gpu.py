"""``rnampnn_design`` (csrc/design.hip) on the device, against the float64 restatement of its contract in tests/_design_ref.py.

One padded batch, lengths ``LENGTHS`` (RNA b has LENGTHS[b] nucleotides; T = 300), logits 3 * randn, S = 4.  The constraints, by (RNA, position):

  pairs        (1; 0,1)      the whole length-2 RNA
               (2; 0,62)     first and last nucleotide of the 63-mer
               (5; 0,256)    partners in different 256-strides
               (6; 3,259)    partners in different 256-strides
               (6; 62,64)    partners in different waves; 62 is IUPAC R
               (6; 10,40) and (6; 20,50)   crossing (pseudoknot); 10 is fixed to G: a fixed nucleotide on one side of a pair
               (5; 50,60)    50 has allowed = 0: drawn as free inside the pair, counts 1
               (6; 100,110)  both fixed to A: two incompatible fixed nucleotides, both draw on their own, counts 2
  allowed      (3; 0..3) = G N R A; (5; 100) = R; (2; 5) = 0xF2 (bits above 3 are ignored: U); (6; 150) = 0: drawn as free, counts 1
  malformed    (4; 5) -> 70, in the padding of the 65-mer, whose entry points back at 5;  (4; 6) -> 100000;  (4; 7) -> -5
  partner      (5; 9) -> 9, a self-partner;  (5; 20) -> 30 while 30 -> -1, and (5; 40) -> 50 while 50 -> 60: asymmetric entries
  bias         variant "global": four floats; variant "perpos": (B,T,4), drawn with wobble = 0; variant "plain": none

so ``infeasible`` is [0, 0, 0, 0, 0, 1, 3, 0] in every variant."""
import csv
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

import _design_ref as R  # noqa: E402
from _design_case import SMALL, _bytes, _specs, _write_data, _checkpoint  # noqa: E402

LENGTHS = [1, 2, 63, 64, 65, 257, 300, 0]
T = 300
S = 4
SEED = 0x1234_5678_9ABC_DEF1                                       # above 2^32: the 64-bit seed arithmetic is exercised
PAIRS = [(1, 0, 1), (2, 0, 62), (5, 0, 256), (6, 3, 259), (6, 62, 64), (6, 10, 40), (6, 20, 50), (5, 50, 60), (6, 100, 110)]
FEASIBLE = PAIRS[:-1]
INFEASIBLE = [0, 0, 0, 0, 0, 1, 3, 0]
VARIANTS = {"plain": dict(bias=None, wobble=True), "global": dict(bias="global", wobble=True), "perpos": dict(bias="perpos", wobble=False)}
NEAR = 1e-5                                                        # draws this close to a cumulative boundary (relative) are not compared


def _nll_bound(sum64, n):
    """tests/test_rnampnn_score_gpu.py: _nll_bound."""
    return 1e-5 * abs(sum64) + 1e-6 * n


def host_case():
    """The batch on the host (numpy): logits, mask, allowed, partner, the two biases, the packed layout."""
    B = len(LENGTHS)
    gen = torch.Generator().manual_seed(41)
    logits = 3.0 * torch.randn(B, T, 4, generator=gen)
    mask = torch.zeros(B, T)
    for b, n in enumerate(LENGTHS):
        mask[b, :n] = 1
    logits = logits * mask[..., None]
    allowed = np.full((B, T), 15, dtype=np.uint8)
    partner = np.full((B, T), -1, dtype=np.int32)
    for b, i, j in PAIRS:
        partner[b, i], partner[b, j] = j, i
    allowed[6, 62] = 9; allowed[6, 10] = 8; allowed[5, 50] = 0; allowed[6, 100] = 1; allowed[6, 110] = 1
    allowed[3, 0:4] = [8, 15, 9, 1]; allowed[5, 100] = 9; allowed[2, 5] = 0xF2; allowed[6, 150] = 0
    partner[4, 5] = 70; partner[4, 70] = 5; partner[4, 6] = 100000; partner[4, 7] = -5
    partner[5, 9] = 9; partner[5, 20] = 30; partner[5, 40] = 50
    d = dict(B=B, logits=logits.numpy(), mask=mask.numpy(), allowed=allowed, partner=partner)
    d["global"] = np.array([0.5, -1.0, 0.25, -0.5], dtype=np.float32)
    d["perpos"] = (0.5 * torch.randn(B, T, 4, generator=gen)).numpy()
    d["packed"] = np.ascontiguousarray(d["logits"][d["mask"] != 0])
    d["cu"] = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    return d


def cold_argmax(h):
    """Per feasible pair: (the argmax cell of logit_i(a) + logit_j(b) over the compatible cells both masks admit, its lead over the runner-up),
    in float64, with wobble."""
    out = {}
    for b, i, j in FEASIBLE:
        mi, mj = int(h["allowed"][b, i]) & 15 or 15, int(h["allowed"][b, j]) & 15 or 15
        cells = sorted(((float(h["logits"][b, i, a]) + float(h["logits"][b, j, c]), (a, c)) for (a, c) in R.PAIRS[True]
                        if (mi >> a) & 1 and (mj >> c) & 1), reverse=True)
        out[(b, i, j)] = (cells[0][1], cells[0][0] - cells[1][0] if len(cells) > 1 else np.inf)
    return out


@pytest.fixture(scope="module")
def case():
    """Inputs on the device + the float64 references, computed once and never written to."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.constraints import DesignConstraints
    h = host_case()
    d = dict(h=h, B=h["B"])
    for k in ("logits", "mask", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    d["cons"] = {}
    for name, v in VARIANTS.items():
        bias = None if v["bias"] is None else torch.from_numpy(h[v["bias"]])
        d["cons"][name] = DesignConstraints(torch.from_numpy(h["allowed"]), torch.from_numpy(h["partner"]), bias, v["wobble"]).to_device("cuda")
    d["ref"] = {}
    return d


def _ref(case, variant, temperature, n=S, seed=SEED):
    key = (variant, temperature, n, seed)
    if key not in case["ref"]:
        h, v = case["h"], VARIANTS[variant]
        case["ref"][key] = R.design_ref(h["logits"], LENGTHS, temperature, n, seed, h["allowed"], h["partner"], v["wobble"],
                                        None if v["bias"] is None else h[v["bias"]])
    return case["ref"][key]


def _design(case, variant="global", temperature=1.0, n=S, seed=SEED, layout="padded"):
    from rnampnn.model.rnampnn import design_from_logits
    kw = dict(n_samples=n, temperature=temperature, seed=seed, constraints=case["cons"][variant])
    if layout == "padded":
        return design_from_logits(case["logits"], mask=case["mask"], **kw)
    return design_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_reference(case, variant, temperature):
    want, margin, bad, _ = _ref(case, variant, temperature)
    valid = case["h"]["mask"][None].repeat(S, 0) != 0
    near = valid & ~(margin > NEAR)                                 # the reference's own count: it does not depend on the kernel
    share = near.sum() / valid.sum()
    print(f"{variant} temperature {temperature}: {int(near.sum())} of {int(valid.sum())} draws within {NEAR} of a boundary ({share:.4%})")
    assert share <= 0.01
    seqs, _, infeasible = _design(case, variant, temperature)
    got = seqs.cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (S, case["B"], T)
    differ = (got != want) & valid & ~near
    print(f"{variant} temperature {temperature}: {int(differ.sum())} draws differ from the reference; "
          f"{int(((got != want) & near).sum())} of the left-out ones differ")
    assert not differ.any(), np.argwhere(differ)[:10].tolist()
    assert (got[~valid] == -1).all() and infeasible.tolist() == bad.tolist() == INFEASIBLE


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_constraints_hold_in_every_draw(case, variant):
    seqs, _, infeasible = _design(case, variant, 1.0)
    got = seqs.cpu().numpy()
    h, wobble = case["h"], VARIANTS[variant]["wobble"]
    _, _, bad, plan = _ref(case, variant, 1.0)
    assert infeasible.dtype == torch.int32 and infeasible.tolist() == bad.tolist() == INFEASIBLE
    for b, n in enumerate(LENGTHS):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
    for s in range(S):
        assert got[s, 3, 0] == 3 and got[s, 3, 3] == 0 and got[s, 3, 2] in (0, 3)          # G N R A
        assert got[s, 5, 100] in (0, 3) and got[s, 6, 62] in (0, 3) and got[s, 2, 5] == 1  # R, R on a pair, bits above 3 ignored
        assert got[s, 6, 10] == 3 and got[s, 6, 40] in ((1, 2) if wobble else (2,))       # G fixed: its partner is U or C
        assert got[s, 6, 100] == 0 and got[s, 6, 110] == 0                                 # the infeasible pair keeps both fixed letters
        for b, i, j in FEASIBLE:
            assert (int(got[s, b, i]), int(got[s, b, j])) in R.PAIRS[wobble], (s, b, i, j)
    assert len(R.PAIRS[True]) == 6 and len(R.PAIRS[False]) == 4
    # the well-formed pairs are exactly the listed ones: the malformed entries pair nothing
    assert sorted((b, t, int(plan.mate[b, t])) for b in range(case["B"]) for t in range(T) if plan.mate[b, t] > t) == sorted(PAIRS)


def test_nan_logits_and_nan_bias_still_give_ids(case):
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    logits = case["logits"].clone()
    logits[6, 3] = float("nan"); logits[6, 64, 1] = float("nan"); logits[5, 7] = float("inf"); logits[2, 9] = -float("inf")
    bias = torch.zeros(case["B"], T, 4, device="cuda")
    bias[6, 200] = float("nan"); bias[3, 1, 2] = float("nan")
    c = case["cons"]["plain"]
    seqs, nll, bad = design_from_logits(logits, mask=case["mask"], n_samples=S, temperature=1.0, seed=SEED,
                                        constraints=DesignConstraints(c.allowed, c.partner, bias, True))
    got = seqs.cpu().numpy()
    for b, n in enumerate(LENGTHS):
        assert ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all() and (got[:, b, n:] == -1).all()
    assert bad.tolist() == INFEASIBLE and (got[:, 6, 10] == 3).all() and (got[:, 3, 0] == 3).all()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_cold_limit_is_the_constrained_argmax(case):
    best = cold_argmax(case["h"])
    lead = min(v[1] for v in best.values())
    print("smallest lead of a pair's best cell over its runner-up:", lead)
    assert lead >= 0.05                                            # 50 temperatures: the runner-up is drawn with probability e^-50
    seqs, _, infeasible = _design(case, "plain", 1e-3)
    got = seqs.cpu().numpy()
    for (b, i, j), (cell, _) in best.items():
        for s in range(S):
            assert (int(got[s, b, i]), int(got[s, b, j])) == cell, (s, b, i, j)
    assert infeasible.tolist() == INFEASIBLE                       # no feasible pair underflowed into the infeasible branch
    assert infeasible.tolist() == _ref(case, "plain", 1e-3)[2].tolist()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("variant, temperature", [("global", 1.0), ("perpos", 0.3)])
def test_seq_nll_is_rnampnn_scores_byte_for_byte(case, variant, temperature):
    from rnampnn.model.rnampnn import score_logits
    seqs, nll, _ = _design(case, variant, temperature)
    assert nll.dtype == torch.float32 and nll.shape == (S, case["B"])
    assert _bytes(nll) == _bytes(score_logits(case["logits"], mask=case["mask"], seqs=seqs, want=("seq_nll",))["seq_nll"])
    assert _bytes(nll) == _bytes(score_logits(case["packed"], cu_seqlens=case["cu"], seqs=seqs, want=("seq_nll",))["seq_nll"])
    x = torch.from_numpy(case["h"]["logits"]).double()
    m = torch.from_numpy(case["h"]["mask"]).double()
    lse = torch.logsumexp(x, dim=-1)
    ids = seqs.cpu().long().clamp(min=0)
    for s in range(S):
        ref = ((lse - torch.gather(x, 2, ids[s][..., None])[..., 0]) * m).sum(1)
        for b, n in enumerate(LENGTHS):
            got, want = float(nll[s, b]), float(ref[b])
            print(f"sample {s} RNA {b} n {n}: {got:.6f} f64 {want:.6f} |d| {abs(got - want):.3e} bound {_nll_bound(want, n):.3e}")
            assert abs(got - want) <= _nll_bound(want, n), (s, b)
    assert float(nll[:, LENGTHS.index(0)].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("variant", ["global", "perpos"])
def test_layout_padding_and_batch_independence(case, variant):
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    a, b, p = _design(case, variant), _design(case, variant), _design(case, variant, layout="packed")
    for x, y, z in zip(a, b, p):
        assert _bytes(x) == _bytes(y) and _bytes(x) == _bytes(z)
    # T = 320, garbage beyond every length: NaN logits, random allowed / partner / bias entries
    T2, B = 320, case["B"]
    gen = torch.Generator().manual_seed(7)
    c = case["cons"][variant]
    inside = torch.zeros(B, T2, dtype=torch.bool)
    for r, n in enumerate(LENGTHS):
        inside[r, :n] = True
    inside = inside.cuda()

    def grow(t, junk):
        big = junk.to(t.dtype).cuda()
        big[:, :T] = torch.where(inside[:, :T].view(B, T, *([1] * (t.dim() - 2))), t, big[:, :T])
        return big
    logits = grow(case["logits"], torch.full((B, T2, 4), float("nan")))
    allowed = grow(c.allowed, torch.randint(0, 256, (B, T2), generator=gen))
    partner = grow(c.partner, torch.randint(-5, 400, (B, T2), generator=gen))
    bias = c.bias if c.bias.dim() == 1 else grow(c.bias, torch.full((B, T2, 4), float("nan")))
    big = design_from_logits(logits, mask=inside.float(), n_samples=S, temperature=1.0, seed=SEED,
                             constraints=DesignConstraints(allowed, partner, bias, c.wobble))
    assert big[0].shape == (S, B, T2) and bool((big[0][:, :, T:] == -1).all())
    assert _bytes(big[0][:, :, :T].contiguous()) == _bytes(a[0]) and _bytes(big[1]) == _bytes(a[1]) and _bytes(big[2]) == _bytes(a[2])
    # another seed, and sample 0 when S goes from 1 to 4
    other = _design(case, variant, seed=SEED + 1)
    assert _bytes(other[0]) != _bytes(a[0]) and _bytes(other[2]) == _bytes(a[2])
    one = _design(case, variant, n=1)
    assert one[0].shape == (1, B, T) and _bytes(one[0][0]) == _bytes(a[0][0]) and _bytes(one[1][0]) == _bytes(a[1][0])
    # a sub-batch in another order: the draws of RNA b follow its batch index only through (s, b, t)
    sub = design_from_logits(case["logits"][:6], mask=case["mask"][:6], n_samples=S, temperature=1.0, seed=SEED,
                             constraints=DesignConstraints(c.allowed[:6], c.partner[:6], c.bias if c.bias.dim() == 1 else c.bias[:6], c.wobble))
    assert _bytes(sub[0]) == _bytes(a[0][:, :6].contiguous()) and _bytes(sub[1]) == _bytes(a[1][:, :6].contiguous())


def test_free_design_needs_no_constraint_tensors(case):
    """No constraints at all: null allowed / partner / bias; the same draws as explicit all-free tensors."""
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    B = case["B"]
    free = DesignConstraints(torch.full((B, T), 15, dtype=torch.uint8), torch.full((B, T), -1, dtype=torch.int32), torch.zeros(4), False)
    a = design_from_logits(case["logits"], mask=case["mask"], n_samples=2, temperature=0.7, seed=3)
    b = design_from_logits(case["logits"], mask=case["mask"], n_samples=2, temperature=0.7, seed=3, constraints=free)
    c = design_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, n_samples=2, temperature=0.7, seed=3)
    for x, y, z in zip(a, b, c):
        assert _bytes(x) == _bytes(y) == _bytes(z)
    assert a[2].tolist() == [0] * B
    want, margin, _, _ = R.design_ref(case["h"]["logits"], LENGTHS, 0.7, 2, 3)
    ok = margin > NEAR
    assert (a[0].cpu().numpy()[ok] == want[ok]).all()
    with pytest.raises(ValueError, match="padded to"):
        design_from_logits(case["logits"], mask=case["mask"], n_samples=1, temperature=1.0, seed=0,
                           constraints=DesignConstraints(free.allowed[:, :10], None, None, True))
    with pytest.raises(ValueError, match="temperature"):
        design_from_logits(case["logits"], mask=case["mask"], n_samples=1, temperature=0.0, seed=0)


# ---------------------------------------------------------------------------------------------------------------- 6
MODEL_LENGTHS = [33, 20, 41]
# GNRA on a 4-pair stem / a pseudoknot / one fixed last nucleotide


def _check_specs(seqs, specs, lengths, wobble=True):
    """Every drawn sequence (S,B,T) satisfies its RNA's pattern and structure."""
    from rnampnn.utils.constraints import parse_dot_bracket, parse_pattern
    got = seqs.cpu().numpy()
    for b, ((pattern, structure), n) in enumerate(zip(specs, lengths)):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
        if pattern:
            assert ((parse_pattern(pattern)[None].astype(np.int64) >> got[:, b, :n]) & 1).all(), b
        if structure:
            p = parse_dot_bracket(structure)
            for t in np.nonzero(p > np.arange(n))[0]:
                for s in range(got.shape[0]):
                    assert (int(got[s, b, t]), int(got[s, b, p[t]])) in R.PAIRS[wobble], (s, b, t)


def test_rnampnn_design_without_and_with_constraints():
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.data import pad_batch
    torch.manual_seed(0)
    m = RNAMPNN(precision="f32", **SMALL).cuda().eval()
    items = [(synth.synth_rna(n, i, seed=1), synth.synth_labels(n, i, seed=1)) for i, n in enumerate(MODEL_LENGTHS)]
    _, c, mask, lens = pad_batch(items, pin=False)
    c, mask = c.cuda(), mask.cuda()
    out = m.design(c, mask, n_samples=3, temperature=1.0, seed=3)
    assert len(out) == 2
    seqs = m.sample(c, mask, temperature=1.0, n_samples=3, seed=3)
    assert torch.equal(out[0], seqs) and _bytes(out[1]) == _bytes(m.score_sequences(c, mask, seqs)[0])
    cons = DesignConstraints.from_specs(_specs(), lens, int(mask.shape[1]))
    tri = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=cons)
    assert len(tri) == 3 and tri[0].shape == (3, 3, max(lens)) and tri[0].dtype == torch.int8 and tri[2].tolist() == [0, 0, 0]
    _check_specs(tri[0], _specs(), lens)
    assert _bytes(tri[1]) == _bytes(m.score_sequences(c, mask, tri[0])[0])


def test_rdesign_model_designs_and_scores():
    import __graft_entry__ as g
    g.build()
    from rdesign.model.rdesign import RNAModel
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    torch.manual_seed(0)
    m = RNAModel(num_mpnn_layers=1).cuda().eval()
    B, Tm = len(MODEL_LENGTHS), max(MODEL_LENGTHS)
    X, mask = torch.zeros(B, Tm, 6, 3), torch.zeros(B, Tm)
    labels = torch.zeros(B, Tm, dtype=torch.int32)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
        mask[i, :n] = 1
        labels[i, :n] = torch.from_numpy(synth.synth_labels(n, i, seed=1)).to(torch.int32)
    X, mask = X.cuda(), mask.cuda()
    cons = DesignConstraints.from_specs(_specs(), MODEL_LENGTHS, Tm, bias=[0.0, 0.0, 0.0, -0.25])
    seqs, nll, bad = m.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS)
    assert seqs.shape == (3, B, Tm) and seqs.dtype == torch.int8 and nll.shape == (3, B) and bad.tolist() == [0, 0, 0]
    _check_specs(seqs, _specs(), MODEL_LENGTHS)
    free = m.design(X, mask, n_samples=3, temperature=1.0, seed=5)
    assert len(free) == 3 and free[0].shape == (3, B, Tm) and free[2].tolist() == [0, 0, 0] and not torch.equal(free[0], seqs)
    nll2, match, valid = m.score_sequences(X, mask, seqs, labels=labels.cuda())
    assert _bytes(nll2) == _bytes(nll) and valid.tolist() == MODEL_LENGTHS and match.shape == (3, B)
    assert match.tolist() == [[int(((seqs[s, b].cpu() == labels[b]) & (mask[b].cpu() == 1)).sum()) for b in range(B)] for s in range(3)]
    nll3, none, _ = m.score_sequences(X, mask, seqs[1])
    assert none is None and _bytes(nll3[0]) == _bytes(nll[1])
    # float64 NLL on this model's own (packed) logits
    x = m.forward_logits(X, mask).double().cpu()
    lse, start = torch.logsumexp(x, dim=-1), 0
    for b, n in enumerate(MODEL_LENGTHS):
        for s in range(3):
            ids = seqs[s, b, :n].cpu().long()
            ref = float((lse[start:start + n] - x[start:start + n].gather(1, ids[:, None])[:, 0]).sum())
            assert abs(float(nll[s, b]) - ref) <= _nll_bound(ref, n), (s, b)
        start += n


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_a_constraints_file(family, tmp_path):
    import __graft_entry__ as g
    g.build()
    import predict as P
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    specs = dict(zip(ids, _specs()))
    _write_data(tmp_path / "data", ids + ["r3"], lens + [27])        # r3 is not in the constraints file: unconstrained
    with open(tmp_path / "cons.csv", "w") as f:
        f.write("pdb_id,fixed,structure\n")
        for rid in ids:
            f.write(f"{rid},{specs[rid][0] or ''},{specs[rid][1] or ''}\n")
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    sub, des = str(tmp_path / "submit.csv"), str(tmp_path / "designs.csv")
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", sub, "--samples", "3", "--temperature", "1.0", "--designs-out", des,
              "--batch-size", "2"]
    rows = P.run(P.parse(common + ["--constraints", str(tmp_path / "cons.csv"), "--bias", "G=-0.25"]), log=lambda *a: None)
    assert [r[0] for r in rows] == sorted(ids + ["r3"])
    d = list(csv.reader(open(des)))
    assert d[0] == ["pdb_id", "sample", "seq", "nll_per_nt", "recovery", "infeasible"] and len(d) == 1 + 3 * 4
    assert [(r[0], r[1]) for r in d[1:]] == [(rid, str(s)) for rid in sorted(ids + ["r3"]) for s in range(3)]
    length = dict(zip(ids + ["r3"], lens + [27]))
    for r in d[1:]:
        assert len(r[2]) == length[r[0]] and set(r[2]) <= set("AUCG") and float(r[3]) > 0 and 0.0 <= float(r[4]) <= 1.0 and r[5] == "0"
        if r[0] in specs:
            ids_ = torch.tensor([["AUCG".index(ch) for ch in r[2]]], dtype=torch.int8)[None]
            _check_specs(ids_, [specs[r[0]]], [length[r[0]]])
    # a row that does not fit its structure names the id
    with open(tmp_path / "bad.csv", "w") as f:
        f.write("pdb_id,fixed,structure\nr1,,((..))\n")
    with pytest.raises(ValueError, match="r1"):
        P.run(P.parse(common + ["--constraints", str(tmp_path / "bad.csv")]), log=lambda *a: None)


def test_predict_without_the_new_flags_writes_what_the_sampler_path_writes(tmp_path):
    """No constraint flag: the designs come from ``rnampnn_sample`` on the scattered logits and ``rnampnn_score``, as before - restated
    here from the model's own calls - and the file has no ``infeasible`` column."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    from rnampnn.model.rnampnn import letters_padded, sample_from_logits, score_logits
    from rnampnn.utils.data import PackedLoader, bucket_batches
    from rnampnn.utils.predict import load_structures
    from rnampnn.utils.train import load_checkpoint
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    ck = str(tmp_path / "model.pt")
    _checkpoint("rnampnn", ck)
    sub, des = str(tmp_path / "submit.csv"), str(tmp_path / "designs.csv")
    P.run(P.parse(["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", sub, "--samples", "2", "--temperature", "1.0", "--seed", "11",
                   "--designs-out", des, "--batch-size", "2"]), log=lambda *a: None)
    model, _ = load_checkpoint(ck, device=torch.device("cuda:0"))
    model.eval()
    items = load_structures(str(tmp_path / "data"), max_len=128)
    lengths = [int(c.shape[0]) for _, c, _ in items]
    lines, preds = {}, {}
    for bi, (coords, cu, max_len, idx) in enumerate(PackedLoader(items, bucket_batches(lengths, 2, 32768, seed=0), device=model._device())):
        logits = model.forward_packed(coords, cu, max_len)
        padded = torch.zeros(len(idx), max_len, 4, device="cuda")
        mask = torch.zeros(len(idx), max_len, device="cuda")
        lab = torch.zeros(len(idx), max_len, dtype=torch.int32)
        for r, i in enumerate(idx):
            lo = int(cu[r])
            padded[r, :lengths[i]] = logits[lo:lo + lengths[i]]
            mask[r, :lengths[i]] = 1
            lab[r, :lengths[i]] = torch.from_numpy(items[i][2]).to(torch.int32)
        draws = sample_from_logits(padded, mask, 1.0, 2, 11 + bi)
        sc = score_logits(logits, cu_seqlens=cu, labels=lab, seqs=draws, want=("seq_nll", "seq_match"))
        pred = letters_padded(score_logits(logits, cu_seqlens=cu, want=("pred",), max_len=max_len)["pred"])
        for r, i in enumerate(idx):
            preds[i] = pred[r]
            lines[i] = [f"{items[i][0]},{s},{letters_padded(draws[s])[r]},{float(sc['seq_nll'][s, r]) / lengths[i]:.6f},"
                        f"{int(sc['seq_match'][s, r]) / lengths[i]:.6f}\n" for s in range(2)]
    want = "pdb_id,sample,seq,nll_per_nt,recovery\n" + "".join("".join(lines[i]) for i in range(len(items)))
    assert open(des).read() == want
    assert open(sub).read() == "pdb_id,seq\n" + "".join(f"{items[i][0]},{preds[i]}\n" for i in range(len(items)))
