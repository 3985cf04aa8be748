"""``rnampnn_design_gc`` (csrc/design_gc.hip) on the device, against the float64 restatement of its contract in tests/_design_gc_ref.py.

The batch is the one ``_design_gc_ref`` describes next to ``CASE_LENGTHS`` (lengths 0, 1, 2, 3, 63, 64, 65, 257, 300; T = 300, S = 4, logits
3 * randn, the global bias -4 on C and G, a seed above 2^32): a hairpin, pairs across the 256-stride and across a node boundary of every
level of the 257-mer, a pseudoknot, a fixed end inside a pair, an infeasible pair, ``allowed = 0``, a malformed partner table; the free
window, a single count, the far tail (>= 80 % G+C under that bias), an unreachable window, lo > hi and out-of-range windows.  The windows are
absolute counts, so the entry is called through ctypes; the Python surface (fractions) has its own tests at the end.

Device and restatement differ by last-bit exp / log and the summation order inside a node (about 1e-12 relative), so a draw whose path has
a selection within 1e-8 of a cumulative boundary is left out of the equality check; tests/test_design_gc_cpu.py bounds the share of such
draws by 1 % for the restatement alone, and the same bound is asserted here."""
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

import _design_gc_ref as G  # noqa: E402
from _design_ref import PAIRS  # noqa: E402
from _design_case import SMALL, raw_design, _bytes, _dev, _specs, _write_data, _checkpoint  # noqa: E402

LENGTHS, T, S, SEED = G.CASE_LENGTHS, G.CASE_T, G.CASE_S, G.CASE_SEED
NEAR = 1e-8
T_MAX = 1017                                                       # the largest padded extent whose tree fits 160 KiB of LDS


def design_gc(logits, lo, hi, seed=SEED, S=S, **kw):
    """The C entry on device tensors (numpy arrays are uploaded) -> dict of its five outputs."""
    return raw_design("rnampnn_design_gc", (_dev(lo, torch.int32), _dev(hi, torch.int32)),
                      (("gc_count", torch.int32, True), ("gc_miss", torch.int32, False)), logits, seed=seed, S=S, **kw)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = G.case_arrays()
    d = dict(h=h, run={})
    for k in ("logits", "mask", "allowed", "partner", "packed", "cu", "lo", "hi"):
        d[k] = torch.from_numpy(h[k]).cuda()
    d["bias"] = torch.from_numpy(G.CASE_BIAS).cuda()
    return d


def _run(case, temperature=1.0, layout="padded"):
    """The batch through the kernel, once per (temperature, layout)."""
    key = (float(temperature), layout)
    if key not in case["run"]:
        kw = dict(temperature=temperature, allowed=case["allowed"], partner=case["partner"], bias=case["bias"])
        if layout == "padded":
            case["run"][key] = design_gc(case["logits"], case["lo"], case["hi"], mask=case["mask"], **kw)
        else:
            case["run"][key] = design_gc(case["packed"], case["lo"], case["hi"], cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _window(b):
    lo = min(max(G.CASE_LO[b], 0), LENGTHS[b])
    return lo, max(min(max(G.CASE_HI[b], 0), LENGTHS[b]), lo)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_restatement(case, temperature):
    out = _run(case, temperature)
    want, margin, bad, miss, _ = G.case_ref(temperature)
    got = out["seqs"].cpu().numpy()
    near = margin <= NEAR
    print(f"temperature {temperature}: {near.mean():.4%} of the {near.size} (sample, RNA) draws left out (a selection within {NEAR} of a boundary)")
    assert near.mean() <= 0.01
    assert out["gc_miss"].tolist() == miss.tolist() == G.CASE_MISS
    assert out["infeasible"].tolist() == bad.tolist() == G.CASE_INFEASIBLE
    differ = [(s, b) for s in range(S) for b in range(len(LENGTHS)) if not near[s, b] and not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"


def test_gc_count_is_the_count_of_the_bytes_and_lies_in_the_window(case):
    for temperature in (1.0, 0.3, 1e-3):
        out = _run(case, temperature)
        got = out["seqs"].cpu().numpy()
        count = out["gc_count"].cpu().numpy()
        assert np.array_equal(count, (got >= 2).sum(axis=2))
        for b, n in enumerate(LENGTHS):
            assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
            lo, hi = _window(b)
            if G.CASE_MISS[b] == 0:
                assert ((count[:, b] >= lo) & (count[:, b] <= hi)).all(), (temperature, b, count[:, b])
        assert (count[:, 2] == 0).all()                            # the unreachable window: the nearest reachable count


def test_masks_and_pair_compatibility_hold_in_every_draw(case):
    h = case["h"]
    for temperature in (1.0, 1e-3):
        got = _run(case, temperature)["seqs"].cpu().numpy()
        for b, n in enumerate(LENGTHS):
            m = h["allowed"][b, :n].astype(np.int64) & 15
            m = np.where(m == 0, 15, m)
            assert ((m[None] >> got[:, b, :n]) & 1).all(), b
        for b, i, j in G.CASE_PAIRS:
            if b != 2:                                             # (2; 0,1) is the infeasible pair
                assert all((int(got[s, b, i]), int(got[s, b, j])) in PAIRS[True] for s in range(S)), (b, i, j)
        assert (got[:, 4, 5] == 3).all() and np.isin(got[:, 4, 57], [1, 2]).all()      # G fixed inside a pair: its partner is C or U


def test_cold_limit_is_the_max_plus_optimum(case):
    """Temperature 1e-3: an alternative whose sum of (logit + bias) falls short by more than 0.05 carries a weight below e^-50
    (tests/test_design_gc_cpu.py confirms it for the restatement's own draw)."""
    h = case["h"]
    got = _run(case, 1e-3)["seqs"].cpu().numpy()
    zb = h["logits"].astype(np.float64) + G.CASE_BIAS.astype(np.float64)
    for b, n in enumerate(LENGTHS):
        if n == 0:
            continue
        best = G.GcPlan(h["logits"][b], n, 1.0, h["lo"][b], h["hi"][b], h["allowed"][b], h["partner"][b], True, G.CASE_BIAS, maxplus=True).optimum()
        for s in range(S):
            total = float(sum(zb[b, t, got[s, b, t]] for t in range(n)))
            assert best - 0.05 <= total <= best + 1e-9, (b, s, total, best)


def test_seq_nll_is_rnampnn_scores_byte_for_byte(case):
    from rnampnn.model.decode import score_logits
    for layout in ("padded", "packed"):
        out = _run(case, 0.3, layout)
        if layout == "padded":
            sc = score_logits(case["logits"], mask=case["mask"], seqs=out["seqs"], want=("seq_nll",))
        else:
            sc = score_logits(case["packed"], cu_seqlens=case["cu"], seqs=out["seqs"], want=("seq_nll",))
        assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"]), layout
        assert float(out["seq_nll"][:, 0].abs().max()) == 0.0 and bool((out["seq_nll"][:, 1:] > 0).all())


def test_layout_padding_batch_and_sample_count_do_not_change_the_bytes(case):
    h = case["h"]
    base = _run(case, 0.3)
    kw = dict(temperature=0.3, bias=case["bias"])
    # packed, and a second call
    for other in (_run(case, 0.3, "packed"), design_gc(case["logits"], case["lo"], case["hi"], mask=case["mask"], allowed=case["allowed"],
                                                       partner=case["partner"], **kw)):
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in base)
    # T = 320 with garbage beyond every length: NaN logits, random masks, partners that point anywhere
    B, T2 = len(LENGTHS), 320
    rng = np.random.RandomState(5)
    logits = np.full((B, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B, T2)).astype(np.uint8)
    partner = rng.randint(-3, 400, size=(B, T2)).astype(np.int32)
    mask = np.zeros((B, T2), dtype=np.float32)
    for b, n in enumerate(LENGTHS):
        logits[b, :n], allowed[b, :n], partner[b, :n], mask[b, :n] = h["logits"][b, :n], h["allowed"][b, :n], h["partner"][b, :n], 1
    partner[5, 25], partner[5, 70] = 70, 25                       # the table of the 64-mer keeps its entry in the padding that points back
    wide = design_gc(logits, h["lo"], h["hi"], mask=mask, allowed=allowed, partner=partner, **kw)
    assert _bytes(wide["seqs"][:, :, :T]) == _bytes(base["seqs"]) and bool((wide["seqs"][:, :, T:] == -1).all())
    assert all(_bytes(base[k]) == _bytes(wide[k]) for k in ("seq_nll", "infeasible", "gc_count", "gc_miss"))
    # a leading sub-batch; S = 1 against S = 4
    sub = design_gc(case["logits"][:5], case["lo"][:5], case["hi"][:5], mask=case["mask"][:5], allowed=case["allowed"][:5],
                    partner=case["partner"][:5], **kw)
    assert _bytes(sub["seqs"]) == _bytes(base["seqs"][:, :5]) and _bytes(sub["seq_nll"]) == _bytes(base["seq_nll"][:, :5])
    assert _bytes(sub["gc_count"]) == _bytes(base["gc_count"][:, :5]) and sub["gc_miss"].tolist() == G.CASE_MISS[:5]
    one = design_gc(case["logits"], case["lo"], case["hi"], mask=case["mask"], allowed=case["allowed"], partner=case["partner"], S=1, **kw)
    assert _bytes(one["seqs"][0]) == _bytes(base["seqs"][0]) and _bytes(one["seq_nll"][0]) == _bytes(base["seq_nll"][0])
    assert one["infeasible"].tolist() == G.CASE_INFEASIBLE and one["gc_miss"].tolist() == G.CASE_MISS
    # a per-position bias that repeats the global one
    per = design_gc(case["logits"], case["lo"], case["hi"], mask=case["mask"], allowed=case["allowed"], partner=case["partner"],
                    temperature=0.3, bias=case["bias"].expand(B, T, 4).contiguous())
    assert all(_bytes(base[k]) == _bytes(per[k]) for k in base)


def test_nan_logits_still_give_ids_and_an_in_range_count(case):
    """Row 7 (the 257-mer) gets NaN, +inf and -inf logits: ids in 0..3, gc_count = the count of the bytes; every other row keeps its bytes."""
    base = _run(case, 1.0)
    logits = case["logits"].clone()
    logits[7, 40] = float("nan")
    logits[7, 41, 2] = float("inf")
    logits[7, 42, 1] = float("-inf")
    logits[7, 128:140] = float("nan")
    out = design_gc(logits, case["lo"], case["hi"], mask=case["mask"], allowed=case["allowed"], partner=case["partner"], bias=case["bias"])
    got = out["seqs"].cpu().numpy()
    assert ((got[:, 7, :257] >= 0) & (got[:, 7, :257] <= 3)).all() and (got[:, 7, 257:] == -1).all()
    count = out["gc_count"].cpu().numpy()
    assert np.array_equal(count, (got >= 2).sum(axis=2)) and ((count[:, 7] >= 0) & (count[:, 7] <= 257)).all()
    rows = [b for b in range(len(LENGTHS)) if b != 7]
    assert _bytes(out["seqs"][:, rows]) == _bytes(base["seqs"][:, rows]) and _bytes(out["gc_count"][:, rows]) == _bytes(base["gc_count"][:, rows])
    assert out["infeasible"].tolist() == G.CASE_INFEASIBLE
    nan_bias = design_gc(case["logits"], case["lo"], case["hi"], mask=case["mask"], allowed=case["allowed"], partner=case["partner"],
                         bias=torch.full((4,), float("nan")))
    got = nan_bias["seqs"].cpu().numpy()
    assert all(((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all() and (got[:, b, n:] == -1).all() for b, n in enumerate(LENGTHS))
    assert np.array_equal(nan_bias["gc_count"].cpu().numpy(), (got >= 2).sum(axis=2))


# ---------------------------------------------------------------------------------------------------------------- the size limit
def test_the_largest_extent_that_fits_and_one_past_it():
    """One RNA of T_MAX nucleotides (the tree fills the LDS a workgroup may ask for): the window holds, the draws equal the restatement and
    the NLL bytes are rnampnn_score's.  T_MAX + 1 is NotImplementedError naming the limit."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import design_gc_from_logits, score_logits
    n = T_MAX
    rng = np.random.RandomState(11)
    logits = (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32)
    mask = np.ones((1, n), dtype=np.float32)
    partner = np.full((1, n), -1, dtype=np.int32)
    for i in range(150):                                           # a long hairpin whose pairs cross the root's boundary
        partner[0, 300 + i], partner[0, 800 - i] = 800 - i, 300 + i
    allowed = np.full((1, n), 15, dtype=np.uint8)
    allowed[0, ::7] = 12                                           # S = C or G
    lo, hi = np.array([560], dtype=np.int32), np.array([600], dtype=np.int32)
    out = design_gc(logits, lo, hi, mask=mask, S=2, allowed=allowed, partner=partner)
    want, margin, bad, miss, _ = G.design_gc_ref(logits, [n], 1.0, 2, SEED, lo, hi, allowed, partner, True)
    got, count = out["seqs"].cpu().numpy(), out["gc_count"].cpu().numpy()
    assert out["gc_miss"].tolist() == miss.tolist() == [0] and out["infeasible"].tolist() == bad.tolist() == [0]
    assert np.array_equal(count, (got >= 2).sum(axis=2)) and ((count >= 560) & (count <= 600)).all()
    print(f"T = {n}: margins {margin[:, 0]}")
    for s in range(2):
        assert margin[s, 0] <= NEAR or np.array_equal(got[s, 0], want[s, 0]), s
        assert all((int(got[s, 0, 300 + i]), int(got[s, 0, 800 - i])) in PAIRS[True] for i in range(150))
    sc = score_logits(torch.from_numpy(logits).cuda(), mask=torch.from_numpy(mask).cuda(), seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])
    with pytest.raises(NotImplementedError, match=rf"the limit is 163840 \(T <= {T_MAX}\)"):
        design_gc_from_logits(torch.zeros(1, n + 1, 4, device="cuda"), mask=torch.ones(1, n + 1, device="cuda"), n_samples=1, temperature=1.0)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_design_gc_from_logits_forms_the_counts_on_the_device(case):
    """Fractions -> counts per RNA (lo = ceil(f_lo n - 1e-6), hi = floor(f_hi n + 1e-6)) in both layouts, a pair and a (B,2) device tensor."""
    from rnampnn.model.decode import design_gc_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    cons = DesignConstraints(case["allowed"], case["partner"], case["bias"], True)
    lo = np.array([int(np.ceil(0.4 * n - 1e-6)) for n in LENGTHS], dtype=np.int32)
    hi = np.array([int(np.floor(0.6 * n + 1e-6)) for n in LENGTHS], dtype=np.int32)
    want = design_gc(case["logits"], lo, hi, mask=case["mask"], temperature=0.5, seed=77, allowed=case["allowed"], partner=case["partner"],
                     bias=case["bias"])
    kw = dict(n_samples=S, temperature=0.5, seed=77, constraints=cons)
    fr = torch.tensor([[0.4, 0.6]] * len(LENGTHS), dtype=torch.float64, device="cuda")   # (float32 fractions carry their rounding into f * n)
    for name, got in (("padded", design_gc_from_logits(case["logits"], mask=case["mask"], gc_content=(0.4, 0.6), **kw)),
                      ("packed", design_gc_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, gc_content=(0.4, 0.6), **kw)),
                      ("tensor", design_gc_from_logits(case["logits"], mask=case["mask"], gc_content=fr, **kw))):
        assert len(got) == 5 and [t.dtype for t in got] == [torch.int8, torch.float32, torch.int32, torch.int32, torch.int32]
        for a, k in zip(got, ("seqs", "seq_nll", "infeasible", "gc_count", "gc_miss")):
            assert _bytes(a) == _bytes(want[k]), (name, k)
    count, miss = want["gc_count"].cpu().numpy(), want["gc_miss"].tolist()
    # n = 1: ceil(0.4) = 1 > floor(0.6) = 0 is read as (1, 1); n = 2 is fixed to AA: the count 1 is out of reach
    assert miss == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    for b, n in enumerate(LENGTHS):
        if miss[b] == 0:
            assert ((count[:, b] >= lo[b]) & (count[:, b] <= max(hi[b], lo[b]))).all(), b


MODEL_LENGTHS = [33, 20, 41]


def _check_window(seqs, count, lengths, lo_f, hi_f):
    got = seqs.cpu().numpy()
    assert np.array_equal(count.cpu().numpy(), (got >= 2).sum(axis=2))
    for b, n in enumerate(lengths):
        lo, hi = int(np.ceil(lo_f * n - 1e-6)), int(np.floor(hi_f * n + 1e-6))
        assert ((got[:, b, :n] >= 2).sum(axis=1) >= lo).all() and ((got[:, b, :n] >= 2).sum(axis=1) <= hi).all(), b


def test_both_models_design_under_a_gc_window():
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
    tri = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=cons)
    assert len(tri) == 3                                            # None keeps today's path and today's return value
    for constraints in (None, cons):
        out = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=constraints, gc_content=(0.5, 0.6))
        assert len(out) == 5 and out[0].shape == (3, 3, max(lens)) and out[2].tolist() == [0, 0, 0] and out[4].tolist() == [0, 0, 0]
        _check_window(out[0], out[3], lens, 0.5, 0.6)
        assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    with pytest.raises(ValueError, match="gc_content together with states"):
        m.design(c, mask, states=[1, 2], gc_content=(0.5, 0.6))
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    out = r.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS, gc_content=(0.3, 0.4))
    assert len(out) == 5 and out[0].shape == (3, 3, max(lens)) and out[4].tolist() == [0, 0, 0]
    _check_window(out[0], out[3], lens, 0.3, 0.4)
    assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    assert len(r.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS)) == 3


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_a_gc_window(family, tmp_path):
    """--gc-content adds the columns gc and gc_miss and holds every draw to the window, alone and next to the constraint flags; the
    designs file written without the flag is byte for byte the same before and after."""
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
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    sub = str(tmp_path / "submit.csv")
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", sub, "--samples", "3", "--temperature", "1.0", "--batch-size", "2"]
    quiet = dict(log=lambda *a: None)
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "before.csv")]), **quiet)
    length = dict(zip(ids, lens))
    for name, flags in (("gc", []), ("gc_cons", ["--constraints", str(tmp_path / "cons.csv"), "--bias", "G=-0.25", "--omit", "", "--no-wobble"])):
        des = str(tmp_path / f"{name}.csv")
        P.run(P.parse(common + ["--designs-out", des, "--gc-content", "0.5:0.6"] + flags), **quiet)
        d = list(csv.reader(open(des)))
        base = ["pdb_id", "sample", "seq", "nll_per_nt", "recovery"] + (["infeasible"] if flags or family == "rdesign" else [])
        assert d[0] == base + ["gc", "gc_miss"] and len(d) == 1 + 3 * 3
        for r in d[1:]:
            n = length[r[0]]
            k = sum(ch in "CG" for ch in r[2])
            assert len(r[2]) == n and r[-1] == "0" and r[-2] == f"{k / n:.6f}"
            assert int(np.ceil(0.5 * n - 1e-6)) <= k <= int(np.floor(0.6 * n + 1e-6)), r
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "after.csv")]), **quiet)
    assert open(tmp_path / "before.csv", "rb").read() == open(tmp_path / "after.csv", "rb").read()
    assert list(csv.reader(open(tmp_path / "before.csv")))[0][-1] in ("recovery", "infeasible")
    with pytest.raises(ValueError, match="--gc-content.*--states"):
        P.run(P.parse(common + ["--gc-content", "0.5:0.6", "--states", str(tmp_path / "cons.csv")]), **quiet)
