"""``rnampnn_design_count_long`` / ``rnampnn_design_count_profile_long`` (csrc/design_long.hip): the count tree in a workspace in global
memory, on the device.

Anchor.  Wherever the LDS entries accept a call - the G+C tests' batch, the count tests' batch at cap 8 (the k_min rule) and at cap T, at
temperatures 1.0 and 0.1 - every output with ``tree="global"`` equals the output with ``tree="lds"`` byte for byte: two HIP paths, no
restatement.

Long lengths.  The cases of tests/_design_long_case.py - 1018, 1025, 2049 uncapped, 2868 at cap 8 with the k_min rule, one padded batch of
the lengths 1, 2, 3, 700, 1300 - against the float64 restatements.  Device and restatement differ by last-bit exp / log and the order of
summation inside a node, so a draw whose path has a selection within NEAR = 1e-8 of a cumulative boundary could differ; the cases are chosen
so that the restatement's smallest margin exceeds NEAR (asserted here and in tests/test_design_long_cpu.py), and NO draw is left out.
Profiles are held to the tolerances of tests/test_design_profile_gpu.py (``_agree``: marginals 1e-8 absolute, scalars 1e-8 max(1, |value|)).

Independence: the bytes do not depend on the layout, the batch, S, the padded extent or what the workspace held before the call."""
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

import _design_count_ref as R  # noqa: E402
import _design_gc_ref as G  # noqa: E402
import _design_long_case as L  # noqa: E402
import test_design_profile_gpu as TP  # noqa: E402  (its TOL is the profile tolerance, its count_profile the LDS entry)
from _design_ref import PAIRS  # noqa: E402
from _design_case import SMALL, agree_profile, profile_outputs, raw_design, raw_profile, _bytes, _dev, _write_data  # noqa: E402

NEAR = L.NEAR
FURTHER = (("count", torch.int32, True), ("count_miss", torch.int32, False))
OUTPUTS = ("seqs", "seq_nll", "infeasible", "count", "count_miss")
LONG_PADDING = 1408                                                # the padded extent of the models that design the 1,300-nt RNA


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _workspace(symbol, B, T, cap, fill=None):
    """A workspace of ``symbol``(B, T, cap) bytes -> (uint8 tensor, the size as the ABI takes it); ``fill``: a byte it holds everywhere."""
    from rnampnn import _native
    need = int(getattr(_native.lib(), symbol)(B, T, max(int(cap), 1)))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws, C.c_size_t(need)


def count_long(logits, counted, lo, hi, cap, ws=None, S=L.S, seed=L.SEED, **kw):
    """The C entry on device tensors (numpy arrays are uploaded) -> dict of its five outputs.  ``ws``: (tensor, size), else a fresh one."""
    m, cu = kw.get("mask"), kw.get("cu")
    B = int(m.shape[0]) if m is not None else len(cu) - 1
    T = int(m.shape[1]) if m is not None else int(kw["T"])
    ws = _workspace("rnampnn_design_count_long_workspace_bytes", B, T, cap) if ws is None else ws
    return raw_design("rnampnn_design_count_long", (_dev(counted, torch.uint8), _dev(lo, torch.int32), _dev(hi, torch.int32), int(cap), *ws),
                      FURTHER, logits, seed=seed, S=S, **kw)


def profile_long(c, ws=None, layout="padded"):
    """``rnampnn_design_count_profile_long`` on a case of ``_design_long_case`` -> dict of its six outputs."""
    ws = _workspace("rnampnn_design_count_profile_long_workspace_bytes", c["B"], c["T"], c["cap"]) if ws is None else ws
    own = (_dev(c["counted"], torch.uint8), _dev(c["lo"], torch.int32), _dev(c["hi"], torch.int32), int(c["cap"]), *ws)
    kw = dict(mask=c["mask"]) if layout == "padded" else dict(cu=c["cu"], T=c["T"])
    return raw_profile("rnampnn_design_count_profile_long", own, c["logits"] if layout == "padded" else c["packed"], allowed=c["allowed"],
                       partner=c["partner"], wobble=c["wobble"], **kw)


def _run(c, layout="padded", **kw):
    """A case of ``_design_long_case`` through the draw entry."""
    args = dict(allowed=c["allowed"], partner=c["partner"], wobble=c["wobble"])
    args.update(dict(mask=c["mask"]) if layout == "padded" else dict(cu=c["cu"], T=c["T"]))
    args.update(kw)
    return count_long(c["logits"] if layout == "padded" else c["packed"], c["counted"], c["lo"], c["hi"], c["cap"], **args)


_RUNS = {}


def _base(name):
    """The case through the draw entry in the padded layout, once per process."""
    if name not in _RUNS:
        _RUNS[name] = _run(L.case(name))
    return _RUNS[name]


# ---------------------------------------------------------------------------------------------------------------- 1: the anchor
@pytest.mark.parametrize("temperature", [1.0, 0.1])
def test_anchor_the_gc_batch_has_the_bytes_of_the_lds_entry(built, temperature):
    """``design_gc_from_logits``: "lds" is rnampnn_design_gc, "global" rnampnn_design_count_long with C|G counted and a cap of T, "auto"
    takes the LDS entry here - the same five-tuple, byte for byte."""
    from rnampnn.model.decode import design_gc_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    h = G.case_arrays()
    lg, m = _dev(h["logits"]), _dev(h["mask"])
    cons = DesignConstraints(_dev(h["allowed"]), _dev(h["partner"]), _dev(G.CASE_BIAS), True)
    window = torch.stack([torch.tensor(h["lo"]), torch.tensor(h["hi"])], dim=1).to(torch.float64) / torch.tensor(
        [max(n, 1) for n in G.CASE_LENGTHS], dtype=torch.float64)[:, None]
    window = window.clamp(0, 1).cuda()                                 # fractions whose counts gc_counts turns back into the case's windows
    kw = dict(mask=m, n_samples=G.CASE_S, temperature=temperature, seed=G.CASE_SEED, constraints=cons, gc_content=window)
    lds, glob, auto = (design_gc_from_logits(lg, tree=tree, **kw) for tree in ("lds", "global", "auto"))
    assert len(lds) == len(glob) == 5 and [t.dtype for t in glob] == [t.dtype for t in lds] and [t.shape for t in glob] == [t.shape for t in lds]
    assert lds[4].tolist()[2] == 1                                     # the unreachable window of RNA 2 is part of the comparison
    for k, a, b, c in zip(OUTPUTS, lds, glob, auto):
        assert _bytes(a) == _bytes(b) == _bytes(c), k


@pytest.mark.parametrize("cap", R.CASE_CAPS)
@pytest.mark.parametrize("temperature", [1.0, 0.1])
def test_anchor_the_count_batch_has_the_bytes_of_the_lds_entry(built, temperature, cap):
    """The count tests' batch - the budget, windows nothing reaches, and at cap 8 the k_min rule on RNA 8 - through
    ``design_count_from_logits`` with a device window: every output is the LDS entry's."""
    from rnampnn.model.decode import design_count_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    h = R.case_arrays()
    cons = DesignConstraints(_dev(h["allowed"]), _dev(h["partner"]), None, R.CASE_WOBBLE)
    window = torch.stack([torch.tensor(h["lo"]), torch.tensor(h["hi"])], dim=1).cuda()
    kw = dict(mask=_dev(h["mask"]), n_samples=R.CASE_S, temperature=temperature, seed=R.CASE_SEED, constraints=cons, counted=_dev(h["counted"]),
              window=window, cap=cap)
    lds, glob = (design_count_from_logits(_dev(h["logits"]), tree=tree, **kw) for tree in ("lds", "global"))
    plans = R.case_ref(1.0, cap)[5]
    assert plans[8].at_min == (cap == 8) and lds[4].tolist()[8] == plans[8].k_min - 3
    for k, a, b in zip(OUTPUTS, lds, glob):
        assert _bytes(a) == _bytes(b), k
    packed = design_count_from_logits(_dev(h["packed"]), tree="global", cu_seqlens=_dev(h["cu"]), max_len=R.CASE_T,
                                      **{k: v for k, v in kw.items() if k != "mask"})
    for k, a, b in zip(OUTPUTS, lds, packed):
        assert _bytes(a) == _bytes(b), ("packed", k)


@pytest.mark.parametrize("temperature", [1.0, 0.1])
def test_anchor_every_field_of_the_profile_has_the_bytes_of_the_lds_entry(built, temperature):
    """``design_profile_from_logits`` in its three count modes on the count tests' batch, and the raw entries at cap 8 (the k_min rule)."""
    from rnampnn.model.decode import design_profile_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    h = R.case_arrays()
    lg, m = _dev(h["logits"]), _dev(h["mask"])
    cons = DesignConstraints(_dev(h["allowed"]), _dev(h["partner"]), None, R.CASE_WOBBLE)
    for mode, own in (("plain", {}), ("gc_content", dict(gc_content=(0.3, 0.5))), ("mutations", dict(mutations=(_dev(h["reference"]), 1, 5)))):
        lds, glob, auto = (design_profile_from_logits(lg, mask=m, temperature=temperature, constraints=cons, tree=tree, **own)
                           for tree in ("lds", "global", "auto"))
        assert lds.mode == glob.mode == auto.mode == mode
        for k in TP.OUTPUTS:
            assert _bytes(getattr(lds, k)) == _bytes(getattr(glob, k)) == _bytes(getattr(auto, k)), (mode, k)
    c = dict(B=len(R.CASE_LENGTHS), T=R.CASE_T, logits=h["logits"], mask=h["mask"], allowed=h["allowed"], partner=h["partner"], counted=h["counted"],
             lo=h["lo"], hi=h["hi"], wobble=R.CASE_WOBBLE, packed=h["packed"], cu=h["cu"])
    for cap in R.CASE_CAPS:
        lds = TP.count_profile(h["logits"], h["counted"], h["lo"], h["hi"], cap, mask=h["mask"], allowed=h["allowed"], partner=h["partner"])
        assert lds["miss"].tolist()[8] > 0
        for layout in ("padded", "packed"):
            glob = profile_long(dict(c, cap=cap), layout=layout)
            for k in TP.OUTPUTS:
                assert _bytes(lds[k]) == _bytes(glob[k]), (cap, layout, k)


# ---------------------------------------------------------------------------------------------------------------- 2: long lengths
@pytest.mark.parametrize("name", ["gc1018", "gc1025", "gc2049", "mut2868", "mixed"])
def test_long_draws_equal_the_float64_restatement(built, name):
    """No draw is left out: the restatement's smallest margin exceeds NEAR.  seq_nll is rnampnn_score's byte for byte, ``count`` is the
    count of the written bytes and lies in the window wherever count_miss is 0; the pairs pair and the stripe's sets hold."""
    from rnampnn.model.decode import score_logits
    c = L.case(name)
    want, margin, bad, miss, plans = L.draw_ref(name)
    print(f"{name}: the restatement's smallest margin {margin.min():.3e}")
    assert margin.min() > NEAR
    out = _base(name)
    got, count = out["seqs"].cpu().numpy(), out["count"].cpu().numpy()
    assert out["count_miss"].tolist() == miss.tolist() and out["infeasible"].tolist() == bad.tolist()
    differ = [(s, b) for s in range(L.S) for b in range(c["B"]) if not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"
    assert np.array_equal(count, L.count_of(got, c["counted"]))
    for b, n in enumerate(c["lengths"]):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
        top = min(n, c["cap"])
        lo = min(max(int(c["lo"][b]), 0), top)
        hi = max(min(max(int(c["hi"][b]), 0), top), lo)
        if miss[b] == 0:
            assert ((count[:, b] >= lo) & (count[:, b] <= hi)).all(), (b, count[:, b], lo, hi)
        assert ((c["allowed"][b, :n].astype(np.int64)[None] >> got[:, b, :n]) & 1).all(), b
        if n >= 64:
            assert all((int(got[s, b, i]), int(got[s, b, j])) in PAIRS[c["wobble"]] for s in range(L.S) for i, j in L.hairpin(n)), b
    if name == "mut2868":                                               # a window nothing reaches: the k_min rule
        assert miss[0] == 0 and miss[1] > 0 and plans[1].at_min and (count[:, 1] == plans[1].k_min).all() and plans[1].k_min == 8 + miss[1]
    sc = score_logits(_dev(c["logits"]), mask=_dev(c["mask"]), seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])


@pytest.mark.parametrize("name", ["pf1025", "pf1458", "mixed"])
def test_long_profiles_agree_with_the_float64_restatement(built, name):
    c = L.case(name)
    out = profile_long(c)
    agree_profile(out, L.profile_ref(name), f"long profile {name}", tol=TP.TOL)
    marg = out["marginals"].cpu().numpy()
    for b, n in enumerate(c["lengths"]):
        assert (marg[b, n:] == 0).all() and np.allclose(marg[b, :n].sum(axis=1), 1.0, atol=1e-9)
    # the draw entry's flags, byte for byte
    draw = _run(c, S=1)
    assert _bytes(out["infeasible"]) == _bytes(draw["infeasible"]) and _bytes(out["miss"]) == _bytes(draw["count_miss"])


# ---------------------------------------------------------------------------------------------------------------- 3: independence
def test_the_bytes_do_not_depend_on_layout_batch_samples_extent_or_the_workspace(built):
    c = L.case("mixed")
    B, T = c["B"], c["T"]
    base = _base("mixed")

    def same(a, b, what):
        differ = [k for k in OUTPUTS if _bytes(a[k]) != _bytes(b[k])]
        assert not differ, (what, differ)
    same(base, _run(c, layout="packed"), "packed")
    # what the workspace held before the call: 0xFF everywhere (NaN as doubles, with the sign set), quiet NaNs, the previous call's contents
    ws = _workspace("rnampnn_design_count_long_workspace_bytes", B, T, c["cap"], fill=0xFF)
    same(base, _run(c, ws=ws), "a workspace of 0xFF")
    ws[0].view(torch.float64).fill_(float("nan"))
    same(base, _run(c, ws=ws), "a workspace of NaN")
    same(base, _run(c, ws=ws), "the previous call's workspace")
    same(base, _run(c, ws=ws, layout="packed"), "the previous call's workspace, packed")
    # S = 2 is the first two of S = 5
    five = _run(c, S=5)
    assert all(_bytes(five[k][:L.S]) == _bytes(base[k]) for k in ("seqs", "seq_nll", "count"))
    assert all(_bytes(five[k]) == _bytes(base[k]) for k in ("infeasible", "count_miss"))
    # the 700-mer alone (B = 1) at its row index: garbage rows around it, another B and T
    b, n = 3, c["lengths"][3]
    rng = np.random.RandomState(5)
    B2, T2 = 4, 704
    logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    partner = rng.randint(-3, 2000, size=(B2, T2)).astype(np.int32)
    counted = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    mask = np.zeros((B2, T2), dtype=np.float32)
    logits[b, :n], allowed[b, :n], partner[b, :n], counted[b, :n], mask[b, :n] = (c["logits"][b, :n], c["allowed"][b, :n], c["partner"][b, :n],
                                                                                 c["counted"][b, :n], 1)
    lo, hi = np.full(B2, c["lo"][b], dtype=np.int32), np.full(B2, c["hi"][b], dtype=np.int32)
    one = count_long(logits, counted, lo, hi, T2, mask=mask, allowed=allowed, partner=partner, wobble=c["wobble"])
    assert _bytes(one["seqs"][:, b, :n]) == _bytes(base["seqs"][:, b, :n]) and bool((one["seqs"][:, b, n:] == -1).all())
    assert all(_bytes(one[k][:, b]) == _bytes(base[k][:, b]) for k in ("seq_nll", "count"))
    assert all(int(one[k][b]) == int(base[k][b]) for k in ("infeasible", "count_miss"))
    assert bool((one["seqs"][:, :b] == -1).all())
    # a larger padded T with the same rows (the cap stays: only the extent grows)
    T3 = T + 77
    wide = {k: np.concatenate([c[k], np.full((B, 77) + c[k].shape[2:], fill, dtype=c[k].dtype)], axis=1)
            for k, fill in (("logits", 0), ("mask", 0), ("allowed", 255), ("partner", 5), ("counted", 255))}
    big = count_long(wide["logits"], wide["counted"], c["lo"], c["hi"], T3, mask=wide["mask"], allowed=wide["allowed"], partner=wide["partner"],
                     wobble=c["wobble"])
    assert _bytes(big["seqs"][:, :, :T]) == _bytes(base["seqs"]) and bool((big["seqs"][:, :, T:] == -1).all())
    assert all(_bytes(big[k]) == _bytes(base[k]) for k in ("seq_nll", "infeasible", "count", "count_miss"))


def test_the_profile_does_not_depend_on_layout_or_the_workspace(built):
    c = L.case("mixed")
    base = profile_long(c)
    ws = _workspace("rnampnn_design_count_profile_long_workspace_bytes", c["B"], c["T"], c["cap"], fill=0xFF)
    for what, other in (("packed", profile_long(c, layout="packed")), ("a workspace of 0xFF", profile_long(c, ws=ws)),
                        ("the previous call's workspace", profile_long(c, ws=ws))):
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in TP.OUTPUTS), what


def test_both_entries_replay_from_a_captured_graph_with_the_same_bytes(built):
    """Several launches on one stream and nothing else: a captured call replays, twice, with the bytes of the plain call."""
    from _design_case import design_outputs
    c = L.case("mixed")
    base, pbase = _base("mixed"), profile_long(c)
    out, pout = design_outputs(FURTHER, L.S, c["B"], c["T"]), profile_outputs(c["B"], c["T"])
    ws = _workspace("rnampnn_design_count_long_workspace_bytes", c["B"], c["T"], c["cap"])
    pws = _workspace("rnampnn_design_count_profile_long_workspace_bytes", c["B"], c["T"], c["cap"])
    dev = {k: _dev(c[k]) for k in ("logits", "mask", "allowed", "partner", "counted", "lo", "hi")}

    def both():
        count_long(dev["logits"], dev["counted"], dev["lo"], dev["hi"], c["cap"], ws=ws, mask=dev["mask"], allowed=dev["allowed"],
                   partner=dev["partner"], wobble=c["wobble"], out=out)
        raw_profile("rnampnn_design_count_profile_long", (dev["counted"], dev["lo"], dev["hi"], int(c["cap"]), *pws), dev["logits"],
                    mask=dev["mask"], allowed=dev["allowed"], partner=dev["partner"], wobble=c["wobble"], out=pout)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                          # (what a first call sets up happens outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(2):
        for t in list(out.values()) + list(pout.values()):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS)
        assert all(_bytes(pbase[k]) == _bytes(pout[k]) for k in TP.OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- 4: the surface
LONG_N = 1300


def _long_models():
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    torch.manual_seed(0)
    return RNAMPNN(precision="f32", **dict(SMALL, padding_len=LONG_PADDING)).cuda().eval(), RNAModel(num_mpnn_layers=1).cuda().eval()


def test_both_models_design_a_1300_nt_rna_inside_a_gc_window(built):
    """``tree="auto"`` takes the long entry where LDS refuses: the G+C count of every draw lies in 45-60 % of 1,300; without ``tree`` the
    call fails with the message it has always had."""
    from rnampnn.utils import synth
    m, r = _long_models()
    coords = torch.from_numpy(synth.synth_rna(LONG_N, 3, seed=1).astype(np.float32))[None].cuda()
    mask = torch.ones(1, LONG_N, device="cuda")
    lo, hi = L.gc_window(LONG_N)
    for model, x, kw in ((m, coords, {}), (r, coords[:, :, :6].contiguous(), dict(lengths=[LONG_N]))):
        out = model.design(x, mask, n_samples=2, temperature=1.0, seed=3, gc_content=L.GC, tree="auto", **kw)
        assert len(out) == 5 and out[0].shape == (2, 1, LONG_N) and out[4].tolist() == [0]
        seqs = out[0].cpu().numpy()
        gc = (seqs >= 2).sum(axis=2)
        assert np.array_equal(gc, out[3].cpu().numpy()) and ((gc >= lo) & (gc <= hi)).all(), gc
        glob = model.design(x, mask, n_samples=2, temperature=1.0, seed=3, gc_content=L.GC, tree="global", **kw)
        assert all(_bytes(a) == _bytes(b) for a, b in zip(out, glob))
        with pytest.raises(NotImplementedError, match=r"rnampnn_design_gc: T = \d+ needs \d+ bytes of LDS for the count tree, the limit is 163840 \(T <= 1017\)"):
            model.design(x, mask, n_samples=2, temperature=1.0, seed=3, gc_content=L.GC, **kw)
        prof = model.design_profile(x, mask, temperature=1.0, gc_content=L.GC, tree="auto", **kw)
        assert prof.mode == "gc_content" and prof.miss.tolist() == [0]
        assert np.allclose(prof.marginals.cpu().numpy()[0].sum(axis=1), 1.0, atol=1e-9)


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_designs_a_1300_nt_rna_with_tree_auto(family, tmp_path):
    import __graft_entry__ as g
    g.build()
    import predict as P
    _write_data(tmp_path / "data", ["long0"], [LONG_N])
    ck = str(tmp_path / "model.pt")
    torch.manual_seed(0)
    if family == "rnampnn":
        from rnampnn.model.rnampnn import RNAMPNN
        from rnampnn.utils.train import save_checkpoint
        save_checkpoint(ck, RNAMPNN(precision="f32", **dict(SMALL, padding_len=LONG_PADDING)))
    else:
        from rdesign.model.rdesign import RNAModel
        from rdesign.utils.train import save_checkpoint
        save_checkpoint(ck, RNAModel(num_mpnn_layers=1))
    des = str(tmp_path / "designs.csv")
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--samples", "2", "--temperature", "1.0",
              "--gc-content", "0.45:0.60", "--designs-out", des]
    P.run(P.parse(common + ["--tree", "auto"]), log=lambda *a: None)
    d = list(csv.reader(open(des)))
    assert d[0][-2:] == ["gc", "gc_miss"] and len(d) == 1 + 2
    for row in d[1:]:
        frac = sum(ch in "CG" for ch in row[2]) / LONG_N
        assert row[0] == "long0" and len(row[2]) == LONG_N and row[-1] == "0" and 0.45 <= frac <= 0.60, row[:2]
    with pytest.raises(NotImplementedError, match=r"rnampnn_design_gc: T = \d+ needs \d+ bytes of LDS for the count tree, the limit is 163840 \(T <= 1017\)"):
        P.run(P.parse(common), log=lambda *a: None)
