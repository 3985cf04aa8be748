"""The device-side fit of the gradient-boosted-tree read-out (`rnampnn_gbdt_fit`, csrc/gbdt_fit.hip) against its
numpy restatement `tests/_gbdt_fit_ref.py`.  PARITY UNPINNED against XGBoost (not installed, no XGBoost-produced fixture): the restatement
and the device follow the same written algorithm, whose tree growth is integer / fp64 arithmetic, so the comparisons are EXACT.

Every GPU case runs under a deadline of its own (`_deadline`): a watchdog that ends the process if the case hangs, since a hung GPU call
cannot be interrupted from Python.  The device parts were measured on an MI355X (each case states its time); 3x any of them is below
6 s, so every deadline is the floor of 30 s that the first use of the runtime in a process (code-object load, first allocations: 0.6 s
measured) and a busy box leave room for.  The numpy restatement runs OUTSIDE the deadlines (15 s at the largest case)."""
import contextlib
import ctypes as C
import faulthandler
import json
import os
import re
import time

import numpy as np
import pytest
import torch

import _gbdt_fit_ref as ref
from oracle import gbdt_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAY_KEYS = ("tree_offsets", "tree_class", "left_children", "right_children", "split_indices", "split_conditions", "default_left")
DEADLINE = 30
NEW_SYMBOLS = ("rnampnn_gbdt_fit", "rnampnn_gbdt_export", "rnampnn_gbdt_bin", "rnampnn_gbdt_grow_tree")


@contextlib.contextmanager
def _deadline(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True)
    t0 = time.perf_counter()
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()
        print(f"[deadline {seconds} s] took {time.perf_counter() - t0:.2f} s")


def make_task(n, f, seed, num_class=4):
    """Seeded rows whose label depends on a few features plus noise (learnable, not separable)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, f).astype(np.float32)
    s0 = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.4 * rs.randn(n)
    s1 = X[:, 3] - 0.7 * X[:, min(5, f - 1)] + 0.4 * rs.randn(n)
    y = ((s0 > 0).astype(np.int32) + 2 * (s1 > 0.3).astype(np.int32)) % num_class
    return X, y.astype(np.int32)


def assert_same_model(a, b):
    for k in ("num_class", "num_feature"):
        assert int(a[k]) == int(b[k]), k
    assert np.float32(a["base_score"]) == np.float32(b["base_score"])
    for k in ARRAY_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)             # bitwise
        if not np.array_equal(x, y):
            i = int(np.flatnonzero(x != y)[0])
            t = int(np.searchsorted(np.asarray(a["tree_offsets"]), i, side="right") - 1) if k not in ("tree_offsets", "tree_class") else i
            raise AssertionError(f"{k} differs first at index {i} (tree {t}): {np.asarray(a[k])[i]!r} vs {np.asarray(b[k])[i]!r}")


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_restatement_on_a_hand_made_case():
    """One feature, four rows, one round, depth 1, two classes.  Cuts: v = [0,1,2,3], candidates v[floor(i*4/256)] = 0,1,2,3 -> {1,2,3}
    (0 = v[0] dropped), bins [0,1,2,3].  Margins 0.5/0.5 -> p = 0.5: class 0 has g = [-.5,-.5,.5,.5], h = .5 each; lambda = 1.
    Cut 0 (x < 1): HL = 0.5 < min_child_weight = 1, inadmissible; cut 2: HR = 0.5, inadmissible; cut 1 (x < 2): GL = -1, HL = 1, GR = 1,
    HR = 1, G = 0, H = 2 -> gain = 0.5 * (1/2 + 1/2 - 0) = 0.5.  Leaves: left = 0.1 * -(-1)/(1+1) = 0.05, right = -0.05; class 1 mirrored."""
    X = np.array([[0.0], [1.0], [2.0], [3.0]], np.float32)
    y = np.array([0, 0, 1, 1], np.int32)
    cuts, n_cuts = ref.make_cuts(X)
    assert n_cuts.tolist() == [3] and cuts[0, :3].tolist() == [1.0, 2.0, 3.0]
    bins = ref.bin_matrix(X, cuts, n_cuts)
    assert bins[:, 0].tolist() == [0, 1, 2, 3]
    g, h = ref.gradients(np.full((4, 2), 0.5, np.float32), y)
    assert g[0].tolist() == [-524288, -524288, 524288, 524288] and h[0].tolist() == [524288] * 4
    trace = []
    tree, leaf = ref.grow_tree(bins, cuts, n_cuts, g[0], h[0], None, None, max_depth=1, learning_rate=0.1, trace=trace)
    assert trace == [(0, 0, 2 << 20, 0.5, 0, 1)]
    # with min_child_weight = 0 the outer cuts are admissible too: gain = 0.5 * (0.25/1.5 + 0.25/2.5) = 2/15 < 0.5, the split stays
    tr0 = []
    ref.grow_tree(bins, cuts, n_cuts, g[0], h[0], None, None, max_depth=1, learning_rate=0.1, min_child_weight=0.0, trace=tr0)
    assert tr0 == trace
    a, margins = ref.fit(X, y, num_class=2, n_estimators=1, max_depth=1, learning_rate=0.1, subsample=1.0, colsample_bytree=1.0)
    lo, hi = np.float32(0.1 * (-1.0 / 2.0)), np.float32(0.1 * (1.0 / 2.0))       # -0.05 / +0.05 as the fp64 product rounded to f32
    assert lo == np.float32(-0.05) and hi == np.float32(0.05)
    assert a["tree_offsets"].tolist() == [0, 3, 6] and a["tree_class"].tolist() == [0, 1]
    assert a["left_children"].tolist() == [1, -1, -1] * 2 and a["right_children"].tolist() == [2, -1, -1] * 2
    assert a["split_indices"].tolist() == [0] * 6 and a["default_left"].tolist() == [0] * 6
    assert a["split_conditions"].tolist() == [2.0, hi, lo, 2.0, lo, hi]
    half = np.float32(0.5)
    assert margins[:, 0].tolist() == [half + hi, half + hi, half + lo, half + lo]
    assert margins[:, 1].tolist() == [half + lo, half + lo, half + hi, half + hi]


def test_restatement_margins_equal_oracle_prediction_of_its_export():
    """Pins the cut / bin / `<` convention: walking the exported trees on the raw floats (x < split_condition) lands every training
    row in the leaf the binned growth put it in, so the margins agree bit for bit."""
    X, y = make_task(300, 12, seed=3)
    X[:, 7] = np.round(X[:, 7])                   # few distinct values, many rows equal to a cut
    X[:, 9] = 1.5                                 # constant: no cuts, never split on
    a, margins = ref.fit(X, y, n_estimators=3, max_depth=4, seed=11)
    pred, om = gbdt_oracle.predict(a, X)
    assert np.array_equal(om.view(np.uint32), margins.view(np.uint32))
    assert not np.any(a["split_indices"][a["left_children"] >= 0] == 9)
    assert (pred == y).mean() > np.bincount(y).max() / len(y)


def test_json_round_trip_is_the_identity(tmp_path):
    from rnampnn.model.xgb import parse_xgboost_json, to_xgboost_json
    X, y = make_task(200, 8, seed=5)
    a, _ = ref.fit(X, y, n_estimators=2, max_depth=3, seed=1, base_score=0.3)
    path = tmp_path / "m.json"
    path.write_text(json.dumps(to_xgboost_json(a)))
    b = parse_xgboost_json(str(path))
    assert_same_model(a, b)
    for k in ARRAY_KEYS:
        assert b[k].dtype == a[k].dtype, k


def test_torch_cuts_equal_the_restatement():
    """`quantile_cuts` (torch, the plumbing the device fit takes its cuts from) against `make_cuts`, here on the CPU."""
    from rnampnn.model.xgb import quantile_cuts
    X, _ = make_task(777, 10, seed=8)
    X[:, 2] = np.round(X[:, 2] * 2)
    X[:, 4] = -3.0
    for max_bin in (256, 16):
        c, n = ref.make_cuts(X, max_bin)
        ct, nt = quantile_cuts(torch.from_numpy(X), max_bin)
        assert np.array_equal(n, nt.numpy()) and np.array_equal(c.view(np.uint32), ct.numpy().view(np.uint32))


def test_header_declares_and_native_resolves_the_fit_entry_points():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rnampnn_hip.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/rnampnn_hip.h"
        assert name in _native.SYMBOLS and hasattr(lib, name), name
    assert "rnampnn_gbdt_params" in text


def test_fit_has_no_cpu_fallback():
    from rnampnn.model.xgb import GBDTReadout
    with pytest.raises(RuntimeError):
        GBDTReadout.fit(torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64), n_estimators=1, max_depth=1)


# ------------------------------------------------------------------------------------------------------------------- GPU
def _params(**kw):
    from rnampnn import _native
    p = dict(ref.DEFAULTS); p.update(kw)
    return _native.GbdtParams(**{k: (int(v) if k in ("num_class", "n_estimators", "max_depth", "max_bin", "seed") else float(v)) for k, v in p.items()})


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_bins(X, cuts, n_cuts, ldx=None):
    from rnampnn import _native
    n, f = X.shape
    xd = _dev(X)
    if ldx is not None:
        wide = torch.full((n, ldx), float("nan"), device="cuda")
        wide[:, :f] = xd
        xd = wide
    cd, nd = _dev(cuts), _dev(n_cuts)
    out = torch.zeros(n, f, dtype=torch.uint8, device="cuda")
    rc = _native.lib().rnampnn_gbdt_bin(C.c_void_p(xd.data_ptr()), n, int(xd.stride(0)), f, C.c_void_p(cd.data_ptr()), C.c_void_p(nd.data_ptr()),
                                        C.c_void_p(out.data_ptr()), None)
    assert rc == 0, _native.lib().rnampnn_gbdt_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_tree(bins, cuts, n_cuts, g, h, rmask, fmask, **kw):
    from rnampnn import _native
    p = _params(**kw)
    n, f = bins.shape
    cap = (1 << (p.max_depth + 1)) - 1
    bd, cd, nd, gd, hd = _dev(bins), _dev(cuts), _dev(n_cuts), _dev(g.astype(np.int32)), _dev(h.astype(np.int32))
    rm = _dev(rmask.astype(np.uint8)) if rmask is not None else None
    fm = _dev(fmask.astype(np.uint8)) if fmask is not None else None
    left, right, idx = (np.zeros(cap, np.int32) for _ in range(3))
    cond, nn = np.zeros(cap, np.float32), C.c_int32()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _native.lib().rnampnn_gbdt_grow_tree(C.byref(p), ptr(bd), n, f, ptr(cd), ptr(nd), ptr(gd), ptr(hd), ptr(rm), ptr(fm),
                                              hp(left), hp(right), hp(idx), hp(cond), C.byref(nn), None)
    assert rc == 0, _native.lib().rnampnn_gbdt_last_error()
    k = nn.value
    return dict(left_children=left[:k], right_children=right[:k], split_indices=idx[:k], split_conditions=cond[:k])


@pytest.mark.gpu
def test_device_bins_equal_the_restatement():
    """Measured: 0.28 s, the start of the runtime in the process included."""
    X, _ = make_task(3000, 20, seed=2)
    X[:, 1] = np.round(X[:, 1])                   # 9 or so distinct values: fewer than max_bin, every row equal to a cut or to v[0]
    X[:, 2] = 0.25                                # constant column: no cuts, every bin 0
    X[:, 3] = np.round(X[:, 3] * 40) / 40         # about 250 distinct values
    cuts, n_cuts = ref.make_cuts(X)
    X[:100, 4] = cuts[4, np.arange(100) % n_cuts[4]]       # values that sit exactly on a cut
    want = ref.bin_matrix(X, cuts, n_cuts)
    assert n_cuts[2] == 0 and n_cuts[1] < 20 and (want[:, 2] == 0).all()
    with _deadline(DEADLINE):
        assert np.array_equal(device_bins(X, cuts, n_cuts), want)
        assert np.array_equal(device_bins(X, cuts, n_cuts, ldx=37), want)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,nfeat,nrows,masks,mcw", [(1, 16, 700, False, 1.0), (3, 16, 700, True, 1.0), (3, 256, 2500, False, 1.0),
                                                        (8, 16, 6000, True, 1.0), (8, 256, 6000, False, 1.0), (8, 256, 6000, True, 1.0),
                                                        (8, 16, 40, False, 0.0)])
def test_device_tree_equals_the_restatement(depth, nfeat, nrows, masks, mcw):
    """Every input is an integer, so any difference is a bug.  The last case has fewer rows (40) than leaves (256).
    Measured: below 0.01 s per case (allocation of the workspace included)."""
    X, y = make_task(nrows, nfeat, seed=depth * 1000 + nfeat)
    X[:, 1] = np.round(X[:, 1])
    cuts, n_cuts = ref.make_cuts(X)
    bins = ref.bin_matrix(X, cuts, n_cuts)
    g, h = ref.gradients(np.full((nrows, 4), 0.5, np.float32) + 0.1 * X[:, :4], y)
    rmask = ref.row_mask(5, 2, nrows, 0.8) if masks else None
    fmask = ref.feature_mask(5, 9, nfeat, 0.8) if masks else None
    kw = dict(max_depth=depth, learning_rate=0.1, reg_lambda=1.0, gamma=0.0, min_child_weight=mcw)
    want, _ = ref.grow_tree(bins, cuts, n_cuts, g[1], h[1], rmask, fmask, **kw)
    with _deadline(DEADLINE):
        got = device_tree(bins, cuts, n_cuts, g[1], h[1], rmask, fmask, **kw)
    n = len(want["left_children"])
    assert depth == 1 or n > 3, "the case grew no tree worth comparing"
    a = ref.assemble([want], [1], 4, nfeat, 0.5)
    b = ref.assemble([got], [1], 4, nfeat, 0.5)
    assert_same_model(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("rounds,depth,nfeat,nrows", [(3, 3, 16, 500), (10, 8, 256, 20000)])
def test_device_fit_equals_the_restatement(rounds, depth, nfeat, nrows):
    """Full fit, subsample = colsample_bytree = 0.8: all seven arrays, leaf values bitwise.  The only legitimate source of a mismatch is
    a fp64 `exp` that differs in its last bit between libm and the device library AND straddles a 2^-20 rounding boundary.
    Measured (device part; the restatement runs outside the deadline): 0.59 s (the first fit of the process) and 0.11 s, against 14.6 s of numpy at the large case."""
    from rnampnn.model.xgb import GBDTReadout
    X, y = make_task(nrows, nfeat, seed=rounds)
    kw = dict(n_estimators=rounds, max_depth=depth, subsample=0.8, colsample_bytree=0.8, seed=17)
    with _deadline(DEADLINE):
        t0 = time.perf_counter()
        model = GBDTReadout.fit(_dev(X), _dev(y), **kw)
        torch.cuda.synchronize()
        dev_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want, margins = ref.fit(X, y, **kw)
    print(f"fit ({rounds}, {depth}, {nfeat}, {nrows}): device {dev_s:.3f} s, numpy restatement {time.perf_counter() - t0:.1f} s")
    assert_same_model(want, model.arrays)
    with _deadline(DEADLINE):
        got_m = model.margins(_dev(X[:400])).cpu().numpy()
    assert np.array_equal(got_m.view(np.uint32), margins[:400].view(np.uint32))


@pytest.mark.gpu
def test_fit_is_reproducible_and_independent_of_ldx():
    """Measured: 0.08 s for the four fits."""
    from rnampnn.model.xgb import GBDTReadout
    X, y = make_task(5000, 40, seed=21)
    kw = dict(n_estimators=4, max_depth=6, subsample=0.8, colsample_bytree=0.8)
    xd, yd = _dev(X), _dev(y)
    wide = torch.zeros(5000, 64, device="cuda")
    wide[:, :40] = xd
    with _deadline(DEADLINE):
        a = GBDTReadout.fit(xd, yd, seed=3, **kw).arrays
        b = GBDTReadout.fit(xd, yd, seed=3, **kw).arrays
        c = GBDTReadout.fit(wide[:, :40], yd, seed=3, **kw).arrays           # same rows, row stride 64
        d = GBDTReadout.fit(xd, yd, seed=4, **kw).arrays
    assert not wide[:, :40].is_contiguous()
    assert_same_model(a, b)
    assert_same_model(a, c)
    for k in ARRAY_KEYS:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert any(a[k].tobytes() != d[k].tobytes() for k in ARRAY_KEYS), "another seed must sample other rows and features"


@pytest.mark.gpu
def test_fitted_handle_predicts_like_the_oracle_on_its_export():
    """The handle `rnampnn_gbdt_fit` returns goes through the existing `rnampnn_gbdt_predict` unchanged.  Measured: 0.01 s."""
    from rnampnn.model.xgb import GBDTReadout
    X, y = make_task(4000, 32, seed=33)
    with _deadline(DEADLINE):
        model = GBDTReadout.fit(_dev(X), _dev(y), n_estimators=6, max_depth=5, seed=2)
        rows = X[::13][:300]
        got_m = model.margins(_dev(rows)).cpu().numpy()
        got_p = model.predict(_dev(rows)).cpu().numpy()
    ref_p, ref_m = gbdt_oracle.predict(model.arrays, rows)
    assert np.array_equal(got_m.view(np.uint32), ref_m.view(np.uint32))
    assert np.array_equal(got_p, ref_p)
    with pytest.raises(ValueError):
        bad = X.copy(); bad[5, 3] = np.inf
        GBDTReadout.fit(_dev(bad), _dev(y), n_estimators=1, max_depth=2)
    with pytest.raises(ValueError):
        GBDTReadout.fit(_dev(X), _dev(y + 3), n_estimators=1, max_depth=2)


@pytest.mark.gpu
def test_reference_shape_fit():
    """150 rounds x 4 classes, depth 8, 256 features, as many rows as one C2 batch has valid nucleotides (256 RNAs of 100-140 nt):
    completes, is reproducible, `score` equals the score recomputed from `predict`, and the held-out half of the task is predicted
    better than its majority class.  No comparison with the restatement at this size (numpy needs minutes).
    Measured: 0.84 s per fit, 1.7 s for the whole device part."""
    from rnampnn.model.xgb import GBDTReadout
    from rnampnn.utils import synth
    _, mask, _ = synth.synth_batch(synth.synth_lengths(256, 100, 140, seed=1))
    n = int(mask.sum())
    assert 256 * 100 <= n <= 256 * 140
    X, y = make_task(2 * n, 256, seed=77)
    xd, yd = _dev(X), _dev(y)
    kw = dict(n_estimators=150, max_depth=8, learning_rate=0.1, subsample=0.8, colsample_bytree=0.8, seed=42)
    with _deadline(DEADLINE):
        t0 = time.perf_counter()
        model = GBDTReadout.fit(xd[:n], yd[:n], **kw)
        torch.cuda.synchronize()
        print(f"reference-shape fit: {n} rows, {time.perf_counter() - t0:.2f} s, {int(model.arrays['tree_offsets'][-1])} nodes")
        again = GBDTReadout.fit(xd[:n], yd[:n], **kw)
        train_score = model.score(xd[:n], yd[:n])
        pred = model.predict(xd[:n]).cpu().numpy()
        held_out = model.score(xd[n:], yd[n:])
    assert len(model.arrays["tree_class"]) == 600 and model.arrays["tree_class"][:5].tolist() == [0, 1, 2, 3, 0]
    for k in ARRAY_KEYS:
        assert model.arrays[k].tobytes() == again.arrays[k].tobytes(), k
    assert train_score == int((pred == y[:n]).sum()) / n
    majority = np.bincount(y[n:]).max() / n
    print(f"train score {train_score:.4f}, held-out score {held_out:.4f}, majority class {majority:.4f}")
    assert held_out > majority


@pytest.mark.gpu
def test_rnampnn_fit_xgb_readout_end_to_end(tmp_path):
    """A small closed-form-weight RNAMPNN: `fit_xgb_readout` on a synthetic batch, then `predict_sequences` takes the tree route; the
    saved JSON loaded into a fresh model gives the same sequences.  Measured: 0.11 s."""
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    lengths = [21, 34, 40, 28, 37]
    coords, mask, labels = synth.synth_batch(lengths, first_index=3)
    hp = dict(num_res_neighbours=8, num_res_mpnn_layers=2, padding_len=40, precision="f32", n_estimators=8, xgb_max_depth=4)

    def make():
        m = RNAMPNN(**hp)
        sd = synth.closed_form_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.cuda().eval()

    model = make()
    c, m, y = torch.from_numpy(coords), torch.from_numpy(mask), torch.from_numpy(labels)
    with _deadline(DEADLINE):
        before = model.predict_sequences(c, m)                      # no tree model yet: the Readout argmax
        score = model.fit_xgb_readout([(y, c, m)], seed=7)
        seqs = model.predict_sequences(c, m)
        emb = model.embedding(c, m)
        pred = model.xgb_readout.predict(emb).cpu().numpy()
        path = tmp_path / "fitted.json"
        model.xgb_readout.save_json(str(path))
        fresh = make()
        fresh.load_xgb_readout(str(path))
        seqs_fresh = fresh.predict_sequences(c, m)
    assert len(model.xgb_readout.arrays["tree_class"]) == 8 * 4 and model.xgb_readout.num_feature == 256
    want = ["".join("AUCG"[i] for i in pred[b][:n]) for b, n in enumerate(lengths)]
    assert seqs == want and seqs != before
    assert seqs_fresh == seqs
    truth = ["".join("AUCG"[i] for i in labels[b][:n]) for b, n in enumerate(lengths)]
    agree = sum(a == b for s, t in zip(seqs, truth) for a, b in zip(s, t)) / sum(lengths)
    assert abs(agree - score) < 1e-12
