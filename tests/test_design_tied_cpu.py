"""Host side of multi-state design (``rnampnn_design_tied``): the float64 restatement itself (its chain draw against brute force, its
reduction to tests/_design_ref.py for one state per group, the keep-two rule on malformed graphs, its near-boundary share on the GPU case),
``read_states_csv``, predict.py's ``--states`` flag, and the ABI entry with its argument errors (no launch happens, so no GPU is needed)."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_ref as R  # noqa: E402
import _design_tied_ref as TR  # noqa: E402


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    return _native


# ---------------------------------------------------------------------------------------------------------------- the chain draw
def brute_joint(z, masks, cyc, wob):
    """{assignment: probability} by enumeration: prod_k exp(z_k(c_k)) over the assignments the masks admit whose edges are all compatible."""
    L = len(masks)
    zmax = [max(z[k][c] for c in range(4) if (masks[k] >> c) & 1) for k in range(L)]
    edges = [(k, k + 1) for k in range(L - 1)] + ([(L - 1, 0)] if cyc else [])
    out = {}
    for asg in itertools.product(*[[c for c in range(4) if (masks[k] >> c) & 1] for k in range(L)]):
        if all((R.COMPAT[wob][asg[i]] >> asg[j]) & 1 for i, j in edges):
            out[asg] = float(np.exp(sum(z[k][asg[k]] - zmax[k] for k in range(L))))
    tot = sum(out.values())
    return {a: v / tot for a, v in out.items()} if tot > 0 else {}


def implied_probability(st, asg):
    """The probability the restatement's procedure gives to ``asg``: the product of the conditionals its draws are made from."""
    p = [1.0]

    def choose(k, cells, w):
        p[0] *= float(w[cells.index(asg[k])] / np.sum(w)) if asg[k] in cells else 0.0
        return asg[k]
    assert TR.sample_chain(st, choose) == list(asg)
    return p[0]


@pytest.mark.parametrize("wob", [True, False])
def test_the_chain_draw_is_the_brute_force_joint(wob):
    """Random paths and even cycles of 3..8 nodes with masks at temperature 0.3: the implied joint equals enumeration to 1e-12, and a
    component is infeasible exactly when enumeration finds no assignment."""
    rng = np.random.default_rng(5 + wob)
    worst, n_inf, n_cyc = 0.0, 0, 0
    for trial in range(60):
        cyc = trial % 2 == 1
        L = int(rng.integers(3, 9))
        if cyc and L % 2:
            L += 1
        z = 3.0 * rng.standard_normal((L, 4)) / 0.3
        masks = [int(rng.choice([15, 15, 15, 15, 9, 6, 8, 3, 1])) for _ in range(L)]
        J = brute_joint(z, masks, cyc, wob)
        st = TR.prepare_chain(z, masks, cyc, wob)
        assert (st is None) == (not J), (trial, L, cyc, masks)
        n_inf += st is None
        n_cyc += cyc and st is not None
        if st is None:
            continue
        total = 0.0
        for asg, pj in J.items():
            p = implied_probability(st, asg)
            worst, total = max(worst, abs(p - pj)), total + p
        assert abs(total - 1.0) <= 1e-12
    print(f"wobble {wob}: worst |implied - brute force| {worst:.3e}; {n_inf} infeasible components, {n_cyc} feasible cycles")
    assert worst <= 1e-12 and n_inf > 0 and n_cyc > 5


def test_an_odd_cycle_is_infeasible_and_a_long_chain_does_not_underflow():
    z = np.zeros((3, 4))
    assert TR.prepare_chain(z, [15, 15, 15], True, True) is None     # the compatibility graph A-U-G-C is bipartite
    assert TR.prepare_chain(z, [15, 15, 15], False, True) is not None
    # 40 nodes at temperature 0.3: relative to the product of the nodes' best classes the partition sum is below the smallest float64
    # (linear forward weights would need the per-step normalisation); the stored lambdas stay at a largest component of 0
    rng = np.random.default_rng(0)
    z = 6.0 * rng.standard_normal((40, 4)) / 0.3
    z[:, 1] -= 40.0; z[:, 3] -= 40.0
    st = TR.prepare_chain(z, [15] * 40, False, True)
    assert st is not None and st["fw"][1] - z[1:].max(axis=1).sum() < -745.0 and all(a.max() == 0.0 for a in st["fw"][0])
    asg = TR.sample_chain(st, lambda k, cells, w: cells[int(np.argmax(w))])
    assert all((R.COMPAT[True][a] >> b) & 1 for a, b in zip(asg[:-1], asg[1:]))


def test_the_cold_limit_of_the_reference_is_the_constrained_argmax():
    """Temperature 1e-3 on the GPU case: exp(z - max) is 0 for every class but one, yet every feasible component stays feasible and draws its
    float64 argmax."""
    import test_design_tied_gpu as G
    h = G.host_case()
    best = G.cold_argmax(h)
    seqs, _, bad, _ = G.host_ref(h, "plain", 1e-3)
    assert bad.tolist() == G.INFEASIBLE
    for (b0, nodes), (asg, lead) in best.items():
        assert lead >= 0.05 and all(seqs[s, b0, list(nodes)].tolist() == asg for s in range(G.S)), (b0, nodes[:4])


# ---------------------------------------------------------------------------------------------------------------- reduction
@pytest.mark.parametrize("variant", ["plain", "global", "perpos"])
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_one_state_per_group_is_the_existing_yardstick(variant, temperature):
    import test_design_gpu as G1
    h, v = G1.host_case(), G1.VARIANTS[variant]
    bias = None if v["bias"] is None else h[v["bias"]]
    want = R.design_ref(h["logits"], G1.LENGTHS, temperature, G1.S, G1.SEED, h["allowed"], h["partner"], v["wobble"], bias)
    got = TR.design_tied_ref(h["logits"], G1.LENGTHS, np.arange(h["B"] + 1), temperature, G1.S, G1.SEED, None, h["allowed"], h["partner"],
                             v["wobble"], bias)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tolist() == want[2].tolist() == G1.INFEASIBLE
    assert not [c for c in got[3].components() if len(c[1]) > 2]
    assert sorted((b, n[0], n[1]) for b, n, kind in got[3].components() if kind == "pair") == sorted(G1.FEASIBLE)


# ---------------------------------------------------------------------------------------------------------------- malformed graphs
def _tiny(M, n, T=16, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, T, 4)).astype(np.float32), np.full((M, T), -1, dtype=np.int32), [n] * M


def test_a_degree_three_node_keeps_its_first_two_neighbours_and_counts_one():
    logits, partner, lengths = _tiny(3, 14)
    for m, j in enumerate((5, 9, 12)):
        partner[m, 0], partner[m, j] = j, 0
    seqs, margin, bad, plan = TR.design_tied_ref(logits, lengths, [0, 3], 1.0, 8, 3, partner=partner)
    assert bad.tolist() == [1, 1, 1]
    # 12 keeps 0, but 0 dropped it: the edge is not live and 12 draws alone
    assert [(n, k) for _, n, k in plan.components() if k != "single"] == [([5, 0, 9], "path")]
    assert all((int(s[0, 5]), int(s[0, 0])) in R.PAIRS[True] and (int(s[0, 0]), int(s[0, 9])) in R.PAIRS[True] for s in seqs)
    assert (seqs[:, 0] == seqs[:, 1]).all() and (seqs[:, 0] == seqs[:, 2]).all() and (seqs[:, :, 14:] == -1).all()
    # the same neighbour in two states is one neighbour: no count, a plain pair
    logits, partner, lengths = _tiny(3, 14)
    for m, j in enumerate((5, 5, 9)):
        partner[m, 0], partner[m, j] = j, 0
    _, _, bad, plan = TR.design_tied_ref(logits, lengths, [0, 3], 1.0, 1, 3, partner=partner)
    assert bad.tolist() == [0, 0, 0] and [(n, k) for _, n, k in plan.components() if k != "single"] == [([5, 0, 9], "path")]


def test_a_length_mismatched_group_uses_the_common_prefix_and_empty_groups_write_nothing():
    logits, partner, _ = _tiny(3, 0)
    partner[0, 2], partner[0, 6] = 6, 2
    partner[1, 3], partner[1, 8] = 8, 3                             # 8 is beyond the common prefix of 7: not a pair
    seqs, margin, bad, plan = TR.design_tied_ref(logits, [10, 7, 5], [0, 2, 2, 9], 1.0, 2, 1, partner=partner)
    assert (seqs[:, :2, :7] >= 0).all() and (seqs[:, :2, 7:] == -1).all() and (seqs[:, 0] == seqs[:, 1]).all()
    assert [(b, n, k) for b, n, k in plan.components() if k != "single"] == [(0, [2, 6], "pair")]
    assert (seqs[:, 2, :5] >= 0).all() and (seqs[:, 2, 5:] == -1).all() and bad.tolist() == [0, 0, 0]     # group_cu is clamped to [0, B]
    assert np.isinf(margin[:, :2, 7:]).all()
    none = TR.design_tied_ref(logits, [10, 7, 5], [0, 2, 1, 1], 1.0, 1, 1)[0]        # a decreasing pair and a repeated value: empty groups
    assert (none[:, 2] == -1).all() and (none[:, :2, :7] >= 0).all()


def test_weights_and_masks_combine_over_the_states():
    logits = np.zeros((2, 4, 4), dtype=np.float32)
    logits[0, :, 0] = 30.0                                          # state 0 wants A everywhere, state 1 wants G
    logits[1, :, 3] = 30.0
    allowed = np.full((2, 4), 15, dtype=np.uint8)
    allowed[0, 1], allowed[1, 1] = 9, 5                            # R and M = A
    allowed[0, 2], allowed[1, 2] = 1, 2                            # A and U = nothing: free, counts 1
    for w, want in (([1.0, 0.5], 0), ([0.5, 1.0], 3), ([1.0, -1.0], 0), ([-1.0, 1.0], 3)):
        seqs, _, bad, _ = TR.design_tied_ref(logits, [4, 4], [0, 2], 1.0, 3, 9, weight=w, allowed=allowed)
        assert (seqs[:, :, [0, 3]] == want).all() and (seqs[:, :, 1] == 0).all() and bad.tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------------------- near-boundary share
@pytest.mark.parametrize("variant", ["global", "perpos"])
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_reference_near_boundary_share_on_the_gpu_case(variant, temperature):
    """The reference's own share of valid positions (a component counts with its worst draw) within NEAR of a cumulative boundary - those
    the GPU test leaves out - is at most 1 %, the NaN state's positions included."""
    import test_design_tied_gpu as G
    h = G.host_case()
    _, margin, bad, _ = G.host_ref(h, variant, temperature)
    valid = np.broadcast_to(G.valid_mask(), margin.shape)
    near = valid & ~(margin > G.NEAR)
    print(f"{variant} temperature {temperature}: {int(near.sum())} of {int(valid.sum())} positions within {G.NEAR} of a boundary or NaN "
          f"({near.sum() / valid.sum():.4%}); {int(np.isnan(margin).sum())} NaN")
    assert G.NEAR == 1e-5 and near.sum() / valid.sum() <= 0.01
    assert bad.tolist() == G.INFEASIBLE and np.isinf(margin[~valid]).all()


def test_the_gpu_case_has_a_cold_lead():
    import test_design_tied_gpu as G
    best = G.cold_argmax(G.host_case())
    assert len(best) == len(G.COMPONENTS) - 1 and min(v[1] for v in best.values()) >= 0.05
    # brute force over the 6-cycle agrees with the max-product used there
    h = G.host_case()
    z = G.group_score(h, 1, 2)[[60, 70, 80, 90, 100, 110]]
    J = brute_joint(z, [15] * 6, True, True)
    assert list(max(J, key=J.get)) == best[(1, (60, 70, 80, 90, 100, 110))][0]


# ---------------------------------------------------------------------------------------------------------------- states file, CLI
def test_read_states_csv_and_its_errors(tmp_path):
    from rnampnn.utils.constraints import read_states_csv
    from rnampnn.utils.predict import group_batches, state_groups
    path = tmp_path / "s.csv"
    path.write_text("design_id,pdb_id,weight\nsw,r2,\nsw,r0,0.5\nnmr,m1,1\nnmr,m2,-0.25\n")
    table = read_states_csv(str(path))
    assert table == {"sw": [("r2", 1.0), ("r0", 0.5)], "nmr": [("m1", 1.0), ("m2", -0.25)]} and list(table) == ["sw", "nmr"]
    (tmp_path / "twice.csv").write_text("design_id,pdb_id,weight\nsw,r2,\nother,r2,\n")
    with pytest.raises(ValueError, match="r2"):
        read_states_csv(str(tmp_path / "twice.csv"))
    (tmp_path / "col.csv").write_text("design_id,pdb_id\nsw,r2\n")
    with pytest.raises(ValueError, match="weight"):
        read_states_csv(str(tmp_path / "col.csv"))
    (tmp_path / "num.csv").write_text("design_id,pdb_id,weight\nsw,r2,abc\n")
    with pytest.raises(ValueError, match="abc"):
        read_states_csv(str(tmp_path / "num.csv"))
    ids, lengths = ["m1", "m2", "r0", "r1", "r2"], [20, 20, 33, 41, 33]
    groups = state_groups(table, ids, lengths)
    assert groups == [("nmr", [0, 1], [1.0, -0.25]), ("r1", [3], [1.0]), ("sw", [4, 2], [1.0, 0.5])]
    assert group_batches(groups, lengths, 3, 1 << 30) == [[0], [2, 1]] and group_batches(groups, lengths, 1, 1 << 30) == [[0], [2], [1]]
    assert group_batches(groups, lengths, 8, 70) == [[0], [2], [1]]
    with pytest.raises(ValueError, match="sw"):
        state_groups(table, ids, [20, 20, 33, 41, 30])
    with pytest.raises(ValueError, match="m2"):
        state_groups(table, ["m1", "r0", "r1", "r2"], [20, 33, 41, 33])
    with pytest.raises(ValueError, match="r1"):
        state_groups({"r1": [("r0", 1.0)]}, ids, lengths)


def test_predict_parses_the_states_flag(tmp_path):
    import predict
    p = predict.parse(["--ckpt", "x.pt", "--data", "d"])
    assert p.states is None and predict.design_options(p) == {}
    p = predict.parse(["--ckpt", "x.pt", "--data", "d", "--samples", "2", "--states", "s.csv"])
    assert p.states == "s.csv" and predict.design_options(p) == {}


def test_state_lengths_are_checked_on_the_host():
    from rnampnn.model.rnampnn import check_state_lengths
    check_state_lengths([2, 1, 0], [7, 7, 9])
    with pytest.raises(ValueError, match="group 1"):
        check_state_lengths([1, 2], [7, 7, 9])
    with pytest.raises(ValueError, match="sum to B"):
        check_state_lengths([1, 1], [7, 7, 9])


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_rnampnn_design_tied(native):
    text = open(os.path.join(REPO, "include", "rnampnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+rnampnn_design_tied\s*\(([^;]*)\)\s*;", text)
    assert m, "include/rnampnn_hip.h does not declare rnampnn_design_tied"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert "rnampnn_design_tied" in native.SYMBOLS and len(native.SYMBOLS["rnampnn_design_tied"][1]) == n_params == 22
    assert hasattr(native.lib(), "rnampnn_design_tied")
    import __graft_entry__ as g
    assert "design_tied.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_tied.hip")) and "design_dev.h" in g.HEADERS


def _call(native, **kw):
    """rnampnn_design_tied with made-up (never dereferenced) addresses: every case below must return before a launch."""
    a = dict(logits=0x1000, n_rows=64, mask=0x2000, cu=None, B=2, T=8, group_cu=0x7000, G=1, weight=None, temperature=1.0, S=4, seed=1,
             seed_dev=None, allowed=None, partner=None, wobble=1, bias=None, per_position=0, seqs=0x3000, seq_nll=0x4000, infeasible=0x5000)
    a.update(kw)
    vp = lambda v: None if v is None else C.c_void_p(v)
    return native.lib().rnampnn_design_tied(vp(a["logits"]), a["n_rows"], vp(a["mask"]), vp(a["cu"]), a["B"], a["T"], vp(a["group_cu"]), a["G"],
                                            vp(a["weight"]), a["temperature"], a["S"], C.c_uint64(a["seed"]), vp(a["seed_dev"]),
                                            vp(a["allowed"]), vp(a["partner"]), a["wobble"], vp(a["bias"]), a["per_position"], vp(a["seqs"]),
                                            vp(a["seq_nll"]), vp(a["infeasible"]), None)


@pytest.mark.parametrize("kw, text", [
    (dict(group_cu=None), "null group_cu"), (dict(G=0), "G = 0"), (dict(G=-2), "G = -2"),
    (dict(logits=None), "null logits"),
    (dict(B=0), "empty batch"), (dict(B=-3), "empty batch"), (dict(T=0), "empty batch"),
    (dict(S=0), "S = 0"), (dict(S=-1), "S = -1"),
    (dict(S=65535), "at most 65534"),
    (dict(mask=None, cu=None), "exactly one of mask"), (dict(cu=0x6000), "exactly one of mask"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("inf")), "temperature"), (dict(temperature=float("nan")), "temperature"),
    (dict(logits=0x1004), "16-byte aligned"), (dict(bias=0x8004, per_position=1), "16-byte aligned"),
    (dict(mask=None, cu=0x6000, n_rows=-1), "negative row count"),
])
def test_argument_errors_are_value_errors_before_any_launch(native, kw, text):
    rc = _call(native, **kw)
    assert rc == native.ERR_BAD_ARG
    with pytest.raises(ValueError, match=text):
        native.check(rc)


def test_a_call_with_every_output_null_returns_ok_without_a_launch(native):
    assert _call(native, seqs=None, seq_nll=None, infeasible=None) == 0
    assert _call(native, S=65534, T=100000, partner=0x9000, seqs=None, seq_nll=None, infeasible=None) == 0


def test_an_extent_beyond_the_lds_is_unsupported_and_names_the_limit(native):
    rc = _call(native, T=5000, partner=0x9000)
    assert rc == native.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match=r"limit is 163840 \(T <= 4962"):
        native.check(rc)


def test_design_from_logits_refuses_host_logits_and_bad_states(native):
    import torch
    from rnampnn.model.rnampnn import design_from_logits
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        design_from_logits(torch.zeros(2, 4, 4), mask=torch.ones(2, 4), n_samples=1, temperature=1.0, seed=0, states=[2])
