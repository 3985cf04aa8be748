"""The coordinate front end of the forward - geometry records (`k_geom`) and the k-NN graph (`k_knn_queue`) - on the bf16 path at k = 30.

What is pinned, always by equality (neighbour lists are integers, and logits are compared as bytes):
  * single RNAs of n = 1, 2, 17, 30, 31, 33, 64, 65, 144, 145, 256 residues (no neighbour at all; n <= k with the phantom slot; exactly k real
    neighbours; the first key that lands on a lane's second queue slot; both sides of the NK = 4 / 9 / 16 instantiations), each as a call of
    its own (T = n) and as a shard of a longer batch (T_norm > T);
  * a batch of {5, 140, 31, 128, 129} residues in padded and in packed form: every RNA's list and logits are what the RNA gives alone;
  * the lists equal the oracle's (`O.knn_graph`).  The tie-free inputs are drawn so that no two distances of a row are closer than 1.1e-4
    relative; the test asserts > 1e-4 on the coordinates it uses, so the f32 rounding of a centroid (1e-7) cannot reorder a row;
  * exact ties, lower index first: the committed tie fixtures of tests/test_knn_ties_gpu.py, integer lattices and duplicated points (their
    centroids, squared distances and therefore distance bits are exact in f32, on the device and in the oracle alike);
  * a workspace painted 0xFF, `stop_after = 1`, and the stage entry points (`launch_geom` + `launch_knn` behind `raw_edge_features`) give
    the lists of the whole forward."""
import os

import numpy as np
import pytest
import torch

from _tap_oracle import TIE_FIXTURES, load_fixture

pytestmark = pytest.mark.gpu

K = 30
P = 264                                   # padding_len: every T and T_norm used here
SINGLES = [1, 2, 17, 30, 31, 33, 64, 65, 144, 145, 256]
BATCH = [5, 140, 31, 128, 129]
GAP = 1e-4                                # asserted; the draw keeps MARGIN (in the logarithm)
MARGIN = 1.1e-4
SEED = 20
# atom offsets around a residue's centre (integers that sum to zero: a lattice point stays the exact centroid)
TEMPLATE = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1], [0, 0, 0]], np.float64)

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------------------------------------ inputs (CPU)
def centroid_dist(res):
    """(n, 7, 3) f32 -> (n, n) f64 distances of the centroids, sqrt(|.|^2 + 1e-6), diagonal +inf."""
    c = res.astype(np.float64).mean(1)
    d = np.sqrt(((c[:, None] - c[None]) ** 2).sum(-1) + 1e-6)
    np.fill_diagonal(d, np.inf)
    return d


def min_rel_gap(res):
    """Smallest (b - a) / a over neighbouring distances a <= b of one row; +inf where a row has fewer than two."""
    if res.shape[0] < 3:
        return np.inf
    s = np.sort(centroid_dist(res), axis=1)[:, :-1]
    return float(((s[:, 1:] - s[:, :-1]) / s[:, :-1]).min())


CLOUD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coord_front", "tie_free_cloud256.npy")


def draw_tie_free_cloud():
    """How tests/golden/coord_front/tie_free_cloud256.npy was drawn (a minute and a half of rejection sampling, so the result is committed and
    this is not run by the tests): 256 residues (256, 7, 3) f32, a branching walk; a residue is accepted only if its distance to every
    accepted one keeps MARGIN (in the logarithm) from every other distance of both rows."""
    rng = np.random.default_rng(SEED)
    res = np.zeros((256, 7, 3), np.float32)
    cen = np.zeros((256, 3))
    logd = np.full((256, 256), np.inf)
    m = 0
    while m < 256:
        step = rng.normal(size=3)
        base = cen[rng.integers(m)] if m else np.zeros(3)
        r = ((base + step * (rng.uniform(4.0, 9.0) / np.linalg.norm(step)))[None] + 1.3 * TEMPLATE + 0.15 * rng.normal(size=(7, 3))).astype(np.float32)
        c = r.astype(np.float64).mean(0)
        if m:
            d = np.sqrt(((cen[:m] - c) ** 2).sum(1) + 1e-6)
            ld = np.log(d)
            if d.min() < 3.0 or (m > 1 and np.diff(np.sort(ld)).min() <= MARGIN) or np.abs(logd[:m, :m] - ld[:, None]).min() <= MARGIN:
                continue
            logd[:m, m] = logd[m, :m] = ld
        res[m], cen[m] = r, c
        m += 1
    return res


def tie_free_cloud():
    """The committed draw.  Any subset of its residues, in any order, keeps the property; every test asserts it on what it uses."""
    return cached("cloud", lambda: np.load(CLOUD))


def rna(n, r=0):
    """n residues of the cloud: a different, rotated selection for every r, so that no two RNAs of a batch share a coordinate."""
    return tie_free_cloud()[np.roll(np.arange(256), -37 * r)[:n]]


def padded(rnas, T):
    coords = np.zeros((len(rnas), T, 7, 3), np.float32)
    mask = np.zeros((len(rnas), T), np.float32)
    for b, x in enumerate(rnas):
        coords[b, :len(x)], mask[b, :len(x)] = x, 1
    return torch.from_numpy(coords), torch.from_numpy(mask)


def oracle_lists(coords, mask, T_norm, k=K):
    """`O.knn_graph` of the batch padded to max(T, T_norm) - what the call stands for - cut back to the T rows the call returns."""
    from oracle import rnampnn_oracle as O
    B, T = mask.shape
    Tp = max(T, T_norm)
    c, m = torch.zeros(B, Tp, 7, 3), torch.zeros(B, Tp)
    c[:, :T], m[:, :T] = coords, mask
    return O.knn_graph(c, m, k)[:, :T]


def lattice(nx, ny, nz, step=2.0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * step
    return (g[:, None] + TEMPLATE[None]).astype(np.float32)


TIE_INPUTS = {"lattice_4x4x4": lambda: lattice(4, 4, 4), "lattice_5x5x5": lambda: lattice(5, 5, 5), "lattice_6x5x5": lambda: lattice(6, 5, 5),
              "line_17": lambda: lattice(17, 1, 1), "duplicates_34": lambda: np.repeat(lattice(17, 1, 1), 2, 0),
              "duplicates_3x50": lambda: np.tile(lattice(5, 5, 2), (3, 1, 1))}


# ------------------------------------------------------------------------------------------------ the device side
def model(k=K, L=1):
    def make():
        from rnampnn.model._schema import DEFAULT_HPARAMS, state_dict_shapes
        from test_hip_parity import _model
        hp = dict(DEFAULT_HPARAMS, num_res_neighbours=k, padding_len=P, num_res_mpnn_layers=L)
        return _model(hp, state_dict_shapes(hp), "bf16")[0]
    return cached(("model", k, L), make)


def tob(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def forward(m, coords, mask, T_norm=0):
    """Whole forward with the graph tap -> (edge_index CPU, logits bytes)."""
    out = m.forward_taps(coords, mask, ["edge_index"], T_norm=T_norm)
    return out["edge_index"].cpu(), tob(out["logits"])


def lists_stop_after_1(m, coords, mask, T_norm=0):
    return m._run(coords, mask, want_logits=False, T_norm=T_norm, taps=dict(names=("edge_index",), stop_after=1))["edge_index"].cpu()


def lists_stage(m, coords, mask, T_norm=0):
    """`launch_geom` + `launch_knn` as separate launches (the stage entry point has no T_norm: the input is padded to it instead)."""
    B, T = mask.shape
    Tp = max(T, T_norm)
    c, mk = torch.zeros(B, Tp, 7, 3), torch.zeros(B, Tp)
    c[:, :T], mk[:, :T] = coords, mask
    return m.raw_edge_features(c, mk)[1].cpu()[:, :T]


def check_all_forms(m, coords, mask, T_norm, k=K):
    """The whole forward against the oracle, a 0xFF workspace, stop_after = 1 and the stage entry points -> (lists, logits bytes)."""
    want = oracle_lists(coords, mask, T_norm, k)
    idx, logits = forward(m, coords, mask, T_norm)
    assert torch.equal(idx, want), "forward: lists differ from the oracle's"
    m._ws.fill_(0xFF)
    idx_ff, logits_ff = forward(m, coords, mask, T_norm)
    assert torch.equal(idx_ff, idx) and logits_ff == logits, "a workspace painted 0xFF changed the result"
    assert np.isfinite(np.frombuffer(logits, np.float32)).all()
    assert torch.equal(lists_stop_after_1(m, coords, mask, T_norm), idx), "stop_after = 1 returns other lists"
    assert torch.equal(lists_stage(m, coords, mask, T_norm), idx), "launch_geom + launch_knn return other lists"
    return idx, logits


# ------------------------------------------------------------------------------------------------ tests
def test_the_drawn_coordinates_are_tie_free():
    """CPU check of the inputs of every oracle comparison below (fails, never skips)."""
    for n in SINGLES:
        g = min_rel_gap(rna(n))
        assert g > GAP, f"n = {n}: smallest relative gap {g:.2e} of two distances of a row"
    for r, n in enumerate(BATCH):
        g = min_rel_gap(rna(n, r + 1))
        assert g > GAP, f"batch RNA {r} (n = {n}): smallest relative gap {g:.2e}"


@pytest.mark.parametrize("shard", [False, True], ids=["T_eq_n", "T_norm_gt_T"])
@pytest.mark.parametrize("n", SINGLES)
def test_single_rna(n, shard):
    x = rna(n)
    assert min_rel_gap(x) > GAP
    coords, mask = padded([x], n)
    T_norm = n + 3 if shard else 0
    idx, _ = check_all_forms(model(), coords, mask, T_norm)
    # the cases the lengths stand for
    real = min(K, n - 1)
    assert (idx[0, :, :real] >= 0).all() and (idx[0, :, :real] < n).all()
    if real < K:
        assert (idx[0, :, real] == (n if shard else -1)).all() and (idx[0, :, real + 1:] == -1).all()


def alone(r, n, T):
    """RNA r as a batch of one, padded to the batch's T like every RNA of the batch (the kernels behind the graph are chosen by T)."""
    def make():
        coords, mask = padded([rna(n, r + 1)], T)
        idx, logits = forward(model(), coords, mask)
        return idx[:, :n], np.frombuffer(logits, np.float32).reshape(T, 4)[:n].tobytes()
    return cached(("alone", r, n, T), make)


@pytest.mark.parametrize("form", ["padded", "packed"])
def test_batch_equals_every_rna_alone(form):
    T = max(BATCH)
    rnas = [rna(n, r + 1) for r, n in enumerate(BATCH)]
    for x in rnas:
        assert min_rel_gap(x) > GAP
    coords, mask = padded(rnas, T)
    m = model()
    if form == "padded":
        idx, logits = check_all_forms(m, coords, mask, 0)
        logits = np.frombuffer(logits, np.float32).reshape(len(BATCH), T, 4)
        for r, n in enumerate(BATCH):
            a_idx, a_logits = alone(r, n, T)
            assert torch.equal(idx[r, :n], a_idx[0]), f"RNA {r} (n = {n}): lists in the batch differ from the RNA alone"
            assert (idx[r, n:] == -1).all()
            assert logits[r, :n].tobytes() == a_logits, f"RNA {r} (n = {n}): logits in the batch differ from the RNA alone"
    else:
        packed = coords[mask == 1].contiguous()
        cu = torch.tensor([0] + list(np.cumsum(BATCH)), dtype=torch.int32)
        rows = m.forward_packed(packed, cu, max_len=T).cpu().numpy()
        m._ws.fill_(0xFF)
        assert m.forward_packed(packed, cu, max_len=T).cpu().numpy().tobytes() == rows.tobytes()
        for r, n in enumerate(BATCH):
            assert rows[int(cu[r]):int(cu[r + 1])].tobytes() == alone(r, n, T)[1], f"RNA {r} (n = {n}): packed logits differ from the RNA alone"


@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_committed_tie_fixtures(name):
    from oracle import rnampnn_oracle as O
    arrs, hp, _ = load_fixture("rnampnn_ties", name)
    k = int(hp["num_res_neighbours"])
    assert int(hp["padding_len"]) <= P
    coords, mask = torch.from_numpy(arrs["coords"]), torch.from_numpy(arrs["mask"])
    idx, _ = check_all_forms(model(k), coords, mask, 0, k)
    assert O.edge_index_in_class(torch.from_numpy(arrs["edge_index"]).long(), idx, mask, k)


@pytest.mark.parametrize("shard", [False, True], ids=["T_eq_n", "T_norm_gt_T"])
@pytest.mark.parametrize("name", list(TIE_INPUTS))
def test_exact_ties_lower_index_first(name, shard):
    x = TIE_INPUTS[name]()
    n = x.shape[0]
    d = centroid_dist(x)
    assert (np.sort(d, 1)[:, :-2] == np.sort(d, 1)[:, 1:-1]).any(), "the input has no tie"
    coords, mask = padded([x], n)
    idx, _ = check_all_forms(model(), coords, mask, n + 2 if shard else 0)
    # lower index first, checked without the oracle: along a row the (distance, index) pairs ascend
    real = min(K, n - 1)
    j = idx[0, :, :real].numpy()
    dj = np.take_along_axis(d, j, 1)
    assert ((dj[:, 1:] > dj[:, :-1]) | ((dj[:, 1:] == dj[:, :-1]) & (j[:, 1:] > j[:, :-1]))).all()
