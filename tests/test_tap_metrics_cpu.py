"""The per-layer h / e taps on the CPU: the oracle pinned to the reference's own modules at every ResMPNN layer, and the yardstick of
test_mpnn_taps_gpu.py - the error of bf16 autocast in the tap metrics of ``_tap_metrics`` - with its control.

Why taps: at the closed-form weights the logits barely depend on the ten ResMPNN layers (|h_post| <= 0.14 next to |raw_emb| <= 3.7 in the
embedding), so an output channel of an edge MLP routed to the wrong place moves the logits by 3e-5, below every logit bound of the suite,
and the h taps by less than their own bf16 noise.  Only the e tap of that layer, per channel, shows it (``test_swapped_channels_*``)."""
import numpy as np
import pytest
import torch

from _tap_metrics import MIN_ROWS_FOR_CH, tap_error, tap_error_padded, valid_rows
from _tap_oracle import closed_form_sd, load_fixture, oracle_runs, run_oracle, swapped
from oracle import rnampnn_oracle as O
from rnampnn.utils import synth

CASE_A = dict(lens=[40, 37, 33, 12], first_index=700, k=30, layers=(1, 2, 5, 10))
# bf16 autocast against plain f32, measured with the REFERENCE's modules (tools/gen_golden.py: RefComposite) over four configurations - this
# one, 3 layers, k = 4 with the one-Linear edge update, k = 32: (low, high) of every figure; the oracle must sit in 0.5 x low .. 2 x high.
REF_AUTOCAST = {"e": dict(max_ch=(0.023, 0.032), med_ch=(0.011, 0.011), max_row=(0.009, 0.014)),
                "h": dict(max_ch=(0.022, 0.039), max_row=(0.022, 0.024))}
REF_AUTOCAST_E_ABSMAX = 0.25          # "up to", at |e| up to 17


# ------------------------------------------------------------------------------------------------ the metric itself
def test_metric_on_constructed_errors():
    rng = np.random.default_rng(0)
    R = rng.standard_normal((400, 128)) * np.linspace(0.5, 2.0, 128)
    assert tap_error(R, R).absmax == 0 and tap_error(R, R).max_ch == 0
    G = R.copy(); G[:, [5, 77]] = G[:, [77, 5]]                    # two channels exchanged: ~ sqrt(2) of their rms, nothing elsewhere
    t = tap_error(G, R)
    assert t.worst_ch in (5, 77) and t.max_ch > 1.0 and t.med_ch == 0 and t.ch_ok
    assert t.max_row < t.max_ch / 4                                # ... two of 128 channels: diluted in a row
    G = R.copy(); G[[17]] = R[[18]]                                # one row taken from its neighbour
    t = tap_error(G, R)
    assert t.worst_row == 17 and t.max_row > 1.0 and t.med_row == 0 and t.max_ch < 0.2
    G = R * 1.01
    t = tap_error(G, R)
    assert abs(t.max_ch - 0.01) < 1e-12 and abs(t.max_row - 0.01) < 1e-12 and abs(t.med_ch - 0.01) < 1e-12
    Rq = R.copy(); Rq[:, 3] *= 1e-6                                # a nearly silent channel: the floor, a quarter of the median rms, applies
    t = tap_error(Rq + 1e-3, Rq)
    assert t.max_ch < 1e-3 / (0.25 * 0.5) and t.max_ch == pytest.approx(1e-3 / (0.25 * np.median(np.sqrt((Rq * Rq).mean(0)))))
    assert not tap_error(R[:MIN_ROWS_FOR_CH - 1], R[:MIN_ROWS_FOR_CH - 1]).ch_ok


def test_valid_rows_selects_edges_of_valid_residues():
    e = np.arange(2 * 3 * 2 * 4, dtype=np.float32).reshape(2, 3, 2, 4)
    mask = np.array([[1, 1, 0], [1, 0, 0]], np.float32)
    idx = np.array([[[1, 2], [0, -1], [0, 1]], [[-1, -1], [0, 0], [0, 0]]])
    rows = valid_rows(e, mask, idx)
    assert rows.shape == (3, 4) and np.array_equal(rows, e.reshape(-1, 4)[[0, 1, 2]])
    assert valid_rows(e[:, :, 0], mask).shape == (3, 4)


# ------------------------------------------------------------------------------------------------ oracle vs reference, every layer
@pytest.fixture(scope="module")
def all_layers():
    arrs, hp, shapes = load_fixture("rnampnn_taps", "all_layers_k6")
    sd = synth.closed_form_state_dict(shapes)
    runs = oracle_runs(hp, sd, arrs["coords"], arrs["mask"], modes=("f32",))
    # the f64 oracle on its own f64 graph: in f64 the row itself (1e6 + 1e-3) no longer ties with the padded residues (1e6)
    runs["f64"] = run_oracle(hp, sd, arrs["coords"], arrs["mask"], "f64")
    return arrs, hp, runs


def test_oracle_taps_match_reference_at_every_layer(all_layers):
    """f32 oracle against the reference's f32 run: h_l and e_l within 1e-4 for l = 0 .. 10, the bound test_stage_taps_match_reference uses
    at layer 1 - or, where the reference's own f32 run is further than a quarter of that from its f64 run, 4 x that distance (``noise_*``
    of the fixture; measured at most 1.8e-5 on h and 4.4e-6 on e, so 1e-4 decides everywhere)."""
    arrs, hp, runs = all_layers
    mask = torch.from_numpy(arrs["mask"])
    L = hp["num_res_mpnn_layers"]
    assert L == 10 and hp["num_res_neighbours"] == 6
    idx = O.canonical_edge_index(torch.from_numpy(arrs["edge_index"]).long(), mask)
    got = runs["f32"]
    assert torch.equal(got["edge_index"], idx)
    assert int((idx != -1).sum()) == 12 * 6 + 7 * 6 + 3 * 3                   # n = 3: two neighbours and the phantom
    for l in range(L + 1):
        for n, ei in (("h", None), ("e", idx)):
            tol = max(1e-4, 4.0 * float(arrs[f"noise_{n}"][l]))
            t = tap_error_padded(got[f"{n}{l}"], arrs[f"{n}{l}"], arrs["mask"], ei)
            print(f"{n}{l:<2d} f32 oracle vs reference: {t}  (bound {tol:.1e})")
            assert t.absmax < tol, (n, l, t.absmax)
            assert float(np.abs(valid_rows(arrs[f"{n}{l}"], arrs["mask"], ei)).max()) > 0.5      # the fixture holds the tap
    assert np.abs(got[f"h{L}"].numpy() - arrs["hL"]).max() < 1e-4
    assert np.abs(got["logits"].numpy() - arrs["logits"]).max() < 2e-5


def test_f64_oracle_taps_match_reference_f64(all_layers):
    arrs, hp, runs = all_layers
    L = hp["num_res_mpnn_layers"]
    idx = runs["f64"]["edge_index"]
    assert torch.equal(idx, runs["f32"]["edge_index"])
    for n, ei in (("h", None), ("e", idx)):
        t = tap_error_padded(runs["f64"][f"{n}{L}"], arrs[f"{n}{L}_f64"], arrs["mask"], ei)
        print(f"{n}{L} f64 oracle vs reference f64: {t}")
        assert t.absmax < 1e-9
    assert np.abs(runs["f64"]["logits"].numpy() - arrs["logits_f64"]).max() < 1e-9


# ------------------------------------------------------------------------------------------------ the yardstick and its control
@pytest.fixture(scope="module")
def case_a():
    from rnampnn.model._schema import DEFAULT_HPARAMS
    hp = dict(DEFAULT_HPARAMS, num_res_neighbours=CASE_A["k"], padding_len=max(CASE_A["lens"]))
    sd, _ = closed_form_sd(hp)
    coords, mask, _ = synth.synth_batch(CASE_A["lens"], first_index=CASE_A["first_index"])
    runs = oracle_runs(hp, sd, coords, mask, modes=("f32", "autocast"))             # asserts: same graph under autocast
    runs["swapped"] = run_oracle(hp, swapped(sd, hp), coords, mask, "f32")
    return hp, mask, runs


def test_autocast_error_is_what_the_reference_shows(case_a):
    """bf16 autocast against plain f32 in the tap metrics, e and h at layers 1, 2, 5, 10: within 0.5 x .. 2 x of the figures of the
    reference's own modules.  A metric that silently measured nothing (an empty selection, a tap compared with itself) falls out below."""
    hp, mask, runs = case_a
    idx = runs["f32"]["edge_index"]
    for l in CASE_A["layers"]:
        for n, ei in (("e", idx), ("h", None)):
            t = tap_error_padded(runs["autocast"][f"{n}{l}"], runs["f32"][f"{n}{l}"], mask, ei)
            print(f"{n}{l:<2d} autocast vs f32: {t}")
            assert t.rows == (3444 if n == "e" else 122)
            for field, (lo, hi) in REF_AUTOCAST[n].items():
                assert 0.5 * lo <= getattr(t, field) <= 2.0 * hi, (n, l, field, getattr(t, field))
            if n == "e":
                assert 0.0 < t.absmax <= 2.0 * REF_AUTOCAST_E_ABSMAX


def test_swapped_channels_show_in_e4_and_not_in_the_logits(case_a):
    hp, mask, runs = case_a
    idx = runs["f32"]["edge_index"]
    assert torch.equal(runs["swapped"]["edge_index"], idx)
    auto = tap_error_padded(runs["autocast"]["e4"], runs["f32"]["e4"], mask, idx)
    swap = tap_error_padded(runs["swapped"]["e4"], runs["f32"]["e4"], mask, idx)
    dlogit = float((runs["swapped"]["logits"] - runs["f32"]["logits"]).abs().max())
    dh = {l: float((runs["swapped"][f"h{l}"] - runs["f32"][f"h{l}"]).abs().max()) for l in (5, 10)}
    print(f"e4 swapped : {swap}\ne4 autocast: {auto}\nmax |dlogit| {dlogit:.2e}  max |dh5| {dh[5]:.2e}  max |dh10| {dh[10]:.2e}")
    assert swap.worst_ch in (5, 77)
    assert swap.max_ch >= 10.0 * auto.max_ch                   # measured 0.41 against 0.032
    assert torch.equal(runs["swapped"]["e3"], runs["f32"]["e3"])
    assert dlogit < 1e-4                                       # ... which is why the logit tests cannot stand in for the tap tests
