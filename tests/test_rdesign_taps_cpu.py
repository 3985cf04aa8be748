"""The yardstick of test_rdesign_taps_gpu.py, pinned from the oracle alone (no product code runs here): the three oracle runs of every case
see one k-NN graph, the bf16-autocast figures the device is measured in are conditioned, every case is what its name says, a truncated
model's h_V is the tap of the full model, and the negative control passes today's final-tensor bound while missing the tap bound."""
import pytest
import torch

from oracle import rdesign_oracle as O
from _tap_metrics import MIN_ROWS_FOR_CH, tap_error
from test_mpnn_taps_gpu import M_BF16
from _rdesign_tap_oracle import CASES, WEIGHT_SEEDS, case_inputs, oracle_runs, run_oracle, swapped_inputs, truncated, truncated_config

YARDSTICK_MAX = 0.05             # autocast max ch / max row of every asserted tap: a yardstick beyond this would bound nothing
FINAL_TOL = 5e-2                 # the flat bound of test_forward_bf16_within_tolerance on the final h_V and the logits

_cache = {}


def _setup(name, seed):
    if (name, seed) not in _cache:
        kw, cfg, sd, X, mask, depths = case_inputs(name, seed)
        _cache[(name, seed)] = dict(cfg=cfg, sd=sd, X=X, mask=mask, depths=depths, runs=oracle_runs(cfg, sd, X, mask))   # asserts equal graphs
    return _cache[(name, seed)]


@pytest.mark.parametrize("seed", WEIGHT_SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_yardstick_is_conditioned_and_case_is_what_it_says(name, seed):
    s = _setup(name, seed)
    cfg, mask, runs = s["cfg"], s["mask"], s["runs"]
    B, T = mask.shape
    N, K = int(mask.sum()), cfg.k_neighbors
    assert N >= MIN_ROWS_FOR_CH and N == sum(CASES[name][1])
    assert int(runs["f32"]["attend"].sum()) == sum(n * min(n, K) for n in CASES[name][1])
    if name.startswith("B_"):
        assert K == 64 and N * K > 65536 and B * T * K > 65536           # > 512 tiles of 128 rows, live and on the host's bound
    if name.startswith(("C_", "D_")):
        assert N == 257
    if name.startswith("E_"):
        assert N == 256 and (N * K) % 128 == 0
    print()
    for l in s["depths"]:
        A = tap_error(runs["autocast"][f"h_V{l}"], runs["f64"][f"h_V{l}"])
        F = tap_error(runs["f32"][f"h_V{l}"], runs["f64"][f"h_V{l}"])
        print(f"{name} seed {seed} h_V{l} autocast: {A}\n{'':{len(name)}s}             f32: absmax {F.absmax:.2e}")
        assert A.ch_ok and 0 < A.max_ch <= YARDSTICK_MAX and 0 < A.max_row <= YARDSTICK_MAX
    dl = (runs["autocast"]["logits"] - runs["f64"]["logits"]).abs().max()
    assert dl > 0


@pytest.mark.parametrize("name", list(CASES))
def test_truncated_model_is_the_tap(name):
    """``O.forward`` with ``num_mpnn_layers = l`` on ``truncated(sd, l)`` gives h_V bit-equal to tap h_V{l} of the full run (f32)."""
    s = _setup(name, 0)
    for l in s["depths"]:
        sd_l = truncated(s["sd"], l)
        cfg_l = truncated_config(s["cfg"], l)
        assert set(sd_l) == set(O.state_dict_shapes(cfg_l))
        with torch.no_grad():
            h_V, _ = O.forward(s["X"], s["mask"], sd_l, cfg_l)
        assert torch.equal(h_V.to(torch.float64), s["runs"]["f32"][f"h_V{l}"]), f"{name}: truncation at {l} is not the tap"


def test_swapped_inputs_pass_the_final_bound_and_miss_the_tap_bound():
    """The control from the weights alone: case A, seed 0, input columns 5 and 77 of the neighbour block of layer 2's first message Linear
    exchanged, f32 oracle against the UNSWAPPED f64 oracle."""
    s = _setup("A_defaults", 0)
    ref = s["runs"]["f64"]
    bad_sd = swapped_inputs(s["sd"], 1, "neighbour")
    key = "mpnn_layers.1.message_layers.0.weight"
    assert not torch.equal(bad_sd[key], s["sd"][key]) and all(torch.equal(bad_sd[k], v) for k, v in s["sd"].items() if k != key)
    assert torch.equal(bad_sd[key][:, 256 + 5], s["sd"][key][:, 256 + 77]) and torch.equal(bad_sd[key][:, :256], s["sd"][key][:, :256])
    bad = run_oracle(s["cfg"], bad_sd, s["X"], s["mask"], "f32")
    dh = float((bad["h_V9"] - ref["h_V9"]).abs().max())
    dl = float((bad["logits"] - ref["logits"]).abs().max())
    K = tap_error(bad["h_V2"], ref["h_V2"])
    A = tap_error(s["runs"]["autocast"]["h_V2"], ref["h_V2"])
    print(f"\nswapped: final |dh_V| {dh:.2e}  |dlogit| {dl:.2e} (bound {FINAL_TOL});  h_V2 swapped  {K}\n{'':47s}h_V2 autocast {A}\n"
          f"swapped / autocast max ch: {K.max_ch / A.max_ch:.2f}")
    assert dh < FINAL_TOL and dl < FINAL_TOL                                   # today's tests do not see it
    assert (bad["h_V1"] - s["runs"]["f32"]["h_V1"]).abs().max() == 0           # layer 1 is untouched
    assert K.max_ch >= 2 * M_BF16 * A.max_ch                                   # the tap bound does
