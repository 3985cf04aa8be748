"""The rdesign forward (``rdesign_forward``: the f32 branch, and under ``RDESIGN_PREC_BF16`` the trainer's MFMA edge kernels te_gemm,
te_mlp2_fwd and tm_gemm_nt, k_rd_segsum_b and the bf16 rownorm that writes h_E) pinned to the f64 oracle through the h_V tap of the layers
that matter, per channel and per row (``_tap_metrics``), at every kernel form the message stack takes.

Taps need no ABI entry: h_E is never updated in this model, so h_V of a model built with ``num_mpnn_layers = l`` and loaded with the first
``l`` layers of the state dict is the tap after layer ``l`` (test_rdesign_taps_cpu.py holds the oracle to that identity bit for bit).

Reference: ``oracle.rdesign_oracle.forward`` in float64; its k-NN lists, the f32 oracle's and the autocast run's are equal on every case
(``_rdesign_tap_oracle.oracle_runs`` asserts it) and the device's ``edge_index`` must equal them.  Bounds (the rule of test_mpnn_taps_gpu.py):
  f32   ``absmax`` and the largest row rms of every tap <= max(2e-4, 4 x max |f32 oracle - f64 oracle| on that tap); the logits likewise.
  bf16  ``max ch``, ``max row`` and ``absmax`` of every tap <= M_BF16 x the same figure of the f32 oracle under bf16 autocast against the
        same reference; max |dlogit| at full depth <= M_BF16 x the autocast run's.  The measured ratios are printed (DESIGN.md section 9
        holds the table); they are records, the bound is M_BF16.
Cases and what each exercises: ``_rdesign_tap_oracle.CASES``."""
import pytest
import torch

from _tap_metrics import tap_error
from _rdesign_tap_oracle import CASES, WEIGHT_SEEDS, case_inputs, oracle_runs, swapped_inputs, truncated
from test_mpnn_taps_gpu import F32_TAP_TOL, M_BF16

pytestmark = pytest.mark.gpu

CONTROL_FACTOR = 1.5             # the CPU file pins >= 2 x M_BF16 x autocast from the weights alone; device rounding may partly cancel in the worst channel
FIGURES = ("max_ch", "max_row", "absmax")

_cache = {}


def _setup(name, seed):
    """-> dict(kw, cfg, sd, X, mask, depths, runs = {"f64", "f32", "autocast"}: oracle taps), computed once per module."""
    if (name, seed) not in _cache:
        kw, cfg, sd, X, mask, depths = case_inputs(name, seed)
        _cache[(name, seed)] = dict(kw=kw, cfg=cfg, sd=sd, X=X, mask=mask, depths=depths, runs=oracle_runs(cfg, sd, X, mask))
    return _cache[(name, seed)]


def _tap(kw, sd, l, precision, X, mask):
    """The device's (edge_index, h_V, logits) of the first ``l`` layers, on the CPU.  The workspace is painted 0xFF first (NaN in f32 and
    bf16): every model here is new, and the allocator would otherwise hand it the block of the previous depth, where a row that a kernel
    skips may still hold the right values of the same layer."""
    from rdesign.model.rdesign import RNAModel
    m = RNAModel(precision=precision, **dict(kw, num_mpnn_layers=l))
    m.load_state_dict(truncated(sd, l))
    m = m.cuda().eval()
    m._ws_args(int(X.shape[0]), int(X.shape[1]), m.device)
    m._ws.fill_(0xFF)
    out = m._run(X, mask, want=("edge_index", "h_V", "logits"))
    return {k: v.cpu() for k, v in out.items()}


def _ratio(k, a):
    return k / a if a > 0 else (0.0 if k == 0 else float("inf"))


def _check_tap(label, precision, got, runs, key, failures):
    ref = runs["f64"][key]
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    K = tap_error(got, ref)
    if precision == "f32":
        tol = max(F32_TAP_TOL, 4.0 * tap_error(runs["f32"][key], ref).absmax)
        print(f"{label} {key:>5s} f32 : {K}  row rms max {K.max_row_rms:.3e}  bound {tol:.1e}")
        if not (K.absmax <= tol and K.max_row_rms <= tol):
            failures.append((label, key, "absmax", K.absmax, tol))
        return K
    A = tap_error(runs["autocast"][key], ref)
    ratio = {f: _ratio(getattr(K, f), getattr(A, f)) for f in FIGURES}
    print(f"{label} {key:>5s} bf16: {K}\n{'':{len(label)}s}   autocast: {A}\n{'':{len(label)}s}   kernel / autocast: ch {ratio['max_ch']:.2f}  "
          f"row {ratio['max_row']:.2f}  absmax {ratio['absmax']:.2f}")
    assert K.ch_ok
    for f in FIGURES:
        if not ratio[f] <= M_BF16:
            failures.append((label, key, f, getattr(K, f), M_BF16 * getattr(A, f)))
    return K


def _check_logits(label, precision, got, runs, failures):
    ref = runs["f64"]["logits"]
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err = float((got.to(torch.float64) - ref).abs().max())
    if precision == "f32":
        tol = max(F32_TAP_TOL, 4.0 * float((runs["f32"]["logits"] - ref).abs().max()))
        print(f"{label} logits f32 : max |dlogit| {err:.3e}  bound {tol:.1e}")
    else:
        auto = float((runs["autocast"]["logits"] - ref).abs().max())
        tol = M_BF16 * auto
        print(f"{label} logits bf16: max |dlogit| {err:.3e}  autocast {auto:.3e}  kernel / autocast: {_ratio(err, auto):.2f}")
    if not err <= tol:
        failures.append((label, "logits", "absmax", err, tol))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("seed", WEIGHT_SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_layer_taps_match_f64_oracle(name, seed, precision):
    s = _setup(name, seed)
    cfg, mask, runs = s["cfg"], s["mask"], s["runs"]
    E_idx, attend = runs["f32"]["E_idx"], runs["f32"]["attend"]
    B, T = mask.shape
    label = f"{name}/s{seed}"
    print(f"\n{label}: k = {cfg.k_neighbors}, L = {cfg.num_mpnn_layers}, msg {cfg.num_message_layers}, {B} RNAs, T = {T}, {int(mask.sum())} residues, "
          f"{int(mask.sum()) * cfg.k_neighbors} edge rows ({int(attend.sum())} attended) of {B * T * cfg.k_neighbors}")
    failures = []
    for l in s["depths"]:
        out = _tap(s["kw"], s["sd"], l, precision, s["X"], mask)
        idx = out["edge_index"][:, :, :E_idx.shape[2]]
        assert bool(((idx >= 0) == attend).all()) and bool((out["edge_index"][:, :, E_idx.shape[2]:] < 0).all()), f"{label}: the kernel attends other slots than the oracle"
        assert bool((idx[attend] == E_idx[attend]).all()), f"{label}: the kernel's neighbour lists are not the oracle's"
        _check_tap(label, precision, out["h_V"], runs, f"h_V{l}", failures)
        if l == cfg.num_mpnn_layers:
            _check_logits(label, precision, out["logits"], runs, failures)
    assert not failures, failures


def test_swapped_inputs_miss_the_tap_bound():
    """Negative control on the device: case A, seed 0, depth 2.  A bf16 model loaded with input columns 5 and 77 of the neighbour block of
    layer 2's first message Linear exchanged (``swapped_inputs``: correct code on other weights - the final h_V and the logits stay inside
    the flat 5e-2 of the final-tensor tests, test_rdesign_taps_cpu.py) against the UNSWAPPED f64 tap: ``max ch`` of h_V2 must miss the
    bound of test_layer_taps_match_f64_oracle by 1.5 x or more, and the model with the right weights passes that bound."""
    s = _setup("A_defaults", 0)
    runs = s["runs"]
    ref = runs["f64"]["h_V2"]
    A = tap_error(runs["autocast"]["h_V2"], ref)
    bad_sd = swapped_inputs(s["sd"], 1, "neighbour")
    K = tap_error(_tap(s["kw"], bad_sd, 2, "bf16", s["X"], s["mask"])["h_V"], ref)
    G = tap_error(_tap(s["kw"], s["sd"], 2, "bf16", s["X"], s["mask"])["h_V"], ref)
    print(f"\nh_V2 swapped : {K}\nh_V2 right   : {G}\nh_V2 autocast: {A}\nswapped / bound: {K.max_ch / (M_BF16 * A.max_ch):.2f}  right / bound: "
          f"{G.max_ch / (M_BF16 * A.max_ch):.2f}")
    assert K.ch_ok and A.max_ch > 0
    assert K.max_ch >= CONTROL_FACTOR * M_BF16 * A.max_ch
    assert G.max_ch <= M_BF16 * A.max_ch
