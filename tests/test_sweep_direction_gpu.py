"""The fused ResMPNN launches (kernels_mpnn.hip) sweep the edge tensor in alternating directions.  That may not change a result: which wave
computes a block, and when, does not enter its arithmetic.

k = 30, bf16, L = 4: launch 1 (edge embedding + message 1) sweeps ascending, 2 descending, 3 ascending, 4 descending; an e tap at layer l
puts an edge-only launch behind launch l, which takes the next direction.  Taps at layer 2 and at layer 3 therefore see the e of a descending
and of an ascending <edge, message> launch, through an ascending and a descending edge-only launch.  The closed-form weights give nearly flat logits, so the h / e taps carry the checks.  (Against the
oracle the same taps are held in test_mpnn_taps_gpu.py; here two kernels and two batch compositions are compared.)

Batches, chosen for where the logical -> physical block mapping can break (8 waves per workgroup; 8 or more workgroups: eight contiguous
ranges, one per XCD):
  a  one RNA of 5 nt, T = 8         fewer blocks than waves, one workgroup, the single-range mapping; phantom neighbour, absent edges
  b  (33, 9, 7), T = 40             49 blocks in ranges of 7: the eighth range is empty
  c  (40, 9, 8), T = 40             57 blocks in ranges of 8: the eighth range holds one block
  d  36 RNAs of 100 - 140 nt        ~4,300 blocks: waves go past their two static blocks into dealt ones, the prefetch of the next block
                                    crosses the translation

Per-RNA bit identity across batch composition (the RNA in its batch against the RNA alone at the same T and T_norm - another grid, another
range, another position in its range) holds on the commit before this change as well; it was measured there with this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, L, PAD = 30, 4, 144
TAPS = ("h_layer", "e_layer")
TAP_LAYERS = (2, 3)
V3_TOL = 1e-2            # test_round3_fused_kernel_matches_the_round4_kernel


def _lengths_d():
    from rnampnn.utils import synth
    return [int(n) for n in synth.synth_lengths(36, 100, 140, seed=4, first_index=0)]


BATCHES = {"a_one_rna_5nt": ([5], 8), "b_eighth_range_empty": ([33, 9, 7], 40), "c_eighth_range_one_block": ([40, 9, 8], 40),
           "d_dealt_blocks": (None, 140)}

_cache = {}


def _model():
    if "model" not in _cache:
        from rnampnn.model.rnampnn import RNAMPNN
        from rnampnn.utils import synth
        model = RNAMPNN(precision="bf16", num_res_neighbours=K, num_res_mpnn_layers=L, padding_len=PAD)
        sd = synth.closed_form_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _cache["model"] = model.to("cuda:0").eval()
    return _cache["model"]


def _batch(name):
    from rnampnn.utils import synth
    lens, T = BATCHES[name]
    lens = _lengths_d() if lens is None else lens
    coords, mask, _ = synth.synth_batch(lens, first_index=300, max_len=T)
    return lens, torch.from_numpy(coords), torch.from_numpy(mask)


def _run(c, m, T_norm):
    """-> {"logits", ("h_layer", 2), ("e_layer", 2), ("h_layer", 3), ("e_layer", 3)} as CPU tensors; the logits come from a forward
    without taps."""
    model = _model()
    out = {"logits": model(c, m, T_norm=T_norm).cpu()}
    for tl in TAP_LAYERS:
        t = model.forward_taps(c, m, list(TAPS), tap_layer=tl, T_norm=T_norm)
        for name in TAPS:
            out[(name, tl)] = t[name].cpu()
    return out


def _batch_run(name):
    """The batch's run, computed once and shared by the tests."""
    if ("run", name) not in _cache:
        lens, c, m = _batch(name)
        _cache[("run", name)] = (lens, c, m, _run(c, m, int(c.shape[1])))
    return _cache[("run", name)]


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_rna_is_bit_identical_in_its_batch_and_alone(name):
    lens, c, m, full = _batch_run(name)
    T = int(c.shape[1])
    n_blocks = sum(lens)
    print(f"\n{name}: {len(lens)} RNAs, {n_blocks} blocks, T = {T}")
    if name.startswith("b_"):
        assert n_blocks == 49
    if name.startswith("c_"):
        assert n_blocks == 57
    if name.startswith("d_"):
        assert n_blocks > 4000
    for key, v in full.items():
        assert torch.isfinite(v).all(), key
    assert float(full[("e_layer", 2)].abs().max()) > 0.1 and float(full[("h_layer", 3)].abs().max()) > 0.1     # the taps are not flat
    assert not torch.equal(full[("e_layer", 2)], full[("e_layer", 3)])
    for i in range(len(lens)):
        alone = _run(c[i:i + 1], m[i:i + 1], T)
        for key, v in alone.items():
            a, b = v[0].numpy(), full[key][i].numpy()
            same = a.tobytes() == b.tobytes()
            if not same:
                print(f"{name}: RNA {i} ({lens[i]} nt) {key}: max |d| {np.abs(a - b).max():.3e}, {int((a != b).sum())} of {a.size} values differ")
            assert same, (name, i, key)


def _tap_bound(ref):
    """Bound on |round 3 - round 4| of an h / e tap.  The two kernels sum in different orders and round the f16 pre-activation, the packed
    f16 GELU and the running f16 e differently, so after up to L edge updates a value may sit a few f16 ulps apart.  e is stored as f16 of
    0.3244 e, so next to the largest |e| of these batches (~23, stored 7.5) one ulp is 2^-8 / 0.3244 = 1.2e-2 in units of e; an f16 ulp is never
    more than 2^-10 of its value, so 2^-7 of the largest value allows 8 ulps of it or more.  A block read from or written to the wrong place
    is off by the order of the value itself, 100 times as much."""
    return float(ref.abs().max()) * 2.0 ** -7


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_matches_the_round3_kernel(monkeypatch, name):
    """RNAMPNN_MPNN_V3=1: the round-3 kernel sweeps ascending only.  Logits within the 1e-2 of
    test_round3_fused_kernel_matches_the_round4_kernel, the taps within `_tap_bound`."""
    lens, c, m, full = _batch_run(name)
    monkeypatch.setenv("RNAMPNN_MPNN_V3", "1")
    alt = _run(c, m, int(c.shape[1]))
    monkeypatch.delenv("RNAMPNN_MPNN_V3")
    assert any(not torch.equal(alt[key], full[key]) for key in full)              # (a different kernel really ran)
    for key in full:
        d = float((alt[key] - full[key]).abs().max())
        print(f"\n{name}: {key}: max |round 3 - round 4| {d:.3e} (max |value| {float(alt[key].abs().max()):.3f})")
    assert float((alt["logits"] - full["logits"]).abs().max()) < V3_TOL, name
    for key in full:
        if key != "logits":
            assert float((alt[key] - full[key]).abs().max()) < _tap_bound(alt[key]), (name, key)
