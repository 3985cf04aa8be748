"""The fused ResMPNN launches (kernels_mpnn.hip) run 12 waves per workgroup - three per SIMD - in the <edge, message>, <message> and <edge>
instantiations and 8 in layer 1's embedding variant, and address global memory as "scalar base of the block + 32-bit lane offset".  Neither
may change a result: which wave computes a block does not enter its arithmetic, and a block's base is the same address however it is formed.

k = 30, bf16, L = 4, closed-form weights (as test_sweep_direction_gpu.py, whose tap layers are used here too: taps at layer 2 and 3 see the e
of a descending and of an ascending <edge, message> launch through an ascending and a descending edge-only launch, so every batch below runs
in both sweep directions).

Batches, chosen for the wave count and the addressing.  The grid follows the PADDED size (B x T residues / waves per workgroup, rounded up to
a multiple of 8 from 8 on, at most one workgroup per CU); the blocks are the real residues; with 8 or more workgroups each XCD owns a
contiguous eighth of the blocks, and a workgroup takes its 2 x NW static blocks first and is dealt the rest through the LDS counter.
  a_one_rna_5nt            (5,), T = 8         fewer blocks than waves: a wave without a block reads block 0 and leaves; n <= k: absent edges and
                                               the phantom neighbour take the zero-row select of the Q offsets
  b_one_rna_13nt           (13,), T = 16       one more block than a workgroup has waves (12 first blocks + 1)
  c_one_rna_25nt           (25,), T = 32       2 x 12 + 1
  d_49_blocks              (33, 11, 5), T = 40 ranges of 7, the eighth empty
  e_57_blocks              (40, 12, 5), T = 40 ranges of 8, the eighth holds one block
  f_97_blocks              (59, 25, 13), T = 64    ranges of 13 (12 + 1); RNAs of 13 and 25 nt at other grid positions than in b and c
  g_4300_blocks            54 RNAs of 20 - 140 nt  one workgroup per CU, both static rounds in use; the prefetch of the next block crosses the
                                               logical -> physical translation
  h_7000_blocks            90 RNAs of 20 - 140 nt  more than 2 x 12 blocks per workgroup at 256 CUs: blocks dealt through the counter (g does not get
                                               there with 12 waves; the benchmarked workload, 120 blocks per workgroup, lives there)

Properties: every RNA's logits and its h / e taps at two layers are bit-identical in its batch and alone (same T and T_norm: another grid,
another range, another base); the batch agrees with the round-3 kernel (RNAMPNN_MPNN_V3=1, 8 waves, its own addressing) within the bounds of
test_sweep_direction_gpu.py; the packed entry point returns the padded one's valid rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, L, PAD = 30, 4, 144
TAPS = ("h_layer", "e_layer")
TAP_LAYERS = (2, 3)
V3_TOL = 1e-2            # test_sweep_direction_gpu.py / test_round3_fused_kernel_matches_the_round4_kernel

BATCHES = {"a_one_rna_5nt": ([5], 8), "b_one_rna_13nt": ([13], 16), "c_one_rna_25nt": ([25], 32), "d_49_blocks": ([33, 11, 5], 40),
           "e_57_blocks": ([40, 12, 5], 40), "f_97_blocks": ([59, 25, 13], 64), "g_4300_blocks": (54, 140), "h_7000_blocks": (90, 140)}
TOTALS = {"a_one_rna_5nt": 5, "b_one_rna_13nt": 13, "c_one_rna_25nt": 25, "d_49_blocks": 49, "e_57_blocks": 57, "f_97_blocks": 97}

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
    if isinstance(lens, int):
        lens = [int(n) for n in synth.synth_lengths(lens, 20, 140, seed=11, first_index=0)]
    coords, mask, _ = synth.synth_batch(lens, first_index=500, max_len=T)
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
    print(f"\n{name}: {len(lens)} RNAs of {min(lens)} - {max(lens)} nt, {n_blocks} blocks, T = {T}")
    if name in TOTALS:
        assert n_blocks == TOTALS[name]
    if name.startswith("g_"):
        assert 4000 < n_blocks < 2 * 12 * 256 and min(lens) < 30 and max(lens) > 130
    if name.startswith("h_"):
        assert n_blocks > 2 * 12 * 256 + 256                       # every workgroup of a 256-CU grid is dealt blocks behind its static ones
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
    """Bound on |round 3 - round 4| of an h / e tap, as in test_sweep_direction_gpu.py: the two kernels sum in different orders and round the
    f16 pre-activation, the packed f16 GELU and the running f16 e differently, so after up to L edge updates a value may sit a few f16 ulps
    apart; an f16 ulp is never more than 2^-10 of its value, so 2^-7 of the largest value allows 8 ulps of it or more.  A block read from or
    written to the wrong place is off by the order of the value itself, 100 times as much."""
    return float(ref.abs().max()) * 2.0 ** -7


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_matches_the_round3_kernel(monkeypatch, name):
    """RNAMPNN_MPNN_V3=1: the round-3 kernel (8 waves, ascending only, per-lane 64-bit addresses).  Logits within 1e-2, taps within `_tap_bound`."""
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


@pytest.mark.parametrize("name", ["f_97_blocks", "g_4300_blocks"])
def test_packed_entry_point_gives_the_padded_rows(name):
    from rnampnn.utils.data import pack_batch
    lens, c, m, full = _batch_run(name)
    T = int(c.shape[1])
    packed, cu, max_len = pack_batch([c[b, :n] for b, n in enumerate(lens)])
    assert max_len == max(lens) <= T and int(cu[-1]) == sum(lens)
    lp = _model().forward_packed(packed.cuda(), cu.cuda(), T, T_norm=T).cpu()
    assert torch.equal(lp, full["logits"][m.bool()]), name
