"""The GraphNormalization statistics dispatch, pinned to the oracle at the padded lengths where it changes kernel.

`launch_graph_norm_packed` picks its instance by the batch's padded length T: rows in registers up to 160 and up to 256, the loop over
memory up to 512, four workgroups per RNA above; `launch_node_update` leaves the per-RNA form above 256 and its `k_gn_coef` takes the loop
branch there.  The other GPU tests sit at T <= 144 or at the 4,417-nt cases, so nothing small crossed 256 or 512.  Each batch here starts
one residue past a threshold (161, 257, 513) and carries a 1-nt and a 40-nt RNA beside the long one.  Weights, form and bounds are those
of test_configs_gpu.py::test_longest_length_of_the_reference_data_4417_nt: closed-form weights, four ResMPNN layers, logits against the
oracle on the same batch, exactly 0 on padded positions.  A pin, not a new claim: it passed unchanged on the commit before the
statistics kernels were folded into one (docs/experiments.md, "the node side folded")."""
import pytest
import torch

from test_configs_gpu import _hp, _model, _oracle, bf16_tol

pytestmark = pytest.mark.gpu

BATCHES = ([161, 1, 40], [257, 1, 40], [513, 1, 40])
_REF = {}


def _case(lens):
    """(coords, mask, hp, oracle logits) of one batch; the oracle runs once per batch and serves both precisions."""
    from rnampnn.model._schema import state_dict_shapes
    from rnampnn.utils import synth
    key = tuple(lens)
    if key not in _REF:
        coords, mask, _ = synth.synth_batch(list(lens), first_index=7000)
        hp = _hp(num_res_neighbours=30, padding_len=max(lens), num_res_mpnn_layers=4)
        sd = synth.closed_form_state_dict(state_dict_shapes(hp))
        _REF[key] = (coords, mask, hp, sd, _oracle(hp, sd, coords, mask))
    return _REF[key]


@pytest.mark.parametrize("lens", BATCHES, ids=lambda l: f"T{l[0]}")
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_statistics_dispatch_against_the_oracle(precision, lens):
    coords, mask, hp, sd, ref = _case(lens)
    assert coords.shape[1] == lens[0]
    model, _ = _model(hp, precision, sd)
    lg = model(torch.from_numpy(coords), torch.from_numpy(mask)).cpu()
    assert torch.isfinite(lg).all()
    assert (lg[torch.from_numpy(mask) == 0] == 0).all()
    err = float((lg - ref).abs().max())
    print(f"{precision} T={lens[0]}: max |dlogit| {err:.3e}")
    assert err < (1e-4 if precision == "f32" else bf16_tol(ref, mask)), err
