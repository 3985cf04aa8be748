"""CPU checks of the boundary: the C-ABI library loads, exports every symbol that
include/rnampnn_hip.h declares, and registers exactly the reference's state-dict schema.
No compute is launched (there is no GPU in the build container)."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN_CASES, REPO

GOLDEN_CASES = [c for c in GOLDEN_CASES if not c.startswith("rdesign_")]     # rdesign_*.npz: the sibling model's fixtures (test_rdesign_golden_*.py)


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    return _native


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "rnampnn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rnampnn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(native):
    lib = native.lib()
    declared = _declared_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/rnampnn_hip.h but not exported"
    assert sorted(native.SYMBOLS) == declared
    assert b"gfx950" in lib.rnampnn_version()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_schema_matches_reference_state_dict(native, golden, name):
    """Keys, order and shapes equal the reference model's state_dict recorded in the fixture."""
    from rnampnn.model._schema import state_dict_shapes, DEFAULT_HPARAMS
    arrs, hp, shapes = golden(name)
    full = dict(DEFAULT_HPARAMS); full.update(hp)
    mine = state_dict_shapes(full)
    assert list(mine.keys()) == list(shapes.keys())
    assert all(tuple(mine[k]) == tuple(shapes[k]) for k in mine)
    h = native.Handle(full, native.PREC_F32)
    sch = h.weight_schema()
    assert [k for k, _ in sch] == list(shapes.keys())
    assert all(n == int(np.prod(shapes[k])) for k, n in sch)
    h.close()


def test_default_model_has_reference_parameter_count():
    from rnampnn.model.rnampnn import RNAMPNN
    m = RNAMPNN(precision="f32")
    assert sum(p.numel() for p in m.parameters()) == 3_536_900


def test_error_codes_map_to_reference_exceptions(native):
    from rnampnn.model._schema import DEFAULT_HPARAMS
    hp = dict(DEFAULT_HPARAMS)
    with pytest.raises(NotImplementedError):
        native.Handle(dict(hp, num_res_neighbours=64), native.PREC_F32)     # k > KMAX
    with pytest.raises(NotImplementedError):
        native.Handle(dict(hp, res_embedding_dim=64), native.PREC_F32)
    with pytest.raises(ValueError):
        native.Handle(dict(hp, num_res_neighbours=0), native.PREC_F32)
    from rnampnn.model.feature import ResFeature
    with pytest.raises(AssertionError):
        ResFeature(num_neighbours=3, num_inside_dist_atoms=1)               # feature.py:169


@pytest.mark.parametrize("change, message", [
    (dict(embedding_ffn_dim=48), "FFN widths must be multiples of 32"),
    (dict(readout_hidden_dim=48), "FFN widths must be multiples of 32"),
    (dict(post_fusion_ffn_dim=2080), "FFN widths must be multiples of 32"),
    (dict(num_raw_ffn_dim=2080), "FFN widths must be multiples of 32"),
    (dict(num_post_fusion_heads=3), "attention heads must be 2, 4, 8 or 16"),
    (dict(num_embedding_attn_layers=1, num_embedding_heads=32), "attention heads must be 2, 4, 8 or 16"),
    (dict(num_readout_layers=0), "layer counts must be >= 1"),
])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_node_side_shapes_outside_the_range_are_refused_at_create(native, change, message, precision):
    """The edges of the node-side range rnampnn_create accepts (widths: multiples of 32 in [32, 2048]; heads 2, 4, 8 or 16 where an
    attention layer exists; every FFN / read-out count >= 1): one step outside is refused at create time with the library's message,
    in both precisions.  The same head counts without an attention layer are legal (tests/_node_shape_cases.py, case no_attention)."""
    from rnampnn.model._schema import DEFAULT_HPARAMS
    prec = native.PREC_F32 if precision == "f32" else native.PREC_BF16
    with pytest.raises(NotImplementedError, match=message):
        native.Handle(dict(DEFAULT_HPARAMS, **change), prec)
    native.Handle(dict(DEFAULT_HPARAMS, num_post_fusion_attn_layers=0, num_post_fusion_heads=3, num_embedding_heads=32), prec).close()


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU instead of computing elsewhere."""
    import torch
    from rnampnn.model.rnampnn import RNAMPNN
    m = RNAMPNN(precision="f32", num_res_mpnn_layers=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, 7, 3), torch.ones(1, 4))


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "rna-mpnn_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "rnampnn_oracle" not in text, f


def test_collate_and_separate_contract():
    """featurize / separate reproduce the reference collate layout (utils/data.py:110-142, 594-604)."""
    import torch
    from rnampnn.utils.data import check_prefix_mask, featurize, separate
    from rnampnn.config.glob import VOCAB, REVERSE_VOCAB, NUM_RES_TYPES, NUM_MAIN_SEQ_ATOMS
    assert VOCAB == {'A': 0, 'U': 1, 'C': 2, 'G': 3} and REVERSE_VOCAB[3] == 'G' and NUM_RES_TYPES == 4 and NUM_MAIN_SEQ_ATOMS == 7
    items = [{'sequence': torch.eye(4)[torch.tensor([0, 1, 2])], 'coordinates': torch.ones(3, 7, 3), 'id': 'a'},
             {'sequence': torch.eye(4)[torch.tensor([3, 3, 1, 0, 2])], 'coordinates': 2 * torch.ones(5, 7, 3), 'id': 'b'}]
    seq, xyz, mask, ids = featurize(items)
    assert seq.shape == (2, 5, 4) and xyz.shape == (2, 5, 7, 3) and ids == ['a', 'b']
    assert mask.tolist() == [[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]] and float(xyz[0, 3:].abs().sum()) == 0
    check_prefix_mask(mask)
    with pytest.raises(ValueError):
        check_prefix_mask(torch.tensor([[1., 0., 1.]]))
    flat = torch.arange(8.)
    sep = separate(flat, torch.tensor([3, 5]))
    assert sep.tolist() == [[0, 1, 2, 0, 0], [3, 4, 5, 6, 7]]


def test_training_path_issues_no_runtime_memset():
    """Round 4 (profiles/r04_graph_memset_root_cause.txt): a hipMemsetAsync captured by torch.cuda.CUDAGraph zeroes on the first replay and
    writes garbage from the second one on (this stack), which corrupted the captured training step in round 3.  The sources of the training
    path therefore zero and copy with their own kernels (launch_zero_bytes / launch_copy_bytes); the only runtime memsets left are in eager
    set-up code and a test tap that are never captured."""
    import re
    csrc = os.path.join(REPO, "rna-mpnn_amd", "csrc")
    for name in ("kernels_train.hip", "kernels_train.h", "red_queue.h", "train_dev.h", "bf16_core.h"):
        src = open(os.path.join(csrc, name)).read()
        assert "hipMemsetAsync" not in src and "hipMemset(" not in src, name
    inc = open(os.path.join(csrc, "train.cpp")).read()
    body = inc[:inc.index("rnampnn_edge_raw_features")] if "rnampnn_edge_raw_features" in inc else inc
    assert "hipMemsetAsync" not in body, "train.cpp: a runtime memset inside the (capturable) training entry points"
    assert len(re.findall(r"launch_zero_bytes\(", body)) >= 4
    # ... and the two helpers themselves launch kernels, never the runtime's memset / copy
    f32 = open(os.path.join(csrc, "kernels_f32.hip")).read()
    for fn in ("launch_zero_bytes", "launch_copy_bytes"):
        m = re.search(r"^void " + fn + r"\(.*?^\}", f32, flags=re.S | re.M)
        assert m, fn
        assert "hipMemsetAsync" not in m.group(0) and "hipMemcpyAsync" not in m.group(0), fn


AB_SWITCHES = {"RNAMPNN_MPNN_V3", "RNAMPNN_NO_BWD1_PAIR", "RNAMPNN_F32_ATTN", "RNAMPNN_NO_RED_BATCH", "RNAMPNN_EMBED_TWO_LAUNCH",
               "RNAMPNN_NODE_UPDATE_TWO_LAUNCH"}


def test_ab_switch_inventory():
    """The library reads exactly the run-time A/B switches a GPU test uses as its reference form, each through ab_switch (rnampnn_internal.h),
    and DESIGN.md section 5 lists every one of them."""
    import glob
    csrc = os.path.join(REPO, "rna-mpnn_amd", "csrc")
    srcs = {p: open(p).read() for ext in ("hip", "cpp", "h", "inc") for p in glob.glob(os.path.join(csrc, "*." + ext))}
    read = set()
    for text in srcs.values():
        read |= set(re.findall(r'\b(?:getenv|ab_switch)\("([^"]+)"\)', text))
    assert read == AB_SWITCHES
    getenv_calls = [(os.path.basename(p), n) for p, t in srcs.items() for n in re.findall(r"\bgetenv\(([^)]*)\)", t)]
    assert getenv_calls == [("rnampnn_internal.h", "name")], getenv_calls
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for name in AB_SWITCHES:
        assert name in design, name
