"""CPU checks of the rdesign bf16-mixed training step: the `_ex` C ABI is declared, bound and exported; the new translation unit keeps the
code base's rules (no runtime fill / copy calls, no atomics, no environment switches, ordered reductions); the default stays the exact-f32
step and its refusal; there is no CPU fallback; the host-only size queries accept either handle and the bf16 tape is at most 0.6 of the f32
one.  Parity: the checker of the GPU file is a restatement (tests/_rdesign_train_ref.py), pinned at p = 0 to the reference's own autograd by
tests/test_rdesign_golden_cpu.py; the step itself is compared with the reference directly in tests/test_rdesign_golden_gpu.py."""
import os
import re

import pytest
import torch

from conftest import REPO
from test_rdesign_cpu import _batch

NEW = ("rdesign_train_workspace_bytes_ex", "rdesign_train_tape_bytes_ex", "rdesign_loss_and_grad_ex")
TUS = ("rdesign_train.hip", "rdesign_train_bf16.hip")          # every translation unit that holds training-step code
F32, MIXED = 0, 1


def _lib():
    import __graft_entry__ as g
    g.build()
    from rdesign import _native
    return g, _native, _native.lib()


def test_ex_entry_points_are_declared_bound_and_exported():
    g, _native, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rdesign_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in rdesign_hip.h"
        assert name in _native.SYMBOLS
        assert hasattr(lib, name)
    assert re.search(r"#define\s+RDESIGN_TRAIN_F32\s+0\b", text) and re.search(r"#define\s+RDESIGN_TRAIN_BF16_MIXED\s+1\b", text)
    assert (_native.TRAIN_F32, _native.TRAIN_BF16_MIXED) == (F32, MIXED)
    assert "rdesign_train_bf16.hip" in g.SOURCES


def test_new_translation_unit_keeps_the_rules():
    """Every unit on its own keeps the bans; the reduction bracket and the gradient zeroing are written once for both steps, so their presence
    is asked of the units together; the tape convention stays with the bf16 sequence."""
    from __graft_entry__ import SOURCES
    srcs = {}
    for tu in TUS:
        assert tu in SOURCES
        srcs[tu] = open(os.path.join(REPO, "rna-mpnn_amd", "csrc", tu)).read()
    codes = {tu: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S)) for tu, src in srcs.items()}
    for tu, code in codes.items():
        for call in ("hipMemset", "hipMemcpy", "memset(", "memcpy("):
            assert call not in code, f"{call} in {tu}: use launch_zero_bytes / launch_copy_bytes"
        assert "atomic" not in code, f"no atomics in {tu}: cross-workgroup sums go through ordered reductions / fixed-order partials"
        assert "getenv" not in code and "ab_switch" not in code, tu
        assert "hipDeviceSynchronize" not in code and "hipStreamSynchronize" not in code, tu
    for fn in ("red_begin", "red_end", "launch_zero_bytes"):
        assert any(fn in code for code in codes.values())
    assert "launch_zero_bytes" in codes["rdesign_train_bf16.hip"]
    assert "tape convention" in srcs["rdesign_train_bf16.hip"].lower()      # the header comment states it per tensor


def test_default_is_the_f32_step_and_there_is_no_cpu_fallback():
    from rdesign.model.rdesign import RNAModel
    X, mask = _batch([5])
    S = torch.zeros(1, 5, dtype=torch.long)
    batch = (X, S, mask, [5], None)
    b = RNAModel(num_mpnn_layers=1, precision="bf16")
    assert b.train_precision == "f32" and RNAModel(num_mpnn_layers=1, precision="f32").train_precision == "f32"
    assert "train_precision" not in b.state_dict() and "train_precision" not in b.hparams
    with pytest.raises(NotImplementedError, match="f32") as e:
        b.loss_and_grad(X, S, mask)
    assert "train_precision" in str(e.value) and "bf16" in str(e.value)        # the refusal names the way out
    with pytest.raises(NotImplementedError, match="f32"):
        b.training_step(batch)
    for prec in ("bf16", "f32"):
        m = RNAModel(num_mpnn_layers=1, precision=prec, train_precision="bf16")
        assert m.train_precision == "bf16"
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.loss_and_grad(X, S, mask)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.training_step(batch)
    b.train_precision = "bf16"                                   # settable after construction
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.loss_and_grad(X, S, mask)
    with pytest.raises(ValueError, match="train_precision"):
        b.train_precision = "int8"
    with pytest.raises(ValueError, match="train_precision"):
        RNAModel(num_mpnn_layers=1, train_precision="int8")
    assert b.train_precision == "bf16"


def test_size_queries_accept_either_handle_and_the_bf16_tape_is_smaller():
    """Host-only.  0.6: per layer the f32 tape holds M = 3 edge tensors (75 node-tensor equivalents at k = 25) plus about 10 node-tensor
    equivalents; halving the edge part gives 0.56."""
    from rdesign.model.rdesign import RNAModel
    _, _native, lib = _lib()
    hb, hf = RNAModel(precision="bf16")._handle, RNAModel(precision="f32")._handle
    assert lib.rdesign_train_workspace_bytes(hb.ptr, 3, 12) == 0                         # the old query keeps its refusal
    assert lib.rdesign_train_workspace_bytes_ex(hb.ptr, 3, 12, F32) == 0 and b"f32" in lib.rdesign_last_error().lower()
    assert lib.rdesign_train_workspace_bytes_ex(hb.ptr, 3, 12, MIXED) > 0
    assert lib.rdesign_train_workspace_bytes_ex(hf.ptr, 3, 12, MIXED) == lib.rdesign_train_workspace_bytes_ex(hb.ptr, 3, 12, MIXED)
    assert lib.rdesign_train_workspace_bytes_ex(hf.ptr, 3, 12, F32) == lib.rdesign_train_workspace_bytes(hf.ptr, 3, 12) > 0
    assert lib.rdesign_train_tape_bytes_ex(hf.ptr, 3, 12, F32) == lib.rdesign_train_tape_bytes(hf.ptr, 3, 12) > 0
    for flags in (2, -1, 7):                                                             # unknown flags
        assert lib.rdesign_train_workspace_bytes_ex(hf.ptr, 3, 12, flags) == 0 and lib.rdesign_train_tape_bytes_ex(hf.ptr, 3, 12, flags) == 0
        assert lib.rdesign_loss_and_grad_ex(hf.ptr, None, None, None, 3, 12, 0.0, 0, flags, None, None, None, None, 0, None) == _native.ERR_BAD_ARG
    f32_tape = lib.rdesign_train_tape_bytes_ex(hf.ptr, 64, 500, F32)
    mixed_tape = lib.rdesign_train_tape_bytes_ex(hb.ptr, 64, 500, MIXED)
    print(f"\ntape at the reference defaults, B = 64, T = 500: f32 {f32_tape / 2 ** 30:.2f} GiB, bf16-mixed {mixed_tape / 2 ** 30:.2f} GiB "
          f"({mixed_tape / f32_tape:.3f}); workspace {lib.rdesign_train_workspace_bytes_ex(hf.ptr, 64, 500, F32) / 2 ** 30:.2f} -> "
          f"{lib.rdesign_train_workspace_bytes_ex(hb.ptr, 64, 500, MIXED) / 2 ** 30:.2f} GiB")
    assert 0 < mixed_tape <= 0.6 * f32_tape
    assert mixed_tape < lib.rdesign_train_workspace_bytes_ex(hb.ptr, 64, 500, MIXED) < lib.rdesign_train_workspace_bytes_ex(hf.ptr, 64, 500, F32)
    # the row limits of the f32 step apply unchanged, and a message depth the mixed step is not built for is refused
    assert lib.rdesign_train_workspace_bytes_ex(hb.ptr, 4096, 1024, MIXED) == 0 and b"2^26" in lib.rdesign_last_error()
    for depth, ok in ((1, False), (2, True), (3, True), (4, False)):
        h = RNAModel(num_mpnn_layers=1, num_message_layers=depth)._handle
        assert (lib.rdesign_train_workspace_bytes_ex(h.ptr, 3, 12, MIXED) > 0) == ok
        if not ok:
            assert b"num_message_layers" in lib.rdesign_last_error()
            assert lib.rdesign_loss_and_grad_ex(h.ptr, None, None, None, 3, 12, 0.0, 0, MIXED, None, None, None, None, 0, None) == 2   # UNSUPPORTED


# rdesign_train_workspace_bytes_ex F32, rdesign_train_tape_bytes_ex F32, the same two for MIXED, rdesign_workspace_bytes: the values of the
# build before the two steps shared one workspace description (every tensor is rounded to 256 bytes on its own: no total depends on carve order)
_K6 = dict(k_neighbors=6, num_mpnn_layers=2)
PINNED_SIZES = (
    (_K6, 3, 12, (69286656, 1180416, 69350400, 793344, 622080)),
    (_K6, 4, 40, (76756736, 5245440, 75233792, 3525120, 2750976)),
    ({}, 3, 12, (84779264, 14598912, 78428672, 8147712, 1992960)),
    ({}, 64, 500, (15766188800, 12976640000, 9655609088, 7242240000, 1768066816)),
    (dict(k_neighbors=30, num_mpnn_layers=3, dim_dense_layers=512, num_readout_layers=2, readout_hidden_dim=128, num_message_layers=2,
          num_dense_layers=1), 4, 40, (103390976, 19417600, 93020672, 10816000, 10774016)),
    (dict(k_neighbors=8, num_mpnn_layers=1, dim_dense_layers=128, num_dense_layers=2, num_readout_layers=3, readout_hidden_dim=128),
     3, 12, (69007104, 774912, 69126144, 480000, 729344)),
)


@pytest.mark.parametrize("case", range(len(PINNED_SIZES)))
def test_size_queries_of_an_f32_handle_are_pinned(case):
    """Host-only: byte totals and tape totals are part of what callers allocate by; sharing the workspace description must not move them."""
    from rdesign.model.rdesign import RNAModel
    _, _native, lib = _lib()
    kw, B, T, want = PINNED_SIZES[case]
    h = RNAModel(precision="f32", **kw)._handle
    got = (lib.rdesign_train_workspace_bytes_ex(h.ptr, B, T, F32), lib.rdesign_train_tape_bytes_ex(h.ptr, B, T, F32),
           lib.rdesign_train_workspace_bytes_ex(h.ptr, B, T, MIXED), lib.rdesign_train_tape_bytes_ex(h.ptr, B, T, MIXED),
           lib.rdesign_workspace_bytes(h.ptr, B, T))
    assert got == want
    assert (lib.rdesign_train_workspace_bytes(h.ptr, B, T), lib.rdesign_train_tape_bytes(h.ptr, B, T)) == want[:2]
