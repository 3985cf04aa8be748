"""The guard mechanism of tests/_isolation.py on CPU tensors: the negative control of every `check()` of test_isolation_gpu.py.
The damage is always a host-side write; no device kernel writes into a guard on purpose."""
import pytest
import torch

import _isolation as iso

CASES = [((5, 3), torch.float32, 16), ((7,), torch.int64, 16), ((1027,), torch.float32, 16), ((3, 2, 4), torch.bfloat16, 16),
         ((1000,), torch.uint8, 256), ((0,), torch.float32, 16)]


@pytest.mark.parametrize("shape,dtype,align", CASES)
def test_payload_is_aligned_and_has_the_exact_extent(shape, dtype, align):
    g = iso.guarded(shape, dtype, fill=0, guard_bytes=512, align=align, device="cpu")
    item = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    assert tuple(g.view.shape) == shape and g.view.dtype == dtype and g.view.is_contiguous()
    assert g.nbytes() == numel * item == g.payload_bytes.numel()
    assert g.ptr().value == g.buf.data_ptr() + g.lo and g.ptr().value % align == 0
    if numel:
        assert g.view.data_ptr() == g.ptr().value
    assert g.lo >= 512 and g.buf.numel() - g.hi >= 512            # both guards are at least guard_bytes long
    assert bool((g.buf[:g.lo] == iso.FF).all()) and bool((g.buf[g.hi:] == iso.FF).all())
    g.check()


def test_fill_forms():
    g = iso.guarded((4, 2), torch.float32, fill=float("nan"), guard_bytes=64, device="cpu")
    assert bool(torch.isnan(g.view).all())
    g = iso.guarded((4,), torch.int32, fill=7, guard_bytes=64, device="cpu")
    assert g.view.tolist() == [7] * 4
    g = iso.guarded((2, 3), torch.int32, fill=torch.arange(6).reshape(2, 3), guard_bytes=64, device="cpu")
    assert g.view.dtype == torch.int32 and g.view.reshape(-1).tolist() == list(range(6))
    for dt, probe in ((torch.float32, lambda v: bool(torch.isnan(v).all())), (torch.bfloat16, lambda v: bool(torch.isnan(v).all())),
                      (torch.int32, lambda v: bool((v == -1).all())), (torch.int64, lambda v: bool((v == -1).all()))):
        g = iso.guarded((6,), dt, fill=None, guard_bytes=64, device="cpu")      # pattern (a): 0xFF = NaN / -1
        assert probe(g.view), dt
    g.check()


@pytest.mark.parametrize("side", ["front_first", "front_last", "back_first", "back_last"])
def test_check_fails_after_a_one_byte_host_write_in_a_guard(side):
    g = iso.guarded((33,), torch.float32, fill=1.5, guard_bytes=128, device="cpu")
    g.check()
    before = iso.tobytes(g.view)
    pos = {"front_first": 0, "front_last": g.lo - 1, "back_first": g.hi, "back_last": g.buf.numel() - 1}[side]
    g.buf[pos] = 0xFE
    with pytest.raises(AssertionError, match=side.split("_")[0] + " guard damaged"):
        g.check()
    assert iso.tobytes(g.view) == before
    g.buf[pos] = iso.FF
    g.check()


def test_a_write_inside_the_payload_leaves_the_guards_whole():
    g = iso.guarded((33,), torch.float32, fill=1.5, guard_bytes=128, device="cpu")
    g.view[0] = 2.0
    g.view[-1] = 3.0
    g.payload_bytes[5] = 9
    g.check()


def test_repaint_changes_the_guards_and_not_the_payload():
    g = iso.guarded((9, 4), torch.float32, fill=torch.arange(36.0).reshape(9, 4), guard_bytes=128, device="cpu")
    before = iso.tobytes(g.view)
    g.repaint(0x00)
    assert bool((g.buf[:g.lo] == 0).all()) and bool((g.buf[g.hi:] == 0).all())
    assert iso.tobytes(g.view) == before
    g.check()                                   # the new pattern is the one checked from now on
    g.buf[g.hi] = iso.FF
    with pytest.raises(AssertionError, match="back guard damaged"):
        g.check()


def test_paint_bytes_and_first_diff():
    g = iso.guarded((10,), torch.int32, fill=0, guard_bytes=64, device="cpu")
    iso.paint_bytes(g, torch.arange(100, dtype=torch.int32))                     # longer source: its leading bytes
    assert g.view.tolist() == list(range(10))
    iso.paint_bytes(g, torch.tensor([1, 2, 3], dtype=torch.int32))               # shorter source: repeated
    assert g.view.tolist() == [1, 2, 3, 1, 2, 3, 1, 2, 3, 1]
    g.check()
    a = iso.tobytes(g.view)
    assert iso.first_diff(a, a) is None
    g.view[2] = 77
    assert iso.first_diff(a, iso.tobytes(g.view)) == 8
