"""Helpers of the isolation tests (tests/test_isolation_cpu.py, tests/test_isolation_gpu.py): guarded buffers, the two poison
patterns and thin ctypes callers of the C ABI that take caller-owned inputs, outputs and workspace.

A guarded buffer is ONE uint8 allocation: front guard | payload at an aligned address | back guard.  The guards hold one byte
pattern.  A write past the payload's extent damages a guard (`check()` fails); a read past it shows as an output that changes when
the guards are repainted.  No kernel ever writes into a guard on purpose: the negative control of the mechanism is a host-side
write (test_isolation_cpu.py).

Poison patterns, exactly two: (a) byte 0xFF everywhere - NaN as f32 and bf16, -1 (the library's own "invalid" sentinel) as int32 and
int64; (b) stale - the bytes a real call of the same entry point left behind on another, larger shape (`paint_bytes` copies them in).
Nothing here reads as a huge positive integer: a path that consumes an uninitialised index shows as a value difference, it is not
made to dereference garbage."""
import ctypes as C

import numpy as np
import torch

FF = 0xFF
GUARD_BYTES = 4096


class Guarded:
    """`view`: the payload, exactly the requested extent.  `buf`: the whole uint8 allocation.  `lo`, `hi`: payload byte range in it."""

    def __init__(self, buf, lo, hi, view, pattern):
        self.buf, self.lo, self.hi, self.view, self.pattern = buf, lo, hi, view, int(pattern)

    @property
    def payload_bytes(self):
        """The payload as a flat uint8 view (same memory as `view`)."""
        return self.buf[self.lo:self.hi]

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.lo)

    def nbytes(self):
        return self.hi - self.lo

    def check(self, what="buffer"):
        """Both guards still hold their pattern."""
        for name, g, base in (("front", self.buf[:self.lo], 0), ("back", self.buf[self.hi:], self.hi)):
            bad = (g != self.pattern).nonzero()
            if bad.numel():
                off = int(bad[0]) + base - self.lo
                raise AssertionError(f"{what}: {name} guard damaged, {bad.shape[0]} byte(s), first at payload offset {off} "
                                     f"(payload is [0, {self.hi - self.lo}))")

    def repaint(self, pattern):
        """New guard contents; the payload is left alone."""
        self.pattern = int(pattern)
        self.buf[:self.lo] = self.pattern
        self.buf[self.hi:] = self.pattern


def guarded(shape, dtype, fill=None, guard_bytes=GUARD_BYTES, pattern=FF, align=16, device="cuda"):
    """One buffer `front guard | payload | back guard`, the payload's ADDRESS a multiple of `align` (256 for workspaces, 16 otherwise).
    fill: None = the payload holds `pattern` bytes too; a number = `fill_`; a tensor = copied in (cast to dtype)."""
    shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = item * int(np.prod(shape, dtype=np.int64)) if shape else item
    buf = torch.empty(2 * guard_bytes + nbytes + align, dtype=torch.uint8, device=device)
    buf.fill_(int(pattern))
    base = buf.data_ptr()
    lo = (base + guard_bytes + align - 1) // align * align - base
    hi = lo + nbytes
    view = buf[lo:hi].view(dtype).view(shape)
    if fill is not None:
        if torch.is_tensor(fill):
            view.copy_(fill.to(dtype).reshape(shape))
        else:
            view.fill_(fill)
    return Guarded(buf, lo, hi, view, pattern)


def paint_bytes(g, src):
    """Pattern (b): the payload of `g` takes the leading bytes of `src` (any tensor), repeated if `src` is the shorter one."""
    dst = g.payload_bytes
    s = src.reshape(-1).view(torch.uint8)
    n, m = dst.numel(), s.numel()
    for o in range(0, n, m):
        c = min(m, n - o)
        dst[o:o + c] = s[:c]


def tobytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def first_diff(a, b):
    """Byte offset of the first difference of two bytes objects of equal length, or None."""
    if a == b:
        return None
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if x.size != y.size:
        return min(x.size, y.size)
    return int(np.flatnonzero(x != y)[0])


def _p(t):
    if t is None:
        return None
    if isinstance(t, Guarded):
        return t.ptr()
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- main model (include/rnampnn_hip.h)
RN_TAPS = ("logits", "embedding", "edge_index", "raw", "h0", "e0", "h_layer", "e_layer", "h_post", "raw_emb")


def rn_tap_shapes(B, T, k):
    f, i = torch.float32, torch.int64
    return {"logits": ((B, T, 4), f), "embedding": ((B, T, 256), f), "edge_index": ((B, T, k), i), "raw": ((B, T, 28), f),
            "h0": ((B, T, 128), f), "e0": ((B, T, k, 128), f), "h_layer": ((B, T, 128), f), "e_layer": ((B, T, k, 128), f),
            "h_post": ((B, T, 128), f), "raw_emb": ((B, T, 128), f)}


def rn_forward(h, coords, mask, B, T, T_norm, outs, tap_layer, ws, ws_bytes):
    from rnampnn import _native as N
    io = N.RnaMpnnForwardIO()
    io.coords, io.mask, io.B, io.T, io.T_norm, io.stop_after, io.tap_layer = _p(coords), _p(mask), B, T, T_norm, 0, tap_layer
    for name, t in outs.items():
        setattr(io, name, _p(t))
    N.check(N.lib().rnampnn_forward(h, C.byref(io), _p(ws), C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()


def rn_forward_packed(h, coords_p, cu, B, N_total, T_max, T_norm, logits, emb, ws, ws_bytes):
    from rnampnn import _native as N
    N.check(N.lib().rnampnn_forward_packed(h, _p(coords_p), _p(cu), B, N_total, T_max, T_norm, _p(logits), _p(emb), _p(ws),
                                           C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()


def rn_loss_and_grad(h, coords, mask, labels, B, T, T_norm, p, seed, flags, loss, logits, grad, ws, ws_bytes):
    from rnampnn import _native as N
    N.check(N.lib().rnampnn_loss_and_grad(h, _p(coords), _p(mask), _p(labels), B, T, T_norm, C.c_float(p), C.c_uint64(seed), flags,
                                          _p(loss), _p(logits), _p(grad), _p(ws), C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()


def rn_train_forward(h, coords, mask, B, T, T_norm, p, seed, flags, logits, ws, ws_bytes):
    from rnampnn import _native as N
    tape = C.c_int64(0)
    N.check(N.lib().rnampnn_train_forward(h, _p(coords), _p(mask), B, T, T_norm, C.c_float(p), C.c_uint64(seed), flags, _p(logits),
                                          _p(ws), C.c_size_t(ws_bytes), _stream(), C.byref(tape)))
    torch.cuda.synchronize()
    return int(tape.value)


def rn_train_backward(h, tape, dlogits, B, T, accumulate, grad, ws, ws_bytes):
    from rnampnn import _native as N
    N.check(N.lib().rnampnn_train_backward(h, C.c_int64(tape), _p(dlogits), B, T, accumulate, _p(grad), _p(ws), C.c_size_t(ws_bytes),
                                           _stream()))
    torch.cuda.synchronize()


def rn_adam(param, grad, m, v, numel, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=3):
    from rnampnn import _native as N
    N.check(N.lib().rnampnn_adam_step(_p(param), _p(grad), _p(m), _p(v), C.c_int64(numel), C.c_float(lr), C.c_float(b1), C.c_float(b2),
                                      C.c_float(eps), C.c_float(wd), step, _stream()))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- rdesign (include/rdesign_hip.h)
def rd_forward(h, X, mask, B, T, outs, ws, ws_bytes):
    from rdesign import _native as N
    g = lambda k: _p(outs.get(k))
    N.check(N.lib().rdesign_forward(h, _p(X), _p(mask), B, T, g("h_V"), g("logits"), g("edge_index"), g("node_raw"), g("edge_raw"),
                                    _p(ws), C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()


def rd_readout(h, h_V, n_rows, logits, ws, ws_bytes):
    from rdesign import _native as N
    N.check(N.lib().rdesign_readout(h, _p(h_V), n_rows, _p(logits), _p(ws), C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()


def rd_loss_and_grad_ex(h, X, mask, labels, B, T, p, seed, flags, loss, logits, grad, ws, ws_bytes):
    from rdesign import _native as N
    N.check(N.lib().rdesign_loss_and_grad_ex(h, _p(X), _p(mask), _p(labels), B, T, C.c_float(p), C.c_uint64(seed), flags, _p(loss),
                                             _p(logits), _p(grad), _p(ws), C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()


def rd_score(logits, pred, n_rows, mask, labels, B, T, correct, valid, nll, pred_out, ws, ws_bytes):
    from rdesign import _native as N
    N.check(N.lib().rdesign_score(_p(logits), _p(pred), n_rows, _p(mask), _p(labels), B, T, _p(correct), _p(valid), _p(nll),
                                  _p(pred_out), _p(ws), C.c_size_t(ws_bytes), _stream()))
    torch.cuda.synchronize()
