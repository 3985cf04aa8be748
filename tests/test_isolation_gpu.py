"""Isolation of the C ABI: a call reads only what its contract says it reads and writes only what its contract says it writes.

Every check has one form: run an entry point twice with everything it must NOT depend on changed between the runs, then assert that
everything it must produce is bit-identical (`tensor.cpu().numpy().tobytes()`) and everything it must not touch is unchanged.  The clean
run is pinned to the reference by the parity tests, so nothing here carries a tolerance: the comparisons are byte equality, guard
integrity, finiteness and three negative controls (poison in a VALID row moves the logits; a host write breaks a guard -
test_isolation_cpu.py; a call changes painted workspace bytes).

Legs.  A: padded coordinates / labels overwritten (1e3 * randn with label 77, NaN with label -1).  B: workspace painted 0xFF, then with
the bytes a call on a larger shape with other inputs and another seed left (stale), against a zeroed one; big -> small -> big through ONE
workspace; the wrappers' own `_ws` / `_tws` / idle tape slot painted between calls.  C: outputs prefilled NaN (-1 for integers) against
7.  D: every input, output and workspace of every run comes from `_isolation.guarded`, `ws_bytes` is exactly the size query's value,
`check()` runs on every buffer after every call, and repainting the guards of the INPUTS 0xFF -> 0x00 changes no output.

    entry point                                   A    B    C    D
    rnampnn_forward (f32, bf16; every tap)        x    x    x    x
    rnampnn_forward_packed (f32, bf16)            n/a  x    x    x    A: a packed batch has no padding (D covers reads past its end)
    rnampnn_loss_and_grad (f32, bf16-mixed; p)    x    x    x    x
    rnampnn_train_forward + _train_backward       x    x    x    x    A includes the padded rows of dlogits
    rnampnn_adam_step                             n/a  n/a  x    x    A, B: no padding, no workspace; C = floats beyond numel untouched
    rdesign_forward (f32, bf16; every tap)        x    x    x    x
    rdesign_readout (f32, bf16)                   n/a  x    x    x    A: n_rows caller rows, no padding
    rdesign_loss_and_grad_ex (f32, bf16-mixed; p) x    x    x    x    edges_75k: B and D only (the large shape is there for the batched reduction launches)
    rdesign_score                                 n/a  x    x    x    A: tests/test_rdesign_trainer_gpu.py has it

Main-model padding rule (include/rnampnn_hip.h, `RnaMpnnForwardIO.coords`): row t == n of an RNA with n - 1 < k is the phantom neighbour's
record and belongs to the result, so it stays zero; every other row t >= n is poisoned.  rdesign: every row t >= n of X is poisoned."""
import numpy as np
import pytest
import torch

import _isolation as iso

pytestmark = pytest.mark.gpu

LENS = [41, 1, 9, 31, 30, 33]            # n == T, a lone residue, n < k, n - 1 == k, n == k, n > k (k = 30)
BIG = [300, 7, 64]                       # max_len > 256: the LDS-row k_knn
STALE_LENS = [310, 9, 70]                # the shape whose leftovers are the stale pattern (larger than BIG)
RN_CFG = {"k30": (30, 48), "k20": (20, 48), "big": (30, 320)}          # num_res_neighbours, padding_len; 2 ResMPNN layers
# name -> (cfg, lengths, T, T_norm, index of an RNA whose mask is cleared with its coordinates left in place)
RN_CASES = {"T41": ("k30", LENS, 41, 0, None), "T41_norm48": ("k30", LENS, 41, 48, None), "T44": ("k30", LENS, 44, 0, None),
            "k20_T44": ("k20", LENS, 44, 0, None), "T41_rna1_masked": ("k30", LENS, 41, 0, 1), "knn_lds_T300": ("big", BIG, 300, 0, None)}
RN_TRAIN_CASES = ["T41", "T41_norm48", "T44", "k20_T44", "T41_rna1_masked"]
F32, BF16 = 0, 1
PRECS = ["f32", "bf16"]


# ================================================================================================ the engine
class Spec:
    """One entry point at one shape.  inputs: name -> CPU tensor; outputs: name -> (shape, dtype); need: the size query's value;
    call(gin, gout, ws, ws_bytes); rows: name -> leading rows the header says are written (absent = all); poison(kind) -> inputs of
    leg A or None; finite: outputs that must be finite under NaN poison; expect(result): what the header promises of the values."""

    def __init__(self, name, inputs, outputs, need, call, rows=None, poison=None, finite=(), expect=None, ws_align=256):
        self.name, self.inputs, self.outputs, self.need, self.call = name, inputs, outputs, int(need), call
        self.rows, self.poison, self.finite, self.expect, self.ws_align = rows or {}, poison, finite, expect, ws_align
        assert self.need > 0, f"{name}: the size query returned 0"


def _prefill(fill, dtype):
    if fill == "nan":
        return float("nan") if dtype.is_floating_point else -1
    return fill


def run(spec, inputs=None, fill="nan", ws_paint=0, in_guard=iso.FF, ws=None, ws_bytes=None):
    """One call with every buffer guarded -> ({output: bytes of the part the header says is written}, workspace)."""
    inputs = spec.inputs if inputs is None else inputs
    gin = {k: iso.guarded(v.shape, v.dtype, fill=v, pattern=in_guard) for k, v in inputs.items()}
    gout = {k: iso.guarded(shp, dt, fill=_prefill(fill, dt)) for k, (shp, dt) in spec.outputs.items()}
    if ws is None:
        ws = iso.guarded((spec.need,), torch.uint8, fill=None, align=spec.ws_align)
        ws_bytes = spec.need                                                    # exactly the size query's value
        if torch.is_tensor(ws_paint):
            iso.paint_bytes(ws, ws_paint)
        elif ws_paint != iso.FF:
            ws.view.fill_(ws_paint)
    spec.call(gin, gout, ws, ws_bytes)
    for k, g in list(gin.items()) + list(gout.items()) + [("workspace", ws)]:
        g.check(f"{spec.name}: {k}")
    res = {}
    for k, g in gout.items():
        v = g.view
        if k in spec.rows:
            r = spec.rows[k]
            tail = v[r:]
            assert iso.tobytes(tail) == iso.tobytes(torch.full_like(tail, _prefill(fill, v.dtype))), \
                f"{spec.name}: {k} rows >= {r} no longer hold their prefill"
            v = v[:r]
        res[k] = iso.tobytes(v)
    return res, ws


def same(a, b, what):
    for k in a:
        d = iso.first_diff(a[k], b[k])
        assert d is None, f"{what}: {k} differs, first at byte {d} of {len(a[k])}"


def assert_finite(res, names, what):
    for k in names:
        assert np.isfinite(np.frombuffer(res[k], np.float32)).all(), f"{what}: {k} is not finite"


def painted_share(spec, ws):
    """Control of leg B: the call changed painted bytes of [0, need).  Prints the share still equal to the paint."""
    left = int((ws.payload_bytes == iso.FF).sum())
    print(f"\n{spec.name}: {left / spec.need:.1%} of the {spec.need} workspace bytes still hold the 0xFF paint")
    assert left < spec.need, f"{spec.name}: the call changed no byte of the painted workspace"


def legs(spec, stale, do_a=True, do_c=True):
    base, _ = run(spec)                                              # zeroed workspace, NaN prefill, guards 0xFF, clean inputs
    r, ws = run(spec, ws_paint=iso.FF)                               # B
    same(base, r, f"{spec.name} leg B (0xFF workspace)")
    painted_share(spec, ws)
    r, _ = run(spec, ws_paint=stale)
    same(base, r, f"{spec.name} leg B (stale workspace)")
    if do_c:
        r, _ = run(spec, fill=7)                                     # C
        same(base, r, f"{spec.name} leg C (prefill 7 against NaN)")
    r, _ = run(spec, in_guard=0x00)                                  # D
    same(base, r, f"{spec.name} leg D (input guards 0x00)")
    if do_a and spec.poison is not None:                             # A
        for kind in ("randn", "nan"):
            r, _ = run(spec, inputs=spec.poison(kind))
            same(base, r, f"{spec.name} leg A ({kind})")
            if kind == "nan":
                assert_finite(r, spec.finite, f"{spec.name} leg A (nan)")
    if spec.expect is not None:
        spec.expect(base)
    return base


def sequence(big, small):
    """big -> small -> big through ONE workspace: both big results bit-equal, the small one equal to a call on a fresh zeroed workspace."""
    ws = iso.guarded((big.need,), torch.uint8, fill=0, align=256)
    b1, _ = run(big, ws=ws, ws_bytes=big.need)
    s, _ = run(small, ws=ws, ws_bytes=big.need)
    b2, _ = run(big, ws=ws, ws_bytes=big.need)
    same(b1, b2, f"{big.name} before / after {small.name} in one workspace")
    same(run(small)[0], s, f"{small.name} after {big.name} in one workspace")
    same(run(big)[0], b1, f"{big.name} in a workspace of its own")


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def stale_of(key, make_spec, **kw):
    """Pattern (b): the workspace bytes a real call of the entry point left on the larger shape (kept on the device)."""
    return cached(("stale",) + key, lambda: run(make_spec(), **kw)[1].payload_bytes)


# ================================================================================================ main model
def rn_model(cfg, prec):
    def make():
        from test_hip_parity import _model
        from rnampnn.model._schema import DEFAULT_HPARAMS, state_dict_shapes
        k, P = RN_CFG[cfg]
        hp = dict(DEFAULT_HPARAMS, num_res_neighbours=k, padding_len=P, num_res_mpnn_layers=2)
        m, _ = _model(hp, state_dict_shapes(hp), prec)
        m._ensure()
        return m
    return cached(("rn_model", cfg, prec), make)


def rn_batch(lengths, T, seed=0, first=40, masked=None):
    from rnampnn.utils import synth
    coords, mask, labels = synth.synth_batch(lengths, first_index=first, seed=seed, max_len=T)
    if masked is not None:
        mask[masked] = 0                                             # the coordinates stay where they are
    return torch.from_numpy(coords), torch.from_numpy(mask), torch.from_numpy(labels).to(torch.int32)


def rn_poison(coords, mask, k, kind, labels=None, dlogits=None):
    """Leg A of the padded main-model inputs: rows t > n, and row t == n where n - 1 >= k (module docstring)."""
    g = torch.Generator().manual_seed(11)
    n = mask.sum(1).long()
    t = torch.arange(mask.shape[1])[None, :]
    pad = (t > n[:, None]) | ((t == n[:, None]) & (n[:, None] - 1 >= k))
    assert not bool((pad & (mask == 1)).any()) and bool(pad.any())
    out = {"mask": mask, "coords": coords.clone()}
    if kind == "randn":
        out["coords"][pad] = 1e3 * torch.randn((int(pad.sum()),) + tuple(coords.shape[2:]), generator=g)
    else:
        out["coords"][pad] = float("nan")
    if labels is not None:
        out["labels"] = labels.clone()
        out["labels"][mask == 0] = 77 if kind == "randn" else -1
    if dlogits is not None:
        out["dlogits"] = dlogits.clone()
        out["dlogits"][mask == 0] = 1e3 if kind == "randn" else float("nan")
    return out


def rn_expect_padded(mask, names):
    """Values of the padded rows (t >= n) of the main model's taps, as include/rnampnn_hip.h states them."""
    pad = (mask == 0).numpy()

    def check(res):
        B, T = pad.shape
        for k in names:
            a = np.frombuffer(res[k], np.int64 if k == "edge_index" else np.float32).reshape(B, T, -1)[pad]
            if k == "edge_index":
                assert (a == -1).all(), k
            elif k == "raw":
                assert (a[:, :21] == np.float32(1e6)).all() and (a[:, 21:] == 0).all(), k
            else:
                assert (a == 0).all(), k
    return check


def rn_forward_spec(case, prec, lengths=None, T=None, seed=0, first=40):
    from rnampnn import _native as N
    cfg, lens, T0, T_norm, masked = RN_CASES[case]
    lens, T = (lens if lengths is None else lengths), (T0 if T is None else T)
    m = rn_model(cfg, prec)
    h, k, B = m._handle.ptr, RN_CFG[cfg][0], len(lens)
    coords, mask, _ = rn_batch(lens, T, seed, first, masked)
    need = N.lib().rnampnn_workspace_bytes(h, B, T)
    return Spec(f"rnampnn_forward[{prec},{case},T={T}]", {"coords": coords, "mask": mask}, iso.rn_tap_shapes(B, T, k), need,
                lambda gi, go, ws, wb: iso.rn_forward(h, gi["coords"], gi["mask"], B, T, T_norm, go, 2, ws, wb),
                poison=(lambda kind: rn_poison(coords, mask, k, kind)) if bool((mask.sum(1) < T - 1).any()) else None,
                finite=("logits", "embedding", "h_post"), expect=rn_expect_padded(mask, iso.RN_TAPS))


def rn_stale_forward(prec):
    return stale_of(("rn_forward", prec), lambda: rn_forward_spec("knn_lds_T300", prec, STALE_LENS, 313, seed=9, first=700), ws_paint=iso.FF)


@pytest.mark.parametrize("case", list(RN_CASES))
@pytest.mark.parametrize("prec", PRECS)
def test_rnampnn_forward(prec, case):
    spec = rn_forward_spec(case, prec)
    assert spec.poison is not None
    legs(spec, rn_stale_forward(prec))


def rn_packed_spec(prec, cfg, lengths, T_norm, seed=0, first=40):
    from rnampnn import _native as N
    m = rn_model(cfg, prec)
    h, B, n_tot = m._handle.ptr, len(lengths), sum(lengths)
    coords, mask, _ = rn_batch(lengths, max(lengths), seed, first)
    packed = coords[mask == 1].contiguous()
    cu = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    need = N.lib().rnampnn_workspace_bytes_packed(h, B, n_tot)
    return Spec(f"rnampnn_forward_packed[{prec},{cfg},N={n_tot},T_norm={T_norm}]", {"coords": packed, "cu": cu},
                {"logits": ((n_tot, 4), torch.float32), "embedding": ((n_tot, 256), torch.float32)}, need,
                lambda gi, go, ws, wb: iso.rn_forward_packed(h, gi["coords"], gi["cu"], B, n_tot, max(lengths), T_norm, go["logits"],
                                                             go["embedding"], ws, wb))


@pytest.mark.parametrize("case", ["k30", "k30_norm48", "k20", "knn_lds"])
@pytest.mark.parametrize("prec", PRECS)
def test_rnampnn_forward_packed(prec, case):
    cfg, lengths, T_norm = {"k30": ("k30", LENS, 0), "k30_norm48": ("k30", LENS, 48), "k20": ("k20", LENS, 0), "knn_lds": ("big", BIG, 0)}[case]
    stale = stale_of(("rn_packed", prec), lambda: rn_packed_spec(prec, "big", STALE_LENS, 0, seed=9, first=700), ws_paint=iso.FF)
    legs(rn_packed_spec(prec, cfg, lengths, T_norm), stale)


def rn_grad_layout(m):
    """-> (numel, bool array: the floats of the flat gradient that belong to no parameter)."""
    import ctypes as C
    from rnampnn import _native as N
    numel = int(N.lib().rnampnn_grad_numel(m._handle.ptr))
    pad = np.ones(numel, bool)
    for i, (_, n) in enumerate(m._handle.weight_schema()):
        off = C.c_int64()
        N.check(N.lib().rnampnn_weight_offset(m._handle.ptr, i, C.byref(off)))
        pad[off.value: off.value + n] = False
    return numel, pad


def expect_grad_padding_zero(pad):
    def check(res):
        g = np.frombuffer(res["grad"], np.float32)
        assert (g[pad] == 0).all(), "padding floats of the flat gradient are not zero"
        assert g[~pad].any()
    return check


def rn_train_spec(case, flags, p, tape=False, lengths=None, T=None, seed=0, first=40, drop_seed=5):
    from rnampnn import _native as N
    cfg, lens, T0, T_norm, masked = RN_CASES[case]
    lens, T = (lens if lengths is None else lengths), (T0 if T is None else T)
    m = rn_model(cfg, "f32" if flags == F32 else "bf16")
    h, k, B = m._handle.ptr, RN_CFG[cfg][0], len(lens)
    coords, mask, labels = rn_batch(lens, T, seed, first, masked)
    numel, gpad = rn_grad_layout(m)
    need = N.lib().rnampnn_train_workspace_bytes(h, B, T)
    outs = {"logits": ((B, T, 4), torch.float32), "grad": ((numel,), torch.float32)}
    pad_logits = rn_expect_padded(mask, ("logits",))
    zero_pad = expect_grad_padding_zero(gpad)
    expect = lambda res: (pad_logits(res), zero_pad(res))
    can_poison = bool((mask.sum(1) < T - 1).any())
    tag = f"[{'f32' if flags == F32 else 'bf16-mixed'},p={p},{case},T={T}]"
    if tape:
        dlogits = torch.randn(B, T, 4, generator=torch.Generator().manual_seed(17)) * 1e-2

        def call(gi, go, ws, wb):
            t = iso.rn_train_forward(h, gi["coords"], gi["mask"], B, T, T_norm, p, drop_seed, flags, go["logits"], ws, wb)
            iso.rn_train_backward(h, t, gi["dlogits"], B, T, 0, go["grad"], ws, wb)
        return Spec("rnampnn_train_forward+backward" + tag, {"coords": coords, "mask": mask, "dlogits": dlogits}, outs, need, call,
                    poison=(lambda kind: rn_poison(coords, mask, k, kind, dlogits=dlogits)) if can_poison else None,
                    finite=("logits", "grad"), expect=expect)
    outs["loss"] = ((1,), torch.float32)
    return Spec("rnampnn_loss_and_grad" + tag, {"coords": coords, "mask": mask, "labels": labels}, outs, need,
                lambda gi, go, ws, wb: iso.rn_loss_and_grad(h, gi["coords"], gi["mask"], gi["labels"], B, T, T_norm, p, drop_seed, flags,
                                                            go["loss"], go["logits"], go["grad"], ws, wb),
                poison=(lambda kind: rn_poison(coords, mask, k, kind, labels=labels)) if can_poison else None,
                finite=("loss", "logits", "grad"), expect=expect)


def rn_stale_train(flags):
    return stale_of(("rn_train", flags), lambda: rn_train_spec("knn_lds_T300", flags, 0.3, lengths=STALE_LENS, T=313, seed=9, first=700, drop_seed=99),
                    ws_paint=iso.FF)


@pytest.mark.parametrize("case", RN_TRAIN_CASES)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("flags", [F32, BF16], ids=["f32", "bf16_mixed"])
def test_rnampnn_loss_and_grad(flags, p, case):
    spec = rn_train_spec(case, flags, p)
    assert spec.poison is not None
    legs(spec, rn_stale_train(flags))


@pytest.mark.parametrize("flags", [F32, BF16], ids=["f32", "bf16_mixed"])
def test_rnampnn_train_forward_backward_through_one_tape(flags):
    legs(rn_train_spec("T44", flags, 0.1, tape=True), rn_stale_train(flags))


@pytest.mark.parametrize("prec", PRECS)
def test_rnampnn_forward_big_small_big_in_one_workspace(prec):
    sequence(rn_forward_spec("knn_lds_T300", prec), rn_forward_spec("knn_lds_T300", prec, LENS, 44))


@pytest.mark.parametrize("flags", [F32, BF16], ids=["f32", "bf16_mixed"])
def test_rnampnn_training_step_big_small_big_in_one_workspace(flags):
    sequence(rn_train_spec("knn_lds_T300", flags, 0.1), rn_train_spec("knn_lds_T300", flags, 0.1, lengths=LENS, T=44))


@pytest.mark.parametrize("prec", PRECS)
def test_rnampnn_wrapper_hands_over_the_painted_workspaces(prec):
    """`RNAMPNN` with its own buffers: `_ws` and the idle tape slot painted 0xFF, then left stale by a larger call."""
    m = rn_model("big", prec)
    m.train_precision = prec
    coords, mask, labels = rn_batch(LENS, 44)
    big = rn_batch(STALE_LENS, 313, seed=9, first=700)
    base = iso.tobytes(m(coords, mask))
    m._ws.fill_(iso.FF)
    assert iso.tobytes(m(coords, mask)) == base
    assert bool((m._ws != iso.FF).any())                              # the call ran in the buffer that was painted
    m(big[0], big[1])
    assert iso.tobytes(m(coords, mask)) == base

    def step(b, seed):
        loss = m.loss_and_grad(b[2].long(), b[0], b[1], dropout=0.1, seed=seed)
        return iso.tobytes(loss) + iso.tobytes(m.flat_grad)
    step(big, 99)                                                     # sizes the slot for both shapes
    g0 = step((coords, mask, labels), 5)
    idle = [s for s in m._tape_pool if not s["busy"]]
    assert idle
    for s in idle:
        s["ws"].fill_(iso.FF)
    assert step((coords, mask, labels), 5) == g0
    assert any(bool((s["ws"] != iso.FF).any()) for s in idle)
    step(big, 99)
    assert step((coords, mask, labels), 5) == g0


@pytest.mark.parametrize("numel", [1, 255, 1027])
def test_rnampnn_adam_step_stays_inside_numel(numel):
    """p, m, v hold 7 more floats than `numel` and must keep them; g holds exactly `numel` floats, and what lies behind it (the guard,
    repainted) must not reach the result."""
    gen = torch.Generator().manual_seed(numel)
    host = {"p": torch.randn(numel + 7, generator=gen), "m": torch.randn(numel + 7, generator=gen) * 1e-2,
            "v": torch.rand(numel + 7, generator=gen) * 1e-3, "g": torch.randn(numel, generator=gen)}
    results = []
    for pattern, tail in ((iso.FF, float("nan")), (0x00, 7.0)):
        bufs = {k: iso.guarded(t.shape, torch.float32, fill=t, pattern=pattern if k == "g" else iso.FF) for k, t in host.items()}
        for k in "pmv":
            bufs[k].view[numel:] = tail
        iso.rn_adam(bufs["p"], bufs["g"], bufs["m"], bufs["v"], numel)
        for k, b in bufs.items():
            b.check(f"adam numel={numel}: {k}")
        for k in "pmv":
            assert iso.tobytes(bufs[k].view[numel:]) == iso.tobytes(torch.full((7,), tail)), f"{k} beyond numel was written"
            assert iso.tobytes(bufs[k].view[:numel]) != iso.tobytes(host[k][:numel]), f"{k} was not updated"
        assert iso.tobytes(bufs["g"].view) == iso.tobytes(host["g"])
        results.append({k: iso.tobytes(bufs[k].view[:numel]) for k in "pmv"})
    same(results[0], results[1], f"adam numel={numel}")
    assert_finite(results[0], "pmv", f"adam numel={numel}")


# ================================================================================================ rdesign
def rd_shapes():
    from test_rdesign_train_gpu import SHAPES
    return SHAPES


def rd_model(shape, prec):
    def make():
        from test_rdesign_train_gpu import _model
        m = _model(rd_shapes()[shape][0], precision=prec)[0]
        m._ensure()
        return m
    return cached(("rd_model", shape, prec), make)


def rd_batch(shape, Tpad, seed=5, label_seed=3, lengths=None):
    from test_rdesign_cpu import _batch
    lengths = rd_shapes()[shape][1] if lengths is None else lengths
    X, mask = _batch(lengths, seed=seed)
    if Tpad:
        X = torch.cat([X, torch.zeros(X.shape[0], Tpad, 6, 3)], 1)
        mask = torch.cat([mask, torch.zeros(mask.shape[0], Tpad)], 1)
    S = torch.randint(0, 4, tuple(mask.shape), generator=torch.Generator().manual_seed(label_seed), dtype=torch.int32)
    S[mask == 0] = 0
    return X.contiguous(), mask.contiguous(), S


def rd_poison(X, mask, kind, labels=None):
    """Leg A: every row t >= n of X (`chain_atom` never reads them), and the padded labels."""
    pad = mask == 0
    assert bool(pad.any())
    out = {"X": X.clone(), "mask": mask}
    if kind == "randn":
        out["X"][pad] = 1e3 * torch.randn((int(pad.sum()), 6, 3), generator=torch.Generator().manual_seed(11))
    else:
        out["X"][pad] = float("nan")
    if labels is not None:
        out["labels"] = labels.clone()
        out["labels"][pad] = 77 if kind == "randn" else -1
    return out


def rd_forward_spec(shape, prec, Tpad, **kw):
    from rdesign import _native as N
    m = rd_model(shape, prec)
    h, K = m._handle.ptr, m.hparams["k_neighbors"]
    X, mask, _ = rd_batch(shape, Tpad, **kw)
    B, T, n = X.shape[0], X.shape[1], int(mask.sum())
    f = torch.float32
    outs = {"h_V": ((B * T, 128), f), "logits": ((B * T, 4), f), "edge_index": ((B, T, K), torch.int64), "node_raw": ((B * T, 101), f),
            "edge_raw": ((B * T * K, 115), f)}
    pad = (mask == 0).numpy()

    def expect(res):
        assert (np.frombuffer(res["edge_index"], np.int64).reshape(B, T, K)[pad] == -1).all()
    return Spec(f"rdesign_forward[{prec},{shape},T={T}]", {"X": X, "mask": mask}, outs, N.lib().rdesign_workspace_bytes(h, B, T),
                lambda gi, go, ws, wb: iso.rd_forward(h, gi["X"], gi["mask"], B, T, go, ws, wb),
                rows={"h_V": n, "logits": n, "node_raw": n, "edge_raw": n * K},
                poison=(lambda kind: rd_poison(X, mask, kind)) if pad.any() else None, finite=("h_V", "logits", "node_raw", "edge_raw"),
                expect=expect)


def rd_stale_forward(prec):
    return stale_of(("rd_forward", prec), lambda: rd_forward_spec("edges_75k", prec, 3, seed=8), ws_paint=iso.FF)


@pytest.mark.parametrize("Tpad", [0, 3])
@pytest.mark.parametrize("shape", ["short_k6", "defaults", "readout2"])
@pytest.mark.parametrize("prec", PRECS)
def test_rdesign_forward(prec, shape, Tpad):
    spec = rd_forward_spec(shape, prec, Tpad)
    assert spec.poison is not None
    legs(spec, rd_stale_forward(prec))


def rd_readout_spec(shape, prec, n_rows, seed=0):
    from rdesign import _native as N
    m = rd_model(shape, prec)
    h = m._handle.ptr
    x = torch.randn(n_rows, 128, generator=torch.Generator().manual_seed(seed))
    return Spec(f"rdesign_readout[{prec},{shape},n={n_rows}]", {"h_V": x}, {"logits": ((n_rows, 4), torch.float32)},
                N.lib().rdesign_readout_workspace_bytes(h, n_rows),
                lambda gi, go, ws, wb: iso.rd_readout(h, gi["h_V"], n_rows, go["logits"], ws, wb))


@pytest.mark.parametrize("shape", ["short_k6", "readout2"])        # the 4-way Linear alone, and behind a hidden layer
@pytest.mark.parametrize("prec", PRECS)
def test_rdesign_readout(prec, shape):
    stale = stale_of(("rd_readout", prec, shape), lambda: rd_readout_spec(shape, prec, 301, seed=1), ws_paint=iso.FF)
    for n_rows in (1, 77):
        legs(rd_readout_spec(shape, prec, n_rows), stale)


def rd_grad_layout(m):
    numel = int(m._flat.numel())
    pad = np.ones(numel, bool)
    for _, n, off in m._handle.weight_schema():
        pad[off: off + n] = False
    return numel, pad


def rd_train_spec(shape, flags, p, Tpad, drop_seed=71, **kw):
    from rdesign import _native as N
    m = rd_model(shape, "f32")
    h = m._handle.ptr
    X, mask, S = rd_batch(shape, Tpad, **kw)
    B, T, n = X.shape[0], X.shape[1], int(mask.sum())
    numel, gpad = rd_grad_layout(m)
    assert numel == int(N.lib().rdesign_param_numel(h))
    f = torch.float32
    return Spec(f"rdesign_loss_and_grad_ex[{'f32' if flags == F32 else 'bf16-mixed'},p={p},{shape},T={T}]", {"X": X, "mask": mask, "labels": S},
                {"loss": ((1,), f), "logits": ((B * T, 4), f), "grad": ((numel,), f)}, N.lib().rdesign_train_workspace_bytes_ex(h, B, T, flags),
                lambda gi, go, ws, wb: iso.rd_loss_and_grad_ex(h, gi["X"], gi["mask"], gi["labels"], B, T, p, drop_seed, flags, go["loss"],
                                                               go["logits"], go["grad"], ws, wb),
                rows={"logits": n}, poison=(lambda kind: rd_poison(X, mask, kind, labels=S)) if bool((mask == 0).any()) else None,
                finite=("loss", "logits", "grad"), expect=expect_grad_padding_zero(gpad))


def rd_stale_train(flags):
    return stale_of(("rd_train", flags), lambda: rd_train_spec("edges_75k", flags, 0.3, 3, drop_seed=99, seed=8, label_seed=4), ws_paint=iso.FF)


@pytest.mark.parametrize("Tpad", [0, 3])
@pytest.mark.parametrize("shape", ["short_k6", "defaults", "readout2"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("flags", [F32, BF16], ids=["f32", "bf16_mixed"])
def test_rdesign_loss_and_grad_ex(flags, p, shape, Tpad):
    spec = rd_train_spec(shape, flags, p, Tpad)
    assert spec.poison is not None
    legs(spec, rd_stale_train(flags))


@pytest.mark.parametrize("flags", [F32, BF16], ids=["f32", "bf16_mixed"])
def test_rdesign_training_step_over_65536_edge_rows(flags):
    """edges_75k: several batched reduction launches.  Legs B and D, and the shape sequence through one workspace."""
    big = rd_train_spec("edges_75k", flags, 0.1, 0)
    assert int(big.inputs["mask"].sum()) * 25 > 65536
    legs(big, rd_stale_train(flags), do_a=False, do_c=False)
    small_lengths = rd_shapes()["short_k6"][1]
    sequence(big, rd_train_spec("edges_75k", flags, 0.1, 3, lengths=small_lengths))


@pytest.mark.parametrize("prec", PRECS)
def test_rdesign_forward_big_small_big_in_one_workspace(prec):
    sequence(rd_forward_spec("edges_75k", prec, 0), rd_forward_spec("edges_75k", prec, 3, lengths=rd_shapes()["short_k6"][1]))


def rd_score_spec(lengths, Tpad, seed=0):
    from rdesign import _native as N
    X, mask, S = rd_batch(None, Tpad, lengths=lengths, label_seed=seed + 3)
    B, T, n = mask.shape[0], mask.shape[1], int(mask.sum())
    rows = n + 3                                                   # the packed buffers may hold more rows than mask.sum()
    logits = torch.randn(rows, 4, generator=torch.Generator().manual_seed(seed))
    i32 = torch.int32
    return Spec(f"rdesign_score[B={B},T={T}]", {"logits": logits, "mask": mask, "labels": S},
                {"correct": ((B,), i32), "valid": ((B,), i32), "nll": ((B,), torch.float32), "pred_out": ((rows,), i32)},
                N.lib().rdesign_score_workspace_bytes(B),
                lambda gi, go, ws, wb: iso.rd_score(gi["logits"], None, rows, gi["mask"], gi["labels"], B, T, go["correct"], go["valid"],
                                                    go["nll"], go["pred_out"], ws, wb),
                rows={"pred_out": n}, ws_align=16)


def test_rdesign_score_workspace_and_guards():
    from test_rdesign_train_gpu import BIG_LENGTHS
    stale = stale_of(("rd_score",), lambda: rd_score_spec(BIG_LENGTHS, 3, seed=1), ws_paint=iso.FF)
    for lengths in ([12, 4, 9], [40, 33, 25, 7, 1]):
        base = legs(rd_score_spec(lengths, 3), stale)
        assert np.frombuffer(base["valid"], np.int32).tolist() == lengths


@pytest.mark.parametrize("prec", PRECS)
def test_rdesign_wrapper_hands_over_the_painted_workspaces(prec):
    """`RNAModel` with its own buffers: `_ws` and `_tws` painted 0xFF, then left stale by a larger call."""
    m = rd_model("edges_75k", prec)
    m.train_precision = prec
    X, mask, S = rd_batch("edges_75k", 3, lengths=rd_shapes()["short_k6"][1])
    big = rd_batch("edges_75k", 3, seed=8, label_seed=4)
    m.eval()
    m.forward_logits(big[0], big[1])                                 # sizes _ws for both shapes
    base = iso.tobytes(m.forward_logits(X, mask))
    m._ws.fill_(iso.FF)
    assert iso.tobytes(m.forward_logits(X, mask)) == base
    assert bool((m._ws != iso.FF).any())
    m.forward_logits(big[0], big[1])
    assert iso.tobytes(m.forward_logits(X, mask)) == base

    def step(b, seed):
        loss = m.loss_and_grad(b[0], b[2].long(), b[1], dropout=0.1, seed=seed)
        return iso.tobytes(loss) + iso.tobytes(m.flat_grad)
    step(big, 99)
    g0 = step((X, mask, S), 71)
    m._tws.fill_(iso.FF)
    assert step((X, mask, S), 71) == g0
    assert bool((m._tws != iso.FF).any())
    step(big, 99)
    assert step((X, mask, S), 71) == g0


# ================================================================================================ negative control of leg A
@pytest.mark.parametrize("model", ["rnampnn", "rdesign"])
def test_the_same_poison_in_a_valid_row_moves_the_logits(model):
    if model == "rnampnn":
        spec = rn_forward_spec("T44", "f32")
        key, row = "coords", (3, 5)
    else:
        spec = rd_forward_spec("short_k6", "f32", 3)
        key, row = "X", (2, 5)
    assert float(spec.inputs["mask"][row]) == 1
    base, _ = run(spec)
    bad = dict(spec.inputs)
    bad[key] = spec.inputs[key].clone()
    bad[key][row] = 1e3 * torch.randn(bad[key].shape[2:], generator=torch.Generator().manual_seed(11))
    moved, _ = run(spec, inputs=bad)
    assert moved["logits"] != base["logits"]
    assert np.isfinite(np.frombuffer(moved["logits"], np.float32)).all()
    if model == "rnampnn":
        # the one padded row leg A leaves alone does belong to the result: row n of RNA 2 (n = 9, n - 1 < k) is its phantom neighbour's record
        n = int(spec.inputs["mask"][2].sum())
        assert n == 9 and n - 1 < 30
        bad = dict(spec.inputs)
        bad["coords"] = spec.inputs["coords"].clone()
        bad["coords"][2, n] = 1e3 * torch.randn(7, 3, generator=torch.Generator().manual_seed(11))
        assert run(spec, inputs=bad)[0]["logits"] != base["logits"]
