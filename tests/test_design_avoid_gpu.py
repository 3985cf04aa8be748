"""``rnampnn_design_avoid`` (csrc/design_avoid.hip) on the device, against the float64 restatement of its contract in
tests/_design_avoid_ref.py, against a substring scan of the written bytes and against ``rnampnn_score``.

The batch is the one ``_design_avoid_ref`` describes next to ``CASE_LENGTHS`` (lengths 0, 1, 2, 3, 63, 64, 65, 257, 300; T = 300, S = 4,
logits 3 * randn with G raised by 6 on three RNAs, a seed above 2^32, a fixed stretch that spells a motif, fixed GGG between free
positions, ``allowed = 0``, IUPAC and omitted letters, a per-position bias) under three automata: no run longer than 3, an overlapping /
suffix set, and a set with exactly 64 states; temperatures 1.0 and 0.3.

Device and restatement differ by last-bit exp / log (about 1e-13 relative after 300 steps of the backward pass), so a draw whose path has a
selection within 1e-8 of a cumulative boundary is left out of the equality check; tests/test_design_avoid_cpu.py bounds the share of such
draws by 1 % for the restatement alone, and the same bound is asserted here."""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "rna-mpnn_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_avoid_ref as R  # noqa: E402
from _design_case import SMALL, design_outputs, raw_design, _bytes, _dev, _write_data, _checkpoint  # noqa: E402

LENGTHS, T, S, SEED = R.CASE_LENGTHS, R.CASE_T, R.CASE_S, R.CASE_SEED
NEAR = 1e-8
OUTPUTS = ("seqs", "seq_nll", "infeasible", "hits", "avoid_miss")
FURTHER = (("hits", torch.int32, True), ("avoid_miss", torch.int32, False))
FEASIBLE = [b for b in range(len(LENGTHS)) if not R.CASE_MISS[b]]
T_MAX_RUN3 = 1064                                                  # the largest padded extent at 13 live states: 163,792 of 163,840 bytes


def _automaton(name):
    from rnampnn.utils.motifs import MotifAutomaton
    motifs, max_run = R.CASE_AUTOMATA[name]
    return MotifAutomaton.from_motifs(motifs, max_run=max_run)


def design_avoid(logits, delta, n_states, terminal, seed=SEED, S=S, **kw):
    """The C entry on device tensors (numpy arrays are uploaded) -> dict of its five outputs."""
    return raw_design("rnampnn_design_avoid", (_dev(delta, torch.uint8), int(n_states), C.c_uint64(int(terminal))), FURTHER, logits, seed=seed,
                      S=S, **kw)


@pytest.fixture(scope="module")
def case():
    """Inputs on the device, uploaded once and never written to."""
    import __graft_entry__ as g
    g.build()
    h = R.case_arrays()
    d = dict(h=h, run={}, auto={name: _automaton(name) for name in R.CASE_AUTOMATA})
    for k in ("logits", "mask", "allowed", "bias", "packed", "cu"):
        d[k] = torch.from_numpy(h[k]).cuda()
    return d


def _run(case, name, temperature=1.0, layout="padded"):
    """The batch through the kernel, once per (automaton, temperature, layout)."""
    key = (name, float(temperature), layout)
    if key not in case["run"]:
        a = case["auto"][name]
        kw = dict(temperature=temperature, allowed=case["allowed"], bias=case["bias"])
        if layout == "padded":
            case["run"][key] = design_avoid(case["logits"], a.delta, a.n_states, a.terminal, mask=case["mask"], **kw)
        else:
            case["run"][key] = design_avoid(case["packed"], a.delta, a.n_states, a.terminal, cu=case["cu"], T=T, **kw)
    return case["run"][key]


def _ref(case, name, temperature):
    a = case["auto"][name]
    return R.case_ref(name, a.delta.numpy(), a.terminal, temperature)


def _scan(seqs, name):
    words = R.expand(*R.CASE_AUTOMATA[name])
    return np.array([[R.naive_hits(row, words) for row in plane] for plane in seqs], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("name", sorted(R.CASE_AUTOMATA))
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_restatement_and_hold_no_motif(case, name, temperature):
    out = _run(case, name, temperature)
    want, margin, bad, miss, hits, plans = _ref(case, name, temperature)
    got = out["seqs"].cpu().numpy()
    near = margin <= NEAR
    print(f"{name}, temperature {temperature}: {near.mean():.4%} of the {near.size} (sample, RNA) draws left out (a selection within {NEAR} "
          f"of a boundary)")
    assert near.mean() <= 0.01
    assert out["avoid_miss"].tolist() == miss.tolist() == R.CASE_MISS
    assert out["infeasible"].tolist() == bad.tolist() == R.CASE_INFEASIBLE
    differ = [(s, b) for s in range(S) for b in range(len(LENGTHS)) if not near[s, b] and not np.array_equal(got[s, b], want[s, b])]
    assert not differ, f"draws (sample, RNA) that differ from the restatement: {differ}"
    for b, n in enumerate(LENGTHS):
        assert (got[:, b, n:] == -1).all() and ((got[:, b, :n] >= 0) & (got[:, b, :n] <= 3)).all()
    # hits: the output is the recount of the written bytes (a substring scan), 0 on every feasible RNA, positive on the infeasible one,
    # whose draws are the restatement's fallback (checked above: it is part of `want`)
    count = out["hits"].cpu().numpy()
    assert np.array_equal(count, _scan(got, name))
    assert (count[:, FEASIBLE] == 0).all() and (count[:, 4] > 0).all()
    assert np.array_equal(case["auto"][name].hits(out["seqs"]).cpu().numpy(), count)      # the user-facing check, on the device


# ---------------------------------------------------------------------------------------------------------------- 3, 4
def test_seq_nll_is_rnampnn_scores_byte_for_byte_in_both_layouts(case):
    from rnampnn.model.decode import score_logits
    for name in ("max_run3", "states64"):
        padded, packed = _run(case, name, 0.3), _run(case, name, 0.3, "packed")
        assert all(_bytes(padded[k]) == _bytes(packed[k]) for k in OUTPUTS), name
        sc = score_logits(case["logits"], mask=case["mask"], seqs=padded["seqs"], want=("seq_nll",))
        assert _bytes(padded["seq_nll"]) == _bytes(sc["seq_nll"])
        sc = score_logits(case["packed"], cu_seqlens=case["cu"], seqs=packed["seqs"], want=("seq_nll",))
        assert _bytes(packed["seq_nll"]) == _bytes(sc["seq_nll"])
        assert float(padded["seq_nll"][:, 0].abs().max()) == 0.0 and bool((padded["seq_nll"][:, 1:] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- 5
def test_an_rna_alone_equals_the_rna_inside_the_batch(case):
    """RNA 6 (fixed GGG between free positions) alone at its row, in a batch of another B and T whose other rows are empty and hold
    garbage; a device-side seed and a second call give the same bytes."""
    h, a = case["h"], case["auto"]["max_run3"]
    base = _run(case, "max_run3", 0.3)
    B2, T2, n = 8, 80, LENGTHS[6]
    rng = np.random.RandomState(5)
    logits = np.full((B2, T2, 4), np.nan, dtype=np.float32)
    allowed = rng.randint(0, 256, size=(B2, T2)).astype(np.uint8)
    bias = rng.standard_normal((B2, T2, 4)).astype(np.float32)
    mask = np.zeros((B2, T2), dtype=np.float32)
    logits[6, :n], allowed[6, :n], bias[6, :n], mask[6, :n] = h["logits"][6, :n], h["allowed"][6, :n], h["bias"][6, :n], 1
    one = design_avoid(logits, a.delta, a.n_states, a.terminal, mask=mask, allowed=allowed, bias=bias, temperature=0.3)
    assert _bytes(one["seqs"][:, 6, :n]) == _bytes(base["seqs"][:, 6, :n]) and bool((one["seqs"][:, 6, n:] == -1).all())
    assert all(_bytes(one[k][:, 6]) == _bytes(base[k][:, 6]) for k in ("seq_nll", "hits"))
    assert one["avoid_miss"].tolist() == [0] * B2 and int(one["infeasible"][6]) == 0
    assert bool((one["seqs"][:, [0, 1, 2, 3, 4, 5, 7]] == -1).all()) and int(one["hits"].abs().sum()) == 0
    assert bool((one["seqs"][:, 6, 20:23] == 3).all()) and bool((one["seqs"][:, 6, 19] != 3).all()) and bool((one["seqs"][:, 6, 23] != 3).all())
    seed_dev = torch.tensor([SEED], dtype=torch.int64, device="cuda")          # (the bits of a seed below 2^63)
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"])
    for other in (design_avoid(case["logits"], a.delta, a.n_states, a.terminal, **kw),
                  design_avoid(case["logits"], a.delta, a.n_states, a.terminal, seed=0, seed_dev=seed_dev, **kw)):
        assert all(_bytes(base[k]) == _bytes(other[k]) for k in OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_300_samples_cover_the_loop_over_chunks_and_the_first_4_are_the_call_with_4(case):
    """The 65-nt RNA at its row, S = 300 (five chunks of 64 samples, the last one partial): slots 0..3 are the S = 4 call's bytes, every
    slot holds no run longer than 3 and equals the restatement's draw of that slot where the margin allows."""
    a = case["auto"]["max_run3"]
    base = _run(case, "max_run3", 1.0)
    rows = slice(6, 7)
    mask = torch.zeros_like(case["mask"])
    mask[6] = case["mask"][6]
    out = design_avoid(case["logits"], a.delta, a.n_states, a.terminal, S=300, mask=mask, temperature=1.0, allowed=case["allowed"], bias=case["bias"])
    for k in ("seqs", "seq_nll", "hits"):
        assert _bytes(out[k][:4, rows]) == _bytes(base[k][:, rows]), k
    got = out["seqs"].cpu().numpy()[:, 6]
    assert int(out["hits"].abs().sum()) == 0 and _scan(got[None], "max_run3").sum() == 0 and (got[:, 65:] == -1).all()
    assert len(np.unique(got[:, :65], axis=0)) > 290              # the slots are independent draws, not copies of a chunk
    plan = _ref(case, "max_run3", 1.0)[5][6]
    for s in (4, 63, 64, 127, 128, 255, 256, 299):
        want, margin = plan.draw(SEED, s, 6)
        assert margin <= NEAR or np.array_equal(got[s, :65], want), s


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_a_one_state_automaton_equals_the_restatement(case, temperature):
    """delta = one row of zeros, no terminal state: no motif is reachable and the walk is rnampnn_design's draw in fp64."""
    h = case["h"]
    delta = np.zeros((1, 4), dtype=np.uint8)
    out = design_avoid(case["logits"], delta, 1, 0, mask=case["mask"], temperature=temperature, allowed=case["allowed"], bias=case["bias"])
    want, margin, bad, miss, hits, _ = R.design_avoid_ref(h["logits"], LENGTHS, temperature, S, SEED, delta, 0, set(), h["allowed"], h["bias"])
    got = out["seqs"].cpu().numpy()
    near = margin <= NEAR
    assert near.mean() <= 0.01 and out["avoid_miss"].tolist() == [0] * len(LENGTHS) and int(out["hits"].abs().sum()) == 0
    assert out["infeasible"].tolist() == R.CASE_INFEASIBLE
    assert all(near[s, b] or np.array_equal(got[s, b], want[s, b]) for s in range(S) for b in range(len(LENGTHS)))


# ---------------------------------------------------------------------------------------------------------------- 8
def test_the_largest_extent_that_fits_at_13_live_states_and_one_past_it():
    """One RNA of T_MAX_RUN3 nucleotides under max_run = 3 with G raised: the table fills the LDS a workgroup may ask for; no run longer
    than 3, the draw equals the restatement and the NLL bytes are rnampnn_score's.  One more nucleotide is NotImplementedError naming the
    bytes, the limit and the largest T, before any launch; so is T = 291 at 64 live states."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.decode import design_avoid_from_logits, score_logits
    a = _automaton("max_run3")
    n = T_MAX_RUN3
    rng = np.random.RandomState(11)
    logits = (3.0 * rng.standard_normal((1, n, 4))).astype(np.float32)
    logits[0, :, 3] += 6.0
    mask = np.ones((1, n), dtype=np.float32)
    out = design_avoid(logits, a.delta, a.n_states, a.terminal, mask=mask, S=2)
    want, margin, bad, miss, hits, _ = R.design_avoid_ref(logits, [n], 1.0, 2, SEED, a.delta.numpy(), a.terminal, R.expand((), 3))
    got = out["seqs"].cpu().numpy()
    print(f"T = {n}: margins {margin[:, 0]}")
    assert out["avoid_miss"].tolist() == [0] and out["hits"].tolist() == [[0], [0]] and _scan(got, "max_run3").sum() == 0
    assert all(margin[s, 0] <= NEAR or np.array_equal(got[s, 0], want[s, 0]) for s in range(2))
    sc = score_logits(torch.from_numpy(logits).cuda(), mask=torch.from_numpy(mask).cuda(), seqs=out["seqs"], want=("seq_nll",))
    assert _bytes(out["seq_nll"]) == _bytes(sc["seq_nll"])
    with pytest.raises(NotImplementedError, match=rf"T = {n + 1} with 13 live states needs 163928 bytes of LDS.*the limit is 163840 \(T <= {n} at this automaton\)"):
        design_avoid_from_logits(torch.zeros(1, n + 1, 4, device="cuda"), mask=torch.ones(1, n + 1, device="cuda"), n_samples=1, temperature=1.0,
                                 avoid=a)
    full = np.array([[min(s + 1, 63)] * 4 for s in range(64)], dtype=np.uint8)      # a chain of 64 live states
    ok = design_avoid(np.zeros((1, 290, 4), dtype=np.float32), full, 64, 0, mask=np.ones((1, 290), dtype=np.float32), S=1)
    assert ok["avoid_miss"].tolist() == [0] and ok["hits"].tolist() == [[0]]
    with pytest.raises(NotImplementedError, match=r"T = 291 with 64 live states.*\(T <= 290 at this automaton\)"):
        design_avoid(np.zeros((1, 291, 4), dtype=np.float32), full, 64, 0, mask=np.ones((1, 291), dtype=np.float32), S=1)


# ---------------------------------------------------------------------------------------------------------------- 9, 10
def test_every_bad_argument_and_the_partner_are_refused(case):
    from rnampnn import _native
    from rnampnn.model._base import _ptr, _stream
    a = case["auto"]["max_run3"]
    lg, m = case["logits"], case["mask"]
    B = len(LENGTHS)
    delta = a.delta.cuda()
    out = design_outputs(FURTHER, S, B, T)
    partner = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    for t in out.values():
        t.fill_(-7)
    keep = {k: t.clone() for k, t in out.items()}

    def call(logits=lg, mask=m, cu=None, B=B, T=T, temperature=1.0, S=S, delta=delta, n_states=a.n_states, terminal=a.terminal, partner=None):
        return _native.lib().rnampnn_design_avoid(_ptr(logits), B * T, _ptr(mask), _ptr(cu), B, T, float(temperature), S, C.c_uint64(SEED), None,
                                                  None, _ptr(partner), 1, None, 0, _ptr(delta), n_states, C.c_uint64(terminal),
                                                  *[_ptr(out[k]) for k in OUTPUTS], _stream(lg.device))
    BAD, UNSUPPORTED = 1, 2
    codes = {"ok": call()}
    torch.cuda.synchronize()
    assert codes["ok"] == 0 and not any(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)
    for t in out.values():
        t.fill_(-7)
    bad = dict(null_logits=call(logits=None), B0=call(B=0), T0=call(T=0), S0=call(S=0), S_big=call(S=65535), no_layout=call(mask=None),
               both_layouts=call(cu=case["cu"]), temperature0=call(temperature=0.0), temperature_nan=call(temperature=float("nan")),
               null_delta=call(delta=None), states0=call(n_states=0), states65=call(n_states=65), states_negative=call(n_states=-1),
               start_terminal=call(terminal=a.terminal | 1))
    assert bad == {k: BAD for k in bad}, bad
    assert call(partner=partner) == UNSUPPORTED
    with pytest.raises(NotImplementedError, match="base pairs .* are not built together with forbidden motifs.*4\\^depth"):
        _native.check(call(partner=partner))
    with pytest.raises(ValueError, match="state 0, the start, is marked terminal"):
        _native.check(call(terminal=1))
    torch.cuda.synchronize()
    assert all(_bytes(out[k]) == _bytes(keep[k]) for k in OUTPUTS)                 # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- 11
def test_stale_outputs_are_fully_overwritten_and_the_call_replays_from_a_graph(case):
    a = case["auto"]["overlap"]
    base = _run(case, "overlap", 0.3)
    out = design_outputs(FURTHER, S, len(LENGTHS), T)
    args = (case["logits"], a.delta.cuda(), a.n_states, a.terminal)
    kw = dict(mask=case["mask"], temperature=0.3, allowed=case["allowed"], bias=case["bias"], out=out)
    for fill in (-7, 99):
        for t in out.values():
            t.fill_(fill)
        design_avoid(*args, **kw)
        assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS), fill
    got = out["seqs"].cpu().numpy()
    assert all((got[:, b, n:] == -1).all() for b, n in enumerate(LENGTHS))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        design_avoid(*args, **kw)
    for t in out.values():
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_bytes(base[k]) == _bytes(out[k]) for k in OUTPUTS)


# ---------------------------------------------------------------------------------------------------------------- 12: the Python surface
MODEL_LENGTHS = [33, 20, 41]


def test_design_avoid_from_logits_in_both_layouts(case):
    from rnampnn.model.decode import design_avoid_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    a = case["auto"]["overlap"]
    cons = DesignConstraints(case["allowed"], None, case["bias"], True)
    want = _run(case, "overlap", 0.3)
    kw = dict(n_samples=S, temperature=0.3, seed=SEED, constraints=cons)
    for name, got in (("padded", design_avoid_from_logits(case["logits"], mask=case["mask"], avoid=a, **kw)),
                      ("packed", design_avoid_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, avoid=a, **kw)),
                      ("strings", design_avoid_from_logits(case["logits"], mask=case["mask"], avoid=R.CASE_AUTOMATA["overlap"][0], **kw))):
        assert len(got) == 5 and [t.dtype for t in got] == [torch.int8, torch.float32, torch.int32, torch.int32, torch.int32]
        for t, k in zip(got, OUTPUTS):
            assert _bytes(t) == _bytes(want[k]), (name, k)


def test_both_models_design_without_gggg():
    import __graft_entry__ as g
    g.build()
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.data import pad_batch
    from rnampnn.utils.motifs import MotifAutomaton
    torch.manual_seed(0)
    m = RNAMPNN(precision="f32", **SMALL).cuda().eval()
    items = [(synth.synth_rna(n, i, seed=1), synth.synth_labels(n, i, seed=1)) for i, n in enumerate(MODEL_LENGTHS)]
    _, c, mask, lens = pad_batch(items, pin=False)
    c, mask = c.cuda(), mask.cuda()
    words = R.expand(["GGGG"])
    bias = DesignConstraints.from_specs([(None, None)] * 3, lens, int(mask.shape[1]), bias=[0.0, 0.0, 0.0, 4.0])      # G favoured: free draws hold GGGG
    free = m.design(c, mask, n_samples=4, temperature=1.0, seed=3, constraints=bias)
    assert len(m.design(c, mask, n_samples=4, temperature=1.0, seed=3)) == 2                # None keeps today's paths and return values
    assert sum(R.naive_hits(row, words) for plane in free[0].cpu().numpy() for row in plane) > 0
    out = m.design(c, mask, n_samples=4, temperature=1.0, seed=3, constraints=bias, avoid=["GGGG"])
    assert len(out) == 5 and out[0].shape == (4, 3, max(lens)) and out[3].abs().sum().item() == 0 and out[4].tolist() == [0, 0, 0]
    assert sum(R.naive_hits(row, words) for plane in out[0].cpu().numpy() for row in plane) == 0
    assert _bytes(out[1]) == _bytes(m.score_sequences(c, mask, out[0])[0])
    auto = MotifAutomaton.from_motifs(["GGGG"])
    assert _bytes(m.design(c, mask, n_samples=4, temperature=1.0, seed=3, constraints=bias, avoid=auto)[0]) == _bytes(out[0])
    assert MotifAutomaton.from_motifs(["GGGG"]).hits(out[0]).abs().sum().item() == 0
    fixed = DesignConstraints.from_specs([("GGGG" + "." * 29, None), (None, None), (None, None)], lens, int(mask.shape[1]))
    out = m.design(c, mask, n_samples=2, temperature=1.0, seed=3, constraints=fixed, avoid=["GGGG"])
    assert out[4].tolist() == [1, 0, 0] and bool((out[3][:, 0] >= 1).all()) and out[3][:, 1:].abs().sum().item() == 0
    paired = DesignConstraints.from_specs([(None, "((((....))))" + "." * 21), (None, None), (None, None)], lens, int(mask.shape[1]))
    with pytest.raises(ValueError, match="drop `structure`"):
        m.design(c, mask, n_samples=2, constraints=paired, avoid=["GGGG"])
    with pytest.raises(ValueError, match="avoid together with gc_content is not built"):
        m.design(c, mask, n_samples=2, gc_content=(0.4, 0.6), avoid=["GGGG"])
    r = RNAModel(num_mpnn_layers=1).cuda().eval()
    X = torch.zeros(len(MODEL_LENGTHS), max(MODEL_LENGTHS), 6, 3)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
    X = X.cuda()
    out = r.design(X, mask, n_samples=4, temperature=1.0, seed=5, lengths=MODEL_LENGTHS, constraints=bias, avoid=["GGGG"])
    assert len(out) == 5 and out[0].shape == (4, 3, max(lens)) and out[3].abs().sum().item() == 0 and out[4].tolist() == [0, 0, 0]
    assert sum(R.naive_hits(row, words) for plane in out[0].cpu().numpy() for row in plane) == 0
    assert _bytes(out[1]) == _bytes(r.score_sequences(X, mask, out[0])[0])
    assert len(r.design(X, mask, n_samples=2, temperature=1.0, seed=5, lengths=MODEL_LENGTHS)) == 3


@pytest.mark.parametrize("family", ["rnampnn", "rdesign"])
def test_predict_cli_with_forbidden_motifs(family, tmp_path):
    """--avoid / --max-run add the columns motif_hits and avoid_miss; no written design holds a motif or a run longer than 2 although G is
    favoured; the designs file written without the flags is byte for byte the same before and after."""
    import __graft_entry__ as g
    g.build()
    import predict as P
    ids, lens = ["r2", "r0", "r1"], MODEL_LENGTHS
    _write_data(tmp_path / "data", ids, lens)
    ck = str(tmp_path / "model.pt")
    _checkpoint(family, ck)
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", str(tmp_path / "submit.csv"), "--samples", "3", "--temperature", "1.0",
              "--batch-size", "2", "--bias", "G=3"]
    quiet = dict(log=lambda *a: None)
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "before.csv")]), **quiet)
    before = list(csv.reader(open(tmp_path / "before.csv")))
    assert any("GGG" in r[2] for r in before[1:])                  # what the flags are there to prevent
    des = str(tmp_path / "avoid.csv")
    P.run(P.parse(common + ["--designs-out", des, "--avoid", "GAAUUC,ACGT", "--max-run", "2"]), **quiet)
    d = list(csv.reader(open(des)))
    assert d[0] == ["pdb_id", "sample", "seq", "nll_per_nt", "recovery", "infeasible", "motif_hits", "avoid_miss"] and len(d) == 1 + 3 * 3
    for r in d[1:]:
        assert len(r[2]) == lens[ids.index(r[0])] and r[-1] == "0" and r[-2] == "0", r
        assert not any(w in r[2] for w in ("GAAUUC", "ACGU", "AAA", "UUU", "CCC", "GGG")), r
    P.run(P.parse(common + ["--designs-out", str(tmp_path / "after.csv")]), **quiet)
    assert open(tmp_path / "before.csv", "rb").read() == open(tmp_path / "after.csv", "rb").read()
    (tmp_path / "cons.csv").write_text("pdb_id,fixed,structure\nr2," + "." * 33 + ",((((....))))" + "." * 21 + "\n")
    with pytest.raises(ValueError, match="drop `structure` from the constraints of \\['r2'\\]"):
        P.run(P.parse(common + ["--avoid", "GGGG", "--constraints", str(tmp_path / "cons.csv")]), **quiet)
