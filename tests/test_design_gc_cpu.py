"""Host side of design under a G+C content window (``rnampnn_design_gc``): the float64 restatement the device tests compare against
(tests/_design_gc_ref.py) is itself checked - its conditionals multiply to the brute-force conditioned joint, its draws follow the analytic
conditional, its own cold draw is the max-plus optimum, and few of its draws of the device tests' batch pass near a cumulative boundary -
then the fractions-to-counts rule, every ``ValueError``, the ABI's argument errors (no launch happens, so no GPU is needed) and
predict.py's flag."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _design_gc_ref as G  # noqa: E402
from _design_ref import PAIRS  # noqa: E402


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from rnampnn import _native
    return _native


# ---------------------------------------------------------------------------------------------------------------- the restatement is exact
def _brute_force(z, mask, partner, wobble, lo, hi):
    """Every sequence the constraints admit with its weight exp(sum z), by enumeration, written independently of GcPlan: an empty mask is
    free, a pair without an admitted compatible cell is two single positions.  -> {sequence: probability given G+C in [lo, hi]}."""
    n = len(mask)
    mask = [m or 15 for m in mask]
    pairs = []
    for t in range(n):
        j = partner[t]
        if t < j < n and partner[j] == t and any((mask[t] >> a) & 1 and (mask[j] >> c) & 1 for a, c in PAIRS[wobble]):
            pairs.append((t, j))
    joint = {}
    for seq in itertools.product(range(4), repeat=n):
        if all((mask[t] >> seq[t]) & 1 for t in range(n)) and all((seq[i], seq[j]) in PAIRS[wobble] for i, j in pairs):
            if lo <= sum(c >= 2 for c in seq) <= hi:
                joint[seq] = float(np.exp(sum(z[t, seq[t]] for t in range(n))))
    tot = sum(joint.values())
    return {k: v / tot for k, v in joint.items()}


def test_conditionals_multiply_to_the_brute_force_conditioned_joint():
    """12 random cases of 3..7 nucleotides with pairs, masks (an empty one, IUPAC sets, fixed ends), both wobble settings and windows: the
    product of the conditionals along the path of EVERY admissible sequence equals joint / (mass of the window) to 1e-12 (the prototype of
    the method measured 2.9e-15), and a sequence outside the window or the constraints has no path."""
    rng = np.random.RandomState(7)
    worst, cases = 0.0, 0
    while cases < 12:
        n = 3 + cases % 5
        logits = (2.0 * rng.standard_normal((n, 4))).astype(np.float32)
        temp = float(np.float32(rng.choice([1.0, 0.5])))
        wobble = bool(cases % 2)
        mask = [int(v) for v in rng.choice([15, 15, 15, 3, 12, 9, 6, 1, 8, 0], size=n)]
        perm = rng.permutation(n)
        partner = [-1] * n
        for k in range(rng.randint(0, n // 2 + 1)):
            i, j = int(perm[2 * k]), int(perm[2 * k + 1])
            partner[i], partner[j] = j, i
        lo = int(rng.randint(0, n + 1))
        hi = int(rng.randint(lo, n + 1))
        plan = G.GcPlan(logits, n, temp, lo, hi, np.array(mask, dtype=np.uint8), np.array(partner, dtype=np.int32), wobble)
        if plan.miss:
            continue                                               # an unreachable window is the subject of the next test
        want = _brute_force(logits.astype(np.float64) / temp, mask, partner, wobble, lo, hi)
        assert want, "a reachable window admits a sequence"
        total = 0.0
        for seq in itertools.product(range(4), repeat=n):
            lp = plan.path_logprob(seq)
            if seq in want:
                worst = max(worst, abs(np.exp(lp) - want[seq]))
                total += np.exp(lp)
            else:
                assert lp == -np.inf, (cases, seq)
        assert abs(total - 1.0) < 1e-12
        cases += 1
    print(f"largest |product of conditionals - conditioned joint| over 12 cases: {worst:.3e}")
    assert worst < 1e-12


def test_unreachable_windows_go_to_the_nearest_reachable_count_the_lower_on_a_tie():
    logits = np.zeros((6, 4), dtype=np.float32)
    fixed = lambda text: np.array([1 << "AUCG".index(ch) if ch != "N" else 15 for ch in text], dtype=np.uint8)
    p = G.GcPlan(logits, 6, 1.0, 1, 6, fixed("AAAAAA"))
    assert (p.miss, p.target) == (1, 0)
    p = G.GcPlan(logits, 6, 1.0, 0, 1, fixed("GGGCNA"))
    assert (p.miss, p.target) == (3, 4)
    # a GC pair and four fixed A: reachable counts {2}; the window (0, 0) -> 2, miss 2.  AU/GC pair alone: counts {0, 2}, window (1, 1): tie -> 0
    partner = np.array([1, 0, -1, -1, -1, -1], dtype=np.int32)
    p = G.GcPlan(logits, 6, 1.0, 0, 0, fixed("GCAAAA"), partner)
    assert (p.miss, p.target) == (2, 2)
    p = G.GcPlan(logits, 6, 1.0, 1, 1, fixed("NNAAAA"), partner, wobble=False)
    assert (p.miss, p.target) == (1, 0)
    assert [int(c >= 2) for c in p.draw(5, 0, 0)[0]] == [0] * 6
    # lo and hi are clamped to [0, n], then hi = max(hi, lo)
    p = G.GcPlan(logits, 6, 1.0, -5, 100000)
    assert (p.lo, p.hi, p.miss) == (0, 6, 0)
    p = G.GcPlan(logits, 6, 1.0, 4, 2)
    assert (p.lo, p.hi, p.miss) == (4, 4, 0)
    p = G.GcPlan(logits, 0, 1.0, 3, 5)
    assert (p.lo, p.hi, p.miss) == (0, 0, 0) and p.draw(1, 0, 0)[0].shape == (0,)


def test_draw_frequencies_follow_the_analytic_conditional():
    """20,000 draws of one 12-mer with two pairs under the window (4, 7): no draw falls outside it, and every count's frequency lies within
    5 binomial standard deviations of the analytic conditional (the polynomial product over the units, in plain float64 arithmetic)."""
    S, n, lo, hi = 20000, 12, 4, 7
    rng = np.random.RandomState(3)
    logits = (1.5 * rng.standard_normal((n, 4))).astype(np.float32)
    partner = np.full(n, -1, dtype=np.int32)
    for i, j in ((0, 11), (3, 8)):
        partner[i], partner[j] = j, i
    plan = G.GcPlan(logits, n, 0.9, lo, hi, None, partner, True)
    z = logits.astype(np.float64) / float(np.float32(0.9))
    poly = np.ones(1)
    for t in range(n):
        if partner[t] < 0:
            poly = np.convolve(poly, [np.exp(z[t, 0]) + np.exp(z[t, 1]), np.exp(z[t, 2]) + np.exp(z[t, 3])])
        elif partner[t] > t:
            unit = np.zeros(3)
            for a, c in PAIRS[True]:
                unit[(a >= 2) + (c >= 2)] += np.exp(z[t, a] + z[partner[t], c])
            poly = np.convolve(poly, unit)
    want = poly[lo:hi + 1] / poly[lo:hi + 1].sum()
    counts = np.zeros(n + 1, dtype=np.int64)
    for s in range(S):
        seq, _ = plan.draw(99, s, 0, margins=False)
        assert all((int(seq[i]), int(seq[j])) in PAIRS[True] for i, j in ((0, 11), (3, 8)))
        counts[int((seq >= 2).sum())] += 1
    assert counts[:lo].sum() == 0 and counts[hi + 1:].sum() == 0
    for k, p in zip(range(lo, hi + 1), want):
        sd = np.sqrt(p * (1 - p) / S)
        print(f"G+C = {k}: frequency {counts[k] / S:.5f} analytic {p:.5f} ({abs(counts[k] / S - p) / sd:.2f} sd)")
        assert abs(counts[k] / S - p) <= 5 * sd, k


def test_few_reference_draws_of_the_device_batch_pass_near_a_boundary():
    """The device differs from the restatement by last-bit exp / log and by reassociation over about 10 levels, about 1e-12 relative; the
    device tests leave out the draws whose path has a selection within 1e-8 of a cumulative boundary.  For the restatement alone that share
    is at most 1 % at both temperatures (a seed that violates this is to be changed)."""
    for temperature in (1.0, 0.3):
        margin = G.case_ref(temperature)[1]
        share = float((margin <= 1e-8).mean())
        print(f"temperature {temperature}: {share:.4%} of the (sample, RNA) draws within 1e-8 of a boundary, smallest margin {margin.min():.3e}")
        assert share <= 0.01


def test_the_restatements_own_cold_draw_is_the_max_plus_optimum():
    """At temperature 1e-3 an alternative whose sum of (logit + bias) falls short by more than 0.05 carries a weight below e^-50: the
    restatement's draw of every RNA of the device batch lies within 0.05 of the max-plus optimum over the window (or its target)."""
    h = G.case_arrays()
    seqs, _, _, _, _ = G.case_ref(1e-3)
    zb = h["logits"].astype(np.float64) + G.CASE_BIAS.astype(np.float64)
    for b, n in enumerate(G.CASE_LENGTHS):
        best = G.GcPlan(h["logits"][b], n, 1.0, h["lo"][b], h["hi"][b], h["allowed"][b], h["partner"][b], True, G.CASE_BIAS, maxplus=True)
        if n == 0:
            continue
        for s in range(G.CASE_S):
            got = float(sum(zb[b, t, seqs[s, b, t]] for t in range(n)))
            assert best.optimum() - 0.05 <= got <= best.optimum() + 1e-9, (b, s, got, best.optimum())


# ---------------------------------------------------------------------------------------------------------------- fractions -> counts
def test_fractions_become_counts_with_a_slack_of_1e_6():
    from rnampnn.model.decode import gc_counts, gc_fractions
    lengths = torch.tensor([0, 1, 12, 12, 10, 300, 7])
    fr = torch.tensor([[0.0, 1.0], [0.4, 0.6], [0.5, 0.5], [0.45, 0.6], [0.3, 0.7], [0.4, 0.6], [1 / 7, 3 / 7]], dtype=torch.float64)
    lo, hi = gc_counts(gc_fractions(fr, 7), lengths)
    assert lo.dtype == hi.dtype == torch.int32
    # 0.4 * 1 -> ceil = 1 > floor(0.6) = 0: an empty window of counts is the kernel's lo > hi case (read as lo); 0.3 * 10 = 3 exactly
    assert lo.tolist() == [0, 1, 6, 6, 3, 120, 1] and hi.tolist() == [0, 0, 6, 7, 7, 180, 3]
    for lo_f, hi_f in ((0.1, 0.3), (0.7, 0.9)):                    # 0.1 * 30 and 0.7 * 10 are not exact in binary: the slack keeps 3 and 7
        lo, hi = gc_counts(gc_fractions((lo_f, hi_f), 2), torch.tensor([30, 10]))
        assert lo.tolist() == [round(lo_f * 30), round(lo_f * 10)] and hi.tolist() == [round(hi_f * 30), round(hi_f * 10)]
    assert gc_fractions((0.25, 0.75), 3).tolist() == [[0.25, 0.75]] * 3


@pytest.mark.parametrize("value, text", [((-0.1, 0.5), r"\[0, 1\]"), ((0.2, 1.5), r"\[0, 1\]"), ((0.6, 0.4), "lo > hi"),
                                         ((float("nan"), 0.5), r"\[0, 1\]"), ((0.1, 0.2, 0.3), "pair"),
                                         (torch.tensor([[0.1, 0.5], [0.7, 0.2]]), "lo > hi"), (torch.zeros(3, 2), "pair")])
def test_bad_fractions_are_value_errors(value, text):
    from rnampnn.model.decode import gc_fractions
    with pytest.raises(ValueError, match=text):
        gc_fractions(value, 2)


def test_design_gc_refuses_host_logits_and_the_models_refuse_states():
    from rdesign.model.rdesign import RNAModel
    from rnampnn.model.decode import design_gc_from_logits
    from rnampnn.model.rnampnn import RNAMPNN
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        design_gc_from_logits(torch.zeros(1, 4, 4), mask=torch.ones(1, 4), n_samples=1, temperature=1.0, gc_content=(0.0, 1.0))
    for cls in (RNAMPNN, RNAModel):                                # the refusal comes before anything touches the device
        with pytest.raises(ValueError, match="gc_content together with states is not built"):
            cls.design(None, torch.zeros(2, 4, 7, 3), torch.ones(2, 4), states=[2], gc_content=(0.4, 0.6))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_rnampnn_design_gc(native):
    text = open(os.path.join(REPO, "include", "rnampnn_hip.h")).read()
    assert int(re.search(r"#define\s+RNAMPNN_DESIGN_GC_SALT\s+(0x[0-9A-Fa-f]+)ull", text).group(1), 16) == G.SALT
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+rnampnn_design_gc\s*\(([^;]*)\)\s*;", text)
    assert m, "include/rnampnn_hip.h does not declare rnampnn_design_gc"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert "rnampnn_design_gc" in native.SYMBOLS and len(native.SYMBOLS["rnampnn_design_gc"][1]) == n_params == 23
    assert hasattr(native.lib(), "rnampnn_design_gc")
    import __graft_entry__ as g
    assert "design_gc.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "design_gc.hip"))


def _call(native, **kw):
    """rnampnn_design_gc with made-up (never dereferenced) addresses: every case below must return before a launch."""
    a = dict(logits=0x1000, n_rows=64, mask=0x2000, cu=None, B=2, T=8, temperature=1.0, S=4, seed=1, seed_dev=None, allowed=None, partner=None,
             wobble=1, bias=None, per_position=0, gc_lo=0x7000, gc_hi=0x8000, seqs=0x3000, seq_nll=0x4000, infeasible=0x5000, gc_count=0x9000,
             gc_miss=0xA000)
    a.update(kw)
    vp = lambda v: None if v is None else C.c_void_p(v)
    return native.lib().rnampnn_design_gc(vp(a["logits"]), a["n_rows"], vp(a["mask"]), vp(a["cu"]), a["B"], a["T"], a["temperature"], a["S"],
                                          C.c_uint64(a["seed"]), vp(a["seed_dev"]), vp(a["allowed"]), vp(a["partner"]), a["wobble"],
                                          vp(a["bias"]), a["per_position"], vp(a["gc_lo"]), vp(a["gc_hi"]), vp(a["seqs"]), vp(a["seq_nll"]),
                                          vp(a["infeasible"]), vp(a["gc_count"]), vp(a["gc_miss"]), None)


@pytest.mark.parametrize("kw, text", [
    (dict(logits=None), "null logits"),
    (dict(B=0), "empty batch"), (dict(B=-3), "empty batch"), (dict(T=0), "empty batch"),
    (dict(gc_lo=None), "null gc_lo or gc_hi"), (dict(gc_hi=None), "null gc_lo or gc_hi"),
    (dict(S=0), "S = 0"), (dict(S=-1), "S = -1"),
    (dict(S=65535), "at most 65534"),
    (dict(mask=None, cu=None), "exactly one of mask"), (dict(cu=0x6000), "exactly one of mask"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("inf")), "temperature"), (dict(temperature=float("nan")), "temperature"),
    (dict(logits=0x1004), "16-byte aligned"),
    (dict(bias=0x6004, per_position=1), "16-byte aligned"),
    (dict(mask=None, cu=0x6000, n_rows=-1), "negative row count"),
])
def test_argument_errors_are_value_errors_before_any_launch(native, kw, text):
    rc = _call(native, **kw)
    assert rc == native.ERR_BAD_ARG
    with pytest.raises(ValueError, match=text):
        native.check(rc)


def test_a_call_with_every_output_null_returns_ok_without_a_launch(native):
    none = dict(seqs=None, seq_nll=None, infeasible=None, gc_count=None, gc_miss=None)
    assert _call(native, **none) == 0
    assert _call(native, S=65534, T=100000, **none) == 0


def test_a_padded_extent_past_the_lds_limit_is_unsupported_and_names_the_limit(native):
    """The size check precedes the launch, so it needs no GPU: T = 1018 needs 163,960 bytes, 1017 is the largest extent that fits."""
    rc = _call(native, T=1018)
    with pytest.raises(NotImplementedError, match=r"T = 1018 needs 163960 bytes .* the limit is 163840 \(T <= 1017\)"):
        native.check(rc)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_predict_parses_gc_content_and_refuses_states():
    import predict
    from rnampnn.utils.constraints import parse_gc_content
    base = ["--ckpt", "x.pt", "--data", "d"]
    p = predict.parse(base)
    assert p.gc_content is None and predict.gc_option(p) == {} and predict.design_options(p) == {}
    p = predict.parse(base + ["--samples", "2", "--gc-content", "0.45:0.6", "--omit", "U", "--no-wobble", "--bias", "G=-1"])
    assert predict.gc_option(p) == {"gc_content": (0.45, 0.6)} and predict.design_options(p)["omit"] == "U"
    assert parse_gc_content("0:1") == (0.0, 1.0) and parse_gc_content(" .5 : .5 ") == (0.5, 0.5)
    for bad in ("0.5", "0.6:0.4", "-0.1:0.5", "0.2:1.2", "a:b", "0.1:0.2:0.3", ":", "nan:0.5"):
        with pytest.raises(ValueError, match="gc-content"):
            parse_gc_content(bad)
    with pytest.raises(ValueError, match="--gc-content.*--states"):
        predict.gc_option(predict.parse(base + ["--samples", "2", "--gc-content", "0.4:0.6", "--states", "s.csv"]))
    with pytest.raises(ValueError, match="--gc-content needs --samples"):
        predict.gc_option(predict.parse(base + ["--gc-content", "0.4:0.6"]))
    with pytest.raises(ValueError, match="--gc-content.*--states"):   # run() refuses before it opens the checkpoint
        predict.run(predict.parse(["--ckpt", "/nonexistent.pt", "--data", "d", "--samples", "2", "--gc-content", "0.4:0.6", "--states", "s.csv"]))
