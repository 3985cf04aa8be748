"""``rnampnn_score`` (csrc/score.hip) on the device: against ``rnampnn_argmax_recovery`` bit for bit, against float64 torch on the same
logits within the project's NLL bound, packed == padded byte for byte, reproducible, blind to everything beyond an RNA's length, and
every argument error a ``ValueError``.  One padded batch holds every length at which the kernel's loop changes shape: 1, one short of /
exactly / one over a wave, one over the 256-thread workgroup, T itself, and an empty RNA."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rna-mpnn_amd"))

LENGTHS = [1, 63, 64, 65, 257, 300, 0]
T = 300
ALL = ("valid", "pred", "correct", "label_nll", "label_loss", "seq_nll", "seq_match")


def _nll_bound(sum64, n):
    """tests/test_rdesign_trainer_gpu.py: _nll_bound - f32 expf / logf are good to a few ulp and a fixed-order f32 sum of n terms carries
    a relative error of about (log2 n + 4) * 2^-24 ~ 1e-6; the bound leaves a factor of 8 over that."""
    return 1e-5 * abs(sum64) + 1e-6 * n


@pytest.fixture(scope="module")
def case():
    """Inputs on the device + the float64 reference, computed once and never written to."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.rnampnn import sample_from_logits
    B = len(LENGTHS)
    gen = torch.Generator().manual_seed(23)
    logits = 3.0 * torch.randn(B, T, 4, generator=gen)
    # first-maximum ties and a flat row, inside RNAs that span more than one wave
    logits[4, 3] = torch.tensor([1.5, 1.5, 0.0, -1.0]); logits[4, 200] = torch.tensor([0.0, 2.0, 2.0, -1.0])
    logits[5, 256] = torch.tensor([3.0, 0.0, 3.0, 3.0]); logits[5, 299] = torch.tensor([0.25, 0.25, 0.25, 0.25])
    logits[0, 0] = torch.tensor([-2.0, -2.0, -2.0, -2.0])
    mask = torch.zeros(B, T)
    labels = torch.zeros(B, T, dtype=torch.int32)
    for b, n in enumerate(LENGTHS):
        mask[b, :n] = 1
        labels[b, :n] = torch.randint(0, 4, (n,), generator=gen, dtype=torch.int32)
    logits = logits * mask[..., None]                              # what the forward writes: zero on padded rows
    d = dict(B=B, logits=logits.cuda(), mask=mask.cuda(), labels=labels.cuda())
    d["seqs"] = sample_from_logits(d["logits"], d["mask"], 1.0, 3, seed=5)          # (3, B, T) int8, -1 on padding
    # packed layout of the same rows
    valid = mask.bool()
    d["packed"] = logits[valid].contiguous().cuda()
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(LENGTHS), 0)
    d["cu"] = cu.cuda()
    # float64 reference on the SAME f32 logits
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    pick = lambda ids: torch.gather(x, 2, ids.long().clamp(min=0)[..., None])[..., 0]
    d["ref_nll"] = ((lse - pick(labels)) * mask.double()).sum(1)
    p = torch.softmax(x, dim=-1)                                   # mix_loss: cross-entropy applied to the probabilities
    lsp = torch.log_softmax(p, dim=-1)
    d["ref_loss"] = (-torch.gather(lsp, 2, labels.long()[..., None])[..., 0] * mask.double()).sum(1)
    seqs = d["seqs"].cpu()
    d["ref_seq_nll"] = torch.stack([((lse - pick(seqs[s])) * mask.double()).sum(1) for s in range(3)])
    d["ref_seq_match"] = torch.stack([((seqs[s].int() == labels) & valid).sum(1) for s in range(3)]).to(torch.int32)
    return d


def _score(case, S=3, layout="padded", **kw):
    from rnampnn.model.rnampnn import score_logits
    seqs = case["seqs"][:S] if S else None
    want = tuple(n for n in ALL if S or not n.startswith("seq_"))
    args = dict(labels=case["labels"], seqs=seqs, want=want)
    args.update(kw)
    if layout == "padded":
        return score_logits(case["logits"], mask=case["mask"], **args)
    return score_logits(case["packed"], cu_seqlens=case["cu"], **args)


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("S", [1, 3])
def test_counts_equal_argmax_recovery_and_sums_meet_the_float64_bound(case, S):
    from rnampnn.model.rnampnn import argmax_recovery
    out = _score(case, S)
    pred, correct, valid = argmax_recovery(case["logits"], case["mask"], case["labels"])
    assert out["pred"].dtype == torch.int8 and _bytes(out["pred"]) == _bytes(pred)
    assert _bytes(out["correct"]) == _bytes(correct) and _bytes(out["valid"]) == _bytes(valid)
    assert out["valid"].tolist() == LENGTHS
    assert out["pred"][4, 3] == 0 and out["pred"][4, 200] == 1 and out["pred"][5, 256] == 0 and out["pred"][5, 299] == 0
    assert out["seq_nll"].shape == (S, case["B"]) and out["seq_match"].shape == (S, case["B"])
    assert torch.equal(out["seq_match"].cpu(), case["ref_seq_match"][:S])
    for b, n in enumerate(LENGTHS):
        rows = [("label_nll", float(out["label_nll"][b]), float(case["ref_nll"][b])),
                ("label_loss", float(out["label_loss"][b]), float(case["ref_loss"][b]))]
        rows += [(f"seq_nll[{s}]", float(out["seq_nll"][s, b]), float(case["ref_seq_nll"][s, b])) for s in range(S)]
        for name, got, want in rows:
            print(f"RNA {b} n {n} {name}: {got:.6f} f64 {want:.6f} |d| {abs(got - want):.3e} bound {_nll_bound(want, n):.3e}")
            assert abs(got - want) <= _nll_bound(want, n), (b, name)
    # the empty RNA: zeros everywhere, -1 over its whole pred row
    e = LENGTHS.index(0)
    assert float(out["label_nll"][e]) == 0.0 and float(out["label_loss"][e]) == 0.0 and int(out["correct"][e]) == 0
    assert float(out["seq_nll"][:, e].abs().sum()) == 0.0 and int(out["seq_match"][:, e].sum()) == 0 and bool((out["pred"][e] == -1).all())
    # a sequence scored as labels and as a candidate takes the same path through the reduction: the same bytes
    as_labels = _score(case, 0, labels=case["seqs"][0].to(torch.int32).clamp(min=0), want=("label_nll",))
    assert _bytes(as_labels["label_nll"]) == _bytes(out["seq_nll"][0])


@pytest.mark.parametrize("S", [1, 3])
def test_packed_equals_padded_and_a_second_call_gives_the_same_bytes(case, S):
    a, b, c = _score(case, S), _score(case, S), _score(case, S, layout="packed")
    for name in ALL:
        assert _bytes(a[name]) == _bytes(b[name]), name
        assert _bytes(a[name]) == _bytes(c[name]), name
    # the packed layout takes T from max_len too, and needs neither labels nor seqs for the decode
    from rnampnn.model.rnampnn import score_logits
    d = score_logits(case["packed"], cu_seqlens=case["cu"], want=("pred", "valid"), max_len=T)
    assert _bytes(d["pred"]) == _bytes(a["pred"]) and _bytes(d["valid"]) == _bytes(a["valid"])


def test_nothing_beyond_an_rnas_length_is_read_and_nothing_beyond_an_output_is_written(case):
    from rnampnn.model.rnampnn import SCORE_OUTPUTS, score_logits
    S, B = 3, case["B"]
    clean = _score(case, S)
    m = case["mask"]
    logits = torch.where(m[..., None] != 0, case["logits"], torch.full_like(case["logits"], float("nan")))
    logits[:, :, 0] = torch.where(m != 0, logits[:, :, 0], torch.full_like(m, 1e30))
    labels = torch.where(m != 0, case["labels"], torch.full_like(case["labels"], 77))
    seqs = torch.where(m[None] != 0, case["seqs"], torch.full_like(case["seqs"], 99))
    # every output sits in the middle of a longer allocation filled with a guard pattern
    shapes = {n: tuple(clean[n].shape) for n in ALL}
    pad, guard = 64, {torch.int32: 0x5A5A5A5A, torch.int8: 0x5A, torch.float32: -7.25}
    store, out = {}, {}
    for n in ALL:
        numel = int(torch.tensor(shapes[n]).prod())
        store[n] = torch.full((numel + 2 * pad,), guard[SCORE_OUTPUTS[n]], dtype=SCORE_OUTPUTS[n], device="cuda")
        out[n] = store[n][pad: pad + numel].view(shapes[n])
    dirty = score_logits(logits, mask=m, labels=labels, seqs=seqs, want=ALL, out=out)
    for n in ALL:
        assert dirty[n] is out[n]
        assert _bytes(dirty[n]) == _bytes(clean[n]), n
        assert bool((store[n][:pad] == guard[SCORE_OUTPUTS[n]]).all()) and bool((store[n][-pad:] == guard[SCORE_OUTPUTS[n]]).all()), n
    # packed: garbage in the rows beyond cu[B] of a longer logits tensor
    big = torch.full((case["packed"].shape[0] + 100, 4), float("nan"), device="cuda")
    big[: case["packed"].shape[0]] = case["packed"]
    p = score_logits(big, cu_seqlens=case["cu"], labels=labels, seqs=seqs, want=ALL)
    for n in ALL:
        assert _bytes(p[n]) == _bytes(clean[n]), n


def test_a_malformed_mask_or_cu_stays_inside_the_tensors(case):
    """Lengths and cu are clamped to the extents: the numbers mean nothing, the call returns and every count stays within [0, T]."""
    from rnampnn.model.rnampnn import score_logits
    B = case["B"]
    m = torch.full((B, T), 5.0, device="cuda")                      # sums to 5 T
    m[1] = -3.0
    m[2, ::2] = 0.0                                                 # not a prefix
    out = score_logits(case["logits"], mask=m, labels=case["labels"], seqs=case["seqs"], want=ALL)
    v = out["valid"].tolist()
    assert v[0] == T and v[1] == 0 and all(0 <= n <= T for n in v)
    cu = torch.tensor([-5, 40, 20, 10_000, 10_001, 10_002, -7, 3], dtype=torch.int32, device="cuda")
    out = score_logits(case["packed"], cu_seqlens=cu, labels=case["labels"], seqs=case["seqs"], want=ALL)
    v = out["valid"].tolist()
    assert v == [45, 0, T, 0, 0, 0, 10] and all(0 <= int(c) <= n for c, n in zip(out["correct"].tolist(), v))
    assert bool(torch.isfinite(out["label_nll"]).all())


def test_argument_errors_raise_value_error(case):
    from rnampnn.model.rnampnn import score_logits
    lg, m, cu, lab, sq = case["logits"], case["mask"], case["cu"], case["labels"], case["seqs"]
    with pytest.raises(ValueError, match="exactly one of mask"):
        score_logits(lg, labels=lab, max_len=T)                                     # neither
    with pytest.raises(ValueError, match="exactly one of mask"):
        score_logits(lg, mask=m, cu_seqlens=cu, labels=lab)                         # both
    off = torch.zeros(lg.numel() + 4, device="cuda")[1:1 + lg.numel()].view(lg.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        score_logits(off, mask=m, labels=lab)
    with pytest.raises(ValueError, match="S = -1"):
        score_logits(lg, mask=m, labels=lab, seqs=sq, n_seqs=-1, want=("valid",))
    with pytest.raises(ValueError, match="need seqs"):
        score_logits(lg, mask=m, labels=lab, want=("seq_nll",))
    with pytest.raises(ValueError, match="need seqs"):
        score_logits(lg, mask=m, labels=lab, want=("seq_match",))
    with pytest.raises(ValueError, match="need labels"):
        score_logits(lg, mask=m, want=("correct",))
    with pytest.raises(ValueError, match="need labels"):
        score_logits(lg, mask=m, seqs=sq, want=("seq_match",))
    with pytest.raises(ValueError, match="need labels"):
        score_logits(lg, mask=m, want=("label_loss",))
    with pytest.raises(ValueError):
        score_logits(lg, mask=m, labels=lab[:, :10])                                # labels of another extent
    with pytest.raises(ValueError):
        score_logits(lg, mask=m, labels=lab, want=("nll",))                         # an output that does not exist
    # what needs no labels works without them
    out = score_logits(lg, mask=m, seqs=sq, want=("valid", "pred", "seq_nll"))
    assert out["valid"].tolist() == LENGTHS and out["seq_nll"].shape == (3, case["B"])
