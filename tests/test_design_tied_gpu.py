"""``rnampnn_design_tied`` (csrc/design_tied.hip) on the device, against the float64 restatement of its contract in tests/_design_tied_ref.py.

One padded batch of 18 rows in 10 groups (T = 300, S = 4, logits 3 * randn); ``STATES`` rows per group, row b has ``LENGTHS[b]`` nucleotides:

  group 0  row 0        M = 1, 300 nt   pairs (3,259) (62,64) (10,40), 10 fixed to G, 62 = R, 150 has allowed = 0 (counts 1)
  group 1  rows 1-2     M = 2, 300 nt   a switch: a 3-node path 10 - 270 - 140 over both 256-strides; the 4-cycle 20-30-40-50 with 30 fixed to
                                        G; the 6-cycle 60-70-80-90-100-110; the 5-path 120-125-130-135-138 with 130 = R in one state; the
                                        40-node zigzag path 150, 299, 151, 298, ... whose edges alternate between the states
  group 2  rows 3-5     M = 3, 257 nt   5 pairs with 256, 100 and 200 in the three states: a degree-3 node (keeps 256 and 100, counts 1; 200
                                        is dropped and draws alone); A(fixed) 30 - 40 - 50 C(fixed): an infeasible path, counts 3;
                                        weights 1, -0.5, 0
  group 3  rows 6-9     M = 4, 65 nt    four conformers with one hairpin (k, 64 - k), k < 10; 20 = R and M in two states (AND = A);
                                        40 = A and U in two states (empty AND: drawn as free, counts 1)
  group 4  rows 10-11   M = 2, 63 / 65 nt   mismatched lengths: the common prefix of 63; (10,64) of the longer state is out of it
  group 5  -            M = 0           an empty group
  group 6  row 12       M = 1, 0 nt
  group 7  row 13       M = 1, 1 nt
  group 8  rows 14-15   M = 2, 2 nt     the whole RNA is one pair in one state
  group 9  rows 16-17   M = 2, 63 nt    NaN logits in the second state (a whole row, and single classes, one of them on the pair (3,40))

``infeasible`` is ``INFEASIBLE`` in every variant.

Permuting the groups: a draw is a function of (seed, s, b0, t) with b0 the group's first row, and groups are consecutive rows, so a group
that moves draws from other uniforms.  The permuted batch is therefore compared with the restatement of the permuted batch and its
``infeasible`` with the permuted counts; "the same bytes per group" is asserted for everything that keeps b0 (layouts, a larger T, a
sub-batch of leading groups, other group tables over the same rows)."""
import csv
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

import _design_ref as R  # noqa: E402
import _design_tied_ref as TR  # noqa: E402
from _design_case import SMALL, _bytes, _write_data  # noqa: E402

T = 300
S = 4
SEED = 0x1234_5678_9ABC_DEF1
GEN_SEED = 41
STATES = [1, 2, 3, 4, 2, 0, 1, 1, 2, 2]
LENGTHS = [300, 300, 300, 257, 257, 257, 65, 65, 65, 65, 63, 65, 0, 1, 2, 2, 63, 63]
WEIGHTS = [1.0, 1.0, 0.5, 1.0, -0.5, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0]
INFEASIBLE = [1, 0, 0, 4, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
GROUP_CU = np.concatenate([[0], np.cumsum(STATES)]).astype(np.int32)
ZIGZAG = [150 + k // 2 if k % 2 == 0 else 299 - k // 2 for k in range(40)]
VARIANTS = {"plain": dict(bias=None, wobble=True), "global": dict(bias="global", wobble=True), "perpos": dict(bias="perpos", wobble=False)}
NEAR = 1e-5                                                        # draws this close to a cumulative boundary (relative) are not compared
NAN_ROWS = (16, 17)
# (first row of the group, nodes in the order of the contract, kind): every component of more than one node
COMPONENTS = [(0, [3, 259], "pair"), (0, [10, 40], "pair"), (0, [62, 64], "pair"),
              (1, [10, 270, 140], "path"), (1, [20, 30, 40, 50], "cycle"), (1, [60, 70, 80, 90, 100, 110], "cycle"),
              (1, [120, 125, 130, 135, 138], "path"), (1, ZIGZAG, "path"), (3, [100, 5, 256], "path")] + \
             [(6, [k, 64 - k], "pair") for k in range(10)] + [(10, [0, 62], "pair"), (14, [0, 1], "pair"), (16, [3, 40], "pair")]


def host_case(gen_seed=GEN_SEED):
    """The batch on the host (numpy): logits, mask, allowed, partner, the two biases, the packed layout."""
    B = len(LENGTHS)
    gen = torch.Generator().manual_seed(gen_seed)
    logits = 3.0 * torch.randn(B, T, 4, generator=gen)
    mask = torch.zeros(B, T)
    for b, n in enumerate(LENGTHS):
        mask[b, :n] = 1
    logits = logits * mask[..., None]
    logits[17, 5] = float("nan"); logits[17, 3, 1] = float("nan"); logits[17, 20, 2] = float("nan")
    allowed = np.full((B, T), 15, dtype=np.uint8)
    partner = np.full((B, T), -1, dtype=np.int32)

    def pair(row, i, j):
        partner[row, i], partner[row, j] = j, i
    pair(0, 3, 259); pair(0, 62, 64); pair(0, 10, 40)
    allowed[0, 10] = 8; allowed[0, 62] = 9; allowed[0, 150] = 0
    pair(1, 10, 270); pair(2, 270, 140)
    pair(1, 20, 30); pair(1, 40, 50); pair(2, 30, 40); pair(2, 50, 20)
    allowed[1, 30] = 8
    pair(1, 60, 70); pair(1, 80, 90); pair(1, 100, 110); pair(2, 70, 80); pair(2, 90, 100); pair(2, 110, 60)
    pair(1, 120, 125); pair(1, 130, 135); pair(2, 125, 130); pair(2, 135, 138)
    allowed[2, 130] = 9
    for k in range(39):
        pair(1 + k % 2, ZIGZAG[k], ZIGZAG[k + 1])
    pair(3, 5, 256); pair(4, 5, 100); pair(5, 5, 200)
    pair(3, 30, 40); pair(4, 40, 50)
    allowed[3, 30] = 1; allowed[3, 50] = 4
    for r in range(6, 10):
        for k in range(10):
            pair(r, k, 64 - k)
    allowed[6, 20] = 9; allowed[8, 20] = 5; allowed[6, 40] = 1; allowed[7, 40] = 2
    pair(10, 0, 62); pair(11, 0, 62); pair(11, 10, 64)
    pair(14, 0, 1)
    pair(16, 3, 40)
    d = dict(B=B, logits=logits.numpy(), mask=mask.numpy(), allowed=allowed, partner=partner, weight=np.array(WEIGHTS, dtype=np.float32))
    d["global"] = np.array([0.5, -1.0, 0.25, -0.5], dtype=np.float32)
    d["perpos"] = (0.5 * torch.randn(B, T, 4, generator=gen)).numpy()
    d["packed"] = np.ascontiguousarray(d["logits"][d["mask"] != 0])
    d["cu"] = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    return d


def host_ref(h, variant, temperature, n=S, seed=SEED, group_cu=GROUP_CU, weight="case"):
    v = VARIANTS[variant]
    return TR.design_tied_ref(h["logits"], LENGTHS, group_cu, temperature, n, seed, h["weight"] if isinstance(weight, str) else weight,
                              h["allowed"], h["partner"], v["wobble"], None if v["bias"] is None else h[v["bias"]])


def valid_mask(group_cu=GROUP_CU, lengths=LENGTHS):
    """(B,T) bool: the positions a group writes an id to (t < n_g)."""
    out = np.zeros((len(lengths), T), dtype=bool)
    for g in range(len(group_cu) - 1):
        rows = range(int(group_cu[g]), int(group_cu[g + 1]))
        if len(rows):
            out[list(rows), :min(lengths[b] for b in rows)] = True
    return out


def group_score(h, b0, M, wob=True, bias=None):
    """(n_g,4) f64: sum_m weight_m logit_m (+ bias of the first row) of the group starting at row b0, untempered."""
    n = min(LENGTHS[b0:b0 + M])
    z = sum(float(h["weight"][b]) * h["logits"][b, :n].astype(np.float64) for b in range(b0, b0 + M))
    return z if bias is None else z + (bias if bias.ndim == 1 else bias[b0, :n]).astype(np.float64)


def best_assignment(z, masks, cyc, wob, clamp=None):
    """Max-product over a path or a cycle v_0 .. v_{L-1} in float64: -> (best total of z_k(c_k), the assignment), (-inf, None) when no
    compatible assignment exists.  ``clamp`` = (k, c) fixes one node."""
    L = len(masks)
    ok = lambda k, c: (masks[k] >> c) & 1 and (clamp is None or clamp[0] != k or clamp[1] == c)
    best = (-np.inf, None)
    for head in range(4) if cyc else [None]:
        if cyc and not ok(0, head):
            continue
        score = {c: (z[0][c], [c]) for c in range(4) if ok(0, c) and (head is None or c == head)}
        for k in range(1, L):
            nxt = {}
            for c in range(4):
                if not ok(k, c):
                    continue
                cands = [(sc + z[k][c], path + [c]) for a, (sc, path) in score.items() if (R.COMPAT[wob][a] >> c) & 1]
                if cands:
                    nxt[c] = max(cands, key=lambda x: x[0])
            score = nxt
        for c, (sc, path) in score.items():
            if (not cyc or (R.COMPAT[wob][c] >> head) & 1) and sc > best[0]:
                best = (sc, path)
    return best


def cold_argmax(h):
    """Per component of more than one node outside the NaN group: (its float64 argmax, the lead over the best assignment that differs in at
    least one node), with wobble and no bias."""
    starts = {int(GROUP_CU[g]): STATES[g] for g in range(len(STATES)) if STATES[g]}
    out = {}
    for b0, nodes, kind in COMPONENTS:
        if b0 in NAN_ROWS:
            continue
        z = group_score(h, b0, starts[b0])[nodes]
        masks = [int(np.bitwise_and.reduce(h["allowed"][b0:b0 + starts[b0], t]) & 15) or 15 for t in nodes]
        top, asg = best_assignment(z, masks, kind == "cycle", True)
        other = max(best_assignment(z, masks, kind == "cycle", True, clamp=(k, c))[0] for k in range(len(nodes)) for c in range(4) if c != asg[k])
        out[(b0, tuple(nodes))] = (asg, top - other)
    return out


@pytest.fixture(scope="module")
def case():
    """Inputs on the device + the float64 references, computed once and never written to."""
    import __graft_entry__ as g
    g.build()
    from rnampnn.utils.constraints import DesignConstraints
    h = host_case()
    d = dict(h=h, B=h["B"])
    for k in ("logits", "mask", "packed", "cu", "weight"):
        d[k] = torch.from_numpy(h[k]).cuda()
    d["cons"] = {}
    for name, v in VARIANTS.items():
        bias = None if v["bias"] is None else torch.from_numpy(h[v["bias"]])
        d["cons"][name] = DesignConstraints(torch.from_numpy(h["allowed"]), torch.from_numpy(h["partner"]), bias, v["wobble"]).to_device("cuda")
    d["ref"] = {}
    return d


def _ref(case, variant, temperature, n=S, seed=SEED):
    key = (variant, temperature, n, seed)
    if key not in case["ref"]:
        case["ref"][key] = host_ref(case["h"], variant, temperature, n, seed)
    return case["ref"][key]


def _design(case, variant="global", temperature=1.0, n=S, seed=SEED, layout="padded", states=STATES):
    from rnampnn.model.rnampnn import design_from_logits
    kw = dict(n_samples=n, temperature=temperature, seed=seed, constraints=case["cons"][variant], states=states, state_weights=case["weight"])
    if layout == "padded":
        return design_from_logits(case["logits"], mask=case["mask"], **kw)
    return design_from_logits(case["packed"], cu_seqlens=case["cu"], max_len=T, **kw)


def _compare(got, want, margin, valid, label):
    """Draws equal the restatement wherever the component's margin exceeds NEAR; prints the left-out share."""
    valid = np.broadcast_to(valid, got.shape)
    near = valid & ~(margin > NEAR)
    print(f"{label}: {int(near.sum())} of {int(valid.sum())} draws left out (margin <= {NEAR} or NaN: {near.sum() / max(valid.sum(), 1):.4%}); "
          f"{int(((got != want) & near).sum())} of them differ")
    differ = (got != want) & valid & ~near
    assert not differ.any(), np.argwhere(differ)[:10].tolist()
    assert (got[~valid] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("variant", ["global", "perpos"])
@pytest.mark.parametrize("temperature", [1.0, 0.3])
def test_draws_equal_the_float64_reference(case, variant, temperature):
    want, margin, bad, plan = _ref(case, variant, temperature)
    seqs, _, infeasible = _design(case, variant, temperature)
    got = seqs.cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (S, case["B"], T)
    _compare(got, want, margin, valid_mask(), f"{variant} temperature {temperature}")
    assert infeasible.dtype == torch.int32 and infeasible.tolist() == bad.tolist() == INFEASIBLE
    # the components are the listed ones: the malformed entries, the dropped edge and the out-of-prefix pair link nothing
    assert sorted((b0, nodes) for b0, nodes, kind in plan.components() if kind != "single") == \
        sorted((b0, nodes) for b0, nodes, _ in COMPONENTS if not (b0 == 3 and nodes[0] == 30))


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("variant", ["global", "perpos"])
def test_invariants_hold_in_every_draw(case, variant):
    seqs, _, infeasible = _design(case, variant, 1.0)
    got = seqs.cpu().numpy()
    wobble = VARIANTS[variant]["wobble"]
    valid = valid_mask()
    assert infeasible.tolist() == INFEASIBLE
    assert (got[:, ~valid] == -1).all() and ((got[:, valid] >= 0) & (got[:, valid] <= 3)).all()     # a NaN state still gives ids
    for g in range(len(STATES)):                                    # all rows of a group hold identical bytes
        for b in range(int(GROUP_CU[g]) + 1, int(GROUP_CU[g + 1])):
            assert got[:, b].tobytes() == got[:, int(GROUP_CU[g])].tobytes(), b
    for s in range(S):
        for b0, nodes, kind in COMPONENTS:
            if b0 in NAN_ROWS:
                continue
            edges = list(zip(nodes[:-1], nodes[1:])) + ([(nodes[-1], nodes[0])] if kind == "cycle" else [])
            for i, j in edges:                                      # every live edge holds a compatible pair
                assert (int(got[s, b0, i]), int(got[s, b0, j])) in R.PAIRS[wobble], (s, b0, i, j)
        assert got[s, 0, 10] == 3 and got[s, 0, 62] in (0, 3)       # masks: G fixed, R
        assert got[s, 1, 30] == 3 and got[s, 1, 130] in (0, 3)      # G fixed on the 4-cycle, R on the 5-path
        assert got[s, 3, 30] == 0 and got[s, 3, 50] == 2            # the infeasible path keeps both fixed letters
        assert got[s, 6, 20] == 0                                   # R and M = A


# ---------------------------------------------------------------------------------------------------------------- 3
def test_cold_limit_is_the_constrained_argmax(case):
    best = cold_argmax(case["h"])
    lead = min(v[1] for v in best.values())
    print("smallest lead of a component's best assignment over its runner-up:", lead)
    assert lead >= 0.05                                            # 50 temperatures: the runner-up is drawn with probability e^-50
    seqs, _, infeasible = _design(case, "plain", 1e-3)
    got = seqs.cpu().numpy()
    for (b0, nodes), (asg, _) in best.items():
        for s in range(S):
            assert got[s, b0, list(nodes)].tolist() == asg, (s, b0, nodes[:4])
    assert infeasible.tolist() == INFEASIBLE                       # no feasible component underflowed into the infeasible branch
    assert infeasible.tolist() == _ref(case, "plain", 1e-3)[2].tolist()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("variant, temperature", [("global", 1.0), ("perpos", 0.3)])
def test_seq_nll_is_rnampnn_scores_byte_for_byte(case, variant, temperature):
    from rnampnn.model.rnampnn import score_logits
    seqs, nll, _ = _design(case, variant, temperature)
    assert nll.dtype == torch.float32 and nll.shape == (S, case["B"])
    assert _bytes(nll) == _bytes(score_logits(case["logits"], mask=case["mask"], seqs=seqs, want=("seq_nll",))["seq_nll"])
    assert _bytes(nll) == _bytes(score_logits(case["packed"], cu_seqlens=case["cu"], seqs=seqs, want=("seq_nll",))["seq_nll"])
    packed = _design(case, variant, temperature, layout="packed")
    assert _bytes(packed[1]) == _bytes(nll)
    assert float(nll[:, 12].abs().sum()) == 0.0                    # the empty RNA
    assert bool(torch.isfinite(nll[:, :16]).all()) and bool((nll[:, [0, 1, 2, 3, 6, 10, 11]] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("variant", ["global", "perpos"])
def test_layout_padding_and_batch_independence(case, variant):
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    a, b, p = _design(case, variant), _design(case, variant), _design(case, variant, layout="packed")
    for x, y, z in zip(a, b, p):
        assert _bytes(x) == _bytes(y) and _bytes(x) == _bytes(z)
    # T = 320, garbage beyond every length: NaN logits, random allowed / partner / bias entries
    T2, B = 320, case["B"]
    gen = torch.Generator().manual_seed(7)
    c = case["cons"][variant]
    inside = torch.zeros(B, T2, dtype=torch.bool)
    for r, n in enumerate(LENGTHS):
        inside[r, :n] = True
    inside = inside.cuda()

    def grow(t, junk):
        big = junk.to(t.dtype).cuda()
        big[:, :T] = torch.where(inside[:, :T].view(B, T, *([1] * (t.dim() - 2))), t, big[:, :T])
        return big
    logits = grow(case["logits"], torch.full((B, T2, 4), float("nan")))
    allowed = grow(c.allowed, torch.randint(0, 256, (B, T2), generator=gen))
    partner = grow(c.partner, torch.randint(-5, 400, (B, T2), generator=gen))
    bias = c.bias if c.bias.dim() == 1 else grow(c.bias, torch.full((B, T2, 4), float("nan")))
    big = design_from_logits(logits, mask=inside.float(), n_samples=S, temperature=1.0, seed=SEED, states=STATES, state_weights=case["weight"],
                             constraints=DesignConstraints(allowed, partner, bias, c.wobble))
    assert big[0].shape == (S, B, T2) and bool((big[0][:, :, T:] == -1).all())
    assert _bytes(big[0][:, :, :T].contiguous()) == _bytes(a[0]) and _bytes(big[1]) == _bytes(a[1]) and _bytes(big[2]) == _bytes(a[2])
    # another seed, and sample 0 when S goes from 1 to 4
    other = _design(case, variant, seed=SEED + 1)
    assert _bytes(other[0]) != _bytes(a[0]) and _bytes(other[2]) == _bytes(a[2])
    one = _design(case, variant, n=1)
    assert one[0].shape == (1, B, T) and _bytes(one[0][0]) == _bytes(a[0][0]) and _bytes(one[1][0]) == _bytes(a[1][0])
    # a sub-batch of the leading groups (rows 0..9), and the same rows under another table (no empty group): G and the other groups do not matter
    sub = design_from_logits(case["logits"][:10], mask=case["mask"][:10], n_samples=S, temperature=1.0, seed=SEED, states=STATES[:4],
                             state_weights=case["weight"][:10],
                             constraints=DesignConstraints(c.allowed[:10], c.partner[:10], c.bias if c.bias.dim() == 1 else c.bias[:10], c.wobble))
    for x, y in zip(sub, a):
        assert _bytes(x) == _bytes((y[:, :10] if y.dim() > 1 else y[:10]).contiguous())
    dense = _design(case, variant, states=[k for k in STATES if k])
    for x, y in zip(dense, a):
        assert _bytes(x) == _bytes(y)


def test_a_permuted_group_order_follows_the_restatement(case):
    """Groups are consecutive rows and the uniform is that of the group's first row, so a moved group draws other ids: the permuted batch
    equals the restatement OF THE PERMUTED BATCH, and the counts move with their groups."""
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    h = case["h"]
    order = [9, 3, 5, 1, 0, 8, 2, 7, 4, 6]                            # groups in another order
    rows = [b for g in order for b in range(int(GROUP_CU[g]), int(GROUP_CU[g + 1]))]
    states = [STATES[g] for g in order]
    cu = np.concatenate([[0], np.cumsum(states)]).astype(np.int32)
    lengths = [LENGTHS[b] for b in rows]
    want, margin, bad, _ = TR.design_tied_ref(h["logits"][rows], lengths, cu, 0.3, S, SEED, h["weight"][rows], h["allowed"][rows],
                                              h["partner"][rows], True, h["global"])
    assert bad.tolist() == [INFEASIBLE[b] for b in rows]
    idx = torch.tensor(rows).cuda()
    c = case["cons"]["global"]
    seqs, nll, infeasible = design_from_logits(case["logits"][idx], mask=case["mask"][idx], n_samples=S, temperature=0.3, seed=SEED,
                                               states=states, state_weights=case["weight"][idx],
                                               constraints=DesignConstraints(c.allowed[idx], c.partner[idx], c.bias, True))
    assert infeasible.tolist() == bad.tolist()
    _compare(seqs.cpu().numpy(), want, margin, valid_mask(cu, lengths), "permuted groups, temperature 0.3")


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("variant, temperature", [("global", 1.0), ("perpos", 0.3)])
def test_one_state_per_group_is_rnampnn_design(case, variant, temperature):
    """Every row a group of its own, no weights: the draws of ``rnampnn_design`` (f32) wherever the float64 margin exceeds NEAR."""
    from rnampnn.model.rnampnn import design_from_logits
    B = case["B"]
    kw = dict(mask=case["mask"], n_samples=S, temperature=temperature, seed=SEED, constraints=case["cons"][variant])
    tied = design_from_logits(case["logits"], states=[1] * B, **kw)
    plain = design_from_logits(case["logits"], **kw)
    want, margin, bad, _ = host_ref(case["h"], variant, temperature, group_cu=np.arange(B + 1), weight=None)
    valid = case["h"]["mask"] != 0
    _compare(tied[0].cpu().numpy(), want, margin, valid, f"one state per group, {variant}, tied kernel")
    _compare(plain[0].cpu().numpy(), want, margin, valid, f"one state per group, {variant}, rnampnn_design")
    assert tied[2].tolist() == plain[2].tolist() == bad.tolist()
    same = (tied[0] == plain[0]).all(dim=2).cpu().numpy()           # where the two kernels drew the same row, the NLL bytes agree too
    same[:, list(NAN_ROWS)] = False
    assert same[:, :16].mean() > 0.9
    assert (tied[1].cpu().numpy().view(np.uint32)[same] == plain[1].cpu().numpy().view(np.uint32)[same]).all()


def test_argument_errors_of_the_python_layer(case):
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    kw = dict(mask=case["mask"], n_samples=1, temperature=1.0, seed=0)
    with pytest.raises(ValueError, match="sum to B"):
        design_from_logits(case["logits"], states=[1, 2], **kw)
    with pytest.raises(ValueError, match="state_weights"):
        design_from_logits(case["logits"], states=STATES, state_weights=torch.ones(3), **kw)
    with pytest.raises(ValueError, match="states"):
        design_from_logits(case["logits"], state_weights=case["weight"], **kw)
    with pytest.raises(NotImplementedError, match="LDS"):           # the extent that does not fit names the limit
        design_from_logits(torch.zeros(1, 6000, 4, device="cuda"), mask=torch.ones(1, 6000, device="cuda"), n_samples=1, temperature=1.0,
                           seed=0, states=[1],
                           constraints=DesignConstraints(None, torch.full((1, 6000), -1, dtype=torch.int32, device="cuda"), None, True))


def test_the_reference_padding_length_fits(case):
    """T = 4500 (the reference's padding_len) with a partner table: 148.6 KB of dynamic LDS; one 3-node chain at the far end."""
    from rnampnn.model.rnampnn import design_from_logits
    from rnampnn.utils.constraints import DesignConstraints
    Tl = 4500
    gen = torch.Generator().manual_seed(3)
    logits = 3.0 * torch.randn(2, Tl, 4, generator=gen)
    partner = np.full((2, Tl), -1, dtype=np.int32)
    partner[0, 7], partner[0, 4499] = 4499, 7
    partner[1, 4499], partner[1, 2300] = 2300, 4499
    want, margin, bad, plan = TR.design_tied_ref(logits.numpy(), [Tl, Tl], [0, 2], 1.0, 2, SEED, None, None, partner, True, None)
    assert [(n, k) for _, n, k in plan.components() if k != "single"] == [([7, 4499, 2300], "path")]
    seqs, nll, infeasible = design_from_logits(logits.cuda(), mask=torch.ones(2, Tl).cuda(), n_samples=2, temperature=1.0, seed=SEED, states=[2],
                                               constraints=DesignConstraints(None, torch.from_numpy(partner), None, True).to_device("cuda"))
    assert infeasible.tolist() == bad.tolist() == [0, 0]
    _compare(seqs.cpu().numpy(), want, margin, np.ones((2, Tl), dtype=bool), "T = 4500")


# ---------------------------------------------------------------------------------------------------------------- 7
MODEL_LENGTHS = [33, 33, 41]
# the two states of a switch (4..7 pair with 15..12 in one state and with 23..20 in the other: four 3-node chains) + one RNA alone
SPECS = [(None, "....((((....))))" + "." * 17), (None, "....[[[[" + "." * 12 + "]]]]" + "." * 9), ("." * 40 + "U", None)]


def _check_switch(seqs, wobble=True):
    from rnampnn.utils.constraints import parse_dot_bracket
    got = seqs.cpu().numpy()
    assert (got[:, 0] == got[:, 1]).all() and (got[:, :2, 33:] == -1).all() and (got[:, 2, 40] == 1).all()
    for _, structure in SPECS[:2]:                                  # the one sequence is pair-compatible in both states
        p = parse_dot_bracket(structure)
        for t in np.nonzero(p > np.arange(33))[0]:
            for s in range(got.shape[0]):
                assert (int(got[s, 0, t]), int(got[s, 0, p[t]])) in R.PAIRS[wobble], (s, t)


def test_rnampnn_design_with_states():
    import __graft_entry__ as g
    g.build()
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    from rnampnn.utils.data import pad_batch
    torch.manual_seed(0)
    m = RNAMPNN(precision="f32", **SMALL).cuda().eval()
    items = [(synth.synth_rna(n, i, seed=1), synth.synth_labels(n, i, seed=1)) for i, n in enumerate(MODEL_LENGTHS)]
    _, c, mask, lens = pad_batch(items, pin=False)
    c, mask = c.cuda(), mask.cuda()
    cons = DesignConstraints.from_specs(SPECS, lens, int(mask.shape[1]))
    seqs, nll, bad = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, constraints=cons, states=[2, 1], state_weights=[1.0, 0.5, 1.0],
                              lengths=lens)
    assert seqs.shape == (3, 3, max(lens)) and seqs.dtype == torch.int8 and bad.tolist() == [0, 0, 0]
    _check_switch(seqs)
    assert _bytes(nll) == _bytes(m.score_sequences(c, mask, seqs)[0])
    free = m.design(c, mask, n_samples=3, temperature=1.0, seed=3, states=[2, 1])
    assert len(free) == 3 and bool((free[0][:, 0] == free[0][:, 1]).all())
    with pytest.raises(ValueError, match="group 1"):
        m.design(c, mask, n_samples=1, states=[1, 2], lengths=lens)


def test_rdesign_model_designs_with_states():
    import __graft_entry__ as g
    g.build()
    from rdesign.model.rdesign import RNAModel
    from rnampnn.utils import synth
    from rnampnn.utils.constraints import DesignConstraints
    torch.manual_seed(0)
    m = RNAModel(num_mpnn_layers=1).cuda().eval()
    B, Tm = len(MODEL_LENGTHS), max(MODEL_LENGTHS)
    X, mask = torch.zeros(B, Tm, 6, 3), torch.zeros(B, Tm)
    for i, n in enumerate(MODEL_LENGTHS):
        X[i, :n] = torch.from_numpy(synth.synth_rna(n, i, seed=1)[:, :6].astype(np.float32))
        mask[i, :n] = 1
    X, mask = X.cuda(), mask.cuda()
    cons = DesignConstraints.from_specs(SPECS, MODEL_LENGTHS, Tm)
    seqs, nll, bad = m.design(X, mask, n_samples=3, temperature=1.0, seed=5, constraints=cons, lengths=MODEL_LENGTHS, states=[2, 1])
    assert seqs.shape == (3, B, Tm) and nll.shape == (3, B) and bad.tolist() == [0, 0, 0]
    _check_switch(seqs)
    assert _bytes(m.score_sequences(X, mask, seqs, lengths=MODEL_LENGTHS)[0]) == _bytes(nll)
    with pytest.raises(ValueError, match="group 1"):
        m.design(X, mask, n_samples=1, lengths=MODEL_LENGTHS, states=[1, 2])


def test_predict_cli_with_a_states_file(tmp_path):
    import __graft_entry__ as g
    g.build()
    import predict as P
    from rnampnn.model.rnampnn import RNAMPNN
    from rnampnn.utils.train import save_checkpoint
    ids, lens = ["r2", "r0", "r1", "r3"], [33, 33, 41, 27]           # r2 and r0 are the two states of design "sw"; r1 and r3 stand alone
    _write_data(tmp_path / "data", ids, lens)
    (tmp_path / "states.csv").write_text("design_id,pdb_id,weight\nsw,r2,\nsw,r0,0.5\n")
    with open(tmp_path / "cons.csv", "w") as f:
        f.write("pdb_id,fixed,structure\n" + "".join(f"{rid},{SPECS[k][0] or ''},{SPECS[k][1] or ''}\n" for k, rid in enumerate(ids[:3])))
    torch.manual_seed(0)
    ck = str(tmp_path / "model.pt")
    save_checkpoint(ck, RNAMPNN(precision="f32", **SMALL))
    sub, des = str(tmp_path / "submit.csv"), str(tmp_path / "designs.csv")
    common = ["--ckpt", ck, "--data", str(tmp_path / "data"), "--out", sub, "--samples", "3", "--temperature", "1.0", "--designs-out", des,
              "--batch-size", "3"]
    rows = P.run(P.parse(common + ["--states", str(tmp_path / "states.csv"), "--constraints", str(tmp_path / "cons.csv")]), log=lambda *a: None)
    assert [r[0] for r in rows] == sorted(ids)                      # the per-structure file is what it was
    d = list(csv.reader(open(des)))
    assert d[0] == ["design_id", "sample", "seq", "infeasible", "states", "nll_per_nt", "recovery"] and len(d) == 1 + 3 * 3
    assert [(r[0], r[1]) for r in d[1:]] == [(did, str(s)) for did in ["r1", "r3", "sw"] for s in range(3)]
    for r in d[1:]:
        names = r[4].split(";")
        assert names == (["r2", "r0"] if r[0] == "sw" else [r[0]]) and r[3] == "0" and set(r[2]) <= set("AUCG")
        assert len(r[5].split(";")) == len(r[6].split(";")) == len(names) and all(float(v) > 0 for v in r[5].split(";"))
        assert all(0.0 <= float(v) <= 1.0 for v in r[6].split(";")) and len(r[2]) == dict(zip(ids, lens))[names[0]]
        if r[0] == "sw":
            arr = torch.full((1, 3, 41), -1, dtype=torch.int8)
            arr[0, 0, :33] = arr[0, 1, :33] = torch.tensor(["AUCG".index(ch) for ch in r[2]], dtype=torch.int8)
            arr[0, 2, 40] = 1
            _check_switch(arr)
    # without the flag: the columns of the per-structure file (its bytes are pinned by tests/test_design_gpu.py)
    P.run(P.parse(common + ["--constraints", str(tmp_path / "cons.csv")]), log=lambda *a: None)
    d2 = list(csv.reader(open(des)))
    assert d2[0] == ["pdb_id", "sample", "seq", "nll_per_nt", "recovery", "infeasible"] and len(d2) == 1 + 3 * 4
    # states of different lengths, and a listed structure that is not there, name the design / the id
    (tmp_path / "bad.csv").write_text("design_id,pdb_id,weight\nmix,r2,\nmix,r1,\n")
    with pytest.raises(ValueError, match="mix"):
        P.run(P.parse(common + ["--states", str(tmp_path / "bad.csv")]), log=lambda *a: None)
    (tmp_path / "bad2.csv").write_text("design_id,pdb_id,weight\nsw,r2,\nsw,zz,\n")
    with pytest.raises(ValueError, match="zz"):
        P.run(P.parse(common + ["--states", str(tmp_path / "bad2.csv")]), log=lambda *a: None)


def test_predict_cli_refuses_states_for_an_rdesign_checkpoint(tmp_path):
    import __graft_entry__ as g
    g.build()
    import predict as P
    from rdesign.model.rdesign import RNAModel
    from rdesign.utils.train import save_checkpoint
    torch.manual_seed(0)
    ck = str(tmp_path / "model.pt")
    save_checkpoint(ck, RNAModel(num_mpnn_layers=1))
    (tmp_path / "states.csv").write_text("design_id,pdb_id,weight\nsw,r2,\n")
    with pytest.raises(ValueError, match="rnampnn checkpoints only"):
        P.run(P.parse(["--ckpt", ck, "--data", str(tmp_path), "--samples", "2", "--states", str(tmp_path / "states.csv")]), log=lambda *a: None)
