"""Float64 numpy restatement of the draw ``rnampnn_design_tied`` documents (include/rnampnn_hip.h): the yardstick of
tests/test_design_tied_*.py.  The hash, the selection rule and the compatibility sets are those of tests/_design_ref.py; new are the group
quantities (weighted sum of the states' logits, AND of their masks, common length), the union graph with its keep-two rule, and the exact
draw over a path or a cycle (``prepare_chain`` / ``sample_chain``; the forward weights are kept as logarithms, so a chain stays feasible
at any temperature).  ``sample_chain`` takes the choice as a callback, so the same code draws
(the callback is the selection rule) and states the probability it assigns to a given assignment (tests/test_design_tied_cpu.py multiplies
the conditionals and compares with brute force).  Per draw the margin is the relative distance of the uniform to the nearest cumulative
boundary; a component carries the minimum over its draws, because one flipped draw legitimately changes the rest of the chain."""
import numpy as np

from _design_ref import COMPAT, _select, mix64, u24  # noqa: F401

NEG = -np.inf


def _fmax(a):
    """The largest component, ignoring NaN (C's fmax); -inf when there is none."""
    return float(np.fmax.reduce(np.asarray(a, dtype=np.float64), initial=NEG))


def _cells(mask):
    return [c for c in range(4) if (mask >> c) & 1]


def omega(z, mask):
    with np.errstate(invalid="ignore", over="ignore"):
        mx = _fmax([z[c] for c in _cells(mask)])
        return np.array([np.exp(z[c] - mx) if (mask >> c) & 1 else 0.0 for c in range(4)])


def _lse(vals):
    """log sum exp; -inf when no term is above -inf (NaN included)."""
    m = _fmax(vals)
    if not m > NEG:
        return NEG
    with np.errstate(invalid="ignore", over="ignore"):
        return m + float(np.log(sum(np.exp(float(v) - m) for v in vals)))


def _through(la, wob):
    """log sum_a exp(lambda(a)) C(a, c) for every c, over exactly the classes that pair with c."""
    return np.array([_lse([la[a] for a in range(4) if (COMPAT[wob][c] >> a) & 1]) for c in range(4)])


def _forward(zs, masks, wob, head):
    """The forward pass in the log domain (lambda_k = log alpha_k), each lambda_k minus its largest component.
    -> (lambdas of v_0 .. v_{L-1}, the sum of those components), or None when one of them is not above -inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        mx0 = _fmax([zs[0][c] for c in _cells(masks[0])])
        la = np.array([zs[0][c] - mx0 if (masks[0] >> c) & 1 and (head is None or c == head) else NEG for c in range(4)])
        if not _fmax(la) > NEG:
            return None
        las, logn = [la], 0.0
        for k in range(1, len(masks)):
            t = _through(la, wob)
            nx = np.array([zs[k][c] + t[c] if (masks[k] >> c) & 1 else NEG for c in range(4)])
            mx = _fmax(nx)
            if not mx > NEG:
                return None
            la = nx - mx
            logn += mx
            las.append(la)
    return las, logn


def _weights(la, eligible):
    """exp(lambda(c) - max over the eligible classes) for the classes in ``eligible``, 0 for the others."""
    with np.errstate(invalid="ignore", over="ignore"):
        mx = _fmax([la[c] for c in range(4) if (eligible >> c) & 1])
        return np.array([np.exp(la[c] - mx) if (eligible >> c) & 1 else 0.0 for c in range(4)])


def prepare_chain(z, masks, cyc, wob):
    """z: (L,4) of v_0 .. v_{L-1} (L >= 3), masks: their admitted sets (never empty).  -> the sample-independent state, or None when the
    component is infeasible."""
    st = dict(z=np.asarray(z, dtype=np.float64), masks=list(masks), cyc=cyc, wob=wob)
    if not cyc:
        st["fw"] = _forward(st["z"], masks, wob, None)
        return st if st["fw"] is not None else None
    lz = []
    for h in range(4):
        fw = _forward(st["z"], masks, wob, h)
        lz.append(_lse([fw[0][-1][c] for c in range(4) if (COMPAT[wob][h] >> c) & 1]) + fw[1] if fw is not None else NEG)
    mx = _fmax(lz)
    if not mx > NEG:
        return None
    with np.errstate(invalid="ignore"):
        st["head_w"] = np.exp(np.array(lz) - mx)
    return st


def sample_chain(st, choose):
    """choose(k, cells, weights) -> the class of v_k.  -> the classes of v_0 .. v_{L-1}."""
    masks, wob, L = st["masks"], st["wob"], len(st["masks"])
    out = [None] * L
    if st["cyc"]:
        cells = _cells(masks[0])
        head = out[0] = choose(0, cells, st["head_w"][cells])
        las = _forward(st["z"], masks, wob, head)[0]
        eligible = COMPAT[wob][head]
    else:
        las, eligible = st["fw"][0], 15
    for k in range(L - 1, 0 if st["cyc"] else -1, -1):
        cells = _cells(masks[k])
        out[k] = choose(k, cells, _weights(las[k], eligible)[cells])
        eligible = COMPAT[wob][out[k]]
    return out


class TiedPlan:
    """Everything about one batch that does not depend on the sample index."""

    def __init__(self, logits, lengths, group_cu, temperature, weight=None, allowed=None, partner=None, wobble=True, bias=None):
        logits = np.asarray(logits)
        self.B, self.T = logits.shape[0], logits.shape[1]
        temp = float(np.float32(temperature))
        wob = bool(wobble)
        self.infeasible = np.zeros(self.B, dtype=np.int32)
        self.groups = []
        cu = [min(max(int(v), 0), self.B) for v in group_cu]
        for gi in range(len(cu) - 1):
            b0, M = cu[gi], cu[gi + 1] - cu[gi]
            if M <= 0:
                continue
            n = min(int(lengths[b]) for b in range(b0, b0 + M))
            z = np.zeros((n, 4))
            mask = np.full(n, 15, dtype=np.int64)
            with np.errstate(invalid="ignore", over="ignore"):
                for b in range(b0, b0 + M):
                    w = 1.0 if weight is None else float(np.float32(weight[b]))
                    z = z + w * logits[b, :n].astype(np.float64)
                    if allowed is not None:
                        mask &= np.asarray(allowed)[b, :n].astype(np.int64)
                if bias is not None:
                    bi = np.asarray(bias).astype(np.float64)
                    z = z + (bi if bi.ndim == 1 else bi[b0, :n])
                z = z / temp
            mask &= 15
            bad = int((mask == 0).sum())
            mask = np.where(mask == 0, 15, mask)
            keep = [[] for _ in range(n)]
            if partner is not None:
                for t in range(n):
                    for b in range(b0, b0 + M):
                        j = int(partner[b][t])
                        if 0 <= j < n and j != t and int(partner[b][j]) == t and j not in keep[t]:
                            if len(keep[t]) < 2:
                                keep[t].append(j)
                            elif len(keep[t]) == 2:
                                keep[t].append(-1)                 # marks "more than two": counted once
                bad += sum(1 for k in keep if len(k) > 2)
                keep = [k[:2] for k in keep]
            live = [[j for j in keep[t] if t in keep[j]] for t in range(n)]
            g = dict(b0=b0, M=M, n=n, z=z, mask=mask, live=live, single=[], pair=[], chain=[], wob=wob)
            seen = np.zeros(n, dtype=bool)
            for t in range(n):
                if seen[t]:
                    continue
                nodes, cyc = self._component(live, t)
                seen[nodes] = True
                if len(nodes) == 1:
                    g["single"].append(t)
                    continue
                feasible = False
                if len(nodes) == 2:
                    i, j = nodes
                    cells = [(a, c) for a in range(4) for c in range(4) if (mask[i] >> a) & 1 and (mask[j] >> c) & 1 and (COMPAT[wob][a] >> c) & 1]
                    if cells:
                        lz = np.array([z[i, a] + z[j, c] for a, c in cells])
                        with np.errstate(invalid="ignore"):
                            g["pair"].append((i, j, cells, np.exp(lz - np.max(lz))))
                        feasible = True
                else:
                    st = prepare_chain(z[nodes], [int(mask[v]) for v in nodes], cyc, wob)
                    if st is not None:
                        g["chain"].append((nodes, st))
                        feasible = True
                if not feasible:
                    bad += len(nodes)
                    g["single"] += nodes
            g["omega"] = {t: omega(z[t], int(mask[t])) for t in g["single"]}
            self.infeasible[b0:b0 + M] = bad
            self.groups.append(g)

    @staticmethod
    def _component(live, t):
        """t is the smallest index of its component (the scan is ascending).  -> (v_0, v_1, ... in the order of the contract, is a cycle)."""
        if not live[t]:
            return [t], False
        nodes, stack = {t}, [t]
        while stack:
            for j in live[stack.pop()]:
                if j not in nodes:
                    nodes.add(j); stack.append(j)
        ends = sorted(v for v in nodes if len(live[v]) == 1)
        cyc = not ends
        v0 = t if cyc else ends[0]
        order, prev, cur = [v0], v0, min(live[v0])
        while cur != v0:
            order.append(cur)
            nxt = [j for j in live[cur] if j != prev]
            if not nxt:
                break
            prev, cur = cur, nxt[0]
        assert len(order) == len(nodes)
        return order, cyc

    def components(self):
        """[(b0, nodes, 'single' | 'pair' | 'path' | 'cycle')] of the feasible components, for tests that look at the structure."""
        out = []
        for g in self.groups:
            out += [(g["b0"], [t], "single") for t in g["single"]] + [(g["b0"], [i, j], "pair") for i, j, _, _ in g["pair"]]
            out += [(g["b0"], nodes, "cycle" if st["cyc"] else "path") for nodes, st in g["chain"]]
        return out

    def draw(self, seed, s):
        """Sample s -> (seqs (B,T) int8 with -1 where nothing is written, margin (B,T) f64 with inf there)."""
        seqs = np.full((self.B, self.T), -1, dtype=np.int8)
        margin = np.full((self.B, self.T), np.inf)
        for g in self.groups:
            b0, n = g["b0"], g["n"]
            q, mg = np.full(n, -1, dtype=np.int8), np.full(n, np.inf)
            for t in g["single"]:
                q[t], mg[t] = _select(_cells(int(g["mask"][t])), g["omega"][t][_cells(int(g["mask"][t]))], u24(seed, s, b0, t))
            for i, j, cells, w in g["pair"]:
                (a, c), m = _select(cells, w, u24(seed, s, b0, i))
                q[i], q[j], mg[i], mg[j] = a, c, m, m
            for nodes, st in g["chain"]:
                worst = [np.inf]

                def choose(k, cells, w):
                    c, m = _select(cells, w, u24(seed, s, b0, nodes[k]))
                    worst[0] = min(worst[0], m) if m == m else np.nan
                    return c
                q[nodes] = sample_chain(st, choose)
                mg[nodes] = worst[0]
            seqs[b0:b0 + g["M"], :n] = q
            margin[b0:b0 + g["M"], :n] = mg
        return seqs, margin


def design_tied_ref(logits, lengths, group_cu, temperature, S, seed, weight=None, allowed=None, partner=None, wobble=True, bias=None):
    """-> (seqs (S,B,T) int8, margin (S,B,T) f64, infeasible (B,) int32, plan)."""
    plan = TiedPlan(logits, lengths, group_cu, temperature, weight, allowed, partner, wobble, bias)
    out = [plan.draw(int(seed), s) for s in range(S)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), plan.infeasible, plan
