"""Float64 numpy restatement of the draw ``rnampnn_design`` documents (include/rnampnn_hip.h): the yardstick of tests/test_design_*.py.
The reference project has no sampler, so the contract itself is restated: Python-int ``mix64``, f64 weights, the same cell order, the same
selection rule and the same fallbacks.  Besides the chosen ids it returns, per draw, how far the uniform lies from the nearest cumulative
boundary relative to the total - an f32 kernel may legitimately land on the other side of a boundary closer than its rounding."""
import numpy as np

M64 = (1 << 64) - 1
# AUCG = 0..3: the classes that pair with class a
COMPAT = {True: (0b0010, 0b1001, 0b1000, 0b0110), False: (0b0010, 0b0001, 0b1000, 0b0100)}
PAIRS = {w: {(a, b) for a in range(4) for b in range(4) if (COMPAT[w][a] >> b) & 1} for w in (True, False)}


def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def u24(seed, s, b, t):
    h = mix64((seed + 0x9E3779B97F4A7C15 * (s + 1)) & M64)
    h = mix64(h ^ ((0xD6E8FEB86659FD93 * (b + 1)) & M64))
    h = mix64(h ^ ((0xBF58476D1CE4E5B9 * (t + 1)) & M64))
    return h >> 40


def _select(cells, w, u_bits):
    """cells: ids in order; w: their f64 weights -> (chosen id, relative distance of u to the nearest cumulative boundary)."""
    cum = np.cumsum(w)
    tot = cum[-1]
    u = u_bits * 2.0 ** -24 * tot
    hit = np.nonzero(cum > u)[0]
    k = int(hit[0]) if hit.size else len(cells) - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = float(np.min(np.abs(cum - u)) / tot)
    return cells[k], margin


class Plan:
    """Everything about one batch that does not depend on the sample index: per valid position its kind and its cumulative weights."""

    def __init__(self, logits, lengths, temperature, allowed=None, partner=None, wobble=True, bias=None):
        logits = np.asarray(logits)
        self.B, self.T = logits.shape[0], logits.shape[1]
        self.lengths = [int(n) for n in lengths]
        temp = float(np.float32(temperature))
        z = logits.astype(np.float64)
        if bias is not None:
            z = z + np.asarray(bias).astype(np.float64)            # (4,) or (B,T,4)
        z = z / temp
        wob = bool(wobble)
        self.infeasible = np.zeros(self.B, dtype=np.int32)
        self.mate = np.full((self.B, self.T), -1, dtype=np.int64)  # the partner of a well-formed pair, feasible or not
        self.feasible = np.zeros((self.B, self.T), dtype=bool)     # ... and whether the pair has a cell
        self.single, self.pair = {}, {}
        for b, n in enumerate(self.lengths):
            mask = np.full(n, 15, dtype=np.int64) if allowed is None else (np.asarray(allowed)[b, :n].astype(np.int64) & 15)
            self.infeasible[b] += int((mask == 0).sum())
            mask = np.where(mask == 0, 15, mask)
            for t in range(n):
                j = -1 if partner is None else int(partner[b][t])
                if 0 <= j < n and j != t and int(partner[b][j]) == t:
                    self.mate[b, t] = j
            for t in range(n):
                j = int(self.mate[b, t])
                if j > t:
                    cells = [(a, c) for a in range(4) for c in range(4)
                             if (mask[t] >> a) & 1 and (mask[j] >> c) & 1 and (COMPAT[wob][a] >> c) & 1]
                    if cells:
                        lz = np.array([z[b, t, a] + z[b, j, c] for a, c in cells])
                        with np.errstate(invalid="ignore"):
                            self.pair[(b, t)] = (cells, np.exp(lz - np.max(lz)), j)
                        self.feasible[b, t] = self.feasible[b, j] = True
                    else:
                        self.infeasible[b] += 2
            for t in range(n):
                if not self.feasible[b, t]:
                    cls = [c for c in range(4) if (mask[t] >> c) & 1]
                    zz = z[b, t, cls]
                    with np.errstate(invalid="ignore"):
                        self.single[(b, t)] = (cls, np.exp(zz - np.max(zz)))

    def draw(self, seed, s, seqs=None, margin=None):
        """Sample s -> (seqs (B,T) int8 with -1 on padding, margin (B,T) f64 with inf on padding)."""
        seqs = np.full((self.B, self.T), -1, dtype=np.int8) if seqs is None else seqs
        margin = np.full((self.B, self.T), np.inf) if margin is None else margin
        for (b, t), (cls, w) in self.single.items():
            seqs[b, t], margin[b, t] = _select(cls, w, u24(seed, s, b, t))
        for (b, t), (cells, w, j) in self.pair.items():
            (a, c), m = _select(cells, w, u24(seed, s, b, t))
            seqs[b, t], seqs[b, j] = a, c
            margin[b, t] = margin[b, j] = m
        return seqs, margin


def design_ref(logits, lengths, temperature, S, seed, allowed=None, partner=None, wobble=True, bias=None):
    """-> (seqs (S,B,T) int8, margin (S,B,T) f64, infeasible (B,) int32, plan)."""
    plan = Plan(logits, lengths, temperature, allowed, partner, wobble, bias)
    out = [plan.draw(int(seed), s) for s in range(S)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), plan.infeasible, plan
