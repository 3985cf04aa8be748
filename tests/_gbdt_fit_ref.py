"""Numpy restatement of the device-side gradient-boosted-tree fit.  TEST INFRASTRUCTURE ONLY: the product never
imports this file.  PARITY UNPINNED (no xgboost in the image): it restates XGBoost's published multi:softmax gradient / hessian, split
gain and leaf weight, and this project's own cuts, binning and sampling, exactly as `csrc/gbdt_fit.hip` does them:

* cuts per feature: sorted column v, candidates v[floor(i * N / max_bin)], i = 1 .. max_bin - 1, duplicates and values equal to v[0]
  dropped (a zero cut is stored as +0.0); bin(x) = number of cuts <= x; a split at cut j sends bin <= j left and has
  split_condition = cuts[j];
* u(seed, a, b) = top 24 bits of the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (a * 2^32 + b + 1), as a fraction of 2^24;
  row i takes part in round r iff u(seed, 2r, i) < subsample; tree t keeps the max(1, floor(colsample * F)) features with the smallest
  u(seed, 2t + 1, f), ties to the lower index;
* gradients: fp64 softmax (row maximum subtracted, sum in class order), g = p - [y == c], h = max(2 p (1 - p), 1e-16), rounded to
  nearest onto the grid 2^-20 and held as integers; histograms are integer sums (fp64 `np.bincount` is exact: the sums stay below 2^53);
* gain = 0.5 * (GL^2 / (HL + lambda) + GR^2 / (HR + lambda) - G^2 / (H + lambda)) - gamma in fp64, admissible iff both children have
  H >= min_child_weight and gain > 1e-6, best = largest gain, then lowest feature, then lowest cut; leaf = f32(lr * -G / (H + lambda));
* nodes are numbered breadth-first; every row (sampled or not) adds its leaf to margin[:, c] in f32.
"""
import numpy as np

SCALE = 1048576.0
INV_SCALE = 1.0 / 1048576.0
MIN_GAIN = 1e-6
NCUT = 255

DEFAULTS = dict(num_class=4, n_estimators=150, max_depth=8, learning_rate=0.1, subsample=0.8, colsample_bytree=0.8, reg_lambda=1.0,
                gamma=0.0, min_child_weight=1.0, max_bin=256, base_score=0.5, seed=0)


def hash_u(seed, a, b):
    """u(seed, a, b) for an array (or scalar) b -> float64 in [0, 1)."""
    with np.errstate(over="ignore"):
        b = np.asarray(b, np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * ((np.uint64(a) << np.uint64(32)) + b + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) * (1.0 / 16777216.0)


def row_mask(seed, rnd, n, subsample):
    if subsample >= 1.0:
        return np.ones(n, bool)
    return hash_u(seed, 2 * rnd, np.arange(n)) < subsample


def feature_mask(seed, tree, F, colsample):
    m = np.ones(F, bool)
    if colsample < 1.0:
        k = max(1, int(np.floor(colsample * F)))
        order = np.argsort(hash_u(seed, 2 * tree + 1, np.arange(F)), kind="stable")
        m[:] = False
        m[order[:k]] = True
    return m


def make_cuts(X, max_bin=256):
    """-> cuts (F, 255) f32 (unused entries 0), n_cuts (F) i32."""
    X = np.asarray(X, np.float32)
    N, F = X.shape
    cuts, n_cuts = np.zeros((F, NCUT), np.float32), np.zeros(F, np.int32)
    idx = (np.arange(1, max_bin, dtype=np.int64) * N) // max_bin
    for f in range(F):
        v = np.sort(X[:, f])
        cand = v[idx] + np.float32(0.0)               # a zero cut is stored as +0.0 whatever the sort put first
        keep = cand != v[0]
        keep[1:] &= cand[1:] != cand[:-1]
        c = cand[keep]
        cuts[f, :len(c)] = c
        n_cuts[f] = len(c)
    return cuts, n_cuts


def bin_matrix(X, cuts, n_cuts):
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape, np.uint8)
    for f in range(X.shape[1]):
        out[:, f] = np.searchsorted(cuts[f, :n_cuts[f]], X[:, f], side="right")
    return out


def gradients(margins, y):
    """(N, C) f32 margins -> integer g, h (C, N) int32 on the grid 2^-20."""
    m = margins.astype(np.float64)
    e = np.exp(m - m.max(axis=1, keepdims=True))
    s = np.zeros(len(m))
    for c in range(m.shape[1]):                  # class order
        s = s + e[:, c]
    p = e / s[:, None]
    onehot = (np.arange(m.shape[1])[None, :] == np.asarray(y)[:, None]).astype(np.float64)
    g = p - onehot
    h = np.maximum(2.0 * p * (1.0 - p), 1e-16)
    return np.rint(g * SCALE).astype(np.int32).T.copy(), np.rint(h * SCALE).astype(np.int32).T.copy()


def leaf_value(G, H, lr, lam):
    return np.float32(lr * (-(np.float64(G) * INV_SCALE) / (np.float64(H) * INV_SCALE + lam)))


def grow_tree(bins, cuts, n_cuts, g, h, rmask, fmask, *, max_depth, learning_rate, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0, trace=None):
    """One tree -> dict(left_children, right_children, split_indices, split_conditions) breadth-first, and the heap leaf of every row
    (its value, for all N rows).  `trace`, if a list, receives (heap node, G, H, best gain, feature, cut) per searched node."""
    N, F = bins.shape
    flist = np.flatnonzero(fmask if fmask is not None else np.ones(F, bool))
    nfs = len(flist)
    heap_n = (1 << (max_depth + 1)) - 1
    state = np.zeros(heap_n, np.int8)            # 0 absent, 1 leaf, 2 split
    feat, cutj = np.zeros(heap_n, np.int64), np.zeros(heap_n, np.int64)
    cond = np.zeros(heap_n, np.float32)
    nodeG, nodeH = np.zeros(heap_n, np.int64), np.zeros(heap_n, np.int64)
    pos = np.zeros(N, np.int64)                  # heap node of every row (all rows walk; only sampled rows are summed)
    sampled = np.ones(N, bool) if rmask is None else np.asarray(rmask, bool)
    gs, hs = g.astype(np.float64), h.astype(np.float64)
    valid_cut = np.arange(256)[None, :] < n_cuts[flist][:, None]          # (nfs, 256)
    for d in range(max_depth):
        base, n_level = (1 << d) - 1, 1 << d
        exists = np.array([n == 0 or state[(n - 1) >> 1] == 2 for n in range(base, base + n_level)])
        rows = np.flatnonzero(sampled & (pos >= base))           # the sampled rows standing on a node of this level
        key = ((pos[rows] - base)[:, None] * nfs + np.arange(nfs)[None, :]) * 256 + bins[rows][:, flist]
        size = n_level * nfs * 256
        hg = np.bincount(key.ravel(), weights=np.repeat(gs[rows], nfs), minlength=size).reshape(n_level, nfs, 256)
        hh = np.bincount(key.ravel(), weights=np.repeat(hs[rows], nfs), minlength=size).reshape(n_level, nfs, 256)
        GL, HL = np.cumsum(hg, axis=2), np.cumsum(hh, axis=2)              # integer-valued fp64, exact
        G, H = GL[:, :1, -1:], HL[:, :1, -1:]                              # node totals (same for every feature)
        gl, hl = GL * INV_SCALE, HL * INV_SCALE
        gr, hr = (G - GL) * INV_SCALE, (H - HL) * INV_SCALE
        gt, ht = G * INV_SCALE, H * INV_SCALE
        with np.errstate(divide="ignore", invalid="ignore"):
            gain = 0.5 * ((gl * gl / (hl + reg_lambda) + gr * gr / (hr + reg_lambda)) - gt * gt / (ht + reg_lambda)) - gamma
        ok = valid_cut[None] & (hl >= min_child_weight) & (hr >= min_child_weight) & (gain > MIN_GAIN)
        gain = np.where(ok, gain, -np.inf).reshape(n_level, -1)
        best = gain.argmax(axis=1)                                         # first maximum = lowest feature, then lowest cut
        for i in range(n_level):
            n = base + i
            if not exists[i]:
                continue
            Gi, Hi = int(G[i, 0, 0]), int(H[i, 0, 0])
            bg = gain[i, best[i]]
            if trace is not None:
                trace.append((n, Gi, Hi, float(bg), int(flist[best[i] // 256]), int(best[i] % 256)))
            if bg > MIN_GAIN:
                fs, j = divmod(int(best[i]), 256)
                state[n], feat[n], cutj[n], cond[n] = 2, flist[fs], j, cuts[flist[fs], j]
                nodeG[2 * n + 1], nodeH[2 * n + 1] = int(GL[i, fs, j]), int(HL[i, fs, j])
                nodeG[2 * n + 2], nodeH[2 * n + 2] = Gi - int(GL[i, fs, j]), Hi - int(HL[i, fs, j])
            else:
                state[n], cond[n] = 1, leaf_value(Gi, Hi, learning_rate, reg_lambda)
        # every row standing on a node that split moves to its child
        here = state[pos] == 2
        idx = np.flatnonzero(here & (pos >= base))
        p = pos[idx]
        pos[idx] = 2 * p + 1 + (bins[idx, feat[p]] > cutj[p])
    base = (1 << max_depth) - 1
    for n in range(base, heap_n):
        if state[(n - 1) >> 1] == 2:
            state[n], cond[n] = 1, leaf_value(nodeG[n], nodeH[n], learning_rate, reg_lambda)
    present = np.flatnonzero(state != 0)
    newid = -np.ones(heap_n, np.int64)
    newid[present] = np.arange(len(present))
    split = state[present] == 2
    left = np.where(split, newid[np.minimum(2 * present + 1, heap_n - 1)], -1).astype(np.int32)
    right = np.where(split, newid[np.minimum(2 * present + 2, heap_n - 1)], -1).astype(np.int32)
    tree = dict(left_children=left, right_children=right, split_indices=np.where(split, feat[present], 0).astype(np.int32),
                split_conditions=cond[present].astype(np.float32))
    return tree, cond[pos]


def assemble(trees, classes, num_class, num_feature, base_score):
    """Per-tree dicts -> the arrays of `parse_xgboost_json`."""
    offs = np.zeros(len(trees) + 1, np.int32)
    offs[1:] = np.cumsum([len(t["left_children"]) for t in trees])
    cat = lambda k, dt: np.concatenate([t[k] for t in trees]).astype(dt)
    return dict(num_class=int(num_class), num_feature=int(num_feature), base_score=float(np.float32(base_score)), tree_offsets=offs,
                tree_class=np.asarray(classes, np.int32), left_children=cat("left_children", np.int32),
                right_children=cat("right_children", np.int32), split_indices=cat("split_indices", np.int32),
                split_conditions=cat("split_conditions", np.float32), default_left=np.zeros(int(offs[-1]), np.uint8))


def fit(X, y, **kw):
    """-> (arrays dict as `parse_xgboost_json` gives, final margins (N, C) f32 on the training rows)."""
    p = dict(DEFAULTS); p.update(kw)
    X = np.asarray(X, np.float32)
    if not np.isfinite(X).all():
        raise ValueError("X holds a non-finite value")
    N, F = X.shape
    C = p["num_class"]
    cuts, n_cuts = make_cuts(X, p["max_bin"])
    bins = bin_matrix(X, cuts, n_cuts)
    margins = np.full((N, C), np.float32(p["base_score"]), np.float32)
    trees, classes = [], []
    for r in range(p["n_estimators"]):
        rmask = row_mask(p["seed"], r, N, p["subsample"])
        g, h = gradients(margins, y)
        for c in range(C):
            fmask = feature_mask(p["seed"], r * C + c, F, p["colsample_bytree"])
            tree, leaf = grow_tree(bins, cuts, n_cuts, g[c], h[c], rmask, fmask, max_depth=p["max_depth"], learning_rate=p["learning_rate"],
                                   reg_lambda=p["reg_lambda"], gamma=p["gamma"], min_child_weight=p["min_child_weight"])
            margins[:, c] = margins[:, c] + leaf.astype(np.float32)
            trees.append(tree); classes.append(c)
    return assemble(trees, classes, C, F, p["base_score"]), margins
