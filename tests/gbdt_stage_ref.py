"""Plain numpy reference of every stage of the GBDT engines (int64 / fp64, no GPU).

One function per stage of csrc/hip/gbdt_hist.hip; each takes the *traced input* of its stage
(gentun_amd.models.gbdt_hip.cv_trace), so an error in one stage does not compound into the next and a
near-tie split cannot make the two sides diverge. The formulas are those of csrc/gbdt/engine.cpp.
:func:`chained_cv` runs the same stages as a whole cross-validation in fp64 without quantisation; it is
checked against the CPU engine in tests/test_gbdt_stage_ref.py, which is how this reference is itself
tested. Used by tests/test_gbdt_stages.py (GPU)."""

import math

import numpy as np

M64 = (1 << 64) - 1
EPS = 2.0 ** -52
P_NAMES = ("eta", "min_child_weight", "max_depth", "gamma", "max_delta_step", "subsample", "colsample_bytree",
           "colsample_bylevel", "lambda", "alpha", "scale_pos_weight", "base_score")


def pdict(parr):
    return dict(zip(P_NAMES, (float(v) for v in parr)))


# ---- random streams (cv_protocol.h splitmix / Rng / row_uniform / draw_tree / level_features) ---------------

def smix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _smix_u64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def row_uniform(key, rows):
    """cv_protocol.h row_uniform for an array of row indices (uint64 arithmetic wraps like the C++)."""
    x = _smix_u64(np.uint64(key) ^ _smix_u64(np.asarray(rows).astype(np.uint64)))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def tree_draws(seed, k, rnd, c, F, D, p):
    """The draws of one tree (fold k, round, class c): the row-subsample key (0 without subsampling) and
    every level's feature scan order (lists of feature indices), as cv_protocol.h draw_tree / level_features."""
    fold_round = smix((seed & M64) ^ smix((k * 1000003 + rnd * 7919 + 17) & M64))
    state = [fold_round if c == 0 else smix(fold_round ^ smix((c * 0x51ED27 + 3) & M64))]

    def nxt():
        state[0] = smix(state[0])
        return state[0]

    key = nxt() if p["subsample"] < 1.0 else 0
    feats = list(range(F))
    if p["colsample_bytree"] < 1.0:
        kk = max(1, int(math.floor(p["colsample_bytree"] * F + 1e-9)))
        for i in range(F):
            j = i + nxt() % (F - i)
            feats[i], feats[j] = feats[j], feats[i]
        feats = sorted(feats[:kk])
    level_key = nxt() if p["colsample_bylevel"] < 1.0 else 0
    levels = []
    for d in range(D + 1):
        lf = list(feats)
        if p["colsample_bylevel"] < 1.0 and len(lf) > 1:
            m = len(lf)
            kk = max(1, int(math.floor(p["colsample_bylevel"] * m + 1e-9)))
            ls = smix(level_key ^ smix(d + 1))
            for i in range(m):
                ls = smix(ls)
                j = i + ls % (m - i)
                lf[i], lf[j] = lf[j], lf[i]
            lf = lf[:kk]
        levels.append(lf)
    return key, levels


def order_to_feats(order_row):
    """Feature scan order (list) from the engine's table: order[f] = 1 + position of f, 0 = not sampled."""
    order_row = np.asarray(order_row)
    f = np.nonzero(order_row > 0)[0]
    return [int(v) for v in f[np.argsort(order_row[f], kind="stable")]]


# ---- gradients, fixed-point scale, quantisation ----------------------------------------------------------------

def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def grad(margin, y, kind, c=0, spw=1.0):
    """fp64 (g, h) of every row from the margins [n][K]. kind: 0 squared error, 1 reg:logistic, 2 binary
    (scale_pos_weight on the positives), 3 softmax class c."""
    m = np.asarray(margin, np.float64)
    y = np.asarray(y, np.float64)
    if kind == 0:
        return m[:, 0] - y, np.ones(len(y))
    if kind == 3:
        e = np.exp(m - m.max(axis=1, keepdims=True))
        pr = e[:, c] / e.sum(axis=1)
        return pr - (y.astype(np.int64) == c), np.maximum(2.0 * pr * (1.0 - pr), 1e-16)
    pr = sigmoid(m[:, 0])
    g, h = pr - y, np.maximum(pr * (1.0 - pr), 1e-16)
    if kind == 2:
        w = np.where(y > 0.5, spw, 1.0)
        g, h = g * w, h * w
    return g, h


def lg_n(n, hconst):
    e = 0
    while (1 << e) < n + 1:
        e += 1
    return max(e, 32) if hconst else e


def fx_exp(mx, lgn):
    """Fixed-point exponent from a fold's max |value| (fp32): max * 2^se * n < 2^62."""
    _, e = math.frexp(float(mx))                     # mx < 2^e; frexp(0) gives e = 0
    return min(100, 61 - e - lgn)


def scale(g32, h32, n, hconst):
    """(max |g|, max |h|, se_g, se_h) over all n rows of the fold."""
    mg, mh = np.float32(np.max(np.abs(g32))), np.float32(np.max(np.abs(h32)))
    lgn = lg_n(n, hconst)
    return mg, mh, fx_exp(mg, lgn), fx_exp(mh, lgn)


def quantise(v32, se):
    """rint(v * 2^se) as int64: exact (power-of-two scale, round to nearest even)."""
    return np.rint(np.asarray(v32, np.float64) * 2.0 ** se).astype(np.int64)


# ---- rows, histograms ---------------------------------------------------------------------------------------------

def root_rows(fold_of, k, key, subsample):
    """Sorted root rows of fold k: the other folds' rows, Bernoulli(subsample) by row_uniform."""
    rows = np.nonzero(np.asarray(fold_of) != k)[0]
    if subsample < 1.0:
        rows = rows[row_uniform(key, rows) < subsample]
    return rows


def _exact_bincount(idx, q, size):
    """Exact int64 sums per index: hi / lo split so that every float sum stays far below 2^53."""
    lo = (q & 0x7FFFFFFF).astype(np.float64)
    hi = (q >> 31).astype(np.float64)
    assert len(q) < (1 << 21)
    return ((np.bincount(idx, weights=hi, minlength=size).astype(np.int64) << 31)
            + np.bincount(idx, weights=lo, minlength=size).astype(np.int64))


def hist(bins, rows, qg, qh):
    """Exact histogram [F][256][2] (int64) of the rows: sums of qg[row], qh[row] per (feature, bin)."""
    F = bins.shape[1]
    rows = np.asarray(rows, np.int64)
    out = np.zeros((F, 256, 2), np.int64)
    if len(rows) == 0:
        return out
    idx = (bins[rows].astype(np.int64) + 256 * np.arange(F, dtype=np.int64)[None, :]).ravel()
    out[:, :, 0] = _exact_bincount(idx, np.repeat(qg[rows], F), F * 256).reshape(F, 256)
    out[:, :, 1] = _exact_bincount(idx, np.repeat(qh[rows], F), F * 256).reshape(F, 256)
    return out


def hist_f64(bins, rows, g, h):
    """fp64 histogram (the chained driver: no quantisation), rows summed in list order."""
    F = bins.shape[1]
    idx = (bins[rows].astype(np.int64) + 256 * np.arange(F, dtype=np.int64)[None, :]).ravel()
    out = np.zeros((F, 256, 2))
    out[:, :, 0] = np.bincount(idx, weights=np.repeat(g[rows], F), minlength=F * 256).reshape(F, 256)
    out[:, :, 1] = np.bincount(idx, weights=np.repeat(h[rows], F), minlength=F * 256).reshape(F, 256)
    return out


# ---- gains, split scan ----------------------------------------------------------------------------------------------

def _thr_l1(g, a):
    return np.where(g > a, g - a, np.where(g < -a, g + a, 0.0))


def calc_weight(p, G, H):
    G, H = np.asarray(G, np.float64), np.asarray(H, np.float64)
    ok = ~((H < p["min_child_weight"]) | (H <= 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = -_thr_l1(G, p["alpha"]) / (H + p["lambda"])
    if p["max_delta_step"] != 0.0:
        w = np.where(np.abs(w) > p["max_delta_step"], np.copysign(p["max_delta_step"], w), w)
    return np.where(ok, w, 0.0)


def calc_gain(p, G, H):
    G, H = np.asarray(G, np.float64), np.asarray(H, np.float64)
    ok = ~((H < p["min_child_weight"]) | (H <= 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        if p["max_delta_step"] == 0.0:
            t = _thr_l1(G, p["alpha"])
            r = t * t / (H + p["lambda"])
        else:
            w = calc_weight(p, G, H)
            r = -(2.0 * G * w + (H + p["lambda"]) * w * w)
            if p["alpha"] != 0.0:
                r = r + p["alpha"] * np.abs(w)
    return np.where(ok, r, 0.0)


def scan(hnode, G, H, feats, nbins, p, ig=1.0, ih=1.0):
    """engine.cpp build_tree's sequential scan over one node's histogram [F][256][2] (int64 with the
    fixed-point steps ig, ih, or fp64 with 1, 1), features in the level's order ``feats``, bins b with
    b + 1 < nbins[f]: a later candidate replaces the best only if better by more than 1e-12.

    Returns None without a candidate, else a dict: feature, bin, gain, GL, HL (prefix sums in the
    histogram's own type), ``gap`` = gain - (largest gain of a candidate that makes other children, see below), ``tol`` =
    2e-12 + 64 eps (|gain_L| + |gain_R| + |gain_parent|) and ``gains`` = {feature: gains per bin, nan
    where not a candidate}."""
    if len(feats) == 0:
        return None
    feats = np.asarray(feats, np.int64)
    pre = np.cumsum(hnode[feats], axis=1)                         # exact for int64
    GLr, HLr = pre[:, :, 0], pre[:, :, 1]
    GL, HL = GLr.astype(np.float64) * ig, HLr.astype(np.float64) * ih
    Gf, Hf = float(G) * ig, float(H) * ih
    GR, HR = Gf - GL, Hf - HL
    mcw = p["min_child_weight"]
    valid = (np.arange(256)[None, :] + 1 < np.asarray(nbins)[feats][:, None])
    valid &= ~((HL < mcw) | (HR < mcw) | (HL <= 0.0) | (HR <= 0.0))
    gl, gr, gp = calc_gain(p, GL, HL), calc_gain(p, GR, HR), float(calc_gain(p, Gf, Hf))
    chg = gl + gr - gp
    gains = {int(f): np.where(valid[i], chg[i], np.nan) for i, f in enumerate(feats)}
    cand = (valid & (chg > 1e-12)).ravel()
    pos = np.nonzero(cand)[0]
    if len(pos) == 0:
        return None
    c = chg.ravel()[pos]
    at = 0
    while True:                                                     # the sequential record chain
        later = np.nonzero(c[at + 1:] > c[at] + 1e-12)[0]
        if len(later) == 0:
            break
        at += 1 + int(later[0])
    fi, b = divmod(int(pos[at]), 256)
    # a candidate differs from the chosen one when it makes other children: the same (GL, HL) (an empty bin,
    # a duplicated column) or the mirrored pair (GL, HL) = (G - GL*, H - H*) (another feature sorting the
    # same rows the other way round; tiny nodes do this all the time) gives the same two gain terms, so the
    # scan order decides and not the rounding. Integers: the mirror is exact only while every sum converts
    # to fp64 exactly (< 2^53); fp64 sums: up to their own rounding, 64 eps (|G| + |GL*|).
    same = (GLr == GLr[fi, b]) & (HLr == HLr[fi, b])
    if np.issubdtype(hnode.dtype, np.integer):
        if max(abs(int(G)), abs(int(H)), int(np.abs(pre).max())) < (1 << 53):
            same |= (GLr == int(G) - int(GLr[fi, b])) & (HLr == int(H) - int(HLr[fi, b]))
    else:
        same |= ((np.abs(GLr - (Gf - GLr[fi, b])) <= 64 * EPS * (abs(Gf) + abs(GLr[fi, b])))
                 & (np.abs(HLr - (Hf - HLr[fi, b])) <= 64 * EPS * (abs(Hf) + abs(HLr[fi, b]))))
    other = chg[valid & ~same]
    gap = float(c[at] - other.max()) if other.size else math.inf
    tol = 2e-12 + 64 * EPS * (abs(float(gl[fi, b])) + abs(float(gr[fi, b])) + abs(gp))
    return {"feature": int(feats[fi]), "bin": b, "gain": float(c[at]), "GL": GLr[fi, b], "HL": HLr[fi, b],
            "gap": gap, "tol": tol, "gains": gains}


# ---- plan, partition, walk ------------------------------------------------------------------------------------------

def leaf_value(p, G, H, ig=1.0, ih=1.0):
    """weight x eta as the fp32 the engines store."""
    return np.float32(float(calc_weight(p, float(G) * ig, float(H) * ih)) * p["eta"])


def keeps_split(p, feature, bin_, gain):
    """The pruning rule (engine.cpp: best.feature < 0 || gain < gamma || gain <= 1e-12 -> leaf)."""
    return feature >= 0 and bin_ >= 0 and gain >= p["gamma"] and gain > 1e-12


def partition(bins, rows, feature, thr):
    """(left rows, right rows) of a split: left = bin <= thr; list order kept."""
    rows = np.asarray(rows)
    left = bins[rows, feature] <= thr
    return rows[left], rows[~left]


def walk(bins, tree_fb, D):
    """Heap index of the leaf every row reaches. tree_fb: [2^(D+1) - 1][2] (feature, bin), feature < 0 = leaf."""
    n = bins.shape[0]
    node = np.zeros(n, np.int64)
    ar = np.arange(n)
    for _ in range(D + 1):
        f, t = tree_fb[node, 0], tree_fb[node, 1]
        inner = f >= 0
        if not inner.any():
            break
        go_left = bins[ar, np.where(inner, f, 0)] <= t
        node = np.where(inner, np.where(go_left, 2 * node + 1, 2 * node + 2), node)
    return node


# ---- metrics ------------------------------------------------------------------------------------------------------------

def metric_terms(metric, objective, margin, y):
    """Per-row fp64 term of metric 0 rmse (squared error), 1 mae, 2 logloss, 3 error, 5 merror, 6 mlogloss;
    objective: the engine's code (0 reg:linear .. 5 multi:softprob). margin [n][K]."""
    m = np.asarray(margin, np.float64)
    y = np.asarray(y, np.float64)
    eps = 1e-15
    if metric in (0, 1):
        pred = sigmoid(m[:, 0]) if objective in (1, 2) else m[:, 0]
        d = pred - y
        return d * d if metric == 0 else np.abs(d)
    if metric == 2:
        pr = np.minimum(1 - eps, np.maximum(eps, sigmoid(m[:, 0])))
        return -(y * np.log(pr) + (1 - y) * np.log(1 - pr))
    if metric == 3:
        pos = (m[:, 0] > 0.0) if objective == 3 else (sigmoid(m[:, 0]) > 0.5)
        return (pos != (y > 0.5)).astype(np.float64)
    arg = np.argmax(m, axis=1)                                     # first maximum, as the engines
    if metric == 5:
        return (arg != y.astype(np.int64)).astype(np.float64)
    mx = m.max(axis=1)
    z = np.exp(m - mx[:, None]).sum(axis=1)
    pr = np.maximum(eps, np.exp(m[np.arange(len(y)), y.astype(np.int64)] - mx) / z)
    return -np.log(pr)


def metric_value(metric, terms):
    v = float(np.sum(terms)) / max(1, len(terms))
    return math.sqrt(v) if metric == 0 else v


def auc_sums(score, y):
    """(tie-averaged rank sum of the positives, positives, negatives) of engine.cpp auc_score."""
    score = np.asarray(score) + 0.0                               # -0 -> +0
    y = np.asarray(y)
    o = np.argsort(score, kind="stable")
    s = score[o]
    first = np.concatenate(([True], s[1:] != s[:-1]))
    gid = np.cumsum(first) - 1
    starts = np.nonzero(first)[0]
    ends = np.concatenate((starts[1:], [len(s)])) - 1
    avg = 0.5 * (starts + ends) + 1.0
    pos = y[o] > 0.5
    return float(np.sum(avg[gid][pos])), int(pos.sum()), int((~pos).sum())


def auc_value(rank_sum, npos, nneg):
    if npos == 0 or nneg <= 0:
        return 0.5
    return (rank_sum - npos * (npos + 1) / 2) / (npos * nneg)


# ---- the chained driver: a whole CV from the stages above, fp64, no quantisation ----------------------------

def _kind(objective):
    return 3 if objective >= 4 else (0 if objective == 0 else (1 if objective == 1 else 2))


def chained_cv(bins, nbins, y, fold_of, nfold, parr, objective, num_class, metrics, nrounds, seed):
    """gbdt_cv (engine.cpp) rebuilt from the stage functions. Returns (history [nrounds][n_metrics][4],
    stats) with stats = {"split_nodes", "ambiguous"}: nodes whose best split's gap to a different
    candidate is below scan()'s tol."""
    p = pdict(parr)
    n, F = bins.shape
    y = np.asarray(y, np.float32)
    fold_of = np.asarray(fold_of)
    D = max(0, int(p["max_depth"]))
    K = max(2, num_class) if objective >= 4 else 1
    kind = _kind(objective)
    base = p["base_score"]
    if objective in (1, 2):
        b = min(1 - 1e-7, max(1e-7, base))
        base = math.log(b / (1 - b))
    margins = [np.full((n, K), base, np.float64) for _ in range(nfold)]
    tsz = (2 << D) - 1
    out = np.zeros((nrounds, len(metrics), 4))
    stats = {"split_nodes": 0, "ambiguous": 0}
    for rnd in range(nrounds):
        vals = np.zeros((nfold, len(metrics), 2))
        for k in range(nfold):
            train = np.nonzero(fold_of != k)[0]
            test = np.nonzero(fold_of == k)[0]
            for c in range(K):
                key, levels = tree_draws(seed, k, rnd, c, F, D, p)
                g, h = grad(margins[k], y, kind, c, p["scale_pos_weight"])
                rows0 = root_rows(fold_of, k, key, p["subsample"])
                tree = np.full((tsz, 2), -1, np.int64)
                leaf = np.zeros(tsz)
                level = [(0, rows0, float(np.sum(g[rows0])), float(np.sum(h[rows0])))]
                for d in range(D + 1):
                    nxt = []
                    for j, rows, G, H in level:
                        nid = (1 << d) - 1 + j
                        leaf[nid] = float(calc_weight(p, G, H)) * p["eta"]
                        if d == D or len(rows) < 2:
                            continue
                        s = scan(hist_f64(bins, rows, g, h), G, H, levels[d], nbins, p)
                        if s is None or not keeps_split(p, s["feature"], s["bin"], s["gain"]):
                            continue
                        stats["split_nodes"] += 1
                        stats["ambiguous"] += s["gap"] < s["tol"]
                        tree[nid] = (s["feature"], s["bin"])
                        lr, rr = partition(bins, rows, s["feature"], s["bin"])
                        nxt.append((2 * j, lr, float(s["GL"]), float(s["HL"])))
                        nxt.append((2 * j + 1, rr, G - float(s["GL"]), H - float(s["HL"])))
                    level = nxt
                margins[k][:, c] += leaf[walk(bins, tree, D)]
            for mi, met in enumerate(metrics):
                for q, rows in enumerate((train, test)):
                    if met == 4:
                        vals[k, mi, q] = auc_value(*auc_sums(margins[k][rows, 0], y[rows]))
                    else:
                        vals[k, mi, q] = metric_value(met, metric_terms(met, objective, margins[k][rows], y[rows]))
        out[rnd, :, 0], out[rnd, :, 1] = vals[:, :, 0].mean(axis=0), vals[:, :, 0].std(axis=0)
        out[rnd, :, 2], out[rnd, :, 3] = vals[:, :, 1].mean(axis=0), vals[:, :, 1].std(axis=0)
    return out, stats
