"""Feature importance and SHAP contributions of the fitted GBDT model on the CPU: the node statistics (cover,
gain) out of the engine, ``Booster.get_score``, and ``predict(pred_contribs=True)`` against a brute-force oracle
that shares nothing with the package: the value function of csrc/gbdt/shap_tables.h written as a recursion, and
Shapley values by enumerating all 2^F feature subsets."""

import json
import math

import numpy as np
import pytest

import gbdt_stage_ref as ref
from gentun_amd.models import gbdt
from gentun_amd.models.booster import Booster
from gentun_amd.utils.data import make_regression

F8 = 8


# ---- the oracle -----------------------------------------------------------------------------------------------
def tree_values(bst, t, row, n_features):
    """v_t(row, S) for every feature subset S (bit i of the index = feature i in S)."""
    o = int(bst.tree_offsets[t])
    out = np.zeros(1 << n_features)
    for S in range(1 << n_features):
        def rec(j):
            f = int(bst.feature[o + j])
            if f < 0:
                return float(bst.value[o + j])
            lch = int(bst.left[o + j])
            if (S >> f) & 1:
                return rec(lch if not (row[f] > bst.threshold[o + j]) else lch + 1)
            cl, cr = float(bst.cover[o + lch]), float(bst.cover[o + lch + 1])
            return cl / (cl + cr) * rec(lch) + cr / (cl + cr) * rec(lch + 1)
        out[S] = rec(0)
    return out


def oracle_contribs(bst, rows, ntree_limit=0):
    """[n, K, F + 1] by the definition: Shapley values of sum_t v_t per class, bias = base + sum_t v_t(x, {})."""
    n_features = bst.n_features
    rounds = ntree_limit or bst.num_rounds
    fact = [math.factorial(k) for k in range(n_features + 1)]
    weight = [fact[k] * fact[n_features - k - 1] / fact[n_features] for k in range(n_features)]
    size = np.array([bin(S).count("1") for S in range(1 << n_features)])
    out = np.zeros((len(rows), bst.K, n_features + 1))
    for r, row in enumerate(rows):
        for c in range(bst.K):
            val = np.zeros(1 << n_features)
            for rnd in range(rounds):
                val += tree_values(bst, rnd * bst.K + c, row, n_features)
            for i in range(n_features):
                without = np.array([S for S in range(1 << n_features) if not (S >> i) & 1])
                out[r, c, i] = sum(weight[size[S]] * (val[S | (1 << i)] - val[S]) for S in without)
            out[r, c, n_features] = bst.base_margin + val[0]
    return out


def leaf_scale(bst, ntree_limit=0):
    """S of the bound: |base_margin| + sum over the used trees' leaves of |value|."""
    end = int(bst.tree_offsets[(ntree_limit or bst.num_rounds) * bst.K])
    leaf = bst.feature[:end] < 0
    return abs(bst.base_margin) + float(np.abs(bst.value[:end][leaf]).sum())


def odd_rows(F, seed, n):
    """Rows no model saw: NaN, +-inf and values beyond the training range."""
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((n, F))).astype(np.float32)
    for p, v in ((0.05, np.nan), (0.02, np.inf), (0.02, -np.inf), (0.02, 1e30), (0.02, -1e30)):
        z[rng.random(z.shape) < p] = v
    return z


# ---- models ---------------------------------------------------------------------------------------------------
N = 2000
_FITS = {}


def _data(kind):
    x, y = make_regression(n=N, f=F8, seed=21)
    x = np.ascontiguousarray(x, np.float32)
    if kind == "binary":
        y = (y > np.median(y)).astype(np.float32)
    elif kind == "multi":
        y = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3])).astype(np.float32)
    elif kind == "two":                          # only two informative features: paths repeat a feature
        y = (np.sin(2.0 * x[:, 1]) + x[:, 4] * x[:, 4]).astype(np.float32)
    return x, np.ascontiguousarray(y, np.float32)


MODELS = {
    "reg": ("reg", {"objective": "reg:linear", "max_depth": 4}, 6),
    "binary": ("binary", {"objective": "binary:logistic", "max_depth": 3}, 3),
    "multi": ("multi", {"objective": "multi:softprob", "num_class": 3, "max_depth": 3}, 3),
    "two": ("two", {"objective": "reg:linear", "max_depth": 5}, 3),
    "stump": ("reg", {"objective": "reg:linear", "max_depth": 1}, 2),
}


def fit(name):
    if name not in _FITS:
        kind, params, rounds = MODELS[name]
        x, y = _data(kind)
        _FITS[name] = (x, y, gbdt.train(params, x, y, num_boost_round=rounds, seed=3))
    return _FITS[name]


def mixed_rows(x, seed):
    return np.concatenate([x[:20], odd_rows(x.shape[1], seed, 20)])


def reach_counts(bst, t, x, weights=None):
    """Per node of tree t: the (weighted) number of rows of x that reach it, by a numpy walk."""
    o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
    out = np.zeros(e - o)
    members = {0: np.arange(len(x))}
    for j in range(e - o):
        rows = members[j]
        out[j] = len(rows) if weights is None else float(np.sum(weights[rows]))
        if bst.feature[o + j] >= 0:
            right = x[rows, bst.feature[o + j]] > bst.threshold[o + j]
            members[int(bst.left[o + j])] = rows[~right]
            members[int(bst.left[o + j]) + 1] = rows[right]
    return out, members


# ---- contributions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("reg", 0), ("binary", 0), ("multi", 0), ("multi", 2), ("two", 0)])
def test_contribs_equal_the_bruteforce_oracle(name, limit):
    x, _y, bst = fit(name)
    rows = mixed_rows(x, 5)
    assert len(rows) == 40
    got = bst.predict(rows, pred_contribs=True, ntree_limit=limit)
    assert got.dtype == np.float64
    assert got.shape == ((40, F8 + 1) if bst.K == 1 else (40, bst.K, F8 + 1))
    want = oracle_contribs(bst, rows, limit)
    bound = 1e-12 * leaf_scale(bst, limit)
    err = float(np.abs(got.reshape(want.shape) - want).max())
    print(name, limit, "max |phi - oracle|", err, "bound", bound)
    assert err <= bound
    if name == "two":                            # the merged-element path: some path splits twice on a feature
        o, e = int(bst.tree_offsets[0]), int(bst.tree_offsets[1])
        inner = bst.feature[o:e][bst.feature[o:e] >= 0]
        assert len(inner) > len(set(inner.tolist()))


def test_contribs_do_not_depend_on_threads():
    x, _y, bst = fit("multi")
    rows = np.concatenate([x, odd_rows(F8, 6, 300)])
    one = bst.predict(rows, pred_contribs=True, nthreads=1)
    assert one.tobytes() == bst.predict(rows, pred_contribs=True, nthreads=4).tobytes()


_WIDE = {}


def wide_fit():
    if not _WIDE:
        x, y = make_regression(n=5000, f=33, seed=2)
        x = np.ascontiguousarray(x, np.float32)
        y = (y > np.median(y)).astype(np.float32)
        _WIDE["fit"] = (x, y, gbdt.train({"objective": "binary:logistic", "max_depth": 5}, x, y, num_boost_round=5))
    return _WIDE["fit"]


def test_additivity_and_bias_on_5000_by_33():
    x, _y, bst = wide_fit()
    assert x.shape == (5000, 33)
    got = bst.predict(x, pred_contribs=True)
    margin = bst.predict(x, output_margin=True)
    bound = 1e-12 * leaf_scale(bst)
    err = float(np.abs(got.sum(axis=1) - margin).max())
    print("max |sum phi - margin|", err, "bound", bound)
    assert err <= bound
    # the bias: one value for every row, base + sum_t E_t with E_t recomputed here from the covers
    assert np.all(got[:, -1] == got[0, -1])
    bias = bst.base_margin
    for t in range(bst.num_trees):
        o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
        reach = np.zeros(e - o)
        reach[0] = 1.0
        for j in range(e - o):
            if bst.feature[o + j] >= 0:
                lch = int(bst.left[o + j])
                cl, cr = bst.cover[o + lch], bst.cover[o + lch + 1]
                reach[lch], reach[lch + 1] = reach[j] * cl / (cl + cr), reach[j] * cr / (cl + cr)
        leaf = bst.feature[o:e] < 0
        bias += float(np.sum(reach[leaf] * bst.value[o:e][leaf]))
    assert abs(got[0, -1] - bias) <= bound


def test_depth_zero_contributes_only_the_bias():
    x, y = _data("reg")
    bst = gbdt.train({"objective": "reg:linear", "max_depth": 0}, x, y, num_boost_round=3)
    got = bst.predict(mixed_rows(x, 7), pred_contribs=True)
    assert np.all(got[:, :-1] == 0.0)
    assert np.all(np.abs(got[:, -1] - (bst.base_margin + bst.value.sum())) <= 1e-12 * leaf_scale(bst))
    assert np.all(bst.gain == 0.0) and bst.get_score("weight") == {}


# ---- node statistics ------------------------------------------------------------------------------------------
def test_cover_is_the_row_count_for_squared_error():
    x, _y, bst = fit("reg")
    assert bst.cover.dtype == np.float64 and bst.gain.dtype == np.float64
    assert len(bst.cover) == len(bst.gain) == len(bst.feature)
    for t in range(bst.num_trees):
        o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
        counts, _ = reach_counts(bst, t, x)
        assert bst.cover[o:e].tolist() == counts.tolist(), t
    assert np.all(bst.gain[bst.feature < 0] == 0.0) and np.all(bst.gain[bst.feature >= 0] > 0.0)


def _tree0_gradients(name):
    x, y, bst = fit(name)
    if name == "reg":
        return x, bst, bst.base_margin - y.astype(np.float64), np.ones(len(y))
    p = 1.0 / (1.0 + math.exp(-bst.base_margin))
    return x, bst, p - y.astype(np.float64), np.full(len(y), max(p * (1.0 - p), 1e-16))


def test_binary_tree0_cover_is_the_hessian_sum():
    x, bst, _g, h = _tree0_gradients("binary")
    want, _ = reach_counts(bst, 0, x, weights=h)
    got = bst.cover[:int(bst.tree_offsets[1])]
    assert np.all(np.abs(got - want) <= 1e-9 * want)


@pytest.mark.parametrize("name", ["reg", "binary"])
def test_tree0_gain_is_the_loss_change_of_the_split(name):
    x, bst, g, h = _tree0_gradients(name)
    p = dict(bst.params)
    _, members = reach_counts(bst, 0, x)
    G = {j: float(np.sum(g[rows])) for j, rows in members.items()}
    H = {j: float(np.sum(h[rows])) for j, rows in members.items()}
    checked = 0
    for j in range(int(bst.tree_offsets[1])):
        if bst.feature[j] < 0:
            continue
        lch = int(bst.left[j])
        want = float(ref.calc_gain(p, G[lch], H[lch]) + ref.calc_gain(p, G[lch + 1], H[lch + 1])
                     - ref.calc_gain(p, G[j], H[j]))
        print(name, "node", j, "gain", bst.gain[j], "recomputed", want)
        assert abs(bst.gain[j] - want) <= 1e-9 * abs(want)
        checked += 1
    assert checked >= 3


def test_subsample_covers_the_sampled_rows_only():
    x, y = _data("reg")
    bst = gbdt.train({"objective": "reg:linear", "max_depth": 3, "subsample": 0.6}, x, y, num_boost_round=2)
    for t in range(bst.num_trees):
        assert 0.0 < bst.cover[int(bst.tree_offsets[t])] < len(x)


# ---- get_score ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reg", "multi", "stump"])
def test_get_score_against_numpy(name):
    _x, _y, bst = fit(name)
    used = sorted(set(bst.feature[bst.feature >= 0].tolist()))
    if name == "stump":
        assert 1 <= len(used) <= 2
    for kind in ("weight", "gain", "cover", "total_gain", "total_cover"):
        got = bst.get_score(kind)
        assert sorted(got) == sorted("f{}".format(j) for j in used)
        for j in used:
            sel = bst.feature == j
            stat = bst.gain[sel] if kind.endswith("gain") else bst.cover[sel]
            want = {"weight": int(sel.sum())}.get(kind, stat.sum() if kind.startswith("total_") else stat.mean())
            assert got["f{}".format(j)] == pytest.approx(want, rel=1e-12), (kind, j)
    assert bst.get_fscore() == bst.get_score("weight") == bst.get_score()
    with pytest.raises(ValueError):
        bst.get_score("shap")


# ---- persistence ----------------------------------------------------------------------------------------------
def test_save_load_keeps_statistics_and_contribs(tmp_path):
    x, _y, bst = fit("multi")
    path = str(tmp_path / "model.npz")
    bst.save(path)
    back = Booster.load(path)
    assert back.cover.tobytes() == bst.cover.tobytes() and back.gain.tobytes() == bst.gain.tobytes()
    rows = mixed_rows(x, 8)
    assert back.predict(rows, pred_contribs=True).tobytes() == bst.predict(rows, pred_contribs=True).tobytes()
    with np.load(path, allow_pickle=False) as f:
        assert json.loads(str(f["header"][()]))["format"] == "gentun-gbdt/1"


def test_file_without_statistics_loads_and_says_so(tmp_path):
    x, _y, bst = fit("multi")
    path = str(tmp_path / "model.npz")
    bst.save(path)
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files if k not in ("cover", "gain")}
    old = str(tmp_path / "old.npz")
    np.savez(old, **arrays)
    back = Booster.load(old)
    assert back.cover is None and back.gain is None
    rows = mixed_rows(x, 9)
    assert back.predict(rows, output_margin=True).tobytes() == bst.predict(rows, output_margin=True).tobytes()
    assert back.get_score("weight") == bst.get_score("weight")
    with pytest.raises(ValueError, match="without node statistics"):
        back.predict(rows, pred_contribs=True)
    with pytest.raises(ValueError, match="without node statistics"):
        back.get_score("gain")


# ---- error paths ----------------------------------------------------------------------------------------------
def test_pred_contribs_excludes_pred_leaf():
    x, _y, bst = fit("reg")
    with pytest.raises(ValueError):
        bst.predict(x[:3], pred_contribs=True, pred_leaf=True)


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_bad_child_covers_are_a_malformed_forest(bad):
    x, _y, bst = fit("reg")
    cover = bst.cover.copy()
    lch = int(bst.left[0])
    cover[lch] = bad
    cover[lch + 1] = 0.0 if bad == 0.0 else cover[lch + 1]
    broken = Booster(bst.tree_offsets, bst.feature, bst.threshold, bst.split_bin, bst.left, bst.value, bst.objective,
                     bst.K, bst.base_margin, bst.n_features, bst.params, bst.history, cover=cover, gain=bst.gain)
    with pytest.raises(ValueError, match="malformed"):
        broken.predict(x[:3], pred_contribs=True)
