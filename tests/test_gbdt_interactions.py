"""SHAP interaction values of the fitted GBDT model on the CPU: ``predict(pred_interactions=True)`` against a
brute-force oracle that shares nothing with the package -- the value function of csrc/gbdt/shap_tables.h as the
recursion of test_gbdt_explain.py, and the Shapley interaction index by enumerating all 2^F feature subsets --
plus the structure xgboost's layout promises: symmetry, rows that add up to the contributions, the bias corner."""

import math

import numpy as np
import pytest

import gbdt_stage_cases as cases
from gentun_amd.models import gbdt
from gentun_amd.models.booster import Booster
from test_gbdt_explain import fit, leaf_scale, mixed_rows, odd_rows, tree_values

F8 = 8


# ---- the oracle -----------------------------------------------------------------------------------------------
def oracle_interactions(bst, rows, ntree_limit=0):
    """[n, K, F + 1, F + 1] by the definition: off the diagonal half the Shapley interaction index of sum_t v_t,
    on it the Shapley value minus the rest of the row, in the corner base + sum_t v_t(x, {})."""
    F = bst.n_features
    rounds = ntree_limit or bst.num_rounds
    fact = [math.factorial(k) for k in range(F + 1)]
    w1 = np.array([fact[k] * fact[F - k - 1] / fact[F] for k in range(F)])
    w2 = np.array([fact[k] * fact[F - k - 2] / (2.0 * fact[F - 1]) for k in range(F - 1)])
    subsets = np.arange(1 << F)
    size = np.array([bin(S).count("1") for S in subsets])
    out = np.zeros((len(rows), bst.K, F + 1, F + 1))
    for r, row in enumerate(rows):
        for c in range(bst.K):
            val = np.zeros(1 << F)
            for rnd in range(rounds):
                val += tree_values(bst, rnd * bst.K + c, row, F)
            m = out[r, c]
            for i in range(F):
                bi = 1 << i
                for j in range(i + 1, F):
                    bj = 1 << j
                    S = subsets[(subsets & (bi | bj)) == 0]
                    m[i, j] = m[j, i] = float(np.sum(w2[size[S]] * (val[S | bi | bj] - val[S | bi] - val[S | bj]
                                                                    + val[S])))
            for i in range(F):
                bi = 1 << i
                S = subsets[(subsets & bi) == 0]
                phi = float(np.sum(w1[size[S]] * (val[S | bi] - val[S])))
                m[i, i] = phi - (m[i, :F].sum() - m[i, i])
            m[F, F] = bst.base_margin + val[0]
    return out


def twelve_rows(x, seed):
    return np.concatenate([x[:6], odd_rows(x.shape[1], seed, 6)])


def check_structure(bst, rows, phi, **kw):
    """What every output promises, whatever computed it: ``kw`` goes to the pred_contribs / margin calls."""
    n, F = rows.shape
    full = phi.reshape(n, bst.K, F + 1, F + 1)
    contribs = bst.predict(rows, pred_contribs=True, **kw).reshape(n, bst.K, F + 1)
    margin = bst.predict(rows, output_margin=True, **{k: v for k, v in kw.items() if k != "nthreads"})
    margin = margin.reshape(n, bst.K)
    assert full.tobytes() == np.ascontiguousarray(full.transpose(0, 1, 3, 2)).tobytes()      # bitwise symmetric
    assert np.ascontiguousarray(full[:, :, F, F]).tobytes() == np.ascontiguousarray(contribs[:, :, F]).tobytes()
    assert np.all(full[:, :, F, :F] == 0.0) and np.all(full[:, :, :F, F] == 0.0)
    bound = 1e-12 * leaf_scale(bst, kw.get("ntree_limit", 0))
    err_rows = float(np.abs(full.sum(axis=3) - contribs).max())
    err_all = float(np.abs(full.sum(axis=(2, 3)) - margin).max())
    print("max |row sums - contribs|", err_rows, "max |sum - margin|", err_all, "bound", bound)
    assert err_rows <= bound and err_all <= bound


# ---- against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("reg", 0), ("binary", 0), ("multi", 0), ("multi", 2), ("two", 0)])
def test_interactions_equal_the_bruteforce_oracle(name, limit):
    x, _y, bst = fit(name)
    rows = twelve_rows(x, 5)
    assert len(rows) == 12
    got = bst.predict(rows, pred_interactions=True, ntree_limit=limit)
    assert got.dtype == np.float64
    assert got.shape == ((12, F8 + 1, F8 + 1) if bst.K == 1 else (12, bst.K, F8 + 1, F8 + 1))
    want = oracle_interactions(bst, rows, limit)
    bound = 1e-12 * leaf_scale(bst, limit)
    err = float(np.abs(got.reshape(want.shape) - want).max())
    print(name, limit, "max |Phi - oracle|", err, "bound", bound)
    assert err <= bound
    assert np.abs(want[:, :, :F8, :F8][:, :, ~np.eye(F8, dtype=bool)]).max() > 0.0     # there is something to find
    if name == "two":                            # the merged-element path: some path splits twice on a feature
        o, e = int(bst.tree_offsets[0]), int(bst.tree_offsets[1])
        inner = bst.feature[o:e][bst.feature[o:e] >= 0]
        assert len(inner) > len(set(inner.tolist()))


@pytest.mark.parametrize("name,limit", [("reg", 0), ("binary", 0), ("multi", 0), ("multi", 2), ("two", 0)])
def test_structure(name, limit):
    x, _y, bst = fit(name)
    rows = mixed_rows(x, 5)
    check_structure(bst, rows, bst.predict(rows, pred_interactions=True, ntree_limit=limit), ntree_limit=limit)


# ---- depth-specific models --------------------------------------------------------------------------------------
def test_stumps_have_no_interactions():
    x, _y, bst = fit("stump")
    rows = mixed_rows(x, 7)
    got = bst.predict(rows, pred_interactions=True)
    contribs = bst.predict(rows, pred_contribs=True)
    off = ~np.eye(F8 + 1, dtype=bool)
    assert np.all(got[:, off] == 0.0)
    diag = np.ascontiguousarray(got[:, np.arange(F8 + 1), np.arange(F8 + 1)])
    assert diag.tobytes() == contribs.tobytes()
    assert np.any(contribs[:, :F8] != 0.0)


def test_depth_zero_is_only_the_bias():
    x, y = fit("reg")[:2]
    bst = gbdt.train({"objective": "reg:linear", "max_depth": 0}, x, y, num_boost_round=3)
    rows = mixed_rows(x, 7)
    got = bst.predict(rows, pred_interactions=True)
    corner = got[:, F8, F8].copy()
    assert corner.tobytes() == np.ascontiguousarray(bst.predict(rows, pred_contribs=True)[:, F8]).tobytes()
    got[:, F8, F8] = 0.0
    assert np.all(got == 0.0)


# ---- thread counts ----------------------------------------------------------------------------------------------
def test_interactions_do_not_depend_on_threads():
    x, _y, bst = fit("multi")
    rows = np.concatenate([x, odd_rows(F8, 6, 300)])
    one = bst.predict(rows, pred_interactions=True, nthreads=1)
    assert one.tobytes() == bst.predict(rows, pred_interactions=True, nthreads=4).tobytes()


# ---- API behaviour ----------------------------------------------------------------------------------------------
def test_shapes_and_dtype():
    for name, K in (("reg", 1), ("multi", 3)):
        x, _y, bst = fit(name)
        assert bst.K == K
        got = bst.predict(x[:5], pred_interactions=True)
        assert got.dtype == np.float64
        assert got.shape == ((5, F8 + 1, F8 + 1) if K == 1 else (5, 3, F8 + 1, F8 + 1))
        assert bst.predict(x[0], pred_interactions=True).shape == got[:1].shape
        assert bst.predict(x[:0], pred_interactions=True).shape == (0,) + got.shape[1:]


def test_pred_interactions_excludes_the_other_outputs():
    x, _y, bst = fit("reg")
    with pytest.raises(ValueError):
        bst.predict(x[:3], pred_interactions=True, pred_contribs=True)
    with pytest.raises(ValueError):
        bst.predict(x[:3], pred_interactions=True, pred_leaf=True)


def test_file_without_statistics_says_so(tmp_path):
    x, _y, bst = fit("multi")
    path = str(tmp_path / "model.npz")
    bst.save(path)
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files if k not in ("cover", "gain")}
    old = str(tmp_path / "old.npz")
    np.savez(old, **arrays)
    with pytest.raises(ValueError, match="without node statistics"):
        Booster.load(old).predict(x[:3], pred_interactions=True)


def test_save_load_gives_the_same_bytes(tmp_path):
    x, _y, bst = fit("multi")
    path = str(tmp_path / "model.npz")
    bst.save(path)
    rows = mixed_rows(x, 8)
    want = bst.predict(rows, pred_interactions=True)
    assert Booster.load(path).predict(rows, pred_interactions=True).tobytes() == want.tobytes()


def test_paths_beyond_sixteen_unique_features_work_on_the_cpu():
    c = cases.load("B3")
    bst = gbdt.train({"objective": "reg:linear", "max_depth": 30, "min_child_weight": 0, "lambda": 0.0}, c["x"],
                     c["y"], num_boost_round=1, seed=0)
    longest, feats = 0, {0: frozenset()}
    for j in range(int(bst.tree_offsets[1])):
        if bst.feature[j] >= 0:
            feats[int(bst.left[j])] = feats[int(bst.left[j]) + 1] = feats[j] | {int(bst.feature[j])}
        else:
            longest = max(longest, len(feats[j]))
    assert 16 < longest <= 64
    rows = c["x"][:10]
    check_structure(bst, rows, bst.predict(rows, pred_interactions=True))
