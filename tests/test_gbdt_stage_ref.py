"""The stage reference (tests/gbdt_stage_ref.py) is itself checked here, without a GPU: its chained driver
against the CPU engine, its exact histogram against np.add.at, the ambiguous-node share of every GPU case,
and the numpy mirrors of the engine's structs. Measured values: profiles/gbdt_stage_oracle.txt."""

import numpy as np
import pytest

import gbdt_stage_cases as cases
import gbdt_stage_ref as ref
from gentun_amd.models import gbdt
from gentun_amd.utils.data import kfold, make_regression

# name -> (params, bound). Bound = 100x the largest relative deviation of any metric column, chained driver
# vs gbdt.cv, measured per case (profiles/gbdt_stage_oracle.txt: 8.6e-14, 1.4e-13, 1.6e-13, 3.2e-15,
# 9.7e-15), never looser than 1e-6: both sides are fp64 and differ only in summation order
TINY = {
    "reg:linear": ({"objective": "reg:linear", "eval_metric": ["rmse", "mae"]}, 8.6e-12),
    "binary:logistic": ({"objective": "binary:logistic", "scale_pos_weight": 2.0,
                         "eval_metric": ["logloss", "error", "auc"]}, 1.5e-11),
    "multi:softprob": ({"objective": "multi:softprob", "num_class": 3, "eval_metric": ["merror", "mlogloss"]}, 1.7e-11),
    "sampling": ({"objective": "reg:linear", "subsample": 0.7, "colsample_bytree": 0.7, "colsample_bylevel": 0.6},
                 3.3e-13),
    "regularised": ({"objective": "reg:linear", "lambda": 3.0, "alpha": 0.5, "gamma": 0.1, "max_delta_step": 0.3,
                     "min_child_weight": 5}, 9.8e-13),
}


def _tiny_data(name):
    x, y = make_regression(n=600, f=6, seed=21)
    if name == "binary:logistic":
        y = (y > np.median(y)).astype(np.float32)
    elif name == "multi:softprob":
        y = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3])).astype(np.float32)
    return x, y


def _chained(params, x, y, folds, rounds, seed):
    p, obj = gbdt.resolve_params(params)
    metric = params.get("eval_metric") or gbdt.DEFAULT_METRIC[obj]
    metrics = [metric] if isinstance(metric, str) else list(metric)
    bins, nb = gbdt.quantize(x)
    fold_of = np.full(len(y), -1, np.int32)
    for k, (_tr, va) in enumerate(folds):
        fold_of[va] = k
    parr = np.array([p[k] for k in gbdt.PARAM_ORDER], np.float64)
    hist, stats = ref.chained_cv(bins, nb, y, fold_of, len(folds), parr, obj, int(params.get("num_class", 0) or 0),
                                 [gbdt.METRICS[m] for m in metrics], rounds, seed)
    return metrics, hist, stats


@pytest.mark.parametrize("name", sorted(TINY))
def test_chained_driver_matches_cpu_engine(name):
    params, bound = TINY[name]
    params = dict(params, max_depth=3, eta=0.3)
    x, y = _tiny_data(name)
    folds = kfold(600, 3, seed=0)
    cpu = gbdt.cv(params, x, y, num_boost_round=6, nfold=3, seed=5, folds=folds)
    metrics, hist, _ = _chained(params, x, y, folds, 6, 5)
    worst = 0.0
    for j, m in enumerate(metrics):
        for q, col in enumerate(("train-{}-mean", "train-{}-std", "test-{}-mean", "test-{}-std")):
            a = np.array(cpu[col.format(m)])
            dev = np.max(np.abs(a - hist[:, j, q]) / np.maximum(np.abs(a), 1e-300))
            worst = max(worst, float(dev))
    print("chained vs cpu engine [{}]: max relative deviation {:.3e} (bound {:.1e})".format(name, worst, bound))
    assert worst <= min(bound, 1e-6)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_gpu_cases_have_few_ambiguous_nodes(name):
    """The share of split nodes whose best candidate is within scan()'s tol of a different one stays at or
    below 1 % on every GPU case (the duplicated column of F1 / F2 ties exactly: scan order decides)."""
    c = cases.load(name)
    bins, nb = gbdt.quantize(c["x"])
    _, stats = ref.chained_cv(bins, nb, c["y"], c["fold_of"], c["nfold"], c["parr"], c["obj"], c["num_class"],
                              [int(m) for m in c["marr"]], c["traced"], c["seed"])
    print("case {}: {} split nodes, {} ambiguous, grid {} ({}multiple of 8)".format(
        name, stats["split_nodes"], stats["ambiguous"], c["grid"], "" if c["grid"] % 8 == 0 else "not a "))
    assert stats["ambiguous"] <= 0.01 * stats["split_nodes"]


def test_exact_histogram_matches_add_at():
    rng = np.random.default_rng(3)
    n, F = 4000, 7
    bins = rng.integers(0, 256, (n, F)).astype(np.uint8)
    qg = rng.integers(-(1 << 49), 1 << 49, n)                     # sums far above 2^53
    qh = rng.integers(0, 1 << 49, n)
    rows = rng.permutation(n)[:3001]
    want = np.zeros((F, 256, 2), np.int64)
    for f in range(F):
        np.add.at(want[f, :, 0], bins[rows, f], qg[rows])
        np.add.at(want[f, :, 1], bins[rows, f], qh[rows])
    np.testing.assert_array_equal(ref.hist(bins, rows, qg, qh), want)


def test_scan_rule_ties_and_gap():
    """Equal integers in two features: the earlier one in scan order wins and the tie is not a gap; a
    candidate better by less than 1e-12 does not replace an earlier one."""
    p = ref.pdict([0.3, 1.0, 3, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.5])
    h = np.zeros((3, 256, 2), np.int64)
    h[0, :4] = [(-40, 10), (-10, 10), (10, 10), (40, 10)]
    h[1] = h[0]
    h[2, :2] = [(-20, 20), (20, 20)]
    nb = [4, 4, 2]
    for feats, want in (([0, 1, 2], 0), ([1, 0, 2], 1), ([2, 1, 0], 1)):
        s = ref.scan(h, 0, 40, feats, nb, p)
        assert (s["feature"], s["bin"]) == (want, 1) and s["gap"] > 1.0
    hf = h.astype(np.float64)
    hf[1, 0, 0] -= 1.5e-14                                         # feature 1 better by ~1e-13 < 1e-12
    s = ref.scan(hf, 0.0, 40.0, [0, 1], nb, p)
    assert s["gains"][1][1] > s["gains"][0][1] and s["feature"] == 0 and s["gap"] < s["tol"]


def test_auc_sums_match_bruteforce():
    rng = np.random.default_rng(4)
    s = np.round(rng.standard_normal(300), 1).astype(np.float32)  # heavy ties
    y = (rng.random(300) < 0.4).astype(np.float32)
    r, npos, nneg = ref.auc_sums(s, y)
    want = sum(0.5 * ((s < v).sum() + 1 + (s <= v).sum()) for v in s[y > 0.5])
    assert r == want and npos == int(y.sum()) and nneg == 300 - npos


def test_struct_mirrors_match_engine_layout():
    from gentun_amd.models import gbdt_hip as H
    lay = H.trace_layout()
    assert lay["LNode"] == H.LNODE.itemsize and lay["Chunk"] == H.CHUNK.itemsize and lay["Red"] == H.RED.itemsize
    assert lay["SplitOut"] == H.SPLITOUT.itemsize and lay["NodeBest"] == H.NODEBEST.itemsize
    assert lay["GB_R"] == 16384 and lay["HB_FC"] == 32 and lay["HB_FG"] == 16 and lay["GB_MAXD"] == 12
