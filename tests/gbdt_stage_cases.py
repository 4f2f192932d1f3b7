"""Datasets and parameters of the GBDT stage-oracle cases (tests/test_gbdt_stages.py on the GPU; the CPU
test tests/test_gbdt_stage_ref.py counts their ambiguous nodes with the chained reference driver).

``grid`` is the histogram launch's grid product maxch x nfb x nfold (maxch = ceil(n / 16384) + 2^(D-1) + 2,
nfb = ceil(F / 32) on the packed squared-error path, ceil(F / 16) on the (g, h) path): hist_kernel remaps
its workgroups over the XCDs only when the product is a multiple of 8."""

import numpy as np

from gentun_amd.models import gbdt
from gentun_amd.utils.data import kfold, make_regression


def _reg(n, f, seed):
    return make_regression(n=n, f=max(f, 5), seed=seed)


def _binary(n, f, seed):
    x, y = _reg(n, f, seed)
    return x, (y > np.median(y)).astype(np.float32)


def _multi(n, f, seed):
    x, y = _reg(n, f, seed)
    return x, np.digitize(y, np.quantile(y, [1 / 3, 2 / 3])).astype(np.float32)


def _wide(n, f, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, f)).astype(np.float32)
    y = (x[:, 0] + 0.5 * x[:, f // 2] - x[:, f - 1] + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return x, y


def _odd_columns(n, seed):
    x, y = _reg(n, 8, seed)
    rng = np.random.default_rng(seed + 100)
    x[:, 5] = x[:, 0]                                   # duplicated column: exact gain ties across features
    x[:, 6] = 7.0                                       # constant
    x[:, 7] = np.nan                                    # NaN column
    x[:, 2] = rng.integers(0, 3, n)                     # 3-valued
    return x, y


def _flat(n, seed):
    x, _ = _reg(n, 6, seed)
    return x, np.full(n, 0.5, np.float32)               # y == base_score: all gradients zero


# name -> (data maker, args, params, nfold, rounds, traced rounds, heavy tags on, seed, grid product)
CASES = {
    # bench-width predict (R 64, 4 threads per row, 5 folds over 4 lanes); packed histogram, 8 feature blocks
    "A": (_wide, (6000, 256, 1), {"objective": "reg:linear", "max_depth": 4}, 5, 2, 2, True, 0, 11 * 8 * 5),
    # packed tail block with one real feature; 7 x 2 x 4 = 56 is remapped, 7 x 2 x 3 = 42 is not
    "B4": (_reg, (5000, 33, 2), {"objective": "reg:linear", "max_depth": 3}, 4, 2, 2, True, 0, 7 * 2 * 4),
    "B3": (_reg, (5000, 33, 2), {"objective": "reg:linear", "max_depth": 3}, 3, 2, 2, True, 0, 7 * 2 * 3),
    # (g, h) path with a tail block of 8
    "C": (_binary, (5000, 40, 3), {"objective": "binary:logistic", "scale_pos_weight": 2.0, "max_depth": 3,
                                   "eval_metric": ["logloss", "error", "rmse", "mae"]}, 3, 2, 2, True, 0, 7 * 3 * 3),
    # 156,000 train rows: 10 partial slots at the root (unrolled 8 + 2), multi-slot children
    "D": (_reg, (312000, 5, 4), {"objective": "reg:linear", "max_depth": 3}, 2, 1, 1, True, 0, 26 * 1 * 2),
    # sampling, per-class trees, ORDER-driven scan
    "E": (_multi, (5003, 9, 5), {"objective": "multi:softprob", "num_class": 3, "subsample": 0.6,
                                 "colsample_bytree": 0.7, "colsample_bylevel": 0.6, "max_depth": 5,
                                 "eval_metric": ["merror", "mlogloss"]}, 3, 3, 3, True, 0, 19 * 1 * 3),
    # duplicated / constant / NaN / 3-valued columns
    "F1": (_odd_columns, (3000, 6), {"objective": "reg:linear", "max_depth": 4, "lambda": 3.0, "alpha": 0.5,
                                     "gamma": 0.1, "min_child_weight": 5, "max_delta_step": 0.3}, 3, 2, 2, True, 0,
           11 * 1 * 3),
    "F2": (_odd_columns, (3000, 6), {"objective": "reg:linear", "max_depth": 4}, 3, 2, 2, True, 0, 11 * 1 * 3),
    # degenerate trees
    "G0": (_reg, (2000, 6, 7), {"objective": "reg:linear", "max_depth": 0}, 3, 2, 2, True, 0, 4 * 1 * 3),
    "Gz": (_flat, (2000, 7), {"objective": "reg:linear", "max_depth": 3}, 3, 2, 2, True, 0, 7 * 1 * 3),
    # deep levels, absent nodes, count < 2 nodes; two predict fold-blocks / LDS above 64 KB
    "H10": (_reg, (20000, 6, 8), {"objective": "reg:linear", "max_depth": 10, "min_child_weight": 0}, 5, 1, 1,
            False, 0, 516 * 1 * 5),
    "H12": (_reg, (20000, 6, 8), {"objective": "reg:linear", "max_depth": 12, "min_child_weight": 0}, 2, 1, 1,
            False, 0, 2052 * 1 * 2),
    # predict with R == 0 (rows wider than the LDS budget)
    "I": (_wide, (200, 8200, 9), {"objective": "reg:linear", "max_depth": 2}, 2, 1, 1, False, 0, 5 * 257 * 2),
    # auc: heavy ties (stumps), 6-bit segment ids
    "J3": (_binary, (5000, 6, 10), {"objective": "binary:logistic", "eval_metric": "auc", "max_depth": 1}, 3, 3, 3,
           True, 0, 4 * 1 * 3),
    "J32": (_binary, (5000, 6, 10), {"objective": "binary:logistic", "eval_metric": "auc", "max_depth": 1}, 32, 1, 1,
            True, 0, 4 * 1 * 32),
}

_DATA = {}


def load(name):
    """(x, y, folds, fold_of, parr, objective, num_class, marr, rounds, traced rounds, heavy, seed, grid) of a
    case; datasets are built once per process."""
    maker, args, params, nfold, rounds, traced, heavy, seed, grid = CASES[name]
    dkey = (maker.__name__, args)
    if dkey not in _DATA:
        x, y = maker(*args)
        _DATA[dkey] = (np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32))
    x, y = _DATA[dkey]
    n = x.shape[0]
    folds = kfold(n, nfold, seed=seed)
    fold_of = np.full(n, -1, np.int32)
    for k, (_tr, va) in enumerate(folds):
        fold_of[va] = k
    p, obj = gbdt.resolve_params(params)
    num_class = int(params.get("num_class", 0) or 0)
    metric = params.get("eval_metric") or gbdt.DEFAULT_METRIC[obj]
    metrics = [metric] if isinstance(metric, str) else list(metric)
    parr = np.array([p[k] for k in gbdt.PARAM_ORDER], np.float64)
    marr = np.array([gbdt.METRICS[m] for m in metrics], np.int32)
    return {"x": x, "y": y, "folds": folds, "fold_of": fold_of, "nfold": nfold, "params": params, "parr": parr,
            "obj": obj, "num_class": num_class, "marr": marr, "rounds": rounds, "traced": traced, "heavy": heavy,
            "seed": seed, "grid": grid}
