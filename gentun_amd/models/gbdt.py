"""Python front-end of the native GBDT engine (``xgb.cv`` replacement).

``cv(params, x, y, num_boost_round, nfold, early_stopping_rounds, seed)``
returns a dict of per-round lists ``{'train-<m>-mean', 'train-<m>-std',
'test-<m>-mean', 'test-<m>-std'}`` truncated at the best round when early
stopping is on -- the shape ``xgb.cv`` returns as a DataFrame (reference
call site gentun/models/xgboost_models.py:32-37).

Folds: shuffled, non-stratified k-fold with the given seed (xgboost 0.72
``cv`` defaults: ``shuffle=True``, ``stratified=False``, ``seed=0``).

``train(params, x, y, num_boost_round, seed)`` fits the final model on all rows
and returns a :class:`~gentun_amd.models.booster.Booster` (``xgb.train``);
``cuts(x)`` are the quantiser's per-feature bin bounds.
"""

import ctypes
import math

import numpy as np

from ..ops import _lib
from ..utils.data import kfold

OBJECTIVES = {
    "reg:linear": 0, "reg:squarederror": 0, "reg:logistic": 1, "binary:logistic": 2, "binary:logitraw": 3,
    "multi:softmax": 4, "multi:softprob": 5,
}
METRICS = {"rmse": 0, "mae": 1, "logloss": 2, "error": 3, "auc": 4, "merror": 5, "mlogloss": 6}
DEFAULT_METRIC = {0: "rmse", 1: "rmse", 2: "logloss", 3: "logloss", 4: "merror", 5: "mlogloss"}
PARAM_ORDER = ("eta", "min_child_weight", "max_depth", "gamma", "max_delta_step", "subsample",
               "colsample_bytree", "colsample_bylevel", "lambda", "alpha", "scale_pos_weight", "base_score")
DEFAULTS = {"eta": 0.3, "min_child_weight": 1.0, "max_depth": 6, "gamma": 0.0, "max_delta_step": 0.0,
            "subsample": 1.0, "colsample_bytree": 1.0, "colsample_bylevel": 1.0, "lambda": 1.0, "alpha": 0.0,
            "scale_pos_weight": 1.0, "base_score": 0.5}
ALIASES = {"learning_rate": "eta", "reg_lambda": "lambda", "reg_alpha": "alpha", "min_split_loss": "gamma"}


def _as_arrays(x, y):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float32).reshape(-1))
    if x.ndim != 2 or x.shape[0] != y.shape[0]:
        raise ValueError("x must be 2-D with as many rows as y")
    return x, y


# keys the engine accepts without using: xgboost plumbing / verbosity knobs
IGNORED = {"silent", "verbosity", "nthread", "n_jobs", "seed", "random_state", "tree_method", "eval_metric",
           "objective", "booster", "num_class", "disable_default_eval_metric"}


def resolve_params(params):
    """Engine parameters from an xgboost-style dict. Only ``booster='gbtree'``
    exists here (the reference forwards ``booster`` to xgb.cv,
    gentun/models/xgboost_models.py:16-22): gblinear / dart raise instead of
    silently training trees, and unknown keys raise too."""
    booster = params.get("booster", "gbtree")
    if booster != "gbtree":
        raise ValueError("booster {!r} is not supported: the native engine implements gbtree only".format(booster))
    p = dict(DEFAULTS)
    for k, v in params.items():
        k = ALIASES.get(k, k)
        if k in p:
            p[k] = float(v)
        elif k not in IGNORED:
            raise ValueError("unsupported GBDT parameter {!r}".format(k))
    obj = params.get("objective", "reg:linear")
    if obj not in OBJECTIVES:
        raise ValueError("unsupported objective {!r}".format(obj))
    return p, OBJECTIVES[obj]


def _setup(params, y):
    """(engine params, objective code, num_class, metric names) of a cv / train call."""
    p, obj = resolve_params(params)
    num_class = int(params.get("num_class", 0) or 0)
    if obj in (4, 5) and num_class < 2:
        num_class = int(y.max()) + 1
    metric = params.get("eval_metric") or DEFAULT_METRIC[obj]
    metrics = [metric] if isinstance(metric, str) else list(metric)
    for m in metrics:
        if m not in METRICS:
            raise ValueError("unsupported eval_metric {!r}".format(m))
    return p, obj, num_class, metrics


def cv(params, x, y, num_boost_round=10, nfold=3, early_stopping_rounds=None, seed=0, device=None,
       nthreads=0, folds=None):
    x_key = x                     # dataset identity: the GPU path caches its bins per dataset
    x, y = _as_arrays(x, y)
    p, obj, num_class, metrics = _setup(params, y)
    n = x.shape[0]
    if folds is None:
        folds = kfold(n, nfold, seed=seed)
    fold_of = np.full(n, -1, np.int32)
    for k, (_tr, va) in enumerate(folds):
        fold_of[va] = k
    nrounds = int(num_boost_round)
    hist = np.zeros((nrounds, len(metrics), 4), np.float64)
    parr = np.array([p[k] for k in PARAM_ORDER], np.float64)
    marr = np.array([METRICS[m] for m in metrics], np.int32)
    kept = None
    if device is not None and str(device).startswith("cuda"):
        from . import gbdt_hip
        kept = gbdt_hip.cv(x, y, fold_of, len(folds), parr, obj, num_class, marr, nrounds,
                           early_stopping_rounds or 0, seed, hist, x_key=x_key)
    if kept is None:
        lib = _lib.gbdt()
        kept = lib.gbdt_cv(x.ctypes.data, n, x.shape[1], y.ctypes.data, fold_of.ctypes.data, len(folds),
                           parr.ctypes.data, obj, num_class, marr.ctypes.data, len(metrics), nrounds,
                           int(early_stopping_rounds or 0), ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF),
                           int(nthreads), hist.ctypes.data)
    if kept < 0:
        raise RuntimeError("gbdt_cv failed ({})".format(kept))
    out = {}
    for j, m in enumerate(metrics):
        out["train-{}-mean".format(m)] = hist[:kept, j, 0].tolist()
        out["train-{}-std".format(m)] = hist[:kept, j, 1].tolist()
        out["test-{}-mean".format(m)] = hist[:kept, j, 2].tolist()
        out["test-{}-std".format(m)] = hist[:kept, j, 3].tolist()
    return out


def quantize(x):
    x, _ = _as_arrays(x, np.zeros(len(x)))
    n, f = x.shape
    bins = np.zeros((n, f), np.uint8)
    nb = np.zeros(f, np.int32)
    _lib.gbdt().gbdt_quantize(x.ctypes.data, n, f, bins.ctypes.data, nb.ctypes.data)
    return bins, nb


def cuts(x):
    """Per-feature upper bounds of the quantiser's bins, a list of float32 arrays:
    ``bin = min(searchsorted(cuts[f], v with NaN -> -inf, 'left'), nbins[f] - 1)``."""
    x, _ = _as_arrays(x, np.zeros(len(x)))
    n, f = x.shape
    nb = np.zeros(f, np.int32)
    up = np.zeros((f, 256), np.float32)
    if _lib.gbdt().gbdt_cuts(x.ctypes.data, n, f, nb.ctypes.data, up.ctypes.data) != 0:
        raise RuntimeError("gbdt_cuts failed")
    return [up[j, :nb[j]].copy() for j in range(f)]


def base_margin(obj, base_score):
    """cv_protocol.h base_margin: logit of base_score for the logistic objectives only."""
    if obj not in (1, 2):
        return float(base_score)
    b = min(1 - 1e-7, max(1e-7, float(base_score)))
    return math.log(b / (1 - b))          # libm's log, as std::log in the engines


def train(params, x, y, num_boost_round=10, seed=0, device=None, nthreads=0, return_margin=False):
    """Fit the final model on all rows (``xgb.train``): the engines' cv protocol with one fold and no test rows,
    so ``history['train-<m>']`` equals ``cv(..., folds=[(all rows, [])])['train-<m>-mean']``. Parameters,
    objectives, ``num_class`` inference and metrics are those of :func:`cv`. Returns a
    :class:`~gentun_amd.models.booster.Booster` (with ``return_margin``: also the engine's final margins, fp64
    ``[n, K]`` on the CPU, the fp32 training margins widened on the GPU). ``nthreads`` is accepted for symmetry
    with :func:`cv`: one booster grows on one thread (the quantiser uses every core)."""
    from .booster import Booster
    x_key = x
    x, y = _as_arrays(x, y)
    p, obj, num_class, metrics = _setup(params, y)
    K = max(2, num_class) if obj in (4, 5) else 1
    n, F = x.shape
    nrounds = int(num_boost_round)
    if nrounds < 1:
        raise ValueError("num_boost_round must be >= 1")
    parr = np.array([p[k] for k in PARAM_ORDER], np.float64)
    marr = np.array([METRICS[m] for m in metrics], np.int32)
    hist = np.zeros((nrounds, len(metrics)), np.float64)
    useed = seed & 0xFFFFFFFFFFFFFFFF
    if device is not None and str(device).startswith("cuda"):
        from . import gbdt_hip
        arrays, margin = gbdt_hip.train(x, y, parr, obj, num_class, marr, nrounds, useed, hist, x_key=x_key,
                                        return_margin=return_margin)
    else:
        lib = _lib.gbdt()
        margin = np.zeros((n, K), np.float64) if return_margin else None
        handle = ctypes.c_void_p()
        rc = lib.gbdt_train(x.ctypes.data, n, F, y.ctypes.data, parr.ctypes.data, obj, num_class, marr.ctypes.data,
                            len(metrics), nrounds, ctypes.c_ulonglong(useed), hist.ctypes.data,
                            None if margin is None else margin.ctypes.data, ctypes.byref(handle))
        if rc < 0:
            raise RuntimeError("gbdt_train failed ({})".format(rc))
        try:
            sizes = np.zeros(2, np.int64)
            lib.gbdt_forest_size(handle, sizes.ctypes.data)
            nt, nn = int(sizes[0]), int(sizes[1])
            arrays = {"tree_offsets": np.zeros(nt + 1, np.int64), "feature": np.zeros(nn, np.int32),
                      "threshold": np.zeros(nn, np.float32), "split_bin": np.zeros(nn, np.int32),
                      "left": np.zeros(nn, np.int32), "value": np.zeros(nn, np.float64)}
            lib.gbdt_forest_copy(handle, *[arrays[k].ctypes.data for k in ("tree_offsets", "feature", "threshold",
                                                                           "split_bin", "left", "value")])
            arrays["cover"], arrays["gain"] = np.zeros(nn, np.float64), np.zeros(nn, np.float64)
            lib.gbdt_forest_stats(handle, arrays["cover"].ctypes.data, arrays["gain"].ctypes.data)
        finally:
            lib.gbdt_forest_free(handle)
    history = {"train-{}".format(m): hist[:, j].tolist() for j, m in enumerate(metrics)}
    bst = Booster(objective=obj, num_class=K, base_margin=base_margin(obj, p["base_score"]), n_features=F,
                  params=p, history=history, **arrays)
    return (bst, margin) if return_margin else bst
