"""``Booster`` -- the fitted GBDT model that :func:`gentun_amd.models.gbdt.train` returns (``xgb.train`` /
``Booster.predict`` next to ``xgb.cv``).

Compact trees only. Tree ``t`` is round ``t // K``, class ``t % K``; its nodes are
``[tree_offsets[t], tree_offsets[t + 1])``, numbered in level order, left to right, existing nodes only:

* ``feature``    int32, -1 = leaf
* ``threshold``  float32: a row goes left when ``not (x[feature] > threshold)``, so NaN goes left as it does
  in training. ``threshold = upper[split_bin]`` of the quantiser, which makes the float rule equal to the
  training rule ``bin <= split_bin`` on every row, so raw rows land in the leaves the training run used.
* ``split_bin``  int32
* ``left``       int32, tree-local; the right child is ``left + 1``
* ``value``      float64 leaf values (eta applied)
* ``cover``      float64, optional: the hessian sum of the rows training had in the node (sampled rows only
  with ``subsample < 1``)
* ``gain``       float64, optional: the loss change of the node's split, 0 for leaves

One predict rule for both predictors (CPU: csrc/gbdt/engine.cpp ``gbdt_predict``; MI355X:
csrc/hip/gbdt_predict.hip): the margin of class ``c`` is the base margin plus the leaf values of that class's
trees, added one tree at a time in tree order in fp64 with one accumulator per (row, class). The two are
therefore bit-identical. Output transforms run on the host from the margins.

``predict(pred_contribs=True)`` are SHAP values under the cover-weighted value function that
csrc/gbdt/shap_tables.h defines; both predictors (``gbdt_predict_contribs``, csrc/hip/gbdt_shap.hip) run that
header's arithmetic in its order and are bit-identical too. ``get_score`` is host-only numpy. A model saved
before the node statistics existed loads with ``cover is None`` and raises where they are needed.

``predict(pred_interactions=True)`` are SHAP interaction values under the same value function
(csrc/gbdt/shap_interactions.h): ``[F + 1, F + 1]`` per row and class, symmetric, every row of the matrix adding
up to the contribution, the bias in the last corner. ``gbdt_predict_interactions`` and
csrc/hip/gbdt_shap_inter.hip are bit-identical as well.
"""

import json

import numpy as np

from ..ops import _lib

FORMAT = "gentun-gbdt/1"
_ARRAYS = (("tree_offsets", np.int64), ("feature", np.int32), ("threshold", np.float32), ("split_bin", np.int32),
           ("left", np.int32), ("value", np.float64))
_STATS = ("cover", "gain")            # optional float64 members, one entry per node
IMPORTANCE_TYPES = ("weight", "gain", "cover", "total_gain", "total_cover")
_OBJ_NAMES = {0: "reg:linear", 1: "reg:logistic", 2: "binary:logistic", 3: "binary:logitraw", 4: "multi:softmax",
              5: "multi:softprob"}


def _is_gpu(device):
    return device is not None and str(device).startswith("cuda")


class Booster(object):

    def __init__(self, tree_offsets, feature, threshold, split_bin, left, value, objective, num_class, base_margin,
                 n_features, params, history, cover=None, gain=None):
        given = dict(tree_offsets=tree_offsets, feature=feature, threshold=threshold, split_bin=split_bin, left=left,
                     value=value)
        for name, dt in _ARRAYS:
            setattr(self, name, np.ascontiguousarray(given[name], dtype=dt).reshape(-1))
        self.objective = int(objective)       # gbdt.OBJECTIVES code
        self.K = int(num_class)               # trees per round: 1, or the classes of a multi: objective
        self.base_margin = float(base_margin)
        self.n_features = int(n_features)
        self.params = dict(params)
        self.history = {k: [float(v) for v in vs] for k, vs in history.items()}
        nn = len(self.feature)
        if (len(self.tree_offsets) < 1 or self.tree_offsets[0] != 0 or self.tree_offsets[-1] != nn
                or np.any(np.diff(self.tree_offsets) < 1) or (len(self.tree_offsets) - 1) % self.K
                or any(len(getattr(self, name)) != nn for name, _ in _ARRAYS[1:])):
            raise ValueError("inconsistent Booster arrays")
        if (cover is None) != (gain is None):
            raise ValueError("cover and gain come together")
        self.cover = self.gain = None
        if cover is not None:
            self.cover = np.ascontiguousarray(cover, dtype=np.float64).reshape(-1)
            self.gain = np.ascontiguousarray(gain, dtype=np.float64).reshape(-1)
            if len(self.cover) != nn or len(self.gain) != nn:
                raise ValueError("inconsistent Booster arrays")

    @property
    def num_trees(self):
        return len(self.tree_offsets) - 1

    @property
    def num_rounds(self):
        return self.num_trees // self.K

    @property
    def objective_name(self):
        return _OBJ_NAMES[self.objective]

    # ---- prediction -------------------------------------------------------------------------------------
    def _rows(self, x):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != self.n_features:
            raise ValueError("x must be 2-D with {} features, got shape {}".format(self.n_features, x.shape))
        return x

    def _used_trees(self, ntree_limit):
        k = int(ntree_limit or 0)
        if k < 0 or k > self.num_rounds:
            raise ValueError("ntree_limit {} is beyond the model's {} rounds".format(k, self.num_rounds))
        return (k if k > 0 else self.num_rounds) * self.K

    def _raw(self, x, ntrees, want_leaf, device, nthreads):
        n = x.shape[0]
        margin = None if want_leaf else np.empty((n, self.K), np.float64)
        leaf = np.empty((n, ntrees), np.int32) if want_leaf else None
        if n == 0:
            return margin, leaf
        if _is_gpu(device):
            from . import gbdt_hip
            gbdt_hip.predict(self, x, ntrees, margin, leaf)
            return margin, leaf
        rc = _lib.gbdt().gbdt_predict(
            x.ctypes.data, n, x.shape[1], self.tree_offsets.ctypes.data, self.feature.ctypes.data,
            self.threshold.ctypes.data, self.left.ctypes.data, self.value.ctypes.data, ntrees, self.K,
            self.base_margin, int(nthreads), None if want_leaf else margin.ctypes.data,
            leaf.ctypes.data if want_leaf else None)
        if rc != 0:
            raise RuntimeError("gbdt_predict failed ({})".format(rc))
        return margin, leaf

    def _need_stats(self):
        if self.cover is None:
            raise ValueError("this model was saved without node statistics (cover / gain): train it again to "
                             "get importances by gain or cover and SHAP contributions")

    def _contribs(self, x, ntrees, device, nthreads):
        self._need_stats()
        n, F = x.shape
        out = np.empty((n, self.K, F + 1), np.float64)
        if n > 0 and _is_gpu(device):
            from . import gbdt_hip
            gbdt_hip.predict_contribs(self, x, ntrees, out)
        elif n > 0:
            rc = _lib.gbdt().gbdt_predict_contribs(
                x.ctypes.data, n, F, self.tree_offsets.ctypes.data, self.feature.ctypes.data,
                self.threshold.ctypes.data, self.left.ctypes.data, self.value.ctypes.data, self.cover.ctypes.data,
                ntrees, self.K, self.base_margin, int(nthreads), out.ctypes.data)
            if rc == -2:
                raise ValueError("malformed forest: a split out of bounds, or children's covers that are not "
                                 "finite and >= 0 with a positive sum")
            if rc == -3:
                raise ValueError("a path with more than 64 unique features")
            if rc != 0:
                raise RuntimeError("gbdt_predict_contribs failed ({})".format(rc))
        return out[:, 0, :] if self.K == 1 else out

    def _interactions(self, x, ntrees, device, nthreads):
        self._need_stats()
        n, F = x.shape
        out = np.empty((n, self.K, F + 1, F + 1), np.float64)
        if n > 0 and _is_gpu(device):
            from . import gbdt_hip
            gbdt_hip.predict_interactions(self, x, ntrees, out)
        elif n > 0:
            rc = _lib.gbdt().gbdt_predict_interactions(
                x.ctypes.data, n, F, self.tree_offsets.ctypes.data, self.feature.ctypes.data,
                self.threshold.ctypes.data, self.left.ctypes.data, self.value.ctypes.data, self.cover.ctypes.data,
                ntrees, self.K, self.base_margin, int(nthreads), out.ctypes.data)
            if rc == -2:
                raise ValueError("malformed forest: a split out of bounds, or children's covers that are not "
                                 "finite and >= 0 with a positive sum")
            if rc == -3:
                raise ValueError("a path with more than 64 unique features")
            if rc != 0:
                raise RuntimeError("gbdt_predict_interactions failed ({})".format(rc))
        return out[:, 0] if self.K == 1 else out

    def predict(self, x, output_margin=False, pred_leaf=False, ntree_limit=0, device=None, nthreads=0,
                pred_contribs=False, pred_interactions=False):
        """float64 predictions with xgboost's shapes: ``[n]`` (regression / binary, and the argmax class of
        ``multi:softmax``) or ``[n, K]`` (``multi:softprob``); ``output_margin`` the raw margins (``[n]`` or
        ``[n, K]``); ``pred_leaf`` int32 ``[n, T]`` tree-local leaf indices; ``pred_contribs`` float64 SHAP
        contributions to the margin, ``[n, F + 1]`` (``[n, K, F + 1]`` for K > 1) with the bias in the last
        column; ``pred_interactions`` float64 SHAP interaction values, ``[n, F + 1, F + 1]``
        (``[n, K, F + 1, F + 1]`` for K > 1), each matrix symmetric with rows that add up to the contributions
        and the bias in the last corner; ``ntree_limit=k`` the first ``k`` rounds. ``device='cuda:0'`` runs the
        walk on the GPU."""
        if pred_contribs and pred_leaf:
            raise ValueError("pred_contribs and pred_leaf exclude each other")
        if pred_interactions and (pred_contribs or pred_leaf):
            raise ValueError("pred_interactions excludes pred_contribs and pred_leaf")
        x = self._rows(x)
        ntrees = self._used_trees(ntree_limit)
        if pred_contribs:
            return self._contribs(x, ntrees, device, nthreads)
        if pred_interactions:
            return self._interactions(x, ntrees, device, nthreads)
        margin, leaf = self._raw(x, ntrees, bool(pred_leaf), device, nthreads)
        if pred_leaf:
            return leaf
        if self.K == 1:
            m = margin[:, 0]
            if output_margin or self.objective in (0, 3):
                return m
            return 1.0 / (1.0 + np.exp(-m))
        if output_margin:
            return margin
        if self.objective == 4:
            return np.argmax(margin, axis=1).astype(np.float64)
        e = np.exp(margin - margin.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    # ---- feature importance (host only) -------------------------------------------------------------------
    def get_score(self, importance_type="weight"):
        """``{"f<j>": value}`` over the features that occur in at least one split (xgboost's naming): ``weight``
        the number of splits on the feature, ``gain`` / ``cover`` the mean and ``total_gain`` / ``total_cover``
        the sum of the splits' gain / cover."""
        if importance_type not in IMPORTANCE_TYPES:
            raise ValueError("importance_type {!r}: expected one of {}".format(importance_type, IMPORTANCE_TYPES))
        inner = self.feature >= 0
        count = np.bincount(self.feature[inner], minlength=self.n_features)
        used = np.flatnonzero(count)
        if importance_type == "weight":
            return {"f{}".format(j): int(count[j]) for j in used}
        self._need_stats()
        stat = self.gain if importance_type.endswith("gain") else self.cover
        total = np.bincount(self.feature[inner], weights=stat[inner], minlength=self.n_features)
        if not importance_type.startswith("total_"):
            total = total / np.maximum(count, 1)
        return {"f{}".format(j): float(total[j]) for j in used}

    def get_fscore(self):
        return self.get_score("weight")

    # ---- file format: one .npz, the arrays plus a JSON header string --------------------------------------
    def save(self, path):
        header = {"format": FORMAT, "objective": self.objective, "K": self.K, "base_margin": self.base_margin,
                  "n_features": self.n_features, "params": self.params, "history": self.history}
        arrays = {name: getattr(self, name) for name, _ in _ARRAYS}
        if self.cover is not None:
            arrays.update({name: getattr(self, name) for name in _STATS})
        with open(path, "wb") as f:
            np.savez(f, header=np.array(json.dumps(header)), **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "header" not in z.files:
                raise ValueError("{}: not a {} file".format(path, FORMAT))
            header = json.loads(str(z["header"][()]))
            if header.get("format") != FORMAT:
                raise ValueError("{}: format {!r}, expected {!r}".format(path, header.get("format"), FORMAT))
            arrays = {name: z[name] for name, _ in _ARRAYS}
            if all(name in z.files for name in _STATS):       # absent in files written before they existed
                arrays.update({name: z[name] for name in _STATS})
        return cls(objective=header["objective"], num_class=header["K"], base_margin=header["base_margin"],
                   n_features=header["n_features"], params=header["params"], history=header["history"], **arrays)


def compact_heap_tree(tree_xy, leaf, max_depth, cover=None, gain=None):
    """One heap-indexed GPU tree (``tree_xy`` int [2^(D+1) - 1][2] = (feature, split bin), feature -1 = leaf;
    ``leaf`` float32 values) -> ``(feature, split_bin, left, value)`` in the Booster's numbering, by a
    level-order walk from the root: entries the walk does not reach (stale heap slots of earlier trees) are
    dropped. With the heap-indexed fp64 tables ``cover`` and ``gain``: ``(..., value, cover, gain)``, the gain
    of a leaf 0."""
    feature, split_bin, left, value = [], [], [], []
    ocover, ogain = [], []
    level, depth = [0], 0
    while level:
        nxt = []
        base = len(feature) + len(level)          # compact index of the next level's first node
        for hid in level:
            f, b = int(tree_xy[hid][0]), int(tree_xy[hid][1])
            value.append(float(leaf[hid]))
            if cover is not None:
                ocover.append(float(cover[hid]))
                ogain.append(float(gain[hid]) if f >= 0 and depth < max_depth else 0.0)
            if f >= 0 and depth < max_depth:
                feature.append(f)
                split_bin.append(b)
                left.append(base + len(nxt))
                nxt += [2 * hid + 1, 2 * hid + 2]
            else:
                feature.append(-1)
                split_bin.append(-1)
                left.append(-1)
        level, depth = nxt, depth + 1
    if cover is not None:
        return feature, split_bin, left, value, ocover, ogain
    return feature, split_bin, left, value
