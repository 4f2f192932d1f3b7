"""MI355X GBDT path: host quantisation (C++), histogram / split / partition /
predict kernels on the GPU (csrc/hip/gbdt_hist.hip: row-major bins, per-node
row segments, smaller-child histograms + subtraction). Used by
:func:`gentun_amd.models.gbdt.cv` when ``device`` is a CUDA/HIP device;
every objective (regression, logistic, binary, multi-class) and every metric
run on the GPU (auc: one radix sort of every fold's margins per round plus a
binary-search rank kernel). The one unsupported case, auc with more than 32
folds, falls back to the CPU engine with a one-time ``RuntimeWarning`` (never
silently)."""

import ctypes
import warnings

import numpy as np

from ..ops import _lib

GPU_OBJECTIVES = (0, 1, 2, 3, 4, 5)      # every objective of models/gbdt.py OBJECTIVES
GPU_METRICS = (0, 1, 2, 3, 4, 5, 6)      # every metric of models/gbdt.py METRICS
AUC, AUC_MAX_FOLDS = 4, 32                # auc sorts 2 segments per fold into a 6-bit segment id


def supported(obj, metrics, nfold=1):
    return (obj in GPU_OBJECTIVES and len(metrics) >= 1 and all(int(m) in GPU_METRICS for m in metrics)
            and not (nfold > AUC_MAX_FOLDS and any(int(m) == AUC for m in metrics)))


def _fn():
    L = _lib.hip()
    f = L.gbdt_cv_hip
    if not getattr(f, "_typed", False):
        c = ctypes
        f.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_int,
                      c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_ulonglong,
                      c.c_longlong, c.c_void_p]
        f.restype = c.c_int
        f._typed = True
    return f


_QCACHE = []      # (x object, shape, bins, nbins, key): every GA candidate reuses its dataset's bins
_KEYS = [0]


def quantize_rm(x):
    """Row-major uint8 bins [n][Fs] (Fs = F rounded up to 4, zero padding) +
    bins per feature + a cache key, computed once per dataset object: the
    device keeps its copy of the bins for that key across candidates."""
    for ent in _QCACHE:
        if ent[0] is x and ent[1] == x.shape:
            return ent[2], ent[3], ent[4]
    xc = np.ascontiguousarray(x, dtype=np.float32)
    n, f = xc.shape
    b = np.zeros((n, f), np.uint8)
    nb = np.zeros(f, np.int32)
    _lib.gbdt().gbdt_quantize(xc.ctypes.data, n, f, b.ctypes.data, nb.ctypes.data)
    fs = (f + 3) // 4 * 4
    if fs != f:
        bp = np.zeros((n, fs), np.uint8)
        bp[:, :f] = b
        b = bp
    _KEYS[0] += 1
    _QCACHE.append((x, x.shape, b, nb, _KEYS[0]))
    while len(_QCACHE) > 2:
        _QCACHE.pop(0)
    return b, nb, _KEYS[0]


_DCACHE = []      # (x object, shape, nbins, key): datasets quantised on the device (G1 kernels)


def _qfn():
    L = _lib.hip()
    f = L.gbdt_quantize_hip
    if not getattr(f, "_typed", False):
        c = ctypes
        f.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_longlong, c.c_void_p]
        f.restype = c.c_int
        L.gbdt_bins_hip_copy.argtypes = [c.c_longlong, c.c_void_p, c.c_size_t]
        L.gbdt_bins_hip_copy.restype = c.c_int
        f._typed = True
    return f


def quantize_device(x, force=False, ident=None):
    """Quantise ``x`` on the GPU (gbdt_quant.hip: transpose, segmented radix
    sort, cuts, binary-search binning; bit-identical to the CPU engine) into
    the device bins cache. Returns ``(nbins, key, Fs)``; cached per dataset
    object (``ident``, default ``x``)."""
    ident = x if ident is None else ident
    if not force:
        for ent in _DCACHE:
            if ent[0] is ident and ent[1] == x.shape:
                return ent[2], ent[3], ent[4]
    xc = np.ascontiguousarray(x, dtype=np.float32)
    n, f = xc.shape
    fs = (f + 3) // 4 * 4
    nb = np.zeros(f, np.int32)
    _KEYS[0] += 1
    key = _KEYS[0]
    rc = _qfn()(xc.ctypes.data, n, f, fs, key, nb.ctypes.data)
    if rc != 0:
        raise RuntimeError("gbdt_quantize_hip failed ({})".format(rc))
    _DCACHE[:] = [e for e in _DCACHE if not (e[0] is ident)]
    _DCACHE.append((ident, x.shape, nb, key, fs))
    while len(_DCACHE) > 2:
        _DCACHE.pop(0)
    return nb, key, fs


def device_bins(x, key, fs):
    """Copy of the device-resident bins of ``key`` (tests / debugging)."""
    out = np.zeros((x.shape[0], fs), np.uint8)
    _qfn()
    rc = _lib.hip().gbdt_bins_hip_copy(key, out.ctypes.data, out.nbytes)
    if rc != 0:
        raise RuntimeError("bins of key {} not resident ({})".format(key, rc))
    return out


_WARNED = set()


def _warn_fallback(obj, marr, nfold):
    key = (int(obj), tuple(int(m) for m in marr), int(nfold))
    if key in _WARNED:
        return
    _WARNED.add(key)
    warnings.warn("gbdt.cv(device='cuda'): eval_metric auc with {} folds (GPU auc supports <= {}); this "
                  "cross-validation runs on the CPU engine (csrc/gbdt/engine.cpp)".format(nfold, AUC_MAX_FOLDS),
                  RuntimeWarning, stacklevel=3)


def cv(x, y, fold_of, nfold, parr, obj, num_class, marr, nrounds, esr, seed, hist, x_key=None):
    if not supported(obj, marr, nfold):
        _warn_fallback(obj, marr, nfold)
        return None
    xk = x if x_key is None else x_key
    fold_of = np.ascontiguousarray(fold_of.astype(np.int32))
    y = np.ascontiguousarray(y.astype(np.float32))
    marr = np.ascontiguousarray(marr.astype(np.int32))
    for attempt in (0, 1):
        nb, key, fs = quantize_device(x, force=attempt > 0, ident=xk)
        kept = _fn()(None, fs, nb.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data,
                     fold_of.ctypes.data, int(nfold), parr.ctypes.data, int(obj), int(num_class), marr.ctypes.data,
                     len(marr), int(nrounds), int(esr), ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF), key,
                     hist.ctypes.data)
        if kept != -7:                       # -7: another dataset evicted the device bins
            return kept
    return kept


# ---- stage trace (csrc/hip/gbdt_hist.hip gbdt_cv_hip_trace; tests/test_gbdt_stages.py) --------------------
TRACE_TAGS = ("GH", "MX", "KEYS", "ORDER", "ROOT", "TREE", "LEAF", "MARGIN", "LNODES", "CHUNKS", "REDS", "COUNTS",
              "HIST", "CAND", "BEST", "SPLITV", "ROWS", "NXT", "MET", "AUC")     # bit i of the mask = TRACE_TAGS[i]
TRACE_HEAVY = ("HIST", "CAND")
LNODE = np.dtype([("start", "<i4"), ("count", "<i4"), ("G", "<i8"), ("H", "<i8"), ("exists", "<i4"),
                  ("built", "<i4"), ("parent", "<i4"), ("pad", "<i4")])
CHUNK = np.dtype([("node", "<i4"), ("start", "<i4"), ("count", "<i4"), ("slot", "<i4")])
RED = np.dtype([("node", "<i4"), ("first", "<i4"), ("nslots", "<i4"), ("pad", "<i4")])
SPLITOUT = np.dtype([("gain", "<f8"), ("GL", "<i8"), ("HL", "<i8"), ("bin", "<i4"), ("order", "<i4")])
NODEBEST = np.dtype([("gain", "<f8"), ("GL", "<i8"), ("HL", "<i8"), ("feature", "<i4"), ("bin", "<i4")])
INT2 = np.dtype([("x", "<i4"), ("y", "<i4")])
TRACE_DTYPES = {"GH": np.dtype("<f4"), "MX": np.dtype("<u4"), "KEYS": np.dtype("<u8"), "ORDER": np.dtype("<i4"),
                "ROOT": np.dtype("<i4"), "TREE": INT2, "LEAF": np.dtype("<f4"), "MARGIN": np.dtype("<f4"),
                "LNODES": LNODE, "CHUNKS": CHUNK, "REDS": RED, "COUNTS": np.dtype("<i4"), "HIST": np.dtype("<i8"),
                "CAND": SPLITOUT, "BEST": NODEBEST, "SPLITV": INT2, "ROWS": np.dtype("<i4"), "NXT": LNODE,
                "MET": np.dtype("<f8"), "AUC": np.dtype("<f8")}
_SINK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                         ctypes.c_void_p, ctypes.c_longlong)


def trace_mask(tags):
    m = 0
    for t in tags:
        m |= 1 << TRACE_TAGS.index(t)
    return m


def trace_layout():
    """Struct sizes and constants of the engine: sizeof LNode, Chunk, Red, SplitOut, NodeBest; GB_R, HB_FC,
    HB_FG, GB_MAXD."""
    f = _lib.hip().gbdt_trace_layout
    f.argtypes = [ctypes.c_void_p]
    f.restype = ctypes.c_int
    out = np.zeros(9, np.int32)
    if f(out.ctypes.data) != 9:
        raise RuntimeError("gbdt_trace_layout: unexpected length")
    return dict(zip(("LNode", "Chunk", "Red", "SplitOut", "NodeBest", "GB_R", "HB_FC", "HB_FG", "GB_MAXD"),
                    (int(v) for v in out)))


def _tfn():
    f = _lib.hip().gbdt_cv_hip_trace
    if not getattr(f, "_typed", False):
        c = ctypes
        f.argtypes = list(_fn().argtypes) + [c.c_int, c.c_uint, _SINK, c.c_void_p]
        f.restype = c.c_int
        f._typed = True
    return f


def cv_trace(x, y, fold_of, nfold, parr, obj, num_class, marr, nrounds, esr, seed, hist, trace_rounds=1,
             tags=None, x_key=None):
    """:func:`cv` through ``gbdt_cv_hip_trace``: returns ``(kept, {(round, cls, depth, tag): ndarray})`` with
    the engine's buffers after every stage of the first ``trace_rounds`` rounds (flat arrays of
    ``TRACE_DTYPES[tag]``; per-tree and per-round blocks have depth -1, the margins before a tree -2).
    ``tags`` defaults to every tag but the heavy ones (``TRACE_HEAVY``)."""
    if not supported(obj, marr, nfold):
        raise ValueError("objective / metrics not supported by the GPU engine")
    tags = [t for t in TRACE_TAGS if t not in TRACE_HEAVY] if tags is None else list(tags)
    blocks = {}

    def sink(_user, rnd, cls, depth, tag, data, nbytes):
        name = TRACE_TAGS[int(tag).bit_length() - 1]
        blocks[(rnd, cls, depth, name)] = np.frombuffer(ctypes.string_at(data, nbytes), dtype=TRACE_DTYPES[name])

    cb = _SINK(sink)
    xk = x if x_key is None else x_key
    fold_of = np.ascontiguousarray(fold_of.astype(np.int32))
    y = np.ascontiguousarray(y.astype(np.float32))
    marr = np.ascontiguousarray(marr.astype(np.int32))
    for attempt in (0, 1):
        blocks.clear()
        nb, key, fs = quantize_device(x, force=attempt > 0, ident=xk)
        kept = _tfn()(None, fs, nb.ctypes.data, x.shape[0], x.shape[1], y.ctypes.data, fold_of.ctypes.data,
                      int(nfold), parr.ctypes.data, int(obj), int(num_class), marr.ctypes.data, len(marr),
                      int(nrounds), int(esr), ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF), key, hist.ctypes.data,
                      int(trace_rounds), trace_mask(tags), cb, None)
        if kept != -7:
            break
    return kept, blocks


# ---- final model: training (gbdt_train_hip), device cuts, forest prediction (csrc/hip/gbdt_predict.hip) -------
PREDICT_CHUNK_ROWS = 1 << 18      # rows per upload of Booster.predict(device='cuda...'); tests lower it
_TREE_SINK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.c_int, ctypes.c_int)
_TREE_STATS_SINK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)


def device_cuts(key, nbins):
    """The quantiser's cuts of the device-resident dataset ``key``: a list of float32 arrays (``gbdt.cuts``)."""
    f = _lib.hip().gbdt_cuts_hip_copy
    f.argtypes = [ctypes.c_longlong, ctypes.c_void_p]
    f.restype = ctypes.c_int
    up = np.zeros((len(nbins), 256), np.float32)
    rc = f(key, up.ctypes.data)
    if rc != 0:
        raise RuntimeError("cuts of key {} not resident ({})".format(key, rc))
    return [up[j, :nbins[j]].copy() for j in range(len(nbins))]


def train(x, y, parr, obj, num_class, marr, nrounds, seed, hist, x_key=None, return_margin=False):
    """``gbdt.train`` on the GPU: the cv loop with one fold and no test rows; every tree's heap tables (nodes,
    leaf values, and the fp64 node statistics cover / gain) come back with the round's metric read-back and are
    compacted here to the Booster's level-order numbering, with thresholds from the device quantiser's cuts.
    Returns ``(Booster arrays, margins or None)``."""
    from .booster import compact_heap_tree
    if not supported(obj, marr, 1):
        raise ValueError("objective / metrics not supported by the GPU engine")
    maxd = trace_layout()["GB_MAXD"]
    if parr[2] > maxd:
        raise ValueError("max_depth {:g} is beyond the GPU engine's deepest tree ({}): train on the CPU "
                         "engine instead".format(parr[2], maxd))
    f = _lib.hip().gbdt_train_hip_stats
    c = ctypes
    f.argtypes = [c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_void_p,
                  c.c_int, c.c_int, c.c_ulonglong, c.c_longlong, c.c_void_p, _TREE_STATS_SINK, c.c_void_p,
                  c.c_void_p]
    f.restype = c.c_int
    xk = x if x_key is None else x_key
    y = np.ascontiguousarray(y.astype(np.float32))
    marr = np.ascontiguousarray(marr.astype(np.int32))
    n, F = x.shape
    K = max(2, int(num_class)) if obj in (4, 5) else 1
    margin32 = np.zeros((n, K), np.float32) if return_margin else None
    trees = []

    def sink(_user, _rnd, _cls, tree_p, leaf_p, cover_p, gain_p, tsz, max_depth):
        txy = np.frombuffer(ctypes.string_at(tree_p, 8 * tsz), dtype="<i4").reshape(tsz, 2)
        leaf = np.frombuffer(ctypes.string_at(leaf_p, 4 * tsz), dtype="<f4")
        cover = np.frombuffer(ctypes.string_at(cover_p, 8 * tsz), dtype="<f8")
        gain = np.frombuffer(ctypes.string_at(gain_p, 8 * tsz), dtype="<f8")
        trees.append(compact_heap_tree(txy, leaf, max_depth, cover, gain))

    cb = _TREE_STATS_SINK(sink)
    for attempt in (0, 1):
        del trees[:]
        nb, key, fs = quantize_device(x, force=attempt > 0, ident=xk)
        rc = f(fs, nb.ctypes.data, n, F, y.ctypes.data, parr.ctypes.data, int(obj), int(num_class), marr.ctypes.data,
               len(marr), int(nrounds), ctypes.c_ulonglong(seed), key, hist.ctypes.data, cb, None,
               None if margin32 is None else margin32.ctypes.data)
        if rc != -7:                         # -7: another dataset evicted the device bins
            break
    if rc < 0:
        raise RuntimeError("gbdt_train_hip failed ({})".format(rc))
    upper = device_cuts(key, nb)
    offsets, feature, split_bin, left, value, threshold, cover, gain = [0], [], [], [], [], [], [], []
    for (tf, tb, tl, tv, tc, tg) in trees:
        cover += tc
        gain += tg
        feature += tf
        split_bin += tb
        left += tl
        value += tv
        threshold += [float(upper[a][b]) if a >= 0 else 0.0 for a, b in zip(tf, tb)]
        offsets.append(len(feature))
    arrays = {"tree_offsets": offsets, "feature": feature, "threshold": threshold, "split_bin": split_bin,
              "left": left, "value": value, "cover": cover, "gain": gain}
    return arrays, (None if margin32 is None else margin32.astype(np.float64))


def predict_rows(n_features):
    """Rows per block that gbdt_predict.hip stages in LDS for this width (0: rows are read from global memory)."""
    f = _lib.hip().gbdt_predict_hip_rows
    f.argtypes = [ctypes.c_int]
    f.restype = ctypes.c_int
    return int(f(int(n_features)))


def predict(bst, x, ntrees, out_margin, out_leaf, timing=None):
    """Margins (fp64 ``[n, K]``) or leaf indices (int32 ``[n, ntrees]``) of ``x`` with the first ``ntrees`` trees
    of ``bst`` on the GPU; bit-identical to the CPU predictor. ``timing``: a list that receives
    ``[kernel ms, ms including transfers]``."""
    f = _lib.hip().gbdt_predict_hip
    c = ctypes
    f.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int,
                  c.c_int, c.c_double, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p]
    f.restype = c.c_int
    ms = np.zeros(2, np.float64)
    rc = f(x.ctypes.data, x.shape[0], x.shape[1], bst.tree_offsets.ctypes.data, bst.feature.ctypes.data,
           bst.threshold.ctypes.data, bst.left.ctypes.data, bst.value.ctypes.data, int(ntrees), bst.K,
           bst.base_margin, int(PREDICT_CHUNK_ROWS), None if out_margin is None else out_margin.ctypes.data,
           None if out_leaf is None else out_leaf.ctypes.data, ms.ctypes.data)
    if rc != 0:
        raise RuntimeError("gbdt_predict_hip failed ({})".format(rc))
    if timing is not None:
        timing[:] = ms.tolist()


# ---- SHAP contributions (csrc/hip/gbdt_shap.hip) ------------------------------------------------------------
def shap_limit():
    """The most unique features on one root-to-leaf path that gbdt_shap.hip handles."""
    f = _lib.hip().gbdt_shap_hip_limit
    f.argtypes = []
    f.restype = ctypes.c_int
    return int(f())


def shap_rows(n_features):
    """Rows per block that gbdt_shap.hip stages in LDS for this width (0: rows are read from global memory)."""
    f = _lib.hip().gbdt_shap_hip_rows
    f.argtypes = [ctypes.c_int]
    f.restype = ctypes.c_int
    return int(f(int(n_features)))


def predict_contribs(bst, x, ntrees, out, timing=None):
    """SHAP contributions (fp64 ``[n, K, F + 1]``, the bias last) of ``x`` with the first ``ntrees`` trees of
    ``bst`` on the GPU; bit-identical to the CPU predictor. ``timing``: a list that receives
    ``[kernel ms, ms including transfers]``."""
    f = _lib.hip().gbdt_shap_hip
    c = ctypes
    f.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                  c.c_void_p, c.c_int, c.c_int, c.c_double, c.c_int, c.c_void_p, c.c_void_p]
    f.restype = c.c_int
    ms = np.zeros(2, np.float64)
    rc = f(x.ctypes.data, x.shape[0], x.shape[1], bst.tree_offsets.ctypes.data, bst.feature.ctypes.data,
           bst.threshold.ctypes.data, bst.left.ctypes.data, bst.value.ctypes.data, bst.cover.ctypes.data, int(ntrees),
           bst.K, bst.base_margin, int(PREDICT_CHUNK_ROWS), out.ctypes.data, ms.ctypes.data)
    if rc == -2:
        raise ValueError("malformed forest: a split out of bounds, or children's covers that are not finite and "
                         ">= 0 with a positive sum")
    if rc == -3:
        raise ValueError("a path of this model has more than {} unique features, the limit of the GPU SHAP "
                         "kernel: use the CPU predictor (device=None)".format(shap_limit()))
    if rc != 0:
        raise RuntimeError("gbdt_shap_hip failed ({})".format(rc))
    if timing is not None:
        timing[:] = ms.tolist()


# ---- SHAP interaction values (csrc/hip/gbdt_shap_inter.hip) -------------------------------------------------
def shap_inter_limit():
    """The most unique features on one root-to-leaf path that gbdt_shap_inter.hip handles."""
    f = _lib.hip().gbdt_shap_inter_hip_limit
    f.argtypes = []
    f.restype = ctypes.c_int
    return int(f())


def shap_inter_plan(n, n_features, num_class=1):
    """``(rows per device chunk, feature-axis split S)`` of a ``predict_interactions`` call with these sizes, or
    ``None`` when one row's output is beyond the kernel's per-buffer bound."""
    f = _lib.hip().gbdt_shap_inter_hip_plan
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    plan = np.zeros(2, np.int32)
    rc = f(int(n), int(n_features), int(num_class), int(PREDICT_CHUNK_ROWS), plan.ctypes.data)
    if rc == -4:
        return None
    if rc != 0:
        raise ValueError("gbdt_shap_inter_hip_plan: bad sizes ({})".format(rc))
    return int(plan[0]), int(plan[1])


def predict_interactions(bst, x, ntrees, out, timing=None, split=0):
    """SHAP interaction values (fp64 ``[n, K, F + 1, F + 1]``) of ``x`` with the first ``ntrees`` trees of ``bst``
    on the GPU; bit-identical to the CPU predictor. ``timing``: a list that receives ``[kernel ms, ms including
    transfers]``. ``split``: the kernel's feature-axis split, 0 = its own choice (the result does not depend on
    it; tools compare the two)."""
    f = _lib.hip().gbdt_shap_inter_hip_split
    c = ctypes
    f.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                  c.c_void_p, c.c_int, c.c_int, c.c_double, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
    f.restype = c.c_int
    ms = np.zeros(2, np.float64)
    rc = f(x.ctypes.data, x.shape[0], x.shape[1], bst.tree_offsets.ctypes.data, bst.feature.ctypes.data,
           bst.threshold.ctypes.data, bst.left.ctypes.data, bst.value.ctypes.data, bst.cover.ctypes.data, int(ntrees),
           bst.K, bst.base_margin, int(PREDICT_CHUNK_ROWS), int(split), out.ctypes.data, ms.ctypes.data)
    if rc == -2:
        raise ValueError("malformed forest: a split out of bounds, or children's covers that are not finite and "
                         ">= 0 with a positive sum")
    if rc == -3:
        raise ValueError("a path of this model has more than {} unique features, the limit of the GPU SHAP "
                         "interaction kernel: use the CPU predictor (device=None)".format(shap_inter_limit()))
    if rc == -4:
        raise ValueError("one row's interaction values ({} x {} x {} doubles) exceed the GPU kernel's 256 MB "
                         "buffers: use the CPU predictor (device=None)".format(bst.K, x.shape[1] + 1, x.shape[1] + 1))
    if rc != 0:
        raise RuntimeError("gbdt_shap_inter_hip failed ({})".format(rc))
    if timing is not None:
        timing[:] = ms.tolist()
