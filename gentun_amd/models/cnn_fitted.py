"""``CnnClassifier`` -- a fitted Genetic-CNN model, independent of any training job.

What a search leaves behind for keeping: the decoded architecture, the few configuration values the
forward pass needs and the trained parameters as host fp32 arrays in plain layouts (conv kernels OIHW,
``dense1.w`` rows in NCHW-flatten order -- the torch executor's names and shapes without the group
axis). It is written to / read from one ``.npz`` (``gentun-cnn/1``: a JSON header string plus the
arrays, no pickle) and predicts on

* the CPU, or any torch device with ``backend="torch"``: the stock-torch functional forward of
  :meth:`gentun_amd.models.cnn_engine.TorchFoldJob._forward` in evaluation mode with one group;
* an MI355X: :class:`HipPredictor`, the forward-only launches of the HIP executor's evaluation
  (:meth:`gentun_amd.models.cnn_hip.HipPopJob._build_eval_ops`) over a staging tensor of ``EB`` images,
  ending in ``gt_head_predict`` (csrc/hip/cnn_dense.hip), which writes logits and probabilities instead
  of a loss against a label.

``GeneticCnnModel.fit()`` (models/cnn.py) trains a candidate on every row and returns one of these.
"""

import json

import numpy as np
import torch
import torch.nn.functional as F

from ..ops.cnn_kernels import IG_MAX_STEPS, SG_METHODS, SG_STATS
from .genome import ConvSpec, make_plan

FORMAT = "gentun-cnn/1"
OUTPUTS = ("proba", "logits", "label")
_BN_KINDS = ("gamma", "beta", "running_mean", "running_var")


TTA_MAX_VIEWS = 16           # TTA_MAXV of csrc/hip/cnn_tta.hip


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def tta_views(tta, input_shape):
    """The views ``((dy, dx, flip), ...)`` of a test-time augmentation setting for images of ``input_shape``
    ``(H, W, C)``, as a tuple of int triples (``None`` for ``None``).

    ``tta`` is an explicit sequence of 1 to 16 pairwise distinct views ``(dy, dx, flip)`` (integers with
    ``|dy| < H`` and ``|dx| < W``; ``flip`` a bool or 0 / 1), returned as given, or the shorthand
    ``{"shift": s, "flip": bool}`` of ``TrainConfig.augment`` (``0 <= s < min(H, W)``; either key may be
    absent), which expands, identity first, to: for ``flip`` in (0, 1) if enabled else (0,), for
    ``(dy, dx)`` in ``[(0, 0), (-s, 0), (s, 0), (0, -s), (0, s)]`` if ``s > 0`` else ``[(0, 0)]`` -- 1, 2, 5
    or 10 views. ``ValueError`` on anything else."""
    if tta is None:
        return None
    H, W = int(input_shape[0]), int(input_shape[1])
    if isinstance(tta, dict):
        unknown = sorted(set(tta) - {"shift", "flip"}, key=repr)
        if unknown:
            raise ValueError("tta: unknown keys {}".format(unknown))
        shift, flip = tta.get("shift", 0), tta.get("flip", False)
        if not _is_int(shift) or shift < 0:
            raise ValueError("tta: shift must be a non-negative integer")
        if not isinstance(flip, (bool, np.bool_)):
            raise ValueError("tta: flip must be a bool")
        if shift >= min(H, W):
            raise ValueError("tta: shift {} must be below min(H, W) = {} of the image".format(shift, min(H, W)))
        s = int(shift)
        shifts = [(0, 0), (-s, 0), (s, 0), (0, -s), (0, s)] if s > 0 else [(0, 0)]
        return tuple((dy, dx, f) for f in ((0, 1) if flip else (0,)) for dy, dx in shifts)
    if isinstance(tta, (str, bytes)) or not isinstance(tta, (list, tuple, np.ndarray)):
        raise ValueError("tta must be None, a sequence of (dy, dx, flip) views or a dict with the keys 'shift' "
                         "and / or 'flip'")
    if not 1 <= len(tta) <= TTA_MAX_VIEWS:
        raise ValueError("tta: 1 to {} views, got {}".format(TTA_MAX_VIEWS, len(tta)))
    views = []
    for view in tta:
        if isinstance(view, (str, bytes)) or not isinstance(view, (list, tuple, np.ndarray)) or len(view) != 3:
            raise ValueError("tta: a view is (dy, dx, flip), got {!r}".format(view))
        dy, dx, flip = view
        if not _is_int(dy) or not _is_int(dx):
            raise ValueError("tta: dy and dx must be integers, got {!r}".format(view))
        if abs(int(dy)) >= H or abs(int(dx)) >= W:
            raise ValueError("tta: view {!r} needs |dy| < {} and |dx| < {}".format(view, H, W))
        if not (isinstance(flip, (bool, np.bool_)) or (_is_int(flip) and int(flip) in (0, 1))):
            raise ValueError("tta: flip must be a bool or 0 / 1, got {!r}".format(view))
        views.append((int(dy), int(dx), int(flip)))
    if len(set(views)) != len(views):
        raise ValueError("tta: the views must be pairwise distinct")
    return tuple(views)


def tta_transform(x, dy, dx, flip):
    """View ``(dy, dx, flip)`` of images ``x [n, H, W, C]``: ``out[i, j] = x[i - dy, f(j - dx)]`` inside the
    image, zeros outside it; ``f(u) = W - 1 - u`` where ``flip`` (flip first, then translate) -- training's
    augmentation (csrc/hip/cnn_augment.hip) under a fixed draw. Slicing only: the values are moved, never
    changed."""
    n, H, W, _ = x.shape
    src = x[:, :, ::-1] if flip else x
    out = np.zeros_like(x)
    out[:, max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = \
        src[:, max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)]
    return out


def tta_combine(per_view):
    """The mean over views of ``per_view`` (a sequence of equal-shape arrays) in view order and in their
    dtype: ``acc = p[0]``, ``acc = acc + p[v]``, then ``acc * (1 / V)`` with ``1 / V`` rounded to that dtype
    first -- the add and the multiply rounded separately, as ``gt_head_tta`` does on the device."""
    acc = np.asarray(per_view[0])
    one = acc.dtype.type
    for p in per_view[1:]:
        acc = acc + p
    return (acc * (one(1) / one(len(per_view)))).astype(acc.dtype, copy=False)


MC_MAX_SAMPLES = 64          # MC_MAXT of csrc/hip/cnn_head_mc.hip
MC_OUTPUTS = ("proba", "std", "entropy", "mutual_info", "label")


def mc_check(samples, dropout, seed, batch):
    """The validated ``(samples, dropout, seed, batch)`` of a Monte-Carlo dropout request, before any forward
    runs: ``samples`` an int in ``1..64``, ``dropout`` a float in ``[0, 1)``, ``seed`` an int in ``[0, 2^32)``,
    ``batch`` a positive int (``predict``'s rule). ``ValueError`` on anything else."""
    if not _is_int(samples) or not 1 <= int(samples) <= MC_MAX_SAMPLES:
        raise ValueError("predict_mc: samples must be an integer in [1, {}], got {!r}".format(MC_MAX_SAMPLES, samples))
    if isinstance(dropout, (bool, np.bool_)) or not isinstance(dropout, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(dropout) < 1.0:
        raise ValueError("predict_mc: dropout must be a number in [0, 1), got {!r}".format(dropout))
    if not _is_int(seed) or not 0 <= int(seed) < 2 ** 32:
        raise ValueError("predict_mc: seed must be an integer in [0, 2^32), got {!r}".format(seed))
    if not _is_int(batch) or int(batch) < 1:
        raise ValueError("batch must be a positive integer")
    return int(samples), float(dropout), int(seed), int(batch)


def mc_keep_scale(dropout):
    """``fp32(1) / (fp32(1) - fp32(dropout))``, training's ``keep_scale``."""
    return np.float32(1) / (np.float32(1) - np.float32(dropout))


def mc_entropy(p):
    """``-sum_c p ln p`` over the last axis in the dtype of ``p``, with ``0 ln 0 = 0``."""
    p = np.asarray(p)
    safe = np.where(p > 0, p, p.dtype.type(1))
    return -(p * np.log(safe)).sum(-1, dtype=p.dtype)


def mc_statistics(p, weights):
    """The Monte-Carlo dropout statistics of sample probabilities ``p [k, n, T, C]`` under normalised member
    weights ``[k]``, in the dtype of ``p`` (fp32: what both backends return; the HIP kernel forms the same
    quantities in the same arrangement on the device):

    per member the mean over ``t``, shifted by the first sample (``p_0 + mean_t(p_t - p_0)``: exact when every
    sample is the same), and the two-pass variance around it; ``proba = sum_m w_m mean_m`` in member order;
    ``std = sqrt(sum_m w_m (var_m + (mean_m - proba)^2))``, the population variance over all ``(m, t)`` by the
    law of total variance; ``entropy = H(proba)``; ``expected_entropy = sum_m w_m mean_t H(p_{m,t})``;
    ``mutual_info = max(entropy - expected_entropy, 0)`` by :func:`mc_mutual_info`; ``label`` the first maximum
    of ``proba``."""
    p = np.asarray(p)
    ft = p.dtype.type
    w = np.asarray(weights, p.dtype)
    inv_t = ft(1) / ft(p.shape[2])
    mean = p[:, :, 0] + (p - p[:, :, :1]).sum(2, dtype=p.dtype) * inv_t
    var = ((p - mean[:, :, None]) ** 2).sum(2, dtype=p.dtype) * inv_t
    h = mc_entropy(p)                                                    # [k, n, T]
    hmean = h[:, :, 0] + (h - h[:, :, :1]).sum(2, dtype=p.dtype) * inv_t
    proba = w[0] * mean[0]
    for g in range(1, p.shape[0]):
        proba = proba + w[g] * mean[g]
    tv, eh = np.zeros_like(proba), np.zeros(p.shape[1], p.dtype)
    for g in range(p.shape[0]):
        tv = tv + w[g] * (var[g] + (mean[g] - proba) ** 2)
        eh = eh + w[g] * hmean[g]
    entropy = mc_entropy(proba)
    return {"proba": proba, "std": np.sqrt(tv), "entropy": entropy, "expected_entropy": eh,
            "mutual_info": mc_mutual_info(p, w), "label": np.argmax(proba, axis=1).astype(np.int64)}


def mc_mutual_info(p, weights):
    """``max(H(sum_m w_m mean_t p_{m,t}) - sum_m w_m mean_t H(p_{m,t}), 0)`` of sample probabilities
    ``p [k, n, T, C]``, both entropies taken in fp64 from the samples as they are and the difference rounded once
    to the dtype of ``p``. The difference of the two fp32 entropies would carry their representation error,
    ``2^-23`` of an entropy near 1, which is 2e-5 of a mutual information of 5e-3; errors of the samples
    themselves move both entropies alike and cancel."""
    p64, w = np.asarray(p, np.float64), np.asarray(weights, np.float64)
    proba = np.tensordot(w, p64.mean(2), 1)
    expected = np.tensordot(w, mc_entropy(p64).mean(2), 1)
    return np.maximum(mc_entropy(proba) - expected, 0.0).astype(np.asarray(p).dtype)


def mc_result(stats, samples):
    """What ``predict_mc`` returns from :func:`mc_statistics`-shaped arrays (``samples [k, n, T, C]`` or None)."""
    out = {name: stats[name] for name in MC_OUTPUTS}
    if samples is not None:
        out["samples"] = np.ascontiguousarray(np.transpose(samples, (1, 0, 2, 3)))       # [n, k, T, C]
    return out


def mc_check_hip(classes):
    """The ``ValueError`` of more classes than the HIP head kernels take, before a predictor is built."""
    if classes > 16:
        raise ValueError("HIP head kernel supports at most 16 classes")


OCC_MAX_CELLS = 4096         # OCC_MAX_CELLS of csrc/hip/cnn_occlude.hip
OCC_SCORES = ("proba", "logit")


def occlusion_grid(input_shape, patch, stride=None):
    """``(Gh, Gw)``, the grid of an occlusion request over images of ``input_shape`` ``(H, W, C)``.

    ``patch`` is an int with ``1 <= patch <= min(H, W)``; ``stride`` an int with ``1 <= stride <= patch`` (every
    pixel is covered) or ``None`` for ``patch``. ``Gh = ceil((H - patch) / stride) + 1`` and ``Gw`` likewise, at
    most ``OCC_MAX_CELLS`` cells together. Cell ``(gi, gj)``, of flat index ``gi * Gw + gj``, covers the rows
    ``[gi * stride, min(gi * stride + patch, H))`` and the columns likewise: the last window is clipped, not
    moved. ``ValueError`` on anything else."""
    H, W = int(input_shape[0]), int(input_shape[1])
    if stride is None:
        stride = patch
    if not _is_int(patch) or not _is_int(stride):
        raise ValueError("occlusion: patch and stride must be integers, got {!r} and {!r}".format(patch, stride))
    patch, stride = int(patch), int(stride)
    if not 1 <= patch <= min(H, W):
        raise ValueError("occlusion: patch {} must be in [1, min(H, W) = {}]".format(patch, min(H, W)))
    if not 1 <= stride <= patch:
        raise ValueError("occlusion: stride {} must be in [1, patch = {}]".format(stride, patch))
    Gh, Gw = -(-(H - patch) // stride) + 1, -(-(W - patch) // stride) + 1
    if Gh * Gw > OCC_MAX_CELLS:
        raise ValueError("occlusion: {} x {} cells, at most {}".format(Gh, Gw, OCC_MAX_CELLS))
    return Gh, Gw


def occlusion_fill(fill, channels):
    """``fill`` (a number or ``channels`` numbers, finite) as an fp32 array ``[channels]``."""
    try:
        f = np.asarray(fill, np.float64)
    except (TypeError, ValueError):
        raise ValueError("occlusion: fill must be a number or {} numbers, got {!r}".format(channels, fill))
    if f.ndim == 0:
        f = np.full(channels, float(f))
    if f.shape != (channels,) or not np.isfinite(f).all():
        raise ValueError("occlusion: fill must be a finite number or {} of them, got {!r}".format(channels, fill))
    return f.astype(np.float32)


def occlusion_views(x, patch, stride=None, fill=0.0):
    """The occluded copies ``[n, Gh * Gw, H, W, C]`` of images ``x [n, H, W, C]``: copy ``gi * Gw + gj`` of an
    image has ``fill[c]`` inside cell ``(gi, gj)`` of :func:`occlusion_grid` and the image elsewhere. Slicing
    only; ``fill`` is rounded to the dtype of ``x``."""
    n, H, W, C = x.shape
    Gh, Gw = occlusion_grid((H, W, C), patch, stride)
    stride = int(patch if stride is None else stride)
    f = occlusion_fill(fill, C).astype(x.dtype)
    out = np.repeat(x[:, None], Gh * Gw, axis=1)
    for gi in range(Gh):
        for gj in range(Gw):
            out[:, gi * Gw + gj, gi * stride:gi * stride + int(patch), gj * stride:gj * stride + int(patch)] = f
    return out


def occlusion_targets(target, n, classes, what="occlusion"):
    """``target`` of an occlusion (or Grad-CAM: ``what``) request as ``None`` (the model's own label of every
    image) or int64 ``[n]`` from one class index or ``n`` of them in ``[0, classes)``."""
    if target is None:
        return None
    t = np.asarray(target)
    if t.dtype == np.bool_ or not np.issubdtype(t.dtype, np.integer) or t.ndim > 1:
        raise ValueError("{}: target must be None, a class index or one class index per image".format(what))
    t = np.full(n, int(t), np.int64) if t.ndim == 0 else t.astype(np.int64)
    if t.shape != (n,):
        raise ValueError("{}: {} targets for {} images".format(what, t.shape[0], n))
    if n and (t.min() < 0 or t.max() >= classes):
        raise ValueError("{}: targets must be in [0, {})".format(what, classes))
    return t


CAM_SCORES = ("logit", "proba")
CAM_MAX_PIXELS = 1024        # CAM_MAXPX of csrc/hip/cnn_dense.hip


def cam_shape(plan, input_shape):
    """``(hr, wr)``, the real pixels of the last feature map of ``plan`` (the last stage's pooled map, what the
    dense head flattens) for images of ``input_shape`` ``(H, W, C)``: every stage halves, rounding down --
    8 x 8 for 32 x 32 with two stages, 7 x 7 for 28 x 28."""
    stages = len(plan.kernels_per_layer)
    hr, wr = int(input_shape[0]) >> stages, int(input_shape[1]) >> stages
    if hr < 1 or wr < 1:
        raise ValueError("{} stages leave no pixel of a {} x {} image".format(stages, input_shape[0], input_shape[1]))
    return hr, wr


def _bilinear_matrix(n_in, n_out):
    """fp64 ``[n_out, n_in]``: bilinear interpolation with half-pixel centres, the source coordinate
    ``(o + 0.5) * n_in / n_out - 0.5`` clamped at 0 and the right neighbour at ``n_in - 1``."""
    src = np.maximum((np.arange(n_out) + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = src - i0
    M = np.zeros((n_out, n_in), np.float64)
    np.add.at(M, (np.arange(n_out), i0), 1.0 - lam)
    np.add.at(M, (np.arange(n_out), i1), lam)
    return M


def cam_upsample(maps, size):
    """``maps`` ``[n, hr, wr]`` -> fp32 ``[n, H, W]`` for ``size = (H, W)``: bilinear with half-pixel centres, the
    rule of ``F.interpolate(mode="bilinear", align_corners=False)``, evaluated in fp64 and rounded once. Host
    numpy only; the identity when the sizes match."""
    maps = np.asarray(maps)
    if maps.ndim != 3:
        raise ValueError("cam_upsample: maps must be [n, hr, wr], got shape {}".format(maps.shape))
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError("cam_upsample: size must be positive, got {!r}".format(size))
    if (H, W) == maps.shape[1:]:
        return maps.astype(np.float32)
    My, Mx = _bilinear_matrix(maps.shape[1], H), _bilinear_matrix(maps.shape[2], W)
    return np.einsum("yi,nij,xj->nyx", My, maps.astype(np.float64), Mx).astype(np.float32)


def cam_check(score, relu, upsample, batch):
    """The ``ValueError`` of a bad Grad-CAM option, before any work."""
    if score not in CAM_SCORES:
        raise ValueError("score {!r}: expected one of {}".format(score, CAM_SCORES))
    for name, v in (("relu", relu), ("upsample", upsample)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("gradcam: {} must be a bool, got {!r}".format(name, v))
    if not _is_int(batch) or int(batch) < 1:
        raise ValueError("batch must be a positive integer")


def cam_check_hip(plan, input_shape):
    """The ``ValueError`` of a last feature map with more pixels than ``gt_head_gradcam`` takes, before a
    predictor is built."""
    hr, wr = cam_shape(plan, input_shape)
    if hr * wr > CAM_MAX_PIXELS:
        raise ValueError("gradcam: a last feature map of {} x {} pixels, at most {} on the HIP path".format(
            hr, wr, CAM_MAX_PIXELS))


SAL_METHODS = ("gradient", "gradxinput", "integrated")
SAL_REDUCE = ("absmax", "sum", None)
SAL_MAX_STEPS = IG_MAX_STEPS     # one constant: cnn_kernels checks it against the library's IG_MAXM


SG_DEFAULTS = {"samples": 32, "noise": 0.15, "seed": 0, "stat": "mean"}


def smooth_spec(smooth, method="gradient"):
    """The validated ``(samples, noise fp32, seed, stat)`` of a ``smooth=`` request (missing keys take
    ``SG_DEFAULTS``), or None for ``smooth=None``; ``ValueError`` on anything else."""
    if smooth is None:
        return None
    if not isinstance(smooth, dict) or set(smooth) - set(SG_DEFAULTS):
        raise ValueError("smooth {!r}: expected None or a dict with keys from {}".format(smooth, sorted(SG_DEFAULTS)))
    if method == "integrated":
        raise ValueError("saliency: smooth= does not combine with method='integrated'")
    o = dict(SG_DEFAULTS, **smooth)
    if not _is_int(o["samples"]) or not 1 <= int(o["samples"]) <= SAL_MAX_STEPS:
        raise ValueError("smooth: samples must be an integer in [1, {}], got {!r}".format(SAL_MAX_STEPS, o["samples"]))
    nz = o["noise"]
    if isinstance(nz, (bool, np.bool_)) or not isinstance(nz, (int, float, np.integer, np.floating)) \
            or not np.isfinite(nz) or not 0 <= nz <= 1:
        raise ValueError("smooth: noise must be a finite number in [0, 1], got {!r}".format(nz))
    if not _is_int(o["seed"]) or not 0 <= int(o["seed"]) < 2 ** 32:
        raise ValueError("smooth: seed must be an integer in [0, 2^32), got {!r}".format(o["seed"]))
    if not (isinstance(o["stat"], str) and o["stat"] in SG_STATS):
        raise ValueError("smooth: stat {!r}: expected one of {}".format(o["stat"], SG_STATS))
    return int(o["samples"]), np.float32(nz), int(o["seed"]), o["stat"]


def saliency_check(score, method, steps, baseline, reduce, batch, channels, smooth=None):
    """The validated ``(steps, baseline fp32 [channels])`` of a saliency request; ``ValueError`` on a bad option
    (``smooth`` included: :func:`smooth_spec`), before any work."""
    if score not in CAM_SCORES:
        raise ValueError("score {!r}: expected one of {}".format(score, CAM_SCORES))
    if method not in SAL_METHODS:
        raise ValueError("method {!r}: expected one of {}".format(method, SAL_METHODS))
    if not (reduce is None or (isinstance(reduce, str) and reduce in SAL_REDUCE)):
        raise ValueError("reduce {!r}: expected one of {}".format(reduce, SAL_REDUCE))
    if not _is_int(steps) or not 1 <= int(steps) <= SAL_MAX_STEPS:
        raise ValueError("saliency: steps must be an integer in [1, {}], got {!r}".format(SAL_MAX_STEPS, steps))
    if not _is_int(batch) or int(batch) < 1:
        raise ValueError("batch must be a positive integer")
    smooth_spec(smooth, method)
    try:
        base = occlusion_fill(baseline, channels)
    except ValueError:
        raise ValueError("saliency: baseline must be a finite number or {} of them, got {!r}".format(
            channels, baseline))
    return int(steps), base


def ig_alphas(steps):
    """fp32 ``[steps]``: the midpoints ``(k + 0.5) / steps`` of integrated gradients, rounded once."""
    return ((np.arange(steps, dtype=np.float64) + 0.5) / steps).astype(np.float32)


def ig_point(x, x0, alpha):
    """``x0 + alpha * (x - x0)`` in the dtype of ``x``, every operation rounded separately (``gt_ig_points``)."""
    ft = x.dtype.type
    return x0.astype(x.dtype) + ft(alpha) * (x - x0.astype(x.dtype))


def saliency_finish(grads, x, x0, method):
    """The signed attribution ``[n, H, W, C]`` of the gradients ``grads`` (a list: one array for ``"gradient"`` and
    ``"gradxinput"``, one per interpolation point in ascending order for ``"integrated"``) in their dtype, as
    ``gt_ig_reduce`` forms it: the ordered sum, ``* (1 / m)`` with ``1 / m`` rounded first, ``* (x - x0)``."""
    ft = grads[0].dtype.type
    acc = grads[0]
    for g in grads[1:]:
        acc = acc + g
    if method == "gradient":
        return acc
    xs = x.astype(acc.dtype)
    if method == "gradxinput":
        return xs * acc
    return (xs - x0.astype(acc.dtype)) * (acc * (ft(1) / ft(len(grads))))


def smooth_sigma(x, noise):
    """fp32 ``[n]``: ``fp32(noise) * (max - min)`` of every image of ``x`` ``[n, H, W, C]``, in fp32."""
    xs = x.astype(np.float32, copy=False)
    return np.float32(noise) * (xs.max(axis=(1, 2, 3)) - xs.min(axis=(1, 2, 3)))


def smooth_point(x, sigma, seed, k, n0=0):
    """Sample ``k`` of every image of ``x`` ``[n, H, W, C]`` (images ``n0 ..`` of the call) in the dtype of ``x``:
    ``x + sigma_n * z`` with ``z`` of :func:`gentun_amd.utils.rng.sg_noise``. fp32: ``sigma_n * z`` is rounded to
    fp32, then the sum (``gt_sg_points``); fp64 stays fp64."""
    from ..utils.rng import sg_noise
    n, h, w, c = x.shape
    z = sg_noise(seed, n0 + np.arange(n), [k], h, w, c)[:, 0]
    return x + (sigma.astype(np.float64).reshape(-1, 1, 1, 1) * z).astype(x.dtype)


def smooth_finish(grads, x, method, stat):
    """The signed attribution ``[n, H, W, C]`` of the gradients ``grads`` at the noisy points (a list in ascending
    sample order) in their dtype, as ``gt_sg_reduce`` forms it: the ordered sums ``s1`` of ``g`` and ``s2`` of
    ``g * g``, ``mean = s1 * (1 / S)`` and ``msq = s2 * (1 / S)`` with ``1 / S`` rounded first; ``"mean"``: the mean,
    ``"sq"``: ``msq``, ``"var"``: ``max(msq - mean * mean, 0)``; ``"gradxinput"`` multiplies by the clean ``x``
    (``"mean"``) or by ``x * x``."""
    ft = grads[0].dtype.type
    s1, s2 = grads[0], grads[0] * grads[0]
    for g in grads[1:]:
        s1, s2 = s1 + g, s2 + g * g
    inv = ft(1) / ft(len(grads))
    mean, msq = s1 * inv, s2 * inv
    a = mean if stat == "mean" else msq if stat == "sq" else np.maximum(msq - mean * mean, ft(0))
    if method == "gradient":
        return a
    xs = x.astype(a.dtype)
    return a * xs if stat == "mean" else a * (xs * xs)


def saliency_reduce(a, reduce):
    """The channel reduction of a signed attribution ``[n, H, W, C]``: ``"absmax"`` ``max_c |a|``, ``"sum"`` the
    channels added in order, ``None`` the array itself."""
    if reduce is None:
        return a
    if reduce == "absmax":
        return np.abs(a).max(axis=3)
    acc = a[..., 0]
    for c in range(1, a.shape[3]):
        acc = acc + a[..., c]
    return acc


def saliency_check_hip(classes, steps, method, EB, smooth=None):
    """The ``ValueError`` of what the HIP saliency path does not take, before its state is built."""
    if classes > 16:
        raise ValueError("HIP head kernel supports at most 16 classes")
    if method == "integrated" and steps > EB:
        raise ValueError("saliency: {} steps do not fit {} rows per launch".format(steps, EB))
    if smooth is not None and smooth[0] > EB:
        raise ValueError("saliency: {} smooth samples do not fit {} rows per launch".format(smooth[0], EB))


def occlusion_by_views(scores, x, target, patch, stride, fill, batch, rows=4096):
    """The occlusion map by :func:`occlusion_views`: ``scores(images [k, H, W, C])`` returns ``(score, proba)``,
    fp32 ``[k, classes]`` each, ``batch`` rows per forward -- the score vectors to difference and the
    probabilities whose first maximum is the label. Returns ``(map [n, Gh, Gw], target int64 [n], base fp32 [n])``
    with ``map[r, gi, gj] = score(x[r])[t_r] - score(O_cell(x[r]))[t_r]``, one fp32 subtraction.

    The copies of all images form one sequence of ``n * Gh * Gw`` rows; it is produced a few images at a time
    and scored in pieces of a multiple of ``batch`` rows (about ``rows``), so every forward holds the rows it
    would hold if the whole sequence were given to ``scores`` at once."""
    n = x.shape[0]
    Gh, Gw = occlusion_grid(x.shape[1:], patch, stride)
    Cc = Gh * Gw
    sc, pr = scores(x)
    tgt = np.argmax(pr, axis=1).astype(np.int64) if target is None else target
    base = np.asarray(sc, np.float32)[np.arange(n), tgt]
    piece = int(batch) * max(1, int(rows) // int(batch))
    step = max(1, piece // Cc)
    wanted = np.repeat(tgt, Cc)                          # the class to keep of every row of the sequence
    occluded = np.empty(n * Cc, np.float32)
    pending, done = np.empty((0,) + x.shape[1:], np.float32), 0
    for s in range(0, n, step):
        views = occlusion_views(x[s:s + step], patch, stride, fill)
        pending = np.concatenate([pending, views.reshape((-1,) + x.shape[1:])])
        last = s + step >= n
        while len(pending) >= piece or (last and len(pending)):
            k = min(piece, len(pending))
            sv = np.asarray(scores(pending[:k])[0], np.float32)
            occluded[done:done + k] = sv[np.arange(k), wanted[done:done + k]]
            pending, done = pending[k:], done + k
    return (np.repeat(base, Cc) - occluded).reshape(n, Gh, Gw), tgt, base


RISE_MAX_MASKS = 8192        # RISE_MAX_MASKS of csrc/hip/cnn_rise.hip
RISE_MAX_CELLS = 16          # RISE_MAX_CELLS of csrc/hip/cnn_rise.hip
RISE_KEY = 0x52495345        # hash4 counter of the mask key ("RISE")


def rise_check(input_shape, n, masks, cells, p, seed, batch):
    """The validated ``(masks, cells, p, seed)`` of a RISE request over ``n`` images of ``input_shape``
    ``(H, W, C)``, before any forward runs: ``masks`` an int in ``1..8192``, ``cells`` an int in ``2..16`` and at
    most ``min(H, W)``, ``0 < p < 1``, ``seed`` an int in ``[0, 2^32)``, ``n * masks < 2^31``, ``batch`` a positive
    int. ``ValueError`` on anything else."""
    H, W = int(input_shape[0]), int(input_shape[1])
    if not _is_int(masks) or not 1 <= int(masks) <= RISE_MAX_MASKS:
        raise ValueError("rise: masks must be an integer in [1, {}], got {!r}".format(RISE_MAX_MASKS, masks))
    if not _is_int(cells) or not 2 <= int(cells) <= min(RISE_MAX_CELLS, H, W):
        raise ValueError("rise: cells must be an integer in [2, min({}, H, W) = {}], got {!r}".format(
            RISE_MAX_CELLS, min(RISE_MAX_CELLS, H, W), cells))
    if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating)) \
            or not 0.0 < float(p) < 1.0:
        raise ValueError("rise: p must be a number in (0, 1), got {!r}".format(p))
    if not _is_int(seed) or not 0 <= int(seed) < 2 ** 32:
        raise ValueError("rise: seed must be an integer in [0, 2^32), got {!r}".format(seed))
    if not _is_int(batch) or int(batch) < 1:
        raise ValueError("batch must be a positive integer")
    if int(n) * int(masks) >= 2 ** 31:
        raise ValueError("rise: {} images x {} masks, fewer than 2^31 items".format(n, masks))
    return int(masks), int(cells), float(p), int(seed)


def rise_threshold(p):
    """``uint32(p * 2^32)``: a grid bit is 1 iff its draw is below this."""
    return int(float(p) * 4294967296.0) & 0xFFFFFFFF


def rise_inv(masks, p):
    """``1 / (masks * p)`` in fp64, the map's normalisation."""
    return 1.0 / (float(masks) * float(p))


def rise_masks(input_shape, masks, cells, p, seed, first=0):
    """fp32 ``[masks, H, W]``: the masks ``first .. first + masks - 1`` of a RISE setting, shared by all images;
    mask ``i`` is a function of ``(seed, i, cells, p, H, W)`` only. With ``s = cells``, ``ch = ceil(H / s)``,
    ``cw = ceil(W / s)``, ``thr = uint32(p * 2^32)`` and ``k_i = hash4(seed, i, RISE_KEY, 0)`` (``utils.rng``): the
    grid bit ``g(a, b) = 1`` iff ``hash4(k_i, a, b, 1) < thr`` for ``a, b`` in ``0..s+1``; the offsets
    ``oy = hash4(k_i, 0, 0, 2) mod ch``, ``ox = hash4(k_i, 0, 0, 3) mod cw``; for pixel ``(y, x)``, ``Y = y + oy``,
    ``a = Y // ch``, ``ty = fp32(Y - a * ch) / fp32(ch)`` (``X``, ``b``, ``tx`` likewise) and
    ``M[y, x] = top + ty * (bot - top)`` with ``top = g(a, b) + tx * (g(a, b+1) - g(a, b))`` and ``bot`` the same in
    row ``a + 1`` -- all in fp32, every product and sum rounded separately (``gt_rise_views`` / ``gt_rise_masks``
    are the device twins, tests/rise_ref.py the loop oracle)."""
    from ..utils.rng import hash4
    H, W = int(input_shape[0]), int(input_shape[1])
    s = int(cells)
    ch, cw = -(-H // s), -(-W // s)
    f32 = np.float32
    i = np.arange(int(first), int(first) + int(masks), dtype=np.uint64)
    key = hash4(int(seed), i, RISE_KEY, 0)
    ab = np.arange(s + 2, dtype=np.uint64)
    g = (hash4(key[:, None, None], ab[None, :, None], ab[None, None, :], 1)
         < np.uint64(rise_threshold(p))).astype(f32)                               # [masks, s + 2, s + 2]
    oy = (hash4(key, 0, 0, 2) % np.uint64(ch)).astype(np.int64)
    ox = (hash4(key, 0, 0, 3) % np.uint64(cw)).astype(np.int64)
    Y = np.arange(H)[None, :] + oy[:, None]                                        # [masks, H]
    X = np.arange(W)[None, :] + ox[:, None]                                        # [masks, W]
    a, b = Y // ch, X // cw
    ty = ((Y - a * ch).astype(f32) / f32(ch))[:, :, None]
    tx = ((X - b * cw).astype(f32) / f32(cw))[:, None, :]
    m = np.arange(len(i))[:, None, None]
    a, b = a[:, :, None], b[:, None, :]
    g00, g01, g10, g11 = g[m, a, b], g[m, a, b + 1], g[m, a + 1, b], g[m, a + 1, b + 1]
    top = g00 + tx * (g01 - g00)
    bot = g10 + tx * (g11 - g10)
    return (top + ty * (bot - top)).astype(f32, copy=False)


def rise_views(x, M, fill):
    """The masked copies ``[n, k, H, W, C]`` of fp32 images ``x [n, H, W, C]`` under masks ``M [k, H, W]``:
    ``fill[c] + M[y, x] * (img[y, x, c] - fill[c])`` in fp32, the difference, the product and the sum rounded
    separately."""
    f = occlusion_fill(fill, x.shape[3])
    x = np.asarray(x, np.float32)
    return f + M[None, :, :, :, None] * (x[:, None] - f)


def rise_by_views(scores, x, target, masks, cells, p, seed, fill, batch, rows=4096):
    """The RISE map by :func:`rise_masks` and :func:`rise_views`: ``scores(images [k, H, W, C])`` returns
    ``(score, proba)``, fp32 ``[k, classes]`` each, ``batch`` rows per forward (as in :func:`occlusion_by_views`).
    Returns ``(map fp32 [n, H, W], target int64 [n], base fp32 [n])`` with
    ``map[r] = (sum_i s_{r,i} M_i) * inv`` accumulated in fp64 and rounded once, ``s_{r,i}`` the score of the
    target of ``V_i(x[r])`` and ``inv = 1 / (masks * p)``.

    The copies of all images form one sequence of ``n * masks`` rows, item ``r * masks + i``; it is produced in
    pieces of a multiple of ``batch`` rows (about ``rows``), so every forward holds the rows it would hold if the
    whole sequence were given to ``scores`` at once."""
    n, H, W = x.shape[0], x.shape[1], x.shape[2]
    sc, pr = scores(x)
    tgt = np.argmax(pr, axis=1).astype(np.int64) if target is None else target
    base = np.asarray(sc, np.float32)[np.arange(n), tgt]
    piece = int(batch) * max(1, int(rows) // int(batch))
    acc = np.zeros((n, H * W), np.float64)
    cache = {}                                           # first mask of a block of masks -> [<= piece, H, W]

    def block(i0):
        if i0 not in cache:
            cache.clear()
            cache[i0] = rise_masks(x.shape[1:], min(piece, masks - i0), cells, p, seed, first=i0)
        return cache[i0]
    for w0 in range(0, n * masks, piece):
        k = min(piece, n * masks - w0)
        views = np.empty((k,) + x.shape[1:], np.float32)
        used, j = [], 0
        while j < k:                                     # runs of one image inside one block of masks
            r, i = divmod(w0 + j, masks)
            i0 = i // piece * piece
            cnt = min(k - j, masks - i, i0 + piece - i)
            Mb = block(i0)[i - i0:i - i0 + cnt]
            views[j:j + cnt] = rise_views(x[r:r + 1], Mb, fill)[0]
            used.append((r, j, Mb))
            j += cnt
        sv = np.asarray(scores(views)[0], np.float32)
        for r, j, Mb in used:
            s = sv[j:j + len(Mb), tgt[r]].astype(np.float64)
            M64 = Mb.reshape(len(Mb), -1).astype(np.float64)
            for t in range(len(Mb)):                     # ascending i; every product is exact in fp64
                acc[r] += s[t] * M64[t]
    return (acc * rise_inv(masks, p)).astype(np.float32).reshape(n, H, W), tgt, base


def rise_check_hip(classes):
    """The ``ValueError`` of more classes than the HIP head kernels take, before a predictor is built."""
    if classes > 16:
        raise ValueError("HIP head kernel supports at most 16 classes")


NN_METRICS = ("l2", "cosine")
NN_MAX_K = 16                # NN_MAXK of csrc/hip/cnn_neighbors.hip


def embed_check(batch, backend):
    """The validated ``batch`` of an ``embed`` / ``neighbors`` request; ``ValueError`` on a bad ``batch`` or
    ``backend``."""
    if not _is_int(batch) or int(batch) < 1:
        raise ValueError("batch must be a positive integer")
    if backend not in (None, "hip", "torch"):
        raise ValueError("unknown backend {!r}".format(backend))
    return int(batch)


def neighbors_check(k, metric, bank, input_shape, D, batch, backend):
    """The validated ``(k, metric, bank, images, batch)`` of a ``neighbors`` request, before any forward runs.
    ``bank`` comes back as contiguous fp32, ``images`` says whether it holds images ``[N, H, W, C]`` (to embed) or
    embeddings ``[N, D]``. ``ValueError`` on: ``k`` not an int in ``1..16`` or above ``N``; a metric outside
    ``NN_METRICS``; a bank that is neither form, whose ``D`` is not the model's or whose embeddings are not
    finite; a bad ``batch`` or ``backend``."""
    if not _is_int(k) or not 1 <= int(k) <= NN_MAX_K:
        raise ValueError("neighbors: k must be an integer in [1, {}], got {!r}".format(NN_MAX_K, k))
    if metric not in NN_METRICS:
        raise ValueError("neighbors: metric {!r}: expected one of {}".format(metric, NN_METRICS))
    batch = embed_check(batch, backend)
    bank = np.asarray(bank)
    images = bank.ndim == 4
    if images:
        if tuple(bank.shape[1:]) != tuple(input_shape):
            raise ValueError("neighbors: a bank of images must be [N, {}, {}, {}], got shape {}".format(
                *(tuple(input_shape) + (bank.shape,))))
    elif bank.ndim != 2:
        raise ValueError("neighbors: bank must be images [N, H, W, C] or embeddings [N, D], got shape {}".format(
            bank.shape))
    elif bank.shape[1] != D:
        raise ValueError("neighbors: the bank has {} features, the model's embedding has {}".format(bank.shape[1], D))
    if int(k) > bank.shape[0]:
        raise ValueError("neighbors: k = {} exceeds the bank's {} rows".format(k, bank.shape[0]))
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    if not images and not np.isfinite(bank).all():
        raise ValueError("neighbors: the bank's embeddings must be finite")
    return int(k), metric, bank, images, batch


def neighbors_search(q, b, k, metric, rows=1 << 22):
    """``(index int64 [n, k], distance fp32 [n, k])`` of fp32 embeddings ``q [n, D]`` against ``b [N, D]``, the
    definition every backend is held to: ``q.b``, ``|q|^2`` and ``|b|^2`` are fp64 sums over the features in
    feature order (every product of two fp32 values is exact in fp64), the distance

    * ``"l2"``: ``max(|q|^2 + |b|^2 - 2 q.b, 0)``
    * ``"cosine"``: ``1 - q.b / (sqrt(|q|^2) sqrt(|b|^2))``, 1 when either norm is 0

    is formed in fp64 and rounded to fp32 once, and the neighbours are the first ``k`` of a stable sort of the
    fp32 distances: ascending ``(distance, bank index)``. The one summation order makes a query that is a bank row
    its own neighbour at l2 distance exactly 0. ``rows``: (query, bank) pairs held at a time."""
    q64, b64 = np.asarray(q, np.float64), np.asarray(b, np.float64)
    n, N, D = q64.shape[0], b64.shape[0], q64.shape[1]
    bb = np.zeros(N)
    for d in range(D):
        bb += b64[:, d] * b64[:, d]
    idx, dist = np.empty((n, k), np.int64), np.empty((n, k), np.float32)
    step = max(1, rows // max(N, 1))
    for s in range(0, n, step):
        qs = q64[s:s + step]
        dot, qq = np.zeros((qs.shape[0], N)), np.zeros(qs.shape[0])
        for d in range(D):
            dot += np.multiply.outer(qs[:, d], b64[:, d])
            qq += qs[:, d] * qs[:, d]
        if metric == "l2":
            dd = np.maximum(qq[:, None] + bb[None, :] - 2.0 * dot, 0.0)
        else:
            den = np.sqrt(qq)[:, None] * np.sqrt(bb)[None, :]
            dd = np.where(den > 0.0, 1.0 - dot / np.where(den > 0.0, den, 1.0), 1.0)
        d32 = dd.astype(np.float32)
        order = np.argsort(d32, axis=1, kind="stable")[:, :k]
        idx[s:s + step] = order
        dist[s:s + step] = np.take_along_axis(d32, order, axis=1)
    return idx, dist


def _nn_backend(device, backend):
    dev = torch.device("cpu" if device is None else device)
    return dev, backend or ("hip" if dev.type == "cuda" else "torch")


def embed_torch(members, x, dev, batch, dtype=torch.float32):
    """The members' stock-torch embeddings side by side in member order, ``[n, len(members) * dense_units]``."""
    return np.concatenate([m._torch_embed(x, dev, batch, dtype) for m in members], axis=1)


def embed_run(model, members, x, device, batch, backend):
    """``embed`` of a classifier (``members = [model]``) or an ensemble."""
    batch = embed_check(batch, backend)
    x = members[0]._check_x(x)
    dev, backend = _nn_backend(device, backend)
    if backend == "hip":
        pred = model.hip_predictor(dev, batch)
        return neighbor_state(pred, len(members)).embed(pred, x)
    return embed_torch(members, x, dev, batch)


def neighbors_run(model, members, x, bank, k, metric, device, batch, backend):
    """``neighbors`` of a classifier (``members = [model]``) or an ensemble."""
    first = members[0]
    k, metric, bank, images, batch = neighbors_check(k, metric, bank, first.input_shape,
                                                     len(members) * first.dense_units, batch, backend)
    x = first._check_x(x)
    dev, backend = _nn_backend(device, backend)
    if backend == "hip":
        pred = model.hip_predictor(dev, batch)
        return neighbor_state(pred, len(members)).run(pred, x, bank, images, k, metric)
    q = embed_torch(members, x, dev, batch)
    return neighbors_search(q, embed_torch(members, bank, dev, batch) if images else bank, k, metric)


GAUSS_KEYS = ("count", "mean", "cov", "whiten", "wmean", "shrink")


def gaussian_check(labels, shrink, bank, input_shape, classes, D, batch, backend):
    """The validated ``(labels int64 [N], C, shrink, bank, images, batch)`` of a ``gaussian_fit`` request, before
    any forward runs. ``labels=None`` is one Gaussian for the whole bank (``C = 1``, all-zero labels); otherwise
    ``C = classes`` and ``labels`` is an int array ``[N]`` in ``0..classes-1`` or one-hot ``[N, classes]``.
    ``ValueError`` on labels of another form, length or range; ``shrink`` outside ``[0, 1]``; a bank that is
    neither images of the model's shape nor finite embeddings ``[N, D]``, or that is empty; a bad ``batch`` or
    ``backend``."""
    batch = embed_check(batch, backend)
    if isinstance(shrink, bool) or not isinstance(shrink, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(shrink) <= 1.0:
        raise ValueError("gaussian_fit: shrink must be a number in [0, 1], got {!r}".format(shrink))
    bank = np.asarray(bank)
    images = bank.ndim == 4
    if images:
        if tuple(bank.shape[1:]) != tuple(input_shape):
            raise ValueError("gaussian_fit: a bank of images must be [N, {}, {}, {}], got shape {}".format(
                *(tuple(input_shape) + (bank.shape,))))
    elif bank.ndim != 2:
        raise ValueError("gaussian_fit: bank must be images [N, H, W, C] or embeddings [N, D], got shape {}".format(
            bank.shape))
    elif bank.shape[1] != D:
        raise ValueError("gaussian_fit: the bank has {} features, the model's embedding has {}".format(
            bank.shape[1], D))
    N = bank.shape[0]
    if N < 1:
        raise ValueError("gaussian_fit: the bank is empty")
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    if not images and not np.isfinite(bank).all():
        raise ValueError("gaussian_fit: the bank's embeddings must be finite")
    if labels is None:
        return np.zeros(N, np.int64), 1, float(shrink), bank, images, batch
    y = np.asarray(labels)
    if y.ndim == 2 and y.shape == (N, classes):
        y = np.argmax(y, axis=1)
    elif y.ndim != 1 or y.shape[0] != N or y.dtype.kind not in "iu":
        raise ValueError("gaussian_fit: labels must be {0} integers or one-hot [{0}, {1}], got shape {2} of {3}"
                         .format(N, classes, y.shape, y.dtype))
    y = y.astype(np.int64)
    if y.min() < 0 or y.max() >= classes:
        raise ValueError("gaussian_fit: labels must lie in [0, {}]".format(classes - 1))
    return y, int(classes), float(shrink), bank, images, batch


def mahalanobis_check(stats, G, U, batch, backend):
    """The validated ``(stats as arrays, C, batch)`` of a ``mahalanobis`` request, before any forward runs:
    ``ValueError`` on a ``stats`` that lacks a key of ``GAUSS_KEYS``, whose shapes disagree with each other or
    with the model's ``G`` members and ``U`` units, or whose ``whiten`` / ``wmean`` are not finite; a bad
    ``batch`` or ``backend``."""
    batch = embed_check(batch, backend)
    try:
        st = {k: np.asarray(stats[k]) for k in GAUSS_KEYS}
    except (KeyError, TypeError, IndexError):
        raise ValueError("mahalanobis: stats must be the dict gaussian_fit returns (keys {})".format(GAUSS_KEYS))
    C = st["count"].shape[0] if st["count"].ndim == 1 else 0
    want = {"mean": (G, C, U), "cov": (G, U, U), "whiten": (G, U, U), "wmean": (G, C, U)}
    if C < 1 or any(st[k].shape != v for k, v in want.items()):
        raise ValueError("mahalanobis: stats are not this model's ({} member(s) of {} units): shapes {}".format(
            G, U, {k: st[k].shape for k in GAUSS_KEYS}))
    if not (np.isfinite(st["whiten"]).all() and np.isfinite(st["wmean"]).all()):
        raise ValueError("mahalanobis: stats hold values that are not finite")
    st["whiten"] = np.ascontiguousarray(st["whiten"], np.float32)
    st["wmean"] = np.ascontiguousarray(st["wmean"], np.float32)
    return st, C, batch


def gaussian_moments(f, labels, C):
    """``(count int64 [C], mean fp32 [C, U], cov fp64 [U, U])`` of fp32 features ``f [N, U]``, the definition:
    ``mean_c`` is the fp64 sum of the class's rows in row order over its count, rounded to fp32 (zeros for an
    empty class); ``c_r = fp32(f_r - mean_{y_r})``, one fp32 subtraction per element; ``cov`` is the fp64 sum of
    ``c_r c_r^T`` in row order (every product of two fp32 values is exact in fp64) divided by ``N``: symmetric to
    the bit. One pass over the rows, one ``U x U`` update each: minutes for 60,000 x 500."""
    f = np.asarray(f, np.float32)
    N, U = f.shape
    count = np.bincount(labels, minlength=C).astype(np.int64)
    sums = np.zeros((C, U))
    np.add.at(sums, labels, f.astype(np.float64))            # unbuffered: row order
    mean = (sums / np.maximum(count, 1)[:, None]).astype(np.float32)
    c = (f - mean[labels]).astype(np.float64)
    acc = np.zeros((U, U))
    for r in range(N):
        acc += np.multiply.outer(c[r], c[r])
    return count, mean, acc / N


def gaussian_whiten(cov, mean, shrink):
    """``(W fp32 [U, U], t fp32 [C, U])`` of one member: ``shrunk = (1 - shrink) cov + shrink (trace(cov) / U) I``,
    ``shrunk = L L^T`` by fp64 Cholesky, ``W = fp32(L^-T)`` and ``t_c = fp32(W^T mean_c)`` in fp64 from the fp32
    ``W``. ``ValueError`` naming ``shrink`` when ``shrunk`` is not positive definite."""
    U = cov.shape[0]
    shrunk = (1.0 - shrink) * cov + shrink * (np.trace(cov) / U) * np.eye(U)
    try:
        Li = np.linalg.inv(np.linalg.cholesky(shrunk))
        if not np.isfinite(Li).all():
            raise np.linalg.LinAlgError("not finite")
    except np.linalg.LinAlgError:
        raise ValueError("gaussian_fit: the covariance is singular at shrink={!r} (dead units or too few rows): "
                         "pass a larger shrink".format(shrink))
    W = np.ascontiguousarray(Li.T).astype(np.float32)
    return W, (mean.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)


def gaussian_stats(count, mean, cov, shrink):
    """The ``stats`` dict of ``gaussian_fit`` from the members' moments ``mean [G, C, U]``, ``cov [G, U, U]``."""
    wt = [gaussian_whiten(cov[g], mean[g], shrink) for g in range(len(cov))]
    return {"count": count, "mean": mean, "cov": cov, "whiten": np.stack([w for w, _ in wt]),
            "wmean": np.stack([t for _, t in wt]), "shrink": np.float64(shrink)}


def mahalanobis_distance(f, W, t, count, rows=4096):
    """fp32 ``[n, C]`` squared distances of fp32 features ``f [n, U]`` of one member, the definition:
    ``z = f W`` and ``d_c = sum_j (z_j - t_cj)^2`` in fp64 over the fp32 values, rounded to fp32 once; ``+inf``
    for a class without rows."""
    W64, t64 = np.asarray(W, np.float64), np.asarray(t, np.float64)
    out = np.empty((f.shape[0], t64.shape[0]), np.float32)
    for s in range(0, f.shape[0], rows):
        z = np.asarray(f[s:s + rows], np.float64) @ W64
        out[s:s + rows] = ((z[:, None, :] - t64[None]) ** 2).sum(-1)
    out[:, np.asarray(count) == 0] = np.inf
    return out


def member_mean(d, weights):
    """The weighted mean of the members' distances ``d [G, n, C]`` in member order with the rounding of the
    ensemble's other means (``acc = w[0] * d[0]``, then ``acc = acc + w[g] * d[g]``, fp32)."""
    w = np.asarray(weights, np.float32)
    acc = w[0] * d[0]
    for g in range(1, len(d)):
        acc = acc + w[g] * d[g]
    return acc.astype(np.float32)


def gaussian_fit_run(model, members, bank, labels, shrink, device, batch, backend):
    """``gaussian_fit`` of a classifier (``members = [model]``) or an ensemble."""
    first, G, U = members[0], len(members), members[0].dense_units
    labels, C, shrink, bank, images, batch = gaussian_check(labels, shrink, bank, first.input_shape, first.classes,
                                                            G * U, batch, backend)
    dev, backend = _nn_backend(device, backend)
    if backend == "hip":
        gaussian_check_hip(C)
        pred = model.hip_predictor(dev, batch)
        count, mean, cov = gaussian_state(pred, G).fit(pred, bank, images, labels, C)
    else:
        f = embed_torch(members, bank, dev, batch) if images else bank
        mom = [gaussian_moments(f[:, g * U:(g + 1) * U], labels, C) for g in range(G)]
        count, mean, cov = mom[0][0], np.stack([m[1] for m in mom]), np.stack([m[2] for m in mom])
    return gaussian_stats(count, mean, cov, shrink)


def mahalanobis_run(model, members, weights, x, stats, device, batch, backend):
    """``mahalanobis`` of a classifier (``members = [model]``, weight 1) or an ensemble."""
    first, G, U = members[0], len(members), members[0].dense_units
    st, C, batch = mahalanobis_check(stats, G, U, batch, backend)
    x = first._check_x(x)
    dev, backend = _nn_backend(device, backend)
    if backend == "hip":
        gaussian_check_hip(C)
        pred = model.hip_predictor(dev, batch)
        d = gaussian_state(pred, G).distance(pred, x, st, C)
    else:
        f = embed_torch(members, x, dev, batch)
        d = np.stack([mahalanobis_distance(f[:, g * U:(g + 1) * U], st["whiten"][g], st["wmean"][g], st["count"])
                      for g in range(G)])
    return member_mean(d, weights)


def predict_batch(batch):
    """Rows per launch of the HIP predictor: ``batch`` rounded up to a multiple of 32, at least 32 and
    at most 256 (the cap of ``HipPopJob.eval_batch``)."""
    return max(32, min(256, (int(batch) + 31) // 32 * 32))


class CnnClassifier(object):

    def __init__(self, genes, nodes, input_shape, kernels_per_layer, kernel_sizes, dense_units, classes, params,
                 batch_norm=False, bn_eps=1e-3, loss="bce_compat", dtype="fp32", metrics=None):
        self.genes = dict(genes)
        self.nodes = tuple(int(v) for v in nodes)
        self.input_shape = tuple(int(v) for v in input_shape)
        self.kernels_per_layer = tuple(int(v) for v in kernels_per_layer)
        self.kernel_sizes = tuple(tuple(int(v) for v in k) for k in kernel_sizes)
        self.dense_units = int(dense_units)
        self.classes = int(classes)
        self.batch_norm = bool(batch_norm)
        self.bn_eps = float(bn_eps)
        self.loss = loss
        self.dtype = dtype
        self.metrics = dict(metrics or {})
        self.plan = make_plan(self.genes, self.nodes, self.input_shape, self.kernels_per_layer, self.kernel_sizes,
                              self.dense_units, self.classes)
        self.params = {}
        for name, shape in self.param_shapes():
            if name not in params:
                raise ValueError("missing parameter {!r}".format(name))
            a = np.ascontiguousarray(params[name], dtype=np.float32)
            if a.shape != shape:
                raise ValueError("parameter {!r} has shape {}, expected {}".format(name, a.shape, shape))
            self.params[name] = a
        self._torch_params = {}      # (device, dtype) -> {name: tensor}
        self._predictors = {}        # (device, EB) -> HipPredictor

    # ------------------------------------------------------------ structure
    def param_shapes(self):
        """``[(name, shape)]`` in the torch executor's order (cnn_engine.TorchFoldJob) without the group axis."""
        p, out = self.plan, []
        for st in p.convs():
            out.append((st.name + ".w", (st.cout, st.cin, st.k[0], st.k[1])))
            out.append((st.name + ".b", (st.cout,)))
            if self.batch_norm:
                out += [(st.name + "." + kind, (st.cout,)) for kind in _BN_KINDS]
        out.append(("dense1.w", (p.flatten, p.dense_units)))
        out.append(("dense1.b", (p.dense_units,)))
        out.append(("dense2.w", (p.dense_units, p.classes)))
        out.append(("dense2.b", (p.classes,)))
        return out

    def header(self):
        return {"format": FORMAT, "genes": self.genes, "nodes": list(self.nodes),
                "input_shape": list(self.input_shape), "kernels_per_layer": list(self.kernels_per_layer),
                "kernel_sizes": [list(k) for k in self.kernel_sizes], "dense_units": self.dense_units,
                "classes": self.classes, "batch_norm": self.batch_norm, "bn_eps": self.bn_eps, "loss": self.loss,
                "dtype": self.dtype, "metrics": self.metrics}

    # ------------------------------------------------------------ export / import
    @classmethod
    def from_job(cls, job, group=0, metrics=None):
        """The parameters of group ``group`` of a live job (either executor) as a classifier."""
        plan, cfg = job.members[job.gmember[group]][0], job.cfg
        params = _export_hip(job, plan, group) if hasattr(job, "stage_cp") else _export_torch(job, group)
        return cls(plan.genes, plan.nodes, plan.input_shape, plan.kernels_per_layer, plan.kernel_sizes,
                   plan.dense_units, plan.classes, params, batch_norm=cfg.batch_norm, bn_eps=cfg.bn_eps,
                   loss=cfg.loss, dtype=cfg.dtype, metrics=metrics)

    def load_into(self, job, group=0):
        """Write the parameters into group ``group`` of a job of this architecture (the inverse of
        :meth:`from_job`). A HIP job gets the real extent of its padded masters, every padding element
        zero, and its derived weight planes rebuilt."""
        plan = job.members[job.gmember[group]][0]
        if plan.key() != self.plan.key() or bool(job.cfg.batch_norm) != self.batch_norm:
            raise ValueError("the job trains another architecture than this classifier's")
        if hasattr(job, "stage_cp"):
            _import_hip(self, job, group)
        else:
            _import_torch(self, job, group)

    # ------------------------------------------------------------ file format
    def save(self, path):
        """One ``.npz``: the JSON header string plus one array per parameter."""
        with open(path, "wb") as f:
            np.savez(f, header=np.array(json.dumps(self.header())), **self.params)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "header" not in z.files:
                raise ValueError("{}: not a {} file".format(path, FORMAT))
            header = json.loads(str(z["header"][()]))
            if header.get("format") != FORMAT:
                raise ValueError("{}: format {!r}, expected {!r}".format(path, header.get("format"), FORMAT))
            params = {name: z[name] for name in z.files if name != "header"}
        return cls(header["genes"], header["nodes"], header["input_shape"], header["kernels_per_layer"],
                   header["kernel_sizes"], header["dense_units"], header["classes"], params,
                   batch_norm=header["batch_norm"], bn_eps=header["bn_eps"], loss=header["loss"],
                   dtype=header["dtype"], metrics=header.get("metrics"))

    # ------------------------------------------------------------ prediction
    def _check_x(self, x):
        x = np.asarray(x)
        if x.ndim == 3:
            x = x[None]
        if x.ndim != 4 or tuple(x.shape[1:]) != self.input_shape:
            raise ValueError("x must be [n, {}, {}, {}] (or one [H, W, C] image), got shape {}".format(
                *(self.input_shape + (tuple(np.shape(x)),))))
        return np.ascontiguousarray(x, dtype=np.float32)

    def predict(self, x, device=None, output="proba", batch=256, backend=None, dtype=None, tta=None):
        """Class probabilities (``"proba"``: softmax, fp32 ``[n, classes]``), ``"logits"`` or ``"label"``
        (int64: the most probable class, the lowest index on ties) of ``x`` ``[n, H, W, C]`` (or one
        ``[H, W, C]`` image), ``batch`` rows at a time.

        ``device`` None or ``"cpu"``: the stock-torch forward in fp32 (``dtype=torch.float64``: the
        tests' oracle). A ``cuda`` device: the HIP predictor; ``backend="torch"`` the stock-torch forward
        there instead. Both paths fill a short chunk with zero images (to ``EB`` rows on the HIP path,
        to a multiple of 32 on the torch path) and return the real rows only, so a row's result does
        not depend on how many rows are predicted with it.

        ``tta`` (test-time augmentation; see :func:`tta_views`): the logits / probabilities become the mean
        over the views of the image, in view order in fp32 (:func:`tta_combine`), the label the first
        maximum of the mean probabilities. The torch backend predicts each view in turn; the HIP predictor
        builds the views on the device (``gt_tta_views``) and averages them in the head (``gt_head_tta``)."""
        if output not in OUTPUTS:
            raise ValueError("output {!r}: expected one of {}".format(output, OUTPUTS))
        if int(batch) < 1:
            raise ValueError("batch must be positive")
        x = self._check_x(x)
        views = tta_views(tta, self.input_shape)
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            if dtype is not None:
                raise ValueError("dtype is an option of the torch backend")
            logits, proba = self.hip_predictor(dev, batch).run(x, views=views)
        elif backend == "torch" and views is None:
            logits, proba = self._torch_predict(x, dev, int(batch), dtype or torch.float32)
        elif backend == "torch":
            per = [self._torch_predict(tta_transform(x, *v), dev, int(batch), dtype or torch.float32) for v in views]
            logits, proba = tta_combine([p[0] for p in per]), tta_combine([p[1] for p in per])
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        if output == "logits":
            return logits
        if output == "proba":
            return proba
        return np.argmax(proba, axis=1).astype(np.int64)          # first maximum: the head kernels' scan

    def predict_classes(self, x, **kw):
        return self.predict(x, output="label", **kw)

    def occlusion(self, x, target=None, patch=4, stride=None, fill=0.0, score="proba", device=None, batch=256,
                  backend=None, return_info=False):
        """Occlusion sensitivity (Zeiler & Fergus) of ``x`` ``[n, H, W, C]`` (or one image): fp32
        ``[n, Gh, Gw]`` with ``map[r, gi, gj] = s(x[r]) - s(O_cell(x[r]))``, one fp32 subtraction, where
        ``O_cell`` replaces cell ``(gi, gj)`` of :func:`occlusion_grid` by ``fill`` (a number or one per channel)
        and ``s`` is the probability (``score="proba"``) or the logit (``"logit"``) of the target class. Positive:
        the region supports the class.

        ``target``: ``None`` for the model's own label of the unoccluded image (the first maximum of the
        probabilities), one class index, or one per image. ``return_info=True`` returns
        ``(map, {"target": int64 [n], "base": fp32 [n]})``, the classes used and ``s(x[r])``.

        ``device`` / ``backend`` / ``batch`` as in :meth:`predict`: the CPU or ``backend="torch"`` feeds
        :func:`occlusion_views` to the stock-torch forward and subtracts in numpy; a ``cuda`` device uploads every
        image once, builds the occluded copies on the device (``gt_occlude_views``), packs them densely into
        launches of ``EB`` rows and keeps one float per copy (``gt_head_occlusion``)."""
        if score not in OCC_SCORES:
            raise ValueError("score {!r}: expected one of {}".format(score, OCC_SCORES))
        if int(batch) < 1:
            raise ValueError("batch must be positive")
        x = self._check_x(x)
        occlusion_grid(self.input_shape, patch, stride)
        fill = occlusion_fill(fill, self.input_shape[2])
        target = occlusion_targets(target, x.shape[0], self.classes)
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            res = self.hip_predictor(dev, batch).occlusion(x, target, patch, stride, fill, score)
        elif backend == "torch":
            def scores(images):
                logits, proba = self._torch_predict(images, dev, int(batch), torch.float32)
                return (logits if score == "logit" else proba), proba
            res = occlusion_by_views(scores, x, target, patch, stride, fill, int(batch))
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        return (res[0], {"target": res[1], "base": res[2]}) if return_info else res[0]

    def rise(self, x, target=None, masks=2048, cells=7, p=0.5, seed=0, fill=0.0, score="proba", device=None,
             batch=256, backend=None, return_info=False):
        """RISE saliency (Petsiuk et al., randomized input sampling) of ``x`` ``[n, H, W, C]`` (or one image): fp32
        ``[n, H, W]`` with ``map[r] = (sum_i s_{r,i} M_i) / (masks * p)``, where the ``masks`` random soft masks
        ``M_i`` (:func:`rise_masks`: a ``cells`` x ``cells`` grid of bits set with probability ``p``, upsampled
        bilinearly under a random shift; functions of ``seed``, shared by all images) blend the image with ``fill``
        (:func:`rise_views`) and ``s`` is the probability (``score="proba"``) or the logit (``"logit"``) of the
        target class of the blended image. Per pixel, by perturbation alone: no gradient is taken.

        ``target``, ``fill``, ``return_info`` and ``device`` / ``backend`` / ``batch`` as in :meth:`occlusion`. The
        CPU or ``backend="torch"`` feeds the views to the stock-torch forward and accumulates in fp64
        (:func:`rise_by_views`); a ``cuda`` device uploads every image once, blends on the device
        (``gt_rise_views``), packs the copies densely into launches of ``EB`` rows, keeps one score per copy
        (``gt_head_rise``) and forms ``scores x masks`` on the matrix cores (``gt_rise_accumulate``)."""
        if score not in OCC_SCORES:
            raise ValueError("score {!r}: expected one of {}".format(score, OCC_SCORES))
        x = self._check_x(x)
        masks, cells, p, seed = rise_check(self.input_shape, x.shape[0], masks, cells, p, seed, batch)
        fill = occlusion_fill(fill, self.input_shape[2])
        target = occlusion_targets(target, x.shape[0], self.classes, "rise")
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            rise_check_hip(self.classes)
            res = self.hip_predictor(dev, batch).rise(x, target, masks, cells, p, seed, fill, score)
        elif backend == "torch":
            def scores(images):
                logits, proba = self._torch_predict(images, dev, int(batch), torch.float32)
                return (logits if score == "logit" else proba), proba
            res = rise_by_views(scores, x, target, masks, cells, p, seed, fill, int(batch))
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        return (res[0], {"target": res[1], "base": res[2]}) if return_info else res[0]

    def gradcam(self, x, target=None, score="logit", relu=True, upsample=False, device=None, batch=256,
                backend=None, return_info=False):
        """Grad-CAM (Selvaraju et al.) of ``x`` ``[n, H, W, C]`` (or one image) at the network's last feature map
        ``A [C, hr, wr]`` (:func:`cam_shape`): fp32 ``[n, hr, wr]`` with
        ``cam[i, j] = sum_c alpha[c] * A[c, i, j]``, ``alpha[c]`` the mean over the pixels of ``dS/dA[c]``, then
        ``max(., 0)`` unless ``relu=False``. ``S`` is the logit (``score="logit"``) or the probability
        (``"proba"``) of the target class: ``None`` for the model's own label (the first maximum of the
        probabilities), one class index, or one per image. One forward per image; :meth:`occlusion` costs one per
        grid cell.

        ``upsample=True`` returns ``[n, H, W]`` by :func:`cam_upsample`, applied on the host after either
        backend. ``return_info=True`` returns ``(map, {"target": int64 [n], "base": fp32 [n]})``, the classes
        used and ``S(x[r])``.

        ``device`` / ``backend`` / ``batch`` as in :meth:`predict`: the CPU or ``backend="torch"`` runs the
        stock-torch forward up to ``A`` and the dense head under autograd; a ``cuda`` device runs the HIP
        predictor's forward and ``gt_head_gradcam``, where the gradient collapses to the dense head's weights
        (``gt_cam_w1sum``, once per predictor)."""
        cam_check(score, relu, upsample, batch)
        x = self._check_x(x)
        target = occlusion_targets(target, x.shape[0], self.classes, "gradcam")
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            cam_check_hip(self.plan, self.input_shape)
            res = self.hip_predictor(dev, batch).gradcam(x, target, score, bool(relu))
        elif backend == "torch":
            res = self._torch_gradcam(x, target, score, bool(relu), dev, int(batch), torch.float32)
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        cam = cam_upsample(res[0], self.input_shape[:2]) if upsample else res[0]
        return (cam, {"target": res[1], "base": res[2]}) if return_info else cam

    def saliency(self, x, target=None, score="logit", method="gradient", steps=16, baseline=0.0, reduce="absmax",
                 device=None, batch=256, backend=None, return_info=False, smooth=None):
        """Per-pixel attribution of ``x`` ``[n, H, W, C]`` (or one image) at input resolution, fp32. With ``s`` the
        logit (``score="logit"``) or the probability (``"proba"``) of the target class (``None``: the model's own
        label, one class index, or one per image -- :meth:`gradcam`'s definitions) and ``g = ds/dx``:

        ``method="gradient"``: ``a = g(x)``; ``"gradxinput"``: ``a = x * g(x)``; ``"integrated"`` (Sundararajan et
        al., midpoint rule): ``a = (x - x0) * (1/m) * sum_k g(x0 + ((k + 0.5)/m)(x - x0))`` with ``m = steps`` in
        1..64 and ``x0 = baseline`` (a number or one per channel), the sum in ascending ``k`` in fp32
        (:func:`saliency_finish`).

        ``reduce="absmax"`` returns ``max_c |a|`` ``[n, H, W]``, ``"sum"`` the channels added in order, ``None`` the
        signed ``[n, H, W, C]``. ``return_info=True`` returns ``(map, {"target": int64 [n], "base": fp32 [n]})``
        with ``base = s(x)``; for ``"integrated"`` also ``"baseline_score"``, ``s(x0)`` per row, so that
        ``a.sum() ~ base - baseline_score`` (completeness).

        ``smooth={"samples": S, "noise": f, "seed": s, "stat": "mean" | "sq" | "var"}`` (``"gradient"`` and
        ``"gradxinput"`` only; missing keys: 32, 0.15, 0, ``"mean"``) replaces ``g(x)`` by a statistic of the
        gradients at ``S <= 64`` noisy copies ``x + sigma_n z`` with ``sigma_n = f * (max - min)`` of image ``n``
        and ``z`` standard normal, keyed by ``(seed, index of the image in the call, sample, pixel, channel)``
        (:func:`gentun_amd.utils.rng.sg_noise`): the mean (SmoothGrad, Smilkov et al.), the mean of squares
        (SmoothGrad^2) or the variance (VarGrad, Adebayo et al.), formed by :func:`smooth_finish`;
        ``"gradxinput"`` multiplies by the clean ``x`` (``x * x`` for ``"sq"`` and ``"var"``). Target and ``base``
        are those of the clean image.

        ``device`` / ``backend`` / ``batch`` as in :meth:`predict`: the CPU or ``backend="torch"`` runs the
        stock-torch forward under autograd on the input; a ``cuda`` device runs the HIP predictor's forward with the
        pool masks on, then the training step's own data-gradient launches in evaluation mode down to
        ``gt_conv_in_dgrad`` (:class:`SaliencyState`)."""
        steps, x0 = saliency_check(score, method, steps, baseline, reduce, batch, self.input_shape[2], smooth)
        smooth = smooth_spec(smooth, method)
        x = self._check_x(x)
        target = occlusion_targets(target, x.shape[0], self.classes, "saliency")
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            saliency_check_hip(self.classes, steps, method, predict_batch(batch), smooth)
            res = self.hip_predictor(dev, batch).saliency(x, target, score, method, steps, x0, reduce, smooth)
        elif backend == "torch":
            a, tgt, base, bs = self._torch_saliency(x, target, score, method, steps, x0, dev, int(batch),
                                                    torch.float32, smooth)
            res = (saliency_reduce(a, reduce), tgt, base, bs)
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        return (res[0], saliency_info(res, method)) if return_info else res[0]

    def _torch_input_grad(self, x, target, score, dev, batch, dtype):
        """``(g [n, H, W, C], target int64 [n], s [n])`` by stock torch in ``dtype``: the forward of
        :meth:`_torch_predict` with autograd on the input, ``g = ds/dx`` for the score ``s`` of the target (the
        first maximum of the probabilities where ``target`` is None). Chunks of ``batch`` rows, filled with zero
        images to a multiple of 32 exactly as :meth:`_torch_predict` fills them. ``x`` may be fp64."""
        P = self._tensors(dev, dtype)
        n = x.shape[0]
        h, w, c = self.input_shape
        ftype = np.float64 if dtype == torch.float64 else np.float32
        grad, base, tgt = np.empty((n, h, w, c), ftype), np.empty(n, ftype), np.empty(n, np.int64)
        for s in range(0, n, batch):
            m = min(batch, n - s)
            buf = np.zeros(((m + 31) // 32 * 32, c, h, w), x.dtype)
            buf[:m] = x[s:s + m].transpose(0, 3, 1, 2)
            xb = torch.from_numpy(buf).to(device=dev, dtype=dtype).requires_grad_(True)
            with torch.enable_grad():
                logits = self._torch_forward(xb, P)
                proba = torch.softmax(logits, dim=-1)
                if target is None:                   # first maximum: the head kernels' scan
                    t = np.argmax(proba[:m].detach().cpu().numpy(), axis=1).astype(np.int64)
                else:
                    t = target[s:s + m]
                rows = torch.arange(m, device=dev)
                picked = (logits if score == "logit" else proba)[rows, torch.from_numpy(t).to(dev)]
                g, = torch.autograd.grad(picked.sum(), xb)
            grad[s:s + m] = g[:m].permute(0, 2, 3, 1).cpu().numpy()
            base[s:s + m] = picked.detach().cpu().numpy()
            tgt[s:s + m] = t
        return grad, tgt, base

    def _torch_saliency(self, x, target, score, method, steps, x0, dev, batch, dtype, smooth=None):
        """``(a [n, H, W, C] signed, target int64 [n], base [n], baseline_score [n] or None)`` by stock torch in
        ``dtype`` (fp32, or fp64: the tests' reference, which also forms the interpolation points and the sums in
        fp64): :meth:`_torch_input_grad` at ``x`` -- or, for ``"integrated"``, at every point of
        :func:`ig_point` for the target and ``base`` of ``x`` itself -- finished by :func:`saliency_finish`. With
        ``smooth`` (:func:`smooth_spec`'s tuple): the gradients at the points of :func:`smooth_point` for the
        target of ``x`` itself, finished by :func:`smooth_finish`."""
        ftype = np.float64 if dtype == torch.float64 else np.float32
        xs = x.astype(ftype)
        g, tgt, base = self._torch_input_grad(xs, target, score, dev, batch, dtype)
        if smooth is not None:
            S, noise, seed, stat = smooth
            sigma = smooth_sigma(x, noise)
            grads = [self._torch_input_grad(smooth_point(xs, sigma, seed, k), tgt, score, dev, batch, dtype)[0]
                     for k in range(S)]
            return smooth_finish(grads, xs, method, stat), tgt, base, None
        if method != "integrated":
            return saliency_finish([g], xs, x0, method), tgt, base, None
        grads = [self._torch_input_grad(ig_point(xs, x0, al), tgt, score, dev, batch, dtype)[0]
                 for al in ig_alphas(steps)]
        zero = np.broadcast_to(x0, (1,) + self.input_shape).copy()
        lg, pr = self._torch_predict(zero, dev, batch, dtype)
        bs = (lg if score == "logit" else pr)[0][tgt]
        return saliency_finish(grads, xs, x0, method), tgt, base, bs

    def predict_mc(self, x, samples=32, dropout=0.5, seed=0, device=None, batch=256, backend=None,
                   return_samples=False):
        """Monte-Carlo dropout (Gal & Ghahramani) of ``x`` ``[n, H, W, C]`` (or one image): ``samples`` forward
        passes of the dense head with the dropout between its two layers switched on at rate ``dropout`` (model
        files do not record the rate: the reference's 0.5 unless given), everything before it in evaluation
        mode. Returns a dict of fp32 arrays (:func:`mc_statistics`): ``proba [n, classes]``, the mean
        probability; ``std [n, classes]``, its standard deviation over the samples; ``entropy [n]`` of the mean;
        ``mutual_info [n]`` (BALD), the entropy minus the samples' mean entropy (:func:`mc_mutual_info`); ``label`` int64 ``[n]``, the
        first maximum of ``proba``. ``return_samples=True`` adds ``samples`` ``[n, 1, samples, classes]``.

        The mask of sample ``t``, image ``n`` (the index in ``x``, so chunking changes no bit) and hidden unit
        ``u`` is ``utils.rng.mc_masks(seed, 0, ...)``; a kept unit is ``h[u] * keep_scale``. With ``dropout=0``
        every sample is the plain forward.

        ``device`` / ``backend`` / ``batch`` as in :meth:`predict`: the CPU or ``backend="torch"`` runs the
        stock-torch forward up to the hidden row once and the second dense layer per sample; a ``cuda`` device
        runs the HIP predictor's forward and ``gt_head_mc`` (csrc/hip/cnn_head_mc.hip), which draws the masks on
        the device and writes only the statistics."""
        samples, dropout, seed, batch = mc_check(samples, dropout, seed, batch)
        x = self._check_x(x)
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            mc_check_hip(self.classes)
            return self.hip_predictor(dev, batch).predict_mc(x, samples, dropout, seed, bool(return_samples))
        if backend != "torch":
            raise ValueError("unknown backend {!r}".format(backend))
        p = self._torch_mc(x, 0, samples, dropout, seed, dev, batch, torch.float32)[None]
        return mc_result(mc_statistics(p, np.ones(1, np.float32)), p if return_samples else None)

    def embed(self, x, device=None, batch=256, backend=None):
        """The feature vectors of ``x`` ``[n, H, W, C]`` (or one image), fp32 ``[n, dense_units]``: the post-ReLU
        output of the dense hidden layer in evaluation mode (no dropout), real units only.

        ``device`` / ``backend`` / ``batch`` as in :meth:`predict`: the CPU or ``backend="torch"`` runs the
        stock-torch forward up to the hidden row; a ``cuda`` device runs the HIP predictor's forward and
        ``gt_dense_fwd`` and copies the real units of its output."""
        return embed_run(self, [self], x, device, batch, backend)

    def neighbors(self, x, bank, k=5, metric="l2", device=None, batch=256, backend=None):
        """The ``k`` (1..16) nearest rows of ``bank`` to every image of ``x`` in the feature space of
        :meth:`embed`: ``(index int64 [n, k], distance fp32 [n, k])`` in ascending ``(distance, bank index)``
        order, so a tie goes to the lower index. ``bank`` is images ``[N, H, W, C]``, embedded first, or fp32
        embeddings ``[N, dense_units]`` from :meth:`embed` (embed a bank once, search it many times).
        ``metric="l2"`` is the squared Euclidean distance ``max(|q|^2 + |b|^2 - 2 q.b, 0)``, ``"cosine"`` is
        ``1 - q.b / (|q| |b|)``, 1 when either norm is 0. Arguments are checked before any forward runs
        (:func:`neighbors_check`).

        The CPU or ``backend="torch"`` embeds by stock torch and searches on the host in fp64
        (:func:`neighbors_search`, the definition). A ``cuda`` device keeps the bank on the device as bf16
        planes (``gt_nn_bank``) and runs the product on the matrix cores with the selection fused
        (``gt_nn_topk``, ``gt_nn_merge``; csrc/hip/cnn_neighbors.hip) at fp32 accuracy: a distance is within
        the split-fp32 bound of the definition's and depends on its own query and bank row only, so results do
        not change with ``batch``; where two distances differ by less than the bound the order may differ from
        the host's. A bf16 fit rounds a bank of fp32 embeddings to bf16. A bank whose planes would pass 1 GiB on
        the device is a ``ValueError`` that names ``backend="torch"``.

        The host search is the definition, not a fast path: it updates all ``n x N`` sums once per feature, which
        is seconds for 1,000 x 10,000 x 500 and many minutes at 10,000 x 50,000 x 500 -- split such a bank and
        merge the results, or search it on the device. A bank row whose distance overflows to ``+inf`` is never
        returned by the device; a query with fewer than ``k`` finite distances gets ``(2^31 - 1, +inf)`` there."""
        return neighbors_run(self, [self], x, bank, k, metric, device, batch, backend)

    def gaussian_fit(self, bank, labels=None, shrink=0.01, device=None, batch=256, backend=None):
        """Class-conditional Gaussians with one tied covariance in the feature space of :meth:`embed` (Lee et al.,
        2018), for :meth:`mahalanobis`. ``bank`` is images ``[N, H, W, C]`` or embeddings ``[N, dense_units]``
        as in :meth:`neighbors`; ``labels`` an int array ``[N]`` in ``0..classes-1`` or one-hot ``[N, classes]``,
        ``None`` for one Gaussian over the whole bank; ``shrink`` in ``[0, 1]`` blends the covariance with
        ``trace / U`` times the identity. Returns a plain dict of numpy arrays (``np.savez`` keeps it; nothing goes
        into model files): ``count`` int64 ``[C]``, ``mean`` fp32 ``[1, C, U]``, ``cov`` fp64 ``[1, U, U]`` (the
        within-class scatter over ``N``, before shrinkage), ``whiten`` fp32 ``[1, U, U]`` (``W = L^-T`` of the
        shrunk covariance ``L L^T``), ``wmean`` fp32 ``[1, C, U]`` (``W^T mean_c``) and ``shrink``. A singular
        covariance (dead units at ``shrink=0``) is a ``ValueError`` that names ``shrink``.

        The CPU or ``backend="torch"`` embeds by stock torch and runs the fp64 host definitions
        (:func:`gaussian_moments`, :func:`gaussian_whiten`). A ``cuda`` device keeps the bank's hidden rows on the
        device (at most 1 GiB, else a ``ValueError`` naming ``backend="torch"``) and forms the sums and the
        scatter matrix there (csrc/hip/cnn_gaussian.hip): ``cov`` is within the split-fp32 bound of the
        definition's at a reduction length of 1024 rows and does not depend on ``batch``; at most 16 classes."""
        return gaussian_fit_run(self, [self], bank, labels, shrink, device, batch, backend)

    def mahalanobis(self, x, stats, device=None, batch=256, backend=None):
        """fp32 ``[n, C]``: the squared Mahalanobis distance of every image of ``x`` to every class Gaussian of
        ``stats`` (:meth:`gaussian_fit`), ``+inf`` for a class without rows. ``d.min(1)`` is the
        out-of-distribution score, ``d.argmin(1)`` the Gaussian-discriminant label. On a ``cuda`` device the
        whitening product and the per-class sums run in one kernel (``gt_fs_dist``) at fp32 accuracy."""
        return mahalanobis_run(self, [self], np.ones(1, np.float32), x, stats, device, batch, backend)

    def _torch_embed(self, x, dev, batch, dtype):
        """``embed`` by stock torch in ``dtype`` (fp32, or fp64: the tests' oracle): the chunks of
        :meth:`_torch_predict` up to the hidden row."""
        P = self._tensors(dev, dtype)
        n = x.shape[0]
        h, w, c = self.input_shape
        out = np.empty((n, self.dense_units), np.float64 if dtype == torch.float64 else np.float32)
        with torch.no_grad():
            for s in range(0, n, batch):
                m = min(batch, n - s)
                buf = np.zeros(((m + 31) // 32 * 32, c, h, w), np.float32)
                buf[:m] = x[s:s + m].transpose(0, 3, 1, 2)
                hid = self._torch_hidden(self._torch_features(torch.from_numpy(buf).to(device=dev, dtype=dtype), P), P)
                out[s:s + m] = hid[:m].cpu().numpy()
        return out

    def hip_predictor(self, device, batch=256):
        """The cached :class:`HipPredictor` of (device, rows per launch)."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (str(dev), predict_batch(batch))
        pred = self._predictors.get(key)
        if pred is None:
            pred = self._predictors[key] = HipPredictor(self, dev, key[1])
        return pred

    def _tensors(self, dev, dtype):
        key = (str(dev), dtype)
        P = self._torch_params.get(key)
        if P is None:
            P = self._torch_params[key] = {k: torch.from_numpy(v).to(device=dev, dtype=dtype)
                                           for k, v in self.params.items()}
        return P

    def _torch_forward(self, xb, P):
        """``xb`` [n, C, H, W] -> logits [n, classes]: TorchFoldJob._forward(train=False), one group."""
        return self._torch_head(self._torch_features(xb, P), P)

    def _torch_features(self, xb, P):
        """``xb`` [n, C, H, W] -> the output of the plan's last step [n, C_last, hr, wr]."""
        acts = {"input": xb}
        for st in self.plan.steps:
            if isinstance(st, ConvSpec):
                inp = acts[st.inputs[0]]
                for extra in st.inputs[1:]:
                    inp = inp + acts[extra]
                z = F.conv2d(inp, P[st.name + ".w"], P[st.name + ".b"], padding=(st.k[0] // 2, st.k[1] // 2))
                if self.batch_norm:
                    n = st.name
                    xh = (z - P[n + ".running_mean"].view(1, -1, 1, 1)) * \
                        torch.rsqrt(P[n + ".running_var"].view(1, -1, 1, 1) + self.bn_eps)
                    z = xh * P[n + ".gamma"].view(1, -1, 1, 1) + P[n + ".beta"].view(1, -1, 1, 1)
                acts[st.name] = F.relu(z)
            else:
                acts[st.name] = F.max_pool2d(acts[st.srcs[0]], 2, 2)
        return acts[self.plan.steps[-1].name]

    def _torch_head(self, A, P):
        """The last feature map [n, C_last, hr, wr] -> logits [n, classes]."""
        feat = A.reshape(1, A.shape[0], -1)
        h = F.relu(torch.baddbmm(P["dense1.b"][None, None, :], feat, P["dense1.w"][None]))
        return torch.baddbmm(P["dense2.b"][None, None, :], h, P["dense2.w"][None])[0]

    def _torch_hidden(self, A, P):
        """The last feature map [n, C_last, hr, wr] -> the hidden row ``h = relu(feat W1 + b1)`` [n, units]."""
        feat = A.reshape(1, A.shape[0], -1)
        return F.relu(torch.baddbmm(P["dense1.b"][None, None, :], feat, P["dense1.w"][None]))[0]

    def _torch_mc(self, x, member, samples, dropout, seed, dev, batch, dtype):
        """The Monte-Carlo dropout samples ``p [n, samples, classes]`` by stock torch in ``dtype`` (fp32, or
        fp64: the tests' reference) as member ``member`` of an ensemble: the forward of :meth:`_torch_predict`
        up to the hidden row once per chunk (rows filled with zero images to a multiple of 32), then per sample
        the masked row (``utils.rng.mc_masks``), the second dense layer at the chunk's padded rows and the
        softmax."""
        from ..utils.rng import mc_masks
        P = self._tensors(dev, dtype)
        n = x.shape[0]
        h, w, c = self.input_shape
        ftype = np.float64 if dtype == torch.float64 else np.float32
        scale = float(mc_keep_scale(dropout))
        out = np.empty((n, samples, self.classes), ftype)
        with torch.no_grad():
            for s in range(0, n, batch):
                m = min(batch, n - s)
                rows = (m + 31) // 32 * 32
                buf = np.zeros((rows, c, h, w), np.float32)
                buf[:m] = x[s:s + m].transpose(0, 3, 1, 2)
                hid = self._torch_hidden(self._torch_features(torch.from_numpy(buf).to(device=dev, dtype=dtype), P), P)
                keep = torch.from_numpy(mc_masks(seed, member, samples, np.arange(s, s + rows), self.dense_units,
                                                 dropout)).to(dev)
                kept = hid * torch.tensor(scale, dtype=dtype, device=dev)
                for t in range(samples):
                    hm = torch.where(keep[t], kept, torch.zeros_like(kept))
                    lg = torch.baddbmm(P["dense2.b"][None, None, :], hm[None], P["dense2.w"][None])[0, :m]
                    out[s:s + m, t] = torch.softmax(lg, dim=-1).cpu().numpy()
        return out

    def _torch_gradcam(self, x, target, score, relu, dev, batch, dtype):
        """``(map [n, hr, wr], target int64 [n], base [n])`` by stock torch in ``dtype`` (fp32, or fp64: the
        tests' oracle): the forward of :meth:`_torch_predict` up to the last feature map ``A`` without autograd,
        then the dense head with autograd on ``A``, ``alpha = grad.mean((2, 3))``. Chunks of ``batch`` rows,
        filled with zero images to a multiple of 32 exactly as :meth:`_torch_predict` fills them."""
        P = self._tensors(dev, dtype)
        n = x.shape[0]
        h, w, c = self.input_shape
        hr, wr = cam_shape(self.plan, self.input_shape)
        ftype = np.float64 if dtype == torch.float64 else np.float32
        cam, base, tgt = np.empty((n, hr, wr), ftype), np.empty(n, ftype), np.empty(n, np.int64)
        for s in range(0, n, batch):
            m = min(batch, n - s)
            buf = np.zeros(((m + 31) // 32 * 32, c, h, w), np.float32)
            buf[:m] = x[s:s + m].transpose(0, 3, 1, 2)
            with torch.no_grad():
                A = self._torch_features(torch.from_numpy(buf).to(device=dev, dtype=dtype), P)
            A = A.detach().requires_grad_(True)
            with torch.enable_grad():
                logits = self._torch_head(A, P)
                proba = torch.softmax(logits, dim=-1)
                if target is None:                   # first maximum: the head kernels' scan
                    t = np.argmax(proba[:m].detach().cpu().numpy(), axis=1).astype(np.int64)
                else:
                    t = target[s:s + m]
                rows = torch.arange(m, device=dev)
                picked = (logits if score == "logit" else proba)[rows, torch.from_numpy(t).to(dev)]
                grad, = torch.autograd.grad(picked.sum(), A)
            with torch.no_grad():
                alpha = grad[:m].mean((2, 3))
                cm = (alpha[:, :, None, None] * A[:m]).sum(1)
                cam[s:s + m] = cm.cpu().numpy()
                base[s:s + m] = picked.detach().cpu().numpy()
            tgt[s:s + m] = t
        if relu:
            cam = np.maximum(cam, ftype(0))
        return cam, tgt, base

    def _torch_predict(self, x, dev, batch, dtype):
        P = self._tensors(dev, dtype)
        n = x.shape[0]
        h, w, c = self.input_shape
        logits = np.empty((n, self.classes), np.float64 if dtype == torch.float64 else np.float32)
        proba = np.empty_like(logits)
        with torch.no_grad():
            for s in range(0, n, batch):
                # a fresh NCHW buffer: canonical strides (a permuted one-channel image keeps NHWC strides and
                # the convolution then takes its channels-last path, with other rounding than the
                # executor's), rows padded with zero images to a multiple of 32 like the HIP predictor's
                # launches (the BLAS / convolution paths of a batch of a few rows round differently)
                m = min(batch, n - s)
                buf = np.zeros(((m + 31) // 32 * 32, c, h, w), np.float32)
                buf[:m] = x[s:s + m].transpose(0, 3, 1, 2)
                lg = self._torch_forward(torch.from_numpy(buf).to(device=dev, dtype=dtype), P)[:m]
                if dtype not in (torch.float32, torch.float64):
                    lg = lg.float()
                logits[s:s + batch] = lg.cpu().numpy()
                proba[s:s + batch] = torch.softmax(lg, dim=-1).cpu().numpy()
        return logits, proba


# ---------------------------------------------------------------------------
# parameter layouts of the two executors
# ---------------------------------------------------------------------------

def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _export_torch(job, g):
    V = job._views()
    out = {}
    for name, _, _, _ in job.shapes:
        out[name] = _np(V[name][g])
    for name, run in job.bn_run.items():
        out[name + ".running_mean"] = _np(run[0][g])
        out[name + ".running_var"] = _np(run[1][g])
    return out


def _import_torch(clf, job, g):
    with torch.no_grad():
        V = job._views()
        for name, _, _, _ in job.shapes:
            V[name][g].copy_(torch.from_numpy(clf.params[name]))
        for name, run in job.bn_run.items():
            run[0][g].copy_(torch.from_numpy(clf.params[name + ".running_mean"]))
            run[1][g].copy_(torch.from_numpy(clf.params[name + ".running_var"]))


def _hip_dense_geometry(job, plan):
    hs, ws = job.final_hw
    hr, wr = job.final_hw_real
    return hs, ws, hr, wr, job.final_cp, plan.kernels_per_layer[-1], plan.dense_units


def _export_hip(job, plan, g):
    """Strip the channel padding, the ``Up`` padding and the padded-pixel rows of ``W1`` from the HIP
    executor's fp32 masters (conv kernels ``[Coutp][KH][KW][Cinp]``, ``W1`` ``[hs][ws][Cp][Up]``)."""
    layers = {L.name: L for L in job.layers}
    out = {}
    for st in plan.convs():
        L = layers[st.name]
        out[st.name + ".w"] = _np(L.w[0][g][:L.cout, :, :, :L.cin].permute(0, 3, 1, 2))
        out[st.name + ".b"] = _np(L.b[0][g][:L.cout])
        if job.bn:
            out[st.name + ".gamma"] = _np(L.gamma[0][g][:L.cout])
            out[st.name + ".beta"] = _np(L.beta[0][g][:L.cout])
            out[st.name + ".running_mean"] = _np(L.bn_run[0][g][:L.cout])
            out[st.name + ".running_var"] = _np(L.bn_run[1][g][:L.cout])
    hs, ws, hr, wr, cp, C, U = _hip_dense_geometry(job, plan)
    W1 = job.views["W1"][0][g].view(hs, ws, cp, job.Up)[:hr, :wr, :C, :U]            # NHWC features
    out["dense1.w"] = _np(W1.permute(2, 0, 1, 3).reshape(C * hr * wr, U))              # -> NCHW flatten
    out["dense1.b"] = _np(job.views["b1"][0][g][:U])
    out["dense2.w"] = _np(job.views["W2"][0][g][:U])
    out["dense2.b"] = _np(job.views["b2"][0][g])
    return out


def _import_hip(clf, job, g):
    plan, dev = clf.plan, job.device
    layers = {L.name: L for L in job.layers}

    def t(name):
        return torch.from_numpy(clf.params[name]).to(dev)

    for L in job.layers:                         # every element of the group, padding included, to its
        L.w[0][g].zero_()                        # untrained value; layers the genome lacks stay there
        L.b[0][g].zero_()
        if job.bn:
            L.gamma[0][g].zero_()
            L.beta[0][g].zero_()
            L.bn_run[0][g].zero_()
            L.bn_run[1][g].fill_(1.0)
    for st in plan.convs():
        L = layers[st.name]
        L.w[0][g][:L.cout, :, :, :L.cin].copy_(t(st.name + ".w").permute(0, 2, 3, 1))
        L.b[0][g][:L.cout].copy_(t(st.name + ".b"))
        if job.bn:
            L.gamma[0][g][:L.cout].copy_(t(st.name + ".gamma"))
            L.beta[0][g][:L.cout].copy_(t(st.name + ".beta"))
            L.bn_run[0][g][:L.cout].copy_(t(st.name + ".running_mean"))
            L.bn_run[1][g][:L.cout].copy_(t(st.name + ".running_var"))
    hs, ws, hr, wr, cp, C, U = _hip_dense_geometry(job, plan)
    for name in ("W1", "b1", "W2", "b2"):
        job.views[name][0][g].zero_()
    W1 = job.views["W1"][0][g].view(hs, ws, cp, job.Up)
    W1[:hr, :wr, :C, :U].copy_(t("dense1.w").view(C, hr, wr, U).permute(1, 2, 0, 3))
    job.views["b1"][0][g][:U].copy_(t("dense1.b"))
    job.views["W2"][0][g][:U].copy_(t("dense2.w"))
    job.views["b2"][0][g].copy_(t("dense2.b"))
    job._refresh_copies()        # bf16 planes, fragment planes and Winograd planes from the masters


# ---------------------------------------------------------------------------
# HIP predictor
# ---------------------------------------------------------------------------

class TtaState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for one tuple of test-time
    augmentation views: the raw chunk buffer of ``R = EB // V`` images in the staging tensor's layout and
    element type (zero outside the real extent), the arguments of ``gt_tta_views`` (raw chunk -> rows
    ``v * R + r`` of the staging tensor) and of ``gt_head_tta`` (per member the mean over the views, then
    the members' weighted mean and votes), and the outputs of ``R`` rows. The predictor's job, evaluation
    launches and gather table are used as they are, at ``EB`` rows."""

    def __init__(self, pred, views, G, weight):
        K, job, stage, C = pred.K, pred.job, pred.stage, pred.classes
        self.views, self.V = tuple(views), len(views)
        self.R = R = pred.EB // self.V
        if not 1 <= self.V <= K.TTA_MAXV or R < 1:
            raise ValueError("{} views do not fit {} rows per launch".format(self.V, pred.EB))
        dev = pred.device
        self.raw = torch.zeros((R,) + tuple(stage.shape[1:]), dtype=stage.dtype, device=dev)
        self.weight = weight
        self.logits = torch.empty((G, R, C), dtype=torch.float32, device=dev)
        self.proba = torch.empty_like(self.logits)
        self.ens = torch.empty((R, C), dtype=torch.float32, device=dev)
        self.votes = torch.empty((R, C), dtype=torch.int32, device=dev)
        va = K.TtaViewArgs()
        va.raw, va.out = self.raw.data_ptr(), stage.data_ptr()
        va.R, va.V, va.rows = R, self.V, pred.EB
        va.Hp, va.Wp, va.Cp = (int(d) for d in stage.shape[1:])
        va.Hr, va.Wr = pred.hwc[0], pred.hwc[1]
        va.prec = 1 if stage.dtype == torch.float32 else 0
        for i, (dy, dx, flip) in enumerate(self.views):
            va.dy[i], va.dx[i], va.flip[i] = dy, dx, flip
        self.view_args = va
        self.heads = {}
        for members in (False, True):            # the member outputs are written on request only
            a = K.HeadTtaArgs()
            a.plog, a.b2, a.weight = pred.df.plog, job.views["b2"][0].data_ptr(), weight.data_ptr()
            a.logits = self.logits.data_ptr() if members else 0
            a.proba = self.proba.data_ptr() if members else 0
            a.ens, a.votes = self.ens.data_ptr(), self.votes.data_ptr()
            a.G, a.B, a.Up, a.C = G, pred.EB, job.Up, C
            a.R, a.V, a.inv_v = R, self.V, float(np.float32(1) / np.float32(self.V))
            self.heads[members] = a

    def upload(self, chunk, hwc):
        """``chunk`` [m <= R, H, W, C] host fp32 into the raw buffer; rows past ``m`` become zero images."""
        m = chunk.shape[0]
        h, w, c = hwc
        if m < self.R:
            self.raw[m:].zero_()
        self.raw[:m, :h, :w, :c].copy_(torch.from_numpy(chunk).to(self.raw.device))

    def forward(self, pred, members, what):
        """The launches of one chunk on the current stream: raw buffer -> views in the staging tensor ->
        the predictor's forward at ``EB`` rows -> the outputs of ``R`` rows."""
        job, K = pred.job, pred.K
        s = job._stream()
        K.check(job.L.gt_tta_views(self.view_args, s), "tta_views")
        job._run_fwd(s, pred.ops)
        K.check(job.L.gt_dense_fwd(pred.df, s), "dense_fwd({})".format(what))
        K.check(job.L.gt_head_tta(self.heads[bool(members)], s), "head_tta")


class OcclusionState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for one occlusion setting
    ``(patch, stride, fill, score)``: the raw buffer of up to ``EB`` images in the staging tensor's layout and
    element type (zero outside the real extent and in the channel padding), the fill value in that type, the
    arguments of ``gt_occlude_views`` (raw buffer -> the launch's items in the staging tensor) and of
    ``gt_head_occlusion`` (phase 0: target and base score per image; phase 1: one map element per launch row)
    and the results of one group. The unit of work is the item ``w = r * Cc + cell``; items are packed densely
    into launches of ``EB`` rows. The predictor's job, evaluation launches and gather table are used as they
    are, at ``EB`` rows."""

    def __init__(self, pred, patch, stride, fill, score, G, weight):
        K, job, stage = pred.K, pred.job, pred.stage
        h, w, c = pred.hwc
        self.Gh, self.Gw = occlusion_grid(pred.hwc, patch, stride)
        self.Cc = Cc = self.Gh * self.Gw
        EB, dev = pred.EB, pred.device
        self.raw = torch.zeros((EB,) + tuple(stage.shape[1:]), dtype=stage.dtype, device=dev)
        f = torch.zeros(int(stage.shape[3]), dtype=torch.float32)
        f[:c] = torch.from_numpy(occlusion_fill(fill, c))
        self.fill = f.to(stage.dtype).to(dev)            # rounded to the staging type on the host
        self.weight = weight
        self.tgt = torch.empty(EB, dtype=torch.int32, device=dev)
        self.base = torch.empty(EB, dtype=torch.float32, device=dev)
        self.map = torch.empty(EB * Cc, dtype=torch.float32, device=dev)
        va = K.OccludeArgs()
        va.raw, va.out, va.fill = self.raw.data_ptr(), stage.data_ptr(), self.fill.data_ptr()
        va.Cc, va.Gw, va.patch = Cc, self.Gw, int(patch)
        va.stride = int(patch if stride is None else stride)
        va.rows = va.cap = EB
        va.Hp, va.Wp, va.Cp = (int(d) for d in stage.shape[1:])
        va.Hr, va.Wr = h, w
        va.prec = 1 if stage.dtype == torch.float32 else 0
        self.view_args = va
        a = K.HeadOcclusionArgs()
        a.plog, a.b2, a.weight = pred.df.plog, job.views["b2"][0].data_ptr(), weight.data_ptr()
        a.tgt, a.base, a.map = self.tgt.data_ptr(), self.base.data_ptr(), self.map.data_ptr()
        a.G, a.B, a.Up, a.C = G, EB, job.Up, pred.classes
        a.Cc, a.logit = Cc, 1 if score == "logit" else 0
        self.head = a

    def upload(self, chunk, target, hwc):
        """``chunk`` [m <= EB, H, W, C] host fp32 into the raw buffer (rows past ``m`` become zero images) and
        its targets (int64 ``[m]``, or ``None``: -1, the label) into ``tgt``."""
        m = chunk.shape[0]
        h, w, c = hwc
        if m < self.raw.shape[0]:
            self.raw[m:].zero_()
        self.raw[:m, :h, :w, :c].copy_(torch.from_numpy(chunk).to(self.raw.device))
        if target is None:
            self.tgt.fill_(-1)
        else:
            self.tgt[:m].copy_(torch.from_numpy(target.astype(np.int32)).to(self.tgt.device))

    def launch(self, pred, m, w0, base):
        """One launch set on the current stream: the items from ``w0`` (``base``: the ``m`` images as they are)
        -> the staging tensor -> the predictor's forward at ``EB`` rows -> ``tgt`` / ``base`` or ``map``."""
        job, K = pred.job, pred.K
        s = job._stream()
        va, a = self.view_args, self.head
        va.m, va.w0, va.base = m, w0, 1 if base else 0
        a.m, a.w0, a.phase = m, w0, 0 if base else 1
        K.check(job.L.gt_occlude_views(va, s), "occlude_views")
        job._run_fwd(s, pred.ops)
        K.check(job.L.gt_dense_fwd(pred.df, s), "dense_fwd(occlusion)")
        K.check(job.L.gt_head_occlusion(a, s), "head_occlusion")

    def run(self, pred, x, target):
        """``x`` [n, H, W, C] host fp32 -> ``(map [n, Gh, Gw], target int64 [n], base fp32 [n])`` as host
        arrays: per group of ``EB`` images one upload, one base launch and ``ceil(m * Cc / EB)`` packed launches;
        the results gather on the device and are read back once."""
        n, EB, Cc, dev = x.shape[0], pred.EB, self.Cc, pred.device
        with torch.cuda.device(dev):
            out = torch.empty(n * Cc, dtype=torch.float32, device=dev)
            tgt = torch.empty(n, dtype=torch.int32, device=dev)
            base = torch.empty(n, dtype=torch.float32, device=dev)
            for s in range(0, n, EB):
                m = min(EB, n - s)
                self.upload(x[s:s + m], None if target is None else target[s:s + m], pred.hwc)
                self.launch(pred, m, 0, True)
                for w0 in range(0, m * Cc, EB):
                    self.launch(pred, m, w0, False)
                out[s * Cc:(s + m) * Cc].copy_(self.map[:m * Cc])
                tgt[s:s + m].copy_(self.tgt[:m])
                base[s:s + m].copy_(self.base[:m])
            return (out.cpu().numpy().reshape(n, self.Gh, self.Gw), tgt.cpu().numpy().astype(np.int64),
                    base.cpu().numpy())


def occlusion_state(pred, patch, stride, fill, score, G, weight):
    """The cached :class:`OcclusionState` of a predictor (its ``_occ`` dict) for one setting."""
    stride = int(patch if stride is None else stride)
    key = (int(patch), stride, tuple(float(v) for v in fill), score)
    st = pred._occ.get(key)
    if st is None:
        with torch.cuda.device(pred.device):
            st = pred._occ[key] = OcclusionState(pred, int(patch), stride, fill, score, G, weight)
    return st


class RiseState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for one RISE setting
    ``(masks, cells, p, seed, fill, score)``: the raw buffer of up to ``EB`` fp32 images in the staging tensor's
    layout, the fill value, the three bf16 planes of every mask ``[3][Pp][Kp]`` (``gt_rise_masks``, once), the
    scores ``S [EB][Kp]`` (zeroed once: ``gt_head_rise`` writes the real entries only) and the arguments of
    ``gt_rise_views``, ``gt_head_occlusion`` phase 0 (target and base score per image), ``gt_head_rise`` and
    ``gt_rise_accumulate``. The unit of work is the item ``w = r * masks + i``; items are packed densely into
    launches of ``EB`` rows. The predictor's job, evaluation launches and gather table are used as they are."""

    def __init__(self, pred, masks, cells, p, seed, fill, score, G, weight):
        K, job, stage = pred.K, pred.job, pred.stage
        h, w, c = pred.hwc
        EB, dev = pred.EB, pred.device
        self.masks, self.P = masks, h * w
        self.Kp, self.Pp = (masks + 31) // 32 * 32, (h * w + 63) // 64 * 64
        self.raw = torch.zeros((EB,) + tuple(stage.shape[1:]), dtype=torch.float32, device=dev)
        f = torch.zeros(int(stage.shape[3]), dtype=torch.float32)
        f[:c] = torch.from_numpy(occlusion_fill(fill, c))
        self.fill = f.to(dev)
        self.weight = weight
        self.tgt = torch.empty(EB, dtype=torch.int32, device=dev)
        self.base = torch.empty(EB, dtype=torch.float32, device=dev)
        self.S = torch.zeros((EB, self.Kp), dtype=torch.float32, device=dev)
        self.planes = torch.empty((3, self.Pp, self.Kp), dtype=torch.int16, device=dev)
        self.map = torch.empty((EB, self.P), dtype=torch.float32, device=dev)
        self.scores = None           # [n, masks] on the device: the scores of the last run
        thr = rise_threshold(p)
        ma = K.RiseMaskArgs()
        ma.planes, ma.masks, ma.Kp, ma.cells = self.planes.data_ptr(), masks, self.Kp, cells
        ma.seed, ma.thr, ma.Hr, ma.Wr, ma.Pp = seed, thr, h, w, self.Pp
        K.check(job.L.gt_rise_masks(ma, job._stream()), "rise_masks")
        va = K.RiseViewArgs()
        va.raw, va.out, va.fill = self.raw.data_ptr(), stage.data_ptr(), self.fill.data_ptr()
        va.masks, va.cells, va.seed, va.thr = masks, cells, seed, thr
        va.rows = va.cap = EB
        va.Hp, va.Wp, va.Cp = (int(d) for d in stage.shape[1:])
        va.Hr, va.Wr, va.Cr = h, w, c
        va.prec = 1 if stage.dtype == torch.float32 else 0
        self.view_args = va
        b = K.HeadOcclusionArgs()                        # phase 0 only: the map is never written
        b.plog, b.b2, b.weight = pred.df.plog, job.views["b2"][0].data_ptr(), weight.data_ptr()
        b.tgt, b.base, b.map = self.tgt.data_ptr(), self.base.data_ptr(), 0
        b.G, b.B, b.Up, b.C = G, EB, job.Up, pred.classes
        b.Cc, b.w0, b.phase, b.logit = masks, 0, 0, 1 if score == "logit" else 0
        self.base_head = b
        a = K.HeadRiseArgs()
        a.plog, a.b2, a.weight = b.plog, b.b2, b.weight
        a.tgt, a.S = self.tgt.data_ptr(), self.S.data_ptr()
        a.G, a.B, a.Up, a.C = G, EB, job.Up, pred.classes
        a.masks, a.Kp, a.logit = masks, self.Kp, b.logit
        self.head = a
        g = K.RiseAccArgs()
        g.planes, g.S, g.out = self.planes.data_ptr(), self.S.data_ptr(), self.map.data_ptr()
        g.masks, g.Kp, g.P, g.Pp = masks, self.Kp, self.P, self.Pp
        g.inv = float(np.float32(rise_inv(masks, p)))
        self.acc = g

    def upload(self, chunk, target, hwc):
        """``chunk`` [m <= EB, H, W, C] host fp32 into the raw buffer and its targets (int64 ``[m]``, or ``None``:
        -1, the label) into ``tgt``. Rows past ``m`` are never read."""
        m = chunk.shape[0]
        h, w, c = hwc
        self.raw[:m, :h, :w, :c].copy_(torch.from_numpy(chunk).to(self.raw.device))
        if target is None:
            self.tgt.fill_(-1)
        else:
            self.tgt[:m].copy_(torch.from_numpy(target.astype(np.int32)).to(self.tgt.device))

    def launch(self, pred, m, w0, base):
        """One launch set on the current stream: the items from ``w0`` (``base``: the ``m`` images as they are)
        -> the staging tensor -> the predictor's forward at ``EB`` rows -> ``tgt`` / ``base`` or ``S``."""
        job, K = pred.job, pred.K
        s = job._stream()
        va = self.view_args
        va.m, va.w0, va.base = m, w0, 1 if base else 0
        K.check(job.L.gt_rise_views(va, s), "rise_views")
        job._run_fwd(s, pred.ops)
        K.check(job.L.gt_dense_fwd(pred.df, s), "dense_fwd(rise)")
        if base:
            self.base_head.m = m
            K.check(job.L.gt_head_occlusion(self.base_head, s), "head_occlusion(rise)")
        else:
            self.head.m, self.head.w0 = m, w0
            K.check(job.L.gt_head_rise(self.head, s), "head_rise")

    def run(self, pred, x, target):
        """``x`` [n, H, W, C] host fp32 -> ``(map [n, H, W], target int64 [n], base fp32 [n])`` as host arrays:
        per group of ``EB`` images one upload, one base launch set, ``ceil(m * masks / EB)`` packed launch sets
        and one accumulate launch; the results gather on the device and are read back once."""
        n, EB, masks, dev = x.shape[0], pred.EB, self.masks, pred.device
        h, w, _ = pred.hwc
        job, K = pred.job, pred.K
        with torch.cuda.device(dev):
            out = torch.empty((n, self.P), dtype=torch.float32, device=dev)
            tgt = torch.empty(n, dtype=torch.int32, device=dev)
            base = torch.empty(n, dtype=torch.float32, device=dev)
            self.scores = torch.empty((n, masks), dtype=torch.float32, device=dev)
            for s in range(0, n, EB):
                m = min(EB, n - s)
                self.upload(x[s:s + m], None if target is None else target[s:s + m], pred.hwc)
                self.launch(pred, m, 0, True)
                for w0 in range(0, m * masks, EB):
                    self.launch(pred, m, w0, False)
                self.acc.m = m
                K.check(job.L.gt_rise_accumulate(self.acc, job._stream()), "rise_accumulate")
                out[s:s + m].copy_(self.map[:m])
                tgt[s:s + m].copy_(self.tgt[:m])
                base[s:s + m].copy_(self.base[:m])
                self.scores[s:s + m].copy_(self.S[:m, :masks])
            return (out.cpu().numpy().reshape(n, h, w), tgt.cpu().numpy().astype(np.int64), base.cpu().numpy())


def rise_state(pred, masks, cells, p, seed, fill, score, G, weight):
    """The cached :class:`RiseState` of a predictor (its ``_rise`` dict) for one setting."""
    key = (masks, cells, p, seed, tuple(float(v) for v in fill), score)
    st = pred._rise.get(key)
    if st is None:
        with torch.cuda.device(pred.device):
            st = pred._rise[key] = RiseState(pred, masks, cells, p, seed, fill, score, G, weight)
    return st


def cam_wbar(pred, G):
    """``wbar [G][Cp][Up]`` of a HIP predictor, ``W1`` summed over the real pixels of the last feature map
    (``gt_cam_w1sum``): a constant of the loaded parameters, computed on the first Grad-CAM request."""
    if pred._cam_wbar is None:
        K, job = pred.K, pred.job
        (hs, ws), (hr, wr) = job.final_hw, job.final_hw_real
        wbar = torch.empty((G, job.final_cp, job.Up), dtype=torch.float32, device=pred.device)
        a = K.CamW1SumArgs()
        a.w1, a.wbar = job.views["W1"][0].data_ptr(), wbar.data_ptr()
        a.G, a.hs, a.ws, a.hr, a.wr = G, hs, ws, hr, wr
        a.Cp, a.Cr, a.Up = job.final_cp, job.members[0][0].kernels_per_layer[-1], job.Up
        K.check(job.L.gt_cam_w1sum(a, job._stream()), "cam_w1sum")
        pred._cam_wbar = wbar
    return pred._cam_wbar


class GradcamState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for one Grad-CAM setting
    ``(score, relu)``: the arguments of ``gt_head_gradcam`` over the predictor's own buffers (the partial logits,
    the pooled feature map and the hidden activations that ``gt_dense_fwd`` read and wrote, the fp32 masters of
    ``W2`` and ``b2``, ``wbar``) and the results of one chunk. The predictor's job, evaluation launches, staging
    tensor and ``upload`` are used as they are, at ``EB`` rows."""

    def __init__(self, pred, score, relu, G, weight):
        K, job, EB, dev = pred.K, pred.job, pred.EB, pred.device
        (hs, ws), (hr, wr) = job.final_hw, job.final_hw_real     # at most CAM_MAX_PIXELS: cam_check_hip
        self.hr, self.wr, self.weight = hr, wr, weight
        self.wbar = cam_wbar(pred, G)
        self.tgt = torch.empty(EB, dtype=torch.int32, device=dev)
        self.base = torch.empty(EB, dtype=torch.float32, device=dev)
        self.map = torch.empty((EB, hr, wr), dtype=torch.float32, device=dev)
        a = K.HeadGradcamArgs()
        a.plog, a.b2, a.weight = pred.df.plog, job.views["b2"][0].data_ptr(), weight.data_ptr()
        a.feat, a.hid, a.w2, a.wbar = pred.df.x, pred.df.out, pred.df.w2, self.wbar.data_ptr()
        a.tgt, a.base, a.map = self.tgt.data_ptr(), self.base.data_ptr(), self.map.data_ptr()
        a.G, a.B, a.Up, a.C = G, EB, job.Up, pred.classes
        a.hs, a.ws, a.hr, a.wr = hs, ws, hr, wr
        a.Cp, a.Cr = job.final_cp, job.members[0][0].kernels_per_layer[-1]
        a.prec, a.logit, a.relu = pred.df.prec, 1 if score == "logit" else 0, 1 if relu else 0
        a.inv_n = float(np.float32(1) / np.float32(hr * wr))
        self.head = a

    def forward(self, pred, m):
        """The launches of one chunk of ``m`` images on the current stream: staging tensor -> the predictor's
        forward at ``EB`` rows -> ``map`` / ``tgt`` / ``base`` of the first ``m`` rows."""
        job, K = pred.job, pred.K
        s = job._stream()
        self.head.m = m
        job._run_fwd(s, pred.ops)
        K.check(job.L.gt_dense_fwd(pred.df, s), "dense_fwd(gradcam)")
        K.check(job.L.gt_head_gradcam(self.head, s), "head_gradcam")

    def run(self, pred, x, target):
        """``x`` [n, H, W, C] host fp32 -> ``(map [n, hr, wr], target int64 [n], base fp32 [n])`` as host arrays:
        per chunk of ``EB`` images one upload and one launch set; the results gather on the device and are read
        back once."""
        n, EB, dev = x.shape[0], pred.EB, pred.device
        with torch.cuda.device(dev):
            out = torch.empty((n, self.hr, self.wr), dtype=torch.float32, device=dev)
            tgt = torch.empty(n, dtype=torch.int32, device=dev)
            base = torch.empty(n, dtype=torch.float32, device=dev)
            for s in range(0, n, EB):
                m = min(EB, n - s)
                pred.upload(x[s:s + m])
                if target is None:
                    self.tgt.fill_(-1)               # the kernel puts the label there
                else:
                    self.tgt[:m].copy_(torch.from_numpy(target[s:s + m].astype(np.int32)).to(dev))
                self.forward(pred, m)
                out[s:s + m].copy_(self.map[:m])
                tgt[s:s + m].copy_(self.tgt[:m])
                base[s:s + m].copy_(self.base[:m])
            return out.cpu().numpy(), tgt.cpu().numpy().astype(np.int64), base.cpu().numpy()


def gradcam_state(pred, score, relu, G, weight):
    """The cached :class:`GradcamState` of a predictor (its ``_cam`` dict) for one setting."""
    key = (score, bool(relu))
    st = pred._cam.get(key)
    if st is None:
        with torch.cuda.device(pred.device):
            st = pred._cam[key] = GradcamState(pred, score, bool(relu), G, weight)
    return st


class McState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for Monte-Carlo dropout: the
    outputs of one chunk of ``EB`` rows and one argument struct of ``gt_head_mc`` over the predictor's own
    buffers (the hidden activations ``gt_dense_fwd`` wrote in evaluation mode, the fp32 masters of ``W2`` and
    ``b2``, the members' weights). The predictor's job, evaluation launches, staging tensor and ``upload`` are
    used as they are, at ``EB`` rows."""

    def __init__(self, pred, G, weight):
        K, job, EB, dev, C = pred.K, pred.job, pred.EB, pred.device, pred.classes
        self.G, self.weight = G, weight
        self.proba = torch.empty((EB, C), dtype=torch.float32, device=dev)
        self.std = torch.empty_like(self.proba)
        self.entropy = torch.empty(EB, dtype=torch.float32, device=dev)
        self.expected = torch.empty_like(self.entropy)
        self.mutual = torch.empty_like(self.entropy)
        self.label = torch.empty(EB, dtype=torch.int32, device=dev)
        self.samples = None                      # [EB][G][T][C], allocated when asked for
        a = K.HeadMcArgs()
        a.h, a.w2, a.b2, a.weight = pred.df.out, pred.df.w2, job.views["b2"][0].data_ptr(), weight.data_ptr()
        a.proba, a.std = self.proba.data_ptr(), self.std.data_ptr()
        a.entropy, a.expected_entropy = self.entropy.data_ptr(), self.expected.data_ptr()
        a.mutual_info, a.label = self.mutual.data_ptr(), self.label.data_ptr()
        a.G, a.B, a.Up, a.Ur, a.C = G, EB, job.Up, job.members[0][0].dense_units, C
        a.prec = pred.df.prec
        self.head = a

    def run(self, pred, x, samples, dropout, seed, return_samples):
        """``x`` [n, H, W, C] host fp32 -> the dict of ``predict_mc`` as host arrays: per chunk of ``EB`` images
        one upload, the evaluation launches, ``gt_dense_fwd`` and ``gt_head_mc`` with ``n0`` the chunk's offset;
        the results gather on the device and are read back once."""
        from ..utils.rng import mc_threshold
        job, K, a = pred.job, pred.K, self.head
        n, EB, dev, C, G, T = x.shape[0], pred.EB, pred.device, pred.classes, self.G, samples
        a.T, a.thr, a.seed = T, mc_threshold(dropout), seed
        a.keep_scale, a.inv_T = float(mc_keep_scale(dropout)), float(np.float32(1) / np.float32(T))
        with torch.cuda.device(dev):
            a.samples = 0
            if return_samples:
                if self.samples is None or self.samples.numel() < EB * G * T * C:
                    self.samples = torch.empty(EB * G * T * C, dtype=torch.float32, device=dev)
                a.samples = self.samples.data_ptr()
                smp = torch.empty((n, G, T, C), dtype=torch.float32, device=dev)
            proba = torch.empty((n, C), dtype=torch.float32, device=dev)
            std = torch.empty_like(proba)
            ent = torch.empty(n, dtype=torch.float32, device=dev)
            mi = torch.empty_like(ent)
            label = torch.empty(n, dtype=torch.int32, device=dev)
            for s in range(0, n, EB):
                m = min(EB, n - s)
                pred.upload(x[s:s + m])
                a.m, a.n0 = m, s
                st = job._stream()
                job._run_fwd(st, pred.ops)
                K.check(job.L.gt_dense_fwd(pred.df, st), "dense_fwd(mc)")
                K.check(job.L.gt_head_mc(a, st), "head_mc")
                proba[s:s + m].copy_(self.proba[:m])
                std[s:s + m].copy_(self.std[:m])
                ent[s:s + m].copy_(self.entropy[:m])
                mi[s:s + m].copy_(self.mutual[:m])
                label[s:s + m].copy_(self.label[:m])
                if return_samples:
                    smp[s:s + m].copy_(self.samples[:m * G * T * C].view(m, G, T, C))
            out = {"proba": proba.cpu().numpy(), "std": std.cpu().numpy(), "entropy": ent.cpu().numpy(),
                   "mutual_info": mi.cpu().numpy(),
                   "label": label.cpu().numpy().astype(np.int64)}
            if return_samples:
                out["samples"] = smp.cpu().numpy()
        return out


def mc_state(pred, G, weight):
    """The cached :class:`McState` of a predictor (its ``_mc``), built on the first request."""
    if pred._mc is None:
        with torch.cuda.device(pred.device):
            pred._mc = McState(pred, G, weight)
    return pred._mc


def nn_slices(tiles, qtiles, cus):
    """Bank slices of one ``gt_nn_topk`` launch: enough workgroups (query tiles x slices) for two per compute
    unit, at most one slice per bank tile and ``NN_MAX_SLICES``. Any value gives the same bits."""
    from ..ops.cnn_kernels import NN_MAX_SLICES
    return int(max(1, min(NN_MAX_SLICES, tiles, -(-2 * cus // qtiles))))


def nn_bank_rows(N, Dp, npl):
    """Rows of the resident bank of ``N`` rows, ``N`` rounded up to the bank tile; ``ValueError`` (before any
    forward or allocation) when its ``npl`` bf16 planes of ``Dp`` stored features pass the launchers' 1 GiB."""
    from ..ops.cnn_kernels import NN_BANK_TILE, NN_MAX_PLANE_BYTES
    Np = -(-N // NN_BANK_TILE) * NN_BANK_TILE
    if npl * Np * Dp * 2 > NN_MAX_PLANE_BYTES:
        raise ValueError("neighbors: a bank of {} rows x {} stored features takes {:.2f} GiB of planes on the "
                         "device, above the HIP path's 1 GiB; use backend=\"torch\"".format(
                             N, Dp, npl * Np * Dp * 2.0 / 2 ** 30))
    return Np


class NeighborState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for ``embed`` / ``neighbors``: a
    view of the hidden activations ``gt_dense_fwd`` writes in evaluation mode (``[G][EB][Up]``) and the argument
    structs of csrc/hip/cnn_neighbors.hip over it. The predictor's job, evaluation launches, staging tensor and
    ``upload`` are used as they are, at ``EB`` rows. The bank of a request lives for that request only."""

    FLAT_ROWS = 8192             # rows of a host bank uploaded at a time

    def __init__(self, pred, G):
        job = pred.job
        self.G, self.Up, self.Ur, self.prec = G, job.Up, job.members[0][0].dense_units, int(pred.df.prec)
        self.hidden = pred.hidden
        assert self.hidden.data_ptr() == pred.df.out and tuple(self.hidden.shape) == (G, pred.EB, self.Up)
        self.cus = torch.cuda.get_device_properties(pred.device).multi_processor_count

    def _src(self, pred):
        s = pred.K.NnSrc()
        s.h, s.G, s.B, s.Up, s.Ur, s.flat, s.ld = pred.df.out, self.G, pred.EB, self.Up, self.Ur, 0, 0
        return s

    def forward(self, pred, chunk):
        """One chunk into the staging tensor and through the evaluation launches up to the hidden rows; the
        launches' stream comes back."""
        job = pred.job
        pred.upload(chunk)
        st = job._stream()
        job._run_fwd(st, pred.ops)
        pred.K.check(job.L.gt_dense_fwd(pred.df, st), "dense_fwd(embed)")
        return st

    def embed(self, pred, x):
        """``x`` [n, H, W, C] host fp32 -> [n, G * Ur] host fp32: the real units of every member, member order."""
        n, EB = x.shape[0], pred.EB
        with torch.cuda.device(pred.device):
            out = torch.empty((n, self.G, self.Ur), dtype=torch.float32, device=pred.device)
            for s in range(0, n, EB):
                m = min(EB, n - s)
                self.forward(pred, x[s:s + m])
                out[s:s + m].copy_(self.hidden[:, :m, :self.Ur].permute(1, 0, 2))
            return out.view(n, self.G * self.Ur).cpu().numpy()

    def bank(self, pred, bank, images):
        """The resident bank of a request, ``(planes, norm, N, Np)``: per chunk of ``EB`` images the forward and
        ``gt_nn_bank`` over the hidden rows, or per ``FLAT_ROWS`` rows of host embeddings one upload and the same
        kernel over the fp32 buffer; the last launch also writes the zero rows up to ``Np``."""
        K, L, dev = pred.K, pred.job.L, pred.device
        N, Dp, npl = bank.shape[0], self.G * self.Up, 3 if self.prec else 1
        Np = nn_bank_rows(N, Dp, npl)
        planes = torch.empty((npl, Np, Dp), dtype=torch.bfloat16, device=dev)
        norm = torch.empty(Np, dtype=torch.float32, device=dev)
        a = K.NnBankArgs()
        a.planes, a.norm, a.prec, a.N, a.Np = planes.data_ptr(), norm.data_ptr(), self.prec, N, Np
        if images:
            a.src, a.sprec, step = self._src(pred), self.prec, pred.EB
        else:
            ld = -(-bank.shape[1] // 32) * 32
            step = min(self.FLAT_ROWS, N)
            buf = torch.zeros((step, ld), dtype=torch.float32, device=dev)
            s = a.src
            s.h, s.G, s.B, s.Up, s.Ur, s.flat, s.ld = buf.data_ptr(), self.G, step, self.Up, self.Ur, 1, ld
            a.sprec = 1
        for s0 in range(0, N, step):
            m = min(step, N - s0)
            if images:
                st = self.forward(pred, bank[s0:s0 + m])
            else:
                buf[:m, :bank.shape[1]].copy_(torch.from_numpy(bank[s0:s0 + m]).to(dev))
                st = pred.job._stream()
            a.m, a.n0, a.rows = m, s0, (Np - s0 if s0 + m == N else m)
            K.check(L.gt_nn_bank(a, st), "nn_bank")
        return planes, norm, N, Np

    def run(self, pred, x, bank, images, k, metric, slices=None):
        """``(index int64 [n, k], distance fp32 [n, k])`` of validated arguments: the bank, then per chunk of
        ``EB`` queries the forward, ``gt_nn_topk`` over ``slices`` bank slices (:func:`nn_slices` unless given)
        and ``gt_nn_merge`` into the request's results, which are read back once."""
        K, L, dev, EB = pred.K, pred.job.L, pred.device, pred.EB
        n = x.shape[0]
        with torch.cuda.device(dev):
            planes, norm, N, Np = self.bank(pred, bank, images)
            S = nn_slices(Np // K.NN_BANK_TILE, EB // 32, self.cus) if slices is None else int(slices)
            cand_d = torch.empty((EB, S, k), dtype=torch.float32, device=dev)
            cand_i = torch.empty((EB, S, k), dtype=torch.int32, device=dev)
            idx = torch.empty((n, k), dtype=torch.int32, device=dev)
            dist = torch.empty((n, k), dtype=torch.float32, device=dev)
            t = K.NnTopkArgs()
            t.q, t.planes, t.bnorm = self._src(pred), planes.data_ptr(), norm.data_ptr()
            t.cand_d, t.cand_i = cand_d.data_ptr(), cand_i.data_ptr()
            t.prec, t.N, t.Np, t.k, t.S, t.metric = self.prec, N, Np, k, S, NN_METRICS.index(metric)
            g = K.NnMergeArgs()
            g.cand_d, g.cand_i, g.S, g.k = t.cand_d, t.cand_i, S, k
            for s in range(0, n, EB):
                m = min(EB, n - s)
                st = self.forward(pred, x[s:s + m])
                t.m = g.m = m
                g.out_d, g.out_i = dist[s:].data_ptr(), idx[s:].data_ptr()
                K.check(L.gt_nn_topk(t, st), "nn_topk")
                K.check(L.gt_nn_merge(g, st), "nn_merge")
            return idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()


def neighbor_state(pred, G):
    """The cached :class:`NeighborState` of a predictor (its ``_nn``), built on the first request."""
    if pred._nn is None:
        with torch.cuda.device(pred.device):
            pred._nn = NeighborState(pred, G)
    return pred._nn


def gaussian_check_hip(C):
    """The ``ValueError`` of more classes than ``gt_fs_sums`` / ``gt_fs_dist`` take, before a predictor is built."""
    from ..ops.cnn_kernels import FS_MAX_CLASSES
    if C > FS_MAX_CLASSES:
        raise ValueError("the HIP Gaussian kernels take at most {} classes, got {}; use backend=\"torch\"".format(
            FS_MAX_CLASSES, C))


def fs_store_rows(N, G, Up):
    """Rows of the feature store of a fit of ``N`` rows, ``N`` rounded up to ``FS_ROW_PAD``; ``ValueError`` (before
    any forward or allocation) when ``G x rows x Up`` fp32 values pass the launchers' 1 GiB."""
    from ..ops.cnn_kernels import FS_MAX_STORE_BYTES, FS_ROW_PAD
    Np = -(-N // FS_ROW_PAD) * FS_ROW_PAD
    if G * Np * Up * 4 > FS_MAX_STORE_BYTES:
        raise ValueError("gaussian_fit: {} rows x {} stored features take {:.2f} GiB on the device, above the HIP "
                         "path's 1 GiB; use backend=\"torch\"".format(N, G * Up, G * Np * Up * 4.0 / 2 ** 30))
    return Np


class GaussianState(object):
    """What a HIP predictor adds for ``gaussian_fit`` / ``mahalanobis``: the argument structs of
    csrc/hip/cnn_gaussian.hip over the hidden rows of the predictor's :class:`NeighborState`, whose forward and
    source view are used as they are. The feature store, the planes and the partials of a fit live for that
    request only."""

    PART_BYTES = 256 << 20       # fp32 scatter partials held at a time: the slices of one round

    def __init__(self, pred, G):
        self.nn = neighbor_state(pred, G)

    def fit(self, pred, bank, images, labels, C):
        """``(count int64 [C], mean fp32 [G, C, Ur], cov fp64 [G, Ur, Ur])`` of validated arguments: the bank's
        hidden rows into the store (or the embeddings uploaded as they are), ``gt_fs_sums`` and the means on the
        host, ``gt_fs_center``, then rounds of ``gt_fs_scatter`` + ``gt_fs_reduce``."""
        K, L, dev, nn = pred.K, pred.job.L, pred.device, self.nn
        G, Up, Ur, N = nn.G, nn.Up, nn.Ur, bank.shape[0]
        Np = fs_store_rows(N, G, Up)
        S = -(-N // K.FS_SLICE_ROWS)
        count = np.bincount(labels, minlength=C).astype(np.int64)
        with torch.cuda.device(dev):
            src = K.NnSrc()
            if images:
                store = torch.empty((G, Np, Up), dtype=nn.hidden.dtype, device=dev)
                for s0 in range(0, N, pred.EB):
                    m = min(pred.EB, N - s0)
                    nn.forward(pred, bank[s0:s0 + m])
                    store[:, s0:s0 + m].copy_(nn.hidden[:, :m])
                src.h, src.G, src.B, src.Up, src.Ur, src.flat, src.ld = store.data_ptr(), G, Np, Up, Ur, 0, 0
                sprec = nn.prec
            else:
                store = torch.from_numpy(bank).to(dev)
                src.h, src.G, src.B, src.Up, src.Ur, src.flat, src.ld = store.data_ptr(), G, N, Up, Ur, 1, G * Ur
                sprec = 1
            st = pred.job._stream()
            lab = torch.from_numpy(labels.astype(np.int32)).to(dev)
            part = torch.empty((S, G, C, Up), dtype=torch.float64, device=dev)
            a = K.FsSumsArgs()
            a.src, a.label, a.part, a.sprec, a.N, a.C = src, lab.data_ptr(), part.data_ptr(), sprec, N, C
            K.check(L.gt_fs_sums(a, st), "fs_sums")
            sums = np.zeros((G, C, Up))
            for p in part.cpu().numpy():                     # slice order
                sums += p
            mean = (sums / np.maximum(count, 1)[None, :, None]).astype(np.float32)
            mean_d = torch.from_numpy(mean).to(dev)
            planes = torch.empty((3, G, Up, Np), dtype=torch.bfloat16, device=dev)
            c = K.FsCenterArgs()
            c.src, c.label, c.mean, c.planes = src, lab.data_ptr(), mean_d.data_ptr(), planes.data_ptr()
            c.sprec, c.N, c.Np, c.C = sprec, N, Np, C
            K.check(L.gt_fs_center(c, st), "fs_center")
            slices = -(-Np // K.FS_SLICE_ROWS)
            per = int(max(1, min(slices, self.PART_BYTES // (G * Up * Up * 4))))
            buf = torch.empty((per, G, Up, Up), dtype=torch.float32, device=dev)
            acc = torch.empty((G, Up, Up), dtype=torch.float64, device=dev)
            t, r = K.FsScatterArgs(), K.FsReduceArgs()
            t.planes, t.part, t.G, t.Up, t.Np = planes.data_ptr(), buf.data_ptr(), G, Up, Np
            r.part, r.acc, r.G, r.Up = buf.data_ptr(), acc.data_ptr(), G, Up
            for s0 in range(0, slices, per):
                t.s0, t.ns = s0, min(per, slices - s0)
                r.ns, r.first, r.last = t.ns, int(s0 == 0), int(s0 + t.ns == slices)
                K.check(L.gt_fs_scatter(t, st), "fs_scatter")
                K.check(L.gt_fs_reduce(r, st), "fs_reduce")
            cov = acc[:, :Ur, :Ur].cpu().numpy() / N
        return count, np.ascontiguousarray(mean[:, :, :Ur]), np.ascontiguousarray(cov)

    def distance(self, pred, x, st, C):
        """fp32 ``[G, n, C]`` of validated arguments: the planes of ``W^T`` and the whitened means once, then per
        chunk of ``EB`` images the forward and ``gt_fs_dist`` into the request's result, read back once."""
        K, L, dev, nn = pred.K, pred.job.L, pred.device, self.nn
        G, Up, Ur, n = nn.G, nn.Up, nn.Ur, x.shape[0]
        with torch.cuda.device(dev):
            wt = torch.zeros((G, Up, Up), dtype=torch.float32, device=dev)
            wt[:, :Ur, :Ur].copy_(torch.from_numpy(st["whiten"]).to(dev).transpose(1, 2))
            planes = torch.empty((3, G, Up, Up), dtype=torch.bfloat16, device=dev)
            for p in range(3):                               # the exact split of common.h: wt = p0 + p1 + p2
                planes[p].copy_(wt)
                wt -= planes[p].float()
            tm = torch.zeros((G, C, Up), dtype=torch.float32, device=dev)
            tm[:, :, :Ur].copy_(torch.from_numpy(st["wmean"]).to(dev))
            out = torch.empty((G, n, C), dtype=torch.float32, device=dev)
            a = K.FsDistArgs()
            a.q, a.wt, a.wmean, a.out = nn._src(pred), planes.data_ptr(), tm.data_ptr(), out.data_ptr()
            a.sprec, a.C, a.ldo = nn.prec, C, n
            a.empty = int(sum(1 << c for c in range(C) if st["count"][c] == 0))
            for s in range(0, n, pred.EB):
                a.m, a.r0 = min(pred.EB, n - s), s
                K.check(L.gt_fs_dist(a, nn.forward(pred, x[s:s + a.m])), "fs_dist")
            return out.cpu().numpy()


def gaussian_state(pred, G):
    """The cached :class:`GaussianState` of a predictor (its ``_gauss``), built on the first request."""
    if pred._gauss is None:
        with torch.cuda.device(pred.device):
            pred._gauss = GaussianState(pred, G)
    return pred._gauss


def saliency_info(res, method):
    """The ``return_info`` dict of ``(map, target, base, baseline_score)``."""
    info = {"target": res[1], "base": res[2]}
    if method == "integrated":
        info["baseline_score"] = res[3]
    return info


class SaliencyState(object):
    """What a HIP predictor (``HipPredictor`` or ``HipEnsemblePredictor``) adds for input-gradient saliency: an
    evaluation-mode backward chain over the predictor's own activations, down to the staging tensor.

    * the masked forward: copies of the predictor's evaluation launches with the pool argmax masks switched back
      on (``pmask`` twins at ``EB`` rows, in the fused conv / BN-apply epilogues and the separate pool launch);
      the activations are the plain forward's, byte for byte;
    * ``gt_head_saliency``: label, base score and ``dH`` of every member;
    * the job's own backward records (``bwd_ops``) without the weight gradients: ``gt_dense_dgrad`` and every
      data-gradient / pool-backward launch copied with its pointers remapped to gradient twins at ``EB`` rows,
      the fused un-pools kept, ``gt_bn_bwd_eval`` in place of each BatchNorm backward;
    * ``gt_conv_in_dgrad``, the data gradient of the input conv, then ``gt_ig_reduce``.

    One stream, no graph. The gradient twins and masks double the predictor's twin footprint. The predictor's
    job, evaluation launches, staging tensor and ``upload`` are used as they are."""

    def __init__(self, pred, G, weight):
        K, job, EB, dev = pred.K, pred.job, pred.EB, pred.device
        Q = job.Q
        self.G, self.weight = G, weight
        rows, remap = job._eval_remap                # the activation twins of the predictor's own evaluation launches
        remap = dict(remap)
        must = [t.data_ptr() for t in list(job.act.values()) + list(job.zpre.values()) + [job.hdrop]]
        if rows != EB or any(p not in remap for p in must):
            raise RuntimeError("saliency: the predictor's evaluation launches have no twin of some activation")
        self.grad = {}
        for name, t in job.grad.items():
            e = self.grad[name] = torch.zeros((Q, EB) + tuple(t.shape[2:]), dtype=t.dtype, device=dev)
            remap[t.data_ptr()] = e.data_ptr()
        self.pmask = []
        for st in job.stages:
            e = torch.zeros((Q * EB,) + tuple(st.pmask.shape[1:]), dtype=torch.uint8, device=dev)
            self.pmask.append(e)
            remap[st.pmask.data_ptr()] = e.data_ptr()

        small = set(t.data_ptr() for t in list(job.grad.values()) + [st.pmask for st in job.stages]) | set(must)

        def rp(ptr):
            """A training-batch buffer -> its twin at ``EB`` rows (a missing twin is an error, never a launch over
            the short buffer); the dataset, parameters and tables stay."""
            ptr = ptr or 0
            if ptr in small and ptr not in remap:
                raise RuntimeError("saliency: no twin at {} rows for the buffer at {:#x}".format(EB, ptr))
            return remap.get(ptr, ptr)
        # ---- masked forward
        self.fwd_ops = []
        for (kind, a, mk), (_, b, _) in zip(job.fwd_ops, pred.ops):
            if kind == "conv":
                c = K.ConvArgs.from_buffer_copy(b)
                c.pool_mask = rp(a.pool_mask)
                self.fwd_ops.append((kind, c, None))
            elif kind == "bn":
                c = K.BnArgs.from_buffer_copy(b)
                c.pool_mask = rp(a.pool_mask)
                self.fwd_ops.append((kind, c, None))
            else:
                self.fwd_ops.append((kind, b, rp(mk)))
        # ---- head and dense data gradient
        self.tgt = torch.full((EB,), -1, dtype=torch.int32, device=dev)
        self.base = torch.empty(EB, dtype=torch.float32, device=dev)
        self.dH = torch.zeros((Q, EB, job.Up), dtype=torch.float32, device=dev)
        self.dHp = torch.zeros((job.npl, Q, EB, job.Up), dtype=torch.int16, device=dev)
        h = K.HeadSaliencyArgs()
        h.plog, h.b2, h.weight = pred.df.plog, job.views["b2"][0].data_ptr(), weight.data_ptr()
        h.hid, h.w2 = pred.df.out, pred.df.w2
        h.tgt, h.base, h.dH, h.dHp = (self.tgt.data_ptr(), self.base.data_ptr(), self.dH.data_ptr(),
                                      self.dHp.data_ptr())
        h.G, h.B, h.Up, h.C, h.prec = G, EB, job.Up, pred.classes, pred.df.prec
        self.head = h
        dd = K.DenseDgradArgs.from_buffer_copy(job.dense_dgrad_args)
        dd.dH, dd.dHp, dd.dx, dd.B = self.dH.data_ptr(), self.dHp.data_ptr(), rp(dd.dx), EB
        dd.unpool_mask, dd.unpool_x0, dd.unpool_x1 = rp(dd.unpool_mask), rp(dd.unpool_x0), rp(dd.unpool_x1)
        self.dd = dd
        # ---- the backward chain
        self.bwd = []
        for kind, a, L in job.bwd_ops:
            if kind == "conv":
                c = K.ConvArgs.from_buffer_copy(a)
                for i in range(K.MAXSLOT):
                    c.inp[i], c.out[i], c.out_mask[i] = rp(c.inp[i]), rp(c.out[i]), rp(c.out_mask[i])
                c.pool_y, c.pool_mask, c.unpool_x1 = rp(c.pool_y), rp(c.pool_mask), rp(c.unpool_x1)
                c.st, c.B = job.eval_state.data_ptr(), EB
                job._set_twopass(c)
                if L.slots[0] in job.unpool_fused and not job.L.gt_conv_fast_probe_any(c):
                    raise RuntimeError("saliency: no kernel un-pools the gradient of {} at {} rows".format(
                        L.slots[0], EB))
                self.bwd.append(("conv", c))
            elif kind == "pool_bwd":
                pm, sel, gp, g0, g1, _qb, _b, hh, ww, cc, one, prec = a
                self.bwd.append(("pool_bwd", (rp(pm), sel, rp(gp), rp(g0), rp(g1), Q * EB, EB, hh, ww, cc, one, prec)))
            elif kind == "bn_bwd":
                b = K.BnBwdEvalArgs()
                b.dy, b.gamma, b.run = self.grad[L.name].data_ptr(), L.gamma[0].data_ptr(), L.bn_run.data_ptr()
                b.G, b.B, b.H, b.W, b.Cp, b.Cr = Q, EB, L.H, L.W, L.coutp, L.cout
                b.Hr, b.Wr = (L.Hr, L.Wr) if job.pad_hw is not None else (L.H, L.W)
                b.chunk_px = L.bn_chunk
                b.nchunk = -(-(EB * L.H * L.W) // L.bn_chunk)
                b.eps, b.prec = job.cfg.bn_eps, job.prec
                self.bwd.append(("bn_bwd", b))
        # ---- the input conv's data gradient and the finishing kernel
        L0 = job.stages[0].layers[0]
        stage = pred.stage
        self.dx = torch.zeros((Q, EB) + tuple(stage.shape[1:]), dtype=torch.float32, device=dev)
        ci = K.ConvInDgradArgs()
        ci.dz, ci.w, ci.dx = self.grad[L0.name].data_ptr(), L0.w[0].data_ptr(), self.dx.data_ptr()
        ci.G, ci.B, ci.Hp, ci.Wp = Q, EB, L0.H, L0.W
        ci.Hr, ci.Wr = pred.hwc[0], pred.hwc[1]
        ci.Coutp, ci.Cout, ci.C8, ci.Cr, ci.KH, ci.KW, ci.prec = L0.coutp, L0.cout, L0.cinp, L0.cin, L0.KH, L0.KW, job.prec
        self.cin = ci
        h_, w_, c_ = pred.hwc
        self.raw = torch.zeros_like(stage)                       # the images of an integrated-gradients chunk
        self.x0 = torch.zeros(int(stage.shape[3]), dtype=torch.float32, device=dev)
        self.out = torch.empty(EB * h_ * w_ * c_, dtype=torch.float32, device=dev)
        r = K.IgReduceArgs()
        r.dx, r.x0, r.weight, r.out = self.dx.data_ptr(), self.x0.data_ptr(), weight.data_ptr(), self.out.data_ptr()
        r.G, r.B = G, EB
        r.Hp, r.Wp, r.Hr, r.Wr, r.Cr = int(stage.shape[1]), int(stage.shape[2]), h_, w_, c_
        r.prec = 1 if stage.dtype == torch.float32 else 0
        self.red = r
        p = K.IgPointsArgs()
        p.raw, p.out, p.x0, p.rows = self.raw.data_ptr(), stage.data_ptr(), self.x0.data_ptr(), EB
        p.Hp, p.Wp, p.Hr, p.Wr, p.Cr, p.prec = r.Hp, r.Wp, h_, w_, c_, r.prec
        self.pts = p
        # ---- smooth=: the per-row sigma, gt_sg_points in place of gt_ig_points, gt_sg_reduce in place of gt_ig_reduce
        self.sigma = torch.zeros(EB, dtype=torch.float32, device=dev)
        sp = K.SgPointsArgs()
        sp.raw, sp.out, sp.sigma, sp.rows = self.raw.data_ptr(), stage.data_ptr(), self.sigma.data_ptr(), EB
        sp.Hp, sp.Wp, sp.Hr, sp.Wr, sp.Cr, sp.prec = r.Hp, r.Wp, h_, w_, c_, r.prec
        self.sg_pts = sp
        sr = K.SgReduceArgs()
        sr.dx, sr.x, sr.weight, sr.out = self.dx.data_ptr(), self.raw.data_ptr(), weight.data_ptr(), self.out.data_ptr()
        sr.G, sr.B = G, EB
        sr.Hp, sr.Wp, sr.Hr, sr.Wr, sr.Cr, sr.prec = r.Hp, r.Wp, h_, w_, c_, r.prec
        self.sg_red = sr

    def forward(self, pred, rows, logit):
        """Masked forward and head of the staging tensor on the current stream: ``tgt`` / ``base`` / ``dH`` of the
        first ``rows`` rows."""
        job, K = pred.job, pred.K
        s = job._stream()
        self.head.m, self.head.logit = rows, logit
        job._run_fwd(s, self.fwd_ops)
        K.check(job.L.gt_dense_fwd(pred.df, s), "dense_fwd(saliency)")
        K.check(job.L.gt_head_saliency(self.head, s), "head_saliency")

    def backward(self, pred, rows):
        """``dH`` -> ``dx`` of the first ``rows`` rows: the dense data gradient, the remapped chain and the input
        conv's data gradient, on the current stream."""
        job, K = pred.job, pred.K
        L, s = job.L, job._stream()
        K.check(L.gt_dense_dgrad(self.dd, s), "dense_dgrad(saliency)")
        for kind, a in self.bwd:
            if kind == "conv":
                K.check(L.gt_conv_fwd(a, s), "conv_dgrad(saliency)")
            elif kind == "bn_bwd":
                K.check(L.gt_bn_bwd_eval(a, s), "bn_bwd_eval")
            else:
                K.check(L.gt_pool_bwd_mask(*a, s), "pool_bwd(saliency)")
        self.cin.m = rows
        K.check(L.gt_conv_in_dgrad(self.cin, s), "conv_in_dgrad")

    def reduce(self, pred, x, R, m, method, reduce):
        """``gt_ig_reduce`` of ``R`` raw rows whose images are the first rows of ``x``."""
        r = self.red
        r.x, r.R, r.m = x.data_ptr(), R, m
        r.method, r.reduce = SAL_METHODS.index(method), {None: 0, "absmax": 1, "sum": 2}[reduce]
        r.inv_m = float(np.float32(1) / np.float32(m))
        pred.K.check(pred.job.L.gt_ig_reduce(r, pred.job._stream()), "ig_reduce")

    def _set_targets(self, target, s, m):
        if target is None:
            self.tgt.fill_(-1)                   # the kernel puts the label there
        else:
            self.tgt[:m].copy_(torch.from_numpy(target[s:s + m].astype(np.int32)).to(self.tgt.device))

    def run_smooth(self, pred, x, target, score, method, reduce, smooth):
        """:meth:`run` with ``smooth`` (:func:`smooth_spec`'s tuple): per chunk of ``R = EB // S`` images one
        upload, a forward of the clean images (label and base score), ``gt_sg_points``, one launch set over the
        ``S * R`` points and ``gt_sg_reduce``; a short last chunk runs ``S * mm`` points only."""
        S, noise, seed, stat = smooth
        n, EB, dev, K = x.shape[0], pred.EB, pred.device, pred.K
        h, w, c = pred.hwc
        logit = 1 if score == "logit" else 0
        per = h * w * (c if reduce is None else 1)
        R = EB // S
        sigma = torch.from_numpy(smooth_sigma(x, noise))
        sp, sr = self.sg_pts, self.sg_red
        sp.S, sp.seed = S, seed
        sr.S, sr.inv_s = S, float(np.float32(1) / np.float32(S))
        sr.stat, sr.method = SG_STATS.index(stat), SG_METHODS.index(method)
        sr.reduce = {None: 0, "absmax": 1, "sum": 2}[reduce]
        with torch.cuda.device(dev):
            out = torch.empty(n * per, dtype=torch.float32, device=dev)
            tgt = torch.empty(n, dtype=torch.int32, device=dev)
            base = torch.empty(n, dtype=torch.float32, device=dev)
            for s in range(0, n, R):
                mm = min(R, n - s)
                pred.upload(x[s:s + mm])
                self._set_targets(target, s, mm)
                self.forward(pred, mm, logit)                            # label and base score of the clean images
                tgt[s:s + mm].copy_(self.tgt[:mm])
                base[s:s + mm].copy_(self.base[:mm])
                self.raw[:mm].copy_(pred.stage[:mm])
                self.tgt[:S * mm].copy_(self.tgt[:mm].repeat(S))         # row k * mm + r: the target of image r
                self.sigma[:mm].copy_(sigma[s:s + mm].to(dev))
                sp.R, sp.n0, sr.R = mm, s, mm
                K.check(pred.job.L.gt_sg_points(sp, pred.job._stream()), "sg_points")
                self.forward(pred, S * mm, logit)
                self.backward(pred, S * mm)
                K.check(pred.job.L.gt_sg_reduce(sr, pred.job._stream()), "sg_reduce")
                out[s * per:(s + mm) * per].copy_(self.out[:mm * per])
            shape = (n, h, w, c) if reduce is None else (n, h, w)
            return (out.cpu().numpy().reshape(shape), tgt.cpu().numpy().astype(np.int64), base.cpu().numpy(), None)

    def run(self, pred, x, target, score, method, steps, x0, reduce, smooth=None):
        """``x`` [n, H, W, C] host fp32 -> ``(map, target int64 [n], base fp32 [n], baseline_score or None)`` as
        host arrays. ``"gradient"`` / ``"gradxinput"``: per chunk of ``EB`` images one upload and one launch set.
        ``"integrated"``: per chunk of ``R = EB // steps`` images one upload, a forward of the images themselves
        (label and base score), ``gt_ig_points`` and one launch set over the ``steps * R`` points; one more
        forward per call scores the baseline. Results gather on the device and are read back once. ``smooth``:
        :meth:`run_smooth`."""
        if smooth is not None:
            return self.run_smooth(pred, x, target, score, method, reduce, smooth)
        n, EB, dev = x.shape[0], pred.EB, pred.device
        h, w, c = pred.hwc
        logit = 1 if score == "logit" else 0
        per = h * w * (c if reduce is None else 1)
        ig = method == "integrated"
        m = steps if ig else 1
        R = EB // m if ig else EB
        with torch.cuda.device(dev):
            out = torch.empty(n * per, dtype=torch.float32, device=dev)
            tgt = torch.empty(n, dtype=torch.int32, device=dev)
            base = torch.empty(n, dtype=torch.float32, device=dev)
            bscore = None
            self.x0.zero_()
            if ig:
                f = torch.zeros(int(pred.stage.shape[3]), dtype=torch.float32)
                f[:c] = torch.from_numpy(x0)
                self.x0.copy_(f.to(pred.stage.dtype).float().to(dev))    # rounded to the staging type on the host
                C = pred.classes                                         # s(x0) of every class: row k, target k
                pred.upload(np.broadcast_to(self.x0[:c].cpu().numpy(), (C, h, w, c)).copy())
                self.tgt[:C].copy_(torch.arange(C, dtype=torch.int32, device=dev))
                self.forward(pred, C, logit)
                bscore = self.base[:C].clone()
                self.pts.m = m
                for k, al in enumerate(ig_alphas(m)):
                    self.pts.alpha[k] = float(al)
            for s in range(0, n, R):
                mm = min(R, n - s)
                pred.upload(x[s:s + mm])
                self._set_targets(target, s, mm)
                rows = mm
                if ig:                                                   # a short last chunk runs m * mm points only
                    self.forward(pred, mm, logit)                        # label and base score of the images
                    tgt[s:s + mm].copy_(self.tgt[:mm])
                    base[s:s + mm].copy_(self.base[:mm])
                    self.raw[:mm].copy_(pred.stage[:mm])
                    self.tgt[:m * mm].copy_(self.tgt[:mm].repeat(m))     # row k * mm + r: the target of image r
                    self.pts.R = mm
                    pred.K.check(pred.job.L.gt_ig_points(self.pts, pred.job._stream()), "ig_points")
                    rows = m * mm
                self.forward(pred, rows, logit)
                self.backward(pred, rows)
                self.reduce(pred, self.raw if ig else pred.stage, mm, m, method, reduce)
                out[s * per:(s + mm) * per].copy_(self.out[:mm * per])
                if not ig:
                    tgt[s:s + mm].copy_(self.tgt[:mm])
                    base[s:s + mm].copy_(self.base[:mm])
            t = tgt.cpu().numpy().astype(np.int64)
            shape = (n, h, w, c) if reduce is None else (n, h, w)
            return (out.cpu().numpy().reshape(shape), t, base.cpu().numpy(),
                    None if bscore is None else bscore.cpu().numpy()[t])


def saliency_state(pred, G, weight):
    """The cached :class:`SaliencyState` of a predictor (its ``_sal``), built on the first request."""
    if pred._sal is None:
        with torch.cuda.device(pred.device):
            pred._sal = SaliencyState(pred, G, weight)
    return pred._sal


class HipPredictor(object):
    """Forward-only HIP launches of one fitted model at ``EB`` rows per launch.

    Hosted on a one-group ``HipPopJob`` built over a staging tensor of ``EB`` zero images in the
    executor's dataset layout: the job supplies the padded geometry, the parameter buffers and the
    evaluation launches (``_build_eval_ops``: batch ``EB``, running statistics, no pool masks) with the
    gather table ``arange(EB)``; it is never initialised, trained or captured. Each chunk of the input
    is written into the staging tensor (a short tail is filled with zero images) and
    ``gt_head_predict`` ends the chain. Independent of the number of rows predicted, so one predictor
    serves every ``predict`` call of its (device, ``EB``)."""

    def __init__(self, clf, device, EB):
        from ..ops import cnn_kernels as K
        from . import cnn_engine as E
        from .cnn_hip import HipPopJob
        self.K, self.EB, self.device, self.classes = K, int(EB), torch.device(device), clf.classes
        if self.EB % 32 or not 32 <= self.EB <= 256:
            raise ValueError("rows per launch must be a multiple of 32 in [32, 256]")
        h, w, c = clf.input_shape
        cfg = E.TrainConfig(epochs=(1,), learning_rate=(0.0,), batch_size=32, dropout=0.0, loss=clf.loss,
                            dtype=clf.dtype, use_graph=False, batch_norm=clf.batch_norm, bn_eps=clf.bn_eps)
        rows = np.arange(self.EB)
        x0 = np.zeros((self.EB, h, w, c), np.float32)
        y0 = np.zeros((self.EB, clf.classes), np.float32)
        cache = list(E._DATA_CACHE)              # the staging tensor is this predictor's alone: it neither
        try:                                     # stays in the dataset cache nor evicts a training set
            job = HipPopJob(clf.plan, x0, y0, [(rows, rows)], cfg, self.device, fold_ids=[0])
        finally:
            E._DATA_CACHE[:] = cache
        self.job = job
        self.stage = job.data.x                  # [EB][Hp][Wp][C8], fp32 (nhwc8f) or bf16 (nhwc8)
        self.hwc = (h, w, c)
        with torch.cuda.device(self.device):
            clf.load_into(job, 0)
            self.ops, self.df, _, self._keep = job._build_eval_ops(self.EB)
            self.hidden = job._eval_hidden       # [1][EB][Up], what gt_dense_fwd writes
            self.gather = torch.arange(self.EB, dtype=torch.int64, device=self.device)
            for kind, b, _ in self.ops:
                if kind == "conv" and b.gather:
                    b.gather = self.gather.data_ptr()
            self.logits = torch.empty((1, self.EB, clf.classes), dtype=torch.float32, device=self.device)
            self.proba = torch.empty_like(self.logits)
            hp = K.HeadPredictArgs()
            hp.plog, hp.b2 = self.df.plog, job.views["b2"][0].data_ptr()
            hp.logits, hp.proba = self.logits.data_ptr(), self.proba.data_ptr()
            hp.G, hp.B, hp.Up, hp.C = 1, self.EB, job.Up, clf.classes
            self.head = hp
        self._tta = {}               # views -> TtaState, created on first use
        self._occ = {}               # (patch, stride, fill, score) -> OcclusionState, created on first use
        self._rise = {}              # (masks, cells, p, seed, fill, score) -> RiseState, created on first use
        self._one = None             # the one member's weight 1.0 on the device, for the occlusion head
        self._cam = {}               # (score, relu) -> GradcamState, created on first use
        self._cam_wbar = None        # W1 summed over the real pixels (cam_wbar), on the first Grad-CAM request
        self._mc = None              # McState, created on the first Monte-Carlo dropout request
        self._sal = None             # SaliencyState, created on the first saliency request
        self._nn = None              # NeighborState, created on the first embed / neighbors request
        self._gauss = None           # GaussianState, created on the first gaussian_fit / mahalanobis request

    def forward(self):
        """The launches of one chunk on the current stream: staging tensor -> ``logits`` / ``proba``."""
        job, K = self.job, self.K
        s = job._stream()
        job._run_fwd(s, self.ops)
        K.check(job.L.gt_dense_fwd(self.df, s), "dense_fwd(predict)")
        K.check(job.L.gt_head_predict(self.head, s), "head_predict")

    def upload(self, chunk):
        """``chunk`` [m <= EB, H, W, C] host fp32 into the staging tensor; rows past ``m`` become zero images."""
        m = chunk.shape[0]
        h, w, c = self.hwc
        if m < self.EB:
            self.stage[m:].zero_()
        self.stage[:m, :h, :w, :c].copy_(torch.from_numpy(chunk).to(self.device))

    def tta_state(self, views):
        """The cached :class:`TtaState` of a view tuple: one member of weight 1.0 (``1.0f * p`` is ``p``)."""
        st = self._tta.get(views)
        if st is None:
            with torch.cuda.device(self.device):
                one = torch.ones(1, dtype=torch.float32, device=self.device)
                st = self._tta[views] = TtaState(self, views, 1, one)
        return st

    def occlusion(self, x, target, patch, stride, fill, score):
        """``(map, target, base)`` of validated arguments (``CnnClassifier.occlusion``): one member of weight
        1.0 (``1.0f * p`` is ``p``)."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        return occlusion_state(self, patch, stride, fill, score, 1, self._one).run(self, x, target)

    def rise(self, x, target, masks, cells, p, seed, fill, score):
        """``(map, target, base)`` of validated arguments (``CnnClassifier.rise``): one member of weight 1.0
        (``1.0f * p`` is ``p``)."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        return rise_state(self, masks, cells, p, seed, fill, score, 1, self._one).run(self, x, target)

    def gradcam(self, x, target, score, relu):
        """``(map, target, base)`` of validated arguments (``CnnClassifier.gradcam``): one member of weight 1.0
        (``1.0f * v`` is ``v``)."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        return gradcam_state(self, score, relu, 1, self._one).run(self, x, target)

    def predict_mc(self, x, samples, dropout, seed, return_samples):
        """The dict of validated arguments (``CnnClassifier.predict_mc``): one member of weight 1.0."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        return mc_state(self, 1, self._one).run(self, x, samples, dropout, seed, return_samples)

    def saliency(self, x, target, score, method, steps, x0, reduce, smooth=None):
        """``(map, target, base, baseline_score)`` of validated arguments (``CnnClassifier.saliency``): one member
        of weight 1.0 (``1.0f * v`` is ``v``)."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        return saliency_state(self, 1, self._one).run(self, x, target, score, method, steps, x0, reduce, smooth)

    def run(self, x, views=None):
        """``x`` [n, H, W, C] host fp32 -> (logits, proba) host fp32 ``[n, classes]``; with ``views`` (a tuple
        of ``(dy, dx, flip)``) the means over those views of every row, ``EB // len(views)`` rows per launch."""
        n, EB = x.shape[0], self.EB
        logits = torch.empty((n, self.classes), dtype=torch.float32, device=self.device)
        proba = torch.empty_like(logits)
        if views is not None:
            st = self.tta_state(tuple(views))
            R = st.R
            with torch.cuda.device(self.device):
                if st.V * R < EB:
                    self.stage[st.V * R:].zero_()            # rows no view is written to
                for s in range(0, n, R):
                    m = min(R, n - s)
                    st.upload(x[s:s + m], self.hwc)
                    st.forward(self, True, "predict")
                    logits[s:s + m].copy_(st.logits[0, :m])
                    proba[s:s + m].copy_(st.proba[0, :m])
                return logits.cpu().numpy(), proba.cpu().numpy()
        with torch.cuda.device(self.device):
            for s in range(0, n, EB):
                m = min(EB, n - s)
                self.upload(x[s:s + m])
                self.forward()
                logits[s:s + m].copy_(self.logits[0, :m])
                proba[s:s + m].copy_(self.proba[0, :m])
            return logits.cpu().numpy(), proba.cpu().numpy()
