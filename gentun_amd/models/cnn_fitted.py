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
        self._one = None             # the one member's weight 1.0 on the device, for the occlusion head
        self._cam = {}               # (score, relu) -> GradcamState, created on first use
        self._cam_wbar = None        # W1 summed over the real pixels (cam_wbar), on the first Grad-CAM request

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

    def gradcam(self, x, target, score, relu):
        """``(map, target, base)`` of validated arguments (``CnnClassifier.gradcam``): one member of weight 1.0
        (``1.0f * v`` is ``v``)."""
        if self._one is None:
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        return gradcam_state(self, score, relu, 1, self._one).run(self, x, target)

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
