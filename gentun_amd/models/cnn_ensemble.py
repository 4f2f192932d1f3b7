"""``CnnEnsemble`` -- the top few networks of a Genetic-CNN search, fitted and served together.

A search ends with a population whose best individuals sit close together; the ensemble averages the
class probabilities of ``k`` fitted :class:`~gentun_amd.models.cnn_fitted.CnnClassifier` members of one
search space (weighted mean, in member order, every multiply and add rounded to fp32) and counts their
votes. It predicts on

* the CPU, or any torch device with ``backend="torch"``: each member's stock-torch forward, combined in
  numpy fp32;
* an MI355X: :class:`HipEnsemblePredictor`, ONE ``k``-group ``HipPopJob`` whose groups are the members
  (the executor's superset network: one launch per layer serves all of them), ending in
  ``gt_head_ensemble`` (csrc/hip/cnn_dense.hip), which writes the members' logits and probabilities on
  request and always their weighted mean and votes, so member probabilities never pass through the host.

:func:`fit_ensemble` trains the members on every row -- on the HIP executor as one population job with one
group per member, each bit-identical to ``GeneticCnnModel.fit()`` of that genome alone -- and
:func:`top_genomes` picks the genomes from an evaluated population. One ``.npz`` (``gentun-cnn-ensemble/1``)
holds the whole ensemble; every member stays an ordinary ``CnnClassifier``.
"""

import json
import math

import numpy as np
import torch

from .cnn_fitted import (CnnClassifier, TtaState, cam_check, cam_check_hip, cam_upsample, gradcam_state,
                         occlusion_by_views, occlusion_fill, occlusion_grid, occlusion_state, occlusion_targets,
                         predict_batch, tta_views)

FORMAT = "gentun-cnn-ensemble/1"
OUTPUTS = ("proba", "label", "votes", "vote_label", "member_proba", "member_logits")
MAX_MEMBERS = 64             # ENS_MAXG of csrc/hip/cnn_dense.hip
# what every member shares: the search space and the configuration values the forward pass reads
SHARED = ("nodes", "input_shape", "kernels_per_layer", "kernel_sizes", "dense_units", "classes", "batch_norm",
          "bn_eps", "dtype", "loss")


def _genes_key(genes):
    return tuple(sorted(genes.items()))


def normalise_weights(weights, k):
    """``k`` finite non-negative numbers with a positive sum -> fp32 weights summing to one (normalised in
    fp64, then rounded); ``None``: uniform."""
    if weights is None:
        w = np.ones(k, np.float64)
    else:
        w = np.asarray(weights, np.float64).reshape(-1)
        if w.shape[0] != k:
            raise ValueError("{} weights for {} members".format(w.shape[0], k))
        if not np.isfinite(w).all():
            raise ValueError("weights must be finite")
        if (w < 0).any():
            raise ValueError("weights must be non-negative")
        if not w.sum() > 0:
            raise ValueError("weights must have a positive sum")
    return (w / w.sum()).astype(np.float32)


def combine(member_proba, weights):
    """``(proba, votes)`` of member probabilities ``[k, n, C]`` fp32: the weighted mean in member order
    (``acc = w[0] * p[0]``, then ``acc = acc + w[g] * p[g]``: numpy rounds the product and the sum
    separately, and so does ``gt_head_ensemble``) and the number of members whose first maximum is each
    class."""
    p = np.asarray(member_proba, np.float32)
    w = np.asarray(weights, np.float32)
    acc = w[0] * p[0]
    for g in range(1, p.shape[0]):
        acc = acc + w[g] * p[g]
    C = p.shape[2]
    votes = (np.argmax(p, axis=2)[:, :, None] == np.arange(C)[None, None, :]).sum(0).astype(np.int32)
    return acc.astype(np.float32), votes


def combine_maps(member_maps, weights):
    """The weighted mean of ``k`` equal-shape fp32 arrays in member order with :func:`combine`'s rounding
    (``acc = w[0] * a[0]``, then ``acc = acc + w[g] * a[g]``)."""
    w = np.asarray(weights, np.float32)
    acc = w[0] * np.asarray(member_maps[0], np.float32)
    for g in range(1, len(member_maps)):
        acc = acc + w[g] * np.asarray(member_maps[g], np.float32)
    return acc.astype(np.float32)


def vote_label(votes, proba):
    """The class with the most votes; ties go to the larger mean probability, then to the lower index."""
    tied = votes == votes.max(axis=1, keepdims=True)
    return np.argmax(np.where(tied, proba, -np.inf), axis=1).astype(np.int64)


class CnnEnsemble(object):

    def __init__(self, members, weights=None, metrics=None):
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError("an ensemble has 1 to {} members, got {}".format(MAX_MEMBERS, len(members)))
        for m in members:
            if not isinstance(m, CnnClassifier):
                raise ValueError("members must be CnnClassifier objects, got {}".format(type(m).__name__))
        first = members[0]
        for i, m in enumerate(members[1:], 1):
            for field in SHARED:
                if getattr(m, field) != getattr(first, field):
                    raise ValueError("member {} differs from member 0 in {}: {!r} != {!r}".format(
                        i, field, getattr(m, field), getattr(first, field)))
        seen = {}
        for i, m in enumerate(members):
            j = seen.setdefault(_genes_key(m.genes), i)
            if j != i:
                raise ValueError("members {} and {} have the same genes {}".format(j, i, m.genes))
        self.members = members
        self.weights = normalise_weights(weights, len(members))
        self.metrics = dict(metrics or {})
        self.classes, self.input_shape = first.classes, first.input_shape
        self._predictors = {}        # (device, EB) -> HipEnsemblePredictor
        self._rows = {}              # (device, requested rows per launch) -> EB

    def __len__(self):
        return len(self.members)

    # ------------------------------------------------------------ file format
    def header(self):
        return {"format": FORMAT, "members": [m.header() for m in self.members], "metrics": self.metrics}

    def save(self, path):
        """One ``.npz``: the JSON header string (the members' headers), the fp32 weights and member ``i``'s
        parameter ``name`` as ``m<i>.<name>``."""
        arrays = {"m{}.{}".format(i, name): a for i, m in enumerate(self.members) for name, a in m.params.items()}
        with open(path, "wb") as f:
            np.savez(f, header=np.array(json.dumps(self.header())), weights=self.weights, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "header" not in z.files:
                raise ValueError("{}: not a {} file".format(path, FORMAT))
            header = json.loads(str(z["header"][()]))
            if header.get("format") != FORMAT:
                raise ValueError("{}: format {!r}, expected {!r}".format(path, header.get("format"), FORMAT))
            weights = np.array(z["weights"], np.float32)
            members = []
            for i, h in enumerate(header["members"]):
                prefix = "m{}.".format(i)
                params = {name[len(prefix):]: z[name] for name in z.files if name.startswith(prefix)}
                members.append(CnnClassifier(h["genes"], h["nodes"], h["input_shape"], h["kernels_per_layer"],
                                             h["kernel_sizes"], h["dense_units"], h["classes"], params,
                                             batch_norm=h["batch_norm"], bn_eps=h["bn_eps"], loss=h["loss"],
                                             dtype=h["dtype"], metrics=h.get("metrics")))
        ens = cls(members, metrics=header.get("metrics"))
        if weights.shape != ens.weights.shape:
            raise ValueError("{}: {} weights for {} members".format(path, weights.shape[0], len(members)))
        ens.weights = weights        # the stored fp32 values, not a second normalisation of them
        return ens

    # ------------------------------------------------------------ prediction
    def predict(self, x, device=None, output="proba", batch=256, backend=None, tta=None):
        """One of ``OUTPUTS`` for ``x`` ``[n, H, W, C]`` (or one image), ``batch`` rows at a time:

        ``"proba"`` fp32 ``[n, classes]``, the weighted mean of the members' probabilities; ``"label"`` int64,
        its first maximum; ``"votes"`` int32 ``[n, classes]``, the members whose most probable class is each
        class; ``"vote_label"`` int64, the most voted class (ties: larger mean probability, then lower
        index); ``"member_proba"`` / ``"member_logits"`` fp32 ``[k, n, classes]``.

        ``device`` None or ``"cpu"``, or ``backend="torch"``: every member's stock-torch forward and the
        combination in numpy fp32. A ``cuda`` device: :class:`HipEnsemblePredictor`. A short chunk is
        filled with zero images and only the real rows are returned, as in ``CnnClassifier.predict``.

        ``tta`` (test-time augmentation, ``cnn_fitted.tta_views``): every member's probabilities and logits
        become their means over the views, as in ``CnnClassifier.predict(tta=...)``; the weighted mean, the
        votes and the labels are formed from those."""
        return self.predict_outputs(x, (output,), device=device, batch=batch, backend=backend, tta=tta)[output]

    def predict_outputs(self, x, outputs=OUTPUTS, device=None, batch=256, backend=None, tta=None):
        """``{name: array}`` of several ``OUTPUTS`` from one pass over ``x``."""
        outputs = tuple(outputs)
        for output in outputs:
            if output not in OUTPUTS:
                raise ValueError("output {!r}: expected one of {}".format(output, OUTPUTS))
        if int(batch) < 1:
            raise ValueError("batch must be positive")
        x = self.members[0]._check_x(x)
        views = tta_views(tta, self.input_shape)
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        res = {}
        if backend == "hip":
            res = self.hip_predictor(dev, batch).run(x, members="member_proba" in outputs or
                                                     "member_logits" in outputs, views=views)
        elif backend == "torch":
            kw = dict(device=dev, batch=int(batch), backend="torch", tta=views)
            res["member_proba"] = np.stack([np.asarray(m.predict(x, output="proba", **kw), np.float32)
                                            for m in self.members])
            if "member_logits" in outputs:
                res["member_logits"] = np.stack([np.asarray(m.predict(x, output="logits", **kw), np.float32)
                                                 for m in self.members])
            res["proba"], res["votes"] = combine(res["member_proba"], self.weights)
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        if "label" in outputs:
            res["label"] = np.argmax(res["proba"], axis=1).astype(np.int64)
        if "vote_label" in outputs:
            res["vote_label"] = vote_label(res["votes"], res["proba"])
        return {name: res[name] for name in outputs}

    def predict_classes(self, x, **kw):
        return self.predict(x, output="label", **kw)

    def occlusion(self, x, target=None, patch=4, stride=None, fill=0.0, score="proba", device=None, batch=256,
                  backend=None, return_info=False):
        """Occlusion sensitivity of the ensemble, ``CnnClassifier.occlusion`` with the weighted mean of the
        members' probabilities (``"proba"`` of :meth:`predict`) as the score: fp32 ``[n, Gh, Gw]``, the score of
        the target class minus its score with the cell replaced by ``fill``. ``target=None``: the first maximum
        of the weighted mean of the unoccluded image. The members' logits have no weighted mean here:
        ``score="logit"`` raises ``ValueError``."""
        if score != "proba":
            raise ValueError("score {!r}: an ensemble's occlusion score is 'proba'".format(score))
        if int(batch) < 1:
            raise ValueError("batch must be positive")
        x = self.members[0]._check_x(x)
        occlusion_grid(self.input_shape, patch, stride)
        fill = occlusion_fill(fill, self.input_shape[2])
        target = occlusion_targets(target, x.shape[0], self.classes)
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            res = self.hip_predictor(dev, batch).occlusion(x, target, patch, stride, fill)
        elif backend == "torch":
            def scores(images):
                member = np.stack([m._torch_predict(images, dev, int(batch), torch.float32)[1] for m in self.members])
                proba = combine(member, self.weights)[0]
                return proba, proba
            res = occlusion_by_views(scores, x, target, patch, stride, fill, int(batch))
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        return (res[0], {"target": res[1], "base": res[2]}) if return_info else res[0]

    def gradcam(self, x, target=None, score="logit", relu=True, upsample=False, device=None, batch=256,
                backend=None, return_info=False):
        """Grad-CAM of the ensemble (``CnnClassifier.gradcam``): fp32 ``[n, hr, wr]``, the weighted mean, in member
        order, of the members' maps (``acc = w[0] * cam_0``, then ``acc = acc + w[g] * cam_g``, the product and
        the sum rounded separately as in :func:`combine`). Every member's map is that of its own score (its logit
        or its probability) of the ensemble's target, with its own ReLU applied first when ``relu=True``.
        ``target=None``: the first maximum of the weighted mean of the members' probabilities.

        With ``score="proba"`` and ``relu=False`` the mean is exactly the Grad-CAM of the combined probability
        (the gradient is linear in the score). With ``relu=True`` the ReLU per member is a definition, not an
        identity: a region that one member counts against the class does not cancel another member's support.
        ``info["base"]`` is the weighted mean of the members' scores of the target: the combined probability, or
        with ``score="logit"`` the weighted mean of the members' logits."""
        cam_check(score, relu, upsample, batch)
        x = self.members[0]._check_x(x)
        target = occlusion_targets(target, x.shape[0], self.classes, "gradcam")
        dev = torch.device("cpu" if device is None else device)
        if backend is None:
            backend = "hip" if dev.type == "cuda" else "torch"
        if backend == "hip":
            cam_check_hip(self.members[0].plan, self.input_shape)
            res = self.hip_predictor(dev, batch).gradcam(x, target, score, bool(relu))
        elif backend == "torch":
            if target is None:
                member = np.stack([m._torch_predict(x, dev, int(batch), torch.float32)[1] for m in self.members])
                target = np.argmax(combine(member, self.weights)[0], axis=1).astype(np.int64)
            per = [m._torch_gradcam(x, target, score, bool(relu), dev, int(batch), torch.float32)
                   for m in self.members]
            res = (combine_maps([p[0] for p in per], self.weights), target,
                   combine_maps([p[2] for p in per], self.weights))
        else:
            raise ValueError("unknown backend {!r}".format(backend))
        cam = cam_upsample(res[0], self.input_shape[:2]) if upsample else res[0]
        return (cam, {"target": res[1], "base": res[2]}) if return_info else cam

    def distill(self, x, y_onehot, genes=None, alpha=0.5, temperature=1.0, device=None, **additional_parameters):
        """Fit one student on a blend of the hard labels and this ensemble's probabilities
        (:func:`gentun_amd.models.cnn_distill.distill`). ``genes=None``: the first member's genes."""
        from .cnn_distill import distill
        return distill(self, x, y_onehot, dict(self.members[0].genes) if genes is None else genes, alpha=alpha,
                       temperature=temperature, device=device, **additional_parameters)

    def hip_predictor(self, device, batch=256):
        """The cached :class:`HipEnsemblePredictor` of (device, rows per launch). The rows per launch are
        ``predict_batch(batch)`` lowered by the executor's rule for evaluation twins (``EVAL_TWIN_BUDGET``
        over all ``k`` groups, multiples of 32, at least 32); ``.EB`` of the result is the value chosen."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        want = predict_batch(batch)
        EB = self._rows.get((str(dev), want))
        if EB is None:
            pred = HipEnsemblePredictor(self, dev, want)         # may choose fewer rows than asked for
            EB = self._rows[(str(dev), want)] = self._rows[(str(dev), pred.EB)] = pred.EB
            self._predictors.setdefault((str(dev), EB), pred)
        return self._predictors[(str(dev), EB)]


# ---------------------------------------------------------------------------
# HIP predictor
# ---------------------------------------------------------------------------

class HipEnsemblePredictor(object):
    """Forward-only HIP launches of all ``k`` members at ``EB`` rows per launch.

    Hosted on one ``k``-group ``HipPopJob`` (member ``i`` is group ``i``, a member of its own with the one
    fold (all rows, all rows)) over a staging tensor of ``EB`` zero images, as ``HipPredictor`` is hosted
    on a one-group job: never initialised, trained or captured, the dataset cache left as found. Every
    group reads the same staged rows (gather table ``arange(EB)`` per group); the chain is the evaluation
    launches, ``gt_dense_fwd`` and ``gt_head_ensemble``. ``EB`` is the requested value lowered by
    ``HipPopJob.eval_batch`` -- the activation twins of all ``k`` groups stay inside ``EVAL_TWIN_BUDGET``."""

    def __init__(self, ens, device, EB):
        from ..ops import cnn_kernels as K
        self.K, self.device = K, torch.device(device)
        self.k, self.classes = len(ens.members), ens.classes
        EB = int(EB)
        if EB % 32 or not 32 <= EB <= 256:
            raise ValueError("rows per launch must be a multiple of 32 in [32, 256]")
        job = self._host(ens, EB)
        rows = int(job.eval_batch())
        if rows < EB:                            # k groups of EB rows would not fit the twin budget
            del job
            job = self._host(ens, rows)
        self.EB = EB = rows
        self.job = job
        self.stage = job.data.x                  # [EB][Hp][Wp][C8], fp32 (nhwc8f) or bf16 (nhwc8)
        self.hwc = tuple(ens.input_shape)
        k, C = self.k, self.classes
        with torch.cuda.device(self.device):
            for g, m in enumerate(ens.members):
                m.load_into(job, g)
            self.ops, self.df, _, self._keep = job._build_eval_ops(EB)
            self.gather = torch.arange(EB, dtype=torch.int64, device=self.device).repeat(k, 1).contiguous()
            for kind, b, _ in self.ops:
                if kind == "conv" and b.gather:
                    b.gather = self.gather.data_ptr()
            self.weight = torch.from_numpy(ens.weights.copy()).to(self.device)
            self.logits = torch.empty((k, EB, C), dtype=torch.float32, device=self.device)
            self.proba = torch.empty_like(self.logits)
            self.ens = torch.empty((EB, C), dtype=torch.float32, device=self.device)
            self.votes = torch.empty((EB, C), dtype=torch.int32, device=self.device)
            self.heads = {}
            for members in (False, True):        # the member outputs are written on request only
                a = K.HeadEnsembleArgs()
                a.plog, a.b2, a.weight = self.df.plog, job.views["b2"][0].data_ptr(), self.weight.data_ptr()
                a.logits = self.logits.data_ptr() if members else 0
                a.proba = self.proba.data_ptr() if members else 0
                a.ens, a.votes = self.ens.data_ptr(), self.votes.data_ptr()
                a.G, a.B, a.Up, a.C = k, EB, job.Up, C
                self.heads[members] = a
        self._tta = {}               # views -> TtaState, created on first use
        self._occ = {}               # (patch, stride, fill, score) -> OcclusionState, created on first use
        self._cam = {}               # (score, relu) -> GradcamState, created on first use
        self._cam_wbar = None        # W1 summed over the real pixels (cam_wbar), on the first Grad-CAM request

    def _host(self, ens, EB):
        from . import cnn_engine as E
        from .cnn_hip import HipPopJob
        first = ens.members[0]
        h, w, c = first.input_shape
        cfg = E.TrainConfig(epochs=(1,), learning_rate=(0.0,), batch_size=32, dropout=0.0, loss=first.loss,
                            dtype=first.dtype, use_graph=False, batch_norm=first.batch_norm, bn_eps=first.bn_eps)
        rows = np.arange(EB)
        x0 = np.zeros((EB, h, w, c), np.float32)
        y0 = np.zeros((EB, first.classes), np.float32)
        cache = list(E._DATA_CACHE)              # the staging tensor is this predictor's alone
        try:
            return HipPopJob(None, x0, y0, None, cfg, self.device,
                             members=[(m.plan, [(rows, rows)], [0]) for m in ens.members])
        finally:
            E._DATA_CACHE[:] = cache

    def forward(self, members=False):
        """The launches of one chunk on the current stream: staging tensor -> ``ens`` / ``votes`` (and
        ``logits`` / ``proba`` of every member with ``members``)."""
        job, K = self.job, self.K
        s = job._stream()
        job._run_fwd(s, self.ops)
        K.check(job.L.gt_dense_fwd(self.df, s), "dense_fwd(ensemble)")
        K.check(job.L.gt_head_ensemble(self.heads[bool(members)], s), "head_ensemble")

    def upload(self, chunk):
        """``chunk`` [m <= EB, H, W, C] host fp32 into the staging tensor; rows past ``m`` become zero images."""
        m = chunk.shape[0]
        h, w, c = self.hwc
        if m < self.EB:
            self.stage[m:].zero_()
        self.stage[:m, :h, :w, :c].copy_(torch.from_numpy(chunk).to(self.device))

    def tta_state(self, views):
        """The cached ``TtaState`` of a view tuple over the ``k`` members and their weights."""
        st = self._tta.get(views)
        if st is None:
            with torch.cuda.device(self.device):
                st = self._tta[views] = TtaState(self, views, self.k, self.weight)
        return st

    def occlusion(self, x, target, patch, stride, fill):
        """``(map, target, base)`` of validated arguments (``CnnEnsemble.occlusion``) over the ``k`` members and
        their weights."""
        return occlusion_state(self, patch, stride, fill, "proba", self.k, self.weight).run(self, x, target)

    def gradcam(self, x, target, score, relu):
        """``(map, target, base)`` of validated arguments (``CnnEnsemble.gradcam``) over the ``k`` members and
        their weights."""
        return gradcam_state(self, score, relu, self.k, self.weight).run(self, x, target)

    def run(self, x, members=False, views=None):
        """``x`` [n, H, W, C] host fp32 -> ``{"proba", "votes"}`` (+ ``"member_proba"``, ``"member_logits"``)
        as host arrays; the chunks' results gather on the device and are read back once. With ``views`` (a
        tuple of ``(dy, dx, flip)``) every member's outputs are the means over those views,
        ``EB // len(views)`` rows per launch."""
        n, EB, k, C = x.shape[0], self.EB, self.k, self.classes
        ens = torch.empty((n, C), dtype=torch.float32, device=self.device)
        votes = torch.empty((n, C), dtype=torch.int32, device=self.device)
        if members:
            logits = torch.empty((k, n, C), dtype=torch.float32, device=self.device)
            proba = torch.empty_like(logits)
        with torch.cuda.device(self.device):
            st = None if views is None else self.tta_state(tuple(views))
            rows, res = (EB, self) if st is None else (st.R, st)     # rows per chunk, who holds its results
            if st is not None and st.V * st.R < EB:
                self.stage[st.V * st.R:].zero_()                     # rows no view is written to
            for s in range(0, n, rows):
                m = min(rows, n - s)
                if st is None:
                    self.upload(x[s:s + m])
                    self.forward(members)
                else:
                    st.upload(x[s:s + m], self.hwc)
                    st.forward(self, members, "ensemble")
                ens[s:s + m].copy_(res.ens[:m])
                votes[s:s + m].copy_(res.votes[:m])
                if members:
                    logits[:, s:s + m].copy_(res.logits[:, :m])
                    proba[:, s:s + m].copy_(res.proba[:, :m])
            out = {"proba": ens.cpu().numpy(), "votes": votes.cpu().numpy()}
            if members:
                out["member_logits"], out["member_proba"] = logits.cpu().numpy(), proba.cpu().numpy()
        return out


# ---------------------------------------------------------------------------
# fitting
# ---------------------------------------------------------------------------

def _fit_metrics(res, rows):
    return {"loss": float(res["val_loss"][0]), "binary_accuracy": float(res["binary_accuracy"][0]),
            "categorical_accuracy": float(res["categorical_accuracy"][0]), "rows": int(rows)}


def fit_ensemble(x, y, genes_list, weights=None, device=None, **additional_parameters):
    """Train one network per genome of ``genes_list`` on every row of ``x`` with the search's own settings
    (``additional_parameters``: what ``GeneticCnnModel`` takes) and return them as a :class:`CnnEnsemble`.

    HIP backend: ONE population job with one group per member, each with the fold (all rows, all rows) and
    the fold id ``nfold`` -- the seeds and streams of ``GeneticCnnModel.fit()``, keyed by (seed, genes, fold
    id), so member ``i`` is bit-identical to ``fit()`` of genome ``i`` alone. Torch backend: each model's
    ``fit()`` in turn (its population job agrees with single jobs only to rounding). Every member's
    ``metrics`` are what ``fit()`` records; the ensemble's hold the training-set categorical accuracy of
    ``output="label"``, the row count and the members' genes."""
    from . import cnn_engine as E
    from ..utils.data import labels_from_onehot
    from .cnn import GeneticCnnModel
    genes_list = [dict(g) for g in genes_list]
    k = len(genes_list)
    if not 1 <= k <= MAX_MEMBERS:
        raise ValueError("an ensemble has 1 to {} members, got {}".format(MAX_MEMBERS, k))
    if len({_genes_key(g) for g in genes_list}) != k:
        raise ValueError("the genomes of an ensemble must be pairwise distinct")
    normalise_weights(weights, k)                # a bad weight raises before anything trains
    models = [GeneticCnnModel(x, y, g, device=device, **additional_parameters) for g in genes_list]
    first = models[0]
    if first.backend == "hip":
        rows = np.arange(len(first.x_train))
        job = E.make_population_job("hip", [(m.model, [(rows, rows)], [m.nfold]) for m in models], first.x_train,
                                    first.y_train, first.cfg, first.device)
        job.launch()
        res = job.finish()
        for g, m in enumerate(models):
            m.jobs = [job]
            m.fitted = CnnClassifier.from_job(job, g, metrics=_fit_metrics(res[g], len(rows)))
    else:
        for m in models:
            m.fit()
    ens = CnnEnsemble([m.fitted for m in models], weights=weights)
    label = ens.predict(first.x_train, device=first.device, output="label", backend=first.backend)
    hits = int((label == np.asarray(labels_from_onehot(first.y_train))).sum())
    ens.metrics = {"categorical_accuracy": hits / float(len(label)), "rows": int(len(label)),
                   "genes": [m.genes for m in ens.members]}
    return ens


def top_genomes(population, k, maximize=None):
    """The genes of the ``k`` fittest individuals of ``population`` (a ``Population`` or any sequence of
    individuals) with pairwise distinct genes, fittest first, ties in population order. Only fitnesses that
    are already computed count (nothing is evaluated; a failed evaluation's infinite fitness is no
    fitness), so fewer than ``k`` come back when fewer distinct evaluated individuals exist."""
    if maximize is None:
        maximize = bool(getattr(population, "maximize", True))
    scored = []
    for ind in population:
        if ind.get_fitness_status() and math.isfinite(ind.fitness):
            scored.append((-ind.fitness if maximize else ind.fitness, ind))
    scored.sort(key=lambda t: t[0])              # stable: ties keep the population's order
    out, seen = [], set()
    for _, ind in scored:
        key = _genes_key(ind.get_genes())
        if key not in seen:
            seen.add(key)
            out.append(dict(ind.get_genes()))
        if len(out) >= int(k):
            break
    return out[:max(0, int(k))]
