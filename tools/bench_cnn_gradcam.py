"""Grad-CAM (``gradcam(...)``) throughput on one GPU at the headline search space (nodes (3, 5), kernels (20, 50),
5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` and a ``CnnEnsemble`` of k = 4, fitted for one epoch
on ``--fit-rows`` glyph images, over ``--rows`` held-out 32x32x3 ones (8 x 8 maps):

(i)   ``gradcam(x, device=...)`` on the HIP predictor: the forward launches, then ``gt_head_gradcam``;
(ii)  plain HIP ``predict`` of the same rows -- the floor: the same uploads and forward launches;
(iii) ``gradcam(backend="torch")`` on the same GPU: stock-torch forward and autograd through the dense head;
(iv)  ``occlusion(patch=4)`` (64 forwards per image) on the first ``--occ-rows`` rows, for context.

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. After that, in a
pass of its own, an estimate of the device time of ``gt_head_gradcam`` alone at ``EB`` rows -- 20 back-to-back
launches between two events on the stream, not a trace -- next to that of the forward launches it follows (conv
stages + ``gt_dense_fwd``), and of ``gt_cam_w1sum`` into its existing buffer. One JSON line per model as it
finishes, then the whole result as the last line.

``--trace`` is the child of a kernel trace run of its own (``tools/gpu.sh cnn-gradcam`` starts it under
``rocprofv3 --kernel-trace --stats``): it fits the models, calls ``gradcam`` on ``--rows`` rows three times per
model and exits; the trace's statistics then hold the kernels' own durations.

usage: python tools/bench_cnn_gradcam.py [--rows 10000] [--occ-rows 1000] [--fit-rows 2000] [--k 4] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10000)
ap.add_argument("--occ-rows", type=int, default=1000)
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--score", choices=("logit", "proba"), default="logit")
ap.add_argument("--models", default="classifier,ensemble")
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--trace", action="store_true", help="fit, call gradcam three times per model and exit")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import fit_ensemble  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_gradcam needs a GPU")
dev = torch.device(args.device)
shape = (32, 32, 3)
space = dict(nodes=(3, 5), input_shape=shape, kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
             dense_units=500, classes=10)
rng = np.random.default_rng(0)


def genomes(k):
    out, seen = [], set()
    while len(out) < k:
        g = {"S_1": "".join(rng.choice(["0", "1"], 3)), "S_2": "".join(rng.choice(["0", "1"], 10))}
        if tuple(g.values()) not in seen:
            seen.add(tuple(g.values()))
            out.append(g)
    return out


def timed(fn):
    """ms of ``fn()`` by the host clock (``fn`` ends in a device synchronise)."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0), out


def device_us(fn, n=20):
    """us per call between two events on the current stream around ``n`` calls of ``fn``."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return 1e3 * a.elapsed_time(b) / n


def summary(ms, rows):
    return {"median_ms": round(statistics.median(ms), 3), "best_ms": round(min(ms), 3),
            "rows_per_s": round(rows / (1e-3 * statistics.median(ms)))}


n_fit = args.fit_rows
fx, fy = make_glyph_classification(n=n_fit + args.rows, shape=shape, classes=10, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x = np.ascontiguousarray(fx[n_fit:])
fx, fy = fx[:n_fit], fy[:n_fit]
kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
          dtype=args.dtype, seed=5, backend="hip")
gs = genomes(args.k)
result = {"metric": "gradcam(score={!r}), images/s".format(args.score), "rows": args.rows, "occ_rows": args.occ_rows,
          "fit_rows": n_fit, "dtype": args.dtype, "reps": args.reps, "batch": args.batch,
          "device": torch.cuda.get_device_name(dev), "cases": {}}
with torch.cuda.device(dev):
    models = []
    if "classifier" in args.models:
        models.append((GeneticCnnModel(fx, fy, gs[0], device=dev, **kw).fit(), "classifier"))
    if "ensemble" in args.models:
        models.append((fit_ensemble(fx, fy, gs, device=dev, **kw), "ensemble_k{}".format(args.k)))

    if args.trace:
        for model, name in models:
            for _ in range(3):
                model.gradcam(x, score=args.score, device=dev, batch=args.batch)
            torch.cuda.synchronize(dev)
        print(json.dumps({"trace": [name for _, name in models], "rows": args.rows}), flush=True)
        sys.exit(0)

    for model, name in models:
        pred = model.hip_predictor(dev, args.batch)
        xo = x[:args.occ_rows]
        paths = {
            "i_hip_gradcam": (lambda: model.gradcam(x, score=args.score, device=dev, batch=args.batch), args.rows),
            "ii_hip_predict": (lambda: model.predict(x, device=dev, output="proba", batch=args.batch), args.rows),
            "iii_torch_gradcam": (lambda: model.gradcam(x, score=args.score, device=dev, batch=args.batch,
                                                        backend="torch"), args.rows),
            "iv_hip_occlusion_patch4": (lambda: model.occlusion(xo, patch=4, device=dev, batch=args.batch),
                                        len(xo)),
        }
        first, outs, total = {}, {}, {p: [] for p in paths}
        for p, (fn, _) in paths.items():                 # warm-up: predictors and states are built here
            first[p], outs[p] = timed(fn)
        for _ in range(args.reps):                       # alternated run by run
            for p, (fn, _) in paths.items():
                total[p].append(timed(fn)[0])
        raw = {b: model.gradcam(x[:512], score=args.score, relu=False, device=dev, batch=args.batch, backend=b)
               for b in ("hip", "torch")}
        # a pass of its own: the new kernels alone next to the launches they follow, over the staging tensor
        job, K = pred.job, pred.K
        st = pred._cam[(args.score, True)]
        st.tgt.fill_(-1)
        st.head.m = pred.EB

        def fwd():
            s = job._stream()
            job._run_fwd(s, pred.ops)
            K.check(job.L.gt_dense_fwd(pred.df, s), "dense_fwd")

        (hs, ws), (hr, wr) = job.final_hw, job.final_hw_real
        wa = K.CamW1SumArgs()                            # into the predictor's own wbar: the same values again
        wa.w1, wa.wbar = job.views["W1"][0].data_ptr(), pred._cam_wbar.data_ptr()
        wa.G, wa.hs, wa.ws, wa.hr, wa.wr = st.head.G, hs, ws, hr, wr
        wa.Cp, wa.Cr, wa.Up = st.head.Cp, st.head.Cr, job.Up

        def w1sum():
            K.check(job.L.gt_cam_w1sum(wa, job._stream()), "cam_w1sum")
        rec = {"rows_per_launch": pred.EB,
               "map": list(outs["i_hip_gradcam"].shape[1:]),
               "max_rel_diff_i_vs_iii_raw_map": float(np.abs(raw["hip"].astype(np.float64) - raw["torch"]).max()
                                                      / np.abs(raw["torch"]).max()),
               "device_us_forward_launches": round(device_us(fwd), 2),
               "device_us_head_gradcam": round(device_us(
                   lambda: K.check(job.L.gt_head_gradcam(st.head, job._stream()), "head_gradcam")), 2),
               "device_us_head_predict_or_ensemble": round(device_us(
                   lambda: K.check(job.L.gt_head_predict(pred.head, job._stream()), "head") if name == "classifier"
                   else K.check(job.L.gt_head_ensemble(pred.heads[False], job._stream()), "head")), 2),
               "device_us_cam_w1sum_once": round(device_us(w1sum, 5), 2)}
        for p, (_, rows) in paths.items():
            rec[p] = dict(summary(total[p], rows), first_call_ms=round(first[p], 1), rows=rows)
        rec["i_over_ii"] = round(rec["i_hip_gradcam"]["median_ms"] / rec["ii_hip_predict"]["median_ms"], 3)
        rec["iii_over_i"] = round(rec["iii_torch_gradcam"]["median_ms"] / rec["i_hip_gradcam"]["median_ms"], 3)
        rec["occlusion_over_gradcam_per_image"] = round(
            (rec["iv_hip_occlusion_patch4"]["median_ms"] / len(xo)) / (rec["i_hip_gradcam"]["median_ms"] / args.rows), 1)
        result["cases"][name] = rec
        print(json.dumps({name: rec}), flush=True)
print(json.dumps(result), flush=True)
