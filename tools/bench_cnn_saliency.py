"""Input-gradient saliency (``saliency(...)``) throughput on one GPU at the headline search space (nodes (3, 5),
kernels (20, 50), 5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` and a ``CnnEnsemble`` of k = 4,
fitted for one epoch on ``--fit-rows`` glyph images, over ``--rows`` held-out 32x32x3 ones:

(i)   ``saliency(x, method="gradient", device=...)`` on the HIP predictor: the masked forward, ``gt_head_saliency``,
      the evaluation-mode backward chain, ``gt_conv_in_dgrad`` and ``gt_ig_reduce``;
(ii)  plain HIP ``predict`` of the same rows -- the floor: the same uploads and forward launches;
(iii) ``saliency(backend="torch")`` on the same GPU: stock-torch forward with autograd on the input;
(iv)  ``saliency(method="integrated", steps=--steps)`` on the HIP predictor over the first ``--ig-rows`` rows;
(v)   ``saliency(smooth={"samples": --samples})`` on the HIP predictor over the same ``--ig-rows`` rows: the points
      drawn by ``gt_sg_points``, the statistics formed by ``gt_sg_reduce``;
(vi)  the same map by hand: one ``predict`` for the labels, ``--samples`` plain HIP ``saliency`` calls on noisy copies
      made on the host (``smooth_point``) and the numpy finish (``smooth_finish``);
(vii) ``saliency(smooth=..., backend="torch")`` on the same GPU.

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. One JSON line per
model as it finishes, then the whole result as the last line.

``--trace`` is the child of a kernel trace run of its own (``tools/gpu.sh cnn-saliency`` starts it under
``rocprofv3 --kernel-trace --stats``): it fits the models, calls ``saliency`` on ``--rows`` rows three times per model
and exits; the trace's statistics then hold the kernels' own durations. With ``--trace-smooth`` the three calls are
those of (v) instead.

usage: python tools/bench_cnn_saliency.py [--rows 10000] [--ig-rows 1000] [--steps 16] [--fit-rows 2000] [--k 4]
                                            [--samples 16]
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
ap.add_argument("--ig-rows", type=int, default=1000)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--models", default="classifier,ensemble")
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--trace", action="store_true", help="fit, call saliency three times per model and exit")
ap.add_argument("--trace-smooth", action="store_true", help="--trace with the smooth calls of (v)")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import fit_ensemble  # noqa: E402
from gentun_amd.models.cnn_fitted import saliency_reduce, smooth_finish, smooth_point, smooth_sigma  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_saliency needs a GPU")
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


def summary(ms, rows):
    return {"median_ms": round(statistics.median(ms), 3), "best_ms": round(min(ms), 3),
            "rows_per_s": round(rows / (1e-3 * statistics.median(ms)))}


n_fit = args.fit_rows
fx, fy = make_glyph_classification(n=n_fit + args.rows, shape=shape, classes=10, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x = np.ascontiguousarray(fx[n_fit:])
xi = x[:args.ig_rows]
fx, fy = fx[:n_fit], fy[:n_fit]
kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
          dtype=args.dtype, seed=5, backend="hip")
gs = genomes(args.k)
smooth = {"samples": args.samples, "noise": 0.15, "seed": 0, "stat": "mean"}


def by_hand(model, on):
    """(vi): the SmoothGrad map of ``xi`` from plain calls and host work."""
    t = model.predict(xi, output="label", **on)
    sigma = smooth_sigma(xi, smooth["noise"])
    g = [model.saliency(smooth_point(xi, sigma, smooth["seed"], k), target=t, reduce=None, **on)
         for k in range(args.samples)]
    return saliency_reduce(smooth_finish(g, xi, "gradient", "mean"), "absmax")


result = {"metric": "saliency(), images/s", "rows": args.rows, "ig_rows": len(xi), "steps": args.steps,
          "samples": args.samples,
          "fit_rows": n_fit, "dtype": args.dtype, "reps": args.reps, "batch": args.batch,
          "device": torch.cuda.get_device_name(dev), "cases": {}}
with torch.cuda.device(dev):
    models = []
    if "classifier" in args.models:
        models.append((GeneticCnnModel(fx, fy, gs[0], device=dev, **kw).fit(), "classifier"))
    if "ensemble" in args.models:
        models.append((fit_ensemble(fx, fy, gs, device=dev, **kw), "ensemble_k{}".format(args.k)))

    if args.trace or args.trace_smooth:
        for model, name in models:
            for _ in range(3):
                if args.trace_smooth:
                    model.saliency(xi, device=dev, batch=args.batch, smooth=smooth)
                else:
                    model.saliency(x, device=dev, batch=args.batch)
            torch.cuda.synchronize(dev)
        print(json.dumps({"trace": [name for _, name in models], "rows": args.rows}), flush=True)
        sys.exit(0)

    for model, name in models:
        on = dict(device=dev, batch=args.batch)
        paths = {"i_hip_gradient": (lambda: model.saliency(x, **on), args.rows),
                 "ii_hip_predict": (lambda: model.predict(x, output="proba", **on), args.rows),
                 "iii_torch_gradient": (lambda: model.saliency(x, backend="torch", **on), args.rows),
                 "iv_hip_integrated": (lambda: model.saliency(xi, method="integrated", steps=args.steps, **on), len(xi)),
                 "v_hip_smooth": (lambda: model.saliency(xi, smooth=smooth, **on), len(xi)),
                 "vi_hip_smooth_by_hand": (lambda: by_hand(model, on), len(xi)),
                 "vii_torch_smooth": (lambda: model.saliency(xi, smooth=smooth, backend="torch", **on), len(xi))}
        first, outs, total = {}, {}, {p: [] for p in paths}
        for p, (fn, _) in paths.items():                 # warm-up: predictors and states are built here
            first[p], outs[p] = timed(fn)
        for _ in range(args.reps):                       # alternated run by run
            for p, (fn, _) in paths.items():
                total[p].append(timed(fn)[0])
        hip, ref = outs["i_hip_gradient"], outs["iii_torch_gradient"]
        rec = {"rows_per_launch": model.hip_predictor(dev, args.batch).EB,
               "median_rel_diff_i_vs_iii": float(np.median(np.abs(hip - ref).max((1, 2)) / ref.max((1, 2))))}
        for p, (_, rows) in paths.items():
            rec[p] = dict(summary(total[p], rows), first_call_ms=round(first[p], 1))
        rec["i_over_ii"] = round(rec["i_hip_gradient"]["median_ms"] / rec["ii_hip_predict"]["median_ms"], 3)
        rec["iii_over_i"] = round(rec["iii_torch_gradient"]["median_ms"] / rec["i_hip_gradient"]["median_ms"], 3)
        rec["vi_over_v"] = round(rec["vi_hip_smooth_by_hand"]["median_ms"] / rec["v_hip_smooth"]["median_ms"], 3)
        rec["vii_over_v"] = round(rec["vii_torch_smooth"]["median_ms"] / rec["v_hip_smooth"]["median_ms"], 3)
        rec["max_abs_diff_v_vs_vi"] = float(np.abs(outs["v_hip_smooth"] - outs["vi_hip_smooth_by_hand"]).max())
        result["cases"][name] = rec
        print(json.dumps({name: rec}), flush=True)
print(json.dumps(result), flush=True)
