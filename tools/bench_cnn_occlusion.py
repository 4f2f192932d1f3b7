"""Occlusion sensitivity (``occlusion(...)``) throughput on one GPU at the headline search space (nodes (3, 5),
kernels (20, 50), 5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` and a ``CnnEnsemble`` of k = 4,
fitted for one epoch on ``--fit-rows`` glyph images, over ``--rows`` held-out 32x32x3 ones; patch 4 at stride 4
(64 cells per image) and patch 4 at stride 2 (225 cells):

(i)   ``occlusion(x, device=...)`` on the HIP predictor: every image uploaded once, the occluded copies built on
      the device (gt_occlude_views) and packed densely into launches, one float per copy kept (gt_head_occlusion);
(ii)  the same bytes without the new kernels: ``occlusion_views`` in numpy, plain HIP ``predict`` calls, the
      numpy subtraction -- what a user did before;
(iii) ``backend="torch"`` on the same GPU.

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. Each case also
reports whether (i) and (ii) are byte-equal, and the device time per copy of (i) (events around the launches of a
whole call, divided by rows x cells) next to the device time per row of the plain predictor's launches over the
same staging tensor. One JSON line per case as it finishes, then the whole result as the last line.

usage: python tools/bench_cnn_occlusion.py [--rows 1000] [--fit-rows 2000] [--k 4] [--reps 5] [--device cuda:0]
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
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--strides", default="4,2", help="strides of patch 4 to measure")
ap.add_argument("--models", default="classifier,ensemble")
ap.add_argument("--device", default="cuda:0")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import fit_ensemble  # noqa: E402
from gentun_amd.models.cnn_fitted import occlusion_grid, occlusion_views  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_occlusion needs a GPU")
dev = torch.device(args.device)
shape = (32, 32, 3)
space = dict(nodes=(3, 5), input_shape=shape, kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
             dense_units=500, classes=10)
PATCH = 4
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


def device_ms(fn):
    """ms between two events on the current stream around ``fn()``."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def summary(ms, views):
    return {"median_ms": round(statistics.median(ms), 3), "best_ms": round(min(ms), 3),
            "views_per_s": round(views / (1e-3 * statistics.median(ms)))}


fx, fy = make_glyph_classification(n=args.fit_rows + args.rows, shape=shape, classes=10, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x = np.ascontiguousarray(fx[args.fit_rows:])
fx, fy = fx[:args.fit_rows], fy[:args.fit_rows]
kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
          dtype=args.dtype, seed=5, backend="hip")
gs = genomes(args.k)
result = {"metric": "occlusion(patch=4, score='proba'), occluded copies/s", "rows": args.rows,
          "fit_rows": args.fit_rows, "dtype": args.dtype, "reps": args.reps, "batch": args.batch,
          "device": torch.cuda.get_device_name(dev), "cases": {}}
with torch.cuda.device(dev):
    models = []
    if "classifier" in args.models:
        models.append((GeneticCnnModel(fx, fy, gs[0], device=dev, **kw).fit(), "classifier"))
    if "ensemble" in args.models:
        models.append((fit_ensemble(fx, fy, gs, device=dev, **kw), "ensemble_k{}".format(args.k)))

    for model, name in models:
        pred = model.hip_predictor(dev, args.batch)
        model.predict(x, device=dev, output="label", batch=args.batch)
        # the plain predictor's launches alone, over whatever the staging tensor holds: device time per row
        pred.forward()
        plain_us = 1e3 * device_ms(lambda: [pred.forward() for _ in range(20)]) / (20 * pred.EB)
        for stride in (int(s) for s in args.strides.split(",")):
            Gh, Gw = occlusion_grid(shape, PATCH, stride)
            Cc, views = Gh * Gw, args.rows * Gh * Gw
            step = max(1, 16384 // Cc)                   # images whose copies the host holds at a time

            def by_hand():
                # before occlusion(): the copies on the host, plain predicts, the subtraction on the host
                proba = model.predict(x, device=dev, output="proba", batch=args.batch)
                t = np.argmax(proba, axis=1)
                out = np.empty((args.rows, Cc), np.float32)
                for s in range(0, args.rows, step):
                    v = occlusion_views(x[s:s + step], PATCH, stride, 0.0)
                    m = v.shape[0]
                    p = model.predict(v.reshape((-1,) + shape), device=dev, output="proba", batch=args.batch)
                    sel = p.reshape(m, Cc, -1)[np.arange(m), :, t[s:s + m]]
                    out[s:s + m] = proba[s:s + m][np.arange(m), t[s:s + m]][:, None] - sel
                return out.reshape(args.rows, Gh, Gw)

            paths = {
                "i_hip_occlusion": lambda: model.occlusion(x, patch=PATCH, stride=stride, device=dev, batch=args.batch),
                "ii_hip_views_by_hand": by_hand,
                "iii_torch_backend": lambda: model.occlusion(x, patch=PATCH, stride=stride, device=dev,
                                                             batch=args.batch, backend="torch"),
            }
            first, outs, total = {}, {}, {p: [] for p in paths}
            for p, fn in paths.items():                  # warm-up: predictors and occlusion state are built here
                first[p], outs[p] = timed(fn)
            for _ in range(args.reps):                   # alternated run by run
                for p, fn in paths.items():
                    total[p].append(timed(fn)[0])
            st = [v for k, v in pred._occ.items() if k[:2] == (PATCH, stride)][0]
            dev_ms = statistics.median(device_ms(lambda: st.run(pred, x, None)) for _ in range(3))
            launches = sum(1 + -(-min(pred.EB, args.rows - s) * Cc // pred.EB) for s in range(0, args.rows, pred.EB))
            rec = {"stride": stride, "cells": Cc, "views": views, "rows_per_launch": pred.EB, "launches": launches,
                   "i_equals_ii": outs["i_hip_occlusion"].tobytes() == outs["ii_hip_views_by_hand"].tobytes(),
                   "max_abs_diff_i_vs_iii": float(np.abs(outs["i_hip_occlusion"].astype(np.float64)
                                                         - outs["iii_torch_backend"]).max()),
                   "device_us_per_view_i": round(1e3 * dev_ms / views, 4),
                   "device_us_per_row_plain_launches": round(plain_us, 4)}
            for p in paths:
                rec[p] = dict(summary(total[p], views), first_call_ms=round(first[p], 1))
            rec["ii_over_i"] = round(rec["ii_hip_views_by_hand"]["median_ms"] / rec["i_hip_occlusion"]["median_ms"], 3)
            rec["iii_over_i"] = round(rec["iii_torch_backend"]["median_ms"] / rec["i_hip_occlusion"]["median_ms"], 3)
            result["cases"]["{}_stride{}".format(name, stride)] = rec
            print(json.dumps({"{}_stride{}".format(name, stride): rec}), flush=True)
print(json.dumps(result), flush=True)
