"""RISE saliency (``rise(...)``) throughput on one GPU at the headline search space (nodes (3, 5), kernels
(20, 50), 5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` and a ``CnnEnsemble`` of k = 4, fitted for
one epoch on ``--fit-rows`` glyph images, over ``--rows`` held-out 32x32x3 ones at ``--masks`` masks:

(i)   ``rise(x, device=...)`` on the HIP predictor: every image uploaded once, the masked copies blended on the
      device (gt_rise_views) and packed densely into launches, one score per copy kept (gt_head_rise), the map by
      gt_rise_accumulate;
(ii)  the same map without the new kernels: ``rise_masks`` / ``rise_views`` in numpy, plain HIP ``predict`` calls,
      an fp64 numpy accumulate;
(iii) ``backend="torch"`` on the same GPU.

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. Each case also
reports the device time per masked copy of (i) (events around a whole call, divided by rows x masks) next to the
device time per row of the plain predictor's launches. ``--trace`` runs three calls of (i) and twenty plain launch
sets per model and nothing else, for a kernel trace of its own. One JSON line per case, then the whole result.

usage: python tools/bench_cnn_rise.py [--rows 1000] [--masks 2048] [--fit-rows 2000] [--k 4] [--reps 5] [--trace]
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
ap.add_argument("--masks", type=int, default=2048)
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--models", default="classifier,ensemble")
ap.add_argument("--paths", default="i,ii,iii")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--device", default="cuda:0")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import fit_ensemble  # noqa: E402
from gentun_amd.models.cnn_fitted import rise_inv, rise_masks, rise_views  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_rise needs a GPU")
dev = torch.device(args.device)
shape = (32, 32, 3)
space = dict(nodes=(3, 5), input_shape=shape, kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
             dense_units=500, classes=10)
CELLS, P, SEED = 7, 0.5, 0
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


fx, fy = make_glyph_classification(n=args.fit_rows + args.rows, shape=shape, classes=10, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x = np.ascontiguousarray(fx[args.fit_rows:])
fx, fy = fx[:args.fit_rows], fy[:args.fit_rows]
kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
          dtype=args.dtype, seed=5, backend="hip")
gs = genomes(args.k)
views = args.rows * args.masks
result = {"metric": "rise(masks={}, cells=7, p=0.5), masked copies/s".format(args.masks), "rows": args.rows,
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
        pred.forward()

        def hip():
            return model.rise(x, masks=args.masks, cells=CELLS, p=P, seed=SEED, device=dev, batch=args.batch)
        if args.trace:
            for _ in range(3):
                hip()
            for _ in range(20):
                pred.forward()
            torch.cuda.synchronize(dev)
            continue
        plain_us = 1e3 * device_ms(lambda: [pred.forward() for _ in range(20)]) / (20 * pred.EB)
        Ms = rise_masks(shape, args.masks, CELLS, P, SEED)
        M64 = Ms.reshape(args.masks, -1).astype(np.float64)
        step = max(1, 16384 // args.masks)                   # images whose copies the host holds at a time

        def by_hand():
            # before rise(): the copies on the host, plain predicts, the accumulate on the host
            t = np.argmax(model.predict(x, device=dev, output="proba", batch=args.batch), axis=1)
            out = np.empty((args.rows, shape[0] * shape[1]), np.float32)
            for s in range(0, args.rows, step):
                v = rise_views(x[s:s + step], Ms, 0.0)
                m = v.shape[0]
                p = model.predict(v.reshape((-1,) + shape), device=dev, output="proba", batch=args.batch)
                sel = p.reshape(m, args.masks, -1)[np.arange(m), :, t[s:s + m]]
                out[s:s + m] = sel.astype(np.float64) @ M64 * rise_inv(args.masks, P)
            return out.reshape((args.rows,) + shape[:2])

        paths = {"i": ("i_hip_rise", hip), "ii": ("ii_hip_views_by_hand", by_hand),
                 "iii": ("iii_torch_backend", lambda: model.rise(x, masks=args.masks, cells=CELLS, p=P, seed=SEED,
                                                                 device=dev, batch=args.batch, backend="torch"))}
        paths = dict(paths[p] for p in ["i"] + [p for p in args.paths.split(",") if p != "i"])    # (i) always runs
        first, outs, total = {}, {}, {p: [] for p in paths}
        for p, fn in paths.items():                      # warm-up: predictors and the RISE state are built here
            first[p], outs[p] = timed(fn)
        for _ in range(args.reps):                       # alternated run by run
            for p, fn in paths.items():
                total[p].append(timed(fn)[0])
        st = [v for k, v in pred._rise.items() if k[0] == args.masks][0]
        dev_ms = statistics.median(device_ms(lambda: st.run(pred, x, None)) for _ in range(3))
        rec = {"masks": args.masks, "views": views, "rows_per_launch": pred.EB,
               "device_us_per_view_i": round(1e3 * dev_ms / views, 4),
               "device_us_per_row_plain_launches": round(plain_us, 4)}
        for p in paths:
            med = statistics.median(total[p])
            rec[p] = {"median_ms": round(med, 3), "best_ms": round(min(total[p]), 3),
                      "views_per_s": round(views / (1e-3 * med)), "first_call_ms": round(first[p], 1)}
            if p != "i_hip_rise":
                rec[p]["over_i"] = round(med / statistics.median(total["i_hip_rise"]), 3)
                rec[p]["max_abs_diff_vs_i"] = float(np.abs(outs[p].astype(np.float64) - outs["i_hip_rise"]).max())
        rec["largest_abs_map"] = float(np.abs(outs["i_hip_rise"]).max())
        result["cases"][name] = rec
        print(json.dumps({name: rec}), flush=True)
print(json.dumps(result), flush=True)
