"""Nearest-neighbour search (``neighbors(...)``) on one GPU at the headline search space (nodes (3, 5), kernels
(20, 50), 5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` and a ``CnnEnsemble`` of k = 4, fitted for
one epoch on ``--fit-rows`` glyph images: ``--rows`` query images against a bank of ``--bank`` images, ``--k``
neighbours:

(i)   ``neighbors(x, bank, device=...)`` on the HIP path: both forwards, ``gt_nn_bank``, ``gt_nn_topk``, ``gt_nn_merge``;
(ii)  ``embed`` of both on the HIP path, then ``torch.cdist`` + ``topk`` on the same GPU, 2048 queries at a time
      (host array to host array like the others, so the embeddings come to the host and go back: 120 MB each way for
      the classifier, 480 MB for the ensemble, which is part of what (i) saves);
(iii) ``embed`` of both on the HIP path, then a host search: fp64 BLAS distances and ``argpartition``, 1024 queries
      at a time (not the sequential-sum definition of ``neighbors_search``, which is far slower).

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. One JSON line per
model as it finishes, then the whole result as the last line.

``--trace`` is the child of a kernel trace run of its own (``tools/gpu.sh cnn-neighbors`` starts it under
``rocprofv3 --kernel-trace --stats``): it fits the models, calls ``neighbors`` twice per model and exits.

usage: python tools/bench_cnn_neighbors.py [--rows 10000] [--bank 50000] [--k 5] [--fit-rows 2000] [--members 4]
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
ap.add_argument("--bank", type=int, default=50000)
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--metric", default="l2")
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--members", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--models", default="classifier,ensemble")
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--no-host", action="store_true", help="leave path (iii) out")
ap.add_argument("--trace", action="store_true", help="fit, call neighbors twice per model and exit")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import fit_ensemble  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_neighbors needs a GPU")
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
            "queries_per_s": round(rows / (1e-3 * statistics.median(ms)))}


def cdist_topk(model, x, bank):
    q = torch.from_numpy(model.embed(x, device=dev, batch=args.batch)).to(dev)
    b = torch.from_numpy(model.embed(bank, device=dev, batch=args.batch)).to(dev)
    idx, dist = [], []
    for s in range(0, len(q), 2048):
        d = torch.cdist(q[s:s + 2048], b)
        v, i = torch.topk(d, args.k, dim=1, largest=False)
        idx.append(i)
        dist.append(v * v)
    return torch.cat(idx).cpu().numpy(), torch.cat(dist).cpu().numpy()


def host_search(model, x, bank):
    q = model.embed(x, device=dev, batch=args.batch).astype(np.float64)
    b = model.embed(bank, device=dev, batch=args.batch).astype(np.float64)
    bb, idx, dist = (b * b).sum(1), [], []
    for s in range(0, len(q), 1024):
        qs = q[s:s + 1024]
        d = np.maximum((qs * qs).sum(1)[:, None] + bb[None, :] - 2.0 * (qs @ b.T), 0.0)
        part = np.argpartition(d, args.k, axis=1)[:, :args.k]
        o = np.argsort(np.take_along_axis(d, part, 1), axis=1, kind="stable")
        idx.append(np.take_along_axis(part, o, 1))
        dist.append(np.take_along_axis(d, idx[-1], 1).astype(np.float32))
    return np.concatenate(idx), np.concatenate(dist)


if args.metric != "l2":
    sys.exit("the comparison paths measure the l2 metric")
n_fit = args.fit_rows
fx, fy = make_glyph_classification(n=n_fit + args.rows + args.bank, shape=shape, classes=10, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x = np.ascontiguousarray(fx[n_fit:n_fit + args.rows])
bank = np.ascontiguousarray(fx[n_fit + args.rows:])
fx, fy = fx[:n_fit], fy[:n_fit]
kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
          dtype=args.dtype, seed=5, backend="hip")
gs = genomes(args.members)
result = {"metric": "neighbors(k={}, {}), queries/s".format(args.k, args.metric), "rows": args.rows,
          "bank": args.bank, "fit_rows": n_fit, "dtype": args.dtype, "reps": args.reps, "batch": args.batch,
          "device": torch.cuda.get_device_name(dev), "cases": {}}
with torch.cuda.device(dev):
    models = []
    if "classifier" in args.models:
        models.append((GeneticCnnModel(fx, fy, gs[0], device=dev, **kw).fit(), "classifier"))
    if "ensemble" in args.models:
        models.append((fit_ensemble(fx, fy, gs, device=dev, **kw), "ensemble_k{}".format(args.members)))

    if args.trace:
        for model, name in models:
            for _ in range(2):
                model.neighbors(x, bank, k=args.k, metric=args.metric, device=dev, batch=args.batch)
            torch.cuda.synchronize(dev)
        print(json.dumps({"trace": [name for _, name in models], "rows": args.rows, "bank": args.bank}), flush=True)
        sys.exit(0)

    for model, name in models:
        paths = {"i_hip_neighbors": lambda: model.neighbors(x, bank, k=args.k, metric=args.metric, device=dev,
                                                            batch=args.batch),
                 "ii_hip_embed_cdist_topk": lambda: cdist_topk(model, x, bank)}
        if not args.no_host:
            paths["iii_hip_embed_host_search"] = lambda: host_search(model, x, bank)
        first, outs, total = {}, {}, {p: [] for p in paths}
        for p, fn in paths.items():                      # warm-up: predictors and states are built here
            first[p], outs[p] = timed(fn)
        for _ in range(args.reps):                       # alternated run by run
            for p, fn in paths.items():
                total[p].append(timed(fn)[0])
        pred = model.hip_predictor(dev, args.batch)
        rec = {"rows_per_launch": pred.EB, "features": pred._nn.G * pred._nn.Ur,
               "index_agreement_i_vs_ii": float((outs["i_hip_neighbors"][0] == outs["ii_hip_embed_cdist_topk"][0]).mean())}
        if not args.no_host:
            rec["index_agreement_i_vs_iii"] = float((outs["i_hip_neighbors"][0] ==
                                                     outs["iii_hip_embed_host_search"][0]).mean())
        for p in paths:
            rec[p] = dict(summary(total[p], args.rows), first_call_ms=round(first[p], 1))
        rec["ii_over_i"] = round(rec["ii_hip_embed_cdist_topk"]["median_ms"] / rec["i_hip_neighbors"]["median_ms"], 3)
        result["cases"][name] = rec
        print(json.dumps({name: rec}), flush=True)
print(json.dumps(result), flush=True)
