"""Feature-space Gaussian (``gaussian_fit`` / ``mahalanobis``) on one GPU at the headline search space (nodes (3, 5),
kernels (20, 50), 5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` fitted for one epoch on
``--fit-rows`` glyph images: a bank of ``--bank`` images, ``--rows`` query images:

(i)   ``gaussian_fit(bank, labels, device=...)`` then ``mahalanobis(x, stats, device=...)`` on the HIP path;
(ii)  ``embed`` of both on the HIP path, then torch fp32 on the same GPU: per-class means, ``Xc.T @ Xc``, the fp64
      host factorisation of (i), and ``cdist`` of the whitened queries to the whitened means;
(iii) ``embed`` of both on the HIP path, then fp64 BLAS on the host (not the sequential-sum definition of
      ``gaussian_moments``, which is far slower).

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the paths
alternate run by run in this one process and the median of ``--reps`` runs is reported as the last JSON line.
``--trace`` is the child of a kernel trace run of its own (``tools/gpu.sh cnn-gaussian``): fit, two calls, exit.

usage: python tools/bench_cnn_gaussian.py [--rows 10000] [--bank 50000] [--fit-rows 2000] [--reps 5]
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
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--shrink", type=float, default=0.01)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--trace", action="store_true", help="fit, call gaussian_fit and mahalanobis twice and exit")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_fitted import gaussian_stats  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_gaussian needs a GPU")
dev = torch.device(args.device)
shape, C = (32, 32, 3), 10
n_fit = args.fit_rows
fx, fy = make_glyph_classification(n=n_fit + args.rows + args.bank, shape=shape, classes=C, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x = np.ascontiguousarray(fx[n_fit:n_fit + args.rows])
bank, lab = np.ascontiguousarray(fx[n_fit + args.rows:]), fy[n_fit + args.rows:].argmax(1)
model = GeneticCnnModel(fx[:n_fit], fy[:n_fit], {"S_1": "101", "S_2": "0101110011"}, nodes=(3, 5), input_shape=shape,
                        kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)), dense_units=500, classes=C,
                        dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
                        dtype=args.dtype, seed=5, backend="hip", device=dev).fit()
kw = dict(device=dev, batch=args.batch)


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0), out


def hip():
    st = model.gaussian_fit(bank, labels=lab, shrink=args.shrink, **kw)
    return st, model.mahalanobis(x, st, **kw)


def moments(xp, b, onehot, count):
    mean = (onehot.T @ b) / xp.clip(count, 1, None)[:, None]
    c = b - onehot @ mean
    return mean, (c.T @ c) / len(b)


def torch32():
    b = torch.from_numpy(model.embed(bank, **kw)).to(dev)
    q = torch.from_numpy(model.embed(x, **kw)).to(dev)
    oh = torch.from_numpy(np.eye(C, dtype=np.float32)[lab]).to(dev)
    mean, cov = moments(torch, b, oh, oh.sum(0))
    st = gaussian_stats(np.bincount(lab, minlength=C), mean.cpu().numpy()[None], cov.double().cpu().numpy()[None],
                        args.shrink)
    W = torch.from_numpy(st["whiten"][0]).to(dev)
    d = torch.cdist(q @ W, torch.from_numpy(st["wmean"][0]).to(dev))
    return st, (d * d).cpu().numpy()


def host64():
    b, q = model.embed(bank, **kw).astype(np.float64), model.embed(x, **kw).astype(np.float64)
    oh = np.eye(C)[lab]
    mean, cov = moments(np, b, oh, oh.sum(0))
    st = gaussian_stats(np.bincount(lab, minlength=C), mean.astype(np.float32)[None], cov[None], args.shrink)
    z = q @ st["whiten"][0].astype(np.float64)
    return st, ((z[:, None, :] - st["wmean"][0][None].astype(np.float64)) ** 2).sum(-1).astype(np.float32)


with torch.cuda.device(dev):
    if args.trace:
        for _ in range(2):
            hip()
        torch.cuda.synchronize(dev)
        print(json.dumps({"trace": "classifier", "rows": args.rows, "bank": args.bank}), flush=True)
        sys.exit(0)
    paths = {"i_hip_gaussian": hip, "ii_hip_embed_torch_fp32": torch32, "iii_hip_embed_host_fp64": host64}
    first, outs, total = {}, {}, {p: [] for p in paths}
    for p, fn in paths.items():
        first[p], outs[p] = timed(fn)
    for _ in range(args.reps):
        for p, fn in paths.items():
            total[p].append(timed(fn)[0])
ref = outs["iii_hip_embed_host_fp64"][1].astype(np.float64)
rec = {"metric": "gaussian_fit + mahalanobis, ms per call pair", "rows": args.rows, "bank": args.bank,
       "fit_rows": n_fit, "dtype": args.dtype, "reps": args.reps, "batch": args.batch, "shrink": args.shrink,
       "device": torch.cuda.get_device_name(dev)}
for p in paths:
    rec[p] = {"median_ms": round(statistics.median(total[p]), 3), "best_ms": round(min(total[p]), 3),
              "first_call_ms": round(first[p], 1),
              "rel_distance_error_vs_iii": float(np.abs(outs[p][1] - ref).max() / np.abs(ref).max()),
              "label_agreement_vs_iii": float((outs[p][1].argmin(1) == ref.argmin(1)).mean())}
rec["ii_over_i"] = round(rec["ii_hip_embed_torch_fp32"]["median_ms"] / rec["i_hip_gaussian"]["median_ms"], 3)
print(json.dumps(rec), flush=True)
