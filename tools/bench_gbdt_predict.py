"""Booster.predict throughput: the MI355X forest predictor (csrc/hip/gbdt_predict.hip) against the CPU predictor
(csrc/gbdt/engine.cpp gbdt_predict) on the same box, same rows, same forest; the two results are compared bit
for bit before anything is timed.

The forest is synthetic (``--trees`` full trees of depth ``--depth`` with random features and thresholds drawn
from the data's range), so the bench does not wait for a training run; a walk costs the same as in a trained
forest of that shape. Reported per predictor: best of ``--reps`` runs; for the GPU both the kernel time and the
time including the row upload and the margin read-back.

usage: python tools/bench_gbdt_predict.py [--rows 1000000] [--features 256] [--trees 500] [--depth 6] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--features", type=int, default=256)
ap.add_argument("--trees", type=int, default=500)
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--classes", type=int, default=1)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--device", default="cuda:0")
args = ap.parse_args()

from gentun_amd.models import gbdt_hip  # noqa: E402
from gentun_amd.models.booster import Booster  # noqa: E402

rng = np.random.default_rng(0)
x = rng.standard_normal((args.rows, args.features), dtype=np.float32)
nn = (2 << args.depth) - 1                      # a full tree in level order: children of i are 2i + 1, 2i + 2
inner = (1 << args.depth) - 1
T = args.trees * args.classes
feature = np.full((T, nn), -1, np.int32)
feature[:, :inner] = rng.integers(0, args.features, (T, inner))
left = np.full((T, nn), -1, np.int32)
left[:, :inner] = 2 * np.arange(inner) + 1
threshold = np.zeros((T, nn), np.float32)
threshold[:, :inner] = rng.standard_normal((T, inner))
bst = Booster(tree_offsets=np.arange(T + 1) * nn, feature=feature, threshold=threshold,
              split_bin=np.where(feature >= 0, 0, -1), left=left, value=0.01 * rng.standard_normal((T, nn)),
              objective=5 if args.classes > 1 else 0, num_class=args.classes, base_margin=0.5,
              n_features=args.features, params={}, history={})

cpu_s, gpu_total_ms, gpu_kernel_ms = [], [], []
for _ in range(args.reps):
    t0 = time.perf_counter()
    cpu = bst.predict(x, output_margin=True, nthreads=args.threads)
    cpu_s.append(time.perf_counter() - t0)
for _ in range(args.reps + 1):                  # the first GPU run also loads the library and creates the context
    out = np.empty((args.rows, args.classes), np.float64)
    ms = []
    gbdt_hip.predict(bst, x, T, out, None, timing=ms)
    gpu_kernel_ms.append(ms[0])
    gpu_total_ms.append(ms[1])
same = out.reshape(cpu.shape).tobytes() == cpu.tobytes()
print(json.dumps({"metric": "Booster.predict, rows/s", "rows": args.rows, "features": args.features,
                  "trees": args.trees, "depth": args.depth, "classes": args.classes,
                  "rows_per_block": gbdt_hip.predict_rows(args.features), "bitwise_equal_to_cpu": same,
                  "gpu_kernel_ms": round(min(gpu_kernel_ms[1:]), 3), "gpu_with_transfers_ms": round(min(gpu_total_ms[1:]), 3),
                  "gpu_first_call_ms": round(gpu_total_ms[0], 3),
                  "cpu_threads": args.threads, "cpu_ms": round(1e3 * min(cpu_s), 3),
                  "gpu_kernel_rows_per_s": round(args.rows / (1e-3 * min(gpu_kernel_ms[1:]))),
                  "gpu_rows_per_s": round(args.rows / (1e-3 * min(gpu_total_ms[1:]))),
                  "cpu_rows_per_s": round(args.rows / min(cpu_s))}), flush=True)
sys.exit(0 if same else 1)
