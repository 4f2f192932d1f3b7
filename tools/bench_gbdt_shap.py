"""Booster.predict(pred_contribs=True) throughput: the MI355X SHAP kernel (csrc/hip/gbdt_shap.hip) against the CPU
predictor (csrc/gbdt/engine.cpp gbdt_predict_contribs) on the same box, same rows, same forest; the two outputs
are compared byte for byte.

The forest is synthetic (``--trees`` full trees of depth ``--depth`` with random features, thresholds drawn from
the data's range and covers that halve, unevenly, at every split), so the bench does not wait for a training run;
a leaf costs the same as in a trained forest of that shape. Reported: the GPU's kernel time and its time
including the table build, the row upload and the read-back (best of ``--reps`` runs after a first call that
loads the library), and the CPU predictor with ``--threads`` threads (best of ``--cpu-reps``).

``--interactions`` measures Booster.predict(pred_interactions=True) instead (csrc/hip/gbdt_shap_inter.hip against
gbdt_predict_interactions), in the same way; ``--splits 0,1,16`` then times the kernel with each feature-axis
split in turn (0: its own choice), alternating them within every repetition, and compares every output.

usage: python tools/bench_gbdt_shap.py [--rows 200000] [--features 256] [--trees 500] [--depth 6] [--threads 16]
                                       [--interactions [--splits 0,1]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--features", type=int, default=256)
ap.add_argument("--trees", type=int, default=500)
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--classes", type=int, default=1)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--cpu-reps", type=int, default=1, help="0: GPU timings only, nothing is compared")
ap.add_argument("--interactions", action="store_true", help="pred_interactions instead of pred_contribs")
ap.add_argument("--splits", default="0", help="with --interactions: feature-axis splits to time, 0 = the kernel's choice")
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
cover = np.zeros((T, nn))
cover[:, 0] = args.rows
for i in range(inner):
    share = rng.uniform(0.2, 0.8, T)
    cover[:, 2 * i + 1] = cover[:, i] * share
    cover[:, 2 * i + 2] = cover[:, i] - cover[:, 2 * i + 1]
bst = Booster(tree_offsets=np.arange(T + 1) * nn, feature=feature, threshold=threshold,
              split_bin=np.where(feature >= 0, 0, -1), left=left, value=0.01 * rng.standard_normal((T, nn)),
              objective=5 if args.classes > 1 else 0, num_class=args.classes, base_margin=0.5,
              n_features=args.features, params={}, history={}, cover=cover, gain=np.zeros((T, nn)))

if args.interactions:
    splits = [int(v) for v in args.splits.split(",")]
    F1 = args.features + 1
    outs = {sp: np.empty((args.rows, args.classes, F1, F1), np.float64) for sp in splits}
    kernel_ms, total_ms = {sp: [] for sp in splits}, {sp: [] for sp in splits}
    for _ in range(args.reps + 1):              # the first GPU run also loads the library and creates the context
        for sp in splits:
            ms = []
            gbdt_hip.predict_interactions(bst, x, T, outs[sp], timing=ms, split=sp)
            kernel_ms[sp].append(ms[0])
            total_ms[sp].append(ms[1])
    cpu_s, cpu = [], None
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        cpu = bst.predict(x, pred_interactions=True, nthreads=args.threads)
        cpu_s.append(time.perf_counter() - t0)
    ref = cpu if cpu_s else outs[splits[0]]
    same = all(o.reshape(ref.shape).tobytes() == ref.tobytes() for o in outs.values())
    nm = min(1000, args.rows)
    margin = bst.predict(x[:nm], output_margin=True).reshape(nm, args.classes)
    additive = float(np.abs(outs[splits[0]][:nm].sum(axis=(2, 3)) - margin).max())
    plan = gbdt_hip.shap_inter_plan(args.rows, args.features, args.classes)
    best = splits[0]
    print(json.dumps({"metric": "Booster.predict(pred_interactions=True), rows/s", "rows": args.rows,
                      "features": args.features, "trees": args.trees, "depth": args.depth, "classes": args.classes,
                      "chunk_rows": plan[0], "chosen_split": plan[1],
                      "bytewise_equal_to_cpu" if cpu_s else "splits_bytewise_equal": same,
                      "max_abs_sum_minus_margin_first_1000_rows": additive,
                      "gpu_kernel_ms": round(min(kernel_ms[best][1:]), 3),
                      "gpu_with_transfers_ms": round(min(total_ms[best][1:]), 3),
                      "gpu_first_call_ms": round(total_ms[best][0], 3),
                      "gpu_kernel_ms_by_split": {str(sp): [round(v, 3) for v in kernel_ms[sp][1:]] for sp in splits},
                      "cpu_threads": args.threads, "cpu_ms": round(1e3 * min(cpu_s), 3) if cpu_s else None,
                      "gpu_kernel_rows_per_s": round(args.rows / (1e-3 * min(kernel_ms[best][1:]))),
                      "gpu_rows_per_s": round(args.rows / (1e-3 * min(total_ms[best][1:]))),
                      "cpu_rows_per_s": round(args.rows / min(cpu_s)) if cpu_s else None}), flush=True)
    sys.exit(0 if same else 1)

gpu_total_ms, gpu_kernel_ms = [], []
out = np.empty((args.rows, args.classes, args.features + 1), np.float64)
for _ in range(args.reps + 1):                  # the first GPU run also loads the library and creates the context
    ms = []
    gbdt_hip.predict_contribs(bst, x, T, out, timing=ms)
    gpu_kernel_ms.append(ms[0])
    gpu_total_ms.append(ms[1])
cpu_s, cpu = [], None
for _ in range(args.cpu_reps):
    t0 = time.perf_counter()
    cpu = bst.predict(x, pred_contribs=True, nthreads=args.threads)
    cpu_s.append(time.perf_counter() - t0)
same = out.reshape(cpu.shape).tobytes() == cpu.tobytes() if cpu_s else None
margin = bst.predict(x[:1000], output_margin=True).reshape(1000, args.classes)
additive = float(np.abs(out[:1000].sum(axis=2) - margin).max())
print(json.dumps({"metric": "Booster.predict(pred_contribs=True), rows/s", "rows": args.rows, "features": args.features,
                  "trees": args.trees, "depth": args.depth, "classes": args.classes,
                  "rows_per_block": gbdt_hip.shap_rows(args.features), "bytewise_equal_to_cpu": same,
                  "max_abs_sum_minus_margin_first_1000_rows": additive,
                  "gpu_kernel_ms": round(min(gpu_kernel_ms[1:]), 3), "gpu_with_transfers_ms": round(min(gpu_total_ms[1:]), 3),
                  "gpu_first_call_ms": round(gpu_total_ms[0], 3),
                  "cpu_threads": args.threads, "cpu_ms": round(1e3 * min(cpu_s), 3) if cpu_s else None,
                  "gpu_kernel_rows_per_s": round(args.rows / (1e-3 * min(gpu_kernel_ms[1:]))),
                  "gpu_rows_per_s": round(args.rows / (1e-3 * min(gpu_total_ms[1:]))),
                  "cpu_rows_per_s": round(args.rows / min(cpu_s)) if cpu_s else None}), flush=True)
sys.exit(1 if same is False else 0)
