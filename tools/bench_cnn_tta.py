"""Test-time augmentation (``predict(tta=...)``) throughput on one GPU at the headline search space (nodes (3, 5),
kernels (20, 50), 5x5 input convs, dense 500, 10 classes) for a ``CnnClassifier`` and a ``CnnEnsemble`` of k = 4,
fitted for one epoch with ``augment={"shift": 2, "flip": True}`` on ``--fit-rows`` glyph images and predicting
``--rows`` held-out ones; V = 2 (``{"flip": True}``) and V = 10 (``{"shift": 2, "flip": True}``) views:

(i)   ``predict(x, tta=...)`` on the HIP predictor: views built on the device (gt_tta_views), one forward launch
      set per chunk of ``EB // V`` rows, the mean over the views in the head (gt_head_tta);
(ii)  the same result without the new kernels: the views in numpy, V plain HIP ``predict`` calls, the ordered
      fp32 combine in numpy -- what a user did before;
(iii) ``backend="torch"`` with ``tta`` on the same GPU.

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. Each case also
reports whether (i) and (ii) are byte-equal and the held-out accuracy without and with TTA.

usage: python tools/bench_cnn_tta.py [--rows 10000] [--fit-rows 2000] [--k 4] [--reps 5] [--device cuda:0]
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
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--device", default="cuda:0")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import combine, fit_ensemble  # noqa: E402
from gentun_amd.models.cnn_fitted import tta_combine, tta_transform, tta_views  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_tta needs a GPU")
dev = torch.device(args.device)
shape = (32, 32, 3)
space = dict(nodes=(3, 5), input_shape=shape, kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
             dense_units=500, classes=10)
AUG = {"shift": 2, "flip": True}
SETTINGS = {"2": {"flip": True}, "10": AUG}
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


fx, fy = make_glyph_classification(n=args.fit_rows + args.rows, shape=shape, classes=10, seed=0, noise=0.5)
fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
x, lab = np.ascontiguousarray(fx[args.fit_rows:]), fy[args.fit_rows:].argmax(1)
fx, fy = fx[:args.fit_rows], fy[:args.fit_rows]
kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
          dtype=args.dtype, seed=5, backend="hip", augment=AUG)
gs = genomes(args.k)
result = {"metric": "predict(output='proba', tta=...), held-out rows/s", "rows": args.rows, "fit_rows": args.fit_rows,
          "dtype": args.dtype, "reps": args.reps, "batch": args.batch, "device": torch.cuda.get_device_name(dev),
          "cases": {}}
with torch.cuda.device(dev):
    clf = GeneticCnnModel(fx, fy, gs[0], device=dev, **kw).fit()
    ens = fit_ensemble(fx, fy, gs, device=dev, **kw)

    for model, name in ((clf, "classifier"), (ens, "ensemble_k{}".format(args.k))):
        plain = model.predict(x, device=dev, output="proba", batch=args.batch)
        for vname, tta in SETTINGS.items():
            views = tta_views(tta, shape)

            def by_hand():
                # before tta=: the views on the host, V plain calls, the combine on the host. For the ensemble the
                # mean over the views is taken per member before the members are combined, as tta= defines it.
                if model is clf:
                    return tta_combine([clf.predict(tta_transform(x, *v), device=dev, output="proba", batch=args.batch)
                                        for v in views])
                per = [ens.predict(tta_transform(x, *v), device=dev, output="member_proba", batch=args.batch)
                       for v in views]
                return combine(tta_combine(per), ens.weights)[0]

            paths = {
                "i_hip_tta": lambda: model.predict(x, device=dev, output="proba", batch=args.batch, tta=tta),
                "ii_hip_views_by_hand": by_hand,
                "iii_torch_backend": lambda: model.predict(x, device=dev, output="proba", batch=args.batch,
                                                           backend="torch", tta=tta),
            }
            first, outs, total = {}, {}, {p: [] for p in paths}
            for p, fn in paths.items():                  # warm-up: predictors and TTA state are built here
                first[p], outs[p] = timed(fn)
            for _ in range(args.reps):                   # alternated run by run
                for p, fn in paths.items():
                    total[p].append(timed(fn)[0])
            pred = model.hip_predictor(dev, args.batch)
            st = pred.tta_state(views)
            rec = {"views": len(views), "rows_per_launch": pred.EB, "raw_rows_per_launch": st.R,
                   "chunks": -(-args.rows // st.R),
                   "i_equals_ii": outs["i_hip_tta"].tobytes() == outs["ii_hip_views_by_hand"].tobytes(),
                   "max_abs_proba_diff_i_vs_iii": float(np.abs(outs["i_hip_tta"].astype(np.float64)
                                                                - outs["iii_torch_backend"]).max()),
                   "accuracy_plain": float((plain.argmax(1) == lab).mean()),
                   "accuracy_tta": float((outs["i_hip_tta"].argmax(1) == lab).mean())}
            for p in paths:
                rec[p] = dict(summary(total[p], args.rows), first_call_ms=round(first[p], 1))
            rec["ii_over_i"] = round(rec["ii_hip_views_by_hand"]["median_ms"] / rec["i_hip_tta"]["median_ms"], 3)
            rec["iii_over_i"] = round(rec["iii_torch_backend"]["median_ms"] / rec["i_hip_tta"]["median_ms"], 3)
            result["cases"]["{}_V{}".format(name, vname)] = rec
print(json.dumps(result), flush=True)
