"""CnnEnsemble.predict throughput on one GPU at the headline search space (nodes (3, 5), kernels (20, 50), 5x5
input convs, dense 500, 10 classes), k members of distinct random genomes with random Glorot-scaled parameters:

(a) ``CnnEnsemble.predict(output="proba")`` on the HIP predictor (one k-group launch set + gt_head_ensemble);
(b) the way without the ensemble: the same k ``CnnClassifier.predict`` calls one after another on their own HIP
    predictors, plus the numpy combine;
(c) ``backend="torch"`` on the same GPU.

Host array to host array, every call ending in a device synchronise; one warm-up call of every path, then the
paths alternate run by run in this one process and the median of ``--reps`` runs is reported. The device time
of (a) alone (the launches of every chunk on device-resident input) comes from two HIP events. (a) and (b)
must be byte-equal. With ``--fit-rows`` > 0 the tool also times ``fit_ensemble`` of the k members (one
population job) against k ``GeneticCnnModel.fit()`` calls, one epoch each, first call of each way after one
warm-up fit of a single member (library load, kernel selection).

usage: python tools/bench_cnn_ensemble.py [--rows 10000] [--k 4,16] [--reps 5] [--fit-rows 2000] [--device cuda:0]
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
ap.add_argument("--k", default="4,16")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--fit-rows", type=int, default=2000)
ap.add_argument("--device", default="cuda:0")
args = ap.parse_args()

from gentun_amd.models.cnn import GeneticCnnModel  # noqa: E402
from gentun_amd.models.cnn_ensemble import CnnEnsemble, combine, fit_ensemble  # noqa: E402
from gentun_amd.models.cnn_fitted import CnnClassifier  # noqa: E402
from gentun_amd.models.genome import make_plan  # noqa: E402
from gentun_amd.utils.data import make_glyph_classification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_cnn_ensemble needs a GPU")
dev = torch.device(args.device)
space = dict(nodes=(3, 5), input_shape=(32, 32, 3), kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
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


def classifier(genes):
    plan = make_plan(genes, **space)
    params = {}
    for st in plan.convs():
        fan = st.cin * st.k[0] * st.k[1]
        params[st.name + ".w"] = (rng.standard_normal((st.cout, st.cin) + tuple(st.k)) / np.sqrt(fan)).astype(np.float32)
        params[st.name + ".b"] = (0.1 * rng.standard_normal(st.cout)).astype(np.float32)
    params["dense1.w"] = (rng.standard_normal((plan.flatten, 500)) / np.sqrt(plan.flatten)).astype(np.float32)
    params["dense1.b"] = (0.1 * rng.standard_normal(500)).astype(np.float32)
    params["dense2.w"] = (rng.standard_normal((500, 10)) / np.sqrt(500)).astype(np.float32)
    params["dense2.b"] = (0.1 * rng.standard_normal(10)).astype(np.float32)
    return CnnClassifier(genes, params=params, dtype=args.dtype, **space)


def timed(fn):
    """ms of ``fn()`` by the host clock (``fn`` ends in a device synchronise)."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0), out


def events(fn):
    """Device ms of the launches ``fn()`` enqueues."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms, rows):
    return {"median_ms": round(statistics.median(ms), 3), "best_ms": round(min(ms), 3),
            "rows_per_s": round(rows / (1e-3 * statistics.median(ms)))}


x = rng.random((args.rows, 32, 32, 3), dtype=np.float32)
result = {"metric": "CnnEnsemble.predict(output='proba'), rows/s", "rows": args.rows, "dtype": args.dtype,
          "reps": args.reps, "batch": args.batch, "device": torch.cuda.get_device_name(dev), "k": {}}
with torch.cuda.device(dev):
    for k in [int(v) for v in args.k.split(",")]:
        ens = CnnEnsemble([classifier(g) for g in genomes(k)])
        paths = {
            "a_hip_ensemble": lambda: ens.predict(x, device=dev, output="proba", batch=args.batch),
            "b_hip_members_one_by_one": lambda: combine(
                np.stack([m.predict(x, device=dev, output="proba", batch=args.batch) for m in ens.members]),
                ens.weights)[0],
            "c_torch_backend": lambda: ens.predict(x, device=dev, output="proba", batch=args.batch, backend="torch"),
        }
        first, outs, total = {}, {}, {name: [] for name in paths}
        for name, fn in paths.items():                   # warm-up: predictors are built here
            first[name], outs[name] = timed(fn)
        for _ in range(args.reps):                       # alternated run by run
            for name, fn in paths.items():
                total[name].append(timed(fn)[0])
        assert outs["a_hip_ensemble"].tobytes() == outs["b_hip_members_one_by_one"].tobytes(), \
            "the ensemble's launches and the members one by one disagree"
        pred = ens.hip_predictor(dev, args.batch)
        nch = -(-args.rows // pred.EB)
        pred.upload(x[:pred.EB])

        def compute():
            for _ in range(nch):
                pred.forward()
        compute()
        comp = [events(compute) for _ in range(args.reps)]
        rec = {"rows_per_launch": pred.EB, "chunks": nch, "a_equals_b": True,
               "max_abs_proba_diff_a_vs_c": float(np.abs(outs["a_hip_ensemble"].astype(np.float64)
                                                         - outs["c_torch_backend"]).max()),
               "a_device_compute": summary(comp, args.rows)}
        for name in paths:
            rec[name] = dict(summary(total[name], args.rows), first_call_ms=round(first[name], 1))
        rec["b_over_a"] = round(rec["b_hip_members_one_by_one"]["median_ms"] / rec["a_hip_ensemble"]["median_ms"], 3)
        rec["c_over_a"] = round(rec["c_torch_backend"]["median_ms"] / rec["a_hip_ensemble"]["median_ms"], 3)
        result["k"][str(k)] = rec
        del ens, pred
        if args.fit_rows > 0:
            fx, fy = make_glyph_classification(n=args.fit_rows, shape=(32, 32, 3), classes=10, seed=0, noise=0.5)
            fx, fy = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
            kw = dict(space, dropout_probability=0.5, nfold=5, epochs=(1,), learning_rate=(1e-3,), batch_size=32,
                      dtype=args.dtype, seed=5, backend="hip")
            gs = genomes(k)
            GeneticCnnModel(fx, fy, gs[0], device=dev, **kw).fit()                   # warm-up
            t_ens, fitted = timed(lambda: fit_ensemble(fx, fy, gs, device=dev, **kw))
            t_one, alone = timed(lambda: [GeneticCnnModel(fx, fy, g, device=dev, **kw).fit() for g in gs])
            same = all(a.params[n].tobytes() == m.params[n].tobytes()
                       for a, m in zip(alone, fitted.members) for n in a.params)
            rec["fit"] = {"rows": args.fit_rows, "epochs": 1, "fit_ensemble_ms": round(t_ens, 1),
                          "k_fit_calls_ms": round(t_one, 1), "k_fits_over_fit_ensemble": round(t_one / t_ens, 3),
                          "members_equal_fits_alone": same}
print(json.dumps(result), flush=True)
