"""CnnClassifier.predict throughput on one GPU: the HIP predictor (gentun_amd/models/cnn_fitted.py HipPredictor:
the executor's forward-only launches + gt_head_predict) at 32 and 256 rows per launch against the stock-torch
forward (``backend="torch"``) on the same device, same rows, same parameters.

The model is the headline search space (nodes (3, 5), kernels (20, 50), 5x5 input convs, dense 500, 10 classes)
with one mid-density genome and random Glorot-scaled parameters, so the bench does not wait for a training run;
a forward costs the same as with trained parameters. Two timings per path, after one warm-up call of every
shape: ``total`` -- ``predict(output="proba")`` from host array to host array (upload, compute, read-back; host
clock around a call that ends in a device synchronise) -- and ``compute`` -- the launches of every chunk on
device-resident input between two HIP events. Median and best of ``--reps`` runs.

usage: python tools/bench_cnn_predict.py [--rows 10000] [--reps 5] [--device cuda:0]
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
ap.add_argument("--genes", default="101,0101110011")
ap.add_argument("--device", default="cuda:0")
args = ap.parse_args()

from gentun_amd.models.cnn_fitted import CnnClassifier  # noqa: E402
from gentun_amd.models.genome import make_plan  # noqa: E402

genes = dict(zip(("S_1", "S_2"), args.genes.split(",")))
space = dict(nodes=(3, 5), input_shape=(32, 32, 3), kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
             dense_units=500, classes=10)
rng = np.random.default_rng(0)
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
clf = CnnClassifier(genes, params=params, dtype=args.dtype, **space)
x = rng.random((args.rows, 32, 32, 3), dtype=np.float32)
if not torch.cuda.is_available():
    sys.exit("bench_cnn_predict needs a GPU")
dev = torch.device(args.device)


def timed(fn):
    """ms of ``fn()`` by the host clock (``fn`` ends in a device synchronise)."""
    t0 = time.perf_counter()
    out = fn()
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


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "best_ms": round(min(ms), 3),
            "rows_per_s": round(args.rows / (1e-3 * statistics.median(ms)))}


result = {"metric": "CnnClassifier.predict(output='proba'), rows/s", "rows": args.rows, "genes": genes,
          "dtype": args.dtype, "reps": args.reps, "device": torch.cuda.get_device_name(dev), "paths": {}}
probas = {}
with torch.cuda.device(dev):
    for name, kw in (("hip_batch32", dict(batch=32)), ("hip_batch256", dict(batch=256)),
                     ("torch_batch256", dict(batch=256, backend="torch"))):
        first_ms, probas[name] = timed(lambda: clf.predict(x, device=dev, output="proba", **kw))     # warm-up
        total = [timed(lambda: clf.predict(x, device=dev, output="proba", **kw))[0] for _ in range(args.reps)]
        B = kw["batch"]
        nch = -(-args.rows // B)
        if "backend" in kw:
            P = clf._tensors(dev, torch.float32)
            chunks = [torch.from_numpy(np.ascontiguousarray(x[s:s + B].transpose(0, 3, 1, 2))).to(dev)
                      for s in range(0, args.rows, B)]

            def compute():
                with torch.no_grad():
                    for xb in chunks:
                        torch.softmax(clf._torch_forward(xb, P), dim=-1)
        else:
            pred = clf.hip_predictor(dev, B)
            pred.upload(x[:pred.EB])

            def compute():
                for _ in range(nch):
                    pred.forward()
        compute()
        comp = [events(compute) for _ in range(args.reps)]
        result["paths"][name] = {"first_call_ms": round(first_ms, 1), "launches_of": B, "chunks": nch,
                                 "total": summary(total), "compute": summary(comp)}
ref = probas["torch_batch256"].astype(np.float64)
result["max_abs_proba_diff_vs_torch"] = {k: float(np.abs(v - ref).max()) for k, v in probas.items() if k.startswith("hip")}
result["hip_batch32_equals_batch256"] = probas["hip_batch32"].tobytes() == probas["hip_batch256"].tobytes()
t, h = result["paths"]["torch_batch256"], result["paths"]["hip_batch256"]
result["hip256_over_torch"] = {"total": round(t["total"]["median_ms"] / h["total"]["median_ms"], 3),
                               "compute": round(t["compute"]["median_ms"] / h["compute"]["median_ms"], 3)}
print(json.dumps(result), flush=True)
