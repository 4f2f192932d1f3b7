"""Step time of a population job with and without the shift-and-flip augmentation (TrainConfig.augment) at the
headline search space (32x32x3, fp32, batch 32), graph replay, after warm-up.

Variants, each measured in a fresh child process (``--child``), alternating run by run in one call:

(a) ``--parent DIR``: the same measurement in another built tree (the parent commit), when given;
(b) this tree, augmentation off;
(c) this tree, ``{"shift": 4, "flip": True}``.

A child builds one population job of ``groups / 5`` random candidates x 5 folds (reset="all": every fold a
group of the same launches), captures the one-step graph exactly as ``FoldJob.launch`` does, replays
``--warmup`` steps and times ``--steps`` replays between two HIP events. The parent process prints one JSON
line: per group count and variant the median and the spread (min .. max) of the runs, (b) - (a) and (c) - (b),
and the bytes gt_augment moves with their time at ``--hbm-gbs`` (computed from the shapes, not measured).

The kernel's own time comes from a rocprofv3 --kernel-trace --stats run of ``--child`` (tools/gpu.sh cnn-augment).

usage: python tools/bench_augment.py [--groups 25,80] [--reps 3] [--steps 40] [--warmup 10] [--parent DIR]
       python tools/bench_augment.py --accuracy
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--groups", default="25,80")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--parent", default=None, metavar="DIR", help="a built tree of the parent commit (variant a)")
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth for the bound (MI355X: 8 TB/s peak)")
ap.add_argument("--accuracy", action="store_true",
                help="instead: 5-fold validation accuracy of three fixed candidates on the hard synthetic data, "
                     "augmentation off / shift 2 / shift 4 + flip (an observation, no threshold)")
ap.add_argument("--child", default=None, metavar="ROOT:GROUPS:AUG", help="measure one variant (internal)")
args = ap.parse_args()


def child(spec):
    root, groups, aug = spec.split(":")
    sys.path.insert(0, os.path.abspath(root))
    os.environ.setdefault("GENTUN_NO_AUTOBUILD", "1")
    import random
    import numpy as np
    import torch
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.genome import make_plan
    from gentun_amd.utils.data import make_cifar_like, stratified_kfold
    dev = torch.device("cuda", 0)
    P = int(groups) // 5
    x, y = make_cifar_like(n=2500, seed=0)                       # 2000 training rows per fold: 63 steps per epoch
    folds = stratified_kfold(np.argmax(y, 1), 5, seed=0)
    rnd = random.Random(0)
    plans = []
    for _ in range(P):
        g = {"S_1": "".join(rnd.choice("01") for _ in range(3)), "S_2": "".join(rnd.choice("01") for _ in range(10))}
        plans.append(make_plan(g, (3, 5), (32, 32, 3), (20, 50), ((5, 5), (5, 5)), 500, 10))
    kw = {"augment": {"shift": 4, "flip": True}} if aug == "1" else {}
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-3,), batch_size=32, dtype="fp32", loss="ce", reset="all", **kw)
    job = E.make_population_job("hip", [(p, folds, list(range(5))) for p in plans], x, y, cfg, dev)
    assert args.warmup + args.steps <= job.steps_per_epoch
    job.init_params()
    job._k_steps = 1
    graph = job._capture()
    job.reset_optimizer(1e-3)
    job._new_epoch_order()
    for _ in range(args.warmup):
        graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"groups": job.G, "ms_per_step": e0.elapsed_time(e1) / args.steps}), flush=True)


def accuracy():
    import numpy as np
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.utils.data import make_variant_classification
    x, y = make_variant_classification(n=2000, shape=(32, 32, 3), classes=10, seed=0, noise=0.7, label_noise=0.3)
    genomes = [{"S_1": "101", "S_2": "0101110011"}, {"S_1": "000", "S_2": "0000000000"},
               {"S_1": "111", "S_2": "1111111111"}]
    out = {"data": "hard (make_variant_classification n=2000 32x32x3, 10 classes, noise 0.7, label noise 0.3)",
           "protocol": "5 folds, epochs (8, 2) at lr (1e-3, 1e-4), batch 32, loss ce, seed 0", "settings": {}}
    for name, aug in (("off", None), ("shift2", {"shift": 2, "flip": False}), ("shift4_flip", {"shift": 4, "flip": True})):
        rows = []
        for g in genomes:
            m = GeneticCnnModel(x, y, g, (3, 5), (32, 32, 3), (20, 50), ((5, 5), (5, 5)), 500, 0.5, 10, nfold=5,
                                epochs=(8, 2), learning_rate=(1e-3, 1e-4), batch_size=32, loss="ce", seed=0,
                                reset="all", augment=aug)
            m.cross_validate()
            rows.append({"val_cat_acc": round(float(np.mean(m.fold_metrics["categorical_accuracy"])), 4),
                         "val_loss": round(float(np.mean(m.fold_metrics["val_loss"])), 4)})
        out["settings"][name] = rows
    print(json.dumps(out), flush=True)


def run_child(root, groups, aug):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "{}:{}:{}".format(root, groups, aug),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit("bench_augment: child {} failed with {}".format(cmd[-5:], r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    variants = ([("a_parent", os.path.abspath(args.parent), "0")] if args.parent else []) + [("b_off", ROOT, "0"), ("c_on", ROOT, "1")]
    out = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "results": []}
    for groups in (int(g) for g in args.groups.split(",")):
        runs = {name: [] for name, _, _ in variants}
        for _ in range(args.reps):
            for name, root, aug in variants:                    # alternate the variants run by run
                runs[name].append(run_child(root, groups, aug))
        row = {"groups": groups}
        for name, ms in runs.items():
            row[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                         "max_ms": round(max(ms), 4)}
        row["c_minus_b_ms"] = round(row["c_on"]["median_ms"] - row["b_off"]["median_ms"], 4)
        if args.parent:
            row["b_minus_a_ms"] = round(row["b_off"]["median_ms"] - row["a_parent"]["median_ms"], 4)
            row["a_spread_ms"] = round(row["a_parent"]["max_ms"] - row["a_parent"]["min_ms"], 4)
        nbytes = groups * 32 * 32 * 32 * 8 * 4                   # Q B Hp Wp Cp fp32, read once and written once
        row["augment_bytes_in"] = row["augment_bytes_out"] = nbytes
        row["augment_hbm_bound_us"] = round(2 * nbytes / (args.hbm_gbs * 1e9) * 1e6, 2)
        out["results"].append(row)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if args.child:
        child(args.child)
    elif args.accuracy:
        sys.path.insert(0, ROOT)
        accuracy()
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_augment needs a GPU")
        main()
