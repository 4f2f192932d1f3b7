"""Step time of a population job with mixup / CutMix (TrainConfig.mix) at the headline search space (32x32x3,
fp32, batch 32), graph replay, after warm-up.

Variants, each measured in a fresh child process (``--child``), alternating run by run in one call:

    parent_off, parent_aug   ``--parent DIR``: another built tree (the parent commit), without and with
                             ``augment={"shift": 4, "flip": True}``, when given
    off, aug                 this tree, the same two settings (``mix=None``)
    mixup, cutmix            this tree, ``mix={"kind": ..., "alpha": 1, "prob": 1.0}``
    aug+mixup, aug+cutmix    the same with the augmentation on

A child builds one population job of ``groups / 5`` random candidates x 5 folds (reset="all"), captures the
one-step graph exactly as ``FoldJob.launch`` does, replays ``--warmup`` steps and times ``--steps`` replays
between two HIP events. The parent process prints one JSON line: per group count and variant the median and
the spread (min .. max) of the runs, and the bytes gt_augment_mix must move with their time at ``--hbm-gbs``
(computed from the shapes, not measured): one read and one write of the batch for cutmix, two reads and one
write for mixup.

The kernels' own time comes from a rocprofv3 --kernel-trace --stats run of ``--child`` (tools/gpu.sh cnn-mix).

usage: python tools/bench_cnn_mix.py [--groups 25,80] [--reps 5] [--steps 40] [--warmup 10] [--parent DIR]
       python tools/bench_cnn_mix.py --accuracy
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = {"shift": 4, "flip": True}

ap = argparse.ArgumentParser()
ap.add_argument("--groups", default="25,80")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--parent", default=None, metavar="DIR", help="a built tree of the parent commit")
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth for the bound (MI355X: 8 TB/s peak)")
ap.add_argument("--accuracy", action="store_true",
                help="instead: held-out accuracy of one candidate on the synthetic glyphs without mixing, with "
                     "mixup and with cutmix, one seed (a record, no threshold)")
ap.add_argument("--child", default=None, metavar="ROOT:GROUPS:VARIANT", help="measure one variant (internal)")
args = ap.parse_args()


def settings(variant):
    kw = {}
    for part in variant.split("+"):
        if part == "aug":
            kw["augment"] = AUG
        elif part == "smooth":                                  # the soft-target head, for the kernel trace
            kw["label_smoothing"] = 0.1
        elif part in ("mixup", "cutmix"):
            kw["mix"] = {"kind": part, "alpha": 1, "prob": 1.0}
    return kw


def child(spec):
    root, groups, variant = spec.split(":")
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
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-3,), batch_size=32, dtype="fp32", loss="ce", reset="all",
                        **settings(variant))
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
    from gentun_amd.utils.data import make_glyph_classification
    x, y = make_glyph_classification(n=2500, shape=(32, 32, 3), classes=10, seed=0, noise=1.0)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    xt, yt, xh, yh = x[:2000], y[:2000], x[2000:], y[2000:]
    out = {"data": "make_glyph_classification n=2500 32x32x3, 10 classes, noise 1.0: 2000 rows to fit, 500 held out",
           "protocol": "fit(), epochs (8, 2) at lr (1e-3, 1e-4), batch 32, loss ce, seed 0, one candidate", "held_out": {}}
    for name in ("plain", "mixup", "cutmix"):
        mix = None if name == "plain" else {"kind": name, "alpha": 1, "prob": 1.0}
        m = GeneticCnnModel(xt, yt, {"S_1": "101", "S_2": "0101110011"}, (3, 5), (32, 32, 3), (20, 50),
                            ((5, 5), (5, 5)), 500, 0.5, 10, nfold=5, epochs=(8, 2), learning_rate=(1e-3, 1e-4),
                            batch_size=32, loss="ce", seed=0, reset="all", mix=mix)
        pred = np.asarray(m.fit().predict(xh))
        pred = pred.argmax(1) if pred.ndim == 2 else pred
        out["held_out"][name] = round(float((pred == yh.argmax(1)).mean()), 4)
    print(json.dumps(out), flush=True)


def run_child(root, groups, variant):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "{}:{}:{}".format(root, groups, variant),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit("bench_cnn_mix: child {} failed with {}".format(cmd[-5:], r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    variants = [("parent_" + v, os.path.abspath(args.parent), v) for v in ("off", "aug")] if args.parent else []
    variants += [(v, ROOT, v) for v in ("off", "aug", "mixup", "cutmix", "aug+mixup", "aug+cutmix")]
    out = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "results": []}
    for groups in (int(g) for g in args.groups.split(",")):
        runs = {name: [] for name, _, _ in variants}
        for _ in range(args.reps):
            for name, root, variant in variants:                # alternate the variants run by run
                runs[name].append(run_child(root, groups, variant))
        row = {"groups": groups}
        for name, ms in runs.items():
            row[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                         "max_ms": round(max(ms), 4)}
        nbytes = groups * 32 * 32 * 32 * 8 * 4                   # Q B Hp Wp Cp fp32: one pass over the batch
        row["batch_bytes"] = nbytes
        row["cutmix_hbm_bound_us"] = round(2 * nbytes / (args.hbm_gbs * 1e9) * 1e6, 2)
        row["mixup_hbm_bound_us"] = round(3 * nbytes / (args.hbm_gbs * 1e9) * 1e6, 2)
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
            sys.exit("bench_cnn_mix needs a GPU")
        main()
