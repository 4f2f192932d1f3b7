"""Step time of a population job on hard labels and on soft targets (label smoothing, a target table) at the
headline search space (32x32x3, fp32, batch 32), graph replay, after warm-up; and a distillation record.

Variants, each measured in a fresh child process (``--child``), alternating run by run in one call:

(a) ``--parent DIR``: the same measurement in another built tree (the parent commit), when given;
(b) this tree, both settings off (the train plan holds gt_head);
(c1) this tree, ``label_smoothing=0.1`` (gt_head_soft, two constants);
(c2) this tree, a random valid target table (gt_head_soft, C more floats read per row).

A child builds one population job of ``groups / 5`` random candidates x 5 folds (reset="all": every fold a
group of the same launches), captures the one-step graph exactly as ``FoldJob.launch`` does, replays
``--warmup`` steps and times ``--steps`` replays between two HIP events. The parent process prints one JSON
line: per group count and variant the median and the spread (min .. max) of the runs, (b) - (a) and (c) - (b).

``--accuracy``: a record, not a claim, with one seed -- a k = 4 ensemble teacher and a student of the first
member's genes on 2,000 synthetic glyphs; held-out accuracy of the teacher, the plain student, the smoothed
student and the distilled student at alpha in {0.5, 1.0} and T in {1, 2}.

The kernel's own time comes from a rocprofv3 --kernel-trace --stats run of ``--child`` (tools/gpu.sh cnn-distill).

usage: python tools/bench_distill.py [--groups 25,80] [--reps 5] [--steps 40] [--warmup 10] [--parent DIR]
       python tools/bench_distill.py --accuracy
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--parent", default=None, metavar="DIR", help="a built tree of the parent commit (variant a)")
ap.add_argument("--accuracy", action="store_true", help="instead: the distillation record (see above)")
ap.add_argument("--child", default=None, metavar="ROOT:GROUPS:VARIANT", help="measure one variant (internal)")
args = ap.parse_args()


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
    kw = {"label_smoothing": 0.1} if variant == "smooth" else {}
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-3,), batch_size=32, dtype="fp32", loss="ce", reset="all", **kw)
    members = [(p, folds, list(range(5))) for p in plans]
    if variant == "table":
        from gentun_amd.models.cnn_hip import HipPopJob
        t = np.random.default_rng(0).dirichlet(np.ones(10), size=len(x))
        table = np.ascontiguousarray((t / t.sum(1, keepdims=True)).astype(np.float32))
        job = HipPopJob(None, x, y, None, cfg, dev, members=members, soft_targets=table)
    else:
        job = E.make_population_job("hip", members, x, y, cfg, dev)
    names = [op[1] for op in job._step_plan() if op[0] == "k"]
    assert ("gt_head_soft" in names) == (variant in ("smooth", "table")), names
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
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.utils.data import make_glyph_classification
    x, y = make_glyph_classification(n=2500, shape=(32, 32, 3), classes=10, seed=0, noise=1.0)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    xtr, ytr, xte, lte = x[:2000], y[:2000], x[2000:], np.argmax(y[2000:], 1)
    genomes = [{"S_1": "101", "S_2": "0101110011"}, {"S_1": "000", "S_2": "0000000000"},
               {"S_1": "111", "S_2": "1111111111"}, {"S_1": "011", "S_2": "1010010001"}]
    space = dict(nodes=(3, 5), input_shape=(32, 32, 3), kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
                 dense_units=500, dropout_probability=0.5, classes=10, nfold=5, epochs=(8, 2),
                 learning_rate=(1e-3, 1e-4), batch_size=32, loss="ce", seed=0)

    def held_out(model):
        return round(float((model.predict(xte, output="label") == lte).mean()), 4)
    out = {"data": "make_glyph_classification n=2500 32x32x3, 10 classes, noise 1.0: 2000 training rows, 500 held out",
           "protocol": "fit on all training rows, epochs (8, 2) at lr (1e-3, 1e-4), batch 32, loss ce, seed 0",
           "genes": genomes}
    teacher = fit_ensemble(xtr, ytr, genomes, **space)
    out["teacher_k4"] = held_out(teacher)
    out["teacher_members"] = [held_out(m) for m in teacher.members]
    out["student_plain"] = held_out(GeneticCnnModel(xtr, ytr, genomes[0], **space).fit())
    out["student_smoothed_0.1"] = held_out(GeneticCnnModel(xtr, ytr, genomes[0], label_smoothing=0.1, **space).fit())
    out["student_distilled"] = {}
    for alpha in (0.5, 1.0):
        for T in (1.0, 2.0):
            s = teacher.distill(xtr, ytr, alpha=alpha, temperature=T, **space)
            out["student_distilled"]["alpha{}_T{}".format(alpha, T)] = held_out(s)
    print(json.dumps(out), flush=True)


def run_child(root, groups, variant):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "{}:{}:{}".format(root, groups, variant),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit("bench_distill: child {} failed with {}".format(cmd[-5:], r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    variants = ([("a_parent", os.path.abspath(args.parent), "off")] if args.parent else []) + \
        [("b_off", ROOT, "off"), ("c_smooth", ROOT, "smooth"), ("c_table", ROOT, "table")]
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
        for name in ("c_smooth", "c_table"):
            row[name + "_minus_b_us"] = round((row[name]["median_ms"] - row["b_off"]["median_ms"]) * 1e3, 1)
        if args.parent:
            row["b_minus_a_us"] = round((row["b_off"]["median_ms"] - row["a_parent"]["median_ms"]) * 1e3, 1)
            row["a_spread_us"] = round((row["a_parent"]["max_ms"] - row["a_parent"]["min_ms"]) * 1e3, 1)
            row["b_inside_a_spread"] = row["a_parent"]["min_ms"] <= row["b_off"]["median_ms"] <= row["a_parent"]["max_ms"]
        out["results"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)          # progress: a line per group count
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
            sys.exit("bench_distill needs a GPU")
        main()
