"""Mixup / CutMix training (TrainConfig.mix) on the CPU: the setting's checks, the draw rule's numpy twin
(gentun_amd/utils/rng.mix_draws) against the loop oracle (tests/mix_ref.py), the torch executor's mixed
batches and target rows against the oracle byte for byte, and the plumbing."""

import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mix_ref as R
from test_cnn_augment import FOLDS, _data, _plan, _space, _stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = {"shift": 2, "flip": True}


@pytest.mark.parametrize("mix,want", [
    (None, None), ({"kind": "mixup"}, {"kind": "mixup", "alpha": 1, "prob": 1.0}),
    ({"kind": "cutmix", "alpha": 8, "prob": 0.25}, {"kind": "cutmix", "alpha": 8, "prob": 0.25}),
    ({}, ValueError), ({"kind": "cutout"}, ValueError), ({"kind": "mixup", "beta": 1}, ValueError),
    ({"kind": "mixup", "alpha": 0}, ValueError), ({"kind": "mixup", "alpha": 9}, ValueError),
    ({"kind": "mixup", "alpha": 1.5}, ValueError), ({"kind": "mixup", "alpha": True}, ValueError),
    ({"kind": "mixup", "prob": 0.0}, ValueError), ({"kind": "mixup", "prob": 1.5}, ValueError),
    ({"kind": "mixup", "prob": float("nan")}, ValueError), ("mixup", ValueError)])
def test_normalize_mix(mix, want):
    from gentun_amd.models import cnn_engine as E
    if want is ValueError:
        for f in (E.normalize_mix, lambda m: E.TrainConfig(mix=m)):
            with pytest.raises(ValueError):
                f(mix)
    else:
        assert E.normalize_mix(mix) == want and E.TrainConfig(mix=mix).mix == want
        assert E.TrainConfig().mix is None


def test_twin_equals_the_oracle():
    from gentun_amd.utils import rng
    P = R.p24_of(0.5)
    seen = set()
    for key in (0, 1, 0x3039, 0xdeadbeef, 0xffffffff):
        for nv in (1, 2, 3, 5, 16):
            for alpha in (1, 2, 3, 8):
                ap, o, m, cy, cx = rng.mix_draws(key, np.arange(24), nv, alpha, P, (6, 5))
                for t in range(24):
                    d = R.draw(key, t, nv, alpha, P, 6, 5)
                    seen.add(d is None)
                    assert bool(ap[t]) == (d is not None) and (nv >= 2 or d is None)
                    if d is not None:
                        assert (int(o[t]), int(m[t])) == (d["o"], d["m"]) and 1 <= d["o"] <= nv - 1
                        box = rng.mix_box(cy[t], cx[t], m[t], 6, 5)
                        assert box == d["box"]
                        for kind in ("mixup", "cutmix"):
                            a, b = rng.mix_weights(kind, m[t], box, 6, 5), R.weights_of(kind, d["m"], d["box"], 6, 5)
                            assert [np.float32(v).tobytes() for v in a] == [np.float32(v).tobytes() for v in b]
    assert seen == {True, False}
    # the edge values of the pure functions: m = 0 pastes the whole partner, m = 2^24 - 1 leaves an empty box
    for f_box, f_w in ((rng.mix_box, rng.mix_weights), (R.box_of, R.weights_of)):
        assert f_box(2, 2, 0, 6, 5) == (0, 5, 0, 5) and f_box(3, 3, 0, 6, 5) == (0, 6, 1, 5)
        assert [float(v) for v in f_w("mixup", 0, None, 6, 5)] == [0.0, 1.0]
        empty = f_box(2, 2, R.ONE24 - 1, 6, 5)
        assert empty == (2, 2, 2, 2)
        assert [float(v) for v in f_w("cutmix", R.ONE24 - 1, empty, 6, 5)] == [1.0, 0.0]
        lam, lam1 = f_w("cutmix", 0, (0, 6, 1, 5), 6, 5)
        assert abs(float(lam) + float(lam1) - 1.0) <= 2.0 ** -23
    # the definition, pinned: (key, step, nv, alpha) -> (o, m, box) at prob 0.5 on a 6 x 5 image
    fixed = [(0x0, 1, 5, 1, (2, 7570771, (2, 6, 2, 5))), (0x1, 1, 2, 3, (1, 9211353, (3, 6, 0, 3))),
             (0x3039, 7, 16, 8, (9, 7716968, (1, 5, 3, 5))), (0xdeadbeef, 64, 3, 2, (1, 9722953, (4, 6, 0, 3))),
             (0xffffffff, 0, 1, 1, None), (0x2a, 1000000, 32, 3, None), (0x7, 3, 5, 1, None),
             (0x7, 4, 5, 1, (3, 8379895, (0, 2, 1, 4)))]
    for key, t, nv, alpha, want in fixed:
        d = R.draw(key, t, nv, alpha, P, 6, 5)
        assert (None if d is None else (d["o"], d["m"], d["box"])) == want


@pytest.mark.parametrize("alpha", [1, 3])
def test_median_rule_is_beta(alpha):
    """Mean and second moment of lam over n = 16384 keys against Beta(alpha, alpha): 1/2 and
    1/4 + 1 / (4 (2 alpha + 1)). A variable in [0, 1] has variance at most 1/4, so the standard error of either
    sample moment is at most 0.5 / sqrt(n); the bound is five of them, 0.0195."""
    from gentun_amd.utils import rng
    n = 16384
    m = rng.mix_draws(np.arange(n) * 2654435761, 3, 8, alpha, R.ONE24, (8, 8))[2]
    lam = m / float(R.ONE24)
    bound = 5 * 0.5 / np.sqrt(n)
    assert abs(lam.mean() - 0.5) < bound
    assert abs((lam ** 2).mean() - (0.25 + 1.0 / (4 * (2 * alpha + 1)))) < bound


def _cfg(mix, aug=None, **kw):
    from gentun_amd.models import cnn_engine as E
    base = dict(epochs=(1,), learning_rate=(1e-2,), batch_size=16, loss="ce", reset="all", augment=aug)
    base.update(kw)
    if mix != "absent":
        base["mix"] = mix
    return E.TrainConfig(**base)


def _record(job, monkeypatch, steps=3):
    """``steps`` train steps over an epoch boundary: (sample ids, global step, batch, target rows) of each."""
    from gentun_amd.models import cnn_engine as E
    seen = []
    gather, forward, loss = job._gather, job._forward, E.loss_and_metrics
    job._gather = lambda idx: (seen.append([idx.clone().numpy(), job.global_step]), gather(idx))[1]
    job._forward = lambda xb, train, nval=None: (seen[-1].append(xb.detach().clone()), forward(xb, train, nval))[1]
    monkeypatch.setattr(E, "loss_and_metrics", lambda lg, yb, mode: (seen[-1].append(yb.clone().numpy()),
                                                                      loss(lg, yb, mode))[1])
    job.init_params()
    job.reset_optimizer(1e-2)
    for s in range(steps):
        if s % job.steps_per_epoch == 0:
            job._new_epoch_order()
        job.train_step()
    job._gather, job._forward = gather, forward
    monkeypatch.setattr(E, "loss_and_metrics", loss)
    return seen


@pytest.mark.parametrize("aug", [None, AUG], ids=["alone", "augment"])
@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_torch_executor_equals_the_oracle(kind, aug, monkeypatch):
    from gentun_amd.models import cnn_engine as E
    x, y = _data()
    xs = np.asarray(x, np.float32)
    mix = {"kind": kind, "alpha": 2, "prob": 1.0}
    job = E.TorchFoldJob(_plan(), x, y, FOLDS, _cfg(mix, aug, label_smoothing=0.1), "cpu", fold_ids=[0, 1])
    t_on, t_off = E.smoothing_targets(0.1, 4)
    rows = np.where(np.asarray(y) > 0, t_on, t_off).astype(np.float32)
    seen = _record(job, monkeypatch, 3)                          # batches of 16, 4 (short), 16
    assert [s[1] for s in seen] == [1, 2, 3]
    for k, (ids, step, xb, yb) in enumerate(seen):
        nv = [4, 4] if k == 1 else [16, 16]
        wx, wt = R.mixed_step(xs, ids, rows[ids], nv, job.aug_seeds, job.fold_ids, step, mix, aug, (8, 8))
        assert _stored(xb, 2).tobytes() == wx.tobytes() and yb.tobytes() == wt.tobytes(), k
        plain = R.augment_batch(xs, ids, job.aug_seeds, job.fold_ids, step, 2 if aug else 0, bool(aug), (8, 8))
        assert wx[:, :nv[0]].tobytes() != plain[:, :nv[0]].tobytes()               # the real rows did change
        assert wx[:, nv[0]:].tobytes() == plain[:, nv[0]:].tobytes()               # the padding rows never


def test_skipped_steps_are_the_plain_step():
    """prob = 1/64: the oracle names the skipped steps; a job trained over them alone equals the plain job."""
    from gentun_amd.models import cnn_engine as E
    x, y = _data()
    mix = {"kind": "mixup", "alpha": 1, "prob": 1.0 / 64}
    flats = []
    for m in (mix, None):
        job = E.TorchFoldJob(_plan(), x, y, FOLDS[:1], _cfg(m, dropout=0.0), "cpu", fold_ids=[0])
        job.init_params()
        job.reset_optimizer(1e-2)
        job._new_epoch_order()
        key = R.key_of(job.aug_seeds[0], 0)
        assert R.draw(key, 1, 16, 1, R.p24_of(mix["prob"]), 8, 8) is None           # step 1 is skipped
        job.train_step()
        flats.append(job.flat.detach().clone())
    assert torch.equal(flats[0], flats[1])


def test_plumbing(tmp_path, monkeypatch):
    """Individual, settings key, checkpoint, command line, and the dp_group refusal."""
    import gentun_amd.__main__ as M
    from gentun_amd import GeneticAlgorithm, GeneticCnnIndividual, Population
    from gentun_amd.checkpoint import load
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.parallel.evaluators import _check_shared_settings, _settings_key
    from gentun_amd.utils import rng
    x, y = _data()
    mix = {"kind": "cutmix", "alpha": 2, "prob": 0.5}
    ind = GeneticCnnIndividual(x, y, genes={'S_1': '101'}, **_space(mix=mix))
    assert ind.get_additional_parameters()["mix"] == mix and ind.copy().build_fitness_model().cfg.mix == mix
    plain, none = (GeneticCnnIndividual(x, y, genes={'S_1': '011'}, **_space(**kw)) for kw in ({}, {"mix": None}))
    assert _settings_key(plain.build_fitness_model()) == _settings_key(none.build_fitness_model())
    with pytest.raises(ValueError, match="differ"):
        _check_shared_settings([(ind, ind.build_fitness_model(), 0), (plain, plain.build_fitness_model(), 1)])
    rng.seed(4)
    pop = Population(GeneticCnnIndividual, x, y, size=2, additional_parameters=_space(mix=mix))
    GeneticAlgorithm(pop, seed=4, checkpoint_dir=str(tmp_path), verbose=False, tournament_size=2).run(1)
    assert load(str(tmp_path))["additional_parameters"]["mix"] == mix
    resumed = GeneticAlgorithm.resume(str(tmp_path), GeneticCnnIndividual, x, y, verbose=False)
    assert all(i.build_fitness_model().cfg.mix == mix for i in resumed.population)
    got = {}
    monkeypatch.setattr(M, "_run_search", lambda args, species, x, y, extra, maximize=True, keep=None:
                        got.update(extra, cfg=species(x, y, **extra).build_fitness_model(device="cpu").cfg))
    base = ["cnn", "--samples", "40", "--input-shape", "8,8,1", "--classes", "4", "--nodes", "3", "--kernels", "4",
            "--kernel-sizes", "3", "--dense", "8"]
    M.main(base + ["--mix", "cutmix", "--mix-alpha", "2", "--mix-prob", "0.5"])
    assert got["mix"] == mix and got["cfg"].mix == mix
    M.main(base)
    assert got["mix"] is None and got["cfg"].mix is None
    with pytest.raises(SystemExit):
        M.mix_setting(argparse.Namespace(mix="mixup", mix_alpha=9, mix_prob=1.0))
    with pytest.raises(ValueError, match="mix with dp_group"):
        E.TorchFoldJob(_plan(), x, y, FOLDS, _cfg(mix, dp_group=object()), "cpu", fold_ids=[0, 1])


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_mix.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"plain", "mixup", "cutmix"} and all(0.0 <= v <= 1.0 for v in out.values())
