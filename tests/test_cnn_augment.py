"""Shift-and-flip training augmentation (TrainConfig.augment) on the CPU: the draw rule and its numpy twin
(gentun_amd/utils/rng.py), the oracle (tests/augment_ref.py) checked by hand, the torch executor's augmented
batches against the oracle byte for byte, determinism, data parallelism and the plumbing from the command
line and the individual down to the training config."""

import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUG = {"shift": 2, "flip": True}


# ------------------------------------------------------------------ draws
def test_draw_statistics_and_fixed_vector():
    from gentun_amd.utils import rng
    for seed in (0, 1, 12345, 0xdeadbeef):
        for fid in (0, 3, 5):
            key = rng.aug_key(seed, fid)
            assert key == R.key_of(seed, fid)
            dy, dx, fl = rng.aug_draws(key, np.arange(64)[:, None], np.arange(32)[None, :], 4, True)
            assert dy.shape == (64, 32)
            for v in (dy, dx):
                counts = np.bincount((v + 4).ravel(), minlength=9)
                assert len(counts) == 9 and counts.min() >= 170 and counts.max() <= 290, counts
            assert 0.45 <= fl.mean() <= 0.55
            # the twin and the oracle's scalar rule agree draw by draw
            for t, r in ((0, 0), (5, 7), (63, 31)):
                assert (dy[t, r], dx[t, r], fl[t, r]) == R.draw(key, t, r, 4, True)
    # the definition, pinned: (key, step, row) -> (dy, dx, flip) at shift 4
    fixed = [(0x0, 1, 0, (4, 4, 1)), (0x1, 1, 5, (-2, 1, 0)), (0x3039, 7, 31, (-4, 3, 0)),
             (0xdeadbeef, 64, 3, (0, 4, 1)), (0x632be5ab, 2, 16, (-2, -4, 1)), (0xffffffff, 0, 0, (0, 4, 0)),
             (0x2a, 1000000, 17, (-2, -4, 1)), (0x7, 3, 47, (-1, 4, 0))]
    for key, t, r, want in fixed:
        dy, dx, fl = rng.aug_draws(key, t, np.asarray([r]), 4, True)
        assert (int(dy[0]), int(dx[0]), int(fl[0])) == want
        assert R.draw(key, t, r, 4, True) == want
    dy, dx, fl = rng.aug_draws(7, 3, np.arange(50), 0, True)
    assert not dy.any() and not dx.any() and fl.any()
    assert not rng.aug_draws(7, 3, np.arange(50), 3, False)[2].any()
    assert int(rng.hash4(1, 2, 3, 4)) == R.hash4(1, 2, 3, 4) and int(rng.mix32(0xffffffff)) == R.mix32(0xffffffff)


# ------------------------------------------------------------------ the oracle, by hand
IMG = np.arange(1, 21, dtype=np.float32).reshape(5, 4, 1)      # rows 1..4, 5..8, 9..12, 13..16, 17..20


def _plane(rows):
    return np.asarray(rows, np.float32)[:, :, None]


def test_oracle_by_hand():
    # dy = +1 (down), dx = -1 (left), flipped: out[i, j] = img[i - 1, 3 - (j + 1)]
    want = _plane([[0, 0, 0, 0], [3, 2, 1, 0], [7, 6, 5, 0], [11, 10, 9, 0], [15, 14, 13, 0]])
    assert np.array_equal(R.transform(IMG, 1, -1, 1), want)
    # extreme shifts s = 3 (< min(5, 4)): one row / column survives
    want = _plane([[0, 0, 0, 0]] * 3 + [[0, 0, 0, 1], [0, 0, 0, 5]])
    assert np.array_equal(R.transform(IMG, 3, 3, 0), want)
    want = _plane([[16, 0, 0, 0], [20, 0, 0, 0]] + [[0, 0, 0, 0]] * 3)
    assert np.array_equal(R.transform(IMG, -3, -3, 0), want)
    # s = 0: flip only
    want = _plane([[4, 3, 2, 1], [8, 7, 6, 5], [12, 11, 10, 9], [16, 15, 14, 13], [20, 19, 18, 17]])
    assert np.array_equal(R.transform(IMG, 0, 0, 1), want)
    assert np.array_equal(R.transform(IMG, 0, 0, 0), IMG)
    # 5 x 4 stored in 8 x 8: the flip mirrors the REAL extent, zeros everywhere outside it
    out = R.transform(IMG, 1, -1, 1, stored_hw=(8, 8))
    want8 = np.zeros((8, 8, 1), np.float32)
    want8[:5, :4] = _plane([[0, 0, 0, 0], [3, 2, 1, 0], [7, 6, 5, 0], [11, 10, 9, 0], [15, 14, 13, 0]])
    assert np.array_equal(out, want8)
    # the batch form: sample ids, per-group keys, stored channels
    data = np.stack([IMG, IMG + 100])
    b = R.augment_batch(data, [[1, 0, 1]], [9], [2], 4, 1, True, (5, 4), (8, 8), 8)
    assert b.shape == (1, 3, 8, 8, 8) and not b[..., 1:].any() and not b[:, :, 5:].any() and not b[:, :, :, 4:].any()
    for col, sid in enumerate((1, 0, 1)):
        d = R.draw(R.key_of(9, 2), 4, col, 1, True)
        assert np.array_equal(b[0, col, :5, :4, :1], R.transform(data[sid], *d))


# ------------------------------------------------------------------ torch executor against the oracle
def _data(n=60, shape=(8, 8, 3)):
    from gentun_amd.utils.data import make_image_classification
    return make_image_classification(n=n, shape=shape, classes=4, seed=0, noise=0.3)


FOLDS = [(np.arange(20), np.arange(40, 60)), (np.arange(20, 40), np.arange(40, 60))]    # batches of 16 and 4


def _plan(genes=None, shape=(8, 8, 3)):
    from gentun_amd.models.genome import make_plan
    return make_plan(genes or {'S_1': '101'}, (3,), shape, (4,), ((3, 3),), 16, 4)


def _cfg(aug, **kw):
    from gentun_amd.models import cnn_engine as E
    base = dict(epochs=(1,), learning_rate=(1e-2,), batch_size=16, loss="ce", reset="all")
    base.update(kw)
    if aug != "absent":
        base["augment"] = aug
    return E.TrainConfig(**base)


def _record(job, steps=3):
    """Run ``steps`` train steps over an epoch boundary; the (sample ids, global step, batch) of each."""
    seen = []
    gather, forward = job._gather, job._forward

    def rec_gather(idx):
        seen.append([idx.clone().numpy(), job.global_step])
        return gather(idx)

    def rec_forward(xb, train, nval=None):
        seen[-1].append(xb.detach().clone())
        return forward(xb, train, nval)
    job._gather, job._forward = rec_gather, rec_forward
    job.init_params()
    job.reset_optimizer(1e-2)
    for s in range(steps):
        if s % job.steps_per_epoch == 0:
            job._new_epoch_order()
        job.train_step()
    job._gather, job._forward = gather, forward
    return seen


def _stored(xb, G):
    """[B, G*C, H, W] -> the oracle's [G][B][H][W][C]."""
    Bn, GC, H, W = xb.shape
    return xb.view(Bn, G, GC // G, H, W).permute(1, 0, 3, 4, 2).contiguous().numpy()


def test_torch_fold_job_batches_equal_the_oracle():
    from gentun_amd.models import cnn_engine as E
    x, y = _data()
    per_fold0 = []
    for nf in (1, 2):
        job = E.TorchFoldJob(_plan(), x, y, FOLDS[:nf], _cfg(AUG), "cpu", fold_ids=list(range(nf)))
        assert job.steps_per_epoch == 2
        seen = _record(job, 3)
        assert [s[1] for s in seen] == [1, 2, 3]                 # the global step runs on across the epoch boundary
        for ids, step, xb in seen:
            want = R.augment_batch(np.asarray(x, np.float32), ids, job.aug_seeds, job.fold_ids, step, 2, True, (8, 8))
            got = _stored(xb, nf)
            assert got.tobytes() == want.tobytes()
            assert got.tobytes() != np.asarray(x, np.float32)[ids].tobytes()          # something moved
        per_fold0.append([_stored(xb, nf)[0].tobytes() for _, _, xb in seen])
    assert per_fold0[0] == per_fold0[1]                          # a fold's batches: alone or beside another fold


def test_torch_pop_job_member_batches_alone_and_batched():
    from gentun_amd.models import cnn_engine as E
    x, y = _data()
    pa, pb = _plan({'S_1': '101'}), _plan({'S_1': '011'})
    alone = E.TorchPopJob(None, x, y, None, _cfg(AUG), "cpu", members=[(pa, [FOLDS[0]], [0])])
    both = E.TorchPopJob(None, x, y, None, _cfg(AUG), "cpu", members=[(pb, [FOLDS[1]], [1]), (pa, [FOLDS[0]], [0])])
    sa, sb = _record(alone, 3), _record(both, 3)
    for (ida, _, xa), (idb, _, xb) in zip(sa, sb):
        assert np.array_equal(ida[0], idb[1])
        assert _stored(xa, 1)[0].tobytes() == _stored(xb, 2)[1].tobytes()


def test_evaluate_and_predict_see_the_raw_images():
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.models.cnn_fitted import CnnClassifier
    x, y = _data()
    res = []
    for aug in (None, AUG):
        job = E.TorchFoldJob(_plan(), x, y, FOLDS, _cfg(aug), "cpu", fold_ids=[0, 1])
        job.init_params()
        res.append([t.numpy().tobytes() for t in job.evaluate()])
    assert res[0] == res[1]
    model = GeneticCnnModel(x, y, {'S_1': '101'}, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 0.5, 4, nfold=2, epochs=(1,),
                            learning_rate=(1e-2,), batch_size=16, loss="ce", backend="torch", device="cpu", augment=AUG)
    clf = model.fit()
    assert "augment" not in clf.header()
    logits = clf.predict(x, output="logits", device="cpu")
    # the same weights in a job that never heard of augmentation: its forward of the raw images
    plain = E.TorchFoldJob(_plan(), x, y, [FOLDS[0]], _cfg("absent"), "cpu", fold_ids=[0])
    clf.load_into(plain)
    with torch.no_grad():
        ref = plain._forward(plain._gather(torch.arange(len(x))[None, :]), False)[0].numpy()
    assert np.array_equal(np.asarray(logits, np.float32), ref)
    with tempfile.TemporaryDirectory() as d:
        clf.save(os.path.join(d, "m.npz"))
        back = CnnClassifier.load(os.path.join(d, "m.npz"))
    assert np.array_equal(back.predict(x, output="logits", device="cpu"), logits)


def _cv(aug, **kw):
    from gentun_amd.models.cnn import GeneticCnnModel
    x, y = _data()
    extra = {} if aug == "absent" else {"augment": aug}
    extra.update(kw)
    m = GeneticCnnModel(x, y, {'S_1': '101'}, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 0.5, 4, nfold=2, epochs=(2, 1),
                        learning_rate=(1e-2, 1e-3), batch_size=16, loss="ce", backend="torch", device="cpu", **extra)
    m.cross_validate()
    return m.fold_metrics


def test_determinism_and_effect():
    a, b = _cv(AUG), _cv(AUG)
    assert a == b
    off, absent = _cv(None), _cv("absent")
    assert off == absent
    assert a["val_loss"] != off["val_loss"]
    assert _cv({"shift": 0, "flip": True})["val_loss"] != off["val_loss"]


# ------------------------------------------------------------------ data parallelism
def _dp_job(dp_group=None):
    from gentun_amd.models import cnn_engine as E
    x, y = _data(shape=(8, 8, 1))
    fold = (np.arange(40), np.arange(40, 60))
    from gentun_amd.models.genome import make_plan
    plan = make_plan({'S_1': '101', 'S_2': '0000000000'}, (3, 5), (8, 8, 1), (4, 8), ((3, 3), (3, 3)), 16, 4)
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-2,), batch_size=16, dtype="fp32", loss="bce_compat",
                        dropout=0.5, dp_group=dp_group, augment=AUG)
    return E.TorchFoldJob(plan, x, y, [fold, (fold[0][::-1].copy(), fold[1])], cfg, "cpu", fold_ids=[0, 1])


def _dp_train(job):
    job.init_params()
    job.reset_optimizer(1e-2)
    job._new_epoch_order()
    for _ in range(job.steps_per_epoch):
        job.train_step()
    return job.flat.detach().clone()


def _dp_worker(rank, port, out):
    import torch.distributed as dist
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{}".format(port), rank=rank, world_size=2)
    try:
        torch.save(_dp_train(_dp_job(dp_group=dist.group.WORLD)), os.path.join(out, "rank{}.pt".format(rank)))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_data_parallel_with_augmentation_matches_single_process():
    single = _dp_train(_dp_job())
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(_free_port(), d), nprocs=2, join=True)
        r0 = torch.load(os.path.join(d, "rank0.pt"), weights_only=True)
        r1 = torch.load(os.path.join(d, "rank1.pt"), weights_only=True)
    assert torch.equal(r0, r1)
    # the bound of tests/test_data_parallel.py: the slices' gradient sums in another order, nothing else
    assert torch.allclose(r0, single, atol=2e-6, rtol=1e-5), (r0 - single).abs().max()


# ------------------------------------------------------------------ plumbing
def test_train_config_refusals():
    from gentun_amd.models import cnn_engine as E
    assert E.TrainConfig().augment is None and E.TrainConfig(augment=None).augment is None
    assert E.TrainConfig(augment={"shift": 3}).augment == {"shift": 3, "flip": False}
    assert E.TrainConfig(augment={"flip": True}).augment == {"shift": 0, "flip": True}
    for bad in ({"shift": 1, "rotate": 2}, {"shift": -1, "flip": True}, {"shift": 0, "flip": False}, {},
                {"shift": 1.5}, "flip", {"shift": 1, "flip": 1}):
        with pytest.raises(ValueError):
            E.TrainConfig(augment=bad)
    x, y = _data()
    with pytest.raises(ValueError, match="below"):               # too large for the 8 x 8 image
        E.TorchFoldJob(_plan(), x, y, FOLDS, _cfg({"shift": 8, "flip": False}), "cpu", fold_ids=[0, 1])
    E.TorchFoldJob(_plan(), x, y, FOLDS, _cfg({"shift": 7, "flip": False}), "cpu", fold_ids=[0, 1])
    from gentun_amd.models.cnn import GeneticCnnModel
    with pytest.raises(ValueError, match="below"):
        GeneticCnnModel(x, y, {'S_1': '101'}, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 0.5, 4, backend="torch",
                        device="cpu", augment={"shift": 8})


def _space(**kw):
    base = dict(nodes=(3,), input_shape=(8, 8, 3), kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
                dropout_probability=0.5, classes=4, nfold=2, epochs=(1,), learning_rate=(1e-2,), batch_size=16,
                loss="ce", seed=3, backend="torch", device="cpu")
    base.update(kw)
    return base


def test_individual_and_settings_key():
    from gentun_amd import GeneticCnnIndividual
    from gentun_amd.parallel.evaluators import _check_shared_settings
    x, y = _data()
    ind = GeneticCnnIndividual(x, y, genes={'S_1': '101'}, **_space(augment=AUG))
    assert ind.get_additional_parameters()["augment"] == AUG
    assert ind.build_fitness_model().cfg.augment == AUG
    assert ind.copy().augment == AUG
    plain = GeneticCnnIndividual(x, y, genes={'S_1': '011'}, **_space())
    assert plain.get_additional_parameters()["augment"] is None and plain.build_fitness_model().cfg.augment is None
    ma, mb, mc = (i.build_fitness_model() for i in (ind, ind.copy(), plain))
    _check_shared_settings([(ind, ma, 0), (ind, mb, 1)])
    with pytest.raises(ValueError, match="differ"):
        _check_shared_settings([(ind, ma, 0), (plain, mc, 1)])
    other = GeneticCnnIndividual(x, y, genes={'S_1': '101'}, **_space(augment={"shift": 1, "flip": True}))
    with pytest.raises(ValueError, match="differ"):
        _check_shared_settings([(ind, ma, 0), (other, other.build_fitness_model(), 1)])


def test_checkpoint_round_trip(tmp_path):
    from gentun_amd import GeneticAlgorithm, GeneticCnnIndividual, Population
    from gentun_amd.checkpoint import load
    from gentun_amd.utils import rng
    x, y = _data()
    rng.seed(4)
    pop = Population(GeneticCnnIndividual, x, y, size=2, additional_parameters=_space(augment=AUG))
    ga = GeneticAlgorithm(pop, seed=4, checkpoint_dir=str(tmp_path), verbose=False, tournament_size=2)
    ga.run(1)
    assert load(str(tmp_path))["additional_parameters"]["augment"] == AUG
    resumed = GeneticAlgorithm.resume(str(tmp_path), GeneticCnnIndividual, x, y, verbose=False)
    assert all(ind.augment == AUG and ind.build_fitness_model().cfg.augment == AUG for ind in resumed.population)


def _dist_hist(ga):
    """Every evaluated candidate's genes, fitness and per-fold scores."""
    return sorted((tuple(sorted(ind.get_genes().items())), ind.get_fitness(), tuple(ind.fold_scores))
                  for ind in ga.evaluated_population)


def _dist_proc(rank, world, port, q):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank),
                       "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank)})
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    torch.set_num_threads(1)
    from gentun_amd import GeneticAlgorithm, GeneticCnnIndividual
    from gentun_amd.parallel import DistComm
    from gentun_amd.parallel.distributed import DistributedPopulation, GentunWorker
    from gentun_amd.parallel.evaluators import SequentialEvaluator
    from gentun_amd.utils import rng
    import test_cnn_augment as T
    x, y = T._data()
    comm = DistComm(backend="gloo", timeout_s=120)
    if rank == 0:
        rng.seed(11)
        pop = DistributedPopulation(GeneticCnnIndividual, x, y, size=4, comm=comm, evaluator=SequentialEvaluator(),
                                    additional_parameters=T._space(augment=T.AUG))
        ga = GeneticAlgorithm(pop, verbose=False, tournament_size=2)
        ga.run(1)
        ga.population.shutdown()
        q.put(("hist", T._dist_hist(ga)))
    else:
        # the evaluator rank is built WITHOUT the setting: it must arrive in rank 0's config broadcast
        seen, build = [], GeneticCnnIndividual.build_fitness_model

        def recording(self, device=None):
            model = build(self, device)
            seen.append(model.cfg.augment)
            return model
        GeneticCnnIndividual.build_fitness_model = recording
        GentunWorker(GeneticCnnIndividual, x, y, comm=comm, evaluator=SequentialEvaluator()).work()
        q.put(("worker", seen))
    comm.destroy()


def test_gloo_distributed_population_matches_single_process():
    from gentun_amd import GeneticAlgorithm, GeneticCnnIndividual, Population
    from gentun_amd.utils import rng
    x, y = _data()

    def local(aug):
        rng.seed(11)
        ga = GeneticAlgorithm(Population(GeneticCnnIndividual, x, y, size=4,
                                         additional_parameters=_space(augment=aug)), verbose=False, tournament_size=2)
        ga.run(1)
        return _dist_hist(ga)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dist_proc, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got["hist"] == local(AUG)
    assert got["worker"] and all(a == AUG for a in got["worker"])     # the evaluator rank trained with the setting


def test_cli_flags_reach_the_config(monkeypatch):
    import gentun_amd.__main__ as M
    ns = argparse.Namespace
    assert M.augment_setting(ns(augment_shift=0, augment_flip=False)) is None
    assert M.augment_setting(ns(augment_shift=3, augment_flip=False)) == {"shift": 3, "flip": False}
    assert M.augment_setting(ns(augment_shift=0, augment_flip=True)) == {"shift": 0, "flip": True}
    got = {}

    def fake_search(args, species, x, y, extra, maximize=True, keep=None):
        got.update(extra)
        ind = species(x, y, **extra)
        got["cfg"] = ind.build_fitness_model(device="cpu").cfg
        return None
    monkeypatch.setattr(M, "_run_search", fake_search)
    base = ["cnn", "--samples", "40", "--input-shape", "8,8,1", "--classes", "4", "--nodes", "3", "--kernels", "4",
            "--kernel-sizes", "3", "--dense", "8"]
    M.main(base + ["--augment-shift", "2", "--augment-flip"])
    assert got["augment"] == {"shift": 2, "flip": True} and got["cfg"].augment == {"shift": 2, "flip": True}
    M.main(base)
    assert got["augment"] is None and got["cfg"].augment is None


def test_fit_ensemble_members_equal_fit_alone():
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn import GeneticCnnModel
    x, y = _data()
    genomes = [{"S_1": "101"}, {"S_1": "011"}]
    space = _space(augment=AUG)
    ens = fit_ensemble(x, y, genomes, **space)
    plain = fit_ensemble(x, y, genomes, **_space())
    for genes, member, other in zip(genomes, ens.members, plain.members):
        alone = GeneticCnnModel(x, y, genes, **space).fit()
        assert sorted(alone.params) == sorted(member.params)
        assert all(alone.params[k].tobytes() == member.params[k].tobytes() for k in alone.params)
        assert any(other.params[k].tobytes() != member.params[k].tobytes() for k in alone.params)
        assert member.header().keys() == other.header().keys()         # gentun-cnn/1 unchanged


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_augment.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"plain", "augmented"} and all(0.0 <= v <= 1.0 for v in out.values())


def test_prog_ops_contiguous_with_augment_last():
    from gentun_amd.ops import cnn_kernels as K
    vals = sorted(K.PROG_OPS.values())
    assert vals == list(range(len(vals)))
    assert K.PROG_OPS["gt_augment"] == vals[-1]
    # the native enum mirrors the table (csrc/hip/step_prog.hip)
    with open(os.path.join(ROOT, "csrc", "hip", "step_prog.hip")) as f:
        src = f.read()
    assert "OP_AUGMENT = {}".format(vals[-1]) in src and "OP_COUNT = {}".format(len(vals)) in src
