"""Soft-target training on the CPU (torch executor): label smoothing and distillation.

``smoothing_targets`` and the refusals; the fp64 oracle of tests/soft_ref.py against central finite differences;
the torch executor's training loss against the oracle; the one-hot table and ``label_smoothing=0`` against the
hard-label path, byte for byte; evaluation on hard labels; ``soft_targets`` / ``distill``; and the plumbing of
``label_smoothing`` (modelled on the ``augment`` tests of tests/test_cnn_augment.py)."""

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

import soft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.1
GENES = {'S_1': '101'}


def _data(n=60, shape=(8, 8, 3)):
    from gentun_amd.utils.data import make_image_classification
    return make_image_classification(n=n, shape=shape, classes=4, seed=0, noise=0.3)


def _space(**kw):
    base = dict(nodes=(3,), input_shape=(8, 8, 3), kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
                dropout_probability=0.5, classes=4, nfold=2, epochs=(1,), learning_rate=(1e-2,), batch_size=16,
                loss="ce", seed=3, backend="torch", device="cpu")
    base.update(kw)
    return base


def _model(genes=None, **kw):
    from gentun_amd.models.cnn import GeneticCnnModel
    x, y = _data()
    return GeneticCnnModel(x, y, genes or GENES, **_space(**kw))


def _same(a, b):
    return sorted(a.params) == sorted(b.params) and all(a.params[k].tobytes() == b.params[k].tobytes()
                                                        for k in a.params)


def _onehot_table(y):
    t = np.zeros(np.asarray(y).shape, np.float32)
    t[np.arange(len(t)), np.argmax(y, 1)] = 1.0
    return t


_FITS = {}


def _plain_fit(loss="ce"):
    """``fit()`` on the hard labels: computed once, shared, left unchanged."""
    if loss not in _FITS:
        _FITS[loss] = _model(loss=loss).fit()
    return _FITS[loss]


# ------------------------------------------------------------------ the targets and the refusals
def test_smoothing_targets_by_hand():
    from gentun_amd.models.cnn_engine import smoothing_targets
    # (0.1, 10): fp32(0.1) / 10 = 0x3c23d70a; 1 - fp32(0.1) rounds to 0x3f666666, + t_off rounds to 0x3f68f5c2
    want = {(0.1, 10): (0x3f68f5c2, 0x3c23d70a), (0.5, 2): (0x3f400000, 0x3e800000),
            (0.25, 1): (0x3f800000, 0x3e800000)}
    for (eps, C), (on, off) in want.items():
        t_on, t_off = smoothing_targets(eps, C)
        assert isinstance(t_on, np.float32) and isinstance(t_off, np.float32)
        assert (int(t_on.view(np.uint32)), int(t_off.view(np.uint32))) == (on, off), (eps, C)
        assert abs(float(t_on) + (C - 1) * float(t_off) - 1.0) <= 1e-6
        assert (t_on, t_off) == R.smoothing_targets(eps, C)


def test_refusals_before_a_job_is_built(monkeypatch):
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.models.genome import make_plan
    x, y = _data()
    for bad in (True, False, -0.1, 1.0, 1.5, float("nan"), float("inf"), "0.1", [0.1]):
        with pytest.raises(ValueError):
            E.TrainConfig(label_smoothing=bad)
        with pytest.raises(ValueError):
            GeneticCnnModel(x, y, GENES, **_space(label_smoothing=bad))
    assert E.TrainConfig(label_smoothing=0).label_smoothing == 0.0 == E.TrainConfig().label_smoothing
    assert E.TrainConfig(label_smoothing=np.float32(0.25)).label_smoothing == 0.25

    built = []
    init = E.FoldJob.__init__

    def recording(self, *a, **kw):
        init(self, *a, **kw)
        built.append(self)                      # reached only when nothing raised before the job's own work
    monkeypatch.setattr(E.FoldJob, "__init__", recording)
    good = _onehot_table(y)
    nan, neg, off = good.copy(), good.copy(), good.copy()
    nan[3, 0] = np.nan
    neg[3] = (1.5, -0.5, 0.0, 0.0)
    off[3] = (0.5, 0.5, 2e-4, 0.0)
    tables = (good[:-1], good[:, :3], good.reshape(-1), nan, neg, off, good.astype(object), "table")
    plan = make_plan(GENES, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 4)
    rows = np.arange(len(x))
    for bad in tables:
        with pytest.raises(ValueError):
            _model().fit(soft_targets=bad)
        with pytest.raises(ValueError):
            E.make_job("torch", plan, x, y, [(rows, rows)], E.TrainConfig(), "cpu", soft_targets=bad)
    with pytest.raises(ValueError, match="both"):
        _model(label_smoothing=EPS).fit(soft_targets=good)
    assert built == []
    # a row sum 1e-4 off by less than the tolerance passes, as does an integer table
    near = good.copy()
    near[3] = (0.5, 0.5 - 5e-5, 0.0, 0.0)
    assert E.check_soft_targets(near, len(x), 4).dtype == np.float32
    assert E.check_soft_targets(good.astype(np.int64), len(x), 4).tobytes() == good.tobytes()
    assert E.check_soft_targets(np.asfortranarray(good.astype(np.float64)), len(x), 4).flags.c_contiguous


def test_hip_executor_refuses_dp_group_before_any_work():
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn_hip import HipPopJob
    from gentun_amd.models.genome import make_plan
    x, y = _data()
    plan = make_plan(GENES, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 4)
    rows = np.arange(len(x))
    for kw, cfg in (({"soft_targets": _onehot_table(y)}, E.TrainConfig(dp_group=object())),
                    ({}, E.TrainConfig(dp_group=object(), label_smoothing=EPS))):
        with pytest.raises(ValueError, match="dp_group are not supported by the HIP executor"):
            HipPopJob(plan, x, y, [(rows, rows)], cfg, "cpu", fold_ids=[0], **kw)


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("mode", ["ce", "bce_compat"])
def test_oracle_dz_against_central_differences(mode):
    """``<dz, d>`` against ``(L(z + e d) - L(z - e d)) / 2e`` along random unit directions, e = 1e-6, for a
    random table and for smoothed labels, with a short batch (the bound of tests/test_cnn_gradcam.py)."""
    rng = np.random.default_rng(5)
    B, C, N = 7, 5, 30
    labels = rng.integers(0, C, N)
    sids = rng.integers(0, N, B)
    table = R.random_table(rng, N, C, labels, peak=0.3)
    worst = 0.0
    for kw in ({"table": table}, {"eps": 0.1}, {"eps": 0.9}, {}):
        t = R.target_rows(labels, sids, C, **kw)
        z = 2.0 * rng.standard_normal((B, C))
        dz = R.batch_dz(z, t, mode, nvalid=5)
        assert not dz[5:].any() and np.abs(dz[:5]).max() > 0
        for _ in range(4):
            d = rng.standard_normal((B, C))
            d /= np.sqrt((d ** 2).sum())
            e = 1e-6
            fd = (R.batch_loss(z + e * d, t, mode, nvalid=5) - R.batch_loss(z - e * d, t, mode, nvalid=5)) / (2 * e)
            an = float((dz * d).sum())
            worst = max(worst, abs(fd - an) / np.abs(dz).max())
    print("[cnn-soft] oracle dz vs central differences ({}): {:.3e}".format(mode, worst))
    assert worst <= 1e-6


# ------------------------------------------------------------------ torch executor against the oracle
@pytest.mark.parametrize("mode", ["ce", "bce_compat"])
@pytest.mark.parametrize("kind", ["table", "eps"])
def test_torch_training_loss_equals_the_oracle(monkeypatch, kind, mode):
    """One training batch (16 rows, the second group's batch short): the per-row losses the torch executor
    differentiates against the oracle's at the executor's own logits. fp32 softmax and log of probabilities
    above ~1e-3 carry a few ulp each and C = 4 terms are summed: 5e-6 covers it with a wide margin."""
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.genome import make_plan
    x, y = _data()
    labels = np.argmax(y, 1)
    table = R.random_table(np.random.default_rng(2), len(x), 4, labels, peak=0.5)
    folds = [(np.arange(40), np.arange(40, 60)), (np.arange(12), np.arange(40, 60))]
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-2,), batch_size=16, loss=mode, reset="all",
                        label_smoothing=EPS if kind == "eps" else 0.0)
    plan = make_plan(GENES, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 4)
    job = E.TorchFoldJob(plan, x, y, folds, cfg, "cpu", fold_ids=[0, 1],
                         soft_targets=table if kind == "table" else None)
    seen = {}
    real = E.loss_and_metrics

    def recording(logits, targets, m):
        out = real(logits, targets, m)
        seen.update(logits=logits.detach().double().numpy(), targets=targets.detach().numpy(),
                    per=out[0].detach().numpy())
        return out
    monkeypatch.setattr(E, "loss_and_metrics", recording)
    job.init_params()
    job.reset_optimizer(1e-2)
    job._new_epoch_order()
    ids = job.epoch_idx[0].numpy().copy()
    job.train_step()
    worst = 0.0
    for g in range(2):
        want_t = R.target_rows(labels, ids[g], 4, table=table if kind == "table" else None,
                               eps=EPS if kind == "eps" else 0.0)
        assert np.array_equal(seen["targets"][g].astype(np.float64), want_t)
        for b in range(16):
            want = R.row_loss(seen["logits"][g, b], want_t[b], mode)
            worst = max(worst, abs(float(seen["per"][g, b]) - want))
    print("[cnn-soft] torch loss vs oracle ({}, {}): {:.3e}".format(kind, mode, worst))
    assert worst <= 5e-6


# ------------------------------------------------------------------ off is off; the effect
@pytest.mark.parametrize("loss", ["ce", "bce_compat"])
def test_one_hot_table_equals_plain_fit(loss):
    _, y = _data()
    assert _same(_model(loss=loss).fit(soft_targets=_onehot_table(y)), _plain_fit(loss))


def test_label_smoothing_zero_is_off_and_eps_has_an_effect():
    from gentun_amd.parallel.evaluators import _settings_key
    x, y = _data()
    from gentun_amd.models.cnn import GeneticCnnModel
    never = GeneticCnnModel(x, y, GENES, **_space())
    zero = GeneticCnnModel(x, y, GENES, **_space(label_smoothing=0))
    some = GeneticCnnModel(x, y, GENES, **_space(label_smoothing=EPS))
    assert _settings_key(never) == _settings_key(zero) != _settings_key(some)
    assert _same(zero.fit(), _plain_fit())
    a, b = some.fit(), _model(label_smoothing=EPS).fit()
    assert _same(a, b) and not _same(a, _plain_fit())
    assert a.header().keys() == _plain_fit().header().keys()          # nothing of it in the model file


def test_metrics_are_computed_on_hard_labels():
    x, y = _data()
    labels = np.argmax(y, 1)
    wrong = np.zeros(np.asarray(y).shape, np.float32)
    wrong[np.arange(len(wrong)), (labels + 1) % 4] = 1.0               # a table that contradicts every label
    clf = _model(epochs=(40,), dropout_probability=0.0, dense_units=32).fit(soft_targets=wrong)
    got = clf.predict(x, output="label", device="cpu")
    assert clf.metrics["rows"] == len(x)
    assert round(clf.metrics["categorical_accuracy"] * len(x)) == int((got == labels).sum())
    assert (got == (labels + 1) % 4).sum() > (got == labels).sum()    # it did learn the table


# ------------------------------------------------------------------ soft_targets / distill
def _teachers():
    if "teachers" not in _FITS:
        from gentun_amd.models import fit_ensemble
        x, y = _data()
        _FITS["teachers"] = fit_ensemble(x, y, [GENES, {'S_1': '011'}], weights=[3.0, 1.0], **_space(epochs=(3,)))
    return _FITS["teachers"]


def test_soft_targets_of_a_classifier_and_an_ensemble():
    from gentun_amd.models import CnnEnsemble, soft_targets
    x, y = _data()
    ens = _teachers()
    clf = ens.members[0]
    assert soft_targets(clf, x, y, alpha=0.0).tobytes() == _onehot_table(y).tobytes()
    assert soft_targets(ens, x, y, alpha=0.0, temperature=3.0).tobytes() == _onehot_table(y).tobytes()
    t = soft_targets(clf, x, y, alpha=1.0, temperature=1.0)
    assert t.dtype == np.float32 and t.shape == (len(x), 4) and t.flags.c_contiguous
    assert np.abs(t - clf.predict(x, output="proba", device="cpu")).max() <= 1e-6
    one = CnnEnsemble([clf])
    for kw in (dict(alpha=1.0), dict(alpha=0.4, temperature=2.5)):
        assert soft_targets(one, x, y, **kw).tobytes() == soft_targets(clf, x, y, **kw).tobytes()
    # the weighted ensemble: the ordered formula in plain numpy
    logits = np.asarray(ens.predict(x, output="member_logits", device="cpu"), np.float32).astype(np.float64)
    q = np.zeros((len(x), 4))
    for m in range(2):
        z = logits[m] / 2.0
        e = np.exp(z - z.max(1, keepdims=True))
        q = q + np.float64(ens.weights[m]) * (e / e.sum(1, keepdims=True))
    want = (0.25 * _onehot_table(y).astype(np.float64) + 0.75 * q).astype(np.float32)
    got = soft_targets(ens, x, y, alpha=0.75, temperature=2.0)
    assert got.tobytes() == want.tobytes()
    assert abs(float(ens.weights[0]) - 0.75) < 1e-6
    for tab in (t, got):
        assert np.abs(tab.astype(np.float64).sum(1) - 1.0).max() <= 1e-6 and tab.min() >= 0
    for bad in (dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=True), dict(temperature=0.0), dict(temperature=-1.0),
                dict(temperature=float("inf")), dict(temperature=float("nan")), dict(alpha="a")):
        with pytest.raises(ValueError):
            soft_targets(clf, x, y, **bad)
    with pytest.raises(ValueError):
        soft_targets(clf, x, np.asarray(y)[:, :3])
    with pytest.raises(ValueError):
        soft_targets(clf, np.asarray(x)[:, :7], y)
    with pytest.raises(ValueError):
        soft_targets(clf, np.asarray(x)[:-1], y)
    with pytest.raises(ValueError):
        soft_targets(object(), x, y)


def test_distill_equals_the_manual_fit():
    from gentun_amd.models import distill, soft_targets
    x, y = _data()
    ens = _teachers()
    table = soft_targets(ens, x, y, alpha=0.6, temperature=2.0, device="cpu")
    manual = _model().fit(soft_targets=table)
    student = distill(ens, x, y, GENES, alpha=0.6, temperature=2.0, **_space())
    assert _same(student, manual) and not _same(student, _plain_fit())
    assert student.metrics == manual.metrics and student.metrics["rows"] == len(x)
    short = ens.distill(x, y, alpha=0.6, temperature=2.0, **_space())       # genes=None: the first member's
    assert short.genes == ens.members[0].genes == GENES and _same(short, manual)
    other = ens.distill(x, y, genes={'S_1': '110'}, alpha=0.6, temperature=2.0, **_space())
    assert other.genes == {'S_1': '110'}


# ------------------------------------------------------------------ data parallelism (torch executor)
def _dp_job(dp_group=None, table=False):
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.genome import make_plan
    x, y = _data(shape=(8, 8, 1))
    fold = (np.arange(40), np.arange(40, 60))
    plan = make_plan({'S_1': '101', 'S_2': '0000000000'}, (3, 5), (8, 8, 1), (4, 8), ((3, 3), (3, 3)), 16, 4)
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-2,), batch_size=16, dtype="fp32", loss="bce_compat",
                        dropout=0.5, dp_group=dp_group, label_smoothing=0.0 if table else EPS)
    soft = R.random_table(np.random.default_rng(4), len(x), 4, np.argmax(y, 1), peak=0.5) if table else None
    return E.TorchFoldJob(plan, x, y, [fold, (fold[0][::-1].copy(), fold[1])], cfg, "cpu", fold_ids=[0, 1],
                          soft_targets=soft)


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
        for table in (False, True):
            torch.save(_dp_train(_dp_job(dp_group=dist.group.WORLD, table=table)),
                       os.path.join(out, "rank{}_{}.pt".format(rank, int(table))))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_data_parallel_with_soft_targets_matches_single_process():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(_free_port(), d), nprocs=2, join=True)
        for table in (False, True):
            single = _dp_train(_dp_job(table=table))
            r0 = torch.load(os.path.join(d, "rank0_{}.pt".format(int(table))), weights_only=True)
            r1 = torch.load(os.path.join(d, "rank1_{}.pt".format(int(table))), weights_only=True)
            assert torch.equal(r0, r1)
            # the bound of tests/test_data_parallel.py: the slices' gradient sums in another order, nothing else
            assert torch.allclose(r0, single, atol=2e-6, rtol=1e-5), (r0 - single).abs().max()


# ------------------------------------------------------------------ plumbing
def test_individual_and_settings_key():
    from gentun_amd import GeneticCnnIndividual
    from gentun_amd.parallel.evaluators import _check_shared_settings
    x, y = _data()
    ind = GeneticCnnIndividual(x, y, genes={'S_1': '101'}, **_space(label_smoothing=EPS))
    assert ind.get_additional_parameters()["label_smoothing"] == EPS
    assert ind.build_fitness_model().cfg.label_smoothing == EPS
    assert ind.copy().label_smoothing == EPS
    plain = GeneticCnnIndividual(x, y, genes={'S_1': '011'}, **_space())
    assert plain.get_additional_parameters()["label_smoothing"] == 0.0
    assert plain.build_fitness_model().cfg.label_smoothing == 0.0
    ma, mb, mc = (i.build_fitness_model() for i in (ind, ind.copy(), plain))
    _check_shared_settings([(ind, ma, 0), (ind, mb, 1)])
    with pytest.raises(ValueError, match="differ"):
        _check_shared_settings([(ind, ma, 0), (plain, mc, 1)])
    other = GeneticCnnIndividual(x, y, genes={'S_1': '101'}, **_space(label_smoothing=0.2))
    with pytest.raises(ValueError, match="differ"):
        _check_shared_settings([(ind, ma, 0), (other, other.build_fitness_model(), 1)])


def test_checkpoint_round_trip(tmp_path):
    from gentun_amd import GeneticAlgorithm, GeneticCnnIndividual, Population
    from gentun_amd.checkpoint import load
    from gentun_amd.utils import rng
    x, y = _data()
    rng.seed(4)
    pop = Population(GeneticCnnIndividual, x, y, size=2, additional_parameters=_space(label_smoothing=EPS))
    ga = GeneticAlgorithm(pop, seed=4, checkpoint_dir=str(tmp_path), verbose=False, tournament_size=2)
    ga.run(1)
    saved = load(str(tmp_path))["additional_parameters"]
    assert saved["label_smoothing"] == EPS and "soft_targets" not in saved
    resumed = GeneticAlgorithm.resume(str(tmp_path), GeneticCnnIndividual, x, y, verbose=False)
    assert all(ind.label_smoothing == EPS and ind.build_fitness_model().cfg.label_smoothing == EPS
               for ind in resumed.population)


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
    import test_cnn_soft as T
    x, y = T._data()
    comm = DistComm(backend="gloo", timeout_s=120)
    if rank == 0:
        rng.seed(11)
        pop = DistributedPopulation(GeneticCnnIndividual, x, y, size=4, comm=comm, evaluator=SequentialEvaluator(),
                                    additional_parameters=T._space(label_smoothing=T.EPS))
        ga = GeneticAlgorithm(pop, verbose=False, tournament_size=2)
        ga.run(1)
        ga.population.shutdown()
        q.put(("hist", T._dist_hist(ga)))
    else:
        # the evaluator rank is built WITHOUT the setting: it must arrive in rank 0's config broadcast
        seen, build = [], GeneticCnnIndividual.build_fitness_model

        def recording(self, device=None):
            model = build(self, device)
            seen.append(model.cfg.label_smoothing)
            return model
        GeneticCnnIndividual.build_fitness_model = recording
        GentunWorker(GeneticCnnIndividual, x, y, comm=comm, evaluator=SequentialEvaluator()).work()
        q.put(("worker", seen))
    comm.destroy()


def test_gloo_distributed_population_matches_single_process():
    from gentun_amd import GeneticAlgorithm, GeneticCnnIndividual, Population
    from gentun_amd.utils import rng
    x, y = _data()

    def local(eps):
        rng.seed(11)
        ga = GeneticAlgorithm(Population(GeneticCnnIndividual, x, y, size=4,
                                         additional_parameters=_space(label_smoothing=eps)), verbose=False,
                              tournament_size=2)
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
    assert got["hist"] == local(EPS)
    assert got["worker"] and all(e == EPS for e in got["worker"])     # the evaluator rank trained with the setting


def test_cli_flags(monkeypatch, tmp_path):
    import gentun_amd.__main__ as M
    from gentun_amd.models import CnnEnsemble, soft_targets
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.models.cnn_fitted import CnnClassifier
    ns = argparse.Namespace
    assert M.label_smoothing_setting(ns()) == 0.0 and M.label_smoothing_setting(ns(label_smoothing=0.2)) == 0.2
    with pytest.raises(SystemExit):
        M.label_smoothing_setting(ns(label_smoothing=1.0))
    got = {}

    def fake_search(args, species, x, y, extra, maximize=True, keep=None):
        got.update(extra=dict(extra), x=x, y=y)
        inds = [species(x, y, genes={"S_1": g}, **extra) for g in ("101", "011", "110")]
        for f, ind in zip((0.5, 0.9, 0.7), inds):
            ind.set_fitness(f)
        got["cfg"] = inds[0].build_fitness_model(device="cpu").cfg
        keep["population"] = inds
        return {"best_genes": inds[1].get_genes()}
    monkeypatch.setattr(M, "_run_search", fake_search)
    monkeypatch.setattr(M, "_device", lambda: torch.device("cpu"))
    base = ["cnn", "--samples", "40", "--input-shape", "8,8,1", "--classes", "4", "--nodes", "3", "--kernels", "4",
            "--kernel-sizes", "3", "--dense", "8", "--epochs", "1", "--lr", "1e-2", "--nfold", "2", "--loss", "ce"]
    M.main(base + ["--label-smoothing", "0.2"])
    assert got["extra"]["label_smoothing"] == 0.2 and got["cfg"].label_smoothing == 0.2
    M.main(base)
    assert got["extra"]["label_smoothing"] == 0.0 and got["cfg"].label_smoothing == 0.0
    with pytest.raises(SystemExit):
        M.main(base + ["--distill", str(tmp_path / "s.npz")])                 # no teacher
    ens_path, stu_path = str(tmp_path / "top2.npz"), str(tmp_path / "student.npz")
    M.main(base + ["--save-ensemble", ens_path, "--ensemble-size", "2", "--distill", stu_path,
                   "--distill-alpha", "0.3", "--distill-temperature", "2"])
    ens, student = CnnEnsemble.load(ens_path), CnnClassifier.load(stu_path)
    assert [m.genes for m in ens.members] == [{"S_1": "011"}, {"S_1": "110"}] and student.genes == {"S_1": "011"}
    table = soft_targets(ens, got["x"], got["y"], alpha=0.3, temperature=2.0, device="cpu")
    manual = GeneticCnnModel(got["x"], got["y"], {"S_1": "011"}, device="cpu", **got["extra"]).fit(soft_targets=table)
    assert _same(student, manual)


def test_fit_ensemble_members_equal_fit_alone():
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn import GeneticCnnModel
    x, y = _data()
    genomes = [{"S_1": "101"}, {"S_1": "011"}]
    space = _space(label_smoothing=EPS)
    ens = fit_ensemble(x, y, genomes, **space)
    plain = fit_ensemble(x, y, genomes, **_space())
    for genes, member, other in zip(genomes, ens.members, plain.members):
        alone = GeneticCnnModel(x, y, genes, **space).fit()
        assert _same(alone, member) and not _same(other, member)
        assert member.header().keys() == other.header().keys()         # gentun-cnn/1 unchanged


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_distill.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"teacher", "plain", "smoothed", "distilled"} and all(0.0 <= v <= 1.0 for v in out.values())


def test_prog_ops_mirror_the_native_enum():
    """Every launch entry point of ``PROG_OPS`` has the number the enum of csrc/hip/step_prog.hip gives it, the
    numbers are contiguous and ``OP_COUNT`` is their count; ``gt_head_soft`` is among them."""
    import re
    from gentun_amd.ops import cnn_kernels as K
    with open(os.path.join(ROOT, "csrc", "hip", "step_prog.hip")) as f:
        src = f.read()
    enum = {name: int(v) for name, v in re.findall(r"\b(OP_[A-Z_0-9]+) = (\d+)", src)}
    count = enum.pop("OP_COUNT")
    assert sorted(enum.values()) == list(range(count)) == sorted(K.PROG_OPS.values())
    assert K.PROG_OPS["gt_head_soft"] == enum["OP_HEAD_SOFT"] and K.PROG_OPS["gt_head"] == enum["OP_HEAD"]
    assert K.PROG_OPS["gt_augment"] == enum["OP_AUGMENT"]
    assert "case OP_HEAD_SOFT: return gt_head_soft(" in src
