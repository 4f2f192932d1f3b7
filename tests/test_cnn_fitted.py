"""The fitted Genetic-CNN model on the CPU (torch executor): ``GeneticCnnModel.fit`` / ``predict`` and
``CnnClassifier`` export, file format and prediction (gentun_amd/models/cnn_fitted.py)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (input shape, classes, nodes, kernels, kernel sizes, genes, batch_norm)
CASES = {
    "plain": ((8, 8, 3), 3, (3,), (4,), ((3, 3),), {"S_1": "101"}, False),
    "bn2": ((16, 16, 1), 3, (3, 3), (4, 6), ((3, 3), (3, 3)), {"S_1": "110", "S_2": "011"}, True),
}
N, BATCH = 96, 32


def _data(shape, classes, n=N, seed=0):
    rng = np.random.default_rng(seed)
    lab = np.arange(n) % classes
    proto = rng.standard_normal((classes,) + shape).astype(np.float32)
    x = (proto[lab] + 0.5 * rng.standard_normal((n,) + shape)).astype(np.float32)
    return x, np.eye(classes, dtype=np.float32)[lab], lab


def _model(case, seed=3):
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes, nodes, kernels, ks, genes, bn = CASES[case]
    x, y, lab = _data(shape, classes)
    m = GeneticCnnModel(x, y, genes, nodes, shape, kernels, ks, 16, 0.5, classes, nfold=3, epochs=(1,),
                        learning_rate=(1e-2,), batch_size=BATCH, seed=seed, backend="torch", device="cpu",
                        batch_norm=bn)
    return m, x, lab


_FITS = {}


def _fit(case):
    """One fit per case, shared (and left unchanged) by the tests."""
    if case not in _FITS:
        m, x, lab = _model(case)
        _FITS[case] = (m, m.fit(), x, lab)
    return _FITS[case]


def _equal_arrays(a, b):
    return sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a)


def test_fit_returns_a_deterministic_classifier_distinct_from_cv_folds():
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x, lab = _fit("plain")
    assert isinstance(clf, CnnClassifier) and m.fitted is clf and len(m.jobs) == 1
    assert m.jobs[0].fold_ids == [m.nfold]
    assert list(clf.params) == [k for k, _ in clf.param_shapes()]
    assert clf.params["s1_in.w"].shape == (4, 3, 3, 3) and clf.params["dense1.w"].shape == (4 * 4 * 4, 16)
    again = _model("plain")[0].fit()
    assert _equal_arrays(clf.params, again.params) and again.metrics == clf.metrics
    cv = _model("plain")[0]
    cv.cross_validate()
    fold0 = CnnClassifier.from_job(cv.jobs[0].jobs[0])
    assert not _equal_arrays(clf.params, fold0.params)
    assert not np.array_equal(clf.params["s1_in.w"], fold0.params["s1_in.w"])


@pytest.mark.parametrize("case", ["plain", "bn2"])
def test_logits_equal_the_live_jobs_evaluation_forward(case):
    m, clf, x, lab = _fit(case)
    job = m.jobs[0]
    with torch.no_grad():
        ref = job._forward(job._gather(torch.arange(len(x))[None]), False)[0]
    got = torch.from_numpy(clf.predict(x, output="logits"))
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    if case == "bn2":          # the running statistics moved off (0, 1) and are what the forward reads
        assert np.abs(clf.params["s1_in.running_mean"]).max() > 0
        broken = dict(clf.params)
        broken["s1_in.running_mean"] = np.zeros_like(broken["s1_in.running_mean"])
        other = type(clf)(clf.genes, clf.nodes, clf.input_shape, clf.kernels_per_layer, clf.kernel_sizes,
                          clf.dense_units, clf.classes, broken, batch_norm=True, bn_eps=clf.bn_eps)
        assert not np.array_equal(other.predict(x, output="logits"), got.numpy())


def test_outputs_and_single_image():
    m, clf, x, lab = _fit("plain")
    logits, proba = clf.predict(x, output="logits"), clf.predict(x)
    assert proba.shape == (N, 3) and proba.dtype == np.float32
    # a sum of 3 fp32 terms, each a correctly rounded quotient by their fp32 sum: a few ulps of 1
    assert np.abs(proba.astype(np.float64).sum(1) - 1.0).max() <= 4 * 2.0 ** -23
    label = clf.predict(x, output="label")
    assert label.dtype == np.int64 and np.array_equal(label, np.argmax(logits, 1))
    assert np.array_equal(clf.predict_classes(x), label)
    one = clf.predict(x[5], output="logits")
    assert one.shape == (1, 3)
    assert np.array_equal(m.predict(x[:4], output="label"), label[:4])       # the model forwards to the classifier


@pytest.mark.parametrize("case", ["plain", "bn2"])
def test_chunking_does_not_change_a_row(case):
    m, clf, x, lab = _fit(case)
    big = torch.from_numpy(clf.predict(x, output="logits", batch=256))
    for n in (1, BATCH, BATCH + 1):
        got = torch.from_numpy(clf.predict(x[:n], output="logits", batch=BATCH))
        assert torch.equal(got, big[:n]), n
    assert torch.equal(torch.from_numpy(clf.predict(x, output="proba", batch=BATCH)),
                       torch.from_numpy(clf.predict(x, output="proba", batch=256)))


@pytest.mark.parametrize("case", ["plain", "bn2"])
def test_metrics_are_the_training_set_evaluation(case):
    m, clf, x, lab = _fit(case)
    hits = int((clf.predict_classes(x) == lab).sum())
    assert clf.metrics["rows"] == N
    assert round(clf.metrics["categorical_accuracy"] * N) == hits
    assert abs(clf.metrics["categorical_accuracy"] * N - hits) < 1e-3
    assert np.isfinite(clf.metrics["loss"]) and 0.0 <= clf.metrics["binary_accuracy"] <= 1.0


@pytest.mark.parametrize("case", ["plain", "bn2"])
def test_save_load_round_trip(case, tmp_path):
    from gentun_amd.models.cnn_fitted import FORMAT, CnnClassifier
    m, clf, x, lab = _fit(case)
    path = str(tmp_path / "model.npz")
    clf.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert json.loads(str(z["header"][()]))["format"] == FORMAT == "gentun-cnn/1"
        assert sorted(z.files) == sorted(["header"] + list(clf.params))
    back = CnnClassifier.load(path)
    assert back.header() == clf.header()
    assert _equal_arrays(back.params, clf.params)
    assert all(v.dtype == np.float32 for v in back.params.values())
    assert np.array_equal(back.predict(x), clf.predict(x))


def test_load_into_a_torch_job_is_the_inverse_of_from_job():
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x, lab = _fit("bn2")
    fresh = _model("bn2", seed=11)[0]
    job = fresh.make_jobs(fold_ids=[0])[0]
    job = getattr(job, "jobs", None) or job
    job.init_params()
    assert not _equal_arrays(CnnClassifier.from_job(job).params, clf.params)
    clf.load_into(job)
    assert _equal_arrays(CnnClassifier.from_job(job).params, clf.params)


def test_wrong_format_and_wrong_shapes_raise(tmp_path):
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x, lab = _fit("plain")
    path = str(tmp_path / "other.npz")
    header = dict(clf.header(), format="gentun-cnn/9")
    np.savez(path, header=np.array(json.dumps(header)), **clf.params)
    with pytest.raises(ValueError) as exc:
        CnnClassifier.load(path)
    assert "gentun-cnn/9" in str(exc.value) and "gentun-cnn/1" in str(exc.value)
    for bad in (np.zeros((2, 8, 9, 3), np.float32), np.zeros((2, 8, 8, 1), np.float32), np.zeros((8, 8), np.float32)):
        with pytest.raises(ValueError):
            clf.predict(bad)
    with pytest.raises(ValueError):
        clf.predict(x, output="classes")


def test_predict_before_fit_raises():
    m, x, lab = _model("plain")
    with pytest.raises(RuntimeError, match="before fit"):
        m.predict(x)


def test_reset_weights_acts_on_the_fitted_job():
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, x, lab = _model("plain")
    before = m.fit()
    assert m.reset_weights() == 1
    after = CnnClassifier.from_job(m.jobs[0])
    assert not np.array_equal(after.params["s1_in.w"], before.params["s1_in.w"])        # kernels re-drawn
    for name in ("s1_in.b", "dense1.b", "dense2.b"):
        assert np.array_equal(after.params[name], before.params[name])                    # biases kept
    assert _equal_arrays(m.fitted.params, before.params)                                  # the classifier is a copy


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_example_runs_on_the_cpu(tmp_path):
    r = _run([os.path.join(ROOT, "examples", "cnn_fit_predict.py"), "--device", "cpu", "--out",
              str(tmp_path / "model.npz")], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["reloaded_predictions_equal"] is True and os.path.exists(line["saved_model"])


def test_cnn_command_saves_the_refitted_winner(tmp_path):
    from gentun_amd.models.cnn_fitted import CnnClassifier
    path = str(tmp_path / "winner.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")     # a CPU run
    r = subprocess.run([sys.executable, "-m", "gentun_amd", "cnn", "--pop", "2", "--gens", "1", "--samples", "96",
                        "--input-shape", "8,8,3", "--nodes", "3", "--kernels", "4", "--kernel-sizes", "3", "--dense",
                        "16", "--classes", "3", "--nfold", "2", "--epochs", "1", "--lr", "1e-3", "--save-model", path],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"')]      # the two result lines
    search, saved = lines[-2], lines[-1]
    assert saved["saved_model"] == path and saved["genes"] == search["best_genes"]
    clf = CnnClassifier.load(path)
    assert clf.genes == saved["genes"] and clf.metrics == saved["metrics"] and clf.metrics["rows"] == 96
    assert clf.predict(np.zeros((2, 8, 8, 3), np.float32)).shape == (2, 3)


def test_save_model_of_the_cnn_command(tmp_path):
    """What ``python -m gentun_amd cnn --save-model`` runs after the search, on the CPU."""
    from gentun_amd.__main__ import save_cnn_model
    from gentun_amd.models.cnn_fitted import CnnClassifier
    shape, classes, nodes, kernels, ks, genes, bn = CASES["plain"]
    x, y, lab = _data(shape, classes)
    extra = dict(nodes=nodes, input_shape=shape, kernels_per_layer=kernels, kernel_sizes=ks, dense_units=16,
                 dropout_probability=0.5, classes=classes, nfold=3, epochs=(1,), learning_rate=(1e-2,),
                 batch_size=BATCH, seed=3)
    path = str(tmp_path / "best.npz")
    line = save_cnn_model(path, x, y, genes, extra, device="cpu")
    assert json.loads(json.dumps(line))["saved_model"] == path and line["genes"] == genes
    clf = CnnClassifier.load(path)
    assert clf.metrics == line["metrics"]
    assert _equal_arrays(clf.params, _fit("plain")[1].params)          # the same fit as GeneticCnnModel.fit()
