"""The fitted Genetic-CNN ensemble on the CPU (torch executor): ``fit_ensemble``, ``CnnEnsemble`` combination,
file format, refusals, ``top_genomes``, the example and ``--save-ensemble``
(gentun_amd/models/cnn_ensemble.py). The configuration is the smallest one of tests/test_cnn_fitted.py."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE, CLASSES, N, BATCH = (8, 8, 3), 3, 96, 32
GENOMES = [{"S_1": "101"}, {"S_1": "111"}, {"S_1": "011"}]
SPACE = dict(nodes=(3,), input_shape=SHAPE, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
             dropout_probability=0.5, classes=CLASSES, nfold=3, epochs=(1,), learning_rate=(1e-2,), batch_size=BATCH,
             seed=3, backend="torch")
K = len(GENOMES)


def _data(n=N, seed=0):
    rng = np.random.default_rng(seed)
    lab = np.arange(n) % CLASSES
    proto = rng.standard_normal((CLASSES,) + SHAPE).astype(np.float32)
    x = (proto[lab] + 0.5 * rng.standard_normal((n,) + SHAPE)).astype(np.float32)
    return x, np.eye(CLASSES, dtype=np.float32)[lab], lab


_FIT = {}


def _fit():
    """One ensemble fit, shared (and left unchanged) by the tests."""
    if not _FIT:
        from gentun_amd.models import fit_ensemble
        x, y, lab = _data()
        _FIT["v"] = (fit_ensemble(x, y, GENOMES, device="cpu", **SPACE), x, y, lab)
    return _FIT["v"]


def _equal_arrays(a, b):
    return sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a)


def _ordered_combine(mp, w):
    """The contract, written out: fp32 products and sums, member order."""
    w = np.asarray(w, np.float32)
    acc = np.multiply(w[0], mp[0], dtype=np.float32)
    for g in range(1, len(mp)):
        acc = np.add(acc, np.multiply(w[g], mp[g], dtype=np.float32), dtype=np.float32)
    votes = np.zeros(mp.shape[1:], np.int32)
    for g in range(len(mp)):
        votes[np.arange(mp.shape[1]), np.argmax(mp[g], 1)] += 1
    return acc, votes


def test_members_equal_their_fit_alone():
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn import GeneticCnnModel
    ens, x, y, lab = _fit()
    assert isinstance(ens, CnnEnsemble) and len(ens) == K and [m.genes for m in ens.members] == GENOMES
    for genes, member in zip(GENOMES, ens.members):
        alone = GeneticCnnModel(x, y, genes, device="cpu", **SPACE).fit()
        assert _equal_arrays(alone.params, member.params)
        assert alone.metrics == member.metrics and member.metrics["rows"] == N
    label = ens.predict(x, output="label")
    assert ens.metrics["rows"] == N and ens.metrics["genes"] == GENOMES
    assert ens.metrics["categorical_accuracy"] == float((label == lab).sum()) / N


@pytest.mark.parametrize("weights", [None, [3.0, 1.0, 4.0], [1, 0, 0]])
def test_combine_is_the_ordered_fp32_mean_and_the_argmax_count(weights):
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = _fit()
    ens = CnnEnsemble(fitted.members, weights=weights)
    w64 = np.ones(K) if weights is None else np.asarray(weights, np.float64)
    assert ens.weights.dtype == np.float32 and ens.weights.tobytes() == (w64 / w64.sum()).astype(np.float32).tobytes()
    out = ens.predict_outputs(x)
    mp = out["member_proba"]
    assert mp.shape == (K, N, CLASSES) and mp.dtype == np.float32 and out["member_logits"].shape == mp.shape
    for g, m in enumerate(ens.members):
        assert mp[g].tobytes() == m.predict(x).tobytes()
        assert out["member_logits"][g].tobytes() == m.predict(x, output="logits").tobytes()
    proba, votes = _ordered_combine(mp, ens.weights)
    assert out["proba"].dtype == np.float32 and out["proba"].tobytes() == proba.tobytes()
    assert out["votes"].dtype == np.int32 and out["votes"].tobytes() == votes.tobytes()
    assert (out["votes"].sum(1) == K).all()
    assert out["label"].dtype == np.int64 and np.array_equal(out["label"], np.argmax(proba, 1))
    assert out["vote_label"].dtype == np.int64
    # every output alone is what the joint pass gave
    for name in out:
        assert ens.predict(x, output=name).tobytes() == out[name].tobytes(), name
    # k terms w_g p_g with sum_g w_g = 1 and sum_c p_gc = 1, each within a few roundings: the k * C products and
    # sums of a row round once each, at most 2^-24 of a value that is at most 1
    assert np.abs(out["proba"].astype(np.float64).sum(1) - 1.0).max() <= K * CLASSES * 2.0 ** -23
    if weights == [1, 0, 0]:
        assert out["proba"].tobytes() == ens.members[0].predict(x).tobytes()


def test_one_member_equals_its_classifier():
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = _fit()
    clf = fitted.members[1]
    ens = CnnEnsemble([clf])
    assert ens.weights.tolist() == [1.0]
    assert ens.predict(x).tobytes() == clf.predict(x).tobytes()
    assert np.array_equal(ens.predict(x, output="label"), clf.predict(x, output="label"))
    assert np.array_equal(ens.predict(x, output="vote_label"), clf.predict(x, output="label"))
    assert ens.predict(x, output="member_logits")[0].tobytes() == clf.predict(x, output="logits").tobytes()
    one = ens.predict(x[5])
    assert one.shape == (1, CLASSES) and one.tobytes() == clf.predict(x[5]).tobytes()


def test_chunking_does_not_change_a_row():
    ens, x, y, lab = _fit()
    xs = x[:70]
    a, b = ens.predict_outputs(xs, batch=32), ens.predict_outputs(xs, batch=256)
    perm = np.random.default_rng(1).permutation(70)
    c = ens.predict_outputs(xs[perm], batch=32)
    for name in a:
        axis = 1 if name.startswith("member_") else 0
        assert a[name].tobytes() == b[name].tobytes(), name
        back = np.empty_like(c[name])
        if axis:
            back[:, perm] = c[name]
        else:
            back[perm] = c[name]
        assert back.tobytes() == a[name].tobytes(), name


def test_vote_label_tie_rules(monkeypatch):
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = _fit()
    ens = CnnEnsemble(fitted.members, weights=[0.25, 0.25, 0.5])       # every product and sum below is exact
    fixed = np.array([
        # row 0: one vote each; class 2 has the largest mean
        [[.5, .25, .25], [.5, .25, .25], [.5, .25, .25], [.4375, .3125, .25]],
        [[.25, .5, .25], [.5, .25, .25], [.25, .5, .25], [.4375, .3125, .25]],
        [[.25, .25, .5], [0., 1., 0.], [.3125, .3125, .375], [.4375, .3125, .25]],
    ], np.float32)
    # row 1: votes (2, 1, 0) although class 1 has the larger mean; row 2: one vote each, classes 0 and 1 tie in the
    # mean above class 2; row 3: all three vote for class 0
    for g, m in enumerate(ens.members):
        monkeypatch.setattr(m, "predict", lambda x, g=g, **kw: fixed[g][:len(x)].copy())
    out = ens.predict_outputs(x[:4], outputs=("proba", "votes", "label", "vote_label"))
    assert out["votes"].tolist() == [[1, 1, 1], [2, 1, 0], [1, 1, 1], [3, 0, 0]]
    assert out["proba"][0].tolist() == [.3125, .3125, .375]
    assert out["proba"][1].tolist() == [.25, .625, .125]
    assert out["proba"][2].tolist() == [.34375, .34375, .3125]
    assert out["vote_label"].tolist() == [2, 0, 0, 0]
    assert out["label"].tolist() == [2, 1, 0, 0]


def test_save_load_round_trip(tmp_path):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_ensemble import FORMAT
    from gentun_amd.models.cnn_fitted import CnnClassifier
    fitted, x, y, lab = _fit()
    ens = CnnEnsemble(fitted.members, weights=[3.0, 1.0, 4.0], metrics=fitted.metrics)
    path = str(tmp_path / "ensemble.npz")
    ens.save(path)
    with np.load(path, allow_pickle=False) as z:
        header = json.loads(str(z["header"][()]))
        assert header["format"] == FORMAT == "gentun-cnn-ensemble/1"
        assert header["members"] == [m.header() for m in ens.members]
        assert len(z.files) == 2 + sum(len(m.params) for m in ens.members)
        assert z["weights"].dtype == np.float32
    back = CnnEnsemble.load(path)
    assert back.weights.tobytes() == ens.weights.tobytes() and back.metrics == ens.metrics
    assert back.header() == ens.header()
    for a, b in zip(back.members, ens.members):
        assert isinstance(a, CnnClassifier) and _equal_arrays(a.params, b.params) and a.metrics == b.metrics
    for name in ("proba", "votes", "member_logits"):
        assert back.predict(x, output=name).tobytes() == ens.predict(x, output=name).tobytes()
    # the two formats refuse each other by name
    with pytest.raises(ValueError, match="gentun-cnn-ensemble/1"):
        CnnClassifier.load(path)
    single = str(tmp_path / "member.npz")
    back.members[0].save(single)                       # a member is an ordinary classifier
    assert _equal_arrays(CnnClassifier.load(single).params, ens.members[0].params)
    with pytest.raises(ValueError, match="gentun-cnn/1"):
        CnnEnsemble.load(single)


def _variant(clf, genes, **changes):
    """A zero-parameter classifier like ``clf`` with other genes and one changed field."""
    from gentun_amd.models.cnn_fitted import CnnClassifier
    from gentun_amd.models.genome import make_plan
    kw = dict(nodes=clf.nodes, input_shape=clf.input_shape, kernels_per_layer=clf.kernels_per_layer,
              kernel_sizes=clf.kernel_sizes, dense_units=clf.dense_units, classes=clf.classes,
              batch_norm=clf.batch_norm, bn_eps=clf.bn_eps, loss=clf.loss, dtype=clf.dtype)
    kw.update(changes)
    shim = CnnClassifier.__new__(CnnClassifier)
    shim.plan = make_plan(genes, kw["nodes"], kw["input_shape"], kw["kernels_per_layer"], kw["kernel_sizes"],
                          kw["dense_units"], kw["classes"])
    shim.batch_norm = kw["batch_norm"]
    params = {name: np.zeros(shape, np.float32) for name, shape in shim.param_shapes()}
    return CnnClassifier(genes, params=params, **kw)


@pytest.mark.parametrize("field,value,genes", [
    ("nodes", (4,), {"S_1": "100101"}), ("input_shape", (8, 8, 1), None), ("kernels_per_layer", (6,), None),
    ("kernel_sizes", ((5, 5),), None), ("dense_units", 8, None), ("classes", 4, None), ("batch_norm", True, None),
    ("bn_eps", 1e-2, None), ("dtype", "bf16", None), ("loss", "ce", None)])
def test_mixed_search_spaces_are_refused(field, value, genes):
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = _fit()
    first = fitted.members[0]
    other = _variant(first, genes or {"S_1": "111"}, **{field: value})
    assert len(CnnEnsemble([first, _variant(first, {"S_1": "111"})])) == 2        # the same space: accepted
    with pytest.raises(ValueError, match=field):
        CnnEnsemble([first, other])


def test_refusals():
    from gentun_amd.models import CnnEnsemble, fit_ensemble
    fitted, x, y, lab = _fit()
    members = fitted.members
    with pytest.raises(ValueError, match="1 to 64"):
        CnnEnsemble([])
    with pytest.raises(ValueError, match="1 to 64"):
        CnnEnsemble([members[0]] * 65)
    with pytest.raises(ValueError, match="same genes"):
        CnnEnsemble([members[0], members[1], _variant(members[0], members[0].genes)])
    for bad, what in (([1.0, 1.0], "weights for"), ([1.0, -1.0, 1.0], "non-negative"),
                      ([1.0, float("nan"), 1.0], "finite"), ([1.0, float("inf"), 1.0], "finite"),
                      ([0.0, 0.0, 0.0], "positive sum")):
        with pytest.raises(ValueError, match=what):
            CnnEnsemble(members, weights=bad)
    with pytest.raises(ValueError, match="output"):
        fitted.predict(x, output="classes")
    for bad in (np.zeros((2, 8, 9, 3), np.float32), np.zeros((2, 8, 8, 1), np.float32), np.zeros((8, 8), np.float32)):
        with pytest.raises(ValueError):
            fitted.predict(bad)
    with pytest.raises(ValueError, match="backend"):
        fitted.predict(x, backend="keras")
    # fit_ensemble refuses before it trains
    with pytest.raises(ValueError, match="distinct"):
        fit_ensemble(x, y, [GENOMES[0], dict(GENOMES[0])], device="cpu", **SPACE)
    with pytest.raises(ValueError, match="1 to 64"):
        fit_ensemble(x, y, [], device="cpu", **SPACE)
    with pytest.raises(ValueError, match="non-negative"):
        fit_ensemble(x, y, GENOMES, weights=[1, -1, 1], device="cpu", **SPACE)


class _Ind(object):
    def __init__(self, bits, fitness):
        self.genes, self.fitness = {"S_1": bits}, fitness

    def get_genes(self):
        return self.genes

    def get_fitness_status(self):
        return self.fitness is not None

    def get_fitness(self):
        raise AssertionError("top_genomes must not evaluate")


def test_top_genomes():
    from gentun_amd.models.cnn_ensemble import top_genomes

    class Pop(list):
        maximize = True

    pop = Pop([_Ind("001", 0.5), _Ind("010", 0.9), _Ind("010", 0.9), _Ind("011", None), _Ind("100", 0.9),
               _Ind("101", 0.7), _Ind("110", float("-inf"))])
    bits = lambda gs: [g["S_1"] for g in gs]  # noqa: E731
    assert bits(top_genomes(pop, 3)) == ["010", "100", "101"]          # duplicate skipped, ties in order
    assert bits(top_genomes(pop, 1)) == ["010"]
    assert bits(top_genomes(pop, 10)) == ["010", "100", "101", "001"]  # the unevaluated and the failed are left out
    pop.maximize = False
    assert bits(top_genomes(pop, 2)) == ["001", "101"]
    assert bits(top_genomes(list(pop), 2)) == ["010", "100"]           # a plain sequence: maximize
    assert bits(top_genomes(list(pop), 2, maximize=False)) == ["001", "101"]
    assert top_genomes(pop, 0) == [] and top_genomes(Pop(), 3) == []


def _run(args, cwd, **env):
    env = dict(os.environ, PYTHONPATH=ROOT, **env)
    return subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_example_runs_on_the_cpu(tmp_path):
    r = _run([os.path.join(ROOT, "examples", "cnn_ensemble.py"), "--device", "cpu", "--out",
              str(tmp_path / "ensemble.npz")], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["reloaded_predictions_equal"] is True and os.path.exists(line["saved_ensemble"])
    assert len(line["genes"]) == 3 and line["train_metrics"]["rows"] == 384


CLI = ["-m", "gentun_amd", "cnn", "--pop", "4", "--gens", "1", "--samples", "96", "--input-shape", "8,8,3", "--nodes",
       "3", "--kernels", "4", "--kernel-sizes", "3", "--dense", "16", "--classes", "3", "--nfold", "2", "--epochs", "1",
       "--lr", "1e-3"]


def _json_lines(stdout):
    return [json.loads(ln) for ln in stdout.splitlines() if ln.startswith('{"')]


def test_cnn_command_saves_the_ensemble(tmp_path):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_fitted import CnnClassifier
    path, single = str(tmp_path / "top.npz"), str(tmp_path / "winner.npz")
    cpu = dict(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = _run(CLI + ["--save-model", single, "--save-ensemble", path, "--ensemble-size", "2"], str(tmp_path), **cpu)
    assert r.returncode == 0, r.stderr[-2000:]
    search, saved, line = _json_lines(r.stdout)
    assert saved["saved_model"] == single and line["saved_ensemble"] == path
    assert len(line["genes"]) == 2 and line["genes"][0] != line["genes"][1]
    assert line["genes"][0] == search["best_genes"]            # one generation: its fittest leads the ensemble
    ens = CnnEnsemble.load(path)
    assert [m.genes for m in ens.members] == line["genes"] and ens.metrics == line["metrics"]
    assert [m.metrics for m in ens.members] == line["member_metrics"] and ens.metrics["rows"] == 96
    assert ens.predict(np.zeros((2, 8, 8, 3), np.float32)).shape == (2, 3)
    # the refitted winner is the ensemble's first member: the same fit
    assert _equal_arrays(CnnClassifier.load(single).params, ens.members[0].params)
    # without the flag: the parent's lines, nothing more
    plain = _run(CLI, str(tmp_path), **cpu)
    assert plain.returncode == 0, plain.stderr[-2000:]
    only, = _json_lines(plain.stdout)
    assert sorted(only) == ["best_fitness", "best_genes", "history"] and only["best_genes"] == search["best_genes"]
    assert "saved_ensemble" not in plain.stdout and "saved_model" not in plain.stdout
    text = lambda out: [ln for ln in out.splitlines() if not ln.startswith('{"')]  # noqa: E731
    assert text(plain.stdout) == text(r.stdout)
