"""Monte-Carlo dropout of fitted Genetic-CNN models on the CPU (torch executor): ``utils.rng.mc_masks`` and the
``predict_mc`` method of ``CnnClassifier`` / ``CnnEnsemble`` / ``GeneticCnnModel`` against the fp64 oracle of
tests/mc_ref.py. The fits are those of tests/test_cnn_tta.py (shared inside one pytest process, left unchanged)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mc_ref as R
import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS = 6
TINY = 4 * 2.0 ** -23
NAMES = ("proba", "std", "entropy", "mutual_info")


def _hidden64(clf, x):
    """The fp64 forward's hidden rows ``h [n, units]``, rows padded to a multiple of 32 as ``predict`` pads them."""
    buf = np.zeros(((len(x) + 31) // 32 * 32,) + (clf.input_shape[2],) + clf.input_shape[:2], np.float32)
    buf[:len(x)] = x.transpose(0, 3, 1, 2)
    P = clf._tensors(torch.device("cpu"), torch.float64)
    with torch.no_grad():
        return clf._torch_hidden(clf._torch_features(torch.from_numpy(buf).double(), P), P)[:len(x)].numpy()


def _oracle(members, weights, x, samples, dropout, seed):
    return R.oracle(np.stack([_hidden64(m, x) for m in members]), np.stack([m.params["dense2.w"] for m in members]),
                    np.stack([m.params["dense2.b"] for m in members]), weights, samples, dropout, seed,
                    np.arange(len(x)))


def test_masks_against_a_pinned_vector():
    from gentun_amd.utils.rng import MC_KEY, hash4, mc_masks
    assert int(hash4(7, 2, MC_KEY, 0)) == 368376980
    m = mc_masks(7, 2, 3, [0, 1000], 16, 0.3)
    assert m.dtype == np.bool_ and m.shape == (3, 2, 16)
    assert [int("".join("1" if b else "0" for b in r), 2) for r in m.reshape(6, 16)] == \
        [60203, 63646, 34799, 19229, 45055, 49099]


@pytest.mark.parametrize("dropout", [0.0, 0.3, 0.5, 0.999])
def test_masks_against_a_loop_and_the_binomial_share(dropout):
    from gentun_amd.utils.rng import MC_KEY, hash4, mc_masks
    seed, member, rows = 2 ** 32 - 1, 5, [3, 70000]
    thr = int(dropout * 4294967296.0)
    key = int(hash4(seed, member, MC_KEY, 0))
    got = mc_masks(seed, member, 4, rows, 9, dropout)
    for t in range(4):
        for i, n in enumerate(rows):
            for u in range(9):
                assert bool(got[t, i, u]) == (int(hash4(key, t, n, u)) >= thr)
    big = mc_masks(11, 0, 64, np.arange(50), 500, dropout)              # 1.6 M draws: five standard deviations
    q, N = 1.0 - thr / 4294967296.0, big.size
    assert abs(big.mean() - q) <= 5 * np.sqrt(q * (1 - q) / N) + 1e-12


@pytest.mark.parametrize("k,weights", [(0, None), (1, None), (3, [3.0, 1.0, 4.0])], ids=["clf", "ens1", "ens3"])
@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_torch_backend_against_the_oracle(case, k, weights):
    """``max |diff| <= 1e-5 * max |oracle|`` per output, the bound of the Grad-CAM CPU test for the same comparison.

    Measured: ``proba`` 6.7e-8, ``std`` 4.3e-7, ``entropy`` 6.2e-8, ``mutual_info`` 1.6e-7 to 5.3e-7 (as the fp32
    difference of the two fp32 entropies it was 2.3e-5 on the one-member ``mnist`` cases, whose largest mutual
    information is 5.5e-3: ``mc_mutual_info`` takes both entropies in fp64)."""
    from gentun_amd.models import CnnEnsemble
    fitted, x = T._ensemble(case)
    obj = fitted.members[0] if k == 0 else CnnEnsemble(fitted.members[:k], weights=weights)
    members, w = ([obj], np.ones(1, np.float32)) if k == 0 else (obj.members, obj.weights)
    xs = x[:NROWS]
    got = obj.predict_mc(xs, samples=17, dropout=0.4, seed=9, return_samples=True)
    want = _oracle(members, w, xs, 17, 0.4, 9)
    assert set(got) == set(NAMES) | {"label", "samples"} and got["label"].dtype == np.int64
    assert got["samples"].shape == (NROWS, len(members), 17, obj.classes)
    for name in NAMES + ("samples",):
        assert got[name].dtype == np.float32 and got[name].shape == want[name].shape
        err = float(np.abs(got[name] - want[name]).max() / np.abs(want[name]).max())
        print("[cnn-mc] torch backend vs oracle ({}, {}, {}): {:.3e}".format(case, k, name, err))
        assert err <= 1e-5
    assert want["std"].max() > 1e-3 and np.array_equal(got["label"], want["label"])
    assert got["proba"].tobytes() == obj.predict_mc(xs, samples=17, dropout=0.4, seed=9)["proba"].tobytes()
    p64 = members[0]._torch_mc(xs, 0, 17, 0.4, 9, torch.device("cpu"), 256, torch.float64)
    assert p64.dtype == np.float64 and np.abs(p64 - want["samples"][:, 0]).max() <= 1e-12


@pytest.mark.parametrize("what", ["clf", "ens"])
def test_no_dropout_is_the_plain_forward(what):
    obj = T._fit("rgb")[1] if what == "clf" else T._ensemble("rgb")[0]
    x = T._fit("rgb")[2]
    got = obj.predict_mc(x[:40], samples=5, dropout=0)
    assert np.abs(got["proba"] - obj.predict(x[:40])).max() <= TINY
    assert got["std"].max() <= TINY if what == "clf" else got["std"].max() > TINY      # members still disagree
    assert (got["mutual_info"].max() <= TINY) == (what == "clf") and (got["mutual_info"] >= 0).all()


@pytest.mark.parametrize("what", ["clf", "ens"])
def test_chunking_and_seeds(what):
    """96 rows: one chunk at batch 256, three at batch 32 (see tests/test_cnn_gradcam.py on the row count)."""
    obj = T._fit("mnist_bn")[1] if what == "clf" else T._ensemble("mnist_bn")[0]
    x = T._fit("mnist_bn")[2]
    a = obj.predict_mc(x, samples=8, seed=3, batch=256, return_samples=True)
    b = obj.predict_mc(x, samples=8, seed=3, batch=32, return_samples=True)
    c = obj.predict_mc(x, samples=8, seed=4, batch=256, return_samples=True)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["samples"].tobytes() != c["samples"].tobytes() and a["std"].tobytes() != c["std"].tobytes()
    one = obj.predict_mc(x[5], samples=8, seed=3)                       # one [H, W, C] image is image 0
    assert one["proba"].shape == (1, obj.classes)


BAD = [dict(samples=0), dict(samples=65), dict(samples=2.0), dict(samples=True), dict(samples=None),
       dict(dropout=1.0), dict(dropout=-0.1), dict(dropout="0.5"), dict(dropout=None), dict(dropout=True),
       dict(dropout=float("nan")), dict(seed=-1), dict(seed=2 ** 32), dict(seed=1.0), dict(batch=0),
       dict(batch=1.5), dict(backend="numpy")]


@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_refusals_come_before_any_forward(kw):
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    seen = []
    keep = type(clf)._torch_features
    type(clf)._torch_features = lambda *a, **k: seen.append(1) or keep(*a, **k)
    try:
        for obj in (clf, ens, m):
            with pytest.raises(ValueError):
                obj.predict_mc(x[:4], **kw)
        assert not seen
        clf.predict_mc(x[:4], samples=2, seed=2 ** 32 - 1, dropout=np.float32(0.25))
        assert seen
    finally:
        type(clf)._torch_features = keep


def test_model_forwards_its_dropout_probability():
    from gentun_amd.models.cnn import GeneticCnnModel
    m, clf, x = T._fit("rgb")
    assert m.dropout_probability == 0.5
    m.dropout_probability = 0.25
    try:
        assert m.predict_mc(x[:4], seed=1)["std"].tobytes() == clf.predict_mc(x[:4], seed=1, dropout=0.25)["std"].tobytes()
        assert m.predict_mc(x[:4], dropout=0.5)["std"].tobytes() == clf.predict_mc(x[:4])["std"].tobytes()
    finally:
        m.dropout_probability = 0.5
    shape, classes, _ = T.CASES["rgb"]
    fresh = GeneticCnnModel(x, np.eye(classes, dtype=np.float32)[np.arange(len(x)) % classes], T.GENOMES[0],
                            device="cpu", **T._space("rgb"))
    with pytest.raises(RuntimeError):
        fresh.predict_mc(x[:4])
    clf.classes = 17                                                 # refused before a predictor is built: no GPU here
    try:
        with pytest.raises(ValueError, match="16 classes"):
            clf.predict_mc(x[:4], backend="hip")
    finally:
        clf.classes = 4


def test_predict_and_model_files_are_unchanged(tmp_path):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    before, after = str(tmp_path / "before.npz"), str(tmp_path / "after.npz")
    for obj, load in ((clf, CnnClassifier.load), (ens, CnnEnsemble.load)):
        header = json.dumps(obj.header())
        obj.save(before)
        plain = obj.predict(x[:40])
        want = obj.predict_mc(x[:4], samples=4)
        obj.save(after)
        assert T._sha(before) == T._sha(after) and json.dumps(obj.header()) == header and "dropout" not in header
        assert load(after).predict_mc(x[:4], samples=4)["std"].tobytes() == want["std"].tobytes()
        assert obj.predict(x[:40]).tobytes() == plain.tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_mc_dropout.py"), "--device", "cpu",
                        "--images", "16", "--samples", "8"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"images", "samples", "accuracy", "mutual_info_held_out", "mutual_info_noise"}
    assert out["mutual_info_held_out"] >= 0 and out["mutual_info_noise"] >= 0
