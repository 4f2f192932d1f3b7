"""RISE saliency of fitted Genetic-CNN models on the CPU (torch executor): ``rise_check``, ``rise_masks`` and the
``rise`` method of ``CnnClassifier`` / ``CnnEnsemble`` / ``GeneticCnnModel``. The contract: the masks are those of
the loop oracle tests/rise_ref.py byte for byte, and the map is the oracle's fp64 accumulate of the floats the
plain ``predict`` returns for the oracle's views. The fits are those of tests/test_cnn_tta.py (shared, unchanged)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rise_ref as R
import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS, MASKS = 3, 40
SETTINGS = {"mnist": (7, 0.5, 0.0), "mnist_bn": (4, 0.3, -0.5), "rgb": (7, 0.5, [0.5, -1.0, 0.25]),
            "rgb_bn": (16, 0.7, 0.0)}                  # case -> (cells, p, fill)


@pytest.mark.parametrize("H, W, cells, p", [(6, 5, 2, 0.5), (28, 28, 7, 0.5), (32, 32, 7, 0.1), (32, 32, 7, 0.9),
                                            (32, 32, 16, 0.5)])
def test_numpy_twin_equals_the_oracle(H, W, cells, p):
    from gentun_amd.models.cnn_fitted import rise_masks
    got = rise_masks((H, W, 1), 6, cells, p, 11)
    assert got.dtype == np.float32 and got.shape == (6, H, W)
    assert got.tobytes() == R.masks(H, W, 6, cells, p, 11).tobytes()
    assert got.min() >= 0 and got.max() <= 1 and 0 < got.mean() < 1
    assert rise_masks((H, W, 1), 2, cells, p, 11, first=3).tobytes() == got[3:5].tobytes()


def test_one_pinned_mask():
    """Mask 0 of 6 x 5 at cells = 2, p = 0.5, seed 0 (cells of 3 x 3 pixels): every value is a ninth."""
    want = np.array([[2, 0, 2, 4, 6], [3, 0, 3, 6, 9], [4, 3, 4, 5, 6], [5, 6, 5, 4, 3], [6, 9, 6, 3, 0],
                     [6, 9, 7, 5, 3]]) / 9.0
    assert np.abs(R.mask(6, 5, 0, 2, 0.5, 0) - want).max() <= 2.0 ** -23


def test_mean_of_2048_masks_is_p():
    """Every pixel of a mask lies in [0, 1] with mean p (a convex mix of Bernoulli(p) bits), so its variance is at
    most p (1 - p) and the mean of 2,048 independent masks lies within 5 standard deviations, 5 * sqrt(0.25 / 2048)
    = 0.055, of p at every pixel (two-sided tail 6e-7 x 1,024 pixels). The oracle's own 2,048 masks were checked
    against the same bound once: largest deviation 0.0213."""
    from gentun_amd.models.cnn_fitted import rise_masks
    mean = rise_masks((32, 32, 3), 2048, 7, 0.5, 0).mean(0, dtype=np.float64)
    assert np.abs(mean - 0.5).max() <= 5 * np.sqrt(0.25 / 2048)


def _want(predict, x, t, cells, p, seed, fill, batch, n_masks=MASKS):
    Ms = R.masks(x.shape[1], x.shape[2], n_masks, cells, p, seed)
    sv = predict(R.views(x, Ms, fill), batch).reshape(len(x), n_masks, -1)[np.arange(len(x)), :, t]
    return R.accumulate(sv, Ms, p), predict(x, batch)[np.arange(len(x)), t]


@pytest.mark.parametrize("score", ["proba", "logit"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_map_is_the_oracles_accumulate_of_plain_predictions(case, score):
    m, clf, x = T._fit(case)
    xs = x[:NROWS]
    cells, p, fill = SETTINGS[case]
    label = clf.predict(xs, output="label")
    other = (label + 1) % clf.classes

    def predict(images, batch):
        return clf.predict(images, output="logits" if score == "logit" else "proba", batch=batch)
    for batch, target, t in ((256, None, label), (32, 1, np.full(NROWS, 1)), (32, other, other)):
        want, base = _want(predict, xs, t, cells, p, 5, fill, batch)
        got, info = clf.rise(xs, target=target, masks=MASKS, cells=cells, p=p, seed=5, fill=fill, score=score,
                             batch=batch, return_info=True)
        assert got.dtype == np.float32 and got.shape == xs.shape[:3] and np.isfinite(got).all()
        assert got.tobytes() == want.tobytes(), (target, batch, float(np.abs(got - want).max()))
        assert info["target"].dtype == np.int64 and np.array_equal(info["target"], t)
        assert info["base"].dtype == np.float32 and info["base"].tobytes() == base.tobytes()
    kw = dict(masks=MASKS, cells=cells, p=p, fill=fill, score=score)
    assert m.rise(xs, target=other, seed=5, batch=32, **kw).tobytes() == got.tobytes()      # the model forwards
    assert clf.rise(xs, target=other, seed=5, batch=32, **kw).tobytes() == got.tobytes()    # the same seed repeats
    assert clf.rise(xs, target=other, seed=6, batch=32, **kw).tobytes() != got.tobytes()
    assert clf.rise(xs[1], seed=5, **kw).tobytes() == clf.rise(xs[1:2], seed=5, **kw).tobytes()


@pytest.mark.parametrize("weights", [None, [3.0, 1.0, 4.0]])
@pytest.mark.parametrize("k", [1, 3])
def test_ensemble_scores_are_the_combine_of_its_members(k, weights):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_ensemble import combine
    fitted, x = T._ensemble("rgb_bn")
    ens = CnnEnsemble(fitted.members[:k], weights=None if weights is None else weights[:k])
    xs = x[:NROWS]

    def predict(images, batch):
        return combine(np.stack([mb.predict(images, batch=batch) for mb in ens.members]), ens.weights)[0]
    label = ens.predict(xs, output="label")
    for target, t in ((None, label), ((label + 1) % ens.classes,) * 2):
        want, base = _want(predict, xs, t, 7, 0.5, 2, [0.5, -1.0, 0.25], 32)
        got, info = ens.rise(xs, target=target, masks=MASKS, seed=2, fill=[0.5, -1.0, 0.25], batch=32,
                             return_info=True)
        assert got.tobytes() == want.tobytes() and info["base"].tobytes() == base.tobytes()
        assert np.array_equal(info["target"], t)
    if k == 1:
        assert got.tobytes() == ens.members[0].rise(xs, target=t, masks=MASKS, seed=2, fill=[0.5, -1.0, 0.25],
                                                    batch=32).tobytes()
    with pytest.raises(ValueError):
        ens.rise(xs, score="logit")


def test_a_constant_score_gives_the_sum_of_the_masks():
    from gentun_amd.models.cnn_fitted import rise_by_views, rise_masks
    x = np.zeros((2, 6, 5, 3), np.float32)

    def scores(images):
        s = np.full((len(images), 4), 0.375, np.float32)
        return s, s
    got = rise_by_views(scores, x, np.array([1, 2]), 33, 2, 0.25, 9, np.zeros(3, np.float32), 8)[0]
    want = 0.375 * rise_masks(x.shape[1:], 33, 2, 0.25, 9).sum(0, dtype=np.float64) / (33 * 0.25)
    assert np.allclose(got, want, rtol=1e-6, atol=0) and got[0].tobytes() == got[1].tobytes()


def test_every_refusal_comes_before_a_forward(monkeypatch):
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")

    def forward(*a, **kw):
        raise AssertionError("a forward ran")
    monkeypatch.setattr(CnnClassifier, "_torch_predict", forward)
    for obj in (clf, ens, m):
        for kw in (dict(masks=0), dict(masks=8193), dict(masks=2.0), dict(masks=True), dict(cells=1), dict(cells=17),
                   dict(cells=7.0), dict(p=0.0), dict(p=1.0), dict(p=-0.5), dict(p="0.5"), dict(p=None),
                   dict(seed=-1), dict(seed=2 ** 32), dict(seed=1.5), dict(target=3), dict(target=[0, 1]),
                   dict(fill=[1.0, 2.0]), dict(fill=float("nan")), dict(score="logits"), dict(batch=0),
                   dict(backend="numpy")):
            with pytest.raises(ValueError):
                obj.rise(x[:4], **kw)
    with pytest.raises(ValueError):
        clf.rise(x[:4, :27])                                                # not this model's images
    from gentun_amd.models.cnn_fitted import rise_check
    for n, masks, cells in ((1, 8, 6), (2 ** 18, 8192, 5)):                 # cells <= min(H, W); 2^31 items
        with pytest.raises(ValueError):
            rise_check((6, 5, 1), n, masks, cells, 0.5, 0, 32)
    assert rise_check((6, 5, 1), 1, 8, np.int64(5), 0.5, 0, 32) == (8, 5, 0.5, 0)


def test_predict_and_model_files_are_unchanged(tmp_path):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    before, after = str(tmp_path / "before.npz"), str(tmp_path / "after.npz")
    for obj, load in ((clf, CnnClassifier.load), (ens, CnnEnsemble.load)):
        obj.save(before)
        plain = obj.predict(x[:40])
        want = obj.rise(x[:2], masks=8)
        obj.save(after)
        assert T._sha(before) == T._sha(after) and "rise" not in json.dumps(obj.header())
        back = load(after)
        assert back.rise(x[:2], masks=8).tobytes() == want.tobytes()
        assert back.predict(x[:40]).tobytes() == plain.tobytes() == obj.predict(x[:40]).tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_rise.py"), "--device", "cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"images", "shape", "masks", "cells", "largest"} and out["shape"] == [16, 16]
