"""Occlusion sensitivity of fitted Genetic-CNN models on the CPU (torch executor): ``occlusion_grid``,
``occlusion_views`` and the ``occlusion`` method of ``CnnClassifier`` / ``CnnEnsemble`` / ``GeneticCnnModel``
(gentun_amd/models/cnn_fitted.py, cnn_ensemble.py, cnn.py).

Every comparison is byte equality or a refusal. The contract: ``map[r, gi, gj] = s(x[r]) - s(O_cell(x[r]))``, one
fp32 subtraction, with ``O_cell`` by the per-pixel oracle tests/occlusion_ref.py and ``s`` the plain ``predict``
of the same model. The fits are those of tests/test_cnn_tta.py (shared inside one pytest process, left
unchanged)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import occlusion_ref as R
import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS = 6


# ---------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------

def test_grid_sizes():
    from gentun_amd.models.cnn_fitted import OCC_MAX_CELLS, occlusion_grid
    assert occlusion_grid((32, 32, 3), 4, 4) == (8, 8)
    assert occlusion_grid((32, 32, 3), 4) == (8, 8) and occlusion_grid((32, 32, 3), 4, None) == (8, 8)
    assert occlusion_grid((32, 32, 3), 4, 2) == (15, 15)
    assert occlusion_grid((28, 28, 1), 4, 2) == (13, 13)
    assert occlusion_grid((6, 5, 3), 4, 3) == (2, 2)                     # windows [0, 4), [3, 6) / [3, 5): clipped
    assert R.windows(6, 4, 3) == [(0, 4), (3, 6)] and R.windows(5, 4, 3) == [(0, 4), (3, 5)]
    assert occlusion_grid((28, 28, 1), 28) == (1, 1) and occlusion_grid((6, 5, 3), 5) == (2, 1)
    assert occlusion_grid((6, 5, 3), np.int64(2), np.int32(1)) == (5, 4)
    assert occlusion_grid((64, 64, 1), 1) == (64, 64) and OCC_MAX_CELLS == 4096      # exactly the most
    assert all(type(v) is int for v in occlusion_grid((6, 5, 3), np.int64(2), np.int32(1)))
    for H, W in ((6, 5), (7, 7), (28, 28), (9, 32)):                     # the formula against the walk
        for patch in range(1, min(H, W) + 1):
            for stride in range(1, patch + 1):
                assert occlusion_grid((H, W, 1), patch, stride) == R.grid(H, W, patch, stride), (H, W, patch, stride)


@pytest.mark.parametrize("patch, stride", [
    (4, 5), (1, 2),                                     # stride > patch: pixels would be skipped
    (0, None), (0, 0), (4, 0), (-1, None), (4, -1), (-4, -4),
    (4.0, None), (4, 2.0), (2.5, 1), ("4", None), (4, "2"), (True, None), (4, True), (None, None), ((4, 4), None),
    (7, None), (6, 1),                                  # patch <= min(6, 5)
])
def test_grid_refusals(patch, stride):
    from gentun_amd.models.cnn_fitted import occlusion_grid
    with pytest.raises(ValueError):
        occlusion_grid((6, 5, 3), patch, stride)


def test_grid_refuses_more_than_4096_cells():
    from gentun_amd.models.cnn_fitted import occlusion_grid
    with pytest.raises(ValueError):
        occlusion_grid((65, 64, 1), 1)
    with pytest.raises(ValueError):
        occlusion_grid((128, 128, 3), 2, 1)
    assert occlusion_grid((128, 128, 3), 2, 2) == (64, 64)


# ---------------------------------------------------------------------------------------------------------
# the numpy twin against the oracle
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(6, 5, 3), (28, 28, 1)])
def test_numpy_twin_equals_the_oracle(shape):
    from gentun_amd.models.cnn_fitted import occlusion_grid, occlusion_views
    H, W, C = shape
    x = np.random.default_rng(H).standard_normal((2,) + shape).astype(np.float32)
    x[0, 0, 0, 0] = -0.0                                # copied, never changed: the sign of a zero too
    keep = x.copy()
    settings = [(1, 1), (2, 2), (3, 2), (4, 3), (4, 1), (min(H, W), None), (min(H, W), 1), (5, 4)]
    fills = [0.0, -1.5, np.float32(0.25)] + ([[0.5, -2.0, 3.0], (1, 2, 3), np.array([-0.0, 0.0, 7.0])] if C == 3
                                             else [[2.0], np.array([-3.5])])
    for k, (patch, stride) in enumerate(settings):
        Gh, Gw = occlusion_grid(shape, patch, stride)
        for fill in (fills if k < 3 else fills[k % len(fills):][:1]):
            got = occlusion_views(x, patch, stride, fill)
            assert got.shape == (2, Gh * Gw, H, W, C) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
            want = R.views(x, patch, patch if stride is None else stride, fill)
            assert got.tobytes() == want.tobytes(), (patch, stride, fill)
            assert got.tobytes() != np.repeat(x[:, None], Gh * Gw, 1).tobytes()
    assert x.tobytes() == keep.tobytes()                                 # the input is left alone
    # the clipped edge cells of 6 x 5 at patch 4 / stride 3: 2 x 1 pixels in the corner
    if shape == (6, 5, 3):
        v = occlusion_views(x, 4, 3, 9.0)
        changed = (v[0, 3] != x[0]).any(-1)
        assert changed.sum() == 3 * 2 and changed[3:, 3:].all()
    assert occlusion_views(x, 2).tobytes() == occlusion_views(x, 2, 2, 0.0).tobytes()
    for bad in ([1.0, 2.0], [1.0] * (C + 1), "a", None, float("nan"), [float("inf")] * C, [[0.0] * C]):
        with pytest.raises(ValueError):
            occlusion_views(x, 2, 2, bad)


# ---------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------

_VIEWS = {}


def _oracle_views(x, patch, stride, fill):
    """``[n * Cc, H, W, C]`` by the oracle; computed once per (image set, setting)."""
    key = (x.shape, x[:2].tobytes(), patch, stride, repr(fill))
    if key not in _VIEWS:
        v = R.views(x, patch, stride, fill)
        _VIEWS[key] = v.reshape((-1,) + x.shape[1:])
    return _VIEWS[key]


def _want(predict, x, target, patch, stride, fill):
    """``(map, target, base)`` written out: plain predicts of the images and of the oracle's copies."""
    n = len(x)
    base_all = predict(x)
    t = np.asarray(target)
    views = _oracle_views(x, patch, stride, fill)
    Cc = len(views) // n
    sv = predict(views).reshape(n, Cc, -1)
    base = base_all[np.arange(n), t]
    out = np.empty((n, Cc), np.float32)
    for r in range(n):
        for cell in range(Cc):
            out[r, cell] = np.subtract(base[r], sv[r, cell, t[r]], dtype=np.float32)
    return out.reshape((n,) + R.grid(x.shape[1], x.shape[2], patch, stride)), base


SETTINGS = {"mnist": (4, 2, 0.0), "mnist_bn": (7, 7, -0.5), "rgb": (8, 8, [0.5, -1.0, 0.25]), "rgb_bn": (12, 10, 0.0)}


@pytest.mark.parametrize("score", ["proba", "logit"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_map_is_base_minus_the_predictions_of_the_oracles_views(case, score):
    """At both batch sizes the map is made of the floats ``predict`` returns at that batch size for the oracle's
    copies (up to 1014 rows here, several forwards of 256 or 32 rows)."""
    m, clf, x = T._fit(case)
    xs = x[:NROWS]
    patch, stride, fill = SETTINGS[case]
    output = "logits" if score == "logit" else "proba"
    label = clf.predict(xs, output="label")
    other = (label + 1 + np.arange(NROWS) % (clf.classes - 1)) % clf.classes       # never the predicted class
    assert (other != label).all()
    for batch in (256, 32):
        def predict(images):
            return clf.predict(images, output=output, batch=batch)
        for target, t in ((None, label), (1, np.full(NROWS, 1)), (np.int64(0), np.zeros(NROWS, int)),
                          (other, other), (list(other), other)):
            want, base = _want(predict, xs, t, patch, stride, fill)
            got, info = clf.occlusion(xs, target=target, patch=patch, stride=stride, fill=fill, score=score,
                                      batch=batch, return_info=True)
            assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
            assert got.tobytes() == want.tobytes(), (target, batch, float(np.abs(got - want).max()))
            assert set(info) == {"target", "base"}
            assert info["target"].dtype == np.int64 and np.array_equal(info["target"], t)
            assert info["base"].dtype == np.float32 and info["base"].tobytes() == base.tobytes()
            plain = clf.occlusion(xs, target=target, patch=patch, stride=stride, fill=fill, score=score, batch=batch)
            assert isinstance(plain, np.ndarray) and plain.tobytes() == got.tobytes()
    assert np.abs(got).max() > 0                        # the copies are not the image
    one = clf.occlusion(xs[2], patch=patch, stride=stride, fill=fill, score=score)           # one [H, W, C] image
    assert one.tobytes() == clf.occlusion(xs[2:3], patch=patch, stride=stride, fill=fill, score=score).tobytes()


@pytest.mark.parametrize("case", ["mnist_bn", "rgb"])
def test_batch_32_and_256_give_equal_bits(case):
    """6 images x 16 cells = 96 copies: one forward of 96 rows at batch 256, three of 32 at batch 32. The
    stock-torch CPU forward that ``predict`` runs returns the same bits for a row up to 128 rows per forward
    and not beyond (measured: ``predict(x[:b], batch=b)`` against ``predict(x[:b], batch=32)`` is equal at b = 64,
    96, 128 and off by one ulp of the largest logit at b = 160 to 256), which is why the project's CPU chunking
    tests stay at 96 rows or fewer; so does this one. Beyond that the map follows ``predict`` at the same
    ``batch`` (the test above)."""
    m, clf, x = T._fit(case)
    xs = x[:NROWS]
    patch = clf.input_shape[0] // 4
    for score in ("proba", "logit"):
        a = clf.occlusion(xs, patch=patch, fill=0.5, score=score, batch=256)
        assert a.shape == (NROWS, 4, 4)
        assert clf.occlusion(xs, patch=patch, fill=0.5, score=score, batch=32).tobytes() == a.tobytes()
        assert clf.occlusion(xs[::-1], patch=patch, fill=0.5, score=score, batch=32)[::-1].tobytes() == a.tobytes()
        assert clf.occlusion(xs[:5], patch=patch, fill=0.5, score=score, batch=64).tobytes() == a[:5].tobytes()


def test_defaults_are_patch_4_stride_4_fill_0_proba():
    m, clf, x = T._fit("rgb")
    got = clf.occlusion(x[:3])
    assert got.shape == (3, 8, 8)
    assert got.tobytes() == clf.occlusion(x[:3], None, 4, 4, 0.0, "proba", "cpu", 256, "torch", False).tobytes()


@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_a_cell_that_already_holds_the_fill_scores_exactly_zero(case):
    m, clf, x = T._fit(case)
    C = clf.input_shape[2]
    fill = [0.5, -1.0, 0.25][:C]
    xs = x[:3].copy()
    xs[0, 8:16, 16:24] = fill                           # cell (1, 2) of patch 8 / stride 8
    xs[1] = fill                                        # every cell
    for score in ("proba", "logit"):
        got = clf.occlusion(xs, patch=8, stride=8, fill=fill, score=score)
        assert got[0, 1, 2] == 0.0 and got[0].any()
        assert not got[1].any() and got[2].any()
    assert not clf.occlusion(np.zeros_like(xs), patch=5, stride=3).any()        # the default fill


def test_refusals():
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    for obj in (clf, ens, m):
        for kw in (dict(patch=0), dict(patch=29), dict(patch=4, stride=5), dict(patch=4.0), dict(stride=0),
                   dict(patch=-1), dict(target=3), dict(target=-1), dict(target=[0, 1]), dict(target=[0, 1, 2, 3, 3]),
                   dict(target=1.0), dict(target=[[0, 1, 2, 0]]), dict(target=True),
                   dict(fill=[1.0, 2.0]), dict(fill="x"), dict(fill=float("nan")),
                   dict(score="logits"), dict(score="label"), dict(score=None), dict(batch=0),
                   dict(backend="numpy")):
            with pytest.raises(ValueError):
                obj.occlusion(x[:4], **kw)
    assert clf.occlusion(x[:1], patch=1).shape == (1, 28, 28)            # 784 cells of one pixel: allowed
    with pytest.raises(ValueError):
        ens.occlusion(x[:4], score="logit")
    with pytest.raises(ValueError):
        clf.occlusion(x[:4, :27])
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes, _ = T.CASES["mnist"]
    fresh = GeneticCnnModel(x, np.eye(classes, dtype=np.float32)[np.arange(len(x)) % classes], T.GENOMES[0],
                            device="cpu", **T._space("mnist"))
    with pytest.raises(RuntimeError):
        fresh.occlusion(x[:4])


# ---------------------------------------------------------------------------------------------------------
# the ensemble
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, [3.0, 1.0, 4.0]])
@pytest.mark.parametrize("k", [1, 3])
def test_ensemble_is_the_combine_of_its_members(k, weights):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_ensemble import combine
    fitted, x = T._ensemble("rgb_bn")
    ens = CnnEnsemble(fitted.members[:k], weights=None if weights is None else weights[:k])
    xs = x[:NROWS]
    patch, stride, fill = 8, 6, [0.5, -1.0, 0.25]

    def predict(images):
        return combine(np.stack([member.predict(images) for member in ens.members]), ens.weights)[0]
    assert predict(xs).tobytes() == ens.predict(xs).tobytes()
    label = ens.predict(xs, output="label")
    other = (label + 1) % ens.classes
    for target, t in ((None, label), (2, np.full(NROWS, 2)), (other, other)):
        want, base = _want(predict, xs, t, patch, stride, fill)
        got, info = ens.occlusion(xs, target=target, patch=patch, stride=stride, fill=fill, return_info=True)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), float(np.abs(got - want).max())
        assert np.array_equal(info["target"], t) and info["base"].tobytes() == base.tobytes()
    a = ens.occlusion(xs, patch=8, fill=fill, batch=256)                 # 96 copies: see the classifier's test
    assert a.shape == (NROWS, 4, 4) and ens.occlusion(xs, patch=8, fill=fill, batch=32).tobytes() == a.tobytes()
    if k == 1:                                          # one member of weight 1.0 is its classifier
        assert ens.occlusion(xs, patch=patch, stride=stride, fill=fill).tobytes() == \
            ens.members[0].occlusion(xs, patch=patch, stride=stride, fill=fill).tobytes()
    with pytest.raises(ValueError):
        ens.occlusion(xs, score="logit")


# ---------------------------------------------------------------------------------------------------------
# around it
# ---------------------------------------------------------------------------------------------------------

def test_model_forwards_the_arguments():
    m, clf, x = T._fit("rgb")
    kw = dict(target=1, patch=8, stride=4, fill=0.5, score="logit")
    got, info = m.occlusion(x[:4], return_info=True, **kw)
    want, winfo = clf.occlusion(x[:4], return_info=True, **kw)
    assert got.shape == (4, 7, 7) and got.tobytes() == want.tobytes()
    assert info["base"].tobytes() == winfo["base"].tobytes() and (info["target"] == 1).all()


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
        want = obj.occlusion(x[:4], patch=7)
        obj.save(after)
        assert T._sha(before) == T._sha(after) and json.dumps(obj.header()) == header and "occlu" not in header
        back = load(after)
        assert back.occlusion(x[:4], patch=7).tobytes() == want.tobytes()
        assert back.predict(x[:40]).tobytes() == plain.tobytes() == obj.predict(x[:40]).tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_occlusion.py"), "--device", "cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"images", "grid", "patch", "stride", "largest_drop"} and out["grid"] == [4, 4]
    assert r.stdout.count("\n") > 4 * out["images"]                     # the text heat maps came first
