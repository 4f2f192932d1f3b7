"""``saliency`` of fitted Genetic-CNN models on the CPU (torch backend): central differences of the fp64 score, the
methods and reductions against their formulas, completeness, ensembles, refusals. Fits: tests/test_cnn_tta.py."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS = 6
CPU = torch.device("cpu")


def _score64(clf, x64, t, score):
    return clf._torch_input_grad(x64, t, score, CPU, 256, torch.float64)[2]


@pytest.mark.parametrize("score", ["logit", "proba"])
@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_gradient_against_central_differences(case, score):
    """``<g, d>`` in fp64 along random directions against ``(s(x + e d) - s(x - e d)) / 2e``, e = 1e-6, bound 1e-6."""
    m, clf, x = T._fit(case)
    xs = x[:NROWS].astype(np.float64)
    rng = np.random.default_rng(7)
    t = rng.integers(0, clf.classes, NROWS)
    g = clf._torch_saliency(x[:NROWS], t, score, "gradient", 1, np.zeros(xs.shape[3], np.float32), CPU, 256,
                            torch.float64)[0]
    assert g.dtype == np.float64 and g.shape == xs.shape
    eps, worst = 1e-6, 0.0
    for k in range(4):
        d = rng.standard_normal(xs.shape)
        d /= np.sqrt((d ** 2).sum((1, 2, 3), keepdims=True))
        fd = (_score64(clf, xs + eps * d, t, score) - _score64(clf, xs - eps * d, t, score)) / (2 * eps)
        an = (g * d).sum((1, 2, 3))
        worst = max(worst, float(np.abs(fd - an).max() / np.abs(an).max()))
    print("[cnn-saliency] gradient vs central differences ({}, {}): {:.3e}".format(case, score, worst))
    assert np.abs(g).max() > 0 and worst <= 1e-6


@pytest.mark.parametrize("case", ["mnist", "rgb"])
def test_methods_reductions_and_batches(case):
    m, clf, x = T._fit(case)
    xs = x[:40]
    C = xs.shape[3]
    x0 = np.linspace(-0.5, 0.25, C).astype(np.float32)
    g, info = clf.saliency(xs, reduce=None, return_info=True)
    t = info["target"]
    assert np.array_equal(t, clf.predict(xs, output="label")) and set(info) == {"target", "base"}
    assert info["base"].tobytes() == clf.predict(xs, output="logits")[np.arange(40), t].tobytes()
    assert clf.saliency(xs, method="gradxinput", reduce=None).tobytes() == (xs * g).tobytes()
    mid = x0 + np.float32(0.5) * (xs - x0)
    gm = clf.saliency(mid, target=t, reduce=None)
    ig, iinfo = clf.saliency(xs, method="integrated", steps=1, baseline=x0, reduce=None, return_info=True)
    assert ig.tobytes() == ((xs - x0) * (gm * np.float32(1))).tobytes() and np.array_equal(iinfo["target"], t)
    assert iinfo["baseline_score"].tobytes() == \
        clf.predict(np.broadcast_to(x0, (1,) + xs.shape[1:]).copy(), output="logits")[0][t].tobytes()
    assert clf.saliency(xs).tobytes() == np.abs(g).max(3).tobytes()                       # absmax is the default
    want = g[..., 0] if C == 1 else (g[..., 0] + g[..., 1]) + g[..., 2]
    assert clf.saliency(xs, reduce="sum").tobytes() == want.tobytes()
    for kw in (dict(), dict(method="integrated", steps=3, score="proba")):                # batch 32 = batch 256
        assert clf.saliency(xs, batch=32, **kw).tobytes() == clf.saliency(xs, batch=256, **kw).tobytes()
    assert m.saliency(xs[:4], target=1).tobytes() == clf.saliency(xs[:4], target=1).tobytes()


@pytest.mark.parametrize("score", ["logit", "proba"])
def test_integrated_gradients_completeness(score):
    """In fp64 the largest ``|sum a - (base - baseline_score)|`` of the images shrinks from 4 to 64 steps of the
    midpoint rule (a single image's 4-step sum can land close by chance; the score is only piecewise smooth)."""
    m, clf, x = T._fit("rgb")
    gap = {}
    for steps in (4, 64):
        a, t, base, bs = clf._torch_saliency(x[:NROWS], None, score, "integrated", steps, np.zeros(3, np.float32), CPU,
                                             256, torch.float64)
        gap[steps] = np.abs(a.sum((1, 2, 3)) - (base - bs))
    print("[cnn-saliency] completeness gap", score, "4 steps", gap[4].max(), "64 steps", gap[64].max())
    assert gap[64].max() < gap[4].max()


def test_ensemble_is_the_ordered_combine_of_its_members():
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_ensemble import combine_maps
    fitted, x = T._ensemble("rgb")
    xs = x[:NROWS]
    for weights in (None, [3.0, 1.0, 4.0]):
        ens = fitted if weights is None else CnnEnsemble(fitted.members, weights=weights)
        for score, method in (("proba", "gradient"), ("logit", "integrated")):
            got, info = ens.saliency(xs, score=score, method=method, steps=2, reduce=None, return_info=True)
            t = info["target"]
            assert np.array_equal(t, ens.predict(xs, output="label"))
            per = [mem.saliency(xs, target=t, score=score, method=method, steps=2, reduce=None, return_info=True)
                   for mem in ens.members]
            assert got.tobytes() == combine_maps([p[0] for p in per], ens.weights).tobytes()
            assert info["base"].tobytes() == combine_maps([p[1]["base"] for p in per], ens.weights).tobytes()


BAD = [dict(score="loss"), dict(method="smoothgrad"), dict(steps=0), dict(steps=65), dict(steps=2.0), dict(steps=True),
       dict(baseline=[0.0, 1.0]), dict(baseline=float("nan")), dict(baseline="x"), dict(reduce="max"), dict(reduce=0),
       dict(target=7), dict(target=[0, 1]), dict(target=1.5), dict(batch=0), dict(batch=2.5), dict(backend="tf")]


@pytest.mark.parametrize("bad", BAD, ids=[str(sorted(b.items())[0]) for b in BAD])
def test_refusals_come_before_any_forward(bad, monkeypatch):
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    for obj, owners in ((clf, [clf]), (ens, ens.members)):
        ran = []
        for o in owners:
            monkeypatch.setattr(o, "_torch_forward", lambda *a, **k: ran.append(1))
            monkeypatch.setattr(o, "hip_predictor", lambda *a, **k: ran.append(1))
        with pytest.raises(ValueError):
            obj.saliency(x[:3], **bad)
        assert not ran


def test_predict_and_model_files_are_unchanged(tmp_path):
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    before, after = str(tmp_path / "before.npz"), str(tmp_path / "after.npz")
    for obj in (clf, ens):
        obj.save(before)
        plain, cam = obj.predict(x[:40]), obj.gradcam(x[:4])
        obj.saliency(x[:4], method="integrated", steps=2)
        obj.save(after)
        assert T._sha(before) == T._sha(after)
        assert obj.predict(x[:40]).tobytes() == plain.tobytes() and obj.gradcam(x[:4]).tobytes() == cam.tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_saliency.py"), "--device", "cpu",
                        "--steps", "4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["map"] == [16, 16] and out["method"] == "integrated" and out["largest"] > 0
    assert out["completeness_gap"] is not None and r.stdout.count("\n") > 16 * out["images"]
