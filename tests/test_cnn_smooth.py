"""``saliency(smooth=...)`` on the CPU (torch backend): the noise twin against its formula, the maps byte-equal to the
written-out statistics of the per-point gradients, ensembles, refusals. Fits: tests/test_cnn_tta.py."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F1 = np.float32(1)


def _points(x, samples, noise, seed, n0=0):
    """The noisy copies of fp32 ``x`` in sample order: ``x + fp32(sigma_n * z)``."""
    from gentun_amd.utils.rng import sg_noise
    n, h, w, c = x.shape
    sigma = np.float32(noise) * (x.max(axis=(1, 2, 3)) - x.min(axis=(1, 2, 3)))
    z = sg_noise(seed, n0 + np.arange(n), samples, h, w, c)
    return [x + (sigma.astype(np.float64)[:, None, None, None] * z[:, k]).astype(np.float32) for k in range(samples)]


def _finish(gs, x, method, stat):
    """The definition, written out: ordered fp32 sums, ``* (1 / S)``, the statistic, the method factor."""
    s1, s2 = gs[0], gs[0] * gs[0]
    for g in gs[1:]:
        s1, s2 = s1 + g, s2 + g * g
    inv = F1 / np.float32(len(gs))
    mean, msq = s1 * inv, s2 * inv
    a = {"mean": mean, "sq": msq, "var": np.maximum(msq - mean * mean, np.float32(0))}[stat]
    return a if method == "gradient" else a * (x if stat == "mean" else x * x)


def test_sg_noise_pinned_draws_moments_and_keys():
    from gentun_amd.utils.rng import sg_noise
    # (seed, n, k, p, c) -> z: hash4, u = ((r >> 9) * 2 + 1) 2^-24, sqrt(-2 ln u0) cos(2 pi u1), in Python floats
    pinned = [((7, 0, 0, 0, 0), 1.0310756390668048), ((7, 3, 2, 17, 1), -0.06309380026234383),
              ((7, 1000, 63, 1023, 2), 1.5447209631571526), ((4294967295, 5, 1, 29, 0), 0.5595083360494522)]
    for (seed, n, k, p, c), want in pinned:
        z = sg_noise(seed, n, 64, 32, 32, 3)
        assert z.dtype == np.float64 and z.shape == (1, 64, 32, 32, 3)
        assert abs(z[0, k, p // 32, p % 32, c] - want) <= 1e-15
    z = sg_noise(1, np.arange(82), 4, 32, 32, 3)             # 1,007,616 draws
    se = 1 / np.sqrt(z.size)
    print("[cnn-smooth] mean {:.3e} var - 1 {:.3e} max |z| {:.3f}".format(z.mean(), z.var() - 1, np.abs(z).max()))
    assert abs(z.mean()) <= 5 * se and abs(z.var() - 1) <= 5 * np.sqrt(2) * se and np.abs(z).max() <= 5.77
    assert sg_noise(1, [5, 81], [3], 32, 32, 3).tobytes() == z[[5, 81], 3:4].tobytes()    # (seed, n, k, p, c) only
    assert sg_noise(1, 5, 4, 32, 32, 1).tobytes() == z[5:6, ..., :1].tobytes()
    assert not np.array_equal(sg_noise(2, 5, 4, 32, 32, 3), z[5:6])


@pytest.mark.parametrize("stat", ["mean", "sq", "var"])
@pytest.mark.parametrize("method", ["gradient", "gradxinput"])
@pytest.mark.parametrize("case", ["rgb", "mnist_bn"])
def test_torch_backend_is_the_written_out_finish(case, method, stat):
    from gentun_amd.models.cnn_fitted import smooth_finish
    m, clf, x = T._fit(case)
    xs = x[:40]
    sm = {"samples": 3, "noise": 0.2, "seed": 9, "stat": stat}
    got, info = clf.saliency(xs, method=method, reduce=None, smooth=sm, return_info=True)
    t = info["target"]
    assert np.array_equal(t, clf.predict(xs, output="label")) and set(info) == {"target", "base"}
    assert info["base"].tobytes() == clf.predict(xs, output="logits")[np.arange(40), t].tobytes()
    gs = [clf.saliency(p, target=t, reduce=None) for p in _points(xs, 3, 0.2, 9)]
    want = _finish(gs, xs, method, stat)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes() and np.abs(got).max() > 0
    assert smooth_finish(gs, xs, method, stat).tobytes() == want.tobytes()
    assert clf.saliency(xs, method=method, smooth=sm, batch=32).tobytes() == np.abs(want).max(3).tobytes()
    assert m.saliency(xs[:4], method=method, smooth=sm, reduce=None).tobytes() == want[:4].tobytes()
    assert clf.saliency(xs[8:16], target=t[8:16], method=method, smooth=sm, reduce=None).tobytes() == \
        _finish([clf.saliency(p, target=t[8:16], reduce=None) for p in _points(xs[8:16], 3, 0.2, 9)], xs[8:16],
                method, stat).tobytes()                      # the image index is the one within the call


@pytest.mark.parametrize("samples", [1, 2])
def test_zero_noise_mean_is_the_plain_map(samples):
    m, clf, x = T._fit("rgb")
    for method in ("gradient", "gradxinput"):
        plain = clf.saliency(x[:40], method=method, reduce=None)
        sm = {"samples": samples, "noise": 0, "stat": "mean"}
        assert clf.saliency(x[:40], method=method, reduce=None, smooth=sm).tobytes() == plain.tobytes()


def test_ensemble_is_the_ordered_combine_of_its_members():
    from gentun_amd.models.cnn_ensemble import combine_maps
    ens, x = T._ensemble("rgb")
    xs, sm = x[:6], {"samples": 2, "noise": 0.1, "stat": "var"}
    got, info = ens.saliency(xs, score="proba", method="gradxinput", reduce=None, smooth=sm, return_info=True)
    t = info["target"]
    assert np.array_equal(t, ens.predict(xs, output="label"))
    per = [mem.saliency(xs, target=t, score="proba", method="gradxinput", reduce=None, smooth=sm) for mem in ens.members]
    assert got.tobytes() == combine_maps(per, ens.weights).tobytes() and np.abs(got).max() > 0


BAD = [dict(smooth=4), dict(smooth=[("samples", 4)]), dict(smooth={"sample": 4}), dict(smooth={"samples": 0}),
       dict(smooth={"samples": 65}), dict(smooth={"samples": 2.0}), dict(smooth={"samples": True}),
       dict(smooth={"noise": -0.1}), dict(smooth={"noise": 1.5}), dict(smooth={"noise": float("nan")}),
       dict(smooth={"noise": "0.1"}), dict(smooth={"seed": -1}), dict(smooth={"seed": 2 ** 32}),
       dict(smooth={"seed": 1.0}), dict(smooth={"stat": "median"}), dict(smooth={"stat": 0}),
       dict(smooth={}, method="integrated"), dict(smooth={"samples": 2}, method="smoothgrad")]


@pytest.mark.parametrize("bad", BAD, ids=str)
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


def test_plain_results_and_model_files_are_unchanged(tmp_path):
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    before, after = str(tmp_path / "before.npz"), str(tmp_path / "after.npz")
    for obj in (clf, ens):
        obj.save(before)
        plain = [obj.predict(x[:40]), obj.gradcam(x[:4]), obj.saliency(x[:4]), obj.saliency(x[:4], smooth=None),
                 obj.saliency(x[:4], method="integrated", steps=2)]
        obj.saliency(x[:4], smooth={"samples": 2})
        obj.save(after)
        assert T._sha(before) == T._sha(after) and plain[2].tobytes() == plain[3].tobytes()
        again = [obj.predict(x[:40]), obj.gradcam(x[:4]), obj.saliency(x[:4]), obj.saliency(x[:4], smooth=None),
                 obj.saliency(x[:4], method="integrated", steps=2)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, again))


def test_example_runs_with_smooth():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_saliency.py"), "--device", "cpu",
                        "--method", "gradient", "--smooth", "4", "--stat", "var"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["map"] == [16, 16] and out["smooth"] == {"samples": 4, "noise": 0.15, "stat": "var"}
    assert out["largest"] > 0 and out["completeness_gap"] is None
