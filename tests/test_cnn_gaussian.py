"""``gaussian_fit`` / ``mahalanobis`` of fitted Genetic-CNN models on the CPU (torch executor) against the plain-loop
oracle of tests/gaussian_ref.py. The fits are those of tests/test_cnn_tta.py (shared inside one pytest process,
left unchanged)."""

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gaussian_ref as R
import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("count", "mean", "cov", "whiten", "wmean", "shrink")


def _bank(N, D, classes, seed=0):
    """A full-rank flat bank with class structure; class ``classes - 1`` stays empty."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, classes - 1, N)
    return (rng.standard_normal((N, D)) + 2.0 * rng.standard_normal((classes, D))[lab]).astype(np.float32), lab


def _same(a, b):
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


@pytest.mark.parametrize("ens", [False, True])
@pytest.mark.parametrize("shrink", [0.0, 0.1])
def test_fit_and_distance_equal_the_oracle(shrink, ens):
    from gentun_amd.models.cnn_fitted import mahalanobis_distance
    fitted, x = T._ensemble("rgb")
    obj, G = (fitted, 3) if ens else (fitted.members[0], 1)
    bank, lab = _bank(60, 16 * G, obj.classes)
    st = obj.gaussian_fit(bank, labels=lab, shrink=shrink)
    assert st["cov"].dtype == np.float64 and st["whiten"].dtype == st["mean"].dtype == np.float32
    assert st["count"].dtype == np.int64 and st["count"][-1] == 0 and float(st["shrink"]) == shrink
    for g in range(G):
        f = bank[:, 16 * g:16 * g + 16]
        count, mean, cov = R.moments_ref(f, lab, obj.classes)
        W, t = R.whiten_ref(cov, mean, shrink)
        assert np.array_equal(count, st["count"]) and mean.tobytes() == st["mean"][g].tobytes()
        assert cov.tobytes() == st["cov"][g].tobytes() and np.array_equal(cov, cov.T)
        assert np.abs(W - st["whiten"][g]).max() <= 2.0 ** -22 * np.abs(W).max()
        d = mahalanobis_distance(f, st["whiten"][g], st["wmean"][g], st["count"])
        ref = R.distance_ref(f, st["whiten"][g], st["wmean"][g], st["count"])
        assert d.dtype == np.float32 and np.isinf(d[:, -1]).all() and np.isinf(ref[:, -1]).all()
        assert (np.abs(d[:, :-1] - ref[:, :-1]) <= 2.0 ** -23 * ref[:, :-1]).all()


def test_trace_identity():
    """With ``shrink=0`` the mean over the bank's rows of ``d[r, y_r]`` is ``U``, asserted to 1e-9 relative. The
    definition rounds ``W`` and ``t`` to fp32, which moves that mean by about ``2 * mean_i(eps_i)``, ``|eps_i| <=
    2^-24`` the rounding of ``W_ii``: measured 5e-9 .. 1.4e-8 relative on random 60 x 16 banks, above 1e-9 whatever
    the code does. So the bank here is full rank with a factor that fp32 holds exactly -- two classes of means
    ``+-3``, each holding ``+-s_i e_i`` for every unit, ``s_i`` powers of two: ``cov = diag(s_i^2 / 16)`` -- and on a
    random bank the identity is held to 1e-9 through the fp64 factor of the returned ``cov`` instead."""
    from gentun_amd.models.cnn_fitted import mahalanobis_distance
    _, clf, _ = T._fit("mnist")
    U = 16
    s = 2.0 ** (np.arange(U) % 5 - 2)
    rows = np.concatenate([np.diag(s), -np.diag(s)])
    bank = np.concatenate([rows + 3.0, rows - 3.0]).astype(np.float32)
    lab = np.repeat([0, 1], 2 * U)
    st = clf.gaussian_fit(bank, labels=lab, shrink=0.0)
    own = mahalanobis_distance(bank, st["whiten"][0], st["wmean"][0], st["count"])[np.arange(4 * U), lab]
    assert abs(own.astype(np.float64).mean() - U) <= 1e-9 * U
    bank, lab = _bank(60, U, clf.classes)
    st = clf.gaussian_fit(bank, labels=lab, shrink=0.0)
    z = np.linalg.solve(np.linalg.cholesky(st["cov"][0]), (bank - st["mean"][0][lab]).astype(np.float64).T)
    assert abs((z * z).sum(0).mean() - U) <= 1e-9 * U


def test_label_forms_bank_forms_batch_and_model():
    m, clf, x = T._fit("mnist")
    lab = np.arange(70) % clf.classes
    a = clf.gaussian_fit(x[:70], labels=lab)
    _same(a, clf.gaussian_fit(x[:70], labels=np.eye(clf.classes, dtype=np.float32)[lab]))       # one-hot
    _same(a, clf.gaussian_fit(clf.embed(x[:70]), labels=lab, batch=32))                         # embedded before
    _same(a, m.gaussian_fit(x[:70], labels=lab))
    one = clf.gaussian_fit(x[:70])
    zero = clf.gaussian_fit(x[:70], labels=np.zeros(70, np.int64))                              # C = classes
    _same(one, {k: (zero[k][:1] if k == "count" else zero[k][:, :1] if k in ("mean", "wmean") else zero[k])
                for k in KEYS})
    assert one["count"].tolist() == [70] and one["mean"].shape == (1, 1, 16)
    d = clf.mahalanobis(x[:40], a)
    assert d.dtype == np.float32 and d.shape == (40, clf.classes) and np.isfinite(d).all() and (d >= 0).all()
    assert d.tobytes() == clf.mahalanobis(x[:40], a, batch=32).tobytes() == m.mahalanobis(x[:40], a).tobytes()
    assert clf.mahalanobis(x[0], one).shape == (1, 1)


def test_ensemble_is_the_ordered_mean_of_its_members():
    ens, x = T._ensemble("rgb_bn")
    lab = np.arange(70) % ens.classes
    st = ens.gaussian_fit(x[:70], labels=lab, shrink=0.05)
    assert st["cov"].shape == (3, 16, 16) and st["mean"].shape == (3, ens.classes, 16)
    per = []
    for g, mem in enumerate(ens.members):
        sg = mem.gaussian_fit(x[:70], labels=lab, shrink=0.05)
        assert all(np.asarray(sg[k][0]).tobytes() == np.asarray(st[k][g]).tobytes() for k in KEYS[1:5])
        per.append(mem.mahalanobis(x[:40], sg))
    w = np.asarray(ens.weights, np.float32)
    acc = w[0] * per[0]
    for g in (1, 2):
        acc = acc + w[g] * per[g]
    assert ens.mahalanobis(x[:40], st, batch=32).tobytes() == acc.astype(np.float32).tobytes()


def test_a_singular_covariance_names_shrink():
    _, clf, _ = T._fit("mnist")
    bank, lab = _bank(60, 16, clf.classes)
    bank[:, 3] = 0.0             # a dead unit
    with pytest.raises(ValueError, match="shrink"):
        clf.gaussian_fit(bank, labels=lab, shrink=0.0)
    assert np.isfinite(clf.gaussian_fit(bank, labels=lab, shrink=0.01)["whiten"]).all()


BAD_FIT = [
    (dict(labels="short"), "labels must be"), (dict(labels="range"), "labels must lie"),
    (dict(labels="float"), "labels must be"), (dict(shrink=-0.1), "shrink"), (dict(shrink=1.5), "shrink"),
    (dict(shrink=True), "shrink"), (dict(bank="D15"), "features"), (dict(bank="nan"), "finite"),
    (dict(bank="3d"), "bank must be"), (dict(bank="shape"), "bank of images"), (dict(bank="empty"), "empty"),
    (dict(batch=0), "batch"), (dict(backend="triton"), "backend"),
]
BAD_DIST = [(dict(stats="G"), "not this model's"), (dict(stats="U"), "not this model's"),
            (dict(stats="key"), "stats must be"), (dict(stats="nan"), "not finite"), (dict(batch=1.5), "batch"),
            (dict(backend="triton"), "backend")]


@pytest.mark.parametrize("ens", [False, True])
@pytest.mark.parametrize("kw,msg", BAD_FIT + BAD_DIST, ids=[str(i) for i in range(len(BAD_FIT + BAD_DIST))])
def test_refusals_come_before_any_forward(kw, msg, ens, monkeypatch):
    from gentun_amd.models.cnn_fitted import CnnClassifier
    fitted, x = T._ensemble("mnist")
    obj, G = (fitted, 3) if ens else (fitted.members[0], 1)
    C, D = obj.classes, 16 * G
    good = obj.gaussian_fit(_bank(40, D, C)[0], labels=_bank(40, D, C)[1], shrink=0.1)

    def no_forward(*a, **k):
        raise AssertionError("a forward ran before the refusal")
    monkeypatch.setattr(CnnClassifier, "_torch_features", no_forward)
    kw = dict(kw)
    if "stats" in kw:
        how, st = kw.pop("stats"), dict(good)
        if how == "G":
            st = {k: (np.concatenate([v, v]) if k in KEYS[1:5] else v) for k, v in st.items()}
        elif how == "U":
            st["whiten"] = st["whiten"][:, :15, :15]
        elif how == "key":
            del st["wmean"]
        else:
            st["wmean"] = np.full_like(st["wmean"], np.nan)
        with pytest.raises(ValueError, match=msg):
            obj.mahalanobis(x[:2], st, **kw)
        return
    banks = {"D15": np.zeros((8, D - 1), np.float32), "nan": np.full((8, D), np.nan, np.float32),
             "3d": np.zeros((8, 4, D), np.float32), "shape": np.zeros((8, 28, 27, 1), np.float32),
             "empty": np.zeros((0, D), np.float32)}
    labels = {"short": np.zeros(7, np.int64), "range": np.full(8, C, np.int64), "float": np.zeros(8, np.float32)}
    bank = banks[kw.pop("bank")] if "bank" in kw else x[:8]
    if "labels" in kw:
        kw["labels"] = labels[kw["labels"]]
    with pytest.raises(ValueError, match=msg):
        obj.gaussian_fit(bank, **kw)
    if "batch" in kw or "backend" in kw:
        with pytest.raises(ValueError, match=msg):
            obj.mahalanobis(x[:2], good, **kw)


def test_model_files_are_unchanged(tmp_path):
    _, clf, x = T._fit("mnist")
    sha = []
    for name in ("before.npz", "after.npz"):
        clf.save(str(tmp_path / name))
        with open(str(tmp_path / name), "rb") as f:
            sha.append(hashlib.sha256(f.read()).hexdigest())
        st = clf.gaussian_fit(x[:40], labels=np.arange(40) % clf.classes)
        clf.mahalanobis(x[:4], st)
    assert sha[0] == sha[1]
    np.savez(str(tmp_path / "stats.npz"), **st)
    back = dict(np.load(str(tmp_path / "stats.npz")))
    assert clf.mahalanobis(x[:4], back).tobytes() == clf.mahalanobis(x[:4], st).tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_gaussian.py"), "--device", "cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["bank_rows"] == 224 - out["held_out_rows"] and sum(out["class_counts"]) == out["bank_rows"]
    assert 0.0 <= out["auroc_noise_vs_held_out"] <= 1.0 and 0.0 <= out["agreement_with_predict"] <= 1.0
