"""Test-time augmentation of fitted Genetic-CNN models on the CPU (torch executor): the ``tta=`` argument of
``CnnClassifier.predict`` / ``CnnEnsemble.predict`` (gentun_amd/models/cnn_fitted.py, cnn_ensemble.py).

Every comparison is byte equality or a refusal. The contract, written out in ``_ordered_mean``: per row and
class ``acc = p_0``, ``acc = acc + p_v`` in view order, ``out = acc * (1 / V)`` with ``1 / V`` rounded first,
all in the dtype of the per-view arrays; the views are ``tests/augment_ref.transform``'s."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, BATCH = 96, 32
# name -> (input shape, classes, batch_norm)
CASES = {
    "mnist": ((28, 28, 1), 3, False),
    "mnist_bn": ((28, 28, 1), 3, True),
    "rgb": ((32, 32, 3), 4, False),
    "rgb_bn": ((32, 32, 3), 4, True),
}
GENOMES = [{"S_1": "101"}, {"S_1": "111"}, {"S_1": "011"}]
V16 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (3, -2, 0), (-27, 0, 0), (0, 27, 0),
       (0, 0, 1), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1), (-3, 2, 1), (27, 0, 1), (0, -27, 1)]
VIEWS = {1: [(0, 0, 0)], 2: {"flip": True}, 5: {"shift": 2}, 16: V16}


def _space(case):
    shape, classes, bn = CASES[case]
    return dict(nodes=(3,), input_shape=shape, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
                dropout_probability=0.5, classes=classes, nfold=3, epochs=(1,), learning_rate=(1e-2,),
                batch_size=BATCH, seed=3, backend="torch", batch_norm=bn)


def _data(shape, classes, n=N, seed=0):
    rng = np.random.default_rng(seed)
    lab = np.arange(n) % classes
    proto = rng.standard_normal((classes,) + shape).astype(np.float32)
    x = (proto[lab] + 0.5 * rng.standard_normal((n,) + shape)).astype(np.float32)
    return x, np.eye(classes, dtype=np.float32)[lab], lab


_FITS, _ENS = {}, {}


def _fit(case):
    """(model, classifier, x) of one fit per case, shared (and left unchanged) by the tests."""
    if case not in _FITS:
        from gentun_amd.models.cnn import GeneticCnnModel
        shape, classes, _ = CASES[case]
        x, y, _ = _data(shape, classes)
        m = GeneticCnnModel(x, y, GENOMES[0], device="cpu", **_space(case))
        _FITS[case] = (m, m.fit(), x)
    return _FITS[case]


def _ensemble(case):
    if case not in _ENS:
        from gentun_amd.models import fit_ensemble
        shape, classes, _ = CASES[case]
        x, y, _ = _data(shape, classes)
        _ENS[case] = (fit_ensemble(x, y, GENOMES, device="cpu", **_space(case)), x)
    return _ENS[case]


def _oracle_views(x, views):
    """``[V]`` arrays ``[n, H, W, C]``: the oracle's transform, image by image."""
    return [np.stack([R.transform(img, dy, dx, fl) for img in x]) for dy, dx, fl in views]


def _ordered_mean(per_view):
    dt = per_view[0].dtype
    acc = per_view[0]
    for p in per_view[1:]:
        acc = np.add(acc, p, dtype=dt)
    inv = dt.type(1) / dt.type(len(per_view))
    assert type(inv) is dt.type
    return np.multiply(acc, inv, dtype=dt)


# ---------------------------------------------------------------------------------------------------------
# the views
# ---------------------------------------------------------------------------------------------------------

def test_shorthand_sizes_and_order():
    from gentun_amd.models.cnn_fitted import tta_views
    s = 3
    shifts = [(0, 0), (-s, 0), (s, 0), (0, -s), (0, s)]
    assert tta_views(None, (8, 8, 3)) is None
    assert tta_views({}, (8, 8, 3)) == ((0, 0, 0),)
    assert tta_views({"shift": 0, "flip": False}, (8, 8, 3)) == ((0, 0, 0),)
    assert tta_views({"flip": True}, (8, 8, 3)) == ((0, 0, 0), (0, 0, 1))
    assert tta_views({"shift": s}, (8, 8, 3)) == tuple((dy, dx, 0) for dy, dx in shifts)
    assert tta_views({"shift": np.int64(s), "flip": np.bool_(True)}, (8, 8, 3)) == \
        tuple((dy, dx, 0) for dy, dx in shifts) + tuple((dy, dx, 1) for dy, dx in shifts)
    assert tta_views({"shift": 4, "flip": False}, (6, 5, 3)) == \
        ((0, 0, 0), (-4, 0, 0), (4, 0, 0), (0, -4, 0), (0, 4, 0))
    for tta in ({}, {"flip": True}, {"shift": 1}, {"shift": 1, "flip": True}):
        views = tta_views(tta, (8, 8, 3))
        assert len(views) in (1, 2, 5, 10) and views[0] == (0, 0, 0)
        assert all(type(v) is tuple and all(type(e) is int for e in v) for v in views)


def test_explicit_views_pass_through():
    from gentun_amd.models.cnn_fitted import tta_views
    views = [(0, 0, 0), (5, -4, 1), (-5, 4, 0), (0, 0, 1)]
    assert tta_views(views, (6, 5, 3)) == tuple(views)
    assert tta_views(tuple(views), (6, 5, 3)) == tuple(views)
    got = tta_views([(np.int32(1), np.int64(-2), True), [0, 0, np.bool_(False)], (0, 1, np.int8(1))], (6, 5, 3))
    assert got == ((1, -2, 1), (0, 0, 0), (0, 1, 1))
    assert all(type(e) is int for v in got for e in v)
    assert tta_views(V16, (28, 28, 1)) == tuple(V16) and len(set(V16)) == 16
    assert tta_views(tta_views(V16, (28, 28, 1)), (28, 28, 1)) == tuple(V16)       # its own output is a valid input


@pytest.mark.parametrize("tta", [
    {"shift": 1, "rotate": 2},                          # unknown key
    {"shift": -1}, {"shift": 5}, {"shift": 6},          # out of range: 0 <= s < min(6, 5)
    {"shift": 1.0}, {"shift": True}, {"shift": "1"},    # not an integer
    {"flip": 1}, {"flip": "yes"},                       # not a bool
    [],                                                 # no view
    [(0, 0, 0)] * 2, [(1, 0, 1), (0, 0, 1), (1, 0, True)],         # duplicates
    [(i, 0, 0) for i in range(-5, 6)] + [(i, 1, 0) for i in range(-5, 1)],     # 17 distinct views
    [(6, 0, 0)], [(-6, 0, 0)], [(0, 5, 0)], [(0, -5, 0)],           # |dy| < 6, |dx| < 5
    [(0.0, 0, 0)], [(0, 1.5, 0)], [(True, 0, 0)], [("1", 0, 0)], [(None, 0, 0)],    # non-integers
    [(0, 0, 2)], [(0, 0, -1)], [(0, 0, 0.0)], [(0, 0, None)],       # flip is a bool or 0 / 1
    [(0, 0)], [(0, 0, 0, 0)], [0, 0, 0], ["abc"],       # not triples
    "flip", 3, 1.5, True, {(0, 0, 0)}, object(),        # neither a sequence nor a dict
])
def test_refusals(tta):
    from gentun_amd.models.cnn_fitted import tta_views
    with pytest.raises(ValueError):
        tta_views(tta, (6, 5, 3))


def test_predict_refuses_before_predicting():
    m, clf, x = _fit("mnist")
    ens, _ = _ensemble("mnist")
    for bad in ({"shift": 28}, [(28, 0, 0)], [(0, 0, 0), (0, 0, 0)], {"crop": 1}):
        with pytest.raises(ValueError):
            clf.predict(x[:4], tta=bad)
        with pytest.raises(ValueError):
            clf.predict_classes(x[:4], tta=bad)
        with pytest.raises(ValueError):
            ens.predict(x[:4], tta=bad)
        with pytest.raises(ValueError):
            ens.predict_outputs(x[:4], ("votes",), tta=bad)
        with pytest.raises(ValueError):
            m.predict(x[:4], tta=bad)


@pytest.mark.parametrize("shape", [(6, 5, 3), (28, 28, 1)])
def test_numpy_twin_equals_the_oracle(shape):
    from gentun_amd.models.cnn_fitted import tta_transform
    H, W, _ = shape
    x = np.random.default_rng(H).standard_normal((3,) + shape).astype(np.float32)
    x[0, 0, 0, 0] = -0.0                                # moved, never changed: the sign of a zero too
    keep = x.copy()
    top = min(H, W) - 1
    shifts = sorted({0, 1, -1, top, -top})
    seen = 0
    for dy in shifts + [H - 1, 1 - H]:
        for dx in shifts + [W - 1, 1 - W]:
            for flip in (0, 1, False, True):
                got = tta_transform(x, dy, dx, flip)
                assert got.shape == x.shape and got.dtype == x.dtype and got.flags["C_CONTIGUOUS"]
                for i in range(len(x)):
                    assert got[i].tobytes() == R.transform(x[i], dy, dx, int(flip)).tobytes(), (dy, dx, flip, i)
                seen += 1
    assert seen == 7 * 7 * 4 and x.tobytes() == keep.tobytes()           # the input is left alone
    assert tta_transform(x, 0, 0, 0).tobytes() == x.tobytes()
    x64 = x.astype(np.float64)
    assert tta_transform(x64, 1, -1, 1).dtype == np.float64
    assert tta_transform(x64, 1, -1, 1).astype(np.float32).tobytes() == tta_transform(x, 1, -1, 1).tobytes()


# ---------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2, 5, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_predict_is_the_ordered_mean_over_the_views(case, V):
    from gentun_amd.models.cnn_fitted import tta_views
    m, clf, x = _fit(case)
    xs = x[:40]
    views = tta_views(VIEWS[V], clf.input_shape)
    assert len(views) == V
    tx = _oracle_views(xs, views)
    for output in ("proba", "logits"):
        want = _ordered_mean([clf.predict(t, output=output) for t in tx])
        got = clf.predict(xs, output=output, tta=VIEWS[V])
        assert got.dtype == np.float32 and got.shape == (40, clf.classes)
        assert got.tobytes() == want.tobytes(), (output, float(np.abs(got - want).max()))
        if output == "proba":
            label = clf.predict(xs, output="label", tta=VIEWS[V])
            assert label.dtype == np.int64 and np.array_equal(label, np.argmax(want, 1))
            assert np.array_equal(clf.predict_classes(xs, tta=VIEWS[V]), label)
        if V > 1:                                       # the views are not copies of the image
            assert got.tobytes() != clf.predict(xs, output=output).tobytes()


@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_the_identity_view_is_no_tta(case):
    m, clf, x = _fit(case)
    for output in ("proba", "logits", "label"):
        plain = clf.predict(x, output=output)
        for tta in ([(0, 0, 0)], ((0, 0, False),), {}, {"shift": 0, "flip": False}):
            assert clf.predict(x, output=output, tta=tta).tobytes() == plain.tobytes()
        assert clf.predict(x, output=output, tta=None).tobytes() == plain.tobytes()


@pytest.mark.parametrize("case", ["mnist_bn", "rgb"])
def test_batch_and_row_order_do_not_change_a_row(case):
    m, clf, x = _fit(case)
    tta = {"shift": 2, "flip": True}
    for output in ("proba", "logits"):
        a = clf.predict(x, output=output, tta=tta, batch=256)
        assert clf.predict(x, output=output, tta=tta, batch=32).tobytes() == a.tobytes()
        assert clf.predict(x[::-1], output=output, tta=tta, batch=32)[::-1].tobytes() == a.tobytes()
        assert clf.predict(x[7], output=output, tta=tta).tobytes() == a[7:8].tobytes()
        assert clf.predict(x[:33], output=output, tta=tta, batch=32).tobytes() == a[:33].tobytes()


def test_fp64_stays_fp64():
    m, clf, x = _fit("mnist_bn")
    xs = x[:40]
    views = VIEWS[16]
    tx = _oracle_views(xs, views)
    for output in ("proba", "logits"):
        per = [clf.predict(t, output=output, dtype=torch.float64) for t in tx]
        assert per[0].dtype == np.float64
        got = clf.predict(xs, output=output, tta=views, dtype=torch.float64)
        assert got.dtype == np.float64 and got.tobytes() == _ordered_mean(per).tobytes()
        # not the fp32 result widened: the forward itself ran in fp64
        assert not np.array_equal(got, clf.predict(xs, output=output, tta=views).astype(np.float64))


def test_model_forwards_the_argument():
    m, clf, x = _fit("rgb")
    tta = {"flip": True}
    assert m.predict(x[:40], tta=tta).tobytes() == clf.predict(x[:40], tta=tta).tobytes()
    assert m.predict(x[:40], output="logits", tta=tta).tobytes() != m.predict(x[:40], output="logits").tobytes()


# ---------------------------------------------------------------------------------------------------------
# the ensemble
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, [3.0, 1.0, 4.0]])
@pytest.mark.parametrize("k", [1, 3])
def test_ensemble_is_the_combine_of_its_members_tta(k, weights):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_ensemble import combine, vote_label
    fitted, x = _ensemble("rgb_bn")
    ens = CnnEnsemble(fitted.members[:k], weights=None if weights is None else weights[:k])
    xs = x[:40]
    for tta in ({"shift": 2}, V16[7:10]):
        out = ens.predict_outputs(xs, tta=tta)
        for g, member in enumerate(ens.members):
            assert out["member_proba"][g].tobytes() == member.predict(xs, tta=tta).tobytes()
            assert out["member_logits"][g].tobytes() == member.predict(xs, output="logits", tta=tta).tobytes()
        proba, votes = combine(out["member_proba"], ens.weights)
        assert out["proba"].dtype == np.float32 and out["proba"].tobytes() == proba.tobytes()
        assert out["votes"].dtype == np.int32 and out["votes"].tobytes() == votes.tobytes()
        assert np.array_equal(out["label"], np.argmax(proba, 1))
        assert np.array_equal(out["vote_label"], vote_label(votes, proba))
        assert (votes.sum(1) == k).all()
        for name in ("proba", "votes", "label", "vote_label", "member_logits"):
            assert ens.predict(xs, output=name, tta=tta).tobytes() == out[name].tobytes()
        assert np.array_equal(ens.predict_classes(xs, tta=tta), out["label"])
        assert out["member_logits"].tobytes() != ens.predict(xs, output="member_logits").tobytes()
    plain = ens.predict_outputs(xs)
    same = ens.predict_outputs(xs, tta=[(0, 0, 0)])
    assert all(same[name].tobytes() == plain[name].tobytes() for name in plain)


# ---------------------------------------------------------------------------------------------------------
# around it
# ---------------------------------------------------------------------------------------------------------

def _sha(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_save_and_load_never_record_tta(tmp_path):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, clf, x = _fit("mnist")
    ens, _ = _ensemble("mnist")
    tta = {"shift": 1, "flip": True}
    before, after = str(tmp_path / "before.npz"), str(tmp_path / "after.npz")
    for obj, load in ((clf, CnnClassifier.load), (ens, CnnEnsemble.load)):
        header = json.dumps(obj.header())
        obj.save(before)
        want = obj.predict(x[:40], tta=tta)
        obj.save(after)
        assert _sha(before) == _sha(after) and json.dumps(obj.header()) == header and "tta" not in header
        with np.load(after, allow_pickle=False) as z:
            assert "tta" not in str(z["header"][()]) and not [f for f in z.files if "tta" in f]
        back = load(after)
        assert back.predict(x[:40], tta=tta).tobytes() == want.tobytes()
        assert back.predict(x[:40]).tobytes() == obj.predict(x[:40]).tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_tta.py"), "--device", "cpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"held_out_rows", "views", "accuracy", "accuracy_tta"} and out["views"] == 10
    assert 0.0 <= out["accuracy"] <= 1.0 and 0.0 <= out["accuracy_tta"] <= 1.0
