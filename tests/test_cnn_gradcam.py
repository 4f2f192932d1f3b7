"""Grad-CAM of fitted Genetic-CNN models on the CPU (torch executor): ``cam_shape``, ``cam_upsample`` and the
``gradcam`` method of ``CnnClassifier`` / ``CnnEnsemble`` / ``GeneticCnnModel`` (gentun_amd/models/cnn_fitted.py,
cnn_ensemble.py, cnn.py), against the fp64 oracle of tests/gradcam_ref.py, which differentiates through both dense
layers without the collapse the HIP kernels rest on; the oracle itself against central finite differences; the
fp32 twin of the kernels against the oracle within an a-priori rounding bound. The fits are those of
tests/test_cnn_tta.py (shared inside one pytest process, left unchanged)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradcam_ref as R
import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS = 6
_FEATS = {}


def _features(clf, x, dtype=torch.float32):
    """The last feature map ``A [n, C, hr, wr]`` of ``x`` by the classifier's own stock-torch forward in ``dtype``,
    rows padded to a multiple of 32 as ``predict`` pads them; computed once per (classifier, rows, dtype)."""
    key = (id(clf), len(x), dtype)
    if key not in _FEATS:
        buf = np.zeros(((len(x) + 31) // 32 * 32,) + tuple(np.transpose(x, (0, 3, 1, 2)).shape[1:]), np.float32)
        buf[:len(x)] = x.transpose(0, 3, 1, 2)
        with torch.no_grad():
            A = clf._torch_features(torch.from_numpy(buf).to(dtype), clf._tensors(torch.device("cpu"), dtype))
        _FEATS[key] = A[:len(x)].numpy().copy()
    return _FEATS[key]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------
# the oracle; the shape; the upsampling
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("score", ["logit", "proba"])
@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_oracle_gradient_against_central_differences(case, score):
    """The directional derivative of the fp64 score along random unit directions of ``A``: the oracle's
    ``<dS/dA, d>`` against ``(S(A + e d) - S(A - e d)) / 2e`` with e = 1e-6 (the score is piecewise smooth; the
    rounding of the difference is about 1e-16 / e = 1e-10 of a score of order one)."""
    m, clf, x = T._fit(case)
    A = _features(clf, x[:NROWS]).astype(np.float64)
    rng = np.random.default_rng(7)
    t = rng.integers(0, clf.classes, NROWS)
    _, dA = R.oracle(clf.params, A, t, score)
    eps, worst = 1e-6, 0.0
    for k in range(4):
        d = rng.standard_normal(A.shape)
        d /= np.sqrt((d ** 2).sum((1, 2, 3), keepdims=True))
        fd = (R.score64(clf.params, A + eps * d, t, score) - R.score64(clf.params, A - eps * d, t, score)) / (2 * eps)
        an = (dA * d).sum((1, 2, 3))
        worst = max(worst, float(np.abs(fd - an).max() / np.abs(an).max()))
    print("[cnn-gradcam] oracle vs central differences ({}, {}): {:.3e}".format(case, score, worst))
    assert np.abs(dA).max() > 0 and worst <= 1e-6


def test_cam_shape():
    from gentun_amd.models.cnn_fitted import cam_shape
    from gentun_amd.models.genome import make_plan

    def plan(shape, stages):
        genes = {"S_1": "101", "S_2": "1010010001"} if stages == 2 else {"S_1": "101"}
        return make_plan(genes, (3, 5)[:stages], shape, (4, 8)[:stages], ((3, 3), (3, 3))[:stages], 16, 3)
    want = {((32, 32, 3), 1): (16, 16), ((32, 32, 3), 2): (8, 8), ((28, 28, 1), 1): (14, 14), ((28, 28, 1), 2): (7, 7),
            ((6, 5, 3), 1): (3, 2), ((6, 5, 3), 2): (1, 1)}
    for (shape, stages), hw in want.items():
        got = cam_shape(plan(shape, stages), shape)
        assert got == hw and all(type(v) is int for v in got), (shape, stages)
    with pytest.raises(ValueError):
        cam_shape(plan((6, 5, 3), 2), (3, 3, 3))
    for case in ("mnist", "rgb"):                        # and what the forward really leaves
        m, clf, x = T._fit(case)
        assert _features(clf, x[:NROWS]).shape[2:] == cam_shape(clf.plan, clf.input_shape)
        assert clf.gradcam(x[:2]).shape == (2,) + cam_shape(clf.plan, clf.input_shape)


def test_upsample_is_torchs_bilinear_rule():
    import torch.nn.functional as F
    from gentun_amd.models.cnn_fitted import cam_upsample
    rng = np.random.default_rng(0)
    for (hr, wr), (H, W) in (((8, 8), (32, 32)), ((7, 7), (28, 28)), ((3, 2), (6, 5)), ((1, 1), (6, 5)),
                             ((14, 14), (28, 28)), ((5, 7), (4, 3)), ((2, 3), (2, 9))):
        maps = rng.standard_normal((3, hr, wr)).astype(np.float32)
        got = cam_upsample(maps, (H, W))
        want = F.interpolate(torch.from_numpy(maps)[:, None], size=(H, W), mode="bilinear", align_corners=False)
        assert got.dtype == np.float32 and got.shape == (3, H, W)
        assert np.abs(got - want[:, 0].numpy()).max() <= 1e-6, ((hr, wr), (H, W))
    maps = rng.standard_normal((2, 7, 5)).astype(np.float32)
    maps[0, 0, 0] = -0.0
    assert cam_upsample(maps, (7, 5)).tobytes() == maps.tobytes()        # the identity when the sizes match
    for bad in (dict(maps=maps[0], size=(7, 5)), dict(maps=maps, size=(0, 5)), dict(maps=maps, size=(7, -1))):
        with pytest.raises(ValueError):
            cam_upsample(**bad)


# ---------------------------------------------------------------------------------------------------------
# the fp32 twin of the kernels
# ---------------------------------------------------------------------------------------------------------

def _kernel_buffers(clf, A, pad=1):
    """The classifier's head in the HIP executor's layouts, as fp32 numpy: ``W1 [1, hs * ws * Cp, Up]`` over
    NHWC features with ``pad`` padded pixel rows / columns holding NaN (never to be read), channels padded to a
    multiple of 8 and units to a multiple of 64 with zeros, ``W2 [1, Up, C]``; the feature map
    ``[1, n, hs, ws, Cp]``, the hidden activations ``[1, n, Up]`` and the logits / probabilities ``[1, n, C]`` by
    fp32 numpy."""
    n, C, hr, wr = A.shape
    U = clf.dense_units
    hs, ws, Cp, Up = hr + pad, wr + pad, (C + 7) // 8 * 8, (U + 63) // 64 * 64
    W1 = np.full((hs, ws, Cp, Up), np.nan, np.float32)
    W1[:hr, :wr] = 0.0
    W1[:hr, :wr, :C, :U] = clf.params["dense1.w"].reshape(C, hr, wr, U).transpose(1, 2, 0, 3)
    W2 = np.zeros((Up, clf.classes), np.float32)
    W2[:U] = clf.params["dense2.w"]
    feat = np.zeros((n, hs, ws, Cp), np.float32)
    feat[:, :hr, :wr, :C] = A.transpose(0, 2, 3, 1)
    z = (A.reshape(n, -1) @ clf.params["dense1.w"] + clf.params["dense1.b"]).astype(np.float32)
    hid = np.zeros((n, Up), np.float32)
    hid[:, :U] = np.maximum(z, np.float32(0))
    logits = (hid[:, :U] @ clf.params["dense2.w"] + clf.params["dense2.b"]).astype(np.float32)
    e = np.exp(logits - logits.max(1, keepdims=True))
    proba = (e / e.sum(1, keepdims=True)).astype(np.float32)
    return dict(W1=W1.reshape(1, hs * ws * Cp, Up), W2=W2[None], feat=feat[None], hid=hid[None],
                logits=logits[None], proba=proba[None], geom=(hs, ws, hr, wr, Cp, C))


@pytest.mark.parametrize("score", ["logit", "proba"])
@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_twin_against_the_oracle_within_the_rounding_bound(case, score):
    m, clf, x = T._fit(case)
    A = _features(clf, x[:NROWS])
    b = _kernel_buffers(clf, A)
    hs, ws, hr, wr, Cp, Cr = b["geom"]
    wbar = R.w1sum_twin(b["W1"], hs, ws, hr, wr, Cp, Cr)
    assert np.isfinite(wbar).all() and not wbar[:, Cr:].any()            # the NaN rows of padded pixels: not read
    one = np.ones(1, np.float32)
    for tgt in (np.full(NROWS, -1), np.arange(NROWS) % clf.classes):
        got, t, base = R.head_twin(b["logits"], b["proba"], one, b["feat"], b["hid"], b["W2"], wbar, tgt, hr, wr,
                                   Cr, score == "logit", False)
        assert got.dtype == np.float32 and got.shape == (NROWS, hr, wr)
        assert np.array_equal(t, np.where(tgt < 0, b["proba"][0].argmax(1), tgt))
        assert base.tobytes() == (b["logits"] if score == "logit" else b["proba"])[0][np.arange(NROWS), t].tobytes()
        U = clf.dense_units
        h64, p64 = b["hid"][0, :, :U].astype(np.float64), b["proba"][0].astype(np.float64)
        want, _ = R.oracle(clf.params, A, t, score, h=h64, proba=p64)
        bound = R.rounding_bound(clf.params, A, h64, p64, t, score)
        err = np.abs(got - want)
        print("[cnn-gradcam] twin vs oracle ({}, {}): largest error {:.3e}, of its bound {:.3f}, of the map {:.3e}"
              .format(case, score, float(err.max()), float((err[bound > 0] / bound[bound > 0]).max()),
                      _rel(got, want)))
        assert np.abs(want).max() > 0 and bound.max() > 0
        assert (err <= bound).all()                      # where every term is zero (a dead pixel) both are exact
        relu = R.head_twin(b["logits"], b["proba"], one, b["feat"], b["hid"], b["W2"], wbar, tgt, hr, wr, Cr,
                           score == "logit", True)[0]
        assert relu.tobytes() == np.where(got > 0, got, np.float32(0)).tobytes()


# ---------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("score", ["logit", "proba"])
@pytest.mark.parametrize("case", list(T.CASES))
def test_torch_backend_against_the_oracle(case, score):
    """``max |diff| / max |oracle map| <= 1e-5``: stock-torch fp32 autograd measured 2.5e-7 to 1.1e-6 against an
    fp64 autograd Grad-CAM on these fits; the bound is roughly ten times that."""
    m, clf, x = T._fit(case)
    xs = x[:NROWS]
    A = _features(clf, xs)
    label = clf.predict(xs, output="label")
    other = (label + 1 + np.arange(NROWS) % (clf.classes - 1)) % clf.classes
    assert np.array_equal(R.head64(clf.params, A)[3].argmax(1), label)
    for target, t in ((None, label), (1, np.full(NROWS, 1)), (other, other), (list(other), other)):
        want, _ = R.oracle(clf.params, A, t, score)
        assert np.abs(want).max() > 0                    # the oracle map is not all zero
        got, info = clf.gradcam(xs, target=target, score=score, relu=False, return_info=True)
        assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
        err = _rel(got, want)
        print("[cnn-gradcam] torch backend vs oracle ({}, {}, {}): {:.3e}".format(
            case, score, "label" if target is None else "given", err))
        assert err <= 1e-5
        assert set(info) == {"target", "base"} and info["target"].dtype == np.int64 and info["base"].dtype == np.float32
        assert np.array_equal(info["target"], t)
        # the fp64 path of the same code (the GPU tests' reference) on its own fp64 feature map
        g64 = clf._torch_gradcam(xs, t, score, False, torch.device("cpu"), 256, torch.float64)[0]
        assert g64.dtype == np.float64
        assert _rel(g64, R.oracle(clf.params, _features(clf, xs, torch.float64), t, score)[0]) <= 1e-9
    one = clf.gradcam(xs[2], score=score)                # one [H, W, C] image
    assert one.tobytes() == clf.gradcam(xs[2:3], score=score).tobytes()


@pytest.mark.parametrize("case", ["mnist", "mnist_bn"])      # fits whose raw maps hold both signs at both scores
def test_relu_is_the_maximum_with_zero(case):
    m, clf, x = T._fit(case)
    t = np.arange(NROWS) % clf.classes
    for score in ("logit", "proba"):
        raw = clf.gradcam(x[:NROWS], target=t, score=score, relu=False)
        assert (raw < 0).any() and (raw > 0).any()
        want = np.maximum(raw, np.float32(0)).tobytes()
        assert clf.gradcam(x[:NROWS], target=t, score=score, relu=True).tobytes() == want
        assert clf.gradcam(x[:NROWS], target=t, score=score).tobytes() == want


@pytest.mark.parametrize("case", ["mnist", "rgb_bn"])
def test_info_agrees_with_predict(case):
    m, clf, x = T._fit(case)
    xs = x[:40]
    label = clf.predict(xs, output="label")
    for score, output in (("logit", "logits"), ("proba", "proba")):
        plain = clf.predict(xs, output=output)
        _, info = clf.gradcam(xs, score=score, return_info=True)
        assert np.array_equal(info["target"], label)
        assert info["base"].tobytes() == plain[np.arange(40), label].tobytes()
        _, info = clf.gradcam(xs, target=2, score=score, return_info=True)
        assert (info["target"] == 2).all() and info["base"].tobytes() == plain[:, 2].copy().tobytes()


@pytest.mark.parametrize("case", ["mnist_bn", "rgb"])
def test_batch_32_and_256_give_equal_bits(case):
    """96 rows: one chunk at batch 256, three at batch 32 (the project's CPU chunking tests stay at 96 rows or
    fewer: stock torch's CPU forward keeps a row's bits up to 128 rows per forward)."""
    m, clf, x = T._fit(case)
    assert len(x) == 96
    for score in ("logit", "proba"):
        a, ia = clf.gradcam(x, score=score, batch=256, return_info=True)
        b, ib = clf.gradcam(x, score=score, batch=32, return_info=True)
        assert a.tobytes() == b.tobytes() and ia["base"].tobytes() == ib["base"].tobytes()
        assert np.array_equal(ia["target"], ib["target"])
        assert clf.gradcam(x[:5], score=score, batch=64).tobytes() == a[:5].tobytes()


def test_defaults_and_upsample():
    from gentun_amd.models.cnn_fitted import cam_upsample
    m, clf, x = T._fit("rgb")
    got = clf.gradcam(x[:3])
    assert got.shape == (3, 16, 16)
    assert got.tobytes() == clf.gradcam(x[:3], None, "logit", True, False, "cpu", 256, "torch", False).tobytes()
    up, info = clf.gradcam(x[:3], upsample=True, return_info=True)
    assert up.shape == (3, 32, 32) and up.tobytes() == cam_upsample(got, (32, 32)).tobytes()
    assert set(info) == {"target", "base"}


def test_refusals():
    m, clf, x = T._fit("mnist")
    ens, _ = T._ensemble("mnist")
    calls = []
    for obj in (clf, ens, m):
        for kw in (dict(score="logits"), dict(score="label"), dict(score=None), dict(score=0),
                   dict(relu=1), dict(relu=None), dict(relu="yes"), dict(upsample=1), dict(upsample=None),
                   dict(upsample=(28, 28)), dict(target=3), dict(target=-1), dict(target=[0, 1]),
                   dict(target=[0, 1, 2, 3, 3]), dict(target=1.0), dict(target=[[0, 1, 2, 0]]), dict(target=True),
                   dict(batch=0), dict(batch=-32), dict(batch=1.5), dict(backend="numpy")):
            with pytest.raises(ValueError):
                obj.gradcam(x[:4], **kw)
            calls.append(kw)
    with pytest.raises(ValueError):
        clf.gradcam(x[:4, :27])
    # a bad option is refused before any work: no forward runs
    seen = []
    keep = clf._torch_features
    clf._torch_features = lambda *a, **k: seen.append(1) or keep(*a, **k)
    try:
        for kw in (dict(score="x"), dict(relu=0), dict(upsample="no"), dict(target=9), dict(batch=0)):
            with pytest.raises(ValueError):
                clf.gradcam(x[:4], **kw)
        assert not seen
        clf.gradcam(x[:4])
        assert seen
    finally:
        del clf._torch_features
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes, _ = T.CASES["mnist"]
    fresh = GeneticCnnModel(x, np.eye(classes, dtype=np.float32)[np.arange(len(x)) % classes], T.GENOMES[0],
                            device="cpu", **T._space("mnist"))
    with pytest.raises(RuntimeError):
        fresh.gradcam(x[:4])


def test_hip_path_refuses_more_than_1024_pixels_before_a_predictor_is_built():
    """66 x 64 with one stage leaves 33 x 32 = 1056 pixels: the HIP path refuses from ``cam_shape`` alone -- no
    predictor is asked for (there is no GPU here to build one on) -- and the torch backend takes it."""
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_fitted import CnnClassifier
    rng = np.random.default_rng(0)
    shape = (66, 64, 1)
    members = []
    for genes in ({"S_1": "101"}, {"S_1": "111"}):
        kw = dict(genes=genes, nodes=(3,), input_shape=shape, kernels_per_layer=(2,), kernel_sizes=((3, 3),),
                  dense_units=4, classes=3)
        params = {n: (0.1 * rng.standard_normal(s)).astype(np.float32) for n, s in _shapes(kw)}
        members.append(CnnClassifier(params=params, **kw))
    x = rng.standard_normal((2,) + shape).astype(np.float32)
    for obj in (members[0], CnnEnsemble(members)):
        asked = []
        obj.hip_predictor = lambda *a, **k: asked.append(1)
        with pytest.raises(ValueError, match="1024"):
            obj.gradcam(x, backend="hip")
        with pytest.raises(ValueError, match="1024"):
            obj.gradcam(x, device="cuda:0")
        assert not asked
        assert obj.gradcam(x).shape == (2, 33, 32)


def _shapes(kw):
    """``param_shapes`` of the architecture ``kw`` without a classifier: through the plan."""
    from gentun_amd.models.genome import make_plan
    p = make_plan(kw["genes"], kw["nodes"], kw["input_shape"], kw["kernels_per_layer"], kw["kernel_sizes"],
                  kw["dense_units"], kw["classes"])
    out = []
    for st in p.convs():
        out += [(st.name + ".w", (st.cout, st.cin, st.k[0], st.k[1])), (st.name + ".b", (st.cout,))]
    return out + [("dense1.w", (p.flatten, p.dense_units)), ("dense1.b", (p.dense_units,)),
                  ("dense2.w", (p.dense_units, p.classes)), ("dense2.b", (p.classes,))]


# ---------------------------------------------------------------------------------------------------------
# the ensemble
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, [3.0, 1.0, 4.0]])
@pytest.mark.parametrize("k", [1, 3])
def test_ensemble_is_the_ordered_combine_of_its_members_maps(k, weights):
    from gentun_amd.models import CnnEnsemble
    fitted, x = T._ensemble("rgb_bn")
    ens = CnnEnsemble(fitted.members[:k], weights=None if weights is None else weights[:k])
    xs = x[:NROWS]
    label = ens.predict(xs, output="label")
    other = (label + 1) % ens.classes
    for score, output in (("logit", "logits"), ("proba", "proba")):
        for relu in (True, False):
            for target, t in ((None, label), (2, np.full(NROWS, 2)), (other, other)):
                per = [mem.gradcam(xs, target=t, score=score, relu=relu, return_info=True) for mem in ens.members]
                want = R.ordered_mean(ens.weights, np.stack([p[0] for p in per]))
                base = R.ordered_mean(ens.weights, np.stack([p[1]["base"] for p in per]))
                got, info = ens.gradcam(xs, target=target, score=score, relu=relu, return_info=True)
                assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (score, relu, target)
                assert np.array_equal(info["target"], t) and info["base"].tobytes() == base.tobytes()
        member = np.stack([mem.predict(xs, output=output) for mem in ens.members])
        _, info = ens.gradcam(xs, score=score, return_info=True)
        assert info["base"].tobytes() == R.ordered_mean(ens.weights, member)[np.arange(NROWS), label].tobytes()
    assert ens.gradcam(xs, score="proba", return_info=True)[1]["base"].tobytes() == \
        ens.predict(xs)[np.arange(NROWS), label].tobytes()
    if k == 1:                                           # one member of weight 1.0 is its classifier
        assert ens.gradcam(xs).tobytes() == ens.members[0].gradcam(xs).tobytes()
    else:                                                # relu=False, proba: the Grad-CAM of the combined probability
        A = [_features(mem, xs) for mem in ens.members]
        want = sum(float(w) * R.oracle(mem.params, a, label, "proba")[0] for w, mem, a in zip(ens.weights, ens.members, A))
        assert _rel(ens.gradcam(xs, score="proba", relu=False), want) <= 1e-5
    a = ens.gradcam(x, batch=256)
    assert ens.gradcam(x, batch=32).tobytes() == a.tobytes()              # 96 rows: see the classifier's test


# ---------------------------------------------------------------------------------------------------------
# around it
# ---------------------------------------------------------------------------------------------------------

def test_model_forwards_the_arguments():
    m, clf, x = T._fit("rgb")
    kw = dict(target=1, score="proba", relu=False, upsample=True)
    got, info = m.gradcam(x[:4], return_info=True, **kw)
    want, winfo = clf.gradcam(x[:4], return_info=True, **kw)
    assert got.shape == (4, 32, 32) and got.tobytes() == want.tobytes()
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
        occ = obj.occlusion(x[:4], patch=7)
        want = obj.gradcam(x[:4], score="proba")
        obj.save(after)
        assert T._sha(before) == T._sha(after) and json.dumps(obj.header()) == header and "cam" not in header
        back = load(after)
        assert back.gradcam(x[:4], score="proba").tobytes() == want.tobytes()
        assert back.predict(x[:40]).tobytes() == plain.tobytes() == obj.predict(x[:40]).tobytes()
        assert obj.occlusion(x[:4], patch=7).tobytes() == occ.tobytes()


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_gradcam.py"), "--device", "cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"images", "map", "score", "upsample", "largest"} and out["map"] == [4, 4]
    assert out["largest"] > 0 and r.stdout.count("\n") > 4 * out["images"]          # the text heat maps came first
