"""Grad-CAM of fitted Genetic-CNN models on an MI355X: ``gt_cam_w1sum`` and ``gt_head_gradcam``
(csrc/hip/cnn_dense.hip) alone against their fp32 numpy twins (tests/gradcam_ref.py) on synthetic buffers, then
``gradcam(device=cuda)`` of ``CnnClassifier`` and ``CnnEnsemble`` through the HIP predictors against the twin fed
the predictor's own device buffers after a plain forward of the same chunk, and against the members' own
predictors combined in order.

Every comparison but the last test's is byte equality or a refusal. The fits are those of
tests/test_cnn_fitted_gpu.py and tests/test_cnn_ensemble_gpu.py (320 rows, 1 epoch, batch 32; shared with them
inside one pytest process, left unchanged) plus the 16-member ensemble of tests/test_cnn_occlusion_gpu.py."""

import numpy as np
import pytest
import torch

import gradcam_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F

pytestmark = pytest.mark.gpu

GUARD = 512                  # elements past an output: all stay NaN


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _f32(t):
    return t.float().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# gt_cam_w1sum alone
# ---------------------------------------------------------------------------------------------------------

def _w1sum(w1, wbar, G, geom, over=()):
    from gentun_amd.ops import cnn_kernels as K
    a = K.CamW1SumArgs()
    a.w1, a.wbar, a.G = w1.data_ptr(), wbar.data_ptr(), G
    a.hs, a.ws, a.hr, a.wr, a.Cp, a.Cr, a.Up = geom
    for k, v in dict(over).items():
        setattr(a, k, v)
    rc = K.lib().gt_cam_w1sum(a, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("geom", [(8, 8, 7, 7, 8, 4, 64), (4, 4, 4, 4, 16, 16, 128)], ids=["padded", "full"])
def test_w1sum_kernel_equals_the_twin(geom, G):
    hs, ws, hr, wr, Cp, Cr, Up = geom
    rng = np.random.default_rng(G + hs)
    W1 = rng.standard_normal((G, hs, ws, Cp, Up)).astype(np.float32)
    W1[:, hr:] = np.nan                                  # rows of padded pixels: never read
    W1[:, :, wr:] = np.nan
    W1[:, :, :, Cr:] = np.nan                            # nor channels past the real ones
    W1 = W1.reshape(G, hs * ws * Cp, Up)
    n = G * Cp * Up
    out = torch.full((n + GUARD,), float("nan"), device=_dev())
    assert _w1sum(torch.from_numpy(W1).to(_dev()), out, G, geom) == 0
    want = R.w1sum_twin(W1, hs, ws, hr, wr, Cp, Cr)
    assert np.isfinite(want).all() and want[:, :Cr].any() and not want[:, Cr:].any()
    got = out.cpu().numpy()
    assert got[:n].tobytes() == want.tobytes()
    assert np.isnan(got[n:]).all()                       # the guard tail


def test_w1sum_refusals():
    from gentun_amd.ops import cnn_kernels as K
    geom = (8, 8, 7, 7, 8, 4, 64)
    w1 = torch.ones(3 * 8 * 8 * 8 * 64, device=_dev())
    out = torch.full((3 * 8 * 64 + GUARD,), float("nan"), device=_dev())
    for kw in (dict(w1=0), dict(wbar=0), dict(G=0), dict(G=65), dict(Up=24), dict(Up=0), dict(Up=4112), dict(Cp=12),
               dict(Cp=0), dict(Cp=264), dict(Cr=0), dict(Cr=9), dict(hr=9), dict(wr=9), dict(hr=0), dict(wr=-1),
               dict(hs=40, ws=40, hr=33, wr=32)):
        assert _w1sum(w1, out, 3, geom, over=kw) != 0, kw
        assert torch.isnan(out).all(), kw
    assert K.lib().gt_cam_w1sum(None, _stream()) != 0
    assert _w1sum(w1, out, 3, geom) == 0 and (out[:3 * 8 * 64].view(3, 8, 64)[:, :4] == 49.0).all()


# ---------------------------------------------------------------------------------------------------------
# gt_head_gradcam alone
# ---------------------------------------------------------------------------------------------------------

HB = 64                      # launch rows


class _Cam(object):
    """Synthetic buffers of one launch: random partial logits (row 0 of every member: the two last classes tie
    at the top), features and hidden activations in ``dtype`` (the hidden ones half zeros, with ``+0.0``,
    ``-0.0`` and the smallest positive value of the type in units 0, 1, 2 of every row), random ``W2`` and
    ``wbar``, NaN in the features' padded pixels and channels, NaN-filled outputs."""

    def __init__(self, G, nt, C, geom, dtype, seed):
        self.G, self.Up, self.geom, self.dtype = G, nt * 16, geom, dtype
        hs, ws, hr, wr, Cp, Cr = geom
        rng = np.random.default_rng(seed)
        feat = rng.standard_normal((G, HB, hs, ws, Cp)).astype(np.float32)
        feat[:, :, hr:] = np.nan
        feat[:, :, :, wr:] = np.nan
        feat[..., Cr:] = np.nan
        hid = np.maximum(rng.standard_normal((G, HB, self.Up)), 0).astype(np.float32)
        self.feat = torch.from_numpy(feat).to(device=_dev(), dtype=dtype)
        self.hid = torch.from_numpy(hid).to(device=_dev(), dtype=dtype)
        tiny = torch.tensor([1], dtype=torch.int32 if dtype == torch.float32 else torch.int16).view(dtype)
        self.hid[:, :, 0], self.hid[:, :, 1], self.hid[:, :, 2] = 0.0, -0.0, tiny.to(_dev())[0]
        self.wbar = torch.from_numpy(rng.standard_normal((G, Cp, self.Up)).astype(np.float32)).to(_dev())
        self.classes(C, seed + 1)

    def classes(self, C, seed):
        """The buffers that depend on the class count: partial logits, ``b2`` and ``W2``; the features, hidden
        activations and ``wbar`` stay, so one object serves every class count of its geometry and type."""
        G, nt = self.G, self.Up // 16
        self.C = C
        rng = np.random.default_rng(seed)
        plog = rng.standard_normal((G, nt, HB, C)).astype(np.float32)
        b2 = rng.standard_normal((G, C)).astype(np.float32)
        if C >= 2:
            plog[:, :, 0, :] = 0.0
            plog[:, 0, 0, C - 2:] = 7.0
            b2[:, C - 1] = b2[:, C - 2]
        self.plog, self.b2 = torch.from_numpy(plog).to(_dev()), torch.from_numpy(b2).to(_dev())
        self.logits, self.proba = F._head_predict(self.plog, self.b2)    # [G][B][C]: every launch row
        self.W2 = torch.from_numpy(rng.standard_normal((G, self.Up, C)).astype(np.float32)).to(_dev())
        self.host = tuple(_f32(t) for t in (self.feat, self.hid, self.W2, self.wbar))     # what the twin reads
        self.fresh()
        return self

    def fresh(self, tgt=None):
        hs, ws, hr, wr, Cp, Cr = self.geom
        self.tgt = torch.full((HB,), -7, dtype=torch.int32, device=_dev())
        if tgt is not None:
            self.tgt[:len(tgt)] = torch.from_numpy(np.asarray(tgt, np.int32)).to(_dev())
        self.base = torch.full((HB,), float("nan"), device=_dev())
        self.map = torch.full((HB * hr * wr + GUARD,), float("nan"), device=_dev())

    def launch(self, w, m, logit, relu, over=()):
        from gentun_amd.ops import cnn_kernels as K
        hs, ws, hr, wr, Cp, Cr = self.geom
        a = K.HeadGradcamArgs()
        a.plog, a.b2, a.weight = self.plog.data_ptr(), self.b2.data_ptr(), w.data_ptr()
        a.feat, a.hid, a.w2, a.wbar = self.feat.data_ptr(), self.hid.data_ptr(), self.W2.data_ptr(), self.wbar.data_ptr()
        a.tgt, a.base, a.map = self.tgt.data_ptr(), self.base.data_ptr(), self.map.data_ptr()
        a.G, a.B, a.Up, a.C, a.m = self.G, HB, self.Up, self.C, m
        a.hs, a.ws, a.hr, a.wr, a.Cp, a.Cr = hs, ws, hr, wr, Cp, Cr
        a.prec, a.logit, a.relu = 1 if self.dtype == torch.float32 else 0, int(logit), int(relu)
        a.inv_n = float(np.float32(1) / np.float32(hr * wr))
        for k, v in dict(over).items():
            setattr(a, k, v)
        rc = K.lib().gt_head_gradcam(a, _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool(torch.isnan(self.base).all() and torch.isnan(self.map).all() and (self.tgt == -7).all())

    def check(self, w, m, logit, relu, tgt):
        hs, ws, hr, wr, Cp, Cr = self.geom
        self.fresh(tgt)
        assert self.launch(torch.from_numpy(w).to(_dev()), m, logit, relu) == 0
        feat, hid, W2, wbar = self.host
        want, t, base = R.head_twin(self.logits[:, :m], self.proba[:, :m], w, feat[:, :m], hid[:, :m], W2, wbar, tgt,
                                    hr, wr, Cr, logit, relu)
        # one class: its probability is 1 whatever the features, and the probability's map is exactly zero
        assert np.isfinite(want).all() and (np.abs(want).max() > 0) == (self.C > 1 or bool(logit))
        key = (self.G, self.C, self.Up, self.geom, m, logit, relu)
        n = m * hr * wr
        got = self.map.cpu().numpy()
        assert got[:n].tobytes() == want.tobytes(), (key, float(np.abs(got[:n] - want.reshape(-1)).max()))
        assert np.isnan(got[n:]).all(), key                                  # rows >= m and the guard tail
        assert np.array_equal(self.tgt.cpu().numpy()[:m], t) and (self.tgt[m:] == -7).all(), key
        assert self.base.cpu().numpy()[:m].tobytes() == base.tobytes() and torch.isnan(self.base[m:]).all(), key
        # label and base against gt_head_predict's rows, written out
        mean = E._ordered_combine(self.proba[:, :m], w)[0]
        label = np.argmax(mean, 1)
        assert np.array_equal(t, np.where(np.asarray(tgt) < 0, label, tgt)), key
        if self.C >= 2 and tgt[0] < 0:
            assert mean[0, self.C - 2] == mean[0, self.C - 1] == mean[0].max() and t[0] == self.C - 2    # the tie
        score = E._ordered_combine(self.logits[:, :m], w)[0] if logit else mean
        assert base.tobytes() == score[np.arange(m), t].tobytes(), key
        if self.G == 1:
            assert base.tobytes() == (self.logits if logit else self.proba)[0][np.arange(m), t].tobytes(), key
        return want


# (hs, ws, hr, wr, Cp, Cr): padded 7 x 7 in 8 x 8 with 4 of 8 channels; nothing padded; 289 pixels (two per thread)
GEOMS = [(8, 8, 7, 7, 8, 4), (4, 4, 4, 4, 16, 16), (17, 18, 17, 17, 8, 3)]


# G = 1: the classifier's use, three waves without a member; 3: ragged; 64: the LDS tables are full. 2 tiles:
# Up = 32, half the lanes of the channel sums hold no unit; 68: Up = 1088, every thread's unit loop runs 4 or 5 times.
# Every class count 1 to 16, in both element types at G = 1 and 3 and in one (alternating) at G = 64, where the
# twin of 64 members is what takes the time; the geometry moves with (C // 2 + type), so every (type, geometry)
# pair occurs in every parameter set (G = 64 leaves out the 289-pixel geometry: 40 MB of features). Per (C, type):
# the weights uniform or ragged, m = 33 at both scores (ReLU off and on in turn) and m = 1 (the tie row alone,
# its target the label) at one.
@pytest.mark.parametrize("nt", [2, 68])
@pytest.mark.parametrize("G", [1, 3, 64])
def test_head_gradcam_kernel(G, nt):
    ngeom = 3 if G < 64 else 2
    cams = {}
    for C in range(1, 17):
        for d in ((0, 1) if G < 64 else (C % 2,)):
            dtype = (torch.float32, torch.bfloat16)[d]
            gi = (C // 2 + d) % ngeom
            if (gi, d) not in cams:
                cams[(gi, d)] = _Cam(G, nt, C, GEOMS[gi], dtype, 1000 * G + 10 * nt + 2 * gi + d)
            c = cams[(gi, d)].classes(C, 100 * C + d)
            ragged = np.random.default_rng(C).random(G) + 0.1
            w = np.ones(1, np.float32) if G == 1 else \
                ((np.ones(G) / G) if (C + d) % 2 else (ragged / ragged.sum())).astype(np.float32)
            given = np.where(np.arange(33) % 2 == 0, -1, np.arange(33) % C)
            for logit in (0, 1):
                relu = (C + d + logit) % 2
                got = c.check(w, 33, logit, relu, given)
                if G == 1 and C % 5 == 0:                # ReLU on against ReLU off, same launch otherwise
                    other = c.check(w, 33, logit, 1 - relu, given)
                    raw, cut = (other, got) if relu else (got, other)
                    assert cut.tobytes() == np.where(raw > 0, raw, np.float32(0)).tobytes()
            c.check(w, 1, C % 2, (C // 2 + d) % 2, np.array([-1]))
    assert len(cams) == 2 * ngeom


def test_head_gradcam_refusals():
    from gentun_amd.ops import cnn_kernels as K
    c = _Cam(3, 2, 4, GEOMS[0], torch.float32, 5)
    w = torch.full((3,), 1 / 3, device=_dev())
    c.fresh(np.full(5, -1))
    c.tgt[:] = -7
    for kw in (dict(plog=0), dict(b2=0), dict(weight=0), dict(feat=0), dict(hid=0), dict(w2=0), dict(wbar=0),
               dict(tgt=0), dict(base=0), dict(map=0), dict(C=0), dict(C=17), dict(G=0), dict(G=65), dict(Up=24),
               dict(Up=0), dict(Up=4112), dict(Cp=12), dict(Cp=264), dict(Cp=0), dict(Cr=0), dict(Cr=9),
               dict(hs=40, ws=40, hr=33, wr=32), dict(hr=9), dict(wr=9), dict(hr=0), dict(wr=0), dict(m=0), dict(m=-1),
               dict(m=HB + 1), dict(B=0), dict(prec=2), dict(prec=-1), dict(logit=2), dict(logit=-1), dict(relu=2),
               dict(relu=-1)):
        assert c.launch(w, 5, 0, 1, over=kw) != 0, kw
        assert c.untouched(), kw
    assert K.lib().gt_head_gradcam(None, _stream()) != 0
    c.fresh(np.full(HB, -1))
    assert c.launch(w, HB, 1, 1) == 0 and not torch.isnan(c.base).any()          # the edges are accepted: m = B
    big = _Cam(1, 2, 2, (32, 32, 32, 32, 8, 1), torch.bfloat16, 6)              # 1024 pixels: the most
    big.check(np.ones(1, np.float32), 2, 0, 0, np.array([-1, 1]))


# ---------------------------------------------------------------------------------------------------------
# end to end: the classifier
# ---------------------------------------------------------------------------------------------------------

CLF_CASES = ["chain", "mnist", "bn", "bf16"]             # plain 32x32x3 fp32, 28x28x1 stored 32x32, BatchNorm, bf16
NROWS = 70                                               # the last chunk is short at both batch sizes
_CHUNKS = {}


def _buffer(pred, ptr, shape):
    """The predictor's own evaluation twin at device address ``ptr`` as a tensor of ``shape``."""
    for t in pred._keep:
        if t.data_ptr() == ptr:
            return t.view(shape)
    raise AssertionError("no evaluation twin at {:#x}".format(ptr))


def _plain_chunks(pred, xs, G):
    """Per chunk of ``EB`` rows of ``xs``: the predictor's device buffers after a plain forward (``upload`` +
    ``forward``) as host fp32 arrays ``(logits, proba [G, m, C], feat [G, m, hs, ws, Cp], hid [G, m, Up])``;
    computed once per (predictor, rows)."""
    key = (id(pred), len(xs))
    if key not in _CHUNKS:
        job, EB = pred.job, pred.EB
        (hs, ws), Cp = job.final_hw, job.final_cp
        out = []
        with torch.cuda.device(_dev()):
            for s in range(0, len(xs), EB):
                m = min(EB, len(xs) - s)
                pred.upload(xs[s:s + m])
                pred.forward(True) if G > 1 else pred.forward()
                torch.cuda.synchronize()
                feat = _buffer(pred, pred.df.x, (G, EB, hs, ws, Cp))
                hid = _buffer(pred, pred.df.out, (G, EB, job.Up))
                out.append((_f32(pred.logits)[:, :m], _f32(pred.proba)[:, :m], _f32(feat)[:, :m], _f32(hid)[:, :m]))
        _CHUNKS[key] = out
    return _CHUNKS[key]


def _twin_of_predictor(pred, xs, G, w, target, logit, relu):
    """``(map, target, base)`` by the twin from the predictor's own buffers, chunk by chunk."""
    job = pred.job
    (hs, ws), (hr, wr), Cp = job.final_hw, job.final_hw_real, job.final_cp
    Cr = job.members[0][0].kernels_per_layer[-1]
    W1 = _f32(job.views["W1"][0]).reshape(G, hs * ws * Cp, job.Up)
    wbar = R.w1sum_twin(W1, hs, ws, hr, wr, Cp, Cr)
    W2 = _f32(job.views["W2"][0]).reshape(G, job.Up, -1)
    maps, ts, bases, s = [], [], [], 0
    for logits, proba, feat, hid in _plain_chunks(pred, xs, G):
        m = logits.shape[1]
        tgt = np.full(m, -1) if target is None else target[s:s + m]
        got = R.head_twin(logits, proba, w, feat, hid, W2, wbar, tgt, hr, wr, Cr, logit, relu)
        maps.append(got[0]), ts.append(got[1]), bases.append(got[2])
        s += m
    return np.concatenate(maps), np.concatenate(ts), np.concatenate(bases), wbar


@pytest.mark.parametrize("batch", [32, 256])
@pytest.mark.parametrize("case", CLF_CASES)
def test_gradcam_is_the_twin_of_the_predictors_own_buffers(case, batch):
    from gentun_amd.models.cnn_fitted import cam_shape
    m, job, clf, x, lab = F._fit(case)
    xs = x[10:10 + NROWS]
    pred = clf.hip_predictor(_dev(), batch)
    assert pred.EB == batch
    hr, wr = cam_shape(clf.plan, clf.input_shape)
    assert (hr, wr) == tuple(pred.job.final_hw_real) == ((7, 7) if case == "mnist" else (8, 8))
    label = clf.predict(xs, device=_dev(), output="label", batch=batch)
    other = (label + 1 + np.arange(NROWS)) % clf.classes
    one = np.ones(1, np.float32)
    for score, relu, target, t in (("logit", True, None, label), ("proba", False, other, other),
                                   ("proba", True, None, label), ("logit", False, 3, np.full(NROWS, 3))):
        got, info = clf.gradcam(xs, target=target, score=score, relu=relu, device=_dev(), batch=batch,
                                return_info=True)
        tt = None if target is None else t
        want, wt, wbase, wbar = _twin_of_predictor(pred, xs, 1, one, tt, score == "logit", relu)
        assert got.dtype == np.float32 and got.shape == (NROWS, hr, wr) and np.isfinite(got).all()
        assert got.tobytes() == want.tobytes(), (score, relu, float(np.abs(got - want).max()))
        assert info["target"].dtype == np.int64 and np.array_equal(info["target"], t) and np.array_equal(wt, t)
        assert info["base"].dtype == np.float32 and info["base"].tobytes() == wbase.tobytes()
        plain = clf.predict(xs, device=_dev(), output="logits" if score == "logit" else "proba", batch=batch)
        assert info["base"].tobytes() == plain[np.arange(NROWS), t].tobytes()
        assert np.abs(got).max() > 0
        assert _f32(pred._cam_wbar).tobytes() == wbar.tobytes()
    assert clf.hip_predictor(_dev(), batch) is pred and len(pred._cam) == 4              # the cached predictor, lazily
    if batch == 256:                                     # batch 32 = batch 256, and the model forwards
        for score in ("logit", "proba"):
            assert clf.gradcam(xs, score=score, device=_dev(), batch=32).tobytes() == \
                clf.gradcam(xs, score=score, device=_dev(), batch=256).tobytes()
        assert m.gradcam(xs[:5], upsample=True).tobytes() == clf.gradcam(xs[:5], upsample=True, device=_dev()).tobytes()


@pytest.mark.parametrize("case", ["mnist", "bf16"])
def test_predict_tta_and_occlusion_are_unchanged_by_gradcam(case):
    m, job, clf, x, lab = F._fit(case)
    xs = x[:70]
    tta = {"shift": 2, "flip": True}
    for batch in (32, 256):
        def others():
            out = [clf.predict(xs, device=_dev(), output=o, batch=batch) for o in ("logits", "proba")]
            out.append(clf.predict(xs, device=_dev(), output="logits", batch=batch, tta=tta))
            out.append(clf.occlusion(xs[:3], patch=8, fill=0.5, device=_dev(), batch=batch))
            return out
        before = others()
        first = clf.gradcam(xs, score="proba", device=_dev(), batch=batch)
        after = others()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # and the other way round: the Grad-CAM path after the plain, the TTA and the occlusion path
        assert clf.gradcam(xs, score="proba", device=_dev(), batch=batch).tobytes() == first.tobytes()


def test_cross_validate_is_unchanged_by_gradcam():
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    scores = list(m.fold_scores)
    m.fit()
    plain = m.predict(x[:40], output="logits")
    assert m.gradcam(x[:4]).shape == (4, 7, 7)                           # the model forwards to the classifier
    assert m.predict(x[:40], output="logits").tobytes() == plain.tobytes()
    assert m.cross_validate() == first and m.fold_scores == scores


# ---------------------------------------------------------------------------------------------------------
# end to end: the ensemble
# ---------------------------------------------------------------------------------------------------------

def _check_ensemble(ens, xs, twin):
    """``ens.gradcam`` against its members' own predictors (at the ensemble's rows per launch and targets)
    combined in member order; with ``twin`` also against the twin of the ensemble predictor's own buffers."""
    pred = ens.hip_predictor(_dev(), 256)
    n = len(xs)
    label = ens.predict(xs, device=_dev(), output="label")
    other = (label + 2) % ens.classes
    for score, relu, target, t in (("logit", True, None, label), ("proba", False, other, other),
                                   ("proba", True, None, label)):
        got, info = ens.gradcam(xs, target=target, score=score, relu=relu, device=_dev(), return_info=True)
        per = [mem.gradcam(xs, target=t, score=score, relu=relu, device=_dev(), batch=pred.EB, return_info=True)
               for mem in ens.members]
        want = R.ordered_mean(ens.weights, np.stack([p[0] for p in per]))
        base = R.ordered_mean(ens.weights, np.stack([p[1]["base"] for p in per]))
        assert got.dtype == np.float32 and np.isfinite(got).all() and np.abs(got).max() > 0
        assert got.tobytes() == want.tobytes(), (score, relu, float(np.abs(got - want).max()))
        assert np.array_equal(info["target"], t) and info["base"].tobytes() == base.tobytes()
        if twin:
            tw = _twin_of_predictor(pred, xs, len(ens), ens.weights, None if target is None else t,
                                    score == "logit", relu)
            assert got.tobytes() == tw[0].tobytes() and np.array_equal(tw[1], t)
            assert info["base"].tobytes() == tw[2].tobytes()
    assert ens.gradcam(xs, score="proba", device=_dev(), return_info=True)[1]["base"].tobytes() == \
        ens.predict(xs, device=_dev())[np.arange(n), label].tobytes()
    return pred


@pytest.mark.parametrize("case", list(E.CASES))
def test_ensemble_of_three(case):
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = E._fit(case)
    xs = x[10:10 + NROWS]
    plain = fitted.predict_outputs(x[:70], device=_dev(), batch=256)
    for weights in (None, [3.0, 1.0, 4.0]):
        ens = fitted if weights is None else CnnEnsemble(fitted.members, weights=weights)
        _check_ensemble(ens, xs, True)
    again = fitted.predict_outputs(x[:70], device=_dev(), batch=256)     # the plain path after the Grad-CAM path
    for name in plain:
        assert again[name].tobytes() == plain[name].tobytes(), name


def test_ensemble_of_sixteen_runs_at_the_lowered_rows_per_launch():
    import test_cnn_occlusion_gpu as O
    import test_cnn_tta_gpu as T
    from gentun_amd.models import fit_ensemble
    shape, classes = E.CASES["rgb"][:2]
    x, y, lab = E._data(shape, classes)
    if "ens" not in O._SIXTEEN:
        O._SIXTEEN["ens"] = fit_ensemble(x, y, T._genomes16(), device=_dev(), **E._space("rgb"))
    ens = O._SIXTEEN["ens"]
    assert len(ens) == 16
    pred = _check_ensemble(ens, x[10:10 + NROWS], False)
    assert pred.EB == pred.job.eval_batch() and 32 <= pred.EB < 256 and pred.EB < NROWS
    print("[cnn-gradcam] k = 16: {} rows per launch".format(pred.EB))


# ---------------------------------------------------------------------------------------------------------
# refusal; accuracy
# ---------------------------------------------------------------------------------------------------------

def test_more_than_16_classes():
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes = (8, 8, 3), 17
    x, y, lab = F._noise_data(shape, classes, n=64)
    kw = dict(nodes=(3,), input_shape=shape, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
              dropout_probability=0.5, classes=classes, nfold=2, epochs=(1,), learning_rate=(1e-3,), batch_size=32)
    clf = GeneticCnnModel(x, y, {"S_1": "101"}, backend="torch", device="cpu", **kw).fit()
    assert clf.gradcam(x[:4], target=16).shape == (4, 4, 4)
    assert clf.gradcam(x[:4], device=_dev(), backend="torch").shape == (4, 4, 4)
    with pytest.raises(ValueError, match="16 classes"):
        clf.gradcam(x[:4], device=_dev())


@pytest.mark.parametrize("case", ["chain", "mnist", "bn"])
def test_map_against_the_fp64_autograd_map(case):
    """fp32 fits, ``relu=False``: the largest error of the HIP map against the fp64 autograd map (the torch
    backend in fp64 on the CPU), relative to the largest fp64 map value, is at most 4x that of the stock-torch
    fp32 autograd map (same GPU) against the same fp64 map -- the factor of the predictor's logits and of the
    occlusion map. The gradient jumps where a hidden unit crosses zero, so images whose smallest fp64 ``|z_u|``
    over the real units is below ``1e-5 * max |z|`` of the batch are left out, at most 10 % of them."""
    m, job, clf, x, lab = F._fit(case)
    xs = x[10:10 + NROWS]
    cpu = torch.device("cpu")
    buf = np.zeros((96,) + (clf.input_shape[2],) + clf.input_shape[:2], np.float32)
    buf[:NROWS] = xs.transpose(0, 3, 1, 2)
    with torch.no_grad():
        A64 = clf._torch_features(torch.from_numpy(buf).double(), clf._tensors(cpu, torch.float64))[:NROWS].numpy()
    z = np.abs(R.head64(clf.params, A64)[0])
    keep = z.min(1) >= 1e-5 * z.max()
    out = int((~keep).sum())
    assert out <= NROWS // 10
    t = clf.predict(xs, device=_dev(), output="label")
    for score in ("logit", "proba"):
        ref = clf._torch_gradcam(xs, t, score, False, cpu, 256, torch.float64)[0]
        assert ref.dtype == np.float64
        hip = clf.gradcam(xs, target=t, score=score, relu=False, device=_dev())
        t32 = clf.gradcam(xs, target=t, score=score, relu=False, device=_dev(), backend="torch")
        scale = float(np.abs(ref[keep]).max())
        e_hip = float(np.abs(hip - ref)[keep].max()) / scale
        e_torch = float(np.abs(t32 - ref)[keep].max()) / scale
        print("[cnn-gradcam] {} {} map vs fp64: HIP {:.3e}, torch fp32 (GPU) {:.3e}, left out {} of {}".format(
            case, score, e_hip, e_torch, out, NROWS))
        assert scale > 0 and e_hip <= 4 * e_torch
