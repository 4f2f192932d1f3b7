"""Occlusion sensitivity of fitted Genetic-CNN models on an MI355X: ``gt_occlude_views`` (csrc/hip/cnn_occlude.hip)
alone against the per-pixel oracle (tests/occlusion_ref.py), ``gt_head_occlusion`` (csrc/hip/cnn_dense.hip) alone
against ``gt_head_predict``'s rows combined in numpy, then ``occlusion(device=cuda)`` of ``CnnClassifier`` and
``CnnEnsemble`` through the HIP predictors against the same predictors fed the oracle's occluded images through
plain ``predict``, followed by the numpy subtraction.

Every comparison but the last test's is byte equality or a refusal; they rest on a property the suite already
tests, that a row's HIP prediction does not depend on its position or on the rows beside it. The fits are those
of tests/test_cnn_fitted_gpu.py and tests/test_cnn_ensemble_gpu.py (320 rows, 1 epoch, batch 32; shared with them
inside one pytest process, left unchanged) plus one 16-member ensemble."""

import numpy as np
import pytest
import torch

import occlusion_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------
# gt_occlude_views alone
# ---------------------------------------------------------------------------------------------------------

GEOMETRIES = {"cifar": ((32, 32, 3), (32, 32, 8)), "mnist": ((28, 28, 1), (32, 32, 8)), "odd": ((6, 5, 3), (8, 8, 8))}
GUARD = 4096                 # elements past the staging tensor: all stay NaN
M, ROWS = 3, 10              # images in the raw buffer, rows per launch


class _Occ(object):
    """A raw buffer ``[m][Hp][Wp][Cp]`` of small positive integers (exact in bf16, never 0) in the real extent --
    in the channel padding too, which the kernel copies -- and NaN outside the real extent, which it must not
    read; a fill of ``Cp`` other integers; a NaN-filled staging tensor of ``rows`` rows with a NaN guard tail."""

    def __init__(self, real, stored, dtype, m=M, rows=ROWS, seed=0):
        (self.Hr, self.Wr, self.C), (self.Hp, self.Wp, self.Cp) = real, stored
        self.m, self.rows, self.dtype = m, rows, dtype
        rs = np.random.RandomState(seed)
        self.data = rs.randint(1, 200, size=(m, self.Hr, self.Wr, self.Cp)).astype(np.float32)
        self.fillv = (200 + np.arange(self.Cp)).astype(np.float32)       # told apart from every data value
        raw = np.full((m, self.Hp, self.Wp, self.Cp), np.nan, np.float32)
        raw[:, :self.Hr, :self.Wr] = self.data
        self.raw = torch.from_numpy(raw).to(device=_dev(), dtype=dtype).contiguous()
        self.fill = torch.from_numpy(self.fillv).to(device=_dev(), dtype=dtype)
        self.img = self.Hp * self.Wp * self.Cp
        self.out = torch.full((rows * self.img + GUARD,), float("nan"), dtype=dtype, device=_dev())
        self.nan_bits = _bits(self.out)[0].item()
        self.seen = {}

    def args(self, patch, stride, w0=0, base=0, over=()):
        from gentun_amd.ops import cnn_kernels as K
        Gh, Gw = R.grid(self.Hr, self.Wr, patch, stride)
        a = K.OccludeArgs()
        a.raw, a.out, a.fill = self.raw.data_ptr(), self.out.data_ptr(), self.fill.data_ptr()
        a.m, a.w0, a.Cc, a.Gw, a.patch, a.stride = self.m, w0, Gh * Gw, Gw, patch, stride
        a.rows = a.cap = self.rows
        a.Hp, a.Wp, a.Hr, a.Wr, a.Cp = self.Hp, self.Wp, self.Hr, self.Wr, self.Cp
        a.prec, a.base = 1 if self.dtype == torch.float32 else 0, base
        for k, v in dict(over).items():                  # any field, after the consistent ones
            setattr(a, k, v)
        return a

    def launch(self, a):
        from gentun_amd.ops import cnn_kernels as K
        self.out.fill_(float("nan"))
        rc = K.lib().gt_occlude_views(a, _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self, start=0):
        return bool((_bits(self.out[start:]) == self.nan_bits).all().item())

    def oracle(self, r, cell, patch, stride):
        key = (r, cell, patch, stride)
        if key not in self.seen:
            self.seen[key] = R.occlude(self.data[r], cell, patch, stride, self.fillv, (self.Hp, self.Wp))
        return self.seen[key]

    def check(self, patch, stride, w0, base):
        Gh, Gw = R.grid(self.Hr, self.Wr, patch, stride)
        Cc = Gh * Gw
        want = np.zeros((self.rows, self.Hp, self.Wp, self.Cp), np.float32)
        live = 0
        for j in range(self.rows):
            w = j if base else w0 + j
            if w < (self.m if base else self.m * Cc):
                want[j] = self.oracle(w, None, patch, stride) if base else self.oracle(w // Cc, w % Cc, patch, stride)
                live += 1
        assert not np.isnan(want).any()                  # zeros outside the real extent, never the raw NaN
        n = self.rows * self.img
        got = self.out[:n].cpu()
        want = torch.from_numpy(want).to(self.dtype).reshape(-1)
        assert torch.equal(_bits(got), _bits(want)), (patch, stride, w0, base)
        assert self.untouched(n)                         # the guard past `rows`
        return live


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_views_kernel_equals_the_oracle(geom, dtype):
    real, stored = GEOMETRIES[geom]
    top = min(real[0], real[1])
    c = _Occ(real, stored, dtype)
    # patch 1, 2 and the whole image; stride < patch; the last windows of (4, 3) are clipped at 32 and 6 x 5
    # pixels, those of (5, 4) at 32 and 28
    for patch, stride in ((1, 1), (2, 2), (top, top), (4, 2), (4, 3), (top, 1) if geom == "odd" else (5, 4)):
        Cc = int(np.prod(R.grid(real[0], real[1], patch, stride)))
        assert c.launch(c.args(patch, stride, base=1, w0=7)) == 0        # base mode: m < rows, w0 is not read
        assert c.check(patch, stride, 0, True) == M
        starts = {0, max(0, Cc - 4), max(0, M * Cc - 3)}                 # straddles images 0 | 1; ends mid-image
        for w0 in sorted(starts):
            assert c.launch(c.args(patch, stride, w0=w0)) == 0
            live = c.check(patch, stride, w0, False)
            assert live == min(ROWS, M * Cc - w0)
        if Cc >= 4:
            assert (Cc - 4) // Cc != (Cc - 4 + ROWS - 1) // Cc           # that launch does hold two images
    # the last cell of a clipped grid changes fewer pixels than a whole patch
    cp, cs = (4, 3) if geom == "odd" else (5, 4)
    a = c.oracle(0, int(np.prod(R.grid(real[0], real[1], cp, cs))) - 1, cp, cs)
    assert 0 < (a[:real[0], :real[1]] != c.data[0]).any(-1).sum() < cp * cp
    # exactly as many staging rows as items, and one row only
    for rows, w0 in ((M * 4, 0), (1, 5)):
        c = _Occ(real, stored, dtype, rows=rows, seed=1)
        assert R.grid(real[0], real[1], top - 1, top - 1) == (2, 2)
        assert c.launch(c.args(top - 1, top - 1, w0=w0)) == 0
        assert c.check(top - 1, top - 1, w0, False) == rows


def test_views_launcher_refusals():
    from gentun_amd.ops import cnn_kernels as K
    c = _Occ((6, 5, 3), (8, 8, 8), torch.float32)
    assert c.launch(c.args(4, 3)) == 0 and not c.untouched()              # the accepted call does write
    assert K.lib().gt_occlude_views(None, _stream()) != 0
    for kw in (dict(raw=0), dict(out=0), dict(fill=0), dict(Cp=12), dict(Cp=4), dict(Cp=0), dict(Hr=9), dict(Wr=9),
               dict(Hr=0), dict(Wr=-1), dict(patch=0), dict(patch=6), dict(patch=-4), dict(stride=0), dict(stride=5),
               dict(stride=-1), dict(Cc=3), dict(Cc=5), dict(Cc=0), dict(Gw=1), dict(Gw=4), dict(Gw=0),
               dict(Cc=2, Gw=1),                                          # a grid, but not this geometry's
               dict(m=0), dict(m=-1), dict(w0=-1), dict(w0=-2 ** 31), dict(rows=0), dict(rows=-1),
               dict(rows=ROWS + 1), dict(cap=ROWS - 1), dict(cap=0), dict(prec=2), dict(prec=-1), dict(base=2),
               dict(w0=2 ** 31 - 1), dict(m=2 ** 30),                     # items past 32 bits
               dict(Hp=2 ** 15, Wp=2 ** 15, Cp=2 ** 15)):                 # chunks past FastDiv's range
        assert c.launch(c.args(4, 3, over=kw)) != 0, kw
        assert c.untouched(), kw
    big = _Occ((65, 64, 1), (72, 64, 8), torch.float32, m=1, rows=1)
    assert big.launch(big.args(1, 1)) != 0 and big.untouched()            # 4160 cells
    assert c.launch(c.args(5, 1)) == 0                                    # patch = min(Hr, Wr) is the largest
    assert c.launch(c.args(4, 3, w0=M * 4)) == 0 and c.check(4, 3, M * 4, False) == 0      # past the items: zeros


# ---------------------------------------------------------------------------------------------------------
# gt_head_occlusion alone
# ---------------------------------------------------------------------------------------------------------

def _head_occ(plog, b2, w, tgt, base, mp, m, Cc, w0, phase, logit=0, over=()):
    """One launch over device tensors ``tgt`` / ``base`` / ``mp``, which it may write; returns the status."""
    from gentun_amd.ops import cnn_kernels as K
    G, nt, B, C = plog.shape
    a = K.HeadOcclusionArgs()
    a.plog, a.b2, a.weight = plog.data_ptr(), b2.data_ptr(), w.data_ptr()
    a.tgt, a.base, a.map = tgt.data_ptr(), base.data_ptr(), mp.data_ptr()
    a.G, a.B, a.Up, a.C = G, B, nt * 16, C
    a.m, a.Cc, a.w0, a.phase, a.logit = m, Cc, w0, phase, logit
    for k, v in dict(over).items():                      # any field, after the consistent ones
        setattr(a, k, v)
    rc = K.lib().gt_head_occlusion(a, _stream())
    torch.cuda.synchronize()
    return rc


HM, HCC, HB = 5, 13, 32      # 65 items: launches from 0, 32 (mid-image 2) and 64 (one live row)


def _check_head(plog, b2, w, score, proba, C):
    """Phase 0 with given and with -1 targets, then phase 1 at three starts, against ``score`` / ``proba``
    ``[B][C]``, the launch rows' score vectors and combined probabilities by numpy."""
    G = plog.shape[0]
    dev = plog.device
    logit = 0 if score is proba else 1
    label = np.argmax(proba, 1)
    for given in (np.full(HM, -1), np.arange(HM) % C, np.array([C - 1, -1, 0, -1, C // 2])):
        tgt = torch.full((HB,), -7, dtype=torch.int32, device=dev)
        tgt[:HM] = torch.from_numpy(given.astype(np.int32))
        base = torch.full((HB,), float("nan"), device=dev)
        mp = torch.full((HM * HCC + 8,), float("nan"), device=dev)
        assert _head_occ(plog, b2, w, tgt, base, mp, HM, HCC, 0, 0, logit) == 0
        t = np.where(given < 0, label[:HM], given)
        assert np.array_equal(tgt.cpu().numpy()[:HM], t) and (tgt[HM:] == -7).all()
        assert base.cpu().numpy()[:HM].tobytes() == score[np.arange(HM), t].tobytes()
        assert torch.isnan(base[HM:]).all() and torch.isnan(mp).all()    # rows past m and the map: untouched
    # phase 1 reads tgt and base: any values, not those of phase 0
    rng = np.random.default_rng(C)
    t = rng.integers(0, C, HM)
    b = rng.standard_normal(HM).astype(np.float32)
    tgt = torch.from_numpy(t.astype(np.int32)).to(dev)
    base = torch.from_numpy(b).to(dev)
    for w0 in (0, 20, 64):
        mp = torch.full((HM * HCC + 8,), float("nan"), device=dev)
        assert _head_occ(plog, b2, w, tgt, base, mp, HM, HCC, w0, 1, logit) == 0
        live = min(HB, HM * HCC - w0)
        items = w0 + np.arange(live)
        want = np.subtract(b[items // HCC], score[np.arange(live), t[items // HCC]], dtype=np.float32)
        got = mp.cpu().numpy()
        assert got[w0:w0 + live].tobytes() == want.tobytes(), (G, C, w0)
        assert np.isnan(got[:w0]).all() and np.isnan(got[w0 + live:]).all()
        assert np.array_equal(tgt.cpu().numpy(), t) and base.cpu().numpy().tobytes() == b.tobytes()


# G = 1: the classifier's use, three waves without a member; 3: ragged; 64: the LDS table is full and every
# wave's member loop runs 16 times. 68 tiles: the lane's stride loop runs twice.
@pytest.mark.parametrize("nt", [2, 68])
@pytest.mark.parametrize("G", [1, 3, 64])
def test_head_occlusion_kernel(G, nt):
    for C in (1, 2, 3, 10, 16):
        rng = np.random.default_rng(100 * G + nt + C)
        plog = rng.standard_normal((G, nt, HB, C)).astype(np.float32)
        b2 = rng.standard_normal((G, C)).astype(np.float32)
        if C >= 2:                                       # row 0 of every member: the two last classes tie at the top
            plog[:, :, 0, :] = 0.0
            plog[:, 0, 0, C - 2:] = 7.0
            b2[:, C - 1] = b2[:, C - 2]
        dp, db = torch.from_numpy(plog).to(_dev()), torch.from_numpy(b2).to(_dev())
        row_logits, row_proba = F._head_predict(dp, db)                  # [G][B][C]: every launch row
        ragged = rng.random(G) + 0.1
        for w in ([np.ones(1, np.float32)] if G == 1 else
                  [(np.ones(G) / G).astype(np.float32), (ragged / ragged.sum()).astype(np.float32)]):
            dw = torch.from_numpy(w).to(_dev())
            proba = E._ordered_combine(row_proba, w)[0]
            if C >= 2:
                assert proba[0, C - 2] == proba[0, C - 1] == proba[0].max()          # the exact tie: the lower wins
            _check_head(dp, db, dw, proba, proba, C)
            if G == 1:
                assert proba.tobytes() == row_proba[0].tobytes()         # 1.0f * p is p
                _check_head(dp, db, dw, row_logits[0], proba, C)         # score = logit, the label still by proba


def test_head_occlusion_refusals():
    t, o = torch.zeros(4096, device=_dev()), torch.zeros(4096, device=_dev())
    ti = torch.zeros(4096, dtype=torch.int32, device=_dev())
    plog, b2, w = t[:3 * 2 * 32 * 2].view(3, 2, 32, 2), t[:6].view(3, 2), t[:3]

    def rc(m=5, Cc=13, w0=0, phase=1, logit=0, p=plog, **kw):
        return _head_occ(p, b2, w, ti, o[:64], o[64:], m, Cc, w0, phase, logit, over=kw)
    for kw in (dict(G=0), dict(G=65), dict(C=0), dict(C=17), dict(Up=24), dict(Up=0), dict(B=0), dict(m=0), dict(m=-1),
               dict(Cc=0), dict(Cc=-1), dict(m=2 ** 20, Cc=2 ** 12), dict(phase=2), dict(phase=-1), dict(logit=2),
               dict(logit=1),                                             # the logit score with three members
               dict(w0=-1), dict(w0=65), dict(w0=2 ** 31 - 1), dict(map=0),
               dict(phase=0, m=33),                                       # more images than launch rows
               dict(plog=0), dict(b2=0), dict(weight=0), dict(tgt=0), dict(base=0)):
        assert rc(**kw) != 0, kw
    from gentun_amd.ops import cnn_kernels as K
    assert K.lib().gt_head_occlusion(None, _stream()) != 0
    torch.cuda.synchronize()
    assert not bool(o.any()) and not bool(ti.any())     # nothing was launched (a base score here is 0.5)
    assert rc(w0=64) == 0 and rc(phase=0, map=0) == 0 and rc(logit=1, p=plog[:1]) == 0     # the edges are accepted


# ---------------------------------------------------------------------------------------------------------
# end to end: the classifier
# ---------------------------------------------------------------------------------------------------------

CLF_CASES = ["chain", "mnist", "bn", "bf16"]             # plain 32x32x3 fp32, 28x28x1 stored 32x32, BatchNorm, bf16
# (images, patch, stride, batch): 80 items over 3 packed launches of 32 rows; 338 (28 x 28) or 450 items over 2 of 256
SHAPES = [(5, 8, 8, 32), (2, 4, 2, 256)]
FILL = 0.5
_VIEWS = {}


def _oracle_views(x, patch, stride, fill):
    """``[n * Cc, H, W, C]`` by the oracle; computed once per (image set, setting)."""
    key = (x.shape, x.tobytes(), patch, stride, repr(fill))
    if key not in _VIEWS:
        _VIEWS[key] = R.views(x, patch, stride, fill).reshape((-1,) + x.shape[1:])
    return _VIEWS[key]


def _want(predict, x, t, patch, stride, fill):
    """``(map, base)`` written out: ``predict`` of the images and of the oracle's copies, one fp32 subtraction."""
    n = len(x)
    views = _oracle_views(x, patch, stride, fill)
    Cc = len(views) // n
    base = predict(x)[np.arange(n), t]
    sv = predict(views).reshape(n, Cc, -1)[np.arange(n), :, t]
    out = np.subtract(base[:, None], sv, dtype=np.float32)
    return out.reshape((n,) + R.grid(x.shape[1], x.shape[2], patch, stride)), base


@pytest.mark.parametrize("shape", SHAPES, ids=["5x16@32", "2xp4s2@256"])
@pytest.mark.parametrize("case", CLF_CASES)
def test_occlusion_is_base_minus_the_predictions_of_the_oracles_views(case, shape):
    m, job, clf, x, lab = F._fit(case)
    n, patch, stride, batch = shape
    xs = x[10:10 + n]
    Gh, Gw = R.grid(clf.input_shape[0], clf.input_shape[1], patch, stride)
    pred = clf.hip_predictor(_dev(), batch)
    assert pred.EB == batch and -(-n * Gh * Gw // batch) == (3 if batch == 32 else 2)
    label = clf.predict(xs, device=_dev(), output="label", batch=batch)
    other = (label + 1 + np.arange(n)) % clf.classes
    for score, output in (("proba", "proba"), ("logit", "logits")):
        def predict(images):
            return clf.predict(images, device=_dev(), output=output, batch=batch)
        for target, t in ((None, label), (other, other), (3, np.full(n, 3))):
            want, base = _want(predict, xs, t, patch, stride, FILL)
            got, info = clf.occlusion(xs, target=target, patch=patch, stride=stride, fill=FILL, score=score,
                                      device=_dev(), batch=batch, return_info=True)
            assert got.dtype == np.float32 and got.shape == (n, Gh, Gw) and np.isfinite(got).all()
            assert got.tobytes() == want.tobytes(), (score, target, float(np.abs(got - want).max()))
            assert info["target"].dtype == np.int64 and np.array_equal(info["target"], t)
            assert info["base"].dtype == np.float32 and info["base"].tobytes() == base.tobytes()
        assert np.abs(got).max() > 0
    assert clf.hip_predictor(_dev(), batch) is pred and len(pred._occ) >= 2          # the cached predictor, lazily
    assert m.occlusion(xs, patch=patch, stride=stride, fill=FILL, batch=batch).tobytes() == \
        clf.occlusion(xs, patch=patch, stride=stride, fill=FILL, batch=batch, device=_dev()).tobytes()


@pytest.mark.parametrize("case", CLF_CASES)
def test_a_cell_that_already_holds_the_fill_scores_exactly_zero(case):
    m, job, clf, x, lab = F._fit(case)
    C = clf.input_shape[2]
    fill = [0.5, -1.0, 0.25][:C]
    xs = x[:3].copy()
    xs[0, 8:16, 16:24] = fill                           # cell (1, 2) of patch 8 / stride 8
    xs[1] = fill                                        # every cell
    for score in ("proba", "logit"):
        got = clf.occlusion(xs, patch=8, stride=8, fill=fill, score=score, device=_dev(), batch=32)
        assert got[0, 1, 2] == 0.0 and got[0].any()
        assert not got[1].any() and got[2].any()
    assert not clf.occlusion(np.zeros_like(xs), patch=5, stride=3, device=_dev()).any()     # the default fill


@pytest.mark.parametrize("case", ["mnist", "bf16"])
def test_predict_and_tta_are_unchanged_by_occlusion(case):
    m, job, clf, x, lab = F._fit(case)
    xs = x[:70]
    tta = {"shift": 2, "flip": True}
    for batch in (32, 256):
        before = [clf.predict(xs, device=_dev(), output=o, batch=batch) for o in ("logits", "proba")]
        before.append(clf.predict(xs, device=_dev(), output="logits", batch=batch, tta=tta))
        first = clf.occlusion(xs[:3], patch=4, stride=3, fill=-2.0, device=_dev(), batch=batch)
        after = [clf.predict(xs, device=_dev(), output=o, batch=batch) for o in ("logits", "proba")]
        after.append(clf.predict(xs, device=_dev(), output="logits", batch=batch, tta=tta))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # and the other way round: the occlusion path after the plain and the TTA path
        assert clf.occlusion(xs[:3], patch=4, stride=3, fill=-2.0, device=_dev(), batch=batch).tobytes() == \
            first.tobytes()


def test_cross_validate_is_unchanged_by_occlusion():
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    scores = list(m.fold_scores)
    m.fit()
    plain = m.predict(x[:40], output="logits")
    assert m.occlusion(x[:4], patch=7).shape == (4, 4, 4)                # the model forwards to the classifier
    assert m.predict(x[:40], output="logits").tobytes() == plain.tobytes()
    assert m.cross_validate() == first and m.fold_scores == scores


# ---------------------------------------------------------------------------------------------------------
# end to end: the ensemble
# ---------------------------------------------------------------------------------------------------------

def _check_ensemble(ens, xs, patch, stride, members):
    from gentun_amd.models.cnn_ensemble import combine
    pred = ens.hip_predictor(_dev(), 256)
    n = len(xs)
    views = _oracle_views(xs, patch, stride, FILL)

    def predict(images):
        out = ens.predict_outputs(images, ("member_proba",), device=_dev(), batch=256)["member_proba"]
        for g in members:                               # the members' own predictors at the ensemble's rows
            assert out[g].tobytes() == ens.members[g].predict(images, device=_dev(), batch=pred.EB).tobytes(), g
        return combine(out, ens.weights)[0]
    assert predict(xs).tobytes() == ens.predict(xs, device=_dev()).tobytes()
    label = ens.predict(xs, device=_dev(), output="label")
    other = (label + 2) % ens.classes
    for target, t in ((None, label), (other, other)):
        want, base = _want(predict, xs, t, patch, stride, FILL)
        got, info = ens.occlusion(xs, target=target, patch=patch, stride=stride, fill=FILL, device=_dev(),
                                  return_info=True)
        assert got.dtype == np.float32 and np.isfinite(got).all() and np.abs(got).max() > 0
        assert got.tobytes() == want.tobytes(), (target, float(np.abs(got - want).max()))
        assert np.array_equal(info["target"], t) and info["base"].tobytes() == base.tobytes()
    with pytest.raises(ValueError):
        ens.occlusion(xs, score="logit", device=_dev())
    return pred, len(views)


@pytest.mark.parametrize("case", list(E.CASES))
def test_ensemble_of_three(case):
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = E._fit(case)
    xs = x[10:13]
    plain = fitted.predict_outputs(x[:70], device=_dev(), batch=256)
    for weights in (None, [3.0, 1.0, 4.0]):
        ens = fitted if weights is None else CnnEnsemble(fitted.members, weights=weights)
        pred, items = _check_ensemble(ens, xs, 8, 6, range(E.K3) if weights is None else ())
        assert items == 3 * 25                          # 5 x 5 cells at 32 x 32 and at 28 x 28 (clipped there)
    again = fitted.predict_outputs(x[:70], device=_dev(), batch=256)     # the plain path after the occlusion path
    for name in plain:
        assert again[name].tobytes() == plain[name].tobytes(), name


_SIXTEEN = {}


def test_ensemble_of_sixteen_packs_launches_of_fewer_rows():
    import test_cnn_tta_gpu as T
    from gentun_amd.models import fit_ensemble
    shape, classes = E.CASES["rgb"][:2]
    x, y, lab = E._data(shape, classes)
    if "ens" not in _SIXTEEN:
        _SIXTEEN["ens"] = fit_ensemble(x, y, T._genomes16(), device=_dev(), **E._space("rgb"))
    ens = _SIXTEEN["ens"]
    assert len(ens) == 16
    pred, items = _check_ensemble(ens, x[10:13], 8, 8, (0, 15))
    # 16 groups fit the twin budget only below the 256 rows asked for: 48 items straddle the launches
    assert pred.EB == pred.job.eval_batch() and 32 <= pred.EB < 256 and items == 48
    print("[cnn-occlusion] k = 16: {} rows per launch, {} packed launches".format(pred.EB, -(-items // pred.EB)))


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
    assert clf.occlusion(x[:4], target=16).shape == (4, 2, 2)
    assert clf.occlusion(x[:4], device=_dev(), backend="torch").shape == (4, 2, 2)
    with pytest.raises(ValueError, match="16 classes"):
        clf.occlusion(x[:4], device=_dev())


def test_logit_map_against_the_fp64_map():
    """The largest error of the HIP logit-score map against the fp64 torch-backend map is at most 4x that of the
    stock-torch fp32 map (same GPU) against the same fp64 map: the yardstick of
    tests/test_cnn_fitted_gpu.py::test_logits_against_the_fp64_oracle, here without its floor. The map is a
    difference of two logits, so its error is that of the logits, not smaller."""
    m, job, clf, x, lab = F._fit("chain")
    e_hip = e_torch = scale = 0.0
    for n, patch, stride, batch in SHAPES:
        xs = x[10:10 + n]
        t = clf.predict(xs, device=_dev(), output="label")
        views = _oracle_views(xs, patch, stride, FILL)

        def predict64(images):
            return clf.predict(images, device="cpu", output="logits", dtype=torch.float64)
        base = predict64(xs)[np.arange(n), t]
        ref = base[:, None] - predict64(views).reshape(n, len(views) // n, -1)[np.arange(n), :, t]
        assert ref.dtype == np.float64
        kw = dict(target=t, patch=patch, stride=stride, fill=FILL, score="logit", device=_dev(), batch=batch)
        hip = clf.occlusion(xs, **kw).reshape(n, -1)
        t32 = clf.occlusion(xs, backend="torch", **kw).reshape(n, -1)
        e_hip = max(e_hip, float(np.abs(hip - ref).max()))
        e_torch = max(e_torch, float(np.abs(t32 - ref).max()))
        scale = max(scale, float(np.abs(ref).max()))
    print("[cnn-occlusion] logit map vs fp64: HIP {:.3e}, torch fp32 (GPU) {:.3e}, largest |map| {:.3e}".format(
        e_hip, e_torch, scale))
    assert e_hip <= 4 * e_torch
