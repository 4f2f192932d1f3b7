"""RISE saliency on an MI355X: ``gt_rise_views`` / ``gt_rise_masks`` (csrc/hip/cnn_rise.hip) byte for byte against
the loop oracle tests/rise_ref.py, ``gt_head_rise`` against ``gt_head_predict``'s rows combined in numpy,
``gt_rise_accumulate`` against an fp64 product, then ``rise(device=cuda)`` against the same predictors fed the
oracle's views through plain ``predict``. The accumulate's bound is the project's form for a split-fp32 reduction
of length ``K`` (tests/test_cnn_saliency_gpu.py, ``gt_conv_in_dgrad``): ``(K + 4) * 2^-24 * sum |terms|``."""

import numpy as np
import pytest
import torch

import rise_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F
from test_cnn_occlusion_gpu import GEOMETRIES, _bits, _dev, _stream

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
GUARD, M, ROWS, NMASK, SEED, P = 4096, 3, 10, 7, 3, 0.5


def _K():
    from gentun_amd.ops import cnn_kernels as K
    return K


def _thr(p):
    return int(p * 4294967296.0)


def _set(a, over):
    for k, v in dict(over).items():                      # any field, after the consistent ones
        setattr(a, k, v)
    return a


def _bound(S, Ms, p):
    """``(fp64 map, bound)`` of scores ``S [n, K]`` and masks ``Ms [K, H, W]``."""
    inv, M64 = 1.0 / (len(Ms) * p), Ms.reshape(len(Ms), -1).astype(np.float64)
    return S.astype(np.float64) @ M64 * inv, (len(Ms) + 4) * EPS * inv * (np.abs(S).astype(np.float64) @ M64)


class _Views(object):
    """A raw fp32 buffer ``[m][Hp][Wp][Cp]``: random data in the real extent and real channels, NaN everywhere
    else (never read); a NaN-filled staging tensor of ``rows`` rows with a NaN guard tail."""

    def __init__(self, real, stored, dtype, rows=ROWS):
        (self.Hr, self.Wr, self.C), (self.Hp, self.Wp, self.Cp) = real, stored
        self.rows, self.dtype = rows, dtype
        rng = np.random.default_rng(self.Hr)
        self.data = rng.standard_normal((M,) + real).astype(np.float32)
        self.fillv = np.array([0.5, -1.0, 0.25], np.float32)[:self.C]
        raw = np.full((M,) + stored, np.nan, np.float32)
        raw[:, :self.Hr, :self.Wr, :self.C] = self.data
        fill = np.full(self.Cp, np.nan, np.float32)
        fill[:self.C] = self.fillv
        self.raw, self.fill = torch.from_numpy(raw).to(_dev()), torch.from_numpy(fill).to(_dev())
        self.img = self.Hp * self.Wp * self.Cp
        self.out = torch.full((rows * self.img + GUARD,), float("nan"), dtype=dtype, device=_dev())
        self.nan_bits = _bits(self.out)[0].item()

    def launch(self, cells, w0=0, base=0, over=()):
        a = _K().RiseViewArgs()
        a.raw, a.out, a.fill = self.raw.data_ptr(), self.out.data_ptr(), self.fill.data_ptr()
        a.m, a.w0, a.masks, a.cells, a.seed, a.thr = M, w0, NMASK, cells, SEED, _thr(P)
        a.rows = a.cap = self.rows
        a.Hp, a.Wp, a.Hr, a.Wr, a.Cp, a.Cr = self.Hp, self.Wp, self.Hr, self.Wr, self.Cp, self.C
        a.prec, a.base = 1 if self.dtype == torch.float32 else 0, base
        self.out.fill_(float("nan"))
        rc = _K().lib().gt_rise_views(_set(a, over), _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self, start=0):
        return bool((_bits(self.out[start:]) == self.nan_bits).all().item())

    def check(self, cells, w0, base):
        Ms = R.masks(self.Hr, self.Wr, NMASK, cells, P, SEED)
        want = np.zeros((self.rows, self.Hp, self.Wp, self.Cp), np.float32)
        for j in range(self.rows):
            w = j if base else w0 + j
            if w < (M if base else M * NMASK):
                r, i = (w, None) if base else divmod(w, NMASK)
                want[j] = R.view(self.data[r], None if base else Ms[i], self.fillv, (self.Hp, self.Wp, self.Cp))
        n = self.rows * self.img
        want = torch.from_numpy(want).to(self.dtype).reshape(-1)
        assert torch.equal(_bits(self.out[:n].cpu()), _bits(want)), (cells, w0, base)
        assert self.untouched(n)                         # the guard past `rows`


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_views_kernel_equals_the_oracle(geom, dtype):
    real, stored = GEOMETRIES[geom]
    c = _Views(real, stored, dtype)
    for cells in (2, 7 if geom != "odd" else 3, min(16, real[0], real[1])):
        assert c.launch(cells, base=1, w0=5) == 0        # base mode: m < rows, w0 is not read
        c.check(cells, 0, True)
        for w0 in (0, NMASK - 4, M * NMASK - 3, M * NMASK):      # straddles images 0 | 1; ends mid-image; past the end
            assert c.launch(cells, w0=w0) == 0
            c.check(cells, w0, False)


@pytest.mark.parametrize("H, W, cells, masks", [(6, 5, 2, 33), (28, 28, 7, 8), (32, 32, 16, 5)])
def test_mask_planes_sum_to_the_oracles_masks(H, W, cells, masks):
    Kp, Pp = (masks + 31) // 32 * 32, (H * W + 63) // 64 * 64
    planes = torch.full((3, Pp, Kp), float("nan"), dtype=torch.bfloat16, device=_dev())
    a = _K().RiseMaskArgs()
    a.planes, a.masks, a.Kp, a.cells, a.seed, a.thr = planes.data_ptr(), masks, Kp, cells, SEED, _thr(0.3)
    a.Hr, a.Wr, a.Pp = H, W, Pp
    for over in (dict(planes=0), dict(masks=0), dict(masks=8193), dict(Kp=Kp + 32), dict(cells=1), dict(cells=17),
                 dict(cells=min(H, W) + 1), dict(Pp=Pp + 64), dict(Hr=0)):
        b = _K().RiseMaskArgs.from_buffer_copy(a)
        assert _K().lib().gt_rise_masks(_set(b, over), _stream()) < 0, over
    torch.cuda.synchronize()
    assert torch.isnan(planes).all()                     # a refusal launches nothing
    assert _K().lib().gt_rise_masks(a, _stream()) == 0
    p = planes.cpu().float().numpy()
    got = (p[0] + p[1]) + p[2]                           # exact: the planes are a split of an fp32 value
    want = np.zeros((Pp, Kp), np.float32)
    want[:H * W, :masks] = R.masks(H, W, masks, cells, 0.3, SEED).reshape(masks, -1).T
    assert got.tobytes() == want.tobytes() and not p[:, H * W:].any() and not p[:, :, masks:].any()


HM, HK, HB = 5, 13, 32       # 65 items: launches from 0, 20 (mid-image 1) and 64 (one live row)


@pytest.mark.parametrize("G", [1, 3, 64])
def test_head_rise_kernel(G):
    C, nt, Kp = 10, 68, 32
    rng = np.random.default_rng(G)
    plog = torch.from_numpy(rng.standard_normal((G, nt, HB, C)).astype(np.float32)).to(_dev())
    b2 = torch.from_numpy(rng.standard_normal((G, C)).astype(np.float32)).to(_dev())
    w = rng.random(G) + 0.1
    w = (w / w.sum()).astype(np.float32) if G > 1 else np.ones(1, np.float32)
    row_logits, row_proba = F._head_predict(plog, b2)
    t = rng.integers(0, C, HM)
    tgt, dw = torch.from_numpy(t.astype(np.int32)).to(_dev()), torch.from_numpy(w).to(_dev())
    for logit in ((0, 1) if G == 1 else (0,)):
        score = row_logits[0] if logit else E._ordered_combine(row_proba, w)[0]
        for w0 in (0, 20, 64):
            S = torch.full((HM, Kp), float("nan"), device=_dev())
            a = _K().HeadRiseArgs()
            a.plog, a.b2, a.weight, a.tgt, a.S = (v.data_ptr() for v in (plog, b2, dw, tgt, S))
            a.G, a.B, a.Up, a.C, a.m, a.masks, a.Kp, a.w0, a.logit = G, HB, nt * 16, C, HM, HK, Kp, w0, logit
            for over in (dict(S=0), dict(tgt=0), dict(G=65), dict(C=17), dict(Up=24), dict(m=0), dict(masks=0),
                         dict(Kp=64), dict(w0=-1), dict(w0=HM * HK), dict(logit=2), dict(m=2 ** 20, masks=8192, Kp=8192)):
                b = _K().HeadRiseArgs.from_buffer_copy(a)
                assert _K().lib().gt_head_rise(_set(b, over), _stream()) < 0, over
            if G > 1:
                a.logit = 1
                assert _K().lib().gt_head_rise(a, _stream()) < 0             # the logit score with several members
                a.logit = 0
            torch.cuda.synchronize()
            assert torch.isnan(S).all()
            assert _K().lib().gt_head_rise(a, _stream()) == 0
            live = min(HB, HM * HK - w0)
            items = w0 + np.arange(live)
            want = np.full((HM, Kp), np.nan, np.float32)
            want[items // HK, items % HK] = score[np.arange(live), t[items // HK]]
            assert S.cpu().numpy().tobytes() == want.tobytes(), (G, logit, w0)   # padding and other items: untouched


_PLANES, WORST = {}, [0.0]


def _planes(H, W, masks):
    """``(planes on the device, masks [K, H, W] by the numpy twin)`` of one setting (cells 2, p 0.5), once."""
    if (H, W, masks) not in _PLANES:
        from gentun_amd.models.cnn_fitted import rise_masks
        Kp, Pp = (masks + 31) // 32 * 32, (H * W + 63) // 64 * 64
        planes = torch.empty((3, Pp, Kp), dtype=torch.bfloat16, device=_dev())
        a = _K().RiseMaskArgs()
        a.planes, a.masks, a.Kp, a.cells, a.seed, a.thr = planes.data_ptr(), masks, Kp, 2, SEED, _thr(P)
        a.Hr, a.Wr, a.Pp = H, W, Pp
        assert _K().lib().gt_rise_masks(a, _stream()) == 0
        _PLANES[(H, W, masks)] = (planes, rise_masks((H, W, 1), masks, 2, P, SEED))
    return _PLANES[(H, W, masks)]


@pytest.mark.parametrize("H, W", [(6, 5), (28, 28), (32, 32)])
@pytest.mark.parametrize("masks", [1, 31, 32, 33, 2048])
def test_accumulate_against_fp64(masks, H, W):
    planes, Ms = _planes(H, W, masks)
    Kp, Pn, Pp = planes.shape[2], H * W, planes.shape[1]
    for m in (1, 17, 33):
        rng = np.random.default_rng(masks + m)
        S = np.full((m + 3, Kp), np.nan, np.float32)     # rows >= m: NaN, never read
        S[:m] = 0
        S[:m, :masks] = rng.standard_normal((m, masks)) * 10.0 ** rng.integers(-3, 3, (m, masks))
        dS = torch.from_numpy(S).to(_dev())
        out = torch.full((m * Pn + 64,), float("nan"), device=_dev())
        a = _K().RiseAccArgs()
        a.planes, a.S, a.out = planes.data_ptr(), dS.data_ptr(), out.data_ptr()
        a.m, a.masks, a.Kp, a.P, a.Pp = m, masks, Kp, Pn, Pp
        a.inv = float(np.float32(1.0 / (masks * P)))
        for over in (dict(planes=0), dict(S=0), dict(out=0), dict(m=0), dict(masks=0), dict(masks=8193), dict(Kp=Kp + 32),
                     dict(P=0), dict(Pp=Pp + 64), dict(inv=0.0), dict(inv=float("nan"))):
            b = _K().RiseAccArgs.from_buffer_copy(a)
            assert _K().lib().gt_rise_accumulate(_set(b, over), _stream()) < 0, over
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
        assert _K().lib().gt_rise_accumulate(a, _stream()) == 0
        got = out.cpu().numpy()
        ref, bound = _bound(S[:m, :masks], Ms, P)
        err = np.abs(got[:m * Pn].reshape(m, Pn) - ref)
        WORST[0] = max(WORST[0], float((err / np.maximum(bound, 1e-300)).max()))
        print("[cnn-rise] accumulate K={} m={} P={}: worst error / bound {:.3f}".format(masks, m, Pn, WORST[0]))
        assert (err <= bound).all() and np.isnan(got[m * Pn:]).all()


def _end_to_end(obj, predict, xs, n_masks, batch, score="proba"):
    """``rise`` on the GPU: the device scores are ``predict`` of the oracle's views, the map their accumulate."""
    n, (H, W, _) = len(xs), xs.shape[1:]
    fill = [0.5, -1.0, 0.25][:xs.shape[3]]
    Ms = R.masks(H, W, n_masks, 7, P, SEED)
    t = np.argmax(obj.predict(xs, device=_dev(), batch=batch), 1) if score == "proba" else np.arange(n) % obj.classes
    got, info = obj.rise(xs, target=None if score == "proba" else t, masks=n_masks, seed=SEED, fill=fill, score=score,
                         device=_dev(), batch=batch, return_info=True)
    pred = obj.hip_predictor(_dev(), batch)
    want = predict(R.views(xs, Ms, fill)).reshape(n, n_masks, -1)[np.arange(n), :, t]
    st = [s for k, s in pred._rise.items() if k[0] == n_masks and k[5] == score][0]
    assert st.scores.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(info["target"], t) and info["base"].tobytes() == predict(xs)[np.arange(n), t].tobytes()
    ref, bound = _bound(want, Ms, P)
    assert got.shape == (n, H, W) and (np.abs(got.reshape(n, -1) - ref) <= bound).all()
    return pred


@pytest.mark.parametrize("n, n_masks, batch", [(3, 96, 32), (2, 300, 256)])
@pytest.mark.parametrize("case", ["chain", "mnist", "bn", "bf16"])
def test_rise_scores_and_map_of_a_classifier(case, n, n_masks, batch):
    m, job, clf, x, lab = F._fit(case)
    xs = x[10:10 + n]
    before = [clf.predict(x[:70], device=_dev(), output="logits", batch=batch),
              clf.occlusion(xs, patch=8, device=_dev(), batch=batch), clf.saliency(xs, device=_dev(), batch=batch)]
    for score, output in (("proba", "proba"), ("logit", "logits")):
        _end_to_end(clf, lambda im: clf.predict(im, device=_dev(), output=output, batch=batch), xs, n_masks, batch, score)
    after = [clf.predict(x[:70], device=_dev(), output="logits", batch=batch),
             clf.occlusion(xs, patch=8, device=_dev(), batch=batch), clf.saliency(xs, device=_dev(), batch=batch)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


@pytest.mark.parametrize("case", list(E.CASES) + ["sixteen"])
def test_rise_of_an_ensemble(case):
    if case == "sixteen":                               # the 16-member fit of tests/test_cnn_occlusion_gpu.py, shared
        import test_cnn_occlusion_gpu as O
        import test_cnn_tta_gpu as T
        from gentun_amd.models import fit_ensemble
        x, y, _ = E._data(*E.CASES["rgb"][:2])
        if "ens" not in O._SIXTEEN:
            O._SIXTEEN["ens"] = fit_ensemble(x, y, T._genomes16(), device=_dev(), **E._space("rgb"))
        ens = O._SIXTEEN["ens"]
    else:
        ens, x = E._fit(case)[:2]
    pred = _end_to_end(ens, lambda im: ens.predict(im, device=_dev(), batch=256), x[10:13], 96, 256)
    assert pred.EB < 256 or case != "sixteen"            # 16 groups: fewer rows per launch, items still straddle
    with pytest.raises(ValueError):
        ens.rise(x[:2], score="logit", device=_dev())


def test_cross_validate_is_unchanged_and_17_classes_are_refused():
    from gentun_amd.models.cnn import GeneticCnnModel
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    m.fit()
    assert m.rise(x[:2], masks=40).shape == (2,) + x.shape[1:3]          # the model forwards to the classifier
    assert m.cross_validate() == first
    xs, y, _ = F._noise_data((8, 8, 3), 17, n=64)
    kw = dict(nodes=(3,), input_shape=(8, 8, 3), kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
              dropout_probability=0.5, classes=17, nfold=2, epochs=(1,), learning_rate=(1e-3,), batch_size=32)
    clf = GeneticCnnModel(xs, y, {"S_1": "101"}, backend="torch", device="cpu", **kw).fit()
    assert clf.rise(xs[:2], masks=8, device=_dev(), backend="torch").shape == (2, 8, 8)
    with pytest.raises(ValueError, match="16 classes"):
        clf.rise(xs[:2], masks=8, device=_dev())


def test_views_launcher_refusals():
    c = _Views((6, 5, 3), (8, 8, 8), torch.float32)
    assert c.launch(2) == 0 and not c.untouched()                         # the accepted call does write
    assert _K().lib().gt_rise_views(None, _stream()) < 0
    for kw in (dict(raw=0), dict(out=0), dict(fill=0), dict(Cp=12), dict(Cp=0), dict(Hr=9), dict(Wr=9), dict(Hr=0),
               dict(Cr=0), dict(Cr=9), dict(masks=0), dict(masks=8193), dict(cells=1), dict(cells=6), dict(cells=17),
               dict(m=0), dict(w0=-1), dict(rows=0), dict(rows=ROWS + 1), dict(cap=ROWS - 1), dict(prec=2),
               dict(base=2), dict(w0=2 ** 31 - 1), dict(m=2 ** 20, masks=8192),
               dict(Hp=2 ** 15, Wp=2 ** 15, Cp=2 ** 15)):
        assert c.launch(2, over=kw) < 0, kw
        assert c.untouched(), kw
