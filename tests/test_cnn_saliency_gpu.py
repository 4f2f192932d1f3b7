"""Saliency on the MI355X: ``gt_conv_in_dgrad`` inside the fp32 accumulation bound of an fp64 loop, the small kernels
byte-equal to fp32 numpy formulas written out here, ``saliency(device=cuda)`` end to end (the Grad-CAM tests' fits)."""

import ctypes

import numpy as np
import pytest
import torch

import gradcam_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F
import test_cnn_gradcam_gpu as GC
from test_cnn_gradcam_gpu import _dev, _f32, _stream

pytestmark = pytest.mark.gpu
GUARD, B = 512, 64


def _run(name, **fields):          # launch gt_<name> with its struct filled from fields; the return code
    from gentun_amd.ops import cnn_kernels as K
    a = getattr(K, "".join(p.title() for p in name.split("_")) + "Args")()
    for k, v in fields.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    rc = getattr(K.lib(), "gt_" + name)(a, _stream())
    torch.cuda.synchronize()
    return rc


def _dev_t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=_dev(), dtype=dtype)


def _nan(n):
    return torch.full((n,), float("nan"), device=_dev())


def _pad_nan(a, Hr, Wr, Cr):
    a[..., Hr:, :, :], a[..., :, Wr:, :], a[..., Cr:] = np.nan, np.nan, np.nan
    return a


def _conv_ref(dz, w, Hr, Wr, Cout, Cr):
    """fp64 ``(dx, sum |dz| |w|)`` ``[G, m, Hp, Wp, Cr]``, tap by tap over the real extent; zero at padded pixels."""
    G, m, Hp, Wp, _ = dz.shape
    KH, KW = w.shape[2:4]
    ph, pw = KH // 2, KW // 2
    d = np.zeros((G, m, Hp + 2 * ph, Wp + 2 * pw, Cout))
    d[:, :, ph:ph + Hr, pw:pw + Wr] = dz[:, :, :Hr, :Wr, :Cout].astype(np.float64)
    out, mag = np.zeros((G, m, Hp, Wp, Cr)), np.zeros((G, m, Hp, Wp, Cr))
    for kh in range(KH):
        for kw in range(KW):
            sh = d[:, :, 2 * ph - kh:2 * ph - kh + Hp, 2 * pw - kw:2 * pw - kw + Wp]     # dz[i + ph - kh][j + pw - kw]
            wk = w[:, :Cout, kh, kw, :Cr].astype(np.float64)
            out += np.einsum("gbijo,goc->gbijc", sh, wk)
            mag += np.einsum("gbijo,goc->gbijc", np.abs(sh), np.abs(wk))
    for a in (out, mag):
        a[:, :, Hr:], a[:, :, :, Wr:] = 0.0, 0.0
    return out, mag


def _conv_case(geom, k, prec, Cr, Cout, G, rows, seed=0):
    Hp, Wp, Hr, Wr = geom
    Coutp = (Cout + 7) // 8 * 8
    rng = np.random.default_rng(seed)
    dz = _dev_t(_pad_nan(rng.standard_normal((G, rows, Hp, Wp, Coutp)).astype(np.float32), Hr, Wr, Cout),
                torch.float32 if prec else torch.bfloat16)
    wh = (rng.standard_normal((G, Coutp, k, k, 8)) * 0.1).astype(np.float32)
    wh[..., Cr:] = np.nan
    args = dict(dz=dz, w=_dev_t(wh), G=G, B=rows, Hp=Hp, Wp=Wp, Hr=Hr, Wr=Wr, Coutp=Coutp, Cout=Cout, C8=8, Cr=Cr,
                KH=k, KW=k, prec=prec)
    return dz, wh, args


@pytest.mark.parametrize("prec", [1, 0], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cout", [16, 20, 64])           # padded to 16, 24 and 64: one and two k-steps
@pytest.mark.parametrize("Cr", [1, 3])
@pytest.mark.parametrize("k", [5, 3])
@pytest.mark.parametrize("geom", [(8, 8, 6, 5), (32, 32, 28, 28), (32, 32, 32, 32)], ids=["6x5in8", "28in32", "32"])
def test_conv_in_dgrad_kernel(geom, k, Cr, Cout, prec):
    """Per output element ``|dx - dx64| <= (KH * KW * Cout + 4) * 2^-24 * sum |dz| |w|``: the fp32 accumulation
    bound, every product within 2 ulps (common.h). NaN planted in every padding is never read; exact zeros outside the
    real extent; rows >= m and the guard tail untouched; another launch batch and row position give the same bits."""
    Hp, Wp, Hr, Wr = geom
    for G, m in ((1, 33), (3, 1)):
        dz, wh, args = _conv_case(geom, k, prec, Cr, Cout, G, B, seed=k + prec)
        n = G * B * Hp * Wp * 8
        dx = _nan(n + GUARD)
        assert _run("conv_in_dgrad", dx=dx, m=m, **args) == 0
        got = dx.cpu().numpy()
        assert np.isnan(got[n:]).all() and np.isnan(got[:n].reshape(G, B, -1)[:, m:]).all()
        got = got[:n].reshape(G, B, Hp, Wp, 8)[:, :m]
        want, mag = _conv_ref(_f32(dz)[:, :m], wh, Hr, Wr, Cout, Cr)
        assert np.isfinite(got).all()
        assert not got[:, :, Hr:].any() and not got[:, :, :, Wr:].any() and not got[..., Cr:].any()
        err, bound = np.abs(got[..., :Cr] - want), (k * k * Cout + 4) * 2.0 ** -24 * mag
        print("[cnn-saliency] conv_in_dgrad", G, m, "error / bound", float((err[mag > 0] / bound[mag > 0]).max()))
        assert np.abs(want).max() > 0 and (err <= bound).all()
        dz2 = torch.full((G, m + 1) + tuple(dz.shape[2:]), float("nan"), device=_dev(), dtype=dz.dtype)
        dz2[:, 1:] = dz[:, :m]
        dx2 = _nan(G * (m + 1) * Hp * Wp * 8)
        assert _run("conv_in_dgrad", dx=dx2, m=m + 1, **dict(args, dz=dz2, B=m + 1)) == 0
        assert dx2.cpu().numpy().reshape(G, m + 1, Hp, Wp, 8)[:, 1:].tobytes() == got.tobytes()


@pytest.mark.parametrize("over", [dict(KH=7, KW=7), dict(KW=3), dict(Wp=12), dict(Cr=4), dict(Coutp=72), dict(Coutp=20),
                                  dict(m=B + 1), dict(m=0), dict(C8=16), dict(prec=2), dict(Hr=9), dict(dz=0)], ids=str)
def test_conv_in_dgrad_refusals(over):
    dz, wh, args = _conv_case((8, 8, 6, 5), 5, 1, 3, 20, 1, B)
    dx = _nan(B * 8 * 8 * 8)
    assert _run("conv_in_dgrad", **dict(dict(args, dx=dx, m=2), **over)) != 0 and torch.isnan(dx).all()


@pytest.mark.parametrize("logit", [1, 0], ids=["logit", "proba"])
@pytest.mark.parametrize("C", [1, 2, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("G", [1, 3])
def test_head_saliency_kernel(G, dtype, C, logit):
    """``tgt`` / ``base`` byte-equal to ``gt_head_gradcam``'s; ``dH`` byte-equal to phase (b) of gradcam_ref.head_twin
    (which keeps its ``dH`` to itself, so its lines are repeated here), its bf16 planes the exact split."""
    cam = GC._Cam(G, 5, C, GC.GEOMS[0], dtype, seed=G)
    w = np.ones(1, np.float32) if G == 1 else np.array([0.5, 0.125, 0.375], np.float32)
    wd, (prec, npl) = _dev_t(w), ((1, 3) if dtype == torch.float32 else (0, 1))
    for m, given in ((B, False), (37, True), (37, False)):
        tgt = (np.arange(m) * 5 % C) if given else np.full(m, -1)
        cam.fresh(tgt)
        assert cam.launch(wd, m, logit, 1) == 0
        t_cam, base_cam = cam.tgt.cpu().numpy()[:m], cam.base.cpu().numpy()[:m]
        tg = torch.full((B,), -1, dtype=torch.int32, device=_dev())
        tg[:m] = _dev_t(tgt.astype(np.int32), torch.int32)
        base, dH = _nan(B), _nan(G * B * cam.Up)
        dHp = torch.full((npl, G, B, cam.Up), 0x7fc0, dtype=torch.int16, device=_dev())
        args = dict(plog=cam.plog, b2=cam.b2, weight=wd, hid=cam.hid, w2=cam.W2, tgt=tg, base=base, dH=dH, dHp=dHp,
                    G=G, B=B, Up=cam.Up, C=C, m=m, prec=prec, logit=logit)
        assert _run("head_saliency", **args) == 0
        assert np.array_equal(tg.cpu().numpy()[:m], t_cam) and base.cpu().numpy()[:m].tobytes() == base_cam.tobytes()
        assert torch.isnan(base[m:]).all()
        p, hid, W2 = cam.proba[:, :m], cam.host[1][:, :m], cam.host[2]
        hot = (np.arange(C)[None, :] == t_cam[:, None]).astype(np.float32)
        want = np.zeros((G, B, cam.Up), np.float32)
        for g in range(G):
            coef = hot if logit else p[g][np.arange(m), t_cam][:, None] * (hot - p[g])
            acc = coef[:, None, 0] * W2[g][None, :, 0]
            for c in range(1, C):
                acc = acc + coef[:, None, c] * W2[g][None, :, c]
            want[g, :m] = np.where(hid[g].view(np.int32) > 0, acc, np.float32(0))
        assert dH.cpu().numpy().tobytes() == want.tobytes()
        planes = dHp.view(torch.bfloat16).float().cpu().numpy()
        assert not prec or np.array_equal(planes.sum(0, dtype=np.float64), want)            # exact (-0 sums to +0)
        assert planes[0].tobytes() == torch.from_numpy(want).to(torch.bfloat16).float().numpy().tobytes()


GEOMS, DTYPES = [(8, 8, 6, 5), (32, 32, 28, 28)], [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=["6x5in8", "28in32"])
def test_bn_bwd_eval_kernel(geom, dtype):
    from gentun_amd.ops.cnn_kernels import bn_chunk_px
    Hp, Wp, Hr, Wr = geom
    G, rows, Cp, Cr, eps = 2, 3, 24, 20, np.float32(1e-3)
    rng = np.random.default_rng(0)
    dy = _dev_t(rng.standard_normal((G, rows, Hp, Wp, Cp)).astype(np.float32), dtype)
    buf = torch.cat([dy.reshape(-1), torch.full((GUARD,), float("nan"), device=_dev(), dtype=dtype)])
    gamma = rng.standard_normal((G, Cp)).astype(np.float32)
    run = np.stack([rng.standard_normal((G, Cp)), rng.uniform(0.5, 2.0, (G, Cp))]).astype(np.float32)
    chunk = bn_chunk_px(Hp, Wp, Cp)
    args = dict(dy=buf, gamma=_dev_t(gamma), run=_dev_t(run), G=G, B=rows, H=Hp, W=Wp, Hr=Hr, Wr=Wr, Cp=Cp, Cr=Cr,
                chunk_px=chunk, nchunk=-(-(rows * Hp * Wp) // chunk), eps=float(eps), prec=int(dtype == torch.float32))
    assert _run("bn_bwd_eval", **args) == 0
    want = _f32(dy) * (gamma * (np.float32(1) / np.sqrt(run[1] + eps)))[:, None, None, None, :]
    want[:, :, Hr:], want[:, :, :, Wr:], want[..., Cr:] = 0, 0, 0
    n = dy.numel()
    assert _f32(buf[:n]).tobytes() == _f32(_dev_t(want.reshape(-1), dtype)).tobytes() and torch.isnan(buf[n:]).all()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("m,Rr", [(1, 3), (4, 1), (4, 3)])
@pytest.mark.parametrize("Cr", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=["6x5in8", "28in32"])
def test_ig_kernels(geom, dtype, Cr, m, Rr, G):
    """The points, then per method the ordered sum over k, ``* (1/m)``, ``* (x - x0)`` (or ``* x``), the ordered mean of
    the members and the channel reduction: fp32 numpy, one rounding per operation. Spare rows and padding untouched."""
    Hp, Wp, Hr, Wr = geom
    prec, rows, f1 = int(dtype == torch.float32), m * Rr + 2, np.float32(1)
    rng = np.random.default_rng(1)
    x = _dev_t(rng.standard_normal((Rr, Hp, Wp, 8)).astype(np.float32), dtype)
    x0h = np.zeros(8, np.float32)
    x0h[:Cr] = _f32(_dev_t(rng.standard_normal(Cr).astype(np.float32), dtype))
    x0, stage = _dev_t(x0h), torch.full((rows, Hp, Wp, 8), float("nan"), device=_dev(), dtype=dtype)
    alpha = ((np.arange(m) + 0.5) / m).astype(np.float32)
    img = dict(Hp=Hp, Wp=Wp, Hr=Hr, Wr=Wr, Cr=Cr, prec=prec)
    pargs = dict(raw=x, out=stage, x0=x0, R=Rr, m=m, rows=rows, alpha=(ctypes.c_float * 64)(*alpha), **img)
    assert _run("ig_points", **pargs) == 0
    xh, b = _f32(x)[:, :Hr, :Wr, :Cr], x0h[:Cr]
    pts = np.concatenate([b + al * (xh - b) for al in alpha])
    got = _f32(stage)
    assert got[:m * Rr, :Hr, :Wr, :Cr].tobytes() == _f32(_dev_t(pts, dtype)).tobytes()
    got[:m * Rr, :Hr, :Wr, :Cr] = np.nan
    assert np.isnan(got).all()
    dxh = _pad_nan(rng.standard_normal((G, rows, Hp, Wp, 8)).astype(np.float32), Hr, Wr, Cr)
    wh = (np.ones(1) if G == 1 else np.array([0.5, 0.125, 0.375])).astype(np.float32)
    rargs = dict(dx=_dev_t(dxh), x=x, x0=x0, weight=_dev_t(wh), G=G, B=rows, R=Rr, **img)
    for method, reduce in [(a, r) for a in range(3) for r in range(3)]:
        mm = m if method == 2 else 1
        per = Hr * Wr * (Cr if reduce == 0 else 1)
        out = _nan(Rr * per + GUARD)
        assert _run("ig_reduce", out=out, m=mm, method=method, reduce=reduce, inv_m=float(f1 / np.float32(mm)),
                    **rargs) == 0
        v = None
        for g in range(G):
            s = dxh[g, :Rr, :Hr, :Wr, :Cr]
            for kk in range(1, mm):
                s = s + dxh[g, kk * Rr:(kk + 1) * Rr, :Hr, :Wr, :Cr]
            a = (s, xh * s, (xh - b) * (s * (f1 / np.float32(mm))))[method]
            v = wh[g] * a if g == 0 else v + wh[g] * a
        if reduce == 2:
            v = v[..., 0] if Cr == 1 else (v[..., 0] + v[..., 1]) + v[..., 2]
        want = np.abs(v).max(3) if reduce == 1 else v
        got = out.cpu().numpy()
        assert got[:Rr * per].tobytes() == want.tobytes() and np.isnan(got[Rr * per:]).all(), (method, reduce)


NROWS = 64


@pytest.mark.parametrize("case", ["chain", "mnist", "bn", "bf16"])
def test_gradient_against_the_fp64_autograd_gradient(case):
    """64 images. Batch 32 = batch 256; the masked forward leaves the plain forward's activations; fp32 fits: per
    image ``e = max |g - g64| / max |g64|`` against ``_torch_saliency(dtype=float64)``: ``median(e_hip) <= 4 *
    median(e_torch)`` (the factor of the logits and the Grad-CAM maps) and at most 8 images with ``e_hip > 100 *
    median(e_torch)`` (a ReLU or max-pool decision that flips between precisions moves a gradient discontinuously).
    The bf16 fit's figures are printed, not asserted."""
    m, job, clf, x, lab = F._fit(case)
    xs = x[10:10 + NROWS]
    t = clf.predict(xs, device=_dev(), output="label")
    hip, info = clf.saliency(xs, target=t, reduce=None, device=_dev(), batch=256, return_info=True)
    assert hip.dtype == np.float32 and np.isfinite(hip).all() and np.array_equal(info["target"], t)
    assert clf.saliency(xs, target=t, reduce=None, device=_dev(), batch=32).tobytes() == hip.tobytes()
    assert info["base"].tobytes() == clf.predict(xs, device=_dev(), output="logits")[np.arange(NROWS), t].tobytes()
    pred = clf.hip_predictor(_dev(), 256)                # the masked forward against the plain one, same buffers
    (hs, ws), Cp = pred.job.final_hw, pred.job.final_cp
    with torch.cuda.device(_dev()):
        pred.upload(xs)
        pred.forward()
        torch.cuda.synchronize()
        feat = GC._buffer(pred, pred.df.x, (1, pred.EB, hs, ws, Cp))
        hid = GC._buffer(pred, pred.df.out, (1, pred.EB, pred.job.Up))
        plain = (feat.clone(), hid.clone())
        feat.zero_(), hid.zero_()
        pred._sal.forward(pred, NROWS, 1)
        torch.cuda.synchronize()
        assert torch.equal(feat, plain[0]) and torch.equal(hid, plain[1]) and feat.abs().max() > 0
    ref = clf._torch_saliency(xs, t, "logit", "gradient", 1, np.zeros(xs.shape[3], "f4"), torch.device("cpu"), 256,
                              torch.float64)[0]
    t32 = clf.saliency(xs, target=t, reduce=None, device=_dev(), backend="torch")
    scale = np.abs(ref).max((1, 2, 3))
    e_hip, e_torch = np.abs(hip - ref).max((1, 2, 3)) / scale, np.abs(t32 - ref).max((1, 2, 3)) / scale
    med_h, med_t = float(np.median(e_hip)), float(np.median(e_torch))
    out_h, out_t = int((e_hip > 100 * med_t).sum()), int((e_torch > 100 * med_t).sum())
    print("[cnn-saliency] {} gradient vs fp64: median e HIP {:.3e}, torch fp32 (GPU) {:.3e}; outliers HIP {}, torch {}"
          .format(case, med_h, med_t, out_h, out_t))
    assert scale.min() > 0 and (case == "bf16" or (med_h <= 4 * med_t and out_h <= 8))


def test_integrated_is_the_formula_of_the_points_gradients():
    """Byte-equal to the written-out formula over ``"gradient"`` maps of the points; 70 images: a short last chunk."""
    m, job, clf, x, lab = F._fit("chain")
    xs, f1 = x[10:80], np.float32(1)
    x0 = np.array([0.25, 0.0, -0.5], np.float32)
    got, info = clf.saliency(xs, method="integrated", steps=4, baseline=x0, score="proba", reduce="sum",
                             device=_dev(), return_info=True)
    t = info["target"]
    assert np.array_equal(t, clf.predict(xs, device=_dev(), output="label"))
    s = None
    for al in ((np.arange(4) + 0.5) / 4).astype(np.float32):
        g = clf.saliency(x0 + al * (xs - x0), target=t, score="proba", reduce=None, device=_dev())
        s = g if s is None else s + g
    a = (xs - x0) * (s * (f1 / np.float32(4)))
    assert got.tobytes() == ((a[..., 0] + a[..., 1]) + a[..., 2]).tobytes() and np.abs(got).max() > 0
    proba = clf.predict(np.concatenate([xs, np.broadcast_to(x0, (1,) + xs.shape[1:])]), device=_dev())
    assert info["base"].tobytes() == proba[np.arange(70), t].tobytes()
    assert info["baseline_score"].tobytes() == proba[70][t].tobytes()


def test_ensemble_of_three_and_the_other_paths_are_unchanged():
    """Byte-equal to the ordered combine of its members' own predictors; the other paths' bytes stay."""
    ens, x, y, lab = E._fit("rgb")
    xs, mem = x[10:50], ens.members[0]

    def others():
        return [ens.predict(xs, device=_dev()), mem.predict(xs, device=_dev(), output="logits"),
                mem.gradcam(xs, device=_dev()), mem.occlusion(xs[:3], patch=8, device=_dev())]
    before = others()
    pred = ens.hip_predictor(_dev(), 256)
    for score, method in (("proba", "gradient"), ("logit", "integrated")):
        kw = dict(score=score, method=method, steps=3, device=_dev(), return_info=True)
        got, info = ens.saliency(xs, reduce="absmax", **kw)
        assert np.array_equal(info["target"], ens.predict(xs, device=_dev(), output="label"))
        per = [mm.saliency(xs, target=info["target"], reduce=None, batch=pred.EB, **kw) for mm in ens.members]
        want = np.abs(R.ordered_mean(ens.weights, np.stack([p[0] for p in per]))).max(3)
        assert got.tobytes() == want.tobytes() and np.abs(got).max() > 0, (score, method)
        assert info["base"].tobytes() == R.ordered_mean(ens.weights, np.stack([p[1]["base"] for p in per])).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, others()))


def test_cross_validate_is_unchanged_and_more_than_16_classes_are_refused():
    from gentun_amd.models.cnn import GeneticCnnModel
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    m.fit()
    assert m.saliency(x[:4]).shape == (4, 28, 28)            # the model forwards to the classifier
    assert m.cross_validate() == first
    shape, classes = (8, 8, 3), 17
    x, y, lab = F._noise_data(shape, classes, n=64)
    kw = dict(nodes=(3,), input_shape=shape, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
              dropout_probability=0.5, classes=classes, nfold=2, epochs=(1,), learning_rate=(1e-3,), batch_size=32)
    clf = GeneticCnnModel(x, y, {"S_1": "101"}, backend="torch", device="cpu", **kw).fit()
    with pytest.raises(ValueError, match="16 classes"):
        clf.saliency(x[:4], device=_dev())
