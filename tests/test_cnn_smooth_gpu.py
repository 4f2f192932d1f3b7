"""``saliency(smooth=...)`` on the MI355X: ``gt_sg_points`` against the fp64 twin inside a bound measured on the
reference, ``gt_sg_reduce`` byte-equal to the fp32 numpy formula, ``saliency(device=cuda, smooth=...)`` end to end
(the saliency tests' fits and helpers)."""

import numpy as np
import pytest
import torch

import gradcam_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F
from test_cnn_gradcam_gpu import _dev, _f32
from test_cnn_saliency_gpu import GUARD, _dev_t, _nan, _pad_nan, _run
from test_cnn_smooth import _finish

pytestmark = pytest.mark.gpu
GEOMS = [(32, 32, 32, 32, 3), (32, 32, 28, 28, 1), (8, 8, 6, 5, 3)]
GIDS = ["32x32x3", "28x28x1in32", "6x5x3in8"]
DTYPES = [torch.float32, torch.bfloat16]
SEED, N0 = 11, 37


def _z32_error(z64, n, S, Hr, Wr, Cr):
    """The largest ``|z32 - z64|`` of the same draws with the formula evaluated in numpy fp32: the reference's own
    error, which scales the bound of the kernel."""
    from gentun_amd.utils.rng import SG_KEY, hash4
    d = ((np.arange(Hr * Wr, dtype=np.uint64)[:, None] * np.uint64(4) + np.arange(Cr, dtype=np.uint64)) * np.uint64(2))
    nn, k = np.asarray(n, np.uint64).reshape(-1, 1, 1, 1), np.arange(S, dtype=np.uint64).reshape(1, -1, 1, 1)
    u = [(((hash4(SEED ^ SG_KEY, nn, k, d + np.uint64(j)) >> np.uint64(9)) * np.uint64(2) + np.uint64(1))
          .astype(np.float32) * np.float32(2.0 ** -24)) for j in range(2)]
    z32 = np.sqrt(np.float32(-2) * np.log(u[0])) * np.cos(np.float32(2 * np.pi) * u[1])
    assert z32.dtype == np.float32
    return float(np.abs(z32.reshape(z64.shape) - z64).max())


@pytest.mark.parametrize("S,Rr", [(1, 1), (3, 2), (64, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=GIDS)
def test_sg_points_kernel(geom, dtype, S, Rr):
    """``|x_dev - x64| <= 4 e_ref sigma + u |x64|`` with ``e_ref`` the largest error of the fp32 numpy evaluation of
    the same draws against fp64 and ``u`` the unit roundoff of the staging type (2^-24, 2^-8): measured on an MI355X
    ``e_ref`` 9.1e-07 to 1.6e-06 and, in fp32 staging, ``(err - u |x64|) / sigma`` at most 4.9e-07 (profiles/
    cnn_smoothgrad.txt). Spare rows, padding and the guard tail keep their NaN; NaN in the raw padding is not used;
    ``sigma = 0`` copies the raw rows byte for byte."""
    from gentun_amd.utils.rng import sg_noise
    Hp, Wp, Hr, Wr, Cr = geom
    prec, rows = int(dtype == torch.float32), S * Rr + 2
    rng = np.random.default_rng(S)
    x = _dev_t(_pad_nan(rng.standard_normal((Rr, Hp, Wp, 8)).astype(np.float32), Hr, Wr, Cr), dtype)
    xh = _f32(x)[:, :Hr, :Wr, :Cr]
    sig = rng.uniform(0.05, 0.6, Rr).astype(np.float32)
    n = rows * Hp * Wp * 8
    z64 = sg_noise(SEED, N0 + np.arange(Rr), S, Hr, Wr, Cr)                         # [R, S, Hr, Wr, Cr]
    e_ref = _z32_error(z64, N0 + np.arange(Rr), S, Hr, Wr, Cr)
    for sigma in (sig, np.zeros(Rr, np.float32)):
        buf = torch.full((n + GUARD,), float("nan"), device=_dev(), dtype=dtype)
        args = dict(raw=x, out=buf, sigma=_dev_t(sigma), R=Rr, S=S, rows=rows, n0=N0, seed=SEED, Hp=Hp, Wp=Wp, Hr=Hr,
                    Wr=Wr, Cr=Cr, prec=prec)
        assert _run("sg_points", **args) == 0
        got = _f32(buf)
        assert np.isnan(got[n:]).all()
        got = got[:n].reshape(rows, Hp, Wp, 8)
        real = got[:S * Rr, :Hr, :Wr, :Cr].reshape(S, Rr, Hr, Wr, Cr).copy()
        got[:S * Rr, :Hr, :Wr, :Cr] = np.nan
        assert np.isnan(got).all() and np.isfinite(real).all()
        if not sigma.any():
            assert real.tobytes() == np.broadcast_to(xh, real.shape).tobytes()
            continue
        s64 = sigma.astype(np.float64)[:, None, None, None]
        want = (xh.astype(np.float64) + s64 * z64.transpose(1, 0, 2, 3, 4))         # [S, R, Hr, Wr, Cr]
        err = np.abs(real - want)
        bound = 4 * e_ref * s64 + (2.0 ** -24 if prec else 2.0 ** -8) * np.abs(want)
        print("[cnn-smooth] sg_points e_ref {:.3e}; max (err - rounding) / sigma {:.3e}; err / bound {:.3f}".format(
            e_ref, float(((err - (bound - 4 * e_ref * s64)) / s64).max()), float((err / bound).max())))
        assert (err <= bound).all()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("S,Rr", [(1, 1), (5, 3), (64, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS[1:], ids=GIDS[1:])
def test_sg_reduce_kernel(geom, dtype, S, Rr, G):
    """Byte-equal to the ordered fp32 sums, the statistic, the method factor, the ordered mean of the members and the
    channel reduction, for every stat x method x reduce; NaN in the spare rows and the padding is not used."""
    Hp, Wp, Hr, Wr, Cr = geom
    prec, rows = int(dtype == torch.float32), S * Rr + 2
    rng = np.random.default_rng(G)
    x = _dev_t(_pad_nan(rng.standard_normal((Rr, Hp, Wp, 8)).astype(np.float32), Hr, Wr, Cr), dtype)
    xh = _f32(x)[:, :Hr, :Wr, :Cr]
    dxh = _pad_nan(rng.standard_normal((G, rows, Hp, Wp, 8)).astype(np.float32), Hr, Wr, Cr)
    dxh[:, S * Rr:] = np.nan
    wh = (np.ones(1) if G == 1 else np.array([0.5, 0.125, 0.375])).astype(np.float32)
    rargs = dict(dx=_dev_t(dxh), x=x, weight=_dev_t(wh), G=G, B=rows, R=Rr, S=S, Hp=Hp, Wp=Wp, Hr=Hr, Wr=Wr, Cr=Cr,
                 prec=prec, inv_s=float(np.float32(1) / np.float32(S)))
    gs = [[dxh[g, k * Rr:(k + 1) * Rr, :Hr, :Wr, :Cr] for k in range(S)] for g in range(G)]
    for stat, method, reduce in [(s, a, r) for s in range(3) for a in range(2) for r in range(3)]:
        per = Hr * Wr * (Cr if reduce == 0 else 1)
        out = _nan(Rr * per + GUARD)
        assert _run("sg_reduce", out=out, stat=stat, method=method, reduce=reduce, **rargs) == 0
        v = R.ordered_mean(wh, np.stack([_finish(gs[g], xh, ("gradient", "gradxinput")[method],
                                                 ("mean", "sq", "var")[stat]) for g in range(G)]))
        if reduce == 2:
            v = v[..., 0] if Cr == 1 else (v[..., 0] + v[..., 1]) + v[..., 2]
        want = np.abs(v).max(3) if reduce == 1 else v
        got = out.cpu().numpy()
        assert got[:Rr * per].tobytes() == want.tobytes() and np.isnan(got[Rr * per:]).all(), (stat, method, reduce)


REFUSED = [("sg_points", o) for o in (dict(S=0), dict(S=65), dict(R=0), dict(R=3), dict(prec=2), dict(Cr=4), dict(Hr=9),
                                      dict(Wp=0), dict(raw=0), dict(out=0), dict(sigma=0), dict(n0=-1))] + \
          [("sg_reduce", o) for o in (dict(S=0), dict(S=65), dict(R=3), dict(G=0), dict(stat=3), dict(stat=-1),
                                      dict(method=2), dict(reduce=3), dict(prec=-1), dict(Cr=0), dict(Wr=9),
                                      dict(dx=0), dict(x=0), dict(weight=0))]


@pytest.mark.parametrize("name,over", REFUSED, ids=str)
def test_launcher_refusals_launch_nothing(name, over):
    S, Rr, rows = 2, 2, 5                                    # R = 3: S * R = 6 rows do not fit
    img = dict(Hp=8, Wp=8, Hr=6, Wr=5, Cr=3, prec=1)
    x, out = torch.zeros((Rr + 1, 8, 8, 8), device=_dev()), _nan(rows * 8 * 8 * 8)
    if name == "sg_points":
        args = dict(raw=x, out=out, sigma=torch.ones(4, device=_dev()), R=Rr, S=S, rows=rows, n0=0, seed=1, **img)
    else:
        args = dict(dx=torch.ones((1, rows, 8, 8, 8), device=_dev()), x=x, weight=torch.ones(1, device=_dev()), out=out,
                    G=1, B=rows, R=Rr, S=S, stat=0, method=0, reduce=0, inv_s=0.5, **img)
    args.update(over)
    assert _run(name, **args) < 0 and torch.isnan(out).all()


NROWS = 64
SM = {"samples": 4, "noise": 0.1, "seed": 0, "stat": "mean"}


@pytest.mark.parametrize("case", ["chain", "mnist", "bn"])
def test_smoothgrad_against_fp64_autograd_on_the_twins_points(case):
    """64 images, 4 samples, noise 0.1, signed maps. Per image ``e = max |a - a64| / max |a64|`` against the fp64
    autograd result on the twin's points: ``median(e_hip) <= 4 * median(e_torch_fp32)`` and at most 8 images with
    ``e_hip > 100 * median(e_torch)`` (a noisy point on a ReLU or max-pool kink), the images chosen so that the
    torch fp32 run alone stays within that cap. Chunks of 8 and of 64 images (batch 32 and 256) give the same
    bits; target and base are the clean image's."""
    m, job, clf, x, lab = F._fit(case)
    xs = x[10:10 + NROWS]
    t = clf.predict(xs, device=_dev(), output="label")
    hip, info = clf.saliency(xs, reduce=None, device=_dev(), batch=256, smooth=SM, return_info=True)
    assert hip.dtype == np.float32 and np.isfinite(hip).all() and np.array_equal(info["target"], t)
    assert info["base"].tobytes() == clf.predict(xs, device=_dev(), output="logits")[np.arange(NROWS), t].tobytes()
    assert clf.saliency(xs, reduce=None, device=_dev(), batch=32, smooth=SM).tobytes() == hip.tobytes()
    ref = clf._torch_saliency(xs, t, "logit", "gradient", 1, np.zeros(xs.shape[3], "f4"), torch.device("cpu"), 256,
                              torch.float64, (4, np.float32(0.1), 0, "mean"))[0]
    t32 = clf.saliency(xs, target=t, reduce=None, device=_dev(), backend="torch", smooth=SM)
    scale = np.abs(ref).max((1, 2, 3))
    e_hip, e_torch = np.abs(hip - ref).max((1, 2, 3)) / scale, np.abs(t32 - ref).max((1, 2, 3)) / scale
    med_h, med_t = float(np.median(e_hip)), float(np.median(e_torch))
    out_h, out_t = int((e_hip > 100 * med_t).sum()), int((e_torch > 100 * med_t).sum())
    print("[cnn-smooth] {} smoothgrad vs fp64: median e HIP {:.3e}, torch fp32 (GPU) {:.3e}; outliers HIP {}, torch {}"
          .format(case, med_h, med_t, out_h, out_t))
    assert scale.min() > 0 and out_t <= 8 and med_h <= 4 * med_t and out_h <= 8


@pytest.mark.parametrize("samples", [1, 2])
def test_zero_noise_mean_is_the_plain_hip_map(samples):
    m, job, clf, x, lab = F._fit("chain")
    xs = x[10:80]                                            # 70 images: a short last chunk
    for method in ("gradient", "gradxinput"):
        plain = clf.saliency(xs, method=method, reduce="sum", device=_dev())
        got = clf.saliency(xs, method=method, reduce="sum", device=_dev(), batch=64,
                           smooth={"samples": samples, "noise": 0, "stat": "mean"})
        assert got.tobytes() == plain.tobytes() and np.abs(got).max() > 0


def test_ensemble_of_three_and_the_other_paths_are_unchanged():
    """Byte-equal to the ordered combine of its members' own predictors; the other paths' bytes stay."""
    ens, x, y, lab = E._fit("rgb")
    xs, mem = x[10:50], ens.members[0]
    sm = {"samples": 3, "noise": 0.2, "seed": 5, "stat": "var"}

    def others():
        return [ens.predict(xs, device=_dev()), mem.predict(xs, device=_dev(), output="logits"),
                mem.gradcam(xs, device=_dev()), mem.saliency(xs, device=_dev()),
                ens.saliency(xs, method="integrated", steps=3, device=_dev())]
    before = others()
    pred = ens.hip_predictor(_dev(), 256)
    kw = dict(score="proba", method="gradxinput", device=_dev(), smooth=sm, return_info=True)
    got, info = ens.saliency(xs, reduce="absmax", **kw)
    assert np.array_equal(info["target"], ens.predict(xs, device=_dev(), output="label"))
    per = [mm.saliency(xs, target=info["target"], reduce=None, batch=pred.EB, **kw) for mm in ens.members]
    want = np.abs(R.ordered_mean(ens.weights, np.stack([p[0] for p in per]))).max(3)
    assert got.tobytes() == want.tobytes() and np.abs(got).max() > 0
    assert info["base"].tobytes() == R.ordered_mean(ens.weights, np.stack([p[1]["base"] for p in per])).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, others()))


def test_cross_validate_is_unchanged_and_too_many_samples_are_refused():
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    m.fit()
    assert m.saliency(x[:4], smooth={"samples": 2}).shape == (4, 28, 28)     # the model forwards to the classifier
    assert m.cross_validate() == first
    with pytest.raises(ValueError, match="do not fit 32 rows"):
        m.saliency(x[:4], batch=32, smooth={"samples": 33})
