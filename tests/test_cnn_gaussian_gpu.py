"""``gaussian_fit`` / ``mahalanobis`` on an MI355X: the kernels of csrc/hip/cnn_gaussian.hip alone on hand-made
buffers (NaN in padding units, in rows ``>= N`` and in guard tails) against fp64 numpy, then through the HIP
predictors of the fits of tests/test_cnn_fitted_gpu.py and tests/test_cnn_ensemble_gpu.py (shared, left unchanged).

Bounds, ``EPS = 2^-24`` (the project's split-fp32 bound: a length-``n`` product sum is within ``(n + 4) EPS
sum |a_i| |b_i|``):
* scatter entry ``(i, j)``: ``(FS_SLICE_ROWS + 4) EPS sum_r |c_ri| |c_rj|`` -- fp32 sums run over one slice of rows,
  the slices join in fp64.
* distance: ``z_j`` is a length-``Ur`` product sum, so it is within ``e_j = (Ur + 4) EPS sum_i |f_i| |W_ij|`` of the
  exact one. With ``a_j = z_j - t_cj`` exact and ``a_j + x_j``, ``|x_j| <= e_j`` computed, the squares differ by
  ``2 a_j x_j + x_j^2``: at most ``sum_j (2 |a_j| e_j + e_j^2)`` over the columns. The epilogue's own subtraction,
  square and ``Ur`` fp32 additions of non-negative terms add at most ``(Ur + 4) EPS d_c``."""

import numpy as np
import pytest
import torch

import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GUARD, DEV = 256, "cuda:0"
SLICE = 1024                 # FS_SLICE_ROWS (asserted against the library)
WORST = {}


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _nan(n, dtype=torch.float32):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)


def _split(c):
    """The three bf16 planes of an fp32 tensor (common.h split8)."""
    out = []
    for _ in range(3):
        out.append(c.bfloat16())
        c = c - out[-1].float()
    return torch.stack(out)


def _lib():
    from gentun_amd.ops import cnn_kernels as K
    assert K.FS_SLICE_ROWS == SLICE
    return K, K.lib()


def _features(G, N, Ur, C, dtype, seed=0):
    """Non-negative features ``[G, N, Ur]`` with class structure and labels that leave class ``C - 1`` empty."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, max(C - 1, 1), N)
    f = np.maximum(rng.standard_normal((G, N, Ur)) + rng.standard_normal((G, C, Ur))[:, lab], 0).astype(np.float32)
    return _dev(f, dtype).float().cpu().numpy(), lab


def _src(K, s, f, Up, dtype, flat):
    """``f [G, N, Ur]`` as the device buffer of an NnSrc, NaN in padding units and in 3 rows past ``N``."""
    G, N, Ur = f.shape
    if flat:
        buf = np.full((N + 3, G * Ur + 5), np.nan, np.float32)
        buf[:N, :G * Ur] = f.transpose(1, 0, 2).reshape(N, G * Ur)
    else:
        buf = np.full((G, N + 3, Up), np.nan, np.float32)
        buf[:, :N, :Ur] = f
    t = _dev(buf, torch.float32 if flat else dtype)
    s.h, s.G, s.B, s.Up, s.Ur, s.flat, s.ld = t.data_ptr(), G, N + 3, Up, Ur, int(flat), buf.shape[1] if flat else 0
    return t


# (Up, Ur, N, C, G, dtype, flat source): every value of the issue's table -- one tile and a ragged second one, a
# single row, a row tile edge, a second slice of 76 rows, one class and sixteen, one member and three
FIT = [
    (32, 20, 1, 1, 1, torch.float32, False),
    (32, 20, 129, 3, 3, torch.bfloat16, False),
    (32, 20, SLICE + 76, 16, 1, torch.float32, True),
    (160, 130, 1, 3, 1, torch.bfloat16, False),
    (160, 130, 129, 16, 3, torch.float32, True),
    (160, 130, SLICE + 76, 1, 1, torch.float32, False),
    (160, 130, SLICE + 76, 3, 3, torch.bfloat16, False),
]


@pytest.mark.parametrize("case", FIT, ids=lambda c: "-".join(str(v).replace("torch.", "") for v in c))
def test_fit_kernels_against_fp64(case):
    Up, Ur, N, C, G, dtype, flat = case
    K, L = _lib()
    f, lab = _features(G, N, Ur, C, dtype)
    Np, S = -(-N // 64) * 64, -(-N // SLICE)
    a = K.FsSumsArgs()
    keep = _src(K, a.src, f, Up, dtype, flat)
    labd = _dev(lab.astype(np.int32))
    part = _nan(S * G * C * Up, torch.float64)
    a.label, a.part, a.sprec, a.N, a.C = labd.data_ptr(), part.data_ptr(), int(flat or dtype == torch.float32), N, C
    assert L.gt_fs_sums(a, None) == 0
    want = np.zeros((S, G, C, Up))
    for s in range(S):
        rows = slice(s * SLICE, min(N, (s + 1) * SLICE))
        for g in range(G):
            np.add.at(want[s, g, :, :Ur], lab[rows], f[g, rows].astype(np.float64))
    got = part.cpu().numpy()
    assert got[:want.size].tobytes() == want.tobytes() and np.isnan(got[want.size:]).all()
    count = np.bincount(lab, minlength=C)
    mean = np.full((G, C, Up), np.nan, np.float32)
    mean[:, :, :Ur] = (want.sum(0)[:, :, :Ur] / np.maximum(count, 1)[None, :, None]).astype(np.float32)
    meand, planes = _dev(mean), _nan(3 * G * Up * Np, torch.bfloat16)
    c = K.FsCenterArgs()
    c.src, c.label, c.mean, c.planes = a.src, a.label, meand.data_ptr(), planes.data_ptr()
    c.sprec, c.N, c.Np, c.C = a.sprec, N, Np, C
    assert L.gt_fs_center(c, None) == 0
    cen = np.zeros((G, Up, Np), np.float32)
    cen[:, :Ur, :N] = (f - mean[:, lab, :Ur]).transpose(0, 2, 1)
    assert torch.equal(planes[:3 * G * Up * Np].view(torch.int16),
                       _split(_dev(cen)).reshape(-1).view(torch.int16)) and torch.isnan(planes[-GUARD:]).all()
    slices, res = -(-Np // SLICE), []
    for per in (slices, 1):                                  # one round, then one slice per round
        buf, acc = _nan(per * G * Up * Up), _nan(G * Up * Up, torch.float64)
        t, r = K.FsScatterArgs(), K.FsReduceArgs()
        t.planes, t.part, t.G, t.Up, t.Np = planes.data_ptr(), buf.data_ptr(), G, Up, Np
        r.part, r.acc, r.G, r.Up = buf.data_ptr(), acc.data_ptr(), G, Up
        for s0 in range(0, slices, per):
            t.s0, t.ns, r.ns, r.first, r.last = s0, per, per, int(s0 == 0), int(s0 + per == slices)
            assert L.gt_fs_scatter(t, None) == 0 and L.gt_fs_reduce(r, None) == 0
        assert torch.isnan(buf[-GUARD:]).all() and torch.isnan(acc[-GUARD:]).all()
        res.append(acc[:G * Up * Up].cpu().numpy().reshape(G, Up, Up))
    assert res[0].tobytes() == res[1].tobytes() and np.array_equal(res[0], res[0].transpose(0, 2, 1))
    c64 = cen.astype(np.float64)
    ref = c64 @ c64.transpose(0, 2, 1)
    bound = (SLICE + 4) * EPS * (np.abs(c64) @ np.abs(c64).transpose(0, 2, 1))
    ratio = float((np.abs(res[0] - ref) / np.maximum(bound, 1e-300)).max())
    WORST["scatter"] = max(WORST.get("scatter", 0.0), ratio)
    print("[cnn-gaussian] scatter {}: worst error / bound {:.3f} (all cases so far {:.3f})".format(
        case, ratio, WORST["scatter"]))
    assert (np.abs(res[0] - ref) <= bound).all()
    del keep


def _dist(K, L, f, W, t, count, Up, dtype, r0=0, extra=0):
    """``gt_fs_dist`` over hidden rows ``f [G, m, Ur]``: the ``[G, m, C]`` result; untouched memory stays NaN."""
    (G, m, Ur), C = f.shape, t.shape[1]
    hid = np.full((G, 64, Up), np.nan, np.float32)
    hid[:, :m, :Ur] = f
    hid = _dev(hid, dtype)
    wt = np.zeros((G, Up, Up), np.float32)
    wt[:, :Ur, :Ur] = W.transpose(0, 2, 1)
    planes = _split(_dev(wt)).contiguous()
    tm = np.full((G, C, Up), np.nan, np.float32)
    tm[:, :, :Ur] = t
    tm, ldo = _dev(tm), m + r0 + extra
    out = _nan(G * ldo * C)
    a = K.FsDistArgs()
    q = a.q
    q.h, q.G, q.B, q.Up, q.Ur = hid.data_ptr(), G, 64, Up, Ur
    a.wt, a.wmean, a.out, a.sprec, a.m, a.C = planes.data_ptr(), tm.data_ptr(), out.data_ptr(), \
        int(dtype == torch.float32), m, C
    a.empty, a.r0, a.ldo = int(sum(1 << c for c in range(C) if count[c] == 0)), r0, ldo
    assert L.gt_fs_dist(a, None) == 0
    res = out[:G * ldo * C].view(G, ldo, C).cpu().numpy()
    assert torch.isnan(out[-GUARD:]).all() and np.isnan(res[:, :r0]).all() and np.isnan(res[:, r0 + m:]).all()
    return res[:, r0:r0 + m]


def _dist_ref(f, W, t, count):
    """fp64 ``(distance, bound) [m, C]`` of one member (``+inf``, bound 0 for an empty class)."""
    f, W, t = (np.asarray(v, np.float64) for v in (f, W, t))
    Ur = W.shape[0]
    a = np.abs((f @ W)[:, None, :] - t[None])
    e = ((Ur + 4) * EPS * (np.abs(f) @ np.abs(W)))[:, None, :]
    d = (a * a).sum(-1)
    bound = (2 * a * e + e * e).sum(-1) + (Ur + 4) * EPS * d
    d[:, np.asarray(count) == 0], bound[:, np.asarray(count) == 0] = np.inf, 0.0
    return d, bound


def _within(tag, got, d, bound):
    fin = np.isfinite(d)
    assert np.array_equal(np.isinf(got), ~fin) and (got[~fin] > 0).all()
    ratio = float((np.abs(got[fin] - d[fin]) / bound[fin]).max()) if fin.any() else 0.0
    WORST["dist"] = max(WORST.get("dist", 0.0), ratio)
    print("[cnn-gaussian] distance {}: worst error / bound {:.3f} (all cases so far {:.3f})".format(
        tag, ratio, WORST["dist"]))
    assert ratio <= 1.0


@pytest.mark.parametrize("m", [1, 33])
@pytest.mark.parametrize("Up,Ur,C,G,dtype", [(32, 20, 1, 1, torch.float32), (32, 20, 16, 3, torch.bfloat16),
                                             (160, 130, 3, 3, torch.float32), (160, 130, 16, 1, torch.bfloat16)])
def test_dist_kernel_against_fp64(Up, Ur, C, G, dtype, m):
    """Row ``m - 1`` repeats row 0; a second launch puts the rows at offset 5 of a longer result: a row's bytes do
    not depend on where it sits."""
    K, L = _lib()
    rng = np.random.default_rng(1)
    f = _features(G, m, Ur, C, dtype, seed=2)[0]
    f[:, m - 1] = f[:, 0]
    W = (np.triu(rng.standard_normal((G, Ur, Ur))) / np.sqrt(Ur)).astype(np.float32)
    t = rng.standard_normal((G, C, Ur)).astype(np.float32)
    count = np.array([1] * (C - 1) + [C == 1])
    got = _dist(K, L, f, W, t, count, Up, dtype)
    assert got[:, 0].tobytes() == got[:, m - 1].tobytes()
    assert got.tobytes() == _dist(K, L, f, W, t, count, Up, dtype, r0=5, extra=2).tobytes()
    for g in range(G):
        _within((Up, Ur, C, G, m, g), got[g], *_dist_ref(f[g], W[g], t[g], count))


REFUSED = [dict(Up=48), dict(C=0), dict(C=17), dict(m=0), dict(N=0), dict(N=1 << 24, Np=1 << 24), dict(ns=0)]


@pytest.mark.parametrize("over", REFUSED, ids=lambda o: "-".join("{}{}".format(*kv) for kv in o.items()))
def test_launchers_refuse_and_launch_nothing(over):
    """Valid arguments over NaN-filled outputs, one field overridden: a non-zero return and every output NaN."""
    K, L = _lib()
    G, N, Ur, Up, C = 1, 40, 20, 32, 3
    f, lab = _features(G, N, Ur, C, torch.float32)
    outs = [_nan(G * C * Up, torch.float64), _nan(3 * G * Up * 64, torch.bfloat16), _nan(G * Up * Up),
            _nan(G * Up * Up, torch.float64), _nan(G * 64 * C)]
    labd, mean = _dev(lab.astype(np.int32)), _dev(np.zeros((G, C, Up), np.float32))
    a, c, t, r, d = K.FsSumsArgs(), K.FsCenterArgs(), K.FsScatterArgs(), K.FsReduceArgs(), K.FsDistArgs()
    keep = [_src(K, s, f, Up, torch.float32, False) for s in (a.src, c.src, d.q)]
    a.label, a.part, a.sprec, a.N, a.C = labd.data_ptr(), outs[0].data_ptr(), 1, N, C
    c.label, c.mean, c.planes, c.sprec, c.N, c.Np, c.C = a.label, mean.data_ptr(), outs[1].data_ptr(), 1, N, 64, C
    t.planes, t.part, t.G, t.Up, t.Np, t.s0, t.ns = outs[1].data_ptr(), outs[2].data_ptr(), G, Up, 64, 0, 1
    r.part, r.acc, r.G, r.Up, r.ns, r.first, r.last = outs[2].data_ptr(), outs[3].data_ptr(), G, Up, 1, 1, 1
    d.wt, d.wmean, d.out, d.sprec, d.m, d.C, d.ldo = outs[1].data_ptr(), mean.data_ptr(), outs[4].data_ptr(), 1, N, C, 64
    hit = 0
    for args, fn in ((a, L.gt_fs_sums), (c, L.gt_fs_center), (t, L.gt_fs_scatter), (r, L.gt_fs_reduce),
                     (d, L.gt_fs_dist)):
        mine = [(o, k) for o in (args, getattr(args, "src", None), getattr(args, "q", None)) if o is not None
                for k in over if hasattr(o, k)]
        for o, k in mine:
            setattr(o, k, over[k])
        if mine:
            hit += 1
            assert fn(args, None) != 0
    torch.cuda.synchronize()
    assert hit and all(torch.isnan(o.float()).all() for o in outs)
    del keep


# through the predictors: plain fp32 ("ones"), a 3-member ensemble, a bf16 fit; the shared fits have 500 dense units
BANK, NQ = slice(20, 320), 40


def _fitted(case):
    if case == "ens3":
        ens, x = E._fit("rgb")[:2]
        return ens, ens.members, x
    clf, x = F._fit(case)[2:4]
    return clf, [clf], x


@pytest.mark.parametrize("case", ["ones", "ens3", "bf16"])
def test_through_the_predictor(case, monkeypatch):
    """A bank of 300 images at batch 32 (ten chunks): ``cov`` within the scatter bound and the distances within the
    distance bound of the host definitions on HIP's own ``embed`` output and the returned ``stats``; the same bytes
    from batch 256 and from the bank embedded beforehand; the ensemble's distance is the ordered mean of its
    members'; the two refusals of the HIP path."""
    from gentun_amd.models import cnn_fitted as M
    from gentun_amd.ops import cnn_kernels as K
    obj, members, x = _fitted(case)
    G, U, C = len(members), members[0].dense_units, obj.classes
    lab = np.arange(300) % max(C - 1, 1)                     # the last class stays empty
    st = obj.gaussian_fit(x[BANK], labels=lab, device=DEV, batch=32)
    eb = obj.embed(x[BANK], device=DEV)
    for other in (obj.gaussian_fit(x[BANK], labels=lab, device=DEV, batch=256),
                  obj.gaussian_fit(eb, labels=lab, device=DEV, batch=32)):
        assert all(np.asarray(other[k]).tobytes() == np.asarray(st[k]).tobytes() for k in M.GAUSS_KEYS)
    assert st["cov"].shape == (G, U, U) and np.array_equal(st["cov"], st["cov"].transpose(0, 2, 1))
    for g in range(G):
        f = eb[:, g * U:(g + 1) * U]
        count, mean, cov = M.gaussian_moments(f, lab, C)
        c = np.abs((f - mean[lab]).astype(np.float64))
        assert np.array_equal(count, st["count"]) and mean.tobytes() == st["mean"][g].tobytes()
        assert (np.abs(st["cov"][g] - cov) <= (SLICE + 4) * EPS * (c.T @ c) / 300).all()
    d = obj.mahalanobis(x[:NQ], st, device=DEV, batch=32)
    assert d.dtype == np.float32 and d.shape == (NQ, C) and np.isinf(d[:, -1]).all()
    assert d.tobytes() == obj.mahalanobis(x[:NQ], st, device=DEV, batch=256).tobytes()
    pred = obj.hip_predictor(DEV, 32)
    per = M.gaussian_state(pred, G).distance(pred, x[:NQ], M.mahalanobis_check(st, G, U, 32, None)[0], C)
    w = np.asarray(obj.weights, np.float32) if G > 1 else np.ones(1, np.float32)
    assert M.member_mean(per, w).tobytes() == d.tobytes()
    eq = obj.embed(x[:NQ], device=DEV)
    for g in range(G):
        _within("{} member {}".format(case, g), per[g],
                *_dist_ref(eq[:, g * U:(g + 1) * U], st["whiten"][g], st["wmean"][g], st["count"]))
    many = {k: (np.zeros(17, np.int64) + 1 if k == "count" else np.zeros((G, 17, U), np.float32)
                if k in ("mean", "wmean") else v) for k, v in st.items()}
    with pytest.raises(ValueError, match="at most 16 classes"):
        obj.mahalanobis(x[:2], many, device=DEV)
    monkeypatch.setattr(K, "FS_MAX_STORE_BYTES", 1 << 18)
    with pytest.raises(ValueError, match='backend="torch"'):
        obj.gaussian_fit(eb, labels=lab, device=DEV)


@pytest.mark.parametrize("case", ["c3", "ens3"])
def test_other_requests_are_unchanged_by_a_fit(case):
    obj, members, x = _fitted(case)
    xs, m = x[:70], F._model("c3", nfold=2)[0] if case == "c3" else None
    before = (obj.predict(xs, device=DEV), obj.neighbors(xs, x[70:200], k=3, device=DEV), m and m.cross_validate())
    obj.mahalanobis(xs, obj.gaussian_fit(x[70:200], device=DEV), device=DEV)
    after = (obj.predict(xs, device=DEV), obj.neighbors(xs, x[70:200], k=3, device=DEV), m and m.cross_validate())
    assert before[0].tobytes() == after[0].tobytes() and before[2] == after[2]
    assert all(b.tobytes() == a.tobytes() for b, a in zip(before[1], after[1]))
