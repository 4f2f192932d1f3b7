"""Test-time augmentation of fitted Genetic-CNN models on an MI355X: ``gt_tta_views`` (csrc/hip/cnn_tta.hip)
alone against the numpy oracle (tests/augment_ref.py), ``gt_head_tta`` (csrc/hip/cnn_dense.hip) alone against
``gt_head_predict`` / ``gt_head_ensemble`` and numpy, then ``predict(tta=...)`` of ``CnnClassifier`` and
``CnnEnsemble`` through the HIP predictors against the same predictors fed the oracle's views one by one.

Every comparison is byte equality or a refusal. The fits are those of tests/test_cnn_fitted_gpu.py and
tests/test_cnn_ensemble_gpu.py (320 rows, 1 epoch, batch 32; shared with them inside one pytest process, left
unchanged) plus one 16-member ensemble."""

import numpy as np
import pytest
import torch

import augment_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F

pytestmark = pytest.mark.gpu

SHORTHAND = {"shift": 2, "flip": True}                   # 10 views: 3 rows per launch of 32 leave 2 rows unused
V16 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (3, -2, 0), (-27, 0, 0), (0, 27, 0),
       (0, 0, 1), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1), (-3, 2, 1), (27, 0, 1), (0, -27, 1)]
NROWS = 70                                               # the last chunk is short (3, 16 and 25 rows per chunk)


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _ordered_mean(per_view):
    """The contract, written out: fp32 sums in view order, then one fp32 product with fp32 1 / V."""
    acc = per_view[0]
    for p in per_view[1:]:
        acc = np.add(acc, p, dtype=np.float32)
    inv = np.float32(1) / np.float32(len(per_view))
    return np.multiply(acc, inv, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------
# gt_tta_views alone
# ---------------------------------------------------------------------------------------------------------

GEOMETRIES = {"cifar": ((32, 32, 3), (32, 32, 8)), "mnist": ((28, 28, 1), (32, 32, 8)), "odd": ((6, 5, 3), (8, 8, 8))}
SPARE, GUARD = 2, 4096       # staging rows past V * R, elements past the staging tensor: all stay NaN


def _view_table(V, Hr, Wr):
    """``V`` distinct views mixing both signs, |d| = min(Hr, Wr) - 1, the largest |dy| and |dx|, and flips."""
    top = min(Hr, Wr) - 1
    table = [(0, 0, 1), (-top, top, 0), (top, -top, 1), (1 - Hr, 0, 0), (0, Wr - 1, 1), (Hr - 1, 1 - Wr, 0),
             (1, -2, 1), (-2, 1, 0), (0, 0, 0), (2, 2, 1), (-1, -1, 0), (top, 0, 1), (0, -top, 0), (1, 1, 1),
             (-1, 2, 1), (2, -1, 0)]
    assert len(set(table)) == 16
    return {1: [table[2]], 2: table[:2], 16: table}[V]


class _Views(object):
    """A raw chunk ``[R][Hp][Wp][Cp]`` of small positive integers (exact in bf16, never 0) in the real extent --
    in the channel padding too, which the kernel copies -- and NaN outside the real extent, which it must not
    read; a NaN-filled staging tensor of ``rows`` rows with a NaN guard tail."""

    def __init__(self, real, stored, dtype, Rr, rows, seed=0):
        (self.Hr, self.Wr, self.C), (self.Hp, self.Wp, self.Cp) = real, stored
        self.R, self.rows, self.dtype = Rr, rows, dtype
        rs = np.random.RandomState(seed)
        self.data = rs.randint(1, 200, size=(Rr, self.Hr, self.Wr, self.Cp)).astype(np.float32)
        raw = np.full((Rr, self.Hp, self.Wp, self.Cp), np.nan, np.float32)
        raw[:, :self.Hr, :self.Wr] = self.data
        self.raw = torch.from_numpy(raw).to(device=_dev(), dtype=dtype).contiguous()
        self.img = self.Hp * self.Wp * self.Cp
        self.out = torch.full((rows * self.img + GUARD,), float("nan"), dtype=dtype, device=_dev())
        self.nan_bits = _bits(self.out)[0].item()

    def args(self, views):
        from gentun_amd.ops import cnn_kernels as K
        a = K.TtaViewArgs()
        a.raw, a.out = self.raw.data_ptr(), self.out.data_ptr()
        a.R, a.V, a.rows = self.R, len(views), self.rows
        a.Hp, a.Wp, a.Hr, a.Wr, a.Cp = self.Hp, self.Wp, self.Hr, self.Wr, self.Cp
        a.prec = 1 if self.dtype == torch.float32 else 0
        for i, (dy, dx, flip) in enumerate(views[:K.TTA_MAXV]):
            a.dy[i], a.dx[i], a.flip[i] = dy, dx, flip
        return a

    def launch(self, a):
        from gentun_amd.ops import cnn_kernels as K
        self.out.fill_(float("nan"))
        rc = K.lib().gt_tta_views(a, _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self, start=0):
        return bool((_bits(self.out[start:]) == self.nan_bits).all().item())

    def check(self, views):
        want = np.stack([R.transform(self.data[r], dy, dx, fl, (self.Hp, self.Wp))
                         for dy, dx, fl in views for r in range(self.R)])
        assert not np.isnan(want).any()                  # zeros outside the real extent, never the raw NaN
        n = len(views) * self.R * self.img
        got = self.out[:n].cpu()
        assert torch.equal(_bits(got), _bits(torch.from_numpy(want).to(self.dtype).reshape(-1))), views
        assert self.untouched(n)                         # rows >= V * R and the guard


@pytest.mark.parametrize("Rr", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_views_kernel_equals_the_oracle(geom, dtype, Rr):
    real, stored = GEOMETRIES[geom]
    c = _Views(real, stored, dtype, Rr, 16 * Rr + SPARE)
    for V in (1, 2, 16):
        views = _view_table(V, real[0], real[1])
        assert c.launch(c.args(views)) == 0
        c.check(views)
    # exactly as many staging rows as views x raw rows
    c = _Views(real, stored, dtype, Rr, 2 * Rr, seed=1)
    views = _view_table(2, real[0], real[1])
    assert c.launch(c.args(views)) == 0
    c.check(views)


def test_views_launcher_refusals():
    from gentun_amd.ops import cnn_kernels as K
    c = _Views((6, 5, 3), (8, 8, 8), torch.float32, 3, 8)
    ok = [(0, 0, 0), (5, -4, 1)]
    assert c.launch(c.args(ok)) == 0 and not c.untouched()                # the accepted call does write
    assert K.lib().gt_tta_views(None, _stream()) != 0

    def bad(views=ok, **kw):
        a = c.args(views)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for a in (bad(raw=0), bad(out=0), bad(Cp=12), bad(Cp=4), bad(Cp=0), bad(Hr=9), bad(Wr=9), bad(Hr=0), bad(V=0),
              bad(V=17), bad(V=-1), bad([(6, 0, 0)]), bad([(-6, 0, 0)]), bad([(0, 5, 0)]), bad([(0, -5, 0)]),
              bad([(0, 0, 0), (0, 0, 1), (-2 ** 31, 0, 0)]), bad(Hr=2, Wr=8, views=[(2, 0, 0)]),
              bad(ok + [(1, 1, 1)]),                                       # 3 views x 3 rows > 8 staging rows
              bad(rows=5), bad(rows=0), bad(R=0), bad(R=-1), bad(prec=2),
              bad(R=2 ** 30, rows=2 ** 31 - 1),                            # V * R past every int
              bad(Hp=2 ** 15, Wp=2 ** 15, Cp=2 ** 15)):                    # chunks past FastDiv's range
        assert c.launch(a) != 0
        assert c.untouched()
    assert c.launch(c.args([(-5, 4, 1), (5, -4, 0)])) == 0                # |dy| = Hr - 1, |dx| = Wr - 1 are the largest


# ---------------------------------------------------------------------------------------------------------
# gt_head_tta alone
# ---------------------------------------------------------------------------------------------------------

def _head_tta(plog, b2, w, Rr, V, members=True):
    from gentun_amd.ops import cnn_kernels as K
    G, nt, B, C = plog.shape
    logits = torch.full((G, Rr, C), float("nan"), dtype=torch.float32, device=plog.device)
    proba = torch.full_like(logits, float("nan"))
    ens = torch.full((Rr, C), float("nan"), dtype=torch.float32, device=plog.device)
    votes = torch.full((Rr, C), -1, dtype=torch.int32, device=plog.device)
    a = K.HeadTtaArgs()
    a.plog, a.b2, a.weight = plog.data_ptr(), b2.data_ptr(), w.data_ptr()
    a.logits, a.proba = (logits.data_ptr(), proba.data_ptr()) if members else (0, 0)
    a.ens, a.votes = ens.data_ptr(), votes.data_ptr()
    a.G, a.B, a.Up, a.C, a.R, a.V = G, B, nt * 16, C, Rr, V
    a.inv_v = float(np.float32(1) / np.float32(V))
    K.check(K.lib().gt_head_tta(a, _stream()), "head_tta")
    torch.cuda.synchronize()
    return logits.cpu().numpy(), proba.cpu().numpy(), ens.cpu().numpy(), votes.cpu().numpy()


_POOL = {}


def _pool(n):
    """``n`` standard normal fp32 values: one draw of the largest case, shared and left unchanged."""
    if "v" not in _POOL:
        _POOL["v"] = np.random.default_rng(7).standard_normal(64 * 68 * 256 * 16).astype(np.float32)
    return _POOL["v"][:n]


def _weights(G, seed):
    w = np.random.default_rng(seed).random(G) + 0.1
    return [(np.ones(G) / G).astype(np.float32), (w / w.sum()).astype(np.float32)]


# G = 1: the classifier's use, three waves without a member; 3: ragged; 64: the LDS table is full and every
# wave's member loop runs 16 times. 68 tiles: the lane's stride loop runs twice.
@pytest.mark.parametrize("nt", [2, 68])
@pytest.mark.parametrize("G", [1, 3, 64])
def test_head_tta_kernel(G, nt):
    for V, Rr, B in ((2, 1, 32), (5, 3, 32), (16, 2, 32), (10, 25, 256)):
        for C in (1, 3, 10, 16):
            plog = _pool(G * nt * B * C).reshape(G, nt, B, C).copy()
            b2 = np.random.default_rng(100 * G + C).standard_normal((G, C)).astype(np.float32)
            if C >= 2:
                # raw row 0: views 0 and 1 favour one of the two last classes each, by the same margin, every
                # further view ties them; every other class is far enough down to add an exact 0 to the
                # softmax sum. p_0 + p_1 is p_1 + p_0, so the two classes tie exactly only after averaging.
                for v in range(V):
                    plog[:, :, v * Rr, :] = 0.0
                    plog[:, 0, v * Rr, :C - 2] = -300.0
                    plog[:, 0, v * Rr, C - 2:] = 7.0
                plog[:, 0, 0, C - 1] = 0.0
                plog[:, 0, Rr, C - 2] = 0.0
                b2[:, C - 1] = b2[:, C - 2]
            dp, db = torch.from_numpy(plog).to(_dev()), torch.from_numpy(b2).to(_dev())
            row_logits, row_proba = F._head_predict(dp, db)              # [G][B][C]: every launch row
            want_logits = _ordered_mean([row_logits[:, v * Rr:(v + 1) * Rr] for v in range(V)])
            want_proba = _ordered_mean([row_proba[:, v * Rr:(v + 1) * Rr] for v in range(V)])
            for w in _weights(G, G + C):
                dw = torch.from_numpy(w).to(_dev())
                logits, proba, ens, votes = _head_tta(dp, db, dw, Rr, V)
                assert logits.tobytes() == want_logits.tobytes(), (V, Rr, B, C)
                assert proba.tobytes() == want_proba.tobytes(), (V, Rr, B, C)
                want, count = E._ordered_combine(want_proba, w)
                assert ens.tobytes() == want.tobytes(), (V, Rr, B, C, float(np.abs(ens - want).max()))
                assert votes.tobytes() == count.tobytes(), (V, Rr, B, C)
                if C >= 2:
                    assert (row_proba[:, 0, C - 2] > row_proba[:, 0, C - 1]).all()          # view 0 alone: no tie
                    assert (proba[:, 0, C - 2] == proba[:, 0, C - 1]).all() and votes[0, C - 2] == G
                # null member pointers: the same mean and votes, nothing else written
                l0, p0, ens0, votes0 = _head_tta(dp, db, dw, Rr, V, members=False)
                assert np.isnan(l0).all() and np.isnan(p0).all()
                assert ens0.tobytes() == ens.tobytes() and votes0.tobytes() == votes.tobytes()


@pytest.mark.parametrize("G", [1, 5, 64])
def test_head_tta_of_one_view_is_the_ensemble_head(G):
    for nt, B, C in ((2, 33, 3), (68, 32, 16), (4, 1, 1), (4, 256, 10)):
        plog = _pool(G * nt * B * C).reshape(G, nt, B, C)
        b2 = np.random.default_rng(G + C).standard_normal((G, C)).astype(np.float32)
        dp, db = torch.from_numpy(plog).to(_dev()), torch.from_numpy(b2).to(_dev())
        for w in _weights(G, 3):
            dw = torch.from_numpy(w).to(_dev())
            for members in (True, False):
                want = E._head_ensemble(dp, db, dw, members=members)
                got = _head_tta(dp, db, dw, B, 1, members=members)
                for a, b in zip(got, want):                              # logits, proba, ens, votes
                    assert a.tobytes() == b.tobytes(), (nt, B, C, members)
                assert np.isfinite(got[2]).all() and np.isnan(got[0]).all() == (not members)


def test_head_tta_refusals():
    from gentun_amd.ops import cnn_kernels as K
    t = torch.zeros(4096, device=_dev())

    def args(**kw):
        a = K.HeadTtaArgs()
        a.plog = a.b2 = a.weight = a.logits = a.proba = a.ens = a.votes = t.data_ptr()
        a.G, a.B, a.Up, a.C, a.R, a.V, a.inv_v = 1, 32, 16, 2, 2, 16, 1.0 / 16
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw in (dict(G=0), dict(G=65), dict(C=0), dict(C=17), dict(Up=24), dict(Up=0), dict(R=0), dict(R=-1),
               dict(V=0), dict(V=17), dict(R=3), dict(V=4, R=9), dict(B=31), dict(B=0), dict(R=2 ** 30, V=8),
               dict(plog=0), dict(b2=0), dict(weight=0), dict(ens=0), dict(votes=0)):
        assert K.lib().gt_head_tta(args(**kw), _stream()) != 0, kw
    assert K.lib().gt_head_tta(None, _stream()) != 0
    torch.cuda.synchronize()
    assert not bool(t.any())                           # nothing was launched


# ---------------------------------------------------------------------------------------------------------
# end to end: the classifier
# ---------------------------------------------------------------------------------------------------------

CLF_CASES = ["chain", "mnist", "bn", "bf16"]             # plain 32x32x3 fp32, 28x28x1 stored 32x32, BatchNorm, bf16
_VIEWS_OF = {}


def _oracle_views(x, views):
    """``{view: [n, H, W, C]}`` by the oracle, image by image; computed once per (image set, view)."""
    key = (x.shape, x[:2].tobytes())
    have = _VIEWS_OF.setdefault(key, {})
    for v in views:
        if v not in have:
            have[v] = np.stack([R.transform(img, *v) for img in x])
    return [have[v] for v in views]


def _clf(case):
    m, job, clf, x, lab = F._fit(case)
    return clf, x[:NROWS]


@pytest.mark.parametrize("batch", [32, 256])
@pytest.mark.parametrize("case", CLF_CASES)
def test_predict_is_the_ordered_mean_over_the_views(case, batch):
    from gentun_amd.models.cnn_fitted import tta_views
    clf, xs = _clf(case)
    for tta in (SHORTHAND, V16):
        views = tta_views(tta, clf.input_shape)
        st = clf.hip_predictor(_dev(), batch).tta_state(views)
        assert st.R == batch // len(views) and st.R >= 2
        tx = _oracle_views(xs, views)
        for output in ("logits", "proba"):
            want = _ordered_mean([clf.predict(t, device=_dev(), output=output, batch=batch) for t in tx])
            got = clf.predict(xs, device=_dev(), output=output, batch=batch, tta=tta)
            assert got.dtype == np.float32 and got.shape == (NROWS, clf.classes) and np.isfinite(got).all()
            assert got.tobytes() == want.tobytes(), (output, len(views), float(np.abs(got - want).max()))
            assert got.tobytes() != clf.predict(xs, device=_dev(), output=output, batch=batch).tobytes()
        label = clf.predict(xs, device=_dev(), output="label", batch=batch, tta=tta)
        assert label.dtype == np.int64 and np.array_equal(label, np.argmax(want, 1))     # of the mean probabilities
        assert np.array_equal(clf.predict_classes(xs, device=_dev(), batch=batch, tta=tta), label)


@pytest.mark.parametrize("case", CLF_CASES)
def test_the_identity_view_is_no_tta_and_tta_leaves_no_trace(case):
    clf, xs = _clf(case)
    for batch in (32, 256):
        plain = {o: clf.predict(xs, device=_dev(), output=o, batch=batch) for o in ("proba", "logits", "label")}
        for o, want in plain.items():
            assert clf.predict(xs, device=_dev(), output=o, batch=batch, tta=[(0, 0, 0)]).tobytes() == want.tobytes()
            assert clf.predict(xs, device=_dev(), output=o, batch=batch, tta={}).tobytes() == want.tobytes()
        pred = clf.hip_predictor(_dev(), batch)
        clf.predict(xs, device=_dev(), batch=batch, tta=SHORTHAND)       # 30 of 32 / 250 of 256 staging rows written
        clf.predict(xs[:3], device=_dev(), batch=batch, tta=V16)
        assert clf.hip_predictor(_dev(), batch) is pred and len(pred._tta) >= 3     # the cached predictor, lazily
        for o, want in plain.items():                                   # the plain path after the TTA path
            assert clf.predict(xs, device=_dev(), output=o, batch=batch).tobytes() == want.tobytes()
        with pytest.raises(ValueError):
            clf.predict(xs, device=_dev(), tta=SHORTHAND, dtype=torch.float64)     # an option of the torch backend


def test_row_order_does_not_change_a_row():
    clf, xs = _clf("mnist")
    a = clf.predict(xs, device=_dev(), output="logits", batch=256, tta=SHORTHAND)
    rev = clf.predict(xs[::-1], device=_dev(), output="logits", batch=256, tta=SHORTHAND)
    assert rev[::-1].tobytes() == a.tobytes()
    assert clf.predict(xs[7], device=_dev(), output="logits", batch=256, tta=SHORTHAND).tobytes() == a[7:8].tobytes()


def test_cross_validate_is_unchanged_by_tta():
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    scores = list(m.fold_scores)
    m.fit()
    plain = m.predict(x[:40], output="logits")
    assert m.predict(x[:40], tta=SHORTHAND).shape == (40, 3)             # the model forwards the argument
    assert m.predict(x[:40], output="logits").tobytes() == plain.tobytes()
    assert m.cross_validate() == first and m.fold_scores == scores


# ---------------------------------------------------------------------------------------------------------
# end to end: the ensemble
# ---------------------------------------------------------------------------------------------------------

def _check_ensemble(ens, xs, tta, members):
    from gentun_amd.models.cnn_ensemble import combine, vote_label
    pred = ens.hip_predictor(_dev(), 256)
    out = ens.predict_outputs(xs, device=_dev(), batch=256, tta=tta)
    k = len(ens)
    assert out["member_proba"].shape == (k, len(xs), ens.classes) and np.isfinite(out["member_logits"]).all()
    for g in members:
        m = ens.members[g]
        assert out["member_proba"][g].tobytes() == \
            m.predict(xs, device=_dev(), output="proba", batch=pred.EB, tta=tta).tobytes(), g
        assert out["member_logits"][g].tobytes() == \
            m.predict(xs, device=_dev(), output="logits", batch=pred.EB, tta=tta).tobytes(), g
    proba, votes = combine(out["member_proba"], ens.weights)
    want = E._ordered_combine(out["member_proba"], ens.weights)
    assert proba.tobytes() == want[0].tobytes() and votes.tobytes() == want[1].tobytes()
    assert out["proba"].dtype == np.float32 and out["proba"].tobytes() == proba.tobytes()
    assert out["votes"].dtype == np.int32 and out["votes"].tobytes() == votes.tobytes()
    assert np.array_equal(out["label"], np.argmax(proba, 1))
    assert np.array_equal(out["vote_label"], vote_label(votes, proba))
    # null member pointers
    assert ens.predict(xs, device=_dev(), output="proba", tta=tta).tobytes() == proba.tobytes()
    assert ens.predict(xs, device=_dev(), output="votes", tta=tta).tobytes() == votes.tobytes()
    return pred, out


@pytest.mark.parametrize("case", list(E.CASES))
def test_ensemble_of_three(case):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models.cnn_fitted import tta_views
    fitted, x, y, lab = E._fit(case)
    xs = x[:NROWS]
    plain = fitted.predict_outputs(xs, device=_dev(), batch=256)
    for weights in (None, [3.0, 1.0, 4.0]):
        ens = fitted if weights is None else CnnEnsemble(fitted.members, weights=weights)
        for tta in (SHORTHAND, V16):
            pred, out = _check_ensemble(ens, xs, tta, range(E.K3))
            st = pred.tta_state(tta_views(tta, ens.input_shape))
            assert st.R == pred.EB // st.V and st.R >= 2
            assert out["member_logits"].tobytes() != plain["member_logits"].tobytes()
    same = fitted.predict_outputs(xs, device=_dev(), batch=256, tta=[(0, 0, 0)])
    again = fitted.predict_outputs(xs, device=_dev(), batch=256)         # the plain path after the TTA path
    for name in plain:
        assert same[name].tobytes() == plain[name].tobytes() and again[name].tobytes() == plain[name].tobytes(), name


def _genomes16():
    out = [F.CHAIN, F.ONES, F.MIXED]
    i = 0
    while len(out) < 16:
        i += 1
        g = {"S_1": format(1 + i % 7, "03b"), "S_2": format((i * 397 + 85) % 1024, "010b")}
        if g not in out:
            out.append(g)
    return out


def test_ensemble_of_sixteen_keeps_two_rows_per_launch():
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn_fitted import tta_views
    shape, classes = E.CASES["rgb"][:2]
    x, y, lab = E._data(shape, classes)
    ens = fit_ensemble(x, y, _genomes16(), device=_dev(), **E._space("rgb"))
    assert len(ens) == 16
    xs = x[:NROWS]
    for tta in (V16, SHORTHAND):
        pred, out = _check_ensemble(ens, xs, tta, (0, 5, 10, 15) if tta is V16 else (3,))
        st = pred.tta_state(tta_views(tta, ens.input_shape))
        # 16 groups fit the twin budget only below the 256 rows asked for
        assert pred.EB == pred.job.eval_batch() and 32 <= pred.EB < 256
        assert st.R == pred.EB // st.V and st.R >= 2
        print("[cnn-tta] k = 16: {} rows per launch, {} views of {} rows".format(pred.EB, st.V, st.R))
