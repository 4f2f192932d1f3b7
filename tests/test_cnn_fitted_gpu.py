"""The fitted Genetic-CNN model on an MI355X: ``gt_head_predict`` alone, then ``GeneticCnnModel.fit`` on the HIP
executor and ``CnnClassifier.predict`` through the HIP predictor (gentun_amd/models/cnn_fitted.py) against the
job's own evaluation, the exported file, the chunking and the fp64 oracle.

Every fit: 320 rows, 1 epoch, batch 32. One fit per case, shared by the tests and left unchanged."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, BATCH = 320, 32
EPS = 2.0 ** -24            # one fp32 rounding (half an ulp) relative to the value rounded

CHAIN = {"S_1": "101", "S_2": "1010010001"}
ONES = {"S_1": "111", "S_2": "1111111111"}
MIXED = {"S_1": "101", "S_2": "0101110011"}
SPACE = dict(nodes=(3, 5), kernels=(20, 50), ks=((5, 5), (5, 5)), dense=500)
# name -> (input shape, classes, genes, batch_norm, dtype, loss)
CASES = {
    "chain": ((32, 32, 3), 10, CHAIN, False, "fp32", "bce_compat"),
    "ones": ((32, 32, 3), 10, ONES, False, "fp32", "bce_compat"),
    "mnist": ((28, 28, 1), 10, MIXED, False, "fp32", "ce"),          # stored 32 x 32: W1 has padded-pixel rows
    "bn": ((32, 32, 3), 10, MIXED, True, "fp32", "ce"),
    "bn_mnist": ((28, 28, 1), 10, CHAIN, True, "fp32", "bce_compat"),
    "c3": ((28, 28, 1), 3, CHAIN, False, "fp32", "bce_compat"),
    "c16": ((32, 32, 3), 16, MIXED, False, "fp32", "ce"),
    "bf16": ((32, 32, 3), 10, MIXED, False, "bf16", "bce_compat"),
}
FP32_CASES = [c for c in CASES if CASES[c][4] == "fp32"]

# Floor of the oracle bound where stock torch's own fp32 error is tiny: the largest error of the stock-torch
# fp32 forward on the same GPU against the fp64 reference over FP32_CASES, relative to the largest logit
# (measured on an MI355X: 4.1e-07 to 8.6e-07, rounded up; profiles/cnn_predict.txt, which also lists the HIP
# errors, 1.4e-07 to 4.9e-07). A valid fp32 execution of these networks is that far from fp64.
ORACLE_FLOOR = 1e-6


def _dev():
    return torch.device("cuda", 0)


def _data(shape, classes, n=N, seed=0):
    """Glyph images: one epoch of 10 steps already tells rows apart on them in most cases (on noise every row
    gets the same class), so the hit counts below are counts of distinct decisions."""
    from gentun_amd.utils.data import make_glyph_classification
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=seed, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return x, y, y.argmax(1)


def _noise_data(shape, classes, n, seed=0):
    rng = np.random.default_rng(seed)
    lab = np.arange(n) % classes
    proto = rng.standard_normal((classes,) + shape).astype(np.float32)
    x = (0.5 * proto[lab] + 0.5 * rng.standard_normal((n,) + shape)).astype(np.float32)
    return x, np.eye(classes, dtype=np.float32)[lab], lab


def _model(case, nfold=5, backend="hip", device=None):
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes, genes, bn, dtype, loss = CASES[case]
    x, y, lab = _data(shape, classes)
    m = GeneticCnnModel(x, y, genes, SPACE["nodes"], shape, SPACE["kernels"], SPACE["ks"], SPACE["dense"], 0.5,
                        classes, nfold=nfold, epochs=(1,), learning_rate=(1e-3,), batch_size=BATCH, loss=loss,
                        dtype=dtype, seed=5, backend=backend, device=device or _dev(), batch_norm=bn)
    return m, x, lab


_FITS = {}


def _fit(case):
    """(model, live job, classifier loaded from the saved file, x, labels) of one HIP fit per case."""
    if case not in _FITS:
        import os
        import tempfile
        from gentun_amd.models.cnn_fitted import CnnClassifier
        m, x, lab = _model(case)
        clf = m.fit()
        path = os.path.join(tempfile.mkdtemp(), case + ".npz")
        CnnClassifier.from_job(m.jobs[0], metrics=clf.metrics).save(path)
        _FITS[case] = (m, m.jobs[0], CnnClassifier.load(path), x, lab)
    return _FITS[case]


# ---------------------------------------------------------------------------------------------------------
# the head kernel alone
# ---------------------------------------------------------------------------------------------------------

def _head_predict(plog, b2):
    from gentun_amd.ops import cnn_kernels as K
    G, nt, B, C = plog.shape
    logits = torch.full((G, B, C), float("nan"), dtype=torch.float32, device=plog.device)
    proba = torch.full_like(logits, float("nan"))
    a = K.HeadPredictArgs()
    a.plog, a.b2, a.logits, a.proba = plog.data_ptr(), b2.data_ptr(), logits.data_ptr(), proba.data_ptr()
    a.G, a.B, a.Up, a.C = G, B, nt * 16, C
    K.check(K.lib().gt_head_predict(a, torch.cuda.current_stream(plog.device).cuda_stream), "head_predict")
    torch.cuda.synchronize()
    return logits.cpu().numpy(), proba.cpu().numpy()


@pytest.mark.parametrize("nt", [2, 64, 68])          # Up / 16; 68 tiles: the lane's stride loop runs twice
def test_head_predict_kernel(nt):
    rng = np.random.default_rng(nt)
    G = 2
    for B in (32, 256):
        for C in (2, 3, 10, 16):
            plog = rng.standard_normal((G, nt, B, C)).astype(np.float32)
            b2 = rng.standard_normal((G, C)).astype(np.float32)
            # row 0 of every group: the two last classes tie exactly at the top
            plog[:, :, 0, :] = 0.0
            plog[:, 0, 0, C - 2:] = 7.0
            b2[:, C - 1] = b2[:, C - 2]
            logits, proba = _head_predict(torch.from_numpy(plog).to(_dev()), torch.from_numpy(b2).to(_dev()))
            assert np.isfinite(logits).all() and np.isfinite(proba).all()
            p64 = plog.astype(np.float64)
            ref = p64.sum(1) + b2.astype(np.float64)[:, None, :]
            # at most nt roundings on any path of the reduction (ceil(nt / 64) adds per lane, 6 tree levels of
            # which only those joining non-empty lanes round, + b2), each at most EPS of a partial sum, which
            # is at most the sum of the magnitudes
            bound = nt * EPS * (np.abs(p64).sum(1) + np.abs(b2.astype(np.float64))[:, None, :])
            err = np.abs(logits - ref)
            assert (err <= bound).all(), (B, C, float((err / bound).max()))
            # softmax of the kernel's own logits in fp64. Per probability p = e_c / z: the subtraction of the
            # maximum (EPS |arg|), expf (1 ulp = 2 EPS), both again in z weighted by the probabilities
            # (sum_j p_j |arg_j| <= log C < 3), C - 1 roundings of the sum and one of the division:
            # |dp| <= p EPS (2 + |arg| + 2 + 3 + C - 1 + 1) with p |arg| <= 1 / e: (C + 8) EPS
            lg = logits.astype(np.float64)
            e = np.exp(lg - lg.max(-1, keepdims=True))
            sm = e / e.sum(-1, keepdims=True)
            perr = np.abs(proba - sm).max()
            assert perr <= (C + 8) * EPS, (B, C, perr)
            assert np.abs(proba.astype(np.float64).sum(-1) - 1.0).max() <= (C + 8) * EPS * C
            # the tie: equal logits, equal probabilities, and the label rule (first maximum) picks the lower
            assert (logits[:, 0, C - 2] == logits[:, 0, C - 1]).all()
            assert (logits[:, 0, C - 2] == logits[:, 0].max(-1)).all()
            assert (proba[:, 0, C - 2] == proba[:, 0, C - 1]).all()
            assert (np.argmax(proba[:, 0], -1) == C - 2).all()


def test_head_predict_refuses_what_the_head_refuses():
    from gentun_amd.ops import cnn_kernels as K
    a = K.HeadPredictArgs()
    t = torch.zeros(64, device=_dev())
    a.plog = a.b2 = a.logits = a.proba = t.data_ptr()
    a.G, a.B, a.Up, a.C = 1, 1, 16, 17
    assert K.lib().gt_head_predict(a, 0) != 0          # more than 16 classes: nothing is launched
    a.C, a.Up = 2, 24
    assert K.lib().gt_head_predict(a, 0) != 0          # Up is a whole number of 16-unit tiles


# ---------------------------------------------------------------------------------------------------------
# the predictor scores what the evaluation scored
# ---------------------------------------------------------------------------------------------------------

def _loss64(proba, lab, loss):
    p = proba.astype(np.float64)
    n, C = p.shape
    if loss == "ce":
        return -np.log(np.maximum(p[np.arange(n), lab], 1e-30))
    y = np.eye(C)[lab]
    lo, hi = np.float64(np.float32(1e-7)), np.float64(np.float32(1.0) - np.float32(1e-7))
    pc = np.clip(p, lo, hi)
    return -(y * np.log(pc) + (1.0 - y) * np.log(1.0 - pc)).sum(1) / C


@pytest.mark.parametrize("case", list(CASES))
def test_predictions_are_what_the_fit_evaluated(case):
    m, job, clf, x, lab = _fit(case)
    loss_sum, _binc, catc = (float(t[0]) for t in job._eval)
    proba = clf.predict(x, device=_dev(), output="proba", batch=256)
    label = clf.predict(x, device=_dev(), output="label", batch=256)
    assert proba.shape == (N, CASES[case][1]) and proba.dtype == np.float32 and label.dtype == np.int64
    hits = int((label == lab).sum())
    assert hits == int(catc) and float(int(catc)) == catc
    assert round(clf.metrics["categorical_accuracy"] * N) == hits
    per = _loss64(proba, lab, CASES[case][5])
    # the job's sum: per row the loss in fp32 from the same fp32 probabilities -- per class a clip, 1 - p
    # (EPS absolute), two logf (1 ulp each), products and the running mean over C: at most (C + 4) roundings
    # of magnitude max(1, row loss) -- then an fp64 sum over the n rows rounded once to fp32
    C = CASES[case][1]
    bound = N * (C + 4) * 2 * EPS * max(1.0, float(per.max())) + 2 * EPS * abs(loss_sum)
    print("[cnn-predict] {}: train rows hit {} / {} ({} distinct labels), loss sum job {:.6f} predictor {:.6f} "
          "(bound {:.2e})".format(case, hits, N, len(np.unique(label)), loss_sum, per.sum(), bound))
    assert abs(per.sum() - loss_sum) <= bound


# ---------------------------------------------------------------------------------------------------------
# export / import
# ---------------------------------------------------------------------------------------------------------

def _zero_outside(t, real):
    t = t.clone()
    t[real] = 0
    return not bool(t.any())


@pytest.mark.parametrize("case", ["ones", "mnist", "bn_mnist"])
def test_export_import_is_exact(case):
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, job, clf, x, lab = _fit(case)
    pred = clf.hip_predictor(_dev(), 256)
    pj = pred.job
    assert pj is not job and pj.Q == 1 and pj.stage_cp == job.stage_cp
    mine = {L.name: L for L in pj.layers}
    names = {st.name for st in clf.plan.convs()}
    for L in job.layers:
        P = mine[L.name]
        real = (slice(0, L.cout), slice(None), slice(None), slice(0, L.cin))
        if L.name in names:
            assert torch.equal(P.w[0][0][real], L.w[0][0][real]) and torch.equal(P.b[0][0][:L.cout], L.b[0][0][:L.cout])
            assert bool(P.w[0][0][real].any())
            if job.bn:
                for a, b in ((P.gamma[0][0], L.gamma[0][0]), (P.beta[0][0], L.beta[0][0]),
                             (P.bn_run[0][0], L.bn_run[0][0]), (P.bn_run[1][0], L.bn_run[1][0])):
                    assert torch.equal(a[:L.cout], b[:L.cout])
                assert _zero_outside(P.gamma[0][0], slice(0, L.cout)) and _zero_outside(P.beta[0][0], slice(0, L.cout))
        else:
            real = (slice(0, 0),) * 4                  # a node this genome lacks: all zero
        assert _zero_outside(P.w[0][0], real) and _zero_outside(P.b[0][0], slice(0, L.cout if L.name in names else 0))
    hs, ws = pj.final_hw
    hr, wr = pj.final_hw_real
    cp, Cl, U = pj.final_cp, clf.kernels_per_layer[-1], clf.dense_units
    if case != "ones":
        assert (hs, ws) == (8, 8) and (hr, wr) == (7, 7)         # padded pixels exist
    real = (slice(0, hr), slice(0, wr), slice(0, Cl), slice(0, U))
    W1p, W1j = (j.views["W1"][0][0].view(hs, ws, cp, j.Up) for j in (pj, job))
    assert torch.equal(W1p[real], W1j[real]) and _zero_outside(W1p, real) and pj.Up > U
    for name, real in (("b1", slice(0, U)), ("W2", slice(0, U)), ("b2", slice(None))):
        a, b = pj.views[name][0][0], job.views[name][0][0]
        assert torch.equal(a[real], b[real]) and _zero_outside(a, real)
    # the file holds what the live job holds: a predictor filled from the job gives the same bits
    direct = CnnClassifier.from_job(job)
    assert all(direct.params[k].tobytes() == clf.params[k].tobytes() for k in clf.params)
    a = clf.predict(x[:300], device=_dev(), output="logits", batch=256)
    b = direct.predict(x[:300], device=_dev(), output="logits", batch=256)
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------
# chunking
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["chain", "bn_mnist"])
def test_chunking_does_not_change_a_row(case):
    m, job, clf, x, lab = _fit(case)
    xs = x[:300]                                         # at batch 256: one full chunk and a tail of 44
    a = clf.predict(xs, device=_dev(), output="logits", batch=256)
    assert np.isfinite(a).all() and len(clf._predictors) >= 1
    rev = clf.predict(xs[::-1], device=_dev(), output="logits", batch=256)
    assert rev[::-1].tobytes() == a.tobytes()
    one = clf.predict(xs[7], device=_dev(), output="logits", batch=256)
    assert one.tobytes() == a[7:8].tobytes()
    assert clf.hip_predictor(_dev(), 256) is clf.hip_predictor(_dev(), 255)       # one predictor per (device, EB)
    assert clf.hip_predictor(_dev(), 1).EB == 32 and clf.hip_predictor(_dev(), 1000).EB == 256


# ---------------------------------------------------------------------------------------------------------
# against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------

def _rel(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("case", FP32_CASES)
def test_logits_against_the_fp64_oracle(case):
    """The yardstick of tests/test_hip_step_parity.py: the HIP error, relative to the largest logit, is at
    most 4x the error of the stock-torch fp32 forward on the same GPU against the same fp64 reference (or
    ORACLE_FLOOR). bf16 is a faster, coarser mode and has no fp32 yardstick: it is held to the evaluation
    it reproduces (test_predictions_are_what_the_fit_evaluated)."""
    m, job, clf, x, lab = _fit(case)
    xs = x[:300]
    ref = clf.predict(xs, device="cpu", output="logits", dtype=torch.float64)
    assert ref.dtype == np.float64
    t32 = clf.predict(xs, device=_dev(), output="logits", backend="torch")
    h256 = clf.predict(xs, device=_dev(), output="logits", batch=256)
    h32 = clf.predict(xs, device=_dev(), output="logits", batch=32)
    e_t, e_256, e_32 = _rel(t32, ref), _rel(h256, ref), _rel(h32, ref)
    print("[cnn-predict] {}: rel. logit error vs fp64: HIP batch 256 {:.3e}, batch 32 {:.3e}, torch fp32 (GPU) {:.3e}; "
          "batch 32 and 256 bit-identical: {}".format(case, e_256, e_32, e_t, h32.tobytes() == h256.tobytes()))
    assert max(e_256, e_32) <= max(4 * e_t, ORACLE_FLOOR)


# ---------------------------------------------------------------------------------------------------------
# nothing existing moved; refusal
# ---------------------------------------------------------------------------------------------------------

def test_cross_validate_is_unchanged_by_fit_and_predict():
    m, x, lab = _model("c3", nfold=2)
    first = m.cross_validate()
    scores, metrics = list(m.fold_scores), {k: list(v) for k, v in m.fold_metrics.items()}
    clf = m.fit()
    assert m.predict(x[:40]).shape == (40, 3) and m.fitted is clf
    assert m.fold_scores == scores                       # fit() leaves the CV results alone
    again = m.cross_validate()
    assert again == first and m.fold_scores == scores and m.fold_metrics == metrics


def test_reset_weights_after_fit():
    from gentun_amd.models.cnn_fitted import CnnClassifier
    m, x, lab = _model("c3")
    before = m.fit()
    assert m.reset_weights() == 1
    torch.cuda.synchronize()
    after = CnnClassifier.from_job(m.jobs[0])
    for name in before.params:
        same = np.array_equal(after.params[name], before.params[name])
        assert same == (not name.endswith(".w")), name          # kernels re-drawn, biases kept


def test_more_than_16_classes():
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes = (8, 8, 3), 17
    x, y, lab = _noise_data(shape, classes, n=64)
    kw = dict(nodes=(3,), input_shape=shape, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
              dropout_probability=0.5, classes=classes, nfold=2, epochs=(1,), learning_rate=(1e-3,), batch_size=32)
    with pytest.raises(ValueError, match="16 classes"):
        GeneticCnnModel(x, y, {"S_1": "101"}, backend="hip", device=_dev(), **kw).fit()
    clf = GeneticCnnModel(x, y, {"S_1": "101"}, backend="torch", device="cpu", **kw).fit()
    assert clf.predict(x).shape == (64, 17)
    assert clf.predict(x, device=_dev(), backend="torch").shape == (64, 17)
    with pytest.raises(ValueError, match="16 classes"):
        clf.predict(x, device=_dev())
