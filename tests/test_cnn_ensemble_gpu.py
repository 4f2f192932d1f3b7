"""The fitted Genetic-CNN ensemble on an MI355X: ``gt_head_ensemble`` alone against ``gt_head_predict`` and numpy,
then ``fit_ensemble`` on the HIP executor and ``CnnEnsemble.predict`` through ``HipEnsemblePredictor``
(gentun_amd/models/cnn_ensemble.py) against the members served and fitted alone, the ordered fp32 combine,
the chunking and the fp64 oracle.

Every fit: 320 rows, 1 epoch, batch 32, the three genomes of tests/test_cnn_fitted_gpu.py. One ensemble fit
and three single fits per case, shared by the tests and left unchanged."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, BATCH = 320, 32
CHAIN = {"S_1": "101", "S_2": "1010010001"}
ONES = {"S_1": "111", "S_2": "1111111111"}
MIXED = {"S_1": "101", "S_2": "0101110011"}
GENOMES = [CHAIN, ONES, MIXED]
K3 = len(GENOMES)
# name -> (input shape, classes, batch_norm, dtype, loss)
CASES = {
    "rgb": ((32, 32, 3), 10, False, "fp32", "bce_compat"),
    "bn_mnist": ((28, 28, 1), 10, True, "fp32", "ce"),            # stored 32 x 32; running statistics
    "bf16": ((32, 32, 3), 10, False, "bf16", "bce_compat"),
}
FP32_CASES = [c for c in CASES if CASES[c][3] == "fp32"]
ORACLE_FLOOR = 1e-6          # tests/test_cnn_fitted_gpu.py: the same measurement, the same margin


def _dev():
    return torch.device("cuda", 0)


def _data(shape, classes, n=N, seed=0):
    from gentun_amd.utils.data import make_glyph_classification
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=seed, noise=0.5)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return x, y, y.argmax(1)


def _space(case, nfold=5):
    shape, classes, bn, dtype, loss = CASES[case]
    return dict(nodes=(3, 5), input_shape=shape, kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
                dense_units=500, dropout_probability=0.5, classes=classes, nfold=nfold, epochs=(1,),
                learning_rate=(1e-3,), batch_size=BATCH, loss=loss, dtype=dtype, seed=5, backend="hip",
                batch_norm=bn)


_FITS, _ALONE = {}, {}


def _fit(case):
    """(ensemble, x, labels) of one HIP ensemble fit per case."""
    if case not in _FITS:
        from gentun_amd.models import fit_ensemble
        shape, classes = CASES[case][:2]
        x, y, lab = _data(shape, classes)
        _FITS[case] = (fit_ensemble(x, y, GENOMES, device=_dev(), **_space(case)), x, y, lab)
    return _FITS[case]


def _alone(case):
    """The three classifiers of ``GeneticCnnModel.fit()`` alone, on the ensemble's arrays."""
    if case not in _ALONE:
        from gentun_amd.models.cnn import GeneticCnnModel
        ens, x, y, lab = _fit(case)
        _ALONE[case] = [GeneticCnnModel(x, y, g, device=_dev(), **_space(case)).fit() for g in GENOMES]
    return _ALONE[case]


def _ordered_combine(mp, w):
    """The contract, written out: fp32 products and sums in member order; votes by first maximum."""
    w = np.asarray(w, np.float32)
    acc = np.multiply(w[0], mp[0], dtype=np.float32)
    for g in range(1, len(mp)):
        acc = np.add(acc, np.multiply(w[g], mp[g], dtype=np.float32), dtype=np.float32)
    votes = np.zeros(mp.shape[1:], np.int32)
    for g in range(len(mp)):
        votes[np.arange(mp.shape[1]), np.argmax(mp[g], 1)] += 1
    return acc, votes


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


def _head_ensemble(plog, b2, w, members=True):
    from gentun_amd.ops import cnn_kernels as K
    G, nt, B, C = plog.shape
    logits = torch.full((G, B, C), float("nan"), dtype=torch.float32, device=plog.device)
    proba = torch.full_like(logits, float("nan"))
    ens = torch.full((B, C), float("nan"), dtype=torch.float32, device=plog.device)
    votes = torch.full((B, C), -1, dtype=torch.int32, device=plog.device)
    a = K.HeadEnsembleArgs()
    a.plog, a.b2, a.weight = plog.data_ptr(), b2.data_ptr(), w.data_ptr()
    a.logits, a.proba = (logits.data_ptr(), proba.data_ptr()) if members else (0, 0)
    a.ens, a.votes = ens.data_ptr(), votes.data_ptr()
    a.G, a.B, a.Up, a.C = G, B, nt * 16, C
    K.check(K.lib().gt_head_ensemble(a, torch.cuda.current_stream(plog.device).cuda_stream), "head_ensemble")
    torch.cuda.synchronize()
    return logits.cpu().numpy(), proba.cpu().numpy(), ens.cpu().numpy(), votes.cpu().numpy()


# G = 1, 3: waves without a member still reach the barrier; 5: a wave's member loop runs twice, unevenly;
# 64: the LDS table is full. 68 tiles: the lane's stride loop runs twice.
@pytest.mark.parametrize("nt", [2, 68])
@pytest.mark.parametrize("G", [1, 3, 5, 16, 64])
def test_head_ensemble_kernel(G, nt):
    rng = np.random.default_rng(100 * G + nt)
    for B in (1, 33):
        for C in (1, 3, 16):
            plog = rng.standard_normal((G, nt, B, C)).astype(np.float32)
            b2 = rng.standard_normal((G, C)).astype(np.float32)
            if C >= 2:      # row 0: every member ties its two last classes exactly at the top
                plog[:, :, 0, :] = 0.0
                plog[:, 0, 0, C - 2:] = 7.0
                b2[:, C - 1] = b2[:, C - 2]
            dp, db = torch.from_numpy(plog).to(_dev()), torch.from_numpy(b2).to(_dev())
            ref_logits, ref_proba = _head_predict(dp, db)
            w64 = rng.random(G) + 0.1
            for weights in (np.ones(G), w64):
                w = (weights / weights.sum()).astype(np.float32)
                dw = torch.from_numpy(w).to(_dev())
                logits, proba, ens, votes = _head_ensemble(dp, db, dw)
                assert logits.tobytes() == ref_logits.tobytes(), (B, C)
                assert proba.tobytes() == ref_proba.tobytes(), (B, C)
                want, count = _ordered_combine(ref_proba, w)
                assert ens.tobytes() == want.tobytes(), (B, C, float(np.abs(ens - want).max()))
                assert votes.tobytes() == count.tobytes(), (B, C)
                if C >= 2:
                    assert votes[0, C - 2] == G and (ref_proba[:, 0, C - 2] == ref_proba[:, 0, C - 1]).all()
                # null member pointers: the same mean and votes, nothing else written
                l0, p0, ens0, votes0 = _head_ensemble(dp, db, dw, members=False)
                assert np.isnan(l0).all() and np.isnan(p0).all()
                assert ens0.tobytes() == ens.tobytes() and votes0.tobytes() == votes.tobytes()


def test_head_ensemble_refusals():
    from gentun_amd.ops import cnn_kernels as K
    a = K.HeadEnsembleArgs()
    t = torch.zeros(64, device=_dev())
    a.plog = a.b2 = a.weight = a.logits = a.proba = a.ens = a.votes = t.data_ptr()
    a.G, a.B, a.Up, a.C = 65, 1, 16, 2
    assert K.lib().gt_head_ensemble(a, 0) != 0         # more members than the LDS table holds
    a.G, a.C = 1, 17
    assert K.lib().gt_head_ensemble(a, 0) != 0         # more than 16 classes
    a.C, a.Up = 2, 24
    assert K.lib().gt_head_ensemble(a, 0) != 0         # Up is a whole number of 16-unit tiles
    a.Up, a.B = 16, 0
    assert K.lib().gt_head_ensemble(a, 0) != 0         # no row
    torch.cuda.synchronize()
    assert not bool(t.any())                           # nothing was launched


# ---------------------------------------------------------------------------------------------------------
# A. a member in the ensemble's launches is the member served alone
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_members_equal_their_own_predictor(case):
    ens, x, y, lab = _fit(case)
    xs = x[:300]                                         # at 256 rows per launch: one full chunk, a tail of 44
    pred = ens.hip_predictor(_dev(), 256)
    # the BatchNorm twins of three groups do not fit the budget at 256 rows: the executor's rule lowers them
    assert pred.EB == pred.job.eval_batch() and pred.EB % 32 == 0 and (pred.EB == 256 or CASES[case][2])
    assert pred.stage.shape[0] == pred.EB and pred.job.Q == K3 and ens.hip_predictor(_dev(), 255) is pred
    print("[cnn-ensemble] {}: {} rows per launch".format(case, pred.EB))
    out = ens.predict_outputs(xs, device=_dev(), batch=256)
    assert out["member_logits"].shape == (K3, 300, 10) and out["member_logits"].dtype == np.float32
    assert np.isfinite(out["member_logits"]).all()
    for g, m in enumerate(ens.members):
        assert out["member_logits"][g].tobytes() == m.predict(xs, device=_dev(), output="logits", batch=pred.EB).tobytes()
        assert out["member_proba"][g].tobytes() == m.predict(xs, device=_dev(), output="proba", batch=pred.EB).tobytes()
    # the members differ: the groups are not copies of one another
    assert not np.array_equal(out["member_logits"][0], out["member_logits"][1])


def test_rows_per_launch_follow_the_twin_budget(monkeypatch):
    from gentun_amd.models import CnnEnsemble
    from gentun_amd.models import cnn_hip
    fitted, x, y, lab = _fit("rgb")
    job = fitted.hip_predictor(_dev(), 256).job
    per_img = sum(t[0, 0].numel() * t.element_size() for t in list(job.act.values()) + list(job.zpre.values()))
    per_img += job.Up * 4 * 2
    monkeypatch.setattr(cnn_hip, "EVAL_TWIN_BUDGET", per_img * K3 * 64 + 1)       # 64 rows of 3 groups fit, 96 do not
    ens = CnnEnsemble(fitted.members, weights=fitted.weights)
    pred = ens.hip_predictor(_dev(), 256)
    assert pred.EB == 64 and pred.stage.shape[0] == 64 and ens.hip_predictor(_dev(), 64) is pred
    assert ens.hip_predictor(_dev(), 32).EB == 32
    xs = x[:100]
    got = ens.predict(xs, device=_dev(), output="member_logits", batch=256)
    for g, m in enumerate(ens.members):
        assert got[g].tobytes() == m.predict(xs, device=_dev(), output="logits", batch=pred.EB).tobytes()
    monkeypatch.setattr(cnn_hip, "EVAL_TWIN_BUDGET", 1)                           # never below 32
    assert CnnEnsemble(fitted.members).hip_predictor(_dev(), 256).EB == 32


# ---------------------------------------------------------------------------------------------------------
# B. the combination
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_combine_on_the_device_is_the_ordered_fp32_combine(case):
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = _fit(case)
    xs = x[:300]
    for weights in (None, [3.0, 1.0, 4.0], [1, 0, 0]):
        ens = fitted if weights is None else CnnEnsemble(fitted.members, weights=weights)
        out = ens.predict_outputs(xs, device=_dev(), batch=256)
        proba, votes = _ordered_combine(out["member_proba"], ens.weights)
        assert out["proba"].dtype == np.float32 and out["proba"].tobytes() == proba.tobytes()
        assert out["votes"].dtype == np.int32 and out["votes"].tobytes() == votes.tobytes()
        assert np.array_equal(out["label"], np.argmax(proba, 1)) and out["label"].dtype == np.int64
        assert ens.predict(xs, device=_dev(), output="proba").tobytes() == proba.tobytes()     # null member pointers
        assert ens.predict(xs, device=_dev(), output="votes").tobytes() == votes.tobytes()
        if weights == [1, 0, 0]:
            assert out["proba"].tobytes() == ens.members[0].predict(xs, device=_dev()).tobytes()
    one = CnnEnsemble([fitted.members[2]])
    alone = fitted.members[2].predict(xs, device=_dev(), batch=256)
    assert one.predict(xs, device=_dev(), batch=256).tobytes() == alone.tobytes()
    assert np.array_equal(one.predict(xs, device=_dev(), output="vote_label"), np.argmax(alone, 1))
    hits = int((fitted.predict(x, device=_dev(), output="label") == lab).sum())
    assert fitted.metrics["rows"] == N and fitted.metrics["categorical_accuracy"] == hits / float(N)
    print("[cnn-ensemble] {}: train rows hit by the mean {} / {}, by the members {}".format(
        case, hits, N, [round(m.metrics["categorical_accuracy"] * N) for m in fitted.members]))


# ---------------------------------------------------------------------------------------------------------
# C. a member fitted in the ensemble's population job is the member fitted alone
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", FP32_CASES)
def test_members_equal_their_fit_alone(case):
    ens, x, y, lab = _fit(case)
    for g, (member, alone) in enumerate(zip(ens.members, _alone(case))):
        assert member.genes == alone.genes == GENOMES[g]
        assert sorted(member.params) == sorted(alone.params)
        for name, _ in alone.param_shapes():             # forward order: the first differing layer is named
            assert member.params[name].tobytes() == alone.params[name].tobytes(), (g, name)
        assert member.metrics == alone.metrics


def test_cross_validate_is_unchanged_by_fit_ensemble():
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes = (28, 28, 1), 3
    x, y, lab = _data(shape, classes)
    space = dict(_space("rgb", nfold=2), input_shape=shape, classes=classes)
    m = GeneticCnnModel(x, y, CHAIN, device=_dev(), **space)
    first = m.cross_validate()
    scores = list(m.fold_scores)
    ens = fit_ensemble(x, y, GENOMES[:2], device=_dev(), **space)
    assert ens.predict(x[:40], device=_dev()).shape == (40, 3)
    assert m.cross_validate() == first and m.fold_scores == scores


# ---------------------------------------------------------------------------------------------------------
# D. chunking
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_chunking_does_not_change_a_row(case):
    ens, x, y, lab = _fit(case)
    xs = x[:70]
    a = ens.predict_outputs(xs, device=_dev(), batch=32)
    b = ens.predict_outputs(xs, device=_dev(), batch=256)
    perm = np.random.default_rng(1).permutation(70)
    c = ens.predict_outputs(xs[perm], device=_dev(), batch=32)
    assert ens.hip_predictor(_dev(), 32).EB == 32 and ens.hip_predictor(_dev(), 256).EB > 32
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
        back = np.empty_like(c[name])
        if name.startswith("member_"):
            back[:, perm] = c[name]
        else:
            back[perm] = c[name]
        assert back.tobytes() == a[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------
# E. against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------

def _rel(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("case", FP32_CASES)
def test_member_logits_against_the_fp64_oracle(case):
    """The bound of tests/test_cnn_fitted_gpu.py: relative to the largest logit, at most 4x the error of the
    stock-torch fp32 forward on the same GPU against the same fp64 reference (or ORACLE_FLOOR)."""
    ens, x, y, lab = _fit(case)
    xs = x[:128]                                         # three fp64 forwards on the CPU: fewer rows, the same bound
    got = ens.predict(xs, device=_dev(), output="member_logits", batch=256)
    for g, m in enumerate(ens.members):
        ref = m.predict(xs, device="cpu", output="logits", dtype=torch.float64)
        t32 = m.predict(xs, device=_dev(), output="logits", backend="torch")
        e_t, e_h = _rel(t32, ref), _rel(got[g], ref)
        print("[cnn-ensemble] {} member {}: rel. logit error vs fp64: HIP ensemble {:.3e}, torch fp32 (GPU) {:.3e}".format(
            case, g, e_h, e_t))
        assert e_h <= max(4 * e_t, ORACLE_FLOOR)


# ---------------------------------------------------------------------------------------------------------
# refusal
# ---------------------------------------------------------------------------------------------------------

def test_more_than_16_classes():
    from gentun_amd.models import fit_ensemble
    shape, classes = (8, 8, 3), 17
    rng = np.random.default_rng(0)
    lab = np.arange(64) % classes
    x = rng.standard_normal((64,) + shape).astype(np.float32)
    y = np.eye(classes, dtype=np.float32)[lab]
    kw = dict(nodes=(3,), input_shape=shape, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
              dropout_probability=0.5, classes=classes, nfold=2, epochs=(1,), learning_rate=(1e-3,), batch_size=32)
    genomes = [{"S_1": "101"}, {"S_1": "111"}]
    with pytest.raises(ValueError, match="16 classes"):
        fit_ensemble(x, y, genomes, backend="hip", device=_dev(), **kw)
    ens = fit_ensemble(x, y, genomes, backend="torch", device="cpu", **kw)
    assert ens.predict(x).shape == (64, 17)
    assert ens.predict(x, device=_dev(), backend="torch").shape == (64, 17)
    with pytest.raises(ValueError, match="16 classes"):
        ens.predict(x, device=_dev())
