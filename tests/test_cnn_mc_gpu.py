"""Monte-Carlo dropout of fitted Genetic-CNN models on an MI355X: ``gt_head_mc`` (csrc/hip/cnn_head_mc.hip) alone
on synthetic buffers against the fp64 oracle of tests/mc_ref.py, then ``predict_mc(device=cuda)`` of
``CnnClassifier`` and ``CnnEnsemble`` through the HIP predictors against the oracle fed the predictor's own hidden
buffer after a plain forward of the same chunk.

The error of an output is ``E = max |diff| / max |oracle|`` and the assertion ``E_hip <= 4 * max(E_torch, 2^-23)``,
``E_torch`` being the same quantity from stock-torch fp32 operations on the same GPU under the same masks (the
yardstick of the Grad-CAM and soft-head tests; the floor is one fp32 ulp of 1). Where the oracle's output is zero
(``std`` and ``mutual_info`` of one member without dropout or with one sample; they and the entropies with one
class) ``E`` has no denominator: there ``max |output| <= 4 * 2^-23`` is asserted instead, the CPU test's rule for
that case. The fits are those of tests/test_cnn_fitted_gpu.py and tests/test_cnn_ensemble_gpu.py (shared inside
one pytest process, left unchanged)."""

import numpy as np
import pytest
import torch

import mc_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F
import test_cnn_gradcam_gpu as Gc

pytestmark = pytest.mark.gpu

GUARD = 512                  # elements past an output: all stay NaN
HB = 64                      # launch rows
ULP = 2.0 ** -23
NAMES = ("proba", "std", "entropy", "expected_entropy", "mutual_info", "samples")
NROWS = 70


def _dev():
    return torch.device("cuda", 0)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _check(tag, got, h, W2, b2, w, T, dropout, seed, rows, Ur, names=NAMES):
    """``got`` (the kernel's outputs of ``rows``) against the oracle of ``h [G, n, U]``, next to stock torch in fp32
    on the GPU from the same masks and the shared fp32 statistics."""
    from gentun_amd.models.cnn_fitted import mc_keep_scale, mc_statistics
    from gentun_amd.utils.rng import mc_masks
    G = h.shape[0]
    want = R.oracle(h, W2, b2, w, T, dropout, seed, rows, units=Ur)
    p32 = []
    for g in range(G):
        keep = torch.from_numpy(mc_masks(seed, g, T, rows, Ur, dropout)).to(_dev())
        hg = torch.from_numpy(np.ascontiguousarray(h[g][:, :Ur])).to(_dev()) * float(mc_keep_scale(dropout))
        z = torch.where(keep, hg[None], torch.zeros_like(hg)[None]) @ torch.from_numpy(W2[g][:Ur]).to(_dev())
        p32.append(torch.softmax(z + torch.from_numpy(b2[g]).to(_dev()), -1).permute(1, 0, 2).cpu().numpy())
    t32 = mc_statistics(np.stack(p32), w)
    t32["samples"] = np.stack(p32).transpose(1, 0, 2, 3)
    for name in names:
        assert np.isfinite(got[name]).all(), (tag, name)
        if np.abs(want[name]).max() <= 1e-12:                # zero but for fp64 rounding: E has no denominator
            print("[cnn-mc] {} {} where the oracle's is zero: HIP {:.3e}".format(tag, name, float(np.abs(got[name]).max())))
            assert np.abs(got[name]).max() <= 4 * ULP, (tag, name)
            continue
        e_hip, e_torch = _rel(got[name], want[name]), _rel(t32[name], want[name])
        print("[cnn-mc] {} {} vs fp64: HIP {:.3e}, torch fp32 (GPU) {:.3e}".format(tag, name, e_hip, e_torch))
        assert e_hip <= 4 * max(e_torch, ULP), (tag, name)
    return want


# ---------------------------------------------------------------------------------------------------------
# gt_head_mc alone
# ---------------------------------------------------------------------------------------------------------

class _Mc(object):
    """Synthetic buffers of one launch: ``h = relu(N(0, 1))`` (half exact zeros) in ``dtype``, ``W2 ~ N(0, 1)``,
    NaN in the padded units of both, unequal weights, NaN-filled outputs with a guard tail."""

    def __init__(self, Up=64, Ur=50, C=10, T=16, G=1, m=33, n0=0, dropout=0.5, dtype=torch.float32, seed=7):
        self.kw = dict(Up=Up, Ur=Ur, C=C, T=T, G=G, m=m, n0=n0, dropout=dropout, seed=seed)
        self.dtype = dtype
        rng = np.random.default_rng(Up + C + T + G)
        h = np.maximum(rng.standard_normal((G, HB, Up)), 0).astype(np.float32)
        W2 = rng.standard_normal((G, Up, C)).astype(np.float32)
        h[:, :, Ur:], W2[:, Ur:] = np.nan, np.nan
        self.h = torch.from_numpy(h).to(device=_dev(), dtype=dtype)
        self.W2 = torch.from_numpy(W2).to(_dev())
        self.b2 = torch.from_numpy(rng.standard_normal((G, C)).astype(np.float32)).to(_dev())
        w = rng.random(G) + 0.1
        self.w = (w / w.sum()).astype(np.float32)
        self.weight = torch.from_numpy(self.w).to(_dev())
        self.fresh()

    def fresh(self):
        k, nan = self.kw, float("nan")
        self.out = {"proba": torch.full((HB * k["C"] + GUARD,), nan, device=_dev()),
                    "std": torch.full((HB * k["C"] + GUARD,), nan, device=_dev()),
                    "entropy": torch.full((HB + GUARD,), nan, device=_dev()),
                    "expected_entropy": torch.full((HB + GUARD,), nan, device=_dev()),
                    "mutual_info": torch.full((HB + GUARD,), nan, device=_dev()),
                    "samples": torch.full((HB * k["G"] * k["T"] * k["C"] + GUARD,), nan, device=_dev())}
        self.label = torch.full((HB + GUARD,), -7, dtype=torch.int32, device=_dev())

    def launch(self, over=()):
        from gentun_amd.models.cnn_fitted import mc_keep_scale
        from gentun_amd.ops import cnn_kernels as K
        from gentun_amd.utils.rng import mc_threshold
        k = self.kw
        a = K.HeadMcArgs()
        a.h, a.w2, a.b2, a.weight = self.h.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.weight.data_ptr()
        for name, t in self.out.items():
            setattr(a, name, t.data_ptr())
        a.label = self.label.data_ptr()
        a.G, a.B, a.Up, a.Ur, a.C, a.T, a.m = k["G"], HB, k["Up"], k["Ur"], k["C"], k["T"], k["m"]
        a.prec = 1 if self.dtype == torch.float32 else 0
        a.thr, a.seed, a.n0 = mc_threshold(k["dropout"]), k["seed"], k["n0"]
        a.keep_scale, a.inv_T = float(mc_keep_scale(k["dropout"])), float(np.float32(1) / np.float32(k["T"]))
        for name, v in dict(over).items():
            setattr(a, name, v)
        rc = K.lib().gt_head_mc(a, torch.cuda.current_stream(_dev()).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool(all(torch.isnan(t).all() for t in self.out.values()) and (self.label == -7).all())

    def host(self):
        """The outputs' written parts as host arrays; everything past them must still hold the fill."""
        k = self.kw
        m, C, G, T = k["m"], k["C"], k["G"], k["T"]
        shapes = {"proba": (m, C), "std": (m, C), "entropy": (m,), "expected_entropy": (m,), "mutual_info": (m,),
                  "samples": (m, G, T, C)}
        sizes = {name: int(np.prod(shape)) for name, shape in shapes.items()}
        got = {}
        for name, t in self.out.items():
            flat = t.cpu().numpy()
            assert np.isnan(flat[sizes[name]:]).all(), (name, "rows >= m or the guard tail")
            got[name] = flat[:sizes[name]].reshape(shapes[name])
        label = self.label.cpu().numpy()
        assert (label[m:] == -7).all()
        got["label"] = label[:m]
        return got


BASE = dict()
CASES = [BASE, dict(Up=576, Ur=500), dict(C=1), dict(C=16), dict(T=1), dict(T=17), dict(T=64), dict(G=3),
         dict(G=64, m=5), dict(m=1), dict(n0=1000), dict(dropout=0.0), dict(dropout=0.3),
         dict(dtype=torch.bfloat16), dict(dtype=torch.bfloat16, dropout=0.3),
         dict(Up=576, Ur=500, C=16, T=64, G=3, m=33, n0=1000, dropout=0.3, dtype=torch.bfloat16)]


@pytest.mark.parametrize("kw", CASES, ids=["-".join("{}{}".format(k, v) for k, v in c.items()).replace("torch.", "")
                                           or "base" for c in CASES])
def test_head_mc_kernel(kw):
    c = _Mc(**kw)
    k = c.kw
    assert c.launch() == 0
    got = c.host()
    h = c.h.float().cpu().numpy()[:, :k["m"]]
    _check(str(kw), got, h, c.W2.cpu().numpy(), c.b2.cpu().numpy(), c.w, k["T"], k["dropout"], k["seed"],
           k["n0"] + np.arange(k["m"]), k["Ur"])
    assert np.array_equal(got["label"], np.argmax(got["proba"], 1))              # the first maximum of its own proba
    first = {name: v.copy() for name, v in got.items()}
    c.fresh()
    assert c.launch() == 0
    again = c.host()
    assert all(again[name].tobytes() == first[name].tobytes() for name in first)
    c.fresh()
    assert c.launch(over=dict(samples=0)) == 0 and torch.isnan(c.out["samples"]).all()    # samples may be null
    assert c.out["proba"].cpu().numpy()[:k["m"] * k["C"]].tobytes() == first["proba"].tobytes()


def test_head_mc_refusals():
    from gentun_amd.ops import cnn_kernels as K
    c = _Mc(G=3)
    for kw in (dict(h=0), dict(w2=0), dict(b2=0), dict(weight=0), dict(proba=0), dict(std=0), dict(entropy=0),
               dict(expected_entropy=0), dict(mutual_info=0), dict(label=0), dict(C=0), dict(C=17), dict(G=0), dict(G=65), dict(Up=32),
               dict(Up=96), dict(Up=0), dict(Up=4160), dict(Ur=0), dict(Ur=65), dict(T=0), dict(T=65), dict(m=0),
               dict(m=-1), dict(m=HB + 1), dict(prec=2), dict(prec=-1), dict(keep_scale=float("inf")),
               dict(keep_scale=float("nan"))):
        assert c.launch(over=kw) != 0, kw
        assert c.untouched(), kw
    assert K.lib().gt_head_mc(None, torch.cuda.current_stream(_dev()).cuda_stream) != 0
    assert c.launch(over=dict(m=HB)) == 0 and not torch.isnan(c.out["entropy"][:HB]).any()     # the edge m = B


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------

def _hidden(pred, xs, G):
    """The predictor's own hidden buffer ``[G, n, Up]`` after a plain forward of every chunk of ``xs``."""
    return np.concatenate([chunk[3] for chunk in Gc._plain_chunks(pred, xs, G)], axis=1)


def _against_the_oracle(obj, pred, xs, G, w, dropout, tag):
    """``predict_mc`` at the predictor's rows per launch against the oracle fed the predictor's own hidden buffer
    (``expected_entropy`` is not returned: the kernel test covers it)."""
    job = pred.job
    got = obj.predict_mc(xs, samples=17, dropout=dropout, seed=5, device=_dev(), batch=pred.EB, return_samples=True)
    assert got["label"].dtype == np.int64 and np.array_equal(got["label"], np.argmax(got["proba"], 1))
    W2 = Gc._f32(job.views["W2"][0]).reshape(G, job.Up, -1)
    b2 = Gc._f32(job.views["b2"][0]).reshape(G, -1)
    want = _check(tag, got, _hidden(pred, xs, G), W2, b2, w, 17, dropout, 5, np.arange(len(xs)),
                  job.members[0][0].dense_units, names=("proba", "std", "entropy", "mutual_info", "samples"))
    return got, want


@pytest.mark.parametrize("case", ["chain", "bf16"])
def test_classifier_against_the_oracle_of_its_own_hidden_buffer(case):
    m, job, clf, x, lab = F._fit(case)
    xs = x[10:10 + NROWS]
    one = np.ones(1, np.float32)
    pred = clf.hip_predictor(_dev(), 32)
    got, want = _against_the_oracle(clf, pred, xs, 1, one, 0.5, case)
    assert want["std"].max() > 100 * ULP                     # the samples differ by far more than rounding
    big = clf.predict_mc(xs, samples=17, dropout=0.5, seed=5, device=_dev(), batch=256, return_samples=True)
    assert all(big[name].tobytes() == got[name].tobytes() for name in big)      # batch 32 = batch 256
    assert m.predict_mc(xs[:5], samples=17, seed=5)["std"].tobytes() == got["std"][:5].tobytes()  # the model forwards
    # without dropout: proba as close to the oracle as predict's own proba
    none = clf.predict_mc(xs, samples=3, dropout=0, device=_dev(), batch=32)
    ref = R.oracle(_hidden(pred, xs, 1), Gc._f32(pred.job.views["W2"][0]).reshape(1, pred.job.Up, -1),
                   Gc._f32(pred.job.views["b2"][0]).reshape(1, -1), one, 1, 0.0, 0, np.arange(NROWS),
                   units=clf.dense_units)["proba"]
    e_mc, e_plain = _rel(none["proba"], ref), _rel(clf.predict(xs, device=_dev(), batch=32), ref)
    print("[cnn-mc] {} no dropout, proba vs fp64: predict_mc {:.3e}, predict {:.3e}".format(case, e_mc, e_plain))
    assert e_mc <= 4 * max(e_plain, ULP) and none["std"].max() <= 4 * ULP and none["mutual_info"].max() <= 4 * ULP


def test_ensemble_of_three_against_the_oracle():
    from gentun_amd.models import CnnEnsemble
    fitted, x, y, lab = E._fit("rgb")
    ens = CnnEnsemble(fitted.members, weights=[3.0, 1.0, 4.0])
    pred = ens.hip_predictor(_dev(), 256)
    _against_the_oracle(ens, pred, x[10:10 + NROWS], 3, ens.weights, 0.5, "ens3")


def test_ensemble_of_sixteen_is_the_combination_of_its_members_samples():
    import test_cnn_occlusion_gpu as O
    import test_cnn_tta_gpu as T
    from gentun_amd.models import fit_ensemble
    from gentun_amd.models.cnn_fitted import mc_statistics
    shape, classes = E.CASES["rgb"][:2]
    x, y, lab = E._data(shape, classes)
    if "ens" not in O._SIXTEEN:
        O._SIXTEEN["ens"] = fit_ensemble(x, y, T._genomes16(), device=_dev(), **E._space("rgb"))
    ens = O._SIXTEEN["ens"]
    xs = x[10:10 + NROWS]
    got = ens.predict_mc(xs, samples=8, seed=2, device=_dev(), return_samples=True)
    pred = ens.hip_predictor(_dev(), 256)
    assert 32 <= pred.EB < NROWS and got["samples"].shape == (NROWS, 16, 8, classes)
    # the statistics in fp64 of the kernel's own samples: a few fp32 roundings of values of at most 1 away
    want = mc_statistics(got["samples"].transpose(1, 0, 2, 3).astype(np.float64), ens.weights)
    for name in ("proba", "std"):
        assert np.abs(got[name] - want[name]).max() <= 4 * ULP, name
    # member 0 draws in the ensemble what it draws alone (member index 0) at the same rows per launch
    alone = ens.members[0].predict_mc(xs, samples=8, seed=2, device=_dev(), batch=pred.EB, return_samples=True)
    assert alone["samples"][:, 0].tobytes() == got["samples"][:, 0].tobytes()
    assert alone["samples"][:, 0].tobytes() != got["samples"][:, 1].tobytes()


@pytest.mark.parametrize("case", ["mnist", "bf16"])
def test_the_other_paths_are_unchanged_by_predict_mc(case):
    m, job, clf, x, lab = F._fit(case)
    xs = x[:NROWS]

    def others():
        return [clf.predict(xs, device=_dev(), output="logits"), clf.predict(xs, device=_dev(), tta={"flip": True}),
                clf.gradcam(xs[:8], device=_dev())]
    before = others()
    first = clf.predict_mc(xs, device=_dev())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, others()))
    assert clf.predict_mc(xs, device=_dev())["std"].tobytes() == first["std"].tobytes()


def test_cross_validate_is_unchanged_by_predict_mc():
    m, x, lab = F._model("c3", nfold=2)
    first = m.cross_validate()
    scores = list(m.fold_scores)
    m.fit()
    assert m.predict_mc(x[:4])["proba"].shape == (4, 3)
    assert m.cross_validate() == first and m.fold_scores == scores


def test_more_than_16_classes():
    from gentun_amd.models.cnn import GeneticCnnModel
    shape, classes = (8, 8, 3), 17
    x, y, lab = F._noise_data(shape, classes, n=64)
    kw = dict(nodes=(3,), input_shape=shape, kernels_per_layer=(4,), kernel_sizes=((3, 3),), dense_units=16,
              dropout_probability=0.5, classes=classes, nfold=2, epochs=(1,), learning_rate=(1e-3,), batch_size=32)
    clf = GeneticCnnModel(x, y, {"S_1": "101"}, backend="torch", device="cpu", **kw).fit()
    assert clf.predict_mc(x[:4], device=_dev(), backend="torch")["proba"].shape == (4, 17)
    with pytest.raises(ValueError, match="16 classes"):
        clf.predict_mc(x[:4], device=_dev())
