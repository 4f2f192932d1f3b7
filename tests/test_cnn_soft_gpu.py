"""Soft-target training on an MI355X: ``gt_head_soft`` (csrc/hip/cnn_dense.hip) alone on synthetic buffers, then
inside the HIP executor (gentun_amd/models/cnn_hip.py) and through ``distill``.

The kernel's buffers are built as tests/test_hip_kernels.py::test_head builds them; the fits are the smallest the
fitted-model GPU tests use (tests/test_cnn_fitted_gpu.py: 320 rows, 1 epoch, batch 32; the plain fits are shared
with that file inside one pytest process and left unchanged). The fp64 oracle is tests/soft_ref.py."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import soft_ref as R

pytestmark = pytest.mark.gpu

EPS = 0.1
NAN = float("nan")


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------

class _Head(object):
    """Synthetic buffers of one head launch. ``plog`` holds random partial logits in every tile (``saturated``:
    logits of +/-40 in tile 0, so probabilities leave bce_compat's clip range); ``valid`` marks a short batch."""

    OUTS = ("dz", "dH", "gw2", "gb2", "gb1", "dHp")

    def __init__(self, G, B, Up, C, prec, loss, seed=0, N=50, saturated=False, short=True, std=1.0, guard=0):
        from gentun_amd.ops import cnn_kernels as K
        self.K, self.dims, self.prec, self.guard = K, (G, B, Up, C), prec, guard
        dev, nt = _dev(), Up // 16
        g = torch.Generator(device="cpu").manual_seed(seed)
        h = F.relu(torch.randn(G, B, Up, generator=g))
        self.h = (h if prec else h.to(torch.bfloat16)).contiguous().to(dev)
        self.w2 = (torch.randn(G, Up, C, generator=g) * 0.05).to(dev)
        self.b2 = (torch.randn(G, C, generator=g) * 0.1).to(dev)
        if saturated:
            plog = torch.zeros(G, nt, B, C)
            plog[:, 0] = torch.where(torch.rand(G, B, C, generator=g) < 0.5, -40.0, 40.0)
        else:
            plog = torch.randn(G, nt, B, C, generator=g) * (std / nt ** 0.5)
        self.plog = plog.contiguous().to(dev)
        self.labels_cpu = torch.randint(0, C, (N,), generator=g)
        self.labels = self.labels_cpu.to(dev)
        self.gather_cpu = torch.randint(0, N, (1, G, B), generator=g)
        self.gather = self.gather_cpu.to(dev)
        self.nvalid = [max(0, B - 3 - q) for q in range(G)] if short else [B] * G
        self.valid = torch.tensor([self.nvalid], dtype=torch.int32, device=dev)
        self.st = torch.zeros(8, dtype=torch.int32, device=dev)
        self.N = N
        self.fresh()

    def fresh(self):
        G, B, Up, C = self.dims
        dev, npl = _dev(), 3 if self.prec else 1
        self.dz = torch.full((G * B * C + self.guard,), NAN, device=dev)
        self.dH = torch.full((G, B, Up), NAN, device=dev)
        self.gw2 = torch.full((G, Up, C), NAN, device=dev)
        self.gb2 = torch.full((G, C), NAN, device=dev)
        self.gb1 = torch.full((G, Up), NAN, device=dev)
        self.dHp = torch.full((npl, G, B, Up), -1, dtype=torch.int16, device=dev)

    def args(self, loss):
        a = self.K.HeadArgs()
        a.h, a.w2, a.b2 = self.h.data_ptr(), self.w2.data_ptr(), self.b2.data_ptr()
        a.labels, a.gather, a.st = self.labels.data_ptr(), self.gather.data_ptr(), self.st.data_ptr()
        a.dH, a.gw2, a.gb2, a.gb1 = self.dH.data_ptr(), self.gw2.data_ptr(), self.gb2.data_ptr(), self.gb1.data_ptr()
        a.eval_out, a.dz, a.plog = 0, self.dz.data_ptr(), self.plog.data_ptr()
        a.G, a.B, a.Up, a.C = self.dims
        a.loss_ce, a.drop_scale, a.eval, a.prec = int(loss == "ce"), 2.0, 0, self.prec
        a.valid, a.valid_norm, a.dHp = self.valid.data_ptr(), 0, self.dHp.data_ptr()
        return a

    def soft_args(self, loss, table=None, t_on=1.0, t_off=0.0):
        s = self.K.HeadSoftArgs()
        s.head = self.args(loss)
        s.soft = table.data_ptr() if table is not None else 0
        s.t_on, s.t_off = t_on, t_off
        return s

    def outputs(self):
        torch.cuda.synchronize()
        return {k: _bits(getattr(self, k)) for k in self.OUTS}

    def onehot_table(self):
        return F.one_hot(self.labels_cpu, self.dims[3]).float().contiguous().to(_dev())

    def logits64(self):
        return (self.plog.double().sum(1) + self.b2.double()[:, None, :]).cpu().numpy()


@pytest.mark.parametrize("prec", [1, 0], ids=["fp32", "bf16"])
@pytest.mark.parametrize("loss", ["ce", "bce_compat"])
@pytest.mark.parametrize("dims", [(1, 1, 32, 1), (3, 33, 1088, 16), (2, 64, 512, 10)])
def test_one_hot_targets_reproduce_gt_head_bit_for_bit(dims, loss, prec):
    """An exact one-hot table, and smoothing with t_on = 1, t_off = 0: every output of the launch pair (dz, dH,
    gw2, gb2, gb1, the dHp planes) byte-equal to gt_head's, with a short batch and with saturated logits."""
    for saturated in (False, True):
        b = _Head(*dims, prec=prec, loss=loss, seed=dims[1], saturated=saturated)
        L = b.K.lib()
        b.K.check(L.gt_head(b.args(loss), _stream()), "head")
        want = b.outputs()
        if dims[1] > 3:
            assert np.isfinite(np.frombuffer(want["dz"], np.float32)).all()
        table = b.onehot_table()
        for s in (dict(table=table), dict(t_on=1.0, t_off=0.0)):
            b.fresh()
            b.K.check(L.gt_head_soft(b.soft_args(loss, **s), _stream()), "head_soft")
            got = b.outputs()
            for k in b.OUTS:
                assert got[k] == want[k], (k, saturated, sorted(s))
        if saturated and loss == "bce_compat" and dims[3] > 1:
            # the clipped branch did run: a saturated class has dp = 0, so some row's dz is exactly zero
            p = torch.softmax(torch.from_numpy(b.logits64()), -1)
            assert ((p < 1e-7) | (p > 1 - 1e-7)).any()


@pytest.mark.parametrize("loss", ["ce", "bce_compat"])
@pytest.mark.parametrize("kind", ["table", "eps0.1", "eps0.9"])
def test_dz_error_against_the_oracle_is_stock_torch_level(kind, loss):
    """``max|dz - dz_fp64| / max|dz_fp64|`` of the kernel and of stock-torch fp32 autograd of ``loss_and_metrics``
    on the same GPU, both from the same fp32 partial logits: E_hip <= 4 * E_torch (the yardstick of
    tests/test_cnn_fitted_gpu.py). The logits are drawn with standard deviation 2 and every probability lies in
    [1e-5, 1 - 1e-5] (asserted on the fp64 side), so no probability comes near bce_compat's clip bounds."""
    from gentun_amd.models.cnn_engine import loss_and_metrics, smoothing_targets
    G, B, Up, C = 2, 32, 512, 10
    b = _Head(G, B, Up, C, prec=1, loss=loss, seed=11, std=2.0)
    rng = np.random.default_rng(3)
    labels, sids = b.labels_cpu.numpy(), b.gather_cpu.numpy()[0]
    table = R.random_table(rng, b.N, C, labels, peak=0.3)
    eps = float(kind[3:]) if kind.startswith("eps") else 0.0
    z64 = b.logits64()
    p64 = np.stack([[R.softmax(z64[g, r]) for r in range(B)] for g in range(G)])
    assert p64.min() >= 1e-5 and p64.max() <= 1 - 1e-5, (p64.min(), p64.max())
    assert 1.5 < z64.std() < 2.5
    want = np.zeros((G, B, C))
    targets = np.zeros((G, B, C))
    for g in range(G):
        targets[g] = R.target_rows(labels, sids[g], C, table=table if kind == "table" else None, eps=eps)
        want[g] = R.batch_dz(z64[g], targets[g], loss, nvalid=b.nvalid[g])
    # the kernel
    tab_t = torch.from_numpy(table).to(_dev())
    t_on, t_off = smoothing_targets(eps, C) if eps else (1.0, 0.0)
    s = b.soft_args(loss, table=tab_t if kind == "table" else None, t_on=float(t_on), t_off=float(t_off))
    b.K.check(b.K.lib().gt_head_soft(s, _stream()), "head_soft")
    torch.cuda.synchronize()
    got = b.dz.view(G, B, C).double().cpu().numpy()
    # stock torch, fp32, same GPU: the logits summed from the same partial logits, the executor's own weighting
    logits = (b.plog.sum(1) + b.b2[:, None, :]).detach().requires_grad_(True)
    tt = torch.from_numpy(targets.astype(np.float32)).to(_dev())       # the fp32 targets, exactly
    assert np.array_equal(tt.double().cpu().numpy(), targets)
    per, _, _ = loss_and_metrics(logits, tt, loss)
    nv = torch.tensor(b.nvalid, device=_dev()).view(G, 1).float()
    wt = (torch.arange(B, device=_dev())[None, :].float() < nv).float() / nv.clamp_min(1.0)
    (per * wt).sum().backward()
    ref32 = logits.grad.double().cpu().numpy()
    scale = np.abs(want).max()
    e_hip, e_torch = np.abs(got - want).max() / scale, np.abs(ref32 - want).max() / scale
    print("[cnn-soft] dz vs fp64 oracle ({}, {}): E_hip {:.3e}  E_torch {:.3e}  ratio {:.2f}".format(
        kind, loss, e_hip, e_torch, e_hip / e_torch))
    assert scale > 0 and e_torch > 0
    assert e_hip <= 4 * e_torch


@pytest.mark.parametrize("loss", ["ce", "bce_compat"])
def test_guard_tail_and_unreferenced_rows(loss):
    """dz is NaN-filled with a guard tail; table rows that no sample id references are NaN: the written part is
    finite (no such row was read) and the tail is untouched."""
    G, B, Up, C = 3, 33, 1088, 7
    b = _Head(G, B, Up, C, prec=1, loss=loss, seed=2, N=400, guard=64)
    table = torch.from_numpy(R.random_table(np.random.default_rng(1), b.N, C))
    used = torch.zeros(b.N, dtype=torch.bool)
    used[b.gather_cpu.reshape(-1)] = True
    assert 0 < int(used.sum()) < b.N
    table[~used] = NAN
    b.K.check(b.K.lib().gt_head_soft(b.soft_args(loss, table=table.to(_dev())), _stream()), "head_soft")
    torch.cuda.synchronize()
    dz = b.dz.cpu()
    assert torch.isfinite(dz[:G * B * C]).all() and torch.isnan(dz[G * B * C:]).all()
    for k in ("dH", "gw2", "gb2", "gb1"):
        assert torch.isfinite(getattr(b, k)).all(), k
    # rows past the short batch carry zero weight
    assert not dz[:G * B * C].view(G, B, C)[0, b.nvalid[0]:].any()


def test_launcher_refusals_launch_nothing():
    G, B, Up, C = 2, 32, 512, 10
    b = _Head(G, B, Up, C, prec=1, loss="ce", seed=4)
    L = b.K.lib()
    table = b.onehot_table()
    untouched = b.outputs()

    def mod(**kw):
        s = b.soft_args("ce", table=kw.pop("table", table), t_on=kw.pop("t_on", 1.0), t_off=kw.pop("t_off", 0.0))
        for k, v in kw.items():
            setattr(s.head, k, v)
        return s
    bad = [mod(eval=1), mod(B=65), mod(C=0), mod(C=17), mod(Up=520), mod(plog=0), mod(b2=0), mod(labels=0),
           mod(gather=0), mod(dz=0), mod(table=None, t_on=NAN), mod(table=None, t_off=float("inf")),
           mod(table=None, t_on=float("-inf"))]
    for s in bad:
        assert L.gt_head_soft(s, _stream()) < 0
    null = ctypes.POINTER(b.K.HeadSoftArgs)()
    assert L.gt_head_soft(null, _stream()) < 0
    assert b.outputs() == untouched
    # non-finite smoothing values are ignored when a table is given
    b.K.check(L.gt_head_soft(mod(t_on=NAN, t_off=NAN), _stream()), "head_soft")
    assert b.outputs() != untouched


# ---------------------------------------------------------------------------------------------------------
# inside a job
# ---------------------------------------------------------------------------------------------------------

def _onehot_table(lab, classes):
    t = np.zeros((len(lab), classes), np.float32)
    t[np.arange(len(lab)), lab] = 1.0
    return t


def _params_equal(a, b):
    return sorted(a.params) == sorted(b.params) and all(a.params[k].tobytes() == b.params[k].tobytes()
                                                        for k in a.params)


@pytest.mark.parametrize("case", ["chain", "mnist"])          # 32x32x3 bce_compat; 28x28x1 stored in 32x32, ce
def test_fit_on_a_one_hot_table_equals_plain_fit(case):
    import test_cnn_fitted_gpu as T
    _, job, clf, x, lab = T._fit(case)
    m, _, _ = T._model(case)
    soft = m.fit(soft_targets=_onehot_table(lab, T.CASES[case][1]))
    names = [op[1] for op in m.jobs[0]._step_plan() if op[0] == "k"]
    assert "gt_head_soft" in names and "gt_head" not in names
    assert _params_equal(soft, clf)
    assert _bits(m.jobs[0].flat) == _bits(job.flat)                    # the masters themselves
    assert soft.metrics == clf.metrics
    # the evaluation counted hits against argmax(y), as predict does
    got = soft.predict(x, output="label", device=_dev())
    assert round(soft.metrics["categorical_accuracy"] * len(x)) == int((got == lab).sum())


def _small(shape=(32, 32, 3), n=160, classes=10):
    from gentun_amd.utils.data import make_glyph_classification
    x, y = make_glyph_classification(n=n, shape=shape, classes=classes, seed=0, noise=0.5)
    return np.asarray(x, np.float32), np.asarray(y, np.float32)


G3 = [{'S_1': '101', 'S_2': '0101110011'}, {'S_1': '000', 'S_2': '0000000000'}, {'S_1': '111', 'S_2': '1111111111'}]


def _plans(genes, shape=(32, 32, 3)):
    from gentun_amd.models.genome import make_plan
    return [make_plan(g, (3, 5), shape, (20, 50), ((5, 5), (5, 5)), 500, 10) for g in genes]


def _cfg(**kw):
    from gentun_amd.models import cnn_engine as E
    base = dict(epochs=(1,), learning_rate=(1e-3,), batch_size=32, dtype="fp32", loss="ce", reset="all")
    base.update(kw)
    return E.TrainConfig(**base)


def _soft_kw(kind, x, y):
    """(TrainConfig extras, job extras) of a random valid table or of label smoothing."""
    if kind == "eps":
        return {"label_smoothing": EPS}, {}
    table = R.random_table(np.random.default_rng(9), len(x), y.shape[1], np.argmax(y, 1), peak=0.5)
    return {}, {"soft_targets": table}


@pytest.mark.parametrize("shape", [(32, 32, 3), (28, 28, 1)])
@pytest.mark.parametrize("kind", ["table", "eps"])
def test_graph_eager_and_native_step_program(kind, shape, monkeypatch):
    """Three steps through each issue path: byte-equal masters."""
    from gentun_amd.models import cnn_hip
    x, y = _small(shape, n=128)
    fold = (np.arange(96), np.arange(96, 128))               # 3 steps of 32
    ckw, jkw = _soft_kw(kind, x, y)
    flats = {}
    for mode in ("native", "python", "graph"):
        monkeypatch.setattr(cnn_hip, "NATIVE_STEPS", mode == "native")
        job = cnn_hip.HipPopJob(None, x, y, None, _cfg(use_graph=mode == "graph", **ckw), _dev(),
                                members=[(p, [fold], [0]) for p in _plans(G3[:2], shape)], **jkw)
        assert job.steps_per_epoch == 3
        job.launch().finish()
        torch.cuda.synchronize()
        assert job.state[5].item() == 3
        if mode == "native":
            assert getattr(job, "_prog", None) is not None
        flats[mode] = _bits(job.flat)
    assert flats["native"] == flats["python"] == flats["graph"]
    plain = cnn_hip.HipPopJob(None, x, y, None, _cfg(), _dev(), members=[(p, [fold], [0]) for p in _plans(G3[:2], shape)])
    plain.launch().finish()
    assert _bits(plain.flat) != flats["graph"]              # the setting does change the training


@pytest.mark.parametrize("kind", ["table", "eps"])
def test_population_batch_invariance(kind):
    from gentun_amd.models.cnn_hip import HipPopJob
    from gentun_amd.utils.data import stratified_kfold
    x, y = _small(n=160)
    folds = stratified_kfold(np.argmax(y, 1), 2, seed=0)
    ckw, jkw = _soft_kw(kind, x, y)
    plans = _plans(G3)
    alone = HipPopJob(None, x, y, None, _cfg(**ckw), _dev(), members=[(plans[0], folds, [0, 1])], **jkw)
    ra = alone.launch().finish()
    members = [(plans[1], folds, [0, 1]), (plans[0], folds, [0, 1]), (plans[2], [folds[1]], [1])]
    rp = HipPopJob(None, x, y, None, _cfg(**ckw), _dev(), members=members, **jkw).launch().finish()
    assert rp[1] == ra[0], (rp[1], ra[0])


@pytest.mark.parametrize("loss", ["ce", "bce_compat"])
@pytest.mark.parametrize("kind", ["table", "eps"])
def test_one_step_gradients_match_fp64_autograd(kind, loss):
    """One SGD step (lr 1, no dropout, no BatchNorm) against fp64 autograd on the oracle's target rows, at the
    bound of tests/test_hip_step_parity.py: ``max(2e-4, 4 x torch fp32's error)`` on the HIP forward's ReLU
    decisions, and the free-running comparison within one flipped near-tie decision."""
    import test_hip_step_parity as P
    from gentun_amd.models.cnn_hip import HipPopJob
    x, y, fold, plan = P._setup(P.GENES[0])
    labels = np.argmax(y, 1)
    ckw, jkw = _soft_kw(kind, np.asarray(x), np.asarray(y))
    cfg = _cfg(learning_rate=(1.0,), dropout=0.0, loss=loss, optimizer="sgd", momentum=0.9, use_graph=False,
               reset="kernels", **ckw)
    job = HipPopJob(plan, x, y, [fold], cfg, _dev(), fold_ids=[0], **jkw)
    job.init_params()
    w0 = P._hip_weights(job)
    job.reset_optimizer(1.0)
    job._new_epoch_order()
    idx = job.epoch_idx[0, 0].cpu().numpy()
    job.train_step()
    torch.cuda.synchronize()
    got = P._hip_grads(job)
    xb = torch.from_numpy(np.asarray(x)[idx]).permute(0, 3, 1, 2)
    yb = torch.from_numpy(R.target_rows(labels, idx, 10, table=jkw.get("soft_targets"),
                                        eps=ckw.get("label_smoothing", 0.0)))
    assert not np.array_equal(yb.numpy(), np.asarray(y, np.float64)[idx])
    masks = {L.name: (job.act[L.name][0][..., :L.cout] > 0).permute(0, 3, 1, 2).cpu() for L in job.layers}

    def errs(g, ref):
        out = {}
        for k, r in ref.items():
            if isinstance(r, tuple):
                out[k + ".w"] = P._rel(g[k][0], r[0])
                if r[1].abs().max() > 0:
                    out[k + ".b"] = P._rel(g[k][1], r[1])
            else:
                out[k] = P._rel(g[k], r)
        return out
    ref, r32 = P._reference_grads(plan, w0, xb, yb, loss), P._reference_grads(plan, w0, xb, yb, loss, torch.float32)
    worst, worst32 = errs(got, ref), errs(r32, ref)
    assert set(k.split(".")[0] for k in worst) >= set(L.name for L in job.layers)
    for k, e in worst.items():
        assert e < max(2e-4, 4 * worst32[k], 3e-2), (k, e, worst32[k])
    ref_m = P._reference_grads(plan, w0, xb, yb, loss, masks=masks)
    r32_m = P._reference_grads(plan, w0, xb, yb, loss, torch.float32, masks=masks)
    worst, worst32 = errs(got, ref_m), errs(r32_m, ref_m)
    kmax = max(worst, key=worst.get)
    print("[cnn-soft parity] {} {}: worst rel grad err HIP {:.2e} ({}); torch fp32 there {:.2e}".format(
        kind, loss, worst[kmax], kmax, worst32[kmax]))
    for k, e in worst.items():
        assert e < max(2e-4, 4 * worst32[k]), (k, e, worst32[k])


def test_off_is_off():
    """Neither setting: no gt_head_soft in the plan and no table; and cross_validate returns the same bytes
    before and after a soft fit ran on the device."""
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.models.cnn_hip import HipPopJob
    from gentun_amd.ops import cnn_kernels as K
    from gentun_amd.utils.data import stratified_kfold
    x, y = _small(n=96)
    folds = stratified_kfold(np.argmax(y, 1), 2, seed=0)
    plan = _plans(G3[:1])[0]
    names = {}
    for key, cfg, kw in (("absent", E.TrainConfig(epochs=(1,), learning_rate=(1e-3,), batch_size=32, reset="all"), {}),
                         ("zero", _cfg(label_smoothing=0, loss="bce_compat"), {}),
                         ("eps", _cfg(label_smoothing=EPS, loss="bce_compat"), {}),
                         ("table", _cfg(loss="bce_compat"), {"soft_targets": _onehot_table(np.argmax(y, 1), 10)})):
        job = HipPopJob(plan, x, y, folds, cfg, _dev(), fold_ids=[0, 1], **kw)
        names[key] = [op[1] if op[0] == "k" else op[0] for op in job._step_plan() + job._adam_plan()]
        assert (job.head_soft_args is None) == (key in ("absent", "zero"))
        assert (job.soft is None) == (key != "table")
        hd = job._eval_ops(job.eval_batch())[2]
        assert isinstance(hd, K.HeadArgs) and hd.eval == 1                # evaluation keeps gt_head
    assert names["absent"] == names["zero"] and "gt_head_soft" not in names["zero"]
    for key in ("eps", "table"):
        assert "gt_head" not in names[key]
        assert [n.replace("gt_head_soft", "gt_head") for n in names[key]] == names["zero"]

    def cv():
        m = GeneticCnnModel(x, y, G3[0], (3, 5), (32, 32, 3), (20, 50), ((5, 5), (5, 5)), 500, 0.5, 10, nfold=2,
                            epochs=(1,), learning_rate=(1e-3,), batch_size=32, loss="ce", seed=1, backend="hip",
                            device=_dev())
        m.cross_validate()
        return m
    before = cv().fold_metrics
    m = cv()
    m.fit(soft_targets=R.random_table(np.random.default_rng(0), len(x), 10))
    assert cv().fold_metrics == before == m.fold_metrics


def test_distill_from_an_ensemble_on_the_hip_path():
    from gentun_amd.models import distill, fit_ensemble, soft_targets
    from gentun_amd.models.cnn import GeneticCnnModel
    x, y = _small(n=160)
    lab = np.argmax(y, 1)
    space = dict(nodes=(3, 5), input_shape=(32, 32, 3), kernels_per_layer=(20, 50), kernel_sizes=((5, 5), (5, 5)),
                 dense_units=500, dropout_probability=0.5, classes=10, nfold=2, epochs=(1,), learning_rate=(1e-3,),
                 batch_size=32, loss="ce", seed=2, backend="hip")
    ens = fit_ensemble(x, y, G3, weights=[2.0, 1.0, 1.0], device=_dev(), **space)
    table = soft_targets(ens, x, y, alpha=0.7, temperature=2.0, device=_dev())
    cpu = soft_targets(ens, x, y, alpha=0.7, temperature=2.0, device="cpu")           # the torch backend
    assert np.abs(table.astype(np.float64) - cpu.astype(np.float64)).max() <= 1e-6
    assert np.abs(table.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    student = distill(ens, x, y, G3[0], alpha=0.7, temperature=2.0, device=_dev(), **space)
    manual = GeneticCnnModel(x, y, G3[0], device=_dev(), **space).fit(soft_targets=table)
    assert _params_equal(student, manual) and student.metrics == manual.metrics
    short = ens.distill(x, y, alpha=0.7, temperature=2.0, device=_dev(), **space)
    assert short.genes == G3[0] and _params_equal(short, manual)
    got = student.predict(x, output="label", device=_dev())
    assert round(student.metrics["categorical_accuracy"] * len(x)) == int((got == lab).sum())


def test_hip_data_parallel_with_soft_targets_is_refused():
    from gentun_amd.models.cnn_hip import HipPopJob

    class FakeGroup(object):
        pass
    x, y = _small(n=96)
    fold = (np.arange(64), np.arange(64, 96))
    plan = _plans(G3[:1])[0]
    with pytest.raises(ValueError, match="dp_group are not supported by the HIP executor"):
        HipPopJob(plan, x, y, [fold], _cfg(dp_group=FakeGroup(), label_smoothing=EPS), _dev(), fold_ids=[0])
    with pytest.raises(ValueError, match="dp_group are not supported by the HIP executor"):
        HipPopJob(plan, x, y, [fold], _cfg(dp_group=FakeGroup()), _dev(), fold_ids=[0],
                  soft_targets=_onehot_table(np.argmax(y, 1), 10))
