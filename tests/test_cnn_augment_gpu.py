"""Shift-and-flip training augmentation on the MI355X: the gt_augment kernel (csrc/hip/cnn_augment.hip)
against the numpy oracle (tests/augment_ref.py) byte for byte, its launcher's refusals, and the HIP executor
with ``TrainConfig.augment`` set: the augmented batch of every step, one-step gradients against fp64
autograd on the oracle's batch, batch invariance, graph / eager / native step program, the unchanged step
plan with augmentation off, the shape-specialised kernels of the first layer, and cross-validation."""

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

AUG = {"shift": 4, "flip": True}
N, B, STEPS = 40, 32, 3


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------ the kernel, called directly
class _Case(object):
    """A dataset of small positive integers (exact in bf16, never 0) stored zero-padded, a 3-step gather
    table with ids 0, N - 1 and a repeated id in every batch, and a NaN-filled output with a guard tail."""

    GUARD = 4096

    def __init__(self, real, stored, dtype, Q, seed=0):
        (self.Hr, self.Wr, self.C), (self.Hp, self.Wp, self.Cp) = real, stored
        self.Q, self.dtype = Q, dtype
        rs = np.random.RandomState(seed)
        self.data = rs.randint(1, 200, size=(N, self.Hr, self.Wr, self.C)).astype(np.float32)
        pad = np.zeros((N, self.Hp, self.Wp, self.Cp), np.float32)
        pad[:, :self.Hr, :self.Wr, :self.C] = self.data
        self.src = torch.from_numpy(pad).to(device=_dev(), dtype=dtype).contiguous()
        ids = rs.randint(0, N, size=(STEPS, Q, B)).astype(np.int64)
        ids[:, :, 0], ids[:, :, 1], ids[:, :, 3] = 0, N - 1, ids[:, :, 2]
        self.ids = ids
        self.table = torch.from_numpy(ids).to(_dev())
        self.seeds = [0xdeadbeef, 1, 12345][:Q]
        self.fids = [5, 0, 3][:Q]
        self.seeds_t = torch.tensor(np.asarray(self.seeds, np.uint32).view(np.int32), device=_dev())
        self.fids_t = torch.tensor(self.fids, dtype=torch.int32, device=_dev())
        self.state = torch.zeros(8, dtype=torch.int32, device=_dev())
        self.n = Q * B * self.Hp * self.Wp * self.Cp
        self.out = torch.full((self.n + self.GUARD,), float("nan"), dtype=dtype, device=_dev())
        self.nan_bits = _bits(self.out)[0].item()

    def args(self, shift, flip, row_off=0):
        from gentun_amd.ops import cnn_kernels as K
        a = K.AugArgs()
        a.src, a.out, a.gather, a.st = (self.src.data_ptr(), self.out.data_ptr(), self.table.data_ptr(),
                                        self.state.data_ptr())
        a.fold_ids, a.seeds, a.row_off = self.fids_t.data_ptr(), self.seeds_t.data_ptr(), row_off
        a.Q, a.B, a.Hp, a.Wp, a.Hr, a.Wr, a.Cp = self.Q, B, self.Hp, self.Wp, self.Hr, self.Wr, self.Cp
        a.shift, a.flip, a.prec = shift, 1 if flip else 0, 1 if self.dtype == torch.float32 else 0
        return a

    def launch(self, a):
        from gentun_amd.ops import cnn_kernels as K
        self.out.fill_(float("nan"))
        rc = K.lib().gt_augment(a, torch.cuda.current_stream(_dev()).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self, whole=False):
        return bool((_bits(self.out if whole else self.out[self.n:]) == self.nan_bits).all().item())

    def check(self, cur_step, gstep, shift, flip, row_off):
        want = R.augment_batch(self.data, self.ids[cur_step], self.seeds, self.fids, gstep, shift, flip,
                               (self.Hr, self.Wr), (self.Hp, self.Wp), self.Cp, row_off)
        want = torch.from_numpy(want).to(self.dtype).reshape(-1)
        got = self.out[:self.n].cpu()
        assert torch.equal(_bits(got), _bits(want)), (cur_step, gstep, shift, flip, row_off)
        assert self.untouched()                      # nothing past the buffer


GEOMETRIES = {"cifar": ((32, 32, 3), (32, 32, 8)), "mnist": ((28, 28, 1), (32, 32, 8)), "odd": ((6, 5, 3), (8, 8, 8))}


@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_kernel_equals_the_oracle(geom, dtype, Q):
    from gentun_amd.ops import cnn_kernels as K
    real, stored = GEOMETRIES[geom]
    c = _Case(real, stored, dtype, Q)
    smax = min(real[:2]) - 1
    combos = [(0, True)] + [(s, f) for s in sorted({1, 4, smax}) for f in (False, True)]
    where = [(0, 1, 0), (2, 7, 16)]                  # (cur_step, global_step, row_off): steps 0 and 2 of the table
    for i, (shift, flip) in enumerate(combos):
        for cur, gstep, off in (where if i == 1 else [where[i % 2]]):
            c.state.zero_()
            c.state[1], c.state[5] = cur, gstep       # StepState.cur_step / global_step set by hand
            assert c.launch(c.args(shift, flip, off)) == 0
            c.check(cur, gstep, shift, flip, off)
    # the same fields prepared by gt_step_begin: step_ctr 2 -> cur_step 2, global_step 6 -> 7
    c.state.zero_()
    c.state[0], c.state[5] = 2, 6
    K.check(K.lib().gt_step_begin(c.state.data_ptr(), torch.cuda.current_stream(_dev()).cuda_stream), "step_begin")
    assert c.launch(c.args(1, True, 16)) == 0
    assert c.state.cpu().tolist()[:2] == [3, 2] and c.state[5].item() == 7
    c.check(2, 7, 1, True, 16)


def test_launcher_refusals():
    c = _Case((6, 5, 3), (8, 8, 8), torch.float32, 1)
    c.state[5] = 1
    assert c.launch(c.args(1, True)) == 0 and not c.untouched(whole=True)      # the accepted call does write

    def bad(**kw):
        a = c.args(1, True)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for a in (bad(Cp=12), bad(Cp=4), bad(Hr=9), bad(Wr=9), bad(shift=5), bad(shift=6), bad(shift=-1),
              bad(Hr=2, Wr=8, shift=2), bad(src=0), bad(out=0), bad(gather=0), bad(st=0), bad(Q=0), bad(B=0),
              bad(prec=2)):
        assert c.launch(a) != 0
        assert c.untouched(whole=True)
    assert c.launch(c.args(4, False)) == 0            # min(6, 5) - 1 is the largest shift


# ------------------------------------------------------------------ in the executor
def _headline_plans(genes):
    from gentun_amd.models.genome import make_plan
    return [make_plan(g, (3, 5), (32, 32, 3), (20, 50), ((5, 5), (5, 5)), 500, 10) for g in genes]


G3 = [{'S_1': '101', 'S_2': '0101110011'}, {'S_1': '000', 'S_2': '0000000000'}, {'S_1': '111', 'S_2': '1111111111'}]


def _cfg(aug=AUG, **kw):
    from gentun_amd.models import cnn_engine as E
    base = dict(epochs=(1,), learning_rate=(1e-3,), batch_size=32, dtype="fp32", loss="ce", reset="all", augment=aug)
    base.update(kw)
    return E.TrainConfig(**base)


def _data32(n, seed=3):
    from gentun_amd.utils.data import make_image_classification, stratified_kfold
    x, y = make_image_classification(n=n, shape=(32, 32, 3), classes=10, seed=seed, noise=0.35, shift=3)
    return x, y, stratified_kfold(np.argmax(y, 1), 2, seed=0)


@pytest.mark.parametrize("which", ["small", "headline"])
def test_augmented_batch_in_the_executor(which):
    from gentun_amd.models.cnn_hip import HipPopJob
    from gentun_amd.models.genome import make_plan
    from gentun_amd.utils.data import make_image_classification, stratified_kfold
    if which == "small":
        x, y = make_image_classification(n=192, shape=(8, 8, 3), classes=4, seed=1)
        folds = stratified_kfold(np.argmax(y, 1), 2, seed=0)          # 96 training rows: 3 steps of 32
        plan = make_plan({'S_1': '101'}, (3,), (8, 8, 3), (4,), ((3, 3),), 16, 4)
        hw = (8, 8)
    else:
        x, y, folds = _data32(192)
        plan = _headline_plans(G3[:1])[0]
        hw = (32, 32)
    cfg = _cfg({"shift": 2, "flip": True}, use_graph=False)
    job = HipPopJob(plan, x, y, folds, cfg, _dev(), fold_ids=[0, 1])          # 2 groups
    assert job.aug_x is not None and tuple(job.aug_x.shape) == (2 * 32,) + hw + (8,)
    job.init_params()
    job.reset_optimizer(1e-3)
    job._new_epoch_order()
    xs = np.asarray(x, np.float32)
    for k in range(3):
        ids = job.epoch_idx[k].cpu().numpy()
        job.train_step()
        torch.cuda.synchronize()
        assert job.state[5].item() == k + 1
        want = R.augment_batch(xs, ids, job.aug_seeds, job.fold_ids, k + 1, 2, True, hw, hw, 8)
        got = job.aug_x.view(2, 32, hw[0], hw[1], 8).cpu().numpy()
        assert got.tobytes() == want.tobytes(), k
    assert job.data.x[:, :, :, :3].cpu().numpy().tobytes() == xs.tobytes()    # the dataset itself is never written


# a max-pool argmax that differs from the fp64 network's own is a rounding-level near-tie only when the fp64 gap
# between the two candidates is below this fraction of the layer's largest activation: 64 fp32 unit roundoffs
# (2^-24 each), the accumulated rounding of the 450-term fp32 sums of a 3x3 x 50-channel conv and of the layers
# in front of it. Anything above it is a wrong decision and fails the test.
POOL_TIE_GAP = 2.0 ** -18


class _HipPoolDecisions(object):
    """``F`` of tests/test_hip_step_parity.py with the 2x2 max-pool taking the HIP forward's decisions.

    The reference of that file takes the HIP forward's ReLU decisions, so that the arithmetic is compared and
    not the tie-breaking; a max-pool window whose two largest values differ by less than the forward's fp32
    rounding is the same thing one layer later. Measured on the MI355X with shift 4 + flip on genome 0:
    one of 102,400 stage-2 windows holds 0.00664999569 and 0.0066500036 in fp32 and 0.00665001037 and
    0.00665000072 in fp64 -- the other order, 1e-8 apart -- and routing that one gradient element to the
    neighbouring pixel moves every conv weight gradient by 5e-4 to 1e-3 of its largest entry while every
    bias gradient behind the pool and the dense gradients stay at 1e-6. The executor routes by its own
    fp32 values in every window (checked there too). So the reference pools by the HIP argmax, and every
    window where that differs from the fp64 argmax must be a near-tie (POOL_TIE_GAP); the bound on the
    gradients is unchanged."""

    def __init__(self, job, plan):
        import torch.nn.functional as F
        from gentun_amd.models.genome import PoolSpec
        self.conv2d, self.relu, self._F = F.conv2d, F.relu, F
        self.argmax, self.flips = {}, 0
        for st in plan.steps:
            if isinstance(st, PoolSpec):
                src = job.act[st.srcs[0]][0]
                C = {L.name: L.cout for L in job.layers}[st.srcs[0]]
                v = src[..., :C].permute(0, 3, 1, 2).cpu()
                self.argmax[v.shape[2]] = self._windows(v).argmax(2)            # keyed by the source height

    def _windows(self, t):
        return self._F.unfold(t, 2, stride=2).view(t.shape[0], t.shape[1], 4, -1)

    def max_pool2d(self, src, k, s):
        assert (k, s) == (2, 2)
        Bn, C, H, W = src.shape
        u, idx = self._windows(src), self.argmax[H]
        out = u.gather(2, idx[:, :, None, :]).squeeze(2)
        if src.dtype == torch.float64:
            with torch.no_grad():
                top = u.max(2).values
                gap = top - out
                differs = gap > 0
                self.flips += int(differs.sum())
                worst = (gap.max() / src.abs().max()).item()
                print("[augment parity]   pool at {}x{}: HIP argmax differs from fp64 at {} of {} windows, "
                      "largest gap {:.2e} of the layer maximum".format(H, W, int(differs.sum()), gap.numel(), worst))
                assert worst <= POOL_TIE_GAP, worst
        return out.view(Bn, C, H // 2, W // 2)


@pytest.mark.parametrize("gi", [0, 1])
def test_one_step_gradients_on_the_augmented_batch(gi, monkeypatch):
    """Augmentation moves data and adds no arithmetic: the bound is tests/test_hip_step_parity.py's own
    ``max(2e-4, 4 x torch fp32's error)``, on the HIP forward's ReLU and (near-tie) max-pool decisions
    (:class:`_HipPoolDecisions`)."""
    import test_hip_step_parity as P
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn_hip import HipPopJob
    x, y, fold, plan = P._setup(P.GENES[gi])
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1.0,), batch_size=32, dropout=0.0, loss="ce", dtype="fp32",
                        optimizer="sgd", momentum=0.9, use_graph=False, augment=AUG)
    job = HipPopJob(plan, x, y, [fold], cfg, _dev(), fold_ids=[0])
    job.init_params()
    w0 = P._hip_weights(job)
    job.reset_optimizer(1.0)
    job._new_epoch_order()
    idx = job.epoch_idx[0].cpu().numpy()                     # [1][B]
    job.train_step()
    torch.cuda.synchronize()
    got = P._hip_grads(job)
    xa = R.augment_batch(np.asarray(x, np.float32), idx, job.aug_seeds, job.fold_ids, 1, 4, True, (32, 32))[0]
    assert xa.tobytes() != np.asarray(x, np.float32)[idx[0]].tobytes()
    xb = torch.from_numpy(xa).permute(0, 3, 1, 2)
    yb = torch.from_numpy(np.asarray(y)[idx[0]]).double()
    masks = {L.name: (job.act[L.name][0][..., :L.cout] > 0).permute(0, 3, 1, 2).cpu() for L in job.layers}
    pools = _HipPoolDecisions(job, plan)
    monkeypatch.setattr(P, "F", pools)
    ref = P._reference_grads(plan, w0, xb, yb, "ce", masks=masks)
    r32 = P._reference_grads(plan, w0, xb, yb, "ce", torch.float32, masks=masks)

    def errs(g):
        out = {}
        for k, r in ref.items():
            if isinstance(r, tuple):
                out[k + ".w"] = P._rel(g[k][0], r[0])
                if r[1].abs().max() > 0:
                    out[k + ".b"] = P._rel(g[k][1], r[1])
            else:
                out[k] = P._rel(g[k], r)
        return out
    worst, worst32 = errs(got), errs(r32)
    for k in sorted(worst):
        print("[augment parity]   {:10s} HIP {:.2e}  torch fp32 {:.2e}".format(k, worst[k], worst32[k]))
    kmax = max(worst, key=worst.get)
    print("[augment parity] genes {}: worst rel grad err HIP {:.2e} ({}); torch fp32 there {:.2e}; pool decisions "
          "taken from HIP at {} near-tie windows".format(P.GENES[gi], worst[kmax], kmax, worst32[kmax], pools.flips))
    assert set(k.split(".")[0] for k in worst) >= set(L.name for L in job.layers)
    for k, e in worst.items():
        assert e < max(2e-4, 4 * worst32[k]), (k, e, worst32[k])


def test_population_batch_invariance_with_augmentation():
    from gentun_amd.models import cnn_engine as E
    x, y, folds = _data32(320)
    cfg = _cfg()
    plans = _headline_plans(G3)
    alone = E.make_job("hip", plans[0], x, y, folds, cfg, _dev()).launch().finish()
    members = [(plans[1], folds, [0, 1]), (plans[0], folds, [0, 1]), (plans[2], [folds[1]], [1])]
    pop = E.make_population_job("hip", members, x, y, cfg, _dev()).launch().finish()
    assert pop[1] == alone, (pop[1], alone)
    plain = E.make_job("hip", plans[0], x, y, folds, _cfg(None), _dev()).launch().finish()
    assert plain["val_loss"] != alone["val_loss"]             # the setting does change the training


def test_graph_eager_and_native_step_program(monkeypatch):
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models import cnn_hip
    x, y, _ = _data32(160)
    fold = (np.arange(128), np.arange(128, 160))              # 4 steps of 32
    plans = _headline_plans(G3[:2])
    flats = {}
    for mode in ("native", "python", "graph"):
        monkeypatch.setattr(cnn_hip, "NATIVE_STEPS", mode == "native")
        job = E.make_population_job("hip", [(p, [fold], [0]) for p in plans], x, y, _cfg(use_graph=mode == "graph"),
                                    _dev())
        assert job.steps_per_epoch == 4
        job.launch().finish()
        torch.cuda.synchronize()
        assert job.state[5].item() == 4
        if mode == "native":
            assert getattr(job, "_prog", None) is not None
        flats[mode] = job.flat.detach().cpu().clone()
    assert torch.equal(flats["native"], flats["python"])
    assert torch.equal(flats["native"], flats["graph"])


def test_off_is_off():
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn_hip import HipPopJob
    x, y, folds = _data32(96)
    plan = _headline_plans(G3[:1])[0]
    names = {}
    for key, cfg in (("absent", E.TrainConfig(epochs=(1,), learning_rate=(1e-3,), batch_size=32, reset="all")),
                     ("none", _cfg(None)), ("on", _cfg())):
        job = HipPopJob(plan, x, y, folds, cfg, _dev(), fold_ids=[0, 1])
        names[key] = [op[1] if op[0] == "k" else op[0] for op in job._step_plan() + job._adam_plan()]
        if key == "on":
            assert job.aug_x is not None and job.train_fwd_ops is not job.fwd_ops
            # the evaluation launches are copied from the dataset-reading list
            first = [a for kind, a, _ in job.fwd_ops if kind == "conv" and a.gather][0]
            assert first.inp[0] == job.data.x.data_ptr() and first.gather == job.epoch_idx.data_ptr()
        else:
            assert job.aug_x is None and job.aug_args is None and job.aug_table is None
            assert job.train_fwd_ops is job.fwd_ops
    assert names["absent"] == names["none"] and "gt_augment" not in names["none"]
    assert names["on"][:2] == ["gt_step_begin", "gt_augment"]
    assert names["on"][:1] + names["on"][2:] == names["none"]          # one launch more, nothing else


@pytest.mark.parametrize("shape", [(32, 32, 3), (28, 28, 1)])
def test_first_layer_stays_on_the_shape_specialised_kernels(shape):
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn_hip import fast_path_report
    from gentun_amd.models.genome import make_plan
    from gentun_amd.ops import cnn_kernels as K
    from gentun_amd.utils.data import make_image_classification, stratified_kfold
    x, y = make_image_classification(n=96, shape=shape, classes=10, seed=1)
    folds = stratified_kfold(np.argmax(y, 1), 2, seed=0)
    plans = [make_plan(g, (3, 5), shape, (20, 50), ((5, 5), (5, 5)), 500, 10) for g in G3[:2]]
    assert fast_path_report(plans[0], ngroups=4)["generic_launches"] == 0
    job = E.make_population_job("hip", [(p, folds, [0, 1]) for p in plans], x, y, _cfg(), _dev())
    L = K.lib()
    firsts = 0
    for kind, a, Lr in job.train_fwd_ops + job.bwd_ops:
        if kind == "conv":
            assert L.gt_conv_fast_probe_any(a) == 1, Lr.name
        elif kind == "wgrad":
            assert L.gt_wgrad_fast_band(a.KH, a.KW, a.Cinp, a.Coutp, a.H, a.W, a.prec) > 0, Lr.name
        if kind in ("conv", "wgrad") and a.gather:
            firsts += 1
            assert a.inp[0] == job.aug_x.data_ptr() and a.gather == job.aug_table.data_ptr()
    assert firsts == 2                                         # the first conv and its weight gradient
    assert tuple(job.aug_x.shape[1:]) == (32, 32, 8)
    res = job.launch().finish()                                # and the padded geometry trains
    assert all(np.isfinite(v) for r in res for v in r["val_loss"])


@pytest.mark.parametrize("reset", ["kernels", "all"])
def test_cross_validate_is_reproducible(reset):
    from gentun_amd.models.cnn import GeneticCnnModel
    from gentun_amd.utils.data import make_image_classification
    x, y = make_image_classification(n=200, shape=(32, 32, 3), classes=10, seed=3, noise=0.35, shift=3)
    out = []
    for _ in range(2):
        m = GeneticCnnModel(x, y, G3[0], (3, 5), (32, 32, 3), (20, 50), ((5, 5), (5, 5)), 500, 0.5, 10, nfold=2,
                            epochs=(1, 1), learning_rate=(1e-3, 1e-4), batch_size=32, loss="ce", seed=1,
                            backend="hip", device=_dev(), reset=reset, augment=AUG)
        m.cross_validate()
        out.append(m.fold_metrics)
    assert out[0] == out[1]
    assert all(np.isfinite(v) for v in out[0]["val_loss"])


def test_hip_data_parallel_with_augmentation_is_refused():
    from gentun_amd.models.cnn_hip import HipPopJob

    class FakeGroup(object):
        pass
    x, y, folds = _data32(96)
    with pytest.raises(ValueError, match="augment with dp_group"):
        HipPopJob(_headline_plans(G3[:1])[0], x, y, folds, _cfg(dp_group=FakeGroup()), _dev(), fold_ids=[0, 1])
