"""Mixup / CutMix training on the MI355X: gt_augment_mix (csrc/hip/cnn_mix.hip) against the loop oracle
(tests/mix_ref.py) byte for byte, gt_head_mix (csrc/hip/cnn_dense.hip) against gt_head / gt_head_soft on steps
that are not mixed and against the fp64 oracle of tests/soft_ref.py on steps that are, both launchers'
refusals, and the HIP executor with ``TrainConfig.mix`` set."""

import numpy as np
import pytest
import torch

import mix_ref as R
import soft_ref as S
import test_cnn_augment_gpu as TA
from test_cnn_soft_gpu import _Head, _stream

pytestmark = pytest.mark.gpu

N, B = 40, 5
NV = [5, 3, 2, 1]                                   # the valid-row table: one table row per batch size
SEEDS, FIDS = [0xdeadbeef, 1, 12345], [5, 0, 3]
KEY0 = R.key_of(SEEDS[0], FIDS[0])
P_HALF = R.p24_of(0.5)
KINDS = {"mixup": 0, "cutmix": 1}
# (table row, global step, alpha) of every launch, chosen with the oracle for group 0's key at prob 0.5 so that
# together they hold every case of CASES; the last one is the empty box, per real image size
LAUNCHES = [(1, 1, 3), (2, 1, 1), (3, 1, 1), (0, 4, 1), (0, 6, 1), (0, 2, 3)]
EMPTY = {(6, 5): (0, 48, 1), (28, 28): (0, 664, 1)}
CASES = {"applied", "skipped", "o=1", "o=nv-1", "top", "bottom", "left", "right", "empty"}


def _dev():
    return torch.device("cuda", 0)


def _cases(d, nv, hr, wr):
    if d is None:
        return {"skipped"}
    (y0, y1, x0, x1), (b0, b1, b2, b3) = d["unclipped"], d["box"]
    out = {"applied", "o=1" if d["o"] == 1 and nv > 2 else "", "o=nv-1" if d["o"] == nv - 1 and nv > 2 else "",
           "top" if y0 < 0 else "", "bottom" if y1 > hr else "", "left" if x0 < 0 else "",
           "right" if x1 > wr else "", "empty" if (b1 - b0) * (b3 - b2) == 0 else ""}
    return out - {""}


class _Case(object):
    """tests/test_cnn_augment_gpu.py's case at B = 5: integer-valued data stored zero-padded, a gather table with
    ids 0, N - 1 and a repeated id in every batch, a NaN-filled output with a guard tail."""

    GUARD = 4096

    def __init__(self, real, stored, dtype, Q):
        (self.Hr, self.Wr, self.C), (self.Hp, self.Wp, self.Cp) = real, stored
        self.Q, self.dtype = Q, dtype
        rs = np.random.RandomState(0)
        self.data = rs.randint(1, 200, size=(N, self.Hr, self.Wr, self.C)).astype(np.float32)
        pad = np.zeros((N, self.Hp, self.Wp, self.Cp), np.float32)
        pad[:, :self.Hr, :self.Wr, :self.C] = self.data
        self.src = torch.from_numpy(pad).to(device=_dev(), dtype=dtype).contiguous()
        self.ids = rs.randint(0, N, size=(len(NV), Q, B)).astype(np.int64)
        self.ids[:, :, 0], self.ids[:, :, 1], self.ids[:, :, 3] = 0, N - 1, self.ids[:, :, 2]
        self.keep = [torch.from_numpy(self.ids).to(_dev()),
                     torch.tensor(np.repeat(NV, Q).reshape(len(NV), Q), dtype=torch.int32, device=_dev()),
                     torch.tensor(np.asarray(SEEDS[:Q], np.uint32).view(np.int32), device=_dev()),
                     torch.tensor(FIDS[:Q], dtype=torch.int32, device=_dev())]
        self.state = torch.zeros(8, dtype=torch.int32, device=_dev())
        self.n = Q * B * self.Hp * self.Wp * self.Cp
        self.out = torch.full((self.n + self.GUARD,), float("nan"), dtype=dtype, device=_dev())
        self.nan_bits = TA._bits(self.out)[0].item()

    def args(self, kind, alpha, shift=0, flip=False, p24=P_HALF):
        from gentun_amd.ops import cnn_kernels as K
        a = K.MixArgs()
        a.src, a.out, a.st = self.src.data_ptr(), self.out.data_ptr(), self.state.data_ptr()
        a.gather, a.valid, a.seeds, a.fold_ids = (t.data_ptr() for t in self.keep)
        a.Q, a.B, a.Hp, a.Wp, a.Hr, a.Wr, a.Cp = self.Q, B, self.Hp, self.Wp, self.Hr, self.Wr, self.Cp
        a.shift, a.flip, a.prec = shift, 1 if flip else 0, 1 if self.dtype == torch.float32 else 0
        a.kind, a.alpha, a.p24 = KINDS[kind], alpha, p24
        return a

    def launch(self, a, cur=0, gstep=1):
        from gentun_amd.ops import cnn_kernels as K
        self.out.fill_(float("nan"))
        self.state.zero_()
        self.state[1], self.state[5] = cur, gstep          # StepState.cur_step / global_step
        rc = K.lib().gt_augment_mix(a, torch.cuda.current_stream(_dev()).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self, whole=False):
        return bool((TA._bits(self.out if whole else self.out[self.n:]) == self.nan_bits).all().item())


GEOMETRIES = {"mnist": ((28, 28, 1), (32, 32, 8)), "odd": ((6, 5, 3), (8, 8, 8))}


@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_kernel_equals_the_oracle(geom, dtype, kind, Q):
    real, stored = GEOMETRIES[geom]
    c = _Case(real, stored, dtype, Q)
    hr, wr = real[:2]
    seen = set()
    for i, (cur, gstep, alpha) in enumerate(LAUNCHES + [EMPTY[(hr, wr)]]):
        aug = {"shift": 2, "flip": True} if i % 2 else None
        seen |= _cases(R.draw(KEY0, gstep, NV[cur], alpha, P_HALF, hr, wr), NV[cur], hr, wr)
        assert c.launch(c.args(kind, alpha, 2 if aug else 0, bool(aug)), cur, gstep) == 0
        mix = {"kind": kind, "alpha": alpha, "prob": 0.5}
        want, _ = R.mixed_step(c.data, c.ids[cur], np.zeros((Q, B, 1), np.float32), [NV[cur]] * Q, SEEDS, FIDS, gstep,
                               mix, aug, (hr, wr), stored[:2], stored[2])
        want = torch.from_numpy(want).to(dtype).reshape(-1)
        assert torch.equal(TA._bits(c.out[:c.n].cpu()), TA._bits(want)), (cur, gstep, alpha, aug)
        assert c.untouched()                         # nothing past the buffer
    assert seen == CASES                             # a change of the rule cannot silently drop a case


def test_launcher_refusals():
    c = _Case((6, 5, 3), (8, 8, 8), torch.float32, 1)
    assert c.launch(c.args("mixup", 1, 1, True)) == 0 and not c.untouched(whole=True)   # the accepted call writes
    for kw in (dict(Cp=12), dict(Hr=9), dict(Wr=9), dict(shift=5), dict(shift=-1), dict(src=0), dict(out=0),
               dict(gather=0), dict(st=0), dict(Q=0), dict(B=0), dict(prec=2), dict(kind=2), dict(kind=-1),
               dict(alpha=0), dict(alpha=9), dict(p24=0), dict(p24=(1 << 24) + 1), dict(valid=0)):
        a = c.args("mixup", 1, 1, True)
        for k, v in kw.items():
            setattr(a, k, v)
        assert c.launch(a) != 0 and c.untouched(whole=True), kw
    assert c.launch(c.args("cutmix", 8, 4, False, p24=1 << 24)) == 0
    h = _Head(2, 32, 512, 10, prec=1, loss="ce", seed=4)
    before = h.outputs()
    for kw in (dict(kind=2), dict(alpha=0), dict(alpha=9), dict(p24=0), dict(p24=(1 << 24) + 1), dict(Hr=0),
               dict(B=65), dict(eval=1), dict(st=0), dict(dz=0)):
        m = _head_args(h, "ce", "cutmix", 1, "hard", None)
        for k, v in kw.items():
            setattr(m.soft.head if k in ("B", "eval", "st", "dz") else m, k, v)
        assert h.K.lib().gt_head_mix(m, _stream()) < 0, kw
    assert h.outputs() == before


def _head_args(h, loss, kind, alpha, source, table, hw=(28, 28)):
    from gentun_amd.models.cnn_engine import smoothing_targets
    t_on, t_off = smoothing_targets(0.1, h.dims[3]) if source == "eps" else (1.0, 0.0)
    if not hasattr(h, "seeds_t"):
        h.seeds_t = torch.tensor(np.asarray(SEEDS[:h.dims[0]], np.uint32).view(np.int32), device=_dev())
        h.fids_t = torch.tensor(FIDS[:h.dims[0]], dtype=torch.int32, device=_dev())
    m = h.K.HeadMixArgs()
    m.soft = h.soft_args(loss, table=table if source == "table" else None, t_on=float(t_on), t_off=float(t_off))
    m.seeds, m.fold_ids = h.seeds_t.data_ptr(), h.fids_t.data_ptr()
    m.kind, m.alpha, m.p24 = KINDS[kind], alpha, P_HALF
    m.Hr, m.Wr = hw
    m.inv_hw = float(np.float32(1.0) / np.float32(hw[0] * hw[1]))
    return m


@pytest.mark.parametrize("prec,source,C", [(1, "hard", 10), (0, "eps", 2), (1, "table", 16)])
@pytest.mark.parametrize("loss", ["ce", "bce_compat"])
def test_head_mix(loss, prec, source, C):
    """Group 0 has 30 real rows, group 1 one. Step 2 is skipped and group 1 is never mixed: every output equals
    gt_head's (hard labels) or gt_head_soft's. On the applied step 1, dz against the fp64 oracle fed the oracle's
    mixed target rows: E_hip <= 4 x the error of stock-torch fp32 autograd on the same inputs, measured here
    (the rule of tests/test_cnn_soft_gpu.py)."""
    from gentun_amd.models.cnn_engine import loss_and_metrics, smoothing_targets
    G, Bh, Up = 2, 33, 512
    h = _Head(G, Bh, Up, C, prec=prec, loss=loss, seed=7, std=2.0, guard=64)
    h.nvalid = [30, 1]
    h.valid = torch.tensor([h.nvalid], dtype=torch.int32, device=_dev())
    L, labels, sids = h.K.lib(), h.labels_cpu.numpy(), h.gather_cpu.numpy()[0]
    table = S.random_table(np.random.default_rng(3), h.N, C, labels, peak=0.3)
    tab_t = torch.from_numpy(table).to(_dev())
    assert R.draw(KEY0, 2, 30, 2, P_HALF, 28, 28) is None and R.draw(KEY0, 1, 30, 2, P_HALF, 28, 28) is not None
    if source == "hard":
        h.K.check(L.gt_head(h.args(loss), _stream()), "head")
    else:
        h.K.check(L.gt_head_soft(_head_args(h, loss, "mixup", 2, source, tab_t).soft, _stream()), "head_soft")
    plain = h.outputs()
    own = np.stack([S.target_rows(labels, sids[g], C, table=table if source == "table" else None,
                                  eps=0.1 if source == "eps" else 0.0) for g in range(G)]).astype(np.float32)
    z64 = h.logits64()
    for kind in sorted(KINDS):
        for gstep in (2, 1):
            h.fresh()
            h.st[5] = gstep
            h.K.check(L.gt_head_mix(_head_args(h, loss, kind, 2, source, tab_t), _stream()), "head_mix")
            got = h.outputs()
            dz = h.dz.cpu()
            assert torch.isnan(dz[G * Bh * C:]).all()                   # the guard tail
            if gstep == 2:
                assert got == plain
                continue
            dz, dz0 = dz[:G * Bh * C].view(G, Bh, C), torch.frombuffer(bytearray(plain["dz"]), dtype=torch.float32)
            assert torch.equal(dz[1], dz0[:G * Bh * C].view(G, Bh, C)[1])     # the nv = 1 batch
            _, tm = R.mix_batch(np.zeros((G, Bh, 28, 28, 1), np.float32), own, h.nvalid, SEEDS, FIDS, 1, kind, 2,
                                P_HALF, (28, 28))
            assert tm[0, :30].tobytes() != own[0, :30].tobytes() and tm[0, 30:].tobytes() == own[0, 30:].tobytes()
            want = S.batch_dz(z64[0], tm[0].astype(np.float64), loss, nvalid=30)
            logits = (h.plog.sum(1) + h.b2[:, None, :])[0].detach().requires_grad_(True)
            per, _, _ = loss_and_metrics(logits, torch.from_numpy(tm[0]).to(_dev()), loss)
            ((per * (torch.arange(Bh, device=_dev()) < 30).float()).sum() / 30).backward()
            scale = np.abs(want).max()
            e_hip = np.abs(dz[0].double().numpy() - want).max() / scale
            e_torch = np.abs(logits.grad.double().cpu().numpy() - want).max() / scale
            print("[cnn-mix] dz vs fp64 oracle ({}, {}, {}): E_hip {:.3e}  E_torch {:.3e}".format(
                kind, source, loss, e_hip, e_torch))
            assert scale > 0 and e_torch > 0 and e_hip <= 4 * e_torch


# ------------------------------------------------------------------ in the executor
def _cfg(mix, aug=None, **kw):
    return TA._cfg(aug, mix=mix, **kw)


def _mix(kind):
    return {"kind": kind, "alpha": 2, "prob": 0.75}


@pytest.mark.parametrize("aug", [None, {"shift": 2, "flip": True}], ids=["alone", "augment"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_mixed_batch_in_the_executor(kind, aug):
    from gentun_amd.models.cnn_hip import HipPopJob
    x, y, folds = TA._data32(192)                                # 96 training rows: 3 steps of 32
    job = HipPopJob(TA._headline_plans(TA.G3[:1])[0], x, y, folds, _cfg(_mix(kind), aug, use_graph=False), _dev(),
                    fold_ids=[0, 1])
    job.init_params()
    job.reset_optimizer(1e-3)
    job._new_epoch_order()
    xs, oh = np.asarray(x, np.float32), np.asarray(y, np.float32)
    applied = 0
    for k in range(3):
        ids = job.epoch_idx[k].cpu().numpy()
        job.train_step()
        torch.cuda.synchronize()
        want, tm = R.mixed_step(xs, ids, oh[ids], [32, 32], job.aug_seeds, job.fold_ids, k + 1, _mix(kind), aug,
                                (32, 32), (32, 32), 8)
        applied += int(tm.tobytes() != oh[ids].tobytes())
        assert job.aug_x.view(2, 32, 32, 32, 8).cpu().numpy().tobytes() == want.tobytes(), k
    assert applied >= 1


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_step_gradients_on_the_mixed_batch(kind, monkeypatch):
    """The bound of tests/test_cnn_augment_gpu.py::test_one_step_gradients_on_the_augmented_batch,
    ``max(2e-4, 4 x torch fp32's error)`` on the HIP forward's ReLU and near-tie pool decisions, with the
    oracle's mixed batch and mixed target rows as the reference's inputs."""
    import test_hip_step_parity as P
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn_hip import HipPopJob
    x, y, fold, plan = P._setup(P.GENES[0])
    mix = {"kind": kind, "alpha": 2, "prob": 1.0}
    cfg = E.TrainConfig(epochs=(1,), learning_rate=(1.0,), batch_size=32, dropout=0.0, loss="ce", dtype="fp32",
                        optimizer="sgd", momentum=0.9, use_graph=False, augment=TA.AUG, mix=mix)
    job = HipPopJob(plan, x, y, [fold], cfg, _dev(), fold_ids=[0])
    job.init_params()
    w0 = P._hip_weights(job)
    job.reset_optimizer(1.0)
    job._new_epoch_order()
    idx = job.epoch_idx[0].cpu().numpy()
    job.train_step()
    torch.cuda.synchronize()
    got = P._hip_grads(job)
    oh = np.asarray(y, np.float32)[idx]
    xa, tm = R.mixed_step(np.asarray(x, np.float32), idx, oh, [32], job.aug_seeds, job.fold_ids, 1, mix, TA.AUG, (32, 32))
    assert tm.tobytes() != oh.tobytes()
    xb, yb = torch.from_numpy(xa[0]).permute(0, 3, 1, 2), torch.from_numpy(tm[0]).double()
    masks = {L.name: (job.act[L.name][0][..., :L.cout] > 0).permute(0, 3, 1, 2).cpu() for L in job.layers}
    monkeypatch.setattr(P, "F", TA._HipPoolDecisions(job, plan))
    ref = P._reference_grads(plan, w0, xb, yb, "ce", masks=masks)
    r32 = P._reference_grads(plan, w0, xb, yb, "ce", torch.float32, masks=masks)
    checked = 0
    for k, r in ref.items():
        for j, rj in enumerate(r if isinstance(r, tuple) else (r,)):
            if rj.abs().max() > 0:
                gj, tj = (got[k][j], r32[k][j]) if isinstance(r, tuple) else (got[k], r32[k])
                e, e32 = P._rel(gj, rj), P._rel(tj, rj)
                print("[cnn-mix parity] {} {}[{}]: HIP {:.2e}  torch fp32 {:.2e}".format(kind, k, j, e, e32))
                assert e < max(2e-4, 4 * e32), (k, j, e, e32)
                checked += 1
    assert checked >= len(job.layers) + 4


def test_batch_invariance_and_issue_paths(monkeypatch):
    """A candidate's result is the same alone or batched, and graph = eager = native step program."""
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models import cnn_hip
    x, y, folds = TA._data32(320)
    plans = TA._headline_plans(TA.G3)
    cfg = _cfg(_mix("mixup"), TA.AUG)
    alone = E.make_job("hip", plans[0], x, y, folds, cfg, _dev()).launch().finish()
    members = [(plans[1], folds, [0, 1]), (plans[0], folds, [0, 1]), (plans[2], [folds[1]], [1])]
    assert E.make_population_job("hip", members, x, y, cfg, _dev()).launch().finish()[1] == alone
    assert E.make_job("hip", plans[0], x, y, folds, _cfg(None, TA.AUG), _dev()).launch().finish() != alone
    fold = (np.arange(128), np.arange(128, 160))                 # 4 steps of 32
    flats = {}
    for mode in ("native", "python", "graph"):
        monkeypatch.setattr(cnn_hip, "NATIVE_STEPS", mode == "native")
        job = E.make_population_job("hip", [(p, [fold], [0]) for p in plans[:2]], x, y,
                                    _cfg(_mix("cutmix"), use_graph=mode == "graph"), _dev())
        job.launch().finish()
        torch.cuda.synchronize()
        assert job.state[5].item() == 4
        flats[mode] = job.flat.detach().cpu().clone()
    assert torch.equal(flats["native"], flats["python"]) and torch.equal(flats["native"], flats["graph"])


def _scalars(a):
    """The non-pointer fields of an argument block, nested blocks included."""
    from gentun_amd.ops import cnn_kernels as K
    out = []
    for name, typ in a._fields_:
        v = getattr(a, name)
        if isinstance(v, K.C.Structure):
            out.append((name, _scalars(v)))
        elif typ in (K.C.c_int, K.C.c_uint, K.C.c_long, K.C.c_float):
            out.append((name, v))
    return out


def test_off_is_off():
    """``mix=None`` is a config that never mentions it: the same plan and the same arguments (two jobs own
    different buffers, so the pointers are left out of the comparison; every other field is compared)."""
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.cnn_hip import HipPopJob
    from gentun_amd.ops import cnn_kernels as K
    x, y, folds = TA._data32(96)
    plan = TA._headline_plans(TA.G3[:1])[0]
    base = dict(epochs=(1,), learning_rate=(1e-3,), batch_size=32, reset="all")
    seen = {}
    for key, cfg in (("absent", E.TrainConfig(**base)), ("none", E.TrainConfig(mix=None, **base)),
                     ("on", E.TrainConfig(mix=_mix("mixup"), **base))):
        job = HipPopJob(plan, x, y, folds, cfg, _dev(), fold_ids=[0, 1])
        ops = job._step_plan() + job._adam_plan()
        seen[key] = ([op[1] if op[0] == "k" else op[0] for op in ops],
                     [(type(a).__name__, _scalars(a)) for op in ops if op[0] == "k" for a in op[2]
                      if isinstance(a, K.C.Structure)],
                     job.aug_x, job.mix_args, job.head_mix_args)
    assert seen["none"][2:] == (None, None, None) and seen["absent"][2:] == (None, None, None)
    names, on = seen["none"][0], seen["on"][0]
    assert seen["absent"][0] == names and "gt_augment_mix" not in names and "gt_head_mix" not in names
    assert seen["absent"][1] == seen["none"][1]
    assert on[:2] == ["gt_step_begin", "gt_augment_mix"]
    assert [n.replace("gt_head_mix", "gt_head") for n in on[:1] + on[2:]] == names     # one launch more, one swapped


@pytest.mark.parametrize("shape", [(32, 32, 3), (28, 28, 1)])
def test_first_layer_stays_on_the_shape_specialised_kernels(shape):
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models.genome import make_plan
    from gentun_amd.ops import cnn_kernels as K
    from gentun_amd.utils.data import make_image_classification, stratified_kfold
    x, y = make_image_classification(n=96, shape=shape, classes=10, seed=1)
    folds = stratified_kfold(np.argmax(y, 1), 2, seed=0)
    plans = [make_plan(g, (3, 5), shape, (20, 50), ((5, 5), (5, 5)), 500, 10) for g in TA.G3[:2]]
    job = E.make_population_job("hip", [(p, folds, [0, 1]) for p in plans], x, y, _cfg(_mix("cutmix")), _dev())
    L, firsts = K.lib(), 0
    for kind, a, Lr in job.train_fwd_ops + job.bwd_ops:
        if kind == "conv":
            assert L.gt_conv_fast_probe_any(a) == 1, Lr.name                   # 0 generic launches
        elif kind == "wgrad":
            assert L.gt_wgrad_fast_band(a.KH, a.KW, a.Cinp, a.Coutp, a.H, a.W, a.prec) > 0, Lr.name
        if kind in ("conv", "wgrad") and a.gather:
            firsts += 1
            assert a.inp[0] == job.aug_x.data_ptr() and a.gather == job.aug_table.data_ptr()
    assert firsts == 2 and tuple(job.aug_x.shape[1:]) == (32, 32, 8)
    res = job.launch().finish()
    assert all(np.isfinite(v) for r in res for v in r["val_loss"])


def test_hip_data_parallel_with_mix_is_refused():
    from gentun_amd.models.cnn_hip import HipPopJob
    x, y, folds = TA._data32(96)
    with pytest.raises(ValueError, match="mix with dp_group"):
        HipPopJob(TA._headline_plans(TA.G3[:1])[0], x, y, folds, _cfg(_mix("mixup"), dp_group=object()), _dev(),
                  fold_ids=[0, 1])
