"""Two-pass patch staging of the stage-2 3x3 fp32 conv (ConvArgs::twopass, conv_fast_impl.h TWO): the same
MFMAs in the same order from half the LDS, so every output must be BIT-identical to the default 8-row tile's --
forward (both weight layouts, N-ary input sum with its write-back, fused pool, padded geometry) and data
gradient (fan-out with accumulate and ReLU mask) -- and the forward within the fp32 tolerance of the fp64
oracle. 16x16, 50 real channels (56 padded); the small-launch rule is switched off so these small launches
run the 8-row tiles."""

import math

import pytest
import torch
import torch.nn.functional as F

from test_hip_fp32 import DEV, TOL, K, _split, nhwc_pad, pack_w, rel, report, stream

H = W = 16
C, CP, B = 50, 56, 2


@pytest.fixture()
def tiles8():
    """8-row tiles for any launch size (gt_conv_set_smallq(0)), restored afterwards."""
    L = K().lib()
    old = L.gt_conv_set_smallq(0)
    yield L
    L.gt_conv_set_smallq(old)


def _both(L, a, outs, reset=None):
    """Launch `a` with the field clear, then set, on the same buffers; the outputs of each run."""
    Km = K()
    res = []
    for two in (0, 1):
        if reset:
            reset()
        a.twopass = two
        assert L.gt_conv_fast_twopass(a) == two          # the variant really runs (and only when asked for)
        Km.check(L.gt_conv_fwd(a, stream()), "conv")
        torch.cuda.synchronize()
        res.append([t.clone() for t in outs])
    return res


def _fwd_args(Km, G, nin, wfrag, seed):
    torch.manual_seed(seed)
    xs = [torch.randn(G, B, C, H, W) for _ in range(nin)]
    w = torch.randn(G, C, C, 3, 3) / math.sqrt(C * 9)
    b = torch.randn(G, C) * 0.1
    x_in = [torch.stack([nhwc_pad(x[g], CP) for g in range(G)]).to(DEV).contiguous() for x in xs]
    wp = torch.stack([pack_w(w[g], CP, CP) for g in range(G)]).to(DEV)
    wpl = Km.frag_planes(wp.contiguous(), W) if wfrag else _split(wp).contiguous()
    bp = torch.zeros(G, CP, device=DEV)
    bp[:, :C] = b.to(DEV)
    out = torch.full((G, B, H, W, CP), 7.0, device=DEV)
    a = Km.ConvArgs()
    for i, t in enumerate(x_in):
        a.inp[i] = t.data_ptr()
    a.out[0] = out.data_ptr()
    a.ngroups, a.relu, a.epi_bf16 = G, 1, 1
    a.w, a.bias, a.wps = wpl.data_ptr(), bp.data_ptr(), wpl[0].numel()
    a.G, a.B, a.H, a.W, a.Cinp, a.Coutp, a.KH, a.KW = G, B, H, W, CP, CP, 3, 3
    a.TH = Km.conv_tile_rows(H, W)
    a.prec, a.cout_real, a.wfrag = 1, C, wfrag
    return a, out, (xs, w, b), [x_in, wpl, bp]


def _gtab(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("wfrag", [0, 1])
def test_forward_bias_relu(tiles8, wfrag):
    """Bias + ReLU forward, row-major and fragment-major weights: bitwise equal, and within TOL of fp64."""
    Km = K()
    G = 2
    a, out, (xs, w, b), keep = _fwd_args(Km, G, 1, wfrag, 30)
    rows = _gtab([[g, 1, 1, 0] for g in range(G)])
    a.gtab = rows.data_ptr()
    (off,), (on,) = _both(tiles8, a, [out])
    assert torch.equal(off, on)
    worst = 0.0
    for g in range(G):
        ref = F.relu(F.conv2d(xs[0][g].double(), w[g].double(), b[g].double(), padding=1))
        worst = max(worst, rel(on[g, ..., :C].permute(0, 3, 1, 2), ref))
        assert torch.all(on[g, ..., C:] == 0)
    report("conv_fwd two-pass 16x16 50->50{}".format(" wfrag" if wfrag else ""), worst, float("nan"))
    assert worst < TOL


@pytest.mark.gpu
def test_forward_input_sum_and_writeback(tiles8):
    """Two summed input slots: output and the summed-input write-back (every chunk of both parts exactly once)."""
    Km = K()
    a, out, (xs, w, b), keep = _fwd_args(Km, 1, 2, 1, 31)
    rows = _gtab([[0, 0b11, 1, 0]])
    xsum = torch.full((1, B, H, W, CP), 3.0, device=DEV)
    a.gtab, a.xsum = rows.data_ptr(), xsum.data_ptr()
    off, on = _both(tiles8, a, [out, xsum], reset=lambda: xsum.fill_(3.0))
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])
    assert torch.equal(on[1][0, ..., :C].permute(0, 3, 1, 2).cpu(), xs[0][0] + xs[1][0])
    assert torch.all(on[1][..., C:] == 0)
    ref = F.relu(F.conv2d((xs[0][0] + xs[1][0]).double(), w[0].double(), b[0].double(), padding=1))
    assert rel(on[0][0, ..., :C].permute(0, 3, 1, 2), ref) < TOL


@pytest.mark.gpu
def test_forward_fused_pool(tiles8):
    """The fused 2x2 max-pool and its argmax mask."""
    Km = K()
    G = 2
    a, out, _, keep = _fwd_args(Km, G, 1, 1, 32)
    rows = _gtab([[g, 1, 1 | (1 << 24), 0] for g in range(G)])
    py = torch.full((G, B, H // 2, W // 2, CP), 5.0, device=DEV)
    pm = torch.full((G * B, H // 2, W // 2, CP), 9, dtype=torch.uint8, device=DEV)
    a.gtab, a.pool_y, a.pool_mask = rows.data_ptr(), py.data_ptr(), pm.data_ptr()

    def reset():
        py.fill_(5.0)
        pm.fill_(9)
    off, on = _both(tiles8, a, [out, py, pm], reset=reset)
    for x, y in zip(off, on):
        assert torch.equal(x, y)
    pooled = F.max_pool2d(on[0].flatten(0, 1).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(on[1], pooled.reshape(py.shape))


@pytest.mark.gpu
def test_forward_padded_geometry(tiles8):
    """A 14x14 image stored in 16x16 (Hr = Wr = 14): exact zeros outside the real rows / columns."""
    Km = K()
    G = 2
    a, out, _, keep = _fwd_args(Km, G, 1, 0, 33)
    rows = _gtab([[g, 1, 1, 0] for g in range(G)])
    a.gtab, a.Hr, a.Wr = rows.data_ptr(), 14, 14
    (off,), (on,) = _both(tiles8, a, [out])
    assert torch.equal(off, on)
    assert torch.all(on[:, :, 14:] == 0) and torch.all(on[:, :, :, 14:] == 0) and on[:, :, :14, :14, :C].abs().sum() > 0


@pytest.mark.gpu
def test_dgrad_fanout_accumulate_mask(tiles8):
    """Data gradient into two slots: slot 0 written, slot 1 accumulated and ReLU-masked."""
    Km = K()
    torch.manual_seed(34)
    w = torch.randn(1, C, C, 3, 3) / math.sqrt(C * 9)
    dz = torch.randn(1, B, C, H, W)
    wp = torch.stack([pack_w(w[0], CP, CP)]).to(DEV)
    wT = Km.frag_planes(wp.contiguous(), W, dgrad=True)
    dz_p = torch.stack([nhwc_pad(dz[0], CP)]).to(DEV).contiguous()
    out0 = torch.zeros(1, B, H, W, CP, device=DEV)
    prev = torch.randn(1, B, H, W, CP, device=DEV)
    prev[..., C:] = 0
    out1 = prev.clone()
    pmask = torch.randn(1, B, H, W, CP, device=DEV)
    rows = _gtab([[0, 1, 0b11 | (0b10 << 8) | (0b10 << 16), 0]])
    a = Km.ConvArgs()
    a.inp[0] = dz_p.data_ptr()
    a.out[0], a.out[1] = out0.data_ptr(), out1.data_ptr()
    a.out_mask[1] = pmask.data_ptr()
    a.gtab, a.ngroups, a.relu = rows.data_ptr(), 1, 0
    a.w, a.bias, a.wps = wT.data_ptr(), 0, wT[0].numel()
    a.G, a.B, a.H, a.W, a.Cinp, a.Coutp, a.KH, a.KW = 1, B, H, W, CP, CP, 3, 3
    a.TH = Km.conv_tile_rows(H, W)
    a.prec, a.cout_real, a.wfrag = 1, C, 1

    def reset():
        out0.zero_()
        out1.copy_(prev)
    off, on = _both(tiles8, a, [out0, out1], reset=reset)
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])
    ref = torch.nn.grad.conv2d_input((B, C, H, W), w[0].double(), dz[0].double(), padding=1)
    assert rel(on[0][0, ..., :C].permute(0, 3, 1, 2), ref) < TOL
    ref1 = (ref + prev[0, ..., :C].permute(0, 3, 1, 2).double().cpu()) * \
        (pmask[0, ..., :C] > 0).permute(0, 3, 1, 2).cpu()
    assert rel(on[1][0, ..., :C].permute(0, 3, 1, 2), ref1) < TOL


@pytest.mark.gpu
def test_training_is_bit_identical(tiles8):
    """A small population job (2 folds = 2 groups of the S=(3,5) (20, 50) genome, batch 8, 3 Adam steps and
    the evaluation) with the variant off and on: the same losses and the same weights, bit for bit."""
    import numpy as np
    from gentun_amd.models import cnn_engine as E
    from gentun_amd.models import cnn_hip
    from gentun_amd.models.genome import make_plan
    from gentun_amd.utils.data import make_image_classification, stratified_kfold
    x, y = make_image_classification(n=48, shape=(32, 32, 3), classes=10, seed=7, noise=0.35, shift=2)
    folds = stratified_kfold(np.argmax(y, 1), 2, seed=0)          # 24 training rows per fold: 3 steps of 8
    plan = make_plan({'S_1': '101', 'S_2': '0101110011'}, (3, 5), (32, 32, 3), (20, 50), ((5, 5), (5, 5)), 500, 10)
    res, old = {}, cnn_hip.TWOPASS
    try:
        for two in (False, True):
            cnn_hip.TWOPASS = two
            cfg = E.TrainConfig(epochs=(1,), learning_rate=(1e-3,), batch_size=8, dtype="fp32", reset="all")
            job = E.make_job("hip", plan, x, y, folds, cfg, DEV)
            convs = [a for kind, a, _ in job.fwd_ops + job.bwd_ops if kind == "conv"]
            assert any(a.twopass for a in convs) == two
            assert all(a.twopass == 0 or (a.KH, a.Cinp, a.Coutp, a.H) == (3, 56, 56, 16) for a in convs)
            job.launch()
            out = job.finish()
            torch.cuda.synchronize()
            res[two] = (job.flat.detach().cpu().clone(), out)
    finally:
        cnn_hip.TWOPASS = old
    assert torch.equal(res[True][0], res[False][0])
    for key in ("val_loss", "categorical_accuracy"):
        assert np.array_equal(np.asarray(res[True][1][key]), np.asarray(res[False][1][key])), key
    assert np.all(np.isfinite(res[True][1]["val_loss"]))
