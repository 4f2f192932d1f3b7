"""Plain references for the BatchNorm kernels (csrc/hip/cnn_bn.hip). Torch on the CPU only: nothing here
imports the GPU.

``bn_oracle`` / ``bn_oracle_eval``  fp64 oracle of one group: statistics over the real rows and the real
                                    pixels, output for every row, running statistics, autograd gradients,
                                    2x2 max-pool and its argmax mask; next to each quantity the error of stock
                                    torch fp32 against the same oracle (``E_torch``), which sets the bounds
``bn_emulate_fp32``                 fp32 transcription of the four kernels' arithmetic with named mutants. It
                                    is NOT a second oracle: tests/test_bn_ref.py uses it to show that
                                    ``bn_compare`` catches each mutant
``bn_compare``                      the one comparison (errors and bounds) of the CPU and the GPU tests
``CASES`` / ``make_inputs``         geometries and inputs of tests/test_hip_bn_paths.py, shared with the CPU test
"""

import torch
import torch.nn.functional as F

# (B, H, W, Hr, Cp, C, pooled, chunk_px): chunk_px is cnn_kernels.bn_chunk_px(H, W, Cp) worked out by hand; the
# tests assert it so that a change of the rule is noticed
CASES = {
    "a": (3, 16, 16, 14, 24, 20, True, 512),     # chunks straddle images, last chunk 256 px; N = 196 at nv = 1
    "b": (2, 32, 32, 28, 8, 3, True, 512),       # nc8 = 1 (256 pixel-threads per chunk), half-image chunks
    "c": (2, 16, 16, 14, 128, 128, True, 128),   # no padding channels, chunks of 8 rows
    "d": (2, 64, 64, 56, 8, 3, True, 512),       # the 56-in-64 extent padded_hw also produces
    "e": (2, 8, 8, 0, 256, 250, True, 64),       # unpadded fused pool, all 256 threads own a channel
    "f": (3, 14, 14, 0, 56, 50, False, 256),     # 512 % 2W != 0: chunks cut rows, last chunk 76 px
    "g": (3, 7, 7, 0, 104, 100, False, 128),     # nact = 247, last chunk 19 px
}

Q = 5                                # groups of a case
TABLE = (4, 2, 0, 3)                 # group table: out of order, group 1 absent
POOLED = (4, 2, 3)                   # groups whose GroupRec out_mask has bit 24
EPS, MOMENTUM = 1e-3, 0.99           # Keras' defaults, as TrainConfig

FP32_STORED = ("mean", "rstd", "run_mean", "run_var", "dgamma", "dbeta")     # fp32 in both precisions
ACTIVATIONS = ("y", "pool_y", "dz")                                          # bf16 in prec 0
MUTANTS = ("count_hw", "count_plus_row", "pads_in_sums", "drop_last_chunk", "no_shift", "last_max", "rows_B")


def valid_rows(B):
    """``valid`` [2][Q]: row 0 would be wrong if read (StepState.cur_step is 1), row 1 = real rows per group."""
    return [[1, 1, B, B, 1], [B, B, 1, 0, B]]


def make_inputs(case, prec, large_mean=False, seed=0):
    """z, gy [Q,B,H,W,Cp], gamma, beta [Q,Cp], run [2,Q,Cp] as fp32 tensors whose z / gy values are exact in
    the activation type of ``prec`` (what the kernel sees)."""
    B, H, W, Hr, Cp, C, _, _ = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    z = torch.zeros(Q, B, H, W, Cp)
    if large_mean:
        z[..., :C] = torch.randn(Q, B, H, W, C, generator=gen) + 100
    else:
        ne, no = len(range(0, C, 2)), len(range(1, C, 2))
        z[..., 0:C:2] = torch.randn(Q, B, H, W, ne, generator=gen) * 2 + 3
        z[..., 1:C:2] = torch.randint(-2, 3, (Q, B, H, W, no), generator=gen).float()   # equal z: true ties
    gy = torch.randn(Q, B, H, W, Cp, generator=gen) * (torch.rand(Q, B, H, W, Cp, generator=gen) > 0.3)
    gy[..., C:] = 0
    if Hr:                                            # large finite garbage outside the real extent
        junk = 1e3 if prec else 256.0
        for t in (z, gy):
            t[:, :, Hr:] = junk
            t[:, :, :, Hr:] = junk
    if not prec:
        z, gy = z.bfloat16().float(), gy.bfloat16().float()
    gamma, beta = torch.zeros(Q, Cp), torch.zeros(Q, Cp)
    gamma[:, :C] = torch.rand(Q, C, generator=gen) + 0.5
    beta[:, :C] = torch.randn(Q, C, generator=gen) * 0.5
    gamma[:, 0:C:4] = 0.5                             # zero after ReLU: every pool cell an all-zero tie
    beta[:, 0:C:4] = -10.0
    run = torch.stack([torch.randn(Q, Cp, generator=gen) * 0.1, torch.rand(Q, Cp, generator=gen) + 0.5])
    return {"z": z, "gy": gy, "gamma": gamma, "beta": beta, "run": run}


def rel(a, b):
    """max-abs difference over max-abs of the reference ``b`` (``_rel`` of tests/test_hip_bn.py)."""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _extent(H, W, Hr, Wr):
    return (Hr, Wr) if Hr > 0 else (H, W)


def max_pool(y):
    """2x2 max-pool of y [B,H,W,C]."""
    return F.max_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


def pool_mask_encode(y, last=False):
    """Mask bytes [B,H/2,W/2,C] of pool_fwd_kernel for y [B,H,W,C]: bits 0-1 the index of the first strict
    maximum over (0,0), (0,1), (1,0), (1,1), bit 2 = maximum > 0. ``last``: ties go to the last maximum (the
    ``last_max`` mutant)."""
    v = (y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2])
    m = v[0].clone()
    arg = torch.zeros(m.shape, dtype=torch.uint8)
    for q in (1, 2, 3):
        up = v[q] >= m if last else v[q] > m
        m = torch.where(up, v[q], m)
        arg = torch.where(up, torch.full_like(arg, q), arg)
    return arg | ((m > 0).to(torch.uint8) << 2)


def _torch_fp32(z, gamma, beta, run, nv, Hr, Wr, eps, momentum, gy, pool):
    """Stock torch fp32 on the cropped tensor: the reference whose own error sets the bounds."""
    x = z[:nv, :Hr, :Wr].float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w, b = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    rm, rv = run[0].float().clone(), run[1].float().clone()
    out = F.batch_norm(x, rm, rv, w, b, True, 1.0 - momentum, eps)
    with torch.no_grad():
        _, sm, si = torch.native_batch_norm(x.detach(), w.detach(), b.detach(), None, None, True, 0.0, eps)
    y = torch.relu(out.detach()).permute(0, 2, 3, 1)
    t = {"mean": sm, "rstd": si, "run_mean": rm, "run_var": rv, "y": y}
    if gy is not None:
        out.backward(gy[:nv, :Hr, :Wr].float().permute(0, 3, 1, 2))
        t.update(dz=x.grad.permute(0, 2, 3, 1), dgamma=w.grad, dbeta=b.grad)
    if pool:
        t["pool_y"] = max_pool(y)
    return t


def bn_oracle(z, gamma, beta, run, nv, Hr, Wr, eps, momentum, gy=None, pool=False):
    """fp64 oracle of one group. z [B,H,W,C] as the kernel sees it, gamma / beta [C], run [2,C], nv >= 1 real
    rows, Hr x Wr the real extent (0: all of H x W). Returns mean, var (biased), rstd, y [B,H,W,C] (every row
    normalised with the batch statistics, 0 outside the extent), run_mean, run_var (unbiased) after one
    update; with ``gy`` dz (zero-embedded), dgamma, dbeta; with ``pool`` pool_y and pool_mask; and E_torch, the
    error of stock torch fp32 per quantity against these values."""
    z, gamma, beta, run = z.double(), gamma.double(), beta.double(), run.double()
    B, H, W, C = z.shape
    Hr, Wr = _extent(H, W, Hr, Wr)
    assert 1 <= nv <= B
    x = z[:nv, :Hr, :Wr]
    n = nv * Hr * Wr
    mean = x.mean((0, 1, 2))
    var = ((x - mean) ** 2).mean((0, 1, 2))
    rstd = 1.0 / torch.sqrt(var + eps)
    y = torch.zeros_like(z)
    y[:, :Hr, :Wr] = torch.relu(gamma * (z[:, :Hr, :Wr] - mean) * rstd + beta)
    unb = var * n / (n - 1) if n > 1 else var
    ref = {"mean": mean, "var": var, "rstd": rstd, "y": y,
           "run_mean": momentum * run[0] + (1 - momentum) * mean,
           "run_var": momentum * run[1] + (1 - momentum) * unb}
    if gy is not None:
        xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        w, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        F.batch_norm(xc, None, None, w, b, True, 0.0, eps).backward(gy[:nv, :Hr, :Wr].double().permute(0, 3, 1, 2))
        dz = torch.zeros_like(z)
        dz[:nv, :Hr, :Wr] = xc.grad.permute(0, 2, 3, 1)
        ref.update(dz=dz, dgamma=w.grad, dbeta=b.grad)
    if pool:
        ref["pool_y"] = max_pool(y)
        ref["pool_mask"] = pool_mask_encode(y)
    t = _torch_fp32(z, gamma, beta, run, nv, Hr, Wr, eps, momentum, gy, pool)
    crop = {"y": (Hr, Wr), "dz": (Hr, Wr), "pool_y": (Hr // 2, Wr // 2)}     # torch saw the real rows and pixels
    ref["E_torch"] = {q: rel(v, ref[q][:nv, :crop[q][0], :crop[q][1]] if q in crop else ref[q])
                      for q, v in t.items()}
    return ref


def bn_oracle_eval(z, gamma, beta, run, Hr, Wr, eps, pool=False):
    """fp64 oracle of the evaluation forward (running statistics) of one group: y, pool_y, E_torch."""
    z, gamma, beta, run = z.double(), gamma.double(), beta.double(), run.double()
    B, H, W, C = z.shape
    Hr, Wr = _extent(H, W, Hr, Wr)
    y = torch.zeros_like(z)
    y[:, :Hr, :Wr] = torch.relu(gamma * (z[:, :Hr, :Wr] - run[0]) / torch.sqrt(run[1] + eps) + beta)
    x = z[:, :Hr, :Wr].float().permute(0, 3, 1, 2)
    yt = torch.relu(F.batch_norm(x, run[0].float(), run[1].float(), gamma.float(), beta.float(), False, 0.0, eps))
    yt = yt.permute(0, 2, 3, 1)
    ref = {"y": y, "E_torch": {"y": rel(yt, y[:, :Hr, :Wr])}}
    if pool:
        ref["pool_y"] = max_pool(y)
        ref["E_torch"]["pool_y"] = rel(max_pool(yt), ref["pool_y"][:, :Hr // 2, :Wr // 2])
    return ref


def bn_emulate_fp32(z, gamma, beta, run, nv, Hr, Wr, eps, momentum, chunk_px, gy=None, pool=False, prec=1,
                    mutant=None):
    """torch-fp32 transcription of bn_stats / bn_apply / bn_bwd_stats / bn_bwd_apply for one group: shift
    k = z at pixel 0, per-chunk S1 / S2 summed in chunk order, var = max(S2/n - m1^2, 0), the sc / sh apply,
    the backward's two sums. ``mutant`` (one of MUTANTS) plants a named fault."""
    assert mutant is None or mutant in MUTANTS
    f32 = torch.float32
    z, gamma, beta, run = z.to(f32), gamma.to(f32), beta.to(f32), run.to(f32)
    B, H, W, C = z.shape
    HW = H * W
    Hr, Wr = _extent(H, W, Hr, Wr)
    rows = B if mutant == "rows_B" else nv
    zf = z.reshape(B * HW, C)
    p = torch.arange(B * HW)
    pad = ((p % HW) // W >= Hr) | ((p % HW) % W >= Wr)
    skip = torch.zeros_like(pad) if mutant == "pads_in_sums" else pad
    npx = rows * HW
    nch = -(-npx // chunk_px)
    if mutant == "drop_last_chunk" and npx % chunk_px:
        nch -= 1
    n = rows * (HW if mutant == "count_hw" else Hr * Wr) + (Wr if mutant == "count_plus_row" else 0)
    nf = torch.tensor(float(n), dtype=f32)

    def chunk_sums(a, b):
        s1, s2 = torch.zeros(C, dtype=f32), torch.zeros(C, dtype=f32)
        for c in range(nch):
            lo, hi = c * chunk_px, min((c + 1) * chunk_px, npx)
            keep = ~skip[lo:hi]
            s1 = s1 + a[lo:hi][keep].sum(0)
            s2 = s2 + b[lo:hi][keep].sum(0)
        return s1, s2

    k = torch.zeros(C, dtype=f32) if mutant == "no_shift" else zf[0].clone()
    d = zf - k
    s1, s2 = chunk_sums(d, d * d)
    m1 = s1 / nf
    var = torch.clamp(s2 / nf - m1 * m1, min=0.0)
    mean = k + m1
    rstd = torch.rsqrt(var + eps)
    unb = var * nf / (nf - 1.0) if n > 1 else var
    out = {"mean": mean, "rstd": rstd, "run_mean": momentum * run[0] + (1.0 - momentum) * mean,
           "run_var": momentum * run[1] + (1.0 - momentum) * unb}
    sc = gamma * rstd
    sh = beta - mean * gamma * rstd
    y = torch.relu(zf * sc + sh)
    y[pad] = 0.0
    if not prec:
        y = y.bfloat16().float()
    out["y"] = y.reshape(B, H, W, C)
    if pool:
        out["pool_y"] = max_pool(out["y"])
        out["pool_mask"] = pool_mask_encode(out["y"], last=mutant == "last_max")
    if gy is not None:
        g = gy.to(f32).reshape(B * HW, C)
        xh = (zf - mean) * rstd
        sg, sgx = chunk_sums(g, g * xh)
        inv_n = 1.0 / nf
        dz = sc * (g - sg * inv_n - xh * (sgx * inv_n))
        dz[pad | (p >= npx)] = 0.0
        if not prec:
            dz = dz.bfloat16().float()
        out.update(dz=dz.reshape(B, H, W, C), dgamma=sgx, dbeta=sg)
    return out


def bn_bound(q, prec, e_torch):
    """Bound of quantity ``q``: bf16-stored activations keep the project's 2e-2; everything stored in fp32
    gets min(1e-4, max(1e-5, 8 x E_torch)): 1e-4 is the tol of test_bn_kernels_match_batchnorm2d, 1e-5 the
    TOL of tests/test_hip_fp32.py, E_torch the error of stock torch fp32 against the same oracle and 8 a
    margin over it (the kernel applies z*sc + sh, which costs 1.5 to 3.7 times torch's centred form)."""
    if q in ACTIVATIONS and not prec:
        return 2e-2
    return min(1e-4, max(1e-5, 8.0 * e_torch))


def bn_compare(got, ref, prec, rows=None):
    """Compare the quantities of ``got`` with the oracle ``ref`` (bn_oracle / bn_oracle_eval). Returns
    {quantity: error}; appends (quantity, error, E_torch, bound) to ``rows`` before it asserts the bounds.
    ``pool_mask`` is compared byte for byte (error = fraction of differing bytes, bound 0)."""
    errs, bad = {}, []
    for q, v in got.items():
        if q == "pool_mask":
            assert v.dtype == torch.uint8 and v.shape == ref[q].shape
            err, e_t, bound = (v.cpu() != ref[q]).double().mean().item(), 0.0, 0.0
            ok = err == 0.0
        else:
            assert q in FP32_STORED or q in ACTIVATIONS, q
            assert tuple(v.shape) == tuple(ref[q].shape), (q, v.shape, ref[q].shape)
            e_t = ref["E_torch"][q]
            err, bound = rel(v, ref[q]), bn_bound(q, prec, e_t)
            ok = err < bound                           # NaN fails
        errs[q] = err
        if rows is not None:
            rows.append((q, err, e_t, bound))
        if not ok:
            bad.append("{}: {:.3e} (bound {:.3e}, E_torch {:.3e})".format(q, err, bound, e_t))
    assert not bad, "; ".join(bad)
    return errs
