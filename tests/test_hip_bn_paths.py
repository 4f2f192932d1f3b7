"""BatchNorm kernels (csrc/hip/cnn_bn.hip) on the paths every BatchNorm search runs and
tests/test_hip_bn.py leaves at zero: the padded real extent (BnArgs::Hr / Wr), the 2x2 max-pool and argmax
mask fused into bn_apply_kernel, small counts (N = 196) where a one-pixel count error shows, the saved
statistics, ``valid`` read at StepState.cur_step = 1, a group of 0 valid rows, chunk tails. Every quantity is
compared with the fp64 oracle of tests/bn_ref.py through bn_compare, whose bounds come from the error of
stock torch fp32 against the same oracle; tests/test_bn_ref.py shows on the CPU that this comparison fails
a transcription of the kernels with any of seven planted faults. Measured table:
profiles/bn_kernel_accuracy.txt."""

import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

SENT = -7.5                # sentinel of every output buffer: exact in bf16, no value a kernel writes (y >= 0, rstd > 0)
BIT_POOL = 1 << 24


class _Run(object):
    """One case's device buffers and launches."""

    def __init__(self, case, prec, large_mean=False, use_valid=True):
        from gentun_amd.ops import cnn_kernels as K
        self.K, self.L = K, K.lib()
        self.case, self.prec, self.use_valid = case, prec, use_valid
        self.B, self.H, self.W, self.Hr, self.Cp, self.C, self.pooled, chunk = R.CASES[case]
        self.chunk = K.bn_chunk_px(self.H, self.W, self.Cp)        # as the executor computes it
        assert self.chunk == chunk, "bn_chunk_px changed: the cases' chunk tails were worked out for the old rule"
        self.dev = torch.device("cuda", 0)
        self.adt = torch.float32 if prec else torch.bfloat16
        self.inp = R.make_inputs(case, prec, large_mean=large_mean)
        self.nv = R.valid_rows(self.B)[1] if use_valid else [self.B] * R.Q
        d = self.dev
        self.z = self.inp["z"].to(d, self.adt)
        assert torch.equal(self.z.float().cpu(), self.inp["z"])     # the oracle sees what the kernel sees
        self.gamma, self.beta = self.inp["gamma"].to(d), self.inp["beta"].to(d)
        self.valid = torch.tensor(R.valid_rows(self.B), dtype=torch.int32, device=d) if use_valid else None
        self.st = torch.zeros(8, dtype=torch.int32, device=d)
        self.st[1] = 1                                              # StepState.cur_step
        self.stream = torch.cuda.current_stream().cuda_stream

    def args(self, table, buf, B, nchunk, train, y):
        K, a = self.K, self.K.BnArgs()
        tab = torch.tensor([[g, 0, BIT_POOL if g in R.POOLED else 0, 0] for g in table], dtype=torch.int32,
                           device=self.dev)
        buf.setdefault("keep", []).append(tab)
        a.z, a.y, a.gamma, a.beta = buf["z"].data_ptr(), y.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr()
        a.stat, a.run, a.part = buf["stat"].data_ptr(), buf["run"].data_ptr(), buf["part"].data_ptr()
        a.ggamma, a.gbeta = buf["gg"].data_ptr(), buf["gb"].data_ptr()
        a.gtab, a.valid, a.st = tab.data_ptr(), self.valid.data_ptr() if self.valid is not None else 0, \
            self.st.data_ptr()
        a.ngroups, a.G, a.B, a.HW, a.Cp = len(table), R.Q, B, self.H * self.W, self.Cp
        a.nchunk, a.chunk_px = nchunk, self.chunk
        a.momentum, a.eps, a.train, a.prec = R.MOMENTUM, R.EPS, train, self.prec
        a.W, a.Hr, a.Wr = self.W, self.Hr, self.Hr
        if self.pooled:
            a.pool_y = buf["pool_y"].data_ptr()
            a.pool_mask = buf["pool_mask"].data_ptr() if train else 0
        assert a.nchunk * a.chunk_px >= B * a.HW                    # every launch stays inside its buffers
        assert not a.pool_y or a.chunk_px % (2 * self.W) == 0      # the fused pool needs whole row pairs per chunk
        return a

    def buffers(self, B, z):
        d, Cp, H, W = self.dev, self.Cp, self.H, self.W
        nchunk = -(-(B * H * W) // self.chunk)
        buf = {"z": z, "nchunk": nchunk,
               "y": torch.full((R.Q, B, H, W, Cp), SENT, dtype=self.adt, device=d),
               "pool_y": torch.full((R.Q, B, H // 2, W // 2, Cp), SENT, dtype=self.adt, device=d),
               "pool_mask": torch.full((R.Q, B, H // 2, W // 2, Cp), 255, dtype=torch.uint8, device=d),
               "stat": torch.full((R.Q, 2, Cp), SENT, device=d),
               "part": torch.full((R.Q, nchunk, 2, Cp), SENT, device=d),
               "gg": torch.full((R.Q, Cp), SENT, device=d), "gb": torch.full((R.Q, Cp), SENT, device=d),
               "run": self.inp["run"].to(d)}
        return buf

    def train_step(self, table):
        """Training forward, then the backward in place on a copy of gy. Host copies of every buffer."""
        K, L = self.K, self.L
        buf = self.buffers(self.B, self.z)
        a = self.args(table, buf, self.B, buf["nchunk"], 1, buf["y"])
        K.check(L.gt_bn_fwd(a, self.stream), "bn_fwd")
        torch.cuda.synchronize()
        out = {k: buf[k].cpu() for k in ("y", "pool_y", "pool_mask", "stat", "run")}
        out["part_fwd"] = buf["part"].cpu()
        buf["dz"] = self.inp["gy"].to(self.dev, self.adt)
        assert torch.equal(buf["dz"].float().cpu(), self.inp["gy"])
        a = self.args(table, buf, self.B, buf["nchunk"], 1, buf["dz"])
        K.check(L.gt_bn_bwd(a, self.stream), "bn_bwd")
        torch.cuda.synchronize()
        out.update({k: buf[k].cpu() for k in ("dz", "gg", "gb")})
        out["part_bwd"] = buf["part"].cpu()
        for k in ("stat", "run", "y", "pool_y", "pool_mask"):          # the backward writes none of them
            assert torch.equal(buf[k].cpu(), out[k]), k
        return buf, out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else
                               torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run_case(case, prec, large_mean=False, use_valid=True):
    r = _Run(case, prec, large_mean, use_valid)
    B, H, W, Hr, Cp, C, pooled = r.B, r.H, r.W, r.Hr, r.Cp, r.C, r.pooled
    hr = Hr or H
    inp, nvs = r.inp, r.nv
    table = list(R.TABLE)
    buf, out = r.train_step(table)
    label = "{}{}{}".format(case, "+100" if large_mean else "", "" if use_valid else " valid=null")
    worst = {}

    def compare(got, ref, tag):
        rows = []
        try:
            R.bn_compare(got, ref, prec, rows)
        finally:
            for q, err, e_t, bound in rows:
                key = tag + q
                if key not in worst or err / max(bound, 1e-300) > worst[key][0] / max(worst[key][2], 1e-300):
                    worst[key] = (err, e_t, bound)

    def oracle(g, nv):
        return R.bn_oracle(inp["z"][g, ..., :C], inp["gamma"][g, :C], inp["beta"][g, :C], inp["run"][:, g, :C], nv,
                           Hr, Hr, R.EPS, R.MOMENTUM, gy=inp["gy"][g, ..., :C], pool=pooled)

    outside = torch.ones(H, W, dtype=torch.bool)
    outside[:hr, :hr] = False
    try:
        for g in table:
            nv = nvs[g]
            y, dz = out["y"][g].float(), out["dz"][g].float()
            # exact zeros outside the real extent and on the padding channels, on every row
            assert float(y[:, outside].abs().max() if Hr else 0.0) == 0.0, "y outside the extent"
            assert float(y[..., C:].abs().max() if Cp > C else 0.0) == 0.0, "y padding channels"
            assert float(dz[:, outside].abs().max() if Hr else 0.0) == 0.0, "dz outside the extent"
            assert float(dz[nv:].abs().max() if nv < B else 0.0) == 0.0, "dz on rows >= nv"
            assert float(dz[..., C:].abs().max() if Cp > C else 0.0) == 0.0, "dz padding channels"
            assert bool(torch.isfinite(y).all())
            if pooled and g in R.POOLED:
                # the values exactly as stored in y, and pool_fwd_kernel's mask of them
                assert _same(out["pool_y"][g], R.max_pool(out["y"][g].float()).to(r.adt)), "pool_y != max_pool2d(y)"
                assert torch.equal(out["pool_mask"][g], R.pool_mask_encode(y)), "pool_mask"
                assert int(out["pool_mask"][g].max()) <= 7
            elif pooled:
                assert float((out["pool_y"][g].float() - SENT).abs().max()) == 0.0, "pool_y of an unpooled group"
                assert int(out["pool_mask"][g].min()) == 255, "pool_mask of an unpooled group"
            if nv == 0:
                assert _same(out["run"][:, g], inp["run"][:, g]), "run of a group without rows"
                assert float((out["stat"][g] - SENT).abs().max()) == 0.0, "stat of a group without rows"
                assert float(dz.abs().max()) == 0.0 and float(out["gg"][g].abs().max()) == 0.0 \
                    and float(out["gb"][g].abs().max()) == 0.0
                continue
            ref = oracle(g, nv)
            got = {"mean": out["stat"][g, 0, :C], "rstd": out["stat"][g, 1, :C],
                   "run_mean": out["run"][0, g, :C], "run_var": out["run"][1, g, :C], "y": y[..., :C],
                   "dz": dz[..., :C], "dgamma": out["gg"][g, :C], "dbeta": out["gb"][g, :C]}
            if pooled and g in R.POOLED:
                got["pool_y"] = out["pool_y"][g].float()[..., :C]
            compare(got, ref, "")
        # group 1 is not in the table: every slice of it is bit-unchanged
        for k in ("y", "pool_y", "pool_mask", "stat", "part_fwd", "part_bwd", "gg", "gb"):
            s = out[k][1].float()
            assert float((s - (255 if k == "pool_mask" else SENT)).abs().max()) == 0.0, k + " of group 1"
        assert _same(out["run"][:, 1], inp["run"][:, 1]) and _same(out["dz"][1], inp["gy"][1].to(r.adt))
        assert _same(buf["z"].cpu(), inp["z"].to(r.adt)), "z is read-only"

        # ---- launch invariance: group 2 alone, and with the full table in another order
        keys = ("y", "stat", "run", "part_fwd", "part_bwd", "dz", "gg", "gb") + (("pool_y", "pool_mask") if pooled else ())
        for tab in ([2], [3, 0, 2, 4]):
            _, o2 = r.train_step(tab)
            for k in keys:
                a, b = (o2[k][:, 2], out[k][:, 2]) if k == "run" else (o2[k][2], out[k][2])
                assert _same(a, b), "{} of group 2 depends on the launch ({})".format(k, tab)

        # ---- the separate pool kernel on the kernel's own y
        if pooled:
            K = r.K
            py = torch.full_like(buf["pool_y"], SENT)
            pm = torch.full_like(buf["pool_mask"], 255)
            K.check(r.L.gt_pool_fwd_mask(buf["y"].data_ptr(), 0, 0, py.data_ptr(), R.Q * B, B, H, W, Cp, pm.data_ptr(),
                                         prec, r.stream), "pool_fwd_mask")
            torch.cuda.synchronize()
            for g in R.POOLED:
                assert _same(py[g].cpu(), out["pool_y"][g]) and torch.equal(pm[g].cpu(), out["pool_mask"][g]), \
                    "fused pool != pool_fwd_kernel"

        # ---- evaluation forward at another batch, as HipPopJob._eval_ops: train = 0, no mask, B = EB
        EB = B + 1
        gen = torch.Generator().manual_seed(7)
        ze = torch.zeros(R.Q, EB, H, W, Cp)
        ze[:, :B] = inp["z"]
        ze[:, B] = inp["z"][:, 0].flip(0)
        ze[:, B, ..., :C] += torch.randint(-1, 2, (R.Q, H, W, C), generator=gen).float()
        if Hr:
            ze[:, B, Hr:] = inp["z"][0, 0, Hr, 0, 0]
            ze[:, B, :, Hr:] = inp["z"][0, 0, Hr, 0, 0]
        ze = ze.to(r.adt).float()
        eb = r.buffers(EB, ze.to(r.dev, r.adt))
        eb["stat"], eb["run"], eb["part"], eb["pool_mask"] = buf["stat"], buf["run"], buf["part"], buf["pool_mask"]
        a = r.args(table, eb, EB, eb["nchunk"], 0, eb["y"])
        assert a.pool_mask in (0, None) and a.train == 0 and a.B == EB
        K = r.K
        K.check(r.L.gt_bn_fwd(a, r.stream), "bn_fwd(eval)")
        torch.cuda.synchronize()
        for k, k0 in (("stat", "stat"), ("run", "run"), ("part", "part_bwd"), ("pool_mask", "pool_mask")):
            assert _same(eb[k].cpu(), out[k0]), k + " written by the evaluation forward"
        ye, pe = eb["y"].cpu().float(), eb["pool_y"].cpu().float()
        for g in table:
            ref = R.bn_oracle_eval(ze[g, ..., :C], inp["gamma"][g, :C], inp["beta"][g, :C], out["run"][:, g, :C],
                                   Hr, Hr, R.EPS, pool=pooled)
            got = {"y": ye[g, ..., :C]}
            assert float(ye[g][:, outside].abs().max() if Hr else 0.0) == 0.0
            assert float(ye[g][..., C:].abs().max() if Cp > C else 0.0) == 0.0
            if pooled and g in R.POOLED:
                got["pool_y"] = pe[g, ..., :C]
                assert _same(pe[g], R.max_pool(ye[g])), "evaluation pool_y != max_pool2d(y)"
            elif pooled:
                assert float((pe[g] - SENT).abs().max()) == 0.0
            compare(got, ref, "eval ")
        assert float((ye[1] - SENT).abs().max()) == 0.0 and float((pe[1] - SENT).abs().max()) == 0.0
    finally:
        for key in sorted(worst):
            err, e_t, bound = worst[key]
            print("[bn-acc] case {:14s} {} {:14s} rel.err HIP {:.2e}  torch-fp32 {:.2e}  bound {:.2e}".format(
                label, "fp32" if prec else "bf16", key, err, e_t, bound))


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_bn_paths_match_fp64_oracle(case, prec):
    _run_case(case, prec)


@pytest.mark.parametrize("prec", [1, 0])
def test_bn_paths_without_valid(prec):
    """valid = null: every group is full."""
    _run_case("a", prec, use_valid=False)


@pytest.mark.parametrize("prec", [1, 0])
def test_bn_paths_large_mean(prec):
    """z = randn + 100: the shift k = z at pixel 0 keeps S2/n - m1^2 free of cancellation. On the CPU
    transcription the shifted sums are off by 3e-6 and the unshifted ones by 7e-4 (y, fp32)."""
    _run_case("a", prec, large_mean=True)
