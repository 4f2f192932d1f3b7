"""The BatchNorm references (tests/bn_ref.py) checked without a GPU: the fp64 oracle against
torch.nn.BatchNorm2d, the pool-mask encoder against a plain loop on an input that holds every tie situation
by construction, and the comparison function of tests/test_hip_bn_paths.py against an fp32 transcription of
the kernels: it passes the faithful transcription on every case and fails every planted fault."""

import pytest
import torch

import bn_ref as R
from gentun_amd.ops import cnn_kernels as K


# ---- the oracle is BatchNorm2d

def _bn2d(C, gamma, beta, run):
    m = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=1.0 - R.MOMENTUM).double()
    with torch.no_grad():
        m.weight.copy_(gamma)
        m.bias.copy_(beta)
        m.running_mean.copy_(run[0])
        m.running_var.copy_(run[1])
    return m


@pytest.mark.parametrize("B,H,W,Hr,nv", [(3, 6, 6, 0, 3), (3, 8, 8, 6, 3), (4, 8, 8, 6, 2), (2, 4, 6, 0, 1)])
def test_oracle_matches_batchnorm2d(B, H, W, Hr, nv):
    C = 5
    torch.manual_seed(1)
    z = torch.randn(B, H, W, C, dtype=torch.float64) * 2 + 3
    gy = torch.randn(B, H, W, C, dtype=torch.float64)
    gamma, beta = torch.rand(C, dtype=torch.float64) + 0.5, torch.randn(C, dtype=torch.float64)
    run = torch.stack([torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5])
    ref = R.bn_oracle(z, gamma, beta, run, nv, Hr, Hr, R.EPS, R.MOMENTUM, gy=gy, pool=True)
    hr, wr = (Hr, Hr) if Hr else (H, W)
    m = _bn2d(C, gamma, beta, run)
    x = z[:nv, :hr, :wr].permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = m(x)
    out.backward(gy[:nv, :hr, :wr].permute(0, 3, 1, 2))
    tol = 1e-12
    assert R.rel(ref["y"][:nv, :hr, :wr], torch.relu(out).permute(0, 2, 3, 1)) < tol
    assert R.rel(ref["run_mean"], m.running_mean) < tol and R.rel(ref["run_var"], m.running_var) < tol
    assert R.rel(ref["dz"][:nv, :hr, :wr], x.grad.permute(0, 2, 3, 1)) < tol
    assert R.rel(ref["dgamma"], m.weight.grad) < tol and R.rel(ref["dbeta"], m.bias.grad) < tol
    assert R.rel(ref["mean"], x.detach().mean((0, 2, 3))) < tol
    assert R.rel(ref["rstd"], 1 / torch.sqrt(x.detach().var((0, 2, 3), unbiased=False) + R.EPS)) < tol
    # every row (padding rows of a short batch too) is normalised with the batch statistics
    m.eval()
    with torch.no_grad():
        m.running_mean.copy_(ref["mean"])
        m.running_var.copy_(ref["var"])
        yall = torch.relu(m(z[:, :hr, :wr].permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
    assert R.rel(ref["y"][:, :hr, :wr], yall) < tol
    # exact zeros outside the extent and on the rows that are not real
    keep = torch.zeros(B, H, W, dtype=torch.bool)
    keep[:, :hr, :wr] = True
    assert float(ref["y"][~keep].abs().max() if (~keep).any() else 0.0) == 0.0
    keep[nv:] = False
    assert float(ref["dz"][~keep].abs().max() if (~keep).any() else 0.0) == 0.0
    assert torch.equal(ref["pool_y"], R.max_pool(ref["y"]))
    assert torch.equal(ref["pool_mask"], R.pool_mask_encode(ref["y"]))
    # evaluation: running statistics
    m = _bn2d(C, gamma, beta, run).eval()
    ev = R.bn_oracle_eval(z, gamma, beta, run, Hr, Hr, R.EPS, pool=True)
    with torch.no_grad():
        ye = torch.relu(m(z[:, :hr, :wr].permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
    assert R.rel(ev["y"][:, :hr, :wr], ye) < tol
    assert torch.equal(ev["pool_y"], R.max_pool(ev["y"]))


# ---- the mask encoder

def _mask_loop(y):
    B, H, W, C = y.shape
    out = torch.zeros(B, H // 2, W // 2, C, dtype=torch.uint8)
    for b, i, j, c in ((b, i, j, c) for b in range(B) for i in range(H // 2) for j in range(W // 2)
                       for c in range(C)):
        v = [float(y[b, 2 * i + di, 2 * j + dj, c]) for di, dj in ((0, 0), (0, 1), (1, 0), (1, 1))]
        out[b, i, j, c] = v.index(max(v)) | (4 if max(v) > 0 else 0)         # list.index: the first maximum
    return out


def test_pool_mask_encoder_on_every_tie_situation():
    cells = [[0, 0, 0, 0],                           # all zero
             [2, 2, 1, 0], [2, 0, 0, 2],             # positive tie, the first maximum in position 0
             [1, 2, 2, 0], [0, 1, 3, 3], [1, 3, 0, 3],   # positive tie, the first maximum later
             [3, 0, 1, 2], [0, 3, 1, 2], [1, 0, 3, 2], [0, 1, 2, 3],   # a single maximum in each position
             [-1, -2, -2, -1], [-2, -1, -1, -3],     # negative ties: bit 2 clear
             [2, 2, 2, 2], [0, -1, 0, -1]]
    y = torch.zeros(1, 2, 2 * len(cells), 1)
    for j, (a, b, c, d) in enumerate(cells):
        y[0, 0, 2 * j, 0], y[0, 0, 2 * j + 1, 0], y[0, 1, 2 * j, 0], y[0, 1, 2 * j + 1, 0] = a, b, c, d
    torch.manual_seed(0)
    y = torch.cat([y.expand(1, 2, -1, 3), torch.randint(-2, 3, (1, 6, 2 * len(cells), 3)).float()], 1)
    # each situation occurs in what the encoder is given (read back from y, not from the list above)
    v = torch.stack([y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]])
    mx = v.max(0).values
    nmax = (v == mx).sum(0)
    first = (v == mx).int().argmax(0)
    assert bool(((v == 0).all(0)).any()), "an all-zero cell"
    assert bool(((mx > 0) & (nmax > 1) & (first == 0)).any()), "a positive tie led by position 0"
    assert bool(((mx > 0) & (nmax > 1) & (first > 0)).any()), "a positive tie led by a later position"
    for q in range(4):
        assert bool(((nmax == 1) & (first == q)).any()), "a single maximum in position {}".format(q)
    assert bool(((mx < 0) & (nmax > 1)).any()), "a negative tie"
    want = _mask_loop(y)
    assert torch.equal(R.pool_mask_encode(y), want)
    assert int(want.max()) <= 7
    assert not torch.equal(R.pool_mask_encode(y, last=True), want)          # the mutant's rule differs here


# ---- the comparison has teeth

def _group(case, prec, nv, large_mean=False, g=2):
    B, H, W, Hr, Cp, C, pooled, chunk = R.CASES[case]
    assert K.bn_chunk_px(H, W, Cp) == chunk
    inp = R.make_inputs(case, prec, large_mean=large_mean)
    args = (inp["z"][g, ..., :C], inp["gamma"][g, :C], inp["beta"][g, :C], inp["run"][:, g, :C], nv, Hr, Hr,
            R.EPS, R.MOMENTUM)
    kw = {"gy": inp["gy"][g, ..., :C], "pool": pooled}
    return args, kw, chunk


def _check(case, prec, nv, mutant, large_mean=False):
    args, kw, chunk = _group(case, prec, nv, large_mean)
    ref = R.bn_oracle(*args, **kw)
    got = R.bn_emulate_fp32(*args, chunk, prec=prec, mutant=mutant, **kw)
    if "pool_mask" in got:                           # as the GPU test: the encoder on the y under test
        ref = dict(ref, pool_mask=R.pool_mask_encode(got["y"]))
    rows = []
    try:
        return R.bn_compare(got, ref, prec, rows)
    finally:
        for q, err, e_t, bound in rows:
            print("[bn-emu] case {}{} prec {} nv {} {:8s} {:>15s} err {:.2e}  torch-fp32 {:.2e}  bound {:.2e}"
                  .format(case, "+100" if large_mean else "", prec, nv, q, str(mutant), err, e_t, bound))


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_emulation_passes_every_case(case, prec):
    B = R.CASES[case][0]
    for nv in (B, 1):
        errs = _check(case, prec, nv, None)
        assert set(errs) >= set(R.FP32_STORED) | {"y", "dz"}
    if case == "a":
        _check(case, prec, B, None, large_mean=True)


def test_inputs_hold_the_situations_the_cases_are_for():
    for case, (B, H, W, Hr, Cp, C, pooled, chunk) in R.CASES.items():
        for prec in (1, 0):
            inp = R.make_inputs(case, prec)
            z = inp["z"]
            if not Hr:
                assert float(z[..., C:].abs().max() if Cp > C else 0.0) == 0.0     # padding channels
            else:
                junk = 1e3 if prec else 256.0
                assert bool((z[:, :, Hr:] == junk).all()) and bool((z[:, :, :, Hr:] == junk).all())
                assert float(z[:, :, :Hr, :Hr, C:].abs().max() if Cp > C else 0.0) == 0.0
            if pooled:
                args, kw, _ = _group(case, prec, B)
                ref = R.bn_oracle(*args, **kw)
                hr = (Hr or H) // 2
                mk, py = ref["pool_mask"][:, :hr, :hr], ref["pool_y"][:, :hr, :hr]
                yy = ref["y"]
                v = torch.stack([yy[:, 0::2, 0::2], yy[:, 0::2, 1::2], yy[:, 1::2, 0::2], yy[:, 1::2, 1::2]])
                ties = ((v == v.max(0).values).sum(0) > 1)[:, :hr, :hr]
                assert bool((ties & (py > 0)).any()), "a positive tie inside the extent"
                assert bool((mk[..., 0::4] == 0).all()) and bool((py[..., 0::4] == 0).all())   # the beta = -10 channels
                assert {int(b) for b in mk.unique()} >= {0, 4, 5, 6, 7}


MUTANT_CASES = [
    # count mutants: the padded small-N cases (N = 196 at nv = 1)
    ("count_hw", "a", 1, False), ("count_hw", "c", 1, False), ("count_hw", "a", None, False),
    ("count_hw", "b", None, False), ("count_hw", "d", None, False),
    ("count_plus_row", "a", 1, False), ("count_plus_row", "c", 1, False), ("count_plus_row", "a", None, False),
    ("count_plus_row", "d", None, False),
    ("pads_in_sums", "a", None, False), ("pads_in_sums", "d", 1, False),
    # a partial last chunk: 256 of 512, 76 of 256 and 19 of 128 pixels
    ("drop_last_chunk", "a", None, False), ("drop_last_chunk", "f", None, False),
    ("drop_last_chunk", "g", None, False),
    ("no_shift", "a", None, True),
    ("last_max", "a", None, False), ("last_max", "e", 1, False),
    ("rows_B", "a", 1, False), ("rows_B", "g", 1, False),
]


@pytest.mark.parametrize("mutant,case,nv,large_mean", MUTANT_CASES)
def test_every_mutant_is_caught(mutant, case, nv, large_mean):
    nv = nv or R.CASES[case][0]
    precs = (1,) if mutant == "no_shift" else (1, 0)     # bf16 inputs near 100 sum exactly in fp32: no cancellation
    for prec in precs:
        _check(case, prec, nv, None, large_mean)          # the faithful transcription passes the same case
        with pytest.raises(AssertionError):
            _check(case, prec, nv, mutant, large_mean)


def test_every_mutant_has_a_case():
    assert {m for m, _, _, _ in MUTANT_CASES} == set(R.MUTANTS)
