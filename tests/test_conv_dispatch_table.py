"""The shape tables of the specialised conv / wgrad kernels (csrc/hip/cnn_conv_fast.hip, cnn_conv_fast_ext.hip).

``tests/data/conv_dispatch_golden.json`` records, for every argument set of the grid below and every switch
setting, the instantiation, grid, block and LDS bytes the statement-macro dispatcher launched before the tables
replaced it (recorded with ``profiles/dispatch_golden_parent.patch``). The CPU tests assert that
``gt_conv_fast_select`` / ``gt_wgrad_fast_select`` return exactly that choice, and no match for every other
argument set. The GPU test launches every distinct instantiation once and compares with the fp64 oracle."""

import ctypes as C
import itertools
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from test_hip_fp32 import DEV, TOL, K, _split, nhwc_pad, pack_w, rel, report, stream

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "conv_dispatch_golden.json")

KS = (3, 5)
CHANNELS = (8, 24, 32, 56, 64, 104, 128, 256)
IMAGES = ((32, 32), (16, 16), (8, 8), (12, 16))
LAUNCHES = ((1, 32), (2, 32), (5, 32), (25, 32), (80, 32), (2, 8))       # (ngroups, B)
PACKS = {24: 20, 56: 50, 104: 100}      # padded -> the search-space channel count whose last co tile packs

# switch settings: the defaults, then each switch flipped singly (for the rows that matched)
CONV_CONFIGS = [None, ("gt_conv_set_regepi", 0), ("gt_conv_set_smallq", 0), ("gt_conv_set_s2in_ct1", 0)]
WGRAD_CONFIGS = [None, ("gt_wgrad_set_nb", 1), ("gt_wgrad_set_nb", 2), ("gt_wgrad_set_nz", 1), ("gt_wgrad_set_nz", 2),
                 ("gt_wgrad_set_nz", 4), ("gt_wgrad_set_nz", 8)]
CONV_SEL, WGRAD_SEL = 20, 16            # ints of ConvSel / WgradSel


def conv_grid():
    """(k, cinp, coutp, H, W, prec, ngroups, B, cout_real, epi_bf16)"""
    for k, cinp, coutp, (H, W), prec, (ng, B) in itertools.product(KS, CHANNELS, CHANNELS, IMAGES, (0, 1), LAUNCHES):
        for cr in [0, coutp] + ([PACKS[coutp]] if coutp in PACKS else []):
            for epi in (0, 1):
                yield (k, cinp, coutp, H, W, prec, ng, B, cr, epi)


def wgrad_grid(Km):
    """(k, cinp, coutp, H, W, prec, ngroups, B, cout_real, pps, S): the split of wgrad_split, and for the
    specialised shapes one pps that is not a whole number of bands"""
    for k, cinp, coutp, (H, W), prec, (ng, B) in itertools.product(KS, CHANNELS, CHANNELS, IMAGES, (0, 1), LAUNCHES):
        band = Km.wgrad_band(k, k, cinp, coutp, H, W, prec)
        npix = B * H * W
        splits = [Km.wgrad_split(npix, k * k * cinp, coutp, band=band)]
        if band[0]:
            pps = splits[0][0] + band[0] // 2
            splits.append((pps, -(-npix // pps)))
        for cr in [0, coutp] + ([PACKS[coutp]] if coutp in PACKS else []):
            for pps, S in splits:
                yield (k, cinp, coutp, H, W, prec, ng, B, cr, pps, S)


def conv_args(Km, t):
    k, cinp, coutp, H, W, prec, ng, B, cr, epi = t
    a = Km.ConvArgs()
    a.KH, a.KW, a.Cinp, a.Coutp, a.H, a.W = k, k, cinp, coutp, H, W
    a.G = a.ngroups = ng
    a.B, a.prec, a.cout_real, a.epi_bf16 = B, prec, cr, epi
    a.TH = Km.conv_tile_rows(H, W)
    return a


def wgrad_args(Km, t):
    k, cinp, coutp, H, W, prec, ng, B, cr, pps, S = t
    a = Km.WgradArgs()
    a.KH, a.KW, a.Cinp, a.Coutp, a.H, a.W = k, k, cinp, coutp, H, W
    a.G = a.ngroups = ng
    a.B, a.prec, a.cout_real, a.pps, a.S = B, prec, cr, pps, S
    return a


def select(L, fn, a, n):
    """the n ints of the select entry's struct, or None for no match"""
    out = (C.c_int * n)()
    entry = getattr(L, fn)
    return list(out) if entry(C.byref(a), C.cast(out, entry.argtypes[1])) else None


class switched(object):
    """one switch set for the block, the old value put back after it"""

    def __init__(self, L, cfg):
        self.L, self.cfg = L, cfg

    def __enter__(self):
        if self.cfg:
            self.old = getattr(self.L, self.cfg[0])(self.cfg[1])

    def __exit__(self, *exc):
        if self.cfg:
            getattr(self.L, self.cfg[0])(self.old)
        return False


def record(L, grid, make_args, fn, n, configs):
    """{"tried", "configs", "choices", "rows"}: rows = matching argument sets + one index into `choices`
    per switch setting (-1: no match under that setting)"""
    grid = list(grid)
    choices, rows = {}, []
    matched = [t for t in grid if select(L, fn, make_args(t), n) is not None]
    cols = []
    for cfg in configs:
        with switched(L, cfg):
            col = []
            for t in matched:
                s = select(L, fn, make_args(t), n)
                col.append(-1 if s is None else choices.setdefault(tuple(s), len(choices)))
            cols.append(col)
    for i, t in enumerate(matched):
        rows.append(list(t) + [col[i] for col in cols])
    return {"tried": len(grid), "configs": [list(c) if c else None for c in configs],
            "choices": [list(c) for c in sorted(choices, key=choices.get)], "rows": rows}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _check(L, gold, grid, nargs, make_args, fn, n, configs, extra):
    assert gold["configs"] == [list(c) if c else None for c in configs]
    stored = {tuple(r[:nargs]): r[nargs:] for r in gold["rows"]}
    grid = list(grid)
    assert len(grid) == gold["tried"] and len(set(grid)) == len(grid)
    assert set(stored) <= set(grid)
    checked = 0
    for ci, cfg in enumerate(configs):
        with switched(L, cfg):
            for t in (grid if cfg is None else stored):
                a = make_args(t)
                got = select(L, fn, a, n)
                idx = stored[t][ci] if t in stored else -1
                assert got == (gold["choices"][idx] if idx >= 0 else None), (t, cfg)
                extra(a, t, got)
                checked += 1
    return checked


def test_conv_select_matches_golden(golden):
    """gt_conv_fast_select returns the recorded instantiation / grid / block / LDS for every stored row under
    every switch setting, no match for the rest of the grid; the two probes agree with the selection."""
    Km = K()
    L = Km.lib()

    def probes(a, t, got):
        th = got[4] if got else 0
        assert L.gt_conv_fast_probe_any(a) == (1 if got else 0), t
        assert L.gt_conv_fast_probe(a) == (th if th % 2 == 0 else 0), t

    n = _check(L, golden["conv"], conv_grid(), 10, lambda t: conv_args(Km, t), "gt_conv_fast_select", CONV_SEL,
               CONV_CONFIGS, probes)
    print("[dispatch] conv: {} selections checked, {} matching rows, {} distinct choices".format(
        n, len(golden["conv"]["rows"]), len(golden["conv"]["choices"])))


def test_wgrad_select_matches_golden(golden):
    """The same for gt_wgrad_fast_select; gt_wgrad_fast_band is the selected row's R * W."""
    Km = K()
    L = Km.lib()

    def band(a, t, got):
        if got:
            assert L.gt_wgrad_fast_band(a.KH, a.KW, a.Cinp, a.Coutp, a.H, a.W, a.prec) == got[5] * got[4], t

    n = _check(L, golden["wgrad"], wgrad_grid(Km), 11, lambda t: wgrad_args(Km, t), "gt_wgrad_fast_select",
               WGRAD_SEL, WGRAD_CONFIGS, band)
    print("[dispatch] wgrad: {} selections checked, {} matching rows, {} distinct choices".format(
        n, len(golden["wgrad"]["rows"]), len(golden["wgrad"]["choices"])))


def test_select_struct_mirrors():
    """ConvSel / WgradSel of cnn_kernels.py name the ints the entry points fill."""
    Km = K()
    L = Km.lib()
    s = Km.ConvSel()
    assert L.gt_conv_fast_select(C.byref(conv_args(Km, (5, 8, 24, 32, 32, 1, 25, 32, 20, 1))), C.byref(s))
    assert (s.KH, s.KW, s.NCBI, s.W, s.TH, s.NT, s.NCO, s.NWV, s.PREC, s.PK, s.RE, s.CTX, s.SCH) == \
        (5, 5, 1, 32, 8, 2, 3, 4, 1, 1, 1, 0, 0)
    assert (s.gx, s.gy, s.gz, s.block) == (32 * 4, 25, 1, 256) and s.lds == s.lds_fwd
    w = Km.WgradSel()
    pps, S = Km.wgrad_split(32 * 16 * 16, 9 * 56, 56, band=Km.wgrad_band(3, 3, 56, 56, 16, 16, 0))
    assert L.gt_wgrad_fast_select(C.byref(wgrad_args(Km, (3, 56, 56, 16, 16, 0, 25, 32, 0, pps, S))), C.byref(w))
    assert (w.KH, w.KW, w.NCBI, w.NCBO, w.W, w.R, w.NW, w.NB, w.PK, w.NZ, w.PREC) == (3, 3, 7, 7, 16, 16, 8, 2, 0, 1, 0)
    assert (w.gx, w.gy, w.gz, w.block, w.lds) == (S, 25, 1, 512, 0)


# ---------------------------------------------------------------------------
# GPU: every distinct instantiation of the tables launched once
# ---------------------------------------------------------------------------
G_SMALL = 2
B_SMALL = (2, 40)      # 40: the 4-row tiles of shapes that go down to 2 rows need 300 <= workgroups < 600


def _real(cp):
    return 3 if cp == 8 else PACKS.get(cp, cp)


def _data(shape, prec, scale=1.0):
    """fp32: normal values. bf16: sparse small integers, on which bf16 products, fp32 sums and the bf16 stores
    of the outputs are all exact -- so the fp32 tolerance holds for the bf16 kernels as well."""
    if prec == 1:
        return torch.randn(shape) * scale
    return torch.randint(-1, 2, shape).float() * (torch.rand(shape) < 0.1)


def _steer(L, setters, wanted, nkey, fn, n, candidates):
    """the first (switch values, arguments) for which the select entry returns descriptor `wanted`"""
    for vals in itertools.product(*[v for _, v in setters]):
        old = [getattr(L, s)(v) for (s, _), v in zip(setters, vals)]
        try:
            for a in candidates():
                got = select(L, fn, a, n)
                if got is not None and got[:nkey] == wanted:
                    return vals, a
        finally:
            for (s, _), o in zip(setters, old):
                getattr(L, s)(o)
    return None, None


def _images(gold, nkey, desc, hpos):
    """image heights of the golden rows that chose this descriptor"""
    idx = {i for i, c in enumerate(gold["choices"]) if c[:nkey] == desc}
    return sorted({r[hpos] for r in gold["rows"] if idx & set(r[len(r) - len(gold["configs"]):])})


@pytest.mark.gpu
def test_every_table_kernel_against_fp64(golden):
    """Each distinct conv / wgrad instantiation of the golden file: the smallest arguments that select it
    (2 groups, batch 2, steered by the switches; batch 40 for the 4-row tiles that only a grid of 300-599
    workgroups selects, batch 4 where a wgrad split needs it for whole 64-pixel k-steps), checked with the select
    entry, launched once, compared with the fp64 conv2d / weight-gradient oracle at the tolerance of
    test_hip_fp32.py."""
    Km = K()
    L = Km.lib()
    torch.manual_seed(20)
    G = G_SMALL
    conv_set = [("gt_conv_set_smallq", (1, 0)), ("gt_conv_set_regepi", (1, 0)), ("gt_conv_set_s2in_ct1", (1, 0))]
    descs = sorted({tuple(c[:15]) for c in golden["conv"]["choices"]})
    for d in descs:
        d = list(d)
        KH, KW, NCBI, W, TH, NT, NCO, NWV, PREC, PK = d[:10]
        cinp, coutp = NCBI * 8, NCO * 8
        cin, cout = _real(cinp), _real(coutp)
        H = _images(golden["conv"], 15, d, 3)[0]
        vals, a = _steer(L, conv_set, d, 15, "gt_conv_fast_select", CONV_SEL, lambda: [
            conv_args(Km, (KH, cinp, coutp, H, W, PREC, G, B, cout if PK else 0, 1)) for B in B_SMALL])
        assert a is not None, d
        B = a.B
        x = _data((G, B, cin, H, W), PREC)
        w = _data((G, cout, cin, KH, KW), PREC, 1.0 / math.sqrt(cin * KH * KW))
        b = _data((G, cout), PREC, 0.1)
        dt = torch.float32 if PREC else torch.bfloat16
        x_in = torch.stack([nhwc_pad(x[g], cinp) for g in range(G)]).to(DEV, dt).contiguous()
        wp = torch.stack([pack_w(w[g], coutp, cinp) for g in range(G)]).to(DEV)
        wpl = _split(wp).contiguous() if PREC else wp.to(dt).contiguous()
        bp = torch.zeros(G, coutp, device=DEV)
        bp[:, :cout] = b.to(DEV)
        out = torch.full((G, B, H, W, coutp), 7.0, device=DEV, dtype=dt)
        rows = torch.tensor([[g, 1, 1, 0] for g in range(G)], dtype=torch.int32, device=DEV)
        a.inp[0], a.out[0] = x_in.data_ptr(), out.data_ptr()
        a.gtab = rows.data_ptr()
        a.relu = 1
        a.w, a.bias, a.wps = wpl.data_ptr(), bp.data_ptr(), (wpl[0].numel() if PREC else 0)
        old = [getattr(L, s)(v) for (s, _), v in zip(conv_set, vals)]
        try:
            assert select(L, "gt_conv_fast_select", a, CONV_SEL)[:15] == d
            Km.check(L.gt_conv_fwd(a, stream()), "conv")
        finally:
            for (s, _), o in zip(conv_set, old):
                getattr(L, s)(o)
        torch.cuda.synchronize()
        worst = 0.0
        for g in range(G):
            ref = F.relu(F.conv2d(x[g].double(), w[g].double(), b[g].double(), padding=KH // 2))
            worst = max(worst, rel(out[g, ..., :cout].permute(0, 3, 1, 2), ref))
            assert torch.all(out[g, ..., cout:] == 0)
        report("conv_fast_kernel<{}>".format(", ".join(map(str, d[:13]))), worst, float("nan"))
        assert worst < TOL, d

    wgrad_set = [("gt_wgrad_set_nz", (0, 1, 2, 4, 8)), ("gt_wgrad_set_nb", (0, 1, 2))]
    descs = sorted({tuple(c[:11]) for c in golden["wgrad"]["choices"]})
    for d in descs:
        d = list(d)
        KH, KW, NCBI, NCBO, W, R, NW, NB, PK, NZ, PREC = d
        cinp, coutp = NCBI * 8, NCBO * 8
        cin, cout = _real(cinp), _real(coutp)
        H = _images(golden["wgrad"], 11, d, 3)[0]
        band = Km.wgrad_band(KH, KW, cinp, coutp, H, W, PREC)
        for B in (2, 4, 8):        # gt_conv_wgrad wants splits of whole 64-pixel k-steps (8 x 8 images: batch 4)
            pps, S = Km.wgrad_split(B * H * W, KH * KW * cinp, coutp, band=band)
            if pps % 64 == 0:
                break
        vals, a = _steer(L, wgrad_set, d, 11, "gt_wgrad_fast_select", WGRAD_SEL, lambda: [
            wgrad_args(Km, (KH, cinp, coutp, H, W, PREC, G, B, cout if PK else 0, pps, S))])
        assert a is not None, d
        x = _data((G, B, cin, H, W), PREC)
        dz = _data((G, B, cout, H, W), PREC) * (torch.rand(G, B, cout, H, W) > 0.4)
        ref = torch.stack([torch.nn.grad.conv2d_weight(x[g].double(), (cout, cin, KH, KW), dz[g].double(),
                                                       padding=KH // 2) for g in range(G)])
        refb = dz.double().sum((1, 3, 4))
        dt = torch.float32 if PREC else torch.bfloat16
        x_in = torch.stack([nhwc_pad(x[g], cinp) for g in range(G)]).to(DEV, dt).contiguous()
        dz_p = torch.stack([nhwc_pad(dz[g], coutp) for g in range(G)]).to(DEV, dt).contiguous()
        Kdim = KH * KW * cinp
        pw = torch.zeros(S, G, coutp, Kdim, device=DEV)
        pb = torch.zeros(S, G, coutp, device=DEV)
        st = torch.zeros(8, dtype=torch.int32, device=DEV)
        rows = torch.tensor([[g, 1, 0, 0] for g in range(G)], dtype=torch.int32, device=DEV)
        a.inp[0], a.gtab, a.st = x_in.data_ptr(), rows.data_ptr(), st.data_ptr()
        a.dz, a.part_w, a.part_b = dz_p.data_ptr(), pw.data_ptr(), pb.data_ptr()
        old = [getattr(L, s)(v) for (s, _), v in zip(wgrad_set, vals)]
        try:
            assert select(L, "gt_wgrad_fast_select", a, WGRAD_SEL)[:11] == d
            Km.check(L.gt_conv_wgrad(a, stream()), "wgrad")
        finally:
            for (s, _), o in zip(wgrad_set, old):
                getattr(L, s)(o)
        torch.cuda.synchronize()
        got = pw.sum(0).view(G, coutp, KH, KW, cinp)[:, :cout, :, :, :cin].permute(0, 1, 4, 2, 3)
        ew, eb = rel(got, ref), rel(pb.sum(0)[:, :cout], refb)
        report("wgrad kernel<{}>".format(", ".join(map(str, d))), max(ew, eb), float("nan"))
        assert ew < TOL and eb < TOL, d
