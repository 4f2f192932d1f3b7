"""``embed`` / ``neighbors`` on an MI355X: the kernels of csrc/hip/cnn_neighbors.hip alone on hand-made buffers
against an fp64 product, then through the HIP predictors of the fits of tests/test_cnn_fitted_gpu.py and
tests/test_cnn_ensemble_gpu.py (shared inside one pytest process, left unchanged).

The bound of a distance over ``D`` real features, ``EPS = 2^-24`` (the project's split-fp32 bound):
* l2:      ``(D + 4) * EPS * (|q|^2 + |b|^2 + 2 sum_i |q_i b_i|)``
* cosine:  ``(D + 4) * EPS * (sum_i |q_i b_i| + |q.b|) / (|q| |b|) + 4 * EPS`` -- the dot product's accumulation over
  the exact denominator, the two norms' (each ``(D + 4) * EPS`` relative, halved by the root) times ``|cos|``, and
  the roundings of the two roots, their product, the quotient and the difference from 1, all of values <= 1."""

import numpy as np
import pytest
import torch

import neighbors_ref as R
import test_cnn_ensemble_gpu as E
import test_cnn_fitted_gpu as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GUARD, HB = 256, 64          # elements past an output (all keep their fill); rows of the hidden buffer
DEV = "cuda:0"


def reference(q, b, metric, D):
    """fp64 ``(distance, bound)`` ``[m, N]`` of feature rows ``q``, ``b`` holding ``D`` real features."""
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    dot, ab = q @ b.T, np.abs(q) @ np.abs(b).T
    qq, bb = (q * q).sum(1)[:, None], (b * b).sum(1)[None, :]
    if metric == "l2":
        return np.maximum(qq + bb - 2.0 * dot, 0.0), (D + 4) * EPS * (qq + bb + 2.0 * ab)
    den = np.sqrt(qq) * np.sqrt(bb)
    safe = np.where(den > 0, den, 1.0)
    return np.where(den > 0, 1.0 - dot / safe, 1.0), (D + 4) * EPS * (ab + np.abs(dot)) / safe + 4 * EPS


def separated(d, bound, k):
    """``(order [m, N], ok [m, k])``: ``ok[i, r]`` when the reference distance of rank ``r`` is more than twice the
    bound from both its neighbours in the order (among the first ``k + 1``)."""
    order = np.argsort(d, axis=1, kind="stable")
    ds, bs = np.take_along_axis(d, order, 1), np.take_along_axis(bound, order, 1)
    far, n = np.ones((len(d), k + 1), bool), min(k + 1, d.shape[1])
    far[:, 1:n] = ds[:, 1:n] - ds[:, :n - 1] > 2 * np.maximum(bs[:, 1:n], bs[:, :n - 1])
    return order, far[:, :k] & far[:, 1:]


def check(tag, idx, dist, d, bound, order, ok):
    """Every distance within the bound of the fp64 one of the row returned; the reference's index where ``ok``."""
    idx = idx.astype(np.int64)
    ratio = np.abs(dist - np.take_along_axis(d, idx, 1)) / np.take_along_axis(bound, idx, 1)
    print("[cnn-neighbors] {}: worst error / bound {:.3f}, (query, rank) pairs closer than twice the bound: {} of {}"
          .format(tag, float(ratio.max()), int((~ok).sum()), ok.size))
    assert ratio.max() <= 1.0 and (idx == order[:, :idx.shape[1]])[ok].all()


def features(Ur, G, m, N, seed, bf16):
    """Queries ``[G, m, Ur]`` and bank ``[N, G, Ur]``, non-negative with half the units zero like hidden rows: a
    query is one row ``w`` at its own scale, bank row ``j`` is ``w`` plus a row on ``w``'s zero units of squared
    norm ``g_j |w|^2``, the ``g_j`` a shuffled grid; every unit jitters by 0.5 %, so no two dot products agree."""
    rng = np.random.default_rng(seed)
    w = np.maximum(rng.standard_normal(G * Ur), 0)
    q = (0.8 + 0.45 * rng.random((m, 1))) * w * (1 + 0.005 * rng.uniform(-1, 1, (m, G * Ur)))
    e = rng.random((N, G * Ur)) * (w == 0)
    e *= np.sqrt((0.05 + 0.02 * rng.permutation(N)) * (w * w).sum() / (e * e).sum(1))[:, None]
    b = w * (1 + 0.005 * rng.uniform(-1, 1, (N, G * Ur))) + e
    q = np.ascontiguousarray(q.reshape(m, G, Ur).transpose(1, 0, 2)).astype(np.float32)
    b = b.reshape(N, G, Ur).astype(np.float32)
    if bf16:
        q, b = (torch.from_numpy(t).bfloat16().float().numpy() for t in (q, b))
    return q, b


class _Nn(object):
    """A hidden buffer ``[G][HB][Up]`` (NaN in padded units and rows ``>= m``), a bank built by ``gt_nn_bank`` in
    two launches from ``[G][N][Up]`` activations or (``flat``) fp32 ``[N][ld]``, NaN-filled outputs with guards."""

    def __init__(self, q, b, Up, dtype, flat=False):
        from gentun_amd.ops import cnn_kernels as K
        self.K, self.L = K, K.lib()
        (G, m, Ur), N = q.shape, b.shape[0]
        self.dims, self.N, self.prec, self.Np = (G, m, Ur, Up), N, int(dtype == torch.float32), -(-N // 128) * 128
        hid = np.full((G, HB, Up), np.nan, np.float32)
        hid[:, :m, :Ur] = q
        self.hid = torch.from_numpy(hid).to(device=DEV, dtype=dtype)
        self.planes = torch.full((3 if self.prec else 1, self.Np, G * Up), np.nan, dtype=torch.bfloat16, device=DEV)
        self.norm = torch.full((self.Np,), np.nan, device=DEV)
        ld = -(-G * Ur // 32) * 32 + 32
        src = np.full((N, ld) if flat else (G, N, Up), np.nan, np.float32)
        if flat:
            src[:, :G * Ur] = b.reshape(N, G * Ur)
        else:
            src[:, :, :Ur] = b.transpose(1, 0, 2)
        self.src = torch.from_numpy(src).to(device=DEV, dtype=torch.float32 if flat else dtype)
        a = K.NnBankArgs()
        a.planes, a.norm, a.prec, a.N, a.Np = self.planes.data_ptr(), self.norm.data_ptr(), self.prec, N, self.Np
        s, a.sprec = a.src, 1 if flat else self.prec
        s.G, s.B, s.Up, s.Ur, s.flat, s.ld = G, N, Up, Ur, int(flat), ld if flat else 0
        row = self.src.element_size() * (ld if flat else Up)
        for n0, rows in ((0, N // 2), (N // 2, N - N // 2)):
            if rows:
                s.h, a.n0, a.m, a.rows = self.src.data_ptr() + n0 * row, n0, rows, (self.Np - n0 if n0 + rows == N else rows)
                assert self.L.gt_nn_bank(a, None) == 0

    def args(self, k, S, metric):
        G, m, Ur, Up = self.dims
        self.out = [torch.full((HB * S * k + GUARD,), np.nan, device=DEV),
                    torch.full((HB * S * k + GUARD,), -7, dtype=torch.int32, device=DEV),
                    torch.full((HB * k + GUARD,), np.nan, device=DEV),
                    torch.full((HB * k + GUARD,), -7, dtype=torch.int32, device=DEV)]
        t, g = self.K.NnTopkArgs(), self.K.NnMergeArgs()
        q = t.q
        q.h, q.G, q.B, q.Up, q.Ur = self.hid.data_ptr(), G, HB, Up, Ur
        t.planes, t.bnorm, t.cand_d, t.cand_i = [v.data_ptr() for v in [self.planes, self.norm] + self.out[:2]]
        t.prec, t.m, t.N, t.Np, t.k, t.S, t.metric = self.prec, m, self.N, self.Np, k, S, ("l2", "cosine").index(metric)
        g.cand_d, g.cand_i, g.out_d, g.out_i = [v.data_ptr() for v in self.out]
        g.m, g.S, g.k = m, S, k
        return t, g

    def search(self, k, S, metric):
        """``(index [m, k], distance [m, k])``; everything past row ``m`` must have kept its fill."""
        t, g = self.args(k, S, metric)
        assert self.L.gt_nn_topk(t, None) == 0 and self.L.gt_nn_merge(g, None) == 0
        m = self.dims[1]
        for buf, n in zip(self.out, (m * S * k, m * S * k, m * k, m * k)):
            assert (buf[n:] == -7).all() if buf.dtype == torch.int32 else torch.isnan(buf[n:]).all()
        return self.out[3][:m * k].view(m, k).cpu().numpy(), self.out[2][:m * k].view(m, k).cpu().numpy()


# (real units, Up, G, m, N, S, k, metric, dtype, flat bank): every value the issue names -- one k-step and sixteen,
# one bank tile and three, a tile edge on either side, fewer bank rows than k, slices with no tile
KERNEL = [
    (20, 32, 1, 1, 1, 1, 1, "l2", torch.float32, True),
    (20, 32, 1, 33, 127, 1, 5, "cosine", torch.float32, False),
    (20, 32, 3, 33, 129, 3, 16, "l2", torch.float32, True),
    (20, 32, 1, 33, 300, 3, 16, "cosine", torch.bfloat16, False),
    (20, 32, 3, 1, 300, 1, 5, "cosine", torch.float32, False),
    (500, 512, 1, 33, 300, 3, 16, "l2", torch.float32, False),
    (500, 512, 3, 33, 129, 1, 5, "l2", torch.float32, True),
    (500, 512, 1, 1, 127, 3, 1, "cosine", torch.float32, True),
    (500, 512, 3, 33, 300, 3, 5, "l2", torch.bfloat16, False),
    (500, 512, 1, 33, 129, 1, 16, "cosine", torch.bfloat16, False),
]


@pytest.mark.parametrize("case", KERNEL, ids=lambda c: "-".join(str(v).replace("torch.", "") for v in c))
def test_kernels_against_the_fp64_product(case):
    """The inputs' first k + 1 reference distances are more than twice the bound apart (asserted; seed 0 checked on
    the CPU), so the indices must be the reference's."""
    Ur, Up, G, m, N, S, k, metric, dtype, flat = case
    q, b = features(Ur, G, m, N, 0, dtype == torch.bfloat16)
    d, bound = reference(q.transpose(1, 0, 2).reshape(m, G * Ur), b.reshape(N, G * Ur), metric, G * Ur)
    order, ok = separated(d, bound, min(k, N))
    assert ok.all(), "the seed does not separate the reference distances"
    check("kernel {}".format(case), *_Nn(q, b, Up, dtype, flat).search(min(k, N), S, metric), d, bound, order, ok)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_position_independence_and_duplicates(metric, dtype):
    """Query row 33 repeats row 0; bank rows 130 and 290 (other tiles, other slices of three) repeat row 5, which
    query 1 equals. One slice and three give the same bytes, row 33's results are row 0's, and wherever the
    repeated bank row is returned its copies follow it at once with the same bits, in index order."""
    q, b = features(500, 2, 34, 300, 3, dtype == torch.bfloat16)
    q[:, 33], q[:, 1], b[130], b[290] = q[:, 0], b[5], b[5], b[5]
    nn = _Nn(q, b, 512, dtype)
    i1, d1 = nn.search(16, 1, metric)
    i3, d3 = nn.search(16, 3, metric)
    assert i1.tobytes() == i3.tobytes() and d1.tobytes() == d3.tobytes()
    assert i1[0].tobytes() == i1[33].tobytes() and d1[0].tobytes() == d1[33].tobytes()
    hits = [(ri, rd, ri.tolist().index(5)) for ri, rd in zip(i1, d1) if 5 in ri[:14]]
    assert hits and (metric != "l2" or i1[1, :3].tolist() == [5, 130, 290])
    for ri, rd, p in hits:
        assert ri[p:p + 3].tolist() == [5, 130, 290] and rd[p] == rd[p + 1] == rd[p + 2]


REFUSED = [dict(k=0), dict(k=17), dict(k=9, N=8), dict(m=0), dict(Up=48), dict(S=0), dict(S=65),
           dict(N=8000000, Np=8000000)]                     # 1.4 GiB of planes


@pytest.mark.parametrize("over", REFUSED, ids=lambda o: "-".join("{}{}".format(*kv) for kv in o.items()))
def test_launchers_refuse_and_launch_nothing(over):
    nn = _Nn(*features(20, 1, 3, 40, 0, False), 32, torch.float32)
    t, g = nn.args(5, 2, "l2")
    for name, v in over.items():
        for a in (t, g, t.q):
            if hasattr(a, name):
                setattr(a, name, v)
    assert nn.L.gt_nn_topk(t, None) != 0 and nn.L.gt_nn_bank(nn.K.NnBankArgs(), None) != 0
    assert "N" in over or "Up" in over or nn.L.gt_nn_merge(g, None) != 0
    assert all(((b == -7) if b.dtype == torch.int32 else torch.isnan(b)).all() for b in nn.out)


# through the predictors: plain ("ones"), 28 x 28 x 1 ("c3"), BatchNorm, a 3-member ensemble, a bf16 fit. The fits
# "chain" and "mnist" tell no rows apart after their one epoch (squared embedding norms of 0.006) and are not used.
NQ, BANK = 36, slice(20, 320)                # queries are chosen among all 320 rows; 300 of them are the bank


def _fitted(case):
    if case == "ens3":
        ens, x = E._fit("rgb")[:2]
        return ens, ens.members, x
    clf, x = F._fit(case)[2:4]
    return clf, [clf], x


@pytest.mark.parametrize("case", ["ones", "c3", "bn", "ens3"])
def test_embed_against_the_fp64_forward(case):
    """The criterion of test_cnn_fitted_gpu.py's logits: the HIP error, relative to the largest feature, is at
    most 4x that of the stock-torch fp32 forward on the same GPU against the same fp64 reference."""
    from gentun_amd.models.cnn_fitted import embed_torch
    obj, members, x = _fitted(case)
    xs = x[:300]
    ref = embed_torch(members, xs, torch.device("cpu"), 256, torch.float64)
    t32 = obj.embed(xs, device=DEV, backend="torch")
    h256, h32 = obj.embed(xs, device=DEV), obj.embed(xs, device=DEV, batch=32)
    assert h256.dtype == np.float32 and h256.shape == ref.shape == (300, 500 * len(members))
    e_t, e_h = F._rel(t32, ref), F._rel(h256, ref)
    print("[cnn-neighbors] {}: rel. embedding error vs fp64: HIP {:.3e}, torch fp32 (GPU) {:.3e}".format(case, e_h, e_t))
    assert h32.tobytes() == h256.tobytes() and e_h <= max(4 * e_t, F.ORACLE_FLOOR)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("case", ["ones", "c3", "bn", "ens3", "bf16"])
def test_neighbors_through_the_predictor(case, metric, monkeypatch):
    """A bank of 300 images: at batch 32 ten bank chunks (``n0 > 0``, the zero rows on the last launch only), three
    bank tiles, three slices chosen by the host and two query chunks. One epoch leaves the embeddings crowded, so the
    queries are the NQ rows of ``x`` with the fewest reference distances (fp64, on HIP's own embeddings) closer
    than twice the bound to their neighbour in the order: at most 1 (query, rank) pair in 64 is left out of the index
    comparison (asserted); every distance is held to the bound. The same bytes come from batch 256, from the bank
    embedded beforehand (uploaded in three pieces) and, on four queries, the same indices from the loop oracle."""
    from gentun_amd.models.cnn_fitted import NeighborState, nn_slices
    from gentun_amd.ops import cnn_kernels as K
    obj, members, x = _fitted(case)
    k = 3 if case == "c3" else 5                 # the three-class fit's embeddings are the most crowded
    kw = dict(k=k, metric=metric, device=DEV)
    pool = obj.embed(x, device=DEV)
    eb = pool[BANK]
    d, bound = reference(pool, eb, metric, eb.shape[1])
    order, ok = separated(d, bound, k)
    rows = np.sort(np.argsort((~ok).sum(1), kind="stable")[:NQ])
    d, bound, order, ok = d[rows], bound[rows], order[rows], ok[rows]
    assert (~ok).sum() * 64 <= ok.size and nn_slices(3, 1, 256) == 3
    idx, dist = obj.neighbors(x[rows], x[BANK], batch=32, **kw)
    assert idx.dtype == np.int64 and dist.dtype == np.float32 and idx.shape == dist.shape == (NQ, k)
    check("{} {}".format(case, metric), idx, dist, d, bound, order, ok)
    assert (R.neighbors_ref(pool[rows[:4]], eb, k, metric)[0] == idx[:4])[ok[:4]].all()
    monkeypatch.setattr(NeighborState, "FLAT_ROWS", 128)
    for other in (obj.neighbors(x[rows], x[BANK], batch=256, **kw), obj.neighbors(x[rows], eb, batch=32, **kw)):
        assert other[0].tobytes() == idx.tobytes() and other[1].tobytes() == dist.tobytes()
    monkeypatch.setattr(K, "NN_MAX_PLANE_BYTES", 1 << 18)            # the refusal that names the way out
    with pytest.raises(ValueError, match='backend="torch"'):
        obj.neighbors(x[rows], eb, **kw)


@pytest.mark.parametrize("case", ["c3", "ens3"])
def test_other_requests_are_unchanged_by_a_search(case):
    obj, members, x = _fitted(case)
    xs, m = x[:70], F._model("c3", nfold=2)[0] if case == "c3" else None
    before = (obj.predict(xs, device=DEV), obj.predict_mc(xs, samples=4, device=DEV), m and m.cross_validate())
    obj.neighbors(xs, x[70:200], k=3, device=DEV)
    after = (obj.predict(xs, device=DEV), obj.predict_mc(xs, samples=4, device=DEV), m and m.cross_validate())
    assert before[0].tobytes() == after[0].tobytes() and before[2] == after[2]
    assert all(before[1][n].tobytes() == after[1][n].tobytes() for n in before[1])
