"""Plain loop oracle of RISE (CnnClassifier.rise, csrc/hip/cnn_rise.hip), written independently of the model
code: Python integers for the hash, explicit loops over masks and pixels, numpy only for fp32 scalars.

    key_i = hash4(seed, i, 0x52495345, 0)                    s = cells, ch = ceil(H / s), cw = ceil(W / s)
    g_i(a, b) = 1 if hash4(key_i, a, b, 1) < uint32(p * 2^32) else 0
    oy = hash4(key_i, 0, 0, 2) mod ch, ox = hash4(key_i, 0, 0, 3) mod cw
    Y = y + oy, a = Y // ch, ty = fp32(Y - a * ch) / fp32(ch); X, b, tx likewise
    top = g(a, b) + tx * (g(a, b + 1) - g(a, b)); bot the same in row a + 1; M_i[y, x] = top + ty * (bot - top)
    V_i(img)[y, x, c] = fill[c] + M_i[y, x] * (img[y, x, c] - fill[c])
    map[r] = fp32(fp64(sum_i s_{r,i} M_i) * fp64(1 / (masks * p)))

every fp32 operation rounded separately."""

import numpy as np

M32 = 0xFFFFFFFF
F = np.float32


def mix32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def hash4(a, b, c, d):
    h = mix32((a ^ 0x9E3779B9) & M32)
    h = mix32(h ^ b)
    h = mix32(h ^ ((c * 0x85EBCA6B) & M32))
    return mix32(h ^ ((d * 0xC2B2AE35) & M32))


def mask(H, W, i, cells, p, seed):
    """fp32 ``[H, W]``: mask ``i``."""
    ch, cw = (H + cells - 1) // cells, (W + cells - 1) // cells
    thr = int(p * 4294967296.0)
    key = hash4(seed, i, 0x52495345, 0)

    def g(a, b):
        return F(1) if hash4(key, a, b, 1) < thr else F(0)
    oy, ox = hash4(key, 0, 0, 2) % ch, hash4(key, 0, 0, 3) % cw
    out = np.zeros((H, W), F)
    for y in range(H):
        a = (y + oy) // ch
        ty = F(y + oy - a * ch) / F(ch)
        for x in range(W):
            b = (x + ox) // cw
            tx = F(x + ox - b * cw) / F(cw)
            top = F(g(a, b) + F(tx * F(g(a, b + 1) - g(a, b))))
            bot = F(g(a + 1, b) + F(tx * F(g(a + 1, b + 1) - g(a + 1, b))))
            out[y, x] = F(top + F(ty * F(bot - top)))
    return out


_MASKS = {}


def masks(H, W, n, cells, p, seed):
    """fp32 ``[n, H, W]``, computed once per setting and shared (left unchanged) by the tests."""
    key = (H, W, n, cells, p, seed)
    if key not in _MASKS:
        _MASKS[key] = np.stack([mask(H, W, i, cells, p, seed) for i in range(n)])
    return _MASKS[key]


def view(img, M, fill, stored=None):
    """One fp32 image ``[H, W, C]`` under mask ``M`` (``None``: as it is), stored in ``stored = (Hp, Wp, Cp)``
    (zeros outside the real extent and in the channel padding)."""
    H, W, C = img.shape
    out = np.zeros(stored or img.shape, F)
    for c in range(C):
        f = F(fill[c])
        out[:H, :W, c] = img[:, :, c] if M is None else F(f) + M * (img[:, :, c] - f)
    return out


def views(x, Ms, fill):
    """``[n * len(Ms), H, W, C]``: item ``r * len(Ms) + i``."""
    f = np.broadcast_to(np.asarray(fill, F), (x.shape[3],))
    return np.stack([view(img, M, f) for img in x for M in Ms])


def accumulate(S, Ms, p):
    """fp32 ``[n, H, W]`` from scores ``S [n, masks]``: the fp64 sum in ascending ``i``, times fp64 ``inv``."""
    acc = np.zeros((S.shape[0],) + Ms.shape[1:], np.float64)
    for r in range(S.shape[0]):
        for i in range(len(Ms)):
            acc[r] += np.float64(S[r, i]) * Ms[i].astype(np.float64)
    return (acc * (1.0 / (len(Ms) * float(p)))).astype(F)
