"""Plain loop oracle of mixup / cutmix training (TrainConfig.mix), independent of the executors.

Python integers for the draw, explicit loops over rows, pixels and classes, numpy fp32 scalars for the three
roundings of a blend. The definition is that of gentun_amd/models/cnn_engine.py ("The mixed step"):

    r_k = hash4(key, step, 0, 0xA0610000 + k)
    applied  nv >= 2 and (r_0 >> 8) < P24;  o = 1 + r_1 % (nv - 1);  p(b) = (b + o) % nv
    m        the alpha-th smallest of r_{16+j} >> 8, j = 0 .. 2 alpha - 2
    mixup    lam = m 2^-24, lam1 = (2^24 - m) 2^-24;  M[b] = fp32(lam A[b]) + fp32(lam1 A[p(b)])
    cutmix   a box around (r_2 % Hr, r_3 % Wr) with sides isqrt((H H (2^24 - m)) >> 24) is taken from A[p(b)];
             lam = fp32(Hr Wr - area) * inv_hw, lam1 = fp32(area) * inv_hw
    target   t = fp32(lam t_b) + fp32(lam1 t_p)
"""

import math

import numpy as np

from augment_ref import augment_batch, hash4, key_of

CTR = 0xA0610000
ONE24 = 1 << 24


def p24_of(prob):
    return int(round(prob * ONE24))


def box_of(cy, cx, m, hr, wr):
    bh = math.isqrt((hr * hr * (ONE24 - m)) >> 24)
    bw = math.isqrt((wr * wr * (ONE24 - m)) >> 24)
    ty, tx = cy - bh // 2, cx - bw // 2
    return max(ty, 0), min(ty + bh, hr), max(tx, 0), min(tx + bw, wr)


def weights_of(kind, m, box, hr, wr):
    if kind == "mixup":
        return np.float32(m / ONE24), np.float32((ONE24 - m) / ONE24)           # exact: 24-bit integers
    area = (box[1] - box[0]) * (box[3] - box[2])
    inv_hw = np.float32(1.0) / np.float32(hr * wr)
    return np.float32(hr * wr - area) * inv_hw, np.float32(area) * inv_hw


def draw(key, step, nv, alpha, p24, hr, wr):
    """``None`` when the step is not mixed, else ``{"o", "m", "box", "unclipped"}`` (Python integers; the last
    is the box before it is clipped to the image)."""
    r = [hash4(key, step, 0, CTR + k) for k in range(4)]
    if nv < 2 or (r[0] >> 8) >= p24:
        return None
    u = sorted(hash4(key, step, 0, CTR + 16 + j) >> 8 for j in range(2 * alpha - 1))
    m = u[alpha - 1]
    bh, bw = math.isqrt((hr * hr * (ONE24 - m)) >> 24), math.isqrt((wr * wr * (ONE24 - m)) >> 24)
    return {"o": 1 + r[1] % (nv - 1), "m": m, "box": box_of(r[2] % hr, r[3] % wr, m, hr, wr),
            "unclipped": (r[2] % hr - bh // 2, r[2] % hr - bh // 2 + bh, r[3] % wr - bw // 2, r[3] % wr - bw // 2 + bw)}


def blend(lam, a, lam1, b):
    """fp32(lam a) + fp32(lam1 b) on fp32 arrays, every operation rounded to fp32."""
    return (np.float32(lam) * a.astype(np.float32) + np.float32(lam1) * b.astype(np.float32)).astype(np.float32)


def mix_batch(A, targets, nv, seeds, fold_ids, step, kind, alpha, p24, real_hw):
    """``(M, T)``: the stored-layout batch ``A [G][B][Hp][Wp][Cp]`` (fp32 values) and its target rows
    ``targets [G][B][C]`` (fp32) under the mix of global step ``step``; ``nv [G]``: real rows per group."""
    hr, wr = real_hw
    M, T = A.copy(), np.asarray(targets, np.float32).copy()
    G, B = A.shape[:2]
    for g in range(G):
        d = draw(key_of(int(seeds[g]), int(fold_ids[g])), int(step), int(nv[g]), alpha, p24, hr, wr)
        if d is None:
            continue
        lam, lam1 = weights_of(kind, d["m"], d["box"], hr, wr)
        y0, y1, x0, x1 = d["box"]
        for b in range(int(nv[g])):
            p = (b + d["o"]) % int(nv[g])
            if kind == "mixup":
                M[g, b] = blend(lam, A[g, b], lam1, A[g, p])
            else:
                for i in range(y0, y1):
                    for j in range(x0, x1):
                        M[g, b, i, j] = A[g, p, i, j]
            for c in range(T.shape[2]):
                T[g, b, c] = np.float32(lam * np.float32(targets[g][b][c])) + \
                    np.float32(lam1 * np.float32(targets[g][p][c]))
    return M, T


def mixed_step(data, ids, targets, nv, seeds, fold_ids, step, mix, aug, real_hw, stored_hw=None, stored_c=None):
    """The batch the first conv reads and its target rows: augmentation (``aug`` None: the gathered rows), then
    the mix. ``data`` NHWC fp32; ``ids [G][B]`` sample ids; ``targets [G][B][C]`` the rows' own targets."""
    a = aug or {"shift": 0, "flip": False}
    A = augment_batch(data, ids, seeds, fold_ids, step, a["shift"], a["flip"], real_hw, stored_hw, stored_c)
    return mix_batch(A, targets, nv, seeds, fold_ids, step, mix["kind"], mix["alpha"], p24_of(mix["prob"]), real_hw)
