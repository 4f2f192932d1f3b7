"""Grad-CAM references for the tests of ``gradcam()`` (gentun_amd/models/cnn_fitted.py, cnn_ensemble.py) and of
``gt_cam_w1sum`` / ``gt_head_gradcam`` (csrc/hip/cnn_dense.hip).

* :func:`oracle`: plain fp64 numpy from a classifier's exported parameters and a given last feature map ``A``,
  by the UNCOLLAPSED formula -- the full ``dS/dA`` through both dense layers, then its mean over the pixels, then
  the weighted sum of the channels. It shares no step with the code under test.
* :func:`w1sum_twin` / :func:`head_twin`: the two kernels' operations in fp32 numpy, in the kernels' orders, so
  the device results can be compared byte for byte.
* :func:`rounding_bound`: the a-priori bound of the twin's distance from the oracle on the same inputs.
"""

import numpy as np

U32 = 2.0 ** -24             # one fp32 rounding (half an ulp) relative to the value rounded


# ---------------------------------------------------------------------------------------------------------
# fp64 oracle
# ---------------------------------------------------------------------------------------------------------

def head64(params, A):
    """``(z, h, logits, proba)`` in fp64 of the last feature map ``A [n, C, hr, wr]`` (NCHW flatten, the order
    of ``dense1.w``'s rows)."""
    W1, b1 = params["dense1.w"].astype(np.float64), params["dense1.b"].astype(np.float64)
    W2, b2 = params["dense2.w"].astype(np.float64), params["dense2.b"].astype(np.float64)
    z = np.asarray(A, np.float64).reshape(len(A), -1) @ W1 + b1
    h = np.maximum(z, 0.0)
    logits = h @ W2 + b2
    e = np.exp(logits - logits.max(1, keepdims=True))
    return z, h, logits, e / e.sum(1, keepdims=True)


def score64(params, A, t, score):
    """The fp64 score ``[n]`` of class ``t[r]``: the logit or the probability."""
    _, _, logits, proba = head64(params, A)
    return (logits if score == "logit" else proba)[np.arange(len(A)), t]


def coefficients(proba, t, score):
    """``dS/dlogits [n, classes]``: one-hot for the logit, ``p[t] * ([c == t] - p[c])`` for the probability."""
    hot = (np.arange(proba.shape[1])[None, :] == np.asarray(t)[:, None]).astype(proba.dtype)
    if score == "logit":
        return hot
    return proba[np.arange(len(proba)), t][:, None] * (hot - proba)


def oracle(params, A, t, score, h=None, proba=None):
    """``(cam [n, hr, wr] without the ReLU, dS/dA [n, C, hr, wr])`` in fp64. ``h`` / ``proba`` (fp64 values of
    the hidden activations and class probabilities) replace the oracle's own where a comparison is to start from
    the same ones."""
    A = np.asarray(A, np.float64)
    W1, W2 = params["dense1.w"].astype(np.float64), params["dense2.w"].astype(np.float64)
    _, h0, _, p0 = head64(params, A)
    h = h0 if h is None else np.asarray(h, np.float64)
    proba = p0 if proba is None else np.asarray(proba, np.float64)
    dH = (h > 0) * (coefficients(proba, t, score) @ W2.T)
    dA = (dH @ W1.T).reshape(A.shape)                    # the full gradient: nothing collapsed
    alpha = dA.mean((2, 3))
    return (alpha[:, :, None, None] * A).sum(1), dA


def rounding_bound(params, A, h, proba, t, score):
    """fp64 ``[n, hr, wr]``: (roundings on the longest path from the inputs to a map element of one member of
    weight 1) * 2^-24 * (the sum of the absolute values of the terms of that element), for :func:`head_twin`
    with :func:`w1sum_twin` started from the same ``A``, ``h`` (its sign pattern) and fp32 ``proba``.

    The terms of ``cam[p]`` are ``coef[k] * W2[u, k] * W1[(c, i, j), u] * A[c, p] / (hr * wr)`` over every class,
    unit, channel and pixel; ``coef`` for the probability score has the two terms ``p[t] * [k == t]`` and
    ``p[t] * p[k]``. The path: coef (2: the subtraction and the product; 0 for the logit), its product with
    ``W2`` (1), the class sum (C - 1), wbar's pixel sum (hr * wr - 1), the product with wbar (1), the lane's sum
    (ceil(U / 64)), the xor tree (6), ``inv_n`` and the product with it (2), the product with ``A`` (1), the
    channel sum (Cr) and the member's weight (1)."""
    A = np.abs(np.asarray(A, np.float64))
    n, C, hr, wr = A.shape
    W1, W2 = np.abs(params["dense1.w"].astype(np.float64)), np.abs(params["dense2.w"].astype(np.float64))
    U, classes = W2.shape
    proba = np.asarray(proba, np.float64)
    hot = (np.arange(classes)[None, :] == np.asarray(t)[:, None]).astype(np.float64)
    cabs = hot if score == "logit" else proba[np.arange(n), t][:, None] * (hot + proba)
    dH = (np.asarray(h) > 0) * (cabs @ W2.T)
    wbar = W1.reshape(C, hr * wr, U).sum(1)              # [C, U]
    alpha = dH @ wbar.T / (hr * wr)
    terms = (alpha[:, :, None, None] * A).sum(1)
    path = (0 if score == "logit" else 2) + 1 + (classes - 1) + (hr * wr - 1) + 1 + -(-U // 64) + 6 + 2 + 1 + C + 1
    return path * U32 * terms


# ---------------------------------------------------------------------------------------------------------
# fp32 twins of the kernels
# ---------------------------------------------------------------------------------------------------------

def w1sum_twin(W1, hs, ws, hr, wr, Cp, Cr):
    """``gt_cam_w1sum``: ``W1 [G, hs * ws * Cp, Up]`` fp32 -> ``wbar [G, Cp, Up]``: plain fp32 adds over the real
    pixels in row-major order starting from 0; channels >= Cr stay 0. Padded pixels are not read."""
    G, _, Up = W1.shape
    W = W1.reshape(G, hs, ws, Cp, Up)
    acc = np.zeros((G, Cp, Up), np.float32)
    for i in range(hr):
        for j in range(wr):
            acc[:, :Cr] = acc[:, :Cr] + W[:, i, j, :Cr]
    return acc


def ordered_mean(w, per):
    """``w[0] * per[0]``, then ``acc + w[g] * per[g]``: fp32, the product and the sum rounded separately."""
    w = np.asarray(w, np.float32)
    acc = np.multiply(w[0], per[0], dtype=np.float32)
    for g in range(1, len(per)):
        acc = np.add(acc, np.multiply(w[g], per[g], dtype=np.float32), dtype=np.float32)
    return acc


def head_twin(logits, proba, weight, feat, hid, W2, wbar, tgt, hr, wr, Cr, logit, relu):
    """``gt_head_gradcam`` after its softmaxes: ``logits`` / ``proba [G, m, C]`` fp32 are every member's rows as
    ``gt_head_predict`` writes them; ``feat [G, m, hs, ws, Cp]`` and ``hid [G, m, Up]`` the feature map and hidden
    activations as fp32 values (a bf16 buffer converted exactly); ``W2 [G, Up, C]``, ``wbar [G, Cp, Up]`` fp32;
    ``tgt [m]`` ints, negative for the label. Returns ``(map [m, hr, wr], tgt [m], base [m])``."""
    logits, proba = np.asarray(logits, np.float32), np.asarray(proba, np.float32)
    feat, hid = np.asarray(feat, np.float32), np.asarray(hid, np.float32)
    W2, wbar = np.asarray(W2, np.float32), np.asarray(wbar, np.float32)
    G, m, C = proba.shape
    Up = hid.shape[2]
    rows = np.arange(m)
    mean = ordered_mean(weight, proba)
    t = np.where(np.asarray(tgt) < 0, np.argmax(mean, 1), np.asarray(tgt)).astype(np.int64)      # first maximum
    base = (ordered_mean(weight, logits) if logit else mean)[rows, t]
    inv_n = np.float32(1) / np.float32(hr * wr)
    hot = (np.arange(C)[None, :] == t[:, None]).astype(np.float32)
    lanes = np.arange(64)
    cams = []
    for g in range(G):
        p = proba[g]
        coef = hot if logit else p[rows, t][:, None] * (hot - p)                                 # (b)
        live = hid[g].view(np.int32) > 0                 # positive sign, any non-zero magnitude
        dH = coef[:, None, 0] * W2[g][None, :, 0]
        for c in range(1, C):
            dH = dH + coef[:, None, c] * W2[g][None, :, c]
        dH = np.where(live, dH, np.float32(0))
        alpha = np.zeros((m, Cr), np.float32)
        for c in range(Cr):                                                                       # (c)
            prod = dH * wbar[g, c][None, :]
            s = np.zeros((m, 64), np.float32)
            for k in range(0, Up, 64):
                seg = prod[:, k:k + 64]
                s[:, :seg.shape[1]] = s[:, :seg.shape[1]] + seg
            for o in (32, 16, 8, 4, 2, 1):
                s = s + s[:, lanes ^ o]
            alpha[:, c] = s[:, 0] * inv_n
        v = np.zeros((m, hr, wr), np.float32)
        for c in range(Cr):                                                                       # (d)
            v = v + alpha[:, c, None, None] * feat[g, :, :hr, :wr, c]
        if relu:
            v = np.where(v > 0, v, np.float32(0))
        assert dH.dtype == alpha.dtype == v.dtype == np.float32
        cams.append(v)
    return ordered_mean(weight, np.stack(cams)), t, base                                          # (e)
