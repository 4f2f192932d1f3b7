"""The fp64 oracle of Monte-Carlo dropout (gentun_amd/models/cnn_fitted.py ``predict_mc``), straight from the
definition: masks from ``utils.rng.mc_masks``, everything else in numpy fp64. The variance is taken directly over
all ``(m, t)`` samples around the combined mean, not through the decomposition the implementations use."""

import numpy as np

from gentun_amd.utils.rng import mc_masks


def oracle(h, W2, b2, weights, samples, dropout, seed, rows, units=None):
    """``h [k, n, U]`` hidden rows, ``W2 [k, U, C]``, ``b2 [k, C]``, normalised ``weights [k]``, ``rows [n]`` the
    images' indices; only the first ``units`` of ``U`` count. Returns the dict of ``predict_mc`` in fp64 plus
    ``expected_entropy`` and ``samples [n, k, T, C]``."""
    h, W2, b2 = (np.asarray(v, np.float64) for v in (h, W2, b2))
    w = np.asarray(weights, np.float64)
    k, n, U = h.shape
    units = U if units is None else units
    s = float(np.float32(1) / (np.float32(1) - np.float32(dropout)))
    p = np.empty((k, n, samples, W2.shape[2]))
    for m in range(k):
        keep = mc_masks(seed, m, samples, rows, units, dropout)                    # [T, n, units]
        hm = np.where(keep, h[m][None, :, :units] * s, 0.0)
        z = hm @ W2[m][:units] + b2[m]
        e = np.exp(z - z.max(-1, keepdims=True))
        p[m] = (e / e.sum(-1, keepdims=True)).transpose(1, 0, 2)
    wt = w[:, None, None, None]
    proba = (wt * p).sum(0).mean(1)                                                # [n, C]
    var = (wt * (p - proba[None, :, None, :]) ** 2).sum(0).mean(1)

    def H(q):
        return -(q * np.log(np.where(q > 0, q, 1.0))).sum(-1)
    entropy = H(proba)
    expected = (w[:, None, None] * H(p)).sum(0).mean(1)
    return {"proba": proba, "std": np.sqrt(var), "entropy": entropy, "expected_entropy": expected,
            "mutual_info": np.maximum(entropy - expected, 0.0), "label": np.argmax(proba, 1),
            "samples": p.transpose(1, 0, 2, 3)}
