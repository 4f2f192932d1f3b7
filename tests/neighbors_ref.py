"""Plain-loop oracle of ``neighbors`` (gentun_amd/models/cnn_fitted.py), written apart from it: one (query, bank
row) pair at a time, Python floats (fp64), the features summed in feature order."""

import math

import numpy as np


def distance64(q, b, metric):
    """The fp64 distance of two fp32 feature rows."""
    dot = qq = bb = 0.0
    for u, v in zip(q.tolist(), b.tolist()):
        dot += u * v
        qq += u * u
        bb += v * v
    if metric == "l2":
        return max(qq + bb - 2.0 * dot, 0.0)
    den = math.sqrt(qq) * math.sqrt(bb)
    return 1.0 - dot / den if den > 0.0 else 1.0


def neighbors_ref(q, b, k, metric):
    """``(index int64 [n, k], distance fp32 [n, k])``: every distance rounded to fp32 once, then the ``k`` smallest
    ``(distance, index)`` pairs of every query in ascending order."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    d32 = np.array([[distance64(qi, bj, metric) for bj in b] for qi in q]).reshape(len(q), len(b)).astype(np.float32)
    idx, dist = np.empty((len(d32), k), np.int64), np.empty((len(d32), k), np.float32)
    for i, row in enumerate(d32):
        best = sorted((float(d), j) for j, d in enumerate(row))[:k]
        idx[i], dist[i] = [j for _, j in best], [d for d, _ in best]
    return idx, dist
