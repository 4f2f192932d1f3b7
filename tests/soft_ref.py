"""fp64 numpy oracle of the soft-target training head: target rows, both losses and the logit gradient dz.

Independent of the torch code: plain loops over rows and classes, no autograd. The definitions are those of
gentun_amd/models/cnn_engine.py ("The target row").
"""

import numpy as np

CLIP_EPS = 1e-7


def smoothing_targets(eps, classes):
    """(t_on, t_off) in numpy fp32: t_off = fp32(eps) / fp32(C), t_on = (fp32(1) - fp32(eps)) + t_off."""
    e = np.float32(eps)
    t_off = np.float32(e / np.float32(classes))
    t_on = np.float32(np.float32(np.float32(1.0) - e) + t_off)
    return t_on, t_off


def target_rows(labels, sids, classes, table=None, eps=0.0):
    """fp64 [len(sids), C] target rows of the batch rows with sample ids ``sids``."""
    out = np.zeros((len(sids), classes), np.float64)
    t_on, t_off = smoothing_targets(eps, classes)
    for r, sid in enumerate(sids):
        for c in range(classes):
            if table is not None:
                out[r, c] = np.float64(table[sid, c])
            elif eps > 0.0:
                out[r, c] = np.float64(t_on if c == labels[sid] else t_off)
            else:
                out[r, c] = 1.0 if c == labels[sid] else 0.0
    return out


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def row_loss(z, t, mode):
    """The loss of one row with logits ``z`` [C] and target row ``t`` [C]."""
    p = softmax(z)
    C = len(p)
    if mode == "ce":
        return -sum(t[c] * np.log(max(p[c], 1e-30)) for c in range(C))
    tot = 0.0
    for c in range(C):
        pc = min(max(p[c], CLIP_EPS), 1.0 - CLIP_EPS)
        tot += -(t[c] * np.log(pc) + (1.0 - t[c]) * np.log(1.0 - pc))
    return tot / C


def row_dz(z, t, mode, inv_b=1.0):
    """d(inv_b * loss) / dz of one row, as the kernel forms it."""
    p = softmax(z)
    C = len(p)
    if mode == "ce":
        return np.array([(p[c] - t[c]) * inv_b for c in range(C)])
    dp = np.zeros(C)
    s = 0.0
    for c in range(C):
        inside = CLIP_EPS <= p[c] <= 1.0 - CLIP_EPS
        pc = min(max(p[c], CLIP_EPS), 1.0 - CLIP_EPS)
        dp[c] = (pc - t[c]) / (pc * (1.0 - pc)) / C if inside else 0.0
        s += p[c] * dp[c]
    return np.array([p[c] * (dp[c] - s) * inv_b for c in range(C)])


def batch_loss(logits, targets, mode, nvalid=None, nnorm=None):
    """Mean loss over the first ``nvalid`` rows of a batch [B, C] (the Keras short batch), normalised by
    ``nnorm`` (default ``nvalid``)."""
    B = logits.shape[0]
    nv = B if nvalid is None else int(nvalid)
    nn = nv if nnorm is None else int(nnorm)
    return sum(row_loss(logits[b], targets[b], mode) for b in range(nv)) / nn if nn > 0 else 0.0


def batch_dz(logits, targets, mode, nvalid=None, nnorm=None):
    """fp64 [B, C]: the gradient of :func:`batch_loss` by the logits; rows past ``nvalid`` are zero."""
    B = logits.shape[0]
    nv = B if nvalid is None else int(nvalid)
    nn = nv if nnorm is None else int(nnorm)
    out = np.zeros(logits.shape, np.float64)
    for b in range(B):
        inv_b = 1.0 / nn if (b < nv and nn > 0) else 0.0
        out[b] = row_dz(logits[b], targets[b], mode, inv_b)
    return out


def random_table(rng, n, classes, labels=None, peak=0.0):
    """A valid fp32 table: rows of a Dirichlet draw (optionally mixed towards the labels), renormalised in
    fp64 before the one rounding to fp32."""
    t = rng.dirichlet(np.ones(classes), size=n)
    if labels is not None and peak > 0.0:
        oh = np.zeros((n, classes))
        oh[np.arange(n), labels] = 1.0
        t = (1.0 - peak) * t + peak * oh
    t = t / t.sum(1, keepdims=True)
    return np.ascontiguousarray(t.astype(np.float32))
