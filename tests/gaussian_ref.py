"""A plain-loop fp64 oracle of the feature-space Gaussian of ``gaussian_fit`` / ``mahalanobis``
(gentun_amd/models/cnn_fitted.py): moments, shrinkage, whitening and distance of one member, written
independently of the package's vectorised definitions."""

import numpy as np


def moments_ref(f, labels, C):
    """``(count, mean fp32 [C, U], cov fp64 [U, U])``: row-order fp64 sums, fp32 centring, scatter / N."""
    f = np.asarray(f, np.float32)
    N, U = f.shape
    count, sums = [0] * C, [[0.0] * U for _ in range(C)]
    for r in range(N):
        count[labels[r]] += 1
        for u in range(U):
            sums[labels[r]][u] += float(f[r, u])
    mean = np.array([[sums[c][u] / max(count[c], 1) for u in range(U)] for c in range(C)]).astype(np.float32)
    c = [[float(np.float32(f[r, u] - mean[labels[r], u])) for u in range(U)] for r in range(N)]
    cov = np.zeros((U, U))
    for i in range(U):
        for j in range(U):
            s = 0.0
            for r in range(N):
                s += c[r][i] * c[r][j]
            cov[i, j] = s / N
    return np.array(count, np.int64), mean, cov


def whiten_ref(cov, mean, shrink):
    """``(W fp32 [U, U], t fp32 [C, U])``: Cholesky-Banachiewicz of the shrunk covariance, ``W = L^-T`` by forward
    substitution, ``t_c = W^T mean_c`` from the rounded ``W``."""
    U = len(cov)
    tr = sum(cov[i, i] for i in range(U)) / U
    A = [[(1.0 - shrink) * cov[i, j] + (shrink * tr if i == j else 0.0) for j in range(U)] for i in range(U)]
    L = [[0.0] * U for _ in range(U)]
    for i in range(U):
        for j in range(i + 1):
            s = A[i][j] - sum(L[i][k] * L[j][k] for k in range(j))
            L[i][j] = s ** 0.5 if i == j else s / L[j][j]
    inv = [[0.0] * U for _ in range(U)]                      # L^-1, column by column
    for j in range(U):
        for i in range(j, U):
            s = (1.0 if i == j else 0.0) - sum(L[i][k] * inv[k][j] for k in range(j, i))
            inv[i][j] = s / L[i][i]
    W = np.array(inv).T.astype(np.float32)
    t = [[sum(float(mean[c, i]) * float(W[i, j]) for i in range(U)) for j in range(U)] for c in range(len(mean))]
    return W, np.array(t).astype(np.float32)


def distance_ref(f, W, t, count):
    """fp64 ``[n, C]``: ``sum_j (sum_i f_i W_ij - t_cj)^2``, ``+inf`` for an empty class."""
    f, W, t = np.asarray(f, np.float64), np.asarray(W, np.float64), np.asarray(t, np.float64)
    d = np.empty((len(f), len(t)))
    for r in range(len(f)):
        z = [sum(f[r, i] * W[i, j] for i in range(W.shape[0])) for j in range(W.shape[1])]
        for c in range(len(t)):
            d[r, c] = sum((z[j] - t[c, j]) ** 2 for j in range(len(z))) if count[c] else np.inf
    return d
