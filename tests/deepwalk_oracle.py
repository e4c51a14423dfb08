"""numpy oracle of the DeepWalk step (docs/POSITION_SEMANTICS.md): pairs, loss, gradient, lazy Adam as plain formulas.  TEST
INFRASTRUCTURE ONLY: no torch, no GPU.  fp64 by default; `dtype=np.float32` runs the very same arithmetic in fp32 -- the yardstick the GPU
tolerances are derived from (tests/test_deepwalk_gpu.py).  The walk is subgraph_oracle.random_walk, the negative draw
oracle.dropout_mask.drop_hash -- the sampler's own."""
import math

import numpy as np

from oracle.dropout_mask import drop_hash
from subgraph_oracle import random_walk


def pairs(indptr, indices, roots, length, context, negatives, walk_seed, neg_seed):
    """(walks [B, L + 1], start [Q], rest [Q, R]): window q = i * nwin + j starts at walks[i, j]; entries t < c - 1 are the positives
    walks[i, j + 1 + t], the others the uniform negatives (drop_hash(neg_seed, q, t - (c - 1)) * N) >> 32."""
    n = len(indptr) - 1
    walks = random_walk(indptr, indices, roots, length, walk_seed)
    nwin, n_pos = length + 2 - context, context - 1
    q_all = len(walks) * nwin
    i, j = np.divmod(np.arange(q_all), nwin)                          # window q = i * nwin + j
    start = walks[i, j]
    rest = np.zeros((q_all, (1 + negatives) * n_pos), np.int64)
    for t in range(n_pos):
        rest[:, t] = walks[i, j + 1 + t]
    draws = drop_hash(neg_seed, np.arange(q_all)[:, None], np.arange(negatives * n_pos)[None, :])      # uint64 values < 2^32
    rest[:, n_pos:] = ((draws * np.uint64(n)) >> np.uint64(32)).astype(np.int64)                       # (< 2^63: n < 2^31)
    return walks, start, rest


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def loss_and_grad(z, start, rest, context, negatives, dtype=np.float64):
    """(loss, dZ [N, d], touched [N] bool) at the frozen table z: loss = mean over positives of softplus(-s) + mean over negatives of
    softplus(s), s = <z_a, z_x>; touched = the rows that are the start or an entry of some pair."""
    z = np.asarray(z, dtype)
    n_pos_row = context - 1
    q_all, r = rest.shape
    n_pos, n_neg = q_all * n_pos_row, q_all * n_pos_row * negatives
    za, zx = z[start], z[rest]                                        # [Q, d], [Q, R, d]
    s = np.einsum("qd,qrd->qr", za, zx).astype(dtype)
    pos = np.arange(r)[None, :] < n_pos_row
    loss = softplus(-s[:, :n_pos_row]).sum(dtype=dtype) / dtype(n_pos) + softplus(s[:, n_pos_row:]).sum(dtype=dtype) / dtype(n_neg)
    g = np.where(pos, -sigmoid(-s) / dtype(n_pos), sigmoid(s) / dtype(n_neg)).astype(dtype)      # sigmoid(s) - 1 = -sigmoid(-s)
    dz = np.zeros_like(z)
    np.add.at(dz, start, np.einsum("qr,qrd->qd", g, zx).astype(dtype))
    np.add.at(dz, rest.reshape(-1), (g[:, :, None] * za[:, None, :]).reshape(-1, z.shape[1]))
    touched = np.zeros(len(z), bool)
    touched[start] = True
    touched[rest.reshape(-1)] = True
    return dtype(loss), dz, touched


def lazy_adam(z, m, v, dz, touched, lr, betas, eps, t, dtype=np.float64):
    """torch.optim.SparseAdam's arithmetic on the touched rows, step count t (1-based, global); every other row is returned as it came."""
    z, m, v = np.array(z, dtype), np.array(m, dtype), np.array(v, dtype)
    b1, b2 = dtype(betas[0]), dtype(betas[1])
    step_size = dtype(lr * math.sqrt(1 - betas[1] ** t) / (1 - betas[0] ** t))
    r = touched
    m[r] = b1 * m[r] + dtype(1 - betas[0]) * dz[r]
    v[r] = b2 * v[r] + dtype(1 - betas[1]) * dz[r] * dz[r]
    z[r] = z[r] - step_size * (m[r] / (np.sqrt(v[r]) + dtype(eps)))
    return z, m, v


def step(z, m, v, indptr, indices, roots, length, context, negatives, walk_seed, neg_seed, lr, betas, eps, t, dtype=np.float64):
    """One whole step; returns (z, m, v, loss, touched)."""
    _, start, rest = pairs(indptr, indices, roots, length, context, negatives, walk_seed, neg_seed)
    loss, dz, touched = loss_and_grad(z, start, rest, context, negatives, dtype)
    z, m, v = lazy_adam(z, m, v, dz, touched, lr, betas, eps, t, dtype)
    return z, m, v, loss, touched


def centroid_accuracy(z, labels):
    """Nearest-class-centroid accuracy of the rows of z against integer labels (the centroids are the class means of z itself)."""
    z, labels = np.asarray(z, np.float64), np.asarray(labels)
    cents = np.stack([z[labels == c].mean(axis=0) for c in np.unique(labels)])
    d2 = ((z[:, None, :] - cents[None, :, :]) ** 2).sum(axis=2)
    return float((np.unique(labels)[d2.argmin(axis=1)] == labels).mean())
