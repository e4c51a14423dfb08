"""numpy oracle of the node2vec pieces of the position features (docs/POSITION_SEMANTICS.md): the second-order (p, q) walk with its integer
rejection sampling (vectorised over the walks, attempt loop included), the 32-bit CDF of the degree^power negatives and the draw from it,
and the two-table skip-gram step.  TEST INFRASTRUCTURE ONLY: no torch, no GPU.  fp64 by default; `dtype=np.float32` runs the same
arithmetic in fp32, the yardstick of the GPU tolerances.  Everything the one-table oracle already states is taken from it."""
import math

import numpy as np

import deepwalk_oracle as dwo
from oracle.dropout_mask import drop_hash
from subgraph_oracle import random_walk  # noqa: F401  (the walk this one must equal at p = q = 1)

ACCEPT_XOR = 0x4E32564B        # the acceptance draw's seed is the walk seed xor this
ATTEMPT_STRIDE = 128           # attempt a of step s draws at column s + 128 a
MAX_ATTEMPTS = 256             # the 256th candidate is taken whatever its acceptance draw says
P_Q_RANGE = (0.25, 4.0)


# ---------------------------------------------------------------------------------------------------- the walk
def thresholds(p, q):
    """(T_return, T_near, T_far): T_c = min(2^32, floor(w_c / wmax * 2^32)) in double, w = (1/p, 1, 1/q), wmax their largest."""
    w = (1.0 / p, 1.0, 1.0 / q)
    wmax = max(w)
    return tuple(min(2 ** 32, int(math.floor(wc / wmax * 2.0 ** 32))) for wc in w)


def edge_keys(indptr, indices):
    """Sorted distinct keys t * N + x of the stored entries: x appears in row t."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    return np.unique(rows * n + np.asarray(indices, np.int64))


def in_row(keys, n, t, x):
    """Per element: does x appear in row t?"""
    k = t * n + x
    at = np.searchsorted(keys, k)
    return (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == k) if len(keys) else np.zeros(len(k), bool)


def node2vec_walk(indptr, indices, roots, length, p, q, seed):
    """out [n_roots, length + 1] int64, column 0 the roots.  Step 1 is random_walk's.  At step s >= 2, standing on v = out[i, s - 1] with
    t = out[i, s - 2], attempt a draws x = indices[indptr[v] + ((drop_hash(seed, i, s + 128 a) * deg) >> 32)], whose class is return
    (x == t, tested first), near (x appears in row t) or far, and accepts it iff drop_hash(seed ^ 0x4E32564B, i, s + 128 a) < T_class; the
    256th candidate is taken unconditionally.  deg == 0: the walk stays."""
    assert P_Q_RANGE[0] <= p <= P_Q_RANGE[1] and P_Q_RANGE[0] <= q <= P_Q_RANGE[1]
    roots = np.asarray(roots, np.int64)
    out = np.zeros((len(roots), length + 1), np.int64)
    out[:, 0] = roots
    if len(roots) == 0:
        return out
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = len(indptr) - 1
    t_ret, t_near, t_far = (np.uint64(t) for t in thresholds(p, q))
    keys = edge_keys(indptr, indices)
    for s in range(1, length + 1):
        v = out[:, s - 1]
        e0, deg = indptr[v], indptr[v + 1] - indptr[v]
        nxt = v.copy()
        pending = deg > 0
        for a in range(MAX_ATTEMPTS):
            idx = np.flatnonzero(pending)
            if len(idx) == 0:
                break
            col = s + ATTEMPT_STRIDE * a
            r = drop_hash(seed, idx, col)                                           # uint64 values < 2^32
            x = indices[e0[idx] + ((r * deg[idx].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)]
            if s == 1 or a == MAX_ATTEMPTS - 1:
                accept = np.ones(len(idx), bool)
            else:
                t = out[idx, s - 2]
                thr = np.where(x == t, t_ret, np.where(in_row(keys, n, t, x), t_near, t_far))
                accept = drop_hash(seed ^ ACCEPT_XOR, idx, col) < thr
            nxt[idx[accept]] = x[accept]
            pending[idx[accept]] = False
        out[:, s] = nxt
    return out


def step_probabilities(indptr, indices, t, v, p, q):
    """The exact node2vec distribution of the step from v having come from t: {x: probability}, over the stored entries of row v (a
    multi-edge counts as often as it is stored)."""
    n = len(indptr) - 1
    keys = edge_keys(indptr, indices)
    w = {}
    for x in np.asarray(indices[indptr[v]:indptr[v + 1]], np.int64):
        x = int(x)
        wx = 1.0 / p if x == t else (1.0 if in_row(keys, n, np.array([t]), np.array([x]))[0] else 1.0 / q)
        w[x] = w.get(x, 0.0) + wx
    total = sum(w.values())
    return {x: wx / total for x, wx in w.items()}


# ---------------------------------------------------------------------------------------------------- negatives from a distribution
def negative_cdf(indptr, indices, power):
    """int64 [N] of values in [0, 2^32): cdf[n] = min(2^32 - 1, floor(cumsum(w)[n] / sum(w) * 2^32)), w_n = out_degree_n ** power with
    out_degree_n the number of times n occurs in `indices`; degree 0 gives weight 0."""
    n = len(indptr) - 1
    deg = np.bincount(np.asarray(indices, np.int64), minlength=n).astype(np.float64)
    w = np.where(deg > 0, deg ** float(power), 0.0)
    assert w.sum() > 0
    return np.minimum(np.floor(np.cumsum(w) / w.sum() * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.int64)


def draw_from_cdf(cdf, r):
    """The number of n in [0, N - 1) with cdf[n] <= r, per draw r: in [0, N - 1]."""
    cdf = np.asarray(cdf, np.int64)
    return np.searchsorted(cdf[:len(cdf) - 1], np.asarray(r).astype(np.int64), side="right").astype(np.int64)


def pairs_from_walks(walks, n_nodes, context, negatives, neg_seed, cdf=None):
    """(start [Q], rest [Q, R]) as deepwalk_oracle.pairs makes them from its own walks; cdf None: its uniform negatives, else the draw
    r = drop_hash(neg_seed, q, t') is mapped through draw_from_cdf."""
    walks = np.asarray(walks, np.int64)
    length = walks.shape[1] - 1
    nwin, n_pos = length + 2 - context, context - 1
    q_all = len(walks) * nwin
    i, j = np.divmod(np.arange(q_all), nwin)
    start = walks[i, j]
    rest = np.zeros((q_all, (1 + negatives) * n_pos), np.int64)
    for t in range(n_pos):
        rest[:, t] = walks[i, j + 1 + t]
    draws = drop_hash(neg_seed, np.arange(q_all)[:, None], np.arange(negatives * n_pos)[None, :])
    if cdf is None:
        rest[:, n_pos:] = ((draws * np.uint64(n_nodes)) >> np.uint64(32)).astype(np.int64)
    else:
        rest[:, n_pos:] = draw_from_cdf(cdf, draws)
    return start, rest


# ---------------------------------------------------------------------------------------------------- two tables
def loss_and_grad(z, c, start, rest, context, negatives, dtype=np.float64, tied=False):
    """(loss, dZ, dC, touched_z, touched_c) at the frozen tables: s = <z_a, c_x>; dZ[a] = sum g c_x over a's windows (the start list
    alone), dC[x] = sum g z_a over x's positions (the pair list alone); touched_z = the starts, touched_c = the entries.
    tied: c IS z -- both sums go into one accumulator in the one-table oracle's order and (loss, dZ, dZ, touched, touched) comes back."""
    z = np.asarray(z, dtype)
    c = z if tied else np.asarray(c, dtype)
    n_pos_row = context - 1
    q_all, r = rest.shape
    n_pos, n_neg = q_all * n_pos_row, q_all * n_pos_row * negatives
    za, cx = z[start], c[rest]
    s = np.einsum("qd,qrd->qr", za, cx).astype(dtype)
    pos = np.arange(r)[None, :] < n_pos_row
    loss = dwo.softplus(-s[:, :n_pos_row]).sum(dtype=dtype) / dtype(n_pos) + dwo.softplus(s[:, n_pos_row:]).sum(dtype=dtype) / dtype(n_neg)
    g = np.where(pos, -dwo.sigmoid(-s) / dtype(n_pos), dwo.sigmoid(s) / dtype(n_neg)).astype(dtype)
    dz = np.zeros_like(z)
    np.add.at(dz, start, np.einsum("qr,qrd->qd", g, cx).astype(dtype))
    dc = dz if tied else np.zeros_like(c)
    np.add.at(dc, rest.reshape(-1), (g[:, :, None] * za[:, None, :]).reshape(-1, z.shape[1]))
    tz, tc = np.zeros(len(z), bool), np.zeros(len(z), bool)
    tz[start] = True
    tc[rest.reshape(-1)] = True
    if tied:
        tz = tc = tz | tc
    return dtype(loss), dz, dc, tz, tc


def step(state, indptr, indices, roots, length, context, negatives, walk_seed, neg_seed, lr, betas, eps, t, p=1.0, q=1.0, cdf=None,
         dtype=np.float64, tied=False):
    """One whole step.  state = (z, mz, vz, c, mc, vc) (tied: the last three are ignored and returned as None); returns
    (state, loss, touched_z, touched_c).  Both tables take the same step count t."""
    z, mz, vz, c, mc, vc = state
    walks = node2vec_walk(indptr, indices, roots, length, p, q, walk_seed)
    start, rest = pairs_from_walks(walks, len(indptr) - 1, context, negatives, neg_seed, cdf)
    loss, dz, dc, tz, tc = loss_and_grad(z, c, start, rest, context, negatives, dtype, tied)
    z, mz, vz = dwo.lazy_adam(z, mz, vz, dz, tz, lr, betas, eps, t, dtype)
    if tied:
        return (z, mz, vz, None, None, None), loss, tz, tc
    c, mc, vc = dwo.lazy_adam(c, mc, vc, dc, tc, lr, betas, eps, t, dtype)
    return (z, mz, vz, c, mc, vc), loss, tz, tc
