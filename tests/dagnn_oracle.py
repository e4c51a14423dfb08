"""fp64 numpy restatement of DAGNN (docs/DAGNN_SEMANTICS.md): the gated propagation out[i] = sum_k s_k[i] H_k[i], H_k = P H_{k-1},
s_k[i] = sigmoid(<H_k[i], w> + b) over APPNP's operator P = D_in^-1/2 A D_out^-1/2, its explicit backward recurrence, the L-layer model
(APPNP's MLP trunk, with the hidden layers' dropout masks as INPUTS) and full training steps with Adam.  Neither the reference nor dgl
defines this model: this file, its finite differences and the identities with tests/gpr_oracle.py under a zero gate weight
(tests/test_dagnn_cpu.py) are what pins the arithmetic."""
import numpy as np

from appnp_oracle import adam, nll_and_grad
from gpr_oracle import step, step_t, trunk_backward, trunk_forward

W, B = "encoder.propagate.proj.weight", "encoder.propagate.proj.bias"


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def hops(indptr, indices, h0, k):
    """[H_0 .. H_K],  H_0 = h0, H_j = P H_{j-1}."""
    hs = [np.asarray(h0, np.float64)]
    for _ in range(k):
        hs.append(step(indptr, indices, hs[-1]))
    return hs


def gates(hs, w, b):
    """[s_0 .. s_K], s_j [n] = sigmoid(H_j w + b)."""
    w, b = np.asarray(w, np.float64).reshape(-1), float(np.asarray(b, np.float64).reshape(-1)[0])
    return [sigmoid(h @ w + b) for h in hs]


def propagate(indptr, indices, h0, w, b, k):
    """out = sum_{j = 0..K} s_j[:, None] * H_j."""
    hs = hops(indptr, indices, h0, k)
    return sum(s[:, None] * h for s, h in zip(gates(hs, w, b), hs))


def propagate_bwd(indptr, indices, g, h0, w, b, k):
    """(dL/dh0, dL/dw [C], dL/db) from g = dL/dout:  q_j = (g . H_j) s_j (1 - s_j) per row,  D_j = s_j g + q_j w,
    T_K = D_K, T_j = D_j + P^T T_{j+1}, dh0 = T_0;  dw = sum_j H_j^T q_j, db = sum_j sum_i q_j[i]."""
    g = np.asarray(g, np.float64)
    w = np.asarray(w, np.float64).reshape(-1)
    hs = hops(indptr, indices, h0, k)
    ss = gates(hs, w, b)
    qs = [(g * h).sum(1) * s * (1.0 - s) for h, s in zip(hs, ss)]
    t = None
    for j in range(k, -1, -1):
        d = ss[j][:, None] * g + qs[j][:, None] * w[None, :]
        t = d if t is None else d + step_t(indptr, indices, t)
    dw = sum(h.T @ q for h, q in zip(hs, qs))
    db = float(sum(q.sum() for q in qs))
    return t, dw, db


def finite_difference_check(indptr, indices, h0, w, b, k, weight, eps=1e-6):
    """Central differences of L = <weight, propagate(h0, w, b)> in EVERY entry of h0, w and b against propagate_bwd: the largest error
    relative to the largest gradient entry, as (dh0, dw, db)."""
    h0 = np.asarray(h0, np.float64)
    w = np.asarray(w, np.float64).reshape(-1)
    b = float(b)
    loss = lambda h, ww, bb: float((weight * propagate(indptr, indices, h, ww, bb, k)).sum())
    dh0, dw, db = propagate_bwd(indptr, indices, weight, h0, w, b, k)
    fh = np.zeros_like(h0)
    for idx in np.ndindex(*h0.shape):
        d = np.zeros_like(h0)
        d[idx] = eps
        fh[idx] = (loss(h0 + d, w, b) - loss(h0 - d, w, b)) / (2 * eps)
    fw = np.zeros_like(w)
    for c in range(len(w)):
        d = np.zeros_like(w)
        d[c] = eps
        fw[c] = (loss(h0, w + d, b) - loss(h0, w - d, b)) / (2 * eps)
    fb = (loss(h0, w, b + eps) - loss(h0, w, b - eps)) / (2 * eps)
    rel = lambda got, ref: float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
    return rel(fh, dh0), rel(fw, dw), rel(np.asarray([fb]), np.asarray([db]))


def model_forward(params, bn_state, indptr, indices, x, num_layers, norm_type, k):
    """Eval-mode logits of the L-layer model (running statistics, no dropout)."""
    _, h0, _ = trunk_forward(params, x, num_layers, norm_type, bn_state, training=False)
    return propagate(indptr, indices, h0, params[W], params[B], k)


def loss_and_grads(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, k, masks=None, p=0.0):
    """One training-mode forward + backward: (loss, {param name: grad}, the gate's included); bn_state is updated in place."""
    _, h0, cache = trunk_forward(params, x, num_layers, norm_type, bn_state, training=True, masks=masks, p=p)
    logits = propagate(indptr, indices, h0, params[W], params[B], k)
    loss, gl = nll_and_grad(logits, labels, idx)
    dh0, dw, db = propagate_bwd(indptr, indices, gl, h0, params[W], params[B], k)
    grads = trunk_backward(params, cache, dh0, num_layers)
    grads[W] = dw.reshape(np.shape(params[W]))
    grads[B] = np.asarray([db])
    return loss, grads


def train_steps(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, k, masks_per_step, p, lr, wd, steps):
    """`steps` full-graph `train` steps with Adam (L2 weight decay on every parameter, the gate's included, as torch.optim.Adam applies it).
    Returns (losses, grads of the first step, params, Adam state {name: (m, v)}, bn_state)."""
    params = {a: np.asarray(v, np.float64).copy() for a, v in params.items()}
    state, losses, first = {}, [], None
    for s in range(steps):
        m = None if masks_per_step is None else masks_per_step[s]
        loss, grads = loss_and_grads(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, k, m, p)
        if first is None:
            first = {a: v.copy() for a, v in grads.items()}
        losses.append(loss)
        adam(params, grads, state, s + 1, lr, wd)
    return np.asarray(losses), first, params, state, bn_state
