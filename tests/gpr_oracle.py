"""fp64 numpy restatement of GPR-GNN (docs/GPR_SEMANTICS.md): the propagation out = sum_k gamma_k P^k h0 over APPNP's operator
P = D_in^-1/2 A D_out^-1/2, its explicit backward recurrence, the L-layer model (APPNP's MLP trunk, with the hidden layers' dropout masks
as INPUTS) and one full training step with Adam.  Neither the reference nor dgl defines this model: this file and the identity with
tests/appnp_oracle.py under PPR coefficients (tests/test_gpr_cpu.py) are what pins the arithmetic."""
import numpy as np

from appnp_oracle import adam, degree_norms, nll_and_grad
from graphgen import segment_reduce


def _rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def ppr_gamma(k, alpha):
    """APPNP's teleport weights: gamma_j = alpha (1 - alpha)^j for j < K, gamma_K = (1 - alpha)^K (they sum to 1)."""
    g = alpha * (1.0 - alpha) ** np.arange(k + 1, dtype=np.float64)
    g[k] = (1.0 - alpha) ** k
    return g


def step(indptr, indices, h):
    """P h:  (P h)[i] = dst_norm[i] sum_{e = (j -> i)} src_norm[j] h[j]  (multi-edges count; a row without in-edges gives 0)."""
    n = len(indptr) - 1
    dn, sn = degree_norms(indptr, indices, n)
    dst, src = _rows(indptr), indices.astype(np.int64)
    return dn[:, None] * segment_reduce(np.add, sn[src, None] * h[src], dst, n, 0.0)


def step_t(indptr, indices, g):
    """P^T g:  (P^T g)[j] = src_norm[j] sum_{e = (j -> i)} dst_norm[i] g[i]."""
    n = len(indptr) - 1
    dn, sn = degree_norms(indptr, indices, n)
    dst, src = _rows(indptr), indices.astype(np.int64)
    return sn[:, None] * segment_reduce(np.add, dn[dst, None] * g[dst], src, n, 0.0)


def propagate(indptr, indices, h0, gamma):
    """out = sum_{k = 0..K} gamma_k H_k,  H_0 = h0, H_k = P H_{k-1};  K = len(gamma) - 1."""
    h = np.asarray(h0, np.float64)
    gamma = np.asarray(gamma, np.float64)
    out = gamma[0] * h
    for k in range(1, len(gamma)):
        h = step(indptr, indices, h)
        out = out + gamma[k] * h
    return out


def propagate_bwd(indptr, indices, g, h0, gamma):
    """(dL/dh0, dL/dgamma) from g = dL/dout:  G_0 = g, G_k = P^T G_{k-1};  dgamma_k = <G_k, h0>,  dh0 = sum_k gamma_k G_k."""
    gk = np.asarray(g, np.float64)
    h0 = np.asarray(h0, np.float64)
    gamma = np.asarray(gamma, np.float64)
    dh0 = gamma[0] * gk
    dgamma = np.zeros(len(gamma))
    dgamma[0] = (gk * h0).sum()
    for k in range(1, len(gamma)):
        gk = step_t(indptr, indices, gk)
        dgamma[k] = (gk * h0).sum()
        dh0 = dh0 + gamma[k] * gk
    return dh0, dgamma


def finite_difference_check(indptr, indices, h0, gamma, w, entries, eps=1e-3):
    """Central differences of L = <w, propagate(h0, gamma)> against propagate_bwd: returns (max |fd - dgamma|, max |fd - dh0| over
    `entries` = [(row, col), ...]).  L is linear in h0 and in gamma, so the differences are exact up to fp64 rounding."""
    h0 = np.asarray(h0, np.float64)
    gamma = np.asarray(gamma, np.float64)
    loss = lambda h, gm: float((w * propagate(indptr, indices, h, gm)).sum())
    dh0, dgamma = propagate_bwd(indptr, indices, w, h0, gamma)
    eg = 0.0
    for k in range(len(gamma)):
        d = np.zeros_like(gamma)
        d[k] = eps
        eg = max(eg, abs((loss(h0, gamma + d) - loss(h0, gamma - d)) / (2 * eps) - dgamma[k]))
    eh = 0.0
    for r, c in entries:
        d = np.zeros_like(h0)
        d[r, c] = eps
        eh = max(eh, abs((loss(h0 + d, gamma) - loss(h0 - d, gamma)) / (2 * eps) - dh0[r, c]))
    return eg, eh


def trunk_forward(params, x, num_layers, norm_type, bn_state=None, training=False, masks=None, p=0.0, eps=1e-5, momentum=0.1):
    """APPNP's MLP trunk: Linear -> norm -> ReLU -> dropout on hidden layers, a linear last layer.  masks: per hidden layer a uint8
    [n, hidden] keep-mask (training with dropout p; kept elements are scaled by 1 / (1 - p)), or None.  params: {'encoder.layers.i.weight':
    [out, in], ...}.  Returns (h_list, logits, cache) in fp64; cache feeds trunk_backward."""
    h = np.asarray(x, np.float64)
    h_list, cache = [], []
    for l in range(num_layers):
        w, b = params[f"encoder.layers.{l}.weight"], params[f"encoder.layers.{l}.bias"]
        z = h @ w.T + b
        if l == num_layers - 1:
            cache.append((h, None, None, None))
            return h_list, z, cache
        h_list.append(z)
        st = None
        if norm_type == "batch":
            gm, bt = params[f"encoder.norms.{l}.weight"], params[f"encoder.norms.{l}.bias"]
            if training:
                mu, var = z.mean(0), z.var(0)
                if bn_state is not None:
                    m = z.shape[0]
                    bn_state[l] = ((1 - momentum) * bn_state[l][0] + momentum * mu, (1 - momentum) * bn_state[l][1] + momentum * var * m / (m - 1))
            else:
                mu, var = bn_state[l]
            rs = 1.0 / np.sqrt(var + eps)
            xh = (z - mu) * rs
            y = xh * gm + bt
            st = ("batch", xh, rs, gm)
        elif norm_type == "layer":
            gm, bt = params[f"encoder.norms.{l}.weight"], params[f"encoder.norms.{l}.bias"]
            mu, var = z.mean(1, keepdims=True), z.var(1, keepdims=True)
            rs = 1.0 / np.sqrt(var + eps)
            xh = (z - mu) * rs
            y = xh * gm + bt
            st = ("layer", xh, rs, gm)
        else:
            y = z
        keep = None
        if training and masks is not None and p > 0:
            keep = masks[l].astype(np.float64) / (1.0 - p)
        cache.append((h, y, st, keep))
        h = np.maximum(y, 0.0)
        if keep is not None:
            h = h * keep
    raise AssertionError("unreachable")


def trunk_backward(params, cache, dlogits, num_layers):
    """Gradients of the trunk (training-mode batch statistics) for dL/dlogits: {param name: grad}."""
    grads = {}
    dz = dlogits
    for l in range(num_layers - 1, -1, -1):
        h_in = cache[l][0]
        grads[f"encoder.layers.{l}.weight"] = dz.T @ h_in
        grads[f"encoder.layers.{l}.bias"] = dz.sum(0)
        if l == 0:
            break
        dh = dz @ params[f"encoder.layers.{l}.weight"]
        _, y, st, keep = cache[l - 1]
        if keep is not None:
            dh = dh * keep
        dy = dh * (y > 0)
        if st is None:
            dz = dy
            continue
        kind, xh, rs, gm = st
        grads[f"encoder.norms.{l - 1}.weight"] = (dy * xh).sum(0)
        grads[f"encoder.norms.{l - 1}.bias"] = dy.sum(0)
        dxh = dy * gm
        ax = 0 if kind == "batch" else 1
        dz = rs * (dxh - dxh.mean(ax, keepdims=True) - xh * (dxh * xh).mean(ax, keepdims=True))
    return grads


GAMMA = "encoder.propagate.gamma"


def model_forward(params, bn_state, indptr, indices, x, num_layers, norm_type):
    """Eval-mode logits of the L-layer model (running statistics, no dropout)."""
    _, h0, _ = trunk_forward(params, x, num_layers, norm_type, bn_state, training=False)
    return propagate(indptr, indices, h0, params[GAMMA])


def loss_and_grads(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, masks=None, p=0.0):
    """One training-mode forward + backward: (loss, {param name: grad}, gamma's included); bn_state is updated in place."""
    _, h0, cache = trunk_forward(params, x, num_layers, norm_type, bn_state, training=True, masks=masks, p=p)
    logits = propagate(indptr, indices, h0, params[GAMMA])
    loss, gl = nll_and_grad(logits, labels, idx)
    dh0, dgamma = propagate_bwd(indptr, indices, gl, h0, params[GAMMA])
    grads = trunk_backward(params, cache, dh0, num_layers)
    grads[GAMMA] = dgamma
    return loss, grads


def train_steps(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, masks_per_step, p, lr, wd, steps):
    """`steps` full-graph `train` steps with Adam (L2 weight decay on every parameter, gamma included, as torch.optim.Adam applies it).
    Returns (losses, grads of the first step, params, Adam state {name: (m, v)}, bn_state)."""
    params = {a: np.asarray(b, np.float64).copy() for a, b in params.items()}
    state, losses, first = {}, [], None
    for s in range(steps):
        m = None if masks_per_step is None else masks_per_step[s]
        loss, grads = loss_and_grads(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, m, p)
        if first is None:
            first = {k: v.copy() for k, v in grads.items()}
        losses.append(loss)
        adam(params, grads, state, s + 1, lr, wd)
    return np.asarray(losses), first, params, state, bn_state
