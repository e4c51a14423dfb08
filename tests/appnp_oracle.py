"""fp64 numpy restatement of APPNP propagation (dgl APPNPConv, reference models.py:282-344) and of its explicit backward recurrence
(docs/APPNP_SEMANTICS.md).  The edge masks are INPUTS (uint8 [K, nnz] in CSR edge order; None = no edge dropout), so the same oracle
checks the reference's recorded masks and the library's counter-hash masks."""
import numpy as np

from graphgen import segment_reduce


def degree_norms(indptr, indices, n):
    """(dst_norm, src_norm) = (in_deg.clamp(1)^-1/2, out_deg.clamp(1)^-1/2)."""
    in_deg = np.diff(indptr).astype(np.float64)
    out_deg = np.bincount(indices.astype(np.int64), minlength=n).astype(np.float64)
    return np.maximum(in_deg, 1.0) ** -0.5, np.maximum(out_deg, 1.0) ** -0.5


def _rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def _weights(masks, t, nnz, p):
    if masks is None or p == 0:
        return np.ones(nnz)
    return masks[t - 1].astype(np.float64) / (1.0 - p)


def propagate(indptr, indices, h0, k, alpha, masks=None, p=0.0):
    """h_K: for t = 1..K  h_t[i] = (1 - alpha) dst_norm[i] sum_{e = (j -> i)} w_e(t) src_norm[j] h_{t-1}[j] + alpha h0[i]."""
    n = len(indptr) - 1
    h0 = np.asarray(h0, np.float64)
    dn, sn = degree_norms(indptr, indices, n)
    dst, src = _rows(indptr), indices.astype(np.int64)
    h = h0.copy()
    for t in range(1, k + 1):
        w = _weights(masks, t, len(src), p)
        agg = segment_reduce(np.add, w[:, None] * (sn[src, None] * h[src]), dst, n, 0.0)
        h = (1 - alpha) * dn[:, None] * agg + alpha * h0
    return h


def propagate_bwd(indptr, indices, g, k, alpha, masks=None, p=0.0):
    """dL/dh0 from g = dL/dh_K:  acc = 0; for t = K..1: acc += alpha g_t; g_{t-1} = (1 - alpha) P_t^T g_t;  return g_0 + acc,
    P_t = D_in^-1/2 M_t A D_out^-1/2."""
    n = len(indptr) - 1
    dn, sn = degree_norms(indptr, indices, n)
    dst, src = _rows(indptr), indices.astype(np.int64)
    g = np.asarray(g, np.float64).copy()
    acc = np.zeros_like(g)
    for t in range(k, 0, -1):
        acc += alpha * g
        w = _weights(masks, t, len(src), p)
        nxt = segment_reduce(np.add, w[:, None] * (dn[dst, None] * g[dst]), src, n, 0.0)
        g = (1 - alpha) * sn[:, None] * nxt
    return g + acc


def trunk_forward(params, x, num_layers, norm_type, bn_state=None, training=False, eps=1e-5, momentum=0.1):
    """The MLP trunk of the reference's APPNP.forward (models.py:326-340) with dropout p = 0: Linear -> norm -> ReLU on hidden layers.
    params: {'encoder.layers.i.weight': [out, in], ...}.  Returns (h_list, logits, cache) in fp64; cache feeds trunk_backward."""
    h = np.asarray(x, np.float64)
    h_list, cache = [], []
    for l in range(num_layers):
        w, b = params[f"encoder.layers.{l}.weight"], params[f"encoder.layers.{l}.bias"]
        z = h @ w.T + b
        if l == num_layers - 1:
            cache.append((h, None, None))
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
        cache.append((h, y, st))
        h = np.maximum(y, 0.0)
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
        _, y, st = cache[l - 1]
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


def log_softmax(z):
    m = z.max(1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(1, keepdims=True))


def nll_and_grad(logits, labels, idx):
    """NLLLoss(log_softmax(logits)[idx], labels[idx]) and its gradient wrt logits (zero outside idx)."""
    lp = log_softmax(logits[idx])
    loss = -lp[np.arange(len(idx)), labels[idx]].mean()
    p = np.exp(lp)
    p[np.arange(len(idx)), labels[idx]] -= 1.0
    g = np.zeros_like(logits)
    g[idx] = p / len(idx)
    return loss, g


def adam(params, grads, state, step, lr, wd, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam (L2 weight decay folded into the gradient), in place on params / state."""
    for k, g in grads.items():
        g = g + wd * params[k]
        m, v = state.get(k, (np.zeros_like(g), np.zeros_like(g)))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        state[k] = (m, v)
        mh, vh = m / (1 - b1 ** step), v / (1 - b2 ** step)
        params[k] = params[k] - lr * mh / (np.sqrt(vh) + eps)


def train_steps(params, bn_state, indptr, indices, x, labels, idx, num_layers, norm_type, k, alpha, p, masks_per_step, lr, wd, steps):
    """`steps` reference `train` steps of APPNP with trunk dropout 0 and the given per-step edge masks ([K, nnz] each, or None).
    Returns (losses, params, bn_state)."""
    params = {a: np.asarray(b, np.float64).copy() for a, b in params.items()}
    state, losses = {}, []
    for s in range(steps):
        _, h0, cache = trunk_forward(params, x, num_layers, norm_type, bn_state, training=True)
        m = None if masks_per_step is None else masks_per_step[s]
        logits = propagate(indptr, indices, h0, k, alpha, m, p)
        loss, gl = nll_and_grad(logits, labels, idx)
        losses.append(loss)
        dh0 = propagate_bwd(indptr, indices, gl, k, alpha, m, p)
        grads = trunk_backward(params, cache, dh0, num_layers)
        adam(params, grads, state, s + 1, lr, wd)
    return np.asarray(losses), params, bn_state
