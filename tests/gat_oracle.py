"""fp64 numpy oracle of the GAT teacher (dgl 0.6.1 GATConv as docs/GAT_SEMANTICS.md restates it): the layer forward, the explicit backward
of the issue's formulas, the encoder, and the reference's full-graph training step with Adam.  Dropout masks are ARRAYS fed by the
caller (feature masks [N, in], attention masks [E, H], 1 = kept), so the same function replays the reference's recorded masks and the
library's counter-hash masks."""
import numpy as np

from graphgen import segment_reduce


def _edges(indptr, indices):
    n = len(indptr) - 1
    return np.repeat(np.arange(n), np.diff(indptr)), np.asarray(indices).astype(np.int64)


def layer_fwd(indptr, indices, x, w, attn_l, attn_r, relu, feat_mask=None, feat_p=0.0, attn_mask=None, attn_p=0.0, slope=0.2):
    """x [N, in], w [H F, in], attn_* [1, H, F].  Returns (y [N, H F] behind the activation, cache)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    al, ar = np.asarray(attn_l, np.float64)[0], np.asarray(attn_r, np.float64)[0]
    H, F = al.shape
    n = x.shape[0]
    dst, src = _edges(indptr, indices)
    fm = np.ones_like(x) if feat_mask is None else np.asarray(feat_mask, np.float64) / (1.0 - feat_p)
    h = x * fm
    z = (h @ w.T).reshape(n, H, F)
    el, er = (z * al).sum(-1), (z * ar).sum(-1)
    s = el[src] + er[dst]                                  # [E, H]
    e = np.where(s > 0, s, slope * s)
    mx = segment_reduce(np.maximum, e, dst, n, -np.inf)
    ex = np.exp(e - mx[dst])
    den = segment_reduce(np.add, ex, dst, n, 0.0)
    a = ex / den[dst]
    wm = np.ones_like(a) if attn_mask is None else np.asarray(attn_mask, np.float64).reshape(a.shape) / (1.0 - attn_p)
    r = segment_reduce(np.add, (a * wm)[:, :, None] * z[src], dst, n, 0.0)
    y = np.maximum(r, 0) if relu else r
    cache = dict(dst=dst, src=src, h=h, fm=fm, w=w, al=al, ar=ar, z=z, s=s, a=a, wm=wm, r=r, relu=relu, slope=slope,
                 lse=mx + np.log(den), el=el, er=er)
    return y.reshape(n, H * F), cache


def layer_dz(c, gy):
    """gy = dL/dy [N, H F].  Returns (dz [N, H F], dattn_l [1, H, F], dattn_r): what the attention backward kernels write."""
    n, H, F = c["z"].shape
    dst, src, z, a, wm = c["dst"], c["src"], c["z"], c["a"], c["wm"]
    g = np.asarray(gy, np.float64).reshape(n, H, F)
    if c["relu"]:
        g = g * (c["r"] > 0)
    D = (g * c["r"]).sum(-1)                                # [N, H]
    cij = wm * (g[dst] * z[src]).sum(-1)                    # [E, H]
    de = a * (cij - D[dst])
    ds = de * np.where(c["s"] > 0, 1.0, c["slope"])
    der = segment_reduce(np.add, ds, dst, n, 0.0)
    dl = segment_reduce(np.add, ds, src, n, 0.0)
    dz = segment_reduce(np.add, (a * wm)[:, :, None] * g[dst], src, n, 0.0)
    dz += dl[:, :, None] * c["al"] + der[:, :, None] * c["ar"]
    dal = (dl[:, :, None] * z).sum(0)[None]
    dar = (der[:, :, None] * z).sum(0)[None]
    return dz.reshape(n, H * F), dal, dar


def layer_bwd(c, gy):
    """gy = dL/dy [N, H F].  Returns (dx, dW, dattn_l [1, H, F], dattn_r)."""
    dz2, dal, dar = layer_dz(c, gy)
    dw = dz2.T @ c["h"]
    dx = c["fm"] * (dz2 @ c["w"])
    return dx, dw, dal, dar


def model_fwd(params, indptr, indices, feats, num_layers, feat_masks=None, feat_p=0.0, attn_masks=None, attn_p=0.0):
    """params: state_dict-keyed arrays (encoder.layers.{l}.fc.weight | attn_l | attn_r).  Returns (h_list, logits, caches)."""
    h = np.asarray(feats, np.float64)
    h_list, caches = [], []
    for l in range(num_layers):
        pre = f"encoder.layers.{l}."
        h, c = layer_fwd(indptr, indices, h, params[pre + "fc.weight"], params[pre + "attn_l"], params[pre + "attn_r"], l != num_layers - 1,
                         None if feat_masks is None else feat_masks[l], feat_p, None if attn_masks is None else attn_masks[l], attn_p)
        caches.append(c)
        if l != num_layers - 1:
            h_list.append(h)
    return h_list, h, caches


def model_bwd(caches, dlogits):
    grads = {}
    g = dlogits
    for l in range(len(caches) - 1, -1, -1):
        g, dw, dal, dar = layer_bwd(caches[l], g)
        pre = f"encoder.layers.{l}."
        grads[pre + "fc.weight"], grads[pre + "attn_l"], grads[pre + "attn_r"] = dw, dal, dar
    return grads


def nll(logits, labels, idx):
    """NLLLoss()(log_softmax(logits)[idx], labels[idx]) and its gradient with respect to ALL logits."""
    z = logits[idx]
    z = z - z.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    y = np.asarray(labels)[idx]
    loss = -logp[np.arange(len(idx)), y].mean()
    d = np.exp(logp)
    d[np.arange(len(idx)), y] -= 1.0
    full = np.zeros_like(logits)
    full[idx] = d / len(idx)
    return loss, full


def loss_grads(params, indptr, indices, feats, labels, idx, num_layers, feat_masks=None, feat_p=0.0, attn_masks=None, attn_p=0.0):
    _, logits, caches = model_fwd(params, indptr, indices, feats, num_layers, feat_masks, feat_p, attn_masks, attn_p)
    loss, dlog = nll(logits, labels, idx)
    return loss, model_bwd(caches, dlog), logits


def train_steps(params, indptr, indices, feats, labels, idx, num_layers, feat_masks, feat_p, attn_masks, attn_p, lr, wd, steps):
    """`steps` full-graph steps of torch.optim.Adam(lr, weight_decay=wd); feat_masks / attn_masks: per step, per layer.
    Returns (losses, params)."""
    p = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses = []
    for t in range(1, steps + 1):
        loss, grads, _ = loss_grads(p, indptr, indices, feats, labels, idx, num_layers, None if feat_masks is None else feat_masks[t - 1],
                                    feat_p, None if attn_masks is None else attn_masks[t - 1], attn_p)
        losses.append(loss)
        for k in p:
            g = grads[k].reshape(p[k].shape) + wd * p[k]
            m[k] = b1 * m[k] + (1 - b1) * g
            v2[k] = b2 * v2[k] + (1 - b2) * g * g
            p[k] = p[k] - lr / (1 - b1 ** t) * m[k] / (np.sqrt(v2[k]) / np.sqrt(1 - b2 ** t) + eps)
    return np.asarray(losses), p
