"""fp64 numpy oracle of the GraphTransformer teacher (docs/GT_SEMANTICS.md): the layer forward, the explicit backward of the document's
formulas, the encoder, and the full-graph training step with Adam.  Dropout masks are ARRAYS fed by the caller (feature masks [N, in],
attention masks [E, H], 1 = kept), so the same function replays any mask, the library's counter-hash masks among them.  `dtype` (default
fp64) lets the GPU tests run the same arithmetic in fp32 as the stand-in their reduced-gradient tolerance is derived from."""
import numpy as np

from gatv2_oracle import nll                                   # NLLLoss over log_softmax and its gradient: the same for every teacher
from graphgen import segment_reduce

LINS = ("lin_key", "lin_query", "lin_value", "lin_skip")       # TransformerConv's construction order
KEYS = tuple(f"{lin}.{part}" for lin in LINS for part in ("weight", "bias"))


def _edges(indptr, indices):
    n = len(indptr) - 1
    return np.repeat(np.arange(n), np.diff(indptr)), np.asarray(indices).astype(np.int64)


def attn_fwd(indptr, indices, q, k, v, skip, relu, attn_mask=None, attn_p=0.0, dtype=np.float64):
    """q, k, v, skip [N, H, D].  Returns (y [N, H, D] behind the activation, cache): the part the attention kernels evaluate."""
    q, k, v, skip = (np.asarray(t, dtype) for t in (q, k, v, skip))
    n, H, D = q.shape
    dst, src = _edges(indptr, indices)
    scale = dtype(1.0 / np.sqrt(float(D)))
    e = (q[dst] * k[src]).sum(-1) * scale                  # [E, H]
    mx = segment_reduce(np.maximum, e, dst, n, -np.inf)
    ex = np.exp(e - mx[dst])
    den = segment_reduce(np.add, ex, dst, n, 0.0)
    a = ex / den[dst]
    wm = np.ones_like(a) if attn_mask is None else (np.asarray(attn_mask, dtype).reshape(a.shape) / dtype(1.0 - attn_p)).astype(dtype)
    r = segment_reduce(np.add, (a * wm)[:, :, None] * v[src], dst, n, 0.0) + skip
    y = np.maximum(r, 0) if relu else r
    deg = np.diff(indptr)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(deg[:, None] > 0, mx + np.log(den), 0.0)          # a row without in-edges: the kernel stores 0
    cache = dict(dst=dst, src=src, q=q, k=k, v=v, e=e, a=a, wm=wm, r=r, relu=relu, scale=scale, lse=lse)
    return y, cache


def attn_bwd(c, gy):
    """gy = dL/dy [N, H D] or [N, H, D].  Returns (dq, dk, dv [N, H, D], ds = the gradient behind the activation mask [N, H, D],
    t [E, H]): what the backward kernels write, and the skip row's gradient."""
    q, k, v, a, wm, dst, src = c["q"], c["k"], c["v"], c["a"], c["wm"], c["dst"], c["src"]
    n, H, D = q.shape
    g = np.asarray(gy, q.dtype).reshape(n, H, D)
    if c["relu"]:
        g = g * (c["r"] > 0)
    cij = wm * (g[dst] * v[src]).sum(-1)                   # [E, H]
    Di = segment_reduce(np.add, a * cij, dst, n, 0.0)       # sum_k a_ik c_ik (sum_k a_ik = 1); NOT <g_i, r_i>: r holds the skip row
    t = a * (cij - Di[dst])
    dq = segment_reduce(np.add, t[:, :, None] * k[src], dst, n, 0.0) * c["scale"]
    dk = segment_reduce(np.add, t[:, :, None] * q[dst], src, n, 0.0) * c["scale"]
    dv = segment_reduce(np.add, (a * wm)[:, :, None] * g[dst], src, n, 0.0)
    return dq, dk, dv, g, t


def layer_fwd(indptr, indices, x, p, relu, feat_mask=None, feat_p=0.0, attn_mask=None, attn_p=0.0, heads=None, dtype=np.float64):
    """x [N, in]; p: dict keyed by KEYS ([H D, in] weights, [H D] biases); heads: H (default: p["heads"]).  Returns
    (y [N, H D] behind the activation, cache)."""
    x = np.asarray(x, dtype)
    H = int(p["heads"] if heads is None else heads)
    w = {lin: np.asarray(p[lin + ".weight"], dtype) for lin in LINS}
    b = {lin: np.asarray(p[lin + ".bias"], dtype) for lin in LINS}
    n = x.shape[0]
    D = w["lin_key"].shape[0] // H
    fm = np.ones_like(x) if feat_mask is None else (np.asarray(feat_mask, dtype) / dtype(1.0 - feat_p)).astype(dtype)
    h = x * fm
    z = {lin: (h @ w[lin].T + b[lin]).reshape(n, H, D) for lin in LINS}
    y, c = attn_fwd(indptr, indices, z["lin_query"], z["lin_key"], z["lin_value"], z["lin_skip"], relu, attn_mask, attn_p, dtype)
    c.update(h=h, fm=fm, w=w)
    return y.reshape(n, H * D), c


def layer_bwd(c, gy):
    """gy = dL/dy [N, H D].  Returns (dx, grads) with grads keyed by KEYS."""
    n, H, D = c["q"].shape
    dq, dk, dv, ds, _ = attn_bwd(c, gy)
    dz = {"lin_key": dk, "lin_query": dq, "lin_value": dv, "lin_skip": ds}
    grads, dh = {}, 0.0
    for lin in LINS:
        d = dz[lin].reshape(n, H * D)
        grads[lin + ".weight"] = d.T @ c["h"]
        grads[lin + ".bias"] = d.sum(0)
        dh = dh + d @ c["w"][lin]
    return c["fm"] * dh, grads


def _layer_params(params, l):
    pre = f"encoder.layers.{l}."
    return {k: params[pre + k] for k in KEYS}


def model_fwd(params, indptr, indices, feats, num_layers, num_heads, feat_masks=None, feat_p=0.0, attn_masks=None, attn_p=0.0):
    """params: state_dict-keyed arrays (encoder.layers.{l}.lin_key.weight | ...); num_heads on the hidden layers, one head on the last.
    Returns (h_list, logits, caches)."""
    h = np.asarray(feats, np.float64)
    h_list, caches = [], []
    for l in range(num_layers):
        last = l == num_layers - 1
        h, c = layer_fwd(indptr, indices, h, _layer_params(params, l), not last, None if feat_masks is None else feat_masks[l], feat_p,
                         None if attn_masks is None else attn_masks[l], attn_p, heads=1 if last else num_heads)
        caches.append(c)
        if not last:
            h_list.append(h)
    return h_list, h, caches


def model_bwd(caches, dlogits):
    grads = {}
    g = dlogits
    for l in range(len(caches) - 1, -1, -1):
        g, gl = layer_bwd(caches[l], g)
        for k, v in gl.items():
            grads[f"encoder.layers.{l}.{k}"] = v
    return grads


def loss_grads(params, indptr, indices, feats, labels, idx, num_layers, num_heads, feat_masks=None, feat_p=0.0, attn_masks=None,
               attn_p=0.0):
    _, logits, caches = model_fwd(params, indptr, indices, feats, num_layers, num_heads, feat_masks, feat_p, attn_masks, attn_p)
    loss, dlog = nll(logits, labels, idx)
    return loss, model_bwd(caches, dlog), logits


def min_margin(caches):
    """The smallest |pre-activation| over the ReLU layers: no ReLU branch of a run whose error stays below it can flip.  A
    pre-activation that is 0 EXACTLY is left out: it is 0 in any arithmetic, and both branches of the ReLU give 0 there."""
    return min((float(np.abs(c["r"][c["r"] != 0]).min()) for c in caches if c["relu"]), default=np.inf)


def train_steps(params, indptr, indices, feats, labels, idx, num_layers, num_heads, feat_masks, feat_p, attn_masks, attn_p, lr, wd,
                steps):
    """`steps` full-graph steps of torch.optim.Adam(lr, weight_decay=wd); feat_masks / attn_masks: per step, per layer.
    Returns (losses, params)."""
    p = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses = []
    for t in range(1, steps + 1):
        loss, grads, _ = loss_grads(p, indptr, indices, feats, labels, idx, num_layers, num_heads,
                                    None if feat_masks is None else feat_masks[t - 1], feat_p,
                                    None if attn_masks is None else attn_masks[t - 1], attn_p)
        losses.append(loss)
        for k in p:
            g = grads[k].reshape(p[k].shape) + wd * p[k]
            m[k] = b1 * m[k] + (1 - b1) * g
            v2[k] = b2 * v2[k] + (1 - b2) * g * g
            p[k] = p[k] - lr / (1 - b1 ** t) * m[k] / (np.sqrt(v2[k]) / np.sqrt(1 - b2 ** t) + eps)
    return np.asarray(losses), p
