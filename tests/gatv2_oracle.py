"""fp64 numpy oracle of the GATv2 teacher (docs/GATV2_SEMANTICS.md): the layer forward, the explicit backward of the document's formulas,
the encoder, and the full-graph training step with Adam.  Dropout masks are ARRAYS fed by the caller (feature masks [N, in], attention
masks [E, H], 1 = kept), so the same function replays any mask, the library's counter-hash masks among them.  `dtype` (default fp64)
lets the GPU tests run the same arithmetic in fp32 as the stand-in their reduced-gradient tolerance is derived from."""
import numpy as np

from graphgen import segment_reduce


def _edges(indptr, indices):
    n = len(indptr) - 1
    return np.repeat(np.arange(n), np.diff(indptr)), np.asarray(indices).astype(np.int64)


def attn_fwd(indptr, indices, zl, zr, attn, relu, attn_mask=None, attn_p=0.0, slope=0.2, dtype=np.float64):
    """zl, zr [N, H, F], attn [H, F].  Returns (y [N, H, F] behind the activation, cache): the part the attention kernels evaluate."""
    zl, zr, at = np.asarray(zl, dtype), np.asarray(zr, dtype), np.asarray(attn, dtype)
    n, H, F = zl.shape
    dst, src = _edges(indptr, indices)
    u = zl[src] + zr[dst]                                  # [E, H, F]
    lu = np.where(u > 0, u, dtype(slope) * u)
    s = (lu * at).sum(-1)                                  # [E, H]
    mx = segment_reduce(np.maximum, s, dst, n, -np.inf)
    ex = np.exp(s - mx[dst])
    den = segment_reduce(np.add, ex, dst, n, 0.0)
    a = ex / den[dst]
    wm = np.ones_like(a) if attn_mask is None else (np.asarray(attn_mask, dtype).reshape(a.shape) / dtype(1.0 - attn_p)).astype(dtype)
    r = segment_reduce(np.add, (a * wm)[:, :, None] * zl[src], dst, n, 0.0)
    y = np.maximum(r, 0) if relu else r
    cache = dict(dst=dst, src=src, zl=zl, zr=zr, at=at, u=u, lu=lu, s=s, a=a, wm=wm, r=r, relu=relu, slope=dtype(slope),
                 lse=mx + np.log(den))
    return y, cache


def attn_bwd(c, gy):
    """gy = dL/dy [N, H F] or [N, H, F].  Returns (dzl [N, H, F], dzr, dattn [H, F], ds [E, H]): what the backward kernels write."""
    zl, a, wm, dst, src = c["zl"], c["a"], c["wm"], c["dst"], c["src"]
    n, H, F = zl.shape
    g = np.asarray(gy, zl.dtype).reshape(n, H, F)
    if c["relu"]:
        g = g * (c["r"] > 0)
    cij = wm * (g[dst] * zl[src]).sum(-1)                  # [E, H]
    D = segment_reduce(np.add, a * cij, dst, n, 0.0)        # = <g_i, r_i>
    ds = a * (cij - D[dst])
    de = ds[:, :, None] * c["at"] * np.where(c["u"] > 0, 1.0, c["slope"]).astype(zl.dtype)
    dzr = segment_reduce(np.add, de, dst, n, 0.0)
    dzl = segment_reduce(np.add, (a * wm)[:, :, None] * g[dst] + de, src, n, 0.0)
    dattn = (ds[:, :, None] * c["lu"]).sum(0)
    return dzl, dzr, dattn, ds


def layer_fwd(indptr, indices, x, p, relu, feat_mask=None, feat_p=0.0, attn_mask=None, attn_p=0.0, slope=0.2, dtype=np.float64):
    """x [N, in]; p: dict with fc_src.weight / fc_src.bias / fc_dst.weight / fc_dst.bias ([H F, in], [H F]) and attn [1, H, F].
    Returns (y [N, H F] behind the activation, cache)."""
    x = np.asarray(x, dtype)
    ws, bs = np.asarray(p["fc_src.weight"], dtype), np.asarray(p["fc_src.bias"], dtype)
    wd, bd = np.asarray(p["fc_dst.weight"], dtype), np.asarray(p["fc_dst.bias"], dtype)
    at = np.asarray(p["attn"], dtype)[0]
    H, F = at.shape
    n = x.shape[0]
    fm = np.ones_like(x) if feat_mask is None else (np.asarray(feat_mask, dtype) / dtype(1.0 - feat_p)).astype(dtype)
    h = x * fm
    zl = (h @ ws.T + bs).reshape(n, H, F)
    zr = (h @ wd.T + bd).reshape(n, H, F)
    y, c = attn_fwd(indptr, indices, zl, zr, at, relu, attn_mask, attn_p, slope, dtype)
    c.update(h=h, fm=fm, ws=ws, wd=wd)
    return y.reshape(n, H * F), c


def layer_bwd(c, gy):
    """gy = dL/dy [N, H F].  Returns (dx, grads) with grads keyed like layer_fwd's p."""
    n, H, F = c["zl"].shape
    dzl, dzr, dattn, _ = attn_bwd(c, gy)
    dzl, dzr = dzl.reshape(n, H * F), dzr.reshape(n, H * F)
    grads = {"fc_src.weight": dzl.T @ c["h"], "fc_src.bias": dzl.sum(0), "fc_dst.weight": dzr.T @ c["h"], "fc_dst.bias": dzr.sum(0),
             "attn": dattn[None]}
    dx = c["fm"] * (dzl @ c["ws"] + dzr @ c["wd"])
    return dx, grads


KEYS = ("fc_src.weight", "fc_src.bias", "fc_dst.weight", "fc_dst.bias", "attn")


def _layer_params(params, l):
    pre = f"encoder.layers.{l}."
    return {k: params[pre + k] for k in KEYS}


def model_fwd(params, indptr, indices, feats, num_layers, feat_masks=None, feat_p=0.0, attn_masks=None, attn_p=0.0):
    """params: state_dict-keyed arrays (encoder.layers.{l}.fc_src.weight | ... | attn).  Returns (h_list, logits, caches)."""
    h = np.asarray(feats, np.float64)
    h_list, caches = [], []
    for l in range(num_layers):
        h, c = layer_fwd(indptr, indices, h, _layer_params(params, l), l != num_layers - 1,
                         None if feat_masks is None else feat_masks[l], feat_p, None if attn_masks is None else attn_masks[l], attn_p)
        caches.append(c)
        if l != num_layers - 1:
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


def min_margins(caches):
    """(smallest |pre-activation| over the ReLU layers, smallest |u_ij| over all layers): no ReLU / LeakyReLU branch of a run whose
    error stays below them can flip.  A pre-activation that is 0 EXACTLY (every in-edge of the head dropped: a sum of zero weights)
    is left out: it is 0 exactly in any arithmetic, and both branches of the ReLU give 0 there."""
    pre = min((float(np.abs(c["r"][c["r"] != 0]).min()) for c in caches if c["relu"]), default=np.inf)
    return pre, min(float(np.abs(c["u"]).min()) for c in caches)


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
