"""fp64 numpy oracle of the PNA teacher (docs/PNA_SEMANTICS.md): the mean / min / max / std aggregation with first-position arguments, the
layer forward and its explicit backward, the encoder, and the full-graph training step with Adam.  Dropout masks are ARRAYS fed by the
caller (1 = kept), so the same function replays any mask, the library's counter-hash masks among them.  `dtype` (default fp64) lets the
GPU tests run the same arithmetic in fp32 as the stand-in their reduced-gradient tolerance and their gap condition are derived from.

The gradient of max (and of min) goes to ONE edge: the first CSR position of the row that attains the value.  torch's amax autograd shares
it between ties, so nothing here goes through an autograd: the backward is written out."""
import numpy as np

from gatv2_oracle import nll                                   # NLLLoss over log_softmax and its gradient: the same for every teacher

EPS = 1e-5
LAYER_KEYS = ("pre.weight", "pre.bias", "post.weight", "post.bias")          # PNAConv's registration order


def _edges(indptr, indices):
    n = len(indptr) - 1
    return np.repeat(np.arange(n), np.diff(indptr)), np.asarray(indices).astype(np.int64)


def agg_fwd(indptr, indices, b, a=None, dtype=np.float64):
    """b [n_src, F], a [n_dst, F] or None.  Returns (S [n_dst, 4, F] = [a + mean | a + min | a + max | std], mu [n_dst, F],
    arg [n_dst, 2, F] = [argmin | argmax] as CSR positions, -1 for a row without in-edges).  A row without in-edges gets
    S = [0 | 0 | 0 | sqrt(1e-5)] and no a term."""
    b = np.asarray(b, dtype)
    n, f = len(indptr) - 1, b.shape[1]
    dst, src = _edges(indptr, indices)
    s = np.zeros((n, 4, f), dtype)
    mu = np.zeros((n, f), dtype)
    arg = np.full((n, 2, f), -1, np.int64)
    s[:, 3] = np.sqrt(dtype(EPS))
    live = np.diff(indptr) > 0
    if not live.any():
        return s, mu, arg
    starts = np.asarray(indptr[:-1])[live]                     # rows without in-edges own no entry: the live starts delimit every row
    rows = b[src]
    d = np.diff(indptr)[live].astype(dtype)[:, None]
    m = np.add.reduceat(rows, starts, axis=0) / d
    var = np.maximum(np.add.reduceat(rows * rows, starts, axis=0) / d - m * m, 0)
    mn, mx = np.minimum.reduceat(rows, starts, axis=0), np.maximum.reduceat(rows, starts, axis=0)
    full = np.zeros((n, f), dtype)
    pos = np.arange(len(src))[:, None]
    for which, ext in ((0, mn), (1, mx)):                      # the FIRST position that attains the value: the smallest among the equal ones
        full[live] = ext
        arg[live, which] = np.minimum.reduceat(np.where(rows == full[dst], pos, len(src)), starts, axis=0)
    own = 0 if a is None else np.asarray(a, dtype)[live]
    mu[live] = m
    s[live, 0], s[live, 1], s[live, 2], s[live, 3] = own + m, own + mn, own + mx, np.sqrt(var + dtype(EPS))
    return s, mu, arg


def agg_bwd(indptr, indices, ds, b, mu, sigma, arg):
    """db [n_src, F] from ds [n_dst, 4, F] = [g_mean | g_min | g_max | g_std]: per edge e = (u -> v)
    g_mean[v] / d_v + g_std[v] (b[u] - mu[v]) / (d_v sigma[v]) + [argmax[v] == e] g_max[v] + [argmin[v] == e] g_min[v]."""
    b = np.asarray(b)
    dst, src = _edges(indptr, indices)
    d = np.diff(indptr).astype(b.dtype)[dst][:, None]
    e = np.arange(len(src))[:, None]
    ds = np.asarray(ds, b.dtype)
    term = (ds[dst, 0] / d + ds[dst, 3] * (b[src] - mu[dst]) / (d * sigma[dst])
            + (arg[dst, 1] == e) * ds[dst, 2] + (arg[dst, 0] == e) * ds[dst, 1])
    db = np.zeros_like(b)
    np.add.at(db, src, term)
    return db


def scalers(indptr, delta, dtype=np.float64):
    """(s_amp, s_att) [n, 1]: log(max(deg, 1) + 1) / delta and its reciprocal."""
    lg = np.log(np.maximum(np.diff(indptr), 1).astype(dtype) + dtype(1))[:, None]
    return lg / dtype(delta), dtype(delta) / lg


def layer_fwd(indptr, indices, x, p, delta, relu, feat_mask=None, feat_p=0.0, dtype=np.float64):
    """x [N, F]; p: dict keyed by LAYER_KEYS (pre.weight [F, 2F] = [W_dst | W_src], post.weight [Fo, 13F]).  Returns (y [N, Fo] behind the
    activation, cache)."""
    x = np.asarray(x, dtype)
    n, f = x.shape
    wp, bp, wo, bo = (np.asarray(p[k], dtype) for k in LAYER_KEYS)
    fm = np.ones_like(x) if feat_mask is None else (np.asarray(feat_mask, dtype) / dtype(1.0 - feat_p)).astype(dtype)
    h = x * fm
    a = h @ wp[:, :f].T + bp
    b = h @ wp[:, f:].T
    s, mu, arg = agg_fwd(indptr, indices, b, a, dtype)
    amp, att = scalers(indptr, delta, dtype)
    s2 = s.reshape(n, 4 * f)
    cat = np.concatenate([h, s2, amp * s2, att * s2], 1)
    r = cat @ wo.T + bo
    y = np.maximum(r, 0) if relu else r
    return y, dict(indptr=indptr, indices=indices, h=h, fm=fm, b=b, s=s, mu=mu, arg=arg, amp=amp, att=att, cat=cat, r=r, relu=relu, wp=wp,
                   wo=wo, f=f)


def layer_bwd(c, gy):
    """gy = dL/dy [N, Fo].  Returns (dx, grads keyed by LAYER_KEYS)."""
    f, h = c["f"], c["h"]
    n = h.shape[0]
    g = np.asarray(gy, h.dtype)
    if c["relu"]:
        g = g * (c["r"] > 0)
    dcat = g @ c["wo"]
    dt = dcat[:, f:].reshape(n, 3, 4, f)
    ds = dt[:, 0] + c["amp"][:, :, None] * dt[:, 1] + c["att"][:, :, None] * dt[:, 2]          # [n, 4, f]
    has = (np.diff(c["indptr"]) > 0)[:, None]
    da = (ds[:, 0] + ds[:, 1] + ds[:, 2]) * has
    db = agg_bwd(c["indptr"], c["indices"], ds, c["b"], c["mu"], c["s"][:, 3], c["arg"])
    grads = {"post.weight": g.T @ c["cat"], "post.bias": g.sum(0), "pre.weight": np.concatenate([da.T @ h, db.T @ h], 1),
             "pre.bias": da.sum(0)}
    dh = dcat[:, :f] + da @ c["wp"][:, :f] + db @ c["wp"][:, f:]
    return c["fm"] * dh, grads


def _layer_params(params, l):
    return {k: params[f"encoder.layers.{l}.{k}"] for k in LAYER_KEYS}


def _mask(masks, site, like, p, dtype):
    return np.ones_like(like) if masks is None else (np.asarray(masks[site], dtype) / dtype(1.0 - p)).astype(dtype)


def model_fwd(params, indptr, indices, feats, num_layers, delta, masks=None, p=0.0, dtype=np.float64):
    """params: state_dict-keyed arrays (encoder.fc_in.* | encoder.layers.{l}.pre.* | .post.* | encoder.fc_out.*).  masks: L + 2 keep masks
    (site 0: the input [N, feat], sites 1..L: in front of conv l [N, hidden], site L + 1: in front of fc_out).  Returns
    (h_list = [H_1..H_L], logits, cache)."""
    x = np.asarray(feats, dtype)
    w = lambda k: np.asarray(params[k], dtype)
    m0 = _mask(masks, 0, x, p, dtype)
    xd = x * m0
    z0 = xd @ w("encoder.fc_in.weight").T + w("encoder.fc_in.bias")
    h = np.maximum(z0, 0)
    hs, caches = [], []
    for l in range(num_layers):
        h, c = layer_fwd(indptr, indices, h, _layer_params(params, l), delta, True, None if masks is None else masks[l + 1], p, dtype)
        hs.append(h)
        caches.append(c)
    ml = _mask(masks, num_layers + 1, h, p, dtype)
    hd = h * ml
    logits = hd @ w("encoder.fc_out.weight").T + w("encoder.fc_out.bias")
    return hs, logits, dict(xd=xd, z0=z0, layers=caches, ml=ml, hd=hd, w_out=w("encoder.fc_out.weight"), w_in=w("encoder.fc_in.weight"), m0=m0)


def model_bwd(c, dlogits):
    """Returns (grads keyed like the state_dict, dx)."""
    grads = {"encoder.fc_out.weight": dlogits.T @ c["hd"], "encoder.fc_out.bias": dlogits.sum(0)}
    g = (dlogits @ c["w_out"]) * c["ml"]
    for l in range(len(c["layers"]) - 1, -1, -1):
        g, gl = layer_bwd(c["layers"][l], g)
        for k, v in gl.items():
            grads[f"encoder.layers.{l}.{k}"] = v
    dz0 = g * (c["z0"] > 0)
    grads["encoder.fc_in.weight"] = dz0.T @ c["xd"]
    grads["encoder.fc_in.bias"] = dz0.sum(0)
    return grads, (dz0 @ c["w_in"]) * c["m0"]


def loss_grads(params, indptr, indices, feats, labels, idx, num_layers, delta, masks=None, p=0.0, dtype=np.float64):
    _, logits, c = model_fwd(params, indptr, indices, feats, num_layers, delta, masks, p, dtype)
    loss, dlog = nll(logits, labels, idx)
    grads, dx = model_bwd(c, dlog)
    return loss, grads, logits, c, dx


def min_gap(layer_caches):
    """The smallest relative gap, over the given layer caches, rows and columns, between the winning value of max (and of min) and the best
    value of a DIFFERENT source, relative to the layer's max |b|: an argument can flip only where two sources' values are closer than the
    rounding of b.  A row whose in-edges all come from one source has no such rival (a flip between its duplicates moves no gradient: the
    source is the same).  inf when no row has a rival."""
    best = np.inf
    for c in layer_caches:
        b, indptr, src = c["b"], c["indptr"], np.asarray(c["indices"]).astype(np.int64)
        scale = float(np.abs(b).max()) or 1.0
        for v in range(len(indptr) - 1):
            e0, e1 = int(indptr[v]), int(indptr[v + 1])
            if e1 - e0 < 2:
                continue
            s = src[e0:e1]
            rows = b[s]
            for sign, which in ((-1.0, 0), (1.0, 1)):
                win = c["arg"][v, which] - e0                                   # [f] positions inside the row
                cols = np.arange(rows.shape[1])
                rival = s[:, None] != s[win][None, :]                           # [deg, f]: entries of another source than the winner's
                if not rival.any():
                    continue
                vals = np.where(rival, sign * rows, -np.inf)
                gap = sign * rows[win, cols] - vals.max(0)
                gap = gap[np.isfinite(gap)]
                if gap.size:
                    best = min(best, float(gap.min()) / scale)
    return best


def min_margin(cache):
    """The smallest |pre-activation| in front of a ReLU (fc_in's output and every conv layer's) of a model_fwd cache: no ReLU branch of a
    run whose error stays below it can flip.  A pre-activation that is 0 EXACTLY is left out: both branches give 0 there."""
    pre = [cache["z0"]] + [c["r"] for c in cache["layers"] if c["relu"]]
    return min(float(np.abs(r[r != 0]).min()) for r in pre)


def b_distance(caches64, caches32):
    """The largest distance between the layers' b computed in fp32 and in fp64, relative to the layer's max |b| (min_gap's scale)."""
    return max(float(np.abs(c32["b"].astype(np.float64) - c64["b"]).max() / (np.abs(c64["b"]).max() or 1.0))
               for c64, c32 in zip(caches64, caches32))


def train_steps(params, indptr, indices, feats, labels, idx, num_layers, delta, masks, p, lr, wd, steps, dtype=np.float64):
    """`steps` full-graph steps of torch.optim.Adam(lr, weight_decay=wd); masks: per step the L + 2 site masks (or None).  Returns
    (losses, params, exp_avg, exp_avg_sq, first-step gradients, per-step layer caches)."""
    pr = {k: np.asarray(v, dtype).copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in pr.items()}
    v2 = {k: np.zeros_like(v) for k, v in pr.items()}
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses, first, caches = [], None, []
    for t in range(1, steps + 1):
        loss, grads, _, c, _ = loss_grads(pr, indptr, indices, feats, labels, idx, num_layers, delta, None if masks is None else masks[t - 1],
                                          p, dtype)
        losses.append(loss)
        caches.append(c["layers"])
        if first is None:
            first = {k: g.copy() for k, g in grads.items()}
        for k in pr:
            g = grads[k].reshape(pr[k].shape) + wd * pr[k]
            m[k] = b1 * m[k] + (1 - b1) * g
            v2[k] = b2 * v2[k] + (1 - b2) * g * g
            pr[k] = pr[k] - lr / (1 - b1 ** t) * m[k] / (np.sqrt(v2[k]) / np.sqrt(1 - b2 ** t) + eps)
    return np.asarray(losses), pr, m, v2, first, caches


def random_params(rs, num_layers, feat_dim, hidden, label_dim, dtype=np.float32):
    """State-dict-keyed random parameters of models.PNA (no delta: a buffer, not a parameter)."""
    def lin(out_f, in_f):
        return (rs.standard_normal((out_f, in_f)) / np.sqrt(in_f)).astype(dtype), (rs.standard_normal(out_f) * 0.1).astype(dtype)
    p = {}
    p["encoder.fc_in.weight"], p["encoder.fc_in.bias"] = lin(hidden, feat_dim)
    for l in range(num_layers):
        p[f"encoder.layers.{l}.pre.weight"], p[f"encoder.layers.{l}.pre.bias"] = lin(hidden, 2 * hidden)
        p[f"encoder.layers.{l}.post.weight"], p[f"encoder.layers.{l}.post.bias"] = lin(hidden, 13 * hidden)
    p["encoder.fc_out.weight"], p["encoder.fc_out.bias"] = lin(label_dim, hidden)
    return p


def fd_check(params, indptr, indices, feats, labels, idx, num_layers, delta, h=1e-6, per_tensor=6, seed=0):
    """Central finite differences of the loss against loss_grads' explicit backward on `per_tensor` random entries of every parameter and
    of x.  Returns the largest |fd - analytic| / max(1e-6, |analytic|, |fd|).  Meaningful only where min_gap is large against h."""
    rs = np.random.RandomState(seed)
    p64 = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
    x64 = np.asarray(feats, np.float64).copy()
    _, grads, _, _, dx = loss_grads(p64, indptr, indices, x64, labels, idx, num_layers, delta)
    worst = 0.0
    loss_of = lambda: loss_grads(p64, indptr, indices, x64, labels, idx, num_layers, delta)[0]
    for arr, an in [(p64[k], grads[k].reshape(p64[k].shape)) for k in p64] + [(x64, dx)]:
        flat, fa = arr.reshape(-1), an.reshape(-1)
        for i in rs.choice(flat.size, min(per_tensor, flat.size), replace=False):
            keep = flat[i]
            flat[i] = keep + h
            up = loss_of()
            flat[i] = keep - h
            dn = loss_of()
            flat[i] = keep
            fd = (up - dn) / (2 * h)
            worst = max(worst, abs(fd - fa[i]) / max(1e-6, abs(fa[i]), abs(fd)))
    return worst
