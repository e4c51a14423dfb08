"""numpy restatement of the GraphSAGE "mean" aggregator (docs/SAGE_MEAN_SEMANTICS.md; dgl 0.6.1 SAGEConv(aggregator_type="mean") as
published -- the reference never builds it, so this file and the hand-computed answers of test_sage_mean_cpu.py are the pin):

  layer      h_neigh[v] = (1 / deg(v)) sum_{u->v} h_src[u]  (multi-edges count multiply, deg 0 -> 0);  out = fc_self(h_dst) + fc_neigh(h_neigh)
  forward    the L-layer forward with the hidden tails norm -> ReLU -> dropout(identity), norm in none | batch | layer, eval or training
  backward   the gradients of one training step (NLL of log_softmax, mean) with respect to every parameter and the input
  adam/step  torch.optim.Adam and one optimisation step; train_sage = one epoch

Everything runs in `dtype` (default float64).  Run in float32 the same functions are the fp32 stand-in of the same arithmetic whose
distance from the fp64 result bounds what fp32 kernels may lose on the gradient sums.  Blocks are (indptr, indices, n_src) triples, outermost
first, destination rows first among the sources."""
import numpy as np

F64 = np.float64


def mean_agg(indptr, indices, h, dtype=F64):
    """(h_neigh [n_dst, d], dst of every edge, 1 / max(deg, 1))"""
    n_dst = len(indptr) - 1
    deg = np.diff(indptr)
    dst = np.repeat(np.arange(n_dst), deg)
    s = np.zeros((n_dst, h.shape[1]), dtype)
    np.add.at(s, dst, h[np.asarray(indices, np.int64)])
    inv = (1.0 / np.maximum(deg, 1)).astype(dtype)
    return s * inv[:, None], dst, inv


def layer(indptr, indices, h_src, w_self, b_self, w_neigh, b_neigh, project_first=False, dtype=F64):
    """One SAGEConv "mean" layer over a block whose destinations are h_src[:n_dst].  project_first: dgl's in > out order -- fc_neigh before
    the aggregation (its bias after it); algebraically the same."""
    h = np.asarray(h_src, dtype)
    ws, wn = np.asarray(w_self, dtype), np.asarray(w_neigh, dtype)
    n_dst = len(indptr) - 1
    out = h[:n_dst] @ ws.T
    if project_first:
        out = out + mean_agg(indptr, indices, h @ wn.T, dtype)[0]
    else:
        out = out + mean_agg(indptr, indices, h, dtype)[0] @ wn.T
    if b_self is not None:
        out = out + np.asarray(b_self, dtype) + np.asarray(b_neigh, dtype)
    return out


class State:
    """Parameters keyed like the state_dict (encoder.layers.{l}.fc_self|fc_neigh.{weight,bias}, encoder.norms.{l}.{weight,bias} and, for
    BatchNorm, running_mean / running_var); names() is model.parameters() order -- the order of the Adam state."""

    def __init__(self, sd, num_layers, norm="none", eps=1e-5, momentum=0.1, dtype=F64):
        self.L, self.norm, self.eps, self.momentum, self.dtype = num_layers, norm, float(eps), float(momentum), dtype
        self.p = {k: np.array(v, dtype) for k, v in sd.items() if "num_batches_tracked" not in k}
        self.m = {k: np.zeros_like(self.p[k]) for k in self.names()}
        self.v = {k: np.zeros_like(self.p[k]) for k in self.names()}
        self.step = 0

    def names(self):
        out = [f"encoder.layers.{l}.{fc}.{t}" for l in range(self.L) for fc in ("fc_self", "fc_neigh") for t in ("weight", "bias")]
        if self.norm != "none":
            out += [f"encoder.norms.{l}.{t}" for l in range(self.L - 1) for t in ("weight", "bias")]
        return out

    def W(self, l):
        k = f"encoder.layers.{l}."
        return self.p[k + "fc_self.weight"], self.p[k + "fc_self.bias"], self.p[k + "fc_neigh.weight"], self.p[k + "fc_neigh.bias"]

    def G(self, l):
        return self.p[f"encoder.norms.{l}.weight"], self.p[f"encoder.norms.{l}.bias"]


def forward(st, blocks, x, training=False):
    """(logits, cache of the backward).  Hidden tails: norm -> ReLU (dropout 0).  BatchNorm: batch statistics (biased variance) and the
    running-statistics update in training mode, the running statistics in eval mode."""
    dt = st.dtype
    h = np.asarray(x, dt)
    cache = []
    for l, (ip, ix, ns) in enumerate(blocks):
        n_dst = len(ip) - 1
        agg, dst, inv = mean_agg(ip, ix, h, dt)
        ws, bs, wn, bn = st.W(l)
        z = h[:n_dst] @ ws.T + agg @ wn.T + (bs + bn)
        c = dict(h_in=h, agg=agg, dst=dst, inv=inv, ix=np.asarray(ix, np.int64), n_dst=n_dst, z=z)
        if l != st.L - 1:
            y = z
            if st.norm == "layer":
                g, be = st.G(l)
                mu = z.mean(1, keepdims=True)
                rstd = 1.0 / np.sqrt(((z - mu) ** 2).mean(1, keepdims=True) + dt(st.eps))
                xh = (z - mu) * rstd
                y = xh * g + be
                c.update(xh=xh, rstd=rstd)
            elif st.norm == "batch":
                g, be = st.G(l)
                rm, rv = f"encoder.norms.{l}.running_mean", f"encoder.norms.{l}.running_var"
                if training:
                    mu, var = z.mean(0), z.var(0)
                    n = z.shape[0]
                    st.p[rm] = (1 - st.momentum) * st.p[rm] + st.momentum * mu
                    st.p[rv] = (1 - st.momentum) * st.p[rv] + st.momentum * var * (n / max(n - 1, 1))
                else:
                    mu, var = st.p[rm], st.p[rv]
                rstd = 1.0 / np.sqrt(var + dt(st.eps))
                xh = (z - mu) * rstd
                y = xh * g + be
                c.update(xh=xh, rstd=rstd)
            h = np.maximum(y, 0)
            c.update(y=y)
        else:
            h = z
        cache.append(c)
    return h, cache


def loss_and_dlogits(logits, labels, lamb=1.0):
    """NLLLoss(log_softmax) (mean) and d(lamb * loss)/dlogits."""
    z = logits - logits.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    n = len(labels)
    loss = -logp[np.arange(n), labels].mean()
    d = np.exp(logp)
    d[np.arange(n), labels] -= 1.0
    return loss, d * logits.dtype.type(lamb / n)


def tail_backward(st, dh, c, l):
    """norm -> ReLU backward of hidden layer l (training-mode statistics): (dz, {norm parameter gradients})."""
    dy = dh * (c["y"] > 0)
    if st.norm == "none":
        return dy, {}
    g, _ = st.G(l)
    xh, rstd = c["xh"], c["rstd"]
    dxh = dy * g
    ax = 1 if st.norm == "layer" else 0
    dz = rstd * (dxh - dxh.mean(ax, keepdims=True) - xh * (dxh * xh).mean(ax, keepdims=True))
    return dz, {f"encoder.norms.{l}.weight": (dy * xh).sum(0), f"encoder.norms.{l}.bias": dy.sum(0)}


def backward(st, cache, dlogits):
    """(gradients keyed by parameter name, gradient with respect to the input rows)."""
    grads = {}
    dz = np.asarray(dlogits, st.dtype)
    dh = None
    for l in range(st.L - 1, -1, -1):
        c = cache[l]
        ws, _, wn, _ = st.W(l)
        k = f"encoder.layers.{l}."
        n_dst = c["n_dst"]
        grads[k + "fc_self.weight"] = dz.T @ c["h_in"][:n_dst]
        grads[k + "fc_neigh.weight"] = dz.T @ c["agg"]
        grads[k + "fc_self.bias"] = dz.sum(0)
        grads[k + "fc_neigh.bias"] = dz.sum(0)
        da = (dz @ wn) * c["inv"][:, None]
        dh = np.zeros_like(c["h_in"])
        np.add.at(dh, c["ix"], da[c["dst"]])
        dh[:n_dst] += dz @ ws
        if l == 0:
            break
        dz, gn = tail_backward(st, dh, cache[l - 1], l - 1)
        grads.update(gn)
    return grads, dh


def adam(st, grads, lr, weight_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam.step (amsgrad off): L2 decay added to the gradient, bias-corrected moments."""
    st.step += 1
    t = st.step
    for k in st.names():
        gr = grads[k] + weight_decay * st.p[k]
        st.m[k] = beta1 * st.m[k] + (1 - beta1) * gr
        st.v[k] = beta2 * st.v[k] + (1 - beta2) * gr * gr
        denom = np.sqrt(st.v[k]) / np.sqrt(1 - beta2 ** t) + eps
        st.p[k] = st.p[k] - (lr / (1 - beta1 ** t)) * st.m[k] / denom


def step(st, blocks, x, labels, lr, weight_decay=0.0, lamb=1.0):
    """One optimisation step; returns (the unscaled loss, the gradients, the input gradient)."""
    logits, cache = forward(st, blocks, x, training=True)
    loss, dl = loss_and_dlogits(logits, labels, lamb)
    grads, dx = backward(st, cache, dl)
    adam(st, grads, lr, weight_decay)
    return loss, grads, dx


def train_sage(st, batches, feats, labels, lr, weight_decay=0.0):
    """One epoch of train_sage (reference train_and_eval.py:32-56): (mean of the per-batch losses, the per-batch (loss, grads))."""
    per = []
    for inp, outn, blocks in batches:
        loss, grads, _ = step(st, blocks, np.asarray(feats, st.dtype)[inp], labels[outn], lr, weight_decay)
        per.append((float(loss), grads))
    return float(np.mean([l for l, _ in per])), per


def inference(st, indptr, indices, n, x):
    """The layer-wise full-neighbour eval forward over the whole graph: every layer over all n rows."""
    return forward(st, [(indptr, indices, n)] * st.L, x, training=False)[0]
