"""fp64 numpy restatement of one sampled-block GraphSAGE training step with LayerNorm tails (reference models.py:87-97, 101-119 with
norm_type "layer"; train_and_eval.py:39-54): forward, NLL, an explicit backward and torch.optim.Adam (L2 decay folded into the gradient).

Blocks are (indptr, indices, n_src) triples, outermost first; masks[l] (optional) is the 0/1 keep mask of hidden layer l's dropout."""
import numpy as np

F64 = np.float64


def _agg(indptr, indices, n_src, h):
    """SAGEConv 'gcn' aggregation: (sum_{u->v} h[u] + h[v]) / (deg + 1) over the block's destinations."""
    n_dst = len(indptr) - 1
    deg = np.diff(indptr).astype(F64)
    dst = np.repeat(np.arange(n_dst), np.diff(indptr))
    s = np.zeros((n_dst, h.shape[1]), F64)
    np.add.at(s, dst, h[indices.astype(np.int64)])
    return (s + h[:n_dst]) / (deg + 1)[:, None], dst, deg


class State:
    """Parameters keyed like the reference's state_dict (encoder.layers.{l}.fc_neigh.{weight,bias}, encoder.norms.{l}.{weight,bias});
    names() is model.parameters() order (all layers, then all norms) -- the order of the Adam state."""

    def __init__(self, sd, num_layers, eps=1e-5):
        self.L, self.eps = num_layers, float(eps)
        self.p = {k: np.array(v, F64) for k, v in sd.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.step = 0

    def names(self):
        return ([f"encoder.layers.{l}.fc_neigh.{t}" for l in range(self.L) for t in ("weight", "bias")] +
                [f"encoder.norms.{l}.{t}" for l in range(self.L - 1) for t in ("weight", "bias")])

    def W(self, l):
        return self.p[f"encoder.layers.{l}.fc_neigh.weight"], self.p[f"encoder.layers.{l}.fc_neigh.bias"]

    def G(self, l):
        return self.p[f"encoder.norms.{l}.weight"], self.p[f"encoder.norms.{l}.bias"]


def forward(st, blocks, x, masks=None, p=0.0):
    """logits and the cache of the backward (training mode)."""
    h = np.asarray(x, F64)
    cache = []
    for l, (ip, ix, ns) in enumerate(blocks):
        agg, dst, deg = _agg(ip, ix, ns, h)
        w, b = st.W(l)
        z = agg @ w.T + b
        c = dict(h_in=h, agg=agg, dst=dst, deg=deg, ip=ip, ix=ix, z=z)
        if l != st.L - 1:
            g, be = st.G(l)
            mu = z.mean(1, keepdims=True)
            rstd = 1.0 / np.sqrt(((z - mu) ** 2).mean(1, keepdims=True) + st.eps)
            xh = (z - mu) * rstd
            y = xh * g + be
            keep = np.ones_like(y) if masks is None else np.asarray(masks[l], F64)
            h = np.maximum(y, 0) * keep / (1.0 - p)
            c.update(xh=xh, rstd=rstd, y=y, keep=keep)
        else:
            h = z
        cache.append(c)
    return h, cache


def loss_and_dlogits(logits, labels, lamb=1.0):
    """NLLLoss(log_softmax) (mean) and d(lamb * loss)/dlogits."""
    z = logits - logits.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1, keepdims=True))
    logp = z - lse
    n = len(labels)
    loss = -logp[np.arange(n), labels].mean()
    d = np.exp(logp)
    d[np.arange(n), labels] -= 1.0
    return loss, d * (lamb / n)


def ln_tail_backward(dh, c, g, p=0.0):
    """LayerNorm -> ReLU -> dropout backward of one hidden layer: (dz, dgamma, dbeta)."""
    dy = dh * c["keep"] / (1.0 - p) * (c["y"] > 0)
    xh, rstd = c["xh"], c["rstd"]
    dxh = dy * g
    dz = rstd * (dxh - dxh.mean(1, keepdims=True) - xh * (dxh * xh).mean(1, keepdims=True))
    return dz, (dy * xh).sum(0), dy.sum(0)


def backward(st, cache, dlogits, p=0.0):
    """Gradients keyed by parameter name."""
    grads = {}
    dz = np.asarray(dlogits, F64)
    for l in range(st.L - 1, -1, -1):
        c = cache[l]
        w, _ = st.W(l)
        grads[f"encoder.layers.{l}.fc_neigh.weight"] = dz.T @ c["agg"]
        grads[f"encoder.layers.{l}.fc_neigh.bias"] = dz.sum(0)
        if l == 0:
            break
        da = (dz @ w) / (c["deg"] + 1)[:, None]
        dh = np.zeros_like(c["h_in"])
        np.add.at(dh, c["ix"].astype(np.int64), da[c["dst"]])
        dh[:len(da)] += da
        g, _ = st.G(l - 1)
        dz, dg, db = ln_tail_backward(dh, cache[l - 1], g, p)
        grads[f"encoder.norms.{l - 1}.weight"], grads[f"encoder.norms.{l - 1}.bias"] = dg, db
    return grads


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


def step(st, blocks, x, labels, lr, weight_decay=0.0, lamb=1.0, masks=None, p=0.0):
    """One optimisation step; returns the (unscaled) loss."""
    logits, cache = forward(st, blocks, x, masks, p)
    loss, dl = loss_and_dlogits(logits, labels, lamb)
    adam(st, backward(st, cache, dl, p), lr, weight_decay)
    return loss


def train_sage(st, batches, feats, labels, lr, weight_decay=0.0):
    """One epoch of train_sage (train_and_eval.py:32-56): mean of the per-batch losses."""
    losses = [step(st, blocks, feats[inp], labels[outn], lr, weight_decay) for inp, outn, blocks in batches]
    return float(np.mean(losses))


def eval_forward(st, blocks, x):
    """Eval-mode forward (dropout off): the logits."""
    return forward(st, blocks, x)[0]


def load_golden():
    """tests/golden/sage_ln_teacher.npz (make_sage_ln_golden.py) and its batches as (input_nodes, output_nodes, blocks)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sage_ln_teacher.npz"))
    batches = []
    for b in range(3):
        blocks = [(z[f"b{b}.l{l}.indptr"], z[f"b{b}.l{l}.indices"], int(z[f"b{b}.l{l}.n_src"])) for l in range(3)]
        batches.append((z[f"b{b}.input_nodes"], z[f"b{b}.output_nodes"], blocks))
    return z, batches


def sub(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
