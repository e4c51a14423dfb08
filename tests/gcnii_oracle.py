"""fp64 numpy restatement of GCNII (Chen et al., ICML 2020; docs/GCNII_SEMANTICS.md): one conv layer over APPNP's operator
P = D_in^-1/2 A D_out^-1/2, the L-layer stack, their explicit backward, the model (every dropout mask an INPUT) and training steps with
Adam.  Neither the reference nor dgl 0.6.1 defines this model: this file and the identity with tests/appnp_oracle.py at lamda = 0
(tests/test_gcnii_cpu.py) are what pins the arithmetic."""
import numpy as np

from appnp_oracle import adam, nll_and_grad
from gpr_oracle import step as prop, step_t as prop_t

FC_IN_W, FC_IN_B, FC_OUT_W, FC_OUT_B = "encoder.fc_in.weight", "encoder.fc_in.bias", "encoder.fc_out.weight", "encoder.fc_out.bias"


def conv_w(l):
    """The state-dict key of W_l, l = 1..L (the ModuleList counts from 0)."""
    return f"encoder.layers.{l - 1}.weight"


def betas(num_layers, lamda):
    return [float(np.log(lamda / l + 1.0)) for l in range(1, num_layers + 1)]


def _keep(mask, p):
    """The multiplier of a uint8 keep-mask under dropout p (None: the identity)."""
    return 1.0 if mask is None or p == 0 else np.asarray(mask, np.float64) / (1.0 - p)


def layer(indptr, indices, x, h0, w, alpha, beta, mask=None, p=0.0):
    """(S, Z, H) of one layer: S = (1 - alpha) P (x * keep) + alpha h0,  Z = (1 - beta) S + beta S W^T,  H = relu(Z)."""
    x, h0, w = (np.asarray(a, np.float64) for a in (x, h0, w))
    s = (1.0 - alpha) * prop(indptr, indices, x * _keep(mask, p)) + alpha * h0
    z = (1.0 - beta) * s + beta * (s @ w.T)
    return s, z, np.maximum(z, 0.0)


def layer_bwd(indptr, indices, g, h, w, alpha, beta, mask=None, p=0.0, plain=False):
    """(dZ, dS) of one layer from g: dZ = [h > 0] * keep * (g if plain else (1 - alpha) P^T g);  dS = (1 - beta) dZ + beta dZ W.
    h is the layer's saved output, mask the keep-mask of the dropout BEHIND it (keyed by the own row)."""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    t = g if plain else (1.0 - alpha) * prop_t(indptr, indices, g)
    dz = (np.asarray(h) > 0) * (t * _keep(mask, p))
    return dz, (1.0 - beta) * dz + beta * (dz @ w)


def stack(indptr, indices, h0, ws, alpha, bts, masks=None, p=0.0):
    """[(S_l, Z_l, H_l)] for l = 1..L over h0 = H_0; masks[l] keys drop_l (indexable by l = 1..L), or None."""
    out, x = [], np.asarray(h0, np.float64)
    for l, w in enumerate(ws, 1):
        out.append(layer(indptr, indices, x, h0, w, alpha, bts[l - 1], None if masks is None else masks[l], p))
        x = out[-1][2]
    return out


def stack_bwd(indptr, indices, da, fwd, ws, alpha, bts, masks=None, p=0.0):
    """(dH_0, [dW_1..dW_L]) from da = dL/d drop_{L+1}(H_L); fwd = stack(...)'s result; masks[l] for l = 1..L + 1."""
    L = len(ws)
    m = lambda s: None if masks is None else masks[s]
    dws, acc, g = [None] * L, 0.0, np.asarray(da, np.float64)
    for l in range(L, 0, -1):
        s, _, h = fwd[l - 1]
        dz, ds = layer_bwd(indptr, indices, g, h, ws[l - 1], alpha, bts[l - 1], m(l + 1), p, plain=l == L)
        dws[l - 1] = bts[l - 1] * (dz.T @ s)
        acc = acc + alpha * ds
        g = ds
    return (1.0 - alpha) * prop_t(indptr, indices, g) * _keep(m(1), p) + acc, dws


def model_forward(params, indptr, indices, x, num_layers, alpha, lamda, masks=None, p=0.0):
    """(logits, cache): masks[s] for the dropout sites s = 0..L + 1 (None: eval).  cache feeds model_backward and lists every
    pre-activation (Z_0 = fc_in's output, Z_1..Z_L)."""
    m = lambda s: None if masks is None else masks[s]
    xd = np.asarray(x, np.float64) * _keep(m(0), p)
    z0 = xd @ params[FC_IN_W].T + params[FC_IN_B]
    h0 = np.maximum(z0, 0.0)
    ws = [params[conv_w(l)] for l in range(1, num_layers + 1)]
    bts = betas(num_layers, lamda)
    fwd = stack(indptr, indices, h0, ws, alpha, bts, masks, p)
    a = fwd[-1][2] * _keep(m(num_layers + 1), p)
    logits = a @ params[FC_OUT_W].T + params[FC_OUT_B]
    return logits, dict(xd=xd, z0=z0, h0=h0, fwd=fwd, a=a, ws=ws, bts=bts, pre=[z0] + [f[1] for f in fwd], hs=[f[2] for f in fwd])


def model_backward(params, indptr, indices, cache, dlogits, alpha, masks=None, p=0.0):
    grads = {FC_OUT_W: dlogits.T @ cache["a"], FC_OUT_B: dlogits.sum(0)}
    dh0, dws = stack_bwd(indptr, indices, dlogits @ params[FC_OUT_W], cache["fwd"], cache["ws"], alpha, cache["bts"], masks, p)
    for l, dw in enumerate(dws, 1):
        grads[conv_w(l)] = dw
    dz0 = dh0 * (cache["z0"] > 0)
    grads[FC_IN_W], grads[FC_IN_B] = dz0.T @ cache["xd"], dz0.sum(0)
    return grads


def loss_and_grads(params, indptr, indices, x, labels, idx, num_layers, alpha, lamda, masks=None, p=0.0):
    logits, cache = model_forward(params, indptr, indices, x, num_layers, alpha, lamda, masks, p)
    loss, gl = nll_and_grad(logits, labels, idx)
    return loss, model_backward(params, indptr, indices, cache, gl, alpha, masks, p), cache


def train_steps(params, indptr, indices, x, labels, idx, num_layers, alpha, lamda, masks_per_step, p, lr, wd, steps):
    """`steps` full-graph `train` steps with Adam (L2 weight decay on every parameter, one group).  Returns (losses, the first step's
    grads, params, Adam state {name: (m, v)}, the smallest |pre-activation| any step saw)."""
    params = {a: np.asarray(b, np.float64).copy() for a, b in params.items()}
    state, losses, first, min_pre = {}, [], None, np.inf
    for s in range(steps):
        m = None if masks_per_step is None else masks_per_step[s]
        loss, grads, cache = loss_and_grads(params, indptr, indices, x, labels, idx, num_layers, alpha, lamda, m, p)
        min_pre = min(min_pre, min(float(np.abs(z).min()) for z in cache["pre"]))
        if first is None:
            first = {k: v.copy() for k, v in grads.items()}
        losses.append(loss)
        adam(params, grads, state, s + 1, lr, wd)
    return np.asarray(losses), first, params, state, min_pre
