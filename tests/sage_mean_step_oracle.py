"""What tests/sage_mean_oracle.py lacks for the native SAGE "mean" training step (TeacherEngine.step_sage_mean): dropout behind the hidden
tails, GIVEN the keep-masks (torch's Philox stream cannot be reproduced by a kernel, so parity under dropout is stated with the masks as an
input -- oracle/dropout_mask.keep_mask(rows, cols, p, seed) restates the library's counter-based mask):

    h_{l+1} = relu(norm(z_l)) * mask_l / (1 - p)          mask_l [n_dst_l, dims[l+1]], 1 = kept

forward / backward / step mirror the functions of the same names in sage_mean_oracle; with all-ones masks and p = 0 they ARE those
functions (test_sage_mean_step_cpu.py holds them to exact equality)."""
import numpy as np

import sage_mean_oracle as mo


def forward(st, blocks, x, masks=None, p=0.0, training=True):
    """(logits, cache).  masks: one [n_dst_l, dims[l+1]] array per hidden layer (None: no dropout).  mo.forward's arithmetic, line for
    line, with the mask behind every hidden tail; BatchNorm: batch statistics and the running-statistics update when `training`."""
    dt = st.dtype
    h = np.asarray(x, dt)
    cache = []
    for l, (ip, ix, ns) in enumerate(blocks):
        n_dst = len(ip) - 1
        agg, dst, inv = mo.mean_agg(ip, ix, h, dt)
        ws, bs, wn, bn = st.W(l)
        z = h[:n_dst] @ ws.T + agg @ wn.T + (bs + bn)
        c = dict(h_in=h, agg=agg, dst=dst, inv=inv, ix=np.asarray(ix, np.int64), n_dst=n_dst, z=z)
        if l == st.L - 1:
            h = z
        else:
            y = z
            if st.norm != "none":
                g, be = st.G(l)
                if st.norm == "layer":
                    mu = z.mean(1, keepdims=True)
                    var = ((z - mu) ** 2).mean(1, keepdims=True)
                elif training:
                    rm, rv = f"encoder.norms.{l}.running_mean", f"encoder.norms.{l}.running_var"
                    mu, var = z.mean(0), z.var(0)
                    n = z.shape[0]
                    st.p[rm] = (1 - st.momentum) * st.p[rm] + st.momentum * mu
                    st.p[rv] = (1 - st.momentum) * st.p[rv] + st.momentum * var * (n / max(n - 1, 1))
                else:
                    mu, var = st.p[f"encoder.norms.{l}.running_mean"], st.p[f"encoder.norms.{l}.running_var"]
                rstd = 1.0 / np.sqrt(var + dt(st.eps))
                xh = (z - mu) * rstd
                y = xh * g + be
                c.update(xh=xh, rstd=rstd)
            h = np.maximum(y, 0)
            c.update(y=y)
            if masks is not None:
                c["drop"] = np.asarray(masks[l], dt) * dt(1.0 / (1.0 - p))
                h = h * c["drop"]
        cache.append(c)
    return h, cache


def backward(st, cache, dlogits):
    """(gradients keyed by parameter name, gradient with respect to the input rows) -- mo.backward with the dropout scale in the tails."""
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
        prev = cache[l - 1]
        if "drop" in prev:
            dh = dh * prev["drop"]
        dz, gn = mo.tail_backward(st, dh, prev, l - 1)
        grads.update(gn)
    return grads, dh


def step(st, blocks, x, labels, lr, masks=None, p=0.0, weight_decay=0.0, lamb=1.0):
    """One optimisation step under the given masks; returns (the unscaled loss, the gradients, the input gradient)."""
    logits, cache = forward(st, blocks, x, masks, p, training=True)
    loss, dl = mo.loss_and_dlogits(logits, labels, lamb)
    grads, dx = backward(st, cache, dl)
    mo.adam(st, grads, lr, weight_decay)
    return loss, grads, dx
