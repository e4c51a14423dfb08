"""CPU checks of the LayerNorm SAGE teacher's fixture and fp64 oracle (tests/sage_ln_oracle.py): the golden the reference's own
train_sage produced has the promised features, the oracle reproduces it, and the oracle's explicit backward equals torch autograd."""
import numpy as np
import pytest
import torch

import sage_ln_oracle as so


def test_golden_has_the_promised_features():
    z, batches = so.load_golden()
    dims = [int(d) for d in z["dims"]]
    assert len(dims) == 4 and any(d % 4 for d in dims[1:-1])                 # 3 layers, a hidden width that is not a multiple of 4
    degs = [np.diff(ip) for _, _, blks in batches for ip, _, _ in blks]
    assert max(int(d.max()) for d in degs) > 128                             # a hub row above the long-row threshold
    assert any((d == 0).any() for d in degs)                                 # a destination with no in-edges
    assert z["epoch_losses"].shape == (2,) and z["step_losses"].shape == (6,) and int(z["adam_step"]) == 6
    assert z["eval_logits_b0"].shape == (len(batches[0][1]), dims[-1])
    for l in range(2):
        assert not np.allclose(z[f"init.encoder.norms.{l}.weight"], 1.0)    # LayerNorm affine away from its initialisation


def test_oracle_reproduces_the_reference_training():
    z, batches = so.load_golden()
    st = so.State(so.sub(z, "init."), 3, float(z["eps"]))
    feats, labels = z["feats"], z["labels"]
    losses = [so.train_sage(st, batches, feats, labels, float(z["lr"]), float(z["wd"])) for _ in range(2)]
    np.testing.assert_allclose(losses, z["epoch_losses"], atol=2e-5, rtol=0)
    for k in st.names():
        np.testing.assert_allclose(st.p[k], z[f"final.{k}"], atol=2e-5, rtol=0, err_msg=k)
        np.testing.assert_allclose(st.m[k], z[f"exp_avg.{k}"], atol=2e-6, rtol=0, err_msg=k)
        np.testing.assert_allclose(st.v[k], z[f"exp_avg_sq.{k}"], atol=1e-8, rtol=1e-3, err_msg=k)
    inp, _, blks = batches[0]
    np.testing.assert_allclose(so.eval_forward(st, blks, feats[inp]), z["eval_logits_b0"], atol=5e-5, rtol=0)


def _torch_grads(st, blocks, x, labels, masks, p):
    """The same step through float64 torch autograd."""
    P = {k: torch.tensor(v, requires_grad=True) for k, v in st.p.items()}
    h = torch.tensor(x)
    for l, (ip, ix, ns) in enumerate(blocks):
        n_dst = len(ip) - 1
        dst = torch.from_numpy(np.repeat(np.arange(n_dst), np.diff(ip)))
        s = torch.zeros(n_dst, h.shape[1], dtype=torch.float64).index_add(0, dst, h[torch.from_numpy(ix.astype(np.int64))])
        agg = (s + h[:n_dst]) / torch.from_numpy(np.diff(ip) + 1.0)[:, None]
        zz = agg @ P[f"encoder.layers.{l}.fc_neigh.weight"].T + P[f"encoder.layers.{l}.fc_neigh.bias"]
        if l != len(blocks) - 1:
            y = torch.nn.functional.layer_norm(zz, (zz.shape[1],), P[f"encoder.norms.{l}.weight"], P[f"encoder.norms.{l}.bias"], st.eps)
            h = torch.relu(y) * torch.from_numpy(masks[l]) / (1 - p)
        else:
            h = zz
    loss = torch.nn.functional.nll_loss(h.log_softmax(1), torch.from_numpy(labels))
    loss.backward()
    return loss.item(), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("seed,p,const_row", [(0, 0.0, False), (1, 0.5, False), (2, 0.3, True), (3, 0.0, True)])
def test_oracle_backward_matches_torch_autograd(seed, p, const_row):
    z, batches = so.load_golden()
    rs = np.random.RandomState(seed)
    dims = [int(d) for d in z["dims"]]
    inp, outn, blks = batches[seed % 3]
    st = so.State(so.sub(z, "init."), 3, float(z["eps"]))
    for k in st.names():
        st.p[k] = st.p[k] + rs.standard_normal(st.p[k].shape) * 0.05
    x = z["feats"][inp].astype(np.float64)
    if const_row:
        # a constant z row of layer 0 (rstd = 1/sqrt(eps)): a destination whose aggregate is all zeros, with a zero bias there
        st.p["encoder.layers.0.fc_neigh.bias"][:] = 0.3
        x_rows = np.flatnonzero(np.diff(blks[0][0]) == 0)
        assert len(x_rows)
        x[x_rows] = 0.0
    masks = [(rs.random_sample((len(blks[l][0]) - 1, dims[l + 1])) >= p).astype(np.float64) for l in range(2)]
    logits, cache = so.forward(st, blks, x, masks, p)
    if const_row:
        r = cache[0]["rstd"][x_rows, 0]
        np.testing.assert_allclose(r, 1 / np.sqrt(st.eps), rtol=1e-6)
    loss, dl = so.loss_and_dlogits(logits, z["labels"][outn])
    grads = so.backward(st, cache, dl, p)
    tloss, tgrads = _torch_grads(st, blks, x, z["labels"][outn], masks, p)
    assert abs(loss - tloss) < 1e-12
    for k in st.names():
        np.testing.assert_allclose(grads[k], tgrads[k], atol=1e-10, rtol=1e-8, err_msg=k)
