"""CPU checks of the GPR-GNN teacher: the fp64 oracle (tests/gpr_oracle.py) by hand answers, by finite differences and against the APPNP
oracle under PPR coefficients; the initialisations, the state-dict keys, the Model dispatch and its conf defaults, the exported symbols,
and the training config.  No GPU call is made here."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import appnp_oracle as ao
import gpr_oracle as go
from graphgen import csr_from_edges, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_answer_on_a_three_node_path():
    """0 -> 1 -> 2.  in-degrees (0, 1, 1), out-degrees (1, 1, 0): every norm is 1, so P is the shift and out = gamma_0 h + gamma_1 S h +
    gamma_2 S^2 h with (S h)[i] = h[i - 1]."""
    ip, ix = csr_from_edges(np.array([0, 1]), np.array([1, 2]), 3)
    h0 = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]])
    gamma = np.array([0.5, -2.0, 3.0])
    out = go.propagate(ip, ix, h0, gamma)
    want = np.array([[0.5, 5.0], [1.0 - 2.0, 10.0 - 20.0], [2.0 - 4.0 + 3.0, 20.0 - 40.0 + 30.0]])
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)
    g = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    dh0, dgamma = go.propagate_bwd(ip, ix, g, h0, gamma)
    # G_1 = S^T g: rows (g[1], g[2], 0); G_2 = (g[2], 0, 0)
    g1 = np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 0.0]])
    g2 = np.array([[1.0, 1.0], [0.0, 0.0], [0.0, 0.0]])
    np.testing.assert_allclose(dh0, 0.5 * g - 2.0 * g1 + 3.0 * g2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dgamma, [(g * h0).sum(), (g1 * h0).sum(), (g2 * h0).sum()], rtol=0, atol=1e-12)


def test_hand_answer_on_a_multi_edge_and_an_isolated_row():
    """Edges 0 -> 1 twice and 2 -> 1 once; row 0 and row 2 have no in-edge.  in_deg (0, 3, 0) -> dst_norm (1, 3^-1/2, 1); out_deg (2, 0, 1)
    -> src_norm (2^-1/2, 1, 1).  H_1[1] = 3^-1/2 (2 * 2^-1/2 h[0] + h[2]): the multi-edge counts twice; H_1[0] = H_1[2] = 0 and H_2 = 0."""
    ip, ix = csr_from_edges(np.array([0, 0, 2]), np.array([1, 1, 1]), 3)
    h0 = np.array([[3.0], [5.0], [7.0]])
    gamma = np.array([1.0, 2.0, 4.0])
    h1 = (2.0 * 3.0 / np.sqrt(2.0) + 7.0) / np.sqrt(3.0)
    np.testing.assert_allclose(go.propagate(ip, ix, h0, gamma), [[3.0], [5.0 + 2.0 * h1], [7.0]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(go.step(ip, ix, go.step(ip, ix, h0)), 0.0, atol=0)
    dh0, dgamma = go.propagate_bwd(ip, ix, np.array([[0.0], [1.0], [0.0]]), h0, gamma)
    # G_1 = P^T e_1: row 0 gets 2 * 2^-1/2 * 3^-1/2, row 2 gets 3^-1/2; G_2 = 0
    np.testing.assert_allclose(dh0, [[2.0 * 2.0 / np.sqrt(6.0)], [1.0], [2.0 / np.sqrt(3.0)]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dgamma, [5.0, h1, 0.0], rtol=0, atol=1e-12)


def test_oracle_backward_matches_finite_differences():
    ip, ix = random_graph(40, 3, seed=2, power=0.6, isolated=3, hub=20)
    rs = np.random.RandomState(0)
    h0, w = rs.standard_normal((40, 5)), rs.standard_normal((40, 5))
    gamma = rs.uniform(-1, 1, 7)
    eg, eh = go.finite_difference_check(ip, ix, h0, gamma, w, [(0, 0), (7, 3), (39, 4), (13, 1)])
    assert eg < 1e-9 and eh < 1e-9, (eg, eh)


@pytest.mark.parametrize("k,alpha", [(0, 0.1), (1, 0.5), (10, 0.1), (4, 1.0)])
def test_ppr_coefficients_reproduce_the_appnp_oracle(k, alpha):
    """The identity that ties this oracle to arithmetic the reference's golden already pins: forward and dL/dh0."""
    ip, ix = random_graph(60, 4, seed=5, power=0.6, isolated=4, hub=30)
    rs = np.random.RandomState(k)
    h0, g = rs.standard_normal((60, 6)), rs.standard_normal((60, 6))
    gamma = go.ppr_gamma(k, alpha)
    np.testing.assert_allclose(gamma.sum(), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(go.propagate(ip, ix, h0, gamma), ao.propagate(ip, ix, h0, k, alpha, None, 0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(go.propagate_bwd(ip, ix, g, h0, gamma)[0], ao.propagate_bwd(ip, ix, g, k, alpha, None, 0), rtol=1e-12,
                               atol=1e-12)


def test_oracle_model_gradients_match_torch_autograd():
    """The L-layer oracle (trunk with dropout masks, propagation, NLL) against torch autograd on a dense fp64 restatement."""
    n, dims, k, p = 30, (7, 9, 4), 3, 0.5
    ip, ix = random_graph(n, 3, seed=8, power=0.5, isolated=2)
    rs = np.random.RandomState(1)
    x = rs.standard_normal((n, dims[0]))
    labels, idx = rs.randint(0, dims[2], n), np.arange(0, n, 2)
    params = {"encoder.layers.0.weight": rs.standard_normal((dims[1], dims[0])) * 0.3, "encoder.layers.0.bias": rs.standard_normal(dims[1]) * 0.1,
              "encoder.layers.1.weight": rs.standard_normal((dims[2], dims[1])) * 0.3, "encoder.layers.1.bias": rs.standard_normal(dims[2]) * 0.1,
              "encoder.norms.0.weight": rs.uniform(0.5, 1.5, dims[1]), "encoder.norms.0.bias": rs.standard_normal(dims[1]) * 0.1,
              go.GAMMA: rs.uniform(-1, 1, k + 1)}
    mask = (rs.uniform(size=(n, dims[1])) >= p).astype(np.uint8)
    loss, grads = go.loss_and_grads(params, None, ip, ix, x, labels, idx, 2, "layer", [mask], p)
    t = {a: torch.tensor(b, dtype=torch.float64, requires_grad=True) for a, b in params.items()}
    dn, sn = ao.degree_norms(ip, ix, n)
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)), 1.0)
    pm = torch.tensor(dn[:, None] * dense * sn[None, :])
    z = torch.tensor(x) @ t["encoder.layers.0.weight"].T + t["encoder.layers.0.bias"]
    y = F.layer_norm(z, (dims[1],), t["encoder.norms.0.weight"], t["encoder.norms.0.bias"])
    h = torch.relu(y) * torch.tensor(mask / (1 - p))
    h0 = h @ t["encoder.layers.1.weight"].T + t["encoder.layers.1.bias"]
    out, hk = t[go.GAMMA][0] * h0, h0
    for j in range(1, k + 1):
        hk = pm @ hk
        out = out + t[go.GAMMA][j] * hk
    ref = F.nll_loss(out[idx].log_softmax(1), torch.tensor(labels[idx]))
    ref.backward()
    np.testing.assert_allclose(loss, ref.item(), rtol=1e-12)
    for name, g in grads.items():
        np.testing.assert_allclose(g, t[name].grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=name)


def test_the_three_initialisations():
    from glnn_amd.nn import GPRConv
    k, a = 10, 0.1
    ppr = GPRConv(k, a, "PPR").gamma.detach().double().numpy()
    np.testing.assert_allclose(ppr, go.ppr_gamma(k, a), rtol=1e-6)
    np.testing.assert_allclose(ppr.sum(), 1.0, atol=1e-6)
    nppr = GPRConv(k, a, "NPPR").gamma.detach().double().numpy()
    want = a ** np.arange(k + 1, dtype=np.float64)
    np.testing.assert_allclose(nppr, want / np.abs(want).sum(), rtol=1e-6)
    np.testing.assert_allclose(np.abs(nppr).sum(), 1.0, atol=1e-6)
    torch.manual_seed(3)
    rnd = GPRConv(k, a, "Random").gamma.detach().double().numpy()
    np.testing.assert_allclose(np.abs(rnd).sum(), 1.0, atol=1e-6)
    assert (rnd < 0).any() and (rnd > 0).any()
    torch.manual_seed(3)                                             # the draw is torch's generator's: uniform(-b, b), b = sqrt(3 / (K + 1))
    b = (3.0 / (k + 1)) ** 0.5
    raw = torch.nn.init.uniform_(torch.empty(k + 1), -b, b).double().numpy()
    np.testing.assert_allclose(rnd, raw / np.abs(raw).sum(), rtol=1e-6)
    assert GPRConv(0, a, "PPR").gamma.detach().tolist() == [1.0]
    conv = GPRConv(4, 0.5, "PPR")
    assert [n for n, _ in conv.named_parameters()] == ["gamma"] and conv.gamma.shape == (5,) and conv.gamma.dtype == torch.float32


def test_unknown_init_raises_value_error():
    from glnn_amd.models import Model
    from glnn_amd.nn import GPRConv
    with pytest.raises(ValueError):
        GPRConv(3, 0.1, "Uniform")
    with pytest.raises(ValueError):
        Model(_conf(gpr_init="ppr"))


def _conf(**extra):
    return dict(model_name="GPRGNN", num_layers=3, feat_dim=6, hidden_dim=8, label_dim=4, dropout_ratio=0.5, norm_type="batch", device="cpu",
                **extra)


def test_state_dict_keys_are_the_appnp_trunk_plus_gamma():
    from glnn_amd.models import Model
    gpr = Model(_conf())
    appnp = Model(dict(_conf(), model_name="APPNP"))
    assert set(gpr.state_dict()) == set(appnp.state_dict()) | {"encoder.propagate.gamma"}
    for key, v in appnp.state_dict().items():
        assert gpr.state_dict()[key].shape == v.shape, key
    assert gpr.state_dict()["encoder.propagate.gamma"].shape == (11,)
    # the trunk is APPNP's draw for draw: the same seed gives the same Linear weights
    torch.manual_seed(11)
    a = Model(dict(_conf(), model_name="APPNP")).state_dict()
    torch.manual_seed(11)
    b = Model(_conf()).state_dict()
    for key, v in a.items():
        assert torch.equal(v, b[key]), key


def test_model_dispatch_and_conf_defaults():
    from glnn_amd import models
    m = models.Model(_conf())
    enc = m.encoder
    assert type(enc) is models.GPRGNN and isinstance(enc, models.MLP) and m.model_name == "GPRGNN"
    assert (enc.propagate.k, enc.propagate.alpha, enc.propagate.init) == (10, 0.1, "PPR")
    assert enc.num_layers == 3 and len(enc.layers) == 3 and len(enc.norms) == 2 and enc.dropout.p == 0.5
    m = models.Model(_conf(gpr_k=4, gpr_alpha=0.5, gpr_init="NPPR"))
    assert (m.encoder.propagate.k, m.encoder.propagate.alpha, m.encoder.propagate.init) == (4, 0.5, "NPPR")
    assert m.encoder.propagate.gamma.shape == (5,)
    with pytest.raises(ValueError, match="Unknown model_name"):
        models.Model(dict(_conf(), model_name="GPR"))
    # every earlier name still builds its own encoder
    assert type(models.Model(dict(_conf(), model_name="APPNP")).encoder) is models.APPNP
    assert type(models.Model(dict(_conf(), model_name="GCN")).encoder) is models.GCN


def test_forward_refuses_cpu_tensors():
    from glnn_amd import GlnnError, ops
    x = torch.zeros(4, 4)
    ip, ix = torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(GlnnError):
        ops.gpr_prop(ip, ix, 0, x, 1, torch.ones(4), torch.ones(4), None, torch.ones(2), torch.zeros(4, 4))
    with pytest.raises(GlnnError):
        ops.gpr_fold(torch.zeros(8), 2, 4)


def test_library_exports_the_two_symbols_and_reports_bad_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    for name in ("glnn_gpr_prop_f32", "glnn_gpr_fold_f32"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES
    assert h.glnn_abi_version() == 12
    # null pointers with non-empty sizes: -1 and a message; empty inputs: a no-op; nnz >= 2^31: unsupported
    rc = h.glnn_gpr_prop_f32(None, None, 4, 4, None, 4, 4, None, None, None, None, 1, None, 4, None, 4, None, 0, None, None)
    assert rc == -1 and b"null pointer" in h.glnn_last_error()
    assert h.glnn_gpr_prop_f32(None, None, 0, 0, None, 4, 4, None, None, None, None, 1, None, 4, None, 4, None, 0, None, None) == 0
    rc = h.glnn_gpr_prop_f32(None, None, 4, 1 << 31, None, 4, 4, None, None, None, None, 1, None, 4, None, 4, None, 0, None, None)
    assert rc not in (0, -1) and b"2^31" in h.glnn_last_error()
    rc = h.glnn_gpr_fold_f32(None, 3, 100, None, None, 0, None)
    assert rc == -1 and b"null pointer" in h.glnn_last_error()
    assert h.glnn_gpr_fold_f32(None, 0, 0, None, None, 0, None) == 0
    header = open(os.path.join(ROOT, "include", "glnn_hip.h")).read()
    assert f"#define GLNN_GPR_FOLD_CHUNK {_lib.GPR_FOLD_CHUNK}\n" in header


def test_training_config():
    from glnn_amd.utils import get_training_config
    path = os.path.join(ROOT, "train.conf.yaml")
    conf = get_training_config(path, "GPRGNN", "cora")
    assert conf == {"hidden_dim": 128, "num_layers": 2, "dropout_ratio": 0.5, "weight_decay": 0.01, "model_name": "GPRGNN"}
    for ds in ("citeseer", "pubmed", "a-computer", "a-photo"):        # a GPRGNN section wherever a dataset has an APPNP section
        a, g = get_training_config(path, "APPNP", ds), get_training_config(path, "GPRGNN", ds)
        assert {k: v for k, v in g.items() if k != "model_name"} == {k: v for k, v in a.items() if k != "model_name"}
    import yaml
    full = yaml.safe_load(open(path))
    assert all(("GPRGNN" in sec) == ("APPNP" in sec) for name, sec in full.items() if name != "global")
