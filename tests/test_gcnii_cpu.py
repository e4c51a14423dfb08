"""CPU checks of the GCNII teacher: the fp64 oracle (tests/gcnii_oracle.py) by hand answers, by finite differences, against torch autograd
on a dense restatement and against the APPNP oracle at lamda = 0; the layer's beta and initialisation, the state-dict keys, the Model
dispatch and its conf keys, the command-line flags, the training config, the engine's seed stream, the exported symbols and every refusal.
No GPU call is made here."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import appnp_oracle as ao
import gcnii_oracle as co
from graphgen import csr_from_edges, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("identity_w", [True, False])
def test_hand_answer_on_a_three_node_path(identity_w):
    """0 -> 1 -> 2: every norm is 1 and P is the shift, (P h)[i] = h[i - 1].  S = (1 - alpha) shift(x) + alpha h0.  W = I: Z = S whatever
    beta is.  Otherwise Z = (1 - beta) S + beta S W^T with W = [[0, 2], [-1, 0]]: (S W^T)[i] = (2 S[i, 1], -S[i, 0])."""
    ip, ix = csr_from_edges(np.array([0, 1]), np.array([1, 2]), 3)
    x = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]])
    h0 = np.array([[1.0, -1.0], [0.5, 0.5], [-2.0, 2.0]])
    alpha, beta = 0.25, 0.5
    w = np.eye(2) if identity_w else np.array([[0.0, 2.0], [-1.0, 0.0]])
    s, z, h = co.layer(ip, ix, x, h0, w, alpha, beta)
    want_s = 0.75 * np.array([[0.0, 0.0], [1.0, 10.0], [2.0, 20.0]]) + 0.25 * h0
    np.testing.assert_allclose(s, want_s, rtol=0, atol=1e-12)
    want_z = want_s if identity_w else 0.5 * want_s + 0.5 * np.stack([2.0 * want_s[:, 1], -want_s[:, 0]], 1)
    np.testing.assert_allclose(z, want_z, rtol=0, atol=1e-12)
    np.testing.assert_allclose(h, np.maximum(want_z, 0.0), rtol=0, atol=1e-12)
    # backward from g through the transpose (P^T g)[i] = g[i + 1], every H > 0 (h = 1): dZ = 0.75 shift^T(g), dS = (1 - beta) dZ + beta dZ W
    g = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    dz, ds = co.layer_bwd(ip, ix, g, np.ones((3, 2)), w, alpha, beta)
    want_dz = 0.75 * np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 0.0]])
    np.testing.assert_allclose(dz, want_dz, rtol=0, atol=1e-12)
    want_ds = want_dz if identity_w else 0.5 * want_dz + 0.5 * np.stack([-want_dz[:, 1], 2.0 * want_dz[:, 0]], 1)
    np.testing.assert_allclose(ds, want_ds, rtol=0, atol=1e-12)


@pytest.mark.parametrize("identity_w", [True, False])
def test_hand_answer_on_a_multi_edge_and_an_isolated_row(identity_w):
    """Edges 0 -> 1 twice and 2 -> 1 once; rows 0 and 2 have no in-edge.  dst_norm (1, 3^-1/2, 1), src_norm (2^-1/2, 1, 1):
    (P x)[1] = 3^-1/2 (2 * 2^-1/2 x[0] + x[2]) -- the multi-edge counts twice -- and (P x)[0] = (P x)[2] = 0 without an error."""
    ip, ix = csr_from_edges(np.array([0, 0, 2]), np.array([1, 1, 1]), 3)
    x, h0 = np.array([[3.0], [5.0], [7.0]]), np.array([[1.0], [2.0], [-4.0]])
    alpha, beta = 0.1, 0.3
    w = np.eye(1) if identity_w else np.array([[-2.0]])
    px1 = (2.0 * 3.0 / np.sqrt(2.0) + 7.0) / np.sqrt(3.0)
    want_s = np.array([[0.1 * 1.0], [0.9 * px1 + 0.1 * 2.0], [0.1 * -4.0]])
    s, z, h = co.layer(ip, ix, x, h0, w, alpha, beta)
    np.testing.assert_allclose(s, want_s, rtol=0, atol=1e-12)
    want_z = want_s * (1.0 if identity_w else (0.7 + 0.3 * -2.0))
    np.testing.assert_allclose(z, want_z, rtol=0, atol=1e-12)
    np.testing.assert_allclose(h, np.maximum(want_z, 0.0), rtol=0, atol=1e-12)
    # a dropped source: keep-mask 0 on row 0 removes the multi-edge's contribution, the kept rows are scaled by 1 / (1 - p)
    mask = np.array([[0], [1], [1]], np.uint8)
    s2, _, _ = co.layer(ip, ix, x, h0, w, alpha, beta, mask, 0.5)
    np.testing.assert_allclose(s2[1], 0.9 * (2.0 * 7.0 / np.sqrt(3.0)) + 0.2, rtol=0, atol=1e-12)


def _small_problem(seed, n=24, d=5, L=3, p=0.5):
    ip, ix = random_graph(n, 3, seed=seed, power=0.5, isolated=2, hub=12)
    rs = np.random.RandomState(seed)
    f, c = 6, 4
    params = {co.FC_IN_W: rs.standard_normal((d, f)) * 0.4, co.FC_IN_B: rs.standard_normal(d) * 0.1,
              co.FC_OUT_W: rs.standard_normal((c, d)) * 0.4, co.FC_OUT_B: rs.standard_normal(c) * 0.1}
    for l in range(1, L + 1):
        params[co.conv_w(l)] = rs.uniform(-1, 1, (d, d)) / np.sqrt(d)
    x = rs.standard_normal((n, f))
    labels, idx = rs.randint(0, c, n), np.arange(0, n, 2)
    masks = [(rs.uniform(size=(n, f if s == 0 else d)) >= p).astype(np.uint8) for s in range(L + 2)]
    return ip, ix, params, x, labels, idx, masks


def test_oracle_backward_matches_finite_differences():
    L, alpha, lamda, p = 3, 0.2, 1.5, 0.5
    for seed in range(4, 40):               # the first problem without a pre-activation within reach of the step below (an isolated row
        ip, ix, params, x, labels, idx, masks = _small_problem(seed, L=L, p=p)      # whose H_0 is all zero has Z = 0 exactly: a kink)
        loss, grads, cache = co.loss_and_grads(params, ip, ix, x, labels, idx, L, alpha, lamda, masks, p)
        if min(np.abs(z).min() for z in cache["pre"]) > 1e-5:
            break
    assert min(np.abs(z).min() for z in cache["pre"]) > 1e-5
    eps = 1e-6
    rs = np.random.RandomState(0)
    for name, g in grads.items():
        for _ in range(3):
            at = tuple(rs.randint(0, s) for s in g.shape)
            hi, lo = ({k: v.copy() for k, v in params.items()} for _ in range(2))
            hi[name][at] += eps
            lo[name][at] -= eps
            fd = (co.loss_and_grads(hi, ip, ix, x, labels, idx, L, alpha, lamda, masks, p)[0]
                  - co.loss_and_grads(lo, ip, ix, x, labels, idx, L, alpha, lamda, masks, p)[0]) / (2 * eps)
            assert abs(fd - g[at]) < 1e-7 + 1e-6 * abs(g[at]), (name, at, fd, g[at])


def test_oracle_model_gradients_match_torch_autograd():
    """The oracle (every dropout site masked) against torch autograd on a dense fp64 restatement."""
    L, alpha, lamda, p = 3, 0.1, 0.5, 0.5
    ip, ix, params, x, labels, idx, masks = _small_problem(9, L=L, p=p)
    n = len(ip) - 1
    loss, grads, _ = co.loss_and_grads(params, ip, ix, x, labels, idx, L, alpha, lamda, masks, p)
    t = {a: torch.tensor(b, dtype=torch.float64, requires_grad=True) for a, b in params.items()}
    dn, sn = ao.degree_norms(ip, ix, n)
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)), 1.0)
    pm = torch.tensor(dn[:, None] * dense * sn[None, :])
    keep = [torch.tensor(m / (1 - p)) for m in masks]
    h0 = torch.relu((torch.tensor(x) * keep[0]) @ t[co.FC_IN_W].T + t[co.FC_IN_B])
    h = h0
    for l in range(1, L + 1):
        beta = math.log(lamda / l + 1)
        s = (1 - alpha) * (pm @ (h * keep[l])) + alpha * h0
        h = torch.relu((1 - beta) * s + beta * (s @ t[co.conv_w(l)].T))
    out = (h * keep[L + 1]) @ t[co.FC_OUT_W].T + t[co.FC_OUT_B]
    ref = F.nll_loss(out[idx].log_softmax(1), torch.tensor(labels[idx]))
    ref.backward()
    np.testing.assert_allclose(loss, ref.item(), rtol=1e-12)
    assert set(grads) == set(t)
    for name, g in grads.items():
        np.testing.assert_allclose(g, t[name].grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("L,alpha", [(1, 0.5), (4, 0.1), (10, 0.1)])
def test_lamda_zero_stack_is_appnp(L, alpha):
    """lamda = 0 makes every beta_l = log(1) = 0, so Z_l = S_l; over H_0 >= 0 every S_l >= 0 and every ReLU is the identity: the stack
    is APPNP's propagation, arithmetic that tests/golden/appnp_teacher.npz already pins."""
    ip, ix = random_graph(60, 4, seed=5, power=0.6, isolated=4, hub=30)
    rs = np.random.RandomState(L)
    h0 = np.maximum(rs.standard_normal((60, 6)), 0.0)
    ws = [rs.standard_normal((6, 6)) for _ in range(L)]                     # (beta = 0: the weights do not matter)
    bts = co.betas(L, 0.0)
    assert bts == [0.0] * L
    out = co.stack(ip, ix, h0, ws, alpha, bts)[-1][2]
    np.testing.assert_allclose(out, ao.propagate(ip, ix, h0, L, alpha, None, 0), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- layer, model, conf
def test_beta_values_and_init_bounds():
    from glnn_amd.autograd import gcnii_betas
    from glnn_amd.nn import GCNIIConv
    for l, lamda in ((1, 0.5), (2, 0.5), (64, 0.5), (3, 1.5)):
        conv = GCNIIConv(16, l, 0.1, lamda)
        assert conv.beta == pytest.approx(math.log(lamda / l + 1.0), rel=1e-15)
    assert GCNIIConv(8, 1, 0.1, 0.5).beta == pytest.approx(math.log(1.5))
    assert gcnii_betas(3, 0.5) == pytest.approx(co.betas(3, 0.5), rel=1e-15) and gcnii_betas(2, 0.0) == [0.0, 0.0]
    torch.manual_seed(0)
    conv = GCNIIConv(64, 5)
    assert (conv.alpha, conv.lamda) == (0.1, 0.5)
    assert [n for n, _ in conv.named_parameters()] == ["weight"] and conv.weight.shape == (64, 64) and conv.weight.dtype == torch.float32
    b = 1.0 / math.sqrt(64)
    w = conv.weight.detach()
    assert float(w.abs().max()) <= b and float(w.abs().max()) > 0.9 * b and abs(float(w.mean())) < 0.1 * b
    torch.manual_seed(0)                                                    # the draw is torch's generator's uniform(-b, b)
    assert torch.equal(w, torch.nn.init.uniform_(torch.empty(64, 64), -b, b))


def _conf(**extra):
    conf = dict(model_name="GCNII", num_layers=4, feat_dim=6, hidden_dim=8, label_dim=3, dropout_ratio=0.5, norm_type="none", device="cpu")
    conf.update(extra)
    return conf


def test_state_dict_keys():
    from glnn_amd.models import Model
    m = Model(_conf())
    want = {"encoder.fc_in.weight": (8, 6), "encoder.fc_in.bias": (8,), "encoder.fc_out.weight": (3, 8), "encoder.fc_out.bias": (3,)}
    want.update({f"encoder.layers.{l}.weight": (8, 8) for l in range(4)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert co.conv_w(1) == "encoder.layers.0.weight" and co.FC_IN_W in want and co.FC_OUT_B in want


def test_model_dispatch_and_conf_keys():
    from glnn_amd import models
    m = models.Model(_conf())
    enc = m.encoder
    assert type(enc) is models.GCNII and m.model_name == "GCNII"
    assert (enc.alpha, enc.lamda, enc.num_layers, enc.dropout.p, enc.norm_type) == (0.1, 0.5, 4, 0.5, "none")
    assert [lay.layer for lay in enc.layers] == [1, 2, 3, 4] and all((lay.alpha, lay.lamda) == (0.1, 0.5) for lay in enc.layers)
    assert enc.betas() == pytest.approx(co.betas(4, 0.5))
    enc = models.Model(_conf(gcnii_alpha=0.2, gcnii_lamda=1.5)).encoder
    assert (enc.alpha, enc.lamda) == (0.2, 1.5) and enc.betas() == pytest.approx(co.betas(4, 1.5))
    enc = models.Model(_conf(gcnii_alpha=None, gcnii_lamda=None)).encoder   # the flags' unset value: the defaults
    assert (enc.alpha, enc.lamda) == (0.1, 0.5)
    # every earlier name still builds its own encoder: "GCNII" contains "GCN", and is tested first
    base = dict(_conf(), num_layers=2, norm_type="batch")
    assert type(models.Model(dict(base, model_name="GCN")).encoder) is models.GCN
    assert type(models.Model(dict(base, model_name="APPNP")).encoder) is models.APPNP
    assert type(models.Model(dict(base, model_name="GPRGNN")).encoder) is models.GPRGNN
    assert type(models.Model(dict(base, model_name="SAGE")).encoder) is models.SAGE
    assert type(models.Model(dict(base, model_name="MLP")).encoder) is models.MLP
    assert type(models.Model(dict(base, model_name="GAT", num_heads=2, attn_dropout_ratio=0.3)).encoder) is models.GAT
    with pytest.raises(ValueError, match="Unknown model_name"):
        models.Model(dict(_conf(), model_name="GCII"))


def test_out_of_scope_configurations_raise_naming_gcnii():
    from glnn_amd import dist, models
    from glnn_amd.nn import GCNIIConv
    for bad in (dict(hidden_dim=257), dict(hidden_dim=512), dict(norm_type="batch"), dict(norm_type="layer"), dict(num_layers=65)):
        with pytest.raises(NotImplementedError, match="GCNII"):
            models.Model(_conf(**bad))
    models.Model(_conf(hidden_dim=256, num_layers=64))                      # the limits themselves build
    with pytest.raises(NotImplementedError, match="GCNII"):
        GCNIIConv(260, 1)
    m = models.Model(_conf())
    with pytest.raises(NotImplementedError, match="GCNII"):
        dist.ShardedTeacher(m.encoder, None, None, None)
    with pytest.raises(NotImplementedError, match="GCNII"):
        dist.HaloShardedTeacher(m.encoder, None, None, None)
    with pytest.raises(NotImplementedError, match="not implemented for the GCNII teacher"):      # bf16 activation storage
        m.inference(None, torch.zeros(4, 6), dtype=torch.bfloat16)


def test_engine_recognises_the_name_before_gcn():
    """check_supported takes a GCNII model down the GCNII branch (the GCN branch would read GraphConv attributes it does not have): a
    GCNII encoder whose norm_type or activation was changed behind the constructor's back gets the GCNII refusal.  The optimiser must be
    ONE Adam group: the paper's two weight-decay groups are refused."""
    from glnn_amd import models, teacher
    m = models.Model(_conf())
    assert type(m.encoder) is models.GCNII
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    with pytest.raises(RuntimeError, match="on the GPU"):                   # every model check passed; only the device is wrong here
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    for attr, bad in (("norm_type", "batch"), ("activation", F.gelu)):
        good = getattr(m.encoder, attr)
        setattr(m.encoder, attr, bad)
        with pytest.raises(NotImplementedError, match="TeacherEngine: GCNII with norm_type none and ReLU"):
            teacher.check_supported(m, torch.nn.NLLLoss(), opt)
        setattr(m.encoder, attr, good)
    conv = [p for n, p in m.named_parameters() if "layers" in n]
    dense = [p for n, p in m.named_parameters() if "layers" not in n]
    two = torch.optim.Adam([dict(params=conv, weight_decay=0.01), dict(params=dense, weight_decay=5e-4)], lr=0.01)
    with pytest.raises(NotImplementedError, match="one param group"):
        teacher.check_supported(m, torch.nn.NLLLoss(), two)


def test_seed_stream_is_distinct_within_a_step_and_between_steps():
    from glnn_amd.teacher import TeacherEngine
    L = 64
    eng = types.SimpleNamespace(base_seed=1234567, step_count=1, p=0.6)
    one = [TeacherEngine._gcnii_seed(eng, s) for s in range(L + 2)]
    assert len(set(one)) == L + 2 == 66 and all(0 <= v < 1 << 32 for v in one)
    eng.step_count = 2
    two = [TeacherEngine._gcnii_seed(eng, s) for s in range(L + 2)]
    assert len(set(two)) == 66 and not set(one) & set(two)
    assert [TeacherEngine._gcnii_seed(eng, s, step=1) for s in range(L + 2)] == one
    # a stream of its own: apart from the hidden-layer, edge and attention seeds of the same step
    eng.enc = types.SimpleNamespace(edge_drop=0.5, layers=[types.SimpleNamespace(attn_drop=types.SimpleNamespace(p=0.3))] * 8)
    others = {TeacherEngine._seed(eng, l) for l in range(8)} | {TeacherEngine._edge_seed(eng)} | {TeacherEngine._attn_seed(eng, l) for l in range(8)}
    assert not others & set(two)
    eng.p = 0.0
    assert [TeacherEngine._gcnii_seed(eng, s) for s in range(3)] == [0, 0, 0]


def test_seed_streams_are_frozen():
    """The four per-step streams of the engine at base_seed 1234567, step 7 (and step=3 where a stream takes one): the values the methods
    returned before they became calls of teacher._stream_seed.  A stream whose probability is 0 returns 0."""
    from glnn_amd.teacher import TeacherEngine as T
    eng = types.SimpleNamespace(base_seed=1234567, step_count=7, p=0.6)
    eng.enc = types.SimpleNamespace(edge_drop=0.5, layers=[types.SimpleNamespace(attn_drop=types.SimpleNamespace(p=0.3))] * 3)
    assert [T._seed(eng, l) for l in range(3)] == [3955525820, 1064812690, 3377682224]
    assert (T._edge_seed(eng), T._edge_seed(eng, step=3)) == (18478059, 1909480548)
    assert [T._gcnii_seed(eng, s) for s in range(4)] == [689725636, 1727155465, 1644716809, 1755993479]
    assert [T._gcnii_seed(eng, s, step=3) for s in range(4)] == [543932833, 2033871902, 1256181285, 1450154528]
    assert [T._attn_seed(eng, l) for l in range(3)] == [4294299793, 1597889159, 1524044609]
    eng.p, eng.enc.edge_drop, eng.enc.layers[0].attn_drop.p = 0.0, 0.0, 0.0
    assert (T._seed(eng, 0), T._edge_seed(eng), T._gcnii_seed(eng, 1), T._gcnii_seed(eng, 1, step=3), T._attn_seed(eng, 0)) == (0,) * 5


def test_process_draws_are_frozen():
    """The per-process dropout draws at torch.manual_seed(11), count 5: the values before autograd._draw_base (APPNP's: its former inline
    expression, (initial_seed * 0x85EBCA77 + 5 * 0x9E3779B1 + 0x41505050) mod 2^32, worked out by hand).  Replaying a count leaves the
    call counter alone; count None is a new draw."""
    from glnn_amd import autograd
    torch.manual_seed(11)
    c0 = autograd._drop_counter[0]
    assert autograd.gcnii_stack_seeds(5, 4) == [528114116, 2191935343, 3855756570, 1224610501]
    assert autograd.gat_conv_seeds(5) == (527984600, 527984595)
    assert autograd.gatv2_conv_seeds(5) == (529352152, 529352147)
    assert autograd.appnp_edge_seed(5) == 428303330
    assert autograd._drop_counter[0] == c0
    assert autograd.appnp_edge_seed(None) == autograd.appnp_edge_seed(c0 + 1) and autograd._drop_counter[0] == c0 + 1


# ---------------------------------------------------------------------------------------------------------------- CLI, yaml
def test_cli_flags():
    from glnn_amd.cli import get_teacher_args
    a = get_teacher_args(["--teacher", "GCNII"])
    assert a.teacher == "GCNII" and a.gcnii_alpha is None and a.gcnii_lamda is None
    a = get_teacher_args(["--teacher", "GCNII", "--gcnii_alpha", "0.2", "--gcnii_lamda", "1.5"])
    assert (a.gcnii_alpha, a.gcnii_lamda) == (0.2, 1.5)
    assert get_teacher_args(["--teacher", "GCN"]).gcnii_alpha is None       # the default is no error with another teacher
    for argv in (["--teacher", "GCN", "--gcnii_alpha", "0.2"], ["--teacher", "SAGE", "--gcnii_lamda", "1.0"],
                 ["--gcnii_alpha", "0.1"], ["--teacher", "GPRGNN", "--gcnii_lamda", "0.5"]):
        with pytest.raises(SystemExit):
            get_teacher_args(argv)


def test_training_config():
    import yaml
    from glnn_amd.utils import get_training_config
    path = os.path.join(ROOT, "train.conf.yaml")
    paper = {"cora": (64, 64, 0.6), "citeseer": (32, 256, 0.7), "pubmed": (16, 256, 0.5)}
    for ds, (L, hidden, p) in paper.items():
        conf = get_training_config(path, "GCNII", ds)
        assert (conf["num_layers"], conf["hidden_dim"], conf["dropout_ratio"], conf["norm_type"], conf["model_name"]) == (L, hidden, p, "none",
                                                                                                                         "GCNII")
    full = yaml.safe_load(open(path))
    assert all(("GCNII" in sec) == ("GCN" in sec) for name, sec in full.items() if name != "global")
    for ds, sec in full.items():
        if ds == "global" or ds in paper or "GCNII" not in sec:
            continue
        conf, gcn = get_training_config(path, "GCNII", ds), get_training_config(path, "GCN", ds)
        assert conf["num_layers"] == 8 and conf["hidden_dim"] == min(gcn["hidden_dim"], 256) and conf["norm_type"] == "none"
    assert get_training_config(path, "GCN", "cora") == {"hidden_dim": 64, "num_layers": 2, "dropout_ratio": 0.8, "weight_decay": 0.001,
                                                         "model_name": "GCN"}


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_ops_refuse_cpu_tensors_and_wide_rows():
    from glnn_amd import GlnnError, ops
    x = torch.zeros(4, 4)
    ip, ix = torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(GlnnError):
        ops.gcnii_layer(ip, ix, 0, x, x, torch.zeros(4, 4), 0.1, 0.4, torch.ones(4), x_norm=torch.ones(4))
    with pytest.raises(GlnnError):
        ops.gcnii_layer_bwd(ip, ix, 0, x, x, torch.zeros(4, 4), 0.1, 0.4, torch.zeros(4, 4), torch.zeros(4, 4), True, plain=True)
    assert ops.GCNII_MAX_HIDDEN == 256


def test_library_exports_the_two_symbols_and_reports_bad_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    for name in ("glnn_gcnii_layer_f32", "glnn_gcnii_layer_bwd_f32"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES
    assert h.glnn_abi_version() == 12 and _lib.ABI_VERSION == 12
    fwd = lambda n, nnz, d=4: h.glnn_gcnii_layer_f32(None, None, n, nnz, None, 4, d, None, None, None, None, 4, 0.1, 0.4, None, 0.0, 0, None, 0,
                                                     None, 4, None, None)
    bwd = lambda n, nnz, d=4: h.glnn_gcnii_layer_bwd_f32(None, None, n, nnz, None, 4, d, None, None, None, 0, None, 4, 0.0, 0, 0.1, 0.4, None,
                                                         1.0, None, 4, None, 4, None, 4, 1, None, None)
    for call in (fwd, bwd):
        # null pointers with non-empty sizes: -1 and a message; empty inputs: a no-op; nnz >= 2^31 and d > 256: unsupported
        assert call(4, 4) == -1 and b"null pointer" in h.glnn_last_error()
        assert call(0, 0) == 0
        rc = call(4, 1 << 31)
        assert rc == -2 and b"2^31" in h.glnn_last_error()
        rc = call(4, 4, 257)
        assert rc == -2 and b"256" in h.glnn_last_error()
    header = open(os.path.join(ROOT, "include", "glnn_hip.h")).read()
    for name in ("glnn_gcnii_layer_f32", "glnn_gcnii_layer_bwd_f32"):
        assert f"GLNN_API int {name}(" in header
    assert "Simple and Deep Graph Convolutional Networks" in header and "eq. (5)" in header
