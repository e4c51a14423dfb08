"""CPU checks of the DAGNN teacher: the fp64 oracle (tests/dagnn_oracle.py) by hand answers, by finite differences of its own backward,
against torch CPU autograd on a dense restatement and against the GPR-GNN oracle under a zero gate weight; the state-dict keys, the Model
dispatch and its conf default, the engine's step, the command-line flag, the refusal entries and the exported symbols.  No GPU call is
made here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dagnn_oracle as do
import gpr_oracle as go
from graphgen import csr_from_edges, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sig = do.sigmoid


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_hand_answer_on_a_three_node_path():
    """0 -> 1 -> 2: every norm is 1, so P is the shift (P h)[i] = h[i - 1].  w = (1, 0), b = 0: the gate is the sigmoid of column 0."""
    ip, ix = csr_from_edges(np.array([0, 1]), np.array([1, 2]), 3)
    h0 = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]])
    out = do.propagate(ip, ix, h0, [1.0, 0.0], 0.0, 2)
    r0, r1, r2 = h0
    want = np.array([sig(1.0) * r0,                                          # H_1[0] = H_2[0] = 0: the gate 0.5 multiplies a zero row
                     sig(2.0) * r1 + sig(1.0) * r0,
                     sig(4.0) * r2 + sig(2.0) * r1 + sig(1.0) * r0])
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)
    # K = 0: the gate on h0 alone
    np.testing.assert_allclose(do.propagate(ip, ix, h0, [1.0, 0.0], 0.0, 0), sig(h0[:, :1]) * h0, rtol=0, atol=1e-12)
    # the backward for g = e_(2, 1) (row 2, column 1), K = 1: out[2] = s(4) r2 + s(2) r1
    g = np.zeros((3, 2))
    g[2, 1] = 1.0
    dh0, dw, db = do.propagate_bwd(ip, ix, g, h0, [1.0, 0.0], 0.0, 1)
    ds = lambda z: sig(z) * (1.0 - sig(z))
    want_dh0 = np.array([[0.0, 0.0], [ds(2.0) * 20.0, sig(2.0)], [ds(4.0) * 40.0, sig(4.0)]])
    np.testing.assert_allclose(dh0, want_dh0, rtol=0, atol=1e-12)
    q0, q1 = ds(4.0) * 40.0, ds(2.0) * 20.0                                  # the two gates row 2's output passes through
    np.testing.assert_allclose(dw, q0 * r2 + q1 * r1, rtol=0, atol=1e-12)
    assert abs(db - (q0 + q1)) < 1e-12


def test_hand_answer_on_a_multi_edge_and_an_isolated_row():
    """Edges 0 -> 1 twice and 2 -> 1 once; rows 0 and 2 have no in-edge.  dst_norm (1, 3^-1/2, 1), src_norm (2^-1/2, 1, 1):
    H_1[1] = 3^-1/2 (2 * 2^-1/2 h[0] + h[2]) -- the multi-edge counts twice -- H_1[0] = H_1[2] = 0 and H_2 = 0, so an isolated row keeps
    s_0 h0 alone and no zero-in-degree error is raised."""
    ip, ix = csr_from_edges(np.array([0, 0, 2]), np.array([1, 1, 1]), 3)
    h0 = np.array([[3.0], [5.0], [7.0]])
    w, b = [0.5], -1.0
    h1 = (2.0 * 3.0 / np.sqrt(2.0) + 7.0) / np.sqrt(3.0)
    want = [[sig(0.5) * 3.0], [sig(1.5) * 5.0 + sig(0.5 * h1 - 1.0) * h1], [sig(2.5) * 7.0]]
    np.testing.assert_allclose(do.propagate(ip, ix, h0, w, b, 2), want, rtol=0, atol=1e-12)
    hs = do.hops(ip, ix, h0, 2)
    assert not hs[2].any() and not hs[1][[0, 2]].any()


def _small_multigraph():
    """9 nodes, directed, a multi-edge (3 -> 4 twice) and an isolated row (8: no in-edge, no out-edge)."""
    src = np.array([0, 1, 2, 3, 3, 4, 5, 6, 7, 0, 2, 5, 1])
    dst = np.array([1, 2, 3, 4, 4, 5, 6, 7, 0, 4, 6, 1, 7])
    return csr_from_edges(src, dst, 9)


def test_oracle_backward_matches_finite_differences():
    """Every entry of dh0, dw and db against central differences: 1e-6 relative at eps 1e-6 (C = 5, K = 4)."""
    ip, ix = _small_multigraph()
    assert np.diff(ip)[8] == 0 and np.diff(ip)[4] == 3
    rs = np.random.RandomState(0)
    h0, weight = rs.standard_normal((9, 5)), rs.standard_normal((9, 5))
    w, b = rs.standard_normal(5), 0.3
    eh, ew, eb = do.finite_difference_check(ip, ix, h0, w, b, 4, weight, eps=1e-6)
    print(f"finite differences: dh0 {eh:.2e} dw {ew:.2e} db {eb:.2e}")
    assert eh < 1e-6 and ew < 1e-6 and eb < 1e-6, (eh, ew, eb)


def _dense_p(ip, ix):
    n = len(ip) - 1
    a = np.zeros((n, n))
    np.add.at(a, (np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)), 1.0)       # A[i, j] = the number of edges j -> i
    din, dout = np.maximum(a.sum(1), 1.0), np.maximum(a.sum(0), 1.0)
    return a / np.sqrt(din)[:, None] / np.sqrt(dout)[None, :]


@pytest.mark.parametrize("k", [0, 1, 4])
def test_oracle_matches_torch_autograd_on_a_dense_restatement(k):
    ip, ix = random_graph(40, 3, seed=2, power=0.6, isolated=3, hub=20)
    rs = np.random.RandomState(k)
    h0n, gn, wn, bn = rs.standard_normal((40, 5)), rs.standard_normal((40, 5)), rs.standard_normal(5), -0.4
    p = torch.from_numpy(_dense_p(ip, ix))
    h0, w, b = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (h0n, wn, [bn]))
    h, out = h0, torch.sigmoid(h0 @ w + b)[:, None] * h0
    for _ in range(k):
        h = p @ h
        out = out + torch.sigmoid(h @ w + b)[:, None] * h
    np.testing.assert_allclose(do.propagate(ip, ix, h0n, wn, bn, k), out.detach().numpy(), rtol=1e-12, atol=1e-12)
    (out * torch.from_numpy(gn)).sum().backward()
    dh0, dw, db = do.propagate_bwd(ip, ix, gn, h0n, wn, bn, k)
    np.testing.assert_allclose(dh0, h0.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dw, w.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(db, b.grad.item(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("b", [0.0, 0.7, -2.0])
def test_a_zero_gate_weight_gives_gpr_with_a_constant_gamma(b):
    """w = 0: every gate is sigmoid(b), so out = sigmoid(b) sum_k P^k h0 -- GPR-GNN with gamma identically sigmoid(b) (0.5 at b = 0) -- and
    dh0 is GPR's with that gamma."""
    ip, ix = random_graph(60, 4, seed=5, power=0.6, isolated=4, hub=30)
    rs = np.random.RandomState(1)
    h0, g = rs.standard_normal((60, 7)), rs.standard_normal((60, 7))
    k = 6
    gamma = np.full(k + 1, sig(b))
    if b == 0.0:
        assert (gamma == 0.5).all()
    np.testing.assert_allclose(do.propagate(ip, ix, h0, np.zeros(7), b, k), go.propagate(ip, ix, h0, gamma), rtol=1e-13, atol=1e-13)
    dh0, dw, db = do.propagate_bwd(ip, ix, g, h0, np.zeros(7), b, k)
    gdh0, dgamma = go.propagate_bwd(ip, ix, g, h0, gamma)
    np.testing.assert_allclose(dh0, gdh0, rtol=1e-13, atol=1e-13)
    # db = sum_k <G_k, h0> s (1 - s): the gate's slope times GPR's coefficient gradients
    np.testing.assert_allclose(db, sig(b) * (1.0 - sig(b)) * dgamma.sum(), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def _conf(**extra):
    return dict(dict(model_name="DAGNN", num_layers=3, feat_dim=6, hidden_dim=8, label_dim=4, dropout_ratio=0.5, norm_type="batch",
                     device="cpu"), **extra)


def test_teacher_kind_and_the_order_of_the_keys():
    from glnn_amd import kinds, models
    assert models.teacher_kind("DAGNN") == "dagnn" and "dagnn" in models.FULL_GRAPH_KINDS
    keys = [row.key for row in kinds.KINDS]
    assert all(k == "DAGNN" or (k not in "DAGNN" and "DAGNN" not in k) for k in keys)      # no key contains it, it contains none
    for name, kind in (("GPRGNN", "gpr"), ("GCNII", "gcnii"), ("GCN", "gcn"), ("GATv2", "gatv2"), ("GAT", "gat"), ("APPNP", "appnp"),
                       ("SAGE", "sage"), ("MLP3w4", "mlp")):
        assert models.teacher_kind(name) == kind
    with pytest.raises(ValueError, match="Unknown model_name"):
        models.teacher_kind("DAGN")


def test_model_builds_dagnn_with_the_trunk_keys_plus_the_gate():
    from glnn_amd import models
    m = models.Model(_conf())
    appnp = models.Model(_conf(model_name="APPNP"))
    enc = m.encoder
    assert type(enc) is models.DAGNN and isinstance(enc, models._TrunkProp) and m.kind == "dagnn"
    gate = {"encoder.propagate.proj.weight": (1, 4), "encoder.propagate.proj.bias": (1,)}
    assert set(m.state_dict()) == set(appnp.state_dict()) | set(gate)
    for key, shape in gate.items():
        assert tuple(m.state_dict()[key].shape) == shape
    assert enc.k == 10 and enc.propagate.k == 10                             # the conf default
    assert models.Model(_conf(dagnn_k=3)).encoder.k == 3 and models.Model(_conf(dagnn_k=None)).encoder.k == 10
    assert models.Model(_conf(dagnn_k=0)).encoder.k == 0
    # the trunk is APPNP's draw for draw, and the gate is torch's default Linear drawn after it
    torch.manual_seed(11)
    a = models.Model(_conf(model_name="APPNP")).state_dict()
    ref_gate = torch.nn.Linear(4, 1).state_dict()
    torch.manual_seed(11)
    b = models.Model(_conf()).state_dict()
    for key, v in a.items():
        assert torch.equal(v, b[key]), key
    assert torch.equal(b["encoder.propagate.proj.weight"], ref_gate["weight"]) and torch.equal(b["encoder.propagate.proj.bias"], ref_gate["bias"])


def test_conv_refuses_bad_arguments():
    from glnn_amd.nn import DAGNNConv
    with pytest.raises(ValueError, match="k must be >= 0"):
        DAGNNConv(-1, 4)
    with pytest.raises(NotImplementedError, match="256"):
        DAGNNConv(2, 257)
    DAGNNConv(0, 256)
    with pytest.raises(NotImplementedError, match="DAGNNConv.*bipartite"):
        DAGNNConv(2, 4)([None, None], torch.zeros(4, 4))


def test_engine_step_and_check_supported(monkeypatch):
    from glnn_amd import models, ops, teacher
    from glnn_amd.train_and_eval import _full_graph_step
    monkeypatch.setattr(ops, "TensorTable", lambda *a: None)               # the engine's only GPU-bound member
    m = models.Model(_conf())
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    eng = teacher.TeacherEngine(m, opt)
    assert eng.kind == "dagnn" and _full_graph_step(eng, "DAGNN") == eng.step_dagnn
    proj = m.encoder.propagate.proj
    assert eng.grad(proj.weight).shape == (1, 4) and eng.grad(proj.bias).shape == (1,)      # both are tensors of the one Adam table
    m.encoder.activation = torch.tanh
    with pytest.raises(NotImplementedError, match="DAGNN with norm_type"):
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    m = models.Model(_conf(norm_type="none"))
    with pytest.raises(RuntimeError, match="needs the model on the GPU"):    # accepted up to the last check (the device)
        teacher.check_supported(m, torch.nn.NLLLoss(), torch.optim.Adam(m.parameters(), lr=0.01))


def test_cli_takes_dagnn_k_for_dagnn_only(capsys):
    from glnn_amd.cli import _training_config, get_student_args, get_teacher_args
    a = get_teacher_args(["--teacher", "DAGNN"])
    assert a.teacher == "DAGNN" and a.dagnn_k is None
    assert get_teacher_args(["--teacher", "DAGNN", "--dagnn_k", "4"]).dagnn_k == 4
    assert get_teacher_args(["--teacher", "GCN"]).dagnn_k is None           # the default is no error with another teacher
    assert get_student_args(["--teacher", "DAGNN", "--student", "MLP"]).teacher == "DAGNN"
    for argv in (["--teacher", "GPRGNN", "--dagnn_k", "4"], ["--dagnn_k", "4"], ["--teacher", "APPNP", "--dagnn_k", "10"],
                 ["--teacher", "DAGNN", "--dagnn_k", "-1"]):
        with pytest.raises(SystemExit):
            get_teacher_args(argv)
        assert "--dagnn_k" in capsys.readouterr().err
    # train.conf.yaml names no DAGNN section: the dataset's APPNP section (the trunk's hyper-parameters) stands in
    path = os.path.join(ROOT, "train.conf.yaml")
    conf = _training_config(path, "DAGNN", "cora")
    assert conf == {"hidden_dim": 128, "num_layers": 2, "dropout_ratio": 0.5, "weight_decay": 0.01, "model_name": "DAGNN"}
    assert _training_config(path, "DAGNN", "ogbn-arxiv")["model_name"] == "DAGNN"
    from glnn_amd.utils import get_training_config
    assert _training_config(path, "GCN", "cora") == get_training_config(path, "GCN", "cora")


def test_sharded_teachers_name_dagnn_in_their_refusal():
    import glnn_amd.dist as gdist
    from glnn_amd import models
    enc = models.Model(_conf()).encoder
    for cls in (gdist.ShardedTeacher, gdist.HaloShardedTeacher):
        with pytest.raises(NotImplementedError, match="DAGNN teacher is not sharded.*gate"):
            cls(enc, None, None, None)


def test_ops_refuse_cpu_tensors_and_wide_rows():
    from glnn_amd import GlnnError, ops
    x = torch.zeros(4, 4)
    with pytest.raises(GlnnError):
        ops.dagnn_gate(x, 0, torch.zeros(4), torch.zeros(1), torch.zeros(4, 4))
    with pytest.raises(GlnnError):
        ops.dagnn_gate_bwd(x, x, 0, torch.zeros(4), torch.zeros(4), None, torch.zeros(4, 4), torch.zeros(4))
    with pytest.raises(GlnnError):
        ops.dagnn_fold(torch.zeros(8, 4), torch.zeros(8))


def test_library_exports_the_symbols_and_reports_bad_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    for name in ("glnn_dagnn_gate_f32", "glnn_dagnn_gate_bwd_f32", "glnn_dagnn_fold_f32", "glnn_dagnn_fold_workspace_bytes"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib.SIGNATURES
    fwd = lambda n, d=4, k=1: h.glnn_dagnn_gate_f32(None, 4, n, d, None, None, k, None, 4, None, None)
    bwd = lambda n, d=4, k=1: h.glnn_dagnn_gate_bwd_f32(None, 4, None, 4, n, d, None, None, k, None, 4, None, 4, None, None)
    for call in (fwd, bwd):
        assert call(4) == -1 and b"null pointer" in h.glnn_last_error()         # null pointers with non-empty sizes
        assert call(0) == 0                                                     # empty inputs: a no-op
        assert call(4, 257) == -2 and b"256" in h.glnn_last_error()             # GLNN_ERR_UNSUPPORTED, nothing launched
        assert call(4, 0) == -1 and call(4, 4, -1) == -1
    assert h.glnn_dagnn_fold_f32(None, 4, None, 100, 4, None, None, None, 0, None) == -1 and b"null pointer" in h.glnn_last_error()
    chunk = _lib.DAGNN_FOLD_CHUNK
    assert h.glnn_dagnn_fold_workspace_bytes(chunk + 1, 40) == 2 * 41 * 8 and h.glnn_dagnn_fold_workspace_bytes(chunk, 1) == 2 * 8
    header = open(os.path.join(ROOT, "include", "glnn_hip.h")).read()
    assert f"#define GLNN_DAGNN_FOLD_CHUNK {chunk}\n" in header
