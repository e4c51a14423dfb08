"""CPU checks of the GATv2 teacher: the fp64 oracle (tests/gatv2_oracle.py) by hand answers, by finite differences and against torch
autograd on a dense restatement; the property that separates GATv2 from GAT; the state-dict keys and the init RNG stream; the Model
dispatch and its conf contract; every refusal; the command line and the training config; the exported symbols.  No GPU call is made."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import gat_oracle as g1
import gatv2_oracle as vo
from graphgen import csr_from_edges, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glnn_gatv2_attn_fwd_f32", "glnn_gatv2_attn_bwd_f32", "glnn_gatv2_attn_bwd_workspace_floats")


def _lrelu(v):
    return v if v > 0 else 0.2 * v


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_hand_answer_on_a_three_node_path():
    """0 -> 1 -> 2 with self-loops on 0 and 1; H = F = 1, attn = 2.  Rows 0 and 2 have ONE in-edge: a = 1, out = zl[source], ds = 0.
    Row 1 sees u = zl_0 + zr_1 = 2 (score 4) and u = zl_1 + zr_1 = -1 (score 2 * -0.2 = -0.4)."""
    ip, ix = csr_from_edges(np.array([0, 0, 1, 1]), np.array([0, 1, 1, 2]), 3)
    assert ip.tolist() == [0, 1, 3, 4] and ix.tolist() == [0, 0, 1, 1]
    zl, zr, at = np.array([1.0, -2.0, 0.5]).reshape(3, 1, 1), np.array([0.5, 1.0, -1.0]).reshape(3, 1, 1), np.array([[2.0]])
    y, c = vo.attn_fwd(ip, ix, zl, zr, at, relu=False)
    a0 = 1.0 / (1.0 + math.exp(-0.4 - 4.0))
    a1 = 1.0 - a0
    np.testing.assert_allclose(c["s"][:, 0], [2 * 1.5, 4.0, -0.4, 2 * _lrelu(-3.0)], rtol=1e-15)
    np.testing.assert_allclose(c["a"][:, 0], [1.0, a0, a1, 1.0], rtol=1e-14)
    np.testing.assert_allclose(y[:, 0, 0], [1.0, a0 * 1.0 + a1 * -2.0, -2.0], rtol=1e-14)
    np.testing.assert_allclose(c["lse"][:, 0], [3.0, 4.0 + math.log1p(math.exp(-4.4)), -1.2], rtol=1e-14)
    g = np.array([0.5, 1.0, -3.0])
    dzl, dzr, dattn, ds = vo.attn_bwd(c, g.reshape(3, 1))
    D = a0 * 1.0 + a1 * -2.0                                 # g_1 = 1: c_01 = zl_0, c_11 = zl_1
    ds0, ds1 = a0 * (1.0 - D), a1 * (-2.0 - D)
    np.testing.assert_allclose(ds[:, 0], [0.0, ds0, ds1, 0.0], atol=1e-15)
    de0, de1 = ds0 * 2.0 * 1.0, ds1 * 2.0 * 0.2              # u = 2 > 0, u = -1 < 0
    np.testing.assert_allclose(dzr[:, 0, 0], [0.0, de0 + de1, 0.0], atol=1e-15)
    np.testing.assert_allclose(dzl[:, 0, 0], [0.5 * 1.0 + a0 * 1.0 + de0, a1 * 1.0 + de1 + 1.0 * -3.0, 0.0], rtol=1e-14)
    np.testing.assert_allclose(dattn[0, 0], ds0 * 2.0 + ds1 * -0.2, rtol=1e-14)


def test_hand_answer_on_a_multi_edge_beside_a_degree_one_row():
    """Edges 0 -> 1 TWICE (equal scores: a = 1/2 each, each its own term and its own dropout draw) and 0 -> 2 once (a = 1 whatever the
    score).  With the second copy and the lone edge dropped (p = 0.5): out_1 = (1/2) * 2 * zl_0, out_2 = 0 -- but lse_2 is still the
    edge's score: a dropped edge stays in the softmax."""
    ip, ix = csr_from_edges(np.array([0, 0, 0, 0]), np.array([0, 1, 1, 2]), 3)
    zl = np.array([[[1.0, -1.0]], [[9.0, 9.0]], [[9.0, 9.0]]])
    zr = np.array([[[0.0, 0.0]], [[1.0, 0.5]], [[-2.0, 3.0]]])
    at = np.array([[1.0, -3.0]])
    mask = np.array([[1], [1], [0], [0]], np.uint8)
    y, c = vo.attn_fwd(ip, ix, zl, zr, at, relu=False, attn_mask=mask, attn_p=0.5)
    np.testing.assert_allclose(c["a"][:, 0], [1.0, 0.5, 0.5, 1.0], rtol=1e-15)
    np.testing.assert_allclose(y[:, 0], [[2.0, -2.0], [1.0, -1.0], [0.0, 0.0]], rtol=1e-15)
    s2 = 1.0 * _lrelu(1.0 - 2.0) - 3.0 * _lrelu(-1.0 + 3.0)
    np.testing.assert_allclose(c["lse"][2, 0], s2, rtol=1e-15)
    s1 = 1.0 * _lrelu(2.0) - 3.0 * _lrelu(-0.5)
    np.testing.assert_allclose(c["lse"][1, 0], s1 + math.log(2.0), rtol=1e-15)
    # backward: c of the kept copy is 2 <g_1, zl_0>, of the dropped copy 0; D_1 is their mean
    g = np.array([[0.0, 0.0], [1.0, 2.0], [5.0, 5.0]])
    _, dzr, _, ds = vo.attn_bwd(c, g)
    ck = 2.0 * (1.0 * 1.0 + 2.0 * -1.0)
    np.testing.assert_allclose(ds[:, 0], [0.0, 0.5 * (ck - ck / 2), 0.5 * (0.0 - ck / 2), 0.0], atol=1e-15)
    np.testing.assert_allclose(dzr[1:], 0.0, atol=1e-15)      # equal u on both copies: the two de cancel; a lone edge has ds = 0


def _small_layer(seed, n=30, d_in=5, H=3, F=4, multi=True):
    rs = np.random.RandomState(seed)
    ip, ix = random_graph(n, 3, seed=seed, self_loops=True, hub=12)
    p = {"fc_src.weight": rs.standard_normal((H * F, d_in)) * 0.5, "fc_src.bias": rs.standard_normal(H * F) * 0.3,
         "fc_dst.weight": rs.standard_normal((H * F, d_in)) * 0.5, "fc_dst.bias": rs.standard_normal(H * F) * 0.3,
         "attn": rs.standard_normal((1, H, F))}
    x = rs.standard_normal((n, d_in))
    fm, am = (rs.rand(n, d_in) > 0.4).astype(np.uint8), (rs.rand(len(ix), H) > 0.3).astype(np.uint8)
    return ip, ix, p, x, fm, am, rs.standard_normal((n, H * F))


@pytest.mark.parametrize("relu", [False, True])
def test_oracle_backward_matches_finite_differences(relu):
    ip, ix, p, x, fm, am, gy = _small_layer(3)
    y, c = vo.layer_fwd(ip, ix, x, p, relu, fm, 0.4, am, 0.3)
    # no kink within reach of the step (a head with every in-edge dropped is 0 exactly, on both sides of any step)
    assert np.abs(c["u"]).min() > 1e-4 and (not relu or np.abs(c["r"][c["r"] != 0]).min() > 1e-4)
    dx, grads = vo.layer_bwd(c, gy)
    loss = lambda xx, pp: float((vo.layer_fwd(ip, ix, xx, pp, relu, fm, 0.4, am, 0.3)[0] * gy).sum())
    rs, eps = np.random.RandomState(0), 1e-6
    for name, ana in [("x", dx)] + sorted(grads.items()):
        base = x if name == "x" else p[name]
        for _ in range(6):
            i = tuple(rs.randint(0, s) for s in base.shape)
            hi, lo = base.copy(), base.copy()
            hi[i] += eps
            lo[i] -= eps
            f = (loss(hi, p) - loss(lo, p)) if name == "x" else (loss(x, dict(p, **{name: hi})) - loss(x, dict(p, **{name: lo})))
            np.testing.assert_allclose(ana.reshape(base.shape)[i], f / (2 * eps), rtol=2e-6, atol=1e-8, err_msg=f"{name}{i}")


@pytest.mark.parametrize("H,F,relu", [(4, 2, True), (1, 7, False), (3, 5, True)])
def test_oracle_matches_torch_autograd_on_a_dense_restatement(H, F, relu):
    """A simple graph as a dense adjacency A[i, j] = [edge j -> i]: scores, softmax, masks and aggregation as [N, N, H] tensors in
    fp64, gradients by torch autograd."""
    n, d_in, pf, pa = 14, 5, 0.4, 0.3
    rs = np.random.RandomState(10 * H + F)
    A = (rs.rand(n, n) < 0.25) | np.eye(n, dtype=bool)
    dst, src = np.nonzero(A)
    ip, ix = csr_from_edges(src, dst, n)
    np.testing.assert_array_equal(ix, src)                                               # CSR order = row-major order of A
    p = {"fc_src.weight": rs.standard_normal((H * F, d_in)) * 0.5, "fc_src.bias": rs.standard_normal(H * F) * 0.3,
         "fc_dst.weight": rs.standard_normal((H * F, d_in)) * 0.5, "fc_dst.bias": rs.standard_normal(H * F) * 0.3,
         "attn": rs.standard_normal((1, H, F))}
    x, gy = rs.standard_normal((n, d_in)), rs.standard_normal((n, H * F))
    fm, M = (rs.rand(n, d_in) > pf).astype(np.uint8), (rs.rand(n, n, H) > pa).astype(np.uint8)
    y, c = vo.layer_fwd(ip, ix, x, p, relu, fm, pf, M[dst, src], pa)
    dx, grads = vo.layer_bwd(c, gy)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in dict(p, x=x).items()}
    h = t["x"] * torch.from_numpy(fm / (1 - pf))
    zl = (h @ t["fc_src.weight"].T + t["fc_src.bias"]).view(n, H, F)
    zr = (h @ t["fc_dst.weight"].T + t["fc_dst.bias"]).view(n, H, F)
    u = zl[None, :] + zr[:, None]                                                        # [i, j, H, F]
    s = (torch.nn.functional.leaky_relu(u, 0.2) * t["attn"][0]).sum(-1)
    s = s.masked_fill(torch.from_numpy(~A)[:, :, None], -math.inf)
    a = torch.softmax(s, dim=1) * torch.from_numpy(M / (1 - pa))
    out = torch.einsum("ijh,jhf->ihf", a, zl)
    out = torch.relu(out) if relu else out
    np.testing.assert_allclose(y, out.detach().numpy().reshape(n, -1), rtol=1e-12, atol=1e-13)
    out.reshape(n, -1).backward(torch.from_numpy(gy))
    np.testing.assert_allclose(dx, t["x"].grad.numpy(), rtol=1e-10, atol=1e-12)
    for k, v in grads.items():
        np.testing.assert_allclose(v, t[k].grad.numpy().reshape(v.shape), rtol=1e-10, atol=1e-12, err_msg=k)


def test_dynamic_attention_separates_gatv2_from_gat():
    """Sources 0 and 1, destinations 2 and 3 (each with in-edges from both), one head.  One fixed GATv2 layer ranks 0 above 1 for
    destination 2 and 1 above 0 for destination 3.  GAT's score leaky_relu(el[j] + er[i]) is increasing in el[j] for every i, so under
    the GAT oracle the two destinations always rank alike, whatever fc, attn_l and attn_r are."""
    src, dst = np.array([0, 1, 0, 1, 0, 1]), np.array([0, 1, 2, 2, 3, 3])
    ip, ix = csr_from_edges(src, dst, 4)
    x = np.eye(4)
    p = {"fc_src.weight": np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]]), "fc_src.bias": np.zeros(2),
         "fc_dst.weight": np.array([[0.0, 0.0, 0.0, -5.0], [0.0, 0.0, -5.0, 0.0]]), "fc_dst.bias": np.zeros(2),
         "attn": np.ones((1, 1, 2))}
    _, c = vo.layer_fwd(ip, ix, x, p, relu=False)
    a = c["a"][:, 0]
    e = {(int(s), int(d)): k for k, (s, d) in enumerate(zip(c["src"], c["dst"]))}
    np.testing.assert_allclose([c["s"][e[0, 2], 0], c["s"][e[1, 2], 0], c["s"][e[0, 3], 0], c["s"][e[1, 3], 0]], [0.0, -0.8, -0.8, 0.0],
                               atol=1e-15)
    assert a[e[0, 2]] > a[e[1, 2]] and a[e[0, 3]] < a[e[1, 3]]
    rs = np.random.RandomState(0)
    for _ in range(200):
        F = int(rs.randint(1, 5))
        w, al, ar = rs.standard_normal((F, 4)) * 3, rs.standard_normal((1, 1, F)) * 3, rs.standard_normal((1, 1, F)) * 3
        a1 = g1.layer_fwd(ip, ix, x, w, al, ar, False)[1]["a"][:, 0]
        assert (a1[e[0, 2]] - a1[e[1, 2]]) * (a1[e[0, 3]] - a1[e[1, 3]]) >= 0.0


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def _conf(**kw):
    return dict(dict(model_name="GATv2", num_layers=2, feat_dim=8, hidden_dim=16, label_dim=4, dropout_ratio=0.0, norm_type="none",
                     device="cpu", num_heads=4, attn_dropout_ratio=0.1), **kw)


def test_state_dict_keys_and_init_rng_stream():
    """Keys encoder.layers.{i}.fc_src.weight|bias, .fc_dst.weight|bias, .attn.  Per layer the two nn.Linear constructors draw, then
    xavier_normal_(gain relu) on fc_src.weight, fc_dst.weight, attn in that order; biases are zero."""
    from glnn_amd.models import Model
    torch.manual_seed(7)
    m = Model(_conf(num_layers=3))
    sd = m.state_dict()
    shapes = {0: (8, 4, 4), 1: (16, 4, 4), 2: (16, 1, 4)}                  # layer: (in, heads, out)
    assert set(sd) == {f"encoder.layers.{l}.{k}" for l in range(3) for k in vo.KEYS}
    torch.manual_seed(7)
    gain = torch.nn.init.calculate_gain("relu")
    for l, (d_in, H, F) in shapes.items():
        torch.nn.Linear(d_in, H * F)
        torch.nn.Linear(d_in, H * F)
        for k, shape in (("fc_src.weight", (H * F, d_in)), ("fc_dst.weight", (H * F, d_in)), ("attn", (1, H, F))):
            want = torch.nn.init.xavier_normal_(torch.empty(shape), gain=gain)
            assert torch.equal(sd[f"encoder.layers.{l}.{k}"], want), (l, k)
        assert not sd[f"encoder.layers.{l}.fc_src.bias"].any() and not sd[f"encoder.layers.{l}.fc_dst.bias"].any()
        assert tuple(sd[f"encoder.layers.{l}.fc_dst.bias"].shape) == (H * F,)
    assert m.encoder.layers[0].attn_drop.p == 0.1 and m.encoder.layers[2]._num_heads == 1 and m.encoder.layers[2].activation is None


def test_model_dispatch_and_conf_contract():
    from glnn_amd import models
    assert type(models.Model(_conf()).encoder) is models.GATv2
    for name in ("GAT", "GATv", "GAT2"):                                    # the substring rule: these stay v1 GATs
        assert type(models.Model(_conf(model_name=name)).encoder) is models.GAT, name
    base = {k: v for k, v in _conf().items() if k not in ("num_heads", "attn_dropout_ratio")}
    with pytest.raises(NotImplementedError, match="GATv2.*num_heads"):
        models.Model(dict(base, attn_dropout_ratio=0.1))
    with pytest.raises(NotImplementedError, match="GATv2.*attn_dropout_ratio"):
        models.Model(dict(base, num_heads=4))
    with pytest.raises(ValueError, match="GATv2.*multiple"):
        models.Model(_conf(num_heads=3))
    with pytest.raises(ValueError, match="GATv2.*multiple"):
        models.Model(_conf(hidden_dim=2))


def test_out_of_scope_configurations_raise_naming_gatv2():
    from glnn_amd import dist, models
    from glnn_amd.nn import GATv2Conv
    with pytest.raises(NotImplementedError, match="GATv2.*num_layers"):
        models.Model(_conf(num_layers=1))
    m = models.Model(_conf())
    with pytest.raises(NotImplementedError, match="not implemented for the GATv2 teacher"):      # bf16 activation storage
        m.inference(None, torch.zeros(4, 8), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="GATv2"):
        dist.ShardedTeacher(m.encoder, None, None, None)
    with pytest.raises(NotImplementedError, match="GATv2"):
        dist.HaloShardedTeacher(m.encoder, None, None, None)
    with pytest.raises(NotImplementedError, match="GATv2Conv.*bipartite"):
        GATv2Conv((8, 8), 4, 2)
    with pytest.raises(NotImplementedError, match="GATv2Conv.*residual"):
        GATv2Conv(8, 4, 2, residual=True)
    with pytest.raises(NotImplementedError, match="GATv2.*residual"):
        models.GATv2(3, 8, 16, 4, 0.0, torch.nn.functional.relu, residual=True)
    with pytest.raises(NotImplementedError, match="GATv2Conv.*num_heads <= 64"):
        GATv2Conv(8, 1, 65)
    with pytest.raises(NotImplementedError, match="GATv2Conv.*256"):
        GATv2Conv(8, 257, 1)
    with pytest.raises(NotImplementedError, match="GATv2Conv.*activation"):
        GATv2Conv(8, 4, 2, activation=torch.tanh)
    GATv2Conv(8, 4, 64)                                                      # 64 heads of 4: the limit itself is accepted
    lay = GATv2Conv(8, 4, 2)
    with pytest.raises(NotImplementedError, match="GATv2Conv.*bipartite"):
        lay([None, None], torch.zeros(4, 8))


def test_engine_and_train_recognise_the_name_before_gat():
    """check_supported takes a GATv2 model down its own branch (GAT's would pass too, but the engine's kind decides which step runs)."""
    from glnn_amd import models, teacher
    m = models.Model(_conf())
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    m.encoder.layers[0].activation = None                                    # behind the constructor's back
    with pytest.raises(NotImplementedError, match="GATv2"):
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    assert hasattr(teacher.TeacherEngine, "step_gatv2")


def test_one_resolver_routes_every_configured_name(monkeypatch):
    """models.teacher_kind over every model name of train.conf.yaml (read from the file) plus the names a substring rule can mis-route:
    the kind, Model's encoder class, TeacherEngine.kind and train()'s step all follow it.  The expectation is derived apart from the
    resolver: a configured name is a family name with an optional "GA1" prefix and width suffix ("3w4")."""
    import yaml
    from glnn_amd import models, ops, teacher
    from glnn_amd.train_and_eval import _full_graph_step
    family = {"MLP": ("mlp", models.MLP), "SAGE": ("sage", models.SAGE), "GCNII": ("gcnii", models.GCNII), "GCN": ("gcn", models.GCN),
              "APPNP": ("appnp", models.APPNP), "GATv2": ("gatv2", models.GATv2), "GAT": ("gat", models.GAT),
              "GPRGNN": ("gpr", models.GPRGNN)}
    conf = yaml.safe_load(open(os.path.join(ROOT, "train.conf.yaml")))
    names = {name for ds, section in conf.items() if ds != "global" for name in section}
    assert {"MLP", "SAGE", "GCN", "GAT", "GATv2", "MLP3w4"} <= names
    names |= {"GCNII", "GATv2", "GAT", "GCN", "GPRGNN", "MLP3w4"}
    monkeypatch.setattr(ops, "TensorTable", lambda *a: None)               # the engine's only GPU-bound member
    for name in sorted(names):
        kind, cls = family[re.sub(r"\d+w\d+$", "", re.sub(r"^GA1", "", name))]
        assert models.teacher_kind(name) == kind, name
        m = models.Model(_conf(model_name=name))
        assert type(m.encoder) is cls and m.kind == kind, name
        eng = teacher.TeacherEngine(m, torch.optim.Adam(m.parameters(), lr=0.01))
        assert eng.kind == kind, name
        if kind in ("mlp", "sage"):
            with pytest.raises(NotImplementedError, match="no full-graph step"):
                _full_graph_step(eng, name)
        else:
            assert _full_graph_step(eng, name) == getattr(eng, "step_" + kind), name
    for name in ("GCII", "GPR", "gat", ""):
        with pytest.raises(ValueError, match="Unknown model_name"):
            models.teacher_kind(name)


def test_cli_and_training_config():
    from glnn_amd.cli import get_student_args, get_teacher_args
    from glnn_amd.utils import get_training_config
    assert get_teacher_args(["--teacher", "GATv2"]).teacher == "GATv2"
    assert get_student_args(["--teacher", "GATv2", "--student", "MLP"]).teacher == "GATv2"
    path = os.path.join(ROOT, "train.conf.yaml")
    for ds in ("cora", "citeseer", "pubmed", "a-computer", "a-photo"):
        v2, v1 = get_training_config(path, "GATv2", ds), get_training_config(path, "GAT", ds)
        assert {k: v for k, v in v2.items() if k != "model_name"} == {k: v for k, v in v1.items() if k != "model_name"}, ds
    arxiv = get_training_config(path, "GATv2", "ogbn-arxiv")
    assert arxiv["num_heads"] == 8 and arxiv["attn_dropout_ratio"] == 0.3 and arxiv["hidden_dim"] % arxiv["num_heads"] == 0


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_library_exports_the_symbols_and_the_binding_table_matches_the_header():
    from glnn_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glnn_hip.h")).read(), flags=re.S)
    h = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        m = re.search(r"GLNN_API\s+[\w\s\*]+?\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/glnn_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert hasattr(raw, name)
    assert h.glnn_abi_version() == 12 and _lib.ABI_VERSION == 12


def test_entries_report_bad_arguments_before_any_launch():
    from glnn_amd import _lib
    h = _lib.lib()
    fwd = lambda n, nnz, H=2, F=4: h.glnn_gatv2_attn_fwd_f32(None, None, n, nnz, None, 8, None, 8, H, F, None, 0.2, 0.0, 0, 0, None, 8, None,
                                                             None)
    bwd = lambda n, nnz, H=2, F=4: h.glnn_gatv2_attn_bwd_f32(None, None, None, None, None, n, nnz, None, 8, None, 8, H, F, None, None, None, 8,
                                                             0.2, 0.0, 0, None, None, 8, None, 8, None, None, 0, None)
    for call in (fwd, bwd):
        assert call(4, 4) == -1 and b"null pointer" in h.glnn_last_error()
        assert call(0, 0) == 0                                              # empty inputs: a no-op
        assert call(4, 1 << 31) == -2 and b"2^31" in h.glnn_last_error()
        assert call(4, 4, 65, 1) == -2 and b"heads <= 64" in h.glnn_last_error()
        assert call(4, 4, 1, 257) == -2 and b"256" in h.glnn_last_error()
        assert call(4, 4, 0, 4) == -1
    assert h.glnn_gatv2_attn_bwd_workspace_floats(600, 8, 16) >= 128 * ((600 + 7) // 8)
