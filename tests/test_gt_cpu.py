"""CPU checks of the GraphTransformer teacher: the fp64 oracle (tests/gt_oracle.py) by hand answers, by finite differences and against torch
autograd on a dense restatement; the name's resolution; the state-dict keys, shapes and the init RNG stream; every refusal; the command
line and the training config's fallback; the exported symbols and their argument checks.  No GPU call is made."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import gt_oracle as to
from graphgen import csr_from_edges, random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glnn_gt_attn_fwd_f32", "glnn_gt_attn_bwd_f32", "glnn_gt_attn_bwd_workspace_floats")


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_hand_answer_on_a_three_node_path():
    """0 -> 1 -> 2 with self-loops on 0 and 1; H = D = 1 (scale 1).  Rows 0 and 2 have ONE in-edge: a = 1, out = v[source] + skip, t = 0.
    Row 1 sees e = q_1 k_0 = 1 and e = q_1 k_1 = -2."""
    ip, ix = csr_from_edges(np.array([0, 0, 1, 1]), np.array([0, 1, 1, 2]), 3)
    assert ip.tolist() == [0, 1, 3, 4] and ix.tolist() == [0, 0, 1, 1]
    col = lambda *a: np.array(a, np.float64).reshape(3, 1, 1)
    q, k, v, s = col(0.5, 1.0, -1.0), col(1.0, -2.0, 0.5), col(3.0, -1.0, 7.0), col(0.1, 0.2, 0.3)
    y, c = to.attn_fwd(ip, ix, q, k, v, s, relu=False)
    a0 = 1.0 / (1.0 + math.exp(-3.0))
    a1 = 1.0 - a0
    np.testing.assert_allclose(c["e"][:, 0], [0.5, 1.0, -2.0, 2.0], rtol=1e-15)
    np.testing.assert_allclose(c["a"][:, 0], [1.0, a0, a1, 1.0], rtol=1e-14)
    np.testing.assert_allclose(y[:, 0, 0], [3.1, a0 * 3.0 - a1 + 0.2, -0.7], rtol=1e-14)
    np.testing.assert_allclose(c["lse"][:, 0], [0.5, 1.0 + math.log1p(math.exp(-3.0)), 2.0], rtol=1e-14)
    g = np.array([0.5, 1.0, -3.0])
    dq, dk, dv, ds, t = to.attn_bwd(c, g.reshape(3, 1))
    D = a0 * 3.0 + a1 * -1.0                                 # g_1 = 1: c_01 = v_0, c_11 = v_1; the skip row is no part of D
    t0, t1 = a0 * (3.0 - D), a1 * (-1.0 - D)
    np.testing.assert_allclose(t[:, 0], [0.0, t0, t1, 0.0], atol=1e-15)
    np.testing.assert_allclose(dq[:, 0, 0], [0.0, t0 * 1.0 + t1 * -2.0, 0.0], atol=1e-15)
    np.testing.assert_allclose(dk[:, 0, 0], [t0 * 1.0, t1 * 1.0, 0.0], atol=1e-15)
    np.testing.assert_allclose(dv[:, 0, 0], [0.5 + a0, a1 - 3.0, 0.0], rtol=1e-14)
    np.testing.assert_allclose(ds[:, 0, 0], g, rtol=0)                                    # ds = g
    assert abs(D - float((g[1] * (y[1] - s[1])).sum())) < 1e-14 and abs(D - float(g[1] * y[1, 0, 0])) > 0.1   # <g_i, r_i> is not D_i


def test_hand_answer_on_a_multi_edge_beside_a_degree_one_row():
    """Edges 0 -> 1 TWICE (equal scores: a = 1/2 each, each its own term and its own dropout draw) and 0 -> 2 once (a = 1 whatever the
    score); H = 1, D = 2 (scale 2^-1/2).  With the second copy and the lone edge dropped (p = 0.5): out_1 = (1/2) 2 v_0 + s_1,
    out_2 = s_2 -- but lse_2 is still the edge's score: a dropped edge stays in the softmax."""
    ip, ix = csr_from_edges(np.array([0, 0, 0, 0]), np.array([0, 1, 1, 2]), 3)
    q = np.array([[[0.0, 0.0]], [[1.0, 0.5]], [[-2.0, 3.0]]])
    k = np.array([[[1.0, -1.0]], [[9.0, 9.0]], [[9.0, 9.0]]])
    v = np.array([[[2.0, -4.0]], [[9.0, 9.0]], [[9.0, 9.0]]])
    s = np.array([[[0.5, 0.5]], [[1.0, 2.0]], [[-1.0, 4.0]]])
    mask = np.array([[1], [1], [0], [0]], np.uint8)
    y, c = to.attn_fwd(ip, ix, q, k, v, s, relu=False, attn_mask=mask, attn_p=0.5)
    np.testing.assert_allclose(c["a"][:, 0], [1.0, 0.5, 0.5, 1.0], rtol=1e-15)
    np.testing.assert_allclose(y[:, 0], [[4.5, -7.5], [3.0, -2.0], [-1.0, 4.0]], rtol=1e-15)
    np.testing.assert_allclose(c["lse"][2, 0], (-2.0 * 1.0 + 3.0 * -1.0) / math.sqrt(2.0), rtol=1e-15)
    np.testing.assert_allclose(c["lse"][1, 0], (1.0 - 0.5) / math.sqrt(2.0) + math.log(2.0), rtol=1e-15)
    # backward: c of the kept copy is 2 <g_1, v_0>, of the dropped copy 0; D_1 is their mean
    g = np.array([[1.0, 1.0], [1.0, 2.0], [5.0, 5.0]])
    dq, dk, dv, _, t = to.attn_bwd(c, g)
    ck = 2.0 * (1.0 * 2.0 + 2.0 * -4.0)
    np.testing.assert_allclose(t[:, 0], [0.0, 0.5 * (ck - ck / 2), 0.5 * (0.0 - ck / 2), 0.0], atol=1e-15)
    np.testing.assert_allclose(dq, 0.0, atol=1e-15)          # equal k on both copies: the two terms cancel; a lone edge has t = 0
    np.testing.assert_allclose(dk, 0.0, atol=1e-15)          # ... and equal q_1 on both
    np.testing.assert_allclose(dv[0, 0], 2.0 * g[0] + 0.5 * 2.0 * g[1], rtol=1e-15)      # kept self-loop, kept copy; nothing else
    # a row without in-edges: out = skip, lse = 0, dq = 0
    ip0, ix0 = csr_from_edges(np.array([0]), np.array([1]), 3)
    y0, c0 = to.attn_fwd(ip0, ix0, q, k, v, s, relu=False)
    np.testing.assert_array_equal(y0[[0, 2]], s[[0, 2]])
    assert c0["lse"][0, 0] == 0.0 and c0["lse"][2, 0] == 0.0
    assert not to.attn_bwd(c0, g)[0].any()


def _small_layer(seed, n=30, d_in=5, H=3, D=4):
    rs = np.random.RandomState(seed)
    ip, ix = random_graph(n, 3, seed=seed, self_loops=True, hub=12)
    p = {"heads": H}
    for lin in to.LINS:
        p[lin + ".weight"], p[lin + ".bias"] = rs.standard_normal((H * D, d_in)) * 0.5, rs.standard_normal(H * D) * 0.3
    x = rs.standard_normal((n, d_in))
    fm, am = (rs.rand(n, d_in) > 0.4).astype(np.uint8), (rs.rand(len(ix), H) > 0.3).astype(np.uint8)
    return ip, ix, p, x, fm, am, rs.standard_normal((n, H * D))


@pytest.mark.parametrize("relu", [False, True])
def test_oracle_backward_matches_finite_differences(relu):
    ip, ix, p, x, fm, am, gy = _small_layer(3)
    y, c = to.layer_fwd(ip, ix, x, p, relu, fm, 0.4, am, 0.3)
    assert not relu or np.abs(c["r"][c["r"] != 0]).min() > 1e-4            # no kink within reach of the step
    dx, grads = to.layer_bwd(c, gy)
    loss = lambda xx, pp: float((to.layer_fwd(ip, ix, xx, pp, relu, fm, 0.4, am, 0.3)[0] * gy).sum())
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


@pytest.mark.parametrize("H,D,relu", [(4, 2, True), (1, 7, False), (3, 5, True)])
def test_oracle_matches_torch_autograd_on_a_dense_restatement(H, D, relu):
    """A simple graph as a dense adjacency A[i, j] = [edge j -> i]: scores, softmax, masks and aggregation as [N, N, H] tensors in
    fp64, gradients by torch autograd."""
    n, d_in, pf, pa = 14, 5, 0.4, 0.3
    rs = np.random.RandomState(10 * H + D)
    A = (rs.rand(n, n) < 0.25) | np.eye(n, dtype=bool)
    dst, src = np.nonzero(A)
    ip, ix = csr_from_edges(src, dst, n)
    np.testing.assert_array_equal(ix, src)                                               # CSR order = row-major order of A
    p = {"heads": H}
    for lin in to.LINS:
        p[lin + ".weight"], p[lin + ".bias"] = rs.standard_normal((H * D, d_in)) * 0.5, rs.standard_normal(H * D) * 0.3
    x, gy = rs.standard_normal((n, d_in)), rs.standard_normal((n, H * D))
    fm, M = (rs.rand(n, d_in) > pf).astype(np.uint8), (rs.rand(n, n, H) > pa).astype(np.uint8)
    y, c = to.layer_fwd(ip, ix, x, p, relu, fm, pf, M[dst, src], pa)
    dx, grads = to.layer_bwd(c, gy)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in dict(p, x=x).items() if k != "heads"}
    h = t["x"] * torch.from_numpy(fm / (1 - pf))
    z = {lin: (h @ t[lin + ".weight"].T + t[lin + ".bias"]).view(n, H, D) for lin in to.LINS}
    e = torch.einsum("ihd,jhd->ijh", z["lin_query"], z["lin_key"]) / math.sqrt(D)
    e = e.masked_fill(torch.from_numpy(~A)[:, :, None], -math.inf)
    a = torch.softmax(e, dim=1) * torch.from_numpy(M / (1 - pa))
    out = torch.einsum("ijh,jhd->ihd", a, z["lin_value"]) + z["lin_skip"]
    out = torch.relu(out) if relu else out
    np.testing.assert_allclose(y, out.detach().numpy().reshape(n, -1), rtol=1e-12, atol=1e-13)
    out.reshape(n, -1).backward(torch.from_numpy(gy))
    np.testing.assert_allclose(dx, t["x"].grad.numpy(), rtol=1e-10, atol=1e-12)
    for k, v in grads.items():
        np.testing.assert_allclose(v, t[k].grad.numpy().reshape(v.shape), rtol=1e-10, atol=1e-12, err_msg=k)


def test_fp32_mode_runs_the_same_arithmetic_in_fp32():
    ip, ix, p, x, fm, am, gy = _small_layer(4)
    y, c = to.layer_fwd(ip, ix, x, p, True, fm, 0.4, am, 0.3)
    y32, c32 = to.layer_fwd(ip, ix, x, p, True, fm, 0.4, am, 0.3, dtype=np.float32)
    assert y32.dtype == np.float32 and c32["a"].dtype == np.float32 and to.layer_bwd(c32, gy)[0].dtype == np.float32
    err = np.abs(y32 - y).max()
    assert 0 < err < 1e-5


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def _conf(**kw):
    return dict(dict(model_name="GraphTransformer", num_layers=2, feat_dim=8, hidden_dim=16, label_dim=4, dropout_ratio=0.0,
                     norm_type="none", device="cpu", num_heads=4, attn_dropout_ratio=0.1), **kw)


def test_teacher_kind_and_the_order_of_the_keys():
    from glnn_amd import kinds, models
    assert models.teacher_kind("GraphTransformer") == "gt" and "gt" in models.FULL_GRAPH_KINDS
    keys = [row.key for row in kinds.KINDS]
    assert all(k == "GraphTransformer" or (k not in "GraphTransformer" and "GraphTransformer" not in k) for k in keys)
    for name, kind in (("DAGNN", "dagnn"), ("GPRGNN", "gpr"), ("GCNII", "gcnii"), ("GCN", "gcn"), ("GATv2", "gatv2"), ("GAT", "gat"),
                       ("APPNP", "appnp"), ("SAGE", "sage"), ("MLP3w4", "mlp")):
        assert models.teacher_kind(name) == kind
    assert models.teacher_kind("GA1GraphTransformer") == "gt"                # the feature-augmentation prefix
    with pytest.raises(ValueError, match="Unknown model_name"):
        models.teacher_kind("GraphTransforme")


def test_state_dict_keys_shapes_and_init_rng_stream():
    """Keys encoder.layers.{i}.lin_{key,query,value,skip}.weight|bias.  Per layer four nn.Linear constructors draw, in that order, with
    torch's default initialisation; nothing is redrawn."""
    from glnn_amd import models
    torch.manual_seed(7)
    m = models.Model(_conf(num_layers=3))
    assert type(m.encoder) is models.GraphTransformer and isinstance(m.encoder, models._AttnStack) and m.kind == "gt"
    sd = m.state_dict()
    shapes = {0: (8, 4, 4), 1: (16, 4, 4), 2: (16, 1, 4)}                  # layer: (in, heads, out)
    assert set(sd) == {f"encoder.layers.{l}.{k}" for l in range(3) for k in to.KEYS}
    assert list(sd)[:8] == [f"encoder.layers.0.{k}" for k in to.KEYS]        # the registration order is the construction order
    torch.manual_seed(7)
    for l, (d_in, H, D) in shapes.items():
        for lin in to.LINS:
            want = torch.nn.Linear(d_in, H * D)
            assert tuple(sd[f"encoder.layers.{l}.{lin}.weight"].shape) == (H * D, d_in)
            assert tuple(sd[f"encoder.layers.{l}.{lin}.bias"].shape) == (H * D,)
            assert torch.equal(sd[f"encoder.layers.{l}.{lin}.weight"], want.weight) and torch.equal(sd[f"encoder.layers.{l}.{lin}.bias"],
                                                                                                  want.bias), (l, lin)
    lay = m.encoder.layers
    assert lay[0].attn_drop.p == 0.1 and lay[2]._num_heads == 1 and lay[2].activation is None and lay[0]._out_feats == 4
    assert not hasattr(lay[0], "attn") and not hasattr(lay[0], "beta")


def test_conf_contract_is_gats():
    from glnn_amd import models
    base = {k: v for k, v in _conf().items() if k not in ("num_heads", "attn_dropout_ratio")}
    with pytest.raises(NotImplementedError, match="GraphTransformer.*num_heads"):
        models.Model(dict(base, attn_dropout_ratio=0.1))
    with pytest.raises(NotImplementedError, match="GraphTransformer.*attn_dropout_ratio"):
        models.Model(dict(base, num_heads=4))
    with pytest.raises(ValueError, match="GraphTransformer.*multiple"):
        models.Model(_conf(num_heads=3))
    with pytest.raises(ValueError, match="GraphTransformer.*multiple"):
        models.Model(_conf(hidden_dim=2))
    models.Model(_conf(negative_slope=0.3))                                  # accepted, unused


def test_out_of_scope_configurations_raise_naming_the_class():
    from glnn_amd import dist, models
    from glnn_amd.nn import TransformerConv
    with pytest.raises(NotImplementedError, match="GraphTransformer.*num_layers"):
        models.Model(_conf(num_layers=1))
    m = models.Model(_conf())
    with pytest.raises(NotImplementedError, match="not implemented for the GraphTransformer teacher"):   # bf16 activation storage
        m.inference(None, torch.zeros(4, 8), dtype=torch.bfloat16)
    for cls in (dist.ShardedTeacher, dist.HaloShardedTeacher):
        with pytest.raises(NotImplementedError, match="GraphTransformer teacher is not sharded.*key and value rows"):
            cls(m.encoder, None, None, None)
    from glnn_amd.kinds import BY_KEY
    assert "key and value rows" in BY_KEY["GraphTransformer"].unsharded       # the table refuses it with its own phrase
    with pytest.raises(NotImplementedError, match="TransformerConv.*bipartite"):
        TransformerConv((8, 8), 4, 2)
    with pytest.raises(NotImplementedError, match="TransformerConv.*residual"):
        TransformerConv(8, 4, 2, residual=True)
    with pytest.raises(NotImplementedError, match="GraphTransformer.*residual"):
        models.GraphTransformer(3, 8, 16, 4, 0.0, torch.nn.functional.relu, residual=True)
    with pytest.raises(NotImplementedError, match="TransformerConv.*num_heads <= 64"):
        TransformerConv(8, 1, 65)
    with pytest.raises(NotImplementedError, match="TransformerConv.*256"):
        TransformerConv(8, 257, 1)
    with pytest.raises(NotImplementedError, match="TransformerConv.*activation"):
        TransformerConv(8, 4, 2, activation=torch.tanh)
    TransformerConv(8, 4, 64)                                                # 64 heads of 4: the limit itself is accepted
    lay = TransformerConv(8, 4, 2)
    with pytest.raises(NotImplementedError, match="TransformerConv.*bipartite"):
        lay([None, None], torch.zeros(4, 8))


def test_engine_step_and_check_supported(monkeypatch):
    from glnn_amd import models, ops, teacher
    from glnn_amd.train_and_eval import _full_graph_step
    monkeypatch.setattr(ops, "TensorTable", lambda *a: None)               # the engine's only GPU-bound member
    m = models.Model(_conf(dropout_ratio=0.25))
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    eng = teacher.TeacherEngine(m, opt)
    assert eng.kind == "gt" and eng.p == 0.25 and _full_graph_step(eng, "GraphTransformer") == eng.step_gt
    with pytest.raises(RuntimeError, match="needs the model on the GPU"):    # accepted up to the last check (the device)
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    m.encoder.layers[0].activation = None                                    # behind the constructor's back
    with pytest.raises(NotImplementedError, match="GraphTransformer with ReLU hidden layers"):
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)


def test_cli_and_training_config(tmp_path, capsys):
    import yaml
    from glnn_amd.cli import _training_config, get_student_args, get_teacher_args
    from glnn_amd.utils import get_training_config
    assert get_teacher_args(["--teacher", "GraphTransformer"]).teacher == "GraphTransformer"
    assert get_teacher_args(["--teacher", "GraphTransformer", "--subgraph_walk_length", "3"]).subgraph_walk_length == 3
    assert get_student_args(["--teacher", "GraphTransformer", "--student", "MLP"]).teacher == "GraphTransformer"
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "SAGE", "--subgraph_walk_length", "3"])
    assert "GraphTransformer" in capsys.readouterr().err                     # the refusal lists the full-graph teachers
    path = os.path.join(ROOT, "train.conf.yaml")
    conf = _training_config(path, "GraphTransformer", "cora")                # no section of its own: GATv2's stands in
    v2 = get_training_config(path, "GATv2", "cora")
    assert conf == dict(v2, model_name="GraphTransformer") and conf["num_heads"] == 8 and conf["attn_dropout_ratio"] == 0.3
    assert _training_config(path, "GCN", "cora") == get_training_config(path, "GCN", "cora")
    assert _training_config(path, "DAGNN", "cora")["model_name"] == "DAGNN" and "num_heads" not in _training_config(path, "DAGNN", "cora")
    cfg = {"global": {"learning_rate": 0.01}, "only-gat": {"GAT": {"num_heads": 2, "attn_dropout_ratio": 0.5}, "MLP": {}},
           "own": {"GraphTransformer": {"num_heads": 4, "attn_dropout_ratio": 0.1}, "GATv2": {"num_heads": 8, "attn_dropout_ratio": 0.3}},
           "neither": {"MLP": {"hidden_dim": 8}, "GATv2": None}}
    tmp = tmp_path / "conf.yaml"
    tmp.write_text(yaml.safe_dump(cfg))
    assert _training_config(str(tmp), "GraphTransformer", "only-gat") == {"learning_rate": 0.01, "num_heads": 2, "attn_dropout_ratio": 0.5,
                                                                           "model_name": "GraphTransformer"}
    assert _training_config(str(tmp), "GraphTransformer", "own")["num_heads"] == 4
    with pytest.raises(ValueError, match="num_heads and attn_dropout_ratio"):
        _training_config(str(tmp), "GraphTransformer", "neither")


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
    fwd = lambda n, nnz, H=2, D=4: h.glnn_gt_attn_fwd_f32(None, None, n, nnz, None, 8, None, 8, None, 8, None, 8, H, D, 0.0, 0, 0, None, 8,
                                                          None, None)
    bwd = lambda n, nnz, H=2, D=4: h.glnn_gt_attn_bwd_f32(None, None, None, None, None, n, nnz, None, 8, None, 8, None, 8, H, D, None, None, 8,
                                                          0.0, 0, None, None, 8, None, 8, None, 8, None, 0, None)
    for call in (fwd, bwd):
        assert call(4, 4) == -1 and b"null pointer" in h.glnn_last_error()
        assert call(0, 0) == 0                                              # empty inputs: a no-op
        assert call(4, 1 << 31) == -2 and b"2^31" in h.glnn_last_error()
        assert call(4, 4, 65, 1) == -2 and b"heads <= 64" in h.glnn_last_error()
        assert call(4, 4, 1, 257) == -2 and b"256" in h.glnn_last_error()
        assert call(4, 4, 0, 4) == -1
    assert h.glnn_gt_attn_bwd_workspace_floats(700, 8) == 700 * 8 and h.glnn_gt_attn_bwd_workspace_floats(0, 8) == 0
    assert h.glnn_gt_attn_fwd_f32(None, None, 4, 4, None, 8, None, 8, None, 8, None, 8, 2, 4, 1.0, 0, 0, None, 8, None, None) == -1
    assert b"attn_drop" in h.glnn_last_error()


def test_ops_refuse_cpu_tensors():
    from glnn_amd import GlnnError, ops
    z = torch.zeros(3, 8)
    ip, ix = torch.arange(4, dtype=torch.int64), torch.arange(3, dtype=torch.int32)
    with pytest.raises(GlnnError):
        ops.gt_attn_fwd(ip, ix, 3, z, z, z, z, 2, 4)
