"""CPU checks of the PNA teacher: the fp64 oracle (tests/pna_oracle.py) by hand answers on graphs of at most 8 nodes and by finite
differences; the name's resolution; the state-dict keys, shapes, the init RNG stream and the delta buffer; every refusal; the command line,
the training config's stand-in section and the computed delta; the exported symbols and their argument checks.  No GPU call is made."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import pna_oracle as po
from graphgen import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glnn_pna_agg_fwd_f32", "glnn_pna_agg_bwd_f32", "glnn_pna_scale_fwd_f32", "glnn_pna_scale_bwd_f32", "glnn_pna_da_f32")
S0 = math.sqrt(1e-5)


def _csr(indptr, indices):
    return np.asarray(indptr, np.int64), np.asarray(indices, np.int32)


def _col(*a):
    return np.array(a, np.float64).reshape(-1, 1)


def _ds(n, **parts):
    """dS [n, 4, 1] with the named parts (mean, mn, mx, sd) set from per-row lists."""
    ds = np.zeros((n, 4, 1))
    for k, v in parts.items():
        ds[:, ("mean", "mn", "mx", "sd").index(k), 0] = v
    return ds


# ---------------------------------------------------------------------------------------------------------------- the oracle, by hand
def test_hand_answer_on_a_path_with_an_isolated_row_and_single_neighbour_rows():
    """0 -> 1 -> 2 -> 3: row 0 has no in-edge (S = [0, 0, 0, sqrt(1e-5)], no a term, argument -1); every other row has ONE neighbour, so
    mean = min = max = b[u], sigma = sqrt(1e-5) and the gradient through sigma is exactly 0."""
    ip, ix = _csr([0, 0, 1, 2, 3], [0, 1, 2])
    b, a = _col(1.0, 2.0, 4.0, 8.0), _col(10.0, 20.0, 30.0, 40.0)
    s, mu, arg = po.agg_fwd(ip, ix, b, a)
    np.testing.assert_array_equal(s[0, :, 0], [0.0, 0.0, 0.0, S0])
    np.testing.assert_array_equal(s[1:, :, 0], [[21.0, 21.0, 21.0, S0], [32.0, 32.0, 32.0, S0], [44.0, 44.0, 44.0, S0]])
    np.testing.assert_array_equal(mu[:, 0], [0.0, 1.0, 2.0, 4.0])
    np.testing.assert_array_equal(arg[:, :, 0], [[-1, -1], [0, 0], [1, 1], [2, 2]])
    db = po.agg_bwd(ip, ix, _ds(4, sd=[5.0, 7.0, 11.0, 13.0]), b, mu, s[:, 3], arg)
    np.testing.assert_array_equal(db, np.zeros((4, 1)))                       # b[u] - mu is exactly 0 on a single-neighbour row
    db = po.agg_bwd(ip, ix, _ds(4, mean=[9.0, 1.0, 2.0, 3.0], mn=[9.0, 0.5, 0.0, 0.0], mx=[9.0, 0.0, 0.25, 0.0]), b, mu, s[:, 3], arg)
    np.testing.assert_array_equal(db[:, 0], [1.5, 2.25, 3.0, 0.0])            # row 0's dS reaches nobody; source 3 has no out-edge


def test_hand_answer_on_a_triple_edge_the_gradient_arrives_once():
    """Row 1 = {0, 0, 0, 2} (CSR positions 0..3) with b_0 = 3, b_2 = 1: mean 2.5, E b^2 = 7, var 0.75; max at position 0, the FIRST of the
    three copies, min at position 3.  g_max = 1 gives source 0 the gradient once, not three times."""
    ip, ix = _csr([0, 0, 4, 4], [0, 0, 0, 2])
    b = _col(3.0, -5.0, 1.0)
    s, mu, arg = po.agg_fwd(ip, ix, b)
    np.testing.assert_allclose(s[1, :, 0], [2.5, 1.0, 3.0, math.sqrt(0.75 + 1e-5)], rtol=1e-15)
    assert arg[1, :, 0].tolist() == [3, 0]
    db = po.agg_bwd(ip, ix, _ds(3, mx=[0, 1.0, 0]), b, mu, s[:, 3], arg)
    np.testing.assert_array_equal(db[:, 0], [1.0, 0.0, 0.0])
    db = po.agg_bwd(ip, ix, _ds(3, mean=[0, 4.0, 0], mn=[0, 2.0, 0]), b, mu, s[:, 3], arg)
    np.testing.assert_array_equal(db[:, 0], [3.0, 0.0, 1.0 + 2.0])             # the mean reaches every COPY: 3 x 4 / 4
    sg = math.sqrt(0.75 + 1e-5)
    db = po.agg_bwd(ip, ix, _ds(3, sd=[0, 1.0, 0]), b, mu, s[:, 3], arg)
    np.testing.assert_allclose(db[:, 0], [3 * 0.5 / (4 * sg), 0.0, -1.5 / (4 * sg)], rtol=1e-15)


def test_hand_answer_on_a_self_loop():
    """Row 0 = {0 (itself), 1} with b = (2, 6): mean 4, var 4; the min is the row's own value, so g_min comes back to row 0 as a source."""
    ip, ix = _csr([0, 2, 2], [0, 1])
    b = _col(2.0, 6.0)
    s, mu, arg = po.agg_fwd(ip, ix, b, _col(0.5, 0.25))
    np.testing.assert_allclose(s[0, :, 0], [4.5, 2.5, 6.5, math.sqrt(4.0 + 1e-5)], rtol=1e-15)
    np.testing.assert_array_equal(s[1, :, 0], [0.0, 0.0, 0.0, S0])            # row 1 has no in-edge: no a term either
    assert arg[0, :, 0].tolist() == [0, 1]
    db = po.agg_bwd(ip, ix, _ds(2, mn=[1.0, 0.0], mx=[0.5, 0.0]), b, mu, s[:, 3], arg)
    np.testing.assert_array_equal(db[:, 0], [1.0, 0.5])


def test_hand_answer_on_an_exact_tie_between_two_sources():
    """Row 0 = {1, 2, 3} with b_1 = b_2 = 7 > b_3: the lower CSR position (source 1) takes the WHOLE gradient of max; torch's amax would
    give each half.  min_gap sees the tie as a gap of 0."""
    ip, ix = _csr([0, 3, 3, 3, 3], [1, 2, 3])
    b = _col(0.0, 7.0, 7.0, -1.0)
    s, mu, arg = po.agg_fwd(ip, ix, b)
    assert arg[0, :, 0].tolist() == [2, 0] and s[0, 2, 0] == 7.0
    db = po.agg_bwd(ip, ix, _ds(4, mx=[1.0, 0, 0, 0]), b, mu, s[:, 3], arg)
    np.testing.assert_array_equal(db[:, 0], [0.0, 1.0, 0.0, 0.0])
    t = torch.tensor([7.0, 7.0, -1.0], dtype=torch.float64, requires_grad=True)
    t.amax().backward()
    assert t.grad.tolist() == [0.5, 0.5, 0.0]                                # the rule the oracle does NOT follow
    c = dict(b=b, indptr=ip, indices=ix, arg=arg)
    assert po.min_gap([c]) == 0.0
    c2 = dict(c, b=_col(0.0, 7.0, 6.0, -1.0))
    c2["arg"] = po.agg_fwd(ip, ix, c2["b"])[2]
    assert po.min_gap([c2]) == pytest.approx(1.0 / 7.0)                       # max: 7 against 6; min: -1 against 6; over max |b| = 7


def test_hand_answer_of_one_layer_row():
    """F = Fo = 1 on 1 -> 0 <- 2: every term of out[0] = post([x' || S || s_amp S || s_att S]) written out in plain arithmetic."""
    ip, ix = _csr([0, 2, 2, 2], [1, 2])
    x = _col(1.0, 2.0, -4.0)
    wo = np.arange(1, 14, dtype=np.float64).reshape(1, 13) / 10.0
    p = {"pre.weight": np.array([[0.5, 2.0]]), "pre.bias": np.array([0.25]), "post.weight": wo, "post.bias": np.array([-0.75])}
    delta = 0.8
    y, c = po.layer_fwd(ip, ix, x, p, delta, relu=False)
    a0 = 0.5 * 1.0 + 0.25
    b1, b2 = 4.0, -8.0
    mean, var = -2.0, (16.0 + 64.0) / 2 - 4.0
    S = [a0 + mean, a0 + b2, a0 + b1, math.sqrt(var + 1e-5)]
    amp = math.log(3.0) / delta
    want = 0.1 * 1.0 - 0.75 + sum(wo[0, 1 + k * 4 + q] * sc * S[q] for k, sc in enumerate((1.0, amp, 1.0 / amp)) for q in range(4))
    assert y[0, 0] == pytest.approx(want, rel=1e-14)
    amp0 = math.log(2.0) / delta                                              # deg 0: the scalers of max(deg, 1) = 1
    want1 = 0.1 * 2.0 - 0.75 + S0 * (wo[0, 4] + amp0 * wo[0, 8] + wo[0, 12] / amp0)
    assert y[1, 0] == pytest.approx(want1, rel=1e-14)
    dx, grads = po.layer_bwd(c, np.array([[1.0], [0.0], [0.0]]))
    assert grads["post.bias"][0] == 1.0 and grads["post.weight"][0, 0] == 1.0
    np.testing.assert_allclose(grads["post.weight"][0, 1:5], S, rtol=1e-14)
    g_mean, g_mn, g_mx, g_sd = (wo[0, 1 + q] + amp * wo[0, 5 + q] + wo[0, 9 + q] / amp for q in range(4))
    assert grads["pre.bias"][0] == pytest.approx(g_mean + g_mn + g_mx, rel=1e-14)
    db1 = g_mean / 2 + g_sd * (b1 - mean) / (2 * S[3]) + g_mx
    db2 = g_mean / 2 + g_sd * (b2 - mean) / (2 * S[3]) + g_mn
    np.testing.assert_allclose(dx[:, 0], [0.1 + 0.5 * (g_mean + g_mn + g_mx), 2.0 * db1, 2.0 * db2], rtol=1e-13)


def _small_problem(seed, n=8, hidden=4, feat=5, label=3, layers=2):
    rs = np.random.RandomState(seed)
    ip, ix = random_graph(n, 3, seed=seed, isolated=1)
    params = po.random_params(rs, layers, feat, hidden, label, np.float64)
    x = rs.standard_normal((n, feat))
    return ip, ix, params, x, rs.randint(0, label, n), np.arange(0, n, 2)


def test_the_oracles_backward_against_finite_differences():
    """The explicit backward of a whole training loss (two layers, ReLU, NLL) against central differences, on inputs whose min_gap is
    six orders above the step: no argument can flip inside the stencil."""
    ip, ix, params, x, labels, idx = _small_problem(3)
    assert (np.diff(ip) == 0).any() and np.diff(ip).max() >= 3
    caches = po.loss_grads(params, ip, ix, x, labels, idx, 2, 0.9)[3]["layers"]
    gap = po.min_gap(caches)
    assert gap > 1e-3, gap
    worst = po.fd_check(params, ip, ix, x, labels, idx, 2, 0.9, h=1e-6)
    print(f"min_gap {gap:.3e}, worst relative finite-difference error {worst:.3e}")
    assert worst < 1e-5


def test_fp32_arithmetic_of_the_oracle_stays_near_its_fp64():
    ip, ix, params, x, labels, idx = _small_problem(4)
    l64, g64 = po.loss_grads(params, ip, ix, x, labels, idx, 2, 0.9)[:2]
    l32, g32 = po.loss_grads(params, ip, ix, x, labels, idx, 2, 0.9, dtype=np.float32)[:2]
    assert abs(l32 - l64) < 1e-5 and all(g32[k].dtype == np.float32 and np.abs(g32[k] - g64[k]).max() < 1e-4 for k in g64)


# ---------------------------------------------------------------------------------------------------------------- the surface
def _conf(**kw):
    return dict(dict(model_name="PNA", num_layers=2, feat_dim=8, hidden_dim=16, label_dim=4, dropout_ratio=0.0, norm_type="none",
                     device="cpu", pna_delta=1.25), **kw)


def test_teacher_kind_and_the_key_containment_rule():
    from glnn_amd import kinds, models
    assert models.teacher_kind("PNA") == "pna" and models.teacher_kind("GA1PNA") == "pna" and "pna" in models.FULL_GRAPH_KINDS
    keys = [row.key for row in kinds.KINDS]
    assert all(k == "PNA" or (k not in "PNA" and "PNA" not in k) for k in keys)
    for name, kind in (("APPNP", "appnp"), ("GraphTransformer", "gt"), ("DAGNN", "dagnn"), ("GPRGNN", "gpr"), ("GCNII", "gcnii"),
                       ("GCN", "gcn"), ("GATv2", "gatv2"), ("GAT", "gat"), ("SAGE", "sage"), ("MLP3w4", "mlp")):
        assert models.teacher_kind(name) == kind
    assert "PNA" in models.teacher_kind.__doc__
    with pytest.raises(ValueError, match="Unknown model_name"):
        models.teacher_kind("PN")


def test_state_dict_keys_shapes_init_rng_stream_and_delta():
    from glnn_amd import models
    torch.manual_seed(7)
    m = models.Model(_conf(num_layers=2))
    assert type(m.encoder) is models.PNA and m.kind == "pna"
    sd = m.state_dict()
    want_keys = (["encoder.fc_in.weight", "encoder.fc_in.bias"]
                 + [f"encoder.layers.{l}.{k}" for l in range(2) for k in po.LAYER_KEYS] + ["encoder.fc_out.weight", "encoder.fc_out.bias"])
    assert [k for k in sd if k != "encoder.delta"] == want_keys and "encoder.delta" in sd      # registration = construction order
    torch.manual_seed(7)
    lins = [("encoder.fc_in", torch.nn.Linear(8, 16))]
    for l in range(2):
        lins += [(f"encoder.layers.{l}.pre", torch.nn.Linear(32, 16)), (f"encoder.layers.{l}.post", torch.nn.Linear(13 * 16, 16))]
    lins.append(("encoder.fc_out", torch.nn.Linear(16, 4)))
    for name, want in lins:
        assert torch.equal(sd[name + ".weight"], want.weight) and torch.equal(sd[name + ".bias"], want.bias), name
    assert tuple(sd["encoder.layers.1.post.weight"].shape) == (16, 208) and tuple(sd["encoder.layers.0.pre.weight"].shape) == (16, 32)
    assert sd["encoder.delta"].dtype == torch.float64 and float(sd["encoder.delta"]) == 1.25
    assert [n for n, _ in m.named_parameters()] == want_keys                 # delta is a buffer: Adam never sees it
    m2 = models.Model(_conf(pna_delta=0.5))
    m2.load_state_dict(sd)
    assert float(m2.encoder.delta) == 1.25 and all(lay.delta == 1.25 for lay in m2.encoder.layers)      # the loaded constant is the one used
    assert all(lay.feat_drop.p == 0.0 and lay.activation is not None for lay in m.encoder.layers)


def test_missing_delta_wide_hidden_and_norms_raise_naming_pna():
    from glnn_amd import dist, models, ops
    from glnn_amd.nn import PNAConv
    with pytest.raises(ValueError, match="PNA.*pna_delta"):
        models.Model({k: v for k, v in _conf().items() if k != "pna_delta"})
    with pytest.raises(ValueError, match="PNA.*pna_delta"):
        models.Model(_conf(pna_delta=None))
    with pytest.raises(ValueError, match="PNA.*positive"):
        models.Model(_conf(pna_delta=0.0))
    assert ops.PNA_MAX_WIDTH == 256
    with pytest.raises(NotImplementedError, match="PNA: hidden_dim of at most 256"):
        models.Model(_conf(hidden_dim=257))
    models.Model(_conf(hidden_dim=256))
    for norm in ("batch", "layer"):
        with pytest.raises(NotImplementedError, match="PNA: norm_type 'none' only"):
            models.Model(_conf(norm_type=norm))
    with pytest.raises(NotImplementedError, match="PNAConv.*256"):
        PNAConv(257, 8, 1.0)
    with pytest.raises(NotImplementedError, match="PNAConv.*activation"):
        PNAConv(8, 8, 1.0, activation=torch.tanh)
    PNAConv(8, 300, 1.0)                                                     # any output width
    m = models.Model(_conf())
    with pytest.raises(NotImplementedError, match="not implemented for the PNA teacher"):
        m.inference(None, torch.zeros(4, 8), dtype=torch.bfloat16)
    for cls in (dist.ShardedTeacher, dist.HaloShardedTeacher):
        with pytest.raises(NotImplementedError, match="PNA teacher is not sharded.*min, max and std"):
            cls(m.encoder, None, None, None)
    with pytest.raises(NotImplementedError, match="PNAConv.*bipartite"):
        m.encoder.layers[0]([None, None], torch.zeros(4, 16))


def test_engine_step_and_check_supported(monkeypatch):
    from glnn_amd import models, ops, teacher
    from glnn_amd.train_and_eval import _full_graph_step
    monkeypatch.setattr(ops, "TensorTable", lambda *a: None)               # the engine's only GPU-bound member
    m = models.Model(_conf(dropout_ratio=0.25))
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    eng = teacher.TeacherEngine(m, opt)
    assert eng.kind == "pna" and eng.p == 0.25 and _full_graph_step(eng, "PNA") == eng.step_pna
    assert len({eng._pna_seed(s, step=1) for s in range(4)} | {eng._pna_seed(s, step=2) for s in range(4)}) == 8
    with pytest.raises(RuntimeError, match="needs the model on the GPU"):    # accepted up to the last check (the device)
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    m.encoder.norm_type = "batch"                                            # behind the constructor's back
    with pytest.raises(NotImplementedError, match="PNA with norm_type none"):
        teacher.check_supported(m, torch.nn.NLLLoss(), opt)


def test_cli_flag_stand_in_section_and_delta(tmp_path, capsys):
    import yaml
    from glnn_amd.cli import _training_config, get_student_args, get_teacher_args, pna_delta
    from glnn_amd.kinds import BY_KIND
    from glnn_amd.graph import CSRGraph
    from glnn_amd.utils import get_training_config
    args = get_teacher_args(["--teacher", "PNA", "--pna_delta", "1.5"])
    assert args.teacher == "PNA" and args.pna_delta == 1.5
    assert get_teacher_args(["--teacher", "PNA"]).pna_delta is None
    assert get_teacher_args(["--teacher", "PNA", "--subgraph_walk_length", "3"]).subgraph_walk_length == 3
    assert get_student_args(["--teacher", "PNA", "--student", "MLP"]).teacher == "PNA"
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "GCN", "--pna_delta", "1.5"])
    assert "--pna_delta applies to the PNA teacher only" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "PNA", "--pna_delta", "0"])
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "SAGE", "--subgraph_walk_length", "3"])
    assert "PNA" in capsys.readouterr().err                                  # the refusal lists the full-graph teachers
    assert BY_KIND["pna"].stand_ins == ("GCN",) and BY_KIND["pna"].global_alone
    path = os.path.join(ROOT, "train.conf.yaml")
    conf = _training_config(path, "PNA", "cora")                             # no section of its own: GCN's stands in
    assert conf == dict(get_training_config(path, "GCN", "cora"), model_name="PNA")
    cfg = {"global": {"learning_rate": 0.01, "num_layers": 2}, "no-gcn": {"MLP": {"hidden_dim": 8}},
           "own": {"PNA": {"hidden_dim": 64}, "GCN": {"hidden_dim": 32}}}
    tmp = tmp_path / "conf.yaml"
    tmp.write_text(yaml.safe_dump(cfg))
    assert _training_config(str(tmp), "PNA", "no-gcn") == {"learning_rate": 0.01, "num_layers": 2, "model_name": "PNA"}   # global alone
    assert _training_config(str(tmp), "PNA", "own")["hidden_dim"] == 64
    ip = torch.tensor([0, 0, 1, 4, 4, 6], dtype=torch.int64)
    g = CSRGraph(ip, torch.tensor([0, 0, 1, 4, 2, 3], dtype=torch.int32), 5)
    assert pna_delta(g) == float(np.mean(np.log(np.array([0, 1, 3, 0, 2], np.float64) + 1.0)))


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
    assert "GLNN_PNA_MAX_WIDTH 256" in src


def test_entries_report_bad_arguments_before_any_launch():
    from glnn_amd import _lib
    h = _lib.lib()
    fwd = lambda n, nnz, d=8: h.glnn_pna_agg_fwd_f32(None, None, n, 4, nnz, None, 8, d, None, 8, None, 32, None, 8, None, 16, None)
    bwd = lambda n, nnz, d=8: h.glnn_pna_agg_bwd_f32(None, 4, None, None, None, n, nnz, None, 32, None, 8, d, None, 8, None, 8, None, 16,
                                                     None, 8, None)
    for call in (fwd, bwd):
        assert call(4, 4) == -1 and b"null pointer" in h.glnn_last_error()
        assert call(0, 0) == 0                                              # empty inputs: a no-op
        assert call(4, 1 << 31) == -2 and b"2^31" in h.glnn_last_error()
        assert call(4, 4, 257) == -2 and b"256" in h.glnn_last_error()
        assert call(4, 4, 0) == -1 and call(-1, 0) == -1
    one = ctypes.c_void_p(16)                                                # a non-null, aligned address that is never read
    assert h.glnn_pna_agg_fwd_f32(one, one, 4, 4, 4, one, 6, 8, None, 8, one, 32, None, 8, None, 16, None) == -1      # ldb % 4
    assert b"leading" in h.glnn_last_error()
    assert h.glnn_pna_agg_fwd_f32(one, one, 4, 4, 4, one, 8, 8, None, 8, one, 28, None, 8, None, 16, None) == -1      # lds < 4 round4(d)
    assert b"4 round4(d)" in h.glnn_last_error()
    assert h.glnn_pna_agg_fwd_f32(one, one, 4, 4, 4, one, 8, 8, None, 8, one, 32, one, 8, None, 16, None) == -1       # mu without arg
    assert b"go together" in h.glnn_last_error()
    assert h.glnn_pna_scale_fwd_f32(None, 4, 8, 1.0, None, 24, None, 8, 0, None) == -1 and b"null pointer" in h.glnn_last_error()
    assert h.glnn_pna_scale_fwd_f32(one, 4, 8, 0.0, one, 24, one, 8, 0, None) == -1 and b"delta" in h.glnn_last_error()
    assert h.glnn_pna_scale_bwd_f32(one, 4, 8, 1.0, one, 8, one, 20, None) == -1 and b"lddz" in h.glnn_last_error()
    assert h.glnn_pna_da_f32(one, 4, 8, one, 24, one, 8, None) == -1 and b"ldds" in h.glnn_last_error()
    assert h.glnn_pna_scale_fwd_f32(None, 0, 8, 1.0, None, 24, None, 8, 0, None) == 0
    assert h.glnn_pna_scale_bwd_f32(None, 0, 8, 1.0, None, 8, None, 24, None) == 0 and h.glnn_pna_da_f32(None, 0, 8, None, 32, None, 8, None) == 0


def test_ops_refuse_cpu_tensors_and_wide_rows():
    from glnn_amd import GlnnError, ops
    ip, ix = torch.arange(4, dtype=torch.int64), torch.arange(3, dtype=torch.int32)
    with pytest.raises(GlnnError):
        ops.pna_agg_fwd(ip, ix, 3, torch.zeros(3, 8), 3)
    assert ops.PNA_AGGREGATORS == ("mean", "min", "max", "std") and ops.PNA_SCALERS == ("identity", "amplification", "attenuation")
