"""GAT teacher, CPU side: the fp64 oracle (tests/gat_oracle.py) against the reference's golden (tests/golden/gat_teacher.npz), the
oracle's explicit backward against torch autograd on the same formulas in fp64, the C entries in header and binding table, and the
Model dispatch contract."""
import os
import re

import numpy as np
import pytest
import torch

import gat_oracle as go
from graphgen import planted_graph, random_graph, segment_reduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gat_teacher.npz")
ENTRIES = ("glnn_gat_scores_f32", "glnn_gat_attn_fwd_f32", "glnn_gat_attn_bwd_f32", "glnn_gat_attn_bwd_workspace_floats",
           "glnn_gat_attn_mask_u8")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _params(gold, pre="init."):
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


def _masks(gold, tag, L=2):
    n, nnz, H = len(gold["indptr"]) - 1, len(gold["indices"]), int(gold["num_heads"])
    dims = [int(d) for d in gold["dims"]]
    ins, heads = [dims[0], dims[1]], [H, 1]
    fm = [np.unpackbits(gold[f"{tag}.feat_mask{l}"])[:n * ins[l]].reshape(n, ins[l]) for l in range(L)]
    am = [np.unpackbits(gold[f"{tag}.attn_mask{l}"])[:nnz * heads[l]].reshape(nnz, heads[l]) for l in range(L)]
    return fm, am


def test_golden_graph_has_the_shapes_the_kernels_branch_on(gold):
    ip, ix = gold["indptr"], gold["indices"]
    deg = np.diff(ip)
    assert deg.min() >= 1 and deg.max() > 128 and int(gold["zero_in_degree_raises"]) == 1
    out_deg = np.bincount(ix, minlength=len(deg))
    assert out_deg.max() > 128 and ((out_deg > 64) & (out_deg <= 128)).any()           # long and two-chunk rows of the transposed CSR
    dst = np.repeat(np.arange(len(ip) - 1), deg)
    pairs = np.stack([ix.astype(np.int64), dst], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                                   # a multi-edge
    src_set = set(map(tuple, pairs))
    assert any((d, s) not in src_set for s, d in src_set)                                # non-symmetric
    assert set(_params(gold)) == {f"encoder.layers.{l}.{k}" for l in range(2) for k in ("fc.weight", "attn_l", "attn_r")}
    assert gold["init.encoder.layers.0.fc.weight"].shape == (32, 24) and gold["init.encoder.layers.0.attn_l"].shape == (1, 8, 4)
    assert gold["init.encoder.layers.1.fc.weight"].shape == (5, 32) and gold["init.encoder.layers.1.attn_r"].shape == (1, 1, 5)


def test_oracle_eval_forward_matches_the_reference(gold):
    h_list, logits, _ = go.model_fwd(_params(gold), gold["indptr"], gold["indices"], gold["feats"], 2)
    np.testing.assert_allclose(h_list[0], gold["eval.h0"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(logits, gold["eval.logits"], rtol=1e-4, atol=1e-5)


def test_oracle_training_forward_and_gradients_match_the_reference(gold):
    fm, am = _masks(gold, "train")
    loss, grads, logits = go.loss_grads(_params(gold), gold["indptr"], gold["indices"], gold["feats"], gold["labels"], gold["idx_train"], 2,
                                        fm, float(gold["p_feat"]), am, float(gold["p_attn"]))
    np.testing.assert_allclose(logits, gold["train.logits"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(loss, float(gold["train.loss"]), rtol=1e-5)
    for k, g in grads.items():
        np.testing.assert_allclose(g, gold[f"train.grad.{k}"], rtol=1e-3, atol=1e-6, err_msg=k)


def test_oracle_three_train_steps_match_the_reference(gold):
    steps = int(gold["steps"])
    masks = [_masks(gold, f"step{s}") for s in range(steps)]
    losses, params = go.train_steps(_params(gold), gold["indptr"], gold["indices"], gold["feats"], gold["labels"], gold["idx_train"], 2,
                                    [m[0] for m in masks], float(gold["p_feat"]), [m[1] for m in masks], float(gold["p_attn"]),
                                    float(gold["lr"]), float(gold["wd"]), steps)
    np.testing.assert_allclose(losses, gold["losses"], rtol=1e-5)
    for k, v in params.items():
        np.testing.assert_allclose(v, gold[f"final.{k}"], rtol=1e-3, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("H,F,relu", [(8, 4, True), (1, 7, False), (3, 5, True)])
def test_oracle_backward_equals_autograd_in_fp64(H, F, relu):
    """The explicit backward of the issue's formulas against torch autograd on the forward formulas, fp64, with both masks."""
    n, d_in = 40, 6
    ip, ix = random_graph(n, 4, seed=H * 10 + F, self_loops=True, hub=20)
    rs = np.random.RandomState(H + F)
    x, w = rs.standard_normal((n, d_in)), rs.standard_normal((H * F, d_in)) * 0.4
    al, ar = rs.standard_normal((1, H, F)), rs.standard_normal((1, H, F))
    fm, am = (rs.rand(n, d_in) > 0.4).astype(np.uint8), (rs.rand(len(ix), H) > 0.3).astype(np.uint8)
    gy = rs.standard_normal((n, H * F))
    y, c = go.layer_fwd(ip, ix, x, w, al, ar, relu, fm, 0.4, am, 0.3)
    dx, dw, dal, dar = go.layer_bwd(c, gy)
    tx, tw, tl, tr = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, w, al, ar))
    dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(ip)))
    src = torch.from_numpy(ix.astype(np.int64))
    z = ((tx * torch.from_numpy(fm / 0.6)) @ tw.T).view(n, H, F)
    e = torch.nn.functional.leaky_relu((z * tl).sum(-1)[src] + (z * tr).sum(-1)[dst], 0.2)
    ex = torch.exp(e - e.max())
    a = ex / torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, ex)[dst]
    out = torch.zeros(n, H, F, dtype=torch.float64).index_add(0, dst, (a * torch.from_numpy(am / 0.7)).unsqueeze(-1) * z[src])
    out = torch.relu(out) if relu else out
    np.testing.assert_allclose(y, out.detach().numpy().reshape(n, -1), rtol=1e-10, atol=1e-12)
    out.reshape(n, -1).backward(torch.from_numpy(gy))
    for got, ref in ((dx, tx), (dw, tw), (dal, tl), (dar, tr)):
        np.testing.assert_allclose(got, ref.grad.numpy(), rtol=1e-9, atol=1e-11)


def test_header_and_binding_table_carry_the_gat_entries():
    from glnn_amd import _lib
    src = open(os.path.join(ROOT, "include", "glnn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    h = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"GLNN_API\s+[\w\s\*]+?\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/glnn_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert hasattr(h, name)
    assert h.glnn_abi_version() == 12


def test_model_dispatch_contract_on_the_cpu():
    """Model builds GAT only from confs that name BOTH num_heads and attn_dropout_ratio, and honours num_heads."""
    from glnn_amd.models import Model
    base = dict(model_name="GAT", num_layers=2, feat_dim=8, hidden_dim=16, label_dim=4, dropout_ratio=0.0, norm_type="none", device="cpu")
    with pytest.raises(NotImplementedError, match="num_heads"):
        Model(dict(base, attn_dropout_ratio=0.1))
    with pytest.raises(NotImplementedError, match="attn_dropout_ratio"):
        Model(dict(base, num_heads=8))
    with pytest.raises(NotImplementedError, match="num_heads or attn_dropout_ratio"):
        Model(base)
    with pytest.raises(ValueError, match="multiple"):
        Model(dict(base, num_heads=3, attn_dropout_ratio=0.1))
    with pytest.raises(NotImplementedError, match="num_layers"):
        Model(dict(base, num_layers=1, num_heads=8, attn_dropout_ratio=0.1))
    torch.manual_seed(0)
    m = Model(dict(base, num_heads=4, attn_dropout_ratio=0.1))
    sd = m.state_dict()
    assert set(sd) == {f"encoder.layers.{l}.{k}" for l in range(2) for k in ("fc.weight", "attn_l", "attn_r")}      # no res_fc, no bias
    assert tuple(sd["encoder.layers.0.attn_l"].shape) == (1, 4, 4) and tuple(sd["encoder.layers.1.fc.weight"].shape) == (4, 16)
    assert m.encoder.layers[0].attn_drop.p == 0.1 and m.encoder.layers[1]._num_heads == 1


def test_init_draws_the_reference_rng_stream(gold):
    """xavier_normal_(gain relu) on fc.weight, attn_l, attn_r in that order, layer by layer: the same seed gives the golden's weights."""
    from glnn_amd.models import Model
    dims = [int(d) for d in gold["dims"]]
    torch.manual_seed(300)
    m = Model(dict(model_name="GAT", num_layers=2, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[2], dropout_ratio=0.6,
                   norm_type="none", device="cpu", num_heads=8, attn_dropout_ratio=0.3))
    for k, v in m.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), gold[f"init.{k}"], err_msg=k)


def test_gat_layers_refuse_what_is_out_of_scope():
    from glnn_amd.models import GAT
    from glnn_amd.nn import GATConv
    with pytest.raises(NotImplementedError, match="residual"):
        GATConv(8, 4, 2, residual=True)
    with pytest.raises(NotImplementedError, match="residual"):
        GAT(3, 8, 16, 4, 0.0, torch.nn.functional.relu, residual=True)
    with pytest.raises(NotImplementedError, match="bipartite"):
        GATConv((8, 8), 4, 2)


def test_segment_reduce_is_ufunc_at():
    """The oracles' scatter (graphgen.segment_reduce) against numpy's own ufunc.at: unsorted indices, rows nobody names, 1-d .. 3-d values."""
    rs = np.random.RandomState(0)
    n, m = 50, 400
    idx = rs.randint(0, n - 5, size=m)                                       # the last rows stay empty
    idx[idx == 7] = 8                                                        # ... and one in the middle
    for shape in ((m,), (m, 3), (m, 2, 4)):
        vals = rs.standard_normal(shape)
        for ufunc, init in ((np.add, 0.0), (np.maximum, -np.inf)):
            want = np.full((n,) + shape[1:], init)
            ufunc.at(want, idx, vals)
            np.testing.assert_allclose(segment_reduce(ufunc, vals, idx, n, init), want, rtol=1e-14, atol=1e-14)
            order = np.argsort(idx, kind="stable")
            np.testing.assert_allclose(segment_reduce(ufunc, vals[order], idx[order], n, init), want, rtol=1e-14, atol=1e-14)
    assert segment_reduce(np.add, np.zeros((0, 2)), np.zeros(0, np.int64), 3, 0.0).shape == (3, 2)


def test_planted_graph_degrees_are_exact():
    n = 5000
    in_deg, out_deg, lone = {10: 300, 4999: 129, 77: 128}, {3: 200, 2500: 127}, [0, 1, 4000]
    ip, ix = planted_graph(n, 1, in_deg, out_deg, lone)
    deg, out = np.diff(ip), np.bincount(ix, minlength=n)
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and deg.min() == 1
    assert all(deg[r] == d for r, d in in_deg.items()) and all(out[r] == d for r, d in out_deg.items())
    assert (deg[lone] == 1).all() and (ix[ip[lone]] == lone).all()           # the self-loop alone
    assert 2.5 < deg.mean() < 3.5
