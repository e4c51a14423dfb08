"""GAT teacher on the GPU: the attention kernels (csrc/gat.hip) against the fp64 oracle (tests/gat_oracle.py), the mask helper,
determinism, the Model surface against the reference's golden (tests/golden/gat_teacher.npz), gradients and training steps against the
oracle fed the library's masks, the refusals, and the command lines end to end.  Tolerances are those of the APPNP kernel tests
(rtol = atol = 1e-4 for every kernel-level value; rtol 1e-3 / atol 1e-4 for Model-level parameter gradients and trained parameters, as
test_appnp_gpu.py has them).  The per-layer gradients that sum over all rows (dW, dattn, dx) are allowed 4x the error of the fp32 torch
stand-in against the fp64 oracle on the same inputs where that exceeds the APPNP bound (docs/GAT_SEMANTICS.md, Tolerances)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import gat_oracle as go
from graphgen import csr_from_edges, planted_graph, random_graph, scan_geometry, second_trip_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gat_teacher.npz")
DEV = "cuda:0"


def _graph(n=600, seed=3):
    """Non-symmetric multigraph: rows of degree exactly 1 (a self-loop only), a multi-edge, a hub row far above the long-row threshold
    (128) on the destination side AND, for the backward's source pass over the transposed CSR, a hub source of 700 out-edges and a
    source of about 100 (a one-wave row of two 64-entry chunks)."""
    ip, ix = random_graph(n, 6, seed=seed, power=0.6, isolated=9, hub=700, self_loops=True)
    dst = np.repeat(np.arange(n), np.diff(ip))
    src = ix.astype(np.int64)
    rs = np.random.RandomState(seed + 1000)
    open_rows = np.flatnonzero(np.diff(ip) > 1)                           # the degree-1 rows keep their single self-loop
    hub_src, mid_src = int(rs.randint(0, n)), int(rs.randint(0, n))
    src = np.concatenate([src, [src[5], src[5]], np.full(700, hub_src), np.full(90, mid_src)])
    dst = np.concatenate([dst, [dst[5], dst[5]], rs.choice(open_rows, 700), rs.choice(open_rows, 90)])
    ip, ix = csr_from_edges(src, dst, n)
    from glnn_amd.graph import CSRGraph
    return ip, ix, CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)


@pytest.fixture(scope="module")
def graph():
    return _graph()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _layer_inputs(n, d_in, H, F, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, d_in)).astype(np.float32)
    w = (rs.standard_normal((H * F, d_in)) * 0.3).astype(np.float32)
    al, ar = rs.standard_normal((1, H, F)).astype(np.float32), rs.standard_normal((1, H, F)).astype(np.float32)
    gy = rs.standard_normal((n, H * F)).astype(np.float32)
    return x, w, al, ar, gy


def _standin_fp32(ip, ix, x, w, al, ar, relu, fm, p_feat, am, p_attn, gy):
    """The layer in fp32 torch on the CPU (the golden script's stand-in formulas, masks fed as arrays) and its autograd gradients:
    (y, dx, dW, dattn_l, dattn_r).  Its distance from the fp64 oracle is what fp32 arithmetic costs on these inputs; printed next to the
    kernels' distance."""
    n, (_, H, F) = x.shape[0], al.shape
    tx, tw, tl, tr = (torch.tensor(v, dtype=torch.float32, requires_grad=True) for v in (x, w, al, ar))
    dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(ip)))
    src = torch.from_numpy(ix.astype(np.int64))
    fmt = torch.ones_like(tx) if fm is None else torch.from_numpy(fm.astype(np.float32)) / (1.0 - p_feat)
    z = ((tx * fmt) @ tw.T).view(n, H, F)
    e = torch.nn.functional.leaky_relu((z * tl).sum(-1)[src] + (z * tr).sum(-1)[dst], 0.2)
    mx = torch.full((n, H), -float("inf")).index_reduce(0, dst, e.detach(), "amax")
    ex = torch.exp(e - mx[dst])
    a = ex / torch.zeros(n, H).index_add(0, dst, ex)[dst]
    amt = torch.ones_like(a) if am is None else torch.from_numpy(am.astype(np.float32)) / (1.0 - p_attn)
    out = torch.zeros(n, H, F).index_add(0, dst, (a * amt).unsqueeze(-1) * z[src])
    out = torch.relu(out) if relu else out
    out.reshape(n, -1).backward(torch.from_numpy(gy))
    return out.detach().numpy().reshape(n, -1), tx.grad.numpy(), tw.grad.numpy(), tl.grad.numpy(), tr.grad.numpy()


# (H, F) -> gat_rows_kernel<KIND, LPR, UNI> (gat.hip rows_launch: LPR = pow2 >= ceil(H F / 4), at least 4; UNI = F % 4 == 0) and
# HP = pow2 >= H, the head lanes of the score sweeps.  docs/KERNEL_COVERAGE.md lists which case runs which instantiation.
SHAPES = [(8, 16), (8, 8), (8, 7), (1, 47), (1, 7), (1, 16),
          (1, 1),        # LPR 4, one live column
          (3, 5),        # LPR 4, HP 4 with one dead head lane
          (2, 12),       # LPR 8, UNI
          (5, 6),        # LPR 8, HP 8 with three dead head lanes
          (9, 9),        # LPR 32 without UNI, HP 16 with seven dead head lanes
          (16, 3),       # LPR 16, a lane's four columns span two heads, HP 16
          (64, 1),       # LPR 16, four heads per lane, HP 64: one edge per step, no butterfly
          (6, 40),       # LPR 64, UNI
          (7, 33),       # LPR 64 with padding lanes
          (33, 7),       # LPR 64, HP 64 with 31 dead head lanes
          (64, 4),       # LPR 64, UNI: heads = 64 and heads * out_feats = 256 at once
          (1, 256)]      # LPR 64, HP 1, the full-width row


def test_graph_has_the_rows_the_kernels_branch_on(graph):
    ip, ix, _ = graph
    deg = np.diff(ip)
    assert deg.min() == 1 and deg.max() > 128
    out_deg = np.bincount(ix, minlength=len(deg))
    assert out_deg.max() > 128 and ((out_deg > 64) & (out_deg <= 128)).any()           # the source pass: a workgroup row, a two-chunk row
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(len(deg)), deg)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)


def _check_layer(ip, ix, g, H, F, p_attn, d_in=20):
    """One layer on graph (ip, ix, g) against the oracle fed the masks the helpers write; every figure is printed before it is asserted."""
    from glnn_amd import ops
    from glnn_amd.autograd import gat_layer_bwd, gat_layer_fwd
    n, nnz = len(ip) - 1, len(ix)
    relu = H > 1
    p_feat = 0.4 if p_attn > 0 else 0.0
    fs, as_ = 1234 + H, 99 + F
    x, w, al, ar, gy = _layer_inputs(n, d_in, H, F, H * 100 + F)
    tx, tw, tl, tr = _t(x), _t(w), _t(al), _t(ar)
    fm = ops.dropout_mask(n, d_in, p_feat, fs, DEV).cpu().numpy() if p_feat > 0 else None
    am = ops.gat_attn_mask(nnz, H, p_attn, as_, DEV).cpu().numpy() if p_attn > 0 else None
    y, saved = gat_layer_fwd(g, ops.as_feat(tx), tw, tl, tr, H, F, 0.2, relu, p_feat, fs, p_attn, as_, True, want_lse=True)
    ref, c = go.layer_fwd(ip, ix, x, w, al, ar, relu, fm, p_feat, am, p_attn)
    z, el, er, lse = saved
    np.testing.assert_allclose(z.cpu().numpy(), c["z"].reshape(n, -1), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(el.cpu().numpy(), c["el"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(er.cpu().numpy(), c["er"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(lse.cpu().numpy(), c["lse"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    gm = gy * (ref > 0) if relu else gy                                    # the activation mask is the caller's
    da, dw, dal, dar = gat_layer_bwd(g, _t(gm), y, saved, ops.as_feat(tx), tw, tl, tr, H, F, 0.2, p_feat, fs, p_attn, as_, True)
    dx, rdw, rdal, rdar = go.layer_bwd(c, gy)
    dz, _, _ = ops.gat_attn_bwd(g, z, el, er, lse, tl, tr, _t(gm), y, H, F, 0.2, p_attn, as_)
    got = (("dz", dz.cpu().numpy(), go.layer_dz(c, gy)[0]), ("dW", dw.cpu().numpy(), rdw), ("dattn_l", dal.cpu().numpy().reshape(1, H, F), rdal),
           ("dattn_r", dar.cpu().numpy().reshape(1, H, F), rdar), ("dx", da.cpu().numpy() * c["fm"], dx))
    _, sdx, sdw, sdl, sdr = _standin_fp32(ip, ix, x, w, al, ar, relu, fm, p_feat, am, p_attn, gy)
    standin = {"dW": sdw, "dattn_l": sdl, "dattn_r": sdr, "dx": sdx}
    for name, a, b in got:
        e32 = f" fp32 stand-in max|err| {np.abs(standin[name] - b).max():.3e}" if name in standin else ""
        print(f"n={n} H={H} F={F} p_attn={p_attn} {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}{e32}")
    for name, a, b in got:
        # the APPNP kernel bound, or -- where fp32 accumulation over the graph's rows of these unscaled inputs costs more than that -- 4x the
        # error the fp32 stand-in itself shows against the oracle on the same inputs (docs/GAT_SEMANTICS.md, Tolerances).  dz: APPNP bound only.
        e32 = np.abs(standin[name] - b).max() if name in standin else 0.0
        tol = np.maximum(1e-4 + 1e-4 * np.abs(b), 4.0 * e32)
        bad = np.abs(a - b) > tol
        assert not bad.any(), f"{name}: {bad.sum()} elements, max|err| {np.abs(a - b).max():.3e}, fp32 stand-in max|err| {e32:.3e}"


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("p_attn", [0.0, 0.3])
def test_layer_forward_and_backward_match_the_oracle(graph, H, F, p_attn):
    """Scores, attention forward (+ ReLU on the multi-head shapes), attention backward, weight and input gradients against the oracle fed
    the masks the helpers write: dropping exactly the helper's edges / elements in the oracle reproduces the kernels' output.

    (H, F) = (1, 256) is the hard case for the backward's arithmetic: one head of 256 unscaled features gives scores of +-40 and rows
    whose softmax is nearly one-hot, and a hub source sums 700 ds (docs/GAT_SEMANTICS.md, D_i)."""
    ip, ix, g = graph
    _check_layer(ip, ix, g, H, F, p_attn)


# ---------------------------------------------------------------------------------------------------------------- launch geometry
# The numbers rows_launch and gat_rows_kernel derive the grid from, mirrored by name (csrc/gat.hip):
K_BLOCK = 512                 # gat.hip `constexpr int kBlock`: the rows one trip of the long-row scan looks at (n_chunks = ceil(n / kBlock) in gat_rows_kernel)
K_WAVES = K_BLOCK // 64       # gat.hip `constexpr int kWaves`
K_ROWS_PER_WAVE = 8           # gat.hip `constexpr int kRowsPerWave`
K_LONG_ROW = 128              # gat.hip `constexpr int kLongRow`: a row above it is a whole workgroup's
K_LONG_BLOCK_ROWS = 512       # gat.hip `constexpr int kLongBlockRows`
K_LONG_BLOCK_CAP = 512        # gat.hip `constexpr int kLongBlockCap`
BIG_N = K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP + 656      # 262 800: just above the size at which every scan chunk has a workgroup of its own


def _geometry(n):
    """(n_chunks, n_long_blocks, rows_per_block) as gat.hip's rows_launch sets them and the scan loop `for (chunk = blockIdx.x; ...)` of gat_rows_kernel uses them."""
    return scan_geometry(n, K_BLOCK, K_WAVES, K_ROWS_PER_WAVE, K_LONG_BLOCK_ROWS, K_LONG_BLOCK_CAP)


@pytest.fixture(scope="module")
def big_graph():
    from glnn_amd.graph import CSRGraph
    n_chunks, n_long_blocks, _ = _geometry(BIG_N)
    ip, ix = planted_graph(BIG_N, 17, *second_trip_plan(BIG_N, n_chunks, n_long_blocks, K_LONG_ROW))
    return ip, ix, CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), BIG_N)


def test_big_graph_has_the_rows_the_launch_geometry_branches_on(big_graph):
    ip, ix, _ = big_graph
    n = len(ip) - 1
    n_chunks, n_long_blocks, rows_per_block = _geometry(n)
    assert n > K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP and n_chunks > n_long_blocks          # the scan loop makes a second trip
    assert rows_per_block == K_ROWS_PER_WAVE * K_WAVES and n % rows_per_block != 0         # a wave takes eight rows; ragged last block
    deg, out_deg = np.diff(ip), np.bincount(ix, minlength=n)
    for d in (deg, out_deg):                                                # the in-CSR passes and the source pass over the transpose
        long_rows = np.flatnonzero(d > K_LONG_ROW)
        assert (long_rows % n_chunks >= n_long_blocks).sum() >= 2 and (long_rows % n_chunks < n_long_blocks).sum() >= 2
        assert {K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1} <= set(d.tolist())
        assert ((d > 64) & (d < K_LONG_ROW)).any()                           # a one-wave row of two 64-entry chunks
    assert deg.min() == 1 and (deg == 1).sum() > 100 and 2.5 < deg.mean() < 3.5
    last_block = np.arange(n - n % rows_per_block, n)
    assert len(last_block) < rows_per_block and (deg[last_block] > 0).all()


def test_large_n_layer_matches_the_oracle(big_graph):
    """The launch geometry a 600-row graph never reaches (gat.hip rows_launch / gat_rows_kernel): eight rows per wave, a last block that
    ends before its rows do, and long rows -- destinations and, for the source pass, sources -- that the scan finds on its second trip.
    dattn_l / dattn_r sum over all 262 800 rows: the 4x-stand-in clause of the tolerance rule is the one that decides them."""
    ip, ix, g = big_graph
    _check_layer(ip, ix, g, 2, 4, 0.3, d_in=8)


def test_attention_mask_helper_keep_fraction_and_independence():
    from glnn_amd import ops
    nnz, H, p = 50_000, 8, 0.3
    a, b = ops.gat_attn_mask(nnz, H, p, 7, DEV).cpu().numpy(), ops.gat_attn_mask(nnz, H, p, 8, DEV).cpu().numpy()
    assert a.shape == (nnz, H) and set(np.unique(a)) <= {0, 1}
    sd = np.sqrt(nnz * H * p * (1 - p))
    assert abs(a.sum() - nnz * H * (1 - p)) < 5 * sd and abs(b.sum() - nnz * H * (1 - p)) < 5 * sd
    assert abs((a == b).mean() - (p * p + (1 - p) ** 2)) < 0.01              # seeds are independent
    assert abs((a[:, 0] == a[:, 1]).mean() - (p * p + (1 - p) ** 2)) < 0.02  # ... and so are heads
    assert ops.gat_attn_mask(nnz, H, 0.0, 7, DEV).all()


@pytest.mark.parametrize("H,F", [(8, 16), (1, 47), (8, 7), (5, 6), (33, 7)])
def test_two_runs_are_bit_identical(H, F):
    from glnn_amd import ops
    from glnn_amd.autograd import gat_layer_bwd, gat_layer_fwd
    ip, ix, g = _graph(3000, seed=11)
    x, w, al, ar, gy = _layer_inputs(3000, 24, H, F, 5)
    tx, tw, tl, tr, tg = ops.as_feat(_t(x)), _t(w), _t(al), _t(ar), _t(gy)

    def run(seed):
        y, saved = gat_layer_fwd(g, tx, tw, tl, tr, H, F, 0.2, False, 0.5, 3, 0.3, seed, True, want_lse=True)
        return (y,) + gat_layer_bwd(g, tg, y, saved, tx, tw, tl, tr, H, F, 0.2, 0.5, 3, 0.3, seed, True)

    a, b, c = run(99), run(99), run(100)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], c[0])                                       # the seed matters


# ---------------------------------------------------------------------------------------------------------------- Model surface
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _model(gold, p_feat=None, p_attn=None):
    from glnn_amd.models import Model
    dims = gold["dims"]
    conf = dict(model_name="GAT", num_layers=2, feat_dim=int(dims[0]), hidden_dim=int(dims[1]), label_dim=int(dims[2]),
                dropout_ratio=float(gold["p_feat"]) if p_feat is None else p_feat, norm_type="none", device=DEV,
                num_heads=int(gold["num_heads"]), attn_dropout_ratio=float(gold["p_attn"]) if p_attn is None else p_attn)
    m = Model(conf)
    sd = {k[len("init."):]: torch.from_numpy(np.asarray(v)) for k, v in gold.items() if k.startswith("init.")}
    assert set(m.state_dict()) == set(sd)                                    # fc.weight, attn_l, attn_r per layer: no bias, no res_fc
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd)
    return m


def _gold_graph(gold):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(gold["indptr"]).to(DEV), torch.from_numpy(gold["indices"]).to(DEV), len(gold["indptr"]) - 1)


def _params(m):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


def _lib_masks(ops, gold, feat_seeds, attn_seeds):
    """The library's masks of one forward: per layer a feature mask [N, in] and an attention mask [E, H]."""
    n, nnz, dims, H = len(gold["indptr"]) - 1, len(gold["indices"]), gold["dims"], int(gold["num_heads"])
    ins, heads = [int(dims[0]), int(dims[1])], [H, 1]
    fm = [ops.dropout_mask(n, ins[l], float(gold["p_feat"]), feat_seeds[l], DEV).cpu().numpy() for l in range(2)]
    am = [ops.gat_attn_mask(nnz, heads[l], float(gold["p_attn"]), attn_seeds[l], DEV).cpu().numpy() for l in range(2)]
    return fm, am


def test_model_eval_forward_matches_the_reference(gold):
    m = _model(gold)
    m.eval()
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    h_list, logits = m.forward_fitnet(g, x)
    assert len(h_list) == 1 and tuple(h_list[0].shape) == (x.shape[0], int(gold["dims"][1]))
    np.testing.assert_allclose(h_list[0].cpu().numpy(), gold["eval.h0"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(logits.cpu().numpy(), gold["eval.logits"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m(g, x).cpu().numpy(), gold["eval.logits"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m.inference(g, x).cpu().numpy(), gold["eval.logits"], rtol=1e-4, atol=1e-4)


def test_loss_backward_matches_the_oracle_fed_the_library_masks(gold):
    """Model.forward in training mode differentiates through GatConvFn, both dropouts on."""
    from glnn_amd import autograd, ops
    m = _model(gold)
    m.train()
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    idx = torch.from_numpy(gold["idx_train"]).to(DEV)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    c0 = autograd._drop_counter[0]
    logits = m(g, x)
    assert logits.requires_grad and autograd._drop_counter[0] == c0 + 2
    seeds = [autograd.gat_conv_seeds(c0 + 1 + l) for l in range(2)]
    fm, am = _lib_masks(ops, gold, [s[0] for s in seeds], [s[1] for s in seeds])
    loss = torch.nn.NLLLoss()(logits.log_softmax(dim=1)[idx], labels[idx])
    loss.backward()
    ref_loss, grads, ref_logits = go.loss_grads(_params(m), gold["indptr"], gold["indices"], gold["feats"], gold["labels"],
                                                gold["idx_train"], 2, fm, float(gold["p_feat"]), am, float(gold["p_attn"]))
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-4)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[name].reshape(p.shape), rtol=1e-3, atol=1e-4, err_msg=name)


def test_step_gat_gradients_match_the_oracle(gold):
    from glnn_amd import ops, teacher
    m = _model(gold)
    m.train()
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    idx = torch.from_numpy(gold["idx_train"]).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=0.01)
    teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    eng = teacher.get_engine(m, opt)
    params = _params(m)
    eng.step_count += 1
    with torch.no_grad():
        eng._step_gat_body(g, x, labels, idx, 1.0)
    fm, am = _lib_masks(ops, gold, [eng._seed(l) for l in range(2)], [eng._attn_seed(l) for l in range(2)])
    ref_loss, grads, _ = go.loss_grads(params, gold["indptr"], gold["indices"], gold["feats"], gold["labels"], gold["idx_train"], 2, fm,
                                       float(gold["p_feat"]), am, float(gold["p_attn"]))
    np.testing.assert_allclose(eng.loss_out.item(), ref_loss, rtol=1e-4)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(eng.grad(p).cpu().numpy(), grads[name].reshape(p.shape), rtol=1e-3, atol=1e-4, err_msg=name)


def test_train_steps_match_the_oracle(gold):
    """train() (TeacherEngine.step_gat) for three steps == the fp64 oracle fed the library's masks of each step."""
    from glnn_amd import ops, teacher
    from glnn_amd.train_and_eval import train
    m = _model(gold)
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    idx = torch.from_numpy(gold["idx_train"]).to(DEV)
    lr, wd, steps = float(gold["lr"]), float(gold["wd"]), int(gold["steps"])
    opt = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=wd)
    init = _params(m)
    losses, fms, ams = [], [], []
    for s in range(steps):
        losses.append(train(m, g, x, labels, torch.nn.NLLLoss(), opt, idx))
        eng = teacher.get_engine(m, opt)
        assert eng.step_count == s + 1
        fm, am = _lib_masks(ops, gold, [eng._seed(l) for l in range(2)], [eng._attn_seed(l) for l in range(2)])
        fms.append(fm)
        ams.append(am)
    ref_losses, ref_params = go.train_steps(init, gold["indptr"], gold["indices"], gold["feats"], gold["labels"], gold["idx_train"], 2, fms,
                                            float(gold["p_feat"]), ams, float(gold["p_attn"]), lr, wd, steps)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    fin = _params(m)
    for k, v in ref_params.items():
        np.testing.assert_allclose(fin[k], v, rtol=1e-3, atol=1e-4, err_msg=k)
    assert any(not np.array_equal(fms[0][l], fms[1][l]) for l in range(2))       # the seed streams move with the step count


def test_zero_in_degree_raises_and_the_refusals(gold):
    from glnn_amd import dist
    from glnn_amd.graph import CSRGraph
    from glnn_amd.train_and_eval import train
    m = _model(gold)
    m.eval()
    bad = CSRGraph(torch.tensor([0, 1, 1, 2], dtype=torch.int64, device=DEV), torch.tensor([1, 0], dtype=torch.int32, device=DEV), 3)
    x3 = torch.zeros(3, int(gold["dims"][0]), device=DEV)
    with pytest.raises(RuntimeError, match="0-in-degree"):
        m(bad, x3)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    with pytest.raises(RuntimeError, match="0-in-degree"):
        train(m, bad, x3, torch.zeros(3, dtype=torch.int64, device=DEV), torch.nn.NLLLoss(), opt, torch.arange(3, device=DEV))
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    with pytest.raises(NotImplementedError, match="bf16"):
        m.inference(g, x, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="bipartite"):
        m([g], x)
    with pytest.raises(NotImplementedError, match="not sharded"):
        dist.ShardedTeacher(m.encoder, g, None, None)
    with pytest.raises(NotImplementedError, match="not sharded"):
        dist.HaloShardedTeacher(m.encoder, g, None, None)
    # the attention kernels' own limits, through ops: heads <= 64 and heads * out_feats <= 256 (gat.hip set_shape)
    from glnn_amd import ops
    from glnn_amd._lib import GlnnError
    loops = CSRGraph(torch.arange(4, dtype=torch.int64, device=DEV), torch.arange(3, dtype=torch.int32, device=DEV), 3)
    for H, F in ((65, 1), (1, 257), (64, 5)):
        z, al, s3 = torch.zeros(3, H * F, device=DEV), torch.zeros(1, H, F, device=DEV), torch.zeros(3, H, device=DEV)
        with pytest.raises(GlnnError, match=r"heads <= 64 and heads \* out_feats <= 256"):
            ops.gat_scores(z, al, al, H, F)
        with pytest.raises(GlnnError, match=r"heads <= 64 and heads \* out_feats <= 256"):
            ops.gat_attn_fwd(loops.indptr, loops.indices, 3, z, s3, s3, H, F)
        with pytest.raises(GlnnError, match=r"heads <= 64 and heads \* out_feats <= 256"):
            ops.gat_attn_bwd(loops, z, s3, s3, s3, al, al, z, z, H, F)


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_gat_teacher_then_student_cli_on_a_cpf_file(tmp_path):
    """--teacher GAT end to end on the CPF fixture (stored under a CPF dataset name, which is how the loader finds its section of
    train.conf.yaml: dropout 0.6, 8 heads, attention dropout 0.3)."""
    os.makedirs(tmp_path / "data")
    shutil.copy(os.path.join(ROOT, "tests", "golden", "cpf", "tiny_cpf.npz"), tmp_path / "data" / "cora.npz")
    common = ["--dataset", "cora", "--data_path", "data", "--teacher", "GAT", "--device", "0", "--max_epoch", "6", "--patience", "3",
              "--labelrate_train", "3", "--labelrate_val", "5", "--model_config_path", os.path.join(ROOT, "train.conf.yaml"),
              "--save_results"]
    _run("train_teacher.py", common, tmp_path)
    base = tmp_path / "outputs" / "transductive" / "cora"
    out_t = np.load(base / "GAT" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.ndim == 2 and out_t.dtype == np.float32 and np.isfinite(out_t).all()
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    sd = torch.load(base / "GAT" / "seed_0" / "model.pth", map_location="cpu")
    assert tuple(sd["encoder.layers.0.attn_l"].shape) == (1, 8, 16) and "encoder.layers.0.res_fc" not in sd
    _run("train_student.py", common + ["--student", "MLP", "--lamb", "0.5"], tmp_path)
    out_s = np.load(base / "GAT_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == out_t.shape and np.isfinite(out_s).all()
