"""GPR-GNN teacher on the GPU: the propagation and fold kernels (csrc/gpr.hip) against the fp64 oracle (tests/gpr_oracle.py), the identity
with APPNP under PPR coefficients, determinism and launch geometry, the Model surface and the training step against the oracle fed the
library's dropout masks, the refusals, and the command lines end to end.  Tolerances are those of tests/test_appnp_gpu.py; the coefficient
gradient, which sums n * d terms, is allowed 4x the error of an fp32 CPU stand-in of the same sums where that exceeds the bound (the rule of
tests/test_gat_gpu.py; docs/GPR_SEMANTICS.md, Tolerances)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import appnp_oracle as ao
import gpr_oracle as go
from graphgen import csr_from_edges, planted_graph, random_graph, scan_geometry, second_trip_plan, segment_reduce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _csr_graph(ip, ix):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), len(ip) - 1)


def _graph(n=600, seed=3):
    """The graph of tests/test_appnp_gpu.py -- non-symmetric, isolated rows, one destination row far above the long-row threshold (128) --
    plus, for the pass over the transposed CSR, a hub source of 700 out-edges (a whole-workgroup row) and one of about 100 (a one-wave row
    of two 64-entry chunks).  The added edges end in rows that already have in-edges: the isolated rows stay isolated."""
    ip, ix = random_graph(n, 6, seed=seed, power=0.6, isolated=9, hub=700)
    dst, src = np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)
    rs = np.random.RandomState(seed + 1000)
    open_rows = np.flatnonzero(np.diff(ip) > 0)
    hub_src, mid_src = (int(v) for v in rs.choice(n, 2, replace=False))
    src = np.concatenate([src, np.full(700, hub_src), np.full(100, mid_src)])
    dst = np.concatenate([dst, rs.choice(open_rows, 700), rs.choice(open_rows, 100)])
    ip, ix = csr_from_edges(src, dst, n)
    return ip, ix, _csr_graph(ip, ix)


@pytest.fixture(scope="module")
def graph():
    return _graph()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def test_graph_has_the_rows_the_kernel_branches_on(graph):
    ip, ix, _ = graph
    deg, out_deg = np.diff(ip), np.bincount(ix, minlength=len(ip) - 1)
    assert deg.max() > 128 and (deg == 0).sum() >= 9
    assert out_deg.max() > 128 and ((out_deg > 64) & (out_deg <= 128)).any() and (out_deg == 0).any()
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(len(deg)), deg)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                                   # a multi-edge
    assert not np.array_equal(np.sort(deg), np.sort(out_deg))                           # non-symmetric


# ---------------------------------------------------------------------------------------------------------------- propagation
def _nan_feat(a):
    """A device copy of `a` in a NaN-filled [n, round4(d)] buffer: whatever reads a padding column, or leaves one unwritten, shows."""
    n, d = a.shape
    buf = torch.full((n, (d + 3) // 4 * 4), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :d] = _t(a)
    return buf[:, :d]


def _run_raw(g, x0, gamma, k, backward, h0=None):
    """gpr_fwd / gpr_bwd's launch sequence with every buffer pre-filled with NaN (inputs' padding columns included):
    (acc buffer [n, round4(d)], row_dot or None)."""
    from glnn_amd import ops
    n, d = x0.shape
    ld = (d + 3) // 4 * 4
    in_norm, out_norm = g.degree_norms()
    csr = g.transposed(False) if backward else g
    first_norm, row_norm = (in_norm, out_norm) if backward else (out_norm, in_norm)
    nan = lambda: torch.full((n, ld), float("nan"), dtype=torch.float32, device=DEV)
    acc_buf = nan()
    acc = acc_buf[:, :d]
    row_dot = None
    if h0 is not None:
        row_dot = torch.full(((k + 1) * ops.gpr_col_tiles(d) * n,), float("nan"), dtype=torch.float32, device=DEV)
    if k == 0:
        ops.gpr_prop(None, None, 0, x0, 0, None, None, None, gamma, acc, h0=h0, row_dot=row_dot)
        return acc_buf, row_dot, []
    bufs = [nan() for _ in range(min(k - 1, 2))]
    x = x0
    for j in range(1, k + 1):
        out = None if j == k else bufs[j % len(bufs)][:, :d]
        ops.gpr_prop(csr.indptr, csr.indices, g.num_edges(), x, j, first_norm if j == 1 else None, row_norm, first_norm, gamma, acc,
                     out=out, h0=h0, row_dot=row_dot)
        x = out
    return acc_buf, row_dot, bufs


def _standin_dgamma_fp32(ip, ix, dy, h0, k):
    """The coefficient gradient's sums <G_j, h0> in fp32 numpy on the CPU (fp32 norms, products and sums throughout): its distance from the
    fp64 oracle is what fp32 arithmetic costs on these inputs."""
    n = len(ip) - 1
    dn, sn = (v.astype(np.float32) for v in ao.degree_norms(ip, ix, n))
    dst, src = np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)
    gk, h0 = dy.astype(np.float32), h0.astype(np.float32)
    out = [np.sum(gk * h0, dtype=np.float32)]
    for _ in range(k):
        gk = sn[:, None] * segment_reduce(np.add, dn[dst, None] * gk[dst], src, n, np.float32(0.0))
        out.append(np.sum(gk * h0, dtype=np.float32))
    return np.asarray(out, np.float64)


def _check_dgamma(tag, got, ref, standin):
    e32 = np.abs(standin - ref)
    print(f"{tag} dgamma: max|err| {np.abs(got - ref).max():.3e} max|ref| {np.abs(ref).max():.3e} fp32 stand-in max|err| {e32.max():.3e}")
    tol = np.maximum(1e-4 + 1e-4 * np.abs(ref), 4.0 * e32)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{tag} dgamma: {got} vs {ref} (fp32 stand-in err {e32})"


def _check_propagation(ip, ix, g, d, k, seed=0, padding=True):
    from glnn_amd import ops
    from glnn_amd.autograd import gpr_bwd, gpr_fwd
    n = len(ip) - 1
    rs = np.random.RandomState(d * 100 + k + seed)
    h0 = rs.standard_normal((n, d)).astype(np.float32)
    dy = rs.standard_normal((n, d)).astype(np.float32)
    gamma = rs.uniform(-1.0, 1.0, k + 1).astype(np.float32)
    gamma[rs.randint(0, k + 1)] = -0.75                                               # signed for sure
    tg, tag = _t(gamma), f"n={n} d={d} k={k}"
    out = gpr_fwd(g, _t(h0), tg, k).cpu().numpy()
    ref = go.propagate(ip, ix, h0, gamma)
    print(f"{tag} forward: max|err| {np.abs(out - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4)
    dh0, dgamma = gpr_bwd(g, _t(dy), _t(h0), tg, k)
    rdh0, rdg = go.propagate_bwd(ip, ix, dy, h0, gamma)
    print(f"{tag} backward: max|err| {np.abs(dh0.cpu().numpy() - rdh0).max():.3e} max|ref| {np.abs(rdh0).max():.3e}")
    np.testing.assert_allclose(dh0.cpu().numpy(), rdh0, rtol=1e-4, atol=1e-4)
    assert dgamma.shape == (k + 1,)
    _check_dgamma(tag, dgamma.cpu().numpy().astype(np.float64), rdg, _standin_dgamma_fp32(ip, ix, dy, h0, k))
    if not padding:
        return
    # the same launches over NaN-filled buffers: the results do not move, and every padding column [d, ld) comes out zero
    ld = (d + 3) // 4 * 4
    acc_f, _, bufs_f = _run_raw(g, _nan_feat(h0), tg, k, backward=False)
    acc_b, row_dot, bufs_b = _run_raw(g, _nan_feat(dy), tg, k, backward=True, h0=_nan_feat(h0))
    assert torch.equal(acc_f[:, :d].cpu(), torch.from_numpy(out)) and torch.equal(acc_b[:, :d], dh0)
    for buf in [acc_f, acc_b] + bufs_f + bufs_b:
        assert not torch.isnan(buf).any()
        if ld > d:
            assert bool((buf[:, d:] == 0).all())
    assert not torch.isnan(row_dot).any()
    assert torch.equal(ops.gpr_fold(row_dot, k + 1, ops.gpr_col_tiles(d) * n), dgamma)


# the smallest d of every LPR instantiation the launcher can pick (LPR = pow2 >= ceil(min(d, 256) / 4): 1, 2, 4, 8, 16, 32, 64), then a
# width inside a lane group's last float4 (47), the full 256-column row, and two column tiles (300)
WIDTHS = (1, 5, 9, 17, 33, 65, 129, 47, 256, 300)


@pytest.mark.parametrize("k", [0, 1, 2, 10])
@pytest.mark.parametrize("d", WIDTHS)
def test_forward_and_backward_match_the_oracle(graph, d, k):
    ip, ix, g = graph
    _check_propagation(ip, ix, g, d, k)


# ---------------------------------------------------------------------------------------------------------------- the APPNP identity
@pytest.mark.parametrize("alpha", [0.1, 0.5])
@pytest.mark.parametrize("k", [1, 10])
def test_ppr_coefficients_give_appnp(graph, k, alpha):
    """With gamma_j = alpha (1 - alpha)^j, gamma_K = (1 - alpha)^K the new kernels compute what the APPNP oracle and the APPNP kernels
    (edge_drop 0) compute: arithmetic that the reference-generated tests/golden/appnp_teacher.npz already pins."""
    from glnn_amd.autograd import appnp_bwd, appnp_fwd, gpr_bwd, gpr_fwd
    ip, ix, g = graph
    n, d = len(ip) - 1, 47
    rs = np.random.RandomState(k)
    h0 = rs.standard_normal((n, d)).astype(np.float32)
    dy = rs.standard_normal((n, d)).astype(np.float32)
    gamma = _t(go.ppr_gamma(k, alpha))
    out = gpr_fwd(g, _t(h0), gamma, k).cpu().numpy()
    np.testing.assert_allclose(out, ao.propagate(ip, ix, h0, k, alpha, None, 0), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out, appnp_fwd(g, _t(h0), k, alpha, 0.0, 0).cpu().numpy(), rtol=1e-4, atol=1e-4)
    dh0 = gpr_bwd(g, _t(dy), _t(h0), gamma, k)[0].cpu().numpy()
    np.testing.assert_allclose(dh0, appnp_bwd(g, _t(dy), k, alpha, 0.0, 0).cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dh0, ao.propagate_bwd(ip, ix, dy, k, alpha, None, 0), rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------- determinism, geometry
@pytest.mark.parametrize("d", [7, 47])
def test_two_runs_are_bit_identical(d):
    from glnn_amd.autograd import gpr_bwd, gpr_fwd
    ip, ix = random_graph(3000, 6, seed=11, power=0.6, isolated=9, hub=700)
    g = _csr_graph(ip, ix)
    rs = np.random.RandomState(d)
    h0, dy = _t(rs.standard_normal((3000, d))), _t(rs.standard_normal((3000, d)))
    gamma = _t(rs.uniform(-1, 1, 11))
    a, b = gpr_fwd(g, h0, gamma, 10), gpr_fwd(g, h0, gamma, 10)
    assert torch.equal(a, b)
    (da, ga), (db, gb) = gpr_bwd(g, dy, h0, gamma, 10), gpr_bwd(g, dy, h0, gamma, 10)
    assert torch.equal(da, db) and torch.equal(ga, gb)


def test_gamma_is_read_from_device_memory_on_every_call(graph):
    """gamma changed IN PLACE between two calls (what Adam does) changes the result: nothing of it is cached on the host."""
    from glnn_amd.autograd import gpr_bwd, gpr_fwd
    ip, ix, g = graph
    rs = np.random.RandomState(4)
    h0, dy = rs.standard_normal((len(ip) - 1, 12)).astype(np.float32), rs.standard_normal((len(ip) - 1, 12)).astype(np.float32)
    gamma = _t(rs.uniform(-1, 1, 4))
    a = gpr_fwd(g, _t(h0), gamma, 3).clone()
    da = gpr_bwd(g, _t(dy), _t(h0), gamma, 3)[0].clone()
    gamma.mul_(2.0)                                                                     # same tensor, same pointer (exact in fp32)
    b, (db, _) = gpr_fwd(g, _t(h0), gamma, 3), gpr_bwd(g, _t(dy), _t(h0), gamma, 3)
    assert not torch.equal(a, b) and torch.equal(b, 2.0 * a) and torch.equal(db, 2.0 * da)
    gamma[2] = 0.25
    np.testing.assert_allclose(gpr_fwd(g, _t(h0), gamma, 3).cpu().numpy(), go.propagate(ip, ix, h0, gamma.cpu().numpy()), rtol=1e-4, atol=1e-4)


def test_fold_combines_more_than_one_partial():
    """n = GLNN_GPR_FOLD_CHUNK + 1 rows of a degree-1 graph (a ring): the fold's first stage leaves two partials per coefficient, the second
    of ONE entry, and the second stage combines them.  Then the fold alone on sizes around its chunk and block sizes."""
    from glnn_amd import _lib, ops
    chunk = _lib.GPR_FOLD_CHUNK                                                         # 4096: kFoldChunk of csrc/gpr.hip
    n = chunk + 1
    ip, ix = csr_from_edges((np.arange(n) + 1) % n, np.arange(n), n)
    assert (np.diff(ip) == 1).all()
    _check_propagation(ip, ix, _csr_graph(ip, ix), 3, 2, padding=False)
    rs = np.random.RandomState(9)
    for rows, m in ((3, chunk + 1), (1, 1), (2, 255), (4, chunk), (11, 2 * chunk + 5), (2, 257 * chunk + 3)):
        rd = rs.standard_normal((rows, m)).astype(np.float32)
        got = ops.gpr_fold(_t(rd).reshape(-1), rows, m).cpu().numpy()
        ref = rd.astype(np.float64).sum(1)
        # fp64 accumulation, one rounding to fp32 at the end: half an fp32 ulp of the sum plus fp64 noise
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6 * np.sqrt(m))
        assert np.array_equal(got, ops.gpr_fold(_t(rd).reshape(-1), rows, m).cpu().numpy())


# The numbers glnn_gpr_prop_f32 and gpr_prop_kernel derive the grid from, mirrored by name (csrc/row_gather_dev.h, which appnp.hip reads too):
K_BLOCK = 512                 # kBlock: the rows one trip of the long-row scan looks at (n_chunks = ceil(n / kBlock))
K_WAVES = K_BLOCK // 64       # kWaves
K_ROWS_PER_WAVE = 8           # kRowsPerWave
K_LONG_ROW = 128              # kLongRow: a row above it is a whole workgroup's
K_LONG_BLOCK_ROWS = 512       # kLongBlockRows
K_LONG_BLOCK_CAP = 512        # kLongBlockCap
BIG_N = K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP + 656      # 262 800: just above the size at which every scan chunk has a workgroup of its own


def test_large_n_propagation_matches_the_oracle():
    """The launch geometry a 600-row graph never reaches: 64 tickets per row block, a last block that ends before its tickets do, and long
    rows -- destinations forward, sources backward -- that the long-row scan finds on its SECOND trip only."""
    n_chunks, n_long_blocks, rows_per_block = scan_geometry(BIG_N, K_BLOCK, K_WAVES, K_ROWS_PER_WAVE, K_LONG_BLOCK_ROWS, K_LONG_BLOCK_CAP)
    assert n_chunks > n_long_blocks and rows_per_block == K_ROWS_PER_WAVE * K_WAVES and BIG_N % rows_per_block != 0
    ip, ix = planted_graph(BIG_N, 17, *second_trip_plan(BIG_N, n_chunks, n_long_blocks, K_LONG_ROW))
    for deg in (np.diff(ip), np.bincount(ix, minlength=BIG_N)):
        long_rows = np.flatnonzero(deg > K_LONG_ROW)
        assert (long_rows % n_chunks >= n_long_blocks).sum() >= 2 and (long_rows % n_chunks < n_long_blocks).sum() >= 2
        assert {K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1} <= set(deg.tolist())
    _check_propagation(ip, ix, _csr_graph(ip, ix), 8, 2, padding=False)


# ---------------------------------------------------------------------------------------------------------------- model, training step
LR, WD, K_MODEL = 0.01, 0.01, 3
MODEL_DIMS = {"2": (20, 32, 6), "3": (12, 16, 16, 5)}


def _model(dims, norm, dropout, seed=0):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    conf = dict(model_name="GPRGNN", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=dropout,
                norm_type=norm, device=DEV, gpr_k=K_MODEL, gpr_init="Random")
    m = Model(conf)
    if norm != "none":                       # affine parameters away from (1, 0), so that their gradients matter
        with torch.no_grad():
            for nm in m.encoder.norms:
                nm.weight.uniform_(0.5, 1.5)
                nm.bias.uniform_(-0.2, 0.2)
    return m


def _data(n, dims, seed=1):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, dims[0])).astype(np.float32)
    labels = rs.randint(0, dims[-1], n).astype(np.int64)
    idx = np.sort(rs.choice(n, n // 3, replace=False)).astype(np.int64)
    return x, labels, idx


def _np_state(m):
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    L = m.encoder.num_layers
    bn = {l: (sd[f"encoder.norms.{l}.running_mean"], sd[f"encoder.norms.{l}.running_var"]) for l in range(L - 1)
          if f"encoder.norms.{l}.running_mean" in sd}
    params = {k: v for k, v in sd.items() if "running" not in k and "num_batches" not in k}
    return params, bn


CONFIGS = [(dk, norm, p) for dk in MODEL_DIMS for norm in ("none", "batch", "layer") for p in (0.0, 0.5)]


@pytest.mark.parametrize("dims_key,norm,dropout", CONFIGS)
def test_eval_logits_and_one_training_step_match_the_oracle(graph, dims_key, norm, dropout):
    """Model.forward / inference in eval mode, then ONE train() step (TeacherEngine.step_gpr) against the oracle's step fed the library's
    dropout masks: the loss, every gradient (gamma's included), the parameters and both Adam moments after the update."""
    from glnn_amd import ops, teacher
    from glnn_amd.train_and_eval import train
    ip, ix, g = graph
    dims = MODEL_DIMS[dims_key]
    L, n = len(dims) - 1, len(ip) - 1
    m = _model(dims, norm, dropout)
    gamma0 = m.encoder.propagate.gamma.detach().cpu().numpy()
    assert (gamma0 < 0).any() and (gamma0 > 0).any()
    x, labels, idx = _data(n, dims)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    params, bn = _np_state(m)
    m.eval()
    ref_logits = go.model_forward(params, bn, ip, ix, x, L, norm)
    h_list, logits = m.forward_fitnet(g, tx)
    assert len(h_list) == L - 1
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m(g, tx).cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m.inference(g, tx).cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)

    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    loss = train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
    eng = teacher.get_engine(m, opt)
    assert eng.kind == "gpr" and eng.step_count == 1
    masks = None
    if dropout > 0:                                                                     # the masks of step 1, hidden layer l
        masks = [ops.dropout_mask(n, dims[l + 1], dropout, eng._seed(l), DEV).cpu().numpy() for l in range(L - 1)]
    ref_losses, ref_grads, ref_params, ref_state, ref_bn = go.train_steps(params, bn, ip, ix, x, labels, idx, L, norm,
                                                                          None if masks is None else [masks], dropout, LR, WD, 1)
    print(f"{dims} {norm} p={dropout}: loss {loss:.6f} oracle {ref_losses[0]:.6f}")
    np.testing.assert_allclose(loss, ref_losses[0], rtol=1e-4)
    named = dict(m.named_parameters())
    assert set(named) == set(ref_grads)
    for name, p in named.items():
        got = eng.grad(p).cpu().numpy()
        print(f"  grad {name}: max|err| {np.abs(got - ref_grads[name]).max():.3e} max|ref| {np.abs(ref_grads[name]).max():.3e}")
        np.testing.assert_allclose(got, ref_grads[name], rtol=1e-3, atol=1e-4, err_msg=f"grad {name}")
    for name, p in named.items():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref_params[name], rtol=1e-3, atol=1e-4, err_msg=name)
        st = opt.state[p]
        assert float(st["step"]) == 1.0
        np.testing.assert_allclose(st["exp_avg"].cpu().numpy(), ref_state[name][0], rtol=1e-3, atol=1e-4, err_msg=f"exp_avg {name}")
        np.testing.assert_allclose(st["exp_avg_sq"].cpu().numpy(), ref_state[name][1], rtol=1e-3, atol=1e-4, err_msg=f"exp_avg_sq {name}")
    assert not np.array_equal(m.encoder.propagate.gamma.detach().cpu().numpy(), gamma0)  # gamma is trained
    fin = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for l, (rm, rv) in ref_bn.items():
        np.testing.assert_allclose(fin[f"encoder.norms.{l}.running_mean"], rm, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(fin[f"encoder.norms.{l}.running_var"], rv, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dims_key,norm", [(dk, norm) for dk in MODEL_DIMS for norm in ("none", "batch", "layer")])
def test_autograd_path_matches_the_engine_gradients(graph, dims_key, norm):
    """Model.forward in training mode differentiates through GprPropFn: its gradients equal step_gpr's (dropout-free configs)."""
    from glnn_amd import teacher
    from glnn_amd.train_and_eval import train
    ip, ix, g = graph
    dims = MODEL_DIMS[dims_key]
    m = _model(dims, norm, 0.0, seed=2)
    x, labels, idx = _data(len(ip) - 1, dims, seed=3)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    m.train()
    logits = m(g, tx)
    assert logits.requires_grad
    torch.nn.NLLLoss()(logits.log_softmax(dim=1)[ti], tl[ti]).backward()
    auto = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    assert all(v is not None for v in auto.values()) and "encoder.propagate.gamma" in auto
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
    eng = teacher.get_engine(m, opt)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(eng.grad(p).cpu().numpy(), auto[name].cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=name)


def test_three_steps_leave_loadable_and_consistent_state(graph):
    from glnn_amd.train_and_eval import train
    ip, ix, g = graph
    dims = MODEL_DIMS["3"]
    x, labels, idx = _data(len(ip) - 1, dims)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    m = _model(dims, "batch", 0.0)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    losses = [train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti) for _ in range(3)]
    assert all(np.isfinite(losses))
    osd, msd = opt.state_dict(), m.state_dict()
    assert len(osd["state"]) == len(list(m.parameters()))
    for st, p in zip(osd["state"].values(), m.parameters()):
        assert float(st["step"]) == 3.0 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert torch.isfinite(st["exp_avg"]).all() and bool((st["exp_avg_sq"] >= 0).all())
    assert int(msd["encoder.norms.0.num_batches_tracked"]) == 3 and msd["encoder.propagate.gamma"].shape == (K_MODEL + 1,)
    buf = io.BytesIO()                                                                  # a checkpoint round trip (state_dict() hands out the
    torch.save({"model": msd, "optimizer": osd}, buf)                                   # live moment tensors: loading them directly would alias)
    buf.seek(0)
    ckpt = torch.load(buf, map_location=DEV)
    m2 = _model(dims, "batch", 0.0, seed=5)
    m2.load_state_dict(ckpt["model"])
    opt2 = torch.optim.Adam(m2.parameters(), lr=LR, weight_decay=WD)
    opt2.load_state_dict(ckpt["optimizer"])
    l1, l2 = train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti), train(m2, g, tx, tl, torch.nn.NLLLoss(), opt2, ti)
    assert l1 == l2                                                                     # the fourth step of both: same bits
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2), k1


# ---------------------------------------------------------------------------------------------------------------- refusals, command lines
def test_bf16_and_sharded_forms_refuse_gprgnn(graph):
    from glnn_amd import dist
    _, _, g = graph
    m = _model(MODEL_DIMS["2"], "none", 0.0)
    x = torch.zeros(len(graph[0]) - 1, MODEL_DIMS["2"][0], device=DEV)
    with pytest.raises(NotImplementedError, match="GPRGNN"):
        m.inference(g, x, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="GPRGNN"):
        dist.ShardedTeacher(m.encoder, g, None, None)
    with pytest.raises(NotImplementedError, match="GPRGNN"):
        dist.HaloShardedTeacher(m.encoder, g, None, None)
    with pytest.raises(NotImplementedError, match="bipartite"):
        m([g], x)


def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_gprgnn_teacher_then_student_cli(tmp_path):
    common = ["--dataset", "synthetic-cora", "--teacher", "GPRGNN", "--device", "0", "--max_epoch", "3"]
    _run("train_teacher.py", common, tmp_path)
    base = tmp_path / "outputs" / "transductive" / "synthetic-cora"
    out_t = np.load(base / "GPRGNN" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    _run("train_student.py", common + ["--student", "MLP"], tmp_path)
    out_s = np.load(base / "GPRGNN_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
