"""GATv2 teacher on the GPU: the attention kernels (csrc/gatv2.hip) against the fp64 oracle (tests/gatv2_oracle.py) at every lane layout
and launch geometry, the online softmax's edge cases, determinism, the limits, the Model surface, gradients and training steps against
the oracle fed the library's own masks, and the command lines.

Tolerances (docs/GATV2_SEMANTICS.md, Tolerances): rtol = atol = 1e-4 on zl, zr, lse, the outputs, dzl and dzr; the gradients that sum
over all rows (dW_*, db_*, dattn) and dx take max(1e-4 + 1e-4 |ref|, 4 x the error of an fp32 CPU stand-in -- the oracle's own arithmetic
run in fp32 -- against the fp64 oracle on the same inputs); the stand-in's error is computed per case and printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gatv2_oracle as vo
from graphgen import csr_from_edges, planted_graph, random_graph, scan_geometry, second_trip_plan
from test_gat_gpu import _graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def graph():
    return _graph()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _nan_rows(n, d):
    """An [n, d] view of NaN-filled [n, round4(d)] storage: (view, storage)."""
    buf = torch.full((n, (d + 3) // 4 * 4), NAN, dtype=torch.float32, device=DEV)
    return buf[:, :d], buf


def _layer_inputs(n, d_in, H, F, seed):
    rs = np.random.RandomState(seed)
    f32 = lambda a: a.astype(np.float32)
    p = {"fc_src.weight": f32(rs.standard_normal((H * F, d_in)) * 0.3), "fc_src.bias": f32(rs.standard_normal(H * F) * 0.2),
         "fc_dst.weight": f32(rs.standard_normal((H * F, d_in)) * 0.3), "fc_dst.bias": f32(rs.standard_normal(H * F) * 0.2),
         "attn": f32(rs.standard_normal((1, H, F)))}
    return f32(rs.standard_normal((n, d_in))), p, f32(rs.standard_normal((n, H * F)))


# (H, F) -> gatv2_rows_kernel<KIND, LPR, UNI> (gatv2.hip rows_launch: LPR = pow2 >= ceil(H F / 4), at least 4; UNI = F % 4 == 0).
# docs/KERNEL_COVERAGE.md lists which case runs which instantiation.
SHAPES = [(1, 16),       # LPR 4, UNI: one head over the four lanes
          (1, 7),        # LPR 4: a head of two lanes, one padding column
          (1, 1),        # LPR 4, one live column
          (3, 5),        # LPR 4: heads that start and end inside a lane
          (2, 12),       # LPR 8, UNI: heads of three lanes (no power of two)
          (5, 6),        # LPR 8
          (8, 8),        # LPR 16, UNI: heads of two lanes
          (8, 7),        # LPR 16: a lane's columns in two heads
          (1, 47),       # LPR 16: one head over twelve lanes
          (64, 1),       # LPR 16: four heads per lane, no cross-lane sum at all
          (8, 16),       # LPR 32, UNI: the hidden layers of the conf sections at hidden_dim 128
          (9, 9),        # LPR 32 with padding lanes
          (6, 40),       # LPR 64, UNI: heads of ten lanes
          (64, 4),       # LPR 64, UNI: heads = 64 and heads * out_feats = 256 at once, a head per lane
          (1, 256),      # LPR 64, UNI: one head over the whole wave
          (7, 33),       # LPR 64 with padding lanes
          (33, 7)]       # LPR 64: 33 heads


def test_graph_has_the_rows_the_kernels_branch_on(graph):
    ip, ix, _ = graph
    deg = np.diff(ip)
    assert len(deg) == 600 and deg.min() == 1 and deg.max() > 640          # self-loops on the isolated rows; a hub of about 700
    out_deg = np.bincount(ix, minlength=len(deg))
    assert out_deg.max() >= 700 and ((out_deg > 64) & (out_deg <= 128)).any()           # the source pass: a workgroup row, a two-chunk row
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(len(deg)), deg)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                      # a multi-edge


def _check_layer(ip, ix, g, H, F, p_attn, d_in=20):
    """One layer on graph (ip, ix, g) against the oracle fed the masks the helpers write; every figure is printed before it is asserted.
    Every buffer a kernel writes is NaN-filled first, padding columns included, and the padding is checked to come back zero."""
    from glnn_amd import ops
    from glnn_amd.autograd import gatv2_layer_bwd, gatv2_layer_fwd
    n, nnz, hf = len(ip) - 1, len(ix), H * F
    relu = H > 1
    p_feat = 0.4 if p_attn > 0 else 0.0
    fs, as_ = 1234 + H, 99 + F
    x, p, gy = _layer_inputs(n, d_in, H, F, H * 100 + F)
    tp = {k: _t(v) for k, v in p.items()}
    tx = ops.as_feat(_t(x))
    fm = ops.dropout_mask(n, d_in, p_feat, fs, DEV).cpu().numpy() if p_feat > 0 else None
    am = ops.gat_attn_mask(nnz, H, p_attn, as_, DEV).cpu().numpy() if p_attn > 0 else None
    ref, c = vo.layer_fwd(ip, ix, x, p, relu, fm, p_feat, am, p_attn)
    r32, c32 = vo.layer_fwd(ip, ix, x, p, relu, fm, p_feat, am, p_attn, dtype=np.float32)
    # forward
    y, (xd, zl, zr, lse) = gatv2_layer_fwd(g, tx, tp["fc_src.weight"], tp["fc_src.bias"], tp["fc_dst.weight"], tp["fc_dst.bias"], tp["attn"],
                                           H, F, 0.2, relu, p_feat, fs, p_attn, as_, want_lse=True)
    out, out_buf = _nan_rows(n, hf)
    lse2 = torch.full((n, H), NAN, dtype=torch.float32, device=DEV)
    ops.gatv2_attn_fwd(g.indptr, g.indices, nnz, zl, zr, tp["attn"], H, F, 0.2, p_attn, as_, relu=relu, out=out, lse=lse2)
    assert torch.equal(out, y) and torch.equal(lse2, lse) and not out_buf[:, hf:].any()
    for name, a, b in (("zl", zl, c["zl"]), ("zr", zr, c["zr"]), ("lse", lse, c["lse"]), ("out", y, ref)):
        a, b = a.cpu().numpy(), np.asarray(b).reshape(n, -1)
        print(f"n={n} H={H} F={F} p_attn={p_attn} {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=name)
    # backward
    gm = gy * (ref > 0) if relu else gy                                    # the activation mask is the caller's
    tg = ops.as_feat(_t(gm))
    dzl, dzl_buf = _nan_rows(n, hf)
    dzr, dzr_buf = _nan_rows(n, hf)
    dattn = torch.full((hf,), NAN, dtype=torch.float32, device=DEV)
    ops.gatv2_attn_bwd(g, zl, zr, lse, tp["attn"], tg, H, F, 0.2, p_attn, as_, dattn=dattn, dzl=dzl, dzr=dzr)
    assert not dzl_buf[:, hf:].any() and not dzr_buf[:, hf:].any()
    da, dws, dbs, dwd, dbd, dat = gatv2_layer_bwd(g, tg, (xd, zl, zr, lse), tp["fc_src.weight"], tp["fc_dst.weight"], tp["attn"], H, F, 0.2,
                                                  p_attn, as_)
    assert torch.equal(dat, dattn)
    rdzl, rdzr, _, _ = vo.attn_bwd(c, gy)
    for name, a, b in (("dzl", dzl, rdzl), ("dzr", dzr, rdzr)):
        a, b = a.cpu().numpy(), b.reshape(n, -1)
        print(f"n={n} H={H} F={F} p_attn={p_attn} {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=name)
    dx, grads = vo.layer_bwd(c, gy)
    sdx, sgrads = vo.layer_bwd(c32, gy)
    got = [("dx", da.cpu().numpy() * c["fm"], dx, sdx)]
    got += [(k, v.cpu().numpy().reshape(grads[k].shape), grads[k], sgrads[k])
            for k, v in (("fc_src.weight", dws), ("fc_src.bias", dbs), ("fc_dst.weight", dwd), ("fc_dst.bias", dbd), ("attn", dat))]
    worst = []
    for name, a, b, s in got:
        e32 = float(np.abs(s.astype(np.float64) - b).max())
        print(f"n={n} H={H} F={F} p_attn={p_attn} d {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e} "
              f"fp32 stand-in max|err| {e32:.3e}")
        bad = np.abs(a - b) > np.maximum(1e-4 + 1e-4 * np.abs(b), 4.0 * e32)
        if bad.any():
            worst.append(f"{name}: {bad.sum()} elements, max|err| {np.abs(a - b).max():.3e}, fp32 stand-in max|err| {e32:.3e}")
    assert not worst, worst


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("p_attn", [0.0, 0.3])
def test_layer_forward_and_backward_match_the_oracle(graph, H, F, p_attn):
    """The two projections, the attention forward (+ ReLU on the multi-head shapes), the attention backward, weight, bias, attn and input
    gradients against the oracle fed the masks the helpers write, on the 600-row graph: a 700-edge hub destination (a workgroup row with
    every wave's share of the merge), degree-1 rows, a multi-edge, and in the transpose a 700-edge source and one of two chunks."""
    ip, ix, g = graph
    _check_layer(ip, ix, g, H, F, p_attn)


# ---------------------------------------------------------------------------------------------------------------- online softmax
def _score_rows(scores_by_row, n):
    """A graph whose row r has the in-edges scores_by_row[r] (one fresh source per edge, every other row a self-loop) and zl / zr / attn
    (H = 1, F = 4) that give EXACTLY those scores: attn = (1, -1, 0, 0), zr = 0, zl_j = (s, 0, v, v) for s > 0 and (0, -s, v, v) for
    s < 0 -- leaky_relu is the identity on u >= 0.  Columns 2 and 3 carry the values that are aggregated."""
    src, dst, zl = [], [], np.zeros((n, 4), np.float32)
    nxt = len(scores_by_row)
    for r, sc in enumerate(scores_by_row):
        for s in sc:
            src.append(nxt)
            dst.append(r)
            zl[nxt] = (s, 0, 0.5 + s / 80, -s / 40) if s > 0 else (0, -s, 0.5 + s / 80, -s / 40)
            nxt += 1
    assert nxt <= n
    loops = np.arange(len(scores_by_row), n)
    return np.concatenate([src, loops]).astype(np.int64), np.concatenate([dst, loops]).astype(np.int64), zl


def test_online_softmax_late_maximum_reversed_row_and_last_wave_hub():
    """Row 0: 100 edges (one wave, two chunks) whose scores span -40 .. 30 and whose LAST edge scores 40, so the running maximum is
    replaced at the very end.  Row 1: the same edges in reverse order (maximum first).  Row 2: a hub of 500 edges -- eight chunks, one
    per wave, the last of 52 -- whose maximum is the last edge, in the last wave's share; row 3: that hub reversed.  Forward and backward
    against the oracle; reversed rows agree within 1e-4; everything is finite."""
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    rs = np.random.RandomState(0)
    short = np.concatenate([rs.uniform(-40, 30, 99), [40.0]]).astype(np.float32)
    hub = np.concatenate([rs.uniform(-40, 30, 499), [40.0]]).astype(np.float32)
    n = 4 + 2 * (100 + 500) + 20
    src, dst, zl = _score_rows([short, short[::-1], hub, hub[::-1]], n)
    ip, ix = csr_from_edges(src, dst, n)
    assert np.diff(ip)[:4].tolist() == [100, 100, 500, 500] and (np.diff(ip)[4:] == 1).all()
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)
    zr = np.zeros((n, 4), np.float32)
    at = np.array([[1.0, -1.0, 0.0, 0.0]], np.float32)
    ref, c = vo.attn_fwd(ip, ix, zl.reshape(n, 1, 4), zr.reshape(n, 1, 4), at, relu=False)
    np.testing.assert_allclose(c["s"][:100, 0], short, rtol=1e-6)                        # the construction gives the scores it claims
    np.testing.assert_allclose(c["s"][200:700, 0], hub, rtol=1e-6)
    assert c["s"][:100, 0].argmax() == 99 and c["s"][200:700, 0].argmax() == 499 and 499 // 64 == 7
    out, out_buf = _nan_rows(n, 4)
    lse = torch.full((n, 1), NAN, dtype=torch.float32, device=DEV)
    tzl, tzr, tat = _t(zl), _t(zr), _t(at).view(1, 1, 4)
    ops.gatv2_attn_fwd(g.indptr, g.indices, len(ix), tzl, tzr, tat, 1, 4, out=out, lse=lse)
    o, l = out.cpu().numpy(), lse.cpu().numpy()
    print("late-maximum rows: out", o[:4].tolist(), "lse", l[:4, 0].tolist(), "max|err|", np.abs(o - ref.reshape(n, 4)).max())
    assert np.isfinite(o).all() and np.isfinite(l).all()
    np.testing.assert_allclose(o, ref.reshape(n, 4), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(l, c["lse"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(o[0], o[1], rtol=1e-4, atol=1e-4)                          # the edge order does not matter
    np.testing.assert_allclose(o[2], o[3], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(l[[0, 2]], l[[1, 3]], rtol=1e-4, atol=1e-4)
    gy = rs.standard_normal((n, 4)).astype(np.float32)
    dzl, dzr, dattn = ops.gatv2_attn_bwd(g, tzl, tzr, lse, tat, _t(gy), 1, 4)
    rdzl, rdzr, rdat, _ = vo.attn_bwd(c, gy)
    for name, a, b in (("dzl", dzl, rdzl), ("dzr", dzr, rdzr), ("dattn", dattn, rdat)):
        a, b = a.cpu().numpy().reshape(b.shape), np.asarray(b)
        print(f"late-maximum rows {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}")
        assert np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=name)


# ---------------------------------------------------------------------------------------------------------------- launch geometry
# The numbers scan_grid and gatv2_rows_kernel derive the grid from, mirrored by name (csrc/row_gather_dev.h):
K_BLOCK = 512                 # kBlock: the rows one trip of the long-row scan looks at
K_WAVES = K_BLOCK // 64       # kWaves
K_ROWS_PER_WAVE = 8           # kRowsPerWave
K_LONG_ROW = 128              # kLongRow: a row above it is a whole workgroup's
K_LONG_BLOCK_ROWS = 512       # kLongBlockRows
K_LONG_BLOCK_CAP = 512        # kLongBlockCap
BIG_N = K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP + 656      # 262 800: just above the size at which every scan chunk has a workgroup of its own


def _geometry(n):
    return scan_geometry(n, K_BLOCK, K_WAVES, K_ROWS_PER_WAVE, K_LONG_BLOCK_ROWS, K_LONG_BLOCK_CAP)


def test_large_n_layer_matches_the_oracle():
    """The launch geometry a 600-row graph never reaches: eight rows per wave (rows_per_block = kRowsPerWave * kWaves), a last block that
    ends before its rows do, long rows -- destinations and, for the source pass, sources -- that the scan finds on its second trip, and
    the dattn fold's first level over more than kFoldPer partials."""
    from glnn_amd.graph import CSRGraph
    n_chunks, n_long_blocks, rows_per_block = _geometry(BIG_N)
    ip, ix = planted_graph(BIG_N, 17, *second_trip_plan(BIG_N, n_chunks, n_long_blocks, K_LONG_ROW))
    n = len(ip) - 1
    assert n > K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP and n_chunks > n_long_blocks          # the scan loop makes a second trip
    assert rows_per_block == K_ROWS_PER_WAVE * K_WAVES and n % rows_per_block != 0         # a wave takes eight rows; ragged last block
    assert n_long_blocks + -(-n // rows_per_block) > 128                                   # more dattn partials than one fold block takes
    deg, out_deg = np.diff(ip), np.bincount(ix, minlength=n)
    for d in (deg, out_deg):                                                # the in-CSR passes and the source pass over the transpose
        long_rows = np.flatnonzero(d > K_LONG_ROW)
        assert (long_rows % n_chunks >= n_long_blocks).sum() >= 2 and (long_rows % n_chunks < n_long_blocks).sum() >= 2
        assert {K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1} <= set(d.tolist())
        assert ((d > 64) & (d < K_LONG_ROW)).any()                           # a one-wave row of two 64-entry chunks
    assert deg.min() == 1 and (deg == 1).sum() > 100
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)
    _check_layer(ip, ix, g, 2, 4, 0.3, d_in=8)


@pytest.mark.parametrize("H,F", [(8, 16), (1, 47), (8, 7), (5, 6), (33, 7)])
def test_two_runs_are_bit_identical(H, F):
    from glnn_amd import ops
    from glnn_amd.autograd import gatv2_layer_bwd, gatv2_layer_fwd
    ip, ix, g = _graph(3000, seed=11)
    x, p, gy = _layer_inputs(3000, 24, H, F, 5)
    tp = {k: _t(v) for k, v in p.items()}
    tx, tg = ops.as_feat(_t(x)), ops.as_feat(_t(gy))

    def run(seed):
        y, saved = gatv2_layer_fwd(g, tx, tp["fc_src.weight"], tp["fc_src.bias"], tp["fc_dst.weight"], tp["fc_dst.bias"], tp["attn"], H, F,
                                   0.2, False, 0.5, 3, 0.3, seed, want_lse=True)
        return (y, saved[3]) + gatv2_layer_bwd(g, tg, saved, tp["fc_src.weight"], tp["fc_dst.weight"], tp["attn"], H, F, 0.2, 0.3, seed)

    a, b, c = run(99), run(99), run(100)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], c[0])                                       # the seed matters


# ---------------------------------------------------------------------------------------------------------------- Model surface
P_FEAT, P_ATTN, LR, WD, STEPS = 0.5, 0.3, 0.01, 0.01, 3
TORCH_SEED = 4321             # TeacherEngine.base_seed and autograd's seeds come from torch.initial_seed()
DROP_COUNT = 1000             # autograd._drop_counter is set here before a differentiated forward: its masks are then fixed
M_N, M_FEAT, M_HIDDEN, M_HEADS, M_LABEL = 32, 12, 64, 8, 5
# numpy seeds of _problem, found by search: the oracle's smallest |pre-activation| and smallest |u_ij| exceed 1e-4 in the eval
# forward, under the masks of the differentiated forward, and in each of the three training steps (each test asserts its own first)
PROBLEM_SEED = {2: 646, 3: 154306}


def _problem(L, seed):
    """(ip, ix, params, x, labels, idx) of an L-layer GATv2 of 8 heads at hidden 64 on a 32-row multigraph with self-loops."""
    rs = np.random.RandomState(seed)
    ip, ix = random_graph(M_N, 3, seed=seed, self_loops=True)
    dims = [(M_FEAT, M_HEADS, M_HIDDEN // M_HEADS)] + [(M_HIDDEN, M_HEADS, M_HIDDEN // M_HEADS)] * (L - 2) + [(M_HIDDEN, 1, M_LABEL)]
    params = {}
    for l, (d_in, H, F) in enumerate(dims):
        pre = f"encoder.layers.{l}."
        params[pre + "fc_src.weight"] = (rs.standard_normal((H * F, d_in)) * (2.0 / d_in) ** 0.5).astype(np.float32)
        params[pre + "fc_src.bias"] = (rs.standard_normal(H * F) * 0.1).astype(np.float32)
        params[pre + "fc_dst.weight"] = (rs.standard_normal((H * F, d_in)) * (2.0 / d_in) ** 0.5).astype(np.float32)
        params[pre + "fc_dst.bias"] = (rs.standard_normal(H * F) * 0.1).astype(np.float32)
        params[pre + "attn"] = (rs.standard_normal((1, H, F)) * 0.5).astype(np.float32)
    x = rs.standard_normal((M_N, M_FEAT)).astype(np.float32)
    return ip, ix, params, x, rs.randint(0, M_LABEL, M_N).astype(np.int64), np.sort(rs.permutation(M_N)[:16]).astype(np.int64)


def _layer_shapes(L):
    return [(M_FEAT, M_HEADS)] + [(M_HIDDEN, M_HEADS)] * (L - 2) + [(M_HIDDEN, 1)]


def _lib_masks(ops, nnz, L, feat_seeds, attn_seeds):
    """The library's masks of one forward: per layer a feature mask [N, in] and an attention mask [E, H]."""
    shapes = _layer_shapes(L)
    fm = [ops.dropout_mask(M_N, shapes[l][0], P_FEAT, feat_seeds[l], DEV).cpu().numpy() for l in range(L)]
    am = [ops.gat_attn_mask(nnz, shapes[l][1], P_ATTN, attn_seeds[l], DEV).cpu().numpy() for l in range(L)]
    return fm, am


def _assert_margins(caches):
    pre, u = vo.min_margins(caches)
    print(f"smallest |pre-activation| {pre:.3e}, smallest |u_ij| {u:.3e}")
    assert pre > 1e-4 and u > 1e-4


def _model(L, params, p_feat=P_FEAT, p_attn=P_ATTN):
    from glnn_amd.models import GATv2, Model
    m = Model(dict(model_name="GATv2", num_layers=L, feat_dim=M_FEAT, hidden_dim=M_HIDDEN, label_dim=M_LABEL, dropout_ratio=p_feat,
                   norm_type="none", device=DEV, num_heads=M_HEADS, attn_dropout_ratio=p_attn))
    assert type(m.encoder) is GATv2 and set(m.state_dict()) == set(params)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m


def _setup(L):
    from glnn_amd.graph import CSRGraph
    ip, ix, params, x, labels, idx = _problem(L, PROBLEM_SEED[L])
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), M_N)
    return ip, ix, params, x, labels, idx, g, _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)


def _params(m):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("L", [2, 3])
def test_model_eval_forward_and_inference_match_the_oracle(L):
    ip, ix, params, x, labels, idx, g, tx, _, _ = _setup(L)
    h_ref, ref, caches = vo.model_fwd(params, ip, ix, x, L)
    _assert_margins(caches)
    m = _model(L, params)
    m.eval()
    h_list, logits = m.forward_fitnet(g, tx)
    assert len(h_list) == L - 1 and all(tuple(h.shape) == (M_N, M_HIDDEN) for h in h_list)
    for a, b in zip(h_list, h_ref):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(logits.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m(g, tx).cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m.inference(g, tx).cpu().numpy(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("L", [2, 3])
def test_loss_backward_matches_the_oracle_fed_the_library_masks(L, monkeypatch):
    """Model.forward in training mode differentiates through Gatv2ConvFn, both dropouts on."""
    from glnn_amd import autograd, ops
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(L)
    torch.manual_seed(TORCH_SEED)
    monkeypatch.setattr(autograd, "_drop_counter", [DROP_COUNT])
    seeds = [autograd.gatv2_conv_seeds(DROP_COUNT + 1 + l) for l in range(L)]
    fm, am = _lib_masks(ops, len(ix), L, [s[0] for s in seeds], [s[1] for s in seeds])
    ref_loss, grads, ref_logits = vo.loss_grads(params, ip, ix, x, labels, idx, L, fm, P_FEAT, am, P_ATTN)
    _assert_margins(vo.model_fwd(params, ip, ix, x, L, fm, P_FEAT, am, P_ATTN)[2])
    m = _model(L, params)
    m.train()
    logits = m(g, tx)
    assert logits.requires_grad and autograd._drop_counter[0] == DROP_COUNT + L
    loss = torch.nn.NLLLoss()(logits.log_softmax(dim=1)[tidx], tlabels[tidx])
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-4)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[name].reshape(p.shape), rtol=1e-3, atol=1e-4, err_msg=name)


def _engine_masks(ops, eng, nnz, L, step):
    """The masks TeacherEngine draws in step `step` (its seeds depend on base_seed and the step count alone)."""
    keep = eng.step_count
    eng.step_count = step
    try:
        return _lib_masks(ops, nnz, L, [eng._seed(l) for l in range(L)], [eng._attn_seed(l) for l in range(L)])
    finally:
        eng.step_count = keep


@pytest.mark.parametrize("L", [2, 3])
def test_step_gatv2_gradients_match_the_oracle(L):
    from glnn_amd import ops, teacher
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(L)
    torch.manual_seed(TORCH_SEED)
    m = _model(L, params)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    eng = teacher.get_engine(m, opt)
    assert eng.kind == "gatv2" and eng.base_seed == TORCH_SEED
    fm, am = _engine_masks(ops, eng, len(ix), L, 1)
    ref_loss, grads, _ = vo.loss_grads(params, ip, ix, x, labels, idx, L, fm, P_FEAT, am, P_ATTN)
    _assert_margins(vo.model_fwd(params, ip, ix, x, L, fm, P_FEAT, am, P_ATTN)[2])
    eng.step_count += 1
    with torch.no_grad():
        eng._step_gatv2_body(g, tx, tlabels, tidx, 1.0)
    np.testing.assert_allclose(eng.loss_out.item(), ref_loss, rtol=1e-4)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(eng.grad(p).cpu().numpy(), grads[name].reshape(p.shape), rtol=1e-3, atol=1e-4, err_msg=name)


@pytest.mark.parametrize("L", [2, 3])
def test_train_steps_match_the_oracle(L):
    """train() (TeacherEngine.step_gatv2) for three steps == the fp64 oracle's Adam fed the library's masks of each step."""
    from glnn_amd import ops, teacher
    from glnn_amd.train_and_eval import train
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(L)
    torch.manual_seed(TORCH_SEED)
    m = _model(L, params)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    eng = teacher.get_engine(m, opt)
    masks = [_engine_masks(ops, eng, len(ix), L, s + 1) for s in range(STEPS)]
    fms, ams = [mk[0] for mk in masks], [mk[1] for mk in masks]
    for s in range(STEPS):                                                   # the margins of every step, along the oracle's own trajectory
        p = params if s == 0 else vo.train_steps(params, ip, ix, x, labels, idx, L, fms[:s], P_FEAT, ams[:s], P_ATTN, LR, WD, s)[1]
        _assert_margins(vo.model_fwd(p, ip, ix, x, L, fms[s], P_FEAT, ams[s], P_ATTN)[2])
    ref_losses, ref_params = vo.train_steps(params, ip, ix, x, labels, idx, L, fms, P_FEAT, ams, P_ATTN, LR, WD, STEPS)
    losses = []
    for s in range(STEPS):
        losses.append(train(m, g, tx, tlabels, torch.nn.NLLLoss(), opt, tidx))
        assert teacher.get_engine(m, opt) is eng and eng.step_count == s + 1
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    fin = _params(m)
    for k, v in ref_params.items():
        np.testing.assert_allclose(fin[k], v, rtol=1e-3, atol=1e-4, err_msg=k)
    assert any(not np.array_equal(fms[0][l], fms[1][l]) for l in range(L))       # the seed streams move with the step count


def test_limits_and_zero_in_degree():
    from glnn_amd import ops
    from glnn_amd._lib import GlnnError
    from glnn_amd.graph import CSRGraph
    from glnn_amd.train_and_eval import train
    loops = CSRGraph(torch.arange(4, dtype=torch.int64, device=DEV), torch.arange(3, dtype=torch.int32, device=DEV), 3)
    for H, F in ((65, 1), (1, 257)):                                         # heads = 65; heads * out_feats = 257
        z, at, s3 = torch.zeros(3, H * F, device=DEV), torch.zeros(1, H, F, device=DEV), torch.zeros(3, H, device=DEV)
        with pytest.raises(GlnnError, match=r"status -2.*heads <= 64 and heads \* out_feats <= 256"):
            ops.gatv2_attn_fwd(loops.indptr, loops.indices, 3, z, z, at, H, F)
        with pytest.raises(GlnnError, match=r"status -2.*heads <= 64 and heads \* out_feats <= 256"):
            ops.gatv2_attn_bwd(loops, z, z, s3, at, z, H, F)
    ip, ix, params, x, labels, idx = _problem(2, PROBLEM_SEED[2])
    m = _model(2, params)
    m.eval()
    bad = CSRGraph(torch.tensor([0, 1, 1, 2], dtype=torch.int64, device=DEV), torch.tensor([1, 0], dtype=torch.int32, device=DEV), 3)
    x3 = torch.zeros(3, M_FEAT, device=DEV)
    with pytest.raises(RuntimeError, match="0-in-degree"):
        m(bad, x3)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    with pytest.raises(RuntimeError, match="0-in-degree"):
        train(m, bad, x3, torch.zeros(3, dtype=torch.int64, device=DEV), torch.nn.NLLLoss(), opt, torch.arange(3, device=DEV))
    with pytest.raises(NotImplementedError, match="bipartite"):
        m([loops], x3)


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_gatv2_teacher_then_student_cli(tmp_path):
    common = ["--dataset", "synthetic-cora", "--teacher", "GATv2", "--device", "0", "--max_epoch", "2",
              "--model_config_path", os.path.join(ROOT, "train.conf.yaml")]
    _run("train_teacher.py", common + ["--save_results"], tmp_path)
    base = tmp_path / "outputs" / "transductive" / "synthetic-cora"
    out_t = np.load(base / "GATv2" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    curves = np.load(base / "GATv2" / "seed_0" / "loss_and_score.npz")["arr_0"]
    assert np.isfinite(curves).all()                                           # a finite loss every epoch
    sd = torch.load(base / "GATv2" / "seed_0" / "model.pth", map_location="cpu")
    assert tuple(sd["encoder.layers.0.attn"].shape) == (1, 8, 16) and tuple(sd["encoder.layers.1.fc_dst.bias"].shape) == (7,)
    _run("train_student.py", common + ["--student", "MLP"], tmp_path)
    out_s = np.load(base / "GATv2_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
    np.testing.assert_allclose(np.exp(out_s).sum(1), 1.0, atol=1e-4)
