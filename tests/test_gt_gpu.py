"""GraphTransformer teacher on the GPU: the attention kernels (csrc/gt.hip) against the fp64 oracle (tests/gt_oracle.py) at every lane
layout and launch geometry, the online softmax's edge cases, determinism, the limits, the Model surface, gradients and training steps
against the oracle fed the library's own masks, a random-walk subgraph batch, and the command lines.

Tolerances (docs/GT_SEMANTICS.md, Tolerances): rtol = atol = 1e-4 on q, k, v, skip, lse, the outputs, dq, dk and dv; the gradients that
sum over all rows (dW_*, db_*) and dx take max(1e-4 + 1e-4 |ref|, 4 x the error of an fp32 CPU stand-in -- the oracle's own arithmetic
run in fp32 -- against the fp64 oracle on the same inputs); the stand-in's error is computed per case and printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gt_oracle as to
from graphgen import csr_from_edges, planted_graph, random_graph, second_trip_plan
from oracle.dropout_mask import drop_hash, drop_threshold
from test_gat_gpu import _graph
from test_gatv2_gpu import BIG_N, K_LONG_BLOCK_CAP, K_LONG_BLOCK_ROWS, K_LONG_ROW, K_ROWS_PER_WAVE, K_WAVES, SHAPES, _geometry

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


def _layer_inputs(n, d_in, H, D, seed):
    rs = np.random.RandomState(seed)
    f32 = lambda a: a.astype(np.float32)
    p = {"heads": H}
    for lin in to.LINS:
        p[lin + ".weight"], p[lin + ".bias"] = f32(rs.standard_normal((H * D, d_in)) * 0.3), f32(rs.standard_normal(H * D) * 0.2)
    return f32(rs.standard_normal((n, d_in))), p, f32(rs.standard_normal((n, H * D)))


def _flat(p):
    """The (w, b) of the four projections in construction order, as device tensors."""
    return [_t(p[f"{lin}.{part}"]) for lin in to.LINS for part in ("weight", "bias")]


def test_graph_has_the_rows_the_kernels_branch_on(graph):
    ip, ix, _ = graph
    deg = np.diff(ip)
    assert len(deg) == 600 and deg.min() == 1 and deg.max() > 640          # self-loops on the isolated rows; a hub of about 700
    out_deg = np.bincount(ix, minlength=len(deg))
    assert out_deg.max() >= 700 and ((out_deg > 64) & (out_deg <= 128)).any()           # the source pass: a workgroup row, a two-chunk row
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(len(deg)), deg)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                      # a multi-edge


def _check_layer(ip, ix, g, H, D, p_attn, d_in=20):
    """One layer on graph (ip, ix, g) against the oracle fed the masks the helpers write; every figure is printed before it is asserted.
    Every buffer a kernel writes is NaN-filled first, padding columns included, and the padding is checked to come back zero."""
    from glnn_amd import ops
    from glnn_amd.autograd import gt_layer_bwd, gt_layer_fwd
    n, nnz, hd = len(ip) - 1, len(ix), H * D
    relu = H > 1
    p_feat = 0.4 if p_attn > 0 else 0.0
    fs, as_ = 1234 + H, 99 + D
    x, p, gy = _layer_inputs(n, d_in, H, D, H * 100 + D)
    flat = _flat(p)
    wk, wq, wv, ws = flat[0::2]
    tx = ops.as_feat(_t(x))
    fm = ops.dropout_mask(n, d_in, p_feat, fs, DEV).cpu().numpy() if p_feat > 0 else None
    am = ops.gat_attn_mask(nnz, H, p_attn, as_, DEV).cpu().numpy() if p_attn > 0 else None
    ref, c = to.layer_fwd(ip, ix, x, p, relu, fm, p_feat, am, p_attn)
    r32, c32 = to.layer_fwd(ip, ix, x, p, relu, fm, p_feat, am, p_attn, dtype=np.float32)
    # forward
    y, (xd, q, k, v, lse) = gt_layer_fwd(g, tx, *flat, H, D, 0.2, relu, p_feat, fs, p_attn, as_, want_lse=True)
    s = ops.gemm(xd, ws, ep_shift=flat[7])
    out, out_buf = _nan_rows(n, hd)
    lse2 = torch.full((n, H), NAN, dtype=torch.float32, device=DEV)
    ops.gt_attn_fwd(g.indptr, g.indices, nnz, q, k, v, s, H, D, p_attn, as_, relu=relu, out=out, lse=lse2)
    assert torch.equal(out, y) and torch.equal(lse2, lse) and not out_buf[:, hd:].any()
    skip_ref = c["h"] @ c["w"]["lin_skip"].T + np.asarray(p["lin_skip.bias"], np.float64)
    for name, a, b in (("q", q, c["q"]), ("k", k, c["k"]), ("v", v, c["v"]), ("skip", s, skip_ref), ("lse", lse, c["lse"]), ("out", y, ref)):
        a, b = a.cpu().numpy(), np.asarray(b).reshape(n, -1)
        print(f"n={n} H={H} D={D} p_attn={p_attn} {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=name)
    # backward
    gm = gy * (ref > 0) if relu else gy                                    # the activation mask is the caller's
    tg = ops.as_feat(_t(gm))
    bufs = {name: _nan_rows(n, hd) for name in ("dq", "dk", "dv")}
    ops.gt_attn_bwd(g, q, k, v, lse, tg, H, D, p_attn, as_, **{name: b[0] for name, b in bufs.items()})
    assert not any(b[1][:, hd:].any() for b in bufs.values())
    da, dw, db = gt_layer_bwd(g, tg, (xd, q, k, v, lse), wk, wq, wv, ws, H, D, p_attn, as_)
    rdq, rdk, rdv, _, _ = to.attn_bwd(c, gy)
    for name, b in (("dq", rdq), ("dk", rdk), ("dv", rdv)):
        a, b = bufs[name][0].cpu().numpy(), b.reshape(n, -1)
        print(f"n={n} H={H} D={D} p_attn={p_attn} {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=name)
    dx, grads = to.layer_bwd(c, gy)
    sdx, sgrads = to.layer_bwd(c32, gy)
    got = [("dx", da.cpu().numpy() * c["fm"], dx, sdx)]
    for i, lin in enumerate(to.LINS):
        got += [(f"{lin}.weight", dw[i].cpu().numpy(), grads[f"{lin}.weight"], sgrads[f"{lin}.weight"]),
                (f"{lin}.bias", db[i].cpu().numpy(), grads[f"{lin}.bias"], sgrads[f"{lin}.bias"])]
    worst = []
    for name, a, b, s32 in got:
        e32 = float(np.abs(s32.astype(np.float64) - b).max())
        print(f"n={n} H={H} D={D} p_attn={p_attn} d {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e} "
              f"fp32 stand-in max|err| {e32:.3e}")
        bad = np.abs(a - b) > np.maximum(1e-4 + 1e-4 * np.abs(b), 4.0 * e32)
        if bad.any():
            worst.append(f"{name}: {bad.sum()} elements, max|err| {np.abs(a - b).max():.3e}, fp32 stand-in max|err| {e32:.3e}")
    assert not worst, worst


@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("p_attn", [0.0, 0.3])
def test_layer_forward_and_backward_match_the_oracle(graph, H, D, p_attn):
    """The four projections, the attention forward (+ ReLU on the multi-head shapes), both backward passes, weight, bias and input
    gradients against the oracle fed the masks the helpers write, on the 600-row graph: a 700-edge hub destination (a workgroup row with
    every wave's share of the merge), degree-1 rows, a multi-edge, and in the transpose a 700-edge source and one of two chunks.  The 17
    shapes are test_gatv2_gpu's: gt_rows_kernel<KIND, LPR, UNI> is picked as gatv2_rows_kernel is (docs/KERNEL_COVERAGE.md)."""
    ip, ix, g = graph
    _check_layer(ip, ix, g, H, D, p_attn)


def test_large_n_layer_matches_the_oracle():
    """The launch geometry a 600-row graph never reaches: eight rows per wave (rows_per_block = kRowsPerWave * kWaves), a last block that
    ends before its rows do, and long rows -- destinations and, for the source pass, sources -- that the scan finds on its second trip."""
    from glnn_amd.graph import CSRGraph
    n_chunks, n_long_blocks, rows_per_block = _geometry(BIG_N)
    ip, ix = planted_graph(BIG_N, 17, *second_trip_plan(BIG_N, n_chunks, n_long_blocks, K_LONG_ROW))
    n = len(ip) - 1
    assert n > K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP and n_chunks > n_long_blocks          # the scan loop makes a second trip
    assert rows_per_block == K_ROWS_PER_WAVE * K_WAVES and n % rows_per_block != 0         # a wave takes eight rows; ragged last block
    deg, out_deg = np.diff(ip), np.bincount(ix, minlength=n)
    for d in (deg, out_deg):                                                # the in-CSR passes and the source pass over the transpose
        long_rows = np.flatnonzero(d > K_LONG_ROW)
        assert (long_rows % n_chunks >= n_long_blocks).sum() >= 2 and (long_rows % n_chunks < n_long_blocks).sum() >= 2
        assert {K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1} <= set(d.tolist())
        assert ((d > 64) & (d < K_LONG_ROW)).any()                           # a one-wave row of two 64-entry chunks
    assert deg.min() == 1 and (deg == 1).sum() > 100
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)
    _check_layer(ip, ix, g, 2, 4, 0.3, d_in=8)


# ---------------------------------------------------------------------------------------------------------------- online softmax
def _score_rows(scores_by_row, n):
    """A graph whose row r has the in-edges scores_by_row[r] (one fresh source per edge, every other row a self-loop) and q / k / v
    (H = 1, D = 4: scale 1/2) that give EXACTLY those scores: q_r = (2, 0, 0, 0) on the scored rows and 0 elsewhere, k_j = (s, 0, 0, 0).
    v_j carries the values that are aggregated, skip the row's number."""
    src, dst = [], []
    q, k, v = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    nxt = len(scores_by_row)
    for r, sc in enumerate(scores_by_row):
        q[r, 0] = 2.0
        for s in sc:
            src.append(nxt)
            dst.append(r)
            k[nxt, 0] = s
            v[nxt] = (0.5 + s / 200, -s / 100, 1.0, s / 50)
            nxt += 1
    assert nxt <= n
    loops = np.arange(len(scores_by_row), n)
    skip = (np.arange(n, dtype=np.float32)[:, None] * 0.01 + np.array([0.0, 0.25, -0.5, 1.0], np.float32)).astype(np.float32)
    return np.concatenate([src, loops]).astype(np.int64), np.concatenate([dst, loops]).astype(np.int64), q, k, v, skip


def test_online_softmax_scores_near_90_late_maximum_reversed_row_and_last_wave_hub():
    """Row 0: 100 edges (one wave, two chunks) whose scores span -90 .. 60 and whose LAST edge scores 90, so the running maximum is
    replaced at the very end.  Row 1: the same edges in reverse order (maximum first).  Row 2: a hub of 500 edges -- eight chunks, one
    per wave, the last of 52 -- whose maximum is the last edge, in the last wave's share; row 3: that hub reversed.  Forward and backward
    against the oracle; reversed rows agree within 1e-4; everything is finite."""
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    rs = np.random.RandomState(0)
    short = np.concatenate([[-90.0], rs.uniform(-90, 60, 98), [90.0]]).astype(np.float32)
    hub = np.concatenate([[-90.0], rs.uniform(-90, 60, 498), [90.0]]).astype(np.float32)
    n = 4 + 2 * (100 + 500) + 20
    src, dst, q, k, v, skip = _score_rows([short, short[::-1], hub, hub[::-1]], n)
    ip, ix = csr_from_edges(src, dst, n)
    assert np.diff(ip)[:4].tolist() == [100, 100, 500, 500] and (np.diff(ip)[4:] == 1).all()
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)
    r4 = lambda a: a.reshape(n, 1, 4)
    ref, c = to.attn_fwd(ip, ix, r4(q), r4(k), r4(v), r4(skip), relu=False)
    np.testing.assert_allclose(c["e"][:100, 0], short, rtol=1e-6)                        # the construction gives the scores it claims
    np.testing.assert_allclose(c["e"][200:700, 0], hub, rtol=1e-6)
    assert c["e"][:100, 0].argmax() == 99 and c["e"][200:700, 0].argmax() == 499 and 499 // 64 == 7
    assert c["e"].max() == 90.0 and c["e"].min() == -90.0
    out, out_buf = _nan_rows(n, 4)
    lse = torch.full((n, 1), NAN, dtype=torch.float32, device=DEV)
    tq, tk, tv, ts = _t(q), _t(k), _t(v), _t(skip)
    ops.gt_attn_fwd(g.indptr, g.indices, len(ix), tq, tk, tv, ts, 1, 4, out=out, lse=lse)
    o, l = out.cpu().numpy(), lse.cpu().numpy()
    print("late-maximum rows: out", o[:4].tolist(), "lse", l[:4, 0].tolist(), "max|err|", np.abs(o - ref.reshape(n, 4)).max())
    assert np.isfinite(o).all() and np.isfinite(l).all()
    np.testing.assert_allclose(o, ref.reshape(n, 4), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(l, c["lse"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(o[0] - skip[0], o[1] - skip[1], rtol=1e-4, atol=1e-4)      # the edge order does not matter
    np.testing.assert_allclose(o[2] - skip[2], o[3] - skip[3], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(l[[0, 2]], l[[1, 3]], rtol=1e-4, atol=1e-4)
    gy = rs.standard_normal((n, 4)).astype(np.float32)
    dq, dk, dv = ops.gt_attn_bwd(g, tq, tk, tv, lse, _t(gy), 1, 4)
    rdq, rdk, rdv, _, _ = to.attn_bwd(c, gy)
    for name, a, b in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        a, b = a.cpu().numpy(), b.reshape(n, 4)
        print(f"late-maximum rows {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e}")
        assert np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=name)


def test_all_dropped_row_zero_in_degree_row_and_empty_graph():
    """Row 0: three in-edges whose every head is dropped (the seed is found on the CPU restatement of the mask and the library's mask is
    asserted to agree): its output is its skip row, its lse the softmax's all the same.  Row 1: no in-edge at kernel level: out = skip,
    lse = 0, dq = 0.  Row 2: a kept self-loop.  Then n == 0: a no-op that reads no pointer."""
    from glnn_amd import _lib, ops
    from glnn_amd.graph import CSRGraph
    H, D, p = 2, 3, 0.5
    ip, ix = csr_from_edges(np.array([2, 3, 4, 2, 3, 4]), np.array([0, 0, 0, 2, 3, 4]), 5)
    assert ip.tolist() == [0, 3, 3, 4, 5, 6]
    thr = drop_threshold(p)
    eid, hh = np.meshgrid(np.arange(6), np.arange(H), indexing="ij")
    keep = lambda seed: ((drop_hash(seed, eid, hh) & 0xFFFF) >= thr).astype(np.uint8)
    seed = next(s for s in range(1, 100000) if not keep(s)[:3].any() and keep(s)[3].all())
    am = ops.gat_attn_mask(6, H, p, seed, DEV).cpu().numpy()
    np.testing.assert_array_equal(am, keep(seed))
    assert not am[:3].any() and am[3].all()
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), 5)
    rs = np.random.RandomState(1)
    q, k, v, s, gy = (rs.standard_normal((5, H * D)).astype(np.float32) for _ in range(5))
    r3 = lambda a: a.reshape(5, H, D)
    ref, c = to.attn_fwd(ip, ix, r3(q), r3(k), r3(v), r3(s), relu=False, attn_mask=am, attn_p=p)
    out, out_buf = _nan_rows(5, H * D)
    lse = torch.full((5, H), NAN, dtype=torch.float32, device=DEV)
    tq, tk, tv, ts = _t(q), _t(k), _t(v), _t(s)
    ops.gt_attn_fwd(g.indptr, g.indices, 6, tq, tk, tv, ts, H, D, p, seed, out=out, lse=lse)
    o, l = out.cpu().numpy(), lse.cpu().numpy()
    np.testing.assert_array_equal(o[0], s[0])                                # every head of every edge dropped: exactly the skip row
    np.testing.assert_array_equal(o[1], s[1])                                # no in-edge: exactly the skip row
    assert not out_buf[:, H * D:].any() and (l[1] == 0).all()
    np.testing.assert_allclose(o, ref.reshape(5, -1), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(l, c["lse"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(o[2], 2.0 * v[2] + s[2], rtol=1e-5, atol=1e-6)            # a = 1, kept at weight 1 / (1 - p)
    bufs = {name: _nan_rows(5, H * D) for name in ("dq", "dk", "dv")}
    ops.gt_attn_bwd(g, tq, tk, tv, lse, _t(gy), H, D, p, seed, **{name: b[0] for name, b in bufs.items()})
    rdq, rdk, rdv, _, _ = to.attn_bwd(c, gy)
    for name, b in (("dq", rdq), ("dk", rdk), ("dv", rdv)):
        np.testing.assert_allclose(bufs[name][0].cpu().numpy(), b.reshape(5, -1), rtol=1e-4, atol=1e-4, err_msg=name)
        assert not bufs[name][1][:, H * D:].any()
    assert not bufs["dq"][0][1].any() and not bufs["dq"][0][0].any()         # no in-edge; every c_ij = 0, so every t_ij = 0
    h = _lib.lib()
    assert h.glnn_gt_attn_fwd_f32(None, None, 0, 0, None, 8, None, 8, None, 8, None, 8, H, D, 0.0, 0, 0, None, 8, None, None) == 0
    assert h.glnn_gt_attn_bwd_f32(None, None, None, None, None, 0, 0, None, 8, None, 8, None, 8, H, D, None, None, 8, 0.0, 0, None, None, 8,
                                  None, 8, None, 8, None, 0, None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,D", [(8, 16), (1, 47), (8, 7), (5, 6), (33, 7)])
def test_two_runs_are_bit_identical(H, D):
    from glnn_amd import ops
    from glnn_amd.autograd import gt_layer_bwd, gt_layer_fwd
    ip, ix, g = _graph(3000, seed=11)
    x, p, gy = _layer_inputs(3000, 24, H, D, 5)
    flat = _flat(p)
    tx, tg = ops.as_feat(_t(x)), ops.as_feat(_t(gy))

    def run(seed):
        y, saved = gt_layer_fwd(g, tx, *flat, H, D, 0.2, False, 0.5, 3, 0.3, seed, want_lse=True)
        dq, dk, dv = ops.gt_attn_bwd(g, saved[1], saved[2], saved[3], saved[4], tg, H, D, 0.3, seed)
        da, dw, db = gt_layer_bwd(g, tg, saved, *flat[0::2], H, D, 0.3, seed)
        return (y, saved[4], dq, dk, dv, da, *dw, *db)

    a, b, c = run(99), run(99), run(100)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], c[0])                                       # the seed matters


# ---------------------------------------------------------------------------------------------------------------- Model surface
P_FEAT, P_ATTN, LR, WD, STEPS = 0.5, 0.3, 0.01, 0.01, 3
TORCH_SEED = 4321             # TeacherEngine.base_seed and autograd's seeds come from torch.initial_seed()
DROP_COUNT = 1000             # autograd._drop_counter is set here before a differentiated forward: its masks are then fixed
M_N, M_FEAT, M_HIDDEN, M_HEADS, M_LABEL = 32, 12, 64, 8, 5
# numpy seeds of _problem, found by a search on the CPU (the masks restated by oracle/dropout_mask.py): the oracle's smallest
# |pre-activation| exceeds 1e-4 in the eval forward, under the masks of the differentiated forward, and in each of the three training
# steps (each test asserts its own first)
PROBLEM_SEED = {2: 1, 3: 5}


def _problem(L, seed):
    """(ip, ix, params, x, labels, idx) of an L-layer GraphTransformer of 8 heads at hidden 64 on a 32-row multigraph with self-loops."""
    rs = np.random.RandomState(seed)
    ip, ix = random_graph(M_N, 3, seed=seed, self_loops=True)
    dims = [(M_FEAT, M_HIDDEN)] + [(M_HIDDEN, M_HIDDEN)] * (L - 2) + [(M_HIDDEN, M_LABEL)]
    params = {}
    for l, (d_in, hd) in enumerate(dims):
        for lin in to.LINS:
            params[f"encoder.layers.{l}.{lin}.weight"] = (rs.standard_normal((hd, d_in)) * (1.0 / d_in) ** 0.5).astype(np.float32)
            params[f"encoder.layers.{l}.{lin}.bias"] = (rs.standard_normal(hd) * 0.1).astype(np.float32)
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


def _assert_margin(caches):
    pre = to.min_margin(caches)
    print(f"smallest |pre-activation| {pre:.3e}")
    assert pre > 1e-4


def _model(L, params, p_feat=P_FEAT, p_attn=P_ATTN):
    from glnn_amd.models import GraphTransformer, Model
    m = Model(dict(model_name="GraphTransformer", num_layers=L, feat_dim=M_FEAT, hidden_dim=M_HIDDEN, label_dim=M_LABEL,
                   dropout_ratio=p_feat, norm_type="none", device=DEV, num_heads=M_HEADS, attn_dropout_ratio=p_attn))
    assert type(m.encoder) is GraphTransformer and set(m.state_dict()) == set(params)
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
    h_ref, ref, caches = to.model_fwd(params, ip, ix, x, L, M_HEADS)
    _assert_margin(caches)
    m = _model(L, params)
    m.eval()
    h_list, logits = m.forward_fitnet(g, tx)
    assert len(h_list) == L - 1 and all(tuple(h.shape) == (M_N, M_HIDDEN) for h in h_list)
    for a, b in zip(h_list, h_ref):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-4, atol=1e-4)
    for got in (logits, m(g, tx), m.inference(g, tx)):
        print(f"L={L} logits max|err| {np.abs(got.cpu().numpy() - ref).max():.3e}")
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=1e-4)
    with pytest.raises(NotImplementedError, match="not implemented for the GraphTransformer teacher"):
        m.inference(g, tx, dtype=torch.bfloat16)


@pytest.mark.parametrize("L", [2, 3])
def test_loss_backward_matches_the_oracle_fed_the_library_masks(L, monkeypatch):
    """Model.forward in training mode differentiates through GtConvFn, both dropouts on: the gradient of every parameter and of x."""
    from glnn_amd import autograd, ops
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(L)
    torch.manual_seed(TORCH_SEED)
    monkeypatch.setattr(autograd, "_drop_counter", [DROP_COUNT])
    seeds = [autograd.gt_conv_seeds(DROP_COUNT + 1 + l) for l in range(L)]
    assert seeds[0] != autograd.gatv2_conv_seeds(DROP_COUNT + 1) and seeds[0] != autograd.gat_conv_seeds(DROP_COUNT + 1)    # tags of its own
    fm, am = _lib_masks(ops, len(ix), L, [s[0] for s in seeds], [s[1] for s in seeds])
    ref_loss, grads, ref_logits = to.loss_grads(params, ip, ix, x, labels, idx, L, M_HEADS, fm, P_FEAT, am, P_ATTN)
    caches = to.model_fwd(params, ip, ix, x, L, M_HEADS, fm, P_FEAT, am, P_ATTN)[2]
    _assert_margin(caches)
    dlog = to.nll(ref_logits, labels, idx)[1]
    gx = dlog
    for c in caches[::-1]:
        gx = to.layer_bwd(c, gx)[0]
    m = _model(L, params)
    m.train()
    tx = tx.clone().requires_grad_(True)
    logits = m(g, tx)
    assert logits.requires_grad and autograd._drop_counter[0] == DROP_COUNT + L
    loss = torch.nn.NLLLoss()(logits.log_softmax(dim=1)[tidx], tlabels[tidx])
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits, rtol=0, atol=1e-4)
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-4)
    for name, p in m.named_parameters():
        print(f"L={L} d {name}: max|err| {np.abs(p.grad.cpu().numpy() - grads[name].reshape(p.shape)).max():.3e}")
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[name].reshape(p.shape), rtol=1e-3, atol=1e-4, err_msg=name)
    np.testing.assert_allclose(tx.grad.cpu().numpy(), gx, rtol=1e-3, atol=1e-4, err_msg="x")


def _engine_masks(ops, eng, nnz, L, step):
    """The masks TeacherEngine draws in step `step` (its seeds depend on base_seed and the step count alone)."""
    keep = eng.step_count
    eng.step_count = step
    try:
        return _lib_masks(ops, nnz, L, [eng._seed(l) for l in range(L)], [eng._attn_seed(l) for l in range(L)])
    finally:
        eng.step_count = keep


@pytest.mark.parametrize("L", [2, 3])
def test_train_steps_match_the_oracle(L):
    """train() (TeacherEngine.step_gt) for three steps == the fp64 oracle's Adam fed the library's masks of each step."""
    from glnn_amd import ops, teacher
    from glnn_amd.train_and_eval import train
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(L)
    torch.manual_seed(TORCH_SEED)
    m = _model(L, params)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    eng = teacher.get_engine(m, opt)
    assert eng.kind == "gt" and eng.base_seed == TORCH_SEED
    masks = [_engine_masks(ops, eng, len(ix), L, s + 1) for s in range(STEPS)]
    fms, ams = [mk[0] for mk in masks], [mk[1] for mk in masks]
    for s in range(STEPS):                                                   # the margins of every step, along the oracle's own trajectory
        p = params if s == 0 else to.train_steps(params, ip, ix, x, labels, idx, L, M_HEADS, fms[:s], P_FEAT, ams[:s], P_ATTN, LR, WD, s)[1]
        _assert_margin(to.model_fwd(p, ip, ix, x, L, M_HEADS, fms[s], P_FEAT, ams[s], P_ATTN)[2])
    ref_losses, ref_params = to.train_steps(params, ip, ix, x, labels, idx, L, M_HEADS, fms, P_FEAT, ams, P_ATTN, LR, WD, STEPS)
    losses = []
    for s in range(STEPS):
        losses.append(train(m, g, tx, tlabels, torch.nn.NLLLoss(), opt, tidx))
        assert teacher.get_engine(m, opt) is eng and eng.step_count == s + 1
    print(f"L={L} losses {losses} reference {ref_losses.tolist()}")
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-3, atol=1e-4)
    fin = _params(m)
    for k, v in ref_params.items():
        print(f"L={L} {k} after {STEPS} steps: max|err| {np.abs(fin[k] - v).max():.3e}")
        np.testing.assert_allclose(fin[k], v, rtol=1e-3, atol=1e-4, err_msg=k)
    assert any(not np.array_equal(fms[0][l], fms[1][l]) for l in range(L))       # the seed streams move with the step count


def test_train_subgraph_batch_equals_train_on_the_same_subgraph():
    """One batch of train_subgraph against train() over CSRGraph.subgraph of the oracle's node set: the same kernels and the same step
    counter (so the same dropout seeds) on the same arrays -- every parameter is bit-equal."""
    import subgraph_oracle as so
    from glnn_amd import teacher
    from glnn_amd.graph import RandomWalkSubgraphLoader
    from glnn_amd.train_and_eval import train, train_subgraph
    from test_subgraph_gpu import N, _model as sub_model, _sym_graph
    ip, ix, g = _sym_graph()
    rs = np.random.RandomState(2)
    d_in, n_cls = 20, 5
    x = _t(rs.randn(N, d_in))
    y = torch.from_numpy(rs.randint(0, n_cls, N).astype(np.int64)).to(DEV)
    idx_train = rs.choice(N, 32, replace=False).astype(np.int64)
    train_mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    train_mask[torch.from_numpy(idx_train).to(DEV)] = True
    crit = torch.nn.NLLLoss()
    m1 = sub_model("GraphTransformer", d_in, n_cls)
    opt1 = torch.optim.Adam(m1.parameters(), lr=0.01, weight_decay=5e-4)
    loader = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 3, shuffle=False, seed=9)
    assert len(loader) == 1
    loss1 = train_subgraph(m1, loader, x, y, crit, opt1)
    assert teacher.get_engine(m1, opt1).step_count == 1 and teacher.get_engine(m1, opt1).kind == "gt"
    m2 = sub_model("GraphTransformer", d_in, n_cls)
    opt2 = torch.optim.Adam(m2.parameters(), lr=0.01, weight_decay=5e-4)
    walks = so.random_walk(ip, ix, idx_train, 3, loader.rng_seed(1, 0))
    nodes = torch.from_numpy(so.first_appearance(walks.reshape(-1))).to(DEV)
    loss2 = train(m2, g.subgraph(nodes), x[nodes], y[nodes], crit, opt2, torch.nonzero(train_mask[nodes]).reshape(-1))
    for (k1, p1), (k2, p2) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(p1, p2), k1
    assert np.isfinite(loss1) and loss1 == pytest.approx(loss2, rel=1e-6)
    before = sub_model("GraphTransformer", d_in, n_cls).state_dict()
    assert any(not torch.equal(before[k], v) for k, v in m1.state_dict().items())          # the step moved the parameters


def test_limits_and_zero_in_degree():
    from glnn_amd import ops
    from glnn_amd._lib import GlnnError
    from glnn_amd.graph import CSRGraph
    from glnn_amd.train_and_eval import train
    loops = CSRGraph(torch.arange(4, dtype=torch.int64, device=DEV), torch.arange(3, dtype=torch.int32, device=DEV), 3)
    for H, D in ((65, 1), (1, 257)):                                         # heads = 65; heads * out_feats = 257
        z, s3 = torch.zeros(3, H * D, device=DEV), torch.zeros(3, H, device=DEV)
        with pytest.raises(GlnnError, match=r"status -2.*heads <= 64 and heads \* out_feats <= 256"):
            ops.gt_attn_fwd(loops.indptr, loops.indices, 3, z, z, z, z, H, D)
        with pytest.raises(GlnnError, match=r"status -2.*heads <= 64 and heads \* out_feats <= 256"):
            ops.gt_attn_bwd(loops, z, z, z, s3, z, H, D)
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


def test_graph_transformer_teacher_then_student_cli(tmp_path):
    common = ["--dataset", "synthetic-cora", "--teacher", "GraphTransformer", "--device", "0", "--max_epoch", "2",
              "--model_config_path", os.path.join(ROOT, "train.conf.yaml")]
    _run("train_teacher.py", common + ["--save_results"], tmp_path)
    base = tmp_path / "outputs" / "transductive" / "synthetic-cora"
    out_t = np.load(base / "GraphTransformer" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    curves = np.load(base / "GraphTransformer" / "seed_0" / "loss_and_score.npz")["arr_0"]
    assert np.isfinite(curves).all()                                           # a finite loss every epoch
    sd = torch.load(base / "GraphTransformer" / "seed_0" / "model.pth", map_location="cpu")
    assert sd["encoder.layers.0.lin_query.weight"].shape[0] == 128 and tuple(sd["encoder.layers.1.lin_skip.bias"].shape) == (7,)
    _run("train_student.py", common + ["--student", "MLP"], tmp_path)
    out_s = np.load(base / "GraphTransformer_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
    np.testing.assert_allclose(np.exp(out_s).sum(1), 1.0, atol=1e-4)
