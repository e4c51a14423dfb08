"""GCNII teacher on the GPU: the fused layer kernel (csrc/gcnii.hip) forward and backward against the fp64 oracle (tests/gcnii_oracle.py) at
every lane layout and padding case of its dispatcher, determinism and tile-order independence, the identity with the APPNP kernels at
lamda = 0, the Model surface and the training step against the oracle fed the library's dropout masks, depth 64, and the command lines
end to end.  Kernel tolerance: rtol = atol = 1e-4 (tests/parity_rules.py); model level: GPRGNN's rule rtol 1e-3, atol 1e-4, or where that
is more 4x the distance of an fp32 CPU stand-in from the fp64 oracle (the rule of tests/test_gat_gpu.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import appnp_oracle as ao
import gcnii_oracle as co
from graphgen import csr_from_edges, random_graph
from parity_rules import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N = 613                       # not a multiple of the 32-row tile: 20 tiles, the last of 5 rows


def _csr_graph(ip, ix):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), len(ip) - 1)


def _graph_csr(n=N, seed=10):
    """Non-symmetric, multi-edges, isolated rows, one destination of 700 in-edges (a whole-workgroup row and its fold) and one of about
    100 (a one-wave row of two 64-entry chunks) and, for the passes over the transposed CSR, a source of 700 out-edges, one of about 100
    and one without any.  The added edges end in rows that already have in-edges: the isolated rows stay isolated."""
    ip, ix = random_graph(n, 6, seed=seed, power=0.6, isolated=9, hub=700)
    dst, src = np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)
    rs = np.random.RandomState(seed + 1000)
    open_rows = np.flatnonzero(np.diff(ip) > 0)
    hub_src, mid_src = (int(v) for v in rs.choice(n, 2, replace=False))
    mid_dst = int(open_rows[np.argmin(np.diff(ip)[open_rows])])
    src = np.concatenate([src, np.full(700, hub_src), np.full(100, mid_src), np.flatnonzero(np.bincount(src, minlength=n) > 0)[:90]])
    dst = np.concatenate([dst, rs.choice(open_rows, 700), rs.choice(open_rows, 100), np.full(90, mid_dst)])
    return csr_from_edges(src, dst, n)


def _graph():
    ip, ix = _graph_csr()
    return ip, ix, _csr_graph(ip, ix)


@pytest.fixture(scope="module")
def graph():
    return _graph()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _nan_buf(n, d):
    """A NaN-filled [n, round4(d)] buffer and its [n, d] view: an unwritten element or padding column shows."""
    buf = torch.full((n, (d + 3) // 4 * 4), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[:, :d]


def _nan_feat(a):
    """A device copy of `a` whose padding columns are NaN: whatever reads one shows."""
    buf, view = _nan_buf(*a.shape)
    view.copy_(_t(a))
    return view


def _clean(buf, d):
    assert not torch.isnan(buf).any()
    if buf.shape[1] > d:
        assert bool((buf[:, d:] == 0).all())


def test_graph_has_the_rows_the_kernel_branches_on(graph):
    ip, ix, _ = graph
    deg, out_deg = np.diff(ip), np.bincount(ix, minlength=len(ip) - 1)
    assert len(deg) == N and N % 32 != 0
    assert deg.max() >= 700 and (deg == 0).sum() >= 9 and ((deg > 64) & (deg <= 128)).any()
    assert out_deg.max() > 128 and ((out_deg > 64) & (out_deg <= 128)).any() and (out_deg == 0).any()
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(len(deg)), deg)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                                   # a multi-edge
    assert not np.array_equal(np.sort(deg), np.sort(out_deg))                           # non-symmetric
    dn, sn = ao.degree_norms(ip, ix, N)
    assert not np.allclose(dn, sn)                                                      # in-degree on both sides would be another operator


# ---------------------------------------------------------------------------------------------------------------- the layer kernel
# The dispatcher of csrc/gcnii.hip: kpad = 8 ceil(d / 8), LPR = 16 (kpad <= 64) | 32 (kpad <= 128) | 64 (kpad <= 256).  Per LPR: a width
# with d % 8 == 0 (no padding), one with d % 8 == 4 (kpad = d + 4: a zero k-half-group), one with d % 4 != 0 (ld > d: zeroed padding
# columns) -- 8, 64 | 12 | 1, 30 -- 128 | 100 | 65 -- 256 | 132 | 130, 250 -- and the last width of each LPR (64, 128, 256).
WIDTHS = (8, 12, 64, 100, 128, 256, 1, 30, 65, 130, 132, 250)
ALPHA, BETA, P = 0.1, 0.4, 0.5


def _layer_inputs(d, seed=0):
    rs = np.random.RandomState(d * 7 + seed)
    x = rs.standard_normal((N, d)).astype(np.float32)
    h0 = rs.standard_normal((N, d)).astype(np.float32)
    w = (rs.uniform(-1, 1, (d, d)) / math.sqrt(d)).astype(np.float32)
    return rs, x, h0, w


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_layer_forward_matches_the_oracle(graph, d, train, prescaled):
    """prescaled False: unscaled rows in (x_norm = src_norm) and out (out_norm None).  True: rows pre-scaled by src_norm in (x_norm None)
    and out (out_norm = src_norm).  train: the source-keyed dropout, its masks replayed through ops.dropout_mask, and s_out."""
    from glnn_amd import ops
    ip, ix, g = graph
    _, x, h0, w = _layer_inputs(d)
    in_norm, out_norm = g.degree_norms()
    _, sn = ao.degree_norms(ip, ix, N)
    p, seed = (P, 1000 + d) if train else (0.0, 0)
    mask = ops.dropout_mask(N, d, p, seed, DEV).cpu().numpy() if train else None
    if train:
        assert 0.3 < mask.mean() < 0.7
    s_ref, _, h_ref = co.layer(ip, ix, x, h0, w, ALPHA, BETA, mask, p)
    out_buf, out = _nan_buf(N, d)
    s_buf, s_out = _nan_buf(N, d) if train else (None, None)
    xin = _nan_feat((x * sn[:, None]).astype(np.float32)) if prescaled else _nan_feat(x)
    ops.gcnii_layer(g.indptr, g.indices, g.num_edges(), xin, _nan_feat(h0), _t(w), ALPHA, BETA, in_norm, x_norm=None if prescaled else out_norm,
                    out_norm=out_norm if prescaled else None, drop_p=p, drop_seed=seed, s_out=s_out, out=out)
    want = h_ref * sn[:, None] if prescaled else h_ref
    got = out.cpu().numpy()
    print(f"d={d} train={train} prescaled={prescaled}: max|err| {np.abs(got - want).max():.3e} max|ref| {np.abs(want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=TOL, atol=TOL)
    _clean(out_buf, d)
    assert (h_ref > 0).any() and (h_ref == 0).any()                                     # the ReLU acts
    if train:
        np.testing.assert_allclose(s_out.cpu().numpy(), s_ref, rtol=TOL, atol=TOL)
        _clean(s_buf, d)


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_layer_backward_matches_the_oracle(graph, d, plain):
    """Three chained launches as gcnii_bwd issues them.  1: `first`, the plain or the gather form (unscaled rows in, x_norm = dst_norm),
    dz_scale = beta, rows stored pre-scaled by dst_norm.  2: not first, gathers call 1's pre-scaled rows (x_norm None), stores unscaled
    rows.  3: the launch without a product, dL/dH_0.  The saved H are INPUTS of the launches and of the oracle."""
    from glnn_amd import ops
    ip, ix, g = graph
    rs, g1, _, w1 = _layer_inputs(d, seed=1)
    w2 = (rs.uniform(-1, 1, (d, d)) / math.sqrt(d)).astype(np.float32)
    h1, h2 = (np.maximum(rs.standard_normal((N, d)), 0.0).astype(np.float32) for _ in range(2))
    in_norm, out_norm = g.degree_norms()
    dn, _ = ao.degree_norms(ip, ix, N)
    tg, nnz = g.transposed(False), g.num_edges()
    seeds = [77 + d, 78 + d, 79 + d]
    m1, m2, m3 = (ops.dropout_mask(N, d, P, s, DEV).cpu().numpy() for s in seeds)
    beta2 = 0.25
    dz1_ref, ds1_ref = co.layer_bwd(ip, ix, g1, h1, w1, ALPHA, BETA, m1, P, plain=plain)
    dz2_ref, ds2_ref = co.layer_bwd(ip, ix, ds1_ref, h2, w2, ALPHA, beta2, m2, P)
    acc1_ref = ALPHA * ds1_ref
    acc2_ref = acc1_ref + ALPHA * ds2_ref
    dh0_ref = (1 - ALPHA) * co.prop_t(ip, ix, ds2_ref) * (m3 / (1 - P)) + acc2_ref
    (dz_buf, dz), (ds1_buf, ds1), (ds2_buf, ds2), (acc_buf, acc) = (_nan_buf(N, d) for _ in range(4))

    def check(tag, got, ref):
        got = got.cpu().numpy()
        print(f"d={d} plain={plain} {tag}: max|err| {np.abs(got - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
        np.testing.assert_allclose(got, ref, rtol=TOL, atol=TOL, err_msg=tag)

    r = ops.gcnii_layer_bwd(tg.indptr, tg.indices, nnz, _nan_feat(g1), _nan_feat(h1), _t(w1.T), ALPHA, BETA, dz, acc, True,
                            row_norm=out_norm, x_norm=in_norm, out_norm=in_norm, plain=plain, drop_p=P, drop_seed=seeds[0], dz_scale=BETA,
                            ds_out=ds1)
    assert r is ds1
    check("dz 1", dz, BETA * dz1_ref)
    check("ds 1", ds1, ds1_ref * dn[:, None])
    check("acc 1", acc, acc1_ref)
    for buf in (dz_buf, ds1_buf, acc_buf):
        _clean(buf, d)
    dz_buf.fill_(float("nan"))
    ops.gcnii_layer_bwd(tg.indptr, tg.indices, nnz, ds1, _nan_feat(h2), _t(w2.T), ALPHA, beta2, dz, acc, False, row_norm=out_norm,
                        drop_p=P, drop_seed=seeds[1], ds_out=ds2)
    check("dz 2", dz, dz2_ref)
    check("ds 2", ds2, ds2_ref)
    check("acc 2", acc, acc2_ref)
    for buf in (dz_buf, ds2_buf, acc_buf):
        _clean(buf, d)
    dz_buf.fill_(float("nan"))
    r = ops.gcnii_layer_bwd(tg.indptr, tg.indices, nnz, ds2, None, None, ALPHA, 0.0, dz, acc, False, row_norm=out_norm, x_norm=in_norm,
                            drop_p=P, drop_seed=seeds[2])
    assert r is dz
    check("dh0", dz, dh0_ref)
    check("acc kept", acc, acc2_ref)
    _clean(dz_buf, d)


@pytest.mark.parametrize("d", [12, 100, 250])
def test_two_runs_and_a_permuted_tile_order_give_the_same_bits(graph, d):
    from glnn_amd import ops
    ip, ix, g = graph
    rs, x, h0, w = _layer_inputs(d, seed=2)
    in_norm, out_norm = g.degree_norms()
    tiles = (N + 31) // 32
    order = torch.from_numpy(np.random.RandomState(d).permutation(tiles).astype(np.int32)).to(DEV)
    heavy = ops.fused_tile_order(g.indptr, N)
    assert not torch.equal(order, torch.arange(tiles, dtype=torch.int32, device=DEV))
    tx, th0, tw = _t(x), _t(h0), _t(w)

    def fwd(tile_order):
        s = ops.feat_empty(N, d, DEV)
        out = ops.gcnii_layer(g.indptr, g.indices, g.num_edges(), tx, th0, tw, ALPHA, BETA, in_norm, x_norm=out_norm, drop_p=P, drop_seed=5,
                              s_out=s, tile_order=tile_order)
        return out, s

    a, b, c, e = fwd(None), fwd(None), fwd(order), fwd(heavy)
    for other in (b, c, e):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    tg = g.transposed(False)
    th, twt = _t(np.maximum(rs.standard_normal((N, d)), 0.0)), _t(w.T)

    def bwd(tile_order, plain):
        dz, acc = ops.feat_empty(N, d, DEV), ops.feat_empty(N, d, DEV)
        ds = ops.gcnii_layer_bwd(tg.indptr, tg.indices, g.num_edges(), tx, th, twt, ALPHA, BETA, dz, acc, True, row_norm=out_norm,
                                 x_norm=in_norm, plain=plain, drop_p=P, drop_seed=6, dz_scale=BETA, tile_order=tile_order)
        return dz, ds, acc

    for plain in (False, True):
        a, b, c = bwd(None, plain), bwd(None, plain), bwd(order, plain)
        for other in (b, c):
            assert all(torch.equal(u, v) for u, v in zip(a, other))


@pytest.mark.parametrize("L,alpha", [(1, 0.5), (10, 0.1)])
def test_lamda_zero_stack_is_the_appnp_kernels(graph, L, alpha):
    """beta_l = log(0 / l + 1) = 0 and H_0 >= 0: every ReLU is the identity and the stack is APPNP's propagation, on the device too."""
    from glnn_amd.autograd import appnp_fwd, gcnii_betas, gcnii_fwd
    ip, ix, g = graph
    d = 47
    rs = np.random.RandomState(L)
    h0 = np.maximum(rs.standard_normal((N, d)), 0.0).astype(np.float32)
    ws = [_t(rs.standard_normal((d, d))) for _ in range(L)]
    betas = gcnii_betas(L, 0.0)
    assert betas == [0.0] * L
    hs, ss = gcnii_fwd(g, _t(h0), ws, alpha, betas)
    assert ss is None and len(hs) == L
    out = hs[-1].cpu().numpy()
    np.testing.assert_allclose(out, appnp_fwd(g, _t(h0), L, alpha, 0.0, 0).cpu().numpy(), rtol=TOL, atol=TOL)
    np.testing.assert_allclose(out, ao.propagate(ip, ix, h0, L, alpha, None, 0), rtol=TOL, atol=TOL)


def test_ops_argument_checks(graph):
    from glnn_amd import ops
    _, _, g = graph
    in_norm, out_norm = g.degree_norms()
    x = torch.zeros(N, 8, device=DEV)
    w = torch.zeros(8, 8, device=DEV)
    with pytest.raises(NotImplementedError, match="GCNII"):
        ops.gcnii_layer(g.indptr, g.indices, g.num_edges(), torch.zeros(N, 260, device=DEV), torch.zeros(N, 260, device=DEV),
                        torch.zeros(260, 260, device=DEV), 0.1, 0.4, in_norm, x_norm=out_norm)
    with pytest.raises(ValueError):
        ops.gcnii_layer(g.indptr, g.indices, g.num_edges(), x, x, torch.zeros(8, 4, device=DEV), 0.1, 0.4, in_norm, x_norm=out_norm)
    with pytest.raises(ValueError):
        ops.gcnii_layer(g.indptr, g.indices, g.num_edges(), x, x, w, 0.1, 0.4, in_norm, x_norm=out_norm,
                        tile_order=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):                                                     # the dH_0 launch writes dz_out alone
        ops.gcnii_layer_bwd(g.indptr, g.indices, g.num_edges(), x, None, None, 0.1, 0.0, ops.feat_empty(N, 8, DEV), ops.feat_empty(N, 8, DEV),
                            True, row_norm=out_norm)


# ---------------------------------------------------------------------------------------------------------------- model, training step
LR, WD = 0.01, 0.01
N_MODEL, DIMS, L_MODEL = 200, (20, 16, 5), 3


@pytest.fixture(scope="module")
def small_graph():
    ip, ix = random_graph(N_MODEL, 5, seed=21, power=0.6, isolated=4, hub=150)
    return ip, ix, _csr_graph(ip, ix)


def _model(L=L_MODEL, dims=DIMS, dropout=0.0, seed=0, **extra):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    return Model(dict(model_name="GCNII", num_layers=L, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[2], dropout_ratio=dropout,
                      norm_type="none", device=DEV, **extra))


def _data(n, dims, seed):
    """Features of scale 10: the network is positively homogeneous up to its biases, so the pre-activations scale along and the seed
    search below finds inputs that keep all 12,800 of them (per step) further than 1e-4 from 0 within a few dozen seeds."""
    rs = np.random.RandomState(seed)
    x = (10.0 * rs.standard_normal((n, dims[0]))).astype(np.float32)
    labels = rs.randint(0, dims[2], n).astype(np.int64)
    idx = np.sort(rs.choice(n, n // 3, replace=False)).astype(np.int64)
    return x, labels, idx


def _np_params(m):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


def _step_masks(eng, n, dims, L, p, steps):
    """The library's keep-masks of every dropout site of steps 1..steps (site 0 is as wide as the features)."""
    from glnn_amd import ops
    if p == 0:
        return None
    return [[ops.dropout_mask(n, dims[0] if s == 0 else dims[1], p, eng._gcnii_seed(s, step=t), DEV).cpu().numpy() for s in range(L + 2)]
            for t in range(1, steps + 1)]


def _standin_grads_fp32(params, ip, ix, x, labels, idx, L, alpha, lamda, masks, p):
    """The first step's gradients in fp32 on the CPU (torch autograd on a dense restatement, fp32 throughout): its distance from the fp64
    oracle is what fp32 arithmetic costs on these inputs."""
    n = len(ip) - 1
    f32 = torch.float32
    t = {a: torch.tensor(b, dtype=f32, requires_grad=True) for a, b in params.items()}
    dn, sn = ao.degree_norms(ip, ix, n)
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)), 1.0)
    pm = torch.tensor(dn.astype(np.float32)[:, None] * dense.astype(np.float32) * sn.astype(np.float32)[None, :])
    keep = [torch.tensor(1.0, dtype=f32)] * (L + 2) if masks is None else [torch.tensor(m.astype(np.float32) / np.float32(1 - p)) for m in masks]
    h0 = torch.relu((torch.tensor(x, dtype=f32) * keep[0]) @ t[co.FC_IN_W].T + t[co.FC_IN_B])
    h = h0
    for l in range(1, L + 1):
        beta = math.log(lamda / l + 1)
        s = (1 - alpha) * (pm @ (h * keep[l])) + alpha * h0
        h = torch.relu((1 - beta) * s + beta * (s @ t[co.conv_w(l)].T))
    out = (h * keep[L + 1]) @ t[co.FC_OUT_W].T + t[co.FC_OUT_B]
    torch.nn.functional.nll_loss(out[idx].log_softmax(1), torch.tensor(labels[idx])).backward()
    return {a: v.grad.numpy().astype(np.float64) for a, v in t.items()}


def _searched_problem(m, eng, ip, ix, L, dims, p, steps, alpha=0.1, lamda=0.5):
    """Inputs chosen by a seed search on the CPU: the first data seed at which the oracle's smallest |pre-activation| (fc_in's output and
    every Z_l, every step) exceeds the forward parity bar, so that no ReLU mask of the device can differ from the oracle's."""
    n = len(ip) - 1
    params = _np_params(m)
    masks = _step_masks(eng, n, dims, L, p, steps)
    for seed in range(1, 200):
        x, labels, idx = _data(n, dims, seed)
        ref = co.train_steps(params, ip, ix, x, labels, idx, L, alpha, lamda, masks, p, LR, WD, steps)
        if ref[4] > TOL:
            print(f"data seed {seed}: smallest |pre-activation| {ref[4]:.3e}")
            return params, masks, x, labels, idx, ref
    raise AssertionError("no data seed keeps every pre-activation away from 0")


def _check_grad(name, got, ref, standin):
    e32 = np.abs(standin - ref)
    print(f"  grad {name}: max|err| {np.abs(got - ref).max():.3e} max|ref| {np.abs(ref).max():.3e} fp32 stand-in max|err| {e32.max():.3e}")
    tol = np.maximum(1e-4 + 1e-3 * np.abs(ref), 4.0 * e32.max())
    assert not (np.abs(got - ref) > tol).any(), f"grad {name}: max|err| {np.abs(got - ref).max():.3e}, fp32 stand-in {e32.max():.3e}"


@pytest.mark.parametrize("dropout,steps", [(0.0, 1), (0.5, 1), (0.5, 3)])
def test_training_steps_match_the_oracle(small_graph, dropout, steps):
    """train() -> TeacherEngine.step_gcnii against the oracle's steps fed the library's dropout masks: every loss, the first step's
    gradients, and after the last step the parameters and both Adam moments."""
    from glnn_amd import teacher
    from glnn_amd.train_and_eval import train
    ip, ix, g = small_graph
    L, dims = L_MODEL, DIMS
    m = _model(dropout=dropout)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    eng = teacher.get_engine(m, opt)
    assert eng.kind == "gcnii" and eng.p == dropout
    params, masks, x, labels, idx, (ref_losses, ref_grads, ref_params, ref_state, min_pre) = _searched_problem(m, eng, ip, ix, L, dims, dropout,
                                                                                                               steps)
    assert min_pre > TOL
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    named = dict(m.named_parameters())
    assert set(named) == set(ref_grads) and len(named) == L + 4
    standin = _standin_grads_fp32(params, ip, ix, x, labels, idx, L, 0.1, 0.5, None if masks is None else masks[0], dropout)
    for s in range(steps):
        loss = train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
        print(f"p={dropout} step {s + 1}: loss {loss:.6f} oracle {ref_losses[s]:.6f}")
        np.testing.assert_allclose(loss, ref_losses[s], rtol=1e-4)
        if s == 0:
            for name, prm in named.items():
                _check_grad(name, eng.grad(prm).cpu().numpy().astype(np.float64), ref_grads[name], standin[name])
    assert teacher.get_engine(m, opt) is eng and eng.step_count == steps
    for name, prm in named.items():
        np.testing.assert_allclose(prm.detach().cpu().numpy(), ref_params[name], rtol=1e-3, atol=1e-4, err_msg=name)
        st = opt.state[prm]
        assert float(st["step"]) == float(steps)
        np.testing.assert_allclose(st["exp_avg"].cpu().numpy(), ref_state[name][0], rtol=1e-3, atol=1e-4, err_msg=f"exp_avg {name}")
        np.testing.assert_allclose(st["exp_avg_sq"].cpu().numpy(), ref_state[name][1], rtol=1e-3, atol=1e-4, err_msg=f"exp_avg_sq {name}")


def test_eval_forward_and_inference_match_the_oracle(small_graph):
    ip, ix, g = small_graph
    m = _model(dropout=0.5, gcnii_alpha=0.2, gcnii_lamda=1.5).eval()
    x, _, _ = _data(N_MODEL, DIMS, 3)
    ref_logits, cache = co.model_forward(_np_params(m), ip, ix, x, L_MODEL, 0.2, 1.5)
    h_list, logits = m.forward_fitnet(g, _t(x))
    assert len(h_list) == L_MODEL and not logits.requires_grad
    for h, ref in zip(h_list, cache["hs"]):
        np.testing.assert_allclose(h.cpu().numpy(), ref, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(m(g, _t(x)).cpu().numpy(), ref_logits, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(m.inference(g, _t(x)).cpu().numpy(), ref_logits, rtol=TOL, atol=TOL)
    with pytest.raises(NotImplementedError, match="GCNII"):
        m.inference(g, _t(x), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="bipartite"):
        m([g], _t(x))


def test_autograd_path_matches_the_engine_gradients(small_graph):
    """Model.forward in training mode differentiates through GcniiStackFn: its gradients equal step_gcnii's (dropout-free), and with
    dropout it runs and gives every parameter a finite gradient."""
    from glnn_amd import autograd, teacher
    from glnn_amd.train_and_eval import train
    ip, ix, g = small_graph
    m = _model(seed=2)
    x, labels, idx = _data(N_MODEL, DIMS, 5)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    m.train()
    c0 = autograd._drop_counter[0]
    h_list, logits = m.forward_fitnet(g, tx)
    assert logits.requires_grad and len(h_list) == L_MODEL and not h_list[0].requires_grad
    assert autograd._drop_counter[0] == c0 + 1                              # dropout-free: H_0's ReLU tail alone
    torch.nn.NLLLoss()(logits.log_softmax(dim=1)[ti], tl[ti]).backward()
    auto = {name: p.grad.detach().clone() for name, p in m.named_parameters()}
    assert all(v is not None for v in auto.values())
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
    eng = teacher.get_engine(m, opt)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(eng.grad(p).cpu().numpy(), auto[name].cpu().numpy(), rtol=TOL, atol=TOL, err_msg=name)
    md = _model(dropout=0.5, seed=2).train()
    c0 = autograd._drop_counter[0]
    out = md(g, tx)
    assert autograd._drop_counter[0] == c0 + 4                              # the input's, H_0's tail, the stack's one draw, fc_out's
    torch.nn.NLLLoss()(out.log_softmax(dim=1)[ti], tl[ti]).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()) for p in md.parameters())


def test_one_step_twice_from_the_same_state_gives_the_same_bits(small_graph):
    from glnn_amd.train_and_eval import train
    ip, ix, g = small_graph
    x, labels, idx = _data(N_MODEL, DIMS, 7)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    states = []
    for _ in range(2):
        m = _model(dropout=0.5, seed=4)
        opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
        loss = train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
        states.append((loss, [p.detach().clone() for p in m.parameters()]))
    assert states[0][0] == states[1][0]
    assert all(torch.equal(a, b) for a, b in zip(states[0][1], states[1][1]))


def test_depth_64(small_graph):
    """L = 64, hidden 64 (the cora configuration's depth and width): the eval forward against the oracle, then one step with dropout --
    66 dropout sites, 128 saved activations, 68 tensors in the Adam table -- whose loss and classifier gradients are the oracle's and
    which moves every parameter."""
    from glnn_amd import teacher
    from glnn_amd.train_and_eval import train
    ip, ix, g = small_graph
    L, dims, p = 64, (20, 64, 5), 0.5
    m = _model(L=L, dims=dims, dropout=p, seed=6)
    x, labels, idx = _data(N_MODEL, dims, 9)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    params = _np_params(m)
    m.eval()
    ref_logits, _ = co.model_forward(params, ip, ix, x, L, 0.1, 0.5)
    np.testing.assert_allclose(m(g, tx).cpu().numpy(), ref_logits, rtol=TOL, atol=TOL)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    eng = teacher.get_engine(m, opt)
    masks = _step_masks(eng, N_MODEL, dims, L, p, 1)
    assert len(masks[0]) == 66 and len({eng._gcnii_seed(s, step=1) for s in range(L + 2)}) == 66
    ref_loss, ref_grads, _ = co.loss_and_grads(params, ip, ix, x, labels, idx, L, 0.1, 0.5, masks[0], p)
    before = [q.detach().clone() for q in m.parameters()]
    loss = train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
    print(f"L=64: loss {loss:.6f} oracle {ref_loss:.6f}")
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    for name in (co.FC_OUT_W, co.FC_OUT_B):                    # the gradients in front of the loss: no ReLU mask behind them
        got = eng.grad(dict(m.named_parameters())[name]).cpu().numpy()
        np.testing.assert_allclose(got, ref_grads[name], rtol=1e-3, atol=1e-4, err_msg=name)
    assert len(before) == L + 4 == 68 and eng.step_count == 1
    for q, b in zip(m.parameters(), before):
        assert torch.isfinite(q).all() and not torch.equal(q, b) and float(opt.state[q]["step"]) == 1.0


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_gcnii_teacher_then_student_cli(tmp_path):
    common = ["--dataset", "synthetic-cora", "--teacher", "GCNII", "--device", "0", "--max_epoch", "3"]
    _run("train_teacher.py", common + ["--save_results"], tmp_path)
    base = tmp_path / "outputs" / "transductive" / "synthetic-cora"
    out_t = np.load(base / "GCNII" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    curves = np.load(base / "GCNII" / "seed_0" / "loss_and_score.npz")["arr_0"]
    assert np.isfinite(curves).all()                                           # a finite loss every epoch
    sd = torch.load(base / "GCNII" / "seed_0" / "model.pth", map_location="cpu")
    assert sd["encoder.layers.63.weight"].shape == (64, 64) and len(sd) == 64 + 4      # the cora section: 64 layers of width 64
    _run("train_student.py", common + ["--student", "MLP"], tmp_path)
    out_s = np.load(base / "GCNII_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
