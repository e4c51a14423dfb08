"""DAGNN teacher on the GPU: the gate, gate-backward and fold kernels (csrc/dagnn.hip) with the propagation between them against the fp64 oracle (tests/dagnn_oracle.py), the
identities with the GPR-GNN kernels under a zero gate weight, determinism, the device-side gate parameters, the Model surface and the
training step against the oracle fed the library's dropout masks, the refusals, and the command lines end to end.  Tolerances are those of
tests/test_gpr_gpu.py; the gate's gradients, which sum (K + 1) n d terms, are allowed 4x the error of an fp32 CPU stand-in of the same sums
where that exceeds the bound (the rule of tests/test_gat_gpu.py; docs/DAGNN_SEMANTICS.md, Tolerances)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import appnp_oracle as ao
import dagnn_oracle as do
from graphgen import csr_from_edges, random_graph, segment_reduce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _csr_graph(ip, ix):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), len(ip) - 1)


def _graph(n=600, seed=3):
    """The graph of tests/test_gpr_gpu.py: non-symmetric, isolated rows, a multi-edge, one destination row far above the long-row threshold
    (128) and, for the pass over the transposed CSR, a hub source of 700 out-edges (a whole-workgroup row) and one of about 100."""
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
    assert deg.max() > 128 and (deg == 0).sum() >= 9 and ((deg > 0) & (deg <= 128)).any()
    assert out_deg.max() > 128 and ((out_deg > 64) & (out_deg <= 128)).any() and (out_deg == 0).any()
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(len(deg)), deg)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                                   # a multi-edge
    assert not np.array_equal(np.sort(deg), np.sort(out_deg))                           # non-symmetric


# ---------------------------------------------------------------------------------------------------------------- propagation
def _standin_gate_grads_fp32(ip, ix, dy, h0, w, b, k):
    """The gate's gradients dw = sum_j H_j^T q_j, db = sum q in fp32 numpy on the CPU (fp32 norms, products, gates and sums throughout): its
    distance from the fp64 oracle is what fp32 arithmetic costs on these inputs."""
    n = len(ip) - 1
    f = np.float32
    dn, sn = (v.astype(f) for v in ao.degree_norms(ip, ix, n))
    dst, src = np.repeat(np.arange(n), np.diff(ip)), ix.astype(np.int64)
    h, dy, w, b = h0.astype(f), dy.astype(f), w.astype(f), f(b)
    dw, db = np.zeros(len(w), f), f(0.0)
    for j in range(k + 1):
        if j:
            h = dn[:, None] * segment_reduce(np.add, sn[src, None] * h[src], dst, n, f(0.0))
        s = f(1.0) / (f(1.0) + np.exp(-(h @ w + b), dtype=f))
        q = np.sum(dy * h, axis=1, dtype=f) * s * (f(1.0) - s)
        dw = dw + np.sum(h * q[:, None], axis=0, dtype=f)
        db = db + np.sum(q, dtype=f)
    return dw.astype(np.float64), float(db)


def _check_gate_grads(tag, got_w, got_b, ref_w, ref_b, standin):
    got, ref, st = np.append(got_w, got_b), np.append(ref_w, ref_b), np.append(*standin)
    e32 = np.abs(st - ref)
    print(f"{tag} dw/db: max|err| {np.abs(got - ref).max():.3e} max|ref| {np.abs(ref).max():.3e} fp32 stand-in max|err| {e32.max():.3e}")
    tol = np.maximum(1e-4 + 1e-4 * np.abs(ref), 4.0 * e32)
    assert not (np.abs(got - ref) > tol).any(), f"{tag} dw/db: {got} vs {ref} (fp32 stand-in err {e32})"


def _inputs(n, d, k, seed=0):
    rs = np.random.RandomState(d * 100 + k + seed)
    h0 = rs.standard_normal((n, d)).astype(np.float32)
    dy = rs.standard_normal((n, d)).astype(np.float32)
    w = (rs.standard_normal(d) / np.sqrt(d)).astype(np.float32)                        # <row, w> of order 1: gates spread over (0, 1)
    return h0, dy, w, np.float32(0.3)


def _check_propagation(ip, ix, g, d, k, seed=0):
    from glnn_amd.autograd import dagnn_bwd, dagnn_fwd
    n = len(ip) - 1
    h0, dy, w, b = _inputs(n, d, k, seed)
    tw, tb, tag = _t(w).reshape(1, d), _t([b]), f"n={n} d={d} k={k}"
    ref = do.propagate(ip, ix, h0, w, b, k)
    out_eval = dagnn_fwd(g, _t(h0), tw, tb, k)                                          # eval: two ping-pong buffers, nothing kept
    out, (stack, score) = dagnn_fwd(g, _t(h0), tw, tb, k, keep=True)                    # training: the stack and the gates
    print(f"{tag} forward: max|err| {np.abs(out.cpu().numpy() - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, out_eval)                                                   # the same arithmetic whether or not it keeps
    hs = do.hops(ip, ix, h0, k)
    assert stack.shape == ((k + 1) * n, d) and score.shape == ((k + 1) * n,)
    np.testing.assert_allclose(stack.cpu().numpy(), np.concatenate(hs), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(score.cpu().numpy(), np.concatenate(do.gates(hs, w, b)), rtol=1e-4, atol=1e-4)
    dh0, dw, db = dagnn_bwd(g, _t(dy), (stack, score), tw, k)
    rdh0, rdw, rdb = do.propagate_bwd(ip, ix, dy, h0, w, b, k)
    print(f"{tag} backward: max|err| {np.abs(dh0.cpu().numpy() - rdh0).max():.3e} max|ref| {np.abs(rdh0).max():.3e}")
    np.testing.assert_allclose(dh0.cpu().numpy(), rdh0, rtol=1e-4, atol=1e-4)
    assert dw.shape == (d,) and db.shape == (1,)
    _check_gate_grads(tag, dw.cpu().numpy().astype(np.float64), float(db), rdw, rdb, _standin_gate_grads_fp32(ip, ix, dy, h0, w, b, k))
    return out, dh0, dw, db


# the smallest d of every LPR instantiation the launcher can pick (LPR = pow2 >= ceil(d / 4): 1, 2, 4, 8, 16, 32, 64), then a width
# inside a lane group's last float4 (47) and the full 256-column row; k = 0 is the gate alone, without a propagation
WIDTHS = (1, 5, 9, 17, 33, 65, 129, 47, 256)


@pytest.mark.parametrize("k", [0, 1, 2, 10])
@pytest.mark.parametrize("d", WIDTHS)
def test_forward_backward_and_fold_match_the_oracle(graph, d, k):
    ip, ix, g = graph
    _check_propagation(ip, ix, g, d, k)


def test_nan_filled_buffers_and_padding_columns(graph):
    """The row-local launches over buffers pre-filled with NaN, the inputs' padding columns included: nothing reads a padding column, and
    every padding column [d, ld) of a row they write comes out zero."""
    from glnn_amd import ops
    ip, ix, g = graph
    n, d, k, ld = len(ip) - 1, 5, 2, 8
    h0, dy, w, b = _inputs(n, d, k)
    tw, tb = _t(w), _t([b])
    nan = lambda rows: torch.full((rows, ld), float("nan"), dtype=torch.float32, device=DEV)
    hs = do.hops(ip, ix, h0, k)
    stack, gy, acc, score = nan((k + 1) * n), nan(n), nan(n), torch.full(((k + 1) * n,), float("nan"), device=DEV)
    stack[:, :d] = _t(np.concatenate(hs))
    gy[:, :d] = _t(dy)
    for j in range(k + 1):
        ops.dagnn_gate(stack[j * n:(j + 1) * n, :d], j, tw, tb, acc[:, :d], score)
    np.testing.assert_allclose(acc[:, :d].cpu().numpy(), do.propagate(ip, ix, h0, w, b, k), rtol=1e-4, atol=1e-4)
    assert not torch.isnan(acc).any() and not torch.isnan(score).any() and bool((acc[:, d:] == 0).all())
    q, out = torch.full(((k + 1) * n,), float("nan"), device=DEV), nan(n)
    ops.dagnn_gate_bwd(gy[:, :d], stack[k * n:, :d], k, score, tw, None, out[:, :d], q)
    ss = do.gates(hs, w, b)
    qk = (dy * hs[k]).sum(1) * ss[k] * (1 - ss[k])
    np.testing.assert_allclose(out[:, :d].cpu().numpy(), ss[k][:, None] * dy + qk[:, None] * w[None, :], rtol=1e-4, atol=1e-4)
    assert not torch.isnan(out).any() and bool((out[:, d:] == 0).all())
    t = nan(n)
    t[:, :d] = 1.0
    ops.dagnn_gate_bwd(gy[:, :d], stack[:n, :d], 0, score, tw, t[:, :d], t[:, :d], q)     # in place on t, k = 0
    q0 = (dy * hs[0]).sum(1) * ss[0] * (1 - ss[0])
    np.testing.assert_allclose(t[:, :d].cpu().numpy(), ss[0][:, None] * dy + q0[:, None] * w[None, :] + 1.0, rtol=1e-4, atol=1e-4)
    assert not torch.isnan(t).any() and bool((t[:, d:] == 0).all()) and not torch.isnan(q[:n]).any() and not torch.isnan(q[k * n:]).any()
    q[n:k * n] = 0.0
    dw, db = ops.dagnn_fold(stack[:, :d], q)                                            # (the stack's padding is NaN: the fold masks it)
    ref_q = np.concatenate([q0, np.zeros((k - 1) * n), qk])
    np.testing.assert_allclose(dw.cpu().numpy(), np.concatenate(hs).T @ ref_q, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(db.item(), ref_q.sum(), rtol=1e-3, atol=1e-3)


def test_rows_wider_than_256_are_refused_with_nothing_written():
    from glnn_amd import _lib, ops
    n, d = 64, 257
    x = torch.zeros(n, 260, device=DEV)[:, :d]
    acc = torch.full((n, 260), 7.0, device=DEV)
    w, b = torch.zeros(d, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(NotImplementedError, match="256"):
        ops.dagnn_gate(x, 0, w, b, acc[:, :d])
    with pytest.raises(NotImplementedError, match="256"):
        ops.dagnn_fold(x, torch.zeros(n, device=DEV))
    p = lambda t: t.data_ptr()
    rc = _lib.lib().glnn_dagnn_gate_f32(p(x), 260, n, d, p(w), p(b), 0, p(acc), 260, None, None)
    assert rc == -2 and b"256" in _lib.lib().glnn_last_error()                          # GLNN_ERR_UNSUPPORTED, nothing launched
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- the GPR identities
@pytest.mark.parametrize("b", [0.0, 0.7])
@pytest.mark.parametrize("k", [1, 10])
def test_a_zero_gate_weight_gives_the_gpr_kernels_with_a_constant_gamma(graph, k, b):
    """w = 0: every gate is sigmoid(b) (0.5 at b = 0), so the new kernels compute sigmoid(b) sum_j P^j h0 -- what the GPR-GNN kernels, which
    tests/test_gpr_gpu.py pins, compute with gamma identically sigmoid(b) -- and dh0 is gpr_bwd's with that gamma."""
    from glnn_amd.autograd import dagnn_bwd, dagnn_fwd, gpr_bwd, gpr_fwd
    ip, ix, g = graph
    n, d = len(ip) - 1, 47
    rs = np.random.RandomState(k)
    h0, dy = _t(rs.standard_normal((n, d))), _t(rs.standard_normal((n, d)))
    tw, tb = torch.zeros(1, d, device=DEV), _t([b])
    gamma = _t(np.full(k + 1, do.sigmoid(b)))
    out, kept = dagnn_fwd(g, h0, tw, tb, k, keep=True)
    np.testing.assert_allclose(out.cpu().numpy(), gpr_fwd(g, h0, gamma, k).cpu().numpy(), rtol=1e-4, atol=1e-4)
    dh0, dw, db = dagnn_bwd(g, dy, kept, tw, k)
    gdh0, dgamma = gpr_bwd(g, dy, h0, gamma, k)
    np.testing.assert_allclose(dh0.cpu().numpy(), gdh0.cpu().numpy(), rtol=1e-4, atol=1e-4)
    s = do.sigmoid(b)
    np.testing.assert_allclose(db.item(), s * (1 - s) * dgamma.double().sum().item(), rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------------------------------------------------------- determinism, parameters
@pytest.mark.parametrize("d", [7, 47])
def test_two_runs_are_bit_identical(d):
    from glnn_amd.autograd import dagnn_bwd, dagnn_fwd
    n = 3000
    ip, ix = random_graph(n, 6, seed=11, power=0.6, isolated=9, hub=700)
    g = _csr_graph(ip, ix)
    h0, dy, w, b = _inputs(n, d, 10)
    th0, tdy, tw, tb = _t(h0), _t(dy), _t(w), _t([b])
    runs = []
    for _ in range(2):
        out, kept = dagnn_fwd(g, th0, tw, tb, 10, keep=True)
        runs.append((out,) + tuple(dagnn_bwd(g, tdy, kept, tw, 10)))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


def test_gate_parameters_are_read_from_device_memory_on_every_call(graph):
    """w and b changed IN PLACE between two calls (what Adam does) change the result: nothing of them is cached on the host."""
    from glnn_amd.autograd import dagnn_bwd, dagnn_fwd
    ip, ix, g = graph
    n, d, k = len(ip) - 1, 12, 3
    h0, dy, w, b = _inputs(n, d, k)
    tw, tb = _t(w), _t([b])
    a, kept = dagnn_fwd(g, _t(h0), tw, tb, k, keep=True)
    da = dagnn_bwd(g, _t(dy), kept, tw, k)[0].clone()
    a = a.clone()
    tw.mul_(-0.5)                                                                       # same tensors, same pointers
    tb.add_(1.0)
    w2, b2 = tw.cpu().numpy(), float(tb.item())
    c, kept = dagnn_fwd(g, _t(h0), tw, tb, k, keep=True)
    dc = dagnn_bwd(g, _t(dy), kept, tw, k)[0]
    assert not torch.equal(a, c) and not torch.equal(da, dc)
    np.testing.assert_allclose(c.cpu().numpy(), do.propagate(ip, ix, h0, w2, b2, k), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dc.cpu().numpy(), do.propagate_bwd(ip, ix, dy, h0, w2, b2, k)[0], rtol=1e-4, atol=1e-4)


def test_fold_combines_more_than_one_partial():
    """n = GLNN_DAGNN_FOLD_CHUNK + 1 rows of a degree-1 graph (a ring), K = 2: the stack's 3 n rows leave four stage-1 partials, the last of
    three rows, and the second stage combines them.  Then the fold alone on sizes around its chunk and block sizes."""
    from glnn_amd import _lib, ops
    chunk = _lib.DAGNN_FOLD_CHUNK                                                       # 2048: kFoldRows of csrc/dagnn.hip
    n = chunk + 1
    ip, ix = csr_from_edges((np.arange(n) + 1) % n, np.arange(n), n)
    assert (np.diff(ip) == 1).all()
    _check_propagation(ip, ix, _csr_graph(ip, ix), 3, 2)
    rs = np.random.RandomState(9)
    for rows, d in ((chunk + 1, 5), (1, 1), (255, 47), (chunk, 256), (2 * chunk + 5, 40), (300 * chunk + 3, 4)):
        hs, q = rs.standard_normal((rows, d)).astype(np.float32), rs.standard_normal(rows).astype(np.float32)
        ths = ops.feat_empty(rows, d, DEV)
        ths.copy_(_t(hs))
        dw, db = ops.dagnn_fold(ths, _t(q))
        ref_w, ref_b = hs.astype(np.float64).T @ q.astype(np.float64), q.astype(np.float64).sum()
        # fp64 accumulation, one rounding to fp32 at the end: half an fp32 ulp of the sum plus fp64 noise
        np.testing.assert_allclose(dw.cpu().numpy(), ref_w, rtol=1e-6, atol=1e-6 * np.sqrt(rows))
        np.testing.assert_allclose(db.item(), ref_b, rtol=1e-6, atol=1e-6 * np.sqrt(rows))
        dw2, db2 = ops.dagnn_fold(ths, _t(q))
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ---------------------------------------------------------------------------------------------------------------- model, training step
LR, WD, K_MODEL = 0.01, 0.01, 3
MODEL_DIMS = {"2": (20, 32, 6), "3": (12, 16, 16, 5)}
GATE_W, GATE_B = do.W, do.B


def _model(dims, norm, dropout, seed=0):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    conf = dict(model_name="DAGNN", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=dropout,
                norm_type=norm, device=DEV, dagnn_k=K_MODEL)
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
    """Model.forward / inference in eval mode, then ONE train() step (TeacherEngine.step_dagnn) against the oracle's step fed the library's
    dropout masks: the loss, every gradient (the gate's included), the parameters and both Adam moments after the update."""
    from glnn_amd import ops, teacher
    from glnn_amd.train_and_eval import train
    ip, ix, g = graph
    dims = MODEL_DIMS[dims_key]
    L, n = len(dims) - 1, len(ip) - 1
    m = _model(dims, norm, dropout)
    gate0 = m.encoder.propagate.proj.weight.detach().cpu().numpy().copy()
    x, labels, idx = _data(n, dims)
    tx, tl, ti = _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    params, bn = _np_state(m)
    m.eval()
    ref_logits = do.model_forward(params, bn, ip, ix, x, L, norm, K_MODEL)
    h_list, logits = m.forward_fitnet(g, tx)
    assert len(h_list) == L - 1
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m(g, tx).cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m.inference(g, tx).cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)

    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    loss = train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti)
    eng = teacher.get_engine(m, opt)
    assert eng.kind == "dagnn" and eng.step_count == 1
    masks = None
    if dropout > 0:                                                                     # the masks of step 1, hidden layer l
        masks = [ops.dropout_mask(n, dims[l + 1], dropout, eng._seed(l), DEV).cpu().numpy() for l in range(L - 1)]
    ref_losses, ref_grads, ref_params, ref_state, ref_bn = do.train_steps(params, bn, ip, ix, x, labels, idx, L, norm, K_MODEL,
                                                                          None if masks is None else [masks], dropout, LR, WD, 1)
    print(f"{dims} {norm} p={dropout}: loss {loss:.6f} oracle {ref_losses[0]:.6f}")
    np.testing.assert_allclose(loss, ref_losses[0], rtol=1e-4)
    named = dict(m.named_parameters())
    assert set(named) == set(ref_grads) and {GATE_W, GATE_B} <= set(named)
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
    assert not np.array_equal(m.encoder.propagate.proj.weight.detach().cpu().numpy(), gate0)      # the gate is trained
    fin = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for l, (rm, rv) in ref_bn.items():
        np.testing.assert_allclose(fin[f"encoder.norms.{l}.running_mean"], rm, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(fin[f"encoder.norms.{l}.running_var"], rv, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dims_key,norm", [(dk, norm) for dk in MODEL_DIMS for norm in ("none", "batch", "layer")])
def test_autograd_path_matches_the_engine_gradients(graph, dims_key, norm):
    """Model.forward in training mode differentiates through DagnnPropFn: its gradients equal step_dagnn's (dropout-free configs)."""
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
    assert all(v is not None for v in auto.values()) and {GATE_W, GATE_B} <= set(auto)
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
    assert int(msd["encoder.norms.0.num_batches_tracked"]) == 3
    assert msd[GATE_W].shape == (1, dims[-1]) and msd[GATE_B].shape == (1,)
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
def test_bf16_sharded_and_block_forms_refuse_dagnn(graph):
    from glnn_amd import dist
    _, _, g = graph
    m = _model(MODEL_DIMS["2"], "none", 0.0)
    x = torch.zeros(len(graph[0]) - 1, MODEL_DIMS["2"][0], device=DEV)
    with pytest.raises(NotImplementedError, match="DAGNN"):
        m.inference(g, x, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="DAGNN"):
        dist.ShardedTeacher(m.encoder, g, None, None)
    with pytest.raises(NotImplementedError, match="DAGNN"):
        dist.HaloShardedTeacher(m.encoder, g, None, None)
    with pytest.raises(NotImplementedError, match="DAGNN.*bipartite"):
        m([g], x)


def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_dagnn_teacher_then_student_cli(tmp_path):
    common = ["--dataset", "synthetic-cora", "--teacher", "DAGNN", "--device", "0", "--max_epoch", "3"]
    _run("train_teacher.py", common + ["--save_results", "--dagnn_k", "4"], tmp_path)
    base = tmp_path / "outputs" / "transductive" / "synthetic-cora"
    out_t = np.load(base / "DAGNN" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    sd = torch.load(base / "DAGNN" / "seed_0" / "model.pth", map_location="cpu")
    assert sd[GATE_W].shape == (1, 7) and sd[GATE_B].shape == (1,)
    _run("train_student.py", common + ["--student", "MLP"], tmp_path)
    out_s = np.load(base / "DAGNN_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
