"""torch.autograd.Function shims over the C-ABI kernels, so that `loss.backward()` /
`optimizer.step()` in the reference's generic loops (train_and_eval.py:12-56: `train`, `train_sage`)
keep working on HIP for callers that differentiate `Model.forward` themselves: the dense projections, the neighbour
aggregation and the norm/ReLU/dropout tails run on libglnn_hip.so in both directions.  The training loops of this package
do not go through autograd at all -- see student.py (StudentEngine) and teacher.py (TeacherEngine)."""
import functools
import math

import torch

from . import ops


class _LinearFn(torch.autograd.Function):
    """y = x @ w.T (+ b) with w [out,in] (nn.Linear / fc_neigh layout), or y = x @ w (+ b) with w [in,out]
    (dgl GraphConv layout) when w_is_kn."""

    @staticmethod
    def forward(ctx, x, w, b, w_is_kn):
        x = ops.as_feat(x.detach())
        ctx.save_for_backward(x, w)
        ctx.has_bias, ctx.kn = b is not None, w_is_kn
        return ops.gemm(x, w.detach(), w_is_kn=w_is_kn, ep_shift=None if b is None else b.detach())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = ops.as_feat(dy.contiguous())
        dx = dw = db = None
        n_out = w.shape[1] if ctx.kn else w.shape[0]
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dy, w.detach(), w_is_kn=not ctx.kn)       # dy @ W ([out,in])  |  dy @ W^T ([in,out])
        if ctx.needs_input_grad[1] or ctx.has_bias:
            db_buf = torch.empty(n_out, dtype=torch.float32, device=w.device) if ctx.has_bias else None
            if ctx.kn:
                dw = ops.gemm_tn(x, dy)                             # x^T @ dy -> [in,out]
                if ctx.has_bias:
                    ops.col_sum(dy, out=db_buf)
            else:
                dw = ops.gemm_tn(dy, x, col_sum_a=db_buf)           # dy^T @ x -> [out,in]
            db = db_buf
        return dx, dw, db, None


def linear_fn(x, w, b, w_is_kn=False):
    return _LinearFn.apply(x, w, b, w_is_kn)


class SpmmFn(torch.autograd.Function):
    """Neighbour aggregation with its backward over the transposed graph (A^T dY on the SAME gather kernel, over
    glnn_csr_transpose): the teacher TRAINING direction (reference train_and_eval.py:12-56).
      AGG_SUM       y = row_scale * A (col_scale * x)          dx = col_scale * A^T (row_scale * dy)
      AGG_SAGE_GCN  y = (A x + x[:n_dst]) / (deg + 1)          dx = (A^T + I_dst) (dy / (deg + 1))"""

    @staticmethod
    def forward(ctx, graph, x, mode, row_scale=None, col_scale=None):
        ctx.graph, ctx.mode, ctx.n_src, ctx.rs, ctx.cs = graph, mode, x.shape[0], row_scale, col_scale
        return ops.spmm(graph.indptr, graph.indices, x.detach(), graph.num_dst_nodes(), mode, row_scale=row_scale, col_scale=col_scale)

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[1]:          # e.g. the outermost block: its input is feats[input_nodes]
            return None, None, None, None, None
        g = ctx.graph
        dy = ops.as_feat(dy.contiguous())
        if ctx.mode == ops.AGG_SUM:
            t = g.transposed(False)
            dx = ops.spmm(t.indptr, t.indices, dy, ctx.n_src, ops.AGG_SUM, row_scale=ctx.cs, col_scale=ctx.rs)
        else:
            t = g.transposed(True)
            dx = ops.spmm(t.indptr, t.indices, dy, ctx.n_src, ops.AGG_SUM, col_scale=g.inv_deg_plus1())
        return None, dx, None, None, None


def graphconv_fwd(g, a, w, b, relu):
    """dgl GraphConv(norm='both') forward on HIP (reference models.py:193): returns (y, mid, first).
    first (in > out): y = act(rs * A (cs * (a W)) + b), mid = a;  else: mid = rs * A (cs * a), y = act(mid W + b)."""
    rs, cs = g.degree_norms()
    n = g.num_dst_nodes()
    first = w.shape[0] > w.shape[1]
    if first:
        hw = ops.gemm(a, w, w_is_kn=True, row_scale=cs)
        return ops.spmm(g.indptr, g.indices, hw, n, ops.AGG_SUM, row_scale=rs, ep_shift=b, relu=relu), a, True
    mid = ops.spmm(g.indptr, g.indices, a, n, ops.AGG_SUM, row_scale=rs, col_scale=cs)
    return ops.gemm(mid, w, w_is_kn=True, ep_shift=b, relu=relu), mid, False


def graphconv_bwd(g, dz, mid, first, w, gw, want_da):
    """Backward of graphconv_fwd given dz = d/d(pre-activation): writes dW into gw, returns d/da (or None)."""
    rs, cs = g.degree_norms()
    n = g.num_dst_nodes()
    t = g.transposed(False)
    if first:
        dhw = ops.spmm(t.indptr, t.indices, dz, n, ops.AGG_SUM, row_scale=cs, col_scale=rs)      # cs * A^T (rs * dz)
        ops.gemm_tn(mid, dhw, out=gw)                                                       # a^T dhw -> [in, out]
        return ops.gemm(dhw, w) if want_da else None                                        # dhw W^T
    ops.gemm_tn(mid, dz, out=gw)
    if not want_da:
        return None
    return ops.spmm(t.indptr, t.indices, ops.gemm(dz, w), n, ops.AGG_SUM, row_scale=cs, col_scale=rs)


class GraphConvFn(torch.autograd.Function):
    """One dgl GraphConv(norm='both', activation=relu|None) layer as a differentiable op on the HIP path."""

    @staticmethod
    def forward(ctx, graph, feat, w, b, relu):
        a = ops.as_feat(feat.detach())
        y, mid, first = graphconv_fwd(graph, a, w.detach(), None if b is None else b.detach(), relu)
        ctx.graph, ctx.first, ctx.relu, ctx.has_bias = graph, first, relu, b is not None
        ctx.save_for_backward(mid, y, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        mid, y, w = ctx.saved_tensors
        dy = ops.as_feat(dy.contiguous())
        db = torch.empty(w.shape[1], dtype=torch.float32, device=w.device) if ctx.has_bias else None
        if ctx.relu:
            dz, _, _ = ops.bn_relu_bwd(dy, y, dz_col_sum=db)              # y = relu(z): y > 0 <=> z > 0
        else:
            dz = dy
            if db is not None:
                ops.col_sum(dz, out=db)
        gw = torch.empty_like(w)
        da = graphconv_bwd(ctx.graph, dz, mid, ctx.first, w.detach(), gw, ctx.needs_input_grad[1])
        return None, da, gw, db, None


class _NormActDropFn(torch.autograd.Function):
    """dropout(relu(BatchNorm_train(z))) (or dropout(relu(z)) without a norm) as ONE differentiable op on the HIP path:
    glnn_bn_stats_f32 (batch statistics + running-stat update) -> glnn_act_fwd_f32; backward = glnn_bn_relu_bwd_f32 with the
    same counter-based dropout seed.  Replaces `self.norms[l](h)` -> `self.activation(h)` -> `self.dropout(h)` of the
    reference's training-mode forwards (models.py:48-52, 113-117)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, bn, p, seed, relu=True):
        z = ops.as_feat(z.detach())
        ctx.relu = relu
        ctx.layer_norm = isinstance(bn, torch.nn.LayerNorm)
        if ctx.layer_norm:
            y, mean, rstd = ops.layernorm_fwd(z, None if gamma is None else gamma.detach(), None if beta is None else beta.detach(),
                                              eps=bn.eps, relu=relu, drop_p=p, drop_seed=seed)
            ctx.save_for_backward(z, mean, rstd, *(t.detach() for t in (gamma, beta) if t is not None))
            ctx.has_bn, ctx.p, ctx.seed, ctx.affine = False, p, seed, gamma is not None
            return y
        if bn is not None:
            mean, rstd, a_scale, a_shift = ops.bn_stats(z, gamma.detach(), beta.detach(), bn.running_mean, bn.running_var,
                                                        bn.num_batches_tracked, eps=bn.eps, momentum=bn.momentum)
            ctx.save_for_backward(z, gamma.detach(), mean, rstd, a_scale, a_shift)
        else:
            a_scale = a_shift = None
            ctx.save_for_backward(z)
        ctx.has_bn, ctx.p, ctx.seed = bn is not None, p, seed
        return ops.act_fwd(z, a_scale, a_shift, drop_p=p, drop_seed=seed, relu=relu)

    @staticmethod
    def backward(ctx, dy):
        dy = ops.as_feat(dy.contiguous())
        if ctx.layer_norm:
            z, mean, rstd, *aff = ctx.saved_tensors
            gamma, beta = (aff + [None, None])[:2] if ctx.affine else (None, None)
            dz, dgamma, dbeta = ops.layernorm_bwd(dy, z, gamma, beta, mean, rstd, relu=ctx.relu, drop_p=ctx.p, drop_seed=ctx.seed)
            return dz, dgamma, dbeta, None, None, None, None
        if ctx.has_bn:
            z, gamma, mean, rstd, a_scale, a_shift = ctx.saved_tensors
            dz, dgamma, dbeta = ops.bn_relu_bwd(dy, z, gamma, mean, rstd, a_scale, a_shift, drop_p=ctx.p, drop_seed=ctx.seed, relu=ctx.relu)
            return dz, dgamma, dbeta, None, None, None, None
        (z,) = ctx.saved_tensors
        dz, _, _ = ops.bn_relu_bwd(dy, z, drop_p=ctx.p, drop_seed=ctx.seed, relu=ctx.relu)
        return dz, None, None, None, None, None, None


_drop_counter = [0]


def _draw_base(count=None):
    """The base of the count-th per-process dropout draw of a graph teacher's op (a site's seed: (base + its tag) & 0xFFFFFFFF).  None: a
    NEW draw, the one place the call counter advances for APPNP, GCNII and the attention layers; tests replay masks from a recorded count."""
    if count is None:
        _drop_counter[0] += 1
        count = _drop_counter[0]
    return int(torch.initial_seed()) * 0x85EBCA77 + count * 0x9E3779B1


def _differentiable(training, *tensors):
    """The rule of every graph teacher's op: through its autograd.Function only in training mode with something to differentiate;
    otherwise the forward runs under no_grad and keeps nothing for a backward."""
    return training and torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _pingpong(n, d, device, count):
    """buf(t) for step t of a chain of `count` launches that each read the one before: two [n, d] buffers in turn (or one, or none)."""
    bufs = [ops.feat_empty(n, d, device) for _ in range(min(count, 2))]
    return lambda t: bufs[t % len(bufs)]


def norm_act_drop(z, bn, p, relu=True):
    """Training-mode tail of a hidden layer: norm -> ReLU -> dropout (MLP / SAGE, reference models.py:48-52, 113-117) or, with
    relu=False, norm -> dropout (GCN, models.py:195-198: the ReLU sits inside the GraphConv).  bn: nn.BatchNorm1d (reference
    defaults), nn.LayerNorm, or None; p: dropout probability.
    The dropout stream is counter-based: seed = hash(torch.initial_seed(), call counter) -- _draw_base's multipliers the other way
    round, and the counter advances for p = 0 too, so it keeps its own line."""
    _drop_counter[0] += 1
    seed = (int(torch.initial_seed()) * 0x9E3779B1 + _drop_counter[0] * 0x85EBCA77) & 0xFFFFFFFF if p > 0 else 0
    if bn is not None:
        return _NormActDropFn.apply(z, bn.weight, bn.bias, bn, float(p), seed, relu)
    return _NormActDropFn.apply(z, None, None, None, float(p), seed, relu)


# ------------------------------------------------------------------------------------------ APPNP propagation (dgl APPNPConv)
def appnp_fwd(g, h0, k, alpha, edge_drop=0.0, seed=0):
    """h_K of K power iterations  h_t = (1 - alpha) D_in^-1/2 M_t A D_out^-1/2 h_{t-1} + alpha h0  (reference models.py:342, dgl
    APPNPConv): K launches of glnn_appnp_prop_f32 ping-ponging two buffers; M_t = the edge-dropout mask of iteration t (edge_drop = 0: none)."""
    h0 = ops.as_feat(h0)
    n, d = h0.shape
    if k == 0:
        out = ops.feat_empty(n, d, h0.device)
        out.copy_(h0)
        return out
    in_norm, out_norm = g.degree_norms()
    nnz = g.num_edges()
    buf = _pingpong(n, d, h0.device, k)
    x = h0
    for t in range(1, k + 1):
        x = ops.appnp_propagate(g.indptr, g.indices, x, nnz, t, in_norm, out_norm, h0, alpha, edge_drop, seed, x_scaled=t > 1,
                                last=t == k, out=buf(t))
    return x


def appnp_bwd(g, dy, k, alpha, edge_drop=0.0, seed=0):
    """dL/dh0 from dL/dh_K: the propagation is linear, so no iterate is saved --  acc = 0; for t = K..1: acc += alpha g_t,
    g_{t-1} = (1 - alpha) P_t^T g_t;  dL/dh0 = g_0 + acc.  K launches of glnn_appnp_prop_bwd_f32 over the transposed graph with edge ids
    (each launch evaluates the same edge mask as forward iteration t)."""
    dy = ops.as_feat(dy)
    n, d = dy.shape
    if k == 0:
        return dy
    in_norm, out_norm = g.degree_norms()
    tg, t_eids = g.transposed_eids()
    nnz = g.num_edges()
    acc = ops.feat_empty(n, d, dy.device) if k > 1 else None
    buf = _pingpong(n, d, dy.device, k)
    x = dy
    for t in range(k, 0, -1):
        x = ops.appnp_propagate_bwd(tg.indptr, tg.indices, t_eids, x, nnz, t, t == k, in_norm, out_norm, alpha, edge_drop, seed, acc=acc,
                                    out=buf(t))
    return x


class AppnpPropFn(torch.autograd.Function):
    """APPNPConv(k, alpha, edge_drop) as a differentiable op on the HIP path; the backward replays the forward's edge masks from (seed, t)."""

    @staticmethod
    def forward(ctx, graph, h0, k, alpha, edge_drop, seed):
        ctx.graph, ctx.k, ctx.alpha, ctx.edge_drop, ctx.seed = graph, k, alpha, edge_drop, seed
        return appnp_fwd(graph, h0.detach(), k, alpha, edge_drop, seed)

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        dh0 = appnp_bwd(ctx.graph, dy.contiguous(), ctx.k, ctx.alpha, ctx.edge_drop, ctx.seed)
        return None, dh0, None, None, None, None


def appnp_edge_seed(count):
    """The edge-dropout seed of the count-th dropout draw of this process (tests replay the masks from it; None: a new draw)."""
    return (_draw_base(count) + 0x41505050) & 0xFFFFFFFF


def appnp_propagate(graph, h0, k, alpha, edge_drop, training):
    """APPNPConv forward of the reference's APPNP (models.py:342): edge dropout only in training (one _draw_base draw)."""
    p = float(edge_drop) if training else 0.0
    seed = appnp_edge_seed(None) if p > 0 else 0
    if _differentiable(training, h0):
        return AppnpPropFn.apply(graph, h0, int(k), float(alpha), p, seed)
    with torch.no_grad():
        return appnp_fwd(graph, h0, int(k), float(alpha), p, seed)


# ------------------------------------------------------------------------------------------ GPR-GNN propagation (docs/GPR_SEMANTICS.md)
def _gpr_run(csr, nnz, x0, gamma, k, first_norm, row_norm, h0=None):
    """acc = sum_{j <= k} gamma[j] Q^j x0 over `csr` (Q = diag(row_norm) A diag(first_norm)): K launches of glnn_gpr_prop_f32 ping-ponging
    two buffers (the step-K row is not stored), or the k = 0 entry alone.  h0: also the per-row scalars <Q^j x0, h0>; returns (acc, row_dot)."""
    n, d = x0.shape
    acc = ops.feat_empty(n, d, x0.device)
    row_dot = None
    if h0 is not None:
        row_dot = torch.empty((k + 1) * ops.gpr_col_tiles(d) * n, dtype=torch.float32, device=x0.device)
    if k == 0:
        ops.gpr_prop(None, None, 0, x0, 0, None, None, None, gamma, acc, h0=h0, row_dot=row_dot)
        return acc, row_dot
    buf = _pingpong(n, d, x0.device, k - 1)
    x = x0
    for j in range(1, k + 1):
        x = ops.gpr_prop(csr.indptr, csr.indices, nnz, x, j, first_norm if j == 1 else None, row_norm, first_norm, gamma, acc,
                         out=None if j == k else buf(j), h0=h0, row_dot=row_dot)
    return acc, row_dot


def gpr_fwd(g, h0, gamma, k):
    """out = sum_{j = 0..K} gamma[j] P^j h0,  P = D_in^-1/2 A D_out^-1/2 (APPNP's operator; A[i, j] = the number of edges j -> i).  gamma
    [K + 1] is read on the device."""
    h0 = ops.as_feat(h0)
    in_norm, out_norm = g.degree_norms()
    return _gpr_run(g, g.num_edges(), h0, gamma, int(k), out_norm, in_norm)[0]


def gpr_bwd(g, dy, h0, gamma, k):
    """(dL/dh0, dL/dgamma) from dy = dL/dout:  G_0 = dy, G_j = P^T G_{j-1} (a gather over the transposed CSR with the norms swapped);
    dh0 = sum gamma[j] G_j, dgamma[j] = <G_j, h0>.  No forward iterate is saved: the per-row dots leave the K launches' epilogues and
    glnn_gpr_fold_f32 sums them in a fixed order."""
    dy, h0 = ops.as_feat(dy), ops.as_feat(h0)
    n, d = dy.shape
    k = int(k)
    in_norm, out_norm = g.degree_norms()
    tg = g.transposed(False)
    dh0, row_dot = _gpr_run(tg, g.num_edges(), dy, gamma, k, in_norm, out_norm, h0=h0)
    return dh0, ops.gpr_fold(row_dot, k + 1, ops.gpr_col_tiles(d) * n)


class GprPropFn(torch.autograd.Function):
    """GPRConv as a differentiable op on the HIP path: gradients for the trunk's logits and for the K + 1 coefficients."""

    @staticmethod
    def forward(ctx, graph, h0, gamma, k):
        h0 = ops.as_feat(h0.detach())
        ctx.graph, ctx.k = graph, k
        ctx.save_for_backward(h0, gamma)
        return gpr_fwd(graph, h0, gamma.detach(), k)

    @staticmethod
    def backward(ctx, dy):
        h0, gamma = ctx.saved_tensors
        dh0, dgamma = gpr_bwd(ctx.graph, dy.contiguous(), h0, gamma.detach(), ctx.k)
        return None, dh0 if ctx.needs_input_grad[1] else None, dgamma if ctx.needs_input_grad[2] else None, None


def gpr_propagate(graph, h0, gamma, k, training):
    """GPRConv forward, differentiable by _differentiable's rule."""
    if _differentiable(training, h0, gamma):
        return GprPropFn.apply(graph, h0, gamma, int(k))
    with torch.no_grad():
        return gpr_fwd(graph, h0, gamma, int(k))


# ------------------------------------------------------------------------------------------ DAGNN propagation (docs/DAGNN_SEMANTICS.md)
def dagnn_fwd(g, h0, w, b, k, keep=False):
    """out[i] = sum_{j = 0..K} s_j[i] H_j[i],  H_0 = h0, H_j = P H_{j-1}, s_j[i] = sigmoid(<H_j[i], w> + b)  (P = APPNP's operator): per hop
    one glnn_spmm_csr_f32 (rows scaled by dst_norm, sources by src_norm) and one glnn_dagnn_gate_f32.  keep False (eval): two ping-pong
    buffers and out.  keep True (training): every H_j is stored once, into the saved stack [(K + 1) n, d] the next hop gathers from;
    returns (out, (stack, gates [(K + 1) n])).  w [d] / [1, d] and b [1] are read on the device."""
    h0 = ops.as_feat(h0)
    n, d = h0.shape
    k = int(k)
    out = ops.feat_empty(n, d, h0.device)
    stack = score = None
    if keep:
        stack = ops.feat_empty((k + 1) * n, d, h0.device)
        stack[:n].copy_(h0)
        score = torch.empty((k + 1) * n, dtype=torch.float32, device=h0.device)
    ops.dagnn_gate(h0, 0, w, b, out, score)
    if k > 0:
        in_norm, out_norm = g.degree_norms()
        buf = None if keep else _pingpong(n, d, h0.device, k)
        x = h0
        for j in range(1, k + 1):
            x = ops.spmm(g.indptr, g.indices, x, n, ops.AGG_SUM, row_scale=in_norm, col_scale=out_norm,
                         out=stack[j * n:(j + 1) * n] if keep else buf(j))
            ops.dagnn_gate(x, j, w, b, out, score)
    return (out, (stack, score)) if keep else out


def dagnn_bwd(g, dy, kept, w, k):
    """(dL/dh0, dL/dw, dL/db) from dy = dL/dout and the forward's kept (stack, gates):  q_j = <dy, H_j> s_j (1 - s_j),
    D_j = s_j dy + q_j w,  T_K = D_K, T_j = D_j + P^T T_{j+1},  dh0 = T_0 -- per hop one glnn_spmm_csr_f32 over the transposed CSR with the
    norms swapped and one glnn_dagnn_gate_bwd_f32 in place on its output -- and dw = sum_j H_j^T q_j, db = sum q (glnn_dagnn_fold_f32:
    fixed-order fp64 sums over the stack)."""
    dy = ops.as_feat(dy)
    n, d = dy.shape
    k = int(k)
    stack, score = kept
    q = torch.empty((k + 1) * n, dtype=torch.float32, device=dy.device)
    buf = _pingpong(n, d, dy.device, k + 1)
    x = ops.dagnn_gate_bwd(dy, stack[k * n:(k + 1) * n], k, score, w, None, buf(k), q)
    if k > 0:
        in_norm, out_norm = g.degree_norms()
        tg = g.transposed(False)
        for j in range(k - 1, -1, -1):
            t = ops.spmm(tg.indptr, tg.indices, x, n, ops.AGG_SUM, row_scale=out_norm, col_scale=in_norm, out=buf(j))
            x = ops.dagnn_gate_bwd(dy, stack[j * n:(j + 1) * n], j, score, w, t, t, q)
    dw, db = ops.dagnn_fold(stack, q)
    return x, dw, db


class DagnnPropFn(torch.autograd.Function):
    """DAGNNConv as a differentiable op on the HIP path: gradients for the trunk's logits and for the gate's weight and bias."""

    @staticmethod
    def forward(ctx, graph, h0, w, b, k):
        out, (stack, score) = dagnn_fwd(graph, h0.detach(), w.detach(), b.detach(), k, keep=True)
        ctx.graph, ctx.k = graph, k
        ctx.save_for_backward(stack, score, w)
        return out

    @staticmethod
    def backward(ctx, dy):
        stack, score, w = ctx.saved_tensors
        dh0, dw, db = dagnn_bwd(ctx.graph, dy.contiguous(), (stack, score), w.detach(), ctx.k)
        need = ctx.needs_input_grad
        return None, dh0 if need[1] else None, dw.view_as(w) if need[2] else None, db if need[3] else None, None


def dagnn_propagate(graph, h0, w, b, k, training):
    """DAGNNConv forward, differentiable by _differentiable's rule."""
    if _differentiable(training, h0, w, b):
        return DagnnPropFn.apply(graph, h0, w, b, int(k))
    with torch.no_grad():
        return dagnn_fwd(graph, h0, w, b, int(k))


# ------------------------------------------------------------------------------------------ GCNII conv stack (docs/GCNII_SEMANTICS.md)
def gcnii_betas(num_layers, lamda):
    """beta_l = log(lamda / l + 1) for l = 1..L (the paper's identity-mapping weights)."""
    return [math.log(float(lamda) / l + 1.0) for l in range(1, int(num_layers) + 1)]


def gcnii_fwd(g, h0, weights, alpha, betas, drop_p=0.0, seeds=None, save=False):
    """The L conv layers over h0 = H_0: L launches of glnn_gcnii_layer_f32, each gathering the previous layer's UNSCALED rows (every H_l
    is an output of the model; x_norm = src_norm rides in the gather).  seeds (training, drop_p > 0): seeds[l] keys drop_l, l = 1..L.
    Returns ([H_1..H_L], [S_1..S_L] when save else None)."""
    h0 = ops.as_feat(h0)
    n, d = h0.shape
    in_norm, out_norm = g.degree_norms()
    nnz = g.num_edges()
    hs, ss = [], [] if save else None
    x = h0
    for l, w in enumerate(weights, 1):
        s = ops.feat_empty(n, d, h0.device) if save else None
        x = ops.gcnii_layer(g.indptr, g.indices, nnz, x, h0, w, alpha, betas[l - 1], in_norm, x_norm=out_norm,
                            drop_p=drop_p, drop_seed=seeds[l] if drop_p > 0 else 0, s_out=s)
        hs.append(x)
        if save:
            ss.append(s)
    return hs, ss


def gcnii_bwd(g, da, hs, ss, weights, alpha, betas, dws, drop_p=0.0, seeds=None, drop_last=True):
    """dL/dH_0 (before H_0's own ReLU mask) from da = dL/d drop_{L+1}(H_L): L launches of glnn_gcnii_layer_bwd_f32 over the transposed
    graph -- layer L in the plain form, the others gathering the previous launch's dS, stored PRE-SCALED by dst_norm so that no gather of
    the chain multiplies per edge -- each followed by dW_l = (beta_l dZ_l)^T S_l (glnn_gemm_tn_f32 into dws[l - 1]), and one launch
    without a product for H_0.  seeds[l] keys drop_l (l = 1..L + 1); drop_last False: da is already behind drop_{L+1}'s mask (autograd)."""
    da = ops.as_feat(da)
    n, d = da.shape
    L = len(weights)
    in_norm, out_norm = g.degree_norms()
    tg = g.transposed(False)
    nnz = g.num_edges()
    dz, acc = ops.feat_empty(n, d, da.device), ops.feat_empty(n, d, da.device)
    buf = _pingpong(n, d, da.device, L)
    seed = lambda s: seeds[s] if drop_p > 0 else 0
    x = da
    for l in range(L, 0, -1):
        p_l = drop_p if (l < L or drop_last) else 0.0
        x = ops.gcnii_layer_bwd(tg.indptr, tg.indices, nnz, x, hs[l - 1], weights[l - 1].t().contiguous(), alpha, betas[l - 1], dz, acc,
                                first=l == L, row_norm=out_norm, out_norm=in_norm, plain=l == L, drop_p=p_l, drop_seed=seed(l + 1),
                                dz_scale=betas[l - 1], ds_out=buf(l))
        ops.gemm_tn(dz, ss[l - 1], out=dws[l - 1])
    return ops.gcnii_layer_bwd(tg.indptr, tg.indices, nnz, x, None, None, alpha, 0.0, dz, acc, first=False, row_norm=out_norm,
                               drop_p=drop_p, drop_seed=seed(1))


class GcniiStackFn(torch.autograd.Function):
    """The GCNII conv stack as ONE differentiable op on the HIP path: H_L carries the gradient (to H_0 and to every W_l); H_1..H_{L-1} are
    returned for the callers that list hidden states and are not differentiable.  The backward replays the dropout masks from the seeds."""

    @staticmethod
    def forward(ctx, graph, h0, alpha, betas, drop_p, seeds, *weights):
        h0 = ops.as_feat(h0.detach())
        ws = [w.detach() for w in weights]
        hs, ss = gcnii_fwd(graph, h0, ws, alpha, betas, drop_p, seeds, save=True)
        ctx.graph, ctx.cfg, ctx.L = graph, (alpha, betas, drop_p, seeds), len(ws)
        ctx.save_for_backward(*hs, *ss, *weights)
        ctx.mark_non_differentiable(*hs[:-1])
        return tuple(hs)

    @staticmethod
    def backward(ctx, *dys):
        L = ctx.L
        saved = ctx.saved_tensors
        hs, ss, ws = saved[:L], saved[L:2 * L], [w.detach() for w in saved[2 * L:]]
        alpha, betas, drop_p, seeds = ctx.cfg
        dws = [torch.empty_like(w) for w in ws]
        dh0 = gcnii_bwd(ctx.graph, dys[-1].contiguous(), hs, ss, ws, alpha, betas, dws, drop_p, seeds, drop_last=False)
        return (None, dh0 if ctx.needs_input_grad[1] else None, None, None, None, None) + tuple(dws)


def gcnii_stack_seeds(count, sites):
    """The seeds of the dropout sites 0..sites-1 of the count-th dropout draw of this process (tests replay the masks; None: a new draw)."""
    base = _draw_base(count) + 0x47434E32
    return [(base + s * 0x632BE5AB) & 0xFFFFFFFF for s in range(sites)]


def gcnii_stack(graph, h0, weights, alpha, betas, drop_p, training):
    """[H_1..H_L] of the conv stack: the per-layer dropout only in training (one _draw_base draw for all its sites)."""
    p = float(drop_p) if training else 0.0
    seeds = gcnii_stack_seeds(None, len(weights) + 2) if p > 0 else None
    if _differentiable(training, h0, *weights):
        return list(GcniiStackFn.apply(graph, h0, float(alpha), tuple(betas), p, seeds, *weights))
    with torch.no_grad():
        return gcnii_fwd(graph, h0, list(weights), float(alpha), betas, p, seeds)[0]


# ------------------------------------------------------------------------------------------ what the two attention layers share
def _attn_seeds(count, tag_feat, tag_attn):
    """(feature-dropout seed, attention-dropout seed) of the count-th dropout draw of this process (tests replay them; None: a new draw)."""
    base = _draw_base(count)
    return (base + tag_feat) & 0xFFFFFFFF, (base + tag_attn) & 0xFFFFFFFF


gat_conv_seeds = functools.partial(_attn_seeds, tag_feat=0x47415446, tag_attn=0x47415441)
gatv2_conv_seeds = functools.partial(_attn_seeds, tag_feat=0x47563246, tag_attn=0x47563241)


def _attn_conv(fn, layer_fwd, seeds, graph, x, params, shape, feat_drop, attn_drop, training, *extra):
    """Both attention convs: the dropouts only in training (one _draw_base draw).  shape = (heads, out_feats, slope, relu)."""
    fp, ap = (float(feat_drop), float(attn_drop)) if training else (0.0, 0.0)
    fs, as_ = seeds(None) if fp > 0 or ap > 0 else (0, 0)
    args = (*params, *shape, fp, fs, ap, as_, *extra)
    if _differentiable(training, x, *params):
        return fn.apply(graph, x, *args)
    with torch.no_grad():
        return layer_fwd(graph, ops.as_feat(x), *args)[0]


def _attn_backward(dy, y, relu, feat_p, feat_seed, layer_bwd):
    """layer_bwd(gy = dy * [y > 0] for a ReLU layer) with the feature-dropout mask and 1 / (1 - p) on the input gradient it returns first."""
    dy = ops.as_feat(dy.contiguous())
    da, *grads = layer_bwd(ops.bn_relu_bwd(dy, y)[0] if relu else dy)
    if da is not None and feat_p > 0:
        da = ops.act_fwd(da, drop_p=feat_p, drop_seed=feat_seed, relu=False)
    return (da, *grads)


# ------------------------------------------------------------------------------------------ GAT layer (dgl 0.6.1 GATConv)
def gat_layer_fwd(g, x, w, attn_l, attn_r, heads, out_feats, slope, relu, feat_p=0.0, feat_seed=0, attn_p=0.0, attn_seed=0, signed=True,
                  want_lse=False):
    """One GATConv forward (docs/GAT_SEMANTICS.md): projection with the feature dropout in the operand load, el / er from one read of z,
    edge softmax + aggregation (+ ReLU).  Returns (y, (z, el, er, lse)); lse only when the backward will follow."""
    z, z2 = ops.gat_project(x, w, feat_p, feat_seed, signed)
    el, er = ops.gat_scores(z, attn_l, attn_r, heads, out_feats, z2=z2)
    y, lse = ops.gat_attn_fwd(g.indptr, g.indices, g.num_edges(), z, el, er, heads, out_feats, slope, attn_p, attn_seed, relu=relu,
                              want_lse=want_lse)
    return y, (z, el, er, lse)


def gat_layer_bwd(g, gy, y, saved, x, w, attn_l, attn_r, heads, out_feats, slope, feat_p=0.0, feat_seed=0, attn_p=0.0, attn_seed=0,
                  signed=True, need_dx=True, dw=None, dattn_l=None, dattn_r=None):
    """Backward of gat_layer_fwd.  gy = dL/dy ALREADY behind the activation mask (zero where a ReLU layer's y is 0).  Returns
    (da = dz W -- the input gradient BEFORE the feature-dropout mask, or None; dW; dattn_l; dattn_r)."""
    z, el, er, lse = saved
    dz, dal, dar = ops.gat_attn_bwd(g, z, el, er, lse, attn_l, attn_r, gy, y, heads, out_feats, slope, attn_p, attn_seed,
                                    dattn_l=dattn_l, dattn_r=dattn_r)
    dw = ops.gat_project_wgrad(dz, x, feat_p, feat_seed, signed, out=dw)
    da = ops.gemm(dz, w, w_is_kn=True) if need_dx else None
    return da, dw, dal, dar


class GatConvFn(torch.autograd.Function):
    """GATConv as a differentiable op on the HIP path; the backward replays the forward's dropout masks from their seeds."""

    @staticmethod
    def forward(ctx, graph, x, w, attn_l, attn_r, heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed, signed):
        x = ops.as_feat(x.detach())
        y, saved = gat_layer_fwd(graph, x, w.detach(), attn_l.detach(), attn_r.detach(), heads, out_feats, slope, relu, feat_p, feat_seed,
                                 attn_p, attn_seed, signed, want_lse=True)
        ctx.graph, ctx.cfg = graph, (heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed, signed)
        ctx.save_for_backward(x, w, attn_l, attn_r, y, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, attn_l, attn_r, y, z, el, er, lse = ctx.saved_tensors
        heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed, signed = ctx.cfg
        da, dw, dal, dar = _attn_backward(dy, y, relu, feat_p, feat_seed, lambda gy: gat_layer_bwd(
            ctx.graph, gy, y, (z, el, er, lse), x, w.detach(), attn_l.detach(), attn_r.detach(), heads, out_feats, slope, feat_p, feat_seed,
            attn_p, attn_seed, signed, need_dx=ctx.needs_input_grad[1]))
        return (None, da, dw, dal.view_as(attn_l), dar.view_as(attn_r)) + (None,) * 9


def gat_conv(graph, x, w, attn_l, attn_r, heads, out_feats, slope, relu, feat_drop, attn_drop, training, signed=True):
    """GATConv forward (_attn_conv's rule)."""
    return _attn_conv(GatConvFn, gat_layer_fwd, gat_conv_seeds, graph, x, (w, attn_l, attn_r), (heads, out_feats, slope, relu), feat_drop,
                      attn_drop, training, signed)


# ------------------------------------------------------------------------------------------ GATv2 layer (docs/GATV2_SEMANTICS.md)
def gatv2_layer_fwd(g, x, w_src, b_src, w_dst, b_dst, attn, heads, out_feats, slope, relu, feat_p=0.0, feat_seed=0, attn_p=0.0, attn_seed=0,
                    want_lse=False):
    """One GATv2Conv forward: the dropped copy of the input (made once, read by both projections and by both weight gradients; a signed
    input needs nothing else), zl = fc_src, zr = fc_dst, glnn_gatv2_attn_fwd_f32 (+ ReLU).  Returns (y, (xd, zl, zr, lse)); lse only when
    the backward will follow."""
    xd = ops.act_fwd(x, drop_p=feat_p, drop_seed=feat_seed, relu=False) if feat_p > 0 else x
    zl = ops.gemm(xd, w_src, ep_shift=b_src)
    zr = ops.gemm(xd, w_dst, ep_shift=b_dst)
    y, lse = ops.gatv2_attn_fwd(g.indptr, g.indices, g.num_edges(), zl, zr, attn, heads, out_feats, slope, attn_p, attn_seed, relu=relu,
                                want_lse=want_lse)
    return y, (xd, zl, zr, lse)


def gatv2_layer_bwd(g, gy, saved, w_src, w_dst, attn, heads, out_feats, slope, attn_p=0.0, attn_seed=0, need_dx=True, dw_src=None,
                    db_src=None, dw_dst=None, db_dst=None, dattn=None):
    """Backward of gatv2_layer_fwd.  gy = dL/dy ALREADY behind the activation mask (zero where a ReLU layer's y is 0).  Returns
    (da = dzl W_src + dzr W_dst -- the input gradient BEFORE the feature-dropout mask, or None; dW_src; db_src; dW_dst; db_dst; dattn)."""
    xd, zl, zr, lse = saved
    dzl, dzr, dattn = ops.gatv2_attn_bwd(g, zl, zr, lse, attn, gy, heads, out_feats, slope, attn_p, attn_seed, dattn=dattn)
    hf = heads * out_feats
    if db_src is None:
        db_src = torch.empty(hf, dtype=torch.float32, device=zl.device)
    if db_dst is None:
        db_dst = torch.empty(hf, dtype=torch.float32, device=zl.device)
    dw_src = ops.gemm_tn(dzl, xd, out=dw_src, col_sum_a=db_src)
    dw_dst = ops.gemm_tn(dzr, xd, out=dw_dst, col_sum_a=db_dst)
    da = None
    if need_dx:
        da = ops.gemm(dzl, w_src, w_is_kn=True)
        da.add_(ops.gemm(dzr, w_dst, w_is_kn=True))
    return da, dw_src, db_src, dw_dst, db_dst, dattn


class Gatv2ConvFn(torch.autograd.Function):
    """GATv2Conv as a differentiable op on the HIP path; the backward replays the forward's dropout masks from their seeds."""

    @staticmethod
    def forward(ctx, graph, x, w_src, b_src, w_dst, b_dst, attn, heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed):
        x = ops.as_feat(x.detach())
        y, saved = gatv2_layer_fwd(graph, x, w_src.detach(), b_src.detach(), w_dst.detach(), b_dst.detach(), attn.detach(), heads, out_feats,
                                   slope, relu, feat_p, feat_seed, attn_p, attn_seed, want_lse=True)
        ctx.graph, ctx.cfg = graph, (heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed)
        ctx.save_for_backward(w_src, w_dst, attn, y, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        w_src, w_dst, attn, y, xd, zl, zr, lse = ctx.saved_tensors
        heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed = ctx.cfg
        da, dws, dbs, dwd, dbd, dat = _attn_backward(dy, y, relu, feat_p, feat_seed, lambda gy: gatv2_layer_bwd(
            ctx.graph, gy, (xd, zl, zr, lse), w_src.detach(), w_dst.detach(), attn.detach(), heads, out_feats, slope, attn_p, attn_seed,
            need_dx=ctx.needs_input_grad[1]))
        return (None, da, dws, dbs, dwd, dbd, dat.view_as(attn)) + (None,) * 8


def gatv2_conv(graph, x, w_src, b_src, w_dst, b_dst, attn, heads, out_feats, slope, relu, feat_drop, attn_drop, training):
    """GATv2Conv forward (_attn_conv's rule)."""
    return _attn_conv(Gatv2ConvFn, gatv2_layer_fwd, gatv2_conv_seeds, graph, x, (w_src, b_src, w_dst, b_dst, attn),
                      (heads, out_feats, slope, relu), feat_drop, attn_drop, training)


# ------------------------------------------------------------------------------------------ graph-transformer layer (docs/GT_SEMANTICS.md)
gt_conv_seeds = functools.partial(_attn_seeds, tag_feat=0x47545246, tag_attn=0x47545241)
GT_PROJECTIONS = ("key", "query", "value", "skip")        # the order of TransformerConv's four nn.Linear, and of every (w, b) list below


def gt_layer_fwd(g, x, wk, bk, wq, bq, wv, bv, ws, bs, heads, out_feats, slope, relu, feat_p=0.0, feat_seed=0, attn_p=0.0, attn_seed=0,
                 want_lse=False):
    """One TransformerConv forward: the dropped copy of the input (made once, as gatv2_layer_fwd does: read by the four projections and
    by the four weight gradients), k / q / v / skip = the four Linear layers, glnn_gt_attn_fwd_f32 (+ ReLU).  `slope` is _attn_conv's
    shape slot and is not used.  Returns (y, (xd, q, k, v, lse)); lse only when the backward will follow."""
    xd = ops.act_fwd(x, drop_p=feat_p, drop_seed=feat_seed, relu=False) if feat_p > 0 else x
    k = ops.gemm(xd, wk, ep_shift=bk)
    q = ops.gemm(xd, wq, ep_shift=bq)
    v = ops.gemm(xd, wv, ep_shift=bv)
    s = ops.gemm(xd, ws, ep_shift=bs)
    y, lse = ops.gt_attn_fwd(g.indptr, g.indices, g.num_edges(), q, k, v, s, heads, out_feats, attn_p, attn_seed, relu=relu,
                             want_lse=want_lse)
    return y, (xd, q, k, v, lse)


def gt_layer_bwd(g, gy, saved, wk, wq, wv, ws, heads, out_feats, attn_p=0.0, attn_seed=0, need_dx=True, dw=None, db=None):
    """Backward of gt_layer_fwd.  gy = dL/dy ALREADY behind the activation mask (zero where a ReLU layer's y is 0).  dw / db: optional
    lists of four output tensors in GT_PROJECTIONS order.  Returns (da = dk Wk + dq Wq + dv Wv + gy Ws -- the input gradient BEFORE the
    feature-dropout mask, or None; [dWk, dWq, dWv, dWs]; [dbk, dbq, dbv, dbs])."""
    xd, q, k, v, lse = saved
    gy = ops.as_feat(gy)
    dq, dk, dv = ops.gt_attn_bwd(g, q, k, v, lse, gy, heads, out_feats, attn_p, attn_seed)
    hf = heads * out_feats
    dw = [None] * 4 if dw is None else list(dw)
    db = [None] * 4 if db is None else list(db)
    da = None
    for i, (dz, w) in enumerate(((dk, wk), (dq, wq), (dv, wv), (gy, ws))):       # (the skip row's gradient is gy itself)
        if db[i] is None:
            db[i] = torch.empty(hf, dtype=torch.float32, device=gy.device)
        dw[i] = ops.gemm_tn(dz, xd, out=dw[i], col_sum_a=db[i])
        if need_dx:
            t = ops.gemm(dz, w, w_is_kn=True)
            da = t if da is None else da.add_(t)
    return da, dw, db


class GtConvFn(torch.autograd.Function):
    """TransformerConv as a differentiable op on the HIP path; the backward replays the forward's dropout masks from their seeds."""

    @staticmethod
    def forward(ctx, graph, x, wk, bk, wq, bq, wv, bv, ws, bs, heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed):
        x = ops.as_feat(x.detach())
        y, saved = gt_layer_fwd(graph, x, wk.detach(), bk.detach(), wq.detach(), bq.detach(), wv.detach(), bv.detach(), ws.detach(),
                                bs.detach(), heads, out_feats, slope, relu, feat_p, feat_seed, attn_p, attn_seed, want_lse=True)
        ctx.graph, ctx.cfg = graph, (heads, out_feats, relu, feat_p, feat_seed, attn_p, attn_seed)
        ctx.save_for_backward(wk, wq, wv, ws, y, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        wk, wq, wv, ws, y, xd, q, k, v, lse = ctx.saved_tensors
        heads, out_feats, relu, feat_p, feat_seed, attn_p, attn_seed = ctx.cfg
        da, dw, db = _attn_backward(dy, y, relu, feat_p, feat_seed, lambda gy: gt_layer_bwd(
            ctx.graph, gy, (xd, q, k, v, lse), wk.detach(), wq.detach(), wv.detach(), ws.detach(), heads, out_feats, attn_p, attn_seed,
            need_dx=ctx.needs_input_grad[1]))
        return (None, da, dw[0], db[0], dw[1], db[1], dw[2], db[2], dw[3], db[3]) + (None,) * 8


def gt_conv(graph, x, wk, bk, wq, bq, wv, bv, ws, bs, heads, out_feats, relu, feat_drop, attn_drop, training):
    """TransformerConv forward (_attn_conv's rule; the shape's slope slot is unused)."""
    return _attn_conv(GtConvFn, gt_layer_fwd, gt_conv_seeds, graph, x, (wk, bk, wq, bq, wv, bv, ws, bs), (heads, out_feats, 0.0, relu),
                      feat_drop, attn_drop, training)


# ------------------------------------------------------------------------------------------ PNA layer (docs/PNA_SEMANTICS.md)
def pna_conv_seed(count=None):
    """The feature-dropout seed of the count-th dropout draw of this process (tests replay it; None: a new draw)."""
    return (_draw_base(count) + 0x504E4146) & 0xFFFFFFFF


def pna_weights(w_pre, w_post, f):
    """The operands the launches read, cut from PNAConv's two Linear weights (w_pre [F, 2F] = [W_dst | W_src], w_post [Fo, 13F] =
    [W_x | W_0 | W_1 | W_2], one 4F block per scaler): (W_dst, W_src, W_x, W_stack) with W_stack [3 round4(Fo), 4 round4(F)] the three
    scaler blocks one under the other in S's part layout (zeros in the padding), so that ONE product of S gives all three."""
    fo = w_post.shape[0]
    fp, fop = ops.round4(f), ops.round4(fo)
    w_stack = w_post.new_zeros((3, fop, 4, fp))
    w_stack[:, :fo, :, :f] = w_post[:, f:].reshape(fo, 3, 4, f).permute(1, 0, 2, 3)
    return w_pre[:, :f].contiguous(), w_pre[:, f:].contiguous(), w_post[:, :f].contiguous(), w_stack.view(3 * fop, 4 * fp)


def pna_layer_fwd(g, x, w_pre, b_pre, w_post, b_post, delta, relu, feat_p=0.0, feat_seed=0, keep=False):
    """One PNAConv forward: the dropped copy x' of the input (made once), a = x' W_dst^T + b_pre and b = x' W_src^T,
    glnn_pna_agg_fwd_f32 (S = [a + mean | a + min | a + max | std] of b over the in-edges), out = x' W_x^T + b_post, Z = S W_stack^T (one
    product for the three scaler blocks: the 12F matrix is never formed) and glnn_pna_scale_fwd_f32 (out += Z_0 + s_amp Z_1 + s_att Z_2,
    + ReLU).  Returns (out, (x', b, S, mu, arg)); mu and arg only with keep (the backward will follow)."""
    n, f = x.shape
    xd = ops.act_fwd(x, drop_p=feat_p, drop_seed=feat_seed, relu=False) if feat_p > 0 else x
    w_dst, w_src, w_x, w_stack = pna_weights(w_pre, w_post, f)
    a = ops.gemm(xd, w_dst, ep_shift=b_pre)
    b = ops.gemm(xd, w_src)
    s, mu, arg = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), b, g.num_dst_nodes(), a=a, want_arg=keep)
    out = ops.gemm(xd, w_x, ep_shift=b_post)
    z = ops.gemm(s, w_stack)
    ops.pna_scale_fwd(g.indptr, z, out, delta, relu=relu)
    return out, (xd, b, s, mu, arg)


def pna_layer_bwd(g, gy, saved, w_pre, w_post, delta, need_dx=True, dw_pre=None, db_pre=None, dw_post=None, db_post=None):
    """Backward of pna_layer_fwd.  gy = dL/d out ALREADY behind the activation mask.  dZ = [gy | s_amp gy | s_att gy]
    (glnn_pna_scale_bwd_f32), dS = dZ W_stack -- the scalers are folded in BEFORE the gather, which reads 4F gradient floats per edge --
    da (glnn_pna_da_f32), db (glnn_pna_agg_bwd_f32 over the transposed graph), the four weight gradients with their bias column sums.
    Returns (dx' = gy W_x + da W_dst + db W_src -- the input gradient BEFORE the feature-dropout mask, or None; dW_pre; db_pre; dW_post;
    db_post)."""
    xd, b, s, mu, arg = saved
    gy = ops.as_feat(gy)
    n, f = xd.shape
    fo = w_post.shape[0]
    fp, fop = ops.round4(f), ops.round4(fo)
    w_dst, w_src, w_x, w_stack = pna_weights(w_pre, w_post, f)
    dev = gy.device
    dw_pre = torch.empty_like(w_pre) if dw_pre is None else dw_pre
    dw_post = torch.empty_like(w_post) if dw_post is None else dw_post
    db_pre = torch.empty(f, dtype=torch.float32, device=dev) if db_pre is None else db_pre
    db_post = torch.empty(fo, dtype=torch.float32, device=dev) if db_post is None else db_post
    dz = ops.pna_scale_bwd(g.indptr, gy, delta)
    dw_post[:, :f] = ops.gemm_tn(gy, xd, col_sum_a=db_post)
    dw_stack = ops.gemm_tn(dz, s)
    dw_post[:, f:] = dw_stack.view(3, fop, 4, fp)[:, :fo, :, :f].permute(1, 0, 2, 3).reshape(fo, 12 * f)
    ds = ops.gemm(dz, w_stack, w_is_kn=True, out=torch.empty((n, 4 * fp), dtype=torch.float32, device=dev))
    da = ops.pna_da(g.indptr, ds, f)
    db = ops.pna_agg_bwd(g, ds, b, mu, s, arg)
    dw_pre[:, :f] = ops.gemm_tn(da, xd, col_sum_a=db_pre)
    dw_pre[:, f:] = ops.gemm_tn(db, xd)
    dx = None
    if need_dx:
        dx = ops.gemm(gy, w_x, w_is_kn=True)
        dx.add_(ops.gemm(da, w_dst, w_is_kn=True))
        dx.add_(ops.gemm(db, w_src, w_is_kn=True))
    return dx, dw_pre, db_pre, dw_post, db_post


class PnaConvFn(torch.autograd.Function):
    """PNAConv as a differentiable op on the HIP path; the backward replays the forward's dropout mask from its seed."""

    @staticmethod
    def forward(ctx, graph, x, w_pre, b_pre, w_post, b_post, delta, relu, feat_p, feat_seed):
        x = ops.as_feat(x.detach())
        y, saved = pna_layer_fwd(graph, x, w_pre.detach(), b_pre.detach(), w_post.detach(), b_post.detach(), delta, relu, feat_p, feat_seed,
                                 keep=True)
        ctx.graph, ctx.cfg = graph, (delta, relu, feat_p, feat_seed)
        ctx.save_for_backward(w_pre, w_post, y, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        w_pre, w_post, y, xd, b, s, mu, arg = ctx.saved_tensors
        delta, relu, feat_p, feat_seed = ctx.cfg
        da, dwp, dbp, dwo, dbo = _attn_backward(dy, y, relu, feat_p, feat_seed, lambda gy: pna_layer_bwd(
            ctx.graph, gy, (xd, b, s, mu, arg), w_pre.detach(), w_post.detach(), delta, need_dx=ctx.needs_input_grad[1]))
        return (None, da, dwp, dbp, dwo, dbo) + (None,) * 4


def pna_conv(graph, x, w_pre, b_pre, w_post, b_post, delta, relu, feat_drop, training):
    """PNAConv forward: the dropout only in training (one _draw_base draw), through PnaConvFn by _differentiable's rule."""
    fp = float(feat_drop) if training else 0.0
    fs = pna_conv_seed(None) if fp > 0 else 0
    if _differentiable(training, x, w_pre, b_pre, w_post, b_post):
        return PnaConvFn.apply(graph, x, w_pre, b_pre, w_post, b_post, float(delta), relu, fp, fs)
    with torch.no_grad():
        return pna_layer_fwd(graph, ops.as_feat(x), w_pre, b_pre, w_post, b_post, float(delta), relu, fp, fs)[0]
