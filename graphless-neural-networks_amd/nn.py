"""Drop-in modules for the dgl layers the reference's teachers use, computing on libglnn_hip.so.

  SAGEConv(in, out, "gcn")(block, (h, h_dst))   <- dgl.nn.SAGEConv, reference models.py:84-99,112,138
  GraphConv(in, out, activation=)(g, h)          <- dgl.nn.GraphConv, reference models.py:170-187,193
  GATConv(in, out, heads, ...)(g, h)             <- dgl.nn.GATConv, reference models.py:228-267 (docs/GAT_SEMANTICS.md)
  GATv2Conv(in, out, heads, ...)(g, h)           <- GATv2's attention layer (dgl 0.6.1 has none; docs/GATV2_SEMANTICS.md)
  TransformerConv(in, out, heads, ...)(g, h)     <- UniMP's dot-product attention layer with a skip row (docs/GT_SEMANTICS.md)
  GPRConv(k, alpha, init)(g, h)                  <- GPR-GNN's learned K-step propagation (no dgl counterpart; docs/GPR_SEMANTICS.md)
  DAGNNConv(k, in_feats)(g, h)                   <- DAGNN's node-gated K-step propagation (no dgl counterpart; docs/DAGNN_SEMANTICS.md)
  GCNIIConv(hidden, layer, alpha, lamda)(g, h, h0) <- one GCNII conv layer (dgl 0.6.1 has none; docs/GCNII_SEMANTICS.md)
  PNAConv(in, out, delta, ...)(g, h)             <- PyG's PNAConv, one tower, mean/min/max/std x three scalers (docs/PNA_SEMANTICS.md)

Parameter names follow dgl 0.6.1 so that a reference `model.pth` loads: SAGEConv.fc_neigh.{weight,bias}
(weight [out,in], xavier_uniform gain=relu; no fc_self for "gcn"), GraphConv.{weight [in,out] xavier_uniform,
bias zeros}.  Only what the reference constructs is implemented; anything else raises.

Adding a teacher family: its conv here, its row in kinds.KINDS (what every name list, refusal and dispatch reads), its encoder and
Model.__init__ branch in models.py, TeacherEngine.step_<kind> in teacher.py."""

import math

import torch
import torch.nn as nn

from . import ops
from .autograd import (GraphConvFn, SpmmFn, _differentiable, dagnn_propagate, gat_conv, gatv2_conv, gcnii_stack, gt_conv, gpr_propagate, graphconv_fwd,
                       linear_fn, pna_conv)


FUSED_SAGE_MAX_IN = 256   # aggregate-first layers with d_in, d_out <= 256 take the single-launch K1F kernel.  Interleaved
                          # A/B on one MI355X, products shape (scripts/ab_fused.py): 100->256 10.6 vs 12.5 ms,
                          # 128->256 11.4 vs 12.2 ms, 256->256 23.6 vs 25.1 ms (fused vs aggregation + GEMM)


MEAN_COMPOSE_SHAPES = frozenset()      # (d_in, d_out) of "mean" layers that the fused launch does NOT win on a GPU measurement and that
                                       # therefore take the composition (scripts/bench_sage_mean.py; DESIGN.md "SAGE mean")


def mean_row_scale(graph):
    """1 / max(in_deg, 1) per destination row (fp32, cached on the graph): the row scale that turns GLNN_AGG_SUM into the mean."""
    if "inv_deg_clamp1" not in graph._cache:
        graph._cache["inv_deg_clamp1"] = (1.0 / graph.in_degrees().clamp(min=1).to(torch.float32)).contiguous()
    return graph._cache["inv_deg_clamp1"]


def _add_epilogue(y, s, ep_scale, ep_shift, relu, out):
    """epi(y + s) of the composed "mean" form (plumbing of the fallback: the hot forms fuse it)."""
    y = y + s
    if ep_scale is not None:
        y = y * ep_scale
    if ep_shift is not None:
        y = y + ep_shift
    if relu:
        y = torch.relu_(y)
    if out is not None:
        out.copy_(y)
        return out
    return y


class SAGEConv(nn.Module):
    def __init__(self, in_feats, out_feats, aggregator_type, bias=True):
        super().__init__()
        if aggregator_type not in ("gcn", "mean"):
            raise NotImplementedError(f"SAGEConv(..., {aggregator_type!r}): only the 'gcn' aggregator the reference builds (models.py:84-99) and "
                                      "the 'mean' aggregator (docs/SAGE_MEAN_SEMANTICS.md) are implemented")
        self._in_feats, self._out_feats = in_feats, out_feats
        self._aggre_type = aggregator_type
        if aggregator_type == "mean":
            self.fc_self = nn.Linear(in_feats, out_feats, bias=bias)      # (registered first, as dgl 0.6.1 does)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        if self._aggre_type == "mean":
            nn.init.xavier_uniform_(self.fc_self.weight, gain=nn.init.calculate_gain("relu"))
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=nn.init.calculate_gain("relu"))

    def mean_bias(self):
        """The "mean" layer's effective bias fc_self.bias + fc_neigh.bias (None without biases), remembered while both are unmodified."""
        bs, bn = self.fc_self.bias, self.fc_neigh.bias
        if bs is None:
            return None
        key = (ops.PARAM_EPOCH, bs.data_ptr(), bs._version, bn.data_ptr(), bn._version)
        ent = self.__dict__.get("_mean_bias")
        if ent is None or ent[0] != key:
            self.__dict__["_mean_bias"] = ent = (key, (bs.detach() + bn.detach()).contiguous())
        return ent[1]

    def mean_form(self):
        """Which eval form a "mean" layer takes: "fused" (one launch, d_in <= d_out <= 256), "project" (d_in > d_out, d_out <= 256:
        one GEMM against the stacked weights, then the aggregation at the narrower width) or "compose" (aggregation with a row scale
        plus two GEMMs)."""
        if self._in_feats <= self._out_feats <= 256 and (self._in_feats, self._out_feats) not in MEAN_COMPOSE_SHAPES:
            return "fused"
        if self._in_feats > self._out_feats and self._out_feats <= 256:
            return "project"
        return "compose"

    def forward_mean(self, graph, feat, ep_scale=None, ep_shift=None, relu=False, w_packed=None, out=None, form=None):
        """out = fc_self(h_dst) + fc_neigh(mean_{u->v} h[u]) (deg 0: the mean is 0).  ep_* / relu: the fused tail of SAGE.inference, which
        then folds the summed bias itself.  form: force "fused" / "project" / "compose" (tests and A/B timing; default mean_form())."""
        h_src, h_dst = feat if isinstance(feat, tuple) else (feat, feat)
        n_dst = graph.num_dst_nodes()
        if h_dst.shape[0] != n_dst:
            raise ValueError("SAGEConv: h_dst must hold the block's destination rows")
        wn, ws = self.fc_neigh.weight, self.fc_self.weight
        if torch.is_grad_enabled() and (h_src.requires_grad or h_dst.requires_grad or wn.requires_grad or ws.requires_grad):
            agg = SpmmFn.apply(graph, h_src, ops.AGG_SUM, mean_row_scale(graph))
            return linear_fn(h_dst, ws, self.fc_self.bias) + linear_fn(agg, wn, self.fc_neigh.bias)
        fused_tail = ep_scale is not None or ep_shift is not None or relu
        shift = ep_shift if fused_tail else self.mean_bias()
        form = form or self.mean_form()
        if form == "fused":
            order = graph.fused_tile_order() if n_dst == graph.n_dst else None
            return ops.sage_mean_fused(graph.indptr, graph.indices, h_src, n_dst, wn, ws, ep_scale=ep_scale, ep_shift=shift, relu=relu,
                                       x_self=h_dst, w_packed=w_packed, tile_order=order, out=out)
        if form == "project":
            # project first (linear commutes with the mean): ONE product against [W_neigh; W_self], aggregate at the narrower width
            r4 = ops.round4(self._out_feats)
            p = ops.gemm(ops.as_feat(h_src), ops.stack_weight_pair(wn, ws))
            return ops.spmm_sage_mean(graph.indptr, graph.indices, p[:, :self._out_feats], p[:, r4:], n_dst, ep_scale=ep_scale,
                                      ep_shift=shift, relu=relu, out=out)
        if form != "compose":
            raise ValueError(f"SAGEConv.forward_mean: unknown form {form!r}")
        agg = ops.spmm(graph.indptr, graph.indices, h_src, n_dst, ops.AGG_SUM, row_scale=mean_row_scale(graph))
        y = ops.gemm(agg, wn)
        s = ops.gemm(ops.as_feat(h_dst), ws)
        return _add_epilogue(y, s, ep_scale, shift, relu, out)

    def fused_eligible(self):
        """Aggregate-first layers with d_in, d_out <= 256 run on the single-launch K1F kernel ("gcn" only: the "mean" forms are
        mean_form()'s)."""
        return self._aggre_type == "gcn" and self._in_feats <= self._out_feats and self._in_feats <= FUSED_SAGE_MAX_IN and self._out_feats <= 256

    def forward(self, graph, feat, ep_scale=None, ep_shift=None, relu=False, w_packed=None, out=None, agg_out=None, agg_in=None):
        """out = fc_neigh((sum_{u->v} h[u] + h_dst[v]) / (deg(v)+1)).  ep_* / relu: optional fused tail
        (eval-mode BatchNorm + ReLU of the caller) used by SAGE.inference; bias is folded by the caller then.
        w_packed: ops.pack_weight(fc_neigh.weight) of a caller that sweeps many blocks with the same weights (the chunked
        inference loop packs once per layer instead of once per chunk).  out (inference only): where the layer's rows go
        (SAGE.inference hands a placed buffer, ops.placed_for_gather, to the layers whose output the next layer gathers).
        agg_out / agg_in (inference, fused-eligible layers only): the kept neighbour aggregate of ops.sage_fused."""
        if self._aggre_type == "mean":
            if agg_out is not None or agg_in is not None:
                raise NotImplementedError("SAGEConv 'mean': the kept neighbour aggregate (agg_out / agg_in) belongs to the 'gcn' launch")
            return self.forward_mean(graph, feat, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, w_packed=w_packed, out=out)
        h_src, h_dst = feat if isinstance(feat, tuple) else (feat, feat)
        n_dst = graph.num_dst_nodes()
        if h_dst.shape[0] != n_dst:
            raise ValueError("SAGEConv: h_dst must hold the block's destination rows")
        w, b = self.fc_neigh.weight, self.fc_neigh.bias
        needs_grad = torch.is_grad_enabled() and (h_src.requires_grad or w.requires_grad)
        if needs_grad:
            agg = SpmmFn.apply(graph, h_src, ops.AGG_SAGE_GCN)
            return linear_fn(agg, w, b)
        fused_tail = ep_scale is not None or ep_shift is not None or relu
        shift = ep_shift if fused_tail else b
        if (agg_out is not None or agg_in is not None) and not self.fused_eligible():
            raise ValueError("SAGEConv: agg_out / agg_in belong to the fused launch (fused_eligible())")
        # (no ops.HubPlan here: a whole-graph launch is long enough to hide its hub rows behind the heaviest-first tile order -- measured on
        #  the arxiv-shaped graph the extra launch costs 10-60 us per layer and gains nothing; row shards use one: glnn_amd/dist.py)
        if self._in_feats > self._out_feats:
            # project first (linear commutes with the mean): aggregate at the narrower width
            hw = ops.gemm(ops.as_feat(h_src), w)
            return ops.spmm(graph.indptr, graph.indices, hw, n_dst, ops.AGG_SAGE_GCN, ep_scale=ep_scale,
                            ep_shift=shift, relu=relu, out=out)
        if self._in_feats <= FUSED_SAGE_MAX_IN and self._out_feats <= 256:
            # aggregation + projection + epilogue in one launch: the aggregated rows never reach HBM
            order = graph.fused_tile_order() if n_dst == graph.n_dst else None
            return ops.sage_fused(graph.indptr, graph.indices, h_src, n_dst, w, ep_scale=ep_scale, ep_shift=shift, relu=relu,
                                  x_self=h_dst, w_packed=w_packed, tile_order=order, out=out, agg_out=agg_out, agg_in=agg_in)
        agg = ops.spmm(graph.indptr, graph.indices, h_src, n_dst, ops.AGG_SAGE_GCN)
        return ops.gemm(agg, w, ep_scale=ep_scale, ep_shift=shift, relu=relu, out=out)

    def forward_bf16(self, graph, h_src, h_dst, ep_scale=None, ep_shift=None, relu=False, out_dtype=torch.float32):
        """Eval-mode layer with bf16 activation STORAGE (SAGE.inference(..., dtype=torch.bfloat16)): the forms `forward` picks, where every
        matrix an aggregation gathers is bf16 and all arithmetic is fp32.  h_src / h_dst: bf16 rows when the layer aggregates first, fp32
        when it projects first (a GEMM is then their only reader).  out_dtype: torch.bfloat16 when the next layer gathers the result."""
        if self._aggre_type == "mean":
            raise NotImplementedError("SAGEConv 'mean': bf16 activation storage is implemented for the 'gcn' aggregator only")
        n_dst = graph.num_dst_nodes()
        w, b = self.fc_neigh.weight, self.fc_neigh.bias
        fused_tail = ep_scale is not None or ep_shift is not None or relu
        shift = ep_shift if fused_tail else b
        if self._in_feats > self._out_feats:
            # project first in fp32, store the projection as bf16, aggregate it
            hw = ops.to_bf16(ops.gemm(ops.as_feat(h_src), w))
            return ops.spmm(graph.indptr, graph.indices, hw, n_dst, ops.AGG_SAGE_GCN, ep_scale=ep_scale, ep_shift=shift, relu=relu,
                            out_dtype=out_dtype)
        if self._in_feats <= FUSED_SAGE_MAX_IN and self._out_feats <= 256:
            order = graph.fused_tile_order() if n_dst == graph.n_dst else None
            return ops.sage_fused(graph.indptr, graph.indices, h_src, n_dst, w, ep_scale=ep_scale, ep_shift=shift, relu=relu,
                                  x_self=h_dst, tile_order=order, out_dtype=out_dtype)
        # aggregate the bf16 rows into an fp32 matrix, then the fp32 GEMM
        agg = ops.spmm(graph.indptr, graph.indices, h_src, n_dst, ops.AGG_SAGE_GCN, x_self=h_dst, out_dtype=torch.float32)
        y = ops.gemm(agg, w, ep_scale=ep_scale, ep_shift=shift, relu=relu)
        return ops.to_bf16(y) if out_dtype == torch.bfloat16 else y

    def forward_i8(self, graph, h_src, h_dst, ep_scale=None, ep_shift=None, relu=False, out_dtype=torch.float32):
        """Eval-mode layer with int8 activation STORAGE (SAGE.inference(..., dtype=torch.int8); docs/INT8_INFERENCE_SEMANTICS.md): the forms
        `forward_bf16` picks, where every matrix an aggregation gathers is int8 rows (ops.to_int8_rows) and all arithmetic is fp32.
        h_src / h_dst: int8 rows of in_feats columns when the layer aggregates first, fp32 when it projects first (a GEMM is then their only
        reader).  out_dtype: torch.int8 when the next layer gathers the result (int8 rows of out_feats columns come back)."""
        if self._aggre_type == "mean":
            raise NotImplementedError("SAGEConv 'mean': int8 activation storage is implemented for the 'gcn' aggregator only")
        n_dst = graph.num_dst_nodes()
        w, b = self.fc_neigh.weight, self.fc_neigh.bias
        fused_tail = ep_scale is not None or ep_shift is not None or relu
        shift = ep_shift if fused_tail else b
        gathered = min(self._in_feats, self._out_feats)      # the width this layer's aggregation gathers
        if gathered > ops.I8_MAX_WIDTH:
            raise NotImplementedError(f"SAGEConv: int8 rows are at most {ops.I8_MAX_WIDTH} columns wide and this layer aggregates "
                                      f"{gathered} columns (torch.bfloat16 storage takes any width)")
        if self._in_feats > self._out_feats:
            # project first in fp32, store the projection as int8 rows, aggregate them
            hw = ops.to_int8_rows(ops.gemm(ops.as_feat(h_src), w))
            return ops.spmm_sage_gcn_i8(graph.indptr, graph.indices, hw, self._out_feats, n_dst, ep_scale=ep_scale, ep_shift=shift, relu=relu,
                                        out_dtype=out_dtype)
        if self._out_feats <= 256:
            order = graph.fused_tile_order() if n_dst == graph.n_dst else None
            y = ops.sage_fused_i8(graph.indptr, graph.indices, h_src, self._in_feats, n_dst, w, ep_scale=ep_scale, ep_shift=shift, relu=relu,
                                  x_self=h_dst, tile_order=order)
        else:
            # aggregate the int8 rows into an fp32 matrix, then the fp32 GEMM
            agg = ops.spmm_sage_gcn_i8(graph.indptr, graph.indices, h_src, self._in_feats, n_dst, x_self=h_dst, out_dtype=torch.float32)
            y = ops.gemm(agg, w, ep_scale=ep_scale, ep_shift=shift, relu=relu)
        return ops.to_int8_rows(y) if out_dtype == torch.int8 else y


class GraphConv(nn.Module):
    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True, activation=None,
                 allow_zero_in_degree=False):
        super().__init__()
        if norm != "both" or not weight:
            raise NotImplementedError("the reference only builds GraphConv(in, out, activation=...) (models.py:170-187)")
        self._in_feats, self._out_feats = in_feats, out_feats
        self._activation = activation
        self._allow_zero_in_degree = allow_zero_in_degree
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.empty(out_feats)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, graph, feat):
        if not self._allow_zero_in_degree and graph.has_zero_in_degree():
            raise RuntimeError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid "
                               "(dgl GraphConv semantics; add self-loops or set allow_zero_in_degree).")
        act = self._activation
        relu = act is not None and getattr(act, "__name__", "") == "relu"
        if act is not None and not relu:
            raise NotImplementedError("GraphConv: only activation=F.relu or None is used by the reference")
        if torch.is_grad_enabled() and (feat.requires_grad or self.weight.requires_grad):
            return GraphConvFn.apply(graph, feat, self.weight, self.bias, relu)
        return graphconv_fwd(graph, ops.as_feat(feat), self.weight, self.bias, relu)[0]


class _AttnConv(nn.Module):
    """What GATConv, GATv2Conv and TransformerConv share: the constructor's refusals, relu(), forward's guards and the [N, heads, out] view.  A subclass
    registers its parameters in make_parameters() and draws them in reset_parameters() (its own RNG stream) and ends the messages."""
    WHOLE_GRAPH = RESIDUAL = ACTIVATION = ZERO_IN_DEGREE = None

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False):
        super().__init__()
        who = type(self).__name__
        if isinstance(in_feats, (tuple, list)):
            raise NotImplementedError(f"{who}: bipartite (block) inputs are not implemented: {self.WHOLE_GRAPH}")
        if residual:
            raise NotImplementedError(f"{who}: residual=True is not implemented ({self.RESIDUAL})")
        if num_heads < 1 or num_heads > 64 or num_heads * out_feats > 256:
            raise NotImplementedError(f"{who}: the attention kernels take num_heads <= 64 and num_heads * out_feats <= 256")
        self._in_feats, self._out_feats, self._num_heads = in_feats, out_feats, num_heads
        self._allow_zero_in_degree = allow_zero_in_degree
        self.activation = activation
        self.make_parameters(in_feats, out_feats, num_heads)
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.negative_slope = float(negative_slope)
        self.reset_parameters()

    def relu(self):
        act = self.activation
        relu = act is not None and getattr(act, "__name__", "") == "relu"
        if act is not None and not relu:
            raise NotImplementedError(f"{type(self).__name__}: only activation=F.relu or None is {self.ACTIVATION}")
        return relu

    def check_inputs(self, graph, feat):
        if (isinstance(graph, (list, tuple)) or isinstance(feat, tuple) or graph.num_dst_nodes() != graph.num_src_nodes()
                or feat.shape[0] != graph.num_dst_nodes()):
            raise NotImplementedError(f"{type(self).__name__}: block (bipartite) inputs are not implemented: {self.WHOLE_GRAPH}")
        if not self._allow_zero_in_degree and graph.has_zero_in_degree():
            raise RuntimeError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid "
                               f"({self.ZERO_IN_DEGREE}; add self-loops or set allow_zero_in_degree).")

    def by_head(self, y):
        shape = (y.shape[0], self._num_heads, self._out_feats)
        return y.view(shape) if y.is_contiguous() else y.reshape(shape)


class GATConv(_AttnConv):
    """dgl 0.6.1 GATConv on a homogeneous graph (docs/GAT_SEMANTICS.md): fc [heads * out, in] without bias, attn_l / attn_r [1, heads, out],
    no bias parameter, res_fc a None buffer (residual=False only).  forward returns [N, heads, out]."""
    WHOLE_GRAPH = "the reference's GAT runs on the whole graph"
    RESIDUAL = "the reference's Model never sets it"
    ACTIVATION = "used by the reference"
    ZERO_IN_DEGREE = "dgl GATConv semantics"

    def make_parameters(self, in_feats, out_feats, num_heads):
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.register_buffer("res_fc", None)

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, graph, feat, nonneg=None):
        """nonneg: the caller knows feat >= 0 (a ReLU layer's output), so the feature dropout needs one product (ops.gat_project);
        None: looked at here when the dropout is active."""
        self.check_inputs(graph, feat)
        if nonneg is None:
            nonneg = not (self.training and self.feat_drop.p > 0) or ops.is_nonneg(feat)
        return self.by_head(gat_conv(graph, feat, self.fc.weight, self.attn_l, self.attn_r, self._num_heads, self._out_feats,
                                     self.negative_slope, self.relu(), self.feat_drop.p, self.attn_drop.p, self.training, signed=not nonneg))


class GATv2Conv(_AttnConv):
    """GATv2 attention layer on a homogeneous graph (Brody, Alon, Yahav, ICLR 2022; docs/GATV2_SEMANTICS.md): fc_src / fc_dst
    [heads * out, in] WITH bias, attn [1, heads, out]; no share_weights, no residual, no output bias.  forward returns [N, heads, out]."""
    WHOLE_GRAPH = "the GATv2 teacher runs on the whole graph"
    RESIDUAL = "docs/GATV2_SEMANTICS.md, What is refused"
    ACTIVATION = "implemented (the attention kernel's epilogue)"
    ZERO_IN_DEGREE = "GATv2Conv follows dgl GATConv"

    def make_parameters(self, in_feats, out_feats, num_heads):
        self.fc_src = nn.Linear(in_feats, out_feats * num_heads, bias=True)
        self.fc_dst = nn.Linear(in_feats, out_feats * num_heads, bias=True)
        self.attn = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.relu()                                # an activation the kernel's epilogue lacks is refused by the constructor

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc_src.weight, gain=gain)
        nn.init.xavier_normal_(self.fc_dst.weight, gain=gain)
        nn.init.xavier_normal_(self.attn, gain=gain)
        nn.init.zeros_(self.fc_src.bias)
        nn.init.zeros_(self.fc_dst.bias)

    def forward(self, graph, feat):
        self.check_inputs(graph, feat)
        return self.by_head(gatv2_conv(graph, feat, self.fc_src.weight, self.fc_src.bias, self.fc_dst.weight, self.fc_dst.bias, self.attn,
                                       self._num_heads, self._out_feats, self.negative_slope, self.relu(), self.feat_drop.p,
                                       self.attn_drop.p, self.training))


class TransformerConv(_AttnConv):
    """Graph-transformer attention layer on a homogeneous graph (the TransformerConv of UniMP: Shi et al., IJCAI 2021;
    docs/GT_SEMANTICS.md): lin_key / lin_query / lin_value / lin_skip [heads * out, in] WITH bias, torch's default Linear initialisation,
    constructed in that order; scaled dot-product edge softmax, the skip row added to the aggregate.  No beta gate, no edge features, no
    concat=False mean; negative_slope is accepted (the stack passes it) and unused.  forward returns [N, heads, out]."""
    WHOLE_GRAPH = "the GraphTransformer teacher runs on the whole graph"
    RESIDUAL = "docs/GT_SEMANTICS.md, What is refused: lin_skip is the layer's skip connection"
    ACTIVATION = "implemented (the attention kernel's epilogue)"
    ZERO_IN_DEGREE = "TransformerConv follows dgl GATConv"

    def make_parameters(self, in_feats, out_feats, num_heads):
        for name in ("lin_key", "lin_query", "lin_value", "lin_skip"):
            setattr(self, name, nn.Linear(in_feats, out_feats * num_heads, bias=True))
        self.relu()                                # an activation the kernel's epilogue lacks is refused by the constructor

    def reset_parameters(self):
        """Nothing to redraw: the four nn.Linear keep the default initialisation their constructors drew."""

    def forward(self, graph, feat):
        self.check_inputs(graph, feat)
        lins = (self.lin_key, self.lin_query, self.lin_value, self.lin_skip)
        return self.by_head(gt_conv(graph, feat, *(t for lin in lins for t in (lin.weight, lin.bias)), self._num_heads, self._out_feats,
                                    self.relu(), self.feat_drop.p, self.attn_drop.p, self.training))


def _whole_graph_only(graph, feat, who, why):
    """Refuses a block (bipartite) input: a list of blocks, a (src, dst) feature pair, other source than destination rows, other rows."""
    if (isinstance(graph, (list, tuple)) or isinstance(feat, tuple) or graph.num_dst_nodes() != graph.num_src_nodes()
            or feat.shape[0] != graph.num_dst_nodes()):
        raise NotImplementedError(f"{who}: block (bipartite) inputs are not implemented: {why}")


GPR_INITS = ("PPR", "NPPR", "Random")


class GPRConv(nn.Module):
    """GPR-GNN propagation (Chien et al., ICLR 2021; docs/GPR_SEMANTICS.md): out = sum_{j = 0..K} gamma[j] P^j h with ONE parameter,
    gamma [K + 1] fp32, and P = D_in^-1/2 A D_out^-1/2 (APPNP's operator).  No edge dropout, no dropout of its own, no zero-in-degree
    error (a row without in-edges keeps gamma[0] h alone).  init: the paper's released initialisations "PPR" | "NPPR" | "Random"."""

    def __init__(self, k=10, alpha=0.1, init="PPR"):
        super().__init__()
        if init not in GPR_INITS:
            raise ValueError(f"GPRConv: init must be one of {GPR_INITS} (got {init!r})")
        if int(k) < 0:
            raise ValueError(f"GPRConv: k must be >= 0 (got {k})")
        self.k, self.alpha, self.init = int(k), float(alpha), init
        self.gamma = nn.Parameter(torch.empty(self.k + 1, dtype=torch.float32))
        self.reset_parameters()

    def reset_parameters(self):
        k, a = self.k, self.alpha
        j = torch.arange(k + 1, dtype=torch.float64)
        with torch.no_grad():
            if self.init == "PPR":               # APPNP's teleport weights: they sum to 1
                g = a * (1.0 - a) ** j
                g[k] = (1.0 - a) ** k
            elif self.init == "NPPR":
                g = a ** j
                g = g / g.abs().sum()
            else:                                # "Random": uniform(-b, b), b = sqrt(3 / (K + 1)), from torch's default generator
                b = (3.0 / (k + 1)) ** 0.5
                g = nn.init.uniform_(torch.empty(k + 1, dtype=torch.float32), -b, b).to(torch.float64)
                g = g / g.abs().sum()
            self.gamma.copy_(g.to(torch.float32))

    def forward(self, graph, feat):
        _whole_graph_only(graph, feat, "GPRConv", "GPR-GNN propagates over the whole graph")
        return gpr_propagate(graph, feat, self.gamma, self.k, self.training)


class DAGNNConv(nn.Module):
    """DAGNN propagation (Liu, Gao, Ji, KDD 2020; docs/DAGNN_SEMANTICS.md): out[i] = sum_{j = 0..K} s_j[i] (P^j h)[i] with the node-adaptive
    gate s_j[i] = sigmoid(proj((P^j h)[i])), proj = nn.Linear(in_feats, 1) (torch's default initialisation), and P = D_in^-1/2 A D_out^-1/2
    (APPNP's operator).  No edge dropout, no dropout of its own, no zero-in-degree error (a row without in-edges keeps s_0 h alone)."""

    def __init__(self, k=10, in_feats=1):
        super().__init__()
        if int(k) < 0:
            raise ValueError(f"DAGNNConv: k must be >= 0 (got {k})")
        if int(in_feats) > ops.DAGNN_MAX_WIDTH:
            raise NotImplementedError(f"DAGNNConv: DAGNN rows of at most {ops.DAGNN_MAX_WIDTH} columns (the gate is one row-wide dot product; "
                                      f"got {in_feats})")
        self.k, self.in_feats = int(k), int(in_feats)
        self.proj = nn.Linear(self.in_feats, 1)

    def reset_parameters(self):
        self.proj.reset_parameters()

    def forward(self, graph, feat):
        _whole_graph_only(graph, feat, "DAGNNConv", "DAGNN propagates over the whole graph")
        return dagnn_propagate(graph, feat, self.proj.weight, self.proj.bias, self.k, self.training)


class GCNIIConv(nn.Module):
    """One GCNII conv layer (Chen et al., ICML 2020, eq. 5; docs/GCNII_SEMANTICS.md):
    relu((1 - beta) S + beta S W^T),  S = (1 - alpha) P h + alpha h0,  beta = log(lamda / layer + 1),  P = D_in^-1/2 A D_out^-1/2.
    ONE parameter, `weight` [hidden, hidden] (nn.Linear orientation, no bias), uniform(-1 / sqrt(hidden), 1 / sqrt(hidden)) as in the
    paper's released code.  `layer` is 1-based.  No dropout of its own: the encoder (models.GCNII) owns the dropout sites."""

    def __init__(self, hidden, layer, alpha=0.1, lamda=0.5):
        super().__init__()
        if int(hidden) > ops.GCNII_MAX_HIDDEN:
            raise NotImplementedError(f"GCNIIConv: GCNII hidden widths of at most {ops.GCNII_MAX_HIDDEN} (the fused kernel's tile; got {hidden})")
        if int(hidden) < 1 or int(layer) < 1:
            raise ValueError(f"GCNIIConv: hidden and layer must be >= 1 (got {hidden}, {layer})")
        self.hidden, self.layer, self.alpha, self.lamda = int(hidden), int(layer), float(alpha), float(lamda)
        self.weight = nn.Parameter(torch.empty(self.hidden, self.hidden, dtype=torch.float32))
        self.reset_parameters()

    @property
    def beta(self):
        return math.log(self.lamda / self.layer + 1.0)

    def reset_parameters(self):
        b = 1.0 / math.sqrt(self.hidden)
        nn.init.uniform_(self.weight, -b, b)

    def forward(self, graph, feat, h0):
        """feat = H_{l-1}, h0 = H_0 (both [n, hidden]).  Differentiable in training mode when feat IS h0 (a one-layer stack); deeper
        stacks differentiate as a whole (models.GCNII -> autograd.gcnii_stack), so a layer in the middle runs without a graph."""
        _whole_graph_only(graph, feat, "GCNIIConv", "GCNII runs on the whole graph")
        if feat is h0:
            return gcnii_stack(graph, h0, [self.weight], self.alpha, [self.beta], 0.0, self.training)[0]
        if _differentiable(self.training, feat, h0, self.weight):
            raise NotImplementedError("GCNIIConv: a GCNII layer behind another one is differentiated by the whole stack "
                                      "(glnn_amd.autograd.gcnii_stack); call it under torch.no_grad()")
        in_norm, out_norm = graph.degree_norms()
        return ops.gcnii_layer(graph.indptr, graph.indices, graph.num_edges(), feat, h0, self.weight, self.alpha, self.beta, in_norm,
                               x_norm=out_norm)


class PNAConv(nn.Module):
    """Principal Neighbourhood Aggregation (Corso et al., NeurIPS 2020; docs/PNA_SEMANTICS.md): PyG's PNAConv with towers=1,
    pre_layers=1, post_layers=1, divide_input=False, no edge features, aggregators [mean, min, max, std], scalers [identity,
    amplification, attenuation] and without its trailing `lin` (two consecutive Linear maps are one).  Parameters, in registration order,
    torch's default Linear initialisation: pre = Linear(2 in, in) over [x_i || x_j] (destination first), post = Linear(13 in, out) over
    [x || T].  delta > 0 is a constant of the model (the mean of log(deg + 1) over the training graph), not a parameter.  feat_drop: the
    dropout of the layer's input, which both uses of it see; activation: None or ReLU (the scale launch's epilogue).  A row without
    in-edges is legal: its aggregate is [0 | 0 | 0 | sqrt(1e-5)]."""

    def __init__(self, in_feats, out_feats, delta, feat_drop=0.0, activation=None):
        super().__init__()
        if int(in_feats) > ops.PNA_MAX_WIDTH:
            raise NotImplementedError(f"PNAConv: PNA rows of at most {ops.PNA_MAX_WIDTH} columns (one float4 lane row; got in_feats {in_feats})")
        if int(in_feats) < 1 or int(out_feats) < 1:
            raise ValueError(f"PNAConv: in_feats and out_feats must be >= 1 (got {in_feats}, {out_feats})")
        if not float(delta) > 0:
            raise ValueError(f"PNAConv: PNA's delta must be positive (got {delta})")
        if activation is not None and activation is not torch.nn.functional.relu and getattr(activation, "__name__", "") != "relu":
            raise NotImplementedError("PNAConv: the activation must be None or ReLU (the scale launch's epilogue)")
        self.in_feats, self.out_feats, self.delta = int(in_feats), int(out_feats), float(delta)
        self.activation = activation
        self.feat_drop = nn.Dropout(feat_drop)
        self.pre = nn.Linear(2 * self.in_feats, self.in_feats)
        self.post = nn.Linear(13 * self.in_feats, self.out_feats)

    def reset_parameters(self):
        self.pre.reset_parameters()
        self.post.reset_parameters()

    def forward(self, graph, feat):
        _whole_graph_only(graph, feat, "PNAConv", "the PNA teacher runs on the whole graph")
        return pna_conv(graph, feat, self.pre.weight, self.pre.bias, self.post.weight, self.post.bias, self.delta,
                        self.activation is not None, self.feat_drop.p, self.training)
