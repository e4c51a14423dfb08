"""The reference's model zoo surface (reference models.py) on the HIP hot path.

Kept byte-for-byte: class names, constructor arguments, `forward` return conventions ((h_list, h)),
`Model(conf)` substring dispatch ("MLP" tested first, models.py:355,409), `Model.forward /
forward_fitnet / inference`, and state_dict key names (encoder.layers.{i}.weight|bias |
.fc_neigh.weight|bias, encoder.norms.{i}.*).  What changed is where the arithmetic runs: every
Linear / SAGEConv / GraphConv / BatchNorm(eval) / ReLU goes through libglnn_hip.so.

APPNP (an ablation teacher, models.py:282-344) runs its MLP trunk on the same kernels and its K-step propagation on
csrc/appnp.hip (docs/APPNP_SEMANTICS.md).  GAT (models.py:202-279) runs its edge-softmax attention on csrc/gat.hip
(docs/GAT_SEMANTICS.md): every encoder the reference can name is on the HIP path."""
import contextlib
import os
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .autograd import appnp_propagate, gcnii_stack, linear_fn, norm_act_drop
from .kinds import BY_KIND, FULL_GRAPH_KINDS, teacher_kind      # noqa: F401  (the table of kinds; re-exported for the callers of old)
from .nn import DAGNNConv, GATConv, GATv2Conv, GCNIIConv, GPRConv, GraphConv, PNAConv, SAGEConv, TransformerConv, _whole_graph_only


# the activation storages of SAGE.inference(dtype=...) and what the messages call them
_STORAGE = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.int8: "int8"}


def _bn_eval_fold(bn, bias):
    """Per-column (scale, shift) of  BN_eval(x + bias):  y = x*s + ((bias - rm)*s + beta), s = gamma/sqrt(rv+eps)."""
    s = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
    b = bias.detach() if bias is not None else 0.0
    return s.contiguous(), ((b - bn.running_mean) * s + bn.bias.detach()).contiguous()


def _need_hip(x, what):
    if not x.is_cuda:
        raise _lib.GlnnError(f"{what}: tensors must live on the GPU -- this package computes on libglnn_hip.so only, there is no "
                             "CPU path (the reference's default --device -1 selects the CPU: pass --device 0)")


def _check_tail(module):
    """The hidden-layer tails implemented on HIP: BatchNorm1d / LayerNorm with the reference's defaults or no norm, ReLU, dropout."""
    if module.norm_type not in ("none", "batch", "layer"):
        raise NotImplementedError(f"norm_type {module.norm_type!r}: the reference builds 'none', 'batch' or 'layer' (models.py:28-31)")
    act = getattr(module, "activation", F.relu)
    if act is not F.relu and getattr(act, "__name__", "") != "relu":
        raise NotImplementedError("only ReLU hidden activations (what the reference constructs, models.py:371,381)")
    agg = getattr(module, "aggregator_type", None)
    if agg is not None:
        # a SAGE encoder: every path below dispatches on the encoder's aggregator, so the layers must all be of that kind -- a "mean" layer
        # (separate fc_self) must never run through the "gcn" engine, which would silently drop its self weight
        if agg not in ("gcn", "mean"):
            raise NotImplementedError(f"SAGE aggregator_type {agg!r}: 'gcn' (the reference's, models.py:84-99) or 'mean'")
        if any(getattr(lay, "_aggre_type", "gcn") != agg for lay in module.layers):
            raise NotImplementedError(f"SAGE(aggregator_type={agg!r}): every SAGEConv layer must use that aggregator")
    for bn in module.norms:
        if isinstance(bn, nn.LayerNorm):
            if not bn.elementwise_affine or len(bn.normalized_shape) != 1:
                raise NotImplementedError("nn.LayerNorm(hidden_dim) with the reference's defaults (elementwise affine)")
        elif not (bn.affine and bn.track_running_stats and bn.momentum is not None):
            raise NotImplementedError("BatchNorm1d with the reference's defaults (affine, running stats, momentum 0.1)")


def _norm_of(module, l):
    return module.norms[l] if module.norm_type != "none" else None


def drop_hash(seed, row, col):
    """csrc/glnn_common.h's drop_hash on host integers: lowbias32 of seed ^ row * 0x9E3779B1 ^ (col * 0x85EBCA77 + 0x632BE5AB), mod 2^32."""
    m = 0xFFFFFFFF
    h = ((int(seed) & m) ^ (int(row) * 0x9E3779B1 & m) ^ ((int(col) * 0x85EBCA77 + 0x632BE5AB) & m)) & m
    h ^= h >> 16
    h = h * 0x7FEB352D & m
    h ^= h >> 15
    h = h * 0x846CA68B & m
    return h ^ (h >> 16)


SAMPLE_SEED_SALT = 0xFA17


def sample_layer_seed(sample_seed, l):
    """The seed layer l's sampled graph is drawn under in SAGE.inference(fan_out=..., sample_seed=...): drop_hash(sample_seed, l, 0xFA17).
    Each layer draws independently, as dgl's multi-layer sampler does (docs/SAMPLED_INFERENCE_SEMANTICS.md)."""
    return drop_hash(sample_seed, l, SAMPLE_SEED_SALT)


def _eval_tail(module, l, z, relu=True):
    """Eval-mode `norms[l] -> relu -> dropout` of a hidden layer on a materialised z (relu=False: GCN's `norms[l] -> dropout`):
    one glnn_act_fwd_f32 / glnn_norm_drop_fwd_f32 / glnn_layernorm_fwd_f32."""
    if module.norm_type == "batch":
        a_scale, a_shift = _bn_eval_fold(module.norms[l], None)
        return ops.act_fwd(z, a_scale, a_shift, relu=relu)
    if module.norm_type == "layer":
        ln = module.norms[l]
        return ops.layernorm_fwd(z, ln.weight.detach(), ln.bias.detach(), eps=ln.eps, relu=relu, want_stats=False)[0]
    return ops.act_fwd(z) if relu else z


class MLP(nn.Module):
    """reference models.py:7-53"""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, norm_type="none"):
        super().__init__()
        self.num_layers = num_layers
        self.norm_type = norm_type
        self.dropout = nn.Dropout(dropout_ratio)
        self.layers = nn.ModuleList()
        self.norms = nn.ModuleList()
        if num_layers == 1:
            self.layers.append(nn.Linear(input_dim, output_dim))
        else:
            self.layers.append(nn.Linear(input_dim, hidden_dim))
            self._add_norm(hidden_dim)
            for _ in range(num_layers - 2):
                self.layers.append(nn.Linear(hidden_dim, hidden_dim))
                self._add_norm(hidden_dim)
            self.layers.append(nn.Linear(hidden_dim, output_dim))

    def _add_norm(self, hidden_dim):
        if self.norm_type == "batch":
            self.norms.append(nn.BatchNorm1d(hidden_dim))
        elif self.norm_type == "layer":
            self.norms.append(nn.LayerNorm(hidden_dim))

    def forward(self, feats):
        _need_hip(feats, "MLP.forward")
        _check_tail(self)
        if not self.training:
            with torch.no_grad():
                return self._forward_hip_eval(feats)
        h = feats
        h_list = []
        for l, layer in enumerate(self.layers):
            h = linear_fn(h, layer.weight, layer.bias)
            if l != self.num_layers - 1:
                h_list.append(h)
                # norm -> relu -> dropout as one differentiable HIP op (same module state: running stats, affine)
                h = norm_act_drop(h, _norm_of(self, l), self.dropout.p)
        return h_list, h

    def _forward_hip_eval(self, feats, want_hidden=True):
        """Eval-mode chain: each Linear is one glnn_gemm_f32 (dropout is the identity in eval mode).
        want_hidden (what `MLP.forward` returns: h_list = the raw Linear outputs, reference models.py:44-53): BN(eval)+ReLU of
        layer l are folded into the OPERAND LOAD of layer l+1, so z_l is stored exactly as the reference returns it.
        Otherwise (Model.forward / inference / evaluate: only the logits are used) they go into the EPILOGUE of layer l itself,
        relu((x W^T) s + (b s + t)): the next GEMM then reads a plain operand and takes the pipelined kernel -- the 2048-wide
        middle layer of MLP3w8 over millions of rows is the whole cost of evaluating / serving the student."""
        h = ops.as_feat(feats)
        h_list = []
        a_scale = a_shift = None
        if self.norm_type == "layer":          # per-ROW statistics cannot ride in a GEMM's per-column operand transform / epilogue
            for l, layer in enumerate(self.layers):
                z = ops.gemm(h, layer.weight, ep_shift=layer.bias)
                if l != self.num_layers - 1:
                    if want_hidden:
                        h_list.append(z)
                    z = _eval_tail(self, l, z)
                h = z
            return h_list, h
        for l, layer in enumerate(self.layers):
            last = l == self.num_layers - 1
            if want_hidden or last:
                z = ops.gemm(h, layer.weight, a_scale=a_scale, a_shift=a_shift, ep_shift=layer.bias)
            else:
                if self.norm_type == "batch":
                    s, t = _bn_eval_fold(self.norms[l], layer.bias)      # BN_eval(x + bias) = x s + t
                    z = ops.gemm(h, layer.weight, ep_scale=s, ep_shift=t, relu=True)
                else:
                    z = ops.gemm(h, layer.weight, ep_shift=layer.bias, relu=True)
            if not last and want_hidden:
                h_list.append(z)
                if self.norm_type == "batch":
                    a_scale, a_shift = _bn_eval_fold(self.norms[l], None)
                else:
                    a_scale = torch.ones(z.shape[1], device=z.device)
                    a_shift = torch.zeros(z.shape[1], device=z.device)
            h = z
        return h_list, h


class SAGE(nn.Module):
    """reference models.py:62-148"""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none", aggregator_type="gcn"):
        """aggregator_type: "gcn" (what the reference builds) or "mean" (dgl's default SAGE form with a separate fc_self,
        docs/SAGE_MEAN_SEMANTICS.md); anything else raises in SAGEConv."""
        super().__init__()
        self.num_layers = num_layers
        self.hidden_dim = hidden_dim
        self.output_dim = output_dim
        self.norm_type = norm_type
        self.activation = activation
        self.aggregator_type = aggregator_type
        self.dropout = nn.Dropout(dropout_ratio)
        self.layers = nn.ModuleList()
        self.norms = nn.ModuleList()
        if num_layers == 1:
            self.layers.append(SAGEConv(input_dim, output_dim, aggregator_type))
        else:
            self.layers.append(SAGEConv(input_dim, hidden_dim, aggregator_type))
            self._add_norm(hidden_dim)
            for _ in range(num_layers - 2):
                self.layers.append(SAGEConv(hidden_dim, hidden_dim, aggregator_type))
                self._add_norm(hidden_dim)
            self.layers.append(SAGEConv(hidden_dim, output_dim, aggregator_type))

    def _add_norm(self, hidden_dim):
        if self.norm_type == "batch":
            self.norms.append(nn.BatchNorm1d(hidden_dim))
        elif self.norm_type == "layer":
            self.norms.append(nn.LayerNorm(hidden_dim))

    def forward(self, blocks, feats):
        """Sampled-block forward (reference models.py:101-119): training mode through the differentiable HIP ops of
        glnn_amd.autograd, eval mode on the plain kernels (BatchNorm running stats folded into one activation pass)."""
        _need_hip(feats, "SAGE.forward")
        _check_tail(self)
        h = feats
        h_list = []
        for l, (layer, block) in enumerate(zip(self.layers, blocks)):
            h_dst = h[: block.num_dst_nodes()]
            if self.training:
                h = layer(block, (h, h_dst))
                if l != self.num_layers - 1:
                    h_list.append(h)
                    h = norm_act_drop(h, _norm_of(self, l), self.dropout.p)
            else:
                with torch.no_grad():
                    h = layer(block, (h, h_dst))
                    if l != self.num_layers - 1:
                        h_list.append(h)
                        h = _eval_tail(self, l, h)
        return h_list, h

    CHAIN_NEXT_PROJECTION = True      # A/B switch of the chained projection in `inference`
    CACHE_INPUT_AGGREGATE = True      # A/B switch of the kept layer-1 neighbour aggregate in `inference` (_input_aggregate)

    def _tail(self, l):
        """Fused eval tail of layer l: (ep_scale, ep_shift, relu) = BN(eval) o (+bias) o ReLU; dropout is a no-op."""
        mean = self.aggregator_type == "mean"
        bias = self.layers[l].mean_bias() if mean else self.layers[l].fc_neigh.bias      # ("mean": fc_self.bias + fc_neigh.bias)
        if l == self.num_layers - 1:
            return None, bias, False
        if self.activation is not F.relu and getattr(self.activation, "__name__", "") != "relu":
            raise NotImplementedError("SAGE.inference: the reference always passes activation=F.relu (models.py:371)")
        if self.norm_type == "batch":
            # the fold is five small launches per layer: remembered while the BatchNorm's tensors and the bias are unmodified (torch's
            # version counters + ops.PARAM_EPOCH, which this library's raw-pointer writers bump)
            bn = self.norms[l]
            ts = (bn.weight, bn.bias, bn.running_mean, bn.running_var) + ((bias,) if bias is not None else ())
            if mean and bias is not None:      # (the summed bias is a derived tensor: key on the two parameters it came from)
                ts = ts[:-1] + (self.layers[l].fc_self.bias, self.layers[l].fc_neigh.bias)
            key = (ops.PARAM_EPOCH, bn.eps) + tuple((t.data_ptr(), t._version) for t in ts)
            cache = self.__dict__.setdefault("_tail_cache", {})
            ent = cache.get(l)
            if ent is None or ent[0] != key:
                cache[l] = ent = (key,) + _bn_eval_fold(bn, bias)
            return ent[1], ent[2], True
        if self.norm_type == "none":
            return None, bias, True
        raise NotImplementedError("SAGE._tail: LayerNorm has per-row statistics and cannot be folded into a kernel epilogue "
                                  "(SAGE.inference applies it as its own pass; the sharded teachers do not support it)")

    def _layer_tail(self, l):
        """What layer l's launch gets in `inference`: (ep_scale, ep_shift, relu, post_ln).  A LayerNorm hidden layer's launch adds the conv's
        bias only and LayerNorm -> ReLU follow as a pass of their own (post_ln: _eval_tail); every other layer gets the fused `_tail`."""
        if self.norm_type == "layer" and l != self.num_layers - 1:
            return None, self.layers[l].mean_bias() if self.aggregator_type == "mean" else self.layers[l].fc_neigh.bias, False, True
        return self._tail(l) + (False,)

    def _chains_next(self, l):
        """Layer l is fused and layer l+1 projects first: W_{l+1} rides behind l's epilogue and l's rows never reach HBM (products: 2.5 GB)."""
        nxt = self.layers[l + 1] if l + 1 < self.num_layers else None
        return bool(nxt is not None and self.layers[l].fused_eligible() and nxt._in_feats > nxt._out_feats and nxt._out_feats <= 256
                    and SAGE.CHAIN_NEXT_PROJECTION)

    # ---- placement of the matrices the whole-graph launches gather from (ops.placed_for_gather: which allocation holds a matrix
    #      decides whether the gather over it takes 18.1 or 19.4 ms).  Intermediate activations live in buffers that are placed once per
    #      (graph, layer) and reused by every later call -- they are internal: what inference RETURNS is always a fresh tensor; the input
    #      features are copied once into a better allocation if one is found (remembered while the same unmodified tensor comes back).
    def _placed_buffer(self, g, key, rows, d, device, probe=None):
        if not ops.placement_applies(rows, d):
            return None
        cache = self.__dict__.setdefault("_placed", {})
        k = (id(g), key, rows, d, str(device))
        ent = cache.get(k)
        if ent is None or ent[0]() is not g:
            buf = ops.placed_for_gather(rows, d, device, g.indptr, g.indices, g.num_dst_nodes(), what=f"SAGE.inference {key[0]}{key[1]}", zero=True,
                                        probe=probe)
            cache[k] = ent = (weakref.ref(g), buf)
        return ent[1]

    def release_placed(self):
        """Drop the placed buffers this encoder keeps across inference calls (the hidden layers' rows per (graph, layer) and the placed copy
        of the input features, the kept layer-1 aggregate): a long-lived process that is done with a graph gets its memory back."""
        self.__dict__.pop("_placed", None)
        self.__dict__.pop("_placed_x", None)
        self.__dict__.pop("_agg_x", None)
        torch.cuda.empty_cache()

    def _whole_graph_layer(self, l, g, x, projected, place=True, agg=None):
        """Layer l of the whole-graph sweep: (y, projected for layer l+1 or None).  place=False: plain allocations (the launch is being
        used as the PROBE that places the buffer it gathers from -- see _placed_buffer).  agg (layer 0): {"agg_out": m} / {"agg_in": m} of
        _input_aggregate for the fused launch."""
        agg = agg or {}
        layer = self.layers[l]
        if self.aggregator_type != "gcn":
            raise NotImplementedError("SAGE._whole_graph_layer: the chained next-layer projection and the placed buffers belong to the 'gcn' "
                                      f"engine, not to aggregator_type {self.aggregator_type!r}")
        ep_scale, ep_shift, relu, post_ln = self._layer_tail(l)
        n = g.num_dst_nodes()
        nxt = self.layers[l + 1] if l + 1 < self.num_layers else None
        if projected is not None:
            # the dense half of this layer already came out of the previous layer's kernel: aggregate + epilogue only
            return ops.spmm(g.indptr, g.indices, projected, n, ops.AGG_SAGE_GCN, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu), None
        if self._chains_next(l) and not post_ln:      # (LayerNorm sits between the two layers: nothing to chain behind)
            out_next = self._placed_buffer(g, ("proj", l), n, nxt._out_feats, x.device) if place else None
            _, proj = ops.sage_fused(g.indptr, g.indices, x, n, layer.fc_neigh.weight, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu,
                                     x_self=x[:n], w_next=nxt.fc_neigh.weight, want_out=False, tile_order=g.fused_tile_order(),
                                     out_next=out_next, **agg)
            return x, proj                                               # (y is not read: the next layer consumes `proj`)
        out = None
        if place and nxt is not None and not post_ln:
            # a hidden layer's rows are what the next layer gathers from: they go to a placed buffer kept across calls, chosen by timing
            # the NEXT layer's own launch on each candidate allocation
            out = self._placed_buffer(g, ("y", l), n, layer._out_feats, x.device,
                                      probe=lambda cand: self._whole_graph_layer(l + 1, g, cand, None, place=False))
        y = layer(g, (x, x[:n]), ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, out=out, **agg)
        if post_ln:
            y = _eval_tail(self, l, y)
        return y, None

    def _placed_input(self, g, feats, x):
        if not ops.placement_applies(x.shape[0], x.shape[1]) or x.shape[0] < g.num_dst_nodes():
            return x
        ent = self.__dict__.get("_placed_x")
        sig = (id(g), feats.data_ptr(), tuple(feats.shape), feats._version)
        if ent is not None and ent[0]() is feats and ent[1] == sig:
            return ent[2]
        px = ops.place_for_gather(x, g.indptr, g.indices, g.num_dst_nodes(), what="SAGE.inference features")
        self.__dict__["_placed_x"] = (weakref.ref(feats), sig, px)
        return px

    def _input_aggregate(self, g, feats, x):
        """Layer 0 aggregates first in the fused kernel: its gather computes A1 = (A x + x) / (deg+1), which depends on the graph and the
        input features only -- not on any parameter -- and the callers of `inference` (train_and_eval's evaluate once per eval_interval,
        the final soft-label pass) come back with the same graph and the same unmodified `feats` while the weights change.  The first
        forward over a (graph, feats) stores A1 beside its own output (ops.sage_fused(agg_out=...)); later ones read it back instead of
        gathering (agg_in: the same projection code over the same rows, so the same bits).  Remembered under the key of _placed_input --
        the graph and the tensor themselves (weak), its data pointer, shape and in-place version -- and never under the weights.
        Returns (the launch's keyword, the entry to remember once that launch has run or None).  No room (free memory under twice the
        matrix, or the allocation fails): the forward runs as it always did."""
        layer, n = self.layers[0], g.num_dst_nodes()
        if self.aggregator_type != "gcn":
            raise NotImplementedError("SAGE._input_aggregate: the kept layer-1 neighbour aggregate is the 'gcn' aggregate (A x + x)/(deg+1), "
                                      f"not implemented for aggregator_type {self.aggregator_type!r}")
        if not SAGE.CACHE_INPUT_AGGREGATE or not layer.fused_eligible() or x.shape[0] < n or n == 0:
            return {}, None
        try:
            sig = (feats.data_ptr(), tuple(feats.shape), feats._version)
        except RuntimeError:          # tensors created under torch.inference_mode() have no version counter: never kept
            return {}, None
        ent = self.__dict__.get("_agg_x")
        if ent is not None and ent[0]() is g and ent[1]() is feats and ent[2] == sig and ent[3].device == x.device:
            return {"agg_in": ent[3]}, None
        self.__dict__.pop("_agg_x", None)                  # (the stale matrix goes before its successor is allocated)
        try:
            if torch.cuda.mem_get_info(x.device)[0] < 2 * 4 * n * ops.round4(layer._in_feats):
                return {}, None
            buf = ops.feat_empty(n, layer._in_feats, x.device)
        except torch.cuda.OutOfMemoryError:
            return {}, None
        return {"agg_out": buf}, (weakref.ref(g), weakref.ref(feats), sig, buf)

    def _whole_graph_layer_bf16(self, l, g, x, projected):
        """Layer l of the whole-graph sweep with bf16 activation storage: (y, projected for layer l+1 or None).  A matrix is stored as bf16
        exactly when an aggregation gathers it -- the chained projection, a project-first layer's x @ W^T, and a hidden layer's output
        when the next layer aggregates first; all sums, MFMA and epilogues are fp32 and the logits come out fp32."""
        layer = self.layers[l]
        if self.aggregator_type != "gcn":
            raise NotImplementedError(f"SAGE bf16 activation storage: 'gcn' aggregator only, not aggregator_type {self.aggregator_type!r}")
        ep_scale, ep_shift, relu = self._tail(l)
        n = g.num_dst_nodes()
        nxt = self.layers[l + 1] if l + 1 < self.num_layers else None
        out_dtype = torch.bfloat16 if nxt is not None and nxt._in_feats <= nxt._out_feats else torch.float32
        if projected is not None:
            return ops.spmm(g.indptr, g.indices, projected, n, ops.AGG_SAGE_GCN, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu,
                            out_dtype=out_dtype), None
        if self._chains_next(l):
            _, proj = ops.sage_fused(g.indptr, g.indices, x, n, layer.fc_neigh.weight, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu,
                                     x_self=x[:n], w_next=nxt.fc_neigh.weight, want_out=False, tile_order=g.fused_tile_order(),
                                     out_next_dtype=torch.bfloat16)
            return None, proj
        return layer.forward_bf16(g, x, x[:n], ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, out_dtype=out_dtype), None

    def _inference_bf16(self, dataloader, feats, whole_graph):
        g = getattr(dataloader, "graph", None)
        if not whole_graph or g is None:
            raise NotImplementedError("SAGE.inference(dtype=torch.bfloat16): the whole-graph sweep only (whole_graph=True over a loader with a "
                                      "resident graph); the chunked and literal sweeps are fp32")
        if self.norm_type == "layer":
            raise NotImplementedError("SAGE.inference(dtype=torch.bfloat16): LayerNorm teachers are fp32 only (the per-row statistics pass "
                                      "is not part of the bf16 storage path)")
        with torch.no_grad():
            first = self.layers[0]
            if first._in_feats <= first._out_feats:         # layer 0 aggregates its input features: they are gathered, so bf16
                x = ops.as_bf16_feat(feats) if feats.dtype == torch.bfloat16 else ops.to_bf16(feats)
            else:                                           # layer 0 projects first: only its fp32 GEMM reads them
                x = feats.float() if feats.dtype == torch.bfloat16 else feats
            projected = None
            for l in range(self.num_layers):
                x, projected = self._whole_graph_layer_bf16(l, g, x, projected)
            return x

    def _check_i8(self):
        """The refusals of int8 activation storage that depend on the encoder alone, before anything is launched."""
        if self.aggregator_type != "gcn":
            raise NotImplementedError("SAGE.inference(dtype=torch.int8): int8 activation storage is implemented for the 'gcn' aggregator "
                                      f"only, not for aggregator_type {self.aggregator_type!r}")
        if self.norm_type == "layer":
            raise NotImplementedError("SAGE.inference(dtype=torch.int8): LayerNorm teachers are fp32 only (the per-row statistics pass "
                                      "is not part of the int8 storage path)")
        for l, layer in enumerate(self.layers):
            gathered = min(layer._in_feats, layer._out_feats)
            if gathered > ops.I8_MAX_WIDTH:
                form = "aggregates first" if layer._in_feats <= layer._out_feats else "projects first"
                raise NotImplementedError(f"SAGE.inference(dtype=torch.int8): layer {l} {form} and gathers rows of {gathered} columns; int8 "
                                          f"rows hold at most {ops.I8_MAX_WIDTH} (dtype=torch.bfloat16 takes any width)")

    def _input_i8(self, feats):
        """What layer 0 reads in the int8 sweep: int8 rows when it aggregates first (fp32 / bf16 features quantised once per call, rows
        made by ops.to_int8_rows taken as they are), the fp32 features when it projects first (only its GEMM reads them)."""
        first = self.layers[0]
        if feats.dtype == torch.int8:
            if first._in_feats > first._out_feats:
                raise ValueError("SAGE.inference(dtype=torch.int8): layer 0 projects first and its fp32 GEMM reads the features; pass them "
                                 "as float32 or bfloat16, not as int8 rows")
            if feats.dim() != 2 or feats.shape[1] != ops.int8_rows_ld(first._in_feats):
                raise ValueError(f"SAGE.inference(dtype=torch.int8): int8 features must be the rows of ops.to_int8_rows for {first._in_feats} "
                                 f"columns, {ops.int8_rows_ld(first._in_feats)} bytes each (round16(d + 4))")
            return feats
        x = feats.float() if feats.dtype == torch.bfloat16 else feats
        return ops.to_int8_rows(x) if first._in_feats <= first._out_feats else x

    def _whole_graph_layer_i8(self, l, g, x, projected):
        """Layer l of the whole-graph sweep with int8 activation storage: (y, projected for layer l+1 or None).  A matrix is int8 rows
        exactly where the bf16 sweep stores bf16 -- the chained projection, a project-first layer's x @ W^T, and a hidden layer's output
        when the next layer aggregates first; all sums, MFMA and epilogues are fp32 and the logits come out fp32.  The fused launch writes
        fp32, so its chained projection (or its output, when the next layer gathers it) is quantised by a launch of its own."""
        layer = self.layers[l]
        ep_scale, ep_shift, relu = self._tail(l)
        n = g.num_dst_nodes()
        nxt = self.layers[l + 1] if l + 1 < self.num_layers else None
        out_dtype = torch.int8 if nxt is not None and nxt._in_feats <= nxt._out_feats else torch.float32
        if projected is not None:
            return ops.spmm_sage_gcn_i8(g.indptr, g.indices, projected, layer._out_feats, n, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu,
                                        out_dtype=out_dtype), None
        if self._chains_next(l):
            _, proj = ops.sage_fused_i8(g.indptr, g.indices, x, layer._in_feats, n, layer.fc_neigh.weight, ep_scale=ep_scale,
                                        ep_shift=ep_shift, relu=relu, x_self=x[:n], w_next=nxt.fc_neigh.weight, want_out=False,
                                        tile_order=g.fused_tile_order())
            return None, ops.to_int8_rows(proj)
        return layer.forward_i8(g, x, x[:n], ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, out_dtype=out_dtype), None

    def _inference_i8(self, dataloader, feats, whole_graph):
        g = getattr(dataloader, "graph", None)
        if not whole_graph or g is None:
            raise NotImplementedError("SAGE.inference(dtype=torch.int8): the whole-graph sweep only (whole_graph=True over a loader with a "
                                      "resident graph); the chunked and literal sweeps are fp32")
        self._check_i8()
        with torch.no_grad():
            x, projected = self._input_i8(feats), None
            for l in range(self.num_layers):
                x, projected = self._whole_graph_layer_i8(l, g, x, projected)
            return x

    def _inference_mean(self, dataloader, feats, whole_graph, dtype):
        """`inference` of a "mean" encoder, fp32: per layer ONE launch over all rows of the resident CSR (whole_graph) or one per chunk of
        the loader's sweep over global-id row ranges (the same kernels on the same rows: bit-identical), the tail as in `_tail` with the
        summed bias, LayerNorm as its own pass behind the conv.  The "gcn" engine's extras -- the chained next-layer projection, the kept
        layer-1 aggregate, bf16 storage -- are not implemented for this aggregator and raise when asked for."""
        if dtype != torch.float32:
            raise NotImplementedError(f"SAGE.inference(dtype={dtype}): {_STORAGE[dtype]} activation storage is implemented for the 'gcn' "
                                      "aggregator only, not for aggregator_type 'mean'")
        g = getattr(dataloader, "graph", None)
        # whole graph: any loader that sweeps every node of a resident graph in id order (FullNeighborLoader, or the NodeDataLoader the
        # teacher CLI evaluates with: it carries `.graph` exactly then); the chunked sweep also needs the loader's global-id blocks
        if g is None or not (whole_graph or hasattr(dataloader, "global_blocks")):
            raise NotImplementedError("SAGE.inference(aggregator_type 'mean'): a glnn_amd.graph.FullNeighborLoader over the resident graph")
        with torch.no_grad():
            x = ops.as_feat(feats)
            n = g.num_dst_nodes()
            for l, layer in enumerate(self.layers):
                tail = self._layer_tail(l)
                if whole_graph:
                    y = layer(g, (x, x[:n]), ep_scale=tail[0], ep_shift=tail[1], relu=tail[2])
                else:
                    y = ops.feat_empty(n, layer._out_feats, x.device, zero=True)
                    self._mean_engine_layer(l, dataloader, x, y, tail)
                x = _eval_tail(self, l, y) if tail[3] else y
            return x

    def _mean_engine_layer(self, l, dataloader, x, y, tail):
        """Layer l of the "mean" chunked sweep into y: one launch per chunk on the caller's stream, in the layer's own form."""
        layer, form = self.layers[l], self.layers[l].mean_form()
        ep_scale, ep_shift, relu, _ = tail
        wn, ws, d, r4 = layer.fc_neigh.weight, layer.fc_self.weight, layer._out_feats, ops.round4(layer._out_feats)
        if form == "project":
            p = ops.gemm(x, ops.stack_weight_pair(wn, ws))      # a layer that projects first projects x ONCE, not once per chunk
            chunk = lambda s, e, block: ops.spmm_sage_mean(block.indptr, block.indices, p[:, :d], p[s:e, r4:], e - s, ep_scale=ep_scale,
                                                           ep_shift=ep_shift, relu=relu, out=y[s:e])
        else:
            wp = ops.pack_weight_pair(wn, ws) if form == "fused" else None
            chunk = lambda s, e, block: layer(block, (x, x[s:e]), ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, w_packed=wp, out=y[s:e])
        with _chunk_sweep(dataloader, x.device, []) as chunks:
            for _, s, e, block in chunks:
                chunk(s, e, block)

    def _check_fan_out(self, fan_out, dataloader, whole_graph):
        """The refusals of `inference(fan_out=...)`, each naming fan_out; returns the fan-outs as a list of ints."""
        if isinstance(fan_out, (str, bytes)) or not hasattr(fan_out, "__len__"):
            raise ValueError(f"SAGE.inference: fan_out must be a list of {self.num_layers} integers, one per layer (got {fan_out!r})")
        fan_out = list(fan_out)
        if len(fan_out) != self.num_layers:
            raise ValueError(f"SAGE.inference: fan_out names {len(fan_out)} layers, the encoder has {self.num_layers} (got {fan_out!r})")
        for f in fan_out:
            if isinstance(f, bool) or not isinstance(f, int):
                raise ValueError(f"SAGE.inference: fan_out must hold integers (got {f!r} in {fan_out!r})")
            if not 1 <= f <= 64:
                raise ValueError(f"SAGE.inference: every fan_out value must be in [1, 64] (got {f} in {fan_out!r})")
        if not whole_graph:
            raise NotImplementedError("SAGE.inference(fan_out=...): the whole-graph sweep only (whole_graph=True); the chunked and literal "
                                      "sweeps are full-neighbour")
        if getattr(dataloader, "graph", None) is None:
            raise NotImplementedError("SAGE.inference(fan_out=...): a loader over a resident graph (one that sweeps every node in id order "
                                      "and carries `.graph`); this one has none")
        return fan_out

    def inference_over(self, graphs, feats, dtype=torch.float32):
        """The whole-graph forward with layer l aggregating over graphs[l] (CSRGraphs of the same rows: what `inference(fan_out=...)` runs
        over the sampled graphs).  The kernels and forms of the full-neighbour sweep, and none of its state: plain allocations, no placed
        buffers, no placement by trial, no kept layer-1 aggregate -- nothing is read from or written to the encoder's caches."""
        _need_hip(feats, "SAGE.inference_over")
        if len(graphs) != self.num_layers:
            raise ValueError(f"SAGE.inference_over: {len(graphs)} graphs for {self.num_layers} layers")
        if dtype not in _STORAGE:
            raise ValueError(f"SAGE.inference_over: dtype must be torch.float32, torch.bfloat16 or torch.int8, not {dtype}")
        mean = self.aggregator_type != "gcn"
        if mean:
            _check_tail(self)
            if dtype != torch.float32:
                raise NotImplementedError(f"SAGE.inference(dtype={dtype}): {_STORAGE[dtype]} activation storage is implemented for the 'gcn' "
                                          "aggregator only, not for aggregator_type 'mean'")
        elif dtype == torch.bfloat16 and self.norm_type == "layer":
            raise NotImplementedError("SAGE.inference(dtype=torch.bfloat16): LayerNorm teachers are fp32 only (the per-row statistics pass "
                                      "is not part of the bf16 storage path)")
        elif dtype == torch.int8:
            self._check_i8()
        with torch.no_grad():
            if mean:
                x = ops.as_feat(feats)
                for l, (layer, g) in enumerate(zip(self.layers, graphs)):
                    tail = self._layer_tail(l)
                    y = layer(g, (x, x[:g.num_dst_nodes()]), ep_scale=tail[0], ep_shift=tail[1], relu=tail[2])
                    x = _eval_tail(self, l, y) if tail[3] else y
                return x
            projected = None
            if dtype == torch.bfloat16:
                first = self.layers[0]             # (as _inference_bf16: gathered features are bf16, projected-first ones stay fp32)
                if first._in_feats <= first._out_feats:
                    x = ops.as_bf16_feat(feats) if feats.dtype == torch.bfloat16 else ops.to_bf16(feats)
                else:
                    x = feats.float() if feats.dtype == torch.bfloat16 else feats
                for l, g in enumerate(graphs):
                    x, projected = self._whole_graph_layer_bf16(l, g, x, projected)
                return x
            if dtype == torch.int8:
                x = self._input_i8(feats)
                for l, g in enumerate(graphs):
                    x, projected = self._whole_graph_layer_i8(l, g, x, projected)
                return x
            x = ops.as_feat(feats)
            for l, g in enumerate(graphs):
                x, projected = self._whole_graph_layer(l, g, x, projected, place=False)
            return x

    def sampled_graphs(self, g, fan_out, sample_seed=0):
        """[g.sampled(fan_out[l], seed_l)] with seed_l = sample_layer_seed(sample_seed, l): one independent draw per layer."""
        return [g.sampled(f, sample_layer_seed(sample_seed, l)) for l, f in enumerate(fan_out)]

    def inference(self, dataloader, feats, whole_graph=True, dtype=torch.float32, fan_out=None, sample_seed=0):
        """Layer-wise full-neighbour inference (reference models.py:121-148).

        `dataloader` is a glnn_amd.graph.FullNeighborLoader.  whole_graph=True aggregates every destination row
        of a layer in ONE launch over the resident CSR (each dst row is independent, so the result is identical
        to the chunked sweep); whole_graph=False walks the chunks exactly like the reference does
        (gather input rows -> block conv -> fused BN/ReLU -> scatter).

        dtype=torch.bfloat16: the whole-graph sweep with bf16 activation STORAGE (_whole_graph_layer_bf16) -- the gathered matrices move
        half the bytes; arithmetic stays fp32 and the returned logits are fp32.  `feats` may be fp32 (cast once per call) or bf16.  Its
        buffers are plain allocations (no ops.placed_for_gather placement).  Not for whole_graph=False or LayerNorm teachers.

        dtype=torch.int8 (docs/INT8_INFERENCE_SEMANTICS.md): the same sweep with the gathered matrices stored as int8 rows with one fp32
        scale per row (_whole_graph_layer_i8); weights, arithmetic and the returned logits are fp32.  `feats` may be fp32 or bf16 (quantised
        once per call) or rows already made by ops.to_int8_rows.  The bf16 form's refusals, and gathered rows of at most 256 columns.

        fan_out=[f_0, .., f_{L-1}] (docs/SAMPLED_INFERENCE_SEMANTICS.md): neighbour-sampled inference -- layer l aggregates over
        g.sampled(f_l, sample_layer_seed(sample_seed, l)), at most f_l uniformly drawn in-edges per row, through `inference_over`: both
        aggregators, bf16 storage where the full form has it, and none of the full form's caches.  fan_out=None: the full-neighbour code
        path, call for call."""
        if fan_out is not None:
            fan_out = self._check_fan_out(fan_out, dataloader, whole_graph)
            _need_hip(feats, "SAGE.inference")
            return self.inference_over(self.sampled_graphs(dataloader.graph, fan_out, sample_seed), feats, dtype)
        _need_hip(feats, "SAGE.inference")
        if dtype not in _STORAGE:
            raise ValueError(f"SAGE.inference: dtype must be torch.float32, torch.bfloat16 or torch.int8, not {dtype}")
        if self.aggregator_type != "gcn":
            _check_tail(self)
            return self._inference_mean(dataloader, feats, whole_graph, dtype)
        if dtype == torch.bfloat16:
            return self._inference_bf16(dataloader, feats, whole_graph)
        if dtype == torch.int8:
            return self._inference_i8(dataloader, feats, whole_graph)
        g = getattr(dataloader, "graph", None)
        with torch.no_grad():
            x = ops.as_feat(feats)
            if not whole_graph or g is None:                  # (a loader without a resident graph does not sweep arange(N))
                return self._inference_chunked(dataloader, x)
            x = self._placed_input(g, feats, x)
            agg, agg_ent = self._input_aggregate(g, feats, x)
            projected = None          # x @ W_l^T handed over by the previous (fused) layer when layer l projects first
            for l in range(self.num_layers):
                x, projected = self._whole_graph_layer(l, g, x, projected, agg=agg if l == 0 else None)
                if l == 0 and agg_ent is not None:            # (remembered only once the launch that fills it has been issued)
                    self.__dict__["_agg_x"] = agg_ent
            return x

    def _inference_chunked(self, dataloader, x):
        """The reference's sweep (models.py:129-145): global-id blocks where the loader has them and no LayerNorm follows, else its literal loop."""
        for l, layer in enumerate(self.layers):
            tail = self._layer_tail(l)
            y = ops.feat_empty(x.shape[0], self.hidden_dim if l != self.num_layers - 1 else self.output_dim, x.device, zero=True)
            wp = ops.pack_weight(layer.fc_neigh.weight) if layer.fused_eligible() else None     # once per layer, not per chunk
            engine = hasattr(dataloader, "global_blocks") and not tail[3]
            (self._engine_layer if engine else self._literal_layer)(l, dataloader, x, y, tail, wp)
            x = y
        return x

    def _engine_layer(self, l, dataloader, x, y, tail, wp):
        """Layer l over global-id row-range blocks: the conv gathers its source rows from x itself and writes its rows of y (no feats[input_nodes],
        no y[output_nodes] = h), and a layer that projects first projects x once, not per chunk.  Chunks are independent and SHORT (4096 rows:
        128 tiles on 256 CUs), so they go round-robin on SWEEP_STREAMS streams, through ONE prepared call where the layer is a single launch."""
        layer, g = self.layers[l], getattr(dataloader, "graph", None)
        ep_scale, ep_shift, relu, _ = tail
        xp = ops.gemm(x, layer.fc_neigh.weight) if layer._in_feats > layer._out_feats else None
        if g is not None and (xp is not None or layer.fused_eligible()):
            tailed = ep_scale is not None or ep_shift is not None or relu
            launch = (ops.RowRangeLaunch(g.indptr, g.indices, xp, y, ep_scale=ep_scale, ep_shift=ep_shift, relu=relu) if xp is not None else
                      ops.RowRangeLaunch(g.indptr, g.indices, x, y, w=layer.fc_neigh.weight, ep_scale=ep_scale,
                                         ep_shift=ep_shift if tailed else layer.fc_neigh.bias, relu=relu, w_packed=wp))
            chunk = lambda s, e, block: launch(s, e)
        elif xp is not None:
            chunk = lambda s, e, block: ops.spmm(block.indptr, block.indices, xp, e - s, ops.AGG_SAGE_GCN, ep_scale=ep_scale, ep_shift=ep_shift,
                                                 relu=relu, out=y[s:e], x_self=xp[s:e])
        else:
            chunk = lambda s, e, block: layer(block, (x, x[s:e]), ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, w_packed=wp, out=y[s:e])
        with _chunk_sweep(dataloader, x.device, _sweep_streams(x.device)) as chunks:
            for _, s, e, block in chunks:
                chunk(s, e, block)

    def _literal_layer(self, l, dataloader, x, y, tail, wp):
        """Layer l as the reference's loop writes it (models.py:133-145): block build, feats[input_nodes], conv, y[output_nodes] = h."""
        layer, (ep_scale, ep_shift, relu, post_ln) = self.layers[l], tail
        for input_nodes, output_nodes, blocks in dataloader:
            block = blocks[0].int().to(x.device)
            h = ops.gather_rows(x, input_nodes)                              # feats[input_nodes]
            h = layer(block, (h, h[: block.num_dst_nodes()]), ep_scale=ep_scale, ep_shift=ep_shift, relu=relu, w_packed=wp)
            if post_ln:
                h = _eval_tail(self, l, h)
            ops.scatter_rows(h, output_nodes, y)                             # y[output_nodes] = h


@contextlib.contextmanager
def _chunk_sweep(dataloader, device, pool):
    """`with _chunk_sweep(...) as chunks: for k, s, e, block in chunks: <launch rows [s, e)>`: the loader hands out global-id row-range blocks
    for the length of the `with` (switched back also when a chunk raises); chunk k runs with pool[k % len(pool)] as the current stream (an
    empty pool: the caller's); the pool waits for the caller's stream before the first chunk, the caller's for the pool after the last."""
    def chunks():
        for k, (input_nodes, _, blocks) in enumerate(dataloader):
            if input_nodes is not None:
                raise RuntimeError(f"SAGE.inference: {type(dataloader).__name__} has a global_blocks attribute and ignores it: its chunks carry input_nodes")
            s, e = blocks[0].dst_range
            if pool:
                with torch.cuda.stream(pool[k % len(pool)]):
                    yield k, s, e, blocks[0]
            else:
                yield k, s, e, blocks[0]
    cur = torch.cuda.current_stream(device)
    for st in pool:
        st.wait_stream(cur)
    dataloader.global_blocks = True
    it = chunks()
    try:
        yield it
    finally:
        it.close()                # (a chunk that raised left the generator inside its stream context: leave it now, not at collection)
        dataloader.global_blocks = False
    for st in pool:
        cur.wait_stream(st)


SWEEP_STREAMS = int(os.environ.get("GLNN_SWEEP_STREAMS", "8"))      # streams of the engine-mode chunked sweep (<= 1: the caller's stream only)
_SWEEP_POOLS = {}


def _sweep_streams(device):
    if SWEEP_STREAMS <= 1 or device.type != "cuda":
        return []
    key = (device.index, SWEEP_STREAMS)
    if key not in _SWEEP_POOLS:
        _SWEEP_POOLS[key] = [torch.cuda.Stream(device=device) for _ in range(SWEEP_STREAMS)]
    return _SWEEP_POOLS[key]


class GCN(nn.Module):
    """reference models.py:151-199"""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none"):
        super().__init__()
        self.num_layers = num_layers
        self.norm_type = norm_type
        self.dropout = nn.Dropout(dropout_ratio)
        self.layers = nn.ModuleList()
        self.norms = nn.ModuleList()
        if num_layers == 1:
            self.layers.append(GraphConv(input_dim, output_dim, activation=activation))
        else:
            self.layers.append(GraphConv(input_dim, hidden_dim, activation=activation))
            self._add_norm(hidden_dim)
            for _ in range(num_layers - 2):
                self.layers.append(GraphConv(hidden_dim, hidden_dim, activation=activation))
                self._add_norm(hidden_dim)
            self.layers.append(GraphConv(hidden_dim, output_dim))

    def _add_norm(self, hidden_dim):
        if self.norm_type == "batch":
            self.norms.append(nn.BatchNorm1d(hidden_dim))
        elif self.norm_type == "layer":
            self.norms.append(nn.LayerNorm(hidden_dim))

    def forward(self, g, feats):
        """reference models.py:189-199: GraphConv (ReLU inside the conv on hidden layers) -> norms[l] -> dropout (NO ReLU behind
        the norm).  train.conf.yaml's cora-style sections use norm_type none, pokec / penn94 GCN use batch."""
        _need_hip(feats, "GCN.forward")
        _check_tail(self)
        h = feats
        h_list = []
        for l, layer in enumerate(self.layers):
            h = layer(g, h)
            if l != self.num_layers - 1:
                h_list.append(h)
                if self.training:
                    if self.norm_type != "none" or self.dropout.p > 0:
                        h = norm_act_drop(h, _norm_of(self, l), self.dropout.p, relu=False)
                elif self.norm_type != "none":
                    with torch.no_grad():
                        h = _eval_tail(self, l, h, relu=False)
        return h_list, h


class _TrunkProp(MLP):
    """What APPNP and GPRGNN share: the MLP trunk (same layers, norms and state_dict keys), its Linears initialised once more (the
    reference's APPNP does so, models.py:282-344: the RNG stream is kept in step), and forward = self.propagate(g, trunk logits)."""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none"):
        super().__init__(num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, norm_type)
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        for layer in self.layers:
            layer.reset_parameters()

    def forward(self, g, feats):
        h_list, h = super().forward(feats)
        return h_list, self.propagate(g, h)


class APPNP(_TrunkProp):
    """reference models.py:282-344: the trunk followed by dgl APPNPConv(k, alpha, edge_drop) -- K power iterations of personalised-PageRank
    propagation with a fresh edge-dropout mask per iteration in training."""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none", edge_drop=0.5,
                 alpha=0.1, k=10):
        super().__init__(num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type)
        self.k, self.alpha, self.edge_drop = int(k), float(alpha), float(edge_drop)

    def propagate(self, g, h):
        return appnp_propagate(g, h, self.k, self.alpha, self.edge_drop, self.training)


class GPRGNN(_TrunkProp):
    """GPR-GNN (Chien et al., ICLR 2021; docs/GPR_SEMANTICS.md; neither the reference nor dgl 0.6.1 defines it): the trunk followed by
    GPRConv(k, alpha, init) -- K propagation steps over APPNP's operator whose K + 1 mixing coefficients `propagate.gamma` are learned.
    No edge dropout and no dropout in front of the propagation."""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none", k=10, alpha=0.1,
                 init="PPR"):
        super().__init__(num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type)
        self.propagate = GPRConv(k, alpha, init)      # "Random" draws from torch's generator here, after the trunk's layers
        self.k, self.alpha = self.propagate.k, self.propagate.alpha


class DAGNN(_TrunkProp):
    """DAGNN (Liu, Gao, Ji, KDD 2020; docs/DAGNN_SEMANTICS.md; neither the reference nor dgl 0.6.1 defines it): the trunk followed by
    DAGNNConv(k, output_dim) -- K propagation steps over APPNP's operator, each node mixing its K + 1 hops through the learned gate
    `propagate.proj`.  No edge dropout and no dropout in front of the propagation."""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none", k=10):
        super().__init__(num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type)
        self.propagate = DAGNNConv(k, output_dim)     # torch's default Linear initialisation, drawn here, after the trunk's layers
        self.k = self.propagate.k


STACK_MAX_LAYERS = 64


class _ConvStack(nn.Module):
    """What GCNII and PNA share: H_0 = relu(fc_in(drop(x))), num_layers conv layers over hidden_dim columns with a dropout in front of
    each, logits = fc_out(drop(H_L)); forward returns ([H_1..H_L], logits).  A subclass names its width limit and the reasons of its
    refusals (MAX_HIDDEN, WHY = width / norm / ReLU), hands its layers' constructor to __init__ (conv(l), l = 1..num_layers, called
    between fc_in and fc_out: the registration and RNG order) and runs the stack on H_0 (stack(g, h0) -> [H_1..H_L])."""
    MAX_HIDDEN = WHY = None

    def __init__(self, conv, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type):
        super().__init__()
        who, (why_width, why_norm, why_relu) = type(self).__name__, self.WHY
        if hidden_dim > self.MAX_HIDDEN:
            raise NotImplementedError(f"{who}: hidden_dim of at most {self.MAX_HIDDEN} ({why_width}; got {hidden_dim})")
        if norm_type != "none":
            raise NotImplementedError(f"{who}: norm_type 'none' only ({why_norm}; got {norm_type!r})")
        if not 1 <= num_layers <= STACK_MAX_LAYERS:
            raise NotImplementedError(f"{who}: 1 to {STACK_MAX_LAYERS} conv layers (got num_layers {num_layers})")
        if activation is not F.relu and getattr(activation, "__name__", "") != "relu":
            raise NotImplementedError(f"{who}: only the ReLU activation ({why_relu})")
        self.num_layers, self.norm_type, self.activation, self.hidden_dim = num_layers, norm_type, activation, hidden_dim
        self.dropout = nn.Dropout(dropout_ratio)
        self.fc_in = nn.Linear(input_dim, hidden_dim)
        self.layers = nn.ModuleList(conv(l) for l in range(1, num_layers + 1))
        self.fc_out = nn.Linear(hidden_dim, output_dim)

    def forward(self, g, feats):
        who = type(self).__name__
        _need_hip(feats, f"{who}.forward")
        _whole_graph_only(g, feats, who, f"{who} runs on the whole graph")
        if not self.training:
            with torch.no_grad():
                h0 = ops.gemm(ops.as_feat(feats), self.fc_in.weight, ep_shift=self.fc_in.bias, relu=True)
                hs = self.stack(g, h0)
                return hs, ops.gemm(hs[-1], self.fc_out.weight, ep_shift=self.fc_out.bias)
        p = self.dropout.p
        x = norm_act_drop(feats, None, p, relu=False) if p > 0 else feats
        h0 = norm_act_drop(linear_fn(x, self.fc_in.weight, self.fc_in.bias), None, 0.0)
        hs = self.stack(g, h0)
        h = norm_act_drop(hs[-1], None, p, relu=False) if p > 0 else hs[-1]
        return hs, linear_fn(h, self.fc_out.weight, self.fc_out.bias)


class GCNII(_ConvStack):
    """GCNII (Chen, Wei, Huang, Ding, Li, ICML 2020; docs/GCNII_SEMANTICS.md; neither the reference nor dgl 0.6.1 defines it): the stack
    of GCNIIConv layers over H_0 and APPNP's operator."""
    MAX_HIDDEN = ops.GCNII_MAX_HIDDEN
    WHY = ("the fused kernel's tile width", "the paper's model has no norm layers", "the fused layer kernel's epilogue")

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none", alpha=0.1, lamda=0.5):
        super().__init__(lambda l: GCNIIConv(hidden_dim, l, alpha, lamda), num_layers, input_dim, hidden_dim, output_dim, dropout_ratio,
                         activation, norm_type)
        self.alpha, self.lamda = float(alpha), float(lamda)

    def betas(self):
        return [layer.beta for layer in self.layers]

    def stack(self, g, h0):
        return gcnii_stack(g, h0, [layer.weight for layer in self.layers], self.alpha, self.betas(),
                           self.dropout.p if self.training else 0.0, self.training)


class PNA(_ConvStack):
    """PNA (Corso et al., NeurIPS 2020; docs/PNA_SEMANTICS.md; neither the reference nor dgl 0.6.1 defines it) as a stack, so that wide
    input features never reach the gather: PNAConv(hidden, hidden) layers with ReLU, the dropout in front of each being the conv's
    feat_drop.  `delta` is a persistent fp64 buffer: a constant of the model, saved with it and never recomputed on a subgraph or an
    observed graph."""
    MAX_HIDDEN = ops.PNA_MAX_WIDTH
    WHY = ("the aggregation kernel's row width", "BatchNorm / LayerNorm in the PNA stack are out of scope", "the scale launch's epilogue")

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, norm_type="none", delta=1.0):
        if not float(delta) > 0:
            raise ValueError(f"PNA: pna_delta must be positive (got {delta})")
        super().__init__(lambda l: PNAConv(hidden_dim, hidden_dim, delta, dropout_ratio, activation), num_layers, input_dim, hidden_dim,
                         output_dim, dropout_ratio, activation, norm_type)
        self.register_buffer("delta", torch.tensor(float(delta), dtype=torch.float64))
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module._sync_delta())

    def _sync_delta(self):
        """A loaded state_dict brings its own delta: the layers read it as a host float."""
        delta = float(self.delta)
        for layer in self.layers:
            layer.delta = delta

    def stack(self, g, h0):
        hs = [h0]
        for layer in self.layers:
            hs.append(layer(g, hs[-1]))
        return hs[1:]


class _AttnStack(nn.Module):
    """The layer stack GAT, GATv2 and GraphTransformer share (reference models.py:202-279): num_layers convs of class CONV, `num_heads` heads of
    hidden_dim // num_heads features on every hidden layer (ReLU inside the conv, outputs flattened to [N, hidden_dim] and kept in
    h_list), one head of output_dim features on the last.  No norm layers and no dropout outside the convs (feat_drop = dropout_ratio,
    attn_drop).  A subclass names its conv, the tails of its messages and where its conf contract is written (Model.__init__)."""
    CONV = NUM_LAYERS = CONF_DOC = None

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim, dropout_ratio, activation, num_heads=8, attn_drop=0.3,
                 negative_slope=0.2, residual=False):
        super().__init__()
        who, conv = type(self).__name__, self.CONV
        if num_layers <= 1:
            raise NotImplementedError(f"{who}: num_layers must be > 1 ({self.NUM_LAYERS})")
        if residual:
            raise NotImplementedError(f"{who}: residual=True is not implemented ({conv.RESIDUAL})")
        hidden_dim //= num_heads
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.activation = activation
        dims = [input_dim] + [hidden_dim * num_heads] * (num_layers - 1)
        self.layers = nn.ModuleList(conv(d, hidden_dim, num_heads, dropout_ratio, attn_drop, negative_slope, False, activation)
                                    for d in dims[:-1])
        self.layers.append(conv(dims[-1], output_dim, 1, dropout_ratio, attn_drop, negative_slope, False, None))

    def conv_forward(self, l, g, h):
        return self.layers[l](g, h)

    def forward(self, g, feats):
        who = type(self).__name__
        _need_hip(feats, f"{who}.forward")
        if isinstance(g, (list, tuple)):
            raise NotImplementedError(f"{who}: block (bipartite) inputs are not implemented: {self.CONV.WHOLE_GRAPH}")
        h = feats
        h_list = []
        for l in range(self.num_layers):
            h = self.conv_forward(l, g, h)
            if l != self.num_layers - 1:
                h = h.flatten(1)
                h_list.append(h)
            else:
                h = h[:, 0]                    # mean(1) over the last layer's ONE head (models.py:225)
        return h_list, h


class GAT(_AttnStack):
    """reference models.py:202-279 over GATConv (the last layer's mean over one head is a reshape)."""
    CONV = GATConv
    NUM_LAYERS = "the reference asserts it, models.py:218"
    CONF_DOC = "no implicit 8 heads, docs/GAT_SEMANTICS.md"

    def conv_forward(self, l, g, h):
        return self.layers[l](g, h, nonneg=True if l > 0 and self.layers[l - 1].relu() else None)   # a ReLU layer's output is >= 0


class GATv2(_AttnStack):
    """GATv2 (Brody, Alon, Yahav, ICLR 2022; docs/GATV2_SEMANTICS.md; neither the reference nor dgl 0.6.1 defines it) in models.GAT's shape,
    over GATv2Conv."""
    CONV = GATv2Conv
    NUM_LAYERS = "models.GAT's shape: hidden multi-head layers and a one-head last layer"
    CONF_DOC = "docs/GATV2_SEMANTICS.md"


class GraphTransformer(_AttnStack):
    """The graph transformer of UniMP (Shi et al., IJCAI 2021; docs/GT_SEMANTICS.md; neither the reference nor dgl 0.6.1 defines it)
    without its label embedding, in models.GAT's shape, over TransformerConv."""
    CONV = TransformerConv
    NUM_LAYERS = "models.GAT's shape: hidden multi-head layers and a one-head last layer"
    CONF_DOC = "docs/GT_SEMANTICS.md"


_ATTN_STACKS = {"gat": GAT, "gatv2": GATv2, "gt": GraphTransformer}


class Model(nn.Module):
    """Wrapper of different models (reference models.py:347-429).

    GAT confs must name BOTH `num_heads` and `attn_dropout_ratio` (every GAT section of train.conf.yaml does): `num_heads` is honoured
    -- the reference reads only `attn_dropout_ratio` and hard-wires 8 heads, which agrees wherever the reference is configured, since all
    its sections say 8 -- and a conf without either key raises NotImplementedError naming it instead of taking an implicit default.
    hidden_dim must be a positive multiple of num_heads (docs/GAT_SEMANTICS.md)."""

    def __init__(self, conf):
        super().__init__()
        self.model_name = conf["model_name"]
        kind = self.kind
        common = dict(num_layers=conf["num_layers"], input_dim=conf["feat_dim"], hidden_dim=conf["hidden_dim"],
                      output_dim=conf["label_dim"], dropout_ratio=conf["dropout_ratio"])
        if kind == "mlp":
            enc = MLP(norm_type=conf["norm_type"], **common)
        elif kind == "sage":
            enc = SAGE(activation=F.relu, norm_type=conf["norm_type"], aggregator_type=conf.get("sage_aggregator", "gcn"), **common)
        elif kind == "gcnii":
            alpha, lamda = conf.get("gcnii_alpha"), conf.get("gcnii_lamda")          # (absent or None: the paper's defaults)
            enc = GCNII(activation=F.relu, norm_type=conf["norm_type"], alpha=0.1 if alpha is None else alpha,
                        lamda=0.5 if lamda is None else lamda, **common)
        elif kind == "gcn":
            enc = GCN(activation=F.relu, norm_type=conf["norm_type"], **common)
        elif kind == "appnp":
            enc = APPNP(activation=F.relu, norm_type=conf["norm_type"], **common)
        elif kind in _ATTN_STACKS:                   # (the conf contract of GATv2 and GraphTransformer is GAT's)
            cls = _ATTN_STACKS[kind]
            who = cls.__name__
            missing = [k for k in ("num_heads", "attn_dropout_ratio") if k not in conf]
            if missing:
                raise NotImplementedError(f"{conf['model_name']}: the conf does not name {' or '.join(missing)}; {who} is built only from "
                                          f"confs that carry both num_heads and attn_dropout_ratio ({cls.CONF_DOC})")
            heads = int(conf["num_heads"])
            if heads < 1 or conf["hidden_dim"] < heads or conf["hidden_dim"] % heads:
                raise ValueError(f"{who}: hidden_dim ({conf['hidden_dim']}) must be a positive multiple of num_heads ({heads})")
            enc = cls(activation=F.relu, num_heads=heads, attn_drop=conf["attn_dropout_ratio"], **common)
        elif kind == "dagnn":
            k = conf.get("dagnn_k")                                                  # (absent or None: the paper's 10 hops)
            enc = DAGNN(activation=F.relu, norm_type=conf["norm_type"], k=10 if k is None else k, **common)
        elif kind == "pna":
            if conf.get("pna_delta") is None:                                        # (a property of the training graph: no default)
                raise ValueError(f"{conf['model_name']}: the conf does not name pna_delta; a PNA teacher is built only from confs that "
                                 "carry it -- the mean of log(deg + 1) over the training graph, which train_teacher.py computes "
                                 "(docs/PNA_SEMANTICS.md)")
            enc = PNA(activation=F.relu, norm_type=conf["norm_type"], delta=conf["pna_delta"], **common)
        else:
            enc = GPRGNN(activation=F.relu, norm_type=conf["norm_type"], k=conf.get("gpr_k", 10), alpha=conf.get("gpr_alpha", 0.1),
                         init=conf.get("gpr_init", "PPR"), **common)
        self.encoder = enc.to(conf["device"])

    kind = property(lambda self: teacher_kind(self.model_name))

    def forward(self, data, feats):
        """data: a graph `g`, a list of blocks, or None for MLPs."""
        if self.kind == "mlp":
            if not self.encoder.training:           # logits only: the hidden Linear outputs need not be kept raw
                _need_hip(feats, "MLP.forward")
                _check_tail(self.encoder)
                with torch.no_grad():
                    return self.encoder._forward_hip_eval(feats, want_hidden=False)[1]
            return self.encoder(feats)[1]
        return self.encoder(data, feats)[1]

    def forward_fitnet(self, data, feats):
        if self.kind == "mlp":
            return self.encoder(feats)
        return self.encoder(data, feats)

    def inference(self, data, feats, dtype=torch.float32, fan_out=None, sample_seed=0):
        """dtype=torch.bfloat16 / torch.int8: bf16 / int8 activation storage, the SAGE teacher's whole-graph forward only (SAGE.inference).
        fan_out / sample_seed: neighbour-sampled inference, the SAGE teacher only (SAGE.inference; docs/SAMPLED_INFERENCE_SEMANTICS.md)."""
        kind = self.kind
        if fan_out is not None:
            if kind != "sage":
                raise NotImplementedError(f"{self.model_name}.inference(fan_out={fan_out!r}): neighbour-sampled inference is implemented "
                                          "for the SAGE teacher only (the other teachers run on the whole graph)")
            return self.encoder.inference(data, feats, dtype=dtype, fan_out=fan_out, sample_seed=sample_seed)
        if dtype != torch.float32:
            row = BY_KIND[kind]
            what = _STORAGE.get(dtype, "bf16")
            if row.bf16:
                raise NotImplementedError(f"{row.key}.inference(dtype={dtype}): {what} activation storage is not implemented for the {row.key} "
                                          "teacher ({} gathers and stores fp32 rows; {}, {})".format(*row.bf16))
            if kind != "sage":
                raise NotImplementedError(f"{self.model_name}.inference(dtype={dtype}): {what} activation storage is implemented for the SAGE "
                                          "teacher's whole-graph forward only")
            return self.encoder.inference(data, feats, dtype=dtype)
        if kind == "sage":
            return self.encoder.inference(data, feats)
        return self.forward(data, feats)
