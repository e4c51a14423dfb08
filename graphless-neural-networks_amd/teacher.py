"""Teacher TRAINING step on libglnn_hip.so: forward + NLL + backward + Adam as an explicit launch sequence.

One `TeacherEngine.step_sage()` is the loop body of the reference's `train_sage` (reference train_and_eval.py:39-54)

    blocks = [blk.int().to(device) ...]; batch_feats = feats[input_nodes]; logits = model(blocks, batch_feats)
    out = logits.log_softmax(1); loss = criterion(out, labels[output_nodes]); total += loss.item()
    loss *= lamb; optimizer.zero_grad(); loss.backward(); optimizer.step()

and one `step_gcn()` is the reference's full-graph `train` (train_and_eval.py:12-29), with NO autograd graph and NO host
synchronisation:

  SAGE layer l   agg_l = (A_l h_l + h_l[:n_dst]) / (deg+1)          glnn_spmm_csr_f32 (SAGE_GCN); for the OUTERMOST block the
                                                                    gather goes straight into `feats` through the block's
                                                                    global source ids (feats[input_nodes] is never built)
                 z_l = agg_l W_l^T + b_l                            glnn_gemm_f32
                 h_{l+1} = dropout(relu(BN_train(z_l)))             glnn_bn_stats_f32 + glnn_act_fwd_f32
  loss           log_softmax + NLL, d(lamb*loss)/dlogits            glnn_softmax_loss_f32 (labels indexed by output_nodes)
  backward       dW_l = dz_l^T agg_l (+ db_l)                       glnn_gemm_tn_f32
                 dagg_l = dz_l W_l                                  glnn_gemm_f32
                 dh_l = (A_l^T + I_dst) (dagg_l / (deg+1))          glnn_spmm_csr_f32 over glnn_csr_transpose(add_self)
                 dz_{l-1} = BN / ReLU / dropout backward            glnn_bn_relu_bwd_f32 (also yields db_{l-1}, dgamma, dbeta)
  update         one fused multi-tensor Adam launch                 glnn_adam_step_f32

  GCN layer      GraphConv(norm='both'): weight first iff in > out (dgl), D_out^-1/2 / D_in^-1/2 folded into the GEMM row
                 scale and the aggregation's row / column scales, bias + ReLU in the epilogue; backward over the transposed
                 graph with the two scales swapped.

The engine works IN PLACE on the Model's parameters / BatchNorm buffers and on the torch optimizer's state tensors, exactly
like glnn_amd.student.StudentEngine, so state_dict(), early-stopping snapshots and optimizer.state_dict() keep working."""
import ctypes
import functools
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .kinds import BY_KIND, teacher_kind, teacher_names
from .autograd import (appnp_bwd, appnp_fwd, dagnn_bwd, dagnn_fwd, gat_layer_bwd, gat_layer_fwd, gatv2_layer_bwd, gatv2_layer_fwd,
                       gt_layer_bwd, gt_layer_fwd, gcnii_bwd, gcnii_fwd, gpr_bwd, gpr_fwd, graphconv_bwd, graphconv_fwd, pna_layer_bwd,
                       pna_layer_fwd)
from .student import _mix32


def _is_relu(act):
    return act is F.relu or getattr(act, "__name__", "") == "relu"


def _check_criterion_and_optimizer(who, criterion, optimizer):
    """What reference train_teacher.py:234-237 builds: nn.NLLLoss() and a plain single-group torch.optim.Adam."""
    if not (isinstance(criterion, nn.NLLLoss) and criterion.reduction == "mean" and criterion.weight is None
            and criterion.ignore_index == -100):
        raise NotImplementedError(f"{who}: the criterion must be nn.NLLLoss() (reference train_teacher.py:237)")
    grp = optimizer.param_groups
    if type(optimizer) is not torch.optim.Adam or len(grp) != 1 or grp[0].get("amsgrad") or grp[0].get("maximize"):
        raise NotImplementedError(f"{who}: torch.optim.Adam, one param group, no amsgrad/maximize (train_teacher.py:234-236)")


def _check_norms_and_device(who, model):
    """The norm modules with the reference's defaults, and the model on the GPU (the last check: everything else is accepted by then)."""
    for bn in getattr(model.encoder, "norms", ()):
        if isinstance(bn, nn.LayerNorm):
            if not bn.elementwise_affine or len(bn.normalized_shape) != 1:
                raise NotImplementedError(f"{who}: nn.LayerNorm(hidden_dim) with the reference's defaults")
        elif bn.momentum is None or not bn.affine or not bn.track_running_stats:
            raise NotImplementedError(f"{who}: BatchNorm1d with the reference's defaults")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError(f"{who} needs the model on the GPU (HIP path only; the reference's --device -1 default selects the CPU: "
                           "pass --device 0)")


def check_supported(model, criterion, optimizer):
    """Raise unless (model, criterion, optimizer) is what train_teacher.py:232-238 builds for a teacher of a family with a TeacherEngine
    step: the rows of kinds.KINDS that name a rule, each with the sentence it is refused with."""
    enc = model.encoder
    name = model.model_name
    try:
        row = BY_KIND[teacher_kind(name)]
    except ValueError:           # (a name no family claims: refused like the MLP)
        row = BY_KIND["mlp"]
    if row.rule is None:
        raise NotImplementedError(f"TeacherEngine: {teacher_names('or', graph_kinds=True)} teachers only (got {name})")
    _check_criterion_and_optimizer("TeacherEngine", criterion, optimizer)
    norms = ("none",) if row.rule == "stack" else ("none", "batch", "layer")
    if row.rule == "stack":      # GCNII, PNA (the encoder's constructor refused everything else)
        ok = _is_relu(enc.activation) and (row.kind != "pna" or all(_is_relu(lay.activation) for lay in enc.layers))   # (PNAConv has its own)
    elif row.rule == "norm_relu":
        if row.kind == "sage" and getattr(enc, "aggregator_type", "gcn") != "gcn":
            raise NotImplementedError(f"TeacherEngine: the one-call SAGE step implements the 'gcn' aggregator only; a SAGE "
                                      f"{enc.aggregator_type!r} teacher trains through SAGE.forward's differentiable ops (train_sage)")
        ok = _is_relu(enc.activation)
    elif row.rule == "attn":
        ok = _is_relu(enc.activation) and all(lay.relu() for lay in enc.layers[:-1]) and not enc.layers[-1].relu()
    else:                        # "gcn": train.conf.yaml's cora-style GCN none, pokec / penn94 GCN batch
        ok = True
    if not ok or (row.rule != "attn" and enc.norm_type not in norms):      # (the attention stacks have no norm layers)
        raise NotImplementedError("TeacherEngine: " + row.supported)
    if row.rule == "gcn" and any(not _is_relu(lay._activation) for lay in enc.layers[:-1]):
        raise NotImplementedError("TeacherEngine: GraphConv(activation=F.relu) on hidden layers (models.py:170-187)")
    _check_norms_and_device("TeacherEngine", model)


def check_supported_mean(model, criterion, optimizer):
    """Raise unless (model, criterion, optimizer) is a SAGE "mean" teacher that TeacherEngine.step_sage_mean trains: norm_type
    none | batch | layer, ReLU, nn.NLLLoss(), plain single-group Adam, on the GPU.  (check_supported stays the gate of the "gcn" step and
    keeps refusing a "mean" model.)"""
    enc = model.encoder
    name = model.model_name
    if "SAGE" not in name:
        raise NotImplementedError(f"TeacherEngine.step_sage_mean: SAGE teachers only (got {name})")
    if getattr(enc, "aggregator_type", "gcn") != "mean":
        raise NotImplementedError(f"TeacherEngine.step_sage_mean: the 'mean' aggregator only (got {getattr(enc, 'aggregator_type', 'gcn')!r}; "
                                  "a 'gcn' teacher trains through step_sage)")
    if enc.norm_type not in ("none", "batch", "layer"):
        raise NotImplementedError(f"TeacherEngine.step_sage_mean: norm_type none|batch|layer (got {enc.norm_type!r})")
    if not _is_relu(enc.activation):
        raise NotImplementedError("TeacherEngine.step_sage_mean: the hidden activation must be ReLU")
    if any(lay.fc_self.bias is None or lay.fc_neigh.bias is None for lay in enc.layers):
        raise NotImplementedError("TeacherEngine.step_sage_mean: SAGEConv(bias=True) layers only")
    _check_criterion_and_optimizer("TeacherEngine.step_sage_mean", criterion, optimizer)
    _check_norms_and_device("TeacherEngine.step_sage_mean", model)


class _Arena:
    """Bump allocator over one device buffer (base None: sizing pass); 256-byte granules keep every sub-buffer float4-aligned."""

    def __init__(self, base):
        self.base, self.off = base, 0

    def take(self, nbytes):
        p = None if self.base is None else self.base + self.off
        self.off += (int(nbytes) + 255) // 256 * 256
        return p


def _ptr(t):
    return None if t is None else t.data_ptr()


def _r4(c):
    return (c + 3) // 4 * 4


class _GcnBlocks:
    """What TeacherEngine._block_step does for the "gcn" aggregator only (csrc/sage_step.hip): agg_l is the projection's operand, the
    backward reads the transposed block WITH the self entries and 1 / (deg + 1), and one dagg buffer serves every layer."""
    name = "step_sage"

    def static(self, eng):                              # no side descriptor
        return None

    def operands(self, A, y, md, l, n_dst, dims):
        y.agg, y.ld_agg = A.take(4 * n_dst * _r4(dims[l])), _r4(dims[l])

    def transpose(self, A, y, blk):
        # transposed by the loader (NodeDataLoader.global_first_block) -- with the self entries, not the "mean" step's plain form
        if getattr(blk, "t_indptr", None) is not None and getattr(blk, "t_add_self", True) is not False:
            y.t_indptr, y.t_indices, y.inv_deg = _ptr(blk.t_indptr), _ptr(blk.t_indices), _ptr(blk.inv_deg)
            y.tr_ws, y.tr_ws_bytes = None, 0
        else:
            n_dst, n_src = blk.num_dst_nodes(), blk.num_src_nodes()
            nnz_t = blk.num_edges() + n_dst
            wsb = int(_lib.lib().glnn_csr_transpose_workspace_bytes(n_src, nnz_t))
            y.t_indptr, y.t_indices, y.inv_deg = A.take(8 * (n_src + 1)), A.take(4 * max(nnz_t, 1)), A.take(4 * n_dst)
            y.tr_ws, y.tr_ws_bytes = A.take(wsb), (wsb + 7) // 8 * 8

    def input_grad(self, A, d, md, blocks, dims, wd):
        d.dagg, d.ld_dagg = A.take(4 * max(b.num_dst_nodes() for b in blocks[1:]) * wd), wd

    def workspaces(self, eng, d, blocks, dims):
        L, lib = eng.L, _lib.lib()
        if L > 1 and eng.bn:     # room for the outermost layer's BatchNorm backward without passes of its own (round 5)
            d.ws_bn_floats = max(d.ws_bn_floats, int(lib.glnn_sage_step_ws_bn_floats(blocks[0].num_dst_nodes(), dims[1])))
        if eng.ln:               # the LayerNorm backward's column partials (fused into the transposed aggregation, or its own launch)
            for l in range(L - 1):
                d.ws_bn_floats = max(d.ws_bn_floats, int(lib.glnn_sage_step_ws_ln_floats(blocks[l].num_dst_nodes(), dims[l + 1])))
        # (x L: in the one-call step every layer's split slabs wait in ws_tn for the Adam launch to fold them -- csrc/sage_step.hip)
        d.ws_tn_floats = L * (64 * max(dims) + 256 * 128 * 128 + 2 * max(dims) * max(dims))

    def call(self, d, md, lnd, ad, stream):
        entry = ("glnn_sage_train_step" if ad is not None else "glnn_sage_fwd_bwd") + ("_ln_f32" if lnd is not None else "_f32")
        args = [ctypes.byref(a) for a in (d, lnd, ad) if a is not None]
        return getattr(_lib.lib(), entry)(*args, stream), entry


class _MeanBlocks:
    """... and for the "mean" aggregator (csrc/sage_mean_step.hip): the [mean | self] operand pair against the packed [W_neigh | W_self]
    (re-packed in the call), the PLAIN transposed block, and one dcat buffer, layer by layer."""
    name = "step_sage_mean"

    def static(self, eng):                              # the fc_self half of every layer
        md = _lib.SageMeanDesc()
        md.num_layers = eng.L
        for l, layer in enumerate(eng.enc.layers):
            q, w, b = md.layer[l], layer.fc_self.weight, layer.fc_self.bias
            q.w_self, q.b_self, q.gw_self, q.gb_self = _ptr(w), _ptr(b), _ptr(eng.grad(w)), _ptr(eng.grad(b))
        return md

    def operands(self, A, y, md, l, n_dst, dims):
        q = md.layer[l]
        q.ld_cat = 2 * _r4(dims[l])
        q.cat = A.take(4 * n_dst * q.ld_cat)
        q.wcat, q.bsum = A.take(4 * dims[l + 1] * q.ld_cat), A.take(4 * dims[l + 1])

    def transpose(self, A, y, blk):
        # the PLAIN transpose: the loader's when it built that one (t_add_self False), else built inside the C call -- never one that
        # carries the "gcn" step's self entries
        if getattr(blk, "t_indptr", None) is not None and getattr(blk, "t_add_self", None) is False:
            y.t_indptr, y.t_indices = _ptr(blk.t_indptr), _ptr(blk.t_indices)
            y.tr_ws, y.tr_ws_bytes = None, 0
        else:
            n_src, nnz = blk.num_src_nodes(), blk.num_edges()
            wsb = int(_lib.lib().glnn_csr_transpose_workspace_bytes(n_src, nnz))
            y.t_indptr, y.t_indices = A.take(8 * (n_src + 1)), A.take(4 * max(nnz, 1))
            y.tr_ws, y.tr_ws_bytes = A.take(wsb + 8), (wsb + 7) // 8 * 8

    def input_grad(self, A, d, md, blocks, dims, wd):
        dcat = A.take(4 * max(blocks[l].num_dst_nodes() * 2 * _r4(dims[l]) for l in range(1, len(blocks))))
        for l in range(1, len(blocks)):
            md.layer[l].dcat, md.layer[l].ld_dcat = dcat, 2 * _r4(dims[l])

    def workspaces(self, eng, d, blocks, dims):
        lib = _lib.lib()
        if eng.ln:
            for l in range(eng.L - 1):
                n_l = blocks[l].num_dst_nodes()
                d.ws_bn_floats = max(d.ws_bn_floats, int(lib.glnn_sage_step_ws_ln_floats(n_l, dims[l + 1])),
                                     int(lib.glnn_layernorm_bwd_workspace_floats(n_l, dims[l + 1])))
        d.ws_tn_floats = 64 * max(dims) + 256 * 128 * 128 + 2 * max(dims) * max(dims)

    def call(self, d, md, lnd, ad, stream):
        lnp = ctypes.byref(lnd) if lnd is not None else None
        if ad is not None:
            return (_lib.lib().glnn_sage_mean_train_step_f32(ctypes.byref(d), ctypes.byref(md), lnp, ctypes.byref(ad), stream),
                    "glnn_sage_mean_train_step_f32")
        return _lib.lib().glnn_sage_mean_fwd_bwd_f32(ctypes.byref(d), ctypes.byref(md), lnp, stream), "glnn_sage_mean_fwd_bwd_f32"


_GCN_BLOCKS, _MEAN_BLOCKS = _GcnBlocks(), _MeanBlocks()


class TeacherEngine:
    def __init__(self, model, optimizer):
        self.model, self.enc, self.opt = model, model.encoder, optimizer
        self.kind = teacher_kind(model.model_name)
        self.L = self.enc.num_layers
        self.bn = getattr(self.enc, "norm_type", "none") == "batch"
        self.ln = getattr(self.enc, "norm_type", "none") == "layer"
        self.p = float(self.enc.layers[0].feat_drop.p if BY_KIND[self.kind].rule == "attn" else self.enc.dropout.p)
        params = list(model.parameters())
        self.params = params
        dev = params[0].device
        self.dev = dev
        f32 = dict(dtype=torch.float32, device=dev)
        sizes = [(p.numel() + 3) // 4 * 4 for p in params]
        self.flat_grads = torch.zeros(sum(sizes), **f32)
        self.grads, off = [], 0
        for p, sz in zip(params, sizes):
            self.grads.append(self.flat_grads[off:off + p.numel()].view_as(p))
            off += sz
        for p, g in zip(params, self.grads):
            p.grad = g
        self._g = {id(p): g for p, g in zip(params, self.grads)}
        exp_avg, exp_avg_sq = [], []
        for p in params:
            st = optimizer.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            exp_avg.append(st["exp_avg"])
            exp_avg_sq.append(st["exp_avg_sq"])
        self.step_count = int(optimizer.state[params[0]]["step"])
        self.table = ops.TensorTable(params, self.grads, exp_avg, exp_avg_sq)
        self.loss_out = torch.zeros(1, **f32)
        self.loss_accum = torch.zeros(1, **f32)
        self._sage_desc = self._arena = self._arena_stream = None      # step_sage: persistent descriptor and scratch arena
        self._sage_ln = None                                           # step_sage, norm_type "layer": the LayerNorm side descriptor
        self._sage_mean = None                                         # step_sage_mean: the fc_self / operand-buffer side descriptor
        self.mean = self.kind == "sage" and getattr(self.enc, "aggregator_type", "gcn") == "mean"
        self.ws_loss = torch.empty(1024, **f32)
        # step_sage: the hidden layers' h = dropout(relu(norm(z))) is NOT written -- the next layer's aggregation applies that tail to the z
        # rows it gathers (glnn::spmm_csr_tail; same arithmetic per element, so the step is bit-identical to the materialised form, one pass
        # over the layer's activations and its buffer less).  GLNN_TEACHER_GATHER_TAIL=0 (read here, once) keeps the act_fwd launches.
        self.gather_tail = os.environ.get("GLNN_TEACHER_GATHER_TAIL", "1") != "0"
        self._one_call = os.environ.get("GLNN_TEACHER_ONE_CALL", "1") != "0"
        self.base_seed = int(torch.initial_seed()) & 0xFFFFFFFF
        self.grad_sync = None

    # ------------------------------------------------------------------------------------------
    def grad(self, p):
        return self._g[id(p)]

    def _seed(self, layer):
        return _stream_seed(self, 0, 1, layer, self.p > 0)

    def _adam(self):
        g = self.opt.param_groups[0]
        if self.grad_sync is not None:
            self.grad_sync()
        ops.adam_step(self.table, g["lr"], self.step_count, weight_decay=g["weight_decay"], beta1=g["betas"][0], beta2=g["betas"][1],
                      eps=g["eps"])

    def sync_optimizer_state(self):
        for p in self.params:
            self.opt.state[p]["step"] = torch.tensor(float(self.step_count))

    def _tail_fwd(self, l, z):
        """norms[l] -> relu -> dropout of hidden layer l (models.py:113-117), materialised for the next layer's gather."""
        seed = self._seed(l)
        if self.bn:
            bn = self.enc.norms[l]
            stats = ops.bn_stats(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, eps=bn.eps,
                                 momentum=bn.momentum)
        else:
            stats = (None, None, None, None)
        return ops.act_fwd(z, stats[2], stats[3], drop_p=self.p, drop_seed=seed), stats, seed

    def _tail_bwd(self, l, dh, z, stats, seed, bias_grad):
        """dz_l (in place on dh) + dgamma / dbeta + the bias gradient of the layer in front."""
        mean, rstd, a_scale, a_shift = stats
        if self.bn:
            bn = self.enc.norms[l]
            ops.bn_relu_bwd(dh, z, bn.weight, mean, rstd, a_scale, a_shift, dz=dh, dgamma=self.grad(bn.weight), dbeta=self.grad(bn.bias),
                            drop_p=self.p, drop_seed=seed, dz_col_sum=bias_grad)
        else:
            ops.bn_relu_bwd(dh, z, dz=dh, drop_p=self.p, drop_seed=seed, dz_col_sum=bias_grad)
        return dh

    # ------------------------------------------------------------------------------------------ GraphSAGE on blocks
    @torch.no_grad()
    def _sage_signature(self, enc):
        """Everything the persistent glnn_sage_step_desc captured once: the data pointers of every parameter, gradient buffer and BatchNorm
        buffer, and the scalars baked into it.  A step whose signature differs rebuilds the descriptor (only the weight / bias
        pointers used to be compared, so a replaced norm module or a changed dropout left the C call on stale or freed pointers)."""
        ptr = _ptr
        sig = [float(enc.dropout.p), len(enc.layers)]
        for l, layer in enumerate(enc.layers):
            w, b = layer.fc_neigh.weight, layer.fc_neigh.bias
            sig += [ptr(w), ptr(b), ptr(self.grad(w)), ptr(self.grad(b))]
            if self.mean:
                w, b = layer.fc_self.weight, layer.fc_self.bias
                sig += [ptr(w), ptr(b), ptr(self.grad(w)), ptr(self.grad(b))]
            if l != len(enc.layers) - 1 and self.bn:
                bn = enc.norms[l]
                sig += [ptr(bn.weight), ptr(bn.bias), ptr(self.grad(bn.weight)), ptr(self.grad(bn.bias)), ptr(bn.running_mean), ptr(bn.running_var),
                        ptr(bn.num_batches_tracked), bn.eps, bn.momentum]
            elif l != len(enc.layers) - 1 and self.ln:
                ln = enc.norms[l]
                sig += [ptr(ln.weight), ptr(ln.bias), ptr(self.grad(ln.weight)), ptr(self.grad(ln.bias)), ln.eps]
        return sig + [ptr(self.ws_loss), ptr(self.loss_out), ptr(self.loss_accum)]

    def step_sage(self, blocks, feats, labels, output_nodes, lamb=1.0, input_nodes=None):
        """One optimisation step on a batch of sampled blocks (blocks[0] outermost).  `feats` is the GLOBAL feature matrix:
        when blocks[0] carries global source ids (glnn_amd.graph.NodeDataLoader) its aggregation gathers from it directly,
        otherwise feats[input_nodes] is gathered once (blocks that came from elsewhere).  The whole forward + loss + backward
        is ONE C call (glnn_sage_fwd_bwd_f32, csrc/sage_step.hip) over buffers allocated here; Adam follows -- inside the same call
        (glnn_sage_train_step_f32) when nothing sits between the backward and Adam."""
        if self.mean:      # (this step has no fc_self term: it would silently train another model)
            raise NotImplementedError("TeacherEngine.step_sage implements the 'gcn' aggregator; a SAGE 'mean' teacher steps through "
                                      "TeacherEngine.step_sage_mean")
        self._block_step(_GCN_BLOCKS, blocks, feats, labels, output_nodes, lamb, input_nodes)

    def step_sage_mean(self, blocks, feats, labels, output_nodes, lamb=1.0, input_nodes=None):
        """step_sage for a SAGE "mean" teacher (docs/SAGE_MEAN_SEMANTICS.md): the same contract -- in place on the parameters, the BatchNorm
        buffers and the optimiser's moments; `feats` global, gathered through blocks[0]'s global ids when it carries them -- as ONE C call,
        glnn_sage_mean_train_step_f32 (csrc/sage_mean_step.hip): per layer the [mean | self] operand pair and one projection against the
        packed [W_neigh | W_self]; backward over the PLAIN transposed blocks.  grad_sync set (or GLNN_TEACHER_ONE_CALL=0):
        glnn_sage_mean_fwd_bwd_f32, then Adam."""
        if not self.mean:
            raise NotImplementedError("TeacherEngine.step_sage_mean: SAGE 'mean' teachers only; a 'gcn' teacher steps through step_sage")
        self._block_step(_MEAN_BLOCKS, blocks, feats, labels, output_nodes, lamb, input_nodes)

    def _block_descriptors(self, v):
        """Everything of a sampled-block step that does not depend on the batch, written ONCE: sizes, parameter / gradient / BatchNorm
        pointers, the LayerNorm side descriptor, and what variant `v` adds.  (Building the ~150 ctypes fields from nothing was 0.1 ms of the
        0.25 ms of host time per step of a loop that is host-bound.)  _sage_signature() is what they captured."""
        enc, L, ptr = self.enc, self.L, _ptr
        d = _lib.SageStepDesc()
        self._sage_dims = [enc.layers[0].fc_neigh.weight.shape[1]] + [lay.fc_neigh.weight.shape[0] for lay in enc.layers]
        self.p = float(enc.dropout.p)
        d.num_layers, d.batchnorm, d.dropout_p = L, 1 if self.bn else 0, self.p
        for i, n in enumerate(self._sage_dims):
            d.dims[i] = n
        for l, layer in enumerate(enc.layers):
            y = d.layer[l]
            w, b = layer.fc_neigh.weight, layer.fc_neigh.bias
            y.w, y.b, y.gw, y.gb = ptr(w), ptr(b), ptr(self.grad(w)), ptr(self.grad(b))
            if l != L - 1 and self.bn:
                bn = enc.norms[l]
                d.bn_eps, d.bn_momentum = bn.eps, bn.momentum
                y.gamma, y.beta, y.ggamma, y.gbeta = ptr(bn.weight), ptr(bn.bias), ptr(self.grad(bn.weight)), ptr(self.grad(bn.bias))
                y.running_mean, y.running_var, y.nbt = ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked)
        lnd = None
        if self.ln and L > 1:          # nn.LayerNorm tails: parameters and gradients in the side descriptor (the row statistics are scratch);
            lnd = _lib.SageLnDesc()    # a one-layer encoder has no hidden tail and no norm module
            lnd.eps = enc.norms[0].eps
            for l in range(L - 1):
                ln, q = enc.norms[l], lnd.layer[l]
                if ctypes.c_float(ln.eps).value != lnd.eps:
                    raise NotImplementedError("TeacherEngine: the hidden LayerNorms of a SAGE teacher must share one eps")
                q.gamma, q.beta, q.ggamma, q.gbeta = ptr(ln.weight), ptr(ln.bias), ptr(self.grad(ln.weight)), ptr(self.grad(ln.bias))
        self._sage_desc, self._sage_mean, self._sage_ln = d, v.static(self), lnd
        self._sage_static = self._sage_signature(enc)

    def _block_step(self, v, blocks, feats, labels, output_nodes, lamb, input_nodes):
        """The sampled-block step behind step_sage / step_sage_mean; `v` (_GcnBlocks / _MeanBlocks) holds what the two aggregators do
        differently: operand buffers, the transpose the backward reads, two workspace sizes and the C entry."""
        enc, L, who, ptr, r4 = self.enc, self.L, "TeacherEngine." + v.name, _ptr, _r4
        ops._need_cuda(feats, labels, output_nodes, input_nodes)
        if len(blocks) != L:
            raise ValueError(f"{who}: {len(blocks)} blocks for {L} layers")
        if L > _lib.SAGE_MAX_LAYERS:
            raise NotImplementedError(f"TeacherEngine: at most {_lib.SAGE_MAX_LAYERS} layers")
        if labels.dtype != torch.int64 or output_nodes.dtype != torch.int64 or not output_nodes.is_contiguous():
            raise ValueError(f"{who}: labels / output_nodes must be int64 (output_nodes contiguous)")
        x = ops.as_feat(feats)
        dev = self.dev
        if blocks[0].gindices is None:
            if input_nodes is None:
                raise ValueError(f"{who}: blocks without global ids need input_nodes")
            x = ops.gather_rows(x, input_nodes)
        for l in range(1, L):
            if blocks[l].num_src_nodes() != blocks[l - 1].num_dst_nodes():
                raise ValueError(f"{who}: block {l} has {blocks[l].num_src_nodes()} sources, block {l - 1} "
                                 f"{blocks[l - 1].num_dst_nodes()} destinations")
        if x.shape[0] < (blocks[0].num_src_nodes() if blocks[0].gindices is None else 1):
            raise ValueError(f"{who}: the layer-0 source matrix is smaller than the outermost block")
        # The descriptors live across steps; a step only fills in the blocks, the dropout seeds and the scratch pointers.  They are rebuilt
        # when something they captured was replaced (load_state_dict keeps the tensors; .to(), a new norm module, a changed dropout / eps /
        # momentum do not).
        if self._sage_desc is None or self._sage_static != self._sage_signature(enc):
            self._block_descriptors(v)
        d, md, lnd, dims = self._sage_desc, self._sage_mean, self._sage_ln, self._sage_dims
        self.step_count += 1
        d.lamb = float(lamb)
        # Every buffer of the step is scratch that only the C call touches, so they are carved as raw pointers out of ONE arena that
        # persists across steps (same-stream reuse is ordered; it grows when a batch needs more).  ONE pass hands out the pointers.

        def layout(A):
            max_rows, max_hidden = 1, 4
            for l, blk in enumerate(blocks):
                y = d.layer[l]
                n_dst = blk.num_dst_nodes()
                v.operands(A, y, md, l, n_dst, dims)
                y.z, y.ldz = A.take(4 * n_dst * r4(dims[l + 1])), r4(dims[l + 1])
                if l != L - 1:
                    if self.gather_tail and dims[l + 1] <= 256:      # (the tail-in-gather kernels hold a row in registers: d <= 256)
                        y.h, y.ldh = None, 0
                    else:
                        y.h, y.ldh = A.take(4 * n_dst * r4(dims[l + 1])), r4(dims[l + 1])
                    max_rows, max_hidden = max(max_rows, n_dst), max(max_hidden, dims[l + 1])
                    if self.bn:
                        y.mean, y.rstd, y.a_scale, y.a_shift = (A.take(4 * dims[l + 1]) for _ in range(4))
                    if lnd is not None:          # per-ROW statistics of z_l (written by the forward, read by the backward)
                        q = lnd.layer[l]
                        q.mean, q.rstd = A.take(4 * n_dst), A.take(4 * n_dst)
                if l >= 1:
                    v.transpose(A, y, blk)
            d.dlogits, d.ld_dlogits = A.take(4 * blocks[-1].num_dst_nodes() * r4(dims[-1])), r4(dims[-1])
            nchunks = (max_rows + 127) // 128
            d.ws_bn_floats = (3 * nchunks + 2 + 3 * ((nchunks + 63) // 64)) * max_hidden + 1024
            if L > 1:
                wd = r4(max(dims[1:L]))
                v.input_grad(A, d, md, blocks, dims, wd)
                d.dh, d.ld_dh = A.take(4 * max(b.num_src_nodes() for b in blocks[1:]) * wd), wd
            v.workspaces(self, d, blocks, dims)
            # split-K slabs, sized as StudentEngine does; the GEMM only splits outputs of < 256 tiles, i.e. <= 512 slabs of 128 x 128
            d.ws_gemm_floats = min(max(16 * max(b.num_dst_nodes() for b in blocks) * min(dims[1:]), 1 << 20), 512 * 128 * 128)
            d.ws_bn, d.ws_tn, d.ws_gemm = A.take(4 * d.ws_bn_floats), A.take(4 * d.ws_tn_floats), A.take(4 * d.ws_gemm_floats)
            return A.off

        for l, blk in enumerate(blocks):       # the batch: blocks and dropout seeds
            y = d.layer[l]
            glob = l == 0 and blk.gindices is not None
            y.indptr, y.indices = ptr(blk.indptr), ptr(blk.gindices if glob else blk.indices)
            y.n_dst, y.n_src, y.nnz = blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()
            y.self_rows = ptr(blk.dst_nodes) if glob else None
            if l != L - 1:
                y.drop_seed = self._seed(l)
        cur = torch.cuda.current_stream(dev)
        if self._arena_stream is not None and self._arena_stream != cur:
            cur.wait_stream(self._arena_stream)            # the previous step used the arena on another stream
        self._arena_stream = cur
        arena = self._arena
        base = 0 if arena is None else (arena.data_ptr() + 255) // 256 * 256
        total = layout(_Arena(base))
        if arena is None or total + 256 > arena.numel():    # first step / a bigger batch: (re)allocate with headroom, lay out again
            arena = self._arena = torch.empty(int(total * 1.25) + 256, dtype=torch.uint8, device=dev)
            layout(_Arena((arena.data_ptr() + 255) // 256 * 256))
        d.x, d.ldx, d.x_rows = ptr(x), x.stride(0), x.shape[0]      # (x stays alive until the call below is queued: same-stream reuse is ordered)
        d.labels, d.label_rows = ptr(labels), ptr(output_nodes)
        d.ws_loss, d.ws_loss_floats = ptr(self.ws_loss), self.ws_loss.numel()
        d.loss_out, d.loss_accum = ptr(self.loss_out), ptr(self.loss_accum)
        ops.note_param_write()      # (running statistics are written through raw pointers; Adam follows)
        # nothing sits between the backward and Adam (no gradient exchange): the whole step is ONE C call (and in the "gcn" step Adam folds
        # the backward's last partial sums itself); GLNN_TEACHER_ONE_CALL=0 keeps the two calls
        ad = None
        if self.grad_sync is None and self._one_call:
            g_ = self.opt.param_groups[0]
            ad = self.table.desc
            ad.lr, ad.beta1, ad.beta2, ad.eps, ad.weight_decay, ad.step = g_["lr"], g_["betas"][0], g_["betas"][1], g_["eps"], g_["weight_decay"], self.step_count
        rc, entry = v.call(d, md, lnd, ad, ops._stream())
        if rc != 0:
            self.step_count -= 1          # the step never happened: Adam's bias correction and the dropout seeds stay where they were
        _lib.check(rc, entry)
        if ad is None:
            self._adam()

    # ------------------------------------------------------------------------------------------ full-graph steps
    def _run_full_graph(self, body, g, feats, labels, idx_train, lamb):
        """One full-graph optimisation step: body(g, feats, labels, idx_train, lamb) is forward + loss + backward into the gradient
        buffers, Adam follows.  A body that raises leaves step_count -- Adam's bias correction and the dropout seeds -- where it was: the
        step never happened (see _block_step)."""
        ops._need_cuda(feats, labels, idx_train, g.indptr)
        self.step_count += 1
        try:
            body(g, feats, labels, idx_train, lamb)
        except Exception:
            self.step_count -= 1
            raise
        self._adam()

    # ------------------------------------------------------------------------------------------ full-graph GCN
    @torch.no_grad()
    def step_gcn(self, g, feats, labels, idx_train, lamb=1.0):
        if g.has_zero_in_degree() and not all(lay._allow_zero_in_degree for lay in self.enc.layers):
            raise RuntimeError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid "
                               "(dgl GraphConv semantics; add self-loops or set allow_zero_in_degree).")
        self._run_full_graph(self._step_gcn_body, g, feats, labels, idx_train, lamb)

    def _step_gcn_body(self, g, feats, labels, idx_train, lamb):
        enc, L, p = self.enc, self.L, self.p
        a = ops.as_feat(feats)
        saved = []
        norm_kind = enc.norm_type
        for l, layer in enumerate(enc.layers):
            last = l == L - 1
            y, mid, first = graphconv_fwd(g, a, layer.weight, layer.bias, relu=not last)
            seed = self._seed(l)
            stats = None
            if not last:      # reference models.py:195-198: norms[l] -> dropout, NO ReLU behind the norm (it sits inside the conv)
                if norm_kind == "batch":
                    bn = enc.norms[l]
                    stats = ops.bn_stats(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, eps=bn.eps,
                                         momentum=bn.momentum)
                    a = ops.act_fwd(y, stats[2], stats[3], drop_p=p, drop_seed=seed, relu=False)
                elif norm_kind == "layer":
                    ln = enc.norms[l]
                    a, mu, rs = ops.layernorm_fwd(y, ln.weight, ln.bias, eps=ln.eps, relu=False, drop_p=p, drop_seed=seed)
                    stats = (mu, rs)
                else:
                    a = ops.act_fwd(y, drop_p=p, drop_seed=seed) if p > 0 else y       # y >= 0 already (ReLU inside the conv)
            saved.append((mid, first, y, seed, stats))
        dz = self._loss_grad(saved[-1][2], labels, idx_train, lamb, g.num_dst_nodes())
        ops.col_sum(dz, out=self.grad(enc.layers[-1].bias))
        for l in range(L - 1, -1, -1):
            layer = enc.layers[l]
            mid, first, _, _, _ = saved[l]
            da = graphconv_bwd(g, dz, mid, first, layer.weight, self.grad(layer.weight), want_da=l > 0)
            if l == 0:
                break
            _, _, y_prev, seed_prev, stats = saved[l - 1]
            if norm_kind == "batch":       # dropout + norm backward (no ReLU in this tail) -> grad wrt the conv's output y
                bn = enc.norms[l - 1]
                mean, rstd, a_sc, a_sh = stats
                ops.bn_relu_bwd(da, y_prev, bn.weight, mean, rstd, a_sc, a_sh, dz=da, dgamma=self.grad(bn.weight), dbeta=self.grad(bn.bias),
                                drop_p=p, drop_seed=seed_prev, relu=False)
                dz, _, _ = ops.bn_relu_bwd(da, y_prev, dz=da, dz_col_sum=self.grad(enc.layers[l - 1].bias))     # the ReLU inside conv l-1
            elif norm_kind == "layer":
                ln = enc.norms[l - 1]
                _, dg, db = ops.layernorm_bwd(da, y_prev, ln.weight, ln.bias, stats[0], stats[1], relu=False, drop_p=p, drop_seed=seed_prev, dz=da)
                self.grad(ln.weight).copy_(dg)
                self.grad(ln.bias).copy_(db)
                dz, _, _ = ops.bn_relu_bwd(da, y_prev, dz=da, dz_col_sum=self.grad(enc.layers[l - 1].bias))
            else:                          # dropout backward, then the ReLU inside conv l-1 (y > 0 <=> z > 0)
                dz, _, _ = ops.bn_relu_bwd(da, y_prev, dz=da, drop_p=p, drop_seed=seed_prev, dz_col_sum=self.grad(enc.layers[l - 1].bias))


    # ------------------------------------------------------------------------------------------ full-graph APPNP
    def _edge_seed(self, step=None):
        """The edge-dropout seed of step `step` (default: the current one): a stream apart from the hidden-layer seeds _seed(layer < 8)."""
        return _stream_seed(self, 0x41505050, 0x7F, 0, self.enc.edge_drop > 0, step)

    @torch.no_grad()
    def step_appnp(self, g, feats, labels, idx_train, lamb=1.0):
        """The reference's full-graph `train` (train_and_eval.py:12-29) over APPNP (models.py:326-344): the MLP trunk (glnn_gemm_f32 +
        norm / ReLU / dropout tails), K launches of glnn_appnp_prop_f32, NLL over idx_train, K launches of glnn_appnp_prop_bwd_f32 over
        the transposed graph, the trunk backward, Adam."""
        self._run_full_graph(self._step_appnp_body, g, feats, labels, idx_train, lamb)

    def _trunk_tail_fwd(self, l, z):
        """norms[l] -> relu -> dropout of hidden layer l (models.py:334-338)."""
        if self.enc.norm_type == "layer":
            seed = self._seed(l)
            ln = self.enc.norms[l]
            a, mu, rs = ops.layernorm_fwd(z, ln.weight, ln.bias, eps=ln.eps, relu=True, drop_p=self.p, drop_seed=seed)
            return a, (mu, rs), seed
        return self._tail_fwd(l, z)

    def _trunk_tail_bwd(self, l, dh, z, stats, seed, bias_grad):
        if self.enc.norm_type == "layer":
            ln = self.enc.norms[l]
            _, dg, db = ops.layernorm_bwd(dh, z, ln.weight, ln.bias, stats[0], stats[1], relu=True, drop_p=self.p, drop_seed=seed, dz=dh,
                                         dz_col_sum=bias_grad)
            self.grad(ln.weight).copy_(dg)
            self.grad(ln.bias).copy_(db)
            return dh
        return self._tail_bwd(l, dh, z, stats, seed, bias_grad)

    def _trunk_fwd(self, feats):
        """The MLP trunk of APPNP / GPRGNN / DAGNN in training mode: (trunk logits, layer inputs, saved tails)."""
        enc, L = self.enc, self.L
        a = ops.as_feat(feats)
        acts, saved = [a], []
        for l, layer in enumerate(enc.layers):
            z = ops.gemm(a, layer.weight, ep_shift=layer.bias)
            if l != L - 1:
                a, stats, seed = self._trunk_tail_fwd(l, z)
                saved.append((z, stats, seed))
                acts.append(a)
            else:
                a = z
        return a, acts, saved

    def _trunk_bwd(self, dz, acts, saved):
        """Gradients of every trunk parameter from dz = d/d(trunk logits)."""
        enc, L = self.enc, self.L
        for l in range(L - 1, -1, -1):
            layer = enc.layers[l]
            ops.gemm_tn(dz, acts[l], out=self.grad(layer.weight), col_sum_a=self.grad(layer.bias))    # dW = dz^T a, db = sum dz
            if l == 0:
                break
            da = ops.gemm(dz, layer.weight, w_is_kn=True)                        # dz W
            z, stats, seed = saved[l - 1]
            dz = self._trunk_tail_bwd(l - 1, da, z, stats, seed, None)

    def _loss_grad(self, logits, labels, idx_train, lamb, n):
        """NLL over out[idx_train] (train_and_eval.py:22) and its gradient scattered back to [n, C]."""
        logits_tr = ops.gather_rows(logits, idx_train)
        _, dl = ops.softmax_loss(logits_tr, ops.LOSS_NLL, float(lamb), labels=labels, label_rows=idx_train, loss_out=self.loss_out,
                                 loss_accum=self.loss_accum, workspace=self.ws_loss)
        dlog = ops.feat_empty(n, logits.shape[1], self.dev, zero=True)
        ops.scatter_rows(dl, idx_train, dlog)
        return dlog

    def _step_prop_body(self, fwd, bwd, g, feats, labels, idx_train, lamb):
        """A trunk-and-propagate teacher through its per-kind pair: fwd(self, g, h0) -> (logits, kept), bwd(self, g, dlog, h0, kept) ->
        d/d(trunk logits), which also leaves the gradients of the propagation's own parameters."""
        h0, acts, saved = self._trunk_fwd(feats)
        logits, kept = fwd(self, g, h0)
        dlog = self._loss_grad(logits, labels, idx_train, lamb, g.num_dst_nodes())
        self._trunk_bwd(bwd(self, g, dlog, h0, kept), acts, saved)
        ops.note_param_write()

    def _appnp_fwd(self, g, h0):
        enc, seed_e = self.enc, self._edge_seed()
        return appnp_fwd(g, h0, enc.k, enc.alpha, enc.edge_drop, seed_e), seed_e

    def _appnp_bwd(self, g, dlog, h0, seed_e):
        return appnp_bwd(g, dlog, self.enc.k, self.enc.alpha, self.enc.edge_drop, seed_e)

    _step_appnp_body = functools.partialmethod(_step_prop_body, _appnp_fwd, _appnp_bwd)

    # ------------------------------------------------------------------------------------------ full-graph GPR-GNN
    @torch.no_grad()
    def step_gpr(self, g, feats, labels, idx_train, lamb=1.0):
        """The full-graph `train` step over GPRGNN (docs/GPR_SEMANTICS.md): the MLP trunk with its norm / ReLU / dropout tails, K launches
        of glnn_gpr_prop_f32, NLL over idx_train, K launches over the transposed graph whose epilogues leave the per-row <G_k, h0>,
        glnn_gpr_fold_f32 into grad(gamma), the trunk backward, and the ONE Adam launch (gamma is one more tensor of its table)."""
        self._run_full_graph(self._step_gpr_body, g, feats, labels, idx_train, lamb)

    def _gpr_fwd(self, g, h0):
        return gpr_fwd(g, h0, self.enc.propagate.gamma, self.enc.k), None

    def _gpr_bwd(self, g, dlog, h0, _):
        gamma = self.enc.propagate.gamma
        dz, dgamma = gpr_bwd(g, dlog, h0, gamma, self.enc.k)
        self.grad(gamma).copy_(dgamma)
        return dz

    _step_gpr_body = functools.partialmethod(_step_prop_body, _gpr_fwd, _gpr_bwd)

    # ------------------------------------------------------------------------------------------ full-graph DAGNN
    @torch.no_grad()
    def step_dagnn(self, g, feats, labels, idx_train, lamb=1.0):
        """The full-graph `train` step over DAGNN (docs/DAGNN_SEMANTICS.md): the MLP trunk with its norm / ReLU / dropout tails, per hop one
        glnn_spmm_csr_f32 and one glnn_dagnn_gate_f32 that keep every H_k and gate, NLL over idx_train, per hop one glnn_spmm_csr_f32 over
        the transposed graph and one glnn_dagnn_gate_bwd_f32 that leaves the per-row q, glnn_dagnn_fold_f32 into grad(proj.weight) /
        grad(proj.bias), the trunk backward, and the ONE Adam launch (the gate's weight and bias are two more tensors of its table)."""
        self._run_full_graph(self._step_dagnn_body, g, feats, labels, idx_train, lamb)

    def _dagnn_fwd(self, g, h0):
        proj = self.enc.propagate.proj
        return dagnn_fwd(g, h0, proj.weight, proj.bias, self.enc.k, keep=True)

    def _dagnn_bwd(self, g, dlog, h0, kept):
        proj = self.enc.propagate.proj
        dz, dw, db = dagnn_bwd(g, dlog, kept, proj.weight, self.enc.k)
        self.grad(proj.weight).copy_(dw.view_as(proj.weight))
        self.grad(proj.bias).copy_(db)
        return dz

    _step_dagnn_body = functools.partialmethod(_step_prop_body, _dagnn_fwd, _dagnn_bwd)

    # ------------------------------------------------------------------------------------------ full-graph GCNII
    def _gcnii_seed(self, site, step=None):
        """The seed of dropout site `site` (0: the input, l = 1..L: in front of conv layer l, L + 1: in front of fc_out) in step `step`
        (default: the current one): a stream of its own, apart from _seed, _edge_seed and _attn_seed.  site < 131, so no two (step, site)
        pairs share a counter."""
        return _stream_seed(self, 0x47434E32, 0x51, site, self.p > 0, step)

    @torch.no_grad()
    def step_gcnii(self, g, feats, labels, idx_train, lamb=1.0):
        """The full-graph `train` step over GCNII (docs/GCNII_SEMANTICS.md): fc_in (+ ReLU) behind the input dropout, L launches of
        glnn_gcnii_layer_f32 that keep S_l and H_l, fc_out, NLL over idx_train, fc_out's backward, L launches of
        glnn_gcnii_layer_bwd_f32 over the transposed graph with one glnn_gemm_tn_f32 each (beta_l folded into its stored operand), the
        launch for dH_0, H_0's ReLU backward, fc_in's backward, and the ONE Adam launch."""
        self._run_full_graph(self._step_gcnii_body, g, feats, labels, idx_train, lamb)

    def _step_stack_body(self, seed_of, fwd, bwd, g, feats, labels, idx_train, lamb):
        """A stack teacher (models._ConvStack) through its per-kind pair: fwd(self, g, h0, seeds) -> (H_L, kept) and
        bwd(self, g, da, h0, kept, seeds) -> (dH_0, mask), which also leaves the conv layers' gradients.  mask: drop_p / drop_seed of a
        dropout mask dH_0 still lacks, applied inside H_0's ReLU backward (PNA's layer-1 feat_drop); {} = that launch's plain variant."""
        enc, L, p = self.enc, self.L, self.p
        fc_in, fc_out = enc.fc_in, enc.fc_out
        seeds = [seed_of(self, s) for s in range(L + 2)]
        x = ops.as_feat(feats)
        # drop_0(x) is materialised once per step (signed features: the GEMM's operand-load dropout carries a ReLU) and read twice
        xd = ops.act_fwd(x, drop_p=p, drop_seed=seeds[0], relu=False) if p > 0 else x
        h0 = ops.gemm(xd, fc_in.weight, ep_shift=fc_in.bias, relu=True)
        hl, kept = fwd(self, g, h0, seeds)
        a = ops.act_fwd(hl, drop_p=p, drop_seed=seeds[L + 1], relu=False) if p > 0 else hl
        logits = ops.gemm(a, fc_out.weight, ep_shift=fc_out.bias)
        dlog = self._loss_grad(logits, labels, idx_train, lamb, g.num_dst_nodes())
        ops.gemm_tn(dlog, a, out=self.grad(fc_out.weight), col_sum_a=self.grad(fc_out.bias))
        da = ops.gemm(dlog, fc_out.weight, w_is_kn=True)                          # dlog W_out: d/d drop_{L+1}(H_L)
        dh0, mask = bwd(self, g, da, h0, kept, seeds)
        dz0, _, _ = ops.bn_relu_bwd(dh0, h0, dz=dh0, dz_col_sum=self.grad(fc_in.bias), **mask)     # h0 = relu(z0): h0 > 0 <=> z0 > 0
        ops.gemm_tn(dz0, xd, out=self.grad(fc_in.weight))
        ops.note_param_write()

    def _gcnii_fwd(self, g, h0, seeds):
        enc, weights, betas = self.enc, [lay.weight for lay in self.enc.layers], self.enc.betas()      # (read once a step, as before)
        hs, ss = gcnii_fwd(g, h0, weights, enc.alpha, betas, self.p, seeds, save=True)
        return hs[-1], (hs, ss, weights, betas)

    def _gcnii_bwd(self, g, da, h0, kept, seeds):
        hs, ss, weights, betas = kept
        return gcnii_bwd(g, da, hs, ss, weights, self.enc.alpha, betas, [self.grad(w) for w in weights], self.p, seeds), {}

    _step_gcnii_body = functools.partialmethod(_step_stack_body, _gcnii_seed, _gcnii_fwd, _gcnii_bwd)

    # ------------------------------------------------------------------------------------------ full-graph PNA
    def _pna_seed(self, site, step=None):
        """The seed of dropout site `site` (0: the input, l = 1..L: in front of conv layer l -- its feat_drop --, L + 1: in front of fc_out)
        in step `step` (default: the current one): a stream of its own, apart from every other teacher's.  site < 131."""
        return _stream_seed(self, 0x504E4132, 0x67, site, self.p > 0, step)

    @torch.no_grad()
    def step_pna(self, g, feats, labels, idx_train, lamb=1.0):
        """The full-graph `train` step over PNA (docs/PNA_SEMANTICS.md): fc_in (+ ReLU) behind the input dropout; per layer the dropped
        copy of its input, the two halves of `pre`, glnn_pna_agg_fwd_f32 (S, and the means and arguments the backward reads), the x and
        stacked-S products of `post` and glnn_pna_scale_fwd_f32 (+ ReLU); fc_out, NLL over idx_train, fc_out's backward; per layer
        glnn_pna_scale_bwd_f32, the weight gradients of `post`, dS, glnn_pna_da_f32, glnn_pna_agg_bwd_f32 over the transposed graph, the
        weight gradients of `pre` and the input gradient; H_0's ReLU backward, fc_in's backward, and the ONE Adam launch.  Rows without
        in-edges are legal."""
        self._run_full_graph(self._step_pna_body, g, feats, labels, idx_train, lamb)

    def _pna_fwd(self, g, h0, seeds):
        acts, saved = [h0], []
        for l, lay in enumerate(self.enc.layers):
            y, sv = pna_layer_fwd(g, acts[l], lay.pre.weight, lay.pre.bias, lay.post.weight, lay.post.bias, lay.delta, True, self.p,
                                  seeds[l + 1], keep=True)
            acts.append(y)
            saved.append(sv)
        return acts[-1], (acts, saved)

    def _pna_bwd(self, g, da, h0, kept, seeds):
        acts, saved = kept
        for l in range(self.L - 1, -1, -1):
            lay = self.enc.layers[l]
            # the dropout mask of site l + 2 (in front of the next conv, or of fc_out) and the ReLU mask of H_{l+1} (stored post-ReLU)
            gy = ops.bn_relu_bwd(da, acts[l + 1], dz=da, drop_p=self.p, drop_seed=seeds[l + 2])[0]
            da = pna_layer_bwd(g, gy, saved[l], lay.pre.weight, lay.post.weight, lay.delta, need_dx=True, dw_pre=self.grad(lay.pre.weight),
                               db_pre=self.grad(lay.pre.bias), dw_post=self.grad(lay.post.weight), db_post=self.grad(lay.post.bias))[0]
        return da, dict(drop_p=self.p, drop_seed=seeds[1])      # (layer 1's feat_drop mask is still to come)

    _step_pna_body = functools.partialmethod(_step_stack_body, _pna_seed, _pna_fwd, _pna_bwd)

    # ------------------------------------------------------------------------------------------ full-graph GAT
    def _attn_seed(self, layer):
        """The attention-dropout seed of `layer` in the current step: a stream of its own, apart from the feature dropout seeds _seed(layer)."""
        return _stream_seed(self, 0x47415441, 0x3D, layer, float(self.enc.layers[layer].attn_drop.p) > 0)

    @torch.no_grad()
    def step_gat(self, g, feats, labels, idx_train, lamb=1.0):
        """The reference's full-graph `train` (train_and_eval.py:12-29) over GAT (models.py:202-279): per layer the projection with the
        feature dropout in its operand load, glnn_gat_scores_f32 and glnn_gat_attn_fwd_f32; NLL over idx_train; per layer
        glnn_gat_attn_bwd_f32 over the graph and its transpose, the weight gradient and the input gradient; Adam."""
        self._step_attn(self._step_gat_body, "dgl GATConv semantics", g, feats, labels, idx_train, lamb)

    @torch.no_grad()
    def step_gatv2(self, g, feats, labels, idx_train, lamb=1.0):
        """The full-graph `train` step over GATv2 (docs/GATV2_SEMANTICS.md): per layer the dropped copy of the input, the two projections
        and glnn_gatv2_attn_fwd_f32; NLL over idx_train; per layer glnn_gatv2_attn_bwd_f32 over the graph and its transpose, the two weight
        gradients with their bias column sums and the input gradient; the ONE Adam launch."""
        self._step_attn(self._step_gatv2_body, "GATv2Conv follows dgl GATConv", g, feats, labels, idx_train, lamb)

    @torch.no_grad()
    def step_gt(self, g, feats, labels, idx_train, lamb=1.0):
        """The full-graph `train` step over GraphTransformer (docs/GT_SEMANTICS.md): per layer the dropped copy of the input, the four
        projections and glnn_gt_attn_fwd_f32; NLL over idx_train; per layer glnn_gt_attn_bwd_f32 over the graph and its transpose, the
        four weight gradients with their bias column sums and the input gradient; the ONE Adam launch."""
        self._step_attn(self._step_gt_body, "TransformerConv follows dgl GATConv", g, feats, labels, idx_train, lamb)

    def _step_attn(self, body, semantics, g, feats, labels, idx_train, lamb):
        if g.has_zero_in_degree():
            raise RuntimeError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid "
                               f"({semantics}; add self-loops or set allow_zero_in_degree).")
        self._run_full_graph(body, g, feats, labels, idx_train, lamb)

    def _step_attn_body(self, fwd, bwd, signed_input, g, feats, labels, idx_train, lamb):
        """Forward, loss and backward of an attention teacher through its per-kind pair (fwd, bwd).  acts[l] is the input of layer l: the
        features, then the stored (post-ReLU) output of layer l - 1.  signed_input: GAT's, whose feature dropout rides in the projection."""
        enc, L = self.enc, self.L
        acts, saved = [ops.as_feat(feats)], []
        signed0 = signed_input and self.p > 0 and not ops.is_nonneg(feats)
        for l, lay in enumerate(enc.layers):
            fs, as_ = self._seed(l), self._attn_seed(l)
            y, sv = fwd(self, g, lay, acts[l], l != L - 1, fs, as_, signed0 and l == 0)
            saved.append((sv, fs, as_))
            acts.append(y)
        gy = self._loss_grad(acts[L], labels, idx_train, lamb, g.num_dst_nodes())
        for l in range(L - 1, -1, -1):
            lay = enc.layers[l]
            sv, fs, as_ = saved[l]
            da = bwd(self, g, lay, gy, acts[l], acts[l + 1], sv, fs, as_, signed0 and l == 0, l > 0)
            if l > 0:      # the feature-dropout mask of layer l and the ReLU mask of layer l - 1 (its stored output is post-ReLU)
                gy = ops.bn_relu_bwd(da, acts[l], dz=da, drop_p=lay.feat_drop.p, drop_seed=fs)[0]
        ops.note_param_write()

    def _gat_fwd(self, g, lay, x, relu, fs, as_, signed):
        return gat_layer_fwd(g, x, lay.fc.weight, lay.attn_l, lay.attn_r, lay._num_heads, lay._out_feats, lay.negative_slope, relu,
                             lay.feat_drop.p, fs, lay.attn_drop.p, as_, signed, want_lse=True)

    def _gat_bwd(self, g, lay, gy, x, y, sv, fs, as_, signed, need_dx):
        return gat_layer_bwd(g, gy, y, sv, x, lay.fc.weight, lay.attn_l, lay.attn_r, lay._num_heads, lay._out_feats, lay.negative_slope,
                             lay.feat_drop.p, fs, lay.attn_drop.p, as_, signed, need_dx=need_dx, dw=self.grad(lay.fc.weight),
                             dattn_l=self.grad(lay.attn_l).view(-1), dattn_r=self.grad(lay.attn_r).view(-1))[0]

    def _gatv2_fwd(self, g, lay, x, relu, fs, as_, signed):
        return gatv2_layer_fwd(g, x, lay.fc_src.weight, lay.fc_src.bias, lay.fc_dst.weight, lay.fc_dst.bias, lay.attn, lay._num_heads,
                               lay._out_feats, lay.negative_slope, relu, lay.feat_drop.p, fs, lay.attn_drop.p, as_, want_lse=True)

    def _gatv2_bwd(self, g, lay, gy, x, y, sv, fs, as_, signed, need_dx):      # (the dropped input copy is among what the forward saved)
        return gatv2_layer_bwd(g, gy, sv, lay.fc_src.weight, lay.fc_dst.weight, lay.attn, lay._num_heads, lay._out_feats, lay.negative_slope,
                               lay.attn_drop.p, as_, need_dx=need_dx, dw_src=self.grad(lay.fc_src.weight), db_src=self.grad(lay.fc_src.bias),
                               dw_dst=self.grad(lay.fc_dst.weight), db_dst=self.grad(lay.fc_dst.bias), dattn=self.grad(lay.attn).view(-1))[0]

    @staticmethod
    def _gt_lins(lay):
        return lay.lin_key, lay.lin_query, lay.lin_value, lay.lin_skip

    def _gt_fwd(self, g, lay, x, relu, fs, as_, signed):
        return gt_layer_fwd(g, x, *(t for lin in self._gt_lins(lay) for t in (lin.weight, lin.bias)), lay._num_heads, lay._out_feats,
                            lay.negative_slope, relu, lay.feat_drop.p, fs, lay.attn_drop.p, as_, want_lse=True)

    def _gt_bwd(self, g, lay, gy, x, y, sv, fs, as_, signed, need_dx):         # (the dropped input copy is among what the forward saved)
        lins = self._gt_lins(lay)
        return gt_layer_bwd(g, gy, sv, *(lin.weight for lin in lins), lay._num_heads, lay._out_feats, lay.attn_drop.p, as_, need_dx=need_dx,
                            dw=[self.grad(lin.weight) for lin in lins], db=[self.grad(lin.bias) for lin in lins])[0]

    _step_gat_body = functools.partialmethod(_step_attn_body, _gat_fwd, _gat_bwd, True)
    _step_gt_body = functools.partialmethod(_step_attn_body, _gt_fwd, _gt_bwd, False)
    _step_gatv2_body = functools.partialmethod(_step_attn_body, _gatv2_fwd, _gatv2_bwd, False)


def _stream_seed(eng, tag, offset, site, on, step=None):
    """The seed of dropout site `site` in step `step` (default: the engine's current one) of TeacherEngine's stream (tag, offset); 0 when
    the stream's probability is 0 (`on` False)."""
    step = eng.step_count if step is None else step
    return _mix32(eng.base_seed ^ tag ^ _mix32(step * 131 + site + offset)) if on else 0


def get_engine(model, optimizer):
    eng = getattr(model, "_glnn_teacher_engine", None)
    if eng is None or eng.opt is not optimizer or any(a is not b for a, b in zip(eng.params, model.parameters())):
        eng = TeacherEngine(model, optimizer)
        object.__setattr__(model, "_glnn_teacher_engine", eng)
    return eng
