"""Opt-in bf16 serving of an eval-mode MLP student (csrc/gemm_bf16.hip, include/glnn_hip.h: glnn_mlp_forward_bf16).

`compile_student(model)` snapshots the student: per layer the weight rounded ONCE to bf16 and the fp32 epilogue vectors -- the
BatchNorm(eval) + bias fold of models._bn_eval_fold stays an fp32 multiply-add behind the fp32 accumulator, it is NOT folded into the
weight before rounding.  `ServedStudent.logits / log_probs` then run the whole chain as one C call per row block: hidden activations are
stored as bf16 in two reused buffers, every product runs on the bf16 MFMA with fp32 accumulation, the result is fp32.

The default everywhere stays the fp32 path; this module is reached through `compile_student`, `evaluate_mini_batch(dtype=torch.bfloat16)`
and `train_student.py --serve_dtype bfloat16` only.

`fused=True` (opt-in on top of that: `compile_student`, `compile_position_student`, `served_for`, `--serve_fused`) runs the same chain as ONE
launch per row block (csrc/mlp_fused_bf16.hip: glnn_mlp_forward_fused_bf16): a workgroup carries its tile of rows through every layer with
the hidden rows in LDS, no hidden buffers exist, and the results are the chain's bit for bit.  Only that form takes `rows`, a vector of row
ids into a resident feature matrix.

`compile_position_student(model, feats, table, g)` serves a student with position features BY NODE ID (csrc/position_serve.hip:
glnn_position_rows; docs/POSITION_SEMANTICS.md, "Serving by node id"): its input rows are assembled per block of ids from the features,
the saved position table and the graph, and either chain above runs over them unchanged.  Reached through that function and
`serve_student.py` only."""
import ctypes

import torch

from . import _lib, ops
from .models import MLP, _bn_eval_fold, _check_tail
from .train_and_eval import EVAL_BLOCK_ROWS


def _encoder_of(model):
    return getattr(model, "encoder", model)


def compile_student(model, dtype=torch.bfloat16, fused=False):
    """A ServedStudent of `model` (a models.Model wrapping an MLP, or the MLP itself), which must be in eval mode.
    fused: the one-launch form (ServedStudent.fused tells which form runs).
    NotImplementedError: not an MLP, norm_type "layer" (per-row statistics cannot ride in a per-column epilogue), more than
    MLP_MAX_LAYERS layers, training mode; with fused, a chain the one-launch form does not take (the library's reason: a hidden or
    output width above its cap, a tile the device's LDS does not hold).  Parameters on the CPU raise GlnnError like every op."""
    if dtype != torch.bfloat16:
        raise ValueError(f"compile_student: dtype {dtype} (the serving path stores torch.bfloat16; float32 is the default path itself)")
    return ServedStudent(model, _servable_encoder(model, "compile_student"), fused=fused)


def _servable_encoder(model, who):
    """The MLP of `model`, or the NotImplementedError of compile_student's docstring in the name of `who`."""
    enc = _encoder_of(model)
    if not isinstance(enc, MLP):
        raise NotImplementedError(f"{who}: {type(enc).__name__} is not an MLP student (teachers have Model.inference(dtype=...))")
    if enc.norm_type == "layer":
        raise NotImplementedError(f"{who}: norm_type 'layer' has per-row statistics; the bf16 serving path takes 'none' and 'batch'")
    _check_tail(enc)
    if len(enc.layers) > _lib.MLP_MAX_LAYERS:
        raise NotImplementedError(f"{who}: {len(enc.layers)} layers, at most {_lib.MLP_MAX_LAYERS}")
    if model.training or enc.training:
        raise NotImplementedError(f"{who}: the model is in training mode (call model.eval() first: BatchNorm running statistics, no dropout)")
    return enc


class ServedStudent:
    """The bf16 snapshot of an eval-mode MLP.  The snapshot is keyed like ops.pack_weight's cache -- (identity, torch version, data pointer)
    of every parameter and BatchNorm buffer plus ops.PARAM_EPOCH (the training engines write parameters through raw pointers) -- and is
    re-packed by the next call after a key moved; `refresh()` re-packs unconditionally.
    fused: every row block is one glnn_mlp_forward_fused_bf16 launch (tile_rows rows per workgroup) and no hidden buffer is ever allocated;
    otherwise one glnn_gemm_bf16 launch per layer through two reused hidden buffers.  Same bits either way."""

    def __init__(self, model, enc, fused=False):
        self.model, self.enc = model, enc
        self.fused = bool(fused)
        self.tile_rows = 0
        self._key = None
        self._bufs = None
        self.refresh()
        if self.fused:
            self.tile_rows, why = ops.mlp_fused_bf16_tile_rows(self.desc)
            if not self.tile_rows:
                raise NotImplementedError(f"compile_student(fused=True): {why}")

    # ---- snapshot ----
    def _tensors(self):
        ts = []
        for l, layer in enumerate(self.enc.layers):
            ts.append(layer.weight)
            if layer.bias is not None:
                ts.append(layer.bias)
            if self.enc.norm_type == "batch" and l != self.enc.num_layers - 1:
                bn = self.enc.norms[l]
                ts += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return ts

    def _current_key(self):
        return (ops.PARAM_EPOCH,) + tuple((id(t), t.data_ptr(), t._version) for t in self._tensors())

    def refresh(self):
        enc = self.enc
        ops._need_cuda(*self._tensors())
        key = self._current_key()
        self.dims = [enc.layers[0].in_features] + [layer.out_features for layer in enc.layers]
        self.weights, self.scales, self.shifts = [], [], []
        with torch.no_grad():
            for l, layer in enumerate(enc.layers):
                self.weights.append(ops.pack_weight_bf16(layer.weight))
                if l != enc.num_layers - 1 and enc.norm_type == "batch":
                    s, t = _bn_eval_fold(enc.norms[l], layer.bias)            # BN_eval(x + bias) = x s + t, fp32
                    s, t = s.float().contiguous(), t.float().contiguous()
                else:
                    s, t = None, (layer.bias.detach().float().contiguous() if layer.bias is not None else None)
                self.scales.append(s)
                self.shifts.append(t)
        d = _lib.MlpServeDesc()
        d.num_layers = len(enc.layers)
        for l, v in enumerate(self.dims):
            d.dims[l] = v
        for l in range(len(enc.layers)):
            d.w[l] = self.weights[l].data_ptr()
            d.ldw[l] = ops._ld(self.weights[l])
            d.ep_scale[l] = self.scales[l].data_ptr() if self.scales[l] is not None else None
            d.ep_shift[l] = self.shifts[l].data_ptr() if self.shifts[l] is not None else None
        self.desc = d
        self._key = key
        return self

    def _ensure(self):
        if self.model.training or self.enc.training:
            raise NotImplementedError("ServedStudent: the model went back to training mode (serving is eval-mode only)")
        if self._key != self._current_key():
            self.refresh()

    # ---- forward ----
    def _buffers(self, rows, device):
        hidden = self.dims[1:-1]
        if not hidden:
            return None, None, 8
        ld = ops.round8(max(hidden))
        b = self._bufs
        if b is None or b[0].shape[0] < rows or b[0].shape[1] != ld or b[0].device != device:
            n = 2 if len(hidden) > 1 else 1
            self._bufs = b = [torch.empty((rows, ld), dtype=torch.bfloat16, device=device) for _ in range(n)]
        return b[0], (b[1] if len(b) > 1 else None), ld

    def _run(self, feats, out, log_softmax, rows=None, check_rows=True):
        ops._need_cuda(feats, out, rows)
        self._ensure()
        if feats.dim() != 2 or feats.shape[1] != self.dims[0]:
            raise ValueError(f"ServedStudent: features must be [rows, {self.dims[0]}], got {tuple(feats.shape)}")
        if feats.dtype == torch.bfloat16:
            x = ops.as_bf16_feat(feats)
        elif feats.dtype == torch.float32:
            x = ops.as_feat(feats)
        else:
            raise ValueError(f"ServedStudent: features must be float32 or bfloat16, got {feats.dtype}")
        ids = None
        if rows is not None:
            if not self.fused:
                raise ValueError("ServedStudent: rows needs the one-launch form (compile_student(..., fused=True)); the per-layer chain "
                                 "reads consecutive rows")
            if rows.dtype != torch.int64 or rows.dim() != 1:
                raise ValueError("ServedStudent: rows must be an int64 vector")
            ids = rows.contiguous()
            if check_rows and ids.numel():
                lo, hi = torch.stack(torch.aminmax(ids)).tolist()          # (the call's one host read)
                if lo < 0 or hi >= x.shape[0]:
                    raise ValueError(f"ServedStudent: rows must lie in [0, {x.shape[0]}) (got {lo} .. {hi})")
        rows, c = (x.shape[0] if ids is None else ids.numel()), self.dims[-1]
        if out is None:
            out = torch.empty((rows, c), dtype=torch.float32, device=x.device)
        ops._mat(out, "ServedStudent out")
        if tuple(out.shape) != (rows, c):
            raise ValueError(f"ServedStudent: out must be float32 [{rows}, {c}]")
        if rows == 0:
            return out
        fused_lsm = log_softmax and c <= 64
        blk = min(rows, EVAL_BLOCK_ROWS)
        if self.fused:
            for s0 in range(0, rows, blk):
                if ids is None:
                    ops.mlp_forward_fused_bf16(self.desc, x[s0:s0 + blk], out[s0:s0 + blk], log_softmax=fused_lsm)
                else:
                    ops.mlp_forward_fused_bf16(self.desc, x, out[s0:s0 + blk], rows=ids[s0:s0 + blk], log_softmax=fused_lsm)
            if log_softmax and not fused_lsm:
                ops.log_softmax(out, out=out)
            return out
        b0, b1, ld_buf = self._buffers(blk, x.device)
        lib = _lib.lib()
        for s0 in range(0, rows, blk):
            xs, os_ = x[s0:s0 + blk], out[s0:s0 + blk]
            rc = lib.glnn_mlp_forward_bf16(ctypes.byref(self.desc), ops._p(xs), ops._ld(xs), ops._dtype_code(xs), xs.shape[0], ops._p(b0),
                                           ops._p(b1), ld_buf, ops._p(os_), ops._ld(os_), 1 if fused_lsm else 0, ops._stream())
            _lib.check(rc, "glnn_mlp_forward_bf16")
        if log_softmax and not fused_lsm:
            ops.log_softmax(out, out=out)
        return out

    def logits(self, feats, out=None, rows=None, check_rows=True):
        """fp32 logits [rows, C] of fp32 or bf16 features [rows, dims[0]] (rows in blocks of EVAL_BLOCK_ROWS; a row's result does not
        depend on the blocking).  rows (the one-launch form only; ValueError otherwise): an int64 device vector of row ids into `feats`
        (repeats allowed) -- the result is [len(rows), C], row b that of feats[rows[b]], and no gathered copy is made.  check_rows=False
        skips the range check and its host read: the caller then vouches for the ids (one outside feats is never used as an address;
        its row is computed from an all-zero input)."""
        return self._run(feats, out, False, rows, check_rows)

    def log_probs(self, feats, out=None, rows=None, check_rows=True):
        """fp32 log_softmax(logits); for C <= 64 it is the last product's epilogue and the logits never reach memory."""
        return self._run(feats, out, True, rows, check_rows)


POSITION_BLOCK_ROWS = 65536        # ids per assembled block of a ServedPositionStudent


def compile_position_student(model, feats, table, g=None, dtype=torch.bfloat16, fused=False):
    """A ServedPositionStudent: an eval-mode MLP student with position features (docs/POSITION_SEMANTICS.md, "Serving by node id"), served
    by node id from the node features `feats` [N, F] (fp32, or bf16 for the bf16 chain; on the GPU), a position.PositionTable of width D
    and, where a node may lack a table row, the graph `g` -- the [N, F + D] matrix training concatenated is never built.
    dtype: torch.bfloat16 (the ServedStudent chain) or torch.float32 (model.inference + ops.log_softmax).
    fused (bfloat16 only; ValueError otherwise): the assembled block goes through the one-launch form -- two launches per block, not 1 + L.
    Refused: whatever compile_student refuses (NotImplementedError); a first layer that is not F + D wide, a table with unseen nodes (or
    fewer nodes than feats has rows) without g, a graph that does not have feats' rows (ValueError)."""
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"compile_position_student: dtype {dtype} (torch.bfloat16 or torch.float32)")
    if fused and dtype != torch.bfloat16:
        raise ValueError("compile_position_student: fused=True is a form of the bfloat16 chain")
    enc = _servable_encoder(model, "compile_position_student")
    return ServedPositionStudent(model, enc, feats, table, g, dtype, fused)


class ServedPositionStudent:
    """logits / log_probs of a batch of node ids.  Per block of POSITION_BLOCK_ROWS ids one ops.position_rows launch assembles
    [x[v] | pos(v)] into a reused buffer -- bf16 [blk, round8(F + D)] or fp32 [blk, round4(F + D)] -- and the existing chain runs over
    it: a ServedStudent (bf16), or model.inference and ops.log_softmax (fp32).  A row's result does not depend on the blocking or on the
    other ids of the call."""

    def __init__(self, model, enc, feats, table, g, dtype, fused=False):
        ops._need_cuda(feats, table.rows, table.node_ids)
        if feats.dim() != 2 or feats.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"compile_position_student: features must be a float32 or bfloat16 matrix, got {feats.dtype} {tuple(feats.shape)}")
        if feats.dtype == torch.bfloat16 and dtype != torch.bfloat16:
            raise ValueError("compile_position_student: bfloat16 features need dtype=torch.bfloat16 (the kernel does not widen features)")
        n, f = feats.shape
        if n < table.num_nodes:
            raise ValueError(f"compile_position_student: features have {n} rows, the table was fitted against {table.num_nodes} nodes")
        if enc.layers[0].in_features != f + table.dim:
            raise ValueError(f"compile_position_student: the model's first layer takes {enc.layers[0].in_features} columns, features and "
                             f"table give {f} + {table.dim}")
        if g is None and (table.has_unseen or n > table.num_nodes):
            raise ValueError("compile_position_student: the table has no row for some nodes; their position is the mean over their "
                             "in-neighbours, which needs the graph g")
        if g is not None:
            ops._need_cuda(g.indptr, g.indices)
            if g.n_dst != g.n_src or g.num_nodes() != n:
                raise ValueError(f"compile_position_student: g must be the square graph over the {n} rows of the features")
        self.model, self.enc, self.g, self.dtype = model, enc, g, dtype
        self.x = ops.as_bf16_feat(feats) if feats.dtype == torch.bfloat16 else ops._mat(feats, "compile_position_student features")
        self.z, self.slot = table.rows, table.slot(n)
        self.num_nodes, self.width = n, f + table.dim
        self.served = ServedStudent(model, enc, fused=fused) if dtype == torch.bfloat16 else None
        self.fused = bool(fused)
        self._block = None

    def _buffer(self, rows):
        b = self._block
        if b is None or b.shape[0] < rows:
            make = ops.bf16_empty if self.dtype == torch.bfloat16 else ops.feat_empty
            self._block = b = make(rows, self.width, self.x.device)
        return b

    def _run(self, ids, out, log_softmax, check_ids):
        ops._need_cuda(ids, out)
        if ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError("ServedPositionStudent: ids must be an int64 vector")
        ids = ids.contiguous()
        rows, c = ids.numel(), self.enc.layers[-1].out_features
        if check_ids and rows:
            lo, hi = torch.stack(torch.aminmax(ids)).tolist()          # (the call's one host read)
            if lo < 0 or hi >= self.num_nodes:
                raise ValueError(f"ServedPositionStudent: ids must lie in [0, {self.num_nodes}) (got {lo} .. {hi})")
        if self.served is None and (self.model.training or self.enc.training):
            raise NotImplementedError("ServedPositionStudent: the model went back to training mode (serving is eval-mode only)")
        if out is None:
            out = torch.empty((rows, c), dtype=torch.float32, device=self.x.device)
        ops._mat(out, "ServedPositionStudent out")
        if tuple(out.shape) != (rows, c):
            raise ValueError(f"ServedPositionStudent: out must be float32 [{rows}, {c}]")
        blk = min(rows, POSITION_BLOCK_ROWS)
        buf = self._buffer(blk) if rows else None
        with torch.no_grad():
            for s0 in range(0, rows, blk):
                sub = ids[s0:s0 + blk]
                block = ops.position_rows(sub, self.x, self.z, self.slot, g=self.g, out=buf)
                os_ = out[s0:s0 + blk]
                if self.served is not None:
                    self.served._run(block, os_, log_softmax)
                elif log_softmax:
                    ops.log_softmax(self.model.inference(None, block), out=os_)
                else:
                    os_.copy_(self.model.inference(None, block))
        return out

    def logits(self, ids, out=None, check_ids=True):
        """fp32 logits [len(ids), C] of the nodes `ids` (an int64 device vector; repeats allowed).  check_ids=False skips the range check
        and its host read: the caller then vouches that every id is a node."""
        return self._run(ids, out, False, check_ids)

    def log_probs(self, ids, out=None, check_ids=True):
        """fp32 log_softmax(logits)."""
        return self._run(ids, out, True, check_ids)


def served_for(model, fused=False):
    """The ServedStudent cached on `model` (compiled on first use; it re-packs itself when a parameter moved); the one-launch form has a
    cache slot of its own."""
    attr = "_served_student_fused" if fused else "_served_student"
    s = model.__dict__.get(attr)
    if s is None:
        s = compile_student(model, fused=fused)
        model.__dict__[attr] = s
    return s
