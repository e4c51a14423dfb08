"""Opt-in bf16 serving of an eval-mode MLP student (csrc/gemm_bf16.hip, include/glnn_hip.h: glnn_mlp_forward_bf16).

`compile_student(model)` snapshots the student: per layer the weight rounded ONCE to bf16 and the fp32 epilogue vectors -- the
BatchNorm(eval) + bias fold of models._bn_eval_fold stays an fp32 multiply-add behind the fp32 accumulator, it is NOT folded into the
weight before rounding.  `ServedStudent.logits / log_probs` then run the whole chain as one C call per row block: hidden activations are
stored as bf16 in two reused buffers, every product runs on the bf16 MFMA with fp32 accumulation, the result is fp32.

The default everywhere stays the fp32 path; this module is reached through `compile_student`, `evaluate_mini_batch(dtype=torch.bfloat16)`
and `train_student.py --serve_dtype bfloat16` only."""
import ctypes

import torch

from . import _lib, ops
from .models import MLP, _bn_eval_fold, _check_tail
from .train_and_eval import EVAL_BLOCK_ROWS


def _encoder_of(model):
    return getattr(model, "encoder", model)


def compile_student(model, dtype=torch.bfloat16):
    """A ServedStudent of `model` (a models.Model wrapping an MLP, or the MLP itself), which must be in eval mode.
    NotImplementedError: not an MLP, norm_type "layer" (per-row statistics cannot ride in a per-column epilogue), more than
    MLP_MAX_LAYERS layers, training mode.  Parameters on the CPU raise GlnnError like every op."""
    if dtype != torch.bfloat16:
        raise ValueError(f"compile_student: dtype {dtype} (the serving path stores torch.bfloat16; float32 is the default path itself)")
    enc = _encoder_of(model)
    if not isinstance(enc, MLP):
        raise NotImplementedError(f"compile_student: {type(enc).__name__} is not an MLP student (teachers have Model.inference(dtype=...))")
    if enc.norm_type == "layer":
        raise NotImplementedError("compile_student: norm_type 'layer' has per-row statistics; the bf16 serving path takes 'none' and 'batch'")
    _check_tail(enc)
    if len(enc.layers) > _lib.MLP_MAX_LAYERS:
        raise NotImplementedError(f"compile_student: {len(enc.layers)} layers, at most {_lib.MLP_MAX_LAYERS}")
    if model.training or enc.training:
        raise NotImplementedError("compile_student: the model is in training mode (call model.eval() first: BatchNorm running statistics, no dropout)")
    return ServedStudent(model, enc)


class ServedStudent:
    """The bf16 snapshot of an eval-mode MLP.  The snapshot is keyed like ops.pack_weight's cache -- (identity, torch version, data pointer)
    of every parameter and BatchNorm buffer plus ops.PARAM_EPOCH (the training engines write parameters through raw pointers) -- and is
    re-packed by the next call after a key moved; `refresh()` re-packs unconditionally."""

    def __init__(self, model, enc):
        self.model, self.enc = model, enc
        self._key = None
        self._bufs = None
        self.refresh()

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

    def _run(self, feats, out, log_softmax):
        ops._need_cuda(feats, out)
        self._ensure()
        if feats.dim() != 2 or feats.shape[1] != self.dims[0]:
            raise ValueError(f"ServedStudent: features must be [rows, {self.dims[0]}], got {tuple(feats.shape)}")
        if feats.dtype == torch.bfloat16:
            x = ops.as_bf16_feat(feats)
        elif feats.dtype == torch.float32:
            x = ops.as_feat(feats)
        else:
            raise ValueError(f"ServedStudent: features must be float32 or bfloat16, got {feats.dtype}")
        rows, c = x.shape[0], self.dims[-1]
        if out is None:
            out = torch.empty((rows, c), dtype=torch.float32, device=x.device)
        ops._mat(out, "ServedStudent out")
        if tuple(out.shape) != (rows, c):
            raise ValueError(f"ServedStudent: out must be float32 [{rows}, {c}]")
        if rows == 0:
            return out
        fused_lsm = log_softmax and c <= 64
        blk = min(rows, EVAL_BLOCK_ROWS)
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

    def logits(self, feats, out=None):
        """fp32 logits [rows, C] of fp32 or bf16 features [rows, dims[0]] (rows in blocks of EVAL_BLOCK_ROWS; a row's result does not
        depend on the blocking)."""
        return self._run(feats, out, False)

    def log_probs(self, feats, out=None):
        """fp32 log_softmax(logits); for C <= 64 it is the last product's epilogue and the logits never reach memory."""
        return self._run(feats, out, True)


def served_for(model):
    """The ServedStudent cached on `model` (compiled on first use; it re-packs itself when a parameter moved)."""
    s = model.__dict__.get("_served_student")
    if s is None:
        s = compile_student(model)
        model.__dict__["_served_student"] = s
    return s
