"""Thin torch-tensor wrappers over the C ABI (include/glnn_hip.h).  torch is plumbing here: it owns
device memory and the current HIP stream; all arithmetic is in libglnn_hip.so.  Every function
raises on CPU tensors -- there is no fallback path."""
import ctypes

import torch

from . import _lib

AGG_SUM, AGG_SAGE_GCN = 0, 1
LOSS_NLL, LOSS_KL = 0, 1

# Optional per-launch timing (bench.py's roofline leg): a list that receives
# (kernel_name, info_dict, start_event, end_event) for every aggregation / GEMM launch, recorded on the
# stream the kernel is launched on.  None = no events (the default).
_TIMING = None


def set_timing(collector):
    global _TIMING
    _TIMING = collector


class _Timed:
    __slots__ = ("name", "info", "s")

    def __init__(self, name, **info):
        self.name, self.info, self.s = name, info, None

    def __enter__(self):
        if _TIMING is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *exc):
        if self.s is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            _TIMING.append((self.name, self.info, self.s, e))


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream of the current device as a C pointer.  torch.cuda.current_stream() builds a Stream object and
    resolves the device through several Python layers (~8 us per call: 50 us of host time per sampled batch); the raw getter
    torch itself uses for its compiled kernels returns the same handle in well under a microsecond."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return ctypes.c_void_p(_RAW_STREAM(_RAW_DEVICE()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.GlnnError("glnn_amd.ops: tensors must live on the GPU (HIP path only, no CPU fallback)")


def _vec(t, n, name, dtype=torch.float32):
    if t is None:
        return None
    if t.dtype != dtype or t.dim() != 1 or t.numel() < n or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype} vector with >= {n} elements")
    return t


def _mat(t, name):
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected 2-D float32 row-major tensor")
    return t


def _ld(t):
    # the stride of a size-1 dimension is arbitrary in torch/numpy: a single row is as wide as its columns
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def round4(d):
    return (d + 3) // 4 * 4


def feat_empty(n, d, device, zero=False):
    """[n, d] fp32 view of an [n, round4(d)] buffer: rows 16-byte aligned as the float4 kernels need."""
    ld = round4(d)
    buf = (torch.zeros if zero else torch.empty)((n, ld), dtype=torch.float32, device=device)
    return buf[:, :d]


DTYPE_F32, DTYPE_BF16 = 0, 1            # GLNN_DTYPE_* of include/glnn_hip.h


def round8(d):
    return (d + 7) // 8 * 8


def bf16_empty(n, d, device, zero=False):
    """[n, d] bf16 view of an [n, round8(d)] buffer: rows 16-byte aligned as the bf16 kernels need (a lane moves 8 bf16).  The counterpart
    of feat_empty for the matrices the bf16 teacher forward gathers; a plain allocation (no ops.placed_for_gather placement)."""
    buf = (torch.zeros if zero else torch.empty)((n, round8(d)), dtype=torch.bfloat16, device=device)
    return buf[:, :d]


def _bf16_mat(t, name):
    if t.dtype != torch.bfloat16 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected 2-D bfloat16 row-major tensor")
    return t


def as_bf16_feat(t):
    """t itself if its layout suits the bf16 kernels (leading dimension a multiple of 8 elements, 16-byte aligned base), else a padded copy
    (bf16_empty, padding zeroed)."""
    _bf16_mat(t, "as_bf16_feat")
    if _ld(t) % 8 == 0 and _ld(t) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    out = bf16_empty(t.shape[0], t.shape[1], t.device, zero=True)
    out.copy_(t)
    return out


def to_bf16(x, out=None):
    """glnn_cast_f32_bf16: x [n, d] fp32 -> bf16, round to nearest even (bit for bit x.to(torch.bfloat16); NaN stays NaN).  Returns a
    bf16_empty view (or fills `out`, a bf16 [n, d] tensor whose leading dimension is a multiple of 8)."""
    _need_cuda(x, out)
    _mat(x, "to_bf16 x")
    n, d = x.shape
    if out is None:
        out = bf16_empty(n, d, x.device)
    elif tuple(out.shape) != (n, d) or _ld(_bf16_mat(out, "to_bf16 out")) % 8:
        raise ValueError("to_bf16: out must be a bf16 [n, d] tensor with a leading dimension that is a multiple of 8")
    if n == 0 or d == 0:
        return out
    rc = _lib.lib().glnn_cast_f32_bf16(_p(x), _ld(x), n, d, _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_cast_f32_bf16")
    return out


def _out_like(out, out_dtype, default, n, d, device, name):
    """The output of a bf16-input launch: `out` (whose dtype then decides), else a fresh matrix of out_dtype (default: `default`)."""
    if out_dtype is not None and out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{name}: out_dtype must be torch.float32 or torch.bfloat16")
    if out is None:
        dt = default if out_dtype is None else out_dtype
        return bf16_empty(n, d, device) if dt == torch.bfloat16 else feat_empty(n, d, device)
    if out_dtype is not None and out.dtype != out_dtype:
        raise ValueError(f"{name}: out is {out.dtype}, out_dtype {out_dtype}")
    if out.dtype == torch.bfloat16:
        _bf16_mat(out, name)
    else:
        _mat(out, name)
    if out.shape[0] < n or out.shape[1] != d:
        raise ValueError(f"{name}: out must hold {n} rows of {d} columns")
    return out


def _dtype_code(t):
    return DTYPE_BF16 if t.dtype == torch.bfloat16 else DTYPE_F32


# ---- int8 activation storage of the SAGE teacher forward (csrc/sage_i8.hip, docs/INT8_INFERENCE_SEMANTICS.md) ----------------------
DTYPE_I8 = 2                            # GLNN_DTYPE_I8
I8_MAX_WIDTH = 256


def round16(d):
    return (d + 15) // 16 * 16


def int8_rows_ld(d):
    """Bytes of one int8 row of d columns: the values, zero padding, and the row's fp32 scale in the last four."""
    return round16(d + 4)


def int8_rows_empty(n, d, device, zero=False):
    """An [n, round16(d + 4)] torch.int8 matrix for n int8 rows of d columns (include/glnn_hip.h: bytes [0, d) the values, [d, ld - 4) zero,
    the last four the row's fp32 scale); a plain allocation with a 16-byte aligned base."""
    if not 1 <= d <= I8_MAX_WIDTH:
        raise ValueError(f"int8_rows_empty: int8 rows hold 1..{I8_MAX_WIDTH} columns (got {d})")
    return (torch.zeros if zero else torch.empty)((n, int8_rows_ld(d)), dtype=torch.int8, device=device)


def _i8_rows(q, d, name):
    """q as the int8 rows of a d-column matrix, or ValueError."""
    if q.dtype != torch.int8 or q.dim() != 2 or q.shape[1] != int8_rows_ld(d) or (q.shape[0] > 1 and q.stride(0) != q.shape[1]) \
            or (q.shape[1] > 1 and q.stride(1) != 1) or q.data_ptr() % 16:
        raise ValueError(f"{name}: expected int8 rows of {d} columns: a 16-byte aligned torch.int8 [n, {int8_rows_ld(d)}] matrix "
                         "(ops.to_int8_rows)")
    return q


def to_int8_rows(x, out=None):
    """glnn_quant_rows_i8: x [n, d] fp32 -> int8 rows (per row s = max|x| / 127, q = clamp(rint(x * (127 / max|x|)), -127, 127); a zero row
    has s = 0, a row with a NaN or an Inf s = NaN and q = 0).  Returns an int8_rows_empty matrix (or fills `out`, one of those)."""
    _need_cuda(x, out)
    _mat(x, "to_int8_rows x")
    n, d = x.shape
    if out is None:
        out = int8_rows_empty(n, d, x.device)
    elif out.shape[0] != n:
        raise ValueError("to_int8_rows: out must hold the rows of x")
    _i8_rows(out, d, "to_int8_rows out")
    if n == 0:
        return out
    with _Timed("quant_rows_i8", n=n, d=d):
        rc = _lib.lib().glnn_quant_rows_i8(_p(x), _ld(x), n, d, _p(out), out.shape[1], _stream())
    _lib.check(rc, "glnn_quant_rows_i8")
    return out


def int8_rows_scale(q):
    """The per-row scales of int8 rows: the fp32 [n] view of each row's last four bytes."""
    _need_cuda(q)
    if q.dtype != torch.int8 or q.dim() != 2 or q.shape[1] % 16 or not q.is_contiguous():
        raise ValueError("int8_rows_scale: expected contiguous int8 rows (ops.to_int8_rows)")
    return q.view(torch.float32)[:, -1]


def from_int8_rows(q, d):
    """int8 rows -> fp32 [n, d], q * s in plain torch (tests and users; no kernel reads the result)."""
    _need_cuda(q)
    _i8_rows(q, d, "from_int8_rows")
    return q[:, :d].to(torch.float32) * int8_rows_scale(q)[:, None]


def _i8_out(out, out_dtype, n, d, device, name):
    if out_dtype is not None and out_dtype not in (torch.float32, torch.int8):
        raise ValueError(f"{name}: out_dtype must be torch.float32 or torch.int8")
    if out is None:
        return int8_rows_empty(n, d, device) if out_dtype == torch.int8 else feat_empty(n, d, device)
    if out_dtype is not None and out.dtype != out_dtype:
        raise ValueError(f"{name}: out is {out.dtype}, out_dtype {out_dtype}")
    if out.dtype == torch.int8:
        if _i8_rows(out, d, name).shape[0] != n:
            raise ValueError(f"{name}: out must hold {n} int8 rows")
        return out
    _mat(out, name)
    if out.shape[0] < n or out.shape[1] != d:
        raise ValueError(f"{name}: out must hold {n} rows of {d} columns")
    return out


def _i8_graph(indptr, indices, x, d, n_dst, x_self, name):
    _need_cuda(indptr, indices, x, x_self)
    _i8_rows(x, d, f"{name} x")
    if x_self is None:
        x_self = x
    else:
        _i8_rows(x_self, d, f"{name} x_self")
    if x_self.shape[0] < n_dst:
        raise ValueError(f"{name}: x_self must hold the n_dst destination rows")
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise ValueError(f"{name}: indptr must be int64 and indices int32")
    return x_self


def spmm_sage_gcn_i8(indptr, indices, x, d, n_dst, ep_scale=None, ep_shift=None, relu=False, out=None, x_self=None, out_dtype=None):
    """glnn_spmm_sage_gcn_i8: epi((A x + x_self) / (deg + 1)) over int8 rows x (d columns, d <= 256; x_self defaults to x's first n_dst
    rows), fp32 sums.  The output is `out` (its dtype decides), else fresh: fp32 [n_dst, d] (default) or int8 rows (out_dtype=torch.int8:
    each finished row quantised in the launch)."""
    x_self = _i8_graph(indptr, indices, x, d, n_dst, x_self, "spmm_sage_gcn_i8")
    _need_cuda(out)
    out = _i8_out(out, out_dtype, n_dst, d, x.device, "spmm_sage_gcn_i8 out")
    i8 = out.dtype == torch.int8
    with _Timed("spmm_i8", d=d, n_dst=n_dst):
        rc = _lib.lib().glnn_spmm_sage_gcn_i8(
            _p(indptr), _p(indices), n_dst, x.shape[0], _p(x), x.shape[1], d, _p(x_self), x_self.shape[1],
            _p(_vec(ep_scale, d, "ep_scale")), _p(_vec(ep_shift, d, "ep_shift")), 1 if relu else 0,
            _p(out), out.shape[1] if i8 else _ld(out), DTYPE_I8 if i8 else DTYPE_F32, _stream())
    _lib.check(rc, "glnn_spmm_sage_gcn_i8")
    return out


def sage_fused_i8(indptr, indices, x, d_in, n_dst, w, ep_scale=None, ep_shift=None, relu=False, out=None, x_self=None, w_packed=None,
                  w_next=None, out_next=None, want_out=True, tile_order=None):
    """glnn_sage_fused_i8: sage_fused over int8 rows x (d_in columns): the fp32 aggregate tile feeds the same fp32 MFMA passes.  Returns
    out [n_dst, d_out] fp32, or (out or None, out_next [n_dst, d_out2] fp32) with the chained projection w_next.  Both outputs are fp32: a
    projection the next layer gathers goes through to_int8_rows."""
    x_self = _i8_graph(indptr, indices, x, d_in, n_dst, x_self, "sage_fused_i8")
    _need_cuda(w, out, w_next, out_next, tile_order)
    _mat(w, "sage_fused_i8 w")
    d_out = w.shape[0]
    if w.shape[1] != d_in:
        raise ValueError("sage_fused_i8: weight must be [d_out, d_in]")
    if tile_order is not None and (tile_order.dtype != torch.int32 or not tile_order.is_contiguous() or tile_order.numel() != (n_dst + 31) // 32):
        raise ValueError("sage_fused_i8: tile_order must be a contiguous int32 permutation of the ceil(n_dst / 32) tile ids")
    if w_packed is None:
        w_packed = pack_weight(w)
    if out is not None or want_out or w_next is None:
        out = _i8_out(out, torch.float32, n_dst, d_out, x.device, "sage_fused_i8 out")
    w2p, d_out2 = None, 0
    if w_next is not None:
        if w_next.shape[1] != d_out:
            raise ValueError("sage_fused_i8: w_next must be [d_out2, d_out]")
        w2p, d_out2 = pack_weight(w_next), w_next.shape[0]
        out_next = _i8_out(out_next, torch.float32, n_dst, d_out2, x.device, "sage_fused_i8 out_next")
    with _Timed("sage_fused_i8", d=d_in, n_dst=n_dst, d_out=d_out, d_chain=d_out2, d_written=(d_out if out is not None else 0) + d_out2):
        rc = _lib.lib().glnn_sage_fused_i8(
            _p(indptr), _p(indices), n_dst, x.shape[0], _p(x), x.shape[1], d_in, _p(x_self), x_self.shape[1],
            _p(w_packed), d_out, _p(_vec(ep_scale, d_out, "ep_scale")), _p(_vec(ep_shift, d_out, "ep_shift")), 1 if relu else 0,
            _p(out), _ld(out) if out is not None else 0, _p(w2p), d_out2, _p(out_next), _ld(out_next) if out_next is not None else 0,
            _p(tile_order), _stream())
    _lib.check(rc, "glnn_sage_fused_i8")
    return out if w_next is None else (out, out_next)


_RANDPERM_LOCK = __import__("threading").Lock()


def randperm_cpu(n):
    """torch.randperm(n) from the global CPU generator (what the reference draws its mini-batches with, train_and_eval.py:66), issued
    with ONE intra-op thread: the CPU kernel is a serial shuffle, so the permutation is the same for any thread count
    (scripts/probe_randperm.py), but with the 128-thread pool of a GPU host awake the 0.3 ms job took 7-17 ms -- as long as the 177
    optimiser steps of an ogbn-arxiv pass.  Side effect, by design: torch's process-global intra-op thread count is 1 for the ~0.3 ms of
    the call (serialised by a lock; a CPU op running concurrently in another thread of the host program sees one thread meanwhile)."""
    with _RANDPERM_LOCK:
        k = torch.get_num_threads()
        if k <= 1:
            return torch.randperm(n)
        torch.set_num_threads(1)
        try:
            return torch.randperm(n)
        finally:
            torch.set_num_threads(k)


_PADDED = []            # [(weakref to the source tensor, (version, data_ptr, strides), padded copy)], most recent first, <= 2 live entries


def _pad_key(t):
    try:
        ver = t._version
    except RuntimeError:          # tensors created under torch.inference_mode() have no version counter: never cached
        return None
    return (ver, t.data_ptr(), tuple(t.stride()), tuple(t.shape))


def clear_pad_cache():
    """Drop the padded copies as_feat remembers (they are only ever handed out for the very same, unmodified source tensor)."""
    _PADDED.clear()


def as_feat(t):
    """Return t itself if its layout suits the float4 kernels, else a padded copy.
    The copy of a LARGE matrix is remembered while the very same tensor object is passed again unmodified (identity + torch's in-place
    version counter + data pointer and strides): the reference hands the same `feats` to every epoch's train / evaluate call, and re-padding
    a wide unaligned feature matrix (cora 1433, citeseer 3703 columns) was a zero fill and a copy per call.  Writes that bypass the version
    counter -- raw-pointer writes by this library's own kernels, `.data` assignments -- are NOT seen: such tensors are never inputs of
    as_feat in this package (parameters skip the cache through requires_grad).  Entries whose source died are evicted on every call.
    The result of a padding call is READ-ONLY for the caller (it may be handed out again); every call site in this package only reads it."""
    _mat(t, "as_feat")
    if t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    _PADDED[:] = [e for e in _PADDED if e[0]() is not None]
    key = _pad_key(t) if (t.numel() >= (1 << 20) and not t.requires_grad) else None
    if key is not None:
        for i, (ref, k, pad) in enumerate(_PADDED):
            if ref() is t and k == key and pad.device == t.device:
                if i:
                    _PADDED.insert(0, _PADDED.pop(i))
                return pad
    out = feat_empty(t.shape[0], t.shape[1], t.device, zero=True)
    out.copy_(t)
    if key is not None:
        import weakref
        _PADDED[:] = [e for e in _PADDED if e[0]() is not t][:1]
        _PADDED.insert(0, (weakref.ref(t), key, out))
    return out


# ---------------------------------------------------------------------------------------------
class HubPlan:
    """glnn_hub_plan for one (indptr, n_dst) launch range: the rows of more than glnn_hub_row_threshold() in-edges, cut into segments of
    glnn_hub_segment_edges() edges that one workgroup each gathers in front of the aggregation (include/glnn_hip.h, ABI 9).  Built once
    per range (one pass over the degrees and ONE host read-back: the segment count) and reused by every launch over that range; the slab
    is scratch of the launching stream (one stream at a time)."""

    def __init__(self, indptr, n_dst):
        thr, seg = _lib.lib().glnn_hub_row_threshold(), _lib.lib().glnn_hub_segment_edges()
        deg = indptr[1:n_dst + 1] - indptr[:n_dst]
        rows = torch.nonzero(deg > thr).flatten()
        self.n_hub = int(rows.numel())
        self.rows = rows.contiguous()
        segs = (deg[rows] + (seg - 1)) // seg
        self.seg_ptr = torch.zeros(self.n_hub + 1, dtype=torch.int32, device=indptr.device)
        if self.n_hub:
            self.seg_ptr[1:] = segs.cumsum(0).to(torch.int32)
        self.n_seg = int(self.seg_ptr[-1].item()) if self.n_hub else 0
        self.hub_edges = int(deg[rows].sum().item()) if self.n_hub else 0
        self.slab = None
        self.desc = _lib.HubPlanDesc()

    def desc_for(self, d, device):
        """The C descriptor with a slab wide enough for rows of d floats (None when the range has no hub row)."""
        if self.n_hub == 0:
            return None
        ld = (d + 3) // 4 * 4
        if self.slab is None or self.slab.shape[1] < ld:
            self.slab = torch.empty(8 * self.n_seg, ld, dtype=torch.float32, device=device)      # (row 8 s + w: wave w's piece of segment s)
        p = self.desc
        p.rows, p.seg_ptr, p.n_hub, p.n_seg = _p(self.rows), _p(self.seg_ptr), self.n_hub, self.n_seg
        p.slab, p.ld_slab, p.slab_rows = _p(self.slab), self.slab.shape[1], self.slab.shape[0]
        return ctypes.byref(p)


def hub_plan(indptr, n_dst):
    """A HubPlan for launches over rows [0, n_dst) of `indptr`, or None when it has no hub row (cache it per range: it costs a host sync)."""
    _need_cuda(indptr)
    plan = HubPlan(indptr, int(n_dst))
    return plan if plan.n_hub else None


def spmm(indptr, indices, x, n_dst, mode, row_scale=None, col_scale=None, ep_scale=None, ep_shift=None,
         relu=False, out=None, x_self=None, self_rows=None, hub=None, chunks=None, out_dtype=None):
    """K1/K2 glnn_spmm_csr_f32.  x: [n_src, d] feature tensor (see as_feat); returns [n_dst, d].
    chunks (ChunkSignals.launch(...), SAGE_GCN, d <= 256): ONE launch over the chunks of the row range -- `out` (and `x_self`, unless
    self_rows is given) are then WHOLE buffers addressed through the descriptor's per-chunk rows, and every chunk signals its completion.
    x_self (SAGE_GCN only): the destination rows' own features, default x[:n_dst] (a row shard passes its slice).
    self_rows (SAGE_GCN only, int64 [n_dst]): destination v's own row is x_self[self_rows[v]] (global-id blocks).
    hub (optional HubPlan of (indptr, n_dst)): the hub rows' segments are gathered by one workgroup each first (same result bit for bit).
    bf16 x (and x_self): glnn_spmm_csr_bf16, fp32 sums; the output is `out`'s dtype, else out_dtype (default bf16); no hub / chunks."""
    _need_cuda(indptr, indices, x, row_scale, col_scale, ep_scale, ep_shift, out, x_self, self_rows)
    if x.dtype == torch.bfloat16:
        return _spmm_bf16(indptr, indices, x, n_dst, mode, row_scale, col_scale, ep_scale, ep_shift, relu, out, x_self, self_rows, hub,
                          chunks, out_dtype)
    if out_dtype not in (None, torch.float32):
        raise ValueError("spmm: fp32 rows give an fp32 output (a bf16 output needs bf16 rows: ops.to_bf16)")
    x = as_feat(x)
    if self_rows is not None and (self_rows.dtype != torch.int64 or not self_rows.is_contiguous() or self_rows.numel() < n_dst):
        raise ValueError("spmm: self_rows must be a contiguous int64 vector of n_dst row ids")
    if x_self is None:
        x_self = x
    elif (self_rows is None and chunks is None and x_self.shape[0] < n_dst) or x_self.shape[1] != x.shape[1]:
        raise ValueError("spmm: x_self must hold n_dst rows of the same width as x")
    if chunks is not None and (out is None or mode != AGG_SAGE_GCN):
        raise ValueError("spmm(chunks=...): SAGE_GCN with the whole output buffer given (it is addressed by the chunks' rows)")
    n_src, d = x.shape
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise ValueError("spmm: indptr must be int64 and indices int32")
    if out is None:
        out = feat_empty(n_dst, d, x.device)
    _mat(out, "spmm out")
    with _Timed("spmm", d=d, n_dst=n_dst, mode=mode):
        rc = _spmm_call(indptr, indices, n_dst, n_src, x, d, mode, row_scale, col_scale, ep_scale, ep_shift, relu, out,
                        as_feat(x_self), self_rows, hub, chunks)
    _lib.check(rc, "glnn_spmm_csr_f32")
    return out


def _spmm_call(indptr, indices, n_dst, n_src, x, d, mode, row_scale, col_scale, ep_scale, ep_shift, relu, out, x_self,
               self_rows=None, hub=None, chunks=None):
    args = (_p(indptr), _p(indices), n_dst, n_src, _p(x), _ld(x), d, mode,
            _p(_vec(row_scale, n_dst, "row_scale")), _p(_vec(col_scale, n_src, "col_scale")),
            _p(x_self) if mode == AGG_SAGE_GCN else None, _ld(x_self), _p(self_rows),
            _p(_vec(ep_scale, d, "ep_scale")), _p(_vec(ep_shift, d, "ep_shift")), 1 if relu else 0,
            _p(out), _ld(out))
    plan = hub.desc_for(d, x.device) if hub is not None else None
    if chunks is not None:
        return _lib.lib().glnn_spmm_csr_chunks_f32(*args, plan, ctypes.byref(chunks), _stream())
    if plan is not None:
        return _lib.lib().glnn_spmm_csr_plan_f32(*args, plan, _stream())
    return _lib.lib().glnn_spmm_csr_f32(*args, _stream())


def _spmm_bf16(indptr, indices, x, n_dst, mode, row_scale, col_scale, ep_scale, ep_shift, relu, out, x_self, self_rows, hub, chunks,
               out_dtype):
    if hub is not None or chunks is not None:
        raise ValueError("spmm: bf16 rows take neither a hub plan nor chunks")
    x = as_bf16_feat(x)
    if self_rows is not None and (self_rows.dtype != torch.int64 or not self_rows.is_contiguous() or self_rows.numel() < n_dst):
        raise ValueError("spmm: self_rows must be a contiguous int64 vector of n_dst row ids")
    if x_self is None:
        x_self = x
    elif x_self.dtype != torch.bfloat16 or (self_rows is None and x_self.shape[0] < n_dst) or x_self.shape[1] != x.shape[1]:
        raise ValueError("spmm: x_self must be bf16 like x and hold n_dst rows of the same width")
    n_src, d = x.shape
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise ValueError("spmm: indptr must be int64 and indices int32")
    out = _out_like(out, out_dtype, torch.bfloat16, n_dst, d, x.device, "spmm out")
    x_self = as_bf16_feat(x_self)
    with _Timed("spmm_bf16", d=d, n_dst=n_dst, mode=mode):
        rc = _lib.lib().glnn_spmm_csr_bf16(
            _p(indptr), _p(indices), n_dst, n_src, _p(x), _ld(x), d, mode,
            _p(_vec(row_scale, n_dst, "row_scale")), _p(_vec(col_scale, n_src, "col_scale")),
            _p(x_self) if mode == AGG_SAGE_GCN else None, _ld(x_self), _p(self_rows),
            _p(_vec(ep_scale, d, "ep_scale")), _p(_vec(ep_shift, d, "ep_shift")), 1 if relu else 0,
            _p(out), _ld(out), _dtype_code(out), _stream())
    _lib.check(rc, "glnn_spmm_csr_bf16")
    return out


# Parameters and BatchNorm buffers are also written THROUGH RAW POINTERS by this library (the fused Adam launch, the statistics kernels, the
# one-call training steps): torch's version counters do not see those writes.  Every such call site bumps PARAM_EPOCH, and whatever is
# derived from parameters and remembered across calls (packed weights, folded eval-mode BatchNorm tails) is keyed by (identity, torch
# version, PARAM_EPOCH).
PARAM_EPOCH = 0


def note_param_write():
    global PARAM_EPOCH
    PARAM_EPOCH += 1


_PACKED = []          # [(weakref(w), key, packed)], most recent first


def pack_weight(w):
    """glnn_pack_weight_f32: W [d_out, d_in] -> MFMA B-fragment order for sage_fused.  The packed copy of a weight is remembered while
    the same unmodified tensor comes back (an eval-mode teacher forward packs the same three weights on every call: three launches of
    the ~0.9 ms arxiv forward); READ-ONLY for the caller."""
    _need_cuda(w)
    key = (w.data_ptr(), tuple(w.shape), w.stride(0), w._version, PARAM_EPOCH)
    for i, (ref, k, wp) in enumerate(_PACKED):
        if ref() is w and k == key:
            if i:
                _PACKED.insert(0, _PACKED.pop(i))
            return wp
    wp = _pack_weight(w)
    import weakref
    _PACKED[:] = [e for e in _PACKED if e[0]() is not None and e[0]() is not w][:15]
    _PACKED.insert(0, (weakref.ref(w), key, wp))
    return wp


def _pack_weight(w):
    _mat(w, "pack_weight w")
    d_out, d_in = w.shape
    wp = torch.empty(_lib.lib().glnn_packed_weight_floats(d_out, d_in), dtype=torch.float32, device=w.device)
    rc = _lib.lib().glnn_pack_weight_f32(_p(w), _ld(w), d_out, d_in, _p(wp), _stream())
    _lib.check(rc, "glnn_pack_weight_f32")
    return wp


def fused_tile_order(indptr, n_dst):
    """The 32-row tiles of a fused launch over rows [0, n_dst) of `indptr`, heaviest row first (stable): int32 permutation for
    sage_fused(tile_order=...).  One-time index arithmetic per graph / row range (cache it)."""
    deg = (indptr[1:n_dst + 1] - indptr[:n_dst])
    tiles = (n_dst + 31) // 32
    pad = tiles * 32 - n_dst
    if pad:
        deg = torch.cat([deg, deg.new_zeros(pad)])
    return torch.argsort(deg.view(tiles, 32).amax(1), descending=True, stable=True).to(torch.int32)


class ChunkSignals:
    """Completion signals of ONE fused launch over the chunks of a row range (glnn_sage_fused_chunks_f32, round 6): per chunk a signal
    word a stream can wait on and an arrival counter.  `row_start`: first row of every chunk inside the launch's row range + the end
    (multiples of 32).  Per launch: sage_fused(..., chunks=sig.launch(self_rows, out_rows)) stamps a new epoch; then
    sig.wait(stream, c) holds `stream`'s next operation until chunk c's rows are stored and written back -- while the launch still runs.
    Chunks without rows are never signalled (`sig.empty(c)`: do not wait for them)."""
    MAX = _lib.MAX_CHUNKS

    def __init__(self, row_start, device):
        n = len(row_start) - 1
        if not 1 <= n <= self.MAX or row_start[0] != 0 or any(r % 32 for r in row_start[:-1]) or any(a > b for a, b in zip(row_start[:-1], row_start[1:])):
            raise ValueError(f"ChunkSignals: 1..{self.MAX} chunks whose first rows are ascending multiples of 32, starting at 0")
        self.row_start, self.n, self.device, self.epoch = [int(r) for r in row_start], n, device, 0
        self.arrivals = torch.zeros(n, dtype=torch.int32, device=device)
        self._signals = []
        for _ in range(n):
            p = ctypes.c_void_p()
            _lib.check(_lib.lib().glnn_signal_alloc(ctypes.byref(p)), "glnn_signal_alloc")
            self._signals.append(p.value)
        self._n_dst = None

    def empty(self, c, n_dst=None):
        n_dst = self._n_dst if n_dst is None else n_dst
        return min(self.row_start[c + 1], n_dst) <= self.row_start[c]

    def launch(self, self_rows, out_rows, n_dst):
        """The descriptor of the next launch (a new epoch): self_rows[c] / out_rows[c] = the rows of x_self / of the outputs that hold the
        chunk's first row."""
        if len(self_rows) != self.n or len(out_rows) != self.n or self.row_start[-1] < n_dst:
            raise ValueError("ChunkSignals.launch: one self row and one output row per chunk, chunks covering the launch's rows")
        self.epoch += 1
        self._n_dst = int(n_dst)
        d = _lib.ChunkSignalsDesc()
        d.n_chunks = self.n
        for c in range(self.n + 1):
            d.row_start[c] = self.row_start[c]
        for c in range(self.n):
            d.self_row[c], d.out_row[c], d.signal[c] = int(self_rows[c]), int(out_rows[c]), self._signals[c]
        d.arrivals = self.arrivals.data_ptr()
        d.epoch = self.epoch
        return d

    def wait(self, stream, c):
        """`stream` (torch.cuda.Stream) runs nothing further until chunk c of the LAST launch is complete."""
        _lib.check(_lib.lib().glnn_stream_wait_value32(ctypes.c_void_p(stream.cuda_stream), ctypes.c_void_p(self._signals[c]), self.epoch),
                   "glnn_stream_wait_value32")

    def value(self, c):
        v = ctypes.c_uint32()
        _lib.check(_lib.lib().glnn_signal_read(ctypes.c_void_p(self._signals[c]), ctypes.byref(v)), "glnn_signal_read")
        return v.value

    def __del__(self):
        try:
            for p in self._signals:
                _lib.lib().glnn_signal_free(ctypes.c_void_p(p))
        except Exception:
            pass


def sage_fused(indptr, indices, x, n_dst, w, ep_scale=None, ep_shift=None, relu=False, out=None, x_self=None, w_packed=None,
               w_next=None, out_next=None, want_out=True, tile_order=None, hub=None, chunks=None, out_dtype=None, out_next_dtype=None,
               agg_out=None, agg_in=None):
    """K1F glnn_sage_fused_f32: epi(((A x + x_self)/(deg+1)) @ w.T) in one launch (d_in, d_out <= 256).
    w_next [d_out2, d_out]: also returns (.. , out @ w_next.T) -- the projection of the NEXT layer when it projects first;
    with want_out=False the hidden rows themselves are not written at all (returns (None, projected)).
    chunks (ChunkSignals.launch(...)): the launch covers the chunks of a row range -- x_self / out / out_next are then WHOLE buffers
    addressed through the descriptor's per-chunk rows (they must be given), and every chunk signals its completion.
    bf16 x (and x_self): glnn_sage_fused_bf16, the same fp32 MFMA on the fp32 aggregate; out / out_next are stored in their own dtype, else
    in out_dtype / out_next_dtype (default bf16); no hub / chunks.
    agg_out / agg_in (glnn_sage_fused_agg_f32; fp32, no chunks; a feat_empty(n_dst, d_in) matrix): the aggregate
    (A x + x_self)/(deg+1) depends on the graph and on x only.  agg_out: this launch also stores it there (same out / out_next bits).
    agg_in: the launch reads it back instead of gathering -- indptr, indices, x, x_self, tile_order and hub are not used -- and stores the
    bits the agg_out launch with these weights stores; set_timing records it as a "gemm" (m rows, k = d_in, n = d_out), which is what it
    is."""
    _need_cuda(indptr, indices, x, w, ep_scale, ep_shift, out, x_self, w_next, out_next, agg_out, agg_in)
    agg = agg_out if agg_out is not None else agg_in
    if agg is not None:
        if agg_out is not None and agg_in is not None:
            raise ValueError("sage_fused: agg_out and agg_in exclude each other")
        if chunks is not None or (x is not None and x.dtype != torch.float32):
            raise ValueError("sage_fused: agg_out / agg_in belong to the fp32 launch without chunks")
        _mat(agg, "sage_fused agg")
        if agg.shape[0] < n_dst or agg.shape[1] != w.shape[1]:
            raise ValueError("sage_fused: the aggregate must hold n_dst rows of d_in columns")
    if agg_in is not None:
        return _sage_fused_agg_in(agg_in, n_dst, w, ep_scale, ep_shift, relu, out, w_packed, w_next, out_next, want_out)
    if x.dtype == torch.bfloat16:
        return _sage_fused_bf16(indptr, indices, x, n_dst, w, ep_scale, ep_shift, relu, out, x_self, w_packed, w_next, out_next, want_out,
                                tile_order, hub, chunks, out_dtype, out_next_dtype)
    if out_dtype not in (None, torch.float32) or out_next_dtype not in (None, torch.float32):
        raise ValueError("sage_fused: fp32 rows give fp32 outputs (bf16 outputs need bf16 rows: ops.to_bf16)")
    if chunks is not None and (x_self is None or (out is None and want_out) or (w_next is not None and out_next is None)):
        raise ValueError("sage_fused(chunks=...): x_self and the output buffers must be given (they are addressed by the chunks' rows)")
    x = as_feat(x)
    x_self = x if x_self is None else as_feat(x_self)
    n_src, d_in = x.shape
    d_out = w.shape[0]
    if w.shape[1] != d_in:
        raise ValueError("sage_fused: weight must be [d_out, d_in]")
    if tile_order is not None and (tile_order.dtype != torch.int32 or not tile_order.is_contiguous() or tile_order.numel() != (n_dst + 31) // 32):
        raise ValueError("sage_fused: tile_order must be a contiguous int32 permutation of the ceil(n_dst / 32) tile ids")
    if w_packed is None:
        w_packed = pack_weight(w)
    if out is None and (want_out or w_next is None):
        out = feat_empty(n_dst, d_out, x.device)
    w2p, d_out2 = None, 0
    if w_next is not None:
        if w_next.shape[1] != d_out:
            raise ValueError("sage_fused: w_next must be [d_out2, d_out]")
        w2p, d_out2 = pack_weight(w_next), w_next.shape[0]
        if out_next is None:
            out_next = feat_empty(n_dst, d_out2, x.device)
    with _Timed("sage_fused", d=d_in, n_dst=n_dst, d_out=d_out, d_chain=d_out2, d_written=(d_out if out is not None else 0) + d_out2):
        args = (_p(indptr), _p(indices), n_dst, n_src, _p(x), _ld(x), d_in, _p(x_self), _ld(x_self),
                _p(w_packed), d_out, _p(_vec(ep_scale, d_out, "ep_scale")),
                _p(_vec(ep_shift, d_out, "ep_shift")), 1 if relu else 0, _p(out), _ld(out) if out is not None else 0,
                _p(w2p), d_out2, _p(out_next), _ld(out_next) if out_next is not None else 0, _p(tile_order))
        plan = hub.desc_for(d_in, x.device) if hub is not None else None
        if chunks is not None:
            rc = _lib.lib().glnn_sage_fused_chunks_f32(*args, plan, ctypes.byref(chunks), _stream())
        elif agg_out is not None:
            rc = _lib.lib().glnn_sage_fused_agg_f32(*args, plan, _p(agg_out), None, _ld(agg_out), _stream())
        elif plan is not None:
            rc = _lib.lib().glnn_sage_fused_plan_f32(*args, plan, _stream())
        else:
            rc = _lib.lib().glnn_sage_fused_f32(*args, _stream())
    _lib.check(rc, "glnn_sage_fused_f32")
    return out if w_next is None else (out, out_next)


def _sage_fused_agg_in(agg, n_dst, w, ep_scale, ep_shift, relu, out, w_packed, w_next, out_next, want_out):
    d_out, d_in = w.shape
    if w_packed is None:
        w_packed = pack_weight(w)
    if out is None and (want_out or w_next is None):
        out = feat_empty(n_dst, d_out, agg.device)
    w2p, d_out2 = None, 0
    if w_next is not None:
        if w_next.shape[1] != d_out:
            raise ValueError("sage_fused: w_next must be [d_out2, d_out]")
        w2p, d_out2 = pack_weight(w_next), w_next.shape[0]
        if out_next is None:
            out_next = feat_empty(n_dst, d_out2, agg.device)
    with _Timed("gemm", m=n_dst, k=d_in, n=d_out):
        rc = _lib.lib().glnn_sage_fused_agg_f32(
            None, None, n_dst, 0, None, 0, d_in, None, 0, _p(w_packed), d_out, _p(_vec(ep_scale, d_out, "ep_scale")),
            _p(_vec(ep_shift, d_out, "ep_shift")), 1 if relu else 0, _p(out), _ld(out) if out is not None else 0,
            _p(w2p), d_out2, _p(out_next), _ld(out_next) if out_next is not None else 0, None, None, None, _p(agg), _ld(agg), _stream())
    _lib.check(rc, "glnn_sage_fused_agg_f32")
    return out if w_next is None else (out, out_next)


def _sage_fused_bf16(indptr, indices, x, n_dst, w, ep_scale, ep_shift, relu, out, x_self, w_packed, w_next, out_next, want_out, tile_order,
                     hub, chunks, out_dtype, out_next_dtype):
    if hub is not None or chunks is not None:
        raise ValueError("sage_fused: bf16 rows take neither a hub plan nor chunks")
    x = as_bf16_feat(x)
    if x_self is not None and (x_self.dtype != torch.bfloat16 or x_self.shape[0] < n_dst or x_self.shape[1] != x.shape[1]):
        raise ValueError("sage_fused: x_self must be bf16 like x and hold n_dst rows of the same width")
    x_self = x if x_self is None else as_bf16_feat(x_self)
    n_src, d_in = x.shape
    d_out = w.shape[0]
    if w.shape[1] != d_in:
        raise ValueError("sage_fused: weight must be [d_out, d_in]")
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise ValueError("sage_fused: indptr must be int64 and indices int32")
    if tile_order is not None and (tile_order.dtype != torch.int32 or not tile_order.is_contiguous() or tile_order.numel() != (n_dst + 31) // 32):
        raise ValueError("sage_fused: tile_order must be a contiguous int32 permutation of the ceil(n_dst / 32) tile ids")
    if w_packed is None:
        w_packed = pack_weight(w)
    if out is not None or want_out or w_next is None:
        out = _out_like(out, out_dtype, torch.bfloat16, n_dst, d_out, x.device, "sage_fused out")
    w2p, d_out2 = None, 0
    if w_next is not None:
        if w_next.shape[1] != d_out:
            raise ValueError("sage_fused: w_next must be [d_out2, d_out]")
        w2p, d_out2 = pack_weight(w_next), w_next.shape[0]
        out_next = _out_like(out_next, out_next_dtype, torch.bfloat16, n_dst, d_out2, x.device, "sage_fused out_next")
    with _Timed("sage_fused_bf16", d=d_in, n_dst=n_dst, d_out=d_out, d_chain=d_out2, d_written=(d_out if out is not None else 0) + d_out2):
        rc = _lib.lib().glnn_sage_fused_bf16(
            _p(indptr), _p(indices), n_dst, n_src, _p(x), _ld(x), d_in, _p(x_self), _ld(x_self),
            _p(w_packed), d_out, _p(_vec(ep_scale, d_out, "ep_scale")), _p(_vec(ep_shift, d_out, "ep_shift")), 1 if relu else 0,
            _p(out), _ld(out) if out is not None else 0, _dtype_code(out) if out is not None else DTYPE_F32,
            _p(w2p), d_out2, _p(out_next), _ld(out_next) if out_next is not None else 0,
            _dtype_code(out_next) if out_next is not None else DTYPE_F32, _p(tile_order), _stream())
    _lib.check(rc, "glnn_sage_fused_bf16")
    return out if w_next is None else (out, out_next)


# ---- the GraphSAGE "mean" aggregator (csrc/sage_mean.hip, docs/SAGE_MEAN_SEMANTICS.md) -------------------------------------------
_PAIRS = []           # [(kind, weakref(w_neigh), weakref(w_self), key, derived)], most recent first


def _pair_cached(kind, w_neigh, w_self, build):
    """`build()` of a (fc_neigh.weight, fc_self.weight) pair, remembered like pack_weight remembers a packed weight: while the same two
    unmodified tensors come back (identity, torch version, data pointer, PARAM_EPOCH) -- a parameter write re-derives."""
    key = tuple((w.data_ptr(), tuple(w.shape), w.stride(0), w._version) for w in (w_neigh, w_self)) + (PARAM_EPOCH,)
    for i, (kd, rn, rs, k, val) in enumerate(_PAIRS):
        if kd == kind and rn() is w_neigh and rs() is w_self and k == key:
            if i:
                _PAIRS.insert(0, _PAIRS.pop(i))
            return val
    val = build()
    import weakref
    _PAIRS[:] = [e for e in _PAIRS if e[1]() is not None and e[2]() is not None
                 and not (e[0] == kind and e[1]() is w_neigh and e[2]() is w_self)][:15]
    _PAIRS.insert(0, (kind, weakref.ref(w_neigh), weakref.ref(w_self), key, val))
    return val


def _check_pair(w_neigh, w_self, who):
    _need_cuda(w_neigh, w_self)
    _mat(w_neigh, who + " w_neigh")
    _mat(w_self, who + " w_self")
    if w_neigh.shape != w_self.shape:
        raise ValueError(f"{who}: fc_neigh.weight and fc_self.weight must have the same [d_out, d_in] shape")


def pack_weight_pair(w_neigh, w_self):
    """The packed W_cat of sage_mean_fused: glnn_pack_weight_f32 of the [d_out, 2 kpad] matrix [W_neigh | 0 | W_self | 0], kpad = d_in
    rounded up to 8, so that the fused launch is ONE MFMA product over [mean | self] tiles.  Keyed like pack_weight (parameter writes
    re-pack); READ-ONLY for the caller."""
    _check_pair(w_neigh, w_self, "pack_weight_pair")

    def build():
        d_out, d_in = w_neigh.shape
        kpad = round8(d_in)
        cat = torch.zeros(d_out, 2 * kpad, dtype=torch.float32, device=w_neigh.device)
        cat[:, :d_in] = w_neigh.detach()
        cat[:, kpad:kpad + d_in] = w_self.detach()
        return _pack_weight(cat)
    return _pair_cached("cat", w_neigh, w_self, build)


def stack_weight_pair(w_neigh, w_self):
    """[W_neigh; 0; W_self] as ONE [round4(d_out) + d_out, d_in] matrix for the project-first form: gemm(x, stacked) gives the two halves
    spmm_sage_mean reads, the second one starting at the float4-aligned column round4(d_out).  Keyed like pack_weight_pair."""
    _check_pair(w_neigh, w_self, "stack_weight_pair")

    def build():
        d_out, d_in = w_neigh.shape
        r4 = round4(d_out)
        st = torch.zeros(r4 + d_out, d_in, dtype=torch.float32, device=w_neigh.device)
        st[:d_out] = w_neigh.detach()
        st[r4:] = w_self.detach()
        return st
    return _pair_cached("stack", w_neigh, w_self, build)


def sage_mean_fused(indptr, indices, x, n_dst, w_neigh, w_self, ep_scale=None, ep_shift=None, relu=False, out=None, x_self=None,
                    self_rows=None, w_packed=None, tile_order=None):
    """glnn_sage_mean_fused_f32: epi(fc_neigh(mean of the in-neighbours' rows) + fc_self(own row)) in one launch, d_in <= d_out <= 256.
    x [n_src, d_in]; x_self: the destination rows' own features, default x[:n_dst]; self_rows (int64 [n_dst]): destination v's own row is
    x_self[self_rows[v]].  w_packed: pack_weight_pair(w_neigh, w_self) of a caller that sweeps many blocks.  Returns [n_dst, d_out]."""
    _need_cuda(indptr, indices, x, ep_scale, ep_shift, out, x_self, self_rows, w_packed, tile_order)
    _check_pair(w_neigh, w_self, "sage_mean_fused")
    x = as_feat(x)
    x_self = x if x_self is None else as_feat(x_self)
    n_src, d_in = x.shape
    d_out = w_neigh.shape[0]
    if w_neigh.shape[1] != d_in or x_self.shape[1] != d_in:
        raise ValueError("sage_mean_fused: weights must be [d_out, d_in] and x_self as wide as x")
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or indptr.numel() < n_dst + 1:
        raise ValueError("sage_mean_fused: indptr must be int64 with n_dst + 1 entries and indices int32")
    if self_rows is not None:
        if self_rows.dtype != torch.int64 or not self_rows.is_contiguous() or self_rows.numel() < n_dst:
            raise ValueError("sage_mean_fused: self_rows must be a contiguous int64 vector of n_dst row ids")
    elif x_self.shape[0] < n_dst:
        raise ValueError("sage_mean_fused: x_self must hold n_dst rows")
    if tile_order is not None and (tile_order.dtype != torch.int32 or not tile_order.is_contiguous() or tile_order.numel() != (n_dst + 31) // 32):
        raise ValueError("sage_mean_fused: tile_order must be a contiguous int32 permutation of the ceil(n_dst / 32) tile ids")
    if w_packed is None:
        w_packed = pack_weight_pair(w_neigh, w_self)
    if out is None:
        out = feat_empty(n_dst, d_out, x.device)
    _mat(out, "sage_mean_fused out")
    if out.shape[0] < n_dst or out.shape[1] != d_out:
        raise ValueError("sage_mean_fused: out must hold n_dst rows of d_out columns")
    with _Timed("sage_mean_fused", d=d_in, n_dst=n_dst, d_out=d_out):
        rc = _lib.lib().glnn_sage_mean_fused_f32(
            _p(indptr), _p(indices), n_dst, n_src, _p(x), _ld(x), d_in, _p(x_self), _ld(x_self), _p(self_rows), _p(w_packed), d_out,
            _p(_vec(ep_scale, d_out, "ep_scale")), _p(_vec(ep_shift, d_out, "ep_shift")), 1 if relu else 0, _p(out), _ld(out),
            _p(tile_order), _stream())
    _lib.check(rc, "glnn_sage_mean_fused_f32")
    return out


def spmm_sage_mean(indptr, indices, x, s, n_dst, ep_scale=None, ep_shift=None, relu=False, out=None):
    """glnn_spmm_sage_mean_f32: out[v] = epi(mean_{u->v} x[u] + s[v]), d <= 256.  x [n_src, d] and s [>= n_dst, d]: the two halves of
    gemm(h, stack_weight_pair(w_neigh, w_self)) (column views keep their leading dimension).  Returns [n_dst, d]."""
    _need_cuda(indptr, indices, x, s, ep_scale, ep_shift, out)
    x, s = as_feat(x), as_feat(s)
    n_src, d = x.shape
    if s.shape[1] != d or s.shape[0] < n_dst:
        raise ValueError("spmm_sage_mean: s must hold n_dst rows as wide as x")
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or indptr.numel() < n_dst + 1:
        raise ValueError("spmm_sage_mean: indptr must be int64 with n_dst + 1 entries and indices int32")
    if out is None:
        out = feat_empty(n_dst, d, x.device)
    _mat(out, "spmm_sage_mean out")
    if out.shape[0] < n_dst or out.shape[1] != d:
        raise ValueError("spmm_sage_mean: out must hold n_dst rows of d columns")
    with _Timed("spmm_sage_mean", d=d, n_dst=n_dst):
        rc = _lib.lib().glnn_spmm_sage_mean_f32(
            _p(indptr), _p(indices), n_dst, n_src, _p(x), _ld(x), d, _p(s), _ld(s), _p(_vec(ep_scale, d, "ep_scale")),
            _p(_vec(ep_shift, d, "ep_shift")), 1 if relu else 0, _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_spmm_sage_mean_f32")
    return out


class RowRangeLaunch:
    """A PREPARED SAGE-"gcn" launch over row ranges [s, e) of one resident CSR whose column ids are rows of `x` (the engine-mode chunked
    sweep of SAGE.inference, reference models.py:133-145): everything that does not change from chunk to chunk -- the checks of sage_fused /
    spmm, the packed weight, the C argument list -- is done ONCE here; a call only offsets three pointers (indptr + s, the self rows
    x[s:], the output rows out[s:]) and launches.  Same library entries, same arguments, same bits as the per-chunk ops calls (~8 us of
    host time per chunk instead of ~25).  w = None: the stand-alone aggregation (a layer that projected first), else the fused kernel."""

    def __init__(self, indptr, indices, x, out, w=None, ep_scale=None, ep_shift=None, relu=False, w_packed=None):
        _need_cuda(indptr, indices, x, out, w, ep_scale, ep_shift)
        x = as_feat(x)
        _mat(out, "RowRangeLaunch out")
        if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or out.shape[0] < indptr.numel() - 1:
            raise ValueError("RowRangeLaunch: indptr int64, indices int32, one output row per CSR row")
        n_src, d_in = x.shape
        self.keep = (indptr, indices, x, out, w, ep_scale, ep_shift)          # (the pointers below stay valid while this object lives)
        self.n = indptr.numel() - 1
        self.ip0, self.x0, self.ldx, self.o0, self.ldo = indptr.data_ptr(), x.data_ptr(), _ld(x), out.data_ptr(), _ld(out)
        if w is None:
            d = d_in
            if out.shape[1] != d:
                raise ValueError("RowRangeLaunch: out must be as wide as x")
            self.fused, self.info = False, dict(d=d, mode=AGG_SAGE_GCN)
            self.tail = (_p(_vec(ep_scale, d, "ep_scale")), _p(_vec(ep_shift, d, "ep_shift")), 1 if relu else 0)
            self.head = (_p(indices),)
            self.mid = (n_src, self.x0, self.ldx, d, AGG_SAGE_GCN, None, None)
        else:
            d_out = w.shape[0]
            if w.shape[1] != d_in or d_in > 256 or d_out > 256 or out.shape[1] != d_out:
                raise ValueError("RowRangeLaunch: weight [d_out, d_in] with d_in, d_out <= 256, out [n, d_out]")
            wp = pack_weight(w) if w_packed is None else w_packed
            self.keep += (wp,)
            self.fused, self.info = True, dict(d=d_in, d_out=d_out, d_chain=0, d_written=d_out)
            self.head = (_p(indices),)
            self.mid = (n_src, self.x0, self.ldx, d_in)
            self.tail = (_p(wp), d_out, _p(_vec(ep_scale, d_out, "ep_scale")), _p(_vec(ep_shift, d_out, "ep_shift")), 1 if relu else 0)
        self.fn = _lib.lib().glnn_sage_fused_f32 if self.fused else _lib.lib().glnn_spmm_csr_f32

    def __call__(self, s, e):
        if not 0 <= s <= e <= self.n:
            raise ValueError("RowRangeLaunch: row range outside the CSR")
        n_dst = e - s
        ip, xs, o = self.ip0 + 8 * s, self.x0 + 4 * self.ldx * s, self.o0 + 4 * self.ldo * s
        if self.fused:
            args = (ip,) + self.head + (n_dst,) + self.mid + (xs, self.ldx) + self.tail + (o, self.ldo, None, 0, None, 0, None, _stream())
        else:
            args = (ip,) + self.head + (n_dst,) + self.mid + (xs, self.ldx, None) + self.tail + (o, self.ldo, _stream())
        if _TIMING is not None:
            with _Timed("sage_fused" if self.fused else "spmm", n_dst=n_dst, **self.info):
                rc = self.fn(*args)
        else:
            rc = self.fn(*args)
        if rc != 0:
            _lib.check(rc, "glnn_sage_fused_f32" if self.fused else "glnn_spmm_csr_f32")


# ---- placement of gathered matrices (round 5) ------------------------------------------------------------------------------------
# The same aggregation launch over the same graph runs 18.1 ... 19.4 ms (fused D=256, products shape) depending on WHICH allocation
# holds the matrix it gathers from -- stable per buffer, different from one buffer to the next inside one process, unaffected by the
# offset inside an allocation (profiles/r05_bimodal_launch.txt, scripts/bimodal_probe.py): where the driver put the buffer's pages in
# HBM.  A matrix that many launches will gather from is therefore PLACED: a few candidate allocations are timed with a gather over the
# very graph and the fastest one is kept.  One-time set-up work per (graph, matrix), like the tile order or a hub plan; results are
# untouched (it only chooses which memory holds the rows).  Only for matrices far beyond the caches (>= PLACEMENT_MIN_BYTES) that still
# fit many times (<= PLACEMENT_MAX_BYTES).
import os as _os
PLACEMENT_CANDIDATES = int(_os.environ.get("GLNN_PLACEMENT_CANDIDATES", "12"))     # <= 1: off (the first allocation is used)
# Candidates are made in groups of four with a BALLAST allocation between the groups (alive until the choice is made), so that the groups
# come from different regions of HBM: in some processes every allocation of the first region is slow (scripts/placement_ballast_probe.py:
# with three or four regions a 17.9-18.0 ms candidate was found in every one of five processes, the first region alone gave 17.96-18.45).
# Ballast = this fraction of the free device memory, at most PLACEMENT_BALLAST_MAX bytes per gap; 0 = none.
PLACEMENT_BALLAST_FRAC = float(_os.environ.get("GLNN_PLACEMENT_BALLAST_FRAC", "0.15"))
PLACEMENT_BALLAST_MAX = 48 << 30
PLACEMENT_MIN_BYTES = 1 << 30        # (matrices of 0.5-1 GB -- the products features, the 47-wide projection -- showed 1 % spreads: not worth a search)
PLACEMENT_MAX_BYTES = 8 << 30
PLACEMENT_LOG = []             # one record per tuned matrix: {"what", "rows", "d", "ms": [...], "chosen"} (bench.py prints it)


def placement_applies(rows, d):
    nbytes = 4 * rows * round4(d)
    return PLACEMENT_CANDIDATES > 1 and PLACEMENT_MIN_BYTES <= nbytes <= PLACEMENT_MAX_BYTES


def placed_for_gather(rows, d, device, indptr, indices, n_dst, what="", first=None, zero=False, probe=None):
    """An [rows, d] feature buffer for a matrix that launches over (indptr, indices) will gather from, in the allocation where that
    gather runs fastest among PLACEMENT_CANDIDATES tries (all alive at once, so that they are different memory; the losers are freed).
    `first` (optional, [rows, d]): an existing buffer that competes as candidate 0 (returned itself if it wins).  probe(candidate): the
    launch to time -- the caller's own consumer of the matrix where it has one (SAGE.inference times the next layer's launch); default: the
    stand-alone SAGE-gcn aggregation of the candidate.  (A candidate's CONTENT is irrelevant to the timing: zeros when `zero`, else
    whatever the allocator left.)"""
    if not placement_applies(rows, d):
        return first if first is not None else feat_empty(rows, d, device, zero=zero)
    # (What makes an allocation slow is its physical backing: the same virtual addresses gather in 18.0 ms when the request was served from
    #  an unfragmented free pool and in 19.0-19.5 ms when small allocations were made in between, or out of a re-used cached block with
    #  that history: scripts/placement_cause_probe.py, profiles/r05_placement_cause.txt.  Not predictable from here -- hence the probe.)
    # The search is an optimisation and must never be what runs a device out of memory: the candidates + the ballast together
    # stay below the free memory minus a headroom of two more matrices (the probe's own scratch / the next layer's output are allocated
    # while the candidates are alive), the probe loop is under the same handler as the allocations, and every failure falls back to the
    # plain allocation the caller would have made without the search.
    nbytes_m = 4 * rows * round4(d)
    cands, ballast = ([first] if first is not None else []), []
    scratch = None

    def fallback():
        del cands[:], ballast[:]
        torch.cuda.empty_cache()
        return first if first is not None else feat_empty(rows, d, device, zero=zero)

    try:
        budget = torch.cuda.mem_get_info(device)[0] - 2 * nbytes_m
        want = PLACEMENT_CANDIDATES
        while len(cands) < want:
            if budget < nbytes_m:
                break                                     # (a nearly full or shared device: choose among what fits)
            if len(cands) and len(cands) % 4 == 0 and PLACEMENT_BALLAST_FRAC > 0:
                free = torch.cuda.mem_get_info(device)[0]
                nb = int(min(PLACEMENT_BALLAST_FRAC * free, PLACEMENT_BALLAST_MAX))
                # (never squeeze the candidates themselves, nor the headroom)
                if nb >= (1 << 30) and free - nb > 8 * nbytes_m and budget - nb >= (want - len(cands)) * nbytes_m:
                    ballast.append(torch.empty(nb, dtype=torch.uint8, device=device))
                    budget -= nb
            cands.append(feat_empty(rows, d, device, zero=zero))
            budget -= nbytes_m
    except torch.cuda.OutOfMemoryError:
        # a device shared with other tenants (or nearly full): choose among the candidates that did fit
        del ballast[:]
        torch.cuda.empty_cache()
    try:
        if len(cands) <= 1:
            return fallback() if not cands else cands[0]
        if probe is None:
            scratch = feat_empty(n_dst, d, device)

            def probe(c):
                _lib.check(_spmm_call(indptr, indices, n_dst, rows, c, d, AGG_SAGE_GCN, None, None, None, None, False, scratch,
                                      c[:n_dst] if rows >= n_dst else c, None), "glnn_spmm_csr_f32 (placement probe)")
        ms = []
        for c in cands:
            probe(c)
            best = None
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                probe(c)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1)
                best = t if best is None else min(best, t)
            ms.append(best)
    except torch.cuda.OutOfMemoryError:
        scratch = None
        return fallback()
    k = min(range(len(cands)), key=lambda i: ms[i])
    PLACEMENT_LOG.append({"what": what, "rows": int(rows), "d": int(d), "ms": [round(v, 3) for v in ms], "chosen": k})
    keep = cands[k]
    del cands, scratch, ballast
    torch.cuda.empty_cache()          # the losers and the ballast go back to the driver, not into the caching allocator's pool
    return keep


def place_for_gather(x, indptr, indices, n_dst, what="features"):
    """x itself, or a copy of it in a better-placed allocation (see placed_for_gather): for the static input matrix of a teacher forward."""
    x = as_feat(x)
    if not placement_applies(x.shape[0], x.shape[1]) or x.shape[0] < n_dst:
        return x
    best = placed_for_gather(x.shape[0], x.shape[1], x.device, indptr, indices, n_dst, what=what, first=x)
    if best is not x:
        _storage_copy(best, x)
    return best


def _storage_copy(dst, src):
    """dst[:, :] = src including the padding columns of the feature layout (both [rows, d] views of [rows, round4(d)] storage)."""
    d = src.shape[1]
    dst.copy_(src)
    if dst.stride(0) > d:                      # padding columns are zero by the layout's contract
        torch.as_strided(dst, (dst.shape[0], dst.stride(0) - d), (dst.stride(0), 1), dst.storage_offset() + d).zero_()


DEG_RAW, DEG_RSQRT_CLAMP1, DEG_INV_PLUS1 = 0, 1, 2
SELF_ROWS = True      # spmm(..., self_rows=) is available (dist.ShardedTeacher asks: the numpy test backend has no such argument)


def degrees(indptr, indices, n_dst, n_src, nnz, want_out=True, transform=DEG_RAW, want_in=True):
    """glnn_degrees_f32: (t(in_deg) [n_dst], t(out_deg) [n_src]) as fp32; transform: DEG_RAW | DEG_RSQRT_CLAMP1 | DEG_INV_PLUS1."""
    _need_cuda(indptr, indices)
    in_deg = torch.empty(n_dst, dtype=torch.float32, device=indptr.device) if want_in else None
    out_deg = torch.empty(n_src, dtype=torch.float32, device=indptr.device) if want_out else None
    rc = _lib.lib().glnn_degrees_f32(_p(indptr), _p(indices), n_dst, n_src, nnz, transform, _p(in_deg), _p(out_deg), _stream())
    _lib.check(rc, "glnn_degrees_f32")
    return in_deg, out_deg


_DEFAULT_WS = {}


def _default_ws(device):
    """One lazily allocated 64 MB split-K workspace per (device, stream) for callers that pass none: the partials of two GEMMs issued
    on different streams of one device must not share a buffer (reuse on ONE stream is ordered)."""
    key = (str(device), int(_stream().value or 0))
    if key not in _DEFAULT_WS:
        if len(_DEFAULT_WS) >= 8:
            _DEFAULT_WS.clear()                        # a pathological number of streams: start over rather than grow without bound
        _DEFAULT_WS[key] = torch.empty(1 << 24, dtype=torch.float32, device=device)
    return _DEFAULT_WS[key]


def gemm(a, w, w_is_kn=False, a_rows=None, a_scale=None, a_shift=None, row_scale=None, ep_scale=None,
         ep_shift=None, relu=False, out=None, m=None, drop_p=0.0, drop_seed=0, workspace=None):
    """K3 glnn_gemm_f32: out = epi(A' @ W^T) (w [n,k], torch Linear layout) or epi(A' @ W) (w [k,n])."""
    _need_cuda(a, w, a_rows, a_scale, a_shift, row_scale, ep_scale, ep_shift, out)
    _mat(a, "gemm a")
    _mat(w, "gemm w")
    k = a.shape[1]
    n = w.shape[1] if w_is_kn else w.shape[0]
    if (w.shape[0] if w_is_kn else w.shape[1]) != k:
        raise ValueError(f"gemm: inner dimensions differ: a {tuple(a.shape)} w {tuple(w.shape)} kn={w_is_kn}")
    if m is None:
        m = a_rows.numel() if a_rows is not None else a.shape[0]
    if a_rows is not None and (a_rows.dtype != torch.int64 or not a_rows.is_contiguous()):
        raise ValueError("gemm: a_rows must be contiguous int64")
    if out is None:
        out = feat_empty(m, n, a.device)
    _mat(out, "gemm out")
    if w.stride(0) % 4 and w.numel() <= (1 << 22) and (w_is_kn or k < 4 or n > 512 or m >= 1024):
        w = as_feat(w)                              # weights whose rows are not float4-addressable and that the unaligned-W latency kernel does not
                                                    # take, or takes badly ([k, n] with n % 4 != 0, [n, k] with k < 4, or thousands of rows of A):
                                                    # a padded copy per call (nn.Parameters are never cached by as_feat), then the tiled kernels
    if workspace is None and m * n <= (1 << 22) and k >= 2048:
        workspace = _default_ws(a.device)          # lets a deep, narrow product split its reduction (see gemm.hip)
    with _Timed("gemm", m=m, k=k, n=n):
        rc = _gemm_call(a, a_rows, a_scale, a_shift, drop_p, drop_seed, m, k, w, w_is_kn, n, row_scale, ep_scale, ep_shift, relu, out,
                        workspace)
    _lib.check(rc, "glnn_gemm_f32")
    return out


def _gemm_call(a, a_rows, a_scale, a_shift, drop_p, drop_seed, m, k, w, w_is_kn, n, row_scale, ep_scale, ep_shift, relu, out,
               workspace):
    return _lib.lib().glnn_gemm_f32(
        _p(a), _ld(a), _p(a_rows), _p(_vec(a_scale, k, "a_scale")), _p(_vec(a_shift, k, "a_shift")),
        float(drop_p), int(drop_seed) & 0xFFFFFFFF, m, k,
        _p(w), _ld(w), 1 if w_is_kn else 0, n, _p(_vec(row_scale, m, "row_scale")),
        _p(_vec(ep_scale, n, "ep_scale")), _p(_vec(ep_shift, n, "ep_shift")), 1 if relu else 0,
        _p(out), _ld(out), _p(workspace), workspace.numel() if workspace is not None else 0, _stream())


def gemm_tn(a, b, b_rows=None, b_scale=None, b_shift=None, out=None, col_sum_a=None, workspace=None, m=None,
            drop_p=0.0, drop_seed=0):
    """glnn_gemm_tn_f32: out[i,j] = sum_m a[m,i] * b'[m,j]  (weight gradient dW = dZ^T @ A_prev)."""
    _need_cuda(a, b, b_rows, b_scale, b_shift, out, col_sum_a, workspace)
    _mat(a, "gemm_tn a")
    _mat(b, "gemm_tn b")
    if m is None:
        m = a.shape[0]
    ka, nb = a.shape[1], b.shape[1]
    if out is None:
        out = torch.empty((ka, nb), dtype=torch.float32, device=a.device)
    if workspace is None:
        workspace = torch.empty(64 * ka + 256 * 128 * 128, dtype=torch.float32, device=a.device)
    rc = _lib.lib().glnn_gemm_tn_f32(
        _p(a), _ld(a), m, ka, _p(b), _ld(b), _p(b_rows), _p(_vec(b_scale, nb, "b_scale")),
        _p(_vec(b_shift, nb, "b_shift")), float(drop_p), int(drop_seed) & 0xFFFFFFFF, nb, _p(out), _ld(out), _p(col_sum_a), _p(workspace), workspace.numel(), _stream())
    _lib.check(rc, "glnn_gemm_tn_f32")
    return out


def softmax_loss(logits, kind, lamb, labels=None, label_rows=None, target_logp=None, target_rows=None,
                 dlogits=None, logprob_out=None, loss_out=None, loss_accum=None, workspace=None):
    """K4 glnn_softmax_loss_f32.  Returns (loss_out [1] device tensor, dlogits)."""
    _need_cuda(logits, labels, label_rows, target_logp, target_rows, dlogits, logprob_out, loss_out, loss_accum)
    _mat(logits, "softmax_loss logits")
    rows, c = logits.shape
    if dlogits is None:
        dlogits = torch.empty((rows, c), dtype=torch.float32, device=logits.device)
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=logits.device)
    if workspace is None:
        workspace = torch.empty(1024, dtype=torch.float32, device=logits.device)
    if labels is not None and labels.dtype != torch.int64:
        raise ValueError("softmax_loss: labels must be int64")
    rc = _lib.lib().glnn_softmax_loss_f32(
        _p(logits), _ld(logits), rows, c, kind, _p(labels), _p(label_rows),
        _p(target_logp), _ld(target_logp) if target_logp is not None else 0, _p(target_rows), float(lamb),
        _p(dlogits), _ld(dlogits), _p(logprob_out), _ld(logprob_out) if logprob_out is not None else 0,
        _p(loss_out), _p(loss_accum), _p(workspace), workspace.numel(), _stream())
    _lib.check(rc, "glnn_softmax_loss_f32")
    return loss_out, dlogits


def classifier_loss(a, w, bias, kind, lamb=1.0, a_scale=None, a_shift=None, drop_p=0.0, drop_seed=0, labels=None, label_rows=None,
                    target_logp=None, target_rows=None, logits=None, dlogits=None, loss_out=None, loss_accum=None, workspace=None):
    """glnn_classifier_loss_f32: logits = tail(a) . w^T + bias and, with kind >= 0, log_softmax + NLL / KL + dlogits behind it in the same
    launch (large batches in front of a narrow classifier; raises GlnnError(UNSUPPORTED) for other shapes).  kind = -1: logits only.
    Returns (logits, loss_out, dlogits)."""
    _need_cuda(a, w, bias, a_scale, a_shift, labels, label_rows, target_logp, target_rows, logits, dlogits, loss_out, loss_accum)
    _mat(a, "classifier_loss a")
    rows, k = a.shape
    c = w.shape[0]
    dev = a.device
    if logits is None:
        logits = torch.empty((rows, c), dtype=torch.float32, device=dev)
    if kind >= 0:
        if dlogits is None:
            dlogits = torch.empty((rows, c), dtype=torch.float32, device=dev)
        if loss_out is None:
            loss_out = torch.empty(1, dtype=torch.float32, device=dev)
        if workspace is None:
            workspace = torch.empty(1024, dtype=torch.float32, device=dev)
    rc = _lib.lib().glnn_classifier_loss_f32(
        _p(a), _ld(a), _p(a_scale), _p(a_shift), float(drop_p), int(drop_seed) & 0xFFFFFFFF, rows, k, _p(w), _ld(w), c, _p(bias),
        _p(logits), _ld(logits), kind, _p(labels), _p(label_rows), _p(target_logp), _ld(target_logp) if target_logp is not None else 0,
        _p(target_rows), float(lamb), _p(dlogits), _ld(dlogits) if dlogits is not None else 0, _p(loss_out), _p(loss_accum),
        _p(workspace), workspace.numel() if workspace is not None else 0, _stream())
    _lib.check(rc, "glnn_classifier_loss_f32")
    return logits, loss_out, dlogits


def log_softmax(logits, out=None):
    _need_cuda(logits, out)
    _mat(logits, "log_softmax logits")
    rows, c = logits.shape
    if out is None:
        out = torch.empty((rows, c), dtype=torch.float32, device=logits.device)
    rc = _lib.lib().glnn_log_softmax_f32(_p(logits), _ld(logits), rows, c, _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_log_softmax_f32")
    return out


def bn_stats(z, gamma, beta, running_mean, running_var, nbt, eps=1e-5, momentum=0.1, outs=None, workspace=None):
    """K5 glnn_bn_stats_f32.  Returns (mean, rstd, a_scale, a_shift)."""
    note_param_write()
    _need_cuda(z, gamma, beta, running_mean, running_var, nbt, workspace)
    _mat(z, "bn_stats z")
    rows, h = z.shape
    if outs is None:
        outs = tuple(torch.empty(h, dtype=torch.float32, device=z.device) for _ in range(4))
    mean, rstd, a_scale, a_shift = outs
    nchunks = (rows + 127) // 128
    need = 2 * nchunks * h + (3 * ((nchunks + 63) // 64) * h if nchunks > 256 else 0)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=z.device)
    rc = _lib.lib().glnn_bn_stats_f32(_p(z), _ld(z), rows, h, _p(gamma), _p(beta), eps, momentum, _p(running_mean),
                                      _p(running_var), _p(nbt), _p(mean), _p(rstd), _p(a_scale), _p(a_shift),
                                      _p(workspace), workspace.numel(), _stream())
    _lib.check(rc, "glnn_bn_stats_f32")
    return mean, rstd, a_scale, a_shift


def linear_bn_stats(a, w, bias, gamma, beta, running_mean, running_var, nbt, eps=1e-5, momentum=0.1, out=None):
    """glnn_linear_bn_stats_f32: z = a w^T + bias and the BatchNorm1d training statistics of z, the statistics' first pass taken from
    the product kernel's epilogue where that kernel can leave it.  Returns (z, mean, rstd, a_scale, a_shift)."""
    note_param_write()
    _need_cuda(a, w, bias, gamma, beta, running_mean, running_var, nbt, out)
    a = as_feat(a)
    m, k = a.shape
    n = w.shape[0]
    if w.dim() != 2 or w.shape[1] < k or w.stride(1) != 1:
        raise ValueError("linear_bn_stats: w must be [n, k] row-major")
    z = feat_empty(m, n, a.device) if out is None else out
    mean, rstd, a_scale, a_shift = (torch.empty(n, dtype=torch.float32, device=a.device) for _ in range(4))
    nchunks = (m + 127) // 128
    ws_bn = torch.empty(max(2 * nchunks * n + (3 * ((nchunks + 63) // 64) * n if nchunks > 256 else 0), 3 * 128 * n), dtype=torch.float32, device=a.device)
    ws = _default_ws(a.device)
    rc = _lib.lib().glnn_linear_bn_stats_f32(_p(a), _ld(a), m, k, _p(w), w.stride(0), n, _p(bias), _p(z), _ld(z), _p(gamma), _p(beta), eps, momentum,
                                             _p(running_mean), _p(running_var), _p(nbt), _p(mean), _p(rstd), _p(a_scale), _p(a_shift),
                                             _p(ws), ws.numel(), _p(ws_bn), ws_bn.numel(), _stream())
    _lib.check(rc, "glnn_linear_bn_stats_f32")
    return z, mean, rstd, a_scale, a_shift


def bn_relu_bwd(da, z, gamma=None, mean=None, rstd=None, a_scale=None, a_shift=None, dz=None, dgamma=None,
                dbeta=None, workspace=None, drop_p=0.0, drop_seed=0, dz_col_sum=None, relu=True):
    """K5 glnn_bn_relu_bwd_f32 (relu=False: glnn_bn_bwd_f32, the norm -> dropout tail of GCN.forward).  Returns (dz, dgamma,
    dbeta); gamma=None => plain ReLU (+ dropout) backward.
    dz_col_sum: optional [h] output = column sums of dz (the bias gradient of the Linear in front)."""
    _need_cuda(da, z, gamma, mean, rstd, a_scale, a_shift, dz, dgamma, dbeta, workspace)
    _mat(da, "bn_relu_bwd da")
    _mat(z, "bn_relu_bwd z")
    rows, h = z.shape
    if dz is None:
        dz = torch.empty((rows, h), dtype=torch.float32, device=z.device)
    if gamma is not None:
        if dgamma is None:
            dgamma = torch.empty(h, dtype=torch.float32, device=z.device)
        if dbeta is None:
            dbeta = torch.empty(h, dtype=torch.float32, device=z.device)
    if workspace is None and (gamma is not None or dz_col_sum is not None):
        workspace = torch.empty((3 * ((rows + 127) // 128) + 2) * h, dtype=torch.float32, device=z.device)
    if relu:
        rc = _lib.lib().glnn_bn_relu_bwd_f32(_p(da), _ld(da), _p(z), _ld(z), rows, h, _p(gamma), _p(mean), _p(rstd),
                                             _p(a_scale), _p(a_shift), float(drop_p), int(drop_seed) & 0xFFFFFFFF,
                                             _p(dz), _ld(dz), _p(dgamma), _p(dbeta), _p(dz_col_sum),
                                             _p(workspace), workspace.numel() if workspace is not None else 0, _stream())
    else:
        rc = _lib.lib().glnn_bn_bwd_f32(_p(da), _ld(da), _p(z), _ld(z), rows, h, _p(gamma), _p(mean), _p(rstd),
                                        _p(a_scale), _p(a_shift), 0, float(drop_p), int(drop_seed) & 0xFFFFFFFF,
                                        _p(dz), _ld(dz), _p(dgamma), _p(dbeta), _p(dz_col_sum),
                                        _p(workspace), workspace.numel() if workspace is not None else 0, _stream())
    _lib.check(rc, "glnn_bn_relu_bwd_f32")
    return dz, dgamma, dbeta


def layernorm_fwd(z, gamma=None, beta=None, eps=1e-5, relu=True, drop_p=0.0, drop_seed=0, out=None, want_stats=True):
    """glnn_layernorm_fwd_f32: out = dropout(relu?(LayerNorm(z))); returns (out, mean_row, rstd_row) (stats None if not wanted)."""
    _need_cuda(z, gamma, beta, out)
    z = as_feat(z)
    rows, h = z.shape
    if out is None:
        out = feat_empty(rows, h, z.device)
    mean = torch.empty(rows, dtype=torch.float32, device=z.device) if want_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=z.device) if want_stats else None
    rc = _lib.lib().glnn_layernorm_fwd_f32(_p(z), _ld(z), rows, h, _p(_vec(gamma, h, "gamma")), _p(_vec(beta, h, "beta")), float(eps),
                                           1 if relu else 0, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(out), _ld(out), _p(mean),
                                           _p(rstd), _stream())
    _lib.check(rc, "glnn_layernorm_fwd_f32")
    return out, mean, rstd


def layernorm_bwd(da, z, gamma, beta, mean, rstd, relu=True, drop_p=0.0, drop_seed=0, dz=None, dz_col_sum=None, want_param_grads=True):
    """glnn_layernorm_bwd_f32.  Returns (dz, dgamma, dbeta)."""
    _need_cuda(da, z, gamma, beta, mean, rstd, dz, dz_col_sum)
    da, z = as_feat(da), as_feat(z)
    rows, h = z.shape
    if dz is None:
        dz = feat_empty(rows, h, z.device)
    dgamma = torch.empty(h, dtype=torch.float32, device=z.device) if (want_param_grads and gamma is not None) else None
    dbeta = torch.empty(h, dtype=torch.float32, device=z.device) if dgamma is not None else None
    ws = None
    if dgamma is not None or dz_col_sum is not None:
        ws = torch.empty(_lib.lib().glnn_layernorm_bwd_workspace_floats(rows, h), dtype=torch.float32, device=z.device)
    rc = _lib.lib().glnn_layernorm_bwd_f32(_p(da), _ld(da), _p(z), _ld(z), rows, h, _p(_vec(gamma, h, "gamma")), _p(_vec(beta, h, "beta")),
                                           _p(mean), _p(rstd), 1 if relu else 0, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(dz), _ld(dz),
                                           _p(dgamma), _p(dbeta), _p(dz_col_sum), _p(ws), ws.numel() if ws is not None else 0, _stream())
    _lib.check(rc, "glnn_layernorm_bwd_f32")
    return dz, dgamma, dbeta


def col_sum(x, out=None):
    """glnn_col_sum_f32: column sums of a [rows, h] matrix (a bias gradient)."""
    _need_cuda(x, out)
    _mat(x, "col_sum x")
    rows, h = x.shape
    if out is None:
        out = torch.empty(h, dtype=torch.float32, device=x.device)
    ws = torch.empty(((rows + 127) // 128) * h, dtype=torch.float32, device=x.device)
    rc = _lib.lib().glnn_col_sum_f32(_p(x), _ld(x), rows, h, _p(out), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "glnn_col_sum_f32")
    return out


class TensorTable:
    """Device-side pointer table for the multi-tensor Adam (built once per optimiser)."""

    def __init__(self, params, grads, exp_avg, exp_avg_sq):
        dev = params[0].device
        for group in (params, grads, exp_avg, exp_avg_sq):
            for t in group:
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError("TensorTable: contiguous float32 CUDA tensors required")
        self.keep = (list(params), list(grads), list(exp_avg), list(exp_avg_sq))
        mk = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev)
        self.p, self.g, self.m, self.v = mk(params), mk(grads), mk(exp_avg), mk(exp_avg_sq)
        self.sizes = torch.tensor([t.numel() for t in params], dtype=torch.int64, device=dev)
        self.n = len(params)
        self.max_size = max(t.numel() for t in params)
        # glnn_adam_desc (the one-call train step): the same table + a HOST copy of the gradient pointers
        import ctypes
        self.g_host = (ctypes.c_void_p * self.n)(*[t.data_ptr() for t in grads])
        self.desc = _lib.AdamDesc()
        d = self.desc
        d.params, d.grads, d.exp_avg, d.exp_avg_sq, d.sizes = _p(self.p), _p(self.g), _p(self.m), _p(self.v), _p(self.sizes)
        d.grads_host = ctypes.cast(self.g_host, ctypes.c_void_p)
        d.num_tensors, d.max_size = self.n, self.max_size


def adam_step(table, lr, step, weight_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    note_param_write()
    rc = _lib.lib().glnn_adam_step_f32(_p(table.p), _p(table.g), _p(table.m), _p(table.v), _p(table.sizes), table.n,
                                       table.max_size, lr, beta1, beta2, eps, weight_decay, step, _stream())
    _lib.check(rc, "glnn_adam_step_f32")


def act_fwd(z, a_scale=None, a_shift=None, drop_p=0.0, drop_seed=0, out=None, relu=True):
    """glnn_act_fwd_f32: out = dropout(relu(z * a_scale + a_shift)) (plain ReLU without a_scale/a_shift); relu=False:
    glnn_norm_drop_fwd_f32, the same without the ReLU (GCN's norm -> dropout tail)."""
    _need_cuda(z, a_scale, a_shift, out)
    _mat(z, "act_fwd z")
    rows, h = z.shape
    if out is None:
        out = feat_empty(rows, h, z.device)
    if relu:
        rc = _lib.lib().glnn_act_fwd_f32(_p(z), _ld(z), rows, h, _p(_vec(a_scale, h, "a_scale")), _p(_vec(a_shift, h, "a_shift")),
                                         float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(out), _ld(out), _stream())
    else:
        rc = _lib.lib().glnn_norm_drop_fwd_f32(_p(z), _ld(z), rows, h, _p(_vec(a_scale, h, "a_scale")), _p(_vec(a_shift, h, "a_shift")), 0,
                                               float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_act_fwd_f32")
    return out


def dropout_mask(rows, h, drop_p, drop_seed, device):
    mask = torch.empty((rows, h), dtype=torch.uint8, device=device)
    rc = _lib.lib().glnn_dropout_mask_u8(rows, h, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(mask), _stream())
    _lib.check(rc, "glnn_dropout_mask_u8")
    return mask


def sample_neighbors(indptr, indices, seeds, fanout, rng_seed):
    """glnn_sample_neighbors: returns (src [n_seeds, fanout] int32, cnt [n_seeds] int32)."""
    _need_cuda(indptr, indices, seeds)
    n = seeds.numel()
    src = torch.empty((n, fanout), dtype=torch.int32, device=seeds.device)
    cnt = torch.empty(n, dtype=torch.int32, device=seeds.device)
    rc = _lib.lib().glnn_sample_neighbors(_p(indptr), _p(indices), _p(seeds.contiguous()), n, int(fanout), int(rng_seed) & 0xFFFFFFFF,
                                          _p(src), _p(cnt), _stream())
    _lib.check(rc, "glnn_sample_neighbors")
    return src, cnt


def _i32(n, device):
    return torch.empty(max(int(n), 1), dtype=torch.int32, device=device)[:int(n)]


def _check_fanout(name, fanout):
    if isinstance(fanout, bool) or not isinstance(fanout, int) or not 1 <= fanout <= 64:
        raise ValueError(f"{name}: fanout must be an integer in [1, 64] (got {fanout!r})")


def sample_csr_indptr(indptr, n_dst, fanout):
    """glnn_sample_csr_indptr: the indptr [n_dst + 1] of the graph's sampled neighbourhood, the exclusive prefix sum of min(deg, fanout).
    It depends on the graph and the fan-out only (no seed); no host read."""
    _need_cuda(indptr)
    _check_fanout("sample_csr_indptr", fanout)
    n_dst = int(n_dst)
    if indptr.dtype != torch.int64 or indptr.dim() != 1 or not indptr.is_contiguous() or indptr.numel() < n_dst + 1:
        raise ValueError("sample_csr_indptr: indptr must be a contiguous int64 vector of at least n_dst + 1 entries")
    out = torch.empty(n_dst + 1, dtype=torch.int64, device=indptr.device)
    wsb = int(_lib.lib().glnn_sample_csr_workspace_bytes(n_dst))
    ws = torch.empty(max((wsb + 7) // 8, 1), dtype=torch.int64, device=indptr.device)
    with _Timed("sample_csr_indptr", n_dst=n_dst, fanout=fanout):
        rc = _lib.lib().glnn_sample_csr_indptr(_p(indptr), n_dst, fanout, _p(out), _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, "glnn_sample_csr_indptr")
    return out


def sample_csr_fill(indptr, indices, n_dst, n_src, out_indptr, nnz, fanout, rng_seed):
    """glnn_sample_csr_fill: the indices [nnz] (int32) of the sampled neighbourhood whose indptr is out_indptr = sample_csr_indptr(indptr,
    n_dst, fanout) and whose edge count is nnz = out_indptr[n_dst] (the caller's host value).  Row v = what sample_neighbors gives position
    v of seeds = arange(n_dst) under rng_seed, compacted."""
    _need_cuda(indptr, indices, out_indptr)
    _check_fanout("sample_csr_fill", fanout)
    _check_csr(indptr, indices, "sample_csr_fill")
    n_dst, nnz = int(n_dst), int(nnz)
    if out_indptr.dtype != torch.int64 or out_indptr.dim() != 1 or not out_indptr.is_contiguous() or out_indptr.numel() != n_dst + 1 \
            or indptr.numel() < n_dst + 1:
        raise ValueError("sample_csr_fill: indptr / out_indptr must be contiguous int64 vectors of n_dst + 1 entries")
    out = _i32(nnz, indptr.device)
    if nnz == 0:              # (no row has an in-edge: nothing to fill)
        return out
    with _Timed("sample_csr_fill", n_dst=n_dst, fanout=fanout, nnz=nnz):
        rc = _lib.lib().glnn_sample_csr_fill(_p(indptr), _p(indices), n_dst, int(n_src), _p(out_indptr), fanout, int(rng_seed) & 0xFFFFFFFF,
                                             _p(out), _stream())
    _lib.check(rc, "glnn_sample_csr_fill")
    return out


def block_build(seeds, graph_indptr=None, graph_indices=None, smp_src=None, smp_cnt=None, nnz_cap=None, want_global=False, n_nodes=0,
                global_only=False):
    """glnn_block_build_ids: one 1-hop block over the destination nodes `seeds` (int64 device vector).  n_nodes: the size of the id
    universe (every id < n_nodes) when known -- lets wide blocks index their tables by the id itself; 0 = unknown.
    Sampled mode: smp_src [ns, fanout] / smp_cnt [ns] from sample_neighbors.  Full-neighbour mode: the graph CSR and
    nnz_cap (an upper bound of the block's edge count).  Returns (indptr [ns+1], indices [nnz] local ids,
    gindices [nnz] global ids or None, input_nodes [n_src], nnz, n_src); ONE host read-back (the two counts).
    global_only: the global-id block -- (indptr, None, gindices, None, nnz, None): no table, no relabelling (the outermost block of a
    training batch whose consumer gathers from the global feature matrix)."""
    _need_cuda(seeds, graph_indptr, graph_indices, smp_src, smp_cnt)
    dev = seeds.device
    if seeds.dtype != torch.int64 or not seeds.is_contiguous():
        raise ValueError("block_build: seeds must be a contiguous int64 vector")
    ns = seeds.numel()
    if smp_src is not None:
        fanout = smp_src.shape[1]
        if smp_src.dtype != torch.int32 or smp_cnt.dtype != torch.int32 or smp_src.shape[0] != ns or not smp_src.is_contiguous():
            raise ValueError("block_build: smp_src [ns, fanout] / smp_cnt [ns] must be contiguous int32")
        nnz_cap = ns * fanout
    else:
        fanout = 0
        if graph_indptr is None or graph_indices is None or nnz_cap is None:
            raise ValueError("block_build: full-neighbour mode needs the graph CSR and nnz_cap")
    nnz_cap = int(nnz_cap)
    want_global = want_global or global_only
    indptr = torch.empty(ns + 1, dtype=torch.int64, device=dev)
    indices = None if global_only else _i32(nnz_cap, dev)
    gindices = _i32(nnz_cap, dev) if want_global else None
    input_nodes = None if global_only else torch.empty(ns + nnz_cap, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib().glnn_block_workspace_bytes(ns, nnz_cap))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev)
    rc = _lib.lib().glnn_block_build_ids(_p(graph_indptr) if smp_src is None else None, _p(graph_indices) if smp_src is None else None,
                                         _p(seeds), ns, _p(smp_src), _p(smp_cnt), fanout, nnz_cap, _p(indptr), _p(indices), _p(gindices),
                                         _p(input_nodes), _p(counts), int(n_nodes), _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, "glnn_block_build_ids")
    nnz, n_src = (int(v) for v in counts.tolist())          # the only host sync of the block
    if nnz < 0:
        raise _lib.GlnnError(f"block_build: a seed or neighbour id lies outside [0, n_nodes = {int(n_nodes)})")
    if nnz > nnz_cap:
        raise _lib.GlnnError(f"block_build: the block has {nnz} edges, more than nnz_cap = {nnz_cap}")
    if global_only:
        return indptr, None, gindices[:nnz], None, nnz, None
    return indptr, indices[:nnz], (gindices[:nnz] if want_global else None), input_nodes[:n_src], nnz, n_src


def csr_transpose(indptr, indices, n_dst, n_src, nnz, add_self=False):
    """glnn_csr_transpose: (t_indptr [n_src+1], t_indices [nnz (+ n_dst)]) of the CSR-by-destination graph; rows sorted.
    add_self: one extra entry u <- u per destination u (the h_dst term of the SAGE-gcn aggregator's backward)."""
    _need_cuda(indptr, indices)
    dev = indptr.device
    nnz_out = int(nnz) + (int(n_dst) if add_self else 0)
    t_indptr = torch.empty(n_src + 1, dtype=torch.int64, device=dev)
    t_indices = _i32(nnz_out, dev)
    wsb = int(_lib.lib().glnn_csr_transpose_workspace_bytes(n_src, nnz_out))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev)
    rc = _lib.lib().glnn_csr_transpose(_p(indptr), _p(indices) if nnz else None, n_dst, n_src, int(nnz), 1 if add_self else 0,
                                       _p(t_indptr), _p(t_indices) if nnz_out else None, _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, "glnn_csr_transpose")
    return t_indptr, t_indices


def _check_csr(indptr, indices, name):
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or indptr.dim() != 1 or indices.dim() != 1 \
            or not indptr.is_contiguous() or not indices.is_contiguous() or indptr.numel() < 1:
        raise ValueError(f"{name}: expected a CSR of contiguous int64 indptr [n + 1] and int32 indices")


def random_walk(indptr, indices, roots, length, rng_seed):
    """glnn_random_walk: out [n_roots, length + 1] int64, column 0 = roots; step s of walk i follows the in-edge number
    (drop_hash(rng_seed, i, s) * deg) >> 32 of the node it stands on and stays where it is on a node without in-edges.  1 <= length <= 64.
    Every root must be a node id of the graph (as glnn_sample_neighbors expects of its seeds)."""
    _need_cuda(indptr, indices, roots)
    _check_csr(indptr, indices, "random_walk")
    if roots.dtype != torch.int64 or roots.dim() != 1 or not roots.is_contiguous():
        raise ValueError("random_walk: roots must be a contiguous int64 vector")
    length = int(length)
    if not 1 <= length <= 64:
        raise ValueError(f"random_walk: length must be in [1, 64] (got {length})")
    n = roots.numel()
    out = torch.empty((n, length + 1), dtype=torch.int64, device=roots.device)
    with _Timed("random_walk", n_roots=n, length=length):
        rc = _lib.lib().glnn_random_walk(_p(indptr), _p(indices), _p(roots), n, length, int(rng_seed) & 0xFFFFFFFF, _p(out), _stream())
    _lib.check(rc, "glnn_random_walk")
    return out


def node2vec_walk(indptr, indices, roots, length, p, q, rng_seed):
    """glnn_node2vec_walk (docs/POSITION_SEMANTICS.md): random_walk's output with node2vec's second-order bias -- from step 2 on a candidate
    x of the current row is a return (x == walk[s - 2], weight 1/p), near (x is an entry of that node's row, weight 1) or far (weight 1/q),
    drawn by integer rejection sampling (at most 256 attempts).  p = q = 1 gives random_walk's bits.  p, q in [0.25, 4].  `roots`: int64
    vector on the CPU (checked against the graph there, then copied: no device read) or on the device (one copy back for the check).
    A refused argument raises ValueError with the C message."""
    _need_cuda(indptr, indices)
    _check_csr(indptr, indices, "node2vec_walk")
    if roots.dtype != torch.int64 or roots.dim() != 1:
        raise ValueError("node2vec_walk: roots must be an int64 vector")
    dev = indptr.device
    roots_host = roots.contiguous() if not roots.is_cuda else roots.cpu().contiguous()
    roots = roots.contiguous() if roots.is_cuda else roots_host.to(dev)
    n, b, length = indptr.numel() - 1, roots.numel(), int(length)
    out = torch.empty((b, length + 1) if 1 <= length <= 64 else (0, 1), dtype=torch.int64, device=dev)      # (else: refused below)
    with _Timed("node2vec_walk", n_roots=b, length=length):
        rc = _lib.lib().glnn_node2vec_walk(_p(indptr), _p(indices), n, _p(roots), _p(roots_host), b, length, float(p), float(q),
                                           int(rng_seed) & 0xFFFFFFFF, _p(out), _stream())
    _dw_check(rc, "glnn_node2vec_walk")
    return out


SELF_LOOP_MODES = ("keep", "add")


def induced_subgraph_direct(nc, n_nodes):
    """True when a glnn_induced_subgraph build over nc candidates of an n_nodes graph indexes its table by the node id itself, False when
    it probes the open-addressing table (the same results either way)."""
    return bool(_lib.lib().glnn_induced_subgraph_direct(int(nc), int(n_nodes)))


def induced_subgraph(indptr, indices, cand, self_loop="keep", nnz_cap=None):
    """glnn_induced_subgraph: the subgraph of the CSR-by-destination graph induced by the distinct ids of `cand` (int64 device vector,
    repeats allowed).  Returns (nodes [n_sub] = local id -> global id in order of first appearance, sub_indptr [n_sub + 1],
    sub_indices [nnz] int32 local ids, n_sub, nnz, zero_rows = the number of rows without an entry).  self_loop "keep": the graph's own
    entries (= CSRGraph.subgraph(cand) for candidates without repeats); "add": self entries dropped, one k <- k appended to every row.
    nnz_cap: the capacity of sub_indices; None = the bound that always suffices, the sum of the candidates' in-degrees (+ nc with "add"),
    which costs one host read before the call.  One more host read (the three counts) behind it."""
    _need_cuda(indptr, indices, cand)
    _check_csr(indptr, indices, "induced_subgraph")
    if cand.dtype != torch.int64 or cand.dim() != 1 or not cand.is_contiguous():
        raise ValueError("induced_subgraph: cand must be a contiguous int64 vector")
    if self_loop not in SELF_LOOP_MODES:
        raise ValueError(f"induced_subgraph: self_loop must be one of {SELF_LOOP_MODES} (got {self_loop!r})")
    dev = cand.device
    nc, n_nodes = cand.numel(), indptr.numel() - 1
    add = self_loop == "add"
    if nnz_cap is None:
        # (ids out of range are clamped for this read only: the builder reports them)
        c = cand.clamp(0, max(n_nodes - 1, 0))
        nnz_cap = (int((indptr[c + 1] - indptr[c]).sum().item()) if nc and n_nodes else 0) + (nc if add else 0)
    nnz_cap = int(nnz_cap)
    nodes = torch.empty(nc, dtype=torch.int64, device=dev)
    sub_indptr = torch.empty(nc + 1, dtype=torch.int64, device=dev)
    sub_indices = _i32(nnz_cap, dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    wsb = int(_lib.lib().glnn_induced_subgraph_workspace_bytes(nc, n_nodes))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev)
    with _Timed("induced_subgraph", nc=nc, nnz_cap=nnz_cap, self_loop=self_loop):
        rc = _lib.lib().glnn_induced_subgraph(_p(indptr), _p(indices), n_nodes, _p(cand), nc, 1 if add else 0, nnz_cap, _p(nodes),
                                              _p(sub_indptr), _p(sub_indices) if nnz_cap else None, _p(counts), _p(ws), ws.numel() * 8,
                                              _stream())
    _lib.check(rc, "glnn_induced_subgraph")
    n_sub, nnz, zero_rows = (int(v) for v in counts.tolist())
    if n_sub < 0:
        raise _lib.GlnnError(f"induced_subgraph: a candidate id lies outside [0, n_nodes = {n_nodes})")
    if nnz > nnz_cap:
        raise _lib.GlnnError(f"induced_subgraph: the subgraph has {nnz} entries, more than nnz_cap = {nnz_cap}")
    return nodes[:n_sub], sub_indptr[:n_sub + 1], sub_indices[:nnz], n_sub, nnz, zero_rows


def gather_rows(x, rows, out=None):
    _need_cuda(x, rows, out)
    x = as_feat(x)
    d = x.shape[1]
    if rows.dtype != torch.int64:
        raise ValueError("gather_rows: rows must be int64")
    if out is None:
        out = feat_empty(rows.numel(), d, x.device)
    rc = _lib.lib().glnn_gather_rows_f32(_p(x), _ld(x), _p(rows), rows.numel(), d, _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_gather_rows_f32")
    return out


def scatter_rows(x, rows, out):
    _need_cuda(x, rows, out)
    x = as_feat(x)
    d = x.shape[1]
    rc = _lib.lib().glnn_scatter_rows_f32(_p(x), _ld(x), _p(rows), rows.numel(), d, _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_scatter_rows_f32")
    return out


# --------------------------------------------------------------------------------------------- what the graph teachers' wrappers check
_GCNII_ENTRIES = ("gcnii_layer", "gcnii_layer_bwd")      # they word the two rules below their own way, and ask for a little more


def _csr_check(name, indptr, indices, n, x=None):
    """indptr int64, indices int32 (None: a launch without a graph); the GCNII entries also ask for indptr's n + 1 entries, and say so.
    x: the gathered rows, which must hold the graph's n rows."""
    if indptr is None:
        return
    _need_cuda(indptr, indices, x)
    with_len = name in _GCNII_ENTRIES
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or (with_len and indptr.numel() < n + 1):
        raise ValueError(f"{name}: indptr must be int64{' with n + 1 entries' if with_len else ''} and indices int32")
    if x is not None and x.shape[0] < n:
        raise ValueError(f"{name}: x must hold the graph's {n} rows")


def _rows_like(name, what, t, n, d):
    """t (None: no such buffer) is a row-major float32 [n, d]; the GCNII entries also ask for float4-addressable rows, and say so."""
    if t is None:
        return None
    _mat(t, f"{name} {what}")
    rows4 = name in _GCNII_ENTRIES
    if tuple(t.shape) != (n, d) or (rows4 and (_ld(t) % 4 or t.data_ptr() % 16)):
        raise ValueError(f"{name}: {what} must " + ("be [n, d] float32 with float4-addressable rows (ops.feat_empty)" if rows4 else "have x's shape"))
    return t


# --------------------------------------------------------------------------------------------- APPNP propagation
def appnp_propagate(indptr, indices, x, nnz, t, dst_norm, src_norm, h0, alpha, edge_drop=0.0, seed=0, x_scaled=True, last=False, out=None):
    """ONE forward iteration t (1-based) of APPNP propagation, glnn_appnp_prop_f32 (square graph, n = x.shape[0]):
    h_t = (1 - alpha) D_in^-1/2 M_t A D_out^-1/2 h_{t-1} + alpha h0.  x is the previous iteration's stored output -- already scaled by
    src_norm (x_scaled) -- or h0 itself at t = 1 (x_scaled=False: the kernel multiplies by src_norm per edge).  The stored output is
    src_norm * h_t unless `last`."""
    x = as_feat(x)
    h0 = as_feat(h0)
    n, d = h0.shape
    _csr_check("appnp_propagate", indptr, indices, n, x)
    _need_cuda(dst_norm, src_norm, h0, out)
    if x.shape[1] != d:
        raise ValueError("appnp_propagate: x and h0 must have the same width")
    if out is None:
        out = feat_empty(n, d, x.device)
    _mat(out, "appnp_propagate out")
    with _Timed("appnp_prop", d=d, n_dst=n, nnz=int(nnz), edge_drop=float(edge_drop)):
        rc = _lib.lib().glnn_appnp_prop_f32(_p(indptr), _p(indices), n, int(nnz), _p(x), _ld(x), d,
                                            None if x_scaled else _p(_vec(src_norm, n, "src_norm")), _p(_vec(dst_norm, n, "dst_norm")),
                                            None if last else _p(_vec(src_norm, n, "src_norm")), _p(h0), _ld(h0), float(alpha),
                                            float(edge_drop), int(seed) & 0xFFFFFFFF, int(t), _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_appnp_prop_f32")
    return out


def appnp_propagate_bwd(t_indptr, t_indices, t_eids, x, nnz, t, first, dst_norm, src_norm, alpha, edge_drop=0.0, seed=0, acc=None,
                        out=None):
    """ONE backward iteration t (called for t = K .. 1) over the transposed graph with its edge ids (csr_transpose_eids),
    glnn_appnp_prop_bwd_f32.  first (t = K): x = dL/dh_K unscaled and the running sum starts at alpha * x; otherwise x is the previous
    call's output dst_norm * g_t and `acc` the running sum (updated in place).  Returns out: dst_norm * g_{t-1} for t > 1, dL/dh0 at t = 1."""
    x = as_feat(x)
    n, d = x.shape
    _csr_check("appnp_propagate_bwd", t_indptr, t_indices, n, x)
    _need_cuda(t_eids, dst_norm, src_norm, acc, out)
    if out is None:
        out = feat_empty(n, d, x.device)
    _mat(out, "appnp_propagate_bwd out")
    if acc is not None:
        _mat(acc, "appnp_propagate_bwd acc")
    with _Timed("appnp_prop_bwd", d=d, n_dst=n, nnz=int(nnz), edge_drop=float(edge_drop)):
        rc = _lib.lib().glnn_appnp_prop_bwd_f32(_p(t_indptr), _p(t_indices), _p(t_eids), n, int(nnz), _p(x), _ld(x), d,
                                                _p(_vec(dst_norm, n, "dst_norm")) if first else None, _p(_vec(src_norm, n, "src_norm")),
                                                _p(_vec(dst_norm, n, "dst_norm")) if t > 1 else None, float(alpha), float(edge_drop),
                                                int(seed) & 0xFFFFFFFF, int(t), 1 if first else 0, _p(acc), 0 if acc is None else _ld(acc),
                                                _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_appnp_prop_bwd_f32")
    return out


# --------------------------------------------------------------------------------------------- GPR-GNN propagation
def gpr_col_tiles(d):
    """The 256-column tiles of a d-wide row: row_dot of gpr_prop holds one scalar per coefficient, tile and row."""
    return (int(d) + 255) // 256


def gpr_prop(indptr, indices, nnz, x, k, x_norm, row_norm, out_norm, gamma, acc, out=None, h0=None, row_dot=None):
    """ONE step k of GPR-GNN propagation, glnn_gpr_prop_f32 (square graph, n = x.shape[0]), forward or backward by what the caller passes
    (in-CSR with x_norm = out_norm = src_norm, row_norm = dst_norm; transposed CSR with the norms swapped):
    row = row_norm * A (x_norm * x at k = 1, the pre-scaled x after it); acc = (gamma[0] * x at k = 1, else acc) + gamma[k] * row, in
    place; out = out_norm * row unless out is None (the last step).  h0 + row_dot (the backward): row_dot[k] = the per-row <row, h0>, and
    row_dot[0] = <x, h0> at k <= 1.  k = 0: acc = gamma[0] * x without a graph.  gamma is read on the device.  Returns out."""
    _need_cuda(indptr, indices, x, x_norm, row_norm, out_norm, gamma, acc, out, h0, row_dot)
    x = as_feat(x)
    n, d = x.shape
    k = int(k)
    _rows_like("gpr_prop", "acc", acc, n, d)
    if gamma.dtype != torch.float32 or gamma.dim() != 1 or gamma.numel() < k + 1 or not gamma.is_contiguous():
        raise ValueError(f"gpr_prop: gamma must be a contiguous float32 vector of >= {k + 1} coefficients")
    if k > 0:
        _csr_check("gpr_prop", indptr, indices, n, x)
        _vec(row_norm, n, "row_norm")
    _rows_like("gpr_prop", "out", out, n, d)
    if (h0 is None) != (row_dot is None):
        raise ValueError("gpr_prop: h0 and row_dot go together")
    if h0 is not None:
        h0 = _rows_like("gpr_prop", "h0", as_feat(h0), n, d)
        if row_dot.dtype != torch.float32 or not row_dot.is_contiguous() or row_dot.numel() < (k + 1) * gpr_col_tiles(d) * n:
            raise ValueError("gpr_prop: row_dot must be contiguous float32 with >= (k + 1) * ceil(d / 256) * n elements")
    with _Timed("gpr_prop", d=d, n_dst=n, nnz=int(nnz), k=k):
        rc = _lib.lib().glnn_gpr_prop_f32(_p(indptr), _p(indices), n, int(nnz), _p(x), _ld(x), d, _p(_vec(x_norm, n, "x_norm")),
                                          _p(row_norm), _p(_vec(out_norm, n, "out_norm")), _p(gamma), k, _p(acc), _ld(acc), _p(out),
                                          0 if out is None else _ld(out), _p(h0), 0 if h0 is None else _ld(h0), _p(row_dot), _stream())
    _lib.check(rc, "glnn_gpr_prop_f32")
    return out


def gpr_fold(row_dot, rows, m, out=None):
    """dgamma [rows] = the fixed-order fp64 row sums of row_dot [rows, m] (glnn_gpr_fold_f32: chunks of _lib.GPR_FOLD_CHUNK entries, then
    the chunk partials)."""
    _need_cuda(row_dot, out)
    rows, m = int(rows), int(m)
    if row_dot.dtype != torch.float32 or not row_dot.is_contiguous() or row_dot.numel() < rows * m:
        raise ValueError("gpr_fold: row_dot must be contiguous float32 with >= rows * m elements")
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=row_dot.device)
    _vec(out, rows, "gpr_fold out")
    chunks = (m + _lib.GPR_FOLD_CHUNK - 1) // _lib.GPR_FOLD_CHUNK
    ws = torch.empty(max(rows * chunks, 1), dtype=torch.float64, device=row_dot.device)
    rc = _lib.lib().glnn_gpr_fold_f32(_p(row_dot), rows, m, _p(out), _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, "glnn_gpr_fold_f32")
    return out


# --------------------------------------------------------------------------------------------- DAGNN propagation
DAGNN_MAX_WIDTH = 256           # kMaxD of csrc/dagnn.hip: the gate is one row-wide dot product


def _dagnn_gate(name, w, b, d):
    """The gate parameters as the kernels read them: w a contiguous float32 [d] (or nn.Linear's [1, d]), b a float32 [1]."""
    _need_cuda(w, b)
    if w.dtype != torch.float32 or w.numel() != d or not w.is_contiguous() or b.dtype != torch.float32 or b.numel() != 1:
        raise ValueError(f"{name}: w must be a contiguous float32 vector of {d} gate weights and b a float32 scalar tensor")


def _dagnn_width(name, d):
    if d > DAGNN_MAX_WIDTH:
        raise NotImplementedError(f"{name}: DAGNN rows of at most {DAGNN_MAX_WIDTH} columns (the gate is one row-wide dot product; got {d})")


def dagnn_gate(x, k, w, b, acc, score=None):
    """Hop k of DAGNN's forward, glnn_dagnn_gate_f32 (x = H_k [n, d], d <= 256): s = sigmoid(<x, w> + b); acc = (0 at k = 0, else acc) + s * x,
    in place; score (training, [(K + 1) * n]): score[k * n + i] = s.  w, b are read on the device.  Returns acc."""
    _need_cuda(x, acc, score)
    x = as_feat(x)
    n, d = x.shape
    k = int(k)
    _dagnn_width("dagnn_gate", d)
    _dagnn_gate("dagnn_gate", w, b, d)
    _rows_like("dagnn_gate", "acc", acc, n, d)
    if score is not None and (score.dtype != torch.float32 or not score.is_contiguous() or score.numel() < (k + 1) * n):
        raise ValueError("dagnn_gate: score must be contiguous float32 with >= (k + 1) * n elements")
    with _Timed("dagnn_gate", d=d, n_dst=n, k=k):
        rc = _lib.lib().glnn_dagnn_gate_f32(_p(x), _ld(x), n, d, _p(w), _p(b), k, _p(acc), _ld(acc), _p(score), _stream())
    _lib.check(rc, "glnn_dagnn_gate_f32")
    return acc


def dagnn_gate_bwd(g, h, k, score, w, t, out, q):
    """Hop k of DAGNN's backward, glnn_dagnn_gate_bwd_f32: q[k * n + i] = <g, h> s (1 - s) with s = score[k * n + i], g = dL/dresult,
    h = the saved H_k; out = s * g + q * w + t, t = P^T T_{k+1} (None at k = K; may be `out` itself: in place).  Returns out."""
    _need_cuda(g, h, score, w, t, out, q)
    g, h = as_feat(g), as_feat(h)
    n, d = g.shape
    k = int(k)
    _dagnn_width("dagnn_gate_bwd", d)
    if w.dtype != torch.float32 or w.numel() != d or not w.is_contiguous():
        raise ValueError(f"dagnn_gate_bwd: w must be a contiguous float32 vector of {d} gate weights")
    for what, m in (("h", h), ("t", t), ("out", out)):
        _rows_like("dagnn_gate_bwd", what, m, n, d)
    if out is None:
        raise ValueError("dagnn_gate_bwd: out is required")
    for what, v in (("score", score), ("q", q)):
        if v is None or v.dtype != torch.float32 or not v.is_contiguous() or v.numel() < (k + 1) * n:
            raise ValueError(f"dagnn_gate_bwd: {what} must be contiguous float32 with >= (k + 1) * n elements")
    with _Timed("dagnn_gate_bwd", d=d, n_dst=n, k=k):
        rc = _lib.lib().glnn_dagnn_gate_bwd_f32(_p(g), _ld(g), _p(h), _ld(h), n, d, _p(score), _p(w), k, _p(t), 0 if t is None else _ld(t),
                                                _p(out), _ld(out), _p(q), _stream())
    _lib.check(rc, "glnn_dagnn_gate_bwd_f32")
    return out


def dagnn_fold(hs, q, dw=None, db=None):
    """(dw [d], db [1]) = (hs^T q, sum q) over the (K + 1) * n rows of the saved stack hs, glnn_dagnn_fold_f32: fixed-order fp64 sums in chunks
    of _lib.DAGNN_FOLD_CHUNK rows, then the chunk partials."""
    _need_cuda(hs, q, dw, db)
    hs = _mat(hs, "dagnn_fold hs")
    rows, d = hs.shape
    _dagnn_width("dagnn_fold", d)
    if _ld(hs) % 4 or hs.data_ptr() % 16:
        raise ValueError("dagnn_fold: hs must have float4-addressable rows (ops.feat_empty)")
    _vec(q, rows, "dagnn_fold q")
    if dw is None:
        dw = torch.empty(d, dtype=torch.float32, device=hs.device)
    if db is None:
        db = torch.empty(1, dtype=torch.float32, device=hs.device)
    _vec(dw, d, "dagnn_fold dw")
    _vec(db, 1, "dagnn_fold db")
    wsb = int(_lib.lib().glnn_dagnn_fold_workspace_bytes(rows, d))
    ws = torch.empty(max(wsb // 8, 1), dtype=torch.float64, device=hs.device)
    rc = _lib.lib().glnn_dagnn_fold_f32(_p(hs), _ld(hs), _p(q), rows, d, _p(dw), _p(db), _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, "glnn_dagnn_fold_f32")
    return dw, db


# --------------------------------------------------------------------------------------------- PNA aggregation (docs/PNA_SEMANTICS.md)
PNA_MAX_WIDTH = 256             # GLNN_PNA_MAX_WIDTH of include/glnn_hip.h: one float4 lane row
PNA_AGGREGATORS = ("mean", "min", "max", "std")                     # the order of the four parts of S
PNA_SCALERS = ("identity", "amplification", "attenuation")          # the order of the three blocks of T
PNA_STD_EPS = 1e-5


def _pna_width(name, d):
    if d > PNA_MAX_WIDTH:
        raise NotImplementedError(f"{name}: PNA rows of at most {PNA_MAX_WIDTH} columns (one float4 lane row; got {d})")


def _pna_parts(name, what, t, n, parts, d, dtype=torch.float32):
    """t is a contiguous [n, parts * round4(d)] buffer of `dtype` with 16-byte aligned rows: the part layout of S, dS and arg."""
    if t.dtype != dtype or t.dim() != 2 or tuple(t.shape) != (n, parts * round4(d)) or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} [n, {parts} * round4(d)] = [{n}, {parts * round4(d)}] buffer")
    return t


def pna_agg_fwd(indptr, indices, nnz, b, n_dst, a=None, want_arg=False, out=None):
    """glnn_pna_agg_fwd_f32: (S, mu, arg).  S [n_dst, 4 * round4(d)] = [a + mean | a + min | a + max | std] of the rows b[u] over the
    in-edges u -> v, every neighbour row gathered once; a (optional, [n_dst, d]) the destination's own term; a row without in-edges gets
    [0 | 0 | 0 | sqrt(1e-5)].  want_arg (training): mu [n_dst, d] the plain mean and arg int32 [n_dst, 2 * round4(d)] = [argmin | argmax],
    the CSR position of the first edge that attains the value (-1: no in-edges / padding); else (S, None, None)."""
    _need_cuda(indptr, indices, b, a, out)
    b = as_feat(b)
    n_src, d = b.shape
    _pna_width("pna_agg_fwd", d)
    _csr_check("pna_agg_fwd", indptr, indices, 0)
    if indptr.numel() < n_dst + 1:
        raise ValueError(f"pna_agg_fwd: indptr must hold n_dst + 1 = {n_dst + 1} entries")
    if a is not None:
        a = as_feat(a)
        if tuple(a.shape) != (n_dst, d):
            raise ValueError(f"pna_agg_fwd: a must be [n_dst, d] = [{n_dst}, {d}] (got {tuple(a.shape)})")
    dp = round4(d)
    s = torch.empty((n_dst, 4 * dp), dtype=torch.float32, device=b.device) if out is None else _pna_parts("pna_agg_fwd", "out", out, n_dst, 4, d)
    mu = arg = None
    if want_arg:
        mu = feat_empty(n_dst, d, b.device)
        arg = torch.empty((n_dst, 2 * dp), dtype=torch.int32, device=b.device)
    with _Timed("pna_agg_fwd", d=d, n_dst=n_dst):
        rc = _lib.lib().glnn_pna_agg_fwd_f32(_p(indptr), _p(indices), n_dst, n_src, int(nnz), _p(b), _ld(b), d, _p(a), 0 if a is None else _ld(a),
                                             _p(s), 4 * dp, _p(mu), 0 if mu is None else _ld(mu), _p(arg), 2 * dp, _stream())
    _lib.check(rc, "glnn_pna_agg_fwd_f32")
    return s, mu, arg


def pna_agg_bwd(graph, ds, b, mu, sigma, arg, out=None):
    """glnn_pna_agg_bwd_f32 over `graph` (CSRGraph: its row pointers for the degrees, its cached transpose with edge ids for the pass):
    db [n_src, d] from ds [n_dst, 4 * round4(d)] = [g_mean | g_min | g_max | g_std], the forward's b, mu, arg and sigma -- a [n_dst, d]
    matrix or the forward's whole S, whose last part it is.  Every row of db is written; a source no edge references gets zeros."""
    _need_cuda(ds, b, mu, sigma, arg, out)
    b = as_feat(b)
    n_src, d = b.shape
    n_dst = graph.num_dst_nodes()
    _pna_width("pna_agg_bwd", d)
    dp = round4(d)
    if n_src != graph.num_src_nodes():
        raise ValueError(f"pna_agg_bwd: b must hold the graph's {graph.num_src_nodes()} source rows")
    _pna_parts("pna_agg_bwd", "ds", ds, n_dst, 4, d)
    _pna_parts("pna_agg_bwd", "arg", arg, n_dst, 2, d, torch.int32)
    if tuple(sigma.shape) == (n_dst, 4 * dp):
        sigma = _pna_parts("pna_agg_bwd", "sigma", sigma, n_dst, 4, d)[:, 3 * dp:3 * dp + d]
    mu, sigma = as_feat(mu), as_feat(sigma)
    for what, t in (("mu", mu), ("sigma", sigma)):
        if tuple(t.shape) != (n_dst, d):
            raise ValueError(f"pna_agg_bwd: {what} must be [n_dst, d] = [{n_dst}, {d}] (got {tuple(t.shape)})")
    if out is None:
        out = feat_empty(n_src, d, b.device)
    _rows_like("pna_agg_bwd", "out", out, n_src, d)
    if _ld(out) % 4 or out.data_ptr() % 16:
        raise ValueError("pna_agg_bwd: out must have float4-addressable rows (ops.feat_empty)")
    t, t_eids = graph.transposed_eids()
    with _Timed("pna_agg_bwd", d=d, n_dst=n_src):
        rc = _lib.lib().glnn_pna_agg_bwd_f32(_p(graph.indptr), n_dst, _p(t.indptr), _p(t.indices), _p(t_eids), n_src, graph.num_edges(),
                                             _p(ds), 4 * dp, _p(b), _ld(b), d, _p(mu), _ld(mu), _p(sigma), _ld(sigma), _p(arg), 2 * dp,
                                             _p(out), _ld(out), _stream())
    _lib.check(rc, "glnn_pna_agg_bwd_f32")
    return out


def _pna_delta(name, delta):
    delta = float(delta)
    if not delta > 0:
        raise ValueError(f"{name}: PNA's delta must be positive (got {delta})")
    return delta


def pna_scale_fwd(indptr, z, out, delta, relu=False):
    """glnn_pna_scale_fwd_f32, in place on out [n, fo]: out = act(out + z_0 + s_amp z_1 + s_att z_2) with z [n, 3 * round4(fo)] the three
    scaler blocks of the stacked product and s_amp = log(max(deg, 1) + 1) / delta = 1 / s_att per row."""
    _need_cuda(indptr, z, out)
    _mat(out, "pna_scale_fwd out")
    n, fo = out.shape
    if z.dtype != torch.float32 or tuple(z.shape) != (n, 3 * round4(fo)) or z.stride(1) != 1 or _ld(out) < round4(fo):
        raise ValueError(f"pna_scale_fwd: z must be float32 [n, 3 * round4(fo)] = [{n}, {3 * round4(fo)}] and out an ops.feat_empty buffer")
    rc = _lib.lib().glnn_pna_scale_fwd_f32(_p(indptr), n, fo, _pna_delta("pna_scale_fwd", delta), _p(z), _ld(z), _p(out), _ld(out),
                                           1 if relu else 0, _stream())
    _lib.check(rc, "glnn_pna_scale_fwd_f32")
    return out


def pna_scale_bwd(indptr, g, delta):
    """glnn_pna_scale_bwd_f32: dz [n, 3 * round4(fo)] = [g | s_amp g | s_att g] from g [n, fo] = dL/d out behind the activation mask."""
    _need_cuda(indptr, g)
    g = _mat(g, "pna_scale_bwd g")
    n, fo = g.shape
    dz = torch.empty((n, 3 * round4(fo)), dtype=torch.float32, device=g.device)
    rc = _lib.lib().glnn_pna_scale_bwd_f32(_p(indptr), n, fo, _pna_delta("pna_scale_bwd", delta), _p(g), _ld(g), _p(dz), 3 * round4(fo), _stream())
    _lib.check(rc, "glnn_pna_scale_bwd_f32")
    return dz


def pna_da(indptr, ds, d):
    """glnn_pna_da_f32: da [n, d] = g_mean + g_min + g_max of ds [n, 4 * round4(d)] for the rows with in-edges, zeros for the others."""
    _need_cuda(indptr, ds)
    n = ds.shape[0]
    _pna_parts("pna_da", "ds", ds, n, 4, d)
    da = feat_empty(n, d, ds.device)
    rc = _lib.lib().glnn_pna_da_f32(_p(indptr), n, d, _p(ds), 4 * round4(d), _p(da), _ld(da), _stream())
    _lib.check(rc, "glnn_pna_da_f32")
    return da


# --------------------------------------------------------------------------------------------- GCNII conv layer
GCNII_MAX_HIDDEN = 256         # kMaxD of csrc/gcnii.hip: the kernel's tile width


def _gcnii_check(name, indptr, indices, n, d, tile_order):
    if d > GCNII_MAX_HIDDEN:
        raise NotImplementedError(f"{name}: GCNII hidden widths of at most {GCNII_MAX_HIDDEN} (the fused kernel's tile; got {d})")
    _csr_check(name, indptr, indices, n)
    if tile_order is not None and (tile_order.dtype != torch.int32 or not tile_order.is_contiguous() or tile_order.numel() != (n + 31) // 32):
        raise ValueError(f"{name}: tile_order must be a contiguous int32 permutation of the ceil(n / 32) tile ids")


def gcnii_layer(indptr, indices, nnz, x, h0, w, alpha, beta, row_norm, x_norm=None, out_norm=None, drop_p=0.0, drop_seed=0, s_out=None,
                out=None, w_packed=None, tile_order=None):
    """ONE GCNII conv layer forward, glnn_gcnii_layer_f32 (square graph, n = x.shape[0], d <= 256):
    S = (1 - alpha) row_norm * A (x_norm * drop(x)) + alpha h0;  out = out_norm * relu((1 - beta) S + beta S w^T).  x_norm None: x is the
    previous layer's output already scaled by it (that launch's out_norm); out_norm None: unscaled rows.  drop: the feature dropout keyed
    by the source row (dropout_mask(n, d, drop_p, drop_seed)).  s_out (optional, [n, d]) receives S.  w [d, d] in nn.Linear orientation
    (w_packed: pack_weight(w) of a caller that has it).  Returns out."""
    _need_cuda(indptr, indices, x, h0, w, row_norm, x_norm, out_norm, s_out, out, w_packed, tile_order)
    x, h0 = as_feat(x), as_feat(h0)
    n, d = h0.shape
    _gcnii_check("gcnii_layer", indptr, indices, n, d, tile_order)
    if tuple(x.shape) != (n, d) or tuple(w.shape) != (d, d):
        raise ValueError("gcnii_layer: x and h0 must be [n, d] and w [d, d]")
    if w_packed is None:
        w_packed = pack_weight(w)
    if out is None:
        out = feat_empty(n, d, x.device)
    _rows_like("gcnii_layer", "out", out, n, d)
    _rows_like("gcnii_layer", "s_out", s_out, n, d)
    with _Timed("gcnii_layer", d=d, n_dst=n, nnz=int(nnz), train=s_out is not None):
        rc = _lib.lib().glnn_gcnii_layer_f32(
            _p(indptr), _p(indices), n, int(nnz), _p(x), _ld(x), d, _p(_vec(x_norm, n, "x_norm")), _p(_vec(row_norm, n, "row_norm")),
            _p(_vec(out_norm, n, "out_norm")), _p(h0), _ld(h0), float(alpha), float(beta), _p(w_packed), float(drop_p),
            int(drop_seed) & 0xFFFFFFFF, _p(s_out), 0 if s_out is None else _ld(s_out), _p(out), _ld(out), _p(tile_order), _stream())
    _lib.check(rc, "glnn_gcnii_layer_f32")
    return out


def gcnii_layer_bwd(t_indptr, t_indices, nnz, g, h, wt, alpha, beta, dz_out, dh0_acc, first, row_norm=None, x_norm=None, out_norm=None,
                    plain=False, drop_p=0.0, drop_seed=0, dz_scale=1.0, ds_out=None, wt_packed=None, tile_order=None):
    """ONE GCNII conv layer backward, glnn_gcnii_layer_bwd_f32, over the transposed CSR (norms swapped):
    dZ = [h > 0] * drop'(plain ? g : (1 - alpha) row_norm * A^T (x_norm * g)), drop' keyed by the own row; dz_out = dz_scale dZ;
    dS = (1 - beta) dZ + beta dZ W with wt = W^T (wt_packed: pack_weight(wt)); returns ds_out = out_norm * dS;
    dh0_acc = (0 if first else dh0_acc) + alpha dS.  wt None (the launch behind layer 1): dz_out = drop'(...) + dh0_acc = dL/dH_0 (h None; a given h masks the SUM: [h > 0] (drop'(...) + dh0_acc)),
    nothing else is written, returns dz_out."""
    _need_cuda(t_indptr, t_indices, g, h, wt, dz_out, dh0_acc, row_norm, x_norm, out_norm, ds_out, wt_packed, tile_order)
    g = as_feat(g)
    h = None if h is None else as_feat(h)
    n, d = g.shape
    _gcnii_check("gcnii_layer_bwd", None if plain else t_indptr, t_indices, n, d, tile_order)
    tail = wt is None and wt_packed is None
    if not tail:
        if wt_packed is None:
            if tuple(wt.shape) != (d, d):
                raise ValueError("gcnii_layer_bwd: wt must be [d, d]")
            wt_packed = pack_weight(wt)
        if ds_out is None:
            ds_out = feat_empty(n, d, g.device)
        if h is None:
            raise ValueError("gcnii_layer_bwd: a layer launch needs the saved h")
    elif ds_out is not None or plain or first:
        raise ValueError("gcnii_layer_bwd: the dH_0 launch (wt None) is a gather behind a layer launch and writes dz_out alone")
    if dz_out is None or dh0_acc is None:
        raise ValueError("gcnii_layer_bwd: dz_out and dh0_acc are required")
    if h is not None and tuple(h.shape) != (n, d):
        raise ValueError("gcnii_layer_bwd: h must have g's shape")
    for what, t in (("dz_out", dz_out), ("ds_out", ds_out), ("dh0_acc", dh0_acc)):
        _rows_like("gcnii_layer_bwd", what, t, n, d)
    with _Timed("gcnii_layer_bwd", d=d, n_dst=n, nnz=int(nnz), plain=bool(plain)):
        rc = _lib.lib().glnn_gcnii_layer_bwd_f32(
            _p(t_indptr), _p(t_indices), n, int(nnz), _p(g), _ld(g), d, _p(_vec(x_norm, n, "x_norm")), _p(_vec(row_norm, n, "row_norm")),
            _p(_vec(out_norm, n, "out_norm")), 1 if plain else 0, _p(h), 0 if h is None else _ld(h), float(drop_p),
            int(drop_seed) & 0xFFFFFFFF, float(alpha), float(beta), _p(wt_packed), float(dz_scale), _p(dz_out), _ld(dz_out), _p(ds_out),
            0 if ds_out is None else _ld(ds_out), _p(dh0_acc), _ld(dh0_acc), 1 if first else 0, _p(tile_order), _stream())
    _lib.check(rc, "glnn_gcnii_layer_bwd_f32")
    return dz_out if tail else ds_out


def csr_transpose_eids(indptr, indices, n_dst, n_src, nnz):
    """glnn_csr_transpose_eids: (t_indptr [n_src+1], t_indices [nnz], t_eids [nnz]) -- csr_transpose plus the original edge id (CSR
    position) of every transposed entry."""
    _need_cuda(indptr, indices)
    dev = indptr.device
    nnz = int(nnz)
    t_indptr = torch.empty(n_src + 1, dtype=torch.int64, device=dev)
    t_indices, t_eids = _i32(nnz, dev), _i32(nnz, dev)
    wsb = int(_lib.lib().glnn_csr_transpose_workspace_bytes(n_src, nnz))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev)
    rc = _lib.lib().glnn_csr_transpose_eids(_p(indptr), _p(indices) if nnz else None, n_dst, n_src, nnz, _p(t_indptr),
                                            _p(t_indices) if nnz else None, _p(t_eids) if nnz else None, _p(ws), ws.numel() * 8, _stream())
    _lib.check(rc, "glnn_csr_transpose_eids")
    return t_indptr, t_indices, t_eids


# --------------------------------------------------------------------------------------------- DeepWalk position embeddings (csrc/deepwalk.hip)
DEEPWALK_MAX_DIM = 256          # kDwMaxD of csrc/deepwalk.hip


def _dw_check(rc, what):
    """A refused argument of the DeepWalk entries is the caller's ValueError, with the C message; anything else is a GlnnError."""
    if rc == -1:
        raise ValueError(_lib.lib().glnn_last_error().decode(errors="replace"))
    _lib.check(rc, what)


def _dw_table(t, name, rows=None):
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name}: expected a contiguous float32 matrix" + ("" if rows is None else f" of {rows} rows"))
    return t


def deepwalk_windows(n_roots, length, context, negatives):
    """(Q, R) of a DeepWalk step: Q = n_roots * (length + 2 - context) windows of R = (1 + negatives) * (context - 1) entries."""
    return int(n_roots) * (int(length) + 2 - int(context)), (1 + int(negatives)) * (int(context) - 1)


def deepwalk_pairs(indptr, indices, roots, length, context, negatives, walk_seed, neg_seed):
    """glnn_deepwalk_pairs (docs/POSITION_SEMANTICS.md): walks = random_walk(roots, length, walk_seed), then per window q = i * nwin + j its
    start walks[i, j] and its pair row: the context - 1 positives walks[i, j + 1 ..], then negatives * (context - 1) uniform negatives
    (drop_hash(neg_seed, q, t') * N) >> 32.  `roots`: int64 vector on the CPU (checked against the graph there, then copied to the device:
    no device read) or on the device (one copy back for the check).  Returns (walks [B, length + 1] int64, start [Q] int32, rest [Q, R] int32,
    pair_indptr [Q + 1], win_indptr [Q + 1]) -- the two indptr arrays are q * R and q, what the transposes of the pair list and of the
    start list read."""
    _need_cuda(indptr, indices)
    _check_csr(indptr, indices, "deepwalk_pairs")
    if roots.dtype != torch.int64 or roots.dim() != 1:
        raise ValueError("deepwalk_pairs: roots must be an int64 vector")
    dev = indptr.device
    roots_host = roots.contiguous() if not roots.is_cuda else roots.cpu().contiguous()
    roots = roots.contiguous() if roots.is_cuda else roots_host.to(dev)
    n, b = indptr.numel() - 1, roots.numel()
    length, context, negatives = int(length), int(context), int(negatives)
    q, r = deepwalk_windows(b, length, context, negatives)
    ok = 1 <= length <= 64 and 2 <= context <= length + 1 and negatives >= 1 and q * r < 2 ** 31      # (else: refused below, nothing allocated)
    q, r = (q, r) if ok else (0, 0)
    walks = torch.empty((b, length + 1) if ok else (0, 1), dtype=torch.int64, device=dev)
    start, rest = _i32(q, dev), _i32(q * r, dev)
    pair_indptr = torch.empty(q + 1, dtype=torch.int64, device=dev)
    win_indptr = torch.empty(q + 1, dtype=torch.int64, device=dev)
    with _Timed("deepwalk_pairs", n_roots=b, length=length, context=context, negatives=negatives):
        rc = _lib.lib().glnn_deepwalk_pairs(_p(indptr), _p(indices), n, _p(roots), _p(roots_host), b, length, context, negatives,
                                            int(walk_seed) & 0xFFFFFFFF, int(neg_seed) & 0xFFFFFFFF, _p(walks), _p(start), _p(rest),
                                            _p(pair_indptr), _p(win_indptr), _stream())
    _dw_check(rc, "glnn_deepwalk_pairs")
    return walks, start, rest.view(q, r), pair_indptr, win_indptr


def deepwalk_pairs_from_walks(walks, n_nodes, context, negatives, neg_seed, neg_cdf=None):
    """glnn_deepwalk_pairs_from_walks: deepwalk_pairs' pair lists from walks [B, L + 1] (int64, device) that are given -- random_walk's or
    node2vec_walk's.  neg_cdf None: the uniform negatives of deepwalk_pairs (the same bits from the same walks).  neg_cdf [n_nodes] (int64
    values in [0, 2^32), CPU or device; position.negative_cdf builds it): the negative of the draw r is the number of n < n_nodes - 1 with
    neg_cdf[n] <= r.  Returns (start [Q] int32, rest [Q, R] int32, pair_indptr [Q + 1], win_indptr [Q + 1])."""
    _need_cuda(walks)
    if walks.dtype != torch.int64 or walks.dim() != 2 or not walks.is_contiguous():
        raise ValueError("deepwalk_pairs_from_walks: walks must be a contiguous int64 matrix [B, L + 1]")
    dev = walks.device
    b, length = walks.shape[0], walks.shape[1] - 1
    n, context, negatives = int(n_nodes), int(context), int(negatives)
    cdf = None
    if neg_cdf is not None:
        cdf = deepwalk_cdf_words(neg_cdf, dev)
        if cdf.numel() != n:
            raise ValueError(f"deepwalk_pairs_from_walks: neg_cdf must have one entry per node ({n}), got {cdf.numel()}")
    q, r = deepwalk_windows(b, length, context, negatives)
    ok = 1 <= length <= 64 and 2 <= context <= length + 1 and negatives >= 1 and q * r < 2 ** 31      # (else: refused below, nothing allocated)
    q, r = (q, r) if ok else (0, 0)
    start, rest = _i32(q, dev), _i32(q * r, dev)
    pair_indptr = torch.empty(q + 1, dtype=torch.int64, device=dev)
    win_indptr = torch.empty(q + 1, dtype=torch.int64, device=dev)
    with _Timed("deepwalk_pairs_from_walks", n_roots=b, length=length, context=context, negatives=negatives):
        rc = _lib.lib().glnn_deepwalk_pairs_from_walks(_p(walks), b, length, context, negatives, n, int(neg_seed) & 0xFFFFFFFF, _p(cdf),
                                                       _p(start), _p(rest), _p(pair_indptr), _p(win_indptr), _stream())
    _dw_check(rc, "glnn_deepwalk_pairs_from_walks")
    return start, rest.view(q, r), pair_indptr, win_indptr


def deepwalk_cdf_words(cdf, device):
    """The device form of a 32-bit CDF: `cdf` holds integers in [0, 2^32) (int64 tensor or numpy array); returned as an int32 tensor with
    the same 32 bits per entry, which the kernel reads as uint32.  A tensor that is already int32 on the device is taken as that form."""
    if torch.is_tensor(cdf) and cdf.dtype == torch.int32:
        return cdf.to(device).contiguous()
    cdf = torch.as_tensor(cdf).to(torch.int64).reshape(-1)
    if cdf.numel() and (int(cdf.min()) < 0 or int(cdf.max()) >= 2 ** 32):
        raise ValueError("deepwalk_cdf_words: entries must be in [0, 2^32)")
    return torch.where(cdf >= 2 ** 31, cdf - 2 ** 32, cdf).to(torch.int32).to(device).contiguous()


def deepwalk_empty_list(n_nodes, device):
    """An empty per-node list (all-zero indptr [N + 1], no entries) for deepwalk_apply: the side a table of the two-table update does not
    take part in."""
    return torch.zeros(int(n_nodes) + 1, dtype=torch.int64, device=device), _i32(0, device)


def deepwalk_score(z, start, rest, context, negatives, ctx=None):
    """glnn_deepwalk_score_f32 at frozen z [N, d]: g [Q * R] = dLoss/ds of every pair, gs [Q, d] = sum_t g z[rest] (the start-side gradient of
    window q), zs [Q, d] = z[start] (the snapshot the entry side reads), loss_parts [2, Q] = the windows' softplus sums over positives /
    negatives.  Returns (g, gs, zs, loss_parts).  ctx [N, d] (glnn_deepwalk_score_ctx_f32): the entries are read from this second table,
    s = <z[start], ctx[rest]> and gs = sum_t g ctx[rest]; ctx is z itself: the one-table bits."""
    _need_cuda(z, start, rest, ctx)
    _dw_table(z, "deepwalk_score z")
    if ctx is not None and tuple(_dw_table(ctx, "deepwalk_score ctx").shape) != tuple(z.shape):
        raise ValueError("deepwalk_score: ctx must have z's shape")
    if start.dtype != torch.int32 or rest.dtype != torch.int32 or rest.dim() != 2 or not rest.is_contiguous() or not start.is_contiguous() \
            or rest.shape[0] != start.numel():
        raise ValueError("deepwalk_score: start [Q] and rest [Q, R] must be contiguous int32 (ops.deepwalk_pairs)")
    n, d = z.shape
    q, r = rest.shape
    if r != (1 + int(negatives)) * (int(context) - 1):
        raise ValueError(f"deepwalk_score: rest has {r} entries per window, (1 + negatives) * (context - 1) = {(1 + int(negatives)) * (int(context) - 1)}")
    g = torch.empty(max(q * r, 1), dtype=torch.float32, device=z.device)[:q * r]
    gs = torch.empty((q, d), dtype=torch.float32, device=z.device)
    zs = torch.empty((q, d), dtype=torch.float32, device=z.device)
    loss_parts = torch.empty((2, q), dtype=torch.float32, device=z.device)
    with _Timed("deepwalk_score", d=d, n_windows=q, row=r):
        if ctx is None:
            rc = _lib.lib().glnn_deepwalk_score_f32(_p(z), n, d, _p(start), _p(rest), q, int(context), int(negatives), _p(g), _p(gs), _p(zs),
                                                    _p(loss_parts), _stream())
        else:
            rc = _lib.lib().glnn_deepwalk_score_ctx_f32(_p(z), _p(ctx), n, d, _p(start), _p(rest), q, int(context), int(negatives), _p(g),
                                                        _p(gs), _p(zs), _p(loss_parts), _stream())
    _dw_check(rc, "glnn_deepwalk_score_f32" if ctx is None else "glnn_deepwalk_score_ctx_f32")
    return g, gs, zs, loss_parts


def deepwalk_apply(z, m, v, tw, tp, g, gs, zs, loss_parts, context, negatives, lr, betas, eps, step, loss_out=None):
    """glnn_deepwalk_apply_f32: the lazy-Adam update of the rows of z, m, v [N, d] (in place) that are the start or an entry of some pair.
    tw = (t_indptr, t_indices) of csr_transpose over the start list, tp = (t_indptr, t_eids) of csr_transpose_eids over the pair list.
    dz[n] = sum of gs over n's windows + sum of g[e] * zs[e // R] over n's pair-list positions; rows in no pair are not written.
    `step` is the global step count (>= 1).  Returns the loss as a device scalar (loss_out, a float32 tensor of one element, if given)."""
    _need_cuda(z, m, v, g, gs, zs, loss_parts, loss_out, *tw, *tp)
    n, d = _dw_table(z, "deepwalk_apply z").shape
    for name, t in (("m", m), ("v", v)):
        if tuple(_dw_table(t, f"deepwalk_apply {name}").shape) != (n, d):
            raise ValueError(f"deepwalk_apply: {name} must have z's shape")
    q = gs.shape[0]
    if tuple(_dw_table(zs, "deepwalk_apply zs").shape) != (q, d) or _dw_table(gs, "deepwalk_apply gs").shape[1] != d \
            or loss_parts.numel() != 2 * q or not loss_parts.is_contiguous() or loss_parts.dtype != torch.float32 \
            or g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("deepwalk_apply: g, gs, zs and loss_parts must be those of ops.deepwalk_score")
    r = (1 + int(negatives)) * (int(context) - 1)
    (tw_indptr, tw_indices), (tp_indptr, tp_eids) = tw, tp
    if tw_indptr.dtype != torch.int64 or tp_indptr.dtype != torch.int64 or tw_indptr.numel() != n + 1 or tp_indptr.numel() != n + 1 \
            or tw_indices.dtype != torch.int32 or tp_eids.dtype != torch.int32 or tw_indices.numel() not in (0, q) \
            or tp_eids.numel() not in (0, q * r) or g.numel() != q * r:
        raise ValueError("deepwalk_apply: tw / tp must be the transposes of the start list (Q entries) and of the pair list (Q * R entries) over N "
                         "nodes, or ops.deepwalk_empty_list for the side a table takes no part in")
    if loss_out is None:
        loss_out = torch.empty((), dtype=torch.float32, device=z.device)
    elif loss_out.dtype != torch.float32 or loss_out.numel() != 1:
        raise ValueError("deepwalk_apply: loss_out must be a float32 tensor of one element")
    # (an empty list has no storage of its own, and the C entry takes no NULL: its all-zero indptr stands in, every row being empty, never read)
    tw_entries = tw_indices if tw_indices.numel() else tw_indptr
    tp_entries = tp_eids if tp_eids.numel() else tp_indptr
    with _Timed("deepwalk_apply", d=d, n_nodes=n, n_windows=q, row=r):
        rc = _lib.lib().glnn_deepwalk_apply_f32(_p(tw_indptr), _p(tw_entries), _p(tp_indptr), _p(tp_entries), n, d, q, int(context),
                                                int(negatives), _p(g), _p(gs), _p(zs), _p(z), _p(m), _p(v), float(lr), float(betas[0]),
                                                float(betas[1]), float(eps), int(step), _p(loss_parts), _p(loss_out), _stream())
    _dw_check(rc, "glnn_deepwalk_apply_f32")
    return loss_out


def edge_drop_mask(nnz, t, edge_drop, seed, device):
    """glnn_edge_drop_mask_u8: uint8 [nnz], 1 = edge kept in iteration t (1-based) -- the mask the propagation kernels evaluate."""
    mask = torch.empty(max(int(nnz), 1), dtype=torch.uint8, device=device)[:int(nnz)]
    rc = _lib.lib().glnn_edge_drop_mask_u8(int(nnz), int(t), float(edge_drop), int(seed) & 0xFFFFFFFF, _p(mask) if nnz else None, _stream())
    _lib.check(rc, "glnn_edge_drop_mask_u8")
    return mask


# --------------------------------------------------------------------------------------------- GAT attention (csrc/gat.hip)
_UNIT = {}


def _unit_affine(k, device, sign):
    """(scale, shift) = (+-1, 0) vectors of length k: the identity tail that lets glnn_gemm_f32's operand transform apply a dropout mask."""
    key = (str(device), sign)
    if key not in _UNIT or _UNIT[key][0].numel() < k:
        _UNIT[key] = (torch.full((max(k, 1024),), float(sign), dtype=torch.float32, device=device),
                      torch.zeros(max(k, 1024), dtype=torch.float32, device=device))
    return _UNIT[key]


def gat_project(x, w, drop_p=0.0, drop_seed=0, signed=True):
    """(z, z2) with feat_drop(x) @ w^T = z - z2 (z2 None: z alone), the dropout mask keep(row, col) of glnn_dropout_mask_u8 applied in the
    GEMM's operand load: no dropped copy of x exists.  The operand transform is drop(max(x * scale + shift, 0)), so a non-negative x
    (signed=False: a hidden layer's post-ReLU output, bag-of-words features) takes one product with scale 1, and a signed x two, with
    scales +1 and -1 -- max(x, 0) - max(-x, 0) = x under the SAME mask.  gat_scores subtracts z2 while it reads z."""
    x = as_feat(x)
    if drop_p <= 0:
        return gemm(x, w), None
    k = x.shape[1]
    one, zero = _unit_affine(k, x.device, 1)
    z = gemm(x, w, a_scale=one, a_shift=zero, drop_p=drop_p, drop_seed=drop_seed)
    if not signed:
        return z, None
    neg, _ = _unit_affine(k, x.device, -1)
    return z, gemm(x, w, a_scale=neg, a_shift=zero, drop_p=drop_p, drop_seed=drop_seed)


def gat_project_wgrad(dz, x, drop_p=0.0, drop_seed=0, signed=True, out=None):
    """dW = dz^T feat_drop(x) with the mask in glnn_gemm_tn_f32's operand load (gat_project's counterpart)."""
    x = as_feat(x)
    if drop_p <= 0:
        return gemm_tn(dz, x, out=out)
    k = x.shape[1]
    one, zero = _unit_affine(k, x.device, 1)
    dw = gemm_tn(dz, x, b_scale=one, b_shift=zero, drop_p=drop_p, drop_seed=drop_seed, out=out)
    if signed:
        neg, _ = _unit_affine(k, x.device, -1)
        dw.sub_(gemm_tn(dz, x, b_scale=neg, b_shift=zero, drop_p=drop_p, drop_seed=drop_seed))
    return dw


def gat_scores(z, attn_l, attn_r, heads, out_feats, z2=None):
    """glnn_gat_scores_f32: (el, er) [n, heads] from one read of z [n, heads * out_feats]; z2: z -= z2 in place first."""
    _need_cuda(z, z2, attn_l, attn_r)
    _mat(z, "gat_scores z")
    n = z.shape[0]
    hf = heads * out_feats
    if z.shape[1] != hf or attn_l.numel() != hf or attn_r.numel() != hf or not attn_l.is_contiguous() or not attn_r.is_contiguous():
        raise ValueError("gat_scores: z must be [n, heads * out_feats] and attn_l / attn_r contiguous [1, heads, out_feats]")
    if z2 is not None:
        _mat(z2, "gat_scores z2")
    el = torch.empty((n, heads), dtype=torch.float32, device=z.device)
    er = torch.empty((n, heads), dtype=torch.float32, device=z.device)
    rc = _lib.lib().glnn_gat_scores_f32(_p(z), _ld(z), _p(z2), 0 if z2 is None else _ld(z2), n, heads, out_feats, _p(attn_l), _p(attn_r),
                                        _p(el), _p(er), _stream())
    _lib.check(rc, "glnn_gat_scores_f32")
    return el, er


def _attn_out(name, n, heads, out_feats, device, out, lse, want_lse):
    """(out, lse) of an attention forward `name`: allocated where None (lse only when wanted), checked either way."""
    if out is None:
        out = feat_empty(n, heads * out_feats, device)
    _mat(out, f"{name} out")
    if lse is None and want_lse:
        lse = torch.empty((n, heads), dtype=torch.float32, device=device)
    if lse is not None and (lse.shape != (n, heads) or not lse.is_contiguous() or lse.dtype != torch.float32 or not lse.is_cuda):
        raise ValueError(f"{name}: lse must be a contiguous fp32 [n, heads] tensor on the GPU")
    return out, lse


def _attn_bwd_bufs(name, graph, n, heads, out_feats, device, dz, dattn):
    """The common part of an attention backward `name`: (the C call's leading arguments -- in-CSR, cached transpose with edge ids, n, nnz --,
    nnz, the [E, heads] score-gradient scratch, the row buffers dz {name: tensor or None}, the dattn vectors), allocated where None."""
    hf = heads * out_feats
    tg, t_eids = graph.transposed_eids()
    nnz = graph.num_edges()
    csr = (_p(graph.indptr), _p(graph.indices), _p(tg.indptr), _p(tg.indices), _p(t_eids), n, int(nnz))
    ds = torch.empty((max(nnz, 1), heads), dtype=torch.float32, device=device)
    dz = {k: feat_empty(n, hf, device) if t is None else t for k, t in dz.items()}
    _need_cuda(*dz.values())
    for k, t in dz.items():
        _mat(t, f"{name} {k}")
    dattn = [torch.empty(hf, dtype=torch.float32, device=device) if t is None else t for t in dattn]
    return csr, nnz, ds, list(dz.values()), dattn


def _attn_call(name, heads, out_feats, n, nnz, attn_drop, *args):
    """glnn_<name>_f32(*args, stream) under the optional launch timing, its status checked."""
    entry = f"glnn_{name}_f32"
    with _Timed(name, d=heads * out_feats, n_dst=n, nnz=int(nnz), attn_drop=float(attn_drop)):
        rc = getattr(_lib.lib(), entry)(*args, _stream())
    _lib.check(rc, entry)


def gat_attn_fwd(indptr, indices, nnz, z, el, er, heads, out_feats, negative_slope=0.2, attn_drop=0.0, seed=0, relu=False, want_lse=False,
                 out=None):
    """glnn_gat_attn_fwd_f32: (out [n, heads * out_feats], lse [n, heads] or None) -- edge softmax + weighted aggregation of z."""
    z = as_feat(z)
    n = z.shape[0]
    _csr_check("gat_attn_fwd", indptr, indices, n, z)
    _need_cuda(el, er, out)
    out, lse = _attn_out("gat_attn_fwd", n, heads, out_feats, z.device, out, None, want_lse)
    _attn_call("gat_attn_fwd", heads, out_feats, n, nnz, attn_drop, _p(indptr), _p(indices), n, int(nnz), _p(z), _ld(z), heads, out_feats,
               _p(_vec(el.view(-1), n * heads, "el")), _p(_vec(er.view(-1), n * heads, "er")), float(negative_slope), float(attn_drop),
               int(seed) & 0xFFFFFFFF, 1 if relu else 0, _p(out), _ld(out), _p(lse))
    return out, lse


def gat_attn_bwd(graph, z, el, er, lse, attn_l, attn_r, g, y, heads, out_feats, negative_slope=0.2, attn_drop=0.0, seed=0,
                 dattn_l=None, dattn_r=None):
    """glnn_gat_attn_bwd_f32 over `graph` (CSRGraph: its in-CSR and its cached transpose with edge ids): (dz, dattn_l, dattn_r).
    g = dL/d out behind the activation mask, y = the forward's stored output (checked, not read: the kernel forms <g_i, out_i> from the row's
    own edges).  The [E, heads] score-gradient scratch lives for the call."""
    z, g, y = as_feat(z), as_feat(g), as_feat(y)
    n = z.shape[0]
    _csr_check("gat_attn_bwd", graph.indptr, graph.indices, n, z)
    _need_cuda(el, er, lse, attn_l, attn_r, g, y)
    dev = z.device
    csr, nnz, ds, (dz,), (dattn_l, dattn_r) = _attn_bwd_bufs("gat_attn_bwd", graph, n, heads, out_feats, dev, {"dz": None}, (dattn_l, dattn_r))
    der = torch.empty((n, heads), dtype=torch.float32, device=dev)
    dl = torch.empty((n, heads), dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.lib().glnn_gat_attn_bwd_workspace_floats(n, heads, out_feats)), dtype=torch.float32, device=dev)
    _attn_call("gat_attn_bwd", heads, out_feats, n, nnz, attn_drop, *csr, _p(z), _ld(z), heads, out_feats, _p(el), _p(er), _p(lse), _p(attn_l),
               _p(attn_r), _p(g), _ld(g), _p(y), _ld(y), float(negative_slope), float(attn_drop), int(seed) & 0xFFFFFFFF, _p(ds), _p(der),
               _p(dl), _p(dz), _ld(dz), _p(dattn_l), _p(dattn_r), _p(ws), ws.numel())
    return dz, dattn_l, dattn_r


def gat_attn_mask(nnz, heads, attn_drop, seed, device):
    """glnn_gat_attn_mask_u8: uint8 [nnz, heads], 1 = head h of edge e kept -- the mask the attention kernels evaluate."""
    mask = torch.empty((max(int(nnz), 1), heads), dtype=torch.uint8, device=device)[:int(nnz)]
    rc = _lib.lib().glnn_gat_attn_mask_u8(int(nnz), heads, float(attn_drop), int(seed) & 0xFFFFFFFF, _p(mask) if nnz else None, _stream())
    _lib.check(rc, "glnn_gat_attn_mask_u8")
    return mask


# --------------------------------------------------------------------------------------------- GATv2 attention (csrc/gatv2.hip)
def _gatv2_check(zl, zr, attn, heads, out_feats, name):
    hf = heads * out_feats
    if zl.shape[1] != hf or zr.shape != zl.shape or attn.numel() != hf or not attn.is_contiguous() or attn.dtype != torch.float32:
        raise ValueError(f"{name}: zl and zr must be [n, heads * out_feats] and attn contiguous fp32 [1, heads, out_feats]")


def gatv2_attn_fwd(indptr, indices, nnz, zl, zr, attn, heads, out_feats, negative_slope=0.2, attn_drop=0.0, seed=0, relu=False,
                   want_lse=False, out=None, lse=None):
    """glnn_gatv2_attn_fwd_f32: (out [n, heads * out_feats], lse [n, heads] or None) -- the GATv2 edge softmax and the weighted
    aggregation of zl from ONE gather per edge (docs/GATV2_SEMANTICS.md).  lse: a buffer to take the row log-sum-exps (implies want_lse)."""
    zl, zr = as_feat(zl), as_feat(zr)
    n = zl.shape[0]
    _csr_check("gatv2_attn_fwd", indptr, indices, n, zl)
    _need_cuda(zr, attn, out)
    _mat(zr, "gatv2_attn_fwd zr")
    _gatv2_check(zl, zr, attn, heads, out_feats, "gatv2_attn_fwd")
    out, lse = _attn_out("gatv2_attn_fwd", n, heads, out_feats, zl.device, out, lse, want_lse)
    _attn_call("gatv2_attn_fwd", heads, out_feats, n, nnz, attn_drop, _p(indptr), _p(indices), n, int(nnz), _p(zl), _ld(zl), _p(zr), _ld(zr),
               heads, out_feats, _p(attn), float(negative_slope), float(attn_drop), int(seed) & 0xFFFFFFFF, 1 if relu else 0, _p(out),
               _ld(out), _p(lse))
    return out, lse


def gatv2_attn_bwd(graph, zl, zr, lse, attn, g, heads, out_feats, negative_slope=0.2, attn_drop=0.0, seed=0, dattn=None, dzl=None,
                   dzr=None):
    """glnn_gatv2_attn_bwd_f32 over `graph` (CSRGraph: its in-CSR and its cached transpose with edge ids): (dzl, dzr, dattn).
    g = dL/d out behind the activation mask.  The [E, heads] score-gradient scratch and the dattn partials live for the call."""
    zl, zr, g = as_feat(zl), as_feat(zr), as_feat(g)
    n = zl.shape[0]
    _csr_check("gatv2_attn_bwd", graph.indptr, graph.indices, n, zl)
    _need_cuda(zr, lse, attn, g, dattn)
    _mat(zr, "gatv2_attn_bwd zr")
    _mat(g, "gatv2_attn_bwd g")
    _gatv2_check(zl, zr, attn, heads, out_feats, "gatv2_attn_bwd")
    hf = heads * out_feats
    if g.shape != zl.shape or lse.shape != (n, heads) or not lse.is_contiguous() or lse.dtype != torch.float32:
        raise ValueError("gatv2_attn_bwd: g must be [n, heads * out_feats] and lse contiguous fp32 [n, heads]")
    dev = zl.device
    csr, nnz, ds, (dzl, dzr), (dattn,) = _attn_bwd_bufs("gatv2_attn_bwd", graph, n, heads, out_feats, dev, {"dzl": dzl, "dzr": dzr}, (dattn,))
    _vec(dattn, hf, "dattn")
    ws = torch.empty(max(int(_lib.lib().glnn_gatv2_attn_bwd_workspace_floats(n, heads, out_feats)), 1), dtype=torch.float32, device=dev)
    _attn_call("gatv2_attn_bwd", heads, out_feats, n, nnz, attn_drop, *csr, _p(zl), _ld(zl), _p(zr), _ld(zr), heads, out_feats, _p(lse),
               _p(attn), _p(g), _ld(g), float(negative_slope), float(attn_drop), int(seed) & 0xFFFFFFFF, _p(ds), _p(dzl), _ld(dzl), _p(dzr),
               _ld(dzr), _p(dattn), _p(ws), ws.numel())
    return dzl, dzr, dattn


# --------------------------------------------------------------------------------------------- graph-transformer attention (csrc/gt.hip)
def _gt_check(name, n, hf, **rows):
    """q / k / v / skip / g of a graph-transformer call: [n, heads * out_feats] fp32 rows on the GPU (column slabs of one stacked
    projection are fine: each carries its own leading dimension)."""
    _need_cuda(*rows.values())
    for key, t in rows.items():
        _mat(t, f"{name} {key}")
        if t.shape != (n, hf):
            raise ValueError(f"{name}: {key} must be [n, heads * out_feats] = [{n}, {hf}] (got {tuple(t.shape)})")


def gt_attn_fwd(indptr, indices, nnz, q, k, v, skip, heads, out_feats, attn_drop=0.0, seed=0, relu=False, want_lse=False, out=None,
                lse=None):
    """glnn_gt_attn_fwd_f32: (out [n, heads * out_feats], lse [n, heads] or None) -- the scaled dot-product edge softmax, the weighted
    aggregation of v and the skip row (docs/GT_SEMANTICS.md).  lse: a buffer to take the row log-sum-exps (implies want_lse)."""
    q, k, v, skip = as_feat(q), as_feat(k), as_feat(v), as_feat(skip)
    n = q.shape[0]
    _csr_check("gt_attn_fwd", indptr, indices, n, q)
    _gt_check("gt_attn_fwd", n, heads * out_feats, q=q, k=k, v=v, skip=skip)
    _need_cuda(out)
    out, lse = _attn_out("gt_attn_fwd", n, heads, out_feats, q.device, out, lse, want_lse)
    _attn_call("gt_attn_fwd", heads, out_feats, n, nnz, attn_drop, _p(indptr), _p(indices), n, int(nnz), _p(q), _ld(q), _p(k), _ld(k),
               _p(v), _ld(v), _p(skip), _ld(skip), heads, out_feats, float(attn_drop), int(seed) & 0xFFFFFFFF, 1 if relu else 0, _p(out),
               _ld(out), _p(lse))
    return out, lse


def gt_attn_bwd(graph, q, k, v, lse, g, heads, out_feats, attn_drop=0.0, seed=0, dq=None, dk=None, dv=None):
    """glnn_gt_attn_bwd_f32 over `graph` (CSRGraph: its in-CSR and its cached transpose with edge ids): (dq, dk, dv); the gradient of the
    skip row is g itself.  g = dL/d out behind the activation mask.  The two [E, heads] scratches (t and a w) live for the call."""
    q, k, v, g = as_feat(q), as_feat(k), as_feat(v), as_feat(g)
    n = q.shape[0]
    _csr_check("gt_attn_bwd", graph.indptr, graph.indices, n, q)
    _gt_check("gt_attn_bwd", n, heads * out_feats, q=q, k=k, v=v, g=g)
    _need_cuda(lse)
    if lse.shape != (n, heads) or not lse.is_contiguous() or lse.dtype != torch.float32:
        raise ValueError("gt_attn_bwd: lse must be contiguous fp32 [n, heads]")
    dev = q.device
    csr, nnz, ts, (dq, dk, dv), _ = _attn_bwd_bufs("gt_attn_bwd", graph, n, heads, out_feats, dev, {"dq": dq, "dk": dk, "dv": dv}, ())
    ws = torch.empty(max(int(_lib.lib().glnn_gt_attn_bwd_workspace_floats(int(nnz), heads)), 1), dtype=torch.float32, device=dev)
    _attn_call("gt_attn_bwd", heads, out_feats, n, nnz, attn_drop, *csr, _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), heads, out_feats,
               _p(lse), _p(g), _ld(g), float(attn_drop), int(seed) & 0xFFFFFFFF, _p(ts), _p(dq), _ld(dq), _p(dk), _ld(dk), _p(dv), _ld(dv),
               _p(ws), ws.numel())
    return dq, dk, dv


_NONNEG = []          # [(weakref to the tensor, key, answer)]: one entry


def is_nonneg(x):
    """Whether every element of x is >= 0, remembered while the very same unmodified tensor is asked about again (as_feat's identity
    rule): the reference hands the same `feats` to every epoch, so a GAT teacher looks at its input once."""
    import weakref
    key = _pad_key(x)
    if key is not None and _NONNEG and _NONNEG[0][0]() is x and _NONNEG[0][1] == key:
        return _NONNEG[0][2]
    ans = bool((x.detach().min() >= 0).item()) if x.numel() else True
    _NONNEG[:] = [(weakref.ref(x), key, ans)]
    return ans


# ---------------------------------------------------------------------------------------------
# bf16 serving GEMM of the MLP student (csrc/gemm_bf16.hip)
def round64(d):
    return (d + 63) // 64 * 64


def pack_weight_bf16(w):
    """W [n, k] fp32 (torch Linear layout) -> the bf16 [n, round64(k)] operand of gemm_bf16, zeros behind column k (glnn_cast_f32_bf16
    into a zeroed buffer).  Returns the [n, k] view."""
    _need_cuda(w)
    _mat(w, "pack_weight_bf16 w")
    n, k = w.shape
    buf = torch.zeros((n, round64(k)), dtype=torch.bfloat16, device=w.device)
    return to_bf16(w.detach(), out=buf[:, :k])


def _bf16_weight(w, k, name):
    _bf16_mat(w, name)
    if w.shape[1] != k or _ld(w) % 64 or w.data_ptr() % 16:
        raise ValueError(f"{name}: expected a bf16 [n, {k}] view of rows padded to a multiple of 64 (ops.pack_weight_bf16)")
    return w


def gemm_bf16(a, w, ep_scale=None, ep_shift=None, relu=False, out=None, out_dtype=None, log_softmax=False):
    """glnn_gemm_bf16: out = epi(A @ W^T) on the bf16 MFMA with fp32 accumulation.  a: [m, k] fp32 (rounded to bf16 while it is staged) or
    bf16; w: bf16 [n, k] from pack_weight_bf16; out: `out`'s dtype, else out_dtype (default fp32).  log_softmax (n <= 64, fp32 out):
    the rows' log-probabilities instead of the logits."""
    _need_cuda(a, w, ep_scale, ep_shift, out)
    if a.dtype == torch.bfloat16:
        a = as_bf16_feat(a)
    else:
        _mat(a, "gemm_bf16 a")
    m, k = a.shape
    n = w.shape[0]
    _bf16_weight(w, k, "gemm_bf16 w")
    out = _out_like(out, out_dtype, torch.float32, m, n, a.device, "gemm_bf16 out")
    with _Timed("gemm_bf16", m=m, k=k, n=n):
        rc = _lib.lib().glnn_gemm_bf16(_p(a), _ld(a), _dtype_code(a), m, k, _p(w), _ld(w), n, _p(_vec(ep_scale, n, "ep_scale")),
                                       _p(_vec(ep_shift, n, "ep_shift")), 1 if relu else 0, _p(out), _ld(out), _dtype_code(out),
                                       1 if log_softmax else 0, _stream())
    _lib.check(rc, "glnn_gemm_bf16")
    return out[:m] if out.shape[0] != m else out


def mlp_fused_bf16_tile_rows(desc):
    """glnn_mlp_fused_bf16_tile_rows: (rows per workgroup of the one-launch form of the chain `desc`, a _lib.MlpServeDesc; "") or
    (0, the library's reason for not taking it)."""
    h = _lib.lib()
    t = h.glnn_mlp_fused_bf16_tile_rows(ctypes.byref(desc))
    return (t, "") if t > 0 else (0, h.glnn_last_error().decode(errors="replace"))


def mlp_forward_fused_bf16(desc, x, out, rows=None, log_softmax=False):
    """glnn_mlp_forward_fused_bf16: the chain `desc` (a _lib.MlpServeDesc) over x [n_x, dims[0]] (fp32, or a bf16 ops.bf16_empty view) as
    ONE launch into fp32 out [m, C]: logits, or log-probabilities (log_softmax, C <= 64).  rows None: m = n_x and batch row b is x[b];
    otherwise a contiguous int64 device vector of m row ids into x (the kernel computes an id outside [0, n_x) from an all-zero row).
    A chain the one-launch form does not take raises GlnnError (status -2); ask mlp_fused_bf16_tile_rows first."""
    _need_cuda(x, out, rows)
    x = as_bf16_feat(x) if x.dtype == torch.bfloat16 else _mat(x, "mlp_forward_fused_bf16 x")
    n_x = x.shape[0]
    m = n_x
    if rows is not None:
        if rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
            raise ValueError("mlp_forward_fused_bf16: rows must be a contiguous int64 vector")
        m = rows.numel()
    _mat(out, "mlp_forward_fused_bf16 out")
    if out.shape[0] != m or out.shape[1] != desc.dims[desc.num_layers]:
        raise ValueError(f"mlp_forward_fused_bf16: out must be float32 [{m}, {desc.dims[desc.num_layers]}]")
    with _Timed("mlp_forward_fused_bf16", m=m, layers=desc.num_layers):
        rc = _lib.lib().glnn_mlp_forward_fused_bf16(ctypes.byref(desc), _p(x), _ld(x), _dtype_code(x), _p(rows), n_x, m, _p(out), _ld(out),
                                                    1 if log_softmax else 0, _stream())
    _lib.check(rc, "glnn_mlp_forward_fused_bf16")
    return out


# ---------------------------------------------------------------------------------------------
# serving a position-feature student by node id (csrc/position_serve.hip)
def position_rows(ids, x, z, slot, g=None, out=None, out_dtype=None):
    """glnn_position_rows (docs/POSITION_SEMANTICS.md, "Serving by node id"): out[b] = [x[ids[b]] | pos(ids[b])] in one launch.
    ids: contiguous int64 device vector of node ids (the CALLER vouches for their range); x: [N, F] fp32 or bf16 features; z: [R, D] fp32
    position table; slot: int32 [N], node -> row of z or -1.  pos(v) = z[slot[v]] for an embedded node, else the mean of z[slot[u]] over the
    embedded stored entries u of row v of the in-edge CSR of `g` (zeros without one).  g None: no id is unseen (a row that is gets zeros).
    out: `out` (at least len(ids) rows of F + D columns; its dtype decides), else a fresh matrix of out_dtype (default: x's dtype); fp32
    rows are padded to a multiple of 4 columns, bf16 rows to 8, the padding written as 0.  bf16 features with an fp32 output are refused."""
    _need_cuda(ids, x, z, slot, out)
    if ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("position_rows: ids must be a contiguous int64 vector")
    if x.dtype == torch.bfloat16:
        x = as_bf16_feat(x)
    else:
        _mat(x, "position_rows x")
    _dw_table(z, "position_rows z")
    n, f = x.shape
    d = z.shape[1]
    if slot.dtype != torch.int32 or slot.dim() != 1 or not slot.is_contiguous() or slot.numel() != n:
        raise ValueError(f"position_rows: slot must be a contiguous int32 vector with one entry per row of x ({n})")
    indptr = indices = None
    if g is not None:
        indptr, indices = g.indptr, g.indices
        _need_cuda(indptr, indices)
        _check_csr(indptr, indices, "position_rows")
        if indptr.numel() != n + 1:
            raise ValueError(f"position_rows: the graph has {indptr.numel() - 1} rows, x {n}")
    m = ids.numel()
    out = _out_like(out, out_dtype, x.dtype, m, f + d, x.device, "position_rows out")
    with _Timed("position_rows", m=m, f=f, d=d):
        rc = _lib.lib().glnn_position_rows(_p(ids), m, _p(x), _ld(x), _dtype_code(x), f, _p(z), _ld(z), d, z.shape[0], _p(slot), n,
                                           _p(indptr), _p(indices), _p(out), _ld(out), _dtype_code(out), _stream())
    _lib.check(rc, "glnn_position_rows")
    return out[:m] if out.shape[0] != m else out
