/*
 * glnn_hip.h -- C ABI of libglnn_hip.so, the MI355X (gfx950) implementation of the GLNN hot path:
 * teacher neighbour aggregation + dense projections, and the MLP student distillation step.
 *
 * The reference (snap-research/graphless-neural-networks) has NO native/FFI layer: it is pure
 * Python whose graph arithmetic is delegated to dgl==0.6.1 and whose dense arithmetic is
 * torch==1.7.0.  Each entry point below therefore cites the reference *call site* (file:line under
 * /root/reference) whose arithmetic it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer would add at that call site.
 *
 * Conventions (all entry points):
 *   - plain pointers + explicit sizes and leading dimensions (in ELEMENTS), no torch types;
 *   - every data pointer is a DEVICE pointer (HBM) unless the parameter says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only ENQUEUE
 *     work, never synchronise, never allocate or free caller memory;
 *   - return value: 0 = GLNN_OK, negative = glnn_status; glnn_last_error() gives a thread-local
 *     message for the last failing call on this thread;
 *   - fp32 values, int32 column indices, int64 row pointers; row-major matrices;
 *   - feature matrices must have a leading dimension that is a multiple of 4 floats and a
 *     16-byte aligned base (the kernels move float4); columns [d, ld) are padding: read but
 *     never trusted, and written as 0 by kernels that own an output.
 */
#ifndef GLNN_HIP_H
#define GLNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLNN_API __attribute__((visibility("default")))

typedef enum {
  GLNN_OK = 0,
  GLNN_ERR_INVALID_ARG = -1,   /* null pointer, bad size, bad alignment / leading dimension */
  GLNN_ERR_UNSUPPORTED = -2,   /* shape or mode outside what the kernels implement */
  GLNN_ERR_HIP = -3,           /* a HIP runtime call or launch failed */
  GLNN_ERR_NO_DEVICE = -4      /* no gfx950 device visible */
} glnn_status;

GLNN_API int glnn_abi_version(void);               /* bumped on any signature change */
GLNN_API const char* glnn_last_error(void);        /* thread-local, never NULL */
GLNN_API int glnn_device_info(int* cu_count, int* xcd_count, char* arch_buf, int arch_buf_len);
/* sizeof of the descriptor structs below as THIS build sees them (0 = glnn_mlp_step_desc, 1 = glnn_sage_step_desc,
 * 2 = glnn_sage_layer, 3 = glnn_adam_desc, 4 = glnn_hub_plan, 5 = glnn_chunk_signals, 6 = glnn_sage_ln_desc, 7 = glnn_mlp_serve_desc, 8 = glnn_sage_mean_desc; -1 otherwise): lets a binding in another language check its mirror of the layout at load time. */
GLNN_API int64_t glnn_struct_bytes(int which);
/* The library reads its GLNN_* environment switches (csrc/glnn_common.h, glnn::Options: choices between supported, equal-result
 * forms of a launch sequence, for tests and A/B timing) ONCE, at the first call.  This re-reads them; not for concurrent use. */
GLNN_API void glnn_reload_options(void);

/* ------------------------------------------------------------------------------------------
 * K1/K2  CSR neighbour aggregation (SpMM with an implicit all-ones adjacency, multi-edges kept).
 * CSR is over DESTINATION rows: row v lists the sources u of its in-edges u->v.
 *
 * mode GLNN_AGG_SUM       out[v,:] = row_scale[v] * sum_{u->v} col_scale[u] * x[u,:]
 *        replaces g.update_all(fn.copy_u("h","m"), fn.sum("m","h")), reference utils.py:185
 *        (feature_prop) and the aggregation inside dgl GraphConv(norm="both"), reference
 *        models.py:193 (ctor :170-187): col_scale = out_deg.clamp(1)^-1/2,
 *        row_scale = in_deg.clamp(1)^-1/2.  Either scale may be NULL (= 1).
 * mode GLNN_AGG_SAGE_GCN  out[v,:] = (sum_{u->v} x[u,:] + x_self[v,:]) / (in_deg(v) + 1)
 *        replaces the "gcn" aggregator of dgl SAGEConv, reference models.py:112,138
 *        (ctor :84-99); x_self is h_dst = the first n_dst rows of the block's source features
 *        (models.py:109,137), normally x_self == x.  self_rows (optional, SAGE_GCN only): the self row of
 *        destination v is x_self[self_rows[v]] -- with `indices` holding GLOBAL node ids and x = x_self = the whole
 *        feature matrix this folds `batch_feats = feats[input_nodes]` (train_and_eval.py:42) into the first layer's
 *        gather: the outermost block of a training batch is aggregated straight out of `feats`.
 * Epilogue (both modes), per output element, in this order, each optional:
 *        y = y * ep_scale[j] + ep_shift[j] ;  y = max(y, 0) if relu
 *   (bias, eval-mode BatchNorm and ReLU of models.py:139-143 when the dense projection was
 *    applied BEFORE aggregation; NULL/0 otherwise).
 * n_src bounds the column indices (only used for argument checking).  Rows wider than 256 floats
 * are processed in column tiles of 256 (one launch per tile).
 * ------------------------------------------------------------------------------------------ */
#define GLNN_AGG_SUM 0
#define GLNN_AGG_SAGE_GCN 1

GLNN_API int glnn_spmm_csr_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                               int64_t n_src, const float* x, int64_t ldx, int d, int mode,
                               const float* row_scale, const float* col_scale,
                               const float* x_self, int64_t ld_self, const int64_t* self_rows,
                               const float* ep_scale, const float* ep_shift, int relu, float* out,
                               int64_t ldo, void* stream);

/* K1F  Fused SAGE-"gcn" layer for aggregate-first layers (d_in, d_out <= 256):
 *   out[v,:] = epi( ((sum_{u->v} x[u,:] + x_self[v,:]) / (in_deg(v)+1)) @ W^T ),  epi = *ep_scale +ep_shift, ReLU
 * = SAGEConv(in,out,"gcn") + bias + eval BatchNorm + ReLU of reference models.py:138-143 in ONE launch; the
 * aggregated rows stay in LDS and feed the fp32 MFMA directly.  W must be pre-packed into MFMA fragment
 * order with glnn_pack_weight_f32 (glnn_packed_weight_floats(d_out, d_in) floats, 16-byte aligned). */
GLNN_API int64_t glnn_packed_weight_floats(int d_out, int d_in);
GLNN_API int glnn_pack_weight_f32(const float* w, int64_t ldw, int d_out, int d_in, float* w_packed,
                                  void* stream);
/* Optional chained projection (w2_packed != NULL: W2 [d_out2, d_out] packed like W): additionally
 *   out2[v,:] = out[v,:] @ W2^T   (no epilogue)
 * i.e. the dense half of the NEXT layer when that layer projects first (in > out, models.py:138 on the last layer of the
 * products / arxiv teachers): the hidden row goes from the MFMA accumulators through LDS into a second MFMA pass; with
 * out == NULL it never reaches HBM at all. */
GLNN_API int glnn_sage_fused_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                 int64_t n_src, const float* x, int64_t ldx, int d_in,
                                 const float* x_self, int64_t ld_self, const float* w_packed,
                                 int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                 float* out, int64_t ldo, const float* w2_packed, int d_out2,
                                 float* out2, int64_t ldo2, const int32_t* tile_order, void* stream);
/* tile_order (optional, ceil(n_dst / 32) entries: a permutation of the 32-row tile ids): workgroup i takes tile tile_order[i].  A caller
 * that sorts the tiles by their heaviest row (descending in-degree) starts the hub rows of a power-law graph first instead of wherever
 * their ids put them -- what matters for SHORT launches (a row shard's chunk: one 8 k-edge hub row is 100 us of a 0.7 ms launch). */

/* ABI 9: HUB ROWS split over workgroups.  A destination row of more than glnn_hub_row_threshold() in-edges is always summed in segments
 * of glnn_hub_segment_edges() edges, 1/8 of a segment per wave: a wave's share of the row is the sum over the segments (ascending) of its
 * piece of each, gathered into a fresh accumulator; the eight shares are folded like the wave partials of any long row.  The pieces are
 * gathered by the one workgroup that owns the row, or, given a plan, by one workgroup PER SEGMENT in a launch of its own in front of the
 * aggregation, whose partial sums the row's owner reads back.  Same bits either way; what changes is the tail of SHORT launches: a
 * 17 k-edge row of the products graph keeps one workgroup busy for ~0.5 ms at d = 256, most of a row shard's 0.7 ms chunk launch
 * (scripts/hub_tail_probe.py).  The plan is per (indptr, n_dst) launch range and caller-built (one pass over the degrees:
 * glnn_amd.ops.hub_plan):
 *   rows      ascending ids v (relative to `indptr`) of the rows with indptr[v+1] - indptr[v] > threshold; a hub row that is not listed
 *             is summed by its owner; a listed row must have exactly ceil(degree / segment_edges) segments
 *   seg_ptr   [n_hub + 1] running segment count (seg_ptr[0] = 0, seg_ptr[n_hub] = n_seg)
 *   slab      [slab_rows >= 8 n_seg][ld_slab >= d rounded up to 4] floats of scratch (row 8 s + w = wave w's piece of segment s), 16-byte
 *             aligned; overwritten by every call that is given the plan (one stream at a time)
 * Column-tiled launches (d > 256) ignore the plan.  The reference has no counterpart (dgl's SpMM is one launch, models.py:112,138). */
typedef struct glnn_hub_plan {
  const int64_t* rows;
  const int32_t* seg_ptr;
  int32_t n_hub, n_seg;
  float* slab;
  int64_t ld_slab, slab_rows;
} glnn_hub_plan;
GLNN_API int glnn_hub_row_threshold(void);
GLNN_API int glnn_hub_segment_edges(void);
GLNN_API int glnn_spmm_csr_plan_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                    int64_t n_src, const float* x, int64_t ldx, int d, int mode,
                                    const float* row_scale, const float* col_scale,
                                    const float* x_self, int64_t ld_self, const int64_t* self_rows,
                                    const float* ep_scale, const float* ep_shift, int relu, float* out,
                                    int64_t ldo, const glnn_hub_plan* plan, void* stream);
GLNN_API int glnn_sage_fused_plan_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                      int64_t n_src, const float* x, int64_t ldx, int d_in,
                                      const float* x_self, int64_t ld_self, const float* w_packed,
                                      int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                      float* out, int64_t ldo, const float* w2_packed, int d_out2,
                                      float* out2, int64_t ldo2, const int32_t* tile_order,
                                      const glnn_hub_plan* plan, void* stream);
/* The same launch around a KEPT aggregate.  A1 = (sum_{u->v} x[u] + x_self[v]) / (deg+1) depends on the graph and on x only: a caller whose
 * layer aggregates the same input call after call (the teacher's layer 1 over a dataset's features, once per evaluation) keeps it.
 * Exactly one of agg_out / agg_in is non-NULL; ld_agg is a multiple of 4 and >= d_in rounded up to 4; both are 16-byte aligned.
 *   agg_out  the launch of glnn_sage_fused_plan_f32, which also streams every normalised row to agg_out[v, 0:ld_agg) (columns at or beyond
 *            d_in are written as 0, up to d_in rounded up to 8 where ld_agg reaches that far); out / out2 are the bits of the plain launch
 *   agg_in   the gather is replaced by a copy of agg_in[v, 0:d_in rounded up to 4) into the tile; indptr, indices, x, x_self, tile_order
 *            and plan are not read (may be NULL).  The projection, epilogue and chained projection are the same code, so out / out2 are
 *            bit for bit what the agg_out launch with these weights stores.  Without a chained projection, with 36 <= d_in rounded up to 4
 *            <= 128, d_out >= 96 and n_dst >= 2048 the launch is the wave-walk GEMM reading w_packed (the same MFMA chain per output
 *            element: the same bits); GLNN_AGG_IN_ROWWALK=0 keeps the fused launch for every shape. */
GLNN_API int glnn_sage_fused_agg_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                     int64_t n_src, const float* x, int64_t ldx, int d_in,
                                     const float* x_self, int64_t ld_self, const float* w_packed,
                                     int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                     float* out, int64_t ldo, const float* w2_packed, int d_out2,
                                     float* out2, int64_t ldo2, const int32_t* tile_order,
                                     const glnn_hub_plan* plan, float* agg_out, const float* agg_in,
                                     int64_t ld_agg, void* stream);

/* ABI 12 (round 6): ONE fused launch over the CHUNKS of a row shard, with a completion signal per chunk.  A rank of the sharded forward
 * (no reference counterpart: the reference is single-device, train_teacher.py:162-165) produces its rows chunk by chunk so that each
 * chunk's rows can leave over the links while the next is computed; launched one by one the chunks pay a short launch's ramp and tail
 * each (two launches of a rank's layer 2 at N = 8: 2.55 ms, one launch over the same rows: see DESIGN.md section 6).  Here the chunks
 * are tile ranges of ONE launch:
 *   row_start  [n_chunks + 1] first row (relative to `indptr`) of every chunk, multiples of 32 (row_start[0] = 0); row_start[n_chunks]
 *              >= n_dst (a chunk may be short or empty: an EMPTY chunk is never signalled)
 *   self_row   row of `x_self` holding the self row of row_start[c] (the chunk's self rows are consecutive from there)
 *   out_row    row of `out` / `out2` that receives row_start[c]
 *   arrivals   n_chunks device counters, zero before the first launch (the launch leaves them zero)
 *   signal     n_chunks words from glnn_signal_alloc(); when every row of chunk c is stored (acknowledged by the L2) the kernel
 *              stores `epoch` there -- glnn_stream_wait_value32(other_stream, signal[c], epoch) then holds that stream's next
 *              operation (the chunk's all-gather) until the chunk is complete AND written back to device memory, while the launch
 *              is still running.  Use a new, larger epoch per launch (the wait is "value >= epoch", unsigned 32-bit).
 * `tile_order` may permute the tiles freely; completion order follows it (the caller concatenates the chunks' orders). */
#define GLNN_MAX_CHUNKS 8
typedef struct glnn_chunk_signals {
  int32_t n_chunks;
  int64_t row_start[GLNN_MAX_CHUNKS + 1];
  int64_t self_row[GLNN_MAX_CHUNKS];
  int64_t out_row[GLNN_MAX_CHUNKS];
  int32_t* arrivals;
  uint32_t* signal[GLNN_MAX_CHUNKS];
  uint32_t epoch;
} glnn_chunk_signals;
GLNN_API int glnn_sage_fused_chunks_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                        int64_t n_src, const float* x, int64_t ldx, int d_in,
                                        const float* x_self, int64_t ld_self, const float* w_packed,
                                        int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                        float* out, int64_t ldo, const float* w2_packed, int d_out2,
                                        float* out2, int64_t ldo2, const int32_t* tile_order,
                                        const glnn_hub_plan* plan, const glnn_chunk_signals* chunks, void* stream);
/* The stand-alone SAGE-"gcn" aggregation in the same form (glnn_spmm_csr_plan_f32 + chunks; mode = GLNN_AGG_SAGE_GCN, d <= 256): the self
 * row of row v of chunk c is x_self[self_rows ? self_rows[v] : self_row[c] + v - row_start[c]], its output row out_row[c] + v - row_start[c].
 * Rows of more than the long-row threshold are summed by the launch's long-row workgroups chunk by chunk; a chunk signals when its row
 * workgroups AND every long-row workgroup's share of it are stored. */
GLNN_API int glnn_spmm_csr_chunks_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                      int64_t n_src, const float* x, int64_t ldx, int d, int mode,
                                      const float* row_scale, const float* col_scale,
                                      const float* x_self, int64_t ld_self, const int64_t* self_rows,
                                      const float* ep_scale, const float* ep_shift, int relu, float* out,
                                      int64_t ldo, const glnn_hub_plan* plan, const glnn_chunk_signals* chunks,
                                      void* stream);
/* A 32-bit signal word a stream can wait on (hipExtMallocWithFlags(hipMallocSignalMemory)), initialised to 0; its current value;
 * "the next operation of `stream` starts when *signal >= value" (hipStreamWaitValue32, GTE) -- followed by an empty kernel on `stream`,
 * whose end-of-kernel release writes back the L2s in which the signalled rows may still sit. */
GLNN_API int glnn_signal_alloc(uint32_t** signal);
GLNN_API int glnn_signal_free(uint32_t* signal);
GLNN_API int glnn_signal_read(const uint32_t* signal, uint32_t* value);
GLNN_API int glnn_stream_wait_value32(void* stream, uint32_t* signal, uint32_t value);

/* in_deg[v] = t(indptr[v+1]-indptr[v]); out_deg[u] = t(#edges with source u), as floats, t = `transform`:
 *   GLNN_DEG_RAW          the degree itself            g.in_degrees() / g.out_degrees()
 *   GLNN_DEG_RSQRT_CLAMP1 deg.clamp(min=1) ** -0.5     the norm of dgl GraphConv(norm="both") and utils.py:178-179
 *   GLNN_DEG_INV_PLUS1    1 / (deg + 1)                the divisor of the SAGE-"gcn" aggregator (its backward's col_scale)
 * Either output may be NULL.  nnz = indptr[n_dst] (host value).  out_deg need not be zeroed by the caller. */
#define GLNN_DEG_RAW 0
#define GLNN_DEG_RSQRT_CLAMP1 1
#define GLNN_DEG_INV_PLUS1 2
GLNN_API int glnn_degrees_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                              int64_t n_src, int64_t nnz, int transform, float* in_deg,
                              float* out_deg, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3  Dense projection on the fp32 MFMA path (v_mfma_f32_32x32x2_f32, exact fp32).
 *   C[m,n] = epilogue( sum_k A'[m,k] * B[k,n] )
 *   A' = A, or rows gathered through a_rows (A'[m,:] = A[a_rows[m],:], replaces feats[idx]
 *        at reference train_and_eval.py:76 / models.py:136), optionally passed through the
 *        "previous layer tail"  A'[m,k] = drop(max(A[m,k]*a_scale[k] + a_shift[k], 0))  (BatchNorm,
 *        ReLU and training-mode Dropout of reference models.py:48-52 folded into the operand load;
 *        a_scale NULL = identity, no ReLU, no dropout).  drop(v) = keep(m,k) ? v/(1-drop_p) : 0 with
 *        keep() the counter-based mask of glnn_dropout_mask_u8 (drop_p = 0 disables it).
 *   B  = W^T with W [n,k] row-major (torch.nn.Linear / dgl SAGEConv.fc_neigh, b_layout 0)
 *        or W [k,n] row-major (dgl GraphConv.weight, b_layout 1).
 *   epilogue, in order, each optional: * row_scale[m] ; * ep_scale[n] ; + ep_shift[n] ; ReLU.
 *   workspace (optional, floats): lets skinny outputs (few 128x128 tiles, deep K) split the K
 *   reduction over more workgroups; partials are summed in fixed order (deterministic).  NULL = never.
 * replaces fc_neigh / GraphConv weight / nn.Linear: reference models.py:45,112,138,193.
 * ------------------------------------------------------------------------------------------ */
GLNN_API int glnn_gemm_f32(const float* a, int64_t lda, const int64_t* a_rows,
                           const float* a_scale, const float* a_shift, float drop_p,
                           uint32_t drop_seed, int64_t m, int k,
                           const float* b, int64_t ldb, int b_layout, int n,
                           const float* row_scale, const float* ep_scale, const float* ep_shift,
                           int relu, float* c, int64_t ldc, float* workspace,
                           int64_t workspace_floats, void* stream);

/* TN form, the weight-gradient shape:  C[i,j] = sum_m A[m,i] * B'[m,j]   (i < ka, j < nb)
 *   dW[out,in] = dZ^T @ A_prev with A = dZ [m,out] and B = the previous layer's PRE-activation
 *   (or the gathered input features), B' = B passed through the same operand transform as
 *   glnn_gemm_f32 (row gather b_rows, then max(B*b_scale+b_shift,0)), so the activation is
 *   recomputed instead of stored.  Replaces the nn.Linear weight/bias gradient autograd computes
 *   inside loss.backward(), reference train_and_eval.py:84.
 *   col_sum_a != NULL also writes col_sum_a[i] = sum_m A[m,i] (the bias gradient).
 *   workspace (floats) is used for a deterministic split of the m-reduction when the output is
 *   small, and for the column sums (needs >= 64*ka floats for those). */
GLNN_API int glnn_gemm_tn_f32(const float* a, int64_t lda, int64_t m, int ka, const float* b,
                              int64_t ldb, const int64_t* b_rows, const float* b_scale,
                              const float* b_shift, float drop_p, uint32_t drop_seed, int nb,
                              float* c, int64_t ldc,
                              float* col_sum_a, float* workspace, int64_t workspace_floats,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * K4  Losses on raw logits, forward + gradient wrt logits in one pass.
 *   kind GLNN_LOSS_NLL: NLLLoss()(log_softmax(z), y)                 train_student.py:278
 *   kind GLNN_LOSS_KL : KLDivLoss("batchmean", log_target=True)(log_softmax(z), t)  :279
 *   loss_out[0]   = unscaled mean loss of the batch (what .item() reports, train_and_eval.py:80)
 *   loss_accum[0]+= the same (optional, NULL to skip) so a whole pass reads back ONE scalar
 *   dlogits       = d(lamb * loss)/dz   (train_and_eval.py:82 scales the loss by lamb)
 *   logprob_out   = log_softmax(z) (optional)
 *   workspace     >= min(ceil(rows/4), 1024) floats (per-workgroup partial sums; fixed-order reduce)
 *   labels / target_logp may be indexed through label_rows / target_rows (the batch's node ids) so
 *   that labels[idx] / out_t[idx] (train_and_eval.py:79) are never materialised; NULL = identity.
 * ------------------------------------------------------------------------------------------ */
#define GLNN_LOSS_NLL 0
#define GLNN_LOSS_KL 1
GLNN_API int glnn_softmax_loss_f32(const float* logits, int64_t ldz, int64_t rows, int c, int kind,
                                   const int64_t* labels, const int64_t* label_rows,
                                   const float* target_logp, int64_t ldt, const int64_t* target_rows,
                                   float lamb, float* dlogits, int64_t ldg, float* logprob_out,
                                   int64_t ldl, float* loss_out, float* loss_accum,
                                   float* workspace, int64_t workspace_floats, void* stream);

/* The last layer of a student and its criterion in ONE launch (ABI 11; reference models.py:45-52 last Linear + train_and_eval.py:77-84):
 *   logits = tail(a) . w^T + bias,  tail(a) = dropout(relu(a * a_scale + a_shift)) (a_scale / a_shift NULL: a is used as stored),
 *   followed by glnn_softmax_loss_f32's arithmetic on those logits (same loss / dlogits bits), by workgroups that own 16 rows.
 *   For LARGE batches in front of a NARROW classifier: rows > 1024, c <= 48, k % 256 == 0, 256 <= k <= 4096, float4-addressable rows of
 *   a and w; kind < 0: logits only (dlogits / loss_out / workspace unused).  With a criterion: rows <= 4096 and
 *   workspace >= ceil(rows/4) floats.  Any other shape: GLNN_ERR_UNSUPPORTED with nothing launched (use glnn_gemm_f32 +
 *   glnn_softmax_loss_f32). */
GLNN_API int glnn_classifier_loss_f32(const float* a, int64_t lda, const float* a_scale, const float* a_shift,
                                      float drop_p, uint32_t drop_seed, int64_t rows, int k, const float* w, int64_t ldw,
                                      int c, const float* bias, float* logits, int64_t ldz, int kind,
                                      const int64_t* labels, const int64_t* label_rows, const float* target_logp,
                                      int64_t ldt, const int64_t* target_rows, float lamb, float* dlogits, int64_t ldg,
                                      float* loss_out, float* loss_accum, float* workspace, int64_t workspace_floats,
                                      void* stream);

/* row-wise log_softmax only (evaluate paths, train_and_eval.py:98,124). in place allowed. */
GLNN_API int glnn_log_softmax_f32(const float* logits, int64_t ldz, int64_t rows, int c, float* out,
                                  int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5  BatchNorm1d training statistics + backward pieces (reference models.py:28-31,48-49:
 *     eps 1e-5, momentum 0.1, biased batch variance for normalisation, unbiased for running_var).
 *   glnn_bn_stats_f32: from z [rows,h] computes a_scale = gamma*rstd, a_shift = beta - mean*a_scale
 *     (the operand transform the next glnn_gemm_f32 consumes), saves mean/rstd, and updates
 *     running_mean / running_var / num_batches_tracked in place.  workspace: c = ceil(rows/128) row chunks ->
 *     >= 2*c*h floats, plus 3*ceil(c/64)*h when c > 256 (two-level combine of the per-chunk statistics).
 *   glnn_bn_relu_bwd_f32: given da (grad wrt the post-ReLU activation) and z, computes
 *     dy = da * [z*a_scale+a_shift > 0], dgamma = sum dy*xhat, dbeta = sum dy and
 *     dz = gamma*rstd*(dy - mean(dy) - xhat*mean(dy*xhat)); in place on da allowed.
 *     With gamma == NULL (norm_type "none") it is the plain ReLU backward dz = da*[z>0].
 *     dz_col_sum (optional) receives sum over rows of dz = the bias gradient of the Linear in front.
 *     workspace: >= ceil(rows/128)*h*(2 if gamma else 0 + 1 if dz_col_sum else 0) + 2*h floats.
 *     drop_p > 0 first applies the Dropout backward da *= keep(row,col)/(1-drop_p) with the same
 *     (drop_seed) mask the forward operand transform used.
 * ------------------------------------------------------------------------------------------ */
GLNN_API int glnn_bn_stats_f32(const float* z, int64_t ldz, int64_t rows, int h, const float* gamma,
                               const float* beta, float eps, float momentum, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, float* mean_out,
                               float* rstd_out, float* a_scale_out, float* a_shift_out,
                               float* workspace, int64_t workspace_floats, void* stream);

/* ABI 8: z = a W^T + bias [m, n] followed by glnn_bn_stats_f32 on z -- Linear + BatchNorm1d statistics of a hidden layer (reference
 * models.py:43-47, 110-114).  When the product runs on the row-panel kernel (k <= 128 over many rows) or the pipelined kernel
 * (k % 32 == 0, plain operands, >= 64 output tiles) the statistics' first pass comes out of the product's epilogue (per-workgroup /
 * per-tile count, mean, M2 of the stored values) and z is not read again; otherwise the two calls run as they are.  Plain operands
 * only.  ws_bn: as glnn_bn_stats_f32, and >= 3 * 128 * n floats for the row-panel form.  GLNN_GEMM_STATS=0 forces the two-call form. */
GLNN_API int glnn_linear_bn_stats_f32(const float* a, int64_t lda, int64_t m, int k, const float* w, int64_t ldw, int n,
                                      const float* bias, float* z, int64_t ldz, const float* gamma, const float* beta,
                                      float eps, float momentum, float* running_mean, float* running_var,
                                      int64_t* num_batches_tracked, float* mean_out, float* rstd_out, float* a_scale_out,
                                      float* a_shift_out, float* ws_gemm, int64_t ws_gemm_floats, float* ws_bn,
                                      int64_t ws_bn_floats, void* stream);

GLNN_API int glnn_bn_relu_bwd_f32(const float* da, int64_t ldda, const float* z, int64_t ldz,
                                  int64_t rows, int h, const float* gamma, const float* mean,
                                  const float* rstd, const float* a_scale, const float* a_shift,
                                  float drop_p, uint32_t drop_seed,
                                  float* dz, int64_t lddz, float* dgamma, float* dbeta,
                                  float* dz_col_sum,
                                  float* workspace, int64_t workspace_floats, void* stream);

/* out[j] = sum over rows of x[:, j] (fixed summation order): the bias gradient of a layer whose dz does not come out of
 * glnn_bn_relu_bwd_f32 (last GraphConv of the full-graph GCN step, reference train_and_eval.py:12-29).
 * workspace >= ceil(rows/128) * h floats. */
GLNN_API int glnn_col_sum_f32(const float* x, int64_t ldx, int64_t rows, int h, float* out,
                              float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * K6  Fused multi-tensor Adam, torch.optim.Adam semantics (L2 weight decay folded into the
 *     gradient, bias correction, eps outside the sqrt): reference train_student.py:275-277,
 *     train_teacher.py:234-236, stepped at train_and_eval.py:85.
 *   The tensor table is 4 device arrays of `num_tensors` pointers + one of sizes (elements).
 *   `step` is the 1-based step count AFTER this update.
 * ------------------------------------------------------------------------------------------ */
GLNN_API int glnn_adam_step_f32(float* const* params, const float* const* grads,
                                float* const* exp_avg, float* const* exp_avg_sq,
                                const int64_t* sizes, int num_tensors, int64_t max_size,
                                float lr, float beta1, float beta2, float eps, float weight_decay,
                                int64_t step, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole forward + loss + backward of one student step in ONE call (reference train_and_eval.py:74-84:
 * model(None, feats[idx]) -> log_softmax -> criterion -> (loss*lamb).backward()), issuing the K3-K5
 * launches above in a fixed order.  Every buffer is caller-owned; the descriptor only carries pointers:
 *   w/b/gw/gb[l]      Linear l weight [dims[l+1], dims[l]] / bias and their gradients (contiguous)
 *   gamma..nbt[l]     BatchNorm1d after hidden layer l (l < L-1) when batchnorm != 0
 *   mean/rstd/a_scale/a_shift[l]  per-hidden-layer vectors; with batchnorm == 0 a_scale/a_shift must be
 *                     pre-filled with ones/zeros (the operand transform is then the plain ReLU)
 *   z[l] (ldz[l])     pre-activation output of hidden layer l, [max_batch, dims[l+1]]
 *   da/dz             scratch [max_batch, max hidden]; ws_*: workspaces of the individual kernels
 *   loss_out/accum    as in glnn_softmax_loss_f32
 * idx: the batch's row ids into feats (and into labels / target_logp through target_rows), NULL = rows 0..m-1.
 * drop_seeds: host array of L-1 uint32 (one per hidden layer) when dropout_p > 0.
 * The optimiser step is NOT included: call glnn_adam_step_f32 next (a gradient all-reduce may sit between).
 * ------------------------------------------------------------------------------------------ */
#define GLNN_MLP_MAX_LAYERS 8
#define GLNN_MLP_COUNTERS 1024   /* ints behind glnn_mlp_step_desc.sync_counters: one per 64-column block + one for the loss */

/* Optional data-parallel hook (SURVEY.md 8e "Student"): when one batch is split over `world` ranks the
 * BatchNorm batch statistics must be taken over the WHOLE batch for the step to equal the single-GPU
 * reference step.  The library leaves the collective to the host: it fills `send` with `floats` values,
 * calls exchange(ctx, send, recv, floats, stream) and expects recv = the concatenation of every rank's
 * `send` in rank order (an all-gather, enqueued on / ordered after `stream`; ncclAllGather in a native
 * host, torch.distributed in the Python mirror).  Return 0 on success.  Two calls per BatchNorm layer and
 * step: 3*h floats forward (count, mean, M2 per column -> Chan combine in fixed rank order, so every rank
 * derives bit-identical statistics), 2*h floats backward (sum dy, sum dy*xhat).  dgamma/dbeta and all other
 * gradients stay LOCAL sums: the caller's gradient all-reduce completes them. */
typedef int (*glnn_exchange_fn)(void* ctx, const float* send, float* recv, int64_t floats, void* stream);

typedef struct glnn_mlp_step_desc {
  int32_t num_layers;
  int32_t batchnorm;      /* hidden-layer norm: 0 none, 1 nn.BatchNorm1d, 2 nn.LayerNorm (ABI 5: gamma/beta = its affine, bn_eps = its eps,
                           * mean[l]/rstd[l] = max_batch floats of per-ROW statistics, act[l] required, a_scale/a_shift/running_* unused) */
  int32_t dims[GLNN_MLP_MAX_LAYERS + 1];
  float dropout_p;
  float bn_eps;
  float bn_momentum;
  int64_t max_batch;
  float* w[GLNN_MLP_MAX_LAYERS];
  float* b[GLNN_MLP_MAX_LAYERS];
  float* gw[GLNN_MLP_MAX_LAYERS];
  float* gb[GLNN_MLP_MAX_LAYERS];
  float* gamma[GLNN_MLP_MAX_LAYERS];
  float* beta[GLNN_MLP_MAX_LAYERS];
  float* ggamma[GLNN_MLP_MAX_LAYERS];
  float* gbeta[GLNN_MLP_MAX_LAYERS];
  float* running_mean[GLNN_MLP_MAX_LAYERS];
  float* running_var[GLNN_MLP_MAX_LAYERS];
  int64_t* nbt[GLNN_MLP_MAX_LAYERS];
  float* mean[GLNN_MLP_MAX_LAYERS];
  float* rstd[GLNN_MLP_MAX_LAYERS];
  float* a_scale[GLNN_MLP_MAX_LAYERS];
  float* a_shift[GLNN_MLP_MAX_LAYERS];
  float* z[GLNN_MLP_MAX_LAYERS];
  int64_t ldz[GLNN_MLP_MAX_LAYERS];
  float* logits;
  int64_t ld_logits;
  float* dlogits;
  int64_t ld_dlogits;
  float* da;
  int64_t ld_da;
  float* dz;
  int64_t ld_dz;
  float* ws_bn;
  int64_t ws_bn_floats;
  float* ws_tn;
  int64_t ws_tn_floats;
  float* ws_gemm;
  int64_t ws_gemm_floats;
  float* ws_loss;
  int64_t ws_loss_floats;
  float* loss_out;
  float* loss_accum;
  /* batch split over ranks (all zero / NULL = single rank) */
  int32_t world;
  int32_t rank;
  glnn_exchange_fn exchange;
  void* exchange_ctx;
  float* sync_send;      /* >= 3 * max hidden floats */
  float* sync_recv;      /* >= world * 3 * max hidden floats */
  float* sync_rows;      /* 1 float: the global batch row count of the current step (written by the library) */
  /* optional: GLNN_MLP_COUNTERS device ints, ZERO when first handed over (the library leaves them zero).  With them the
   * BatchNorm statistics, the bias-gradient column sums and the loss finish inside their first launch (the last
   * workgroup folds the partials) instead of in a second one: 7 launches fewer per 3-layer step.  ws_loss must then hold
   * >= 256 * 65 floats for the last layer's bias gradient to ride along (label_dim <= 64).  NULL = two-launch forms. */
  int32_t* sync_counters;
  /* optional, per hidden layer l: act[l] [max_batch, ld_act[l]] receives dropout(relu(norm(z[l]))) once per step
   * (glnn_act_fwd_f32) and the next layer's forward and weight-gradient GEMMs read it as a plain operand.  NULL = that tail
   * is recomputed inside their operand loads (nothing stored): cheaper for narrow layers and small batches; with dropout
   * and a wide next layer the per-element mask hash, re-evaluated by every workgroup that stages the tile, costs more
   * than one 8-byte-per-element pass (MLP3w8: 316 vs 260+13 us forward, 309 vs 277 us weight gradient). */
  float* act[GLNN_MLP_MAX_LAYERS];
  int64_t ld_act[GLNN_MLP_MAX_LAYERS];
  /* optional: xb [max_batch, ld_xb] receives feats[idx] once per step (glnn_gather_rows_f32) and the first layer's forward and
   * weight-gradient GEMMs read it as a plain operand -- the weight gradient then qualifies for the pipelined kernel
   * (B=4096, 2048 x 100: 38 + 9 us gathered vs 29 us plain + a 4 us gather).  NULL (or idx == NULL) = rows gathered in the
   * operand loads. */
  float* xb;
  int64_t ld_xb;
  /* optional data-parallel hook: called on the host right after the weight-gradient GEMM of `layer` has been enqueued, i.e.
   * gw[layer] is complete in `stream` order while the rest of the backward (input gradient, BatchNorm backward, the layers
   * in front) is still to be issued -- the host can start that layer's gradient all-reduce on its own stream and overlap
   * it (glnn_amd.dist.OverlappedGradSync: MLP3w8's 16 MB hidden-layer gradient rides under ~0.35 ms of remaining backward).
   * Return 0 on success.  NULL = no call. */
  int (*grad_ready)(void* ctx, int layer, void* stream);
  void* grad_ready_ctx;
  /* optional second [max_batch, ld_dz2] gradient buffer (ABI 7: the aux_stream / ev_main / ev_aux fields of the two-stream backward
   * of ABI 5-6 are gone -- measured slower, removed): small steps collect their weight gradients and issue them as ONE launch at the
   * end of the backward; dz_l then alternates between dz and dz2 so that it outlives the loop. */
  float* dz2;
  int64_t ld_dz2;
} glnn_mlp_step_desc;

GLNN_API int glnn_mlp_fwd_bwd_f32(const glnn_mlp_step_desc* desc, const float* feats, int64_t ldx,
                                  const int64_t* idx, int64_t m, int kind, const int64_t* labels,
                                  const float* target_logp, int64_t ldt, const int64_t* target_rows,
                                  float lamb, const uint32_t* drop_seeds, void* stream);

/* ------------------------------------------------------------------------------------------
 * ABI 6: the WHOLE optimisation step of the student in one call -- glnn_mlp_fwd_bwd_f32 followed by glnn_adam_step_f32 on the
 * same stream (reference train_and_eval.py:74-85: forward, loss, backward, optimizer.step()), for hosts with nothing to put
 * between the two (no gradient exchange).  Because Adam is known to be the next launch and the only consumer of the gradients,
 * the backward leaves the final sums of its gradient partials to it (the split-K slabs of the weight gradients, the per-chunk
 * column sums behind the bias gradients, the per-workgroup loss partials): the fold launches and last-workgroup tails of the
 * two-call form disappear, the sums and their order do not (same bits), and the folded gradients are still stored to `grads`.
 * glnn_adam_desc: the arguments of glnn_adam_step_f32 plus `grads_host`, a HOST copy of the device pointer table `grads`
 * (num_tensors entries; how a pending fold finds its tensor).  num_tensors <= 32 for the folds; more tensors take the plain form.
 * ------------------------------------------------------------------------------------------ */
typedef struct glnn_adam_desc {
  float* const* params; const float* const* grads; float* const* exp_avg; float* const* exp_avg_sq; const int64_t* sizes;
  const float* const* grads_host;
  int32_t num_tensors; int32_t reserved;
  int64_t max_size;
  float lr, beta1, beta2, eps, weight_decay; int32_t reserved2;
  int64_t step;                       /* 1-based step count AFTER this update */
} glnn_adam_desc;

GLNN_API int glnn_mlp_train_step_f32(const glnn_mlp_step_desc* desc, const float* feats, int64_t ldx,
                                     const int64_t* idx, int64_t m, int kind, const int64_t* labels,
                                     const float* target_logp, int64_t ldt, const int64_t* target_rows,
                                     float lamb, const uint32_t* drop_seeds, const glnn_adam_desc* adam, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole forward + NLL + backward of ONE sampled-block GraphSAGE training step in one call (reference
 * train_and_eval.py:39-53 over SAGE.forward, models.py:101-119): per layer glnn_spmm_csr_f32 (SAGE_GCN) -> glnn_gemm_f32 ->
 * glnn_bn_stats_f32 -> glnn_act_fwd_f32; glnn_softmax_loss_f32 with labels[label_rows[i]]; backward per layer
 * glnn_gemm_tn_f32 -> glnn_gemm_f32 -> glnn_csr_transpose(add_self) + glnn_degrees_f32(1/(deg+1)) + glnn_spmm_csr_f32 (SUM
 * over the transposed block) -> glnn_bn_relu_bwd_f32.  Every buffer is caller-owned:
 *   layer[l].indptr/indices   block l (CSR over its destinations; layer[0] outermost), n_src of block l == n_dst of block l-1;
 *                             layer[0] may carry GLOBAL column ids with self_rows[v] = global id of destination v, x = feats
 *   w/b/gw/gb                 fc_neigh weight [dims[l+1], dims[l]] / bias and their gradients (contiguous)
 *   gamma..a_shift            BatchNorm1d after hidden layer l (batchnorm != 0)
 *   agg/z/h                   kept activations: aggregate [n_dst, dims[l]], pre-activation [n_dst, dims[l+1]] (z of the last
 *                             layer = logits), hidden output [n_dst, dims[l+1]] (float4 rows: leading dims % 4 == 0)
 *   t_indptr/t_indices/inv_deg/tr_ws  (l >= 1) outputs / workspace of the block's transpose (glnn_csr_transpose sizes)
 *   dagg [max n_dst_l, max dims[l]], dh [max n_src_l, max dims[l]] (l >= 1)   backward scratch
 * Round 5 (same ABI, same results to rounding): with batchnorm != 0 and float4-addressable buffers big enough (ws_bn >= 2 slots dims[1] +
 * 5 dims[1] + 8 floats, slots = n_dst_0 / 128 + <= 512; ws_tn >= 8 dims[0] dims[1] floats) the BatchNorm backward of the OUTERMOST layer has
 * no pass of its own -- the transposed aggregation stores dy = da behind the tail's masks and the column sums, dz = alpha dy + beta z +
 * gamma is evaluated in the operand loads of dW_0; gb of layer 0 (true gradient 0 in front of a BatchNorm) is then exactly 0.  Otherwise,
 * or with GLNN_SAGE_FUSE_BN_APPLY=0 / GLNN_SAGE_FUSE_BN_DY=0, the launch sequence above.  Blocks of <= 6 in-edges per row on average
 * (layer[l].nnz) take the four-rows-per-wave aggregation kernel (GLNN_SPMM_SHORT=0: never; same bits).
 * The optimiser step is NOT included: call glnn_adam_step_f32 next.
 * ------------------------------------------------------------------------------------------ */
#define GLNN_SAGE_MAX_LAYERS 8
typedef struct glnn_sage_layer {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst, n_src, nnz;
  const int64_t* self_rows;
  float* w; float* b; float* gw; float* gb;
  float* gamma; float* beta; float* ggamma; float* gbeta; float* running_mean; float* running_var; int64_t* nbt;
  float* mean; float* rstd; float* a_scale; float* a_shift;
  float* agg; int64_t ld_agg; float* z; int64_t ldz; float* h; int64_t ldh;      /* h may be NULL (hidden layers): the tail of z is then
                                                                                   * applied inside the next layer's aggregation, never written */
  int64_t* t_indptr; int32_t* t_indices; float* inv_deg; void* tr_ws; int64_t tr_ws_bytes;
  /* (layers >= 1) scratch the step fills: the block transposed with one self entry per destination (glnn_csr_transpose(..., add_self = 1)) and
   * 1 / (in-degree + 1) (glnn_degrees_f32, GLNN_DEG_INV_PLUS1).  tr_ws == NULL: t_indptr / t_indices / inv_deg already HOLD them -- built by
   * the caller, e.g. by its batch loader beside the previous step (round 5: the ten launches leave the step's stream). */
  uint32_t drop_seed;
} glnn_sage_layer;

typedef struct glnn_sage_step_desc {
  int32_t num_layers;
  int32_t batchnorm;
  int32_t dims[GLNN_SAGE_MAX_LAYERS + 1];
  float dropout_p, bn_eps, bn_momentum, lamb;
  glnn_sage_layer layer[GLNN_SAGE_MAX_LAYERS];
  const float* x; int64_t ldx; int64_t x_rows;        /* source matrix of layer 0: feats (global ids) or the gathered batch features */
  const int64_t* labels; const int64_t* label_rows;   /* labels[label_rows[i]] for destination i of the last block (label_rows NULL = i) */
  float* dlogits; int64_t ld_dlogits;
  float* dagg; int64_t ld_dagg; float* dh; int64_t ld_dh;
  float* ws_bn; int64_t ws_bn_floats; float* ws_tn; int64_t ws_tn_floats; float* ws_gemm; int64_t ws_gemm_floats;
  float* ws_loss; int64_t ws_loss_floats;
  float* loss_out; float* loss_accum;
} glnn_sage_step_desc;

GLNN_API int glnn_sage_fwd_bwd_f32(const glnn_sage_step_desc* desc, void* stream);
/* ... and the same followed by the fused Adam launch in ONE call (ABI 11; reference train_and_eval.py:39-53 incl. optimizer.step()):
 * the backward leaves its last partial sums (split slabs of the weight gradients, the last layer's bias-gradient column partials, the
 * per-workgroup losses) to Adam -- the same parameters, moments and loss as glnn_sage_fwd_bwd_f32 + glnn_adam_step_f32, bit for bit.
 * `adam` as in glnn_mlp_train_step_f32. */
GLNN_API int glnn_sage_train_step_f32(const glnn_sage_step_desc* desc, const glnn_adam_desc* adam, void* stream);
/* ABI 10: ws_bn floats with which the outermost layer's BatchNorm backward takes the form without passes of its own (see above) for an
 * outermost block of n_dst_0 destinations and dims[1] = hidden; the step's other uses of ws_bn need (3 chunks + 2 + 3 ceil(chunks / 64)) *
 * max hidden + 1024 floats, chunks = ceil(max n_dst / 128): allocate the larger of the two. */
GLNN_API int64_t glnn_sage_step_ws_bn_floats(int64_t n_dst_0, int hidden);

/* The same step for SAGE teachers whose hidden layers end in nn.LayerNorm(hidden) -> ReLU -> dropout (reference models.py:87-97, 113-117,
 * norm_type "layer"): desc->batchnorm must be 0, the desc's BatchNorm fields are unused; `ln` carries eps and, per hidden layer l, the
 * LayerNorm's weight / bias (gamma, beta), their gradients and the row statistics of z_l (mean / rstd [n_dst_l] floats, written by the
 * forward, read by the backward).  Forward per hidden layer: glnn_layernorm_fwd_f32 (h == NULL: the statistics alone, the next layer's
 * gather applies the tail).  Backward: the transposed aggregation's epilogue is the whole LayerNorm backward (dz stored, dh never
 * written; GLNN_SAGE_FUSE_LN_BWD=0 or a hidden width above 256: the aggregation writes dh, glnn_layernorm_bwd_f32 follows).
 * ws_bn >= max over hidden layers of glnn_sage_step_ws_ln_floats(n_dst_l, dims[l+1]).  No float atomics: bit-reproducible. */
typedef struct glnn_sage_ln_layer {
  const float* gamma; const float* beta; float* ggamma; float* gbeta; float* mean; float* rstd;
} glnn_sage_ln_layer;
typedef struct glnn_sage_ln_desc {
  float eps; int32_t reserved;
  glnn_sage_ln_layer layer[GLNN_SAGE_MAX_LAYERS];     /* hidden layers 0 .. num_layers - 2 */
} glnn_sage_ln_desc;
GLNN_API int glnn_sage_fwd_bwd_ln_f32(const glnn_sage_step_desc* desc, const glnn_sage_ln_desc* ln, void* stream);
/* ... and followed by the fused Adam launch (as glnn_sage_train_step_f32): bit-identical to glnn_sage_fwd_bwd_ln_f32 + glnn_adam_step_f32 */
GLNN_API int glnn_sage_train_step_ln_f32(const glnn_sage_step_desc* desc, const glnn_sage_ln_desc* ln, const glnn_adam_desc* adam,
                                         void* stream);
GLNN_API int64_t glnn_sage_step_ws_ln_floats(int64_t n_dst, int hidden);

/* The same step for SAGE teachers built with the "mean" aggregator (dgl 0.6.1 SAGEConv(in, out, "mean"); docs/SAGE_MEAN_SEMANTICS.md; the
 * reference only builds "gcn", so this replaces no reference call site -- it is train_and_eval.py:39-53 over that layer):
 *   z_l = [mean_l | self_l] [W_neigh | W_self]^T + (b_neigh + b_self),  mean_l[v] = (1 / max(deg v, 1)) sum_{u->v} h_l[u],  self_l[v] = h_l[v]
 * `desc` is the "gcn" step's descriptor with w / b / gw / gb = fc_neigh; agg, ld_agg, dagg, ld_dagg and inv_deg are unused.  `mean` adds,
 * per layer, fc_self and the step's own scratch:
 *   w_self/b_self/gw_self/gb_self  fc_self weight [dims[l+1], dims[l]] / bias and their gradients (contiguous)
 *   cat, ld_cat     the operand pair [mean | self] per destination row, [n_dst, ld_cat] floats, ld_cat == 2 * round4(dims[l]); the self
 *                   half starts at column round4(dims[l]); padding columns are written as zeros
 *   wcat, bsum      [dims[l+1], ld_cat] and [dims[l+1]] floats: [W_neigh | W_self] in the same layout and b_neigh + b_self, re-packed on
 *                   the device by every call (the parameters stay the fc_self / fc_neigh tensors)
 *   dcat, ld_dcat   (l >= 1) dz [W_neigh | W_self], [n_dst, ld_dcat] floats, ld_dcat == ld_cat; layers may share one buffer
 * t_indptr / t_indices of layers >= 1 hold (tr_ws == NULL) or receive (tr_ws != NULL) the PLAIN transposed block,
 * glnn_csr_transpose(..., add_self = 0): "mean" has no identity term.  `ln` NULL: the tails of desc (BatchNorm when desc->batchnorm, else
 * none); non-NULL: LayerNorm tails as in glnn_sage_fwd_bwd_ln_f32.  h == NULL on a hidden layer (width <= 256, else GLNN_ERR_UNSUPPORTED):
 * its tail is evaluated inside the next layer's gather, on the gathered rows and on the self row, bit-identical to the stored form.
 * Backward per layer: two glnn_gemm_tn_f32 over the halves of cat, dcat by glnn_gemm_f32, the transposed aggregation
 * dh[u] = sum_{v: u->v} dcat[v, :d] / max(deg v, 1) + (u < n_dst ? dcat[u, ld_cat/2 : ld_cat/2 + d] : 0) -- every row of dh is written --
 * then glnn_bn_relu_bwd_f32 / glnn_layernorm_bwd_f32; both bias gradients of a layer receive colsum(dz).  Workspaces as the "gcn" step
 * (ws_tn >= 64 * max dims floats).  No float atomics: bit-reproducible.  Bad arguments return GLNN_ERR_INVALID_ARG before any launch. */
typedef struct glnn_sage_mean_layer {
  float* w_self; float* b_self; float* gw_self; float* gb_self;
  float* cat; int64_t ld_cat;
  float* wcat; float* bsum;
  float* dcat; int64_t ld_dcat;
} glnn_sage_mean_layer;
typedef struct glnn_sage_mean_desc {        /* glnn_struct_bytes(8) */
  int32_t num_layers; int32_t reserved;
  glnn_sage_mean_layer layer[GLNN_SAGE_MAX_LAYERS];
} glnn_sage_mean_desc;
GLNN_API int glnn_sage_mean_fwd_bwd_f32(const glnn_sage_step_desc* desc, const glnn_sage_mean_desc* mean, const glnn_sage_ln_desc* ln,
                                        void* stream);
/* ... followed by the fused Adam launch on the same stream: the same bits as glnn_sage_mean_fwd_bwd_f32 + glnn_adam_step_f32 */
GLNN_API int glnn_sage_mean_train_step_f32(const glnn_sage_step_desc* desc, const glnn_sage_mean_desc* mean, const glnn_sage_ln_desc* ln,
                                           const glnn_adam_desc* adam, void* stream);

/* y = dropout(relu(z * a_scale + a_shift)) materialised (a_scale/a_shift NULL: plain ReLU): the `norms[l](h)` ->
 * `activation` -> `dropout` tail of a TRAINING-mode SAGE layer (reference models.py:113-117), whose output the next
 * layer's aggregation gathers.  a_scale/a_shift come from glnn_bn_stats_f32; the backward is glnn_bn_relu_bwd_f32 with
 * the same (drop_p, drop_seed).  z, y: float4 rows (leading dimensions % 4 == 0, >= round4(h)); padding columns of y = 0. */
GLNN_API int glnn_act_fwd_f32(const float* z, int64_t ldz, int64_t rows, int h, const float* a_scale,
                              const float* a_shift, float drop_p, uint32_t drop_seed, float* y, int64_t ldy,
                              void* stream);

/* glnn_act_fwd_f32 / glnn_bn_relu_bwd_f32 with the tail's ReLU optional (ABI 5).  relu = 0 is the hidden-layer tail of the
 * reference's GCN (models.py:189-199: GraphConv(activation=relu) -> norms[l] -> dropout -- the ReLU sits inside the conv, IN
 * FRONT of the norm; train.conf.yaml's pokec / penn94 GCN sections use norm_type batch): y = dropout(z * a_scale + a_shift),
 * and the backward gates nothing by the sign of the normalised value. */
GLNN_API int glnn_norm_drop_fwd_f32(const float* z, int64_t ldz, int64_t rows, int h, const float* a_scale,
                                    const float* a_shift, int relu, float drop_p, uint32_t drop_seed, float* y,
                                    int64_t ldy, void* stream);
GLNN_API int glnn_bn_bwd_f32(const float* da, int64_t ldda, const float* z, int64_t ldz, int64_t rows, int h,
                             const float* gamma, const float* mean, const float* rstd, const float* a_scale,
                             const float* a_shift, int relu, float drop_p, uint32_t drop_seed, float* dz,
                             int64_t lddz, float* dgamma, float* dbeta, float* dz_col_sum, float* workspace,
                             int64_t workspace_floats, void* stream);

/* nn.LayerNorm(hidden) as a hidden-layer tail (reference models.py:28-31, 87-90, 174-186; train.conf.yaml uses norm_type
 * "layer" for the house_class MLP):
 *   forward   y = dropout(relu?(xhat * gamma + beta)),  xhat = (z - mean_row) * rstd_row,  rstd = 1/sqrt(biased var + eps);
 *             mean_out / rstd_out [rows] (optional) are what the backward needs; gamma/beta NULL = no affine.  y may be NULL when
 *             mean_out and rstd_out are given: the statistics alone (the SAGE LayerNorm step applies the tail in the next gather).
 *   backward  dy = da * keep/(1-p) * [relu ? xhat*gamma+beta > 0 : 1];  dgamma = sum_rows dy*xhat, dbeta = sum_rows dy;
 *             dz = rstd * (dy*gamma - mean_cols(dy*gamma) - xhat * mean_cols(dy*gamma*xhat));  dz_col_sum (optional) = sum_rows dz
 *             = the bias gradient of the Linear in front.  workspace >= glnn_layernorm_bwd_workspace_floats(rows, h) floats when
 *             any column sum is requested; h <= 4096.  In place on da allowed (dz == da).
 * Rows are float4 rows (leading dimensions % 4 == 0, >= round4(h), 16-byte aligned); padding columns of y / dz = 0. */
GLNN_API int glnn_layernorm_fwd_f32(const float* z, int64_t ldz, int64_t rows, int h, const float* gamma,
                                    const float* beta, float eps, int relu, float drop_p, uint32_t drop_seed,
                                    float* y, int64_t ldy, float* mean_out, float* rstd_out, void* stream);
GLNN_API int64_t glnn_layernorm_bwd_workspace_floats(int64_t rows, int h);
GLNN_API int glnn_layernorm_bwd_f32(const float* da, int64_t ldda, const float* z, int64_t ldz, int64_t rows, int h,
                                    const float* gamma, const float* beta, const float* mean, const float* rstd,
                                    int relu, float drop_p, uint32_t drop_seed, float* dz, int64_t lddz,
                                    float* dgamma, float* dbeta, float* dz_col_sum, float* workspace,
                                    int64_t workspace_floats, void* stream);

/* The dropout keep-mask the kernels above evaluate on the fly (nn.Dropout, reference models.py:52):
 * mask[r*h + c] = 1 if element (r,c) is kept under (drop_p, drop_seed).  torch's Philox stream cannot
 * be reproduced by a custom kernel, so parity tests run the oracle with THIS mask as an input. */
GLNN_API int glnn_dropout_mask_u8(int64_t rows, int h, float drop_p, uint32_t drop_seed,
                                  uint8_t* mask, void* stream);

/* Uniform in-neighbour sampling WITHOUT replacement for a list of seed (destination) rows: at most `fanout`
 * sources per seed, all of them when in_deg <= fanout (dgl semantics).  Replaces the CPU-side
 * dgl.dataloading.MultiLayerNeighborSampler of reference train_and_eval.py:179-190 (one call per layer).
 * out_src [n_seeds, fanout] int32 global source ids (first out_cnt[i] entries of row i valid). */
GLNN_API int glnn_sample_neighbors(const int64_t* indptr, const int32_t* indices, const int64_t* seeds,
                                   int64_t n_seeds, int fanout, uint32_t rng_seed, int32_t* out_src,
                                   int32_t* out_cnt, void* stream);

/* The sampled neighbourhood of ALL n_dst rows of a resident CSR as a CSR of its own (csrc/sample_csr.hip;
 * docs/SAMPLED_INFERENCE_SEMANTICS.md): what SAGE.inference(fan_out=...) aggregates over.  Entries added, none changed.
 *
 * glnn_sample_csr_indptr: out_indptr [n_dst + 1] = exclusive prefix sum of min(deg(v), fanout) -- it depends on the graph and the
 *   fan-out only, never on a seed; integer work, the same bits on every run.  One call, no host synchronisation.
 *   workspace: glnn_sample_csr_workspace_bytes(n_dst) bytes, 8-byte aligned (not read when n_dst == 0).
 * glnn_sample_csr_fill: out_indices [out_indptr[n_dst]] int32, with out_indptr from the call above under the SAME fanout.  Row v holds
 *   exactly what glnn_sample_neighbors gives seed-list position i = v of seeds = arange(n_dst): a row of at most `fanout` entries
 *   is copied in row order; a longer one gets indices[indptr[v] + picked[s]] in slot s, with Floyd's picks: for s = 0 .. fanout-1,
 *   j = deg - fanout + s, t = ((uint64_t)drop_hash(rng_seed, v, s) * (j + 1)) >> 32, picked[s] = j if t was picked before, else t.
 *   The draw is keyed by the global row id v: a row's picks do not depend on which other rows are in the launch.
 * Both: fanout in [1, 64], n_dst and n_src below 2^31, no null pointer -- else GLNN_ERR_INVALID_ARG with nothing launched and a
 * glnn_last_error text that names the entry; n_dst == 0 is GLNN_OK. */
GLNN_API int64_t glnn_sample_csr_workspace_bytes(int64_t n_dst);
GLNN_API int glnn_sample_csr_indptr(const int64_t* indptr, int64_t n_dst, int fanout, int64_t* out_indptr, void* workspace,
                                    int64_t workspace_bytes, void* stream);
GLNN_API int glnn_sample_csr_fill(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src,
                                  const int64_t* out_indptr, int fanout, uint32_t rng_seed, int32_t* out_indices, void* stream);

/* ------------------------------------------------------------------------------------------
 * Block construction for mini-batch teacher training / chunked inference: what dgl.dataloading.NodeDataLoader does on
 * the CPU per batch in the reference (train_and_eval.py:176-205; blocks consumed at :41 and models.py:109,134-137),
 * here on the device and sized by the batch's FRONTIER (hash table + two single-pass scans), never by N.
 *   seeds [ns]        the block's destination nodes (global ids)
 *   sampled mode      smp_src [ns, fanout] / smp_cnt [ns] from glnn_sample_neighbors, nnz_cap >= ns * fanout
 *   full mode         smp_src = smp_cnt = NULL: every in-edge of every seed from (g_indptr, g_indices);
 *                     nnz_cap >= the block's edge count (the caller's bound; counts[0] reports the true number: when it
 *                     exceeds nnz_cap the capacity was too small -- nothing was written at or past it, call again with more)
 *   nnz_cap == 0      the caller asserts an EMPTY block: no row is read, whatever in-edges the seeds have -- indptr is all
 *                     zeros, input_nodes = seeds, counts = {0, ns}
 * Outputs (caller-owned): indptr [ns+1]; indices [nnz_cap] LOCAL source ids (block CSR over its destinations, edges in
 * the order of smp_src / of the graph's rows); gindices [nnz_cap] the same edges' GLOBAL source ids (optional);
 * input_nodes [ns + nnz_cap]: the block's source nodes = its destinations first (models.py:109), then every other
 * source in order of first appearance; counts (device int64[2]) = {nnz, number of source nodes}.
 * workspace: glnn_block_workspace_bytes(ns, nnz_cap) bytes, 8-byte aligned.  Node ids must be < 0x7F7F7F7F.
 * GLOBAL-ID BLOCK (round 5): indices == NULL and input_nodes == NULL with gindices != NULL -- only indptr and the edges' global source ids
 * are produced (row-count scan + one copy pass; no table, no relabelling), counts = {nnz, -1}: the outermost block of a training batch,
 * whose consumer (glnn_sage_fwd_bwd_f32 with self_rows) gathers from the global feature matrix and never reads local ids. */
GLNN_API int64_t glnn_block_workspace_bytes(int64_t ns, int64_t nnz_cap);
GLNN_API int glnn_block_build(const int64_t* g_indptr, const int32_t* g_indices, const int64_t* seeds,
                              int64_t ns, const int32_t* smp_src, const int32_t* smp_cnt, int fanout,
                              int64_t nnz_cap, int64_t* indptr, int32_t* indices, int32_t* gindices,
                              int64_t* input_nodes, int64_t* counts, void* workspace,
                              int64_t workspace_bytes, void* stream);
/* ABI 8: the same, told the size of the id universe (every seed and neighbour id is < n_nodes; 0 = unknown -> glnn_block_build).
 * When n_nodes is no larger than the two arrays of the frontier hash table (the wider blocks of a large batch), the positions are indexed by
 * the node id itself: one atomicMin per edge, no probing, a smaller fill.  Same workspace size, identical results.  Precondition: every id is in
 * [0, n_nodes); an id outside is never used as an index -- counts[0] comes back as -1 (the block's outputs are then undefined). */
GLNN_API int glnn_block_build_ids(const int64_t* g_indptr, const int32_t* g_indices, const int64_t* seeds,
                                  int64_t ns, const int32_t* smp_src, const int32_t* smp_cnt, int fanout,
                                  int64_t nnz_cap, int64_t* indptr, int32_t* indices, int32_t* gindices,
                                  int64_t* input_nodes, int64_t* counts, int64_t n_nodes, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* Transposed CSR (rows = the original SOURCE nodes, entries = destinations, sorted within a row): the graph
 * loss.backward() walks through dgl's SpMM in the reference (train_and_eval.py:27,54) -- A^T dY is then the same
 * glnn_spmm_csr_f32 gather on the result, deterministic, no float atomics:
 *     d/dx of SUM(row_scale, col_scale)  =  SUM over the transposed CSR with row_scale <-> col_scale swapped;
 *     d/dx of SAGE_GCN                   =  SUM over the transposed CSR built with add_self != 0 (one extra entry u <- u
 *                                           for every destination u < n_dst: the h_dst term) and col_scale = 1/(deg+1).
 * t_indptr [n_src+1], t_indices [nnz + (add_self ? n_dst : 0)]; nnz = indptr[n_dst] (host value);
 * workspace: glnn_csr_transpose_workspace_bytes(n_src, nnz + (add_self ? n_dst : 0)) bytes, 8-byte aligned. */
GLNN_API int64_t glnn_csr_transpose_workspace_bytes(int64_t n_src, int64_t nnz_out);
GLNN_API int glnn_csr_transpose(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src,
                                int64_t nnz, int add_self, int64_t* t_indptr, int32_t* t_indices,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mini-batches for the full-graph teachers: random-walk node sampling and the induced subgraph of the visited nodes, both sized by
 * the batch and never by N or E (docs/SUBGRAPH_SEMANTICS.md).  GraphSAINT's random-walk sampler (Zeng et al., ICLR 2020) without its
 * normalisation coefficients.
 *
 * glnn_random_walk: out [n_roots, length + 1] int64 global ids, column 0 = roots[i].  Step s (1-based) of walk i, standing on v with
 * deg = indptr[v+1] - indptr[v]: deg == 0 -> the walk stays on v; else it moves to
 *     indices[indptr[v] + (((uint64_t)drop_hash(rng_seed, i, s) * deg) >> 32)]
 * (the draw of glnn_sample_neighbors; drop_hash is restated by oracle/dropout_mask.py).  The CSR is stored by destination, so a step
 * follows an IN-edge: v has the in-edge u -> v inside the induced subgraph.  1 <= length <= 64.  Every root must be in [0, n_nodes). */
GLNN_API int glnn_random_walk(const int64_t* indptr, const int32_t* indices, const int64_t* roots, int64_t n_roots, int length,
                              uint32_t rng_seed, int64_t* out, void* stream);

/* glnn_induced_subgraph: the subgraph of (g_indptr, g_indices) induced by the DISTINCT ids of cand [nc] (int64 global ids in
 * [0, n_nodes), repeats allowed).  Outputs (caller-owned):
 *   nodes   [nc]       the distinct candidates in order of first appearance = local id -> global id (first n_sub entries valid)
 *   indptr  [nc + 1]   (first n_sub + 1 entries valid)
 *   indices [nnz_cap]  int32 LOCAL ids: row k holds the in-edges u -> nodes[k] of the graph whose u is in the set, in the order of the
 *                      graph's own row, multi-edges kept
 *   counts  device int64[3] = {n_sub, nnz, rows without an entry}
 * self_loop 0 ("keep"): exactly that -- for candidates without repeats, CSRGraph.subgraph(cand) array for array.
 * self_loop 1 ("add"): self entries are dropped and one k <- k is appended at the end of every row, so no row is empty.
 * SIZING: the caller supplies the capacity nnz_cap of `indices` (the sum of the candidates' in-degrees, + nc with "add", always
 * suffices); counts[1] reports the TRUE number of entries.  counts[1] > nnz_cap: the capacity was too small -- nothing was written past
 * it, `indices` is incomplete.  An id outside [0, n_nodes) is never used as an index: counts[0] comes back as -1 (the other outputs are
 * then undefined, and in bounds).
 * Work and workspace are proportional to nc plus the in-degrees of the candidates.  Integer arithmetic only; "first appearance" comes from
 * atomicMin on list positions and the entry order from ballot ranks, so the same input gives the same bits.  One wave walks a row, 64
 * in-edges per round, whatever its length.
 * workspace: glnn_induced_subgraph_workspace_bytes(nc, n_nodes) bytes, 8-byte aligned.  nc < 2^30, nnz_cap < 2^31, n_nodes < 0x7F7F7F7F.
 * glnn_induced_subgraph_direct: 1 when that build indexes its table by the node id itself (n_nodes no larger than the two arrays of
 * the hash table, 2 x (the power of two >= 2 nc, at least 64)), 0 when it probes an open-addressing table.  Identical results. */
GLNN_API int glnn_induced_subgraph_direct(int64_t nc, int64_t n_nodes);
GLNN_API int64_t glnn_induced_subgraph_workspace_bytes(int64_t nc, int64_t n_nodes);
GLNN_API int glnn_induced_subgraph(const int64_t* g_indptr, const int32_t* g_indices, int64_t n_nodes, const int64_t* cand, int64_t nc,
                                   int self_loop, int64_t nnz_cap, int64_t* nodes, int64_t* indptr, int32_t* indices,
                                   int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * APPNP propagation (dgl APPNPConv(k, alpha, edge_drop) of the reference APPNP teacher, models.py:282-344): K launches of ONE power
 * iteration each, forward and backward, ping-ponging two buffers.  docs/APPNP_SEMANTICS.md states the arithmetic.  Square graph of n nodes,
 * indptr / indices the in-CSR (rows = destinations); dst_norm / src_norm = in_deg.clamp(1)^-1/2 / out_deg.clamp(1)^-1/2 (glnn_degrees_f32,
 * GLNN_DEG_RSQRT_CLAMP1).  Edge mask of step t (1-based): keep edge e iff glnn_edge_drop_mask_u8(t, edge_drop, seed)[e], weight
 * 1 / (1 - edge_drop); edge_drop = 0 disables it.  nnz = indptr[n] < 2^31.  Deterministic (no float atomics).
 *
 * Forward step t:  h_t[i] = (1 - alpha) dst_norm[i] sum_{kept e = (j -> i)} w * xs[j]  +  alpha h0[i],   xs[j] = x_norm[j] x[j] when
 *   x_norm != NULL (t = 1: x = h0, x_norm = src_norm), else x[j] (x = the previous step's output, already scaled).
 *   out[i] = src_norm_out[i] h_t[i] when src_norm_out != NULL (t < K: the next step's pre-scaled input), else h_t[i] (t = K). */
GLNN_API int glnn_appnp_prop_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* x,
                                 int64_t ldx, int d, const float* x_norm, const float* dst_norm, const float* src_norm_out,
                                 const float* h0, int64_t ldh0, float alpha, float edge_drop, uint32_t seed, int t, float* out,
                                 int64_t ldo, void* stream);
/* Backward step t (called for t = K .. 1) over the transposed CSR with the original edge ids (glnn_csr_transpose_eids):
 *   g_{t-1}[j] = (1 - alpha) src_norm[j] sum_{kept e = (j -> i)} w * xs[i],  xs = x_norm * x when x_norm != NULL (first step, t = K:
 *   x = g_K = dL/dh_K unscaled, x_norm = dst_norm), else x (the previous step's output q_t = dst_norm * g_t).
 *   first != 0 (t = K): the running sum starts at alpha g_K[j] (read from x); otherwise it is read from acc.
 *   t > 1: acc[j] += alpha g_{t-1}[j], out[j] = dst_norm_out[j] g_{t-1}[j];   t = 1: out[j] = g_0[j] + acc = dL/dh0 (acc not written).
 *   acc may be NULL when K = 1 (first and t = 1). */
GLNN_API int glnn_appnp_prop_bwd_f32(const int64_t* t_indptr, const int32_t* t_indices, const int32_t* t_eids, int64_t n,
                                     int64_t nnz, const float* x, int64_t ldx, int d, const float* x_norm, const float* src_norm,
                                     const float* dst_norm_out, float alpha, float edge_drop, uint32_t seed, int t, int first,
                                     float* acc, int64_t ldacc, float* out, int64_t ldo, void* stream);
/* glnn_csr_transpose (add_self = 0) plus t_eids [nnz]: the original edge id (CSR position) of every transposed entry; parallel edges keep
 * ascending edge ids.  t_indptr / t_indices are exactly glnn_csr_transpose's.  Workspace as glnn_csr_transpose.
 * GLNN_ERR_UNSUPPORTED for nnz >= 2^31. */
GLNN_API int glnn_csr_transpose_eids(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src,
                                     int64_t nnz, int64_t* t_indptr, int32_t* t_indices, int32_t* t_eids,
                                     void* workspace, int64_t workspace_bytes, void* stream);
/* The APPNP edge keep-mask the propagation kernels evaluate on the fly: mask[e] = 1 iff edge e is kept in step t (t >= 1) under
 * (edge_drop, seed) -- the role glnn_dropout_mask_u8 plays for the feature dropout (parity tests feed it to the oracle). */
GLNN_API int glnn_edge_drop_mask_u8(int64_t nnz, int t, float edge_drop, uint32_t seed, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * DeepWalk position embeddings for the MLP student (Perozzi et al., KDD 2014; used as in NOSMOG, Tian et al., ICLR 2023): one skip-gram
 * step with negative sampling over ONE table z [n_nodes, d] and batch-synchronous lazy Adam.  docs/POSITION_SEMANTICS.md states the
 * arithmetic.  fp32, contiguous rows (leading dimension d), d % 4 == 0, 4 <= d <= 256, 16-byte aligned.  L = length in [1, 64], c = context
 * in [2, L + 1], k = negatives >= 1; nwin = L + 2 - c windows per walk, Q = n_roots nwin windows, R = (1 + k)(c - 1) entries per window;
 * Q R < 2^31 and n_nodes < 2^31.  Any of these violated: GLNN_ERR_INVALID_ARG with nothing launched.  No float atomics; the same input
 * gives the same bits.  A step is glnn_deepwalk_pairs, glnn_deepwalk_score_f32, glnn_csr_transpose(win_indptr, start, Q, n_nodes, Q),
 * glnn_csr_transpose_eids(pair_indptr, rest, Q, n_nodes, Q R), glnn_deepwalk_apply_f32.
 *
 * glnn_deepwalk_pairs: walks [n_roots, L + 1] = glnn_random_walk(roots, L, walk_seed) (called from here), then for window q = i nwin + j:
 *   start[q] = walks[i, j];  rest[q R + t] = walks[i, j + 1 + t] for t < c - 1 (the positives), else the uniform negative
 *   ((uint64_t)drop_hash(neg_seed, q, t - (c - 1)) * n_nodes) >> 32 (kept even where it equals the start or a positive);
 *   pair_indptr[q] = q R and win_indptr[q] = q for q <= Q: the indptr arrays of the two CSRs the transposes read.
 *   roots_host (optional): a host copy of roots; every entry is checked against [0, n_nodes) before anything is launched.  NULL: every
 *   root must be a node id, as glnn_random_walk expects. */
GLNN_API int glnn_deepwalk_pairs(const int64_t* indptr, const int32_t* indices, int64_t n_nodes, const int64_t* roots,
                                 const int64_t* roots_host, int64_t n_roots, int length, int context, int negatives,
                                 uint32_t walk_seed, uint32_t neg_seed, int64_t* walks, int32_t* start, int32_t* rest,
                                 int64_t* pair_indptr, int64_t* win_indptr, void* stream);
/* glnn_deepwalk_score_f32, at frozen z, with s = <z[start[q]], z[rest[q R + t]]>, n_pos = Q (c - 1), n_neg = k n_pos:
 *   g[q R + t] = (sigmoid(s) - 1) / n_pos for a positive, sigmoid(s) / n_neg for a negative;
 *   gs[q] = sum_t g[q R + t] z[rest[q R + t]] (t ascending per lane group, the groups folded by an xor tree);  zs[q] = z[start[q]];
 *   loss_parts[q] = sum over the positives of softplus(-s), loss_parts[Q + q] = sum over the negatives of softplus(s).
 * g [Q R], gs / zs [Q, d], loss_parts [2 Q].  An id outside [0, n_nodes) in start / rest is never used as an index (g = 0 there). */
GLNN_API int glnn_deepwalk_score_f32(const float* z, int64_t n_nodes, int d, const int32_t* start, const int32_t* rest,
                                     int64_t n_windows, int context, int negatives, float* g, float* gs, float* zs,
                                     float* loss_parts, void* stream);
/* glnn_deepwalk_apply_f32: (tw_indptr, tw_indices) = glnn_csr_transpose of (win_indptr, start): per node its windows;
 * (tp_indptr, tp_eids) = t_indptr and t_eids of glnn_csr_transpose_eids of (pair_indptr, rest): per node the pair-list positions at which
 * it is the entry, ascending.  For every node n with a window or an entry:
 *   dz = sum over its windows of gs[q]  +  sum over its positions e of g[e] zs[e / R]      (each list in its stored order, then the two)
 *   m <- beta1 m + (1 - beta1) dz;  v <- beta2 v + (1 - beta2) dz^2;  z <- z - lr sqrt(1 - beta2^step) / (1 - beta1^step) m / (sqrt(v) + eps)
 * in place (torch.optim.SparseAdam's arithmetic, no weight decay; step >= 1 is the global step count; the hyper-parameters are doubles, as
 * there: the bias corrections are formed in double and the step size, beta, 1 - beta and eps rounded to fp32 once).  Every other row of z, m, v is
 * not written.  A node of more than 128 entries is summed by a whole workgroup, the wave partials added in wave order.
 * loss_out (device float) = sum(loss_parts[0 .. Q)) / n_pos + sum(loss_parts[Q .. 2 Q)) / n_neg, summed in fp64 in a fixed order by one
 * more workgroup of the same launch. */
GLNN_API int glnn_deepwalk_apply_f32(const int64_t* tw_indptr, const int32_t* tw_indices, const int64_t* tp_indptr,
                                     const int32_t* tp_eids, int64_t n_nodes, int d, int64_t n_windows, int context, int negatives,
                                     const float* g, const float* gs, const float* zs, float* z, float* m, float* v, double lr,
                                     double beta1, double beta2, double eps, int64_t step, const float* loss_parts, float* loss_out,
                                     void* stream);

/* The rest of the node2vec family (same ABI: entries added, none changed; docs/POSITION_SEMANTICS.md).
 *
 * glnn_node2vec_walk: glnn_random_walk's output with the second-order bias of node2vec (Grover, Leskovec, KDD 2016).  Step 1 is
 * glnn_random_walk's.  At step s >= 2, standing on v with t = out[i, s - 2], a candidate x of row v is a RETURN (x == t, tested first,
 * weight 1/p), NEAR (x is an entry of row t; weight 1) or FAR (weight 1/q).  With wmax = max(1/p, 1, 1/q) and
 * T_class = min(2^32, floor(w_class / wmax * 2^32)) formed in double, attempt a = 0, 1, ... draws
 *     x = indices[indptr[v] + (((uint64_t)drop_hash(rng_seed, i, s + 128 a) * deg) >> 32)]
 * and accepts it iff (uint64_t)drop_hash(rng_seed ^ 0x4E32564B, i, s + 128 a) < T_class(x); after 256 rejected attempts the 256th
 * candidate is taken (probability <= (15/16)^256 < 7e-8 per step).  p = q = 1 accepts attempt 0 everywhere: glnn_random_walk's bits.
 * p, q in [0.25, 4]; 1 <= length <= 64.  roots_host (optional): a host copy of roots, checked against [0, n_nodes) before the launch. */
GLNN_API int glnn_node2vec_walk(const int64_t* indptr, const int32_t* indices, int64_t n_nodes, const int64_t* roots,
                                const int64_t* roots_host, int64_t n_roots, int length, double p, double q, uint32_t rng_seed,
                                int64_t* out, void* stream);
/* glnn_deepwalk_pairs_from_walks: glnn_deepwalk_pairs' four outputs from walks [n_roots, L + 1] that are an INPUT.  neg_cdf NULL: the
 * uniform negative of glnn_deepwalk_pairs.  neg_cdf [n_nodes] (device, ascending 32-bit CDF): with r = drop_hash(neg_seed, q, t') the
 * negative is the number of n in [0, n_nodes - 1) with neg_cdf[n] <= r (an upper-bound binary search over the first n_nodes - 1 entries:
 * in [0, n_nodes - 1] whatever the table holds). */
GLNN_API int glnn_deepwalk_pairs_from_walks(const int64_t* walks, int64_t n_roots, int length, int context, int negatives,
                                            int64_t n_nodes, uint32_t neg_seed, const uint32_t* neg_cdf, int32_t* start, int32_t* rest,
                                            int64_t* pair_indptr, int64_t* win_indptr, void* stream);
/* glnn_deepwalk_score_ctx_f32: glnn_deepwalk_score_f32 with the entries read from a second table, s = <z[start[q]], c[rest[q R + t]]>,
 * gs[q] = sum_t g c[rest]; zs[q] = z[start[q]] as before.  c == z: glnn_deepwalk_score_f32's bits.  The two-table update is two
 * glnn_deepwalk_apply_f32 calls: on (z, m_z, v_z) with the windows list and an EMPTY positions CSR (all-zero tp_indptr), and on
 * (c, m_c, v_c) with an empty windows CSR and the positions list. */
GLNN_API int glnn_deepwalk_score_ctx_f32(const float* z, const float* c, int64_t n_nodes, int d, const int32_t* start,
                                         const int32_t* rest, int64_t n_windows, int context, int negatives, float* g, float* gs,
                                         float* zs, float* loss_parts, void* stream);

/* ------------------------------------------------------------------------------------------
 * GPR-GNN propagation (Chien et al., ICLR 2021): result = sum_{k = 0..K} gamma[k] P^k x0 with K + 1 learned coefficients and APPNP's
 * operator P = D_in^-1/2 A D_out^-1/2.  docs/GPR_SEMANTICS.md states the arithmetic.  ONE entry serves both directions, one call per
 * step k = 1..K (k = 0 alone when K = 0); square graph of n nodes, nnz = indptr[n] < 2^31 (GLNN_ERR_UNSUPPORTED otherwise), no edge
 * dropout.  Deterministic (no float atomics).
 *   forward:   indptr / indices = the in-CSR,          x_norm = src_norm, row_norm = dst_norm, out_norm = src_norm, x0 = h0
 *   backward:  indptr / indices = glnn_csr_transpose,  x_norm = dst_norm, row_norm = src_norm, out_norm = dst_norm, x0 = dL/dresult
 *
 * Step k >= 1:  row[i] = row_norm[i] sum_{e = (j -> i)} xs[j],  xs[j] = x_norm[j] x[j] at k = 1 (x = x0 unscaled; x_norm required), else
 *   x[j] (x = the previous call's `out`, already scaled; x_norm must be NULL).
 *     acc[i] = (k = 1 ? gamma[0] x[i] : acc[i]) + gamma[k] row[i]        -- after step K, acc is the result
 *     out[i] = out_norm[i] row[i]                                          -- out may be NULL (step K: the row is not needed again)
 *   h0 / row_dot (both or neither; the backward): row_dot[(k T + c) n + i] = sum over the columns of 256-column tile c of row[i] h0[i],
 *     T = ceil(d / 256), and at k = 1 also row_dot[c n + i] from x; row_dot holds (K + 1) T n floats.
 * k = 0 (K = 0, no propagation launch, the graph arguments are ignored): acc = gamma[0] x, row_dot[c n + i] as above.
 * gamma [K + 1] is read on the device.  Padding columns [d, ld) of acc and out are written as 0.  acc and out alias no input. */
GLNN_API int glnn_gpr_prop_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* x, int64_t ldx,
                               int d, const float* x_norm, const float* row_norm, const float* out_norm, const float* gamma, int k,
                               float* acc, int64_t ldacc, float* out, int64_t ldo, const float* h0, int64_t ldh0, float* row_dot,
                               void* stream);
/* dgamma[r] = sum of row_dot[r m .. r m + m) for r < rows (rows = K + 1, m = T n), accumulated in fp64 in a geometry that depends on m
 * alone: stage 1 sums chunks of GLNN_GPR_FOLD_CHUNK entries (thread t of 256 takes entries t, t + 256, ...; xor tree over the lanes, the
 * four waves in order), stage 2 sums the chunk partials the same way.  workspace: rows * ceil(m / GLNN_GPR_FOLD_CHUNK) * 8 bytes, 8-byte
 * aligned.  m = 0 writes zeros. */
#define GLNN_GPR_FOLD_CHUNK 4096
GLNN_API int glnn_gpr_fold_f32(const float* row_dot, int rows, int64_t m, float* dgamma, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * DAGNN's gate (Liu, Gao, Ji, "Towards Deeper Graph Neural Networks", KDD 2020): result[i] = sum_{k = 0..K} s_k[i] H_k[i] with
 * H_0 = x0, H_k = P H_{k-1}, APPNP's operator P = D_in^-1/2 A D_out^-1/2 and the node-adaptive gate s_k[i] = sigmoid(<H_k[i], w> + b),
 * evaluated as 1 / (1 + expf(-(dot + b))).  docs/DAGNN_SEMANTICS.md states the arithmetic.  The propagation itself is glnn_spmm_csr_f32
 * (GLNN_AGG_SUM with row_scale / col_scale = the two degree norms); these entries are row-local.  n rows of d <= 256 columns (the gate is
 * one row-wide dot product; GLNN_ERR_UNSUPPORTED otherwise, nothing launched); every row pointer 16-byte aligned with a leading dimension
 * % 4 == 0 and >= round4(d); padding columns [d, round4(d)) of every written row are 0.  w [d] and b [1] are read on the device on every
 * call.  Deterministic (no float atomics); a row's dot products are folded over its lanes in a fixed xor order.  n == 0 is a no-op.
 *
 * glnn_dagnn_gate_f32 -- hop k of the forward, one call per k = 0..K, x = H_k:
 *     s = sigmoid(<x[i], w> + b);   acc[i] = (k == 0 ? 0 : acc[i]) + s x[i];   score[k n + i] = s  (score optional, [(K + 1) n]: training)
 *   After hop K, acc is the result.  acc does not alias x.
 *
 * glnn_dagnn_gate_bwd_f32 -- hop k of the backward, one call per k = K..0:
 *     q      = <g[i], h[i]> s (1 - s),  s = score[k n + i]       g = dL/dresult, h = the saved H_k
 *     out[i] = s g[i] + q w + t[i]                               t = P^T (the previous call's out), NULL at k = K; t may be out itself
 *     q_out[k n + i] = q                                         q_out holds (K + 1) n floats
 *   After k = 0, out = dL/dx0.  out aliases neither g nor h.
 *
 * glnn_dagnn_fold_f32 -- dw[c] = sum_r q[r] hs[r, c], db[0] = sum_r q[r] over the rows = (K + 1) n rows of the saved stack hs [rows, ldh],
 *   accumulated in fp64 in a geometry that depends on (rows, d) alone: stage 1 sums chunks of GLNN_DAGNN_FOLD_CHUNK rows (LPR = pow2 >=
 *   ceil(d / 4) lanes a row, 256 / LPR row groups taking the chunk's rows g, g + 256 / LPR, ... ascending, the groups added in order), stage
 *   2 the chunk partials (thread t of 256 takes chunks t, t + 256, ...; xor tree over the lanes, the four waves in order); one rounding to
 *   fp32.  workspace: glnn_dagnn_fold_workspace_bytes(rows, d) = ceil(rows / GLNN_DAGNN_FOLD_CHUNK) * (d + 1) * 8 bytes, 8-byte aligned.
 *   rows = 0 writes zeros. */
GLNN_API int glnn_dagnn_gate_f32(const float* x, int64_t ldx, int64_t n, int d, const float* w, const float* b, int k, float* acc,
                                 int64_t ldacc, float* score, void* stream);
GLNN_API int glnn_dagnn_gate_bwd_f32(const float* g, int64_t ldg, const float* h, int64_t ldh, int64_t n, int d, const float* score,
                                     const float* w, int k, const float* t, int64_t ldt, float* out, int64_t ldo, float* q_out,
                                     void* stream);
#define GLNN_DAGNN_FOLD_CHUNK 2048
GLNN_API int64_t glnn_dagnn_fold_workspace_bytes(int64_t rows, int d);
GLNN_API int glnn_dagnn_fold_f32(const float* hs, int64_t ldh, const float* q, int64_t rows, int d, float* dw, float* db,
                                 void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GCNII conv layer (Chen, Wei, Huang, Ding, Li, "Simple and Deep Graph Convolutional Networks", ICML 2020), one launch per layer and
 * direction over APPNP's operator P = D_in^-1/2 A D_out^-1/2.  docs/GCNII_SEMANTICS.md states the arithmetic.  Square graph of n nodes,
 * nnz = indptr[n] < 2^31 and d <= 256 (GLNN_ERR_UNSUPPORTED otherwise); every row pointer 16-byte aligned with a leading dimension
 * % 4 == 0 and >= round4(d); padding columns [d, round4(d)) of every output are written as 0.  Deterministic (no float atomics), and
 * independent of tile_order (optional: an int32 permutation of the ceil(n / 32) row tiles).  n == 0 is a no-op.
 *
 * glnn_gcnii_layer_f32 -- the paper's eq. (5), section 3 (initial residual + identity mapping), forward:
 *     S[i]   = (1 - alpha) row_norm[i] sum_{e = (j -> i)} xs[j] + alpha h0[i],   xs[j] = x_norm[j] drop(x)[j] (x_norm NULL: x is already
 *              scaled by it);  drop = the package's feature dropout under (drop_p, drop_seed), keyed by the SOURCE row and the column
 *              (glnn_dropout_mask_u8(n, d, ...)[j]), drop_p = 0: none
 *     out[i] = out_norm[i] relu((1 - beta) S[i] + beta S[i] W^T)      (out_norm NULL: unscaled);  w_packed = glnn_pack_weight_f32 of W [d, d]
 *     s_out (optional) = S, what the weight gradient is taken against. */
GLNN_API int glnn_gcnii_layer_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* x, int64_t ldx,
                                  int d, const float* x_norm, const float* row_norm, const float* out_norm, const float* h0,
                                  int64_t ldh0, float alpha, float beta, const float* w_packed, float drop_p, uint32_t drop_seed,
                                  float* s_out, int64_t lds, float* out, int64_t ldo, const int32_t* tile_order, void* stream);
/* glnn_gcnii_layer_bwd_f32 -- the backward of eq. (5), section 3, over glnn_csr_transpose of the graph (norms swapped):
 *     T[i]  = plain ? g[i] : (1 - alpha) row_norm[i] sum_{e} x_norm[j] g[j]      (g = the previous call's ds_out, or dL/dH_L when plain)
 *     dZ[i] = [h[i] > 0] drop'(T)[i]        drop' = the mask of (drop_p, drop_seed) keyed by the OWN row i;  h = the saved H_l
 *     dz_out = dz_scale dZ                  (dz_scale = beta_l: dW_l = dz_out^T S_l)
 *     dS[i] = (1 - beta) dZ[i] + beta dZ[i] W,   wt_packed = glnn_pack_weight_f32 of W^T;   ds_out[i] = out_norm[i] dS[i] (NULL: unscaled)
 *     dh0_acc[i] = (first ? 0 : dh0_acc[i]) + alpha dS[i]
 *   wt_packed == NULL and ds_out == NULL (the launch behind layer 1; gather form, first == 0, h optional):
 *     dz_out[i] = drop'(T)[i] + dh0_acc[i] = dL/dH_0 (h NULL; with h given the mask covers the sum: [h[i] > 0] (drop'(T)[i] + dh0_acc[i]));
 *     dh0_acc is only read. */
GLNN_API int glnn_gcnii_layer_bwd_f32(const int64_t* t_indptr, const int32_t* t_indices, int64_t n, int64_t nnz, const float* g,
                                      int64_t ldg, int d, const float* x_norm, const float* row_norm, const float* out_norm, int plain,
                                      const float* h, int64_t ldh, float drop_p, uint32_t drop_seed, float alpha, float beta,
                                      const float* wt_packed, float dz_scale, float* dz_out, int64_t lddz, float* ds_out, int64_t ldds,
                                      float* dh0_acc, int64_t ldacc, int first, const int32_t* tile_order, void* stream);

/* ------------------------------------------------------------------------------------------
 * GAT attention (dgl 0.6.1 GATConv of the reference GAT teacher, models.py:202-279): per-destination edge softmax with per-edge scores
 * from two per-node scalars per head.  docs/GAT_SEMANTICS.md states the arithmetic.  Square graph of n nodes, indptr / indices the in-CSR
 * (rows = destinations, edge id = CSR position); z [n, heads * out_feats] the projected rows, head-major columns.  heads <= 64,
 * heads * out_feats <= 256, nnz < 2^31.  Attention dropout: edge e, head h kept iff glnn_gat_attn_mask_u8(...)[e * heads + h], weight
 * 1 / (1 - attn_drop), applied AFTER the normalisation; attn_drop = 0 disables it.  Deterministic (no float atomics).
 *
 * glnn_gat_scores_f32: el[r, h] = <z[r, h, :], attn_l[h, :]>, er likewise with attn_r, from one read of z.  z2 != NULL: z -= z2 first
 *   (stored back into z): the two half-products of a signed input behind the feature dropout. */
GLNN_API int glnn_gat_scores_f32(float* z, int64_t ldz, const float* z2, int64_t ldz2, int64_t n, int heads, int out_feats,
                                 const float* attn_l, const float* attn_r, float* el, float* er, void* stream);
/* out[i] = act( sum_{e = (j -> i)} a_ij w_ij z[j] ),  a_ij = softmax over ALL in-edges of i of leaky_relu(el[j] + er[i], negative_slope)
 *   per head, w_ij the dropout weight; relu != 0: ReLU epilogue.  lse (optional, [n, heads]): max + log(denominator) of every row and
 *   head, what the backward recomputes a_ij from.  A row without in-edges gives zeros. */
GLNN_API int glnn_gat_attn_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* z, int64_t ldz,
                                   int heads, int out_feats, const float* el, const float* er, float negative_slope, float attn_drop,
                                   uint32_t seed, int relu, float* out, int64_t ldo, float* lse, void* stream);
/* Backward of glnn_gat_attn_fwd_f32 + glnn_gat_scores_f32 with respect to z, attn_l and attn_r.  g = dL/d out behind the activation
 * mask.  y = the forward's stored output: still required and checked like g, but not read (D_i = <g_i, out_i> is formed per head as
 * sum_k a_ik c_ik / sum_k a_ik from the row's own c_ik = w_ik <g_i, z_k>, in fp64).  Pass 1 (in-CSR, two sweeps): ds [nnz, heads] scratch and der [n, heads];
 * pass 2 (transposed CSR with original edge ids, glnn_csr_transpose_eids): dz [n, heads * out_feats] and del [n, heads]; then
 * dattn_l = sum_j del_j z_j, dattn_r = sum_i der_i z_i through per-workgroup partials in `workspace`
 * (>= glnn_gat_attn_bwd_workspace_floats floats), folded in fixed order. */
GLNN_API int64_t glnn_gat_attn_bwd_workspace_floats(int64_t n, int heads, int out_feats);
GLNN_API int glnn_gat_attn_bwd_f32(const int64_t* indptr, const int32_t* indices, const int64_t* t_indptr, const int32_t* t_indices,
                                   const int32_t* t_eids, int64_t n, int64_t nnz, const float* z, int64_t ldz, int heads, int out_feats,
                                   const float* el, const float* er, const float* lse, const float* attn_l, const float* attn_r,
                                   const float* g, int64_t ldg, const float* y, int64_t ldy, float negative_slope, float attn_drop,
                                   uint32_t seed, float* ds, float* der, float* del_, float* dz, int64_t lddz, float* dattn_l,
                                   float* dattn_r, float* workspace, int64_t workspace_floats, void* stream);
/* The attention keep-mask the GAT kernels evaluate on the fly: mask[e * heads + h] = 1 iff head h of edge e is kept under
 * (attn_drop, seed) -- the role glnn_edge_drop_mask_u8 plays for APPNP (parity tests feed it to the oracle). */
GLNN_API int glnn_gat_attn_mask_u8(int64_t nnz, int heads, float attn_drop, uint32_t seed, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * GATv2 attention (Brody, Alon, Yahav, ICLR 2022; csrc/gatv2.hip; docs/GATV2_SEMANTICS.md states the arithmetic): per-destination edge
 * softmax whose score needs the whole projected source row.  Square graph of n nodes, indptr / indices the in-CSR (rows = destinations,
 * edge id = CSR position); zl / zr [n, heads * out_feats] the two projections (fc_src / fc_dst), head-major columns; attn
 * [heads * out_feats].  heads <= 64, heads * out_feats <= 256, nnz < 2^31 (GLNN_ERR_UNSUPPORTED otherwise, nothing launched); every row
 * pointer 16-byte aligned with a leading dimension % 4 == 0 and >= round4(heads * out_feats).  Attention dropout: the mask of
 * glnn_gat_attn_mask_u8, weight 1 / (1 - attn_drop), applied AFTER the normalisation (the denominator sums every edge).  No float
 * atomics, no grid barrier: bit-identical run to run.  n == 0 is a no-op.
 *
 * out[i] = act( sum_{e = (j -> i)} a_ij w_ij zl[j] ),  a_ij = softmax over ALL in-edges of i of
 *   s_ij[h] = sum_f attn[h, f] leaky_relu(zl[j, h, f] + zr[i, h, f], negative_slope); ONE gather of zl[j] per edge, online softmax in a
 *   fixed edge order.  relu != 0: ReLU epilogue.  lse (optional, [n, heads]): max + log(denominator), what the backward recomputes a_ij
 *   from.  Padding columns of out are written as zeros; a row without in-edges gives zeros. */
GLNN_API int glnn_gatv2_attn_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* zl, int64_t ldzl,
                                     const float* zr, int64_t ldzr, int heads, int out_feats, const float* attn, float negative_slope,
                                     float attn_drop, uint32_t seed, int relu, float* out, int64_t ldo, float* lse, void* stream);
/* Backward of glnn_gatv2_attn_fwd_f32 with respect to zl, zr and attn.  g = dL/d out behind the activation mask.  Pass 1 (in-CSR, two
 * sweeps, each gathering zl[j]): D_i = sum_k a_ik c_ik / sum_k a_ik in fp64 from the row's own c_ik = w_ik <g_i, zl_k>, then
 * ds [nnz, heads] scratch (ds_ij = a_ij (c_ij - D_i)), dzr [n, heads * out_feats] and per-workgroup partials of dattn in `workspace`
 * (>= glnn_gatv2_attn_bwd_workspace_floats floats); pass 2 (transposed CSR with original edge ids, glnn_csr_transpose_eids): dzl; then
 * dattn [heads * out_feats] folded from the partials in ascending order. */
GLNN_API int64_t glnn_gatv2_attn_bwd_workspace_floats(int64_t n, int heads, int out_feats);
GLNN_API int glnn_gatv2_attn_bwd_f32(const int64_t* indptr, const int32_t* indices, const int64_t* t_indptr, const int32_t* t_indices,
                                     const int32_t* t_eids, int64_t n, int64_t nnz, const float* zl, int64_t ldzl, const float* zr,
                                     int64_t ldzr, int heads, int out_feats, const float* lse, const float* attn, const float* g,
                                     int64_t ldg, float negative_slope, float attn_drop, uint32_t seed, float* ds, float* dzl,
                                     int64_t lddzl, float* dzr, int64_t lddzr, float* dattn, float* workspace, int64_t workspace_floats,
                                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Graph-transformer attention (the TransformerConv of UniMP, Shi et al., IJCAI 2021, without label embedding, beta gate and edge
 * features; csrc/gt.hip; docs/GT_SEMANTICS.md states the arithmetic): per-destination scaled dot-product edge softmax with a skip row.
 * Square graph of n nodes, indptr / indices the in-CSR (rows = destinations, edge id = CSR position); q / k / v / skip
 * [n, heads * out_feats] the four projections, head-major columns, each a pointer and a leading dimension of its own (separate matrices
 * or column slabs of one stacked projection).  heads <= 64, heads * out_feats <= 256, nnz < 2^31 (GLNN_ERR_UNSUPPORTED otherwise,
 * nothing launched); every row pointer 16-byte aligned with a leading dimension % 4 == 0 and >= round4(heads * out_feats).  Attention
 * dropout: the mask of glnn_gat_attn_mask_u8, weight 1 / (1 - attn_drop), applied AFTER the normalisation (the denominator sums every
 * edge).  No float atomics, no grid barrier: bit-identical run to run.  n == 0 is a no-op.
 *
 * out[i] = act( sum_{e = (j -> i)} a_ij w_ij v[j] + skip[i] ),  a_ij = softmax over ALL in-edges of i of
 *   e_ij[h] = <q[i, h, :], k[j, h, :]> / sqrt(out_feats); k[j] and v[j] are gathered once per edge, online softmax in a fixed edge order.
 *   relu != 0: ReLU epilogue.  lse (optional, [n, heads]): max + log(denominator), what the backward recomputes a_ij from (0 for a row
 *   without in-edges).  Padding columns of out are written as zeros; a row without in-edges gives its skip row. */
GLNN_API int glnn_gt_attn_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* q, int64_t ldq,
                                  const float* k, int64_t ldk, const float* v, int64_t ldv, const float* skip, int64_t ldskip, int heads,
                                  int out_feats, float attn_drop, uint32_t seed, int relu, float* out, int64_t ldo, float* lse,
                                  void* stream);
/* Backward of glnn_gt_attn_fwd_f32 with respect to q, k and v (the gradient of skip is g itself).  g = dL/d out behind the activation
 * mask.  Pass 1 (in-CSR, two sweeps, each gathering k[j] and v[j]): D_i = sum_k a_ik c_ik / sum_k a_ik in fp64 from the row's own
 * c_ik = w_ik <g_i, v_k>, then t [nnz, heads] scratch (t_ij = a_ij (c_ij - D_i)), a_ij w_ij [nnz, heads] in `workspace`
 * (>= glnn_gt_attn_bwd_workspace_floats floats) and dq_i = sum_j t_ij k_j / sqrt(out_feats); pass 2 (transposed CSR with original edge
 * ids, glnn_csr_transpose_eids): dk_j = sum_i t_ij q_i / sqrt(out_feats) and dv_j = sum_i a_ij w_ij g_i from the two scratches, with no
 * score recomputed.  A row without in-edges gets dq = 0.  dq, dk, dv: [n, heads * out_feats], padding columns written as zeros. */
GLNN_API int64_t glnn_gt_attn_bwd_workspace_floats(int64_t nnz, int heads);
GLNN_API int glnn_gt_attn_bwd_f32(const int64_t* indptr, const int32_t* indices, const int64_t* t_indptr, const int32_t* t_indices,
                                  const int32_t* t_eids, int64_t n, int64_t nnz, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                  const float* v, int64_t ldv, int heads, int out_feats, const float* lse, const float* g, int64_t ldg,
                                  float attn_drop, uint32_t seed, float* t, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv,
                                  int64_t lddv, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * PNA, Principal Neighbourhood Aggregation (Corso, Cavalleri, Beaini, Lio, Velickovic, NeurIPS 2020; csrc/pna.hip;
 * docs/PNA_SEMANTICS.md states the arithmetic): the mean, min, max and std of the rows b[u] over the in-edges u -> v of a CSR by
 * destination, from ONE gather of every neighbour row.  Rows of d <= GLNN_PNA_MAX_WIDTH floats (GLNN_ERR_UNSUPPORTED otherwise, nothing
 * launched), nnz and the node counts below 2^31; every row pointer 16-byte aligned with a leading dimension % 4 == 0.  dp = round4(d).
 * Deterministic: no float atomics, a row's result does not depend on the other rows of the launch.
 *
 * glnn_pna_agg_fwd_f32 -- s[v] = [a[v] + mean | a[v] + min | a[v] + max | std] in four parts of dp floats (lds >= 4 dp), padding
 *   columns [d, dp) of every part zero; a optional (NULL: no own term); std = sqrt(max(E b^2 - mean^2, 0) + 1e-5) from fp64 sums.  A row
 *   without in-edges gets [0 | 0 | 0 | sqrt(1e-5)] and no a term.  mu and arg (both or neither: training) take the plain mean [n_dst, dp]
 *   and arg[v] = [argmin | argmax] in two parts of dp int32 (ldarg >= 2 dp): the CSR position of the FIRST edge that attains the value,
 *   -1 for a row without in-edges and in the padding.  A NaN never wins a comparison.  n_dst == 0 is a no-op.
 *
 * glnn_pna_agg_bwd_f32 -- the source pass over the transposed CSR with edge ids (glnn_csr_transpose_eids of the forward's CSR; indptr =
 *   the FORWARD's row pointers, read for deg(v)).  With ds[v] = [g_mean | g_min | g_max | g_std] (ldds >= 4 dp), sigma = the std part of
 *   the forward's s (its own leading dimension):
 *     db[u] = sum_{e = (u -> v)} g_mean[v] / deg(v) + g_std[v] (b[u] - mu[v]) / (deg(v) sigma[v]) + [argmax[v] == e] g_max[v]
 *                                + [argmin[v] == e] g_min[v]
 *   in transposed-CSR order, one wave per source row.  Every row of db [n_src, dp] is written; a row no edge references gets zeros.
 *
 * The row-local pieces (fop = round4(fo)); s_amp(v) = log(max(deg(v), 1) + 1) / delta, s_att(v) = 1 / s_amp(v), delta > 0:
 *   glnn_pna_scale_fwd_f32   out[v] = act(out[v] + z_0[v] + s_amp z_1[v] + s_att z_2[v]), z = [z_0 | z_1 | z_2] in parts of fop floats
 *                            (ldz >= 3 fop), in place on out (ldo >= fop; padding columns zero); relu != 0: act = ReLU
 *   glnn_pna_scale_bwd_f32   dz[v] = [g[v] | s_amp g[v] | s_att g[v]]  (lddz >= 3 fop, padding zero)
 *   glnn_pna_da_f32          da[v] = g_mean[v] + g_min[v] + g_max[v] for deg(v) > 0, else 0  (ldda >= dp, padding zero) */
#define GLNN_PNA_MAX_WIDTH 256
GLNN_API int glnn_pna_agg_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, int64_t nnz, const float* b,
                                  int64_t ldb, int d, const float* a, int64_t lda, float* s, int64_t lds, float* mu, int64_t ldmu,
                                  int32_t* arg, int64_t ldarg, void* stream);
GLNN_API int glnn_pna_agg_bwd_f32(const int64_t* indptr, int64_t n_dst, const int64_t* t_indptr, const int32_t* t_indices,
                                  const int32_t* t_eids, int64_t n_src, int64_t nnz, const float* ds, int64_t ldds, const float* b,
                                  int64_t ldb, int d, const float* mu, int64_t ldmu, const float* sigma, int64_t ldsig, const int32_t* arg,
                                  int64_t ldarg, float* db, int64_t lddb, void* stream);
GLNN_API int glnn_pna_scale_fwd_f32(const int64_t* indptr, int64_t n, int fo, float delta, const float* z, int64_t ldz, float* out,
                                    int64_t ldo, int relu, void* stream);
GLNN_API int glnn_pna_scale_bwd_f32(const int64_t* indptr, int64_t n, int fo, float delta, const float* g, int64_t ldg, float* dz,
                                    int64_t lddz, void* stream);
GLNN_API int glnn_pna_da_f32(const int64_t* indptr, int64_t n, int d, const float* ds, int64_t ldds, float* da, int64_t ldda, void* stream);

/* ------------------------------------------------------------------------------------------
 * GraphSAGE "mean" aggregator (csrc/sage_mean.hip; docs/SAGE_MEAN_SEMANTICS.md states the arithmetic):
 *   h_neigh[v] = (1 / max(deg(v), 1)) * sum_{u->v} x[u]        out[v] = fc_neigh(h_neigh[v]) + fc_self(x_self[v])
 * Both entries: CSR over destination rows as glnn_spmm_csr_f32, n_src < 2^31, float4-addressable rows (leading dimensions multiples of 4
 * and >= the width rounded up to 4, 16-byte aligned bases), epi(t) = relu?(t * ep_scale[j] + ep_shift[j]) with NULL = 1 / 0.  No float
 * atomics, no grid barrier: bit-identical run to run, and a row's result does not depend on the other rows of the launch.  A shape
 * outside the stated contract returns GLNN_ERR_UNSUPPORTED with nothing launched.  n_dst == 0 is a no-op.
 *
 * glnn_sage_mean_fused_f32 replaces dgl 0.6.1 SAGEConv(in, out, "mean").forward of an aggregate-first layer (the reference has no call
 *   site: it only builds "gcn") in ONE launch, d_in <= d_out <= 256:  out = epi([h_neigh | x_self] . W_cat^T), one fp32 MFMA product over
 *   K = 2 kpad, kpad = d_in rounded up to 8.  w_cat_packed = glnn_pack_weight_f32 of the [d_out, 2 kpad] matrix whose columns [0, d_in) are
 *   fc_neigh.weight, [kpad, kpad + d_in) fc_self.weight and the rest zeros.  self_rows (optional, int64 [n_dst]): the self row of
 *   destination v is x_self[self_rows[v]], else x_self[v].  tile_order (optional): a permutation of the ceil(n_dst / 32) tile ids (same
 *   bits).  out: ldo >= d_out; columns [d_out, min(d_out rounded up to 4, ldo)) are written as 0. */
GLNN_API int glnn_sage_mean_fused_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const float* x,
                                      int64_t ldx, int d_in, const float* x_self, int64_t ld_self, const int64_t* self_rows,
                                      const float* w_cat_packed, int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                      float* out, int64_t ldo, const int32_t* tile_order, void* stream);
/* glnn_spmm_sage_mean_f32 replaces the aggregation half of dgl 0.6.1 SAGEConv(in, out, "mean").forward when the layer projects first
 *   (in > out; the reference has no call site), and is the general fallback:  out[v, :d] = epi(h_neigh[v, :d] + s[v, :d]),  d <= 256.
 *   After ONE product of the source rows against the stacked [W_neigh; W_self], x is the first half of that matrix and s the second half
 *   of the same rows (own pointer and leading dimension).  out: columns [d, d rounded up to 4) are written as 0. */
GLNN_API int glnn_spmm_sage_mean_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const float* x,
                                     int64_t ldx, int d, const float* s, int64_t lds, const float* ep_scale, const float* ep_shift,
                                     int relu, float* out, int64_t ldo, void* stream);

/* K7  row gather: out[i,:] = x[rows[i],:]  (feats[idx], reference train_and_eval.py:42,76,
 *     models.py:136) and scatter y[rows[i],:] = x[i,:] (models.py:145). */
GLNN_API int glnn_gather_rows_f32(const float* x, int64_t ldx, const int64_t* rows, int64_t n_rows,
                                  int d, float* out, int64_t ldo, void* stream);
GLNN_API int glnn_scatter_rows_f32(const float* x, int64_t ldx, const int64_t* rows, int64_t n_rows,
                                   int d, float* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16 activation storage for the whole-graph SAGE teacher forward (csrc/sage_bf16.hip).  A matrix that an aggregation gathers may be
 * STORED as bf16 (uint16_t bit patterns, torch.bfloat16); every sum, MFMA and epilogue stays fp32 and values are rounded to bf16 only
 * when stored: round to nearest even, NaN -> 0x7FC0 (torch's Tensor.to(torch.bfloat16)).  bf16 matrices need a leading dimension that is a
 * multiple of 8 elements and a 16-byte aligned base (a lane moves 8 bf16); columns [d, ld) are padding, written as 0 by these kernels.
 * An fp32 output keeps the fp32 conventions above (ld a multiple of 4).  Results are deterministic (fixed-order folds, no float atomics)
 * but not bit-equal to the fp32 entries run on the widened rows: a wave splits a row's edges over twice as many lane groups.
 * ------------------------------------------------------------------------------------------ */
#define GLNN_DTYPE_F32 0
#define GLNN_DTYPE_BF16 1

/* out[i, j] = bf16(x[i, j]) for j < d, 0 for the padding columns d <= j < d rounded up to 8 (columns beyond are not touched).
 * ldx >= d (any), ldo a multiple of 8 and >= d. */
GLNN_API int glnn_cast_f32_bf16(const float* x, int64_t ldx, int64_t n, int d, uint16_t* out, int64_t ldo,
                                void* stream);

/* glnn_spmm_csr_f32 over bf16 rows x / x_self (ldx, ld_self multiples of 8 and >= d rounded up to 8), both modes, the same epilogue;
 * `out` holds fp32 (out_dtype GLNN_DTYPE_F32, ldo a multiple of 4) or bf16 (GLNN_DTYPE_BF16, ldo a multiple of 8).  Rows wider than
 * 256 elements are processed in column tiles of 256 within one launch.  No hub plan / chunk variants. */
GLNN_API int glnn_spmm_csr_bf16(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                int64_t n_src, const uint16_t* x, int64_t ldx, int d, int mode,
                                const float* row_scale, const float* col_scale,
                                const uint16_t* x_self, int64_t ld_self, const int64_t* self_rows,
                                const float* ep_scale, const float* ep_shift, int relu, void* out,
                                int64_t ldo, int out_dtype, void* stream);

/* glnn_sage_fused_f32 over bf16 rows x / x_self: the fp32 aggregate of the 32-row tile in LDS feeds the same fp32 MFMA
 * (v_mfma_f32_32x32x2_f32) passes; `out` and the chained `out2` are each stored fp32 or bf16 (out_dtype / out2_dtype, GLNN_DTYPE_*).
 * The chained pass reads the fp32 hidden row, never its rounded copy. */
GLNN_API int glnn_sage_fused_bf16(const int64_t* indptr, const int32_t* indices, int64_t n_dst,
                                  int64_t n_src, const uint16_t* x, int64_t ldx, int d_in,
                                  const uint16_t* x_self, int64_t ld_self, const float* w_packed,
                                  int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                  void* out, int64_t ldo, int out_dtype, const float* w2_packed, int d_out2,
                                  void* out2, int64_t ldo2, int out2_dtype, const int32_t* tile_order, void* stream);

/* ------------------------------------------------------------------------------------------
 * int8 activation storage for the whole-graph SAGE teacher forward (csrc/sage_i8.hip, docs/INT8_INFERENCE_SEMANTICS.md).  A matrix that an
 * aggregation gathers may be STORED as int8 rows with one fp32 scale per row; every sum, MFMA and epilogue stays fp32, weights stay fp32.
 *
 * Row format.  A matrix of n rows by d columns (1 <= d <= 256) is an int8 array [n, ld] with ld = round16(d + 4) bytes EXACTLY and a
 * 16-byte aligned base:
 *   bytes [0, d)         the quantised values q in [-127, 127] (signed)
 *   bytes [d, ld - 4)    zero
 *   bytes [ld - 4, ld)   the row's fp32 scale s, little endian
 * and the value of an element is q * s (the scale sits in the row: one contiguous fetch brings everything an edge needs).
 * Quantisation of a row x, all in fp32: amax = max |x|; s = amax / 127.0f and inv = 127.0f / amax, both correctly rounded divisions;
 * q = min(max(rintf(x * inv), -127), 127), ties to even.  amax == 0: s = 0 and q = 0.  A row holding a NaN or an Inf: s = NaN (0x7FC00000)
 * and q = 0, so the whole row dequantises to NaN.
 * Every entry: n == 0 / n_dst == 0 is a no-op; d > 256 or a leading dimension of int8 rows other than round16(d + 4) is
 * GLNN_ERR_UNSUPPORTED, any other bad argument GLNN_ERR_INVALID_ARG, both with nothing launched and a glnn_last_error text that names the
 * entry.  Results are deterministic (fixed-order folds, no float atomics).
 * ------------------------------------------------------------------------------------------ */
#define GLNN_DTYPE_I8 2

/* x fp32 [n, d] (ldx >= d, any) -> int8 rows `out` (ldo = round16(d + 4)), padding written as 0. */
GLNN_API int glnn_quant_rows_i8(const float* x, int64_t ldx, int64_t n, int d, int8_t* out, int64_t ldo, void* stream);

/* out[v] = epi((sum_{u->v} x[u] + x_self[v]) / (deg(v) + 1)) over int8 rows x [n_src] / x_self [n_dst] (ldx = ld_self = round16(d + 4)),
 * the corrected division and the epilogue epi(z) = relu?(z * ep_scale + ep_shift) of glnn_spmm_csr_f32.  `out` holds fp32 (out_dtype
 * GLNN_DTYPE_F32, ldo a multiple of 4) or int8 rows (GLNN_DTYPE_I8, ldo = round16(d + 4): the lanes that hold a finished row reduce its
 * amax among themselves and quantise before storing).  No row_scale / col_scale / self_rows / hub / chunk variant. */
GLNN_API int glnn_spmm_sage_gcn_i8(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src,
                                   const int8_t* x, int64_t ldx, int d, const int8_t* x_self, int64_t ld_self,
                                   const float* ep_scale, const float* ep_shift, int relu, void* out, int64_t ldo,
                                   int out_dtype, void* stream);

/* glnn_sage_fused_bf16 with phase A reading int8 rows x / x_self (d_in <= 256): the fp32 aggregate of the 32-row tile in LDS feeds the
 * same fp32 MFMA passes; tile_order and the chained w2_packed / out2 as there.  Both outputs are fp32 (a chained projection that the next
 * layer gathers is quantised by glnn_quant_rows_i8). */
GLNN_API int glnn_sage_fused_i8(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src,
                                const int8_t* x, int64_t ldx, int d_in, const int8_t* x_self, int64_t ld_self,
                                const float* w_packed, int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                float* out, int64_t ldo, const float* w2_packed, int d_out2, float* out2, int64_t ldo2,
                                const int32_t* tile_order, void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16 serving of the MLP student (csrc/gemm_bf16.hip): opt-in inference with weights and hidden activations STORED as bf16, every
 * product on the bf16 MFMA (v_mfma_f32_16x16x32_bf16) with fp32 accumulation in a fixed order, an fp32 epilogue, fp32 logits.
 *   out[m, n] = epi( A[m, k] . W[n, k]^T ),  epi(v) = relu?( v * ep_scale[n] + ep_shift[n] ),  then optionally log_softmax of each row.
 * A: bf16 [m, lda] (a_dtype GLNN_DTYPE_BF16: lda a multiple of 8, 16-byte aligned; whatever sits in columns [k, lda) is ignored) or fp32
 *    [m, lda] (GLNN_DTYPE_F32, any lda >= k), rounded to bf16 as glnn_cast_f32_bf16 rounds while it is staged.
 * W: bf16 [n, ldw], ldw a multiple of 64 and >= k, 16-byte aligned, ZEROS in columns [k, ldw) (glnn_cast_f32_bf16 into a zeroed buffer).
 * out: bf16 (ldo a multiple of 8, columns [n, n rounded up to 8) written as 0) or fp32 (any ldo >= n).  ep_scale / ep_shift may be NULL
 *    (1 / 0).  log_softmax (n <= 64, fp32 out): `out` receives log-probabilities (max, expf sum, subtract); the logits are not stored.
 * No split-K, no float atomics: bit-equal run to run, a row's result does not depend on the other rows of the call, and the fp32-A and
 * bf16-A forms of one call agree bit for bit.  m == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
GLNN_API int glnn_gemm_bf16(const void* a, int64_t lda, int a_dtype, int64_t m, int k, const uint16_t* w, int64_t ldw,
                            int n, const float* ep_scale, const float* ep_shift, int relu, void* out, int64_t ldo,
                            int out_dtype, int log_softmax, void* stream);

/* The eval-mode chain of a student (norm "none" or BatchNorm folded into ep_scale / ep_shift; ReLU behind every layer but the last). */
typedef struct glnn_mlp_serve_desc {        /* glnn_struct_bytes(7) */
  int32_t num_layers;                       /* 1 .. GLNN_MLP_MAX_LAYERS */
  int32_t reserved;
  int32_t dims[GLNN_MLP_MAX_LAYERS + 1];    /* dims[l] -> dims[l + 1] is layer l */
  int32_t reserved2;
  const uint16_t* w[GLNN_MLP_MAX_LAYERS];   /* bf16 [dims[l + 1], ldw[l]], see glnn_gemm_bf16 */
  int64_t ldw[GLNN_MLP_MAX_LAYERS];
  const float* ep_scale[GLNN_MLP_MAX_LAYERS];   /* fp32 [dims[l + 1]] or NULL */
  const float* ep_shift[GLNN_MLP_MAX_LAYERS];
} glnn_mlp_serve_desc;

/* logits (or log-probabilities: log_softmax, dims[num_layers] <= 64) of x [m, dims[0]] (x_dtype as a_dtype above) into fp32 out [m, ldo]:
 * num_layers glnn_gemm_bf16 launches on `stream`.  Hidden rows ping-pong between the caller's bf16 buffers buf0 / buf1, each [m, ld_buf]
 * (ld_buf a multiple of 8 and >= every hidden width; buf1 may be NULL for <= 2 layers, both for 1).  Never allocates or synchronises. */
GLNN_API int glnn_mlp_forward_bf16(const glnn_mlp_serve_desc* desc, const void* x, int64_t ldx, int x_dtype, int64_t m,
                                   uint16_t* buf0, uint16_t* buf1, int64_t ld_buf, float* out, int64_t ldo,
                                   int log_softmax, void* stream);

/* The one-launch form of that chain (csrc/mlp_fused_bf16.hip): a workgroup owns a tile of consecutive batch rows and carries it through
 * every layer, the hidden rows as bf16 images in LDS, the weights streamed from the same packed operands.  Every accumulator sees k in
 * the chain's order and every rounding point is the chain's, so the result equals glnn_mlp_forward_bf16's BIT FOR BIT (default MFMA form).
 * Taken: every chain whose hidden and output widths are <= 512 (tiles of 64 rows) and, where the device's LDS holds two 32 x 1024 images
 * plus the 32 KB weight stage (160 KB: gfx950), widths <= 1024 (tiles of 32 rows); dims[0] is arbitrary. */

/* rows per workgroup the fused launch would use for this chain (> 0), or 0 when it does not take it (glnn_last_error says why) */
GLNN_API int glnn_mlp_fused_bf16_tile_rows(const glnn_mlp_serve_desc* desc);

/* glnn_mlp_forward_bf16 as ONE launch, no hidden buffers.  rows == NULL: batch row b is x[b].  Otherwise rows is an int64 device
 * vector of m indices into the n_x rows of x: batch row b is x[rows[b]]; an index outside [0, n_x) is never used as an address,
 * that batch row is computed from an all-zero input row.  Arguments are checked as glnn_mlp_forward_bf16 checks them
 * (GLNN_ERR_INVALID_ARG); m == 0 is a no-op that reads no pointer.  GLNN_ERR_UNSUPPORTED with nothing launched: a hidden or output
 * width above 1024, a tile that does not fit the device's LDS, GLNN_GEMM_BF16_MFMA16=0 in force.  Never allocates or synchronises. */
GLNN_API int glnn_mlp_forward_fused_bf16(const glnn_mlp_serve_desc* desc, const void* x, int64_t ldx, int x_dtype,
                                         const int64_t* rows, int64_t n_x, int64_t m, float* out, int64_t ldo,
                                         int log_softmax, void* stream);

/* ------------------------------------------------------------------------------------------
 * Serving a position-feature student by node id (csrc/position_serve.hip; docs/POSITION_SEMANTICS.md, "Serving by node id"): the
 * student's input rows for a batch of node ids, assembled from the features, the position table and the graph in ONE launch; nothing of
 * size n_nodes is built.  For b < m, v = ids[b]:
 *   out[b, 0:f]     = x[v, 0:f]     x fp32 [n_nodes, ldx] (any ldx >= f) or bf16 (ldx % 8 == 0, 16-byte aligned); fp32 -> fp32, bf16 -> bf16 copy
 *                                   the bits, fp32 -> bf16 rounds as glnn_cast_f32_bf16; bf16 -> fp32 is GLNN_ERR_UNSUPPORTED
 *   out[b, f:f + d] = pos(v)        rounded the same way for a bf16 output.  slot [n_nodes]: node -> row of the fp32 table z [z_rows, ldz]
 *                                   (d % 4 == 0, 4 <= d <= 256, ldz % 4 == 0, 16-byte aligned), a value outside [0, z_rows) = not embedded.
 *                                   Embedded: pos(v) = z[slot[v]].  Otherwise the mean, sum / (float)count in fp32, of z[slot[u]] over the
 *                                   stored entries u of row v of the in-edge CSR (indptr, indices over n_nodes rows) that are embedded -- a
 *                                   multi-edge counts as often as it is stored, an entry outside [0, n_nodes) is skipped -- and exact
 *                                   zeros without one.  indptr == indices == NULL: no id of the batch is unseen (a row that is gets zeros).
 *   out[b, f + d : round(f + d)]    = 0, round = up to a multiple of 4 (fp32 out) or 8 (bf16 out); ldo a multiple of that and >= it, out
 *                                   16-byte aligned.  Columns beyond and rows >= m are not touched.
 * The ids must be node ids (the callers check them); one outside [0, n_nodes) is never used as an index (its row is zeros).  One wave
 * per batch row; an unseen row of more than 128 entries is summed by a whole workgroup, the wave partials added in wave order.  No float
 * atomics: a row's bits depend neither on its position in the batch nor on the other ids.  n_nodes, z_rows < 2^31.  m == 0 is a no-op
 * that reads no pointer; a refused argument is GLNN_ERR_INVALID_ARG with nothing launched. */
GLNN_API int glnn_position_rows(const int64_t* ids, int64_t m, const void* x, int64_t ldx, int x_dtype, int f, const float* z,
                                int64_t ldz, int d, int64_t z_rows, const int32_t* slot, int64_t n_nodes, const int64_t* indptr,
                                const int32_t* indices, void* out, int64_t ldo, int out_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GLNN_HIP_H */
