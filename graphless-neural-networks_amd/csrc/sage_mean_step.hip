// The sampled-block training step of the GraphSAGE "mean" teacher for gfx950 (MI355X) -- docs/SAGE_MEAN_SEMANTICS.md; the "gcn" step's
// launch sequence (csrc/sage_step.hip) with the two aggregations that step cannot express, issued from C++ for the same reason: the step
// is host-bound when its launches come from Python.
//
//   z_l = [mean_l | self_l] [W_neigh | W_self]^T + (b_neigh + b_self)        mean_l[v] = (1 / max(deg v, 1)) sum_{u->v} h_l[u],  self_l[v] = h_l[v]
//
//   sage_mean_cat_kernel   forward aggregation: per destination row the operand pair [mean | self] in ONE buffer of leading dimension
//     2 round4(d_in) (second half at the float4-aligned column round4(d_in); padding columns written as zeros).  Sources: plain local rows,
//     the global feature matrix through global ids + self_rows (outermost block), or pre-activations z of the hidden layer in front with
//     its tail (BatchNorm affine / LayerNorm -> ReLU -> dropout, the counter-based mask keyed by the ACTIVATION's row and column) applied
//     to every gathered row and to the self row -- tail_apply of source_tail_dev.h, so the step is bit-identical to the materialised-h form.
//   sage_mean_bwd_kernel   backward aggregation over the PLAIN transposed block (glnn_csr_transpose, add_self = 0):
//     dh[u] = sum_{v: u->v} inv(v) dcat[v, :d] + (u < n_dst ? dcat[u, off : off + d] : 0),  inv(v) from the forward block's indptr.
//     Every source row is written -- a row no edge references gets exact zeros (+ its self term).
//   pack_pair_kernel       W_cat = [W_neigh | W_self] ([d_out, 2 round4(d_in)], zero padding) and b_neigh + b_self, re-packed every step
//     because the parameters change every step.
//
// Both aggregations run row_gather_dev.h's 32-row tile.  No float atomics, no grid barrier: bit-identical run to run.  Rows wider than 256
// floats are cut into 256-column slabs (blockIdx.y).
// The projections, weight gradients, loss, tails and Adam are the library's existing launches.
#include "row_gather_dev.h"
#include "source_tail_dev.h"
#include "step_common.h"

namespace {

constexpr int kMaxTailD = 256;     // widest hidden layer whose tail the gather evaluates (the limit of glnn::spmm_csr_tail)

struct CatArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const float* x; int64_t ldx; int d;                       // the gathered rows (plain rows, or pre-activations z with `tail`)
  const int64_t* self_rows;                                 // outermost block with global ids: the self row of v is x[self_rows[v]]
  const float* t_scale; const float* t_shift; const float* t_mean; const float* t_rstd; uint32_t t_thr, t_seed; float t_dscale;
  float* cat; int64_t ld_cat;                               // [n_dst, 2 round4(d)]
};

template <int XF>
struct CatLoad : GatherPolicy {
  const float* x; int64_t ldx; int col4; bool col_ok; TailCols tc;
  __device__ __forceinline__ float4 row(int src, float, bool ok) const {
    return (ok && col_ok) ? tail_apply<XF>(tc, ld4(x + (int64_t)src * ldx + col4), (uint32_t)src) : zero4();
  }
};

template <int LPR, int XF>
__global__ __launch_bounds__(kBlock) void sage_mean_cat_kernel(const CatArgs a) {
  __shared__ float4 s_part[4 * 64];
  __shared__ int s_next;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = ((int)blockIdx.y * LPR + lane % LPR) * 4;
  const int dpad = (a.d + 3) & ~3;
  const bool col_ok = col4 < dpad;
  CatLoad<XF> ld;
  ld.x = a.x; ld.ldx = a.ldx; ld.col4 = col4; ld.col_ok = col_ok;
  TailCols& tc = ld.tc;
  if (XF) tc = load_tail_cols(a.t_scale, a.t_shift, a.t_mean, a.t_rstd, a.t_thr, a.t_seed, a.t_dscale, a.d, col4, XF);
  if (threadIdx.x == 0) s_next = 0;
  __syncthreads();
  gather_tile<LPR>(a.indptr, a.indices, a.n_dst, (int64_t)blockIdx.x * kTileRows, lane, wave, &s_next, s_part, ld,
                   [&](int, int64_t v, int64_t deg, float4 sum, bool valid) {
                     if (!valid || lane >= LPR || !col_ok) return;
                     const float inv = 1.0f / (float)(deg > 1 ? deg : 1);      // one IEEE division per row
                     const float4 m = mask_cols(make_float4(sum.x * inv, sum.y * inv, sum.z * inv, sum.w * inv), col4, a.d);
                     const int64_t sr = a.self_rows ? a.self_rows[v] : v;
                     const float4 s = mask_cols(tail_apply<XF>(tc, ld4(a.x + sr * a.ldx + col4), (uint32_t)v), col4, a.d);
                     st4(a.cat + v * a.ld_cat + col4, m);
                     st4(a.cat + v * a.ld_cat + dpad + col4, s);
                   });
}

struct BwdArgs {
  const int64_t* t_indptr; const int32_t* t_indices; int64_t n_src;      // the plain transposed block: a row per SOURCE, entries = destinations
  const int64_t* indptr; int64_t n_dst;                                  // the forward block: inv(v) = 1 / max(indptr[v + 1] - indptr[v], 1)
  const float* dcat; int64_t ld_dcat; int d;                             // [n_dst, 2 round4(d)]: dmean | dself
  float* dh; int64_t ld_dh;                                              // [n_src, >= round4(d)]
};

// each gathered row times inv(v): the product is rounded, then added
struct BwdLoad : GatherPolicy {
  static constexpr bool kWeighted = true;
  const float* dcat; int64_t ld; const int64_t* indptr; int col4; bool col_ok;
  __device__ __forceinline__ float weight(int v, bool ok) const {
    if (!ok) return 0.f;
    const int64_t deg = indptr[v + 1] - indptr[v];
    return 1.0f / (float)(deg > 1 ? deg : 1);
  }
  __device__ __forceinline__ float4 row(int v, float w, bool ok) const {
    if (!ok || !col_ok) return zero4();
    const float4 t = ld4(dcat + (int64_t)v * ld + col4);
    return make_float4(t.x * w, t.y * w, t.z * w, t.w * w);
  }
};

template <int LPR>
__global__ __launch_bounds__(kBlock) void sage_mean_bwd_kernel(const BwdArgs a) {
  __shared__ float4 s_part[4 * 64];
  __shared__ int s_next;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = ((int)blockIdx.y * LPR + lane % LPR) * 4;
  const int dpad = (a.d + 3) & ~3;
  const bool col_ok = col4 < dpad;
  BwdLoad ld;
  ld.dcat = a.dcat; ld.ld = a.ld_dcat; ld.indptr = a.indptr; ld.col4 = col4; ld.col_ok = col_ok;
  if (threadIdx.x == 0) s_next = 0;
  __syncthreads();
  gather_tile<LPR>(a.t_indptr, a.t_indices, a.n_src, (int64_t)blockIdx.x * kTileRows, lane, wave, &s_next, s_part, ld,
                   [&](int, int64_t u, int64_t, float4 sum, bool valid) {
                     if (!valid || lane >= LPR || !col_ok) return;
                     if (u < a.n_dst) sum = add4(sum, ld4(a.dcat + u * a.ld_dcat + dpad + col4));
                     st4(a.dh + u * a.ld_dh + col4, mask_cols(sum, col4, a.d));
                   });
}

struct PackLayer { const float* wn; const float* ws; const float* bn; const float* bs; float* wcat; float* bsum; int d_in, d_out; };
struct PackArgs { PackLayer layer[GLNN_SAGE_MAX_LAYERS]; };

__global__ __launch_bounds__(256) void pack_pair_kernel(const PackArgs a) {
  const PackLayer& y = a.layer[blockIdx.y];
  const int dpad = (y.d_in + 3) & ~3;
  const int64_t total = (int64_t)y.d_out * 2 * dpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(i / (2 * dpad));
    const int c = (int)(i - (int64_t)o * 2 * dpad);
    const int cc = c < dpad ? c : c - dpad;
    const float* w = c < dpad ? y.wn : y.ws;
    y.wcat[i] = cc < y.d_in ? w[(int64_t)o * y.d_in + cc] : 0.f;
    if (c == 0) y.bsum[o] = y.bn[o] + y.bs[o];
  }
}

template <int XF>
int launch_cat(const CatArgs& a, hipStream_t st) {
  const int dv = ((a.d + 3) & ~3) / 4;
  const dim3 grid((unsigned)((a.n_dst + kTileRows - 1) / kTileRows), (unsigned)((dv + 63) / 64));
  with_lpr<16>(lpr_for(dv, 16), [&](auto L) { hipLaunchKernelGGL((sage_mean_cat_kernel<decltype(L)::value, XF>), grid, dim3(kBlock), 0, st, a); });
  return glnn::check_launch("glnn_sage_mean_fwd_bwd_f32: forward aggregation");
}

int launch_bwd(const BwdArgs& a, hipStream_t st) {
  const int dv = ((a.d + 3) & ~3) / 4;
  const dim3 grid((unsigned)((a.n_src + kTileRows - 1) / kTileRows), (unsigned)((dv + 63) / 64));
  with_lpr<16>(lpr_for(dv, 16), [&](auto L) { hipLaunchKernelGGL((sage_mean_bwd_kernel<decltype(L)::value>), grid, dim3(kBlock), 0, st, a); });
  return glnn::check_launch("glnn_sage_mean_fwd_bwd_f32: backward aggregation");
}

inline int r4(int c) { return (c + 3) & ~3; }

// every argument check of the step, before any launch
int check_desc(const glnn_sage_step_desc* d, const glnn_sage_mean_desc* m, const glnn_sage_ln_desc* ln) {
  GLNN_REQUIRE(d && m, "glnn_sage_mean_fwd_bwd_f32: null descriptor");
  GLNN_REQUIRE(d->x && d->labels && d->dlogits && d->loss_out, "glnn_sage_mean_fwd_bwd_f32: null pointer");
  const int L = d->num_layers;
  GLNN_REQUIRE(L >= 1 && L <= GLNN_SAGE_MAX_LAYERS, "glnn_sage_mean_fwd_bwd_f32: num_layers=%d outside [1,%d]", L, GLNN_SAGE_MAX_LAYERS);
  GLNN_REQUIRE(m->num_layers == L, "glnn_sage_mean_fwd_bwd_f32: the mean descriptor has %d layers, the step descriptor %d", m->num_layers, L);
  for (int l = 0; l <= L; ++l) GLNN_REQUIRE(d->dims[l] >= 1, "glnn_sage_mean_fwd_bwd_f32: dims[%d] must be positive", l);
  GLNN_REQUIRE(d->dropout_p >= 0.f && d->dropout_p < 1.f, "glnn_sage_mean_fwd_bwd_f32: dropout_p outside [0, 1)");
  if (ln) GLNN_TRY(glnn::check_sage_ln_desc(d, ln, "glnn_sage_mean_fwd_bwd_f32"));
  GLNN_REQUIRE(d->ldx % 4 == 0 && d->ldx >= r4(d->dims[0]) && glnn::aligned16(d->x),
               "glnn_sage_mean_fwd_bwd_f32: x needs float4 rows (ldx a multiple of 4, >= %d; 16-byte aligned)", r4(d->dims[0]));
  GLNN_REQUIRE(d->ld_dlogits >= d->dims[L], "glnn_sage_mean_fwd_bwd_f32: ld_dlogits < dims[%d]", L);
  int max_hidden = 0;
  for (int l = 0; l < L; ++l) {
    const glnn_sage_layer& y = d->layer[l];
    const glnn_sage_mean_layer& q = m->layer[l];
    const int d_in = d->dims[l], d_out = d->dims[l + 1];
    GLNN_REQUIRE(y.indptr && y.w && y.b && y.gw && y.gb && y.z && q.w_self && q.b_self && q.gw_self && q.gb_self && q.cat && q.wcat && q.bsum,
                 "glnn_sage_mean_fwd_bwd_f32: layer %d: null pointer", l);
    GLNN_REQUIRE(y.indices || y.nnz == 0, "glnn_sage_mean_fwd_bwd_f32: layer %d: null indices with %lld edges", l, (long long)y.nnz);
    GLNN_REQUIRE(y.n_dst >= 1 && y.nnz >= 0, "glnn_sage_mean_fwd_bwd_f32: layer %d: bad block sizes", l);
    GLNN_REQUIRE(y.n_src >= y.n_dst, "glnn_sage_mean_fwd_bwd_f32: layer %d: n_src=%lld < n_dst=%lld (destinations come first among the sources)",
                 l, (long long)y.n_src, (long long)y.n_dst);
    GLNN_REQUIRE(y.n_src < ((int64_t)1 << 31), "glnn_sage_mean_fwd_bwd_f32: layer %d: n_src too large", l);
    GLNN_REQUIRE(l == 0 || y.n_src == d->layer[l - 1].n_dst, "glnn_sage_mean_fwd_bwd_f32: block %d has %lld sources, block %d %lld destinations",
                 l, (long long)y.n_src, l - 1, (long long)d->layer[l - 1].n_dst);
    GLNN_REQUIRE(q.ld_cat == 2ll * r4(d_in), "glnn_sage_mean_fwd_bwd_f32: layer %d: ld_cat=%lld must be 2 * round4(d_in) = %d", l,
                 (long long)q.ld_cat, 2 * r4(d_in));
    GLNN_REQUIRE(y.ldz % 4 == 0 && y.ldz >= r4(d_out), "glnn_sage_mean_fwd_bwd_f32: layer %d: ldz=%lld must be a multiple of 4 and >= %d", l,
                 (long long)y.ldz, r4(d_out));
    GLNN_REQUIRE(glnn::aligned16(q.cat) && glnn::aligned16(q.wcat) && glnn::aligned16(y.z), "glnn_sage_mean_fwd_bwd_f32: layer %d: 16-byte alignment required", l);
    if (l < L - 1) {
      max_hidden = d_out > max_hidden ? d_out : max_hidden;
      if (y.h) GLNN_REQUIRE(y.ldh % 4 == 0 && y.ldh >= r4(d_out) && glnn::aligned16(y.h),
                            "glnn_sage_mean_fwd_bwd_f32: layer %d: ldh=%lld must be a multiple of 4 and >= %d", l, (long long)y.ldh, r4(d_out));
      if (d->batchnorm)
        GLNN_REQUIRE(y.gamma && y.beta && y.ggamma && y.gbeta && y.running_mean && y.running_var && y.mean && y.rstd && y.a_scale && y.a_shift,
                     "glnn_sage_mean_fwd_bwd_f32: BatchNorm of hidden layer %d: null pointer", l);
      if (!y.h && d_out > kMaxTailD)
        return glnn::fail(GLNN_ERR_UNSUPPORTED, "glnn_sage_mean_fwd_bwd_f32: hidden layer %d is %d wide: the tail-in-gather form takes at most %d "
                          "columns, give the layer an h buffer", l, d_out, kMaxTailD);
    }
    if (l >= 1) {
      GLNN_REQUIRE(y.t_indptr && (y.t_indices || y.nnz == 0) && q.dcat, "glnn_sage_mean_fwd_bwd_f32: layer %d needs the transpose buffers and dcat", l);
      GLNN_REQUIRE(q.ld_dcat == q.ld_cat && glnn::aligned16(q.dcat), "glnn_sage_mean_fwd_bwd_f32: layer %d: ld_dcat=%lld must equal ld_cat=%lld", l,
                   (long long)q.ld_dcat, (long long)q.ld_cat);
    }
  }
  if (L > 1)
    GLNN_REQUIRE(d->dh && d->ld_dh % 4 == 0 && d->ld_dh >= r4(max_hidden) && glnn::aligned16(d->dh),
                 "glnn_sage_mean_fwd_bwd_f32: backward scratch dh missing, or ld_dh=%lld not a multiple of 4 >= %d", (long long)d->ld_dh, r4(max_hidden));
  return GLNN_OK;
}

int sage_mean_fwd_bwd_impl(const glnn_sage_step_desc* d, const glnn_sage_mean_desc* m, const glnn_sage_ln_desc* ln, void* stream) {
  GLNN_TRY(check_desc(d, m, ln));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int L = d->num_layers;
  const float p = d->dropout_p;
  // ---- W_cat = [W_neigh | W_self] and b_neigh + b_self of every layer, ONE launch ----------------------------------------------------------
  {
    PackArgs pa = {};
    int64_t most = 1;
    for (int l = 0; l < L; ++l) {
      const glnn_sage_mean_layer& q = m->layer[l];
      pa.layer[l] = {d->layer[l].w, q.w_self, d->layer[l].b, q.b_self, q.wcat, q.bsum, d->dims[l], d->dims[l + 1]};
      const int64_t tot = (int64_t)d->dims[l + 1] * q.ld_cat;
      most = tot > most ? tot : most;
    }
    int64_t blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pack_pair_kernel, dim3((unsigned)blocks, (unsigned)L), dim3(256), 0, st, pa);
    GLNN_TRY(glnn::check_launch("glnn_sage_mean_fwd_bwd_f32: weight pair packing"));
  }
  // ---- forward ---------------------------------------------------------------------------------------------------------------------------
  for (int l = 0; l < L; ++l) {
    const glnn_sage_layer& y = d->layer[l];
    const glnn_sage_mean_layer& q = m->layer[l];
    const int d_in = d->dims[l], d_out = d->dims[l + 1];
    CatArgs a = {};
    a.indptr = y.indptr; a.indices = y.indices; a.n_dst = y.n_dst; a.d = d_in; a.cat = q.cat; a.ld_cat = q.ld_cat;
    if (l == 0) {
      a.x = d->x; a.ldx = d->ldx; a.self_rows = y.self_rows;
      GLNN_TRY(launch_cat<0>(a, st));
    } else if (d->layer[l - 1].h) {
      a.x = d->layer[l - 1].h; a.ldx = d->layer[l - 1].ldh;
      GLNN_TRY(launch_cat<0>(a, st));
    } else {
      // the hidden layer in front left only z: its tail is evaluated on every gathered row and on the self row
      const glnn_sage_layer& pv = d->layer[l - 1];
      a.x = pv.z; a.ldx = pv.ldz;
      a.t_thr = glnn::drop_threshold(p); a.t_seed = pv.drop_seed; a.t_dscale = 1.0f / (1.0f - p);
      if (ln) {
        const glnn_sage_ln_layer& g = ln->layer[l - 1];
        a.t_scale = g.gamma; a.t_shift = g.beta; a.t_mean = g.mean; a.t_rstd = g.rstd;
        GLNN_TRY(launch_cat<2>(a, st));
      } else {
        a.t_scale = d->batchnorm ? pv.a_scale : nullptr; a.t_shift = d->batchnorm ? pv.a_shift : nullptr;
        GLNN_TRY(launch_cat<1>(a, st));
      }
    }
    // z = [mean | self] W_cat^T + (b_neigh + b_self): ONE product over K = 2 round4(d_in) (padding columns are zeros on both sides)
    const int k = (int)q.ld_cat;
    glnn::ColStats cs = {d->ws_bn, d->ws_bn_floats, 0, 0, 0, nullptr, nullptr, nullptr};
    if (l < L - 1 && d->batchnorm && glnn::opts().gemm_stats)
      GLNN_TRY(glnn::gemm_stats(q.cat, q.ld_cat, y.n_dst, k, q.wcat, q.ld_cat, d_out, q.bsum, y.z, y.ldz, d->ws_gemm, d->ws_gemm_floats, stream, &cs));
    else
      GLNN_TRY(glnn_gemm_f32(q.cat, q.ld_cat, nullptr, nullptr, nullptr, 0.f, 0u, y.n_dst, k, q.wcat, q.ld_cat, 0, d_out, nullptr, nullptr, q.bsum, 0,
                             y.z, y.ldz, d->ws_gemm, d->ws_gemm_floats, stream));
    if (l < L - 1) GLNN_TRY(glnn::sage_hidden_tail_fwd(d, ln, l, cs, stream));
  }
  // ---- loss + dlogits (labels indexed by the batch's output nodes) -------------------------------------------------------------------------
  const glnn_sage_layer& top = d->layer[L - 1];
  GLNN_TRY(glnn::softmax_loss(top.z, top.ldz, top.n_dst, d->dims[L], GLNN_LOSS_NLL, d->labels, d->label_rows, nullptr, 0, nullptr, d->lamb,
                              d->dlogits, d->ld_dlogits, nullptr, 0, d->loss_out, d->loss_accum, d->ws_loss, d->ws_loss_floats, stream, nullptr, nullptr));
  // ---- backward --------------------------------------------------------------------------------------------------------------------------
  const float* dz = d->dlogits;
  int64_t ld_dz = d->ld_dlogits;
  for (int l = L - 1; l >= 0; --l) {
    const glnn_sage_layer& y = d->layer[l];
    const glnn_sage_mean_layer& q = m->layer[l];
    const int d_in = d->dims[l], d_out = d->dims[l + 1];
    const int64_t half = q.ld_cat / 2;
    // dW_neigh = dz^T mean, dW_self = dz^T self: the two halves of the operand buffer, straight into the two gradient tensors
    // (the last layer's two bias gradients are both colsum(dz); hidden layers get theirs from the tail backward below)
    GLNN_TRY(glnn_gemm_tn_f32(dz, ld_dz, y.n_dst, d_out, q.cat, q.ld_cat, nullptr, nullptr, nullptr, 0.f, 0u, d_in, y.gw, d_in,
                              l == L - 1 ? y.gb : nullptr, d->ws_tn, d->ws_tn_floats, stream));
    GLNN_TRY(glnn_gemm_tn_f32(dz, ld_dz, y.n_dst, d_out, q.cat + half, q.ld_cat, nullptr, nullptr, nullptr, 0.f, 0u, d_in, q.gw_self, d_in,
                              l == L - 1 ? q.gb_self : nullptr, d->ws_tn, d->ws_tn_floats, stream));
    if (l == 0) break;                                     // the outermost block's input is feats: no gradient needed
    // dcat = dz [W_neigh | W_self] = [dmean | dself]
    GLNN_TRY(glnn_gemm_f32(dz, ld_dz, nullptr, nullptr, nullptr, 0.f, 0u, y.n_dst, d_out, q.wcat, q.ld_cat, 1, (int)q.ld_cat, nullptr, nullptr, nullptr,
                           0, q.dcat, q.ld_dcat, nullptr, 0, stream));
    if (y.tr_ws)                                           // not prebuilt by the caller: the PLAIN transpose (no identity term in "mean")
      GLNN_TRY(glnn_csr_transpose(y.indptr, y.indices, y.n_dst, y.n_src, y.nnz, 0, y.t_indptr, y.t_indices, y.tr_ws, y.tr_ws_bytes, stream));
    BwdArgs b = {y.t_indptr, y.t_indices, y.n_src, y.indptr, y.n_dst, q.dcat, q.ld_dcat, d_in, d->dh, d->ld_dh};
    GLNN_TRY(launch_bwd(b, st));
    // the tail of the layer in front produced h_l: dz_{l-1} in place on dh (+ the norm's gradients and db_{l-1})
    const glnn_sage_layer& prev = d->layer[l - 1];
    if (ln) {
      const glnn_sage_ln_layer& g = ln->layer[l - 1];
      GLNN_TRY(glnn_layernorm_bwd_f32(d->dh, d->ld_dh, prev.z, prev.ldz, prev.n_dst, d_in, g.gamma, g.beta, g.mean, g.rstd, 1, p, prev.drop_seed,
                                      d->dh, d->ld_dh, g.ggamma, g.gbeta, prev.gb, d->ws_bn, d->ws_bn_floats, stream));
    } else {
      GLNN_TRY(glnn::bn_relu_bwd(d->dh, d->ld_dh, prev.z, prev.ldz, prev.n_dst, d_in, d->batchnorm ? prev.gamma : nullptr, prev.mean, prev.rstd,
                                 d->batchnorm ? prev.a_scale : nullptr, d->batchnorm ? prev.a_shift : nullptr, p, prev.drop_seed, d->dh,
                                 d->ld_dh, prev.ggamma, prev.gbeta, prev.gb, d->ws_bn, d->ws_bn_floats, stream, nullptr));
    }
    // db_self = db_neigh = colsum(dz_{l-1})
    if (hipMemcpyAsync(m->layer[l - 1].gb_self, prev.gb, sizeof(float) * (size_t)d_in, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      (void)hipGetLastError();
      return glnn::fail(GLNN_ERR_HIP, "glnn_sage_mean_fwd_bwd_f32: copying the bias gradient of layer %d failed", l - 1);
    }
    dz = d->dh;
    ld_dz = d->ld_dh;
  }
  return GLNN_OK;
}

}  // namespace

extern "C" int glnn_sage_mean_fwd_bwd_f32(const glnn_sage_step_desc* d, const glnn_sage_mean_desc* m, const glnn_sage_ln_desc* ln, void* stream) {
  return sage_mean_fwd_bwd_impl(d, m, ln, stream);
}

// The whole optimisation step in ONE call: the entry above followed by the fused Adam launch on the same stream.  The gradient partials are
// folded by launches of their own (nothing is left pending for Adam), so the two-call form gives the same bits trivially.
extern "C" int glnn_sage_mean_train_step_f32(const glnn_sage_step_desc* d, const glnn_sage_mean_desc* m, const glnn_sage_ln_desc* ln,
                                             const glnn_adam_desc* adam, void* stream) {
  return glnn::step_then_adam(adam, "glnn_sage_mean_train_step_f32", false, stream,
                              [&](glnn::PendingFolds*) { return sage_mean_fwd_bwd_impl(d, m, ln, stream); });
}
