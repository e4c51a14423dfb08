// APPNP propagation (dgl APPNPConv(k=10, alpha=0.1, edge_drop=0.5), reference models.py:282-344) for gfx950 (MI355X):
// one launch per power-iteration step, forward and backward, over the graph's CSR and its transpose.
//
//   forward step t (x = s_{t-1}, stored PRE-SCALED by src_norm, or h0 itself at t = 1 with the per-edge multiply):
//       h_t[i] = (1 - alpha) * dst_norm[i] * dscale * sum_{kept e = (j -> i)} x[j]  +  alpha * h0[i]
//       stored as s_t[i] = src_norm[i] * h_t[i] (out_norm given), or unscaled at t = K
//   backward step t over the transposed CSR (row j = a source node, entries i with the original edge ids t_eids):
//       g_{t-1}[j] = (1 - alpha) * src_norm[j] * dscale * sum_{kept e = (j -> i)} q_t[i],   q_t = dst_norm * g_t
//       acc (first step: alpha * g_K[j] from the unscaled input row) += alpha * g_{t-1}[j];  at t = 1: out = g_0 + acc = dL/dh0
//
// The edge mask of step t is the counter hash edge_keep(seed, thr, t, edge id) evaluated in the gather: nothing E x K is stored, the
// forward and the backward of the same step see the same mask (the backward reads each transposed entry's original edge id), and a
// dropped edge's feature row is never loaded -- the kept entries of a 64-edge index chunk are compacted with ds_permute before the loads.
// Every kept edge carries the same weight 1 / (1 - p), so the sum runs over the plain rows and dscale goes into the row's coefficient.
//
// Mapping: row_gather_dev.h's wave gather under the two-role scan, rows pulled from an LDS ticket.  Wider rows: blockIdx.y = the
// 256-column tile (prop_dev.h's to_col_tile).
#include "prop_dev.h"

namespace {

__device__ __forceinline__ bool edge_keep(uint32_t seed, uint32_t thr, uint32_t t, uint32_t eid) {
  return (glnn::drop_hash(seed, eid, t) & 0xFFFFu) >= thr;
}

struct PropArgs {
  const int64_t* indptr; const int32_t* indices; const int32_t* eids;   // eids NULL: the edge id is the CSR position
  int64_t n; int d;
  const float* x; int64_t ldx;
  const float* x_norm;       // non-NULL: x is UNSCALED, each gathered row is multiplied by x_norm[source]
  const float* row_norm;     // the output row's own norm inside the coefficient (forward: dst_norm, backward: src_norm)
  const float* out_norm;     // non-NULL (not the last step): the stored row is multiplied by out_norm[row]
  float coef;                // (1 - alpha) / (1 - p)
  float alpha;
  uint32_t thr, seed, t;
  const float* h0; int64_t ldh0;                    // forward: the teleport term
  float* acc; int64_t ldacc; int first, last;       // backward: the running alpha-sum
  float* out; int64_t ldo;
  ScanGrid sg;
};

// The gathered rows, with the edge mask of step t as the per-chunk hook: the kept entries of a 64-entry chunk are moved to the low lanes in
// ascending order (ds_permute), so that group g takes kept entries g, g + G, ... and a dropped edge's row is never loaded.
template <bool XN>
struct PropRows : NormRows<XN> {
  const int32_t* eids; uint32_t thr, seed, t;
  __device__ __forceinline__ int chunk(int64_t base, int lane, int cnt, int& my_idx) const {
    if (!thr) return cnt;                                               // (uniform)
    const bool in = lane < cnt;
    const uint32_t eid = eids ? (uint32_t)(in ? eids[base + lane] : 0) : (uint32_t)(base + lane);
    const bool keep = in && edge_keep(seed, thr, t, eid);
    const uint64_t m = __ballot(keep);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int n_keep = __popcll(m);
    const int dst = keep ? below : n_keep + (lane - below);            // a permutation: kept entries first, in ascending order
    my_idx = __builtin_amdgcn_ds_permute(dst << 2, my_idx);
    return n_keep;
  }
};

// the fused epilogue of one row (lanes < LPR with col_ok): norms, teleport / running sum, zeroed padding columns
template <bool BWD>
__device__ __forceinline__ void finish_row(const PropArgs& a, int64_t v, float4 sum, int col4) {
  const float c = a.coef * a.row_norm[v];
  const float sv[4] = {sum.x, sum.y, sum.z, sum.w};
  float y[4], an[4] = {0.f, 0.f, 0.f, 0.f};
  const float on = a.out_norm ? a.out_norm[v] : 1.f;
  if (!BWD) {
    const float4 h = ld4(a.h0 + v * a.ldh0 + col4);
    const float hh[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float hk = fmaf(c, sv[k], a.alpha * hh[k]);
      y[k] = a.out_norm ? hk * on : hk;
    }
  } else {
    float ai[4];
    const float4 p = a.first ? ld4(a.x + v * a.ldx + col4) : ld4(a.acc + v * a.ldacc + col4);
    ai[0] = p.x; ai[1] = p.y; ai[2] = p.z; ai[3] = p.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (a.first) ai[k] = a.alpha * ai[k];                             // alpha g_K[j]
      const float gk = c * sv[k];                                       // g_{t-1}[j]
      if (a.last) {
        y[k] = gk + ai[k];
      } else {
        an[k] = fmaf(a.alpha, gk, ai[k]);
        y[k] = a.out_norm ? gk * on : gk;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (col4 + k >= a.d) { y[k] = 0.f; an[k] = 0.f; }                   // padding columns are written as zero
  st4(a.out + v * a.ldo + col4, make_float4(y[0], y[1], y[2], y[3]));
  if (BWD && !a.last) st4(a.acc + v * a.ldacc + col4, make_float4(an[0], an[1], an[2], an[3]));
}

template <int LPR, bool BWD, bool XN>
__global__ __launch_bounds__(kBlock) void appnp_prop_kernel(const PropArgs a0) {
  PropArgs a = a0;
  to_col_tile<2>(gridDim.y, a.d, a.x, a.out, a.h0, a.acc);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  PropRows<XN> ld;
  ld.x = a.x; ld.ldx = a.ldx; ld.x_norm = a.x_norm; ld.col4 = col4; ld.col_ok = col_ok;
  ld.eids = a.eids; ld.thr = a.thr; ld.seed = a.seed; ld.t = a.t;
  scan_rows(a.indptr, a.n, a.sg, lane, wave, [&](int64_t v, int wave_id, int n_waves) {
    const float4 sum = row_sum<LPR>(a.indptr, a.indices, v, wave_id, n_waves, lane, ld);
    if (wave_id == 0 && lane < LPR && col_ok) finish_row<BWD>(a, v, sum, col4);
  });
}

int prop_launch(PropArgs& a, int64_t nnz, int bwd, const char* what, void* stream) {
  GLNN_TRY(prop_sizes_ok(what, a.n, a.d, nnz));
  GLNN_TRY(prop_nnz_ok(what, nnz, GLNN_ERR_INVALID_ARG, "edge ids"));
  if (a.n == 0) return GLNN_OK;
  GLNN_REQUIRE(a.indptr && (a.indices || nnz == 0) && a.x && a.out && a.row_norm, "%s: null pointer", what);
  GLNN_REQUIRE(bwd ? (a.acc != nullptr || (a.first && a.last)) : a.h0 != nullptr, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(a.x, a.ldx, a.d) && rows_ok(a.out, a.ldo, a.d) && rows_ok(a.h0, a.ldh0, a.d) &&
               rows_ok(a.acc, a.ldacc, a.d), kRowsText, what);
  GLNN_REQUIRE(a.out != a.x && (!a.h0 || a.out != a.h0) && (!a.acc || (a.acc != a.out && a.acc != a.x)),
               "%s: out must not alias the input, h0 or acc", what);
  const int lpr = lpr_for(((a.d < 256 ? a.d : 256) + 3) / 4, 1);
  const int rc = scan_grid(a.n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  const dim3 grid(a.sg.grid_x, (unsigned)((a.d + 255) / 256));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_prop_variant<1>(bwd != 0, a.x_norm != nullptr, lpr, [&](auto BWD, auto XN, auto L) {
    hipLaunchKernelGGL((appnp_prop_kernel<decltype(L)::value, decltype(BWD)::value, decltype(XN)::value>), grid, dim3(kBlock), 0, st, a);
  });
  return glnn::check_launch(what);
}

// t_eids of glnn_csr_transpose_eids: one wave per row v of the ORIGINAL graph; edge e = (u -> v) lands in transposed row u at the first
// position holding v (binary search over the sorted row), plus -- for a multi-edge -- the number of earlier parallel edges u -> v in row v
__global__ __launch_bounds__(256) void tr_eids_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_dst,
                                                      const int64_t* __restrict__ t_indptr, const int32_t* __restrict__ t_indices,
                                                      int32_t* __restrict__ t_eids) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = w; v < n_dst; v += n_waves) {
    const int64_t e0 = indptr[v], e1 = indptr[v + 1];
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const int u = indices[e];
      int64_t lo = t_indptr[u], hi = t_indptr[u + 1];
      const int64_t end = hi;
      while (lo < hi) {                                 // first position with t_indices >= v
        const int64_t mid = (lo + hi) >> 1;
        if (t_indices[mid] < v) lo = mid + 1; else hi = mid;
      }
      int64_t pos = lo;
      if (lo + 1 < end && t_indices[lo + 1] == v)
        for (int64_t f = e0; f < e; ++f) pos += indices[f] == u ? 1 : 0;
      t_eids[pos] = (int32_t)e;
    }
  }
}

__global__ __launch_bounds__(256) void edge_mask_kernel(int64_t nnz, uint32_t t, uint32_t thr, uint32_t seed, uint8_t* __restrict__ mask) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride)
    mask[e] = edge_keep(seed, thr, t, (uint32_t)e) ? 1 : 0;
}

}  // namespace

extern "C" int glnn_appnp_prop_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* x, int64_t ldx,
                                   int d, const float* x_norm, const float* dst_norm, const float* src_norm_out, const float* h0, int64_t ldh0,
                                   float alpha, float edge_drop, uint32_t seed, int t, float* out, int64_t ldo, void* stream) {
  GLNN_REQUIRE(edge_drop >= 0.f && edge_drop < 1.f && t >= 1, "glnn_appnp_prop_f32: need 0 <= edge_drop < 1 and t >= 1");
  PropArgs a = {};
  a.indptr = indptr; a.indices = indices; a.eids = nullptr; a.n = n; a.d = d;
  a.x = x; a.ldx = ldx; a.x_norm = x_norm; a.row_norm = dst_norm; a.out_norm = src_norm_out;
  a.coef = (1.f - alpha) / (1.f - edge_drop); a.alpha = alpha;
  a.thr = glnn::drop_threshold(edge_drop); a.seed = seed; a.t = (uint32_t)t;
  a.h0 = h0; a.ldh0 = ldh0; a.out = out; a.ldo = ldo;
  return prop_launch(a, nnz, 0, "glnn_appnp_prop_f32", stream);
}

extern "C" int glnn_appnp_prop_bwd_f32(const int64_t* t_indptr, const int32_t* t_indices, const int32_t* t_eids, int64_t n, int64_t nnz,
                                       const float* x, int64_t ldx, int d, const float* x_norm, const float* src_norm,
                                       const float* dst_norm_out, float alpha, float edge_drop, uint32_t seed, int t, int first,
                                       float* acc, int64_t ldacc, float* out, int64_t ldo, void* stream) {
  GLNN_REQUIRE(edge_drop >= 0.f && edge_drop < 1.f && t >= 1, "glnn_appnp_prop_bwd_f32: need 0 <= edge_drop < 1 and t >= 1");
  GLNN_REQUIRE(t_eids || edge_drop == 0.f || n == 0 || nnz == 0, "glnn_appnp_prop_bwd_f32: edge dropout needs t_eids");
  GLNN_REQUIRE(t == 1 || dst_norm_out, "glnn_appnp_prop_bwd_f32: steps t > 1 store dst_norm * g (dst_norm_out NULL)");
  PropArgs a = {};
  a.indptr = t_indptr; a.indices = t_indices; a.eids = t_eids; a.n = n; a.d = d;
  a.x = x; a.ldx = ldx; a.x_norm = x_norm; a.row_norm = src_norm; a.out_norm = t > 1 ? dst_norm_out : nullptr;
  a.coef = (1.f - alpha) / (1.f - edge_drop); a.alpha = alpha;
  a.thr = glnn::drop_threshold(edge_drop); a.seed = seed; a.t = (uint32_t)t;
  a.acc = acc; a.ldacc = ldacc; a.first = first ? 1 : 0; a.last = t == 1 ? 1 : 0;
  a.out = out; a.ldo = ldo;
  GLNN_REQUIRE(!a.first || x_norm, "glnn_appnp_prop_bwd_f32: the first step gathers the unscaled g_K (x_norm = dst_norm required)");
  return prop_launch(a, nnz, 1, "glnn_appnp_prop_bwd_f32", stream);
}

extern "C" int glnn_csr_transpose_eids(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, int64_t nnz,
                                       int64_t* t_indptr, int32_t* t_indices, int32_t* t_eids, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
  if (nnz >= ((int64_t)1 << 31)) return glnn::fail(GLNN_ERR_UNSUPPORTED, "glnn_csr_transpose_eids: nnz >= 2^31 (edge ids are int32)");
  GLNN_REQUIRE(t_eids || nnz == 0, "glnn_csr_transpose_eids: null t_eids");
  const int rc = glnn_csr_transpose(indptr, indices, n_dst, n_src, nnz, 0, t_indptr, t_indices, workspace, workspace_bytes, stream);
  if (rc != GLNN_OK || nnz == 0 || n_dst == 0 || n_src == 0) return rc;
  int64_t blocks = (n_dst * 64 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(tr_eids_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), indptr, indices, n_dst,
                     t_indptr, t_indices, t_eids);
  return glnn::check_launch("glnn_csr_transpose_eids");
}

extern "C" int glnn_edge_drop_mask_u8(int64_t nnz, int t, float edge_drop, uint32_t seed, uint8_t* mask, void* stream) {
  GLNN_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31) && edge_drop >= 0.f && edge_drop < 1.f && t >= 1 && (mask || nnz == 0),
               "glnn_edge_drop_mask_u8: bad arguments");
  if (nnz == 0) return GLNN_OK;
  int64_t blocks = (nnz + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(edge_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), nnz, (uint32_t)t,
                     glnn::drop_threshold(edge_drop), seed, mask);
  return glnn::check_launch("glnn_edge_drop_mask_u8");
}
