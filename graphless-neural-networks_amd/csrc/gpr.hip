// GPR-GNN propagation (Chien et al., ICLR 2021; docs/GPR_SEMANTICS.md) for gfx950 (MI355X): out = sum_{k = 0..K} gamma_k P^k h0 with
// K + 1 LEARNED coefficients, P = D_in^-1/2 A D_out^-1/2 (prop_dev.h: what the three files over P share).  One launch per step
// k = 1..K serves both directions: the forward over the in-CSR with (x_norm, row_norm, out_norm) = (src_norm, dst_norm, src_norm), the
// backward over the transposed CSR with the norms swapped (G_k = P^T G_{k-1}; no edge ids: there is no edge dropout).
//
//   step k:  row[i] = row_norm[i] * sum_{e = (j -> i)} xs[j],   xs = x_norm * x at k = 1 (x = h0 or g, unscaled), else the previous step's
//            stored rows, which are PRE-SCALED by out_norm (no per-edge multiply after step 1)
//            acc[i] = (k = 1 ? gamma_0 * x[i] : acc[i]) + gamma_k * row[i]          (the result after step K)
//            out[i] = out_norm[i] * row[i]                                           (skipped at k = K: out NULL)
//   backward only (h0 given):  row_dot[k][i] = sum_c row[i, c] * h0[i, c]  (lanes of the row folded by shuffles, fixed order), and at
//            k = 1 also row_dot[0][i] from x = g.  glnn_gpr_fold_f32 reduces row_dot [K + 1, m] to dgamma [K + 1] in fp64 with a fixed
//            geometry -- the row tickets below are dynamic, so per-workgroup partials would not be reproducible; per-row scalars are.
//   gamma is read from device memory (the parameter tensor Adam updates in place): no host read.
//
// Mapping: row_gather_dev.h's wave gather under the two-role scan, rows pulled from an LDS ticket.  Wider rows: blockIdx.y = the
// 256-column tile (prop_dev.h's to_col_tile; row_dot then holds one scalar per tile and row).  No float atomics, no grid barrier.
#include "prop_dev.h"

namespace {

constexpr int kFoldChunk = GLNN_GPR_FOLD_CHUNK;      // row_dot entries per stage-1 partial of the fold
constexpr int kFoldBlock = 256;

struct GprArgs {
  const int64_t* indptr; const int32_t* indices;
  int64_t n; int d;
  const float* x; int64_t ldx;
  const float* x_norm;       // non-NULL (k = 1): x is UNSCALED, each gathered row is multiplied by x_norm[source]
  const float* row_norm;     // the output row's own norm (forward: dst_norm, backward: src_norm)
  const float* out_norm;     // the stored row is multiplied by out_norm[row] (the next step's per-source norm)
  const float* gamma; int k;
  float* acc; int64_t ldacc;
  float* out; int64_t ldo;   // NULL at the last step: the row itself is not needed again
  const float* h0; int64_t ldh0; float* row_dot;    // backward: row_dot[(k * tiles + tile) * n + row]
  ScanGrid sg;
};

// sum over the LPR lanes of a row (every lane of the wave calls it; lanes outside the row's columns pass 0)
template <int LPR>
__device__ __forceinline__ float fold_row(float v) {
#pragma unroll
  for (int m = LPR >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// The fused epilogue of one row.  EVERY lane of the wave calls it (the row_dot shuffles need all of them); `on` marks the lanes that own
// four columns of the row (lane < LPR and col4 < d), the only ones that touch memory.
template <int LPR, bool DOT>
__device__ __forceinline__ void finish_row(const GprArgs& a, int64_t v, float4 sum, int col4, bool on, int lane, int tile, int tiles) {
  const bool first = a.k == 1;
  float r[4] = {0.f, 0.f, 0.f, 0.f}, x0[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    const float c = a.row_norm[v];
    r[0] = c * sum.x; r[1] = c * sum.y; r[2] = c * sum.z; r[3] = c * sum.w;
    const float gk = a.gamma[a.k];
    float4 p = first ? ld4(a.x + v * a.ldx + col4) : ld4(a.acc + v * a.ldacc + col4);
    x0[0] = p.x; x0[1] = p.y; x0[2] = p.z; x0[3] = p.w;
    const float g0 = first ? a.gamma[0] : 1.f;
    float an[4], y[4];
    const float onrm = a.out ? a.out_norm[v] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (col4 + t >= a.d) { r[t] = 0.f; x0[t] = 0.f; }                 // padding columns are written as zero
      an[t] = fmaf(gk, r[t], first ? g0 * x0[t] : x0[t]);
      y[t] = onrm * r[t];
    }
    st4(a.acc + v * a.ldacc + col4, make_float4(an[0], an[1], an[2], an[3]));
    if (a.out) st4(a.out + v * a.ldo + col4, make_float4(y[0], y[1], y[2], y[3]));
  }
  if (DOT) {
    float dk = 0.f, d0 = 0.f;
    if (on) {
      const float4 h = ld4(a.h0 + v * a.ldh0 + col4);
      const float hh[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (col4 + t < a.d) { dk = fmaf(r[t], hh[t], dk); d0 = fmaf(x0[t], hh[t], d0); }
    }
    dk = fold_row<LPR>(dk);
    if (first) d0 = fold_row<LPR>(d0);                                  // (uniform)
    if (on && lane == 0) {
      a.row_dot[((int64_t)a.k * tiles + tile) * a.n + v] = dk;
      if (first) a.row_dot[(int64_t)tile * a.n + v] = d0;
    }
  }
}

template <int LPR, bool XN, bool DOT>
__global__ __launch_bounds__(kBlock) void gpr_prop_kernel(const GprArgs a0) {
  GprArgs a = a0;
  const int tile = (int)blockIdx.y, tiles = (int)gridDim.y;
  to_col_tile<2>(tiles, a.d, a.x, a.acc, a.out, a.h0);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  const bool on = lane < LPR && col_ok;
  NormRows<XN> ld;
  ld.x = a.x; ld.ldx = a.ldx; ld.x_norm = a.x_norm; ld.col4 = col4; ld.col_ok = col_ok;
  scan_rows(a.indptr, a.n, a.sg, lane, wave, [&](int64_t v, int wave_id, int n_waves) {
    float4 sum = row_sum<LPR>(a.indptr, a.indices, v, wave_id, n_waves, lane, ld);
    if (wave_id == 0) finish_row<LPR, DOT>(a, v, sum, col4, on, lane, tile, tiles);      // (wave-uniform: all 64 lanes reach its shuffles)
  });
}

// K = 0 / the k = 0 entry: acc = gamma_0 x (padding zero) and row_dot[0] = <x, h0> per row and tile; one wave per row, no gather
template <int LPR, bool DOT>
__global__ __launch_bounds__(kBlock) void gpr_scale_kernel(const GprArgs a0) {
  GprArgs a = a0;
  const int tile = (int)blockIdx.y, tiles = (int)gridDim.y;
  // to_col_tile written out: behind the function this kernel alone comes out with another prologue (a branch where the two selects
  // are now) and 30 SGPRs for 34, every LPR; appnp_prop_kernel and gpr_prop_kernel come out the same instruction for instruction
  if (tiles > 1) {
    const int off = 256 * tile;
    a.x += off; a.acc += off; a.d = a0.d - off < 256 ? a0.d - off : 256;
    if (a.h0) a.h0 += off;
  }
  const int lane = threadIdx.x & 63;
  const int col4 = (lane % LPR) * 4;
  const bool on = lane < LPR && col4 < a.d;
  const float g0 = a.gamma[0];
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t v = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); v < a.n; v += n_waves) {      // (wave-uniform)
    float x0[4] = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      const float4 p = ld4(a.x + v * a.ldx + col4);
      x0[0] = p.x; x0[1] = p.y; x0[2] = p.z; x0[3] = p.w;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (col4 + t >= a.d) x0[t] = 0.f;
      st4(a.acc + v * a.ldacc + col4, make_float4(g0 * x0[0], g0 * x0[1], g0 * x0[2], g0 * x0[3]));
    }
    if (DOT) {
      float d0 = 0.f;
      if (on) {
        const float4 h = ld4(a.h0 + v * a.ldh0 + col4);
        const float hh[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (col4 + t < a.d) d0 = fmaf(x0[t], hh[t], d0);
      }
      d0 = fold_row<LPR>(d0);
      if (on && lane == 0) a.row_dot[(int64_t)tile * a.n + v] = d0;
    }
  }
}

template <bool DOT>
void launch_scale(int lpr, dim3 grid, hipStream_t st, const GprArgs& a) {
  with_lpr<1>(lpr, [&](auto L) { hipLaunchKernelGGL((gpr_scale_kernel<decltype(L)::value, DOT>), grid, dim3(kBlock), 0, st, a); });
}

// fp64 sum of one wave's values in a fixed xor tree, then the block's waves in wave order (thread 0 holds the result)
__device__ __forceinline__ double block_sum_f64(double v, double* s_w) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kFoldBlock / 64; ++w) t += s_w[w];
  return t;
}

// stage 1: partial[r][c] = sum of row_dot[r][c kFoldChunk .. +kFoldChunk) -- thread t takes entries t, t + 256, ... of the chunk
__global__ __launch_bounds__(kFoldBlock) void gpr_fold_chunks_kernel(const float* __restrict__ row_dot, int64_t m, int64_t n_chunks,
                                                                     double* __restrict__ partial) {
  __shared__ double s_w[kFoldBlock / 64];
  const int64_t c = blockIdx.x, r = blockIdx.y;
  const int64_t b = c * kFoldChunk;
  const int64_t e = b + kFoldChunk < m ? b + kFoldChunk : m;
  const float* p = row_dot + r * m;
  double s = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += kFoldBlock) s += (double)p[i];
  const double t = block_sum_f64(s, s_w);
  if (threadIdx.x == 0) partial[r * n_chunks + c] = t;
}

// stage 2: dgamma[r] = sum of partial[r][0 .. n_chunks) -- thread t takes partials t, t + 256, ..., then the same tree
__global__ __launch_bounds__(kFoldBlock) void gpr_fold_final_kernel(const double* __restrict__ partial, int64_t n_chunks,
                                                                    float* __restrict__ dgamma) {
  __shared__ double s_w[kFoldBlock / 64];
  const int64_t r = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n_chunks; i += kFoldBlock) s += partial[r * n_chunks + i];
  const double t = block_sum_f64(s, s_w);
  if (threadIdx.x == 0) dgamma[r] = (float)t;
}

}  // namespace

extern "C" int glnn_gpr_prop_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* x, int64_t ldx, int d,
                                 const float* x_norm, const float* row_norm, const float* out_norm, const float* gamma, int k, float* acc,
                                 int64_t ldacc, float* out, int64_t ldo, const float* h0, int64_t ldh0, float* row_dot, void* stream) {
  const char* what = "glnn_gpr_prop_f32";
  GLNN_TRY(prop_sizes_ok(what, n, d, nnz, k >= 0));
  GLNN_TRY(prop_nnz_ok(what, nnz, GLNN_ERR_UNSUPPORTED, "CSR positions"));
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(x && acc && gamma, "%s: null pointer", what);
  GLNN_REQUIRE(k == 0 || (indptr && (indices || nnz == 0) && row_norm), "%s: null pointer", what);
  GLNN_REQUIRE((h0 == nullptr) == (row_dot == nullptr), "%s: h0 and row_dot go together", what);
  GLNN_REQUIRE(k != 1 || x_norm, "%s: step 1 gathers the unscaled rows (x_norm required)", what);
  GLNN_REQUIRE(k <= 1 || !x_norm, "%s: steps k > 1 gather pre-scaled rows (x_norm must be NULL)", what);
  GLNN_REQUIRE(k == 0 || !out || out_norm, "%s: a stored row is pre-scaled for the next step (out_norm required with out)", what);
  GLNN_REQUIRE(rows_ok(x, ldx, d) && rows_ok(acc, ldacc, d) && rows_ok(k ? out : nullptr, ldo, d) && rows_ok(h0, ldh0, d),
               kRowsText, what);
  GLNN_REQUIRE(acc != x && (k == 0 || !out || (out != x && out != acc)) && (!h0 || h0 != acc), "%s: acc / out must not alias an input", what);
  GprArgs a = {};
  a.indptr = indptr; a.indices = indices; a.n = n; a.d = d;
  a.x = x; a.ldx = ldx; a.x_norm = x_norm; a.row_norm = row_norm; a.out_norm = out_norm;
  a.gamma = gamma; a.k = k; a.acc = acc; a.ldacc = ldacc; a.out = k ? out : nullptr; a.ldo = ldo;
  a.h0 = h0; a.ldh0 = ldh0; a.row_dot = row_dot;
  const int lpr = lpr_for(((d < 256 ? d : 256) + 3) / 4, 1);
  const unsigned tiles = (unsigned)((d + 255) / 256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (k == 0) {
    int64_t blocks = (n + kWaves - 1) / kWaves;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks, tiles);
    if (h0) launch_scale<true>(lpr, grid, st, a); else launch_scale<false>(lpr, grid, st, a);
    return glnn::check_launch(what);
  }
  const int rc = scan_grid(n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  const dim3 grid(a.sg.grid_x, tiles);
  with_prop_variant<1>(x_norm != nullptr, h0 != nullptr, lpr, [&](auto XN, auto DOT, auto L) {
    hipLaunchKernelGGL((gpr_prop_kernel<decltype(L)::value, decltype(XN)::value, decltype(DOT)::value>), grid, dim3(kBlock), 0, st, a);
  });
  return glnn::check_launch(what);
}

static int64_t fold_workspace_bytes(int rows, int64_t m) {
  return (int64_t)rows * ((m + kFoldChunk - 1) / kFoldChunk) * (int64_t)sizeof(double);
}

extern "C" int glnn_gpr_fold_f32(const float* row_dot, int rows, int64_t m, float* dgamma, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  const char* what = "glnn_gpr_fold_f32";
  GLNN_REQUIRE(rows >= 0 && m >= 0, "%s: bad size", what);
  if (rows == 0) return GLNN_OK;
  GLNN_REQUIRE(dgamma, "%s: null pointer", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (m == 0) {                                         // an empty graph: every coefficient gradient is 0
    hipError_t e = hipMemsetAsync(dgamma, 0, sizeof(float) * rows, st);
    if (e != hipSuccess) return glnn::fail(GLNN_ERR_HIP, "%s: memset failed: %s", what, hipGetErrorString(e));
    return GLNN_OK;
  }
  GLNN_REQUIRE(row_dot && workspace, "%s: null pointer", what);
  GLNN_REQUIRE(rows <= 65535, "%s: at most 65535 coefficients", what);
  const int64_t n_chunks = (m + kFoldChunk - 1) / kFoldChunk;
  GLNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= fold_workspace_bytes(rows, m),
               "%s: workspace too small (rows * ceil(m / GLNN_GPR_FOLD_CHUNK) * 8 bytes) or not 8-byte aligned", what);
  GLNN_REQUIRE(n_chunks < ((int64_t)1 << 31), "%s: m too large", what);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(gpr_fold_chunks_kernel, dim3((unsigned)n_chunks, (unsigned)rows), dim3(kFoldBlock), 0, st, row_dot, m, n_chunks, partial);
  hipLaunchKernelGGL(gpr_fold_final_kernel, dim3((unsigned)rows), dim3(kFoldBlock), 0, st, partial, n_chunks, dgamma);
  return glnn::check_launch(what);
}
