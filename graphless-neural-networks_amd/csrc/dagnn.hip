// DAGNN's gate (Liu, Gao, Ji, KDD 2020; docs/DAGNN_SEMANTICS.md) for gfx950 (MI355X): out[i] = sum_{k = 0..K} s_k[i] H_k[i] with
// H_0 = h0, H_k = P H_{k-1}, P = D_in^-1/2 A D_out^-1/2 and a NODE-ADAPTIVE gate s_k[i] = sigmoid(<H_k[i], w> + b) over the hops.
// The propagation H_k = P H_{k-1} (and P^T T_{k+1} in the backward) is glnn_spmm_csr_f32 with its row and column scales, the kernel the
// GCN teacher runs; this file holds what is DAGNN's own, three row-local kernels without a gather:
//
//   gate, step k:       s = sigmoid(<x[i], w> + b), x = H_k;  acc[i] = (k = 0 ? 0 : acc[i]) + s x[i];  score[k n + i] = s
//   gate backward, k:   q = <g[i], h[i]> s (1 - s), s = score[k n + i], h = the saved H_k;  out[i] = s g[i] + q w + t[i]  (t = P^T T_{k+1},
//                       NULL at k = K);  q_out[k n + i] = q
//   fold:               dw = Hs^T q, db = sum q over the (K + 1) n stacked rows, in fp64 with a fixed geometry: per-row scalars leave the
//                       backward, so the sums do not depend on which workgroup took which row (gpr.hip's rule).
//   w, b are read from device memory (the parameter tensors Adam updates in place): no host read.
//
// Mapping: row_gather_dev.h's lane layout, one wave per row, LPR lanes moving float4.  The gate is a whole-row dot product, so d <= 256:
// the LPR lanes of a row fold it with xor shuffles in a fixed order.  No float atomics, no grid barrier.
#include "prop_dev.h"

namespace {

constexpr int kMaxD = 256;
constexpr int kFoldRows = GLNN_DAGNN_FOLD_CHUNK;      // stacked rows per stage-1 partial of the fold
constexpr int kFoldBlock = 256;

struct GateArgs {
  int64_t n; int d;
  const float* w; const float* b; int k;
  const float* x; int64_t ldx;      // forward: H_k
  float* acc; int64_t ldacc;        // forward: the gated sum
  float* score;                     // forward: [(K + 1) n] gates, or NULL (eval)
  const float* g; int64_t ldg;      // backward: G = dL/dout
  const float* h; int64_t ldh;      // backward: the saved H_k
  const float* gate;                // backward: the forward's score
  const float* t; int64_t ldt;      // backward: P^T T_{k+1}, or NULL (k = K); may be `out` itself
  float* out; int64_t ldo;          // backward: T_k
  float* q;                         // backward: [(K + 1) n]
};

// sum over the LPR lanes of a row, xor LPR / 2 down to 1 (every lane of the wave calls it)
template <int LPR>
__device__ __forceinline__ float row_fold(float v) {
#pragma unroll
  for (int m = LPR >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// <a, b> of a row from each lane's four columns, in a fixed order
template <int LPR>
__device__ __forceinline__ float row_dot(const float (&a)[4], const float (&b)[4]) {
  return row_fold<LPR>(fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]))));
}

__device__ __forceinline__ float gate_of(float dot, float b) { return 1.f / (1.f + expf(-(dot + b))); }

// the lane's four gate weights; zero in the padding columns and outside the row
__device__ __forceinline__ void load_w(const float* w, int col4, int d, float (&wv)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) wv[t] = col4 + t < d ? w[col4 + t] : 0.f;
}

// the lane's four columns of a row; zero in the padding columns and for lanes that own none (`on` false: no load)
__device__ __forceinline__ void load_row(const float* p, int col4, int d, bool on, float (&r)[4]) {
  const float4 v = on ? mask_cols(ld4(p + col4), col4, d) : zero4();
  r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
}

// one wave per row; `on` marks the lanes that own four columns of the row, the only ones that touch it
template <int LPR, bool FIRST, bool KEEP>
__global__ __launch_bounds__(kBlock) void dagnn_gate_kernel(const GateArgs a) {
  const int lane = threadIdx.x & 63;
  const int col4 = (lane % LPR) * 4;
  const bool on = lane < LPR && col4 < a.d;
  float wv[4];
  load_w(a.w, col4, a.d, wv);
  const float bias = a.b[0];
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t v = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); v < a.n; v += n_waves) {      // (wave-uniform)
    float p[4], c[4] = {0.f, 0.f, 0.f, 0.f};
    load_row(a.x + v * a.ldx, col4, a.d, on, p);
    if (!FIRST) load_row(a.acc + v * a.ldacc, col4, a.d, on, c);
    const float s = gate_of(row_dot<LPR>(p, wv), bias);
    if (on) st4(a.acc + v * a.ldacc + col4, make_float4(fmaf(s, p[0], c[0]), fmaf(s, p[1], c[1]), fmaf(s, p[2], c[2]), fmaf(s, p[3], c[3])));
    if (KEEP && lane == 0) a.score[(int64_t)a.k * a.n + v] = s;
  }
}

template <int LPR, bool ADD>
__global__ __launch_bounds__(kBlock) void dagnn_gate_bwd_kernel(const GateArgs a) {
  const int lane = threadIdx.x & 63;
  const int col4 = (lane % LPR) * 4;
  const bool on = lane < LPR && col4 < a.d;
  float wv[4];
  load_w(a.w, col4, a.d, wv);
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t v = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); v < a.n; v += n_waves) {      // (wave-uniform)
    float gr[4], hr[4], tr[4] = {0.f, 0.f, 0.f, 0.f};
    load_row(a.g + v * a.ldg, col4, a.d, on, gr);
    load_row(a.h + v * a.ldh, col4, a.d, on, hr);
    if (ADD) load_row(a.t + v * a.ldt, col4, a.d, on, tr);
    const float s = a.gate[(int64_t)a.k * a.n + v];
    const float q = row_dot<LPR>(gr, hr) * s * (1.f - s);
    if (on)
      st4(a.out + v * a.ldo + col4, make_float4(fmaf(q, wv[0], fmaf(s, gr[0], tr[0])), fmaf(q, wv[1], fmaf(s, gr[1], tr[1])),
                                                fmaf(q, wv[2], fmaf(s, gr[2], tr[2])), fmaf(q, wv[3], fmaf(s, gr[3], tr[3]))));
    if (lane == 0) a.q[(int64_t)a.k * a.n + v] = q;
  }
}

dim3 row_wave_grid(int64_t n) {
  int64_t blocks = (n + kWaves - 1) / kWaves;
  return dim3((unsigned)(blocks > 4096 ? 4096 : blocks));
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

// stage 1: partial[c][0 .. d) = sum over the stacked rows r of chunk c of q[r] hs[r], partial[c][d] = sum q[r].  LPR lanes a row (float4
// each), 256 / LPR rows in flight: row group g takes the rows g, g + 256 / LPR, ... of the chunk, ascending; the groups are summed in order.
template <int LPR>
__global__ __launch_bounds__(kFoldBlock) void dagnn_fold_chunks_kernel(const float* __restrict__ hs, int64_t ld, const float* __restrict__ q,
                                                                       int64_t rows, int d, double* __restrict__ partial) {
  constexpr int RG = kFoldBlock / LPR, W = LPR * 4;
  __shared__ double s_part[RG][W + 1];
  const int col4 = ((int)threadIdx.x % LPR) * 4, rg = (int)threadIdx.x / LPR;
  const bool col_ok = col4 < d;
  const int64_t r0 = (int64_t)blockIdx.x * kFoldRows;
  const int64_t r1 = r0 + kFoldRows < rows ? r0 + kFoldRows : rows;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, sq = 0.0;
  for (int64_t r = r0 + rg; r < r1; r += RG) {
    const double qv = (double)q[r];
    sq += qv;
    if (col_ok) {
      const float4 h = ld4(hs + r * ld + col4);
      s[0] += qv * (double)h.x; s[1] += qv * (double)h.y; s[2] += qv * (double)h.z; s[3] += qv * (double)h.w;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) s_part[rg][col4 + t] = s[t];
  if (col4 == 0) s_part[rg][W] = sq;
  __syncthreads();
  for (int c = threadIdx.x; c <= W; c += kFoldBlock) {
    if (c >= d && c != W) continue;                     // padding columns of the stack are not summed
    double t = 0.0;
    for (int g = 0; g < RG; ++g) t += s_part[g][c];
    partial[(int64_t)blockIdx.x * (d + 1) + (c == W ? d : c)] = t;
  }
}

// stage 2: workgroup c sums partial[0 .. n_chunks)[c] -- thread t takes chunks t, t + 256, ..., then the tree; c < d: dw[c], c = d: db
__global__ __launch_bounds__(kFoldBlock) void dagnn_fold_final_kernel(const double* __restrict__ partial, int64_t n_chunks, int d,
                                                                      float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double s_w[kFoldBlock / 64];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n_chunks; i += kFoldBlock) s += partial[i * (d + 1) + c];
  const double t = block_sum_f64(s, s_w);
  if (threadIdx.x == 0) {
    if (c < d) dw[c] = (float)t; else db[0] = (float)t;
  }
}

int sizes_ok(const char* what, int64_t n, int d, int k) {
  GLNN_REQUIRE(n >= 0 && d >= 1 && k >= 0, "%s: bad size", what);
  return d <= kMaxD ? GLNN_OK : glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: rows of at most %d columns (the gate is one row-wide dot product; got %d)",
                                           what, kMaxD, d);
}

}  // namespace

extern "C" int glnn_dagnn_gate_f32(const float* x, int64_t ldx, int64_t n, int d, const float* w, const float* b, int k, float* acc,
                                   int64_t ldacc, float* score, void* stream) {
  const char* what = "glnn_dagnn_gate_f32";
  GLNN_TRY(sizes_ok(what, n, d, k));
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(x && acc && w && b, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(x, ldx, d) && rows_ok(acc, ldacc, d), kRowsText, what);
  GLNN_REQUIRE(acc != x, "%s: acc must not alias x", what);
  GateArgs a = {};
  a.n = n; a.d = d; a.w = w; a.b = b; a.k = k; a.x = x; a.ldx = ldx; a.acc = acc; a.ldacc = ldacc; a.score = score;
  with_prop_variant<1>(k == 0, score != nullptr, lpr_for((d + 3) / 4, 1), [&](auto FIRST, auto KEEP, auto L) {
    hipLaunchKernelGGL((dagnn_gate_kernel<decltype(L)::value, decltype(FIRST)::value, decltype(KEEP)::value>), row_wave_grid(n), dim3(kBlock),
                       0, reinterpret_cast<hipStream_t>(stream), a);
  });
  return glnn::check_launch(what);
}

extern "C" int glnn_dagnn_gate_bwd_f32(const float* g, int64_t ldg, const float* h, int64_t ldh, int64_t n, int d, const float* score,
                                       const float* w, int k, const float* t, int64_t ldt, float* out, int64_t ldo, float* q_out,
                                       void* stream) {
  const char* what = "glnn_dagnn_gate_bwd_f32";
  GLNN_TRY(sizes_ok(what, n, d, k));
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(g && h && score && w && out && q_out, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(g, ldg, d) && rows_ok(h, ldh, d) && rows_ok(t, ldt, d) && rows_ok(out, ldo, d), kRowsText, what);
  GLNN_REQUIRE(out != g && out != h, "%s: out must not alias g or h", what);
  GateArgs a = {};
  a.n = n; a.d = d; a.w = w; a.k = k; a.g = g; a.ldg = ldg; a.h = h; a.ldh = ldh; a.gate = score; a.t = t; a.ldt = ldt;
  a.out = out; a.ldo = ldo; a.q = q_out;
  with_lpr<1>(lpr_for((d + 3) / 4, 1), [&](auto L) {
    if (t) hipLaunchKernelGGL((dagnn_gate_bwd_kernel<decltype(L)::value, true>), row_wave_grid(n), dim3(kBlock), 0,
                              reinterpret_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL((dagnn_gate_bwd_kernel<decltype(L)::value, false>), row_wave_grid(n), dim3(kBlock), 0,
                            reinterpret_cast<hipStream_t>(stream), a);
  });
  return glnn::check_launch(what);
}

extern "C" int64_t glnn_dagnn_fold_workspace_bytes(int64_t rows, int d) {
  if (rows < 0 || d < 1) return 0;
  return ((rows + kFoldRows - 1) / kFoldRows) * (int64_t)(d + 1) * (int64_t)sizeof(double);
}

extern "C" int glnn_dagnn_fold_f32(const float* hs, int64_t ldh, const float* q, int64_t rows, int d, float* dw, float* db, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  const char* what = "glnn_dagnn_fold_f32";
  GLNN_TRY(sizes_ok(what, rows, d, 0));
  GLNN_REQUIRE(dw && db, "%s: null pointer", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (rows == 0) {                                      // an empty graph: both gradients are 0
    hipError_t e = hipMemsetAsync(dw, 0, sizeof(float) * d, st);
    if (e == hipSuccess) e = hipMemsetAsync(db, 0, sizeof(float), st);
    if (e != hipSuccess) return glnn::fail(GLNN_ERR_HIP, "%s: memset failed: %s", what, hipGetErrorString(e));
    return GLNN_OK;
  }
  GLNN_REQUIRE(hs && q && workspace, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(hs, ldh, d), kRowsText, what);
  const int64_t n_chunks = (rows + kFoldRows - 1) / kFoldRows;
  GLNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= glnn_dagnn_fold_workspace_bytes(rows, d),
               "%s: workspace too small (glnn_dagnn_fold_workspace_bytes) or not 8-byte aligned", what);
  GLNN_REQUIRE(n_chunks < ((int64_t)1 << 31), "%s: too many rows", what);
  double* partial = static_cast<double*>(workspace);
  with_lpr<1>(lpr_for((d + 3) / 4, 1), [&](auto L) {
    hipLaunchKernelGGL((dagnn_fold_chunks_kernel<decltype(L)::value>), dim3((unsigned)n_chunks), dim3(kFoldBlock), 0, st, hs, ldh, q, rows, d,
                       partial);
  });
  hipLaunchKernelGGL(dagnn_fold_final_kernel, dim3((unsigned)(d + 1)), dim3(kFoldBlock), 0, st, partial, n_chunks, d, dw, db);
  return glnn::check_launch(what);
}
