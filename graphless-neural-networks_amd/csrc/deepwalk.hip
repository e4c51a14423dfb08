// DeepWalk position embeddings for the MLP student (docs/POSITION_SEMANTICS.md): the skip-gram step with negative sampling over ONE
// embedding table Z [N, d], batch-synchronous lazy Adam -- node2vec's objective with p = q = 1.  What the usual GPU composition does with
// nn.Embedding(sparse=True) + SparseAdam (gather / bmm / index_add with float atomics / coalesce with a sort) is three launches here, with
// a fixed summation order and no float atomics: the same input gives the same bits.
//
//   dw_pairs   walks [B, L + 1] -> per window q = i nwin + j: start[q] = W[i, j] and the pair row rest[q] of R = (1 + k)(c - 1) entries, the
//              c - 1 positives W[i, j + 1 ..] then k (c - 1) uniform negatives ((uint64)drop_hash(neg_seed, q, t') N) >> 32 -- the sampler's
//              own draw; it also writes the two arithmetic indptr arrays (q R and q) the transposes read.
//   dw_score   one wave per window, lane groups of LPR lanes moving float4 as in row_gather_dev.h: z_a once, then per entry the row, the
//              dot (xor shuffles inside the group), g[q R + t] = dLoss/ds, and the start-side gradient Gs[q] = sum_t g z_x; the snapshot
//              Zs[q] = z_a and the window's two loss partials.
//   dw_apply   the two-role scan over the N nodes: dZ[n] = sum over its windows of Gs[q] (the transposed start list), then
//              sum over its entries of g[eid] Zs[eid / R] (the transposed pair list, ascending edge ids), in that order; then the lazy-Adam
//              update of row n of Z, M, V in place.  It reads Gs, Zs and g only, never Z of another row.  Nodes with neither list are not
//              written.  One more workgroup of the same launch folds the loss partials in fp64, fixed order, into a device scalar.
//
// The rest of the node2vec family, each behind an entry of its own and the same kernels: glnn_deepwalk_pairs_from_walks takes the walks
// as an input (glnn_node2vec_walk's, csrc/node2vec.hip) and may draw the negatives through a 32-bit CDF; glnn_deepwalk_score_ctx_f32 reads
// the entries from a second table C (C == Z: the one-table bits), after which dZ comes from the start list alone and dC from the pair list
// alone -- two dw_apply launches, each with the other list empty.
#include "row_gather_dev.h"

namespace {

constexpr int kDwMaxD = 256;

// ------------------------------------------------------------------------------------------------ pairs
struct PairArgs {
  const int64_t* walks; int64_t n_roots; int length, context, negatives; int64_t n_nodes; uint32_t neg_seed;
  const uint32_t* neg_cdf;      // NULL: uniform negatives; else [n_nodes], the draw is the number of n < N - 1 with neg_cdf[n] <= r
  int32_t* start; int32_t* rest; int64_t* pair_indptr; int64_t* win_indptr;
};

__global__ __launch_bounds__(256) void dw_pairs_kernel(const PairArgs a) {
  const int nwin = a.length + 2 - a.context;
  const int n_pos = a.context - 1;
  const int R = (1 + a.negatives) * n_pos;
  const int64_t Q = a.n_roots * nwin;
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= Q * R) return;
  const int64_t q = id / R;
  const int t = (int)(id - q * R);
  const int64_t i = q / nwin;
  const int j = (int)(q - i * nwin);
  const int64_t* w = a.walks + i * (int64_t)(a.length + 1) + j;
  if (t < n_pos) {
    a.rest[id] = (int32_t)w[1 + t];
  } else {
    const uint32_t r = glnn::drop_hash(a.neg_seed, (uint32_t)q, (uint32_t)(t - n_pos));
    if (a.neg_cdf == nullptr) {
      a.rest[id] = (int32_t)(((uint64_t)r * (uint64_t)a.n_nodes) >> 32);
    } else {                                                               // upper bound over the first N - 1 entries: in [0, N - 1] whatever they hold
      int64_t lo = 0, hi = a.n_nodes - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.neg_cdf[mid] <= r) lo = mid + 1; else hi = mid;
      }
      a.rest[id] = (int32_t)lo;
    }
  }
  if (t == 0) {
    a.start[q] = (int32_t)w[0];
    a.pair_indptr[q] = q * R;
    a.win_indptr[q] = q;
    if (q == Q - 1) {
      a.pair_indptr[Q] = Q * R;
      a.win_indptr[Q] = Q;
    }
  }
}

// ------------------------------------------------------------------------------------------------ score
// the exact log-sigmoid forms: softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigmoid(x) = 1 / (1 + exp(-x)) evaluated on the side that
// does not overflow; no epsilon inside a log
__device__ __forceinline__ float dw_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float dw_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

struct ScoreArgs {
  const float* z; const float* c; int64_t n_nodes; int d;      // the start row comes from z, the entries from c (c == z: one table)
  const int32_t* start; const int32_t* rest; int64_t n_win; int n_pos; int R;
  float inv_pos, inv_neg;
  float* g; float* gs; float* zs; float* loss_parts;
};

template <int LPR>
__global__ __launch_bounds__(256) void dw_score_kernel(const ScoreArgs a) {
  constexpr int G = 64 / LPR;
  constexpr int kU = 4;
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // (wave-uniform)
  if (q >= a.n_win) return;
  const int grp = lane / LPR;
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  const int s = a.start[q];
  const bool s_ok = (unsigned)s < (unsigned)a.n_nodes;                   // (an id outside the table is never an index: the window counts for nothing)
  const float4 za = (s_ok && col_ok) ? ld4(a.z + (int64_t)s * a.d + col4) : zero4();
  const int32_t* row = a.rest + q * a.R;
  float4 acc = zero4();
  float lp = 0.f, ln = 0.f;
  for (int t0 = 0; t0 < a.R; t0 += G * kU) {                             // (uniform trip count: every lane reaches the shuffles)
    float4 zx[kU];
    bool ok[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {                                       // kU rows in flight per group before the first dot
      const int t = t0 + u * G + grp;
      const int x = t < a.R ? row[t] : -1;
      ok[u] = s_ok && (unsigned)x < (unsigned)a.n_nodes;
      zx[u] = (ok[u] && col_ok) ? ld4(a.c + (int64_t)x * a.d + col4) : zero4();
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int t = t0 + u * G + grp;
      float dot = fmaf(za.x, zx[u].x, fmaf(za.y, zx[u].y, fmaf(za.z, zx[u].z, za.w * zx[u].w)));
#pragma unroll
      for (int m = LPR >> 1; m >= 1; m >>= 1) dot += __shfl_xor(dot, m);
      float gt = 0.f;
      if (ok[u]) {
        const bool pos = t < a.n_pos;
        gt = pos ? -dw_sigmoid(-dot) * a.inv_pos : dw_sigmoid(dot) * a.inv_neg;      // (sigmoid(s) - 1 = -sigmoid(-s))
        if (pos) lp += dw_softplus(-dot); else ln += dw_softplus(dot);               // (counted once, by the group's first lane: below)
      }
      if (t < a.R && lane % LPR == 0) a.g[q * a.R + t] = gt;
      acc = fma4(gt, zx[u], acc);
    }
  }
  if (lane % LPR != 0) { lp = 0.f; ln = 0.f; }
  acc = fold_groups<LPR>(acc);
#pragma unroll
  for (int m = 32; m >= LPR; m >>= 1) { lp += __shfl_xor(lp, m); ln += __shfl_xor(ln, m); }
  if (lane < LPR && col_ok) {
    st4(a.gs + q * a.d + col4, acc);
    st4(a.zs + q * a.d + col4, za);
  }
  if (lane == 0) {
    a.loss_parts[q] = lp;
    a.loss_parts[a.n_win + q] = ln;
  }
}

// ------------------------------------------------------------------------------------------------ apply
struct ApplyArgs {
  const int64_t* tw_indptr; const int32_t* tw_indices;       // node -> its windows (the transposed start list)
  const int64_t* tp_indptr; const int32_t* tp_eids;          // node -> the pair-list positions q R + t at which it is the entry
  int64_t n_nodes; int d; int R;
  const float* gs; const float* zs; const float* g;
  float* z; float* m; float* v;
  float step_size, beta1, beta2, c1, c2, eps;       // c1 = 1 - beta1, c2 = 1 - beta2, rounded from the doubles
  const float* loss_parts; int64_t n_win; double inv_pos, inv_neg; float* loss_out;
  ScanGrid sg;
};

// g[eid] * Zs[eid / R]: the index stream is the edge ids themselves, the weight rides along with each
struct PairRows : GatherPolicy {
  static constexpr bool kWeighted = true;
  const float* g; const float* zs; int64_t ld; int R; int col4; bool col_ok;
  __device__ __forceinline__ float weight(int idx, bool in_range) const { return in_range ? g[idx] : 0.f; }
  __device__ __forceinline__ float4 row(int src, float, bool ok) const { return (ok && col_ok) ? ld4(zs + (int64_t)(src / R) * ld + col4) : zero4(); }
  __device__ __forceinline__ float4 add(float4 acc, float4 v, int, float w) const { return fma4(w, v, acc); }
};

template <int LPR>
__global__ __launch_bounds__(kBlock) void dw_apply_kernel(const ApplyArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x == a.sg.grid_x) {                            // the extra workgroup: the loss
    __shared__ double s_w[2][kWaves];
    double sp = 0.0, sn = 0.0;
    for (int64_t i = threadIdx.x; i < a.n_win; i += kBlock) { sp += (double)a.loss_parts[i]; sn += (double)a.loss_parts[a.n_win + i]; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { sp += __shfl_xor(sp, m); sn += __shfl_xor(sn, m); }
    if (lane == 0) { s_w[0][wave] = sp; s_w[1][wave] = sn; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double tp = 0.0, tn = 0.0;
      for (int w = 0; w < kWaves; ++w) { tp += s_w[0][w]; tn += s_w[1][w]; }
      *a.loss_out = (float)(tp * a.inv_pos + tn * a.inv_neg);
    }
    return;
  }
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  const bool on = lane < LPR && col_ok;
  NormRows<false> win;
  win.x = a.gs; win.ldx = a.d; win.x_norm = nullptr; win.col4 = col4; win.col_ok = col_ok;
  PairRows pr;
  pr.g = a.g; pr.zs = a.zs; pr.ld = a.d; pr.R = a.R; pr.col4 = col4; pr.col_ok = col_ok;
  scan_rows(a.tp_indptr, a.n_nodes, a.sg, lane, wave, [&](int64_t n, int wave_id, int n_waves) {
    const int64_t w0 = a.tw_indptr[n], w1 = a.tw_indptr[n + 1], p0 = a.tp_indptr[n], p1 = a.tp_indptr[n + 1];
    if (w0 == w1 && p0 == p1) return;                         // in no pair: not a single write (uniform; only a short row can be empty)
    float4 dw = wave_row_sum<LPR>(a.tw_indices, w0, w1, wave_id, n_waves, lane, win);
    float4 dp = wave_row_sum<LPR>(a.tp_eids, p0, p1, wave_id, n_waves, lane, pr);
    if (n_waves > 1) {
      dw = sum_waves_in_order<LPR>(dw, wave_id, lane);
      __syncthreads();
      dp = sum_waves_in_order<LPR>(dp, wave_id, lane);
    }
    if (wave_id != 0 || !on) return;
    const float4 dz = add4(dw, dp);
    const int64_t off = n * a.d + col4;
    const float4 m0 = ld4(a.m + off), v0 = ld4(a.v + off), z0 = ld4(a.z + off);
    const float gz[4] = {dz.x, dz.y, dz.z, dz.w}, mo[4] = {m0.x, m0.y, m0.z, m0.w}, vo[4] = {v0.x, v0.y, v0.z, v0.w}, zo[4] = {z0.x, z0.y, z0.z, z0.w};
    float mn[4], vn[4], zn[4];
    const float c1 = a.c1, c2 = a.c2;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      mn[t] = fmaf(a.beta1, mo[t], c1 * gz[t]);
      vn[t] = fmaf(a.beta2, vo[t], c2 * gz[t] * gz[t]);
      zn[t] = zo[t] - a.step_size * (mn[t] / (sqrtf(vn[t]) + a.eps));
    }
    st4(a.m + off, make_float4(mn[0], mn[1], mn[2], mn[3]));
    st4(a.v + off, make_float4(vn[0], vn[1], vn[2], vn[3]));
    st4(a.z + off, make_float4(zn[0], zn[1], zn[2], zn[3]));
  });
}

// what the three entries check alike: N, c, k, the width, and Q R < 2^31 (a pair-list position is an int32 edge id)
int dw_sizes(const char* what, int64_t n_nodes, int64_t n_windows, int context, int negatives, int* R) {
  GLNN_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "%s: the table must have 1 <= N < 2^31 rows (got %lld)", what, (long long)n_nodes);
  GLNN_REQUIRE(context >= 2 && context <= 65, "%s: context size must be in [2, walk length + 1] (got %d)", what, context);
  GLNN_REQUIRE(negatives >= 1, "%s: negatives per positive must be >= 1 (got %d)", what, negatives);
  GLNN_REQUIRE(n_windows >= 0, "%s: negative size", what);
  const int64_t r = (1 + (int64_t)negatives) * (context - 1);                      // (< 2^38)
  GLNN_REQUIRE(n_windows == 0 || r <= (((int64_t)1 << 31) - 1) / n_windows, "%s: the pair list must have Q R < 2^31 entries (got Q = %lld, R = %lld)",
               what, (long long)n_windows, (long long)r);
  *R = (int)r;
  return GLNN_OK;
}

int dw_width(const char* what, int d) {
  GLNN_REQUIRE(d >= 4 && d % 4 == 0 && d <= kDwMaxD, "%s: the embedding width must be a multiple of 4 in [4, %d] (got %d)", what, kDwMaxD, d);
  return GLNN_OK;
}

// the pair launch behind both pair entries: windows and pair rows from walks that are already on the device
int dw_pairs_launch(const char* what, const int64_t* walks, int64_t n_roots, int length, int context, int negatives, int64_t n_nodes,
                    uint32_t neg_seed, const uint32_t* neg_cdf, int R, int32_t* start, int32_t* rest, int64_t* pair_indptr, int64_t* win_indptr,
                    hipStream_t st) {
  const int64_t Q = n_roots * (int64_t)(length + 2 - context);
  PairArgs a;
  a.walks = walks; a.n_roots = n_roots; a.length = length; a.context = context; a.negatives = negatives; a.n_nodes = n_nodes;
  a.neg_seed = neg_seed; a.neg_cdf = neg_cdf; a.start = start; a.rest = rest; a.pair_indptr = pair_indptr; a.win_indptr = win_indptr;
  hipLaunchKernelGGL(dw_pairs_kernel, dim3((unsigned)((Q * R + 255) / 256)), dim3(256), 0, st, a);
  return glnn::check_launch(what);
}

// the score launch behind both score entries
int dw_score_launch(const char* what, const float* z, const float* c, int64_t n_nodes, int d, const int32_t* start, const int32_t* rest,
                    int64_t n_windows, int context, int negatives, float* g, float* gs, float* zs, float* loss_parts, void* stream) {
  int R;
  int rc = dw_sizes(what, n_nodes, n_windows, context, negatives, &R);
  if (rc == GLNN_OK) rc = dw_width(what, d);
  if (rc != GLNN_OK || n_windows == 0) return rc;
  GLNN_REQUIRE(z && c && start && rest && g && gs && zs && loss_parts, "%s: null pointer", what);
  GLNN_REQUIRE(glnn::aligned16(z) && glnn::aligned16(c) && glnn::aligned16(gs) && glnn::aligned16(zs), "%s: z, gs and zs must be 16-byte aligned", what);
  ScoreArgs a;
  a.z = z; a.c = c; a.n_nodes = n_nodes; a.d = d; a.start = start; a.rest = rest; a.n_win = n_windows; a.n_pos = context - 1; a.R = R;
  a.inv_pos = (float)(1.0 / ((double)n_windows * (context - 1)));
  a.inv_neg = (float)(1.0 / ((double)n_windows * (context - 1) * negatives));
  a.g = g; a.gs = gs; a.zs = zs; a.loss_parts = loss_parts;
  const dim3 grid((unsigned)((n_windows + 3) / 4));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_lpr<1>(lpr_for(d / 4, 1), [&](auto L) { hipLaunchKernelGGL((dw_score_kernel<decltype(L)::value>), grid, dim3(256), 0, st, a); });
  return glnn::check_launch(what);
}

}  // namespace

extern "C" int glnn_deepwalk_pairs(const int64_t* indptr, const int32_t* indices, int64_t n_nodes, const int64_t* roots,
                                   const int64_t* roots_host, int64_t n_roots, int length, int context, int negatives, uint32_t walk_seed,
                                   uint32_t neg_seed, int64_t* walks, int32_t* start, int32_t* rest, int64_t* pair_indptr,
                                   int64_t* win_indptr, void* stream) {
  const char* what = "glnn_deepwalk_pairs";
  GLNN_REQUIRE(length >= 1 && length <= 64, "%s: walk length must be in [1, 64] (got %d)", what, length);
  GLNN_REQUIRE(context >= 2 && context <= length + 1, "%s: context size must be in [2, walk length + 1] (got %d for walk length %d)", what,
               context, length);
  GLNN_REQUIRE(n_roots >= 0 && n_roots < ((int64_t)1 << 32), "%s: the number of roots must be in [0, 2^32)", what);
  const int64_t Q = n_roots * (int64_t)(length + 2 - context);
  int R;
  int rc = dw_sizes(what, n_nodes, Q, context, negatives, &R);
  if (rc != GLNN_OK) return rc;
  GLNN_REQUIRE(pair_indptr && win_indptr, "%s: null pointer", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_roots == 0) {
    if (hipMemsetAsync(pair_indptr, 0, sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(win_indptr, 0, sizeof(int64_t), st) != hipSuccess)
      return glnn::fail(GLNN_ERR_HIP, "%s: memset failed", what);
    return GLNN_OK;
  }
  GLNN_REQUIRE(indptr && indices && roots && walks && start && rest, "%s: null pointer", what);
  if (roots_host)                                             // (NULL: the caller vouches for the roots, as with glnn_random_walk)
    for (int64_t i = 0; i < n_roots; ++i)
      GLNN_REQUIRE(roots_host[i] >= 0 && roots_host[i] < n_nodes, "%s: root %lld (position %lld) is outside the graph of %lld nodes", what,
                   (long long)roots_host[i], (long long)i, (long long)n_nodes);
  rc = glnn_random_walk(indptr, indices, roots, n_roots, length, walk_seed, walks, stream);
  if (rc != GLNN_OK) return rc;
  return dw_pairs_launch(what, walks, n_roots, length, context, negatives, n_nodes, neg_seed, nullptr, R, start, rest, pair_indptr, win_indptr, st);
}

// glnn_deepwalk_pairs without its walk: `walks` is an input (glnn_random_walk's or glnn_node2vec_walk's), and the negatives may come from a
// distribution given as a 32-bit CDF.  neg_cdf == NULL and glnn_random_walk's walks: glnn_deepwalk_pairs' outputs bit for bit.
extern "C" int glnn_deepwalk_pairs_from_walks(const int64_t* walks, int64_t n_roots, int length, int context, int negatives, int64_t n_nodes,
                                              uint32_t neg_seed, const uint32_t* neg_cdf, int32_t* start, int32_t* rest,
                                              int64_t* pair_indptr, int64_t* win_indptr, void* stream) {
  const char* what = "glnn_deepwalk_pairs_from_walks";
  GLNN_REQUIRE(length >= 1 && length <= 64, "%s: walk length must be in [1, 64] (got %d)", what, length);
  GLNN_REQUIRE(context >= 2 && context <= length + 1, "%s: context size must be in [2, walk length + 1] (got %d for walk length %d)", what,
               context, length);
  GLNN_REQUIRE(n_roots >= 0 && n_roots < ((int64_t)1 << 32), "%s: the number of roots must be in [0, 2^32)", what);
  const int64_t Q = n_roots * (int64_t)(length + 2 - context);
  int R;
  int rc = dw_sizes(what, n_nodes, Q, context, negatives, &R);
  if (rc != GLNN_OK) return rc;
  GLNN_REQUIRE(pair_indptr && win_indptr, "%s: null pointer", what);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_roots == 0) {
    if (hipMemsetAsync(pair_indptr, 0, sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(win_indptr, 0, sizeof(int64_t), st) != hipSuccess)
      return glnn::fail(GLNN_ERR_HIP, "%s: memset failed", what);
    return GLNN_OK;
  }
  GLNN_REQUIRE(walks && start && rest, "%s: null pointer", what);
  return dw_pairs_launch(what, walks, n_roots, length, context, negatives, n_nodes, neg_seed, neg_cdf, R, start, rest, pair_indptr, win_indptr, st);
}

extern "C" int glnn_deepwalk_score_f32(const float* z, int64_t n_nodes, int d, const int32_t* start, const int32_t* rest, int64_t n_windows,
                                       int context, int negatives, float* g, float* gs, float* zs, float* loss_parts, void* stream) {
  return dw_score_launch("glnn_deepwalk_score_f32", z, z, n_nodes, d, start, rest, n_windows, context, negatives, g, gs, zs, loss_parts, stream);
}

// glnn_deepwalk_score_f32 with the entries read from a second table c [n_nodes, d]; the start row and the snapshot zs still come from z.
// c == z: glnn_deepwalk_score_f32's bits.
extern "C" int glnn_deepwalk_score_ctx_f32(const float* z, const float* c, int64_t n_nodes, int d, const int32_t* start, const int32_t* rest,
                                           int64_t n_windows, int context, int negatives, float* g, float* gs, float* zs, float* loss_parts,
                                           void* stream) {
  return dw_score_launch("glnn_deepwalk_score_ctx_f32", z, c, n_nodes, d, start, rest, n_windows, context, negatives, g, gs, zs, loss_parts, stream);
}

extern "C" int glnn_deepwalk_apply_f32(const int64_t* tw_indptr, const int32_t* tw_indices, const int64_t* tp_indptr, const int32_t* tp_eids,
                                       int64_t n_nodes, int d, int64_t n_windows, int context, int negatives, const float* g,
                                       const float* gs, const float* zs, float* z, float* m, float* v, double lr, double beta1, double beta2,
                                       double eps, int64_t step, const float* loss_parts, float* loss_out, void* stream) {
  const char* what = "glnn_deepwalk_apply_f32";
  int R;
  int rc = dw_sizes(what, n_nodes, n_windows, context, negatives, &R);
  if (rc == GLNN_OK) rc = dw_width(what, d);
  if (rc != GLNN_OK) return rc;
  GLNN_REQUIRE(step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: need step >= 1 and betas in [0, 1)", what);
  if (n_windows == 0) return GLNN_OK;
  GLNN_REQUIRE(tw_indptr && tw_indices && tp_indptr && tp_eids && g && gs && zs && z && m && v && loss_parts && loss_out, "%s: null pointer", what);
  GLNN_REQUIRE(glnn::aligned16(z) && glnn::aligned16(m) && glnn::aligned16(v) && glnn::aligned16(gs) && glnn::aligned16(zs),
               "%s: z, m, v, gs and zs must be 16-byte aligned", what);
  ApplyArgs a;
  a.tw_indptr = tw_indptr; a.tw_indices = tw_indices; a.tp_indptr = tp_indptr; a.tp_eids = tp_eids;
  a.n_nodes = n_nodes; a.d = d; a.R = R; a.gs = gs; a.zs = zs; a.g = g; a.z = z; a.m = m; a.v = v;
  // torch.optim.SparseAdam's step size, from the hyper-parameters as doubles (1 - 0.999f is off by 1.3e-5 of itself: the step size would be)
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  a.step_size = (float)(lr * sqrt(bc2) / bc1);
  a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.eps = (float)eps;
  a.c1 = (float)(1.0 - beta1); a.c2 = (float)(1.0 - beta2);
  a.loss_parts = loss_parts; a.n_win = n_windows;
  a.inv_pos = 1.0 / ((double)n_windows * (context - 1));
  a.inv_neg = 1.0 / ((double)n_windows * (context - 1) * negatives);
  a.loss_out = loss_out;
  rc = scan_grid(n_nodes, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  const dim3 grid(a.sg.grid_x + 1);                           // (+ 1: the workgroup that folds the loss)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_lpr<1>(lpr_for(d / 4, 1), [&](auto L) { hipLaunchKernelGGL((dw_apply_kernel<decltype(L)::value>), grid, dim3(kBlock), 0, st, a); });
  return glnn::check_launch(what);
}
