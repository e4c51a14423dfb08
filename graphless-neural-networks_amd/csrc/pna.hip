// PNA: Principal Neighbourhood Aggregation (Corso et al., NeurIPS 2020) for gfx950 (MI355X) -- docs/PNA_SEMANTICS.md.
//
//   S[v] = [ a[v] + mean | a[v] + min | a[v] + max | std ]  of the rows b[u], u -> v        (four parts of round4(d) floats each)
//
//   pna_agg_fwd_kernel   ONE gather of every neighbour row feeds all four statistics.  row_gather_dev.h's lane mapping (LPR lanes of
//     float4 a row, the 64 / LPR lane groups on different entries, one wave per row of <= kLongRow entries, the whole workgroup on a longer
//     one, under the two-role scan); the fold is NOT add4, so the loop and the two folds are written here and the header is untouched.
//       sum b, sum b^2   fp64 per lane, folded in a fixed order (xor tree over the groups; waves w + (w + 4), then (0 + 1) + (2 + 3)):
//                        a common offset of the column survives (the squares of fp32 values are exact in fp64).
//       min, max         (value, CSR position) pairs: the better value wins, an equal value with the smaller position wins -- a total
//                        order, so neither the result nor its argument depends on the lane layout.  Every comparison is an ordered
//                        < / > / == against an incumbent that starts at +-inf: a NaN is never "better", so a NaN never wins (a column
//                        whose entries are all NaN comes out as +-inf with argument -1).
//   pna_agg_bwd_kernel   the source pass over the transposed CSR with edge ids, one wave per source row: per entry (v, e) it gathers
//     dS[v], mu[v], sigma[v], arg[v] and the degree of v and adds  g_mu / d + g_sigma (b[u] - mu) / (d sigma) + [argmax == e] g_max +
//     [argmin == e] g_min  in transposed-CSR order (the groups folded by the xor tree).  Every source row is written.
//   pna_scale_fwd / pna_scale_bwd / pna_da   the row-local pieces: the three degree scalers applied to the stacked product
//     Z = S [W_0 | W_1 | W_2]^T (the 12 F wide matrix is never formed), their backward, and da = g_mean + g_min + g_max.
//
// No float atomics, no grid barrier: results are bit-identical run to run and a row's result does not depend on the other rows of the launch.
#include <climits>

#include "row_gather_dev.h"

namespace {

constexpr int kMaxD = GLNN_PNA_MAX_WIDTH;
constexpr double kVarEps = 1e-5;

// one lane's statistics of its four columns
struct PnaAcc {
  double s[4], q[4];
  float mn[4], mx[4];
  int amn[4], amx[4];
};

__device__ __forceinline__ void acc_init(PnaAcc& r) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    r.s[t] = 0.0; r.q[t] = 0.0;
    r.mn[t] = __builtin_huge_valf(); r.mx[t] = -__builtin_huge_valf();
    r.amn[t] = INT_MAX; r.amx[t] = INT_MAX;
  }
}

// (value, position) pairs: the challenger takes the place iff it is better, or equal and earlier (a NaN challenger fails both tests)
__device__ __forceinline__ void take_min(float& v, int& p, float ov, int op) {
  if (ov < v || (ov == v && op < p)) { v = ov; p = op; }
}
__device__ __forceinline__ void take_max(float& v, int& p, float ov, int op) {
  if (ov > v || (ov == v && op < p)) { v = ov; p = op; }
}

__device__ __forceinline__ void acc_merge(PnaAcc& r, const PnaAcc& o) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    r.s[t] += o.s[t];
    r.q[t] += o.q[t];
    take_min(r.mn[t], r.amn[t], o.mn[t], o.amn[t]);
    take_max(r.mx[t], r.amx[t], o.mx[t], o.amx[t]);
  }
}

// the lane groups' statistics into the lanes < LPR (every lane ends with its xor partners' total: + and the pair order are symmetric)
template <int LPR>
__device__ __forceinline__ void acc_fold_groups(PnaAcc& r) {
#pragma unroll
  for (int m = 32; m >= LPR; m >>= 1) {
    PnaAcc o;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      o.s[t] = __shfl_xor(r.s[t], m); o.q[t] = __shfl_xor(r.q[t], m);
      o.mn[t] = __shfl_xor(r.mn[t], m); o.mx[t] = __shfl_xor(r.mx[t], m);
      o.amn[t] = __shfl_xor(r.amn[t], m); o.amx[t] = __shfl_xor(r.amx[t], m);
    }
    acc_merge(r, o);
  }
}

// The 8 wave partials of a long row (lanes < LPR) through 4 LDS slots in a fixed order: waves 4-7 park, waves 0-3 merge theirs, wave 0
// merges the four.  The total is in wave 0's lanes < LPR.  Called by ALL waves of the workgroup; a barrier must follow before the next call
// (scan_rows has one behind every long row).
struct PnaSlots {
  double d[4][8][64];
  float f[4][8][64];
  int i[4][8][64];
};
__device__ __forceinline__ void slot_store(PnaSlots& s, int slot, int lane, const PnaAcc& r) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    s.d[slot][t][lane] = r.s[t]; s.d[slot][4 + t][lane] = r.q[t];
    s.f[slot][t][lane] = r.mn[t]; s.f[slot][4 + t][lane] = r.mx[t];
    s.i[slot][t][lane] = r.amn[t]; s.i[slot][4 + t][lane] = r.amx[t];
  }
}
__device__ __forceinline__ void slot_load(const PnaSlots& s, int slot, int lane, PnaAcc& r) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    r.s[t] = s.d[slot][t][lane]; r.q[t] = s.d[slot][4 + t][lane];
    r.mn[t] = s.f[slot][t][lane]; r.mx[t] = s.f[slot][4 + t][lane];
    r.amn[t] = s.i[slot][t][lane]; r.amx[t] = s.i[slot][4 + t][lane];
  }
}
template <int LPR>
__device__ __forceinline__ void acc_fold_waves(PnaAcc& r, int wave, int lane) {
  __shared__ PnaSlots s_slots;
  if (wave >= 4 && lane < LPR) slot_store(s_slots, wave - 4, lane, r);
  __syncthreads();
  if (wave < 4 && lane < LPR) {
    PnaAcc o;
    slot_load(s_slots, wave, lane, o);
    acc_merge(r, o);
    slot_store(s_slots, wave, lane, r);
  }
  __syncthreads();
  if (wave == 0 && lane < LPR) {
    PnaAcc o, p;
    slot_load(s_slots, 1, lane, o);
    acc_merge(r, o);                       // (0 + 1)
    slot_load(s_slots, 2, lane, o);
    slot_load(s_slots, 3, lane, p);
    acc_merge(o, p);                       // (2 + 3)
    acc_merge(r, o);
  }
}

struct PnaFwdArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const float* b; int64_t ldb; int d;
  const float* a; int64_t lda;            // optional: the destination's own term
  float* s; int64_t lds;                  // [n_dst, 4 round4(d)]
  float* mu; int64_t ldmu;                // training: the plain mean (the backward's centre)
  int32_t* arg; int64_t ldarg;            // training: [n_dst, 2 round4(d)] = [argmin | argmax]
  ScanGrid sg;
};

// This wave's share of the entries [e0, e1) of a row -- the 64-entry chunks e0 + 64 (wave_id + k n_waves) -- into r.  Group g of the wave
// takes the entries g, g + G, ... of a chunk, ascending, so inside a lane the positions only grow: a strict < / > keeps the first one.
template <int LPR>
__device__ __forceinline__ void wave_row_stats(const PnaFwdArgs& a, int64_t e0, int64_t e1, int wave_id, int n_waves, int lane, int col4,
                                               bool col_ok, PnaAcc& r) {
  constexpr int G = 64 / LPR;
  constexpr int U = 64 / G < 4 ? 64 / G : 4;      // rows in flight per group
  const int g = lane / LPR;
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
    for (int j = 0; j < cnt; j += G * U) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ei = j + u * G + g;
        const int src = (G == 1) ? __builtin_amdgcn_readlane(my_idx, ei & 63) : __shfl(my_idx, ei & 63);
        v[u] = (ei < cnt && col_ok) ? ld4(a.b + (int64_t)src * a.ldb + col4) : zero4();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ei = j + u * G + g;
        if (ei < cnt) {
          const int pos = (int)(base + ei);       // (nnz < 2^31: checked by the entry)
          const float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const double dx = (double)x[t];
            r.s[t] += dx;
            r.q[t] = fma(dx, dx, r.q[t]);
            if (x[t] < r.mn[t]) { r.mn[t] = x[t]; r.amn[t] = pos; }
            if (x[t] > r.mx[t]) { r.mx[t] = x[t]; r.amx[t] = pos; }
          }
        }
      }
    }
  }
}

__device__ __forceinline__ int4 mask_args(int4 p, int col4, int d) {
  if (col4 + 0 >= d || p.x == INT_MAX) p.x = -1;
  if (col4 + 1 >= d || p.y == INT_MAX) p.y = -1;
  if (col4 + 2 >= d || p.z == INT_MAX) p.z = -1;
  if (col4 + 3 >= d || p.w == INT_MAX) p.w = -1;
  return p;
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void pna_agg_fwd_kernel(const PnaFwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  const bool on = lane < LPR && col_ok;
  const int dp = (a.d + 3) & ~3;
  scan_rows(a.indptr, a.n_dst, a.sg, lane, wave, [&](int64_t v, int wave_id, int n_waves) {
    const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
    PnaAcc r;
    acc_init(r);
    wave_row_stats<LPR>(a, e0, e1, wave_id, n_waves, lane, col4, col_ok, r);
    acc_fold_groups<LPR>(r);
    if (n_waves > 1) acc_fold_waves<LPR>(r, wave_id, lane);      // (uniform over the workgroup: scan_rows calls a long row with all waves)
    if (wave_id != 0 || !on) return;
    float* srow = a.s + v * a.lds + col4;
    const int64_t deg = e1 - e0;
    if (deg == 0) {                                              // no message: zeros, and the std of nothing is sqrt(eps); no a term
      const float s0 = sqrtf((float)kVarEps);
      st4(srow, zero4()); st4(srow + dp, zero4()); st4(srow + 2 * dp, zero4());
      st4(srow + 3 * dp, mask_cols(make_float4(s0, s0, s0, s0), col4, a.d));
      if (a.mu) st4(a.mu + v * a.ldmu + col4, zero4());
      if (a.arg) {
        int4* ap = reinterpret_cast<int4*>(a.arg + v * a.ldarg + col4);
        ap[0] = make_int4(-1, -1, -1, -1);
        *reinterpret_cast<int4*>(a.arg + v * a.ldarg + dp + col4) = make_int4(-1, -1, -1, -1);
      }
      return;
    }
    const double inv = 1.0 / (double)deg;
    float m[4], sg[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double mean = r.s[t] * inv;
      double var = r.q[t] * inv - mean * mean;
      var = var > 0.0 ? var : 0.0;
      m[t] = (float)mean;
      sg[t] = sqrtf((float)(var + kVarEps));
    }
    const float4 av = a.a ? ld4(a.a + v * a.lda + col4) : zero4();
    st4(srow, mask_cols(make_float4(av.x + m[0], av.y + m[1], av.z + m[2], av.w + m[3]), col4, a.d));
    st4(srow + dp, mask_cols(make_float4(av.x + r.mn[0], av.y + r.mn[1], av.z + r.mn[2], av.w + r.mn[3]), col4, a.d));
    st4(srow + 2 * dp, mask_cols(make_float4(av.x + r.mx[0], av.y + r.mx[1], av.z + r.mx[2], av.w + r.mx[3]), col4, a.d));
    st4(srow + 3 * dp, mask_cols(make_float4(sg[0], sg[1], sg[2], sg[3]), col4, a.d));
    if (a.mu) st4(a.mu + v * a.ldmu + col4, mask_cols(make_float4(m[0], m[1], m[2], m[3]), col4, a.d));
    if (a.arg) {
      *reinterpret_cast<int4*>(a.arg + v * a.ldarg + col4) = mask_args(make_int4(r.amn[0], r.amn[1], r.amn[2], r.amn[3]), col4, a.d);
      *reinterpret_cast<int4*>(a.arg + v * a.ldarg + dp + col4) = mask_args(make_int4(r.amx[0], r.amx[1], r.amx[2], r.amx[3]), col4, a.d);
    }
  });
}

struct PnaBwdArgs {
  const int64_t* indptr;                                    // the FORWARD CSR's row pointers: deg(v)
  const int64_t* t_indptr; const int32_t* t_indices; const int32_t* t_eids; int64_t n_src;
  const float* ds; int64_t ldds;                            // [n_dst, 4 round4(d)] = [g_mean | g_min | g_max | g_std]
  const float* b; int64_t ldb; int d;
  const float* mu; int64_t ldmu; const float* sigma; int64_t ldsig;
  const int32_t* arg; int64_t ldarg;
  float* db; int64_t lddb;
};

template <int LPR>
__global__ __launch_bounds__(kBlock) void pna_agg_bwd_kernel(const PnaBwdArgs a) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane / LPR;
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  const int dp = (a.d + 3) & ~3;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + wave; u < a.n_src; u += n_waves) {      // (wave-uniform)
    const int64_t t0 = a.t_indptr[u], t1 = a.t_indptr[u + 1];
    const float4 bq = col_ok ? ld4(a.b + u * a.ldb + col4) : zero4();
    const float bu[4] = {bq.x, bq.y, bq.z, bq.w};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t base = t0; base < t1; base += 64) {
      const int64_t rem = t1 - base;
      const int cnt = rem < 64 ? (int)rem : 64;
      const int my_v = lane < cnt ? ld_idx_stream(a.t_indices + base + lane) : 0;
      const int my_e = lane < cnt ? ld_idx_stream(a.t_eids + base + lane) : 0;
      for (int j = 0; j < cnt; j += G) {
        const int ei = j + g;
        const int v = __shfl(my_v, ei & 63);
        const int e = __shfl(my_e, ei & 63);
        if (ei < cnt && col_ok) {
          const float deg = (float)(a.indptr[v + 1] - a.indptr[v]);
          const float inv_d = 1.0f / deg;
          const float* gp = a.ds + (int64_t)v * a.ldds + col4;
          const float4 g_mu = ld4(gp), g_mn = ld4(gp + dp), g_mx = ld4(gp + 2 * dp), g_sg = ld4(gp + 3 * dp);
          const float4 mu = ld4(a.mu + (int64_t)v * a.ldmu + col4), sg = ld4(a.sigma + (int64_t)v * a.ldsig + col4);
          const int4 amn = *reinterpret_cast<const int4*>(a.arg + (int64_t)v * a.ldarg + col4);
          const int4 amx = *reinterpret_cast<const int4*>(a.arg + (int64_t)v * a.ldarg + dp + col4);
          const float gmu[4] = {g_mu.x, g_mu.y, g_mu.z, g_mu.w}, gmn[4] = {g_mn.x, g_mn.y, g_mn.z, g_mn.w};
          const float gmx[4] = {g_mx.x, g_mx.y, g_mx.z, g_mx.w}, gsg[4] = {g_sg.x, g_sg.y, g_sg.z, g_sg.w};
          const float mm[4] = {mu.x, mu.y, mu.z, mu.w}, ss[4] = {sg.x, sg.y, sg.z, sg.w};
          const int imn[4] = {amn.x, amn.y, amn.z, amn.w}, imx[4] = {amx.x, amx.y, amx.z, amx.w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            float term = fmaf(gsg[t] * (bu[t] - mm[t]), inv_d / ss[t], gmu[t] * inv_d);
            if (imx[t] == e) term += gmx[t];
            if (imn[t] == e) term += gmn[t];
            acc[t] += term;
          }
        }
      }
    }
    const float4 tot = fold_groups<LPR>(make_float4(acc[0], acc[1], acc[2], acc[3]));
    if (lane < LPR && col_ok) st4(a.db + u * a.lddb + col4, mask_cols(tot, col4, a.d));
  }
}

// ---------------------------------------------------------------------------------------------------------------- row-local pieces
// the amplification and attenuation scalers of row v: log(max(deg, 1) + 1) / delta and its reciprocal
__device__ __forceinline__ void pna_scalers(const int64_t* indptr, int64_t v, float delta, float* amp, float* att) {
  const int64_t deg = indptr[v + 1] - indptr[v];
  const float l = logf((float)(deg > 1 ? deg : 1) + 1.0f);
  *amp = l / delta;
  *att = delta / l;
}

constexpr int kRowBlock = 256;

// out[v] = act(out[v] + Z_0[v] + s_amp Z_1[v] + s_att Z_2[v]),  Z = [Z_0 | Z_1 | Z_2] in parts of fop = round4(fo) floats
__global__ __launch_bounds__(kRowBlock) void pna_scale_fwd_kernel(const int64_t* __restrict__ indptr, int64_t n, int fo, int fop, float delta,
                                                                  const float* __restrict__ z, int64_t ldz, float* __restrict__ out,
                                                                  int64_t ldo, int relu) {
  const int64_t total = n * fop;
  for (int64_t i = (int64_t)blockIdx.x * kRowBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRowBlock) {
    const int64_t v = i / fop;
    const int c = (int)(i - v * fop);
    float y = 0.f;
    if (c < fo) {
      float amp, att;
      pna_scalers(indptr, v, delta, &amp, &att);
      const float* zr = z + v * ldz + c;
      y = fmaf(att, zr[2 * fop], fmaf(amp, zr[fop], out[v * ldo + c] + zr[0]));
      if (relu) y = fmaxf(y, 0.f);
    }
    out[v * ldo + c] = y;                 // (padding columns [fo, fop): zeros)
  }
}

// dZ[v] = [g[v] | s_amp g[v] | s_att g[v]]
__global__ __launch_bounds__(kRowBlock) void pna_scale_bwd_kernel(const int64_t* __restrict__ indptr, int64_t n, int fo, int fop, float delta,
                                                                  const float* __restrict__ g, int64_t ldg, float* __restrict__ dz,
                                                                  int64_t lddz) {
  const int64_t total = n * fop;
  for (int64_t i = (int64_t)blockIdx.x * kRowBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRowBlock) {
    const int64_t v = i / fop;
    const int c = (int)(i - v * fop);
    float g0 = 0.f, amp = 0.f, att = 0.f;
    if (c < fo) {
      pna_scalers(indptr, v, delta, &amp, &att);
      g0 = g[v * ldg + c];
    }
    float* zr = dz + v * lddz + c;
    zr[0] = g0; zr[fop] = amp * g0; zr[2 * fop] = att * g0;
  }
}

// da[v] = (g_mean + g_min) + g_max for deg(v) > 0, else 0 (a row without a message has no a term)
__global__ __launch_bounds__(kRowBlock) void pna_da_kernel(const int64_t* __restrict__ indptr, int64_t n, int d, int dp,
                                                           const float* __restrict__ ds, int64_t ldds, float* __restrict__ da, int64_t ldda) {
  const int64_t total = n * dp;
  for (int64_t i = (int64_t)blockIdx.x * kRowBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRowBlock) {
    const int64_t v = i / dp;
    const int c = (int)(i - v * dp);
    float y = 0.f;
    if (c < d && indptr[v + 1] > indptr[v]) {
      const float* gp = ds + v * ldds + c;
      y = (gp[0] + gp[dp]) + gp[2 * dp];
    }
    da[v * ldda + c] = y;
  }
}

inline unsigned row_local_grid(int64_t total) {
  int64_t blocks = (total + kRowBlock - 1) / kRowBlock;
  if (blocks > (1 << 16)) blocks = 1 << 16;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

inline bool args_ok(const int32_t* p, int64_t ld, int d) {
  return p == nullptr || (glnn::aligned16(p) && ld % 4 == 0 && ld >= 2 * ((d + 3) & ~3));
}

}  // namespace

extern "C" int glnn_pna_agg_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, int64_t nnz, const float* b,
                                    int64_t ldb, int d, const float* a, int64_t lda, float* s, int64_t lds, float* mu, int64_t ldmu,
                                    int32_t* arg, int64_t ldarg, void* stream) {
  const char* what = "glnn_pna_agg_fwd_f32";
  GLNN_REQUIRE(n_dst >= 0 && n_src >= 0 && nnz >= 0 && d >= 1, "%s: bad size", what);
  if (d > kMaxD) return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: rows of at most %d floats (got %d)", what, kMaxD, d);
  if (nnz >= ((int64_t)1 << 31) || n_src >= ((int64_t)1 << 31))
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: nnz and n_src below 2^31 (CSR positions and source ids are 32-bit)", what);
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && (indices || nnz == 0) && b && s, "%s: null pointer", what);
  GLNN_REQUIRE((mu == nullptr) == (arg == nullptr), "%s: mu and arg go together (the backward needs both)", what);
  const int dp = (d + 3) & ~3;
  GLNN_REQUIRE(rows_ok(b, ldb, d) && rows_ok(a, lda, d) && rows_ok(mu, ldmu, d), "%s: b, a and mu must be 16-byte aligned with a leading "
               "dimension %% 4 == 0 and >= round4(d)", what);
  GLNN_REQUIRE(glnn::aligned16(s) && lds % 4 == 0 && lds >= 4 * dp, "%s: s must be 16-byte aligned with lds %% 4 == 0 and >= 4 round4(d)", what);
  GLNN_REQUIRE(args_ok(arg, ldarg, d), "%s: arg must be 16-byte aligned with ldarg %% 4 == 0 and >= 2 round4(d)", what);
  PnaFwdArgs k = {};
  k.indptr = indptr; k.indices = indices; k.n_dst = n_dst; k.b = b; k.ldb = ldb; k.d = d; k.a = a; k.lda = lda; k.s = s; k.lds = lds;
  k.mu = mu; k.ldmu = ldmu; k.arg = arg; k.ldarg = ldarg;
  GLNN_TRY(scan_grid(n_dst, what, &k.sg));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_lpr<1>(lpr_for(dp / 4, 1), [&](auto L) {
    hipLaunchKernelGGL((pna_agg_fwd_kernel<decltype(L)::value>), dim3(k.sg.grid_x), dim3(kBlock), 0, st, k);
  });
  return glnn::check_launch(what);
}

extern "C" int glnn_pna_agg_bwd_f32(const int64_t* indptr, int64_t n_dst, const int64_t* t_indptr, const int32_t* t_indices,
                                    const int32_t* t_eids, int64_t n_src, int64_t nnz, const float* ds, int64_t ldds, const float* b,
                                    int64_t ldb, int d, const float* mu, int64_t ldmu, const float* sigma, int64_t ldsig, const int32_t* arg,
                                    int64_t ldarg, float* db, int64_t lddb, void* stream) {
  const char* what = "glnn_pna_agg_bwd_f32";
  GLNN_REQUIRE(n_dst >= 0 && n_src >= 0 && nnz >= 0 && d >= 1, "%s: bad size", what);
  if (d > kMaxD) return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: rows of at most %d floats (got %d)", what, kMaxD, d);
  if (nnz >= ((int64_t)1 << 31) || n_dst >= ((int64_t)1 << 31))
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: nnz and n_dst below 2^31 (CSR positions and row ids are 32-bit)", what);
  if (n_src == 0) return GLNN_OK;
  GLNN_REQUIRE(t_indptr && b && db, "%s: null pointer", what);
  GLNN_REQUIRE(nnz == 0 || (indptr && t_indices && t_eids && ds && mu && sigma && arg), "%s: null pointer", what);
  const int dp = (d + 3) & ~3;
  GLNN_REQUIRE(rows_ok(b, ldb, d) && rows_ok(mu, ldmu, d) && rows_ok(sigma, ldsig, d) && rows_ok(db, lddb, d),
               "%s: b, mu, sigma and db must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(d)", what);
  GLNN_REQUIRE(ds == nullptr || (glnn::aligned16(ds) && ldds % 4 == 0 && ldds >= 4 * dp),
               "%s: ds must be 16-byte aligned with ldds %% 4 == 0 and >= 4 round4(d)", what);
  GLNN_REQUIRE(args_ok(arg, ldarg, d), "%s: arg must be 16-byte aligned with ldarg %% 4 == 0 and >= 2 round4(d)", what);
  GLNN_REQUIRE(db != b && db != ds, "%s: db must not alias an input", what);
  PnaBwdArgs k = {};
  k.indptr = indptr; k.t_indptr = t_indptr; k.t_indices = t_indices; k.t_eids = t_eids; k.n_src = n_src; k.ds = ds; k.ldds = ldds;
  k.b = b; k.ldb = ldb; k.d = d; k.mu = mu; k.ldmu = ldmu; k.sigma = sigma; k.ldsig = ldsig; k.arg = arg; k.ldarg = ldarg;
  k.db = db; k.lddb = lddb;
  int64_t blocks = (n_src + kWaves - 1) / kWaves;
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_lpr<1>(lpr_for(dp / 4, 1), [&](auto L) {
    hipLaunchKernelGGL((pna_agg_bwd_kernel<decltype(L)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, st, k);
  });
  return glnn::check_launch(what);
}

extern "C" int glnn_pna_scale_fwd_f32(const int64_t* indptr, int64_t n, int fo, float delta, const float* z, int64_t ldz, float* out,
                                      int64_t ldo, int relu, void* stream) {
  const char* what = "glnn_pna_scale_fwd_f32";
  GLNN_REQUIRE(n >= 0 && fo >= 1, "%s: bad size", what);
  GLNN_REQUIRE(delta > 0.f, "%s: delta must be positive", what);
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && z && out, "%s: null pointer", what);
  const int fop = (fo + 3) & ~3;
  GLNN_REQUIRE(ldz >= 3 * fop && ldo >= fop, "%s: ldz >= 3 round4(fo) and ldo >= round4(fo)", what);
  GLNN_REQUIRE(n * (int64_t)fop < ((int64_t)1 << 40), "%s: n too large", what);
  hipLaunchKernelGGL(pna_scale_fwd_kernel, dim3(row_local_grid(n * fop)), dim3(kRowBlock), 0, reinterpret_cast<hipStream_t>(stream), indptr,
                     n, fo, fop, delta, z, ldz, out, ldo, relu);
  return glnn::check_launch(what);
}

extern "C" int glnn_pna_scale_bwd_f32(const int64_t* indptr, int64_t n, int fo, float delta, const float* g, int64_t ldg, float* dz,
                                      int64_t lddz, void* stream) {
  const char* what = "glnn_pna_scale_bwd_f32";
  GLNN_REQUIRE(n >= 0 && fo >= 1, "%s: bad size", what);
  GLNN_REQUIRE(delta > 0.f, "%s: delta must be positive", what);
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && g && dz, "%s: null pointer", what);
  const int fop = (fo + 3) & ~3;
  GLNN_REQUIRE(lddz >= 3 * fop && ldg >= fo, "%s: lddz >= 3 round4(fo) and ldg >= fo", what);
  GLNN_REQUIRE(n * (int64_t)fop < ((int64_t)1 << 40), "%s: n too large", what);
  hipLaunchKernelGGL(pna_scale_bwd_kernel, dim3(row_local_grid(n * fop)), dim3(kRowBlock), 0, reinterpret_cast<hipStream_t>(stream), indptr,
                     n, fo, fop, delta, g, ldg, dz, lddz);
  return glnn::check_launch(what);
}

extern "C" int glnn_pna_da_f32(const int64_t* indptr, int64_t n, int d, const float* ds, int64_t ldds, float* da, int64_t ldda,
                               void* stream) {
  const char* what = "glnn_pna_da_f32";
  GLNN_REQUIRE(n >= 0 && d >= 1, "%s: bad size", what);
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && ds && da, "%s: null pointer", what);
  const int dp = (d + 3) & ~3;
  GLNN_REQUIRE(ldds >= 4 * dp && ldda >= dp, "%s: ldds >= 4 round4(d) and ldda >= round4(d)", what);
  hipLaunchKernelGGL(pna_da_kernel, dim3(row_local_grid(n * dp)), dim3(kRowBlock), 0, reinterpret_cast<hipStream_t>(stream), indptr, n, d, dp,
                     ds, ldds, da, ldda);
  return glnn::check_launch(what);
}
