// int8 activation STORAGE for the whole-graph SAGE teacher forward (gfx950): the matrices an aggregation gathers are kept as int8 rows
// with one fp32 scale per row, every sum, MFMA and epilogue stays fp32 (docs/INT8_INFERENCE_SEMANTICS.md; the philosophy of sage_bf16.hip).
//
//   glnn_quant_rows_i8      fp32 [n, d] -> int8 rows [n, ld], ld = round16(d + 4): bytes [0, d) the values q in [-127, 127], bytes
//                           [d, ld - 4) zero, bytes [ld - 4, ld) the row's fp32 scale s; an element is q * s
//   glnn_spmm_sage_gcn_i8   epi((A x + x_self) / (deg + 1)) over int8 rows, fp32 or int8-row output (d <= 256)
//   glnn_sage_fused_i8      the K1F fused layer of glnn_sage_fused_bf16 with phase A reading int8 rows; fp32 outputs
//
// Mapping (sage_bf16.hip's): one wave per destination row of degree <= kLongRow, pulled from an LDS ticket; longer rows are taken by a
// whole workgroup, eight wave partials folded in LDS in fixed order.  A lane moves 16 bytes = 16 int8 per load, so LPR = ceil(d / 16)
// lanes (rounded up to a power of two) cover a row's VALUES and G = 64 / LPR groups of lanes take different in-edges.  The scale is a
// 4-byte load of each lane's own from the end of the same row (the line its group is fetching anyway): no lane is spent on a tail piece
// that holds nothing but the scale, so a 256-column row keeps LPR = 16 although it has 17 pieces.  int8 becomes fp32 by sign-extending
// conversion and enters the sum as fmaf(s, q, acc).  The group sums are folded with cross-lane adds in fixed order: results are
// bit-reproducible from run to run (no float atomics).  An int8 output row is quantised by the lanes that hold it (amax by cross-lane
// max) and written with plain vector stores.
#include <cmath>

#include "glnn_common.h"

namespace {

#ifndef GLNN_I8_U
#define GLNN_I8_U 8
#endif
constexpr int kBlock = 512;               // 8 waves
constexpr int kWaves = kBlock / 64;
constexpr int kRowsPerWave = 16;
constexpr int kLongRow = 128;             // degree above which a whole workgroup takes the row (spmm.hip's GLNN_LONG_ROW)
constexpr int kLongBlockRows = 512;
constexpr int kLongBlockCap = 512;
constexpr int kMaxLpr = 16;               // d <= 256

struct F16 { float v[16]; };
__device__ __forceinline__ F16 zero16() {
  F16 r;
#pragma unroll
  for (int t = 0; t < 16; ++t) r.v[t] = 0.f;
  return r;
}
__device__ __forceinline__ uint4 ld16(const int8_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ float ld_scale(const int8_t* row, int64_t ld) { return *reinterpret_cast<const float*>(row + ld - 4); }
// a += s * q for the 16 signed bytes of one piece
__device__ __forceinline__ void fma_q(F16& a, float s, uint4 q) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int b = 0; b < 4; ++b) a.v[4 * t + b] = fmaf(s, (float)(int)(int8_t)(w[t] >> (8 * b)), a.v[4 * t + b]);
  }
}
__device__ __forceinline__ void add16(F16& a, const F16& b) {
#pragma unroll
  for (int t = 0; t < 16; ++t) a.v[t] += b.v[t];
}
__device__ __forceinline__ int ld_idx_stream(const int32_t* p) { return __builtin_nontemporal_load(p); }

// the fp32 kernels' (a + s) / d with ONE residual correction (spmm.hip div_corrected): the same quotient at every aggregation site
__device__ __forceinline__ float div_corrected(float a, float d, float rd) {
  const float q = a * rd;
  const float e = fmaf(-q, d, a);
  return fmaf(e, rd, q);
}

// group g of the lanes (lane / LPR) takes the edges e with (e - base) % G == g of every 64-edge chunk dealt to this wave (chunks
// e0 + 64 (wave_id + k n_waves)), in ascending order, into `acc`.  Bytes past column d of a row's last value piece (zeros, or the scale
// itself) are accumulated like values and dropped by sage_mean.
template <int LPR, int U>
__device__ __forceinline__ void gather_acc(const int32_t* __restrict__ indices, int64_t e0, int64_t e1, int wave_id, int n_waves,
                                           const int8_t* __restrict__ x, int64_t ldx, int col16, bool col_ok, int lane, F16& acc) {
  constexpr int G = 64 / LPR;
  const int g = lane / LPR;
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(indices + base + lane) : 0;
    for (int j = 0; j < cnt; j += G * U) {
      uint4 q[U];
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ei = j + u * G + g;
        const int src = __shfl(my_idx, ei & 63);
        const bool ok = (ei < cnt) && col_ok;
        const int8_t* row = x + (int64_t)src * ldx;
        q[u] = ok ? ld16(row + col16) : make_uint4(0u, 0u, 0u, 0u);
        s[u] = ok ? ld_scale(row, ldx) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) fma_q(acc, s[u], q[u]);
    }
  }
}
// the G group sums folded (fixed order); every lane ends up holding the sum of its column piece
template <int LPR>
__device__ __forceinline__ void fold_groups(F16& acc) {
#pragma unroll
  for (int m = 32; m >= LPR; m >>= 1) {
#pragma unroll
    for (int t = 0; t < 16; ++t) acc.v[t] += __shfl_xor(acc.v[t], m);
  }
}
template <int LPR, int U>
__device__ __forceinline__ F16 gather_sum(const int32_t* __restrict__ indices, int64_t e0, int64_t e1, int wave_id, int n_waves,
                                          const int8_t* __restrict__ x, int64_t ldx, int col16, bool col_ok, int lane) {
  F16 acc = zero16();
  gather_acc<LPR, U>(indices, e0, e1, wave_id, n_waves, x, ldx, col16, col_ok, lane, acc);
  fold_groups<LPR>(acc);
  return acc;
}
// SAGE "gcn" mean (acc + self) / (deg + 1), columns >= d zeroed (col_ok lanes only: the others hold no piece of the self row)
__device__ __forceinline__ F16 sage_mean(const F16& acc, const int8_t* self_row, int64_t ld_self, int64_t deg, int col16, int d) {
  F16 t = acc;
  fma_q(t, ld_scale(self_row, ld_self), ld16(self_row + col16));
  const float dp1 = (float)deg + 1.0f;
  const float rd = __builtin_amdgcn_rcpf(dp1);
  F16 y;
#pragma unroll
  for (int k = 0; k < 16; ++k) y.v[k] = col16 + k < d ? div_corrected(t.v[k], dp1, rd) : 0.f;
  return y;
}

// ---- quantisation of one row held by an aligned group of LPR lanes (lane j of the group: columns [16 j, 16 j + 16), zeros past d) ----
// amax = max |y|, s = amax / 127, inv = 127 / amax (both correctly rounded), q = clamp(rint(y * inv), -127, 127); amax == 0: s = 0, q = 0;
// a NaN or an Inf in the row: s = NaN, q = 0.  Called by WHOLE waves (the cross-lane max reads every lane of the group); `writer` lanes
// store: value piece j by lane j, with the scale in its last word where the tail shares that piece, else the tail piece by lane 0.
template <int LPR>
__device__ __forceinline__ void quant_store(const F16& y, int col16, int d, int8_t* row, int64_t ld, bool writer) {
  float amax = 0.f;
  int bad = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float f = fabsf(y.v[t]);
    bad |= !(f <= 3.402823466e+38f);                     // NaN or Inf
    amax = fmaxf(amax, f);
  }
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, m));
    bad |= __shfl_xor(bad, m);
  }
  const bool flat = bad || amax == 0.f;
  const float s = bad ? __uint_as_float(0x7FC00000u) : __fdiv_rn(amax, 127.0f);
  const float inv = __fdiv_rn(127.0f, amax);
  uint32_t w[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    w[t] = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float r = fminf(fmaxf(rintf(y.v[4 * t + b] * inv), -127.f), 127.f);
      const int q = flat ? 0 : (int)r;
      w[t] |= ((uint32_t)q & 0xFFu) << (8 * b);
    }
  }
  if (!writer) return;
  const int piece = col16 >> 4;
  const int n_val = (d + 15) >> 4;                       // pieces that hold values
  const int n_all = (int)(ld >> 4);                      // n_val, or n_val + 1 when the scale has a piece of its own
  if (piece < n_val) {
    if (piece == n_all - 1) w[3] = __float_as_uint(s);   // (d <= 16 piece + 12 then: the last word holds no value)
    *reinterpret_cast<uint4*>(row + col16) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (piece == 0 && n_all > n_val) *reinterpret_cast<uint4*>(row + ld - 16) = make_uint4(0u, 0u, 0u, __float_as_uint(s));
}

// ---- stand-alone aggregation ----------------------------------------------------------------------------------------------
struct AggArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const int8_t* x; int64_t ldx; int d;
  const int8_t* x_self; int64_t ld_self;
  const float* ep_scale; const float* ep_shift; int relu;
  void* out; int64_t ldo;
  int n_long_blocks; int rows_per_block;
};

// epilogue of one row, called by whole waves (lane % LPR owns column piece col16; only lanes < LPR store): +self / (deg+1), then
// scale / shift / ReLU; columns >= d are 0
template <int LPR, bool OUT_I8>
__device__ __forceinline__ void finish_row(const AggArgs& a, int64_t v, int64_t deg, const F16& acc, int lane, int col16) {
  const bool col_ok = col16 < a.d;
  F16 y = zero16();
  if (col_ok) {
    y = sage_mean(acc, a.x_self + v * a.ld_self, a.ld_self, deg, col16, a.d);
#pragma unroll
    for (int t = 0; t < 16; ++t) {                       // (the epilogue vectors are read per row: kept in registers across the gather they
      const bool ok = col16 + t < a.d;                   //  would cost the kernel a wave of occupancy)
      float z = y.v[t];
      if (a.ep_scale && ok) z *= a.ep_scale[col16 + t];
      if (a.ep_shift && ok) z += a.ep_shift[col16 + t];
      if (a.relu) z = fmaxf(z, 0.f);
      y.v[t] = ok ? z : 0.f;
    }
  }
  if constexpr (OUT_I8) {
    quant_store<LPR>(y, col16, a.d, static_cast<int8_t*>(a.out) + v * a.ldo, a.ldo, lane < LPR);
  } else {
    if (lane < LPR && col_ok) {
      float* o = static_cast<float*>(a.out) + v * a.ldo + col16;
#pragma unroll
      for (int k = 0; k < 4; ++k) {                      // (ldo is only >= d rounded to 4)
        if (col16 + 4 * k < a.d) *reinterpret_cast<float4*>(o + 4 * k) = make_float4(y.v[4 * k], y.v[4 * k + 1], y.v[4 * k + 2], y.v[4 * k + 3]);
      }
    }
  }
}

template <int LPR, int U, bool OUT_I8>
__global__ __launch_bounds__(kBlock) void spmm_i8_kernel(const AggArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col16 = (lane % LPR) * 16;
  const bool col_ok = col16 < a.d;
  if ((int)blockIdx.x < a.n_long_blocks) {
    // long rows: chunk c of 512 rows owns the rows congruent to c modulo n_chunks, one row at a time by all eight waves, partials folded
    // in LDS in wave order
    __shared__ int64_t s_rows[kBlock];
    __shared__ int s_count;
    __shared__ F16 s_part[kWaves][kMaxLpr];
    const int64_t n_chunks = (a.n_dst + kBlock - 1) / kBlock;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += a.n_long_blocks) {
      if (threadIdx.x == 0) s_count = 0;
      __syncthreads();
      const int64_t r = (int64_t)threadIdx.x * n_chunks + chunk;
      if (r < a.n_dst && (a.indptr[r + 1] - a.indptr[r]) > kLongRow) s_rows[atomicAdd(&s_count, 1)] = r;
      __syncthreads();
      const int n_found = s_count;
      for (int i = 0; i < n_found; ++i) {
        const int64_t v = s_rows[i];
        const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
        const F16 acc = gather_sum<LPR, U>(a.indices, e0, e1, wave, kWaves, a.x, a.ldx, col16, col_ok, lane);
        if (lane < LPR) s_part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0) {
          F16 t = s_part[0][lane % LPR];
#pragma unroll 1                                         // (unrolled, the seven partials are all read first: 112 registers)
          for (int w = 1; w < kWaves; ++w) add16(t, s_part[w][lane % LPR]);
          finish_row<LPR, OUT_I8>(a, v, e1 - e0, t, lane, col16);
        }
        __syncthreads();
      }
    }
    return;
  }

  __shared__ int s_ticket;
  if (threadIdx.x == 0) s_ticket = 0;
  __syncthreads();
  const int64_t row_base = ((int64_t)blockIdx.x - a.n_long_blocks) * a.rows_per_block;
#pragma unroll 1
  while (true) {
    int lr = 0;
    if (lane == 0) lr = atomicAdd(&s_ticket, 1);
    lr = __builtin_amdgcn_readfirstlane(lr);
    if (lr >= a.rows_per_block) break;
    const int64_t v = row_base + lr;
    if (v >= a.n_dst) break;
    const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
    if (e1 - e0 > kLongRow) continue;
    const F16 acc = gather_sum<LPR, U>(a.indices, e0, e1, 0, 1, a.x, a.ldx, col16, col_ok, lane);
    finish_row<LPR, OUT_I8>(a, v, e1 - e0, acc, lane, col16);
  }
}

// lanes per row: the value pieces ceil(d / 16), rounded up to a power of two, at least 2
inline int lpr_of(int d) {
  const int p = (d + 15) / 16;
  return p <= 2 ? 2 : p <= 4 ? 4 : p <= 8 ? 8 : 16;
}

template <bool OUT_I8>
void launch_agg(const AggArgs& a, dim3 grid, hipStream_t st) {
  constexpr int U = GLNN_I8_U;
  switch (lpr_of(a.d)) {
    case 2: hipLaunchKernelGGL((spmm_i8_kernel<2, U, OUT_I8>), grid, dim3(kBlock), 0, st, a); break;
    case 4: hipLaunchKernelGGL((spmm_i8_kernel<4, U, OUT_I8>), grid, dim3(kBlock), 0, st, a); break;
    case 8: hipLaunchKernelGGL((spmm_i8_kernel<8, U, OUT_I8>), grid, dim3(kBlock), 0, st, a); break;
    default: hipLaunchKernelGGL((spmm_i8_kernel<16, U, OUT_I8>), grid, dim3(kBlock), 0, st, a); break;
  }
}

// ---- fused SAGE layer (K1F over int8 rows) -----------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kFusedRows = 32;

struct FusedArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const int8_t* x; int64_t ldx; int d_in;
  const int8_t* x_self; int64_t ld_self;
  const float* w_packed; int d_out; int kgroups;
  const float* ep_scale; const float* ep_shift; int relu;
  float* out; int64_t ldo;
  const float* w2_packed; int d_out2; int kgroups2; float* out2; int64_t ldo2;
  const int32_t* tile_order;
};

// the 16 columns of one lane into row lr of the aggregate tile: kpad is a multiple of 8, so a lane's second half may lie past it
__device__ __forceinline__ void put_tile(float* lds_a, int lda, int kpad, int lr, int col16, const F16& y) {
  float* p = lds_a + lr * lda + col16;
  if (col16 < kpad) {
    *reinterpret_cast<float4*>(p) = make_float4(y.v[0], y.v[1], y.v[2], y.v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(y.v[4], y.v[5], y.v[6], y.v[7]);
  }
  if (col16 + 8 < kpad) {
    *reinterpret_cast<float4*>(p + 8) = make_float4(y.v[8], y.v[9], y.v[10], y.v[11]);
    *reinterpret_cast<float4*>(p + 12) = make_float4(y.v[12], y.v[13], y.v[14], y.v[15]);
  }
}

// phase A of glnn_sage_fused_bf16 over int8 rows (the aggregate tile [32 x kpad] in LDS, fp32), phases B / C exactly its fp32 MFMA passes
template <int LPR, int U>
__global__ __launch_bounds__(kBlock) void sage_fused_i8_kernel(const FusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_a[];      // [32][kpad + 4]
  __shared__ F16 s_part[kWaves / 2][kMaxLpr];                         // 4 KiB (the fp32 kernel's LDS budget)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col16 = (lane % LPR) * 16;
  const bool col_ok = col16 < a.d_in;
  const int kpad = a.kgroups * 8;
  const int lda = kpad + 4;
  const int tile_id = a.tile_order ? a.tile_order[blockIdx.x] : (int)blockIdx.x;
  const int64_t row0 = (int64_t)tile_id * kFusedRows;

  __shared__ int s_next;
  if (threadIdx.x == 0) s_next = 0;
  __syncthreads();
#pragma unroll 1
  while (true) {
    int lr = 0;
    if (lane == 0) lr = atomicAdd(&s_next, 1);
    lr = __builtin_amdgcn_readfirstlane(lr);
    if (lr >= kFusedRows) break;
    const int64_t v = row0 + lr;
    F16 y = zero16();
    bool deferred = false;
    if (v < a.n_dst) {
      const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
      deferred = e1 - e0 > kLongRow;
      if (!deferred) {
        const F16 acc = gather_sum<LPR, U>(a.indices, e0, e1, 0, 1, a.x, a.ldx, col16, col_ok, lane);
        if (lane < LPR && col_ok) y = sage_mean(acc, a.x_self + v * a.ld_self, a.ld_self, e1 - e0, col16, a.d_in);
      }
    }
    if (!deferred && lane < LPR) put_tile(lds_a, lda, kpad, lr, col16, y);
  }
  __syncthreads();
  // long rows of the tile: all eight waves on one row, partials folded through four LDS slots in fixed order
#pragma unroll 1
  for (int lr = 0; lr < kFusedRows; ++lr) {
    const int64_t v = row0 + lr;
    if (v >= a.n_dst) break;
    const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
    if (e1 - e0 <= kLongRow) continue;
    const F16 acc = gather_sum<LPR, U>(a.indices, e0, e1, wave, kWaves, a.x, a.ldx, col16, col_ok, lane);
    if (wave >= 4 && lane < LPR) s_part[wave - 4][lane] = acc;
    __syncthreads();
    if (wave < 4 && lane < LPR) {
      F16 t = acc;
      add16(t, s_part[wave][lane]);
      s_part[wave][lane] = t;
    }
    __syncthreads();
    if (wave == 0 && lane < LPR) {
      F16 t = s_part[0][lane], t2 = s_part[2][lane];
      add16(t, s_part[1][lane]);
      add16(t2, s_part[3][lane]);
      add16(t, t2);
      F16 y = zero16();
      if (col_ok) y = sage_mean(t, a.x_self + v * a.ld_self, a.ld_self, e1 - e0, col16, a.d_in);
      put_tile(lds_a, lda, kpad, lr, col16, y);
    }
    __syncthreads();
  }

  // ---- phase B: [32 x K] (LDS) x W panel `wave` (packed, L2) on the fp32 MFMA ----
  const int n_tiles = (a.d_out + 31) / 32;
  const int nt = wave;
  const bool chain = a.w2_packed != nullptr;
  if (nt >= n_tiles && !chain) return;
  const int li = lane & 31, kk = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (nt < n_tiles) {
    const float4* wp = reinterpret_cast<const float4*>(a.w_packed) + ((int64_t)nt * a.kgroups) * 64 + lane;
    const float* ap = lds_a + li * lda + kk * 4;
    constexpr int PF = 4;
    float4 bq[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) bq[q] = (q < a.kgroups) ? wp[(int64_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kg0 = 0; kg0 < a.kgroups; kg0 += PF) {
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int kg = kg0 + q;
        if (kg < a.kgroups) {
          const float4 bv = bq[q];
          const int nxt = kg + PF;
          if (nxt < a.kgroups) bq[q] = wp[(int64_t)nxt * 64];
          const float4 av = *reinterpret_cast<const float4*>(ap + kg * 8);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
        }
      }
    }
  }
  // epilogue: C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  const int col = nt * 32 + li;
  const int ldh = a.kgroups2 * 8 + 4;
  if (chain) __syncthreads();                            // every wave is done reading the aggregate tile: the LDS is reused
  if (nt < n_tiles) {
    const bool col_ok2 = col < a.d_out;
    const float es = (a.ep_scale && col_ok2) ? a.ep_scale[col] : 1.f;
    const float eh = (a.ep_shift && col_ok2) ? a.ep_shift[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = (r & 3) + 8 * (r >> 2) + 4 * kk;
      const int64_t row = row0 + lr;
      float v = fmaf(acc[r], es, eh);
      if (a.relu) v = fmaxf(v, 0.f);
      if (!col_ok2) v = 0.f;
      if (a.out && col_ok2 && row < a.n_dst) a.out[row * a.ldo + col] = v;
      if (chain && col < a.kgroups2 * 8) lds_a[lr * ldh + col] = v;        // the chained pass reads the fp32 hidden row
    }
  }
  if (!chain) return;
  __syncthreads();
  // ---- phase C: [32 x d_out] hidden tile (LDS) x W2 panel `wave` -> out2 ----
  const int n_tiles2 = (a.d_out2 + 31) / 32;
  if (nt >= n_tiles2) return;
  const float4* wp = reinterpret_cast<const float4*>(a.w2_packed) + ((int64_t)nt * a.kgroups2) * 64 + lane;
  const float* ap = lds_a + li * ldh + kk * 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int kg = 0; kg < a.kgroups2; ++kg) {
    const float4 bv = wp[(int64_t)kg * 64];
    const float4 av = *reinterpret_cast<const float4*>(ap + kg * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
  }
  const int col2 = nt * 32 + li;
  if (col2 < a.d_out2) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
      if (row < a.n_dst) a.out2[row * a.ldo2 + col2] = acc[r];
    }
  }
}

// ---- quantise ---------------------------------------------------------------------------------------------------------------
// a group of LPR lanes per row, G = 64 / LPR rows per wave step; lane j of a group reads columns [16 j, 16 j + 16) (float4 loads when the
// source rows are 16-byte aligned) and stores piece j
template <int LPR, bool VEC>
__global__ __launch_bounds__(256) void quant_rows_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int d, int8_t* __restrict__ out,
                                                         int64_t ldo) {
  constexpr int G = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR;
  const int col16 = (lane % LPR) * 16;
  const int64_t wave_id = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t r0 = wave_id * G; r0 < n; r0 += n_waves * G) {
    const int64_t r = r0 + g;
    F16 y = zero16();
    if (r < n && col16 < d) {
      const float* p = x + r * ldx + col16;
      if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {                    // (ldx % 4 == 0: a float4 that starts below d ends inside the row)
          if (col16 + 4 * k < d) {
            const float4 f = *reinterpret_cast<const float4*>(p + 4 * k);
            y.v[4 * k] = f.x; y.v[4 * k + 1] = f.y; y.v[4 * k + 2] = f.z; y.v[4 * k + 3] = f.w;
          }
        }
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          if (col16 + t < d) y.v[t] = p[t];
        }
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        if (col16 + t >= d) y.v[t] = 0.f;
      }
    }
    quant_store<LPR>(y, col16, d, out + (r < n ? r : 0) * ldo, ldo, r < n);
  }
}

template <int LPR>
void launch_quant(bool vec, unsigned blocks, hipStream_t st, const float* x, int64_t ldx, int64_t n, int d, int8_t* out, int64_t ldo) {
  if (vec) hipLaunchKernelGGL((quant_rows_kernel<LPR, true>), dim3(blocks), dim3(256), 0, st, x, ldx, n, d, out, ldo);
  else hipLaunchKernelGGL((quant_rows_kernel<LPR, false>), dim3(blocks), dim3(256), 0, st, x, ldx, n, d, out, ldo);
}

inline int64_t round16_i8(int d) { return ((int64_t)d + 4 + 15) / 16 * 16; }

// the width / leading-dimension part of the row format: GLNN_ERR_UNSUPPORTED with nothing launched
int check_rows(const char* who, const char* what, int d, int64_t ld) {
  if (d > 256) return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: d=%d: int8 rows are at most 256 columns wide", who, d);
  if (ld != round16_i8(d)) {
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: %s=%lld: an int8 row of %d columns is exactly %lld bytes (round16(d + 4))", who, what,
                      (long long)ld, d, (long long)round16_i8(d));
  }
  return GLNN_OK;
}

}  // namespace

extern "C" int glnn_quant_rows_i8(const float* x, int64_t ldx, int64_t n, int d, int8_t* out, int64_t ldo, void* stream) {
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(x && out, "glnn_quant_rows_i8: null pointer");
  GLNN_REQUIRE(n > 0 && d >= 1 && ldx >= d, "glnn_quant_rows_i8: bad n / d / ldx");
  GLNN_TRY(check_rows("glnn_quant_rows_i8", "ldo", d, ldo));
  GLNN_REQUIRE(glnn::aligned16(out), "glnn_quant_rows_i8: out must be 16-byte aligned");
  const int lpr = lpr_of(d);
  const int64_t steps = (n + 64 / lpr - 1) / (64 / lpr);            // wave steps
  int64_t blocks = (steps + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  const bool vec = glnn::aligned16(x) && ldx % 4 == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (lpr) {
    case 2: launch_quant<2>(vec, (unsigned)blocks, st, x, ldx, n, d, out, ldo); break;
    case 4: launch_quant<4>(vec, (unsigned)blocks, st, x, ldx, n, d, out, ldo); break;
    case 8: launch_quant<8>(vec, (unsigned)blocks, st, x, ldx, n, d, out, ldo); break;
    default: launch_quant<16>(vec, (unsigned)blocks, st, x, ldx, n, d, out, ldo); break;
  }
  return glnn::check_launch("glnn_quant_rows_i8");
}

extern "C" int glnn_spmm_sage_gcn_i8(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const int8_t* x,
                                     int64_t ldx, int d, const int8_t* x_self, int64_t ld_self, const float* ep_scale,
                                     const float* ep_shift, int relu, void* out, int64_t ldo, int out_dtype, void* stream) {
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && x && x_self && out, "glnn_spmm_sage_gcn_i8: null pointer");
  GLNN_REQUIRE(n_dst > 0 && n_src >= 0 && n_src < (int64_t)1 << 31, "glnn_spmm_sage_gcn_i8: bad n_dst/n_src");
  GLNN_REQUIRE(d >= 1, "glnn_spmm_sage_gcn_i8: d=%d must be >= 1", d);
  GLNN_REQUIRE(out_dtype == GLNN_DTYPE_F32 || out_dtype == GLNN_DTYPE_I8, "glnn_spmm_sage_gcn_i8: unknown out_dtype %d", out_dtype);
  GLNN_TRY(check_rows("glnn_spmm_sage_gcn_i8", "ldx", d, ldx));
  GLNN_TRY(check_rows("glnn_spmm_sage_gcn_i8", "ld_self", d, ld_self));
  if (out_dtype == GLNN_DTYPE_I8) GLNN_TRY(check_rows("glnn_spmm_sage_gcn_i8", "ldo", d, ldo));
  else GLNN_REQUIRE(ldo % 4 == 0 && ldo >= ((d + 3) & ~3), "glnn_spmm_sage_gcn_i8: ldo=%lld must be a multiple of 4 and >= %d", (long long)ldo, (d + 3) & ~3);
  GLNN_REQUIRE(glnn::aligned16(x) && glnn::aligned16(x_self) && glnn::aligned16(out), "glnn_spmm_sage_gcn_i8: x/x_self/out must be 16-byte aligned");
  AggArgs a;
  a.indptr = indptr; a.indices = indices; a.n_dst = n_dst; a.x = x; a.ldx = ldx; a.d = d; a.x_self = x_self; a.ld_self = ld_self;
  a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.relu = relu; a.out = out; a.ldo = ldo;
  int64_t n_long = (n_dst + kLongBlockRows - 1) / kLongBlockRows;
  if (n_long > kLongBlockCap) n_long = kLongBlockCap;
  a.n_long_blocks = (int)n_long;
  int64_t rpw = n_dst / (2048 * kWaves);
  if (rpw < 1) rpw = 1;
  if (rpw > kRowsPerWave) rpw = kRowsPerWave;
  a.rows_per_block = (int)(kWaves * rpw);
  const int64_t row_blocks = (n_dst + a.rows_per_block - 1) / a.rows_per_block;
  GLNN_REQUIRE(row_blocks + n_long < ((int64_t)1 << 31), "glnn_spmm_sage_gcn_i8: n_dst too large for one launch");
  const dim3 grid((unsigned)(row_blocks + n_long));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (out_dtype == GLNN_DTYPE_I8) launch_agg<true>(a, grid, st);
  else launch_agg<false>(a, grid, st);
  return glnn::check_launch("glnn_spmm_sage_gcn_i8");
}

extern "C" int glnn_sage_fused_i8(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const int8_t* x,
                                  int64_t ldx, int d_in, const int8_t* x_self, int64_t ld_self, const float* w_packed, int d_out,
                                  const float* ep_scale, const float* ep_shift, int relu, float* out, int64_t ldo,
                                  const float* w2_packed, int d_out2, float* out2, int64_t ldo2, const int32_t* tile_order,
                                  void* stream) {
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && x && x_self && w_packed && (out || w2_packed), "glnn_sage_fused_i8: null pointer");
  GLNN_REQUIRE(!w2_packed || (out2 && d_out2 >= 1 && d_out2 <= 256 && ldo2 >= d_out2 && glnn::aligned16(w2_packed)),
               "glnn_sage_fused_i8: the chained projection needs out2 with ldo2 >= d_out2 in [1,256]");
  GLNN_REQUIRE(n_dst > 0 && n_src >= 0 && n_src < (int64_t)1 << 31, "glnn_sage_fused_i8: bad n_dst/n_src");
  GLNN_REQUIRE(d_in >= 1 && d_out >= 1 && d_out <= 256, "glnn_sage_fused_i8: d_in must be >= 1 and d_out in [1,256]");
  GLNN_TRY(check_rows("glnn_sage_fused_i8", "ldx", d_in, ldx));
  GLNN_TRY(check_rows("glnn_sage_fused_i8", "ld_self", d_in, ld_self));
  GLNN_REQUIRE(!out || ldo >= d_out, "glnn_sage_fused_i8: ldo=%lld must be >= d_out", (long long)ldo);
  GLNN_REQUIRE(glnn::aligned16(x) && glnn::aligned16(x_self) && glnn::aligned16(w_packed), "glnn_sage_fused_i8: 16-byte alignment required");
  const int64_t blocks = (n_dst + kFusedRows - 1) / kFusedRows;
  GLNN_REQUIRE(blocks < ((int64_t)1 << 31), "glnn_sage_fused_i8: n_dst too large for one launch");
  FusedArgs a;
  a.indptr = indptr; a.indices = indices; a.n_dst = n_dst; a.x = x; a.ldx = ldx; a.d_in = d_in; a.x_self = x_self; a.ld_self = ld_self;
  a.w_packed = w_packed; a.d_out = d_out; a.kgroups = (d_in + 7) / 8; a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.relu = relu;
  a.out = out; a.ldo = ldo;
  a.w2_packed = w2_packed; a.d_out2 = w2_packed ? d_out2 : 0; a.kgroups2 = w2_packed ? (d_out + 7) / 8 : 0; a.out2 = out2; a.ldo2 = ldo2;
  a.tile_order = tile_order;
  const int kg_lds = a.kgroups2 > a.kgroups ? a.kgroups2 : a.kgroups;
  const size_t smem = sizeof(float) * kFusedRows * (kg_lds * 8 + 4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  constexpr int U = GLNN_I8_U;
  // LPR * 16 >= kpad (d_in rounded up to 8): every column of the LDS tile is written by phase A
  switch (lpr_of(d_in)) {
    case 2: hipLaunchKernelGGL((sage_fused_i8_kernel<2, U>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a); break;
    case 4: hipLaunchKernelGGL((sage_fused_i8_kernel<4, U>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a); break;
    case 8: hipLaunchKernelGGL((sage_fused_i8_kernel<8, U>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a); break;
    default: hipLaunchKernelGGL((sage_fused_i8_kernel<16, U>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a); break;
  }
  return glnn::check_launch("glnn_sage_fused_i8");
}
