// bf16 activation STORAGE for the whole-graph SAGE teacher forward (gfx950): the matrices an aggregation gathers are kept as bf16,
// every sum, MFMA and epilogue stays fp32.  The gathers move half the bytes per edge; nothing else changes.
//
//   glnn_cast_f32_bf16     fp32 [n, d] -> bf16 [n, ld] (ld a multiple of 8: every row 16-byte aligned), padding columns written as 0
//   glnn_spmm_csr_bf16     the SAGE_GCN / SUM aggregation of glnn_spmm_csr_f32 over bf16 rows, fp32 or bf16 output
//   glnn_sage_fused_bf16   the K1F fused layer of glnn_sage_fused_f32 over bf16 rows (fp32 MFMA on the fp32 aggregate), each of out /
//                          out2 stored fp32 or bf16
//
// Mapping (the fp32 kernels', spmm.hip): one wave per destination row of degree <= kLongRow, pulled from an LDS ticket; longer rows are
// taken by a whole workgroup (the first n_long_blocks workgroups of the aggregation launch, the tile's own workgroup in the fused
// launch), eight wave partials folded in LDS in fixed order.  A lane moves 16 bytes = 8 bf16 per load (expanded to fp32 in registers),
// so LPR = ceil(d / 8) lanes cover a row and G = 64 / LPR groups of lanes take different in-edges: at the same U loads per group in
// flight a wave holds TWICE the edges of the fp32 kernel of the same width.  The group sums are folded with cross-lane adds in fixed order:
// results are bit-reproducible from run to run (no float atomics).  Stores round to nearest even (torch's Tensor.to(torch.bfloat16):
// NaN -> the canonical quiet NaN 0x7FC0), written in plain C++.
#include "bf16_mfma_dev.h"      // bf16_t, f32_to_bf16_bits, pack2

namespace {

#ifndef GLNN_BF16_U
#define GLNN_BF16_U 8
#endif
constexpr int kBlock = 512;               // 8 waves
constexpr int kWaves = kBlock / 64;
constexpr int kRowsPerWave = 16;          // (the fp32 kernel's sweep-chosen value)
constexpr int kLongRow = 128;             // degree above which a whole workgroup takes the row (spmm.hip's GLNN_LONG_ROW)
constexpr int kLongBlockRows = 512;
constexpr int kLongBlockCap = 512;

struct F8 { float v[8]; };
__device__ __forceinline__ F8 zero8() {
  F8 r;
#pragma unroll
  for (int t = 0; t < 8; ++t) r.v[t] = 0.f;
  return r;
}
__device__ __forceinline__ uint4 ld8(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void add_u4(F8& a, uint4 q) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    a.v[2 * t] += __uint_as_float(w[t] << 16);
    a.v[2 * t + 1] += __uint_as_float(w[t] & 0xFFFF0000u);
  }
}
__device__ __forceinline__ void fma_u4(F8& a, float s, uint4 q) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    a.v[2 * t] = fmaf(s, __uint_as_float(w[t] << 16), a.v[2 * t]);
    a.v[2 * t + 1] = fmaf(s, __uint_as_float(w[t] & 0xFFFF0000u), a.v[2 * t + 1]);
  }
}
__device__ __forceinline__ F8 unpack(uint4 q) {
  F8 r = zero8();
  add_u4(r, q);
  return r;
}
__device__ __forceinline__ void add8(F8& a, const F8& b) {
#pragma unroll
  for (int t = 0; t < 8; ++t) a.v[t] += b.v[t];
}
__device__ __forceinline__ int ld_idx_stream(const int32_t* p) { return __builtin_nontemporal_load(p); }

// the fp32 kernels' (a + s) / d with ONE residual correction (spmm.hip div_corrected): the same quotient at every aggregation site
__device__ __forceinline__ float div_corrected(float a, float d, float rd) {
  const float q = a * rd;
  const float e = fmaf(-q, d, a);
  return fmaf(e, rd, q);
}

// group g of the lanes (lane / LPR) takes the edges e with (e - base) % G == g of every 64-edge chunk dealt to this wave (chunks
// e0 + 64 (wave_id + k n_waves)), in ascending order, into `acc`
template <int LPR, int U, bool CS>
__device__ __forceinline__ void gather_acc(const int32_t* __restrict__ indices, int64_t e0, int64_t e1, int wave_id, int n_waves,
                                           const bf16_t* __restrict__ x, int64_t ldx, int col8, bool col_ok,
                                           const float* __restrict__ col_scale, int lane, F8& acc) {
  constexpr int G = 64 / LPR;
  const int g = lane / LPR;
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(indices + base + lane) : 0;
    float my_cs = 1.f;
    if (CS) my_cs = lane < cnt ? col_scale[my_idx] : 0.f;
    for (int j = 0; j < cnt; j += G * U) {
      uint4 q[U];
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ei = j + u * G + g;
        const int src = __shfl(my_idx, ei & 63);
        if (CS) s[u] = __shfl(my_cs, ei & 63);
        const bool ok = (ei < cnt) && col_ok;
        q[u] = ok ? ld8(x + (int64_t)src * ldx + col8) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (CS) fma_u4(acc, s[u], q[u]);
        else add_u4(acc, q[u]);
      }
    }
  }
}
// the G group sums folded into lanes < LPR (fixed order)
template <int LPR>
__device__ __forceinline__ void fold_groups(F8& acc) {
#pragma unroll
  for (int m = 32; m >= LPR; m >>= 1) {
#pragma unroll
    for (int t = 0; t < 8; ++t) acc.v[t] += __shfl_xor(acc.v[t], m);
  }
}
template <int LPR, int U, bool CS>
__device__ __forceinline__ F8 gather_sum(const int32_t* __restrict__ indices, int64_t e0, int64_t e1, int wave_id, int n_waves,
                                         const bf16_t* __restrict__ x, int64_t ldx, int col8, bool col_ok,
                                         const float* __restrict__ col_scale, int lane) {
  F8 acc = zero8();
  gather_acc<LPR, U, CS>(indices, e0, e1, wave_id, n_waves, x, ldx, col8, col_ok, col_scale, lane, acc);
  fold_groups<LPR>(acc);
  return acc;
}
// SAGE "gcn" mean (acc + self) / (deg + 1), columns >= d zeroed
__device__ __forceinline__ F8 sage_mean(const F8& acc, uint4 self, int64_t deg, int col8, int d) {
  const F8 s = unpack(self);
  const float dp1 = (float)deg + 1.0f;
  const float rd = __builtin_amdgcn_rcpf(dp1);
  F8 y;
#pragma unroll
  for (int t = 0; t < 8; ++t) y.v[t] = col8 + t < d ? div_corrected(acc.v[t] + s.v[t], dp1, rd) : 0.f;
  return y;
}

// ---- stand-alone aggregation ----------------------------------------------------------------------------------------------
struct AggArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const bf16_t* x; int64_t ldx; int d;
  const float* row_scale; const float* col_scale;
  const bf16_t* x_self; int64_t ld_self; const int64_t* self_rows;
  const float* ep_scale; const float* ep_shift; int relu;
  void* out; int64_t ldo;
  int n_long_blocks; int rows_per_block;
};

// epilogue of one row (lanes < LPR with col8 < d): +self / (deg+1) or *row_scale, then scale / shift / ReLU; padding columns are 0
template <int MODE, bool OUT_BF16>
__device__ __forceinline__ void finish_row(const AggArgs& a, int64_t v, int64_t deg, const F8& acc, int col8, const F8& es, const F8& eh) {
  F8 y;
  if (MODE == GLNN_AGG_SAGE_GCN) {
    const int64_t sr = a.self_rows ? a.self_rows[v] : v;
    y = sage_mean(acc, ld8(a.x_self + sr * a.ld_self + col8), deg, col8, a.d);
  } else {
    const float rs = a.row_scale ? a.row_scale[v] : 1.0f;
#pragma unroll
    for (int t = 0; t < 8; ++t) y.v[t] = acc.v[t] * rs;
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    float z = y.v[t];
    if (a.ep_scale) z *= es.v[t];
    if (a.ep_shift) z += eh.v[t];
    if (a.relu) z = fmaxf(z, 0.f);
    y.v[t] = col8 + t < a.d ? z : 0.f;
  }
  if constexpr (OUT_BF16) {
    bf16_t* o = static_cast<bf16_t*>(a.out) + v * a.ldo + col8;
    *reinterpret_cast<uint4*>(o) = make_uint4(pack2(y.v[0], y.v[1]), pack2(y.v[2], y.v[3]), pack2(y.v[4], y.v[5]), pack2(y.v[6], y.v[7]));
  } else {
    float* o = static_cast<float*>(a.out) + v * a.ldo + col8;
    *reinterpret_cast<float4*>(o) = make_float4(y.v[0], y.v[1], y.v[2], y.v[3]);
    if (col8 + 4 < a.d) *reinterpret_cast<float4*>(o + 4) = make_float4(y.v[4], y.v[5], y.v[6], y.v[7]);   // (ldo is only >= d rounded to 4)
  }
}

template <int LPR, int U, int MODE, bool CS, bool OUT_BF16>
__global__ __launch_bounds__(kBlock) void spmm_bf16_kernel(const AggArgs a0) {
  AggArgs a = a0;
  if (gridDim.y > 1) {                                   // rows wider than 256: blockIdx.y = the 256-column tile of this workgroup
    const int off = 256 * (int)blockIdx.y;
    a.x += off;
    a.d = a0.d - off < 256 ? a0.d - off : 256;
    if (a.x_self) a.x_self += off;
    if (a.ep_scale) a.ep_scale += off;
    if (a.ep_shift) a.ep_shift += off;
    a.out = OUT_BF16 ? (void*)(static_cast<bf16_t*>(a.out) + off) : (void*)(static_cast<float*>(a.out) + off);
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col8 = (lane % LPR) * 8;
  const bool col_ok = col8 < a.d;
  F8 es, eh;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const bool ok = col8 + t < a.d;
    es.v[t] = (a.ep_scale && ok) ? a.ep_scale[col8 + t] : 1.f;
    eh.v[t] = (a.ep_shift && ok) ? a.ep_shift[col8 + t] : 0.f;
  }

  if ((int)blockIdx.x < a.n_long_blocks) {
    // long rows: chunk c of 512 rows owns the rows congruent to c modulo n_chunks (a degree-sorted order is dealt round-robin, as in
    // spmm.hip), one row at a time by all eight waves, partials folded in LDS in wave order
    __shared__ int64_t s_rows[kBlock];
    __shared__ int s_count;
    __shared__ F8 s_part[kWaves][32];
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
        const F8 acc = gather_sum<LPR, U, CS>(a.indices, e0, e1, wave, kWaves, a.x, a.ldx, col8, col_ok, a.col_scale, lane);
        if (lane < LPR) s_part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && lane < LPR && col_ok) {
          F8 t = s_part[0][lane];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) add8(t, s_part[w][lane]);
          finish_row<MODE, OUT_BF16>(a, v, e1 - e0, t, col8, es, eh);
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
    const F8 acc = gather_sum<LPR, U, CS>(a.indices, e0, e1, 0, 1, a.x, a.ldx, col8, col_ok, a.col_scale, lane);
    if (lane < LPR && col_ok) finish_row<MODE, OUT_BF16>(a, v, e1 - e0, acc, col8, es, eh);
  }
}

template <int LPR, bool OUT_BF16>
void launch_agg(const AggArgs& a, int mode, dim3 grid, hipStream_t st) {
  constexpr int U = GLNN_BF16_U;
  if (mode == GLNN_AGG_SAGE_GCN) hipLaunchKernelGGL((spmm_bf16_kernel<LPR, U, GLNN_AGG_SAGE_GCN, false, OUT_BF16>), grid, dim3(kBlock), 0, st, a);
  else if (a.col_scale) hipLaunchKernelGGL((spmm_bf16_kernel<LPR, U, GLNN_AGG_SUM, true, OUT_BF16>), grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((spmm_bf16_kernel<LPR, U, GLNN_AGG_SUM, false, OUT_BF16>), grid, dim3(kBlock), 0, st, a);
}
template <bool OUT_BF16>
void launch_agg_d(const AggArgs& a, int mode, dim3 grid, hipStream_t st) {
  const int d8 = (a.d < 256 ? a.d + 7 : 256 + 7) / 8;                   // 16-byte pieces of a row (of a 256-column tile)
  if (d8 <= 2) launch_agg<2, OUT_BF16>(a, mode, grid, st);
  else if (d8 <= 4) launch_agg<4, OUT_BF16>(a, mode, grid, st);
  else if (d8 <= 8) launch_agg<8, OUT_BF16>(a, mode, grid, st);
  else if (d8 <= 16) launch_agg<16, OUT_BF16>(a, mode, grid, st);
  else launch_agg<32, OUT_BF16>(a, mode, grid, st);
}

// ---- fused SAGE layer (K1F over bf16 rows) -----------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kFusedRows = 32;

struct FusedArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const bf16_t* x; int64_t ldx; int d_in;
  const bf16_t* x_self; int64_t ld_self;
  const float* w_packed; int d_out; int kgroups;
  const float* ep_scale; const float* ep_shift; int relu;
  void* out; int64_t ldo;
  const float* w2_packed; int d_out2; int kgroups2; void* out2; int64_t ldo2;
  const int32_t* tile_order;
};

template <bool BF16>
__device__ __forceinline__ void store1(void* base, int64_t idx, float v) {
  if constexpr (BF16) static_cast<bf16_t*>(base)[idx] = (bf16_t)f32_to_bf16_bits(v);
  else static_cast<float*>(base)[idx] = v;
}

// phase A of glnn_sage_fused_f32 over bf16 rows (the aggregate tile [32 x kpad] in LDS, fp32), phases B / C exactly its fp32 MFMA passes
template <int LPR, int U, bool OUT_BF16, bool OUT2_BF16>
__global__ __launch_bounds__(kBlock) void sage_fused_bf16_kernel(const FusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_a[];      // [32][kpad + 4]
  __shared__ F8 s_part[kWaves / 2][32];                               // 4 KiB (the fp32 kernel's LDS budget)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col8 = (lane % LPR) * 8;
  const bool col_ok = col8 < a.d_in;
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
    F8 y = zero8();
    bool deferred = false;
    if (v < a.n_dst) {
      const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
      deferred = e1 - e0 > kLongRow;
      if (!deferred) {
        const F8 acc = gather_sum<LPR, U, false>(a.indices, e0, e1, 0, 1, a.x, a.ldx, col8, col_ok, nullptr, lane);
        if (lane < LPR && col_ok) y = sage_mean(acc, ld8(a.x_self + v * a.ld_self + col8), e1 - e0, col8, a.d_in);
      }
    }
    if (!deferred && lane < LPR && col8 < kpad) {
      float* p = lds_a + lr * lda + col8;
      *reinterpret_cast<float4*>(p) = make_float4(y.v[0], y.v[1], y.v[2], y.v[3]);
      *reinterpret_cast<float4*>(p + 4) = make_float4(y.v[4], y.v[5], y.v[6], y.v[7]);
    }
  }
  __syncthreads();
  // long rows of the tile: all eight waves on one row, partials folded through four LDS slots in fixed order
#pragma unroll 1
  for (int lr = 0; lr < kFusedRows; ++lr) {
    const int64_t v = row0 + lr;
    if (v >= a.n_dst) break;
    const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
    if (e1 - e0 <= kLongRow) continue;
    const F8 acc = gather_sum<LPR, U, false>(a.indices, e0, e1, wave, kWaves, a.x, a.ldx, col8, col_ok, nullptr, lane);
    if (wave >= 4 && lane < LPR) s_part[wave - 4][lane] = acc;
    __syncthreads();
    if (wave < 4 && lane < LPR) {
      F8 t = acc;
      add8(t, s_part[wave][lane]);
      s_part[wave][lane] = t;
    }
    __syncthreads();
    if (wave == 0 && lane < LPR && col8 < kpad) {
      F8 t = s_part[0][lane], t2 = s_part[2][lane];
      add8(t, s_part[1][lane]);
      add8(t2, s_part[3][lane]);
      add8(t, t2);
      F8 y = zero8();
      if (col_ok) y = sage_mean(t, ld8(a.x_self + v * a.ld_self + col8), e1 - e0, col8, a.d_in);
      float* p = lds_a + lr * lda + col8;
      *reinterpret_cast<float4*>(p) = make_float4(y.v[0], y.v[1], y.v[2], y.v[3]);
      *reinterpret_cast<float4*>(p + 4) = make_float4(y.v[4], y.v[5], y.v[6], y.v[7]);
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
      if (a.out && col_ok2 && row < a.n_dst) store1<OUT_BF16>(a.out, row * a.ldo + col, v);
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
      if (row < a.n_dst) store1<OUT2_BF16>(a.out2, row * a.ldo2 + col2, acc[r]);
    }
  }
}

template <int LPR>
void launch_fused(const FusedArgs& a, bool out_bf16, bool out2_bf16, unsigned blocks, size_t smem, hipStream_t st) {
  constexpr int U = GLNN_BF16_U;
  if (out_bf16 && out2_bf16) hipLaunchKernelGGL((sage_fused_bf16_kernel<LPR, U, true, true>), dim3(blocks), dim3(kBlock), smem, st, a);
  else if (out_bf16) hipLaunchKernelGGL((sage_fused_bf16_kernel<LPR, U, true, false>), dim3(blocks), dim3(kBlock), smem, st, a);
  else if (out2_bf16) hipLaunchKernelGGL((sage_fused_bf16_kernel<LPR, U, false, true>), dim3(blocks), dim3(kBlock), smem, st, a);
  else hipLaunchKernelGGL((sage_fused_bf16_kernel<LPR, U, false, false>), dim3(blocks), dim3(kBlock), smem, st, a);
}

// ---- cast -------------------------------------------------------------------------------------------------------------------
// one thread per 8 output elements (one 16-byte store); the padding columns [d, d rounded up to 8) are written as 0
__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int d, bf16_t* __restrict__ out, int64_t ldo) {
  const int64_t per_row = (d + 7) / 8;
  const int64_t total = n * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row) * 8;
    const float* p = x + r * ldx + c;
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = c + t < d ? p[t] : 0.f;
    *reinterpret_cast<uint4*>(out + r * ldo + c) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
  }
}

}  // namespace

extern "C" int glnn_cast_f32_bf16(const float* x, int64_t ldx, int64_t n, int d, uint16_t* out, int64_t ldo, void* stream) {
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(x && out, "glnn_cast_f32_bf16: null pointer");
  GLNN_REQUIRE(n > 0 && d >= 1 && ldx >= d, "glnn_cast_f32_bf16: bad n / d / ldx");
  GLNN_REQUIRE(ldo % 8 == 0 && ldo >= d && glnn::aligned16(out), "glnn_cast_f32_bf16: ldo=%lld must be a multiple of 8 and >= d, out 16-byte aligned",
               (long long)ldo);
  const int64_t total = n * ((d + 7) / 8);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, ldx, n, d, out, ldo);
  return glnn::check_launch("glnn_cast_f32_bf16");
}

extern "C" int glnn_spmm_csr_bf16(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src,
                                  const uint16_t* x, int64_t ldx, int d, int mode, const float* row_scale,
                                  const float* col_scale, const uint16_t* x_self, int64_t ld_self, const int64_t* self_rows,
                                  const float* ep_scale, const float* ep_shift, int relu, void* out, int64_t ldo, int out_dtype,
                                  void* stream) {
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && x && out, "glnn_spmm_csr_bf16: null pointer");
  GLNN_REQUIRE(n_dst > 0 && n_src >= 0 && n_src < (int64_t)1 << 31, "glnn_spmm_csr_bf16: bad n_dst/n_src");
  GLNN_REQUIRE(d >= 1, "glnn_spmm_csr_bf16: d=%d must be >= 1", d);
  GLNN_REQUIRE(mode == GLNN_AGG_SUM || mode == GLNN_AGG_SAGE_GCN, "glnn_spmm_csr_bf16: unknown mode %d", mode);
  GLNN_REQUIRE(out_dtype == GLNN_DTYPE_F32 || out_dtype == GLNN_DTYPE_BF16, "glnn_spmm_csr_bf16: unknown out_dtype %d", out_dtype);
  const int d8 = (d + 7) & ~7;
  const int dpad_out = out_dtype == GLNN_DTYPE_BF16 ? d8 : (d + 3) & ~3;
  const int out_align = out_dtype == GLNN_DTYPE_BF16 ? 8 : 4;
  GLNN_REQUIRE(ldx % 8 == 0 && ldx >= d8, "glnn_spmm_csr_bf16: ldx=%lld must be a multiple of 8 and >= %d", (long long)ldx, d8);
  GLNN_REQUIRE(ldo % out_align == 0 && ldo >= dpad_out, "glnn_spmm_csr_bf16: ldo=%lld must be a multiple of %d and >= %d", (long long)ldo,
               out_align, dpad_out);
  GLNN_REQUIRE(glnn::aligned16(x) && glnn::aligned16(out), "glnn_spmm_csr_bf16: x/out must be 16-byte aligned");
  if (mode == GLNN_AGG_SAGE_GCN) {
    GLNN_REQUIRE(x_self && ld_self % 8 == 0 && ld_self >= d8 && glnn::aligned16(x_self), "glnn_spmm_csr_bf16: SAGE_GCN needs x_self with ld multiple of 8");
    GLNN_REQUIRE(!row_scale && !col_scale, "glnn_spmm_csr_bf16: scales are not used in SAGE_GCN mode");
  } else {
    GLNN_REQUIRE(!self_rows, "glnn_spmm_csr_bf16: self_rows belongs to SAGE_GCN mode");
  }
  const int col_tiles = (d + 255) / 256;
  GLNN_REQUIRE(col_tiles <= 65535, "glnn_spmm_csr_bf16: d too large");
  AggArgs a;
  a.indptr = indptr; a.indices = indices; a.n_dst = n_dst; a.x = x; a.ldx = ldx; a.d = d;
  a.row_scale = row_scale; a.col_scale = col_scale; a.x_self = mode == GLNN_AGG_SAGE_GCN ? x_self : nullptr; a.ld_self = ld_self;
  a.self_rows = self_rows; a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.relu = relu; a.out = out; a.ldo = ldo;
  int64_t n_long = (n_dst + kLongBlockRows - 1) / kLongBlockRows;
  if (n_long > kLongBlockCap) n_long = kLongBlockCap;
  a.n_long_blocks = (int)n_long;
  int64_t rpw = n_dst / (2048 * kWaves);
  if (rpw < 1) rpw = 1;
  if (rpw > kRowsPerWave) rpw = kRowsPerWave;
  a.rows_per_block = (int)(kWaves * rpw);
  const int64_t row_blocks = (n_dst + a.rows_per_block - 1) / a.rows_per_block;
  GLNN_REQUIRE(row_blocks + n_long < ((int64_t)1 << 31), "glnn_spmm_csr_bf16: n_dst too large for one launch");
  const dim3 grid((unsigned)(row_blocks + n_long), (unsigned)col_tiles);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (out_dtype == GLNN_DTYPE_BF16) launch_agg_d<true>(a, mode, grid, st);
  else launch_agg_d<false>(a, mode, grid, st);
  return glnn::check_launch("glnn_spmm_csr_bf16");
}

extern "C" int glnn_sage_fused_bf16(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const uint16_t* x,
                                    int64_t ldx, int d_in, const uint16_t* x_self, int64_t ld_self, const float* w_packed,
                                    int d_out, const float* ep_scale, const float* ep_shift, int relu, void* out,
                                    int64_t ldo, int out_dtype, const float* w2_packed, int d_out2, void* out2, int64_t ldo2,
                                    int out2_dtype, const int32_t* tile_order, void* stream) {
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && x && x_self && w_packed && (out || w2_packed), "glnn_sage_fused_bf16: null pointer");
  GLNN_REQUIRE((out_dtype == GLNN_DTYPE_F32 || out_dtype == GLNN_DTYPE_BF16) && (out2_dtype == GLNN_DTYPE_F32 || out2_dtype == GLNN_DTYPE_BF16),
               "glnn_sage_fused_bf16: unknown out_dtype / out2_dtype");
  GLNN_REQUIRE(!w2_packed || (out2 && d_out2 >= 1 && d_out2 <= 256 && ldo2 >= d_out2 && glnn::aligned16(w2_packed)),
               "glnn_sage_fused_bf16: the chained projection needs out2 with ldo2 >= d_out2 in [1,256]");
  GLNN_REQUIRE(n_dst > 0 && n_src >= 0 && n_src < (int64_t)1 << 31, "glnn_sage_fused_bf16: bad n_dst/n_src");
  GLNN_REQUIRE(d_in >= 1 && d_in <= 256 && d_out >= 1 && d_out <= 256, "glnn_sage_fused_bf16: d_in and d_out must be in [1,256]");
  const int d8 = (d_in + 7) & ~7;
  GLNN_REQUIRE(ldx % 8 == 0 && ldx >= d8 && ld_self % 8 == 0 && ld_self >= d8 && (!out || ldo >= d_out),
               "glnn_sage_fused_bf16: leading dimensions (ldx, ld_self multiples of 8 and >= %d; ldo >= d_out)", d8);
  GLNN_REQUIRE(glnn::aligned16(x) && glnn::aligned16(x_self) && glnn::aligned16(w_packed), "glnn_sage_fused_bf16: 16-byte alignment required");
  const int64_t blocks = (n_dst + kFusedRows - 1) / kFusedRows;
  GLNN_REQUIRE(blocks < ((int64_t)1 << 31), "glnn_sage_fused_bf16: n_dst too large for one launch");
  FusedArgs a;
  a.indptr = indptr; a.indices = indices; a.n_dst = n_dst; a.x = x; a.ldx = ldx; a.d_in = d_in; a.x_self = x_self; a.ld_self = ld_self;
  a.w_packed = w_packed; a.d_out = d_out; a.kgroups = (d_in + 7) / 8; a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.relu = relu;
  a.out = out; a.ldo = ldo;
  a.w2_packed = w2_packed; a.d_out2 = w2_packed ? d_out2 : 0; a.kgroups2 = w2_packed ? (d_out + 7) / 8 : 0; a.out2 = out2; a.ldo2 = ldo2;
  a.tile_order = tile_order;
  const int kg_lds = a.kgroups2 > a.kgroups ? a.kgroups2 : a.kgroups;
  const size_t smem = sizeof(float) * kFusedRows * (kg_lds * 8 + 4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool ob = out_dtype == GLNN_DTYPE_BF16, o2b = out2_dtype == GLNN_DTYPE_BF16;
  // LPR * 8 >= kpad (a multiple of 8): every column of the LDS tile is written by phase A
  const int k8 = a.kgroups;
  if (k8 <= 2) launch_fused<2>(a, ob, o2b, (unsigned)blocks, smem, st);
  else if (k8 <= 4) launch_fused<4>(a, ob, o2b, (unsigned)blocks, smem, st);
  else if (k8 <= 8) launch_fused<8>(a, ob, o2b, (unsigned)blocks, smem, st);
  else if (k8 <= 16) launch_fused<16>(a, ob, o2b, (unsigned)blocks, smem, st);
  else launch_fused<32>(a, ob, o2b, (unsigned)blocks, smem, st);
  return glnn::check_launch("glnn_sage_fused_bf16");
}
