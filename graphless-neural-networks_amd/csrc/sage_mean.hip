// KM: the GraphSAGE "mean" aggregator for gfx950 (MI355X) -- docs/SAGE_MEAN_SEMANTICS.md.
//
//   out[v] = epi( fc_neigh( (1 / max(deg(v), 1)) * sum_{u->v} x[u] ) + fc_self(x_self[v]) )
//
// Replaces dgl 0.6.1 SAGEConv(aggregator_type="mean") (see include/glnn_hip.h); the reference has no call site -- it only builds "gcn".
//
//   sage_mean_fused_kernel   aggregate-first layers (d_in <= d_out <= 256), ONE launch per layer.  A workgroup of 8 waves owns a tile of 32
//     destination rows:
//       phase A  row_gather_dev.h's 32-row tile: a wave gathers and sums one row's in-neighbours, scales by 1 / max(deg, 1) and parks the
//                row in LDS columns [0, kpad); the row's SELF row goes beside it, columns [kpad, 2 kpad);
//       phase B  wave w multiplies the [32 x 2 kpad] tile with the w-th 32-column panel of W_cat = [W_neigh | W_self] on the fp32 MFMA
//                (v_mfma_f32_32x32x2_f32) -- one product over K = 2 kpad.  W_cat arrives packed in B-fragment order (glnn_pack_weight_f32 of
//                the concatenation), one coalesced 1 KiB load per k-group and wave from L2;
//       epilogue per-column scale / shift and ReLU, stored from the accumulators.
//     Neither the mean rows nor a second product's output reach HBM.
//   spmm_sage_mean_kernel    the project-first form (d_in > d_out) and the general fallback: out = epi(mean of x rows + s), x and s the two
//     halves of ONE projection of the source rows against the stacked [W_neigh; W_self].  Phase A of the fused kernel with a store instead
//     of the LDS tile.
//
// No float atomics and no grid barrier: a row's value is a fixed-order sum over its own edges (one wave, or eight waves with a fixed split
// and fold), so results are bit-identical run to run and do not depend on which other rows are in the launch or on the tile order.
#include "row_gather_dev.h"

namespace {

constexpr int kMaxD = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// stream-once data (output rows) with the non-temporal hint: it must not evict the re-used feature rows
__device__ __forceinline__ void st4_stream(float* p, float4 v) {
  f32x4_t t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t*>(p));
}

struct MeanArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_dst;
  const float* x; int64_t ldx; int d_in;                                  // the gathered rows
  const float* x_self; int64_t ld_self; const int64_t* self_rows;         // fused: the self rows (optional indirection); stand-alone: s
  const float* w_packed; int d_out; int kgroups;                          // kgroups = ceil(d_in / 8) PER HALF of W_cat
  const float* ep_scale; const float* ep_shift; int relu;
  float* out; int64_t ldo;
  const int32_t* tile_order;
};

// phase A of both kernels.  finish(lr, v, deg, sum, valid): row_gather_dev.h gather_tile
template <int LPR, class Fin>
__device__ __forceinline__ void aggregate_tile(const MeanArgs& a, int64_t row0, int lane, int wave, int col4, bool col_ok, int* s_next,
                                               float4* s_part, Fin&& finish) {
  NormRows<false> ld;
  ld.x = a.x; ld.ldx = a.ldx; ld.x_norm = nullptr; ld.col4 = col4; ld.col_ok = col_ok;
  gather_tile<LPR>(a.indptr, a.indices, a.n_dst, row0, lane, wave, s_next, s_part, ld, finish);
}
__device__ __forceinline__ float inv_deg(int64_t deg) { return 1.0f / (float)(deg > 1 ? deg : 1); }

// dynamic LDS (all of the kernel's LDS, so that its base stays 16-byte aligned): [tile floats][4 x 64 float4 fold slots][ticket]
__host__ __device__ inline size_t fold_bytes() { return sizeof(float4) * 4 * 64 + 16; }

template <int LPR>
__global__ __launch_bounds__(kBlock) void sage_mean_fused_kernel(const MeanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_a[];      // [32][2 kpad + 4]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d_in;
  const int kpad = a.kgroups * 8;
  const int lda = 2 * kpad + 4;      // (2 kpad + 4) % 64 == 4 for kpad % 32 == 0: row r of a fragment read starts 4 banks after row r - 1
  float4* s_part = reinterpret_cast<float4*>(lds_a + kTileRows * lda);
  int* s_next = reinterpret_cast<int*>(s_part + 4 * 64);
  const int tile_id = a.tile_order ? a.tile_order[blockIdx.x] : (int)blockIdx.x;
  const int64_t row0 = (int64_t)tile_id * kTileRows;
  if (threadIdx.x == 0) *s_next = 0;
  __syncthreads();

  aggregate_tile<LPR>(a, row0, lane, wave, col4, col_ok, s_next, s_part,
                      [&](int lr, int64_t v, int64_t deg, float4 sum, bool valid) {      // (rows past n_dst too: zeros are parked)
                        if (lane >= LPR || col4 >= kpad) return;      // (LPR * 4 >= kpad: the lanes < LPR cover the padded row)
                        float4 m = zero4(), s = zero4();
                        if (valid && col_ok) {
                          const float inv = inv_deg(deg);
                          m = mask_cols(make_float4(sum.x * inv, sum.y * inv, sum.z * inv, sum.w * inv), col4, a.d_in);
                          const int64_t sr = a.self_rows ? a.self_rows[v] : v;
                          s = mask_cols(ld4(a.x_self + sr * a.ld_self + col4), col4, a.d_in);
                        }
                        st4(lds_a + lr * lda + col4, m);
                        st4(lds_a + lr * lda + kpad + col4, s);
                      });

  // ---- phase B: [32 x 2 kpad] (LDS) x W_cat panel `wave` (packed, L2) on the MFMA ----------------------------------------------
  const int n_tiles = (a.d_out + 31) / 32;
  const int nt = wave;
  if (nt >= n_tiles) return;
  const int li = lane & 31, kk = lane >> 5;
  const int kg_all = 2 * a.kgroups;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  {
    const float4* wp = reinterpret_cast<const float4*>(a.w_packed) + ((int64_t)nt * kg_all) * 64 + lane;
    const float* ap = lds_a + li * lda + kk * 4;
    constexpr int PF = 4;                      // B fragments in flight
    float4 bq[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) bq[q] = (q < kg_all) ? wp[(int64_t)q * 64] : zero4();
    for (int kg0 = 0; kg0 < kg_all; kg0 += PF) {
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int kg = kg0 + q;
        if (kg < kg_all) {
          const float4 bv = bq[q];
          const int nxt = kg + PF;
          if (nxt < kg_all) bq[q] = wp[(int64_t)nxt * 64];
          const float4 av = ld4(ap + kg * 8);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
        }
      }
    }
  }
  // ---- epilogue: C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -----------------------
  const int col = nt * 32 + li;
  const bool col_live = col < a.d_out;
  const int dpad_out = (a.d_out + 3) & ~3;
  if (col >= dpad_out || col >= a.ldo) return;      // (the padding columns of a float4-addressable output row come out as zeros)
  const float es = (a.ep_scale && col_live) ? a.ep_scale[col] : 1.f;
  const float eh = (a.ep_shift && col_live) ? a.ep_shift[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
    float v = fmaf(acc[r], es, eh);
    if (a.relu) v = fmaxf(v, 0.f);
    if (!col_live) v = 0.f;
    if (row < a.n_dst) a.out[row * a.ldo + col] = v;
  }
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void spmm_sage_mean_kernel(const MeanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_a[];
  float4* s_part = reinterpret_cast<float4*>(lds_a);
  int* s_next = reinterpret_cast<int*>(s_part + 4 * 64);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d_in;
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  float es[4], eh[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bool ok = col4 + t < a.d_in;
    es[t] = (a.ep_scale && ok) ? a.ep_scale[col4 + t] : 1.f;
    eh[t] = (a.ep_shift && ok) ? a.ep_shift[col4 + t] : 0.f;
  }
  if (threadIdx.x == 0) *s_next = 0;
  __syncthreads();
  aggregate_tile<LPR>(a, row0, lane, wave, col4, col_ok, s_next, s_part,
                      [&](int, int64_t v, int64_t deg, float4 sum, bool valid) {
                        if (!valid || lane >= LPR || !col_ok) return;
                        const float inv = inv_deg(deg);
                        const float4 s = ld4(a.x_self + v * a.ld_self + col4);
                        float o[4] = {sum.x * inv + s.x, sum.y * inv + s.y, sum.z * inv + s.z, sum.w * inv + s.w};
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                          o[t] = fmaf(o[t], es[t], eh[t]);
                          if (a.relu) o[t] = fmaxf(o[t], 0.f);
                        }
                        st4_stream(a.out + v * a.ldo + col4, mask_cols(make_float4(o[0], o[1], o[2], o[3]), col4, a.d_in));
                      });
}

// dynamic LDS above the 64 KB default needs the attribute once per kernel and device
template <class K>
int configure_lds(K kernel, size_t smem, int* configured_mask, const char* who) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return glnn::fail(GLNN_ERR_NO_DEVICE, "%s: no HIP device", who);
  if (dev < 0 || dev >= 32) dev = 31;
  if (dev != 31 && ((*configured_mask >> dev) & 1)) return GLNN_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
    (void)hipGetLastError();
    return glnn::fail(GLNN_ERR_HIP, "%s: hipFuncSetAttribute(max dynamic LDS=%zu) failed", who, smem);
  }
  if (dev != 31) *configured_mask |= 1 << dev;
  return GLNN_OK;
}

template <int LPR>
int launch_fused(const MeanArgs& a, unsigned blocks, size_t smem, hipStream_t st) {
  static int configured = 0;
  constexpr size_t smem_max = sizeof(float) * kTileRows * (2 * kMaxD + 4) + sizeof(float4) * 4 * 64 + 16;
  const int rc = configure_lds(sage_mean_fused_kernel<LPR>, smem_max, &configured, "glnn_sage_mean_fused_f32");
  if (rc != GLNN_OK) return rc;
  hipLaunchKernelGGL((sage_mean_fused_kernel<LPR>), dim3(blocks), dim3(kBlock), smem, st, a);
  return glnn::check_launch("glnn_sage_mean_fused_f32");
}

}  // namespace

extern "C" int glnn_sage_mean_fused_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const float* x,
                                        int64_t ldx, int d_in, const float* x_self, int64_t ld_self, const int64_t* self_rows,
                                        const float* w_cat_packed, int d_out, const float* ep_scale, const float* ep_shift, int relu,
                                        float* out, int64_t ldo, const int32_t* tile_order, void* stream) {
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && x && x_self && w_cat_packed && out, "glnn_sage_mean_fused_f32: null pointer");      // indices NULL iff no edges
  GLNN_REQUIRE(n_dst > 0 && n_src >= 0 && n_src < (int64_t)1 << 31, "glnn_sage_mean_fused_f32: bad n_dst/n_src");
  GLNN_REQUIRE(d_in >= 1 && d_out >= 1, "glnn_sage_mean_fused_f32: d_in and d_out must be positive");
  if (d_in > d_out || d_out > kMaxD)
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "glnn_sage_mean_fused_f32: aggregate-first layers with d_in <= d_out <= %d only (got %d -> %d)",
                      kMaxD, d_in, d_out);
  const int dpad = (d_in + 3) & ~3;
  GLNN_REQUIRE(ldx % 4 == 0 && ldx >= dpad && ld_self % 4 == 0 && ld_self >= dpad && ldo >= d_out,
               "glnn_sage_mean_fused_f32: leading dimensions (ldx, ld_self multiples of 4 and >= %d; ldo >= d_out)", dpad);
  GLNN_REQUIRE(glnn::aligned16(x) && glnn::aligned16(x_self) && glnn::aligned16(w_cat_packed),
               "glnn_sage_mean_fused_f32: 16-byte alignment required");
  MeanArgs a = {};
  a.indptr = indptr; a.indices = indices; a.n_dst = n_dst; a.x = x; a.ldx = ldx; a.d_in = d_in; a.x_self = x_self; a.ld_self = ld_self;
  a.self_rows = self_rows; a.w_packed = w_cat_packed; a.d_out = d_out; a.kgroups = (d_in + 7) / 8; a.ep_scale = ep_scale;
  a.ep_shift = ep_shift; a.relu = relu; a.out = out; a.ldo = ldo; a.tile_order = tile_order;
  const int64_t blocks = (n_dst + kTileRows - 1) / kTileRows;
  GLNN_REQUIRE(blocks < ((int64_t)1 << 31), "glnn_sage_mean_fused_f32: n_dst too large for one launch");
  const size_t smem = sizeof(float) * kTileRows * (2 * a.kgroups * 8 + 4) + fold_bytes();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // float4 per padded half row: LPR * 4 >= kpad
  return with_lpr<16>(lpr_for(a.kgroups * 2, 16), [&](auto L) { return launch_fused<decltype(L)::value>(a, (unsigned)blocks, smem, st); });
}

extern "C" int glnn_spmm_sage_mean_f32(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const float* x,
                                       int64_t ldx, int d, const float* s, int64_t lds, const float* ep_scale, const float* ep_shift,
                                       int relu, float* out, int64_t ldo, void* stream) {
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && x && s && out, "glnn_spmm_sage_mean_f32: null pointer");      // indices NULL iff no edges
  GLNN_REQUIRE(n_dst > 0 && n_src >= 0 && n_src < (int64_t)1 << 31, "glnn_spmm_sage_mean_f32: bad n_dst/n_src");
  GLNN_REQUIRE(d >= 1, "glnn_spmm_sage_mean_f32: d must be positive");
  if (d > kMaxD) return glnn::fail(GLNN_ERR_UNSUPPORTED, "glnn_spmm_sage_mean_f32: rows of at most %d floats (got %d)", kMaxD, d);
  const int dpad = (d + 3) & ~3;
  GLNN_REQUIRE(ldx % 4 == 0 && ldx >= dpad && lds % 4 == 0 && lds >= dpad && ldo % 4 == 0 && ldo >= dpad,
               "glnn_spmm_sage_mean_f32: leading dimensions (ldx, lds, ldo multiples of 4 and >= %d)", dpad);
  GLNN_REQUIRE(glnn::aligned16(x) && glnn::aligned16(s) && glnn::aligned16(out), "glnn_spmm_sage_mean_f32: 16-byte alignment required");
  MeanArgs a = {};
  a.indptr = indptr; a.indices = indices; a.n_dst = n_dst; a.x = x; a.ldx = ldx; a.d_in = d; a.x_self = s; a.ld_self = lds;
  a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.relu = relu; a.out = out; a.ldo = ldo;
  const int64_t blocks = (n_dst + kTileRows - 1) / kTileRows;
  GLNN_REQUIRE(blocks < ((int64_t)1 << 31), "glnn_spmm_sage_mean_f32: n_dst too large for one launch");
  const size_t smem = fold_bytes();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_lpr<16>(lpr_for(dpad / 4, 16), [&](auto L) {
    hipLaunchKernelGGL((spmm_sage_mean_kernel<decltype(L)::value>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a);
  });
  return glnn::check_launch("glnn_spmm_sage_mean_f32");
}
