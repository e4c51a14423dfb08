// GCNII (Chen et al., "Simple and Deep Graph Convolutional Networks", ICML 2020; docs/GCNII_SEMANTICS.md) for gfx950 (MI355X): one launch
// per conv layer and direction over P = D_in^-1/2 A D_out^-1/2 (prop_dev.h: what the three files over P share).
//
//   forward   S = (1 - alpha) P drop(H_{l-1}) + alpha H_0          (eq. 5: initial residual)
//             H_l = relu((1 - beta) S + beta S W^T)                 (eq. 5: identity mapping)
//   backward  dZ = [H_l > 0] drop'((1 - alpha) P^T dS_{l+1})        (layer L: drop'(dH_L), loaded, not gathered)
//             dS = (1 - beta) dZ + beta dZ W,   dh0_acc (+)= alpha dS
//
//   gcnii_layer_kernel   A workgroup of 8 waves owns a tile of 32 rows:
//       phase A  row_gather_dev.h's 32-row tile: a wave gathers and sums one row's neighbours (the per-source norm, when the rows are not
//                pre-scaled, rides along with the index), applies the row's own terms (norm, dropout mask keyed by the own row, residual
//                row, ReLU mask) and parks the row T in LDS columns [0, kpad); the training forward streams it to `t_out` (S, for the
//                weight gradient), the backward stores t_scale T (beta dZ, the other operand).  The plain form loads the tile's own rows
//                instead of gathering: a ticket loop of its own, since it reads no CSR;
//       phase B  wave w multiplies the [32 x kpad] tile with the w-th 32-column panel of the packed weight (glnn_pack_weight_f32 of W
//                forward, of W^T backward) on the fp32 MFMA (v_mfma_f32_32x32x2_f32), one coalesced 1 KiB load per k-group from L2;
//       epilogue (1 - beta) T + beta acc with T read back from LDS at the accumulator's (row, col); ReLU (forward); the backward also
//                updates dh0_acc -- a row is one workgroup's per launch and the launches of a step are serial.
//     w_packed NULL (the backward's last launch, dH_0): phase A alone, T is the result.
//
// No float atomics and no grid barrier: a row's value is a fixed-order sum over its own edges (one wave, or eight waves with a fixed split
// and fold), so results are bit-identical run to run and do not depend on which other rows are in the launch or on the tile order.
#include "prop_dev.h"

namespace {

constexpr int kMaxD = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float4 mul4(float s, float4 v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }
// the feature dropout of the package on four adjacent columns of `row` (col4 % 4 == 0: two hashes, 16 bits per element)
__device__ __forceinline__ float4 drop4(float4 v, uint32_t seed, uint32_t thr, float dscale, uint32_t row, int col4) {
  const uint32_t h0 = glnn::drop_hash(seed, row, (uint32_t)col4 >> 1), h1 = glnn::drop_hash(seed, row, ((uint32_t)col4 >> 1) + 1u);
  return make_float4((h0 & 0xFFFFu) >= thr ? v.x * dscale : 0.f, (h0 >> 16) >= thr ? v.y * dscale : 0.f,
                     (h1 & 0xFFFFu) >= thr ? v.z * dscale : 0.f, (h1 >> 16) >= thr ? v.w * dscale : 0.f);
}

struct GcniiArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n; int d; int kgroups;      // kgroups = ceil(d / 8)
  const float* x; int64_t ldx;          // the gathered rows (plain: the tile's own rows)
  const float* x_norm;                  // non-NULL: x is UNSCALED, each gathered row is multiplied by x_norm[source]
  const float* row_norm; float c;       // T = c row_norm[v] sum   (plain: T = the row)
  uint32_t src_thr, own_thr, seed; float dscale;      // dropout keyed by the SOURCE row (training forward) or by the OWN row (backward)
  const float* add; int64_t ldadd; float add_scale;   // T += add_scale add[v]   (forward: alpha H_0; dH_0 launch: dh0_acc)
  const float* hmask; int64_t ldh;      // T = 0 where hmask[v] <= 0 (the saved H_l)
  float* t_out; int64_t ldt; float t_scale;           // t_out[v] = t_scale T
  const float* w_packed; float beta;
  float* out; int64_t ldo; const float* out_norm; int relu;
  float* dh0_acc; int64_t ldacc; float alpha; int first;
  const int32_t* tile_order; int plain;
};

// the gathered rows; DROP: the training forward's mask, keyed by the SOURCE row, on every loaded element before it enters the sum
template <bool XN, bool DROP>
struct LayerRows : NormRows<XN> {
  uint32_t seed, thr; float dscale;
  __device__ __forceinline__ float4 add(float4 acc, float4 v, int src, float w) const {
    if (DROP) v = drop4(v, seed, thr, dscale, (uint32_t)src, this->col4);
    return NormRows<XN>::add(acc, v, src, w);
  }
};

// dynamic LDS (all of the kernel's LDS, so that its base stays 16-byte aligned): [tile floats][4 x 64 float4 fold slots][ticket]
__host__ __device__ inline size_t fold_bytes() { return sizeof(float4) * 4 * 64 + 16; }

template <int LPR, bool XN, bool DROP>
__global__ __launch_bounds__(kBlock) void gcnii_layer_kernel(const GcniiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_a[];      // [32][kpad + 4]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  const int kpad = a.kgroups * 8;
  const int lda = kpad + 4;          // (kpad + 4) % 64 == 4 for kpad % 32 == 0: row r of a fragment read starts 4 banks after row r - 1
  float4* s_part = reinterpret_cast<float4*>(lds_a + kTileRows * lda);
  int* s_next = reinterpret_cast<int*>(s_part + 4 * 64);
  const int tile_id = a.tile_order ? a.tile_order[blockIdx.x] : (int)blockIdx.x;
  const int64_t row0 = (int64_t)tile_id * kTileRows;
  if (threadIdx.x == 0) *s_next = 0;
  __syncthreads();

  // ---- phase A ------------------------------------------------------------------------------------------------------------------
  // called by ONE whole wave per tile row lr (valid == false: the row is past n); `sum` is in the lanes < LPR
  auto finish = [&](int lr, int64_t v, int64_t, float4 sum, bool valid) {
    if (lane >= LPR || col4 >= kpad) return;      // (LPR * 4 >= kpad: the lanes < LPR cover the padded row)
    float4 t = zero4();
    if (valid && col_ok) {
      t = a.plain ? sum : mul4(a.c * a.row_norm[v], sum);
      if (a.own_thr) t = drop4(t, a.seed, a.own_thr, a.dscale, (uint32_t)v, col4);
      if (a.add) t = fma4(a.add_scale, ld4(a.add + v * a.ldadd + col4), t);
      if (a.hmask) {
        const float4 h = ld4(a.hmask + v * a.ldh + col4);
        t = make_float4(h.x > 0.f ? t.x : 0.f, h.y > 0.f ? t.y : 0.f, h.z > 0.f ? t.z : 0.f, h.w > 0.f ? t.w : 0.f);
      }
      t = mask_cols(t, col4, a.d);
      if (a.t_out) st4(a.t_out + v * a.ldt + col4, mul4(a.t_scale, t));
    }
    st4(lds_a + lr * lda + col4, t);
  };
  if (a.plain) {
#pragma unroll 1
    for (int lr = tile_ticket(s_next, lane); lr < kTileRows; lr = tile_ticket(s_next, lane)) {
      const int64_t v = row0 + lr;
      finish(lr, v, 0, (v < a.n && lane < LPR && col_ok) ? ld4(a.x + v * a.ldx + col4) : zero4(), v < a.n);
    }
    __syncthreads();
  } else {
    LayerRows<XN, DROP> ld;
    ld.x = a.x; ld.ldx = a.ldx; ld.x_norm = a.x_norm; ld.col4 = col4; ld.col_ok = col_ok;
    ld.seed = a.seed; ld.thr = a.src_thr; ld.dscale = a.dscale;
    gather_tile<LPR>(a.indptr, a.indices, a.n, row0, lane, wave, s_next, s_part, ld, finish);
  }
  if (!a.w_packed) return;      // the dH_0 launch: T (stored through t_out) is the result

  // ---- phase B: [32 x kpad] (LDS) x weight panel `wave` (packed, L2) on the MFMA ----------------------------------------------------
  const int n_tiles = (a.d + 31) / 32;
  const int nt = wave;
  if (nt >= n_tiles) return;
  const int li = lane & 31, kk = lane >> 5;
  const int kg_all = a.kgroups;
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
  // ---- epilogue: C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ---------------------------
  const int col = nt * 32 + li;
  const bool col_live = col < a.d;
  if (col >= ((a.d + 3) & ~3)) return;      // (the padding columns of a float4-addressable row come out as zeros)
  const float omb = 1.f - a.beta;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rl = (r & 3) + 8 * (r >> 2) + 4 * kk;
    const int64_t row = row0 + rl;
    if (row >= a.n) continue;
    float v = fmaf(a.beta, acc[r], omb * lds_a[rl * lda + col]);
    if (a.relu) v = fmaxf(v, 0.f);
    if (!col_live) v = 0.f;
    if (a.dh0_acc) {
      float* p = a.dh0_acc + row * a.ldacc + col;
      *p = a.first ? a.alpha * v : fmaf(a.alpha, v, *p);
    }
    a.out[row * a.ldo + col] = a.out_norm ? a.out_norm[row] * v : v;
  }
}

// the geometry depends on d alone (LPR, the LDS tile) and on ceil(n / 32): no branch on n
int launch(GcniiArgs& a, const char* what, void* stream) {
  a.kgroups = (a.d + 7) / 8;
  const int64_t blocks = (a.n + kTileRows - 1) / kTileRows;
  GLNN_REQUIRE(blocks < ((int64_t)1 << 31), "%s: n too large for one launch", what);
  const size_t smem = sizeof(float) * kTileRows * (a.kgroups * 8 + 4) + fold_bytes();      // <= 37392 bytes at d = 256
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // DROP: the training forward, the source-keyed mask on every gathered element.  float4 per padded row: LPR * 4 >= kpad
  with_prop_variant<16>(a.x_norm != nullptr, a.src_thr != 0, lpr_for(a.kgroups * 2, 16), [&](auto XN, auto DROP, auto L) {
    hipLaunchKernelGGL((gcnii_layer_kernel<decltype(L)::value, decltype(XN)::value, decltype(DROP)::value>), dim3((unsigned)blocks),
                       dim3(kBlock), smem, st, a);
  });
  return glnn::check_launch(what);
}

// the first checks of both entries, in their order
int entry_checks(const char* what, int64_t n, int d, int64_t nnz, float drop_p) {
  GLNN_TRY(prop_sizes_ok(what, n, d, nnz));
  GLNN_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p must be in [0, 1)", what);
  GLNN_TRY(prop_nnz_ok(what, nnz, GLNN_ERR_UNSUPPORTED, "CSR positions"));
  if (d > kMaxD) return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: hidden widths of at most %d (got %d)", what, kMaxD, d);
  return GLNN_OK;
}

}  // namespace

extern "C" int glnn_gcnii_layer_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* x, int64_t ldx,
                                    int d, const float* x_norm, const float* row_norm, const float* out_norm, const float* h0,
                                    int64_t ldh0, float alpha, float beta, const float* w_packed, float drop_p, uint32_t drop_seed,
                                    float* s_out, int64_t lds, float* out, int64_t ldo, const int32_t* tile_order, void* stream) {
  const char* what = "glnn_gcnii_layer_f32";
  GLNN_TRY(entry_checks(what, n, d, nnz, drop_p));
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && (indices || nnz == 0) && x && row_norm && h0 && w_packed && out, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(x, ldx, d) && rows_ok(h0, ldh0, d) && rows_ok(s_out, lds, d) && rows_ok(out, ldo, d) && glnn::aligned16(w_packed),
               kRowsText, what);
  GLNN_REQUIRE(out != x && out != h0 && (!s_out || (s_out != x && s_out != h0 && s_out != out)), "%s: out / s_out must not alias an input",
               what);
  GcniiArgs a = {};
  a.indptr = indptr; a.indices = indices; a.n = n; a.d = d; a.x = x; a.ldx = ldx; a.x_norm = x_norm; a.row_norm = row_norm;
  a.c = 1.f - alpha; a.src_thr = glnn::drop_threshold(drop_p); a.seed = drop_seed; a.dscale = 1.0f / (1.0f - drop_p);
  a.add = h0; a.ldadd = ldh0; a.add_scale = alpha; a.t_out = s_out; a.ldt = lds; a.t_scale = 1.f; a.w_packed = w_packed; a.beta = beta;
  a.out = out; a.ldo = ldo; a.out_norm = out_norm; a.relu = 1; a.tile_order = tile_order;
  return launch(a, what, stream);
}

extern "C" int glnn_gcnii_layer_bwd_f32(const int64_t* t_indptr, const int32_t* t_indices, int64_t n, int64_t nnz, const float* g,
                                        int64_t ldg, int d, const float* x_norm, const float* row_norm, const float* out_norm, int plain,
                                        const float* h, int64_t ldh, float drop_p, uint32_t drop_seed, float alpha, float beta,
                                        const float* wt_packed, float dz_scale, float* dz_out, int64_t lddz, float* ds_out, int64_t ldds,
                                        float* dh0_acc, int64_t ldacc, int first, const int32_t* tile_order, void* stream) {
  const char* what = "glnn_gcnii_layer_bwd_f32";
  GLNN_TRY(entry_checks(what, n, d, nnz, drop_p));
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(g && dz_out && dh0_acc && (h || !wt_packed), "%s: null pointer", what);
  GLNN_REQUIRE(plain || (t_indptr && (t_indices || nnz == 0) && row_norm), "%s: null pointer (the gather form needs the transposed CSR)", what);
  GLNN_REQUIRE((wt_packed == nullptr) == (ds_out == nullptr), "%s: wt_packed and ds_out go together (both NULL: the dH_0 launch)", what);
  GLNN_REQUIRE(wt_packed || (!plain && !first), "%s: the dH_0 launch is a gather behind at least one layer launch", what);
  GLNN_REQUIRE(rows_ok(g, ldg, d) && rows_ok(h, ldh, d) && rows_ok(dz_out, lddz, d) && rows_ok(ds_out, ldds, d) && rows_ok(dh0_acc, ldacc, d) &&
               glnn::aligned16(wt_packed), kRowsText, what);
  GLNN_REQUIRE(dz_out != g && ds_out != g && dh0_acc != g && dz_out != ds_out && dz_out != dh0_acc && (!ds_out || ds_out != dh0_acc) &&
               (!h || (h != dz_out && h != ds_out && h != dh0_acc)), "%s: outputs must not alias an input or each other", what);
  GcniiArgs a = {};
  a.indptr = t_indptr; a.indices = t_indices; a.n = n; a.d = d; a.x = g; a.ldx = ldg; a.x_norm = plain ? nullptr : x_norm;
  a.row_norm = row_norm; a.c = 1.f - alpha; a.own_thr = glnn::drop_threshold(drop_p); a.seed = drop_seed; a.dscale = 1.0f / (1.0f - drop_p);
  a.hmask = h; a.ldh = ldh; a.t_out = dz_out; a.ldt = lddz; a.t_scale = dz_scale; a.w_packed = wt_packed; a.beta = beta;
  a.out = ds_out; a.ldo = ldds; a.out_norm = out_norm; a.tile_order = tile_order; a.plain = plain ? 1 : 0;
  if (wt_packed) { a.dh0_acc = dh0_acc; a.ldacc = ldacc; a.alpha = alpha; a.first = first ? 1 : 0; }
  else { a.add = dh0_acc; a.ldadd = ldacc; a.add_scale = 1.f; }
  return launch(a, what, stream);
}
