// bf16 serving GEMM of the MLP student (gfx950 only):
//   out[m, n] = epi( A[m, k] . W[n, k]^T ),  epi(v) = relu?( v * ep_scale[n] + ep_shift[n] ),  then optionally a row-wise log_softmax
//   glnn_gemm_bf16          one product
//   glnn_mlp_forward_bf16   the whole eval-mode chain of a student as ONE C call (launches only: no allocation, no synchronisation)
//
// Storage rule: A is bf16 [m, lda] (rows padded to 8 elements, the layout of ops.bf16_empty) or fp32 [m, lda] rounded to bf16 on its way
// into LDS (round to nearest even, NaN -> 0x7FC0: the bits of glnn_cast_f32_bf16); W is bf16 [n, ldw] with ldw a multiple of 64 and zeros
// behind column k; every product runs on v_mfma_f32_16x16x32_bf16 (or 32x32x16: glnn::Options::gemm_bf16_mfma16 = 0) with fp32 accumulation;
// the epilogue is fp32; the output is bf16 (padding columns written as 0) or fp32.
//
// Structure (one kernel template): 128 x BN output tile (BN = 128, or 64 for narrow outputs), BK = 64, four waves.  Both operands are
// staged into ONE __shared__ array holding two buffers by the staging of bf16_mfma_dev.h (16-byte global_load_lds copies, the XOR swizzle
// on the SOURCE address; the fp32 A operand through registers: it has to be converted); rounding, fragment read, epilogue element and
// log-softmax tail come from that header too, shared with the one-launch form (mlp_fused_bf16.hip).  The copy of k-tile t+1 is issued
// before the MFMAs of tile t, one barrier per k-step.  Workgroup ids are remapped so that the tiles an XCD runs concurrently share rows
// of A.  The bf16 output goes through an LDS transpose of this file's own (padded rows, 16-byte stores).
//
// Fixed order: a row's accumulator sees k ascending in steps of the MFMA depth, whatever else is in the call -- no split-K, no atomics.  So
// results are bit-equal run to run, f(x)[a:b] == f(x[a:b]), and the fp32-A and bf16-A forms of one call give the same bits.
// A's columns behind k (row padding, or whatever follows a narrower row) are zeroed in registers in the last k-tile, never trusted.
#include "bf16_mfma_dev.h"

namespace {

constexpr int kThreads = kStageThreads;
constexpr int BM = 128;

struct GemmArgs {
  const void* a; int64_t lda; int64_t m; int k;
  const bf16_t* w; int64_t ldw; int n;
  const float* ep_scale; const float* ep_shift; int relu;
  void* out; int64_t ldo;
  int tiles_n;
};

template <int MF> struct Acc;
template <> struct Acc<32> { typedef floatx16 type; };
template <> struct Acc<16> { typedef floatx4 type; };

// BN: columns of the tile (128: waves 2 x 2 of 64 x 64; 64: waves 4 x 1 of 32 x 64).  MF: 32 = v_mfma_f32_32x32x16_bf16, 16 = 16x16x32.
// LSM (BN = 64, fp32 output, n <= 64): out = log_softmax of the row (max, expf sum, subtract); the logits never reach memory.
template <int BN, bool A_F32, bool OUT_BF16, bool LSM, int MF>
__global__ __launch_bounds__(kThreads) void gemm_bf16_kernel(const GemmArgs g) {
  constexpr int WM = BN == 128 ? 64 : 32, WN = 64;
  constexpr int MR = WM / MF, NR = WN / MF;
  constexpr int KS = MF == 32 ? 16 : 32;           // k per MFMA
  constexpr int NACC = MF == 32 ? 16 : 4;
  constexpr int A_BYTES = BM * kRowBytes, W_BYTES = BN * kRowBytes, BUF_BYTES = A_BYTES + W_BYTES;
  typedef typename Acc<MF>::type acc_t;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // XCD-aware remap (bijective for any grid size): consecutive ids of one XCD walk the column tiles of one row panel
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  const int tile_m = wgid / g.tiles_n, tile_n = wgid - tile_m * g.tiles_n;
  const int64_t row0 = (int64_t)tile_m * BM;
  const int col0 = tile_n * BN;
  const int wm0 = BN == 128 ? (wave >> 1) * WM : wave * WM;
  const int wn0 = BN == 128 ? (wave & 1) * WN : 0;
  const int lane_r = lane % MF, lane_q = lane / MF;

  const int nk = (g.k + BK - 1) / BK;
  const bf16_t* a16 = static_cast<const bf16_t*>(g.a);
  const float* a32 = static_cast<const float*>(g.a);
  const bool vec_ok = A_F32 && (g.lda % 4 == 0) && glnn::aligned16(g.a);

  acc_t acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int e = 0; e < NACC; ++e) acc[i][j][e] = 0.f;

  // bf16 operands: row pointers and chunk columns kept (computed once); the fp32 A keeps its registers for the rows in flight instead
  constexpr int PA = BM * 8 / kThreads, PW = BN * 8 / kThreads;
  float4 areg[2 * PA];
  const ClampedRows<float, int64_t> rows32{a32, g.lda, g.m, row0};
  const LiveChunks<ClampedRows<float, int64_t>> sa32{rows32, tid};
  KeptChunks<PA, bf16_t> sa;
  KeptChunks<PW, bf16_t> sw;
  sw.init(ClampedRows<bf16_t, int64_t>{g.w, g.ldw, g.n, col0}, tid);
  if constexpr (A_F32) {
    stage_load_f32<PA>(sa32, g.k, vec_ok, 0, areg);
    stage_write_f32<PA>(areg, smem, tid);
  } else {
    sa.init(ClampedRows<bf16_t, int64_t>{a16, g.lda, g.m, row0}, tid);
    stage_issue<PA>(sa, (int)g.lda, 0, smem, tid);
  }
  stage_issue<PW>(sw, (int)g.ldw, 0, smem + A_BYTES, tid);

  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's LDS-DMA copies of tile kt have landed
    __syncthreads();                                        // ... and everybody's; all reads of the other buffer are done
    unsigned char* cur = smem + (kt & 1) * BUF_BYTES;
    unsigned char* nxt = smem + ((kt + 1) & 1) * BUF_BYTES;
    const bool more = kt + 1 < nk;
    if (more) {
      if constexpr (A_F32) stage_load_f32<PA>(sa32, g.k, vec_ok, kt + 1, areg);
      else stage_issue<PA>(sa, (int)g.lda, kt + 1, nxt, tid);
      stage_issue<PW>(sw, (int)g.ldw, kt + 1, nxt + A_BYTES, tid);
    }
    const int krem = (!A_F32 && !more) ? g.k - kt * BK : BK;      // valid k of this tile (BK: no masking)
#pragma unroll
    for (int ks = 0; ks < BK / KS; ++ks) {
      const int lc = ks * (KS / 8) + lane_q;
      bf16x8 af[MR], bfr[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        uint4 u = frag_read(cur, wm0 + i * MF + lane_r, lc);
        if (krem < BK) mask_k_tail(u, krem - lc * 8);
        af[i] = __builtin_bit_cast(bf16x8, u);
      }
#pragma unroll
      for (int j = 0; j < NR; ++j) bfr[j] = __builtin_bit_cast(bf16x8, frag_read(cur + A_BYTES, wn0 + j * MF + lane_r, lc));
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          if constexpr (MF == 32) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    if constexpr (A_F32) {
      if (more) stage_write_f32<PA>(areg, nxt, tid);
    }
  }

  // ---- epilogue (fp32): v * scale + shift, ReLU ----
  auto row_of = [&](int i, int e) { return wm0 + i * MF + (MF == 32 ? (e & 3) + 8 * (e >> 2) + 4 * lane_q : lane_q * 4 + e); };
  float sc[NR], sh[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) ep_consts(g.ep_scale, g.ep_shift, col0 + wn0 + j * MF + lane_r, g.n, sc[j], sh[j]);
  auto ep = [&](float v, int j) { return epi(v, sc[j], sh[j], g.relu); };

  if constexpr (OUT_BF16) {
    constexpr int LDT = (BN + 8) * 2;          // bytes per row of the LDS tile (padded: the two lane groups of a store hit different banks)
    __syncthreads();                           // the staging buffers are free
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int cl = wn0 + j * MF + lane_r;
        const bool live = col0 + cl < g.n;
#pragma unroll
        for (int e = 0; e < NACC; ++e) {
          const float v = ep(acc[i][j][e], j);
          *reinterpret_cast<bf16_t*>(smem + row_of(i, e) * LDT + cl * 2) = live ? (bf16_t)f32_to_bf16_bits(v) : (bf16_t)0;
        }
      }
    __syncthreads();
    bf16_t* out = static_cast<bf16_t*>(g.out);
    const int npad = (g.n + 7) & ~7;
#pragma unroll
    for (int p = 0; p < BM * (BN / 8) / kThreads; ++p) {
      const int idx = p * kThreads + tid;
      const int row = idx / (BN / 8), c8 = idx % (BN / 8);
      const int gc = col0 + c8 * 8;
      if (row0 + row < g.m && gc < npad)
        *reinterpret_cast<uint4*>(out + (row0 + row) * g.ldo + gc) = *reinterpret_cast<const uint4*>(smem + row * LDT + c8 * 16);
    }
  } else if constexpr (LSM) {
    static_assert(BN + 1 == kLsmLd, "the log-softmax tile is 64 logits + the row's log-sum-exp");
    float* t = reinterpret_cast<float*>(smem);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < NACC; ++e) t[row_of(i, e) * kLsmLd + wn0 + j * MF + lane_r] = ep(acc[i][j][e], j);
    __syncthreads();
    log_softmax_rows<BM>(t, g.n, row0, g.m, static_cast<float*>(g.out), g.ldo);
  } else {
    float* out = static_cast<float*>(g.out);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int gc = col0 + wn0 + j * MF + lane_r;
#pragma unroll
        for (int e = 0; e < NACC; ++e) {
          const int64_t gr = row0 + row_of(i, e);
          if (gr < g.m && gc < g.n) out[gr * g.ldo + gc] = ep(acc[i][j][e], j);
        }
      }
  }
}

template <int BN, bool A_F32, bool OUT_BF16, bool LSM>
void launch_mf(const GemmArgs& g, unsigned grid, hipStream_t s, bool mfma16) {
  if (mfma16) hipLaunchKernelGGL((gemm_bf16_kernel<BN, A_F32, OUT_BF16, LSM, 16>), dim3(grid), dim3(kThreads), 0, s, g);
  else hipLaunchKernelGGL((gemm_bf16_kernel<BN, A_F32, OUT_BF16, LSM, 32>), dim3(grid), dim3(kThreads), 0, s, g);
}

template <int BN>
void launch_bn(const GemmArgs& g, unsigned grid, hipStream_t s, bool a_f32, bool out_bf16, bool lsm, bool mfma16) {
  if (lsm) {
    if constexpr (BN == 64) {
      if (a_f32) launch_mf<64, true, false, true>(g, grid, s, mfma16);
      else launch_mf<64, false, false, true>(g, grid, s, mfma16);
    }
    return;
  }
  if (a_f32) {
    if (out_bf16) launch_mf<BN, true, true, false>(g, grid, s, mfma16);
    else launch_mf<BN, true, false, false>(g, grid, s, mfma16);
  } else {
    if (out_bf16) launch_mf<BN, false, true, false>(g, grid, s, mfma16);
    else launch_mf<BN, false, false, false>(g, grid, s, mfma16);
  }
}

// Argument checks + launch of one product; `name` is the public entry reported in errors.
int gemm_bf16(const char* name, const void* a, int64_t lda, int a_dtype, int64_t m, int k, const uint16_t* w, int64_t ldw, int n,
              const float* ep_scale, const float* ep_shift, int relu, void* out, int64_t ldo, int out_dtype, int log_softmax, void* stream) {
  GLNN_REQUIRE(a_dtype == GLNN_DTYPE_F32 || a_dtype == GLNN_DTYPE_BF16, "%s: unknown a_dtype %d", name, a_dtype);
  GLNN_REQUIRE(out_dtype == GLNN_DTYPE_F32 || out_dtype == GLNN_DTYPE_BF16, "%s: unknown out_dtype %d", name, out_dtype);
  GLNN_REQUIRE(m >= 0 && k >= 1 && n >= 1 && lda < (1ll << 31) && ldw < (1ll << 31), "%s: bad m / k / n", name);
  GLNN_REQUIRE(!log_softmax || (n <= 64 && out_dtype == GLNN_DTYPE_F32), "%s: log_softmax needs n <= 64 and an fp32 output", name);
  if (a_dtype == GLNN_DTYPE_BF16)
    GLNN_REQUIRE(lda % 8 == 0 && lda >= k, "%s: lda=%lld must be a multiple of 8 and >= k for a bf16 A", name, (long long)lda);
  else
    GLNN_REQUIRE(lda >= k, "%s: lda=%lld must be >= k", name, (long long)lda);
  GLNN_REQUIRE(ldw % 64 == 0 && ldw >= k, "%s: ldw=%lld must be a multiple of 64 and >= k (zero padding behind k)", name, (long long)ldw);
  if (out_dtype == GLNN_DTYPE_BF16)
    GLNN_REQUIRE(ldo % 8 == 0 && ldo >= n, "%s: ldo=%lld must be a multiple of 8 and >= n for a bf16 output", name, (long long)ldo);
  else
    GLNN_REQUIRE(ldo >= n, "%s: ldo=%lld must be >= n", name, (long long)ldo);
  if (m == 0) return GLNN_OK;
  GLNN_REQUIRE(a && w && out, "%s: null pointer", name);
  GLNN_REQUIRE(glnn::aligned16(w) && (a_dtype != GLNN_DTYPE_BF16 || glnn::aligned16(a)) && (out_dtype != GLNN_DTYPE_BF16 || glnn::aligned16(out)),
               "%s: bf16 matrices must be 16-byte aligned", name);
  const bool narrow = n <= 64;
  const int bn = narrow ? 64 : 128;
  const int64_t tiles_m = (m + BM - 1) / BM, tiles_n = (n + bn - 1) / bn;
  GLNN_REQUIRE(tiles_m * tiles_n < (1ll << 31), "%s: too many tiles", name);
  GemmArgs g{a, lda, m, k, w, ldw, n, ep_scale, ep_shift, relu ? 1 : 0, out, ldo, (int)tiles_n};
  const unsigned grid = (unsigned)(tiles_m * tiles_n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool mfma16 = glnn::opts().gemm_bf16_mfma16 != 0;
  if (narrow) launch_bn<64>(g, grid, s, a_dtype == GLNN_DTYPE_F32, out_dtype == GLNN_DTYPE_BF16, log_softmax != 0, mfma16);
  else launch_bn<128>(g, grid, s, a_dtype == GLNN_DTYPE_F32, out_dtype == GLNN_DTYPE_BF16, false, mfma16);
  return glnn::check_launch(name);
}

}  // namespace

extern "C" int glnn_gemm_bf16(const void* a, int64_t lda, int a_dtype, int64_t m, int k, const uint16_t* w, int64_t ldw, int n,
                              const float* ep_scale, const float* ep_shift, int relu, void* out, int64_t ldo, int out_dtype,
                              int log_softmax, void* stream) {
  return gemm_bf16("glnn_gemm_bf16", a, lda, a_dtype, m, k, w, ldw, n, ep_scale, ep_shift, relu, out, ldo, out_dtype, log_softmax, stream);
}

extern "C" int glnn_mlp_forward_bf16(const glnn_mlp_serve_desc* d, const void* x, int64_t ldx, int x_dtype, int64_t m, uint16_t* buf0,
                                     uint16_t* buf1, int64_t ld_buf, float* out, int64_t ldo, int log_softmax, void* stream) {
  const char* name = "glnn_mlp_forward_bf16";
  GLNN_TRY(check_serve_desc(name, d, log_softmax));
  GLNN_REQUIRE(x_dtype == GLNN_DTYPE_F32 || x_dtype == GLNN_DTYPE_BF16, "%s: unknown x_dtype %d", name, x_dtype);
  GLNN_REQUIRE(m >= 0, "%s: bad m", name);
  const int L = d->num_layers;
  for (int l = 0; l + 1 < L; ++l)
    GLNN_REQUIRE(ld_buf % 8 == 0 && ld_buf >= d->dims[l + 1], "%s: ld_buf=%lld must be a multiple of 8 and >= every hidden width", name,
                 (long long)ld_buf);
  if (m == 0) return GLNN_OK;
  GLNN_REQUIRE(x && out && (L == 1 || buf0) && (L <= 2 || buf1), "%s: null pointer", name);
  for (int l = 0; l < L; ++l) GLNN_REQUIRE(d->w[l], "%s: null weight of layer %d", name, l);
  const void* in = x;
  int64_t ld_in = ldx;
  int in_dtype = x_dtype;
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    void* o = last ? static_cast<void*>(out) : static_cast<void*>((l & 1) ? buf1 : buf0);
    const int rc = gemm_bf16(name, in, ld_in, in_dtype, m, d->dims[l], d->w[l], d->ldw[l], d->dims[l + 1], d->ep_scale[l], d->ep_shift[l],
                             last ? 0 : 1, o, last ? ldo : ld_buf, last ? GLNN_DTYPE_F32 : GLNN_DTYPE_BF16, last ? log_softmax : 0, stream);
    if (rc != GLNN_OK) return rc;
    in = o;
    ld_in = ld_buf;
    in_dtype = GLNN_DTYPE_BF16;
  }
  return GLNN_OK;
}
