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
// staged by 16-byte global_load_lds copies into ONE __shared__ array holding two buffers; the XOR swizzle (16-byte chunk ^ ((row >> 1) & 7))
// is applied to the SOURCE address, the LDS image stays lane-linear.  The copy of k-tile t+1 is issued before the MFMAs of tile t, one
// barrier per k-step.  The fp32 A operand is staged through registers instead (it has to be converted).  Workgroup ids are remapped so that
// the tiles an XCD runs concurrently share rows of A.
//
// Fixed order: a row's accumulator sees k ascending in steps of the MFMA depth, whatever else is in the call -- no split-K, no atomics.  So
// results are bit-equal run to run, f(x)[a:b] == f(x[a:b]), and the fp32-A and bf16-A forms of one call give the same bits.
// A's columns behind k (row padding, or whatever follows a narrower row) are zeroed in registers in the last k-tile, never trusted.
#include "glnn_common.h"

namespace {

typedef uint16_t bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int BM = 128, BK = 64;
constexpr int kRowBytes = BK * 2;              // one staged row: 128 B = 8 chunks of 16 B

__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  if (f != f) return 0x7FC0u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t pack2(float lo, float hi) { return f32_to_bf16_bits(lo) | (f32_to_bf16_bits(hi) << 16); }

struct GemmArgs {
  const void* a; int64_t lda; int64_t m; int k;
  const bf16_t* w; int64_t ldw; int n;
  const float* ep_scale; const float* ep_shift; int relu;
  void* out; int64_t ldo;
  int tiles_n;
};

// 16-byte LDS-DMA copies of ROWS rows x 64 bf16 of a row-major bf16 matrix (one k-tile) into a lane-linear LDS image.
// Rows behind the matrix are clamped to its last row (their results are never stored); chunks that start behind `ld` are redirected to
// the row's first chunk (they only meet k indices that are masked or that W zero-fills) -- no read leaves the matrix.
// The row pointers and swizzled chunk columns do not depend on the k-tile: computed once.
template <int ROWS>
struct StageBf16 {
  static constexpr int P = ROWS * 8 / kThreads;
  const bf16_t* rowp[P];
  int col8[P];
  int ld, wave_base;
  __device__ __forceinline__ void init(const bf16_t* __restrict__ src, int64_t ld_, int64_t nrows, int64_t row0, int tid) {
    ld = (int)ld_;
    wave_base = (tid & ~63) * 16;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int idx = p * kThreads + tid;
      const int row = idx >> 3, pc = idx & 7;
      int64_t grow = row0 + row;
      if (grow > nrows - 1) grow = nrows - 1;
      rowp[p] = src + grow * ld_;
      col8[p] = (pc ^ ((row >> 1) & 7)) * 8;
    }
  }
  __device__ __forceinline__ void issue(int kt, unsigned char* dst) const {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      int col = kt * BK + col8[p];
      if (col >= ld) col = 0;
      const bf16_t* g = rowp[p] + col;
      unsigned char* l = dst + p * kThreads * 16 + wave_base;      // wave-uniform: the hardware adds lane * 16
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
    }
  }
};

// The fp32 A operand of k-tile kt: 4 chunks of 8 floats per thread, zero-filled behind k, rows clamped.
__device__ __forceinline__ void load_a_f32(const float* __restrict__ a, int64_t lda, int64_t m, int k, bool vec_ok, int64_t row0, int kt,
                                           int tid, float4 (&r)[8]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * kThreads + tid;
    const int row = idx >> 3, pc = idx & 7;
    const int lc = pc ^ ((row >> 1) & 7);
    int64_t grow = row0 + row;
    if (grow > m - 1) grow = m - 1;
    const int col = kt * BK + lc * 8;
    const float* s = a + grow * lda + col;
    if (vec_ok && col + 8 <= k) {
      r[2 * p] = *reinterpret_cast<const float4*>(s);
      r[2 * p + 1] = *reinterpret_cast<const float4*>(s + 4);
    } else {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (col + j < k) ? s[j] : 0.f;
      r[2 * p] = make_float4(v[0], v[1], v[2], v[3]);
      r[2 * p + 1] = make_float4(v[4], v[5], v[6], v[7]);
    }
  }
}
__device__ __forceinline__ void write_a_f32(const float4 (&r)[8], unsigned char* dst, int tid) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * kThreads + tid;
    uint4 u;
    u.x = pack2(r[2 * p].x, r[2 * p].y);
    u.y = pack2(r[2 * p].z, r[2 * p].w);
    u.z = pack2(r[2 * p + 1].x, r[2 * p + 1].y);
    u.w = pack2(r[2 * p + 1].z, r[2 * p + 1].w);
    *reinterpret_cast<uint4*>(dst + idx * 16) = u;
  }
}

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

  float4 areg[8];
  StageBf16<BM> sa;
  StageBf16<BN> sw;
  sw.init(g.w, g.ldw, g.n, col0, tid);
  if constexpr (A_F32) {
    load_a_f32(a32, g.lda, g.m, g.k, vec_ok, row0, 0, tid, areg);
    write_a_f32(areg, smem, tid);
  } else {
    sa.init(a16, g.lda, g.m, row0, tid);
    sa.issue(0, smem);
  }
  sw.issue(0, smem + A_BYTES);

  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's LDS-DMA copies of tile kt have landed
    __syncthreads();                                        // ... and everybody's; all reads of the other buffer are done
    unsigned char* cur = smem + (kt & 1) * BUF_BYTES;
    unsigned char* nxt = smem + ((kt + 1) & 1) * BUF_BYTES;
    const bool more = kt + 1 < nk;
    if (more) {
      if constexpr (A_F32) load_a_f32(a32, g.lda, g.m, g.k, vec_ok, row0, kt + 1, tid, areg);
      else sa.issue(kt + 1, nxt);
      sw.issue(kt + 1, nxt + A_BYTES);
    }
    // the bf16 A image may hold anything behind column k (row padding, the next row): zero those elements of the fragment
    const int krem = (!A_F32 && !more) ? g.k - kt * BK : BK;      // valid k of this tile (BK: no masking)
#pragma unroll
    for (int ks = 0; ks < BK / KS; ++ks) {
      const int lc = ks * (KS / 8) + lane_q;
      bf16x8 af[MR], bfr[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const int row = wm0 + i * MF + lane_r;
        uint4 u = *reinterpret_cast<const uint4*>(cur + row * kRowBytes + ((lc ^ ((row >> 1) & 7)) << 4));
        if (krem < BK) {
          const int v = krem - lc * 8;      // valid elements of this chunk (<= 0: none, >= 8: all)
          u.x = v >= 2 ? u.x : (v == 1 ? (u.x & 0xFFFFu) : 0u);
          u.y = v >= 4 ? u.y : (v == 3 ? (u.y & 0xFFFFu) : 0u);
          u.z = v >= 6 ? u.z : (v == 5 ? (u.z & 0xFFFFu) : 0u);
          u.w = v >= 8 ? u.w : (v == 7 ? (u.w & 0xFFFFu) : 0u);
        }
        af[i] = __builtin_bit_cast(bf16x8, u);
      }
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int row = wn0 + j * MF + lane_r;
        const uint4 u = *reinterpret_cast<const uint4*>(cur + A_BYTES + row * kRowBytes + ((lc ^ ((row >> 1) & 7)) << 4));
        bfr[j] = __builtin_bit_cast(bf16x8, u);
      }
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          if constexpr (MF == 32) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    if constexpr (A_F32) {
      if (more) write_a_f32(areg, nxt, tid);
    }
  }

  // ---- epilogue (fp32): v * scale + shift, ReLU ----
  auto row_of = [&](int i, int e) { return wm0 + i * MF + (MF == 32 ? (e & 3) + 8 * (e >> 2) + 4 * lane_q : lane_q * 4 + e); };
  float sc[NR], sh[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int gc = col0 + wn0 + j * MF + lane_r;
    sc[j] = (g.ep_scale && gc < g.n) ? g.ep_scale[gc] : 1.f;
    sh[j] = (g.ep_shift && gc < g.n) ? g.ep_shift[gc] : 0.f;
  }
  auto epi = [&](float v, int j) {
    v = fmaf(v, sc[j], sh[j]);
    return g.relu ? fmaxf(v, 0.f) : v;
  };

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
          const float v = epi(acc[i][j][e], j);
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
    constexpr int LDT = BN + 1;                // floats per row; [row][BN] holds the row's log-sum-exp
    float* t = reinterpret_cast<float*>(smem);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < NACC; ++e) t[row_of(i, e) * LDT + wn0 + j * MF + lane_r] = epi(acc[i][j][e], j);
    __syncthreads();
    if (tid < BM) {
      const float* zr = t + tid * LDT;
      float mx = -INFINITY;
      for (int j = 0; j < g.n; ++j) mx = fmaxf(mx, zr[j]);
      float se = 0.f;
      for (int j = 0; j < g.n; ++j) se += expf(zr[j] - mx);
      t[tid * LDT + BN] = mx + logf(se);
    }
    __syncthreads();
    float* out = static_cast<float*>(g.out);
    const int rows = (int)((g.m - row0) < BM ? (g.m - row0) : BM);
    for (int idx = tid; idx < rows * g.n; idx += kThreads) {
      const int row = idx / g.n, c = idx - row * g.n;
      out[(row0 + row) * g.ldo + c] = t[row * LDT + c] - t[row * LDT + BN];
    }
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
          if (gr < g.m && gc < g.n) out[gr * g.ldo + gc] = epi(acc[i][j][e], j);
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
  GLNN_REQUIRE(d, "%s: null descriptor", name);
  GLNN_REQUIRE(d->num_layers >= 1 && d->num_layers <= GLNN_MLP_MAX_LAYERS, "%s: num_layers=%d outside 1..%d", name, d->num_layers,
               GLNN_MLP_MAX_LAYERS);
  GLNN_REQUIRE(x_dtype == GLNN_DTYPE_F32 || x_dtype == GLNN_DTYPE_BF16, "%s: unknown x_dtype %d", name, x_dtype);
  GLNN_REQUIRE(m >= 0, "%s: bad m", name);
  const int L = d->num_layers;
  for (int l = 0; l <= L; ++l) GLNN_REQUIRE(d->dims[l] >= 1, "%s: dims[%d]=%d", name, l, d->dims[l]);
  for (int l = 0; l + 1 < L; ++l)
    GLNN_REQUIRE(ld_buf % 8 == 0 && ld_buf >= d->dims[l + 1], "%s: ld_buf=%lld must be a multiple of 8 and >= every hidden width", name,
                 (long long)ld_buf);
  GLNN_REQUIRE(!log_softmax || d->dims[L] <= 64, "%s: log_softmax needs an output width <= 64", name);
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
