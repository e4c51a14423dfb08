// One-launch bf16 serving of the MLP student (gfx950 only): glnn_mlp_forward_bf16's chain with the hidden rows kept in LDS.
//   glnn_mlp_fused_bf16_tile_rows   rows per workgroup the launch would use for a chain, or 0 when it does not take it
//   glnn_mlp_forward_fused_bf16     the whole chain as ONE launch: no hidden buffers, no allocation, no synchronisation
//
// An MLP is row-local: one workgroup (256 threads, 2 x 2 waves) owns T consecutive batch rows and carries them through every layer.
//   layer 0      the A operand comes from global memory in k-tiles of 64 through the staging of bf16_mfma_dev.h (16-byte LDS-DMA copies
//                of bf16 rows; fp32 rows rounded through registers), optionally through a `rows` index
//   hidden rows  the fp32 epilogue (epi: relu(fmaf(acc, ep_scale, ep_shift))) rounded to bf16 into one of two LDS images of T x pitch elements that ping-pong;
//                the next layer reads its A fragments from the image
//   weights      the chain's packed operand (bf16 [n, ldw], ldw % 64 == 0, zeros behind k), streamed as 128-row x 64-k tiles through a
//                double-buffered LDS stage by global_load_lds; the tile of the next (k-tile, column panel) unit is issued before the MFMAs
//                of the current one, one barrier per unit.  Every workgroup reads all weights once (L2 / Infinity Cache resident).
//   products     v_mfma_f32_16x16x32_bf16 only.  A wave holds the accumulators of its (T / 2) x 64 block of EVERY 128-column panel of the
//                layer (T x 1024 / 256 = 128 fp32 per thread at most), so the k loop is outermost: an A fragment is read once per k-tile
//                and an accumulator sees k ascending in steps of 32 -- the chain's order, hence the chain's bits.
//   last layer   fp32 logits from registers to `out`, or (log_softmax, width <= 64) through an fp32 LDS tile and log_softmax_rows.
// Staging, fragment read, k-tail mask, epilogue element and log-softmax tail are the definitions of bf16_mfma_dev.h, shared with the chain;
// what is this file's own is the hidden-row image and the (k-tile, panel) loop.
//
// Image layout: row pitch = the widest hidden layer rounded up to 128 elements (a multiple of 256 B, one LDS bank row), the 16-byte chunk
// index XORed with (row & 15).  A ds_read_b128 is served in groups of 16 lanes that hold 16 distinct fragment rows and two adjacent chunk
// indices c (even) and c + 1: c ^ r over eight rows and (c ^ 1) ^ r over the other eight are 16 distinct slots of the bank row, so the
// fragment reads are conflict-free.  Padding each row by 16 bytes instead leaves one 2-way conflict per group (row 11 at chunk c + 1
// meets row 12 at chunk c), and a pitch of an odd multiple of 128 B breaks the XOR scheme -- hence the rounding to 128 elements.
//
// LDS budget: two images (2 x T x pitch x 2 B; at least 128 elements of pitch, because layer 0's A stage lives in the image layer 0 does
// not write) + the weight stage (2 x 16 KB; the log-softmax tile reuses it).  T = 64 for widths <= 512 (160 KB at 512), T = 32 up to 1024
// (160 KB at 1024); the entry refuses what the device's LDS does not hold.
#include <type_traits>

#include "bf16_mfma_dev.h"

namespace {

constexpr int kThreads = kStageThreads;
constexpr int NP = 128;                        // columns per panel (one weight tile: NP rows x BK)
constexpr int kWTileBytes = NP * kRowBytes;    // 16 KB
constexpr int kCap = 1024;                     // widest hidden / output layer taken

struct FusedArgs {
  glnn_mlp_serve_desc d;
  const void* x; int64_t ldx;
  const int64_t* rows; int64_t n_x;
  int64_t m;
  float* out; int64_t ldo;
  int lsm;
  int pitch;                                   // elements per image row (a multiple of 128)
};

template <int T>
struct Geo {
  static constexpr int MR = T / 32;            // 16-row fragments per wave (waves 2 x 2 of (T / 2) x 64)
  static constexpr int NR = 4;                 // 16-column fragments per wave and panel
  static constexpr int NPANEL = 256 / T;       // panels whose accumulators a thread holds: 128 fp32
  static constexpr int A_BYTES = T * kRowBytes;
  static constexpr int PA = T * 8 / kThreads;  // 16-byte chunks of layer 0's A stage per thread
};
// Layer 0's A operand, T rows x BK per k-tile: the rows of x behind this thread's chunks (batch rows through the `rows` index), kept
template <int T, bool A_F32>
using AChunks = KeptChunks<Geo<T>::PA, std::conditional_t<A_F32, float, bf16_t>>;

// The products of one layer into acc.  FIRST: A from global memory (x / rows) through the A stage; otherwise from the image `img`.
template <int T, bool A_F32, bool FIRST>
__device__ __forceinline__ void layer_products(const FusedArgs& g, int k, int n, const bf16_t* __restrict__ w, int ldw,
                                               const unsigned char* img, unsigned char* astage, unsigned char* wstage,
                                               const AChunks<T, A_F32>& sa, bool vec_ok, const bool (&valid)[Geo<T>::MR],
                                               floatx4 (&acc)[Geo<T>::NPANEL][Geo<T>::MR][Geo<T>::NR]) {
  constexpr int MR = Geo<T>::MR, NR = Geo<T>::NR, NPANEL = Geo<T>::NPANEL, A_BYTES = Geo<T>::A_BYTES, PA = Geo<T>::PA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave >> 1) * (T / 2), wn0 = (wave & 1) * 64;
  const int lane_r = lane & 15, lane_q = lane >> 4;
  const int nk = (k + BK - 1) / BK, np = (n + NP - 1) / NP;
  const int pitch_b = g.pitch * 2;

  float4 areg[2 * PA];
  if constexpr (FIRST) {
    if constexpr (A_F32) {
      stage_load_f32<PA>(sa, k, vec_ok, 0, areg);
      stage_write_f32<PA>(areg, astage, tid);
    } else {
      stage_issue<PA>(sa, (int)g.ldx, 0, astage, tid);
    }
  }
  // unit = (k-tile, panel), panels innermost; (ktn, pn) is the next unit whose weight tile has not been issued yet.  They are run-time
  // values on purpose: the weight rows are LiveChunks -- one address computation per issue, nothing per panel for the compiler to hoist
  // out of the loop and spill.  (A chunk behind ldw, which stage_issue would redirect, does not exist: ldw % 64 == 0 and ldw >= k.)
  int pn = 0, ktn = 0;
  auto issue_next = [&](unsigned char* dst) {
    if (ktn < nk) {
      const ClampedRows<bf16_t, int> wrows{w, ldw, n, pn * NP};
      stage_issue<NP * 8 / kThreads>(LiveChunks<ClampedRows<bf16_t, int>>{wrows, tid}, ldw, ktn, dst, tid);
      if (++pn == np) {
        pn = 0;
        ++ktn;
      }
    }
  };
  issue_next(wstage);

  int u = 0;                                   // the weight tile of unit u is in stage buffer u & 1
  for (int kt = 0; kt < nk; ++kt) {
    bf16x8 af[2][MR];
    const bool more = kt + 1 < nk;
#pragma unroll
    for (int p = 0; p < NPANEL; ++p) {
      if (p < np) {                            // workgroup-uniform
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's LDS-DMA copies of the unit have landed
        __syncthreads();                                        // ... and everybody's; all reads of the other buffers are done
        const unsigned char* cur = wstage + (u & 1) * kWTileBytes;
        unsigned char* nxt = wstage + ((u + 1) & 1) * kWTileBytes;
        issue_next(nxt);
        if (p == 0) {
          if constexpr (FIRST) {
            if (more) {
              if constexpr (A_F32) stage_load_f32<PA>(sa, k, vec_ok, kt + 1, areg);
              else stage_issue<PA>(sa, (int)g.ldx, kt + 1, astage + ((kt + 1) & 1) * A_BYTES, tid);
            }
          }
          const int krem = (FIRST && !A_F32 && !more) ? k - kt * BK : BK;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int lc = ks * 4 + lane_q;
#pragma unroll
            for (int i = 0; i < MR; ++i) {
              const int row = wm0 + i * 16 + lane_r;
              uint4 v;
              if constexpr (FIRST) {
                v = frag_read(astage + (kt & 1) * A_BYTES, row, lc);
                if (krem < BK) mask_k_tail(v, krem - lc * 8);
                if (!valid[i]) v = make_uint4(0u, 0u, 0u, 0u);      // a `rows` index outside x: an all-zero input row
              } else {
                v = *reinterpret_cast<const uint4*>(img + row * pitch_b + (((kt * 8 + lc) ^ (row & 15)) << 4));
              }
              af[ks][i] = __builtin_bit_cast(bf16x8, v);
            }
          }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int lc = ks * 4 + lane_q;
          bf16x8 bfr[NR];
#pragma unroll
          for (int j = 0; j < NR; ++j) bfr[j] = __builtin_bit_cast(bf16x8, frag_read(cur, wn0 + j * 16 + lane_r, lc));
#pragma unroll
          for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j) acc[p][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bfr[j], acc[p][i][j], 0, 0, 0);
        }
        if constexpr (FIRST && A_F32) {
          if (p == 0 && more) stage_write_f32<PA>(areg, astage + ((kt + 1) & 1) * A_BYTES, tid);
        }
        ++u;
      }
    }
  }
}

template <int T, bool A_F32>
__global__ __launch_bounds__(kThreads) void mlp_fused_kernel(const FusedArgs g) {
  constexpr int MR = Geo<T>::MR, NR = Geo<T>::NR, NPANEL = Geo<T>::NPANEL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int pitch_b = g.pitch * 2;
  auto image = [&](int i) { return smem + (i & 1) * T * pitch_b; };
  unsigned char* wstage = smem + 2 * T * pitch_b;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave >> 1) * (T / 2), wn0 = (wave & 1) * 64;
  const int lane_r = lane & 15, lane_q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int L = g.d.num_layers;
  const bool vec_ok = A_F32 && (g.ldx % 4 == 0) && glnn::aligned16(g.x);

  typedef std::conditional_t<A_F32, float, bf16_t> x_t;
  AChunks<T, A_F32> sa;
  sa.init(IdRows<x_t>{static_cast<const x_t*>(g.x), g.ldx, g.rows, g.n_x, g.m, row0}, tid);
  bool valid[MR];
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    valid[i] = true;
    if (g.rows) {
      int64_t b = row0 + wm0 + i * 16 + lane_r;
      if (b > g.m - 1) b = g.m - 1;
      const int64_t s = g.rows[b];
      valid[i] = s >= 0 && s < g.n_x;
    }
  }

  floatx4 acc[NPANEL][MR][NR];
  for (int l = 0; l < L; ++l) {
#pragma unroll
    for (int p = 0; p < NPANEL; ++p)
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[p][i][j][e] = 0.f;

    // layer l writes image[l & 1] and reads image[(l - 1) & 1]; layer 0's A stage sits in image[1], which layer 0 does not write
    const int k = g.d.dims[l], n = g.d.dims[l + 1];
    const bf16_t* w = g.d.w[l];
    const int ldw = (int)g.d.ldw[l];
    if (l == 0) layer_products<T, A_F32, true>(g, k, n, w, ldw, nullptr, image(1), wstage, sa, vec_ok, valid, acc);
    else layer_products<T, A_F32, false>(g, k, n, w, ldw, image(l - 1), nullptr, wstage, sa, vec_ok, valid, acc);

    // ---- epilogue (fp32): v * scale + shift, ReLU behind every layer but the last ----
    const int np = (n + NP - 1) / NP;
    const bool last = l == L - 1;
    const float* ep_scale = g.d.ep_scale[l];
    const float* ep_shift = g.d.ep_shift[l];
    if (last && g.lsm) __syncthreads();        // the log-softmax tile reuses the weight stage: every wave is done reading it
    unsigned char* dst = image(l);
#pragma unroll
    for (int p = 0; p < NPANEL; ++p) {
      if (p < np) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int col = p * NP + wn0 + j * 16 + lane_r;
          float sc, sh;
          ep_consts(ep_scale, ep_shift, col, n, sc, sh);
          if (!last) {
            // the bf16 image of the hidden row: columns [n, round64(n)) are zeros, nothing is read behind them
            if (col < ((n + 63) & ~63)) {
#pragma unroll
              for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const int row = wm0 + i * 16 + lane_q * 4 + e;
                  const float v = epi(acc[p][i][j][e], sc, sh, true);
                  *reinterpret_cast<bf16_t*>(dst + row * pitch_b + ((((col >> 3) ^ (row & 15)) << 4) | ((col & 7) << 1))) =
                      col < n ? (bf16_t)f32_to_bf16_bits(v) : (bf16_t)0;
                }
            }
          } else if (g.lsm) {
            if (col < 64) {
#pragma unroll
              for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  reinterpret_cast<float*>(wstage)[(wm0 + i * 16 + lane_q * 4 + e) * kLsmLd + col] = epi(acc[p][i][j][e], sc, sh, false);
            }
          } else if (col < n) {
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int64_t gr = row0 + wm0 + i * 16 + lane_q * 4 + e;
                if (gr < g.m) g.out[gr * g.ldo + col] = epi(acc[p][i][j][e], sc, sh, false);
              }
          }
        }
      }
    }
    __syncthreads();                           // the image is complete; the weight stage and the other image are free
  }

  if (g.lsm) log_softmax_rows<T>(reinterpret_cast<float*>(wstage), g.d.dims[L], row0, g.m, g.out, g.ldo);
}

struct Plan { int tile_rows; int pitch; size_t smem; };

// What the launch would use for the chain `d` (behind check_serve_desc): GLNN_OK and *pl, or the refusal (GLNN_ERR_UNSUPPORTED for a chain
// the fused form does not take), the reason in glnn_last_error.
int make_plan(const char* name, const glnn_mlp_serve_desc* d, Plan* pl) {
  const int L = d->num_layers;
  if (glnn::opts().gemm_bf16_mfma16 == 0)
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: GLNN_GEMM_BF16_MFMA16=0 is in force; the one-launch form exists on v_mfma_f32_16x16x32_bf16 only "
                      "(its results are defined as the bits of the default chain)", name);
  int widest = 0, hidden = 0;
  for (int l = 1; l <= L; ++l) {
    if (d->dims[l] > kCap)
      return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: dims[%d]=%d is above the one-launch form's width cap of %d (use glnn_mlp_forward_bf16)", name, l,
                        d->dims[l], kCap);
    if (d->dims[l] > widest) widest = d->dims[l];
    if (l < L && d->dims[l] > hidden) hidden = d->dims[l];
  }
  pl->tile_rows = widest <= 512 ? 64 : 32;
  pl->pitch = hidden <= 128 ? 128 : (hidden + 127) & ~127;
  pl->smem = (size_t)2 * pl->tile_rows * pl->pitch * 2 + 2 * kWTileBytes;
  int dev = 0, lds = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return glnn::fail(GLNN_ERR_NO_DEVICE, "%s: no HIP device to size the tile for", name);
  }
  if (pl->smem > (size_t)lds)
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: a tile of %d rows x %d columns needs %zu bytes of LDS, the device gives a workgroup %d", name,
                      pl->tile_rows, pl->pitch, pl->smem, lds);
  return GLNN_OK;
}

template <class K>
int configure_lds(K kernel, size_t smem, const char* name) {
  if (smem <= 64 * 1024) return GLNN_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
    (void)hipGetLastError();
    return glnn::fail(GLNN_ERR_HIP, "%s: hipFuncSetAttribute(max dynamic LDS=%zu) failed", name, smem);
  }
  return GLNN_OK;
}

template <int T, bool A_F32>
int launch(const FusedArgs& g, size_t smem, hipStream_t s, const char* name) {
  GLNN_TRY(configure_lds(mlp_fused_kernel<T, A_F32>, smem, name));
  const unsigned grid = (unsigned)((g.m + T - 1) / T);
  hipLaunchKernelGGL((mlp_fused_kernel<T, A_F32>), dim3(grid), dim3(kThreads), smem, s, g);
  return glnn::check_launch(name);
}

}  // namespace

extern "C" int glnn_mlp_fused_bf16_tile_rows(const glnn_mlp_serve_desc* desc) {
  const char* name = "glnn_mlp_fused_bf16_tile_rows";
  Plan pl;
  return check_serve_desc(name, desc, 0) == GLNN_OK && make_plan(name, desc, &pl) == GLNN_OK ? pl.tile_rows : 0;
}

extern "C" int glnn_mlp_forward_fused_bf16(const glnn_mlp_serve_desc* d, const void* x, int64_t ldx, int x_dtype, const int64_t* rows,
                                           int64_t n_x, int64_t m, float* out, int64_t ldo, int log_softmax, void* stream) {
  const char* name = "glnn_mlp_forward_fused_bf16";
  GLNN_TRY(check_serve_desc(name, d, log_softmax));
  GLNN_REQUIRE(x_dtype == GLNN_DTYPE_F32 || x_dtype == GLNN_DTYPE_BF16, "%s: unknown x_dtype %d", name, x_dtype);
  GLNN_REQUIRE(m >= 0 && ldx < (1ll << 31), "%s: bad m / ldx", name);
  const int L = d->num_layers;
  if (m == 0) return GLNN_OK;
  if (x_dtype == GLNN_DTYPE_BF16)
    GLNN_REQUIRE(ldx % 8 == 0 && ldx >= d->dims[0], "%s: ldx=%lld must be a multiple of 8 and >= dims[0] for bf16 rows", name, (long long)ldx);
  else
    GLNN_REQUIRE(ldx >= d->dims[0], "%s: ldx=%lld must be >= dims[0]", name, (long long)ldx);
  for (int l = 0; l < L; ++l)
    GLNN_REQUIRE(d->ldw[l] % 64 == 0 && d->ldw[l] >= d->dims[l] && d->ldw[l] < (1ll << 31),
                 "%s: ldw[%d]=%lld must be a multiple of 64 and >= dims[%d] (zero padding behind k)", name, l, (long long)d->ldw[l], l);
  GLNN_REQUIRE(ldo >= d->dims[L], "%s: ldo=%lld must be >= dims[%d]", name, (long long)ldo, L);
  GLNN_REQUIRE(x && out, "%s: null pointer", name);
  GLNN_REQUIRE(!rows || n_x >= 1, "%s: rows given, but x has n_x=%lld rows", name, (long long)n_x);
  for (int l = 0; l < L; ++l) GLNN_REQUIRE(d->w[l] && glnn::aligned16(d->w[l]), "%s: the weight of layer %d is null or not 16-byte aligned", name, l);
  GLNN_REQUIRE(x_dtype != GLNN_DTYPE_BF16 || glnn::aligned16(x), "%s: bf16 matrices must be 16-byte aligned", name);
  Plan pl;
  GLNN_TRY(make_plan(name, d, &pl));
  GLNN_REQUIRE((m + pl.tile_rows - 1) / pl.tile_rows < (1ll << 31), "%s: too many tiles", name);
  FusedArgs g{*d, x, ldx, rows, n_x, m, out, ldo, log_softmax ? 1 : 0, pl.pitch};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool f32 = x_dtype == GLNN_DTYPE_F32;
  if (pl.tile_rows == 64) return f32 ? launch<64, true>(g, pl.smem, s, name) : launch<64, false>(g, pl.smem, s, name);
  return f32 ? launch<32, true>(g, pl.smem, s, name) : launch<32, false>(g, pl.smem, s, name);
}
