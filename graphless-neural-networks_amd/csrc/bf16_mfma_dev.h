// Device-side pieces shared by the bf16 serving kernels (gemm_bf16.hip: the per-layer chain; mlp_fused_bf16.hip: the one-launch form, which
// is DEFINED as producing the chain's bits): the rounding, the staging of a 64-wide k-tile into LDS, the fragment read, the fp32 epilogue
// and the log-softmax tail each have their one definition here.  sage_bf16.hip and position_serve.hip take the rounding from here too.
// Included inside each translation unit; everything here is static to the including file.
#pragma once
#include <cmath>

#include "glnn_common.h"

namespace {

typedef uint16_t bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// ---- rounding: nearest even, NaN -> 0x7FC0 (torch's Tensor.to(torch.bfloat16); the bits of glnn_cast_f32_bf16) ----
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  if (f != f) return 0x7FC0u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t pack2(float lo, float hi) { return f32_to_bf16_bits(lo) | (f32_to_bf16_bits(hi) << 16); }

// ---- staging: ROWS rows x 64 k of a row-major matrix (one k-tile) into a lane-linear LDS image, by workgroups of 256 threads ----
// A staged row is 128 B = 8 chunks of 16 B; thread tid moves the chunks idx = p * 256 + tid, p < ROWS * 8 / 256: image row idx >> 3,
// image chunk idx & 7.  The XOR swizzle is applied to the SOURCE chunk (the image stays lane-linear, as the LDS-DMA copy needs it) and
// again where a fragment is read.
constexpr int kStageThreads = 256;
constexpr int BK = 64;                         // k per staged tile
constexpr int kRowBytes = BK * 2;

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

__device__ __forceinline__ void lds_dma16(const bf16_t* g, unsigned char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// Where an image row comes from (T = bf16_t or float): `base` and the row's element offset from it.  No source ever yields a row outside
// its matrix.
// Rows row0, row0 + 1, ... of `base`, those behind the matrix clamped to its last row (their results are never stored).  I = int64_t, or
// int where the caller's indices are (the weight panels of the one-launch form: less address arithmetic per issue).
template <class T, class I>
struct ClampedRows {
  const T* base; I ld, nrows, row0;
  __device__ __forceinline__ int64_t operator()(int row) const {
    I r = row0 + row;
    if (r > nrows - 1) r = nrows - 1;
    return (int64_t)r * ld;
  }
};
// Batch rows row0, row0 + 1, ... (clamped to m - 1) read through the index `ids` (NULL: the batch row itself); an id outside [0, n_x) is
// replaced by row 0 -- the caller zeroes the fragment of such a row.
template <class T>
struct IdRows {
  const T* base; int64_t ld; const int64_t* ids; int64_t n_x, m, row0;
  __device__ __forceinline__ int64_t operator()(int row) const {
    int64_t b = row0 + row;
    if (b > m - 1) b = m - 1;
    int64_t s = b;
    if (ids) {
      s = ids[b];
      if (s < 0 || s >= n_x) s = 0;
    }
    return s * ld;
  }
};

// The thread's P chunks as (pointer, element offset of the row from it, swizzled source column), in two forms with one interface:
//   KeptChunks  row pointers and columns computed once (they do not depend on the k-tile) and held in registers
//   LiveChunks  recomputed at every use: nothing per chunk stays live -- for a kernel at its register ceiling, and for operands whose
//               registers are better spent elsewhere
// A chunk's address is formed as (pointer + column) + offset, the column first: it is the same for all of a thread's chunks (a step of
// 32 rows does not reach (row >> 1) & 7), so in the live form one add per chunk remains.  A row source that returned a pointer cost
// mlp_fused_kernel 30-54 more 64-bit adds and about 1 % of its time (NOTES.md).
template <int P, class T>
struct KeptChunks {
  const T* rowp[P];
  int col8[P];
  template <class Rows>
  __device__ __forceinline__ void init(const Rows& rows, int tid) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int idx = p * kStageThreads + tid, row = idx >> 3;
      rowp[p] = rows.base + rows(row);
      col8[p] = swz(row, idx & 7) * 8;
    }
  }
  __device__ __forceinline__ int col(int p) const { return col8[p]; }
  __device__ __forceinline__ void row(int p, const T*& bp, int64_t& off) const { bp = rowp[p], off = 0; }
};
template <class Rows>
struct LiveChunks {
  const Rows& rows;
  int tid;
  __device__ __forceinline__ int col(int p) const {
    const int idx = p * kStageThreads + tid;
    return swz(idx >> 3, idx & 7) * 8;
  }
  template <class T>
  __device__ __forceinline__ void row(int p, const T*& bp, int64_t& off) const { bp = rows.base, off = rows((p * kStageThreads + tid) >> 3); }
};

// bf16 rows: 16-byte LDS-DMA copies of k-tile kt.  A chunk that starts behind `ld` is redirected to the row's first chunk (it only meets k
// indices that are masked or that a zero-padded W multiplies by 0) -- no read leaves the matrix.
template <int P, class Chunks>
__device__ __forceinline__ void stage_issue(const Chunks& c, int ld, int kt, unsigned char* dst, int tid) {
  const int wave_base = (tid & ~63) * 16;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    int col = kt * BK + c.col(p);
    if (col >= ld) col = 0;
    const bf16_t* bp;
    int64_t off;
    c.row(p, bp, off);
    lds_dma16(bp + col + off, dst + p * kStageThreads * 16 + wave_base);      // wave-uniform: the hardware adds lane * 16
  }
}
// fp32 rows go through registers (they have to be rounded): 8 floats per chunk, zero-filled behind k; vec_ok: rows take 16-byte loads
template <int P, class Chunks>
__device__ __forceinline__ void stage_load_f32(const Chunks& c, int k, bool vec_ok, int kt, float4 (&r)[2 * P]) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int col = kt * BK + c.col(p);
    const float* s;
    int64_t off;
    c.row(p, s, off);
    s += col + off;
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
template <int P>
__device__ __forceinline__ void stage_write_f32(const float4 (&r)[2 * P], unsigned char* dst, int tid) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    uint4 u;
    u.x = pack2(r[2 * p].x, r[2 * p].y);
    u.y = pack2(r[2 * p].z, r[2 * p].w);
    u.z = pack2(r[2 * p + 1].x, r[2 * p + 1].y);
    u.w = pack2(r[2 * p + 1].z, r[2 * p + 1].w);
    *reinterpret_cast<uint4*>(dst + (p * kStageThreads + tid) * 16) = u;
  }
}

// ---- fragments: the 8 bf16 of k-chunk lc of a staged row ----
__device__ __forceinline__ uint4 frag_read(const unsigned char* tile, int row, int lc) {
  return *reinterpret_cast<const uint4*>(tile + row * kRowBytes + (swz(row, lc) << 4));
}
// A bf16 row may hold anything behind column k (row padding, the next row): keep the first `valid` elements of the chunk (<= 0: none,
// >= 8: all), zero the rest.  Only the last k-tile needs it.
__device__ __forceinline__ void mask_k_tail(uint4& u, int valid) {
  u.x = valid >= 2 ? u.x : (valid == 1 ? (u.x & 0xFFFFu) : 0u);
  u.y = valid >= 4 ? u.y : (valid == 3 ? (u.y & 0xFFFFu) : 0u);
  u.z = valid >= 6 ? u.z : (valid == 5 ? (u.z & 0xFFFFu) : 0u);
  u.w = valid >= 8 ? u.w : (valid == 7 ? (u.w & 0xFFFFu) : 0u);
}

// ---- epilogue (fp32): relu?( v * scale[col] + shift[col] ), one fmaf; scale / shift default to 1 / 0 (NULL, or a column behind n) ----
__device__ __forceinline__ void ep_consts(const float* scale, const float* shift, int col, int n, float& sc, float& sh) {
  sc = (scale && col < n) ? scale[col] : 1.f;
  sh = (shift && col < n) ? shift[col] : 0.f;
}
__device__ __forceinline__ float epi(float v, float sc, float sh, bool relu) {
  v = fmaf(v, sc, sh);
  return relu ? fmaxf(v, 0.f) : v;
}

// Row-wise log_softmax of the first n (<= 64) columns of an fp32 LDS tile of ROWS rows x kLsmLd floats (complete and visible to the
// workgroup on entry), into rows [row0, min(row0 + ROWS, m)) of out.  The order is part of the contract: max ascending, expf sum ascending,
// mx + logf(se) kept in the row's 65th float, subtracted on the way out.
constexpr int kLsmLd = 65;
template <int ROWS>
__device__ __forceinline__ void log_softmax_rows(float* t, int n, int64_t row0, int64_t m, float* __restrict__ out, int64_t ldo) {
  const int tid = threadIdx.x;
  if (tid < ROWS) {
    const float* zr = t + tid * kLsmLd;
    float mx = -INFINITY;
    for (int j = 0; j < n; ++j) mx = fmaxf(mx, zr[j]);
    float se = 0.f;
    for (int j = 0; j < n; ++j) se += expf(zr[j] - mx);
    t[tid * kLsmLd + 64] = mx + logf(se);
  }
  __syncthreads();
  const int rows = (int)((m - row0) < ROWS ? (m - row0) : ROWS);
  for (int idx = tid; idx < rows * n; idx += kStageThreads) {
    const int row = idx / n, c = idx - row * n;
    out[(row0 + row) * ldo + c] = t[row * kLsmLd + c] - t[row * kLsmLd + 64];
  }
}

// ---- host: what every serving entry asks of its chain descriptor first ----
inline int check_serve_desc(const char* name, const glnn_mlp_serve_desc* d, int log_softmax) {
  GLNN_REQUIRE(d, "%s: null descriptor", name);
  GLNN_REQUIRE(d->num_layers >= 1 && d->num_layers <= GLNN_MLP_MAX_LAYERS, "%s: num_layers=%d outside 1..%d", name, d->num_layers,
               GLNN_MLP_MAX_LAYERS);
  for (int l = 0; l <= d->num_layers; ++l) GLNN_REQUIRE(d->dims[l] >= 1, "%s: dims[%d]=%d", name, l, d->dims[l]);
  GLNN_REQUIRE(!log_softmax || d->dims[d->num_layers] <= 64, "%s: log_softmax needs an output width <= 64", name);
  return GLNN_OK;
}

}  // namespace
