// The CSR row gather shared by the graph-teacher kernels (appnp.hip, gpr.hip and gcnii.hip through prop_dev.h, gat.hip and gatv2.hip
// through attn_dev.h, sage_mean.hip, sage_mean_step.hip; deepwalk.hip borrows the lane layout):
// the ideas of spmm.hip for narrow rows, tuned there and kept in ONE place here.  Included inside each translation unit; everything is
// static to the including file.
//
// Mapping.  A row of up to 256 floats is LPR lanes moving float4 (16 bytes per lane, coalesced).  The G = 64 / LPR lane groups of a wave
// take different entries of the same row -- group g the entries g, g + G, ... of a 64-entry chunk, ascending, min(8, 64 / G) row loads in
// flight each -- and are folded with cross-lane adds, xor 32 down to LPR.  The column indices of a chunk are read once, one per lane, with
// the non-temporal hint, and handed round with cross-lane moves.  A wave of n_waves takes the chunks wave_id, wave_id + n_waves, ...  Every
// sum therefore has a fixed order: no float atomics, results are bit-identical run to run whichever rows share the launch.
//
// Two ways of giving rows to waves, both with one wave per row of <= kLongRow entries and all eight waves of a workgroup on a longer one:
//   the 32-row tile (gather_tile)   a workgroup owns kTileRows rows: its waves draw the short ones from an LDS ticket, then take the long
//                                   ones together, the eight partials folded through four LDS slots (fold_waves_tree);
//   the two-role scan (scan_rows)   the first n_long_blocks workgroups search the row lengths (find_long_rows) and take every long row of
//                                   the graph, the partials summed in wave order; the others take the short rows of their block.
// gat.hip and gatv2.hip write the two loops out around find_long_rows, with the short rows assigned statically, and
// do NOT share them as a function.  A scan_rows_static<ASCENDING>(indptr, n, sg, wave, row) here, tried with the build's flags, left every
// gatv2_rows_kernel figure alone but took gat_rows_kernel<2, ..> from 71 / 71 / 77 / 90 VGPRs (LPR 32 / 16 / 8 / 4, UNI) to 107 / 109 /
// 112 / 120 and its non-UNI forms from 84 - 102 to 113 - 126: a wave per SIMD less.  Taking sg and the callable by reference, by value, or
// an if / else in place of the early return gave the same figures to the register.  Do not retry it.
#pragma once
#include <type_traits>

#include "glnn_common.h"

namespace {

using glnn::rows_ok;

constexpr int kBlock = 512;                // 8 waves
constexpr int kWaves = kBlock / 64;
constexpr int kLongRow = 128;              // entries above which a whole workgroup takes the row (spmm.hip's threshold, measured there)
constexpr int kTileRows = 32;              // gather_tile: rows per workgroup
constexpr int kRowsPerWave = 8;            // scan_rows: most short rows per wave and workgroup
constexpr int kLongBlockRows = 512;        // scan_rows: one long-role workgroup per this many rows ...
constexpr int kLongBlockCap = 512;         // ... up to this many

// ---------------------------------------------------------------------------------------------------------------- float4 helpers
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// the index stream is read once: the non-temporal hint keeps it from evicting the re-used feature rows
__device__ __forceinline__ int ld_idx_stream(const int32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
typedef float f32x2 __attribute__((ext_vector_type(2)));
// the pairs (x, y) and (z, w) are added as such (v_pk_add_f32 on the loaded registers in place): left to itself the vectoriser sometimes
// pairs (y, x), and a gathered row then has to be copied behind a full wait for its load
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  const f32x2 lo = (f32x2){a.x, a.y} + (f32x2){b.x, b.y}, hi = (f32x2){a.z, a.w} + (f32x2){b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 fma4(float s, float4 v, float4 a) {
  return make_float4(fmaf(s, v.x, a.x), fmaf(s, v.y, a.y), fmaf(s, v.z, a.z), fmaf(s, v.w, a.w));
}
__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
  return make_float4(__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m));
}
// the lane groups' sums into the lanes < LPR
template <int LPR>
__device__ __forceinline__ float4 fold_groups(float4 acc) {
#pragma unroll
  for (int m = 32; m >= LPR; m >>= 1) acc = add4(acc, shfl_xor4(acc, m));
  return acc;
}
// columns [d, ..) of a lane's four are padding: exact zeros whatever the row held there
__device__ __forceinline__ float4 mask_cols(float4 y, int col4, int d) {
  if (col4 + 0 >= d) y.x = 0.f;
  if (col4 + 1 >= d) y.y = 0.f;
  if (col4 + 2 >= d) y.z = 0.f;
  if (col4 + 3 >= d) y.w = 0.f;
  return y;
}

// ---------------------------------------------------------------------------------------------------------------- the wave gather
// What a caller's policy P may replace (all resolved at compile time: the loop below never asks which caller it serves).
struct GatherPolicy {
  // true: a per-entry scalar weight(idx, in_range), loaded by the lane that holds the index, rides along with it to row() and add()
  static constexpr bool kWeighted = false;
  __device__ __forceinline__ float weight(int, bool) const { return 0.f; }
  // float4 row(int src, float w, bool ok) const: the lane's four columns of entry `src`; zeros, and no load, outside the row's columns and
  // for !ok (a position past the chunk's entries) -- every policy has one
  // how a row enters the running sum
  __device__ __forceinline__ float4 add(float4 acc, float4 v, int, float) const { return add4(acc, v); }
  // per-chunk hook: may rearrange the cnt indices the lanes hold; returns how many of them (in the low lanes) are gathered
  __device__ __forceinline__ int chunk(int64_t, int, int cnt, int&) const { return cnt; }
};

// Rows of x, optionally UNSCALED (XN: each gathered row is multiplied by x_norm[source], one fma per element)
template <bool XN>
struct NormRows : GatherPolicy {
  static constexpr bool kWeighted = XN;
  const float* x; int64_t ldx; const float* x_norm; int col4; bool col_ok;
  __device__ __forceinline__ float weight(int idx, bool in_range) const { return in_range ? x_norm[idx] : 0.f; }
  __device__ __forceinline__ float4 row(int src, float, bool ok) const { return (ok && col_ok) ? ld4(x + (int64_t)src * ldx + col4) : zero4(); }
  __device__ __forceinline__ float4 add(float4 acc, float4 v, int, float w) const { return XN ? fma4(w, v, acc) : add4(acc, v); }
};

// Sum over this wave's share of the entries [e0, e1) -- the 64-entry chunks e0 + 64 (wave_id + k n_waves) -- of p.row(indices[e], ..),
// entered by p.add.  The total is in the lanes < LPR.
template <int LPR, class P>
__device__ __forceinline__ float4 wave_row_sum(const int32_t* __restrict__ indices, int64_t e0, int64_t e1, int wave_id, int n_waves, int lane,
                                               const P& p) {
  constexpr int G = 64 / LPR;
  constexpr int U = 64 / G < 8 ? 64 / G : 8;      // entries in flight per group (G U <= 64: one chunk)
  const int g = lane / LPR;
  float4 acc = zero4();
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    int my_idx = lane < cnt ? ld_idx_stream(indices + base + lane) : 0;
    const int n = p.chunk(base, lane, cnt, my_idx);
    float my_w = 0.f;
    if (P::kWeighted) my_w = p.weight(my_idx, lane < n);
    for (int j = 0; j < n; j += G * U) {
      float4 v[U];
      float w[U];
      int src[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ei = j + u * G + g;               // (G == 1: uniform, the scalar path)
        src[u] = (G == 1) ? __builtin_amdgcn_readlane(my_idx, ei & 63) : __shfl(my_idx, ei & 63);
        w[u] = 0.f;
        if (P::kWeighted) w[u] = (G == 1) ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), ei & 63))
                                          : __shfl(my_w, ei & 63);
        v[u] = p.row(src[u], w[u], ei < n);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc = p.add(acc, v[u], src[u], w[u]);
    }
  }
  return fold_groups<LPR>(acc);
}

// ---------------------------------------------------------------------------------------------------------------- the 32-row tile
// The 8 wave partials of a row (lanes < LPR) through 4 LDS slots of 64 float4 in a fixed order: waves 4-7 park, waves 0-3 add theirs,
// wave 0 sums the four.  The total is in wave 0's lanes < LPR; a barrier must follow before the slots are used again.
template <int LPR>
__device__ __forceinline__ float4 fold_waves_tree(float4 acc, int wave, int lane, float4* s_part) {
  if (wave >= 4 && lane < LPR) s_part[(wave - 4) * 64 + lane] = acc;
  __syncthreads();
  if (wave < 4 && lane < LPR) s_part[wave * 64 + lane] = add4(acc, s_part[wave * 64 + lane]);
  __syncthreads();
  float4 t = zero4();
  if (wave == 0 && lane < LPR) t = add4(add4(s_part[lane], s_part[64 + lane]), add4(s_part[128 + lane], s_part[192 + lane]));
  return t;
}

// the next row of the tile for this wave (uniform); *s_next must be 0 and visible before the first draw
__device__ __forceinline__ int tile_ticket(int* s_next, int lane) {
  int lr = 0;
  if (lane == 0) lr = atomicAdd(s_next, 1);
  return __builtin_amdgcn_readfirstlane(lr);
}

// One tile of a CSR, rows [row0, row0 + kTileRows).  finish(lr, v, n_entries, sum, valid) is called by ONE whole wave per tile row lr;
// `sum` is in the lanes < LPR; valid == false: the row is past n_rows (nothing was read).  Ends behind a barrier.
template <int LPR, class P, class Fin>
__device__ __forceinline__ void gather_tile(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
                                            int64_t row0, int lane, int wave, int* s_next, float4* s_part, const P& p, Fin&& finish) {
#pragma unroll 1
  while (true) {
    const int lr = tile_ticket(s_next, lane);
    if (lr >= kTileRows) break;
    const int64_t v = row0 + lr;
    if (v >= n_rows) { finish(lr, v, (int64_t)0, zero4(), false); continue; }
    const int64_t e0 = indptr[v], e1 = indptr[v + 1];
    if (e1 - e0 > kLongRow) continue;
    finish(lr, v, e1 - e0, wave_row_sum<LPR>(indices, e0, e1, 0, 1, lane, p), true);
  }
  __syncthreads();
  // long rows of this tile: all 8 waves on one row at a time (uniform loop: every wave sees the same row lengths)
#pragma unroll 1
  for (int lr = 0; lr < kTileRows; ++lr) {
    const int64_t v = row0 + lr;
    if (v >= n_rows) break;
    const int64_t e0 = indptr[v], e1 = indptr[v + 1];
    if (e1 - e0 <= kLongRow) continue;
    const float4 t = fold_waves_tree<LPR>(wave_row_sum<LPR>(indices, e0, e1, wave, kWaves, lane, p), wave, lane, s_part);
    if (wave == 0) finish(lr, v, e1 - e0, t, true);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- the two-role scan
// The 8 wave partials of a row (lanes < LPR) summed in wave order; the total is in wave 0's lanes < LPR.  A barrier must follow before the
// next call (scan_rows has one behind every long row).
template <int LPR>
__device__ __forceinline__ float4 sum_waves_in_order(float4 acc, int wave, int lane) {
  __shared__ float4 s_part[kWaves][64];
  if (lane < LPR) s_part[wave][lane] = acc;
  __syncthreads();
  float4 t = zero4();
  if (wave == 0 && lane < LPR) {
    t = s_part[0][lane];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t = add4(t, s_part[w][lane]);
  }
  return t;
}

// what scan_grid (below) makes of the row count: grid.x = grid_x = n_long_blocks + ceil(n / rows_per_block)
struct ScanGrid { int n_long_blocks, rows_per_block; unsigned grid_x; };

// One trip of the long role's search, by the whole workgroup: of the rows chunk, chunk + n_chunks, ... (n_chunks = ceil(n / kBlock), one
// row per thread: a degree-sorted order is dealt round-robin) those of more than kLongRow entries, in *rows; returns how many.  The order
// they come in does not matter: each row is one workgroup's.  A barrier must follow the last use of *rows before the next trip.
__device__ __forceinline__ int find_long_rows(const int64_t* indptr, int64_t n, int64_t n_chunks, int64_t chunk, const int64_t** rows) {
  __shared__ int64_t s_rows[kBlock];
  __shared__ int s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const int64_t r = (int64_t)threadIdx.x * n_chunks + chunk;
  if (r < n && (indptr[r + 1] - indptr[r]) > kLongRow) s_rows[atomicAdd(&s_count, 1)] = r;
  __syncthreads();
  *rows = s_rows;
  return s_count;
}

// Every row of the launch, once: row(v, wave_id, n_waves) is called by all kWaves waves of a workgroup for a row of more than kLongRow
// entries (a barrier follows) and as row(v, 0, 1) by one wave for any other.  Workgroups below n_long_blocks are the long role: workgroup
// c takes the trips c, c + n_long_blocks, ... of find_long_rows.  The others own rows_per_block consecutive rows each, which their waves
// draw from an LDS ticket, and skip the long ones.
template <class Row>
__device__ __forceinline__ void scan_rows(const int64_t* indptr, int64_t n, const ScanGrid& sg, int lane, int wave, Row&& row) {
  if ((int)blockIdx.x < sg.n_long_blocks) {
    const int64_t n_chunks = (n + kBlock - 1) / kBlock;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += sg.n_long_blocks) {
      const int64_t* rows;
      const int n_found = find_long_rows(indptr, n, n_chunks, chunk, &rows);
      for (int i = 0; i < n_found; ++i) {
        row(rows[i], wave, kWaves);
        __syncthreads();
      }
    }
    return;
  }
  __shared__ int s_ticket;
  if (threadIdx.x == 0) s_ticket = 0;
  __syncthreads();
  const int64_t row_base = ((int64_t)blockIdx.x - sg.n_long_blocks) * sg.rows_per_block;
#pragma unroll 1
  while (true) {
    const int lr = tile_ticket(&s_ticket, lane);
    if (lr >= sg.rows_per_block) break;
    const int64_t v = row_base + lr;
    if (v >= n) break;
    if (indptr[v + 1] - indptr[v] > kLongRow) continue;
    row(v, 0, 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the grid of a scan_rows kernel over n >= 1 rows
inline int scan_grid(int64_t n, const char* what, ScanGrid* g) {
  int64_t n_long = (n + kLongBlockRows - 1) / kLongBlockRows;
  if (n_long > kLongBlockCap) n_long = kLongBlockCap;
  int64_t rpw = n / (2048 * kWaves);                  // more rows per wave once every CU has its workgroups
  if (rpw < 1) rpw = 1;
  if (rpw > kRowsPerWave) rpw = kRowsPerWave;
  const int64_t row_blocks = (n + rpw * kWaves - 1) / (rpw * kWaves);
  GLNN_REQUIRE(n_long + row_blocks < ((int64_t)1 << 31), "%s: n too large for one launch", what);
  *g = {(int)n_long, (int)(rpw * kWaves), (unsigned)(n_long + row_blocks)};
  return GLNN_OK;
}

// LPR for rows of `float4s` 16-byte pieces: the power of two at or above it, between min_lpr and 64 (wider rows are cut into column tiles)
inline int lpr_for(int float4s, int min_lpr) {
  int lpr = min_lpr;
  while (lpr < float4s && lpr < 64) lpr <<= 1;
  return lpr;
}

// f(std::integral_constant<int, LPR>) for the run-time lpr (a power of two; below MIN_LPR it is MIN_LPR, above 64 it is 64)
template <int MIN_LPR, class F>
inline auto with_lpr(int lpr, F&& f) {
  if constexpr (MIN_LPR < 64) {
    if (lpr <= MIN_LPR) return f(std::integral_constant<int, MIN_LPR>{});
    return with_lpr<MIN_LPR * 2>(lpr, f);
  } else {
    return f(std::integral_constant<int, 64>{});
  }
}

}  // namespace
