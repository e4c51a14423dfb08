// What the three teachers over P = D_in^-1/2 A D_out^-1/2 (appnp.hip, gpr.hip, gcnii.hip) share beyond row_gather_dev.h: the host-side
// choice of a kernel instantiation, the first checks of their C entries, the column-tile shift and the row sum of the two scan kernels.
// Included inside each translation unit; everything is static to it.  The masks, the three epilogues and the argument structs differ.
#pragma once
#include "row_gather_dev.h"

namespace {

// f(bool_constant<A>, bool_constant<B>, integral_constant<int, LPR>) for two run-time flags and lpr (with_lpr<MIN_LPR>)
template <int MIN_LPR, class F>
inline void with_prop_variant(bool a, bool b, int lpr, F&& f) {
  auto pick_lpr = [&](auto A, auto B) { with_lpr<MIN_LPR>(lpr, [&](auto L) { f(A, B, L); }); };
  auto pick_b = [&](auto A) { if (b) pick_lpr(A, std::true_type{}); else pick_lpr(A, std::false_type{}); };
  if (a) pick_b(std::true_type{}); else pick_b(std::false_type{});
}

// The first checks of an entry (`more`: a size of its own).  The status of the nnz bound is the caller's (APPNP's entries say
// GLNN_ERR_INVALID_ARG, the others GLNN_ERR_UNSUPPORTED), and so is `ids`, what it calls 32-bit.  kRowsText: the text for buffers that
// fail rows_ok (glnn_common.h).
inline int prop_sizes_ok(const char* what, int64_t n, int d, int64_t nnz, bool more = true) {
  return n >= 0 && d >= 1 && nnz >= 0 && more ? GLNN_OK : glnn::fail(GLNN_ERR_INVALID_ARG, "%s: bad size", what);
}
inline int prop_nnz_ok(const char* what, int64_t nnz, int status, const char* ids) {
  return nnz < ((int64_t)1 << 31) ? GLNN_OK : glnn::fail(status, "%s: nnz >= 2^31 (%s are 32-bit)", what, ids);
}
constexpr char kRowsText[] = "%s: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(d)";

// Rows wider than 256 floats: blockIdx.y is the 256-column tile of this workgroup.  Moves every row pointer to it -- the first ALWAYS of
// them are always there, a later one may be NULL and stays so -- and makes d the tile's width (tiles == 1: nothing changes).  The order
// (those buffers, d, the others) and the type of `tiles` (unsigned in appnp.hip, int in gpr.hip) are what the kernels had written out,
// and they compile to what they were; any other order moves their prologues.  gpr_scale_kernel keeps its shift written out: behind this
// function, one with a wrapper type for the optional buffers, or one returning d, it comes out with 30 SGPRs for 34.
template <int ALWAYS, class Tiles, class... T>
__device__ __forceinline__ void to_col_tile(Tiles tiles, int& d, T*&... rows) {
  if (tiles > 1) {
    const int off = 256 * (int)blockIdx.y;
    int i = 0;
    ((i++ < ALWAYS ? (void)(rows += off) : (void)0), ...);
    d = d - off < 256 ? d - off : 256;
    i = 0;
    ((i++ >= ALWAYS && rows ? (void)(rows += off) : (void)0), ...);
  }
}

// scan_rows' row(v, wave_id, n_waves) up to the epilogue: the row's sum, in the lanes < LPR of wave 0 (of the one wave).  With it
// appnp_prop_kernel compiles to what it was and 20 of the 28 gpr_prop_kernel (every LPR but 16 and 64) to the same instructions in another
// order, every resource figure equal; a wrapper around scan_rows and the epilogue too moves 26 appnp_prop_kernel as well.
template <int LPR, class P>
__device__ __forceinline__ float4 row_sum(const int64_t* indptr, const int32_t* indices, int64_t v, int wave_id, int n_waves, int lane,
                                          const P& ld) {
  float4 sum = wave_row_sum<LPR>(indices, indptr[v], indptr[v + 1], wave_id, n_waves, lane, ld);
  if (n_waves > 1) sum = sum_waves_in_order<LPR>(sum, wave_id, lane);
  return sum;
}

}  // namespace
