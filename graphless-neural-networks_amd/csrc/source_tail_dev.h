// The hidden tail evaluated in the gather: an aggregation whose source rows are stored as pre-activations z applies
//     h = dropout(relu(norm(z)))
// to every row it gathers (and to the self row) instead of reading an h that a pass of its own wrote.  ONE definition, used by the "gcn"
// aggregation (spmm.hip) and the "mean" step's operand gather (sage_mean_step.hip): both training steps promise the bits of the
// materialised-h form, so the arithmetic below is glnn_act_fwd_f32's / glnn_layernorm_fwd_f32's per element, roundings included.
// Included inside each translation unit; everything is static to the including file.  Needs nothing but glnn_common.h.
#pragma once
#include "glnn_common.h"

namespace {

// per-lane constants of the tail: the lane's four columns' scale / shift (BatchNorm a_scale / a_shift, or LayerNorm gamma / beta), the
// dropout of the ACTIVATION's (row, column), and for a LayerNorm the per-row statistics arrays
struct TailCols { float s[4], h[4]; uint32_t thr, seed; float dscale; int col; bool affine; const float* mean; const float* rstd; };

// The lane owns columns [col4, col4 + 4) of rows d wide; scale == NULL: no affine (norm "none"); columns >= d are padding; xf as
// tail_apply's XF (2: LayerNorm).  scale / shift / d come by reference and xf stays an int compared where it is used, so that each caller's
// argument loads sit where its own copy of this function had them: spmm.hip's kernels compile to the instructions they had before.
__device__ __forceinline__ TailCols load_tail_cols(const float* const& scale, const float* const& shift, const float* mean, const float* rstd,
                                                   uint32_t thr, uint32_t seed, float dscale, const int& d, int col4, int xf) {
  TailCols x;
  x.thr = thr; x.seed = seed; x.dscale = dscale; x.col = col4; x.affine = scale != nullptr;
  x.mean = mean; x.rstd = rstd;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bool ok = x.affine && col4 + t < d;
    x.s[t] = ok ? scale[col4 + t] : (xf == 2 ? 0.f : 1.f);      // (LayerNorm: padding columns come out as 0)
    x.h[t] = ok ? shift[col4 + t] : 0.f;
  }
  return x;
}

// XF == 0: v as it is;  XF == 1: drop(relu(z * s + h)) (BatchNorm affine / none);  XF == 2: drop(relu(((z - mean_r) * rstd_r) * s + h))
// (LayerNorm, the statistics of row `row`)
template <int XF>
__device__ __forceinline__ float4 tail_apply(const TailCols& x, float4 v, uint32_t row) {
  if (XF == 0) return v;
  float o[4] = {v.x, v.y, v.z, v.w};
  float mu = 0.f, rs = 1.f;
  if (XF == 2) { mu = x.mean[row]; rs = x.rstd[row]; }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float y;
    if (XF == 2) {
      y = (o[t] - mu) * rs;
      asm volatile("" : "+v"(y));      // xhat rounded as glnn_layernorm_fwd_f32 rounds it, then ONE fma with gamma / beta
      y = fmaf(y, x.s[t], x.h[t]);
    } else {
      y = x.affine ? fmaf(o[t], x.s[t], x.h[t]) : o[t];
    }
    y = fmaxf(y, 0.f);
    if (x.thr) y = glnn::drop_keep(x.seed, x.thr, row, (uint32_t)(x.col + t)) ? y * x.dscale : 0.f;
    asm volatile("" : "+v"(y));        // the ROUNDED tail value is what gets summed (act_fwd stored it): no fma of y * dscale into the row sum
    o[t] = y;
  }
  return make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace
