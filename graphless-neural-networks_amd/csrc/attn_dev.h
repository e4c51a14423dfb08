// What the two edge-softmax teachers (gat.hip, gatv2.hip) share beyond row_gather_dev.h: the score helpers, the attention dropout's keep
// rule and the host-side choice of a rows-kernel instantiation.  Included inside each translation unit; everything is static to it.
// The row loops themselves are NOT here: see "the two-role scan" in row_gather_dev.h.
#pragma once
#include "row_gather_dev.h"

namespace {

constexpr int kU = 4;                      // edges in flight per lane group
constexpr float kNegBig = -3.0e38f;

__device__ __forceinline__ float lrelu(float s, float slope) { return s > 0.f ? s : s * slope; }
// the attention dropout: head `head` of edge `eid` is kept (glnn_gat_attn_mask_u8 writes the same rule out)
__device__ __forceinline__ bool attn_keep(uint32_t seed, uint32_t thr, uint32_t eid, uint32_t head) {
  return (glnn::drop_hash(seed, eid, head) & 0xFFFFu) >= thr;
}

// f(integral_constant<int, KIND>, bool_constant<UNI>, integral_constant<int, LPR>) for the run-time pass (kind 0 forward, 1 backward over
// the in-CSR, 2 backward over the transposed CSR), uni (a lane's four columns share a head: out_feats % 4 == 0) and lpr (with_lpr<4>)
template <class F>
inline void with_attn_variant(int kind, bool uni, int lpr, F&& f) {
  auto pick_lpr = [&](auto K, auto U) { with_lpr<4>(lpr, [&](auto L) { f(K, U, L); }); };
  auto pick_uni = [&](auto K) { if (uni) pick_lpr(K, std::true_type{}); else pick_lpr(K, std::false_type{}); };
  if (kind == 0) pick_uni(std::integral_constant<int, 0>{});
  else if (kind == 1) pick_uni(std::integral_constant<int, 1>{});
  else pick_uni(std::integral_constant<int, 2>{});
}

}  // namespace
