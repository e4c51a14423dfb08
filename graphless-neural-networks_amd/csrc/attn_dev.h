// What the edge-softmax teachers (gat.hip, gatv2.hip, gt.hip) share beyond row_gather_dev.h: the score helpers, the attention dropout's keep
// rule and the host-side choice of a rows-kernel instantiation; and, for the two whose score is a sum over a head's columns (gatv2.hip,
// gt.hip), the lane description, the segmented per-head sums, the online-softmax merge and the fp64 row store.  Included inside each
// translation unit; everything is static to it.  The helpers that take `a` read the launch's argument struct by its field names
// (H, F, HF, seg_lanes: attn_set_shape fills them).
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

// ---------------------------------------------------------------------------------------------------------------- the lane description
// what a lane knows about its four columns; fixed for the launch
template <bool UNI>
struct Lay {
  static constexpr int NK = UNI ? 1 : 4;
  int sub, gbase, col4;
  bool col_ok;
  int hk[4];                               // the heads of the lane's columns (padding columns: the last head, to which they add zeros)
  int seg_lo;                              // the lane of the group in which the head of this lane's LAST column starts
  int end_lane[NK], end_slot[NK];          // where the head of column k ends: wave lane and column slot
  bool cin_ok;                             // the head of column 0 started in an earlier lane
  bool first[4];                           // column k is the first of its head (that lane writes the head's lse / ds)
  float at[4];                             // the launch's per-column vector (gatv2.hip: attn), 0 on padding and where there is none
};

// COLS: the launch has a per-column vector col_vec [HF] (gatv2.hip: attn) that goes into Lay::at
template <int LPR, bool UNI, bool COLS, class A>
__device__ __forceinline__ Lay<UNI> make_lay(const A& a, const float* col_vec, int lane) {
  Lay<UNI> L;
  L.sub = lane % LPR;
  L.gbase = lane - L.sub;
  L.col4 = L.sub * 4;
  L.col_ok = L.col4 < a.HF;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = L.col4 + k;
    const int h = (UNI ? L.col4 : c) / a.F;
    L.hk[k] = h < a.H ? h : a.H - 1;
    L.first[k] = c < a.HF && c - (c / a.F) * a.F == 0;
    L.at[k] = (COLS && c < a.HF) ? col_vec[c] : 0.f;
  }
  L.seg_lo = (L.hk[3] * a.F) >> 2;
#pragma unroll
  for (int k = 0; k < Lay<UNI>::NK; ++k) {
    const int e = L.hk[k] * a.F + a.F - 1;
    L.end_lane[k] = L.gbase + (e >> 2);
    L.end_slot[k] = e & 3;
  }
  L.cin_ok = L.sub > 0 && L.hk[0] * a.F < L.col4;
  return L;
}

// tot[k] = the sum of t over the columns of column k's head (every lane of the wave takes part).  In fp64: a score of +-90 over 256
// columns summed in fp32 is off by a few 1e-6, which the softmax turns into a relative error of its weights and the backward's
// ds = a (c - D) multiplies by |c - D| ~ 50 on every one of a hub's 700 edges (docs/GATV2_SEMANTICS.md, Tolerances).
template <bool UNI>
__device__ __forceinline__ void head_sums(const Lay<UNI>& L, int lane, int seg_lanes, const double t[4], double tot[Lay<UNI>::NK]) {
  if constexpr (UNI) {
    double v = (t[0] + t[1]) + (t[2] + t[3]);
    for (int d = 1; d < seg_lanes; d <<= 1) {
      const double o = __shfl(v, (lane - d) & 63);
      if (L.sub - d >= L.seg_lo) v += o;
    }
    tot[0] = __shfl(v, L.end_lane[0]);
  } else {
    double p[4];                           // in-lane inclusive sums within a head
    p[0] = t[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) p[k] = (L.hk[k] == L.hk[k - 1] ? p[k - 1] : 0.0) + t[k];
    double v = p[3];
    for (int d = 1; d < seg_lanes; d <<= 1) {
      const double o = __shfl(v, (lane - d) & 63);
      if (L.sub - d >= L.seg_lo) v += o;
    }
    const double up = __shfl(v, (lane - 1) & 63);
    const double cin = L.cin_ok ? up : 0.0;
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = p[k] + (L.hk[k] == L.hk[0] ? cin : 0.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double r0 = __shfl(q[0], L.end_lane[k]), r1 = __shfl(q[1], L.end_lane[k]);
      const double r2 = __shfl(q[2], L.end_lane[k]), r3 = __shfl(q[3], L.end_lane[k]);
      const int s = L.end_slot[k];
      tot[k] = s == 0 ? r0 : s == 1 ? r1 : s == 2 ? r2 : r3;
    }
  }
}

// c[k] = <x, y> over the columns of column k's head
template <bool UNI, class A>
__device__ __forceinline__ void head_dots(const A& a, const Lay<UNI>& L, int lane, float4 x, float4 y, double c[Lay<UNI>::NK]) {
  const double t[4] = {(double)x.x * (double)y.x, (double)x.y * (double)y.y, (double)x.z * (double)y.z, (double)x.w * (double)y.w};
  head_sums<UNI>(L, lane, a.seg_lanes, t, c);
}

// the LDS of a rows kernel of pass KIND: the forward's softmax states, the destination pass's (sum a, sum a c), the wide row sums
template <int KIND, int NK>
struct HeadSmem {
  float4 part[kWaves][64];
  float4 mx[KIND == 0 ? kWaves : 1][64];
  float4 den[KIND == 0 ? kWaves : 1][64];
  double red[KIND == 1 ? kWaves : 1][64][2 * NK];
  double wide[KIND == 0 ? 1 : kWaves][64][4];
};

// ---------------------------------------------------------------------------------------------------------------- fp64 row sums
// A gradient row is a sum over the row's edges of terms that cancel (a hub's 700 terms of size 100 leave elements of size 0.1): the
// lanes add in fp64, the groups and a long row's waves are folded in fp64, and the row is rounded once.
template <int LPR>
__device__ __forceinline__ void fold_groups_wide(double v[4]) {
#pragma unroll
  for (int m = 32; m >= LPR; m >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += __shfl_xor(v[k], m);
  }
}

// the fp64 row sum of the lanes < LPR of wave 0 (a long row: over the waves, in wave order), stored to row v of out [., ldo] with zeros
// in the padding columns [hf, ..)
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void store_wide_row(float* out, int64_t ldo, int hf, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves,
                                               int lane, SM& sm, double acc[4]) {
  fold_groups_wide<LPR>(acc);
  if (n_waves > 1) {
    if (lane < LPR) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sm.wide[wave_id][lane][k] = acc[k];
    }
    __syncthreads();
    if (wave_id == 0 && lane < LPR) {
      for (int w = 1; w < n_waves; ++w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += sm.wide[w][lane][k];
      }
    }
  }
  if (wave_id == 0 && lane < LPR && L.col_ok)
    st4(out + v * ldo + L.col4, mask_cols(make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]), L.col4, hf));
  if (n_waves > 1) __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- the online softmax
// (m, den, acc) <- (m, den, acc) merged with (mo, deno, acco): two partial softmax states over disjoint edge sets
template <int NK>
__device__ __forceinline__ void merge_state(float m[NK], float den[NK], float acc[4], const float mo[NK], const float deno[NK],
                                            const float acco[4]) {
  float sa[NK], sb[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const float mn = fmaxf(m[k], mo[k]);
    sa[k] = __expf(m[k] - mn);
    sb[k] = __expf(mo[k] - mn);
    den[k] = den[k] * sa[k] + deno[k] * sb[k];
    m[k] = mn;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = acc[k] * sa[NK == 1 ? 0 : k] + acco[k] * sb[NK == 1 ? 0 : k];
}

__device__ __forceinline__ float4 pack4(const float* v, int nk) {
  return nk == 1 ? make_float4(v[0], v[0], v[0], v[0]) : make_float4(v[0], v[1 % nk], v[2 % nk], v[3 % nk]);
}

// The merge of a whole row -- the lane groups by xor moves, then a long row's waves through LDS in wave order -- is written out in
// gatv2.hip's fwd_row and as merge_row_state in gt.hip, NOT shared: as a function here, called from gatv2.hip, it left the arithmetic
// and every register count alone but gave gatv2_rows_kernel<0, ..> another instruction schedule (thousands of lines of the generated
// assembly differ).  With it written out there, gatv2.hip's device code is instruction for instruction what it was before the helpers
// above moved here, which is the condition under which they moved.

// ---------------------------------------------------------------------------------------------------------------- host side
// The shape fields of an argument struct.  GLNN_ERR_UNSUPPORTED: a shape the kernels do not take; GLNN_ERR_INVALID_ARG: arguments that
// make no sense
template <class A>
int attn_set_shape(A& a, int64_t n, int64_t nnz, int heads, int f, float p, const char* what) {
  GLNN_REQUIRE(n >= 0 && nnz >= 0 && heads >= 1 && f >= 1, "%s: bad size", what);
  GLNN_REQUIRE(p >= 0.f && p < 1.f, "%s: attn_drop in [0, 1)", what);
  if (nnz >= ((int64_t)1 << 31)) return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: nnz >= 2^31 (edge ids are 32-bit)", what);
  if (heads > 64 || (int64_t)heads * f > 256)
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: needs heads <= 64 and heads * out_feats <= 256", what);
  a.n = n; a.H = heads; a.F = f; a.HF = heads * f;
  a.seg_lanes = f % 4 == 0 ? f / 4 : (f + 2) / 4 + 1;        // most lanes a head's columns lie in
  a.thr = glnn::drop_threshold(p);
  a.dscale = 1.f / (1.f - p);
  return GLNN_OK;
}

}  // namespace
