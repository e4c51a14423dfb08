// GATv2 attention (Brody, Alon, Yahav, ICLR 2022; docs/GATV2_SEMANTICS.md) for gfx950 (MI355X): per-destination edge softmax whose score
// needs the WHOLE projected source row, forward and backward.
//
//   zl / zr [N, H F] = the two projections (head-major columns), attn [H F]
//   u_ij = zl[j] + zr[i],  s_ij[h] = sum_f attn[h, f] leaky_relu(u_ij[h, f]),  a_ij = softmax over the in-edges of i
//   forward  (in-CSR, row i):     out[i] = act(sum_j a_ij w_ij zl[j]),  lse[i] = max + log(sum exp)            ONE gather of zl[j] per edge
//   backward (in-CSR, row i):     c_ij = w_ij <g_i, zl_j>,  D_i = sum_k a_ik c_ik / sum_k a_ik (fp64),  ds_ij = a_ij (c_ij - D_i) -> ds [E, H],
//                                 dzr_i = sum_j de_ij,  de_ij[f] = ds_ij attn[f] lrelu'(u_ij[f]),  dattn[f] += ds_ij lrelu(u_ij[f])
//   backward (transposed, row j): dzl_j = sum_i a_ij w_ij g_i + de_ij     (gathers zr[i] and g[i], reads ds and lse[i] by edge id / row)
//
// w_ij = the attention dropout of gat.hip (glnn_gat_attn_mask_u8 writes the same mask out): it multiplies the aggregated term only, the
// denominator sums every edge, so an edge with every head dropped is still gathered -- its score is part of the softmax.
//
// Lane layout: row_gather_dev.h's.  A row of H F <= 256 floats is LPR lanes moving float4; the G = 64 / LPR lane groups take different
// edges.  A head's score is a sum over the head's columns, which are CONSECUTIVE lanes of the group but neither a power of two of them nor
// (F % 4 != 0) whole lanes: an inclusive segmented scan over the lanes (log2 steps, the segment starts are fixed per lane) leaves every
// head's total in the lane of its last column, from where the head's lanes fetch it -- one cross-lane move when a lane's four columns share
// a head (UNI, F % 4 == 0), the slot picked per column otherwise.  Each group keeps a running (max, denominator, accumulator) per column
// and updates it online, edge by edge in ascending order; the groups are merged with xor moves, a long row's eight waves through LDS in wave
// order.  Rows go to waves by the two-role scan with the static assignment of short rows (as gat.hip).  No float atomics, no grid barrier.
#include "attn_dev.h"

namespace {

constexpr int kU2 = 2;                     // edges in flight per lane group in the source pass (two rows are gathered per edge; else kU)
constexpr int kFoldPer = 128;              // dattn partials summed per workgroup of the first fold

struct V2Args {
  const int64_t* indptr; const int32_t* indices; const int32_t* eids;   // eids NULL: the edge id is the CSR position
  int64_t n; int H, F, HF, seg_lanes;
  const float* zl; int64_t ldzl;
  const float* zr; int64_t ldzr;
  const float* attn;
  float slope; uint32_t thr, seed; float dscale;
  int relu;
  float* out; int64_t ldo;                 // forward: out; destination pass: dzr; source pass: dzl
  float* lse;                              // forward: optional [N, H] store; backward: the stored values
  const float* g; int64_t ldg;             // backward: gradient of the layer's output (behind the activation mask)
  float* ds;                               // [E, H] scratch
  float* part;                             // destination pass: [grid_x, H F] partials of dattn
  ScanGrid sg;
};

// u = zl_j + zr_i of the lane's columns and the scores of their heads
template <bool UNI>
__device__ __forceinline__ void edge_scores(const V2Args& a, const Lay<UNI>& L, int lane, float4 zl, float4 zr, float u[4],
                                            double s[Lay<UNI>::NK]) {
  u[0] = zl.x + zr.x; u[1] = zl.y + zr.y; u[2] = zl.z + zr.z; u[3] = zl.w + zr.w;
  const double ud[4] = {(double)zl.x + (double)zr.x, (double)zl.y + (double)zr.y, (double)zl.z + (double)zr.z, (double)zl.w + (double)zr.w};
  double t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = (double)L.at[k] * (ud[k] > 0.0 ? ud[k] : ud[k] * (double)a.slope);
  head_sums<UNI>(L, lane, a.seg_lanes, t, s);
}

// ---------------------------------------------------------------------------------------------- forward, one destination row
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void fwd_row(const V2Args& a, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves, int lane, SM& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int g = lane / LPR;
  const float4 zr4 = L.col_ok ? ld4(a.zr + v * a.ldzr + L.col4) : zero4();
  float m[NK], den[NK], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < NK; ++k) { m[k] = kNegBig; den[k] = 0.f; }
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
    for (int j = 0; j < cnt; j += G * kU) {
      float4 x[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ei = j + u * G + g;
        const int src = __shfl(my_idx, ei & 63);
        x[u] = (ei < cnt && L.col_ok) ? ld4(a.zl + (int64_t)src * a.ldzl + L.col4) : zero4();
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ei = j + u * G + g;
        float uu[4];
        double s[NK];
        edge_scores<UNI>(a, L, lane, x[u], zr4, uu, s);
        if (ei < cnt) {
          float sc[NK], w[NK];
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const float mn = fmaxf(m[k], (float)s[k]);
            sc[k] = __expf(m[k] - mn);
            const float p = __expf((float)(s[k] - (double)mn));
            den[k] = den[k] * sc[k] + p;
            m[k] = mn;
            w[k] = p;
            if (a.thr) w[k] = attn_keep(a.seed, a.thr, (uint32_t)(base + ei), (uint32_t)L.hk[k]) ? p * a.dscale : 0.f;
          }
          const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = acc[k] * sc[UNI ? 0 : k] + w[UNI ? 0 : k] * xs[k];
        }
      }
    }
  }
  // the lane groups, then (a long row) the waves in wave order
#pragma unroll
  for (int mask = 32; mask >= LPR; mask >>= 1) {
    float mo[NK], deno[NK], acco[4];
#pragma unroll
    for (int k = 0; k < NK; ++k) { mo[k] = __shfl_xor(m[k], mask); deno[k] = __shfl_xor(den[k], mask); }
#pragma unroll
    for (int k = 0; k < 4; ++k) acco[k] = __shfl_xor(acc[k], mask);
    merge_state<NK>(m, den, acc, mo, deno, acco);
  }
  if (n_waves > 1) {
    if (lane < LPR) {
      sm.part[wave_id][lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      sm.mx[wave_id][lane] = pack4(m, NK);
      sm.den[wave_id][lane] = pack4(den, NK);
    }
    __syncthreads();
    if (wave_id == 0 && lane < LPR) {
      for (int w = 1; w < n_waves; ++w) {
        const float4 pa = sm.part[w][lane], pm = sm.mx[w][lane], pd = sm.den[w][lane];
        const float mo4[4] = {pm.x, pm.y, pm.z, pm.w}, do4[4] = {pd.x, pd.y, pd.z, pd.w}, acco[4] = {pa.x, pa.y, pa.z, pa.w};
        float mo[NK], deno[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) { mo[k] = mo4[k]; deno[k] = do4[k]; }
        merge_state<NK>(m, den, acc, mo, deno, acco);
      }
    }
  }
  if (wave_id == 0 && lane < LPR && L.col_ok) {
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = den[UNI ? 0 : k];
      o[k] = d > 0.f ? acc[k] / d : 0.f;
      if (a.relu) o[k] = fmaxf(o[k], 0.f);
      if (L.col4 + k >= a.HF) o[k] = 0.f;
      if (a.lse && L.first[k]) a.lse[v * a.H + L.hk[k]] = d > 0.f ? m[UNI ? 0 : k] + logf(d) : 0.f;
    }
    st4(a.out + v * a.ldo + L.col4, make_float4(o[0], o[1], o[2], o[3]));
  }
  if (n_waves > 1) __syncthreads();
}

// ---------------------------------------------------------------------------------------------- backward, destination side (in-CSR)
// Two sweeps over the row's edges, each gathering zl[j]: the first sums a_ij and a_ij c_ij per head in fp64 (D_i is the mean of the SAME
// c values under the SAME weights the second sweep uses: docs/GAT_SEMANTICS.md, "D_i"), the second recomputes a_ij and c_ij with the same
// instructions, writes ds and sums de into dzr_i and ds lrelu(u) into the wave's dattn registers (datt).
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void bwd_dst_row(const V2Args& a, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves, int lane, SM& sm,
                                            float datt[4]) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int g = lane / LPR;
  const float4 zr4 = L.col_ok ? ld4(a.zr + v * a.ldzr + L.col4) : zero4();
  const float4 g4 = L.col_ok ? ld4(a.g + v * a.ldg + L.col4) : zero4();
  float lse[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) lse[k] = a.lse[v * a.H + L.hk[k]];
  double S[NK], P[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) { S[k] = 0.0; P[k] = 0.0; }
  double dz[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
      const int64_t rem = e1 - base;
      const int cnt = rem < 64 ? (int)rem : 64;
      const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
      for (int j = 0; j < cnt; j += G * kU) {
        float4 x[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int ei = j + u * G + g;
          const int src = __shfl(my_idx, ei & 63);
          x[u] = (ei < cnt && L.col_ok) ? ld4(a.zl + (int64_t)src * a.ldzl + L.col4) : zero4();
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int ei = j + u * G + g;
          float uu[4];
          double s[NK], c[NK];
          edge_scores<UNI>(a, L, lane, x[u], zr4, uu, s);
          head_dots<UNI>(a, L, lane, g4, x[u], c);
          if (ei < cnt) {
            const int64_t eid = base + ei;
            float dsv[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
              const float at = __expf((float)(s[k] - (double)lse[k]));
              double cw = c[k] * (double)a.dscale;
              if (a.thr && !attn_keep(a.seed, a.thr, (uint32_t)eid, (uint32_t)L.hk[k])) cw = 0.0;
              if (sweep == 0) {
                S[k] += (double)at;
                P[k] += (double)at * cw;
              } else {
                dsv[k] = at * (float)(cw - P[k]);              // P holds D_i in the second sweep
              }
            }
            if (sweep == 1) {
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const float d = dsv[UNI ? 0 : k];
                if (L.first[k] && (!UNI || k == 0)) a.ds[eid * a.H + L.hk[k]] = d;
                dz[k] += (double)((d * L.at[k]) * (uu[k] > 0.f ? 1.f : a.slope));
                datt[k] = fmaf(d, lrelu(uu[k], a.slope), datt[k]);
              }
            }
          }
        }
      }
    }
    if (sweep == 0) {
#pragma unroll
      for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int mask = 32; mask >= LPR; mask >>= 1) { S[k] += __shfl_xor(S[k], mask); P[k] += __shfl_xor(P[k], mask); }
      }
      if (n_waves > 1) {
        if (lane < LPR) {
#pragma unroll
          for (int k = 0; k < NK; ++k) { sm.red[wave_id][lane][2 * k] = S[k]; sm.red[wave_id][lane][2 * k + 1] = P[k]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          S[k] = sm.red[0][L.sub][2 * k]; P[k] = sm.red[0][L.sub][2 * k + 1];
          for (int w = 1; w < n_waves; ++w) { S[k] += sm.red[w][L.sub][2 * k]; P[k] += sm.red[w][L.sub][2 * k + 1]; }
        }
      }
#pragma unroll
      for (int k = 0; k < NK; ++k) P[k] = S[k] > 0.0 ? P[k] / S[k] : 0.0;
    }
  }
  store_wide_row<LPR, UNI>(a.out, a.ldo, a.HF, L, v, wave_id, n_waves, lane, sm, dz);
}

// ---------------------------------------------------------------------------------------------- backward, source side (transposed CSR)
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void bwd_src_row(const V2Args& a, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves, int lane, SM& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int g = lane / LPR;
  const float4 zl4 = L.col_ok ? ld4(a.zl + v * a.ldzl + L.col4) : zero4();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
    const int my_eid = lane < cnt ? (a.eids ? ld_idx_stream(a.eids + base + lane) : (int)(base + lane)) : 0;
    for (int j = 0; j < cnt; j += G * kU2) {
      float4 r[kU2], gg[kU2];
      int64_t dst[kU2], eid[kU2];
#pragma unroll
      for (int u = 0; u < kU2; ++u) {
        const int ei = j + u * G + g;
        dst[u] = __shfl(my_idx, ei & 63);
        eid[u] = __shfl(my_eid, ei & 63);
        const bool ok = ei < cnt && L.col_ok;
        r[u] = ok ? ld4(a.zr + dst[u] * a.ldzr + L.col4) : zero4();
        gg[u] = ok ? ld4(a.g + dst[u] * a.ldg + L.col4) : zero4();
      }
#pragma unroll
      for (int u = 0; u < kU2; ++u) {
        const int ei = j + u * G + g;
        float uu[4];
        double s[NK];
        edge_scores<UNI>(a, L, lane, zl4, r[u], uu, s);
        if (ei < cnt) {
          float w[NK], dsv[NK];
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const float at = __expf((float)(s[k] - (double)a.lse[dst[u] * a.H + L.hk[k]]));
            w[k] = at * a.dscale;
            if (a.thr && !attn_keep(a.seed, a.thr, (uint32_t)eid[u], (uint32_t)L.hk[k])) w[k] = 0.f;
            dsv[k] = a.ds[eid[u] * a.H + L.hk[k]];
          }
          const float gs[4] = {gg[u].x, gg[u].y, gg[u].z, gg[u].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[k] = fma((double)w[UNI ? 0 : k], (double)gs[k], acc[k]);
            acc[k] += (double)((dsv[UNI ? 0 : k] * L.at[k]) * (uu[k] > 0.f ? 1.f : a.slope));
          }
        }
      }
    }
  }
  store_wide_row<LPR, UNI>(a.out, a.ldo, a.HF, L, v, wave_id, n_waves, lane, sm, acc);
}

// KIND 0 forward, 1 backward over the in-CSR (ds, dzr, dattn partials), 2 backward over the transposed CSR (dzl)
template <int KIND, int LPR, bool UNI>
__global__ __launch_bounds__(kBlock) void gatv2_rows_kernel(const V2Args a) {
  __shared__ HeadSmem<KIND, UNI ? 1 : 4> sm;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Lay<UNI> L = make_lay<LPR, UNI, true>(a, a.attn, lane);
  float datt[4] = {0.f, 0.f, 0.f, 0.f};
  auto do_row = [&](int64_t v, int wave_id, int n_waves) {
    if (KIND == 0) fwd_row<LPR, UNI>(a, L, v, wave_id, n_waves, lane, sm);
    else if (KIND == 1) bwd_dst_row<LPR, UNI>(a, L, v, wave_id, n_waves, lane, sm, datt);
    else bwd_src_row<LPR, UNI>(a, L, v, wave_id, n_waves, lane, sm);
  };
  // row_gather_dev.h's two roles, short rows assigned statically: gat_rows_kernel's loops plus the ascending order of KIND 1, written
  // out in both.  THIS kernel keeps every register figure behind a shared scan_rows_static; gat.hip's KIND 2 does not (see there).
  if ((int)blockIdx.x < a.sg.n_long_blocks) {
    const int64_t n_chunks = (a.n + kBlock - 1) / kBlock;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += a.sg.n_long_blocks) {
      const int64_t* rows;
      const int n_found = find_long_rows(a.indptr, a.n, n_chunks, chunk, &rows);
      int64_t last = -1;
      for (int i = 0; i < n_found; ++i) {
        int64_t v = rows[i];
        if (KIND == 1) {                                          // ascending rows: the trip's rows come in any order, and the sum
          v = INT64_MAX;                                          // in the dattn registers must have a fixed one
          for (int q = 0; q < n_found; ++q) {
            const int64_t r = rows[q];
            if (r > last && r < v) v = r;
          }
          last = v;
        }
        do_row(v, wave, kWaves);
        __syncthreads();
      }
    }
  } else {
    const int64_t row_base = ((int64_t)blockIdx.x - a.sg.n_long_blocks) * a.sg.rows_per_block;
    for (int lr = wave; lr < a.sg.rows_per_block; lr += kWaves) {
      const int64_t v = row_base + lr;
      if (v >= a.n) break;
      if (a.indptr[v + 1] - a.indptr[v] > kLongRow) continue;
      do_row(v, 0, 1);
    }
  }
  if (KIND == 1) {                                                // this workgroup's share of dattn: groups, then waves in wave order
    float4 d4 = fold_groups<LPR>(make_float4(datt[0], datt[1], datt[2], datt[3]));
    __syncthreads();
    if (lane < LPR) sm.part[wave][lane] = d4;
    __syncthreads();
    if (wave == 0 && lane < LPR && L.col_ok) {
      d4 = sm.part[0][lane];
      for (int w = 1; w < kWaves; ++w) d4 = add4(d4, sm.part[w][lane]);
      const float o[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (L.col4 + k < a.HF) a.part[(int64_t)blockIdx.x * a.HF + L.col4 + k] = o[k];
    }
  }
}

// out[b] = sum of the partials [b per, (b + 1) per) in ascending order (thread = column)
__global__ __launch_bounds__(256) void gatv2_fold_kernel(const float* __restrict__ part, int64_t nparts, int per, int HF, float* __restrict__ out) {
  const int c = threadIdx.x;
  if (c >= HF) return;
  const int64_t p0 = (int64_t)blockIdx.x * per;
  const int64_t p1 = p0 + per < nparts ? p0 + per : nparts;
  float s = 0.f;
  for (int64_t p = p0; p < p1; ++p) s += part[p * HF + c];
  out[(int64_t)blockIdx.x * HF + c] = s;
}

int rows_launch(V2Args& a, int kind, const char* what, void* stream) {
  with_attn_variant(kind, a.F % 4 == 0, lpr_for((a.HF + 3) / 4, 4), [&](auto K, auto U, auto L) {
    hipLaunchKernelGGL((gatv2_rows_kernel<decltype(K)::value, decltype(L)::value, decltype(U)::value>), dim3(a.sg.grid_x), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
  });
  return glnn::check_launch(what);
}

}  // namespace

extern "C" int glnn_gatv2_attn_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* zl, int64_t ldzl,
                                       const float* zr, int64_t ldzr, int heads, int out_feats, const float* attn, float negative_slope,
                                       float attn_drop, uint32_t seed, int relu, float* out, int64_t ldo, float* lse, void* stream) {
  const char* what = "glnn_gatv2_attn_fwd_f32";
  V2Args a = {};
  int rc = attn_set_shape(a, n, nnz, heads, out_feats, attn_drop, what);
  if (rc != GLNN_OK) return rc;
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && (indices || nnz == 0) && zl && zr && attn && out, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(zl, ldzl, a.HF) && rows_ok(zr, ldzr, a.HF) && rows_ok(out, ldo, a.HF) && out != zl && out != zr,
               "%s: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(heads * out_feats); out must not alias "
               "zl or zr", what);
  rc = scan_grid(n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  a.indptr = indptr; a.indices = indices; a.zl = zl; a.ldzl = ldzl; a.zr = zr; a.ldzr = ldzr; a.attn = attn; a.slope = negative_slope;
  a.seed = seed; a.relu = relu ? 1 : 0; a.out = out; a.ldo = ldo; a.lse = lse;
  return rows_launch(a, 0, what, stream);
}

extern "C" int64_t glnn_gatv2_attn_bwd_workspace_floats(int64_t n, int heads, int out_feats) {
  ScanGrid sg;
  if (n < 1 || heads < 1 || out_feats < 1 || scan_grid(n, "glnn_gatv2_attn_bwd_workspace_floats", &sg) != GLNN_OK) return 0;
  const int64_t nparts = sg.grid_x;
  return (nparts + (nparts + kFoldPer - 1) / kFoldPer) * heads * out_feats;
}

extern "C" int glnn_gatv2_attn_bwd_f32(const int64_t* indptr, const int32_t* indices, const int64_t* t_indptr, const int32_t* t_indices,
                                       const int32_t* t_eids, int64_t n, int64_t nnz, const float* zl, int64_t ldzl, const float* zr,
                                       int64_t ldzr, int heads, int out_feats, const float* lse, const float* attn, const float* g,
                                       int64_t ldg, float negative_slope, float attn_drop, uint32_t seed, float* ds, float* dzl,
                                       int64_t lddzl, float* dzr, int64_t lddzr, float* dattn, float* workspace, int64_t workspace_floats,
                                       void* stream) {
  const char* what = "glnn_gatv2_attn_bwd_f32";
  V2Args a = {};
  int rc = attn_set_shape(a, n, nnz, heads, out_feats, attn_drop, what);
  if (rc != GLNN_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n == 0) {                                                   // no rows: dattn (when given) is the empty sum
    if (!dattn) return GLNN_OK;
    hipLaunchKernelGGL(gatv2_fold_kernel, dim3(1), dim3(256), 0, st, workspace, (int64_t)0, 1, a.HF, dattn);
    return glnn::check_launch(what);
  }
  GLNN_REQUIRE(indptr && t_indptr && (nnz == 0 || (indices && t_indices && t_eids && ds)) && zl && zr && lse && attn && g && dzl && dzr &&
               dattn && workspace, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(zl, ldzl, a.HF) && rows_ok(zr, ldzr, a.HF) && rows_ok(g, ldg, a.HF) && rows_ok(dzl, lddzl, a.HF) &&
               rows_ok(dzr, lddzr, a.HF) && dzl != g && dzl != zl && dzl != zr && dzr != g && dzr != zl && dzr != zr && dzl != dzr,
               "%s: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(heads * out_feats); dzl and dzr must not "
               "alias an input or each other", what);
  GLNN_REQUIRE(workspace_floats >= glnn_gatv2_attn_bwd_workspace_floats(n, heads, out_feats), "%s: workspace too small", what);
  rc = scan_grid(n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  const int64_t nparts = a.sg.grid_x, n1 = (nparts + kFoldPer - 1) / kFoldPer;
  a.zl = zl; a.ldzl = ldzl; a.zr = zr; a.ldzr = ldzr; a.attn = attn; a.slope = negative_slope; a.seed = seed;
  a.lse = const_cast<float*>(lse); a.g = g; a.ldg = ldg; a.ds = ds; a.part = workspace;
  a.indptr = indptr; a.indices = indices; a.eids = nullptr; a.out = dzr; a.ldo = lddzr;
  rc = rows_launch(a, 1, what, stream);
  if (rc != GLNN_OK) return rc;
  a.indptr = t_indptr; a.indices = t_indices; a.eids = t_eids; a.out = dzl; a.ldo = lddzl;
  rc = rows_launch(a, 2, what, stream);
  if (rc != GLNN_OK) return rc;
  float* part2 = workspace + nparts * a.HF;
  hipLaunchKernelGGL(gatv2_fold_kernel, dim3((unsigned)n1), dim3(256), 0, st, workspace, nparts, kFoldPer, a.HF, part2);
  hipLaunchKernelGGL(gatv2_fold_kernel, dim3(1), dim3(256), 0, st, part2, n1, (int)n1, a.HF, dattn);
  return glnn::check_launch(what);
}
