// Graph-transformer attention (the TransformerConv of UniMP: Shi et al., IJCAI 2021, without label embedding, beta gate and edge features;
// docs/GT_SEMANTICS.md) for gfx950 (MI355X): per-destination scaled dot-product edge softmax with a skip row, forward and backward.
//
//   q / k / v / skip [N, H D] = the four projections (head-major columns)
//   e_ij[h] = <q_i[h], k_j[h]> / sqrt(D),  a_ij = softmax over the in-edges of i
//   forward  (in-CSR, row i):     out[i] = act(sum_j a_ij w_ij v[j] + skip[i]),  lse[i] = max + log(sum exp)      k[j] and v[j] gathered once
//   backward (in-CSR, row i):     c_ij = w_ij <g_i, v_j>,  D_i = sum_k a_ik c_ik / sum_k a_ik (fp64),  t_ij = a_ij (c_ij - D_i) -> t [E, H],
//                                 a_ij w_ij -> aw [E, H],  dq_i = sum_j t_ij k_j / sqrt(D)
//   backward (transposed, row j): dk_j = sum_i t_ij q_i / sqrt(D),  dv_j = sum_i (a_ij w_ij) g_i     (gathers q[i] and g[i], reads t and aw
//                                 by edge id: no score is recomputed and no cross-lane sum is needed on this side)
//   dskip = g is the caller's.
//
// w_ij = the attention dropout of gat.hip (glnn_gat_attn_mask_u8 writes the same mask out): it multiplies the aggregated term only, the
// denominator sums every edge.  The lane layout, the segmented per-head sums in fp64, the online softmax and its merges are attn_dev.h's
// (shared with gatv2.hip); rows go to waves by the two-role scan with the static assignment of short rows (as gat.hip).  No float
// atomics, no grid barrier: results are bit-identical run to run.
#include "attn_dev.h"

namespace {

constexpr int kU2 = 2;                     // edges in flight per lane group in the destination pass (two rows per edge beside q_i and g_i)

struct GtArgs {
  const int64_t* indptr; const int32_t* indices; const int32_t* eids;   // eids NULL: the edge id is the CSR position
  int64_t n; int H, F, HF, seg_lanes;
  const float* q; int64_t ldq;
  const float* k; int64_t ldk;
  const float* v; int64_t ldv;
  const float* skip; int64_t ldskip;
  double qscale;                           // 1 / sqrt(D)
  uint32_t thr, seed; float dscale;
  int relu;
  float* out; int64_t ldo;                 // forward: out; destination pass: dq; source pass: dk
  float* out2; int64_t ldo2;               // source pass: dv
  float* lse;                              // forward: optional [N, H] store; backward: the stored values
  const float* g; int64_t ldg;             // backward: gradient of the layer's output (behind the activation mask)
  float* ts; float* aw;                    // [E, H] each: t_ij and a_ij w_ij, written by the destination pass, read by the source pass
  ScanGrid sg;
};

// the states of a row's lane groups merged by xor moves into every lane, then (a long row) the waves' through LDS in wave order into wave
// 0's lanes < LPR (gatv2.hip's fwd_row has the same lines written out: attn_dev.h says why).  The caller's barrier must follow before sm
// is used again.
template <int LPR, int NK, class SM>
__device__ __forceinline__ void merge_row_state(float m[NK], float den[NK], float acc[4], int wave_id, int n_waves, int lane, SM& sm) {
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
}

// ---------------------------------------------------------------------------------------------- forward, one destination row
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void fwd_row(const GtArgs& a, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves, int lane, SM& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int g = lane / LPR;
  const float4 q4 = L.col_ok ? ld4(a.q + v * a.ldq + L.col4) : zero4();
  float m[NK], den[NK], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < NK; ++k) { m[k] = kNegBig; den[k] = 0.f; }
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
    for (int j = 0; j < cnt; j += G * kU) {
      float4 kk[kU], vv[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ei = j + u * G + g;
        const int64_t src = __shfl(my_idx, ei & 63);
        const bool ok = ei < cnt && L.col_ok;
        kk[u] = ok ? ld4(a.k + src * a.ldk + L.col4) : zero4();
        vv[u] = ok ? ld4(a.v + src * a.ldv + L.col4) : zero4();
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ei = j + u * G + g;
        double s[NK];
        head_dots<UNI>(a, L, lane, q4, kk[u], s);
        if (ei < cnt) {
          float sc[NK], w[NK];
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const double sk = s[k] * a.qscale;
            const float mn = fmaxf(m[k], (float)sk);
            sc[k] = __expf(m[k] - mn);
            const float p = __expf((float)(sk - (double)mn));
            den[k] = den[k] * sc[k] + p;
            m[k] = mn;
            w[k] = p;
            if (a.thr) w[k] = attn_keep(a.seed, a.thr, (uint32_t)(base + ei), (uint32_t)L.hk[k]) ? p * a.dscale : 0.f;
          }
          const float xs[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = acc[k] * sc[UNI ? 0 : k] + w[UNI ? 0 : k] * xs[k];
        }
      }
    }
  }
  merge_row_state<LPR, NK>(m, den, acc, wave_id, n_waves, lane, sm);      // the lane groups, then (a long row) the waves in wave order
  if (wave_id == 0 && lane < LPR && L.col_ok) {
    const float4 s4 = ld4(a.skip + v * a.ldskip + L.col4);
    const float sk[4] = {s4.x, s4.y, s4.z, s4.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = den[UNI ? 0 : k];
      o[k] = (d > 0.f ? acc[k] / d : 0.f) + sk[k];                        // a row without in-edges is its skip row
      if (a.relu) o[k] = fmaxf(o[k], 0.f);
      if (L.col4 + k >= a.HF) o[k] = 0.f;
      if (a.lse && L.first[k]) a.lse[v * a.H + L.hk[k]] = d > 0.f ? m[UNI ? 0 : k] + logf(d) : 0.f;
    }
    st4(a.out + v * a.ldo + L.col4, make_float4(o[0], o[1], o[2], o[3]));
  }
  if (n_waves > 1) __syncthreads();
}

// ---------------------------------------------------------------------------------------------- backward, destination side (in-CSR)
// Two sweeps over the row's edges, each gathering k[j] and v[j]: the first sums a_ij and a_ij c_ij per head in fp64 (D_i is the mean of the
// SAME c values under the SAME weights the second sweep uses: docs/GAT_SEMANTICS.md, "D_i"; <g_i, out_i> is not D_i here, out_i holds the
// skip row), the second recomputes a_ij and c_ij with the same instructions, writes t and a w and sums t k_j into dq_i.
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void bwd_dst_row(const GtArgs& a, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves, int lane, SM& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int g = lane / LPR;
  const float4 q4 = L.col_ok ? ld4(a.q + v * a.ldq + L.col4) : zero4();
  const float4 g4 = L.col_ok ? ld4(a.g + v * a.ldg + L.col4) : zero4();
  float lse[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) lse[k] = a.lse[v * a.H + L.hk[k]];
  double S[NK], P[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) { S[k] = 0.0; P[k] = 0.0; }
  double dq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
      const int64_t rem = e1 - base;
      const int cnt = rem < 64 ? (int)rem : 64;
      const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
      for (int j = 0; j < cnt; j += G * kU2) {
        float4 kk[kU2], vv[kU2];
#pragma unroll
        for (int u = 0; u < kU2; ++u) {
          const int ei = j + u * G + g;
          const int64_t src = __shfl(my_idx, ei & 63);
          const bool ok = ei < cnt && L.col_ok;
          kk[u] = ok ? ld4(a.k + src * a.ldk + L.col4) : zero4();
          vv[u] = ok ? ld4(a.v + src * a.ldv + L.col4) : zero4();
        }
#pragma unroll
        for (int u = 0; u < kU2; ++u) {
          const int ei = j + u * G + g;
          double s[NK], c[NK];
          head_dots<UNI>(a, L, lane, q4, kk[u], s);
          head_dots<UNI>(a, L, lane, g4, vv[u], c);
          if (ei < cnt) {
            const int64_t eid = base + ei;
            float tv[NK], wv[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
              const float at = __expf((float)(s[k] * a.qscale - (double)lse[k]));
              double cw = c[k] * (double)a.dscale;
              wv[k] = at * a.dscale;
              if (a.thr && !attn_keep(a.seed, a.thr, (uint32_t)eid, (uint32_t)L.hk[k])) { cw = 0.0; wv[k] = 0.f; }
              if (sweep == 0) {
                S[k] += (double)at;
                P[k] += (double)at * cw;
              } else {
                tv[k] = at * (float)(cw - P[k]);                // P holds D_i in the second sweep
              }
            }
            if (sweep == 1) {
              const float ks[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const float t = tv[UNI ? 0 : k];
                if (L.first[k] && (!UNI || k == 0)) {
                  a.ts[eid * a.H + L.hk[k]] = t;
                  a.aw[eid * a.H + L.hk[k]] = wv[UNI ? 0 : k];
                }
                dq[k] = fma((double)t, (double)ks[k], dq[k]);
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
#pragma unroll
  for (int k = 0; k < 4; ++k) dq[k] *= a.qscale;
  store_wide_row<LPR, UNI>(a.out, a.ldo, a.HF, L, v, wave_id, n_waves, lane, sm, dq);
}

// ---------------------------------------------------------------------------------------------- backward, source side (transposed CSR)
template <int LPR, bool UNI, class SM>
__device__ __forceinline__ void bwd_src_row(const GtArgs& a, const Lay<UNI>& L, int64_t v, int wave_id, int n_waves, int lane, SM& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int g = lane / LPR;
  double dk[4] = {0.0, 0.0, 0.0, 0.0}, dv[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? ld_idx_stream(a.indices + base + lane) : 0;
    const int my_eid = lane < cnt ? (a.eids ? ld_idx_stream(a.eids + base + lane) : (int)(base + lane)) : 0;
    for (int j = 0; j < cnt; j += G * kU2) {
      float4 qq[kU2], gg[kU2];
      float t[kU2][NK], w[kU2][NK];
#pragma unroll
      for (int u = 0; u < kU2; ++u) {
        const int ei = j + u * G + g;
        const int64_t dst = __shfl(my_idx, ei & 63);
        const int64_t eid = __shfl(my_eid, ei & 63);
        const bool ok = ei < cnt && L.col_ok;
        qq[u] = ok ? ld4(a.q + dst * a.ldq + L.col4) : zero4();
        gg[u] = ok ? ld4(a.g + dst * a.ldg + L.col4) : zero4();
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          t[u][k] = ok ? a.ts[eid * a.H + L.hk[k]] : 0.f;
          w[u][k] = ok ? a.aw[eid * a.H + L.hk[k]] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < kU2; ++u) {
        const float qs[4] = {qq[u].x, qq[u].y, qq[u].z, qq[u].w}, gs[4] = {gg[u].x, gg[u].y, gg[u].z, gg[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          dk[k] = fma((double)t[u][UNI ? 0 : k], (double)qs[k], dk[k]);
          dv[k] = fma((double)w[u][UNI ? 0 : k], (double)gs[k], dv[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) dk[k] *= a.qscale;
  store_wide_row<LPR, UNI>(a.out, a.ldo, a.HF, L, v, wave_id, n_waves, lane, sm, dk);
  store_wide_row<LPR, UNI>(a.out2, a.ldo2, a.HF, L, v, wave_id, n_waves, lane, sm, dv);
}

// KIND 0 forward, 1 backward over the in-CSR (t, a w, dq), 2 backward over the transposed CSR (dk, dv)
template <int KIND, int LPR, bool UNI>
__global__ __launch_bounds__(kBlock) void gt_rows_kernel(const GtArgs a) {
  __shared__ HeadSmem<KIND, UNI ? 1 : 4> sm;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Lay<UNI> L = make_lay<LPR, UNI, false>(a, nullptr, lane);
  auto do_row = [&](int64_t v, int wave_id, int n_waves) {
    if (KIND == 0) fwd_row<LPR, UNI>(a, L, v, wave_id, n_waves, lane, sm);
    else if (KIND == 1) bwd_dst_row<LPR, UNI>(a, L, v, wave_id, n_waves, lane, sm);
    else bwd_src_row<LPR, UNI>(a, L, v, wave_id, n_waves, lane, sm);
  };
  // row_gather_dev.h's two roles, short rows assigned statically: gatv2_rows_kernel's loops without the ascending order of its KIND 1
  // (no sum here runs across rows, so the order in which a trip's long rows come does not matter)
  if ((int)blockIdx.x < a.sg.n_long_blocks) {
    const int64_t n_chunks = (a.n + kBlock - 1) / kBlock;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += a.sg.n_long_blocks) {
      const int64_t* rows;
      const int n_found = find_long_rows(a.indptr, a.n, n_chunks, chunk, &rows);
      for (int i = 0; i < n_found; ++i) {
        do_row(rows[i], wave, kWaves);
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
}

int rows_launch(GtArgs& a, int kind, const char* what, void* stream) {
  with_attn_variant(kind, a.F % 4 == 0, lpr_for((a.HF + 3) / 4, 4), [&](auto K, auto U, auto L) {
    hipLaunchKernelGGL((gt_rows_kernel<decltype(K)::value, decltype(L)::value, decltype(U)::value>), dim3(a.sg.grid_x), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
  });
  return glnn::check_launch(what);
}

}  // namespace

extern "C" int glnn_gt_attn_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* q, int64_t ldq,
                                    const float* k, int64_t ldk, const float* v, int64_t ldv, const float* skip, int64_t ldskip, int heads,
                                    int out_feats, float attn_drop, uint32_t seed, int relu, float* out, int64_t ldo, float* lse,
                                    void* stream) {
  const char* what = "glnn_gt_attn_fwd_f32";
  GtArgs a = {};
  int rc = attn_set_shape(a, n, nnz, heads, out_feats, attn_drop, what);
  if (rc != GLNN_OK) return rc;
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && (indices || nnz == 0) && q && k && v && skip && out, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(q, ldq, a.HF) && rows_ok(k, ldk, a.HF) && rows_ok(v, ldv, a.HF) && rows_ok(skip, ldskip, a.HF) &&
               rows_ok(out, ldo, a.HF) && out != q && out != k && out != v && out != skip,
               "%s: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(heads * out_feats); out must not alias "
               "q, k, v or skip", what);
  rc = scan_grid(n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  a.indptr = indptr; a.indices = indices; a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.skip = skip; a.ldskip = ldskip;
  a.qscale = 1.0 / sqrt((double)out_feats);
  a.seed = seed; a.relu = relu ? 1 : 0; a.out = out; a.ldo = ldo; a.lse = lse;
  return rows_launch(a, 0, what, stream);
}

extern "C" int64_t glnn_gt_attn_bwd_workspace_floats(int64_t nnz, int heads) {
  if (nnz < 1 || heads < 1 || nnz >= ((int64_t)1 << 31)) return 0;
  return nnz * heads;                                            // a_ij w_ij per edge and head
}

extern "C" int glnn_gt_attn_bwd_f32(const int64_t* indptr, const int32_t* indices, const int64_t* t_indptr, const int32_t* t_indices,
                                    const int32_t* t_eids, int64_t n, int64_t nnz, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                    const float* v, int64_t ldv, int heads, int out_feats, const float* lse, const float* g, int64_t ldg,
                                    float attn_drop, uint32_t seed, float* t, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv,
                                    int64_t lddv, float* workspace, int64_t workspace_floats, void* stream) {
  const char* what = "glnn_gt_attn_bwd_f32";
  GtArgs a = {};
  int rc = attn_set_shape(a, n, nnz, heads, out_feats, attn_drop, what);
  if (rc != GLNN_OK) return rc;
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && t_indptr && (nnz == 0 || (indices && t_indices && t_eids && t && workspace)) && q && k && v && lse && g && dq &&
               dk && dv, "%s: null pointer", what);
  GLNN_REQUIRE(rows_ok(q, ldq, a.HF) && rows_ok(k, ldk, a.HF) && rows_ok(v, ldv, a.HF) && rows_ok(g, ldg, a.HF) && rows_ok(dq, lddq, a.HF) &&
               rows_ok(dk, lddk, a.HF) && rows_ok(dv, lddv, a.HF),
               "%s: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(heads * out_feats)", what);
  for (const float* o : {(const float*)dq, (const float*)dk, (const float*)dv})
    GLNN_REQUIRE(o != q && o != k && o != v && o != g, "%s: dq, dk and dv must not alias an input", what);
  GLNN_REQUIRE(dq != dk && dq != dv && dk != dv, "%s: dq, dk and dv must not alias each other", what);
  GLNN_REQUIRE(workspace_floats >= glnn_gt_attn_bwd_workspace_floats(nnz, heads), "%s: workspace too small", what);
  rc = scan_grid(n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.qscale = 1.0 / sqrt((double)out_feats); a.seed = seed;
  a.lse = const_cast<float*>(lse); a.g = g; a.ldg = ldg; a.ts = t; a.aw = workspace;
  a.indptr = indptr; a.indices = indices; a.eids = nullptr; a.out = dq; a.ldo = lddq;
  rc = rows_launch(a, 1, what, stream);
  if (rc != GLNN_OK) return rc;
  a.indptr = t_indptr; a.indices = t_indices; a.eids = t_eids; a.out = dk; a.ldo = lddk; a.out2 = dv; a.ldo2 = lddv;
  return rows_launch(a, 2, what, stream);
}
