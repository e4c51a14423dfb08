// GAT attention (dgl 0.6.1 GATConv of the reference GAT teacher, models.py:202-279) for gfx950 (MI355X): per-destination edge softmax
// with per-edge scores from two per-node scalars per head, forward and backward.  docs/GAT_SEMANTICS.md states the arithmetic.
//
//   z [N, H F] = the projected rows (head-major columns), el / er [N, H] = <z, attn_l> / <z, attn_r> per head (gat_scores_kernel)
//   forward  (in-CSR, row i):     e_ij = leaky_relu(el[j] + er[i]),  a_ij = exp(e_ij - max_i) / sum_i,  out[i] = act(sum_j a_ij w_ij z[j])
//   backward (in-CSR, row i):     ds_ij = a_ij (w_ij <g_i, z_j> - <g_i, out_i>) * (e_ij > 0 ? 1 : slope)  -> ds [E, H],  der_i = sum_j ds_ij
//                                 (<g_i, out_i> as sum_k a_ik w_ik <g_i, z_k> / sum_k a_ik in fp64: see bwd_dst_row)
//   backward (transposed, row j): dz_j = sum_i a_ij w_ij g_i + del_j attn_l + der_j attn_r,   del_j = sum_i ds_ij (read by edge id)
//   dattn_l / dattn_r = column sums of del z / der z: per-workgroup partials, folded in fixed order
//
// w_ij = the attention dropout: keep iff (drop_hash(seed, edge id, head) & 0xFFFF) >= threshold, weight 1 / (1 - p); evaluated on the fly in
// every pass (glnn_gat_attn_mask_u8 writes it out for tests).  Nothing E x H x F is stored; eval mode stores nothing of size E; training keeps
// the row log-sum-exp [N, H] and one [E, H] scratch (ds).
//
// Two lane layouts.  Scores: lane = (edge slot, head) with HP = pow2 >= H heads per slot, 64 / HP edges per step, 4 H bytes gathered per edge;
// per-head reductions are xor butterflies over the slots.  Values: a row of H F <= 256 floats is LPR lanes moving float4, the G = 64 / LPR
// lane groups take different edges and are folded with cross-lane adds (row_gather_dev.h's mapping); each lane recomputes the weight of its
// own head from el[j] (4 bytes, the same 32-byte segment for the whole group).  Rows go to waves by that header's two-role scan with the
// static assignment of short rows; a long row's eight partials are folded through LDS in wave order.  No float atomics.
#include "attn_dev.h"

namespace {

struct GatArgs {
  const int64_t* indptr; const int32_t* indices; const int32_t* eids;   // eids NULL: the edge id is the CSR position
  int64_t n; int H, F, HF, hp_shift;
  const float* z; int64_t ldz;             // forward: gathered rows; backward (dst pass): gathered rows
  const float* el; const float* er;        // [N, H]
  float slope; uint32_t thr, seed; float dscale;
  int relu;
  float* out; int64_t ldo;                 // forward: out; src pass: dz
  float* lse;                              // forward: optional [N, H] store; backward: the stored values
  const float* g; int64_t ldg;             // backward: gradient of the layer's output (behind the activation mask)
  const float* y; int64_t ldy;             // backward: the layer's stored output (kept in the C ABI, not read: see bwd_dst_row)
  float* ds;                               // [E, H] scratch
  float* der; float* del_;                 // [N, H]
  const float* attn_l; const float* attn_r;
  ScanGrid sg;
};

struct Smem {
  double red[kWaves][64];                   // holds a float exactly; the backward's per-head sums are doubles
  float4 part[kWaves][64];
  float4 part2[kWaves][64];
};

__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }

// per-head reduction over the edge slots of a wave (and, for a long row, over the workgroup's waves in wave order)
template <bool MAX, typename T>
__device__ __forceinline__ T reduce_heads(T v, int HP, int h, int wave_id, int n_waves, int lane, Smem& sm) {
  for (int m = HP; m < 64; m <<= 1) {
    const T o = __shfl_xor(v, m);
    v = MAX ? max_of(v, o) : v + o;
  }
  if (n_waves > 1) {
    if (lane < HP) sm.red[wave_id][lane] = v;
    __syncthreads();
    v = (T)sm.red[0][h];
    for (int w = 1; w < n_waves; ++w) v = MAX ? max_of(v, (T)sm.red[w][h]) : v + (T)sm.red[w][h];
    __syncthreads();
  }
  return v;
}

// the heads of a lane's four columns (clamped for padding columns)
template <bool UNI>
__device__ __forceinline__ void lane_heads(const GatArgs& a, int col4, int hk[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int h = (col4 + (UNI ? 0 : k)) / a.F;
    hk[k] = h < a.H ? h : a.H - 1;
  }
}

// ---------------------------------------------------------------------------------------------- forward, one destination row
template <int LPR, bool UNI>
__device__ __forceinline__ void fwd_row(const GatArgs& a, int64_t v, int wave_id, int n_waves, int lane, Smem& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int HP = 1 << a.hp_shift, EPP = 64 >> a.hp_shift;
  const int slot = lane >> a.hp_shift, h = lane & (HP - 1);
  const bool hv = h < a.H;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const float er_h = hv ? a.er[v * a.H + h] : 0.f;

  // scores sweep: per-head max, then the denominator
  float mx = kNegBig;
  if (hv)
    for (int64_t e = e0 + (int64_t)wave_id * EPP + slot; e < e1; e += (int64_t)n_waves * EPP)
      mx = fmaxf(mx, lrelu(a.el[(int64_t)a.indices[e] * a.H + h] + er_h, a.slope));
  mx = reduce_heads<true>(mx, HP, h, wave_id, n_waves, lane, sm);
  float sum = 0.f;
  if (hv)
    for (int64_t e = e0 + (int64_t)wave_id * EPP + slot; e < e1; e += (int64_t)n_waves * EPP)
      sum += __expf(lrelu(a.el[(int64_t)a.indices[e] * a.H + h] + er_h, a.slope) - mx);
  sum = reduce_heads<false>(sum, HP, h, wave_id, n_waves, lane, sm);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  if (a.lse && wave_id == 0 && lane < a.H) a.lse[v * a.H + lane] = sum > 0.f ? mx + logf(sum) : 0.f;

  // value sweep
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.HF;
  const int g = lane / LPR;
  const uint64_t gmask = (LPR == 64 ? ~0ull : ((1ull << LPR) - 1ull)) << (g * LPR);
  int hk[4];
  lane_heads<UNI>(a, col4, hk);
  float mk[NK], ik[NK], ek[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) { mk[k] = __shfl(mx, hk[k]); ik[k] = __shfl(inv, hk[k]); ek[k] = __shfl(er_h, hk[k]); }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? a.indices[base + lane] : 0;
    for (int j = 0; j < cnt; j += G * kU) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ei = j + u * G + g;
        const int src = __shfl(my_idx, ei & 63);
        const bool ok = ei < cnt && col_ok;
        float w[4];
        bool live = false;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          w[k] = 0.f;
          if (ok) {
            w[k] = __expf(lrelu(a.el[(int64_t)src * a.H + hk[k]] + ek[k], a.slope) - mk[k]) * ik[k];
            if (a.thr) w[k] = attn_keep(a.seed, a.thr, (uint32_t)(base + ei), (uint32_t)hk[k]) ? w[k] * a.dscale : 0.f;
            live = live || w[k] != 0.f;
          }
        }
        if (UNI) { w[1] = w[0]; w[2] = w[0]; w[3] = w[0]; }
        const bool any = (__ballot(live) & gmask) != 0ull;      // every head of the edge dropped: its row is not loaded
        if (ok && any) {
          const float4 x = ld4(a.z + (int64_t)src * a.ldz + col4);
          acc.x = fmaf(w[0], x.x, acc.x); acc.y = fmaf(w[1], x.y, acc.y); acc.z = fmaf(w[2], x.z, acc.z); acc.w = fmaf(w[3], x.w, acc.w);
        }
      }
    }
  }
  acc = fold_groups<LPR>(acc);
  if (n_waves > 1) {
    if (lane < LPR) sm.part[wave_id][lane] = acc;
    __syncthreads();
    if (wave_id == 0 && lane < LPR) {
      acc = sm.part[0][lane];
      for (int w = 1; w < n_waves; ++w) acc = add4(acc, sm.part[w][lane]);
    }
  }
  if (wave_id == 0 && lane < LPR && col_ok) {
    float o[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (a.relu) o[k] = fmaxf(o[k], 0.f);
      if (col4 + k >= a.HF) o[k] = 0.f;
    }
    st4(a.out + v * a.ldo + col4, make_float4(o[0], o[1], o[2], o[3]));
  }
  if (n_waves > 1) __syncthreads();
}

// ---------------------------------------------------------------------------------------------- backward, destination side (in-CSR)
// ds_ij = a_ij (c_ij - D_i) with c_ij = w_ij <g_i, z_j> and D_i = <g_i, out_i> = sum_k a_ik c_ik.  On a row whose softmax is close to
// one-hot (scores of +-40 at heads * out_feats = 256) c_ij - D_i cancels to (1 - a_ij) c_ij, so D_i has to be the mean of the SAME c values
// under the SAME weights: two sweeps, the first leaves c_ij in ds and sums a and a c per head in fp64, the second reads c_ij back (each lane
// its own entries) and writes ds.  <g_i, y_i> from the stored output differs from that mean by the forward's rounding (1e-5 of |c|), which
// the sum over a hub's edges in the source pass then multiplies.
template <int LPR, bool UNI>
__device__ __forceinline__ void bwd_dst_row(const GatArgs& a, int64_t v, int wave_id, int n_waves, int lane, Smem& sm) {
  const int HP = 1 << a.hp_shift, EPP = 64 >> a.hp_shift;
  const int slot = lane >> a.hp_shift, h = lane & (HP - 1);
  const bool hv = h < a.H;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int F = a.F;
  const float er_h = hv ? a.er[v * a.H + h] : 0.f, lse_h = hv ? a.lse[v * a.H + h] : 0.f;
  double S = 0.0, P = 0.0;
  if (hv) {
    const float* gp = a.g + v * a.ldg + h * F;
    for (int64_t e = e0 + (int64_t)wave_id * EPP + slot; e < e1; e += (int64_t)n_waves * EPP) {
      const int64_t j = a.indices[e];
      const float at = __expf(lrelu(a.el[j * a.H + h] + er_h, a.slope) - lse_h);
      float c = 0.f;
      if (!a.thr || attn_keep(a.seed, a.thr, (uint32_t)e, (uint32_t)h)) {
        const float* zp = a.z + j * a.ldz + h * F;
        if (UNI) {
          for (int f = 0; f < F; f += 4) {
            const float4 p = ld4(gp + f), q = ld4(zp + f);
            c = fmaf(p.x, q.x, c); c = fmaf(p.y, q.y, c); c = fmaf(p.z, q.z, c); c = fmaf(p.w, q.w, c);
          }
        } else {
          for (int f = 0; f < F; ++f) c = fmaf(gp[f], zp[f], c);
        }
        c *= a.dscale;
      }
      a.ds[e * a.H + h] = c;
      S += (double)at;
      P += (double)at * (double)c;
    }
  }
  S = reduce_heads<false>(S, HP, h, wave_id, n_waves, lane, sm);
  P = reduce_heads<false>(P, HP, h, wave_id, n_waves, lane, sm);
  float der = 0.f;
  if (hv) {
    const double D = S > 0.0 ? P / S : 0.0;
    for (int64_t e = e0 + (int64_t)wave_id * EPP + slot; e < e1; e += (int64_t)n_waves * EPP) {
      const float s = a.el[(int64_t)a.indices[e] * a.H + h] + er_h;
      const float at = __expf(lrelu(s, a.slope) - lse_h);
      const float dsv = at * (float)((double)a.ds[e * a.H + h] - D) * (s > 0.f ? 1.f : a.slope);
      a.ds[e * a.H + h] = dsv;
      der += dsv;
    }
  }
  der = reduce_heads<false>(der, HP, h, wave_id, n_waves, lane, sm);
  if (wave_id == 0 && lane < a.H) a.der[v * a.H + lane] = der;
}

// ---------------------------------------------------------------------------------------------- backward, source side (transposed CSR)
template <int LPR, bool UNI>
__device__ __forceinline__ void bwd_src_row(const GatArgs& a, int64_t v, int wave_id, int n_waves, int lane, Smem& sm) {
  constexpr int G = 64 / LPR;
  constexpr int NK = UNI ? 1 : 4;
  const int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.HF;
  const int g = lane / LPR;
  const uint64_t gmask = (LPR == 64 ? ~0ull : ((1ull << LPR) - 1ull)) << (g * LPR);
  int hk[4];
  lane_heads<UNI>(a, col4, hk);
  float elk[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) elk[k] = a.el[v * a.H + hk[k]];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float dl[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t base = e0 + (int64_t)wave_id * 64; base < e1; base += (int64_t)n_waves * 64) {
    const int64_t rem = e1 - base;
    const int cnt = rem < 64 ? (int)rem : 64;
    const int my_idx = lane < cnt ? a.indices[base + lane] : 0;
    const int my_eid = lane < cnt ? (a.eids ? a.eids[base + lane] : (int)(base + lane)) : 0;
    for (int j = 0; j < cnt; j += G * kU) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ei = j + u * G + g;
        const int64_t dst = __shfl(my_idx, ei & 63);
        const int64_t eid = __shfl(my_eid, ei & 63);
        const bool ok = ei < cnt && col_ok;
        float w[4];
        bool live = false;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          w[k] = 0.f;
          if (ok) {
            const int64_t o = dst * a.H + hk[k];
            w[k] = __expf(lrelu(elk[k] + a.er[o], a.slope) - a.lse[o]);
            if (a.thr) w[k] = attn_keep(a.seed, a.thr, (uint32_t)eid, (uint32_t)hk[k]) ? w[k] * a.dscale : 0.f;
            live = live || w[k] != 0.f;
            dl[k] += a.ds[eid * a.H + hk[k]];
          }
        }
        if (UNI) { w[1] = w[0]; w[2] = w[0]; w[3] = w[0]; }
        const bool any = (__ballot(live) & gmask) != 0ull;
        if (ok && any) {
          const float4 x = ld4(a.g + dst * a.ldg + col4);
          acc.x = fmaf(w[0], x.x, acc.x); acc.y = fmaf(w[1], x.y, acc.y); acc.z = fmaf(w[2], x.z, acc.z); acc.w = fmaf(w[3], x.w, acc.w);
        }
      }
    }
  }
  if (UNI) { dl[1] = dl[0]; dl[2] = dl[0]; dl[3] = dl[0]; }
  float4 d4 = make_float4(dl[0], dl[1], dl[2], dl[3]);
  acc = fold_groups<LPR>(acc);
  d4 = fold_groups<LPR>(d4);
  if (n_waves > 1) {
    if (lane < LPR) { sm.part[wave_id][lane] = acc; sm.part2[wave_id][lane] = d4; }
    __syncthreads();
    if (wave_id == 0 && lane < LPR) {
      acc = sm.part[0][lane]; d4 = sm.part2[0][lane];
      for (int w = 1; w < n_waves; ++w) { acc = add4(acc, sm.part[w][lane]); d4 = add4(d4, sm.part2[w][lane]); }
    }
  }
  if (wave_id == 0 && lane < LPR && col_ok) {
    const float s[4] = {acc.x, acc.y, acc.z, acc.w};
    const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = col4 + k;
      o[k] = 0.f;
      if (c < a.HF) {
        const int hh = c / a.F;
        o[k] = s[k] + dd[k] * a.attn_l[c] + a.der[v * a.H + hh] * a.attn_r[c];
        if (c - hh * a.F == 0) a.del_[v * a.H + hh] = dd[k];
      }
    }
    st4(a.out + v * a.ldo + col4, make_float4(o[0], o[1], o[2], o[3]));
  }
  if (n_waves > 1) __syncthreads();
}

template <int KIND, int LPR, bool UNI>
__device__ __forceinline__ void do_row(const GatArgs& a, int64_t v, int wave_id, int n_waves, int lane, Smem& sm) {
  if (KIND == 0) fwd_row<LPR, UNI>(a, v, wave_id, n_waves, lane, sm);
  else if (KIND == 1) bwd_dst_row<LPR, UNI>(a, v, wave_id, n_waves, lane, sm);
  else bwd_src_row<LPR, UNI>(a, v, wave_id, n_waves, lane, sm);
}

// KIND 0 forward, 1 backward over the in-CSR (ds, der), 2 backward over the transposed CSR (dz, del)
template <int KIND, int LPR, bool UNI>
__global__ __launch_bounds__(kBlock) void gat_rows_kernel(const GatArgs a) {
  __shared__ Smem sm;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // row_gather_dev.h's two roles with the loops WRITTEN OUT, short rows assigned statically.  Behind a callback -- scan_rows', or a
  // scan_rows_static shared with gatv2_rows_kernel, whose loops are these -- the KIND 2 kernels go from 71 / 71 / 77 / 90 VGPRs (LPR 32 /
  // 16 / 8 / 4, UNI) to 107 / 109 / 112 / 120 and from 84 - 102 to 113 - 126 (non-UNI): a wave per SIMD less.  Measured with the build's
  // flags, three forms of the shared function, the same figures each time (row_gather_dev.h, "the two-role scan"): leave them here.
  if ((int)blockIdx.x < a.sg.n_long_blocks) {
    const int64_t n_chunks = (a.n + kBlock - 1) / kBlock;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += a.sg.n_long_blocks) {
      const int64_t* rows;
      const int n_found = find_long_rows(a.indptr, a.n, n_chunks, chunk, &rows);
      for (int i = 0; i < n_found; ++i) {
        do_row<KIND, LPR, UNI>(a, rows[i], wave, kWaves, lane, sm);
        __syncthreads();
      }
    }
    return;
  }
  const int64_t row_base = ((int64_t)blockIdx.x - a.sg.n_long_blocks) * a.sg.rows_per_block;
  for (int lr = wave; lr < a.sg.rows_per_block; lr += kWaves) {
    const int64_t v = row_base + lr;
    if (v >= a.n) break;
    if (a.indptr[v + 1] - a.indptr[v] > kLongRow) continue;
    do_row<KIND, LPR, UNI>(a, v, 0, 1, lane, sm);
  }
}

int set_shape(GatArgs& a, int64_t n, int64_t nnz, int heads, int f, float p, const char* what) {
  GLNN_REQUIRE(n >= 0 && nnz >= 0 && heads >= 1 && f >= 1, "%s: bad size", what);
  GLNN_REQUIRE(nnz < ((int64_t)1 << 31), "%s: nnz >= 2^31 (edge ids are 32-bit)", what);
  GLNN_REQUIRE(heads <= 64 && (int64_t)heads * f <= 256, "%s: needs heads <= 64 and heads * out_feats <= 256", what);
  GLNN_REQUIRE(p >= 0.f && p < 1.f, "%s: attn_drop in [0, 1)", what);
  a.n = n; a.H = heads; a.F = f; a.HF = heads * f;
  a.hp_shift = 0;
  while ((1 << a.hp_shift) < heads) ++a.hp_shift;
  a.thr = glnn::drop_threshold(p);
  a.dscale = 1.f / (1.f - p);
  return GLNN_OK;
}

int rows_launch(GatArgs& a, int kind, const char* what, void* stream) {
  const int rc = scan_grid(a.n, what, &a.sg);
  if (rc != GLNN_OK) return rc;
  with_attn_variant(kind, a.F % 4 == 0, lpr_for((a.HF + 3) / 4, 4), [&](auto K, auto U, auto L) {
    hipLaunchKernelGGL((gat_rows_kernel<decltype(K)::value, decltype(L)::value, decltype(U)::value>), dim3(a.sg.grid_x), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
  });
  return glnn::check_launch(what);
}

// el / er of every row from ONE read of z: lane = (row slot, head), F products each.  z2 != NULL: z -= z2 first, stored back (the two
// half-products of a signed input behind the feature dropout, see ops.gat_project)
__global__ __launch_bounds__(256) void gat_scores_kernel(float* __restrict__ z, int64_t ldz, const float* __restrict__ z2, int64_t ldz2, int64_t n,
                                                         int H, int F, int hp_shift, int vec4, const float* __restrict__ attn_l,
                                                         const float* __restrict__ attn_r, float* __restrict__ el, float* __restrict__ er) {
  const int HP = 1 << hp_shift;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> hp_shift;
  const int h = (int)(t & (HP - 1));
  if (h >= H) return;
  for (int64_t r = t >> hp_shift; r < n; r += stride) {
    float* zp = z + r * ldz + h * F;
    const float* al = attn_l + h * F;
    const float* ar = attn_r + h * F;
    double sl = 0.0, sr = 0.0;                              // fp64 sums: a score of +-40 over 256 columns keeps its last fp32 bits, which
    if (vec4) {                                             // the softmax's exponentials magnify; F % 4 == 0 and aligned rows: 16-byte moves
      for (int f = 0; f < F; f += 4) {
        float4 x = ld4(zp + f);
        if (z2) {
          const float4 y = ld4(z2 + r * ldz2 + h * F + f);
          x = make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w);
          st4(zp + f, x);
        }
        const float4 l4 = ld4(al + f), r4 = ld4(ar + f);
        sl = fma((double)x.x, (double)l4.x, sl); sl = fma((double)x.y, (double)l4.y, sl);
        sl = fma((double)x.z, (double)l4.z, sl); sl = fma((double)x.w, (double)l4.w, sl);
        sr = fma((double)x.x, (double)r4.x, sr); sr = fma((double)x.y, (double)r4.y, sr);
        sr = fma((double)x.z, (double)r4.z, sr); sr = fma((double)x.w, (double)r4.w, sr);
      }
    } else
    for (int f = 0; f < F; ++f) {
      float x = zp[f];
      if (z2) { x -= z2[r * ldz2 + h * F + f]; zp[f] = x; }
      sl = fma((double)x, (double)al[f], sl);
      sr = fma((double)x, (double)ar[f], sr);
    }
    el[r * H + h] = (float)sl;
    er[r * H + h] = (float)sr;
  }
}

// dattn partials: workgroup b sums rows [b rows_per, ..) of del z and der z per column (thread = column), rows ascending
__global__ __launch_bounds__(256) void gat_dattn_part_kernel(const float* __restrict__ z, int64_t ldz, int64_t n, int H, int F, int64_t rows_per,
                                                             const float* __restrict__ del_, const float* __restrict__ der,
                                                             float* __restrict__ part) {
  const int c = threadIdx.x;
  const int HF = H * F;
  if (c >= HF) return;
  const int h = c / F;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per;
  const int64_t r1 = r0 + rows_per < n ? r0 + rows_per : n;
  float pl = 0.f, pr = 0.f;
  for (int64_t r = r0; r < r1; ++r) {
    const float x = z[r * ldz + c];
    pl = fmaf(del_[r * H + h], x, pl);
    pr = fmaf(der[r * H + h], x, pr);
  }
  part[((int64_t)blockIdx.x * 2 + 0) * HF + c] = pl;
  part[((int64_t)blockIdx.x * 2 + 1) * HF + c] = pr;
}

__global__ __launch_bounds__(256) void gat_dattn_fold_kernel(const float* __restrict__ part, int nparts, int HF, float* __restrict__ dl,
                                                             float* __restrict__ dr) {
  const int c = threadIdx.x;
  if (c >= HF) return;
  float sl = 0.f, sr = 0.f;
  for (int p = 0; p < nparts; ++p) {                      // fixed order
    sl += part[((int64_t)p * 2 + 0) * HF + c];
    sr += part[((int64_t)p * 2 + 1) * HF + c];
  }
  dl[c] = sl;
  dr[c] = sr;
}

__global__ __launch_bounds__(256) void gat_mask_kernel(int64_t total, int H, uint32_t thr, uint32_t seed, uint8_t* __restrict__ mask) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
    mask[i] = attn_keep(seed, thr, (uint32_t)(i / H), (uint32_t)(i % H)) ? 1 : 0;
}

int64_t dattn_parts(int64_t n, int64_t* rows_per) {
  int64_t rp = (n + 1023) / 1024;
  if (rp < 256) rp = 256;
  *rows_per = rp;
  return (n + rp - 1) / rp;
}

}  // namespace

extern "C" int glnn_gat_scores_f32(float* z, int64_t ldz, const float* z2, int64_t ldz2, int64_t n, int heads, int out_feats,
                                   const float* attn_l, const float* attn_r, float* el, float* er, void* stream) {
  GatArgs a = {};
  const int rc = set_shape(a, n, 0, heads, out_feats, 0.f, "glnn_gat_scores_f32");
  if (rc != GLNN_OK) return rc;
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(z && attn_l && attn_r && el && er, "glnn_gat_scores_f32: null pointer");
  GLNN_REQUIRE(ldz >= a.HF && (!z2 || ldz2 >= a.HF), "glnn_gat_scores_f32: leading dimension below heads * out_feats");
  int64_t blocks = ((n << a.hp_shift) + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const int vec4 = out_feats % 4 == 0 && glnn::aligned16(z) && ldz % 4 == 0 && (!z2 || (glnn::aligned16(z2) && ldz2 % 4 == 0)) &&
                   glnn::aligned16(attn_l) && glnn::aligned16(attn_r);
  hipLaunchKernelGGL(gat_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z, ldz, z2, ldz2, n, heads,
                     out_feats, a.hp_shift, vec4, attn_l, attn_r, el, er);
  return glnn::check_launch("glnn_gat_scores_f32");
}

extern "C" int glnn_gat_attn_fwd_f32(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, const float* z, int64_t ldz,
                                     int heads, int out_feats, const float* el, const float* er, float negative_slope, float attn_drop,
                                     uint32_t seed, int relu, float* out, int64_t ldo, float* lse, void* stream) {
  GatArgs a = {};
  const int rc = set_shape(a, n, nnz, heads, out_feats, attn_drop, "glnn_gat_attn_fwd_f32");
  if (rc != GLNN_OK) return rc;
  if (n == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && (indices || nnz == 0) && z && el && er && out, "glnn_gat_attn_fwd_f32: null pointer");
  GLNN_REQUIRE(rows_ok(z, ldz, a.HF) && rows_ok(out, ldo, a.HF) && out != z,
               "glnn_gat_attn_fwd_f32: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(heads * out_feats); out != z");
  a.indptr = indptr; a.indices = indices; a.z = z; a.ldz = ldz; a.el = el; a.er = er; a.slope = negative_slope; a.seed = seed;
  a.relu = relu ? 1 : 0; a.out = out; a.ldo = ldo; a.lse = lse;
  return rows_launch(a, 0, "glnn_gat_attn_fwd_f32", stream);
}

extern "C" int64_t glnn_gat_attn_bwd_workspace_floats(int64_t n, int heads, int out_feats) {
  int64_t rows_per;
  return dattn_parts(n < 1 ? 1 : n, &rows_per) * 2 * heads * out_feats;
}

extern "C" int glnn_gat_attn_bwd_f32(const int64_t* indptr, const int32_t* indices, const int64_t* t_indptr, const int32_t* t_indices,
                                     const int32_t* t_eids, int64_t n, int64_t nnz, const float* z, int64_t ldz, int heads, int out_feats,
                                     const float* el, const float* er, const float* lse, const float* attn_l, const float* attn_r,
                                     const float* g, int64_t ldg, const float* y, int64_t ldy, float negative_slope, float attn_drop,
                                     uint32_t seed, float* ds, float* der, float* del_, float* dz, int64_t lddz, float* dattn_l,
                                     float* dattn_r, float* workspace, int64_t workspace_floats, void* stream) {
  GatArgs a = {};
  const int rc = set_shape(a, n, nnz, heads, out_feats, attn_drop, "glnn_gat_attn_bwd_f32");
  if (rc != GLNN_OK) return rc;
  GLNN_REQUIRE(dattn_l && dattn_r, "glnn_gat_attn_bwd_f32: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n == 0) {
    hipLaunchKernelGGL(gat_dattn_fold_kernel, dim3(1), dim3(256), 0, st, workspace, 0, a.HF, dattn_l, dattn_r);
    return glnn::check_launch("glnn_gat_attn_bwd_f32");
  }
  GLNN_REQUIRE(indptr && t_indptr && (nnz == 0 || (indices && t_indices && t_eids && ds)) && z && el && er && lse && attn_l && attn_r && g && y &&
               der && del_ && dz && workspace, "glnn_gat_attn_bwd_f32: null pointer");
  GLNN_REQUIRE(rows_ok(z, ldz, a.HF) && rows_ok(g, ldg, a.HF) && rows_ok(y, ldy, a.HF) && rows_ok(dz, lddz, a.HF) && dz != g && dz != z,
               "glnn_gat_attn_bwd_f32: rows must be 16-byte aligned with a leading dimension %% 4 == 0 and >= round4(heads * out_feats); dz must "
               "not alias g or z");
  GLNN_REQUIRE(workspace_floats >= glnn_gat_attn_bwd_workspace_floats(n, heads, out_feats), "glnn_gat_attn_bwd_f32: workspace too small");
  a.z = z; a.ldz = ldz; a.el = el; a.er = er; a.slope = negative_slope; a.seed = seed; a.lse = const_cast<float*>(lse);
  a.g = g; a.ldg = ldg; a.y = y; a.ldy = ldy; a.ds = ds; a.der = der; a.del_ = del_; a.attn_l = attn_l; a.attn_r = attn_r;
  a.indptr = indptr; a.indices = indices; a.eids = nullptr;
  int r = rows_launch(a, 1, "glnn_gat_attn_bwd_f32", stream);
  if (r != GLNN_OK) return r;
  a.indptr = t_indptr; a.indices = t_indices; a.eids = t_eids; a.out = dz; a.ldo = lddz;
  r = rows_launch(a, 2, "glnn_gat_attn_bwd_f32", stream);
  if (r != GLNN_OK) return r;
  int64_t rows_per;
  const int64_t nparts = dattn_parts(n, &rows_per);
  hipLaunchKernelGGL(gat_dattn_part_kernel, dim3((unsigned)nparts), dim3(256), 0, st, z, ldz, n, heads, out_feats, rows_per, del_, der, workspace);
  hipLaunchKernelGGL(gat_dattn_fold_kernel, dim3(1), dim3(256), 0, st, workspace, (int)nparts, a.HF, dattn_l, dattn_r);
  return glnn::check_launch("glnn_gat_attn_bwd_f32");
}

extern "C" int glnn_gat_attn_mask_u8(int64_t nnz, int heads, float attn_drop, uint32_t seed, uint8_t* mask, void* stream) {
  GLNN_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31) && heads >= 1 && attn_drop >= 0.f && attn_drop < 1.f && (mask || nnz == 0),
               "glnn_gat_attn_mask_u8: bad arguments");
  if (nnz == 0) return GLNN_OK;
  int64_t blocks = (nnz * heads + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gat_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), nnz * heads, heads,
                     glnn::drop_threshold(attn_drop), seed, mask);
  return glnn::check_launch("glnn_gat_attn_mask_u8");
}
