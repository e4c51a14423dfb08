// Serving a position-feature student by node id (docs/POSITION_SEMANTICS.md, "Serving by node id"): glnn_position_rows assembles the
// student's input rows [x[v] | pos(v) | 0-padding] for a batch of node ids straight from the features, the position table and the graph.
// pos(v) is the table row z[slot[v]] of an embedded node and, for a node the table never saw, the mean of the table rows of its embedded
// in-neighbours -- position.fill_unseen's definition restricted to the rows asked for; nothing of size N is built.
//
// One launch, one wave per batch row, the two roles of row_gather_dev.h's scan_rows written out over `ids` (scan_rows itself walks the CSR
// rows of its launch; here a row of the launch is ids[b], and only an UNSEEN id has a CSR row to sum):
//   the long role   the first n_long_blocks workgroups search the batch (one position per thread, as find_long_rows does) for unseen ids
//                   of more than kLongRow entries; each is taken by all eight waves, the partials added in wave order
//                   (sum_waves_in_order), the embedded-entry counts added beside them as integers; the feature copy of such a row is
//                   spread over the 512 threads;
//   the short role  every other workgroup owns eight consecutive batch positions, one per wave, and skips the long ones.
// Which role takes a row depends on the row's own entry count only, and every sum has a fixed order (wave_row_sum; no float atomics): a
// row's bits depend neither on its position in the batch nor on the other ids of the call.
//
// The neighbour sum is wave_row_sum<LPR> with a policy (SlotRows) whose per-entry weight CARRIES slot[u]: the lane that holds the index
// loads the slot (an entry outside [0, n_nodes) or a slot outside [0, z_rows) becomes -1), its bits ride along as NormRows<true>'s weight
// does, and row() returns zeros without a load for a negative slot.  The count of embedded entries is the popcount of a ballot over the
// same lanes, once per 64-entry chunk.
//
// The output row.  A row of `out` starts 16-byte aligned (ldo % 4 == 0 for fp32, % 8 for bf16) and is written as 16-byte pieces of
// E = 4 (fp32) or 8 (bf16) elements.  The f / E whole pieces of the feature part are a coalesced copy, 16 bytes per lane: from 16-byte
// loads where the source rows allow them (bf16 always: ldx % 8 == 0 and an aligned x are required; fp32: x 16-byte aligned and
// ldx % 4 == 0 -- the raw [N, 1433] features of the CLIs are not), else from element loads;
// fp32 -> bf16 rounds as glnn_cast_f32_bf16 does, equal dtypes copy the bits.  The position part starts at column f, which in general is
// not even 4-byte aligned (bf16, odd f): the tail of the row -- the f % E last feature elements, the d position elements and the zero
// padding up to the next multiple of E -- is STAGED in LDS in the output's element type (one slice per wave, at most 264 words) and
// written out as aligned 16-byte pieces behind a barrier.  No store assumes more than the row's own alignment.
#include "bf16_mfma_dev.h"      // f32_to_bf16_bits, pack2: the bits of glnn_cast_f32_bf16
#include "row_gather_dev.h"

namespace {

constexpr int kPosMaxD = 256;
constexpr int kTailWords = 264;        // fp32: round4(3 + 256) = 260 words; bf16: round8(7 + 256) = 264 elements = 132 words

struct PosArgs {
  const int64_t* ids; int64_t m;
  const void* x; int64_t ldx; int x_bf16; int x_vec; int f;       // x_vec: the rows of an fp32 x take 16-byte loads
  const float* z; int64_t ldz; int d; int64_t z_rows;
  const int32_t* slot; int64_t n_nodes;
  const int64_t* indptr; const int32_t* indices;
  void* out; int64_t ldo;
  int n_long_blocks;
};

// z[slot[u]] of the entries u of a CSR row; the weight of an entry is its slot, -1 for "not embedded"
struct SlotRows : GatherPolicy {
  static constexpr bool kWeighted = true;
  const float* z; int64_t ldz; int64_t z_rows; const int32_t* slot; int64_t n_nodes; int col4; bool col_ok;
  int* count;                     // embedded entries seen so far (wave-uniform; weight() is called by the whole wave, once per chunk)
  __device__ __forceinline__ float weight(int idx, bool in_range) const {
    int s = -1;
    if (in_range && (unsigned)idx < (unsigned)n_nodes) {
      s = slot[idx];
      if ((unsigned)s >= (unsigned)z_rows) s = -1;
    }
    *count += __popcll(__ballot(s >= 0));
    return __builtin_bit_cast(float, s);
  }
  __device__ __forceinline__ float4 row(int, float w, bool ok) const {
    const int s = __builtin_bit_cast(int, w);
    return (ok && col_ok && s >= 0) ? ld4(z + (int64_t)s * ldz + col4) : zero4();
  }
};

// the slot of node v, -1 for "not embedded" (v in [0, n_nodes))
__device__ __forceinline__ int slot_of(const PosArgs& a, int64_t v) {
  const int s = a.slot[v];
  return (unsigned)s < (unsigned)a.z_rows ? s : -1;
}

// an unseen id whose CSR row has more than kLongRow entries: the long role's
__device__ __forceinline__ bool is_long(const PosArgs& a, int64_t v) {
  if (a.indptr == nullptr || v < 0 || v >= a.n_nodes || slot_of(a, v) >= 0) return false;
  return a.indptr[v + 1] - a.indptr[v] > kLongRow;
}

template <bool OBF>
__device__ __forceinline__ void put_elem(uint32_t* s, int i, uint32_t bits) {
  if constexpr (OBF) reinterpret_cast<uint16_t*>(s)[i] = (uint16_t)bits;
  else s[i] = bits;
}

// element j of row v of x in the output's element type: the same bits for equal dtypes, rounded for fp32 -> bf16
template <bool OBF>
__device__ __forceinline__ uint32_t x_elem(const PosArgs& a, int64_t v, int j) {
  if (a.x_bf16) return static_cast<const uint16_t*>(a.x)[v * a.ldx + j];                 // (OBF only: the entry refuses bf16 -> fp32)
  const uint32_t u = static_cast<const uint32_t*>(a.x)[v * a.ldx + j];
  if constexpr (OBF) return f32_to_bf16_bits(__uint_as_float(u));
  else return u;
}

// the whole 16-byte pieces p0, p0 + stride, ... of the feature part of batch row b (node v; !v_ok: zeros)
template <bool OBF>
__device__ __forceinline__ void copy_features(const PosArgs& a, int64_t b, int64_t v, bool v_ok, int p0, int stride) {
  constexpr int E = OBF ? 8 : 4;
  const int nfull = a.f / E;
  uint4* orow = reinterpret_cast<uint4*>(static_cast<char*>(a.out) + b * a.ldo * (OBF ? 2 : 4));
  for (int p = p0; p < nfull; p += stride) {
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (v_ok) {
      if constexpr (!OBF) {
        const uint32_t* src = static_cast<const uint32_t*>(a.x) + v * a.ldx + p * 4;
        q = a.x_vec ? *reinterpret_cast<const uint4*>(src) : make_uint4(src[0], src[1], src[2], src[3]);
      } else if (a.x_bf16) {
        q = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.x) + v * a.ldx + p * 8);      // (bf16 rows are always 16-byte rows)
      } else {
        const float* src = static_cast<const float*>(a.x) + v * a.ldx + p * 8;
        float e[8];
        if (a.x_vec) {
          const float4 lo = ld4(src), hi = ld4(src + 4);
          e[0] = lo.x; e[1] = lo.y; e[2] = lo.z; e[3] = lo.w; e[4] = hi.x; e[5] = hi.y; e[6] = hi.z; e[7] = hi.w;
        } else {
#pragma unroll
          for (int t = 0; t < 8; ++t) e[t] = src[t];
        }
        q = make_uint4(pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7]));
      }
    }
    orow[p] = q;
  }
}

// one wave: the tail of the row into its LDS slice -- the f % E last feature elements, pos (in the lanes < LPR), the zero padding
template <int LPR, bool OBF>
__device__ __forceinline__ void stage_tail(const PosArgs& a, int64_t v, bool v_ok, float4 pos, int lane, uint32_t* s) {
  constexpr int E = OBF ? 8 : 4;
  const int tail0 = a.f / E * E, ft = a.f - tail0;
  const int col4 = (lane % LPR) * 4;
  if (lane < ft) put_elem<OBF>(s, lane, v_ok ? x_elem<OBF>(a, v, tail0 + lane) : 0u);
  if (lane < LPR && col4 < a.d) {
    const float pv[4] = {pos.x, pos.y, pos.z, pos.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) put_elem<OBF>(s, ft + col4 + t, OBF ? f32_to_bf16_bits(pv[t]) : __float_as_uint(pv[t]));
  }
  const int end = ft + a.d, npad = (end + E - 1) / E * E - end;
  if (lane < npad) put_elem<OBF>(s, end + lane, 0u);
}

// one wave, behind a barrier: the staged tail to the row of `out` as aligned 16-byte pieces
template <bool OBF>
__device__ __forceinline__ void write_tail(const PosArgs& a, int64_t b, int lane, const uint32_t* s) {
  constexpr int E = OBF ? 8 : 4;
  const int nfull = a.f / E, ft = a.f - nfull * E;
  const int npieces = (ft + a.d + E - 1) / E;
  uint4* orow = reinterpret_cast<uint4*>(static_cast<char*>(a.out) + b * a.ldo * (OBF ? 2 : 4)) + nfull;
  for (int p = lane; p < npieces; p += 64) orow[p] = reinterpret_cast<const uint4*>(s)[p];
}

template <int LPR, bool OBF>
__global__ __launch_bounds__(kBlock) void position_rows_kernel(const PosArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tail[kWaves][kTailWords];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col4 = (lane % LPR) * 4;
  const bool col_ok = col4 < a.d;
  int count = 0;
  SlotRows sr;
  sr.z = a.z; sr.ldz = a.ldz; sr.z_rows = a.z_rows; sr.slot = a.slot; sr.n_nodes = a.n_nodes; sr.col4 = col4; sr.col_ok = col_ok;
  sr.count = &count;

  if ((int)blockIdx.x < a.n_long_blocks) {                              // ---- the long role: every long unseen row of the batch
    __shared__ int64_t s_rows[kBlock];
    __shared__ int s_found;
    __shared__ int s_cnt[kWaves];
    const int64_t n_chunks = (a.m + kBlock - 1) / kBlock;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += a.n_long_blocks) {
      if (threadIdx.x == 0) s_found = 0;
      __syncthreads();
      const int64_t mine = (int64_t)threadIdx.x * n_chunks + chunk;     // (find_long_rows' dealing, over batch positions)
      if (mine < a.m && is_long(a, a.ids[mine])) s_rows[atomicAdd(&s_found, 1)] = mine;
      __syncthreads();
      const int n_found = s_found;
      for (int i = 0; i < n_found; ++i) {
        const int64_t b = s_rows[i], v = a.ids[b];
        count = 0;
        const float4 part = wave_row_sum<LPR>(a.indices, a.indptr[v], a.indptr[v + 1], wave, kWaves, lane, sr);
        if (lane == 0) s_cnt[wave] = count;
        float4 pos = sum_waves_in_order<LPR>(part, wave, lane);         // (behind its barrier: s_cnt is visible too)
        if (wave == 0) {
          int c = 0;
#pragma unroll
          for (int w = 0; w < kWaves; ++w) c += s_cnt[w];
          const float fc = (float)c;
          pos = c > 0 ? make_float4(pos.x / fc, pos.y / fc, pos.z / fc, pos.w / fc) : zero4();
          stage_tail<LPR, OBF>(a, v, true, pos, lane, s_tail[0]);
        }
        copy_features<OBF>(a, b, v, true, threadIdx.x, kBlock);
        __syncthreads();
        if (wave == 0) write_tail<OBF>(a, b, lane, s_tail[0]);
        __syncthreads();                                                // (s_tail, s_cnt and the partial slots are free again)
      }
    }
    return;
  }

  // ---- the short role: batch position b is this wave's
  const int64_t b = ((int64_t)blockIdx.x - a.n_long_blocks) * kWaves + wave;
  bool mine = b < a.m;
  int64_t v = 0;
  bool v_ok = false;
  if (mine) {
    v = a.ids[b];
    v_ok = v >= 0 && v < a.n_nodes;                                     // (the callers check the ids; one outside the graph is never an index)
    if (v_ok && is_long(a, v)) mine = false;
  }
  if (mine) {
    float4 pos = zero4();
    const int s = v_ok ? slot_of(a, v) : -1;
    if (s >= 0) {
      if (lane < LPR && col_ok) pos = ld4(a.z + (int64_t)s * a.ldz + col4);
    } else if (v_ok && a.indptr != nullptr) {
      pos = wave_row_sum<LPR>(a.indices, a.indptr[v], a.indptr[v + 1], 0, 1, lane, sr);
      const float fc = (float)count;
      pos = count > 0 ? make_float4(pos.x / fc, pos.y / fc, pos.z / fc, pos.w / fc) : zero4();
    }
    stage_tail<LPR, OBF>(a, v, v_ok, pos, lane, s_tail[wave]);
    copy_features<OBF>(a, b, v, v_ok, lane, 64);
  }
  __syncthreads();
  if (mine) write_tail<OBF>(a, b, lane, s_tail[wave]);
}

}  // namespace

extern "C" int glnn_position_rows(const int64_t* ids, int64_t m, const void* x, int64_t ldx, int x_dtype, int f, const float* z, int64_t ldz,
                                  int d, int64_t z_rows, const int32_t* slot, int64_t n_nodes, const int64_t* indptr, const int32_t* indices,
                                  void* out, int64_t ldo, int out_dtype, void* stream) {
  const char* what = "glnn_position_rows";
  GLNN_REQUIRE(x_dtype == GLNN_DTYPE_F32 || x_dtype == GLNN_DTYPE_BF16, "%s: unknown x_dtype %d", what, x_dtype);
  GLNN_REQUIRE(out_dtype == GLNN_DTYPE_F32 || out_dtype == GLNN_DTYPE_BF16, "%s: unknown out_dtype %d", what, out_dtype);
  if (x_dtype == GLNN_DTYPE_BF16 && out_dtype == GLNN_DTYPE_F32)
    return glnn::fail(GLNN_ERR_UNSUPPORTED, "%s: bf16 features (x_dtype) with an fp32 output (out_dtype) are not implemented", what);
  GLNN_REQUIRE(m >= 0, "%s: m must be >= 0 (got %lld)", what, (long long)m);
  GLNN_REQUIRE(f >= 1, "%s: f must be >= 1 (got %d)", what, f);
  GLNN_REQUIRE(d >= 4 && d % 4 == 0 && d <= kPosMaxD, "%s: d must be a multiple of 4 in [4, %d] (got %d)", what, kPosMaxD, d);
  GLNN_REQUIRE(ldz >= d && ldz % 4 == 0, "%s: ldz must be a multiple of 4 and >= d (got %lld)", what, (long long)ldz);
  const bool obf = out_dtype == GLNN_DTYPE_BF16;
  const int E = obf ? 8 : 4;
  const int64_t need = ((int64_t)f + d + E - 1) / E * E;
  GLNN_REQUIRE(ldo >= need && ldo % E == 0, "%s: ldo must be a multiple of %d and >= f + d rounded up to it, %lld (got %lld)", what, E,
               (long long)need, (long long)ldo);
  GLNN_REQUIRE(ldx >= f, "%s: ldx must be >= f (got %lld)", what, (long long)ldx);
  GLNN_REQUIRE(x_dtype != GLNN_DTYPE_BF16 || ldx % 8 == 0, "%s: bf16 ldx must be a multiple of 8 (got %lld)", what, (long long)ldx);
  GLNN_REQUIRE((indptr == nullptr) == (indices == nullptr), "%s: indptr and indices must both be given or both be NULL", what);
  GLNN_REQUIRE(n_nodes >= 0 && n_nodes < ((int64_t)1 << 31), "%s: n_nodes must be in [0, 2^31) (got %lld)", what, (long long)n_nodes);
  GLNN_REQUIRE(z_rows >= 0 && z_rows < ((int64_t)1 << 31), "%s: z_rows must be in [0, 2^31) (got %lld)", what, (long long)z_rows);
  if (m == 0) return GLNN_OK;
  GLNN_REQUIRE(ids && x && z && slot && out, "%s: null pointer (ids, x, z, slot, out)", what);
  GLNN_REQUIRE(glnn::aligned16(z) && glnn::aligned16(out) && (x_dtype != GLNN_DTYPE_BF16 || glnn::aligned16(x)),
               "%s: z, out and a bf16 x must be 16-byte aligned", what);
  PosArgs a;
  a.ids = ids; a.m = m; a.x = x; a.ldx = ldx; a.x_bf16 = x_dtype == GLNN_DTYPE_BF16; a.f = f;
  a.x_vec = glnn::aligned16(x) && ldx % 4 == 0;
  a.z = z; a.ldz = ldz; a.d = d; a.z_rows = z_rows; a.slot = slot; a.n_nodes = n_nodes; a.indptr = indptr; a.indices = indices;
  a.out = out; a.ldo = ldo;
  int64_t n_long = indptr ? (m + kLongBlockRows - 1) / kLongBlockRows : 0;
  if (n_long > kLongBlockCap) n_long = kLongBlockCap;
  a.n_long_blocks = (int)n_long;
  const int64_t blocks = n_long + (m + kWaves - 1) / kWaves;
  GLNN_REQUIRE(blocks < ((int64_t)1 << 31), "%s: m too large for one launch", what);
  const dim3 grid((unsigned)blocks);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_lpr<1>(lpr_for(d / 4, 1), [&](auto L) {
    if (obf) hipLaunchKernelGGL((position_rows_kernel<decltype(L)::value, true>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((position_rows_kernel<decltype(L)::value, false>), grid, dim3(kBlock), 0, st, a);
  });
  return glnn::check_launch(what);
}
