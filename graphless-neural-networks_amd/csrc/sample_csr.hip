// The sampled neighbourhood of EVERY destination row of a resident CSR as a CSR of its own (docs/SAMPLED_INFERENCE_SEMANTICS.md): what
// SAGE.inference(fan_out=...) aggregates over -- the "Neighbour Sample" teacher baseline of the GLNN paper's inference comparison.
//   glnn_sample_csr_indptr   out_indptr = exclusive prefix sum of min(deg(v), fanout): the graph and the fan-out only, never the seed
//                            (frontier_dev.h's single-pass scan: integer work, the same bits on every run);
//   glnn_sample_csr_fill     out_indices: row v = what glnn_sample_neighbors (csrc/sample.hip) gives seed-list position i = v of
//                            seeds = arange(n_dst) -- the same Floyd picks from the same counter-based draw, keyed by the global row id.
// The fill is NOT one thread per row: a group of F lanes (F = 8 / 16 / 32 / 64 by the fan-out: 8 / 4 / 2 / 1 rows per wave) owns a row and
// lane s owns slot s -- it makes its own draw and stores its own index, so a row's stores are contiguous.  Floyd's duplicate rule is
// sequential in s; it is resolved by `fanout` steps that broadcast slot s's draw within the group and compare it with the RESOLVED picks of
// the lower slots.  j_s = deg - fanout + s exceeds every earlier pick (each is <= j_q, q < s), so a redirected pick needs no second check.
// No scratch arrays, no atomics, no LDS.
#include "glnn_common.h"
#include "frontier_dev.h"

namespace {

struct SampledRowCount {
  const int64_t* indptr; int fanout;
  __device__ int operator()(int64_t i) const {
    const int64_t deg = indptr[i + 1] - indptr[i];
    return deg < (int64_t)fanout ? (int)deg : fanout;
  }
};
struct WriteSampledIndptr {
  int64_t* out; int64_t n;
  __device__ void operator()(int64_t i, long long ex, int v) const {
    out[i] = ex;
    if (i == n - 1) out[n] = ex + v;
  }
};

template <int F>
__global__ __launch_bounds__(256) void sample_csr_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                              const int64_t* __restrict__ out_indptr, int64_t n_dst, int fanout,
                                                              uint32_t seed, int32_t* __restrict__ out_indices) {
  constexpr int kRows = 256 / F;                      // rows per workgroup
  const int s = (int)(threadIdx.x % F);               // the slot this lane owns
  const int64_t v = (int64_t)blockIdx.x * kRows + (int64_t)(threadIdx.x / F);
  if (v >= n_dst) return;                             // (a whole lane group leaves together: every branch below is uniform per group)
  const int64_t e0 = indptr[v];
  const int64_t deg = indptr[v + 1] - e0;
  int32_t* dst = out_indices + out_indptr[v];
  if (deg <= (int64_t)fanout) {                       // short row: copied in row order
    if ((int64_t)s < deg) dst[s] = indices[e0 + s];
    return;
  }
  // Floyd: slot s draws t in [0, j], j = deg - fanout + s, and takes j instead when t was picked by a lower slot
  const int64_t j = deg - (int64_t)fanout + s;
  const uint32_t r = glnn::drop_hash(seed, (uint32_t)v, (uint32_t)s);
  const long long t = (long long)(((uint64_t)r * (uint64_t)(j + 1)) >> 32);       // (lanes s >= fanout: never stored, never compared)
  long long pick = t;
  const int lane = (int)(threadIdx.x & 63);
  const unsigned long long group = (F == 64 ? ~0ull : ((1ull << (F & 63)) - 1ull)) << (lane & ~(F - 1));
  for (int q = 1; q < fanout; ++q) {                  // (slot 0 has no lower slot; `fanout` is uniform: the groups of a wave stay in step)
    const long long tq = __shfl(t, q, F);             // slot q's draw, broadcast within the group
    const bool hit = s < q && pick == tq;             // ... against the resolved picks of slots 0 .. q-1
    const unsigned long long hits = __ballot(hit) & group;
    if (s == q && hits) pick = j;
  }
  if (s < fanout) dst[s] = indices[e0 + pick];
}

}  // namespace

extern "C" int64_t glnn_sample_csr_workspace_bytes(int64_t n_dst) {
  if (n_dst < 0) return 0;
  return ((n_dst + kScanTile - 1) / kScanTile + 1) * 8;          // the scan's status words + its ticket (kept 8-byte aligned)
}

extern "C" int glnn_sample_csr_indptr(const int64_t* indptr, int64_t n_dst, int fanout, int64_t* out_indptr, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  GLNN_REQUIRE(fanout >= 1 && fanout <= 64, "glnn_sample_csr_indptr: fanout must be in [1,64] (got %d)", fanout);
  GLNN_REQUIRE(n_dst >= 0 && n_dst < (1ll << 31), "glnn_sample_csr_indptr: n_dst must be in [0, 2^31) (got %lld)", (long long)n_dst);
  GLNN_REQUIRE(indptr && out_indptr, "glnn_sample_csr_indptr: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_dst == 0) {
    if (hipMemsetAsync(out_indptr, 0, sizeof(int64_t), st) != hipSuccess) return glnn::fail(GLNN_ERR_HIP, "glnn_sample_csr_indptr: memset failed");
    return GLNN_OK;
  }
  GLNN_REQUIRE(workspace, "glnn_sample_csr_indptr: null pointer (workspace)");
  GLNN_REQUIRE(workspace_bytes >= glnn_sample_csr_workspace_bytes(n_dst) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "glnn_sample_csr_indptr: workspace needs %lld bytes, 8-byte aligned", (long long)glnn_sample_csr_workspace_bytes(n_dst));
  const int64_t blocks = (n_dst + kScanTile - 1) / kScanTile;
  unsigned long long* status = reinterpret_cast<unsigned long long*>(workspace);
  int* ticket = reinterpret_cast<int*>(status + blocks);
  GLNN_TRY(fill7f(workspace, (size_t)((blocks + 1) * 8), st, "glnn_sample_csr_indptr(fill)"));
  return launch_scan(SampledRowCount{indptr, fanout}, n_dst, status, ticket, WriteSampledIndptr{out_indptr, n_dst}, nullptr, st,
                     "glnn_sample_csr_indptr(scan)");
}

extern "C" int glnn_sample_csr_fill(const int64_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, const int64_t* out_indptr,
                                    int fanout, uint32_t rng_seed, int32_t* out_indices, void* stream) {
  GLNN_REQUIRE(fanout >= 1 && fanout <= 64, "glnn_sample_csr_fill: fanout must be in [1,64] (got %d)", fanout);
  GLNN_REQUIRE(n_dst >= 0 && n_dst < (1ll << 31) && n_src >= 0 && n_src < (1ll << 31),
               "glnn_sample_csr_fill: n_dst and n_src must be in [0, 2^31) (got %lld, %lld)", (long long)n_dst, (long long)n_src);
  if (n_dst == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && indices && out_indptr && out_indices, "glnn_sample_csr_fill: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define GLNN_SAMPLE_CSR(F_)                                                                                                              \
  hipLaunchKernelGGL((sample_csr_fill_kernel<F_>), dim3((unsigned)((n_dst + (256 / F_) - 1) / (256 / F_))), dim3(256), 0, st, indptr, \
                     indices, out_indptr, n_dst, fanout, rng_seed, out_indices)
  if (fanout <= 8) GLNN_SAMPLE_CSR(8);
  else if (fanout <= 16) GLNN_SAMPLE_CSR(16);
  else if (fanout <= 32) GLNN_SAMPLE_CSR(32);
  else GLNN_SAMPLE_CSR(64);
#undef GLNN_SAMPLE_CSR
  return glnn::check_launch("glnn_sample_csr_fill");
}
