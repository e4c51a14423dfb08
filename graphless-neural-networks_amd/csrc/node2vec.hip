// node2vec's second-order (p, q) walks (Grover, Leskovec, KDD 2016) for the position features (docs/POSITION_SEMANTICS.md): the walk of
// glnn_random_walk with the step biased by where the walk came from.  Standing on v, having come from t = walk[s - 2], a candidate x of
// row v is a RETURN (x == t, weight 1/p; tested first), NEAR (x appears in row t, weight 1) or FAR (weight 1/q).  Sampling is rejection
// sampling in integers, so that tests/node2vec_oracle.py reproduces it bit for bit: attempt a of step s of walk i draws the candidate with
// drop_hash(seed, i, s + 128 a) -- attempt 0 is glnn_random_walk's own draw -- and accepts it iff
// drop_hash(seed ^ 0x4E32564B, i, s + 128 a) < T_class, T_class = min(2^32, floor(w_class / wmax * 2^32)) formed in double on the host.
// After 256 rejected attempts the 256th candidate is taken.
//
// Rows are not sorted by source, so "x appears in row t" is a scan.  One WAVE per walk, as the induced-subgraph builder walks its rows
// (csrc/subgraph.hip): the walk's state is wave-uniform (held in scalar registers through readfirstlane), the lanes stride row t 256
// entries a round (four independent loads per lane) and an any-lane ballot answers; a 17 k-entry hub row is 69 rounds of the whole wave,
// not 17 k loads of one lane, and the attempt loop has no per-lane divergence.  The scan runs only where it can change the outcome: the
// acceptance draw h is compared with both thresholds first, and a candidate with h below the smaller or at or above the larger of T_near,
// T_far needs no class.
// Plain C++: no inline assembly, no LDS, no atomics.
#include <cmath>

#include "glnn_common.h"

namespace {

constexpr uint32_t kN2vAcceptXor = 0x4E32564Bu;      // the acceptance draw's seed is the walk seed xor this
constexpr int kN2vAttemptStride = 128;               // attempt a of step s draws at column s + 128 a (s <= 64: no two attempts share one)
constexpr int kN2vMaxAttempts = 256;                 // the last of them is taken whatever its acceptance draw says
constexpr int kN2vScanLoads = 4;                     // entries of row t each lane has in flight per round of the scan (256 per wave and round)
constexpr uint64_t kN2vAlways = (uint64_t)1 << 32;   // a threshold no 32-bit draw reaches: always accepted, no draw made

struct N2vArgs {
  const int64_t* indptr; const int32_t* indices; const int64_t* roots; int64_t n_roots; int length; uint32_t seed;
  uint64_t t_ret, t_near, t_far;
  int64_t* out;
};

// Latency-bound and load-dependent (every step waits for indptr[v], then for the candidate): no occupancy is asked of the register
// allocator beyond the block size; the kernel needs few registers and hides latency with waves, of which there is one per walk.
__global__ __launch_bounds__(256) void node2vec_walk_kernel(const N2vArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);         // (wave-uniform)
  if (i >= a.n_roots) return;
  const uint64_t t_lo = a.t_near < a.t_far ? a.t_near : a.t_far, t_hi = a.t_near < a.t_far ? a.t_far : a.t_near;
  const bool unbiased = a.t_ret == kN2vAlways && t_lo == kN2vAlways;       // p = q = 1: glnn_random_walk's step everywhere
  const uint32_t acc_seed = a.seed ^ kN2vAcceptXor;
  int v = __builtin_amdgcn_readfirstlane((int)a.roots[i]);                // (node ids are int32: `indices` is)
  int t = v;
  int64_t* row = a.out + i * (int64_t)(a.length + 1);
  if (lane == 0) row[0] = v;
  for (int s = 1; s <= a.length; ++s) {
    const int64_t e0 = a.indptr[v];
    const int64_t deg = a.indptr[v + 1] - e0;
    int nxt = v;                                                          // (deg == 0: the walk stays where it is)
    if (deg > 0) {
      if (s == 1 || unbiased) {
        const uint32_t r = glnn::drop_hash(a.seed, (uint32_t)i, (uint32_t)s);
        nxt = a.indices[e0 + (int64_t)(((uint64_t)r * (uint64_t)deg) >> 32)];
      } else {
        const int64_t t0 = a.indptr[t];
        const int64_t tdeg = a.indptr[t + 1] - t0;
        for (int att = 0; att < kN2vMaxAttempts; ++att) {
          const uint32_t col = (uint32_t)(s + kN2vAttemptStride * att);
          const uint32_t r = glnn::drop_hash(a.seed, (uint32_t)i, col);
          const int x = __builtin_amdgcn_readfirstlane(a.indices[e0 + (int64_t)(((uint64_t)r * (uint64_t)deg) >> 32)]);
          nxt = x;
          if (att == kN2vMaxAttempts - 1) break;                          // the cap: the 256th candidate is taken
          const uint64_t h = glnn::drop_hash(acc_seed, (uint32_t)i, col);
          bool accept;
          if (x == t) {
            accept = h < a.t_ret;
          } else if (h < t_lo) {
            accept = true;                                                // below both thresholds: near or far, accepted
          } else if (h >= t_hi) {
            accept = false;                                               // at or above both: near or far, rejected
          } else {
            bool near = false;                                            // x in row t?  lanes stride the row, any lane answers
            for (int64_t j0 = 0; j0 < tdeg; j0 += 64 * kN2vScanLoads) {   // (tdeg is uniform across the wave: every lane takes every round)
              bool hit = false;
#pragma unroll
              for (int u = 0; u < kN2vScanLoads; ++u) {                   // independent loads in flight per lane: a round waits for memory once
                const int64_t j = j0 + u * 64 + lane;
                const bool in = j < tdeg;
                const int y = in ? a.indices[t0 + j] : 0;
                hit |= in && y == x;
              }
              if (__ballot(hit) != 0ull) { near = true; break; }
            }
            accept = h < (near ? a.t_near : a.t_far);
          }
          if (accept) break;
        }
      }
    }
    t = v;
    v = __builtin_amdgcn_readfirstlane(nxt);
    if (lane == 0) row[s] = v;
  }
}

// T_c = min(2^32, floor(w_c / wmax * 2^32)) in double: w_c == wmax gives exactly 2^32
uint64_t n2v_threshold(double w, double wmax) {
  const double t = std::floor(w / wmax * 4294967296.0);
  return t >= 4294967296.0 ? kN2vAlways : (uint64_t)t;
}

}  // namespace

extern "C" int glnn_node2vec_walk(const int64_t* indptr, const int32_t* indices, int64_t n_nodes, const int64_t* roots,
                                  const int64_t* roots_host, int64_t n_roots, int length, double p, double q, uint32_t rng_seed,
                                  int64_t* out, void* stream) {
  const char* what = "glnn_node2vec_walk";
  GLNN_REQUIRE(length >= 1 && length <= 64, "%s: walk length must be in [1, 64] (got %d)", what, length);
  GLNN_REQUIRE(p >= 0.25 && p <= 4.0 && q >= 0.25 && q <= 4.0, "%s: p and q must be in [0.25, 4] (got p = %g, q = %g)", what, p, q);
  GLNN_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "%s: the graph must have 1 <= N < 2^31 nodes (got %lld)", what, (long long)n_nodes);
  GLNN_REQUIRE(n_roots >= 0 && n_roots < ((int64_t)1 << 32), "%s: the walk index is a 32-bit counter of the draw", what);
  if (n_roots == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && indices && roots && out, "%s: null pointer", what);
  if (roots_host)                                             // (NULL: the caller vouches for the roots, as with glnn_random_walk)
    for (int64_t i = 0; i < n_roots; ++i)
      GLNN_REQUIRE(roots_host[i] >= 0 && roots_host[i] < n_nodes, "%s: root %lld (position %lld) is outside the graph of %lld nodes", what,
                   (long long)roots_host[i], (long long)i, (long long)n_nodes);
  const double w_ret = 1.0 / p, w_far = 1.0 / q;
  const double wmax = std::fmax(std::fmax(w_ret, 1.0), w_far);
  N2vArgs a;
  a.indptr = indptr; a.indices = indices; a.roots = roots; a.n_roots = n_roots; a.length = length; a.seed = rng_seed;
  a.t_ret = n2v_threshold(w_ret, wmax); a.t_near = n2v_threshold(1.0, wmax); a.t_far = n2v_threshold(w_far, wmax);
  a.out = out;
  hipLaunchKernelGGL(node2vec_walk_kernel, dim3((unsigned)((n_roots + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return glnn::check_launch(what);
}
