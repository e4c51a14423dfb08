// Frontier-sized index building blocks shared by csrc/blocks.hip (block builder, CSR transpose) and csrc/subgraph.hip (induced subgraphs):
//   * scan_kernel: single-pass exclusive scan with decoupled look-back (one launch; workgroup order taken from an atomic ticket so that
//     every predecessor a workgroup waits on is already resident); value source and consumer are functors, so the producer and the
//     consumer are fused into the scan instead of being separate passes;
//   * fill7f: the workspaces' 0x7F fill as ONE launch (0x7F7F7F7F = the tables' EMPTY key / "no position" value; the look-back status
//     words read as state EMPTY; the ticket counters start at 0x7F7F7F7F);
//   * an open-addressing hash table (linear probing, atomicCAS on int32 keys).
// Everything sits in an anonymous namespace: each translation unit that includes this header gets its own copy.
#pragma once
#include "glnn_common.h"

namespace {

constexpr int kFill32 = 0x7F7F7F7F;
constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kScanThreads * kScanItems;

// look-back status word: top 2 bits = state (01 = EMPTY, what the 0x7F memset leaves; 10 = aggregate; 11 = inclusive prefix)
constexpr unsigned long long kStAgg = 2ull << 62, kStPrefix = 3ull << 62, kStMask = (1ull << 62) - 1;

// The status word carries its own payload (state + value in ONE 64-bit word), so nothing else has to become visible with
// it: relaxed agent-scope atomics (write-through / L2-bypassing accesses) are enough.  Release / acquire at agent scope
// would write back / invalidate the XCD's whole L2 in every workgroup -- on this 8-XCD part that is what a device-scope
// fence costs.
__device__ __forceinline__ void st_release(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_acquire(unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// out(i, exclusive prefix, value) for i in [0,n); *total = sum.  status: >= ceil(n/1024) words, ticket: 1 int, both 0x7F-filled.
template <class V, class W>
__global__ __launch_bounds__(kScanThreads) void scan_kernel(V val, int64_t n, unsigned long long* status, int* ticket, W out,
                                                            int64_t* total) {
  __shared__ int s_bid;
  __shared__ int s_wave[kScanThreads / 64];
  __shared__ long long s_prefix;
  if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1) - kFill32;
  __syncthreads();
  const int bid = s_bid;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)bid * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  int tsum = 0;
#pragma unroll
  for (int t = 0; t < kScanItems; ++t) {
    v[t] = (base + t < n) ? val(base + t) : 0;
    tsum += v[t];
  }
  int inc = tsum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int wave_off = 0, block_sum = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) wave_off += s_wave[w];
    block_sum += s_wave[w];
  }
  if (wave == 0) {
    // decoupled look-back, 64 predecessors per round: lane i inspects workgroup j - i; the wave adds the aggregates up to
    // the nearest published inclusive prefix (a single thread walking the status words one dependent load at a time cost
    // 30-65 us on the 245-workgroup scans of a training batch)
    long long prefix = 0;
    if (bid > 0) {
      if (lane == 0) st_release(status + bid, kStAgg | (unsigned long long)block_sum);
      int j = bid - 1;
      while (true) {
        const int idx = j - lane;
        const unsigned long long sw = idx >= 0 ? ld_acquire(status + idx) : kStPrefix;      // before workgroup 0: prefix 0
        const unsigned long long state = sw >> 62;
        const unsigned long long empties = __ballot(state < 2), prefixes = __ballot(state == 3);
        const int first_p = prefixes ? (__ffsll((unsigned long long)prefixes) - 1) : 64;
        const unsigned long long window = first_p >= 63 ? ~0ull : ((1ull << (first_p + 1)) - 1);
        if (empties & window) {        // a predecessor inside the window holds its ticket (it is resident) but has not published yet
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        unsigned long long v = lane <= first_p ? (sw & kStMask) : 0ull;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const unsigned lo = __shfl_xor((unsigned)(v & 0xFFFFFFFFull), off), hi = __shfl_xor((unsigned)(v >> 32), off);
          v += ((unsigned long long)hi << 32) | lo;
        }
        prefix += (long long)v;
        if (first_p < 64) break;
        j -= 64;
      }
    }
    if (lane == 0) {
      st_release(status + bid, kStPrefix | (unsigned long long)(prefix + block_sum));
      s_prefix = prefix;
      if (bid == (int)gridDim.x - 1 && total) *total = prefix + block_sum;
    }
  }
  __syncthreads();
  long long ex = s_prefix + wave_off + (inc - tsum);
#pragma unroll
  for (int t = 0; t < kScanItems; ++t) {
    if (base + t < n) out(base + t, ex, v[t]);
    ex += v[t];
  }
}

// The workspaces' 0x7F fill as ONE launch: hipMemsetAsync of a few MB at an arbitrary word count shows up as two fill kernels (aligned body +
// tail), and a training step issues eight of them (three blocks built, two transposed): ~5 us each.  p: 4-byte aligned, nwords 32-bit words.
__global__ __launch_bounds__(256) void fill7f_kernel(uint32_t* __restrict__ p, int64_t nwords) {
  const uint32_t v = 0x7F7F7F7Fu;
  int64_t head = (16 - (int64_t)(reinterpret_cast<uintptr_t>(p) & 15)) & 15;
  head >>= 2;
  if (head > nwords) head = nwords;
  const int64_t body4 = (nwords - head) >> 2, tail0 = head + 4 * body4;
  uint4* __restrict__ q = reinterpret_cast<uint4*>(p + head);
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = gtid; i < body4; i += stride) q[i] = make_uint4(v, v, v, v);
  if (gtid < head) p[gtid] = v;
  if (gtid < nwords - tail0) p[tail0 + gtid] = v;
}
static int fill7f(void* p, size_t bytes, hipStream_t st, const char* what) {
  if (bytes == 0) return GLNN_OK;
  if ((bytes & 3) || (reinterpret_cast<uintptr_t>(p) & 3)) {                      // (not the layouts of this file; kept correct)
    return hipMemsetAsync(p, 0x7F, bytes, st) == hipSuccess ? GLNN_OK : glnn::fail(GLNN_ERR_HIP, "%s: memset failed", what);
  }
  const int64_t nwords = (int64_t)(bytes >> 2);
  int64_t blocks = (nwords / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(fill7f_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<uint32_t*>(p), nwords);
  return glnn::check_launch(what);
}

template <class V, class W>
int launch_scan(V val, int64_t n, unsigned long long* status, int* ticket, W out, int64_t* total, hipStream_t st, const char* what) {
  const int64_t blocks = (n + kScanTile - 1) / kScanTile;
  if (blocks == 0) return GLNN_OK;
  hipLaunchKernelGGL((scan_kernel<V, W>), dim3((unsigned)blocks), dim3(kScanThreads), 0, st, val, n, status, ticket, out, total);
  return glnn::check_launch(what);
}

__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ int ht_insert(int* keys, unsigned mask, int key) {
  unsigned slot = hash32((unsigned)key) & mask;
  while (true) {
    const int prev = atomicCAS(&keys[slot], kFill32, key);
    if (prev == kFill32 || prev == key) return (int)slot;
    slot = (slot + 1) & mask;
  }
}

}  // namespace
