// Random-walk node sampling and frontier-sized induced subgraphs on the GPU: what lets the full-graph teachers (GCN, APPNP, GAT, GATv2,
// GPRGNN, GCNII) train in mini-batches -- every TeacherEngine.step_* takes any CSRGraph, so a small induced subgraph is a batch.
// Integer, latency-bound work sized by the CANDIDATE LIST and the in-degrees of its nodes, never by N or E (CSRGraph.subgraph allocates an
// N-sized remap, expands and masks all E edges and argsorts the rest).  docs/SUBGRAPH_SEMANTICS.md states the contract.
//
//   glnn_random_walk        one thread per walk: `length` dependent steps, each ONE counter-based draw (glnn::drop_hash, the draw of
//                           csrc/sample.hip) over the current node's in-edges;
//   glnn_induced_subgraph   candidates -> table insert (atomicMin on list positions, so "first appearance" does not depend on arrival
//                           order) -> scan over first occurrences (dense local ids, `nodes`) -> row counts (one wave per row, lanes
//                           stride the graph's row, membership = a table lookup) -> scan (indptr) -> fill (the same walk, entries
//                           placed by ballot rank: the graph's own row order).
// The scan, the 0x7F-filled workspace and the hash / direct-index table are those of the block builder (csrc/frontier_dev.h).
#include "glnn_common.h"
#include "frontier_dev.h"

namespace {

// ------------------------------------------------------------------------------------------------ random walk
__global__ __launch_bounds__(256) void random_walk_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                          const int64_t* __restrict__ roots, int64_t n_roots, int length, uint32_t seed,
                                                          int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_roots) return;
  int64_t v = roots[i];
  int64_t* row = out + i * (int64_t)(length + 1);
  row[0] = v;
  for (int s = 1; s <= length; ++s) {
    const int64_t e0 = indptr[v];
    const int64_t deg = indptr[v + 1] - e0;
    if (deg > 0) {              // (deg == 0: the walk stays where it is)
      const uint32_t r = glnn::drop_hash(seed, (uint32_t)i, (uint32_t)s);
      v = indices[e0 + (int64_t)(((uint64_t)r * (uint64_t)deg) >> 32)];
    }
    row[s] = v;
  }
}

// ------------------------------------------------------------------------------------------------ induced subgraph
struct SubArgs {
  const int64_t* g_indptr; const int32_t* g_indices;      // graph CSR by destination
  const int64_t* cand; int64_t nc;                        // candidate node ids (repeats allowed)
  int n_nodes;                                            // id universe: ids outside [0, n_nodes) are reported, never indexed with
  int add_self;                                           // 0 = keep, 1 = add (drop self entries, append one per row)
  int64_t nnz_cap;                                        // entries `indices` can hold
  int64_t* nodes;               // out [nc]     local id -> global id
  int64_t* indptr;              // out [nc + 1]
  int32_t* indices;             // out [nnz_cap] local ids
  int64_t* counts;              // out device [3]: n_sub (-1: an id out of range), nnz (true count), rows without an entry
  int* keys; int* pos; unsigned mask; int direct;         // the table: see slot / lookup below
  int* slot_of_cand;            // [nc] table slot of candidate j, -1 for an id out of range
  int* rowcnt;                  // [nc] entries of row k
  int64_t* n_sub;               // total of the first-occurrence scan
  int* bad;                     // set to 0 (from the 0x7F fill) by an id out of range
  int* zero_rows;               // 0x7F7F7F7F + the number of rows without an entry
};

// The position word of a candidate node (one per table slot, 0x7F-filled = absent), as in the block builder:
//   insert   candidate j writes j by atomicMin -> the node's FIRST list position, whatever order the threads arrive in;
//   scan     candidate j is a first occurrence iff pos == j; its dense local id replaces the word with bit 30 set (never equal to a j');
//   lookup   local id = pos & 0x3FFFFFFF.
constexpr int kSubLocalBit = 1 << 30;

template <bool DIRECT>
__global__ __launch_bounds__(256) void sub_insert_kernel(const SubArgs a) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.nc) return;
  const int64_t v = a.cand[j];
  if (v < 0 || v >= (int64_t)a.n_nodes) {
    *a.bad = 0;
    a.slot_of_cand[j] = -1;
    return;
  }
  const int slot = DIRECT ? (int)v : ht_insert(a.keys, a.mask, (int)v);
  atomicMin(&a.pos[slot], (int)j);
  a.slot_of_cand[j] = slot;
}

struct SubFirstSeen {
  SubArgs a;
  __device__ int operator()(int64_t j) const {
    const int slot = a.slot_of_cand[j];
    return (slot >= 0 && a.pos[slot] == (int)j) ? 1 : 0;
  }
};
struct SubAssignLocal {
  SubArgs a;
  __device__ void operator()(int64_t j, long long ex, int flag) const {
    if (flag) {
      a.pos[a.slot_of_cand[j]] = (int)ex | kSubLocalBit;
      a.nodes[ex] = a.cand[j];
    }
  }
};

// local id of graph node `key`, -1 when it is not in the set (read-only: runs in launches behind the first-occurrence scan)
template <bool DIRECT>
__device__ __forceinline__ int sub_lookup(const SubArgs& a, int key) {
  if ((unsigned)key >= (unsigned)a.n_nodes) return -1;
  if (DIRECT) {
    const int p = a.pos[key];
    return p == kFill32 ? -1 : (p & (kSubLocalBit - 1));
  }
  unsigned slot = hash32((unsigned)key) & a.mask;
  while (true) {                // (the table holds <= nc keys in >= 2 nc slots: an EMPTY slot ends every probe sequence)
    const int k = a.keys[slot];
    if (k == key) return a.pos[slot] & (kSubLocalBit - 1);
    if (k == kFill32) return -1;
    slot = (slot + 1) & a.mask;
  }
}

// One wave per row k < n_sub, lanes stride the in-edges of nodes[k] 64 at a time (a 700-entry hub row is 11 rounds of the whole wave, not
// 700 steps of one lane).  FILL = false: count the entries the row keeps.  FILL = true: write them, each at indptr[k] + its rank among the
// kept entries (ballot prefix) -- the graph's own row order, multi-edges kept; mode `add` drops self entries and appends ONE k <- k.
template <bool DIRECT, bool FILL>
__global__ __launch_bounds__(256) void sub_rows_kernel(const SubArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t k = t >> 6;
  const int lane = (int)(t & 63);
  const int64_t n_sub = *a.n_sub;
  if (FILL && t == 0) {
    a.counts[0] = *a.bad == 0 ? -1 : n_sub;
    a.counts[1] = n_sub > 0 ? a.indptr[n_sub] : 0;
    a.counts[2] = (int64_t)*a.zero_rows - kFill32;
    if (n_sub == 0) a.indptr[0] = 0;
  }
  if (k >= n_sub) return;
  const int64_t v = a.nodes[k];
  const int64_t g0 = a.g_indptr[v], cnt = a.g_indptr[v + 1] - g0;
  const int64_t base = FILL ? a.indptr[k] : 0;
  int64_t kept = 0;
  for (int64_t i0 = 0; i0 < cnt; i0 += 64) {          // (cnt is uniform across the wave: every lane takes every round)
    const int64_t i = i0 + lane;
    int local = -1;
    if (i < cnt) {
      const int u = a.g_indices[g0 + i];
      if (!(a.add_self && (int64_t)u == v)) local = sub_lookup<DIRECT>(a, u);
    }
    const unsigned long long in = __ballot(local >= 0);
    if (FILL && local >= 0) {
      const int64_t at = base + kept + __popcll(in & ((1ull << lane) - 1));
      if (at < a.nnz_cap) a.indices[at] = local;       // (counts[1] reports the true nnz: the caller checks it against nnz_cap)
    }
    kept += __popcll(in);
  }
  if (lane == 0) {
    if (a.add_self) {
      if (FILL && base + kept < a.nnz_cap) a.indices[base + kept] = (int)k;
      kept += 1;
    }
    if (!FILL) {
      a.rowcnt[k] = (int)kept;
      if (kept == 0) atomicAdd(a.zero_rows, 1);
    }
  }
}

struct SubRowCount {
  SubArgs a;
  __device__ int operator()(int64_t k) const { return k < *a.n_sub ? a.rowcnt[k] : 0; }
};
struct SubWriteIndptr {
  SubArgs a;
  __device__ void operator()(int64_t k, long long ex, int v) const {
    const int64_t n_sub = *a.n_sub;
    if (k < n_sub) a.indptr[k] = ex;
    if (k == n_sub - 1) a.indptr[n_sub] = ex + v;
  }
};

__global__ void sub_empty_kernel(int64_t* counts, int64_t* indptr) {
  counts[0] = counts[1] = counts[2] = 0;
  indptr[0] = 0;
}

uint64_t sub_table_cap(int64_t nc) {
  uint64_t cap = 64;
  while (cap < (uint64_t)(2 * nc)) cap <<= 1;
  return cap;
}

}  // namespace

extern "C" int glnn_random_walk(const int64_t* indptr, const int32_t* indices, const int64_t* roots, int64_t n_roots, int length,
                                uint32_t rng_seed, int64_t* out, void* stream) {
  GLNN_REQUIRE(n_roots >= 0 && length >= 1 && length <= 64, "glnn_random_walk: length must be in [1,64]");
  if (n_roots == 0) return GLNN_OK;
  GLNN_REQUIRE(indptr && indices && roots && out, "glnn_random_walk: null pointer");
  GLNN_REQUIRE(n_roots < ((int64_t)1 << 32), "glnn_random_walk: the walk index is a 32-bit counter of the draw");
  hipLaunchKernelGGL(random_walk_kernel, dim3((unsigned)((n_roots + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     indptr, indices, roots, n_roots, length, rng_seed, out);
  return glnn::check_launch("glnn_random_walk");
}

// 1: the table of an (nc, n_nodes) build is indexed by the node id itself; 0: open addressing over 2..4 nc slots
extern "C" int glnn_induced_subgraph_direct(int64_t nc, int64_t n_nodes) {
  if (nc < 0 || n_nodes <= 0) return 0;
  return (uint64_t)n_nodes <= 2 * sub_table_cap(nc) ? 1 : 0;
}

extern "C" int64_t glnn_induced_subgraph_workspace_bytes(int64_t nc, int64_t n_nodes) {
  if (nc < 0 || n_nodes < 0) return -1;
  const int64_t b = (nc + kScanTile - 1) / kScanTile;
  return (2 * b + 3) * 8 + (int64_t)(2 * sub_table_cap(nc) * sizeof(int)) + 2 * nc * (int64_t)sizeof(int) + 64;
}

extern "C" int glnn_induced_subgraph(const int64_t* g_indptr, const int32_t* g_indices, int64_t n_nodes, const int64_t* cand, int64_t nc,
                                     int self_loop, int64_t nnz_cap, int64_t* nodes, int64_t* indptr, int32_t* indices,
                                     int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  GLNN_REQUIRE(nc >= 0 && nnz_cap >= 0 && n_nodes >= 0, "glnn_induced_subgraph: negative size");
  GLNN_REQUIRE(self_loop == 0 || self_loop == 1, "glnn_induced_subgraph: self_loop must be 0 (keep) or 1 (add)");
  GLNN_REQUIRE(counts && indptr, "glnn_induced_subgraph: null counts/indptr");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (nc == 0) {
    hipLaunchKernelGGL(sub_empty_kernel, dim3(1), dim3(1), 0, st, counts, indptr);
    return glnn::check_launch("glnn_induced_subgraph");
  }
  GLNN_REQUIRE(g_indptr && g_indices && cand && nodes && workspace && (indices || nnz_cap == 0), "glnn_induced_subgraph: null pointer");
  GLNN_REQUIRE(nc < ((int64_t)1 << 30) && nnz_cap < ((int64_t)1 << 31) && n_nodes < kFill32,
               "glnn_induced_subgraph: candidate list / capacity / id universe too large for 32-bit positions");
  GLNN_REQUIRE(workspace_bytes >= glnn_induced_subgraph_workspace_bytes(nc, n_nodes) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "glnn_induced_subgraph: workspace needs %lld bytes, 8-byte aligned", (long long)glnn_induced_subgraph_workspace_bytes(nc, n_nodes));
  const uint64_t cap = sub_table_cap(nc);
  const bool direct = glnn_induced_subgraph_direct(nc, n_nodes) != 0;
  const uint64_t tab = direct ? (uint64_t)((n_nodes + 1) & ~(int64_t)1) : cap;      // entries per table (even: what follows stays 8-byte aligned)
  const int64_t b = (nc + kScanTile - 1) / kScanTile;
  // layout: [status1 b][status2 b][ticket1, ticket2][n_sub (8 bytes)][bad, zero_rows] | (keys,) pos | -- 0x7F-filled up to here
  //         slot_of_cand [nc] | rowcnt [nc]
  unsigned long long* status1 = reinterpret_cast<unsigned long long*>(workspace);
  unsigned long long* status2 = status1 + b;
  int* tickets = reinterpret_cast<int*>(status2 + b);
  int64_t* n_sub = reinterpret_cast<int64_t*>(tickets + 2);
  int* flags = reinterpret_cast<int*>(n_sub + 1);
  int* tables = flags + 2;
  SubArgs a;
  a.g_indptr = g_indptr; a.g_indices = g_indices; a.cand = cand; a.nc = nc; a.n_nodes = (int)n_nodes; a.add_self = self_loop;
  a.nnz_cap = nnz_cap; a.nodes = nodes; a.indptr = indptr; a.indices = indices; a.counts = counts;
  a.direct = direct ? 1 : 0; a.mask = (unsigned)(cap - 1);
  a.keys = direct ? nullptr : tables;
  a.pos = direct ? tables : tables + tab;
  a.slot_of_cand = a.pos + tab; a.rowcnt = a.slot_of_cand + nc;
  a.n_sub = n_sub; a.bad = flags; a.zero_rows = flags + 1;
  int rc = fill7f(workspace, (size_t)((2 * b + 3) * 8) + (direct ? 1 : 2) * tab * sizeof(int), st, "glnn_induced_subgraph(fill)");
  if (rc != GLNN_OK) return rc;
  const dim3 per_cand((unsigned)((nc + 255) / 256)), per_row((unsigned)((nc * 64 + 255) / 256));
  if (direct) hipLaunchKernelGGL(sub_insert_kernel<true>, per_cand, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(sub_insert_kernel<false>, per_cand, dim3(256), 0, st, a);
  rc = glnn::check_launch("glnn_induced_subgraph(insert)");
  if (rc != GLNN_OK) return rc;
  rc = launch_scan(SubFirstSeen{a}, nc, status1, tickets, SubAssignLocal{a}, n_sub, st, "glnn_induced_subgraph(scan first occurrences)");
  if (rc != GLNN_OK) return rc;
  if (direct) hipLaunchKernelGGL((sub_rows_kernel<true, false>), per_row, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((sub_rows_kernel<false, false>), per_row, dim3(256), 0, st, a);
  rc = glnn::check_launch("glnn_induced_subgraph(count rows)");
  if (rc != GLNN_OK) return rc;
  rc = launch_scan(SubRowCount{a}, nc, status2, tickets + 1, SubWriteIndptr{a}, nullptr, st, "glnn_induced_subgraph(scan rows)");
  if (rc != GLNN_OK) return rc;
  if (direct) hipLaunchKernelGGL((sub_rows_kernel<true, true>), per_row, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((sub_rows_kernel<false, true>), per_row, dim3(256), 0, st, a);
  return glnn::check_launch("glnn_induced_subgraph(fill rows)");
}
