"""numpy oracle of glnn_random_walk and glnn_induced_subgraph (docs/SUBGRAPH_SEMANTICS.md).  TEST INFRASTRUCTURE ONLY: plain loops over
small graphs, no torch, no GPU.  The walk's draw is oracle.dropout_mask.drop_hash, the restatement of csrc/glnn_common.h's drop_hash."""
import numpy as np

from oracle.dropout_mask import drop_hash


def random_walk(indptr, indices, roots, length, seed):
    """out [n_roots, length + 1] int64: column 0 the root; step s (1-based) of walk i standing on v moves to
    indices[indptr[v] + ((drop_hash(seed, i, s) * deg) >> 32)], or stays on v when deg == 0."""
    roots = np.asarray(roots, np.int64)
    out = np.zeros((len(roots), length + 1), np.int64)
    out[:, 0] = roots
    if len(roots) == 0:
        return out
    r = drop_hash(seed, np.arange(len(roots))[:, None], np.arange(length + 1)[None, :])      # [n_roots, length + 1] uint64 < 2^32
    for i in range(len(roots)):
        v = int(roots[i])
        for s in range(1, length + 1):
            e0, deg = int(indptr[v]), int(indptr[v + 1] - indptr[v])
            if deg > 0:
                v = int(indices[e0 + ((int(r[i, s]) * deg) >> 32)])
            out[i, s] = v
    return out


def first_appearance(cand):
    """The distinct values of cand in order of first appearance."""
    cand = np.asarray(cand, np.int64)
    _, first = np.unique(cand, return_index=True)
    return cand[np.sort(first)]


def induced_subgraph(indptr, indices, cand, self_loop="keep"):
    """(nodes, sub_indptr, sub_indices int32, zero_rows): row k holds the in-edges u -> nodes[k] whose u is in the set, in the graph's own
    row order, multi-edges kept.  "add": self entries dropped, one k <- k appended to every row."""
    assert self_loop in ("keep", "add")
    nodes = first_appearance(cand)
    local = {int(v): k for k, v in enumerate(nodes)}
    sub_indptr, sub_indices = [0], []
    for k, v in enumerate(nodes):
        for u in indices[indptr[v]:indptr[v + 1]]:
            u = int(u)
            if u in local and not (self_loop == "add" and u == int(v)):
                sub_indices.append(local[u])
        if self_loop == "add":
            sub_indices.append(k)
        sub_indptr.append(len(sub_indices))
    sub_indptr = np.asarray(sub_indptr, np.int64)
    zero_rows = int((np.diff(sub_indptr) == 0).sum())
    return nodes, sub_indptr, np.asarray(sub_indices, np.int32), zero_rows


def hash_slot(ids, cap):
    """Home slot of each id in the builder's open-addressing table of `cap` slots (csrc/frontier_dev.h hash32, masked)."""
    x = np.asarray(ids, np.uint64) & np.uint64(0xFFFFFFFF)
    M = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M
    x ^= x >> np.uint64(16)
    return (x & np.uint64(cap - 1)).astype(np.int64)


def table_cap(nc):
    cap = 64
    while cap < 2 * nc:
        cap <<= 1
    return cap


def six_node_graph():
    """6 nodes: a multi-edge 1 -> 0 (twice), a self-loop on 2, node 5 isolated (no in-edge, no out-edge), 4 without in-edges.
    Edges u -> v (v aggregates from u), listed in the order of v's row: 0: [1, 1, 2]   1: [0, 3]   2: [2, 1, 4]   3: [2]   4: []   5: []"""
    rows = [[1, 1, 2], [0, 3], [2, 1, 4], [2], [], []]
    indptr = np.zeros(7, np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    return indptr, np.asarray([u for r in rows for u in r], np.int32)
