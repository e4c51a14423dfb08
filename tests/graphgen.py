"""Small seeded CSR graphs for the tests (numpy; CSR over destination rows, int64 indptr, int32 indices)."""
import numpy as np


def csr_from_edges(src, dst, n_dst):
    order = np.argsort(dst, kind="stable")
    indices = np.asarray(src)[order].astype(np.int32)
    counts = np.bincount(dst, minlength=n_dst)
    indptr = np.zeros(n_dst + 1, np.int64)
    np.cumsum(counts, out=indptr[1:])
    return indptr, indices


def random_graph(n, avg_deg, seed, power=0.0, self_loops=False, symmetric=False, isolated=0, hub=0):
    """Random multigraph (duplicates kept on purpose: ogbn-arxiv keeps multi-edges, reference
    dataloader.py:75-76).  `isolated` rows get zero in-degree, `hub` adds one very-high-degree row."""
    rs = np.random.RandomState(seed)
    m = int(n * avg_deg)
    if power > 0:
        w = (np.arange(n) + 3.0) ** (-power)
        w = rs.permutation(w / w.sum())
        dst = rs.choice(n, size=m, p=w)
    else:
        dst = rs.randint(0, n, size=m)
    src = rs.randint(0, n, size=m)
    if hub:
        h = rs.randint(0, n)
        src = np.concatenate([src, rs.randint(0, n, size=hub)])
        dst = np.concatenate([dst, np.full(hub, h)])
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    if isolated:
        iso = rs.choice(n, size=isolated, replace=False)
        keep = ~np.isin(dst, iso)
        src, dst = src[keep], dst[keep]
    if self_loops:
        src = np.concatenate([src, np.arange(n)])
        dst = np.concatenate([dst, np.arange(n)])
    return csr_from_edges(src, dst, n)


def segment_reduce(ufunc, vals, idx, n, init):
    """out[r] = ufunc-reduction of vals[idx == r] over axis 0, `init` for the rows no entry names: what `ufunc.at` leaves in an
    init-filled array, by one stable sort and one `reduceat` (entries of a row are folded in their given order).  The fp64 oracles
    use it so that a graph of a few hundred thousand rows costs them a fraction of a second."""
    idx = np.asarray(idx)
    vals = np.asarray(vals)
    counts = np.bincount(idx, minlength=n)
    out = np.full((n,) + vals.shape[1:], init, dtype=vals.dtype)
    if len(idx) == 0:
        return out
    if np.any(idx[1:] < idx[:-1]):
        vals = vals[np.argsort(idx, kind="stable")]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    live = counts > 0
    out[live] = ufunc.reduceat(vals, starts[live], axis=0)
    return out


def planted_graph(n, seed, in_deg, out_deg, lone, extra=2.0):
    """Large multigraph built without a loop over its rows: a self-loop on every row and about `extra` random in-edges per row (mean
    degree about 1 + extra), around rows whose degrees are EXACT -- `in_deg` {row: in-degree}, `out_deg` {row: out-degree}, `lone`
    (rows whose only in-edge is their self-loop).  No random edge touches a planted row; the planted edges' other ends are drawn from
    the unplanted rows (with replacement: a hub may see a multi-edge)."""
    rs = np.random.RandomState(seed)
    in_rows, out_rows = np.array(sorted(in_deg), np.int64), np.array(sorted(out_deg), np.int64)
    in_cnt = np.array([in_deg[r] for r in in_rows], np.int64)
    out_cnt = np.array([out_deg[r] for r in out_rows], np.int64)
    lone = np.asarray(lone, np.int64)
    planted = np.concatenate([in_rows, out_rows, lone])
    assert len(np.unique(planted)) == len(planted) and planted.min() >= 0 and planted.max() < n
    special = np.zeros(n, bool)
    special[planted] = True
    m = int(n * extra)
    src, dst = rs.randint(0, n, size=m), rs.randint(0, n, size=m)
    keep = ~(special[src] | special[dst])
    pool = np.flatnonzero(~special)
    hub_dst = np.repeat(in_rows, in_cnt - 1)
    fan_src = np.repeat(out_rows, out_cnt - 1)
    loops = np.arange(n)
    src = np.concatenate([src[keep], rs.choice(pool, hub_dst.size), fan_src, loops])
    dst = np.concatenate([dst[keep], hub_dst, rs.choice(pool, fan_src.size), loops])
    return csr_from_edges(src, dst, n)


def scan_geometry(n, block, waves, rows_per_wave, long_block_rows, long_block_cap):
    """(n_chunks, n_long_blocks, rows_per_block) as the row kernels of gat.hip and appnp.hip derive them from their constants (the
    caller names those): the long-row scan looks at n_chunks chunks of `block` rows with n_long_blocks workgroups, the other workgroups
    take rows_per_block rows each."""
    n_chunks = -(-n // block)
    n_long_blocks = min(-(-n // long_block_rows), long_block_cap)
    rows_per_block = min(max(n // (2048 * waves), 1), rows_per_wave) * waves
    return n_chunks, n_long_blocks, rows_per_block


def second_trip_plan(n, n_chunks, n_long_blocks, long_row):
    """(in_deg, out_deg, lone) for planted_graph.  The scan reaches row r = k n_chunks + c (thread k, chunk c) in trip c // n_long_blocks
    of workgroup c % n_long_blocks, so a long row with r % n_chunks >= n_long_blocks is found on a SECOND trip only.  Planted on both
    sides (destinations for the in-CSR passes, sources for the passes over the transpose): long rows of either trip, rows just below,
    at and just above `long_row`, a one-wave row of two 64-entry chunks; `lone` rows keep their self-loop alone."""
    assert n_chunks >= n_long_blocks + 2 and 510 * n_chunks + n_long_blocks < n
    late = lambda k, c: k * n_chunks + n_long_blocks + c
    early = lambda k, c: k * n_chunks + c
    in_deg = {late(3, 0): 300, late(200, 1): long_row + 1, late(510, 0): 190, early(10, 7): 700, early(194, 284): 200,
              early(40, 100): long_row - 1, early(41, 101): long_row, early(42, 102): long_row + 1, early(43, 103): 65}
    out_deg = {late(5, 1): 260, late(333, 0): long_row + 1, early(77, 300): 500,
               early(50, 200): long_row - 1, early(51, 201): long_row, early(52, 202): long_row + 1, early(53, 203): 90}
    lone = np.arange(11, n, 997)
    lone = lone[~np.isin(lone, list(in_deg) + list(out_deg))]
    return in_deg, out_deg, lone
