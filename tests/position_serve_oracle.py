"""The fp64 oracle of glnn_position_rows (docs/POSITION_SEMANTICS.md, "Serving by node id"), in numpy alone: the student's input rows
[x[v] | pos(v)] of a batch of node ids, with the per-row figures the error bound of the GPU test is made from."""
import numpy as np


def rows(ids, x, z, slot, indptr=None, indices=None):
    """ids [m]; x [n, f]; z [r, d]; slot [n] (node -> row of z, anything outside [0, r) = not embedded); indptr / indices: the in-edge CSR
    over the n nodes (None: no id is unseen, a row that is gets zeros).  Returns
      out       [m, f + d] float64: out[b, :f] = x[v], out[b, f:] = z[slot[v]] for an embedded v, else the mean of z[slot[u]] over the stored
                entries u of row v that are embedded (a multi-edge as often as it is stored; an entry outside [0, n) is skipped), zeros
                without one
      count     [m] int64: the embedded entries that were averaged (0 for an embedded v)
      mean_abs  [m, d] float64: sum |z[slot[u], j]| / count over the same entries (0 where count is 0)"""
    ids = np.asarray(ids, np.int64)
    x = np.asarray(x, np.float64)
    z = np.asarray(z, np.float64)
    slot = np.asarray(slot, np.int64)
    n, f = x.shape
    r, d = z.shape
    out = np.zeros((len(ids), f + d), np.float64)
    count = np.zeros(len(ids), np.int64)
    mean_abs = np.zeros((len(ids), d), np.float64)
    for b, v in enumerate(ids):
        out[b, :f] = x[v]
        if 0 <= slot[v] < r:
            out[b, f:] = z[slot[v]]
            continue
        if indptr is None:
            continue
        total, total_abs, c = np.zeros(d), np.zeros(d), 0
        for u in np.asarray(indices[indptr[v]:indptr[v + 1]], np.int64):
            if 0 <= u < n and 0 <= slot[u] < r:
                total += z[slot[u]]
                total_abs += np.abs(z[slot[u]])
                c += 1
        if c:
            out[b, f:] = total / c
            mean_abs[b] = total_abs / c
        count[b] = c
    return out, count, mean_abs
