"""numpy oracles of the integer half of the minibatch training path: glnn_sample_neighbors (csrc/sample.hip), glnn_block_build
(csrc/blocks.hip), glnn_csr_transpose (csrc/blocks.hip) and glnn_csr_transpose_eids (csrc/appnp.hip).  TEST INFRASTRUCTURE ONLY: plain
loops over small graphs, no torch, no GPU.  The sampler's draw is oracle.dropout_mask.drop_hash, the restatement of csrc/glnn_common.h's
drop_hash."""
import numpy as np

from oracle.dropout_mask import drop_hash

NO_ENTRY = -1            # what sample_neighbors leaves in the slots of a row past its count


def floyd_positions(deg, fanout, seed, rows):
    """Floyd's algorithm as the kernel runs it, for rows of more than `fanout` entries: deg [m] the rows' lengths, rows [m] the index i
    of each row in the seed list (the RNG is keyed by it, not by the node id).  For s = 0 .. fanout-1: j = deg - fanout + s,
    t = (drop_hash(seed, i, s) * (j + 1)) >> 32, position j if t was picked before, else t.
    Returns (picked [m, fanout] int64, redirected [m, fanout] bool)."""
    deg = np.asarray(deg, np.int64)
    rows = np.asarray(rows, np.int64)
    assert (deg > fanout).all()
    picked = np.full((len(deg), fanout), -1, np.int64)
    redirected = np.zeros((len(deg), fanout), bool)
    for s in range(fanout):
        j = deg - fanout + s
        r = drop_hash(seed, rows, s)                                   # uint64 < 2^32
        t = ((r * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        dup = (picked[:, :s] == t[:, None]).any(axis=1)
        picked[:, s] = np.where(dup, j, t)
        redirected[:, s] = dup
    return picked, redirected


def sample_neighbors(indptr, indices, seeds, fanout, seed):
    """(src [n_seeds, fanout] int32, cnt [n_seeds] int32, n_redirects): a row of at most `fanout` entries keeps them in row order, a
    longer one gives indices[e0 + picked[s]] in slot s (floyd_positions).  Slots past cnt[i] hold NO_ENTRY.  n_redirects counts the
    picks that went to j because t was taken."""
    indptr = np.asarray(indptr, np.int64)
    seeds = np.asarray(seeds, np.int64)
    e0 = indptr[seeds]
    deg = indptr[seeds + 1] - e0
    src = np.full((len(seeds), fanout), NO_ENTRY, np.int32)
    cnt = np.minimum(deg, fanout).astype(np.int32)
    for i in np.flatnonzero(deg <= fanout):
        src[i, :deg[i]] = indices[e0[i]:e0[i] + deg[i]]
    big = np.flatnonzero(deg > fanout)
    picked, redirected = floyd_positions(deg[big], fanout, seed, big)
    if len(big):
        src[big] = np.asarray(indices)[e0[big, None] + picked]
    return src, cnt, int(redirected.sum())


def inclusion_statistic(counts, draws, fanout):
    """Chi-square statistic of the inclusion counts of the deg positions of one row over `draws` samples of `fanout` positions without
    replacement: every count has mean E = draws * fanout / deg and variance E (1 - fanout / deg); the counts sum to draws * fanout, so
    sum((c - E)^2 / var) * (deg - 1) / deg has deg - 1 degrees of freedom."""
    counts = np.asarray(counts, np.float64)
    deg = len(counts)
    e = draws * fanout / deg
    return float(((counts - e) ** 2 / (e * (1.0 - fanout / deg))).sum() * (deg - 1) / deg)


def chi2_quantile(df, upper_tail):
    """The value a chi-square variable of `df` degrees of freedom exceeds with probability `upper_tail`: bisection on the regularised
    upper incomplete gamma function Q(df / 2, x / 2), evaluated by its series (x < a + 1) or its continued fraction (Numerical Recipes
    section 6.2)."""
    import math

    def q(a, x):
        if x <= 0:
            return 1.0
        lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
        if x < a + 1:
            term = total = 1.0 / a
            n = a
            for _ in range(10000):
                n += 1
                term *= x / n
                total += term
                if abs(term) < abs(total) * 1e-16:
                    break
            return 1.0 - total * lead
        tiny = 1e-300
        b = x + 1 - a
        c = 1 / tiny
        d = 1 / b
        h = d
        for i in range(1, 10000):
            an = -i * (i - a)
            b += 2
            d = an * d + b
            d = tiny if abs(d) < tiny else d
            c = b + an / c
            c = tiny if abs(c) < tiny else c
            d = 1 / d
            delta = d * c
            h *= delta
            if abs(delta - 1) < 1e-16:
                break
        return lead * h

    lo, hi = 0.0, float(df)
    while q(df / 2.0, hi / 2.0) > upper_tail:
        hi *= 2
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if q(df / 2.0, mid / 2.0) > upper_tail:
            lo = mid
        else:
            hi = mid
    return hi


def first_appearance_block(seeds, rows):
    """numpy restatement of glnn_block_build: rows[i] = global source ids of destination i, in order.  The block's source nodes are its
    destinations first, then every other source in order of first appearance.  Returns (indptr, local indices int32, input_nodes)."""
    pos = {int(v): i for i, v in enumerate(seeds)}
    input_nodes = [int(v) for v in seeds]
    indptr, local = [0], []
    for r in rows:
        for u in r:
            u = int(u)
            if u not in pos:
                pos[u] = len(input_nodes)
                input_nodes.append(u)
            local.append(pos[u])
        indptr.append(len(local))
    return np.asarray(indptr, np.int64), np.asarray(local, np.int32), np.asarray(input_nodes, np.int64)


def table_direct(ns, nnz_cap, n_nodes):
    """Whether block_build_impl indexes its tables by the node id itself: 0 < n_nodes <= 2 cap, cap = the power of two at or above
    2 (ns + nnz_cap), at least 64."""
    cap = 64
    while cap < 2 * (ns + nnz_cap):
        cap <<= 1
    return 0 < n_nodes <= 2 * cap


def csr_transpose(indptr, indices, n_dst, n_src, add_self=False):
    """(t_indptr [n_src + 1] int64, t_indices int32, t_eids int32 or None): the CSR-ordered edges (destination ascending, row order
    within a destination) stably sorted by source -- the destinations of one source come out ascending, parallel edges u -> v in
    ascending edge id (t_eids = np.lexsort((eid, dst, src))).  add_self: one entry u <- u per u < n_dst in sorted position among the
    row's destinations; no edge ids then."""
    indptr = np.asarray(indptr, np.int64)
    nnz = int(indptr[n_dst])
    dst = np.repeat(np.arange(n_dst, dtype=np.int64), np.diff(indptr[:n_dst + 1]))
    src = np.asarray(indices[:nnz], np.int64)
    t_indptr = np.zeros(n_src + 1, np.int64)
    if add_self:
        src = np.concatenate([src, np.arange(n_dst, dtype=np.int64)])
        dst = np.concatenate([dst, np.arange(n_dst, dtype=np.int64)])
        order = np.lexsort((dst, src))
    else:
        order = np.argsort(src, kind="stable")
    np.cumsum(np.bincount(src, minlength=n_src), out=t_indptr[1:])
    return t_indptr, dst[order].astype(np.int32), (None if add_self else order.astype(np.int32))


def row_profile(t_indptr, t_indices):
    """(length [n] of every row, has_tie [n]: the row holds some value twice -- rows are sorted, so two neighbouring entries are equal)."""
    t_indptr = np.asarray(t_indptr, np.int64)
    n = len(t_indptr) - 1
    length = np.diff(t_indptr)
    row = np.repeat(np.arange(n), length)
    ix = np.asarray(t_indices)
    tie = (row[1:] == row[:-1]) & (ix[1:] == ix[:-1])
    return length, np.bincount(row[1:][tie], minlength=n) > 0


SORT_LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65)
LONG_ROW = 700


def sort_path_graph(n=3000, seed=3):
    """Square graph of n rows whose SOURCES have planted out-degrees -- the rows of the transpose, which tr_sort_kernel orders in
    registers (1..4 entries), by shuffle rank (5..64) or by the quadratic rank (above 64).  For each k of SORT_LENGTHS and for LONG_ROW:
    one source with k distinct destinations and (k >= 2) one with a repeated destination, so that tied keys occur in every path; the
    tied 5-entry row holds one destination three times (a, a, a, b, c), the tied long row one three times and another twice.  No
    planted source is a destination of its own, but for planted[("loop", False)], whose only out-edge is its self-loop: with add_self
    its row is the tied row of two entries.  Every other source gets three random out-edges on average.
    Returns (indptr, indices, planted) with planted = {(k, tied): source}."""
    rs = np.random.RandomState(seed)
    ks = list(SORT_LENGTHS) + [LONG_ROW]
    slots = [(k, tied) for k in ks for tied in (False, True) if not (tied and k < 2)] + [("loop", False)]
    nodes = rs.permutation(n)[:len(slots)]
    planted = {slot: int(u) for slot, u in zip(slots, nodes)}
    special = np.zeros(n, bool)
    special[nodes] = True
    src = rs.randint(0, n, size=3 * n)
    dst = rs.randint(0, n, size=3 * n)
    keep = ~special[src]
    src, dst = [src[keep]], [dst[keep]]
    for (k, tied), u in planted.items():
        pool = np.setdiff1d(np.arange(n), [u])
        if k == "loop":
            k, d = 1, np.asarray([u])
        elif not tied:
            d = rs.choice(pool, k, replace=False)
        else:
            extra = 3 if k == LONG_ROW else (2 if k == 5 else 1)             # entries that repeat an earlier destination
            d = rs.choice(pool, k - extra, replace=False)
            reps = [d[0], d[0], d[1]] if k == LONG_ROW else ([d[0], d[0]] if k == 5 else [d[0]])
            d = np.concatenate([d, reps])
        assert len(d) == k
        d = rs.permutation(d)
        src.append(np.full(k, u, np.int64))
        dst.append(d)
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.argsort(dst, kind="stable")
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=indptr[1:])
    return indptr, src[order].astype(np.int32), planted
