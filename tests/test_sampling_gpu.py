"""The integer half of the minibatch training path on the GPU, array for array against the numpy oracles of tests/sampling_oracle.py:
glnn_sample_neighbors (every compiled fan-out bound, the draws themselves), glnn_block_build / glnn_block_build_ids (wide fan-outs, the
direct / hash switch, bad ids, a capacity that is too small), glnn_csr_transpose (the three sort paths with tied keys, the block form,
the separate zero fill and the capped grids at 2^23 entries) and glnn_csr_transpose_eids (the order among parallel edges).
Everything is exact: no tolerances.  docs/KERNEL_COVERAGE.md maps the branches to the tests here."""
import ctypes

import numpy as np
import pytest
import torch

import sampling_oracle as so
import subgraph_oracle as sgo
from graphgen import csr_from_edges, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, WORD64, WORD32 = 512, -0x0123456789ABCDEF, 0x5A5A5A5A          # (a relabel workgroup is 256 threads: the tail is wider than one)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _full(n, word, dtype):
    return torch.full((n + GUARD,), word, dtype=dtype, device=DEV)


def _np(t):
    return t.cpu().numpy()


class _G:
    """random_graph(2000, 30, seed=11, power=0.7, hub=900, isolated=15): for every fan-out from 7 to 64 it has rows below, at, one above
    and far above the fan-out (asserted where used); 15 rows have no in-edge, the hub has 983."""
    n = 2000

    def __init__(self):
        self.ip, self.ix = random_graph(self.n, 30, seed=11, power=0.7, hub=900, isolated=15)
        self.deg = np.diff(self.ip)
        assert self.deg.max() == 983 and (self.deg == 0).sum() == 15
        self.tip, self.tix = _t(self.ip), _t(self.ix)

    def rows(self, seeds):
        return [self.ix[self.ip[v]:self.ip[v + 1]] for v in seeds]


@pytest.fixture(scope="module")
def G():
    return _G()


# ------------------------------------------------------------------------------------------------ sampler
def _raw_sample(tip, tix, seeds, n_seeds, fanout, rng_seed):
    """glnn_sample_neighbors on sentinel-filled buffers of exactly [n_seeds, fanout] / [n_seeds] words followed by GUARD sentinel words."""
    from glnn_amd import _lib, ops
    h = _lib.lib()
    rows = max(fanout, 0)
    src = _full(n_seeds * rows, WORD32, torch.int32)
    cnt = _full(n_seeds, WORD32, torch.int32)
    rc = h.glnn_sample_neighbors(_p(tip), _p(tix), _p(seeds), n_seeds, fanout, rng_seed, _p(src), _p(cnt), ops._stream())
    torch.cuda.synchronize()
    return rc, _np(src), _np(cnt)


@pytest.mark.parametrize("fanout", [1, 7, 8, 9, 16, 17, 32, 33, 63, 64])
def test_sampler_equals_the_oracle_bit_for_bit(G, fanout):
    """Fan-outs on both sides of every bound of the dispatch (F = 8 / 16 / 32 / 64).  Seeds: a permutation of all nodes plus one row of
    fanout + 1 entries a hundred times (the RNG is keyed by the seed's index: a hundred different draws in which the last pick nearly
    always meets a taken position)."""
    from glnn_amd import _lib
    deg, f = G.deg, fanout
    if f == 1:
        assert (deg == 0).any() and (deg > 1).any()
        tight = int(np.flatnonzero(deg > f)[np.argmin(deg[deg > f])])          # (no row of two entries: the shortest row that is sampled)
    else:
        assert (deg < f).any() and (deg == f).any() and (deg == f + 1).any() and (deg > 2 * f).any()
        tight = int(np.flatnonzero(deg == f + 1)[0])
    seeds = np.concatenate([np.random.RandomState(f).permutation(G.n), np.full(100, tight)]).astype(np.int64)
    n = len(seeds)
    assert n % 256 != 0 and n > 256                                               # several workgroups, a ragged last one
    rng_seed = 1000 + f
    want_src, want_cnt, n_redirects = so.sample_neighbors(G.ip, G.ix, seeds, f, rng_seed)
    if f >= 7:
        assert n_redirects > 0                                                    # Floyd's duplicate redirect is taken at this F
    rc, src, cnt = _raw_sample(G.tip, G.tix, _t(seeds), n, f, rng_seed)
    assert rc == 0, _lib.lib().glnn_last_error()
    assert np.array_equal(cnt[:n], want_cnt)
    src, tail = src[:n * f].reshape(n, f), src[n * f:]
    written = np.arange(f)[None, :] < want_cnt[:, None]
    assert np.array_equal(src[written], want_src[written])                        # the first cnt[i] entries of every row, in order
    assert (src[~written] == WORD32).all()                                        # a short row's other slots are not touched
    assert (tail == WORD32).all() and (cnt[n:] == WORD32).all()
    rc, src2, _ = _raw_sample(G.tip, G.tix, _t(seeds), n, f, rng_seed + 1)        # another seed, other draws: the oracle's
    want2, _, _ = so.sample_neighbors(G.ip, G.ix, seeds, f, rng_seed + 1)
    src2 = src2[:n * f].reshape(n, f)
    assert rc == 0 and np.array_equal(src2[written], want2[written]) and not np.array_equal(src2, src)


def test_sampler_without_seeds_and_refused_fanouts(G):
    from glnn_amd import _lib
    seeds = _t(np.arange(300, dtype=np.int64))
    rc, src, cnt = _raw_sample(G.tip, G.tix, seeds, 0, 10, 1)                     # no seeds: OK, nothing launched
    assert rc == 0 and (src == WORD32).all() and (cnt == WORD32).all()
    for fanout in (0, 65, -1):
        from glnn_amd import ops
        h = _lib.lib()
        src = _full(300 * 65, WORD32, torch.int32)
        cnt = _full(300, WORD32, torch.int32)
        rc = h.glnn_sample_neighbors(_p(G.tip), _p(G.tix), _p(seeds), 300, fanout, 1, _p(src), _p(cnt), ops._stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"[1,64]" in h.glnn_last_error()
        assert (src == WORD32).all() and (cnt == WORD32).all()


# ------------------------------------------------------------------------------------------------ block builder
def _check_block(got, seeds, rows):
    ip, ix, gix, inp, nnz, n_src = got
    w_ip, w_ix, w_in = so.first_appearance_block(seeds, rows)
    flat = np.concatenate(rows).astype(np.int32) if len(w_ix) else np.zeros(0, np.int32)
    assert nnz == w_ip[-1] and n_src == len(w_in)
    assert ip.dtype == torch.int64 and ix.dtype == torch.int32 and inp.dtype == torch.int64
    assert np.array_equal(_np(ip), w_ip) and np.array_equal(_np(ix), w_ix) and np.array_equal(_np(inp), w_in)
    assert np.array_equal(_np(gix), flat)
    return w_ip, w_ix, w_in


@pytest.mark.parametrize("n_nodes", [0, 2000, 2001])
@pytest.mark.parametrize("fanout", [17, 33, 64])
def test_block_build_sampled_at_wide_fanouts(G, fanout, n_nodes):
    """block_insert_kernel<false, DIRECT> behind the F = 32 / 64 samplers; n_nodes = 2001 is odd (the table is rounded to 2002 entries so
    that the array behind it stays 8-byte aligned), 0 selects the hash table."""
    from glnn_amd import ops
    ns = 700
    seeds = np.random.RandomState(fanout).permutation(G.n)[:ns].astype(np.int64)
    assert so.table_direct(ns, ns * fanout, n_nodes) == (n_nodes > 0)
    smp, cnt = ops.sample_neighbors(G.tip, G.tix, _t(seeds), fanout, 77)
    smp_h, cnt_h = _np(smp), _np(cnt)
    want_src, want_cnt, _ = so.sample_neighbors(G.ip, G.ix, seeds, fanout, 77)
    assert np.array_equal(cnt_h, want_cnt) and (cnt_h == fanout).any() and (cnt_h < fanout).any()
    rows = [smp_h[i, :cnt_h[i]] for i in range(ns)]
    assert all(np.array_equal(r, want_src[i, :cnt_h[i]]) for i, r in enumerate(rows))
    got = ops.block_build(_t(seeds), smp_src=smp, smp_cnt=cnt, want_global=True, n_nodes=n_nodes)
    _check_block(got, seeds, rows)


def test_block_build_is_the_same_on_both_sides_of_the_direct_hash_switch(G):
    """n_nodes = 2 cap indexes the tables by the id, 2 cap + 1 hashes: identical blocks, and the hash build probes."""
    from glnn_amd import ops
    ns = 20
    seeds = np.random.RandomState(5).permutation(G.n)[:ns].astype(np.int64)
    rows = G.rows(seeds)
    nnz = sum(len(r) for r in rows)
    cap = sgo.table_cap(ns + nnz)
    assert 2 * cap >= G.n and so.table_direct(ns, nnz, 2 * cap) and not so.table_direct(ns, nnz, 2 * cap + 1)
    direct = ops.block_build(_t(seeds), G.tip, G.tix, nnz_cap=nnz, want_global=True, n_nodes=2 * cap)
    hashed = ops.block_build(_t(seeds), G.tip, G.tix, nnz_cap=nnz, want_global=True, n_nodes=2 * cap + 1)
    _, _, w_in = _check_block(direct, seeds, rows)
    _check_block(hashed, seeds, rows)
    assert all(torch.equal(a, b) for a, b in zip(direct[:4], hashed[:4])) and direct[4:] == hashed[4:]
    home = sgo.hash_slot(w_in, cap)
    assert len(np.unique(w_in)) == len(w_in) and len(np.unique(home)) < len(w_in)      # two frontier ids share a home slot: a probe happened


def test_out_of_range_ids_in_a_sampled_block_are_reported(G):
    """Direct mode: a sampled source equal to n_nodes, a sampled source of -1 and a seed equal to n_nodes are each reported (never used
    as an index); with an in-range id in the same place the same arrays build the oracle's block."""
    from glnn_amd import GlnnError, ops
    ns, fanout, n = 700, 17, G.n
    assert so.table_direct(ns, ns * fanout, n)
    perm = np.random.RandomState(8).permutation(n).astype(np.int64)
    seeds = perm[:ns]
    smp, cnt = ops.sample_neighbors(G.tip, G.tix, _t(seeds), fanout, 5)
    smp_h, cnt_h = _np(smp), _np(cnt)
    i = int(np.flatnonzero(cnt_h == fanout)[3])
    for where, bad, good in (("src", n, 7), ("src", -1, n - 1), ("seed", n, int(perm[ns + 1]))):
        for value in (bad, good):
            s, m = seeds.copy(), smp_h.copy()
            if where == "src":
                m[i, fanout - 1] = value
            else:
                s[i] = value
            if value == bad:
                with pytest.raises(GlnnError, match="outside"):
                    ops.block_build(_t(s), smp_src=_t(m), smp_cnt=cnt, want_global=True, n_nodes=n)
            else:
                got = ops.block_build(_t(s), smp_src=_t(m), smp_cnt=cnt, want_global=True, n_nodes=n)
                _check_block(got, s, [m[k, :cnt_h[k]] for k in range(ns)])


def test_out_of_range_ids_in_a_full_neighbour_block_are_reported(G):
    """The same three in full-neighbour mode.  The graph handed over has one more (empty) row than n_nodes, so that the row of the seed
    n_nodes exists: the builder reads a seed's row bounds before it looks the seed up."""
    from glnn_amd import GlnnError, ops
    ns, n = 20, G.n
    seeds = np.random.RandomState(5).permutation(n)[:ns].astype(np.int64)
    free = int(np.setdiff1d(np.arange(n), seeds)[11])
    ip = np.concatenate([G.ip, G.ip[-1:]])
    tip = _t(ip)
    cap = int(G.deg[seeds].sum() + G.deg[free]) + 3                              # (room for the row of the seed put in later)
    assert so.table_direct(ns, cap, n) and G.deg[seeds[4]] > 2
    at = int(G.ip[seeds[4]]) + 2                                                  # an entry in the row of the fifth seed
    for where, bad, good in (("src", n, 7), ("src", -1, n - 1), ("seed", n, free)):
        for value in (bad, good):
            s, x = seeds.copy(), G.ix.copy()
            if where == "src":
                x[at] = value
            else:
                s[4] = value
            if value == bad:
                with pytest.raises(GlnnError, match="outside"):
                    ops.block_build(_t(s), tip, _t(x), nnz_cap=cap, want_global=True, n_nodes=n)
            else:
                got = ops.block_build(_t(s), tip, _t(x), nnz_cap=cap, want_global=True, n_nodes=n)
                _check_block(got, s, [x[ip[v]:ip[v + 1]] for v in s])


def _raw_block(tip, tix, seeds, nnz_cap, n_nodes, global_only=False):
    """glnn_block_build_ids (full-neighbour mode) on sentinel-filled buffers of exactly the documented sizes followed by GUARD sentinel
    words each; returns the whole buffers, tails included."""
    from glnn_amd import _lib, ops
    h = _lib.lib()
    ns = seeds.numel()
    indptr = _full(ns + 1, WORD64, torch.int64)
    indices = _full(nnz_cap, WORD32, torch.int32)
    gindices = _full(nnz_cap, WORD32, torch.int32)
    input_nodes = _full(ns + nnz_cap, WORD64, torch.int64)
    counts = _full(2, WORD64, torch.int64)
    wsb = int(h.glnn_block_workspace_bytes(ns, nnz_cap))
    ws = _full((wsb + 7) // 8, WORD64, torch.int64)
    rc = h.glnn_block_build_ids(_p(tip), _p(tix), _p(seeds), ns, None, None, 0, nnz_cap, _p(indptr), None if global_only else _p(indices),
                                _p(gindices), None if global_only else _p(input_nodes), _p(counts), n_nodes, _p(ws), wsb, ops._stream())
    assert rc == 0, h.glnn_last_error()
    torch.cuda.synchronize()
    assert (counts[2:] == WORD64).all() and (ws[(wsb + 7) // 8:] == WORD64).all()
    return _np(indptr), _np(indices), _np(gindices), _np(input_nodes), counts[:2].tolist()


@pytest.fixture(scope="module")
def small_block():
    """300 nodes, 150 seeds: small enough that the id-indexed tables are chosen even at a capacity of one edge."""
    ip, ix = random_graph(300, 6, seed=3, hub=100)
    seeds = np.random.RandomState(4).permutation(300)[:150].astype(np.int64)
    rows = [ix[ip[v]:ip[v + 1]] for v in seeds]
    return ip, ix, seeds, rows, so.first_appearance_block(seeds, rows)


@pytest.mark.parametrize("form", ["hash", "direct", "global_only"])
def test_a_block_capacity_that_is_too_small_is_reported_never_written_past(small_block, form):
    """The guard e0 + k < nnz_cap of the full-neighbour passes: counts[0] is the TRUE edge count, and no word at or after the capacity
    is written in any output -- nor anything after indptr[ns]."""
    from glnn_amd import GlnnError, ops
    ip, ix, seeds, rows, (w_ip, w_ix, w_in) = small_block
    ns, nnz, n = len(seeds), int(w_ip[-1]), len(ip) - 1
    flat = np.concatenate(rows)
    tip, tix, tseeds = _t(ip), _t(ix), _t(seeds)
    n_nodes = 0 if form == "hash" else n
    glob = form == "global_only"
    for cap in (nnz - 1, nnz // 2, 1, nnz):
        assert so.table_direct(ns, cap, n_nodes) == (form != "hash")
        indptr, indices, gindices, input_nodes, counts = _raw_block(tip, tix, tseeds, cap, n_nodes, glob)
        assert counts[0] == nnz                                                   # the true count comes back
        assert np.array_equal(indptr[:ns + 1], w_ip) and (indptr[ns + 1:] == WORD64).all()
        assert (gindices[cap:] == WORD32).all() and np.array_equal(gindices[:cap], flat[:cap])
        assert (indices[cap:] == WORD32).all() and (input_nodes[ns + cap:] == WORD64).all()
        if glob:
            assert counts[1] == -1 and (indices == WORD32).all() and (input_nodes == WORD64).all()
        else:
            # what fits is what the full build holds there: first appearance is decided edge by edge, in order
            n_src = ns + len(np.unique(w_ix[:cap][w_ix[:cap] >= ns]))
            assert counts[1] == n_src and np.array_equal(indices[:cap], w_ix[:cap])
            assert np.array_equal(input_nodes[:n_src], w_in[:n_src]) and (input_nodes[n_src:] == WORD64).all()
        if cap < nnz:
            with pytest.raises(GlnnError, match="more than nnz_cap"):
                ops.block_build(tseeds, tip, tix, nnz_cap=cap, want_global=True, n_nodes=n_nodes, global_only=glob)


def test_capacity_zero_asserts_an_empty_block(small_block):
    """include/glnn_hip.h: nnz_cap == 0 with seeds is the caller's statement that the block has no edge -- no row is read: indptr is all
    zeros, input_nodes = the seeds, counts = {0, ns}, whatever in-edges the seeds have."""
    from glnn_amd import ops
    ip, ix, seeds, rows, (w_ip, _, _) = small_block
    ns = len(seeds)
    assert w_ip[-1] > 0
    for n_nodes in (0, len(ip) - 1):
        indptr, indices, gindices, input_nodes, counts = _raw_block(_t(ip), _t(ix), _t(seeds), 0, n_nodes)
        assert counts == [0, ns] and (indptr[:ns + 1] == 0).all() and (indptr[ns + 1:] == WORD64).all()
        assert np.array_equal(input_nodes[:ns], seeds) and (input_nodes[ns:] == WORD64).all()
        assert (indices == WORD32).all() and (gindices == WORD32).all()
    got = ops.block_build(_t(seeds), _t(ip), _t(ix), nnz_cap=0)
    assert got[4] == 0 and got[5] == ns and got[1].numel() == 0 and torch.equal(got[3], _t(seeds)) and not got[0].any()


# ------------------------------------------------------------------------------------------------ CSR transpose
def _check_transpose(got, want):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0]))
    assert torch.equal(got[1].cpu(), torch.from_numpy(want[1]))


@pytest.fixture(scope="module")
def sort_graph():
    ip, ix, planted = so.sort_path_graph()
    return ip, ix, planted, _t(ip), _t(ix)


def _assert_sort_classes(t_ip, t_ix, lengths):
    """Rows of each of `lengths` entries and a long row exist, with and without a value held twice."""
    length, tie = so.row_profile(t_ip, t_ix)
    for k in lengths:
        assert ((length == k) & ~tie).any(), k
        if k >= 2:
            assert ((length == k) & tie).any(), k
    assert ((length >= so.LONG_ROW) & tie).any() and ((length >= so.LONG_ROW) & ~tie).any()


@pytest.mark.parametrize("add_self", [False, True])
def test_transpose_sort_paths_with_tied_keys(sort_graph, add_self):
    """tr_sort_kernel: the register network (1..4 entries), the shuffle rank (5..64) and the quadratic rank (above 64), on rows at both
    ends of each range, each with and without tied keys.  add_self lengthens every row by one: the classes are asserted again."""
    from glnn_amd import ops
    ip, ix, planted, tip, tix = sort_graph
    n, nnz = len(ip) - 1, len(ix)
    want = so.csr_transpose(ip, ix, n, n, add_self)
    _assert_sort_classes(want[0], want[1], (1, 2, 3, 4, 5, 64, 65) if add_self else so.SORT_LENGTHS)
    got = ops.csr_transpose(tip, tix, n, n, nnz, add_self)
    _check_transpose(got, want)
    again = ops.csr_transpose(tip, tix, n, n, nnz, add_self)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("ns", [1024, 1000])
def test_transpose_of_a_sampled_block_with_self_entries(ns):
    """The form training uses: n_dst < n_src, add_self.  1024 destinations end on a scan tile's edge, 1000 inside a tile."""
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    n = 30000
    ip, ix = random_graph(n, 12, seed=9, power=0.6, hub=9000, isolated=50)
    tip, tix = _t(ip), _t(ix)
    seeds = _t(np.random.RandomState(ns).permutation(n)[:ns].astype(np.int64))
    smp, cnt = ops.sample_neighbors(tip, tix, seeds, 10, 4321)
    b_ip, b_ix, _, _, nnz, n_src = ops.block_build(seeds, smp_src=smp, smp_cnt=cnt, n_nodes=n)
    assert ns < n_src and n_src > 2 * 1024 and nnz > 2 * ns
    want = so.csr_transpose(_np(b_ip), _np(b_ix), ns, n_src, True)
    length = np.diff(want[0])
    assert (length[:ns] >= 1).all() and (length[ns:] >= 1).all() and length.min() == 1 and length.max() > 2
    _check_transpose(ops.csr_transpose(b_ip, b_ix, ns, n_src, nnz, True), want)
    t = CSRGraph(b_ip, b_ix, ns, n_src).transposed(add_self=True)
    assert t.n_dst == n_src and t.n_src == ns and t.num_edges() == nnz + ns
    _check_transpose((t.indptr, t.indices), want)


class _Large:
    """n_dst = 2^21 destinations of four in-edges each, sources uniform over n_src = 2^21 + 70: 2^23 edges."""
    n_dst, n_src = 1 << 21, (1 << 21) + 70

    def __init__(self):
        self.ip = np.arange(self.n_dst + 1, dtype=np.int64) * 4
        self.ix = np.random.RandomState(23).randint(0, self.n_src, size=4 * self.n_dst).astype(np.int32)
        self.tix = _t(self.ix)


@pytest.fixture(scope="module")
def large():
    return _Large()


@pytest.mark.parametrize("case", ["last_single_fill", "first_zero_fill", "zero_fill_through_self_entries"])
def test_transpose_at_the_fill_switch_and_over_the_capped_grids(large, case):
    """nnz_out = 2^23 - 1 is the last size whose cursors start from the workspace's one 0x7F fill, 2^23 the first with the separate zero
    fill (reached once by edges alone, once through add_self's entries).  At these sizes tr_count_kernel asks for more than 4096
    workgroups, tr_fill_kernel for more than 8192 and tr_sort_kernel for 8193: every stride loop makes a second trip."""
    from glnn_amd import ops
    n_dst, n_src, full = large.n_dst, large.n_src, 1 << 23
    add_self = case == "zero_fill_through_self_entries"
    nnz = {"last_single_fill": full - 1, "first_zero_fill": full, "zero_fill_through_self_entries": full - n_dst}[case]
    ip = np.minimum(large.ip, nnz)                                                # the first nnz edges: later rows are empty
    nnz_out = nnz + (n_dst if add_self else 0)
    assert nnz_out == (full - 1 if case == "last_single_fill" else full)
    assert (nnz + 255) // 256 > 4096 and (n_dst * 64 + 255) // 256 > 8192 and (n_src + 255) // 256 == 8193
    want = so.csr_transpose(ip, large.ix, n_dst, n_src, add_self)
    length = np.diff(want[0])
    assert 4 < length.max() <= 64 and (length <= 4).mean() > 0.5                  # both cheap sort paths, nothing for the quadratic one
    got = ops.csr_transpose(_t(ip), large.tix, n_dst, n_src, nnz, add_self)
    assert got[1].numel() == nnz_out
    _check_transpose(got, want)


# ------------------------------------------------------------------------------------------------ transpose with edge ids
def _check_eids(got, want):
    _check_transpose(got, want)
    assert got[2].dtype == torch.int32 and torch.equal(got[2].cpu(), torch.from_numpy(want[2]))


def test_transpose_eids_equals_the_lexsort_on_the_planted_graph(sort_graph):
    """Parallel edges u -> v keep ascending edge ids: three of them in a 5-entry row, three and two in the 700-entry row, two in the
    65-entry row (asserted from the oracle's rows)."""
    from glnn_amd import ops
    ip, ix, planted, tip, tix = sort_graph
    n, nnz = len(ip) - 1, len(ix)
    want = so.csr_transpose(ip, ix, n, n, False)
    dst = np.repeat(np.arange(n), np.diff(ip))
    assert np.array_equal(want[2], np.lexsort((np.arange(nnz), dst, ix)))
    row = lambda u: want[1][want[0][u]:want[0][u + 1]]
    assert np.bincount(row(planted[(5, True)])).max() == 3 and np.bincount(row(planted[(65, True)])).max() == 2
    c = np.bincount(row(planted[(so.LONG_ROW, True)]))
    assert (c == 3).sum() == 1 and (c == 2).sum() == 1
    _check_eids(ops.csr_transpose_eids(tip, tix, n, n, nnz), want)


def test_transpose_eids_rectangular_and_empty():
    from glnn_amd import ops
    n_dst, n_src = 500, 1300
    rs = np.random.RandomState(12)
    src, dst = rs.randint(0, n_src, 6000), rs.randint(0, n_dst, 6000)
    src[:400], dst[:400] = src[400:800], dst[400:800]                             # 400 parallel pairs
    src[800:900], dst[800:900] = n_src - 1, rs.randint(0, 40, 100)                # the last source: 100 entries over 40 destinations
    ip, ix = csr_from_edges(src, dst, n_dst)
    want = so.csr_transpose(ip, ix, n_dst, n_src, False)
    length, tie = so.row_profile(want[0], want[1])
    assert tie.sum() > 100 and length[n_src - 1] >= 100 and tie[n_src - 1]
    _check_eids(ops.csr_transpose_eids(_t(ip), _t(ix), n_dst, n_src, len(ix)), want)
    empty = ops.csr_transpose_eids(torch.zeros(n_dst + 1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                   n_dst, n_src, 0)
    assert empty[0].tolist() == [0] * (n_src + 1) and empty[1].numel() == 0 and empty[2].numel() == 0
