"""The numpy oracles of tests/sampling_oracle.py checked on their own (no GPU): the sampler's restatement draws distinct in-range
positions, uniformly, at every fan-out class the kernel is compiled for; the transpose oracle and the planted sort-path graph hold
what the GPU tests rely on.  tests/test_sampling_gpu.py then requires the kernels to equal these oracles bit for bit."""
import math

import numpy as np
import pytest

import sampling_oracle as so
from graphgen import random_graph


def test_chi2_quantile_against_known_values():
    """Textbook values: chi-square(1) exceeds 3.841 with probability 0.05, chi-square(10) exceeds 23.209 with 0.01; for 2 degrees of
    freedom the upper tail is exp(-x / 2) exactly."""
    assert abs(so.chi2_quantile(1, 0.05) - 3.8415) < 1e-3
    assert abs(so.chi2_quantile(10, 0.01) - 23.2093) < 1e-3
    assert abs(so.chi2_quantile(2, 1e-4) - (-2 * math.log(1e-4))) < 1e-8
    assert abs(so.chi2_quantile(38, 1e-4) - 80.0) < 1.5             # the bound test_teacher_gpu.py states for 38 degrees of freedom


@pytest.mark.parametrize("deg,fanout", [(2, 1), (9, 8), (17, 16), (33, 32), (65, 64), (983, 64), (40, 10), (1000, 1)])
def test_picked_positions_are_distinct_and_in_range(deg, fanout):
    rows = 500
    picked, redirected = so.floyd_positions(np.full(rows, deg), fanout, 99, np.arange(rows))
    assert picked.shape == (rows, fanout) and picked.min() >= 0 and picked.max() < deg
    assert all(len(np.unique(p)) == fanout for p in picked)
    if deg == fanout + 1 and fanout >= 7:
        assert redirected.any()                                       # (nearly every row redirects: the last draw is U[0, deg) over one free slot)
    # a redirected pick is the j of its step
    s = np.arange(fanout)[None, :]
    assert (picked[redirected] == (deg - fanout + s).repeat(rows, 0)[redirected]).all()


@pytest.mark.parametrize("deg,fanout", [(40, 10), (40, 33), (65, 64), (200, 64)])
def test_inclusion_is_uniform(deg, fanout):
    """One row, 10^4 draws keyed by the seed index, seed 20240917: every position is included with probability fanout / deg.  Measured:
    42.9, 25.9, 39.4, 193.6 for the four cases; the bound is the chi-square quantile at 1 - 1e-4 for deg - 1 degrees of freedom.  The
    cases put fan-outs on the 16-, 64- (33 and 64) wide instantiations; with the bit-for-bit GPU test the check holds for every F."""
    draws = 10000
    picked, _ = so.floyd_positions(np.full(draws, deg), fanout, 20240917, np.arange(draws))
    counts = np.bincount(picked.ravel(), minlength=deg)
    assert counts.sum() == draws * fanout
    stat = so.inclusion_statistic(counts, draws, fanout)
    bound = so.chi2_quantile(deg - 1, 1e-4)
    print(f"deg {deg} fanout {fanout}: statistic {stat:.1f}, bound {bound:.1f}")
    assert stat < bound, (stat, bound)


def test_sample_neighbors_row_classes_on_a_small_graph():
    indptr, indices = random_graph(300, 6, seed=2, isolated=10, hub=90)
    seeds = np.random.RandomState(1).permutation(300)
    deg = np.diff(indptr)[seeds]
    fanout = 6
    assert (deg == 0).any() and (deg == fanout).any() and (deg == fanout + 1).any() and (deg > 64).any()
    src, cnt, n_red = so.sample_neighbors(indptr, indices, seeds, fanout, 5)
    assert np.array_equal(cnt, np.minimum(deg, fanout)) and n_red > 0
    for i, v in enumerate(seeds):
        pool = indices[indptr[v]:indptr[v + 1]]
        if deg[i] <= fanout:
            assert np.array_equal(src[i, :cnt[i]], pool)                  # kept whole, in row order
        else:
            avail = pool.tolist()
            for u in src[i]:
                avail.remove(int(u))                                      # a sub-multiset of the row: without replacement
        assert (src[i, cnt[i]:] == so.NO_ENTRY).all()
    # keyed by the seed's index: the same node at two places of the list draws differently, the same list the same
    twice = np.concatenate([seeds, seeds])
    src2, _, _ = so.sample_neighbors(indptr, indices, twice, fanout, 5)
    big = np.flatnonzero(deg > 3 * fanout)
    assert np.array_equal(src2[:300], src) and not np.array_equal(src2[300:][big], src[big])


def test_first_appearance_block_by_hand():
    ip, ix, inp = so.first_appearance_block([7, 3], [[9, 3, 9, 4], [], ])
    assert ip.tolist() == [0, 4, 4] and ix.tolist() == [2, 1, 2, 3] and inp.tolist() == [7, 3, 9, 4]
    assert so.table_direct(10, 22, 128) and not so.table_direct(10, 22, 129) and not so.table_direct(10, 22, 0)


def test_transpose_oracle_by_hand_and_against_lexsort():
    # 3 destinations, 6 sources (the hand case of test_teacher_gpu.py): rows 0: [4, 1]  1: []  2: [5, 5, 0]
    indptr = np.array([0, 2, 2, 5], np.int64)
    indices = np.array([4, 1, 5, 5, 0], np.int32)
    t_ip, t_ix, t_e = so.csr_transpose(indptr, indices, 3, 6, False)
    assert t_ip.tolist() == [0, 1, 2, 2, 2, 3, 5] and t_ix.tolist() == [2, 0, 0, 2, 2] and t_e.tolist() == [4, 1, 0, 2, 3]
    t_ip, t_ix, t_e = so.csr_transpose(indptr, indices, 3, 6, True)
    assert t_ip.tolist() == [0, 2, 4, 5, 5, 6, 8] and t_ix.tolist() == [0, 2, 0, 1, 2, 0, 2, 2] and t_e is None
    ip, ix = random_graph(200, 5, seed=4, hub=150)
    dst = np.repeat(np.arange(200), np.diff(ip))
    t_ip, t_ix, t_e = so.csr_transpose(ip, ix, 200, 200, False)
    assert np.array_equal(t_e, np.lexsort((np.arange(len(ix)), dst, ix)))
    assert np.array_equal(t_ix, dst[t_e]) and np.array_equal(ix[t_e], np.repeat(np.arange(200), np.diff(t_ip)))


def test_sort_path_graph_has_the_planted_rows():
    indptr, indices, planted = so.sort_path_graph()
    n = len(indptr) - 1
    t_ip, t_ix, _ = so.csr_transpose(indptr, indices, n, n, False)
    length, tie = so.row_profile(t_ip, t_ix)
    for (k, tied), u in planted.items():
        assert length[u] == (1 if k == "loop" else k) and bool(tie[u]) == tied
    loop = planted[("loop", False)]
    assert t_ix[t_ip[loop]] == loop
    row = lambda u: t_ix[t_ip[u]:t_ip[u + 1]]
    assert np.bincount(row(planted[(5, True)])).max() == 3                        # three parallel edges in a row shorter than 64
    c = np.bincount(row(planted[(so.LONG_ROW, True)]))
    assert (c == 3).sum() == 1 and (c == 2).sum() == 1                            # three and two in a row longer than 64
    assert np.bincount(row(planted[(65, True)])).max() == 2
