"""CPU-side checks of the node2vec pieces of the position features (docs/POSITION_SEMANTICS.md): the numpy oracle
(tests/node2vec_oracle.py) against the uniform walk it must equal at p = q = 1, against node2vec's exact step distribution, against hand
answers for the CDF draw and against torch autograd + SparseAdam over two tables in fp64; the quality of what it trains (the condition the
GPU functional test rests on); the C-ABI agreement and refusals of the new entry points (no launch: they return before one); the student's
new command-line flags.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deepwalk_oracle as dwo
import node2vec_oracle as nvo
from deepwalk_cases import BETAS, EPS, init_embedding, step_seeds
from graphgen import csr_from_edges, random_graph
from node2vec_cases import QUALITY, quality_lists
from oracle.dropout_mask import drop_hash
from subgraph_oracle import random_walk, six_node_graph


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("graph", ["six", "random", "symmetric"])
def test_oracle_walk_at_p_q_one_is_the_uniform_walk(graph):
    if graph == "six":
        indptr, indices = six_node_graph()
    else:
        indptr, indices = random_graph(60, 4, seed=3, isolated=5, symmetric=graph == "symmetric")
    roots = np.arange(len(indptr) - 1).repeat(2)
    for length in (1, 2, 64):
        assert np.array_equal(nvo.node2vec_walk(indptr, indices, roots, length, 1.0, 1.0, 77), random_walk(indptr, indices, roots, length, 77))


def test_thresholds_by_hand():
    """wmax is the largest weight and gets exactly 2^32 (always accepted, no draw); the others floor(w / wmax * 2^32)."""
    assert nvo.thresholds(1.0, 1.0) == (2 ** 32, 2 ** 32, 2 ** 32)
    assert nvo.thresholds(0.25, 4.0) == (2 ** 32, 2 ** 30, 2 ** 28)              # weights 4, 1, 1/4
    assert nvo.thresholds(4.0, 0.25) == (2 ** 28, 2 ** 30, 2 ** 32)
    assert nvo.thresholds(2.0, 1.0) == (2 ** 31, 2 ** 32, 2 ** 32)
    assert nvo.thresholds(1.0, 3.0) == (2 ** 32, 2 ** 32, int(np.floor(1.0 / 3.0 * 2.0 ** 32)))


def three_class_graph():
    """Symmetric, 5 nodes: 0-1, 0-2, 1-2, 1-3, 1-4, 2-3.  Rows: 0: [1, 2]  1: [0, 2, 3, 4]  2: [0, 1, 3]  3: [1, 2]  4: [1].  In the state
    (t, v) = (0, 1) the candidates of row 1 are 0 (return), 2 (near: 2 is in row 0), 3 and 4 (far)."""
    und = [(0, 1), (0, 2), (1, 2), (1, 3), (1, 4), (2, 3)]
    src = np.array([a for a, _ in und] + [b for _, b in und])
    dst = np.array([b for _, b in und] + [a for a, _ in und])
    return csr_from_edges(src, dst, 5)


@pytest.mark.parametrize("p, q", [(0.25, 4.0), (4.0, 0.25)])
def test_oracle_walk_follows_the_exact_node2vec_distribution(p, q):
    """4e5 walks of length 2 from root 0, seed 2 (fixed: the outcome is fixed); over the ~2e5 with walk[1] == 1 the empirical distribution of
    step 2 sits within 5 standard errors sqrt(pi (1 - pi) / M) of (1/p, 1, 1/q, 1/q) / sum per candidate.  Measured: the largest deviation
    is 0.85 standard errors at (0.25, 4) and 1.04 at (4, 0.25)."""
    indptr, indices = three_class_graph()
    want = nvo.step_probabilities(indptr, indices, 0, 1, p, q)
    w = np.array([1 / p, 1.0, 1 / q, 1 / q])
    assert sorted(want) == [0, 2, 3, 4] and np.allclose([want[x] for x in (0, 2, 3, 4)], w / w.sum(), rtol=1e-15)
    walks = nvo.node2vec_walk(indptr, indices, np.zeros(400000, np.int64), 2, p, q, 2)
    sel = walks[walks[:, 1] == 1]
    m = len(sel)
    assert m >= 190000
    for x, pi in want.items():
        dev = (np.mean(sel[:, 2] == x) - pi) / np.sqrt(pi * (1 - pi) / m)
        print(f"p={p} q={q} candidate {x}: exact {pi:.5f}, {dev:+.2f} standard errors over {m} walks")
        assert abs(dev) <= 5.0, (x, dev)


def test_oracle_walk_on_a_non_symmetric_graph_uses_the_stored_rows():
    """Six-node graph, rows 0: [1, 1, 2]  1: [0, 3]  2: [2, 1, 4]  3: [2]  4: []  5: [].  From t = 0 on v = 1: 0 is the return, 3 is FAR (3 is
    not an entry of row 0, whatever row 3 holds).  From t = 2 on v = 2 (the self-loop): 2 is the return, 1 is near (row 2 holds 1), 4 too."""
    indptr, indices = six_node_graph()
    assert nvo.step_probabilities(indptr, indices, 0, 1, 0.5, 4.0) == {0: 2.0 / 2.25, 3: 0.25 / 2.25}
    assert nvo.step_probabilities(indptr, indices, 2, 2, 0.5, 4.0) == {2: 0.5, 1: 0.25, 4: 0.25}
    walks = nvo.node2vec_walk(indptr, indices, [5, 4, 3, 0, 2], 6, 0.5, 4.0, 3)
    assert walks[0].tolist() == [5] * 7 and walks[1].tolist() == [4] * 7 and walks[2, 1] == 2
    rows = [[1, 1, 2], [0, 3], [2, 1, 4], [2], [], []]
    for i in range(5):
        for s in range(1, 7):
            assert int(walks[i, s]) in (rows[int(walks[i, s - 1])] or [int(walks[i, s - 1])])


# ------------------------------------------------------------------------------------------------ the CDF
def test_oracle_cdf_and_draws_on_the_six_node_graph_by_hand():
    """Out-degrees (occurrences in `indices` = [1, 1, 2, 0, 3, 2, 1, 4, 2]): 1, 3, 3, 1, 1, 0.  power 1: cumulative 1, 4, 7, 8, 9, 9 of 9."""
    indptr, indices = six_node_graph()
    cdf = nvo.negative_cdf(indptr, indices, 1.0)
    assert cdf.tolist() == [2 ** 32 * k // 9 for k in (1, 4, 7, 8)] + [2 ** 32 - 1, 2 ** 32 - 1]
    r = np.array([0, cdf[0] - 1, cdf[0], cdf[1] - 1, cdf[1], cdf[3], 2 ** 32 - 2, 2 ** 32 - 1])
    assert nvo.draw_from_cdf(cdf, r).tolist() == [0, 0, 1, 1, 2, 4, 4, 5]          # (the last: the 2^-32 artefact on the trailing zero-weight node)
    assert nvo.draw_from_cdf(np.array([7]), np.array([0, 7, 2 ** 32 - 1])).tolist() == [0, 0, 0]      # one node: always node 0
    assert nvo.draw_from_cdf(np.full(4, 2 ** 32 - 1), np.array([0, 2 ** 32 - 2, 2 ** 32 - 1])).tolist() == [0, 0, 3]
    assert nvo.draw_from_cdf(np.array([0, 0, 5, 9]), np.array([0, 4, 5, 9])).tolist() == [2, 2, 3, 3]
    # power 0.75 through the pair list: negatives are the CDF draws of drop_hash(neg_seed, q, t')
    cdf = nvo.negative_cdf(indptr, indices, 0.75)
    walks = random_walk(indptr, indices, [0, 3], 3, 11)
    start, rest = nvo.pairs_from_walks(walks, 6, 3, 2, 77, cdf)
    assert start.tolist() == walks[:, :2].reshape(-1).tolist()
    for qq in range(4):
        for t in range(4):
            assert rest[qq, 2 + t] == int(np.searchsorted(cdf[:5], int(drop_hash(77, qq, t)), side="right"))
    # without a CDF and with the uniform walk: the one-table oracle's lists
    _, s1, r1 = dwo.pairs(indptr, indices, [0, 3], 3, 3, 2, 11, 77)
    s2, r2 = nvo.pairs_from_walks(walks, 6, 3, 2, 77)
    assert np.array_equal(s1, s2) and np.array_equal(r1, r2)


def test_cdf_never_draws_a_node_of_degree_zero_and_follows_the_weights():
    """60-node random graph with 5 nodes that never occur as a source; 1e5 draws at power 0.75: none of them is drawn, and every other
    node's frequency sits within 5 standard errors of deg^0.75 / sum (measured: at most 3.4 over the 55 nodes)."""
    indptr, indices = random_graph(60, 4, seed=3)
    src_free = np.array([7, 19, 33, 48, 59])
    keep = ~np.isin(indices, src_free)
    dst = np.repeat(np.arange(60), np.diff(indptr))[keep]
    indptr, indices = csr_from_edges(indices[keep], dst, 60)
    deg = np.bincount(indices, minlength=60).astype(np.float64)
    assert (deg[src_free] == 0).all() and deg[-1] == 0                       # (a trailing zero-weight node: the 2^-32 artefact's place)
    cdf = nvo.negative_cdf(indptr, indices, 0.75)
    m = 100000
    draws = nvo.draw_from_cdf(cdf, drop_hash(5, np.arange(m), 0))
    cnt = np.bincount(draws, minlength=60)
    assert cnt[src_free].sum() == 0
    pi = deg ** 0.75 / (deg ** 0.75).sum()
    live = deg > 0
    dev = (cnt[live] / m - pi[live]) / np.sqrt(pi[live] * (1 - pi[live]) / m)
    print(f"largest deviation {np.abs(dev).max():.2f} standard errors")
    assert np.abs(dev).max() <= 5.0
    from glnn_amd.position import negative_cdf
    assert np.array_equal(negative_cdf(indices, 60, 0.75), cdf)              # the host side builds the same table
    with pytest.raises(ValueError, match="weight 0"):
        negative_cdf(np.zeros(0, np.int32), 4, 0.75)


# ------------------------------------------------------------------------------------------------ two tables against torch
def _torch_loss(emb, ctx, start, rest, context):
    za = emb(torch.as_tensor(start))
    cx = ctx(torch.as_tensor(rest))
    s = (za[:, None, :] * cx).sum(dim=2)
    return F.softplus(-s[:, :context - 1]).mean() + F.softplus(s[:, context - 1:]).mean()


@pytest.mark.parametrize("case", ["six", "random"])
def test_two_table_gradient_and_three_steps_equal_torch_sparse_adam_in_fp64(case):
    if case == "six":
        indptr, indices = six_node_graph()
        roots, length, context, negatives = np.array([5, 0, 3, 0, 2]), 4, 3, 2
    else:
        indptr, indices = random_graph(60, 4, seed=3, isolated=5)
        roots, length, context, negatives = np.arange(0, 60, 7), 6, 4, 1
    n, d, lr = len(indptr) - 1, 8, 0.05
    cdf = nvo.negative_cdf(indptr, indices, 0.75)
    rng = np.random.default_rng(0)
    z0, c0 = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    emb, ctx = torch.nn.Embedding(n, d, sparse=True).double(), torch.nn.Embedding(n, d, sparse=True).double()
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(z0))
        ctx.weight.copy_(torch.from_numpy(c0))
    opt = torch.optim.SparseAdam(list(emb.parameters()) + list(ctx.parameters()), lr=lr, betas=BETAS, eps=EPS)
    state = (z0.copy(), np.zeros_like(z0), np.zeros_like(z0), c0.copy(), np.zeros_like(z0), np.zeros_like(z0))

    def rel(a, b):
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)

    for t in (1, 2, 3):
        walks = nvo.node2vec_walk(indptr, indices, roots, length, 0.5, 2.0, 100 + t)
        start, rest = nvo.pairs_from_walks(walks, n, context, negatives, 200 + t, cdf)
        loss, dz, dc, tz, tc = nvo.loss_and_grad(state[0], state[3], start, rest, context, negatives)
        before = (emb.weight.detach().numpy().copy(), ctx.weight.detach().numpy().copy())
        opt.zero_grad()
        tl = _torch_loss(emb, ctx, start, rest, context)
        tl.backward()
        gz, gc = emb.weight.grad.coalesce(), ctx.weight.grad.coalesce()
        assert abs(loss - tl.item()) <= 1e-12 * abs(tl.item())
        assert rel(dz, gz.to_dense().numpy()) <= 1e-12 and rel(dc, gc.to_dense().numpy()) <= 1e-12
        assert sorted(set(gz.indices()[0].tolist())) == np.flatnonzero(tz).tolist()          # the starts alone
        assert sorted(set(gc.indices()[0].tolist())) == np.flatnonzero(tc).tolist()          # the entries alone
        opt.step()
        new, loss2, tz2, tc2 = nvo.step(state, indptr, indices, roots, length, context, negatives, 100 + t, 200 + t, lr, BETAS, EPS, t,
                                        p=0.5, q=2.0, cdf=cdf)
        assert loss2 == loss and np.array_equal(tz2, tz) and np.array_equal(tc2, tc)
        for k, (mod, touched) in enumerate(((emb, tz), (ctx, tc))):
            st = opt.state[mod.weight]
            w = mod.weight.detach().numpy()
            assert rel(new[3 * k], w) <= 1e-12 and rel(new[3 * k + 1], st["exp_avg"].numpy()) <= 1e-12
            assert rel(new[3 * k + 2], st["exp_avg_sq"].numpy()) <= 1e-12
            assert np.array_equal(w[~touched], before[k][~touched]) and np.array_equal(new[3 * k][~touched], state[3 * k][~touched])
        assert ((~tz).any() and (~tc).any()) or case == "six"
        state = new


def test_tied_tables_reproduce_the_one_table_oracle_exactly():
    indptr, indices = random_graph(60, 4, seed=3, isolated=5)
    roots, length, context, negatives, lr = np.arange(0, 60, 7), 6, 4, 1, 0.05
    z0 = np.random.default_rng(0).standard_normal((60, 8))
    for dtype in (np.float64, np.float32):
        one = (z0.astype(dtype), np.zeros((60, 8), dtype), np.zeros((60, 8), dtype))
        two = one + (None, None, None)
        for t in (1, 2, 3):
            z, m, v, loss, touched = dwo.step(*one, indptr, indices, roots, length, context, negatives, 10 + t, 20 + t, lr, BETAS, EPS, t, dtype)
            two, loss2, tz, tc = nvo.step(two, indptr, indices, roots, length, context, negatives, 10 + t, 20 + t, lr, BETAS, EPS, t,
                                          dtype=dtype, tied=True)
            one = (z, m, v)
            assert loss2 == loss and np.array_equal(tz, touched) and np.array_equal(tc, touched)
            assert all(np.array_equal(a, b) for a, b in zip(one, two[:3]))


# ------------------------------------------------------------------------------------------------ quality of the oracle alone
def test_oracle_node2vec_embedding_separates_the_planted_communities():
    """What the GPU functional test rests on.  The 512-node planted-community case of the one-table quality test with (p, q) = (0.5, 2),
    power 0.75 and a context table, its other settings unchanged (d = 16, L = 10, c = 5, k = 1, lr = 0.05, 100 steps): the fp64 oracle
    reaches a nearest-class-centroid accuracy of 0.9961, 0.9961, 0.9961, 0.9941 for the init seeds 0-3 (fp32: the same four values), the
    loss falling from 3.45 to 0.72.  All four are at least 0.97, so the bar of 0.95 holds here and on the device."""
    indptr, indices, labels, c, lists = quality_lists()
    for seed in range(4):
        z = init_embedding(512, c["d"], seed).astype(np.float64)
        ctx = init_embedding(512, c["d"], seed + 1).astype(np.float64)
        st = (z, np.zeros_like(z), np.zeros_like(z), ctx, np.zeros_like(z), np.zeros_like(z))
        losses = []
        for s, (start, rest) in enumerate(lists):
            loss, dz, dc, tz, tc = nvo.loss_and_grad(st[0], st[3], start, rest, c["context"], c["negatives"])
            st = dwo.lazy_adam(st[0], st[1], st[2], dz, tz, c["lr"], BETAS, EPS, s + 1) + \
                dwo.lazy_adam(st[3], st[4], st[5], dc, tc, c["lr"], BETAS, EPS, s + 1)
            losses.append(float(loss))
        acc = dwo.centroid_accuracy(st[0], labels)
        print(f"seed {seed}: accuracy {acc:.4f}, loss {losses[0]:.3f} -> {losses[-1]:.3f}")
        assert acc >= 0.97, (seed, acc)              # the condition under which the bar below may be asserted at all
        assert acc >= QUALITY["bar"]
        assert losses[-1] < 0.5 * losses[0]


# ------------------------------------------------------------------------------------------------ C ABI
NEW = ("glnn_node2vec_walk", "glnn_deepwalk_pairs_from_walks", "glnn_deepwalk_score_ctx_f32")


def _h():
    from glnn_amd import _lib
    return _lib.lib()


def test_new_entries_are_bound_and_the_abi_version_is_unchanged():
    from glnn_amd import _lib, ops
    h = _h()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.glnn_abi_version() == 12
    assert callable(ops.node2vec_walk) and callable(ops.deepwalk_pairs_from_walks)


def _walk_rc(h, n_nodes=6, n_roots=4, length=4, p=1.0, q=1.0, roots_host=None):
    return h.glnn_node2vec_walk(None, None, n_nodes, None, roots_host, n_roots, length, p, q, 1, None, None)


@pytest.mark.parametrize("kw, needle", [
    (dict(p=0.2), b"p and q must be in [0.25, 4]"), (dict(p=4.5), b"p and q"), (dict(q=0.0), b"p and q"), (dict(q=5.0), b"p and q"),
    (dict(p=float("nan")), b"p and q"), (dict(length=0), b"walk length"), (dict(length=65), b"walk length"), (dict(n_nodes=2 ** 31), b"N < 2^31"),
    (dict(), b"null pointer"),
])
def test_walk_refuses_bad_arguments_before_any_pointer_is_used(kw, needle):
    h = _h()
    assert _walk_rc(h, **kw) == -1 and needle in h.glnn_last_error()


def test_walk_refuses_a_root_outside_the_graph_and_takes_an_empty_batch():
    h = _h()
    bad = (ctypes.c_int64 * 4)(0, 5, 6, 1)
    one = ctypes.c_int64(0)
    ptr = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)       # non-NULL stand-ins: the refusal comes before any of them is used
    rc = h.glnn_node2vec_walk(ptr, ptr, 6, ptr, ctypes.cast(bad, ctypes.c_void_p), 4, 4, 0.5, 2.0, 1, ptr, None)
    assert rc == -1 and b"root 6 (position 2) is outside the graph of 6 nodes" in h.glnn_last_error()
    assert _walk_rc(h, n_roots=0) == 0


def test_pairs_from_walks_and_score_ctx_refuse_bad_shapes_and_null_pointers():
    h = _h()

    def pairs_rc(n_nodes=6, n_roots=4, length=4, context=3, negatives=1):
        return h.glnn_deepwalk_pairs_from_walks(None, n_roots, length, context, negatives, n_nodes, 2, None, None, None, None, None, None)

    for kw, needle in ((dict(context=1), b"context size"), (dict(context=6), b"context size"), (dict(negatives=0), b"negatives per positive"),
                       (dict(length=65), b"walk length"), (dict(n_nodes=0), b"N < 2^31"), (dict(n_roots=2 ** 26, length=64, context=2), b"Q R < 2^31"),
                       (dict(), b"null pointer")):
        assert pairs_rc(**kw) == -1 and needle in h.glnn_last_error(), kw

    def score_rc(n_nodes=6, d=8, q=4, context=3, negatives=1):
        return h.glnn_deepwalk_score_ctx_f32(None, None, n_nodes, d, None, None, q, context, negatives, None, None, None, None, None)

    for kw, needle in ((dict(d=6), b"multiple of 4"), (dict(d=260), b"multiple of 4"), (dict(context=1), b"context size"), (dict(), b"null pointer")):
        assert score_rc(**kw) == -1 and needle in h.glnn_last_error(), kw
    assert b"glnn_deepwalk_score_ctx_f32" in h.glnn_last_error()
    assert score_rc(q=0) == 0


def test_wrappers_refuse_cpu_tensors_and_the_class_checks_its_arguments():
    from glnn_amd import GlnnError, ops
    from glnn_amd.graph import CSRGraph
    from glnn_amd.position import DeepWalk
    indptr, indices = six_node_graph()
    with pytest.raises(GlnnError):
        ops.node2vec_walk(torch.from_numpy(indptr), torch.from_numpy(indices), torch.arange(3), 4, 0.5, 2.0, 1)
    with pytest.raises(GlnnError):
        ops.deepwalk_pairs_from_walks(torch.zeros((2, 5), dtype=torch.int64), 6, 3, 1, 2)
    with pytest.raises(GlnnError):
        ops.deepwalk_score(torch.zeros(6, 8), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32), 3, 1, ctx=torch.zeros(6, 8))
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        DeepWalk(CSRGraph(torch.from_numpy(indptr), torch.from_numpy(indices), 6), 8, p=0.5, q=2.0, negative_power=0.75, context_table=True)
    words = ops.deepwalk_cdf_words(np.array([0, 5, 2 ** 31, 2 ** 32 - 1]), "cpu")
    assert words.dtype == torch.int32 and words.tolist() == [0, 5, -2 ** 31, -1]          # the same 32 bits, read as uint32 by the kernel
    with pytest.raises(ValueError):
        ops.deepwalk_cdf_words(np.array([2 ** 32]), "cpu")


# ------------------------------------------------------------------------------------------------ flags
def _args(*extra):
    from glnn_amd.cli import get_student_args
    return get_student_args(["--dataset", "synthetic-cora"] + list(extra))


def test_node2vec_flags_default_to_off_and_are_parsed():
    a = _args()
    assert (a.position_p, a.position_q, a.position_negative_power, a.position_context_table) == (1.0, 1.0, 0.0, False)
    a = _args("--position_dim", "16", "--position_p", "0.5", "--position_q", "2", "--position_negative_power", "0.75", "--position_context_table")
    assert (a.position_dim, a.position_p, a.position_q, a.position_negative_power, a.position_context_table) == (16, 0.5, 2.0, 0.75, True)


@pytest.mark.parametrize("extra", [("--position_p", "0.2"), ("--position_p", "4.5"), ("--position_q", "0.1"), ("--position_q", "8"),
                                   ("--position_negative_power", "-0.5"), ("--position_p", "nan")])
def test_node2vec_flags_are_checked_by_the_parser(extra):
    with pytest.raises(SystemExit):
        _args("--position_dim", "8", *extra)
