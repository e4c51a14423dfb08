"""GPU checks of the node2vec pieces of the position features (csrc/node2vec.hip, csrc/deepwalk.hip, glnn_amd/position.py;
docs/POSITION_SEMANTICS.md) against the numpy oracle tests/node2vec_oracle.py: the biased walk bit for bit (rows of at most 64, of 65 to
256 and of more than 256 entries, multi-edges, self-loops, an isolated root, a non-symmetric graph), its identity with the uniform walk at
p = q = 1, the pair lists with and without a CDF bit for bit, the context score with the embedding as its own context bit for bit, three
two-table optimiser steps within ten times the oracle's own fp32-against-fp64 error with untouched rows bit for bit, the default path's
bits, the quality of the embedding, and every refusal."""
import re

import numpy as np
import pytest
import torch

import deepwalk_oracle as dwo
import node2vec_oracle as nvo
from deepwalk_cases import BETAS, EPS, clustered_case, init_embedding, step_seeds
from graphgen import csr_from_edges, random_graph
from node2vec_cases import QUALITY
from subgraph_oracle import six_node_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PQ = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.25), (2.0, 1.0), (1.0, 2.0)]


def mixed_graph(symmetric):
    """300 nodes: random_graph's hub row (290 extra in-edges: more than 256 entries) and 4 rows without in-edges, then a row of about 100
    entries (two rounds of the wave's scan), 20 stored edges doubled (multi-edges) and 10 self-loops.  symmetric: every added edge both ways
    (the rows without in-edges still occur as sources: only that part is one-way)."""
    indptr, indices = random_graph(300, 4, seed=7, symmetric=symmetric, isolated=4, hub=290)
    deg = np.diff(indptr)
    dst = np.repeat(np.arange(300), deg)
    src = indices.astype(np.int64)
    rs = np.random.RandomState(11)
    mid = int(np.flatnonzero((deg > 0) & (deg < 30))[5])
    add_src, add_dst = rs.randint(0, 300, size=100), np.full(100, mid)
    if symmetric:
        live = deg[add_src] > 0                                           # (keep the rows without in-edges without in-edges)
        add_src, add_dst = np.concatenate([add_src, add_dst[live]]), np.concatenate([add_dst, add_src[live]])
    dup = rs.choice(len(src), size=20, replace=False)
    loops = np.flatnonzero(deg > 0)[::25][:10]
    src = np.concatenate([src, add_src, src[dup], loops])
    dst = np.concatenate([dst, add_dst, dst[dup], loops])
    return csr_from_edges(src, dst, 300)


def star_graph(n=300):
    """Hub 0 and n - 1 leaves, both directions stored: row 0 = [1 .. n - 1], row i = [0]."""
    indptr = np.concatenate([[0], n - 1 + np.arange(n)]).astype(np.int64)
    return indptr, np.concatenate([np.arange(1, n), np.zeros(n - 1)]).astype(np.int32)


def dev_graph(indptr, indices):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV), len(indptr) - 1)


GRAPHS = {"six": six_node_graph, "mixed": lambda: mixed_graph(True), "mixed_oneway": lambda: mixed_graph(False), "star": star_graph,
          "clustered": lambda: clustered_case()[:2]}
_G = {}


def graph(name):
    if name not in _G:
        indptr, indices = GRAPHS[name]()
        _G[name] = (indptr, indices, dev_graph(indptr, indices))
    return _G[name]


def roots_for(indptr, n_roots):
    """Repeated roots in every case but B = 1; from B = 63 on the last root is a node without in-edges where the graph has one."""
    n = len(indptr) - 1
    roots = (np.arange(n_roots) * 5 + n - 1) % n
    roots[n_roots // 2:] = roots[:n_roots - n_roots // 2]
    empty = np.flatnonzero(np.diff(indptr) == 0)
    if n_roots > 1 and len(empty):
        roots[-1] = empty[0]
    return roots.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("symmetric", [True, False])
def test_mixed_graph_has_the_rows_the_walk_kernel_branches_on(symmetric):
    indptr, indices = mixed_graph(symmetric)
    deg = np.diff(indptr)
    dst = np.repeat(np.arange(300), deg)
    assert deg.max() > 256 and ((deg >= 65) & (deg <= 256)).any() and (deg == 0).sum() >= 4 and ((deg > 0) & (deg <= 64)).any()
    key = dst * 300 + indices
    assert len(np.unique(key)) < len(key) - 20 + 1 and (indices == dst).sum() >= 10          # multi-edges, self-loops
    back = np.isin(indices.astype(np.int64) * 300 + dst, key)                                  # is the reverse edge stored?
    assert (back.mean() > 0.95) == symmetric


@pytest.mark.parametrize("pq", PQ)
@pytest.mark.parametrize("name", ["six", "mixed", "mixed_oneway"])
def test_walk_equals_the_oracle_bit_for_bit(name, pq):
    """length in {1, 2, 64} x n_roots in {1, 63, 257}; at (1, 1) also the uniform walk's bits; two runs give the same bits."""
    from glnn_amd import ops
    indptr, indices, g = graph(name)
    p, q = pq
    for length in (1, 2, 64):
        for n_roots in (1, 63, 257):
            roots = roots_for(indptr, n_roots)
            want = nvo.node2vec_walk(indptr, indices, roots, length, p, q, 123)
            r = torch.from_numpy(roots)
            got = ops.node2vec_walk(g.indptr, g.indices, r, length, p, q, 123)
            assert got.dtype == torch.int64 and tuple(got.shape) == (n_roots, length + 1)
            assert np.array_equal(got.cpu().numpy(), want), (length, n_roots)
            again = ops.node2vec_walk(g.indptr, g.indices, r.to(DEV), length, p, q, 123)      # (roots on the device: one copy back for the check)
            assert torch.equal(got, again)
            if pq == (1.0, 1.0):
                assert torch.equal(got, ops.random_walk(g.indptr, g.indices, r.to(DEV), length, 123))
    if pq != (1.0, 1.0) and name != "six":                                 # the bias is at work: not the uniform walk
        assert not np.array_equal(want, nvo.node2vec_walk(indptr, indices, roots, 64, 1.0, 1.0, 123))


# ------------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("lck", [(1, 2, 1), (4, 3, 2), (10, 5, 1), (64, 10, 1)])
@pytest.mark.parametrize("name", ["six", "mixed"])
def test_pairs_from_walks_without_a_cdf_equal_deepwalk_pairs(name, lck):
    from glnn_amd import ops
    indptr, indices, g = graph(name)
    length, context, negatives = lck
    for n_roots in (1, 7, 300):
        r = torch.from_numpy(roots_for(indptr, n_roots))
        walks, start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs(g.indptr, g.indices, r, length, context, negatives, 123, 456)
        got = ops.deepwalk_pairs_from_walks(walks, g.n_src, context, negatives, 456)
        for a, b in zip(got, (start, rest, pair_indptr, win_indptr)):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _cdf_case(case):
    """(n_nodes, walks, cdf): the table of the graph at power 0.75; one node; a table of all 2^32 - 1; a table whose first entries are 0."""
    if case in ("six", "mixed"):
        indptr, indices, _ = graph(case)
        walks = nvo.node2vec_walk(indptr, indices, roots_for(indptr, 63), 10, 0.5, 2.0, 5)
        return len(indptr) - 1, walks, nvo.negative_cdf(indptr, indices, 0.75)
    if case == "one_node":
        return 1, np.zeros((3, 11), np.int64), np.array([2 ** 32 - 1])
    walks = np.arange(7 * 11).reshape(7, 11) % 6
    if case == "all_max":
        return 6, walks, np.full(6, 2 ** 32 - 1)
    return 6, walks, np.array([0, 0, 0, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1])          # leading_zeros


@pytest.mark.parametrize("case", ["six", "mixed", "one_node", "all_max", "leading_zeros"])
def test_pairs_from_walks_with_a_cdf_equal_the_oracle(case):
    from glnn_amd import ops
    n, walks, cdf = _cdf_case(case)
    for context, negatives in ((5, 1), (3, 3)):
        start, rest = nvo.pairs_from_walks(walks, n, context, negatives, 456, cdf)
        gs, gr, pair_indptr, win_indptr = ops.deepwalk_pairs_from_walks(torch.from_numpy(walks).to(DEV), n, context, negatives, 456, neg_cdf=cdf)
        q, r = rest.shape
        assert gs.dtype == gr.dtype == torch.int32 and tuple(gr.shape) == (q, r)
        assert np.array_equal(gs.cpu().numpy(), start) and np.array_equal(gr.cpu().numpy(), rest)
        assert np.array_equal(pair_indptr.cpu().numpy(), np.arange(q + 1) * r) and np.array_equal(win_indptr.cpu().numpy(), np.arange(q + 1))
        neg = rest[:, context - 1:]
        assert neg.min() >= 0 and neg.max() <= n - 1
        if case == "all_max":
            assert set(np.unique(neg)) <= {0, 5}                              # every draw below 2^32 - 1 lands on node 0
        if case == "leading_zeros":
            assert neg.min() == 3                                              # the zero-weight prefix is never drawn


# ------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("d", [4, 16, 100, 256])
def test_score_with_the_embedding_as_its_own_context_gives_the_one_table_bits(d):
    from glnn_amd import ops
    indptr, indices, g = graph("mixed")
    _, start, rest, _, _ = ops.deepwalk_pairs(g.indptr, g.indices, torch.from_numpy(roots_for(indptr, 63)), 6, 4, 2, 1, 2)
    z = torch.from_numpy(init_embedding(300, d, 0)).to(DEV)
    one = ops.deepwalk_score(z, start, rest, 4, 2)
    two = ops.deepwalk_score(z, start, rest, 4, 2, ctx=z)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    other = ops.deepwalk_score(z, start, rest, 4, 2, ctx=torch.from_numpy(init_embedding(300, d, 1)).to(DEV))
    assert not torch.equal(one[0], other[0]) and torch.equal(one[2], other[2])      # another context: other scores, the same snapshot of z


# ------------------------------------------------------------------------------------------------ three two-table steps against the oracle
# name -> (graph, roots, walk length, context, negatives, lr): the cases of tests/test_deepwalk_gpu.py, here with (p, q) = (0.5, 2),
# degree^0.75 negatives and a context table
STEP_CASES = {
    "six": ("six", np.array([5, 0, 3, 0, 2, 4, 1]), 4, 3, 2, 0.05),
    "star": ("star", np.arange(300), 4, 3, 1, 0.05),                     # the hub: start and entry of far more than 128 pairs
    "clustered": ("clustered", np.arange(512), 10, 5, 1, 0.05),
    "clustered8": ("clustered", np.arange(8) * 61, 10, 5, 1, 0.05),       # 8 roots: most of the 512 rows are in no pair
    "leaf300": ("star", np.full(300, 7), 1, 2, 1, 0.05),                  # one leaf 300 times: a start list of 300 behind a short entry list
}
STEP_P, STEP_Q, STEP_POWER = 0.5, 2.0, 0.75
KEYS = ("z", "mz", "vz", "c", "mc", "vc")
_REF = {}


def reference(case, d):
    """Three oracle steps of `case` at width d, once: per step the fp64 state, loss and touched rows, and the case's yardstick -- how far
    the SAME arithmetic in fp32 (numpy, on the CPU) lands from fp64, per tensor, the largest of the three steps."""
    if (case, d) not in _REF:
        gname, roots, length, context, negatives, lr = STEP_CASES[case]
        indptr, indices, _ = graph(gname)
        n = len(indptr) - 1
        cdf = nvo.negative_cdf(indptr, indices, STEP_POWER)
        rng = np.random.default_rng(1)
        init = [init_embedding(n, d, 0), (0.01 * rng.standard_normal((n, d))).astype(np.float32), (1e-4 * (0.5 + rng.random((n, d)))).astype(np.float32),
                init_embedding(n, d, 1), (0.01 * rng.standard_normal((n, d))).astype(np.float32), (1e-4 * (0.5 + rng.random((n, d)))).astype(np.float32)]
        st = {dt: tuple(x.astype(dt) for x in init) for dt in (np.float64, np.float32)}
        steps = []
        for t in (1, 2, 3):
            out = {dt: nvo.step(st[dt], indptr, indices, roots, length, context, negatives, 10 + t, 20 + t, lr, BETAS, EPS, t, p=STEP_P, q=STEP_Q,
                                cdf=cdf, dtype=dt) for dt in st}
            st = {dt: out[dt][0] for dt in out}
            s64, loss, tz, tc = out[np.float64]
            s32, loss32 = out[np.float32][:2]
            yard = {k: np.abs(a32 - a).max() for k, a, a32 in zip(KEYS, s64, s32)}
            yard["loss"] = abs(float(loss32) - float(loss))
            steps.append((s64, float(loss), tz, tc, yard))
        yard = {k: max(s[4][k] for s in steps) for k in KEYS + ("loss",)}
        _REF[(case, d)] = (init, [s[:4] + (yard,) for s in steps])
    return _REF[(case, d)]


@pytest.mark.parametrize("d", [4, 16, 100, 256])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_three_two_table_steps_against_the_fp64_oracle(case, d):
    """Tolerance: per case and tensor, 10 x the distance between the oracle run in fp32 and in fp64, the largest of the case's three steps
    (the rule of tests/test_deepwalk_gpu.py).  Every distance, bound and device figure is printed next to the assertion.  Rows of Z that
    start no window and rows of C that are no entry keep their bits."""
    from glnn_amd.position import DeepWalk
    gname, roots, length, context, negatives, lr = STEP_CASES[case]
    _, _, g = graph(gname)
    init, steps = reference(case, d)
    dw = DeepWalk(g, d, length, context, negatives, lr=lr, betas=BETAS, eps=EPS, seed=0, p=STEP_P, q=STEP_Q, negative_power=STEP_POWER,
                  context_table=True)
    tensors = dict(zip(KEYS, (dw.embedding, dw.exp_avg, dw.exp_avg_sq, dw.context, dw.context_exp_avg, dw.context_exp_avg_sq)))
    assert np.array_equal(dw.embedding.cpu().numpy(), init[0]) and np.array_equal(dw.context.cpu().numpy(), init[3])      # the oracle's initial bits
    for k in ("mz", "vz", "mc", "vc"):
        tensors[k].copy_(torch.from_numpy(init[KEYS.index(k)]))
    prev = dict(zip(KEYS, init))
    for t, (want, loss, tz, tc, yard) in zip((1, 2, 3), steps):
        got_loss = dw.step(torch.from_numpy(roots.astype(np.int64)), 10 + t, 20 + t)
        got = {k: tensors[k].cpu().numpy() for k in KEYS}
        for k, w in zip(KEYS, want):
            err, bound = np.abs(got[k] - w).max(), 10 * yard[k]
            print(f"{case} d={d} step {t} {k}: fp32 oracle vs fp64 {yard[k]:.3g}, bound {bound:.3g}, device vs fp64 {err:.3g}")
            assert err <= bound, (case, d, t, k, err, bound)
        err, bound = abs(got_loss.item() - loss), 10 * yard["loss"]
        print(f"{case} d={d} step {t} loss: fp32 oracle vs fp64 {yard['loss']:.3g}, bound {bound:.3g}, device vs fp64 {err:.3g}")
        assert err <= bound, (case, d, t, "loss", err, bound)
        for k in KEYS:
            untouched = ~(tz if k.endswith("z") else tc)
            assert np.array_equal(got[k][untouched], prev[k][untouched]), (case, d, t, k)
        prev = got
    if case == "clustered8":
        assert (~steps[0][2]).sum() > 256 and (~steps[0][3]).sum() > 256
    assert dw.steps == 3


# ------------------------------------------------------------------------------------------------ the default path
def test_default_arguments_give_the_bits_of_the_old_ops_driven_by_hand():
    """DeepWalk() with the four switches at their defaults, three fit batches (512 nodes, 171 roots per batch), against the launch
    sequence as it was before the switches existed, written out with the ops."""
    from glnn_amd import ops
    from glnn_amd.position import DeepWalk
    _, _, g = graph("clustered")
    torch.manual_seed(5)
    dw = DeepWalk(g, 16, 10, 5, 1, lr=0.05, seed=3)
    assert dw.context is None and dw.neg_cdf is None
    losses = dw.fit(1, 171)
    assert dw.steps == 3
    torch.manual_seed(5)
    gen = torch.Generator()
    gen.manual_seed(3)
    z = torch.randn((512, 16), generator=gen, dtype=torch.float32).to(DEV)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    order = ops.randperm_cpu(512)
    total = 0.0
    for b, s in enumerate(range(0, 512, 171)):
        walk_seed = (3 * 1000003 + 1 * 7919 + b * 31) & 0xFFFFFFFF
        _, start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs(g.indptr, g.indices, order[s:s + 171], 10, 5, 1, walk_seed, walk_seed ^ 0x4E454753)
        gr, gs, zs, loss_parts = ops.deepwalk_score(z, start, rest, 5, 1)
        q, r = rest.shape
        tw = ops.csr_transpose(win_indptr, start, q, 512, q)
        tp_indptr, _, tp_eids = ops.csr_transpose_eids(pair_indptr, rest.view(-1), q, 512, q * r)
        total += ops.deepwalk_apply(z, m, v, tw, (tp_indptr, tp_eids), gr, gs, zs, loss_parts, 5, 1, 0.05, (0.9, 0.999), 1e-8, b + 1).item()
    assert torch.equal(dw.embedding, z) and torch.equal(dw.exp_avg, m) and torch.equal(dw.exp_avg_sq, v)
    assert abs(losses[0] - total / 3) <= 1e-6 * abs(total / 3)


def test_each_switch_alone_changes_the_table_and_the_same_seed_gives_the_same_bits():
    from glnn_amd.position import DeepWalk
    _, _, g = graph("clustered")

    def fit(**kw):
        torch.manual_seed(5)
        dw = DeepWalk(g, 16, 10, 5, 1, lr=0.05, seed=3, **kw)
        dw.fit(1, 171)
        return dw.embedding.clone()

    base = fit()
    for kw in (dict(p=0.5), dict(q=2.0), dict(negative_power=0.75), dict(context_table=True)):
        a = fit(**kw)
        assert torch.equal(a, fit(**kw)) and not torch.equal(a, base), kw


# ------------------------------------------------------------------------------------------------ functional
def test_node2vec_embedding_separates_the_planted_communities():
    """The configuration tests/test_node2vec_cpu.py settled on, through DeepWalk.step: the fp64 oracle alone reaches 0.994 to 0.996 there
    (init seeds 0-3) and fp32 gives the same four values, so the bar of 0.95 leaves room only for a real defect."""
    from glnn_amd.position import DeepWalk
    _, _, labels, c = clustered_case()
    _, _, g = graph("clustered")
    dw = DeepWalk(g, c["d"], c["length"], c["context"], c["negatives"], lr=c["lr"], betas=BETAS, eps=EPS, seed=0, p=QUALITY["p"], q=QUALITY["q"],
                  negative_power=QUALITY["power"], context_table=True)
    roots = torch.arange(512)
    losses = [dw.step(roots, *step_seeds(s)) for s in range(c["steps"])]
    acc = dwo.centroid_accuracy(dw.embedding.cpu().numpy(), labels)
    first, last = losses[0].item(), losses[-1].item()
    print(f"accuracy {acc:.4f}, loss {first:.3f} -> {last:.3f}")
    assert acc >= QUALITY["bar"], acc
    assert last < 0.5 * first


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_is_a_value_error_with_the_c_message_and_nothing_is_written():
    from glnn_amd import _lib, ops
    from glnn_amd.position import DeepWalk
    _, _, g = graph("six")
    roots = torch.arange(6)
    for p, q in ((0.2, 1.0), (1.0, 4.5), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="glnn_node2vec_walk.*" + re.escape("p and q must be in [0.25, 4]")):
            ops.node2vec_walk(g.indptr, g.indices, roots, 4, p, q, 1)
    with pytest.raises(ValueError, match="glnn_node2vec_walk.*walk length"):
        ops.node2vec_walk(g.indptr, g.indices, roots, 65, 0.5, 2.0, 1)
    for bad in ([0, 6, 1], [0, -1, 1]):                                   # on the CPU and on the device: checked on the host, never an index
        for r in (torch.tensor(bad), torch.tensor(bad, device=DEV)):
            with pytest.raises(ValueError, match="glnn_node2vec_walk.*outside the graph of 6 nodes"):
                ops.node2vec_walk(g.indptr, g.indices, r, 4, 0.5, 2.0, 1)
    walks = ops.node2vec_walk(g.indptr, g.indices, roots, 4, 0.5, 2.0, 1)
    for (context, negatives), needle in (((1, 1), "context size"), ((6, 1), "context size"), ((3, 0), "negatives per positive")):
        with pytest.raises(ValueError, match="glnn_deepwalk_pairs_from_walks.*" + re.escape(needle)):
            ops.deepwalk_pairs_from_walks(walks, 6, context, negatives, 2)
    with pytest.raises(ValueError, match="one entry per node"):
        ops.deepwalk_pairs_from_walks(walks, 6, 3, 1, 2, neg_cdf=np.arange(5))
    start, rest, _, _ = ops.deepwalk_pairs_from_walks(walks, 6, 3, 1, 2)
    z = torch.zeros((6, 8), device=DEV)
    out = [torch.zeros(n, device=DEV) for n in (rest.numel(), 6 * 8, 6 * 8, 2 * 6)]
    with pytest.raises(ValueError, match="glnn_deepwalk_score_ctx_f32.*null pointer"):      # a null table pointer, handed to the C entry itself
        rc = _lib.lib().glnn_deepwalk_score_ctx_f32(z.data_ptr(), None, 6, 8, start.data_ptr(), rest.data_ptr(), start.numel(), 3, 1,
                                                    *[o.data_ptr() for o in out], None)
        ops._dw_check(rc, "glnn_deepwalk_score_ctx_f32")
    torch.cuda.synchronize()
    assert not any(o.any() for o in out)
    with pytest.raises(ValueError, match="ctx must have z's shape"):
        ops.deepwalk_score(z, start, rest, 3, 1, ctx=torch.zeros((6, 4), device=DEV))
    for kw in (dict(p=0.2), dict(q=5.0), dict(negative_power=-1.0)):
        with pytest.raises(ValueError):
            DeepWalk(g, 8, 4, 3, 1, **kw)
    dw = DeepWalk(g, 8, 4, 3, 1, p=0.5, q=2.0, negative_power=0.75, context_table=True)
    before = [t.clone() for t in (dw.embedding, dw.exp_avg, dw.exp_avg_sq, dw.context, dw.context_exp_avg, dw.context_exp_avg_sq)]
    with pytest.raises(ValueError, match="outside the graph"):
        dw.step(torch.tensor([0, 9]), 1, 2)
    after = (dw.embedding, dw.exp_avg, dw.exp_avg_sq, dw.context, dw.context_exp_avg, dw.context_exp_avg_sq)
    assert dw.steps == 0 and all(torch.equal(a, b) for a, b in zip(before, after))
    assert dw.step(torch.zeros(0, dtype=torch.int64), 1, 2).item() == 0.0 and dw.steps == 0      # an empty batch is no step
