"""glnn_position_rows and ServedPositionStudent on the GPU (docs/POSITION_SEMANTICS.md, "Serving by node id") against the fp64 oracle of
tests/position_serve_oracle.py.

Feature columns and the rows of embedded nodes are copies: equal bits.  The rows of unseen nodes are fp32 means, held to
    |got - want| <= 1.01 * count * 2^-24 * mean_abs      per column, mean_abs = sum |z[slot[u], j]| / count
the first-order bound of an fp32 sum of `count` terms in any order ((count - 1) roundings of partial sums, each at most 2^-24 of
sum |z|) plus the one division (2^-24 of the mean), with 1 % for the second-order terms -- derived, not measured; rows with count 0 are
exact zeros.  bf16 outputs of unseen rows: bf16_rules.assert_within_one_ulp."""
import functools

import numpy as np
import pytest
import torch

import bf16_rules
import graphgen
import position_serve_oracle as pso
from subgraph_oracle import six_node_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
def _sentinel(dtype):
    """What the output buffers are pre-filled with: a value the kernel never writes here, exact in the buffer's dtype."""
    return 12288.0 if dtype == torch.bfloat16 else 12345.0


# ------------------------------------------------------------------------------------------------ the graphs
@functools.lru_cache(maxsize=None)
def big_case():
    """300 nodes, 3 of them isolated; rows of 129 (the hub, just above kLongRow), exactly 128 and 1100 entries, a stored multi-edge, an
    unseen node with a self-loop, a node whose in-neighbours are all unseen.  About 30 % of the nodes are unseen, all of those among them.
    Returns (indptr, indices, unseen mask, the named nodes)."""
    n = 300
    indptr, indices = graphgen.random_graph(n, 6.0, 5, isolated=3)
    rows = [list(indices[indptr[v]:indptr[v + 1]]) for v in range(n)]
    rs = np.random.RandomState(17)
    iso = [v for v in range(n) if not rows[v]]
    assert len(iso) >= 3
    pick = [int(v) for v in rs.permutation([v for v in range(n) if rows[v]])[:9]]
    hub, r128, r1100, multi, selfl, lonely = pick[:6]
    rows[hub] = list(rs.randint(0, n, 129))
    rows[r128] = list(rs.randint(0, n, 128))
    rows[r1100] = list(rs.randint(0, n, 1100))
    rows[multi] = [pick[6], pick[6], pick[6], pick[7]]
    rows[selfl] = [selfl, pick[7], pick[8]]
    rows[lonely] = [hub, selfl, iso[0]]
    unseen = rs.rand(n) < 0.25
    unseen[pick[6:9]] = False                                    # the multi-edge's source is embedded: it counts three times
    unseen[[hub, r128, r1100, multi, selfl, lonely, iso[0]]] = True
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    indices = np.asarray([u for r in rows for u in r], np.int32)
    named = dict(hub=hub, r128=r128, r1100=r1100, multi=multi, selfl=selfl, lonely=lonely, iso=iso[0])
    assert 0.2 < unseen.mean() < 0.4
    return indptr, indices, unseen, named


@functools.lru_cache(maxsize=None)
def six_case():
    indptr, indices = six_node_graph()
    return indptr, indices, np.array([True, False, False, False, True, True]), dict()


@functools.lru_cache(maxsize=None)
def batches(which):
    """The id vectors of a case, by m: 1 (the hub / node 0), 31 (with repeats), 33 (descending), 1000 (every node, with repeats)."""
    indptr, _, unseen, named = big_case() if which == "big" else six_case()
    n = len(indptr) - 1
    rs = np.random.RandomState(23)
    special = list(named.values()) or [0]
    b31 = np.concatenate([special, special[:3], rs.randint(0, n, 31)])[:31]
    b33 = np.sort(np.concatenate([special, rs.randint(0, n, 33)])[:33])[::-1].copy()
    b1000 = np.concatenate([np.arange(n), special, rs.randint(0, n, 1000)])[:1000]
    return {1: np.asarray(special[:1], np.int64), 31: b31.astype(np.int64), 33: b33.astype(np.int64), 1000: rs.permutation(b1000).astype(np.int64)}


@functools.lru_cache(maxsize=None)
def data(which, f, d):
    """x [n, f] fp32, z [r, d] fp32 N(0, 1), slot, and the oracle over EVERY node (computed once, indexed by the batches)."""
    indptr, indices, unseen, _ = big_case() if which == "big" else six_case()
    n = len(indptr) - 1
    rs = np.random.RandomState(1000 * f + d)
    x = rs.standard_normal((n, f)).astype(np.float32)
    obs = np.nonzero(~unseen)[0]
    z = rs.standard_normal((len(obs), d)).astype(np.float32)
    slot = np.full(n, -1, np.int32)
    slot[obs] = np.arange(len(obs), dtype=np.int32)
    want, count, mean_abs = pso.rows(np.arange(n), x, z, slot, indptr, indices)
    return x, z, slot, want, count, mean_abs


def _dev(which, f, d):
    from glnn_amd.graph import CSRGraph
    indptr, indices, _, _ = big_case() if which == "big" else six_case()
    x, z, slot, _, _, _ = data(which, f, d)
    g = CSRGraph(torch.from_numpy(indptr), torch.from_numpy(indices), len(indptr) - 1).to(DEV)
    return g, torch.from_numpy(x).to(DEV), torch.from_numpy(z).to(DEV), torch.from_numpy(slot).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def _launch(ids, x, z, slot, g, out_dtype, extra_rows=3):
    """ops.position_rows into a sentinel-filled buffer with spare rows and spare columns; returns (the [m, f + d] result, the buffer)."""
    from glnn_amd import ops
    e = 8 if out_dtype == torch.bfloat16 else 4
    m, w = ids.numel(), x.shape[1] + z.shape[1]
    buf = torch.full((m + extra_rows, (w + e - 1) // e * e + e), _sentinel(out_dtype), dtype=out_dtype, device=DEV)
    got = ops.position_rows(ids, x, z, slot, g=g, out=buf[:, :w])
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (m, w)
    return got, buf


# ------------------------------------------------------------------------------------------------ the kernel against the oracle
SHAPES = [(1, 4), (7, 16), (100, 100), (128, 256), (1433, 16), (33, 36),
          (5, 256),       # (an fp32 tail of 65 pieces: the one shape at which the write-out loop of a wave runs twice)
          (12, 8), (64, 32)]      # (LPR 2 and 8: the two lane layouts the shapes above leave out)


@pytest.mark.parametrize("which", ["six", "big"])
@pytest.mark.parametrize("f, d", SHAPES)
def test_rows_against_the_oracle(which, f, d):
    from glnn_amd import ops
    g, x, z, slot = _dev(which, f, d)
    _, _, slot_h, want_all, count_all, mean_abs_all = data(which, f, d)
    xb = ops.to_bf16(x)
    pairs = [(x, torch.float32), (ops.as_feat(x), torch.float32), (x, torch.bfloat16), (xb, torch.bfloat16)]
    checked_long = 0
    for m, ids_h in batches(which).items():
        ids = torch.from_numpy(ids_h).to(DEV)
        seen = slot_h[ids_h] >= 0
        want, count, mean_abs = want_all[ids_h], count_all[ids_h], mean_abs_all[ids_h]
        z_seen = z[torch.from_numpy(slot_h[ids_h][seen].astype(np.int64)).to(DEV)]
        for xin, odt in pairs:
            got, buf = _launch(ids, xin, z, slot, g, odt)
            e = 8 if odt == torch.bfloat16 else 4
            pad_end = (f + d + e - 1) // e * e
            # untouched: rows >= m and the columns behind the padding; the padding itself is exact zeros
            assert (buf[m:] == _sentinel(odt)).all() and (buf[:m, pad_end:] == _sentinel(odt)).all()
            assert (_bits(buf[:m, f + d:pad_end]) == 0).all()
            # feature columns and seen rows: equal bits
            if odt == torch.float32:
                want_x, want_z = x[ids], z_seen
            else:
                want_x = xb[ids] if xin.dtype == torch.bfloat16 else ops.to_bf16(x[ids])
                want_z = ops.to_bf16(z_seen)
            assert np.array_equal(_bits(got[:, :f]), _bits(want_x)), (m, xin.dtype, odt)
            assert np.array_equal(_bits(got[:, f:][torch.from_numpy(seen).to(DEV)]), _bits(want_z)), (m, xin.dtype, odt)
            # unseen rows: every one of them is compared
            pos = got[:, f:][torch.from_numpy(~seen).to(DEV)]
            w_u, c_u, a_u = want[~seen][:, f:], count[~seen], mean_abs[~seen]
            assert (_bits(pos[torch.from_numpy(c_u == 0).to(DEV)]) == 0).all()
            if odt == torch.float32:
                err = np.abs(pos.cpu().numpy().astype(np.float64) - w_u)
                bound = 1.01 * c_u[:, None] * 2.0 ** -24 * a_u
                worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
                print(f"{which} f={f} d={d} m={m} x={xin.dtype} ld={xin.stride(0)}: {len(c_u)} unseen rows, max count {c_u.max() if len(c_u) else 0}, "
                      f"worst err / bound {worst:.3f}")
                assert (err <= bound).all(), (m, worst)
            else:
                bf16_rules.assert_within_one_ulp(pos, w_u)
            checked_long += int((c_u > 0).sum())
    assert checked_long > 0


def test_the_long_rows_are_in_the_batches():
    """The geometry the cases are there for: entry counts on both sides of kLongRow = 128 and a row of several chunks per wave."""
    indptr, _, unseen, named = big_case()
    deg = np.diff(indptr)
    assert deg[named["hub"]] == 129 and deg[named["r128"]] == 128 and deg[named["r1100"]] == 1100 and deg[named["iso"]] == 0
    _, _, _, _, count, _ = data("big", 7, 16)
    assert count[named["lonely"]] == 0 and count[named["multi"]] == 4 and count[named["selfl"]] == 2
    assert all(unseen[v] for v in named.values()) and batches("big")[1][0] == named["hub"]
    assert all(v in batches("big")[1000] and v in batches("big")[33] and v in batches("big")[31] for v in named.values())


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
def test_a_row_depends_on_nothing_but_its_id(odt):
    from glnn_amd import ops
    f, d = 33, 36
    g, x, z, slot = _dev("big", f, d)
    ids_h = batches("big")[1000]
    ids = torch.from_numpy(ids_h).to(DEV)
    a = ops.position_rows(ids, x, z, slot, g=g, out_dtype=odt)
    b = ops.position_rows(ids, x, z, slot, g=g, out_dtype=odt)
    assert np.array_equal(_bits(a), _bits(b))                                            # two runs
    perm = torch.from_numpy(np.random.RandomState(5).permutation(len(ids_h))).to(DEV)
    c = ops.position_rows(ids[perm].contiguous(), x, z, slot, g=g, out_dtype=odt)
    assert np.array_equal(_bits(a[perm]), _bits(c))                                      # another place in the batch, other neighbours
    first = {int(v): i for i, v in reversed(list(enumerate(ids_h)))}
    for v in batches("big")[33]:                                                         # each id alone
        one = ops.position_rows(torch.tensor([int(v)], device=DEV), x, z, slot, g=g, out_dtype=odt)
        assert np.array_equal(_bits(one[0]), _bits(a[first[int(v)]])), int(v)


def test_without_a_graph_an_unseen_row_is_zeros():
    from glnn_amd import ops
    f, d = 7, 16
    _, x, z, slot = _dev("big", f, d)
    _, _, slot_h, _, _, _ = data("big", f, d)
    ids_h = batches("big")[33]
    got = ops.position_rows(torch.from_numpy(ids_h).to(DEV), x, z, slot)
    seen = torch.from_numpy(slot_h[ids_h] >= 0).to(DEV)
    assert (_bits(got[:, f:][~seen]) == 0).all() and (~seen).any()
    assert torch.equal(got[:, f:][seen], z[torch.from_numpy(slot_h[ids_h].astype(np.int64)).to(DEV)[seen]])
    assert torch.equal(got[:, :f], x[torch.from_numpy(ids_h).to(DEV)])


# ------------------------------------------------------------------------------------------------ composition
def _student(width):
    """A small BatchNorm student dims = (width, 64, 64, 7) in eval mode with drawn parameters and running statistics."""
    from glnn_amd.models import Model
    torch.manual_seed(3)
    model = Model(dict(model_name="MLP", num_layers=3, feat_dim=width, hidden_dim=64, label_dim=7, dropout_ratio=0.5, norm_type="batch", device=DEV))
    with torch.no_grad():
        for bn in model.encoder.norms:
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.2)
    return model.eval()


def _table(which, f, d):
    from glnn_amd.position import PositionTable
    indptr, _, unseen, _ = big_case() if which == "big" else six_case()
    _, z, _, _, _, _ = data(which, f, d)
    return PositionTable(torch.from_numpy(z).to(DEV), torch.from_numpy(np.nonzero(~unseen)[0]).to(DEV), len(indptr) - 1)


def test_served_position_student_composes_the_existing_chains(monkeypatch):
    from glnn_amd import ops, serve
    f, d = 33, 36
    g, x, z, slot = _dev("big", f, d)
    _, _, slot_h, _, _, _ = data("big", f, d)
    table = _table("big", f, d)
    assert table.has_unseen and torch.equal(table.slot(), slot)
    model = _student(f + d)
    plain = serve.compile_student(model)
    ids_h = batches("big")[1000]
    ids = torch.from_numpy(ids_h).to(DEV)
    served = serve.compile_position_student(model, x, table, g)
    # all ids seen: the path a user has today, over the materialised [N, F + D] matrix
    seen_ids = ids[torch.from_numpy(slot_h[ids_h] >= 0).to(DEV)].contiguous()
    cat = torch.cat([x, table.dense(g)], 1)
    assert torch.equal(served.log_probs(seen_ids), plain.log_probs(cat[seen_ids]))
    assert torch.equal(served.logits(seen_ids), plain.logits(cat[seen_ids]))
    # with unseen ids: the chain over the block the kernel itself assembled
    block = ops.position_rows(ids, x, z, slot, g=g, out_dtype=torch.bfloat16)
    want = plain.log_probs(block)
    got = served.log_probs(ids)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    # the fp32 form over its own fp32 block
    served32 = serve.compile_position_student(model, x, table, g, dtype=torch.float32)
    block32 = ops.position_rows(ids, x, z, slot, g=g)
    assert torch.equal(served32.log_probs(ids), ops.log_softmax(model.inference(None, block32)))
    assert torch.equal(served32.logits(ids), model.inference(None, block32))
    # blocks of 64 ids: the same bits as one block
    monkeypatch.setattr(serve, "POSITION_BLOCK_ROWS", 64)
    out = torch.full((len(ids_h), 7), 7.0, device=DEV)
    assert served.log_probs(ids, out=out) is out and torch.equal(out, want)


def test_compile_position_student_refusals():
    from glnn_amd import serve
    f, d = 33, 36
    g, x, z, slot = _dev("big", f, d)
    table = _table("big", f, d)
    with pytest.raises(ValueError, match="first layer"):
        serve.compile_position_student(_student(f + d + 4), x, table, g)
    with pytest.raises(ValueError, match="needs the graph"):
        serve.compile_position_student(_student(f + d), x, table)
    with pytest.raises(NotImplementedError):
        serve.compile_position_student(_student(f + d).train(), x, table, g)
    with pytest.raises(ValueError, match="dtype"):
        serve.compile_position_student(_student(f + d), x, table, g, dtype=torch.float16)
    served = serve.compile_position_student(_student(f + d), x, table, g)
    out = torch.full((3, 7), 7.0, device=DEV)
    for bad in ([0, 300, 1], [5, -1, 2]):
        with pytest.raises(ValueError, match=r"ids must lie in \[0, 300\)"):
            served.log_probs(torch.tensor(bad, device=DEV), out=out)
    assert (out == 7.0).all()                                                            # nothing was launched for those calls
    assert torch.isfinite(served.log_probs(torch.tensor([0, 299, 1], device=DEV), out=out)).all()
