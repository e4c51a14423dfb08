"""glnn_random_walk / glnn_induced_subgraph, RandomWalkSubgraphLoader and train_subgraph on the GPU (docs/SUBGRAPH_SEMANTICS.md).
Everything is exact: integer arrays against the numpy oracle (tests/subgraph_oracle.py) and against CSRGraph.subgraph on CPU tensors,
parameters against a hand loop of train() with torch.equal.  No tolerances."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import subgraph_oracle as so
from graphgen import csr_from_edges, random_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N = 600
MODES = ("keep", "add")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges(ip, ix):
    return ix.astype(np.int64), np.repeat(np.arange(len(ip) - 1), np.diff(ip))


class _G:
    """The 600-node test graph: a 700-edge hub row, a 150-entry row (more than one round of a wave, fewer than 256), isolated rows
    (in-degree 0), self-loops on every seventh row that has in-edges, and an explicit multi-edge pair."""

    def __init__(self):
        ip, ix = random_graph(N, 6.0, seed=11, isolated=8, hub=700)
        src, dst = _edges(ip, ix)
        deg = np.diff(ip)
        self.hub = int(np.argmax(deg))
        self.iso = np.flatnonzero(deg == 0)
        live = np.flatnonzero(deg > 0)
        loops = live[::7]
        self.mid = int(live[live != self.hub][5])
        rs = np.random.RandomState(4)
        mid_src = rs.choice(np.setdiff1d(np.arange(N), self.iso), 150)
        self.multi = (int(src[dst == live[3]][0]), int(live[3]))             # this edge exists: listed once more below
        src = np.concatenate([src, loops, mid_src, [self.multi[0]]])
        dst = np.concatenate([dst, loops, np.full(150, self.mid), [self.multi[1]]])
        self.ip, self.ix = csr_from_edges(src, dst, N)
        self.loops = loops
        deg = np.diff(self.ip)
        assert deg[self.hub] > 700 and 64 < deg[self.mid] <= 256 and len(self.iso) >= 8 and (deg[self.iso] == 0).all()
        self.tip, self.tix = _t(self.ip), _t(self.ix)
        self._ref = {}

    def oracle(self, key, cand, mode):
        """The oracle's answer for a named candidate list, computed once and shared."""
        if (key, mode) not in self._ref:
            self._ref[(key, mode)] = so.induced_subgraph(self.ip, self.ix, cand, mode)
        return self._ref[(key, mode)]


@pytest.fixture(scope="module")
def G():
    return _G()


# ------------------------------------------------------------------------------------------------ walk
@pytest.mark.parametrize("length", [1, 4, 64])
@pytest.mark.parametrize("n_roots", [1, 257, 0])
def test_walk_equals_the_oracle_bit_for_bit(G, length, n_roots):
    from glnn_amd import ops
    rs = np.random.RandomState(length * 1000 + n_roots)
    roots = rs.randint(0, N, size=n_roots).astype(np.int64)
    if n_roots:
        roots[0] = G.iso[0]                       # a degree-0 root
    if n_roots > 2:
        roots[1], roots[-1] = G.hub, G.iso[1]     # (the last walk of the ragged last workgroup)
    out = ops.random_walk(G.tip, G.tix, _t(roots), length, 1234)
    assert out.shape == (n_roots, length + 1) and out.dtype == torch.int64
    ref = so.random_walk(G.ip, G.ix, roots, length, 1234)
    assert np.array_equal(out.cpu().numpy(), ref)
    if n_roots:
        assert (out[0] == int(G.iso[0])).all()    # it repeats itself
    if n_roots == 257:
        other = ops.random_walk(G.tip, G.tix, _t(roots), length, 1235)
        assert not torch.equal(other, out)        # another seed, other walks
        assert np.array_equal(other.cpu().numpy(), so.random_walk(G.ip, G.ix, roots, length, 1235))
        assert torch.equal(ops.random_walk(G.tip, G.tix, _t(roots), length, 1234), out)


def test_walk_argument_checks(G):
    from glnn_amd import ops
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        ops.random_walk(G.tip, G.tix, _t(np.zeros(3, np.int64)), 0, 1)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        ops.random_walk(G.tip, G.tix, _t(np.zeros(3, np.int64)), 65, 1)
    with pytest.raises(ValueError, match="int64"):
        ops.random_walk(G.tip, G.tix, _t(np.zeros(3, np.int32)), 2, 1)


# ------------------------------------------------------------------------------------------------ builder
def _independent_set(ip, ix, want, seed):
    """Nodes with no edge between any two of them and no self-loop."""
    src, dst = _edges(ip, ix)
    adj = {}
    for u, v in zip(src.tolist(), dst.tolist()):
        adj.setdefault(u, set()).add(v)
        adj.setdefault(v, set()).add(u)
    chosen, blocked = [], set()
    for v in np.random.RandomState(seed).permutation(len(ip) - 1).tolist():
        if v in blocked or v in adj.get(v, ()):
            continue
        chosen.append(v)
        blocked |= adj.get(v, set())
        if len(chosen) == want:
            break
    return np.asarray(chosen, np.int64)


def _cands(G):
    rs = np.random.RandomState(21)
    hub_src = G.ix[G.ip[G.hub]:G.ip[G.hub + 1]][:120].astype(np.int64)
    subset = so.first_appearance(np.concatenate([[G.hub, G.mid, G.multi[0], G.multi[1], G.loops[0], G.loops[1], G.iso[0]], hub_src,
                                                 rs.choice(N, 60, replace=False)]))
    repeats = np.concatenate([subset[:50], subset[:50][::-1], rs.randint(0, N, 80), [G.hub, G.hub]]).astype(np.int64)
    return {"empty": np.zeros(0, np.int64), "one": np.asarray([G.loops[2]], np.int64), "one_isolated": np.asarray([G.iso[2]], np.int64),
            "perm": rs.permutation(N).astype(np.int64), "subset": subset, "repeats": repeats, "no_edge": _independent_set(G.ip, G.ix, 40, 2)}


def _check(got, ref, cand, mode):
    nodes, sip, six, n_sub, nnz, zero = got
    rnodes, rip, rix, rzero = ref
    assert n_sub == len(rnodes) and nnz == len(rix) and zero == rzero
    assert nodes.dtype == torch.int64 and sip.dtype == torch.int64 and six.dtype == torch.int32
    assert np.array_equal(nodes.cpu().numpy(), rnodes)
    assert np.array_equal(sip.cpu().numpy(), rip)
    assert np.array_equal(six.cpu().numpy(), rix)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["empty", "one", "one_isolated", "perm", "subset", "repeats", "no_edge"])
def test_builder_equals_the_oracle_and_csrgraph_subgraph(G, case, mode):
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    cand = _cands(G)[case]
    ref = G.oracle(case, cand, mode)
    got = ops.induced_subgraph(G.tip, G.tix, _t(cand), mode)
    _check(got, ref, cand, mode)
    nodes, sip, six, n_sub, nnz, zero = got
    if case != "repeats" and mode == "keep":          # candidates without repeats: CSRGraph.subgraph on CPU tensors, array for array
        sub = CSRGraph(torch.from_numpy(G.ip), torch.from_numpy(G.ix), N).subgraph(torch.from_numpy(cand))
        assert torch.equal(sub.indptr, sip.cpu()) and torch.equal(sub.indices, six.cpu())
        assert np.array_equal(nodes.cpu().numpy(), cand)
    if case == "repeats":
        assert n_sub < len(cand) and np.array_equal(nodes.cpu().numpy(), so.first_appearance(cand))
    if case == "no_edge":
        assert n_sub == 40 and ((zero == n_sub and nnz == 0) if mode == "keep" else (zero == 0 and nnz == n_sub))
    if case == "subset":                              # graph rows of one round of the wave, of several, and of more than 256 entries are walked
        rows = np.diff(G.ip)[ref[0]]
        assert rows.max() > 256 and ((rows > 64) & (rows <= 256)).any() and ((rows > 0) & (rows <= 64)).any() and (rows == 0).any()
        assert np.diff(ref[1]).max() > 64             # and a subgraph row is filled across rounds (ranks carried from round to round)
    if mode == "add" and n_sub:
        last = six.cpu().numpy()[ref[1][1:] - 1]
        assert np.array_equal(last, np.arange(n_sub)) and zero == 0


def test_builder_argument_checks(G):
    from glnn_amd import ops
    with pytest.raises(ValueError, match="self_loop"):
        ops.induced_subgraph(G.tip, G.tix, _t(np.zeros(3, np.int64)), "both")
    with pytest.raises(ValueError, match="int64"):
        ops.induced_subgraph(G.tip, G.tix, _t(np.zeros(3, np.int32)))


# ------------------------------------------------------------------------------------------------ table modes
@pytest.fixture(scope="module")
def sparse_200k():
    """200 000 nodes, about two in-edges each, plus 3000 edges among the 1000 highest ids (so that a few hundred of those induce edges)."""
    n = 200_000
    ip, ix = random_graph(n, 2.0, seed=5)
    src, dst = _edges(ip, ix)
    rs = np.random.RandomState(6)
    top = n - 1000
    src = np.concatenate([src, top + rs.randint(0, 1000, 3000)])
    dst = np.concatenate([dst, top + rs.randint(0, 1000, 3000)])
    return csr_from_edges(src, dst, n)


@pytest.mark.parametrize("mode", MODES)
def test_hash_table_mode_with_probing(sparse_200k, mode):
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    ip, ix = sparse_200k
    n = len(ip) - 1
    cand = (n - 1000 + np.random.RandomState(8).choice(1000, 300, replace=False)).astype(np.int64)
    cand[0] = n - 1                                   # the top of the id range
    cand = so.first_appearance(cand)
    assert not ops.induced_subgraph_direct(len(cand), n)                      # open addressing: asserted, not assumed
    home = so.hash_slot(cand, so.table_cap(len(cand)))
    assert len(np.unique(home)) < len(cand)                                   # at least two candidates share a home slot: probing happens
    ref = so.induced_subgraph(ip, ix, cand, mode)
    assert len(ref[2]) > 100
    got = ops.induced_subgraph(_t(ip), _t(ix), _t(cand), mode)
    _check(got, ref, cand, mode)
    if mode == "keep":
        sub = CSRGraph(torch.from_numpy(ip), torch.from_numpy(ix), n).subgraph(torch.from_numpy(cand))
        assert torch.equal(sub.indptr, got[1].cpu()) and torch.equal(sub.indices, got[2].cpu())


@pytest.mark.parametrize("mode", MODES)
def test_direct_table_mode_over_several_scan_workgroups(mode):
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    n = 6000
    ip, ix = random_graph(n, 6.0, seed=9, isolated=20, hub=400)
    cand = np.random.RandomState(10).permutation(n)[:5000].astype(np.int64)
    assert ops.induced_subgraph_direct(len(cand), n) and len(cand) > 4 * 1024         # direct mode; five workgroups in each scan
    ref = so.induced_subgraph(ip, ix, cand, mode)
    got = ops.induced_subgraph(_t(ip), _t(ix), _t(cand), mode)
    _check(got, ref, cand, mode)
    if mode == "keep":
        sub = CSRGraph(torch.from_numpy(ip), torch.from_numpy(ix), n).subgraph(torch.from_numpy(cand))
        assert torch.equal(sub.indptr, got[1].cpu()) and torch.equal(sub.indices, got[2].cpu())


# ------------------------------------------------------------------------------------------------ bad input, bit identity
GUARD, WORD64, WORD32 = 64, -0x0123456789ABCDEF, 0x5A5A5A5A


def _raw(tip, tix, cand, mode, nnz_cap):
    """glnn_induced_subgraph on buffers of exactly the documented sizes followed by GUARD sentinel words each."""
    from glnn_amd import _lib, ops
    h = _lib.lib()
    nc, n = cand.numel(), tip.numel() - 1
    nodes = torch.full((nc + GUARD,), WORD64, dtype=torch.int64, device=DEV)
    sip = torch.full((nc + 1 + GUARD,), WORD64, dtype=torch.int64, device=DEV)
    six = torch.full((nnz_cap + GUARD,), WORD32, dtype=torch.int32, device=DEV)
    counts = torch.full((3 + GUARD,), WORD64, dtype=torch.int64, device=DEV)
    wsb = int(h.glnn_induced_subgraph_workspace_bytes(nc, n))
    ws = torch.full(((wsb + 7) // 8 + GUARD,), WORD64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = h.glnn_induced_subgraph(p(tip), p(tix), n, p(cand), nc, 1 if mode == "add" else 0, nnz_cap, p(nodes), p(sip), p(six), p(counts),
                                 p(ws), wsb, ops._stream())
    assert rc == 0, h.glnn_last_error()
    torch.cuda.synchronize()
    assert (nodes[nc:] == WORD64).all() and (sip[nc + 1:] == WORD64).all() and (six[nnz_cap:] == WORD32).all()
    assert (counts[3:] == WORD64).all() and (ws[(wsb + 7) // 8:] == WORD64).all()
    return nodes[:nc], sip[:nc + 1], six[:nnz_cap], counts[:3].tolist()


@pytest.mark.parametrize("mode", MODES)
def test_out_of_range_ids_are_reported_not_indexed(G, sparse_200k, mode):
    from glnn_amd import GlnnError, ops
    good = _cands(G)["subset"]
    for bad_id in (N, -1, (1 << 31) + 5, -(1 << 40)):
        cand = _t(np.concatenate([good[:30], [bad_id], good[30:]]).astype(np.int64))
        cap = int(np.diff(G.ip)[good].sum()) + len(good) + 1
        _, _, _, counts = _raw(G.tip, G.tix, cand, mode, cap)                 # direct mode
        assert counts[0] == -1
        with pytest.raises(GlnnError, match="outside"):
            ops.induced_subgraph(G.tip, G.tix, cand, mode)
    _, sip, _, counts = _raw(G.tip, G.tix, _t(np.asarray([N, -1, N + 7], np.int64)), mode, 4)      # nothing but bad ids: an empty subgraph
    assert counts == [-1, 0, 0] and int(sip[0]) == 0
    ip, ix = sparse_200k                                                      # hash mode
    n = len(ip) - 1
    cand = _t(np.asarray([n - 1, n, n - 2, 5, -7, n - 3] * 20, np.int64))
    _, _, _, counts = _raw(_t(ip), _t(ix), cand, mode, 64)
    assert counts[0] == -1


@pytest.mark.parametrize("mode", MODES)
def test_a_capacity_that_is_too_small_is_reported_never_written_past(G, mode):
    from glnn_amd import GlnnError, ops
    cand = _cands(G)["subset"]
    rnodes, rip, rix, rzero = G.oracle("subset", cand, mode)
    for cap in (len(rix) - 5, len(rix) // 2, 0):
        nodes, sip, six, counts = _raw(G.tip, G.tix, _t(cand), mode, cap)
        assert counts == [len(rnodes), len(rix), rzero] and counts[1] > cap          # the TRUE count comes back
        assert np.array_equal(sip.cpu().numpy(), rip)
        assert np.array_equal(six.cpu().numpy(), rix[:cap])                          # what fits is what the full build holds there
        with pytest.raises(GlnnError, match="more than nnz_cap"):
            ops.induced_subgraph(G.tip, G.tix, _t(cand), mode, nnz_cap=cap)
    nodes, sip, six, counts = _raw(G.tip, G.tix, _t(cand), mode, len(rix))           # the exact capacity suffices
    assert counts[1] == len(rix) and np.array_equal(six.cpu().numpy(), rix)


@pytest.mark.parametrize("mode", MODES)
def test_two_runs_give_the_same_bits(G, mode):
    cand = _t(_cands(G)["repeats"])
    cap = int(np.diff(G.ip)[_cands(G)["repeats"]].sum()) + cand.numel()
    a, b = _raw(G.tip, G.tix, cand, mode, cap), _raw(G.tip, G.tix, cand, mode, cap)
    n_sub, nnz = a[3][0], a[3][1]
    assert a[3] == b[3] and n_sub > 0 and nnz > 0
    assert torch.equal(a[0][:n_sub], b[0][:n_sub]) and torch.equal(a[1][:n_sub + 1], b[1][:n_sub + 1]) and torch.equal(a[2][:nnz], b[2][:nnz])


# ------------------------------------------------------------------------------------------------ loader and training
def _sym_graph():
    from glnn_amd.graph import CSRGraph
    ip, ix = random_graph(N, 3.0, seed=31, symmetric=True, self_loops=True, hub=80)
    return ip, ix, CSRGraph(_t(ip), _t(ix), N)


def _model(name, d_in, n_cls, seed=0):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    conf = dict(model_name=name, num_layers=2, feat_dim=d_in, hidden_dim=16, label_dim=n_cls, dropout_ratio=0.5, norm_type="none",
                device=DEV, num_heads=2, attn_dropout_ratio=0.3)
    if name == "GCN":
        conf["norm_type"] = "batch"
    if name == "GCNII":
        conf["num_layers"] = 4
    return Model(conf)


def test_loader_yields_the_oracles_batches():
    from glnn_amd.graph import RandomWalkSubgraphLoader
    ip, ix, g = _sym_graph()
    idx_train = np.random.RandomState(1).choice(N, 70, replace=False).astype(np.int64)
    loader = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 3, shuffle=False, seed=5)
    assert len(loader) == 3
    is_train = np.zeros(N, bool)
    is_train[idx_train] = True
    for epoch in (1, 2):
        batches = list(loader)
        assert len(batches) == 3
        for b, (sub, nodes, local) in enumerate(batches):
            roots = idx_train[b * 32:(b + 1) * 32]
            walks = so.random_walk(ip, ix, roots, 3, loader.rng_seed(epoch, b))
            rnodes, rip, rix, rzero = so.induced_subgraph(ip, ix, walks.reshape(-1), "keep")
            assert np.array_equal(nodes.cpu().numpy(), rnodes)
            assert np.array_equal(sub.indptr.cpu().numpy(), rip) and np.array_equal(sub.indices.cpu().numpy(), rix)
            assert sub.n_dst == sub.n_src == len(rnodes) and sub.num_edges() == len(rix)
            assert sub._cache["zero_in"] == (rzero > 0) and sub.has_zero_in_degree() == (rzero > 0)
            assert np.array_equal(local.cpu().numpy(), np.flatnonzero(is_train[rnodes]))          # ALL training nodes present, not only the roots
            assert len(local) >= len(roots)
    shuffled = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 3, shuffle=True, seed=5)
    roots_seen = torch.cat([nodes[:1] for _, nodes, _ in shuffled])              # (the first node of a batch is its first root)
    assert len(roots_seen) == 3 and is_train[roots_seen.cpu().numpy()].all()


@pytest.mark.parametrize("name", ["GCN", "APPNP", "GAT", "GCNII"])
def test_train_subgraph_equals_a_hand_loop_of_train(name):
    """Three batches of train_subgraph against train() over CSRGraph.subgraph of the ORACLE's node sets: the same kernels and the same
    step counter (so the same dropout seeds) on the same arrays -- every parameter is bit-equal."""
    from glnn_amd import teacher
    from glnn_amd.graph import RandomWalkSubgraphLoader
    from glnn_amd.train_and_eval import train, train_subgraph
    ip, ix, g = _sym_graph()
    rs = np.random.RandomState(2)
    d_in, n_cls = 20, 5
    x = _t(rs.randn(N, d_in).astype(np.float32))
    y = _t(rs.randint(0, n_cls, N).astype(np.int64))
    idx_train = rs.choice(N, 96, replace=False).astype(np.int64)
    train_mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    train_mask[_t(idx_train)] = True
    crit = torch.nn.NLLLoss()

    m1 = _model(name, d_in, n_cls)
    opt1 = torch.optim.Adam(m1.parameters(), lr=0.01, weight_decay=5e-4)
    loader = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 3, shuffle=False, seed=9)
    loss1 = train_subgraph(m1, loader, x, y, crit, opt1)
    assert teacher.get_engine(m1, opt1).step_count == 3

    m2 = _model(name, d_in, n_cls)
    opt2 = torch.optim.Adam(m2.parameters(), lr=0.01, weight_decay=5e-4)
    losses = []
    for b in range(3):
        walks = so.random_walk(ip, ix, idx_train[b * 32:(b + 1) * 32], 3, loader.rng_seed(1, b))
        nodes = _t(so.first_appearance(walks.reshape(-1)))
        sub = g.subgraph(nodes)
        local = torch.nonzero(train_mask[nodes]).reshape(-1)
        losses.append(train(m2, sub, x[nodes], y[nodes], crit, opt2, local))
    for (k1, p1), (k2, p2) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(p1, p2), k1
    assert np.isfinite(loss1) and loss1 == pytest.approx(np.mean(losses), rel=1e-6)          # (one fp32 running sum against three host reads)
    assert int(opt1.state[next(m1.parameters())]["step"]) == 3


def test_keep_raises_the_zero_in_degree_error_on_a_directed_graph_and_add_does_not():
    from glnn_amd.graph import CSRGraph, RandomWalkSubgraphLoader
    from glnn_amd.train_and_eval import train_subgraph
    ip, ix = random_graph(N, 3.0, seed=41, isolated=5)                       # directed; five rows without in-edges
    g = CSRGraph(_t(ip), _t(ix), N)
    rs = np.random.RandomState(3)
    x = _t(rs.randn(N, 12).astype(np.float32))
    y = _t(rs.randint(0, 4, N).astype(np.int64))
    iso = np.flatnonzero(np.diff(ip) == 0)
    idx_train = np.concatenate([iso[:1], np.setdiff1d(np.arange(N), iso)[:31]]).astype(np.int64)         # a degree-0 root: its row is empty under "keep"
    crit = torch.nn.NLLLoss()
    m = _model("GCN", 12, 4)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    keep = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 2, self_loop="keep", shuffle=False, seed=1)
    with pytest.raises(RuntimeError, match="0-in-degree"):
        train_subgraph(m, keep, x, y, crit, opt)
    add = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 2, self_loop="add", shuffle=False, seed=1)
    loss = train_subgraph(m, add, x, y, crit, opt)
    assert np.isfinite(loss)
    for sub, _, _ in add:
        assert not sub.has_zero_in_degree()


def test_cli_trains_a_gcn_teacher_on_subgraphs(tmp_path):
    conf = tmp_path / "conf.yaml"
    conf.write_text("global: {hidden_dim: 64, num_layers: 2}\ncora:\n  GCN: {dropout_ratio: 0, weight_decay: 0.001}\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py"), "--dataset", "synthetic-cora", "--teacher", "GCN",
                        "--device", "0", "--subgraph_walk_length", "2", "--batch_size", "32", "--max_epoch", "30", "--log_level", "10",
                        "--model_config_path", str(conf)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    tdir = tmp_path / "outputs" / "transductive" / "synthetic-cora" / "GCN" / "seed_0"
    out = np.load(tdir / "out.npz")["arr_0"]
    assert out.shape == (2485, 7) and np.isfinite(out).all()                  # one row per node of the GRAPH: evaluation stays full-graph
    losses = [float(v) for v in re.findall(r"Ep\s+\d+ \| loss: ([0-9.]+)", (tdir / "log").read_text())]
    print("epoch mean losses:", losses)
    assert len(losses) == 30 and losses[-1] < losses[0]
