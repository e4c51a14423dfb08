"""GPU checks of neighbour-sampled SAGE inference (csrc/sample_csr.hip, CSRGraph.sampled, SAGE.inference(fan_out=...);
docs/SAMPLED_INFERENCE_SEMANTICS.md).

The integers are exact: a sampled graph equals the compaction of tests/sampling_oracle.py's sample_neighbors over seeds = arange(n).  The
forward is bit-identical to the same layers run over CSRGraphs built on the host from those arrays (same kernels, same inputs) and within
rtol = atol = 1e-4 (tests/parity_rules.py) of an fp64 forward over them; the bf16 case is held to the bound of
tests/test_bf16_inference_gpu.py's end-to-end test (2e-3 of the row's largest value, against an fp64 forward that rounds to bf16 at the
storage points)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sage_mean_oracle as mo
import sampled_inference_cases as sc
from parity_rules import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr_graph(ip, ix, n_dst, n_src=sc.N):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(np.array(ip[:n_dst + 1])).to(DEV), torch.from_numpy(np.array(ix[:ip[n_dst]])).to(DEV), n_dst, n_src)


def _graph(which, n_dst=sc.N):
    ip, ix = sc.big_graph() if which == "big" else sc.small_degree_graph()
    return _csr_graph(ip, ix, n_dst)


def _arrays(g):
    return g.indptr.cpu().numpy(), g.indices.cpu().numpy()


# ---- 1. the integers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sc.SEEDS)
@pytest.mark.parametrize("fanout", sc.FANOUTS)
def test_sampled_graph_equals_the_oracle(fanout, seed):
    ip, ix = sc.big_graph()
    want_ip, want_ix, n_redirects = sc.expected("big", fanout, seed)
    if fanout >= 5:
        assert n_redirects >= 1, "the oracle reports no redirected pick: the duplicate rule would go untested"
    deg = np.diff(ip)
    assert (np.diff(want_ip) == np.minimum(deg, fanout)).all()
    s = _graph("big").sampled(fanout, seed)
    got_ip, got_ix = _arrays(s)
    assert s.n_dst == sc.N and s.n_src == sc.N and got_ip.dtype == np.int64 and got_ix.dtype == np.int32
    assert np.array_equal(got_ip, want_ip)
    assert s.num_edges() == int(want_ip[-1]) == len(got_ix)
    assert np.array_equal(got_ix, want_ix)
    for row in sc.ISOLATED:
        assert got_ip[row + 1] == got_ip[row]
    row = sc.PLANTED[fanout]                                             # deg == fanout: copied in row order
    assert np.array_equal(got_ix[got_ip[row]:got_ip[row + 1]], ix[ip[row]:ip[row + 1]])
    row = sc.PLANTED[fanout + 1]                                         # deg == fanout + 1: drawn -- one entry of the row is left out
    assert got_ip[row + 1] - got_ip[row] == fanout


@pytest.mark.parametrize("fanout", [5, 33])
def test_sampled_graph_of_several_scan_tiles(fanout):
    """5003 rows: five tiles of the row-count scan (its look-back runs), a ragged last workgroup of the fill."""
    import sampling_oracle as so
    from graphgen import random_graph
    n = 5003
    ip, ix = random_graph(n, 9, seed=3, power=0.6, isolated=7, hub=1500)
    src, cnt, n_redirects = so.sample_neighbors(ip, ix, np.arange(n), fanout, sc.SEEDS[1])
    want_ip, want_ix = sc.compact(src, cnt)
    assert n_redirects >= 1 and (np.diff(ip) > fanout).sum() >= 100
    s = _csr_graph(ip, ix, n, n).sampled(fanout, sc.SEEDS[1])
    got_ip, got_ix = _arrays(s)
    assert np.array_equal(got_ip, want_ip) and s.num_edges() == int(want_ip[-1])
    assert np.array_equal(got_ix, want_ix)


# ---- 2. row independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanout", sc.FANOUTS)
def test_first_rows_alone_give_the_same_rows(fanout):
    seed = sc.SEEDS[0]
    whole_ip, whole_ix = _arrays(_graph("big").sampled(fanout, seed))
    part = _graph("big", sc.FIRST_ROWS).sampled(fanout, seed)
    part_ip, part_ix = _arrays(part)
    assert part.n_dst == sc.FIRST_ROWS and part.n_src == sc.N
    assert np.array_equal(part_ip, whole_ip[:sc.FIRST_ROWS + 1])
    assert np.array_equal(part_ix, whole_ix[:whole_ip[sc.FIRST_ROWS]])
    want_ip, want_ix, _ = sc.expected("big", fanout, seed, sc.FIRST_ROWS)
    assert np.array_equal(part_ip, want_ip) and np.array_equal(part_ix, want_ix)


# ---- 3. equal results ----------------------------------------------------------------------------------------------------------
def test_same_seed_same_graph_and_seeds_differ_on_the_hub():
    g = _graph("big")
    for fanout in (5, 16, 33):
        a, b = g.sampled(fanout, sc.SEEDS[0]), g.sampled(fanout, sc.SEEDS[0])
        assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
        assert a.indices.data_ptr() != b.indices.data_ptr() and a._cache is not b._cache and a._cache is not g._cache
        assert a.ndata is not g.ndata
        c = g.sampled(fanout, sc.SEEDS[1])
        ip = a.indptr.cpu().numpy()
        lo, hi = ip[sc.HUB], ip[sc.HUB + 1]
        assert hi - lo == fanout and not torch.equal(a.indices[lo:hi], c.indices[lo:hi])
    # the sampled indptr and its edge count are kept per fan-out on the parent: one host read per (graph, fanout)
    assert set(k for k in g._cache if isinstance(k, tuple) and k[0] == "sampled_indptr") == {("sampled_indptr", f) for f in (5, 16, 33)}
    assert g.sampled(5, 1).indptr.data_ptr() == g.sampled(5, 2).indptr.data_ptr()


def test_fanout_at_the_largest_degree_keeps_the_graph():
    g = _graph("small")
    ip, ix = sc.small_degree_graph()
    for seed in sc.SEEDS:
        s = g.sampled(64, seed)
        assert torch.equal(s.indptr, g.indptr) and torch.equal(s.indices, g.indices) and s.num_edges() == len(ix)


# ---- models ---------------------------------------------------------------------------------------------------------------------
DIMS = {2: [12, 40, 5], 3: [100, 256, 256, 47]}          # aggregate-first layers and a project-first last layer in both
FAN_OUT = {2: [5, 9], 3: [17, 8, 33]}
SAMPLE_SEED = 20240


def _model(dims, norm, aggregator, seed=4):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.0,
                       norm_type=norm, device=DEV, sage_aggregator=aggregator))
    with torch.no_grad():
        for nm in model.encoder.norms:
            nm.weight.uniform_(0.5, 1.5)
            nm.bias.uniform_(-0.2, 0.2)
            if norm == "batch":
                nm.running_mean.uniform_(-0.3, 0.3)
                nm.running_var.uniform_(0.5, 2.0)
        for lay in model.encoder.layers:
            lay.fc_neigh.bias.uniform_(-0.2, 0.2)
            if aggregator == "mean":
                lay.fc_self.bias.uniform_(-0.2, 0.2)
    return model.eval()


def _state(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _feats(d):
    f = np.random.RandomState(8).standard_normal((sc.N, d)).astype(np.float32)
    f.setflags(write=False)
    return f


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)          # (a copy: the cached inputs are read-only)


def _agg64(ip, ix, h):
    """sum over in-edges in fp64, per destination row."""
    out = np.zeros((len(ip) - 1, h.shape[1]))
    np.add.at(out, np.repeat(np.arange(len(ip) - 1), np.diff(ip)), h[ix])
    return out


def _tail64(sd, l, L, norm, z, eps=1e-5):
    if l == L - 1:
        return z
    if norm == "batch":
        k = f"encoder.norms.{l}."
        z = (z - sd[k + "running_mean"]) / np.sqrt(sd[k + "running_var"] + eps) * sd[k + "weight"] + sd[k + "bias"]
    elif norm == "layer":
        k = f"encoder.norms.{l}."
        mu = z.mean(1, keepdims=True)
        z = (z - mu) / np.sqrt(((z - mu) ** 2).mean(1, keepdims=True) + eps) * sd[k + "weight"] + sd[k + "bias"]
    return np.maximum(z, 0.0)


def gcn_forward64(sd, L, norm, layers, x, rb=None):
    """fp64 SAGE-"gcn" forward with layer l over layers[l] = (indptr, indices): h <- tail((A_l h + h) / (cnt_l + 1) W_l^T + b_l), cnt_l the
    SAMPLED row's length.  rb (the bf16 case): a rounding applied at the storage points of SAGE._whole_graph_layer_bf16, as
    tests/test_bf16_inference_gpu.py's bf16_storage_oracle does -- layer 0's input when it aggregates first, the chained projection, a
    project-first layer's x W^T, a hidden output the next layer aggregates."""
    W = [sd[f"encoder.layers.{l}.fc_neigh.weight"] for l in range(L)]
    B = [sd[f"encoder.layers.{l}.fc_neigh.bias"] for l in range(L)]
    agg_first = [w.shape[1] <= w.shape[0] for w in W]
    rb = rb or (lambda a: a)

    def mean(l, h):
        ip, ix = layers[l]
        return (_agg64(ip, ix, h) + h[:len(ip) - 1]) / (np.diff(ip) + 1.0)[:, None]

    h = x.astype(np.float64)
    if agg_first[0]:
        h = rb(h)
    proj = None
    for l in range(L):
        if proj is not None:
            y, proj = _tail64(sd, l, L, norm, mean(l, proj) + B[l]), None
        elif l + 1 < L and agg_first[l] and not agg_first[l + 1] and norm != "layer":      # the chained next-layer projection
            proj = rb(_tail64(sd, l, L, norm, mean(l, h) @ W[l].T + B[l]) @ W[l + 1].T)
            continue
        elif not agg_first[l]:
            y = _tail64(sd, l, L, norm, mean(l, rb(h @ W[l].T)) + B[l])
        else:
            y = _tail64(sd, l, L, norm, mean(l, h) @ W[l].T + B[l])
        h = rb(y) if l + 1 < L and agg_first[l + 1] else y
    return h


def _close(got, want, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"{what}: max|err| {err.max():.3e} max|ref| {np.abs(want).max():.3e}")
    bad = err > TOL + TOL * np.abs(want)
    assert not bad.any(), f"{what}: {bad.sum()} elements off, max|err| {err.max():.3e}"


def _host_graphs(layers):
    return [_csr_graph(ip, ix, sc.N) for ip, ix in layers]


# ---- 4. the forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["none", "batch", "layer"])
@pytest.mark.parametrize("aggregator", ["gcn", "mean"])
@pytest.mark.parametrize("L", [2, 3])
def test_sampled_forward(L, aggregator, norm):
    from glnn_amd.graph import FullNeighborLoader
    dims, fan_out = DIMS[L], FAN_OUT[L]
    model = _model(dims, norm, aggregator)
    enc = model.encoder
    if aggregator == "gcn":
        assert enc.layers[0].fused_eligible() and enc.layers[-1]._in_feats > enc.layers[-1]._out_feats
    loader = FullNeighborLoader(_graph("big"), 64)
    feats = _t(_feats(dims[0]))
    got = model.inference(loader, feats, fan_out=fan_out, sample_seed=SAMPLE_SEED)
    assert got.shape == (sc.N, dims[-1]) and got.dtype == torch.float32
    layers = sc.expected_layers("big", fan_out, SAMPLE_SEED)
    explicit = enc.inference_over(_host_graphs(layers), feats)
    assert torch.equal(got, explicit)
    sd = _state(model)
    x64 = _feats(dims[0]).astype(np.float64)
    if aggregator == "gcn":
        want = gcn_forward64(sd, L, norm, layers, x64)
    else:
        want = mo.forward(mo.State(sd, L, norm), [(ip, ix, sc.N) for ip, ix in layers], x64)[0]
    _close(got, want, f"sampled {aggregator} {norm} L={L}")
    # the sampled forward is not the full one (the hub row alone loses 2983 of its 3000 in-edges) ...
    assert not torch.equal(got, model.inference(loader, feats))
    # ... it is a function of (fan_out, sample_seed), and another seed is another draw
    assert torch.equal(got, model.inference(loader, feats, fan_out=fan_out, sample_seed=SAMPLE_SEED))
    assert not torch.equal(got, model.inference(loader, feats, fan_out=fan_out, sample_seed=SAMPLE_SEED + 1))


def test_sampled_forward_bf16():
    from glnn_amd.graph import FullNeighborLoader
    L, norm = 3, "batch"
    dims, fan_out = DIMS[L], FAN_OUT[L]
    model = _model(dims, norm, "gcn")
    loader = FullNeighborLoader(_graph("big"), 64)
    feats = _t(_feats(dims[0]))
    got_t = model.inference(loader, feats, dtype=torch.bfloat16, fan_out=fan_out, sample_seed=SAMPLE_SEED)
    assert got_t.dtype == torch.float32 and got_t.shape == (sc.N, dims[-1])
    layers = sc.expected_layers("big", fan_out, SAMPLE_SEED)
    assert torch.equal(got_t, model.encoder.inference_over(_host_graphs(layers), feats, dtype=torch.bfloat16))
    rb = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)
    want = gcn_forward64(_state(model), L, norm, layers, _feats(dims[0]).astype(np.float64), rb=rb)
    got = got_t.cpu().numpy().astype(np.float64)
    scale = np.maximum(np.abs(want).max(1, keepdims=True), 1e-6)
    print(f"sampled bf16: max relative-to-row error {(np.abs(got - want) / scale).max():.3e}")
    assert (np.abs(got - want) <= 2e-3 * scale).all(), float((np.abs(got - want) / scale).max())


@pytest.mark.parametrize("aggregator,norm,L", [("gcn", "batch", 2), ("gcn", "batch", 3), ("gcn", "layer", 3), ("mean", "batch", 3)])
def test_fanout_64_is_the_full_forward_bit_for_bit(aggregator, norm, L):
    from glnn_amd.graph import FullNeighborLoader
    dims = DIMS[L]
    model = _model(dims, norm, aggregator)
    loader = FullNeighborLoader(_graph("small"), 64)
    feats = _t(_feats(dims[0]))
    full = model.inference(loader, feats).clone()
    assert torch.equal(model.inference(loader, feats, fan_out=[64] * L, sample_seed=3), full)
    assert torch.equal(model.inference(loader, feats), full)            # (the second full call reads the kept layer-1 aggregate)


# ---- 5. no poisoning ------------------------------------------------------------------------------------------------------------
def test_a_sampled_call_leaves_the_full_forward_alone():
    from glnn_amd.graph import FullNeighborLoader
    from glnn_amd.models import SAGE
    assert SAGE.CACHE_INPUT_AGGREGATE
    L = 3
    model = _model(DIMS[L], "batch", "gcn")
    enc = model.encoder
    g = _graph("big")
    loader = FullNeighborLoader(g, 64)
    feats = _t(_feats(DIMS[L][0]))
    first = model.inference(loader, feats).clone()
    kept = enc.__dict__.get("_agg_x")
    assert kept is not None, "the full forward did not keep its layer-1 aggregate: the test would show nothing"
    kept_bits = kept[3].clone()
    state = {k: enc.__dict__.get(k) for k in ("_placed", "_placed_x")}
    sampled = model.inference(loader, feats, fan_out=FAN_OUT[L], sample_seed=SAMPLE_SEED)
    assert not torch.equal(sampled, first)
    assert enc.__dict__.get("_agg_x") is kept and torch.equal(kept[3], kept_bits)
    assert all(enc.__dict__.get(k) is v for k, v in state.items())
    assert "tile_order" not in g._cache and "hub_plan" not in g._cache
    third = model.inference(loader, feats)
    assert torch.equal(first, third)


# ---- refusals that need a device ------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from glnn_amd.graph import FullNeighborLoader
    from glnn_amd.models import Model
    model = _model(DIMS[2], "none", "gcn")
    g = _graph("big")
    loader = FullNeighborLoader(g, 64)
    feats = _t(_feats(12))
    with pytest.raises(NotImplementedError, match="fan_out"):
        model.encoder.inference(loader, feats, whole_graph=False, fan_out=[5, 5])
    with pytest.raises(ValueError, match="fan_out"):
        model.inference(loader, feats, fan_out=[5, 65])
    gcn = Model(dict(model_name="GCN", num_layers=2, feat_dim=12, hidden_dim=40, label_dim=5, dropout_ratio=0.0, norm_type="none", device=DEV)).eval()
    with pytest.raises(NotImplementedError, match="fan_out"):
        gcn.inference(g, feats, fan_out=[5, 5])
    import ctypes
    from glnn_amd import _lib
    h = _lib.lib()
    ip = g.indptr
    out = torch.empty(sc.N + 1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert h.glnn_sample_csr_indptr(p(ip), sc.N, 65, p(out), None, 0, None) == -1 and b"glnn_sample_csr_indptr" in h.glnn_last_error()
    assert h.glnn_sample_csr_indptr(p(ip), sc.N, 5, p(out), None, 0, None) == -1 and b"glnn_sample_csr_indptr" in h.glnn_last_error()
    assert h.glnn_sample_csr_fill(p(ip), p(g.indices), sc.N, 1 << 31, p(out), 5, 0, p(out), None) == -1 and b"glnn_sample_csr_fill" in h.glnn_last_error()
    assert h.glnn_sample_csr_fill(p(ip), None, sc.N, sc.N, p(out), 5, 0, p(out), None) == -1 and b"null pointer" in h.glnn_last_error()
    assert h.glnn_sample_csr_fill(None, None, 0, 0, None, 5, 0, None, None) == 0


# ---- 6. the command line --------------------------------------------------------------------------------------------------------
def test_teacher_cli_inference_fan_out(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    args = ["--dataset", "synthetic-cora", "--teacher", "SAGE", "--device", "0", "--inference_fan_out", "5,5", "--max_epoch", "3",
            "--patience", "3", "--exp_setting", "tran", "--save_results"]
    outs = []
    for run in ("a", "b"):
        cwd = tmp_path / run
        cwd.mkdir()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py")] + args, cwd=cwd, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out_dir = cwd / "outputs" / "transductive" / "synthetic-cora" / "SAGE" / "seed_0"
        out = np.load(out_dir / "out.npz")["arr_0"]
        assert out.shape == (2485, 7) and out.dtype == np.float32 and np.isfinite(out).all()
        np.testing.assert_allclose(np.exp(out).sum(1), 1.0, atol=1e-4)
        log = (out_dir / "log").read_text()
        assert log.count("inference_fan_out: [5, 5] -- sampled edges per layer") == 1, log[-2000:]
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])
