"""The kept layer-1 neighbour aggregate of SAGE.inference (glnn_sage_fused_agg_f32, ops.sage_fused(agg_out= / agg_in=),
SAGE._input_aggregate): A1 = (A x + x) / (deg+1) depends on the graph and the features only, so the first forward over a (graph, feats)
stores it and later ones read it back.  The read-back launch runs the gathering launch's own projection code over the same rows: every
comparison between the two here is torch.equal, never a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

from graphgen import random_graph
from oracle import teacher_oracle as to
from test_model_gpu import DEV, TOL, _sage_model

pytestmark = pytest.mark.gpu

N = 4001          # a tail tile (4001 = 125 * 32 + 1), isolated rows, rows above 128 edges, one hub row above 1024
_GRAPHS = {}


def _graph(seed=7):
    """(indptr, indices) as numpy and on the device: one graph per seed, shared by every test (read-only)."""
    if seed not in _GRAPHS:
        indptr, indices = random_graph(N, 10, seed, power=0.6, isolated=4, hub=1500)
        deg = np.diff(indptr)
        assert deg.max() > 1024 and (deg > 128).sum() > 1 and (deg == 0).sum() >= 4
        _GRAPHS[seed] = (indptr, indices, torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV))
    return _GRAPHS[seed]


def _agg_buffer(d_in, ld=None, device=DEV):
    """A NaN-filled [N, ld] buffer and its [N, d_in] view (ld: d_in rounded up to 4, like ops.feat_empty)."""
    ld = (d_in + 3) // 4 * 4 if ld is None else ld
    buf = torch.full((N, ld), float("nan"), dtype=torch.float32, device=device)
    return buf, buf[:, :d_in]


# ------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("order", [False, True], ids=["id_order", "tile_order"])
@pytest.mark.parametrize("chain", [False, True], ids=["plain", "chained"])
@pytest.mark.parametrize("d_in,d_out", [(100, 256), (7, 48), (104, 256), (256, 256), (64, 200)])
def test_fused_launch_writes_the_aggregate_and_reads_it_back_to_the_same_bits(d_in, d_out, chain, order):
    from glnn_amd import ops
    indptr, indices, ip, ix = _graph()
    rs = np.random.RandomState(d_in * 1000 + d_out)
    x = torch.from_numpy(rs.standard_normal((N, d_in)).astype(np.float32)).to(DEV)
    w = torch.from_numpy((rs.standard_normal((d_out, d_in)) * 0.1).astype(np.float32)).to(DEV)
    scale = torch.from_numpy(rs.uniform(.5, 1.5, d_out).astype(np.float32)).to(DEV)
    shift = torch.from_numpy(rs.uniform(-.2, .2, d_out).astype(np.float32)).to(DEV)
    w_next = torch.from_numpy((rs.standard_normal((47, d_out)) * 0.1).astype(np.float32)).to(DEV) if chain else None
    kw = dict(ep_scale=scale, ep_shift=shift, relu=True, w_next=w_next, tile_order=ops.fused_tile_order(ip, N) if order else None)

    def both(res):
        return res if chain else (res, None)

    out0, next0 = both(ops.sage_fused(ip, ix, x, N, w, **kw))
    # (a) the launch that also stores the aggregate stores the same outputs
    buf, agg = _agg_buffer(d_in)
    out1, next1 = both(ops.sage_fused(ip, ix, x, N, w, agg_out=agg, **kw))
    assert torch.equal(out1, out0) and (not chain or torch.equal(next1, next0))
    # (b) the aggregate itself against an fp64 recomputation; its padding columns are zero
    deg = torch.from_numpy(np.diff(indptr)).to(DEV)
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), deg)
    want = x.double().index_add(0, rows, x.double()[ix.long()]) / (deg.double() + 1)[:, None]
    assert float((agg.double() - want).abs().max()) <= TOL
    assert buf.shape[1] == d_in or bool((buf[:, d_in:] == 0).all())
    # (c) the launch that reads it back: the same bits, also when only the chained projection is written
    out2, next2 = both(ops.sage_fused(None, None, None, N, w, agg_in=agg, **kw))
    assert torch.equal(out2, out0) and (not chain or torch.equal(next2, next0))
    if chain:
        none, next3 = ops.sage_fused(ip, ix, x, N, w, agg_in=agg, want_out=False, **kw)
        assert none is None and torch.equal(next3, next0)


def test_aggregate_with_a_wide_leading_dimension_and_reused_output_buffers():
    """ld_agg beyond the padded width: columns [d_in, d_in rounded up to 8) are written as zeros, the rest of a row is not touched, and
    the read-back launch gives the same bits into caller-provided buffers."""
    from glnn_amd import ops
    _, _, ip, ix = _graph()
    d_in, d_out = 7, 48
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.standard_normal((N, d_in)).astype(np.float32)).to(DEV)
    w = torch.from_numpy((rs.standard_normal((d_out, d_in)) * 0.1).astype(np.float32)).to(DEV)
    out0 = ops.sage_fused(ip, ix, x, N, w)
    buf, agg = _agg_buffer(d_in, ld=16)
    assert torch.equal(ops.sage_fused(ip, ix, x, N, w, agg_out=agg), out0)
    assert bool((buf[:, d_in:8] == 0).all()) and bool(torch.isnan(buf[:, 8:]).all())
    out = ops.feat_empty(N, d_out, DEV, zero=True)
    assert ops.sage_fused(None, None, None, N, w, agg_in=agg, out=out) is out and torch.equal(out, out0)


def test_bad_aggregate_arguments_are_an_error_status_not_a_crash():
    from glnn_amd import _lib, ops
    _, _, ip, ix = _graph()
    d_in, d_out = 100, 64
    x = ops.feat_empty(N, d_in, DEV, zero=True)
    out = ops.feat_empty(N, d_out, DEV)
    agg = ops.feat_empty(N, d_in, DEV)
    wp = ops.pack_weight(torch.zeros(d_out, d_in, device=DEV))
    h = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(agg_out, agg_in, ld_agg, graph=True):
        g_ = (p(ip), p(ix), N, N, p(x), x.stride(0), d_in, p(x), x.stride(0)) if graph else (None, None, N, 0, None, 0, d_in, None, 0)
        return h.glnn_sage_fused_agg_f32(*g_, p(wp), d_out, None, None, 0, p(out), out.stride(0), None, 0, None, 0, None, None,
                                         agg_out, agg_in, ld_agg, None)

    assert call(p(agg), p(agg), 100) == -1 and b"exactly one" in h.glnn_last_error()
    assert call(None, None, 100) == -1 and b"exactly one" in h.glnn_last_error()
    for ld in (98, 96, 102):                                    # not a multiple of 4 / narrower than d_in rounded up to 4
        assert call(p(agg), None, ld) == -1 and b"ld_agg" in h.glnn_last_error()
        assert call(None, p(agg), ld, graph=False) == -1 and b"ld_agg" in h.glnn_last_error()
    assert call(None, ctypes.c_void_p(agg.data_ptr() + 4), 100, graph=False) == -1 and b"alignment" in h.glnn_last_error()
    assert call(p(agg), None, 100, graph=False) == -1 and b"null pointer" in h.glnn_last_error()     # the miss path needs its graph
    with pytest.raises(ValueError):
        ops.sage_fused(ip, ix, x, N, torch.zeros(d_out, d_in, device=DEV), agg_out=agg, agg_in=agg)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- model level
MODEL_CASES = [(dims, norm) for dims in ([100, 256, 256, 47], [64, 48, 48, 12], [100, 256, 47]) for norm in ("batch", "none", "layer")]


def _model(dims, norm, seed):
    if norm != "layer":
        return _sage_model(dims, norm, seed)[0]
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type="layer", device=DEV))
    with torch.no_grad():
        for nm in model.encoder.norms:
            nm.weight.uniform_(.5, 1.5)
            nm.bias.uniform_(-.2, .2)
        for lay in model.encoder.layers:
            lay.fc_neigh.bias.normal_(0, .1)
    return model.eval()


def _fresh_copy(model, dims, norm):
    from glnn_amd.models import Model
    other = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type=norm, device=DEV))
    other.load_state_dict(model.state_dict())
    return other.eval()


def _oracle(indptr, indices, x, model, norm):
    """The numpy oracle at the model's CURRENT state (LayerNorm, which to.sage_inference does not have, as float64 numpy per layer)."""
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    L = model.encoder.num_layers
    layers = [dict(weight=sd[f"encoder.layers.{i}.fc_neigh.weight"], bias=sd[f"encoder.layers.{i}.fc_neigh.bias"]) for i in range(L)]
    if norm != "layer":
        norms = [dict(weight=sd[f"encoder.norms.{i}.weight"], bias=sd[f"encoder.norms.{i}.bias"], running_mean=sd[f"encoder.norms.{i}.running_mean"],
                      running_var=sd[f"encoder.norms.{i}.running_var"]) for i in range(L - 1)] if norm == "batch" else None
        return to.sage_inference(indptr, indices, x, layers, norms)
    h = np.ascontiguousarray(x, np.float32)
    for i, lay in enumerate(layers):
        h = to.sage_conv_gcn(indptr, indices, h, lay["weight"], lay["bias"])
        if i != L - 1:
            z = h.astype(np.float64)
            z = (z - z.mean(1, keepdims=True)) / np.sqrt(z.var(1, keepdims=True) + model.encoder.norms[i].eps)
            h = np.ascontiguousarray(np.maximum(z * sd[f"encoder.norms.{i}.weight"] + sd[f"encoder.norms.{i}.bias"], 0), np.float32)
    return h


def _launches(fn):
    """(result, [(name, info)] of the launches ops.set_timing saw during fn())."""
    from glnn_amd import ops
    rec = []
    ops.set_timing(rec)
    try:
        res = fn()
    finally:
        ops.set_timing(None)
    return res, [(name, info) for name, info, _, _ in rec]


def _gathers(launches, d):
    return [1 for name, info in launches if name in ("sage_fused", "spmm") and info["d"] == d]


def _setup(dims, norm, seed=3):
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    indptr, indices, ip, ix = _graph()
    x = np.random.RandomState(seed).standard_normal((N, dims[0])).astype(np.float32)
    model = _model(dims, norm, seed)
    loader = FullNeighborLoader(CSRGraph(ip, ix, N), 512)
    return indptr, indices, x, model, loader, torch.from_numpy(x).to(DEV)


@pytest.mark.parametrize("dims,norm", MODEL_CASES)
def test_second_inference_reads_the_aggregate_and_equals_the_first(dims, norm, monkeypatch):
    from glnn_amd.models import SAGE
    indptr, indices, x, model, loader, feats = _setup(dims, norm)
    d_in = dims[0]
    cached = model.encoder.layers[0].fused_eligible()
    first, l1 = _launches(lambda: model.inference(loader, feats))
    second, l2 = _launches(lambda: model.inference(loader, feats))
    assert first.data_ptr() != second.data_ptr() and torch.equal(second, first)
    with monkeypatch.context() as m:
        m.setattr(SAGE, "CACHE_INPUT_AGGREGATE", False)
        off, l3 = _launches(lambda: model.inference(loader, feats))
    assert torch.equal(off, first)
    np.testing.assert_allclose(second.cpu().numpy(), _oracle(indptr, indices, x, model, norm), atol=TOL, rtol=0)
    assert not [1 for name, info in l2 if name == "sage_fused" and info["d"] == d_in]
    assert len([1 for name, info in l2 if name == "gemm" and info["k"] == d_in]) == 1
    if cached:            # (a layer 0 that projects first has nothing to keep: its calls are the same launches every time)
        assert len(_gathers(l1, d_in)) == 1 and len(_gathers(l3, d_in)) == 1 and not _gathers(l2, d_in)
        assert not [1 for name, info in l1 if name == "gemm" and info["k"] == d_in]
    else:
        assert [n_ for n_, _ in l1] == [n_ for n_, _ in l2] == [n_ for n_, _ in l3]


@pytest.mark.parametrize("dims,norm", MODEL_CASES)
def test_weight_updates_keep_the_aggregate_and_feature_or_graph_changes_drop_it(dims, norm, monkeypatch):
    from glnn_amd.graph import CSRGraph, FullNeighborLoader, MultiLayerNeighborSampler, NodeDataLoader
    from glnn_amd.models import SAGE
    from glnn_amd.teacher import TeacherEngine
    indptr, indices, x, model, loader, feats = _setup(dims, norm, seed=5)
    g, d_in = loader.graph, dims[0]
    cached = model.encoder.layers[0].fused_eligible()
    model.inference(loader, feats)

    def same_as_a_fresh_uncached_model(what):
        model.eval()
        got, launches = _launches(lambda: model.inference(loader, feats))
        with monkeypatch.context() as m:
            m.setattr(SAGE, "CACHE_INPUT_AGGREGATE", False)
            want = _fresh_copy(model, dims, norm).inference(loader, feats)
        assert torch.equal(got, want), what
        if cached:
            assert not _gathers(launches, d_in), what            # the weights changed, the aggregate did not: no new gather of the features
        return got

    a = same_as_a_fresh_uncached_model("unchanged")
    with torch.no_grad():
        model.encoder.layers[0].fc_neigh.weight.mul_(1.5)
        model.encoder.layers[-1].fc_neigh.bias.add_(0.3)
    b = same_as_a_fresh_uncached_model("in-place update")
    assert float((a - b).abs().max()) > 1e-3
    model.load_state_dict({k: (v * 0.9 if v.dtype.is_floating_point else v) for k, v in model.state_dict().items()})
    same_as_a_fresh_uncached_model("load_state_dict")
    labels = torch.from_numpy(np.random.RandomState(4).randint(0, dims[-1], N)).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    model.train()
    eng = TeacherEngine(model, opt)
    nl = NodeDataLoader(g, torch.arange(512), MultiLayerNeighborSampler([4] * (len(dims) - 1)), batch_size=512, shuffle=False, seed=1)
    for input_nodes, output_nodes, blocks in nl:
        eng.step_sage(blocks, feats, labels, output_nodes, 1.0, input_nodes=input_nodes)
    c = same_as_a_fresh_uncached_model("one TeacherEngine step")
    assert float((c - b).abs().max()) > 1e-4

    def recomputed(loader_, feats_, ip_, ix_, x_, what):
        got, launches = _launches(lambda: model.inference(loader_, feats_))
        np.testing.assert_allclose(got.cpu().numpy(), _oracle(ip_, ix_, x_, model, norm), atol=TOL, rtol=0, err_msg=what)
        if cached:
            assert len(_gathers(launches, d_in)) == 1, what
            _, again = _launches(lambda: model.inference(loader_, feats_))
            assert not _gathers(again, d_in), what
        return got

    feats.mul_(0.5)
    recomputed(loader, feats, indptr, indices, 0.5 * x, "features modified in place")
    x2 = np.random.RandomState(9).standard_normal((N, d_in)).astype(np.float32)
    recomputed(loader, torch.from_numpy(x2).to(DEV), indptr, indices, x2, "another feature tensor on the same graph")
    indptr2, indices2, ip2, ix2 = _graph(seed=8)
    recomputed(FullNeighborLoader(CSRGraph(ip2, ix2, N), 512), feats, indptr2, indices2, 0.5 * x, "the same features on another graph")


def test_release_placed_drops_the_aggregate_and_an_allocation_failure_leaves_the_forward_alone(monkeypatch):
    from glnn_amd import ops
    dims, norm = [100, 256, 47], "batch"
    indptr, indices, x, model, loader, feats = _setup(dims, norm, seed=6)
    first = model.inference(loader, feats)
    assert "_agg_x" in model.encoder.__dict__
    model.encoder.release_placed()
    assert "_agg_x" not in model.encoder.__dict__
    again, launches = _launches(lambda: model.inference(loader, feats))
    assert torch.equal(again, first) and len(_gathers(launches, dims[0])) == 1 and "_agg_x" in model.encoder.__dict__
    model.encoder.release_placed()
    real = ops.feat_empty

    def no_room_for_the_aggregate(rows, d, device, zero=False):
        if d == dims[0]:
            raise torch.cuda.OutOfMemoryError("no memory for the kept aggregate")
        return real(rows, d, device, zero=zero)
    monkeypatch.setattr(ops, "feat_empty", no_room_for_the_aggregate)
    for _ in range(2):
        got, launches = _launches(lambda: model.inference(loader, feats))
        assert torch.equal(got, first) and len(_gathers(launches, dims[0])) == 1 and "_agg_x" not in model.encoder.__dict__
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (4 * N * dims[0], 1 << 40))      # free memory under twice the matrix
    monkeypatch.setattr(ops, "feat_empty", real)
    got, launches = _launches(lambda: model.inference(loader, feats))
    assert torch.equal(got, first) and len(_gathers(launches, dims[0])) == 1 and "_agg_x" not in model.encoder.__dict__
