"""GPU checks of the GraphSAGE "mean" aggregator (csrc/sage_mean.hip, docs/SAGE_MEAN_SEMANTICS.md) against the fp64 numpy oracle
(tests/sage_mean_oracle.py): the layer in its three eval forms, the equal-result properties of the two kernels, SAGE.inference (whole graph
and chunked sweep, three tails), the refused combinations, and one train_sage epoch through the differentiable ops.

Tolerances: rtol = atol = 1e-4 (tests/parity_rules.py) for every forward value, the loss and the trained parameters; parameter gradients
are allowed that or, where it is more, 4x the distance of the fp32 run of the oracle's own arithmetic from its fp64 run (the bound of
tests/test_gat_gpu.py; the measured distances are printed and recorded in NOTES.md)."""
import functools

import numpy as np
import pytest
import torch

import sage_mean_oracle as mo
from graphgen import csr_from_edges

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
N_SRC = 300
HUB, HUB_EDGES = 17, 3000          # far above the kernels' long-row threshold (128 in-edges: the whole workgroup takes the row)
LONG, LONG_EDGES = 50, 130         # just above it
ISOLATED = (3, 40, 69, 200, 299)
# d_in picks sage_mean_fused_kernel<LPR> (16 / 32 / 64 up to 64 / 128 / 256 columns), d_out picks spmm_sage_mean_kernel<dv> of the
# project-first form in the same way: (12, 65) is the smallest d_out on its <32> (docs/KERNEL_COVERAGE.md)
WIDTHS = [(100, 256), (256, 256), (256, 47), (12, 40), (5, 3), (12, 65)]


@functools.lru_cache(maxsize=None)
def _edges():
    rs = np.random.RandomState(11)
    m = 1500
    src, dst = rs.randint(0, N_SRC, m), rs.randint(0, N_SRC, m)
    keep = ~np.isin(dst, ISOLATED + (HUB, LONG))
    src, dst = src[keep], dst[keep]
    extra_src = [7, 7, 7, 120, 120, 10]               # 7 -> 5 three times and 120 -> 64 twice (multi-edges), the self-loop 10 -> 10
    extra_dst = [5, 5, 5, 64, 64, 10]
    src = np.concatenate([src, extra_src, rs.randint(0, N_SRC, HUB_EDGES), rs.randint(0, N_SRC, LONG_EDGES)])
    dst = np.concatenate([dst, extra_dst, np.full(HUB_EDGES, HUB), np.full(LONG_EDGES, LONG)])
    ip, ix = csr_from_edges(src, dst, N_SRC)
    deg = np.diff(ip)
    assert deg[HUB] == HUB_EDGES and deg[LONG] == LONG_EDGES and all(deg[i] == 0 for i in ISOLATED)
    assert len(np.unique(ix[ip[HUB]:ip[HUB + 1]])) < HUB_EDGES          # drawn with repetition
    return ip, ix


def _csr(n_dst):
    ip, ix = _edges()
    return ip[:n_dst + 1], ix[:ip[n_dst]]


def _graph(n_dst):
    from glnn_amd.graph import CSRGraph
    ip, ix = _csr(n_dst)
    return CSRGraph(torch.from_numpy(ip.copy()).to(DEV), torch.from_numpy(ix.copy()).to(DEV), n_dst, N_SRC)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(d_in, d_out):
    """Inputs of one width (fp32 values) and the oracle's fp64 answers without bias for n_dst = 300; computed once, never modified."""
    rs = np.random.RandomState(d_in * 1000 + d_out)
    x = rs.standard_normal((N_SRC, d_in)).astype(np.float32)
    ws = (rs.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    wn = (rs.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    bs, bn = (rs.standard_normal(d_out) * 0.1).astype(np.float32), (rs.standard_normal(d_out) * 0.1).astype(np.float32)
    es, eh = rs.uniform(0.5, 1.5, d_out).astype(np.float32), (rs.standard_normal(d_out) * 0.3).astype(np.float32)
    ip, ix = _csr(N_SRC)
    ref = mo.layer(ip, ix, x.astype(np.float64), ws, None, wn, None)
    ref.setflags(write=False)
    return dict(x=x, ws=ws, wn=wn, bs=bs, bn=bn, es=es, eh=eh, ref=ref)


def _layer(d_in, d_out):
    from glnn_amd.nn import SAGEConv
    c = _case(d_in, d_out)
    lay = SAGEConv(d_in, d_out, "mean").to(DEV)
    with torch.no_grad():
        lay.fc_self.weight.copy_(_t(c["ws"])); lay.fc_self.bias.copy_(_t(c["bs"]))
        lay.fc_neigh.weight.copy_(_t(c["wn"])); lay.fc_neigh.bias.copy_(_t(c["bn"]))
    return lay.eval(), c


def _forms(d_in, d_out):
    return (["fused"] if d_in <= d_out <= 256 else []) + ["project", "compose"]


def _close(got, want, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"{what}: max|err| {err.max():.3e} max|ref| {np.abs(want).max():.3e}")
    bad = err > TOL + TOL * np.abs(want)
    assert not bad.any(), f"{what}: {bad.sum()} elements off, max|err| {err.max():.3e}"


def _nan_out(n, d):
    buf = torch.full((n, (d + 3) // 4 * 4), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[:, :d]


@pytest.mark.parametrize("n_dst", [300, 70])
@pytest.mark.parametrize("d_in,d_out", WIDTHS)
def test_layer_matches_the_oracle(d_in, d_out, n_dst):
    """The form SAGEConv picks for the width, without and with the fused tail (scale, shift, ReLU); the padding columns of a float4-
    addressable output row come out as zeros."""
    lay, c = _layer(d_in, d_out)
    assert lay.mean_form() == ("project" if d_in > d_out else "fused")
    g = _graph(n_dst)
    x = _t(c["x"])
    ref = c["ref"][:n_dst]
    with torch.no_grad():
        buf, out = _nan_out(n_dst, d_out)
        y = lay(g, (x, x[:n_dst]), out=out)
        _close(y, ref + (c["bs"].astype(np.float64) + c["bn"]), f"{d_in}->{d_out} n_dst={n_dst} plain")
        assert y.data_ptr() == out.data_ptr() and not torch.isnan(buf).any() and (buf[:, d_out:] == 0).all()
        buf, out = _nan_out(n_dst, d_out)
        y = lay(g, (x, x[:n_dst]), ep_scale=_t(c["es"]), ep_shift=_t(c["eh"]), relu=True, out=out)
        _close(y, np.maximum(ref * c["es"] + c["eh"], 0), f"{d_in}->{d_out} n_dst={n_dst} tail")
        assert not torch.isnan(buf).any() and (buf[:, d_out:] == 0).all()
        if d_out >= 32:
            assert (y == 0).any() and (y > 0).any()          # the ReLU did something


@pytest.mark.parametrize("d_in,d_out", [(100, 256), (12, 40), (3, 5)])
def test_self_rows_indirection(d_in, d_out):
    """self_rows: destination v's own row is x_self[self_rows[v]] -- the same bits as the direct launch over the permuted rows."""
    from glnn_amd import ops
    lay, c = _layer(d_in, d_out)
    ip, ix = _csr(70)
    ipd, ixd = torch.from_numpy(ip.copy()).to(DEV), torch.from_numpy(ix.copy()).to(DEV)
    x = _t(c["x"])
    perm = torch.from_numpy(np.random.RandomState(3).permutation(N_SRC)[:70].astype(np.int64)).to(DEV)
    wn, ws = lay.fc_neigh.weight.detach(), lay.fc_self.weight.detach()
    direct = ops.sage_mean_fused(ipd, ixd, x, 70, wn, ws, x_self=ops.as_feat(x[perm].contiguous()), ep_shift=_t(c["eh"]))
    through = ops.sage_mean_fused(ipd, ixd, x, 70, wn, ws, x_self=x, self_rows=perm, ep_shift=_t(c["eh"]))
    assert torch.equal(direct, through)
    want = mo.layer(ip, ix, c["x"].astype(np.float64), c["ws"], None, c["wn"], None)          # self rows 0..69 ...
    want = want - c["x"][:70].astype(np.float64) @ c["ws"].astype(np.float64).T + c["x"][perm.cpu().numpy()].astype(np.float64) @ c["ws"].astype(np.float64).T
    _close(through, want + c["eh"], f"{d_in}->{d_out} self_rows")


@pytest.mark.parametrize("d_in,d_out", WIDTHS)
def test_equal_result_properties(d_in, d_out):
    """Bit for bit: two runs of one launch; rows [0, 70) launched alone against the same rows of the whole-graph launch; with and without
    a tile order.  For every single-launch form the width has."""
    from glnn_amd import ops
    lay, c = _layer(d_in, d_out)
    x = _t(c["x"])
    g300, g70 = _graph(300), _graph(70)
    es, eh = _t(c["es"]), _t(c["eh"])
    with torch.no_grad():
        for form in [f for f in _forms(d_in, d_out) if f != "compose"]:
            a = lay.forward_mean(g300, (x, x), ep_scale=es, ep_shift=eh, relu=True, form=form).clone()
            b = lay.forward_mean(g300, (x, x), ep_scale=es, ep_shift=eh, relu=True, form=form)
            assert torch.equal(a, b), form
            part = lay.forward_mean(g70, (x, x[:70]), ep_scale=es, ep_shift=eh, relu=True, form=form)
            assert torch.equal(part, a[:70]), form
        if d_in <= d_out:
            wn, ws = lay.fc_neigh.weight.detach(), lay.fc_self.weight.detach()
            plain = ops.sage_mean_fused(g300.indptr, g300.indices, x, 300, wn, ws, ep_scale=es, ep_shift=eh, relu=True)
            order = torch.from_numpy(np.random.RandomState(1).permutation(10).astype(np.int32)).to(DEV)
            ordered = ops.sage_mean_fused(g300.indptr, g300.indices, x, 300, wn, ws, ep_scale=es, ep_shift=eh, relu=True, tile_order=order)
            assert torch.equal(plain, ordered)


@pytest.mark.parametrize("d_in,d_out", WIDTHS)
def test_forms_agree(d_in, d_out):
    """The fused launch, the composition (aggregation with a row scale + two GEMMs) and the project-first form on the same layer."""
    lay, c = _layer(d_in, d_out)
    x = _t(c["x"])
    g = _graph(300)
    want = c["ref"] + (c["bs"].astype(np.float64) + c["bn"])
    with torch.no_grad():
        outs = {form: lay.forward_mean(g, (x, x), form=form) for form in _forms(d_in, d_out)}
    assert len(outs) >= 2
    for form, y in outs.items():
        _close(y, want, f"{d_in}->{d_out} {form}")
    names = list(outs)
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            a, b = outs[names[i]].double(), outs[names[j]].double()
            assert bool(((a - b).abs() <= TOL + TOL * b.abs()).all()), (names[i], names[j], float((a - b).abs().max()))


# ---- SAGE.inference -------------------------------------------------------------------------------------------------------------
DIMS = [20, 32, 32, 6]


def _model(norm, dims=DIMS, seed=4):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.0,
                       norm_type=norm, device=DEV, sage_aggregator="mean"))
    with torch.no_grad():
        for nm in model.encoder.norms:
            nm.weight.uniform_(0.5, 1.5)
            nm.bias.uniform_(-0.2, 0.2)
            if norm == "batch":
                nm.running_mean.uniform_(-0.3, 0.3)
                nm.running_var.uniform_(0.5, 2.0)
        for lay in model.encoder.layers:
            lay.fc_self.bias.uniform_(-0.2, 0.2)
            lay.fc_neigh.bias.uniform_(-0.2, 0.2)
    return model


def _state(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _feats(d=DIMS[0]):
    f = np.random.RandomState(8).standard_normal((N_SRC, d)).astype(np.float32)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("norm", ["batch", "none", "layer"])
def test_inference_whole_graph_equals_the_chunked_sweep_and_the_oracle(norm):
    from glnn_amd.graph import FullNeighborLoader
    model = _model(norm).eval()
    g = _graph(300)
    feats = _t(_feats())
    whole = model.inference(FullNeighborLoader(g, 64), feats)
    chunked = model.encoder.inference(FullNeighborLoader(g, 64), feats, whole_graph=False)
    assert whole.shape == (300, 6) and torch.equal(whole, chunked)
    ip, ix = _csr(300)
    want = mo.inference(mo.State(_state(model), 3, norm), ip, ix, 300, _feats().astype(np.float64))
    _close(whole, want, f"inference {norm}")
    # the sampled-block eval forward (SAGE.forward) over full-neighbour blocks is the same function
    with torch.no_grad():
        blocks = model(([g] * 3), feats)
    _close(blocks, want, f"eval forward {norm}")


def test_refused_combinations_name_the_aggregator():
    from glnn_amd import dist, ops
    from glnn_amd.graph import FullNeighborLoader
    model = _model("batch").eval()
    enc = model.encoder
    g = _graph(300)
    feats = _t(_feats())
    loader = FullNeighborLoader(g, 64)
    with pytest.raises(NotImplementedError, match="mean"):          # the chained next-layer projection (the "gcn" engine's layer call)
        enc._whole_graph_layer(1, g, ops.as_feat(feats), None)
    with pytest.raises(NotImplementedError, match="mean"):          # the kept layer-1 aggregate
        enc._input_aggregate(g, feats, ops.as_feat(feats))
    with pytest.raises(NotImplementedError, match="mean"):
        enc.layers[0](g, (feats, feats), agg_out=ops.feat_empty(300, 20, DEV))
    with pytest.raises(NotImplementedError, match="mean"):          # bf16 activation storage
        model.inference(loader, feats, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="mean"):
        enc.layers[0].forward_bf16(g, ops.to_bf16(feats), ops.to_bf16(feats))
    shards = dist.ShardSpec(300, 1, 0) if hasattr(dist, "ShardSpec") else None
    with pytest.raises(NotImplementedError, match="mean"):          # the sharded teacher forwards
        dist.ShardedTeacher(enc, g, shards, ops)
    with pytest.raises(NotImplementedError, match="mean"):
        dist.HaloShardedTeacher(enc, g, shards, ops)
    with pytest.raises(NotImplementedError):
        from glnn_amd.nn import SAGEConv
        SAGEConv(8, 8, "pool")


# ---- training -------------------------------------------------------------------------------------------------------------------
def _batches(g):
    from glnn_amd.graph import MultiLayerNeighborSampler, NodeDataLoader
    dev = list(NodeDataLoader(g, torch.arange(128), MultiLayerNeighborSampler([3, 3]), batch_size=64, shuffle=False, seed=5))
    assert len(dev) == 2
    host = []
    for inp, outn, blocks in dev:
        assert inp is not None
        host.append((inp.cpu().numpy(), outn.cpu().numpy(),
                     [(b.indptr.cpu().numpy(), b.indices.cpu().numpy(), b.num_src_nodes()) for b in blocks]))
    return dev, host


@pytest.mark.parametrize("norm", ["none", "layer"])
def test_train_sage_epoch_matches_the_oracle(norm):
    """One train_sage epoch of two batches (fan-out 3,3; dropout 0) through SAGE.forward's differentiable ops, torch's NLLLoss and Adam:
    the mean loss, the gradients of the first and of the last batch and the parameters after the two Adam steps."""
    from glnn_amd import train_and_eval as te
    dims = [20, 32, 6]
    lr = 1e-3
    g = _graph(300)
    feats, featsd = _feats(), _t(_feats())
    labels = np.random.RandomState(2).randint(0, 6, N_SRC).astype(np.int64)
    labelsd = torch.from_numpy(labels).to(DEV)
    dev, host = _batches(g)
    crit = torch.nn.NLLLoss()

    def run(nb):
        model = _model(norm, dims)
        sd0 = _state(model)
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        loss = te.train_sage(model, dev[:nb], featsd, labelsd, crit, opt)
        st64, st32 = mo.State(sd0, 2, norm), mo.State(sd0, 2, norm, dtype=np.float32)
        want, per64 = mo.train_sage(st64, host[:nb], feats, labels, lr)
        _, per32 = mo.train_sage(st32, host[:nb], feats, labels, lr)
        return model, loss, want, per64[-1][1], per32[-1][1], st64

    for nb in (1, 2):
        model, loss, want, g64, g32, st64 = run(nb)
        print(f"{norm} batches={nb}: loss {loss:.6f} oracle {want:.6f}")
        assert abs(loss - want) < TOL + TOL * abs(want)
        for k, prm in model.named_parameters():
            got, ref = prm.grad.detach().cpu().numpy().astype(np.float64), g64[k]
            e32 = np.abs(g32[k].astype(np.float64) - ref).max()
            err = np.abs(got - ref)
            print(f"{norm} batches={nb} {k}: max|err| {err.max():.3e} max|ref| {np.abs(ref).max():.3e} fp32 stand-in max|err| {e32:.3e}")
            tol = np.maximum(TOL + TOL * np.abs(ref), 4.0 * e32)
            assert not (err > tol).any(), f"{k}: max|err| {err.max():.3e}, fp32 stand-in {e32:.3e}"
        if nb == 2:
            for k, v in _state(model).items():
                if "num_batches_tracked" not in k:
                    np.testing.assert_allclose(v, st64.p[k], atol=TOL, rtol=0, err_msg=k)
