"""SAGE.inference's dispatch on the GPU: every form (whole-graph fp32 first and second call, whole-graph bf16, the chunked engine sweep,
the reference's literal sweep) of every aggregator and norm issues, name for name and argument for argument, the timed launches it
issued before the forms shared one layer plan and one chunk sweep (recorded then, written out below); the forms agree with each other;
a chunk that raises leaves the loader and the encoder as they were.  bf16 storage exists for "gcn" without LayerNorm only and the literal
sweep for "gcn" only: the other combinations are held to their refusal texts.

A 300-row graph swept in chunks of 64 (five chunks, the last of 44 rows) and two encoders are the smallest shapes that take every branch:
[20, 32, 32, 6] -- layers 0 and 1 aggregate first (fused), layer 1 chains layer 2's projection in the whole-graph form, layer 2 projects
first in the chunked form (one gemm, then the prepared unfused launch); [40, 24, 24, 6] -- layer 0 projects first, layer 1 is fused."""
import functools
import hashlib

import numpy as np
import pytest
import torch

from graphgen import random_graph
from parity_rules import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, BATCH = 300, 64
DIMS = {"wide": [20, 32, 32, 6], "narrow": [40, 24, 24, 6]}
AGGS, NORMS = ("gcn", "mean"), ("none", "batch", "layer")
FORMS = ("whole", "whole_again", "bf16", "engine", "literal")
# (aggregator, norm, form) that SAGE.inference refuses, with a piece of the refusal's text; every other combination has its recorded
# sequence below.  bf16 storage is "gcn" without LayerNorm only; the literal sweep does not exist for "mean" (a loader without a resident
# graph and global-id blocks is refused).
REFUSED = {("gcn", "layer", "bf16"): "LayerNorm teachers are fp32 only"}
REFUSED.update({("mean", n, "bf16"): "implemented for the 'gcn' aggregator only, not for aggregator_type 'mean'" for n in NORMS})
REFUSED.update({("mean", n, "literal"): "aggregator_type 'mean'.: a glnn_amd.graph.FullNeighborLoader over the resident graph" for n in NORMS})

# What ops.set_timing's collector receives during ONE inference call, recorded before the refactor: [launch, how many times in a row],
# a launch written as its name and its info in the collector's order (the prepared ops.RowRangeLaunch names n_dst first, the per-chunk
# ops calls d: the text also says which of the per-chunk forms ran).  The m of a literal sweep's gemm is its block's source rows.
_GCN_WIDE_ENGINE_TAIL = [
    ["gemm(m=300, k=32, n=6)", 1],
    ["spmm(n_dst=64, d=6, mode=1)", 4], ["spmm(n_dst=44, d=6, mode=1)", 1]]
_GCN_WIDE_LITERAL_HIDDEN = [
    ["sage_fused(d=20, n_dst=64, d_out=32, d_chain=0, d_written=32)", 4], ["sage_fused(d=20, n_dst=44, d_out=32, d_chain=0, d_written=32)", 1],
    ["sage_fused(d=32, n_dst=64, d_out=32, d_chain=0, d_written=32)", 4], ["sage_fused(d=32, n_dst=44, d_out=32, d_chain=0, d_written=32)", 1]]
_GCN_NARROW_LITERAL_HIDDEN = [
    ["gemm(m=267, k=40, n=24)", 1], ["spmm(d=24, n_dst=64, mode=1)", 1], ["gemm(m=244, k=40, n=24)", 1], ["spmm(d=24, n_dst=64, mode=1)", 1],
    ["gemm(m=245, k=40, n=24)", 1], ["spmm(d=24, n_dst=64, mode=1)", 1], ["gemm(m=219, k=40, n=24)", 1], ["spmm(d=24, n_dst=64, mode=1)", 1],
    ["gemm(m=186, k=40, n=24)", 1], ["spmm(d=24, n_dst=44, mode=1)", 1],
    ["sage_fused(d=24, n_dst=64, d_out=24, d_chain=0, d_written=24)", 4], ["sage_fused(d=24, n_dst=44, d_out=24, d_chain=0, d_written=24)", 1]]
_RECORDED = [      # (aggregator, norms, dims, forms, the sequence)
    ("gcn", ("none", "batch"), "wide", ("whole",), [
        ["sage_fused(d=20, n_dst=300, d_out=32, d_chain=0, d_written=32)", 1],
        ["sage_fused(d=32, n_dst=300, d_out=32, d_chain=6, d_written=6)", 1],
        ["spmm(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("none", "batch"), "wide", ("whole_again",), [
        ["gemm(m=300, k=20, n=32)", 1],
        ["sage_fused(d=32, n_dst=300, d_out=32, d_chain=6, d_written=6)", 1],
        ["spmm(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("none", "batch"), "wide", ("bf16",), [
        ["sage_fused_bf16(d=20, n_dst=300, d_out=32, d_chain=0, d_written=32)", 1],
        ["sage_fused_bf16(d=32, n_dst=300, d_out=32, d_chain=6, d_written=6)", 1],
        ["spmm_bf16(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("none", "batch"), "wide", ("engine",), [
        ["sage_fused(n_dst=64, d=20, d_out=32, d_chain=0, d_written=32)", 4], ["sage_fused(n_dst=44, d=20, d_out=32, d_chain=0, d_written=32)", 1],
        ["sage_fused(n_dst=64, d=32, d_out=32, d_chain=0, d_written=32)", 4], ["sage_fused(n_dst=44, d=32, d_out=32, d_chain=0, d_written=32)", 1]]
        + _GCN_WIDE_ENGINE_TAIL),
    ("gcn", ("none", "batch", "layer"), "wide", ("literal",), _GCN_WIDE_LITERAL_HIDDEN + [
        ["gemm(m=267, k=32, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1], ["gemm(m=244, k=32, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1],
        ["gemm(m=245, k=32, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1], ["gemm(m=219, k=32, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1],
        ["gemm(m=186, k=32, n=6)", 1], ["spmm(d=6, n_dst=44, mode=1)", 1]]),
    ("gcn", ("none", "batch"), "narrow", ("whole", "whole_again"), [
        ["gemm(m=300, k=40, n=24)", 1], ["spmm(d=24, n_dst=300, mode=1)", 1],
        ["sage_fused(d=24, n_dst=300, d_out=24, d_chain=6, d_written=6)", 1],
        ["spmm(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("none", "batch"), "narrow", ("bf16",), [
        ["gemm(m=300, k=40, n=24)", 1], ["spmm_bf16(d=24, n_dst=300, mode=1)", 1],
        ["sage_fused_bf16(d=24, n_dst=300, d_out=24, d_chain=6, d_written=6)", 1],
        ["spmm_bf16(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("none", "batch"), "narrow", ("engine",), [
        ["gemm(m=300, k=40, n=24)", 1], ["spmm(n_dst=64, d=24, mode=1)", 4], ["spmm(n_dst=44, d=24, mode=1)", 1],
        ["sage_fused(n_dst=64, d=24, d_out=24, d_chain=0, d_written=24)", 4], ["sage_fused(n_dst=44, d=24, d_out=24, d_chain=0, d_written=24)", 1],
        ["gemm(m=300, k=24, n=6)", 1], ["spmm(n_dst=64, d=6, mode=1)", 4], ["spmm(n_dst=44, d=6, mode=1)", 1]]),
    ("gcn", ("none", "batch", "layer"), "narrow", ("literal",), _GCN_NARROW_LITERAL_HIDDEN + [
        ["gemm(m=267, k=24, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1], ["gemm(m=244, k=24, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1],
        ["gemm(m=245, k=24, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1], ["gemm(m=219, k=24, n=6)", 1], ["spmm(d=6, n_dst=64, mode=1)", 1],
        ["gemm(m=186, k=24, n=6)", 1], ["spmm(d=6, n_dst=44, mode=1)", 1]]),
    # LayerNorm: nothing chains behind a hidden layer, and a loader WITH the engine mode sweeps the hidden layers literally, the last as engine
    ("gcn", ("layer",), "wide", ("whole",), [
        ["sage_fused(d=20, n_dst=300, d_out=32, d_chain=0, d_written=32)", 1],
        ["sage_fused(d=32, n_dst=300, d_out=32, d_chain=0, d_written=32)", 1],
        ["gemm(m=300, k=32, n=6)", 1], ["spmm(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("layer",), "wide", ("whole_again",), [
        ["gemm(m=300, k=20, n=32)", 1],
        ["sage_fused(d=32, n_dst=300, d_out=32, d_chain=0, d_written=32)", 1],
        ["gemm(m=300, k=32, n=6)", 1], ["spmm(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("layer",), "wide", ("engine",), _GCN_WIDE_LITERAL_HIDDEN + _GCN_WIDE_ENGINE_TAIL),
    ("gcn", ("layer",), "narrow", ("whole", "whole_again"), [
        ["gemm(m=300, k=40, n=24)", 1], ["spmm(d=24, n_dst=300, mode=1)", 1],
        ["sage_fused(d=24, n_dst=300, d_out=24, d_chain=0, d_written=24)", 1],
        ["gemm(m=300, k=24, n=6)", 1], ["spmm(d=6, n_dst=300, mode=1)", 1]]),
    ("gcn", ("layer",), "narrow", ("engine",), _GCN_NARROW_LITERAL_HIDDEN + [
        ["gemm(m=300, k=24, n=6)", 1], ["spmm(n_dst=64, d=6, mode=1)", 4], ["spmm(n_dst=44, d=6, mode=1)", 1]]),
    # "mean": the tail never changes a launch (LayerNorm is an untimed pass of its own), and nothing is kept between calls
    ("mean", NORMS, "wide", ("whole", "whole_again"), [
        ["sage_mean_fused(d=20, n_dst=300, d_out=32)", 1],
        ["sage_mean_fused(d=32, n_dst=300, d_out=32)", 1],
        ["gemm(m=300, k=32, n=14)", 1], ["spmm_sage_mean(d=6, n_dst=300)", 1]]),
    ("mean", NORMS, "wide", ("engine",), [
        ["sage_mean_fused(d=20, n_dst=64, d_out=32)", 4], ["sage_mean_fused(d=20, n_dst=44, d_out=32)", 1],
        ["sage_mean_fused(d=32, n_dst=64, d_out=32)", 4], ["sage_mean_fused(d=32, n_dst=44, d_out=32)", 1],
        ["gemm(m=300, k=32, n=14)", 1], ["spmm_sage_mean(d=6, n_dst=64)", 4], ["spmm_sage_mean(d=6, n_dst=44)", 1]]),
    ("mean", NORMS, "narrow", ("whole", "whole_again"), [
        ["gemm(m=300, k=40, n=48)", 1], ["spmm_sage_mean(d=24, n_dst=300)", 1],
        ["sage_mean_fused(d=24, n_dst=300, d_out=24)", 1],
        ["gemm(m=300, k=24, n=14)", 1], ["spmm_sage_mean(d=6, n_dst=300)", 1]]),
    ("mean", NORMS, "narrow", ("engine",), [
        ["gemm(m=300, k=40, n=48)", 1], ["spmm_sage_mean(d=24, n_dst=64)", 4], ["spmm_sage_mean(d=24, n_dst=44)", 1],
        ["sage_mean_fused(d=24, n_dst=64, d_out=24)", 4], ["sage_mean_fused(d=24, n_dst=44, d_out=24)", 1],
        ["gemm(m=300, k=24, n=14)", 1], ["spmm_sage_mean(d=6, n_dst=64)", 4], ["spmm_sage_mean(d=6, n_dst=44)", 1]]),
]
SEQUENCE = {f"{a}-{n}-{d}-{f}": seq for a, norms, d, forms, seq in _RECORDED for n in norms for f in forms}      # "aggregator-norm-dims-form"


@functools.lru_cache(maxsize=None)
def _problem(d_in):
    """The graph (three rows without in-edges, one hub of 200) and the features of one input width; made once, never modified."""
    from glnn_amd.graph import CSRGraph
    ip, ix = random_graph(N, 6, seed=7, isolated=3, hub=200)
    deg = np.diff(ip)
    assert (deg == 0).sum() >= 3 and deg.max() >= 200
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), N)
    x = torch.from_numpy(np.random.RandomState(d_in).standard_normal((N, d_in)).astype(np.float32)).to(DEV)
    return g, x


def _encoder(agg, norm, dims):
    from glnn_amd.models import Model
    torch.manual_seed(11)
    model = Model(dict(model_name="SAGE", num_layers=3, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.5,
                       norm_type=norm, sage_aggregator=agg, device=DEV))
    with torch.no_grad():
        for m in model.encoder.norms:
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.2, 0.2)
            if norm == "batch":
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
        for lay in model.encoder.layers:
            lay.fc_neigh.bias.normal_(0, 0.1)
            if agg == "mean":
                lay.fc_self.bias.normal_(0, 0.1)
    return model.eval().encoder


class Plain:
    """A loader WITHOUT the engine mode (tests/test_model_gpu.py builds the same): the literal loop of the reference."""

    def __init__(self, inner):
        self.inner = inner

    def __iter__(self):
        return iter(self.inner)


def _call(enc, loader, x, form):
    if form == "bf16":
        return enc.inference(loader, x, dtype=torch.bfloat16)
    if form == "literal":
        return enc.inference(Plain(loader), x, whole_graph=False)
    return enc.inference(loader, x, whole_graph=form != "engine")


def run(agg, norm, dims_name, form):
    """One timed inference call of a fresh encoder in `form`: (the output, the launches as [[text, repeats], ...])."""
    from glnn_amd import ops
    from glnn_amd.graph import FullNeighborLoader
    g, x = _problem(DIMS[dims_name][0])
    enc, loader = _encoder(agg, norm, DIMS[dims_name]), FullNeighborLoader(g, BATCH)
    assert len(loader) == 5
    if form == "whole_again":                  # the second call over the same graph and features reads the kept layer-1 aggregate
        enc.inference(loader, x)
    timed = []
    ops.set_timing(timed)
    try:
        out = _call(enc, loader, x, form)
    finally:
        ops.set_timing(None)
    torch.cuda.synchronize()
    runs = []
    for name, info, _, _ in timed:
        text = name + "(" + ", ".join(f"{k}={v}" for k, v in info.items()) + ")"
        if runs and runs[-1][0] == text:
            runs[-1][1] += 1
        else:
            runs.append([text, 1])
    return out, runs


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


CASES = [(a, n, d, f) for a in AGGS for n in NORMS for d in DIMS for f in FORMS]


@pytest.mark.parametrize("agg,norm,dims_name,form", CASES)
def test_launches_are_the_recorded_sequence(agg, norm, dims_name, form):
    if (agg, norm, form) in REFUSED:
        with pytest.raises(NotImplementedError, match=REFUSED[agg, norm, form]):
            run(agg, norm, dims_name, form)
        return
    out, runs = run(agg, norm, dims_name, form)
    print(agg, norm, dims_name, form, digest(out), runs)
    assert out.shape == (N, 6) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert runs == SEQUENCE[f"{agg}-{norm}-{dims_name}-{form}"]


@pytest.mark.parametrize("dims_name", list(DIMS))
@pytest.mark.parametrize("norm", NORMS)
def test_mean_chunked_equals_whole_graph_bit_for_bit(norm, dims_name):
    whole, _ = run("mean", norm, dims_name, "whole")
    chunked, _ = run("mean", norm, dims_name, "engine")
    assert torch.equal(whole, chunked)


@pytest.mark.parametrize("dims_name", list(DIMS))
@pytest.mark.parametrize("norm", NORMS)
def test_gcn_chunked_and_literal_agree_with_whole_graph(norm, dims_name):
    whole, _ = run("gcn", norm, dims_name, "whole")
    again, _ = run("gcn", norm, dims_name, "whole_again")
    assert torch.equal(whole, again)
    for form in ("engine", "literal"):
        got, _ = run("gcn", norm, dims_name, form)
        err = float((got - whole).abs().max())
        print(norm, dims_name, form, f"max|diff| {err:.3e}")
        assert err <= TOL


@pytest.mark.parametrize("agg,patched", [("gcn", "RowRangeLaunch.__call__"), ("mean", "sage_mean_fused")])
def test_a_chunk_that_raises_leaves_loader_and_encoder_as_they_were(agg, patched, monkeypatch):
    """The third per-chunk launch fails in Python (nothing faults on the device): inference raises, the loader is out of engine mode, the
    current stream is the caller's again, and the next call computes what the call before the failure did."""
    from glnn_amd import ops
    from glnn_amd.graph import FullNeighborLoader
    g, x = _problem(20)
    enc, loader = _encoder(agg, "batch", DIMS["wide"]), FullNeighborLoader(g, BATCH)
    before = enc.inference(loader, x, whole_graph=False)
    stream = torch.cuda.current_stream()
    calls = []
    owner, attr = (ops.RowRangeLaunch, "__call__") if agg == "gcn" else (ops, "sage_mean_fused")
    real = getattr(owner, attr)

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("third chunk")
        return real(*a, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(owner, attr, failing)
        with pytest.raises(RuntimeError, match="third chunk"):
            enc.inference(loader, x, whole_graph=False)
    assert len(calls) == 3
    assert loader.global_blocks is False
    assert torch.cuda.current_stream() == stream
    torch.cuda.synchronize()
    assert torch.equal(enc.inference(loader, x, whole_graph=False), before)


@pytest.mark.parametrize("agg", AGGS)
def test_a_loader_that_ignores_global_blocks_is_an_error(agg):
    from glnn_amd.graph import FullNeighborLoader
    g, x = _problem(20)

    class Deaf(Plain):
        global_blocks = False

    loader = Deaf(FullNeighborLoader(g, BATCH))
    loader.graph = g
    with pytest.raises(RuntimeError, match="Deaf"):
        _encoder(agg, "none", DIMS["wide"]).inference(loader, x, whole_graph=False)
