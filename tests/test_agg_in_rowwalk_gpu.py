"""The kept-aggregate hit path through the wave-walk GEMM (glnn_sage_fused_agg_f32 with agg_in -> glnn::gemm_rowwalk_packed, K3w of
csrc/gemm_rowpanel.hip reading the packed weight).  Per output element the walk issues the MFMA chain of the fused kernel's phase B over the
same operands (the derivation stands above sage_fused_agg_in in csrc/spmm.hip), so every comparison here is torch.equal: the gathering
launch that wrote the aggregate, the hit through the walk, and the hit with GLNN_AGG_IN_ROWWALK=0 (sage_fused_kernel<.., kAggIn>).
Which kernel ran is read from the device kernel names torch.profiler records -- the library has no counter, and ops.set_timing calls the hit
a "gemm" on either route."""
import numpy as np
import pytest
import torch

from graphgen import random_graph
from test_model_gpu import DEV, _sage_model

pytestmark = pytest.mark.gpu

WALK, FUSED = "gemm_rowwalk_kernel", "sage_fused_kernel"
_GRAPHS, _FEATS = {}, {}


def _graph(m):
    """One graph per size, shared and read-only: mean degree ~6 and one row above the long-row threshold (128 edges), so that the agg_out
    launch stores the aggregate from both of its store sites."""
    if m not in _GRAPHS:
        indptr, indices = random_graph(m, 6, seed=m, hub=200)
        assert np.diff(indptr).max() > 128
        _GRAPHS[m] = (torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV))
    return _GRAPHS[m]


def _feats(m, d_in):
    if (m, d_in) not in _FEATS:
        _FEATS[m, d_in] = torch.from_numpy(np.random.RandomState(m + d_in).standard_normal((m, d_in)).astype(np.float32)).to(DEV)
    return _FEATS[m, d_in]


def _kernels(fn):
    """(fn(), names of the device kernels launched meanwhile)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return res, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _case(m, d_in, d_out, epi, relu, chain=False):
    """The inputs of one case and the gathering launch's results: (kw, agg, out0, next0)."""
    from glnn_amd import ops
    ip, ix = _graph(m)
    x = _feats(m, d_in)
    rs = np.random.RandomState(1000 * d_in + d_out)
    w = torch.from_numpy((rs.standard_normal((d_out, d_in)) * 0.1).astype(np.float32)).to(DEV)
    scale = torch.from_numpy(rs.uniform(.5, 1.5, d_out).astype(np.float32)).to(DEV) if epi else None
    shift = torch.from_numpy(rs.uniform(-.2, .2, d_out).astype(np.float32)).to(DEV) if epi else None
    w_next = torch.from_numpy((rs.standard_normal((47, d_out)) * 0.1).astype(np.float32)).to(DEV) if chain else None
    kw = dict(w=w, ep_scale=scale, ep_shift=shift, relu=relu, w_next=w_next)
    buf = torch.full((m, ops.round4(d_in)), float("nan"), dtype=torch.float32, device=DEV)
    agg = buf[:, :d_in]
    res = ops.sage_fused(ip, ix, x, m, agg_out=agg, **kw)
    out0, next0 = res if chain else (res, None)
    assert not bool(torch.isnan(buf).any()) and (buf.shape[1] == d_in or bool((buf[:, d_in:] == 0).all()))
    return kw, agg, out0, next0


def _hit(m, agg, kw, d_out):
    """The read-back launch into a NaN-filled output (an element it does not write fails torch.equal): (out, out_next or None, kernels)."""
    from glnn_amd import ops
    out = ops.feat_empty(m, d_out, DEV)
    out.fill_(float("nan"))
    res, names = _kernels(lambda: ops.sage_fused(None, None, None, m, agg_in=agg, out=out, **kw))
    got, nxt = res if kw["w_next"] is not None else (res, None)
    assert got is out
    return out, nxt, [n for n in names if WALK in n or FUSED in n]


# m: 2048 = the fewest rows the walk takes; 4131 = 129 wave tiles + 3 rows (a partial last tile, waves with unequal tile counts).
# d_in: 36 = the shortest reduction; 37: k = 40, the stored pad columns are zeros; 100: 13 k-groups, the upper half of the last one behind
# k; 128 = the longest.  d_out: 96 = the narrowest, one short panel; 200: a partial second panel and a partial last 32-column tile of the
# packing; 256: two full panels.  Every d_in meets d_out = 256; scale / shift and ReLU on and off.
KERNEL_CASES = [(2048, 36, 256, True, True), (4131, 37, 256, True, True), (4131, 100, 256, True, True), (2048, 128, 256, False, False),
                (4131, 100, 96, True, False), (2048, 37, 200, False, True), (4131, 128, 200, True, True), (2048, 36, 96, False, False),
                (4131, 100, 256, False, True)]


@pytest.mark.parametrize("m,d_in,d_out,epi,relu", KERNEL_CASES)
def test_hit_through_the_wave_walk_equals_the_gathering_launch_and_the_fused_hit(m, d_in, d_out, epi, relu, monkeypatch):
    kw, agg, out0, _ = _case(m, d_in, d_out, epi, relu)
    on, _, k_on = _hit(m, agg, kw, d_out)
    monkeypatch.setenv("GLNN_AGG_IN_ROWWALK", "0")
    off, _, k_off = _hit(m, agg, kw, d_out)
    assert len(k_on) == 1 and WALK in k_on[0], k_on
    assert len(k_off) == 1 and FUSED in k_off[0], k_off
    assert torch.equal(on, out0) and torch.equal(off, out0) and torch.equal(on, off)


FALLBACK_CASES = {
    "m_2047": (2047, 100, 256, False, {}),
    "d_in_32": (2048, 32, 256, False, {}),
    "d_out_64": (2048, 100, 64, False, {}),
    "chained": (2048, 100, 256, True, {}),
    "rowpanel_0": (2048, 100, 256, False, {"GLNN_GEMM_ROWPANEL": "0"}),
    "rowpanel_2": (2048, 100, 256, False, {"GLNN_GEMM_ROWPANEL": "2"}),
}


@pytest.mark.parametrize("name", list(FALLBACK_CASES))
def test_shapes_and_switches_the_walk_does_not_take_run_the_fused_hit(name, monkeypatch):
    """Outside the walk's range the launch is sage_fused_kernel<.., kAggIn> as before: no error, the same bits as with the switch off."""
    m, d_in, d_out, chain, env = FALLBACK_CASES[name]
    kw, agg, out0, next0 = _case(m, d_in, d_out, True, True, chain=chain)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, nxt, k_got = _hit(m, agg, kw, d_out)
    monkeypatch.setenv("GLNN_AGG_IN_ROWWALK", "0")
    off, nxt_off, k_off = _hit(m, agg, kw, d_out)
    for names in (k_got, k_off):
        assert len(names) == 1 and FUSED in names[0], names
    assert torch.equal(got, out0) and torch.equal(off, out0)
    if chain:
        assert torch.equal(nxt, next0) and torch.equal(nxt_off, next0)


def test_model_hits_run_the_walk_and_equal_the_cold_and_the_uncached_forward(monkeypatch):
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    from glnn_amd.models import SAGE
    m, dims = 4131, [100, 256, 256, 47]
    ip, ix = _graph(m)
    feats = _feats(m, dims[0])
    model = _sage_model(dims, "batch", 3)[0]
    loader = FullNeighborLoader(CSRGraph(ip, ix, m), 512)

    def uncached():
        with monkeypatch.context() as mp:
            mp.setattr(SAGE, "CACHE_INPUT_AGGREGATE", False)
            return model.inference(loader, feats)

    cold, k_cold = _kernels(lambda: model.inference(loader, feats))
    hit, k_hit = _kernels(lambda: model.inference(loader, feats))
    assert not [n for n in k_cold if WALK in n] and len([n for n in k_hit if WALK in n]) == 1
    assert cold.data_ptr() != hit.data_ptr() and torch.equal(hit, cold) and torch.equal(uncached(), cold)
    with torch.no_grad():
        model.encoder.layers[0].fc_neigh.weight.mul_(1.5)
        model.encoder.norms[0].bias.add_(0.1)
    hit2, k_hit2 = _kernels(lambda: model.inference(loader, feats))
    assert len([n for n in k_hit2 if WALK in n]) == 1
    assert torch.equal(hit2, uncached()) and float((hit2 - hit).abs().max()) > 1e-3
