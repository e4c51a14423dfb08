"""The four kernel families of csrc/spmm.hip that only the SAGE "gcn" training step launches, each checked as ONE operation -- device
buffers in, device buffer out, fp64 in between (tests/sage_step_kernel_oracle.py) -- row by row, within the derived bound
(T + 16) * 2^-24 * condition:

  spmm_csr_short_kernel        layer 0's aggregation of a sparse block                 (glnn::spmm_csr_nnz)
  spmm_csr_kernel<.., XF>      layer 1's aggregation with layer 0's tail in the gather (glnn::spmm_csr_tail)
  spmm_bn_dy_kernel            transposed aggregation + first BatchNorm-backward pass  (glnn::spmm_csr_bn_dy)
  spmm_ln_dz_kernel            transposed aggregation + the LayerNorm backward         (glnn::spmm_csr_ln_dz)

A two-layer TeacherEngine.step_sage on the planted batch (tests/sage_step_graphs.py) runs each family once; the step's scratch survives
the call (eng._sage_desc holds raw pointers into eng._arena).  Every test prints the largest error / bound it saw (pytest -s)."""
import functools
import time

import numpy as np
import pytest
import torch

import sage_step_graphs as sg
import sage_step_kernel_oracle as ko

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = np.float64


def scratch(eng, ptr, rows, ld, dtype=torch.float32):
    """[rows, ld] view of the step's scratch behind the raw pointer `ptr` of a descriptor field."""
    off = int(ptr) - eng._arena.data_ptr()
    nbytes = rows * ld * torch.empty((), dtype=dtype).element_size()
    assert 0 <= off and off + nbytes <= eng._arena.numel(), "the pointer does not lie inside the engine's arena"
    return eng._arena[off:off + nbytes].view(dtype).view(rows, ld)


def _host(t):
    return t.detach().cpu().numpy()


def _graph(indptr, indices, n_src):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(np.asarray(indptr, np.int64)).to(DEV), torch.from_numpy(np.asarray(indices, np.int32)).to(DEV),
                    len(indptr) - 1, n_src)


@functools.lru_cache(maxsize=None)
def _planted():
    b = sg.planted_batch()
    return b, [_graph(*blk) for blk in b["blocks"]]


@functools.lru_cache(maxsize=None)
def _large():
    b = sg.large_batch()
    return b, [_graph(*blk) for blk in b["blocks"]]


class Step:
    """One checked step: the inputs on the host and every buffer the kernels read or wrote, as numpy arrays."""


def run_step(b, blocks, f, h, norm, p, global_ids=False):
    """A first step allocates the arena; the arena is filled with NaN; the second step is the one that is read back.  lr = 0 and
    weight_decay = 0: the Adam launch inside the call leaves every parameter where the oracle has it."""
    from glnn_amd import ops
    from glnn_amd.models import Model
    from glnn_amd.teacher import TeacherEngine
    (ip0, ix0, n_src0), (ip1, ix1, n_dst0) = b["blocks"]
    n_dst1 = len(ip1) - 1
    x, labels, sd = sg.case_inputs(f, h, norm, n_rows=n_src0, n_out=n_dst1)
    torch.manual_seed(7)
    model = Model(dict(model_name="SAGE", num_layers=2, feat_dim=f, hidden_dim=h, label_dim=sg.N_CLASSES, dropout_ratio=p, norm_type=norm,
                       device=DEV))
    state = model.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            state[k].copy_(torch.from_numpy(v))
    model.train()
    eng = TeacherEngine(model, torch.optim.Adam(model.parameters(), lr=0.0, weight_decay=0.0))
    blk0 = blocks[0]
    if global_ids:          # as NodeDataLoader sets them: the aggregation gathers from the global matrix, the self rows by id
        inp, gidx, dstn = sg.global_ids(b, n_src0 + 1000)
        feats_h = np.full((n_src0 + 1000, f), np.nan, np.float32)      # (a row outside the block is never read)
        feats_h[inp] = x
        blk0 = _graph(ip0, ix0, n_src0)
        blk0.gindices, blk0.dst_nodes = torch.from_numpy(gidx).to(DEV), torch.from_numpy(dstn).to(DEV)
        input_nodes = torch.from_numpy(inp).to(DEV)
    else:
        feats_h, input_nodes = x, torch.arange(n_src0, device=DEV)
    feats = ops.as_feat(torch.from_numpy(feats_h).to(DEV))
    lab, outn = torch.from_numpy(labels).to(DEV), torch.arange(n_dst1, device=DEV)
    args = ([blk0, blocks[1]], feats, lab, outn, 1.0)
    eng.step_sage(*args, input_nodes=input_nodes)
    torch.cuda.synchronize()
    arena = eng._arena
    n4 = arena.numel() // 4 * 4
    arena[:n4].view(torch.float32).fill_(float("nan"))
    eng.step_sage(*args, input_nodes=input_nodes)
    torch.cuda.synchronize()
    assert eng._arena is arena and eng.gather_tail
    d, s = eng._sage_desc, Step()
    y0, y1 = d.layer[0], d.layer[1]
    assert y0.h is None                                     # layer 0's tail is evaluated in layer 1's gather
    s.b, s.f, s.h, s.norm, s.p, s.x, s.sd, s.global_ids = b, f, h, norm, p, x, sd, global_ids
    s.n_dst0, s.n_dst1 = n_dst0, n_dst1
    s.agg0 = _host(scratch(eng, y0.agg, n_dst0, y0.ld_agg))
    s.z0 = _host(scratch(eng, y0.z, n_dst0, y0.ldz))
    s.agg1 = _host(scratch(eng, y1.agg, n_dst1, y1.ld_agg))
    s.dagg = _host(scratch(eng, d.dagg, n_dst1, d.ld_dagg))
    s.dh = _host(scratch(eng, d.dh, n_dst0, d.ld_dh))
    s.inv_deg = _host(scratch(eng, y1.inv_deg, 1, n_dst1))[0]
    s.t_indptr = _host(scratch(eng, y1.t_indptr, 1, n_dst0 + 1, torch.int64))[0]
    s.t_indices = _host(scratch(eng, y1.t_indices, 1, len(ix1) + n_dst1, torch.int32))[0]
    if norm == "batch":
        s.mean, s.rstd, s.a_scale, s.a_shift = (_host(scratch(eng, q, 1, h))[0] for q in (y0.mean, y0.rstd, y0.a_scale, y0.a_shift))
    elif norm == "layer":
        q = eng._sage_ln.layer[0]
        s.mean, s.rstd = _host(scratch(eng, q.mean, 1, n_dst0))[0], _host(scratch(eng, q.rstd, 1, n_dst0))[0]
    s.mask = _host(ops.dropout_mask(n_dst0, h, p, eng._seed(0), DEV)) if p > 0 else None
    enc = model.encoder
    s.gb0 = _host(eng.grad(enc.layers[0].fc_neigh.bias))
    if norm != "none":
        s.ggamma, s.gbeta = _host(eng.grad(enc.norms[0].weight)), _host(eng.grad(enc.norms[0].bias))
        assert np.array_equal(_host(enc.norms[0].weight), sd["encoder.norms.0.weight"])      # lr = 0: Adam moved nothing
    s.ws_bn_floats = int(d.ws_bn_floats)
    assert np.isfinite(float(eng.loss_out.item()))
    return s


def compare(what, got, want, tol, skip=None, rows_info=None):
    """max error / bound over the elements that are compared; exact equality where the bound is 0; nothing NaN.  A miss names the row."""
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite elements"
    err = np.abs(got - want)
    live = np.ones(err.shape, bool) if skip is None else ~np.broadcast_to(skip, err.shape)
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(live, ratio, 0.0)
    worst = tuple(int(i) for i in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    r = float(ratio[worst])
    info = "" if rows_info is None else f", {rows_info(worst[0])}"
    print(f"{what}: error / bound = {r:.4f} at {worst}")
    assert r <= 1.0, f"{what}: error / bound = {r:.3f} at {worst}: got {float(got[worst])!r}, fp64 {float(want[worst])!r}, bound {float(np.asarray(tol)[worst])!r}{info}"
    return r


def zero_padding(what, buf, d):
    assert np.isfinite(buf).all(), f"{what}: NaN"
    assert buf.shape[1] >= d
    assert not buf[:, d:].any(), f"{what}: padding columns [{d}, {buf.shape[1]}) are not exact zeros"


def dscale(p):
    """1 / (1 - p) as the library rounds it (an input of the kernels, like the mask)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_of(s):
    """The keep mask as the oracle takes it (it divides by 1 - p): kept elements weigh dscale(p) after that division."""
    return None if s.mask is None else s.mask.astype(F64) * (dscale(s.p) * (1.0 - s.p))


# ------------------------------------------------------------------------------------------------ the four operations
def check_short(s):
    ip0, ix0, _ = s.b["blocks"][0]
    f = s.f
    x = s.x.astype(F64)
    want, cond, d1 = ko.sage_mean(ip0, ix0, x, np.abs(x))
    zero_padding("layer[0].agg", s.agg0, f)
    deg = np.diff(ip0)
    return compare("short-row aggregation", s.agg0[:, :f], want, ko.bound(d1, cond), rows_info=lambda r: f"row {r} has {deg[r]} in-edges")


def tail_of(s):
    z, h = s.z0[:, :s.h], s.h
    if s.norm == "layer":
        return ko.tail_ln(z, s.mean, s.rstd, s.sd["encoder.norms.0.weight"], s.sd["encoder.norms.0.bias"], keep_of(s), s.p)
    if s.norm == "batch":
        return ko.tail_bn(z, s.a_scale, s.a_shift, keep_of(s), s.p)
    return ko.tail_bn(z, None, None, keep_of(s), s.p)


def check_tail_gather(s):
    ip1, ix1, _ = s.b["blocks"][1]
    hv, hc = tail_of(s)
    want, cond, d1 = ko.sage_mean(ip1, ix1, hv, hc)
    zero_padding("layer[1].agg", s.agg1, s.h)
    deg = np.diff(ip1)
    return compare("tail in the gather", s.agg1[:, :s.h], want, ko.bound(d1, cond), rows_info=lambda r: f"row {r} has {deg[r]} in-edges")


def transposed(s):
    t_ip, t_ix = s.b["t1"]
    assert np.array_equal(s.t_indptr, t_ip) and np.array_equal(s.t_indices, t_ix)      # the device's transposed block has these rows
    np.testing.assert_allclose(s.inv_deg, 1.0 / (np.diff(s.b["blocks"][1][0]) + 1.0), rtol=2e-7, atol=0)
    return ko.transposed_sum(t_ip, t_ix, s.dagg[:, :s.h], s.inv_deg)


def undecided_caps(s, und):
    """At most 0.1 % of the rows hold an undecided gate, and no planted row does."""
    rows = np.flatnonzero(und.any(1))
    assert len(rows) <= s.n_dst0 // 1000, f"{len(rows)} rows with an undecided ReLU gate"
    assert not set(rows) & set(s.b.get("t_planted", sg.backward_planted_rows(s.b))), "a planted row has an undecided ReLU gate"
    return rows


def check_bn_dy(s):
    da, dac, terms = transposed(s)
    r = ko.bn_dy(da, dac, s.z0[:, :s.h], s.mean, s.rstd, s.a_scale, s.a_shift, keep_of(s), s.p)
    undecided_caps(s, r["undecided"])
    tlen = terms[:, 0]
    info = lambda row: f"row {row} of the transposed block has {int(tlen[row])} entries"
    zero_padding("dh", s.dh, s.h)
    ratios = [compare("bn_dy epilogue: dy", s.dh[:, :s.h], r["dy"][0], ko.bound(terms, r["dy"][1]), skip=r["undecided"], rows_info=info)]
    ratios.append(compare("bn_dy epilogue: dbeta", s.gbeta, r["S1"][0], ko.bound(s.n_dst0, r["S1"][1]) + r["flip"][0]))
    ratios.append(compare("bn_dy epilogue: dgamma", s.ggamma, r["S2"][0], ko.bound(s.n_dst0, r["S2"][1]) + r["flip"][1]))
    assert not s.gb0.any()      # the deferred form: the bias in front of the BatchNorm has gradient exactly 0
    return max(ratios)


def bn_dy_fuses(s):
    """glnn::spmm_csr_bn_dy's predicate (behind the deferred apply: float4 rows, feature width > 64)."""
    return 64 < s.h <= 256 and s.h % 4 == 0 and s.f > 64


def ln_dz_fuses(s):
    """glnn::spmm_csr_ln_dz's predicate: hidden <= 256 and a workspace of glnn_sage_step_ws_ln_floats floats."""
    from glnn_amd import _lib
    return s.h <= 256 and s.ws_bn_floats >= int(_lib.lib().glnn_sage_step_ws_ln_floats(s.n_dst0, s.h))


def check_ln_dz(s):
    da, dac, terms = transposed(s)
    r = ko.ln_dz(da, dac, s.z0[:, :s.h], s.mean, s.rstd, s.sd["encoder.norms.0.weight"], s.sd["encoder.norms.0.bias"], keep_of(s), s.p)
    undecided_caps(s, r["undecided"])
    skip = r["undecided"].any(1)[:, None]                   # an undecided gate moves its whole row of dz
    tlen = terms[:, 0]
    info = lambda row: f"row {row} of the transposed block has {int(tlen[row])} entries"
    zero_padding("dh", s.dh, s.h)
    ratios = [compare("ln_dz epilogue: dz", s.dh[:, :s.h], r["dz"][0], ko.bound(terms + s.h, r["dz"][1]), skip=skip, rows_info=info)]
    ratios.append(compare("ln_dz epilogue: dgamma", s.ggamma, r["dgamma"][0], ko.bound(s.n_dst0, r["dgamma"][1]) + r["flip"][1]))
    ratios.append(compare("ln_dz epilogue: dbeta", s.gbeta, r["dbeta"][0], ko.bound(s.n_dst0, r["dbeta"][1]) + r["flip"][0]))
    ratios.append(compare("ln_dz epilogue: sum dz", s.gb0, r["sum_dz"][0], ko.bound(s.n_dst0, r["sum_dz"][1]) + r["flip"][2]))
    return max(ratios)


# ------------------------------------------------------------------------------------------------ the tests
def _ids(cases):
    return [pytest.param(*c, id="-".join(str(v) for v in c)) for c in cases]


def test_constants_of_the_builder_are_the_library_s():
    from glnn_amd import _lib
    assert _lib.lib().glnn_hub_row_threshold() == sg.HUB_ROW and _lib.lib().glnn_hub_segment_edges() == sg.HUB_SEG


@pytest.mark.parametrize("f,h,norm,p", _ids([(sg.F_STEP, h, norm, p) for h in sg.TAIL_H for norm in sg.NORMS for p in sg.PS]))
def test_tail_in_the_gather_matches_fp64(f, h, norm, p):
    """spmm_csr_kernel<LPR, U, SAGE, false, XF>: LPR 4 | 8 | 16 | 32 | 64 at both ends of its width class, XF 1 (BatchNorm affine, none)
    and 2 (LayerNorm), with and without dropout; layer[1].agg row by row."""
    b, blocks = _planted()
    check_tail_gather(run_step(b, blocks, f, h, norm, p))


@pytest.mark.parametrize("f,h,norm,p,ids", _ids([(f, 16, "none", 0.0, ids) for f in sg.SHORT_F for ids in ("local", "global")]))
def test_short_row_aggregation_matches_fp64(f, h, norm, p, ids):
    """spmm_csr_short_kernel<32 | 64>: four rows per ticket over the planted block 0 (batch, carried tail, lone row, skipped long row,
    ragged last ticket), with local ids and with the global ids of a loader's outermost block (the self_rows lane load)."""
    b, blocks = _planted()
    ip0, ix0, _ = b["blocks"][0]
    assert len(ix0) <= 6 * sg.N_DST0 and f > 64 and sg.row_geometry(sg.N_DST0)[2] % sg.SHORT_ROWS == 0      # the dispatcher's predicate
    check_short(run_step(b, blocks, f, h, norm, p, global_ids=ids == "global"))


@pytest.mark.parametrize("f,h,norm,p", _ids([(sg.F_STEP, h, "batch", p) for h in sg.BN_DY_H for p in sg.PS]))
def test_bn_dy_epilogue_matches_fp64(f, h, norm, p):
    """spmm_bn_dy_kernel<32 | 64, U, DROP>: dy row by row, dgamma and dbeta against the fp64 column sums, the bias gradient exactly 0."""
    b, blocks = _planted()
    s = run_step(b, blocks, f, h, norm, p)
    assert bn_dy_fuses(s)
    check_bn_dy(s)


@pytest.mark.parametrize("f,h,norm,p", _ids([(sg.F_STEP, h, "layer", p) for h in sg.LN_DZ_H for p in sg.PS]))
def test_ln_dz_epilogue_matches_fp64(f, h, norm, p):
    """spmm_ln_dz_kernel<8 | 16 | 32 | 64, U, DROP>: dz row by row (inv_h = 1 / h over the real columns, padding columns exact zeros), and
    the three folded column sums."""
    b, blocks = _planted()
    s = run_step(b, blocks, f, h, norm, p)
    assert ln_dz_fuses(s)
    check_ln_dz(s)


@pytest.mark.parametrize("f,h,norm,p", _ids([(68, 68, norm, 0.3) for norm in ("batch", "layer")]))
def test_large_n_launch_geometry(f, h, norm, p):
    """All three kernels of the step at 16 rows per wave, a ragged last workgroup and a long-row scan of 514 chunks over 512 workgroups
    (long rows planted where only the second trip finds them)."""
    t0 = time.time()
    b, blocks = _large()
    ip1 = b["blocks"][1][0]
    late = [r for r in b["dst"][1] if r % 514 >= 512 and ip1[r + 1] - ip1[r] > sg.LONG_ROW]
    tlen = np.diff(b["t1"][0])
    late_t = [u for u in b["src1"] if u % 514 >= 512 and tlen[u] > sg.LONG_ROW]
    assert {r % 514 for r in late} == {512, 513} and {u % 514 for u in late_t} == {512, 513}
    b["t_planted"] = sorted(b["src1"])
    s = run_step(b, blocks, f, h, norm, p)
    check_short(s)
    check_tail_gather(s)
    if norm == "batch":
        assert bn_dy_fuses(s)
        check_bn_dy(s)
    else:
        assert ln_dz_fuses(s)
        check_ln_dz(s)
    print(f"large-n case took {time.time() - t0:.1f} s")


def test_public_spmm_at_large_n():
    """glnn_spmm_csr_f32 at n = 262 800, d = 5 (LPR 4): SAGE mode, and SUM with row and column scales."""
    from glnn_amd import ops
    t0 = time.time()
    n, d = sg.BIG_DST1, 5
    ip, ix, planted = sg.big_graph_for_public_spmm(n)
    rs = np.random.RandomState(11)
    x = rs.standard_normal((n, d)).astype(np.float32)
    row_s, col_s = rs.uniform(0.1, 1, n).astype(np.float32), rs.uniform(0.1, 1, n).astype(np.float32)
    dip, dix, dx = (torch.from_numpy(a).to(DEV) for a in (ip, ix, x))
    deg = np.diff(ip)
    info = lambda r: f"row {r} has {deg[r]} in-edges"
    x64 = x.astype(F64)
    want, cond, d1 = ko.sage_mean(ip, ix, x64, np.abs(x64))
    got = ops.spmm(dip, dix, dx, n, ops.AGG_SAGE_GCN)
    compare("public spmm, SAGE", _host(got), want, ko.bound(d1, cond), rows_info=info)
    a = ko._adj(ip, ix, n, col_s.astype(F64)[ix.astype(np.int64)])
    want, cond = (a @ x64) * row_s[:, None], (a @ np.abs(x64)) * row_s[:, None]
    got = ops.spmm(dip, dix, dx, n, ops.AGG_SUM, row_scale=torch.from_numpy(row_s).to(DEV), col_scale=torch.from_numpy(col_s).to(DEV))
    compare("public spmm, SUM with both scales", _host(got), want, ko.bound(deg[:, None], cond), rows_info=info)
    print(f"public spmm at large n took {time.time() - t0:.1f} s")
