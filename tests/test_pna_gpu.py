"""PNA teacher on the GPU: the aggregation kernels (csrc/pna.hip) against numpy at every lane layout, the PNAConv layer, the Model surface,
training steps against the fp64 oracle (tests/pna_oracle.py) fed the library's own masks, a random-walk subgraph epoch and the command lines.

Tolerances (docs/PNA_SEMANTICS.md, Tolerances).  min, max, a + min and a + max are BIT-equal to numpy fp32 (max and min do not round, fp32
addition is monotone and both sides add the same two numbers) and the arguments are equal as integers; mean, sigma, every other forward value,
the losses and the trained parameters take rtol = atol = 1e-4 (tests/parity_rules.TOL).  Parameter gradients and the Adam moments take that or,
where it is more, 4 x the distance of the oracle's own arithmetic run in fp32 from its fp64 run on the same inputs (the rule of
tests/test_gat_gpu.py; the distances are printed).

Gap condition.  The gradient of max / min is discontinuous where two DIFFERENT sources' values are closer than the fp32 rounding of b.  Every
gradient test first asserts that the oracle's min_gap (relative to the layer's max |b|) is at least GAP_MIN, and excludes nothing: every
element is compared.  Measured on the CPU on these inputs (the tests print the figures again): the largest distance between b in fp32 and
in fp64, relative to the layer's max |b|, is 3.63e-7 on the model case (all layers of the three steps) and 0 on the layer cases, whose b is
exact by construction (_grad_case says why); rounded up to 4.0e-7, and GAP_MIN is 32 x that, 1.28e-5.  The model seed was picked on the
CPU so that the oracle alone satisfies it; achieved min_gap: 3.06e-5 on the model case, 6.67e-3 on every layer case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pna_oracle as po
from graphgen import csr_from_edges, random_graph
from parity_rules import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAN = float("nan")
B_DISTANCE_MAX = 4.0e-7            # the measured fp32-against-fp64 distance of b, 3.63e-7, rounded up (module docstring)
GAP_MIN = 32 * B_DISTANCE_MAX      # 1.28e-5
N_SRC = 300
HUB, HUB_EDGES = 17, 3000          # far above the long-row threshold (128 in-edges: the whole workgroup takes the row)
AROUND = {50: 130, 51: 128, 52: 129}          # rows just around it: 128 is the last one-wave row
ISOLATED = (3, 40, 69, 200, 299)
BUSY = 123                         # a source with more than 128 out-edges (the source pass walks 64 entries at a time)
# the smallest F on each pna_agg_*_kernel<LPR> (LPR = 1, 2, 4, 8, 16, 32, 64 lanes a row: up to 4, 8, .., 256 columns), then 100 and 256
# (docs/KERNEL_COVERAGE.md)
WIDTHS = [1, 5, 9, 17, 33, 65, 129, 100, 256]
OUT_WIDTH = {5: 2, 9: 300}         # PNAConv's Fo where it is not F: narrower, and wider than any row the gather takes


@functools.lru_cache(maxsize=None)
def _edges():
    rs = np.random.RandomState(11)
    m = 1500
    src, dst = rs.randint(0, N_SRC, m), rs.randint(0, N_SRC, m)
    keep = ~np.isin(dst, ISOLATED + (HUB,) + tuple(AROUND))
    src, dst = src[keep], dst[keep]
    extra_src, extra_dst = [7, 7, 7, 10], [5, 5, 5, 10]                 # the triple edge 7 -> 5 and the self-loop 10 -> 10
    fan = np.setdiff1d(np.arange(N_SRC), ISOLATED + (HUB,) + tuple(AROUND))[:150]       # source BUSY reaches 150 rows: three chunks of the source pass
    src = np.concatenate([src, extra_src, np.full(len(fan), BUSY), rs.randint(0, N_SRC, HUB_EDGES)] + [rs.randint(0, N_SRC, k) for k in AROUND.values()])
    dst = np.concatenate([dst, extra_dst, fan, np.full(HUB_EDGES, HUB)] + [np.full(k, r) for r, k in AROUND.items()])
    ip, ix = csr_from_edges(src, dst, N_SRC)
    deg = np.diff(ip)
    assert deg[HUB] == HUB_EDGES and all(deg[r] == k for r, k in AROUND.items()) and all(deg[i] == 0 for i in ISOLATED)
    assert len(np.unique(ix[ip[HUB]:ip[HUB + 1]])) < HUB_EDGES            # drawn with repetition
    assert (ix[ip[5]:ip[6]] == 7).sum() == 3 and 10 in ix[ip[10]:ip[11]]
    return ip, ix


def _csr(n_dst):
    ip, ix = _edges()
    return ip[:n_dst + 1], ix[:ip[n_dst]]


def _graph(n_dst):
    from glnn_amd.graph import CSRGraph
    ip, ix = _csr(n_dst)
    return CSRGraph(torch.from_numpy(ip.copy()).to(DEV), torch.from_numpy(ix.copy()).to(DEV), n_dst, N_SRC)


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)          # (a copy: the cached cases are read-only arrays)


def _r4(d):
    return (d + 3) // 4 * 4


def _parts(a, dtype=np.float32, fill=0):
    """[n, P, F] -> the device layout [n, P * round4(F)] (padding = fill)."""
    n, parts, f = a.shape
    out = np.full((n, parts, _r4(f)), fill, dtype)
    out[:, :, :f] = a
    return _t(out.reshape(n, parts * _r4(f)), dtype)


def _unparts(t, parts, f):
    """The device layout back as ([n, P, F], the padding columns)."""
    a = t.cpu().numpy().reshape(t.shape[0], parts, _r4(f))
    return a[:, :, :f], a[:, :, f:]


@functools.lru_cache(maxsize=None)
def _agg_case(f, kind):
    """fp32 inputs of one width and numpy's answers for n_dst = 300, computed once and never modified.  kind "noise": unit noise with a
    common offset of +1000 on the last column; kind "ints": small integers as floats (many exact ties)."""
    rs = np.random.RandomState(1000 + f)
    if kind == "ints":
        b = rs.randint(-3, 4, (N_SRC, f)).astype(np.float32)
    else:
        b = rs.standard_normal((N_SRC, f)).astype(np.float32)
        b[:, f - 1] += np.float32(1000.0)
    a = rs.standard_normal((N_SRC, f)).astype(np.float32)
    ip, ix = _csr(N_SRC)
    s64, mu64, arg = po.agg_fwd(ip, ix, b.astype(np.float64), a.astype(np.float64))
    s32 = po.agg_fwd(ip, ix, b, a, dtype=np.float32)[0]
    for arr in (b, a, s64, mu64, arg, s32):
        arr.setflags(write=False)
    return dict(b=b, a=a, s64=s64, mu64=mu64, arg=arg, s32=s32)


def test_graph_has_the_rows_the_kernels_branch_on():
    ip, ix = _edges()
    deg = np.diff(ip)
    assert len(deg) == 300 and deg.max() == 3000 and {128, 129, 130} <= set(deg.tolist()) and (deg == 0).sum() >= 5
    assert max(AROUND) < 70 and HUB < 70 and sum(i < 70 for i in ISOLATED) == 3          # n_dst = 70 keeps every kind of row
    out_deg = np.bincount(ix, minlength=N_SRC)
    assert out_deg[BUSY] > 128 and np.median(out_deg) > 8                                 # the source pass: three chunks; several rounds of the lane groups
    assert np.bincount(_csr(70)[1], minlength=N_SRC)[BUSY] > 20


# ---------------------------------------------------------------------------------------------------------------- aggregation forward
@pytest.mark.parametrize("n_dst", [300, 70])
@pytest.mark.parametrize("f", WIDTHS)
def test_aggregation_forward(f, n_dst):
    """Same fp32 B on both sides.  min, max and a + . bit-equal; arg equal; mean and sigma within 1e-4, the +1000 column included; padding
    zeros (arguments: -1); the deg-0 rows [0 | 0 | 0 | sqrt(1e-5)] with no a term; without a the parts are the plain statistics."""
    from glnn_amd import ops
    c = _agg_case(f, "noise")
    g = _graph(n_dst)
    tb, ta = ops.as_feat(_t(c["b"])), ops.as_feat(_t(c["a"][:n_dst]))
    out = torch.full((n_dst, 4 * _r4(f)), NAN, dtype=torch.float32, device=DEV)
    s, mu, arg = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), tb, n_dst, a=ta, want_arg=True, out=out)
    assert s is out
    sv, spad = _unparts(s, 4, f)
    av, apad = _unparts(arg, 2, f)
    assert not spad.any() and (apad == -1).all() and np.isfinite(sv).all()
    np.testing.assert_array_equal(sv[:, 1], c["s32"][:n_dst, 1])             # a + min: bit-equal
    np.testing.assert_array_equal(sv[:, 2], c["s32"][:n_dst, 2])             # a + max: bit-equal
    np.testing.assert_array_equal(av, c["arg"][:n_dst])
    err_mu = np.abs(sv[:, 0] - c["s64"][:n_dst, 0]).max()
    err_sg = np.abs(sv[:, 3] - c["s64"][:n_dst, 3]).max()
    err_off = np.abs(sv[:, 3, f - 1] - c["s64"][:n_dst, 3, f - 1]).max()
    print(f"F={f} n_dst={n_dst}: a + mean max|err| {err_mu:.3e}, sigma max|err| {err_sg:.3e}, sigma of the +1000 column max|err| {err_off:.3e}")
    np.testing.assert_allclose(sv[:, 0], c["s64"][:n_dst, 0], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(sv[:, 3], c["s64"][:n_dst, 3], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(mu.cpu().numpy(), c["mu64"][:n_dst], rtol=TOL, atol=TOL)
    iso = [i for i in ISOLATED if i < n_dst]
    assert (sv[iso, :3] == 0).all() and (sv[iso, 3] == np.float32(np.sqrt(np.float32(1e-5)))).all() and (av[iso] == -1).all()
    s0, mu0, arg0 = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), tb, n_dst)        # eval form: no a, no arguments
    assert mu0 is None and arg0 is None
    b_rows = [c["b"][_csr(n_dst)[1][_csr(n_dst)[0][v]:_csr(n_dst)[0][v + 1]]] for v in (HUB, 5, 51)]
    got = _unparts(s0, 4, f)[0]
    for v, rows in zip((HUB, 5, 51), b_rows):
        np.testing.assert_array_equal(got[v, 1], rows.min(0))
        np.testing.assert_array_equal(got[v, 2], rows.max(0))
    np.testing.assert_array_equal(got[:, 3], sv[:, 3])                       # sigma does not see a


@pytest.mark.parametrize("f", WIDTHS)
def test_aggregation_arguments_under_exact_ties(f):
    """B holds small integers: almost every min and max is attained many times, by one source's duplicates and by different sources; the
    argument is still the FIRST CSR position, whatever lane group or wave met it."""
    from glnn_amd import ops
    c = _agg_case(f, "ints")
    g = _graph(N_SRC)
    s, mu, arg = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), ops.as_feat(_t(c["b"])), N_SRC, want_arg=True)
    av = _unparts(arg, 2, f)[0]
    np.testing.assert_array_equal(av, c["arg"])
    ip, ix = _csr(N_SRC)
    assert (av[HUB] < ip[HUB] + 512).all()                                   # seven values over 3000 entries: the first hit comes early
    sv = _unparts(s, 4, f)[0]
    s_plain = po.agg_fwd(ip, ix, c["b"], None, dtype=np.float32)[0]
    np.testing.assert_array_equal(sv[:, 1:3], s_plain[:, 1:3])
    np.testing.assert_allclose(sv[:, [0, 3]], po.agg_fwd(ip, ix, c["b"].astype(np.float64))[0][:, [0, 3]], rtol=TOL, atol=TOL)


@pytest.mark.parametrize("f", [5, 100, 256])
def test_a_chunk_of_rows_equals_the_whole_launch_and_two_runs_agree(f):
    """Rows [10, 60) (the hub, the rows around the threshold, an isolated row) as a launch of their own: bit-equal to the same rows of
    the whole launch, the arguments shifted by the chunk's first CSR position."""
    from glnn_amd import ops
    c = _agg_case(f, "noise")
    g = _graph(N_SRC)
    tb, ta = ops.as_feat(_t(c["b"])), ops.as_feat(_t(c["a"]))
    whole = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), tb, N_SRC, a=ta, want_arg=True)
    again = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), tb, N_SRC, a=ta, want_arg=True)
    assert all(torch.equal(u, v) for u, v in zip(whole, again))
    lo_row, hi_row = 10, 60
    sub = g.row_range(lo_row, hi_row)
    lo = int(_csr(N_SRC)[0][lo_row])
    part = ops.pna_agg_fwd(sub.indptr, sub.indices, sub.num_edges(), tb, hi_row - lo_row, a=ops.as_feat(_t(c["a"][lo_row:hi_row])), want_arg=True)
    assert torch.equal(part[0], whole[0][lo_row:hi_row]) and torch.equal(part[1], whole[1][lo_row:hi_row])
    shifted = torch.where(part[2] >= 0, part[2] + lo, part[2])
    assert torch.equal(shifted, whole[2][lo_row:hi_row])


# ---------------------------------------------------------------------------------------------------------------- aggregation backward
@pytest.mark.parametrize("n_dst", [300, 70])
@pytest.mark.parametrize("f", WIDTHS)
def test_aggregation_backward(f, n_dst):
    """Same dS, B, mu, sigma and arg on both sides (the oracle's, rounded to fp32): within 1e-4; the source rows no edge references (20
    sources past the 300 the edges name) are exact zeros; the padding is zero; two runs are bit-equal."""
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    c = _agg_case(f, "noise")
    ip, ix = _csr(n_dst)
    n_src = N_SRC + 20
    g = CSRGraph(torch.from_numpy(ip.copy()).to(DEV), torch.from_numpy(ix.copy()).to(DEV), n_dst, n_src)
    rs = np.random.RandomState(f)
    ds = rs.standard_normal((n_dst, 4, f)).astype(np.float32)
    b = np.concatenate([c["b"], rs.standard_normal((20, f)).astype(np.float32)])
    mu, sg = c["mu64"][:n_dst].astype(np.float32), c["s64"][:n_dst, 3].astype(np.float32)
    arg = c["arg"][:n_dst]
    ref = po.agg_bwd(ip, ix, ds.astype(np.float64), b.astype(np.float64), mu.astype(np.float64), sg.astype(np.float64), arg)
    out_buf = torch.full((n_src, _r4(f)), NAN, dtype=torch.float32, device=DEV)
    args = (g, _parts(ds), ops.as_feat(_t(b)), ops.as_feat(_t(mu)), ops.as_feat(_t(sg)), _parts(arg, np.int32, -1))
    db = ops.pna_agg_bwd(*args, out=out_buf[:, :f])
    got = db.cpu().numpy()
    print(f"F={f} n_dst={n_dst}: db max|err| {np.abs(got - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=TOL, atol=TOL)
    unref = np.bincount(ix, minlength=n_src) == 0
    assert unref.sum() >= 20 and not got[unref].any() and not out_buf[:, f:].any() and got[~unref].any()
    assert torch.equal(ops.pna_agg_bwd(*args), db)


def test_large_n_launch_geometry():
    """The scan geometry a 300-row graph never reaches (test_gatv2_gpu's planted graph of 262 800 rows): eight rows per wave, a last block
    that ends before its rows do, long rows the scan finds on its second trip, and in the source pass sources of up to 500 out-edges
    (eight chunks of one wave).  F = 6: forward and backward against numpy."""
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    from graphgen import planted_graph, second_trip_plan
    from test_gatv2_gpu import BIG_N, K_LONG_ROW, K_ROWS_PER_WAVE, K_WAVES, _geometry
    n_chunks, n_long_blocks, rows_per_block = _geometry(BIG_N)
    ip, ix = planted_graph(BIG_N, 17, *second_trip_plan(BIG_N, n_chunks, n_long_blocks, K_LONG_ROW))
    n, f = len(ip) - 1, 6
    assert n_chunks > n_long_blocks and rows_per_block == K_ROWS_PER_WAVE * K_WAVES and n % rows_per_block != 0
    long_rows = np.flatnonzero(np.diff(ip) > K_LONG_ROW)
    assert (long_rows % n_chunks >= n_long_blocks).sum() >= 2 and (long_rows % n_chunks < n_long_blocks).sum() >= 2
    rs = np.random.RandomState(3)
    b, a = rs.standard_normal((n, f)).astype(np.float32), rs.standard_normal((n, f)).astype(np.float32)
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)
    tb = ops.as_feat(_t(b))
    s, mu, arg = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), tb, n, a=ops.as_feat(_t(a)), want_arg=True)
    s64, mu64, arg64 = po.agg_fwd(ip, ix, b.astype(np.float64), a.astype(np.float64))
    s32 = po.agg_fwd(ip, ix, b, a, dtype=np.float32)[0]
    sv, av = _unparts(s, 4, f)[0], _unparts(arg, 2, f)[0]
    np.testing.assert_array_equal(sv[:, 1:3], s32[:, 1:3])
    np.testing.assert_array_equal(av, arg64)
    np.testing.assert_allclose(sv[:, [0, 3]], s64[:, [0, 3]], rtol=TOL, atol=TOL)
    ds = rs.standard_normal((n, 4, f)).astype(np.float32)
    mu32, sg32 = mu64.astype(np.float32), s64[:, 3].astype(np.float32)
    ref = po.agg_bwd(ip, ix, ds.astype(np.float64), b.astype(np.float64), mu32.astype(np.float64), sg32.astype(np.float64), arg64)
    db = ops.pna_agg_bwd(g, _parts(ds), tb, ops.as_feat(_t(mu32)), ops.as_feat(_t(sg32)), _parts(arg64, np.int32, -1))
    print(f"n={n}: db max|err| {np.abs(db.cpu().numpy() - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(db.cpu().numpy(), ref, rtol=TOL, atol=TOL)


def test_row_local_pieces_and_empty_inputs():
    """The scalers (forward and backward) and da against numpy at an odd width; n == 0 launches nothing."""
    from glnn_amd import _lib, ops
    ip, ix = _csr(N_SRC)
    g = _graph(N_SRC)
    rs = np.random.RandomState(5)
    fo, delta = 7, 0.9
    z, base, gy = (rs.standard_normal(s).astype(np.float32) for s in ((N_SRC, 3, fo), (N_SRC, fo), (N_SRC, fo)))
    amp, att = po.scalers(ip, delta)
    out_buf = torch.full((N_SRC, _r4(fo)), NAN, dtype=torch.float32, device=DEV)
    out_buf[:, :fo] = _t(base)
    out = ops.pna_scale_fwd(g.indptr, _parts(z), out_buf[:, :fo], delta, relu=True)
    ref = np.maximum(base + z[:, 0] + amp * z[:, 1] + att * z[:, 2], 0)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    assert not out_buf[:, fo:].any()
    dz, dpad = _unparts(ops.pna_scale_bwd(g.indptr, ops.as_feat(_t(gy)), delta), 3, fo)
    np.testing.assert_allclose(dz, np.stack([gy, amp * gy, att * gy], 1), rtol=1e-5, atol=1e-6)
    assert not dpad.any()
    ds = rs.standard_normal((N_SRC, 4, fo)).astype(np.float32)
    da = ops.pna_da(g.indptr, _parts(ds), fo).cpu().numpy()
    np.testing.assert_array_equal(da, ((ds[:, 0] + ds[:, 1]) + ds[:, 2]) * (np.diff(ip) > 0)[:, None])
    h = _lib.lib()
    assert h.glnn_pna_agg_fwd_f32(None, None, 0, 0, 0, None, 8, 8, None, 8, None, 32, None, 8, None, 16, None) == 0
    assert h.glnn_pna_agg_bwd_f32(None, 0, None, None, None, 0, 0, None, 32, None, 8, 8, None, 8, None, 8, None, 16, None, 8, None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the layer
def _layer_case(f, seed):
    """(x, params, gy, delta) of PNAConv(F, Fo) on the 300-node graph, fp32 values."""
    rs = np.random.RandomState(seed * 1000 + f)
    fo = OUT_WIDTH.get(f, f)
    f32 = lambda a: a.astype(np.float32)
    p = {"pre.weight": f32(rs.standard_normal((f, 2 * f)) / np.sqrt(2 * f)), "pre.bias": f32(rs.standard_normal(f) * 0.1),
         "post.weight": f32(rs.standard_normal((fo, 13 * f)) / np.sqrt(13 * f)), "post.bias": f32(rs.standard_normal(fo) * 0.1)}
    return f32(rs.standard_normal((N_SRC, f))), p, f32(rs.standard_normal((N_SRC, fo))), 1.1


def _grad_case(f):
    """The layer case of the gradient check.  With Gaussian inputs no seed meets the gap condition at the wide rows (300 rows x 256 columns x
    {min, max} rivals: about 1.5e5 gaps, each below GAP_MIN with probability ~5e-5; a CPU search over 200 seeds found none at F = 256), so b
    is made well separated instead: column c of x is a permutation of {-150 .. 149} / 64 and W_src a signed permutation matrix times 1/2,
    so b[:, i] = +-x[:, pi(i)] / 2 -- exact in fp32 and fp64 alike (every other term of the product is an exact 0), no two sources equal
    in any column, neighbouring values 1/128 apart.  W_dst, post, the biases and gy stay Gaussian."""
    x, p, gy, delta = _layer_case(f, 1)
    rs = np.random.RandomState(77 + f)
    x = np.stack([(rs.permutation(N_SRC) - 150) / 64.0 for _ in range(f)], 1).astype(np.float32)
    w_src = np.zeros((f, f), np.float32)
    w_src[np.arange(f), rs.permutation(f)] = rs.choice([-0.5, 0.5], f)
    p = dict(p)
    p["pre.weight"] = np.concatenate([p["pre.weight"][:, :f], w_src], 1)
    return x, p, gy, delta


def _layer_gap(x, p, delta):
    """(min_gap, fp32-against-fp64 distance of b, fp64 cache, fp32 cache) of a linear-layer case on the 300-node graph."""
    ip, ix = _csr(N_SRC)
    c64 = po.layer_fwd(ip, ix, x, p, delta, False)[1]
    c32 = po.layer_fwd(ip, ix, x, p, delta, False, dtype=np.float32)[1]
    return po.min_gap([c64]), po.b_distance([c64], [c32]), c64, c32


def _check_grads(tag, got, ref, standin):
    """got / ref / standin: dicts of arrays.  |got - ref| <= max(1e-4 + 1e-4 |ref|, 4 x max |standin - ref|) on every element."""
    worst = []
    for name in ref:
        a, b = np.asarray(got[name], np.float64).reshape(ref[name].shape), ref[name]
        e32 = float(np.abs(np.asarray(standin[name], np.float64).reshape(b.shape) - b).max())
        print(f"{tag} d {name}: max|err| {np.abs(a - b).max():.3e} max|ref| {np.abs(b).max():.3e} fp32 stand-in max|err| {e32:.3e}")
        bad = np.abs(a - b) > np.maximum(TOL + TOL * np.abs(b), 4.0 * e32)
        if bad.any():
            worst.append(f"{name}: {bad.sum()} elements, max|err| {np.abs(a - b).max():.3e}, fp32 stand-in max|err| {e32:.3e}")
    assert not worst, worst


def _layer_module(f, p, delta, relu, feat_drop=0.0):
    from glnn_amd.nn import PNAConv
    fo = p["post.weight"].shape[0]
    lay = PNAConv(f, fo, delta, feat_drop, torch.nn.functional.relu if relu else None).to(DEV)
    lay.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return lay


@pytest.mark.parametrize("f", WIDTHS)
def test_layer_forward_and_gradients_match_the_oracle(f):
    """PNAConv through PnaConvFn on the 300-node graph (hub, threshold rows, isolated rows, the triple edge, the self-loop): the ReLU
    layer's values within 1e-4 on Gaussian inputs; the gradients of the linear layer (no ReLU branch to flip) of every parameter and of x
    by the rule above on _grad_case's inputs, after the gap condition has been asserted."""
    ip, ix = _csr(N_SRC)
    g = _graph(N_SRC)
    x, p, gy, delta = _layer_case(f, 1)
    ref_relu = po.layer_fwd(ip, ix, x, p, delta, True)[0]
    with torch.no_grad():
        y = _layer_module(f, p, delta, True).eval()(g, _t(x))
    print(f"F={f}: out max|err| {np.abs(y.cpu().numpy() - ref_relu).max():.3e} max|ref| {np.abs(ref_relu).max():.3e}")
    np.testing.assert_allclose(y.cpu().numpy(), ref_relu, rtol=TOL, atol=TOL)
    x, p, gy, delta = _grad_case(f)
    gap, dist, c64, c32 = _layer_gap(x, p, delta)
    print(f"F={f}: fp32-against-fp64 distance of b {dist:.3e}, min_gap {gap:.3e} (GAP_MIN {GAP_MIN:.1e})")
    assert dist <= B_DISTANCE_MAX and gap >= GAP_MIN
    lay = _layer_module(f, p, delta, False).train()
    tx = _t(x).requires_grad_(True)
    out = lay(g, tx)
    assert out.requires_grad
    np.testing.assert_allclose(out.detach().cpu().numpy(), po.layer_fwd(ip, ix, x, p, delta, False)[0], rtol=TOL, atol=TOL)
    out.backward(_t(gy))
    dx, grads = po.layer_bwd(c64, gy.astype(np.float64))
    sdx, sgrads = po.layer_bwd(c32, gy)
    got = {k: v.grad.cpu().numpy() for k, v in lay.named_parameters()}
    _check_grads(f"F={f}", dict(got, x=tx.grad.cpu().numpy()), dict(grads, x=dx), dict(sgrads, x=sdx))


def test_layer_dropout_replays_the_counter_based_mask():
    """p > 0: the forward under a fixed seed equals the oracle fed the mask oracle/dropout_mask.py restates (and the library's own mask
    helper writes the same bits); both uses of the input see x'."""
    from glnn_amd import ops
    from glnn_amd.autograd import pna_layer_fwd
    from oracle.dropout_mask import keep_mask
    ip, ix = _csr(N_SRC)
    g = _graph(N_SRC)
    f, p_drop, seed = 33, 0.4, 77
    x, p, _, delta = _layer_case(f, 1)
    mask = keep_mask(N_SRC, f, p_drop, seed)
    np.testing.assert_array_equal(ops.dropout_mask(N_SRC, f, p_drop, seed, DEV).cpu().numpy(), mask)
    ref, c = po.layer_fwd(ip, ix, x, p, delta, True, mask, p_drop)
    w = [_t(p[k]) for k in po.LAYER_KEYS]
    y, saved = pna_layer_fwd(g, ops.as_feat(_t(x)), *w, delta, True, p_drop, seed, keep=True)
    np.testing.assert_allclose(saved[0].cpu().numpy(), c["h"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=TOL, atol=TOL)
    assert 0.3 < 1 - mask.mean() < 0.5 and not np.allclose(ref, po.layer_fwd(ip, ix, x, p, delta, True)[0], atol=1e-2)


# ---------------------------------------------------------------------------------------------------------------- Model surface
LR, WD, STEPS = 0.01, 5e-4, 3
M_N, M_FEAT, M_HIDDEN, M_LABEL, M_L = 60, 8, 8, 4, 2
M_DELTA = 1.3
TORCH_SEED = 4321             # TeacherEngine.base_seed comes from torch.initial_seed()
# numpy seed of _problem, searched on the CPU: the first seed at which the oracle's min_gap >= GAP_MIN and its smallest |pre-activation|
# > 1e-4 in every layer of every one of the three dropout-free steps (the test asserts both first).  Under dropout no seed can do: with
# hidden = 8, ReLU and p = 0.5 about one row of x' in ten is all zeros, so several sources carry b = 0 EXACTLY and min_gap is 0 at every one
# of the 100 seeds tried; the dropout steps are therefore checked through what the gap does not touch -- the first step's loss
PROBLEM_SEED = 3


def _problem(seed):
    """(ip, ix, params, x, labels, idx): a 60-node multigraph with three isolated rows, dims [8, 8, 8, 4]."""
    rs = np.random.RandomState(seed)
    ip, ix = random_graph(M_N, 3, seed=seed, isolated=3)
    params = po.random_params(rs, M_L, M_FEAT, M_HIDDEN, M_LABEL)
    x = rs.standard_normal((M_N, M_FEAT)).astype(np.float32)
    return ip, ix, params, x, rs.randint(0, M_LABEL, M_N).astype(np.int64), np.sort(rs.permutation(M_N)[:24]).astype(np.int64)


def _model(params, p=0.0):
    from glnn_amd.models import PNA, Model
    m = Model(dict(model_name="PNA", num_layers=M_L, feat_dim=M_FEAT, hidden_dim=M_HIDDEN, label_dim=M_LABEL, dropout_ratio=p,
                   norm_type="none", device=DEV, pna_delta=M_DELTA))
    assert type(m.encoder) is PNA and set(m.state_dict()) == set(params) | {"encoder.delta"}
    m.load_state_dict(dict({k: torch.from_numpy(v) for k, v in params.items()}, **{"encoder.delta": torch.tensor(M_DELTA, dtype=torch.float64)}))
    return m


def _setup(seed):
    from glnn_amd.graph import CSRGraph
    ip, ix, params, x, labels, idx = _problem(seed)
    deg = np.diff(ip)
    pairs = np.stack([ix.astype(np.int64), np.repeat(np.arange(M_N), deg)], 1)
    assert (deg == 0).sum() >= 3 and len(np.unique(pairs, axis=0)) < len(pairs)           # isolated rows and a multi-edge
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), M_N)
    return ip, ix, params, x, labels, idx, g, _t(x), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)


def _engine_masks(eng, p, steps):
    """The keep-masks of every dropout site of steps 1..steps as TeacherEngine.step_pna draws them (None for p = 0)."""
    from glnn_amd import ops
    if p == 0:
        return None
    return [[ops.dropout_mask(M_N, M_FEAT if s == 0 else M_HIDDEN, p, eng._pna_seed(s, step=t), DEV).cpu().numpy() for s in range(M_L + 2)]
            for t in range(1, steps + 1)]


def _model_conditions(params, ip, ix, x, labels, idx, masks, p, steps):
    """(min_gap, b distance, smallest |pre-activation|) over every layer of every step of the oracle's own trajectory."""
    r64 = po.train_steps(params, ip, ix, x, labels, idx, M_L, M_DELTA, masks, p, LR, WD, steps)
    r32 = po.train_steps(params, ip, ix, x, labels, idx, M_L, M_DELTA, masks, p, LR, WD, steps, dtype=np.float32)
    gap = min(po.min_gap(c) for c in r64[5])
    dist = max(po.b_distance(a, b) for a, b in zip(r64[5], r32[5]))
    margin, pr = np.inf, params
    for t in range(steps):
        margin = min(margin, po.min_margin(po.model_fwd(pr, ip, ix, x, M_L, M_DELTA, None if masks is None else masks[t], p)[2]))
        pr = po.train_steps(params, ip, ix, x, labels, idx, M_L, M_DELTA, masks, p, LR, WD, t + 1)[1]
    return gap, dist, margin, r64, r32


def test_model_forward_fitnet_and_inference_match_the_oracle():
    ip, ix, params, x, labels, idx, g, tx, _, _ = _setup(PROBLEM_SEED)
    h_ref, ref, cache = po.model_fwd(params, ip, ix, x, M_L, M_DELTA)
    m = _model(params, p=0.5).eval()
    h_list, logits = m.forward_fitnet(g, tx)
    assert len(h_list) == M_L and all(tuple(h.shape) == (M_N, M_HIDDEN) for h in h_list) and not logits.requires_grad
    for a, b in zip(h_list, h_ref):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=TOL, atol=TOL)
    for got in (logits, m(g, tx), m.inference(g, tx)):
        print(f"logits max|err| {np.abs(got.cpu().numpy() - ref).max():.3e}")
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=TOL, atol=TOL)
    mt = _model(params, p=0.0).train()                                       # the training-mode forward, dropout-free: the same values
    lt = mt(g, tx)
    assert lt.requires_grad
    np.testing.assert_allclose(lt.detach().cpu().numpy(), ref, rtol=TOL, atol=TOL)
    with pytest.raises(NotImplementedError, match="not implemented for the PNA teacher"):
        m.inference(g, tx, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="bipartite"):
        m([g], tx)


def test_first_step_under_dropout_matches_the_oracle_fed_the_engines_masks():
    """p = 0.5: the loss of step 1 (a forward quantity: no gap condition) equals the oracle's under the four site masks step_pna draws, the
    step moves every parameter, and the masks of step 2 are others."""
    from glnn_amd import teacher
    from glnn_amd.train_and_eval import train
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(PROBLEM_SEED)
    torch.manual_seed(TORCH_SEED)
    m = _model(params, 0.5)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    eng = teacher.get_engine(m, opt)
    masks = _engine_masks(eng, 0.5, 2)
    ref_loss = po.loss_grads(params, ip, ix, x, labels, idx, M_L, M_DELTA, masks[0], 0.5)[0]
    before = [q.detach().clone() for q in m.parameters()]
    loss = train(m, g, tx, tlabels, torch.nn.NLLLoss(), opt, tidx)
    print(f"p=0.5 step 1: loss {loss:.6f} oracle {ref_loss:.6f}")
    np.testing.assert_allclose(loss, ref_loss, rtol=TOL, atol=TOL)
    assert all(torch.isfinite(q).all() and not torch.equal(q, b) for q, b in zip(m.parameters(), before))
    assert any(not np.array_equal(masks[0][s], masks[1][s]) for s in range(M_L + 2))       # the seed stream moves with the step count


@pytest.mark.parametrize("p", [0.0])
def test_train_steps_match_the_oracle(p):
    """train() (TeacherEngine.step_pna) for three steps against the fp64 oracle's Adam: every loss, the first step's gradients, and after
    the last step the parameters and both Adam moments."""
    from glnn_amd import teacher
    from glnn_amd.train_and_eval import train
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(PROBLEM_SEED)
    torch.manual_seed(TORCH_SEED)
    m = _model(params, p)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    eng = teacher.get_engine(m, opt)
    assert eng.kind == "pna" and eng.base_seed == TORCH_SEED and eng.p == p
    masks = _engine_masks(eng, p, STEPS)
    gap, dist, margin, r64, r32 = _model_conditions(params, ip, ix, x, labels, idx, masks, p, STEPS)
    print(f"p={p}: fp32-against-fp64 distance of b {dist:.3e}, min_gap {gap:.3e} (GAP_MIN {GAP_MIN:.1e}), smallest |pre-activation| {margin:.3e}")
    assert dist <= B_DISTANCE_MAX and gap >= GAP_MIN and margin > TOL
    ref_losses, ref_params, ref_m, ref_v, ref_g1 = r64[:5]
    named = dict(m.named_parameters())
    assert set(named) == set(ref_g1)
    losses = []
    for s in range(STEPS):
        losses.append(train(m, g, tx, tlabels, torch.nn.NLLLoss(), opt, tidx))
        assert teacher.get_engine(m, opt) is eng and eng.step_count == s + 1
        if s == 0:
            _check_grads(f"p={p} step 1", {k: eng.grad(v).cpu().numpy() for k, v in named.items()}, ref_g1, r32[4])
    print(f"p={p} losses {losses} oracle {ref_losses.tolist()}")
    np.testing.assert_allclose(losses, ref_losses, rtol=TOL, atol=TOL)
    for k, v in named.items():
        print(f"p={p} {k} after {STEPS} steps: max|err| {np.abs(v.detach().cpu().numpy() - ref_params[k]).max():.3e}")
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref_params[k], rtol=TOL, atol=TOL, err_msg=k)
    _check_grads(f"p={p} exp_avg", {k: opt.state[v]["exp_avg"].cpu().numpy() for k, v in named.items()}, ref_m, r32[2])
    _check_grads(f"p={p} exp_avg_sq", {k: opt.state[v]["exp_avg_sq"].cpu().numpy() for k, v in named.items()}, ref_v, r32[3])
    assert float(m.encoder.delta) == M_DELTA                                 # the constant is not trained


def test_autograd_gradients_equal_the_engine_step():
    """Model.forward in training mode differentiates through PnaConvFn: dropout-free, its gradients are step_pna's (the same launches)."""
    from glnn_amd import teacher
    from glnn_amd.train_and_eval import train
    ip, ix, params, x, labels, idx, g, tx, tlabels, tidx = _setup(PROBLEM_SEED)
    m = _model(params).train()
    logits = m(g, tx)
    torch.nn.NLLLoss()(logits.log_softmax(dim=1)[tidx], tlabels[tidx]).backward()
    auto = {name: prm.grad.detach().clone() for name, prm in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    train(m, g, tx, tlabels, torch.nn.NLLLoss(), opt, tidx)
    eng = teacher.get_engine(m, opt)
    for name, prm in m.named_parameters():
        np.testing.assert_allclose(eng.grad(prm).cpu().numpy(), auto[name].cpu().numpy(), rtol=TOL, atol=TOL, err_msg=name)
    md = _model(params, p=0.5).train()
    out = md(g, tx)
    torch.nn.NLLLoss()(out.log_softmax(dim=1)[tidx], tlabels[tidx]).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() and bool((q.grad != 0).any()) for q in md.parameters())


def test_train_subgraph_epoch_with_zero_in_degree_rows():
    """One epoch of train_subgraph ("keep": rows of the induced subgraphs may lose every in-edge, which PNA allows) against train() over
    CSRGraph.subgraph of the oracle's node set: the same kernels and step counter on the same arrays -- every parameter is bit-equal."""
    import subgraph_oracle as so
    from glnn_amd import teacher
    from glnn_amd.graph import CSRGraph, RandomWalkSubgraphLoader
    from glnn_amd.train_and_eval import train, train_subgraph
    n, d_in, n_cls = 400, 12, 5
    ip, ix = random_graph(n, 2.0, seed=23, isolated=40)
    g = CSRGraph(_t(ip, np.int64), _t(ix, np.int32), n)
    rs = np.random.RandomState(2)
    x = _t(rs.randn(n, d_in))
    y = torch.from_numpy(rs.randint(0, n_cls, n).astype(np.int64)).to(DEV)
    idx_train = rs.choice(n, 32, replace=False).astype(np.int64)
    train_mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    train_mask[torch.from_numpy(idx_train).to(DEV)] = True
    crit = torch.nn.NLLLoss()

    def model():
        from glnn_amd.models import Model
        torch.manual_seed(0)
        return Model(dict(model_name="PNA", num_layers=2, feat_dim=d_in, hidden_dim=16, label_dim=n_cls, dropout_ratio=0.5,
                          norm_type="none", device=DEV, pna_delta=0.8))

    m1 = model()
    opt1 = torch.optim.Adam(m1.parameters(), lr=0.01, weight_decay=5e-4)
    loader = RandomWalkSubgraphLoader(g, torch.from_numpy(idx_train), 32, 3, shuffle=False, seed=9)
    assert len(loader) == 1
    loss1 = train_subgraph(m1, loader, x, y, crit, opt1)
    assert teacher.get_engine(m1, opt1).step_count == 1 and teacher.get_engine(m1, opt1).kind == "pna"
    m2 = model()
    opt2 = torch.optim.Adam(m2.parameters(), lr=0.01, weight_decay=5e-4)
    walks = so.random_walk(ip, ix, idx_train, 3, loader.rng_seed(1, 0))
    nodes = torch.from_numpy(so.first_appearance(walks.reshape(-1))).to(DEV)
    sub = g.subgraph(nodes)
    assert sub.has_zero_in_degree()
    loss2 = train(m2, sub, x[nodes], y[nodes], crit, opt2, torch.nonzero(train_mask[nodes]).reshape(-1))
    for (k1, p1), (k2, p2) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(p1, p2), k1
    assert np.isfinite(loss1) and loss1 == pytest.approx(loss2, rel=1e-6)
    before = model().state_dict()
    assert any(not torch.equal(before[k], v) for k, v in m1.state_dict().items())          # the step moved the parameters
    assert float(m1.encoder.delta) == 0.8                                    # ... and not delta: it is not recomputed on the subgraph


def test_limits_and_dist_refusals():
    from glnn_amd import dist, ops
    from glnn_amd._lib import GlnnError
    g = _graph(N_SRC)
    wide = torch.zeros(N_SRC, 260, device=DEV)
    with pytest.raises(NotImplementedError, match="PNA rows of at most 256"):
        ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), wide, N_SRC)
    s, mu, arg = ops.pna_agg_fwd(g.indptr, g.indices, g.num_edges(), torch.zeros(N_SRC, 8, device=DEV), N_SRC, want_arg=True)
    with pytest.raises(ValueError, match="ds must be"):
        ops.pna_agg_bwd(g, s[:, :16].contiguous(), torch.zeros(N_SRC, 8, device=DEV), mu, s, arg)
    with pytest.raises(GlnnError):
        ops.pna_agg_fwd(g.indptr.cpu(), g.indices, g.num_edges(), torch.zeros(N_SRC, 8, device=DEV), N_SRC)
    m = _model(_problem(0)[2])
    for cls in (dist.ShardedTeacher, dist.HaloShardedTeacher):
        with pytest.raises(NotImplementedError, match="PNA teacher is not sharded"):
            cls(m.encoder, None, None, None)


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout + r.stderr


def test_pna_teacher_then_student_cli(tmp_path):
    common = ["--dataset", "synthetic-cora", "--teacher", "PNA", "--device", "0", "--max_epoch", "3",
              "--model_config_path", os.path.join(ROOT, "train.conf.yaml")]
    _run("train_teacher.py", common + ["--save_results", "--console_log"], tmp_path)
    base = tmp_path / "outputs" / "transductive" / "synthetic-cora"
    out_t = np.load(base / "PNA" / "seed_0" / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    curves = np.load(base / "PNA" / "seed_0" / "loss_and_score.npz")["arr_0"]
    assert np.isfinite(curves).all()                                           # a finite loss every epoch
    sd = torch.load(base / "PNA" / "seed_0" / "model.pth", map_location="cpu")
    hidden = sd["encoder.fc_in.weight"].shape[0]
    assert tuple(sd["encoder.layers.0.post.weight"].shape) == (hidden, 13 * hidden) and tuple(sd["encoder.fc_out.bias"].shape) == (7,)
    log = (base / "PNA" / "seed_0" / "log").read_text()
    assert "pna_delta:" in log and float(sd["encoder.delta"]) > 0              # computed once from the loaded graph, logged, saved
    _run("train_student.py", common + ["--student", "MLP"], tmp_path)
    out_s = np.load(base / "PNA_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
    np.testing.assert_allclose(np.exp(out_s).sum(1), 1.0, atol=1e-4)
