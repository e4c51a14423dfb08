"""int8 activation storage of the whole-graph SAGE teacher forward (csrc/sage_i8.hip, ops.to_int8_rows / spmm_sage_gcn_i8 / sage_fused_i8,
SAGE.inference(..., dtype=torch.int8); docs/INT8_INFERENCE_SEMANTICS.md).

Kernel tests: the inputs are int8 rows whose scales are powers of two in [2^-6, 2^2], so every element is a multiple of 2^-6 below 2^9 and
the fp64 aggregation of the dequantised rows is the truth.  An fp32 output agrees with it within TOL (tests/bf16_rules.py); an int8 output
(q, s) has s within TOL relative of rowmax|y| / 127 and every element within s / 2 + TOL rowmax|y| + ABS_FLOOR of y.  The fused layer's
weights are scaled by 2^-7: its inputs reach 508 where the bf16 tests' are O(1), and the TOL rule is absolute -- an fp32 product of 256 terms
of that size carries about 1e-4 of rounding alone -- so the weights bring the products back to O(1), exactly (a power of two).

End to end: the logits against tests/int8_oracle.py's storage oracle within the row-relative bound B = 4 x 1.559e-3 = 6.236e-3, where
1.559e-3 is the largest row-relative difference between that oracle in fp64 and the same oracle with float32 arithmetic over the three
cases below (measured on a CPU by `python tests/int8_oracle.py`: 1.559e-3 for [100, 256, 256, 47], where float32 arithmetic moves elements
of a stored matrix to the neighbouring step; 3.3e-7 and 2.3e-7 for the two small cases, where it moved none).  B was fixed before any
kernel ran."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import int8_oracle as io
from bf16_rules import ABS_FLOOR, TOL
from graphgen import csr_from_edges, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# value pieces of 16 bytes per row 1, 1, 1, 3, 7, 16, 16, 16 (lanes per row 2, 2, 2, 4, 8, 16, 16, 16); the scale shares the last value
# piece at 3, 12, 100 and 252 and takes a piece of its own at 13, 47, 253 and 256 (the 17th there)
WIDTHS = [3, 12, 13, 47, 100, 252, 253, 256]
N = 2003
SENSITIVITY = 1.559e-3            # fp32-vs-fp64 storage oracle, row-relative, the largest of the E2E cases (python tests/int8_oracle.py)
B = 4 * SENSITIVITY
W_SCALE = 2.0 ** -7


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows_dev(q, s):
    """(q, s) -> the stored int8 rows on the device."""
    return _dev(io.row_bytes(q, s).view(np.int8))


def _rows_host(t, d):
    """device int8 rows -> (q int8 [n, d], s float32 [n], all bytes uint8 [n, ld])."""
    b = t.cpu().numpy().view(np.uint8)
    return b[:, :d].view(np.int8), b[:, -4:].copy().view("<f4")[:, 0], b


@functools.lru_cache(maxsize=None)
def _graph():
    """n not a multiple of 32, isolated rows, multi-edges, one hub row far above the long-row threshold, and two planted rows of degree
    exactly 128 (the last one-wave row) and 129 (the first workgroup row)."""
    indptr, indices = random_graph(N, 14, seed=3, power=0.6, isolated=9, hub=1500)
    deg = np.diff(indptr)
    rows = [int(r) for r in np.flatnonzero((deg > 0) & (deg < 100))[[5, 700]]]
    dst = np.repeat(np.arange(N), deg)
    keep = ~np.isin(dst, rows)
    rs = np.random.RandomState(11)
    src = np.concatenate([indices[keep], rs.randint(0, N, 128), rs.randint(0, N, 129)])
    dst = np.concatenate([dst[keep], np.full(128, rows[0]), np.full(129, rows[1])])
    indptr, indices = csr_from_edges(src, dst, N)
    deg = np.diff(indptr)
    assert deg[rows[0]] == 128 and deg[rows[1]] == 129 and deg.max() >= 1500 and (deg == 0).sum() >= 9
    return indptr, indices


@functools.lru_cache(maxsize=None)
def _exact_rows(d, seed):
    """Random int8 rows with power-of-two scales: (q, s, the dequantised matrix in fp64)."""
    rs = np.random.RandomState(seed)
    q = rs.randint(-127, 128, size=(N, d)).astype(np.int8)
    s = (2.0 ** rs.randint(-6, 3, size=N)).astype(np.float32)
    return q, s, io.dequant(q, s)


def _agg64(indptr, indices, x64, n_dst):
    g = np.concatenate([np.zeros((1, x64.shape[1])), np.cumsum(x64[indices], axis=0)], axis=0)
    return g[indptr[1:n_dst + 1]] - g[indptr[:n_dst]]


def _mean64(indptr, indices, x64, n_dst):
    deg = np.diff(indptr[:n_dst + 1]).astype(np.float64)
    return (_agg64(indptr, indices, x64, n_dst) + x64[:n_dst]) / (deg + 1)[:, None]


def _check_fp32(got, want, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{what}: max|err| {err.max():.3e}  max|ref| {np.abs(want).max():.3e}")
    assert (err <= TOL).all(), f"{what}: max|err| {err.max():.3e}"


def _check_i8(got, d, want, what):
    q, s, b = _rows_host(got, d)
    ld = io.round16(d + 4)
    assert b.shape == (want.shape[0], ld) and not b[:, d:ld - 4].any()
    rowmax = np.abs(want).max(1)
    s64 = s.astype(np.float64)
    s_err = np.abs(s64 - rowmax / 127)
    s_ok = (s_err <= TOL * rowmax / 127) | ((s64 < ABS_FLOOR) & (rowmax / 127 < ABS_FLOOR))
    err = np.abs(q.astype(np.float64) * s64[:, None] - want)
    bound = (s64 / 2 + TOL * rowmax + ABS_FLOOR)[:, None]
    print(f"{what}: max relative scale error {(s_err / np.maximum(rowmax / 127, 1e-30))[rowmax > 0].max():.3e}  "
          f"max (|q s - y| - s / 2) / rowmax {((err - s64[:, None] / 2) / np.maximum(rowmax, 1e-30)[:, None])[rowmax > 0].max():.3e}")
    assert s_ok.all(), f"{what}: {int((~s_ok).sum())} scales off"
    assert np.abs(q.astype(np.int32)).max() <= 127
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements off, max {err.max():.3e}"


# ---- quantise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_quantise_matches_the_rule_bit_for_bit(d):
    from glnn_amd import ops
    n = 301
    rs = np.random.RandomState(d)
    x = (rs.standard_normal((n, d)) * np.exp(rs.uniform(-8, 8, (n, 1)))).astype(np.float32)
    x[0] = 0                                                             # a zero row
    x[1, d // 2] = np.nan                                                # a NaN row
    x[2, d - 1] = -np.inf                                                # an Inf row
    x[3] = (rs.randint(-126, 126, d) + 0.5).astype(np.float32)           # ties at .5 under s = 1 ...
    x[3, 0] = 127.0
    x[4] = x[3] * np.float32(0.25)                                       # ... and under s = 1/4
    x[5] = -x[3]
    q, s = io.quantise_rows(x)
    want = io.row_bytes(q, s)
    assert s[3] == 1.0 and s[4] == 0.25 and (q[3, 1:] % 2 == 0).all()    # (the oracle sent every tie to the even step)
    got = ops.to_int8_rows(_dev(x))
    assert got.dtype == torch.int8 and tuple(got.shape) == (n, ops.int8_rows_ld(d)) and got.data_ptr() % 16 == 0
    gq, gs, gb = _rows_host(got, d)
    assert np.array_equal(gq, q)                                         # the values
    assert not gb[:, d:-4].any()                                         # the padding
    assert np.array_equal(gs.view(np.uint32), s.view(np.uint32))         # the scale, NaN rows included
    assert np.array_equal(gb, want)
    assert np.isnan(ops.from_int8_rows(got, d)[1:3].cpu().numpy()).all() # the poison is not lost
    assert np.array_equal(ops.from_int8_rows(got, d)[3:].cpu().numpy(), io.dequant(q, s, np.float32)[3:])
    assert np.array_equal(ops.int8_rows_scale(got)[3:].cpu().numpy(), s[3:])
    # a strided, unaligned fp32 source (the scalar-load form), into a poisoned `out`
    xw = torch.zeros(n, d + 5, device=DEV)
    xw[:, 1:d + 1] = _dev(x)
    out = torch.full((n, ops.int8_rows_ld(d)), 0x55, dtype=torch.int8, device=DEV)
    assert ops.to_int8_rows(xw[:, 1:d + 1], out=out) is out
    assert np.array_equal(out.cpu().numpy().view(np.uint8), want)


# ---- aggregation ---------------------------------------------------------------------------------------------------------------
def _epilogue(d, want, rs):
    es = rs.uniform(0.5, 1.5, d).astype(np.float32)
    eh = rs.uniform(-0.3, 0.3, d).astype(np.float32)
    return np.maximum(want * es + eh, 0.0), dict(ep_scale=_dev(es), ep_shift=_dev(eh), relu=True)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("epi", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.int8])
def test_spmm_i8_against_fp64(d, epi, out_dtype):
    from glnn_amd import ops
    indptr, indices = _graph()
    q, s, x64 = _exact_rows(d, d)
    want, kw = _mean64(indptr, indices, x64, N), {}
    if epi:
        want, kw = _epilogue(d, want, np.random.RandomState(7))
    ip, ix, xq = _dev(indptr), _dev(indices), _rows_dev(q, s)
    got = ops.spmm_sage_gcn_i8(ip, ix, xq, d, N, out_dtype=out_dtype, **kw)
    assert got.dtype == out_dtype
    if out_dtype == torch.float32:
        assert tuple(got.shape) == (N, d)
        _check_fp32(got, want, f"spmm_i8 d={d} epi={epi}")
    else:
        _check_i8(got, d, want, f"spmm_i8 -> int8 d={d} epi={epi}")
    again = ops.spmm_sage_gcn_i8(ip, ix, xq, d, N, out_dtype=out_dtype, **kw)
    assert torch.equal(got, again)                                       # run-to-run bit-reproducible


@pytest.mark.parametrize("d", [13, 100, 256])
def test_spmm_i8_row_subset(d):
    """an output over the first n_dst < n_src rows, into a caller's buffer."""
    from glnn_amd import ops
    indptr, indices = _graph()
    q, s, x64 = _exact_rows(d, d + 1)
    n_dst = 1000
    ip, ix = _dev(indptr[:n_dst + 1].copy()), _dev(indices[:indptr[n_dst]].copy())
    want = _mean64(indptr, indices, x64, n_dst)
    xq = _rows_dev(q, s)
    _check_fp32(ops.spmm_sage_gcn_i8(ip, ix, xq, d, n_dst), want, f"spmm_i8 subset d={d}")
    out = ops.int8_rows_empty(n_dst, d, DEV)
    assert ops.spmm_sage_gcn_i8(ip, ix, xq, d, n_dst, x_self=xq[:n_dst], out=out) is out
    _check_i8(out, d, want, f"spmm_i8 subset -> int8 d={d}")


# ---- fused layer ---------------------------------------------------------------------------------------------------------------
def _weight(rs, d_out, d_in):
    return (rs.standard_normal((d_out, d_in)) / np.sqrt(d_in) * W_SCALE).astype(np.float32)


@pytest.mark.parametrize("d_in", WIDTHS)
def test_sage_fused_i8_against_fp64(d_in):
    from glnn_amd import ops
    indptr, indices = _graph()
    q, s, x64 = _exact_rows(d_in, d_in + 2)
    d_out = 256 if d_in >= 100 else 64
    rs = np.random.RandomState(d_in)
    w = _weight(rs, d_out, d_in)
    agg = _mean64(indptr, indices, x64, N)
    ip, ix, xq, wt = _dev(indptr), _dev(indices), _rows_dev(q, s), _dev(w)
    plain = ops.sage_fused_i8(ip, ix, xq, d_in, N, wt)
    assert plain.dtype == torch.float32 and tuple(plain.shape) == (N, d_out)
    _check_fp32(plain, agg @ w.astype(np.float64).T, f"sage_fused_i8 d_in={d_in}")
    hid, kw = _epilogue(d_out, agg @ w.astype(np.float64).T, rs)
    got = ops.sage_fused_i8(ip, ix, xq, d_in, N, wt, tile_order=ops.fused_tile_order(ip, N), **kw)
    _check_fp32(got, hid, f"sage_fused_i8 d_in={d_in} epilogue")
    assert torch.equal(got, ops.sage_fused_i8(ip, ix, xq, d_in, N, wt, **kw))      # two launches (and any tile order): equal bits
    n_dst = 777                                                                    # a row subset with a ragged last tile
    sub = ops.sage_fused_i8(_dev(indptr[:n_dst + 1].copy()), _dev(indices[:indptr[n_dst]].copy()), xq, d_in, n_dst, wt, **kw)
    assert torch.equal(sub, got[:n_dst])


@pytest.mark.parametrize("dims", [(100, 256, 47), (17, 32, 6)])
def test_sage_fused_i8_chained_projection(dims):
    from glnn_amd import ops
    d_in, d_out, d_out2 = dims
    indptr, indices = _graph()
    q, s, x64 = _exact_rows(d_in, d_in + 3)
    rs = np.random.RandomState(d_in)
    w, w2 = _weight(rs, d_out, d_in), (rs.standard_normal((d_out2, d_out)) / np.sqrt(d_out)).astype(np.float32)
    hid, kw = _epilogue(d_out, _mean64(indptr, indices, x64, N) @ w.astype(np.float64).T, rs)
    proj = hid @ w2.astype(np.float64).T
    ip, ix, xq, wt, w2t = _dev(indptr), _dev(indices), _rows_dev(q, s), _dev(w), _dev(w2)
    out, out2 = ops.sage_fused_i8(ip, ix, xq, d_in, N, wt, w_next=w2t, **kw)
    assert out.dtype == torch.float32 and out2.dtype == torch.float32 and tuple(out2.shape) == (N, d_out2)
    _check_fp32(out, hid, f"sage_fused_i8 chain {dims} out")
    _check_fp32(out2, proj, f"sage_fused_i8 chain {dims} out2")
    none, out2b = ops.sage_fused_i8(ip, ix, xq, d_in, N, wt, w_next=w2t, want_out=False, tile_order=ops.fused_tile_order(ip, N), **kw)
    assert none is None and torch.equal(out2b, out2)                               # same bits without the hidden rows / with a tile order


def test_int8_ops_validate_their_arguments():
    from glnn_amd import GlnnError, ops
    indptr, indices = random_graph(200, 6, seed=1)
    ip, ix = _dev(indptr), _dev(indices)
    xq = ops.int8_rows_empty(200, 16, DEV, zero=True)
    with pytest.raises(ValueError):
        ops.spmm_sage_gcn_i8(ip, ix, xq, 12, 200)                                  # 12 columns are 16-byte rows, these are 32
    with pytest.raises(ValueError):
        ops.spmm_sage_gcn_i8(ip, ix, torch.zeros(200, 16, device=DEV), 16, 200)    # fp32 rows
    with pytest.raises(ValueError):
        ops.spmm_sage_gcn_i8(ip, ix, xq, 16, 200, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.spmm_sage_gcn_i8(ip, ix, xq, 16, 200, out=torch.zeros(200, 16, device=DEV), out_dtype=torch.int8)
    with pytest.raises(ValueError):
        ops.sage_fused_i8(ip, ix, xq, 16, 200, torch.zeros(8, 15, device=DEV))
    with pytest.raises(ValueError):
        ops.to_int8_rows(torch.zeros(4, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.to_int8_rows(torch.zeros(4, 300, device=DEV))
    with pytest.raises(GlnnError):
        ops.spmm_sage_gcn_i8(ip, ix, xq.cpu(), 16, 200)
    assert ops.to_int8_rows(torch.zeros(0, 7, device=DEV)).shape == (0, 16)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _sage_model(dims, norm, layers, norms):
    """A SAGE teacher holding exactly the parameters of int8_oracle.e2e_case."""
    from glnn_amd.models import Model
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type=norm, device=DEV))
    with torch.no_grad():
        for lay, p in zip(model.encoder.layers, layers):
            lay.fc_neigh.weight.copy_(_dev(p["weight"]))
            lay.fc_neigh.bias.copy_(_dev(p["bias"]))
        for bn, p in zip(model.encoder.norms, norms or []):
            for k in ("weight", "bias", "running_mean", "running_var"):
                getattr(bn, k).copy_(_dev(p[k]))
    return model.eval()


@pytest.mark.parametrize("dims,norm", io.E2E)
def test_sage_inference_int8_end_to_end(dims, norm):
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    indptr, indices, x, layers, norms = io.e2e_case(dims, norm)
    n = io.E2E_N
    model = _sage_model(dims, norm, layers, norms)
    g = CSRGraph(_dev(indptr), _dev(indices), n)
    loader = FullNeighborLoader(g, 512)
    xt = _dev(x)
    got_t = model.inference(loader, xt, dtype=torch.int8)
    assert got_t.dtype == torch.float32 and tuple(got_t.shape) == (n, dims[-1])
    got = got_t.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()

    want = io.int8_storage_oracle(indptr, indices, x, layers, norms)
    rel = io.row_relative(got, want)
    print(f"int8 e2e {dims}: row-relative error against the storage oracle {rel:.3e} (B = {B:.3e})")
    assert rel <= B, rel
    wmax = np.abs(want).max(1)
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * B * wmax
    print(f"int8 e2e {dims}: {int(clear.sum())} of {n} rows have a clear argmax")
    assert clear.any() and (got.argmax(1) == want.argmax(1))[clear].all()

    # a repeated call, pre-quantised features and bf16 features of the same values
    assert torch.equal(model.inference(loader, xt, dtype=torch.int8), got_t)
    if dims[0] <= dims[1]:                                               # (layer 0 gathers its input: the features may come as int8 rows)
        assert torch.equal(model.inference(loader, ops.to_int8_rows(xt), dtype=torch.int8), got_t)
        with pytest.raises(ValueError, match="int8"):
            model.inference(loader, ops.to_int8_rows(xt)[:, :16], dtype=torch.int8)
    else:
        assert torch.equal(model.inference(loader, xt.to(torch.bfloat16), dtype=torch.int8), got_t)    # (0 / 1 features are exact in bf16)
    # the default stays the fp32 forward, call for call
    assert torch.equal(model.inference(loader, xt, dtype=torch.float32), model.inference(loader, xt))


@pytest.mark.parametrize("dims,norm", [([20, 32, 6], "none"), ([24, 32, 32, 5], "batch")])
def test_int8_fan_out_at_the_largest_degree_is_the_full_forward(dims, norm):
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    n = 900
    indptr, indices = random_graph(n, 8, seed=4, isolated=5)
    assert np.diff(indptr).max() <= 64
    _, _, _, layers, norms = io.e2e_case(dims, norm)
    model = _sage_model(dims, norm, layers, norms)
    loader = FullNeighborLoader(CSRGraph(_dev(indptr), _dev(indices), n), 256)
    xt = _dev(np.random.RandomState(2).standard_normal((n, dims[0])).astype(np.float32))
    full = model.inference(loader, xt, dtype=torch.int8)
    L = len(dims) - 1
    assert torch.equal(model.inference(loader, xt, dtype=torch.int8, fan_out=[64] * L, sample_seed=3), full)
    sampled = model.inference(loader, xt, dtype=torch.int8, fan_out=[2] * L, sample_seed=3)
    assert sampled.shape == full.shape and torch.isfinite(sampled).all() and not torch.equal(sampled, full)
    assert torch.equal(model.encoder.inference_over([loader.graph] * L, xt, dtype=torch.int8), full)


def test_sage_inference_int8_refusals():
    from glnn_amd import dist
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    from glnn_amd.models import Model
    n = 500
    indptr, indices = random_graph(n, 6, seed=2)
    g = CSRGraph(_dev(indptr), _dev(indices), n)
    loader = FullNeighborLoader(g, 128)
    x = torch.randn(n, 16, device=DEV)
    conf = dict(model_name="SAGE", num_layers=2, feat_dim=16, hidden_dim=32, label_dim=4, dropout_ratio=0.0, norm_type="batch", device=DEV)
    model = Model(conf).eval()
    with pytest.raises(NotImplementedError, match="int8"):
        model.encoder.inference(loader, x, whole_graph=False, dtype=torch.int8)
    with pytest.raises(ValueError):
        model.inference(loader, x, dtype=torch.float16)
    with pytest.raises(ValueError):
        model.encoder.inference_over([g, g], x, dtype=torch.float16)
    ln = Model(dict(conf, norm_type="layer")).eval()
    for call in (lambda: ln.inference(loader, x, dtype=torch.int8), lambda: ln.encoder.inference_over([g, g], x, dtype=torch.int8)):
        with pytest.raises(NotImplementedError, match="int8"):
            call()
    mean = Model(dict(conf, sage_aggregator="mean")).eval()
    for call in (lambda: mean.inference(loader, x, dtype=torch.int8), lambda: mean.inference(loader, x, dtype=torch.int8, fan_out=[4, 4]),
                 lambda: mean.encoder.layers[0].forward_i8(g, x, x)):
        with pytest.raises(NotImplementedError, match="int8"):
            call()
    # an aggregate-first layer wider than 256 columns: the message points to bfloat16
    wide = Model(dict(conf, feat_dim=300, hidden_dim=320)).eval()
    with pytest.raises(NotImplementedError, match="int8.*bfloat16"):
        wide.inference(loader, torch.randn(n, 300, device=DEV), dtype=torch.int8)
    for name in ("GCN", "APPNP", "MLP"):
        m = Model(dict(conf, model_name=name, norm_type="none")).eval()
        with pytest.raises(NotImplementedError, match="int8"):
            m.inference(g, x, dtype=torch.int8)
    for cls in (dist.ShardedTeacher, dist.HaloShardedTeacher):
        with pytest.raises(NotImplementedError, match="int8"):
            cls.forward(object.__new__(cls), torch.zeros(1, device=DEV), dtype=torch.int8)


def test_teacher_cli_int8_round_trip(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    args = ["--dataset", "synthetic-cora", "--teacher", "SAGE", "--device", "0", "--max_epoch", "3", "--patience", "3",
            "--exp_setting", "tran", "--inference_dtype", "int8"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py")] + args, cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.load(tmp_path / "outputs" / "transductive" / "synthetic-cora" / "SAGE" / "seed_0" / "out.npz")["arr_0"]
    assert out.shape == (2485, 7) and out.dtype == np.float32
    np.testing.assert_allclose(np.exp(out).sum(1), 1.0, atol=1e-4)
