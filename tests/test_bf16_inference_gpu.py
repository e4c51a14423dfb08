"""bf16 activation storage of the whole-graph SAGE teacher forward (csrc/sage_bf16.hip, ops.to_bf16 / spmm / sage_fused on bf16 rows,
SAGE.inference(..., dtype=torch.bfloat16)).  Inputs of the kernel tests are bf16 matrices, so their values are exact in fp64: an fp32
output must agree with the fp64 result within TOL, a bf16 output within one bf16 ulp of that result rounded to bf16 (or within ABS_FLOOR of
it, the fp32 arithmetic's own error, where cancellation leaves a value near zero)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from graphgen import random_graph
from oracle import teacher_oracle as to

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [3, 7, 17, 47, 100, 128, 256]        # 16-byte pieces per row 1, 1, 3, 6, 13, 16, 32: LPR 2, 2, 4, 8, 16, 16, 32 of both dispatchers


def _bits(t):
    """bf16 tensor -> int64 numpy bit patterns (0..65535)."""
    return t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def _ordered(bits):
    """bf16 bit patterns -> integers in value order (+0 and -0 equal): neighbours in value differ by 1."""
    mag = bits & 0x7FFF
    return np.where(bits & 0x8000, -mag, mag)


def _round_bf16(a64):
    return torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).to(torch.bfloat16)


ABS_FLOOR = 2e-5      # fp32 arithmetic error: where cancellation leaves a value near zero its bf16 ulp is finer than the fp32 sum's error


def _assert_within_one_ulp(got_bf16, want64):
    got = _ordered(_bits(got_bf16))
    want = _ordered(_bits(_round_bf16(want64)))
    diff = np.abs(got - want)
    err = np.abs(got_bf16.float().cpu().numpy().astype(np.float64) - want64)
    bad = (diff > 1) & (err > ABS_FLOOR)
    assert not bad.any(), f"{int(bad.sum())} elements more than one bf16 ulp and {ABS_FLOOR} away (max err {err[bad].max()})"


def _graph(n=2003, seed=3):
    # n not a multiple of 32, isolated rows, multi-edges (random multigraph) and one hub row above the long-row threshold
    indptr, indices = random_graph(n, 9, seed=seed, power=0.6, isolated=7, hub=1500)
    return indptr, indices


def _agg64(indptr, indices, x64, n_dst):
    """sum over in-edges in fp64 (prefix sums of the gathered rows; exact enough in fp64 for these sizes)."""
    g = np.concatenate([np.zeros((1, x64.shape[1])), np.cumsum(x64[indices], axis=0)], axis=0) if len(indices) else np.zeros((1, x64.shape[1]))
    return g[indptr[1:n_dst + 1]] - g[indptr[:n_dst]]


def _bf16_input(n, d, seed):
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)).to(DEV)
    from glnn_amd import ops
    xb = ops.to_bf16(x)
    return xb, xb.float().cpu().numpy().astype(np.float64)


# ---- cast ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 47, 100, 256])
def test_cast_matches_torch_bit_for_bit(d):
    from glnn_amd import ops
    n = 301
    rs = np.random.RandomState(d)
    x = (rs.standard_normal((n, d)) * np.exp(rs.uniform(-30, 30, (n, d)))).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, 1e-40, -3e-39, 1.17e-38, 3.4e38, -3.4e38], np.float32)
    flat[:special.size] = special
    # exact ties: bf16 value + half an ulp, with even and odd lower halves
    u = rs.randint(0x3F00, 0x4100, size=64).astype(np.uint32)
    ties = ((u << 16) | 0x8000).view(np.float32)
    flat[special.size:special.size + 64] = ties
    nan_payload = np.array([0x7F800001, 0xFFC12345, 0x7FFFFFFF], np.uint32).view(np.float32)
    flat[special.size + 64:special.size + 67] = nan_payload
    xt = torch.from_numpy(x).to(DEV)
    got = ops.to_bf16(xt)
    want = xt.to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (n, d)
    assert got.stride(0) == ops.round8(d) and got.data_ptr() % 16 == 0
    gb, wb = _bits(got), _bits(want)
    nan = np.isnan(x)
    assert np.array_equal(gb[~nan], wb[~nan])
    assert np.isnan(got.float().cpu().numpy()[nan]).all()                    # NaN stays NaN
    full = got.as_strided((n, ops.round8(d)), (ops.round8(d), 1))
    assert (_bits(full[:, d:]) == 0).all()                                    # padding columns written as 0
    # a wider strided fp32 source
    xw = torch.zeros(n, d + 5, device=DEV)
    xw[:, :d] = torch.nan_to_num(xt)
    assert np.array_equal(_bits(ops.to_bf16(xw[:, :d])), _bits(xw[:, :d].to(torch.bfloat16)))


# ---- aggregation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", ["sage", "sum"])
@pytest.mark.parametrize("epi", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_spmm_bf16_against_fp64(d, mode, epi, out_dtype):
    from glnn_amd import ops
    indptr, indices = _graph()
    n = len(indptr) - 1
    xb, x64 = _bf16_input(n, d, seed=d)
    rs = np.random.RandomState(7)
    deg = np.diff(indptr).astype(np.float64)
    kw = {}
    agg = None
    if mode == "sage":
        agg = (_agg64(indptr, indices, x64, n) + x64[:n]) / (deg + 1)[:, None]
    else:
        rsc = (1.0 / np.sqrt(np.maximum(deg, 1))).astype(np.float32)
        csc = rs.uniform(0.5, 1.5, n).astype(np.float32) if epi else None
        xs = x64 * (csc.astype(np.float64)[:, None] if csc is not None else 1.0)
        agg = _agg64(indptr, indices, xs, n) * rsc.astype(np.float64)[:, None]
        kw["row_scale"] = torch.from_numpy(rsc).to(DEV)
        if csc is not None:
            kw["col_scale"] = torch.from_numpy(csc).to(DEV)
    want = agg
    if epi:
        es = rs.uniform(0.5, 1.5, d).astype(np.float32)
        eh = rs.uniform(-0.3, 0.3, d).astype(np.float32)
        want = np.maximum(agg * es + eh, 0.0)
        kw.update(ep_scale=torch.from_numpy(es).to(DEV), ep_shift=torch.from_numpy(eh).to(DEV), relu=True)
    ip, ix = torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV)
    got = ops.spmm(ip, ix, xb, n, ops.AGG_SAGE_GCN if mode == "sage" else ops.AGG_SUM, out_dtype=out_dtype, **kw)
    assert got.dtype == out_dtype and tuple(got.shape) == (n, d)
    if out_dtype == torch.float32:
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL, rtol=0)
    else:
        _assert_within_one_ulp(got, want)
    again = ops.spmm(ip, ix, xb, n, ops.AGG_SAGE_GCN if mode == "sage" else ops.AGG_SUM, out_dtype=out_dtype, **kw)
    assert torch.equal(got.contiguous().view(torch.int16) if out_dtype == torch.bfloat16 else got,
                       again.contiguous().view(torch.int16) if out_dtype == torch.bfloat16 else again)    # run-to-run bit-reproducible


def test_spmm_bf16_wide_rows_and_row_subset():
    """rows wider than 256 (column tiles in one launch) and an output over the first n_dst < n_src rows."""
    from glnn_amd import ops
    indptr, indices = _graph(n=1500, seed=5)
    n = len(indptr) - 1
    d = 300
    xb, x64 = _bf16_input(n, d, seed=11)
    n_dst = 1000
    ip, ix = torch.from_numpy(indptr[:n_dst + 1].copy()).to(DEV), torch.from_numpy(indices[:indptr[n_dst]].copy()).to(DEV)
    deg = np.diff(indptr[:n_dst + 1]).astype(np.float64)
    want = (_agg64(indptr, indices, x64, n_dst) + x64[:n_dst]) / (deg + 1)[:, None]
    got = ops.spmm(ip, ix, xb, n_dst, ops.AGG_SAGE_GCN, out_dtype=torch.float32)
    np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL, rtol=0)
    _assert_within_one_ulp(ops.spmm(ip, ix, xb, n_dst, ops.AGG_SAGE_GCN, out_dtype=torch.bfloat16), want)


# ---- fused layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_in", WIDTHS)
@pytest.mark.parametrize("out_dtype,out2_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                                  (torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)])
def test_sage_fused_bf16_against_fp64(d_in, out_dtype, out2_dtype):
    from glnn_amd import ops
    indptr, indices = _graph(seed=d_in)
    n = len(indptr) - 1
    xb, x64 = _bf16_input(n, d_in, seed=d_in + 1)
    d_out, d_out2 = 256 if d_in >= 100 else 64, 47
    rs = np.random.RandomState(d_in)
    w = (rs.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    w2 = (rs.standard_normal((d_out2, d_out)) / np.sqrt(d_out)).astype(np.float32)
    es = rs.uniform(0.5, 1.5, d_out).astype(np.float32)
    eh = rs.uniform(-0.3, 0.3, d_out).astype(np.float32)
    deg = np.diff(indptr).astype(np.float64)
    agg = (_agg64(indptr, indices, x64, n) + x64[:n]) / (deg + 1)[:, None]
    hid = np.maximum((agg @ w.astype(np.float64).T) * es + eh, 0.0)
    proj = hid @ w2.astype(np.float64).T
    ip, ix = torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV)
    wt, w2t = torch.from_numpy(w).to(DEV), torch.from_numpy(w2).to(DEV)
    kw = dict(ep_scale=torch.from_numpy(es).to(DEV), ep_shift=torch.from_numpy(eh).to(DEV), relu=True)

    def check(got, want, dt):
        assert got.dtype == dt
        if dt == torch.float32:
            np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL, rtol=0)
        else:
            _assert_within_one_ulp(got, want)

    out = ops.sage_fused(ip, ix, xb, n, wt, out_dtype=out_dtype, **kw)
    check(out, hid, out_dtype)
    out_a, out2 = ops.sage_fused(ip, ix, xb, n, wt, w_next=w2t, out_dtype=out_dtype, out_next_dtype=out2_dtype, **kw)
    check(out_a, hid, out_dtype)
    check(out2, proj, out2_dtype)
    none, out2b = ops.sage_fused(ip, ix, xb, n, wt, w_next=w2t, want_out=False, out_next_dtype=out2_dtype,
                                 tile_order=ops.fused_tile_order(ip, n), **kw)
    assert none is None
    assert torch.equal(out2b.float(), out2.float())                           # same bits without the hidden rows / with a tile order


def test_bf16_ops_validate_their_arguments():
    from glnn_amd import GlnnError, ops
    indptr, indices = _graph(n=200, seed=1)
    ip, ix = torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV)
    xb = ops.bf16_empty(200, 16, DEV, zero=True)
    with pytest.raises(ValueError):
        ops.spmm(ip, ix, torch.zeros(200, 16, device=DEV), 200, ops.AGG_SAGE_GCN, out_dtype=torch.bfloat16)   # fp32 rows -> fp32 out
    with pytest.raises(ValueError):
        ops.spmm(ip, ix, xb, 200, ops.AGG_SAGE_GCN, out=torch.zeros(200, 16, device=DEV), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.spmm(ip, ix, xb, 200, ops.AGG_SAGE_GCN, x_self=torch.zeros(200, 16, device=DEV))
    with pytest.raises(ValueError):
        ops.sage_fused(ip, ix, xb, 200, torch.zeros(8, 15, device=DEV))
    with pytest.raises(ValueError):
        ops.to_bf16(torch.zeros(4, 4, dtype=torch.float64, device=DEV))
    # an unaligned bf16 view is copied into an aligned padded buffer, not rejected
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((200, 21)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    a = ops.spmm(ip, ix, x, 200, ops.AGG_SAGE_GCN, out_dtype=torch.float32)
    b = ops.spmm(ip, ix, ops.to_bf16(x.float()), 200, ops.AGG_SAGE_GCN, out_dtype=torch.float32)
    assert torch.equal(a, b)
    # the C entries refuse what the wrappers would never send
    from glnn_amd import _lib
    h = _lib.lib()
    assert h.glnn_spmm_csr_bf16(None, None, 4, 4, None, 8, 4, 1, None, None, None, 8, None, None, None, 0, None, 8, 0, None) == -1
    assert b"null pointer" in h.glnn_last_error()
    p = ops._p
    rc = h.glnn_spmm_csr_bf16(p(ip), p(ix), 200, 200, p(xb), 12, 16, 1, None, None, p(xb), 16, None, None, None, 0, p(a), 16, 0, None)
    assert rc == -1 and b"ldx" in h.glnn_last_error()
    rc = h.glnn_spmm_csr_bf16(p(ip), p(ix), 200, 200, p(xb), 16, 16, 1, None, None, p(xb), 16, None, None, None, 0, p(a), 16, 7, None)
    assert rc == -1
    assert h.glnn_cast_f32_bf16(p(a), 16, 200, 16, p(xb), 12, None) == -1
    with pytest.raises(GlnnError):
        ops.spmm(ip, ix, xb.cpu(), 200, ops.AGG_SAGE_GCN)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _sage_model(dims, norm, seed):
    from glnn_amd.models import Model
    L = len(dims) - 1
    torch.manual_seed(seed)
    model = Model(dict(model_name="SAGE", num_layers=L, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type=norm, device=DEV))
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for bn in model.encoder.norms:
            h = bn.weight.shape[0]
            bn.weight.copy_(torch.from_numpy(rs.uniform(.5, 1.5, h).astype(np.float32)))
            bn.bias.copy_(torch.from_numpy(rs.uniform(-.2, .2, h).astype(np.float32)))
            bn.running_mean.copy_(torch.from_numpy(rs.uniform(-.3, .3, h).astype(np.float32)))
            bn.running_var.copy_(torch.from_numpy(rs.uniform(.5, 1.5, h).astype(np.float32)))
        for lay in model.encoder.layers:
            lay.fc_neigh.bias.copy_(torch.from_numpy((rs.standard_normal(lay.fc_neigh.bias.shape[0]) * .1).astype(np.float32)))
    model.eval()
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    layers = [dict(weight=sd[f"encoder.layers.{i}.fc_neigh.weight"], bias=sd[f"encoder.layers.{i}.fc_neigh.bias"]) for i in range(L)]
    norms = [dict(weight=sd[f"encoder.norms.{i}.weight"], bias=sd[f"encoder.norms.{i}.bias"],
                  running_mean=sd[f"encoder.norms.{i}.running_mean"], running_var=sd[f"encoder.norms.{i}.running_var"])
             for i in range(L - 1)] if norm == "batch" else None
    return model, layers, norms


def _rb64(a64):
    return _round_bf16(a64).float().numpy().astype(np.float64)


def bf16_storage_oracle(indptr, indices, x, layers, norms, eps=1e-5):
    """fp64 SAGE forward that rounds to bf16 at exactly the storage points of the bf16 sweep (SAGE._whole_graph_layer_bf16): layer 0's
    input when it aggregates first, the chained projection, a project-first layer's x @ W^T, a hidden output the next layer aggregates."""
    n = len(indptr) - 1
    deg = np.diff(indptr).astype(np.float64)
    L = len(layers)
    W = [lay["weight"].astype(np.float64) for lay in layers]
    agg_first = [w.shape[1] <= w.shape[0] for w in W]

    def mean(h):
        return (_agg64(indptr, indices, h, n) + h[:n]) / (deg + 1)[:, None]

    def tail(l, z):
        z = z + layers[l]["bias"].astype(np.float64)
        if l == L - 1:
            return z
        if norms is not None:
            bn = norms[l]
            z = (z - bn["running_mean"]) / np.sqrt(bn["running_var"].astype(np.float64) + eps) * bn["weight"] + bn["bias"]
        return np.maximum(z, 0.0)

    h = x.astype(np.float64)
    if agg_first[0]:
        h = _rb64(h)
    proj = None
    for l in range(L):
        din, dout = W[l].shape[1], W[l].shape[0]
        gathered_next = l + 1 < L and agg_first[l + 1]
        if proj is not None:
            y, proj = tail(l, mean(proj)), None
        elif l + 1 < L and agg_first[l] and din <= 256 and dout <= 256 and not agg_first[l + 1] and W[l + 1].shape[0] <= 256:
            proj = _rb64(tail(l, mean(h) @ W[l].T) @ W[l + 1].T)
            continue
        elif not agg_first[l]:
            y = tail(l, mean(_rb64(h @ W[l].T)))
        else:
            y = tail(l, mean(h) @ W[l].T)
        h = _rb64(y) if gathered_next else y
    return h


E2E = [([100, 256, 256, 47], "batch"), ([128, 256, 256, 40], "batch"), ([20, 32, 6], "none"), ([1433, 128, 7], "none"),
       ([300, 320, 5], "none")]


@pytest.mark.parametrize("dims,norm", E2E)
def test_sage_inference_bf16_end_to_end(dims, norm):
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    n = 4000 if dims[0] <= 300 else 2500
    indptr, indices = random_graph(n, 14, seed=dims[0], power=0.6, isolated=9, hub=1500)
    rs = np.random.RandomState(0)
    x = rs.standard_normal((n, dims[0])).astype(np.float32)
    if dims[0] > 1000:                                  # cora-like: sparse non-negative bag-of-words rows
        x = (rs.uniform(size=(n, dims[0])) < 0.02).astype(np.float32)
    model, layers, norms = _sage_model(dims, norm, seed=1)
    g = CSRGraph(torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV), n)
    loader = FullNeighborLoader(g, 512)
    xt = torch.from_numpy(x).to(DEV)
    got_t = model.inference(loader, xt, dtype=torch.bfloat16)
    assert got_t.dtype == torch.float32 and tuple(got_t.shape) == (n, dims[-1])
    got = got_t.cpu().numpy().astype(np.float64)
    rowmax = np.abs(got).max(1, keepdims=True)

    want_b = bf16_storage_oracle(indptr, indices, x, layers, norms)
    assert (np.abs(got - want_b) <= 2e-3 * np.maximum(np.abs(want_b).max(1, keepdims=True), 1e-6)).all(), \
        float((np.abs(got - want_b) / np.maximum(np.abs(want_b).max(1, keepdims=True), 1e-6)).max())

    want = to.sage_inference(indptr, indices, x, layers, norms).astype(np.float64)
    wmax = np.abs(want).max(1, keepdims=True)
    assert (np.abs(got - want) <= 2e-2 * np.maximum(1.0, wmax)).all(), float((np.abs(got - want) / np.maximum(1.0, wmax)).max())
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 0.05 * wmax[:, 0]
    agree = (got.argmax(1) == want.argmax(1))[clear].mean()
    assert agree >= 0.99, agree
    assert np.isfinite(rowmax).all()

    # already-bf16 features give the same forward
    assert torch.equal(model.inference(loader, xt.to(torch.bfloat16), dtype=torch.bfloat16), got_t)
    # determinism, and the default stays the fp32 forward
    assert torch.equal(model.inference(loader, xt, dtype=torch.bfloat16), got_t)
    assert torch.equal(model.inference(loader, xt, dtype=torch.float32), model.inference(loader, xt))


def test_sage_inference_bf16_refusals():
    from glnn_amd.graph import CSRGraph, FullNeighborLoader
    from glnn_amd.models import Model
    n = 500
    indptr, indices = random_graph(n, 6, seed=2)
    g = CSRGraph(torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV), n)
    loader = FullNeighborLoader(g, 128)
    x = torch.randn(n, 16, device=DEV)
    model, _, _ = _sage_model([16, 32, 4], "batch", seed=3)
    with pytest.raises(NotImplementedError):
        model.encoder.inference(loader, x, whole_graph=False, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        model.inference(loader, x, dtype=torch.float16)
    ln = Model(dict(model_name="SAGE", num_layers=2, feat_dim=16, hidden_dim=32, label_dim=4, dropout_ratio=0.0, norm_type="layer",
                    device=DEV)).eval()
    with pytest.raises(NotImplementedError):
        ln.inference(loader, x, dtype=torch.bfloat16)
    for name in ("GCN", "APPNP", "MLP"):
        m = Model(dict(model_name=name, num_layers=2, feat_dim=16, hidden_dim=32, label_dim=4, dropout_ratio=0.0, norm_type="none",
                       device=DEV)).eval()
        with pytest.raises(NotImplementedError):
            m.inference(g, x, dtype=torch.bfloat16)


def test_sharded_teacher_refuses_bf16():
    from glnn_amd import dist
    with pytest.raises(NotImplementedError):
        dist.ShardedTeacher.forward(object.__new__(dist.ShardedTeacher), torch.zeros(1, device=DEV), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        dist.HaloShardedTeacher.forward(object.__new__(dist.HaloShardedTeacher), torch.zeros(1, device=DEV), dtype=torch.bfloat16)


def test_teacher_cli_bf16_round_trip(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    args = ["--dataset", "synthetic-cora", "--teacher", "SAGE", "--device", "0", "--max_epoch", "3", "--patience", "3",
            "--exp_setting", "tran", "--inference_dtype", "bfloat16"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py")] + args, cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.load(tmp_path / "outputs" / "transductive" / "synthetic-cora" / "SAGE" / "seed_0" / "out.npz")["arr_0"]
    assert out.shape == (2485, 7) and out.dtype == np.float32
    np.testing.assert_allclose(np.exp(out).sum(1), 1.0, atol=1e-4)
