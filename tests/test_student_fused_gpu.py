"""The one-launch form of the bf16 student chain on the GPU (csrc/mlp_fused_bf16.hip: glnn_mlp_forward_fused_bf16, ops.mlp_forward_fused_bf16,
serve.compile_student(fused=True), evaluate_mini_batch(fused=True), --serve_fused).

The fused kernel is held to the per-layer chain BIT FOR BIT ("equal" below: torch.equal on the int32 views of finite outputs) -- the chain
pins k ascending in MFMA steps, no split-K, an fp32 fmaf epilogue and one rounding point per layer, and the fused kernel keeps all of that
-- layer by layer, so that a wrong hidden layer cannot hide behind the layers after it.  One test goes around the chain: the fused
log-probabilities against the fp64 oracle of tests/student_serve_oracle.py under the bound of test_served_student_against_the_oracle."""
import ctypes
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_rules as br
import graphgen
import student_serve_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (dims, norm, cora-like features, must be taken): every chain with widths <= 512 is taken; the last two only where the query says so
CHAINS = [
    ((20, 32, 6), "none", False, True),
    ((100, 47), "none", False, True),
    ((300, 320, 5), "none", False, True),
    ((1433, 128, 7), "none", True, True),
    ((100, 256, 256, 47), "batch", False, True),
    ((128, 512, 512, 40), "batch", False, True),
    ((16, 24, 40, 8, 72, 136, 264, 520, 3), "batch", False, False),      # widths either side of multiples of 8, 16 and 64; 520 > 512
    ((128, 1024, 1024, 40), "batch", False, False),
]


def _equal(a, b):
    return bool(torch.isfinite(a).all()) and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _desc(layers, norms, num_layers=None):
    """The glnn_mlp_serve_desc of a drawn chain (weights packed by ops.pack_weight_bf16, BatchNorm(eval) + bias folded in fp32 as
    serve.ServedStudent folds them) and the tensors it points into."""
    from glnn_amd import _lib, ops
    L = len(layers)
    d = _lib.MlpServeDesc()
    d.num_layers = L if num_layers is None else num_layers
    keep = []
    d.dims[0] = layers[0]["weight"].shape[1]
    for l, lay in enumerate(layers):
        w = ops.pack_weight_bf16(torch.from_numpy(lay["weight"]).to(DEV))
        b = torch.from_numpy(lay["bias"]).to(DEV)
        s = None
        if norms is not None and l != L - 1:
            n = {k: torch.from_numpy(v).to(DEV) for k, v in norms[l].items()}
            s = (n["weight"] / torch.sqrt(n["running_var"] + 1e-5)).contiguous()
            b = ((b - n["running_mean"]) * s + n["bias"]).contiguous()
        keep += [w, b, s]
        d.dims[l + 1] = lay["weight"].shape[0]
        d.w[l], d.ldw[l] = w.data_ptr(), w.stride(0)
        d.ep_scale[l] = s.data_ptr() if s is not None else None
        d.ep_shift[l] = b.data_ptr()
    return d, keep


def _prefix(d, l):
    """The first l layers of the chain d as a chain of their own (its last layer has no ReLU and gives fp32 logits)."""
    from glnn_amd import _lib
    p = _lib.MlpServeDesc()
    ctypes.memmove(ctypes.byref(p), ctypes.byref(d), ctypes.sizeof(p))
    p.num_layers = l
    return p


def _chain(d, x, lsm=False):
    """glnn_mlp_forward_bf16 over x (any leading dimension the entry takes), hidden buffers of its own."""
    from glnn_amd import _lib, ops
    m, L = x.shape[0], d.num_layers
    out = torch.full((m, d.dims[L]), 3.0, dtype=torch.float32, device=DEV)
    ld = ops.round8(max([d.dims[l] for l in range(1, L)] + [8]))
    b0 = torch.empty((m, ld), dtype=torch.bfloat16, device=DEV)
    b1 = torch.empty((m, ld), dtype=torch.bfloat16, device=DEV)
    rc = _lib.lib().glnn_mlp_forward_bf16(ctypes.byref(d), ops._p(x), ops._ld(x), ops._dtype_code(x), m, ops._p(b0), ops._p(b1), ld, ops._p(out),
                                          ops._ld(out), 1 if lsm else 0, ops._stream())
    _lib.check(rc, "glnn_mlp_forward_bf16")
    return out


def _fused(d, x, lsm=False, rows=None):
    from glnn_amd import ops
    m = x.shape[0] if rows is None else rows.numel()
    out = torch.full((m, d.dims[d.num_layers]), 5.0, dtype=torch.float32, device=DEV)
    return ops.mlp_forward_fused_bf16(d, x, out, rows=rows, log_softmax=lsm)


def _forms(x):
    """The three feature forms of one matrix: fp32 rows whose leading dimension is no multiple of 4, fp32 float4 rows, bf16 rows."""
    from glnn_amd import ops
    n, k = x.shape
    odd = k if k % 4 else k + 1
    buf = torch.zeros((n, odd), dtype=torch.float32, device=DEV)
    buf[:, :k] = x
    unaligned = buf[:, :k]
    aligned = ops.feat_empty(n, k, DEV, zero=True)
    aligned.copy_(x)
    assert ops._ld(unaligned) % 4 != 0 and ops._ld(aligned) % 4 == 0
    x16 = ops.as_bf16_feat(x.to(torch.bfloat16))
    assert np.array_equal(br.bits(x16), br.bits(br.round_bf16(x.cpu().numpy())))          # the rounding the fp32 forms get on their way in
    return {"fp32 unaligned": unaligned, "fp32 aligned": aligned, "bf16": x16}


# ------------------------------------------------------------------------------------------------ 1. bit-equal to the chain, layer by layer
@pytest.mark.parametrize("case", range(len(CHAINS)))
def test_fused_equals_the_chain_layer_by_layer(case):
    from glnn_amd import ops
    dims, norm, cora, required = CHAINS[case]
    L = len(dims) - 1
    x_h, layers, norms = so.draw_case(dims, norm, 3 * 64 + 5, seed=100 + case, cora_like=cora)
    d, keep = _desc(layers, norms)
    T, why = ops.mlp_fused_bf16_tile_rows(d)
    if not T:
        assert not required, why
        assert why and "glnn_mlp_fused_bf16_tile_rows" in why
        with pytest.raises(Exception, match="status -2"):
            _fused(d, torch.zeros((4, dims[0]), device=DEV))
        return                                                               # the device does not hold this chain's tile: refused, by name
    assert T % 16 == 0 and T <= 64
    print(f"{dims}: tiles of {T} rows")
    forms = _forms(torch.from_numpy(x_h).to(DEV))
    checked = 0
    for m in (1, T - 1, T, T + 1, 3 * T + 5):
        ref = None
        for name, x in forms.items():
            got = [_fused(_prefix(d, l), x[:m]) for l in range(1, L + 1)] + [_fused(d, x[:m], lsm=True)]
            want = [_chain(_prefix(d, l), x[:m]) for l in range(1, L + 1)] + [_chain(d, x[:m], lsm=True)]
            for l, (g, w) in enumerate(zip(got, want)):
                assert _equal(g, w), (dims, m, name, "log_softmax" if l == L else f"prefix of {l + 1} layers",
                                      float((g - w).abs().max()))
                checked += 1
            # the three forms of the features give the same bits (the fp32 forms round on their way in)
            if ref is None:
                ref = got
            else:
                assert all(_equal(g, r) for g, r in zip(got, ref)), (dims, m, name)
    assert checked == 5 * 3 * (L + 1)


# ------------------------------------------------------------------------------------------------ 2. around the chain: the fp64 oracle
def _mlp(dims, norm, layers, norms):
    """models.Model("MLP") on the GPU carrying the drawn parameters, in eval mode."""
    from glnn_amd.models import Model
    model = Model(dict(model_name="MLP", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.5,
                       norm_type=norm, device=DEV))
    with torch.no_grad():
        for l, lay in enumerate(model.encoder.layers):
            lay.weight.copy_(torch.from_numpy(layers[l]["weight"]))
            lay.bias.copy_(torch.from_numpy(layers[l]["bias"]))
        if norms is not None:
            for l, bn in enumerate(model.encoder.norms):
                for name in ("weight", "bias", "running_mean", "running_var"):
                    getattr(bn, name).copy_(torch.from_numpy(norms[l][name]))
    return model.eval()


@functools.lru_cache(maxsize=None)
def _drawn(dims, norm, n, seed):
    x, layers, norms = so.draw_case(dims, norm, n, seed=seed)
    return x, layers, norms


def _student(dims=(20, 32, 6), norm="none", n=1000, seed=7):
    x, layers, norms = _drawn(dims, norm, n, seed)
    return torch.from_numpy(x).to(DEV), _mlp(dims, norm, layers, norms)


def _log_softmax64(z):
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("dims, norm", [((100, 256, 256, 47), "batch"), ((300, 320, 5), "none")])
def test_fused_student_against_the_oracle(dims, norm):
    """The bound of test_served_student_against_the_oracle -- max(2e-3, 4 x the fp32 stand-in's distance) x the row's largest |logit| --
    on the fused logits and on the fused log-probabilities (against the fp64 log_softmax of the oracle's logits; both normalised by the
    oracle's logits).  Nothing here runs the per-layer chain."""
    from glnn_amd import serve
    x, layers, norms = _drawn(dims, norm, 512, 11)
    want = so.forward(x, layers, norms)
    stand = so.forward(x, layers, norms, accumulate="fp32")
    bound = max(2e-3, 4 * so.rel_err(stand, want))
    s = serve.compile_student(_mlp(dims, norm, layers, norms), fused=True)
    assert s.fused and s.tile_rows > 0
    xt = torch.from_numpy(x).to(DEV)
    logits = s.logits(xt).cpu().numpy().astype(np.float64)
    lp = s.log_probs(xt).cpu().numpy().astype(np.float64)
    assert s._bufs is None                                                   # no hidden buffer was ever allocated
    e_logits = so.rel_err(logits, want)
    e_lp = float((np.abs(lp - _log_softmax64(want)).max(axis=1) / so.row_max(want)).max())
    print(f"{dims} {norm}: fused logits {e_logits:.3g}, log-probabilities {e_lp:.3g}, bound {bound:.3g}")
    assert e_logits <= bound and e_lp <= bound
    assert float(np.abs(np.exp(lp).sum(1) - 1).max()) <= 1e-4


# ------------------------------------------------------------------------------------------------ 3. rows
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_serve_a_subset_without_a_gathered_copy(dtype):
    from glnn_amd import serve
    feats, model = _student()
    feats = feats.to(dtype)
    assert feats.shape[0] == 1000
    s = serve.compile_student(model, fused=True)
    rs = np.random.RandomState(5)
    ids_h = np.concatenate([[999, 0, 17, 17, 0, 999], rs.randint(0, 1000, 194)]).astype(np.int64)
    assert len(ids_h) == 200 and (np.diff(ids_h) < 0).any() and len(set(ids_h.tolist())) < 200
    ids = torch.from_numpy(ids_h).to(DEV)
    for fn in (s.log_probs, s.logits):
        want = fn(feats[ids].contiguous())
        assert _equal(fn(feats, rows=ids), want)
        out = torch.full((200, 6), 9.0, device=DEV)
        assert fn(feats, out=out, rows=ids) is out and _equal(out, want)
    # an id outside the matrix is never an address: its row is what an all-zero input row gives, every other row stays
    want = s.log_probs(feats[ids].contiguous())
    zero = s.log_probs(torch.zeros((1, 20), dtype=dtype, device=DEV))
    bad = ids.clone()
    bad[3], bad[150] = -1, 1000
    got = s.log_probs(feats, rows=bad, check_rows=False)
    assert _equal(got[3:4], zero) and _equal(got[150:151], zero)
    keep = torch.ones(200, dtype=torch.bool, device=DEV)
    keep[3] = keep[150] = False
    assert _equal(got[keep], want[keep])
    for wrong in (-1, 1000):
        one = ids.clone()
        one[7] = wrong
        with pytest.raises(ValueError, match="rows must lie in"):
            s.log_probs(feats, rows=one)
    with pytest.raises(ValueError, match="int64"):
        s.log_probs(feats, rows=ids.to(torch.int32))
    with pytest.raises(ValueError, match="fused=True"):
        serve.compile_student(model).log_probs(feats, rows=ids)              # the per-layer chain reads consecutive rows
    assert tuple(s.log_probs(feats, rows=ids[:0]).shape) == (0, 6)


# ------------------------------------------------------------------------------------------------ 4. row independence, determinism, bounds of the output
def test_rows_are_independent_and_runs_are_deterministic():
    from glnn_amd import _lib, ops
    x_h, layers, norms = _drawn((100, 256, 256, 47), "batch", 512, 11)
    d, keep = _desc(layers, norms)
    T, _ = ops.mlp_fused_bf16_tile_rows(d)
    x = torch.from_numpy(x_h).to(DEV)
    for lsm in (False, True):
        full = _fused(d, x, lsm)
        assert _equal(_fused(d, x, lsm), full)                                # run to run
        for a, b in ((1, 2), (T // 2 + 3, 3 * T + 1), (T + 1, 2 * T), (5, 512)):
            assert _equal(_fused(d, x[a:b], lsm), full[a:b]), (a, b)           # windows that start off a tile boundary
        # a NaN in one input row changes that output row and no other
        xn = x.clone()
        xn[T + 9, 5] = float("nan")
        got = _fused(d, xn, lsm)
        others = torch.ones(512, dtype=torch.bool, device=DEV)
        others[T + 9] = False
        assert _equal(got[others], full[others]) and not torch.equal(got[T + 9], full[T + 9])
    # a wider, longer output buffer keeps its padding columns and the rows behind m
    m, c = 2 * T + 7, 47
    big = torch.full((m + 5, c + 9), 12345.0, device=DEV)
    want = _fused(d, x[:m])
    for lsm in (False, True):
        big.fill_(12345.0)
        ops.mlp_forward_fused_bf16(d, x[:m], big[:m, :c], log_softmax=lsm)
        assert _equal(big[:m, :c], _fused(d, x[:m], lsm))
        assert bool((big[:m, c:] == 12345.0).all()) and bool((big[m:] == 12345.0).all())
    assert _equal(want, _fused(d, x[:m]))
    # m == 0 reads no pointer
    h = _lib.lib()
    assert h.glnn_mlp_forward_fused_bf16(ctypes.byref(d), None, 100, 0, None, 0, 0, None, 47, 0, None) == 0
    assert h.glnn_mlp_forward_fused_bf16(ctypes.byref(d), None, 104, 1, None, 0, 0, None, 47, 1, None) == 0


def test_bf16_rows_ignore_what_sits_behind_their_last_column():
    """Columns [k, ldx) of bf16 rows are not trusted: NaN padding leaves the result unchanged (k = 100: the mask cuts a 16-byte chunk)."""
    from glnn_amd import ops
    x_h, layers, norms = _drawn((100, 256, 256, 47), "batch", 512, 11)
    d, keep = _desc(layers, norms)
    clean = ops.as_bf16_feat(torch.from_numpy(x_h[:150]).to(DEV).to(torch.bfloat16))
    wide = torch.full((150, 136), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, :100] = clean
    assert _equal(_fused(d, wide[:, :100]), _fused(d, clean))


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("width", [2048, 1032])
def test_widths_above_the_cap_are_refused(width):
    from glnn_amd import GlnnError, ops, serve
    dims = (24, width, 5)
    x_h, layers, norms = so.draw_case(dims, "none", 8, seed=width)
    d, keep = _desc(layers, norms)
    T, why = ops.mlp_fused_bf16_tile_rows(d)
    assert T == 0 and str(width) in why and "cap" in why
    out = torch.full((8, 5), 4.0, device=DEV)
    with pytest.raises(GlnnError, match="status -2") as e:
        ops.mlp_forward_fused_bf16(d, torch.from_numpy(x_h).to(DEV), out)
    assert str(width) in str(e.value) and bool((out == 4.0).all())           # nothing was launched
    model = _mlp(dims, "none", layers, norms)
    with pytest.raises(NotImplementedError, match=str(width)):
        serve.compile_student(model, fused=True)
    assert _equal(serve.compile_student(model).logits(torch.from_numpy(x_h).to(DEV)), _chain(d, torch.from_numpy(x_h).to(DEV)))
    # an output layer above the cap as well
    x_h, layers, norms = so.draw_case((24, 32, width), "none", 8, seed=width + 1)
    d, keep = _desc(layers, norms)
    assert ops.mlp_fused_bf16_tile_rows(d)[0] == 0


def test_log_softmax_of_65_classes_is_refused_as_the_chain_refuses_it():
    from glnn_amd import _lib, ops
    x_h, layers, norms = so.draw_case((24, 32, 65), "none", 8, seed=3)
    d, keep = _desc(layers, norms)
    x = torch.from_numpy(x_h).to(DEV)
    assert _equal(_fused(d, x), _chain(d, x))                                 # the logits are fine ...
    h = _lib.lib()
    out = torch.zeros((8, 65), device=DEV)
    b0 = torch.empty((8, 32), dtype=torch.bfloat16, device=DEV)
    rc_chain = h.glnn_mlp_forward_bf16(ctypes.byref(d), ops._p(x), 24, 0, 8, ops._p(b0), None, 32, ops._p(out), 65, 1, ops._stream())
    msg_chain = h.glnn_last_error().decode()
    rc_fused = h.glnn_mlp_forward_fused_bf16(ctypes.byref(d), ops._p(x), 24, 0, None, 0, 8, ops._p(out), 65, 1, ops._stream())
    msg_fused = h.glnn_last_error().decode()
    assert rc_chain == rc_fused == -1
    assert msg_fused == msg_chain.replace("glnn_mlp_forward_bf16", "glnn_mlp_forward_fused_bf16") and "log_softmax" in msg_fused


def test_the_other_mfma_form_is_refused(monkeypatch):
    """GLNN_GEMM_BF16_MFMA16=0 moves the chain to v_mfma_f32_32x32x16_bf16; the fused form's bits are defined against the default form."""
    from glnn_amd import GlnnError, ops
    x_h, layers, norms = so.draw_case((20, 32, 6), "none", 8, seed=3)
    d, keep = _desc(layers, norms)
    x = torch.from_numpy(x_h).to(DEV)
    want = _fused(d, x)
    monkeypatch.setenv("GLNN_GEMM_BF16_MFMA16", "0")
    T, why = ops.mlp_fused_bf16_tile_rows(d)
    assert T == 0 and "GLNN_GEMM_BF16_MFMA16" in why
    with pytest.raises(GlnnError, match="status -2"):
        _fused(d, x)
    monkeypatch.delenv("GLNN_GEMM_BF16_MFMA16")
    assert ops.mlp_fused_bf16_tile_rows(d)[0] > 0 and _equal(_fused(d, x), want)


# ------------------------------------------------------------------------------------------------ 6. wiring
def test_fused_snapshot_follows_parameter_updates():
    """The pattern of test_snapshot_follows_parameter_updates: the cached fused snapshot re-packs itself after a training pass (raw-pointer
    writes, ops.PARAM_EPOCH) and after an in-place torch update; every result is the chain's of a fresh snapshot, bit for bit."""
    from glnn_amd import serve
    from glnn_amd.train_and_eval import evaluate_mini_batch, train_mini_batch
    x_h, layers, norms = _drawn((100, 256, 256, 47), "batch", 512, 11)
    model = _mlp((100, 256, 256, 47), "batch", layers, norms)
    xt = torch.from_numpy(x_h).to(DEV)
    labels = torch.from_numpy(np.random.RandomState(1).randint(0, 47, 512)).to(DEV)
    ev = lambda out, lab: float((out.argmax(1) == lab).float().mean())
    crit = torch.nn.NLLLoss()
    before, l0, s0 = evaluate_mini_batch(model, xt, labels, crit, 128, ev, dtype=torch.bfloat16, fused=True)
    before = before.clone()
    chain0, l1, s1 = evaluate_mini_batch(model, xt, labels, crit, 128, ev, dtype=torch.bfloat16)
    assert _equal(before, chain0) and l0 == l1 and s0 == s1                   # fused=True equals fused=False, loss and score with it
    served = model.__dict__["_served_student_fused"]
    assert served.fused and not model.__dict__["_served_student"].fused and served._bufs is None
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.0)
    train_mini_batch(model, xt, labels, 128, crit, opt)
    after = evaluate_mini_batch(model, xt, labels, crit, 128, ev, dtype=torch.bfloat16, fused=True)[0]
    assert model.__dict__["_served_student_fused"] is served
    assert not torch.equal(after, before)
    assert _equal(after, serve.compile_student(model.eval()).log_probs(xt))
    with torch.no_grad():
        model.encoder.layers[0].weight.mul_(0.5)
    assert _equal(evaluate_mini_batch(model, xt, labels, crit, 128, ev, dtype=torch.bfloat16, fused=True)[0],
                  serve.compile_student(model).log_probs(xt))
    with pytest.raises(ValueError, match="bfloat16"):
        evaluate_mini_batch(model, xt, labels, crit, 128, ev, fused=True)
    model.train()
    with pytest.raises(NotImplementedError):
        served.logits(xt)


def test_row_blocks_do_not_change_a_row(monkeypatch):
    from glnn_amd import serve
    feats, model = _student()
    s = serve.compile_student(model, fused=True)
    want = s.log_probs(feats)
    ids = torch.from_numpy(np.random.RandomState(2).randint(0, 1000, 700)).to(DEV)
    want_ids = s.log_probs(feats, rows=ids)
    monkeypatch.setattr(serve, "EVAL_BLOCK_ROWS", 300)                        # no multiple of the tile
    assert _equal(s.log_probs(feats), want) and _equal(s.log_probs(feats, rows=ids), want_ids)


def _position_case():
    from glnn_amd.graph import CSRGraph
    from glnn_amd.models import Model
    from glnn_amd.position import PositionTable
    n, f, dpos = 300, 33, 36
    indptr, indices = graphgen.random_graph(n, 6.0, 5, isolated=3)
    rs = np.random.RandomState(17)
    unseen = rs.rand(n) < 0.3
    obs = np.nonzero(~unseen)[0]
    g = CSRGraph(torch.from_numpy(np.asarray(indptr, np.int64)), torch.from_numpy(np.asarray(indices, np.int32)), n).to(DEV)
    x = torch.from_numpy(rs.standard_normal((n, f)).astype(np.float32)).to(DEV)
    z = torch.from_numpy(rs.standard_normal((len(obs), dpos)).astype(np.float32)).to(DEV)
    table = PositionTable(z, torch.from_numpy(obs).to(DEV), n)
    torch.manual_seed(3)
    model = Model(dict(model_name="MLP", num_layers=3, feat_dim=f + dpos, hidden_dim=64, label_dim=7, dropout_ratio=0.5, norm_type="batch",
                       device=DEV))
    with torch.no_grad():
        for bn in model.encoder.norms:
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
    ids = torch.from_numpy(np.concatenate([np.arange(n), rs.randint(0, n, 200)]).astype(np.int64)).to(DEV)
    assert table.has_unseen and bool(unseen[ids.cpu().numpy()].any())
    return model.eval(), x, table, g, ids


def test_position_student_fused_equals_the_chain(monkeypatch):
    from glnn_amd import serve
    model, x, table, g, ids = _position_case()
    chain = serve.compile_position_student(model, x, table, g)
    fused = serve.compile_position_student(model, x, table, g, fused=True)
    assert fused.fused and fused.served.fused and not chain.served.fused
    assert _equal(fused.log_probs(ids), chain.log_probs(ids)) and _equal(fused.logits(ids), chain.logits(ids))
    assert fused.served._bufs is None
    monkeypatch.setattr(serve, "POSITION_BLOCK_ROWS", 64)
    assert _equal(fused.log_probs(ids), chain.log_probs(ids))
    with pytest.raises(ValueError, match="bfloat16"):
        serve.compile_position_student(model, x, table, g, dtype=torch.float32, fused=True)


def test_without_the_switch_the_new_entry_is_never_called(monkeypatch):
    """fused=False everywhere: the calls make the launches they made before -- the one-launch entry and its query are not reached, and the
    timed launch names of a position block are the assemble launch alone (the chain goes through glnn_mlp_forward_bf16, untimed as before)."""
    from glnn_amd import ops, serve
    from glnn_amd.train_and_eval import evaluate_mini_batch
    feats, model = _student()
    pmodel, x, table, g, ids = _position_case()

    def boom(*a, **k):
        raise AssertionError("the one-launch entry was called with the switch off")
    monkeypatch.setattr(ops, "mlp_forward_fused_bf16", boom)
    monkeypatch.setattr(ops, "mlp_fused_bf16_tile_rows", boom)
    s = serve.compile_student(model)
    assert s.fused is False and s.tile_rows == 0
    s.log_probs(feats)
    assert s._bufs is not None                                                # the chain's hidden buffers, as before
    labels = torch.zeros(1000, dtype=torch.int64, device=DEV)
    evaluate_mini_batch(model, feats, labels, torch.nn.NLLLoss(), 512, lambda o, y: 0.0, dtype=torch.bfloat16)
    assert "_served_student" in model.__dict__ and "_served_student_fused" not in model.__dict__
    evaluate_mini_batch(model, feats, labels, torch.nn.NLLLoss(), 512, lambda o, y: 0.0)
    timed = []
    ops.set_timing(timed)
    try:
        serve.compile_position_student(pmodel, x, table, g).log_probs(ids)
    finally:
        ops.set_timing(None)
    names = [t[0] for t in timed]
    assert "mlp_forward_fused_bf16" not in names and names.count("position_rows") == 1


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_student_cli_serve_fused_round_trip(tmp_path, monkeypatch):
    """train_student.py --serve_dtype bfloat16 --serve_fused --save_results in a child process: its out.npz is the CHAIN's log-probabilities
    of the saved model over the dataset's features, bit for bit."""
    from glnn_amd import cli, serve
    from glnn_amd.models import Model
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--dataset", "synthetic-cora", "--device", "0", "--max_epoch", "2", "--patience", "2", "--exp_setting", "tran"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py"), "--teacher", "SAGE"] + common, cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    student = ["--teacher", "SAGE", "--student", "MLP", "--serve_dtype", "bfloat16", "--serve_fused", "--save_results"] + common
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_student.py")] + student, cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    sdir = tmp_path / "outputs" / "transductive" / "synthetic-cora" / "SAGE_MLP" / "seed_0"              # the path of a run without the flag
    out = np.load(sdir / "out.npz")["arr_0"]
    assert out.shape == (2485, 7) and out.dtype == np.float32
    monkeypatch.chdir(tmp_path)
    args = cli.get_student_args(student)
    _, feats, _, _, conf = cli._load(args, logging.getLogger("test_student_fused"), args.student)
    assert conf["serve_fused"] is True
    conf["device"] = DEV
    model = Model(conf)
    model.load_state_dict(torch.load(sdir / "model.pth", map_location=DEV))
    want = serve.compile_student(model.eval()).log_probs(feats.to(DEV))
    assert np.isfinite(out).all() and np.array_equal(out.view(np.int32), want.cpu().numpy().view(np.int32))
