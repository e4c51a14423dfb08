"""GPU checks of the native SAGE "mean" training step (csrc/sage_mean_step.hip, TeacherEngine.step_sage_mean, train_sage(mean_step="native"))
against the fp64 numpy oracle (tests/sage_mean_oracle.py, with dropout masks tests/sage_mean_step_oracle.py).

Tolerances: rtol = atol = 1e-4 (tests/parity_rules.py) for the loss, the parameters, the Adam moments and the running statistics;
parameter gradients are allowed that or, where it is more, 4x the distance of the fp32 run of the oracle's own arithmetic from its fp64 run
on the same inputs (the bound of test_sage_mean_gpu.test_train_sage_epoch_matches_the_oracle).  A bias in front of a training-mode
BatchNorm is a gauge direction (the loss does not depend on it: true gradient 0, both sides hold rounding noise, and Adam turns that noise
into O(lr) steps), so those biases, their gradients and moments and the running mean that carries them are skipped, as
tests/test_teacher_gpu.py skips them (_is_gauge).  The measured maxima are printed (NOTES.md lists them once a GPU run is recorded)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sage_mean_oracle as mo
import sage_mean_step_oracle as so
from graphgen import csr_from_edges

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
N = 300
LR = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- inputs (built once, never modified) -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edges():
    rs = np.random.RandomState(11)
    src, dst = rs.randint(0, N, 1800), rs.randint(0, N, 1800)
    keep = ~np.isin(dst, (3, 40))                       # two nodes without in-edges
    return csr_from_edges(np.concatenate([src[keep], [7, 7, 10]]), np.concatenate([dst[keep], [5, 5, 10]]), N)


def _graph():
    from glnn_amd.graph import CSRGraph
    ip, ix = _edges()
    return CSRGraph(torch.from_numpy(ip.copy()).to(DEV), torch.from_numpy(ix.copy()).to(DEV), N, N)


@functools.lru_cache(maxsize=None)
def _feats(d):
    f = np.random.RandomState(8).standard_normal((N, d)).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _labels(c):
    y = np.random.RandomState(2).randint(0, c, N).astype(np.int64)
    y.setflags(write=False)
    return y


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _loader(L, n_seeds=128, **flags):
    from glnn_amd.graph import MultiLayerNeighborSampler, NodeDataLoader
    loader = NodeDataLoader(_graph(), torch.arange(n_seeds), MultiLayerNeighborSampler([3] * L), batch_size=64, shuffle=False, seed=5)
    for k, v in flags.items():
        setattr(loader, k, v)
    return loader


def _host(batches):
    return [(inp.cpu().numpy(), outn.cpu().numpy(), [(b.indptr.cpu().numpy(), b.indices.cpu().numpy(), b.num_src_nodes()) for b in blocks])
            for inp, outn, blocks in batches]


@functools.lru_cache(maxsize=None)
def _batches(L, n_seeds=128):
    """(device batches with local ids and input_nodes, the same on the host) of one pass of the sampled loader."""
    dev = list(_loader(L, n_seeds))
    assert len(dev) == (n_seeds + 63) // 64 and all(inp is not None for inp, _, _ in dev)
    return dev, _host(dev)


def _dims(base, L):
    return [base[0]] + [base[1]] * (L - 1) + [base[2]]


def _model(norm, dims, p=0.0, seed=4):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1] if len(dims) > 2 else 8,
                       label_dim=dims[-1], dropout_ratio=p, norm_type=norm, device=DEV, sage_aggregator="mean"))
    with torch.no_grad():
        for nm in model.encoder.norms:
            nm.weight.uniform_(0.5, 1.5)
            nm.bias.uniform_(-0.2, 0.2)
        for lay in model.encoder.layers:
            lay.fc_self.bias.uniform_(-0.2, 0.2)
            lay.fc_neigh.bias.uniform_(-0.2, 0.2)
    return model.train()


def _state(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def _engine(model, wd=0.0):
    from glnn_amd.teacher import TeacherEngine
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=wd)
    return TeacherEngine(model, opt), opt


def _is_gauge(norm, L, k):
    hidden_bias = k.endswith(".bias") and ".layers." in k and not k.startswith(f"encoder.layers.{L - 1}.")
    return norm == "batch" and (hidden_bias or k.endswith("running_mean"))


def _check_grads(model, norm, L, g64, g32, what):
    worst = 0.0
    for k, prm in model.named_parameters():
        if _is_gauge(norm, L, k):
            continue
        got, ref = prm.grad.detach().cpu().numpy().astype(np.float64), g64[k]
        e32 = np.abs(g32[k].astype(np.float64) - ref).max()
        err = np.abs(got - ref)
        worst = max(worst, err.max())
        print(f"{what} {k}: max|err| {err.max():.3e} max|ref| {np.abs(ref).max():.3e} fp32 stand-in max|err| {e32:.3e}")
        tol = np.maximum(TOL + TOL * np.abs(ref), 4.0 * e32)
        assert not (err > tol).any(), f"{what} {k}: max|err| {err.max():.3e}, fp32 stand-in {e32:.3e}"
    print(f"{what}: worst gradient max|err| {worst:.3e}")


def _step(eng, batch, feats, labels):
    inp, outn, blocks = batch
    eng.step_sage_mean(blocks, feats, labels, outn, 1.0, input_nodes=inp)


def _params_equal(a, b):
    for (k, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(p, q), k


def _moments_equal(oa, ob):
    for sa, sb in zip(oa.state.values(), ob.state.values()):
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


# ---- 1. step vs oracle ----------------------------------------------------------------------------------------------------------------
CASES = [(b, L, norm) for b in ((20, 32, 6), (19, 36, 7)) for L in (1, 2, 3) for norm in ("none", "batch", "layer")]


@pytest.mark.parametrize("base,L,norm", CASES)
def test_two_steps_match_the_oracle(base, L, norm):
    """Loss per step, every parameter gradient after step 1 and step 2; parameters, Adam moments and BatchNorm running statistics after
    step 2.  L = 1 has no backward gather (and no norm) and must still work."""
    dims = _dims(base, L)
    dev, host = _batches(L)
    feats, labels = _feats(dims[0]), _labels(dims[-1])
    featsd, labelsd = _t(feats), _t(labels)
    model = _model(norm, dims)
    sd0 = _state(model)
    eng, opt = _engine(model)
    st64, st32 = mo.State(sd0, L, norm), mo.State(sd0, L, norm, dtype=np.float32)
    for i in range(2):
        inp, outn, blocks = host[i]
        want, g64, _ = mo.step(st64, blocks, feats.astype(np.float64)[inp], labels[outn], LR)
        _, g32, _ = mo.step(st32, blocks, feats[inp], labels[outn], LR)
        _step(eng, dev[i], featsd, labelsd)
        loss = eng.loss_out.item()
        print(f"{dims} {norm} step {i + 1}: loss {loss:.6f} oracle {want:.6f} |err| {abs(loss - want):.3e}")
        assert abs(loss - want) < TOL + TOL * abs(want)
        _check_grads(model, norm, L, g64, g32, f"{dims} {norm} step {i + 1}")
    assert eng.step_count == 2
    worst = 0.0
    for k, v in _state(model).items():
        if "num_batches_tracked" in k:
            assert int(v) == 2
        elif not _is_gauge(norm, L, k):
            worst = max(worst, np.abs(v - st64.p[k]).max())
            np.testing.assert_allclose(v, st64.p[k], atol=TOL, rtol=TOL, err_msg=k)
    for (k, prm) in model.named_parameters():
        if _is_gauge(norm, L, k):
            continue
        s = opt.state[prm]
        np.testing.assert_allclose(s["exp_avg"].cpu().numpy(), st64.m[k], atol=TOL, rtol=TOL, err_msg=k + " exp_avg")
        np.testing.assert_allclose(s["exp_avg_sq"].cpu().numpy(), st64.v[k], atol=TOL, rtol=TOL, err_msg=k + " exp_avg_sq")
    print(f"{dims} {norm}: worst parameter max|err| after two steps {worst:.3e}")


# ---- 2. hand-built blocks that reach every kernel branch ----------------------------------------------------------------------------------
HB_DIMS = [19, 37, 7]
HB_N0, HB_N1, HB_N2 = 500, 330, 40          # sources of block 0; its destinations = sources of block 1; seeds


@functools.lru_cache(maxsize=None)
def _hand_blocks():
    """Block 1 (330 sources, 40 destinations): destination 0 has 300 in-edges (all-waves path, 64-edge chunks with a ragged last one; 150 of
    them are the one edge 7 -> 0, so source 7's row of the TRANSPOSED block is long too), destination 1 exactly 128 (the longest one-wave
    row), destination 2 129 (the shortest all-waves row), destination 3 none, destination 4 the edge 5 -> 4 three times, destination 5 the
    self-loop 5 -> 5; source 329 (>= n_dst) is referenced by no edge.  Block 0 (500 sources, 330 destinations): three random in-edges each."""
    rs = np.random.RandomState(21)
    src = [np.full(150, 7), rs.randint(0, 329, 150), rs.randint(0, 329, 128), rs.randint(0, 329, 129), [5, 5, 5], [5]]
    dst = [np.full(300, 0), np.full(128, 1), np.full(129, 2), [4, 4, 4], [5]]
    for v in range(6, HB_N2):
        src.append(rs.randint(0, 329, 4))
        dst.append(np.full(4, v))
    src, dst = np.concatenate(src), np.concatenate(dst)
    b1 = csr_from_edges(src, dst, HB_N2)
    deg = np.diff(b1[0])
    assert list(deg[:6]) == [300, 128, 129, 0, 3, 1] and 329 not in b1[1] and b1[1].max() < HB_N1
    assert (b1[1] == 7).sum() > 128
    b0 = csr_from_edges(rs.randint(0, HB_N0, 3 * HB_N1), np.repeat(np.arange(HB_N1), 3), HB_N1)
    x = rs.standard_normal((HB_N0, HB_DIMS[0])).astype(np.float32)
    y = rs.randint(0, HB_DIMS[2], HB_N2).astype(np.int64)
    return [b0 + (HB_N0,), b1 + (HB_N1,)], x, y


def _hand_dev():
    from glnn_amd.graph import CSRGraph
    blocks, x, y = _hand_blocks()
    dev = [CSRGraph(_t(ip.copy()), _t(np.asarray(ix, np.int32).copy()), len(ip) - 1, ns) for ip, ix, ns in blocks]
    return dev, _t(x), _t(y)


@pytest.mark.parametrize("norm,gather_tail", [("none", "1"), ("batch", "1"), ("layer", "1"), ("batch", "0")])
def test_hand_built_blocks_and_a_nan_filled_arena(norm, gather_tail, monkeypatch):
    monkeypatch.setenv("GLNN_TEACHER_GATHER_TAIL", gather_tail)
    blocks, x, y = _hand_blocks()
    dev, xd, yd = _hand_dev()
    rows = torch.arange(HB_N2, device=DEV)
    inp = torch.arange(HB_N0, device=DEV)

    def run(poison):
        model = _model(norm, HB_DIMS)
        eng, _ = _engine(model)
        if poison is not None:          # the arena the step carves its scratch from, every byte 0xFF (fp32 NaN), big enough to be kept
            eng._arena = torch.full((poison,), 0xFF, dtype=torch.uint8, device=DEV)
        eng.step_sage_mean(dev, xd, yd, rows, 1.0, input_nodes=inp)
        return model, eng

    model, eng = run(None)
    sd0 = _state(_model(norm, HB_DIMS))
    st64, st32 = mo.State(sd0, 2, norm), mo.State(sd0, 2, norm, dtype=np.float32)
    want, g64, _ = mo.step(st64, blocks, x.astype(np.float64), y, LR)
    _, g32, _ = mo.step(st32, blocks, x, y, LR)
    loss = eng.loss_out.item()
    print(f"hand-built {norm} gather_tail={gather_tail}: loss {loss:.6f} oracle {want:.6f}")
    assert abs(loss - want) < TOL + TOL * abs(want)
    _check_grads(model, norm, 2, g64, g32, f"hand-built {norm} gather_tail={gather_tail}")
    # padding columns and unreferenced dh rows are really written: the same bits over an arena that held NaN everywhere
    model_b, eng_b = run(eng._arena.numel())
    assert eng_b._arena.numel() == eng._arena.numel()
    assert np.isfinite(eng_b.loss_out.item()) and eng_b.loss_out.item() == loss
    for (k, p), (_, q) in zip(model.named_parameters(), model_b.named_parameters()):
        assert torch.isfinite(q.grad).all() and torch.equal(p.grad, q.grad), k
    _params_equal(model, model_b)


# ---- 3. dropout 0.5, given the masks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["none", "batch"])
def test_dropout_step_matches_the_oracle_given_the_masks(norm):
    from oracle.dropout_mask import keep_mask
    L, p = 3, 0.5
    dims = _dims((20, 32, 6), L)
    dev, host = _batches(L)
    feats, labels = _feats(dims[0]), _labels(dims[-1])
    model = _model(norm, dims, p)
    sd0 = _state(model)
    eng, _ = _engine(model)
    _step(eng, dev[0], _t(feats), _t(labels))
    inp, outn, blocks = host[0]
    masks = [keep_mask(len(blocks[l][0]) - 1, dims[l + 1], p, eng._seed(l)) for l in range(L - 1)]          # step_count == 1
    assert all(abs(m.mean() - (1 - p)) < 0.1 for m in masks)
    st64, st32 = mo.State(sd0, L, norm), mo.State(sd0, L, norm, dtype=np.float32)
    want, g64, _ = so.step(st64, blocks, feats.astype(np.float64)[inp], labels[outn], LR, masks, p)
    _, g32, _ = so.step(st32, blocks, feats[inp], labels[outn], LR, masks, p)
    loss = eng.loss_out.item()
    print(f"dropout {norm}: loss {loss:.6f} oracle {want:.6f}")
    assert abs(loss - want) < TOL + TOL * abs(want)
    _check_grads(model, norm, L, g64, g32, f"dropout {norm}")


# ---- 4. the three source forms ----------------------------------------------------------------------------------------------------------
def _two_steps(norm, dims, p, batches, monkeypatch=None, env=None, wd=0.0, steps=2):
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    model = _model(norm, dims, p)
    eng, opt = _engine(model, wd)
    featsd, labelsd = _t(_feats(dims[0])), _t(_labels(dims[-1]))
    for i in range(steps):
        _step(eng, batches[i % len(batches)], featsd, labelsd)
    return model, eng, opt


@pytest.mark.parametrize("norm", ["none", "batch", "layer"])
def test_tail_in_gather_equals_materialised_h_bit_for_bit(norm, monkeypatch):
    dims = _dims((19, 36, 7), 3)
    dev, _ = _batches(3)
    a, ea, _ = _two_steps(norm, dims, 0.5, dev, monkeypatch, {"GLNN_TEACHER_GATHER_TAIL": "1"})
    b, eb, _ = _two_steps(norm, dims, 0.5, dev, monkeypatch, {"GLNN_TEACHER_GATHER_TAIL": "0"})
    assert ea.gather_tail and not eb.gather_tail
    assert ea._sage_desc.layer[0].h is None and eb._sage_desc.layer[0].h is not None
    _params_equal(a, b)


@pytest.mark.parametrize("norm", ["batch", "layer"])
def test_hidden_width_260_takes_the_materialised_form(norm):
    """A hidden layer wider than 256 forces the stored-h form (and the 256-column slabs of both aggregation kernels): against the oracle."""
    L, dims = 2, [20, 260, 6]
    dev, host = _batches(L)
    feats, labels = _feats(20), _labels(6)
    model = _model(norm, dims)
    sd0 = _state(model)
    eng, _ = _engine(model)
    _step(eng, dev[0], _t(feats), _t(labels))
    assert eng.gather_tail and eng._sage_desc.layer[0].h is not None
    inp, outn, blocks = host[0]
    st64, st32 = mo.State(sd0, L, norm), mo.State(sd0, L, norm, dtype=np.float32)
    want, g64, _ = mo.step(st64, blocks, feats.astype(np.float64)[inp], labels[outn], LR)
    _, g32, _ = mo.step(st32, blocks, feats[inp], labels[outn], LR)
    loss = eng.loss_out.item()
    assert abs(loss - want) < TOL + TOL * abs(want)
    _check_grads(model, norm, L, g64, g32, f"width 260 {norm}")


@pytest.mark.parametrize("norm", ["none", "batch"])
def test_global_id_outermost_block_equals_local_blocks_bit_for_bit(norm):
    import copy
    dims = _dims((19, 36, 7), 2)
    local = []
    for inp, outn, blocks in _batches(2)[0]:          # really local: without the global ids a loader block carries beside its local ones
        b0 = copy.copy(blocks[0])
        b0.gindices = None
        local.append((inp, outn, [b0, blocks[1]]))
    glob = list(_loader(2, global_first_block=True, plain_transpose=True))
    assert all(inp is None and blocks[0].gindices is not None and blocks[1].t_add_self is False for inp, _, blocks in glob)
    for (_, oa, ba), (_, ob, bb) in zip(local, glob):
        assert torch.equal(oa, ob) and torch.equal(ba[1].indptr, bb[1].indptr) and torch.equal(ba[1].indices, bb[1].indices)
    a, _, _ = _two_steps(norm, dims, 0.5, local)
    b, _, _ = _two_steps(norm, dims, 0.5, glob)
    _params_equal(a, b)


# ---- 5. one call vs two calls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("norm", ["batch", "layer"])
def test_one_call_equals_two_calls_bit_for_bit(norm, p, wd, monkeypatch):
    dims = _dims((20, 32, 6), 3)
    dev, _ = _batches(3)
    a, ea, oa = _two_steps(norm, dims, p, dev, monkeypatch, {"GLNN_TEACHER_ONE_CALL": "1"}, wd)
    b, eb, ob = _two_steps(norm, dims, p, dev, monkeypatch, {"GLNN_TEACHER_ONE_CALL": "0"}, wd)
    assert ea._one_call and not eb._one_call
    _params_equal(a, b)
    _moments_equal(oa, ob)
    assert torch.equal(ea.loss_out, eb.loss_out) and torch.equal(ea.loss_accum, eb.loss_accum)


# ---- 6. run-to-run determinism -----------------------------------------------------------------------------------------------------------
def test_three_steps_are_bit_reproducible():
    dims = _dims((19, 36, 7), 3)
    dev, _ = _batches(3, 192)
    a, _, oa = _two_steps("batch", dims, 0.5, dev, steps=3)
    b, _, ob = _two_steps("batch", dims, 0.5, dev, steps=3)
    _params_equal(a, b)
    _moments_equal(oa, ob)


# ---- 7. surface --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["none", "layer"])
def test_train_sage_native_epoch_matches_the_oracle(norm):
    """test_sage_mean_gpu.test_train_sage_epoch_matches_the_oracle with mean_step="native": the two-batch epoch, that test's tolerances."""
    from glnn_amd import train_and_eval as te
    dims = [20, 32, 6]
    dev, host = _batches(2)
    feats, labels = _feats(20), _labels(6)
    model = _model(norm, dims)
    sd0 = _state(model)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    loss = te.train_sage(model, dev, _t(feats), _t(labels), torch.nn.NLLLoss(), opt, mean_step="native")
    st64, st32 = mo.State(sd0, 2, norm), mo.State(sd0, 2, norm, dtype=np.float32)
    want, per64 = mo.train_sage(st64, host, feats, labels, LR)
    _, per32 = mo.train_sage(st32, host, feats, labels, LR)
    print(f"train_sage native {norm}: loss {loss:.6f} oracle {want:.6f}")
    assert abs(loss - want) < TOL + TOL * abs(want)
    _check_grads(model, norm, 2, per64[-1][1], per32[-1][1], f"train_sage native {norm}")
    for k, v in _state(model).items():
        if "num_batches_tracked" not in k:
            np.testing.assert_allclose(v, st64.p[k], atol=TOL, rtol=0, err_msg=k)
    assert opt.state_dict()["state"][0]["step"] == 2
    assert getattr(model, "_glnn_teacher_engine", None) is not None


@pytest.mark.parametrize("kw", [{}, {"mean_step": "autograd"}])
def test_train_sage_default_stays_on_the_autograd_path(kw):
    from glnn_amd import train_and_eval as te
    dev, _ = _batches(2)
    model = _model("none", [20, 32, 6])
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    loss = te.train_sage(model, dev, _t(_feats(20)), _t(_labels(6)), torch.nn.NLLLoss(), opt, **kw)
    assert np.isfinite(loss) and getattr(model, "_glnn_teacher_engine", None) is None


def test_step_sage_refuses_a_mean_model_and_names_the_mean_step():
    dev, _ = _batches(2)
    model = _model("none", [20, 32, 6])
    eng, _ = _engine(model)
    inp, outn, blocks = dev[0]
    with pytest.raises(NotImplementedError, match="step_sage_mean"):
        eng.step_sage(blocks, _t(_feats(20)), _t(_labels(6)), outn, 1.0, input_nodes=inp)
    assert eng.step_count == 0


@pytest.mark.parametrize("norm", ["batch", "layer"])
def test_mean_descriptor_rebuilds_when_captured_state_changes(norm):
    """tests/test_sage_ln_gpu.py::test_descriptor_rebuild_after_load_state_dict_a_changed_eps_and_a_replaced_layernorm for step_sage_mean, on
    the hand-built blocks: load_state_dict keeps the tensors (same descriptors, new values); a changed dropout and, for LayerNorm, a changed
    eps are part of the descriptors' signature (both rebuilt).  Each time the next step's loss and gradients are the oracle's for the state
    the model then holds (the bounds of test_dropout_step_matches_the_oracle_given_the_masks)."""
    from oracle.dropout_mask import keep_mask
    blocks, x, y = _hand_blocks()
    dev, xd, yd = _hand_dev()
    rows, inp = torch.arange(HB_N2, device=DEV), torch.arange(HB_N0, device=DEV)
    model = _model(norm, HB_DIMS)
    eng, _ = _engine(model)

    def check(what, p, eps):
        sd = _state(model)
        eng.step_sage_mean(dev, xd, yd, rows, 1.0, input_nodes=inp)
        masks = [keep_mask(HB_N1, HB_DIMS[1], p, eng._seed(0))] if p > 0 else None      # (the step's own seed: step_count stays put)
        st64, st32 = mo.State(sd, 2, norm, eps=eps), mo.State(sd, 2, norm, eps=eps, dtype=np.float32)
        want, g64, _ = so.step(st64, blocks, x.astype(np.float64), y, LR, masks, p)
        _, g32, _ = so.step(st32, blocks, x, y, LR, masks, p)
        loss = eng.loss_out.item()
        print(f"rebuild {norm} {what}: loss {loss:.6f} oracle {want:.6f}")
        assert abs(loss - want) < TOL + TOL * abs(want)
        _check_grads(model, norm, 2, g64, g32, f"rebuild {norm} {what}")

    check("first step", 0.0, 1e-5)
    d, md = eng._sage_desc, eng._sage_mean
    assert d is not None and md is not None
    model.load_state_dict(_model(norm, HB_DIMS, seed=9).state_dict())
    check("after load_state_dict", 0.0, 1e-5)
    assert eng._sage_desc is d and eng._sage_mean is md
    model.encoder.dropout.p = 0.5
    check("after dropout 0.5", 0.5, 1e-5)
    assert eng._sage_desc is not d and eng._sage_mean is not md and eng.p == 0.5
    if norm == "layer":
        d, md = eng._sage_desc, eng._sage_mean
        for nm in model.encoder.norms:
            nm.eps = 1e-3
        check("after eps 1e-3", 0.5, 1e-3)
        assert eng._sage_desc is not d and eng._sage_mean is not md
    assert eng.step_count == (4 if norm == "layer" else 3)


@pytest.mark.parametrize("entry", ["step_sage", "step_sage_mean"])
def test_failed_step_leaves_the_counter_and_seeds_where_they_were(entry):
    """A refused step never happened: step_count -- Adam's bias correction and the dropout seeds -- stays, and the next good step gives the
    bits of the same step on a fresh engine seeded alike (dropout 0.5, so the seeds matter).  Two refusals, both argument checks in front
    of every launch of the step: block 1 with one source more than block 0 has destinations (ValueError, raised in Python), and block 0
    with fewer sources than destinations, which reaches the C entry and is refused by its first loop of checks (GlnnError: the rc != 0
    rollback).  A descriptor with dropout_p = 1 is NOT used: csrc/sage_step.hip does not check dropout_p before its first launch."""
    from glnn_amd._lib import GlnnError
    from glnn_amd.graph import CSRGraph
    from glnn_amd.models import Model
    dev, xd, yd = _hand_dev()
    rows, inp = torch.arange(HB_N2, device=DEV), torch.arange(HB_N0, device=DEV)

    def fresh():
        torch.manual_seed(4)
        model = Model(dict(model_name="SAGE", num_layers=2, feat_dim=HB_DIMS[0], hidden_dim=HB_DIMS[1], label_dim=HB_DIMS[2], dropout_ratio=0.5,
                           norm_type="batch", device=DEV, sage_aggregator="mean" if entry == "step_sage_mean" else "gcn")).train()
        return model, _engine(model)[0]

    def step(eng, blocks):
        getattr(eng, entry)(blocks, xd, yd, rows, 1.0, input_nodes=inp)

    model, eng = fresh()
    step(eng, dev)
    assert eng.step_count == 1
    wide = CSRGraph(dev[1].indptr, dev[1].indices, HB_N2, HB_N1 + 1)
    with pytest.raises(ValueError, match=f"TeacherEngine.{entry}: block 1 has {HB_N1 + 1} sources"):
        step(eng, [dev[0], wide])
    assert eng.step_count == 1
    short = CSRGraph(dev[0].indptr, dev[0].indices, HB_N1, HB_N1 - 1)
    with pytest.raises(GlnnError, match="n_src=329|bad block sizes"):
        step(eng, [short, dev[1]])
    assert eng.step_count == 1
    step(eng, dev)
    assert eng.step_count == 2
    model_b, eng_b = fresh()
    step(eng_b, dev)
    step(eng_b, dev)
    _params_equal(model, model_b)


def test_loader_transposes_with_self_entries_are_not_read():
    """An engine-mode loader in its default ("gcn") form tags its inner transposes add_self=True: step_sage_mean builds its own."""
    dims = [20, 32, 6]
    glob = list(_loader(2, global_first_block=True))[0]
    local = list(_loader(2))[0]
    assert glob[2][1].t_add_self is True and glob[2][1].t_indptr is not None and glob[0] is None
    assert torch.equal(glob[2][1].indices, local[2][1].indices)
    inp, outn, blocks = _host([local])[0]
    feats, labels = _feats(20), _labels(6)
    model = _model("batch", dims)
    sd0 = _state(model)
    eng, _ = _engine(model)
    eng.step_sage_mean(glob[2], _t(feats), _t(labels), glob[1], 1.0)
    assert eng._sage_desc.layer[1].tr_ws is not None
    st64, st32 = mo.State(sd0, 2, "batch"), mo.State(sd0, 2, "batch", dtype=np.float32)
    want, g64, _ = mo.step(st64, blocks, feats.astype(np.float64)[inp], labels[outn], LR)
    _, g32, _ = mo.step(st32, blocks, feats[inp], labels[outn], LR)
    assert abs(eng.loss_out.item() - want) < TOL + TOL * abs(want)
    _check_grads(model, "batch", 2, g64, g32, "add_self transposes")


def test_teacher_cli_native_mean_step(tmp_path):
    args = ["--dataset", "synthetic-cora", "--teacher", "SAGE", "--sage_aggregator", "mean", "--sage_mean_step", "native", "--device", "0",
            "--max_epoch", "3", "--exp_setting", "tran", "--save_results"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py")] + args, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.load(tmp_path / "outputs" / "transductive" / "synthetic-cora" / "SAGE" / "seed_0" / "out.npz")["arr_0"]
    assert out.shape == (2485, 7) and np.isfinite(out).all()
    np.testing.assert_allclose(np.exp(out).sum(1), 1.0, atol=1e-4)


def test_inference_accepts_the_cli_evaluation_loader():
    """The teacher CLI evaluates through a NodeDataLoader that sweeps every node in id order with the one-layer full sampler: it carries the
    resident graph, and the whole-graph "mean" inference over it is the FullNeighborLoader's, bit for bit."""
    from glnn_amd.graph import FullNeighborLoader, MultiLayerFullNeighborSampler, NodeDataLoader
    g = _graph()
    model = _model("batch", [20, 32, 32, 6]).eval()
    feats = _t(_feats(20))
    cli = NodeDataLoader(g, torch.arange(N), MultiLayerFullNeighborSampler(1), batch_size=64, shuffle=False, drop_last=False)
    assert getattr(cli, "graph", None) is g
    assert torch.equal(model.inference(cli, feats), model.inference(FullNeighborLoader(g, 64), feats))
    with pytest.raises(NotImplementedError, match="mean"):          # the chunked sweep still needs the loader's global-id blocks
        model.encoder.inference(cli, feats, whole_graph=False)
