"""GPU checks of the SAGE teacher with LayerNorm tails (norm_type "layer"): TeacherEngine.step_sage on glnn_sage_fwd_bwd_ln_f32 /
glnn_sage_train_step_ln_f32 against the reference's own train_sage (tests/golden/sage_ln_teacher.npz), the fp64 oracle
(tests/sage_ln_oracle.py), the autograd path, and itself across its equal-result forms."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sage_ln_oracle as so
from graphgen import random_graph

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(indptr, indices, n_src=None):
    from glnn_amd.graph import CSRGraph
    n = len(indptr) - 1
    return CSRGraph(torch.from_numpy(np.asarray(indptr, np.int64)).to(DEV), torch.from_numpy(np.asarray(indices, np.int32)).to(DEV), n,
                    n if n_src is None else n_src)


def _model(dims, p=0.0, sd=None, lr=0.01, wd=0.0, seed=3):
    from glnn_amd.models import Model
    torch.manual_seed(seed)
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=p,
                       norm_type="layer", device=DEV))
    if sd is not None:
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    else:
        with torch.no_grad():
            for nm in model.encoder.norms:
                nm.weight.uniform_(0.5, 1.5)
                nm.bias.uniform_(-0.2, 0.2)
    model.train()
    return model, torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)


def _golden_on_device():
    z, batches = so.load_golden()
    feats, labels = torch.from_numpy(z["feats"]).to(DEV), torch.from_numpy(z["labels"]).to(DEV)
    dev = [(torch.from_numpy(i).to(DEV), torch.from_numpy(o).to(DEV), [_graph(ip, ix, ns) for ip, ix, ns in blks]) for i, o, blks in batches]
    return z, batches, feats, labels, dev


def _state(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def test_train_sage_layernorm_matches_the_reference_golden():
    """train_sage (TeacherEngine) on a LayerNorm SAGE model over the fixture's blocks vs the reference's own train_sage: per-epoch
    losses, parameters and Adam moments after two epochs, and the eval forward afterwards."""
    from glnn_amd import train_and_eval as te
    z, batches, feats, labels, dev = _golden_on_device()
    dims = [int(d) for d in z["dims"]]
    model, opt = _model(dims, sd=so.sub(z, "init."), lr=float(z["lr"]), wd=float(z["wd"]))
    crit = torch.nn.NLLLoss()
    means = [te.train_sage(model, dev, feats, labels, crit, opt) for _ in range(2)]
    np.testing.assert_allclose(means, z["epoch_losses"], atol=TOL, rtol=0)
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), z[f"final.{k}"], atol=TOL, rtol=0, err_msg=k)
    for k, prm in model.named_parameters():
        s = opt.state[prm]
        assert int(s["step"]) == int(z["adam_step"])
        np.testing.assert_allclose(s["exp_avg"].cpu().numpy(), z[f"exp_avg.{k}"], atol=TOL, rtol=0, err_msg=k)
        np.testing.assert_allclose(s["exp_avg_sq"].cpu().numpy(), z[f"exp_avg_sq.{k}"], atol=1e-6, rtol=1e-3, err_msg=k)
    model.eval()
    inp, _, blks = dev[0]
    with torch.no_grad():
        out = model(blks, feats[inp])
    out = out[1] if isinstance(out, tuple) else out
    np.testing.assert_allclose(out.cpu().numpy(), z["eval_logits_b0"], atol=TOL, rtol=0)


def _step(eng, blocks, feats, labels, outn, inp):
    from glnn_amd import ops
    eng.step_sage(blocks, ops.as_feat(feats), labels, outn, 1.0, input_nodes=inp)


def test_dropout_steps_match_the_oracle_fed_the_library_masks():
    """Dropout 0.5: the engine's counter-based masks (ops.dropout_mask with the engine's per-layer seeds) fed to the oracle -> the same
    loss and gradients at every step, and the same parameters after three steps."""
    from glnn_amd import ops
    from glnn_amd.teacher import TeacherEngine
    z, batches, feats, labels, dev = _golden_on_device()
    dims = [int(d) for d in z["dims"]]
    p, lr = 0.5, 0.003
    model, opt = _model(dims, p=p, sd=so.sub(z, "init."), lr=lr)
    eng = TeacherEngine(model, opt)
    st = so.State(so.sub(z, "init."), 3, float(z["eps"]))
    for b in range(3):
        inp, outn, blks = dev[b]
        _step(eng, blks, feats, labels, outn, inp)
        masks = [ops.dropout_mask(len(batches[b][2][l][0]) - 1, dims[l + 1], p, eng._seed(l), DEV).cpu().numpy().astype(np.float64)
                 for l in range(2)]
        assert all(abs(m.mean() - (1 - p)) < 0.1 for m in masks)
        logits, cache = so.forward(st, batches[b][2], z["feats"][batches[b][0]], masks, p)
        loss, dl = so.loss_and_dlogits(logits, z["labels"][batches[b][1]])
        grads = so.backward(st, cache, dl, p)
        assert abs(eng.loss_out.item() - loss) < TOL
        for k, prm in model.named_parameters():
            np.testing.assert_allclose(prm.grad.cpu().numpy(), grads[k], atol=2e-5, rtol=1e-3, err_msg=f"step {b} {k}")
        so.adam(st, grads, lr)
    for k, v in _state(model).items():
        np.testing.assert_allclose(v, st.p[k], atol=5e-4, rtol=0, err_msg=k)


def _hub_batches(full, n=20000, dims=(40, 64, 64, 9), seed=9):
    from glnn_amd import ops
    from glnn_amd.graph import MultiLayerFullNeighborSampler, MultiLayerNeighborSampler, NodeDataLoader
    # symmetric: the 3000-edge hub is a long row of the blocks AND of their transposes (the backward's long-row role)
    indptr, indices = random_graph(n, 6, seed=seed, power=0.6, hub=3000, isolated=30, symmetric=True)
    rs = np.random.RandomState(seed)
    fd = ops.as_feat(torch.from_numpy(rs.standard_normal((n, dims[0])).astype(np.float32)).to(DEV))
    ld = torch.from_numpy(rs.randint(0, dims[-1], n).astype(np.int64)).to(DEV)
    g = _graph(indptr, indices)
    if full:
        batches = list(NodeDataLoader(g, torch.arange(512), MultiLayerFullNeighborSampler(3), batch_size=256, shuffle=False, seed=5))
    else:
        batches = list(NodeDataLoader(g, torch.arange(1536), MultiLayerNeighborSampler([5, 10, 15]), batch_size=512, shuffle=False, seed=5))
    return fd, ld, batches


def _run_states(dims, p, fd, ld, batches, wd=0.0):
    from glnn_amd.teacher import TeacherEngine
    model, opt = _model(list(dims), p=p, lr=0.003, wd=wd, seed=2)
    eng = TeacherEngine(model, opt)
    for input_nodes, output_nodes, blocks in batches:
        eng.step_sage(blocks, fd, ld, output_nodes, 1.0, input_nodes=input_nodes)
    torch.cuda.synchronize()
    return ([t.detach().clone() for t in model.state_dict().values()] + [opt.state[q]["exp_avg"].clone() for q in model.parameters()] +
            [eng.grad(q).clone() for q in model.parameters()] + [eng.loss_out.clone()]), eng


def _assert_equal(a, b):
    diffs = [float((x.double() - y.double()).abs().max()) for x, y in zip(a, b)]
    assert all(torch.equal(x, y) for x, y in zip(a, b)), diffs


@pytest.mark.parametrize("p,full", [(0.3, False), (0.0, True), (0.5, True)])
def test_equal_result_forms(p, full, monkeypatch):
    """The gather-tail form equals the materialised h (GLNN_TEACHER_GATHER_TAIL=0) bit for bit; the one-call step equals fwd_bwd + Adam
    (GLNN_TEACHER_ONE_CALL=0) bit for bit; the LayerNorm backward in the transposed aggregation's epilogue agrees with the aggregation +
    glnn_layernorm_bwd_f32 (GLNN_SAGE_FUSE_LN_BWD=0) to rounding."""
    from glnn_amd import _lib
    dims = (40, 64, 64, 9)
    fd, ld, batches = _hub_batches(full, dims=dims)
    if full:
        assert max(int(b.in_degrees().max()) for b in batches[0][2][1:]) > 128
    base, _ = _run_states(dims, p, fd, ld, batches)
    monkeypatch.setenv("GLNN_TEACHER_GATHER_TAIL", "0")
    mat, eng = _run_states(dims, p, fd, ld, batches)
    assert not eng.gather_tail
    _assert_equal(base, mat)
    monkeypatch.setenv("GLNN_TEACHER_GATHER_TAIL", "1")
    monkeypatch.setenv("GLNN_TEACHER_ONE_CALL", "0")
    two, eng = _run_states(dims, p, fd, ld, batches)
    assert not eng._one_call
    _assert_equal(base, two)
    monkeypatch.setenv("GLNN_TEACHER_ONE_CALL", "1")
    monkeypatch.setenv("GLNN_SAGE_FUSE_LN_BWD", "0")
    _lib.lib().glnn_reload_options()
    try:
        unf, _ = _run_states(dims, p, fd, ld, batches[:1])
    finally:
        monkeypatch.delenv("GLNN_SAGE_FUSE_LN_BWD")
        _lib.lib().glnn_reload_options()
    one, _ = _run_states(dims, p, fd, ld, batches[:1])           # (one step: Adam would turn rounding-size gradient differences into lr-size ones)
    for a, b in zip(one, unf):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-4, rtol=1e-3)


def test_hidden_width_above_256_matches_the_oracle():
    """Hidden width 300: h is materialised by the LayerNorm forward and the backward takes aggregation + glnn_layernorm_bwd_f32."""
    from glnn_amd.teacher import TeacherEngine
    z, batches, feats, labels, dev = _golden_on_device()
    dims = [20, 300, 300, 6]
    model, opt = _model(dims)
    sd0 = _state(model)
    eng = TeacherEngine(model, opt)
    inp, outn, blks = dev[0]
    _step(eng, blks, feats, labels, outn, inp)
    assert eng._sage_desc.layer[0].h is not None
    st = so.State(sd0, 3)
    logits, cache = so.forward(st, batches[0][2], z["feats"][batches[0][0]])
    loss, dl = so.loss_and_dlogits(logits, z["labels"][batches[0][1]])
    grads = so.backward(st, cache, dl)
    assert abs(eng.loss_out.item() - loss) < TOL
    for k, prm in model.named_parameters():
        np.testing.assert_allclose(prm.grad.cpu().numpy(), grads[k], atol=2e-5, rtol=1e-3, err_msg=k)


def test_two_identical_runs_are_bit_identical():
    dims = (40, 64, 64, 9)
    fd, ld, batches = _hub_batches(True, dims=dims)
    a, _ = _run_states(dims, 0.3, fd, ld, batches, wd=5e-4)
    b, _ = _run_states(dims, 0.3, fd, ld, batches, wd=5e-4)
    _assert_equal(a, b)
    assert bool(torch.isfinite(a[-1]).all())


def test_engine_gradients_match_the_autograd_path():
    """Model in training mode + loss.backward() (glnn_amd.autograd, norm_act_drop with nn.LayerNorm) on the same blocks: the same
    gradients as the engine's explicit backward."""
    from glnn_amd.teacher import TeacherEngine
    z, batches, feats, labels, dev = _golden_on_device()
    dims = [int(d) for d in z["dims"]]
    inp, outn, blks = dev[1]
    ref, _ = _model(dims, sd=so.sub(z, "init."))
    out = ref(blks, feats[inp])
    logits = out[1] if isinstance(out, tuple) else out
    loss = torch.nn.functional.nll_loss(logits.log_softmax(1), labels[outn])
    loss.backward()
    model, opt = _model(dims, sd=so.sub(z, "init."))
    eng = TeacherEngine(model, opt)
    _step(eng, blks, feats, labels, outn, inp)
    assert abs(eng.loss_out.item() - loss.item()) < TOL
    for (k, a), (_, b) in zip(ref.named_parameters(), model.named_parameters()):
        np.testing.assert_allclose(b.grad.cpu().numpy(), a.grad.cpu().numpy(), atol=2e-5, rtol=1e-3, err_msg=k)


def test_descriptor_rebuild_after_load_state_dict_a_changed_eps_and_a_replaced_layernorm():
    """load_state_dict keeps the tensors (same descriptor, new values); a changed LayerNorm eps is part of the descriptor's signature
    (rebuilt); a replaced nn.LayerNorm module gets a new engine (get_engine).  Each time the next step's gradients are the oracle's for
    the state the model then holds."""
    from glnn_amd import teacher
    z, batches, feats, labels, dev = _golden_on_device()
    dims = [int(d) for d in z["dims"]]
    model, opt = _model(dims, sd=so.sub(z, "init."))
    eng = teacher.get_engine(model, opt)
    inp, outn, blks = dev[0]
    _step(eng, blks, feats, labels, outn, inp)

    def check(eng, b, eps):
        sd = _state(model)
        inp, outn, blks = dev[b]
        _step(eng, blks, feats, labels, outn, inp)
        st = so.State(sd, 3, eps)
        logits, cache = so.forward(st, batches[b][2], z["feats"][batches[b][0]])
        loss, dl = so.loss_and_dlogits(logits, z["labels"][batches[b][1]])
        grads = so.backward(st, cache, dl)
        assert abs(eng.loss_out.item() - loss) < TOL
        for k, prm in model.named_parameters():
            np.testing.assert_allclose(prm.grad.cpu().numpy(), grads[k], atol=2e-5, rtol=1e-3, err_msg=k)

    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in so.sub(z, "final.").items()})
    desc = eng._sage_desc
    check(eng, 1, float(z["eps"]))
    assert eng._sage_desc is desc
    for nm in model.encoder.norms:
        nm.eps = 1e-3
    check(eng, 2, 1e-3)
    assert eng._sage_desc is not desc
    ln = torch.nn.LayerNorm(dims[1], eps=1e-3).to(DEV)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-0.2, 0.2)
    model.encoder.norms[0] = ln
    opt2 = torch.optim.Adam(model.parameters(), lr=0.01)
    eng2 = teacher.get_engine(model, opt2)
    assert eng2 is not eng
    check(eng2, 0, 1e-3)


def test_one_layer_layernorm_teacher_steps_through_the_plain_entry():
    """A one-layer encoder has no hidden tail and no norm module: with norm_type "layer" the engine builds no LayerNorm side descriptor and
    the step is the plain entry's -- the bits of the same model built with norm_type "none"."""
    from glnn_amd import teacher
    from glnn_amd.models import Model
    n_src, n_dst, d, c = 70, 23, 19, 7
    rs = np.random.RandomState(5)
    indptr = np.concatenate([[0], np.cumsum(rs.randint(0, 6, n_dst))])
    blocks = [_graph(indptr, rs.randint(0, n_src, indptr[-1]), n_src)]
    feats, labels = torch.from_numpy(rs.standard_normal((n_src, d)).astype(np.float32)).to(DEV), torch.from_numpy(rs.randint(0, c, n_dst)).to(DEV)
    rows, inp = torch.arange(n_dst, device=DEV), torch.arange(n_src, device=DEV)
    out = {}
    for norm in ("layer", "none"):
        torch.manual_seed(3)
        model = Model(dict(model_name="SAGE", num_layers=1, feat_dim=d, hidden_dim=8, label_dim=c, dropout_ratio=0.5, norm_type=norm,
                           device=DEV)).train()
        eng = teacher.get_engine(model, torch.optim.Adam(model.parameters(), lr=0.01))
        for _ in range(2):
            eng.step_sage(blocks, feats, labels, rows, 1.0, input_nodes=inp)
        assert eng._sage_ln is None and eng.step_count == 2 and np.isfinite(eng.loss_out.item())
        out[norm] = (eng.loss_out.clone(), [p.detach().clone() for p in model.parameters()])
    assert torch.equal(out["layer"][0], out["none"][0])
    _assert_equal(out["layer"][1], out["none"][1])


def _run_cli(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("setting", ["tran", "ind"])
def test_train_teacher_cli_sage_layernorm_then_student(tmp_path, setting):
    common = ["--dataset", "synthetic-cora", "--teacher", "SAGE", "--device", "0", "--max_epoch", "4", "--patience", "3",
              "--exp_setting", setting, "--save_results"]
    _run_cli("train_teacher.py", common + ["--norm_type", "layer"], tmp_path)
    base = tmp_path / "outputs" / ("transductive" if setting == "tran" else "inductive/split_rate_0.2") / "synthetic-cora"
    tdir = base / "SAGE" / "seed_0"
    out_t = np.load(tdir / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)
    _run_cli("train_student.py", common + ["--student", "MLP", "--lamb", "0.5"], tmp_path)
    out_s = np.load(base / "SAGE_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
