"""bf16 serving of the MLP student on the GPU (csrc/gemm_bf16.hip, ops.gemm_bf16, glnn_amd.serve, evaluate_mini_batch(dtype=),
train_student.py --serve_dtype).  The single-product tests use inputs that are exactly representable in bf16, so the fp64 product is exact
(tests/bf16_rules.py); the end-to-end tests compare against tests/student_serve_oracle.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_rules as br
import student_serve_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 31, 257, 4099]
KS = [3, 100, 128, 1433, 2048]
NS = [7, 47, 256, 2048]
LSM_TOL = 1e-5          # fused log_softmax epilogue vs ops.log_softmax of the same call's fp32 logits (measured on an MI355X: 9.5e-7)


def _product_inputs(k, n, seed):
    """A [4099, k] and W [n, k] with N(0,1) and N(0,1)/sqrt(k) values rounded to bf16 (exact in fp64), epilogue vectors, the fp64 product."""
    rs = np.random.RandomState(seed)
    a = torch.from_numpy(rs.standard_normal((max(MS), k)).astype(np.float32)).to(torch.bfloat16)
    w = torch.from_numpy((rs.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)).to(torch.bfloat16)
    es = rs.uniform(0.5, 1.5, n).astype(np.float32)
    eh = rs.uniform(-0.3, 0.3, n).astype(np.float32)
    prod = a.double().numpy() @ w.double().numpy().T
    return a, w, es, eh, prod


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_gemm_bf16_against_fp64(k, n):
    _check_gemm_bf16(k, n, MS)


@pytest.mark.parametrize("n", [47, 256])
def test_gemm_bf16_on_the_32x32_mfma_against_fp64(monkeypatch, n):
    """GLNN_GEMM_BF16_MFMA16=0: the MF = 32 instantiations of gemm_bf16_kernel (v_mfma_f32_32x32x16_bf16), both tile widths, every
    operand / output type and the log-softmax epilogue, under the bounds of the default shape."""
    monkeypatch.setenv("GLNN_GEMM_BF16_MFMA16", "0")
    _check_gemm_bf16(100, n, [31, 257])


def _check_gemm_bf16(k, n, ms):
    from glnn_amd import ops
    a, w, es, eh, prod = _product_inputs(k, n, seed=1000 * k + n)
    a16 = ops.as_bf16_feat(a.to(DEV))
    a32 = a.float().to(DEV)
    wp = ops.pack_weight_bf16(w.float().to(DEV))
    assert wp.stride(0) % 64 == 0 and np.array_equal(br.bits(wp), br.bits(w))        # the pack is the plain rounding (exact here)
    est, eht = torch.from_numpy(es).to(DEV), torch.from_numpy(eh).to(DEV)
    worst32, worst_lsm = 0.0, 0.0
    for m in ms:
        for epi in (False, True):
            want = np.maximum(prod[:m] * es.astype(np.float64) + eh.astype(np.float64), 0.0) if epi else prod[:m]
            kw = dict(ep_scale=est, ep_shift=eht, relu=True) if epi else {}
            o32 = ops.gemm_bf16(a16[:m], wp, **kw)
            assert o32.dtype == torch.float32 and tuple(o32.shape) == (m, n)
            err = float(np.abs(o32.cpu().numpy().astype(np.float64) - want).max())
            worst32 = max(worst32, err)
            assert err <= br.TOL, (m, k, n, epi, err)
            o16 = ops.gemm_bf16(a16[:m], wp, out_dtype=torch.bfloat16, **kw)
            assert o16.dtype == torch.bfloat16 and o16.stride(0) % 8 == 0
            br.assert_within_one_ulp(o16, want)
            full = o16.as_strided((m, ops.round8(n)), (o16.stride(0), 1))
            assert (br.bits(full[:, n:]) == 0).all()                                  # padding columns written as 0
            # the fp32 operand is rounded in the operand path: the same bits as the pre-cast call
            p32 = ops.gemm_bf16(a32[:m], wp, **kw)
            p16 = ops.gemm_bf16(a32[:m], wp, out_dtype=torch.bfloat16, **kw)
            assert torch.equal(p32, o32) and np.array_equal(br.bits(p16), br.bits(o16)), (m, k, n, epi)
            if n <= 64:
                lp = ops.gemm_bf16(a16[:m], wp, log_softmax=True, **kw)
                ref = ops.log_softmax(o32)
                d = float((lp - ref).abs().max())
                worst_lsm = max(worst_lsm, d)
                assert d <= LSM_TOL, (m, k, n, epi, d)
                assert float((lp.double().exp().sum(1) - 1).abs().max()) <= 1e-4
                assert torch.equal(ops.gemm_bf16(a32[:m], wp, log_softmax=True, **kw), lp)
    print(f"k={k} n={n}: max |fp32 out - fp64| {worst32:.3g}, max |fused log_softmax - ops.log_softmax| {worst_lsm:.3g}")


def test_gemm_bf16_ignores_garbage_behind_k():
    """Columns [k, lda) of a bf16 A are not trusted: NaN padding (and a wider matrix's live columns) leave the result unchanged."""
    from glnn_amd import ops
    a, w, _, _, _ = _product_inputs(100, 47, seed=5)
    wp = ops.pack_weight_bf16(w.float().to(DEV))
    clean = ops.as_bf16_feat(a[:300].to(DEV))
    want = ops.gemm_bf16(clean, wp)
    wide = torch.full((300, 136), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, :100] = clean
    assert torch.equal(ops.gemm_bf16(wide[:, :100], wp), want)


def test_gemm_bf16_refusals():
    from glnn_amd import GlnnError, ops
    a = torch.zeros(4, 16, device=DEV)
    wp = ops.pack_weight_bf16(torch.zeros(100, 16, device=DEV))
    with pytest.raises(GlnnError):
        ops.gemm_bf16(a, wp, log_softmax=True)                       # 100 logits do not sit in one tile
    with pytest.raises(ValueError):
        ops.gemm_bf16(a, torch.zeros(100, 16, dtype=torch.bfloat16, device=DEV))   # rows not padded to 64
    with pytest.raises(GlnnError):
        ops.gemm_bf16(a.cpu(), wp)
    assert tuple(ops.gemm_bf16(a[:0], wp).shape) == (0, 100)


def _mlp(dims, norm, layers, norms):
    """models.Model("MLP") on the GPU carrying the drawn parameters, in eval mode."""
    from glnn_amd.models import Model
    L = len(dims) - 1
    model = Model(dict(model_name="MLP", num_layers=L, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.5,
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


def _case(i):
    dims, norm, n, cora = so.CASES[i]
    x, layers, norms = so.draw_case(dims, norm, n, seed=i, cora_like=cora)
    return dims, norm, x, layers, norms, _mlp(dims, norm, layers, norms)


@pytest.mark.parametrize("case", range(len(so.CASES)))
def test_served_student_against_the_oracle(case):
    """ServedStudent.logits against the fp64 oracle within max(2e-3, 4 x the stand-in's distance) x row max, against the plain fp64 forward
    within 2e-2 x max(1, row max), argmax agreement >= 0.99 on clear rows, clear rows at least half of all rows.  Measured on an MI355X
    (kernel / stand-in / bound): 1.07e-3 / 1.75e-3 / 7.0e-3, 9.7e-4 / 1.14e-3 / 4.6e-3, 1.29e-3 / 1.72e-3 / 6.9e-3, 1.5e-7 / 1.2e-7 / 2e-3,
    1.7e-7 / 1.5e-7 / 2e-3, 1.22e-3 / 1.14e-3 / 4.6e-3 for the six models in order (DESIGN.md section 6c has the whole table)."""
    from glnn_amd import serve
    dims, norm, x, layers, norms, model = _case(case)
    want = so.forward(x, layers, norms)
    stand = so.forward(x, layers, norms, accumulate="fp32")
    plain = so.forward(x, layers, norms, round_storage=False)
    xt = torch.from_numpy(x).to(DEV)
    s = serve.compile_student(model)
    got_t = s.logits(xt)
    assert got_t.dtype == torch.float32 and tuple(got_t.shape) == (x.shape[0], dims[-1])
    got = got_t.cpu().numpy().astype(np.float64)
    e_kernel, e_stand = so.rel_err(got, want), so.rel_err(stand, want)
    bound = max(2e-3, 4 * e_stand)
    e_plain = so.rel_err(got, plain, floor=1.0)
    clear = so.clear_rows(want)
    agree = float((got.argmax(1) == want.argmax(1))[clear].mean())
    print(f"{dims} {norm}: kernel {e_kernel:.3g} stand-in {e_stand:.3g} bound {bound:.3g} | vs plain {e_plain:.3g} | clear {clear.mean():.3f} "
          f"argmax on clear {agree:.4f} (all rows {float((got.argmax(1) == want.argmax(1)).mean()):.4f})")
    assert e_kernel <= bound
    assert e_plain <= 2e-2
    assert clear.mean() >= 0.5
    assert agree >= 0.99
    # bf16 features are taken as they are: the same bits as fp32 features rounded on the way in
    assert torch.equal(s.logits(xt.to(torch.bfloat16)), got_t)
    # log_probs = log_softmax of the same logits (fused epilogue: all six models have <= 64 classes)
    from glnn_amd import ops
    lp = s.log_probs(xt)
    assert float((lp - ops.log_softmax(got_t)).abs().max()) <= LSM_TOL


def test_rows_are_independent_and_runs_are_deterministic():
    from glnn_amd import serve
    from glnn_amd.train_and_eval import evaluate_mini_batch
    dims, norm, x, layers, norms, model = _case(2)
    xt = torch.from_numpy(x).to(DEV)
    s = serve.compile_student(model)
    full = s.logits(xt)
    assert torch.equal(s.logits(xt), full)                                           # run to run
    for a, b in ((0, 1), (1, 130), (77, 391), (129, 4096), (1000, 1001), (4095, 4096), (257, 2048 + 33)):
        assert torch.equal(s.logits(xt[a:b]), full[a:b]), (a, b)                      # ranges not aligned to any tile
    lp = s.log_probs(xt)
    assert torch.equal(s.log_probs(xt[300:1777]), lp[300:1777])
    labels = torch.from_numpy(np.random.RandomState(0).randint(0, dims[-1], x.shape[0])).to(DEV)
    ev = lambda out, lab: float((out.argmax(1) == lab).float().mean())
    o1, l1, s1 = evaluate_mini_batch(model, xt, labels, torch.nn.NLLLoss(), 512, ev, dtype=torch.bfloat16)
    o2, l2, s2 = evaluate_mini_batch(model, xt, labels, torch.nn.NLLLoss(), 10 ** 6, ev, dtype=torch.bfloat16)
    assert torch.equal(o1, o2) and torch.equal(o1, lp) and l1 == l2 and s1 == s2


def test_row_blocks_do_not_change_a_row(monkeypatch):
    """The served pass walks the rows in blocks of EVAL_BLOCK_ROWS; with a small block (not a multiple of the tile) the bits stay."""
    from glnn_amd import serve
    dims, norm, x, layers, norms, model = _case(5)
    xt = torch.from_numpy(x).to(DEV)
    want = serve.compile_student(model).log_probs(xt)
    monkeypatch.setattr(serve, "EVAL_BLOCK_ROWS", 1000)
    assert torch.equal(serve.compile_student(model).log_probs(xt), want)


def test_snapshot_follows_parameter_updates():
    """Staleness: a training pass through the student engine writes the parameters through raw pointers (ops.PARAM_EPOCH); the next bf16
    evaluation uses the new weights.  So do an in-place torch update and load_state_dict."""
    from glnn_amd import serve
    from glnn_amd.train_and_eval import evaluate_mini_batch, train_mini_batch
    dims, norm, x, layers, norms, model = _case(2)
    xt = torch.from_numpy(x).to(DEV)
    labels = torch.from_numpy(np.random.RandomState(1).randint(0, dims[-1], x.shape[0])).to(DEV)
    ev = lambda out, lab: float((out.argmax(1) == lab).float().mean())
    crit = torch.nn.NLLLoss()
    before = evaluate_mini_batch(model, xt, labels, crit, 512, ev, dtype=torch.bfloat16)[0].clone()
    served = model.__dict__["_served_student"]
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.0)
    train_mini_batch(model, xt, labels, 512, crit, opt)
    after = evaluate_mini_batch(model, xt, labels, crit, 512, ev, dtype=torch.bfloat16)[0]
    assert model.__dict__["_served_student"] is served                                # the cached snapshot re-packed itself
    assert not torch.equal(after, before)
    assert torch.equal(after, serve.compile_student(model.eval()).log_probs(xt))      # ... to exactly a fresh snapshot of the new state
    with torch.no_grad():
        model.encoder.layers[0].weight.mul_(0.5)
    assert torch.equal(evaluate_mini_batch(model, xt, labels, crit, 512, ev, dtype=torch.bfloat16)[0],
                       serve.compile_student(model).log_probs(xt))
    model.train()
    with pytest.raises(NotImplementedError):
        served.logits(xt)


def test_defaults_are_untouched():
    """evaluate_mini_batch without dtype, and with torch.float32, is the fp32 path bit for bit."""
    from glnn_amd import ops
    from glnn_amd.train_and_eval import evaluate_mini_batch
    dims, norm, x, layers, norms, model = _case(2)
    xt = torch.from_numpy(x).to(DEV)
    labels = torch.from_numpy(np.random.RandomState(2).randint(0, dims[-1], x.shape[0])).to(DEV)
    ev = lambda out, lab: float((out.argmax(1) == lab).float().mean())
    with torch.no_grad():
        want = ops.log_softmax(model.inference(None, xt))
    o0 = evaluate_mini_batch(model, xt, labels, torch.nn.NLLLoss(), 512, ev)[0]
    o1 = evaluate_mini_batch(model, xt, labels, torch.nn.NLLLoss(), 512, ev, dtype=torch.float32)[0]
    assert torch.equal(o0, want) and torch.equal(o1, want)
    assert "_served_student" not in model.__dict__
    with pytest.raises(NotImplementedError):
        model.inference(None, xt, dtype=torch.bfloat16)                                # that dtype means gathered-matrix storage: teachers only


def test_compile_student_refusals_on_the_gpu():
    from glnn_amd import serve
    from glnn_amd.models import Model
    conf = dict(num_layers=2, feat_dim=8, hidden_dim=16, label_dim=3, dropout_ratio=0.0, device=DEV)
    with pytest.raises(NotImplementedError):
        serve.compile_student(Model(dict(conf, model_name="SAGE", norm_type="none")).eval())
    with pytest.raises(NotImplementedError):
        serve.compile_student(Model(dict(conf, model_name="MLP", norm_type="layer")).eval())
    with pytest.raises(NotImplementedError):
        serve.compile_student(Model(dict(conf, model_name="MLP", norm_type="batch")).train())
    one = serve.compile_student(Model(dict(conf, model_name="MLP", norm_type="none", num_layers=1)).eval())      # a single Linear: no buffers
    assert tuple(one.logits(torch.zeros(5, 8, device=DEV)).shape) == (5, 3)


def test_student_cli_serve_dtype_round_trip(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--dataset", "synthetic-cora", "--device", "0", "--max_epoch", "3", "--patience", "3", "--exp_setting", "tran"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_teacher.py"), "--teacher", "SAGE"] + common, cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_student.py"), "--teacher", "SAGE", "--student", "MLP", "--serve_dtype", "bfloat16"]
                       + common, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.load(tmp_path / "outputs" / "transductive" / "synthetic-cora" / "SAGE_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out.shape == (2485, 7) and out.dtype == np.float32
    np.testing.assert_allclose(np.exp(out).sum(1), 1.0, atol=1e-4)
