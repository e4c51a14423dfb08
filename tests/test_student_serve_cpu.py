"""Host side of the bf16 student serving path (no GPU needed): the two C entries and their bindings, argument refusals that happen before
any launch, the --serve_dtype flag, compile_student's refusals, and the accuracy of the CPU oracle itself -- so that the bounds the GPU
tests hold the kernels to are known to be satisfiable before a GPU is involved."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import student_serve_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("glnn_gemm_bf16", "glnn_mlp_forward_bf16")


def test_serve_entries_are_exported_and_bound():
    import __graft_entry__ as ge
    from glnn_amd import _lib
    h = ctypes.CDLL(ge.build())
    header = open(os.path.join(ROOT, "include", "glnn_hip.h")).read()
    for name in NEW_ENTRIES:
        assert hasattr(h, name) and name in _lib.SIGNATURES
        m = re.search(r"GLNN_API int " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
    h.glnn_abi_version.restype = ctypes.c_int
    assert h.glnn_abi_version() == 12 and _lib.ABI_VERSION == 12
    assert _lib.lib().glnn_struct_bytes(7) == ctypes.sizeof(_lib.MlpServeDesc)
    assert os.path.exists(os.path.join(ROOT, "graphless-neural-networks_amd", "csrc", "gemm_bf16.hip"))


def _gemm(h, a=None, lda=8, a_dtype=1, m=4, k=8, w=None, ldw=64, n=4, out=None, ldo=8, out_dtype=1, lsm=0):
    return h.glnn_gemm_bf16(a, lda, a_dtype, m, k, w, ldw, n, None, None, 0, out, ldo, out_dtype, lsm, None)


def test_serve_entries_report_invalid_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    err = lambda: h.glnn_last_error()
    assert _gemm(h) == -1 and b"glnn_gemm_bf16: null pointer" in err()
    assert _gemm(h, a_dtype=5) == -1 and b"glnn_gemm_bf16" in err() and b"a_dtype" in err()
    assert _gemm(h, out_dtype=2) == -1 and b"glnn_gemm_bf16" in err() and b"out_dtype" in err()
    assert _gemm(h, lda=12) == -1 and b"glnn_gemm_bf16" in err() and b"lda" in err()          # bf16 rows: multiples of 8
    assert _gemm(h, a_dtype=0, lda=4) == -1 and b"lda" in err()                                # fp32 rows: >= k
    assert _gemm(h, ldw=40) == -1 and b"glnn_gemm_bf16" in err() and b"ldw" in err()          # weights: multiples of 64
    assert _gemm(h, ldo=4) == -1 and b"glnn_gemm_bf16" in err() and b"ldo" in err()
    assert _gemm(h, n=100, ldo=104, out_dtype=0, lsm=1) == -1 and b"log_softmax" in err()     # a row's logits must sit in one tile
    assert _gemm(h, m=0) == 0                                                                  # empty: nothing to do, pointers unread
    d = _lib.MlpServeDesc()
    fwd = lambda desc, m=4, x_dtype=0, ld_buf=16: h.glnn_mlp_forward_bf16(desc, None, 8, x_dtype, m, None, None, ld_buf, None, 4, 0, None)
    assert fwd(None) == -1 and b"glnn_mlp_forward_bf16" in err()
    assert fwd(ctypes.byref(d)) == -1 and b"glnn_mlp_forward_bf16" in err() and b"num_layers" in err()
    d.num_layers = 2
    d.dims[0], d.dims[1], d.dims[2] = 8, 16, 4
    assert fwd(ctypes.byref(d)) == -1 and b"glnn_mlp_forward_bf16: null pointer" in err()
    assert fwd(ctypes.byref(d), x_dtype=3) == -1 and b"x_dtype" in err()
    assert fwd(ctypes.byref(d), ld_buf=12) == -1 and b"ld_buf" in err()
    assert fwd(ctypes.byref(d), m=0) == 0
    d.num_layers = _lib.MLP_MAX_LAYERS + 1
    assert fwd(ctypes.byref(d)) == -1 and b"num_layers" in err()


def test_student_cli_serve_dtype():
    from glnn_amd.cli import get_student_args
    from glnn_amd.train_and_eval import serve_dtype
    assert get_student_args([]).serve_dtype == "float32"
    assert serve_dtype(vars(get_student_args([]))) is torch.float32 and serve_dtype({}) is torch.float32
    assert serve_dtype(vars(get_student_args(["--serve_dtype", "bfloat16"]))) is torch.bfloat16
    with pytest.raises(SystemExit):
        get_student_args(["--serve_dtype", "float16"])


def _model(name, norm="none", layers=2):
    from glnn_amd.models import Model
    return Model(dict(model_name=name, num_layers=layers, feat_dim=8, hidden_dim=16, label_dim=3, dropout_ratio=0.0, norm_type=norm,
                      device="cpu"))


def test_compile_student_refusals_need_no_gpu():
    from glnn_amd import GlnnError, serve
    with pytest.raises(NotImplementedError):
        serve.compile_student(_model("GCN").eval())
    with pytest.raises(NotImplementedError):
        serve.compile_student(_model("MLP", norm="layer").eval())
    with pytest.raises(NotImplementedError):
        serve.compile_student(_model("MLP", norm="batch").train())
    with pytest.raises(NotImplementedError):
        serve.compile_student(_model("MLP", layers=9).eval())
    with pytest.raises(ValueError):
        serve.compile_student(_model("MLP").eval(), dtype=torch.float16)
    with pytest.raises(GlnnError):                                   # an acceptable student whose parameters live on the CPU
        serve.compile_student(_model("MLP", norm="batch").eval())


def test_evaluate_mini_batch_keeps_its_default_and_refuses_other_dtypes():
    import inspect
    from glnn_amd import GlnnError
    from glnn_amd.train_and_eval import evaluate_mini_batch
    sig = inspect.signature(evaluate_mini_batch)
    assert list(sig.parameters)[-1] == "dtype" and sig.parameters["dtype"].default is torch.float32
    with pytest.raises(GlnnError):
        evaluate_mini_batch(_model("MLP"), torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64), None, 2, None, dtype=torch.bfloat16)


@pytest.mark.parametrize("case", range(len(so.CASES)))
def test_oracle_accuracy(case):
    """What the oracle and its fp32 stand-in show on the six models of the end-to-end GPU test.  The GPU test holds the kernels to
    max(2e-3, 4 x stand-in distance) x row max against the oracle and to 2e-2 x max(1, row max) against the plain forward; here: the oracle
    alone stays within 1e-2 of the plain forward (half of that bound is left to the kernel), the stand-in stays within 5e-3 of the oracle (so
    four times it stays below the plain-forward bound), at least half of the rows are clear, and the stand-in's argmax agrees with the oracle's
    on at least 99 % of the clear rows."""
    dims, norm, n, cora = so.CASES[case]
    x, layers, norms = so.draw_case(dims, norm, n, seed=case, cora_like=cora)
    want = so.forward(x, layers, norms)
    plain = so.forward(x, layers, norms, round_storage=False)
    stand = so.forward(x, layers, norms, accumulate="fp32")
    e_plain, e_stand = so.rel_err(want, plain, floor=1.0), so.rel_err(stand, want)
    clear = so.clear_rows(want)
    agree = float((stand.argmax(1) == want.argmax(1))[clear].mean())
    print(f"{dims} {norm}: oracle vs plain {e_plain:.3g}, stand-in vs oracle {e_stand:.3g}, clear {clear.mean():.3f}, argmax on clear {agree:.4f}")
    assert e_plain <= 1e-2
    assert e_stand <= 5e-3
    assert clear.mean() >= 0.5
    assert agree >= 0.99
