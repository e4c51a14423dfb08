"""Host side of the bf16 teacher-forward storage (no GPU needed): the C entries and their bindings, argument refusals that happen before
any launch, the padded-ld helpers and the teacher command line's --inference_dtype."""
import ctypes

import pytest
import torch

NEW_ENTRIES = ("glnn_cast_f32_bf16", "glnn_spmm_csr_bf16", "glnn_sage_fused_bf16")


def test_bf16_entries_are_exported_and_bound():
    import __graft_entry__ as ge
    from glnn_amd import _lib
    h = ctypes.CDLL(ge.build())
    for name in NEW_ENTRIES:
        assert hasattr(h, name) and name in _lib.SIGNATURES
    h.glnn_abi_version.restype = ctypes.c_int
    assert h.glnn_abi_version() == 12


def test_bf16_entries_report_invalid_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    assert h.glnn_spmm_csr_bf16(None, None, 4, 4, None, 8, 4, 1, None, None, None, 8, None, None, None, 0, None, 8, 0, None) == -1
    assert b"glnn_spmm_csr_bf16: null pointer" in h.glnn_last_error()
    assert h.glnn_spmm_csr_bf16(None, None, 0, 0, None, 8, 4, 1, None, None, None, 8, None, None, None, 0, None, 8, 0, None) == 0   # empty
    assert h.glnn_sage_fused_bf16(None, None, 4, 4, None, 8, 4, None, 8, None, 4, None, None, 0, None, 4, 0, None, 0, None, 0, 0,
                                  None, None) == -1
    assert b"glnn_sage_fused_bf16" in h.glnn_last_error()
    assert h.glnn_cast_f32_bf16(None, 4, 4, 4, None, 8, None) == -1
    assert b"glnn_cast_f32_bf16: null pointer" in h.glnn_last_error()


def test_padded_bf16_helpers():
    from glnn_amd import ops
    assert [ops.round8(d) for d in (1, 7, 8, 9, 47, 100, 256)] == [8, 8, 8, 16, 48, 104, 256]
    b = ops.bf16_empty(5, 47, "cpu", zero=True)
    assert b.dtype == torch.bfloat16 and tuple(b.shape) == (5, 47) and b.stride(0) == 48
    assert ops.as_bf16_feat(b) is b
    c = ops.as_bf16_feat(torch.ones(5, 47, dtype=torch.bfloat16))          # ld 47: copied into a padded buffer
    assert c.stride(0) == 48 and torch.equal(c, torch.ones(5, 47, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.as_bf16_feat(torch.ones(5, 47))


def test_bf16_ops_refuse_cpu_tensors():
    from glnn_amd import GlnnError, ops
    x = torch.zeros(4, 8, dtype=torch.bfloat16)
    with pytest.raises(GlnnError):
        ops.to_bf16(torch.zeros(4, 8))
    with pytest.raises(GlnnError):
        ops.spmm(torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), x, 4, ops.AGG_SUM)
    with pytest.raises(GlnnError):
        ops.sage_fused(torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), x, 4, torch.zeros(8, 8))


def test_teacher_cli_inference_dtype():
    from glnn_amd.cli import get_teacher_args
    from glnn_amd.train_and_eval import inference_dtype
    assert get_teacher_args([]).inference_dtype == "float32"
    assert inference_dtype(vars(get_teacher_args([]))) is torch.float32
    args = get_teacher_args(["--teacher", "SAGE", "--inference_dtype", "bfloat16"])
    assert inference_dtype(vars(args)) is torch.bfloat16
    assert inference_dtype({}) is torch.float32
    for teacher in ("GCN", "APPNP", "MLP"):
        with pytest.raises(SystemExit):
            get_teacher_args(["--teacher", teacher, "--inference_dtype", "bfloat16"])
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "SAGE", "--inference_dtype", "float16"])


def test_student_cli_has_no_inference_dtype():
    from glnn_amd.cli import get_student_args
    with pytest.raises(SystemExit):
        get_student_args(["--inference_dtype", "bfloat16"])


def test_model_inference_refuses_bf16_for_non_sage_without_a_gpu():
    from glnn_amd.models import Model
    m = Model(dict(model_name="GCN", num_layers=2, feat_dim=8, hidden_dim=16, label_dim=3, dropout_ratio=0.0, norm_type="none",
                   device="cpu"))
    with pytest.raises(NotImplementedError):
        m.inference(None, torch.zeros(4, 8), dtype=torch.bfloat16)
