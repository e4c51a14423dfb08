"""Host side of the int8 teacher-forward storage (no GPU needed): the C entries and their bindings, argument refusals that happen before
any launch, the row-layout helpers, the teacher command line's --inference_dtype int8 and the numpy oracle's own properties."""
import ctypes

import numpy as np
import pytest
import torch

import int8_oracle as io

NEW_ENTRIES = ("glnn_quant_rows_i8", "glnn_spmm_sage_gcn_i8", "glnn_sage_fused_i8")
UNSUPPORTED = -2


def test_int8_entries_are_exported_and_bound():
    import __graft_entry__ as ge
    from glnn_amd import _lib
    h = ctypes.CDLL(ge.build())
    for name in NEW_ENTRIES:
        assert hasattr(h, name) and name in _lib.SIGNATURES
    h.glnn_abi_version.restype = ctypes.c_int
    assert h.glnn_abi_version() == 12
    assert _lib.ABI_VERSION == 12


def test_int8_entries_report_invalid_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    # quantise: null pointers, the empty call, a leading dimension that is not round16(d + 4), a row wider than 256
    assert h.glnn_quant_rows_i8(None, 4, 4, 4, None, 16, None) == -1
    assert b"glnn_quant_rows_i8: null pointer" in h.glnn_last_error()
    assert h.glnn_quant_rows_i8(None, 4, 0, 4, None, 16, None) == 0
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.glnn_quant_rows_i8(p, 13, 2, 13, p, 16, None) == UNSUPPORTED            # 13 columns need 32 bytes
    assert b"glnn_quant_rows_i8" in h.glnn_last_error() and b"ldo" in h.glnn_last_error()
    assert h.glnn_quant_rows_i8(p, 257, 2, 257, p, 272, None) == UNSUPPORTED
    assert b"glnn_quant_rows_i8" in h.glnn_last_error() and b"256" in h.glnn_last_error()
    # aggregation
    assert h.glnn_spmm_sage_gcn_i8(None, None, 4, 4, None, 16, 4, None, 16, None, None, 0, None, 4, 0, None) == -1
    assert b"glnn_spmm_sage_gcn_i8: null pointer" in h.glnn_last_error()
    assert h.glnn_spmm_sage_gcn_i8(None, None, 0, 0, None, 16, 4, None, 16, None, None, 0, None, 4, 0, None) == 0
    assert h.glnn_spmm_sage_gcn_i8(p, p, 4, 4, p, 32, 4, p, 16, None, None, 0, p, 4, 0, None) == UNSUPPORTED
    assert b"glnn_spmm_sage_gcn_i8" in h.glnn_last_error() and b"ldx" in h.glnn_last_error()
    assert h.glnn_spmm_sage_gcn_i8(p, p, 4, 4, p, 272, 257, p, 272, None, None, 0, p, 260, 0, None) == UNSUPPORTED
    assert h.glnn_spmm_sage_gcn_i8(p, p, 4, 4, p, 16, 4, p, 16, None, None, 0, p, 4, 1, None) == -1      # bf16 is not an output of this entry
    assert b"out_dtype" in h.glnn_last_error()
    assert h.glnn_spmm_sage_gcn_i8(p, p, 4, 4, p, 16, 4, p, 16, None, None, 0, p, 32, 2, None) == UNSUPPORTED   # int8 out: ldo = 16
    # fused layer
    assert h.glnn_sage_fused_i8(None, None, 4, 4, None, 16, 4, None, 16, None, 4, None, None, 0, None, 4, None, 0, None, 0, None, None) == -1
    assert b"glnn_sage_fused_i8: null pointer" in h.glnn_last_error()
    assert h.glnn_sage_fused_i8(None, None, 0, 0, None, 16, 4, None, 16, None, 4, None, None, 0, None, 4, None, 0, None, 0, None, None) == 0
    assert h.glnn_sage_fused_i8(p, p, 4, 4, p, 272, 257, p, 272, p, 4, None, None, 0, p, 4, None, 0, None, 0, None, None) == UNSUPPORTED
    assert b"glnn_sage_fused_i8" in h.glnn_last_error()
    assert h.glnn_sage_fused_i8(p, p, 4, 4, p, 48, 20, p, 32, p, 4, None, None, 0, p, 4, None, 0, None, 0, None, None) == UNSUPPORTED
    assert b"ldx" in h.glnn_last_error()


def test_int8_row_helpers():
    from glnn_amd import ops
    assert [ops.round16(d) for d in (1, 15, 16, 17, 47, 256, 260)] == [16, 16, 16, 32, 48, 256, 272]
    # the scale shares the last value piece up to 12 columns past a multiple of 16, and takes a piece of its own from 13
    assert [ops.int8_rows_ld(d) for d in (3, 12, 13, 16, 47, 100, 252, 253, 256)] == [16, 16, 32, 32, 64, 112, 256, 272, 272]
    assert [io.round16(d + 4) for d in (3, 12, 13, 100, 252, 253, 256)] == [ops.int8_rows_ld(d) for d in (3, 12, 13, 100, 252, 253, 256)]
    q = ops.int8_rows_empty(5, 47, "cpu", zero=True)
    assert q.dtype == torch.int8 and tuple(q.shape) == (5, 64) and q.is_contiguous() and q.data_ptr() % 16 == 0
    assert not q.any()
    for d in (0, 257):
        with pytest.raises(ValueError):
            ops.int8_rows_empty(5, d, "cpu")


def test_int8_ops_refuse_cpu_tensors():
    from glnn_amd import GlnnError, ops
    q = ops.int8_rows_empty(4, 8, "cpu", zero=True)
    ip, ix = torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(GlnnError):
        ops.to_int8_rows(torch.zeros(4, 8))
    with pytest.raises(GlnnError):
        ops.int8_rows_scale(q)
    with pytest.raises(GlnnError):
        ops.from_int8_rows(q, 8)
    with pytest.raises(GlnnError):
        ops.spmm_sage_gcn_i8(ip, ix, q, 8, 4)
    with pytest.raises(GlnnError):
        ops.sage_fused_i8(ip, ix, q, 8, 4, torch.zeros(8, 8))


def test_teacher_cli_inference_dtype_int8():
    from glnn_amd.cli import get_teacher_args
    from glnn_amd.train_and_eval import INFERENCE_DTYPES, inference_dtype
    args = get_teacher_args(["--teacher", "SAGE", "--inference_dtype", "int8"])
    assert args.inference_dtype == "int8" and inference_dtype(vars(args)) is torch.int8
    assert INFERENCE_DTYPES["int8"] is torch.int8
    assert get_teacher_args([]).inference_dtype == "float32"                       # the default stays fp32
    for teacher in ("GCN", "APPNP", "MLP"):
        with pytest.raises(SystemExit):
            get_teacher_args(["--teacher", teacher, "--inference_dtype", "int8"])
    with pytest.raises(SystemExit):
        get_teacher_args(["--teacher", "SAGE", "--sage_aggregator", "mean", "--inference_dtype", "int8"])
    # it composes with neighbour sampling on the command line
    args = get_teacher_args(["--teacher", "SAGE", "--inference_dtype", "int8", "--inference_fan_out", "15,15"])
    assert args.inference_dtype == "int8"


def test_model_inference_refuses_int8_for_non_sage_without_a_gpu():
    from glnn_amd.models import Model
    m = Model(dict(model_name="GCN", num_layers=2, feat_dim=8, hidden_dim=16, label_dim=3, dropout_ratio=0.0, norm_type="none",
                   device="cpu"))
    with pytest.raises(NotImplementedError, match="int8"):
        m.inference(None, torch.zeros(4, 8), dtype=torch.int8)


# ---- the oracle's own properties ---------------------------------------------------------------------------------------------------
def test_oracle_quantisation_error_is_half_a_step():
    rs = np.random.RandomState(0)
    for d in (3, 13, 100, 256):
        x = (rs.standard_normal((200, d)) * np.exp(rs.uniform(-8, 8, (200, 1)))).astype(np.float32)
        q, s = io.quantise_rows(x)
        assert q.dtype == np.int8 and s.dtype == np.float32 and np.abs(q.astype(np.int32)).max() <= 127
        assert (np.abs(q.astype(np.int32)).max(1) == 127).all()                    # the largest element sits on the last step
        err = np.abs(x.astype(np.float64) - io.dequant(q, s))
        # half a step, plus the rounding of s and of x * inv themselves (a few float32 ulps of the row maximum)
        assert (err <= s.astype(np.float64)[:, None] * (0.5 + 1e-4)).all()
        assert np.array_equal(s, (np.abs(x).max(1) / np.float32(127.0)).astype(np.float32))


def test_oracle_zero_nan_and_tie_rows():
    x = np.zeros((5, 7), np.float32)
    x[1] = [1.0, -2.0, np.nan, 0.5, 0, 0, 0]
    x[2] = [np.inf, 1, 2, 3, 4, 5, 6]
    x[3] = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -126.5]                              # s = 1 exactly: ties go to even
    x[4] = [-3.0, 1.0, 0, 0, 0, 0, 0]
    q, s = io.quantise_rows(x)
    assert s[0] == 0 and not q[0].any()
    assert np.isnan(s[1]) and np.isnan(s[2]) and not q[1].any() and not q[2].any()
    assert s[1:3].view(np.uint32).tolist() == [io.NAN_BITS, io.NAN_BITS]
    assert np.isnan(io.dequant(q, s)[1:3]).all()                                   # the whole row dequantises to NaN
    assert s[3] == 1.0 and q[3].tolist() == [127, 0, 2, 2, 0, -2, -126]
    assert q[4].tolist() == [-127, 42, 0, 0, 0, 0, 0]
    b = io.row_bytes(q, s)
    assert b.shape == (5, 16) and not b[:, 7:12].any()
    assert np.array_equal(b[:, 12:].copy().view("<f4")[:, 0].view(np.uint32), s.view(np.uint32))


def test_oracle_storage_points_are_felt():
    """The storage oracle differs from the exact forward by about one quantisation step, and its float32-arithmetic run stays close."""
    dims, norm = io.E2E[1]
    case = io.e2e_case(dims, norm)
    w64 = io.int8_storage_oracle(*case)
    w32 = io.int8_storage_oracle(*case, arith=np.float32).astype(np.float64)
    assert w64.shape == (io.E2E_N, dims[-1]) and np.isfinite(w64).all()
    assert io.row_relative(w32, w64) < 1e-2
