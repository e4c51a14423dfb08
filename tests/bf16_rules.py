"""The bf16 comparison rules of the kernel tests, stated once for the files that share them (the same two rules and constants as
tests/test_bf16_inference_gpu.py): test inputs are exactly representable in bf16, so their products are exact in fp64; an fp32 output must
agree with the fp64 result within TOL, a bf16 output within one bf16 ulp of that result rounded to bf16 -- or within ABS_FLOOR of it, the
fp32 arithmetic's own error, where cancellation leaves a value near zero."""
import numpy as np
import torch

TOL = 1e-4
ABS_FLOOR = 2e-5


def bits(t):
    """bf16 tensor -> int64 numpy bit patterns (0..65535)."""
    return t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def ordered(b):
    """bf16 bit patterns -> integers in value order (+0 and -0 equal): neighbours in value differ by 1."""
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def round_bf16(a64):
    return torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).to(torch.bfloat16)


def assert_within_one_ulp(got_bf16, want64):
    got = ordered(bits(got_bf16))
    want = ordered(bits(round_bf16(want64)))
    diff = np.abs(got - want)
    err = np.abs(got_bf16.float().cpu().numpy().astype(np.float64) - want64)
    bad = (diff > 1) & (err > ABS_FLOOR)
    assert not bad.any(), f"{int(bad.sum())} elements more than one bf16 ulp and {ABS_FLOOR} away (max err {err[bad].max()})"
