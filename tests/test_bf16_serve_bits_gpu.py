"""The bf16 serving kernels (csrc/gemm_bf16.hip, csrc/mlp_fused_bf16.hip and the device header they share, csrc/bf16_mfma_dev.h) against
the bits recorded before the header existed: tests/golden/bf16_serve_bits.json, SHA-256 digests of raw outputs made by
tests/golden/make_bf16_serve_bits.py at the commit named in the record.  The other serving tests hold the one-launch form to the chain and
the chain to an fp64 oracle under a tolerance; a change that moved both kernels' bits together would pass them and fails here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_bf16_serve_bits", os.path.join(GOLDEN, "make_bf16_serve_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_serving_bits_are_the_recorded_ones():
    gen = _generator()
    with open(gen.RECORD) as fh:
        rec = json.load(fh)
    want = rec["digests"]
    got = gen.digests()
    assert sorted(got) == sorted(want), "the cases of the generator and of the record differ: " + str(sorted(set(got) ^ set(want))[:5])
    # every family is there: chains on both MFMA shapes, single products of every operand / output type, the one-launch form through rows
    assert len(want) == 132 and {k.split()[0] for k in want} == {"chain", "gemm", "fused"}
    assert any(" mfma32 " in k for k in want) and any("out-bf16" in k for k in want) and any(k.endswith("log_softmax") for k in want)
    moved = [k for k in sorted(want) if got[k] != want[k]]
    assert not moved, (f"{len(moved)} of {len(want)} outputs no longer have the bits of commit {rec['commit'][:12]}, first: {moved[:6]}.  "
                       "Record and check belong to ONE machine image (compiler, device library: the log-softmax cases go through expf / "
                       "logf): after a change of image, regenerate the record at that commit on the new image before judging a kernel.")
