"""The bits of the bf16 serving kernels (csrc/gemm_bf16.hip, csrc/mlp_fused_bf16.hip) as SHA-256 digests of their raw outputs, recorded at
one commit so that a later change of either kernel -- or of the device header they share -- can be held to "the same bits as before", not
only to "the two forms still agree" (tests/test_student_fused_gpu.py) or "within a tolerance of fp64" (tests/test_student_serve_gpu.py).

Inputs come from student_serve_oracle.draw_case with fixed seeds, so only digests are stored.  Cases (digests() below):
  chain   glnn_mlp_forward_bf16 over 197 rows of four chains: the logits of every prefix and the log-softmax of the whole chain, with bf16
          features and with fp32 features whose leading dimension is no multiple of 4, on both MFMA shapes (GLNN_GEMM_BF16_MFMA16 = 1, 0)
  gemm    glnn_gemm_bf16 alone (scale / shift / ReLU epilogue) at (m, k, n) = (257, 100, 47), (257, 1433, 256), (31, 3, 7): bf16 output
          (the whole padded row) and fp32 output, bf16 A, fp32 A on the scalar path and on the float4 path, both MFMA shapes
  fused   glnn_mlp_forward_fused_bf16 on the first three chains through a `rows` index with a repeat and an id outside the matrix

    python tests/golden/make_bf16_serve_bits.py --commit <id of the commit the library was built from> [--out tests/golden/bf16_serve_bits.json]

Needs an MI355X.  The record belongs to the machine image it was made on (compiler, expf / logf of the device library): make it and
check it (tests/test_bf16_serve_bits_gpu.py) on the same image; it is made at the commit BEFORE a change and not regenerated after it."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                        # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository root
import student_serve_oracle as so                                 # noqa: E402

DEV = "cuda:0"
RECORD = os.path.join(HERE, "bf16_serve_bits.json")
M = 197
CHAINS = [((20, 32, 6), "none"), ((300, 320, 5), "none"), ((100, 256, 256, 47), "batch"), ((16, 24, 40, 8, 72, 136, 264, 520, 3), "batch")]
FUSED_CHAINS = 3                                                  # the first three: what the one-launch form takes on every device
GEMMS = [(257, 100, 47), (257, 1433, 256), (31, 3, 7)]
SWITCH = "GLNN_GEMM_BF16_MFMA16"


def sha(t):
    t = t.contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def fold(layer, norm):
    """(ep_scale or None, ep_shift) of one layer on the device: bias and BatchNorm(eval) folded in fp32 as serve.ServedStudent folds them."""
    b = torch.from_numpy(layer["bias"]).to(DEV)
    if norm is None:
        return None, b
    n = {k: torch.from_numpy(v).to(DEV) for k, v in norm.items()}
    s = (n["weight"] / torch.sqrt(n["running_var"] + 1e-5)).contiguous()
    return s, ((b - n["running_mean"]) * s + n["bias"]).contiguous()


def desc(layers, norms):
    from glnn_amd import _lib, ops
    L = len(layers)
    d = _lib.MlpServeDesc()
    d.num_layers = L
    d.dims[0] = layers[0]["weight"].shape[1]
    keep = []
    for l, lay in enumerate(layers):
        w = ops.pack_weight_bf16(torch.from_numpy(lay["weight"]).to(DEV))
        s, b = fold(lay, norms[l] if norms is not None and l != L - 1 else None)
        keep += [w, s, b]
        d.dims[l + 1] = lay["weight"].shape[0]
        d.w[l], d.ldw[l] = w.data_ptr(), w.stride(0)
        d.ep_scale[l] = s.data_ptr() if s is not None else None
        d.ep_shift[l] = b.data_ptr()
    return d, keep


def prefix(d, l):
    from glnn_amd import _lib
    p = _lib.MlpServeDesc()
    ctypes.memmove(ctypes.byref(p), ctypes.byref(d), ctypes.sizeof(p))
    p.num_layers = l
    return p


def chain(d, x, lsm):
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


def fused(d, x, rows, lsm):
    from glnn_amd import ops
    out = torch.full((rows.numel(), d.dims[d.num_layers]), 5.0, dtype=torch.float32, device=DEV)
    return ops.mlp_forward_fused_bf16(d, x, out, rows=rows, log_softmax=lsm)


def forms(x_h, aligned=False):
    """{name: device matrix}: bf16 rows, fp32 rows whose leading dimension is no multiple of 4 and (aligned) fp32 float4 rows."""
    from glnn_amd import ops
    x = torch.from_numpy(x_h).to(DEV)
    n, k = x.shape
    buf = torch.zeros((n, k if k % 4 else k + 1), dtype=torch.float32, device=DEV)
    buf[:, :k] = x
    res = {"bf16": ops.as_bf16_feat(x.to(torch.bfloat16)), "fp32-unaligned": buf[:, :k]}
    assert ops._ld(res["fp32-unaligned"]) % 4 != 0
    if aligned:
        a = ops.feat_empty(n, k, DEV, zero=True)
        a.copy_(x)
        res["fp32-aligned"] = a
    return res


def _one_setting(tag, with_fused):
    from glnn_amd import ops
    res = {}
    for c, (dims, norm) in enumerate(CHAINS):
        x_h, layers, norms = so.draw_case(dims, norm, M, seed=500 + c)
        d, keep = desc(layers, norms)
        L = len(dims) - 1
        name = "x".join(str(v) for v in dims)
        rs = np.random.RandomState(900 + c)
        ids = rs.randint(0, M, M).astype(np.int64)
        ids[4] = ids[3]                                           # a repeat
        ids[150] = M                                              # one id outside x: computed from an all-zero row (check_rows=False)
        rows = torch.from_numpy(ids).to(DEV)
        for form, x in forms(x_h).items():
            for l in range(1, L + 1):
                res[f"chain {name} {form} {tag} prefix{l}"] = sha(chain(prefix(d, l), x, False))
            res[f"chain {name} {form} {tag} log_softmax"] = sha(chain(d, x, True))
            if with_fused and c < FUSED_CHAINS:
                assert ops.mlp_fused_bf16_tile_rows(d)[0] > 0, name
                for l in range(1, L + 1):
                    res[f"fused {name} {form} rows prefix{l}"] = sha(fused(prefix(d, l), x, rows, False))
                res[f"fused {name} {form} rows log_softmax"] = sha(fused(d, x, rows, True))
    for g, (m, k, n) in enumerate(GEMMS):
        x_h, layers, norms = so.draw_case((k, n, 2), "batch", m, seed=700 + g)
        w = ops.pack_weight_bf16(torch.from_numpy(layers[0]["weight"]).to(DEV))
        s, b = fold(layers[0], norms[0])
        for form, a in forms(x_h, aligned=True).items():
            o32 = ops.gemm_bf16(a, w, ep_scale=s, ep_shift=b, relu=True)
            o16 = ops.gemm_bf16(a, w, ep_scale=s, ep_shift=b, relu=True, out_dtype=torch.bfloat16)
            whole = o16.as_strided((m, ops.round8(n)), (o16.stride(0), 1))       # the padding columns with it
            res[f"gemm {m}x{k}x{n} {form} {tag} out-fp32"] = sha(o32)
            res[f"gemm {m}x{k}x{n} {form} {tag} out-bf16"] = sha(whole)
    return res


def digests():
    """{case name: SHA-256 of the output's raw bytes}.  Flips GLNN_GEMM_BF16_MFMA16 and puts it back."""
    from glnn_amd import _lib
    h = _lib.lib()
    before = os.environ.get(SWITCH)
    res = {}
    try:
        for value, tag in (("1", "mfma16"), ("0", "mfma32")):
            os.environ[SWITCH] = value
            h.glnn_reload_options()
            res.update(_one_setting(tag, with_fused=value == "1"))         # the one-launch form exists on the 16x16x32 shape only
    finally:
        if before is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = before
        h.glnn_reload_options()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit the library under test was built from")
    ap.add_argument("--out", default=RECORD)
    args = ap.parse_args()
    rec = {"what": "SHA-256 of the raw output bytes of the bf16 serving kernels; cases: tests/golden/make_bf16_serve_bits.py",
           "commit": args.commit, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "digests": digests()}
    assert digests() == rec["digests"], "the outputs differ run to run: nothing to record"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(rec['digests'])} digests -> {args.out}")


if __name__ == "__main__":
    main()
