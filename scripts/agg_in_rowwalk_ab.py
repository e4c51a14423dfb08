"""The kept-aggregate hit path (ops.sage_fused(agg_in=...)) on the products layer-1 matrix, 2,449,029 x 100 -> 256 with the scale / shift /
ReLU epilogue: GLNN_AGG_IN_ROWWALK=0 (sage_fused_kernel<.., kAggIn>) against =1 (the wave-walk GEMM reading the packed weight) and against
ops.gemm (the same wave-walk kernel reading the raw weight), one process, HIP events around each launch.
    python scripts/agg_in_rowwalk_ab.py [--rows N] [--rounds 3] [--launches 20]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import _lib, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2449029)
    ap.add_argument("--d-in", type=int, default=100)
    ap.add_argument("--d-out", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    m, d_in, d_out = a.rows, a.d_in, a.d_out
    g = torch.Generator(device="cuda").manual_seed(0)
    agg = ops.feat_empty(m, d_in, "cuda:0", zero=True)
    agg.copy_(torch.randn((m, d_in), device="cuda", generator=g))
    w = torch.randn((d_out, d_in), device="cuda", generator=g) * 0.1
    scale = torch.rand(d_out, device="cuda", generator=g) + 0.5
    shift = torch.rand(d_out, device="cuda", generator=g) - 0.5
    wp = ops.pack_weight(w)
    out = ops.feat_empty(m, d_out, "cuda:0")

    def switch(v):
        os.environ["GLNN_AGG_IN_ROWWALK"] = v
        _lib.lib().glnn_reload_options()

    forms = {
        "agg_in fused (switch 0)": ("0", lambda: ops.sage_fused(None, None, None, m, w, ep_scale=scale, ep_shift=shift, relu=True, out=out,
                                                                w_packed=wp, agg_in=agg)),
        "agg_in walk  (switch 1)": ("1", lambda: ops.sage_fused(None, None, None, m, w, ep_scale=scale, ep_shift=shift, relu=True, out=out,
                                                                w_packed=wp, agg_in=agg)),
        "ops.gemm     (raw W)   ": ("1", lambda: ops.gemm(ops.as_feat(agg), w, ep_scale=scale, ep_shift=shift, relu=True, out=out)),
    }
    results = {}
    for name, (sw, fn) in forms.items():
        switch(sw)
        fn()
        torch.cuda.synchronize()
        results[name] = out.clone()
    names = list(forms)
    print(f"{m} x {d_in} -> {d_out}, {a.launches} launches per round after 3 warm-up launches, min / median / max in ms")
    print("outputs equal:", all(torch.equal(results[names[0]], results[n]) for n in names[1:]))
    for r in range(a.rounds):
        line = []
        for name, (sw, fn) in forms.items():
            switch(sw)
            for _ in range(3):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
            for s, e in ev:
                s.record()
                fn()
                e.record()
            torch.cuda.synchronize()
            t = np.array([s.elapsed_time(e) for s, e in ev])
            line.append(f"{name} {t.min():.3f} / {np.median(t):.3f} / {t.max():.3f}")
        print(f"round {r}: " + "    ".join(line), flush=True)


if __name__ == "__main__":
    main()
