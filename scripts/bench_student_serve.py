"""fp32 vs bf16 serving pass of the MLP student (glnn_amd.serve, csrc/gemm_bf16.hip): the evaluate_mini_batch-equivalent pass -- row blocks
of EVAL_BLOCK_ROWS through the whole chain, log-probabilities out -- over random N(0,1) features and random weights (never zero-filled
operands: they read high) for MLP3w8 with BatchNorm at ogbn-products size (2,449,029 x 100 -> 2048 -> 2048 -> 47) and the arxiv student
(169,343 x 128 -> 256 -> 256 -> 40).  Warm-up, then ALTERNATING fp32 / bf16 rounds, the median of each; per-launch times of the bf16 chain
from device events around every launch (ops.set_timing) in a pass of its own.  One JSON line.

    python scripts/bench_student_serve.py [--reps 7] [--shapes products,arxiv] [--legs fp32,bf16] [--out profiles/student_serve_a.json]

`--legs fp32` uses only API that predates the serving path: run it on a checkout of the parent commit for the baseline the bar is
measured against (bf16 rows/s >= 3 x the parent's fp32 rows/s on the products shape)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import ops                                      # noqa: E402
from glnn_amd.models import Model                             # noqa: E402
from glnn_amd.train_and_eval import EVAL_BLOCK_ROWS           # noqa: E402

SHAPES = {"products": (2449029, [100, 2048, 2048, 47]), "arxiv": (169343, [128, 256, 256, 40])}
TEACHER_FORWARD_MS = (31.6, 32.0)        # the fp32 teacher forward over the products-shaped graph


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def run_shape(name, reps, legs, dev):
    rows, dims = SHAPES[name]
    torch.manual_seed(0)
    x = ops.as_feat(torch.randn(rows, dims[0], device=dev))
    model = Model(dict(model_name="MLP", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type="batch", device=dev))
    with torch.no_grad():                 # non-trivial eval BatchNorm statistics
        for bn in model.encoder.norms:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    model.eval()
    out32 = torch.empty((rows, dims[-1]), dtype=torch.float32, device=dev)
    out16 = torch.empty_like(out32)

    def fp32_pass():
        with torch.no_grad():
            for s0 in range(0, rows, EVAL_BLOCK_ROWS):
                ops.log_softmax(model.inference(None, x[s0:s0 + EVAL_BLOCK_ROWS]), out=out32[s0:s0 + EVAL_BLOCK_ROWS])

    fns = {}
    if "fp32" in legs:
        fns["fp32"] = fp32_pass
    if "bf16" in legs:
        from glnn_amd import serve
        served = serve.compile_student(model)
        fns["bf16"] = lambda: served.log_probs(x, out=out16)
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):                 # alternating rounds
        for k, fn in fns.items():
            ts[k].append(once(fn))
    flops = sum(2.0 * rows * dims[l] * dims[l + 1] for l in range(len(dims) - 1))
    res = {"rows": rows, "dims": dims, "norm": "batch", "reps": reps, "block_rows": EVAL_BLOCK_ROWS, "GFLOP": round(flops / 1e9, 1)}
    for k in fns:
        ms = median(ts[k])
        res[f"{k}_ms"] = round(ms, 3)
        res[f"{k}_ms_all"] = [round(t, 3) for t in ts[k]]
        res[f"{k}_Mrows_per_s"] = round(rows / ms / 1e3, 2)
        res[f"{k}_TF"] = round(flops / ms / 1e9, 1)
    if "fp32" in fns and "bf16" in fns:
        res["speedup_bf16_over_fp32_in_process"] = round(res["fp32_ms"] / res["bf16_ms"], 3)
        res["max_abs_logp_diff"] = float((out16 - out32).abs().max())
        res["argmax_agree"] = round(float((out16.argmax(1) == out32.argmax(1)).float().mean()), 6)
    if "bf16" in fns:                     # per-launch times: device events around every launch, summed per layer over the row blocks
        coll = []
        ops.set_timing(coll)
        m_done = 0
        with torch.no_grad():
            for s0 in range(0, rows, EVAL_BLOCK_ROWS):
                h = x[s0:s0 + EVAL_BLOCK_ROWS]
                for l in range(len(dims) - 1):
                    last = l == len(dims) - 2
                    h = ops.gemm_bf16(h, served.weights[l], ep_scale=served.scales[l], ep_shift=served.shifts[l], relu=not last,
                                      out_dtype=torch.float32 if last else torch.bfloat16, log_softmax=last)
                m_done += h.shape[0]
        torch.cuda.synchronize()
        ops.set_timing(None)
        per = {}
        for nm, info, s, e in coll:
            key = f"{info['k']}->{info['n']}"
            per.setdefault(key, [0.0, 0.0])
            per[key][0] += s.elapsed_time(e)
            per[key][1] += 2.0 * info["m"] * info["k"] * info["n"]
        res["bf16_launches"] = [{"layer": k, "ms": round(v[0], 3), "TF": round(v[1] / v[0] / 1e9, 1)} for k, v in per.items()]
        if name == "products":
            res["teacher_forward_fp32_ms"] = list(TEACHER_FORWARD_MS)
            res["student_bf16_over_teacher_fp32"] = round(res["bf16_ms"] / TEACHER_FORWARD_MS[0], 3)
    del x, model, out32, out16
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="products,arxiv")
    ap.add_argument("--legs", default="fp32,bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    legs = [s for s in args.legs.split(",") if s]
    res = {"what": "MLP student serving pass (evaluate_mini_batch-equivalent), fp32 path vs bf16 serving path (glnn_amd.serve)", "legs": legs}
    for name in [s for s in args.shapes.split(",") if s]:
        res[name] = run_shape(name, max(1, args.reps), legs, dev)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
