"""GAT attention timings (csrc/gat.hip), launch by launch, on the arxiv- and products-shaped synthetic graphs at the reference's GAT
dims (8 heads x 16 features hidden, 1 head x C output), next to the stand-alone aggregation ops.spmm(..., AGG_SUM) at 128 columns on
the same graph in the same process -- the call that moves the same gathered bytes without the softmax.  One JSON line.

    python scripts/bench_gat.py [--reps 10] [--graphs ogbn-arxiv,ogbn-products] [--out profiles/gat_bench.json]

Per entry: median / min / max milliseconds over `reps` timed calls behind 3 warm-up calls.  `value_vs_spmm` = the hidden layer's eval
attention forward over the plain gather.  The training entries use attention dropout 0.3 and feature dropout 0.6; the backward call is
its four launches together (destination pass, source pass, dattn partials, fold) and keeps one [E, H] fp32 scratch."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops          # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return {"med": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def bench_graph(name, reps, dev):
    g = data.make_graph(name, seed=0, device=dev)
    n, nnz = g.n_dst, g.num_edges()
    d_in, C = {"ogbn-arxiv": (128, 40), "ogbn-products": (100, 47)}[name]
    res = {"n": n, "nnz": nnz, "d_in": d_in, "C": C, "ds_scratch_GB": round(nnz * 8 * 4 / 2 ** 30, 2)}
    g.transposed_eids()
    x = ops.feat_empty(n, d_in, dev)
    x.copy_(torch.randn(n, d_in, device=dev))
    for tag, H, F, k, relu in (("hidden", 8, 16, d_in, True), ("output", 1, C, 128, False)):
        w = torch.randn(H * F, k, device=dev) * 0.1
        al, ar = torch.randn(1, H, F, device=dev), torch.randn(1, H, F, device=dev)
        xin = x if k == d_in else torch.relu(torch.randn(n, k, device=dev))
        gy = ops.feat_empty(n, H * F, dev)
        gy.copy_(torch.randn(n, H * F, device=dev))
        r = {}
        r["project"] = timed(lambda: ops.gemm(xin, w), reps)
        r["project_drop"] = timed(lambda: ops.gat_project(xin, w, 0.6, 5, signed=False), reps)
        z = ops.gemm(xin, w)
        r["scores"] = timed(lambda: ops.gat_scores(z, al, ar, H, F), reps)
        el, er = ops.gat_scores(z, al, ar, H, F)
        out = ops.feat_empty(n, H * F, dev)
        r["attn_fwd_eval"] = timed(lambda: ops.gat_attn_fwd(g.indptr, g.indices, nnz, z, el, er, H, F, relu=relu, out=out), reps)
        r["attn_fwd_train"] = timed(lambda: ops.gat_attn_fwd(g.indptr, g.indices, nnz, z, el, er, H, F, attn_drop=0.3, seed=7, relu=relu,
                                                             want_lse=True, out=out), reps)
        y, lse = ops.gat_attn_fwd(g.indptr, g.indices, nnz, z, el, er, H, F, attn_drop=0.3, seed=7, relu=relu, want_lse=True)
        r["attn_bwd"] = timed(lambda: ops.gat_attn_bwd(g, z, el, er, lse, al, ar, gy, y, H, F, attn_drop=0.3, seed=7), reps)
        dz = ops.gat_attn_bwd(g, z, el, er, lse, al, ar, gy, y, H, F, attn_drop=0.3, seed=7)[0]
        r["wgrad_drop"] = timed(lambda: ops.gat_project_wgrad(dz, xin, 0.6, 5, signed=False), reps)
        r["dgrad"] = timed(lambda: ops.gemm(dz, w, w_is_kn=True), reps)
        if tag == "hidden":
            r["spmm_sum_128"] = timed(lambda: ops.spmm(g.indptr, g.indices, z, n, ops.AGG_SUM, out=out), reps)
            r["value_vs_spmm"] = round(r["attn_fwd_eval"]["med"] / r["spmm_sum_128"]["med"], 3)
            r["gather_TBps_eval"] = round((nnz * (4 * H * F + 4 + 4 * H * 3)) / (r["attn_fwd_eval"]["med"] * 1e-3) / 1e12, 3)
        r["eval_forward_ms"] = round(r["project"]["med"] + r["scores"]["med"] + r["attn_fwd_eval"]["med"], 4)
        r["train_layer_ms"] = round(r["project_drop"]["med"] + r["scores"]["med"] + r["attn_fwd_train"]["med"] + r["attn_bwd"]["med"]
                                    + r["wgrad_drop"]["med"] + r["dgrad"]["med"], 4)
        res[tag] = r
        del z, el, er, out, y, lse, dz, gy
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"reps": args.reps}
    for name in args.graphs.split(","):
        res[name + "-shaped"] = bench_graph(name, args.reps, dev)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
