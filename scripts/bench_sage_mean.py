"""SAGE "mean" layer A/B on one MI355X: the fused launch (glnn_sage_mean_fused_f32) or, for a layer that projects first, the stacked
projection + glnn_spmm_sage_mean_f32, against the composition of existing ops (aggregation with a row scale + two GEMMs + the sum), and for
context the SAGE-"gcn" form of the same shape (the kept layer-1 aggregate and the chained projection are off: plain ops calls).

One process, alternating rounds (every form once per round, ROUNDS rounds, each timing ITERS back-to-back launches between device
events after a warm-up); the medians and the min..max spread of the rounds are reported.  Decision rule ("SAGE mean"): the
single-launch form is SAGEConv's default for a shape only where its median beats the composition's by more than the composition's own
spread.  Writes profiles/sage_mean_bench_a.json.

  python scripts/bench_sage_mean.py [--graphs ogbn-products,ogbn-arxiv] [--rounds 7] [--iters 3] [--scale 1.0] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glnn_amd import data, ops            # noqa: E402
from glnn_amd.nn import SAGEConv, mean_row_scale      # noqa: E402

LAYERS = {"ogbn-products": [(100, 256), (256, 256), (256, 47)], "ogbn-arxiv": [(128, 256), (256, 256), (256, 40)]}


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bench_layer(g, d_in, d_out, rounds, iters, dev):
    n = g.n_dst
    torch.manual_seed(d_in * 1000 + d_out)
    x = ops.as_feat(torch.randn(n, d_in, device=dev))
    mean, gcn = SAGEConv(d_in, d_out, "mean").to(dev).eval(), SAGEConv(d_in, d_out, "gcn").to(dev).eval()
    sc, sh = torch.rand(d_out, device=dev) + 0.5, torch.randn(d_out, device=dev)
    out = ops.feat_empty(n, d_out, dev)
    single = "fused" if d_in <= d_out else "project"
    order = g.fused_tile_order()
    mean_row_scale(g)
    forms = {
        single: lambda: mean.forward_mean(g, (x, x), ep_scale=sc, ep_shift=sh, relu=True, out=out, form=single),
        "compose": lambda: mean.forward_mean(g, (x, x), ep_scale=sc, ep_shift=sh, relu=True, out=out, form="compose"),
        "gcn": lambda: gcn(g, (x, x), ep_scale=sc, ep_shift=sh, relu=True, out=out),
    }
    with torch.no_grad():
        a = mean.forward_mean(g, (x, x), ep_scale=sc, ep_shift=sh, relu=True, form=single)
        b = mean.forward_mean(g, (x, x), ep_scale=sc, ep_shift=sh, relu=True, form="compose")
        agree = float((a - b).abs().max())
        del a, b
        for fn in forms.values():          # warm-up: code objects, packed weights, the transposed pads
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                ms[k].append(timed(fn, iters))
    rec = {"d_in": d_in, "d_out": d_out, "single_launch_form": single, "tile_order": order is not None, "max_abs_diff_vs_compose": agree}
    for k, v in ms.items():
        rec[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": [round(t, 4) for t in v]}
    spread = rec["compose"]["max_ms"] - rec["compose"]["min_ms"]
    rec["compose_spread_ms"] = spread
    rec["single_launch_wins"] = rec[single]["median_ms"] < rec["compose"]["median_ms"] - spread
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ogbn-products,ogbn-arxiv")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sage_mean_bench_a.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sage_mean.py measures on the GPU only")
    if args.rounds < 7:
        raise SystemExit("--rounds: at least 7 (the decision compares a median against a spread)")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "scale": args.scale, "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        recs = []
        for d_in, d_out in LAYERS[name]:
            rec = bench_layer(g, d_in, d_out, args.rounds, args.iters, dev)
            recs.append(rec)
            s = rec["single_launch_form"]
            print(f"{name} {d_in}->{d_out}: {s} {rec[s]['median_ms']:.3f} ms  compose {rec['compose']['median_ms']:.3f} ms "
                  f"(spread {rec['compose_spread_ms']:.3f})  gcn {rec['gcn']['median_ms']:.3f} ms  wins={rec['single_launch_wins']}", flush=True)
        result["graphs"][name] = {"n": g.n_dst, "nnz": g.num_edges(), "layers": recs}
        del g
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
