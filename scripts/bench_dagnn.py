"""DAGNN propagation timings (csrc/dagnn.hip + the aggregation kernel) next to the GPR-GNN teacher's (csrc/gpr.hip): the K = 10 forward
(eval and training form) and backward, on the arxiv-shaped and the products-shaped synthetic graphs at C = 40 and C = 47.  Both teachers
run in the same process in alternating rounds; every figure is the median of --rounds (7) rounds.  One JSON line.

    python scripts/bench_dagnn.py [--rounds 7] [--graphs ogbn-arxiv,ogbn-products] [--out profiles/dagnn_bench.json]

What a DAGNN hop adds to a GPR-GNN step, by bytes: GPR-GNN gathers, accumulates and stores in ONE launch; DAGNN's hop is an aggregation
launch (gather + store of the row) and a gate launch that reads the row and the accumulator again and writes the accumulator (12 C bytes a
row more), and its backward reads the saved H_k and the upstream gradient per hop and ends with the fold's second read of the stack.  The
ratios dagnn / gpr are reported, none is gated."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops                                                      # noqa: E402
from glnn_amd.autograd import dagnn_bwd, dagnn_fwd, gpr_bwd, gpr_fwd                # noqa: E402

K = 10


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def alternate(pairs, rounds):
    """pairs: {name: (gpr_fn, dagnn_fn)}.  One warm-up round, then `rounds` rounds of gpr, dagnn, gpr, dagnn, ... per name; every
    measurement repeats its call until the window is about 50 ms (at most 200 times)."""
    out = {}
    for name, (fg, fd) in pairs.items():
        event_ms(fg, 1), event_ms(fd, 1)
        reps = max(1, min(200, int(50.0 / max(event_ms(fg, 1), 1e-3))))
        tg, td = [], []
        for _ in range(rounds):
            tg.append(event_ms(fg, reps))
            td.append(event_ms(fd, reps))
        a, d = median(tg), median(td)
        out[name] = {"gpr_ms": round(a, 4), "dagnn_ms": round(d, 4), "dagnn_over_gpr": round(d / a, 4), "calls_per_measurement": reps,
                     "gpr_min_max_ms": [round(min(tg), 4), round(max(tg), 4)], "dagnn_min_max_ms": [round(min(td), 4), round(max(td), 4)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--widths", default="40,47")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_dagnn.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"K": K, "rounds": args.rounds, "baseline": "GPR-GNN, same process, alternating rounds", "device": torch.cuda.get_device_name(0),
           "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n, nnz = g.n_dst, g.num_edges()
        g.degree_norms(), g.transposed(False)
        entry = {"n": n, "nnz": nnz, "avg_degree": round(nnz / n, 2), "widths": {}}
        for C in (int(c) for c in args.widths.split(",")):
            h0, dy = ops.feat_empty(n, C, dev), ops.feat_empty(n, C, dev)
            h0.copy_(torch.randn(n, C, device=dev))
            dy.copy_(torch.randn(n, C, device=dev))
            gamma = torch.empty(K + 1, device=dev).uniform_(-1, 1)
            w, b = torch.randn(C, device=dev) / C ** 0.5, torch.zeros(1, device=dev)
            kept = dagnn_fwd(g, h0, w, b, K, keep=True)[1]
            entry["widths"][str(C)] = alternate({
                "fwd_eval_k10": (lambda: gpr_fwd(g, h0, gamma, K), lambda: dagnn_fwd(g, h0, w, b, K)),
                "fwd_train_k10": (lambda: gpr_fwd(g, h0, gamma, K), lambda: dagnn_fwd(g, h0, w, b, K, keep=True)),
                "bwd_k10": (lambda: gpr_bwd(g, dy, h0, gamma, K), lambda: dagnn_bwd(g, dy, kept, w, K)),
            }, args.rounds)
            del h0, dy, kept
        res["graphs"][name] = entry
        del g
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
