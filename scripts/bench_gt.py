"""Graph-transformer attention timings (csrc/gt.hip) next to the GATv2 attention launches (csrc/gatv2.hip) at the SAME shapes -- the
arxiv- and products-shaped synthetic graphs, 8 heads x 32 features (256 columns) -- in the same process, in alternating rounds.  One JSON
line.

    python scripts/bench_gt.py [--rounds 5] [--graphs ogbn-arxiv,ogbn-products] [--out profiles/gt_bench.json]

A round times one call each of: GATv2 forward, graph-transformer forward, GATv2 backward, graph-transformer backward (training form:
attention dropout 0.3, the row log-sum-exp stored), so drift of the device hits both alike; medians over the rounds behind 2 warm-up
rounds.  Each backward call is that model's launches together (GATv2: two row passes and the dattn fold; graph transformer: two row
passes).  `ratio_fwd` / `ratio_bwd` = graph-transformer median over GATv2 median.  The graph transformer's forward gathers two rows per
edge (k[j] and v[j]) where GATv2's gathers one, its destination pass four per edge where GATv2's gathers two."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops          # noqa: E402

H, F = 8, 32


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def stats(ts):
    ts = sorted(ts)
    return {"med": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def bench_graph(name, rounds, dev):
    g = data.make_graph(name, seed=0, device=dev)
    n, nnz, hf = g.n_dst, g.num_edges(), H * F
    g.transposed_eids()

    def rows():
        t = ops.feat_empty(n, hf, dev)
        t.copy_(torch.randn(n, hf, device=dev) * 0.3)
        return t

    q, k, v, skip, gy = rows(), rows(), rows(), rows(), rows()
    at = torch.randn(1, H, F, device=dev) * 0.3
    out1, out2 = ops.feat_empty(n, hf, dev), ops.feat_empty(n, hf, dev)
    dbuf = [ops.feat_empty(n, hf, dev) for _ in range(5)]
    _, lse1 = ops.gatv2_attn_fwd(g.indptr, g.indices, nnz, k, q, at, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True)
    _, lse2 = ops.gt_attn_fwd(g.indptr, g.indices, nnz, q, k, v, skip, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True)
    calls = {
        "gatv2_fwd": lambda: ops.gatv2_attn_fwd(g.indptr, g.indices, nnz, k, q, at, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True,
                                                out=out1),
        "gt_fwd": lambda: ops.gt_attn_fwd(g.indptr, g.indices, nnz, q, k, v, skip, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True,
                                          out=out2),
        "gatv2_bwd": lambda: ops.gatv2_attn_bwd(g, k, q, lse1, at, gy, H, F, attn_drop=0.3, seed=7, dzl=dbuf[0], dzr=dbuf[1]),
        "gt_bwd": lambda: ops.gt_attn_bwd(g, q, k, v, lse2, gy, H, F, attn_drop=0.3, seed=7, dq=dbuf[2], dk=dbuf[3], dv=dbuf[4]),
    }
    ts = {key: [] for key in calls}
    for r in range(rounds + 2):
        for key, fn in calls.items():
            t = once(fn)
            if r >= 2:
                ts[key].append(t)
    res = {"n": n, "nnz": nnz, "heads": H, "out_feats": F}
    res.update({key: stats(val) for key, val in ts.items()})
    res["ratio_fwd"] = round(res["gt_fwd"]["med"] / res["gatv2_fwd"]["med"], 3)
    res["ratio_bwd"] = round(res["gt_bwd"]["med"] / res["gatv2_bwd"]["med"], 3)
    res["gt_fwd_gather_TBps"] = round(nnz * (8 * hf + 4) / (res["gt_fwd"]["med"] * 1e-3) / 1e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"rounds": args.rounds}
    for name in args.graphs.split(","):
        res[name + "-shaped"] = bench_graph(name, args.rounds, dev)
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
