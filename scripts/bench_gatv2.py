"""GATv2 attention timings (csrc/gatv2.hip) next to the GAT attention launches (csrc/gat.hip) at the SAME shapes -- the arxiv- and
products-shaped synthetic graphs, 8 heads x 32 features (256 columns) -- in the same process, in alternating rounds.  One JSON line.

    python scripts/bench_gatv2.py [--rounds 9] [--graphs ogbn-arxiv,ogbn-products] [--out profiles/gatv2_bench.json]

A round times one call each of: GAT forward, GATv2 forward, GAT backward, GATv2 backward (training form: attention dropout 0.3, the
row log-sum-exp stored), so drift of the device hits both alike; medians over the rounds behind 2 warm-up rounds.  GAT's forward
entry is glnn_gat_attn_fwd_f32 alone (its scores launch is listed beside it); each backward call is that model's launches together.
`ratio_fwd` / `ratio_bwd` = GATv2 median over GAT median (GAT's forward with its scores launch added in `ratio_fwd_with_scores`)."""
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

    zl, zr, gy = rows(), rows(), rows()
    al, ar = torch.randn(1, H, F, device=dev) * 0.3, torch.randn(1, H, F, device=dev) * 0.3
    out1, out2 = ops.feat_empty(n, hf, dev), ops.feat_empty(n, hf, dev)
    el, er = ops.gat_scores(zl, al, ar, H, F)
    y1, lse1 = ops.gat_attn_fwd(g.indptr, g.indices, nnz, zl, el, er, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True)
    y2, lse2 = ops.gatv2_attn_fwd(g.indptr, g.indices, nnz, zl, zr, al, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True)
    calls = {
        "gat_scores": lambda: ops.gat_scores(zl, al, ar, H, F),
        "gat_fwd": lambda: ops.gat_attn_fwd(g.indptr, g.indices, nnz, zl, el, er, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True,
                                            out=out1),
        "gatv2_fwd": lambda: ops.gatv2_attn_fwd(g.indptr, g.indices, nnz, zl, zr, al, H, F, attn_drop=0.3, seed=7, relu=True, want_lse=True,
                                                out=out2),
        "gat_bwd": lambda: ops.gat_attn_bwd(g, zl, el, er, lse1, al, ar, gy, y1, H, F, attn_drop=0.3, seed=7),
        "gatv2_bwd": lambda: ops.gatv2_attn_bwd(g, zl, zr, lse2, al, gy, H, F, attn_drop=0.3, seed=7),
    }
    ts = {k: [] for k in calls}
    for r in range(rounds + 2):
        for k, fn in calls.items():
            t = once(fn)
            if r >= 2:
                ts[k].append(t)
    res = {"n": n, "nnz": nnz, "heads": H, "out_feats": F}
    res.update({k: stats(v) for k, v in ts.items()})
    res["ratio_fwd"] = round(res["gatv2_fwd"]["med"] / res["gat_fwd"]["med"], 3)
    res["ratio_fwd_with_scores"] = round(res["gatv2_fwd"]["med"] / (res["gat_fwd"]["med"] + res["gat_scores"]["med"]), 3)
    res["ratio_bwd"] = round(res["gatv2_bwd"]["med"] / res["gat_bwd"]["med"], 3)
    res["gatv2_fwd_gather_TBps"] = round(nnz * (4 * hf + 4) / (res["gatv2_fwd"]["med"] * 1e-3) / 1e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
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
