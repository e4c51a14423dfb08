"""The node2vec pieces of the position features (csrc/node2vec.hip, csrc/deepwalk.hip; docs/POSITION_SEMANTICS.md) at the arxiv-shaped and
products-shaped synthetic graphs: --roots walk roots, walk length --walk_length.
  walks     glnn_random_walk against glnn_node2vec_walk at (p, q) = (1, 1), (0.5, 2) and (4, 0.25);
  pairs     glnn_deepwalk_pairs_from_walks on the same walks without and with the degree^0.75 CDF;
  step      the whole DeepWalk.step with one table (the default path) and with two (context_table=True, everything else default).
Every figure is the median of --rounds rounds in the same process, alternating, min and max beside it: host wall-clock around a
synchronize.  One JSON line; no ratio is gated.

    python scripts/bench_node2vec.py [--rounds 5] [--graphs ogbn-arxiv,ogbn-products] [--roots 4096] [--out profiles/node2vec_bench.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_subgraph import rounds_of                                                # noqa: E402
from glnn_amd import data, ops                                                      # noqa: E402
from glnn_amd.position import DeepWalk, negative_cdf                                # noqa: E402

PQ = ((1.0, 1.0), (0.5, 2.0), (4.0, 0.25))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--walk_length", type=int, default=20)
    ap.add_argument("--context", type=int, default=10)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_node2vec.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    L, c, k, d = args.walk_length, args.context, args.negatives, args.dim
    res = {"rounds": args.rounds, "roots": args.roots, "walk_length": L, "context": c, "negatives": k, "dim": d,
           "device": torch.cuda.get_device_name(0), "timing": "same process, alternating rounds, host wall-clock around a synchronize", "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n = g.n_dst
        torch.manual_seed(0)
        roots = torch.randperm(n)[:args.roots].contiguous()
        roots_dev = roots.to(dev)
        deg = (g.indptr[1:] - g.indptr[:-1])
        entry = {"n": n, "nnz": g.num_edges(), "max_in_degree": int(deg.max())}
        # (both walks start from the CPU roots DeepWalk.fit hands over: the copy to the device is inside both figures)
        fns = {"random_walk": lambda: ops.random_walk(g.indptr, g.indices, roots.to(dev), L, 1)}
        for p, q in PQ:
            fns[f"node2vec_walk_p{p:g}_q{q:g}"] = lambda p=p, q=q: ops.node2vec_walk(g.indptr, g.indices, roots, L, p, q, 1)
        walks = ops.random_walk(g.indptr, g.indices, roots_dev, L, 1)
        cdf = ops.deepwalk_cdf_words(negative_cdf(g.indices.cpu().numpy(), n, 0.75), dev)
        fns["pairs_from_walks_uniform"] = lambda: ops.deepwalk_pairs_from_walks(walks, n, c, k, 2)
        fns["pairs_from_walks_cdf"] = lambda: ops.deepwalk_pairs_from_walks(walks, n, c, k, 2, neg_cdf=cdf)
        one = DeepWalk(g, d, L, c, k, lr=0.01, seed=0)
        two = DeepWalk(g, d, L, c, k, lr=0.01, seed=0, context_table=True)
        fns["step_one_table"] = lambda: one.step(roots, 1, 2)
        fns["step_two_tables"] = lambda: two.step(roots, 1, 2)
        t = rounds_of(fns, args.rounds)
        for p, q in PQ:
            t[f"node2vec_walk_p{p:g}_q{q:g}"]["over_random_walk"] = round(t[f"node2vec_walk_p{p:g}_q{q:g}"]["ms"] / t["random_walk"]["ms"], 3)
        entry["timings"] = t
        print(f"# {name}: {json.dumps(entry)}", file=sys.stderr, flush=True)
        res["graphs"][name] = entry
        del g, one, two, walks, cdf
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
