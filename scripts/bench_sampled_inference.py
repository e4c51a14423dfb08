"""Neighbour-sampled SAGE teacher inference against the full-neighbour forward on one MI355X (docs/SAMPLED_INFERENCE_SEMANTICS.md): the
3-layer BatchNorm SAGE-"gcn" teacher of bench.py's shapes (products: 100 -> 256 -> 256 -> 47, arxiv: 128 -> 256 -> 256 -> 40) over the
synthetic products- and arxiv-shaped graphs, with fan-outs 5, 10, 15, 25 per layer and with every in-edge.

One process, alternating rounds (every configuration once per round, ROUNDS rounds, each timing ITERS back-to-back forwards between device
events after a warm-up); medians and the min..max spread of the rounds are reported.  Per configuration:
  forward_ms       SAGE.inference(fan_out=[f] * 3): the three fill launches + the three layers (the sampled indptr is cached per fan-out);
  fill_ms          the three fill launches alone (CSRGraph.sampled);
  edges            the sampled edge count per layer, sum of min(in-degree, f);
  argmax_agree     the share of rows whose arg-max class equals the full forward's (an UNTRAINED teacher over the synthetic features: what
                   moves is how far sampling perturbs the logits, not an accuracy); label_match: arg-max == the synthetic (uniform) label.
"full" is SAGE.inference() in steady state (its kept layer-1 aggregate and placed buffers in use); "full_plain" the same layers through
SAGE.inference_over([g] * 3), i.e. with the plain allocations and no kept aggregate -- the state the sampled path runs in.
Writes profiles/sampled_inference_bench_a.json.

  python scripts/bench_sampled_inference.py [--graphs ogbn-products,ogbn-arxiv] [--rounds 5] [--iters 3] [--scale 1.0] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glnn_amd import data            # noqa: E402
from glnn_amd.graph import FullNeighborLoader      # noqa: E402
from glnn_amd.models import Model      # noqa: E402

FANOUTS = (5, 10, 15, 25)
SAMPLE_SEED = 0


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": [round(t, 4) for t in v]}


def bench_graph(name, rounds, iters, scale, dev):
    g = data.make_graph(name, seed=0, device=dev, scale=scale)
    feats, labels, _, _ = data.make_node_data(name, seed=0, device=dev, n=g.n_dst)
    sh = data.SHAPES[name]
    torch.manual_seed(0)
    model = Model(dict(model_name="SAGE", num_layers=3, feat_dim=sh["f"], hidden_dim=256, label_dim=sh["c"], dropout_ratio=0.5,
                       norm_type="batch", device=dev)).eval()
    enc = model.encoder
    loader = FullNeighborLoader(g, 4096)
    L = enc.num_layers
    forms = {"full": lambda: model.inference(loader, feats), "full_plain": lambda: enc.inference_over([g] * L, feats)}
    fills = {}
    for f in FANOUTS:
        forms[f"fanout_{f}"] = (lambda f=f: model.inference(loader, feats, fan_out=[f] * L, sample_seed=SAMPLE_SEED))
        fills[f"fanout_{f}"] = (lambda f=f: enc.sampled_graphs(g, [f] * L, SAMPLE_SEED))
    with torch.no_grad():
        for fn in list(forms.values()) + list(fills.values()):          # warm-up: code objects, placement, the cached sampled indptrs
            fn()
            fn()
        torch.cuda.synchronize()
        full_arg = model.inference(loader, feats).argmax(1)
        quality, edges = {}, {}
        for k, fn in forms.items():
            arg = fn().argmax(1)
            quality[k] = {"argmax_agree": float((arg == full_arg).float().mean()), "label_match": float((arg == labels).float().mean())}
        for f in FANOUTS:
            edges[f"fanout_{f}"] = [s.num_edges() for s in enc.sampled_graphs(g, [f] * L, SAMPLE_SEED)]
        ms, fill_ms = {k: [] for k in forms}, {k: [] for k in fills}
        for _ in range(rounds):
            for k, fn in forms.items():
                ms[k].append(timed(fn, iters))
            for k, fn in fills.items():
                fill_ms[k].append(timed(fn, iters))
    rec = {"n": g.n_dst, "nnz": g.num_edges(), "max_in_degree": int(g.in_degrees().max().item()), "configs": {}}
    for k in forms:
        rec["configs"][k] = {"forward": stats(ms[k]), **quality[k]}
        if k in fills:
            rec["configs"][k].update(fill=stats(fill_ms[k]), edges=edges[k])
        else:
            rec["configs"][k].update(edges=[g.num_edges()] * L)
    for k, c in rec["configs"].items():
        fill = f"  fill {c['fill']['median_ms']:.3f} ms" if "fill" in c else ""
        print(f"{name} {k}: forward {c['forward']['median_ms']:.3f} ms ({c['forward']['min_ms']:.3f}..{c['forward']['max_ms']:.3f}){fill}  "
              f"edges {c['edges']}  argmax_agree {c['argmax_agree']:.4f}", flush=True)
    enc.release_placed()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ogbn-products,ogbn-arxiv")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_inference_bench_a.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampled_inference.py measures on the GPU only")
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5 (medians of rounds are reported)")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "scale": args.scale,
              "fanouts": list(FANOUTS), "sample_seed": SAMPLE_SEED, "graphs": {}}
    for name in args.graphs.split(","):
        result["graphs"][name] = bench_graph(name, args.rounds, args.iters, args.scale, dev)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
