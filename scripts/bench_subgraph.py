"""Random-walk subgraph training (csrc/subgraph.hip, docs/SUBGRAPH_SEMANTICS.md) at the arxiv-shaped and products-shaped synthetic graphs:
  builder      ops.induced_subgraph (its capacity read and its counts read included) next to CSRGraph.subgraph -- the N- and E-sized torch
               composition this package has always had, unchanged by the native builder -- on the SAME node sets: the nodes visited by
               --roots walks of --walk_length steps.  Both are checked to give the same arrays first.
  sampler      ops.random_walk alone.
  step         seconds per batch of train_and_eval.train_subgraph (walk, builder, row gather and the engine step) for a GCN and a GAT
               teacher, next to ONE full-graph train() step of the same model.  A batch is not an epoch: the full-graph step sees every
               training node once, a batch --roots of them; the script reports both times and the number of batches per epoch.
Every figure is the median of --rounds rounds in the same process, alternating, min and max beside it.  Host wall-clock around a
synchronize (all three forms read back from the device).  One JSON line; no ratio is gated.

    python scripts/bench_subgraph.py [--rounds 7] [--graphs ogbn-arxiv,ogbn-products] [--roots 1024] [--walk_length 3] [--out profiles/subgraph_bench_a.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops, train_and_eval as te                                # noqa: E402
from glnn_amd.graph import RandomWalkSubgraphLoader                                  # noqa: E402
from glnn_amd.models import Model                                                   # noqa: E402


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def rounds_of(fns, rounds, reps=None):
    """fns: {name: fn}, measured in alternating rounds after one warm-up call each; a measurement repeats its call until the window is about
    50 ms (at most 100 times) unless `reps` says otherwise.  {name: {ms (median), min_max_ms, calls_per_measurement}}."""
    first = {name: host_ms(fn, 1) for name, fn in fns.items()}
    t = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            r = reps or max(1, min(100, int(50.0 / max(first[name], 1e-3))))
            t[name].append(host_ms(fn, r))
    return {name: {"ms": round(median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--roots", type=int, default=1024)
    ap.add_argument("--walk_length", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8, help="batches per timed train_subgraph call")
    ap.add_argument("--teachers", default="GCN,GAT")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_subgraph.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"rounds": args.rounds, "roots": args.roots, "walk_length": args.walk_length, "device": torch.cuda.get_device_name(0),
           "baseline": "CSRGraph.subgraph (N-sized remap, E-sized expansion and mask, argsort) on the same node sets; one full-graph "
                       "train() step of the same model; same process, alternating rounds, host wall-clock", "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n, nnz = g.n_dst, g.num_edges()
        feats, labels, _, _ = data.make_node_data(name, seed=0, device=dev, n=n)
        idx_train = torch.randperm(n)[:max(args.roots * args.batches, n // 10)].to(dev)
        roots = idx_train[:args.roots].contiguous()
        entry = {"n": n, "nnz": nnz, "avg_degree": round(nnz / n, 2), "train_nodes": int(idx_train.numel()),
                 "batches_per_epoch": -(-int(idx_train.numel()) // args.roots)}

        walks = ops.random_walk(g.indptr, g.indices, roots, args.walk_length, 1)
        cand = walks.reshape(-1)
        nodes, sip, six, n_sub, sub_nnz, zero = ops.induced_subgraph(g.indptr, g.indices, cand)
        ref = g.subgraph(nodes)
        same = bool(torch.equal(ref.indptr, sip) and torch.equal(ref.indices, six))
        entry["node_set"] = {"candidates": int(cand.numel()), "n_sub": n_sub, "nnz": sub_nnz, "rows_without_entry": zero,
                             "equal_to_csrgraph_subgraph": same}
        t = rounds_of({"random_walk": lambda: ops.random_walk(g.indptr, g.indices, roots, args.walk_length, 1),
                       "native": lambda: ops.induced_subgraph(g.indptr, g.indices, cand),
                       "csrgraph_subgraph": lambda: g.subgraph(nodes)}, args.rounds)
        t["native_over_csrgraph_subgraph"] = round(t["native"]["ms"] / t["csrgraph_subgraph"]["ms"], 5)
        entry["builder"] = t
        print(f"# {name} builder: {json.dumps(entry['node_set'])} {json.dumps(t)}", file=sys.stderr, flush=True)
        del ref, walks
        torch.cuda.empty_cache()

        entry["step"] = {}
        for teacher_name in args.teachers.split(","):
            conf = dict(model_name=teacher_name, num_layers=2, feat_dim=feats.shape[1], hidden_dim=128, label_dim=int(labels.max()) + 1,
                        dropout_ratio=0.5, norm_type="none", device=dev, num_heads=4, attn_dropout_ratio=0.3)
            crit = torch.nn.NLLLoss()
            m_sub, m_full = Model(conf), Model(conf)
            o_sub = torch.optim.Adam(m_sub.parameters(), lr=0.01, weight_decay=0.0005)
            o_full = torch.optim.Adam(m_full.parameters(), lr=0.01, weight_decay=0.0005)
            loader = RandomWalkSubgraphLoader(g, idx_train[:args.roots * args.batches], args.roots, args.walk_length, self_loop="add", seed=0)
            assert len(loader) == args.batches
            t = rounds_of({"train_subgraph_call": lambda: te.train_subgraph(m_sub, loader, feats, labels, crit, o_sub),
                           "full_graph_step": lambda: te.train(m_full, g, feats, labels, crit, o_full, idx_train)}, args.rounds, reps=1)
            per_batch = t["train_subgraph_call"]["ms"] / args.batches
            entry["step"][teacher_name] = {"train_subgraph_ms_per_batch": round(per_batch, 4), "train_subgraph_call": t["train_subgraph_call"],
                                           "batches_per_call": args.batches, "full_graph_step": t["full_graph_step"],
                                           "batch_over_full_graph_step": round(per_batch / t["full_graph_step"]["ms"], 5),
                                           "epoch_of_batches_over_full_graph_step":
                                               round(per_batch * entry["batches_per_epoch"] / t["full_graph_step"]["ms"], 4)}
            print(f"# {name} {teacher_name}: {json.dumps(entry['step'][teacher_name])}", file=sys.stderr, flush=True)
            del m_sub, m_full, o_sub, o_full, loader
            torch.cuda.empty_cache()
        res["graphs"][name] = entry
        del g, feats, labels
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
