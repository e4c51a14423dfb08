"""SAGE "mean" teacher TRAINING step A/B on one MI355X: ms per batch of train_sage through (a) mean_step="autograd" (the differentiable
ops + torch's loss and optimiser: the path before the native step existed) and (b) mean_step="native" (TeacherEngine.step_sage_mean, one C
call per batch), with the "gcn" one-call step on the same loader beside them as a yardstick.

Same graph, node data, loader settings and seed, and the same initial model per aggregator; an epoch is STEPS full batches, sampling
included (as train_sage runs it: blocks built one batch ahead on a side stream).  One process; after a warm-up epoch of every path the
paths are timed in rounds, the order a, b, gcn in even rounds and gcn, b, a in odd ones; medians and the min..max spread of the rounds
are reported.  The bar (docs/SAGE_MEAN_SEMANTICS.md): (b) is faster than (a) by more than (a)'s own spread, on both configurations.

  python scripts/bench_sage_mean_step.py [--configs ogbn-products,ogbn-arxiv] [--rounds 6] [--steps 24] [--out PATH]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glnn_amd import data, train_and_eval as te                        # noqa: E402
from glnn_amd.graph import MultiLayerNeighborSampler, NodeDataLoader   # noqa: E402
from glnn_amd.models import Model                                      # noqa: E402

# the reference's SAGE sections (train.conf.yaml: products B=4096 dropout 0.5 lr 0.003; arxiv B=512 dropout 0.2 lr 0.01), fan-out 5,10,15
CFG = {"ogbn-products": dict(f=100, c=47, B=4096, p=0.5, lr=0.003), "ogbn-arxiv": dict(f=128, c=40, B=512, p=0.2, lr=0.01)}
PATHS = [("mean/autograd", "mean", "autograd"), ("mean/native", "mean", "native"), ("gcn/one-call", "gcn", "autograd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="ogbn-products,ogbn-arxiv")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sage_mean_step_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sage_mean_step.py measures on the GPU only")
    dev = "cuda:0"
    lines = [f"device {torch.cuda.get_device_name(0)}  rounds {args.rounds}  steps/epoch {args.steps}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    for name in args.configs.split(","):
        c = CFG[name]
        g = data.make_graph(name, seed=0, device=dev)
        feats, labels, _, _ = data.make_node_data(name, seed=0, device=dev, n=g.n_dst)
        torch.manual_seed(0)
        idx = torch.randperm(g.n_dst)[:c["B"] * args.steps].to(dev)
        crit = torch.nn.NLLLoss()
        runs = {}
        for tag, agg, step in PATHS:
            torch.manual_seed(0)
            model = Model(dict(model_name="SAGE", num_layers=3, feat_dim=c["f"], hidden_dim=256, label_dim=c["c"], dropout_ratio=c["p"],
                               norm_type="batch", device=dev, sage_aggregator=agg))
            opt = torch.optim.Adam(model.parameters(), lr=c["lr"])
            loader = NodeDataLoader(g, idx, MultiLayerNeighborSampler([5, 10, 15]), batch_size=c["B"], shuffle=True, drop_last=False, seed=0)
            runs[tag] = (model, opt, loader, step)

        def epoch(tag):
            model, opt, loader, step = runs[tag]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = te.train_sage(model, loader, feats, labels, crit, opt, mean_step=step)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / len(loader), loss

        for tag, _, _ in PATHS:          # warm-up: code objects, arenas, autograd's caches
            epoch(tag)
        ms = {tag: [] for tag, _, _ in PATHS}
        for r in range(args.rounds):
            order = PATHS if r % 2 == 0 else PATHS[::-1]
            for tag, _, _ in order:
                t, loss = epoch(tag)
                ms[tag].append(t)
                say(f"{name} round {r} {tag}: {t:.3f} ms/step  loss {loss:.4f}")
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            say(f"{name} {k}: median {med[k]:.3f} ms/step  min {min(v):.3f}  max {max(v):.3f}  ({1e3 / med[k]:.1f} steps/s)")
        spread = max(ms["mean/autograd"]) - min(ms["mean/autograd"])
        wins = med["mean/native"] < med["mean/autograd"] - spread
        ok = ok and wins
        say(f"{name}: native / autograd = {med['mean/native'] / med['mean/autograd']:.3f}  (autograd spread {spread:.3f} ms)  "
            f"native / gcn one-call = {med['mean/native'] / med['gcn/one-call']:.3f}  native faster beyond the spread: {wins}")
        del g, feats, labels, runs
        torch.cuda.empty_cache()
    say(f"bar met on every configuration: {ok}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
