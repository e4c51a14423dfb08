"""GPR-GNN propagation timings (csrc/gpr.hip) next to the APPNP teacher's (csrc/appnp.hip, edge_drop 0): the K = 10 forward and backward
propagation and one full training step, on the arxiv-shaped and the products-shaped synthetic graphs at C = 40 and C = 47.  Both forms run
in the same process in alternating rounds; every figure is the median of --rounds (7) rounds.  One JSON line.

    python scripts/bench_gpr.py [--rounds 7] [--graphs ogbn-arxiv,ogbn-products] [--out profiles/gpr_bench_a.json]

What the GPR launch adds to an APPNP launch, by bytes: one read and one write of the accumulator row (8 C bytes per row) beside a gather
of nnz * 4 C bytes, minus APPNP's teleport-row read in the forward; the backward also writes one float per row (row_dot) and ends with
the fold.  The ratios gpr / appnp are reported, none is gated."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops, train_and_eval as te                                # noqa: E402
from glnn_amd.autograd import appnp_bwd, appnp_fwd, gpr_bwd, gpr_fwd                # noqa: E402
from glnn_amd.models import Model                                                   # noqa: E402

K, ALPHA = 10, 0.1


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


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


def alternate(pairs, rounds, measure):
    """pairs: {name: (appnp_fn, gpr_fn)}.  One warm-up round, then `rounds` rounds of appnp, gpr, appnp, gpr, ... per name; every
    measurement repeats its call until the window is about 50 ms (at most 200 times)."""
    out = {}
    for name, (fa, fg) in pairs.items():
        measure(fa, 1), measure(fg, 1)
        reps = max(1, min(200, int(50.0 / max(measure(fa, 1), 1e-3))))
        ta, tg = [], []
        for _ in range(rounds):
            ta.append(measure(fa, reps))
            tg.append(measure(fg, reps))
        a, g = median(ta), median(tg)
        out[name] = {"appnp_ms": round(a, 4), "gpr_ms": round(g, 4), "gpr_over_appnp": round(g / a, 4), "calls_per_measurement": reps,
                     "appnp_min_max_ms": [round(min(ta), 4), round(max(ta), 4)], "gpr_min_max_ms": [round(min(tg), 4), round(max(tg), 4)]}
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
        raise RuntimeError("bench_gpr.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"K": K, "alpha": ALPHA, "rounds": args.rounds, "baseline": "APPNP (edge_drop 0), same process, alternating rounds",
           "device": torch.cuda.get_device_name(0), "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n, nnz = g.n_dst, g.num_edges()
        g.degree_norms(), g.transposed(False), g.transposed_eids()
        feats, labels, _, _ = data.make_node_data(name, seed=0, device=dev, n=n)
        idx_train = torch.randperm(n)[:max(8, n // 10)].to(dev)
        entry = {"n": n, "nnz": nnz, "avg_degree": round(nnz / n, 2), "widths": {}}
        for C in (int(c) for c in args.widths.split(",")):
            h0, dy = ops.feat_empty(n, C, dev), ops.feat_empty(n, C, dev)
            h0.copy_(torch.randn(n, C, device=dev))
            dy.copy_(torch.randn(n, C, device=dev))
            gamma = torch.empty(K + 1, device=dev).uniform_(-1, 1)
            timings = alternate({
                "fwd_k10": (lambda: appnp_fwd(g, h0, K, ALPHA, 0.0, 0), lambda: gpr_fwd(g, h0, gamma, K)),
                "bwd_k10": (lambda: appnp_bwd(g, dy, K, ALPHA, 0.0, 0), lambda: gpr_bwd(g, dy, h0, gamma, K)),
            }, args.rounds, event_ms)
            del h0, dy
            # the full training step (cora's APPNP section of train.conf.yaml: hidden 128, dropout 0.5, weight decay 0.01), C classes
            steps = {}
            for kind in ("APPNP", "GPRGNN"):
                m = Model(dict(model_name=kind, num_layers=2, feat_dim=feats.shape[1], hidden_dim=128, label_dim=C, dropout_ratio=0.5,
                               norm_type="none", device=dev, gpr_k=K, gpr_alpha=ALPHA))
                if kind == "APPNP":
                    m.encoder.edge_drop = 0.0
                opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=0.01)
                lab = labels % C
                steps[kind] = (lambda m=m, opt=opt, lab=lab: te.train(m, g, feats, lab, torch.nn.NLLLoss(), opt, idx_train))
            timings.update(alternate({"train_step": (steps["APPNP"], steps["GPRGNN"])}, args.rounds, host_ms))
            del steps
            entry["widths"][str(C)] = timings
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
