"""GCNII layer timings (csrc/gcnii.hip): ONE fused forward layer next to two compositions from existing launches, then the L = 8 eval
forward and one full training step, at hidden = 64 and 256 on the arxiv-shaped and the products-shaped synthetic graphs.
  composed         ops.appnp_propagate (edge_drop 0), ops.gemm with beta in its epilogue scale, and the elementwise combine done here in
                   torch as TWO launches (add_: reads both, writes one; relu_: reads one, writes one) -- torch has no single launch for
                   relu(a + k b), so this form carries 2 passes of N * hidden * 4 bytes more than the byte estimate below assumes;
  composed_folded  ops.appnp_propagate, then ONE ops.gemm against W' = (1 - beta) I + beta W with the ReLU in its epilogue: the identity
                   mapping folded into the weight, no combine launch at all (2 passes FEWER than the estimate's composition).
The estimate's composition (a one-launch combine) lies between the two.  All forms of the layer run in the same process in alternating
rounds; every figure is the median of --rounds (7) rounds, min and max beside it.  One JSON line.

    python scripts/bench_gcnii.py [--rounds 7] [--graphs ogbn-arxiv,ogbn-products] [--widths 64,256] [--out profiles/gcnii_bench_a.json]

Expectation from byte counts only: the composition moves about four more passes of N * hidden * 4 bytes per layer (it writes S, reads S,
writes the product, reads both) beside a gather of deg * N * hidden * 4 bytes: the fused launch about 20 % cheaper at degree 14, about
7 % at degree 50.  The ratio fused / composed is reported, none is gated; the package has no second path."""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops, train_and_eval as te                                # noqa: E402
from glnn_amd.models import Model                                                   # noqa: E402

L, ALPHA, LAMDA = 8, 0.1, 0.5


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


def rounds_of(fns, rounds, measure):
    """fns: {name: fn}, measured in alternating rounds (a, b, a, b, ...) after one warm-up call each; every measurement repeats its call
    until the window is about 50 ms (at most 200 times).  {name: {ms (median), min_max_ms, calls_per_measurement}}."""
    for fn in fns.values():
        measure(fn, 1)
    reps = max(1, min(200, int(50.0 / max(measure(next(iter(fns.values())), 1), 1e-3))))
    t = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            t[name].append(measure(fn, reps))
    return {name: {"ms": round(median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)], "calls_per_measurement": reps}
            for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_gcnii.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"L": L, "alpha": ALPHA, "lamda": LAMDA, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "baseline": "composed: appnp_propagate (edge_drop 0) + gemm (beta in the epilogue) + add_ + relu_ in torch; composed_folded: "
                       "appnp_propagate + one gemm against (1 - beta) I + beta W with ReLU; same process, alternating rounds", "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n, nnz = g.n_dst, g.num_edges()
        in_norm, out_norm = g.degree_norms()
        g.transposed(False)
        feats, labels, _, _ = data.make_node_data(name, seed=0, device=dev, n=n)
        idx_train = torch.randperm(n)[:max(8, n // 10)].to(dev)
        entry = {"n": n, "nnz": nnz, "avg_degree": round(nnz / n, 2), "widths": {}}
        for d in (int(c) for c in args.widths.split(",")):
            x, h0 = ops.feat_empty(n, d, dev), ops.feat_empty(n, d, dev)
            x.copy_(torch.randn(n, d, device=dev).relu_())
            h0.copy_(torch.randn(n, d, device=dev).relu_())
            w = torch.empty(d, d, device=dev).uniform_(-1, 1) / math.sqrt(d)
            beta = math.log(LAMDA / 1 + 1)
            out_f, s_c, z_c = (ops.feat_empty(n, d, dev) for _ in range(3))
            beta_vec = torch.full((d,), beta, device=dev)
            w_folded = ((1.0 - beta) * torch.eye(d, device=dev) + beta * w).contiguous()

            def fused():
                return ops.gcnii_layer(g.indptr, g.indices, nnz, x, h0, w, ALPHA, beta, in_norm, x_norm=out_norm, out=out_f)

            def composed():
                s = ops.appnp_propagate(g.indptr, g.indices, x, nnz, 1, in_norm, out_norm, h0, ALPHA, x_scaled=False, last=True, out=s_c)
                z = ops.gemm(s, w, ep_scale=beta_vec, out=z_c)                        # beta S W^T
                return torch.relu_(z.add_(s, alpha=1.0 - beta))

            def composed_folded():
                s = ops.appnp_propagate(g.indptr, g.indices, x, nnz, 1, in_norm, out_norm, h0, ALPHA, x_scaled=False, last=True, out=s_c)
                return ops.gemm(s, w_folded, relu=True, out=z_c)

            err = max(float((fused() - composed()).abs().max()), float((fused() - composed_folded()).abs().max()))
            t = rounds_of({"composed": composed, "composed_folded": composed_folded, "fused": fused}, args.rounds, event_ms)
            timings = {"layer_fwd": {"composed": t["composed"], "composed_folded": t["composed_folded"], "fused": t["fused"],
                                     "fused_over_composed": round(t["fused"]["ms"] / t["composed"]["ms"], 4),
                                     "fused_over_composed_folded": round(t["fused"]["ms"] / t["composed_folded"]["ms"], 4),
                                     "max_abs_diff": err}}
            del x, h0, out_f, s_c, z_c, beta_vec, w_folded
            m = Model(dict(model_name="GCNII", num_layers=L, feat_dim=feats.shape[1], hidden_dim=d, label_dim=int(labels.max()) + 1,
                           dropout_ratio=0.5, norm_type="none", device=dev, gcnii_alpha=ALPHA, gcnii_lamda=LAMDA))
            opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=0.0005)
            m.eval()
            timings["forward_l8_eval"] = rounds_of({"gcnii": lambda: m(g, feats)}, args.rounds, event_ms)["gcnii"]
            step = lambda: te.train(m, g, feats, labels, torch.nn.NLLLoss(), opt, idx_train)
            timings["train_step_l8"] = rounds_of({"gcnii": step}, args.rounds, host_ms)["gcnii"]
            del m, opt
            torch.cuda.empty_cache()
            entry["widths"][str(d)] = timings
            print(f"# {name} hidden {d}: {json.dumps(timings)}", file=sys.stderr, flush=True)      # progress; the result is the last line
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
