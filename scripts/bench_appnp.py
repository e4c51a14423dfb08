"""APPNP propagation timings (csrc/appnp.hip) on the products-shaped synthetic graph at C = 47, K = 10, next to the stand-alone GCN-mode
aggregation (glnn_spmm_csr_f32, row_scale + col_scale) at the same width, plus the full cora APPNP training step.  One JSON line.

    python scripts/bench_appnp.py [--reps 20] [--out profiles/appnp_bench.json]

Algorithmic bytes of one iteration (per kept edge one gathered row of round4(C) floats + one int32 index; per row the indptr entry, the
row norm, one output row, plus the teleport row h0 (forward) or the running sum read + write (backward)); the dropped edges' rows are
not counted, their indices are."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops, train_and_eval as te          # noqa: E402
from glnn_amd.autograd import appnp_bwd, appnp_fwd            # noqa: E402
from glnn_amd.models import Model                             # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    g = data.make_graph("ogbn-products", seed=0, device=dev)
    n, nnz, C, K = g.n_dst, g.num_edges(), 47, 10
    d4 = ops.round4(C)
    in_norm, out_norm = g.degree_norms()
    g.transposed_eids()
    h0 = ops.feat_empty(n, C, dev)
    h0.copy_(torch.randn(n, C, device=dev))
    res = {"graph": "ogbn-products-shaped synthetic", "n": n, "nnz": nnz, "C": C, "K": K}

    def alg(keep, extra_row_floats):
        return nnz * 4 + keep * nnz * 4 * d4 + n * (8 + 4 + 4 * d4 + 4 * extra_row_floats)

    for p in (0.0, 0.5):
        ms = timed(lambda: appnp_fwd(g, h0, K, 0.1, p, 7), args.reps) / K
        res[f"fwd_ms_per_iter_p{p:g}"] = round(ms, 4)
        res[f"fwd_alg_TBps_p{p:g}"] = round(alg(1 - p, d4) / (ms * 1e-3) / 1e12, 3)
    for p in (0.0, 0.5):
        ms = timed(lambda: appnp_bwd(g, h0, K, 0.1, p, 7), args.reps) / K
        res[f"bwd_ms_per_iter_p{p:g}"] = round(ms, 4)
        res[f"bwd_alg_TBps_p{p:g}"] = round(alg(1 - p, 2 * d4) / (ms * 1e-3) / 1e12, 3)
    out = ops.feat_empty(n, C, dev)
    ms = timed(lambda: ops.spmm(g.indptr, g.indices, h0, n, ops.AGG_SUM, row_scale=in_norm, col_scale=out_norm, out=out), args.reps)
    res["spmm_gcn_ms"] = round(ms, 4)
    res["spmm_gcn_alg_TBps"] = round(alg(1.0, 0) / (ms * 1e-3) / 1e12, 3)

    # the full cora APPNP training step (reference train.conf.yaml cora APPNP: hidden 128, dropout 0.5, weight decay 0.01)
    gc = data.make_graph("cora", seed=0, device=dev)
    feats, labels, _, _ = data.make_node_data("cora", seed=0, device=dev, n=gc.n_dst)
    idx_train = torch.randperm(gc.n_dst)[:140].to(dev)
    model = Model(dict(model_name="APPNP", num_layers=2, feat_dim=feats.shape[1], hidden_dim=128, label_dim=7, dropout_ratio=0.5,
                       norm_type="none", device=dev))
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.01)
    crit = torch.nn.NLLLoss()
    for _ in range(5):
        te.train(model, gc, feats, labels, crit, opt, idx_train)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 50
    for _ in range(steps):
        te.train(model, gc, feats, labels, crit, opt, idx_train)
    torch.cuda.synchronize()
    res["cora_step_appnp_ms"] = round((time.perf_counter() - t0) / steps * 1e3, 4)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
