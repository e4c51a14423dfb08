"""fp32 vs bf16 activation storage of the whole-graph SAGE teacher forward (SAGE.inference(..., dtype=torch.bfloat16),
csrc/sage_bf16.hip) on the products-shaped bench graph (data.make_graph, dims [100, 256, 256, 47], BatchNorm) and the arxiv-shaped one
([128, 256, 256, 40]).  Per graph: the forward in both storages (device events, warm-up, median of --reps), their ratio, the algorithmic
bytes of every layer in both storages, the largest |bf16 - fp32| logit difference and the share of rows whose argmax agrees.  One JSON line.

    python scripts/bench_bf16_inference.py [--reps 20] [--graphs ogbn-products,ogbn-arxiv] [--out profiles/bf16_inference_a.json]

Algorithmic bytes of a layer: per edge one int32 index and one gathered row at its STORED width (fp32: round4(d) floats, bf16: round8(d)
bf16), per destination row its indptr entry, its self row and its output row at the stored width; the weights are not counted."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops                                # noqa: E402
from glnn_amd.graph import FullNeighborLoader                 # noqa: E402
from glnn_amd.models import SAGE, Model                       # noqa: E402

DIMS = {"ogbn-products": [100, 256, 256, 47], "ogbn-arxiv": [128, 256, 256, 40]}     # reference train.conf.yaml teachers (BN, 3 layers)


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


def layer_plan(dims):
    """The launches of the whole-graph sweep (SAGE._whole_graph_layer / _whole_graph_layer_bf16), one entry per layer:
    (name, gathered width, output width, whether the output is gathered by the next layer)."""
    L = len(dims) - 1
    plan, projected = [], None
    for l in range(L):
        din, dout = dims[l], dims[l + 1]
        nxt = (dims[l + 1], dims[l + 2]) if l + 1 < L else None
        gathered_next = nxt is not None and nxt[0] <= nxt[1]
        if projected is not None:
            plan.append((f"L{l} aggregate (projected {projected})", projected, dout, gathered_next))
            projected = None
        elif nxt is not None and din <= dout and din <= 256 and dout <= 256 and nxt[0] > nxt[1] and nxt[1] <= 256 and SAGE.CHAIN_NEXT_PROJECTION:
            plan.append((f"L{l} fused {din}->{dout} + chained {nxt[1]}", din, nxt[1], True))
            projected = nxt[1]
        elif din > dout:
            plan.append((f"L{l} project-first {din}->{dout}", dout, dout, gathered_next))
        else:
            plan.append((f"L{l} fused {din}->{dout}" if din <= 256 and dout <= 256 else f"L{l} aggregate {din} + GEMM", din, dout,
                         gathered_next))
    return plan


def alg_bytes(plan, n, nnz, bf16):
    out = []
    for name, dg, dout, gathered_next in plan:
        gw = ops.round8(dg) * 2 if bf16 else ops.round4(dg) * 4
        ow = ops.round8(dout) * 2 if (bf16 and gathered_next) else ops.round4(dout) * 4
        out.append({"layer": name, "bytes": nnz * (4 + gw) + n * (8 + gw + ow)})
    return out


def run_graph(name, reps, dev):
    dims = DIMS[name]
    torch.manual_seed(0)
    g = data.make_graph(name, seed=0, device=dev)
    n, nnz = g.n_dst, g.num_edges()
    feats = ops.as_feat(torch.randn(n, dims[0], device=dev))
    model = Model(dict(model_name="SAGE", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type="batch", device=dev))
    with torch.no_grad():                 # non-trivial eval BatchNorm statistics
        for bn in model.encoder.norms:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    model.eval()
    loader = FullNeighborLoader(g, 4096)
    with torch.no_grad():
        ms32 = timed(lambda: model.inference(loader, feats), reps)
        ms16 = timed(lambda: model.inference(loader, feats, dtype=torch.bfloat16), reps)
        y32 = model.inference(loader, feats)
        y16 = model.inference(loader, feats, dtype=torch.bfloat16)
        diff = float((y16 - y32).abs().max())
        rowmax = float(y32.abs().max())
        agree = float((y16.argmax(1) == y32.argmax(1)).float().mean())
    plan = layer_plan(dims)
    b32, b16 = alg_bytes(plan, n, nnz, False), alg_bytes(plan, n, nnz, True)
    res = {"graph": f"{name}-shaped synthetic", "n": n, "nnz": nnz, "dims": dims, "norm": "batch",
           "fp32_ms": round(ms32, 3), "bf16_ms": round(ms16, 3), "ratio_bf16_over_fp32": round(ms16 / ms32, 4),
           "alg_bytes_fp32": b32, "alg_bytes_bf16": b16,
           "alg_GB_fp32": round(sum(b["bytes"] for b in b32) / 1e9, 3), "alg_GB_bf16": round(sum(b["bytes"] for b in b16) / 1e9, 3),
           "alg_TBps_fp32": round(sum(b["bytes"] for b in b32) / (ms32 * 1e-3) / 1e12, 3),
           "alg_TBps_bf16": round(sum(b["bytes"] for b in b16) / (ms16 * 1e-3) / 1e12, 3),
           "max_abs_logit_diff": diff, "max_abs_logit_fp32": rowmax, "argmax_agree": round(agree, 6), "reps": reps}
    del g, feats, model, loader, y32, y16
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--graphs", default="ogbn-products,ogbn-arxiv")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"what": "whole-graph SAGE teacher forward, fp32 vs bf16 activation storage (Model.inference(..., dtype=torch.bfloat16))"}
    for name in [s for s in args.graphs.split(",") if s]:
        res[name] = run_graph(name, max(1, args.reps), dev)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
