"""Serving a position-feature student by node id (glnn_amd.serve.ServedPositionStudent, csrc/position_serve.hip;
docs/POSITION_SEMANTICS.md, "Serving by node id") at the arxiv-shaped and products-shaped synthetic graphs: F = 128 / 100 features,
D = --dim position columns, an MLP3w8-like BatchNorm student, batches of --batches random ids, --unseen of the nodes without a table row.
  by_id      ServedPositionStudent.log_probs(ids) in bf16: the host-side range check of the ids (one read-back), one assembling launch,
             the bf16 chain;  by_id_unchecked: the same with check_ids=False;
  today      the path a user has without it: ServedStudent.log_probs(cat[ids]) with cat = [X | dense positions] ([N, F + D] fp32)
             materialised BEFORE the clock starts and the [ids] gather inside it;
  assemble   ops.position_rows alone (bf16 output).
Every figure is the median of --rounds rounds in the same process, alternating, min and max beside it: host wall-clock around a
synchronize.  cat_bytes is the [N, F + D] fp32 matrix by_id never builds.  One JSON line; no ratio is gated.

    python scripts/bench_position_serve.py [--rounds 5] [--graphs ogbn-arxiv,ogbn-products] [--out profiles/position_serve_bench.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_subgraph import rounds_of                                                # noqa: E402
from glnn_amd import data, ops, serve                                               # noqa: E402
from glnn_amd.models import Model                                                   # noqa: E402
from glnn_amd.position import PositionTable                                         # noqa: E402

HIDDEN = {"ogbn-arxiv": 256, "ogbn-products": 2048}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--unseen", default="0,0.2")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_position_serve.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    d = args.dim
    res = {"rounds": args.rounds, "dim": d, "device": torch.cuda.get_device_name(0),
           "timing": "same process, alternating rounds, host wall-clock around a synchronize", "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n, f, c = g.n_dst, data.SHAPES[name]["f"], data.SHAPES[name]["c"]
        torch.manual_seed(0)
        x = torch.randn(n, f, device=dev)
        model = Model(dict(model_name="MLP", num_layers=3, feat_dim=f + d, hidden_dim=HIDDEN[name], label_dim=c, dropout_ratio=0.5,
                           norm_type="batch", device=dev))
        with torch.no_grad():
            for bn in model.encoder.norms:
                bn.running_mean.uniform_(-0.2, 0.2)
                bn.running_var.uniform_(0.5, 1.5)
        model.eval()
        plain = serve.compile_student(model)
        entry = {"n": n, "nnz": g.num_edges(), "f": f, "hidden": HIDDEN[name], "cat_bytes": n * (f + d) * 4, "x_bytes": n * f * 4, "cases": {}}
        for frac in [float(s) for s in args.unseen.split(",")]:
            obs = torch.nonzero(torch.rand(n, device=dev) >= frac).flatten()
            table = PositionTable(torch.randn(obs.numel(), d, device=dev), obs, n)
            served = serve.compile_position_student(model, x, table, g if table.has_unseen else None)
            cat = torch.cat([x, table.dense(g)], 1)            # what serving needs today, built before anything is timed
            for m in [int(s) for s in args.batches.split(",")]:
                ids = torch.randint(0, n, (m,), device=dev)
                out_a = torch.empty((m, c), device=dev)
                out_b = torch.empty((m, c), device=dev)
                block = ops.bf16_empty(m, f + d, dev)
                fns = {"by_id": lambda: served.log_probs(ids, out=out_a),
                       "by_id_unchecked": lambda: served.log_probs(ids, out=out_a, check_ids=False),
                       "today": lambda: plain.log_probs(cat[ids], out=out_b),
                       "assemble": lambda: ops.position_rows(ids, x, table.rows, served.slot, g=served.g, out=block)}
                t = rounds_of(fns, args.rounds)
                for k in ("by_id", "by_id_unchecked"):
                    t[k]["over_today"] = round(t[k]["ms"] / t["today"]["ms"], 3)
                t["max_abs_logp_diff"] = float((out_a - out_b).abs().max())
                entry["cases"][f"unseen{frac:g}_m{m}"] = t
                print(f"# {name} unseen {frac:g} m {m}: {json.dumps(t)}", file=sys.stderr, flush=True)
            del cat, served, table
            torch.cuda.empty_cache()
        res["graphs"][name] = entry
        del g, x, model, plain
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
