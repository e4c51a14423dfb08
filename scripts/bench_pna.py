"""PNA aggregation timings (csrc/pna.hip) next to the plain neighbour sum (ops.spmm, AGG_SUM) at the SAME shapes -- the arxiv- and
products-shaped synthetic graphs, F = 64 and F = 256 -- in the same process, in alternating rounds.  One JSON line.  None of its figures
is a pass / fail bar.

    python scripts/bench_pna.py [--rounds 5] [--graphs ogbn-arxiv,ogbn-products] [--widths 64,256] [--out profiles/pna_bench.json]

A round times one call each of: ONE ops.spmm(AGG_SUM) over the graph, glnn_pna_agg_fwd_f32 (training form: mu and the arguments are
written), ONE ops.spmm over the transposed graph, glnn_pna_agg_bwd_f32, and -- at hidden = F, two conv layers, dropout 0.5 -- one
TeacherEngine.step_gcn and one step_pna on the same features; medians over the rounds behind 2 warm-up rounds.  `ratio_fwd` = PNA forward
over the single gather: what four statistics (and 4F + F + 2F stored values per row against F) cost over one sum.  `ratio_bwd` = PNA
backward over the transposed sum: it gathers per entry 4F gradient floats, mu, sigma and the two arguments (8 rows) where the sum gathers
one.  `ratio_step` = step_pna over step_gcn."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, ops, teacher          # noqa: E402
from glnn_amd.models import Model                # noqa: E402

FEAT, LABELS, LAYERS, DROPOUT = 128, 40, 2, 0.5


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


def engine(name, hidden, delta, dev):
    m = Model(dict(model_name=name, num_layers=LAYERS, feat_dim=FEAT, hidden_dim=hidden, label_dim=LABELS, dropout_ratio=DROPOUT,
                   norm_type="none", device=dev, pna_delta=delta))
    for lay in m.encoder.layers:
        if hasattr(lay, "_allow_zero_in_degree"):
            lay._allow_zero_in_degree = True          # the synthetic graphs keep a few rows without in-edges
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=5e-4)
    teacher.check_supported(m, torch.nn.NLLLoss(), opt)
    return teacher.get_engine(m, opt)


def bench_graph(name, f, rounds, dev):
    g = data.make_graph(name, seed=0, device=dev)
    n, nnz = g.n_dst, g.num_edges()
    tg = g.transposed(False)
    g.transposed_eids()
    delta = float(torch.log(g.in_degrees().double() + 1.0).mean())

    def rows(d):
        t = ops.feat_empty(n, d, dev)
        t.copy_(torch.randn(n, d, device=dev))
        return t

    b, a = rows(f), rows(f)
    ds = torch.randn(n, 4 * f, device=dev)
    out1, out2, out3 = ops.feat_empty(n, f, dev), ops.feat_empty(n, f, dev), ops.feat_empty(n, f, dev)
    s_out = torch.empty(n, 4 * f, device=dev)
    s, mu, arg = ops.pna_agg_fwd(g.indptr, g.indices, nnz, b, n, a=a, want_arg=True)
    feats = torch.randn(n, FEAT, device=dev)
    labels = torch.randint(0, LABELS, (n,), device=dev)
    idx = torch.randperm(n, device=dev)[:max(n // 10, 1)].sort().values
    e_gcn, e_pna = engine("GCN", f, delta, dev), engine("PNA", f, delta, dev)
    calls = {
        "sum_fwd": lambda: ops.spmm(g.indptr, g.indices, b, n, ops.AGG_SUM, out=out1),
        "pna_fwd": lambda: ops.pna_agg_fwd(g.indptr, g.indices, nnz, b, n, a=a, want_arg=True, out=s_out),
        "sum_bwd": lambda: ops.spmm(tg.indptr, tg.indices, b, n, ops.AGG_SUM, out=out2),
        "pna_bwd": lambda: ops.pna_agg_bwd(g, ds, b, mu, s, arg, out=out3),
        "step_gcn": lambda: e_gcn.step_gcn(g, feats, labels, idx),
        "step_pna": lambda: e_pna.step_pna(g, feats, labels, idx),
    }
    ts = {key: [] for key in calls}
    for r in range(rounds + 2):
        for key, fn in calls.items():
            t = once(fn)
            if r >= 2:
                ts[key].append(t)
    res = {"n": n, "nnz": nnz, "f": f, "delta": round(delta, 4)}
    res.update({key: stats(val) for key, val in ts.items()})
    res["ratio_fwd"] = round(res["pna_fwd"]["med"] / res["sum_fwd"]["med"], 3)
    res["ratio_bwd"] = round(res["pna_bwd"]["med"] / res["sum_bwd"]["med"], 3)
    res["ratio_step"] = round(res["step_pna"]["med"] / res["step_gcn"]["med"], 3)
    res["pna_fwd_gather_TBps"] = round(nnz * (4 * f + 4) / (res["pna_fwd"]["med"] * 1e-3) / 1e12, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    res = {"rounds": args.rounds}
    for name in args.graphs.split(","):
        for f in (int(w) for w in args.widths.split(",")):
            res[f"{name}-shaped F={f}"] = bench_graph(name, f, args.rounds, dev)
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
