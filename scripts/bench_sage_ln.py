"""Sampled-block SAGE teacher step with LayerNorm tails (norm_type "layer") against BatchNorm tails on the SAME batches: ms per step of
the engine alone (TeacherEngine.step_sage over pre-sampled batches) and of the step including the sampler (NodeDataLoader iteration +
step), on the ogbn-arxiv (B=512, dropout 0.2) and ogbn-products (B=4096, dropout 0.5) configs, fan-out 5,10,15, hidden 256.
The two norms are measured in alternating rounds; the median round is reported.

    python scripts/bench_sage_ln.py [--configs ogbn-arxiv,ogbn-products] [--steps 30] [--rounds 3] [--out profiles/sage_ln_bench_a.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import data, teacher  # noqa: E402
from glnn_amd.graph import MultiLayerNeighborSampler, NodeDataLoader  # noqa: E402
from glnn_amd.models import Model  # noqa: E402

DEV = "cuda:0"
# reference train.conf.yaml (arxiv: B=512, dropout 0.2, lr 0.01; products: B=4096, dropout 0.5, lr 0.003), as scripts/bench_train_sage.py
CFG = {"ogbn-arxiv": dict(f=128, c=40, B=512, p=0.2, lr=0.01, n_train=90941),
       "ogbn-products": dict(f=100, c=47, B=4096, p=0.5, lr=0.003, n_train=196615)}


def _engine(c, norm):
    torch.manual_seed(0)
    model = Model(dict(model_name="SAGE", num_layers=3, feat_dim=c["f"], hidden_dim=256, label_dim=c["c"], dropout_ratio=c["p"],
                       norm_type=norm, device=DEV))
    model.train()
    return teacher.get_engine(model, torch.optim.Adam(model.parameters(), lr=c["lr"]))


def _loader(g, idx, c):
    return NodeDataLoader(g, idx, MultiLayerNeighborSampler([5, 10, 15]), batch_size=c["B"], shuffle=True, drop_last=True, seed=7)


def _time_engine(eng, batches, feats, labels):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for input_nodes, output_nodes, blocks in batches:
        eng.step_sage(blocks, feats, labels, output_nodes, 1.0, input_nodes=input_nodes)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / len(batches)


def _time_with_sampler(eng, g, idx, c, feats, labels, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for input_nodes, output_nodes, blocks in _loader(g, idx, c):
        eng.step_sage(blocks, feats, labels, output_nodes, 1.0, input_nodes=input_nodes)
        n += 1
        if n == steps:
            break
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "SAGE teacher step, LayerNorm vs BatchNorm tails, same batches (ms per step; median of alternating rounds)",
           "fanout": [5, 10, 15], "hidden": 256, "steps": a.steps, "rounds": a.rounds, "configs": {}}
    for name in a.configs.split(","):
        c = CFG[name]
        g = data.make_graph(name, seed=0, device=DEV)
        feats, labels, _, _ = data.make_node_data(name, seed=0, device=DEV, n=g.n_dst)
        torch.manual_seed(0)
        idx = torch.randperm(g.n_dst)[:c["n_train"]].to(DEV)
        batches = []
        for b in _loader(g, idx, c):
            batches.append(b)
            if len(batches) == a.steps:
                break
        engs = {norm: _engine(c, norm) for norm in ("batch", "layer")}
        for eng in engs.values():                                   # warm-up: arena, descriptor, code objects
            _time_engine(eng, batches[:3], feats, labels)
        t_eng = {k: [] for k in engs}
        t_smp = {k: [] for k in engs}
        for _ in range(a.rounds):
            for norm, eng in engs.items():
                t_eng[norm].append(_time_engine(eng, batches, feats, labels))
                t_smp[norm].append(_time_with_sampler(eng, g, idx, c, feats, labels, a.steps))
        row = {"B": c["B"], "dropout": c["p"]}
        for norm in engs:
            row[f"{norm}_engine_ms"] = round(statistics.median(t_eng[norm]), 4)
            row[f"{norm}_with_sampler_ms"] = round(statistics.median(t_smp[norm]), 4)
            row[f"{norm}_engine_rounds_ms"] = [round(t, 4) for t in t_eng[norm]]
            row[f"{norm}_with_sampler_rounds_ms"] = [round(t, 4) for t in t_smp[norm]]
        row["ratio_engine"] = round(row["layer_engine_ms"] / row["batch_engine_ms"], 4)
        row["ratio_with_sampler"] = round(row["layer_with_sampler_ms"] / row["batch_with_sampler_ms"], 4)
        assert all(torch.isfinite(e.loss_out).all() for e in engs.values())
        res["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
