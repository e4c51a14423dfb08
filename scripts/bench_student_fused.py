"""The one-launch form of the bf16 student chain (csrc/mlp_fused_bf16.hip, serve.compile_student(fused=True)) against the per-layer chain
(csrc/gemm_bf16.hip, unchanged), in one process: BatchNorm students over random N(0,1) features and random weights (never zero-filled
operands: they read high), log-probabilities out, at batch sizes from one row to the whole matrix, with fp32 and with bf16 features.

Per cell (shape, feature dtype, m, form):
  device_us   device-event time per call over enough back-to-back calls to fill >= 0.2 s
  host_us     (m <= 1024) host clock around ONE call + synchronise: the online latency, launch overhead included (median of 200 calls)
Warm-up, then ALTERNATING fused / chain rounds, the median of --reps rounds of each.  The same for a ServedPositionStudent (ids ->
assembled block -> chain) at 10 / 4096 / 65,536 ids with check_ids=False.  No time here is a bar: the table is what decides whether a
default may ever change.  One JSON line.

    python scripts/bench_student_fused.py [--reps 7] [--shapes arxiv,products,arxiv_w4] [--out profiles/student_fused_a.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd import ops, serve                               # noqa: E402
from glnn_amd.models import Model                             # noqa: E402
from glnn_amd.position import PositionTable                   # noqa: E402

SHAPES = {"arxiv": (169343, [128, 256, 256, 40]), "products": (2449029, [100, 256, 256, 47]), "arxiv_w4": (169343, [128, 1024, 1024, 40])}
BATCHES = [1, 10, 64, 1024, 16384, None]          # None: every row
FILL_MS = 200.0
HOST_CALLS = 200


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def student(dims, dev):
    torch.manual_seed(0)
    model = Model(dict(model_name="MLP", num_layers=len(dims) - 1, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1],
                       dropout_ratio=0.5, norm_type="batch", device=dev))
    with torch.no_grad():                 # non-trivial eval BatchNorm statistics
        for bn in model.encoder.norms:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    return model.eval()


def device_ms(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def host_us(fn):
    ts = []
    for _ in range(HOST_CALLS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return median(ts)


def measure(fns, reps, with_host):
    """fns: {form: callable}.  Returns {form: {device_us, host_us?}}: alternating rounds, medians."""
    calls = {}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[k] = max(1, min(20000, int(FILL_MS / max(device_ms(fn, 3), 1e-3)) + 1))
    dev = {k: [] for k in fns}
    host = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            dev[k].append(device_ms(fn, calls[k]) * 1e3)
        if with_host:
            for k, fn in fns.items():
                host[k].append(host_us(fn))
    res = {}
    for k in fns:
        res[k] = {"device_us": round(median(dev[k]), 2), "calls_per_round": calls[k]}
        if with_host:
            res[k]["host_us"] = round(median(host[k]), 2)
    return res


def run_shape(name, reps, dev):
    rows, dims = SHAPES[name]
    model = student(dims, dev)
    chain = serve.compile_student(model)
    res = {"rows": rows, "dims": dims, "norm": "batch", "reps": reps}
    try:
        fused = serve.compile_student(model, fused=True)
    except NotImplementedError as e:
        res["refused"] = str(e)
        return res
    res["tile_rows"] = fused.tile_rows
    torch.manual_seed(1)
    x32 = ops.as_feat(torch.randn(rows, dims[0], device=dev))
    feats = {"fp32": x32, "bf16": ops.to_bf16(x32)}
    out_f = torch.empty((rows, dims[-1]), dtype=torch.float32, device=dev)
    out_c = torch.empty_like(out_f)
    cells = []
    for dt, x in feats.items():
        for m in BATCHES:
            mm = rows if m is None else m
            xs, of, oc = x[:mm], out_f[:mm], out_c[:mm]
            fns = {"fused": lambda: fused.log_probs(xs, out=of), "chain": lambda: chain.log_probs(xs, out=oc)}
            r = measure(fns, reps, mm <= 1024)
            same = bool(torch.equal(of.view(torch.int32), oc.view(torch.int32)))
            cell = {"features": dt, "m": mm, "same_bits": same, "fused": r["fused"], "chain": r["chain"],
                    "device_chain_over_fused": round(r["chain"]["device_us"] / r["fused"]["device_us"], 3)}
            if mm <= 1024:
                cell["host_chain_over_fused"] = round(r["chain"]["host_us"] / r["fused"]["host_us"], 3)
            cells.append(cell)
            print(name, json.dumps(cell), file=sys.stderr, flush=True)
    res["cells"] = cells
    del x32, feats, out_f, out_c
    torch.cuda.empty_cache()
    return res


def run_position(reps, dev):
    """ServedPositionStudent over an arxiv-sized table: 128 feature + 128 position columns -> 256 -> 256 -> 40, every node embedded."""
    n, f, d = 169343, 128, 128
    dims = [f + d, 256, 256, 40]
    model = student(dims, dev)
    torch.manual_seed(2)
    x = torch.randn(n, f, device=dev)
    table = PositionTable(torch.randn(n, d, device=dev), torch.arange(n, device=dev), n)
    chain = serve.compile_position_student(model, x, table)
    fused = serve.compile_position_student(model, x, table, fused=True)
    cells = []
    for m in (10, 4096, 65536):
        ids = torch.randint(0, n, (m,), device=dev)
        of = torch.empty((m, dims[-1]), dtype=torch.float32, device=dev)
        oc = torch.empty_like(of)
        fns = {"fused": lambda: fused.log_probs(ids, out=of, check_ids=False), "chain": lambda: chain.log_probs(ids, out=oc, check_ids=False)}
        r = measure(fns, reps, m <= 1024)
        cell = {"ids": m, "same_bits": bool(torch.equal(of.view(torch.int32), oc.view(torch.int32))), "fused": r["fused"], "chain": r["chain"],
                "device_chain_over_fused": round(r["chain"]["device_us"] / r["fused"]["device_us"], 3)}
        if m <= 1024:
            cell["host_chain_over_fused"] = round(r["chain"]["host_us"] / r["fused"]["host_us"], 3)
        cells.append(cell)
        print("position", json.dumps(cell), file=sys.stderr, flush=True)
    return {"nodes": n, "dims": dims, "reps": reps, "cells": cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="arxiv,products,arxiv_w4")
    ap.add_argument("--no_position", action="store_true")
    ap.add_argument("--out", default="profiles/student_fused_a.json")
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"what": "bf16 MLP student serving, one-launch form (fused) vs per-layer chain, log-probabilities; device_us per call from device "
                   "events over >= 0.2 s of back-to-back calls, host_us = host clock of one call + synchronise; medians of alternating rounds"}
    for name in [s for s in args.shapes.split(",") if s]:
        res[name] = run_shape(name, max(1, args.reps), dev)
    if not args.no_position:
        res["position"] = run_position(max(1, args.reps), dev)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
