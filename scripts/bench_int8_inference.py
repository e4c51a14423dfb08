"""int8 activation storage of the whole-graph SAGE teacher forward against the fp32 and bf16 forwards on one MI355X
(docs/INT8_INFERENCE_SEMANTICS.md): the 3-layer BatchNorm SAGE-"gcn" teacher of bench.py's shapes (products: 100 -> 256 -> 256 -> 47,
arxiv: 128 -> 256 -> 256 -> 40) over the synthetic products- and arxiv-shaped graphs.

One process, alternating rounds (every configuration once per round, ROUNDS rounds, each timing ITERS back-to-back forwards between device
events after a warm-up); medians and the min..max spread of the rounds are reported.  Configurations:
  fp32             SAGE.inference() in steady state (its kept layer-1 aggregate and placed buffers in use);
  fp32_no_kept     the same with SAGE.CACHE_INPUT_AGGREGATE off: every forward gathers layer 1 again (what bf16 and int8 also do);
  bf16             dtype=torch.bfloat16, fp32 features cast once per call;
  int8             dtype=torch.int8, fp32 features quantised once per call;
  int8_rows        dtype=torch.int8 over features already held as int8 rows (ops.to_int8_rows once, outside the timing);
  int8_fanout_15   dtype=torch.int8 with fan_out=[15, 15, 15] (the fill launches included).
Per configuration:
  forward_ms       the forward;
  quant_ms         the glnn_quant_rows_i8 launches of one forward (device events around each launch, their sum; the median of the rounds)
                   and quant_share = quant_ms / forward_ms;
  argmax_agree     the share of rows whose arg-max class equals the fp32 forward's.  The teacher is UNTRAINED and the features synthetic:
                   what moves is how far the storage perturbs the logits, not an accuracy; max_rel_err is the largest difference from the
                   fp32 logits relative to the row's largest |logit|.
Writes profiles/int8_inference_bench_a.json.

  python scripts/bench_int8_inference.py [--graphs ogbn-products,ogbn-arxiv] [--rounds 5] [--iters 3] [--scale 1.0] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glnn_amd import data, ops            # noqa: E402
from glnn_amd.graph import FullNeighborLoader      # noqa: E402
from glnn_amd.models import SAGE, Model      # noqa: E402

FANOUT = 15
SAMPLE_SEED = 0


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def quant_ms(fn):
    """The quantise launches of one forward: the sum of their device times."""
    launches = []
    ops.set_timing(launches)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.set_timing(None)
    return sum(s.elapsed_time(e) for name, _, s, e in launches if name == "quant_rows_i8")


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds_ms": [round(t, 4) for t in v]}


def no_kept(fn):
    def run():
        SAGE.CACHE_INPUT_AGGREGATE = False
        try:
            return fn()
        finally:
            SAGE.CACHE_INPUT_AGGREGATE = True
    return run


def bench_graph(name, rounds, iters, scale, dev):
    g = data.make_graph(name, seed=0, device=dev, scale=scale)
    feats, labels, _, _ = data.make_node_data(name, seed=0, device=dev, n=g.n_dst)
    sh = data.SHAPES[name]
    torch.manual_seed(0)
    model = Model(dict(model_name="SAGE", num_layers=3, feat_dim=sh["f"], hidden_dim=256, label_dim=sh["c"], dropout_ratio=0.5,
                       norm_type="batch", device=dev)).eval()
    L = model.encoder.num_layers
    loader = FullNeighborLoader(g, 4096)
    rows = ops.to_int8_rows(feats)
    forms = {
        "fp32": lambda: model.inference(loader, feats),
        "fp32_no_kept": no_kept(lambda: model.inference(loader, feats)),
        "bf16": lambda: model.inference(loader, feats, dtype=torch.bfloat16),
        "int8": lambda: model.inference(loader, feats, dtype=torch.int8),
        "int8_rows": lambda: model.inference(loader, rows, dtype=torch.int8),
        f"int8_fanout_{FANOUT}": lambda: model.inference(loader, feats, dtype=torch.int8, fan_out=[FANOUT] * L, sample_seed=SAMPLE_SEED),
    }
    with torch.no_grad():
        for fn in forms.values():          # warm-up: code objects, placement, the kept aggregate, the cached sampled indptrs
            fn()
            fn()
        torch.cuda.synchronize()
        ref = model.inference(loader, feats)
        ref_arg, ref_max = ref.argmax(1), ref.abs().amax(1, keepdim=True).clamp_min(1e-30)
        quality = {}
        for k, fn in forms.items():
            y = fn()
            quality[k] = {"argmax_agree": float((y.argmax(1) == ref_arg).float().mean()),
                          "max_rel_err": float(((y - ref).abs() / ref_max).max()),
                          "label_match": float((y.argmax(1) == labels).float().mean())}
        ms, qms = {k: [] for k in forms}, {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                ms[k].append(timed(fn, iters))
            for k, fn in forms.items():
                qms[k].append(quant_ms(fn))
    rec = {"n": g.n_dst, "nnz": g.num_edges(), "configs": {}}
    for k in forms:
        fwd, q = stats(ms[k]), statistics.median(qms[k])
        rec["configs"][k] = {"forward": fwd, "quant_ms": q, "quant_share": q / fwd["median_ms"], **quality[k]}
    base = rec["configs"]["fp32"]["forward"]["median_ms"]
    for k, c in rec["configs"].items():
        f = c["forward"]
        print(f"{name} {k}: forward {f['median_ms']:.3f} ms ({f['min_ms']:.3f}..{f['max_ms']:.3f})  x{base / f['median_ms']:.3f} of fp32  "
              f"quantise {c['quant_ms']:.3f} ms ({100 * c['quant_share']:.1f} %)  argmax_agree {c['argmax_agree']:.4f}  "
              f"max_rel_err {c['max_rel_err']:.2e}", flush=True)
    model.encoder.release_placed()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ogbn-products,ogbn-arxiv")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_inference_bench_a.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_int8_inference.py measures on the GPU only")
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5 (medians of rounds are reported)")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "scale": args.scale,
              "fanout": FANOUT, "sample_seed": SAMPLE_SEED, "teacher": "untrained, synthetic features", "graphs": {}}
    for name in args.graphs.split(","):
        result["graphs"][name] = bench_graph(name, args.rounds, args.iters, args.scale, dev)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
