"""One DeepWalk step (csrc/deepwalk.hip, docs/POSITION_SEMANTICS.md) at the arxiv-shaped and products-shaped synthetic graphs: --roots walk
roots, walk length --walk_length, context --context, --negatives negatives per positive, width --dim.
  native            DeepWalk.step: pairs (walk included), score, the two transposes, apply -- and each of those stages alone;
                    transposes_share = the two transposes over the whole step: the part proportional to N.
  torch             the usual composition on the same device, the SAME pair lists and the same initial table: nn.Embedding(sparse=True),
                    the loss in torch ops (softplus), torch.optim.SparseAdam.  It is given the pair lists: compare it with
                    native_given_pairs (score + transposes + apply).
  agreement         max |Z_native - Z_torch| after ONE step from the same table (fp32 both; the summation orders differ).
Every figure is the median of --rounds rounds in the same process, alternating, min and max beside it: host wall-clock around a
synchronize.  One JSON line; no ratio is gated.

    python scripts/bench_deepwalk.py [--rounds 5] [--graphs ogbn-arxiv,ogbn-products] [--roots 4096] [--out profiles/deepwalk_bench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_subgraph import rounds_of                                                # noqa: E402
from glnn_amd import data, ops                                                      # noqa: E402
from glnn_amd.position import DeepWalk                                              # noqa: E402


def torch_step(emb, opt, start, rest, n_pos):
    opt.zero_grad()
    s = (emb(start)[:, None, :] * emb(rest)).sum(dim=2)
    loss = F.softplus(-s[:, :n_pos]).mean() + F.softplus(s[:, n_pos:]).mean()
    loss.backward()
    opt.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", default="ogbn-arxiv,ogbn-products")
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--walk_length", type=int, default=20)
    ap.add_argument("--context", type=int, default=10)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_deepwalk.py needs cuda:0 (MI355X): nothing is measured without the GPU")
    dev = "cuda:0"
    L, c, k, d = args.walk_length, args.context, args.negatives, args.dim
    res = {"rounds": args.rounds, "roots": args.roots, "walk_length": L, "context": c, "negatives": k, "dim": d,
           "device": torch.cuda.get_device_name(0),
           "baseline": "nn.Embedding(sparse=True) + softplus loss in torch ops + torch.optim.SparseAdam on the same device, the same pair "
                       "lists and initial table; same process, alternating rounds, host wall-clock", "graphs": {}}
    for name in args.graphs.split(","):
        g = data.make_graph(name, seed=0, device=dev, scale=args.scale)
        n = g.n_dst
        torch.manual_seed(0)
        roots = torch.randperm(n)[:args.roots].contiguous()
        dw = DeepWalk(g, d, L, c, k, lr=0.01, seed=0)
        z0 = dw.embedding.clone()
        _, start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs(g.indptr, g.indices, roots, L, c, k, 1, 2)
        q, r = rest.shape
        start_l, rest_l = start.long(), rest.long()
        emb = torch.nn.Embedding(n, d, sparse=True, device=dev)
        with torch.no_grad():
            emb.weight.copy_(z0)
        opt = torch.optim.SparseAdam(emb.parameters(), lr=0.01)
        # agreement after one step from the same table
        dw.step(roots, 1, 2)
        torch_step(emb, opt, start_l, rest_l, c - 1)
        entry = {"n": n, "nnz": g.num_edges(), "windows": q, "pairs": q * r,
                 "max_abs_diff_after_one_step": float((dw.embedding - emb.weight.detach()).abs().max())}

        def given_pairs():
            gr, gs, zs, parts = ops.deepwalk_score(dw.embedding, start, rest, c, k)
            tw = ops.csr_transpose(win_indptr, start, q, n, q)
            tp_indptr, _, tp_eids = ops.csr_transpose_eids(pair_indptr, rest.view(-1), q, n, q * r)
            dw.steps += 1
            return ops.deepwalk_apply(dw.embedding, dw.exp_avg, dw.exp_avg_sq, tw, (tp_indptr, tp_eids), gr, gs, zs, parts, c, k, dw.lr,
                                      dw.betas, dw.eps, dw.steps)

        gr, gs, zs, parts = ops.deepwalk_score(dw.embedding, start, rest, c, k)
        tw = ops.csr_transpose(win_indptr, start, q, n, q)
        tp_indptr, _, tp_eids = ops.csr_transpose_eids(pair_indptr, rest.view(-1), q, n, q * r)

        def apply_only():
            dw.steps += 1
            return ops.deepwalk_apply(dw.embedding, dw.exp_avg, dw.exp_avg_sq, tw, (tp_indptr, tp_eids), gr, gs, zs, parts, c, k, dw.lr, dw.betas,
                                      dw.eps, dw.steps)

        t = rounds_of({
            "native_step": lambda: dw.step(roots, 1, 2),
            "native_given_pairs": given_pairs,
            "torch_given_pairs": lambda: torch_step(emb, opt, start_l, rest_l, c - 1),
            "pairs": lambda: ops.deepwalk_pairs(g.indptr, g.indices, roots, L, c, k, 1, 2),
            "score": lambda: ops.deepwalk_score(dw.embedding, start, rest, c, k),
            "transposes": lambda: (ops.csr_transpose(win_indptr, start, q, n, q),
                                   ops.csr_transpose_eids(pair_indptr, rest.view(-1), q, n, q * r)),
            "apply": apply_only,
        }, args.rounds)
        t["transposes_share_of_native_step"] = round(t["transposes"]["ms"] / t["native_step"]["ms"], 4)
        t["native_given_pairs_over_torch"] = round(t["native_given_pairs"]["ms"] / t["torch_given_pairs"]["ms"], 4)
        entry["step"] = t
        print(f"# {name}: {json.dumps(entry)}", file=sys.stderr, flush=True)
        res["graphs"][name] = entry
        del g, dw, emb, opt, z0
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
