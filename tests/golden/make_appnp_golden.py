"""Golden vectors for the APPNP teacher, produced by the reference's own Python (models.APPNP, models.Model, train_and_eval.train).

dgl is absent, so `dgl.nn.APPNPConv` is a small torch stand-in of dgl 0.6.1's published semantics:

    src_norm = out_deg.clamp(1)^-1/2, dst_norm = in_deg.clamp(1)^-1/2;  for t in 1..k:
        feat = dst_norm * (A (w_t * (src_norm * feat)))  with w_t = edge_drop(ones(E))   ;   feat = (1 - alpha) feat + alpha feat_0

In training it RECORDS the edge masks it draws (one [E] mask per iteration; edges in CSR order), so the tests can replay them through
the fp64 oracle (tests/appnp_oracle.py).  The graph is small, seeded, non-symmetric, has isolated nodes, a multi-edge and one row above
the kernels' long-row threshold.  Trunk dropout is 0 (torch's Philox stream cannot be replayed); the edge dropout is the reference's 0.5.

    python tests/golden/make_appnp_golden.py        (build container only: needs the reference checkout)
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_teacher_golden as mtg          # noqa: E402  (Block + import stubs)
from graphgen import csr_from_edges, random_graph      # noqa: E402

RECORDED = []          # masks drawn by the stand-in in training: one [k, E] uint8 array per forward


class StubAPPNPConv(nn.Module):
    """dgl 0.6.1 APPNPConv(k, alpha, edge_drop), differentiable, on an mtg.Block."""

    def __init__(self, k, alpha, edge_drop=0.0):
        super().__init__()
        self._k, self._alpha = k, alpha
        self.edge_drop = nn.Dropout(edge_drop)

    def forward(self, graph, feat):
        n = graph.n_dst
        dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(graph.indptr)))
        src = torch.from_numpy(graph.indices.astype(np.int64))
        in_deg = torch.from_numpy(np.diff(graph.indptr)).float()
        out_deg = torch.bincount(src, minlength=graph.n_src).float()
        src_norm = out_deg.clamp(min=1).pow(-0.5).unsqueeze(1)
        dst_norm = in_deg.clamp(min=1).pow(-0.5).unsqueeze(1)
        feat_0 = feat
        masks = []
        for _ in range(self._k):
            feat = feat * src_norm
            w = self.edge_drop(torch.ones(len(src), 1))
            masks.append((w[:, 0] != 0).numpy().astype(np.uint8))
            feat = torch.zeros(n, feat.shape[1]).index_add(0, dst, feat[src] * w)
            feat = feat * dst_norm
            feat = (1 - self._alpha) * feat + self._alpha * feat_0
        if self.training:
            RECORDED.append(np.stack(masks))
        return feat


def graph():
    """Non-symmetric multigraph: isolated rows, one hub row of > 128 in-edges, and a guaranteed parallel edge."""
    ip, ix = random_graph(260, 3, seed=77, power=0.4, isolated=6, hub=170)
    dst = np.repeat(np.arange(260), np.diff(ip))
    src = ix.astype(np.int64)
    u, v = int(src[10]), int(dst[10])
    src, dst = np.concatenate([src, [u, u]]), np.concatenate([dst, [v, v]])      # (u -> v) three times
    return csr_from_edges(src, dst, 260)


def main():
    mtg._stub_modules()
    sys.modules["dgl.nn"].APPNPConv = StubAPPNPConv
    sys.modules["dgl"].function = None
    for name in ("dgl.function", "ogb", "ogb.nodeproppred"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["ogb.nodeproppred"].Evaluator = type("Evaluator", (), {})
    sys.modules["dgl.function"].copy_u = sys.modules["dgl.function"].sum = None
    sys.path.insert(0, mtg.REF)
    import models as ref_models            # noqa: reference, unmodified
    import train_and_eval as ref_te        # noqa
    torch.set_num_threads(1)

    indptr, indices = graph()
    n, dims = 260, [24, 16, 5]
    rs = np.random.RandomState(77)
    feats = rs.standard_normal((n, dims[0])).astype(np.float32)
    labels = rs.randint(0, dims[-1], n).astype(np.int64)
    idx_train = np.sort(rs.permutation(n)[:80]).astype(np.int64)
    g = mtg.Block(indptr, indices, n, n)
    out = {"indptr": indptr, "indices": indices, "feats": feats, "labels": labels, "idx_train": idx_train, "dims": np.asarray(dims),
           "lr": np.float64(0.01), "wd": np.float64(0.01), "steps": np.int64(3)}
    for seed, norm in enumerate(("none", "batch", "layer")):
        torch.manual_seed(100 + seed)
        conf = dict(model_name="APPNP", num_layers=2, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.0,
                    norm_type=norm, device="cpu")
        model = ref_models.Model(conf)
        if norm == "batch":
            mtg.randomize_norms(model, rs)
        with torch.no_grad():
            for ln in model.encoder.norms if norm == "layer" else ():
                ln.weight.uniform_(0.5, 1.5)
                ln.bias.uniform_(-0.2, 0.2)
            for lay in model.encoder.layers:
                lay.bias.copy_(torch.randn_like(lay.bias) * 0.1)
        tag = f"{norm}"
        for k, v in model.state_dict().items():
            out[f"{tag}.init.{k}"] = v.numpy().copy()
        model.eval()
        with torch.no_grad():
            h_list, logits = model.forward_fitnet(g, torch.from_numpy(feats))
        out[f"{tag}.eval.logits"] = logits.numpy().copy()
        for i, h in enumerate(h_list):
            out[f"{tag}.eval.h{i}"] = h.numpy().copy()
        optimizer = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.01)          # cora APPNP: reference train.conf.yaml:28-30
        RECORDED.clear()
        losses = [ref_te.train(model, g, torch.from_numpy(feats), torch.from_numpy(labels), nn.NLLLoss(), optimizer, torch.from_numpy(idx_train))
                  for _ in range(int(out["steps"]))]
        out[f"{tag}.losses"] = np.asarray(losses)
        out[f"{tag}.masks"] = np.packbits(np.stack(RECORDED), axis=-1)       # [steps, k, ceil(E / 8)]
        for k, v in model.state_dict().items():
            out[f"{tag}.final.{k}"] = v.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "appnp_teacher.npz"), **out)
    print("wrote appnp_teacher.npz", {k: v.shape for k, v in out.items() if k.startswith("none.")})


if __name__ == "__main__":
    main()
