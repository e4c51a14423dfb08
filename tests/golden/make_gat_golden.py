"""Golden vectors for the GAT teacher, produced by the reference's own Python (models.GAT, models.Model, train_and_eval.train).

dgl is absent, so `dgl.nn.GATConv` is a small torch stand-in of dgl 0.6.1's published semantics (docs/GAT_SEMANTICS.md): fc without bias,
attn_l / attn_r, xavier_normal_(gain relu) on the three in that order, feat_drop applied once, leaky_relu(el[src] + er[dst]), edge softmax
over all in-edges of a destination, attn_drop on the normalised weights, sum, activation; a zero-in-degree graph raises.

In training it RECORDS the masks it draws -- one [N, in] feature mask and one [E, H] attention mask per layer call (edges in CSR order)
-- so the tests can replay them through the fp64 oracle (tests/gat_oracle.py).  The masks are drawn as dropout(ones), which is the same
distribution and the same arithmetic as dropout(x).  The graph is small, seeded, non-symmetric, has a multi-edge, one row above the
kernels' long-row threshold and no isolated row (a second tiny graph with one tests the raise).

    python tests/golden/make_gat_golden.py        (build container only: needs the reference checkout)
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_teacher_golden as mtg          # noqa: E402  (Block + import stubs)
from graphgen import csr_from_edges, random_graph      # noqa: E402

RECORDED = []          # (feature mask [N, in], attention mask [E, H]) per layer call in training


class StubGATConv(nn.Module):
    """dgl 0.6.1 GATConv on a homogeneous mtg.Block, differentiable."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False):
        super().__init__()
        assert not residual
        self._num_heads, self._out_feats = num_heads, out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop, self.attn_drop = nn.Dropout(feat_drop), nn.Dropout(attn_drop)
        self.negative_slope = negative_slope
        self.register_buffer("res_fc", None)
        self.activation = activation
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, graph, feat):
        n, H = graph.n_dst, self._num_heads
        deg = np.diff(graph.indptr)
        if (deg == 0).any():
            raise RuntimeError("There are 0-in-degree nodes in the graph")
        dst = torch.from_numpy(np.repeat(np.arange(n), deg))
        src = torch.from_numpy(graph.indices.astype(np.int64))
        fm = self.feat_drop(torch.ones_like(feat))
        z = self.fc(feat * fm).view(n, H, self._out_feats)
        el, er = (z * self.attn_l).sum(-1), (z * self.attn_r).sum(-1)
        e = F.leaky_relu(el[src] + er[dst], self.negative_slope)
        mx = torch.full((n, H), -float("inf"), dtype=e.dtype).index_reduce(0, dst, e.detach(), "amax")
        ex = torch.exp(e - mx[dst])
        den = torch.zeros(n, H, dtype=e.dtype).index_add(0, dst, ex)
        a = ex / den[dst]
        am = self.attn_drop(torch.ones_like(a))
        out = torch.zeros(n, H, self._out_feats, dtype=z.dtype).index_add(0, dst, (a * am).unsqueeze(-1) * z[src])
        if self.training:
            RECORDED.append(((fm != 0).numpy().astype(np.uint8), (am != 0).numpy().astype(np.uint8)))
        return self.activation(out) if self.activation else out


def graph():
    """Non-symmetric multigraph: self-loops (no isolated row), one hub row of > 128 in-edges, one hub SOURCE of > 128 out-edges and one of
    about 90 (the backward's source pass walks the transposed rows), and a guaranteed parallel edge."""
    n = 260
    ip, ix = random_graph(n, 3, seed=78, power=0.4, self_loops=True, hub=170)
    dst = np.repeat(np.arange(n), np.diff(ip))
    src = ix.astype(np.int64)
    u, v = int(src[10]), int(dst[10])
    rs = np.random.RandomState(79)
    src = np.concatenate([src, [u, u], np.full(170, 17), np.full(90, 101)])      # (u -> v) three times; nodes 17 and 101 fan out
    dst = np.concatenate([dst, [v, v], rs.randint(0, n, 170), rs.randint(0, n, 90)])
    return csr_from_edges(src, dst, n)


def _pack(masks):
    """[(fm, am)] per layer call -> packed bit arrays per layer."""
    return [np.packbits(m[0].reshape(-1)) for m in masks], [np.packbits(m[1].reshape(-1)) for m in masks]


def main():
    mtg._stub_modules()
    sys.modules["dgl.nn"].GATConv = StubGATConv
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
    n, dims, L = 260, [24, 32, 5], 2                  # 8 heads x 4 features, then 1 head x 5 classes
    p_feat, p_attn = 0.6, 0.3                          # the reference's GAT sections (train.conf.yaml:22-26)
    rs = np.random.RandomState(78)
    feats = rs.standard_normal((n, dims[0])).astype(np.float32)
    labels = rs.randint(0, dims[-1], n).astype(np.int64)
    idx_train = np.sort(rs.permutation(n)[:80]).astype(np.int64)
    g = mtg.Block(indptr, indices, n, n)
    out = {"indptr": indptr, "indices": indices, "feats": feats, "labels": labels, "idx_train": idx_train, "dims": np.asarray(dims),
           "num_heads": np.int64(8), "p_feat": np.float64(p_feat), "p_attn": np.float64(p_attn), "lr": np.float64(0.01),
           "wd": np.float64(0.01), "steps": np.int64(3)}
    torch.manual_seed(300)
    conf = dict(model_name="GAT", num_layers=L, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=p_feat,
                norm_type="none", device="cpu", attn_dropout_ratio=p_attn, num_heads=8)
    model = ref_models.Model(conf)
    for k, v in model.state_dict().items():
        out[f"init.{k}"] = v.numpy().copy()
    x, y, idx = torch.from_numpy(feats), torch.from_numpy(labels), torch.from_numpy(idx_train)
    model.eval()
    with torch.no_grad():
        h_list, logits = model.forward_fitnet(g, x)
    out["eval.logits"] = logits.numpy().copy()
    for i, h in enumerate(h_list):
        out[f"eval.h{i}"] = h.numpy().copy()
    # one training-mode forward + backward: logits, masks, gradients of every parameter
    model.train()
    RECORDED.clear()
    logits = model(g, x)
    loss = nn.NLLLoss()(logits.log_softmax(dim=1)[idx], y[idx])
    model.zero_grad()
    loss.backward()
    out["train.logits"], out["train.loss"] = logits.detach().numpy().copy(), np.float64(loss.item())
    fms, ams = _pack(RECORDED)
    for l in range(L):
        out[f"train.feat_mask{l}"], out[f"train.attn_mask{l}"] = fms[l], ams[l]
    for k, p in model.named_parameters():
        out[f"train.grad.{k}"] = p.grad.numpy().copy()
    # three train() steps
    model.zero_grad()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.01)          # cora GAT: reference train.conf.yaml:22-26
    RECORDED.clear()
    losses = [ref_te.train(model, g, x, y, nn.NLLLoss(), optimizer, idx) for _ in range(int(out["steps"]))]
    out["losses"] = np.asarray(losses)
    fms, ams = _pack(RECORDED)
    for s in range(int(out["steps"])):
        for l in range(L):
            out[f"step{s}.feat_mask{l}"], out[f"step{s}.attn_mask{l}"] = fms[s * L + l], ams[s * L + l]
    for k, v in model.state_dict().items():
        out[f"final.{k}"] = v.numpy().copy()
    # the raise: a tiny graph with one zero-in-degree row
    model.eval()
    try:
        model(mtg.Block(np.asarray([0, 1, 1, 2], np.int64), np.asarray([1, 0], np.int32), 3, 3), torch.zeros(3, dims[0]))
        out["zero_in_degree_raises"] = np.int64(0)
    except RuntimeError:
        out["zero_in_degree_raises"] = np.int64(1)
    path = os.path.join(HERE, "gat_teacher.npz")
    if os.path.exists(path):
        old = dict(np.load(path))
        if set(old) != set(out) or any(old[k].shape != out[k].shape for k in out):
            print("the existing file has other keys or shapes (the recipe changed): not compared")
        else:
            diff = max(float(np.max(np.abs(old[k].astype(np.float64) - out[k].astype(np.float64)))) if old[k].size else 0.0 for k in out)
            print("max |diff| against the existing file:", diff)
    np.savez_compressed(path, **out)
    print("wrote gat_teacher.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
