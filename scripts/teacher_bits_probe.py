"""Do the full-graph teachers still compute the same bits?  Fixed seeds, one process: per teacher kind (hidden 64, every dropout on:
GAT / GATv2 2 layers, 8 heads, feature and attention dropout; APPNP 2 trunk layers, trunk and edge dropout; GPRGNN 2 trunk layers; GCNII
3 conv layers, dropout 0.5) three train() steps and one train_subgraph epoch on a 600-row graph with a 200-edge hub row and
self-loop-only rows, then the parameter gradients of one autograd step (model(g, feats) in training mode, loss.backward()).  Prints one
sha256 per line; run it on two builds and compare the lines.  Public entry points only: it runs next to any build of the package.
python scripts/teacher_bits_probe.py [--kinds GAT,GATv2,APPNP,GPRGNN,GCNII]"""
import argparse, hashlib, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glnn_amd.graph import CSRGraph, RandomWalkSubgraphLoader
from glnn_amd.models import Model
from glnn_amd.train_and_eval import train, train_subgraph

KINDS = dict(GAT=dict(num_layers=2, num_heads=8, attn_dropout_ratio=0.3), GATv2=dict(num_layers=2, num_heads=8, attn_dropout_ratio=0.3),
             APPNP=dict(num_layers=2), GPRGNN=dict(num_layers=2), GCNII=dict(num_layers=3))      # (APPNP's edge_drop is 0.5 by default)
ap = argparse.ArgumentParser()
ap.add_argument("--kinds", default=",".join(KINDS))
kinds = ap.parse_args().kinds.split(",")

dev, N, D_IN, C = "cuda:0", 600, 24, 5
rs = np.random.RandomState(3)
src, dst = rs.randint(0, N - 8, 3 * N), rs.randint(0, N - 8, 3 * N)          # the last 8 rows keep their self loop alone: in-degree 1
hub = rs.choice(N - 8, 200, replace=False)
src, dst = np.concatenate([src, dst, hub, np.arange(N)]), np.concatenate([dst, src, np.zeros(200, np.int64), np.arange(N)])
order = np.lexsort((src, dst))
indptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int64)
g = CSRGraph(torch.from_numpy(indptr).to(dev), torch.from_numpy(src[order].astype(np.int32)).to(dev), N)
deg = np.diff(indptr)
assert deg.max() > 128 and deg.min() == 1
x = torch.from_numpy(rs.randn(N, D_IN).astype(np.float32)).to(dev)          # signed features: GAT's two half-products
y = torch.from_numpy(rs.randint(0, C, N).astype(np.int64)).to(dev)
idx_train = torch.from_numpy(rs.choice(N, 192, replace=False).astype(np.int64))


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


for name in kinds:
    conf = dict(model_name=name, feat_dim=D_IN, hidden_dim=64, label_dim=C, dropout_ratio=0.5, norm_type="none", device=dev, **KINDS[name])
    torch.manual_seed(11)
    m = Model(conf)
    opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=5e-4)
    crit = torch.nn.NLLLoss()
    losses = [train(m, g, x, y, crit, opt, idx_train.to(dev)) for _ in range(3)]
    print(f"{name} train x3: params {sha(m.parameters())} losses {[f'{v:.7f}' for v in losses]}", flush=True)
    loader = RandomWalkSubgraphLoader(g, idx_train, 64, 3, self_loop="add", shuffle=True, seed=5)
    loss = train_subgraph(m, loader, x, y, crit, opt)
    print(f"{name} train_subgraph epoch: params {sha(m.parameters())} loss {loss:.7f}", flush=True)
    torch.manual_seed(11)
    m = Model(conf).train()
    out = m(g, x).log_softmax(1)
    crit(out[idx_train.to(dev)], y[idx_train.to(dev)]).backward()
    print(f"{name} autograd: grads {sha(p.grad for p in m.parameters())} logits {sha([out])}", flush=True)
