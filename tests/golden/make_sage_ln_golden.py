"""Golden vectors for the SAGE teacher with LayerNorm tails (norm_type "layer"), produced by the reference's own Python.

Reference code that runs here, unmodified, imported from the reference checkout (make_teacher_golden.REF):
  * models.Model / models.SAGE with norm_type="layer": SAGEConv -> nn.LayerNorm(hidden) -> relu -> dropout(p=0) per hidden layer
    (models.py:87-97, 113-117);
  * train_and_eval.train_sage (:32-56): log_softmax -> NLLLoss -> .item() -> backward -> Adam.step(), two epochs over three
    fixed batches of sampled blocks.
The dgl SAGEConv is the differentiable torch stand-in of make_teacher_train_golden.py (dgl itself is absent), with its import
stubs.  The blocks hold a hub destination above the long-row threshold (128 in-edges) and a destination without in-edges; the
hidden width (30) is not a multiple of 4.  Dropout is 0: torch's Philox stream cannot be replayed.

    python tests/golden/make_sage_ln_golden.py        (needs the reference checkout)
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
import make_teacher_golden as mtg                  # noqa: E402  (Block + import stubs)
import make_teacher_train_golden as mttg           # noqa: E402  (differentiable SAGEConv stand-in, block sampler)
from graphgen import random_graph                  # noqa: E402


def main():
    mtg._stub_modules()
    dgl_nn = sys.modules["dgl.nn"]
    dgl_nn.SAGEConv, dgl_nn.GraphConv = mttg.TrainSAGEConv, mttg.TrainGraphConv
    sys.modules["dgl"].function = None
    for name in ("dgl.function", "ogb", "ogb.nodeproppred"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["ogb.nodeproppred"].Evaluator = type("Evaluator", (), {})
    sys.modules["dgl.function"].copy_u = sys.modules["dgl.function"].sum = None
    sys.path.insert(0, mtg.REF)
    import models as ref_models            # noqa: reference, unmodified
    import train_and_eval as ref_te        # noqa
    torch.set_num_threads(1)
    out = {}

    n, dims, fanouts, bsz = 600, [20, 30, 30, 6], [4, 6, 200], 40
    indptr, indices = random_graph(n, 6, seed=51, power=0.5, isolated=5, hub=180)
    deg = np.diff(indptr)
    hub, iso = int(np.argmax(deg)), int(np.flatnonzero(deg == 0)[0])
    assert deg[hub] > 128
    rs = np.random.RandomState(51)
    feats = rs.standard_normal((n, dims[0])).astype(np.float32)
    labels = rs.randint(0, dims[-1], n).astype(np.int64)
    rest = np.setdiff1d(rs.permutation(n), [hub, iso])
    rs.shuffle(rest)
    train_ids = np.concatenate([[hub, iso], rest[:3 * bsz - 2]])          # batch 0 holds the hub and an isolated destination
    batches = []
    for b in range(3):
        seeds = train_ids[b * bsz:(b + 1) * bsz]
        input_nodes, blocks = mttg.sample_blocks(indptr, indices, seeds, fanouts, rs)
        batches.append((torch.from_numpy(input_nodes), torch.from_numpy(seeds), blocks))
        out[f"b{b}.input_nodes"], out[f"b{b}.output_nodes"] = input_nodes, seeds
        for l, blk in enumerate(blocks):
            out[f"b{b}.l{l}.indptr"], out[f"b{b}.l{l}.indices"] = blk.indptr, blk.indices
            out[f"b{b}.l{l}.n_src"] = np.int64(blk.n_src)
    torch.manual_seed(51)
    conf = dict(model_name="SAGE", num_layers=3, feat_dim=dims[0], hidden_dim=dims[1], label_dim=dims[-1], dropout_ratio=0.0,
                norm_type="layer", device="cpu")
    model = ref_models.Model(conf)
    with torch.no_grad():
        for lay in model.encoder.layers:
            lay.fc_neigh.bias.copy_(torch.randn_like(lay.fc_neigh.bias) * 0.1)
        for nm in model.encoder.norms:                    # away from the (1, 0) initialisation, so their gradients matter
            nm.weight.uniform_(0.5, 1.5)
            nm.bias.uniform_(-0.2, 0.2)
    wd = 5e-4
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=wd)        # train_teacher.py:234-236
    step_losses = []
    base = nn.NLLLoss()                                                               # train_teacher.py:237

    def criterion(o, y):
        l = base(o, y)
        step_losses.append(float(l.item()))
        return l

    for k, v in model.state_dict().items():
        out[f"init.{k}"] = v.numpy().copy()
    tf, tl = torch.from_numpy(feats), torch.from_numpy(labels)
    epoch_losses = [ref_te.train_sage(model, batches, tf, tl, criterion, optimizer) for _ in range(2)]
    out["epoch_losses"], out["step_losses"] = np.asarray(epoch_losses), np.asarray(step_losses)
    names = [k for k, _ in model.named_parameters()]
    for k, v in model.state_dict().items():
        out[f"final.{k}"] = v.numpy().copy()
    for k, p in zip(names, model.parameters()):
        st = optimizer.state[p]
        out[f"exp_avg.{k}"], out[f"exp_avg_sq.{k}"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        out["adam_step"] = np.int64(int(st["step"]))
    model.eval()
    with torch.no_grad():
        inp, outn, blks = batches[0]
        out["eval_logits_b0"] = model(blks, tf[inp]).numpy().copy()
    out.update({"indptr": indptr, "indices": indices, "feats": feats, "labels": labels, "dims": np.asarray(dims), "wd": np.float64(wd),
                "lr": np.float64(0.01), "eps": np.float64(model.encoder.norms[0].eps), "hub": np.int64(hub), "isolated": np.int64(iso)})
    path = os.path.join(HERE, "sage_ln_teacher.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; epoch losses", epoch_losses)


if __name__ == "__main__":
    main()
