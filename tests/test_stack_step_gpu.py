"""The scaffold GCNII and PNA share (models._ConvStack, TeacherEngine._step_stack_body) on the GPU: three train() steps of a two-layer
teacher with dropout 0.5 on a 70-row graph with one row without in-edges -- both dropout sites outside the stack, both layers and the
masked H_0 backward.  Two runs from the same seeds are bit-equal, and the timed launches of a step are, name for name, the sequence the
steps issued before they had a scaffold (recorded then, written out below).  The kernels' own lane layouts and long rows belong to
tests/test_gcnii_gpu.py and tests/test_pna_gpu.py."""
import numpy as np
import pytest
import torch

from graphgen import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, FEAT, HIDDEN, LABELS, LAYERS, STEPS = 70, 12, 16, 4, 2, 3

# what ops.set_timing's collector receives during one step (the second), recorded before the two steps shared a scaffold
SEQUENCE = {
    "GCNII": ["gemm", "gcnii_layer", "gcnii_layer", "gemm", "gemm", "gcnii_layer_bwd", "gcnii_layer_bwd", "gcnii_layer_bwd"],
    "PNA": ["gemm", "gemm", "gemm", "pna_agg_fwd", "gemm", "gemm", "gemm", "gemm", "pna_agg_fwd", "gemm", "gemm", "gemm", "gemm", "gemm",
            "pna_agg_bwd", "gemm", "gemm", "gemm", "gemm", "pna_agg_bwd", "gemm", "gemm", "gemm"],
}


def problem():
    ip, ix = random_graph(N, 4, seed=5, isolated=1)
    assert (np.diff(ip) == 0).sum() >= 1
    rs = np.random.RandomState(9)
    x = rs.standard_normal((N, FEAT)).astype(np.float32)
    labels = rs.randint(0, LABELS, N)
    delta = float(np.mean(np.log(np.diff(ip).astype(np.float64) + 1.0)))
    return ip, ix, x, labels, np.arange(0, N, 2), delta


def run(name, dropout=0.5, names=None):
    """STEPS train() steps from fixed seeds: (losses, the state_dict).  names: a list that receives the timed op names of the second step."""
    from glnn_amd import ops
    from glnn_amd.graph import CSRGraph
    from glnn_amd.models import Model
    from glnn_amd.train_and_eval import train
    ip, ix, x, labels, idx, delta = problem()
    g = CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), N)
    tx, tl, ti = torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(idx).to(DEV)
    torch.manual_seed(3)
    m = Model(dict(model_name=name, num_layers=LAYERS, feat_dim=FEAT, hidden_dim=HIDDEN, label_dim=LABELS, dropout_ratio=dropout,
                   norm_type="none", device=DEV, pna_delta=delta))
    opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=5e-4)
    losses = []
    for step in range(STEPS):
        timed = [] if names is not None and step == 1 else None
        ops.set_timing(timed)
        try:
            losses.append(train(m, g, tx, tl, torch.nn.NLLLoss(), opt, ti))
        finally:
            ops.set_timing(None)
        if timed is not None:
            torch.cuda.synchronize()
            names.extend(t[0] for t in timed)
    return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", ["GCNII", "PNA"])
def test_three_steps_repeat_bit_for_bit_and_launch_the_recorded_sequence(name):
    losses, sd = run(name)
    names = []
    losses2, sd2 = run(name, names=names)
    print(name, [l.hex() for l in losses], names)
    assert all(np.isfinite(l) for l in losses) and len(set(losses)) == STEPS
    assert losses == losses2
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert names == SEQUENCE[name]
