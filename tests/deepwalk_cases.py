"""What the CPU and the GPU tests of the DeepWalk position features share: the optimiser constants, the 512-node planted-community
configuration of the quality tests, its seed schedule and the initial table (DeepWalk's own draw).  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

BETAS, EPS = (0.9, 0.999), 1e-8


def clustered_case():
    """The 512-node configuration of the quality tests (CPU here, GPU in tests/test_deepwalk_gpu.py): 4 planted communities of 128 nodes,
    all nodes the roots of one batch per step, the walk / negative seeds of DeepWalk(seed=0).seeds(1, step)."""
    from glnn_amd.data import make_clustered_graph
    g = make_clustered_graph(512, 8, communities=4, p_in=0.9, seed=1)
    cfg = dict(d=16, length=10, context=5, negatives=1, lr=0.05, steps=100)
    return g.indptr.numpy(), g.indices.numpy(), np.arange(512) // 128, cfg


def step_seeds(step):
    walk_seed = (1 * 7919 + step * 31) & 0xFFFFFFFF
    return walk_seed, walk_seed ^ 0x4E454753


def init_embedding(n, d, seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return torch.randn((n, d), generator=gen, dtype=torch.float32).numpy()
