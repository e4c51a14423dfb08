"""DeepWalk position features for the MLP student (docs/POSITION_SEMANTICS.md): the device NOSMOG (Tian et al., ICLR 2023) adds to
GLNN -- a DeepWalk embedding of each node concatenated to its features in front of the MLP, so that inference stays one row lookup and an
MLP.  The skip-gram trainer is csrc/deepwalk.hip: node2vec's objective with p = q = 1, one table, batch-synchronous lazy Adam, a fixed
summation order and no float atomics (the same seed gives the same bits).  torch owns the memory and the CPU permutation; there is no CPU
path."""
import torch

from . import ops


class DeepWalk:
    """One embedding table over the nodes of the square graph `g` (on the GPU), trained by skip-gram with negative sampling over the
    windows of uniform random walks along in-edges (glnn_random_walk).
      .embedding   [N, dim] float32 on g's device; N(0, 1) drawn on the CPU from torch.Generator().manual_seed(seed), so an oracle can
                   start from the same bits
      .step(roots, walk_seed, neg_seed)   one optimiser step over the walks from `roots`; returns the loss as a device scalar
      .fit(epochs, batch_size)            every node a root once per epoch; returns the per-epoch mean loss (one host read per epoch)
    dim % 4 == 0, dim <= 256; 1 <= walk_length <= 64; 2 <= context_size <= walk_length + 1; num_negative >= 1."""

    def __init__(self, g, dim, walk_length=20, context_size=10, num_negative=1, lr=0.01, betas=(0.9, 0.999), eps=1e-8, seed=0):
        if not g.indptr.is_cuda:
            raise RuntimeError("DeepWalk: the trainer runs on the GPU (move the graph with g.to(device))")
        if g.n_dst != g.n_src:
            raise ValueError("DeepWalk: square graphs only")
        dim, walk_length, context_size, num_negative = int(dim), int(walk_length), int(context_size), int(num_negative)
        if dim < 4 or dim % 4 or dim > ops.DEEPWALK_MAX_DIM:
            raise ValueError(f"DeepWalk: dim must be a multiple of 4 in [4, {ops.DEEPWALK_MAX_DIM}] (got {dim})")
        if not 1 <= walk_length <= 64:
            raise ValueError(f"DeepWalk: walk_length must be in [1, 64] (got {walk_length})")
        if not 2 <= context_size <= walk_length + 1:
            raise ValueError(f"DeepWalk: context_size must be in [2, walk_length + 1] (got {context_size} for walk_length {walk_length})")
        if num_negative < 1:
            raise ValueError(f"DeepWalk: num_negative must be >= 1 (got {num_negative})")
        self.g, self.dim = g, dim
        self.walk_length, self.context_size, self.num_negative = walk_length, context_size, num_negative
        self.lr, self.betas, self.eps, self.seed = float(lr), (float(betas[0]), float(betas[1])), float(eps), int(seed)
        gen = torch.Generator()
        gen.manual_seed(self.seed)
        self.embedding = torch.randn((g.n_src, dim), generator=gen, dtype=torch.float32).to(g.device)
        self.exp_avg = torch.zeros_like(self.embedding)
        self.exp_avg_sq = torch.zeros_like(self.embedding)
        self.steps = 0          # optimiser steps taken: Adam's global step count
        self._epoch = 0

    def step(self, roots, walk_seed, neg_seed):
        """One step (docs/POSITION_SEMANTICS.md): walks from `roots` (int64, CPU or device; repeats allowed), the pair list, the scores and
        gradients at the frozen table, the two transposes, the lazy-Adam update in place.  Returns the loss of the step as a device scalar;
        nothing is read back (device roots cost one copy for the range check: pass CPU roots, as fit does)."""
        g, c, k = self.g, self.context_size, self.num_negative
        roots = torch.as_tensor(roots, dtype=torch.int64)
        if roots.numel() == 0:
            return torch.zeros((), dtype=torch.float32, device=g.device)
        _, start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs(g.indptr, g.indices, roots, self.walk_length, c, k, walk_seed, neg_seed)
        gr, gs, zs, loss_parts = ops.deepwalk_score(self.embedding, start, rest, c, k)
        q, r = rest.shape
        tw = ops.csr_transpose(win_indptr, start, q, g.n_src, q)
        tp_indptr, _, tp_eids = ops.csr_transpose_eids(pair_indptr, rest.view(-1), q, g.n_src, q * r)
        loss = ops.deepwalk_apply(self.embedding, self.exp_avg, self.exp_avg_sq, tw, (tp_indptr, tp_eids), gr, gs, zs, loss_parts, c, k,
                                  self.lr, self.betas, self.eps, self.steps + 1)
        self.steps += 1
        return loss

    def seeds(self, epoch, b):
        """(walk_seed, neg_seed) of batch b (0-based) of epoch `epoch` (1-based): RandomWalkSubgraphLoader's schedule."""
        walk_seed = (self.seed * 1000003 + epoch * 7919 + b * 31) & 0xFFFFFFFF
        return walk_seed, walk_seed ^ 0x4E454753

    def fit(self, epochs, batch_size, shuffle=True):
        """`epochs` passes in which every node is a root once, `batch_size` roots per step; the permutation comes from the CPU source
        RandomWalkSubgraphLoader uses (ops.randperm_cpu).  Epochs count on across calls.  Returns the mean loss of each epoch."""
        n, batch_size = self.g.n_src, int(batch_size)
        if batch_size < 1:
            raise ValueError(f"DeepWalk.fit: batch_size must be >= 1 (got {batch_size})")
        means = []
        for _ in range(int(epochs)):
            self._epoch += 1
            order = ops.randperm_cpu(n) if shuffle else torch.arange(n)
            total = torch.zeros((), dtype=torch.float32, device=self.g.device)
            nb = 0
            for b, s in enumerate(range(0, n, batch_size)):
                total += self.step(order[s:s + batch_size], *self.seeds(self._epoch, b))
                nb += 1
            means.append(total.item() / max(nb, 1))
        return means


def fill_unseen(g, z, idx_obs):
    """Position rows for nodes that were not embedded (NOSMOG's inductive recipe): a node outside idx_obs gets the mean of z over its
    in-edges from nodes inside idx_obs (a multi-edge counts as often as it is stored), zeros if it has none; rows inside idx_obs are
    returned as they are.  One ops.spmm sum over [z * 1_obs | 1_obs] and a divide.  g on the GPU, z [N, D] on its device."""
    n, d = z.shape
    if n != g.n_src or g.n_dst != g.n_src:
        raise ValueError("fill_unseen: z must have one row per node of the square graph g")
    obs = torch.zeros(n, dtype=torch.bool, device=z.device)
    obs[torch.as_tensor(idx_obs, dtype=torch.int64, device=z.device)] = True
    x = ops.feat_empty(n, d + 1, z.device, zero=True)
    x[:, :d] = z * obs[:, None]
    x[:, d] = obs
    s = ops.spmm(g.indptr, g.indices, x, n, ops.AGG_SUM)
    mean = s[:, :d] / s[:, d:d + 1].clamp(min=1.0)
    return torch.where(obs[:, None], z, mean)
