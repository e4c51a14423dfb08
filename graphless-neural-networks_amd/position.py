"""DeepWalk position features for the MLP student (docs/POSITION_SEMANTICS.md): the device NOSMOG (Tian et al., ICLR 2023) adds to
GLNN -- a DeepWalk embedding of each node concatenated to its features in front of the MLP, so that inference stays one row lookup and an
MLP.  The skip-gram trainer is csrc/deepwalk.hip: node2vec's objective, batch-synchronous lazy Adam, a fixed summation order and no
float atomics (the same seed gives the same bits).  By default p = q = 1, uniform negatives and one table (DeepWalk with negative
sampling); the rest of the node2vec family is behind switches: biased walks (csrc/node2vec.hip), negatives drawn in proportion to
degree^power, and a separate context table.  torch owns the memory and the CPU permutation; there is no CPU path."""
import numpy as np
import torch

from . import ops


def negative_cdf(indices, n_nodes, power):
    """The 32-bit CDF of the negative distribution w_n = out_degree_n ** power (docs/POSITION_SEMANTICS.md), in fp64 numpy on the CPU:
    out_degree_n = how often n occurs in `indices` (proportional to how often an in-edge walk visits n; degree 0 gives weight 0), and
    cdf[n] = min(2^32 - 1, floor(cumsum(w)[n] / sum(w) * 2^32)).  Returns an int64 numpy array [n_nodes] of values in [0, 2^32).  A graph
    whose weights are all zero is refused."""
    deg = np.bincount(np.asarray(indices, np.int64), minlength=int(n_nodes)).astype(np.float64)
    w = np.where(deg > 0, deg ** float(power), 0.0)
    total = w.sum()
    if not total > 0:
        raise ValueError("negative_cdf: every node has weight 0 (a graph without edges has no degree distribution to draw from)")
    return np.minimum(np.floor(np.cumsum(w) / total * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.int64)


class DeepWalk:
    """One embedding table over the nodes of the square graph `g` (on the GPU), trained by skip-gram with negative sampling over the
    windows of random walks along in-edges (glnn_random_walk; glnn_node2vec_walk when (p, q) != (1, 1)).
      .embedding   [N, dim] float32 on g's device; N(0, 1) drawn on the CPU from torch.Generator().manual_seed(seed), so an oracle can
                   start from the same bits
      .step(roots, walk_seed, neg_seed)   one optimiser step over the walks from `roots`; returns the loss as a device scalar
      .fit(epochs, batch_size)            every node a root once per epoch; returns the per-epoch mean loss (one host read per epoch)
    dim % 4 == 0, dim <= 256; 1 <= walk_length <= 64; 2 <= context_size <= walk_length + 1; num_negative >= 1.
    The node2vec switches; with all four at their defaults a step makes exactly the calls it made before they existed:
      p, q              in [0.25, 4]: the return and in-out parameters of the second-order walk
      negative_power    > 0: negatives are drawn in proportion to out_degree ** negative_power (0.75 is word2vec's); 0: uniform
      context_table     True: the entries of a pair are scored against .context [N, dim], N(0, 1) from manual_seed(seed + 1), which has
                        Adam moments of its own; .embedding stays the output"""

    def __init__(self, g, dim, walk_length=20, context_size=10, num_negative=1, lr=0.01, betas=(0.9, 0.999), eps=1e-8, seed=0,
                 p=1.0, q=1.0, negative_power=0.0, context_table=False):
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
        p, q, negative_power = float(p), float(q), float(negative_power)
        if not (0.25 <= p <= 4.0 and 0.25 <= q <= 4.0):
            raise ValueError(f"DeepWalk: p and q must be in [0.25, 4] (got p = {p}, q = {q})")
        if not negative_power >= 0.0:
            raise ValueError(f"DeepWalk: negative_power must be >= 0 (got {negative_power})")
        self.p, self.q, self.negative_power, self.context_table = p, q, negative_power, bool(context_table)
        self.lr, self.betas, self.eps, self.seed = float(lr), (float(betas[0]), float(betas[1])), float(eps), int(seed)
        gen = torch.Generator()
        gen.manual_seed(self.seed)
        self.embedding = torch.randn((g.n_src, dim), generator=gen, dtype=torch.float32).to(g.device)
        self.exp_avg = torch.zeros_like(self.embedding)
        self.exp_avg_sq = torch.zeros_like(self.embedding)
        self.neg_cdf = None     # int32 words of the 32-bit CDF on the device, built once
        if negative_power > 0.0:
            self.neg_cdf = ops.deepwalk_cdf_words(negative_cdf(g.indices.cpu().numpy(), g.n_src, negative_power), g.device)
        self.context = self.context_exp_avg = self.context_exp_avg_sq = None
        if self.context_table:
            gen = torch.Generator()
            gen.manual_seed(self.seed + 1)
            self.context = torch.randn((g.n_src, dim), generator=gen, dtype=torch.float32).to(g.device)
            self.context_exp_avg = torch.zeros_like(self.context)
            self.context_exp_avg_sq = torch.zeros_like(self.context)
            self._no_list = ops.deepwalk_empty_list(g.n_src, g.device)
            self._loss_scratch = torch.empty((), dtype=torch.float32, device=g.device)
        self._plain = p == 1.0 and q == 1.0 and self.neg_cdf is None and not self.context_table
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
        if self._plain:
            _, start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs(g.indptr, g.indices, roots, self.walk_length, c, k, walk_seed, neg_seed)
        else:
            # (at p = q = 1 this is random_walk's step and bits; the entry is used all the same because it checks the roots on the host)
            walks = ops.node2vec_walk(g.indptr, g.indices, roots, self.walk_length, self.p, self.q, walk_seed)
            start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs_from_walks(walks, g.n_src, c, k, neg_seed, self.neg_cdf)
        gr, gs, zs, loss_parts = ops.deepwalk_score(self.embedding, start, rest, c, k, ctx=self.context)
        q, r = rest.shape
        tw = ops.csr_transpose(win_indptr, start, q, g.n_src, q)
        tp_indptr, _, tp_eids = ops.csr_transpose_eids(pair_indptr, rest.view(-1), q, g.n_src, q * r)
        if self.context is None:
            loss = ops.deepwalk_apply(self.embedding, self.exp_avg, self.exp_avg_sq, tw, (tp_indptr, tp_eids), gr, gs, zs, loss_parts, c, k,
                                      self.lr, self.betas, self.eps, self.steps + 1)
        else:
            # two tables: dZ[a] = sum g c_x comes from the windows list alone, dC[x] = sum g z_a from the positions list alone -- the apply
            # launch sums its two lists separately, so each table is one call of it with the other list empty, at the same step count
            loss = ops.deepwalk_apply(self.embedding, self.exp_avg, self.exp_avg_sq, tw, self._no_list, gr, gs, zs, loss_parts, c, k,
                                      self.lr, self.betas, self.eps, self.steps + 1)
            ops.deepwalk_apply(self.context, self.context_exp_avg, self.context_exp_avg_sq, self._no_list, (tp_indptr, tp_eids), gr, gs, zs,
                               loss_parts, c, k, self.lr, self.betas, self.eps, self.steps + 1, loss_out=self._loss_scratch)
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


class PositionTable:
    """The position embedding as a servable artefact (docs/POSITION_SEMANTICS.md, "Serving by node id"): one row per EMBEDDED node.
      .rows        [R, D] float32, the embedding rows
      .node_ids    [R] int64, the node each row belongs to (distinct, inside [0, num_nodes))
      .num_nodes   the N of the graph the table was fitted against
      .slot(n)     int32 [n], node -> its row, -1 for a node without one; n > num_nodes: the nodes that joined the graph later get -1
      .has_unseen  whether any of the num_nodes nodes lacks a row
      .dense(g)    the [N, D] matrix training concatenates: the rows scattered, then fill_unseen over g
      .save(path) / PositionTable.load(path, device)    an .npz of rows, node_ids and num_nodes
    The tensors live on whatever device they were given on; dense() and serving need the GPU."""

    def __init__(self, rows, node_ids, num_nodes):
        rows, node_ids, num_nodes = torch.as_tensor(rows), torch.as_tensor(node_ids), int(num_nodes)
        if rows.dtype != torch.float32 or rows.dim() != 2:
            raise ValueError("PositionTable: rows must be a float32 matrix [R, D]")
        if node_ids.dtype != torch.int64 or node_ids.dim() != 1 or node_ids.numel() != rows.shape[0]:
            raise ValueError("PositionTable: node_ids must be an int64 vector with one entry per row")
        if node_ids.device != rows.device:
            raise ValueError("PositionTable: rows and node_ids must be on one device")
        if node_ids.numel() and (int(node_ids.min()) < 0 or int(node_ids.max()) >= num_nodes):
            raise ValueError(f"PositionTable: node_ids must lie in [0, num_nodes = {num_nodes})")
        if torch.unique(node_ids).numel() != node_ids.numel():
            raise ValueError("PositionTable: node_ids must be distinct")
        self.rows, self.node_ids, self.num_nodes = rows.contiguous(), node_ids.contiguous(), num_nodes
        self._slots = {}

    @classmethod
    def from_deepwalk(cls, dw, idx_obs=None, num_nodes=None):
        """The table of a fitted DeepWalk.  Transductive (idx_obs None): dw was fitted on the whole graph, row n is node n.  Inductive: dw
        was fitted on g.subgraph(idx_obs) of a graph of num_nodes nodes, row i is node idx_obs[i]."""
        z = dw.embedding
        if idx_obs is None:
            return cls(z, torch.arange(z.shape[0], dtype=torch.int64, device=z.device), z.shape[0] if num_nodes is None else num_nodes)
        if num_nodes is None:
            raise ValueError("PositionTable.from_deepwalk: the inductive form needs num_nodes")
        return cls(z, torch.as_tensor(idx_obs, dtype=torch.int64).to(z.device), num_nodes)

    dim = property(lambda self: self.rows.shape[1])
    device = property(lambda self: self.rows.device)
    has_unseen = property(lambda self: self.rows.shape[0] < self.num_nodes)

    def slot(self, n_nodes=None):
        n = self.num_nodes if n_nodes is None else int(n_nodes)
        if n < self.num_nodes:
            raise ValueError(f"PositionTable.slot: n_nodes = {n} is below the {self.num_nodes} nodes the table was fitted against")
        s = self._slots.get(n)
        if s is None:
            s = torch.full((n,), -1, dtype=torch.int32, device=self.device)
            s[self.node_ids] = torch.arange(self.rows.shape[0], dtype=torch.int32, device=self.device)
            self._slots = {n: s}
        return s

    def dense(self, g):
        n = g.num_nodes()
        if n < self.num_nodes:
            raise ValueError(f"PositionTable.dense: the graph has {n} nodes, the table was fitted against {self.num_nodes}")
        full = torch.zeros((n, self.dim), dtype=torch.float32, device=self.device)
        full[self.node_ids] = self.rows
        return fill_unseen(g, full, self.node_ids) if self.rows.shape[0] < n else full

    def to(self, device):
        return self if torch.device(device) == self.device else PositionTable(self.rows.to(device), self.node_ids.to(device), self.num_nodes)

    def save(self, path):
        np.savez(path, rows=self.rows.detach().cpu().numpy(), node_ids=self.node_ids.cpu().numpy(), num_nodes=np.int64(self.num_nodes))

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as f:
            return cls(torch.from_numpy(f["rows"]).to(device), torch.from_numpy(f["node_ids"]).to(device), int(f["num_nodes"]))


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
