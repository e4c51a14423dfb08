"""CPU-side checks of the DeepWalk position features (docs/POSITION_SEMANTICS.md): the numpy oracle (tests/deepwalk_oracle.py) against torch
autograd + torch.optim.SparseAdam in fp64, its pair lists against hand answers, the quality of the embedding it trains (the condition the
GPU functional test rests on), the C-ABI agreement and refusals of the new entry points (no launch: they return before one), and the
student's new command-line flags.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deepwalk_oracle as dwo
from deepwalk_cases import BETAS, EPS, clustered_case, init_embedding, step_seeds
from graphgen import random_graph
from subgraph_oracle import six_node_graph


# ------------------------------------------------------------------------------------------------ oracle against torch
def _torch_loss(emb, start, rest, context):
    za = emb(torch.as_tensor(start))                                   # [Q, d]
    zx = emb(torch.as_tensor(rest))                                    # [Q, R, d]
    s = (za[:, None, :] * zx).sum(dim=2)
    return F.softplus(-s[:, :context - 1]).mean() + F.softplus(s[:, context - 1:]).mean()


@pytest.mark.parametrize("case", ["six", "random"])
def test_oracle_gradient_and_three_steps_equal_torch_sparse_adam_in_fp64(case):
    if case == "six":
        indptr, indices = six_node_graph()
        roots, length, context, negatives = np.array([5, 0, 3, 0, 2]), 4, 3, 2      # (a repeated root; the isolated node 5)
    else:
        indptr, indices = random_graph(60, 4, seed=3, isolated=5)
        roots, length, context, negatives = np.arange(0, 60, 7), 6, 4, 1             # 9 roots: most rows are in no pair
    n, d, lr = len(indptr) - 1, 8, 0.05
    z0 = np.random.default_rng(0).standard_normal((n, d))
    emb = torch.nn.Embedding(n, d, sparse=True).double()
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(z0))
    opt = torch.optim.SparseAdam(emb.parameters(), lr=lr, betas=BETAS, eps=EPS)
    z, m, v = z0.copy(), np.zeros_like(z0), np.zeros_like(z0)

    def rel(a, b):
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)

    for t in (1, 2, 3):
        _, start, rest = dwo.pairs(indptr, indices, roots, length, context, negatives, 100 + t, 200 + t)
        loss, dz, touched = dwo.loss_and_grad(z, start, rest, context, negatives)
        before = emb.weight.detach().numpy().copy()
        opt.zero_grad()
        tl = _torch_loss(emb, start, rest, context)
        tl.backward()
        grad = emb.weight.grad.coalesce()
        assert abs(loss - tl.item()) <= 1e-12 * abs(tl.item())
        assert rel(dz, grad.to_dense().numpy()) <= 1e-12
        # the rows the oracle leaves untouched are exactly the rows SparseAdam leaves untouched
        assert sorted(set(grad.indices()[0].tolist())) == np.flatnonzero(touched).tolist()
        opt.step()
        z_new, m, v = dwo.lazy_adam(z, m, v, dz, touched, lr, BETAS, EPS, t)
        st = opt.state[emb.weight]
        zt = emb.weight.detach().numpy()
        assert rel(z_new, zt) <= 1e-12 and rel(m, st["exp_avg"].numpy()) <= 1e-12 and rel(v, st["exp_avg_sq"].numpy()) <= 1e-12
        assert np.array_equal(zt[~touched], before[~touched]) and np.array_equal(z_new[~touched], z[~touched])
        assert (~touched).any() or case == "six"
        z = z_new


# ------------------------------------------------------------------------------------------------ pairs by hand
def _drop_hash_int(seed, row, col):
    """lowbias32 of csrc/glnn_common.h in plain Python integers (a second restatement, independent of numpy's widths)."""
    M = 0xFFFFFFFF
    h = (seed ^ (row * 0x9E3779B1 & M) ^ ((col * 0x85EBCA77 + 0x632BE5AB) & M)) & M
    h ^= h >> 16; h = h * 0x7FEB352D & M; h ^= h >> 15; h = h * 0x846CA68B & M; h ^= h >> 16
    return h


def test_oracle_pairs_on_the_six_node_graph_by_hand():
    """Rows: 0: [1, 1, 2]  1: [0, 3]  2: [2, 1, 4]  3: [2]  4: []  5: [].  Node 5 is isolated and node 4 has no in-edge: their walks stay put
    and pair the node with itself; node 3's only in-edge comes from 2."""
    indptr, indices = six_node_graph()
    length, context, negatives, neg_seed = 3, 3, 2, 77
    walks, start, rest = dwo.pairs(indptr, indices, [5, 4, 3, 0], length, context, negatives, 11, neg_seed)
    nwin, n_pos = 2, 2
    assert walks.shape == (4, 4) and start.shape == (8,) and rest.shape == (8, 6)
    assert walks[0].tolist() == [5, 5, 5, 5] and walks[1].tolist() == [4, 4, 4, 4] and walks[2, :2].tolist() == [3, 2]
    # windows 0, 1 (walk 0) and 2, 3 (walk 1): start and both positives are the node itself
    assert start[:4].tolist() == [5, 5, 4, 4] and rest[:4, :n_pos].tolist() == [[5, 5], [5, 5], [4, 4], [4, 4]]
    assert start[4] == 3 and rest[4, 0] == 2 and start[5] == 2
    rows = [[1, 1, 2], [0, 3], [2, 1, 4], [2], [], []]
    for i in range(4):
        for s in range(1, length + 1):                     # every step follows an in-edge of the node it stands on, or stays without one
            here = int(walks[i, s - 1])
            assert int(walks[i, s]) in (rows[here] or [here])
        for j in range(nwin):
            q = i * nwin + j
            assert start[q] == walks[i, j] and rest[q, :n_pos].tolist() == walks[i, j + 1:j + 1 + n_pos].tolist()
            for t in range(negatives * n_pos):             # the uniform negatives, kept even where they hit the start or a positive
                assert rest[q, n_pos + t] == (_drop_hash_int(neg_seed, q, t) * 6) >> 32
    assert rest.min() >= 0 and rest.max() < 6


# ------------------------------------------------------------------------------------------------ quality of the oracle alone
def test_oracle_embedding_separates_the_planted_communities():
    """What the GPU functional test rests on: the oracle alone, 100 steps, reaches a nearest-class-centroid accuracy of 0.996-0.998 (measured,
    init seeds 0-3, fp64 and fp32 alike) against the community labels, and its loss falls from 3.44 to 1.03.  Asserted: >= 0.95."""
    indptr, indices, labels, c = clustered_case()
    roots = np.arange(512)
    lists = [dwo.pairs(indptr, indices, roots, c["length"], c["context"], c["negatives"], *step_seeds(s))[1:] for s in range(c["steps"])]
    for dtype in (np.float64, np.float32):
        for seed in range(4):
            z = init_embedding(512, c["d"], seed).astype(dtype)
            m, v = np.zeros_like(z), np.zeros_like(z)
            losses = []
            for s, (start, rest) in enumerate(lists):
                loss, dz, touched = dwo.loss_and_grad(z, start, rest, c["context"], c["negatives"], dtype)
                z, m, v = dwo.lazy_adam(z, m, v, dz, touched, c["lr"], BETAS, EPS, s + 1, dtype)
                losses.append(float(loss))
            acc = dwo.centroid_accuracy(z, labels)
            print(f"{dtype.__name__} seed {seed}: accuracy {acc:.4f}, loss {losses[0]:.3f} -> {losses[-1]:.3f}")
            assert acc >= 0.95, (dtype.__name__, seed, acc)
            assert losses[-1] < 0.5 * losses[0]


# ------------------------------------------------------------------------------------------------ C ABI
NEW = ("glnn_deepwalk_pairs", "glnn_deepwalk_score_f32", "glnn_deepwalk_apply_f32")


def _h():
    from glnn_amd import _lib
    return _lib.lib()


def test_new_entries_are_bound_and_the_abi_version_is_unchanged():
    from glnn_amd import _lib
    h = _h()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.glnn_abi_version() == 12


def _pairs_rc(h, n_nodes=6, n_roots=4, length=4, context=3, negatives=1, roots_host=None):
    return h.glnn_deepwalk_pairs(None, None, n_nodes, None, roots_host, n_roots, length, context, negatives, 1, 2, None, None, None, None, None, None)


def _score_rc(h, n_nodes=6, d=8, q=4, context=3, negatives=1):
    return h.glnn_deepwalk_score_f32(None, n_nodes, d, None, None, q, context, negatives, None, None, None, None, None)


def _apply_rc(h, n_nodes=6, d=8, q=4, context=3, negatives=1, step=1):
    return h.glnn_deepwalk_apply_f32(None, None, None, None, n_nodes, d, q, context, negatives, None, None, None, None, None, None, 0.01, 0.9,
                                     0.999, 1e-8, step, None, None, None)


@pytest.mark.parametrize("kw, needle", [
    (dict(context=1), b"context size"), (dict(context=6), b"context size"), (dict(negatives=0), b"negatives per positive"),
    (dict(length=0), b"walk length"), (dict(length=65), b"walk length"), (dict(n_nodes=2 ** 31), b"N < 2^31"),
    (dict(n_roots=2 ** 26, length=64, context=2, negatives=1), b"Q R < 2^31"), (dict(n_roots=2 ** 20, length=4, negatives=2 ** 20), b"Q R < 2^31"),
])
def test_pairs_refuses_bad_shapes_before_any_pointer_is_used(kw, needle):
    h = _h()
    assert _pairs_rc(h, **kw) == -1 and needle in h.glnn_last_error()


def test_pairs_refuses_a_root_outside_the_graph():
    h = _h()
    bad = (ctypes.c_int64 * 4)(0, 5, 6, 1)
    one = ctypes.c_int64(0)
    ptr = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)       # non-NULL stand-ins: the refusal comes before any of them is used
    rc = h.glnn_deepwalk_pairs(ptr, ptr, 6, ptr, ctypes.cast(bad, ctypes.c_void_p), 4, 4, 3, 1, 1, 2, ptr, ptr, ptr, ptr, ptr, None)
    assert rc == -1 and b"root 6 (position 2) is outside the graph of 6 nodes" in h.glnn_last_error()
    bad[2] = -1
    rc = h.glnn_deepwalk_pairs(ptr, ptr, 6, ptr, ctypes.cast(bad, ctypes.c_void_p), 4, 4, 3, 1, 1, 2, ptr, ptr, ptr, ptr, ptr, None)
    assert rc == -1 and b"root -1" in h.glnn_last_error()


@pytest.mark.parametrize("call", [_score_rc, _apply_rc])
@pytest.mark.parametrize("kw, needle", [
    (dict(d=6), b"multiple of 4"), (dict(d=0), b"multiple of 4"), (dict(d=260), b"multiple of 4"), (dict(context=1), b"context size"),
    (dict(negatives=0), b"negatives per positive"), (dict(n_nodes=2 ** 31), b"N < 2^31"), (dict(q=2 ** 30, context=3), b"Q R < 2^31"),
])
def test_score_and_apply_refuse_bad_shapes_before_any_pointer_is_used(call, kw, needle):
    h = _h()
    assert call(h, **kw) == -1 and needle in h.glnn_last_error()


def test_empty_batches_are_no_ops_and_null_pointers_are_reported():
    h = _h()
    assert _score_rc(h, q=0) == 0 and _apply_rc(h, q=0) == 0
    assert _score_rc(h) == -1 and b"null pointer" in h.glnn_last_error()
    assert _apply_rc(h) == -1 and b"null pointer" in h.glnn_last_error()
    assert _apply_rc(h, step=0) == -1 and b"step >= 1" in h.glnn_last_error()
    assert _pairs_rc(h) == -1 and b"null pointer" in h.glnn_last_error()


def test_wrappers_refuse_cpu_tensors_and_the_class_checks_its_arguments():
    from glnn_amd import GlnnError, ops
    from glnn_amd.graph import CSRGraph
    from glnn_amd.position import DeepWalk
    indptr, indices = six_node_graph()
    with pytest.raises(GlnnError):
        ops.deepwalk_pairs(torch.from_numpy(indptr), torch.from_numpy(indices), torch.arange(3), 4, 3, 1, 1, 2)
    with pytest.raises(GlnnError):
        ops.deepwalk_score(torch.zeros(6, 8), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32), 3, 1)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        DeepWalk(CSRGraph(torch.from_numpy(indptr), torch.from_numpy(indices), 6), 8)
    assert ops.deepwalk_windows(7, 10, 5, 2) == (49, 12)


# ------------------------------------------------------------------------------------------------ flags
def _args(*extra):
    from glnn_amd.cli import get_student_args
    return get_student_args(["--dataset", "synthetic-cora"] + list(extra))


def test_position_flags_default_to_off():
    a = _args()
    assert a.position_dim == 0
    a = _args("--position_dim", "16", "--position_walk_length", "8", "--position_context", "4", "--position_negatives", "2",
              "--position_epochs", "3", "--position_batch_size", "256", "--position_lr", "0.05")
    assert (a.position_dim, a.position_walk_length, a.position_context, a.position_negatives, a.position_epochs, a.position_batch_size,
            a.position_lr) == (16, 8, 4, 2, 3, 256, 0.05)


@pytest.mark.parametrize("extra", [("--position_dim", "6"), ("--position_dim", "260"), ("--position_dim", "-4"),
                                   ("--position_dim", "8", "--position_walk_length", "65"),
                                   ("--position_dim", "8", "--position_walk_length", "4", "--position_context", "6"),
                                   ("--position_dim", "8", "--position_negatives", "0")])
def test_position_flags_are_checked_by_the_parser(extra):
    with pytest.raises(SystemExit):
        _args(*extra)
