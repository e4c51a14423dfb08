"""CPU-side checks of the random-walk subgraph training surface (docs/SUBGRAPH_SEMANTICS.md): the command-line flags and their refusals,
train_subgraph's refusals, the C-ABI agreement of the new entry points, their host-side argument checks, and the numpy oracle
(tests/subgraph_oracle.py) against hand answers and against CSRGraph.subgraph on CPU tensors.  No kernel runs here."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import subgraph_oracle as so
from graphgen import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("glnn_random_walk", "glnn_induced_subgraph", "glnn_induced_subgraph_workspace_bytes", "glnn_induced_subgraph_direct")


# ------------------------------------------------------------------------------------------------ flags
def _args(*extra):
    from glnn_amd.cli import get_teacher_args
    return get_teacher_args(["--dataset", "synthetic-cora"] + list(extra))


def test_flag_defaults_are_the_full_graph_step():
    a = _args("--teacher", "GCN")
    assert a.subgraph_walk_length == 0 and a.subgraph_self_loop == "keep"
    a = _args("--teacher", "GAT", "--subgraph_walk_length", "3", "--subgraph_self_loop", "add", "--batch_size", "32")
    assert (a.subgraph_walk_length, a.subgraph_self_loop, a.batch_size) == (3, "add", 32)


@pytest.mark.parametrize("teacher", ["SAGE", "MLP"])
def test_walk_length_refuses_teachers_with_their_own_mini_batches(teacher, capsys):
    with pytest.raises(SystemExit):
        _args("--teacher", teacher, "--subgraph_walk_length", "2")
    err = capsys.readouterr().err
    assert "--subgraph_walk_length" in err and f"--teacher {teacher}" in err


@pytest.mark.parametrize("extra,needle", [(["--subgraph_self_loop", "add"], "needs --subgraph_walk_length"),
                                          (["--subgraph_walk_length", "65"], "[0, 64]"),
                                          (["--subgraph_walk_length", "-1"], "[0, 64]"),
                                          (["--subgraph_walk_length", "2", "--subgraph_self_loop", "both"], "invalid choice")])
def test_flag_refusals(extra, needle, capsys):
    with pytest.raises(SystemExit):
        _args("--teacher", "GCN", *extra)
    assert needle in capsys.readouterr().err


def test_yaml_may_carry_both_keys(tmp_path):
    from glnn_amd.utils import get_training_config
    p = tmp_path / "c.yaml"
    p.write_text("global: {hidden_dim: 64, num_layers: 2}\ncora:\n  GCN: {dropout_ratio: 0, subgraph_walk_length: 2, subgraph_self_loop: add}\n")
    conf = get_training_config(str(p), "GCN", "cora")
    assert conf["subgraph_walk_length"] == 2 and conf["subgraph_self_loop"] == "add"


def test_run_loops_build_a_loader_only_when_asked():
    from glnn_amd import train_and_eval as te
    gcn, sage, mlp = (types.SimpleNamespace(model_name=n) for n in ("GCN", "SAGE", "MLP"))
    assert te._subgraph_loader({}, gcn, None, None) is None
    assert te._subgraph_loader({"subgraph_walk_length": 0}, gcn, None, None) is None
    assert te._subgraph_loader({"subgraph_walk_length": 2}, sage, None, None) is None
    assert te._subgraph_loader({"subgraph_walk_length": 2}, mlp, None, None) is None


# ------------------------------------------------------------------------------------------------ train_subgraph refusals
@pytest.mark.parametrize("name,points_to", [("MLP", "train_mini_batch"), ("SAGE", "train_sage")])
def test_train_subgraph_refuses_mlp_and_sage(name, points_to):
    from glnn_amd.train_and_eval import train_subgraph
    with pytest.raises(NotImplementedError, match=points_to):
        train_subgraph(types.SimpleNamespace(model_name=name), [], None, None, None, None)


def test_full_graph_step_table_follows_train():
    from glnn_amd.train_and_eval import _full_graph_step
    eng = types.SimpleNamespace(**{f"step_{k}": k for k in ("gcnii", "appnp", "gatv2", "gat", "gpr", "gcn")})
    for name, want in (("GCN", "gcn"), ("GCNII", "gcnii"), ("GAT", "gat"), ("GATv2", "gatv2"), ("APPNP", "appnp"), ("GPRGNN", "gpr"),
                       ("GA1GCN", "gcn")):
        assert _full_graph_step(eng, name) == want


def test_loader_refuses_a_cpu_graph():
    from glnn_amd.graph import CSRGraph, RandomWalkSubgraphLoader
    ip, ix = so.six_node_graph()
    g = CSRGraph(torch.from_numpy(ip), torch.from_numpy(ix), 6)
    with pytest.raises(RuntimeError, match="built on the GPU"):
        RandomWalkSubgraphLoader(g, torch.arange(3), 2, 2)


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_entry_points_agree_between_header_binding_and_library():
    from test_capi_symbols import header_functions
    from glnn_amd import _lib
    fns = header_functions()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in fns, f"{name} not declared in include/glnn_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == fns[name], name
        assert hasattr(h, name), f"{name} not exported"
    assert _lib.lib().glnn_abi_version() == _lib.ABI_VERSION == 12          # entry points were only added


def test_host_side_argument_checks():
    from glnn_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(8)          # never dereferenced: every call below is refused (or a no-op) before a launch
    assert h.glnn_random_walk(one, one, one, 4, 0, 1, one, None) == -1 and b"[1,64]" in h.glnn_last_error()
    assert h.glnn_random_walk(one, one, one, 4, 65, 1, one, None) == -1
    assert h.glnn_random_walk(None, None, None, 0, 3, 1, None, None) == 0                      # no roots: no-op
    assert h.glnn_random_walk(None, one, one, 4, 3, 1, one, None) == -1 and b"null pointer" in h.glnn_last_error()
    assert h.glnn_induced_subgraph(one, one, 10, one, 4, 2, 8, one, one, one, one, one, 1 << 20, None) == -1
    assert b"self_loop" in h.glnn_last_error()
    assert h.glnn_induced_subgraph(one, one, 10, one, 4, 0, 8, one, one, one, one, one, 8, None) == -1
    assert b"workspace needs" in h.glnn_last_error()
    assert h.glnn_induced_subgraph(one, one, 10, one, 4, 0, 8, None, one, one, one, one, 1 << 20, None) == -1
    assert h.glnn_induced_subgraph_workspace_bytes(-1, 5) == -1
    # workspace: proportional to the candidate list, whatever the graph's size (hash mode), and no smaller in direct mode
    small, big = h.glnn_induced_subgraph_workspace_bytes(300, 200_000), h.glnn_induced_subgraph_workspace_bytes(300, 2_000_000_000)
    assert small == big and small < 64 * 1024
    assert h.glnn_induced_subgraph_workspace_bytes(300, 2000) == small
    # the two table modes (300 candidates: 1024 slots, two arrays; 5000: 16384 slots)
    assert h.glnn_induced_subgraph_direct(300, 200_000) == 0 and h.glnn_induced_subgraph_direct(300, 2048) == 1
    assert h.glnn_induced_subgraph_direct(300, 2049) == 0 and h.glnn_induced_subgraph_direct(5000, 6000) == 1


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from glnn_amd import GlnnError, ops
    ip, ix = (torch.from_numpy(a) for a in so.six_node_graph())
    with pytest.raises(GlnnError):
        ops.random_walk(ip, ix, torch.arange(3), 2, 1)
    with pytest.raises(GlnnError):
        ops.induced_subgraph(ip, ix, torch.arange(3))


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_hand_answers_on_the_six_node_graph():
    ip, ix = so.six_node_graph()
    nodes, sip, six, zero = so.induced_subgraph(ip, ix, [2, 0, 2, 5, 1], "keep")
    assert nodes.tolist() == [2, 0, 5, 1]                               # first appearance; the repeat of 2 adds nothing
    assert sip.tolist() == [0, 2, 5, 5, 6]
    assert six.tolist() == [0, 3, 3, 3, 0, 1] and six.dtype == np.int32          # self-loop of 2 kept, multi-edge 1 -> 0 kept twice, 4 / 3 outside
    assert zero == 1                                                    # the isolated node's row
    nodes, sip, six, zero = so.induced_subgraph(ip, ix, [2, 0, 2, 5, 1], "add")
    assert nodes.tolist() == [2, 0, 5, 1]
    assert sip.tolist() == [0, 2, 6, 7, 9]
    assert six.tolist() == [3, 0, 3, 3, 0, 1, 2, 1, 3] and zero == 0    # 2's own self-loop dropped, then ONE self entry at the end of every row
    nodes, sip, six, zero = so.induced_subgraph(ip, ix, [], "keep")
    assert len(nodes) == 0 and sip.tolist() == [0] and len(six) == 0 and zero == 0


def test_oracle_walk_hand_answers():
    from oracle.dropout_mask import drop_hash
    ip, ix = so.six_node_graph()
    w = so.random_walk(ip, ix, [5, 4, 3, 0], 3, seed=77)
    assert w.shape == (4, 4) and w.dtype == np.int64
    assert w[0].tolist() == [5, 5, 5, 5] and w[1].tolist() == [4, 4, 4, 4]          # no in-edge: the walk stays
    assert w[2, :2].tolist() == [3, 2]                                   # node 3 has ONE in-edge, from 2: forced whatever the draw
    row2 = [2, 1, 4]
    assert w[2, 2] == row2[(int(drop_hash(77, 2, 2)) * 3) >> 32]           # walk 2, step 2, standing on node 2 (3 in-edges)
    assert w[3, 1] == [1, 1, 2][(int(drop_hash(77, 3, 1)) * 3) >> 32]
    for i in range(4):                                                   # every move follows an in-edge of the node it leaves
        for s in range(1, 4):
            a, b = int(w[i, s - 1]), int(w[i, s])
            assert (b in ix[ip[a]:ip[a + 1]]) or (a == b and ip[a] == ip[a + 1])
    assert not np.array_equal(so.random_walk(ip, ix, [0] * 40, 3, seed=1), so.random_walk(ip, ix, [0] * 40, 3, seed=2))
    assert so.random_walk(ip, ix, [], 3, seed=1).shape == (0, 4)


@pytest.mark.parametrize("which", ["six", "random"])
def test_oracle_keep_equals_csrgraph_subgraph_on_cpu(which):
    from glnn_amd.graph import CSRGraph
    if which == "six":
        ip, ix = so.six_node_graph()
        cands = [[2, 0, 5, 1], [0, 1, 2, 3, 4, 5], [4], [5, 3]]
    else:
        ip, ix = random_graph(600, 6.0, seed=3, isolated=8, hub=700)
        rs = np.random.RandomState(0)
        cands = [rs.permutation(600), rs.choice(600, 150, replace=False), np.arange(600)[::-1].copy()]
    g = CSRGraph(torch.from_numpy(ip), torch.from_numpy(ix), len(ip) - 1)
    for cand in cands:
        nodes, sip, six, zero = so.induced_subgraph(ip, ix, cand, "keep")
        ref = g.subgraph(torch.as_tensor(np.asarray(cand), dtype=torch.int64))
        assert nodes.tolist() == list(np.asarray(cand))
        assert ref.indptr.numpy().tolist() == sip.tolist() and ref.indices.numpy().tolist() == six.tolist()
        assert zero == int((ref.in_degrees() == 0).sum())


def test_oracle_hash_restates_the_table():
    """hash_slot / table_cap restate csrc/frontier_dev.h (lowbias32) and the builder's table size: spot values computed by hand."""
    assert so.table_cap(0) == 64 and so.table_cap(32) == 64 and so.table_cap(33) == 128 and so.table_cap(300) == 1024
    assert so.hash_slot([0], 1024).tolist() == [0]
    x = 1
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
    assert so.hash_slot([1], 1 << 20).tolist() == [x & ((1 << 20) - 1)]
