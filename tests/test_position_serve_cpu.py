"""CPU-side checks of serving a position-feature student by node id (docs/POSITION_SEMANTICS.md, "Serving by node id"): the C entry is
exported, bound and refuses what it must before anything is launched (null device pointers throughout); the numpy oracle is held to hand
answers and to position.fill_unseen's formula; PositionTable round-trips through its .npz; serve_student.py parses and refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import graphgen
import position_serve_oracle as pso
from subgraph_oracle import six_node_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1


def _header_arg_count(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glnn_hip.h")).read(), flags=re.S)
    m = re.search(r"GLNN_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return len(m.group(1).split(","))


def _h():
    from glnn_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ the entry
def test_the_entry_is_exported_bound_and_the_abi_version_stays():
    from glnn_amd import _lib
    h = _h()
    assert hasattr(h, "glnn_position_rows")
    assert len(_lib.SIGNATURES["glnn_position_rows"]) == _header_arg_count("glnn_position_rows") == 18
    assert h.glnn_abi_version() == 12 and _lib.ABI_VERSION == 12


_PTR = ctypes.c_void_p(4096)          # a non-NULL, 16-byte aligned stand-in: every call below is refused before a pointer is used


def _rc(h, m=4, ldx=16, x_dtype=F32, f=10, ldz=8, d=8, z_rows=5, n_nodes=6, ldo=20, out_dtype=F32, ids=None, x=None, z=None, slot=None,
        indptr=None, indices=None, out=None):
    return h.glnn_position_rows(ids, m, x, ldx, x_dtype, f, z, ldz, d, z_rows, slot, n_nodes, indptr, indices, out, ldo, out_dtype, None)


@pytest.mark.parametrize("kw, status, needle", [
    (dict(), -1, b"null pointer"),                                                                  # m > 0 and no pointer at all
    (dict(ids=_PTR, x=_PTR, z=_PTR, slot=_PTR), -1, b"null pointer"),                               # ... or out alone missing
    (dict(x=_PTR, z=_PTR, slot=_PTR, out=_PTR), -1, b"null pointer"),                               # ... or ids
    (dict(m=-1), -1, b"m must be"),
    (dict(f=0), -1, b"f must be"),
    (dict(d=0), -1, b"d must be"), (dict(d=6), -1, b"d must be"), (dict(d=260, ldz=260, ldo=272), -1, b"d must be"),
    (dict(ldz=4), -1, b"ldz"), (dict(ldz=10), -1, b"ldz"),
    (dict(ldo=16), -1, b"ldo"), (dict(ldo=22), -1, b"ldo"),                                         # fp32: f + d = 18 -> 20
    (dict(out_dtype=BF16, ldo=20), -1, b"ldo"), (dict(out_dtype=BF16, ldo=16), -1, b"ldo"),         # bf16: 18 -> 24
    (dict(ldx=9), -1, b"ldx"),
    (dict(x_dtype=BF16, out_dtype=BF16, ldo=24, ldx=12), -1, b"bf16 ldx"),
    (dict(x_dtype=2), -1, b"unknown x_dtype"), (dict(out_dtype=-1), -1, b"unknown out_dtype"),
    (dict(x_dtype=BF16, out_dtype=F32), -2, b"bf16 features"),
    (dict(indptr=_PTR), -1, b"indptr and indices"), (dict(indices=_PTR), -1, b"indptr and indices"),
    (dict(n_nodes=2 ** 31), -1, b"n_nodes"), (dict(z_rows=2 ** 31), -1, b"z_rows"),
    (dict(ids=_PTR, x=_PTR, z=ctypes.c_void_p(4100), slot=_PTR, out=_PTR), -1, b"16-byte aligned"),
    (dict(ids=_PTR, x=_PTR, z=_PTR, slot=_PTR, out=ctypes.c_void_p(4104)), -1, b"16-byte aligned"),
])
def test_every_refusal_names_the_entry_and_launches_nothing(kw, status, needle):
    h = _h()
    assert _rc(h, **kw) == status
    msg = h.glnn_last_error()
    assert b"glnn_position_rows" in msg and needle in msg, msg


def test_an_empty_batch_is_a_no_op_that_reads_no_pointer():
    assert _rc(_h(), m=0) == 0


def test_the_wrapper_refuses_cpu_tensors():
    from glnn_amd import GlnnError, ops
    with pytest.raises(GlnnError):
        ops.position_rows(torch.arange(3), torch.zeros(6, 10), torch.zeros(5, 8), torch.zeros(6, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_against_hand_answers_on_the_six_node_graph():
    """rows: 0: [1, 1, 2]   1: [0, 3]   2: [2, 1, 4]   3: [2]   4: []   5: [];  embedded: 1 -> row 0, 2 -> row 1, 3 -> row 2."""
    indptr, indices = six_node_graph()
    x = np.arange(12, dtype=np.float64).reshape(6, 2)
    z = np.array([[1.0, -2.0, 4.0, 8.0], [3.0, 6.0, -4.0, 0.0], [100.0, 100.0, 100.0, 100.0]])
    slot = np.array([-1, 0, 1, 2, -1, -1])
    out, count, mean_abs = pso.rows([1, 0, 4, 2, 5], x, z, slot, indptr, indices)
    assert out.shape == (5, 6) and np.array_equal(out[:, :2], x[[1, 0, 4, 2, 5]])
    assert np.array_equal(out[0, 2:], z[0]) and count[0] == 0                                        # a seen node: its own row
    assert np.array_equal(out[1, 2:], (2 * z[0] + z[1]) / 3) and count[1] == 3                       # unseen: the multi-edge counts twice
    assert np.array_equal(mean_abs[1], (2 * np.abs(z[0]) + np.abs(z[1])) / 3)
    assert np.array_equal(out[2, 2:], np.zeros(4)) and count[2] == 0 and not mean_abs[2].any()       # unseen, no in-edge at all
    assert np.array_equal(out[3, 2:], z[1])
    assert np.array_equal(out[4, 2:], np.zeros(4)) and count[4] == 0
    # an unseen node with exactly two embedded in-neighbours, and one whose only in-neighbours are unseen
    slot = np.array([0, -1, -1, 1, -1, -1])
    out, count, _ = pso.rows([1, 2], x, z, slot, indptr, indices)
    assert np.array_equal(out[0, 2:], (z[0] + z[1]) / 2) and count[0] == 2                           # row 1: [0, 3], both embedded
    assert np.array_equal(out[1, 2:], np.zeros(4)) and count[1] == 0                                 # row 2: [2, 1, 4], none embedded
    # without a graph an unseen row is zeros; a slot outside the table and an entry outside the graph count for nothing
    assert not pso.rows([1], x, z, slot)[0][0, 2:].any()
    out, count, _ = pso.rows([0], x, z, np.array([-1, 0, 7, 2, -1, -1]), indptr, np.array([1, 1, 9, 0, 3, 2, 1, 4, 2], np.int32))
    assert np.array_equal(out[0, 2:], z[0]) and count[0] == 2


def test_oracle_position_columns_are_fill_unseen_restated_in_numpy():
    n, d = 300, 12
    indptr, indices = graphgen.random_graph(n, 5.0, 11, isolated=3, hub=150)
    rs = np.random.RandomState(3)
    z_full = rs.standard_normal((n, d))
    obs = rs.rand(n) < 0.7
    idx_obs = np.nonzero(obs)[0]
    # position.fill_unseen: s = A [z 1_obs | 1_obs], mean = s[:, :d] / max(s[:, d], 1), where(obs, z, mean)
    xa = np.concatenate([z_full * obs[:, None], obs[:, None].astype(np.float64)], axis=1)
    dst = np.repeat(np.arange(n), np.diff(indptr))
    s = np.zeros((n, d + 1))
    np.add.at(s, dst, xa[indices])
    want = np.where(obs[:, None], z_full, s[:, :d] / np.maximum(s[:, d:d + 1], 1.0))
    slot = np.full(n, -1, np.int64)
    slot[idx_obs] = np.arange(len(idx_obs))
    out, count, _ = pso.rows(np.arange(n), np.zeros((n, 1)), z_full[idx_obs], slot, indptr, indices)
    np.testing.assert_allclose(out[:, 1:], want, rtol=0, atol=1e-13)
    assert np.array_equal(count, np.where(obs, 0, s[:, d]).astype(np.int64))
    assert (count[~obs] == 0).any() and (count > 1).any()


# ------------------------------------------------------------------------------------------------ the table
def test_position_table_round_trip_and_slots(tmp_path):
    from glnn_amd.position import PositionTable
    rs = np.random.RandomState(0)
    rows = torch.from_numpy(rs.standard_normal((4, 8)).astype(np.float32))
    ids = torch.tensor([5, 0, 3, 2])
    t = PositionTable(rows, ids, 7)
    assert t.has_unseen and t.dim == 8
    assert t.slot().dtype == torch.int32 and t.slot().tolist() == [1, -1, 3, 2, -1, 0, -1]
    assert t.slot(9).tolist() == [1, -1, 3, 2, -1, 0, -1, -1, -1]            # nodes that joined the graph later have no row
    with pytest.raises(ValueError):
        t.slot(6)
    t.save(tmp_path / "position.npz")
    with np.load(tmp_path / "position.npz") as f:
        assert sorted(f.files) == ["node_ids", "num_nodes", "rows"]
    u = PositionTable.load(tmp_path / "position.npz", "cpu")
    assert torch.equal(u.rows, rows) and torch.equal(u.node_ids, ids) and u.num_nodes == 7
    assert torch.equal(u.slot(), t.slot()) and torch.equal(u.slot(9), t.slot(9))
    full = PositionTable(rows, torch.arange(4), 4)
    assert not full.has_unseen and full.slot().tolist() == [0, 1, 2, 3]
    for bad in ((rows, torch.tensor([0, 1, 2, 7]), 7), (rows, torch.tensor([0, 1, 1, 2]), 7), (rows.double(), ids, 7), (rows, ids[:3], 7)):
        with pytest.raises(ValueError):
            PositionTable(*bad)


# ------------------------------------------------------------------------------------------------ serve_student.py
def _args(*extra):
    from glnn_amd.cli import get_serve_args
    return get_serve_args(["--dataset", "synthetic-cora"] + list(extra))


def test_serve_flags_are_parsed():
    a = _args()
    assert (a.position_dim, a.serve_dtype, a.nodes, a.exp_setting, a.teacher, a.student) == (0, "float32", None, "tran", "SAGE", "MLP")
    a = _args("--teacher", "GCN", "--student", "MLP", "--exp_setting", "ind", "--split_rate", "0.3", "--seed", "2", "--position_dim", "16",
              "--device", "0", "--serve_dtype", "bfloat16", "--output_path", "o", "--nodes", "ids.npy")
    assert (a.teacher, a.exp_setting, a.split_rate, a.seed, a.position_dim, a.device, a.serve_dtype, a.output_path, a.nodes) == \
        ("GCN", "ind", 0.3, 2, 16, 0, "bfloat16", "o", "ids.npy")


@pytest.mark.parametrize("extra, needle", [(("--feature_aug_k", "1"), "--feature_aug_k"), (("--feature_noise", "0.1"), "--feature_noise"),
                                           (("--position_dim", "6"), "--position_dim"), (("--serve_dtype", "float16"), "--serve_dtype")])
def test_serve_flags_are_checked_by_the_parser(extra, needle, capsys):
    with pytest.raises(SystemExit):
        _args(*extra)
    assert needle in capsys.readouterr().err


def test_serve_refuses_a_run_without_its_artefacts(tmp_path, monkeypatch):
    """The check comes before the device is asked for: a directory without position.npz (a plain run, or one without --save_results) is
    refused by name."""
    from glnn_amd.cli import run_serve
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match="no position.npz"):
        run_serve(_args("--position_dim", "16", "--device", "0"))
    d = tmp_path / "outputs" / "transductive" / "synthetic-cora" / "SAGE_PE16MLP" / "seed_0"
    os.makedirs(d)
    (d / "position.npz").write_bytes(b"")
    with pytest.raises(SystemExit, match="no model.pth"):
        run_serve(_args("--position_dim", "16", "--device", "0"))
