"""Host side of neighbour-sampled SAGE inference (no GPU needed): the C entries, their bindings and the refusals made before any launch,
the per-layer seed, the refusals of SAGE.inference / Model.inference(fan_out=...), the conf key and the teacher command line's
--inference_fan_out, and the test graphs' own premises (tests/sampled_inference_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sampled_inference_cases as sc
from oracle.dropout_mask import drop_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("glnn_sample_csr_workspace_bytes", "glnn_sample_csr_indptr", "glnn_sample_csr_fill")


def test_sample_csr_entries_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    from glnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "glnn_hip.h")).read()
    h = ctypes.CDLL(ge.build())
    for name in NEW_ENTRIES:
        assert re.search(r"GLNN_API\s+\w+\s+" + name + r"\s*\(", header), name
        assert hasattr(h, name) and name in _lib.SIGNATURES, name
    h.glnn_abi_version.restype = ctypes.c_int
    assert h.glnn_abi_version() == 12           # entries added, none changed: the version stands


def test_sample_csr_entries_report_invalid_arguments():
    from glnn_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(8)                    # a non-null pointer that is never dereferenced: every call below is refused first
    for fanout in (0, 65, -1):
        assert h.glnn_sample_csr_indptr(one, 4, fanout, one, one, 64, None) == -1
        assert b"glnn_sample_csr_indptr: fanout" in h.glnn_last_error()
        assert h.glnn_sample_csr_fill(one, one, 4, 4, one, fanout, 0, one, None) == -1
        assert b"glnn_sample_csr_fill: fanout" in h.glnn_last_error()
    assert h.glnn_sample_csr_indptr(None, 4, 5, one, one, 64, None) == -1 and b"glnn_sample_csr_indptr: null pointer" in h.glnn_last_error()
    assert h.glnn_sample_csr_indptr(one, 4, 5, None, one, 64, None) == -1 and b"glnn_sample_csr_indptr: null pointer" in h.glnn_last_error()
    assert h.glnn_sample_csr_indptr(one, 4, 5, one, None, 64, None) == -1 and b"glnn_sample_csr_indptr: null pointer" in h.glnn_last_error()
    assert h.glnn_sample_csr_indptr(one, 4, 5, one, one, 8, None) == -1 and b"glnn_sample_csr_indptr: workspace" in h.glnn_last_error()
    assert h.glnn_sample_csr_indptr(one, 1 << 31, 5, one, one, 1 << 30, None) == -1 and b"glnn_sample_csr_indptr: n_dst" in h.glnn_last_error()
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert h.glnn_sample_csr_fill(args[0], args[1], 4, 4, args[2], 5, 0, args[3], None) == -1
        assert b"glnn_sample_csr_fill: null pointer" in h.glnn_last_error()
    assert h.glnn_sample_csr_fill(one, one, 4, 1 << 31, one, 5, 0, one, None) == -1 and b"glnn_sample_csr_fill: n_dst and n_src" in h.glnn_last_error()
    assert h.glnn_sample_csr_fill(None, None, 0, 0, None, 5, 0, None, None) == 0          # no rows: nothing to do
    h.glnn_sample_csr_workspace_bytes.restype = ctypes.c_int64
    assert [h.glnn_sample_csr_workspace_bytes(n) for n in (0, 1, 1024, 1025)] == [8, 16, 16, 24]


def test_ops_and_graph_refuse_before_any_launch():
    from glnn_amd import GlnnError, ops
    from glnn_amd.graph import CSRGraph
    ip, ix = torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(GlnnError):
        ops.sample_csr_indptr(ip, 4, 5)
    with pytest.raises(GlnnError):
        ops.sample_csr_fill(ip, ix, 4, 4, ip, 0, 5, 0)
    g = CSRGraph(ip, ix[:0], 4)
    for bad in (0, 65, 2.0, "5", True, None):
        with pytest.raises(ValueError, match="fanout"):
            g.sampled(bad, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        g.sampled(5, 0)


def test_layer_seed_restated():
    """seed_l = drop_hash(sample_seed, l, 0xFA17): the package's host restatement against oracle/dropout_mask.py's, and one value worked
    out by hand from csrc/glnn_common.h (seed 0, layer 0)."""
    from glnn_amd.models import SAMPLE_SEED_SALT, drop_hash as host_hash, sample_layer_seed
    assert SAMPLE_SEED_SALT == 0xFA17 == sc.SEED_SALT
    for seed in (0, 1, 7, 20240, 0xFFFFFFFF, 1 << 40):
        for l in range(8):
            assert sample_layer_seed(seed, l) == int(drop_hash(seed, l, 0xFA17)) == sc.layer_seed(seed, l)
    rs = np.random.RandomState(0)
    for seed, row, col in rs.randint(0, 1 << 31, size=(50, 3)):
        assert host_hash(seed, row, col) == int(drop_hash(seed, row, col))
    m = 0xFFFFFFFF
    h = (0 ^ 0 ^ ((0xFA17 * 0x85EBCA77 + 0x632BE5AB) & m)) & m
    h ^= h >> 16
    h = h * 0x7FEB352D & m
    h ^= h >> 15
    h = h * 0x846CA68B & m
    h ^= h >> 16
    assert sample_layer_seed(0, 0) == h
    assert len({sample_layer_seed(3, l) for l in range(8)}) == 8          # the layers draw under different seeds


def test_the_test_graphs_hold_their_premises():
    ip, ix = sc.big_graph()
    deg = np.diff(ip)
    assert len(ip) == sc.N + 1 and deg[sc.HUB] == 3000 and deg[sc.LONG] == 130
    for f in sc.FANOUTS:
        assert deg[sc.PLANTED[f]] == f and deg[sc.PLANTED[f + 1]] == f + 1
        for seed in sc.SEEDS:
            sp, sx, n_redirects = sc.expected("big", f, seed)
            assert (np.diff(sp) == np.minimum(deg, f)).all() and len(sx) == sp[-1]
            assert n_redirects >= 1 or f < 5, (f, seed)
    assert list(ix[ip[5]:ip[6]]).count(7) >= 3 and 10 in ix[ip[10]:ip[11]]          # multi-edges, the self-loop
    sip, six = sc.small_degree_graph()
    assert np.diff(sip).max() == 64
    for seed in sc.SEEDS:                                                           # a fan-out at the largest degree keeps the graph
        sp, sx, _ = sc.expected("small", 64, seed)
        assert np.array_equal(sp, sip) and np.array_equal(sx, six)


class _Loader:
    def __init__(self, graph):
        if graph is not None:
            self.graph = graph


def _sage(aggregator="gcn", num_layers=2):
    from glnn_amd.models import Model
    return Model(dict(model_name="SAGE", num_layers=num_layers, feat_dim=8, hidden_dim=16, label_dim=3, dropout_ratio=0.0, norm_type="none",
                      device="cpu", sage_aggregator=aggregator)).eval()


@pytest.mark.parametrize("aggregator", ["gcn", "mean"])
def test_sage_inference_refusals_name_fan_out(aggregator):
    """Every refusal comes before the first launch, so it is raised for CPU tensors too."""
    model = _sage(aggregator)
    x = torch.zeros(4, 8)
    loader = _Loader(object())
    for bad in ([5], [5, 5, 5], [], 5, "5,5", 5.5):
        with pytest.raises(ValueError, match="fan_out"):
            model.encoder.inference(loader, x, fan_out=bad)
    for bad in ([5, 0], [65, 5], [5, -1], [5, 2.0], [5, "5"], [True, 5]):
        with pytest.raises(ValueError, match="fan_out"):
            model.inference(loader, x, fan_out=bad)
    with pytest.raises(NotImplementedError, match="fan_out"):
        model.encoder.inference(loader, x, whole_graph=False, fan_out=[5, 5])
    with pytest.raises(NotImplementedError, match="fan_out"):
        model.inference(_Loader(None), x, fan_out=[5, 5])
    # a valid request reaches the device check (and no further) on a machine without one
    from glnn_amd import GlnnError
    with pytest.raises(GlnnError):
        model.inference(loader, x, fan_out=[5, 5])


@pytest.mark.parametrize("name", ["GCN", "APPNP", "GAT", "MLP", "GCNII"])
def test_model_inference_refuses_fan_out_for_other_teachers(name):
    from glnn_amd.models import Model
    conf = dict(model_name=name, num_layers=2, feat_dim=8, hidden_dim=16, label_dim=3, dropout_ratio=0.0, norm_type="none", device="cpu",
                num_heads=8, attn_dropout_ratio=0.0)
    m = Model(conf).eval()
    with pytest.raises(NotImplementedError, match="fan_out"):
        m.inference(None, torch.zeros(4, 8), fan_out=[5, 5])


def test_evaluate_passes_the_keywords_through():
    from glnn_amd import train_and_eval as te

    class Fake:
        def __init__(self):
            self.calls = []

        def eval(self):
            pass

        def inference(self, data, feats, **kw):
            self.calls.append(kw)
            raise KeyboardInterrupt          # (what follows needs the device)

    fake = Fake()
    for kw in ({}, dict(fan_out=[5, 5], sample_seed=3), dict(dtype=torch.bfloat16, fan_out=[4, 2]), dict(sample_seed=9)):
        with pytest.raises(KeyboardInterrupt):
            te.evaluate(fake, None, None, None, None, None, **kw)
    assert fake.calls == [{}, dict(fan_out=[5, 5], sample_seed=3), dict(dtype=torch.bfloat16, fan_out=[4, 2], sample_seed=0), {}]
    assert te.inference_fan_out({}) is None and te.inference_fan_out({"inference_fan_out": ""}) is None
    assert te.inference_fan_out({"inference_fan_out": None}) is None
    assert te.inference_fan_out({"inference_fan_out": "15,10"}) == [15, 10]
    assert te.inference_fan_out({"inference_fan_out": [15, 10]}) == [15, 10]
    with pytest.raises(ValueError, match="inference_fan_out"):
        te.inference_fan_out({"inference_fan_out": "15,x"})


def test_teacher_cli_inference_fan_out():
    from glnn_amd.cli import get_student_args, get_teacher_args
    from glnn_amd.train_and_eval import inference_fan_out
    assert get_teacher_args([]).inference_fan_out == ""
    assert inference_fan_out(vars(get_teacher_args([]))) is None
    args = get_teacher_args(["--teacher", "SAGE", "--inference_fan_out", "15,15"])
    assert args.inference_fan_out == "15,15" and inference_fan_out(vars(args)) == [15, 15]
    args = get_teacher_args(["--teacher", "SAGE", "--num_layers", "3", "--inference_fan_out", "1,64,33", "--sage_aggregator", "mean"])
    assert inference_fan_out(vars(args)) == [1, 64, 33]
    for argv in (["--teacher", "GCN", "--inference_fan_out", "5,5"],              # not SAGE
                 ["--teacher", "MLP", "--inference_fan_out", "5,5"],
                 ["--teacher", "SAGE", "--inference_fan_out", "5"],                # length != --num_layers (2)
                 ["--teacher", "SAGE", "--inference_fan_out", "5,5,5"],
                 ["--teacher", "SAGE", "--num_layers", "3", "--inference_fan_out", "5,5"],
                 ["--teacher", "SAGE", "--inference_fan_out", "0,5"],              # outside [1, 64]
                 ["--teacher", "SAGE", "--inference_fan_out", "5,65"],
                 ["--teacher", "SAGE", "--inference_fan_out", "5,-1"],
                 ["--teacher", "SAGE", "--inference_fan_out", "5,x"],              # not integers
                 ["--teacher", "SAGE", "--inference_fan_out", "5.0,5"]):
        with pytest.raises(SystemExit):
            get_teacher_args(argv)
    with pytest.raises(SystemExit):
        get_student_args(["--inference_fan_out", "5,5"])
