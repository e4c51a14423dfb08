"""CPU checks of the native SAGE "mean" training step (csrc/sage_mean_step.hip, TeacherEngine.step_sage_mean): the masked oracle of
tests/sage_mean_step_oracle.py against finite differences and against the plain oracle, the two new exports and the descriptor mirror,
the argument checks of the C entries (no launch is made here), the engine's gates and the CLI flag."""
import ctypes

import numpy as np
import pytest
import torch

import sage_mean_oracle as mo
import sage_mean_step_oracle as so
from graphgen import csr_from_edges

DIMS = (5, 6, 3)


def _state(norm, seed=0):
    rs = np.random.RandomState(seed)
    sd = {}
    for l in range(2):
        for fc in ("fc_self", "fc_neigh"):
            sd[f"encoder.layers.{l}.{fc}.weight"] = rs.standard_normal((DIMS[l + 1], DIMS[l])) * 0.5
            sd[f"encoder.layers.{l}.{fc}.bias"] = rs.standard_normal(DIMS[l + 1]) * 0.1
    if norm != "none":
        sd["encoder.norms.0.weight"] = rs.uniform(0.5, 1.5, DIMS[1])
        sd["encoder.norms.0.bias"] = rs.uniform(-0.2, 0.2, DIMS[1])
        if norm == "batch":
            sd["encoder.norms.0.running_mean"] = np.zeros(DIMS[1])
            sd["encoder.norms.0.running_var"] = np.ones(DIMS[1])
    return sd


def _blocks():
    """A 2-layer block pair, n_dst < n_src in both.  Block 1 (9 sources, 4 destinations) has an isolated destination (3), a duplicate edge
    (2 -> 1 twice), a self-loop (2 -> 2) and sources that are no destinations; block 0 (14 sources, 9 destinations) is random with
    destination 1 isolated."""
    rs = np.random.RandomState(5)
    src, dst = rs.randint(0, 14, 27), rs.randint(0, 9, 27)
    keep = dst != 1
    b0 = csr_from_edges(src[keep], dst[keep], 9) + (14,)
    b1 = csr_from_edges(np.array([1, 0, 2, 2, 2, 5, 8]), np.array([0, 1, 1, 1, 2, 2, 0]), 4) + (9,)
    assert np.diff(b1[0])[3] == 0
    return [b0, b1]


@pytest.mark.parametrize("norm", ["none", "batch", "layer"])
def test_masked_oracle_gradients_match_finite_differences(norm):
    sd = _state(norm)
    blocks = _blocks()
    rs = np.random.RandomState(7)
    x = rs.standard_normal((14, DIMS[0]))
    labels = rs.randint(0, DIMS[2], 4)
    p = 0.5
    masks = [(rs.uniform(size=(9, DIMS[1])) >= p).astype(np.uint8)]
    assert 0 < masks[0].mean() < 1

    def loss_of(sd_, x_):
        st_ = mo.State(sd_, 2, norm)
        return mo.loss_and_dlogits(so.forward(st_, blocks, x_, masks, p)[0], labels)[0]

    st = mo.State(sd, 2, norm)
    logits, cache = so.forward(st, blocks, x, masks, p)
    grads, dx = so.backward(st, cache, mo.loss_and_dlogits(logits, labels)[1])
    assert set(grads) == set(st.names())
    eps = 1e-6
    for k in st.names():
        for i in rs.choice(sd[k].size, size=min(4, sd[k].size), replace=False):
            up, dn = {q: v.copy() for q, v in sd.items()}, {q: v.copy() for q, v in sd.items()}
            up[k].flat[i] += eps
            dn[k].flat[i] -= eps
            fd = (loss_of(up, x) - loss_of(dn, x)) / (2 * eps)
            assert abs(fd - grads[k].flat[i]) < 1e-6 + 1e-5 * abs(fd), (k, i, fd, grads[k].flat[i])
    for i in rs.choice(x.size, size=6, replace=False):
        up, dn = x.copy(), x.copy()
        up.flat[i] += eps
        dn.flat[i] -= eps
        fd = (loss_of(sd, up) - loss_of(sd, dn)) / (2 * eps)
        assert abs(fd - dx.flat[i]) < 1e-6 + 1e-5 * abs(fd), (i, fd, dx.flat[i])


@pytest.mark.parametrize("norm", ["none", "batch", "layer"])
def test_all_ones_masks_are_the_plain_oracle(norm):
    blocks = _blocks()
    rs = np.random.RandomState(9)
    x = rs.standard_normal((14, DIMS[0]))
    labels = rs.randint(0, DIMS[2], 4)
    a, b = mo.State(_state(norm), 2, norm), mo.State(_state(norm), 2, norm)
    for _ in range(2):
        la, ga, dxa = mo.step(a, blocks, x, labels, 1e-2, 5e-4)
        lb, gb, dxb = so.step(b, blocks, x, labels, 1e-2, [np.ones((9, DIMS[1]), np.uint8)], 0.0, 5e-4)
        assert la == lb and np.array_equal(dxa, dxb)
        for k in ga:
            assert np.array_equal(ga[k], gb[k]), k
    for k in a.p:
        assert np.array_equal(a.p[k], b.p[k]), k


def test_library_exports_the_step_entries_and_the_descriptor():
    import __graft_entry__ as ge
    h = ctypes.CDLL(ge.build())
    for name in ("glnn_sage_mean_fwd_bwd_f32", "glnn_sage_mean_train_step_f32"):
        assert hasattr(h, name), f"{name} not exported"
    h.glnn_abi_version.restype = ctypes.c_int
    assert h.glnn_abi_version() == 12
    from glnn_amd import _lib
    assert _lib.ABI_VERSION == 12
    assert len(_lib.SIGNATURES["glnn_sage_mean_fwd_bwd_f32"]) == 4 and len(_lib.SIGNATURES["glnn_sage_mean_train_step_f32"]) == 5
    assert _lib.lib().glnn_struct_bytes(8) == ctypes.sizeof(_lib.SageMeanDesc)
    assert ctypes.sizeof(_lib.SageMeanDesc) == 8 + _lib.SAGE_MAX_LAYERS * ctypes.sizeof(_lib.SageMeanLayer)
    assert _lib.lib().glnn_struct_bytes(9) == -1


ONE = 4096          # a non-null, 16-byte aligned dummy address: every check below returns before any pointer is read


def _descs(L=2, dims=(8, 12, 5), n=(40, 20, 10)):
    """Descriptors that pass every check (dummy pointers): block l has n[l] sources and n[l + 1] destinations."""
    from glnn_amd import _lib
    d, m = _lib.SageStepDesc(), _lib.SageMeanDesc()
    d.num_layers, m.num_layers = L, L
    r4 = lambda c: (c + 3) // 4 * 4
    for i, v in enumerate(dims):
        d.dims[i] = v
    for l in range(L):
        y, q = d.layer[l], m.layer[l]
        y.indptr = y.indices = y.w = y.b = y.gw = y.gb = y.z = ONE
        y.n_dst, y.n_src, y.nnz, y.ldz = n[l + 1], n[l], 3, r4(dims[l + 1])
        q.w_self = q.b_self = q.gw_self = q.gb_self = q.cat = q.wcat = q.bsum = ONE
        q.ld_cat = 2 * r4(dims[l])
        if l >= 1:
            y.t_indptr = y.t_indices = q.dcat = ONE
            q.ld_dcat = q.ld_cat
    d.x, d.ldx, d.x_rows = ONE, r4(dims[0]), n[0]
    d.labels = d.dlogits = d.loss_out = d.dh = ONE
    d.ld_dlogits, d.ld_dh = r4(dims[-1]), r4(max(dims[1:-1]))
    return d, m


def test_step_entries_report_bad_arguments_without_launching():
    from glnn_amd import _lib
    h = _lib.lib()
    err = h.glnn_last_error
    fb = lambda d, m, ln=None: h.glnn_sage_mean_fwd_bwd_f32(None if d is None else ctypes.byref(d), None if m is None else ctypes.byref(m), ln, None)
    d, m = _descs()
    # null descriptors / pointers: GLNN_ERR_INVALID_ARG (-1)
    assert fb(None, m) == -1 and b"glnn_sage_mean_fwd_bwd_f32" in err() and b"null" in err()
    assert fb(d, None) == -1 and b"null" in err()
    d.x = None
    assert fb(d, m) == -1 and b"null pointer" in err()
    d, m = _descs()
    m.layer[1].w_self = None
    assert fb(d, m) == -1 and b"layer 1: null pointer" in err()
    d, m = _descs()
    m.layer[1].dcat = None
    assert fb(d, m) == -1 and b"dcat" in err()
    d, m = _descs()
    d.num_layers = 9
    assert fb(d, m) == -1 and b"num_layers" in err()
    d, m = _descs()
    m.num_layers = 1
    assert fb(d, m) == -1 and b"mean descriptor" in err()
    # n_src < n_dst
    d, m = _descs()
    d.layer[0].n_src = 10
    assert fb(d, m) == -1 and b"n_src=10 < n_dst=20" in err()
    # block l sources != block l - 1 destinations
    d, m = _descs()
    d.layer[1].n_src = 21
    assert fb(d, m) == -1 and b"block 1 has 21 sources, block 0 20 destinations" in err()
    # odd leading dimensions
    d, m = _descs()
    m.layer[0].ld_cat = 17
    assert fb(d, m) == -1 and b"ld_cat=17" in err()
    d, m = _descs(dims=(7, 12, 5))
    m.layer[0].ld_cat = 14          # 2 * d_in, not 2 * round4(d_in)
    assert fb(d, m) == -1 and b"ld_cat=14" in err()
    d, m = _descs()
    d.layer[0].ldz = 13
    assert fb(d, m) == -1 and b"ldz=13" in err()
    d, m = _descs()
    m.layer[1].ld_dcat = 16
    assert fb(d, m) == -1 and b"ld_dcat=16" in err()
    d, m = _descs()
    d.ld_dh = 10
    assert fb(d, m) == -1 and b"ld_dh=10" in err()
    d, m = _descs()
    d.ldx = 6
    assert fb(d, m) == -1 and b"ldx" in err()
    # a hidden layer wider than 256 without an h buffer: GLNN_ERR_UNSUPPORTED (-2)
    d, m = _descs(dims=(8, 260, 5))
    assert fb(d, m) == -2 and b"260 wide" in err()
    # LayerNorm tails with batchnorm set, and with a missing pointer
    d, m = _descs()
    ln = _lib.SageLnDesc()
    ln.eps = 1e-5
    d.batchnorm = 1
    assert fb(d, m, ctypes.byref(ln)) == -1 and b"LayerNorm" in err()
    d.batchnorm = 0
    assert fb(d, m, ctypes.byref(ln)) == -1 and b"LayerNorm of hidden layer 0: null pointer" in err()
    # the one-call entry checks its Adam descriptor first, then the same
    d, m = _descs()
    assert h.glnn_sage_mean_train_step_f32(ctypes.byref(d), ctypes.byref(m), None, None, None) == -1 and b"Adam descriptor" in err()
    ad = _lib.AdamDesc()
    ad.params = ad.grads = ad.exp_avg = ad.exp_avg_sq = ad.sizes = ad.grads_host = ONE
    d.layer[0].n_src = 10
    assert h.glnn_sage_mean_train_step_f32(ctypes.byref(d), ctypes.byref(m), None, ctypes.byref(ad), None) == -1 and b"n_src=10" in err()


def _conf(**kw):
    conf = dict(model_name="SAGE", num_layers=3, feat_dim=20, hidden_dim=32, label_dim=6, dropout_ratio=0.0, norm_type="batch", device="cpu",
                sage_aggregator="mean")
    conf.update(kw)
    return conf


def test_check_supported_mean_names_every_refusal():
    from glnn_amd import teacher
    from glnn_amd.models import Model
    nll = torch.nn.NLLLoss()
    adam = lambda mdl, **kw: torch.optim.Adam(mdl.parameters(), **kw)

    def refused(model, crit, opt, exc, text):
        with pytest.raises(exc, match=text):
            teacher.check_supported_mean(model, crit, opt)

    for norm in ("none", "batch", "layer"):          # everything but the device is accepted: the last check names the GPU
        model = Model(_conf(norm_type=norm))
        refused(model, nll, adam(model), RuntimeError, "GPU")
    model = Model(_conf())
    refused(Model(_conf(sage_aggregator="gcn")), nll, adam(model), NotImplementedError, "'mean' aggregator only")
    gcn = Model(dict(_conf(), model_name="GCN"))
    refused(gcn, nll, adam(gcn), NotImplementedError, "SAGE teachers only")
    refused(model, torch.nn.CrossEntropyLoss(), adam(model), NotImplementedError, "NLLLoss")
    refused(model, torch.nn.NLLLoss(reduction="sum"), adam(model), NotImplementedError, "NLLLoss")
    refused(model, nll, torch.optim.SGD(model.parameters(), lr=0.1), NotImplementedError, "Adam")
    refused(model, nll, adam(model, amsgrad=True), NotImplementedError, "amsgrad")
    two = torch.optim.Adam([{"params": list(model.parameters())[:2]}, {"params": list(model.parameters())[2:]}])
    refused(model, nll, two, NotImplementedError, "one param group")
    model.encoder.activation = torch.tanh
    refused(model, nll, adam(model), NotImplementedError, "ReLU")
    model = Model(_conf())
    model.encoder.norm_type = "group"
    refused(model, nll, adam(model), NotImplementedError, "norm_type")
    model = Model(_conf())
    model.encoder.norms[0] = torch.nn.BatchNorm1d(32, affine=False)
    refused(model, nll, adam(model), NotImplementedError, "BatchNorm1d")
    # check_supported stays the gate of the "gcn" step and keeps refusing the aggregator
    model = Model(_conf())
    with pytest.raises(NotImplementedError, match="mean"):
        teacher.check_supported(model, nll, adam(model))


def test_train_sage_rejects_an_unknown_mean_step():
    from glnn_amd import train_and_eval as te
    from glnn_amd.models import Model
    model = Model(_conf())
    with pytest.raises(ValueError, match="mean_step"):
        te.train_sage(model, [], None, None, torch.nn.NLLLoss(), torch.optim.Adam(model.parameters()), mean_step="fused")
    assert te.SAGE_MEAN_STEPS == ("autograd", "native")


def test_teacher_cli_mean_step_flag():
    from glnn_amd.cli import get_teacher_args
    assert get_teacher_args(["--teacher", "SAGE"]).sage_mean_step == "autograd"
    assert get_teacher_args(["--teacher", "SAGE", "--sage_aggregator", "mean"]).sage_mean_step == "autograd"
    args = get_teacher_args(["--teacher", "SAGE", "--sage_aggregator", "mean", "--sage_mean_step", "native"])
    assert args.sage_mean_step == "native" and args.sage_aggregator == "mean"
    assert get_teacher_args(["--teacher", "GCN", "--sage_mean_step", "autograd"]).sage_mean_step == "autograd"
    for bad in (["--teacher", "SAGE", "--sage_mean_step", "native"],                                    # the default aggregator is "gcn"
                ["--teacher", "SAGE", "--sage_aggregator", "gcn", "--sage_mean_step", "native"],
                ["--teacher", "GCN", "--sage_mean_step", "native"],
                ["--teacher", "SAGE", "--sage_aggregator", "mean", "--sage_mean_step", "fused"]):
        with pytest.raises(SystemExit):
            get_teacher_args(bad)


def test_loader_switch_defaults_off():
    from glnn_amd.graph import CSRGraph, MultiLayerNeighborSampler, NodeDataLoader
    g = CSRGraph(torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 4, 4)
    assert g.t_add_self is None
    loader = NodeDataLoader(g, torch.arange(4), MultiLayerNeighborSampler([2, 2]), batch_size=2)
    assert loader.plain_transpose is False and loader.global_first_block is False
