"""APPNP teacher on the GPU: the propagation kernels (csrc/appnp.hip) against the fp64 oracle (tests/appnp_oracle.py), the transpose with
edge ids, the edge masks, determinism, the Model surface against the reference's golden (tests/golden/appnp_teacher.npz), the training
step against the oracle, and the command lines end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import appnp_oracle as ao
from graphgen import planted_graph, random_graph, scan_geometry, second_trip_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "appnp_teacher.npz")
DEV = "cuda:0"


def _graph(n=600, seed=3):
    """Non-symmetric multigraph with isolated rows and a hub row far above the long-row threshold (128)."""
    ip, ix = random_graph(n, 6, seed=seed, power=0.6, isolated=9, hub=700)
    from glnn_amd.graph import CSRGraph
    return ip, ix, CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), n)


@pytest.fixture(scope="module")
def graph():
    return _graph()


def _lib_masks(ops, nnz, k, p, seed):
    if p == 0 or k == 0:
        return None
    return np.stack([ops.edge_drop_mask(nnz, t, p, seed, DEV).cpu().numpy() for t in range(1, k + 1)])


def test_transpose_with_edge_ids(graph):
    from glnn_amd import ops
    ip, ix, g = graph
    n, nnz = len(ip) - 1, len(ix)
    t_ip, t_ix = ops.csr_transpose(g.indptr, g.indices, n, n, nnz)
    e_ip, e_ix, eids = ops.csr_transpose_eids(g.indptr, g.indices, n, n, nnz)
    assert torch.equal(t_ip, e_ip) and torch.equal(t_ix, e_ix)
    eids = eids.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(eids), np.arange(nnz))                              # a permutation of the edge ids
    rows = np.repeat(np.arange(n), np.diff(e_ip.cpu().numpy()))
    dst = np.repeat(np.arange(n), np.diff(ip))
    assert np.array_equal(ix[eids], rows)                                              # indices[t_eids[k]] == row(k)
    assert np.array_equal(dst[eids], e_ix.cpu().numpy())                               # ... and the entry is the edge's destination


def test_edge_masks_keep_fraction_and_independence():
    from glnn_amd import ops
    nnz, p = 200_000, 0.5
    m = {(t, s): ops.edge_drop_mask(nnz, t, p, s, DEV).cpu().numpy() for t in (1, 2, 10) for s in (7, 8)}
    sd = np.sqrt(nnz * p * (1 - p))
    for v in m.values():
        assert set(np.unique(v)) <= {0, 1}
        assert abs(int(v.sum()) - nnz * (1 - p)) < 6 * sd
    keys = list(m)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            agree = (m[keys[i]] == m[keys[j]]).mean()
            assert 0.45 < agree < 0.55, (keys[i], keys[j], agree)
    m0 = ops.edge_drop_mask(nnz, 3, 0.0, 7, DEV)
    assert bool((m0 == 1).all())
    m2 = ops.edge_drop_mask(nnz, 1, 0.2, 9, DEV).float().mean().item()
    assert abs(m2 - 0.8) < 6 * np.sqrt(0.16 / nnz)


def _fwd(g, h0, k, alpha, p, seed):
    from glnn_amd.autograd import appnp_fwd
    return appnp_fwd(g, h0, k, alpha, p, seed)


def _bwd(g, dy, k, alpha, p, seed):
    from glnn_amd.autograd import appnp_bwd
    return appnp_bwd(g, dy, k, alpha, p, seed)


CASES = [(d, k, alpha, p) for d in (1, 7, 40, 47, 64, 256) for k in (0, 1, 10) for alpha in (0.1, 1.0) for p in (0.0, 0.5)
         if not (alpha == 1.0 and k == 0)]
# the widths of the remaining appnp_prop_kernel<LPR, ..> instantiations (prop_launch: LPR = pow2 >= ceil(d / 4)): LPR 4, 4, 8, 8, 32, 32
CASES += [(d, k, 0.1, p) for d in (12, 16, 20, 32, 100, 128) for k in (1, 3) for p in (0.0, 0.5)]


@pytest.mark.parametrize("d,k,alpha,p", CASES)
def test_forward_and_backward_match_the_oracle(graph, d, k, alpha, p):
    ip, ix, g = graph
    _check_propagation(ip, ix, g, d, k, alpha, p)
    deg = np.diff(ip)
    assert deg.max() > 128 and (deg == 0).any()


def _check_propagation(ip, ix, g, d, k, alpha, p):
    from glnn_amd import ops
    n = len(ip) - 1
    rs = np.random.RandomState(d * 100 + k)
    h0 = rs.standard_normal((n, d)).astype(np.float32)
    dy = rs.standard_normal((n, d)).astype(np.float32)
    seed = 1234 + d
    masks = _lib_masks(ops, len(ix), k, p, seed)
    out = _fwd(g, torch.from_numpy(h0).to(DEV), k, alpha, p, seed).cpu().numpy()
    ref = ao.propagate(ip, ix, h0, k, alpha, masks, p)
    print(f"n={n} d={d} k={k} p={p} forward: max|err| {np.abs(out - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4)
    dh0 = _bwd(g, torch.from_numpy(dy).to(DEV), k, alpha, p, seed).cpu().numpy()
    ref = ao.propagate_bwd(ip, ix, dy, k, alpha, masks, p)
    print(f"n={n} d={d} k={k} p={p} backward: max|err| {np.abs(dh0 - ref).max():.3e} max|ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(dh0, ref, rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------- launch geometry
# The numbers prop_launch and appnp_prop_kernel derive the grid from, mirrored by name (csrc/row_gather_dev.h, shared by every scan kernel;
# gat.hip reads the same header, so test_gat_gpu.py plants the same rows):
K_BLOCK = 512                 # row_gather_dev.h  kBlock: the rows one trip of the long-row scan looks at (n_chunks = ceil(n / kBlock), scan_rows)
K_WAVES = K_BLOCK // 64       # row_gather_dev.h  kWaves
K_ROWS_PER_WAVE = 8           # row_gather_dev.h  kRowsPerWave
K_LONG_ROW = 128              # row_gather_dev.h  kLongRow: a row above it is a whole workgroup's
K_LONG_BLOCK_ROWS = 512       # row_gather_dev.h  kLongBlockRows
K_LONG_BLOCK_CAP = 512        # row_gather_dev.h  kLongBlockCap
BIG_N = K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP + 656      # 262 800: just above the size at which every scan chunk has a workgroup of its own


def _geometry(n):
    """(n_chunks, n_long_blocks, rows_per_block) of scan_grid and the scan loop scan_rows (both in csrc/row_gather_dev.h)."""
    return scan_geometry(n, K_BLOCK, K_WAVES, K_ROWS_PER_WAVE, K_LONG_BLOCK_ROWS, K_LONG_BLOCK_CAP)


@pytest.fixture(scope="module")
def big_graph():
    from glnn_amd.graph import CSRGraph
    n_chunks, n_long_blocks, _ = _geometry(BIG_N)
    ip, ix = planted_graph(BIG_N, 17, *second_trip_plan(BIG_N, n_chunks, n_long_blocks, K_LONG_ROW))
    return ip, ix, CSRGraph(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV), BIG_N)


def test_big_graph_has_the_rows_the_launch_geometry_branches_on(big_graph):
    ip, ix, _ = big_graph
    n = len(ip) - 1
    n_chunks, n_long_blocks, rows_per_block = _geometry(n)
    assert n > K_LONG_BLOCK_ROWS * K_LONG_BLOCK_CAP and n_chunks > n_long_blocks          # the scan loop makes a second trip
    assert rows_per_block == K_ROWS_PER_WAVE * K_WAVES and n % rows_per_block != 0         # 64 tickets per block; ragged last block
    deg, out_deg = np.diff(ip), np.bincount(ix, minlength=n)
    for d in (deg, out_deg):                                                # the forward over the in-CSR, the backward over the transpose
        long_rows = np.flatnonzero(d > K_LONG_ROW)
        assert (long_rows % n_chunks >= n_long_blocks).sum() >= 2 and (long_rows % n_chunks < n_long_blocks).sum() >= 2
        assert {K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1} <= set(d.tolist())
        assert ((d > 64) & (d < K_LONG_ROW)).any()                           # a one-wave row of two 64-entry chunks
    assert deg.min() == 1 and (deg == 1).sum() > 100 and 2.5 < deg.mean() < 3.5


def test_large_n_propagation_matches_the_oracle(big_graph):
    """The launch geometry a 600-row graph never reaches (appnp.hip prop_launch / appnp_prop_kernel): 64 tickets per row block, a last
    block that ends before its tickets do, and long rows -- destinations forward, sources backward -- that the scan finds on its second trip."""
    ip, ix, g = big_graph
    _check_propagation(ip, ix, g, 8, 2, 0.1, 0.5)


def test_wide_rows_are_column_tiled(graph):
    """d > 256: the 256-column tiles of one launch."""
    from glnn_amd import ops
    ip, ix, g = graph
    n, d, k, p = len(ip) - 1, 300, 3, 0.5
    rs = np.random.RandomState(5)
    h0 = rs.standard_normal((n, d)).astype(np.float32)
    masks = _lib_masks(ops, len(ix), k, p, 5)
    out = _fwd(g, torch.from_numpy(h0).to(DEV), k, 0.1, p, 5).cpu().numpy()
    np.testing.assert_allclose(out, ao.propagate(ip, ix, h0, k, 0.1, masks, p), rtol=1e-4, atol=1e-4)
    dh0 = _bwd(g, torch.from_numpy(h0).to(DEV), k, 0.1, p, 5).cpu().numpy()
    np.testing.assert_allclose(dh0, ao.propagate_bwd(ip, ix, h0, k, 0.1, masks, p), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("d", [7, 47])
def test_two_runs_are_bit_identical(d):
    ip, ix, g = _graph(3000, seed=11)
    rs = np.random.RandomState(d)
    h0 = torch.from_numpy(rs.standard_normal((3000, d)).astype(np.float32)).to(DEV)
    a, b = _fwd(g, h0, 10, 0.1, 0.5, 99), _fwd(g, h0, 10, 0.1, 0.5, 99)
    assert torch.equal(a, b)
    ga, gb = _bwd(g, h0, 10, 0.1, 0.5, 99), _bwd(g, h0, 10, 0.1, 0.5, 99)
    assert torch.equal(ga, gb)
    assert not torch.equal(a, _fwd(g, h0, 10, 0.1, 0.5, 100))                         # the seed matters


# ---------------------------------------------------------------------------------------------------------------- Model surface
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _model(gold, norm, dropout=0.0):
    from glnn_amd.models import Model
    dims = gold["dims"]
    conf = dict(model_name="APPNP", num_layers=2, feat_dim=int(dims[0]), hidden_dim=int(dims[1]), label_dim=int(dims[2]),
                dropout_ratio=dropout, norm_type=norm, device=DEV)
    m = Model(conf)
    pre = f"{norm}.init."
    sd = {k[len(pre):]: torch.from_numpy(np.asarray(v)) for k, v in gold.items() if k.startswith(pre)}
    assert set(m.state_dict()) == set(sd)
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd)
    return m


def _gold_graph(gold):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(gold["indptr"]).to(DEV), torch.from_numpy(gold["indices"]).to(DEV), len(gold["indptr"]) - 1)


@pytest.mark.parametrize("norm", ["none", "batch", "layer"])
def test_model_eval_forward_matches_the_reference(gold, norm):
    m = _model(gold, norm)
    enc = m.encoder
    assert (enc.k, enc.alpha, enc.edge_drop) == (10, 0.1, 0.5)
    m.eval()
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    h_list, logits = m.forward_fitnet(g, x)
    np.testing.assert_allclose(h_list[0].cpu().numpy(), gold[f"{norm}.eval.h0"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(logits.cpu().numpy(), gold[f"{norm}.eval.logits"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(m.inference(g, x).cpu().numpy(), gold[f"{norm}.eval.logits"], rtol=1e-4, atol=1e-4)


def test_model_keeps_raising_for_gat():
    from glnn_amd.models import Model
    with pytest.raises(NotImplementedError):
        Model(dict(model_name="GAT", num_layers=2, feat_dim=4, hidden_dim=4, label_dim=2, dropout_ratio=0.0, norm_type="none", device=DEV))


@pytest.mark.parametrize("norm", ["none", "batch", "layer"])
def test_train_steps_match_the_oracle(gold, norm):
    """train() (TeacherEngine.step_appnp) for three steps == the fp64 oracle fed the library's edge masks of each step."""
    from glnn_amd import ops, teacher
    from glnn_amd.train_and_eval import train
    m = _model(gold, norm)
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    labels = torch.from_numpy(gold["labels"]).to(DEV)
    idx = torch.from_numpy(gold["idx_train"]).to(DEV)
    lr, wd, steps = float(gold["lr"]), float(gold["wd"]), int(gold["steps"])
    opt = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=wd)
    init = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    losses, masks = [], []
    nnz = len(gold["indices"])
    for s in range(steps):
        losses.append(train(m, g, x, labels, torch.nn.NLLLoss(), opt, idx))
        eng = teacher.get_engine(m, opt)
        masks.append(_lib_masks(ops, nnz, 10, 0.5, eng._edge_seed(s + 1)))
    bn = {l: (init[f"encoder.norms.{l}.running_mean"], init[f"encoder.norms.{l}.running_var"]) for l in range(1) if norm == "batch"}
    params = {k: v for k, v in init.items() if "running" not in k and "num_batches" not in k}
    ref_losses, ref_params, ref_bn = ao.train_steps(params, bn, gold["indptr"], gold["indices"], gold["feats"], gold["labels"],
                                                    gold["idx_train"], 2, norm, 10, 0.1, 0.5, masks, lr, wd, steps)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    fin = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for k, v in ref_params.items():
        np.testing.assert_allclose(fin[k], v, rtol=1e-3, atol=1e-4, err_msg=k)
    for l, (rm, rv) in ref_bn.items():
        np.testing.assert_allclose(fin[f"encoder.norms.{l}.running_mean"], rm, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(fin[f"encoder.norms.{l}.running_var"], rv, rtol=1e-4, atol=1e-5)
        assert int(fin[f"encoder.norms.{l}.num_batches_tracked"]) == int(init[f"encoder.norms.{l}.num_batches_tracked"]) + steps


def test_autograd_path_matches_the_engine_gradients(gold):
    """Model.forward in training mode differentiates through AppnpPropFn: with edge_drop 0 its gradient equals the oracle's."""
    m = _model(gold, "none")
    m.encoder.edge_drop = 0.0
    m.train()
    g = _gold_graph(gold)
    x = torch.from_numpy(gold["feats"]).to(DEV)
    idx = torch.from_numpy(gold["idx_train"]).to(DEV)
    from glnn_amd import autograd
    c0 = autograd._drop_counter[0]
    logits = m(g, x)
    assert logits.requires_grad and autograd._drop_counter[0] == c0 + 1      # the trunk's one hidden tail; edge_drop 0 draws nothing
    params = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    _, h0, cache = ao.trunk_forward(params, gold["feats"], 2, "none", training=True)
    ref_logits = ao.propagate(gold["indptr"], gold["indices"], h0, 10, 0.1)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref_logits, rtol=1e-4, atol=1e-4)
    gl = torch.zeros_like(logits)
    gl[idx] = torch.randn(len(idx), logits.shape[1], device=DEV)
    logits.backward(gl)
    dh0 = ao.propagate_bwd(gold["indptr"], gold["indices"], gl.cpu().numpy().astype(np.float64), 10, 0.1)
    grads = ao.trunk_backward(params, cache, dh0, 2)
    for name, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[name], rtol=1e-3, atol=1e-4, err_msg=name)


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("setting", ["tran", "ind"])
def test_appnp_teacher_then_student_cli(tmp_path, setting):
    common = ["--dataset", "synthetic-cora", "--teacher", "APPNP", "--device", "0", "--max_epoch", "6", "--patience", "3",
              "--exp_setting", setting, "--save_results"]
    _run("train_teacher.py", common, tmp_path)
    base = tmp_path / "outputs" / ("transductive" if setting == "tran" else "inductive/split_rate_0.2") / "synthetic-cora"
    tdir = base / "APPNP" / "seed_0"
    out_t = np.load(tdir / "out.npz")["arr_0"]
    assert out_t.shape == (2485, 7) and out_t.dtype == np.float32
    np.testing.assert_allclose(np.exp(out_t).sum(1), 1.0, atol=1e-4)          # log-probabilities of ALL nodes
    _run("train_student.py", common + ["--student", "MLP", "--lamb", "0.5"], tmp_path)
    out_s = np.load(base / "APPNP_MLP" / "seed_0" / "out.npz")["arr_0"]
    assert out_s.shape == (2485, 7) and np.isfinite(out_s).all()
