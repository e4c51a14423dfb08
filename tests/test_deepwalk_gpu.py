"""GPU checks of the DeepWalk position features (csrc/deepwalk.hip, glnn_amd/position.py; docs/POSITION_SEMANTICS.md) against the numpy
oracle tests/deepwalk_oracle.py: the pair lists bit for bit, three optimiser steps (table, both Adam moments, loss) within ten times the
oracle's own fp32-against-fp64 error, untouched rows bit for bit, the same bits run to run and stream to stream, the quality of the
embedding on a planted-community graph, fill_unseen, and every refusal.  Smallest shapes that reach every path: lane layouts d / 4 =
1, 4, 25 (of 32), 32, 64; the 300-node star, whose hub is the start and the entry of far more than 128 pairs (the workgroup path of
both gathers)."""
import re

import numpy as np
import pytest
import torch

import deepwalk_oracle as dwo
from subgraph_oracle import six_node_graph
from deepwalk_cases import BETAS, EPS, clustered_case, init_embedding, step_seeds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def star_graph(n=300):
    """Hub 0 and n - 1 leaves, both directions stored: row 0 = [1 .. n - 1], row i = [0]."""
    indptr = np.concatenate([[0], n - 1 + np.arange(n)]).astype(np.int64)
    return indptr, np.concatenate([np.arange(1, n), np.zeros(n - 1)]).astype(np.int32)


def dev_graph(indptr, indices):
    from glnn_amd.graph import CSRGraph
    return CSRGraph(torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV), len(indptr) - 1)


GRAPHS = {"six": six_node_graph, "star": star_graph, "clustered": lambda: clustered_case()[:2]}
_G = {}


def graph(name):
    if name not in _G:
        indptr, indices = GRAPHS[name]()
        _G[name] = (indptr, indices, dev_graph(indptr, indices))
    return _G[name]


# ------------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("n_roots", [1, 7, 300])
@pytest.mark.parametrize("lck", [(1, 2, 1), (4, 3, 2), (10, 5, 1), (64, 10, 1)])
@pytest.mark.parametrize("name", ["six", "star"])
def test_pairs_equal_the_oracle_bit_for_bit(name, lck, n_roots):
    from glnn_amd import ops
    indptr, indices, g = graph(name)
    n = len(indptr) - 1
    length, context, negatives = lck
    roots = (np.arange(n_roots) * 5 + n - 1) % n
    roots[n_roots // 2:] = roots[:n_roots - n_roots // 2]                # repeated roots in every case but B = 1
    rw, rs, rr = dwo.pairs(indptr, indices, roots, length, context, negatives, 123, 456)
    for on_device in (False, True):
        r = torch.from_numpy(roots.astype(np.int64))
        walks, start, rest, pair_indptr, win_indptr = ops.deepwalk_pairs(g.indptr, g.indices, r.to(DEV) if on_device else r, length, context,
                                                                         negatives, 123, 456)
        q, rlen = ops.deepwalk_windows(n_roots, length, context, negatives)
        assert tuple(rest.shape) == (q, rlen) == rr.shape and start.dtype == rest.dtype == torch.int32
        assert np.array_equal(walks.cpu().numpy(), rw) and np.array_equal(start.cpu().numpy(), rs) and np.array_equal(rest.cpu().numpy(), rr)
        assert np.array_equal(pair_indptr.cpu().numpy(), np.arange(q + 1) * rlen) and np.array_equal(win_indptr.cpu().numpy(), np.arange(q + 1))


# ------------------------------------------------------------------------------------------------ three steps against the oracle
# name -> (graph, roots, walk length, context, negatives, lr)
STEP_CASES = {
    "six": ("six", np.array([5, 0, 3, 0, 2, 4, 1]), 4, 3, 2, 0.05),
    "star": ("star", np.arange(300), 4, 3, 1, 0.05),                     # the hub: start and entry of far more than 128 pairs
    "clustered": ("clustered", np.arange(512), 10, 5, 1, 0.05),
    "clustered8": ("clustered", np.arange(8) * 61, 10, 5, 1, 0.05),       # 8 roots: most of the 512 rows are in no pair
    "leaf300": ("star", np.full(300, 7), 1, 2, 1, 0.05),                  # one leaf 300 times: a start list of 300 behind a short entry list
}
_REF = {}


def reference(case, d):
    """Three oracle steps of `case` at width d, once: per step the fp64 state and loss and the touched rows, and the case's yardstick -- how
    far the SAME arithmetic in fp32 (numpy, on the CPU) lands from fp64, per tensor, the largest of the three steps (one step's distance of
    a scalar such as the loss can fall below half an ulp of the fp32 result by chance)."""
    if (case, d) not in _REF:
        gname, roots, length, context, negatives, lr = STEP_CASES[case]
        indptr, indices, _ = graph(gname)
        n = len(indptr) - 1
        z0 = init_embedding(n, d, 0)
        rng = np.random.default_rng(1)
        m0, v0 = (0.01 * rng.standard_normal((n, d))).astype(np.float32), (1e-4 * (0.5 + rng.random((n, d)))).astype(np.float32)
        st = {dt: (z0.astype(dt), m0.astype(dt), v0.astype(dt)) for dt in (np.float64, np.float32)}
        steps = []
        for t in (1, 2, 3):
            out = {dt: dwo.step(*st[dt], indptr, indices, roots, length, context, negatives, 10 + t, 20 + t, lr, BETAS, EPS, t, dt) for dt in st}
            st = {dt: out[dt][:3] for dt in out}
            z, m, v, loss, touched = out[np.float64]
            z32, m32, v32, loss32, _ = out[np.float32]
            yard = {"z": np.abs(z32 - z).max(), "m": np.abs(m32 - m).max(), "v": np.abs(v32 - v).max(), "loss": abs(float(loss32) - float(loss))}
            steps.append((z, m, v, float(loss), touched, yard))
        yard = {k: max(s[5][k] for s in steps) for k in ("z", "m", "v", "loss")}      # the case's yardstick: the largest of its three steps
        _REF[(case, d)] = (z0, m0, v0, [s[:5] + (yard,) for s in steps])
    return _REF[(case, d)]


@pytest.mark.parametrize("d", [4, 16, 100, 128, 256])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_three_steps_against_the_fp64_oracle(case, d):
    """Tolerance: per case and tensor, 10 x the distance between the oracle run in fp32 and in fp64 (the device sums in another order than
    numpy), the largest of the case's three steps.  Measured on the 512-node case at d = 16 (|Z| <= 3.8, moments started away from zero):
    max |dZ| of the fp32 oracle 3.1e-7, so the bound is 3.1e-6; the device lands 1.5e-7 / 2.3e-7 / 3.1e-7 from fp64 after 1 / 2 / 3 steps.
    Over all 25 cases the device's largest distance is 0.12 of its bound.  Every distance, bound and device figure is printed next to the
    assertion.  (Adam's hyper-parameters reach the C entry as doubles: 1 - 0.999f is 1.3e-5 off, which put the step size, and Z, 4 ulp off.)"""
    from glnn_amd.position import DeepWalk
    gname, roots, length, context, negatives, lr = STEP_CASES[case]
    _, _, g = graph(gname)
    z0, m0, v0, steps = reference(case, d)
    dw = DeepWalk(g, d, length, context, negatives, lr=lr, betas=BETAS, eps=EPS, seed=0)
    assert np.array_equal(dw.embedding.cpu().numpy(), z0)               # the same initial bits as the oracle's
    dw.exp_avg.copy_(torch.from_numpy(m0))
    dw.exp_avg_sq.copy_(torch.from_numpy(v0))
    prev = (z0, m0, v0)
    for t, (z, m, v, loss, touched, yard) in zip((1, 2, 3), steps):
        got_loss = dw.step(torch.from_numpy(roots.astype(np.int64)), 10 + t, 20 + t)
        got = {"z": dw.embedding.cpu().numpy(), "m": dw.exp_avg.cpu().numpy(), "v": dw.exp_avg_sq.cpu().numpy()}
        for key, want in (("z", z), ("m", m), ("v", v)):
            err, bound = np.abs(got[key] - want).max(), 10 * yard[key]
            print(f"{case} d={d} step {t} {key}: fp32 oracle vs fp64 {yard[key]:.3g}, bound {bound:.3g}, device vs fp64 {err:.3g}")
            assert err <= bound, (case, d, t, key, err, bound)
        err, bound = abs(got_loss.item() - loss), 10 * yard["loss"]
        print(f"{case} d={d} step {t} loss: fp32 oracle vs fp64 {yard['loss']:.3g}, bound {bound:.3g}, device vs fp64 {err:.3g}")
        assert err <= bound, (case, d, t, "loss", err, bound)
        # every row that is in no pair keeps its bits
        for key, before in zip(("z", "m", "v"), prev):
            assert np.array_equal(got[key][~touched], before[~touched]), (case, d, t, key)
        prev = (got["z"], got["m"], got["v"])
    if case == "clustered8":
        assert (~steps[0][4]).sum() > 256
    assert dw.steps == 3


# ------------------------------------------------------------------------------------------------ same input, same bits
def _fit(seed):
    from glnn_amd.position import DeepWalk
    _, _, g = graph("clustered")
    torch.manual_seed(5)                                                # (the permutation comes from the global CPU generator)
    dw = DeepWalk(g, 16, 10, 5, 1, lr=0.05, seed=seed)
    losses = dw.fit(2, 128)
    return dw.embedding.clone(), losses


def test_two_fits_from_the_same_seed_give_the_same_bits():
    a, la = _fit(3)
    b, lb = _fit(3)
    assert torch.equal(a, b) and la == lb and len(la) == 2 and la[1] < la[0]
    c, _ = _fit(4)
    assert not torch.equal(a, c)


def test_a_step_on_a_busy_side_stream_gives_the_same_bits():
    from glnn_amd.position import DeepWalk
    _, _, g = graph("star")
    roots = torch.arange(300)
    runs = []
    for side in (False, True):
        dw = DeepWalk(g, 100, 4, 3, 1, lr=0.05, seed=0)
        torch.cuda.synchronize()
        if side:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                a = torch.randn(1024, 1024, device=DEV)
                for _ in range(8):
                    a = a @ a * 1e-3                                    # another kernel queued in front on the same stream
                loss = dw.step(roots, 1, 2)
            s.synchronize()
        else:
            loss = dw.step(roots, 1, 2)
        torch.cuda.synchronize()
        runs.append((dw.embedding.clone(), dw.exp_avg.clone(), dw.exp_avg_sq.clone(), loss.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ functional
def test_embedding_separates_the_planted_communities():
    """The 512-node configuration of tests/test_deepwalk_cpu.py through DeepWalk.step: the oracle alone reaches 0.996-0.998 there and fp32
    tracks it to 1e-6, so the bar of 0.95 leaves room only for a real defect."""
    from glnn_amd.position import DeepWalk
    _, _, labels, c = clustered_case()
    _, _, g = graph("clustered")
    dw = DeepWalk(g, c["d"], c["length"], c["context"], c["negatives"], lr=c["lr"], betas=BETAS, eps=EPS, seed=0)
    roots = torch.arange(512)
    losses = [dw.step(roots, *step_seeds(s)) for s in range(c["steps"])]
    acc = dwo.centroid_accuracy(dw.embedding.cpu().numpy(), labels)
    first, last = losses[0].item(), losses[-1].item()
    print(f"accuracy {acc:.4f}, loss {first:.3f} -> {last:.3f}")
    assert acc >= 0.95, acc
    assert last < 0.5 * first


# ------------------------------------------------------------------------------------------------ fill_unseen
def test_fill_unseen_against_numpy_on_the_six_node_graph():
    """Rows: 0: [1, 1, 2]  1: [0, 3]  2: [2, 1, 4]  3: [2]  4: []  5: [].  Observed: 1, 2, 4.  Hidden 0 -> (2 z1 + z2) / 3 (the multi-edge
    counts twice), hidden 3 -> z2, hidden 5 (no in-edge at all) -> zeros."""
    from glnn_amd.position import fill_unseen
    indptr, indices, g = graph("six")
    z = np.random.default_rng(0).standard_normal((6, 8)).astype(np.float32)
    obs = [1, 2, 4]
    want = z.copy()
    for n in (0, 3, 5):
        nb = [u for u in indices[indptr[n]:indptr[n + 1]] if u in obs]
        want[n] = np.mean([z[u] for u in nb], axis=0) if nb else 0.0
    got = fill_unseen(g, torch.from_numpy(z).to(DEV), torch.tensor(obs)).cpu().numpy()
    assert np.array_equal(got[obs], z[obs]) and np.array_equal(got[5], np.zeros(8, np.float32))
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.finfo(np.float32).eps * np.abs(z).max())      # a sum of <= 3 rows and a divide


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_is_a_value_error_with_the_c_message_and_nothing_is_written():
    from glnn_amd import ops
    from glnn_amd.position import DeepWalk
    _, _, g = graph("six")
    roots = torch.arange(6)
    for (length, context, negatives), needle in (((4, 1, 1), "context size"), ((4, 6, 1), "context size"), ((4, 3, 0), "negatives per positive"),
                                                 ((64, 2, 2 ** 25), "Q R < 2^31")):
        with pytest.raises(ValueError, match="glnn_deepwalk_pairs.*" + re.escape(needle)):
            ops.deepwalk_pairs(g.indptr, g.indices, roots, length, context, negatives, 1, 2)
    for bad in ([0, 6, 1], [0, -1, 1]):                                   # on the CPU and on the device: checked on the host, never an index
        for r in (torch.tensor(bad), torch.tensor(bad, device=DEV)):
            with pytest.raises(ValueError, match="glnn_deepwalk_pairs.*outside the graph of 6 nodes"):
                ops.deepwalk_pairs(g.indptr, g.indices, r, 4, 3, 1, 1, 2)
    _, start, rest, _, _ = ops.deepwalk_pairs(g.indptr, g.indices, roots, 4, 3, 1, 1, 2)
    for d in (6, 260):
        z = torch.zeros((6, d), device=DEV)
        with pytest.raises(ValueError, match="glnn_deepwalk_score_f32.*multiple of 4"):
            ops.deepwalk_score(z, start, rest, 3, 1)
        assert not z.any()
    with pytest.raises(ValueError):
        DeepWalk(g, 6)
    with pytest.raises(ValueError):
        DeepWalk(g, 8, walk_length=4, context_size=6)
    dw = DeepWalk(g, 8, 4, 3, 1)
    before = (dw.embedding.clone(), dw.exp_avg.clone(), dw.exp_avg_sq.clone())
    with pytest.raises(ValueError, match="outside the graph"):
        dw.step(torch.tensor([0, 9]), 1, 2)
    assert dw.steps == 0 and all(torch.equal(a, b) for a, b in zip(before, (dw.embedding, dw.exp_avg, dw.exp_avg_sq)))
    assert dw.step(torch.zeros(0, dtype=torch.int64), 1, 2).item() == 0.0 and dw.steps == 0      # an empty batch is no step


# ------------------------------------------------------------------------------------------------ the student's wider first layer
@pytest.mark.parametrize("feat, pos, hid, c, bsz, norm", [(1433, 16, 64, 7, 140, "none"), (100, 64, 256, 40, 512, "batch")])
def test_student_engine_takes_the_wider_first_layer(feat, pos, hid, c, bsz, norm):
    """[features | position embedding] is just a wider input: one native student step at feat_dim + D inputs (cora's 1433 + 16, not a
    multiple of 4 before or after; arxiv-like 100 + 64) against torch autograd in float64 on the same module -- loss and every gradient within
    1e-4 of the largest gradient, the bar of scripts/fuzz_vs_torch.py."""
    import copy
    from glnn_amd import ops
    from glnn_amd.models import Model
    from glnn_amd.student import StudentEngine
    torch.manual_seed(11)
    base = Model(dict(model_name="MLP", num_layers=2, feat_dim=feat + pos, hidden_dim=hid, label_dim=c, dropout_ratio=0.0, norm_type=norm, device=DEV))
    x = torch.cat([torch.randn(bsz + 9, feat, device=DEV), torch.randn(bsz + 9, pos, device=DEV)], dim=1)
    idx = torch.randperm(bsz + 9, device=DEV)[:bsz].contiguous()
    tgt = torch.log_softmax(torch.randn(bsz + 9, c, device=DEV), 1)
    model = copy.deepcopy(base).train()
    eng = StudentEngine(model, torch.optim.Adam(model.parameters(), lr=0.01), bsz)
    ref = copy.deepcopy(base).double().train()
    h = x[idx].double()
    h = ref.encoder.layers[0](h)
    if norm == "batch":
        h = ref.encoder.norms[0](h)
    h = ref.encoder.layers[1](torch.relu(h))
    loss = torch.nn.functional.kl_div(torch.log_softmax(h, 1), tgt[idx].double(), reduction="batchmean", log_target=True)
    loss.backward()
    eng.step(ops.as_feat(x), idx, ops.LOSS_KL, ops.as_feat(tgt), 1.0)
    torch.cuda.synchronize()
    assert abs(float(eng.loss_out) - float(loss)) <= 1e-4 * max(1.0, abs(float(loss)))
    gscale = max(float(q.grad.abs().max()) for q in ref.parameters())
    assert eng.grads[0].shape[1] == feat + pos
    for (name, q), g in zip(ref.named_parameters(), eng.grads):
        assert float((g.double() - q.grad).abs().max()) <= 1e-4 * gscale, name
