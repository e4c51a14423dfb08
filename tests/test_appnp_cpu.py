"""CPU checks of the APPNP teacher's oracle (tests/appnp_oracle.py) against the reference's own Python (tests/golden/appnp_teacher.npz,
made by tests/golden/make_appnp_golden.py) and against torch autograd, plus the APPNP training config."""
import os

import numpy as np
import pytest
import torch

import appnp_oracle as ao
from graphgen import random_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "appnp_teacher.npz")
NORMS = ("none", "batch", "layer")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _params(z, tag, which):
    pre = f"{tag}.{which}."
    return {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}


def _bn_state(p):
    return {int(k.split(".")[2]): (p[k], p[k.replace("running_mean", "running_var")]) for k in p if k.endswith("running_mean")}


def _masks(z, tag):
    nnz = len(z["indices"])
    return np.unpackbits(z[f"{tag}.masks"], axis=-1)[..., :nnz]


def test_golden_graph_has_the_promised_features(gold):
    ip, ix = gold["indptr"], gold["indices"]
    n = len(ip) - 1
    deg = np.diff(ip)
    assert deg.max() > 128 and (deg == 0).any()                                       # a long row, isolated rows
    dst = np.repeat(np.arange(n), deg)
    pairs = dst.astype(np.int64) * n + ix
    assert len(np.unique(pairs)) < len(pairs)                                          # a multi-edge
    a = np.zeros((n, n))
    np.add.at(a, (dst, ix), 1)
    assert not np.array_equal(a, a.T)                                                  # non-symmetric
    assert _masks(gold, "none").shape == (3, 10, len(ix))


@pytest.mark.parametrize("norm", NORMS)
def test_oracle_reproduces_the_reference_eval_forward(gold, norm):
    p = _params(gold, norm, "init")
    h_list, h0, _ = ao.trunk_forward(p, gold["feats"], 2, norm, _bn_state(p), training=False)
    np.testing.assert_allclose(h_list[0], gold[f"{norm}.eval.h0"], rtol=1e-5, atol=1e-5)
    logits = ao.propagate(gold["indptr"], gold["indices"], h0, 10, 0.1)
    np.testing.assert_allclose(logits, gold[f"{norm}.eval.logits"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("norm", NORMS)
def test_oracle_reproduces_the_reference_training_steps(gold, norm):
    p = _params(gold, norm, "init")
    masks = _masks(gold, norm)
    losses, params, bn = ao.train_steps({k: v for k, v in p.items() if "running" not in k and "num_batches" not in k}, _bn_state(p),
                                        gold["indptr"], gold["indices"], gold["feats"], gold["labels"], gold["idx_train"], 2, norm, 10, 0.1,
                                        0.5, masks, float(gold["lr"]), float(gold["wd"]), int(gold["steps"]))
    np.testing.assert_allclose(losses, gold[f"{norm}.losses"], rtol=1e-5)
    fin = _params(gold, norm, "final")
    for k, v in params.items():
        np.testing.assert_allclose(v, fin[k], rtol=1e-4, atol=1e-5, err_msg=k)
    for l, (rm, rv) in bn.items():
        np.testing.assert_allclose(rm, fin[f"encoder.norms.{l}.running_mean"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rv, fin[f"encoder.norms.{l}.running_var"], rtol=1e-5, atol=1e-6)


def test_the_recorded_masks_differ_per_iteration_and_step(gold):
    m = _masks(gold, "none")
    assert 0.4 < m.mean() < 0.6
    assert not np.array_equal(m[0, 0], m[0, 1]) and not np.array_equal(m[0, 0], m[1, 0])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 3, 10])
def test_oracle_backward_matches_float64_autograd(seed, k):
    ip, ix = random_graph(90, 4, seed=seed, power=0.5, isolated=4, hub=40)
    n, d, p, alpha = 90, 6, 0.5, 0.1
    rs = np.random.RandomState(seed)
    masks = (rs.rand(k, len(ix)) >= p).astype(np.uint8)
    h0 = rs.standard_normal((n, d))
    g = rs.standard_normal((n, d))
    dn, sn = ao.degree_norms(ip, ix, n)
    dst = torch.from_numpy(np.repeat(np.arange(n), np.diff(ip)))
    src = torch.from_numpy(ix.astype(np.int64))
    x0 = torch.tensor(h0, requires_grad=True)
    h = x0
    for t in range(k):
        w = torch.from_numpy(masks[t].astype(np.float64) / (1 - p)).unsqueeze(1)
        agg = torch.zeros(n, d, dtype=torch.float64).index_add(0, dst, w * torch.from_numpy(sn).unsqueeze(1)[src] * h[src])
        h = (1 - alpha) * torch.from_numpy(dn).unsqueeze(1) * agg + alpha * x0
    np.testing.assert_allclose(h.detach().numpy(), ao.propagate(ip, ix, h0, k, alpha, masks, p), rtol=1e-12, atol=1e-12)
    h.backward(torch.from_numpy(g))
    np.testing.assert_allclose(ao.propagate_bwd(ip, ix, g, k, alpha, masks, p), x0.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_training_config_merges_like_the_reference():
    import glnn_amd  # noqa: F401
    from glnn_amd.utils import get_training_config
    conf = get_training_config(os.path.join(ROOT, "train.conf.yaml"), "APPNP", "cora")
    # reference utils.get_training_config: the `global` section overlaid by cora.APPNP (reference train.conf.yaml:28-30), plus model_name
    assert conf == {"hidden_dim": 128, "num_layers": 2, "dropout_ratio": 0.5, "weight_decay": 0.01, "model_name": "APPNP"}
    for ds in ("citeseer", "pubmed", "a-computer", "a-photo"):
        c = get_training_config(os.path.join(ROOT, "train.conf.yaml"), "APPNP", ds)
        assert (c["dropout_ratio"], c["weight_decay"]) == (0.5, 0.01)
