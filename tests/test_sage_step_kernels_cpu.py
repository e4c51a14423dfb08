"""CPU checks of what tests/test_sage_step_kernels_gpu.py stands on: the fp64 oracle of the step's fused aggregation kernels
(tests/sage_step_kernel_oracle.py) against hand answers, against the fp64 LayerNorm step oracle and the fp32 training oracle on the
planted batch; the planted batch's row classes (tests/sage_step_graphs.py); and the seeds of the GPU cases."""
import functools

import numpy as np
import pytest

import sage_ln_oracle as so
import sage_step_graphs as sg
import sage_step_kernel_oracle as ko
from oracle import student_oracle
from oracle import teacher_train_oracle as tto
from sampling_oracle import csr_transpose

F64 = np.float64


@functools.lru_cache(maxsize=None)
def _batch():
    return sg.planted_batch()


# ------------------------------------------------------------------------------------------------ hand answers on a six-node block
# six sources, three destinations: 0 <- {3, 4}, 1 <- {}, 2 <- {5, 5, 0}
IP, IX = np.array([0, 2, 2, 5], np.int64), np.array([3, 4, 5, 5, 0], np.int32)


def test_mean_with_a_dropped_source_by_hand():
    z = np.array([[1.0, -2.0], [0.5, 0.5], [-1.0, 3.0], [2.0, 2.0], [4.0, -1.0], [-3.0, 1.0]])
    scale, shift = np.array([2.0, 1.0]), np.array([-1.0, 0.5])
    mask = np.ones((6, 2))
    mask[4] = 0                                            # source 4 is dropped whole
    h, hc = ko.tail_bn(z, scale, shift, mask, 0.5)         # kept elements are doubled
    np.testing.assert_array_equal(h[3], [6.0, 5.0])        # relu(2 * 2 - 1) * 2, relu(2 + 0.5) * 2
    np.testing.assert_array_equal(h[4], [0.0, 0.0])
    np.testing.assert_array_equal(h[0], [2.0, 0.0])        # relu(2 - 1) * 2, relu(-2 + 0.5) = 0
    np.testing.assert_array_equal(hc[0], [6.0, 5.0])       # (|2| + |-1|) * 2, (|-2| + |0.5|) * 2: not gated by the ReLU
    v, c, d1 = ko.sage_mean(IP, IX, h, hc)
    np.testing.assert_array_equal(d1[:, 0], [3, 1, 4])
    np.testing.assert_allclose(v[0], [(6.0 + 0.0 + 2.0) / 3, (5.0 + 0.0 + 0.0) / 3], rtol=1e-15)
    np.testing.assert_array_equal(v[1], h[1])              # no in-edges: the row itself
    np.testing.assert_allclose(v[2], (2 * h[5] + h[0] + h[2]) / 4, rtol=1e-15)
    assert np.all(c >= np.abs(v))


def test_dy_row_by_hand():
    # transposed block of the six-node block with self entries: source 0 -> {0 (self), 2}, 5 -> {2, 2}, 3 -> {0}, 1 -> {1 (self)}
    t_ip, t_ix, _ = csr_transpose(IP, IX, 3, 6, add_self=True)
    assert list(np.diff(t_ip)) == [2, 1, 1, 1, 1, 2] and list(t_ix[t_ip[5]:t_ip[6]]) == [2, 2]
    dagg = np.array([[1.0, -1.0], [2.0, 2.0], [-4.0, 8.0]])
    inv = np.array([1 / 3, 1.0, 0.25])
    da, dac, terms = ko.transposed_sum(t_ip, t_ix, dagg, inv)
    np.testing.assert_allclose(da[0], [1 / 3 - 1.0, -1 / 3 + 2.0], rtol=1e-15)
    np.testing.assert_allclose(dac[0], [1 / 3 + 1.0, 1 / 3 + 2.0], rtol=1e-15)      # the subtraction became an addition
    np.testing.assert_allclose(da[5], [-2.0, 4.0], rtol=1e-15)
    assert list(terms[:, 0]) == [2, 1, 1, 1, 1, 2]
    z = np.array([[1.0, -2.0], [0.5, 0.5], [-1.0, 3.0], [2.0, 2.0], [4.0, -1.0], [-3.0, 1.0]])
    mean, rstd = np.array([0.5, 0.25]), np.array([2.0, 4.0])
    a_scale, a_shift = np.array([1.0, 1.0]), np.array([0.0, 0.0])          # gate = z > 0
    mask = np.ones((6, 2))
    mask[5, 1] = 0
    r = ko.bn_dy(da, dac, z, mean, rstd, a_scale, a_shift, mask, 0.5)
    dy = r["dy"][0]
    np.testing.assert_allclose(dy[0], [2 * (1 / 3 - 1.0), 0.0], rtol=1e-15)        # z = (1, -2): second gate closed
    np.testing.assert_array_equal(dy[5], [0.0, 0.0])                               # z = (-3, 1): gate closed, element dropped
    xh = (z - mean) * rstd
    np.testing.assert_allclose(r["S1"][0], dy.sum(0), rtol=1e-15)
    np.testing.assert_allclose(r["S2"][0], (dy * xh).sum(0), rtol=1e-15)
    assert not r["undecided"].any()
    assert np.all(r["S2"][1] >= np.abs(r["S2"][0])) and np.all(r["dy"][1] >= np.abs(dy))


def test_layernorm_dz_row_at_d_3_by_hand():
    """inv_h = 1 / 3: the means of the LayerNorm backward run over the three real columns."""
    z = np.array([[1.0, 2.0, 6.0]])
    mu, var = 3.0, (4.0 + 1.0 + 9.0) / 3
    rstd = 1 / np.sqrt(var)
    gamma, beta = np.array([1.0, 2.0, 0.5]), np.array([0.0, 3.0, 0.0])
    da = np.array([[0.3, -0.6, 0.9]])
    r = ko.ln_dz(da, np.abs(da), z, [mu], [rstd], gamma, beta)
    xh = (z[0] - mu) * rstd
    gate = (xh * gamma + beta > 0)
    assert list(gate) == [False, True, True]
    dy = da[0] * gate
    dxh = dy * gamma
    m1, m2 = dxh.sum() / 3, (dxh * xh).sum() / 3
    np.testing.assert_allclose(r["m1"][0][0, 0], (-1.2 + 0.45) / 3, rtol=1e-15)
    np.testing.assert_allclose(r["dz"][0][0], rstd * (dxh - m1 - xh * m2), rtol=1e-14)
    np.testing.assert_allclose(r["dz"][0].sum(), 0.0, atol=1e-15)                  # a LayerNorm's dz sums to zero over its row
    np.testing.assert_allclose(r["dgamma"][0], dy * xh, rtol=1e-15)
    np.testing.assert_allclose(r["dbeta"][0], dy, rtol=1e-15)
    # the same row padded to four columns (a padding column enters nothing: gamma = beta = z = 0 there, and the mean still runs over 3):
    # what a kernel computes when it counts the padded columns instead is a different number
    wrong = rstd * (dxh - dxh.sum() / 4 - xh * (dxh * xh).sum() / 4)
    assert np.abs(wrong - r["dz"][0][0]).max() > 1e3 * ko.bound(3 + 3, r["dz"][1][0]).max()


def test_padded_row_and_empty_row_by_hand():
    """A destination without in-edges is its own row; a source without entries in the transposed block gets da = 0 and dz = 0 whatever
    its z; its condition sums are 0, so the bound there is exact equality."""
    t_ip, t_ix = np.array([0, 0, 1], np.int64), np.array([0], np.int32)
    da, dac, terms = ko.transposed_sum(t_ip, t_ix, np.array([[2.0, 4.0, 8.0]]), np.array([0.5]))
    np.testing.assert_array_equal(da, [[0, 0, 0], [1, 2, 4]])
    r = ko.ln_dz(da, dac, np.array([[5.0, 1.0, 0.0], [1.0, 2.0, 6.0]]), [2.0, 3.0], [0.4, 0.5], np.ones(3), np.ones(3))
    np.testing.assert_array_equal(r["dz"][0][0], [0, 0, 0])
    np.testing.assert_array_equal(ko.bound(terms + 3, r["dz"][1])[0], [0, 0, 0])


# ------------------------------------------------------------------------------------------------ the planted batch
def test_planted_batch_has_the_rows_the_kernels_branch_on():
    b = _batch()
    sg.check_planted_batch(b)                              # (planted_batch() ran it already; here it is a test of its own)
    inp, gidx, dstn = sg.global_ids(b, 7000)
    ip0, ix0, _ = b["blocks"][0]
    assert len(np.unique(inp)) == len(inp) and np.array_equal(gidx, inp[ix0]) and np.array_equal(dstn, inp[:sg.N_DST0])
    assert not np.array_equal(dstn, np.arange(sg.N_DST0))                          # the self rows are NOT the first rows of the matrix


def test_large_batch_has_the_launch_geometry():
    sg.check_large_batch(sg.large_batch())
    sg.big_graph_for_public_spmm()


def _blocks(b):
    return [(ip, ix, ns) for ip, ix, ns in b["blocks"]]


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_oracle_agrees_with_the_fp64_layernorm_step_oracle(p):
    """tail_ln + sage_mean = the aggregate of layer 1, ln_dz = the backward of layer 0's tail, on the planted batch."""
    b = _batch()
    f, h = 20, 30
    x, labels, sd = sg.case_inputs(f, h, "layer")
    st = so.State(sd, 2)
    rs = np.random.RandomState(3)
    mask = None if p == 0 else (rs.uniform(size=(sg.N_DST0, h)) >= p).astype(F64)
    logits, cache = so.forward(st, _blocks(b), x, None if mask is None else [mask], p)
    loss, dl = so.loss_and_dlogits(logits, labels)
    grads = so.backward(st, cache, dl, p)
    c0 = cache[0]
    g, be = st.G(0)
    mean, rstd = c0["z"].mean(1), c0["rstd"][:, 0]
    hv, hc = ko.tail_ln(c0["z"], mean, rstd, g, be, mask, p)
    ip1, ix1, _ = b["blocks"][1]
    agg, aggc, _ = ko.sage_mean(ip1, ix1, hv, hc)
    np.testing.assert_allclose(agg, cache[1]["agg"], rtol=1e-12, atol=1e-14)
    assert np.all(aggc >= np.abs(agg))
    w1, _ = st.W(1)
    da, dac, _ = ko.transposed_sum(*b["t1"], dl @ w1, 1.0 / (np.diff(ip1) + 1.0))
    r = ko.ln_dz(da, dac, c0["z"], mean, rstd, g, be, mask, p)
    np.testing.assert_allclose(r["dgamma"][0], grads["encoder.norms.0.weight"], rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(r["dbeta"][0], grads["encoder.norms.0.bias"], rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(r["sum_dz"][0], grads["encoder.layers.0.fc_neigh.bias"], rtol=1e-9, atol=1e-16)
    np.testing.assert_allclose(r["dz"][0].T @ c0["agg"], grads["encoder.layers.0.fc_neigh.weight"], rtol=1e-9, atol=1e-15)
    for k in ("dy", "dxh", "m1", "m2", "dz", "dgamma", "dbeta", "sum_dz"):
        assert np.all(r[k][1] >= np.abs(r[k][0])), k


def _fp32_z0(b, f, h, norm):
    x, _, sd = sg.case_inputs(f, h, norm)
    st = tto.TeacherState(sd, "sage", 1)                  # (one layer: the "logits" are z_0, whatever norm follows)
    z0, _ = tto.sage_forward(st, _blocks(b)[:1], x)
    return z0, sd


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_oracle_agrees_with_the_fp32_training_oracle_to_rounding(p):
    """BatchNorm tails, oracle/teacher_train_oracle.py (numpy fp32): its aggregate of layer 1, its dy and its two column sums lie within
    the oracle's own bound of the fp64 values computed from ITS z_0 and statistics (its xhat-first affine map costs two more roundings
    than the kernels' one fma: the bound is taken with twice the slack)."""
    b = _batch()
    f, h = 20, 36
    x, labels, sd = sg.case_inputs(f, h, "batch")
    sd = dict(sd, **{"encoder.norms.0.running_mean": np.zeros(h, np.float32), "encoder.norms.0.running_var": np.ones(h, np.float32),
                     "encoder.norms.0.num_batches_tracked": 0})
    st = tto.TeacherState(sd, "sage", 2, "batch")
    rs = np.random.RandomState(4)
    keep = None if p == 0 else (rs.uniform(size=(sg.N_DST0, h)) >= p).astype(np.float32)
    logits, cache = tto.sage_forward(st, _blocks(b), x, None if keep is None else [keep], p)
    loss, dl = student_oracle.loss_and_dlogits(logits, labels, "nll", 1.0)
    grads = tto.sage_backward(st, cache, dl, p)
    z0 = (cache["agg"][0] @ st.W[0].T + st.b[0]).astype(np.float32)
    t = cache["tails"][0]
    mean = z0.mean(axis=0, dtype=F64).astype(np.float32)
    rstd = t["rstd"]
    a_scale = st.gamma[0].astype(F64) * rstd
    a_shift = st.beta[0].astype(F64) - mean * a_scale
    hv, hc = ko.tail_bn(z0, a_scale, a_shift, keep, p)
    ip1, ix1, _ = b["blocks"][1]
    agg, aggc, d1 = ko.sage_mean(ip1, ix1, hv, hc)
    # the condition of the xhat-first form (|z| + |mean|) rstd gamma + |beta| is the larger one
    xc = (np.abs(z0.astype(F64)) + np.abs(mean)) * rstd * np.abs(st.gamma[0]) + np.abs(st.beta[0])
    _, aggc2, _ = ko.sage_mean(ip1, ix1, hv, xc * (1 if keep is None else keep / (1 - p)))
    assert np.all(aggc2 >= aggc * (1 - 1e-12))
    assert np.all(np.abs(cache["agg"][1] - agg) <= 2 * ko.bound(d1, aggc2))
    dagg = (dl.astype(np.float32) @ st.W[1]).astype(np.float32)                    # (the training oracle divides by deg + 1 itself)
    da, dac, terms = ko.transposed_sum(*b["t1"], dagg, (1.0 / (np.diff(ip1) + 1.0)).astype(np.float32))
    r = ko.bn_dy(da, dac, z0, mean, rstd, a_scale, a_shift, keep, p)
    y64 = ko.pre_bn(z0, a_scale, a_shift)[0]
    sure = ~r["undecided"] & ((y64 > 0) == (t["y"] > 0))
    assert sure.mean() > 0.9999
    # its dy = the rows of dz's input: recomputed the way _tail_bwd does
    dh = (cache["A"][1][0].T @ (dagg / cache["A"][1][1]).astype(np.float32)).astype(np.float32)
    dh[:sg.N_DST1] += (dagg / cache["A"][1][1]).astype(np.float32)
    dy32 = dh * (1 if keep is None else keep * np.float32(1 / (1 - p))) * (t["y"] > 0)
    assert np.all((np.abs(dy32 - r["dy"][0]) <= 2 * ko.bound(terms, r["dy"][1]))[sure])
    if sure.all():
        assert np.all(np.abs(grads[5] - r["S1"][0]) <= 2 * ko.bound(sg.N_DST0, r["S1"][1]))
        assert np.all(np.abs(grads[4] - r["S2"][0]) <= 2 * ko.bound(sg.N_DST0, r["S2"][1]))


# ------------------------------------------------------------------------------------------------ the seeds of the GPU cases
def gate_margins(b, f, h, norm):
    """(|y| / (8 * 2^-24 * condition)) of every element of the fp32 oracle's layer-0 pre-activation: below 1 = undecided."""
    z0, sd = _fp32_z0(b, f, h, norm)
    z = z0.astype(F64)
    if norm == "batch":
        mean, var = z.mean(0), z.var(0)
        a_scale = sd["encoder.norms.0.weight"] / np.sqrt(var + 1e-5)
        y, c = ko.pre_bn(z, a_scale, sd["encoder.norms.0.bias"] - mean * a_scale)
    elif norm == "layer":
        mean, var = z.mean(1), z.var(1)
        y, c, _, _ = ko.pre_ln(z, mean, 1 / np.sqrt(var + 1e-5), sd["encoder.norms.0.weight"], sd["encoder.norms.0.bias"])
    else:
        y, c = ko.pre_bn(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, np.abs(y) / (ko.GATE_ULPS * ko.U * c), np.inf)


def test_relu_gates_are_decided_for_every_seed_the_gpu_tests_use():
    """For every (f, h, norm) the planted-batch GPU tests run: no element of the fp32 CPU oracle's z_0 has its pre-activation within 64
    gate margins of zero, so the GPU's z_0 -- the same numbers to fp32 rounding -- leaves the GPU tests nothing undecided.  (The two
    large-geometry cases cannot be chosen this way: 18 million pre-activations hold about a hundred such elements whatever the seed.
    Their test applies the rule for undecided elements with its caps instead.)"""
    b = _batch()
    for f, h, norm in sorted(set(sg.all_cases())):
        m = gate_margins(b, f, h, norm)
        assert m.min() > 64, (f, h, norm, float(m.min()), int((m <= 64).sum()))


def test_condition_sums_dominate_the_values():
    b = _batch()
    rs = np.random.RandomState(0)
    h = 12
    z = rs.standard_normal((sg.N_DST0, h))
    mask = (rs.uniform(size=z.shape) >= 0.3).astype(F64)
    g, be = rs.uniform(0.5, 1.5, h), rs.uniform(-0.2, 0.2, h)
    mean, rstd = z.mean(1), 1 / np.sqrt(z.var(1) + 1e-5)
    ip1, ix1, _ = b["blocks"][1]
    for hv, hc in (ko.tail_bn(z, g, be, mask, 0.3), ko.tail_bn(z), ko.tail_ln(z, mean, rstd, g, be, mask, 0.3)):
        assert np.all(hc >= np.abs(hv))
        v, c, _ = ko.sage_mean(ip1, ix1, hv, hc)
        assert np.all(c >= np.abs(v))
    dagg = rs.standard_normal((sg.N_DST1, h))
    da, dac, _ = ko.transposed_sum(*b["t1"], dagg, 1.0 / (np.diff(ip1) + 1.0))
    assert np.all(dac >= np.abs(da))
    for r in (ko.bn_dy(da, dac, z, z.mean(0), 1 / np.sqrt(z.var(0) + 1e-5), g, be, mask, 0.3), ko.ln_dz(da, dac, z, mean, rstd, g, be, mask, 0.3)):
        for k, (v, c, *_) in r.items():
            if k not in ("undecided", "flip"):
                assert np.all(c >= np.abs(v) * (1 - 1e-12)), k
