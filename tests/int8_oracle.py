"""The int8 row format of docs/INT8_INFERENCE_SEMANTICS.md stated in numpy, and the SAGE forward that quantises at exactly the storage
points of the int8 sweep (SAGE._whole_graph_layer_i8).  No GPU, no torch.

Run as a script, it measures the arithmetic sensitivity that the end-to-end test's bound is built from: the largest row-relative difference
between the oracle in fp64 and the same oracle with float32 arithmetic, on the end-to-end test's own inputs (`e2e_case`)."""
import numpy as np

from graphgen import random_graph, segment_reduce

NAN_BITS = 0x7FC00000


def round16(d):
    return (d + 15) // 16 * 16


def quantise_rows(x):
    """x float32 [n, d] -> (q int8 [n, d], s float32 [n]).  Per row, all in float32: amax = max |x|; s = amax / 127; inv = 127 / amax;
    q = min(max(rint(x * inv), -127), 127), ties to even.  amax == 0: s = 0, q = 0.  A NaN or an Inf in the row: s = NaN, q = 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        bad = ~np.isfinite(x).all(axis=1)
        amax = np.fmax.reduce(ax, axis=1, initial=np.float32(0)).astype(np.float32)
        s = (amax / np.float32(127.0)).astype(np.float32)
        inv = (np.float32(127.0) / amax).astype(np.float32)
        r = np.rint((x * inv[:, None]).astype(np.float32))
        r = np.fmin(np.fmax(r, np.float32(-127.0)), np.float32(127.0))
    flat = bad | (amax == 0)
    r[flat] = 0
    q = r.astype(np.int8)
    s = s.copy()
    s[bad] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
    return q, s


def row_bytes(q, s):
    """(q, s) -> the stored rows, uint8 [n, round16(d + 4)]: values, zero padding, the scale's four little-endian bytes."""
    n, d = q.shape
    ld = round16(d + 4)
    out = np.zeros((n, ld), np.uint8)
    out[:, :d] = q.view(np.uint8)
    out[:, ld - 4:] = np.ascontiguousarray(s, dtype="<f4").view(np.uint8).reshape(n, 4)
    return out


def dequant(q, s, dtype=np.float64):
    return q.astype(dtype) * np.asarray(s).astype(dtype)[:, None]


def qdq(a, dtype=np.float64):
    """quantise-dequantise of a matrix as the kernels see it (its float32 rounding)."""
    return dequant(*quantise_rows(np.asarray(a).astype(np.float32)), dtype=dtype)


def aggregate(indptr, indices, h, n_dst):
    """sum over in-edges, in h's own dtype (entries of a row folded in CSR order)."""
    dst = np.repeat(np.arange(n_dst), np.diff(indptr[:n_dst + 1]))
    return segment_reduce(np.add, h[indices[:indptr[n_dst]]], dst, n_dst, 0)


def int8_storage_oracle(indptr, indices, x, layers, norms, eps=1e-5, arith=np.float64):
    """SAGE "gcn" forward that quantise-dequantises at exactly the storage points of the int8 sweep -- layer 0's input when it aggregates
    first, the chained projection, a project-first layer's x @ W^T, a hidden output the next layer aggregates -- and computes everything
    else in `arith` (fp64: the oracle; float32: the same forward with the kernels' precision, for the sensitivity measurement)."""
    n = len(indptr) - 1
    deg1 = (np.diff(indptr) + 1).astype(arith)
    L = len(layers)
    W = [lay["weight"].astype(arith) for lay in layers]
    agg_first = [w.shape[1] <= w.shape[0] for w in W]

    def mean(h):
        return ((aggregate(indptr, indices, h, n) + h[:n]) / deg1[:, None]).astype(arith)

    def tail(l, z):
        z = z + layers[l]["bias"].astype(arith)
        if l == L - 1:
            return z
        if norms is not None:
            bn = norms[l]
            z = (z - bn["running_mean"].astype(arith)) / np.sqrt(bn["running_var"].astype(arith) + arith(eps)) * bn["weight"].astype(arith) \
                + bn["bias"].astype(arith)
        return np.maximum(z, 0).astype(arith)

    h = x.astype(arith)
    if agg_first[0]:
        h = qdq(h, arith)
    proj = None
    for l in range(L):
        din, dout = W[l].shape[1], W[l].shape[0]
        gathered_next = l + 1 < L and agg_first[l + 1]
        if proj is not None:
            y, proj = tail(l, mean(proj)), None
        elif l + 1 < L and agg_first[l] and din <= 256 and dout <= 256 and not agg_first[l + 1] and W[l + 1].shape[0] <= 256:
            proj = qdq(tail(l, mean(h) @ W[l].T) @ W[l + 1].T, arith)
            continue
        elif not agg_first[l]:
            y = tail(l, mean(qdq(h @ W[l].T, arith)))
        else:
            y = tail(l, mean(h) @ W[l].T)
        h = qdq(y, arith) if gathered_next else y
    return h


# ---- the end-to-end test's inputs (tests/test_int8_inference_gpu.py), built without torch so that the bound can be measured anywhere ----
E2E = [([100, 256, 256, 47], "batch"), ([20, 32, 6], "none"), ([1433, 128, 7], "none")]
E2E_N = 2500


def e2e_case(dims, norm):
    """(indptr, indices, x, layers, norms) of one end-to-end case: a power-law multigraph with isolated rows and a hub, standard normal
    features (sparse 0/1 bag-of-words rows for the cora-like width), Glorot-scaled weights and non-trivial BatchNorm statistics."""
    n = E2E_N
    indptr, indices = random_graph(n, 14, seed=dims[0], power=0.6, isolated=9, hub=1500)
    rs = np.random.RandomState(dims[0] + 1)
    x = rs.standard_normal((n, dims[0])).astype(np.float32)
    if dims[0] > 1000:
        x = (rs.uniform(size=(n, dims[0])) < 0.02).astype(np.float32)
    layers, norms = [], ([] if norm == "batch" else None)
    for l in range(len(dims) - 1):
        din, dout = dims[l], dims[l + 1]
        a = np.sqrt(6.0 / (din + dout))
        layers.append(dict(weight=rs.uniform(-a, a, (dout, din)).astype(np.float32), bias=(rs.standard_normal(dout) * .1).astype(np.float32)))
        if norm == "batch" and l < len(dims) - 2:
            norms.append(dict(weight=rs.uniform(.5, 1.5, dout).astype(np.float32), bias=rs.uniform(-.2, .2, dout).astype(np.float32),
                              running_mean=rs.uniform(-.3, .3, dout).astype(np.float32),
                              running_var=rs.uniform(.5, 1.5, dout).astype(np.float32)))
    return indptr, indices, x, layers, norms


def row_relative(a, b):
    """max over elements of |a - b| / rowmax|b|."""
    return float((np.abs(a - b) / np.maximum(np.abs(b).max(1, keepdims=True), 1e-30)).max())


def measure_sensitivity():
    out = {}
    for dims, norm in E2E:
        case = e2e_case(dims, norm)
        w64 = int8_storage_oracle(*case, arith=np.float64)
        w32 = int8_storage_oracle(*case, arith=np.float32).astype(np.float64)
        out[tuple(dims)] = row_relative(w32, w64)
    return out


if __name__ == "__main__":
    for dims, v in measure_sensitivity().items():
        print(list(dims), f"fp32-vs-fp64 oracle, row-relative: {v:.3e}   B = 4x = {4 * v:.3e}")
