"""CPU oracle of the bf16 student serving path (glnn_amd.serve): the eval-mode MLP forward that rounds to bf16 at exactly the storage
points -- the features, each weight, each hidden output after its fp32 epilogue -- and nowhere else.

  forward(x, layers, norms)                    fp64 arithmetic between the rounding points: THE oracle
  forward(..., accumulate="fp32")              the same with fp32 products (torch CPU matmul): the STAND-IN for a correct kernel with another
                                               summation order.  Its distance from the oracle is what such a kernel may show: a hidden value
                                               that lands on the other side of a bf16 rounding boundary moves a logit by far more than fp32 noise.
  forward(..., round_storage=False)            the plain fp64 forward (what the fp32 path computes, exactly)

layers: [dict(weight [n, k], bias [n])], norms: [dict(weight, bias, running_mean, running_var)] per hidden layer or None (norm "none").
The BatchNorm(eval) + bias fold is the fp32 epilogue  relu(v * s + t),  s = gamma / sqrt(var + eps),  t = (bias - mean) * s + beta."""
import numpy as np
import torch

CLEAR_MARGIN = 0.05      # a row is "clear" when its top-2 margin exceeds this fraction of its largest |logit|


def bf16(a):
    """Round to bf16 (nearest even), returned as float64."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def fold(layer, norm, eps=1e-5):
    b = layer["bias"].astype(np.float64)
    if norm is None:
        return None, b
    s = norm["weight"].astype(np.float64) / np.sqrt(norm["running_var"].astype(np.float64) + eps)
    return s, (b - norm["running_mean"].astype(np.float64)) * s + norm["bias"].astype(np.float64)


def forward(x, layers, norms=None, accumulate="fp64", round_storage=True, eps=1e-5):
    rnd = bf16 if round_storage else (lambda a: np.asarray(a, dtype=np.float64))
    h = rnd(x)
    L = len(layers)
    for l, layer in enumerate(layers):
        w = rnd(layer["weight"])
        last = l == L - 1
        s, t = fold(layer, None if last or norms is None else norms[l], eps)
        if accumulate == "fp32":
            v = torch.matmul(torch.from_numpy(h.astype(np.float32)), torch.from_numpy(w.astype(np.float32)).t()).numpy()
            sv = np.float32(1.0) if s is None else s.astype(np.float32)
            v = v * sv + t.astype(np.float32)          # fp32 epilogue
            v = v.astype(np.float64)
        else:
            v = h @ w.T
            v = v * (1.0 if s is None else s) + t
        h = v if last else rnd(np.maximum(v, 0.0))
    return h


def row_max(z):
    return np.abs(z).max(axis=1)


def rel_err(got, want, floor=0.0):
    """max over rows of  max_j |got - want| / max(floor, row max of |want|)."""
    return float((np.abs(got - want).max(axis=1) / np.maximum(floor, row_max(want))).max())


def clear_rows(z):
    top2 = np.sort(z, axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) > CLEAR_MARGIN * row_max(z)


def draw_case(dims, norm, n, seed, cora_like=False):
    """(x, layers, norms) of one table row: torch-default-scale uniform weights and biases, BatchNorm vectors drawn as the bf16 teacher test
    draws them, N(0,1) features (cora_like: 2 % non-zero 0/1 rows)."""
    rs = np.random.RandomState(seed)
    layers, norms = [], ([] if norm == "batch" else None)
    for l in range(len(dims) - 1):
        k, m = dims[l], dims[l + 1]
        bound = 1.0 / np.sqrt(k)
        layers.append(dict(weight=rs.uniform(-bound, bound, (m, k)).astype(np.float32), bias=rs.uniform(-bound, bound, m).astype(np.float32)))
        if norm == "batch" and l != len(dims) - 2:
            norms.append(dict(weight=rs.uniform(.5, 1.5, m).astype(np.float32), bias=rs.uniform(-.2, .2, m).astype(np.float32),
                              running_mean=rs.uniform(-.3, .3, m).astype(np.float32), running_var=rs.uniform(.5, 1.5, m).astype(np.float32)))
    if cora_like:
        x = (rs.uniform(size=(n, dims[0])) < 0.02).astype(np.float32)
    else:
        x = rs.standard_normal((n, dims[0])).astype(np.float32)
    return x, layers, norms


# (dims, norm, rows, cora-like): the six models of the end-to-end test
CASES = [
    ((100, 2048, 2048, 47), "batch", 4096, False),
    ((128, 1024, 1024, 40), "batch", 4096, False),
    ((100, 256, 256, 47), "batch", 4096, False),
    ((1433, 128, 7), "none", 2500, True),
    ((20, 32, 6), "none", 4096, False),
    ((300, 320, 5), "none", 4096, False),
]
