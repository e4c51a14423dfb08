"""Graphs, seeds and host-side expectations shared by tests/test_sampled_inference_cpu.py and tests/test_sampled_inference_gpu.py.  TEST
INFRASTRUCTURE ONLY: numpy, no torch, no GPU.  The expected sampled graphs are the compaction of tests/sampling_oracle.py's
sample_neighbors over seeds = arange(n); the per-layer seed is restated from oracle/dropout_mask.py's drop_hash."""
import functools

import numpy as np

import sampling_oracle as so
from graphgen import csr_from_edges
from oracle.dropout_mask import drop_hash

N = 300
HUB, HUB_EDGES = 17, 3000
LONG, LONG_EDGES = 50, 130
ISOLATED = (3, 40, 69, 200, 299)
FANOUTS = (1, 5, 8, 9, 16, 17, 32, 33, 64)          # 8|9, 16|17, 32|33: the boundaries between the lane groups of 8 / 16 / 32 / 64
SEEDS = (7, 0xC0FFEE11)
# for every tested fan-out f one row of exactly f in-edges (copied in row order) and one of f + 1 (the shortest row that is drawn from)
PLANTED_DEGREES = sorted({d for f in FANOUTS for d in (f, f + 1)})
PLANTED = {d: 20 + k for k, d in enumerate(PLANTED_DEGREES)}          # degree -> row (20 .. 34: inside the first 70 rows)
FIRST_ROWS = 70


@functools.lru_cache(maxsize=None)
def big_graph():
    """300 rows, built like _edges() of tests/test_sage_mean_gpu.py: a hub of 3000 in-edges drawn with repetition, a row of 130, multi-edges
    (7 -> 5 three times, 120 -> 64 twice), the self-loop 10 -> 10, five isolated rows, and the planted rows of PLANTED."""
    rs = np.random.RandomState(11)
    m = 1500
    src, dst = rs.randint(0, N, m), rs.randint(0, N, m)
    keep = ~np.isin(dst, ISOLATED + (HUB, LONG) + tuple(PLANTED.values()))
    src, dst = [src[keep]], [dst[keep]]
    src += [np.asarray([7, 7, 7, 120, 120, 10]), rs.randint(0, N, HUB_EDGES), rs.randint(0, N, LONG_EDGES)]
    dst += [np.asarray([5, 5, 5, 64, 64, 10]), np.full(HUB_EDGES, HUB), np.full(LONG_EDGES, LONG)]
    for d, row in PLANTED.items():
        src.append(rs.randint(0, N, d))
        dst.append(np.full(d, row))
    ip, ix = csr_from_edges(np.concatenate(src), np.concatenate(dst), N)
    deg = np.diff(ip)
    assert deg[HUB] == HUB_EDGES and deg[LONG] == LONG_EDGES and all(deg[i] == 0 for i in ISOLATED)
    assert all(deg[row] == d for d, row in PLANTED.items())
    assert len(np.unique(ix[ip[HUB]:ip[HUB + 1]])) < HUB_EDGES          # drawn with repetition
    ip.setflags(write=False)
    ix.setflags(write=False)
    return ip, ix


@functools.lru_cache(maxsize=None)
def small_degree_graph():
    """300 rows whose largest in-degree is exactly 64 (one planted row), three isolated rows: a fan-out of 64 keeps every edge."""
    rs = np.random.RandomState(23)
    m = 1800
    src, dst = rs.randint(0, N, m), rs.randint(0, N, m)
    keep = ~np.isin(dst, (8, 77, 150, 211))
    src = np.concatenate([src[keep], rs.randint(0, N, 64), [30, 30]])
    dst = np.concatenate([dst[keep], np.full(64, 150), [31, 31]])
    ip, ix = csr_from_edges(src, dst, N)
    deg = np.diff(ip)
    assert deg.max() == 64 and deg[150] == 64 and deg[8] == deg[77] == deg[211] == 0
    ip.setflags(write=False)
    ix.setflags(write=False)
    return ip, ix


def compact(src, cnt):
    """(indptr int64, indices int32) of sample_neighbors' padded rows: row i keeps its first cnt[i] slots, rows in order."""
    cnt = np.asarray(cnt, np.int64)
    indptr = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(cnt, out=indptr[1:])
    mask = np.arange(src.shape[1])[None, :] < cnt[:, None]
    return indptr, np.ascontiguousarray(src[mask], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def expected(which, fanout, seed, n_dst=N):
    """(indptr, indices, redirected picks) of the sampled graph of rows [0, n_dst) of `which` ("big" / "small"), from the oracle."""
    ip, ix = big_graph() if which == "big" else small_degree_graph()
    src, cnt, n_redirects = so.sample_neighbors(ip[:n_dst + 1], ix, np.arange(n_dst), fanout, seed)
    sp, sx = compact(src, cnt)
    sp.setflags(write=False)
    sx.setflags(write=False)
    return sp, sx, n_redirects


SEED_SALT = 0xFA17


def layer_seed(sample_seed, l):
    """seed_l of SAGE.inference(fan_out=..., sample_seed=...): drop_hash(sample_seed, l, 0xFA17), the seed first."""
    return int(drop_hash(sample_seed, l, SEED_SALT))


def expected_layers(which, fan_out, sample_seed):
    """[(indptr, indices)] per layer of SAGE.inference(fan_out=fan_out, sample_seed=sample_seed) over `which`."""
    return [expected(which, f, layer_seed(sample_seed, l))[:2] for l, f in enumerate(fan_out)]
