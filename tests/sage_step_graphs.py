"""Hand-written two-block batches for the kernel-level checks of the SAGE "gcn" step (csrc/spmm.hip): every row class the step's
aggregation kernels branch on is planted at a known id and asserted from the arrays that are returned.  numpy only: the GPU tests and
the CPU test share one builder.

The constants below restate csrc/spmm.hip (kLongRow, kHubRow, kHubSeg, kBlock, kShortRows, kShortUnits, the two-unit batch of
spmm_bn_dy_kernel, GLNN_LONG_BLOCK_ROWS / _CAP, kRowsPerWave); tests/test_sage_step_kernels_gpu.py holds the two the library exports
(glnn_hub_row_threshold, glnn_hub_segment_edges) against them."""
import numpy as np

from graphgen import csr_from_edges
from sampling_oracle import csr_transpose

LONG_ROW, HUB_ROW, HUB_SEG, SCAN = 128, 1024, 512, 512
SHORT_ROWS, SHORT_UNITS, DY_UNITS = 4, 3, 2
LONG_BLOCK_ROWS, LONG_BLOCK_CAP, ROWS_PER_WAVE, WAVES = 512, 512, 16, 8
PLANTED_DEGREES = (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 63, 64, 65, 128, 129, 700, 1100)
N_SRC0, N_DST0, N_DST1 = 6000, 2531, 1203


def lpr_of(d):
    """Lanes per row of the gather kernels for rows of d floats (4 only in the public kernel and the tail gather)."""
    dv = (d + 3) // 4
    return 4 if dv <= 4 else 8 if dv <= 8 else 16 if dv <= 16 else 32 if dv <= 32 else 64


def row_geometry(n_dst, min_rows_per_wave=1):
    """(n_chunks of the long-row scan, n_long_blocks, rows_per_block) of a launch over n_dst rows: spmm_impl (min 1 row per wave) and
    bn_dy_grid (min 4)."""
    n_chunks = -(-n_dst // SCAN)
    n_long = min(max(-(-n_dst // LONG_BLOCK_ROWS), 1), LONG_BLOCK_CAP)
    rpw = min(max(n_dst // (2048 * WAVES), min_rows_per_wave), ROWS_PER_WAVE)
    return n_chunks, n_long, WAVES * rpw


def _block(rs, n_src, n_dst, ordinary_max, dst_deg, src_deg=None):
    """A block whose planted destinations `dst_deg` {row: in-degree} and planted sources `src_deg` {id: out-degree} have EXACT degrees:
    the planted edges' other ends and both ends of the random edges (0 .. ordinary_max per unplanted destination) are unplanted."""
    src_deg = src_deg or {}
    deg = rs.randint(0, ordinary_max + 1, n_dst)
    pd = np.array(sorted(dst_deg), np.int64)
    ps = np.array(sorted(src_deg), np.int64)
    assert not set(pd) & set(ps)
    deg[pd] = 0
    pool_src = np.setdiff1d(np.arange(n_src), ps)
    pool_dst = np.setdiff1d(np.arange(n_dst), np.concatenate([pd, ps[ps < n_dst]]))
    dst = [np.repeat(np.arange(n_dst), deg)]
    src = [rs.choice(pool_src, int(deg.sum()))]
    for r in pd:
        dst.append(np.full(dst_deg[r], r))
        src.append(rs.choice(pool_src, dst_deg[r]))
    for u in ps:
        src.append(np.full(src_deg[u], u))
        dst.append(rs.choice(pool_dst, src_deg[u]))
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rs.permutation(len(src))                      # (a row's edges in no particular source order)
    return csr_from_edges(src[perm], dst[perm], n_dst)


def ticket_rows(indptr, v0, lpr, n_dst=None, rows_per_block=8):
    """What spmm_csr_short_kernel does with the ticket of rows v0 .. v0 + 3: per row one of 'batch' (whole row inside the batch),
    'tail' (first units in the batch, the rest carried on), 'lone' (its first units lie behind the 64 loaded indices), 'long' (left to
    the long-row role), 'absent' (behind n_dst)."""
    n_dst = len(indptr) - 1 if n_dst is None else n_dst
    g = 64 // lpr
    nr = min(SHORT_ROWS, n_dst - v0, rows_per_block - v0 % rows_per_block)
    tot = min(int(indptr[v0 + nr] - indptr[v0]), 64)
    out = []
    for r in range(SHORT_ROWS):
        if r >= nr:
            out.append("absent")
            continue
        deg, off = int(indptr[v0 + r + 1] - indptr[v0 + r]), min(int(indptr[v0 + r] - indptr[v0]), 64)
        h = min(deg, SHORT_UNITS * g)
        out.append("long" if deg > LONG_ROW else "lone" if off + h > tot else "batch" if deg <= h else "tail")
    return out


# where the planted rows sit
LONE_TICKET, LONG_TICKET = 1000, 1500                   # block 0: first rows of the two special four-row tickets
DST0 = {0: 16, 1: 17, 2: 33, 3: 34, 4: 51, 5: 66, 6: 83, 7: N_DST0 - 1, 12: 100, 13: N_DST0 - 2, 63: 117, 64: 134, 65: 151, 128: 168,
        129: LONG_TICKET + 1, 700: 202, 1100: 219}
DST1 = {0: 20, 1: 37, 2: 54, 3: 71, 4: 88, 5: 105, 6: 122, 7: N_DST1 - 1, 12: 139, 13: N_DST1 - 2, 63: 156, 64: 173, 65: 190, 128: 207,
        129: 224, 700: 241, 1100: 258}
# block 1's sources = the rows of the transposed block (a self entry for ids < N_DST1): {id: out-degree}
SRC1_INSIDE = {300: 0, 301: 1, 302: 2, 303: 3, 304: 4, 305: 5, 310: 128}                                      # entries = out-degree + 1
SRC1_OUTSIDE = {2000: 0, 2001: 1, 2002: 2, 2004: 3, 2005: 4, 2006: 5, 2010: 64, 2011: 65, 2012: 128, 2013: 129,   # entries = out-degree
                1303: 700, 1808: 300, 2503: 1100}       # ... the last three and 2013: long rows with id % 5 == 3, ids not in thread order


def planted_batch(seed=0):
    """dict(blocks=[(indptr, indices, n_src)] * 2, dst=[{degree: row}] * 2, src1={id: out-degree}, t1=(t_indptr, t_indices)): block 0 of
    6000 sources over 2531 destinations (sparse: the short-row kernel's condition), block 1 of 2531 over 1203."""
    rs = np.random.RandomState(seed)
    d0 = {row: deg for deg, row in DST0.items()}
    d0.update({LONE_TICKET: 60, LONE_TICKET + 1: 3, LONE_TICKET + 2: 5, LONE_TICKET + 3: 2,      # rows 2 (and 3) lie behind index 64
               LONG_TICKET: 2, LONG_TICKET + 2: 3, LONG_TICKET + 3: 4})
    ip0, ix0 = _block(rs, N_SRC0, N_DST0, 7, d0)
    src1 = {**SRC1_INSIDE, **SRC1_OUTSIDE}
    ip1, ix1 = _block(rs, N_DST0, N_DST1, 10, {row: deg for deg, row in DST1.items()}, src1)
    t_ip, t_ix, _ = csr_transpose(ip1, ix1, N_DST1, N_DST0, add_self=True)
    b = dict(blocks=[(ip0, ix0, N_SRC0), (ip1, ix1, N_DST0)], dst=[dict(DST0), dict(DST1)], src1=src1, t1=(t_ip, t_ix))
    check_planted_batch(b)
    return b


def check_planted_batch(b):
    """Every class the builder plants, asserted from the arrays it returns."""
    (ip0, ix0, ns0), (ip1, ix1, ns1) = b["blocks"]
    assert (ns0, len(ip0) - 1, ns1, len(ip1) - 1) == (N_SRC0, N_DST0, N_DST0, N_DST1)
    assert N_DST0 % SHORT_ROWS == 3 and N_DST0 % 32 == 3          # a ragged four-row ticket; a ragged 32-row workgroup in the backward
    for (ip, ix, ns), planted in zip(b["blocks"], b["dst"]):
        assert ip[0] == 0 and ip[-1] == len(ix) and ix.min() >= 0 and ix.max() < ns
        deg = np.diff(ip)
        assert sorted(planted) == sorted(PLANTED_DEGREES) and all(deg[row] == d for d, row in planted.items())
        assert LONG_ROW in planted and LONG_ROW + 1 in planted                     # the last one-wave row, the first long row
        assert max(planted) > HUB_ROW and -(-max(planted) // HUB_SEG) == 3 and max(planted) % HUB_SEG != 0      # three segments, ragged
    assert len(ix0) <= 6 * N_DST0                                                  # the short-row kernel's condition
    # the short kernel's tickets (rows_per_block = 8 at this size): both lane layouts see a lone row behind a 60-edge row, a skipped
    # long row, carried tails, whole-batch rows and the ragged last ticket
    assert row_geometry(N_DST0)[2] == 8
    for lpr in (32, 64):
        assert ticket_rows(ip0, LONE_TICKET, lpr)[2] == "lone" and int(np.diff(ip0)[LONE_TICKET]) == 60
        assert ticket_rows(ip0, LONG_TICKET, lpr)[1] == "long" and "long" not in ticket_rows(ip0, LONG_TICKET, lpr)[::2]
        assert ticket_rows(ip0, N_DST0 - 3, lpr) == [ticket_rows(ip0, N_DST0 - 3, lpr)[0], "tail", "tail", "absent"]
        kinds = {k for v0 in range(0, N_DST0, SHORT_ROWS) for k in ticket_rows(ip0, v0, lpr)}
        assert kinds == {"batch", "tail", "lone", "long", "absent"}
    # the transposed block of layer 1
    t_ip, t_ix = b["t1"]
    tlen = np.diff(t_ip)
    out = np.bincount(ix1, minlength=N_DST0)
    assert len(tlen) == N_DST0 and np.array_equal(tlen, out + (np.arange(N_DST0) < N_DST1))
    assert all(out[u] == d for u, d in b["src1"].items())
    assert tlen[2000] == 0 and tlen[300] == 1                                      # an empty row; a row that is its self entry alone
    for lpr in (32, 64):                                                           # just inside / just over spmm_bn_dy_kernel's batch
        unit = DY_UNITS * 64 // lpr
        assert {unit, unit + 1} <= set(tlen[list(b["src1"])])
    assert {1, 2, 3, 4, 5, 6, 64, 65, 128, 129, 300, 700, 1100} <= set(tlen[list(b["src1"])])
    long_rows = np.flatnonzero(tlen > LONG_ROW)
    n_chunks = row_geometry(N_DST0, 4)[0]
    assert n_chunks == 5 and np.bincount(long_rows % n_chunks, minlength=n_chunks)[3] >= 3      # one scan chunk finds >= 3 long rows
    same = long_rows[long_rows % n_chunks == 3]
    assert np.any(np.diff(tlen[same]) < 0)                                         # ... of different lengths, not in ascending-work order
    assert (tlen > HUB_ROW).sum() == 1


def global_ids(b, n_global, seed=1):
    """(input_nodes, gindices, dst_nodes) as NodeDataLoader sets them on the outermost block: the block's sources are the distinct global
    ids input_nodes (its destinations first), gindices the edges' global source ids."""
    rs = np.random.RandomState(seed)
    ip0, ix0, ns0 = b["blocks"][0]
    input_nodes = rs.permutation(n_global)[:ns0].astype(np.int64)
    return input_nodes, input_nodes[ix0].astype(np.int32), input_nodes[:len(ip0) - 1].copy()


# ------------------------------------------------------------------------------------------------ the large launch geometry
BIG_DST1, BIG_SRC1, BIG_SRC0 = 262800, 262900, 263000


def second_trip_rows(n):
    """Row ids whose scan chunk (r % n_chunks) is taken on a workgroup's SECOND trip (chunk >= n_long_blocks), spread over the threads."""
    n_chunks, n_long, _ = row_geometry(n)
    assert n_chunks == 514 and n_long == 512
    return [k * n_chunks + c for k, c in ((3, 512), (200, 513), (505, 512), (77, 513))]


def large_batch(seed=0):
    """Block 1 of 262 800 destinations over 262 900 sources, block 0 of 262 900 over 263 000 (about three in-edges per row): 16 rows per
    wave, a ragged last workgroup, 514 scan chunks for 512 long-role workgroups; long rows on the second trip among the destinations of
    both blocks and the sources of block 1."""
    rs = np.random.RandomState(seed)
    late1, late_s = second_trip_rows(BIG_DST1), second_trip_rows(BIG_SRC1)
    d1 = dict(zip(late1, (300, 129, 190, 1100)))
    d1.update({40: 700, 41: 128})
    s1 = {u + 514 * 2: d for u, d in zip(late_s, (260, 129, 500, 1100))}
    s1.update({100000: 128, 262850: 200})
    ip1, ix1 = _block(rs, BIG_SRC1, BIG_DST1, 5, d1, s1)
    d0 = dict(zip(second_trip_rows(BIG_SRC1), (300, 129, 190, 1100)))
    ip0, ix0 = _block(rs, BIG_SRC0, BIG_SRC1, 5, d0)
    t_ip, t_ix, _ = csr_transpose(ip1, ix1, BIG_DST1, BIG_SRC1, add_self=True)
    b = dict(blocks=[(ip0, ix0, BIG_SRC0), (ip1, ix1, BIG_SRC1)], dst=[d0, d1], src1=s1, t1=(t_ip, t_ix))
    check_large_batch(b)
    return b


def check_large_batch(b):
    (ip0, ix0, _), (ip1, ix1, _) = b["blocks"]
    for n, min_rpw in ((BIG_DST1, 1), (BIG_SRC1, 1), (BIG_SRC1, 4)):
        n_chunks, n_long, rpb = row_geometry(n, min_rpw)
        assert (n_chunks, n_long, rpb) == (514, 512, 128) and n % rpb != 0         # 16 rows per wave, ragged last workgroup, two trips
    assert len(ix0) <= 6 * BIG_SRC1
    for ip, planted in ((ip0, b["dst"][0]), (ip1, b["dst"][1])):
        deg = np.diff(ip)
        assert all(deg[r] == d for r, d in planted.items())
        late = [r for r in planted if r % 514 >= 512 and deg[r] > LONG_ROW]
        assert {r % 514 for r in late} == {512, 513} and any(deg[r] > HUB_ROW for r in late)
    tlen = np.diff(b["t1"][0])
    assert all(tlen[u] == d + (u < BIG_DST1) for u, d in b["src1"].items())
    late = [u for u in b["src1"] if u % 514 >= 512 and tlen[u] > LONG_ROW]
    assert {u % 514 for u in late} == {512, 513} and any(tlen[u] > HUB_ROW for u in late)


def big_graph_for_public_spmm(n=BIG_DST1, seed=3):
    """A square graph of n rows for ops.spmm at the large geometry: long rows (one of them a hub row) on the scan's second trip."""
    rs = np.random.RandomState(seed)
    planted = dict(zip(second_trip_rows(n), (300, 129, 190, 1100)))
    planted.update({40: 700, 41: 128, 42: 0})
    ip, ix = _block(rs, n, n, 5, planted)
    deg = np.diff(ip)
    assert all(deg[r] == d for r, d in planted.items())
    assert {r % 514 for r in planted if deg[r] > LONG_ROW and r % 514 >= 512} == {512, 513}
    return ip, ix, planted


# ------------------------------------------------------------------------------------------------ the cases of the kernel tests
N_CLASSES = 7
F_STEP = 68                                               # > 64: layer 0 takes the short-row kernel, dW_0 the deferred BatchNorm apply
TAIL_H = (3, 16, 20, 30, 32, 36, 50, 64, 68, 100, 128, 132, 255, 256)       # both ends of LPR 4 | 8 | 16 | 32 | 64, widths with h % 4 != 0
SHORT_F = (68, 100, 128, 130, 200, 256)                   # LPR 32 | 64
BN_DY_H = (68, 100, 128, 132, 200, 256)
LN_DZ_H = (3, 30, 32, 36, 50, 64, 68, 100, 128, 132, 255, 256)
NORMS, PS = ("batch", "none", "layer"), (0.0, 0.3)
# seed of a case's parameters and features where 0 does not pass test_relu_gates_are_decided_for_every_seed_the_gpu_tests_use: the first
# seed for which NO element of the fp32 CPU oracle's layer-0 pre-activation lies within 64 gate margins of zero (found by a search with
# that test's gate_margins(); about one seed in a hundred passes at h = 256, where five such elements are expected)
SEEDS = {(68, 20, "layer"): 2, (68, 30, "batch"): 1, (68, 30, "layer"): 1, (68, 32, "batch"): 4, (68, 36, "layer"): 1, (68, 64, "batch"): 9,
         (68, 64, "layer"): 4, (68, 68, "layer"): 4, (68, 100, "batch"): 10, (68, 100, "layer"): 12, (68, 128, "batch"): 13,
         (68, 128, "layer"): 27, (68, 132, "batch"): 3, (68, 132, "layer"): 43, (68, 255, "batch"): 5, (68, 255, "layer"): 30,
         (68, 256, "batch"): 58, (68, 256, "layer"): 34, (68, 200, "batch"): 9}


def case_seed(f, h, norm):
    return SEEDS.get((f, h, norm), 0)


def all_cases():
    """Every (f, h, norm) the GPU tests run."""
    cases = [(F_STEP, h, norm) for h in TAIL_H for norm in NORMS] + [(f, 16, "none") for f in SHORT_F]
    return cases + [(F_STEP, h, "batch") for h in BN_DY_H] + [(F_STEP, h, "layer") for h in LN_DZ_H]


def case_inputs(f, h, norm, n_rows=N_SRC0, n_out=N_DST1, seed=None):
    """(x [n_rows, f] float32, labels [n_out] int64, state dict of float32 arrays keyed like the model's) of a two-layer f -> h -> 7
    teacher: weights of the usual 1 / sqrt(fan-in) size, a norm weight in [0.5, 1.5] and bias in [-0.2, 0.2]."""
    rs = np.random.RandomState(1000 + (case_seed(f, h, norm) if seed is None else seed))
    x = rs.standard_normal((n_rows, f)).astype(np.float32)
    labels = rs.randint(0, N_CLASSES, n_out).astype(np.int64)
    sd = {}
    for l, (i, o) in enumerate(((f, h), (h, N_CLASSES))):
        sd[f"encoder.layers.{l}.fc_neigh.weight"] = (rs.uniform(-1, 1, (o, i)) * (3.0 / i) ** 0.5).astype(np.float32)
        sd[f"encoder.layers.{l}.fc_neigh.bias"] = rs.uniform(-0.1, 0.1, o).astype(np.float32)
    if norm != "none":
        sd["encoder.norms.0.weight"] = rs.uniform(0.5, 1.5, h).astype(np.float32)
        sd["encoder.norms.0.bias"] = rs.uniform(-0.2, 0.2, h).astype(np.float32)
    return x, labels, sd


def backward_planted_rows(b):
    """The rows of the backward kernels' outputs that were planted: the planted sources of block 1 and the ragged last workgroup."""
    n = b["blocks"][1][2]
    return sorted(set(b["src1"]) | {n - 3, n - 2, n - 1})
