"""Prescribed-degree graphs and plain references for the bin-edge tests.

The degree bins shared by pull.hip, cf.hip and cf_als.hip switch kernels at
in-degree T1=32 and T2=2048 and split hubs into 8192-edge chunks. The
generators (RMAT, bipartite) only hit those edges by luck, so the tests in
test_gpu_cf_ladder.py / test_gpu_pull_ladder.py build graphs from an
explicit in-degree list instead. Rows are emitted in dst order and
Graph.from_edges is a stable counting sort, so the host CSC edge order is
the emission order, and DeviceCSC.from_host keeps it: tile and chunk
positions of every edge are known on both sides.

Everything here is numpy only (no GPU); tests/test_degree_ladder.py runs
the references and the checks' own self-tests on the CPU.
"""
from types import SimpleNamespace

import numpy as np

from lux_amd.graph import Graph

T1, T2, CHUNK_EDGES = 32, 2048, 8192
INF = 0xFFFFFFFF
CF_GAMMA = float(np.float32(0.00000035))  # the kernels' fp32 constant
CF_LAMBDA = 0.001

# thread bin (deg < T1) and the 4-deep gather_range pipeline at step 1
LADDER_THREAD = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 31]
# wave bin (T1 <= deg < T2): lane stride 64 (x4 pipeline = 256), ALS/CF LDS
# tiles of 32 / 64. 34 / 66 / 98 leave a ragged tile of 2 (mod 4), the one
# remainder class of the tiles' 4-wide inner loops the others never hit.
LADDER_WAVE = [32, 33, 34, 63, 64, 65, 66, 95, 96, 97, 98, 127, 128, 129,
               191, 192, 193, 255, 256, 257, 2047]
# chunk bin (deg >= T2): block stride 256 (x4 pipeline = 1024; a thread
# enters the pipelined loop once 768 edges lie past its own), 8192-edge
# chunks, 1 / 2 / 3 / 4 chunks per row
LADDER_CHUNK = [2048, 2049, 2050, 8191, 8192, 8193, 8192 + 255, 8192 + 256,
                8192 + 257, 8192 + 768, 8192 + 769, 8192 + 1023,
                8192 + 1024, 8192 + 1025, 16384, 16385, 24577]
LADDER = LADDER_THREAD + LADDER_WAVE + LADDER_CHUNK


def marker_position(deg, where):
    """Edge index inside a row of in-degree `deg` (> 0) for a marker."""
    if where == "first":
        return 0
    if where == "last":
        return deg - 1
    if where == "chunk_last":   # last edge of the row's first chunk
        return min(deg, CHUNK_EDGES) - 1
    if where == "chunk_first":  # first edge of the row's last chunk
        return ((deg - 1) // CHUNK_EDGES) * CHUNK_EDGES
    raise ValueError(where)


def _csc(nv, degs, srcs, weight=None):
    dst = np.repeat(np.arange(nv, dtype=np.uint32), degs)
    src = np.concatenate(srcs).astype(np.uint32) if srcs else \
        np.zeros(0, np.uint32)
    g = Graph.from_edges(nv, src, dst, weight)
    # the whole point of this module: edge order == emission order
    assert np.array_equal(g.src, src)
    assert np.array_equal(g.col_end, np.cumsum(degs).astype(np.uint64))
    return g, dst


# ---------------------------------------------------------------- plain ----

PLAIN_NV = 512
PLAIN_SHIFT = 6           # 64-vertex src windows -> 8 windows, 4 non-empty
PLAIN_ROWS = 256          # dst rows [0, 256): ladder first, then filler
PLAIN_POOL_BLOCKS = 4     # src pool [256, 512) = 4 windows of 64


def plain_ladder(marker=None, seed=5):
    """Unweighted ladder graph for the pull kernels.

    Rows [0, len(LADDER)) carry the ladder degrees; rows up to 256 are
    low-degree filler; vertices [256, 512) are the source pool and have no
    in-edges. Ladder row i draws every source from pool window i % 4 (one
    2^PLAIN_SHIFT src block), so in the src-blocked CSC its block-local
    degree is still the ladder degree. The last vertex of each pool window
    is a MARKER that random draws never pick: with marker=<where> each
    non-empty ladder row gets its window's marker at exactly one edge,
    marker_position(deg, where). Filler rows draw from all windows."""
    rng = np.random.default_rng(seed)
    w64 = 1 << PLAIN_SHIFT
    pool0 = PLAIN_NV - PLAIN_POOL_BLOCKS * w64
    degs = np.zeros(PLAIN_NV, np.int64)
    degs[:len(LADDER)] = LADDER
    fill = np.arange(len(LADDER), PLAIN_ROWS)
    degs[fill] = (5 * fill) % 23
    markers = pool0 + w64 * np.arange(PLAIN_POOL_BLOCKS) + (w64 - 1)
    regular = np.setdiff1d(np.arange(pool0, PLAIN_NV), markers)
    row_block = np.full(PLAIN_NV, -1, np.int64)
    srcs = []
    for v in range(PLAIN_NV):
        d = int(degs[v])
        if v < len(LADDER):
            blk = v % PLAIN_POOL_BLOCKS
            row_block[v] = blk
            s = pool0 + blk * w64 + rng.integers(0, w64 - 1, d)
            if marker is not None and d > 0:
                s[marker_position(d, marker)] = markers[blk]
        else:
            s = regular[rng.integers(0, len(regular), d)]
        srcs.append(s)
    g, dst = _csc(PLAIN_NV, degs, srcs)
    return SimpleNamespace(g=g, dst=dst, degs=degs, markers=markers,
                           row_block=row_block, pool0=pool0,
                           ladder_rows=np.arange(len(LADDER)))


def pull_sum_ref(lad, old):
    """Per-row sum of old[src] in f64 (exact for small-integer `old`)."""
    g = lad.g
    return np.bincount(lad.dst, weights=np.asarray(old, np.float64)[g.src],
                       minlength=g.nv)


def pull_min_ref(lad, old):
    """Hop relaxation: settled rows keep their label; INF never wraps."""
    g = lad.g
    old = np.asarray(old, np.uint64)
    m = np.where(old[g.src] == INF, INF, old[g.src] + 1)
    best = np.full(g.nv, INF, np.uint64)
    np.minimum.at(best, lad.dst, m)
    return np.where(old != INF, old, best).astype(np.uint32)


def pull_max_ref(lad, old):
    g = lad.g
    old = np.asarray(old, np.uint64)
    best = old.copy()
    np.maximum.at(best, lad.dst, old[g.src])
    return best.astype(np.uint32)


# ------------------------------------------------------------ bipartite ----

def bipartite_ladder(nu=128, ni=128, seed=7):
    """Weighted two-sided ladder for the CF kernels: users [0, nu) draw
    sources from the items [nu, nu+ni) and vice versa; BOTH sides carry the
    whole ladder (so both have hubs) followed by low-degree filler. Weights
    are integers 1..5. nu, ni >= 96 keeps hub Grams full rank for K <= 64."""
    assert nu >= 96 and ni >= 96 and min(nu, ni) >= len(LADDER)
    rng = np.random.default_rng(seed)
    nv = nu + ni
    degs = np.zeros(nv, np.int64)
    for lo, n in ((0, nu), (nu, ni)):
        degs[lo:lo + len(LADDER)] = LADDER
        fill = np.arange(len(LADDER), n)
        degs[lo + fill] = (7 * fill) % 41
    srcs = []
    for v in range(nv):
        d = int(degs[v])
        srcs.append(rng.integers(nu, nv, d) if v < nu
                    else rng.integers(0, nu, d))
    weight = rng.integers(1, 6, int(degs.sum())).astype(np.int32)
    g, dst = _csc(nv, degs, srcs, weight)
    assert np.array_equal(g.weight, weight)
    return SimpleNamespace(g=g, dst=dst, degs=degs, nu=nu, ni=ni)


def int_factors(nv, K, mod=7):
    """Small-integer factors (0..mod-1) that differ by vertex and by
    dimension: exact in fp32 and bf16, so sums over them are exact. A
    multiplicative hash rather than (31*u + 17*k) % 7, which repeats with
    period 7 in u and would hide a gather from vertex u + 7."""
    u = np.arange(nv, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    h = (u * 2654435761 + k * 40503 + u * k * 97 + 12345) & 0xFFFFFFFF
    return ((h >> 7) % mod).astype(np.float32)


def rand_factors(nv, K, seed):
    """The realistic regime of the CF tests: 0.1*N(0,1) + 0.1."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nv, K)) * 0.1 + 0.1).astype(np.float32)


def _rows(g):
    b = 0
    for v in range(g.nv):
        e = int(g.col_end[v])
        yield v, b, e
        b = e


def sgd_gradient_ref(g, old):
    """f64 SGD gradient per dst row: err_e = w_e - <s_e, d>,
    acc = sum_e err_e * s_e, and its absolute-sum scale
    A = sum_e |err_e| |s_e|. With integer factors and zero dst vectors every
    term is an integer far below 2^53, so acc is exact."""
    old = np.asarray(old, np.float64)
    acc = np.zeros_like(old)
    scale = np.zeros_like(old)
    for v, b, e in _rows(g):
        if e > b:
            S = old[g.src[b:e]]
            err = g.weight[b:e].astype(np.float64) - S @ old[v]
            acc[v] = err @ S
            scale[v] = np.abs(err) @ np.abs(S)
    return acc, scale


def hub_gram_ref(g, v, F):
    """int64 upper-triangular 64x64 Gram S^T S and rhs S^T w of row v for
    integer-valued factors F (dims >= K are zero padding)."""
    b = 0 if v == 0 else int(g.col_end[v - 1])
    e = int(g.col_end[v])
    K = F.shape[1]
    S = np.asarray(F, np.float64)[g.src[b:e]]  # ints: f64 matmul is exact
    G = np.zeros((64, 64), np.int64)
    G[:K, :K] = np.rint(S.T @ S).astype(np.int64)
    rhs = np.zeros(64, np.int64)
    rhs[:K] = np.rint(S.T @ g.weight[b:e].astype(np.float64))
    return np.triu(G), rhs


# Bounds of the SGD gradient checks. `got` is newv / CF_GAMMA from a sweep
# into a ZEROED newv: the kernels only do newv += gamma * acc.

SGD_EXACT_RTOL = 1e-6   # gamma multiply (2^-24) + up to 4 chunk atomics
#                         (3 more roundings): < 2.4e-7; one dropped weight-1
#                         edge at degree 24577 moves acc by >= 8e-6
SGD_RAND_RTOL = 1e-4    # of A_k; sequential fp32 at degree 24577: 4.8e-6


def sgd_exact_bad_rows(got, acc):
    """Rows violating |got - acc| <= 1e-6 * acc (acc >= 0 exact ints)."""
    return np.nonzero((np.abs(got - acc) > SGD_EXACT_RTOL * acc).any(1))[0]


def sgd_rand_bad_rows(got, acc, scale):
    """Rows violating |got - acc|_k <= 1e-4 * A_k."""
    return np.nonzero((np.abs(got - acc) > SGD_RAND_RTOL * scale).any(1))[0]
