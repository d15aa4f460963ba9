"""Betweenness-centrality references for test_bc_cpu.py / test_gpu_bc.py.

Numpy only (no GPU, no C++ oracle): a vectorised per-level Brandes, the
hand cases with their closed-form values, the two degree-ladder builders
with theirs, and the tolerance the fp32 results are compared with.
"""
from types import SimpleNamespace

import numpy as np

from degree_ladder import LADDER
from lux_amd.graph import Graph

INF = 0xFFFFFFFF
U = 2.0 ** -24  # fp32 unit roundoff


def edge_lists(g):
    """(src, dst) of every edge in CSC order."""
    deg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    dst = np.repeat(np.arange(g.nv, dtype=np.int64), deg)
    return g.src.astype(np.int64), dst


def brandes(g, source):
    """Per-level Brandes in fp64 over whole edge arrays. Returns
    SimpleNamespace(depth u32, sigma f64, delta f64, levels, dag_edges):
    dag_edges counts the edges u->v with depth[v] == depth[u] + 1, every
    occurrence of a parallel edge on its own."""
    src, dst = edge_lists(g)
    nv = g.nv
    depth = np.full(nv, -1, np.int64)
    depth[source] = 0
    d = 0
    while True:
        new = dst[(depth[src] == d) & (depth[dst] < 0)]
        if new.size == 0:
            break
        d += 1
        depth[new] = d
    levels = d + 1
    dag = (depth[src] >= 0) & (depth[dst] == depth[src] + 1)
    s, t = src[dag], dst[dag]
    sigma = np.zeros(nv, np.float64)
    sigma[source] = 1.0
    for lvl in range(1, levels):
        m = depth[t] == lvl
        sigma += np.bincount(t[m], weights=sigma[s[m]], minlength=nv)
    delta = np.zeros(nv, np.float64)
    for lvl in range(levels - 2, -1, -1):
        m = depth[s] == lvl
        term = sigma[s[m]] / sigma[t[m]] * (1.0 + delta[t[m]])
        delta += np.bincount(s[m], weights=term, minlength=nv)
    delta[source] = 0.0
    return SimpleNamespace(
        depth=np.where(depth < 0, INF, depth).astype(np.uint32),
        sigma=sigma, delta=delta, levels=levels, dag_edges=int(dag.sum()))


def max_degree(g):
    """Larger of the maximum in-degree and the maximum out-degree."""
    indeg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    outdeg = np.bincount(g.src, minlength=g.nv)
    return int(max(indeg.max(initial=0), outdeg.max(initial=0)))


def tolerance(g, depth, expected):
    """(rtol, atol) for fp32 sigma / delta against an fp64 reference.

    A sum of m non-negative fp32 terms in any order is off by at most
    (m-1)u relative, u = 2^-24; each term brings at most 3u of its own
    (ratio, 1 + delta, product); errors compound over at most L levels:
    rtol = 1.01 * L * (maxdeg + 3) * u, atol = rtol * the smallest positive
    expected value."""
    depth = np.asarray(depth)
    reached = depth[depth != INF]
    levels = int(reached.max()) + 1 if reached.size else 1
    rtol = 1.01 * levels * (max_degree(g) + 3) * U
    pos = np.asarray(expected)[np.asarray(expected) > 0]
    return rtol, (rtol * float(pos.min()) if pos.size else 0.0)


def assert_close(got, want, g, depth, what):
    rtol, atol = tolerance(g, depth, want)
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=rtol,
                               atol=atol, err_msg=what)


def assert_sigma_exact(got, want):
    """Path counts below 2^24 are integers every fp32 partial sum holds
    exactly, in any order: asserted on the reference first, then the fp32
    result must equal it."""
    assert want.max() < 2 ** 24 and np.array_equal(want, np.rint(want))
    assert np.array_equal(np.asarray(got, np.float64), want)


# ------------------------------------------------------------ hand cases ----

def _case(name, nv, edges, source=0, **want):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    g = Graph.from_edges(nv, e[:, 0], e[:, 1])
    return SimpleNamespace(name=name, g=g, source=source, want={
        k: np.asarray(v, np.uint32 if k == "depth" else np.float64)
        for k, v in want.items()})


def hand_cases():
    diamond = [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)]
    return [
        _case("chain", 5, [(0, 1), (1, 2), (2, 3), (3, 4)],
              depth=[0, 1, 2, 3, 4], sigma=[1, 1, 1, 1, 1],
              delta=[0, 3, 2, 1, 0]),
        _case("diamond", 5, diamond, depth=[0, 1, 1, 2, 3],
              sigma=[1, 1, 1, 2, 2], delta=[0, 1, 1, 1, 0]),
        # 0->1 twice: two paths into 1, three into 3 and 4;
        # delta[3] = 1, delta[1] = 2/3 * 2, delta[2] = 1/3 * 2
        _case("diamond_doubled", 5, [(0, 1)] + diamond,
              depth=[0, 1, 1, 2, 3], sigma=[1, 2, 1, 3, 3],
              delta=[0, 4 / 3, 2 / 3, 1, 0]),
        # self-loop 1->1, back edge 2->0, component {3, 4} that reaches
        # the rest (3->1) but is not reached
        _case("loop_back_unreached", 5,
              [(0, 1), (1, 1), (1, 2), (2, 0), (3, 4), (4, 3), (3, 1)],
              depth=[0, 1, 2, INF, INF], sigma=[1, 1, 1, 0, 0],
              delta=[0, 1, 0, 0, 0]),
        _case("sink_source", 3, [(1, 0), (1, 2)],
              depth=[0, INF, INF], sigma=[1, 0, 0], delta=[0, 0, 0]),
    ]


# --------------------------------------------------------------- ladders ----

POOL = 256


def in_ladder(seed=3):
    """Forward roles at every bin edge. Source 0 -> a pool of 256 vertices;
    row i has LADDER[i] in-edges drawn with replacement from the pool and
    one out-edge to a private sink. Every pool vertex has sigma 1, so
    sigma[row i] = sigma[sink i] = LADDER[i] exactly; delta[row] = 1 and
    delta[pool p] = sum over its edges p -> row i of 2 / LADDER[i]. The
    degree-0 row and its sink are unreached."""
    rng = np.random.default_rng(seed)
    n = len(LADDER)
    pool = 1 + np.arange(POOL)
    rows = 1 + POOL + np.arange(n)
    sinks = rows + n
    nv = 1 + POOL + 2 * n
    src = [np.zeros(POOL, np.int64), rows]
    dst = [pool, sinks]
    pool_delta = np.zeros(nv, np.float64)
    for i, d in enumerate(LADDER):
        s = rng.integers(1, 1 + POOL, d)
        src.append(s)
        dst.append(np.full(d, rows[i]))
        if d:
            np.add.at(pool_delta, s, 2.0 / d)
    g = Graph.from_edges(nv, np.concatenate(src), np.concatenate(dst))
    lad = np.asarray(LADDER, np.float64)
    live = lad > 0
    depth = np.full(nv, INF, np.uint32)
    depth[0], depth[pool] = 0, 1
    depth[rows[live]], depth[sinks[live]] = 2, 3
    sigma = np.zeros(nv, np.float64)
    sigma[0], sigma[pool] = 1, 1
    sigma[rows], sigma[sinks] = lad, lad
    delta = pool_delta
    delta[rows[live]] = 1.0
    return SimpleNamespace(g=g, source=0, rows=rows, sinks=sinks, pool=pool,
                           depth=depth, sigma=sigma, delta=delta, levels=4)


def out_ladder():
    """Backward roles at every bin edge. Source 0 -> row i, which has
    LADDER[i] out-edges to private leaves. Every sigma is 1 and every q an
    integer, so delta[row i] = LADDER[i] exactly in fp32 in any order."""
    n = len(LADDER)
    rows = 1 + np.arange(n)
    total = int(np.sum(LADDER))
    nv = 1 + n + total
    leaves = 1 + n + np.arange(total)
    g = Graph.from_edges(nv, np.concatenate([np.zeros(n, np.int64),
                                             np.repeat(rows, LADDER)]),
                         np.concatenate([rows, leaves]))
    depth = np.full(nv, 2, np.uint32)
    depth[0], depth[rows] = 0, 1
    sigma = np.ones(nv, np.float64)
    delta = np.zeros(nv, np.float64)
    delta[rows] = LADDER
    return SimpleNamespace(g=g, source=0, rows=rows, leaves=leaves,
                           depth=depth, sigma=sigma, delta=delta, levels=3)


def deep_chain(n=300, fan=2100):
    """More than 256 levels (3 * levels keys no longer fit the order
    kernels' LDS table) with a hub in either direction: chain 0 -> 1 -> ...
    -> n-1, the last chain vertex -> `fan` leaves, every leaf -> one sink.
    sigma is 1 up to the leaves and `fan` at the sink; delta[leaf] = 1/fan,
    delta[n-1] = fan + 1, and one more per step up the chain."""
    chain = np.arange(n)
    leaves = n + np.arange(fan)
    sink = n + fan
    nv = sink + 1
    g = Graph.from_edges(
        nv, np.concatenate([chain[:-1], np.full(fan, n - 1), leaves]),
        np.concatenate([chain[1:], leaves, np.full(fan, sink)]))
    depth = np.concatenate([chain, np.full(fan, n), [n + 1]]).astype(
        np.uint32)
    sigma = np.ones(nv, np.float64)
    sigma[sink] = fan
    delta = np.zeros(nv, np.float64)
    delta[leaves] = 1.0 / fan
    delta[chain[1:]] = fan + 1 + np.arange(n - 2, -1, -1)
    return SimpleNamespace(g=g, source=0, depth=depth, sigma=sigma,
                           delta=delta, levels=n + 2)


# ------------------------------------------------------------------ RMAT ----

RMATS = [(10, 8000, 3), (12, 300000, 5)]  # (scale, ne, seed)


def second_source(g, depth):
    """The reached vertex with the smallest non-zero out-degree, largest id
    on ties."""
    outdeg = np.bincount(g.src, minlength=g.nv)
    ok = np.nonzero((np.asarray(depth) != INF) & (outdeg > 0))[0]
    low = outdeg[ok].min()
    return int(ok[outdeg[ok] == low].max())
