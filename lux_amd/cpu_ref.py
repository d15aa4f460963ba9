"""CPU reference engines (whole-graph and per-partition drivers).

These wrap the native golden implementations (src/core/engines.cpp) and add
the same iterate/exchange structure the GPU engines use, so the distributed
exchange layer can be exercised on CPU (gloo) with identical results to the
single-process path.
"""
import numpy as np

from . import _native as nat
from .graph import Graph

INF = np.uint32(0xFFFFFFFF)


def pagerank(g: Graph, iters: int) -> np.ndarray:
    """Whole-graph PageRank; returns rank/out_degree per vertex (the
    reference's stored form, pagerank_gpu.cu:97-100)."""
    return nat.pagerank_cpu(g.nv, g.ne, g.col_end, g.src, iters)


def sssp(g: Graph, source: int):
    return nat.sssp_cpu(g.nv, g.ne, g.col_end, g.src, source)


def cc(g: Graph):
    return nat.cc_cpu(g.nv, g.ne, g.col_end, g.src)


def cf(g: Graph, K: int, iters: int) -> np.ndarray:
    return nat.cf_cpu(g.nv, g.ne, g.col_end, g.src, g.weight, K, iters)


def cf_loss(g: Graph, K: int, vec: np.ndarray) -> float:
    return nat.cf_loss(g.nv, g.ne, g.col_end, g.src, g.weight, K, vec)


def sssp_check(g: Graph, label: np.ndarray) -> int:
    return nat.sssp_check(g.nv, g.ne, g.col_end, g.src, label)


def cc_check(g: Graph, label: np.ndarray) -> int:
    return nat.cc_check(g.nv, g.ne, g.col_end, g.src, label)


def sssp_weighted(g: Graph, source: int) -> np.ndarray:
    """Exact shortest distances over g.weight (non-negative i32), u32 with
    INF for unreachable vertices: binary-heap Dijkstra with the engines'
    saturation, cand = min(label[u] + w, 0xFFFFFFFE)."""
    assert g.weight is not None, "weighted SSSP needs g.weight"
    return nat.sssp_weighted_cpu(
        g.nv, g.ne, g.col_end, g.src,
        np.ascontiguousarray(g.weight, np.int32), source)


def sssp_weighted_check(g: Graph, label: np.ndarray, source: int) -> int:
    """Edges with label[v] > sat(label[u] + w) for finite label[u], plus
    one if label[source] != 0 (PushEngine.check's weighted invariant)."""
    return int(nat.sssp_weighted_check(
        g.nv, g.col_end, g.src, np.ascontiguousarray(g.weight, np.int32),
        np.ascontiguousarray(label, np.uint32), source))


def betweenness(g: Graph, source: int):
    """Single-source Brandes in fp64: (depth u32, sigma f64, delta f64).
    sigma[source] = 1; sigma[v] sums sigma[u] over the in-edges u->v with
    depth[u] == depth[v] - 1; delta[u] sums sigma[u]/sigma[v] *
    (1 + delta[v]) over the out-edges u->v with depth[v] == depth[u] + 1.
    Parallel edges are distinct paths, self-loops never count, unreached
    vertices have depth INF and sigma = delta = 0, delta[source] is 0, and
    nothing is halved for symmetric inputs (BCEngine's conventions)."""
    if not 0 <= source < g.nv:
        raise ValueError(f"source {source} outside [0, {g.nv})")
    return nat.bc_cpu(g.nv, g.ne, g.col_end, g.src, source)


def triangles(g: Graph):
    """Exact triangle counts: (total int, per_vertex u64[nv]) on the
    underlying simple undirected graph — {u,v} is an edge iff u != v and
    u->v or v->u occurs, so parallel edges collapse and self-loops vanish
    (TCEngine's definition). total counts the unordered pairwise-adjacent
    triples, per_vertex[v] those containing v: per_vertex.sum() == 3*total.
    C++ node-iterator count on the id-oriented adjacency; shares no code
    with tc_engine.orient."""
    return nat.tc_cpu(g.nv, g.ne, g.col_end, g.src)


def edge_support(g: Graph):
    """(edges u32[m, 2], support u32[m]) on the simple undirected graph of
    triangles(): edges are (lo, hi) in original ids, sorted by the key
    (lo << 32) | hi; support[e] is the number of triangles containing e, so
    support.sum() == 3 * total."""
    edges, support, _ = nat.truss_cpu(g.nv, g.ne, g.col_end, g.src,
                                      want_truss=False)
    return edges, support


def truss(g: Graph) -> np.ndarray:
    """trussness u32[m] in the edge order of edge_support(): the largest k
    whose k-truss (the largest subgraph whose every edge lies in at least
    k - 2 triangles of the subgraph) contains the edge; 2 for an edge in no
    triangle. C++ sequential bucket-queue peeling: remove an edge of
    minimum support, decrement the other two edges of each of its
    triangles. Shares no schedule with a round-by-round peel (every round
    dropping all edges below k - 2), which must give the same answer."""
    return nat.truss_cpu(g.nv, g.ne, g.col_end, g.src)[2]


def coreness(g: Graph) -> np.ndarray:
    """coreness u32[nv] on the simple undirected graph of triangles(): the
    largest k whose k-core (the largest subgraph in which every vertex has
    degree >= k) contains the vertex; 0 for a vertex with no simple edge.
    coreness.max() is the degeneracy. C++ sequential Batagelj-Zaversnik
    bucket peel, O(m); shares no code with tc_engine.orient and no schedule
    with KCoreEngine's round-by-round peel."""
    return nat.coreness_cpu(g.nv, g.ne, g.col_end, g.src)


def greedy_colouring(g: Graph, order="degree", seed=1) -> np.ndarray:
    """colour i32[nv] on the simple undirected graph of triangles(): the
    sequential greedy colouring in the priority order `order` — degree:
    larger simple degree first, ties by smaller id; id: smaller id first;
    hash: smaller splitmix64(seed ^ v) >> 1 first, ties by smaller id.
    colour[v] is the smallest colour that no neighbour preceding v has, so
    colour == 0 is the lexicographically first maximal independent set. C++,
    one sequential pass over its own adjacency and its own priority
    permutation with a stamp array; shares no code with tc_engine.orient
    and no schedule with ColouringEngine's rounds."""
    return nat.greedy_colouring_cpu(g.nv, g.ne, g.col_end, g.src, order,
                                    seed)


def scc(g: Graph) -> np.ndarray:
    """label u32[nv] of the directed graph as loaded (row v of the CSC lists
    the sources u of the edges u -> v; parallel edges and self-loops change
    nothing): u and v share a label iff each reaches the other, and the
    label is the largest vertex id of the SCC, so label[v] >= v,
    label[label[v]] == label[v], and a vertex alone in its SCC has
    label[v] == v. C++ iterative Tarjan (an explicit call stack); shares no
    schedule with SCCEngine's trim / forward-backward / colouring."""
    return nat.scc_cpu(g.nv, g.ne, g.col_end, g.src)


def msf(g: Graph):
    """The minimum spanning forest of the simple undirected graph of
    triangles(), the weight of {u, v} being the minimum of g.weight over all
    its occurrences in either direction (any i32). Returns (lo u32[m],
    hi u32[m], w i32[m], in_forest bool[m], total int, labels u32[nv]): the
    simple edges ascending by (lo << 32) | hi — the position is the edge id
    e — the forest under the strict order (w, e), its exact total weight,
    and per vertex the largest vertex id of its component. C++ Kruskal over
    its own sorted edge list; shares no code with tc_engine.orient and no
    schedule with MSFEngine's Boruvka rounds."""
    if g.weight is None:
        raise ValueError("msf needs g.weight")
    return nat.msf_cpu(g.nv, g.ne, g.col_end, g.src,
                       np.ascontiguousarray(g.weight, np.int32))


# ---- partitioned iteration (the distributed-CPU compute step) ----

def pagerank_partitioned(g: Graph, nparts: int, iters: int) -> np.ndarray:
    """Multi-partition PageRank in one process — validates that the
    partitioned iteration composes to the whole-graph result."""
    part = g.partition(nparts)
    deg = g.out_degrees()
    old = nat.pagerank_init(g.nv, deg)
    new = np.empty_like(old)
    for _ in range(iters):
        for p in range(nparts):
            if part.verts(p) == 0:
                continue
            rl, rr, cl, ce, src, _ = g.slice(part, p)
            nat.pagerank_iter_part(g.nv, rl, rr, cl, ce, src, deg, old,
                                   new[rl:rr + 1])
        old, new = new, old
    return old


def sssp_partitioned(g: Graph, nparts: int, source: int):
    part = g.partition(nparts)
    old = np.full(g.nv, INF, np.uint32)
    old[source] = 0
    new = np.empty_like(old)
    iters = 0
    while True:
        changed = 0
        for p in range(nparts):
            if part.verts(p) == 0:
                continue
            rl, rr, cl, ce, src, _ = g.slice(part, p)
            changed += nat.sssp_iter_part(rl, rr, cl, ce, src, old,
                                          new[rl:rr + 1])
        iters += 1
        old, new = new, old
        if changed == 0:
            break
    return old, iters


def cf_als(g: Graph, K: int, iters: int, lam: float = 0.001,
           init: "np.ndarray | None" = None,
           n_users: "int | None" = None) -> np.ndarray:
    """Plain-numpy ALS reference: per sweep, for each vertex with in-edges,
    solve (S^T S + lam I) d = S^T w exactly (S = src vectors of the
    in-edges). Vertices with no in-edges keep their old vector. With
    n_users given (bipartite user/item boundary) the sweep ALTERNATES:
    user rows [0, n_users) solve against the old item factors, then item
    rows solve against the UPDATED users — true Gauss-Seidel ALS, matching
    CFALSEngine. Without it, every row solves against old values
    (simultaneous Jacobi). Solved in float64 here, compared with tolerance
    against the fp32 GPU Cholesky path (src/gpu/cf_als.hip)."""
    import math as _math
    if init is not None:
        vec = np.array(init, dtype=np.float32).reshape(g.nv, K).copy()
    else:
        vec = np.full((g.nv, K), _math.sqrt(1.0 / K), dtype=np.float32)
    eye = lam * np.eye(K, dtype=np.float64)

    def _solve_rows(vec, new, lo, hi):
        b = 0 if lo == 0 else int(g.col_end[lo - 1])
        for v in range(lo, hi):
            e = int(g.col_end[v])
            if e > b:
                S = vec[g.src[b:e]].astype(np.float64)
                w = g.weight[b:e].astype(np.float64)
                G = S.T @ S + eye
                new[v] = np.linalg.solve(G, S.T @ w).astype(np.float32)
            b = e

    for _ in range(iters):
        if n_users is None:
            new = vec.copy()
            _solve_rows(vec, new, 0, g.nv)
            vec = new
        else:
            # in-place is exact per phase: a bipartite row only reads the
            # other side's factors
            _solve_rows(vec, vec, 0, n_users)
            _solve_rows(vec, vec, n_users, g.nv)
    return vec
