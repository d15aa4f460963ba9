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


def cliques(g: Graph, k: int):
    """Exact k-clique counts, 3 <= k <= 8: (total int, per_vertex u64[nv])
    on the simple undirected graph of triangles() (CliqueEngine's
    definition). total counts the k-subsets of pairwise adjacent vertices,
    per_vertex[v] those containing v: per_vertex.sum() == k * total. C++
    recursive search on the id-oriented adjacency that narrows sorted
    candidate lists with two-pointer merges; no bit sets, no degree order,
    no code shared with tc_engine.orient."""
    if not 3 <= k <= 8:
        raise ValueError(f"k must be in 3..8, got {k}")
    return nat.cliques_cpu(g.nv, g.ne, g.col_end, g.src, k)


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


def label_propagation(g: Graph, order="degree", seed=1, init=None,
                      max_sweeps=0):
    """(labels i32[nv], [(sweep, evaluated, changed)]) on the simple
    undirected graph of triangles(): semi-synchronous label propagation, the
    sequential pass in (greedy_colouring(order, seed), id) order of API.md.
    label[v] starts as v or init[v]; a dirty vertex with a neighbour takes
    the smallest most frequent label of its neighbours unless its own is as
    frequent, and then marks its neighbours dirty. Ends after the first
    sweep without a change, or after max_sweeps sweeps if max_sweeps > 0.
    C++, one sequential loop sorting each row; no roles, no tables, no
    classes."""
    return nat.label_propagation_cpu(g.nv, g.ne, g.col_end, g.src, order,
                                     seed, init, max_sweeps)


def modularity(intra, m, tot):
    """intra / m - sum(tot[l]^2) / (4 m^2) from exact integers (tot: an
    iterable of ints), 0.0 for m == 0."""
    from fractions import Fraction
    if m == 0:
        return 0.0
    return float(Fraction(int(intra), m) -
                 Fraction(sum(int(t) * int(t) for t in tot), 4 * m * m))


def community_stats(g: Graph, labels):
    """dict(m, sizes i64[nv], tot i64[nv], intra, modularity) of a labelling
    of the simple undirected graph of triangles(): the vertices and the
    degree sum per label id, and the simple edges inside a community."""
    dst = np.repeat(np.arange(g.nv, dtype=np.int64),
                    np.diff(np.concatenate(([0], g.col_end)).astype(np.int64)))
    s = g.src.astype(np.int64)
    keep = s != dst
    e = np.unique(np.minimum(s, dst)[keep] * g.nv + np.maximum(s, dst)[keep])
    lo, hi = e // max(g.nv, 1), e % max(g.nv, 1)
    m = int(e.size)
    lab = np.asarray(labels, np.int64)
    deg = np.bincount(lo, minlength=g.nv) + np.bincount(hi, minlength=g.nv)
    tot = np.zeros(g.nv, np.int64)
    np.add.at(tot, lab, deg)
    intra = int((lab[lo] == lab[hi]).sum())
    return dict(m=m, sizes=np.bincount(lab, minlength=g.nv), tot=tot,
                intra=intra, modularity=modularity(intra, m, tot[tot > 0]))


def louvain(g: Graph, order="degree", seed=1, weighted=False, init=None,
            max_sweeps=0, max_levels=0):
    """(labels i32[nv], level_trace, sweep_trace) of the Louvain method as
    API.md defines it (LouvainEngine's oracle): per level a greedy colouring,
    sweeps over the colour classes (every member decides on the community
    totals as they stand when its class starts, then the movers are applied),
    the exact integer Qnum = W * in - sum tot^2 after every sweep, and a
    contraction by a sort of the relabelled edge list. level_trace:
    [(level, n, sweeps, moved, Qnum)], sweep_trace: [(level, sweep, moved,
    Qnum)]. Plain numpy and Python ints, one sequential loop per class; no
    roles, no tables, no adjacency records."""
    nv = g.nv
    dst = np.repeat(np.arange(nv, dtype=np.int64),
                    np.diff(np.concatenate(([0], g.col_end)).astype(np.int64)))
    src = g.src.astype(np.int64)
    keep = src != dst
    key = np.minimum(src, dst)[keep] * max(nv, 1) + \
        np.maximum(src, dst)[keep]
    ukey, inv = np.unique(key, return_inverse=True)
    lo, hi = ukey // max(nv, 1), ukey % max(nv, 1)
    w = np.ones(ukey.size, np.int64)
    if weighted:
        if g.weight is None:
            raise ValueError("weighted=True needs g.weight")
        if g.ne and int(g.weight.min()) < 1:
            raise ValueError("every weight must be >= 1")
        w = np.zeros(ukey.size, np.int64)
        np.add.at(w, inv.reshape(-1), g.weight.astype(np.int64)[keep])
    W = 2 * int(w.sum())
    if W >= 1 << 32:
        raise ValueError(f"W = {W} does not fit 32 bits")
    if init is not None:
        init = np.asarray(init)
        if init.shape != (nv,) or init.dtype.kind not in "iu" or \
                (nv and not 0 <= int(init.min()) <= int(init.max()) < nv):
            raise ValueError(f"init must hold {nv} labels in [0, {nv})")
    n, selfw = nv, np.zeros(nv, np.int64)
    vmap = np.arange(nv, dtype=np.int64)
    level_trace, sweep_trace = [], []
    while True:
        level = len(level_trace)
        rows = np.concatenate([lo, hi])
        o = np.argsort(rows, kind="stable")
        adj, aw = np.concatenate([hi, lo])[o], np.concatenate([w, w])[o]
        ptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n))))
        k = selfw.copy()
        np.add.at(k, rows, np.concatenate([w, w]))
        comm = np.arange(n, dtype=np.int64) if level or init is None else \
            init.astype(np.int64)
        tot = np.zeros(n, np.int64)
        np.add.at(tot, comm, k)
        tot, kk = tot.tolist(), k.tolist()
        colour = greedy_colouring(Graph.from_edges(n, lo, hi), order, seed) \
            if lo.size else np.zeros(n, np.int32)
        seq = np.lexsort((np.arange(n), colour))
        cuts = np.flatnonzero(np.diff(colour[seq])) + 1
        classes = [c[ptr[c + 1] > ptr[c]].tolist()
                   for c in np.split(seq, cuts)]

        def qnum():
            inside = int(selfw.sum()) + 2 * int(w[comm[lo] == comm[hi]].sum())
            return W * inside - sum(t * t for t in tot)

        best_q, sweeps, moved = qnum(), 0, 0
        while True:
            saved = comm.copy(), list(tot)
            movers = 0
            for cls in classes:
                moves = []
                for v in cls:
                    A, kv = int(comm[v]), kk[v]
                    cs, a = np.unique(comm[adj[ptr[v]:ptr[v + 1]]],
                                      return_inverse=True)
                    a = np.bincount(a.reshape(-1),
                                    weights=aw[ptr[v]:ptr[v + 1]])
                    own, best = -kv * (tot[A] - kv), None
                    for c, ac in zip(cs.tolist(), a.astype(np.int64).tolist()):
                        if c == A:
                            own += ac * W
                        else:
                            s = ac * W - kv * tot[c]
                            if best is None or s > best[0]:
                                best = (s, c)  # cs ascends: the smallest c
                    if best is not None and best[0] > own:
                        moves.append((v, A, best[1]))
                for v, A, c in moves:
                    comm[v] = c
                    tot[A] -= kk[v]
                    tot[c] += kk[v]
                movers += len(moves)
            sweeps += 1
            q = qnum()
            sweep_trace.append((level, sweeps, movers, q))
            if movers == 0:
                break
            if q <= best_q:
                comm, tot = saved
                break
            best_q, moved = q, moved + movers
            if max_sweeps > 0 and sweeps >= max_sweeps:
                break
        level_trace.append((level, n, sweeps, moved, best_q))
        if moved == 0 and (level or init is None):
            break  # an init is contracted even if nothing moved
        used = np.unique(comm)
        dense = np.searchsorted(used, comm)
        vmap = dense[vmap]
        selfw = np.bincount(dense, weights=selfw,
                            minlength=used.size).astype(np.int64)
        cl, ch = dense[lo], dense[hi]
        np.add.at(selfw, cl[cl == ch], 2 * w[cl == ch])
        n = int(used.size)
        out = cl != ch
        ukey, inv = np.unique(np.minimum(cl, ch)[out] * n +
                              np.maximum(cl, ch)[out], return_inverse=True)
        w2 = np.zeros(ukey.size, np.int64)
        np.add.at(w2, inv.reshape(-1), w[out])
        lo, hi, w = ukey // n, ukey % n, w2
        if max_levels > 0 and len(level_trace) >= max_levels:
            break
    return vmap.astype(np.int32), level_trace, sweep_trace


def multi_source_bfs(g: Graph, sources) -> np.ndarray:
    """i32[k, nv]: the hop distance from each source along the edges
    u -> v of the directed graph as loaded, -1 where unreached. One call of
    the sssp hop oracle per source."""
    out = np.empty((len(sources), g.nv), np.int32)
    for i, s in enumerate(sources):
        out[i] = sssp(g, int(s))[0].view(np.int32)  # INF is -1
    return out


def multi_source_stats(g: Graph, sources, div=8, batch=64):
    """What MSBFSEngine reports, from multi_source_bfs with plain numpy in
    the order API.md defines: dict(depths, reach, dist_sum, harmonic,
    level_counts, reached, farness, eccentricity, closeness, level_trace).
    harmonic is accumulated batch by batch, level by level, one division and
    one addition per vertex and level. level_trace: (batch, level, direction,
    frontier, volume, new_pairs) with the direction the rule
    volume * div > ne gives."""
    depths = multi_source_bfs(g, sources)
    k, nv = depths.shape
    outdeg = g.out_degrees().astype(np.int64)
    hit = depths >= 0
    harmonic = np.zeros(nv, np.float64)
    trace = []
    for b in range(0, k, batch):
        d = depths[b:b + batch]
        for level in range(int(d.max()) + 1):
            new = (d == level).sum(0)
            if level:
                harmonic[new > 0] += new[new > 0] / np.float64(level)
            volume = int(outdeg[new > 0].sum())
            trace.append((b // batch, level,
                          "pull" if volume * div > g.ne else "push",
                          int((new > 0).sum()), volume, int(new.sum())))
    counts = [np.bincount(row[row >= 0]).tolist() for row in depths]
    reached = np.array([sum(c) for c in counts], np.int64)
    farness = np.array([sum(i * n for i, n in enumerate(c)) for c in counts],
                       np.int64)
    closeness = np.divide(reached - 1.0, farness, where=farness > 0,
                          out=np.zeros(k, np.float64))
    return dict(depths=depths, reach=hit.sum(0).astype(np.int32),
                dist_sum=np.where(hit, depths, 0).sum(0, dtype=np.int64),
                harmonic=harmonic, level_counts=counts, reached=reached,
                farness=farness,
                eccentricity=np.array([len(c) - 1 for c in counts], np.int64),
                closeness=closeness, level_trace=trace)


def personalised_pagerank(g: Graph, seeds, damping, iters, tol=0.0):
    """(x f64[nv, K], iterations, residuals) of the recurrence in API.md:
    column c restarts uniformly over seeds[c] (an int or a list of distinct
    ints), x^0 = t, x' = (1 - d) t + d * sum over the entries u -> v of
    x[u] / outdeg(u), d = damping rounded to fp32. Mass leaks at vertices
    without out-edges. residuals[i] is max |x^(i+1) - x^i| over everything;
    with tol > 0 the run ends after the first one <= tol. Plain numpy fp64,
    one np.add.at over the entry list per iteration."""
    d = float(np.float32(damping))
    sets = [[int(s)] if isinstance(s, (int, np.integer)) else
            [int(v) for v in s] for s in seeds]
    src = g.src.astype(np.int64)
    dst = np.repeat(np.arange(g.nv, dtype=np.int64),
                    np.diff(np.concatenate(([0], g.col_end)).astype(np.int64)))
    outdeg = np.bincount(src, minlength=g.nv).astype(np.float64)
    t = np.zeros((g.nv, len(sets)), np.float64)
    for c, s in enumerate(sets):
        t[s, c] = 1.0 / len(s)
    x, residuals = t.copy(), []
    for _ in range(iters):
        y = x / np.maximum(outdeg, 1.0)[:, None]
        acc = np.zeros_like(x)
        np.add.at(acc, dst, y[src])
        new = (1.0 - d) * t + d * acc
        residuals.append(float(np.abs(new - x).max()))
        x = new
        if tol > 0.0 and residuals[-1] <= tol:
            break
    return x, len(residuals), residuals


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


def cf_ials(g: Graph, K: int, iters: int, alpha: float, reg: float, init,
            n_users: int) -> np.ndarray:
    """Plain-numpy implicit-feedback ALS (CFImplicitALSEngine's oracle), all
    float64. Per sweep the user rows [0, n_users) are solved against the item
    factors, then the item rows against the UPDATED users. For row v with Y the
    factor rows of the whole other side and (y_e, w_e) its CSC entries:
        A = Y^T Y + alpha * sum_e w_e y_e y_e^T + reg I
        b = sum_e (1 + alpha w_e) y_e,        x_v = A^-1 b
    The sums run per ENTRY (a parallel edge is one more observation); a row
    with no entries gets x_v = 0."""
    vec = np.array(init, dtype=np.float64).reshape(g.nv, K).copy()
    eye = reg * np.eye(K)

    def _phase(lo, hi, olo, ohi):
        Y = vec[olo:ohi]
        base = Y.T @ Y + eye
        b = 0 if lo == 0 else int(g.col_end[lo - 1])
        for v in range(lo, hi):
            e = int(g.col_end[v])
            if e > b:
                S = vec[g.src[b:e]]
                w = g.weight[b:e].astype(np.float64)
                A = base + alpha * (S.T * w) @ S
                vec[v] = np.linalg.solve(A, (1.0 + alpha * w) @ S)
            else:
                vec[v] = 0.0
            b = e

    for _ in range(iters):
        # in place is exact: a row only reads the other side's factors
        _phase(0, n_users, n_users, g.nv)
        _phase(n_users, g.nv, 0, n_users)
    return vec


def cf_ials_loss(g: Graph, K: int, vec, alpha: float, reg: float,
                 n_users: int) -> float:
    """The objective both cf_ials phases minimise exactly when every rating
    is stored both ways, dense in float64 (users x items table):
        sum_{u,i} (x_u.y_i)^2
        + sum_e [alpha w_e (x.y)^2 - 2 (1 + alpha w_e) (x.y)]
        + reg (|X|^2 + |Y|^2),    e over the user-side entries."""
    vec = np.asarray(vec, dtype=np.float64).reshape(g.nv, K)
    X, Y = vec[:n_users], vec[n_users:]
    ne_u = int(g.col_end[n_users - 1]) if n_users else 0
    dst = np.repeat(np.arange(g.nv), np.diff(g.col_end.astype(np.int64),
                                             prepend=0))[:ne_u]
    p = np.einsum("ek,ek->e", vec[dst], vec[g.src[:ne_u]])
    w = g.weight[:ne_u].astype(np.float64)
    return float(((X @ Y.T) ** 2).sum()
                 + (alpha * w * p * p - 2.0 * (1.0 + alpha * w) * p).sum()
                 + reg * ((X * X).sum() + (Y * Y).sum()))


def cf_topn(vectors, queries, c_lo, c_hi, n, excl_ptr=None, excl_adj=None):
    """Plain-numpy CF top-N (CFTopN's oracle; no C++ twin): for each query
    the first n candidates of [c_lo, c_hi) outside row `query` of the
    exclusion CSR, by descending float64 dot product and ascending id among
    equal scores. -> (items i32[q, n], scores f64[q, n]), padded with -1 and
    -inf."""
    vec = np.asarray(vectors, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.int64)
    cand = np.arange(c_lo, c_hi, dtype=np.int64)
    items = np.full((queries.size, n), -1, np.int32)
    scores = np.full((queries.size, n), -np.inf, np.float64)
    for p, u in enumerate(queries):
        ok = np.ones(cand.size, bool)
        if excl_ptr is not None:
            row = np.asarray(excl_adj[int(excl_ptr[u]):int(excl_ptr[u + 1])],
                             dtype=np.int64)
            ok = ~np.isin(cand, row)
        s = vec[cand[ok]] @ vec[u]
        best = np.lexsort((cand[ok], -s))[:n]
        items[p, :best.size] = cand[ok][best]
        scores[p, :best.size] = s[best]
    return items, scores
