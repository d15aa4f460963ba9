"""Minimum-spanning-forest references for test_msf_cpu.py / test_gpu_msf.py.

Numpy only (no GPU, no C++ oracle): simple_weighted, the simple weighted
edge list of the definition; sync_boruvka, the synchronous Boruvka schedule
MSFEngine follows (so the authority for its rounds and per-round counts,
the dead-row rule included); dense_prim, an independent second definition
for graphs of at most 64 vertices; the hand cases, the hub ladder and the
pinned RMAT graphs.
"""
from types import SimpleNamespace

import numpy as np

import tc_ref
from lux_amd.graph import Graph

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAX_ROUNDS = 34


def simple_weighted(g):
    """(lo, hi, w) i64[m] of the underlying simple undirected graph,
    ascending by (lo << 32) | hi: the position is the edge id. w is the
    minimum weight over all occurrences of {lo, hi}, in either direction;
    self-loops vanish."""
    src, dst = tc_ref.edge_lists(g)
    w = np.asarray(g.weight, np.int64)
    keep = src != dst
    key = (np.minimum(src, dst) << 32 | np.maximum(src, dst))[keep]
    w = w[keep]
    order = np.lexsort((w, key))
    key, w = key[order], w[order]
    first = np.ones(key.size, bool)
    first[1:] = key[1:] != key[:-1]
    key, w = key[first], w[first]
    return key >> 32, key & 0xFFFFFFFF, w


def max_id_labels(nv, comp):
    top = np.zeros(nv, np.int64)
    np.maximum.at(top, comp, np.arange(nv))
    return top[comp]


def sync_boruvka(g, dead=True):
    """The synchronous schedule. A scan gives every component the minimum
    (w, e) entry that leaves it; then every component c with such an edge
    hooks onto the component d at its other end, except that of two
    components that chose the same edge only the smaller id hooks; then
    every vertex is relabelled to its root. A scan after which nothing
    hooks ends the run and is not a round.
    Dead-row rule: in scan s every row not marked dead in an earlier scan
    is walked in full, and a walked row without an entry that leaves its
    component is marked dead; `scanned` is the sum of the walked rows'
    simple degrees (dead=False: every row is walked, 2m per scan).
    Returns lo, hi, w, in_forest bool[m], total (int), nf, labels (the
    largest id of the component), rounds, scans, per_round = [(components
    with an edge, merged, scanned)] per round, scanned (all scans)."""
    lo, hi, w = simple_weighted(g)
    nv, m = g.nv, lo.size
    ids = np.arange(m)
    by_rank = np.lexsort((ids, w))  # the strict order (w, e)
    rank = np.empty(m, np.int64)
    rank[by_rank] = ids
    row, nbr = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    eid = np.concatenate([ids, ids])
    deg = np.bincount(row, minlength=nv)
    comp = np.arange(nv)
    isdead = np.zeros(nv, bool)
    mask = np.zeros(m, bool)
    total, scans, scanned_all, per_round = 0, 0, 0, []
    while m:
        assert scans <= MAX_ROUNDS
        scans += 1
        live = ~isdead if dead else np.ones(nv, bool)
        scanned = int(deg[live].sum())
        scanned_all += scanned
        ext = live[row] & (comp[row] != comp[nbr])
        has = np.zeros(nv, bool)
        has[row[ext]] = True
        isdead |= live & ~has
        best = np.full(nv, m, np.int64)
        np.minimum.at(best, comp[row[ext]], rank[eid[ext]])
        cs = np.nonzero(best != m)[0]
        e = by_rank[best[cs]]
        cl, ch = comp[lo[e]], comp[hi[e]]
        assert np.all((cl == cs) ^ (ch == cs))
        d = np.where(cl == cs, ch, cl)
        hook = ~((best[d] == best[cs]) & (cs > d))
        merged = int(hook.sum())
        if merged == 0:
            assert cs.size == 0
            break
        per_round.append((int(cs.size), merged, scanned))
        assert not mask[e[hook]].any()
        mask[e[hook]] = True
        total += int(w[e[hook]].sum())
        parent = np.arange(nv)
        parent[cs[hook]] = d[hook]
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        comp = parent[comp]
    return SimpleNamespace(
        lo=lo, hi=hi, w=w, in_forest=mask, total=total, nf=int(mask.sum()),
        labels=max_id_labels(nv, comp), rounds=len(per_round), scans=scans,
        per_round=per_round, scanned=scanned_all)


def dense_prim(g):
    """(in_forest bool[m], total) by Prim on the dense matrix of (w, e)
    ranks, one tree per component, for graphs of at most 64 vertices."""
    assert g.nv <= 64
    lo, hi, w = simple_weighted(g)
    nv, m = g.nv, lo.size
    ids = np.arange(m)
    by_rank = np.lexsort((ids, w))
    R = np.full((nv, nv), m, np.int64)
    R[lo[by_rank], hi[by_rank]] = ids
    R[hi[by_rank], lo[by_rank]] = ids
    mask = np.zeros(m, bool)
    seen = np.zeros(nv, bool)
    for root in range(nv):
        if seen[root]:
            continue
        seen[root] = True
        while True:
            cut = R[seen][:, ~seen]
            if cut.size == 0 or cut.min() == m:
                break
            r = int(cut.min())
            e = int(by_rank[r])
            assert seen[lo[e]] != seen[hi[e]]
            mask[e] = True
            seen[lo[e]] = seen[hi[e]] = True
    return mask, int(w[mask].sum())


# ---- graphs ----

def weighted_graph(nv, edges):
    """edges: (src, dst, w) triples, directed as given."""
    src = np.asarray([e[0] for e in edges], np.uint32)
    dst = np.asarray([e[1] for e in edges], np.uint32)
    w = np.asarray([e[2] for e in edges], np.int32)
    return Graph.from_edges(nv, src, dst, w)


def _case(name, nv, edges, **want):
    return SimpleNamespace(name=name, g=weighted_graph(nv, edges), want=want)


PATH_N = 4001
EXTREMES = [I32_MIN, -5, 0, 7, I32_MAX]


def hand_cases():
    """Small graphs with closed-form results: any of total, nf, components,
    rounds, forest (the edge ids) in `want`."""
    n = PATH_N
    return [
        _case("empty", 4, [], total=0, nf=0, components=4, rounds=0, m=0),
        _case("single_vertex", 1, [], total=0, nf=0, components=1, rounds=0),
        _case("one_edge", 2, [(1, 0, 5)], total=5, nf=1, components=1,
              rounds=1, forest=[0]),
        # edges (0,1) (0,2) (1,2) with weights 3, 2, 1
        _case("triangle", 3, [(0, 1, 3), (2, 1, 1), (2, 0, 2)], total=3,
              nf=2, forest=[1, 2]),
        _case("k4_equal", 4, [(a, b, 7) for a in range(4)
                              for b in range(a + 1, 4)],
              total=21, nf=3, forest=[0, 1, 2]),
        # ties must not close the cycle
        _case("cycle4001", n, [(i, (i + 1) % n, 1) for i in range(n)],
              total=n - 1, nf=n - 1, components=1, rounds=1, m=n,
              per_round=[(n, n - 1, 2 * n)]),
        _case("path4001_alternating", n,
              [(i, i + 1, 1 + i % 2) for i in range(n - 1)],
              total=6000, nf=n - 1, components=1, rounds=2,
              per_round=[(n, 2001, 8000), (2000, 1999, 8000)]),
        _case("path4001_increasing", n,
              [(i + 1, i, i + 1) for i in range(n - 1)],
              total=8002000, nf=n - 1, components=1, rounds=1,
              per_round=[(n, n - 1, 8000)]),
        # a triangle, a path of four, the isolated vertices 3 and 8
        _case("two_components_and_isolated", 9,
              [(0, 1, 4), (1, 2, 4), (2, 0, 4), (4, 5, 2), (6, 5, -1),
               (6, 7, 2)], total=11, nf=5, components=4),
        # the minimum over all occurrences wins: {0,1} = 3, {1,2} = 2
        _case("parallel_arcs", 3,
              [(0, 1, 5), (1, 0, 3), (0, 1, 9), (1, 2, 4), (2, 1, 8),
               (2, 1, 2)], total=5, nf=2, m=2, forest=[0, 1]),
        _case("self_loops", 3,
              [(0, 0, -100), (0, 1, 4), (1, 1, 1), (1, 2, 6), (2, 2, -7)],
              total=10, nf=2, m=2),
        _case("extremes_path", 6,
              [(i, i + 1, x) for i, x in enumerate(EXTREMES)],
              total=sum(EXTREMES), nf=5),
        # the heaviest edge, INT32_MAX, closes the cycle
        _case("extremes_cycle", 5,
              [(i, (i + 1) % 5, x) for i, x in enumerate(EXTREMES)],
              total=sum(EXTREMES) - I32_MAX, nf=4),
        _case("int64_total_max", 8, [(i, i + 1, I32_MAX) for i in range(7)],
              total=7 * I32_MAX, nf=7),
        _case("int64_total_min", 8, [(i + 1, i, I32_MIN) for i in range(7)],
              total=7 * I32_MIN, nf=7),
    ]


LADDER = (62, 64, 66, 126, 128, 130, 254, 256, 258, 1022, 1024, 1026, 4098)


def paired_star(L, descending=False):
    """Centre 0, leaves 1..L (L even). Centre edge of leaf i: 10 + i, or
    10 + (L + 1 - i) when descending (the row minimum then sits at the end
    of the centre row); leaf pairs (i, i + 1) for odd i, weight 1.
    Closed form: round 1 joins the pairs and the centre to one of them,
    round 2 every other pair to the centre by its lighter centre edge: 2
    rounds, nf = L, total = L / 2 + sum over odd i of (10 + i). In round 2
    the centre row mixes internal and external entries."""
    assert L % 2 == 0
    edges = [(0, i, 10 + (L + 1 - i if descending else i))
             for i in range(1, L + 1)]
    edges += [(i + 1, i, 1) for i in range(1, L, 2)]
    total = L // 2 + sum(10 + i for i in range(1, L, 2))
    return _case(f"paired_star{L}{'_desc' if descending else ''}", L + 1,
                 edges, total=total, nf=L, components=1, rounds=2, m=L + L // 2,
                 max_degree=L,
                 per_round=[(L + 1, L // 2 + 1, 3 * L),
                            (L // 2, L // 2 - 1, 3 * L)])


def ladder_cases():
    return [paired_star(L, desc) for L in LADDER for desc in (False, True)]


# graph (hash_weights(wmax), seed 1) -> m, forest, total, components,
# isolated, max degree, per_round
RMAT = {
    "rmat12_w1": dict(args=(12, 300000), sym=False, wmax=1, m=160602,
                      nf=3853, total=3853, components=243, isolated=242,
                      max_degree=2402, per_round=[(3854, 3853, 321204)]),
    "rmat12_w16": dict(args=(12, 300000), sym=False, wmax=16, m=160602,
                       nf=3853, total=8283, components=243, isolated=242,
                       max_degree=2402,
                       per_round=[(3854, 3837, 321204), (17, 16, 321204)]),
    "rmat12_w1000": dict(args=(12, 300000), sym=False, wmax=1000, m=160602,
                         nf=3853, total=364387, components=243, isolated=242,
                         max_degree=2402,
                         per_round=[(3854, 3566, 321204), (288, 256, 321204),
                                    (32, 29, 321010), (3, 2, 320988)]),
    "rmat12_sym_w1": dict(args=(12, 300000), sym=True, wmax=1, m=94769,
                          nf=3676, total=3676, components=420, isolated=419,
                          max_degree=1896, per_round=[(3677, 3676, 189538)]),
    "rmat12_sym_w16": dict(args=(12, 300000), sym=True, wmax=16, m=94769,
                           nf=3676, total=7010, components=420, isolated=419,
                           max_degree=1896,
                           per_round=[(3677, 3654, 189538),
                                      (23, 22, 189538)]),
    "rmat12_sym_w1000": dict(args=(12, 300000), sym=True, wmax=1000, m=94769,
                             nf=3676, total=285035, components=420,
                             isolated=419, max_degree=1896,
                             per_round=[(3677, 3388, 189538),
                                        (289, 263, 189538),
                                        (26, 24, 189231), (2, 1, 189201)]),
    "rmat10_w16": dict(args=(10, 8000), sym=False, wmax=16, m=5888, nf=802,
                       total=3414, components=222, isolated=220,
                       max_degree=351,
                       per_round=[(804, 755, 11776), (48, 47, 11776)]),
}


def rmat_graph(name):
    pin = RMAT[name]
    g = Graph.rmat(*pin["args"], seed=3, sym=pin["sym"])
    g.hash_weights(pin["wmax"], seed=1)
    return g


def random_graph(nv, ne, wlo, whi, seed):
    """A seeded random directed multigraph with loops, weights uniform in
    [wlo, whi] (a narrow range makes ties)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, nv, ne)
    dst = rng.integers(0, nv, ne)
    w = rng.integers(wlo, whi + 1, ne)
    return Graph.from_edges(nv, src.astype(np.uint32), dst.astype(np.uint32),
                            w.astype(np.int32))
