"""k-core references for test_kcore_cpu.py / test_gpu_kcore.py.

Numpy only (no GPU, no C++ oracle): the synchronous round-by-round peel
(the schedule KCoreEngine follows, so also the authority for its level and
round counts), the H-index fixpoint (an independent second definition), the
hand cases with their closed-form coreness, and the hub ladder.
"""
from types import SimpleNamespace

import numpy as np

import tc_ref
from lux_amd.graph import Graph


def simple_adjacency(g):
    """(ptr i64[nv+1], adj i64[2m]) of the underlying simple graph, both
    directions of every edge."""
    src, dst = tc_ref.edge_lists(g)
    keep = src != dst
    key = np.unique(np.minimum(src[keep], dst[keep]) << 32 |
                    np.maximum(src[keep], dst[keep]))
    lo, hi = key >> 32, key & 0xFFFFFFFF
    a = np.concatenate([lo, hi])
    b = np.concatenate([hi, lo])
    order = np.argsort(a, kind="stable")
    ptr = np.zeros(g.nv + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(a, minlength=g.nv))
    return ptr, b[order]


def _neighbours(ptr, adj, rows):
    """adj entries of the given rows, concatenated."""
    starts = ptr[rows]
    lens = ptr[rows + 1] - starts
    first = np.cumsum(lens) - lens
    idx = np.arange(int(lens.sum())) - np.repeat(first, lens) + \
        np.repeat(starts, lens)
    return adj[idx]


def sync_peel(g):
    """(coreness i64[nv], levels, rounds) of the synchronous peel: jump to
    k = max(k, min alive degree); a round removes every alive vertex of
    current degree <= k and takes it off its neighbours' degrees; the level
    ends when a round would remove nothing. levels counts the non-empty
    levels (= the distinct coreness values), rounds all rounds."""
    ptr, adj = simple_adjacency(g)
    deg = np.diff(ptr)
    alive = np.ones(g.nv, bool)
    core = np.zeros(g.nv, np.int64)
    k = levels = rounds = 0
    while alive.any():
        k = max(k, int(deg[alive].min()))
        levels += 1
        while True:
            rem = np.nonzero(alive & (deg <= k))[0]
            if rem.size == 0:
                break
            rounds += 1
            core[rem] = k
            alive[rem] = False
            deg -= np.bincount(_neighbours(ptr, adj, rem), minlength=g.nv)
    return core, levels, rounds


def hindex_fixpoint(g):
    """coreness i64[nv] as the fixpoint of c[v] = H-index of c over v's
    neighbours (the largest h with at least h neighbours of c >= h),
    started from c = degree. Every sweep sorts all 2m arcs: small graphs."""
    ptr, adj = simple_adjacency(g)
    nv = g.nv
    row = np.repeat(np.arange(nv), np.diff(ptr))
    pos = np.arange(adj.size) - ptr[row]  # offset inside the row
    c = np.diff(ptr)
    while True:
        val = c[adj]
        order = np.lexsort((-val, row))  # rows in place, values descending
        ok = val[order] >= pos + 1       # a prefix of every row
        new = np.bincount(row[ok], minlength=nv)
        if np.array_equal(new, c):
            return c
        c = new


def _case(name, nv, edges, core, levels=None, rounds=None, g=None):
    if g is None:
        src = np.asarray([e[0] for e in edges], np.uint32)
        dst = np.asarray([e[1] for e in edges], np.uint32)
        g = Graph.from_edges(nv, src, dst)
    return SimpleNamespace(name=name, g=g, levels=levels, rounds=rounds,
                           core=np.asarray(core, np.int64))


PATH_N = 4001
STAR_LEAVES = 5000


def hand_cases():
    """Closed-form coreness (and, where the schedule is the point, levels
    and rounds) of small graphs; `core` is None where only the degeneracy
    is closed-form (bipartite: 9)."""
    tc = {c.name: c.g for c in tc_ref.hand_cases()}
    n = tc_ref.FAN_N
    L = STAR_LEAVES
    star = [(0, i) for i in range(1, L + 1)]
    # the hub 0 is also in a K_10 with 1..9; the leaves are 10..L+9
    star_k10 = tc_ref._clique(10) + [(0, i) for i in range(10, L + 10)]
    k300 = tc_ref._clique(300)
    cases = [
        _case("empty", 4, None, [0] * 4, levels=1, rounds=1, g=tc["empty"]),
        _case("single_edge", 4, None, [0, 1, 1, 0], levels=2, rounds=2,
              g=tc["single_edge"]),
        _case("path5", 5, None, [1] * 5, levels=1, rounds=3, g=tc["path"]),
        _case("one_way_triangle", 3, None, [2] * 3, levels=1, rounds=1,
              g=tc["one_way_triangle"]),
        _case("doubled_triangle_with_loops", 4, None, [2, 2, 2, 0],
              levels=2, rounds=2, g=tc["doubled_triangle_with_loops"]),
        _case("k4", 4, None, [3] * 4, levels=1, rounds=1, g=tc["k4"]),
        _case("k5_minus_edge", 5, None, [3] * 5, levels=1, rounds=2,
              g=tc["k5_minus_edge"]),
        # both ends of the path 1..n leave every round, the hub 0 with the
        # last pair
        _case("fan", n + 1, None, [2] * (n + 1), levels=1, rounds=n // 2,
              g=tc["fan"]),
        # the cascade: two vertices a round, the middle one alone at the end
        _case("path4001", PATH_N,
              [(i, i + 1) for i in range(PATH_N - 1)], [1] * PATH_N,
              levels=1, rounds=PATH_N // 2 + 1),
        # the hub takes L concurrent decrements from k + 1
        _case("star5000", L + 1, star, [1] * (L + 1), levels=1, rounds=2),
        _case("star5000_in_k10", L + 10, star_k10, [9] * 10 + [1] * L,
              levels=2),
        # the level jump 0 -> 299
        _case("k300_plus_isolated", 350, k300, [299] * 300 + [0] * 50,
              levels=2, rounds=2),
    ]
    bip = SimpleNamespace(name="bipartite", g=tc["bipartite"], core=None,
                          degeneracy=9, levels=None, rounds=None)
    return cases + [bip]


def ladder_degrees(hub):
    return sorted({0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65,
                   hub - 1, hub, hub + 1, 2 * hub - 1, 2 * hub,
                   2 * hub + 1})


def ladder(hub, seed=13):
    """Three rows for every degree D of ladder_degrees(hub), each adjacent
    to a seeded D-subset of the pool clique K_P, P = max D + 2, and to
    nothing else: coreness(row) = D (its neighbours all outlast it),
    coreness(pool) = P - 1 (every row is gone before the clique is
    touched), levels = the distinct D values plus one. ids [0, R): the
    rows; [R, R + P): the pool.

    Returns g, rows, degrees (per row), core (closed form), levels."""
    rng = np.random.default_rng(seed)
    degrees = np.repeat(ladder_degrees(hub), 3)
    R = degrees.size
    P = int(degrees.max()) + 2
    pool = np.arange(R, R + P)
    a = np.repeat(pool, P)
    b = np.tile(pool, P)
    keep = a < b
    src, dst = [a[keep]], [b[keep]]
    for r, D in enumerate(degrees):
        src.append(np.full(D, r))
        dst.append(rng.choice(pool, D, replace=False))
    src = np.concatenate(src)
    dst = np.concatenate(dst)
    flip = rng.random(src.size) < 0.5  # the direction given must not matter
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    core = np.concatenate([degrees, np.full(P, P - 1)]).astype(np.int64)
    return SimpleNamespace(
        g=Graph.from_edges(R + P, src.astype(np.uint32),
                           dst.astype(np.uint32)),
        rows=np.arange(R), degrees=degrees, core=core,
        levels=len(set(degrees.tolist())) + 1)
