"""Triangle-counting references for test_tc_cpu.py / test_gpu_tc.py.

Numpy only (no GPU, no C++ oracle): the dense-matrix count, the hand cases
with their closed-form values, and the role ladder with its prescribed
oriented out-degrees and exact per-row counts.
"""
from types import SimpleNamespace

import numpy as np

from lux_amd.graph import Graph


def edge_lists(g):
    """(src, dst) of every edge in CSC order."""
    deg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    dst = np.repeat(np.arange(g.nv, dtype=np.int64), deg)
    return g.src.astype(np.int64), dst


def simple_matrix(g):
    """Symmetric 0/1 float64 adjacency of the underlying simple graph."""
    assert g.nv <= 4096
    src, dst = edge_lists(g)
    A = np.zeros((g.nv, g.nv), np.float64)
    A[src, dst] = 1.0
    A[dst, src] = 1.0
    np.fill_diagonal(A, 0.0)
    return A


def dense_count(g):
    """(total, per_vertex u64[nv], simple edges) from A = the simple
    symmetric 0/1 matrix: per_vertex = ((A @ A) * A).sum(1) / 2, total =
    per_vertex.sum() / 3. float64 BLAS on small integers: exact while every
    count stays below 2^53."""
    A = simple_matrix(g)
    twice = ((A @ A) * A).sum(1)
    assert twice.max(initial=0.0) < 2.0 ** 53
    pv = (twice / 2).astype(np.uint64)
    assert np.array_equal(pv.astype(np.float64) * 2, twice)
    total = int(pv.sum())
    assert total % 3 == 0
    return total // 3, pv, int(A.sum()) // 2


def simple_degrees(g):
    """Simple undirected degree per vertex (any nv)."""
    src, dst = edge_lists(g)
    keep = src != dst
    lo = np.minimum(src[keep], dst[keep])
    hi = np.maximum(src[keep], dst[keep])
    k = np.unique(lo << 32 | hi)
    return np.bincount(k >> 32, minlength=g.nv) + \
        np.bincount(k & 0xFFFFFFFF, minlength=g.nv)


def transitivity(g, total):
    deg = simple_degrees(g)
    wedges = int((deg * (deg - 1) // 2).sum())
    return 3 * total / wedges if wedges else 0.0


def _case(name, nv, edges, total, pv):
    src = [e[0] for e in edges]
    dst = [e[1] for e in edges]
    return SimpleNamespace(
        name=name, g=Graph.from_edges(nv, src, dst),
        want=dict(total=total, per_vertex=np.asarray(pv, np.uint64)))


def _clique(n, skip=()):
    return [(a, b) for a in range(n) for b in range(a + 1, n)
            if (a, b) not in skip]


FAN_N = 70


def hand_cases():
    n = FAN_N
    fan = [(0, i) for i in range(1, n + 1)] + \
        [(i, i + 1) for i in range(1, n)]
    tri = [(0, 1), (1, 2), (2, 0)]
    star_nv = 100
    bip = Graph.bipartite(64, 64, 2000)
    return [
        _case("empty", 4, [], 0, [0, 0, 0, 0]),
        _case("single_edge", 4, [(2, 1)], 0, [0, 0, 0, 0]),
        _case("path", 5, [(0, 1), (1, 2), (3, 2), (3, 4)], 0, [0] * 5),
        _case("one_way_triangle", 3, tri, 1, [1, 1, 1]),
        # every arc twice, one of them also reversed, a loop on each corner
        _case("doubled_triangle_with_loops", 4,
              tri + tri + [(1, 0), (0, 0), (1, 1), (2, 2), (2, 2)], 1,
              [1, 1, 1, 0]),
        _case("k4", 4, _clique(4), 4, [3, 3, 3, 3]),
        # the 3 triangles through both 0 and 1 are gone
        _case("k5_minus_edge", 5, _clique(5, skip=((0, 1),)), 7,
              [3, 3, 5, 5, 5]),
        _case("two_triangles_sharing_an_edge", 4,
              [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)], 2, [1, 2, 2, 1]),
        # id order: d+(0) = nv - 1
        _case("star", star_nv, [(0, i) for i in range(1, star_nv)], 0,
              [0] * star_nv),
        SimpleNamespace(name="bipartite", g=bip, want=dict(
            total=0, per_vertex=np.zeros(bip.nv, np.uint64))),
        # 0 - i for i in 1..n plus the path 1-2-...-n: the triangles are
        # {0, i, i+1}. In id order the match of arc (0, i) is the entry
        # right after i in A(0), and the last matching arc's is the last
        # entry of A(0): both ends of a narrowed search window
        _case("fan", n + 1, fan, n - 1, [n - 1, 1] + [2] * (n - 2) + [1]),
    ]


# lane-stride edges of the A(v) walk. Staged / hub: 64-entry strides, four per
# trip (entered past 192 entries, the fourth stride short below 256). Small:
# 16-entry strides, four per trip.
POOL_DEGREES = (0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 191, 192, 193, 255,
                256, 257, 449)


def ladder_degrees(stage_cap, t1, chunk):
    """Every role and stride boundary at -1 / 0 / +1."""
    return sorted({0, 1, 2, 3, t1 - 1, t1, t1 + 1, 63, 64, 65,
                   chunk - 1, chunk, chunk + 1, 2 * chunk + 1,
                   stage_cap - 1, stage_cap, stage_cap + 1,
                   2 * stage_cap + 1})


def ladder(stage_cap, t1, chunk, seed=11):
    """Role ladder for id order (rank = id, so oriented degrees are the
    ones prescribed here).

    ids [0, L): one ladder row per degree D of ladder_degrees, adjacent to
    a seeded D-subset S of the pool and to nothing else, so its oriented
    out-degree is D and its triangle count is the number of pool edges
    inside S. ids [L, L + P): the pool, P = max(2 * stage_cap + 64, 600).
    Its first len(POOL_DEGREES) vertices are the specials: special k is
    adjacent to exactly POOL_DEGREES[k] higher plain pool vertices and to
    no other pool vertex (oriented degree POOL_DEGREES[k], the lane-stride
    edges of the A(v) walk), and is in S of every row with room for all
    specials. The plain pool vertices carry a seeded random simple graph of
    16 * P drawn pairs.

    Returns g, rows, degrees, row_counts (exact), specials."""
    rng = np.random.default_rng(seed)
    degrees = ladder_degrees(stage_cap, t1, chunk)
    L = len(degrees)
    P = max(2 * stage_cap + 64, 600)
    ns = len(POOL_DEGREES)
    assert degrees[-1] <= P and max(POOL_DEGREES) <= P - ns
    specials = np.arange(L, L + ns)
    plain = np.arange(L + ns, L + P)
    # pool edges, canonical and unique
    a = rng.choice(plain, 16 * P)
    b = rng.choice(plain, 16 * P)
    sa, sb = [], []
    for k, d in enumerate(POOL_DEGREES):
        sa.append(np.full(d, specials[k]))
        sb.append(rng.choice(plain, d, replace=False))
    a = np.concatenate([a] + sa)
    b = np.concatenate([b] + sb)
    keep = a != b
    key = np.unique(np.minimum(a[keep], b[keep]) << 32 |
                    np.maximum(a[keep], b[keep]))
    pa, pb = key >> 32, key & 0xFFFFFFFF
    # ladder rows
    la, lb, counts = [], [], []
    for r, D in enumerate(degrees):
        if D >= ns + 8:
            S = np.concatenate(
                [specials, rng.choice(plain, D - ns, replace=False)])
        else:
            S = rng.choice(plain, D, replace=False)
        inS = np.zeros(L + P, bool)
        inS[S] = True
        counts.append(int((inS[pa] & inS[pb]).sum()))
        la.append(np.full(D, r))
        lb.append(S)
    src = np.concatenate([pa] + la)
    dst = np.concatenate([pb] + lb)
    flip = rng.random(src.size) < 0.5  # the direction given must not matter
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    return SimpleNamespace(
        g=Graph.from_edges(L + P, src, dst), rows=np.arange(L),
        degrees=np.asarray(degrees), specials=specials,
        row_counts=np.asarray(counts, np.uint64))
