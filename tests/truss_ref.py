"""k-truss references for test_truss_cpu.py.

Numpy only (no GPU, no C++ oracle), on tc_ref.simple_matrix: the dense
per-edge support ((A @ A) * A at the edges), a naive dense synchronous peel
for one k, a dense decomposition, and the hand cases' closed-form trussness.
Edges are always the key-sorted (lo, hi) list, lo < hi.
"""
from types import SimpleNamespace

import numpy as np

import tc_ref
from lux_amd.graph import Graph


def edge_list(A):
    """(lo, hi) of every edge of the symmetric 0/1 matrix, key-sorted."""
    lo, hi = np.nonzero(np.triu(A, 1))  # row-major: ascending (lo, hi)
    return lo.astype(np.int64), hi.astype(np.int64)


def dense_support(g):
    """(edges i64[m, 2], support i64[m]): triangles per edge."""
    A = tc_ref.simple_matrix(g)
    lo, hi = edge_list(A)
    S = (A @ A) * A
    return np.stack([lo, hi], 1), S[lo, hi].astype(np.int64)


def dense_peel(g, k):
    """Synchronous peel: every round drops all edges whose support inside
    the current subgraph is below k - 2; a round counts even when it drops
    nothing, and no round runs on a graph without edges or for k == 2.
    Returns (alive bool[m] over the key-sorted edges, rounds)."""
    A = tc_ref.simple_matrix(g)
    lo, hi = edge_list(A)
    rounds = 0
    while k > 2 and A.any():
        rounds += 1
        S = (A @ A) * A
        dead = (A > 0) & (S < k - 2)
        if not dead.any():
            break
        A[dead] = 0.0
    return A[lo, hi] > 0, rounds


def dense_truss(g):
    """trussness i64[m] over the key-sorted edges: an edge that survives the
    peel for k but not for k + 1 has trussness k."""
    A = tc_ref.simple_matrix(g)
    lo, hi = edge_list(A)
    truss = np.full(lo.size, 2, np.int64)
    k = 3
    while A.any():
        while True:  # peel to the k-truss
            S = (A @ A) * A
            dead = (A > 0) & (S < k - 2)
            if not dead.any():
                break
            A[dead] = 0.0
        truss[A[lo, hi] > 0] = k
        k += 1
    return truss


def vertices_of(edges, alive):
    return int(np.unique(edges[alive]).size)


def hand_cases():
    """tc_ref.hand_cases() with closed-form trussness: a constant for every
    edge, or a function of the (lo, hi) arrays."""
    const = dict(empty=2, single_edge=2, path=2, one_way_triangle=3,
                 doubled_triangle_with_loops=3, k4=4, k5_minus_edge=4,
                 two_triangles_sharing_an_edge=3, star=2, bipartite=2, fan=3)
    out = []
    for c in tc_ref.hand_cases():
        t = const[c.name]
        out.append(SimpleNamespace(name=c.name, g=c.g,
                                   truss=lambda lo, hi, t=t:
                                   np.full(lo.shape, t, np.int64)))
    for n in (3, 6, 9):
        edges = [(a, b) for a in range(n) for b in range(a + 1, n)]
        out.append(SimpleNamespace(
            name=f"k{n}_clique",
            g=Graph.from_edges(n, [e[0] for e in edges],
                               [e[1] for e in edges]),
            truss=lambda lo, hi, n=n: np.full(lo.shape, n, np.int64)))
    # K_6 on 0..5 and the pendant triangle {5, 6, 7}
    edges = [(a, b) for a in range(6) for b in range(a + 1, 6)] + \
        [(5, 6), (6, 7), (7, 5)]
    out.append(SimpleNamespace(
        name="k6_with_pendant_triangle",
        g=Graph.from_edges(8, [e[0] for e in edges], [e[1] for e in edges]),
        truss=lambda lo, hi: np.where(hi <= 5, 6, 3).astype(np.int64)))
    return out
