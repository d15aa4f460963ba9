"""Greedy-colouring references for test_colouring_cpu.py /
test_gpu_colouring.py.

Numpy only (no GPU, no C++ oracle): the priority order, the sequential greedy
colouring in that order, the synchronous Jones-Plassmann schedule (the one
ColouringEngine follows, so also the authority for its round count and
per-round sizes), a verifier of the three defining properties, the hand
cases with their closed forms in id order, the clique staircase and the hub
ladder.
"""
from types import SimpleNamespace

import numpy as np

import kcore_ref
import tc_ref
from lux_amd.graph import Graph

ORDERS = ("degree", "id", "hash")
M64 = (1 << 64) - 1


def splitmix64(x):
    """lux::splitmix64 on a uint64 array (wrap-around arithmetic)."""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def priority(g, order="degree", seed=1):
    """rank i64[nv]: rank[v] < rank[u] iff v precedes u."""
    ids = np.arange(g.nv, dtype=np.int64)
    if order == "id":
        return ids
    if order == "degree":
        ptr, _ = kcore_ref.simple_adjacency(g)
        key = -np.diff(ptr)
    elif order == "hash":
        key = (splitmix64(ids.astype(np.uint64) ^ np.uint64(seed & M64)) >>
               np.uint64(1)).astype(np.int64)
    else:
        raise ValueError(order)
    perm = np.lexsort((ids, key))  # by key, ties by id
    rank = np.empty(g.nv, np.int64)
    rank[perm] = ids
    return rank


def split(g, order="degree", seed=1):
    """(rank, ptr, adj, is_pred): the simple adjacency and, per entry, whether
    the neighbour precedes the row's vertex."""
    rank = priority(g, order, seed)
    ptr, adj = kcore_ref.simple_adjacency(g)
    row = np.repeat(np.arange(g.nv), np.diff(ptr))
    return rank, ptr, adj, rank[adj] < rank[row]


def pred_succ_counts(g, order="degree", seed=1):
    """(npred, nsucc) i64[nv]."""
    _, ptr, adj, is_pred = split(g, order, seed)
    row = np.repeat(np.arange(g.nv), np.diff(ptr))
    npred = np.bincount(row[is_pred], minlength=g.nv)
    return npred, np.diff(ptr) - npred


def _mex(c):
    """The smallest non-negative integer not in the i64 array c."""
    seen = np.zeros(c.size + 2, bool)
    seen[c[(c >= 0) & (c <= c.size)]] = True
    return int(np.argmin(seen))


def greedy(g, order="degree", seed=1):
    """colour i64[nv]: one sequential pass in priority order, every vertex
    taking the smallest colour none of its already coloured neighbours
    has."""
    rank = priority(g, order, seed)
    ptr, adj = kcore_ref.simple_adjacency(g)
    colour = np.full(g.nv, -1, np.int64)
    for v in np.argsort(rank, kind="stable"):
        colour[v] = _mex(colour[adj[ptr[v]:ptr[v + 1]]])
    return colour


def sync_jp(g, order="degree", seed=1):
    """(colour i64[nv], rounds, per-round sizes) of the synchronous
    Jones-Plassmann schedule: a round colours every uncoloured vertex whose
    predecessors are all coloured (the mex over the predecessors only), then
    takes it off its successors' pending counts."""
    _, ptr, adj, is_pred = split(g, order, seed)
    row = np.repeat(np.arange(g.nv), np.diff(ptr))
    pending = np.bincount(row[is_pred], minlength=g.nv)
    colour = np.full(g.nv, -1, np.int64)
    front = np.nonzero(pending == 0)[0]
    sizes = []
    while front.size:
        sizes.append(int(front.size))
        for v in front:
            sl = slice(ptr[v], ptr[v + 1])
            colour[v] = _mex(colour[adj[sl][is_pred[sl]]])
        pending[front] = -1  # done
        starts, lens = ptr[front], ptr[front + 1] - ptr[front]
        first = np.cumsum(lens) - lens
        idx = np.arange(int(lens.sum())) - np.repeat(first, lens) + \
            np.repeat(starts, lens)
        succ = adj[idx][~is_pred[idx]]
        pending -= np.bincount(succ, minlength=g.nv)
        front = np.nonzero(pending == 0)[0]
    assert (colour >= 0).all()
    return colour, len(sizes), sizes


def verify(g, colour, order="degree", seed=1):
    """The number of vertices breaking a defining property: colour outside
    [0, |pred(v)|]; an edge to a vertex of the same colour; some
    c < colour[v] that no predecessor has. Zero iff colour is THE greedy
    colouring in this order (by induction along the order)."""
    colour = np.asarray(colour, np.int64)
    _, ptr, adj, is_pred = split(g, order, seed)
    bad = 0
    for v in range(g.nv):
        sl = slice(ptr[v], ptr[v + 1])
        nb = colour[adj[sl]]
        pc = nb[is_pred[sl]]
        c = colour[v]
        ok = 0 <= c <= pc.size and not (nb == c).any() and \
            np.unique(pc[(pc >= 0) & (pc < c)]).size == c
        bad += not ok
    return bad


# ---------------- hand cases ----------------

PATH_N = 4001
STAR_LEAVES = 5000
CROWN_N = 70
CLIQUE_N = 40


def _graph(nv, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return Graph.from_edges(nv, e[:, 0].astype(np.uint32),
                            e[:, 1].astype(np.uint32))


def clique(n):
    """K_n: in id order colour[v] = v, n rounds, and the predecessor rows
    take every length 0..n-1."""
    a, b = np.triu_indices(n, 1)
    return Graph.from_edges(n, a.astype(np.uint32), b.astype(np.uint32))


def _case(name, g, colour=None, rounds=None, ncolours=None):
    return SimpleNamespace(
        name=name, g=g, rounds=rounds, ncolours=ncolours,
        colour=None if colour is None else np.asarray(colour, np.int64))


def hand_cases():
    """Closed forms in id order: `colour`, `rounds` and `ncolours` (None
    where there is no closed form). The other orders are compared with the
    oracle only."""
    tc = {c.name: c.g for c in tc_ref.hand_cases()}
    n, L, k = CROWN_N, STAR_LEAVES, CLIQUE_N
    crown = [(2 * i, 2 * j + 1) for i in range(n) for j in range(n)
             if i != j]
    return [
        _case("empty4", tc["empty"], [0] * 4, rounds=1, ncolours=1),
        # the cascade: one vertex a round
        _case("path4001", _graph(PATH_N, [(i, i + 1)
                                          for i in range(PATH_N - 1)]),
              np.arange(PATH_N) & 1, rounds=PATH_N, ncolours=2),
        _case(f"k{k}", clique(k), np.arange(k), rounds=k, ncolours=k),
        # a successor row longer than the hub limit
        _case("star5000", _graph(L + 1, [(0, i) for i in range(1, L + 1)]),
              [0] + [1] * L, rounds=2, ncolours=2),
        # L concurrent decrements on one pending word, and a predecessor row
        # longer than the hub limit
        _case("reverse_star5000", _graph(L + 1, [(L, i) for i in range(L)]),
              [0] * L + [1], rounds=2, ncolours=2),
        # u_i = 2i, v_i = 2i + 1, u_i ~ v_j iff i != j: greedy in id order
        # needs n colours on a 2-colourable graph
        _case("crown70", _graph(2 * n, crown), np.repeat(np.arange(n), 2),
              rounds=n, ncolours=n),
        _case("doubled_triangle_with_loops",
              tc["doubled_triangle_with_loops"], [0, 1, 2, 0], rounds=3,
              ncolours=3),
        _case("one_way_triangle", tc["one_way_triangle"], [0, 1, 2],
              rounds=3, ncolours=3),
        # users 0..63 first, then the items: two colours, two rounds
        _case("bipartite", tc["bipartite"], rounds=2, ncolours=2),
    ]


def staircase_sizes(window):
    return [31, 32, 33, 63, 64, 65, window - 1, window, window + 1,
            window + 2]


# ---------------- hub ladder ----------------

LADDER_ROWS_PER_DEGREE = 2
LADDER_BAND = 8


def ladder(hub, side, seed=17):
    """Rows of the lengths kcore_ref.ladder_degrees(hub),
    LADDER_ROWS_PER_DEGREE per length D, each adjacent to a seeded D-subset
    of a pool of P = max D + 2 vertices and to nothing else. Pool vertex j is
    also adjacent to the j % LADDER_BAND pool vertices before it, so the
    pool holds LADDER_BAND colours in id order. side "below": ids [0, R) the
    rows, [R, R + P) the pool — in id order a row has D successors and no
    predecessor; side "above": [0, P) the pool, [P, P + R) the rows — a row
    has D predecessors and no successor.

    Returns g, rows, degrees (per row)."""
    rng = np.random.default_rng(seed)
    degrees = np.repeat(kcore_ref.ladder_degrees(hub),
                        LADDER_ROWS_PER_DEGREE)
    R = degrees.size
    P = int(degrees.max()) + 2
    if side == "below":
        rows, pool = np.arange(R), np.arange(R, R + P)
    elif side == "above":
        pool, rows = np.arange(P), np.arange(P, P + R)
    else:
        raise ValueError(side)
    src, dst = [], []
    for j in range(P):
        back = j % LADDER_BAND
        src.append(np.full(back, pool[j]))
        dst.append(pool[j - back:j])
    for r, D in zip(rows, degrees):
        src.append(np.full(D, r))
        dst.append(rng.choice(pool, D, replace=False))
    src = np.concatenate(src)
    dst = np.concatenate(dst)
    flip = rng.random(src.size) < 0.5  # the direction given must not matter
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    return SimpleNamespace(
        g=Graph.from_edges(R + P, src.astype(np.uint32),
                           dst.astype(np.uint32)),
        rows=rows, degrees=degrees, pool=pool)
