"""SCC references for test_scc_cpu.py / test_gpu_scc.py.

Numpy only (no GPU, no C++ oracle): sync_schedule, the synchronous trim /
forward-backward / colouring schedule SCCEngine follows (so the authority
for its phase statistics), the hand cases with their closed-form labels, and
the builders of the star ladder, the planted graphs and the two giants.
"""
from types import SimpleNamespace

import numpy as np

import tc_ref
from lux_amd.graph import Graph


def _csr(nv, rows, cols):
    order = np.argsort(rows, kind="stable")
    ptr = np.zeros(nv + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=nv))
    return ptr, cols[order]


def _neighbours(ptr, adj, rows):
    """(the given rows repeated per entry, their adj entries)."""
    starts = ptr[rows]
    lens = ptr[rows + 1] - starts
    first = np.cumsum(lens) - lens
    idx = np.arange(int(lens.sum())) - np.repeat(first, lens) + \
        np.repeat(starts, lens)
    return np.repeat(rows, lens), adj[idx]


def sync_schedule(g):
    """(label i64[nv], stats) of the synchronous schedule:
    a. trim to fixpoint: a round removes every alive vertex without an alive
       in- or without an alive out-neighbour (self-loops never count);
    b. the pivot (max in_cnt * out_cnt, lowest id first), its forward and
       backward reach over alive edges, the intersection dies with its
       largest id as the label;
    c. recount and trim;
    d. colour rounds while anything is alive: colour = id, the maximum
       propagated along alive out-edges by Jacobi sweeps to the fixpoint,
       one backward traversal from all roots (colour == id) inside equal
       colours, the reached die with label = colour; recount and trim.
    stats: trim_rounds (non-empty), trimmed, pivot (None if b never ran),
    fwbw, reach_rounds (non-empty frontiers of all traversals, the seeds
    included), colour_rounds, colour_sweeps (Jacobi sweeps with a non-empty
    frontier, the last, changeless one included)."""
    nv = g.nv
    src, dst = tc_ref.edge_lists(g)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    optr, oadj = _csr(nv, src, dst)
    iptr, iadj = _csr(nv, dst, src)
    alive = np.ones(nv, bool)
    label = np.full(nv, -1, np.int64)
    st = dict(trim_rounds=0, trimmed=0, pivot=None, fwbw=0, reach_rounds=0,
              colour_rounds=0, colour_sweeps=0)

    def trim():
        on = alive[src] & alive[dst]
        in_cnt = np.bincount(dst[on], minlength=nv)
        out_cnt = np.bincount(src[on], minlength=nv)
        rnd = np.nonzero(alive & ((in_cnt == 0) | (out_cnt == 0)))[0]
        while rnd.size:
            st["trim_rounds"] += 1
            st["trimmed"] += rnd.size
            label[rnd] = rnd
            alive[rnd] = False
            _, outs = _neighbours(optr, oadj, rnd)
            outs = outs[alive[outs]]
            in_cnt -= np.bincount(outs, minlength=nv)
            _, ins = _neighbours(iptr, iadj, rnd)
            ins = ins[alive[ins]]
            out_cnt -= np.bincount(ins, minlength=nv)
            cand = np.unique(np.concatenate([outs, ins]))
            rnd = cand[(in_cnt[cand] == 0) | (out_cnt[cand] == 0)]
        return in_cnt, out_cnt

    def reach(seeds, ptr, adj, colour=None):
        seen = np.zeros(nv, bool)
        seen[seeds] = True
        front = seeds
        while front.size:
            st["reach_rounds"] += 1
            rows, nb = _neighbours(ptr, adj, front)
            ok = alive[nb] & ~seen[nb]
            if colour is not None:
                ok &= colour[nb] == colour[rows]
            front = np.unique(nb[ok])
            seen[front] = True
        return seen

    in_cnt, out_cnt = trim()
    if alive.any():
        prod = np.where(alive, in_cnt.astype(object) * out_cnt.astype(object),
                        -1)
        pivot = int(np.argmax(prod == prod.max()))
        st["pivot"] = pivot
        seed = np.asarray([pivot])
        comp = np.nonzero(reach(seed, optr, oadj) & reach(seed, iptr, iadj))[0]
        st["fwbw"] = comp.size
        label[comp] = comp.max()
        alive[comp] = False
        trim()
    bound = nv
    while alive.any():
        assert bound > 0
        bound -= 1
        st["colour_rounds"] += 1
        colour = np.arange(nv)
        front = np.nonzero(alive)[0]
        while front.size:
            st["colour_sweeps"] += 1
            rows, nb = _neighbours(optr, oadj, front)
            ok = alive[nb]
            new = colour.copy()
            np.maximum.at(new, nb[ok], colour[rows[ok]])
            front = np.nonzero(new != colour)[0]
            colour = new
        roots = np.nonzero(alive & (colour == np.arange(nv)))[0]
        got = np.nonzero(reach(roots, iptr, iadj, colour))[0]
        label[got] = colour[got]
        alive[got] = False
        trim()
    return label, st


# ---- graphs ----

def _graph(nv, edges):
    src = np.asarray([e[0] for e in edges], np.uint32)
    dst = np.asarray([e[1] for e in edges], np.uint32)
    return Graph.from_edges(nv, src, dst)


def _case(name, nv, edges, label, **stats):
    return SimpleNamespace(name=name, g=_graph(nv, edges),
                           label=np.asarray(label, np.int64), stats=stats)


PATH_N = 4001
STAR_LEAVES = 5000


def chain2_edges(n, descending=False):
    """n two-cycles, pair k with one edge to pair k + 1. Ascending: pair k
    is (2k, 2k + 1); descending: pair k is (2(n-1-k), 2(n-1-k) + 1). The
    edge between pairs leaves the odd vertex and enters the even one."""
    base = [2 * (n - 1 - k) if descending else 2 * k for k in range(n)]
    edges = []
    for k, b in enumerate(base):
        edges += [(b, b + 1), (b + 1, b)]
        if k + 1 < n:
            edges.append((b + 1, base[k + 1]))
    return edges


def chain2_labels(n):
    return np.repeat(2 * np.arange(n) + 1, 2)


def star_edges(leaves, out=True, back=False, hub=0, first=1):
    """hub -> leaf for every leaf (out), leaf -> hub (not out), or both
    (back)."""
    edges = []
    for leaf in range(first, first + leaves):
        if out or back:
            edges.append((hub, leaf))
        if not out or back:
            edges.append((leaf, hub))
    return edges


def two_way_star_with_tail(leaves):
    """(nv, edges, label): hub 0, leaves 1..L both ways, and the tail
    leaf 1 -> L+1 -> L+2 -> L+3."""
    L = leaves
    edges = star_edges(L, back=True) + [(1, L + 1), (L + 1, L + 2),
                                        (L + 2, L + 3)]
    label = [L] * (L + 1) + [L + 1, L + 2, L + 3]
    return L + 4, edges, label


def hand_cases():
    """Small graphs with closed-form labels and, where the schedule is the
    point, closed-form statistics."""
    n, L = PATH_N, STAR_LEAVES
    return [
        _case("empty", 4, [], [0, 1, 2, 3], trim_rounds=1, trimmed=4,
              pivot=None, fwbw=0, reach_rounds=0, colour_rounds=0),
        _case("single_vertex", 1, [], [0], trim_rounds=1, trimmed=1),
        # 2 has both counters 0 at the start: removed exactly once
        _case("isolated_vertex", 3, [(0, 1), (1, 0)], [1, 1, 2],
              trim_rounds=1, trimmed=1, pivot=0, fwbw=2),
        _case("self_loop", 1, [(0, 0)], [0], trim_rounds=1, trimmed=1),
        # b loses both counters in the same round
        _case("path3", 3, [(0, 1), (1, 2)], [0, 1, 2], trim_rounds=2,
              trimmed=3, pivot=None),
        _case("path4001", n, [(i, i + 1) for i in range(n - 1)],
              np.arange(n), trim_rounds=n // 2 + 1, trimmed=n, pivot=None,
              colour_rounds=0),
        _case("cycle4001", n, [(i, (i + 1) % n) for i in range(n)],
              [n - 1] * n, trim_rounds=0, trimmed=0, pivot=0, fwbw=n,
              reach_rounds=2 * n, colour_rounds=0),
        _case("chain2_ascending", 128, chain2_edges(64), chain2_labels(64),
              pivot=1, fwbw=2, colour_rounds=1, trim_rounds=0),
        _case("chain2_descending", 128, chain2_edges(64, True),
              chain2_labels(64), pivot=0, fwbw=2, colour_rounds=63,
              trim_rounds=0),
        _case("parallel_edges", 4,
              3 * [(0, 1), (1, 0)] + 3 * [(1, 2), (2, 3)], [1, 1, 2, 3],
              trim_rounds=2, trimmed=2, pivot=0, fwbw=2),
        # the hub's out_cnt takes L concurrent decrements, one enqueue
        _case("out_star", L + 1, star_edges(L), np.arange(L + 1),
              trim_rounds=1, trimmed=L + 1, pivot=None),
        _case("in_star", L + 1, star_edges(L, out=False), np.arange(L + 1),
              trim_rounds=1, trimmed=L + 1, pivot=None),
        _case("two_way_star", L + 1, star_edges(L, back=True),
              [L] * (L + 1), trim_rounds=0, trimmed=0, pivot=0, fwbw=L + 1,
              reach_rounds=4, colour_rounds=0),
    ]


STAR_CASES = ("out_star", "in_star", "two_way_star")


def ladder_leaves(hub):
    return [hub - 1, hub, hub + 1, 2 * hub, 2 * hub + 1]


def ladder_case(leaves):
    nv, edges, label = two_way_star_with_tail(leaves)
    return _case(f"star{leaves}_tail", nv, edges, label, trim_rounds=3,
                 trimmed=3, pivot=0, fwbw=leaves + 1, colour_rounds=0)


def planted(nblocks, maxsize, extra, seed):
    """(g, label): nblocks blocks of uniform size in [1, maxsize]; a block of
    two or more vertices is a directed cycle plus size // 2 random chords;
    `extra` random edges between blocks, always from the lower block index
    to the higher; ids shuffled by a seeded permutation. The label of a
    block is its largest shuffled id."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, maxsize + 1, nblocks)
    first = np.cumsum(sizes) - sizes
    nv = int(sizes.sum())
    block = np.repeat(np.arange(nblocks), sizes)
    src, dst = [], []
    for b in range(nblocks):
        s, f = int(sizes[b]), int(first[b])
        if s < 2:
            continue
        ids = f + np.arange(s)
        src.append(ids)
        dst.append(f + (np.arange(s) + 1) % s)
        src.append(f + rng.integers(0, s, s // 2))
        dst.append(f + rng.integers(0, s, s // 2))
    if nblocks > 1 and extra:
        a = rng.integers(0, nblocks, extra)
        b = rng.integers(0, nblocks, extra)
        ok = a != b
        lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
        src.append(first[lo] + rng.integers(0, sizes[lo]))
        dst.append(first[hi] + rng.integers(0, sizes[hi]))
    src = np.concatenate(src) if src else np.zeros(0, np.int64)
    dst = np.concatenate(dst) if dst else np.zeros(0, np.int64)
    perm = rng.permutation(nv)
    top = np.zeros(nblocks, np.int64)
    np.maximum.at(top, block, perm)
    g = Graph.from_edges(nv, perm[src].astype(np.uint32),
                         perm[dst].astype(np.uint32))
    label = np.empty(nv, np.int64)
    label[perm] = top[block]
    return g, label


def two_giants(scale=10, ne=20000, seed=3, bridges=50):
    """Two copies of Graph.rmat(scale, ne, seed) on disjoint id ranges and
    `bridges` one-way edges from the first copy to the second."""
    g = Graph.rmat(scale, ne, seed=seed)
    src, dst = tc_ref.edge_lists(g)
    n = g.nv
    rng = np.random.default_rng(seed)
    bs = rng.integers(0, n, bridges)
    bd = n + rng.integers(0, n, bridges)
    return Graph.from_edges(
        2 * n, np.concatenate([src, src + n, bs]).astype(np.uint32),
        np.concatenate([dst, dst + n, bd]).astype(np.uint32))


def same_partition(a, b):
    """Whether two label arrays give the same partition of the vertices."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    if a.shape != b.shape:
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return np.unique(pairs[:, 0]).size == pairs.shape[0] == \
        np.unique(pairs[:, 1]).size
