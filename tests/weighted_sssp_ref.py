"""Plain-numpy references for the weighted SSSP tests (no GPU, no native
code): the endpoint-hash weights, a synchronous Bellman-Ford that also
records what the push engine's frontier looks like per iteration, the
engine's push-versus-pull rule, and the hand-made graphs both test files
share.

The Bellman-Ford is independent of the Dijkstra oracle it checks
(lux_amd.cpu_ref.sssp_weighted): Jacobi sweeps over numpy arrays against a
binary heap in C++.
"""
import numpy as np

from lux_amd.graph import Graph

INF = 0xFFFFFFFF
SAT = 0xFFFFFFFE  # min(label + w, SAT): a finite distance never reaches INF
M64 = (1 << 64) - 1


def _splitmix64(x):
    """splitmix64 of src/include/lux/rmat.h over a uint64 array."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def hash_weights_np(src, dst, wmax, seed=1):
    """w = 1 + splitmix64(seed ^ 0x5757575757575757 ^ (src << 32 | dst))
    % wmax — the formula of edge_hash_weight, written out again."""
    key = (np.asarray(src, np.uint64) << np.uint64(32)) \
        | np.asarray(dst, np.uint64)
    h = _splitmix64(np.uint64(seed) ^ np.uint64(0x5757575757575757) ^ key)
    return (np.uint64(1) + h % np.uint64(wmax)).astype(np.int32)


def edge_dst(g):
    """dst of every CSC edge (edges are grouped by dst)."""
    degs = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    return np.repeat(np.arange(g.nv, dtype=np.int64), degs)


def bellman_ford(g, source):
    """Synchronous (Jacobi) min-plus relaxation from `source` over
    g.weight with the saturating add. Iteration k relaxes the out-edges of
    the vertices whose label changed in iteration k-1 (the frontier).

    Returns (labels u32, sizes, vols): per iteration the frontier size at
    its start and the summed out-degree of the frontier — the last
    iteration is the one that changes nothing."""
    nv = g.nv
    src = g.src.astype(np.int64)
    dst = edge_dst(g)
    w = np.asarray(g.weight, np.int32).view(np.uint32).astype(np.uint64)
    outdeg = np.bincount(src, minlength=nv)
    lab = np.full(nv, INF, np.uint64)
    lab[source] = 0
    frontier = np.zeros(nv, bool)
    frontier[source] = True
    sizes, vols = [], []
    while frontier.any():
        assert len(sizes) <= nv, "no fixed point within nv iterations"
        sizes.append(int(frontier.sum()))
        vols.append(int(outdeg[frontier].sum()))
        act = frontier[src]
        cand = np.minimum(lab[src[act]] + w[act], np.uint64(SAT))
        new = lab.copy()
        np.minimum.at(new, dst[act], cand)
        frontier = new != lab
        lab = new
    return lab.astype(np.uint32), sizes, vols


def predict_pull(nv, ne, sizes, vols, evol_div=8):
    """The engine's decision per iteration: pull iff the frontier holds
    more than nv//16 vertices or its out-edge volume exceeds ne//evol_div
    (8 without a visited bitmap; LUX_PUSH_EVOL_DIV overrides it). The seed
    frontier's volume is not priced (its meta record carries 0)."""
    flags = []
    for k, (n, vol) in enumerate(zip(sizes, vols)):
        if k == 0:
            vol = 0
        flags.append(bool(n > nv // 16 or vol > ne // evol_div))
    return flags


def graph_from_wedges(nv, edges):
    """Graph from (src, dst, weight) triples."""
    s, d, w = (np.array(x) for x in zip(*edges))
    return Graph.from_edges(nv, s.astype(np.uint32), d.astype(np.uint32),
                            w.astype(np.int64).astype(np.int32))


BIG = 0x7FFFFFFF

# name -> (nv, [(src, dst, w)], expected labels from vertex 0)
HAND_CASES = {
    # vertex 1 is reached with 10 in iteration 1 and improved to 3 in
    # iteration 3, through 0 -> 2 -> 3 -> 1; one-shot discovery or a
    # settled-row skip leaves 10. Vertices 4..9: a chain hanging off 1
    # that has to be corrected after it.
    "label_correction": (
        10,
        [(0, 1, 10), (0, 2, 1), (2, 3, 1), (3, 1, 1),
         (1, 4, 1), (4, 5, 1), (5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1)],
        [0, 3, 1, 2, 4, 5, 6, 7, 8, 9]),
    # zero-weight edges and a zero-weight cycle 1 -> 2 -> 1
    "zero_cycle": (
        5,
        [(0, 1, 0), (1, 2, 0), (2, 1, 0), (2, 3, 2), (3, 0, 0), (3, 4, 0)],
        [0, 0, 0, 2, 2]),
    # parallel edges with different weights: the minimum wins
    "parallel": (
        4,
        [(0, 1, 7), (0, 1, 3), (0, 1, 9), (1, 2, 1), (1, 2, 1), (0, 2, 5),
         (2, 3, 4), (2, 3, 2)],
        [0, 3, 4, 6]),
    # {4, 5, 6} is not reachable from 0 and stays INF
    "unreachable": (
        7,
        [(0, 1, 2), (1, 2, 2), (2, 0, 2), (3, 0, 1), (4, 5, 1), (5, 6, 1),
         (6, 4, 1), (4, 1, 1)],
        [0, 2, 4, INF, INF, INF, INF]),
    # two edges of weight 0x7FFFFFFF in a row give 0xFFFFFFFE exactly; one
    # more edge must stay there: no wrap, and not INF
    "saturation": (
        5,
        [(0, 1, BIG), (1, 2, BIG), (2, 3, 5), (3, 4, BIG)],
        [0, BIG, SAT, SAT, SAT]),
}


def hand_graph(name, pad_to=None):
    """The named hand-made graph; pad_to adds isolated vertices (INF)."""
    nv, edges, want = HAND_CASES[name]
    want = np.array(want, np.uint32)
    if pad_to is not None and pad_to > nv:
        want = np.concatenate([want, np.full(pad_to - nv, INF, np.uint32)])
        nv = pad_to
    return graph_from_wedges(nv, edges), want
