"""Label propagation on the CPU: the C++ oracle cpu_ref.label_propagation on
hand cases whose labels, traces, intra-community edges and modularity were
worked out from the definition in API.md. Every comparison is equality."""
import numpy as np
import pytest

from lux_amd import cpu_ref
from lux_amd.graph import Graph


def graph(nv, edges):
    e = np.asarray(edges, np.uint32).reshape(-1, 2)
    return Graph.from_edges(nv, e[:, 0].copy(), e[:, 1].copy())


def clique(ids):
    return [(a, b) for a in ids for b in ids if a < b]


# name: (graph, {order: (labels, trace)}, (intra, m, modularity) or None)
CASES = {
    "barbell": (
        graph(6, clique([0, 1, 2]) + clique([3, 4, 5]) + [(2, 3)]),
        dict(degree=([0, 0, 0, 3, 3, 3], [(1, 6, 4), (2, 4, 0)]),
             id=([1, 1, 1, 2, 2, 2], [(1, 6, 5), (2, 4, 0)])),
        (6, 7, 0.35714285714285715)),
    "path6": (
        graph(6, [(i, i + 1) for i in range(5)]),
        dict(degree=([0, 0, 2, 2, 4, 4], [(1, 6, 3), (2, 0, 0)]),
             id=([1, 1, 1, 3, 3, 3], [(1, 6, 4), (2, 1, 0)])),
        None),
    "two_k5": (
        graph(10, clique(range(5)) + clique(range(5, 10)) + [(4, 5)]),
        dict(degree=([0] * 5 + [5] * 5, [(1, 10, 8), (2, 8, 0)]),
             id=([1] * 5 + [4] * 5, [(1, 10, 9), (2, 8, 0)])),
        (20, 21, 0.4523809523809524)),
    "star5": (
        graph(6, [(0, i) for i in range(1, 6)]),
        dict(degree=([1] * 6, [(1, 6, 5), (2, 1, 0)]),
             id=([1] * 6, [(1, 6, 5), (2, 1, 0)])),
        None),
    "loops_and_twins": (  # arcs 1->2, 2->1, 2->2: one simple edge
        graph(4, [(1, 2), (2, 1), (2, 2)]),
        dict(degree=([0, 2, 2, 3], [(1, 2, 1), (2, 0, 0)]),
             id=([0, 2, 2, 3], [(1, 2, 1), (2, 0, 0)])),
        None),
    "k4_tail": (
        graph(6, clique(range(4)) + [(3, 4), (4, 5)]),
        dict(degree=([0, 0, 0, 0, 4, 4], [(1, 6, 4), (2, 3, 0)]),
             id=([1, 1, 1, 1, 3, 3], [(1, 6, 5), (2, 4, 0)])),
        (7, 8, 0.1796875)),
}


@pytest.mark.parametrize("order", ["degree", "id"])
@pytest.mark.parametrize("name", CASES)
def test_hand_cases(name, order):
    g, want, pins = CASES[name]
    labels, trace = cpu_ref.label_propagation(g, order)
    assert labels.dtype == np.int32
    assert (labels.tolist(), trace) == want[order]
    st = cpu_ref.community_stats(g, labels)
    assert int(st["sizes"].sum()) == g.nv
    assert int(st["tot"].sum()) == 2 * st["m"]
    if pins:  # both orders find the same partition
        assert (st["intra"], st["m"], st["modularity"]) == pins


def test_init_and_one_sweep_keep_the_centre_on_a_tie():
    """Star, leaves 1..4 labelled 7 7 9 9 and the centre 9: the tie keeps 9;
    with the centre on 3 the smaller of the tied labels wins. One sweep is
    not convergence, so the trace has exactly one entry."""
    g = graph(10, [(0, i) for i in range(1, 5)])
    init = np.array([9, 7, 7, 9, 9, 5, 6, 7, 8, 9], np.int32)
    labels, trace = cpu_ref.label_propagation(g, "degree", init=init,
                                              max_sweeps=1)
    assert labels[0] == 9 and len(trace) == 1 and trace[0][1] == 5
    init[0] = 3
    labels, _ = cpu_ref.label_propagation(g, "degree", init=init,
                                          max_sweeps=1)
    assert labels[0] == 7
    with pytest.raises(ValueError):
        cpu_ref.label_propagation(g, init=np.full(10, 10, np.int32))
