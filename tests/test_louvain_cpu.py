"""Louvain on the CPU: the oracle cpu_ref.louvain on hand cases worked out
from the definition in API.md. Every comparison is equality."""
import numpy as np
import pytest

from lux_amd import cpu_ref
from lux_amd.graph import Graph
from test_lpa_cpu import CASES

# two cliques joined by one edge: W = 2m, in = 2 (m - 1), tot = m each, so
# Qnum = W * in - 2 m^2
TWO_CLIQUES = {"barbell": (3, 14 * 12 - 2 * 7 * 7),
               "two_k5": (5, 42 * 40 - 2 * 21 * 21)}


@pytest.mark.parametrize("order", ["degree", "id"])
@pytest.mark.parametrize("name", CASES)
def test_hand_cases(name, order):
    g = CASES[name][0]
    labels, levels, sweeps = cpu_ref.louvain(g, order)
    assert labels.dtype == np.int32
    n = levels[-1][1]
    assert sorted(set(labels.tolist())) == list(range(n))  # dense
    assert levels[-1][2:4] == (1, 0) and sweeps[-1][2] == 0
    assert [t[0] for t in levels] == list(range(len(levels)))
    if name in TWO_CLIQUES:
        size, qnum = TWO_CLIQUES[name]
        assert labels.tolist() == [0] * size + [1] * size
        assert levels[-1][4] == qnum == sweeps[-1][3]
    # Qnum of every level is modularity * W^2 of the labels cut there
    for cut in range(1, len(levels) + 1):
        lab, lv, _ = cpu_ref.louvain(g, order, max_levels=cut)
        assert lv == levels[:cut]
        st = cpu_ref.community_stats(g, lab)
        W = 2 * st["m"]
        assert lv[-1][4] == W * 2 * st["intra"] - \
            sum(int(t) ** 2 for t in st["tot"])
        if W:
            assert lv[-1][4] / (W * W) == pytest.approx(st["modularity"],
                                                        abs=1e-15)


def test_weights_sum_over_parallel_and_opposite_arcs():
    """Triangle 0 1 2 with the tail 2-3. Unit weights pair the vertices off;
    with the arcs 1->2, 2->1, 1->2 of weight 2 each, w(1,2) = 6 of W = 18
    draws everything into one community, whose Qnum is W * W - W^2 = 0."""
    g = Graph.from_edges(4, np.array([0, 0, 1, 2, 1, 2], np.uint32),
                         np.array([1, 2, 2, 1, 2, 3], np.uint32),
                         np.array([1, 1, 2, 2, 2, 1], np.int32))
    assert cpu_ref.louvain(g)[0].tolist() == [0, 0, 1, 1]
    labels, levels, sweeps = cpu_ref.louvain(g, weighted=True)
    assert labels.tolist() == [0, 0, 0, 0]
    assert levels == [(0, 4, 2, 3, 0), (1, 1, 1, 0, 0)]
    # the start: in = 0 and k = 2, 7, 8, 1
    g.weight[0] = 0
    with pytest.raises(ValueError):
        cpu_ref.louvain(g, weighted=True)


def test_limits_cut_where_they_say():
    g = Graph.rmat(8, 1500, seed=3)
    _, levels, sweeps = cpu_ref.louvain(g)
    assert len(levels) > 2 and levels[0][2] > 2
    lab, lv, sw = cpu_ref.louvain(g, max_sweeps=2, max_levels=2)
    assert [t[2] for t in lv] == [2, 2] and len(sw) == 4
    assert sw[:2] == sweeps[:2] and lv[0][4] == sweeps[1][3]
    assert int(lab.max()) + 1 == np.unique(lab).size < lv[1][1]
    init = np.zeros(g.nv, np.int32)
    assert cpu_ref.louvain(g, init=init, max_levels=1)[0].max() == 0
    with pytest.raises(ValueError):
        cpu_ref.louvain(g, init=np.full(g.nv, g.nv, np.int32))
