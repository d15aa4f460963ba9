"""cpu_ref.cliques (the sorted-list C++ oracle of CliqueEngine) against
closed forms, against cpu_ref.triangles at k = 3, and against totals from an
independent big-int bit-set count in degree order."""
from math import comb

import numpy as np
import pytest

from lux_amd import cpu_ref
from lux_amd.graph import Graph

# Graph.rmat(10, 40000, seed=3, sym=True): 12,252 simple edges
RMAT10_CLIQUES = {3: 103301, 4: 649951, 5: 3068368, 6: 11188703}


def multipartite(parts, size):
    """The complete multipartite graph, vertex v in part v % parts."""
    n = parts * size
    a, b = np.meshgrid(np.arange(n, dtype=np.uint32),
                       np.arange(n, dtype=np.uint32))
    keep = (a % parts) != (b % parts)
    return Graph.from_edges(n, a[keep], b[keep])


@pytest.mark.parametrize("k", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("n", [2, 8, 20])
def test_complete_graph(n, k):
    g = multipartite(n, 1)
    total, pv = cpu_ref.cliques(g, k)
    assert total == comb(n, k)
    assert (pv == comb(n - 1, k - 1)).all() and pv.dtype == np.uint64


@pytest.mark.parametrize("k", [3, 4, 5, 6])
def test_five_partite(k):
    total, pv = cpu_ref.cliques(multipartite(5, 13), k)
    assert total == comb(5, k) * 13 ** k
    assert (pv == comb(4, k - 1) * 13 ** (k - 1)).all()


@pytest.mark.parametrize("sym", [True, False])
def test_rmat(sym):
    g = Graph.rmat(10, 40000, seed=3, sym=sym)
    t3, pv3 = cpu_ref.triangles(g)
    for k in RMAT10_CLIQUES:
        total, pv = cpu_ref.cliques(g, k)
        assert int(pv.sum()) == k * total
        if sym:
            assert total == RMAT10_CLIQUES[k]
        if k == 3:
            assert total == t3 and np.array_equal(pv, pv3)


@pytest.mark.parametrize("k", [2, 9])
def test_k_out_of_range(k):
    with pytest.raises(ValueError):
        cpu_ref.cliques(multipartite(4, 1), k)
