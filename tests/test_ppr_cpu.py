"""Personalised PageRank on the CPU: cpu_ref.personalised_pagerank against a
closed form, against the PageRank oracle, and the leak at a dangling
vertex."""
import numpy as np

from lux_amd import cpu_ref
from lux_amd.graph import Graph
from lux_amd.types import PR_ALPHA
from test_msbfs_cpu import graph


def test_cycle_closed_form():
    """On a directed n-cycle the walk from the seed is at hop j with
    probability (1 - d) d^j, summed over the laps: / (1 - d^n)."""
    n, seed = 7, 3
    g = graph(n, [(i, (i + 1) % n) for i in range(n)])
    d = float(np.float32(0.85))
    x, iters, res = cpu_ref.personalised_pagerank(g, [seed], 0.85, 400)
    assert iters == 400 and len(res) == 400 and x.shape == (n, 1)
    hops = (np.arange(n) - seed) % n
    np.testing.assert_allclose(x[:, 0], (1 - d) * d ** hops / (1 - d ** n),
                               rtol=1e-12)
    x, iters, res = cpu_ref.personalised_pagerank(g, [seed], 0.85, 400,
                                                  tol=1e-3)
    assert iters == len(res) < 400 and res[-1] <= 1e-3 < res[-2]


def test_all_vertices_seed_is_pagerank():
    """d = PR_ALPHA and the all-vertices seed set is the PageRank recurrence;
    the fp32 oracle sums a row serially, one rounding per entry and a few
    for the epilogue, and nothing cancels."""
    g, iters = Graph.rmat(10, 8000, seed=3), 5
    x = cpu_ref.personalised_pagerank(g, [list(range(g.nv))], PR_ALPHA,
                                      iters)[0][:, 0]
    got = cpu_ref.pagerank(g, iters).astype(np.float64) * \
        np.maximum(g.out_degrees(), 1)
    indeg = np.diff(np.concatenate(([0], g.col_end)).astype(np.int64)).max()
    assert np.all(np.abs(got - x) <= 2 * iters * (indeg + 6) * 2.0 ** -24 * x)


def test_mass_leaks_at_a_dangling_vertex():
    g = graph(3, [(0, 1), (1, 2)])
    x = cpu_ref.personalised_pagerank(g, [0, [0, 2]], 0.5, 3)[0]
    assert x[:, 0].tolist() == [0.5, 0.25, 0.125]  # sums to 0.875
    assert x[:, 1].tolist() == [0.25, 0.125, 0.3125]
