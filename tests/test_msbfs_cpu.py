"""Multi-source BFS on the CPU: cpu_ref.multi_source_bfs and
multi_source_stats against depth rows written by hand from the definition in
API.md. Integer results are compared by equality."""
import numpy as np
import pytest

from lux_amd import cpu_ref
from lux_amd.graph import Graph


def graph(nv, edges):
    e = np.asarray(edges, np.uint32).reshape(-1, 2)
    return Graph.from_edges(nv, e[:, 0].copy(), e[:, 1].copy())


# name: (graph, sources, depth rows)
CASES = {
    "path5": (graph(5, [(i, i + 1) for i in range(4)]), [0, 2],
              [[0, 1, 2, 3, 4], [-1, -1, 0, 1, 2]]),
    "cycle4": (graph(4, [(0, 1), (1, 2), (2, 3), (3, 0)]), [0, 3],
               [[0, 1, 2, 3], [1, 2, 3, 0]]),
    "in_star": (graph(5, [(i, 0) for i in range(1, 5)]), [1, 0],
                [[1, 0, -1, -1, -1], [0, -1, -1, -1, -1]]),
    "out_star": (graph(5, [(0, i) for i in range(1, 5)]), [0, 3],
                 [[0, 1, 1, 1, 1], [-1, -1, -1, 0, -1]]),
    "two_parts": (  # a parallel edge 0 -> 1, a self-loop at 1, 5 isolated
        graph(6, [(0, 1), (0, 1), (1, 1), (1, 2), (3, 4), (4, 3)]), [0, 3, 5],
        [[0, 1, 2, -1, -1, -1], [-1, -1, -1, 0, 1, -1],
         [-1, -1, -1, -1, -1, 0]]),
}


@pytest.mark.parametrize("name", CASES)
def test_hand_cases(name):
    g, sources, rows = CASES[name]
    rows = np.array(rows, np.int32)
    depths = cpu_ref.multi_source_bfs(g, sources)
    assert depths.dtype == np.int32 and np.array_equal(depths, rows)
    st = cpu_ref.multi_source_stats(g, sources)
    hit = rows >= 0
    assert np.array_equal(st["reach"], hit.sum(0))
    assert np.array_equal(st["dist_sum"], (rows * hit).sum(0))
    assert st["reached"].tolist() == hit.sum(1).tolist()
    assert st["farness"].tolist() == (rows * hit).sum(1).tolist()
    assert st["eccentricity"].tolist() == rows.max(1).tolist()
    assert [sum(c) for c in st["level_counts"]] == hit.sum(1).tolist()
    assert sum(t[5] for t in st["level_trace"]) == int(hit.sum())
    assert [t[1] for t in st["level_trace"]] == list(range(rows.max() + 1))


def test_path5_by_hand():
    g, sources, _ = CASES["path5"]
    st = cpu_ref.multi_source_stats(g, sources, div=8)
    assert st["reach"].tolist() == [1, 1, 2, 2, 2]
    assert st["dist_sum"].tolist() == [0, 1, 2, 4, 6]
    assert st["harmonic"].tolist() == [0.0, 1.0, 0.5, 1.0 + 1.0 / 3.0, 0.75]
    assert st["level_counts"] == [[1, 1, 1, 1, 1], [1, 1, 1]]
    assert st["closeness"].tolist() == [4.0 / 10.0, 2.0 / 3.0]
    # ne = 5: pull iff volume * 8 > 5, i.e. any out-edge at all
    assert st["level_trace"] == [
        (0, 0, "pull", 2, 2, 2), (0, 1, "pull", 2, 2, 2),
        (0, 2, "pull", 2, 1, 2), (0, 3, "pull", 1, 1, 1),
        (0, 4, "push", 1, 0, 1)]
    assert [t[2] for t in cpu_ref.multi_source_stats(
        g, sources, div=2)["level_trace"]] == ["push"] * 5


def test_batches_accumulate_and_a_lone_source_has_closeness_zero():
    g, _, _ = CASES["two_parts"]
    st = cpu_ref.multi_source_stats(g, [0, 3, 5], batch=2)
    assert [t[0] for t in st["level_trace"]] == [0, 0, 0, 1]
    assert st["closeness"].tolist() == [2.0 / 3.0, 1.0, 0.0]
    assert st["harmonic"].tolist() == [0.0, 1.0, 0.5, 0.0, 1.0, 0.0]
