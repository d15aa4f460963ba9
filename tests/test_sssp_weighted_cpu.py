"""Weighted SSSP on the CPU: the Dijkstra oracle against a numpy
Bellman-Ford, the endpoint-hash weights against their formula, the check
oracle, and the native driver's refusal of -weighted."""
import os
import subprocess

import numpy as np
import pytest

import weighted_sssp_ref as ref

from lux_amd import cpu_ref
from lux_amd.graph import Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rmat_weighted(scale, ne, seed, wmax):
    """One seed for the edges and for their weights."""
    g = Graph.rmat(scale, ne, seed=seed)
    g.hash_weights(wmax, seed=seed)
    return g


# (scale, ne, seed, wmax) -> frontier sizes and pull decisions of the
# synchronous traversal from vertex 0, worked out independently of this
# code base: they pin the hash formula and the decision rule
TRACES = {
    (10, 8000, 3, 16): ([1, 249, 515, 378, 172, 39, 1],
                        [False, True, True, True, True, False, False]),
    (12, 300000, 5, 16): ([1, 1844, 3059, 2199, 228, 4, 1],
                          [False, True, True, True, False, False, False]),
}


@pytest.mark.parametrize("spec", sorted(TRACES))
def test_bellman_ford_trace(spec):
    g = _rmat_weighted(*spec)
    want, sizes, vols = ref.bellman_ford(g, 0)
    assert np.array_equal(cpu_ref.sssp_weighted(g, 0), want)
    assert (sizes, ref.predict_pull(g.nv, g.ne, sizes, vols)) == TRACES[spec]


def test_dijkstra_vs_bellman_ford_rmat():
    g = _rmat_weighted(10, 8000, 3, 16)
    want, sizes, _vols = ref.bellman_ford(g, 0)
    got = cpu_ref.sssp_weighted(g, 0)
    assert got.dtype == np.uint32
    assert np.array_equal(got, want)
    reached = want != ref.INF
    assert reached.sum() > 500 and not reached.all()
    # weights matter: the hop distances differ
    hops, _ = cpu_ref.sssp(g, 0)
    assert not np.array_equal(hops, want)


@pytest.mark.parametrize("name", sorted(ref.HAND_CASES))
def test_dijkstra_hand_cases(name):
    g, want = ref.hand_graph(name)
    assert np.array_equal(cpu_ref.sssp_weighted(g, 0), want)
    bf, sizes, _ = ref.bellman_ford(g, 0)
    assert np.array_equal(bf, want)
    assert len(sizes) <= g.nv
    assert cpu_ref.sssp_weighted_check(g, want, 0) == 0


def test_dijkstra_other_source():
    g = _rmat_weighted(10, 8000, 3, 16)
    want, _, _ = ref.bellman_ford(g, 5)
    assert np.array_equal(cpu_ref.sssp_weighted(g, 5), want)


def test_dijkstra_rejects_negative_weight():
    g = ref.graph_from_wedges(3, [(0, 1, 1), (1, 2, -1)])
    with pytest.raises(ValueError):
        cpu_ref.sssp_weighted(g, 0)


@pytest.mark.parametrize("wmax,seed", [(16, 1), (1, 1), (1000, 7)])
def test_hash_weights_twin(wmax, seed):
    g = Graph.rmat(10, 8000, seed=3)
    w = g.hash_weights(wmax, seed=seed)
    assert w is g.weight and w.dtype == np.int32 and len(w) == g.ne
    want = ref.hash_weights_np(g.src, ref.edge_dst(g), wmax, seed)
    assert np.array_equal(w, want)
    assert w.min() >= 1 and w.max() <= wmax
    if wmax == 16:
        assert len(np.unique(w)) == 16


def test_hash_weights_depend_on_endpoints_only():
    """Parallel edges share a weight; folded and plain builds agree."""
    g = Graph.rmat(8, 20000, seed=2)  # dense enough for many duplicates
    w = g.hash_weights(16)
    key = (g.src.astype(np.int64) << 32) | ref.edge_dst(g)
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    assert same.any()
    assert (w[order][1:][same] == w[order][:-1][same]).all()


def test_weighted_check_oracle():
    g = _rmat_weighted(10, 8000, 3, 16)
    lab = cpu_ref.sssp_weighted(g, 0)
    assert cpu_ref.sssp_weighted_check(g, lab, 0) == 0
    # one label too large: its in-edges (and only they) are violated
    bad = lab.copy()
    v = int(np.nonzero((lab != ref.INF) & (lab > 0))[0][0])
    bad[v] += 1
    assert cpu_ref.sssp_weighted_check(g, bad, 0) > 0
    # the source must be at distance 0
    bad = lab.copy()
    bad[0] = 1
    assert cpu_ref.sssp_weighted_check(g, bad, 0) > 0
    # an unreachable vertex offers nothing: all-INF but the source is
    # violated only on the source's out-edges
    only = np.full(g.nv, ref.INF, np.uint32)
    only[0] = 0
    n_out = int((g.src == 0).sum() - ((g.src == 0) & (ref.edge_dst(g) == 0))
                .sum())
    assert cpu_ref.sssp_weighted_check(g, only, 0) == n_out


def test_native_sssp_refuses_weighted():
    exe = os.path.join(ROOT, "bin", "sssp")
    if not os.path.exists(exe):
        pytest.skip("bin/sssp not built")
    r = subprocess.run([exe, "-synthetic", "rmat:8:1000", "-weighted"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "-weighted" in r.stderr and "not supported" in r.stderr
    assert "ELAPSED TIME" not in r.stdout
