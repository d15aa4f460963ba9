"""k-truss on the CPU: the C++ oracle (cpu_ref.edge_support / cpu_ref.truss)
against the hand cases' closed forms, the dense numpy references of
truss_ref.py and values pinned from the dense peel; the invariances of the
definition; and the clustering arithmetic of tc_engine on CPU tensors.
Everything is exact integers."""
import numpy as np
import pytest
import torch

import tc_ref
import truss_ref
from lux_amd import cpu_ref
from lux_amd import tc_engine as tce
from lux_amd.graph import Graph

M = 7050  # simple edges of the RMAT below


@pytest.fixture(scope="module")
def rmat10():
    g = Graph.rmat(10, 20000, seed=3, sym=True)
    edges, support = cpu_ref.edge_support(g)
    return dict(g=g, edges=edges, support=support, truss=cpu_ref.truss(g))


# ---- oracle ----

@pytest.mark.parametrize("case", truss_ref.hand_cases(), ids=lambda c: c.name)
def test_oracle_hand_cases(case):
    edges, support = cpu_ref.edge_support(case.g)
    truss = cpu_ref.truss(case.g)
    assert edges.dtype == support.dtype == truss.dtype == np.uint32
    m = edges.shape[0]
    assert edges.shape == (m, 2) and support.shape == truss.shape == (m,)
    want_edges, want_support = truss_ref.dense_support(case.g)
    assert np.array_equal(edges, want_edges)
    assert np.array_equal(support, want_support)
    total, _ = cpu_ref.triangles(case.g)
    assert int(support.sum()) == 3 * total
    want = case.truss(want_edges[:, 0], want_edges[:, 1])
    assert np.array_equal(truss, want)
    assert np.array_equal(truss_ref.dense_truss(case.g), want)


def test_oracle_matches_dense_on_rmat(rmat10):
    g = rmat10["g"]
    want_edges, want_support = truss_ref.dense_support(g)
    assert rmat10["edges"].shape == (M, 2)
    assert np.array_equal(rmat10["edges"], want_edges)
    assert np.array_equal(rmat10["support"], want_support)
    total, _ = cpu_ref.triangles(g)
    assert int(rmat10["support"].sum()) == 3 * total
    assert np.array_equal(rmat10["truss"], truss_ref.dense_truss(g))


# k: rounds of the synchronous dense peel, surviving edges and vertices
PINNED = {4: (4, 5974, 469), 8: (7, 3889, 215), 16: (7, 1133, 59)}


@pytest.mark.parametrize("k", sorted(PINNED))
def test_oracle_against_the_dense_peel(rmat10, k):
    """alive(k) of the round-by-round dense peel == (trussness >= k) of the
    sequential oracle: two schedules, one answer."""
    alive, rounds = truss_ref.dense_peel(rmat10["g"], k)
    assert np.array_equal(alive, rmat10["truss"] >= k)
    assert (rounds, int(alive.sum()),
            truss_ref.vertices_of(rmat10["edges"], alive)) == PINNED[k]


def test_oracle_pinned_decomposition(rmat10):
    truss = rmat10["truss"]
    assert int(truss.max()) == 19
    assert int((truss == 19).sum()) == 972 and int((truss == 2).sum()) == 491
    # an edge of trussness k has at least k - 2 triangles to begin with
    assert (rmat10["support"].astype(np.int64) >= truss.astype(np.int64)
            - 2).all()
    alive, rounds = truss_ref.dense_peel(rmat10["g"], 2)
    assert alive.all() and rounds == 0
    alive, _ = truss_ref.dense_peel(rmat10["g"], 20)
    assert not alive.any()


def test_invariance(rmat10):
    """Relabelling, parallel edges, self-loops and edge direction."""
    g = rmat10["g"]
    src, dst = tc_ref.edge_lists(g)

    def run(s, d):
        h = Graph.from_edges(g.nv, np.asarray(s), np.asarray(d))
        e, sup = cpu_ref.edge_support(h)
        return e, sup, cpu_ref.truss(h)

    for s, d in ((np.concatenate([src, src]), np.concatenate([dst, dst])),
                 (np.concatenate([src, np.arange(g.nv)]),
                  np.concatenate([dst, np.arange(g.nv)])),
                 (src[src < dst], dst[src < dst])):
        e, sup, t = run(s, d)
        assert np.array_equal(e, rmat10["edges"])
        assert np.array_equal(sup, rmat10["support"])
        assert np.array_equal(t, rmat10["truss"])

    p = np.random.default_rng(5).permutation(g.nv)  # v -> p[v]
    e, sup, t = run(p[src], p[dst])
    a, b = p[rmat10["edges"][:, 0]], p[rmat10["edges"][:, 1]]
    key = np.minimum(a, b).astype(np.int64) << 32 | np.maximum(a, b)
    order = np.argsort(key)
    assert np.array_equal(e[:, 0].astype(np.int64) << 32 | e[:, 1],
                          key[order])
    assert np.array_equal(sup, rmat10["support"][order])
    assert np.array_equal(t, rmat10["truss"][order])


def test_oracle_on_the_gpu_test_graphs():
    """The RMAT-12 pair the GPU tests of triangle counting use; pinned from
    the dense peel (symmetric) and from two runs of the oracle (directed)."""
    g = Graph.rmat(12, 300000, seed=3, sym=True)
    edges, support = cpu_ref.edge_support(g)
    truss = cpu_ref.truss(g)
    assert edges.shape[0] == 94769
    assert int(support.astype(np.int64).sum()) == 3 * 1882531
    assert int(truss.max()) == 70
    assert int((truss == 70).sum()) == 3034 and int((truss == 2).sum()) == 1284
    for k, (ne, nvert) in {4: (91701, 2825), 8: (82902, 1897),
                           16: (66454, 1155)}.items():
        alive = truss >= k
        assert (int(alive.sum()), truss_ref.vertices_of(edges, alive)) == \
            (ne, nvert)
    g = Graph.rmat(12, 300000, seed=3)  # duplicates and self-loops
    truss = cpu_ref.truss(g)
    assert truss.shape[0] == 160602
    assert int(truss.max()) == 118 and int((truss == 118).sum()) == 30929


# ---- clustering ----

def test_clustering_arithmetic(rmat10):
    pv = torch.tensor([0, 0, 1, 3, 6, 2, 0], dtype=torch.int64)
    deg = torch.tensor([0, 1, 2, 3, 4, 5, 7], dtype=torch.int64)
    got = tce.clustering(pv, deg)
    assert got.dtype == torch.float64
    assert got.tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 0.2, 0.0]
    g = rmat10["g"]
    _, pv = cpu_ref.triangles(g)
    deg = tc_ref.simple_degrees(g)
    got = tce.clustering(torch.from_numpy(pv.astype(np.int64)),
                         torch.from_numpy(deg.astype(np.int64))).numpy()
    pairs = deg * (deg - 1) // 2
    want = np.where(pairs > 0, pv / np.maximum(pairs, 1), 0.0)
    assert np.array_equal(got, want)
    assert got.max() <= 1.0 and got.max() > 0.0
