"""The minimum-spanning-forest oracle cpu_ref.msf (msf_cpu in engines.cpp,
Kruskal) against the numpy references of msf_ref: the synchronous Boruvka
schedule and, up to 64 vertices, Prim on the dense matrix. The order (w, e)
is strict, so the forest is unique and every comparison is equality, ties
included. Also recomputes the pinned values the GPU tests rely on."""
import numpy as np
import pytest

import msf_ref
from lux_amd import cpu_ref
from lux_amd.graph import Graph


def assert_agree(g, want=None):
    """Oracle == schedule (== Prim up to 64 vertices); returns both."""
    lo, hi, w, mask, total, labels = cpu_ref.msf(g)
    ref = msf_ref.sync_boruvka(g)
    assert lo.dtype == hi.dtype == labels.dtype == np.uint32
    assert w.dtype == np.int32 and mask.dtype == np.bool_
    assert isinstance(total, int)
    assert np.array_equal(lo, ref.lo) and np.array_equal(hi, ref.hi)
    assert np.array_equal(w, ref.w)
    assert np.array_equal(mask, ref.in_forest)
    assert total == ref.total == int(w[mask].astype(np.int64).sum())
    assert np.array_equal(labels, ref.labels)
    comps = int(np.unique(labels).size)
    assert int(mask.sum()) == ref.nf == g.nv - comps
    assert ref.scans == (ref.rounds + 1 if lo.size else 0)
    assert ref.rounds <= max(int(np.ceil(np.log2(max(g.nv, 1)))), 0)
    # without the dead-row rule: the same forest, 2m entries per scan
    plain = msf_ref.sync_boruvka(g, dead=False)
    assert np.array_equal(plain.in_forest, mask)
    assert [r[:2] for r in plain.per_round] == \
        [r[:2] for r in ref.per_round]
    assert all(r[2] == 2 * lo.size for r in plain.per_round)
    assert all(a[2] <= 2 * lo.size for a in ref.per_round)
    if g.nv <= 64:
        pmask, ptotal = msf_ref.dense_prim(g)
        assert np.array_equal(pmask, mask) and ptotal == total
    for key, val in (want or {}).items():
        got = dict(total=total, nf=ref.nf, components=comps,
                   rounds=ref.rounds, m=int(lo.size),
                   per_round=ref.per_round,
                   forest=np.nonzero(mask)[0].tolist(),
                   max_degree=int(np.bincount(
                       np.concatenate([lo, hi]), minlength=1).max())
                   if lo.size else 0)[key]
        assert got == val, (key, got, val)
    return (lo, hi, w, mask, total, labels), ref


def assert_scipy_total(lo, hi, w, nv, total):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import minimum_spanning_tree
    assert w.size == 0 or w.min() >= 1  # scipy reads 0 as "no edge"
    A = sp.csr_matrix((w.astype(np.float64), (lo, hi)), shape=(nv, nv))
    got = minimum_spanning_tree(A).sum()
    assert got < 2.0 ** 53 and int(got) == total


@pytest.mark.parametrize("case", msf_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    (lo, hi, w, _, total, _), _ = assert_agree(case.g, case.want)
    if w.size and w.min() >= 1:
        assert_scipy_total(lo, hi, w, case.g.nv, total)


@pytest.mark.parametrize("case", msf_ref.ladder_cases(), ids=lambda c: c.name)
def test_hub_ladder(case):
    (lo, hi, w, _, total, _), _ = assert_agree(case.g, case.want)
    assert_scipy_total(lo, hi, w, case.g.nv, total)


@pytest.mark.parametrize("seed", range(12))
def test_random_small(seed):
    rng = np.random.default_rng(100 + seed)
    nv = int(rng.integers(2, 65))
    ne = int(rng.integers(0, 6 * nv))
    wlo, whi = [(1, 1), (1, 3), (-4, 4), (msf_ref.I32_MIN, msf_ref.I32_MAX),
                (1, 1000), (0, 1)][seed % 6]
    g = msf_ref.random_graph(nv, ne, wlo, whi, seed)
    (lo, hi, w, _, total, _), _ = assert_agree(g)
    if wlo >= 1:
        assert_scipy_total(lo, hi, w, nv, total)


@pytest.mark.parametrize("name", sorted(msf_ref.RMAT))
def test_rmat_pinned(name):
    pin = msf_ref.RMAT[name]
    g = msf_ref.rmat_graph(name)
    want = {k: pin[k] for k in ("m", "nf", "total", "components",
                                "max_degree", "per_round")}
    (lo, hi, w, _, total, labels), ref = assert_agree(g, want)
    deg = np.bincount(np.concatenate([lo, hi]).astype(np.int64),
                      minlength=g.nv)
    assert int((deg == 0).sum()) == pin["isolated"]
    assert ref.rounds == len(pin["per_round"])
    assert_scipy_total(lo, hi, w, g.nv, total)
    if pin["sym"]:
        cc, _ = cpu_ref.cc(g)
        assert np.array_equal(labels, cc)


def test_weights_are_required():
    g = Graph.rmat(8, 1000, seed=3)
    with pytest.raises(ValueError, match="weight"):
        cpu_ref.msf(g)


def test_direction_and_order_of_the_arcs_do_not_matter():
    g = msf_ref.random_graph(60, 300, 1, 5, 7)
    src, dst = msf_ref.tc_ref.edge_lists(g)
    rng = np.random.default_rng(8)
    flip = rng.random(src.size) < 0.5
    perm = rng.permutation(src.size)
    h = Graph.from_edges(
        g.nv, np.where(flip, dst, src)[perm].astype(np.uint32),
        np.where(flip, src, dst)[perm].astype(np.uint32),
        np.asarray(g.weight)[perm])
    a, b = cpu_ref.msf(g), cpu_ref.msf(h)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
