"""CPU-only checks of tests/degree_ladder.py: the prescribed-degree graphs
are what they claim to be, the int64 / f64 references agree with brute
force, and the bounds the GPU tests assert can tell a wrong kernel from a
right one (an all-zero output, a dropped edge) on reference data alone."""
import numpy as np
import pytest

import degree_ladder as dl


@pytest.fixture(scope="module")
def bip():
    return dl.bipartite_ladder()


@pytest.fixture(scope="module")
def plain():
    return dl.plain_ladder(marker="last")


def _row(g, v):
    b = 0 if v == 0 else int(g.col_end[v - 1])
    return b, int(g.col_end[v])


def test_ladder_covers_every_bin_edge():
    lad = set(dl.LADDER)
    for t in (dl.T1, dl.T2, dl.CHUNK_EDGES):
        assert t - 1 in lad and t in lad and t + 1 in lad
    assert {0, 1, 4, 5} <= lad                      # 4-deep pipeline tail
    assert {63, 64, 65, 127, 128, 129} <= lad       # CF/ALS tile 32 and 64
    assert {2 * dl.CHUNK_EDGES, 2 * dl.CHUNK_EDGES + 1,
            3 * dl.CHUNK_EDGES + 1} <= lad          # 2, 3 and 4 chunks


def test_bipartite_ladder_structure(bip):
    g, nu = bip.g, bip.nu
    n = len(dl.LADDER)
    assert list(bip.degs[:n]) == dl.LADDER
    assert list(bip.degs[nu:nu + n]) == dl.LADDER
    assert (bip.degs == 0).sum() > 2
    nue = int(g.col_end[nu - 1])
    assert g.src[:nue].min() >= nu and g.src[nue:].max() < nu
    assert g.weight.min() == 1 and g.weight.max() == 5
    # hub Grams can reach full rank for K <= 64
    b, e = _row(g, n - 1)
    assert len(np.unique(g.src[b:e])) >= 64
    assert g.ne < 400000


@pytest.mark.parametrize("where", ["first", "last", "chunk_last",
                                   "chunk_first"])
def test_plain_ladder_structure(where):
    lad = dl.plain_ladder(marker=where)
    g = lad.g
    w = 1 << dl.PLAIN_SHIFT
    assert g.nv == dl.PLAIN_NV and list(lad.degs[:len(dl.LADDER)]) \
        == dl.LADDER
    assert g.src.min() >= lad.pool0          # pool rows have no in-edges
    assert lad.degs[lad.pool0:].sum() == 0
    for v in lad.ladder_rows:
        b, e = _row(g, v)
        if e == b:
            continue
        blk = lad.row_block[v]
        s = g.src[b:e].astype(np.int64)
        lo = lad.pool0 + blk * w
        assert s.min() >= lo and s.max() < lo + w   # one src block
        hit = np.nonzero(s == lad.markers[blk])[0]
        assert list(hit) == [dl.marker_position(e - b, where)]
    # filler rows never read a marker
    b = int(g.col_end[len(dl.LADDER) - 1])
    assert not np.isin(g.src[b:], lad.markers).any()
    # every pool window serves thread-, wave- and chunk-bin ladder rows
    for blk in range(dl.PLAIN_POOL_BLOCKS):
        d = lad.degs[lad.ladder_rows][lad.row_block[lad.ladder_rows] == blk]
        assert ((d > 0) & (d < dl.T1)).any()
        assert ((d >= dl.T1) & (d < dl.T2)).any()
        assert (d > dl.CHUNK_EDGES).any()


def test_int_factors_distinct():
    for K in (20, 64, 256):
        F = dl.int_factors(256, K)
        assert F.min() == 0 and F.max() == 6
        assert len(np.unique(F, axis=0)) == 256      # per vertex
        assert len(np.unique(F.T, axis=0)) == K      # per dimension
    for K in (1, 3, 4):  # few dims: still every value, many distinct rows
        F = dl.int_factors(256, K)
        assert len(np.unique(F)) == 7
        assert len(np.unique(F, axis=0)) >= min(7 ** K, 128)


def test_marker_positions():
    assert dl.marker_position(8193, "chunk_last") == 8191
    assert dl.marker_position(8193, "chunk_first") == 8192
    assert dl.marker_position(8192, "chunk_first") == 0
    assert dl.marker_position(24577, "chunk_first") == 24576
    assert dl.marker_position(5, "chunk_last") == 4


def test_pull_refs_match_brute_force(plain):
    g = plain.g
    rng = np.random.default_rng(1)
    ints = rng.integers(0, 7, g.nv)
    lab = rng.integers(0, 1000, g.nv).astype(np.uint32)
    lab[rng.random(g.nv) < 0.4] = dl.INF
    s_ref = dl.pull_sum_ref(plain, ints)
    mn_ref = dl.pull_min_ref(plain, lab)
    mx_ref = dl.pull_max_ref(plain, lab)
    for v in list(range(12)) + [28, 29, 42, 100, 255, 300]:
        b, e = _row(g, v)
        src = g.src[b:e]
        assert s_ref[v] == int(ints[src].sum())
        own = int(lab[v])
        fin = [int(x) + 1 for x in lab[src] if x != dl.INF]
        want = own if own != dl.INF else min(fin, default=dl.INF)
        assert mn_ref[v] == want
        assert mx_ref[v] == max([own] + [int(x) for x in lab[src]])
    assert s_ref.max() < 2 ** 24  # exact in fp32 in any order


def test_pull_min_inf_does_not_wrap(plain):
    lab = np.full(plain.g.nv, dl.INF, np.uint32)
    assert (dl.pull_min_ref(plain, lab) == dl.INF).all()


def test_sgd_exact_reference_and_selfchecks(bip):
    """Exact regime on reference data only: int64 brute force agrees, every
    partial sum is fp32-exact, and the 1e-6 bound rejects an all-zero
    output and a single dropped weight-1 edge at the largest degree."""
    g, nu, K = bip.g, bip.nu, 20
    F = dl.int_factors(g.nv, K)
    F[:nu] = 0  # users are the dst side
    acc, scale = dl.sgd_gradient_ref(g, F)
    assert np.array_equal(acc[:nu], scale[:nu])  # err = w > 0, s >= 0
    assert acc.max() < 2 ** 24 and np.array_equal(acc, np.rint(acc))
    for v in (1, 5, 11, 28, 42):
        b, e = _row(g, v)
        want = (g.weight[b:e, None].astype(np.int64)
                * F[g.src[b:e]].astype(np.int64)).sum(0)
        assert np.array_equal(acc[v].astype(np.int64), want)
    nonempty = np.nonzero(bip.degs[:nu] > 0)[0]
    assert len(dl.sgd_exact_bad_rows(acc[:nu], acc[:nu])) == 0
    assert np.array_equal(
        dl.sgd_exact_bad_rows(np.zeros_like(acc[:nu]), acc[:nu]), nonempty)
    # drop the last edge of the degree-24577 row, with its weight set to 1
    v = len(dl.LADDER) - 1
    b, e = _row(g, v)
    assert e - b == 24577
    less = acc[:nu].copy()
    less[v] -= F[g.src[e - 1]]
    assert v in dl.sgd_exact_bad_rows(less, acc[:nu])
    assert (F[g.src[e - 1]] / acc[v].max()).max() >= 8e-6


@pytest.mark.parametrize("K", [1, 64])
def test_sgd_random_bound_selfchecks(bip, K):
    """Random regime on reference data only: an all-zero (no-op) output
    breaks the 1e-4*A bound on every non-empty row; a gather from the
    neighbouring source does too; sequential fp32 accumulation of the
    largest row stays far inside it."""
    g = bip.g
    old = dl.rand_factors(g.nv, K, seed=3)
    acc, scale = dl.sgd_gradient_ref(g, old)
    nonempty = np.nonzero(bip.degs > 0)[0]
    assert np.array_equal(
        dl.sgd_rand_bad_rows(np.zeros_like(acc), acc, scale), nonempty)
    hubs = np.nonzero(bip.degs >= dl.T1)[0]
    # from the wave bin up, the no-op margin is thousands of bounds wide
    assert (np.abs(acc[hubs]) / scale[hubs]).max(1).min() > 0.3
    shifted = np.roll(old, 1, axis=0)  # every gather off by one vertex
    shifted[0], shifted[bip.nu] = old[bip.nu - 1], old[-1]  # stay on-side
    wrong, _ = dl.sgd_gradient_ref(g, shifted)
    assert np.isin(hubs, dl.sgd_rand_bad_rows(wrong, acc, scale)).all()
    v = len(dl.LADDER) - 1
    b, e = _row(g, v)
    S = old[g.src[b:e]]
    err = (g.weight[b:e].astype(np.float32)
           - (S * old[v]).sum(1, dtype=np.float32))
    seq = np.cumsum(err[:, None] * S, axis=0, dtype=np.float32)[-1]
    assert (np.abs(seq - acc[v]) / scale[v]).max() < 2e-5


def test_hub_gram_reference(bip):
    g, K = bip.g, 20
    F = dl.int_factors(g.nv, K)
    v = bip.nu + len(dl.LADDER) - 1  # item hub, degree 24577
    G, rhs = dl.hub_gram_ref(g, v, F)
    b, e = _row(g, v)
    S = F[g.src[b:e]].astype(np.int64)
    assert np.array_equal(G[:K, :K], np.triu(S.T @ S))
    assert np.array_equal(rhs[:K], S.T @ g.weight[b:e].astype(np.int64))
    assert not G[K:].any() and not G[:, K:].any() and not rhs[K:].any()
    assert G.max() < 2 ** 24 and rhs.max() < 2 ** 24
    assert (np.tril(G, -1) == 0).all()
