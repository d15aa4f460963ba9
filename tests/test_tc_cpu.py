"""Triangle counting on the CPU: the C++ oracle (cpu_ref.triangles) against
the dense-matrix count of tc_ref.py and the hand cases' closed forms, the
torch orientation (tc_engine.orient / build_items) on CPU tensors, and the
invariances of the definition (relabelling, parallel edges, self-loops,
edge direction). Everything is exact integers."""
import numpy as np
import pytest
import torch

import tc_ref
from lux_amd import cpu_ref
from lux_amd import tc_engine as tce
from lux_amd.graph import Graph


def cpu_tensors(g):
    row_ptr = np.concatenate([[0], g.col_end.astype(np.int64)])
    return (torch.from_numpy(row_ptr),
            torch.from_numpy(np.ascontiguousarray(g.src).view(np.int32)))


def simple_edge_set(g):
    src, dst = tc_ref.edge_lists(g)
    keep = src != dst
    return set(zip(np.minimum(src, dst)[keep].tolist(),
                   np.maximum(src, dst)[keep].tolist()))


@pytest.fixture(scope="module")
def rmat10():
    return Graph.rmat(10, 16000, seed=3, sym=True)


# ---- oracle vs dense ----

@pytest.mark.parametrize("case", tc_ref.hand_cases(), ids=lambda c: c.name)
def test_oracle_hand_cases(case):
    total, pv = cpu_ref.triangles(case.g)
    assert pv.dtype == np.uint64 and pv.shape == (case.g.nv,)
    assert total == case.want["total"]
    assert np.array_equal(pv, case.want["per_vertex"])
    dt, dpv, _ = tc_ref.dense_count(case.g)
    assert total == dt and np.array_equal(pv, dpv)
    assert int(pv.sum()) == 3 * total


def test_oracle_matches_dense_on_rmat(rmat10):
    total, pv = cpu_ref.triangles(rmat10)
    dt, dpv, edges = tc_ref.dense_count(rmat10)
    assert total == dt == 22992
    assert edges == 5888
    assert np.array_equal(pv, dpv)
    assert int(pv.sum()) == 3 * total


def test_ladder_row_counts_are_exact():
    lad = tc_ref.ladder(64, tce.TC_T1, tce.TC_CHUNK)
    total, pv = cpu_ref.triangles(lad.g)
    assert np.array_equal(pv[lad.rows], lad.row_counts)
    assert lad.row_counts.max() > 0
    dt, dpv, _ = tc_ref.dense_count(lad.g)
    assert total == dt and np.array_equal(pv, dpv)


# ---- orient on CPU tensors ----

def _check_orientation(g, order, chunk=None):
    row_ptr, col = cpu_tensors(g)
    o = tce.orient(row_ptr, col, g.nv, order, chunk=chunk)
    nv = g.nv
    optr, oadj = o.optr.numpy(), o.oadj.numpy().view(np.uint32)
    perm, rank, deg = o.perm.numpy(), o.rank.numpy(), o.deg.numpy()
    edges = simple_edge_set(g)
    assert o.m == len(edges) == oadj.size == int(optr[nv])
    assert optr[0] == 0 and (np.diff(optr) >= 0).all()
    assert np.array_equal(np.sort(perm), np.arange(nv))
    assert np.array_equal(rank[perm], np.arange(nv))
    assert np.array_equal(deg, tc_ref.simple_degrees(g))
    row = np.repeat(np.arange(nv), np.diff(optr))
    assert (oadj.astype(np.int64) > row).all()  # every entry > its row id
    inner = row[1:] == row[:-1]
    assert (oadj[1:][inner] > oadj[:-1][inner]).all()  # strictly ascending
    if order == "degree":
        assert (np.diff(deg[perm]) >= 0).all()
        ties = np.diff(deg[perm]) == 0
        assert (np.diff(perm)[ties] > 0).all()  # ties by ascending id
    else:
        assert np.array_equal(perm, np.arange(nv))
    a, b = perm[row], perm[oadj.astype(np.int64)]
    back = set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    assert back == edges
    return o


@pytest.mark.parametrize("order", tce.ORDERS)
def test_orient_rmat(rmat10, order):
    o = _check_orientation(rmat10, order)
    assert o.m == 5888


@pytest.mark.parametrize("order", tce.ORDERS)
@pytest.mark.parametrize("case", tc_ref.hand_cases(), ids=lambda c: c.name)
def test_orient_hand_cases(case, order):
    _check_orientation(case.g, order)


@pytest.mark.parametrize("order", tce.ORDERS)
def test_orient_in_small_sort_chunks(rmat10, order):
    """chunk=1000 takes the multi-run merge; the result is the same."""
    want = _check_orientation(rmat10, order)
    for chunk in (1000, 37):
        got = _check_orientation(rmat10, order, chunk=chunk)
        assert torch.equal(got.optr, want.optr)
        assert torch.equal(got.oadj, want.oadj)
        assert torch.equal(got.perm, want.perm)


def test_orient_rejects_unknown_order(rmat10):
    row_ptr, col = cpu_tensors(rmat10)
    with pytest.raises(ValueError, match="order"):
        tce.orient(row_ptr, col, rmat10.nv, "random")


def test_degree_order_bounds_the_out_degree(rmat10):
    row_ptr, col = cpu_tensors(rmat10)
    by_deg = tce.orient(row_ptr, col, rmat10.nv, "degree")
    by_id = tce.orient(row_ptr, col, rmat10.nv, "id")
    dmax = int((by_deg.optr[1:] - by_deg.optr[:-1]).max())
    assert dmax * dmax <= 2 * by_deg.m  # d+ <= sqrt(2m)
    assert dmax < int((by_id.optr[1:] - by_id.optr[:-1]).max())


@pytest.mark.parametrize("cap", [64, 4096])
def test_items_cover_every_arc_once(cap):
    lad = tc_ref.ladder(64, tce.TC_T1, tce.TC_CHUNK)
    row_ptr, col = cpu_tensors(lad.g)
    o = tce.orient(row_ptr, col, lad.g.nv, "id")
    d = np.diff(o.optr.numpy())
    assert np.array_equal(d[lad.rows], lad.degrees)
    assert np.array_equal(d[lad.specials], tc_ref.POOL_DEGREES)
    items = [t.numpy().view(np.uint32) for t in tce.build_items(o.optr, cap)]
    assert len(items) == len(tce.ROLES)
    seen = np.zeros(o.m, np.int64)
    for role, it in enumerate(items):
        assert it.shape[1] == 3
        for u, first, last in it.tolist():
            want = 0 if d[u] < tce.TC_T1 else (1 if d[u] <= cap else 2)
            assert role == want
            assert first < last <= d[u] and last - first <= tce.TC_CHUNK
            assert first % tce.TC_CHUNK == 0
            seen[o.optr[u] + first:o.optr[u] + last] += 1
    assert (seen == 1).all()
    n_items = sum(it.shape[0] for it in items)
    assert n_items == int(np.ceil(d / tce.TC_CHUNK).sum())


# ---- invariance ----

def _from_lists(nv, src, dst):
    return Graph.from_edges(nv, np.asarray(src), np.asarray(dst))


def test_invariance(rmat10):
    g = rmat10
    total, pv = cpu_ref.triangles(g)
    src, dst = tc_ref.edge_lists(g)
    rng = np.random.default_rng(5)

    p = rng.permutation(g.nv)  # v -> p[v]
    t, q = cpu_ref.triangles(_from_lists(g.nv, p[src], p[dst]))
    assert t == total and np.array_equal(q[p], pv)

    t, q = cpu_ref.triangles(_from_lists(
        g.nv, np.concatenate([src, src]), np.concatenate([dst, dst])))
    assert t == total and np.array_equal(q, pv)

    loops = np.arange(g.nv)
    t, q = cpu_ref.triangles(_from_lists(
        g.nv, np.concatenate([src, loops]), np.concatenate([dst, loops])))
    assert t == total and np.array_equal(q, pv)

    one_way = src < dst  # the sym graph holds both arcs of every pair
    t, q = cpu_ref.triangles(_from_lists(g.nv, src[one_way], dst[one_way]))
    assert t == total and np.array_equal(q, pv)
