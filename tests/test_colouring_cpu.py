"""Greedy colouring on the CPU: the C++ oracle cpu_ref.greedy_colouring (one
sequential pass in priority order with a stamp array) against the two numpy
definitions of colouring_ref.py (the sequential greedy pass and the
synchronous Jones-Plassmann schedule), in the three priority orders, on the
hand cases with their closed forms in id order, the hub ladder at
LUX_GCOL_HUB = 64 and both RMAT-12 graphs with their pinned values. A colour
is an integer per vertex: every comparison is equality."""
import numpy as np
import pytest

import colouring_ref as cr
from lux_amd import cpu_ref
from lux_amd.graph import Graph

ORDER = pytest.mark.parametrize("order", cr.ORDERS)


def assert_all_agree(g, order, seed=1):
    """oracle == greedy == sync_jp, and the verifier passes; returns
    (colour, rounds, sizes)."""
    got = cpu_ref.greedy_colouring(g, order, seed)
    assert got.dtype == np.int32 and got.shape == (g.nv,)
    assert np.array_equal(got, cr.greedy(g, order, seed))
    colour, rounds, sizes = cr.sync_jp(g, order, seed)
    assert np.array_equal(got, colour)
    assert sum(sizes) == g.nv and len(sizes) == rounds
    assert cr.verify(g, got, order, seed) == 0
    return colour, rounds, sizes


@ORDER
@pytest.mark.parametrize("case", cr.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, order):
    colour, rounds, _ = assert_all_agree(case.g, order)
    if order != "id":
        return
    if case.colour is not None:
        assert np.array_equal(colour, case.colour)
    assert rounds == case.rounds
    assert int(colour.max()) + 1 == case.ncolours


def test_crown_separates_greedy_from_proper():
    """The 2-colouring of the crown graph is proper but is not the greedy
    colouring in id order: the verifier tells them apart."""
    case = {c.name: c for c in cr.hand_cases()}["crown70"]
    two = np.arange(case.g.nv) & 1
    assert cr.verify(case.g, two, "id") > 0
    assert cr.verify(case.g, case.colour, "id") == 0


@ORDER
@pytest.mark.parametrize("side", ["below", "above"])
def test_ladder_hub64(side, order):
    lad = cr.ladder(64, side)
    assert lad.degrees.max() == 129
    assert lad.g.nv == lad.rows.size + 131
    assert_all_agree(lad.g, order)
    npred, nsucc = cr.pred_succ_counts(lad.g, "id")
    want, zero = (nsucc, npred) if side == "below" else (npred, nsucc)
    assert np.array_equal(want[lad.rows], lad.degrees)
    assert not zero[lad.rows].any()


def test_hash_priority_follows_the_seed():
    g = Graph.rmat(10, 8000, seed=3)
    a = cpu_ref.greedy_colouring(g, "hash", 1)
    b = cpu_ref.greedy_colouring(g, "hash", 2)
    assert not np.array_equal(a, b)
    assert np.array_equal(b, cr.greedy(g, "hash", 2))
    assert cr.verify(g, b, "hash", 2) == 0
    # lux::splitmix64(0), the first output of the generator seeded with 0
    assert int(cr.splitmix64(np.zeros(1, np.uint64))[0]) == \
        0xE220A8397B1DCDAF


@ORDER
def test_engine_rank_is_the_reference_priority(order):
    """The engine's torch rank (wrap-around i64 splitmix64, stable sorts)
    on the host equals colouring_ref.priority."""
    import torch

    from lux_amd.colouring_engine import hash_keys, priority_rank
    g = Graph.rmat(10, 8000, seed=3)
    ptr, _ = cr.kcore_ref.simple_adjacency(g)
    deg = torch.from_numpy(np.diff(ptr))
    for seed in (1, 0xFEDCBA9876543210):
        got = priority_rank(deg, order, seed).numpy()
        assert np.array_equal(got, cr.priority(g, order, seed))
        ids = np.arange(g.nv, dtype=np.uint64)
        want = cr.splitmix64(ids ^ np.uint64(seed)) >> np.uint64(1)
        assert np.array_equal(
            hash_keys(g.nv, seed, "cpu").numpy().astype(np.uint64), want)


def test_unknown_order_raises():
    with pytest.raises(ValueError, match="order"):
        cpu_ref.greedy_colouring(Graph.rmat(8, 1000, seed=3), "random")


# Graph.rmat(12, 40000, seed=7, sym=...): the C++ oracle and both numpy
# definitions agree on every value; rounds are what sync_jp gives
RMAT = {
    False: dict(degree=dict(colours=31, rounds=109, mis=2521, total=5882),
                id=dict(colours=32, rounds=115, mis=2583, total=6093),
                hash=dict(colours=39, rounds=123, mis=2777, total=5512)),
    True: dict(degree=dict(colours=18, rounds=75, mis=2786, total=3686),
               id=dict(colours=22, rounds=72, mis=2872, total=3695),
               hash=dict(colours=27, rounds=80, mis=3005, total=3398)),
}


@ORDER
@pytest.mark.parametrize("sym", [False, True], ids=["directed", "sym"])
def test_rmat12(sym, order):
    g = Graph.rmat(12, 40000, seed=7, sym=sym)
    want = RMAT[sym][order]
    colour, rounds, _ = assert_all_agree(g, order)
    assert int(colour.max()) + 1 == want["colours"]
    assert rounds == want["rounds"]
    assert int((colour == 0).sum()) == want["mis"]
    assert int(colour.sum()) == want["total"]
    npred, _ = cr.pred_succ_counts(g, order)
    assert (colour <= npred).all()


@ORDER
def test_invariant_under_direction_and_duplicates(order):
    """Reversing every arc, or listing every arc twice with loops added,
    changes nothing."""
    g = Graph.rmat(10, 8000, seed=3)
    want = cpu_ref.greedy_colouring(g, order)
    src, dst = cr.tc_ref.edge_lists(g)
    rev = Graph.from_edges(g.nv, dst, src)
    assert np.array_equal(cpu_ref.greedy_colouring(rev, order), want)
    loops = np.arange(g.nv)
    h = Graph.from_edges(g.nv, np.concatenate([src, src, loops]),
                         np.concatenate([dst, dst, loops]))
    assert np.array_equal(cpu_ref.greedy_colouring(h, order), want)
