"""k-core on the CPU: the C++ oracle cpu_ref.coreness (a sequential
Batagelj-Zaversnik bucket peel) against the two numpy definitions of
kcore_ref.py (the synchronous round-by-round peel and the H-index fixpoint),
on the hand cases with their closed forms, the hub ladder at
LUX_KCORE_HUB = 64 and both RMAT-12 graphs with their pinned values.
Coreness is an integer per vertex: every comparison is equality."""
import numpy as np
import pytest

import kcore_ref
from lux_amd import cpu_ref
from lux_amd.graph import Graph


def assert_all_agree(g):
    """oracle == sync_peel == hindex_fixpoint; returns (coreness, levels,
    rounds)."""
    got = cpu_ref.coreness(g)
    assert got.dtype == np.uint32 and got.shape == (g.nv,)
    core, levels, rounds = kcore_ref.sync_peel(g)
    assert np.array_equal(got, core)
    assert np.array_equal(kcore_ref.hindex_fixpoint(g), core)
    assert levels == np.unique(core).size
    return core, levels, rounds


@pytest.mark.parametrize("case", kcore_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    core, levels, rounds = assert_all_agree(case.g)
    if case.core is not None:
        assert np.array_equal(core, case.core)
    else:
        assert int(core.max()) == case.degeneracy
    if case.levels is not None:
        assert levels == case.levels
    if case.rounds is not None:
        assert rounds == case.rounds


def test_ladder_hub64():
    lad = kcore_ref.ladder(64)
    assert lad.degrees.max() == 129 and lad.g.nv == lad.rows.size + 131
    core, levels, _ = assert_all_agree(lad.g)
    assert np.array_equal(core, lad.core)
    assert np.array_equal(core[lad.rows], lad.degrees)
    assert levels == lad.levels


# Graph.rmat(12, 300000, seed=3, sym=...): two independent numpy definitions
# agree on every value; rounds are what kcore_ref.sync_peel gives
RMAT = {
    True: dict(m=94769, degeneracy=119, innermost=292, total=106337,
               levels=68, rounds=155),
    False: dict(m=160602, degeneracy=178, innermost=293, total=183300,
                levels=83, rounds=173),
}


@pytest.mark.parametrize("sym", [True, False], ids=["sym", "directed"])
def test_rmat12(sym):
    g = Graph.rmat(12, 300000, seed=3, sym=sym)
    want = RMAT[sym]
    ptr, _ = kcore_ref.simple_adjacency(g)
    assert int(ptr[-1]) == 2 * want["m"]
    core, levels, rounds = assert_all_agree(g)
    assert int(core.max()) == want["degeneracy"]
    assert int((core == core.max()).sum()) == want["innermost"]
    assert int(core.sum()) == want["total"]
    assert levels == want["levels"]
    assert rounds == want["rounds"]
    assert (core <= np.diff(ptr)).all()


def test_invariant_under_direction_and_duplicates():
    """Reversing every arc, or listing every arc twice with loops added,
    changes nothing."""
    g = Graph.rmat(10, 8000, seed=3)
    want = cpu_ref.coreness(g)
    src, dst = kcore_ref.tc_ref.edge_lists(g)
    assert np.array_equal(cpu_ref.coreness(Graph.from_edges(g.nv, dst, src)),
                          want)
    loops = np.arange(g.nv)
    h = Graph.from_edges(g.nv, np.concatenate([src, src, loops]),
                         np.concatenate([dst, dst, loops]))
    assert np.array_equal(cpu_ref.coreness(h), want)
