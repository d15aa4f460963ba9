"""SCC on the CPU: the C++ oracle cpu_ref.scc (an iterative Tarjan) against
closed forms and against the numpy schedule scc_ref.sync_schedule (trim,
forward-backward, colouring), on the hand cases, the star ladder at
LUX_SCC_HUB = 64, the RMAT graphs with their pinned values, the planted
graphs and the two giants. Labels are integers: every comparison is
equality."""
import numpy as np
import pytest

import scc_ref
from lux_amd import cpu_ref
from lux_amd.graph import Graph


def assert_normalised(label):
    """label[v] >= v, label[label[v]] == label[v]; a class's label is its
    largest member."""
    lab = label.astype(np.int64)
    assert (lab >= np.arange(lab.size)).all()
    assert np.array_equal(lab[lab], lab)
    top = np.zeros(lab.size, np.int64)
    np.maximum.at(top, lab, np.arange(lab.size))
    assert np.array_equal(top[lab], lab)


def assert_all_agree(g):
    """oracle == sync_schedule; returns (label i64, stats)."""
    got = cpu_ref.scc(g)
    assert got.dtype == np.uint32 and got.shape == (g.nv,)
    label, stats = scc_ref.sync_schedule(g)
    assert np.array_equal(got, label)
    assert_normalised(got)
    return label, stats


def assert_stats(stats, want):
    for key, val in want.items():
        assert stats[key] == val, (key, stats[key], val)


@pytest.mark.parametrize("case", scc_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    label, stats = assert_all_agree(case.g)
    assert np.array_equal(label, case.label)
    assert_stats(stats, case.stats)


@pytest.mark.parametrize("leaves", scc_ref.ladder_leaves(64))
def test_star_ladder_hub64(leaves):
    case = scc_ref.ladder_case(leaves)
    label, stats = assert_all_agree(case.g)
    assert np.array_equal(label, case.label)
    assert_stats(stats, case.stats)


# measured with scc_ref.sync_schedule; they agree with the oracle
RMAT = {
    "rmat12": dict(args=(12, 300000), sym=False, sccs=583, largest=3514,
                   stats=dict(trim_rounds=2, trimmed=582, pivot=0,
                              reach_rounds=8, colour_rounds=0)),
    "rmat14": dict(args=(14, 40000), sym=False, sccs=12076, largest=4309,
                   stats=dict(trim_rounds=3, trimmed=12075, pivot=0,
                              reach_rounds=13, colour_rounds=0)),
    "rmat12_sym": dict(args=(12, 300000), sym=True, sccs=420, largest=3677,
                       stats=dict(trim_rounds=1, trimmed=419)),
}


@pytest.mark.parametrize("name", sorted(RMAT))
def test_rmat(name):
    pin = RMAT[name]
    g = Graph.rmat(*pin["args"], seed=3, sym=pin["sym"])
    label, stats = assert_all_agree(g)
    assert np.unique(label).size == pin["sccs"]
    assert int(np.bincount(label).max()) == pin["largest"]
    assert_stats(stats, pin["stats"])


def test_symmetric_graph_gives_the_weak_components():
    """On a symmetric file the SCCs are the weak components, relabelled by
    their maximum id: the partitions are equal, the label values are not
    compared."""
    g = Graph.rmat(12, 300000, seed=3, sym=True)
    cc, _ = cpu_ref.cc(g)
    assert scc_ref.same_partition(cpu_ref.scc(g), cc)
    assert not scc_ref.same_partition(
        cpu_ref.scc(Graph.rmat(12, 300000, seed=3)), cc)


PLANTED = [(300, 64, 3000, 7), (400, 200, 40000, 5)]


@pytest.mark.parametrize("args", PLANTED, ids=lambda a: "-".join(map(str, a)))
def test_planted(args):
    g, want = scc_ref.planted(*args)
    label, stats = assert_all_agree(g)
    assert np.array_equal(label, want)
    assert stats["colour_rounds"] >= 2


def test_two_giants():
    g = scc_ref.two_giants()
    label, stats = assert_all_agree(g)
    n = g.nv // 2
    # the same decomposition twice, the second copy shifted by n
    assert np.array_equal(label[n:], label[:n] + n)
    assert stats["fwbw"] > 1 and stats["colour_rounds"] >= 1


def test_invariant_under_duplicates_and_loops():
    g = Graph.rmat(10, 8000, seed=3)
    want = cpu_ref.scc(g)
    src, dst = scc_ref.tc_ref.edge_lists(g)
    loops = np.arange(g.nv)
    h = Graph.from_edges(g.nv, np.concatenate([src, src, loops]),
                         np.concatenate([dst, dst, loops]))
    assert np.array_equal(cpu_ref.scc(h), want)
    # reversing every edge keeps the components
    r = Graph.from_edges(g.nv, dst, src)
    assert np.array_equal(cpu_ref.scc(r), want)
