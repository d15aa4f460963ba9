"""The bucketed-schedule reference (tests/bucketed_sssp_ref.py) on its own:
its labels against the Dijkstra oracle, its large-delta limit against the
synchronous Bellman-Ford, and the properties of the inputs the GPU tests
rely on — so those tests cannot hide behind the reference."""
import functools

import numpy as np
import pytest

import bucketed_sssp_ref as bref
import weighted_sssp_ref as ref

from lux_amd import cpu_ref
from lux_amd.graph import Graph

DELTAS = [1, 2, 7, 2 ** 31, 2 ** 33]
SMALL = (10, 8000, 3, 16)
WIDE = (12, 300000, 5, 1000)
MULTI = (11, 60000, 17, 16)


@functools.lru_cache(maxsize=None)
def _rmat(scale, ne, seed, wmax):
    g = Graph.rmat(scale, ne, seed=seed)
    g.hash_weights(wmax, seed=seed)
    return g, cpu_ref.sssp_weighted(g, 0)


@functools.lru_cache(maxsize=None)
def _run(spec, delta):
    g, _ = _rmat(*spec)
    return bref.bucketed(g, 0, delta)


def _bf_relaxed(g):
    _, sizes, vols = ref.bellman_ford(g, 0)
    flags = ref.predict_pull(g.nv, g.ne, sizes, vols)
    return sizes, flags, sum(g.ne if f else v for f, v in zip(flags, vols))


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("name", sorted(ref.HAND_CASES))
def test_hand_cases_labels(name, delta):
    g, want = ref.hand_graph(name)
    assert np.array_equal(cpu_ref.sssp_weighted(g, 0), want)
    lab, rows, advances, _ = bref.bucketed(g, 0, delta)
    assert np.array_equal(lab, want)
    if delta >= 2 ** 31:  # one bucket holds every finite distance below it
        assert advances == (1 if name == "saturation"
                            and delta == 2 ** 31 else 0)


@pytest.mark.parametrize("spec,delta", [(SMALL, 4), (WIDE, 64), (MULTI, 4)])
def test_rmat_labels(spec, delta):
    _, want = _rmat(*spec)
    lab, _, _, _ = _run(spec, delta)
    assert np.array_equal(lab, want)


@pytest.mark.parametrize("spec", [SMALL, WIDE, MULTI])
def test_huge_delta_is_bellman_ford(spec):
    """delta = 2^33: limit sits at 0xFFFFFFFE from the start, nothing is
    ever deferred, and the trace is the synchronous one row for row."""
    g, want = _rmat(*spec)
    sizes, flags, relaxed_bf = _bf_relaxed(g)
    lab, rows, advances, relaxed = _run(spec, 2 ** 33)
    assert np.array_equal(lab, want)
    assert advances == 0
    assert [r[1] for r in rows] == sizes
    assert [r[3] for r in rows] == flags
    assert {r[0] for r in rows} == {ref.SAT} and {r[4] for r in rows} == {0}
    assert relaxed == relaxed_bf


def test_small_input_at_delta_4():
    g, _ = _rmat(*SMALL)
    _, rows, advances, relaxed = _run(SMALL, 4)
    assert len(rows) == 11
    assert [i + 1 for i, r in enumerate(rows) if r[3]] == [3, 5]
    assert relaxed == 18548 < _bf_relaxed(g)[2] == 32635
    assert advances == 5


def test_wide_input_at_delta_64():
    g, _ = _rmat(*WIDE)
    _, rows, advances, relaxed = _run(WIDE, 64)
    assert len(rows) == 32
    assert [i + 1 for i, r in enumerate(rows) if r[3]] == [3, 4, 5, 6, 7]
    assert relaxed == 1558191 < _bf_relaxed(g)[2] == 2123645
    # active sets on both sides of the sparse-queue capacity
    capacity = g.nv // 16 + 100
    assert capacity == 356
    active = [r[1] for r in rows]
    assert [a for a in active if a >= capacity] == [698, 690, 494, 386]
    assert sum(a < capacity for a in active) == 28
    # an advance that skips empty buckets, and a bucket that takes more
    # than one iteration
    limits = [r[0] for r in rows]
    assert all((lim + 1) % 64 == 0 for lim in limits)
    steps = {(b - a) // 64 for a, b in zip(limits, limits[1:]) if b != a}
    assert max(steps) > 1
    assert max(limits.count(lim) for lim in set(limits)) > 1
    assert advances == len(set(limits)) - 1 == 18


def test_multi_input_at_delta_4():
    _, rows, advances, _ = _run(MULTI, 4)
    assert len(rows) == 10
    assert [i + 1 for i, r in enumerate(rows) if r[3]] == [2, 3, 4]
    assert advances == 5


def test_saturation_limit_clamps():
    g, want = ref.hand_graph("saturation")
    lab, rows, advances, _ = bref.bucketed(g, 0, 7)
    assert np.array_equal(lab, want)
    limits = [r[0] for r in rows]
    assert limits[-1] == ref.SAT == 0xFFFFFFFE
    # unclamped, the bucket of 0xFFFFFFFE would end at 0x100000003
    assert (ref.SAT // 7 + 1) * 7 - 1 > ref.SAT
    assert bref.next_limit(ref.SAT, 7) == ref.SAT
    assert advances == 2 and rows[-1][4] == 0


def test_deferred_rows_are_consistent():
    """Deferred counts only describe dirty vertices beyond the limit: the
    last row leaves none, and a row that is followed by an advance leaves
    some and no near one."""
    _, rows, advances, _ = _run(SMALL, 4)
    assert rows[-1][4] == 0
    jumps = sum(1 for a, b in zip(rows, rows[1:]) if a[0] != b[0])
    assert jumps == advances
    for a, b in zip(rows, rows[1:]):
        if a[0] != b[0]:
            assert a[4] > 0
