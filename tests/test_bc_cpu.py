"""Betweenness centrality on the CPU: the C++ fp64 oracle
(cpu_ref.betweenness) against the independent numpy Brandes of bc_ref.py,
the hand cases' closed forms, and the ladder builders' stated shapes."""
import numpy as np
import pytest

import bc_ref
from degree_ladder import LADDER
from lux_amd import cpu_ref
from lux_amd.graph import Graph

INF = bc_ref.INF


def _oracle_equals_numpy(g, source):
    depth, sigma, delta = cpu_ref.betweenness(g, source)
    ref = bc_ref.brandes(g, source)
    assert depth.dtype == np.uint32
    assert sigma.dtype == np.float64 and delta.dtype == np.float64
    assert np.array_equal(depth, ref.depth)
    # both fp64, different summation orders
    if ref.sigma.max() < 2 ** 53:
        assert np.array_equal(sigma, ref.sigma)
    else:
        np.testing.assert_allclose(sigma, ref.sigma, rtol=1e-12)
    np.testing.assert_allclose(delta, ref.delta, rtol=1e-11, atol=0)
    return ref


@pytest.mark.parametrize("case", bc_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    ref = _oracle_equals_numpy(case.g, case.source)
    assert np.array_equal(ref.depth, case.want["depth"])
    assert np.array_equal(ref.sigma, case.want["sigma"])
    np.testing.assert_allclose(ref.delta, case.want["delta"], rtol=1e-15)
    depth, sigma, delta = cpu_ref.betweenness(case.g, case.source)
    assert np.array_equal(sigma, case.want["sigma"])
    np.testing.assert_allclose(delta, case.want["delta"], rtol=1e-15)
    unreached = depth == INF
    assert not sigma[unreached].any() and not delta[unreached].any()


@pytest.mark.parametrize("scale,ne,seed", bc_ref.RMATS)
def test_oracle_matches_numpy_on_rmat(scale, ne, seed):
    g = Graph.rmat(scale, ne, seed=seed)
    ref = _oracle_equals_numpy(g, 0)
    assert ref.sigma.max() < 2 ** 24  # what makes the GPU sigma exact
    assert ref.delta[0] == 0.0
    src2 = bc_ref.second_source(g, ref.depth)
    assert src2 != 0
    ref2 = _oracle_equals_numpy(g, src2)
    assert ref2.sigma.max() < 2 ** 24


def test_big_rmat_reaches_multi_chunk_hubs():
    g = Graph.rmat(12, 300000, seed=5)
    indeg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    outdeg = np.bincount(g.src, minlength=g.nv)
    assert indeg.max() > 8192 and outdeg.max() > 8192


def test_source_out_of_range():
    g = bc_ref.hand_cases()[0].g
    with pytest.raises(ValueError):
        cpu_ref.betweenness(g, g.nv)


def test_in_ladder_shape_and_values():
    lad = bc_ref.in_ladder()
    g = lad.g
    assert (g.nv, g.ne) == (355, 163881)
    indeg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    assert np.array_equal(indeg[lad.rows], LADDER)
    assert LADDER[-1] == 24577  # 4 chunks
    ref = _oracle_equals_numpy(g, 0)
    assert ref.levels == lad.levels == 4
    assert np.array_equal(ref.depth, lad.depth)
    assert np.array_equal(ref.sigma, lad.sigma)
    assert np.array_equal(ref.sigma[lad.rows], LADDER)
    np.testing.assert_allclose(ref.delta, lad.delta, rtol=1e-12)
    assert np.nonzero(ref.depth == INF)[0].tolist() == \
        [int(lad.rows[0]), int(lad.sinks[0])]
    assert np.array_equal(ref.delta[lad.rows[1:]], np.ones(len(LADDER) - 1))
    assert ref.delta[lad.rows[0]] == 0
    pool = ref.delta[lad.pool]
    assert 0.16 < pool.min() and pool.max() < 2.3


def test_out_ladder_shape_and_values():
    lad = bc_ref.out_ladder()
    g = lad.g
    assert (g.nv, g.ne) == (163626, 163625)
    outdeg = np.bincount(g.src, minlength=g.nv)
    assert np.array_equal(outdeg[lad.rows], LADDER)
    ref = _oracle_equals_numpy(g, 0)
    assert ref.levels == lad.levels == 3
    assert np.array_equal(ref.depth, lad.depth)
    assert np.array_equal(ref.sigma, lad.sigma)
    assert np.array_equal(ref.delta, lad.delta)
    assert np.array_equal(ref.delta[lad.rows], LADDER)


def test_deep_chain_shape_and_values():
    lad = bc_ref.deep_chain()
    ref = _oracle_equals_numpy(lad.g, 0)
    assert ref.levels == lad.levels == 302 and 3 * ref.levels > 768
    assert bc_ref.max_degree(lad.g) == 2100  # a chunk-bin row each way
    assert np.array_equal(ref.depth, lad.depth)
    assert np.array_equal(ref.sigma, lad.sigma)
    np.testing.assert_allclose(ref.delta, lad.delta, rtol=1e-12)


def test_tolerance_formula():
    case = bc_ref.hand_cases()[1]  # diamond: L = 4, maxdeg = 2
    rtol, atol = bc_ref.tolerance(case.g, case.want["depth"],
                                  case.want["delta"])
    assert rtol == 1.01 * 4 * 5 * 2.0 ** -24
    assert atol == rtol * 1.0


def test_nsrc_flag():
    from lux_amd.apps.common import parse_input_args
    assert parse_input_args(["-start", "5"]).nsrc == 1
    a = parse_input_args(["-synthetic", "rmat:10:8000", "-start", "5",
                          "-nsrc", "3", "-check"])
    assert (a.start, a.nsrc, a.check) == (5, 3, True)
