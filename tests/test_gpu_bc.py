"""GPU betweenness centrality (BCEngine, src/gpu/bc.hip) against the fp64
oracle: hand cases, the in-/out-degree ladders that put a row on every bin
edge of the forward and backward roles, two RMATs with multi-chunk hubs,
engine behaviour and the app. Tolerances come from bc_ref.tolerance; depth
and every sigma below 2^24 compare exactly."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bc_ref  # noqa: E402
from degree_ladder import LADDER  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.bc_engine import BCEngine  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402

INF = bc_ref.INF


@pytest.fixture(autouse=True)
def native_lib_is_loaded():
    """The HIP extension must be the in-tree .so (no silent fallback)."""
    import lux_amd
    path = ng.lib()._name
    assert path.endswith("liblux_gpu.so")
    assert os.path.dirname(os.path.abspath(path)) == \
        os.path.dirname(os.path.abspath(lux_amd.__file__))


def make_engine(g):
    return BCEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def run(eng, source):
    """(depth u32, sigma f32, delta f32) on the host, after run(source)."""
    delta = eng.run(source)
    nv = eng.part.nv
    return (host(eng.depth(), np.uint32)[:nv].copy(),
            host(eng.sigma())[:nv].copy(), host(delta)[:nv].copy())


def assert_matches(got, g, depth, sigma, delta):
    gd, gs, gl = got
    assert np.array_equal(gd, depth)
    bc_ref.assert_sigma_exact(gs, sigma)
    bc_ref.assert_close(gl, delta, g, depth, "delta")
    unreached = depth == INF
    assert not gs[unreached].any() and not gl[unreached].any()


# ---- 1. hand cases ----

@pytest.mark.parametrize("case", bc_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    eng = make_engine(case.g)
    got = run(eng, case.source)
    assert_matches(got, case.g, case.want["depth"], case.want["sigma"],
                   case.want["delta"])
    assert eng.check() == 0


# ---- 2. in-degree ladder: forward roles at every bin edge ----

def test_in_degree_ladder():
    lad = bc_ref.in_ladder()
    eng = make_engine(lad.g)
    gd, gs, gl = run(eng, 0)
    assert eng.levels == 4
    assert np.array_equal(gd, lad.depth)
    bc_ref.assert_sigma_exact(gs, lad.sigma)
    assert np.array_equal(gs[lad.rows], np.asarray(LADDER, np.float32))
    bc_ref.assert_close(gl, lad.delta, lad.g, lad.depth, "delta")
    assert eng.check() == 0


# ---- 3. out-degree ladder: backward roles at every bin edge ----

def test_out_degree_ladder():
    lad = bc_ref.out_ladder()
    eng = make_engine(lad.g)
    gd, gs, gl = run(eng, 0)
    assert eng.levels == 3
    assert np.array_equal(gd, lad.depth)
    bc_ref.assert_sigma_exact(gs, lad.sigma)
    # sigma all 1, q all integers: exact in any order, so one dropped or
    # doubled edge in any thread, wave or chunk row is an integer off
    assert np.array_equal(gl[lad.rows], np.asarray(LADDER, np.float32))
    assert np.array_equal(gl.astype(np.float64), lad.delta)
    assert eng.check() == 0


def test_deep_traversal():
    """302 levels: the level order runs without its LDS key table (it holds
    768 keys = 256 levels), with a chunk-bin row in either direction."""
    lad = bc_ref.deep_chain()
    eng = make_engine(lad.g)
    got = run(eng, 0)
    assert eng.levels == lad.levels
    assert_matches(got, lad.g, lad.depth, lad.sigma, lad.delta)
    assert eng.check() == 0


# ---- 4. RMAT ----

@pytest.fixture(scope="module", params=bc_ref.RMATS,
                ids=lambda p: f"rmat{p[0]}")
def rmat(request):
    scale, ne, seed = request.param
    g = Graph.rmat(scale, ne, seed=seed)
    d0 = cpu_ref.betweenness(g, 0)
    src2 = bc_ref.second_source(g, d0[0])
    return dict(g=g, eng=make_engine(g), sources=[0, src2],
                want={0: d0, src2: cpu_ref.betweenness(g, src2)})


@pytest.mark.parametrize("which", [0, 1])
def test_rmat(rmat, which):
    g, eng = rmat["g"], rmat["eng"]
    source = rmat["sources"][which]
    depth, sigma, delta = rmat["want"][source]
    got = run(eng, source)
    assert_matches(got, g, depth, sigma, delta)
    assert eng.levels == int(depth[depth != INF].max()) + 1
    assert eng.check() == 0
    # the oracle sees one corrupted entry of either array
    v = int(np.argmax(delta))
    assert delta[v] > 0 and sigma[v] > 0
    for arr in (eng.delta(), eng.sigma()):
        keep = arr[v].clone()
        arr[v] = keep * 2 + 1
        assert eng.check() >= 1
        arr[v] = keep
    assert eng.check() == 0


# ---- 5. engine behaviour ----

def test_run_sources_is_the_sum(rmat):
    g, eng = rmat["g"], rmat["eng"]
    a, b = rmat["sources"]
    want = rmat["want"][a][2] + rmat["want"][b][2]
    single = run(eng, a)[2].astype(np.float64) + \
        run(eng, b)[2].astype(np.float64)
    bc = host(eng.run_sources([a, b]))[:g.nv].astype(np.float64)
    assert np.array_equal(host(eng.bc())[:g.nv].astype(np.float64), bc)
    # each delta is within its rtol of its oracle, so a sum of two
    # non-negative ones is within the larger rtol (+ 2^-24 for the fp32
    # add) of the oracle sum, and two such sums within twice that
    rtol = 2 * max(bc_ref.tolerance(g, rmat["want"][s][0],
                                    rmat["want"][s][2])[0] for s in (a, b))
    np.testing.assert_allclose(bc, single, rtol=rtol, atol=0)
    np.testing.assert_allclose(bc, want, rtol=rtol, atol=0)


def test_second_run_leaves_no_state(rmat):
    g, eng = rmat["g"], rmat["eng"]
    a, b = rmat["sources"]
    run(eng, a)
    again = run(eng, b)
    fresh = run(make_engine(g), b)
    assert np.array_equal(again[0], fresh[0])
    assert np.array_equal(again[1], fresh[1])  # sigma: exact integers
    # delta: hub chunks meet in atomics, so two runs may differ by rounding
    depth, _, delta = rmat["want"][b]
    bc_ref.assert_close(again[2], delta, g, depth, "second run")
    bc_ref.assert_close(fresh[2], delta, g, depth, "fresh engine")
    unreached = depth == INF
    assert not again[1][unreached].any() and not again[2][unreached].any()


def test_stats_count_the_dag_edges(rmat):
    g, eng = rmat["g"], rmat["eng"]
    source = rmat["sources"][0]
    run(eng, source)
    ref = bc_ref.brandes(g, source)
    st = eng.stats
    assert [r["level"] for r in st] == list(range(ref.levels))
    assert sum(r["edges_in"] for r in st) == ref.dag_edges
    assert sum(r["edges_out"] for r in st) == ref.dag_edges
    per_level = np.bincount(ref.depth[ref.depth != INF],
                            minlength=ref.levels)
    assert [r["rows_in"] for r in st] == per_level.tolist()
    assert [r["rows_out"] for r in st] == per_level.tolist()


def test_two_parts_raise():
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        BCEngine(part)


# ---- 6. app ----

def test_bc_app_main_check(capsys):
    from lux_amd.apps import bc
    bc.main(["-start", "0", "-synthetic", "rmat:12:300000", "-check"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] bc: " in out and "phases bfs/order/sigma/delta" in out
    assert "[PASS] 0 mistakes" in out
