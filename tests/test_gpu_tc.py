"""GPU triangle counting (TCEngine, src/gpu/tc.hip) against the exact CPU
oracle cpu_ref.triangles: hand cases under both orders, the role ladder
that puts a row on every role, item and lane-stride edge (at the default
stage cap and at LUX_TC_STAGE=64), a symmetric and a directed RMAT under
both orders and the plain kernel, a total past 2^32, engine behaviour and
the app. Counts are integers: every comparison is equality."""
import os
from math import comb

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tc_ref  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd import tc_engine as tce  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.tc_engine import TCEngine  # noqa: E402


@pytest.fixture(autouse=True)
def native_lib_is_loaded():
    """The HIP extension must be the in-tree .so (no silent fallback)."""
    import lux_amd
    path = ng.lib()._name
    assert path.endswith("liblux_gpu.so")
    assert os.path.dirname(os.path.abspath(path)) == \
        os.path.dirname(os.path.abspath(lux_amd.__file__))


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv("LUX_TC_STAGE", raising=False)
    monkeypatch.delenv("LUX_TC_PLAIN", raising=False)


def make_engine(g, order="degree"):
    return TCEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0),
                    order=order)


def host_pv(eng):
    return eng.per_vertex().cpu().numpy().view(np.uint64)


def assert_counts(eng, total, pv):
    assert eng.count(per_vertex=True) == total
    got = host_pv(eng)
    assert got.shape == pv.shape
    assert np.array_equal(got, pv)
    assert int(got.sum()) == 3 * total
    assert eng.count() == total  # the total-only instantiation


# ---- 1. hand cases ----

@pytest.mark.parametrize("order", tce.ORDERS)
@pytest.mark.parametrize("case", tc_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, order):
    total, pv = cpu_ref.triangles(case.g)
    assert total == case.want["total"]
    assert np.array_equal(pv, case.want["per_vertex"])
    eng = make_engine(case.g, order)
    assert_counts(eng, total, pv)
    assert eng.check() == 0
    if case.name == "star" and order == "id":
        assert eng.stats["max_out_degree"] == case.g.nv - 1
    if case.name == "fan" and order == "id":
        assert eng.stats["max_out_degree"] == tc_ref.FAN_N


# ---- 2. role ladder ----

@pytest.mark.parametrize("stage", [None, 64], ids=["default", "stage64"])
def test_role_ladder(stage, monkeypatch):
    if stage is not None:
        monkeypatch.setenv("LUX_TC_STAGE", str(stage))
    cap = stage if stage is not None else tce.TC_STAGE_DEFAULT
    lad = tc_ref.ladder(cap, tce.TC_T1, tce.TC_CHUNK)
    total, pv = cpu_ref.triangles(lad.g)
    assert np.array_equal(pv[lad.rows], lad.row_counts)
    eng = make_engine(lad.g, "id")
    assert eng.stage_cap == cap
    d = (eng.dag.optr[1:] - eng.dag.optr[:-1]).cpu().numpy()
    assert np.array_equal(d[lad.rows], lad.degrees)
    assert np.array_equal(d[lad.specials], tc_ref.POOL_DEGREES)
    assert_counts(eng, total, pv)
    assert np.array_equal(host_pv(eng)[lad.rows], lad.row_counts)
    assert eng.check() == 0
    st = eng.stats
    assert st["items_small"] > 0 and st["items_staged"] > 0 \
        and st["items_hub"] > 0
    assert st["max_out_degree"] == int(lad.degrees.max())


# ---- 3. RMAT ----

RMAT_TRIANGLES = 1882531
RMAT_SIMPLE_EDGES = 94769
RMAT_MAX_OUT = dict(degree=130, id=1896)


@pytest.fixture(scope="module")
def rmat():
    g = Graph.rmat(12, 300000, seed=3, sym=True)
    total, pv = cpu_ref.triangles(g)
    return dict(g=g, total=total, pv=pv)


@pytest.mark.parametrize("plain", [False, True], ids=["roles", "plain"])
@pytest.mark.parametrize("order", tce.ORDERS)
def test_rmat(rmat, order, plain, monkeypatch):
    if plain:
        monkeypatch.setenv("LUX_TC_PLAIN", "1")
    g, total, pv = rmat["g"], rmat["total"], rmat["pv"]
    assert total == RMAT_TRIANGLES
    eng = make_engine(g, order)
    assert eng.plain == plain
    assert_counts(eng, RMAT_TRIANGLES, pv)
    st = eng.stats
    assert st["simple_edges"] == RMAT_SIMPLE_EDGES
    assert st["max_out_degree"] == RMAT_MAX_OUT[order]
    assert st["probes"] > 0
    want = tc_ref.transitivity(g, total)
    assert want > 0
    assert abs(eng.transitivity() - want) <= 1e-12 * want
    assert eng.check() == 0


@pytest.mark.parametrize("order", tce.ORDERS)
def test_rmat_directed(order):
    """One-way arcs with duplicates and self-loops."""
    g = Graph.rmat(12, 300000, seed=3)
    total, pv = cpu_ref.triangles(g)
    assert total > 0
    eng = make_engine(g, order)
    assert_counts(eng, total, pv)
    assert eng.check() == 0


# ---- 4. 64-bit total ----

def test_total_past_32_bits():
    """K_2956: C(2956, 3) = 2956 * 2955 * 2954 / 6 = 4,300,521,820 > 2^32
    triangles, C(2955, 2) per vertex (closed form; about 4.3e9 probes)."""
    n = 2956
    a = np.repeat(np.arange(n, dtype=np.uint32), n)
    b = np.tile(np.arange(n, dtype=np.uint32), n)
    keep = a != b
    g = Graph.from_edges(n, a[keep], b[keep])
    assert g.ne == n * (n - 1)
    want = comb(n, 3)
    assert want == 4300521820 and want > 2 ** 32
    eng = make_engine(g)
    assert eng.count(per_vertex=True) == want
    assert eng.stats["simple_edges"] == comb(n, 2)
    assert eng.stats["probes"] == want  # sum over arcs (u, v) of |A(v)|
    pv = host_pv(eng)
    assert (pv == comb(n - 1, 2)).all()
    assert eng.transitivity() == 1.0


# ---- 5. engine behaviour ----

@pytest.fixture(scope="module")
def rmat_engine(rmat):
    return make_engine(rmat["g"])


def test_count_twice_leaves_no_state(rmat, rmat_engine):
    eng = rmat_engine
    assert eng.count() == rmat["total"]
    assert eng.count() == rmat["total"]
    assert eng.count(per_vertex=True) == rmat["total"]
    assert np.array_equal(host_pv(eng), rmat["pv"])
    assert eng.count(per_vertex=True) == rmat["total"]
    assert np.array_equal(host_pv(eng), rmat["pv"])
    assert eng.stats["probes"] > 0


def test_check_sees_one_corrupted_entry(rmat, rmat_engine):
    eng = rmat_engine
    eng.count(per_vertex=True)
    assert eng.check() == 0
    pv = eng.per_vertex()
    v = int(np.argmax(rmat["pv"]))
    keep = pv[v].clone()
    pv[v] = keep + 1
    assert eng.check() >= 1
    pv[v] = keep
    assert eng.check() == 0


def test_two_parts_raise():
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        TCEngine(part)


def test_stage_cap_is_validated(monkeypatch):
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    assert tce.TC_STAGE_MAX == ng.tc_stage_max()
    monkeypatch.setenv("LUX_TC_STAGE", str(tce.TC_STAGE_MAX + 1))
    with pytest.raises(ValueError, match="LUX_TC_STAGE"):
        TCEngine(part)


# ---- 6. app ----

def test_tc_app_main_check(capsys):
    from lux_amd.apps import tc
    tc.main(["-synthetic", "rmat:12:300000", "-check", "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] tc: " in out and "phases orient/items/count" in out
    assert "items,probes,role" in out
    assert "[PASS] 0 mistakes" in out
