"""GPU k-clique counting (CliqueEngine, src/gpu/clique.hip) against closed
forms, pinned totals and the CPU oracle cpu_ref.cliques: complete graphs at
the wave/block and word edges, a complete 5-partite graph, RMATs under both
orders, both caps and the plain kernel, engine behaviour and the app. Counts
are integers: every comparison is equality."""
import os
from math import comb

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import clique_engine as cqe  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.clique_engine import CliqueEngine  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.tc_engine import ORDERS  # noqa: E402

RMAT10_CLIQUES = {3: 103301, 4: 649951, 5: 3068368, 6: 11188703}
RMAT12_4CLIQUES = 30216369


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
    monkeypatch.delenv("LUX_CLIQUE_CAP", raising=False)
    monkeypatch.delenv("LUX_CLIQUE_PLAIN", raising=False)


def make_engine(g, k, order="degree"):
    return CliqueEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0),
                        k=k, order=order)


def multipartite(parts, size):
    """The complete multipartite graph, vertex v in part v % parts."""
    n = parts * size
    a, b = np.meshgrid(np.arange(n, dtype=np.uint32),
                       np.arange(n, dtype=np.uint32))
    keep = (a % parts) != (b % parts)
    return Graph.from_edges(n, a[keep], b[keep])


def assert_counts(eng, total, pv):
    """pv: the expected u64 array, or one value for every vertex."""
    assert eng.count(per_vertex=True) == total
    got = eng.per_vertex().cpu().numpy().view(np.uint64)
    assert got.shape == (eng.part.nv,)
    assert np.array_equal(got, np.broadcast_to(pv, got.shape))
    assert int(got.sum()) == eng.k * total
    assert eng.count() == total  # the total-only instantiation


# ---- 1. complete graphs, order id: row 0 has n - 1 arcs ----

KN = [(n, k, None) for k in (3, 4, 5) for n in (k, 64, 65, 66, 129, 130)] + \
     [(20, k, None) for k in (6, 7, 8)] + \
     [(n, 4, 64) for n in (4, 64, 65, 66, 129, 130, 131)]


@pytest.mark.parametrize("n,k,cap", KN)
def test_complete_graph(n, k, cap, monkeypatch):
    if cap is not None:
        monkeypatch.setenv("LUX_CLIQUE_CAP", str(cap))
    eng = make_engine(multipartite(n, 1), k, "id")
    assert eng.stats["max_out_degree"] == n - 1
    assert_counts(eng, comb(n, k), comb(n - 1, k - 1))
    st = eng.stats
    assert st["items_hub"] == 0 or cap == 64
    if cap is None:
        assert st["spills"] == 0
        assert (st["items_block"] > 0) == (n - 1 > 64)
    elif n >= 66:
        assert st["items_hub"] > 0 and st["items_block"] == 0
    if n == 131:
        assert st["spills"] > 0


# ---- 2. complete 5-partite graph, parts of 13 ----

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", [3, 4, 5, 6])
def test_five_partite(k, order):
    eng = make_engine(multipartite(5, 13), k, order)
    assert_counts(eng, comb(5, k) * 13 ** k, comb(4, k - 1) * 13 ** (k - 1))
    assert eng.check() == 0


# ---- 3. RMAT-10 ----

@pytest.fixture(scope="module")
def rmat10():
    g = Graph.rmat(10, 40000, seed=3, sym=True)
    return dict(g=g, pv={k: cpu_ref.cliques(g, k)[1] for k in RMAT10_CLIQUES})


RMAT10_CASES = [(k, order, cap, False) for k in RMAT10_CLIQUES
                for order in ORDERS for cap in (None, 64)] + \
               [(4, "degree", None, True)]


@pytest.mark.parametrize("k,order,cap,plain", RMAT10_CASES)
def test_rmat10(rmat10, k, order, cap, plain, monkeypatch):
    if cap is not None:
        monkeypatch.setenv("LUX_CLIQUE_CAP", str(cap))
    if plain:
        monkeypatch.setenv("LUX_CLIQUE_PLAIN", "1")
    eng = make_engine(rmat10["g"], k, order)
    assert eng.plain == plain and eng.cap == (cap or cqe.CAP_DEFAULT)
    assert_counts(eng, RMAT10_CLIQUES[k], rmat10["pv"][k])
    assert eng.check() == 0
    st = eng.stats
    assert st["simple_edges"] == 12252
    if order == "degree":
        assert st["max_out_degree"] == 46
        assert st["items_wave"] > 0
        assert st["items_block"] == 0 and st["items_hub"] == 0
    elif cap is None:
        assert st["items_block"] > 0 and st["items_hub"] == 0
    else:
        assert st["items_hub"] > 0
    if not plain:
        assert st["set_ops"] > 0 and st["built_bits"] > 0


# ---- 4, 5. RMAT-12, symmetric and directed ----

@pytest.fixture(scope="module")
def rmat12():
    g = Graph.rmat(12, 300000, seed=3, sym=True)
    total, pv = cpu_ref.cliques(g, 4)
    return dict(g=g, total=total, pv=pv)


@pytest.mark.parametrize("order", ORDERS)
def test_rmat12(rmat12, order):
    assert rmat12["total"] == RMAT12_4CLIQUES
    eng = make_engine(rmat12["g"], 4, order)
    assert_counts(eng, RMAT12_4CLIQUES, rmat12["pv"])
    st = eng.stats
    assert st["max_out_degree"] == dict(degree=130, id=1896)[order]
    assert st["items_block"] > 0
    assert (st["items_hub"] > 0) == (order == "id")
    assert eng.check() == 0


@pytest.mark.parametrize("order", ORDERS)
def test_rmat12_directed(order):
    """One-way arcs with duplicates and self-loops."""
    g = Graph.rmat(12, 300000, seed=3)
    total, pv = cpu_ref.cliques(g, 4)
    assert total > 0
    assert_counts(make_engine(g, 4, order), total, pv)


# ---- 6. engine and app ----

def test_engine_state_and_check(rmat10):
    eng = make_engine(rmat10["g"], 4)
    for _ in range(2):
        assert_counts(eng, RMAT10_CLIQUES[4], rmat10["pv"][4])
    assert eng.density() == RMAT10_CLIQUES[4] / comb(1024, 4)
    assert eng.check() == 0
    pv = eng.per_vertex()
    v = int(np.argmax(rmat10["pv"][4]))
    pv[v] += 1
    assert eng.check() >= 1
    pv[v] -= 1
    assert eng.check() == 0


def test_bad_arguments_raise(monkeypatch):
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    for k in (2, 9):
        with pytest.raises(ValueError, match="k must be"):
            CliqueEngine(part, k=k)
    with pytest.raises(ValueError, match="single-rank"):
        CliqueEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0))
    assert cqe.CAP_MAX == ng.clique_const("cap_max")
    for cap in (96, 0, cqe.CAP_MAX + 64):
        monkeypatch.setenv("LUX_CLIQUE_CAP", str(cap))
        with pytest.raises(ValueError, match="LUX_CLIQUE_CAP"):
            CliqueEngine(part)


def test_clique_app_main_check(capsys):
    from lux_amd.apps import clique
    clique.main(["-synthetic", "rmat:10:40000", "-clique", "4", "-check",
                 "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] clique: k 4, " in out
    assert "role,class,items" in out
    assert "[PASS] 0 mistakes" in out
    with pytest.raises(SystemExit):
        clique.main(["-synthetic", "rmat:10:40000", "-clique", "9"])
