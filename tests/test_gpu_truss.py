"""GPU k-truss (TrussEngine, src/gpu/truss.hip) against the exact CPU oracle
cpu_ref.edge_support / cpu_ref.truss: the hand cases, cliques across the
lane-held boundary, book graphs across the wave / hub, chunk and fence
boundaries at LUX_TRUSS_HUB=64, RMAT-10 and the directed RMAT-12 with their
pinned values, engine behaviour and the app. Everything is an integer per
edge: every comparison is equality, with the round fusion off and on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import truss_ref  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.truss_engine import TrussEngine  # noqa: E402

KNOBS = ("LUX_TRUSS_HUB", "LUX_TRUSS_FUSE", "LUX_TRUSS_FENCE",
         "LUX_TC_SORT_CHUNK")
FUSE = pytest.mark.parametrize("fuse", [0, None], ids=["nofuse", "fuse"])


def clique(n):
    e = [(a, b) for a in range(n) for b in range(a + 1, n)]
    return Graph.from_edges(n, [x[0] for x in e], [x[1] for x in e])


def book(n):
    """The spine (0, 1) and n pages adjacent to both."""
    pages = list(range(2, n + 2))
    return Graph.from_edges(n + 2, [0] + [0] * n + [1] * n,
                            [1] + pages + pages)


_REF = {}


def reference(name, g):
    """(edges, support, trussness, triangles) of the oracle, once a graph."""
    if name not in _REF:
        edges, support = cpu_ref.edge_support(g)
        out = (edges, support, cpu_ref.truss(g), cpu_ref.triangles(g)[0])
        for x in out[:3]:
            x.setflags(write=False)
        _REF[name] = out
    return _REF[name]


def run(name, g, monkeypatch, fuse=None, hub=None, chunk=None):
    """Decompose g under the knobs and compare everything with the oracle;
    returns (engine, oracle trussness)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in zip(KNOBS, (hub, fuse, None, chunk)):
        if v is not None:
            monkeypatch.setenv(k, str(v))
    edges, support, want, triangles = reference(name, g)
    eng = TrussEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))
    m = edges.shape[0]
    lo, hi = (x.cpu().numpy() for x in eng.edges())
    assert np.array_equal(lo, edges[:, 0]) and np.array_equal(hi, edges[:, 1])
    sup = eng.support().cpu().numpy()
    assert sup.dtype == np.int32 and np.array_equal(sup, support)
    assert int(sup.sum()) == 3 * triangles
    got = eng.decompose().cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    st = eng.stats
    print(st, eng.level_trace[:4])
    assert st["simple_edges"] == m
    assert st["items_lane"] + st["items_wave"] <= m
    assert st["levels"] == len(np.unique(want))
    assert [t[0] for t in eng.level_trace] == sorted(set(want.tolist()))
    assert sum(t[2] for t in eng.level_trace) == m
    assert st["scans"] <= 2 * st["levels"]
    assert st["rounds"] == sum(t[1] for t in eng.level_trace)
    if fuse == 0:
        assert st["fused_rounds"] == 0
        assert st["host_reads"] == st["scans"] + st["rounds"]
    assert eng.check() == 0
    assert eng.kmax() == int(want.max(initial=2))
    assert np.array_equal(eng.truss_sizes().cpu().numpy(), np.bincount(want))
    return eng, want


@FUSE
@pytest.mark.parametrize("case", truss_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, fuse, monkeypatch):
    eng, want = run(case.name, case.g, monkeypatch, fuse=fuse)
    lo, hi = (x.cpu().numpy() for x in eng.edges())
    assert np.array_equal(want, case.truss(lo, hi))
    if case.name == "one_way_triangle":
        assert eng.stats["rounds"] == 1  # all three edges leave together


@FUSE
@pytest.mark.parametrize("n", [64, 65, 66])
def test_cliques_across_the_lane_boundary(n, fuse, monkeypatch):
    eng, want = run(f"k{n}", clique(n), monkeypatch, fuse=fuse)
    assert (want == n).all() and eng.stats["max_degree"] == n - 1
    lane = eng.stats["items_lane"]
    assert lane == (want.size if n <= 65 else 0)
    assert eng.stats["items_wave"] == want.size - lane


@FUSE
@pytest.mark.parametrize("n", [62, 63, 64, 65, 129, 3000])
def test_books_across_the_hub_boundary(n, fuse, monkeypatch):
    eng, want = run(f"book{n}", book(n), monkeypatch, fuse=fuse, hub=64)
    assert (want == 3).all()
    assert int(eng.support()[0].item()) == n  # the spine is edge 0
    items = -(-(n + 1) // 64) if n + 1 > 64 else 0
    assert eng.stats["items_hub"] == eng.stats["hub_items"] == items
    assert (n + 1 > eng.fence) == (n == 3000)  # 3000: two search levels


RMAT10 = dict(m=7050, kmax=19, top=972, two=491,
              alive={4: 5974, 8: 3889, 16: 1133})


@FUSE
@pytest.mark.parametrize("hub,chunk", [(None, None), (64, None), (64, 2048)],
                         ids=["default", "hub64", "hub64-chunked"])
def test_rmat10(hub, chunk, fuse, monkeypatch):
    g = Graph.rmat(10, 20000, seed=3, sym=True)
    eng, want = run("rmat10", g, monkeypatch, fuse=fuse, hub=hub, chunk=chunk)
    assert (want.size, eng.kmax()) == (RMAT10["m"], RMAT10["kmax"])
    sizes = eng.truss_sizes().cpu().numpy()
    assert (int(sizes[-1]), int(sizes[2])) == (RMAT10["top"], RMAT10["two"])
    for k, ne in RMAT10["alive"].items():
        assert int(eng.truss(k).sum().item()) == ne
    if hub == 64:
        assert eng.stats["hub_items"] == eng.stats["items_hub"] > 0
    # a second decompose() starts from scratch
    assert np.array_equal(eng.decompose().cpu().numpy(), want)
    assert sum(t[2] for t in eng.level_trace) == want.size


@FUSE
def test_rmat12_directed(fuse, monkeypatch):
    g = Graph.rmat(12, 300000, seed=3)  # duplicates and self-loops
    eng, want = run("rmat12", g, monkeypatch, fuse=fuse)
    assert want.size == 160602 and eng.kmax() == 118
    assert int(eng.truss_sizes()[-1].item()) == 30929


def test_check_sees_a_raised_entry(monkeypatch):
    eng, _ = run("k6", clique(6), monkeypatch)
    bad = eng.trussness().clone()
    bad[7] += 1  # claims a truss it is not in
    assert eng.check(bad) > 0
    assert eng.check() == 0


def test_two_parts_raise():
    g = Graph.rmat(10, 8000, seed=3)
    with pytest.raises(ValueError, match="single-rank"):
        TrussEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0))


def test_truss_app_main_check(capsys):
    from lux_amd.apps import truss
    truss.main(["-synthetic", "rmat:12:300000", "-truss", "8", "-check",
                "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] truss: kmax " in out
    assert "phases orient/adjacency/support/peel" in out
    assert "the 8-truss has " in out
    assert "k,removed,rounds" in out
    assert "[PASS] 0 mistakes" in out
