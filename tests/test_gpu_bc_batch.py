"""Batched betweenness centrality (BatchedBCEngine, src/gpu/bc_batch.hip)
against the fp64 oracle bc_ref.brandes, per source: hand cases, the in-/out-
degree ladders at every width and at both ends of the hub knob, the batch
edges on an RMAT, a 302-level graph, arguments and the app. Depth and every
sigma below 2^24 compare exactly; tolerances come from bc_ref.tolerance."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bc_ref  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd.bc_batch_engine import BatchedBCEngine  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402

U = bc_ref.U


@pytest.fixture(autouse=True)
def native_lib_is_loaded():
    """The HIP extension must be the in-tree .so (no silent fallback)."""
    import lux_amd
    path = ng.lib()._name
    assert path.endswith("liblux_gpu.so")
    assert os.path.dirname(os.path.abspath(path)) == \
        os.path.dirname(os.path.abspath(lux_amd.__file__))


def make_engine(g, width=None):
    return BatchedBCEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0),
                           width)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "rmat":
        return Graph.rmat(10, 8000, seed=3)
    return getattr(bc_ref, name)().g


@functools.lru_cache(maxsize=None)
def ref(name, source):
    return bc_ref.brandes(graph(name), source)


def assert_columns(eng, g, refs):
    """Every column of the last batch against its source's oracle; the
    padding columns are unreached."""
    k = len(refs)
    dep = eng.depths().cpu().numpy().view(np.uint16).astype(np.uint32)
    dep[dep == 0xFFFF] = bc_ref.INF
    sigma, delta = eng.sigma().cpu().numpy(), eng.delta().cpu().numpy()
    for c, r in enumerate(refs):
        assert np.array_equal(dep[:, c], r.depth), c
        bc_ref.assert_sigma_exact(sigma[:, c], r.sigma)
        bc_ref.assert_close(delta[:, c], r.delta, g, r.depth,
                            f"delta of column {c}")
    assert (dep[:, k:] == bc_ref.INF).all()
    assert not sigma[:, k:].any() and not delta[:, k:].any()
    assert eng.check() == 0


def assert_bc(bc, name, sources, B):
    """bc against the fp64 sum: each delta is within its rtol, the column
    sum adds B * 2^-24 and every further batch one fp32 add."""
    g = graph(name)
    refs = [ref(name, s) for s in sources]
    rtol = max(bc_ref.tolerance(g, r.depth, r.delta)[0] for r in refs) + \
        (B + (len(sources) - 1) // B) * U
    np.testing.assert_allclose(bc.cpu().numpy().astype(np.float64),
                               sum(r.delta for r in refs), rtol=rtol, atol=0)


# ---- 1. hand cases: all nv <= 5 vertices are sources, the rest padding ----

@pytest.mark.parametrize("case", bc_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case):
    eng = make_engine(case.g)
    nv = case.g.nv
    eng.run(range(nv), keep_sigma=True)
    assert eng.B == 16
    assert_columns(eng, case.g, [bc_ref.brandes(case.g, s) for s in range(nv)])


# ---- 2. ladders: every role edge, widths, one to hundreds of chunks ----

@pytest.mark.parametrize("hub", ["default", "min"])
@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("name", ["in_ladder", "out_ladder"])
def test_ladders(name, width, hub, monkeypatch):
    if hub == "min":
        monkeypatch.setenv("LUX_BCB_HUB", str(ng.bcb_hub_min()))
    # source 0 and the B - 1 vertices after it, pool vertices or rows (and,
    # past the 49 rows of the out-ladder, leaves): the columns of one row
    # sit at different depths
    sources = list(range(width))
    eng = make_engine(graph(name), width)
    assert eng.hub == (ng.bcb_hub_min() if hub == "min"
                       else ng.bcb_hub_default())
    bc = eng.run(sources, keep_sigma=True)
    assert_columns(eng, graph(name), [ref(name, s) for s in sources])
    assert_bc(bc, name, sources, width)


# ---- 3. batch edges ----

@pytest.mark.parametrize("k", [1, 17, 64, 65, 130])
def test_batch_edges(k):
    sources = list(range(k))
    eng = make_engine(graph("rmat"))
    first = eng.run(sources, keep_sigma=True).clone()
    B = eng.B
    assert B == (16 if k == 1 else 32 if k == 17 else 64)
    assert_bc(first, "rmat", sources, B)
    last = sources[(k - 1) // B * B:]
    assert_columns(eng, graph("rmat"), [ref("rmat", s) for s in last])
    assert np.array_equal(eng.run(sources, keep_sigma=True).cpu().numpy(),
                          first.cpu().numpy())  # identical bits
    assert eng.check() == 0
    # the oracle sees one corrupted entry of either array
    v = int(np.argmax(ref("rmat", last[0]).delta))
    for arr in (eng.sigma(), eng.delta()):
        keep = arr[v, 0].clone()
        arr[v, 0] = keep * 2 + 1
        assert eng.check() >= 1
        arr[v, 0] = keep
    assert eng.check() == 0


# ---- 4. deep graph: 302 levels, a hub in both directions ----

def test_deep_graph():
    eng = make_engine(graph("deep_chain"))
    eng.run([0, 150], keep_sigma=True)
    assert eng.levels == 302 and eng.B == 16
    assert_columns(eng, graph("deep_chain"),
                   [ref("deep_chain", s) for s in (0, 150)])


# ---- 5. arguments ----

@pytest.mark.parametrize("sources", [[1, 2, 1], [0, 1024], [-1], []],
                         ids=["duplicate", "too_large", "negative", "empty"])
def test_bad_sources_raise(sources):
    with pytest.raises(ValueError):
        make_engine(graph("rmat")).run(sources)


def test_bad_width_raises():
    with pytest.raises(ValueError, match="width"):
        make_engine(graph("rmat"), 48)


@pytest.mark.parametrize("hub", [63, (1 << 20) + 1])
def test_bad_hub_raises(hub, monkeypatch):
    monkeypatch.setenv("LUX_BCB_HUB", str(hub))
    with pytest.raises(ValueError, match="LUX_BCB_HUB"):
        make_engine(graph("rmat"))


def test_two_parts_raise():
    part = GraphPart(DeviceCSC.from_host(graph("rmat"), "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        BatchedBCEngine(part)


# ---- 6. app ----

def test_bc_app_batch_check(capsys):
    from lux_amd.apps import bc
    bc.main(["-start", "0", "-nsrc", "20", "-batch", "16", "-synthetic",
             "rmat:12:300000", "-check"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] bc: batch 16" in out
    assert "phases bfs/order/sigma/delta/reduce" in out
    assert "[PASS] 0 mistakes" in out
