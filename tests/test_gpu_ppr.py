"""GPU personalised PageRank (PPREngine, src/gpu/ppr.hip) against the fp64
oracle cpu_ref.personalised_pagerank: a degree ladder over every row role
held to equality, hand cases and RMAT-12 held to the rounding bound of the
recurrence, the tol run, argument validation, check() and the app."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.ppr_engine import PPREngine  # noqa: E402
from test_msbfs_cpu import CASES, graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_oracle = {}


def oracle(g, seeds, damping, iters):
    """Computed once per input; the graph is kept so that its id stays its
    own."""
    key = (id(g), repr(seeds), damping, iters)
    if key not in _oracle:
        _oracle[key] = (g, cpu_ref.personalised_pagerank(g, seeds, damping,
                                                         iters))
    return _oracle[key][1]


def make_engine(g, monkeypatch, hub=None):
    monkeypatch.delenv("LUX_PPR_HUB", raising=False)
    if hub:
        monkeypatch.setenv("LUX_PPR_HUB", str(hub))
    return PPREngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))


def bound(g, iters):
    """Every operation is on non-negative numbers, so the relative errors
    add up without cancellation: a row of n entries takes n roundings for
    its sum and fewer than 6 for the scaling, the teleport and the stored
    form, 2^-24 each, and an iteration inherits the error of the one before;
    the factor 2 covers the second-order terms."""
    indeg = np.diff(np.concatenate(([0], g.col_end)).astype(np.int64)).max()
    return 2 * iters * (int(indeg) + 6) * 2.0 ** -24


def assert_like_oracle(eng, g, seeds, iters, damping=0.85, exact=False):
    want, n, res = oracle(g, seeds, damping, iters)
    got = eng.run(seeds, iters=iters, damping=damping)
    assert got.shape == (g.nv, len(seeds)) and eng.iterations() == \
        [iters] * ((len(seeds) + 63) // 64)
    again = eng.run(seeds, iters=iters, damping=damping).clone()
    assert torch.equal(got, again)
    assert eng.check() == 0
    got = got.cpu().numpy()
    if exact:
        assert np.array_equal(got, want.astype(np.float32))
    else:
        rel = np.abs(got - want) / np.maximum(want, 1e-300)
        print("max rel err", rel.max(), "bound", bound(g, iters))
        assert np.all(np.abs(got - want) <= bound(g, iters) * want + 1e-30)
    trace = np.array(eng.residual_trace[-1])
    assert trace.shape == (iters,) and eng.stats["host_reads"] == 0
    return eng.stats


# ---- 1. exact ladder ----

HUB = 1024  # the default knob, asserted below
LADDER = [(None, d) for d in (0, 1, 7, 8, 9, 63, 64, 65, HUB - 1, HUB,
                              HUB + 1, 3 * HUB + 5)] + \
         [(64, d) for d in (65, 127, 128, 129, 1000)]


def ladder(deg, K):
    """Leaves 1..deg -> centre 0 -> tail deg + 1, then 2^k isolated
    fillers; column c is seeded on its 2^k leaves, or fillers where the
    leaves run out."""
    size = 1
    while K * size < deg:
        size *= 2
    fill = list(range(deg + 2, deg + 2 + size))
    seeds = []
    for c in range(K):
        own = list(range(c * size + 1, min((c + 1) * size, deg) + 1))
        seeds.append(own + fill[:size - len(own)])
    edges = [(i, 0) for i in range(1, deg + 1)] + [(0, deg + 1)]
    return graph(deg + 2 + size, edges), seeds


@pytest.mark.parametrize("K", [16, 32, 64])
@pytest.mark.parametrize("hub,deg", LADDER)
def test_exact_ladder(hub, deg, K, monkeypatch):
    assert ng.ppr_group_limit() == 8 and ng.ppr_hub_default() == HUB
    g, seeds = ladder(deg, K)
    assert all(len(s) == len(seeds[0]) for s in seeds)
    eng = make_engine(g, monkeypatch, hub)
    st = assert_like_oracle(eng, g, seeds, 2, damping=0.5, exact=True)
    assert eng.hub == (hub or HUB) and st["width"] == K
    assert st["hub_rows"] == (deg > eng.hub)
    assert st["launches"] == 2 + 2 * (1 + st["hub_rows"])


# ---- 2. hand cases and RMAT-12 ----

@pytest.fixture(scope="module")
def graphs():
    out = {name: case[0] for name, case in CASES.items()}
    out["directed"] = Graph.rmat(12, 40000, seed=7)
    out["sym"] = Graph.rmat(12, 40000, seed=7, sym=True)
    return out


def mixed_seeds(g, K):
    """One-hot columns and, from two columns on, one multi-vertex set."""
    seeds = [c % g.nv for c in range(K)]
    if K > 1:
        seeds[-1] = [0, g.nv // 2, g.nv - 1]
    return seeds


@pytest.mark.parametrize("K", [1, 16, 17, 33, 64, 100])
@pytest.mark.parametrize("name,hub", [(n, None) for n in CASES] + [
    ("directed", None), ("directed", 64), ("sym", None), ("sym", 64)])
def test_against_the_oracle(graphs, name, hub, K, monkeypatch):
    g = graphs[name]
    eng = make_engine(g, monkeypatch, hub)
    st = assert_like_oracle(eng, g, mixed_seeds(g, K), 10)
    assert st["width"] == (64 if K > 32 else 32 if K > 16 else 16)
    if hub and name in ("directed", "sym"):
        assert st["hub_rows"] > 0


# ---- 3. tol ----

def test_tol_stops_at_the_first_small_residual(graphs, monkeypatch):
    g, seeds, tol = graphs["directed"], [5, [1, 2, 3], 4000], 1e-6
    eng = make_engine(g, monkeypatch)
    got = eng.run(seeds, iters=500, tol=tol).cpu().numpy()
    (n,), (trace,) = eng.iterations(), eng.residual_trace
    assert 1 < n < 500 and len(trace) == n
    assert trace[-1] <= tol and min(trace[:-1]) > tol
    assert eng.stats["host_reads"] == n
    want = oracle(g, seeds, 0.85, n)[0]
    assert np.all(np.abs(got - want) <= bound(g, n) * want + 1e-30)
    eng.run(seeds, iters=3)
    assert eng.stats["host_reads"] == 0


# ---- 4. arguments ----

def test_arguments_are_validated(monkeypatch):
    g = CASES["cycle4"][0]

    def part(nparts=1):  # a GraphPart takes its DeviceCSC over
        return GraphPart(DeviceCSC.from_host(g, "cuda"), nparts, 0)

    monkeypatch.delenv("LUX_PPR_HUB", raising=False)
    with pytest.raises(ValueError, match="single-rank"):
        PPREngine(part(2))
    for bad in (63, (1 << 20) + 1):
        monkeypatch.setenv("LUX_PPR_HUB", str(bad))
        with pytest.raises(ValueError, match="LUX_PPR_HUB"):
            PPREngine(part())
    monkeypatch.delenv("LUX_PPR_HUB")
    eng = PPREngine(part())
    with pytest.raises(ValueError, match="no result"):
        eng.ranks()
    for bad in ([], [[]], [0, []], [4], [-1], [[0, 1, 0]], [0, [1, 4]]):
        with pytest.raises(ValueError, match="seeds"):
            eng.run(bad)
    for kw, match in ((dict(damping=0.0), "damping"),
                      (dict(damping=1.0), "damping"),
                      (dict(damping=-0.5), "damping"),
                      (dict(iters=0), "iters"), (dict(tol=-1e-3), "tol")):
        with pytest.raises(ValueError, match=match):
            eng.run([0], **kw)
    assert eng.run([0, [1, 2]], iters=4).shape == (4, 2)
    values, vertices = eng.topk(2)
    assert values.shape == vertices.shape == (2, 2)


# ---- 5. check() ----

def test_check_sees_one_halved_entry(graphs, monkeypatch):
    eng = make_engine(graphs["sym"], monkeypatch)
    eng.run(list(range(20)), iters=3)
    assert eng.check() == 0 and eng.state().shape == (4096, 32)
    assert float(eng.state()[7, 7]) > 0.0  # the teleport of column 7
    eng.state()[7, 7] *= 0.5
    assert eng.check() == 1


# ---- 6. the app ----

def test_app_in_a_child_process():
    r = subprocess.run(
        [sys.executable, "-m", "lux_amd.apps.ppr", "-synthetic",
         "rmat:12:40000", "-nsrc", "100", "-ni", "10", "-check", "-verbose",
         "-top", "3"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[PASS] 0 mistakes" in r.stdout and "ELAPSED TIME" in r.stdout
    lines = r.stdout.splitlines()
    g = Graph.rmat(12, 40000)
    rows = [ln.split(",") for ln in
            lines[lines.index("batch,iteration,residual") + 1:]
            if ln[:1].isdigit()]
    assert [(int(b), int(i)) for b, i, _ in rows] == \
        [(b, i) for b in range(2) for i in range(10)]
    for b, cols in enumerate((range(64), range(64, 100))):
        want = oracle(g, list(cols), 0.85, 10)[2]
        got = np.array([float(x) for _, _, x in rows[10 * b:10 * b + 10]])
        print("residuals", got, want)
        assert np.all(np.abs(got - want) <= bound(g, 10) * np.array(want))
    top = [ln.split()[2:] for ln in lines if ln.startswith("[lux] source ")]
    assert len(top) == 100 and all(len(t) == 4 for t in top)
    want = np.concatenate([oracle(g, list(cols), 0.85, 10)[0] for cols in
                           (range(64), range(64, 100))], axis=1)
    for c, t in enumerate(top):
        first, second = np.sort(want[:, c])[-1:-3:-1]
        if first - second > 2 * bound(g, 10) * first:  # no tie by value
            assert int(t[1].split(":")[0]) == int(want[:, c].argmax()), c
