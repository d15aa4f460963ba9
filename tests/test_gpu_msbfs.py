"""GPU multi-source BFS (MSBFSEngine, src/gpu/msbfs.hip) against the CPU
oracle cpu_ref.multi_source_stats: the hand cases, a star ladder over every
row role in both directions, a deep path, the direction rule, RMAT-12 in one
and two batches, engine behaviour and the app. Every integer comparison is
equality; harmonic is held to the rounding bound of its definition."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.msbfs_engine import MSBFSEngine  # noqa: E402
from test_msbfs_cpu import CASES, graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("LUX_MSBFS_HUB", "LUX_MSBFS_PULL_DIV", "LUX_MSBFS_DIR")
DIRS = ("auto", "push", "pull")
_oracle = {}


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def oracle(g, sources):
    """Computed once per (graph, sources); the graph is kept so that its id
    stays its own."""
    key = (id(g), tuple(sources))
    if key not in _oracle:
        _oracle[key] = (g, cpu_ref.multi_source_stats(g, sources, div=8))
    return _oracle[key][1]


def make_engine(g, monkeypatch=None, direction="auto", **knobs):
    for name, val in dict(knobs, LUX_MSBFS_DIR=direction).items():
        monkeypatch.setenv(name, str(val))
    return MSBFSEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))


def host(t):
    return t.cpu().numpy()


def assert_like_oracle(eng, g, sources):
    want = oracle(g, sources)
    assert host(eng.run(sources, depths=True)).tolist() == \
        want["dist_sum"].tolist()
    assert np.array_equal(host(eng.depths()), want["depths"])
    bits = np.unpackbits(host(eng.seen()).view(np.uint8), axis=1)
    reach = bits.reshape(-1, g.nv, 64).sum((0, 2))
    assert np.array_equal(reach, want["reach"])
    assert np.array_equal(host(eng.reach()), want["reach"])
    assert eng.level_counts() == want["level_counts"]
    for key in ("reached", "farness", "eccentricity", "closeness"):
        assert getattr(eng, key)().tolist() == want[key].tolist(), key
    forced = eng.direction != "auto"
    assert eng.level_trace == [
        t[:2] + (eng.direction if forced else t[2],) + t[3:]
        for t in want["level_trace"]]
    st = eng.stats
    assert st["host_reads"] == st["levels"] == len(want["level_trace"])
    assert st["levels"] == st["push_levels"] + st["pull_levels"]
    assert eng.check() == 0
    got, ref = host(eng.harmonic()), want["harmonic"]
    err = np.abs(got - ref).max() / max(ref.max(), 1.0)
    print("harmonic max rel err", err, "levels", st["levels"])
    assert np.all(np.abs(got - ref) <= 2 * (st["levels"] + 1) * 2.0 ** -53
                  * ref)
    return st


# ---- 1. hand cases ----

@pytest.mark.parametrize("nsrc", [1, 2, 64])
@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("name", CASES)
def test_hand_cases(name, direction, nsrc, monkeypatch):
    g, sources, _ = CASES[name]
    sources = (sources + [v for v in range(g.nv) if v not in sources])[:nsrc]
    assert_like_oracle(make_engine(g, monkeypatch, direction), g, sources)


# ---- 2. star ladder ----

HUB = 1024  # the default knob, asserted below
LADDER = [({}, d) for d in (1, 15, 16, 17, 63, 64, 65, HUB - 1, HUB, HUB + 1,
                            3 * HUB + 5)] + \
         [(dict(LUX_MSBFS_HUB=64), d) for d in (65, 127, 128, 129, 1000)]


def star(kind, d):
    """(graph, sources, hub rows in, hub rows out) as multiples of
    d > limit."""
    if kind == "out":  # centre 0 -> leaves 1..d -> sink d + 1
        edges = [(0, i) for i in range(1, d + 1)] + \
                [(i, d + 1) for i in range(1, d + 1)]
        return graph(d + 2, edges), [0, 1, d + 1], 1, 1
    # leaves 1..d -> centre 0 -> tail d + 1 -> fillers
    fill = list(range(d + 2, d + 2 + max(0, 64 - d)))
    edges = [(i, 0) for i in range(1, d + 1)] + [(0, d + 1)] + \
            [(d + 1, f) for f in fill]
    n = min(d, 64)
    leaves = list(range(d - n + 1, d + 1)) if kind == "in" else \
        list(range(1, n + 1))
    return graph(d + 2 + len(fill), edges), leaves + fill, 1, 0


@pytest.mark.parametrize("direction", ["push", "pull"])
@pytest.mark.parametrize("kind", ["in", "saturated_first", "out"])
@pytest.mark.parametrize("knobs,d", LADDER,
                         ids=lambda x: str(x) if isinstance(x, int) else
                         "small" if x else "default")
def test_star_ladder(knobs, d, kind, direction, monkeypatch):
    assert ng.msbfs_hub_default() == HUB and ng.msbfs_thread_limit() == 16
    g, sources, hub_in, hub_out = star(kind, d)
    assert len(sources) == (3 if kind == "out" else 64)
    eng = make_engine(g, monkeypatch, direction, **knobs)
    st = assert_like_oracle(eng, g, sources)
    assert eng.hub == (64 if knobs else HUB)
    assert st["hub_rows_in"] == hub_in * (d > eng.hub)
    assert st["hub_rows_out"] == hub_out * (d > eng.hub)


# ---- 3. deep path, 4. direction rule ----

def test_deep_path(monkeypatch):
    g = graph(300, [(i, i + 1) for i in range(299)])
    st = assert_like_oracle(make_engine(g, monkeypatch), g, [0, 1, 299])
    assert st["levels"] == 300


def test_direction_rule_on_a_broom(monkeypatch):
    """p0..p4 -> c -> 2000 leaves -> q0..q4, ne = 4009: with div = 8 a
    frontier is pulled iff its volume exceeds 501, which holds for c and for
    the leaves and for nothing on the two paths."""
    c, leaves = 5, range(6, 2006)
    edges = [(i, i + 1) for i in range(5)] + [(c, v) for v in leaves] + \
        [(v, 2006) for v in leaves] + [(2006 + i, 2007 + i) for i in range(4)]
    g = graph(2011, edges)
    eng = make_engine(g, monkeypatch)
    st = assert_like_oracle(eng, g, [0, 1])
    dirs = "".join(t[2][2] for t in eng.level_trace)  # s = push, l = pull
    assert dirs.strip("s") == "l" * st["pull_levels"] and \
        dirs[0] == dirs[-1] == "s"
    assert st["push_levels"] > 0 and st["pull_levels"] > 0


# ---- 5. RMAT-12 ----

@pytest.fixture(scope="module")
def rmat():
    return {sym: Graph.rmat(12, 40000, seed=7, sym=sym)
            for sym in (False, True)}


@pytest.mark.parametrize("nsrc", [64, 100])
@pytest.mark.parametrize("knobs", [{}, dict(LUX_MSBFS_HUB=64)],
                         ids=["default", "small"])
@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("sym", [False, True], ids=["directed", "sym"])
def test_rmat(rmat, sym, direction, knobs, nsrc, monkeypatch):
    eng = make_engine(rmat[sym], monkeypatch, direction, **knobs)
    st = assert_like_oracle(eng, rmat[sym], list(range(nsrc)))
    print(st, eng.phase_ms)
    assert eng.seen().shape == ((nsrc + 63) // 64, rmat[sym].nv)
    if knobs:
        assert st["hub_rows_in"] > 0 and st["hub_rows_out"] > 0


# ---- 6. engine behaviour ----

def test_arguments_are_validated(monkeypatch):
    g = CASES["cycle4"][0]

    def part(nparts=1):  # a GraphPart takes its DeviceCSC over
        return GraphPart(DeviceCSC.from_host(g, "cuda"), nparts, 0)

    with pytest.raises(ValueError, match="single-rank"):
        MSBFSEngine(part(2))
    for name, bad in (("LUX_MSBFS_HUB", 0), ("LUX_MSBFS_HUB", (1 << 20) + 1),
                      ("LUX_MSBFS_PULL_DIV", 0), ("LUX_MSBFS_DIR", "up")):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            MSBFSEngine(part())
        monkeypatch.delenv(name)
    eng = MSBFSEngine(part())
    for bad in ([], [0, 0], [4], [-1], [0, 1, 2, 3, 1]):
        with pytest.raises(ValueError, match="sources"):
            eng.run(bad)
    eng.run([0])
    with pytest.raises(ValueError, match="depths"):
        eng.depths()


@pytest.mark.parametrize("depths", [False, True])
def test_check_sees_a_cleared_seen_bit(depths, monkeypatch):
    g = CASES["path5"][0]
    eng = make_engine(g, monkeypatch)
    eng.run([0], depths=depths)
    assert eng.check() == 0
    eng.seen()[0, 2] = 0  # 1 -> 2 with 1 reached; 2 is no source
    assert eng.check() == (2 if depths else 1)  # the edge, and the sign


# ---- 7. the app ----

def test_app_in_a_child_process():
    r = subprocess.run(
        [sys.executable, "-m", "lux_amd.apps.msbfs", "-synthetic",
         "rmat:12:40000", "-nsrc", "100", "-check", "-verbose"], cwd=ROOT,
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[PASS] 0 mistakes" in r.stdout and "ELAPSED TIME" in r.stdout
    lines = r.stdout.splitlines()
    head = "batch,level,direction,frontier,volume,new_pairs"
    rows = [ln.split(",") for ln in lines[lines.index(head) + 1:]
            if ln[:1].isdigit()]
    rows = [(int(r[0]), int(r[1]), r[2]) + tuple(map(int, r[3:]))
            for r in rows]
    want = oracle(Graph.rmat(12, 40000), list(range(100)))
    assert rows == want["level_trace"]
