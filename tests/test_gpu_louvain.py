"""GPU Louvain (LouvainEngine, src/gpu/louvain.hip) against the exact CPU
oracle cpu_ref.louvain: the hand cases, a star ladder taking one decision
through every row role, RMAT-12, planted blocks, engine behaviour and the app.
Labels and traces are integers: every comparison is equality."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.louvain_engine import LouvainEngine  # noqa: E402
from test_lpa_cpu import CASES, clique, graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("LUX_LOUVAIN_HUB", "LUX_LOUVAIN_TABLE", "LUX_LOUVAIN_FUSE")
SMALL = dict(LUX_LOUVAIN_HUB=64, LUX_LOUVAIN_TABLE=64)


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def make_engine(g, monkeypatch=None, order="degree", weighted=False, **knobs):
    for name, val in knobs.items():
        monkeypatch.setenv(name, str(val))
    return LouvainEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0),
                         order=order, weighted=weighted)


def host(t):
    return t.cpu().numpy()


def assert_like_oracle(eng, want, **solve):
    labels, levels, sweeps = want
    got = host(eng.solve(**solve))
    assert got.dtype == np.int32
    assert np.array_equal(got, labels)
    assert eng.level_trace == levels and eng.sweep_trace == sweeps
    assert eng.levels() == len(levels)
    assert eng.num_communities() == int(labels.max()) + 1
    assert np.array_equal(host(eng.sizes()), np.bincount(labels))
    assert eng.modularity() == (float(Fraction(levels[-1][4], eng.W ** 2))
                                if eng.W else 0.0)


# ---- 1. hand cases ----

@pytest.mark.parametrize("fuse", [0, None], ids=["nofuse", "fuse"])
@pytest.mark.parametrize("order", ["degree", "id"])
@pytest.mark.parametrize("name", CASES)
def test_hand_cases(name, order, fuse, monkeypatch):
    g = CASES[name][0]
    eng = make_engine(g, monkeypatch, order,
                      **({} if fuse is None else {"LUX_LOUVAIN_FUSE": fuse}))
    assert_like_oracle(eng, cpu_ref.louvain(g, order))
    assert eng.check() == 0
    assert (eng.stats["fused_classes"] > 0) == (fuse is None)
    assert eng.stats["host_reads"] >= eng.stats["sweeps"]


# ---- 2. star ladder: the centre's decision through every role ----

HUB = 1024  # the default knob, asserted below
LADDER = [({}, d) for d in (1, 2, 15, 16, 17, 63, 64, 65, HUB - 1, HUB,
                            HUB + 1, 9000)] + \
         [(SMALL, d) for d in (65, 127, 128, 129, 1000)]
A, B = 2, 3


def star(d, pattern, own):
    """(graph, init, anchor): the star 0 - 1..d plus seven outside vertices.
    d + 1, d + 2 and d + 3 are isolated anchors of the communities A, B and
    d + 3: they have k = 0 and never move, so the centre chose community c
    iff it ends with the label of c's anchor. d + 4 - d + 5 is the outside
    pair. Leaves of one community have equal k, so tot is a times that."""
    nv, j = d + 8, max(1, d // 4)
    weight, pair = [1] * d, None
    if d == 1:  # the only neighbour's community
        leaves, win = [A], A
    elif pattern == "tie":  # equal a, equal tot: the smaller id, or own
        leaves = [A] * j + [B] * j + list(range(4, 4 + d - 2 * j))
        win = B if own else A
    elif pattern == "heavy":  # equal a, A carries the pair's tot
        leaves = [A] * j + [B] * j + list(range(4, 4 + d - 2 * j))
        win, pair = B, A
    elif pattern == "late":  # the largest id twice, every other id once
        leaves, win = list(range(4, 2 + d)) + [d + 3] * 2, d + 3
    else:  # weights: jb < ja leaves, but of weight 2^20 each
        jb = min(j, 512)
        ja = jb + 1 if d >= 3 else 1
        leaves = [A] * ja + [B] * jb + list(range(4, 4 + d - ja - jb))
        weight = [1] * ja + [1 << 20] * jb + [1] * (d - ja - jb)
        win = B
    assert len(leaves) == d == len(weight)
    perm = np.random.default_rng(d).permutation(d)
    src = np.array([0] * d + [d + 4], np.uint32)
    dst = np.array((1 + perm).tolist() + [d + 5], np.uint32)
    g = Graph.from_edges(nv, src, dst, np.array(weight + [1], np.int32))
    init = np.arange(nv, dtype=np.int32)
    init[1 + perm] = leaves
    init[d + 1], init[d + 2] = A, B
    if pair is not None:
        init[d + 4] = init[d + 5] = pair
    init[0] = B if own and d > 1 else 0
    return g, init, {A: d + 1, B: d + 2, d + 3: d + 3}[win]


@pytest.mark.parametrize("own", [False, True], ids=["absent", "present"])
@pytest.mark.parametrize(
    "knobs,d,pattern",
    [(k, d, p) for k, d in LADDER
     for p in ("tie", "heavy", "late", "weights") if d >= 2 or p == "tie"],
    ids=lambda x: "small" if x == SMALL else "default" if x == {} else str(x))
def test_star_ladder(knobs, d, pattern, own, monkeypatch):
    assert ng.louvain_const("hub_default") == HUB
    g, init, anchor = star(d, pattern, own)
    weighted = pattern == "weights"
    want = cpu_ref.louvain(g, weighted=weighted, init=init, max_sweeps=1,
                           max_levels=1)
    assert want[0][0] == want[0][anchor]
    assert sum(want[0][0] == want[0][a] for a in (d + 1, d + 2, d + 3)) == 1
    eng = make_engine(g, monkeypatch, weighted=weighted, **knobs)
    assert_like_oracle(eng, want, init=torch.from_numpy(init), max_sweeps=1,
                       max_levels=1)
    limit = eng.hub
    assert limit == (64 if knobs else HUB)
    half = eng.table // 2
    assert eng.stats["hub_rows"] == (d > limit)
    assert eng.stats["hub_items"] == (-(-d // half) if d > limit else 0)
    with pytest.raises(ValueError, match="max_levels"):
        eng.check()


# ---- 3. RMAT-12 ----

@pytest.fixture(scope="module")
def rmat():
    """{(sym, order, weighted): (graph, oracle result)}, computed once."""
    out = {}
    for sym in (False, True):
        g = Graph.rmat(12, 40000, seed=7, sym=sym)
        for order in ("degree", "hash"):
            out[sym, order, False] = (g, cpu_ref.louvain(g, order))
    g = Graph.rmat(12, 40000, seed=7)
    g.hash_weights(16)
    out[False, "degree", True] = (g, cpu_ref.louvain(g, weighted=True))
    return out


@pytest.mark.parametrize("knobs", [{}, dict(SMALL, LUX_LOUVAIN_FUSE=0)],
                         ids=["default", "small"])
@pytest.mark.parametrize(
    "sym,order,weighted",
    [(s, o, False) for s in (False, True) for o in ("degree", "hash")] +
    [(False, "degree", True)])
def test_rmat(rmat, sym, order, weighted, knobs, monkeypatch):
    g, want = rmat[sym, order, weighted]
    eng = make_engine(g, monkeypatch, order, weighted, **knobs)
    assert_like_oracle(eng, want)
    print(eng.stats, eng.phase_ms)
    assert eng.check() == 0 and eng.levels() >= 2
    assert eng.stats["host_reads"] >= eng.stats["sweeps"]
    if knobs:
        assert eng.stats["hub_rows"] > 0 and eng.stats["fused_classes"] == 0


# ---- 4. planted blocks ----

def test_planted_blocks(monkeypatch):
    rng = np.random.default_rng(11)
    a, b = np.triu_indices(32, 1)
    keep = [rng.random(a.size) < 0.5 for _ in range(8)]
    edges = np.concatenate(
        [np.stack([a[k] + 32 * i, b[k] + 32 * i], 1)
         for i, k in enumerate(keep)] + [rng.integers(0, 256, (200, 2))])
    g = graph(256, edges)
    eng = make_engine(g, monkeypatch)
    want = cpu_ref.louvain(g)
    assert_like_oracle(eng, want)
    print(eng.num_communities(), eng.modularity())
    assert eng.modularity() == float(Fraction(eng.qnum(), eng.W ** 2))
    assert eng.check() == 0


# ---- 5. engine behaviour ----

def test_arguments_are_validated(monkeypatch):
    g = CASES["two_k5"][0]

    def part(nparts=1, weight=None):  # a GraphPart takes its DeviceCSC over
        csc = DeviceCSC.from_host(g, "cuda")
        if weight is not None:
            csc.weight = torch.full((g.ne,), weight, dtype=torch.int32,
                                    device="cuda")
        return GraphPart(csc, nparts, 0)

    with pytest.raises(ValueError, match="single-rank"):
        LouvainEngine(part(2))
    for name, bad in (("LUX_LOUVAIN_HUB", 63), ("LUX_LOUVAIN_TABLE", 96),
                      ("LUX_LOUVAIN_TABLE", 32768), ("LUX_LOUVAIN_FUSE", -1)):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            LouvainEngine(part())
        monkeypatch.delenv(name)
    with pytest.raises(ValueError, match="part.weight"):
        LouvainEngine(part(), weighted=True)
    with pytest.raises(ValueError, match=">= 1"):
        LouvainEngine(part(weight=0), weighted=True)
    with pytest.raises(ValueError, match="32 bits"):  # W = 2 * 21 * 2^27
        LouvainEngine(part(weight=1 << 27), weighted=True)
    eng = LouvainEngine(part())
    for bad in (torch.zeros(9, dtype=torch.int32), torch.zeros(10),
                torch.full((10,), 10), torch.full((10,), -1)):
        with pytest.raises(ValueError, match="init"):
            eng.solve(init=bad)


def test_check_sees_an_overwritten_label():
    """K6 - K5 - K4 in a chain end as three coarse vertices of k = 31, 22,
    13 and W = 66. With the first two merged by hand, vertex 1 scores
    66 - 22 * 31 for staying and 66 - 22 * 13 for community 2: one mover."""
    g = graph(15, clique(range(6)) + clique(range(6, 11)) +
              clique(range(11, 15)) + [(5, 6), (10, 11)])
    eng = make_engine(g)
    assert host(eng.labels()).tolist() == [0] * 6 + [1] * 5 + [2] * 4
    assert eng.check() == 0
    eng.level_communities()[1] = 0
    assert eng.check() == 1


# ---- 6. the app ----

def test_app_in_a_child_process():
    r = subprocess.run(
        [sys.executable, "-m", "lux_amd.apps.louvain", "-synthetic",
         "rmat:12:40000", "-check", "-verbose"], cwd=ROOT,
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[PASS] 0 mistakes" in r.stdout and "ELAPSED TIME" in r.stdout
    lines = r.stdout.splitlines()
    rows = lines[lines.index("level,sweep,moved,qnum") + 1:]
    rows = [tuple(map(int, ln.split(","))) for ln in rows if ln[:1].isdigit()]
    assert rows == cpu_ref.louvain(Graph.rmat(12, 40000), "degree")[2]
