"""GPU label propagation (LPAEngine, src/gpu/lpa.hip) against the exact CPU
oracle cpu_ref.label_propagation: the hand cases, a star ladder over every
row role and several hub passes, RMAT-12, planted communities, engine
behaviour and the app. Labels are integers: every comparison is equality."""
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
from lux_amd.lpa_engine import LPAEngine  # noqa: E402
from test_lpa_cpu import CASES, graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("LUX_LPA_HUB", "LUX_LPA_TABLE", "LUX_LPA_FUSE")
SMALL = dict(LUX_LPA_HUB=64, LUX_LPA_TABLE=64)


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def make_engine(g, monkeypatch=None, order="degree", **knobs):
    for name, val in knobs.items():
        monkeypatch.setenv(name, str(val))
    return LPAEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0),
                     order=order)


def host(t):
    return t.cpu().numpy()


def assert_converged_like_oracle(eng, g, order):
    want, trace = cpu_ref.label_propagation(g, order)
    got = host(eng.solve())
    assert got.dtype == np.int32
    assert np.array_equal(got, want)
    assert eng.sweep_trace == trace
    assert eng.converged() and eng.sweeps() == len(trace)
    assert eng.stats["host_reads"] == len(trace)
    assert eng.check() == 0
    return want


# ---- 1. hand cases ----

@pytest.mark.parametrize("fuse", [0, None], ids=["nofuse", "fuse"])
@pytest.mark.parametrize("order", ["degree", "id"])
@pytest.mark.parametrize("name", CASES)
def test_hand_cases(name, order, fuse, monkeypatch):
    g = CASES[name][0]
    eng = make_engine(g, monkeypatch, order,
                      **({} if fuse is None else {"LUX_LPA_FUSE": fuse}))
    want = assert_converged_like_oracle(eng, g, order)
    st = cpu_ref.community_stats(g, want)
    assert eng.intra_edges() == st["intra"] and eng.m == st["m"]
    assert np.array_equal(host(eng.sizes()), st["sizes"])
    assert np.array_equal(host(eng.community_degrees()), st["tot"])
    assert eng.modularity() == st["modularity"]
    assert eng.num_communities() == int((st["sizes"] > 0).sum())
    assert (eng.stats["fused_classes"] > 0) == (fuse is None)


# ---- 2. star ladder ----

HUB = 1024  # the default knob, asserted below
LADDER = [({}, d) for d in (1, 2, 15, 16, 17, 63, 64, 65, HUB - 1, HUB,
                            HUB + 1, 9000)] + \
         [(SMALL, d) for d in (65, 127, 128, 129, 1000)]
A, B = 2, 3


def star_pattern(d, pattern):
    """(leaf labels, the centre's label when it is one of them, the winner
    when it is not, the winner when it is)."""
    if pattern == "tie":  # A and B k times, one label k - 1 times
        k = max(1, d // 4)
        rest = d - (3 * k - 1)
        leaves = [A] * k + [B] * k + [4] * (k - 1) + list(range(5, 5 + rest))
        return leaves, B, A, B
    if pattern == "late":  # the largest label twice
        leaves = list(range(2, d + 1)) + [d]
        return leaves, 2, d, d
    return list(range(2, d + 2)), 7 if d > 7 else 2, 2, 7 if d > 7 else 2


@pytest.mark.parametrize("own", ["absent", "present"])
@pytest.mark.parametrize(
    "knobs,d,pattern",
    [(k, d, p) for k, d in LADDER for p in ("tie", "late", "distinct")
     if d >= 2 or p == "distinct"],
    ids=lambda x: "small" if x == SMALL else "default" if x == {} else str(x))
def test_star_ladder(knobs, d, pattern, own, monkeypatch):
    assert ng.lpa_hub_default() == HUB
    leaves, present, win_absent, win_present = star_pattern(d, pattern)
    assert len(leaves) == d
    nv = d + 8
    g = graph(nv, [(0, i) for i in range(1, d + 1)])
    init = np.arange(nv, dtype=np.int32)
    init[1:d + 1] = np.random.default_rng(d).permutation(leaves)
    init[0] = present if own == "present" else 0
    want, trace = cpu_ref.label_propagation(g, "degree", init=init,
                                            max_sweeps=1)
    assert want[0] == (win_present if own == "present" else win_absent)
    eng = make_engine(g, monkeypatch, **knobs)
    got = host(eng.solve(init=torch.from_numpy(init), max_sweeps=1))
    assert np.array_equal(got, want)
    assert eng.sweep_trace == trace
    limit = eng.hub
    assert limit == (64 if knobs else HUB)
    half = eng.table // 2
    assert eng.stats["hub_rows"] == (d > limit)
    assert eng.stats["hub_items"] == (-(-d // half) if d > limit else 0)


# ---- 3. RMAT-12 ----

@pytest.fixture(scope="module")
def rmat():
    return {sym: Graph.rmat(12, 40000, seed=7, sym=sym)
            for sym in (False, True)}


@pytest.mark.parametrize("knobs", [{}, dict(SMALL, LUX_LPA_FUSE=0)],
                         ids=["default", "small"])
@pytest.mark.parametrize("order", ["degree", "hash"])
@pytest.mark.parametrize("sym", [False, True], ids=["directed", "sym"])
def test_rmat(rmat, sym, order, knobs, monkeypatch):
    eng = make_engine(rmat[sym], monkeypatch, order, **knobs)
    assert_converged_like_oracle(eng, rmat[sym], order)
    print(eng.stats, eng.phase_ms)
    if knobs:
        assert eng.stats["hub_rows"] > 0 and eng.stats["fused_classes"] == 0


# ---- 4. planted communities ----

def test_planted_communities(monkeypatch):
    rng = np.random.default_rng(11)
    a, b = np.triu_indices(32, 1)
    keep = [rng.random(a.size) < 0.5 for _ in range(8)]
    edges = np.concatenate(
        [np.stack([a[k] + 32 * i, b[k] + 32 * i], 1)
         for i, k in enumerate(keep)] + [rng.integers(0, 256, (200, 2))])
    g = graph(256, edges)
    eng = make_engine(g, monkeypatch)
    want = assert_converged_like_oracle(eng, g, "degree")
    st = cpu_ref.community_stats(g, want)
    print(eng.num_communities(), eng.modularity())
    assert eng.modularity() == st["modularity"]
    assert eng.intra_edges() == st["intra"]


# ---- 5. engine behaviour ----

def test_arguments_are_validated(monkeypatch):
    g = CASES["two_k5"][0]

    def part(nparts=1):  # a GraphPart takes its DeviceCSC over
        return GraphPart(DeviceCSC.from_host(g, "cuda"), nparts, 0)

    with pytest.raises(ValueError, match="single-rank"):
        LPAEngine(part(2))
    for name, bad in (("LUX_LPA_HUB", 63), ("LUX_LPA_TABLE", 96),
                      ("LUX_LPA_TABLE", 32768), ("LUX_LPA_FUSE", -1)):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            LPAEngine(part())
        monkeypatch.delenv(name)
    eng = LPAEngine(part())
    for bad in (torch.zeros(9, dtype=torch.int32), torch.zeros(10),
                torch.full((10,), 10), torch.full((10,), -1)):
        with pytest.raises(ValueError, match="init"):
            eng.solve(init=bad)


def test_one_sweep_is_not_converged(rmat):
    eng = make_engine(rmat[True])
    eng.solve(max_sweeps=1)
    assert eng.converged() is False and eng.sweeps() == 1
    with pytest.raises(ValueError, match="did not converge"):
        eng.check()


def test_check_sees_an_overwritten_label():
    eng = make_engine(graph(5, [(a, b) for a in range(5)
                                for b in range(a + 1, 5)]))
    lab = eng.labels()
    common = int(lab[0].item())
    assert host(lab).tolist() == [common] * 5 and eng.check() == 0
    lab[3] = (common + 1) % 5  # 3 disagrees with all; the others keep 3 of 4
    assert eng.check() == 1


# ---- 6. the app ----

def test_app_in_a_child_process():
    r = subprocess.run(
        [sys.executable, "-m", "lux_amd.apps.lpa", "-synthetic",
         "rmat:12:40000", "-check", "-verbose"], cwd=ROOT,
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[PASS] 0 mistakes" in r.stdout and "ELAPSED TIME" in r.stdout
    lines = r.stdout.splitlines()
    rows = lines[lines.index("sweep,evaluated,changed") + 1:]
    rows = [tuple(map(int, ln.split(","))) for ln in rows if ln[:1].isdigit()]
    _, trace = cpu_ref.label_propagation(Graph.rmat(12, 40000), "degree")
    assert rows == trace
