"""GPU k-core decomposition (KCoreEngine, src/gpu/kcore.hip) against the
exact CPU oracle cpu_ref.coreness: the hand cases (cascade, under-run and
restore, hub role, level jump), the hub ladder at the default KCORE_HUB and
at LUX_KCORE_HUB=64, a symmetric and a directed RMAT-12 with their pinned
values, the removal order, engine behaviour and the app. Coreness is an
integer per vertex: every comparison is equality, and levels and rounds
equal kcore_ref.sync_peel's with the round fusion off and on."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kcore_ref  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.kcore_engine import KCoreEngine  # noqa: E402

KNOBS = ("LUX_KCORE_HUB", "LUX_KCORE_FUSE")
FUSE = pytest.mark.parametrize("fuse", [0, None], ids=["nofuse", "fuse"])


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
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def make_engine(g, monkeypatch=None, fuse=None, hub=None):
    for name, val in zip(KNOBS, (hub, fuse)):
        if val is not None:
            monkeypatch.setenv(name, str(val))
    return KCoreEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))


def host(t):
    return t.cpu().numpy()


_REF = {}


def reference(name, g):
    """(oracle coreness, sync_peel levels, sync_peel rounds), computed once
    per graph and shared."""
    if name not in _REF:
        want = cpu_ref.coreness(g)
        core, levels, rounds = kcore_ref.sync_peel(g)
        assert np.array_equal(want, core)
        want.setflags(write=False)
        _REF[name] = (want, levels, rounds)
    return _REF[name]


def assert_decomposition(eng, want, levels, rounds):
    got = host(eng.decompose())
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    st = eng.stats
    print(st, eng.phase_ms)
    assert st["levels"] == levels
    assert st["rounds"] == rounds
    # at most two scans and two reads for them per level, one read a launch
    assert levels <= st["scans"] <= 2 * levels
    assert st["host_reads"] <= st["scans"] + rounds
    if eng.fuse == 0:
        assert st["fused_rounds"] == 0
        assert st["host_reads"] == st["scans"] + rounds
    assert eng.check() == 0
    assert eng.degeneracy() == int(want.max(initial=0))


# ---- 1. hand cases ----

@FUSE
@pytest.mark.parametrize("case", kcore_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, fuse, monkeypatch):
    want, levels, rounds = reference(case.name, case.g)
    if case.core is not None:
        assert np.array_equal(want, case.core)
    else:
        assert int(want.max()) == case.degeneracy
    if case.levels is not None:
        assert levels == case.levels
    if case.rounds is not None:
        assert rounds == case.rounds
    eng = make_engine(case.g, monkeypatch, fuse=fuse)
    assert_decomposition(eng, want, levels, rounds)
    st = eng.stats
    if case.name == "path4001" and fuse is None:
        # the cascade is carried by the tail kernel: a read per launch
        assert st["fused_rounds"] == rounds
        assert st["host_reads"] <= 4
    if case.name.startswith("star5000"):
        assert st["max_degree"] >= kcore_ref.STAR_LEAVES > eng.hub
        assert eng.hubcap >= 2


# ---- 2. hub ladder ----

@FUSE
@pytest.mark.parametrize("hub", [None, 64], ids=["default", "hub64"])
def test_hub_ladder(hub, fuse, monkeypatch):
    h = hub if hub is not None else ng.kcore_hub_default()
    lad = kcore_ref.ladder(h)
    want, levels, rounds = reference(f"ladder{h}", lad.g)
    assert np.array_equal(want, lad.core)
    assert np.array_equal(want[lad.rows], lad.degrees)
    # a level per distinct D and one for the pool; every level is one round
    # (a row's neighbours all outlast it, the pool clique goes at once)
    assert levels == rounds == lad.levels
    eng = make_engine(lad.g, monkeypatch, fuse=fuse, hub=hub)
    assert eng.hub == h
    assert_decomposition(eng, want, levels, rounds)
    assert np.array_equal(host(eng.degree)[lad.rows], lad.degrees)
    assert eng.stats["max_degree"] >= 2 * h + 1
    assert eng.hubcap > 0


# ---- 3. RMAT-12 ----

RMAT = {
    True: dict(m=94769, degeneracy=119, innermost=292, total=106337,
               levels=68, rounds=155),
    False: dict(m=160602, degeneracy=178, innermost=293, total=183300,
                levels=83, rounds=173),
}


@pytest.fixture(scope="module")
def rmat():
    out = {}
    for sym in (True, False):
        g = Graph.rmat(12, 300000, seed=3, sym=sym)
        want, levels, rounds = reference(f"rmat12_{sym}", g)
        out[sym] = dict(g=g, want=want, levels=levels, rounds=rounds)
    return out


@FUSE
@pytest.mark.parametrize("hub", [None, 64], ids=["default", "hub64"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "directed"])
def test_rmat(rmat, sym, hub, fuse, monkeypatch):
    r, pin = rmat[sym], RMAT[sym]
    want = r["want"]
    assert r["levels"] == pin["levels"] and r["rounds"] == pin["rounds"]
    assert int(want.max()) == pin["degeneracy"]
    assert int(want.astype(np.int64).sum()) == pin["total"]
    eng = make_engine(r["g"], monkeypatch, fuse=fuse, hub=hub)
    assert_decomposition(eng, want, pin["levels"], pin["rounds"])
    assert eng.stats["simple_edges"] == pin["m"]
    shells = host(eng.shell_sizes())
    assert np.array_equal(shells, np.bincount(want))
    assert int(shells[-1]) == pin["innermost"]
    for k in (0, 1, 8, pin["degeneracy"], pin["degeneracy"] + 1):
        assert int(eng.core(k).sum().item()) == int((want >= k).sum())
    # a second decompose() starts from scratch
    assert np.array_equal(host(eng.decompose()), want)
    assert eng.stats["rounds"] == pin["rounds"]


@FUSE
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "directed"])
def test_order(rmat, sym, fuse, monkeypatch):
    """The removal order is a permutation along which coreness never
    decreases and every vertex has at most coreness[v] later neighbours
    (a degeneracy ordering). Inside a round it is not deterministic."""
    r = rmat[sym]
    g, want = r["g"], r["want"].astype(np.int64)
    eng = make_engine(g, monkeypatch, fuse=fuse)
    order = host(eng.order()).view(np.uint32).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(g.nv))
    assert (np.diff(want[order]) >= 0).all()
    pos = np.empty(g.nv, np.int64)
    pos[order] = np.arange(g.nv)
    ptr, adj = kcore_ref.simple_adjacency(g)
    row = np.repeat(np.arange(g.nv), np.diff(ptr))
    later = np.bincount(row[pos[adj] > pos[row]], minlength=g.nv)
    assert (later <= want).all()


# ---- 4. engine behaviour ----

def test_check_sees_a_corrupted_entry(rmat):
    eng = make_engine(rmat[True]["g"])
    core = eng.coreness()
    assert eng.check() == 0
    v = int(np.argmax(rmat[True]["want"]))
    keep = core[v].clone()
    core[v] = keep + 1  # claims a core it is not in
    assert eng.check() >= 1
    core[v] = keep
    assert eng.check() == 0


def test_two_parts_raise():
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        KCoreEngine(part)


def test_knobs_are_validated(monkeypatch):
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    for name, bad in (("LUX_KCORE_HUB", 0),
                      ("LUX_KCORE_FUSE", ng.kcore_fuse_max() + 1)):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            KCoreEngine(part)
        monkeypatch.delenv(name)


# ---- 5. app ----

def test_kcore_app_main_check(capsys):
    from lux_amd.apps import kcore
    kcore.main(["-synthetic", "rmat:12:300000", "-kcore", "8", "-check",
                "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] kcore: degeneracy " in out
    assert "phases orient/adjacency/peel" in out
    assert "the 8-core has " in out
    assert "k,removed,rounds" in out
    assert "[PASS] 0 mistakes" in out
