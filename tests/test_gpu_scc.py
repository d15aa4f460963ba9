"""GPU strongly connected components (SCCEngine, src/gpu/scc.hip) against
the exact CPU oracle cpu_ref.scc and the numpy schedule
scc_ref.sync_schedule: the hand cases (double loss of counters, cascade,
cycle, slow colouring chain, parallel edges, stars in the hub role), the
star ladder at LUX_SCC_HUB=64, the RMAT graphs with their pinned values,
the planted graphs, the two giants, engine behaviour and the app. Labels are
integers: every comparison is equality, and the phase statistics equal the
schedule's with the step fusion off and on (colour_sweeps: at most the
schedule's)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import scc_ref  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.scc_engine import SCCEngine  # noqa: E402

KNOBS = ("LUX_SCC_HUB", "LUX_SCC_FUSE")
FUSE = pytest.mark.parametrize("fuse", [0, None], ids=["nofuse", "fuse"])
HUB = pytest.mark.parametrize("hub", [None, 64], ids=["default", "hub64"])
EQUAL = ("trim_rounds", "trimmed", "pivot", "fwbw", "reach_rounds",
         "colour_rounds")


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
    return SCCEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))


def host(t):
    return t.cpu().numpy()


_REF = {}


def reference(name, g):
    """(oracle labels u32, sync_schedule stats), computed once per graph
    and shared."""
    if name not in _REF:
        want = cpu_ref.scc(g)
        label, stats = scc_ref.sync_schedule(g)
        assert np.array_equal(want, label)
        want.setflags(write=False)
        _REF[name] = (want, stats)
    return _REF[name]


def assert_decomposition(eng, want, stats):
    got = host(eng.decompose())
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want)
    st = eng.stats
    print(st, eng.phase_ms)
    for key in EQUAL:
        assert st[key] == stats[key], (key, st[key], stats[key])
    assert st["colour_sweeps"] <= stats["colour_sweeps"]
    assert st["colour_sweeps"] >= st["colour_rounds"]
    assert st["host_reads"] <= st["launches"]
    if eng.fuse == 0:
        assert st["fused_steps"] == 0
    assert eng.check() == 0
    assert int(eng.sizes().sum().item()) == want.size
    assert eng.num_components() == np.unique(want).size
    return st


# ---- 1. hand cases ----

@FUSE
@pytest.mark.parametrize("case", scc_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, fuse, monkeypatch):
    want, stats = reference(case.name, case.g)
    assert np.array_equal(want, case.label)
    for key, val in case.stats.items():
        assert stats[key] == val
    eng = make_engine(case.g, monkeypatch, fuse=fuse)
    st = assert_decomposition(eng, want, stats)
    if case.name in ("path4001", "cycle4001") and fuse is None:
        # the cascade is carried by the tail kernel: O(1) launches
        assert st["fused_steps"] >= scc_ref.PATH_N // 2
        assert st["host_reads"] <= 8
    if case.name in scc_ref.STAR_CASES:
        assert max(st["max_in_degree"], st["max_out_degree"]) == \
            scc_ref.STAR_LEAVES > eng.hub
        assert eng.hubcap >= 2 and st["hub_items"] >= 2


@FUSE
@pytest.mark.parametrize("name", scc_ref.STAR_CASES)
def test_stars_hub64(name, fuse, monkeypatch):
    case = {c.name: c for c in scc_ref.hand_cases()}[name]
    want, stats = reference(case.name, case.g)
    eng = make_engine(case.g, monkeypatch, fuse=fuse, hub=64)
    assert eng.hub == 64
    st = assert_decomposition(eng, want, stats)
    assert st["hub_items"] >= scc_ref.STAR_LEAVES // 64


# ---- 2. star ladder ----

@FUSE
@pytest.mark.parametrize("leaves", scc_ref.ladder_leaves(64))
def test_star_ladder_hub64(leaves, fuse, monkeypatch):
    case = scc_ref.ladder_case(leaves)
    want, stats = reference(case.name, case.g)
    assert np.array_equal(want, case.label)
    for key, val in case.stats.items():
        assert stats[key] == val
    eng = make_engine(case.g, monkeypatch, fuse=fuse, hub=64)
    st = assert_decomposition(eng, want, stats)
    assert st["max_out_degree"] == st["max_in_degree"] == leaves
    assert (st["hub_items"] > 0) == (leaves > 64)


# ---- 3. RMAT ----

RMAT = {
    "rmat12": dict(args=(12, 300000), sym=False, sccs=583, largest=3514,
                   stats=dict(trim_rounds=2, trimmed=582, pivot=0,
                              reach_rounds=8, colour_rounds=0)),
    "rmat14": dict(args=(14, 40000), sym=False, sccs=12076, largest=4309,
                   stats=dict(trim_rounds=3, trimmed=12075, pivot=0,
                              reach_rounds=13, colour_rounds=0)),
    "rmat12_sym": dict(args=(12, 300000), sym=True, sccs=420, largest=3677,
                       stats=dict(trim_rounds=1, trimmed=419)),
}


@pytest.fixture(scope="module")
def rmat():
    out = {}
    for name, pin in RMAT.items():
        g = Graph.rmat(*pin["args"], seed=3, sym=pin["sym"])
        want, stats = reference(name, g)
        out[name] = dict(g=g, want=want, stats=stats)
    return out


@FUSE
@HUB
@pytest.mark.parametrize("name", sorted(RMAT))
def test_rmat(rmat, name, hub, fuse, monkeypatch):
    r, pin = rmat[name], RMAT[name]
    want = r["want"]
    for key, val in pin["stats"].items():
        assert r["stats"][key] == val
    assert np.unique(want).size == pin["sccs"]
    eng = make_engine(r["g"], monkeypatch, fuse=fuse, hub=hub)
    assert_decomposition(eng, want, r["stats"])
    assert eng.num_components() == pin["sccs"]
    label, size = eng.largest()
    assert size == pin["largest"] == int(np.bincount(want).max())
    assert label == int(np.argmax(np.bincount(want)))
    mask = host(eng.member_mask(label))
    assert mask.dtype == np.bool_ and np.array_equal(mask, want == label)
    sizes = host(eng.sizes())
    assert sizes.dtype == np.int64
    assert np.array_equal(sizes, np.bincount(want, minlength=want.size))
    # a second decompose() starts from scratch
    assert np.array_equal(host(eng.decompose()).view(np.uint32), want)
    assert eng.stats["trim_rounds"] == pin["stats"]["trim_rounds"]


def test_symmetric_graph_gives_the_weak_components(rmat):
    g = rmat["rmat12_sym"]["g"]
    cc, _ = cpu_ref.cc(g)
    eng = make_engine(g)
    got = host(eng.labels()).view(np.uint32)
    assert scc_ref.same_partition(got, cc)


# ---- 4. planted graphs and the two giants ----

PLANTED = [(300, 64, 3000, 7), (400, 200, 40000, 5)]


@pytest.fixture(scope="module")
def planted():
    out = {}
    for args in PLANTED:
        g, label = scc_ref.planted(*args)
        want, stats = reference(f"planted{args}", g)
        assert np.array_equal(want, label)
        out[args] = dict(g=g, want=want, stats=stats)
    return out


@FUSE
@HUB
@pytest.mark.parametrize("args", PLANTED, ids=lambda a: "-".join(map(str, a)))
def test_planted(planted, args, hub, fuse, monkeypatch):
    r = planted[args]
    assert r["stats"]["colour_rounds"] >= 2
    eng = make_engine(r["g"], monkeypatch, fuse=fuse, hub=hub)
    assert_decomposition(eng, r["want"], r["stats"])


@FUSE
@HUB
def test_two_giants(hub, fuse, monkeypatch):
    g = scc_ref.two_giants()
    want, stats = reference("two_giants", g)
    # forward-backward takes one giant, colouring the other
    assert stats["fwbw"] > 1 and stats["colour_rounds"] >= 1
    eng = make_engine(g, monkeypatch, fuse=fuse, hub=hub)
    assert_decomposition(eng, want, stats)


# ---- 5. engine behaviour ----

def test_check_sees_a_corrupted_entry(rmat):
    r = rmat["rmat12"]
    eng = make_engine(r["g"])
    label = eng.labels()
    assert eng.check() == 0
    want = r["want"]
    giant = int(np.argmax(np.bincount(want)))
    # a trimmed vertex claimed by the giant: the root does not reach it, or
    # it does not reach the root, inside the class
    v = int(np.nonzero((want == np.arange(want.size)) &
                       (np.arange(want.size) < giant))[0][0])
    keep = label[v].clone()
    label[v] = giant
    assert eng.check() >= 1
    label[v] = keep
    assert eng.check() == 0
    if v > 0:
        label[v] = v - 1  # below its own id
        assert eng.check() >= 1
        label[v] = keep
        assert eng.check() == 0


def test_two_parts_raise():
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        SCCEngine(part)


def test_knobs_are_validated(monkeypatch):
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    for name, bad in (("LUX_SCC_HUB", 0),
                      ("LUX_SCC_FUSE", ng.scc_fuse_max() + 1)):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            SCCEngine(part)
        monkeypatch.delenv(name)


# ---- 6. app ----

def test_scc_app_main_check(capsys):
    from lux_amd.apps import scc
    scc.main(["-synthetic", "rmat:12:300000", "-check", "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] scc: " in out and " SCCs, largest " in out
    assert "phases csr/trim/fwbw/colour" in out
    assert "kind,round,removed" in out
    assert "[PASS] 0 mistakes" in out
