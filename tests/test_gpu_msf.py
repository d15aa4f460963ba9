"""GPU minimum spanning forest (MSFEngine, src/gpu/msf.hip) against the
exact CPU oracle cpu_ref.msf and the numpy schedule msf_ref.sync_boruvka:
the hand cases (ties on a cycle, parallel arcs, self-loops, extreme
weights), the hub ladder at the default hub length and at LUX_MSF_HUB=64,
the RMAT graphs with their pinned values, engine behaviour and the app. The
order (w, e) is strict, so every comparison is equality, and the round
statistics equal the schedule's with the dead-row rule on and off."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import msf_ref  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.msf_engine import MSFEngine  # noqa: E402

KNOBS = ("LUX_MSF_HUB", "LUX_MSF_DEAD")
HUB = pytest.mark.parametrize("hub", [None, 64], ids=["default", "hub64"])
DEAD = pytest.mark.parametrize("dead", [None, 0], ids=["dead", "nodead"])


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


def make_engine(g, monkeypatch=None, hub=None, dead=None):
    for name, val in zip(KNOBS, (hub, dead)):
        if val is not None:
            monkeypatch.setenv(name, str(val))
    return MSFEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0))


def host(t):
    return t.cpu().numpy()


_REF = {}


def reference(name, g):
    """(oracle tuple, schedule with the dead-row rule, schedule without),
    computed once per graph and shared."""
    if name not in _REF:
        want = cpu_ref.msf(g)
        ref = msf_ref.sync_boruvka(g)
        plain = msf_ref.sync_boruvka(g, dead=False)
        assert np.array_equal(want[3], ref.in_forest)
        assert want[4] == ref.total
        for arr in want:
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _REF[name] = (want, ref, plain)
    return _REF[name]


def assert_forest(eng, g, want, ref, plain):
    lo, hi, w, mask, total, labels = want
    m = lo.size
    assert eng.solve() == total and isinstance(eng.total_weight(), int)
    assert eng.total_weight() == total
    st = eng.stats
    print(st, eng.phase_ms)
    got = host(eng.in_forest())
    assert got.dtype == np.bool_ and got.shape == (m,)
    assert np.array_equal(got, mask)
    slo, shi, sw = (host(t) for t in eng.simple_edges())
    assert np.array_equal(slo.view(np.uint32), lo)
    assert np.array_equal(shi.view(np.uint32), hi)
    assert sw.dtype == np.int32 and np.array_equal(sw, w)
    flo, fhi, fw = (host(t) for t in eng.edges())
    assert np.array_equal(flo.view(np.uint32), lo[mask])
    assert np.array_equal(fhi.view(np.uint32), hi[mask])
    assert np.array_equal(fw, w[mask])
    lab = host(eng.labels())
    assert lab.dtype == np.int32 and lab.shape == labels.shape
    assert np.array_equal(lab.view(np.uint32), labels)
    comps = int(np.unique(labels).size)
    assert eng.num_components() == comps
    assert eng.num_edges() == int(mask.sum()) == g.nv - comps
    sched = ref if eng.dead else plain
    assert st["rounds"] == sched.rounds == ref.rounds
    assert st["per_round"] == sched.per_round
    if not eng.dead:
        assert all(r[2] == 2 * m for r in st["per_round"])
    assert st["scanned"] == sched.scanned
    assert st["scans"] == (st["rounds"] + 1 if m else 0)
    assert st["host_reads"] <= st["launches"]
    assert st["simple_edges"] == m
    assert eng.check() == 0
    return st


# ---- 1. hand cases ----

@DEAD
@HUB
@pytest.mark.parametrize("case", msf_ref.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, hub, dead, monkeypatch):
    want, ref, plain = reference(case.name, case.g)
    assert want[4] == case.want["total"]
    assert int(want[3].sum()) == case.want["nf"]
    eng = make_engine(case.g, monkeypatch, hub=hub, dead=dead)
    st = assert_forest(eng, case.g, want, ref, plain)
    if "rounds" in case.want:
        assert st["rounds"] == case.want["rounds"]
    if "per_round" in case.want and eng.dead:
        assert st["per_round"] == case.want["per_round"]


# ---- 2. hub ladder ----

@DEAD
@HUB
@pytest.mark.parametrize("case", msf_ref.ladder_cases(), ids=lambda c: c.name)
def test_hub_ladder(case, hub, dead, monkeypatch):
    want, ref, plain = reference(case.name, case.g)
    L = case.want["max_degree"]
    assert want[4] == case.want["total"] and ref.rounds == 2
    assert ref.per_round == case.want["per_round"]
    eng = make_engine(case.g, monkeypatch, hub=hub, dead=dead)
    st = assert_forest(eng, case.g, want, ref, plain)
    assert st["max_degree"] == L and eng.num_edges() == L
    if L > eng.hub:  # the hub role really ran
        assert st["hub_rows"] == 1
        assert st["hub_items"] == -(-L // eng.hub) >= 2
    else:
        assert st["hub_rows"] == st["hub_items"] == 0


def test_default_hub_cases_are_hub_rows():
    hubs = [c for c in msf_ref.ladder_cases()
            if c.want["max_degree"] > ng.msf_hub_default()]
    assert len(hubs) >= 4
    eng = make_engine(hubs[0].g)
    assert eng.stats["max_degree"] == hubs[0].want["max_degree"] > eng.hub


# ---- 3. RMAT ----

@pytest.fixture(scope="module")
def rmat():
    out = {}
    for name in msf_ref.RMAT:
        g = msf_ref.rmat_graph(name)
        out[name] = (g,) + reference(name, g)
    return out


@DEAD
@HUB
@pytest.mark.parametrize("name", sorted(msf_ref.RMAT))
def test_rmat(rmat, name, hub, dead, monkeypatch):
    g, want, ref, plain = rmat[name]
    pin = msf_ref.RMAT[name]
    assert want[0].size == pin["m"] and want[4] == pin["total"]
    assert ref.per_round == pin["per_round"]
    eng = make_engine(g, monkeypatch, hub=hub, dead=dead)
    st = assert_forest(eng, g, want, ref, plain)
    assert st["max_degree"] == pin["max_degree"]
    assert eng.num_edges() == pin["nf"]
    assert eng.num_components() == pin["components"]
    if pin["max_degree"] > eng.hub:
        assert st["hub_rows"] >= 1 and st["hub_items"] >= 2
    if eng.dead:
        assert st["per_round"] == pin["per_round"]
    if pin["sym"]:
        cc, _ = cpu_ref.cc(g)
        assert np.array_equal(host(eng.labels()).view(np.uint32), cc)


# ---- 4. engine behaviour ----

def test_missing_weight_raises():
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    with pytest.raises(ValueError, match="weight"):
        MSFEngine(part)


def test_two_parts_raise():
    g = msf_ref.rmat_graph("rmat10_w16")
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        MSFEngine(part)


def test_knobs_are_validated(monkeypatch):
    g = msf_ref.rmat_graph("rmat10_w16")
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    for name, bad in (("LUX_MSF_HUB", 0), ("LUX_MSF_DEAD", 2)):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            MSFEngine(part)
        monkeypatch.delenv(name)


def test_solve_twice_gives_the_same(rmat):
    g, want, ref, plain = rmat["rmat12_w1000"]
    eng = make_engine(g)
    assert_forest(eng, g, want, ref, plain)
    first = eng.stats
    assert_forest(eng, g, want, ref, plain)
    assert eng.stats == first


def test_device_hash_weights_match_the_host(rmat):
    g, want, ref, plain = rmat["rmat10_w16"]
    bare = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(bare, "cuda"), 1, 0)
    part.hash_weights(16)
    eng = MSFEngine(part)
    assert_forest(eng, g, want, ref, plain)


def test_check_sees_a_corrupted_mask(rmat):
    g, want, _, _ = rmat["rmat12_w16"]
    eng = make_engine(g)
    eng.solve()
    assert eng.check() == 0
    mask, m = want[3], want[0].size
    s = torch.cuda.current_stream().cuda_stream
    # a forest edge cleared on a copy: the forest no longer spans
    copy = eng.in_forest().view(torch.uint8).clone()
    e = int(np.nonzero(mask)[0][7])
    ng.msf_set_mark(s, copy, m, e, 0)
    assert eng.check(mask=copy) >= 1
    # one edge too many: a cycle, the counts no longer match
    copy = eng.in_forest().view(torch.uint8).clone()
    e = int(np.nonzero(~mask)[0][7])
    ng.msf_set_mark(s, copy, m, e, 1)
    assert eng.check(mask=copy) >= 1
    with pytest.raises(ValueError, match="outside"):
        ng.msf_set_mark(s, copy, m, m, 1)
    assert eng.check() == 0


# ---- 5. app ----

def test_msf_app_synthetic_check(capsys):
    from lux_amd.apps import msf
    msf.main(["-synthetic", "rmat:10:8000", "-wmax", "16", "-check",
              "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    # DeviceCSC.rmat's default seed is not the pinned graphs' seed 3
    assert "[lux] msf: total weight " in out and " forest edges of " in out
    assert "round,components_with_edge,merged,scanned" in out
    assert "[PASS] 0 mistakes" in out


def test_msf_app_file(tmp_path, capsys):
    from lux_amd.apps import msf
    g = msf_ref.rmat_graph("rmat10_w16")
    pin = msf_ref.RMAT["rmat10_w16"]
    path = str(tmp_path / "w.lux")
    g.save(path)
    msf.main(["-file", path, "-check", "-verbose"])
    out = capsys.readouterr().out
    assert f"total weight {pin['total']}, {pin['nf']} forest edges of " \
        f"{pin['m']} simple edges, {pin['components']} components" in out
    for i, row in enumerate(pin["per_round"]):
        assert f"{i + 1},{row[0]},{row[1]},{row[2]}" in out
    assert "[PASS] 0 mistakes" in out
    bare = Graph.rmat(10, 8000, seed=3)
    path = str(tmp_path / "plain.lux")
    bare.save(path)
    with pytest.raises(SystemExit, match="weights"):
        msf.main(["-file", path])
