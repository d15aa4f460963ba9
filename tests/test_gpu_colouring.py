"""GPU greedy colouring / MIS (ColouringEngine, src/gpu/colouring.hip)
against the exact CPU oracle cpu_ref.greedy_colouring: the hand cases in the
three priority orders, the clique staircase around the bitmap window, the hub
ladder at the default GCOL_HUB and at LUX_GCOL_HUB=64, a directed and a
symmetric RMAT-12 with their pinned values, engine behaviour, the check
oracle's negative cases and the app. A colour is an integer per vertex: every
comparison is equality, and rounds and per-round sizes equal
colouring_ref.sync_jp's with the round fusion off and on."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import colouring_ref as cr  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.colouring_engine import ColouringEngine  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402

KNOBS = ("LUX_GCOL_HUB", "LUX_GCOL_FUSE")
FUSE = pytest.mark.parametrize("fuse", [0, None], ids=["nofuse", "fuse"])
ORDER = pytest.mark.parametrize("order", cr.ORDERS)


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


def make_engine(g, monkeypatch=None, fuse=None, hub=None, order="degree",
                seed=1):
    for name, val in zip(KNOBS, (hub, fuse)):
        if val is not None:
            monkeypatch.setenv(name, str(val))
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    return ColouringEngine(part, order=order, seed=seed)


def host(t):
    return t.cpu().numpy()


_REF = {}


def reference(name, g, order):
    """(oracle colours, sync_jp rounds, sync_jp per-round sizes), computed
    once per graph and order and shared."""
    key = (name, order)
    if key not in _REF:
        want = cpu_ref.greedy_colouring(g, order)
        colour, rounds, sizes = cr.sync_jp(g, order)
        assert np.array_equal(want, colour)
        want.setflags(write=False)
        _REF[key] = (want, rounds, sizes)
    return _REF[key]


def assert_solution(eng, want, rounds, sizes):
    got = host(eng.solve())
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    st = eng.stats
    print(st, eng.phase_ms)
    assert st["rounds"] == rounds == eng.rounds()
    assert eng.round_trace == [(r + 1, n) for r, n in enumerate(sizes)]
    # the seed launch and at most one launch per round, a read per launch
    assert st["host_reads"] == st["launches"] <= 1 + rounds
    if eng.fuse == 0:
        assert st["fused_rounds"] == 0
        assert st["launches"] == 1 + rounds
    assert st["hub_items"] == st["hub_selects"] + st["hub_chunks"]
    assert eng.check() == 0
    assert eng.num_colours() == int(want.max(initial=-1)) + 1
    assert np.array_equal(host(eng.class_sizes()), np.bincount(want))
    assert np.array_equal(host(eng.independent_set()), want == 0)


# ---- 1. hand cases ----

@FUSE
@ORDER
@pytest.mark.parametrize("case", cr.hand_cases(), ids=lambda c: c.name)
def test_hand_cases(case, order, fuse, monkeypatch):
    want, rounds, sizes = reference(case.name, case.g, order)
    if order == "id":
        if case.colour is not None:
            assert np.array_equal(want, case.colour)
        assert rounds == case.rounds
        assert int(want.max()) + 1 == case.ncolours
    eng = make_engine(case.g, monkeypatch, fuse=fuse, order=order)
    assert_solution(eng, want, rounds, sizes)
    st = eng.stats
    if case.name == "path4001" and order == "id" and fuse is None:
        # the cascade is carried by the tail kernel: the seed's read and one
        # for its launch
        assert st["fused_rounds"] == rounds == cr.PATH_N
        assert st["host_reads"] <= 4
    if case.name == "star5000" and order == "id":
        assert eng.hub < cr.STAR_LEAVES
        assert st["hub_selects"] == 0
        assert st["hub_chunks"] == -(-cr.STAR_LEAVES // eng.hub)
    if case.name == "reverse_star5000" and order == "id":
        assert st["max_pred"] == cr.STAR_LEAVES > eng.hub
        assert st["hub_selects"] == 1 and st["hub_chunks"] == 0


# ---- 2. window staircase ----

def _staircase(n, monkeypatch, fuse, hub):
    g = cr.clique(n)
    want, rounds, sizes = reference(f"k{n}", g, "id")
    assert np.array_equal(want, np.arange(n))
    assert rounds == n and sizes == [1] * n
    eng = make_engine(g, monkeypatch, fuse=fuse, hub=hub, order="id")
    assert_solution(eng, want, rounds, sizes)
    st = eng.stats
    assert st["max_pred"] == st["max_degree"] == n - 1
    # rows 0..n-1 of either kind: the ones longer than hub are hub rows
    long_rows = max(n - 1 - eng.hub, 0)
    assert st["hub_selects"] == long_rows
    assert st["hub_chunks"] == sum(
        -(-d // eng.hub) for d in range(eng.hub + 1, n))
    return eng


@FUSE
@pytest.mark.parametrize("n", cr.staircase_sizes(1024)[:-4])
def test_staircase_small(n, fuse, monkeypatch):
    _staircase(n, monkeypatch, fuse, None)


@FUSE
def test_staircase_window(fuse, monkeypatch):
    """K_n around n = W, the largest at the default hub limit: the wave
    select's rows reach W = hub entries (colours 0..W-1: a full window and a
    second pass), the workgroup select takes W + 1 and beyond."""
    W = ng.gcol_window_bits()
    assert cr.staircase_sizes(W)[-4:] == [W - 1, W, W + 1, W + 2]
    assert ng.gcol_hub_default() == W  # what puts both roles past a window
    for n in cr.staircase_sizes(W)[-4:]:
        eng = _staircase(n, monkeypatch, fuse, None)
    assert eng.stats["hub_selects"] == 1  # the row of W + 1 predecessors


@FUSE
def test_staircase_wave_second_pass(fuse, monkeypatch):
    """K_(W+2) with every row in the wave role."""
    W = ng.gcol_window_bits()
    eng = _staircase(W + 2, monkeypatch, fuse, 4 * W)
    assert eng.stats["hub_items"] == 0


@FUSE
def test_staircase_k200_hub64(fuse, monkeypatch):
    eng = _staircase(200, monkeypatch, fuse, 64)
    assert eng.stats["hub_selects"] == 199 - 64


# ---- 3. hub ladder ----

@FUSE
@pytest.mark.parametrize("hub", [None, 64], ids=["default", "hub64"])
@pytest.mark.parametrize("side", ["below", "above"])
def test_hub_ladder(side, hub, fuse, monkeypatch):
    h = hub if hub is not None else ng.gcol_hub_default()
    lad = cr.ladder(h, side)
    want, rounds, sizes = reference(f"ladder{h}{side}", lad.g, "id")
    npred, nsucc = cr.pred_succ_counts(lad.g, "id")
    rows, zero = (nsucc, npred) if side == "below" else (npred, nsucc)
    assert np.array_equal(rows[lad.rows], lad.degrees)
    assert not zero[lad.rows].any()
    eng = make_engine(lad.g, monkeypatch, fuse=fuse, hub=hub, order="id")
    assert eng.hub == h
    assert_solution(eng, want, rounds, sizes)
    st = eng.stats
    assert np.array_equal(host(eng.npred)[:lad.g.nv], npred)
    assert np.array_equal(host(eng.nsucc)[:lad.g.nv], nsucc)
    # only the ladder rows are long: h - 1 and h stay with the waves; h + 1,
    # 2h - 1 and 2h are two chunks (or one select), 2h + 1 is three
    assert int((npred > h).sum()) + int((nsucc > h).sum()) == \
        4 * cr.LADDER_ROWS_PER_DEGREE
    if side == "below":
        assert st["hub_selects"] == 0
        assert st["hub_chunks"] == (2 + 2 + 2 + 3) * cr.LADDER_ROWS_PER_DEGREE
    else:
        assert st["hub_selects"] == 4 * cr.LADDER_ROWS_PER_DEGREE
        assert st["hub_chunks"] == 0
    assert st["hub_items"] == st["hub_selects"] + st["hub_chunks"] == \
        eng.hubcap


# ---- 4. RMAT-12 ----

# Graph.rmat(12, 40000, seed=7, sym=...), tests/test_colouring_cpu.py
RMAT = {
    False: dict(degree=(31, 109, 2521), id=(32, 115, 2583),
                hash=(39, 123, 2777)),
    True: dict(degree=(18, 75, 2786), id=(22, 72, 2872),
               hash=(27, 80, 3005)),
}


@pytest.fixture(scope="module")
def rmat():
    return {sym: Graph.rmat(12, 40000, seed=7, sym=sym)
            for sym in (False, True)}


@FUSE
@ORDER
@pytest.mark.parametrize("sym", [False, True], ids=["directed", "sym"])
def test_rmat(rmat, sym, order, fuse, monkeypatch):
    g = rmat[sym]
    colours, rounds, mis = RMAT[sym][order]
    want, r, sizes = reference(f"rmat12_{sym}", g, order)
    assert (int(want.max()) + 1, r, int((want == 0).sum())) == \
        (colours, rounds, mis)
    eng = make_engine(g, monkeypatch, fuse=fuse, order=order)
    assert_solution(eng, want, rounds, sizes)
    assert eng.num_colours() == colours
    assert int(eng.independent_set().sum().item()) == mis
    npred, _ = cr.pred_succ_counts(g, order)
    assert eng.stats["max_pred"] == int(npred.max())
    # a second solve() starts from scratch
    assert np.array_equal(host(eng.solve()), want)
    assert eng.stats["rounds"] == rounds


def test_rmat_hub16_and_seed(rmat, monkeypatch):
    """Hub rows on a real graph, and a hash order with another seed."""
    g = rmat[False]
    want, rounds, sizes = reference("rmat12_False", g, "degree")
    eng = make_engine(g, monkeypatch, hub=16)
    assert eng.stats["hub_selects"] > 0 and eng.stats["hub_chunks"] > 0
    assert_solution(eng, want, rounds, sizes)
    eng = make_engine(g, order="hash", seed=2)
    assert np.array_equal(host(eng.solve()),
                          cpu_ref.greedy_colouring(g, "hash", 2))


# ---- 5. engine behaviour ----

def test_independent_set_is_independent_and_maximal(rmat):
    g = rmat[True]
    eng = make_engine(g)
    mis = host(eng.independent_set())
    assert mis.dtype == np.bool_
    ptr, adj = cr.kcore_ref.simple_adjacency(g)
    row = np.repeat(np.arange(g.nv), np.diff(ptr))
    assert not (mis[row] & mis[adj]).any()
    covered = np.bincount(row[mis[adj]], minlength=g.nv) > 0
    assert (mis | covered).all()


def test_two_parts_raise():
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 2, 0)
    with pytest.raises(ValueError, match="single-rank"):
        ColouringEngine(part)


def test_order_and_knobs_are_validated(monkeypatch):
    g = Graph.rmat(10, 8000, seed=3)
    part = GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0)
    with pytest.raises(ValueError, match="order"):
        ColouringEngine(part, order="random")
    for name, bad in (("LUX_GCOL_HUB", 0), ("LUX_GCOL_HUB", (1 << 20) + 1),
                      ("LUX_GCOL_FUSE", -1),
                      ("LUX_GCOL_FUSE", ng.gcol_fuse_max() + 1)):
        monkeypatch.setenv(name, str(bad))
        with pytest.raises(ValueError, match=name):
            ColouringEngine(part)
        monkeypatch.delenv(name)


# ---- 6. the check oracle's negative cases ----

def test_check_sees_each_broken_condition():
    """Entries of the stored colour array are overwritten on the device so
    that one condition breaks at a time. 0-1-2-3 is a path, 4 hangs off 2,
    5 off 0 and 2, 6 off 1 and 3; in id order the colours are
    0 1 0 1 1 1 0."""
    g = cr._graph(7, [(0, 1), (1, 2), (2, 3), (2, 4), (0, 5), (2, 5),
                      (1, 6), (3, 6)])
    eng = make_engine(g, order="id")
    col = eng.colours()
    assert host(col).tolist() == [0, 1, 0, 1, 1, 1, 0]
    assert eng.check() == 0
    broken = {
        "equal colours on an edge": (4, 0),  # 2 and 4 both 0
        "colour too high": (0, 1),           # 0 has no predecessor
        # 5 has the predecessors 0 and 2, both of colour 0: 2 is within
        # [0, 2] and clashes with nobody, but no predecessor holds 1
        "a gap": (5, 2),
        # 6 has the predecessors 1 and 3, both of colour 1: 2 is within
        # [0, 2], clashes with nobody and has its 1 below it, but no
        # predecessor is in class 0, which therefore is not maximal
        "class 0 not maximal": (6, 2),
        "uncoloured": (1, -1),
    }
    for what, (v, c) in broken.items():
        keep = col[v].clone()
        col[v] = c
        assert eng.check() > 0, what
        col[v] = keep
        assert eng.check() == 0, what


# ---- 7. app ----

def test_colouring_app_on_a_file(tmp_path, capsys):
    from lux_amd.apps import colouring
    g = Graph.rmat(10, 8000, seed=3)
    path = str(tmp_path / "g.lux")
    g.save(path)
    for order in cr.ORDERS:
        eng = colouring.main(["-file", path, "-order", order, "-check",
                              "-verbose"])
        out = capsys.readouterr().out
        assert "[PASS] 0 mistakes" in out
        assert f"in {order} order" in out
        assert np.array_equal(host(eng.colours()),
                              cpu_ref.greedy_colouring(g, order))


def test_colouring_app_main_check(capsys):
    from lux_amd.apps import colouring
    eng = colouring.main(["-synthetic", "rmat:12:40000", "-check",
                          "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out
    assert "[lux] colouring: " in out and " colours in degree order" in out
    assert "phases orient/split/solve" in out
    assert "[PASS] 0 mistakes" in out
    lines = out.splitlines()
    first = lines.index("coloured,round")
    rows = [ln for ln in lines[first + 1:] if ln[:1].isdigit()]
    assert len(rows) == eng.rounds() > 1
    assert sum(int(r.split(",")[0]) for r in rows) == eng.part.nv
    with pytest.raises(SystemExit, match="-order"):
        colouring.main(["-synthetic", "rmat:12:40000", "-order", "random"])
