"""PageRank slot path, stream role: the thread bin of every src window run
as one contiguous edge stream (off0 / scol0 / tile0), one wave per tile.
Same two checks as test_gpu_pull_slots (exact integer sums; step-by-step
agreement with the row-table engine, non-hub rows bit for bit), on graphs
that pin the degrees, slot counts and tile cuts at which the role changes
path, plus the tile table itself and the LUX_PULL_STREAM switch.

The order of slots inside a bin is whatever the bin build's atomics gave,
so every graph here is shaped to hit its edge case in any slot order, and
the table checks read the order back from the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_pull_slots import (_engines_agree, _part,  # noqa: E402
                                 _sweep_exact)

from lux_amd.engine import run_pull_slots_sweeps  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402

T1, T2 = 32, 2048
TILE_SLOTS, TILE_EDGES = 64, 512
SHIFT = 6
W = 1 << SHIFT  # src window width


@pytest.fixture(autouse=True)
def _stream_on(monkeypatch):
    monkeypatch.setenv("LUX_PULL_STREAM", "1")


def _graph(nv, rows, seed):
    """rows: (dst row, src window, in-degree from that window)."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([
        k * W + rng.integers(0, min(W, nv - k * W), d) for _, k, d in rows])
    dst = np.concatenate([np.full(d, v) for v, _, d in rows])
    return Graph.from_edges(nv, src.astype(np.uint32), dst.astype(np.uint32))


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _check_tables(part):
    """off0 / scol0 / tile0 of every window against rng0 and col read back
    from the device. Returns per window (thread slots, tile sizes)."""
    assert part.prepare_pull_slots()
    part.prepare_pull_stream()
    out = []
    for src in part.slot_srcs:
        n0 = src["n0"]
        if not n0:
            assert src["nt"] == 0
            out.append((0, []))
            continue
        rng0 = _u32(src["rng0"])[:2 * n0].reshape(n0, 2)
        deg = rng0[:, 1] - rng0[:, 0]
        assert ((deg > 0) & (deg < T1)).all()
        off0 = _u32(src["off0"])
        assert len(off0) == n0 + 1
        assert np.array_equal(off0, np.concatenate([[0], np.cumsum(deg)]))
        col = _u32(src["col"])
        want = np.concatenate([col[b:e] for b, e in rng0])
        assert np.array_equal(_u32(src["scol0"]), want)
        tile0 = _u32(src["tile0"])
        nt = src["nt"]
        assert len(tile0) == nt + 1
        assert tile0[0] == 0 and tile0[nt] == n0
        slots = np.diff(tile0)
        assert (slots > 0).all()  # ascending: tiles cover the slots in order
        assert slots.max() <= TILE_SLOTS
        edges = np.diff(off0[tile0])
        assert edges.max() <= TILE_EDGES
        out.append((n0, list(zip(slots.tolist(), edges.tolist()))))
    return out


def _both_checks(g, part, monkeypatch):
    _sweep_exact(part, g)
    slot = _engines_agree(g, part, monkeypatch, steps=4)
    assert slot._stream_role and slot._graph is not None


def test_stream_degree_ladder(monkeypatch):
    """Thread-bin degrees where the four-way order and its tail change:
    once, in reverse row order, and three times over in one window."""
    ladder = [1, 2, 3, 4, 5, 7, 8, 9, 31]
    rows = [(v, 0, d) for v, d in enumerate(ladder)]
    rows += [(20 + v, 1, d) for v, d in enumerate(reversed(ladder))]
    rows += [(40 + v, 2, d) for v, d in enumerate(ladder * 3)]
    g = _graph(256, rows, 41)
    part = _part(g, SHIFT)
    info = _check_tables(part)
    assert [n for n, _ in info] == [9, 9, 27]
    _both_checks(g, part, monkeypatch)


def test_stream_slot_counts_around_cap(monkeypatch):
    """1, 63, 64, 65 and 129 thread-bin slots in a window: below, at and
    past one 64-slot group, and a ragged third group."""
    counts = [1, 63, 64, 65, 129]
    rows = [(v, k, 1 + (v + k) % 5) for k, n in enumerate(counts)
            for v in range(n)]
    g = _graph(512, rows, 42)
    part = _part(g, SHIFT)
    info = _check_tables(part)
    assert [n for n, _ in info] == counts
    assert [len(t) for _, t in info] == [1, 1, 1, 2, 3]
    _both_checks(g, part, monkeypatch)


def test_stream_tile_edge_cap(monkeypatch):
    """Window 0: 64 slots of degree 31 (1,984 edges: forced cuts, and 512
    is no multiple of 31, so a cut by edges alone would land inside a
    slot). Window 1: 64 x 8 = exactly 512 edges, one tile at both caps.
    Window 2: 63 x 8 + 9 = 513, one edge too many. Window 3: 130 slots of
    degree 31, cuts in a ragged last group."""
    rows = [(v, 0, 31) for v in range(64)]
    rows += [(v, 1, 8) for v in range(64)]
    rows += [(v, 2, 8) for v in range(63)] + [(63, 2, 9)]
    rows += [(v, 3, 31) for v in range(130)]
    g = _graph(256, rows, 43)
    part = _part(g, SHIFT)
    info = _check_tables(part)
    assert [n for n, _ in info] == [64, 64, 64, 130]
    assert info[0][1] == [(16, 496)] * 4
    assert info[1][1] == [(64, 512)]
    assert len(info[2][1]) == 2 and sum(e for _, e in info[2][1]) == 513
    assert info[3][1] == [(16, 496)] * 8 + [(2, 62)]
    _both_checks(g, part, monkeypatch)


def test_stream_rows_between_thread_rows(monkeypatch):
    """Window 0: thread-bin rows with a wave-bin row (degree 32) and a hub
    (degree >= 2048) between them, whose edges scol0 must skip. Window 1:
    no thread-bin slot at all. Window 2: thread-bin slots only. Window 4:
    ragged (nv = 300, 44 wide) with thread-bin slots."""
    rows = [(0, 0, 5), (1, 0, T1), (2, 0, 31), (3, 0, T2 + 100), (4, 0, 1),
            (5, 0, 100), (6, 0, 4), (7, 0, T2), (8, 0, 9)]
    rows += [(10, 1, T1), (11, 1, 500), (12, 1, T2 + 7)]
    rows += [(v, 2, 1 + v % 9) for v in range(100)]
    rows += [(v, 4, 2 + v % 7) for v in range(20, 90)] + [(95, 4, 40)]
    g = _graph(300, rows, 44)
    part = _part(g, SHIFT)
    shape = [(b["n0"], b["n1"] > 0, b["nbig"] > 0) for b in part.blocks]
    assert shape == [(5, True, True), (0, True, True), (100, False, False),
                     (70, True, False)]
    info = _check_tables(part)
    assert [n for n, _ in info] == [5, 0, 100, 70]
    _both_checks(g, part, monkeypatch)


def test_stream_switch_equivalence():
    """LUX_PULL_STREAM=0 (thread per slot) and the stream role on the same
    partition: equal acc on the exact-integer sweep."""
    rows = [(v, 0, 1 + (7 * v) % 31) for v in range(200)]
    rows += [(v, 1, 31) for v in range(70)] + [(80, 1, 64), (81, 1, T2)]
    rows += [(v, 2, 3) for v in range(65)]
    g = _graph(256, rows, 45)
    part = _part(g, SHIFT)
    _check_tables(part)
    ints = np.random.default_rng(5).integers(0, 7, g.nv)
    old = torch.from_numpy(ints.astype(np.float32)).cuda()
    accs = []
    for stream in (False, True):
        acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
        run_pull_slots_sweeps(part, old, acc, stream=stream)
        accs.append(acc)
    torch.cuda.synchronize()
    assert accs[0].any()
    assert torch.equal(accs[0], accs[1])


def test_stream_switch_env(monkeypatch):
    """The engine reads LUX_PULL_STREAM where it reads LUX_PULL_SLOTS."""
    from lux_amd.engine import PagerankEngine
    g = _graph(256, [(v, v % 3, 1 + v % 6) for v in range(150)], 46)
    part = _part(g, SHIFT)
    monkeypatch.setenv("LUX_PULL_STREAM", "0")
    off = PagerankEngine(part)
    assert off._slots and not off._stream_role
    assert getattr(part, "stream_bytes", None) is None  # not built
    monkeypatch.setenv("LUX_PULL_STREAM", "1")
    on = PagerankEngine(part)
    assert on._stream_role and part.stream_bytes > 0
    for _ in range(4):
        off.step()
        on.step()
    assert torch.equal(off.ranks(), on.ranks())  # no hubs: every row
