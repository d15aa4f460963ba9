"""PageRank slot path: per-entry {compact row, edge range} streams, the
active-row accumulator, the one-launch-per-window sweep and the in-place
active-row epilogue, against exact integer sums, the row-table path
(LUX_PULL_SLOTS=0) in the same process, and the CPU reference."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import degree_ladder as dl  # noqa: E402

from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import (DeviceCSC, GraphPart, PagerankEngine,  # noqa
                            run_pull_slots_sweeps)
from lux_amd.graph import Graph  # noqa: E402

T2 = dl.T2
RTOL, ATOL = 2e-4, 1e-9  # the project's PageRank tolerance


def _indeg(g):
    return np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))


def _part(g, shift):
    """Single-rank partition of host graph g; shift=None: unblocked."""
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    if shift is None:
        part.build_bins()
        part.blocks = None
    else:
        part.prepare_pull(force_shift=shift)
        assert part.blocks
    return part


def _sweep_exact(part, g, seed=11):
    """One slot-path sweep over small-integer values: sums stay below 2^24,
    so fp32 is exact in any order; acc scattered back through `active` must
    EQUAL the integer sums, and rows outside `active` have sum 0."""
    assert part.prepare_pull_slots()
    nv, indeg = g.nv, _indeg(g)
    ints = np.random.default_rng(seed).integers(0, 7, nv)
    old = torch.from_numpy(ints.astype(np.float32)).cuda()
    acc = torch.zeros(max(part.na, 1), dtype=torch.float32, device="cuda")
    run_pull_slots_sweeps(part, old, acc)
    torch.cuda.synchronize()
    dst = np.repeat(np.arange(nv), indeg)
    want = np.bincount(dst, weights=ints[g.src].astype(np.float64),
                       minlength=nv)
    assert want.max(initial=0) < 2 ** 24
    active = part.active.cpu().numpy().view(np.uint32)[:part.na]
    assert np.array_equal(active, np.nonzero(indeg > 0)[0])
    got = np.zeros(nv)
    got[active] = acc.cpu().numpy()[:part.na]
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:8]} degrees {indeg[bad[:8]]}"
    inactive = np.setdiff1d(np.arange(nv), active)
    assert not want[inactive].any()


def _hub_rows(part):
    """Rows that are a hub (block-local in-degree >= T2) in any window:
    their chunk partials meet in atomics, in free order on both paths."""
    hub = np.zeros(part.vp, bool)
    srcs = part.blocks if part.blocks else [dict(row_ptr=part.row_ptr)]
    for blk in srcs:
        rp = blk["row_ptr"].cpu().numpy()
        rp = rp.view(np.uint32 if rp.dtype == np.int32 else np.uint64)
        hub |= np.diff(rp.astype(np.int64)) >= T2
    return hub


def _expected_inactive(eng, deg_np):
    ir = np.float32(eng.init_rank)
    return np.where(deg_np == 0, ir,
                    ir / np.maximum(deg_np, 1).astype(np.float32))


def _engines_agree(g, part, monkeypatch, steps=4):
    """Slot-path engine vs the row-table engine on the SAME partition (same
    edge order), step by step, then vs the CPU reference. Steps >= 3
    replay the captured graph."""
    slot = PagerankEngine(part)
    assert slot._slots and slot.new_part is None
    monkeypatch.setenv("LUX_PULL_SLOTS", "0")
    legacy = PagerankEngine(part)
    monkeypatch.delenv("LUX_PULL_SLOTS")
    assert not legacy._slots
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    deg_np = slot.deg.cpu().numpy()
    inactive = np.setdiff1d(
        np.arange(g.nv),
        part.active.cpu().numpy().view(np.uint32)[:part.na])
    assert torch.equal(slot.ranks(), legacy.ranks())
    rank0 = np.float32(1.0 / g.nv)
    init = np.where(deg_np == 0, rank0,
                    rank0 / np.maximum(deg_np, 1).astype(np.float32))
    np.testing.assert_allclose(slot.ranks().cpu().numpy()[inactive],
                               init[inactive], rtol=1e-6)
    want_inactive = _expected_inactive(slot, deg_np)[inactive]
    for it in range(1, steps + 1):
        slot.step()
        legacy.step()
        a, b = slot.ranks(), legacy.ranks()
        assert torch.equal(a[~hub], b[~hub]), f"step {it}"
        torch.testing.assert_close(a[hub], b[hub], rtol=RTOL, atol=ATOL)
        got = a.cpu().numpy()
        assert np.array_equal(got[inactive], want_inactive), f"step {it}"
        if it in (3, steps):
            np.testing.assert_allclose(got, cpu_ref.pagerank(g, it),
                                       rtol=RTOL, atol=ATOL)
    return slot


@functools.lru_cache(maxsize=None)
def _lad():
    return dl.plain_ladder()


@pytest.mark.parametrize("width", ["u32", "u64"])
def test_slots_sum_exact_ladder(width):
    """Every degree at which the thread / wave / chunk roles or the 4-deep
    pipeline change path, plus degree-0 (inactive) rows; blocked u32 row
    tables (4 windows) and the unblocked u64 table."""
    lad = _lad()
    part = _part(lad.g, dl.PLAIN_SHIFT if width == "u32" else None)
    if width == "u32":
        assert len(part.blocks) == dl.PLAIN_POOL_BLOCKS
    _sweep_exact(part, lad.g)
    assert part.na == (lad.degs > 0).sum() < lad.g.nv


def test_slots_same_bits_as_row_tables(monkeypatch):
    """RMAT-12, 2^16 edges, 256-vertex windows (16 windows, some sparse,
    many inactive rows, some deg == 0): non-hub rows bit-identical to the
    row-table path, hub rows and the CPU reference within tolerance,
    inactive rows at their constant; step 4 replays the graph twice."""
    scale, ne, seed = 12, 1 << 16, 21
    g = Graph.rmat(scale, ne, seed=seed)
    part = GraphPart(DeviceCSC.rmat(scale, ne, seed=seed), 1, 0)
    part.prepare_pull(force_shift=8)
    assert len(part.blocks) == 16
    slot = _engines_agree(g, part, monkeypatch, steps=4)
    assert slot._graph is not None
    assert 0 < part.na < g.nv
    assert (slot.deg == 0).any()


def test_slots_empty_graph():
    nv = 1024
    col_end = torch.zeros(nv, dtype=torch.int64, device="cuda")
    src = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng = PagerankEngine(GraphPart(DeviceCSC(nv, 0, col_end, src), 1, 0))
    assert eng._slots and eng.part.na == 0
    for _ in range(3):
        eng.step()
    assert np.array_equal(eng.ranks().cpu().numpy(),
                          np.full(nv, np.float32(eng.init_rank)))


def _random_graph(nv, ne, seed, src_hi=None, all_rows=False):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, src_hi or nv, ne)
    dst = rng.integers(0, nv // 2, ne)  # upper half: no in-edges
    if all_rows:
        dst[:nv] = np.arange(nv)
        dst[nv:] = rng.integers(0, nv, ne - nv)
    return Graph.from_edges(nv, src.astype(np.uint32), dst.astype(np.uint32))


def test_slots_single_source_window(monkeypatch):
    """Every edge comes from src window 0: the other 7 windows are dropped
    by the blocked build."""
    g = _random_graph(256, 3000, 31, src_hi=32)
    part = _part(g, 5)
    assert len(part.blocks) == 1
    _sweep_exact(part, g)
    _engines_agree(g, part, monkeypatch)


def test_slots_every_row_active(monkeypatch):
    g = _random_graph(256, 4000, 32, all_rows=True)
    part = _part(g, 6)
    _sweep_exact(part, g)
    assert part.na == g.nv
    _engines_agree(g, part, monkeypatch)


def test_slots_ragged_last_window(monkeypatch):
    """nv = 300 with 64-vertex windows: the last window is 44 wide."""
    g = _random_graph(300, 5000, 33)
    part = _part(g, 6)
    assert len(part.blocks) == 5
    _sweep_exact(part, g)
    _engines_agree(g, part, monkeypatch)


def test_slots_unblocked_engine(monkeypatch):
    """Small graphs stay unblocked (u64 row table): same contract."""
    g = _random_graph(300, 5000, 34)
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    _engines_agree(g, part, monkeypatch)
    assert part.blocks is None


def test_slots_merged_launch_roles(monkeypatch):
    """Windows whose bins are partly empty: the role offsets inside the
    one launch must not run a role past its list. Window 0: thread + chunk
    rows only (no wave bin); window 1: hubs only; window 2: thread + wave;
    window 3: wave only."""
    nv, w = 256, 64
    rows = [  # (dst row, src window, in-degree)
        (0, 1, 3000), (1, 0, 5), (2, 0, 2500), (3, 2, 40), (4, 2, 3),
        (5, 3, 100), (6, 1, 8200), (7, 0, 31), (8, 3, 2047)]
    rng = np.random.default_rng(35)
    src = np.concatenate([k * w + rng.integers(0, w, d) for _, k, d in rows])
    dst = np.concatenate([np.full(d, v) for v, _, d in rows])
    g = Graph.from_edges(nv, src.astype(np.uint32), dst.astype(np.uint32))
    part = _part(g, 6)
    shape = [(b["n0"] > 0, b["n1"] > 0, b["nbig"] > 0) for b in part.blocks]
    assert shape == [(True, False, True), (False, False, True),
                     (True, True, False), (False, True, False)]
    assert part.blocks[1]["n2"] == 1 + 2  # 3000 -> 1 chunk, 8200 -> 2
    _sweep_exact(part, g)
    _engines_agree(g, part, monkeypatch)


def test_slots_resume_rewrites_inactive_rows(tmp_path):
    """A checkpoint resume overwrites `old` wholesale (possibly with step-0
    state); the next step must restore the inactive rows' constant even
    though the captured graph never touches them."""
    from lux_amd import checkpoint
    g = _random_graph(300, 5000, 36)
    eng = PagerankEngine(_part(g, 6))
    path = str(tmp_path / "pr.ckpt")
    checkpoint.save_engine(path, eng)  # step-0 state
    for _ in range(3):
        eng.step()
    assert eng._graph is not None
    checkpoint.resume_engine(path, eng)
    for _ in range(2):
        eng.step()
    np.testing.assert_allclose(eng.ranks().cpu().numpy(),
                               cpu_ref.pagerank(g, 2), rtol=RTOL, atol=ATOL)
