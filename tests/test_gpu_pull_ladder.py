"""pull.hip on the plain degree ladder: every degree at which the thread,
wave and chunk kernels (or gather_range's 4-deep pipeline) change path,
for the u64 row pointers of the plain CSC and the u32 row pointers of the
src-blocked CSC, in all three modes. One sweep, exact expected values.

In the blocked build every ladder row draws its sources from ONE src
window (tests/degree_ladder.py), so its block-local degree is still the
ladder degree and the uint32_t instantiations of pull_thread_kernel,
pull_wave_kernel and pull_chunk_kernel each meet their bin edges."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import degree_ladder as dl  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd.engine import (DeviceCSC, GraphPart, run_pull,  # noqa: E402
                            run_pull_sweeps)

WIDTHS = ["u64", "u32"]
WHERES = ["first", "last", "chunk_last", "chunk_first"]
INF = dl.INF


@functools.lru_cache(maxsize=None)
def _lad(where):
    return dl.plain_ladder(marker=where)


@functools.lru_cache(maxsize=None)
def _part(where, width):
    lad = _lad(where)
    part = GraphPart(DeviceCSC.from_host(lad.g), 1, 0)
    if width == "u64":
        part.build_bins()
        assert getattr(part, "blocks", None) is None
        d = lad.degs
        assert part.n0 == ((d > 0) & (d < dl.T1)).sum()
        assert part.n1 == ((d >= dl.T1) & (d < dl.T2)).sum()
        assert part.nbig == (d >= dl.T2).sum()
        return part
    part.prepare_pull(force_shift=dl.PLAIN_SHIFT)
    # the 4 pool windows; the 4 windows nobody reads from are dropped
    assert part.blocks is not None
    assert len(part.blocks) == dl.PLAIN_POOL_BLOCKS >= 4
    rows = lad.ladder_rows
    for k, blk in enumerate(part.blocks):
        assert blk["row_u32"] == 1
        assert blk["row_ptr"].dtype == torch.int32
        local = np.diff(blk["row_ptr"].cpu().numpy().view(np.uint32))
        mine = rows[lad.row_block[rows] == k]
        theirs = rows[lad.row_block[rows] != k]
        assert np.array_equal(local[mine], lad.degs[mine])
        assert not local[theirs].any()
        assert blk["n0"] > 0 and blk["n1"] > 0 and blk["nbig"] > 0
    return part


def _labels(a):
    return torch.from_numpy(
        np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def _one_label_sweep(part, mode, old_np):
    old = _labels(old_np)
    new = torch.empty(part.vp, dtype=torch.int32, device="cuda")
    run_pull(part, mode, old, new, None, 0.0)  # seeds new with old
    torch.cuda.synchronize()
    return new.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("width", WIDTHS)
def test_pull_sum_exact(width):
    """PR_SUM sweep alone (no epilogue) over small-integer values into a
    zero-seeded output: sums stay below 2^24, so fp32 is exact in any
    order and the result must EQUAL the integer sums, chunk atomics
    included."""
    lad, part = _lad("last"), _part("last", width)
    nv = lad.g.nv
    ints = np.random.default_rng(11).integers(0, 7, nv)
    old = torch.from_numpy(ints.astype(np.float32)).cuda()
    new = torch.zeros(part.vp, dtype=torch.float32, device="cuda")
    deg = torch.zeros(nv, dtype=torch.int32, device="cuda")  # epilogue only
    run_pull_sweeps(part, ng.PULL_PR, old, new, deg, 0.0)
    torch.cuda.synchronize()
    want = dl.pull_sum_ref(lad, ints)
    assert want.max() < 2 ** 24
    got = new.cpu().numpy()
    bad = np.nonzero(got.astype(np.float64) != want)[0]
    assert len(bad) == 0, f"rows {bad[:8]} degrees {lad.degs[bad[:8]]}"


@pytest.mark.parametrize("width", WIDTHS)
def test_pull_pagerank_random(width):
    """Full PageRank iteration (seed, sweeps, epilogue) with random ranks
    against f64 at the project's PageRank tolerance."""
    lad, part = _lad("last"), _part("last", width)
    g = lad.g
    rng = np.random.default_rng(12)
    old_np = (rng.random(g.nv) / g.nv).astype(np.float32)
    outdeg = np.bincount(g.src, minlength=g.nv)
    init_rank = float(np.float32(0.85 / g.nv))
    old = torch.from_numpy(old_np).cuda()
    new = torch.empty(part.vp, dtype=torch.float32, device="cuda")
    deg = torch.from_numpy(outdeg.astype(np.int32)).cuda()
    run_pull(part, ng.PULL_PR, old, new, deg, init_rank)
    torch.cuda.synchronize()
    pr = init_rank + float(np.float32(0.15)) * dl.pull_sum_ref(lad, old_np)
    want = np.where(outdeg != 0, pr / np.maximum(outdeg, 1), pr)
    np.testing.assert_allclose(new.cpu().numpy(), want, rtol=2e-4,
                               atol=1e-9)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("where", WHERES)
def test_pull_min_exact(where, width):
    """LAB_MIN: new[v] = old[v] if settled, else min over sources of
    (INF if old[s] == INF else old[s] + 1)."""
    lad, part = _lad(where), _part(where, width)
    nv = lad.g.nv
    rows = lad.ladder_rows
    # (1) the only finite sources are the markers of windows 0 and 1, each
    # at exactly one edge per ladder row (first / last edge of the row or
    # of a chunk). Windows 2 and 3: every source INF -> stays INF, no wrap
    # of INF + 1 to 0. Some rows are settled and must keep their label even
    # though a source offers a smaller one.
    old = np.full(nv, INF, np.uint32)
    old[lad.markers[0]], old[lad.markers[1]] = 5, 9
    settled = rows[(rows % 8 < 3) & (lad.degs[rows] > 0)]
    old[settled] = 1000 + settled
    old[len(rows) + 3] = 77  # a settled filler row
    want = dl.pull_min_ref(lad, old)
    fresh = rows[(lad.degs[rows] > 0) & ~np.isin(rows, settled)]
    for k, lab in ((0, 6), (1, 10), (2, INF), (3, INF)):
        assert (want[fresh[lad.row_block[fresh] == k]] == lab).all()
    assert np.array_equal(want[settled], old[settled])
    got = _one_label_sweep(part, ng.PULL_MIN, old)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:8]} degrees {lad.degs[bad[:8]]}"
    # (2) random labels, 40% INF, settled and unsettled rows mixed
    rng = np.random.default_rng(13)
    old = rng.integers(0, 1000, nv).astype(np.uint32)
    old[rng.random(nv) < 0.4] = INF
    old[lad.markers] = [INF, 0, 2000, INF]
    got = _one_label_sweep(part, ng.PULL_MIN, old)
    want = dl.pull_min_ref(lad, old)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:8]} degrees {lad.degs[bad[:8]]}"


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("where", WHERES)
def test_pull_max_exact(where, width):
    """LAB_MAX: new[v] = max(old[v], max over sources of old[s]), with the
    unique row maximum held by the window's marker at the first / last
    edge of the row or of a chunk."""
    lad, part = _lad(where), _part(where, width)
    nv = lad.g.nv
    rows = lad.ladder_rows
    rng = np.random.default_rng(14)
    old = rng.integers(0, 1000, nv).astype(np.uint32)
    old[lad.markers] = 1000000 + np.arange(len(lad.markers))
    top = rows[rows % 5 == 0]
    old[top] = 2000000 + top  # own label already above every source
    want = dl.pull_max_ref(lad, old)
    low = rows[(lad.degs[rows] > 0) & (rows % 5 != 0)]
    assert np.array_equal(want[low], 1000000 + lad.row_block[low])
    assert np.array_equal(want[top], old[top])
    got = _one_label_sweep(part, ng.PULL_MAX, old)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:8]} degrees {lad.degs[bad[:8]]}"
