"""PageRank slot path, hot order, wide sweep: 1024-thread workgroups that
keep KS = 8192 (stream role) or KW = 16384 (wave and chunk roles) of a
window's hottest sources in LDS, on a grid of a few resident workgroups whose
role loops grid-stride (LUX_PULL_HOT_WIDE). Row sums of the stream and wave
roles and every chunk partial are the floats the 256-thread kernel gives, so
non-hub rows are compared bit for bit and hub rows (atomics in free order) at
the project's tolerance.

One graph serves every test: 2^15-wide windows, nv = 2 * 32768 + 1000.
  window 0: more than KW sources with an out-edge; thread rows, wave rows,
            hubs of 8200 and 4 * 8192 + 100 edges (2 + 5 = 7 chunks: with four
            quarters per workgroup one idles through the barriers)
  window 1: between KS and KW sources with an out-edge; no hub
  window 2: ragged, 1000 sources (fewer than KS); no thread-bin row; a hub of
            2148 edges
Sources are drawn as in test_gpu_pull_hot._graph (skewed weights over a random
ranking, some ids never drawn), with a flatter skew so that the sources around
position KW still have a handful of out-edges. The sources at positions
lo + KS - 1, lo + KS, lo + KW - 1 and lo + KW of window 0 are then each made a
source of a thread-bin row, wave-bin rows of 32 and 100 edges and the large
hub by swapping edge destinations, which leaves every in- and out-degree, and
so the hot order, as drawn. The hub rows are ids that are never drawn as a
source: a hub of more than two chunks is summed by atomics in free order, and
with an out-edge its rank would carry that difference into other rows at the
next step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_pull_slots import ATOL, RTOL, _hub_rows, _part  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd.engine import PagerankEngine, run_pull_slots_sweeps  # noqa
from lux_amd.graph import Graph  # noqa: E402

T1, T2, CHUNK = 32, 2048, 8192
KS, KW = 8192, 16384
SHIFT = 15
W = 1 << SHIFT
NV = 2 * W + 1000
# window 0's special rows: thread bin, wave bin (32 and 100 edges), hub
ROW_T, ROW_W32, ROW_W100, ROW_HUB = 20000, 20001, 20002, 25004
SPECIAL = (ROW_T, ROW_W32, ROW_W100, ROW_HUB)
EDGE_VALUES = (11, 13, 17, 19)  # of the four sources at the prefix edges


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in ("LUX_PULL_HOT", "LUX_PULL_HOT_LDS", "LUX_PULL_HOT_WIDE",
              "LUX_PULL_SLOTS", "LUX_PULL_STREAM", "LUX_BLOCK_SHIFT"):
        monkeypatch.delenv(k, raising=False)


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _window(rng, k, rows, drawn, c):
    """rows: (dst row, in-degree from window k). Sources: the window's first
    `drawn` ids, weights 1 / (c + r), r a random rank."""
    ids = np.arange(k * W, min((k + 1) * W, NV))[:drawn]
    w = 1.0 / (c + rng.permutation(len(ids)))
    dst = np.repeat([v for v, _ in rows], [d for _, d in rows])
    return rng.choice(ids, len(dst), p=w / w.sum()), dst


def _hot_positions(outdeg, lo, hi):
    """ids of the window's sources in hot order (out-degree descending, ties
    by ascending id)."""
    ids = np.arange(lo, hi)
    return ids[np.lexsort((ids, -outdeg[lo:hi]))]


def _build():
    rng = np.random.default_rng(53)
    rows0 = [(v, 1 + v % 31) for v in range(10000)]
    rows0 += [(v, T1 + (v * 37) % 400) for v in range(10000, 10600)]
    rows0 += [(ROW_T, 20), (ROW_W32, T1), (ROW_W100, 100), (25003, 8200),
              (ROW_HUB, 4 * CHUNK + 100)]
    rows1 = [(v, 1 + v % 20) for v in range(6000)]
    rows1 += [(v, T1 + v % 150) for v in range(30000, 30200)]
    rows2 = [(v, 100) for v in range(40000, 40050)] + [(50000, T2 + 100)]
    src0, dst0 = _window(rng, 0, rows0, 22000, 4096)
    src1, dst1 = _window(rng, 1, rows1, 12000, 4096)
    src2, dst2 = _window(rng, 2, rows2, 1000, 64)
    # the sources at the prefix edges of window 0 become sources of the
    # special rows: swap destinations with an edge those rows already have
    outdeg0 = np.bincount(src0, minlength=W)
    order = _hot_positions(outdeg0, 0, W)
    edge_srcs = order[[KS - 1, KS, KW - 1, KW]]
    assert outdeg0[edge_srcs].min() >= len(SPECIAL)
    used = np.zeros(len(src0), bool)
    special = np.isin(dst0, SPECIAL)
    at_edge = np.isin(src0, edge_srcs)
    for a in edge_srcs:
        for r in SPECIAL:
            i = np.flatnonzero((src0 == a) & ~special & ~used)[0]
            j = np.flatnonzero((dst0 == r) & ~at_edge & ~used)[0]
            dst0[i], dst0[j] = dst0[j], dst0[i]
            used[i] = used[j] = True
    for a in edge_srcs:
        assert set(SPECIAL) <= set(dst0[src0 == a])
    assert np.array_equal(np.bincount(src0, minlength=W), outdeg0)
    src = np.concatenate([src0, src1, src2]).astype(np.uint32)
    dst = np.concatenate([dst0, dst1, dst2]).astype(np.uint32)
    return Graph.from_edges(NV, src, dst), edge_srcs


@pytest.fixture(scope="module")
def case():
    """Graph, partition with the hot tables built, and reference sweeps over
    small-integer and over float values (shared, never written)."""
    mp = pytest.MonkeyPatch()
    for k in ("LUX_PULL_HOT", "LUX_PULL_HOT_LDS", "LUX_PULL_HOT_WIDE",
              "LUX_PULL_SLOTS", "LUX_PULL_STREAM", "LUX_BLOCK_SHIFT"):
        mp.delenv(k, raising=False)
    try:
        g, edge_srcs = _build()
        part = _part(g, SHIFT)
        eng = PagerankEngine(part)  # builds the hot tables
    finally:
        mp.undo()
    assert eng._hot and eng._stream_role
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(8)
    ints = rng.integers(0, 7, g.nv)
    ints[edge_srcs] = EDGE_VALUES
    tables = {}
    for name, vals in (("int", ints.astype(np.float32)),
                       ("float", rng.random(g.nv).astype(np.float32))):
        old = torch.from_numpy(vals).cuda()
        gold = torch.empty_like(old)
        ng.pull_hot_scatter(s, g.nv, part.pos, old, gold)
        acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
        run_pull_slots_sweeps(part, gold, acc, stream=True, hot=True,
                              hot_lds=2048)
        tables[name] = (old, gold, acc)
    torch.cuda.synchronize()
    return dict(g=g, part=part, edge_srcs=edge_srcs, ints=ints, **tables)


def _wide(case, gold, max_groups=0, pair=(KS, KW)):
    part = case["part"]
    acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
    run_pull_slots_sweeps(part, gold, acc, stream=True, hot=True,
                          hot_lds=2048, hot_wide=pair, max_groups=max_groups)
    torch.cuda.synchronize()
    return acc


def test_wide_graph_shape(case):
    """The graph holds what the sweeps below rely on."""
    g, part = case["g"], case["part"]
    outdeg = np.bincount(g.src.astype(np.int64), minlength=g.nv)
    srcs = part.slot_srcs
    assert [(s["lo"], s["hi"]) for s in srcs] == \
        [(0, W), (W, 2 * W), (2 * W, NV)]
    assert (outdeg[:W] > 0).sum() > KW
    assert not outdeg[[25003, ROW_HUB, 50000]].any()
    assert KS < (outdeg[W:2 * W] > 0).sum() < KW
    assert NV - 2 * W < KS
    # roles per window: 7 chunks (not a multiple of 4) / no hub / no thread
    # bin and one chunk
    assert [s["n2"] for s in srcs] == [7, 0, 1]
    assert srcs[0]["n0"] and srcs[0]["n1"] and srcs[1]["n0"] \
        and srcs[1]["n1"]
    assert srcs[2]["n0"] == 0 and srcs[2]["n1"] == 50
    # the special rows sit in the bins they are named for
    blk0 = np.diff(_u32(part.blocks[0]["row_ptr"]))
    assert blk0[ROW_T] == 20 and blk0[ROW_W32] == T1
    assert blk0[ROW_W100] == 100 and blk0[ROW_HUB] == 4 * CHUNK + 100
    assert blk0[25003] == 8200
    blk2 = np.diff(_u32(part.blocks[2]["row_ptr"]))
    assert blk2[50000] == T2 + 100
    # the four sources sit at the prefix edges of window 0
    pos = _u32(part.pos)
    assert list(pos[case["edge_srcs"]]) == [KS - 1, KS, KW - 1, KW]
    assert len(set(case["ints"][case["edge_srcs"]])) == 4


@pytest.mark.parametrize("max_groups", [0, 3, 4])
def test_wide_sweep_exact(case, max_groups):
    """Integer-valued ranks: every sum is exact, so id order = hot order =
    hot order with 2048 sources from LDS = the wide kernel, on the resident
    grid and on grids of one or two workgroups per role."""
    g, part = case["g"], case["part"]
    old, gold, acc_2048 = case["int"]
    accs = [acc_2048, _wide(case, gold, max_groups)]
    for hot, table in ((False, old), (True, gold)):
        acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
        run_pull_slots_sweeps(part, table, acc, stream=True, hot=hot)
        accs.append(acc)
    torch.cuda.synchronize()
    indeg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    want = np.bincount(np.repeat(np.arange(g.nv), indeg),
                       weights=case["ints"][g.src].astype(np.float64),
                       minlength=g.nv)
    assert want.max() < 2 ** 24
    active = _u32(part.active)[:part.na]
    assert np.array_equal(accs[0].cpu().numpy(), want[active])
    for acc in accs[1:]:
        assert torch.equal(accs[0], acc)


@pytest.mark.parametrize("max_groups", [0, 3, 4])
def test_wide_sweep_float(case, max_groups):
    """Float values: non-hub rows bit-equal to the 2048 kernel's, hub rows
    within the project's tolerance."""
    part = case["part"]
    _, gold, acc_2048 = case["float"]
    acc = _wide(case, gold, max_groups)
    active = _u32(part.active)[:part.na]
    hub = torch.from_numpy(_hub_rows(part)[active]).cuda()
    assert hub.sum() == 3 and (~hub).any()
    assert torch.equal(acc[~hub], acc_2048[~hub])
    torch.testing.assert_close(acc[hub], acc_2048[hub], rtol=RTOL, atol=ATOL)


def test_wide_bad_prefix_pair(case):
    """A pair that is not instantiated raises and launches nothing."""
    part = case["part"]
    _, gold, _ = case["int"]
    acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
    for pair in ((2048, 4096), (KW, KS), (KS, 0)):
        with pytest.raises(ValueError):
            run_pull_slots_sweeps(part, gold, acc, stream=True, hot=True,
                                  hot_lds=2048, hot_wide=pair)
    torch.cuda.synchronize()
    assert not acc.any()


def test_wide_engine(case, monkeypatch):
    """Default engine (wide sweep) vs LUX_PULL_HOT_WIDE=0, three steps (the
    third replays the captured graph); gold stays the permuted `old`."""
    part = case["part"]
    assert PagerankEngine(part)._hot_wide == (KS, KW)
    monkeypatch.setenv("LUX_PULL_HOT_WIDE", "1")
    wide = PagerankEngine(part)
    monkeypatch.setenv("LUX_PULL_HOT_WIDE", "0")
    narrow = PagerankEngine(part)
    assert wide._hot_wide == (KS, KW) and wide._hot_lds == 2048
    assert narrow._hot_wide is None and narrow._hot_lds == 2048
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    pos = torch.from_numpy(_u32(part.pos)).cuda()
    gathered = wide.deg != 0
    for it in range(1, 4):
        wide.step()
        narrow.step()
        a, b = wide.ranks(), narrow.ranks()
        assert torch.equal(a[~hub], b[~hub]), f"step {it}"
        torch.testing.assert_close(a[hub], b[hub], rtol=RTOL, atol=ATOL)
        if it >= 2:  # step 1's constants reach gold before step 2's sweeps
            assert torch.equal(wide.gold[pos][gathered], a[gathered])
    assert wide._graph is not None
