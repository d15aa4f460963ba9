"""PageRank slot path, hot order: inside every src window the sources are
ranked by out-degree (pos), the sweeps run on column copies holding
pos[col] and gather from gold[pos[v]] = old[v], and the epilogue keeps gold
current. Row sums read the same values in the same order as on the
id-ordered tables, so everything here is compared exactly: the order table
against a numpy lexsort, the column copies against pos[col], exact-integer
sweeps and whole engine runs against the id-ordered slot path
(LUX_PULL_HOT=0), the row-table path (LUX_PULL_SLOTS=0) and the CPU
reference, plus the state that reaches gold from outside a step (initial
ranks, the inactive rows' constants, a checkpoint resume). The stream role
additionally serves a window's hottest sources from LDS (LUX_PULL_HOT_LDS,
default 2048): 64-wide windows sit in that prefix whole, the 4096-wide ones
of _wide_graph reach past it, so both sides of its edge are compared too.

Graphs draw their sources with skewed weights per window, so out-degrees
are spread on purpose (hot, cold and never-gathered sources in one window)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_pull_slots import ATOL, RTOL, _hub_rows, _part  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import checkpoint, cpu_ref  # noqa: E402
from lux_amd.engine import PagerankEngine, run_pull_slots_sweeps  # noqa
from lux_amd.graph import Graph  # noqa: E402

T1, T2 = 32, 2048
SHIFT = 6
W = 1 << SHIFT  # src window width
NONE = 0xFFFFFFFF  # apos: row is never gathered

TABLE_KEYS = ("col", "scol0", "off0", "tile0", "cidx0", "cidx1", "cidx2",
              "rng0", "rng1", "rng2")


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in ("LUX_PULL_HOT", "LUX_PULL_HOT_LDS", "LUX_PULL_SLOTS",
              "LUX_PULL_STREAM", "LUX_BLOCK_SHIFT"):
        monkeypatch.delenv(k, raising=False)


def _graph(nv, rows, seed, dead=(), extra=(), w_=W):
    """rows: (dst row, src window, in-degree from that window). A window's
    sources are drawn with weights 1/(1+r), r a random rank of the source
    in its window: a few hot sources, many cold ones, some never drawn.
    dead: ids never drawn (out-degree 0 unless in extra); extra: explicit
    (src, dst) edges."""
    rng = np.random.default_rng(seed)
    weights = {}
    src, dst = [], []
    for v, k, d in rows:
        if k not in weights:
            ids = np.arange(k * w_, min((k + 1) * w_, nv))
            w = 1.0 / (1.0 + rng.permutation(len(ids)))
            w[np.isin(ids, dead)] = 0.0
            weights[k] = (ids, w / w.sum())
        ids, w = weights[k]
        src.append(rng.choice(ids, d, p=w))
        dst.append(np.full(d, v))
    if extra:
        src.append(np.array([s for s, _ in extra]))
        dst.append(np.array([d for _, d in extra]))
    return Graph.from_edges(nv, np.concatenate(src).astype(np.uint32),
                            np.concatenate(dst).astype(np.uint32))


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _outdeg(g):
    return np.bincount(g.src.astype(np.int64), minlength=g.nv)


def _want_pos(nv, outdeg, bounds):
    ids = np.arange(nv)
    win = np.searchsorted(np.asarray(bounds[1:-1]), ids, side="right")
    order = np.lexsort((ids, -outdeg, win))
    pos = np.empty(nv, np.int64)
    pos[order] = ids
    return pos


def _mixed_graph():
    """nv = 512, eight 64-wide windows. Thread-bin rows, wave-bin rows (32
    and 100 edges), hubs (>= 2048 edges from one window; 8200 = two chunks),
    sources with out-edges and no in-edge (every source drawn in windows 2,
    4, 6 and 7: no row from 128 to 191 or above 229 has an in-edge), rows
    with in-edges and out-degree 0 (dead), isolated vertices and an empty
    window (5: no source drawn, no row), a self-loop."""
    rows = [(v, 0, 1 + v % 9) for v in range(40)]
    rows += [(40, 0, T1), (41, 2, 100), (42, 0, T2 + 100), (43, 2, 8200)]
    rows += [(50, 1, 31), (51, 1, 64), (52, 4, 5), (53, 6, 40)]
    rows += [(v, 3, 2 + v % 7) for v in range(100, 128)]
    rows += [(v, 3, 1 + v % 5) for v in range(192, 200)]
    rows += [(v, 7, 3) for v in range(200, 230)]
    dead = (1, 5, 43, 100, 210)
    return _graph(512, rows, 51, dead=dead, extra=[(7, 7)]), dead


# ---------------- order table ----------------

def test_hot_order_table():
    """nv = 300: windows 0 and 3 skewed, window 1 without any out-edge,
    window 2 with every out-degree equal (3), window 4 ragged (44 wide)."""
    nv = 300
    rows = [(v, 0, 1 + v % 9) for v in range(60)]
    rows += [(v, 3, 2 + v % 5) for v in range(30, 120)] + [(5, 3, 200)]
    rows += [(v, 4, 1 + v % 4) for v in range(0, 50)] + [(6, 4, 90)]
    # window 2: source s -> rows s - 128, s - 127, s - 126 (mod 100)
    extra = [(s, (s - 128 + j) % 100) for s in range(128, 192)
             for j in range(3)]
    g = _graph(nv, rows, 50, extra=extra)
    part = _part(g, SHIFT)
    eng = PagerankEngine(part)
    assert eng._hot
    outdeg = _outdeg(g)
    assert np.array_equal(_u32(eng.deg), outdeg)
    bounds = part.hot_bounds()
    assert bounds == [0, 64, 128, 192, 256, 300]
    assert len(part.blocks) == 4  # window 1 is dropped by the blocked build
    pos = _u32(part.pos)
    assert np.array_equal(pos, _want_pos(nv, outdeg, bounds))
    assert np.array_equal(np.sort(pos), np.arange(nv))
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        p = pos[lo:hi]
        assert p.min() == lo and p.max() == hi - 1  # window kept
        by_pos = np.empty(hi - lo, np.int64)
        by_pos[p - lo] = outdeg[lo:hi]
        assert (np.diff(by_pos) <= 0).all()  # descending, zeros at the tail
    assert (outdeg[:64] == 0).any() and (outdeg[:64] > 0).any()
    assert not outdeg[64:128].any()
    assert (outdeg[128:192] == 3).all()
    ident = np.arange(nv)
    assert np.array_equal(pos[64:192], ident[64:192])
    assert not np.array_equal(pos[:64], ident[:64])
    assert not np.array_equal(pos[256:], ident[256:])
    # the epilogue's stream: pos of the active rows, none where deg == 0
    active = _u32(part.active)[:part.na]
    want = np.where(outdeg[active] > 0, pos[active], NONE)
    assert np.array_equal(_u32(part.apos)[:part.na], want)
    assert (want == NONE).any() and (want != NONE).any()


def test_hot_order_unblocked():
    """An unblocked CSC is one window: the order is global."""
    from lux_amd.engine import DeviceCSC, GraphPart
    g, _ = _mixed_graph()
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    eng = PagerankEngine(part)
    assert eng._hot and part.blocks is None
    assert part.hot_bounds() == [0, g.nv]
    assert np.array_equal(_u32(part.pos),
                          _want_pos(g.nv, _outdeg(g), [0, g.nv]))


# ---------------- column copies ----------------

def _snapshot(part):
    return [{k: None if src[k] is None else src[k].clone()
             for k in TABLE_KEYS} for src in part.slot_srcs]


def test_hot_column_copies():
    g, _ = _mixed_graph()
    part = _part(g, SHIFT)
    assert part.prepare_pull_slots()
    part.prepare_pull_stream()  # id-ordered scol0, as other engines use it
    before = _snapshot(part)
    stream_bytes = part.stream_bytes
    eng = PagerankEngine(part)
    assert eng._hot and eng._stream_role
    for _ in range(2):
        eng.step()
    torch.cuda.synchronize()
    pos = _u32(part.pos)
    assert len(part.slot_srcs) == 7
    for src, snap in zip(part.slot_srcs, before):
        for k in TABLE_KEYS:  # id-ordered and shared tables: bit for bit
            if snap[k] is None:
                assert src[k] is None, k
            else:
                assert torch.equal(src[k], snap[k]), k
        assert np.array_equal(_u32(src["hcol"]), pos[_u32(src["col"])])
        if src["n0"]:
            assert np.array_equal(_u32(src["hscol0"]),
                                  pos[_u32(src["scol0"])])
        else:
            assert src["hscol0"] is None
    assert part.stream_bytes > stream_bytes
    assert part.hot_bytes >= 4 * (g.ne + 2 * g.nv + part.na)


def test_hot_scol0_without_id_scol0():
    """The engine alone builds no id-ordered scol0; the hot one then comes
    straight from col. An id-ordered sweep afterwards still gets its own."""
    g, _ = _mixed_graph()
    part = _part(g, SHIFT)
    eng = PagerankEngine(part)
    assert eng._hot and eng._stream_role
    pos = _u32(part.pos)
    for src in part.slot_srcs:
        assert src["scol0"] is None
        n0 = src["n0"]
        if not n0:
            continue
        rng0 = _u32(src["rng0"])[:2 * n0].reshape(n0, 2)
        col = _u32(src["col"])
        want = np.concatenate([col[b:e] for b, e in rng0])
        assert np.array_equal(_u32(src["hscol0"]), pos[want])
    hot_bytes = part.hot_bytes
    part.prepare_pull_stream()
    assert part.hot_bytes == hot_bytes
    for src in part.slot_srcs:
        if src["n0"]:
            assert np.array_equal(pos[_u32(src["scol0"])],
                                  _u32(src["hscol0"]))


# ---------------- exact-integer sweep ----------------

@pytest.mark.parametrize("stream", [False, True])
def test_hot_sweep_exact(stream):
    """Integer-valued ranks: every sum is exact, so acc of the hot-order
    sweeps equals acc of the id-order sweeps on every row, hubs included."""
    g, _ = _mixed_graph()
    part = _part(g, SHIFT)
    eng = PagerankEngine(part)  # builds the hot tables
    assert eng._hot
    ints = np.random.default_rng(6).integers(0, 7, g.nv)
    old = torch.from_numpy(ints.astype(np.float32)).cuda()
    gold = torch.full((g.nv,), -1.0, dtype=torch.float32, device="cuda")
    ng.pull_hot_scatter(torch.cuda.current_stream().cuda_stream, g.nv,
                        part.pos, old, gold)
    pos = torch.from_numpy(_u32(part.pos)).cuda()
    assert torch.equal(gold[pos], old)
    accs = []
    # the LDS prefix (stream role only) holds whole 64-wide windows here
    for hot, table, lds in ((False, old, 0), (True, gold, 0),
                            (True, gold, 2048), (True, gold, 4096)):
        acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
        run_pull_slots_sweeps(part, table, acc, stream=stream, hot=hot,
                              hot_lds=lds)
        accs.append(acc)
    torch.cuda.synchronize()
    indeg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    want = np.bincount(np.repeat(np.arange(g.nv), indeg),
                       weights=ints[g.src].astype(np.float64),
                       minlength=g.nv)
    assert want.max() < 2 ** 24
    active = _u32(part.active)[:part.na]
    assert np.array_equal(accs[0].cpu().numpy(), want[active])
    for acc in accs[1:]:
        assert torch.equal(accs[0], acc)


# ---------------- hot prefix in LDS ----------------

def _wide_graph():
    """4096-wide windows, nv = 2 * 4096 + 1000: windows 0 and 1 have more
    gathered sources than the LDS prefix holds (both sides of the prefix
    edge are read), window 2 is narrower than the prefix."""
    rows = [(v, 0, 40) for v in range(600)] + [(5000, 0, T2 + 1000)]
    rows += [(v, 1, 1 + v % 30) for v in range(1500)] + [(5001, 1, 100)]
    rows += [(v, 2, 3) for v in range(300)]
    return _graph(2 * 4096 + 1000, rows, 52, w_=4096)


def test_hot_lds_prefix_sweep():
    """Exact-integer sweep: id order = hot order = hot order with 2048 / 4096
    sources of every window from LDS."""
    g = _wide_graph()
    part = _part(g, 12)
    outdeg = _outdeg(g)
    assert (outdeg[:4096] > 0).sum() > 2048 < (outdeg[4096:8192] > 0).sum()
    eng = PagerankEngine(part)
    assert eng._hot and eng._hot_lds == 2048
    assert [(s["lo"], s["hi"]) for s in part.slot_srcs] == \
        [(0, 4096), (4096, 8192), (8192, 9192)]
    ints = np.random.default_rng(7).integers(0, 7, g.nv)
    old = torch.from_numpy(ints.astype(np.float32)).cuda()
    gold = torch.empty_like(old)
    ng.pull_hot_scatter(torch.cuda.current_stream().cuda_stream, g.nv,
                        part.pos, old, gold)
    accs = []
    for hot, table, lds in ((False, old, 0), (True, gold, 0),
                            (True, gold, 2048), (True, gold, 4096)):
        acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
        run_pull_slots_sweeps(part, table, acc, stream=True, hot=hot,
                              hot_lds=lds)
        accs.append(acc)
    torch.cuda.synchronize()
    assert accs[0].any()
    for acc in accs[1:]:
        assert torch.equal(accs[0], acc)


def test_hot_lds_prefix_engine(monkeypatch):
    """Default engine (2048 sources from LDS) vs LUX_PULL_HOT_LDS=0 vs the
    row-table path, 4 steps; LUX_PULL_STREAM=0 has no LDS prefix."""
    g = _wide_graph()
    part = _part(g, 12)
    lds = PagerankEngine(part)
    monkeypatch.setenv("LUX_PULL_HOT_LDS", "0")
    plain = PagerankEngine(part)
    monkeypatch.setenv("LUX_PULL_HOT_LDS", "2048")
    monkeypatch.setenv("LUX_PULL_STREAM", "0")
    thread = PagerankEngine(part)
    monkeypatch.delenv("LUX_PULL_STREAM")
    monkeypatch.setenv("LUX_PULL_SLOTS", "0")
    legacy = PagerankEngine(part)
    assert (lds._hot_lds, plain._hot_lds, thread._hot_lds) == (2048, 0, 0)
    assert plain._hot and thread._hot and not legacy._hot
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    for it in range(1, 5):
        for eng in (lds, plain, thread, legacy):
            eng.step()
        a = lds.ranks()
        for other in (plain, thread, legacy):
            b = other.ranks()
            assert torch.equal(a[~hub], b[~hub]), f"step {it}"
            torch.testing.assert_close(a[hub], b[hub], rtol=RTOL, atol=ATOL)
    assert lds._graph is not None
    np.testing.assert_allclose(a.cpu().numpy(), cpu_ref.pagerank(g, 4),
                               rtol=RTOL, atol=ATOL)


# ---------------- engines ----------------

def _check_mixed(g, part, dead):
    """The mixed graph holds every kind of row and source the issue names."""
    outdeg = _outdeg(g)
    indeg = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    degs = np.concatenate([np.diff(_u32(blk["row_ptr"]))
                           for blk in part.blocks])  # per window and row
    assert ((degs > 0) & (degs < T1)).any()
    assert (degs == T1).any() and (degs == 100).any()
    assert (degs >= T2).any()
    assert ((outdeg > 0) & (indeg == 0)).any()
    assert all(indeg[v] > 0 and outdeg[v] == 0 for v in dead)
    assert ((outdeg == 0) & (indeg == 0)).any()
    assert not outdeg[5 * W:6 * W].any()  # empty window
    assert len(part.blocks) == 7
    srcs = g.src.astype(np.int64)
    dsts = np.repeat(np.arange(g.nv), indeg)
    assert ((srcs == 7) & (dsts == 7)).any()  # self-loop


@pytest.mark.parametrize("stream", ["1", "0"])
def test_hot_engine_equivalence(monkeypatch, stream):
    """Hot order vs LUX_PULL_HOT=0 vs LUX_PULL_SLOTS=0 on one partition,
    step by step (steps >= 3 replay the captured graph), non-hub rows bit
    for bit; ranks() stays in id order; CPU reference at the project's
    tolerance; gold is the permuted `old` where it is gathered."""
    monkeypatch.setenv("LUX_PULL_STREAM", stream)
    g, dead = _mixed_graph()
    part = _part(g, SHIFT)
    _check_mixed(g, part, dead)
    hot = PagerankEngine(part)
    monkeypatch.setenv("LUX_PULL_HOT", "0")
    plain = PagerankEngine(part)
    monkeypatch.setenv("LUX_PULL_SLOTS", "0")
    legacy = PagerankEngine(part)
    monkeypatch.delenv("LUX_PULL_SLOTS")
    monkeypatch.delenv("LUX_PULL_HOT")
    assert hot._hot and hot._slots
    assert plain._slots and not plain._hot and not hasattr(plain, "gold")
    assert not legacy._slots and not legacy._hot
    assert hot._stream_role == plain._stream_role == (stream == "1")
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    assert hub.any()
    pos = torch.from_numpy(_u32(part.pos)).cuda()
    gathered = hot.deg != 0
    for it in range(1, 5):
        for eng in (hot, plain, legacy):
            eng.step()
        a = hot.ranks()
        for other in (plain, legacy):
            b = other.ranks()
            assert torch.equal(a[~hub], b[~hub]), f"step {it}"
            torch.testing.assert_close(a[hub], b[hub], rtol=RTOL, atol=ATOL)
        if it >= 2:  # step 1's constants reach gold before step 2's sweeps
            assert torch.equal(hot.gold[pos][gathered], a[gathered])
        if it >= 3:
            np.testing.assert_allclose(a.cpu().numpy(),
                                       cpu_ref.pagerank(g, it), rtol=RTOL,
                                       atol=ATOL)
    assert hot._graph is not None and plain._graph is not None


# ---------------- state ----------------

def _four_steps(part):
    eng = PagerankEngine(part)
    for _ in range(4):
        eng.step()
    return eng.ranks().clone()


def test_hot_ranks_between_steps():
    g, _ = _mixed_graph()
    part = _part(g, SHIFT)
    want = _four_steps(part)
    eng = PagerankEngine(part)
    seen = []
    for _ in range(4):
        eng.step()
        seen.append(eng.ranks().clone())
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    assert torch.equal(eng.ranks()[~hub], want[~hub])
    torch.testing.assert_close(eng.ranks()[hub], want[hub], rtol=RTOL,
                               atol=ATOL)
    assert not torch.equal(seen[0], seen[3])


def test_hot_checkpoint_resume(tmp_path):
    """Save after 2 steps, resume into a fresh engine, 2 more steps: the
    restored `old` must reach gold before the first sweep."""
    g, _ = _mixed_graph()
    part = _part(g, SHIFT)
    want = _four_steps(part)
    first = PagerankEngine(part)
    for _ in range(2):
        first.step()
    path = str(tmp_path / "pr.ckpt")
    checkpoint.save_engine(path, first, iteration=2)
    fresh = PagerankEngine(part)
    assert fresh._hot
    fresh.step()  # gold now holds other values than the checkpoint's
    assert checkpoint.resume_engine(path, fresh) == 2
    for _ in range(2):
        fresh.step()
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    got = fresh.ranks()
    assert torch.equal(got[~hub], want[~hub])
    torch.testing.assert_close(got[hub], want[hub], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got.cpu().numpy(), cpu_ref.pagerank(g, 4),
                               rtol=RTOL, atol=ATOL)


# ---------------- switch ----------------

def test_hot_switch_env(monkeypatch):
    g, _ = _mixed_graph()
    part = _part(g, SHIFT)
    monkeypatch.setenv("LUX_PULL_HOT", "0")
    off = PagerankEngine(part)
    assert off._slots and not off._hot
    assert getattr(part, "pos", None) is None
    assert not getattr(part, "hot_bytes", 0)
    assert all("hcol" not in s and "hscol0" not in s
               for s in part.slot_srcs)
    monkeypatch.delenv("LUX_PULL_HOT")
    on = PagerankEngine(part)
    assert on._hot and part.hot_bytes > 0
    assert part.pos is not None and part.apos is not None
    assert all(s["hcol"] is not None for s in part.slot_srcs)
    assert any(s["hscol0"] is not None for s in part.slot_srcs)
