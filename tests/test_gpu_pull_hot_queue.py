"""PageRank slot path, hot order, wide sweep off a work queue
(pull_slots_stream_hot_queue_kernel, LUX_PULL_HOT_QUEUE): the resident set of
1024-thread workgroups takes work items from a per-window counter, chunk items
first, then wave items, then stream items, and changes role without copying
its prefix again. The role bodies are the wide kernel's, so the reference is
the wide entry on the same tables: non-hub rows bit for bit, hub rows (atomics
in free order) at the project's tolerance.

The graph is test_gpu_pull_hot_wide's: window 0 has more than KW sources and
all three roles (7 hub chunks, 602 wave rows, over a hundred tiles), window 1
between KS and KW sources and no hub, window 2 1000 sources (fewer than KS),
no thread-bin row and one hub chunk. A launch over the first n entries of a
bin (or the first nt tiles) is a launch with that many entries, which is how
the item boundaries and the empty roles are reached."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_pull_slots import ATOL, RTOL, _hub_rows, _part  # noqa: E402
from test_gpu_pull_hot_wide import KS, KW, SHIFT, _build, _u32  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd.engine import (DeviceCSC, GraphPart, PagerankEngine,  # noqa
                            run_pull_slots_sweeps)

# items of pull.hip: WIDE_Q * QUEUE_C hub entries, WIDE_NW * QUEUE_R wave
# rows, WIDE_NW * QUEUE_T tiles
CHUNK = 8192
WIDE_Q, WIDE_NW = 4, 16
QUEUE_C, QUEUE_R, QUEUE_T = 1, 16, 1
PER = {"n2": WIDE_Q * QUEUE_C, "n1": WIDE_NW * QUEUE_R,
       "nt": WIDE_NW * QUEUE_T}
ENV = ("LUX_PULL_HOT", "LUX_PULL_HOT_LDS", "LUX_PULL_HOT_WIDE",
       "LUX_PULL_HOT_QUEUE", "LUX_PULL_SLOTS", "LUX_PULL_STREAM",
       "LUX_BLOCK_SHIFT")


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def case():
    """Partition with the hot tables built, a float gather table, and the
    rows that are a hub in some window (shared, never written)."""
    mp = pytest.MonkeyPatch()
    for k in ENV:
        mp.delenv(k, raising=False)
    try:
        g, _ = _build()
        part = _part(g, SHIFT)
        eng = PagerankEngine(part)  # builds the hot tables
    finally:
        mp.undo()
    assert eng._hot and eng._stream_role
    s = torch.cuda.current_stream().cuda_stream
    old = torch.from_numpy(
        np.random.default_rng(8).random(g.nv).astype(np.float32)).cuda()
    gold = torch.empty_like(old)
    ng.pull_hot_scatter(s, g.nv, part.pos, old, gold)
    active = _u32(part.active)[:part.na]
    hub = torch.from_numpy(_hub_rows(part)[active]).cuda()
    torch.cuda.synchronize()
    return dict(part=part, gold=gold, hub=hub)


def _items(n2, n1, nt):
    return -(-n2 // PER["n2"]) + -(-n1 // PER["n1"]) + -(-nt // PER["nt"])


def _window(case, w, queue, max_groups=0, **n):
    """One launch over window w with the bins cut to n[...] entries. Returns
    (acc, the queue's counter after the launch)."""
    part, gold = case["part"], case["gold"]
    src = dict(part.slot_srcs[w])
    for k, v in n.items():
        assert v <= src[k]
        src[k] = v
    s = torch.cuda.current_stream().cuda_stream
    acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
    head = (s, src["n0"], src["cidx0"], src["nt"], src["tile0"],
            src["off0"], src["hscol0"])
    bins = (src["n1"], src["cidx1"], src["rng1"], src["n2"], src["cidx2"],
            src["rng2"], src["hcol"])
    tail = (gold, acc, src["lo"], src["hi"], KS, KW)
    if not queue:
        ng.pull_slots_stream_hot_wide_iter(*head, *bins, *tail, max_groups)
        torch.cuda.synchronize()
        return acc, None
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    ng.pull_slots_stream_hot_queue_iter(*head, *bins, *tail,
                                        counter.data_ptr(), max_groups)
    torch.cuda.synchronize()
    return acc, int(counter.item())


def _same(case, got, want):
    hub = case["hub"]
    assert torch.equal(got[~hub], want[~hub])
    torch.testing.assert_close(got[hub], want[hub], rtol=RTOL, atol=ATOL)


def test_queue_graph_shape(case):
    """The windows hold what the cases below cut from."""
    srcs = case["part"].slot_srcs
    assert [s["hi"] - s["lo"] for s in srcs] == [1 << SHIFT, 1 << SHIFT, 1000]
    assert srcs[0]["n2"] > PER["n2"] and srcs[0]["n1"] > PER["n1"] \
        and srcs[0]["nt"] > PER["nt"] and srcs[0]["n0"]
    assert srcs[1]["n2"] == 0 and srcs[1]["n1"] and srcs[1]["nt"]
    assert srcs[2]["n0"] == 0 and srcs[2]["n1"] and srcs[2]["n2"] == 1
    assert case["hub"].sum() == 3 and (~case["hub"]).any()


# 1: one workgroup walks chunk -> wave -> stream and makes both role changes;
# 3: a few workgroups; 0: the resident set; 5000: far more workgroups than
# any window has items
@pytest.mark.parametrize("max_groups", [1, 3, 0, 5000])
def test_queue_sweep(case, max_groups):
    """All three windows (the short ones zero-fill their prefix past hi)
    through run_pull_slots_sweeps; every item is claimed exactly once."""
    part, gold = case["part"], case["gold"]
    want = torch.zeros(part.na, dtype=torch.float32, device="cuda")
    run_pull_slots_sweeps(part, gold, want, stream=True, hot=True,
                          hot_lds=2048, hot_wide=(KS, KW))
    got = torch.zeros_like(want)
    counters = torch.zeros(len(part.slot_srcs), dtype=torch.int32,
                           device="cuda")
    run_pull_slots_sweeps(part, gold, got, stream=True, hot=True,
                          hot_lds=2048, hot_wide=(KS, KW),
                          max_groups=max_groups, counters=counters)
    torch.cuda.synchronize()
    _same(case, got, want)
    items = [_items(s["n2"], s["n1"], s["nt"] if s["n0"] else 0)
             for s in part.slot_srcs]
    assert max(items) < 5000
    if max_groups:  # every workgroup claims one item past the end
        assert counters.tolist() == [i + max_groups for i in items]
    else:
        assert all(c > i for c, i in zip(counters.tolist(), items))


@pytest.mark.parametrize("empty", [("n2",), ("n1",), ("n0", "nt"),
                                   ("n2", "n1"), ("n2", "n1", "n0", "nt")])
@pytest.mark.parametrize("max_groups", [1, 7])
def test_queue_empty_roles(case, empty, max_groups):
    """Window 0 with each role empty in turn. ("n2", "n1"): the first item is
    a stream item, the workgroup copies KS sources only and the tile buffers
    lie over the rest. All empty: nothing is launched."""
    n = {k: 0 for k in empty}
    want, _ = _window(case, 0, False, **n)
    got, counter = _window(case, 0, True, max_groups, **n)
    _same(case, got, want)
    if len(empty) == 4:
        assert counter == 0 and not got.any()
    else:
        assert got.any() and counter > max_groups


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("role", ["n2", "n1", "nt"])
@pytest.mark.parametrize("max_groups", [1, 2])
def test_queue_item_boundaries(case, role, delta, max_groups):
    """One entry short of an item, exactly one item, one entry into the
    second item, for each role with the other two as they are."""
    n = {role: PER[role] + delta}
    want, _ = _window(case, 0, False, **n)
    got, counter = _window(case, 0, True, max_groups, **n)
    _same(case, got, want)
    src = dict(case["part"].slot_srcs[0], **n)
    assert counter == _items(src["n2"], src["n1"], src["nt"]) + max_groups


def test_queue_bad_prefix_pair(case):
    """A pair that is not instantiated raises and launches nothing."""
    part, gold = case["part"], case["gold"]
    acc = torch.zeros(part.na, dtype=torch.float32, device="cuda")
    counters = torch.zeros(len(part.slot_srcs), dtype=torch.int32,
                           device="cuda")
    for pair in ((2048, 4096), (KW, KS), (KS, 0)):
        with pytest.raises(ValueError):
            run_pull_slots_sweeps(part, gold, acc, stream=True, hot=True,
                                  hot_lds=2048, hot_wide=pair,
                                  counters=counters)
    torch.cuda.synchronize()
    assert not acc.any() and not counters.any()


def test_queue_engine(monkeypatch):
    """Default engine (queue) against LUX_PULL_HOT_QUEUE=0 on RMAT-13 in
    eight windows, five steps: steps 3 to 5 replay the captured graph, which
    has to clear the counters itself."""
    monkeypatch.setenv("LUX_BLOCK_SHIFT", "10")
    part = GraphPart(DeviceCSC.rmat(13, 400000, seed=5, device="cuda:0"),
                     1, 0)
    queue = PagerankEngine(part)
    # on the same partition: a second build of the tables orders them
    # differently, and row sums with them
    monkeypatch.setenv("LUX_PULL_HOT_QUEUE", "0")
    fixed = PagerankEngine(part)
    assert len(part.slot_srcs) == 8
    assert queue._hot_wide == fixed._hot_wide == (KS, KW)
    assert queue._counters.numel() == 8 and fixed._counters is None
    hub = torch.from_numpy(_hub_rows(part)).cuda()
    assert hub.any() and (~hub).any()
    # a hub of one chunk per window: no free atomic order that its out-edges
    # could carry into other rows at the next step
    assert max(int(np.diff(_u32(b["row_ptr"])).max())
               for b in part.blocks) <= CHUNK
    for it in range(1, 6):
        queue.step()
        fixed.step()
        a, b = queue.ranks(), fixed.ranks()
        assert torch.equal(a[~hub], b[~hub]), f"step {it}"
        torch.testing.assert_close(a[hub], b[hub], rtol=RTOL, atol=ATOL)
        assert (queue._counters > 0).all()
    assert queue._graph is not None and fixed._graph is not None
