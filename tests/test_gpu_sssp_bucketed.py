"""Bucketed (near-far delta-stepping) weighted SSSP on the GPU:
PushEngine(..., weighted=True, delta=D) and the one kernel the schedule
adds, ng.bucket_select. Every comparison is exact: labels must EQUAL the
CPU Dijkstra (lux_amd.cpu_ref.sssp_weighted), the select kernel's outputs a
numpy model of its per-vertex rule, and the engine's per-iteration trace
(limit, active set, push or pull, deferred count, bucket advances) what the
numpy simulation of the schedule gives (tests/bucketed_sssp_ref.py, checked
on its own in tests/test_sssp_bucketed_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bucketed_sssp_ref as bref  # noqa: E402
import weighted_sssp_ref as ref  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.push_engine import PushEngine  # noqa: E402
from lux_amd.types import DENSE_BITMAP, SPARSE_QUEUE  # noqa: E402

INF, SAT = ref.INF, ref.SAT
SMALL = (10, 8000, 3, 16)
WIDE = (12, 300000, 5, 1000)
MULTI = (11, 60000, 17, 16)


@functools.lru_cache(maxsize=None)
def _rmat(scale, ne, seed, wmax):
    """Host graph (one seed for edges and weights) and oracle labels;
    computed once, never modified."""
    g = Graph.rmat(scale, ne, seed=seed)
    g.hash_weights(wmax, seed=seed)
    return g, cpu_ref.sssp_weighted(g, 0)


@functools.lru_cache(maxsize=None)
def _ref(spec, delta):
    g, want = _rmat(*spec)
    lab, rows, advances, relaxed = bref.bucketed(g, 0, delta)
    assert np.array_equal(lab, want)
    return rows, advances, relaxed


def _engine(g, delta, weighted=True):
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    return PushEngine(part, PushEngine.MODE_MIN, source=0,
                      weighted=weighted, delta=delta)


def _labels(eng):
    return eng.final_labels().cpu().numpy().view(np.uint32)


def _trace(eng):
    return [(r["limit"], r["old_frontier"], r["volume"], r["pull_fallback"],
             r["deferred"]) for r in eng.stats]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1: the select kernel alone ----

VPS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 4097]
LIMITS = [0, 5, SAT]
GUARD = 0xABABABAB


def _select_inputs(vp, limit, kind):
    rng = np.random.default_rng(1000 * vp + limit % 997)
    special = np.array([INF, SAT, limit, min(limit + 1, INF), 0, 1, 4, 5, 6,
                        9], np.uint32)
    lab = special[rng.integers(0, len(special), vp)]
    snap = lab.copy()
    words = (vp + 63) // 64
    dirty = rng.integers(0, 2, 64 * words).astype(bool)
    if kind == "random":
        ch = rng.random(vp) < 0.3
        snap[ch] = lab[ch] + np.uint32(1 + rng.integers(0, 3))  # wraps: fine
    elif kind == "all_deferred":
        # every vertex dirty or changed, every label beyond the limit
        lab = (np.uint32(limit) + 1
               + rng.integers(0, 50, vp).astype(np.uint32))
        snap = lab.copy()
        ch = rng.random(vp) < 0.5
        snap[ch] = lab[ch] + np.uint32(7)
        dirty[:] = True
    else:
        assert kind == "advance"  # snapshot == labels: the pure reselect
    return snap, lab, dirty


def _run_select(vp, limit, replace, snap, lab, dirty):
    """Launch bucket_select on guarded buffers; returns the outputs and
    asserts that nothing outside them was written."""
    words = (vp + 63) // 64
    dirty_in = np.packbits(dirty, bitorder="little").view(np.uint32)
    assert len(dirty_in) == 2 * words
    d_dirty = _dev(np.concatenate([dirty_in,
                                   np.full(2, GUARD, np.uint32)]))
    seg_np = np.full(2 + 2 * words + 4, GUARD, np.uint32)
    seg_np[1] = 0  # numNodes preset; the type word is the fixup's
    d_seg = _dev(seg_np).view(torch.uint8)
    meta_np = np.array([11, 12, 13, 14, 15, 16, INF, 0], np.uint32)
    d_meta = _dev(meta_np)
    d_snap, d_lab = _dev(snap), _dev(lab)
    d_limit = _dev(np.array([limit], np.uint32))
    ng.bucket_select(torch.cuda.current_stream().cuda_stream, vp, d_snap,
                     d_lab, d_dirty, d_limit, replace, d_seg, d_meta)
    torch.cuda.synchronize()
    out_dirty, seg, meta = _host(d_dirty), _host(d_seg.view(torch.int32)), \
        _host(d_meta)
    assert np.array_equal(out_dirty[2 * words:], [GUARD, GUARD])
    assert np.array_equal(seg[2 + 2 * words:], [GUARD] * 4)
    assert seg[0] == GUARD
    assert np.array_equal(meta[:6], meta_np[:6])
    assert np.array_equal(_host(d_lab), lab)
    bitmap = seg[2:2 + 2 * words].view(np.uint8)
    return (out_dirty[:2 * words].view(np.uint8), bitmap, int(seg[1]),
            int(meta[6]), int(meta[7]), _host(d_snap))


def _select_model(vp, limit, replace, snap, lab, dirty):
    words = (vp + 63) // 64
    d = snap != lab
    if not replace:
        d = d | dirty[:vp]  # input bits at and beyond vp are ignored
    active = d & (lab <= np.uint32(limit))
    deferred = d & ~active
    pad = np.zeros(64 * words - vp, bool)  # bits beyond vp come out 0
    return (np.packbits(np.concatenate([deferred, pad]), bitorder="little"),
            np.packbits(np.concatenate([active, pad]), bitorder="little"),
            int(active.sum()),
            int(lab[deferred].min()) if deferred.any() else INF,
            int(deferred.sum()), lab.copy())


def _check_select(vp, limit, replace, kind):
    snap, lab, dirty = _select_inputs(vp, limit, kind)
    got = _run_select(vp, limit, replace, snap, lab, dirty)
    want = _select_model(vp, limit, replace, snap, lab, dirty)
    names = ["dirty", "bitmap", "numNodes", "meta[6]", "meta[7]", "snapshot"]
    for name, a, b in zip(names, got, want):
        assert np.array_equal(a, b), (name, a, b)
    return want


@pytest.mark.parametrize("replace", [False, True])
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("vp", VPS)
def test_select_kernel(vp, limit, replace):
    _check_select(vp, limit, replace, "random")


@pytest.mark.parametrize("vp", [1, 65, 1000, 4097])
def test_select_kernel_advance_case(vp):
    """snapshot == labels: push mode reselects from the dirty bits alone,
    pull mode (dirty = changed) selects nothing and clears dirty."""
    want = _check_select(vp, 5, False, "advance")
    assert want[2] > 0 or vp == 1
    want = _check_select(vp, 5, True, "advance")
    assert want[2] == 0 and want[4] == 0 and want[3] == INF
    assert not want[0].any()


@pytest.mark.parametrize("vp", [1, 129, 4097])
def test_select_kernel_all_deferred(vp):
    want = _check_select(vp, 5, False, "all_deferred")
    assert want[2] == 0 and want[4] == vp and 6 <= want[3] < INF


# ---- 2: hand cases ----

# (pad_to, LUX_PUSH_EVOL_DIV): at the graphs' own size every iteration is a
# pull (active 1 > nv // 16 = 0); padded to 64 vertices with the volume
# threshold at ne every iteration is a push
ROUTES = {"pull": (None, None), "push": (64, "1")}


@pytest.mark.parametrize("delta", [1, 2, 7])
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", sorted(ref.HAND_CASES))
def test_hand_cases(name, route, delta, monkeypatch):
    pad_to, div = ROUTES[route]
    monkeypatch.delenv("LUX_PUSH_EVOL_DIV", raising=False)
    if div:
        monkeypatch.setenv("LUX_PUSH_EVOL_DIV", div)
    g, want = ref.hand_graph(name, pad_to=pad_to)
    assert np.array_equal(cpu_ref.sssp_weighted(g, 0), want)
    lab, rows, advances, _ = bref.bucketed(g, 0, delta,
                                           evol_div=int(div or 8))
    assert np.array_equal(lab, want)
    eng = _engine(g, delta)
    eng.run(max_iters=len(rows) + 4)
    got = _labels(eng)
    assert np.array_equal(got, want), (got, want)
    assert eng.check() == 0
    assert _trace(eng) == rows
    assert eng.bucket_advances == advances
    assert {r["pull_fallback"] for r in eng.stats} == {route == "pull"}
    if name == "label_correction" and delta == 2:
        # 10 first, deferred; improved to 3 before its bucket came up
        assert got[1] == 3
    if name == "saturation" and delta == 7:
        assert eng.limit == SAT


# ---- 3: RMAT end to end ----

@pytest.mark.parametrize("spec,delta", [(SMALL, 4), (WIDE, 64)])
def test_rmat_end_to_end(spec, delta, monkeypatch):
    monkeypatch.delenv("LUX_PUSH_EVOL_DIV", raising=False)
    g, want = _rmat(*spec)
    rows, advances, relaxed = _ref(spec, delta)
    eng = _engine(g, delta)
    eng.run(max_iters=len(rows) + 4)
    assert np.array_equal(_labels(eng), want)
    assert eng.check() == 0
    assert [r["limit"] for r in eng.stats] == [r[0] for r in rows]
    assert [r["old_frontier"] for r in eng.stats] == [r[1] for r in rows]
    assert [r["pull_fallback"] for r in eng.stats] == [r[3] for r in rows]
    assert [r["deferred"] for r in eng.stats] == [r[4] for r in rows]
    assert eng.bucket_advances == advances and eng.iterations == len(rows)
    # the set selected right after iteration i is iteration i + 1's unless
    # an advance came between (then it was empty); it stays a bitmap
    # exactly when it does not fit the sparse queue
    dense = []
    for i, r in enumerate(eng.stats):
        same = i + 1 < len(rows) and rows[i + 1][0] == rows[i][0]
        nxt = rows[i + 1][1] if same else 0
        assert r["my_new"] == nxt, i
        assert r["out_dense"] == (nxt >= eng.capacity), i
        dense.append(r["out_dense"])
    if spec == WIDE:
        assert eng.capacity == 356 and dense.count(True) == 4
    assert True in [r[3] for r in rows] and False in [r[3] for r in rows]
    # relaxed edges: the active set's out-edges on a push, all on a pull
    got = sum(g.ne if r["pull_fallback"] else r["volume"]
              for r in eng.stats)
    _, sizes, vols = ref.bellman_ford(g, 0)
    flags = ref.predict_pull(g.nv, g.ne, sizes, vols)
    bf = sum(g.ne if f else v for f, v in zip(flags, vols))
    assert got == relaxed < bf


# ---- 4: a delta beyond every distance is today's engine ----

def test_large_delta_equals_plain_engine(monkeypatch):
    monkeypatch.delenv("LUX_PUSH_EVOL_DIV", raising=False)
    g, want = _rmat(*SMALL)
    plain = _engine(g, None)
    assert plain.delta == 0
    plain.run(max_iters=g.nv)
    big = _engine(g, 2 ** 31)
    big.run(max_iters=g.nv)
    assert np.array_equal(_labels(plain), want)
    assert np.array_equal(_labels(big), want)
    for key in ("old_frontier", "pull_fallback"):
        assert [r[key] for r in big.stats] == [r[key] for r in plain.stats]
    assert big.bucket_advances == 0 and plain.bucket_advances == 0
    assert {r["limit"] for r in big.stats} == {2 ** 31 - 1}
    # the plain engine's rows and pad words are what they were
    assert all("limit" not in r and "deferred" not in r
               for r in plain.stats)
    assert np.array_equal(_host(plain.meta_mine)[6:8], [0, 0])
    zero = _engine(g, 0)
    assert zero.delta == 0 and not hasattr(zero, "dirty")


# ---- 5: four partitions in one process ----

def test_bucketed_multipart_single_process(monkeypatch):
    """4 partitions in one process, the exchange done by hand as in
    test_weighted_multipart_single_process and extended to the advances:
    every engine advances from the same meta table, then the reselected
    segments are cross-copied.

    Label slices travel as in the real exchange: only a rank whose segment
    came out dense publishes its slice, the others' labels ride the annex.
    Whether the replicated labels count as fresh afterwards is the engine's
    own rule (PushEngine._labels_fresh) on the true meta table, and the
    catch-up copy (the engine's _sync_labels) happens only before a pull
    that finds them stale. A rank that changed labels and deferred them all
    reports count 0: taken for "changed nothing", its stale slice would
    reach a pull sweep — the rule is also checked directly at the end (on
    this input the traversal alone never meets that case)."""
    monkeypatch.delenv("LUX_PUSH_EVOL_DIV", raising=False)
    P, delta = 4, 4
    g, want = _rmat(*MULTI)
    rows, advances, _ = _ref(MULTI, delta)
    assert len(rows) == 10
    assert [i + 1 for i, r in enumerate(rows) if r[3]] == [2, 3, 4]
    full = DeviceCSC.from_host(g)
    parts = [GraphPart(full, P, p, keep_full=True) for p in range(P)]
    engines = [PushEngine(parts[p], PushEngine.MODE_MIN, source=0,
                          weighted=True, delta=delta) for p in range(P)]
    fresh = [True] * P
    seen = dict(syncs=0)

    def copy_labels(ei, published_only, mh):
        for j, ej in enumerate(engines):
            if parts[j].vp == 0 or (published_only
                                    and int(mh[j, 0]) != DENSE_BITMAP):
                continue
            ei.labels.narrow(0, parts[j].row_left,
                             parts[j].vp).copy_(ej.labels_part)

    def cross_copy():
        mh = np.stack([_host(e.meta_mine) for e in engines])
        for i, ei in enumerate(engines):
            copy_labels(ei, True, mh)
            for j, ej in enumerate(engines):
                if parts[j].vp == 0:
                    continue
                ei.fq_all.narrow(0, int(ei.seg_off[j]),
                                 ei.seg_bytes[j]).copy_(ej.new_seg)
                cap_j = int(ei.annex_off[j + 1] - ei.annex_off[j])
                ei.fq_annex_all.narrow(0, int(ei.annex_off[j]),
                                       cap_j).copy_(ej.new_annex[:cap_j])
            ei.meta_host = mh.copy()
            fresh[i] = ei._labels_fresh(fresh[i], mh)
            ei.headers = [(int(mh[q, 0]), int(mh[q, 1])) for q in range(P)]
        return mh

    def before_step():
        """The engine's _sync_labels, by hand: a pull reads every label."""
        for i, ei in enumerate(engines):
            pull = ei._bucket_decide()[3]
            if pull and not fresh[i]:
                copy_labels(ei, False, None)
                fresh[i] = True
                seen["syncs"] += 1
            ei.labels_current = True  # decided above; no collective here

    deferred = []
    for it in range(len(rows) + 4):
        before_step()
        for e in engines:
            e.step()
        mh = cross_copy()
        deferred.append(int(mh[:, 7].sum()))
        if engines[0].needs_advance():
            assert all(e.needs_advance() for e in engines)
            for e in engines:
                e.advance()
            mh = cross_copy()
            assert int(mh[:, 1].sum()) > 0
        if int(mh[:, 1].sum()) == 0 and not mh[:, 4].any() \
                and not mh[:, 7].any():
            break
    for ei in engines:
        copy_labels(ei, False, None)
    got = _host(engines[0].labels)
    assert np.array_equal(got, want)
    st = engines[0].stats
    assert [(r["limit"], r["old_frontier"], r["pull_fallback"])
            for r in st] == [(r[0], r[1], r[3]) for r in rows]
    assert deferred == [r[4] for r in rows]
    assert {e.bucket_advances for e in engines} == {advances}
    assert {e.limit for e in engines} == {rows[-1][0]}
    for e in engines:
        e.labels_current = True
    assert sum(e.check() for e in engines) == 0
    assert seen["syncs"] > 0, "no pull ever met stale labels"
    # the rule itself: every rank published but rank 1, whose set came out
    # sparse and empty with 5 vertices deferred. The plain engine reads
    # count 0 as "changed nothing"; here the slice is stale
    mh = np.zeros((P, 8), np.uint32)
    mh[:, 0] = DENSE_BITMAP
    mh[1, 0], mh[1, 1], mh[1, 7] = SPARSE_QUEUE, 0, 5
    plain = PushEngine(parts[0], PushEngine.MODE_MIN, source=0,
                       weighted=True)
    assert plain._labels_fresh(True, mh) is True
    assert engines[0]._labels_fresh(True, mh) is False
    mh[1, 0] = DENSE_BITMAP
    assert engines[0]._labels_fresh(False, mh) is True


def test_plain_multipart_counts_its_own_work_items():
    """The plain multi-partition step shares its expand and exchange
    helpers with the bucketed one: every push iteration still starts from
    a zeroed work-item counter (a vertex gives ceil(local out-degree /
    8192) items, so at most frontier + ep // 8192), and the trace is the
    synchronous Bellman-Ford's."""
    P = 4
    g, want = _rmat(*SMALL)
    _, sizes, _ = ref.bellman_ford(g, 0)
    # pushes: the seed, then the tail of 39 and 1 vertices — the last one
    # would still see the 39's items in an unzeroed counter
    assert sizes[-2:] == [39, 1] and g.nv // 16 == 64
    full = DeviceCSC.from_host(g)
    parts = [GraphPart(full, P, p, keep_full=True) for p in range(P)]
    engines = [PushEngine(parts[p], PushEngine.MODE_MIN, source=0,
                          weighted=True) for p in range(P)]
    pushes = 0
    for it in range(len(sizes) + 2):
        for e in engines:
            e.step()
            row = e.stats[-1]
            if not row["pull_fallback"]:
                pushes += 1
                items = int(_host(e.item_counter)[0])
                assert items <= row["old_frontier"] + e.part.ep // 8192, it
        mh = np.stack([_host(e.meta_mine) for e in engines])
        for ei in engines:
            for j, ej in enumerate(engines):
                if parts[j].vp == 0:
                    continue
                ei.labels.narrow(0, parts[j].row_left,
                                 parts[j].vp).copy_(ej.labels_part)
                ei.fq_all.narrow(0, int(ei.seg_off[j]),
                                 ei.seg_bytes[j]).copy_(ej.new_seg)
                cap_j = int(ei.annex_off[j + 1] - ei.annex_off[j])
                ei.fq_annex_all.narrow(0, int(ei.annex_off[j]),
                                       cap_j).copy_(ej.new_annex[:cap_j])
            ei.meta_host = mh.copy()
            ei.labels_current = True
            ei.headers = [(int(mh[q, 0]), int(mh[q, 1])) for q in range(P)]
        if int(mh[:, 1].sum()) == 0 and not mh[:, 4].any():
            break
    assert np.array_equal(_host(engines[0].labels), want)
    assert [r["old_frontier"] for r in engines[0].stats] == sizes
    assert pushes == 3 * P


# ---- 6: reset and replay ----

def test_reset_and_replay(monkeypatch):
    monkeypatch.delenv("LUX_PUSH_EVOL_DIV", raising=False)
    g, want = _rmat(*SMALL)
    rows, advances, _ = _ref(SMALL, 4)
    eng = _engine(g, 4)
    for rep in range(3):
        if rep:
            eng.reset()
        eng.run(max_iters=len(rows) + 4)
        assert np.array_equal(_labels(eng), want), rep
        assert _trace(eng) == rows, rep
        assert eng.bucket_advances == advances, rep
    # the later traversals replayed captured bodies, the advance's
    # select-only one included
    assert ("bucket", "select") in eng._graphs
    assert ("bucket", "push") in eng._graphs
    assert ("bucket", "pull") in eng._graphs
    assert eng.check() == 0


# ---- 7: the app driver and argument checks ----

def test_app_bucketed_synthetic(capsys):
    from lux_amd.apps import sssp
    eng = sssp.main(["-synthetic", "rmat:10:8000", "-weighted", "-wmax", "9",
                     "-delta", "3", "-check", "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out and "[PASS] 0 mistakes" in out
    header = [ln for ln in out.splitlines() if ln.startswith("deferred,")]
    assert header and "limit" in header[0].split(",")
    assert f"{eng.bucket_advances} bucket advances" in out
    assert eng.delta == 3 and eng.bucket_advances > 0
    g = Graph.rmat(10, 8000, seed=1)
    g.hash_weights(9)  # the builders' default seed
    assert np.array_equal(_labels(eng), cpu_ref.sssp_weighted(g, 0))


def test_delta_needs_weighted():
    from lux_amd.apps import sssp
    with pytest.raises(SystemExit):
        sssp.main(["-synthetic", "rmat:10:8000", "-delta", "3"])
    g, _ = _rmat(*SMALL)
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    with pytest.raises(ValueError):
        PushEngine(part, PushEngine.MODE_MIN, source=0, delta=3)
    with pytest.raises(ValueError):
        PushEngine(part, PushEngine.MODE_MIN, source=0, weighted=True,
                   delta=-1)
