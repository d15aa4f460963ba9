"""Weighted SSSP on the GPU: PushEngine(..., weighted=True) — min-plus push
scatter over the interleaved {dst, weight} CSR, weighted dense pull
fallback (plain and src-blocked CSC), weighted check oracle, device hash
weights. Every comparison is exact: labels must EQUAL the CPU Dijkstra
(lux_amd.cpu_ref.sssp_weighted), and where a test asserts engine decisions
they must equal what the numpy Bellman-Ford simulation predicts
(tests/weighted_sssp_ref.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import degree_ladder as dl  # noqa: E402
import weighted_sssp_ref as ref  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart, run_pull  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.push_engine import PushEngine  # noqa: E402

INF = ref.INF
RMATS = [(10, 8000, 3, 16), (12, 300000, 5, 16)]


@functools.lru_cache(maxsize=None)
def _rmat(scale, ne, seed, wmax):
    """Host graph (one seed for edges and weights), oracle labels and the
    predicted frontier trace; computed once, never modified."""
    g = Graph.rmat(scale, ne, seed=seed)
    g.hash_weights(wmax, seed=seed)
    want = cpu_ref.sssp_weighted(g, 0)
    bf, sizes, vols = ref.bellman_ford(g, 0)
    assert np.array_equal(bf, want)
    return g, want, sizes, vols


def _engine(g, weighted=True, source=0):
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    return PushEngine(part, PushEngine.MODE_MIN, source=source,
                      weighted=weighted)


def _labels(eng):
    return eng.final_labels().cpu().numpy().view(np.uint32)


def _no_evol_div(monkeypatch):
    monkeypatch.delenv("LUX_PUSH_EVOL_DIV", raising=False)


# ---- 1 + 2: label correction and the small hand-made cases ----

# (pad_to, LUX_PUSH_EVOL_DIV): at the graphs' own size every iteration is a
# pull (frontier 1 > nv // 16 = 0); padded to 64 vertices with the volume
# threshold at ne every iteration is a push
ROUTES = {"pull": (None, None), "push": (64, "1")}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", sorted(ref.HAND_CASES))
def test_hand_cases(name, route, monkeypatch):
    pad_to, div = ROUTES[route]
    _no_evol_div(monkeypatch)
    if div:
        monkeypatch.setenv("LUX_PUSH_EVOL_DIV", div)
    g, want = ref.hand_graph(name, pad_to=pad_to)
    assert np.array_equal(cpu_ref.sssp_weighted(g, 0), want)
    eng = _engine(g)
    assert eng.visited is None
    iters = eng.run(max_iters=4 * g.nv)
    assert iters <= HAND_NV[name], "no fixed point within nv iterations"
    got = _labels(eng)
    assert np.array_equal(got, want), (got, want)
    assert eng.check() == 0
    assert {r["pull_fallback"] for r in eng.stats} == {route == "pull"}
    if name == "label_correction":
        # vertex 1: 10 after the first iteration, 3 two iterations later
        assert got[1] == 3
        _, sizes, _ = ref.bellman_ford(g, 0)
        assert [r["old_frontier"] for r in eng.stats] == sizes


HAND_NV = {k: v[0] for k, v in ref.HAND_CASES.items()}


def test_label_correction_two_improvements():
    """Step by step on the pull route: vertex 1 holds 10 after iteration 1
    and 3 after iteration 3 — improved in two different iterations."""
    g, want = ref.hand_graph("label_correction")
    eng = _engine(g)
    seen = []
    for _ in range(3):
        eng.step()
        seen.append(int(_labels(eng)[1]))
    assert seen == [10, 10, 3]
    eng.run(max_iters=64)
    assert np.array_equal(_labels(eng), want)


def test_negative_weight_rejected():
    g = ref.graph_from_wedges(4, [(0, 1, 1), (1, 2, -1), (2, 3, 1)])
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    with pytest.raises(ValueError):
        PushEngine(part, PushEngine.MODE_MIN, source=0, weighted=True)
    # the same part still serves the hop engine
    eng = PushEngine(part, PushEngine.MODE_MIN, source=0)
    eng.run(max_iters=16)
    assert np.array_equal(_labels(eng), [0, 1, 2, 3])


def test_check_counts_violations():
    g, want, _, _ = _rmat(*RMATS[0])
    eng = _engine(g)
    eng.run(max_iters=g.nv)
    assert eng.check() == 0
    bad = want.copy()
    v = int(np.nonzero((want != INF) & (want > 0))[0][0])
    bad[v] += 1
    bad[0] = 7
    eng.labels.copy_(torch.from_numpy(bad.view(np.int32)))
    assert eng.check() == cpu_ref.sssp_weighted_check(g, bad, 0) > 0


# ---- 3: device hash weights ----

def test_device_hash_weights():
    scale, ne, seed = 12, 300000, 5
    g = Graph.rmat(scale, ne, seed=seed)
    want = g.hash_weights(16).copy()
    full = DeviceCSC.rmat(scale, ne, seed=seed)
    w = full.hash_weights(16)
    # the weight of an edge depends on its endpoints only, so compare per
    # (dst row, src) pair — the device CSC may order a row's edges its own way
    dst = ref.edge_dst(g)
    dev_src = full.src.cpu().numpy().view(np.uint32)
    dev_w = w.cpu().numpy()[:ne]
    assert np.array_equal(full.col_end.cpu().numpy().view(np.uint64),
                          g.col_end)
    assert np.array_equal(dev_w, ref.hash_weights_np(dev_src, dst, 16, 1))
    key_h = np.lexsort((want, g.src, dst))
    key_d = np.lexsort((dev_w, dev_src, dst))
    assert np.array_equal(g.src[key_h], dev_src[key_d])
    assert np.array_equal(want[key_h], dev_w[key_d])
    # another seed and wmax: not a constant
    w2 = full.hash_weights(1000, seed=9).cpu().numpy()[:ne]
    assert np.array_equal(w2, ref.hash_weights_np(dev_src, dst, 1000, 9))
    # 3-way split: every part hashes its own slice to the same values
    full.weight = None
    parts = [GraphPart(full, 3, p, keep_full=True) for p in range(3)]
    assert sum(p.ep for p in parts) == ne and min(p.ep for p in parts) > 0
    for p in parts:
        pw = p.hash_weights(16).cpu().numpy()[:p.ep]
        assert np.array_equal(pw, dev_w[p.col_left:p.col_right])


def test_host_graph_upload_keeps_hash_weights():
    """from_host keeps the host edge order: weights equal index by index."""
    g, _, _, _ = _rmat(*RMATS[0])
    full = DeviceCSC.from_host(g)
    host_w = full.weight.cpu().numpy().copy()
    dev_w = full.hash_weights(16, seed=3).cpu().numpy()[:g.ne]
    assert np.array_equal(dev_w, host_w)
    assert np.array_equal(dev_w, g.weight)


# ---- 4: RMAT end to end ----

@pytest.mark.parametrize("spec", RMATS)
def test_rmat_end_to_end(spec, monkeypatch):
    _no_evol_div(monkeypatch)
    g, want, sizes, vols = _rmat(*spec)
    eng = _engine(g)
    assert eng.visited is None and eng.push_col is None
    eng.run(max_iters=g.nv)
    assert np.array_equal(_labels(eng), want)
    assert eng.check() == 0
    flags = ref.predict_pull(g.nv, g.ne, sizes, vols)
    assert [r["old_frontier"] for r in eng.stats] == sizes
    assert [r["pull_fallback"] for r in eng.stats] == flags
    assert True in flags and False in flags[1:]  # both kinds occurred
    # iteration 0 overflows the sparse queue and is rebuilt as a bitmap
    assert sizes[1] > eng.capacity
    assert eng.stats[0]["out_dense"] and not eng.stats[0]["pull_fallback"]
    assert eng.stats[0]["my_new"] == sizes[1]


def test_rmat_hub_has_two_chunks():
    g, _, _, _ = _rmat(*RMATS[1])
    assert int((g.src == 0).sum()) == 11056 > 8192


# ---- 5: push ladder ----

HUB_DEGS = [255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193]
PUSH_NV = 16384
TARGET0 = 32


@functools.lru_cache(maxsize=None)
def _push_ladder():
    """0 -> hub i (weight i), hub i's k-th edge -> vertex TARGET0 + k with
    weight 100 + 16 * ((i + k) % 9). For one target the residues (i + k) % 9
    of the hubs reaching it differ, and i < 16, so the sums i + weight are
    pairwise different: the minimum is unique, and which hub wins changes
    from target to target."""
    edges = [(0, i, i) for i in range(1, 10)]
    for i, d in enumerate(HUB_DEGS, start=1):
        k = np.arange(d)
        edges += zip([i] * d, (TARGET0 + k).tolist(),
                     (100 + 16 * ((i + k) % 9)).tolist())
    g = ref.graph_from_wedges(PUSH_NV, edges)
    want = np.full(PUSH_NV, INF, np.uint64)
    want[0] = 0
    want[1:10] = np.arange(1, 10)
    for i, d in enumerate(HUB_DEGS, start=1):
        k = np.arange(d)
        want[TARGET0 + k] = np.minimum(want[TARGET0 + k],
                                       i + 100 + 16 * ((i + k) % 9))
    return g, want.astype(np.uint32)


def test_push_ladder_dense_output(monkeypatch):
    monkeypatch.setenv("LUX_PUSH_EVOL_DIV", "1")
    g, want = _push_ladder()
    assert sum(HUB_DEGS) == 28416 and g.ne == 28416 + 9
    assert np.array_equal(cpu_ref.sssp_weighted(g, 0), want)
    eng = _engine(g)
    assert eng.capacity == 1124 < 28416 // 16
    eng.run(max_iters=16)
    assert np.array_equal(_labels(eng), want)
    assert eng.check() == 0
    row = eng.stats[1]
    assert row["old_frontier"] == 9 and row["pull_fallback"] is False
    # the upfront-dense scatter ran (the sparse one served iteration 0),
    # and 8193 targets do not fit the sparse queue afterwards
    assert eng._graph_uses.get(("push", True)) == 1
    assert eng._graph_uses.get(("push", False)) == 1
    assert row["out_dense"] and row["my_new"] == max(HUB_DEGS)
    assert eng.stats[0] == dict(iter=1, old_frontier=1, pull_fallback=False,
                                out_dense=False, my_new=9)


# ---- 6: pull ladder ----

NEEDED_DEGS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048,
               2049, 8191, 8192, 8193, 8192 + 1025, 16385]


@functools.lru_cache(maxsize=None)
def _pull_ladder(where):
    """dl.plain_ladder with weights in [2, 17] and finite labels >= 1000 on
    every source; each ladder row's marker edge (at `where`) has weight 1
    and its marker vertex label 500 + window, so that edge alone offers the
    row's minimum, 501 + window."""
    assert set(NEEDED_DEGS) <= set(dl.LADDER)
    lad = dl.plain_ladder(marker=where)
    g = lad.g
    rng = np.random.default_rng(21)
    w = rng.integers(2, 18, g.ne).astype(np.int32)
    begin = np.concatenate([[0], g.col_end[:-1].astype(np.int64)])
    rows = lad.ladder_rows[lad.degs[lad.ladder_rows] > 0]
    pos = begin[rows] + [dl.marker_position(int(lad.degs[v]), where)
                         for v in rows]
    assert np.array_equal(g.src[pos], lad.markers[lad.row_block[rows]])
    w[pos] = 1
    g.weight = w
    old = rng.integers(1000, 2000, g.nv).astype(np.uint32)
    old[lad.markers] = 500 + np.arange(len(lad.markers))
    # dst rows: most hold a finite label above every offer (a settled-row
    # skip would keep it), some INF, some already below every offer
    old[rows] = 5000 + rows
    old[rows[rows % 5 == 1]] = INF
    keep = rows[rows % 7 == 3]
    old[keep] = 100 + keep
    src = g.src.astype(np.int64)
    cand = np.minimum(old[src].astype(np.uint64)
                      + w.astype(np.uint64), ref.SAT)
    want = old.astype(np.uint64)
    np.minimum.at(want, lad.dst, cand)
    want = want.astype(np.uint32)
    won = rows[~np.isin(rows, keep)]
    assert np.array_equal(want[won], 501 + lad.row_block[won])
    assert np.array_equal(want[keep], old[keep])
    return lad, old, want


@pytest.mark.parametrize("width", ["u64", "u32"])
@pytest.mark.parametrize("where", ["first", "last", "chunk_last",
                                   "chunk_first"])
def test_pull_ladder(where, width):
    lad, old_np, want = _pull_ladder(where)
    part = GraphPart(DeviceCSC.from_host(lad.g), 1, 0)
    assert part.weight is not None
    if width == "u64":
        part.build_bins()
        assert getattr(part, "blocks", None) is None
        assert part.nbig == (lad.degs >= dl.T2).sum()
    else:
        part.prepare_pull(force_shift=dl.PLAIN_SHIFT, weighted=True)
        assert len(part.blocks) == dl.PLAIN_POOL_BLOCKS
        tot = 0
        for blk in part.blocks:
            assert blk["row_u32"] == 1 and blk["weight"].dtype == torch.int32
            assert blk["weight"].numel() == blk["col"].numel()
            assert blk["n0"] > 0 and blk["n1"] > 0 and blk["nbig"] > 0
            tot += blk["col"].numel()
        assert tot == lad.g.ne
    old = torch.from_numpy(old_np.view(np.int32).copy()).cuda()
    new = torch.empty(part.vp, dtype=torch.int32, device="cuda")
    run_pull(part, ng.PULL_MIN_W, old, new, None, 0.0)
    torch.cuda.synchronize()
    got = new.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"rows {bad[:8]} degrees {lad.degs[bad[:8]]}"


def test_blocked_weights_follow_their_edges():
    """Every (dst row, src, weight) triple of the plain CSC appears in the
    src-blocked one: the scatter moved col and weight to the same slot."""
    lad, _, _ = _pull_ladder("last")
    g = lad.g
    part = GraphPart(DeviceCSC.from_host(g), 1, 0)
    part.prepare_pull(force_shift=dl.PLAIN_SHIFT)  # first without weights
    assert "weight" not in part.blocks[0]
    part.prepare_pull(force_shift=dl.PLAIN_SHIFT, weighted=True)
    trip = []
    for blk in part.blocks:
        rp = blk["row_ptr"].cpu().numpy().view(np.uint32).astype(np.int64)
        rows = np.repeat(np.arange(part.vp), np.diff(rp))
        trip.append(np.stack([rows, blk["col"].cpu().numpy().view(np.uint32),
                              blk["weight"].cpu().numpy()], 1))
    got = np.concatenate(trip)
    have = np.stack([lad.dst, g.src, g.weight], 1)
    order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(order(got), order(have))


# ---- 7: multi-partition, one process ----

def test_weighted_multipart_single_process(monkeypatch):
    """4 partitions in one process with manual segment / annex / label /
    meta cross-copy (the loop of test_sssp_multipart_single_process)."""
    _no_evol_div(monkeypatch)
    scale, ne, seed, P = 11, 60000, 17, 4
    nv = 1 << scale
    g = Graph.rmat(scale, ne, seed=seed)
    g.hash_weights(16, seed=seed)
    want = cpu_ref.sssp_weighted(g, 0)
    full = DeviceCSC.from_host(g)
    parts = [GraphPart(full, P, p, keep_full=True) for p in range(P)]
    engines = [PushEngine(parts[p], PushEngine.MODE_MIN, source=0,
                          weighted=True) for p in range(P)]
    for it in range(4 * nv):
        for e in engines:
            e.step()
        mh = np.stack([e.meta_mine.cpu().numpy().view(np.uint32)
                       for e in engines])
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
    got = engines[0].labels.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)
    kinds = {r["pull_fallback"] for r in engines[0].stats}
    assert kinds == {True, False}
    _, sizes, _ = ref.bellman_ford(g, 0)
    assert [r["old_frontier"] for r in engines[0].stats] == sizes
    assert sum(e.check() for e in engines) == 0


# ---- 8: reset and replay ----

def test_reset_and_replay(monkeypatch):
    _no_evol_div(monkeypatch)
    g, want, sizes, _ = _rmat(*RMATS[0])
    eng = _engine(g)
    for rep in range(3):
        if rep:
            eng.reset()
        eng.run(max_iters=g.nv)
        assert np.array_equal(_labels(eng), want), rep
        assert [r["old_frontier"] for r in eng.stats] == sizes, rep
    # the later traversals replayed captured iteration bodies
    assert eng._graphs, "no iteration body was captured"
    assert eng.check() == 0


# ---- the app driver ----

def test_app_weighted_synthetic(capsys):
    from lux_amd.apps import sssp
    eng = sssp.main(["-synthetic", "rmat:10:8000", "-weighted", "-wmax", "9",
                     "-start", "0", "-check", "-verbose"])
    out = capsys.readouterr().out
    assert "ELAPSED TIME" in out and "[PASS] 0 mistakes" in out
    assert eng.weighted and eng.visited is None
    g = Graph.rmat(10, 8000, seed=1)
    g.hash_weights(9)  # the builders' default seed
    assert np.array_equal(_labels(eng), cpu_ref.sssp_weighted(g, 0))


def test_app_weighted_file(tmp_path, capsys):
    from lux_amd.apps import sssp
    g, want, _, _ = _rmat(*RMATS[0])
    path = str(tmp_path / "w.lux")
    g.save(path)
    eng = sssp.main(["-file", path, "-weighted", "-check"])
    assert "[PASS] 0 mistakes" in capsys.readouterr().out
    assert np.array_equal(_labels(eng), want)
    # without -weighted the same file gives hop distances, as before
    eng = sssp.main(["-file", path])
    assert np.array_equal(_labels(eng), cpu_ref.sssp(g, 0)[0])
    # a file without weights is an error, not a silent hop run
    plain = str(tmp_path / "plain.lux")
    Graph.rmat(10, 8000, seed=3).save(plain)
    with pytest.raises(IOError):
        sssp.main(["-file", plain, "-weighted"])


# ---- 9: unweighted engine untouched ----

def test_unweighted_engine_untouched():
    g, want_w, _, _ = _rmat(*RMATS[0])
    eng = _engine(g, weighted=False)
    assert eng.part.weight is not None
    assert eng.visited is not None and eng.push_col is not None
    eng.run(max_iters=g.nv)
    hops, _ = cpu_ref.sssp(g, 0)
    got = _labels(eng)
    assert np.array_equal(got, hops)
    assert not np.array_equal(got, want_w)
    assert eng.check() == 0
