"""k-truss decomposition on one GPU: per-edge triangle support and
decremental synchronous peeling with device-side queues (src/gpu/truss.hip).
No reference equivalent.

Definition — the same graph as TCEngine, KCoreEngine and MSFEngine: the
underlying simple undirected graph of whatever the project loads. Edges are
listed in (lo << 32) | hi order, the edge id is the index in that list.
  support(e)   = the number of triangles through e;
  the k-truss  = the largest subgraph whose every edge has support >= k - 2
                 inside it;
  trussness(e) = the largest k whose k-truss holds e, 2 for an edge in no
                 triangle; exact integers in the caller's vertex ids.

Preparation (phase_ms["orient"] and ["adjacency"]): tc_engine.orient(...,
"id") gives the DAG lo -> hi whose arc e is edge e. The 2m directed keys
(a << 32) | b of both directions of every arc, sorted, are the full
adjacency with every row strictly ascending: they are sorted in runs of at
most LUX_TC_SORT_CHUNK keys and merged by row ranges (_sorted_directed_keys,
the sibling of tc_engine._sorted_unique_keys), and truss_adj_fill_kernel
turns each range into aadj, aeid (the edge id of every entry) and elo.

Host-side rules (what a run at RMAT-24 taught an earlier engine, BENCHLOG
r11.1): every tensor that scales with m is one-dimensional, and goes only
through sort, cumsum, bincount, searchsorted, slices, cat of slices and
element-wise ops, in chunks of at most the sort chunk. No boolean-mask
selection, index_put, nonzero or repeat_interleave over an m-sized tensor
happens anywhere in this module — not in the preparation, not in the solve,
not in the result methods; truss(k) and its kin are element-wise
comparisons. All per-edge bookkeeping lives in the kernels (an append-only
queue, returning atomics, one small meta read per launch); the host keeps a
handful of cursors.

support() classifies the edges into the three roles of truss.hip (twice:
once to count, which sizes the hub queue, once to list) and runs the
SUPPORT mode on the lists. decompose() peels level by level, s always
jumping to the minimum alive support: a level is one scan (speculative at
the previous s + 1; if nobody is there, a second one at the minimum it
returned) and then rounds, one PEEL launch each, or one single-workgroup
tail launch for a run of small rounds. The loop is bounded (rounds <= m +
levels, cursors <= m) and raises instead of spinning.

Env knobs: LUX_TRUSS_HUB (an edge whose shorter row is longer than this is
intersected by workgroups, in chunks of this many entries), LUX_TRUSS_FUSE
(largest round the tail kernel takes, 0 = off), LUX_TRUSS_FENCE (entries of
the hub role's LDS table), LUX_TC_SORT_CHUNK (keys per sort).
"""
import os
import time

import torch

from .engine import GraphPart
from .tc_engine import SORT_CHUNK_DEFAULT, orient

U32, U64 = torch.int32, torch.int64
MASK32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF
HUB_MAX = 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sorted_directed_keys(dag, ends, nv, chunk):
    """Yields (base, keys): consecutive ranges of the sorted i64 keys
    (a << 32) | b over both directions of every DAG arc, `base` the index of
    the range's first key among all 2m. `ends` is the cumsum of the full
    degrees. Every torch.sort sees at most `chunk` keys, apart from a single
    row longer than that."""
    dev = dag.optr.device
    runs = []
    step = max(chunk // 2, 1)  # arcs per pair of runs
    for i0 in range(0, dag.m, step):
        i1 = min(i0 + step, dag.m)
        e = torch.arange(i0, i1, dtype=U64, device=dev)
        lo = torch.searchsorted(dag.optr, e, right=True) - 1
        hi = dag.oadj[i0:i1].to(U64) & MASK32
        runs.append((lo << 32) | hi)  # the DAG is in key order already
        runs.append(torch.sort((hi << 32) | lo).values)
    if len(runs) <= 2:
        if runs:
            yield 0, torch.sort(torch.cat(runs)).values
        return
    # the runs are sorted over the whole key space: cut it at row boundaries
    # so that a range gathers at most `chunk` keys from all runs
    r0, base = 0, 0
    while r0 < nv:
        r1 = int(torch.searchsorted(
            ends, torch.tensor([base + chunk], dtype=U64, device=dev),
            right=True).item())
        r1 = min(max(r1, r0 + 1), nv)
        cut = torch.tensor([r0 << 32, r1 << 32], dtype=U64, device=dev)
        part = []
        for k in runs:
            i0, i1 = torch.searchsorted(k, cut).tolist()
            if i1 > i0:
                part.append(k[i0:i1])
        if part:
            yield base, torch.sort(torch.cat(part)).values
        base = int(ends[r1 - 1].item())
        r0 = r1


class TrussEngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "TrussEngine is single-rank: an intersection needs both "
                f"rows on one device (got a GraphPart with "
                f"nparts={part.nparts})")
        from . import _native_gpu as ng
        knobs = {}
        for name, lo, hi in (("hub", 1, HUB_MAX),
                             ("fuse", 0, ng.truss_const("fuse_max")),
                             ("fence", 2, ng.truss_const("fence_max"))):
            env = f"LUX_TRUSS_{name.upper()}"
            knobs[name] = int(os.environ.get(
                env, ng.truss_const(f"{name}_default")))
            if not lo <= knobs[name] <= hi:
                raise ValueError(f"{env}={knobs[name]} outside [{lo}, {hi}]")
        self.hub, self.fuse, self.fence = (knobs[k] for k in
                                           ("hub", "fuse", "fence"))
        chunk = max(int(os.environ.get("LUX_TC_SORT_CHUNK",
                                       SORT_CHUNK_DEFAULT)), 1)
        self.part = part
        self.device = dev = part.device
        self.timed = False  # synchronise and clock the phases (the app)
        self.phase_ms = dict(orient=0.0, adjacency=0.0, support=0.0,
                             peel=0.0)
        nv = part.nv

        t0 = self._now()
        dag = orient(part.row_ptr, part.col, nv, "id", chunk)
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)
        if dag.m >= 1 << 32:
            raise ValueError(f"TrussEngine: {dag.m} simple edges; edge ids "
                             "are 32-bit (m < 2^32)")

        t0 = self._now()
        self.m = m = dag.m
        indeg = torch.zeros(max(nv, 1), dtype=U32, device=dev)
        if m:
            ng.hist_u32(_stream(), m, dag.oadj, indeg)
        degree = (dag.optr[1:] - dag.optr[:-1]) + indeg[:nv]
        self.max_degree = int(degree.max().item()) if nv else 0
        self.aptr = torch.zeros(nv + 1, dtype=U64, device=dev)
        self.aptr[1:] = torch.cumsum(degree, 0)
        self.aadj = torch.empty(max(2 * m, 1), dtype=U32, device=dev)
        self.aeid = torch.empty(max(2 * m, 1), dtype=U32, device=dev)
        self.elo = torch.zeros(max(m, 1), dtype=U32, device=dev)
        self.ehi = dag.oadj if m else torch.empty(1, dtype=U32, device=dev)
        for base, keys in _sorted_directed_keys(dag, self.aptr[1:], nv,
                                                chunk):
            ng.truss_adj_fill(_stream(), nv, m, dag.optr, dag.oadj, keys,
                              base, self.aadj, self.aeid, self.elo)
            del keys
        del dag, indeg, degree
        self.phase_ms["adjacency"] = 1000.0 * (self._now() - t0)

        n = max(m, 1)
        self._sup0 = None  # the support of the whole graph, i32[m]
        self._sup = torch.empty(n, dtype=U32, device=dev)
        self._order = torch.empty(n, dtype=U32, device=dev)
        self._pos = torch.empty(n, dtype=U32, device=dev)
        self._truss = torch.empty(n, dtype=U32, device=dev)
        self._meta = torch.zeros(ng.truss_const("meta_words"), dtype=U32,
                                 device=dev)
        self._bad = torch.zeros(1, dtype=U64, device=dev)
        self._roles = None  # (list u32[m], hubq, nlane, nwave, nhub)
        self._hubq = None
        self._done = False
        self._role_stats = dict(items_lane=0, items_wave=0, items_hub=0)
        self._stats = dict(levels=0, rounds=0, fused_rounds=0, scans=0,
                           launches=0, host_reads=0, hub_items=0)
        self.level_trace = []  # (k, rounds, removed) per level

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    def _read_meta(self):
        """The blocking read of the meta record (u32 values)."""
        self._stats["host_reads"] += 1
        return [x & NONE for x in self._meta.tolist()]

    def _args(self, order, hubq, hubcap, **more):
        from . import _native_gpu as ng
        return ng.truss_args(self.m, hubcap, self.hub, self.fence,
                             aptr=self.aptr, aadj=self.aadj, aeid=self.aeid,
                             elo=self.elo, ehi=self.ehi, order=order,
                             hubq=hubq, meta=self._meta, **more)

    # -------- roles and support --------
    def _classify(self):
        """The role lists of all m edges, built once: lane edges at the
        front of one u32[m] list, wave edges at its back, hub items
        {edge, chunk} in their own queue, which the counting pass sizes."""
        from . import _native_gpu as ng
        if self._roles is None:
            lst = torch.empty(max(self.m, 1), dtype=U32, device=self.device)
            hubq = torch.empty(2, dtype=U32, device=self.device)
            self._meta.zero_()
            ng.truss_classify(_stream(), self._args(lst, hubq, 0), 0)
            c = self._read_meta()
            nhub = c[ng.TRUSS_M_HUBTAIL]
            hubq = torch.empty(2 * max(nhub, 1), dtype=U32,
                               device=self.device)
            self._meta.zero_()
            ng.truss_classify(_stream(), self._args(lst, hubq, nhub), 1)
            self._roles = (lst, hubq, c[ng.TRUSS_M_LANE],
                           c[ng.TRUSS_M_WAVE], nhub)
            self._role_stats = dict(items_lane=c[ng.TRUSS_M_LANE],
                                    items_wave=c[ng.TRUSS_M_WAVE],
                                    items_hub=nhub)
        return self._roles

    def _run_lists(self, mode, **state):
        """One mode over every edge: the lane list with the hub items, then
        the wave list."""
        from . import _native_gpu as ng
        lst, hubq, nlane, nwave, nhub = self._classify()
        a = self._args(lst, hubq, nhub, **state)
        ng.truss_round(_stream(), a, mode, 0, nlane, 0, nhub)
        ng.truss_round(_stream(), a, mode, self.m - nwave, self.m, 0, 0)

    def support(self):
        """Device i32[m]: the triangles through every edge of the whole
        graph, in key order. Counted once and kept."""
        from . import _native_gpu as ng
        if self._sup0 is None:
            t0 = self._now() if self.timed else 0.0
            sup0 = torch.zeros(max(self.m, 1), dtype=U32, device=self.device)
            if self.m:
                self._run_lists(ng.TRUSS_SUPPORT, sup=sup0)
            self._sup0 = sup0
            if self.timed:
                self.phase_ms["support"] = 1000.0 * (self._now() - t0)
        return self._sup0[:self.m]

    # -------- peeling --------
    def decompose(self):
        """Peel the whole graph from its support; returns the device
        trussness, int32[m] in key order."""
        from . import _native_gpu as ng
        m = self.m
        self.support()
        hubcap = self._classify()[4]
        if self._hubq is None:
            self._hubq = torch.empty(2 * max(hubcap, 1), dtype=U32,
                                     device=self.device)
        st = self._stats = dict(levels=0, rounds=0, fused_rounds=0, scans=0,
                                launches=0, host_reads=0, hub_items=0)
        self.level_trace = []
        t0 = self._now() if self.timed else 0.0
        self._sup.copy_(self._sup0)
        self._pos.fill_(-1)
        self._truss.fill_(2)
        self._meta.zero_()
        stream = _stream()
        a = self._args(self._order, self._hubq, hubcap, sup=self._sup,
                       pos=self._pos, truss=self._truss)

        def scan(s):
            ng.truss_scan(stream, a, s)
            st["scans"] += 1
            st["launches"] += 1
            return self._read_meta()

        def bounded(head, tail, hubtail):
            if not head <= tail <= m or hubtail > hubcap or \
                    st["rounds"] > m + st["levels"]:
                raise RuntimeError(
                    f"k-truss peel out of bounds: head={head} tail={tail} "
                    f"m={m} hubtail={hubtail} hubcap={hubcap} "
                    f"rounds={st['rounds']} levels={st['levels']}")

        head = tail = hubhead = hubtail = 0
        s = 0  # the first scan is speculative too: edges in no triangle
        while tail < m:
            r = scan(s)
            if r[ng.TRUSS_M_TAIL] == tail:  # nobody there: jump
                mn = r[ng.TRUSS_M_MIN]
                if mn == NONE or mn <= s:
                    raise RuntimeError(
                        f"k-truss scan at s={s}: {m - tail} edges alive but "
                        f"minimum support {mn}")
                s = mn
                r = scan(s)
                if r[ng.TRUSS_M_TAIL] == tail:
                    raise RuntimeError(f"k-truss scan at s={s} found nobody")
            st["levels"] += 1
            first, rounds0 = tail, st["rounds"]
            tail, hubtail = r[ng.TRUSS_M_TAIL], r[ng.TRUSS_M_HUBTAIL]
            bounded(head, tail, hubtail)
            while head < tail:
                st["launches"] += 1
                if self.fuse and tail - head <= self.fuse and \
                        hubtail == hubhead:
                    ng.truss_tail(stream, a, s, head, tail, hubtail,
                                  self.fuse)
                    r = self._read_meta()
                    st["rounds"] += r[ng.TRUSS_M_FUSED]
                    st["fused_rounds"] += r[ng.TRUSS_M_FUSED]
                    head = r[ng.TRUSS_M_HEAD]
                else:
                    ng.truss_round(stream, a, ng.TRUSS_PEEL, head, tail,
                                   hubhead, hubtail, s)
                    r = self._read_meta()
                    st["rounds"] += 1
                    head, hubhead = tail, hubtail
                tail, hubtail = r[ng.TRUSS_M_TAIL], r[ng.TRUSS_M_HUBTAIL]
                bounded(head, tail, hubtail)
            self.level_trace.append((s + 2, st["rounds"] - rounds0,
                                     tail - first))
            s += 1
        st["hub_items"] = hubtail
        if self.timed:
            self.phase_ms["peel"] = 1000.0 * (self._now() - t0)
        self._done = True
        return self._truss[:m]

    def trussness(self):
        """Device int32[m]: the stored array of the last decompose();
        decomposed now if there is none."""
        if not self._done:
            self.decompose()
        return self._truss[:self.m]

    def edges(self):
        """Device (lo, hi), i64[m] each, in key order."""
        m = self.m
        return (self.elo[:m].to(U64) & MASK32, self.ehi[:m].to(U64) & MASK32)

    def kmax(self):
        return int(self.trussness().max().item()) if self.m else 2

    def truss(self, k):
        """Device bool[m]: the edges of the k-truss."""
        return self.trussness() >= k

    def truss_sizes(self):
        """Device i64[kmax + 1]: the edges of each trussness."""
        return torch.bincount(self.trussness().to(U64))

    def truss_vertices(self, k):
        """The number of vertices the k-truss touches (weighted bincounts of
        the endpoints, a sort chunk at a time)."""
        nv = self.part.nv
        alive = self.truss(k)
        chunk = max(int(os.environ.get("LUX_TC_SORT_CHUNK",
                                       SORT_CHUNK_DEFAULT)), 1)
        cnt = torch.zeros(max(nv, 1), dtype=torch.float64, device=self.device)
        for end in self.edges():
            for i0 in range(0, self.m, chunk):
                cnt += torch.bincount(
                    end[i0:i0 + chunk],
                    weights=alive[i0:i0 + chunk].to(torch.float64),
                    minlength=max(nv, 1))
        return int((cnt > 0).sum().item())

    @property
    def stats(self):
        return dict(simple_edges=self.m, max_degree=self.max_degree,
                    **self._stats, **self._role_stats)

    def check(self, trussness=None):
        """Device check oracle (the CHECK mode of truss.hip) of the stored
        trussness, or of the int32[m] array given: the edges e that break a
        necessary condition — with t = trussness[e], fewer than t - 2
        triangles whose other two edges have trussness >= t, t - 1 or more
        whose other two have >= t + 1, or t outside [2, support + 2].
        Necessary, not sufficient: exactness rests on the tests against the
        CPU oracle."""
        from . import _native_gpu as ng
        t = self.trussness() if trussness is None else trussness
        if t.numel() != self.m or t.dtype != U32 or not t.is_contiguous():
            raise ValueError("check: trussness must be contiguous int32[m]")
        if not self.m:
            return 0
        self.support()
        self._bad.zero_()
        self._run_lists(ng.TRUSS_CHECK, truss=t, sup0=self._sup0,
                        bad=self._bad)
        return int(self._bad.item())
