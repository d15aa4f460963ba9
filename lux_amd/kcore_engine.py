"""k-core decomposition on one GPU: synchronous peeling with device-side
queues (src/gpu/kcore.hip). No reference equivalent.

Definition — the same graph as TCEngine: the underlying simple undirected
graph of whatever the project loads ({u,v} is an edge iff u != v and u->v or
v->u occurs; parallel edges collapse, self-loops vanish).
  the k-core    = the largest subgraph in which every vertex has degree >= k;
  coreness[v]   = the largest k whose k-core contains v, 0 for a vertex with
                  no simple edge; an exact integer in the caller's vertex ids;
  degeneracy    = coreness.max().

Preparation (timed as phase_ms["orient"] and phase_ms["adjacency"]):
tc_engine.orient(..., "id") gives the simple graph as the DAG lo -> hi in
the caller's ids (rank == id: no permutation to undo); the full degree is
the DAG's out-degree plus its in-degree (a histogram of oadj), aptr its
cumsum, and kcore_adj_fill_kernel writes both directions of every arc into
aadj.

decompose() peels level by level, k always jumping to the minimum alive
degree. A level is one scan (append every vertex of degree k; if the
speculative scan at the previous k + 1 finds none, a second one at the
minimum it returned) and then rounds: a round removes the queued vertices
and queues every neighbour whose degree falls to k. Queues, degrees and all
per-round bookkeeping live in the kernels; the host keeps four cursors,
launches one kernel per round and reads the 8-word meta record back once per
launch. Small rounds of a level (at most LUX_KCORE_FUSE entries, no hub row)
are peeled by a single-workgroup kernel that loops over them, so a cascade
costs one launch. The schedule is tests/kcore_ref.sync_peel's, level for
level and round for round. Every host tensor is one-dimensional, and none
that scales with m is written through a mask or an index.

Env knobs: LUX_KCORE_HUB (rows longer than this are peeled by workgroups,
in chunks of this many entries; default the kernels' KCORE_HUB),
LUX_KCORE_FUSE (largest round the single-workgroup kernel takes, 0 = off;
default the kernels' KCORE_FUSE).
"""
import os
import time

import torch

from .engine import GraphPart
from .tc_engine import orient

U32, U64 = torch.int32, torch.int64
NONE = 0xFFFFFFFF
HUB_MAX = 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KCoreEngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "KCoreEngine is single-rank: a peel round decrements "
                "neighbours on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_KCORE_HUB", ng.kcore_hub_default()))
        if not 1 <= hub <= HUB_MAX:
            raise ValueError(f"LUX_KCORE_HUB={hub} outside [1, {HUB_MAX}]")
        fuse = int(os.environ.get("LUX_KCORE_FUSE", ng.kcore_fuse_default()))
        if not 0 <= fuse <= ng.kcore_fuse_max():
            raise ValueError(f"LUX_KCORE_FUSE={fuse} outside "
                             f"[0, {ng.kcore_fuse_max()}]")
        self.part = part
        self.device = part.device
        self.hub, self.fuse = hub, fuse
        self.timed = False  # synchronise and clock decompose() (the app)
        self.phase_ms = dict(orient=0.0, adjacency=0.0, peel=0.0)
        nv = part.nv
        dev = self.device

        t0 = self._now()
        dag = orient(part.row_ptr, part.col, nv, "id")
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)

        t0 = self._now()
        self.m = dag.m
        indeg = torch.zeros(max(nv, 1), dtype=U32, device=dev)
        if dag.m:
            ng.hist_u32(_stream(), dag.m, dag.oadj, indeg)
        self.degree = (dag.optr[1:] - dag.optr[:-1]).to(U32) + indeg[:nv]
        self.aptr = torch.zeros(nv + 1, dtype=U64, device=dev)
        self.aptr[1:] = torch.cumsum(self.degree, 0, dtype=U64)
        self.aadj = torch.empty(max(2 * dag.m, 1), dtype=U32, device=dev)
        indeg.zero_()  # now the per-row cursor
        ng.kcore_adj_fill(_stream(), nv, dag.m, dag.optr, dag.oadj,
                          self.aptr, indeg, self.aadj)
        self.max_degree = int(self.degree.max().item()) if nv else 0
        big = self.degree[self.degree > hub].to(U64)
        self.hubcap = int(((big + (hub - 1)) // hub).sum().item())
        del dag, indeg, big
        self.phase_ms["adjacency"] = 1000.0 * (self._now() - t0)

        self._deg = torch.empty(max(nv, 1), dtype=U32, device=dev)
        self._order = torch.empty(max(nv, 1), dtype=U32, device=dev)
        self._hubq = torch.empty(2 * max(self.hubcap, 1), dtype=U32,
                                 device=dev)
        self._meta = torch.zeros(ng.kcore_meta_words(), dtype=U32,
                                 device=dev)
        self._bad = torch.zeros(1, dtype=U64, device=dev)
        self._done = False
        self._stats = dict(levels=0, rounds=0, fused_rounds=0, scans=0,
                           host_reads=0)
        self.level_trace = []  # (k, rounds, removed) per level

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    # -------- peeling --------
    def _read_meta(self):
        """The blocking read of the meta record (u32 values)."""
        self._stats["host_reads"] += 1
        return [x & NONE for x in self._meta.tolist()]

    def decompose(self):
        """Peel the whole graph; returns the device coreness, i32[nv]."""
        from . import _native_gpu as ng
        nv = self.part.nv
        st = self._stats = dict(levels=0, rounds=0, fused_rounds=0, scans=0,
                                host_reads=0)
        self.level_trace = []
        t0 = self._now() if self.timed else 0.0
        self._deg[:nv] = self.degree
        self._meta.zero_()
        s = _stream()
        common = (self._deg, self._order, self._hubq, self.hubcap,
                  self._meta, self.hub)

        def scan(k):
            ng.kcore_scan(s, nv, self.aptr, *common, k)
            st["scans"] += 1
            return self._read_meta()

        def bounded(head, tail, hubtail):
            if not head <= tail <= nv or hubtail > self.hubcap or \
                    st["rounds"] > nv + st["levels"]:
                raise RuntimeError(
                    f"k-core peel out of bounds: head={head} tail={tail} "
                    f"nv={nv} hubtail={hubtail} hubcap={self.hubcap} "
                    f"rounds={st['rounds']} levels={st['levels']}")

        head = tail = hubhead = hubtail = 0
        k = 0  # the first scan is speculative too: isolated vertices
        while tail < nv:
            m = scan(k)
            if m[0] == tail:  # nobody has degree k: jump to the minimum
                if m[2] == NONE or m[2] <= k:
                    raise RuntimeError(
                        f"k-core scan at k={k}: {nv - tail} vertices alive "
                        f"but minimum degree {m[2]}")
                k = m[2]
                m = scan(k)
                if m[0] == tail:
                    raise RuntimeError(f"k-core scan at k={k} found nobody")
            st["levels"] += 1
            first, rounds0 = tail, st["rounds"]
            tail, hubtail = m[0], m[1]
            bounded(head, tail, hubtail)
            while head < tail:
                if self.fuse and tail - head <= self.fuse and \
                        hubtail == hubhead:
                    ng.kcore_tail(s, nv, self.aptr, self.aadj, *common, k,
                                  head, tail, hubtail, self.fuse)
                    m = self._read_meta()
                    st["rounds"] += m[3]
                    st["fused_rounds"] += m[3]
                    head = m[4]
                else:
                    ng.kcore_peel(s, nv, self.aptr, self.aadj, *common, k,
                                  head, tail, hubhead, hubtail)
                    m = self._read_meta()
                    st["rounds"] += 1
                    head, hubhead = tail, hubtail
                tail, hubtail = m[0], m[1]
                bounded(head, tail, hubtail)
            self.level_trace.append((k, st["rounds"] - rounds0,
                                     tail - first))
            k += 1
        if self.timed:
            self.phase_ms["peel"] = 1000.0 * (self._now() - t0)
        self._done = True
        return self._deg[:nv]

    def coreness(self):
        """Device i32[nv]: the coreness per vertex, original ids. The stored
        array of the last decompose(); decomposed now if there is none."""
        if not self._done:
            self.decompose()
        return self._deg[:self.part.nv]

    def degeneracy(self):
        return int(self.coreness().max().item()) if self.part.nv else 0

    def shell_sizes(self):
        """Device i64[degeneracy + 1]: the vertices of each coreness."""
        return torch.bincount(self.coreness().to(U64))

    def core(self, k):
        """Device bool[nv]: the vertices of the k-core."""
        return self.coreness() >= k

    def order(self):
        """Device u32 (torch.int32 bits)[nv]: the removal order, a
        degeneracy ordering; the order inside a round is not deterministic."""
        self.coreness()
        return self._order[:self.part.nv]

    @property
    def stats(self):
        return dict(simple_edges=self.m, max_degree=self.max_degree,
                    **self._stats)

    def check(self):
        """Device check oracle (kcore_check_kernel): the vertices v that
        break a necessary condition — fewer than coreness[v] neighbours of
        coreness >= coreness[v], coreness[v] + 1 or more of coreness >=
        coreness[v] + 1, or a coreness outside [0, degree]. Necessary, not
        sufficient (the all-zero array passes): exactness rests on the
        tests against the CPU oracle."""
        from . import _native_gpu as ng
        core = self.coreness()
        self._bad.zero_()
        ng.kcore_check(_stream(), self.part.nv, self.aptr, self.aadj, core,
                       self._bad)
        return int(self._bad.item())
