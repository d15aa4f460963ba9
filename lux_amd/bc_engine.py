"""Single-source betweenness centrality (Brandes dependency accumulation)
on one GPU. No reference equivalent.

Definition — directed graph, source s, hop depths depth[]:
  sigma[s] = 1; for v at depth d > 0, sigma[v] is the sum of sigma[u] over
  the in-edges u->v with depth[u] == d-1;
  for u at depth d, delta[u] is the sum, over the out-edges u->v with
  depth[v] == d+1, of sigma[u]/sigma[v] * (1 + delta[v]).
Conventions: parallel edges count as distinct paths (every occurrence in
the edge list is a term); self-loops never pass the depth test; unreached
vertices have sigma = delta = 0; delta[s] is reported as 0; no halving for
undirected inputs (a symmetric graph is a directed graph with both arcs);
bc after several sources is the sum of their delta arrays; values are fp32
on the device, like PageRank's.

Pipeline per source: hop BFS (PushEngine, exact depths), level order of
the reached rows in both directions (src/gpu/bc.hip: histogram over
depth*3 + degree bin, device scan, scatter — one host read of the offsets
table per direction), the sigma pass over the in-edges of levels 1..L-1,
the delta pass over the out-edges of levels L-2..0 (the PushEngine's push
CSR), one launch per level and pass.
"""
import time

import torch

from . import _native_gpu as ng
from .engine import GraphPart
from .push_engine import PushEngine

U32, U64, F32 = torch.int32, torch.int64, torch.float32
EPS32 = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


class BCEngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "BCEngine is single-rank: the delta pass needs a per-level "
                f"sum across ranks (got a GraphPart with nparts="
                f"{part.nparts})")
        self.part = part
        self.device = part.device
        dev = part.device
        nv, ne = part.nv, part.ne
        # hop BFS for the depths; its push CSR (out-edges of every vertex)
        # is the delta pass's adjacency
        self.push = PushEngine(part, PushEngine.MODE_MIN, source=0)
        self.rec = torch.empty(2 * max(nv, 1), dtype=U32, device=dev)
        self._sigma = torch.zeros(max(nv, 1), dtype=F32, device=dev)
        self._delta = torch.zeros(max(nv, 1), dtype=F32, device=dev)
        self._bc = torch.zeros(max(nv, 1), dtype=F32, device=dev)
        # work-list words: one per row, two per hub chunk; a hub has >= 2048
        # edges and ceil(deg / 8192) <= deg / 8192 + 1 chunks, so the pairs
        # take at most 2 * (ne / 8192 + ne / 2048) < ne / 512 words
        self._cap = nv + ne // 512 + 64
        self._list_in = torch.empty(self._cap, dtype=U32, device=dev)
        self._list_out = torch.empty(self._cap, dtype=U32, device=dev)

        def maxdeg(rp, n):
            return int((rp[1:n + 1] - rp[:n]).max().item()) if n else 0
        self.maxdeg = max(maxdeg(part.row_ptr, part.vp),
                          maxdeg(self.push.push_row_ptr, nv))
        self.levels = 0
        self.source = None
        self.timed = False  # synchronise and clock each phase (the app)
        self.phase_ms = dict(bfs=0.0, order=0.0, sigma=0.0, delta=0.0)
        self._off = None
        self._stats = None

    # -------- phases --------
    def _tick(self):
        if not self.timed:
            return 0.0
        torch.cuda.synchronize()
        return time.perf_counter()

    def _tock(self, name, t0):
        if self.timed:
            torch.cuda.synchronize()
            self.phase_ms[name] += 1000.0 * (time.perf_counter() - t0)

    def _order(self, depth, row_ptr, lst):
        """Level order of one direction. Returns the host copy of the
        table: 3L+1 word offsets (key = depth*3 + bin), then L hub-row
        counts. The .cpu() below is the direction's one host read."""
        s = _stream()
        L, nv = self.levels, self.part.nv
        cnt = torch.zeros(3 * L, dtype=U32, device=self.device)
        tab = torch.zeros(4 * L + 1, dtype=U64, device=self.device)
        ng.bc_order_hist(s, nv, depth, row_ptr, L, cnt,
                         tab.narrow(0, 3 * L + 1, L))
        partials = torch.empty(ng.scan_partials_size(3 * L), dtype=U64,
                               device=self.device)
        ng.scan_end_offsets(s, 3 * L, cnt, tab.narrow(0, 1, 3 * L), partials)
        cursor = tab.narrow(0, 0, 3 * L).clone()
        host = tab.cpu().numpy()
        assert int(host[3 * L]) <= self._cap, "bc work list over capacity"
        ng.bc_order_scatter(s, nv, depth, row_ptr, L, cursor, lst)
        return host

    def run(self, source):
        """BFS + level order + sigma pass + delta pass from `source`;
        returns delta (device f32[nv])."""
        p = self.part
        s = _stream()
        source = int(source)
        if not 0 <= source < p.nv:
            raise ValueError(f"source {source} outside [0, {p.nv})")
        self.source = source
        t0 = self._tick()
        if source != self.push.source:
            # PushEngine caches the seed frontier of its first source;
            # drop it so reset() rebuilds the segment for this one
            self.push._fq_init = None
        self.push.reset(source)
        # a level-synchronous hop traversal finds depth k in iteration k and
        # nothing in its last one: iterations == deepest level + 1
        self.levels = L = self.push.run()
        depth = self.push.final_labels()
        self._tock("bfs", t0)

        t0 = self._tick()
        ng.bc_init(s, p.nv, source, depth, self.rec, self._sigma,
                   self._delta)
        off_in = self._order(depth, p.row_ptr, self._list_in)
        off_out = self._order(depth, self.push.push_row_ptr, self._list_out)
        self._tock("order", t0)

        edges = torch.zeros(2 * L, dtype=U64, device=self.device)
        eaddr = edges.data_ptr()
        t0 = self._tick()
        for d in range(1, L):
            o = [int(x) for x in off_in[3 * d:3 * d + 4]]
            ng.bc_level(s, True, self._list_in, o[0], o[1], o[2], o[3],
                        p.row_ptr, p.col, self.rec, self._sigma, self._delta,
                        d, d == L - 1, eaddr + 8 * d)
        self._tock("sigma", t0)
        t0 = self._tick()
        for d in range(L - 2, -1, -1):
            o = [int(x) for x in off_out[3 * d:3 * d + 4]]
            ng.bc_level(s, False, self._list_out, o[0], o[1], o[2], o[3],
                        self.push.push_row_ptr, self.push.push_col, self.rec,
                        self._sigma, self._delta, d, False,
                        eaddr + 8 * (L + d))
        self._tock("delta", t0)
        self._off = (off_in, off_out, edges)
        self._stats = None
        return self._delta

    def run_sources(self, sources):
        """bc() = sum of delta over `sources` (restarts the sum)."""
        self._bc.zero_()
        for src in sources:
            self._bc += self.run(src)
        return self._bc

    # -------- results --------
    def depth(self):
        return self.push.final_labels()

    def sigma(self):
        return self._sigma

    def delta(self):
        return self._delta

    def bc(self):
        return self._bc

    @property
    def stats(self):
        """One row per level of the last run. rows_*: rows the level lists
        for the pass (from the offsets tables); edges_*: edges that passed
        the depth test, i.e. the level's BFS-DAG edges (counted by the
        pass). The sigma pass skips level 0, the delta pass level L-1."""
        if self._stats is None and self._off is not None:
            off_in, off_out, edges = self._off
            L = self.levels
            e = edges.cpu().numpy()

            def rows(off, d):
                return int(off[3 * d + 2] - off[3 * d] + off[3 * L + 1 + d])
            self._stats = [dict(level=d, rows_in=rows(off_in, d),
                                edges_in=int(e[d]),
                                rows_out=rows(off_out, d),
                                edges_out=int(e[L + d])) for d in range(L)]
        return self._stats or []

    def rtol(self):
        """Relative error bound of sigma/delta: a sum of m non-negative
        fp32 terms is off by at most (m-1)u, each term adds 3u of its own,
        compounding over at most L levels."""
        return 1.01 * max(self.levels, 1) * (self.maxdeg + 3) * EPS32

    def check(self):
        """Device check oracle: rows whose sigma or delta, recomputed from
        the final arrays, misses the stored value by more than rtol(), plus
        reached rows with a non-finite sigma."""
        p = self.part
        out = torch.zeros(2, dtype=U64, device=self.device)
        ng.bc_check(_stream(), p.nv, self.source, p.row_ptr, p.col,
                    self.push.push_row_ptr, self.push.push_col,
                    self.push.final_labels(), self._sigma, self._delta,
                    self.rtol(), out)
        return int(out.sum().item())
