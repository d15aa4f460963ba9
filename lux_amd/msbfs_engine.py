"""Multi-source BFS on one GPU, 64 sources per machine word
(src/gpu/msbfs.hip): hop distances from many vertices at once, and what is
summed from them — closeness, harmonic centrality, eccentricities. No
reference equivalent; the definition is in API.md.

The directed graph exactly as loaded: an edge u -> v is followed from u to
v. Sources run in batches of 64, the last one shorter. A batch is seeded
(level 0) and then expanded level by level; a level is one traversal launch
and the epilogue launch, after which the host reads the meta record once.
Entry L of a batch's level_trace describes the frontier at depth L — its
vertices, their out-edge volume, the (source, vertex) pairs found at depth
L — and the direction in which level L expanded it:
    pull iff volume * LUX_MSBFS_PULL_DIV > ne,
unless LUX_MSBFS_DIR forces one. The record of depth 0 needs no launch: the
out-degrees of all sources are fetched once per run(). The batch ends with
the level that finds nothing. Push, pull and auto give identical bits.

Preparation (phase_ms["csr"], ["plan"]): the out-edge CSR as SCCEngine
builds it, and the static role lists of the pull direction by in-degree —
[1, thread limit] one lane per row, up to LUX_MSBFS_HUB one wave per row,
longer rows as {vertex, chunk} items of LUX_MSBFS_HUB entries. The push
direction takes the same roles by out-degree from the queues the epilogue
writes.

Env knobs: LUX_MSBFS_HUB (default the kernels' MSBFS_HUB),
LUX_MSBFS_PULL_DIV (default MSBFS_PULL_DIV), LUX_MSBFS_DIR (auto | push |
pull).
"""
import os
import time

import numpy as np
import torch

from .engine import GraphPart

U32, U64 = torch.int32, torch.int64
DIRS = ("auto", "push", "pull")
DIV_MAX = 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _items(deg, hub):
    """The {vertex, chunk} pairs, flat u32, of the rows longer than hub, and
    the number of such rows."""
    hv = torch.nonzero(deg > hub, as_tuple=True)[0]
    nc = (deg[hv] + (hub - 1)) // hub
    v = torch.repeat_interleave(hv, nc)
    first = torch.repeat_interleave(torch.cumsum(nc, 0) - nc, nc)
    c = torch.arange(v.numel(), device=deg.device) - first
    out = torch.zeros(2 * max(v.numel(), 1), dtype=U32, device=deg.device)
    if v.numel():
        out[0::2] = v.to(U32)
        out[1::2] = c.to(U32)
    return out, int(v.numel()), int(hv.numel())


class MSBFSEngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "MSBFSEngine is single-rank: a level reads the words of "
                "every neighbour on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_MSBFS_HUB", ng.msbfs_hub_default()))
        if not 1 <= hub <= ng.msbfs_hub_max():
            raise ValueError(f"LUX_MSBFS_HUB={hub} outside "
                             f"[1, {ng.msbfs_hub_max()}]")
        div = int(os.environ.get("LUX_MSBFS_PULL_DIV",
                                 ng.msbfs_pull_div_default()))
        if not 1 <= div <= DIV_MAX:
            raise ValueError(f"LUX_MSBFS_PULL_DIV={div} outside "
                             f"[1, {DIV_MAX}]")
        direction = os.environ.get("LUX_MSBFS_DIR", "auto")
        if direction not in DIRS:
            raise ValueError(f"LUX_MSBFS_DIR={direction!r} is not one of "
                             f"{', '.join(DIRS)}")
        self.part = part
        self.device = dev = part.device
        self.hub, self.div, self.direction = hub, div, direction
        self.thr = min(hub, ng.msbfs_thread_limit())
        self.timed = False  # synchronise and clock run() (the app)
        self.phase_ms = dict(csr=0.0, plan=0.0, run=0.0)
        nv, ne = part.nv, part.ep
        if nv < 1:
            raise ValueError("MSBFSEngine needs at least one vertex")
        self.ne = ne
        s = _stream()

        # ---- out-edge CSR: all sources -> their targets ----
        t0 = self._now()
        out_deg = torch.zeros(nv, dtype=U32, device=dev)
        if ne:
            ng.hist_u32(s, ne, part.col, out_deg)
        ends = torch.empty(nv, dtype=U64, device=dev)
        partials = torch.empty(max(ng.scan_partials_size(nv), 1), dtype=U64,
                               device=dev)
        ng.scan_end_offsets(s, nv, out_deg, ends, partials)
        self.out_ptr = torch.zeros(nv + 1, dtype=U64, device=dev)
        ng.local_row_ptr(s, nv, 0, ends, self.out_ptr)
        self.out_col = torch.empty(max(ne, 1), dtype=U32, device=dev)
        if ne:
            cursor = self.out_ptr[:nv].clone()
            ng.csr_scatter(s, ne, part.col, part.row_ptr, part.vp,
                           part.row_left, cursor, self.out_col)
            del cursor
        del ends, partials, out_deg
        self.phase_ms["csr"] = 1000.0 * (self._now() - t0)

        # ---- static role lists of the pull direction, hub capacities ----
        t0 = self._now()
        in_deg = part.row_ptr[1:] - part.row_ptr[:-1]
        self._thr_in = torch.nonzero(
            (in_deg > 0) & (in_deg <= self.thr), as_tuple=True)[0].to(U32)
        self._wav_in = torch.nonzero(
            (in_deg > self.thr) & (in_deg <= hub), as_tuple=True)[0].to(U32)
        n_thr, n_wav = self._thr_in.numel(), self._wav_in.numel()
        if not n_thr:  # never read; the pointers stay valid
            self._thr_in = torch.zeros(1, dtype=U32, device=dev)
        if not n_wav:
            self._wav_in = torch.zeros(1, dtype=U32, device=dev)
        self._hub_in, n_hub, self.hub_rows_in = _items(in_deg, hub)
        out_deg = self.out_ptr[1:] - self.out_ptr[:-1]
        _, hubcap_out, self.hub_rows_out = _items(out_deg, hub)
        del in_deg, out_deg
        self.phase_ms["plan"] = 1000.0 * (self._now() - t0)

        def vec(dtype, n=nv):
            return torch.zeros(n, dtype=dtype, device=dev)

        self._seen, self._front, self._next = vec(U64), vec(U64), vec(U64)
        self._dist_sum, self._reach = vec(U64), vec(U32)
        self._harmonic = vec(torch.float64)
        self._qthr, self._qwav = vec(U32), vec(U32)
        self._qhub = vec(U32, 2 * max(hubcap_out, 1))
        self._meta = vec(U64, ng.msbfs_meta_words())
        self._bad = vec(U64, 1)
        self._args = ng.msbfs_args(
            (part.row_ptr, part.col, self.out_ptr, self.out_col, self._seen,
             self._front, self._next, self._dist_sum, self._harmonic,
             self._reach, self._thr_in, self._wav_in, self._hub_in,
             self._qthr, self._qwav, self._qhub, self._meta),
            nv, n_thr, n_wav, n_hub, hubcap_out, hub, self.thr)
        self._sources = None
        self._depths = self._seen_all = self._src_dev = None
        self._level_counts = []
        self.level_trace = []
        self._stats = self._fresh_stats()

    @staticmethod
    def _fresh_stats():
        return dict(levels=0, push_levels=0, pull_levels=0, launches=0,
                    host_reads=0, edges_scanned=0)

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    def _pull(self, volume):
        if self.direction != "auto":
            return self.direction == "pull"
        return volume * self.div > self.ne

    # -------- the traversal --------
    def run(self, sources, depths=False):
        """Traverse from every source; returns the device dist_sum,
        i64[nv]."""
        from . import _native_gpu as ng
        nv, B = self.part.nv, ng.MSBFS_BATCH
        try:
            src = [int(x) for x in sources]
        except (TypeError, ValueError):
            raise ValueError(f"sources must be a list of vertex ids, got "
                             f"{sources!r}") from None
        if not src or len(set(src)) != len(src) or \
                not 0 <= min(src) <= max(src) < nv:
            raise ValueError(f"sources must be at least one distinct vertex "
                             f"id in [0, {nv}), got {len(src)} "
                             f"({len(set(src))} distinct)")
        k = len(src)
        nb = (k + B - 1) // B
        t0 = self._now() if self.timed else 0.0
        dev, s, a = self.device, _stream(), self._args
        self._sources = src
        self._stats = st = self._fresh_stats()
        self.level_trace, self._level_counts = [], []
        self._src_dev = torch.tensor(src, dtype=U64, device=dev)
        # the depth-0 records: the out-degrees of the sources, one read
        deg0 = (self.out_ptr[self._src_dev + 1] -
                self.out_ptr[self._src_dev]).tolist()
        self._src_dev = self._src_dev.to(U32)
        self._depths = torch.full((k, nv), -1, dtype=U32, device=dev) \
            if depths else None
        self._seen_all = torch.empty((nb, nv), dtype=U64, device=dev)
        for t in (self._dist_sum, self._reach, self._harmonic):
            t.zero_()
        for b in range(nb):
            kb = min(B, k - b * B)
            active = (1 << kb) - 1
            depth = self._depths[b * B:] if depths else None
            for t in (self._seen, self._front, self._next, self._meta):
                t.zero_()
            ng.msbfs_seed(s, a, self._src_dev[b * B:], kb)
            ng.msbfs_epilogue(s, a, 0, kb, depth)
            self._meta.zero_()  # the host already has this record
            st["launches"] += 2
            degs = deg0[b * B:b * B + kb]
            front, volume, pairs = kb, sum(degs), kb
            nthr = sum(1 for d in degs if 0 < d <= self.thr)
            nwav = sum(1 for d in degs if self.thr < d <= self.hub)
            nhub = sum(-(-d // self.hub) for d in degs if d > self.hub)
            counts = [[1] for _ in range(kb)]
            level = 0
            while front:
                if level > nv:
                    raise RuntimeError(f"multi-source BFS does not end: "
                                       f"level {level} of {nv} vertices")
                pull = self._pull(volume)
                self.level_trace.append(
                    (b, level, "pull" if pull else "push", front, volume,
                     pairs))
                if pull:
                    ng.msbfs_pull(s, a, active)
                else:
                    ng.msbfs_push(s, a, nthr, nwav, nhub)
                level += 1
                ng.msbfs_epilogue(s, a, level, kb, depth)
                m = self._meta.tolist()
                self._meta.zero_()
                st["pull_levels" if pull else "push_levels"] += 1
                st["launches"] += 2
                st["host_reads"] += 1
                st["edges_scanned"] += m[ng.MSBFS_M_SCANNED]
                front, volume, pairs = m[ng.MSBFS_M_FRONT], \
                    m[ng.MSBFS_M_VOLUME], m[ng.MSBFS_M_PAIRS]
                nthr, nwav, nhub = m[ng.MSBFS_M_NTHR], m[ng.MSBFS_M_NWAV], \
                    m[ng.MSBFS_M_NHUB]
                if front > nv or nthr + nwav > front or \
                        nhub > a.hubcap_out or pairs > front * kb:
                    raise RuntimeError(
                        f"multi-source BFS record out of bounds at level "
                        f"{level}: frontier {front} of {nv}, queues {nthr} "
                        f"/ {nwav} / {nhub} (hub capacity {a.hubcap_out}), "
                        f"pairs {pairs}")
                for i in range(kb):
                    c = m[ng.MSBFS_M_SRC + i]
                    if c:
                        counts[i].append(c)
            self._seen_all[b] = self._seen
            self._level_counts += counts
        st["levels"] = st["push_levels"] + st["pull_levels"]
        if self.timed:
            self.phase_ms["run"] = 1000.0 * (self._now() - t0)
        return self._dist_sum

    def _ran(self):
        if self._sources is None:
            raise ValueError("no result yet: call run(sources) first")

    # -------- per-vertex results (device) --------
    def seen(self):
        """Device i64[batches, nv]: bit i of row b is set iff the vertex is
        reached from source 64 * b + i."""
        self._ran()
        return self._seen_all

    def reach(self):
        self._ran()
        return self._reach

    def dist_sum(self):
        self._ran()
        return self._dist_sum

    def harmonic(self):
        self._ran()
        return self._harmonic

    def depths(self):
        """Device i32[k, nv], -1 where unreached; kept by
        run(depths=True)."""
        self._ran()
        if self._depths is None:
            raise ValueError("depths were not kept: run(sources, "
                             "depths=True)")
        return self._depths

    # -------- per-source results (host) --------
    def level_counts(self):
        """k lists: the vertices at distance 0, 1, ... of each source. A
        vertex count per level is contiguous: a level without a vertex ends
        a source's traversal."""
        self._ran()
        return [list(c) for c in self._level_counts]

    def reached(self):
        return np.array([sum(c) for c in self.level_counts()], np.int64)

    def farness(self):
        return np.array([sum(d * n for d, n in enumerate(c))
                         for c in self.level_counts()], np.int64)

    def eccentricity(self):
        return np.array([len(c) - 1 for c in self.level_counts()], np.int64)

    def closeness(self):
        r = self.reached().astype(np.float64) - 1.0
        f = self.farness().astype(np.float64)
        return np.divide(r, f, out=np.zeros_like(f), where=f > 0)

    @property
    def stats(self):
        return dict(hub_rows_in=self.hub_rows_in,
                    hub_rows_out=self.hub_rows_out, **self._stats)

    def check(self):
        """Device check (msbfs_check_kernel), summed over the batches: the
        edges u -> v with a bit of seen[u] missing in seen[v]; the sources
        whose own bit is missing at their own vertex; with depths kept, the
        (edge, source) pairs where u has a depth and v has none or one
        larger than depth[u] + 1, the sources whose own depth is not 0, and
        the depths whose sign disagrees with the seen bit. Necessary, not
        sufficient (a depth that is too small passes): exactness rests on
        the tests against the CPU oracle."""
        from . import _native_gpu as ng
        self._ran()
        B, k = ng.MSBFS_BATCH, len(self._sources)
        self._bad.zero_()
        for b in range(self._seen_all.shape[0]):
            depth = None if self._depths is None else self._depths[b * B:]
            ng.msbfs_check(_stream(), self._args, self._seen_all[b], depth,
                           self._src_dev[b * B:], min(B, k - b * B),
                           self._bad)
        return int(self._bad.item())
