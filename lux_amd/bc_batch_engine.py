"""Batched betweenness centrality on one GPU: the Brandes dependencies of
16 / 32 / 64 sources per level sweep (src/gpu/bc_batch.hip). No reference
equivalent.

The per-source definition and conventions are BCEngine's (bc_engine.py):
directed graph, parallel edges are distinct paths, self-loops never pass the
depth test, unreached vertices have sigma = delta = 0, delta[s] = 0, no
halving. bc[v] is the sum over the given sources of delta_s[v], in fp32.
The result is a pure function of the graph, the source list, the width B and
the hub knob: no float atomics, so two runs give the same bits.

Sources run in batches of B, the last one padded with unreached columns.
Per batch: one MSBFSEngine.run(batch, depths=True) for the hop depths;
prepare (transpose the depths to u16 [nv][B], sigma = 1 at the sources); the
level lists of both directions (histogram, device scan, one host read of the
offsets table, scatter); the forward levels 1..L-1 over the CSC; a leaf
launch for level L-1 and the backward levels L-2..1 over the MSBFSEngine's
out-edge CSR; the column sum into bc. One launch per level and pass (two
with hub rows), every launch dimension from the two offsets tables.

Env knob: LUX_BCB_HUB (default the kernels' BCB_HUB, 64..2^20): the longest
row one wave takes; longer rows are split into items of that many edges.
"""
import os
import time

import torch

from . import _native_gpu as ng
from .engine import GraphPart
from .msbfs_engine import MSBFSEngine

I16, U32, U64, F32 = torch.int16, torch.int32, torch.int64, torch.float32
EPS32 = 2.0 ** -24
PHASES = ("bfs", "order", "sigma", "delta", "reduce")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class BatchedBCEngine:
    def __init__(self, part: GraphPart, width=None):
        if part.nparts != 1:
            raise ValueError(
                "BatchedBCEngine is single-rank: the delta pass needs a "
                f"per-level sum across ranks (got a GraphPart with nparts="
                f"{part.nparts})")
        if width is not None and width not in ng.BCB_WIDTHS:
            raise ValueError(f"width={width!r} is not one of "
                             f"{', '.join(map(str, ng.BCB_WIDTHS))}")
        hub = int(os.environ.get("LUX_BCB_HUB", ng.bcb_hub_default()))
        if not ng.bcb_hub_min() <= hub <= ng.bcb_hub_max():
            raise ValueError(f"LUX_BCB_HUB={hub} outside "
                             f"[{ng.bcb_hub_min()}, {ng.bcb_hub_max()}]")
        if part.nv < 1:
            raise ValueError("BatchedBCEngine needs at least one vertex")
        self.part = part
        self.device = part.device
        self.width, self.hub = width, hub
        # hop depths of a batch, and the out-edge CSR of the backward pass
        self.ms = MSBFSEngine(part)
        nv = part.nv

        def maxdeg(rp):
            return int((rp[1:nv + 1] - rp[:nv]).max().item())
        self.maxdeg = max(maxdeg(part.row_ptr), maxdeg(self.ms.out_ptr))
        self._bc = torch.zeros(nv, dtype=F32, device=self.device)
        self._out = torch.zeros(2, dtype=U64, device=self.device)
        self.B = 0
        self._dep = self._val = self._delta = self._sigma = None
        self._scratch = None
        self._kept = False
        self.levels = 0
        self.timed = False  # synchronise and clock each phase (the app)
        self.phase_ms = dict.fromkeys(PHASES, 0.0)
        self._off = []
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

    def _state(self, B):
        if B != self.B:
            nv, dev = self.part.nv, self.device
            self._dep = torch.empty((nv, B), dtype=I16, device=dev)
            self._val = torch.empty((nv, B), dtype=F32, device=dev)
            self._delta = torch.empty((nv, B), dtype=F32, device=dev)
            self._sigma = self._scratch = None
            self.B = B

    def _order(self, row_ptr):
        """Level lists of one direction. Returns the host copy of the table
        (3L+1 word offsets, key = depth*3 + role, then L hub-row counts) and
        the list, sized by the table. The .cpu() below is the direction's
        one host read."""
        s, L, nv, dev = _stream(), self.levels, self.part.nv, self.device
        cnt = torch.zeros(3 * L, dtype=U32, device=dev)
        tab = torch.zeros(4 * L + 1, dtype=U64, device=dev)
        ng.bcb_order_hist(s, nv, self.B, self._dep, row_ptr, L, self.hub, cnt,
                          tab.narrow(0, 3 * L + 1, L))
        partials = torch.empty(max(ng.scan_partials_size(3 * L), 1),
                               dtype=U64, device=dev)
        ng.scan_end_offsets(s, 3 * L, cnt, tab.narrow(0, 1, 3 * L), partials)
        cursor = tab.narrow(0, 0, 3 * L).clone()
        host = tab.cpu().numpy()
        total = int(host[3 * L])
        lst = torch.empty(max(total, 1), dtype=U32, device=dev)
        ng.bcb_order_scatter(s, nv, self.B, self._dep, row_ptr, L, self.hub,
                             cursor, lst, total)
        return host, lst

    def _level(self, forward, lst, off, d, row_ptr, adj, edges, leaf=False):
        o = [int(x) for x in off[3 * d:3 * d + 4]]
        a = ng.BcbLevel(
            lst.data_ptr(), row_ptr.data_ptr(), adj.data_ptr(),
            self._dep.data_ptr(), self._val.data_ptr(),
            self._delta.data_ptr(), self._scratch.data_ptr(), edges,
            o[0], o[1], o[2], o[3], self._scratch.numel() // self.B,
            self.part.nv, self.B, self.hub, d, int(leaf))
        ng.bcb_level(_stream(), a, forward)

    def _batch(self, batch, keep_sigma):
        p, s, B, dev = self.part, _stream(), self.B, self.device
        t0 = self._tick()
        self.ms.run(batch, depths=True)
        self.levels = L = max(len(c) for c in self.ms.level_counts())
        if L > ng.bcb_max_levels():
            raise ValueError(f"a batch of {L} levels does not fit the u16 "
                             f"depths (at most {ng.bcb_max_levels()})")
        self._tock("bfs", t0)

        t0 = self._tick()
        ng.bcb_prepare(s, p.nv, B, len(batch), self.ms.depths(), self._dep,
                       self._val, self._delta)
        off_in, list_in = self._order(p.row_ptr)
        off_out, list_out = self._order(self.ms.out_ptr)
        items = max(int(off[3 * d + 3] - off[3 * d + 2]) // 2
                    for off in (off_in, off_out) for d in range(L))
        if self._scratch is None or self._scratch.numel() < items * B:
            self._scratch = torch.empty(max(items, 1) * B, dtype=F32,
                                        device=dev)
        edges = torch.zeros(2 * L, dtype=U64, device=dev)
        eaddr = edges.data_ptr()
        self._tock("order", t0)

        t0 = self._tick()
        for d in range(1, L):
            self._level(True, list_in, off_in, d, p.row_ptr, p.col,
                        eaddr + 8 * d)
        if keep_sigma:
            if self._sigma is None:
                self._sigma = torch.empty_like(self._val)
            self._sigma.copy_(self._val)
        self._tock("sigma", t0)

        t0 = self._tick()
        for d in range(L - 1, 0, -1):
            # the deepest level has nothing below it: its rows only publish
            # q = 1 / sigma (the leaf launch gathers nothing)
            self._level(False, list_out, off_out, d, self.ms.out_ptr,
                        self.ms.out_col, eaddr + 8 * (L + d), leaf=d == L - 1)
        self._tock("delta", t0)

        t0 = self._tick()
        ng.bcb_reduce(s, p.nv, B, self._delta, self._bc)
        self._tock("reduce", t0)
        self._off.append((off_in, off_out, edges, L))

    def run(self, sources, keep_sigma=False):
        """bc = the sum of delta over `sources` (restarts the sum); returns
        it (device f32[nv])."""
        nv = self.part.nv
        try:
            src = [int(x) for x in sources]
        except (TypeError, ValueError):
            raise ValueError(f"sources must be a list of vertex ids, got "
                             f"{sources!r}") from None
        if not src:
            raise ValueError("sources is empty: need at least one vertex id")
        if len(set(src)) != len(src):
            raise ValueError(f"sources holds duplicates ({len(src)} ids, "
                             f"{len(set(src))} distinct)")
        if not 0 <= min(src) <= max(src) < nv:
            raise ValueError(f"source {min(src) if min(src) < 0 else max(src)}"
                             f" outside [0, {nv})")
        B = self.width or next(w for w in ng.BCB_WIDTHS
                               if w >= min(len(src), 64))
        self._state(B)
        self._bc.zero_()
        self.phase_ms = dict.fromkeys(PHASES, 0.0)
        self._off, self._stats = [], None
        self._kept = False
        for b in range(0, len(src), B):
            self._batch(src[b:b + B], keep_sigma)
        self._kept = bool(keep_sigma)
        return self._bc

    # -------- results --------
    def _ran(self):
        if not self._off:
            raise ValueError("no result yet: call run(sources) first")

    def bc(self):
        return self._bc

    def depths(self):
        """Last batch, device i16[nv, B]: the bits of the u16 depths, 0xFFFF
        (-1) where unreached and in the padding columns."""
        self._ran()
        return self._dep

    def sigma(self):
        """Last batch, device f32[nv, B]; kept by run(sources,
        keep_sigma=True)."""
        self._ran()
        if not self._kept:
            raise ValueError("sigma was not kept: run(sources, "
                             "keep_sigma=True)")
        return self._sigma

    def delta(self):
        self._ran()
        return self._delta

    @property
    def stats(self):
        """One row per batch and level. rows_*: entries the level lists for
        the pass (a row is listed once per distinct depth of its columns);
        edges_*: (edge, column) pairs that passed the depth test, i.e. the
        level's BFS-DAG edges summed over the batch. The sigma pass skips
        level 0, the delta pass levels 0 and L-1."""
        if self._stats is None:
            self._stats = []
            for b, (off_in, off_out, edges, L) in enumerate(self._off):
                e = edges.cpu().numpy()

                def rows(off, d):
                    return int(off[3 * d + 2] - off[3 * d] +
                               off[3 * L + 1 + d])
                self._stats += [dict(batch=b, level=d,
                                     rows_in=rows(off_in, d),
                                     edges_in=int(e[d]),
                                     rows_out=rows(off_out, d),
                                     edges_out=int(e[L + d]))
                                for d in range(L)]
        return self._stats

    def rtol(self):
        """BCEngine.rtol() of the last batch, plus B * 2^-24 for the column
        sum."""
        return 1.01 * max(self.levels, 1) * (self.maxdeg + 3) * EPS32 + \
            self.B * EPS32

    def check(self):
        """Device check oracle (bcb_plain_kernel) of the last batch: the
        (vertex, column) entries whose sigma or delta, recomputed from the
        final arrays, misses the stored value by more than rtol(), plus the
        reached entries with a non-finite sigma."""
        p = self.part
        sigma = self.sigma()
        self._out.zero_()
        ng.bcb_check(_stream(), p.nv, self.B, p.row_ptr, p.col,
                     self.ms.out_ptr, self.ms.out_col, self._dep, sigma,
                     self._delta, self.rtol(), self._out)
        return int(self._out.sum().item())
