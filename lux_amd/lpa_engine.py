"""Community detection on one GPU: semi-synchronous label propagation, one
colour class at a time (src/gpu/lpa.hip). No reference equivalent.

Definition — the same graph as KCoreEngine: the underlying simple undirected
graph of whatever the project loads, N(v) the neighbours, deg the degree, m
the simple edges, everything in the caller's vertex ids.
  colour = the greedy colouring of ColouringEngine(order, seed);
  seq    = all vertices sorted by (colour, id);
  label[v] starts as v (or init[v]), dirty[v] as true.
One sweep visits seq in order. A vertex with deg > 0 and dirty[v] clears
dirty[v], counts cnt(l) = |{u in N(v) : label[u] == l}|, and unless
cnt(label[v]) is the maximum takes the smallest l of maximum count and sets
dirty[u] for all u in N(v). The solve ends after the first sweep without a
change (or after max_sweeps sweeps). A colour class is an independent set,
so evaluating it in parallel equals evaluating it in id order: the result
does not depend on the schedule. Every change raises the number of
monochromatic edges, so there are at most m changes.

Preparation (timed as phase_ms["orient"], ["adjacency"], ["colour"],
["plan"]): tc_engine.orient(..., "id") and kcore_adj_fill give the full
adjacency aptr / aadj; a ColouringEngine on the same part gives the colours
and is freed; vorder is a stable sort of the colours, cptr their counts
scanned. Rows longer than the table role's limit become hub items (vertex,
pass), listed in class order. The launch plan is static: consecutive classes
that together hold at most LUX_LPA_FUSE vertices and no hub row are one
single-workgroup launch, every other class is one launch. A sweep replays
the plan and reads the meta record once. Every host tensor is
one-dimensional, and none that scales with m is written through a mask or an
index.

Env knobs: LUX_LPA_HUB (rows longer than this go through hub items; default
the kernels' LPA_HUB; the table role also never takes a row longer than
LUX_LPA_TABLE / 8, nor the hub role one of 64 or less: `hub` is the limit in
force), LUX_LPA_TABLE (slots of the workgroup's LDS table, a power of two;
default LPA_TABLE), LUX_LPA_FUSE (vertices of a fused launch, 0 = off;
default LPA_FUSE).
"""
import os
import time

import torch

from .colouring_engine import ORDERS, ColouringEngine
from .engine import GraphPart
from .tc_engine import orient

U32, U64 = torch.int32, torch.int64
NONE = 0xFFFFFFFF
HUB_MIN, HUB_MAX = 64, 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


class LPAEngine:
    def __init__(self, part: GraphPart, order="degree", seed=1):
        if part.nparts != 1:
            raise ValueError(
                "LPAEngine is single-rank: a class reads its neighbours' "
                "labels on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        if order not in ORDERS:
            raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_LPA_HUB", ng.lpa_hub_default()))
        if not HUB_MIN <= hub <= HUB_MAX:
            raise ValueError(f"LUX_LPA_HUB={hub} outside "
                             f"[{HUB_MIN}, {HUB_MAX}]")
        table = int(os.environ.get("LUX_LPA_TABLE", ng.lpa_table_default()))
        tmin, tmax = ng.lpa_table_range()
        if not tmin <= table <= tmax or table & (table - 1):
            raise ValueError(f"LUX_LPA_TABLE={table} is not a power of two "
                             f"in [{tmin}, {tmax}]")
        fuse = int(os.environ.get("LUX_LPA_FUSE", ng.lpa_fuse_default()))
        if not 0 <= fuse <= ng.lpa_fuse_max():
            raise ValueError(f"LUX_LPA_FUSE={fuse} outside "
                             f"[0, {ng.lpa_fuse_max()}]")
        self.part = part
        self.device = part.device
        self.order, self.seed = order, int(seed)
        self.hub, self.table, self.fuse = ng.lpa_row_limit(hub, table), \
            table, fuse
        self.timed = False  # synchronise and clock solve() (the app)
        self.phase_ms = dict(orient=0.0, adjacency=0.0, colour=0.0, plan=0.0,
                             solve=0.0)
        nv = part.nv
        n1 = max(nv, 1)
        dev = self.device

        t0 = self._now()
        dag = orient(part.row_ptr, part.col, nv, "id")
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)

        t0 = self._now()
        self.m = dag.m
        indeg = torch.zeros(n1, dtype=U32, device=dev)
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
        del dag, indeg
        self.phase_ms["adjacency"] = 1000.0 * (self._now() - t0)

        t0 = self._now()
        ce = ColouringEngine(part, order=order, seed=seed)
        colour = ce.colours().to(U64).clone()
        self.colours = ce.num_colours()
        del ce
        self.phase_ms["colour"] = 1000.0 * (self._now() - t0)

        t0 = self._now()
        C = self.colours
        self.vorder = torch.sort(colour, stable=True).indices.to(U32)
        count = torch.bincount(colour, minlength=C)
        cptr = torch.zeros(C + 1, dtype=U64, device=dev)
        cptr[1:] = torch.cumsum(count, 0)
        deg64 = self.degree.to(U64)
        cmax = torch.zeros(max(C, 1), dtype=U64, device=dev)
        cmax.scatter_reduce_(0, colour, deg64, "amax")
        # hub rows in class order, and one item per pass of each
        half = table // 2
        vo = self.vorder.to(U64)
        dv = deg64[vo]
        is_hub = dv > self.hub
        hv, hd = vo[is_hub], dv[is_hub]
        passes = (hd + (half - 1)) // half
        self.hub_rows = int(hv.numel())
        self.hub_items = int(passes.sum().item())
        hubr = torch.repeat_interleave(
            torch.arange(self.hub_rows, dtype=U64, device=dev), passes)
        first = torch.cumsum(passes, 0) - passes
        hubp = torch.arange(self.hub_items, dtype=U64, device=dev) - \
            torch.repeat_interleave(first, passes)
        per_class = torch.zeros(max(C, 1), dtype=U64, device=dev)
        per_class.index_add_(0, colour[hv], passes)
        hptr = torch.zeros(C + 1, dtype=U64, device=dev)
        hptr[1:] = torch.cumsum(per_class[:C], 0)
        self._cptr, self._hptr = cptr.to(U32), hptr.to(U32)
        self._hubv = torch.repeat_interleave(hv, passes).to(U32)
        self._hubp, self._hubr = hubp.to(U32), hubr.to(U32)
        if not self.hub_items:  # never read; the pointers stay valid
            self._hubv = torch.zeros(1, dtype=U32, device=dev)
            self._hubp, self._hubr = self._hubv.clone(), self._hubv.clone()
        self._plan, self.fused_classes = self._make_plan(
            count.tolist(), per_class[:C].tolist(), cmax[:C].tolist())
        del colour, count, cmax, deg64, vo, dv, is_hub, hv, hd, passes
        del hubr, hubp, first, per_class, cptr, hptr
        self.phase_ms["plan"] = 1000.0 * (self._now() - t0)

        self._label = torch.empty(n1, dtype=U32, device=dev)
        self._dirty = torch.empty(n1, dtype=U32, device=dev)
        self._hubkey = torch.zeros(max(self.hub_rows, 1), dtype=U64,
                                   device=dev)
        self._hubdone = torch.zeros(max(self.hub_rows, 1), dtype=U32,
                                    device=dev)
        self._meta = torch.zeros(ng.lpa_meta_words(), dtype=U32, device=dev)
        self._bad = torch.zeros(1, dtype=U64, device=dev)
        self._args = ng.lpa_args(
            self.aptr, self.aadj, self.vorder, self._cptr, self._label,
            self._dirty, self._hubv, self._hubp, self._hubr, self._hptr,
            self._hubkey, self._hubdone, self._meta, self._bad, nv, C,
            self.hub_items, self.hub_rows, self.hub, table)
        self._done = self._converged = False
        self._host_reads = 0
        self._trace = []
        self._derived = None

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    def _make_plan(self, count, items, cmax):
        """The launches of a sweep, [(c0, c1, rows, items, max degree,
        fused)], and the number of classes in fused launches."""
        plan, fused_classes, c, C = [], 0, 0, len(count)
        while c < C:
            c1, rows = c, 0
            while self.fuse and c1 < C and items[c1] == 0 and \
                    rows + count[c1] <= self.fuse:
                rows += count[c1]
                c1 += 1
            if c1 - c >= 2:
                plan.append((c, c1, rows, 0, max(cmax[c:c1]), True))
                fused_classes += c1 - c
                c = c1
            else:
                plan.append((c, c + 1, count[c], items[c], cmax[c], False))
                c += 1
        return plan, fused_classes

    # -------- the sweeps --------
    def solve(self, init=None, max_sweeps=0):
        """Propagate until a sweep changes nothing (or for max_sweeps sweeps
        if max_sweeps > 0); returns the device labels, i32[nv]."""
        from . import _native_gpu as ng
        nv = self.part.nv
        if init is not None:
            init = torch.as_tensor(init)
            if init.dtype not in (torch.uint8, torch.int8, torch.int16,
                                  torch.int32, torch.int64) or \
                    tuple(init.shape) != (nv,):
                raise ValueError(f"init must be an integer tensor of shape "
                                 f"[{nv}], got {init.dtype} "
                                 f"{tuple(init.shape)}")
            if nv and not 0 <= int(init.min()) <= int(init.max()) < nv:
                raise ValueError(f"init labels must lie in [0, {nv})")
        self._done = self._converged = False
        self._host_reads, self._trace, self._derived = 0, [], None
        t0 = self._now() if self.timed else 0.0
        if init is None:
            self._label[:nv] = torch.arange(nv, dtype=U32,
                                            device=self.device)
        else:
            self._label[:nv] = init.to(self.device, U32)
        self._dirty.fill_(1)
        self._hubkey.zero_()
        self._hubdone.zero_()
        s, a = _stream(), self._args
        while True:
            self._meta.zero_()
            for c0, c1, rows, items, maxdeg, fused in self._plan:
                ng.lpa_classes(s, a, c0, c1, rows, items, maxdeg, fused)
            meta = [x & NONE for x in self._meta.tolist()]
            self._host_reads += 1
            k = len(self._trace) + 1
            evaluated, changed = meta[ng.LPA_M_EVAL], meta[ng.LPA_M_CHANGED]
            self._trace.append((k, evaluated, changed))
            if changed > evaluated or evaluated > nv or k > self.m + 1:
                raise RuntimeError(
                    f"label propagation out of bounds: sweep {k} evaluated "
                    f"{evaluated} changed {changed}, nv={nv} m={self.m}")
            if changed == 0 or (max_sweeps > 0 and k >= max_sweeps):
                break
        self._converged = changed == 0
        if self.timed:
            self.phase_ms["solve"] = 1000.0 * (self._now() - t0)
        self._done = True
        return self._label[:nv]

    def labels(self):
        """Device i32[nv]: the label per vertex, a vertex id of its
        community. The stored array of the last solve(); solved now if there
        is none."""
        if not self._done:
            self.solve()
        return self._label[:self.part.nv]

    def converged(self):
        self.labels()
        return self._converged

    def sweeps(self):
        self.labels()
        return len(self._trace)

    @property
    def sweep_trace(self):
        """[(sweep, evaluated, changed)], sweeps counted from 1."""
        self.labels()
        return list(self._trace)

    def _stats_of_labels(self):
        """(sizes, tot, intra) of the stored labels, lpa_stats_kernel."""
        if self._derived is None:
            from . import _native_gpu as ng
            nv = self.part.nv
            lab = self.labels()
            sizes = torch.zeros(max(nv, 1), dtype=U64, device=self.device)
            tot = torch.zeros(max(nv, 1), dtype=U64, device=self.device)
            intra = torch.zeros(1, dtype=U64, device=self.device)
            ng.lpa_stats(_stream(), nv, self.aptr, self.aadj, lab, sizes,
                         tot, intra)
            self._derived = (sizes[:nv], tot[:nv], int(intra.item()))
        return self._derived

    def sizes(self):
        """Device i64[nv]: the vertices of the community at each label id,
        0 elsewhere."""
        return self._stats_of_labels()[0]

    def community_degrees(self):
        """Device i64[nv]: the sum of deg over the community at each label
        id."""
        return self._stats_of_labels()[1]

    def intra_edges(self):
        """The simple edges whose two ends carry the same label."""
        return self._stats_of_labels()[2]

    def num_communities(self):
        return int((self.sizes() > 0).sum().item())

    def modularity(self):
        """intra / m - sum(tot[l]^2) / (4 m^2), in exact integer arithmetic
        on the host; 0.0 for m == 0."""
        from .cpu_ref import modularity
        tot = self.community_degrees()
        return modularity(self.intra_edges(), self.m, tot[tot > 0].tolist())

    def member_mask(self, label):
        """Device bool[nv]: the vertices of the community `label`."""
        return self.labels() == int(label)

    @property
    def stats(self):
        return dict(simple_edges=self.m, colours=self.colours,
                    max_degree=self.max_degree, launches=len(self._plan),
                    fused_classes=self.fused_classes, hub_rows=self.hub_rows,
                    hub_items=self.hub_items, sweeps=len(self._trace),
                    host_reads=self._host_reads)

    def check(self):
        """Device check (the class kernel in check mode): the vertices with
        deg > 0 whose own label is less frequent among their neighbours than
        the most frequent one, i.e. that another sweep would change. Zero is
        necessary for a converged result, not sufficient for the right one:
        exactness rests on the tests against the CPU oracle. Raises after a
        solve that did not converge."""
        from . import _native_gpu as ng
        self.labels()
        if not self._converged:
            raise ValueError(
                f"check() after a solve that did not converge "
                f"({len(self._trace)} sweeps, the last changed "
                f"{self._trace[-1][2]})")
        self._bad.zero_()
        ng.lpa_check(_stream(), self._args)
        return int(self._bad.item())
