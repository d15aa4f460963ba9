"""Strongly connected components on one GPU: trim, one forward-backward
pass on the giant, then colouring, with device-side queues
(src/gpu/scc.hip). No reference equivalent.

Definition — the directed graph exactly as loaded: row v of the CSC lists
the sources u of the edges u -> v; parallel edges and self-loops change
nothing and are not removed.
  u and v are in the same SCC iff each reaches the other;
  label[v] = the largest vertex id of v's SCC (u32, the caller's ids), so
             label[v] >= v, label[label[v]] == label[v], and a vertex alone
             in its SCC has label[v] == v.

Preparation (timed as phase_ms["csr"]): the out-edge CSR, built like
PushEngine's push_row_ptr / push_col (a histogram of the sources, a scan, a
scatter), and the static {vertex, chunk} list of the rows longer than the
hub length, which sizes the hub queue and is the work list of the recount.

decompose() follows tests/scc_ref.sync_schedule phase for phase:
  a. trim to fixpoint: a round removes every alive vertex without an alive
     in- or out-neighbour and decrements its neighbours' counters;
  b. the pivot (max in_cnt * out_cnt, lowest id first), a forward and a
     backward traversal from it, the intersection dies with its largest id;
  c. recount and trim;
  d. colour rounds while anything is alive: colour = id, the maximum
     propagated along alive out-edges to its fixpoint, one backward
     traversal from all roots (colour == id) inside equal colours, the
     reached die with label = colour; recount and trim.
Queues, counters and marks live in the kernels; the host keeps a handful of
cursors, launches one kernel per step and reads the 16-word meta record back
once per launch. Small steps (at most LUX_SCC_FUSE entries, no hub row) are
run by a single-workgroup kernel that loops over them, so a path or a cycle
costs a constant number of launches. The statistics equal the schedule's,
except colour_sweeps: the atomic propagation may move a colour several hops
in one step, so the schedule's Jacobi sweep count is an upper bound. Every
host tensor is one-dimensional, and none that scales with ne is written
through a mask or an index.

Env knobs: LUX_SCC_HUB (rows longer than this are walked by workgroups, in
chunks of this many entries; default the kernels' SCC_HUB), LUX_SCC_FUSE
(largest step the single-workgroup kernel takes, 0 = off; default the
kernels' SCC_FUSE).
"""
import os
import time

import torch

from .engine import GraphPart

U32, U64 = torch.int32, torch.int64
NONE = 0xFFFFFFFF
HUB_MAX = 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


class SCCEngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "SCCEngine is single-rank: a traversal follows edges in "
                "both directions on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_SCC_HUB", ng.scc_hub_default()))
        if not 1 <= hub <= HUB_MAX:
            raise ValueError(f"LUX_SCC_HUB={hub} outside [1, {HUB_MAX}]")
        fuse = int(os.environ.get("LUX_SCC_FUSE", ng.scc_fuse_default()))
        if not 0 <= fuse <= ng.scc_fuse_max():
            raise ValueError(f"LUX_SCC_FUSE={fuse} outside "
                             f"[0, {ng.scc_fuse_max()}]")
        self.part = part
        self.device = dev = part.device
        self.hub, self.fuse = hub, fuse
        self.timed = False  # synchronise and clock decompose() (the app)
        self.phase_ms = dict(csr=0.0, trim=0.0, fwbw=0.0, colour=0.0)
        nv, ne = part.nv, part.ep
        n1 = max(nv, 1)
        s = _stream()

        # ---- out-edge CSR: all sources -> their targets ----
        t0 = self._now()
        self.in_ptr, self.in_col = part.row_ptr, part.col
        out_deg = torch.zeros(n1, dtype=U32, device=dev)
        if ne:
            ng.hist_u32(s, ne, part.col, out_deg)
        ends = torch.empty(n1, dtype=U64, device=dev)
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
        in_deg = self.in_ptr[1:] - self.in_ptr[:-1]
        out_deg = out_deg[:nv].to(U64)
        self.max_in_degree = int(in_deg.max().item()) if nv else 0
        self.max_out_degree = int(out_deg.max().item()) if nv else 0
        # the {vertex, chunk} items of every row longer than hub, in-row
        # chunks first: what hubq holds if every vertex is queued once in
        # the trim mode, and the static work list of the recount
        chunks_in = torch.where(in_deg > hub, (in_deg + (hub - 1)) // hub,
                                torch.zeros_like(in_deg))
        vs, cs = [], []
        for deg, base in ((in_deg, torch.zeros_like(in_deg)),
                          (out_deg, chunks_in)):
            hv = torch.nonzero(deg > hub, as_tuple=True)[0]
            nc = (deg[hv] + (hub - 1)) // hub
            vs.append(torch.repeat_interleave(hv, nc))
            first = torch.repeat_interleave(torch.cumsum(nc, 0) - nc, nc)
            cs.append(torch.arange(vs[-1].numel(), device=dev) - first +
                      torch.repeat_interleave(base[hv], nc))
        self.hubcap = vs[0].numel() + vs[1].numel()
        self._hublist = torch.zeros(2 * max(self.hubcap, 1), dtype=U32,
                                    device=dev)
        if self.hubcap:
            self._hublist[0::2] = torch.cat(vs).to(U32)
            self._hublist[1::2] = torch.cat(cs).to(U32)
        del ends, partials, in_deg, out_deg, chunks_in, vs, cs
        self.phase_ms["csr"] = 1000.0 * (self._now() - t0)

        def vec(n=n1):
            return torch.empty(n, dtype=U32, device=dev)

        self._label, self._in_cnt, self._out_cnt = vec(), vec(), vec()
        self._colour, self._mark, self._stamp = vec(), vec(), vec()
        self._tq = vec()        # trim: every vertex at most once per run
        self._rq = vec(2 * n1)  # reach: the forward, then the backward list
        self._cq = vec(2 * n1)  # colour: two halves of nv
        # append modes use all of it, colour steps one half each
        self._hubq = vec(4 * max(self.hubcap, 1))
        self._meta = torch.zeros(ng.scc_meta_words(), dtype=U32, device=dev)
        self._bad = torch.zeros(1, dtype=U64, device=dev)
        self._args = ng.scc_args(
            self.in_ptr, self.in_col, self.out_ptr, self.out_col,
            self._label, self._in_cnt, self._out_cnt, self._colour,
            self._mark, self._stamp, self._hubq, self._meta, nv, hub)
        self._done = False
        self._stats = self._fresh_stats()
        self.events = []  # (kind, round, removed) per phase event

    @staticmethod
    def _fresh_stats():
        return dict(trim_rounds=0, trimmed=0, pivot=None, fwbw=0,
                    reach_rounds=0, colour_rounds=0, colour_sweeps=0,
                    launches=0, host_reads=0, fused_steps=0, hub_items=0)

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    # -------- the host loop --------
    def _read_meta(self, kernels=1):
        """The blocking read of the meta record (u32 values), one per
        launch (an entry point that runs two kernels in a row counts as
        one read and two launches)."""
        self._stats["launches"] += kernels
        self._stats["host_reads"] += 1
        return [x & NONE for x in self._meta.tolist()]

    def _drain(self, st, head, tail, hubhead, hubtail):
        """Run the steps of an append-mode list from [head, tail) on until a
        step is empty. Returns (steps, tail, hubtail)."""
        from . import _native_gpu as ng
        stats, nv, s = self._stats, self.part.nv, _stream()
        steps = launches = 0
        while head < tail:
            if not tail <= st.qcap or hubtail > st.hcap or \
                    not hubhead <= hubtail or steps > nv + launches:
                raise RuntimeError(
                    f"SCC step out of bounds: mode={st.mode} head={head} "
                    f"tail={tail} cap={st.qcap} hub=[{hubhead}, {hubtail}) "
                    f"hubcap={st.hcap} steps={steps} launches={launches}")
            launches += 1
            stats["hub_items"] += hubtail - hubhead
            if self.fuse and tail - head <= self.fuse and hubtail == hubhead:
                ng.scc_tail(s, self._args, st, head, tail, hubtail, self.fuse)
                m = self._read_meta()
                steps += m[ng.SCC_M_FUSED]
                stats["fused_steps"] += m[ng.SCC_M_FUSED]
                if not head < m[ng.SCC_M_HEAD] <= m[st.mw]:
                    raise RuntimeError(
                        f"SCC tail kernel went backwards: head={head} -> "
                        f"{m[ng.SCC_M_HEAD]}, cursor={m[st.mw]}")
                head = m[ng.SCC_M_HEAD]
            else:
                ng.scc_step(s, self._args, st, head, tail, hubhead, hubtail)
                m = self._read_meta()
                steps += 1
                head, hubhead = tail, hubtail
            tail, hubtail = m[st.mw], m[ng.SCC_M_HUBTAIL]
        return steps, tail, hubtail

    def _trim(self):
        """Recount the alive subgraph and trim it to the fixpoint."""
        from . import _native_gpu as ng
        t0 = self._now() if self.timed else 0.0
        stats, nv = self._stats, self.part.nv
        q = self._tq.data_ptr()
        st = ng.scc_step_desc(q, q, nv, ng.SCC_M_TTAIL, 2 * self.hubcap,
                              ng.SCC_TRIM)
        ng.scc_count(_stream(), self._args, st, self._hublist, self.hubcap)
        m = self._read_meta(2 if self.hubcap else 1)
        rounds, tail, _ = self._drain(st, self._thead, m[ng.SCC_M_TTAIL], 0,
                                      m[ng.SCC_M_HUBTAIL])
        stats["trim_rounds"] += rounds
        stats["trimmed"] += tail - self._thead
        self.events.append(("trim", rounds, tail - self._thead))
        self._alive -= tail - self._thead
        self._thead = tail
        if self.timed:
            self.phase_ms["trim"] += 1000.0 * (self._now() - t0)

    def _reach(self, dir, bit, cmode, head, hubhead, m):
        """One masked traversal whose seeds are rq[head : m's cursor)."""
        from . import _native_gpu as ng
        q = self._rq.data_ptr()
        st = ng.scc_step_desc(q, q, 2 * self.part.nv, ng.SCC_M_RTAIL,
                              2 * self.hubcap, ng.SCC_REACH, dir=dir,
                              cmode=cmode, bit=bit)
        steps, tail, hubtail = self._drain(st, head, m[ng.SCC_M_RTAIL],
                                           hubhead, m[ng.SCC_M_HUBTAIL])
        self._stats["reach_rounds"] += steps
        return tail, hubtail

    def _fwbw(self):
        from . import _native_gpu as ng
        t0 = self._now() if self.timed else 0.0
        s, stats = _stream(), self._stats
        ng.scc_pivot(s, self._args)
        pivot = self._read_meta(2)[ng.SCC_M_PIVOT]
        if pivot >= self.part.nv:
            raise RuntimeError(f"SCC pivot: {self._alive} vertices alive "
                               f"after the trim but no positive product")
        stats["pivot"] = pivot
        q = self._rq.data_ptr()
        seed = ng.scc_step_desc(q, q, 2 * self.part.nv, ng.SCC_M_RTAIL,
                                2 * self.hubcap, ng.SCC_REACH, dir=0,
                                bit=ng.SCC_F)
        ng.scc_seed(s, self._args, seed, pivot, 1)
        tail, hubtail = self._reach(0, ng.SCC_F, 0, 0, 0, self._read_meta())
        # the backward list follows the forward one, in rq and in hubq
        seed.dir, seed.bit = 1, ng.SCC_B
        ng.scc_seed(s, self._args, seed, pivot, 0)
        self._reach(1, ng.SCC_B, 0, tail, hubtail, self._read_meta())
        ng.scc_commit(s, self._args, 0)
        m = self._read_meta(2)
        stats["fwbw"] = m[ng.SCC_M_DIED]
        self._alive -= m[ng.SCC_M_DIED]
        self.events.append(("fwbw", 1, m[ng.SCC_M_DIED]))
        if self.timed:
            self.phase_ms["fwbw"] += 1000.0 * (self._now() - t0)

    def _colour_round(self):
        from . import _native_gpu as ng
        t0 = self._now() if self.timed else 0.0
        s, stats, nv, H = _stream(), self._stats, self.part.nv, self.hubcap
        base = self._cq.data_ptr()

        def desc(p):
            """Read half p, write half 1 - p."""
            return ng.scc_step_desc(
                base + 4 * nv * p, base + 4 * nv * (1 - p), nv,
                ng.SCC_M_CTAIL, H, ng.SCC_COLOUR, hr0=H * p,
                hw0=H * (1 - p), step=self._cstep)

        ng.scc_scan(s, self._args, desc(1), 0)  # writes half 0
        m = self._read_meta()
        p, sweeps = 0, 0
        n, nh = m[ng.SCC_M_CTAIL], m[ng.SCC_M_HUBTAIL]
        while n:
            if n > nv or nh > H or sweeps > nv:
                raise RuntimeError(f"SCC colour step out of bounds: n={n} "
                                   f"nv={nv} hub items={nh} hubcap={H} "
                                   f"sweeps={sweeps}")
            self._cstep += 1
            stats["hub_items"] += nh
            if self.fuse and n <= self.fuse and nh == 0:
                ng.scc_tail(s, self._args, desc(p), 0, n, 0, self.fuse, 1)
                m = self._read_meta()
                k = m[ng.SCC_M_FUSED]
                if k < 1:
                    raise RuntimeError("SCC tail kernel did no colour step")
                stats["fused_steps"] += k
                self._cstep += k - 1
            else:
                ng.scc_step(s, self._args, desc(p), 0, n, 0, nh, 1)
                m = self._read_meta()
                k = 1
            sweeps += k
            p = (p + k) % 2
            n, nh = m[ng.SCC_M_CTAIL], m[ng.SCC_M_HUBTAIL]
        stats["colour_sweeps"] += sweeps

        q = self._rq.data_ptr()
        roots = ng.scc_step_desc(q, q, 2 * nv, ng.SCC_M_RTAIL, 2 * H,
                                 ng.SCC_REACH, dir=1, cmode=1, bit=ng.SCC_B)
        ng.scc_scan(s, self._args, roots, 1)
        self._reach(1, ng.SCC_B, 1, 0, 0, self._read_meta())
        ng.scc_commit(s, self._args, 1)
        died = self._read_meta()[ng.SCC_M_DIED]
        if not 1 <= died <= self._alive:
            raise RuntimeError(f"SCC colour round removed {died} of "
                               f"{self._alive} alive vertices")
        self._alive -= died
        stats["colour_rounds"] += 1
        self.events.append(("colour", stats["colour_rounds"], died))
        if self.timed:
            self.phase_ms["colour"] += 1000.0 * (self._now() - t0)

    def decompose(self):
        """Decompose the whole graph; returns the device labels, int32[nv]
        holding u32 bits."""
        nv = self.part.nv
        self._stats = self._fresh_stats()
        self.events = []
        for key in ("trim", "fwbw", "colour"):
            self.phase_ms[key] = 0.0
        self._label.fill_(-1)
        self._mark.zero_()
        self._stamp.zero_()
        self._meta.zero_()
        self._alive, self._thead, self._cstep = nv, 0, 0
        if nv:
            self._trim()
            if self._alive:
                self._fwbw()
                if self._alive:
                    self._trim()
            while self._alive:
                if self._stats["colour_rounds"] >= nv:
                    raise RuntimeError("SCC colouring does not terminate")
                self._colour_round()
                if self._alive:
                    self._trim()
        self._done = True
        return self._label[:nv]

    # -------- results --------
    def labels(self):
        """Device int32[nv] (u32 bits): the label per vertex. The stored
        array of the last decompose(); decomposed now if there is none."""
        if not self._done:
            self.decompose()
        return self._label[:self.part.nv]

    def _labels64(self):
        return self.labels().to(U64) & NONE

    def sizes(self):
        """Device i64[nv]: the component size at each root id, 0
        elsewhere."""
        return torch.bincount(self._labels64(), minlength=self.part.nv)

    def num_components(self):
        return int((self.sizes() > 0).sum().item())

    def largest(self):
        """(label, size) of the largest SCC, the lowest label on a tie."""
        if not self.part.nv:
            return None, 0
        sizes = self.sizes()
        label = int(torch.argmax(sizes).item())
        return label, int(sizes[label].item())

    def member_mask(self, label):
        """Device bool[nv]: the vertices of the SCC with this label."""
        return self._labels64() == int(label)

    @property
    def stats(self):
        return dict(max_in_degree=self.max_in_degree,
                    max_out_degree=self.max_out_degree, **self._stats)

    def check(self):
        """Device check oracle (scc_check_*_kernel): the violations of
        necessary conditions — label[v] < v or label[label[v]] != label[v];
        a vertex its root does not reach, or that does not reach its root,
        inside its own label class (two multi-source traversals from all
        roots, a plain one-lane-per-vertex sweep run to its fixpoint: every
        class is then strongly connected); an edge pair u -> v, v -> u
        between different labels. Necessary, not sufficient: maximality is
        not proved (a proper split of an SCC along a longer cycle passes),
        so exactness rests on the tests against the CPU oracle."""
        from . import _native_gpu as ng
        label = self.labels()
        nv, s = self.part.nv, _stream()
        n1 = max(nv, 1)
        fwd = torch.zeros(n1, dtype=U32, device=self.device)
        bwd = torch.zeros(n1, dtype=U32, device=self.device)
        changed = torch.zeros(1, dtype=U32, device=self.device)
        graph = (self.in_ptr, self.in_col, self.out_ptr, self.out_col)
        self._bad.zero_()
        ng.scc_check_vertex(s, nv, label, fwd, bwd, self._bad, 0)
        for _ in range(nv + 1):
            changed.zero_()
            ng.scc_check_sweep(s, nv, *graph, label, fwd, bwd, changed)
            if not int(changed.item()):
                break
        else:
            raise RuntimeError("SCC check sweep does not terminate")
        ng.scc_check_vertex(s, nv, label, fwd, bwd, self._bad, 1)
        ng.scc_check_pairs(s, nv, self.part.ep, *graph, label, self._bad)
        return int(self._bad.item())
