"""Community detection on one GPU by modularity optimisation: the Louvain
method, one colour class at a time, with decide / apply kernels and a
contraction per level (src/gpu/louvain.hip). No reference equivalent.

Definition (API.md, "Louvain") — the graph of KCoreEngine and LPAEngine, the
underlying simple undirected graph; with weighted=True the weight of {u, v}
is the sum of part.weight over all occurrences of u->v and v->u, else 1. A
level graph has n vertices, a symmetric adjacency with u32 weights, self[v]
(twice the weight contracted inside v) and k[v] = self[v] + the row's weights;
W = sum k is the same at every level and must be below 2^32. A level starts
from comm[v] = v (level 0: init[v] if given), tot[c] = the sum of k over c.
A sweep visits the classes of the level's greedy colouring in order; every
member with a neighbour decides on comm and tot as they stand when its class
starts (score(c) = a(c) * W - k[v] * (tot[c] - [c == comm[v]] k[v]), the
largest score, the smallest c among equals, a move only on a strictly larger
score than staying), then the movers are applied. After each sweep Qnum =
W * in - sum tot^2 = modularity * W^2 is formed from two exact u64 sums. A
level ends at a sweep without a mover, at a sweep whose Qnum does not exceed
the best so far (that sweep is undone; the level starts at the Qnum of its
initial state), or after max_sweeps sweeps. The communities in use become the
vertices of the next level in ascending id order. The solve ends at a level
that keeps no move (level 0 under an init is contracted all the same), or
after max_levels levels; the label of an original
vertex is its vertex in the last level graph. Every value is an integer:
the result does not depend on the schedule and equals cpu_ref.louvain.

Preparation (phase_ms["orient"], ["adjacency"]): tc_engine.orient gives the
simple edges (weighted: the arcs themselves, both ways, self-loops dropped);
sorted records (row << 32 | column, w) go through the contraction's heads and
run-reduce kernels, which sum equal keys into the rows aptr / aadj / aw and
k. Per solve: ["colour"] a ColouringEngine per level (level 0 on the part,
coarse levels on a DeviceCSC of the coarse rows), ["plan"] the class order,
hub items and launch plan as LPAEngine builds them, ["move"] the sweeps,
["aggregate"] relabel kernel, torch.sort, heads and run-reduce kernels.

Env knobs, validated like the LPA ones: LUX_LOUVAIN_HUB (rows longer than
this go through hub items; never above LUX_LOUVAIN_TABLE / 8), LUX_LOUVAIN_
TABLE (slots of the LDS table, a power of two), LUX_LOUVAIN_FUSE (vertices of
a fused launch, 0 = off).
"""
import os
import time
from fractions import Fraction
from types import SimpleNamespace

import torch

from .colouring_engine import ORDERS, ColouringEngine
from .engine import DeviceCSC, GraphPart
from .tc_engine import orient

U32, U64 = torch.int32, torch.int64
MASK32 = 0xFFFFFFFF
SENT = 0x7FFFFFFFFFFFFFFF  # a record to drop (louvain.hip LV_SENT)
HUB_MIN, HUB_MAX = 64, 1 << 20


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _u(t):
    """i64 values of a tensor holding u32 bits."""
    return t.to(U64) & MASK32


class LouvainEngine:
    def __init__(self, part: GraphPart, order="degree", seed=1,
                 weighted=False):
        if part.nparts != 1:
            raise ValueError(
                "LouvainEngine is single-rank: a class reads its "
                "neighbours' communities on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        if order not in ORDERS:
            raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_LOUVAIN_HUB",
                                 ng.louvain_const("hub_default")))
        if not HUB_MIN <= hub <= HUB_MAX:
            raise ValueError(f"LUX_LOUVAIN_HUB={hub} outside "
                             f"[{HUB_MIN}, {HUB_MAX}]")
        table = int(os.environ.get("LUX_LOUVAIN_TABLE",
                                   ng.louvain_const("table_default")))
        tmin, tmax = ng.louvain_const("table_min"), \
            ng.louvain_const("table_max")
        if not tmin <= table <= tmax or table & (table - 1):
            raise ValueError(f"LUX_LOUVAIN_TABLE={table} is not a power of "
                             f"two in [{tmin}, {tmax}]")
        fuse = int(os.environ.get("LUX_LOUVAIN_FUSE",
                                  ng.louvain_const("fuse_default")))
        if not 0 <= fuse <= ng.louvain_const("fuse_max"):
            raise ValueError(f"LUX_LOUVAIN_FUSE={fuse} outside "
                             f"[0, {ng.louvain_const('fuse_max')}]")
        if weighted and part.weight is None:
            raise ValueError("weighted=True needs part.weight")
        self.part, self.device = part, part.device
        self.order, self.seed, self.weighted = order, int(seed), weighted
        self.hub, self.table, self.fuse = \
            ng.louvain_row_limit(hub, table), table, fuse
        self.timed = False  # synchronise and clock solve() (the app)
        self.phase_ms = dict(orient=0.0, adjacency=0.0, colour=0.0, plan=0.0,
                             move=0.0, aggregate=0.0)
        nv, dev = part.nv, self.device

        t0 = self._now()
        if weighted:
            ne = part.ne
            w = part.weight[:ne]
            if ne and int(w.min().item()) < 1:
                raise ValueError("every weight must be >= 1 "
                                 f"(got {int(w.min().item())})")
            e = torch.arange(ne, dtype=U64, device=dev)
            dst = torch.searchsorted(part.row_ptr[:nv + 1], e, right=True) - 1
            src = _u(part.col[:ne])
            loop = src == dst
            sent = torch.full_like(src, SENT)
            keys = torch.cat([torch.where(loop, sent, (dst << 32) | src),
                              torch.where(loop, sent, (src << 32) | dst)])
            w = torch.where(loop, torch.zeros_like(w), w)
            wrec = torch.cat([w, w])
            self.m = None
            del e, dst, src, loop, sent, w
        else:
            dag = orient(part.row_ptr, part.col, nv, "id")
            lo = torch.repeat_interleave(
                torch.arange(nv, dtype=U64, device=dev),
                dag.optr[1:] - dag.optr[:-1])
            hi = _u(dag.oadj)
            keys = torch.cat([(lo << 32) | hi, (hi << 32) | lo])
            wrec = torch.ones(keys.numel(), dtype=U32, device=dev)
            self.m = dag.m
            del dag, lo, hi
        self.W = int(wrec.to(U64).sum().item())
        if self.W >= 1 << 32:
            raise ValueError(f"W = {self.W} (twice the total edge weight) "
                             "does not fit 32 bits")
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)

        t0 = self._now()
        keys, perm = torch.sort(keys)
        self._g0 = self._build_rows(
            keys, wrec[perm], nv, torch.zeros(max(nv, 1), dtype=U32,
                                              device=dev))
        if self.m is None:
            self.m = self._g0.entries // 2
        self.max_degree = int((self._g0.aptr[1:] - self._g0.aptr[:-1])
                              .max().item()) if nv else 0
        del keys, perm, wrec
        self.phase_ms["adjacency"] = 1000.0 * (self._now() - t0)
        self._lv0 = None  # level 0 with its classes and plan, at first solve
        self._last = None
        self._done = self._cut = False
        self._labels = None
        self._level_trace, self._sweep_trace = [], []
        self._st = dict(launches=0, hub_rows=0, hub_items=0, fused_classes=0,
                        host_reads=0, colours=0)

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    def _tick(self):
        return self._now() if self.timed else 0.0

    # -------- level graphs --------
    def _build_rows(self, keys, wrec, n, selfw):
        """The level graph of n vertices from records sorted by key (row <<
        32 | column; SENT sorts last and is dropped): equal keys are summed
        (louvain.hip heads and run-reduce kernels). One host read."""
        from . import _native_gpu as ng
        dev, n1, s = self.device, max(n, 1), _stream()
        nrec = int(keys.numel())
        head = torch.empty(max(nrec, 1), dtype=U64, device=dev)
        deg = torch.zeros(n1, dtype=U32, device=dev)
        ng.louvain_heads(s, nrec, keys, n, head, deg)
        pos = torch.cumsum(head[:nrec], 0)
        entries = int(pos[-1].item()) if nrec else 0
        aptr = torch.zeros(n + 1, dtype=U64, device=dev)
        aptr[1:] = torch.cumsum(_u(deg[:n]), 0)
        aadj = torch.zeros(max(entries, 1), dtype=U32, device=dev)
        aw = torch.zeros(max(entries, 1), dtype=U32, device=dev)
        k = selfw.clone()
        ng.louvain_reduce(s, nrec, keys, wrec, pos, entries, n, aadj, aw, k)
        return SimpleNamespace(n=n, entries=entries, aptr=aptr, aadj=aadj,
                               aw=aw, k=k, selfw=selfw)

    def _prepare(self, g, part):
        """Colour level graph g (through `part`), order its classes, list the
        hub items and plan the launches; allocates the level's state."""
        from . import _native_gpu as ng
        dev, n, n1 = self.device, g.n, max(g.n, 1)
        t0 = self._tick()
        if g.entries:
            ce = ColouringEngine(part, order=self.order, seed=self.seed)
            colour = ce.colours().to(U64).clone()
            C = ce.num_colours()
            del ce
        else:
            colour, C = torch.zeros(n, dtype=U64, device=dev), 1
        self.phase_ms["colour"] += 1000.0 * (self._tick() - t0)

        t0 = self._tick()
        table, half = self.table, self.table // 2
        g.vorder = torch.sort(colour, stable=True).indices.to(U32)
        count = torch.bincount(colour, minlength=C)
        cptr = torch.zeros(C + 1, dtype=U64, device=dev)
        cptr[1:] = torch.cumsum(count, 0)
        deg64 = g.aptr[1:] - g.aptr[:-1]
        cmax = torch.zeros(C, dtype=U64, device=dev)
        cmax.scatter_reduce_(0, colour, deg64, "amax")
        vo = g.vorder.to(U64)
        dv = deg64[vo]
        is_hub = dv > self.hub
        hv, hd = vo[is_hub], dv[is_hub]
        passes = (hd + (half - 1)) // half
        g.hub_rows = int(hv.numel())
        g.hub_items = int(passes.sum().item())
        hubr = torch.repeat_interleave(
            torch.arange(g.hub_rows, dtype=U64, device=dev), passes)
        first = torch.cumsum(passes, 0) - passes
        hubp = torch.arange(g.hub_items, dtype=U64, device=dev) - \
            torch.repeat_interleave(first, passes)
        per_class = torch.zeros(C, dtype=U64, device=dev)
        per_class.index_add_(0, colour[hv], passes)
        hptr = torch.zeros(C + 1, dtype=U64, device=dev)
        hptr[1:] = torch.cumsum(per_class, 0)
        g.cptr, g.hptr = cptr.to(U32), hptr.to(U32)
        g.hubv = torch.repeat_interleave(hv, passes).to(U32)
        g.hubp, g.hubr = hubp.to(U32), hubr.to(U32)
        if not g.hub_items:  # never read; the pointers stay valid
            g.hubv = torch.zeros(1, dtype=U32, device=dev)
            g.hubp, g.hubr = g.hubv.clone(), g.hubv.clone()
        g.colours = C
        g.plan, g.fused_classes = self._make_plan(
            count.tolist(), per_class.tolist(), cmax.tolist())
        g.comm = torch.empty(n1, dtype=U32, device=dev)
        g.next = torch.empty(n1, dtype=U32, device=dev)
        g.tot = torch.zeros(n1, dtype=U64, device=dev)
        g.hubbest = torch.zeros(3 * max(g.hub_items, 1), dtype=U64,
                                device=dev)
        g.hubdone = torch.zeros(max(g.hub_rows, 1), dtype=U32, device=dev)
        g.meta = torch.zeros(ng.louvain_const("meta_words"), dtype=U64,
                             device=dev)
        g.args = ng.louvain_args(
            g.aptr, g.aadj, g.aw, g.k, g.selfw, g.vorder, g.cptr, g.comm,
            g.tot, g.next, g.hubv, g.hubp, g.hubr, g.hptr, g.hubbest,
            g.hubdone, g.meta, self.W, n, C, g.hub_items, g.hub_rows,
            self.hub, table)
        self.phase_ms["plan"] += 1000.0 * (self._tick() - t0)
        return g

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

    def _set_communities(self, g, comm):
        """comm (i64[n]) becomes the level's state; tot follows from k."""
        g.comm[:g.n] = comm.to(U32)
        g.next.copy_(g.comm)
        g.tot.zero_()
        g.tot.index_add_(0, comm, _u(g.k[:g.n]))

    def _qnum(self, g):
        """(movers, Qnum) of the level as it stands: the statistics kernel
        and the one host read of a sweep."""
        from . import _native_gpu as ng
        ng.louvain_stats(_stream(), g.args)
        meta = [x % (1 << 64) for x in g.meta.tolist()]
        self._st["host_reads"] += 1
        return meta[ng.LOUVAIN_M_MOVED], \
            self.W * meta[ng.LOUVAIN_M_IN] - meta[ng.LOUVAIN_M_SQ]

    def _contract(self, g, dense, n2):
        """The next level graph: relabel kernel, a sort of the records, the
        heads and run-reduce kernels."""
        from . import _native_gpu as ng
        dev = self.device
        keys = torch.empty(max(g.entries, 1), dtype=U64, device=dev)
        wrec = torch.empty(max(g.entries, 1), dtype=U32, device=dev)
        self2 = torch.zeros(n2, dtype=U32, device=dev)
        ng.louvain_relabel(_stream(), g.args, dense, n2, keys, wrec, self2)
        keys, perm = torch.sort(keys[:g.entries])
        self._st["host_reads"] += 1
        return self._build_rows(keys, wrec[:g.entries][perm], n2, self2)

    # -------- the solve --------
    def solve(self, init=None, max_sweeps=0, max_levels=0):
        """Levels of sweeps and contractions until a level keeps no move (or
        max_levels levels, each of at most max_sweeps sweeps, 0 = no limit);
        returns the device labels, i32[nv], dense in [0, communities)."""
        from . import _native_gpu as ng
        nv, dev = self.part.nv, self.device
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
        self._done = self._cut = False
        self._level_trace, self._sweep_trace = [], []
        st = self._st = dict(launches=0, hub_rows=0, hub_items=0,
                             fused_classes=0, host_reads=0, colours=0)
        for name in ("colour", "plan", "move", "aggregate"):
            self.phase_ms[name] = 0.0
        if self._lv0 is None:
            self._lv0 = self._prepare(self._g0, self.part)
        g, s = self._lv0, _stream()
        st["colours"] = g.colours
        vmap = None  # original vertex -> level vertex; None: the identity
        while nv:
            level = len(self._level_trace)
            t0 = self._tick()
            for name in ("hub_rows", "hub_items", "fused_classes"):
                st[name] += getattr(g, name)
            ids = torch.arange(g.n, dtype=U64, device=dev)
            self._set_communities(
                g, ids if level or init is None else init.to(dev, U64))
            g.hubdone.zero_()
            g.meta.zero_()
            best = self._qnum(g)[1]
            sweeps = moved = 0
            while True:
                comm0, tot0 = g.comm.clone(), g.tot.clone()
                g.meta.zero_()
                for c0, c1, rows, items, maxdeg, fused in g.plan:
                    ng.louvain_classes(s, g.args, c0, c1, rows, items, maxdeg,
                                       fused)
                    st["launches"] += 1 if fused or not rows else 2
                movers, q = self._qnum(g)
                sweeps += 1
                self._sweep_trace.append((level, sweeps, movers, q))
                if movers > g.n or sweeps > self.W + 1:
                    raise RuntimeError(
                        f"louvain out of bounds: level {level} sweep "
                        f"{sweeps} moved {movers} of {g.n}")
                if movers == 0:
                    break
                if q <= best:
                    g.comm.copy_(comm0)
                    g.tot.copy_(tot0)
                    break
                best, moved = q, moved + movers
                if max_sweeps > 0 and sweeps >= max_sweeps:
                    break
            del comm0, tot0
            self._level_trace.append((level, g.n, sweeps, moved, best))
            self.phase_ms["move"] += 1000.0 * (self._tick() - t0)
            if moved == 0 and (level or init is None):
                break  # an init is contracted even if nothing moved
            t0 = self._tick()
            comm = _u(g.comm[:g.n])
            used = torch.zeros(g.n, dtype=U64, device=dev)
            used[comm] = 1
            dense = torch.cumsum(used, 0) - 1
            n2 = int(dense[-1].item()) + 1
            st["host_reads"] += 1
            lab = dense[comm]
            vmap = lab if vmap is None else lab[vmap]
            self._cut = max_levels > 0 and level + 1 >= max_levels
            if not self._cut:
                g2 = self._contract(g, dense.to(U32), n2)
            self.phase_ms["aggregate"] += 1000.0 * (self._tick() - t0)
            if self._cut:
                break
            csc = DeviceCSC(g2.n, g2.entries, g2.aptr[1:], g2.aadj)
            g = self._prepare(g2, GraphPart(csc, 1, 0, keep_full=True)
                              if g2.entries else None)
            del comm, used, dense, lab, csc, g2
        self._last = g
        self._labels = (torch.arange(nv, dtype=U64, device=dev)
                        if vmap is None else vmap).to(U32)
        self._done = True
        return self._labels

    def labels(self):
        """Device i32[nv]: per original vertex its vertex in the last level
        graph. The stored array of the last solve(); solved now if there is
        none."""
        if not self._done:
            self.solve()
        return self._labels

    def levels(self):
        self.labels()
        return len(self._level_trace)

    @property
    def level_trace(self):
        """[(level, n, sweeps, moved, Qnum)], levels counted from 0; moved
        and Qnum are those of the sweeps the level kept."""
        self.labels()
        return list(self._level_trace)

    @property
    def sweep_trace(self):
        """[(level, sweep, moved, Qnum)], sweeps counted from 1, an undone
        sweep included."""
        self.labels()
        return list(self._sweep_trace)

    def qnum(self):
        """modularity * W^2 of the labels, an exact integer."""
        self.labels()
        return self._level_trace[-1][4] if self._level_trace else 0

    def modularity(self):
        """Qnum / W^2 through exact integers; 0.0 for W == 0."""
        q = self.qnum()
        return float(Fraction(q, self.W * self.W)) if self.W else 0.0

    def num_communities(self):
        lab = self.labels()
        return int(lab.max().item()) + 1 if lab.numel() else 0

    def sizes(self):
        """Device i64[communities]: the original vertices per label."""
        return torch.bincount(self.labels().to(U64),
                              minlength=self.num_communities())

    def member_mask(self, label):
        """Device bool[nv]: the vertices of the community `label`."""
        return self.labels() == int(label)

    def level_communities(self):
        """Device i32[n]: the community per vertex of the last level graph
        as the solve left it (the identity after a solve that ran out), the
        array check() evaluates."""
        self.labels()
        return self._last.comm[:self._last.n]

    @property
    def stats(self):
        return dict(simple_edges=self.m, max_degree=self.max_degree, W=self.W,
                    levels=len(self._level_trace),
                    sweeps=len(self._sweep_trace), **self._st)

    def check(self):
        """Device check (the decide kernel in check mode over every class of
        the last level graph): the vertices that would still move, with tot
        formed anew from level_communities(). Zero is necessary for a solve
        that ran out, not sufficient for the right one: exactness rests on
        the tests against the CPU oracle. Raises after a solve cut short by
        max_levels."""
        from . import _native_gpu as ng
        self.labels()
        if self._cut:
            raise ValueError(
                f"check() after a solve cut short by max_levels "
                f"({len(self._level_trace)} levels)")
        g = self._last
        if not self.part.nv:
            return 0
        g.tot.zero_()
        g.tot.index_add_(0, _u(g.comm[:g.n]), _u(g.k[:g.n]))
        g.meta.zero_()
        ng.louvain_check(_stream(), g.args)
        return g.meta.tolist()[ng.LOUVAIN_M_BAD] % (1 << 64)
