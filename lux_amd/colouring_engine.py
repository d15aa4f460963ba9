"""Greedy vertex colouring and the maximal independent set that comes with
it, on one GPU: Jones-Plassmann rounds with device-side queues
(src/gpu/colouring.hip). No reference equivalent.

Definition — the same graph as TCEngine and KCoreEngine: the underlying
simple undirected graph of whatever the project loads ({u,v} is an edge iff
u != v and u->v or v->u occurs), deg its degree, everything in the caller's
vertex ids. A strict total order "v precedes u" is selected by `order`:
  degree (default)  deg[v] > deg[u], or equal and v < u (largest degree
                    first, Welsh-Powell);
  id                v < u (natural first-fit);
  hash              h(v) < h(u), or equal and v < u, with
                    h(v) = splitmix64(seed ^ v) >> 1 (lux::splitmix64).
pred(v) = the neighbours that precede v, succ(v) the others.
  colour[v] = mex{colour[u] : u in pred(v)}: the sequential greedy colouring
              in priority order, so 0 <= colour[v] <= |pred(v)|, no edge is
              monochromatic, and every c < colour[v] is the colour of a
              predecessor;
  MIS       = the class colour == 0, the lexicographically first maximal
              independent set in priority order (an isolated vertex is in);
  round[v]  = 1 + max(round[u] : u in pred(v)), 1 for an empty pred(v);
              rounds = the vertices on the longest priority-descending path.
The result does not depend on the schedule.

Preparation (timed as phase_ms["orient"] and phase_ms["split"]):
tc_engine.orient(..., "id") gives the simple graph as the DAG lo -> hi in the
caller's ids; the rank (torch: a stable sort of the degrees or of the hash
keys) decides for every arc which end is the predecessor, and the split
kernels write the predecessor rows pptr / padj (read for colours) and the
successor rows sptr / sadj (walked to notify), m entries each.

solve() colours round by round: the vertices whose predecessors are all
coloured take their mex (an LDS bitmap per wave, per workgroup for a
predecessor row longer than LUX_GCOL_HUB) and decrement `pending` of their
successors; the decrement that reaches zero queues the successor for the
next round. Queues and counters live in the kernels; the host keeps four
cursors, launches one kernel per round and reads the meta record back once
per launch. Small rounds (at most LUX_GCOL_FUSE entries, no hub item) are
run by a single-workgroup kernel that loops over them, so a cascade costs
one launch. The schedule is tests/colouring_ref.sync_jp's, round for round.
Every host tensor is one-dimensional, and none that scales with m is written
through a mask or an index.

Env knobs: LUX_GCOL_HUB (rows longer than this are handled by workgroups,
successor rows in chunks of this many entries; default the kernels'
GCOL_HUB), LUX_GCOL_FUSE (largest round the single-workgroup kernel takes,
0 = off: one launch and one host read per round; default the kernels'
GCOL_FUSE).
"""
import os
import time

import torch

from .engine import GraphPart
from .tc_engine import orient

U32, U64 = torch.int32, torch.int64
NONE = 0xFFFFFFFF
HUB_MAX = 1 << 20
ORDERS = ("degree", "id", "hash")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i64(u):
    """The i64 with the bits of the u64 u."""
    u &= (1 << 64) - 1
    return u - (1 << 64) if u >> 63 else u


def _lsr(x, k):
    """Logical shift right of an i64 tensor."""
    return (x >> k) & ((1 << (64 - k)) - 1)


def hash_keys(nv, seed, device):
    """h(v) = splitmix64(seed ^ v) >> 1 for v in [0, nv), i64[nv]
    (wrap-around i64 arithmetic for lux::splitmix64; the shift keeps the key
    non-negative)."""
    x = torch.arange(nv, dtype=U64, device=device) ^ _i64(seed)
    x = x + _i64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return _lsr(x ^ _lsr(x, 31), 1)


def priority_rank(deg, order, seed=1):
    """rank i64[nv] of the priority order: rank[v] < rank[u] iff v precedes
    u. deg: the simple degrees, i64[nv]."""
    nv = deg.numel()
    ids = torch.arange(nv, dtype=U64, device=deg.device)
    if order == "id":
        return ids
    if order == "degree":
        perm = torch.sort(deg, descending=True, stable=True).indices
    elif order == "hash":
        perm = torch.sort(hash_keys(nv, seed, deg.device),
                          stable=True).indices
    else:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    rank = torch.empty_like(perm)
    rank[perm] = ids
    return rank


class ColouringEngine:
    def __init__(self, part: GraphPart, order="degree", seed=1):
        if part.nparts != 1:
            raise ValueError(
                "ColouringEngine is single-rank: a round notifies "
                "successors on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        if order not in ORDERS:
            raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_GCOL_HUB", ng.gcol_hub_default()))
        if not 1 <= hub <= HUB_MAX:
            raise ValueError(f"LUX_GCOL_HUB={hub} outside [1, {HUB_MAX}]")
        fuse = int(os.environ.get("LUX_GCOL_FUSE", ng.gcol_fuse_default()))
        if not 0 <= fuse <= ng.gcol_fuse_max():
            raise ValueError(f"LUX_GCOL_FUSE={fuse} outside "
                             f"[0, {ng.gcol_fuse_max()}]")
        self.part = part
        self.device = part.device
        self.order, self.seed = order, int(seed)
        self.hub, self.fuse = hub, fuse
        self.timed = False  # synchronise and clock solve() (the app)
        self.phase_ms = dict(orient=0.0, split=0.0, solve=0.0)
        nv = part.nv
        n1 = max(nv, 1)
        dev = self.device

        t0 = self._now()
        dag = orient(part.row_ptr, part.col, nv, "id")
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)

        t0 = self._now()
        self.m = dag.m
        self.degree = dag.deg
        rank = priority_rank(dag.deg, order, self.seed).to(U32)
        self.npred = torch.zeros(n1, dtype=U32, device=dev)
        self.nsucc = torch.zeros(n1, dtype=U32, device=dev)
        s = _stream()
        ng.gcol_split_count(s, nv, dag.m, dag.optr, dag.oadj, rank,
                            self.npred, self.nsucc)
        self.pptr = torch.zeros(nv + 1, dtype=U64, device=dev)
        self.pptr[1:] = torch.cumsum(self.npred[:nv], 0, dtype=U64)
        self.sptr = torch.zeros(nv + 1, dtype=U64, device=dev)
        self.sptr[1:] = torch.cumsum(self.nsucc[:nv], 0, dtype=U64)
        self.padj = torch.empty(max(dag.m, 1), dtype=U32, device=dev)
        self.sadj = torch.empty(max(dag.m, 1), dtype=U32, device=dev)
        pcur = torch.zeros(n1, dtype=U32, device=dev)
        scur = torch.zeros(n1, dtype=U32, device=dev)
        ng.gcol_split_fill(s, nv, dag.m, dag.optr, dag.oadj, rank, self.pptr,
                           self.sptr, pcur, scur, self.padj, self.sadj)
        self.max_degree = int(dag.deg.max().item()) if nv else 0
        self.max_pred = int(self.npred.max().item()) if nv else 0
        # hubq: one select item per long predecessor row, ceil(d / hub)
        # chunk items per long successor row
        self.hub_selects = int((self.npred[:nv] > hub).sum().item())
        big = self.nsucc[:nv][self.nsucc[:nv] > hub].to(U64)
        self.hub_chunks = int(((big + (hub - 1)) // hub).sum().item())
        self.hubcap = self.hub_selects + self.hub_chunks
        del dag, rank, pcur, scur, big
        self.phase_ms["split"] = 1000.0 * (self._now() - t0)

        self._colour = torch.empty(n1, dtype=U32, device=dev)
        self._pending = torch.empty(n1, dtype=U32, device=dev)
        self._order = torch.empty(n1, dtype=U32, device=dev)
        self._rtail = torch.zeros(n1, dtype=U32, device=dev)
        self._hubq = torch.empty(2 * max(self.hubcap, 1), dtype=U32,
                                 device=dev)
        self._meta = torch.zeros(ng.gcol_meta_words(), dtype=U32, device=dev)
        self._bad = torch.zeros(1, dtype=U64, device=dev)
        self._args = ng.gcol_args(
            self.pptr, self.padj, self.sptr, self.sadj, self._colour,
            self._pending, self._order, self._hubq, self._rtail, self._meta,
            nv, self.hubcap, hub)
        self._done = False
        self._stats = dict(rounds=0, fused_rounds=0, launches=0,
                           host_reads=0, hub_items=0)
        self._tails = []  # the order cursor after each round; None: in rtail
        self._trace = None

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    # -------- the rounds --------
    def _read_meta(self):
        """The blocking read of the meta record (u32 values)."""
        self._stats["host_reads"] += 1
        return [x & NONE for x in self._meta.tolist()]

    def solve(self):
        """Colour the whole graph; returns the device colours, i32[nv]."""
        from . import _native_gpu as ng
        nv = self.part.nv
        st = self._stats = dict(rounds=0, fused_rounds=0, launches=0,
                                host_reads=0, hub_items=0)
        self._tails, self._trace = [], None
        self._done = False
        t0 = self._now() if self.timed else 0.0
        self._colour.fill_(-1)
        self._pending.copy_(self.npred)
        self._meta.zero_()
        s, a = _stream(), self._args

        def bounded(head, tail, hubtail):
            if not head <= tail <= nv or hubtail > self.hubcap or \
                    st["rounds"] > nv:
                raise RuntimeError(
                    f"colouring out of bounds: head={head} tail={tail} "
                    f"nv={nv} hubtail={hubtail} hubcap={self.hubcap} "
                    f"rounds={st['rounds']}")

        head = tail = hubhead = hubtail = 0
        if nv:
            ng.gcol_seed(s, a)
            st["launches"] += 1
            m = self._read_meta()
            tail, hubtail = m[ng.GCOL_M_TAIL], m[ng.GCOL_M_HUBTAIL]
            bounded(head, tail, hubtail)
        while head < tail:
            if self.fuse and tail - head <= self.fuse and \
                    hubtail == hubhead:
                ng.gcol_tail(s, a, head, tail, hubtail, self.fuse,
                             st["rounds"])
                m = self._read_meta()
                k = m[ng.GCOL_M_FUSED]
                if k < 1 or m[ng.GCOL_M_HEAD] < tail:
                    raise RuntimeError(
                        f"colouring tail kernel made no progress: fused={k} "
                        f"head={m[ng.GCOL_M_HEAD]} after [{head}, {tail})")
                st["rounds"] += k
                st["fused_rounds"] += k
                self._tails += [tail] + [None] * (k - 1)
                head = m[ng.GCOL_M_HEAD]
            else:
                ng.gcol_step(s, a, head, tail, hubhead, hubtail)
                m = self._read_meta()
                st["rounds"] += 1
                self._tails.append(tail)
                head, hubhead = tail, hubtail
            st["launches"] += 1
            tail, hubtail = m[ng.GCOL_M_TAIL], m[ng.GCOL_M_HUBTAIL]
            bounded(head, tail, hubtail)
        if tail != nv:
            raise RuntimeError(f"colouring stopped at {tail} of {nv} "
                               f"vertices after {st['rounds']} rounds")
        st["hub_items"] = hubtail
        if self.timed:
            self.phase_ms["solve"] = 1000.0 * (self._now() - t0)
        self._done = True
        return self._colour[:nv]

    def colours(self):
        """Device i32[nv]: the colour per vertex, original ids. The stored
        array of the last solve(); solved now if there is none."""
        if not self._done:
            self.solve()
        return self._colour[:self.part.nv]

    def num_colours(self):
        return int(self.colours().max().item()) + 1 if self.part.nv else 0

    def class_sizes(self):
        """Device i64[num_colours]: the vertices of each colour."""
        return torch.bincount(self.colours().to(U64))

    def independent_set(self):
        """Device bool[nv]: the class colour == 0, the lexicographically
        first maximal independent set in priority order."""
        return self.colours() == 0

    def rounds(self):
        self.colours()
        return self._stats["rounds"]

    @property
    def round_trace(self):
        """[(round, coloured)] per round, rounds counted from 1. The sizes
        of the rounds the tail kernel fused come from the device in one read
        at the first access; it is not one of the solve's host reads."""
        self.colours()
        if self._trace is None:
            tails = list(self._tails)
            if any(t is None for t in tails):
                dev = [x & NONE for x in self._rtail[:len(tails)].tolist()]
                tails = [d if t is None else t for t, d in zip(tails, dev)]
            self._trace = [(r + 1, t - (tails[r - 1] if r else 0))
                           for r, t in enumerate(tails)]
        return self._trace

    @property
    def stats(self):
        return dict(simple_edges=self.m, max_degree=self.max_degree,
                    max_pred=self.max_pred, hub_selects=self.hub_selects,
                    hub_chunks=self.hub_chunks, **self._stats)

    def check(self):
        """Device check oracle (gcol_check_kernel): the vertices v that
        break a necessary condition over their full neighbourhood —
        colour[v] outside [0, |pred(v)|], a neighbour of the same colour,
        colour[v] = c > 0 without a predecessor of colour c - 1, or
        colour[v] > 0 without a predecessor of colour 0 (class 0 is not
        maximal). Necessary, not sufficient (a gap below c - 1 passes):
        exactness rests on the tests against the CPU oracle."""
        from . import _native_gpu as ng
        col = self.colours()
        self._bad.zero_()
        ng.gcol_check(_stream(), self.part.nv, self.pptr, self.padj,
                      self.sptr, self.sadj, col, self._bad)
        return int(self._bad.item())
