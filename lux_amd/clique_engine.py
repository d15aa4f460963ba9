"""Exact k-clique counting on one GPU, 3 <= k <= 8: the degree-oriented DAG
of tc_engine.orient + LDS bit-matrix kernels (src/gpu/clique.hip). No
reference equivalent.

Definition — the graph is the underlying simple undirected graph of the
input, exactly as for TCEngine: {u,v} is an edge iff u != v and at least one
of u->v, v->u occurs. For 3 <= k <= 8:
  total         = the number of k-subsets of pairwise adjacent vertices, an
                  exact u64;
  per_vertex[v] = the number of those that contain v, an exact u64 in the
                  caller's original vertex ids;
                  per_vertex.sum() == k * total;
  density       = total / C(nv, k), the share of the k-subsets that are
                  cliques.
For k = 3 total and per_vertex equal TCEngine's. k outside 3..8 is a
ValueError.

Method: a k-clique u < v1 < ... < v(k-1) (rank order) is counted once, at
its lowest vertex u, as a (k-1)-clique of the DAG induced on the out-row
A(u). That DAG is a bit matrix in LDS and the search is ANDs and popcounts
on its rows. The role of a row comes from its out-degree d: wave
(k-1 <= d <= 64, one wave per row), block (64 < d <= cap, one workgroup per
row, launched once per size class d <= 128 / 256 / 512 / 1024 with that
class's LDS), hub (d > cap: one item per arc (u, v), the matrix built on
A(u) & A(v); an arc with more than cap common members is a spill and is
counted by the listless search of the plain kernel). Rows with d < k - 1
hold no clique and give no item. Degree order bounds d by sqrt(2m), so the
hub role is the id order's and the test graphs'.

Env knobs: LUX_CLIQUE_CAP (block-role cap in set members, default 1024, a
multiple of 64 in 64..1024), LUX_CLIQUE_PLAIN=1 (count with the
one-lane-per-arc plain kernel).
"""
import os
import time
from math import comb

import torch

from .engine import GraphPart
from .tc_engine import ORDERS, U32, U64, _stream, orient

K_MIN, K_MAX = 3, 8
WAVE_MAX = 64                    # wave role: arcs per row at most
CAP_DEFAULT = 1024               # LUX_CLIQUE_CAP when unset
CAP_MAX = 1024                   # what the kernels accept (CQ_CAP_MAX)
CLASSES = (128, 256, 512, 1024)  # block role: size classes
ROLE_WAVE, ROLE_BLOCK, ROLE_HUB = range(3)


def block_classes(cap):
    """The block role's size classes under `cap`: the CLASSES below it, then
    cap itself."""
    return [c for c in CLASSES if c < cap] + [cap]


def build_items(optr, k, cap):
    """Work items of the oriented rows: a list of (name, role, class, items)
    with items i32 (u32 bits) [n, 2] = {row u, p}. wave and block rows give
    one item {u, 0}, longest rows first; a hub row gives one item per arc
    {u, p} that has at least k - 2 entries after it. Rows of out-degree
    < k - 1 give none."""
    dev = optr.device
    d = optr[1:] - optr[:-1]

    def rows_of(mask):
        rows = torch.nonzero(mask).flatten()
        rows = rows[torch.sort(d[rows], descending=True, stable=True).indices]
        return torch.stack([rows, torch.zeros_like(rows)], 1).to(
            U32).contiguous()

    out = [("wave", ROLE_WAVE, 0,
            rows_of((d >= k - 1) & (d <= WAVE_MAX)))]
    lo = WAVE_MAX
    for c in block_classes(cap):
        out.append((f"block{c}", ROLE_BLOCK, c,
                    rows_of((d >= k - 1) & (d > lo) & (d <= c))))
        lo = c
    rows = torch.nonzero(d > cap).flatten()
    cnt = d[rows]
    u = torch.repeat_interleave(rows, cnt)
    start = torch.cumsum(cnt, 0) - cnt
    p = torch.arange(u.numel(), dtype=U64, device=dev) - \
        torch.repeat_interleave(start, cnt)
    keep = d[u] - p - 1 >= k - 2
    out.append(("hub", ROLE_HUB, cap,
                torch.stack([u[keep], p[keep]], 1).to(U32).contiguous()))
    return out


class CliqueEngine:
    def __init__(self, part: GraphPart, k=4, order="degree"):
        if part.nparts != 1:
            raise ValueError(
                "CliqueEngine is single-rank: an intersection needs both "
                f"rows on one device (got a GraphPart with "
                f"nparts={part.nparts})")
        if order not in ORDERS:
            raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
        if not K_MIN <= int(k) <= K_MAX:
            raise ValueError(f"k must be in {K_MIN}..{K_MAX}, got {k}")
        cap = int(os.environ.get("LUX_CLIQUE_CAP", CAP_DEFAULT))
        if not WAVE_MAX <= cap <= CAP_MAX or cap % 64:
            raise ValueError(f"LUX_CLIQUE_CAP={cap} is not a multiple of 64 "
                             f"in [{WAVE_MAX}, {CAP_MAX}]")
        from . import _native_gpu as ng
        if CAP_MAX > ng.clique_const("cap_max") or \
                K_MAX > ng.clique_const("k_max") or \
                WAVE_MAX != ng.clique_const("wave_max"):
            raise ValueError("CAP_MAX / K_MAX / WAVE_MAX beyond what "
                             "clique.hip takes")
        self.part = part
        self.device = part.device
        self.k = int(k)
        self.order = order
        self.cap = cap
        self.plain = os.environ.get("LUX_CLIQUE_PLAIN", "0") == "1"
        self.timed = False  # synchronise and clock count() (the app)
        self.phase_ms = dict(orient=0.0, items=0.0, count=0.0)
        nv = part.nv

        t0 = self._now()
        self.dag = orient(part.row_ptr, part.col, nv, order)
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)
        t0 = self._now()
        self.items = build_items(self.dag.optr, self.k, cap)
        self.phase_ms["items"] = 1000.0 * (self._now() - t0)

        d = self.dag.optr[1:] - self.dag.optr[:-1]
        self.max_out_degree = int(d.max().item()) if nv else 0
        self._acc = torch.zeros(4, dtype=U64, device=self.device)
        self._pv_rank = torch.zeros(max(nv, 1), dtype=U64,
                                    device=self.device)
        self._total = None
        self._counters = (0, 0, 0)  # set_ops, spills, built_bits
        self._pv = None
        self._other = None  # the other order's DAG, built by check()

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    # -------- counting --------
    def _launch(self, acc, pv):
        from . import _native_gpu as ng
        s, dag = _stream(), self.dag
        if self.plain:
            ng.clique_count_plain(s, self.k, self.part.nv, dag.m, dag.optr,
                                  dag.oadj, acc, pv)
            return
        for _, role, cls, it in self.items:
            ng.clique_count_items(s, role, self.k, dag.optr, dag.oadj, it,
                                  it.shape[0], cls, acc, pv)

    def count(self, per_vertex=False):
        """The total, recounted from zeroed accumulators; per_vertex=True
        also refreshes per_vertex()."""
        self._acc.zero_()
        pv = None
        if per_vertex:
            self._pv_rank.zero_()
            pv = self._pv_rank
        t0 = self._now() if self.timed else 0.0
        self._launch(self._acc, pv)
        acc = self._acc.cpu()  # the count's one host read
        if self.timed:
            self.phase_ms["count"] = 1000.0 * (time.perf_counter() - t0)
        self._total = int(acc[0])
        self._counters = (int(acc[1]), int(acc[2]), int(acc[3]))
        if per_vertex:
            self._pv = self._pv_rank[:self.part.nv][self.dag.rank]
        return self._total

    def per_vertex(self):
        """Device u64[nv] (torch.int64 bits): k-cliques containing each
        vertex, in original ids. The stored array of the last
        count(per_vertex=True); counted now if there is none."""
        if self._pv is None:
            self.count(per_vertex=True)
        return self._pv

    def density(self):
        """total / C(nv, k); 0.0 when nv < k."""
        if self._total is None:
            self.count()
        subsets = comb(self.part.nv, self.k)
        return self._total / subsets if subsets else 0.0

    @property
    def stats(self):
        st = dict(simple_edges=self.dag.m,
                  max_out_degree=self.max_out_degree)
        for name, _, _, it in self.items:
            st[f"items_{name}"] = int(it.shape[0])
        st["items_block"] = sum(int(it.shape[0]) for _, role, _, it
                                in self.items if role == ROLE_BLOCK)
        st["set_ops"], st["spills"], st["built_bits"] = self._counters
        return st

    def check(self):
        """Device check oracle: recount with the plain kernel on the OTHER
        orientation order and compare with the stored total and per-vertex
        array. Returns the number of mismatches: 1 if the totals differ,
        plus the vertices whose counts differ, plus 1 if per_vertex.sum()
        != k * total."""
        from . import _native_gpu as ng
        if self._pv is None or self._total is None:
            self.count(per_vertex=True)
        p = self.part
        if self._other is None:
            other = ORDERS[1 - ORDERS.index(self.order)]
            self._other = orient(p.row_ptr, p.col, p.nv, other)
        o = self._other
        acc = torch.zeros(4, dtype=U64, device=self.device)
        pv = torch.zeros(max(p.nv, 1), dtype=U64, device=self.device)
        ng.clique_count_plain(_stream(), self.k, p.nv, o.m, o.optr, o.oadj,
                              acc, pv)
        want_total = int(acc[0].item())
        want_pv = pv[:p.nv][o.rank]
        bad = int(want_total != self._total)
        bad += int((want_pv != self._pv).sum().item())
        bad += int(int(self._pv.sum().item()) != self.k * self._total)
        return bad
