"""Exact triangle counting on one GPU: degree-oriented DAG + sorted-list
intersection (src/gpu/tc.hip). No reference equivalent.

Definition — the input is any graph the project loads (directed CSC,
possibly with parallel edges and self-loops); the count runs on its
underlying simple undirected graph:
  {u,v} is an edge iff u != v and at least one of u->v, v->u occurs, so
  parallel edges collapse and self-loops vanish. This deliberately differs
  from BCEngine, where every occurrence of a parallel edge is a distinct
  path.
  total         = the number of unordered vertex triples that are pairwise
                  adjacent, an exact u64;
  per_vertex[v] = the number of triangles containing v, an exact u64 in the
                  caller's original vertex ids (a hub's count can pass 2^32);
                  per_vertex.sum() == 3 * total;
  transitivity  = 3 * total / sum_v C(deg(v), 2) with deg the simple
                  undirected degree; 0.0 when the denominator is 0;
  clustering[v] = per_vertex[v] / C(deg(v), 2), f64; 0.0 where deg(v) < 2.

Preparation (orient + build_items, torch ops only, one-off): vertices are
ranked — order="degree": ascending by (simple degree, id); order="id":
rank = id — and relabelled to their rank, and each undirected edge is kept
as the one arc lo -> hi. Rows of the resulting DAG are strictly ascending
and hold only ids above their own, so a triangle u < v < w is found exactly
once, as a w of A(v) that is also in A(u), at the arc (u, v). Rows are cut
into items of at most TC_CHUNK arcs, grouped by the role their out-degree
d selects: small (d < TC_T1), staged (TC_T1 <= d <= stage cap, the row in
LDS), hub (d > stage cap, searched in global memory). Degree order bounds d
by sqrt(2m), which makes the hub role rare; id order is the A/B and the
lever that lets a small test graph reach any d.

Env knobs: LUX_TC_STAGE (stage cap in LDS entries, default 4096, at most
8192), LUX_TC_PLAIN=1 (count with the one-lane-per-arc plain kernel),
LUX_TC_SORT_CHUNK (keys per sort of the orientation, default 2^28).
"""
import os
import time
from types import SimpleNamespace

import torch

from .engine import GraphPart

U32, U64 = torch.int32, torch.int64
MASK32 = 0xFFFFFFFF

TC_T1 = 32               # rows below this out-degree: small role (its
#                          kernel holds a row in 32 lanes: at most 33)
TC_CHUNK = 256           # arcs per work item
TC_STAGE_DEFAULT = 4096  # LUX_TC_STAGE when unset: 16 KiB of LDS
TC_STAGE_MAX = 8192      # what the kernels accept (tc.hip TC_STAGE_MAX)
SORT_CHUNK_DEFAULT = 1 << 28
ORDERS = ("degree", "id")
ROLES = ("small", "staged", "hub")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sorted_unique_keys(pairs, nv, chunk, device):
    """Sorted, duplicate-free i64 keys (min << 32) | max of the pairs (a, b)
    with a != b. `pairs` yields i64 tensor pairs of at most `chunk` entries;
    every torch.sort sees at most `chunk` keys, apart from a single row
    whose copies across the chunks exceed that."""
    parts = []
    for a, b in pairs:
        keep = a != b
        a, b = a[keep], b[keep]
        k = (torch.minimum(a, b) << 32) | torch.maximum(a, b)
        k = torch.unique_consecutive(torch.sort(k).values)
        if k.numel():
            parts.append(k)
    if not parts:
        return torch.empty(0, dtype=U64, device=device)
    if len(parts) == 1:
        return parts[0]
    # the chunks are sorted runs over the whole key space: cut it at row
    # boundaries so that a range gathers at most `chunk` keys from all
    # runs, then sort + unique each range
    cnt = torch.zeros(nv, dtype=U64, device=device)
    for k in parts:
        cnt += torch.bincount(k >> 32, minlength=nv)
    ends = torch.cumsum(cnt, 0)
    out = []
    r0, base = 0, 0
    while r0 < nv:
        r1 = int(torch.searchsorted(
            ends, torch.tensor([base + chunk], dtype=U64, device=device),
            right=True).item())
        r1 = min(max(r1, r0 + 1), nv)
        cut = torch.tensor([r0 << 32, r1 << 32], dtype=U64, device=device)
        runs = []
        for k in parts:
            i0, i1 = torch.searchsorted(k, cut).tolist()
            if i1 > i0:
                runs.append(k[i0:i1])
        if runs:
            out.append(torch.unique_consecutive(
                torch.sort(torch.cat(runs)).values))
        base = int(ends[r1 - 1].item())
        r0 = r1
    return torch.cat(out)


def orient(row_ptr, col, nv, order="degree", chunk=None):
    """CSC (row_ptr i64[nv+1], col u32 bits[ne]: row v lists the sources of
    its in-edges) -> the oriented DAG of the underlying simple graph.
    Returns a namespace with
      optr  i64[nv+1], oadj i32 (u32 bits)[m] — rank-space rows, strictly
            ascending, every entry > the row's own id;
      perm  i64[nv], perm[r] = original id of rank r; rank, its inverse;
      deg   i64[nv], the simple undirected degree per original id;
      m     the number of simple undirected edges.
    Torch ops only: runs on whatever device holds row_ptr and col."""
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if chunk is None:
        chunk = int(os.environ.get("LUX_TC_SORT_CHUNK", SORT_CHUNK_DEFAULT))
    chunk = max(int(chunk), 1)
    dev = row_ptr.device
    row_ptr = row_ptr[:nv + 1]
    ne = int(row_ptr[nv].item()) if nv else 0

    def csc_pairs():
        for e0 in range(0, ne, chunk):
            e1 = min(e0 + chunk, ne)
            e = torch.arange(e0, e1, dtype=U64, device=dev)
            dst = torch.searchsorted(row_ptr, e, right=True) - 1
            yield col[e0:e1].to(U64) & MASK32, dst

    keys = _sorted_unique_keys(csc_pairs(), nv, chunk, dev)
    a, b = keys >> 32, keys & MASK32
    m = int(keys.numel())
    deg = torch.bincount(a, minlength=nv) + torch.bincount(b, minlength=nv)
    ids = torch.arange(nv, dtype=U64, device=dev)
    if order == "degree":
        perm = torch.sort(deg, stable=True).indices  # ties: ascending id
        rank = torch.empty_like(perm)
        rank[perm] = ids

        def ranked_pairs():
            for i0 in range(0, m, chunk):
                yield rank[a[i0:i0 + chunk]], rank[b[i0:i0 + chunk]]

        keys = _sorted_unique_keys(ranked_pairs(), nv, chunk, dev)
    else:
        perm = rank = ids
    optr = torch.zeros(nv + 1, dtype=U64, device=dev)
    optr[1:] = torch.cumsum(torch.bincount(keys >> 32, minlength=nv), 0)
    oadj = (keys & MASK32).to(U32)
    return SimpleNamespace(optr=optr, oadj=oadj, perm=perm, rank=rank,
                           deg=deg, m=m, order=order)


def build_items(optr, stage_cap, t1=TC_T1, chunk=TC_CHUNK):
    """Work items of the oriented rows, one i32 (u32 bits) [n, 3] tensor per
    role in ROLES order: {row u, first, last} = the arcs first..last-1 of
    row u (offsets inside the row). A row of out-degree d >= 1 gives
    ceil(d / chunk) items, all in the role d selects."""
    d = optr[1:] - optr[:-1]
    masks = ((d >= 1) & (d < t1),
             (d >= t1) & (d <= stage_cap),
             (d >= t1) & (d > stage_cap))
    out = []
    for mask in masks:
        rows = torch.nonzero(mask).flatten()
        cnt = (d[rows] + (chunk - 1)) // chunk
        u = torch.repeat_interleave(rows, cnt)
        start = torch.cumsum(cnt, 0) - cnt
        idx = torch.arange(u.numel(), dtype=U64, device=optr.device) - \
            torch.repeat_interleave(start, cnt)
        first = idx * chunk
        last = torch.minimum(first + chunk, d[u])
        out.append(torch.stack([u, first, last], 1).to(U32).contiguous())
    return out


def clustering(per_vertex, deg):
    """Local clustering coefficients, f64[nv]: per_vertex / C(deg, 2), the
    share of a vertex's neighbour pairs that are adjacent; 0 where
    deg < 2. per_vertex and deg are i64 in the same vertex ids."""
    pairs = deg * (deg - 1) // 2
    out = torch.zeros(per_vertex.shape, dtype=torch.float64,
                      device=per_vertex.device)
    has = pairs > 0
    out[has] = per_vertex[has].to(torch.float64) / \
        pairs[has].to(torch.float64)
    return out


class TCEngine:
    def __init__(self, part: GraphPart, order="degree"):
        if part.nparts != 1:
            raise ValueError(
                "TCEngine is single-rank: an intersection needs both rows "
                f"on one device (got a GraphPart with nparts={part.nparts})")
        if order not in ORDERS:
            raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
        cap = int(os.environ.get("LUX_TC_STAGE", TC_STAGE_DEFAULT))
        if not 1 <= cap <= TC_STAGE_MAX:
            raise ValueError(f"LUX_TC_STAGE={cap} outside [1, {TC_STAGE_MAX}]")
        from . import _native_gpu as ng
        if TC_T1 - 1 > ng.tc_small_max() or TC_STAGE_MAX > ng.tc_stage_max():
            raise ValueError("TC_T1 / TC_STAGE_MAX beyond what tc.hip takes")
        self.part = part
        self.device = part.device
        self.order = order
        self.stage_cap = cap
        self.plain = os.environ.get("LUX_TC_PLAIN", "0") == "1"
        self.timed = False  # synchronise and clock count() (the app)
        self.phase_ms = dict(orient=0.0, items=0.0, count=0.0)
        nv = part.nv

        t0 = self._now()
        self.dag = orient(part.row_ptr, part.col, nv, order)
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)
        t0 = self._now()
        self.items = build_items(self.dag.optr, cap)
        self.phase_ms["items"] = 1000.0 * (self._now() - t0)

        d = self.dag.optr[1:] - self.dag.optr[:-1]
        self.max_out_degree = int(d.max().item()) if nv else 0
        self._acc = torch.zeros(2, dtype=U64, device=self.device)
        self._pv_rank = torch.zeros(max(nv, 1), dtype=U64,
                                    device=self.device)
        self._total = None
        self._probes = 0
        self._pv = None
        self._other = None  # the other order's DAG, built by check()

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    # -------- counting --------
    def _launch(self, dag, items, plain, acc, pv):
        from . import _native_gpu as ng
        s = _stream()
        if plain:
            ng.tc_count_plain(s, self.part.nv, dag.m, dag.optr, dag.oadj,
                              acc, pv)
            return
        for role, it in enumerate(items):
            ng.tc_count_items(s, role, dag.optr, dag.oadj, it, it.shape[0],
                              self.stage_cap, acc, pv)

    def count(self, per_vertex=False):
        """The total, recounted from zeroed accumulators; per_vertex=True
        also refreshes per_vertex()."""
        self._acc.zero_()
        pv = None
        if per_vertex:
            self._pv_rank.zero_()
            pv = self._pv_rank
        t0 = self._now() if self.timed else 0.0
        self._launch(self.dag, self.items, self.plain, self._acc, pv)
        acc = self._acc.cpu()  # the count's one host read
        if self.timed:
            self.phase_ms["count"] = 1000.0 * (time.perf_counter() - t0)
        self._total, self._probes = int(acc[0]), int(acc[1])
        if per_vertex:
            self._pv = self._pv_rank[:self.part.nv][self.dag.rank]
        return self._total

    def per_vertex(self):
        """Device u64[nv] (torch.int64 bits): triangles containing each
        vertex, in original ids. The stored array of the last
        count(per_vertex=True); counted now if there is none."""
        if self._pv is None:
            self.count(per_vertex=True)
        return self._pv

    def transitivity(self):
        if self._total is None:
            self.count()
        deg = self.dag.deg
        wedges = int((deg * (deg - 1) // 2).sum().item())
        return 3 * self._total / wedges if wedges else 0.0

    def clustering(self):
        """Device f64[nv], original ids: per_vertex / C(deg, 2) with deg the
        simple undirected degree; 0 where deg < 2."""
        return clustering(self.per_vertex(), self.dag.deg)

    @property
    def stats(self):
        st = dict(simple_edges=self.dag.m,
                  max_out_degree=self.max_out_degree)
        for name, it in zip(ROLES, self.items):
            st[f"items_{name}"] = int(it.shape[0])
        st["probes"] = self._probes  # elements of A(v) searched, last count
        return st

    def check(self):
        """Device check oracle: recount with the plain kernel on the OTHER
        orientation order and compare with the stored total and per-vertex
        array. Returns the number of mismatches: 1 if the totals differ,
        plus the vertices whose counts differ, plus 1 if per_vertex.sum()
        != 3 * total."""
        from . import _native_gpu as ng
        if self._pv is None or self._total is None:
            self.count(per_vertex=True)
        p = self.part
        if self._other is None:
            other = ORDERS[1 - ORDERS.index(self.order)]
            self._other = orient(p.row_ptr, p.col, p.nv, other)
        o = self._other
        acc = torch.zeros(2, dtype=U64, device=self.device)
        pv = torch.zeros(max(p.nv, 1), dtype=U64, device=self.device)
        ng.tc_count_plain(_stream(), p.nv, o.m, o.optr, o.oadj, acc, pv)
        want_total = int(acc[0].item())
        want_pv = pv[:p.nv][o.rank]
        bad = int(want_total != self._total)
        bad += int((want_pv != self._pv).sum().item())
        bad += int(int(self._pv.sum().item()) != 3 * self._total)
        return bad
