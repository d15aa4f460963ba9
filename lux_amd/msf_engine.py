"""Minimum spanning forest on one GPU: synchronous Boruvka rounds
(src/gpu/msf.hip). No reference equivalent.

Definition — the same graph as TCEngine and KCoreEngine: the underlying
simple undirected graph of whatever the project loads ({u,v} is an edge iff
u != v and u->v or v->u occurs; self-loops vanish), with
  weight of {u,v} = the minimum i32 weight over all its occurrences, in
                    either direction (hash weights depend on (src, dst), so
                    the two arcs of a symmetric file differ); any i32;
  edge id e       = the index in the list of simple edges ascending by
                    (lo << 32) | hi; m is their number (m < 2^32);
  order           = (w, e), strict, so the forest is unique: it is the set of
                    edges Kruskal takes when ties break by edge id;
  results         = the forest as a bool mask over the m edges and as a
                    (lo, hi, w) list in key order; its size nf = nv -
                    components; the total weight, an exact Python int (i64 on
                    the device); labels[v] = the largest vertex id of v's
                    component (int32 holding u32 bits), v for an isolated
                    vertex.

Preparation (timed as phase_ms["orient"], ["weights"], ["adjacency"]):
tc_engine.orient(..., "id") gives the simple graph as the DAG lo -> hi, whose
arc e is simple edge e; msf_weights_kernel folds the weight of every CSC arc
into w[e] by an atomic minimum; the full degree is the DAG's out-degree plus
its in-degree, aptr its cumsum, and msf_adj_fill_kernel writes both
directions of every arc into anbr with its edge id in aeid; the rows longer
than the hub length give the static {row, chunk} item list.

solve() follows tests/msf_ref.sync_boruvka round for round: a scan leaves in
best[c] the minimum (w, e) entry that leaves component c; the hook joins
every component with such an edge to the one at its other end (of two that
chose the same edge only the smaller id hooks) and marks the edge; the
flatten relabels every vertex to its root. Then the host reads the 8-word
meta record once; a round in which nothing hooked ends the run. A row whose
scan finds no entry leaving its component is dead and never walked again
(components only merge). At most ceil(log2 nv) rounds do anything, so the
loop raises beyond 34 and never spins. Every host tensor is one-dimensional,
and none that scales with m is written through a mask or an index.

Env knobs: LUX_MSF_HUB (rows longer than this are walked by workgroups, in
chunks of this many entries; default the kernels' MSF_HUB), LUX_MSF_DEAD=0
(walk every row in every scan).
"""
import os
import time

import torch

from .engine import GraphPart
from .tc_engine import orient

U8, U32, U64 = torch.uint8, torch.int32, torch.int64
NONE = 0xFFFFFFFF
HUB_MAX = 1 << 20
MAX_ROUNDS = 34
I32_MAX = (1 << 31) - 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


class MSFEngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "MSFEngine is single-rank: a component's minimum edge is "
                "searched over all its rows on one device "
                f"(got a GraphPart with nparts={part.nparts})")
        if part.weight is None:
            raise ValueError("MSFEngine needs edge weights (part.weight is "
                             "None): load a weighted .lux file or call "
                             "part.hash_weights(wmax)")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_MSF_HUB", ng.msf_hub_default()))
        if not 1 <= hub <= HUB_MAX:
            raise ValueError(f"LUX_MSF_HUB={hub} outside [1, {HUB_MAX}]")
        dead = os.environ.get("LUX_MSF_DEAD", "1")
        if dead not in ("0", "1"):
            raise ValueError(f"LUX_MSF_DEAD={dead} is neither 0 nor 1")
        self.part = part
        self.device = dev = part.device
        self.hub, self.dead = hub, dead == "1"
        self.timed = False  # synchronise and clock solve() (the app)
        self.phase_ms = dict(orient=0.0, weights=0.0, adjacency=0.0,
                             solve=0.0)
        nv = part.nv
        n1 = max(nv, 1)
        s = _stream()

        t0 = self._now()
        dag = orient(part.row_ptr, part.col, nv, "id")
        self.phase_ms["orient"] = 1000.0 * (self._now() - t0)
        self.m = m = dag.m
        if m >= 1 << 32:
            raise ValueError(f"MSFEngine: {m} simple edges, edge ids are "
                             f"32-bit (m < 2^32)")
        m1 = max(m, 1)

        # ---- w[e]: the minimum over the occurrences of edge e ----
        t0 = self._now()
        self._optr = dag.optr
        self._ehi = dag.oadj if m else torch.zeros(1, dtype=U32, device=dev)
        self._w = torch.full((m1,), I32_MAX, dtype=U32, device=dev)
        err = torch.zeros(1, dtype=U64, device=dev)
        if m:
            ng.msf_weights(s, nv, part.ep, part.row_ptr, part.col,
                           part.weight, dag.optr, self._ehi, self._w, err)
            if int(err.item()):
                raise RuntimeError(f"MSF weights: {int(err.item())} arcs "
                                   f"without their simple edge")
        self.phase_ms["weights"] = 1000.0 * (self._now() - t0)

        # ---- both directions of every edge, with its id ----
        t0 = self._now()
        indeg = torch.zeros(n1, dtype=U32, device=dev)
        if m:
            ng.hist_u32(s, m, self._ehi, indeg)
        self.degree = (dag.optr[1:] - dag.optr[:-1]).to(U32) + indeg[:nv]
        self.aptr = torch.zeros(nv + 1, dtype=U64, device=dev)
        self.aptr[1:] = torch.cumsum(self.degree, 0, dtype=U64)
        self._anbr = torch.empty(max(2 * m, 1), dtype=U32, device=dev)
        self._aeid = torch.empty(max(2 * m, 1), dtype=U32, device=dev)
        self._elo = torch.empty(m1, dtype=U32, device=dev)
        indeg.zero_()  # now the per-row cursor
        ng.msf_adj_fill(s, nv, m, dag.optr, self._ehi, self.aptr, indeg,
                        self._anbr, self._aeid, self._elo)
        self.max_degree = int(self.degree.max().item()) if nv else 0
        # the static work list of the hub role: chunk item_chunk[i] of row
        # hubrow[item_row[i]]
        rows = torch.nonzero(self.degree > hub, as_tuple=True)[0]
        nc = (self.degree[rows].to(U64) + (hub - 1)) // hub
        self.hub_rows = int(rows.numel())
        self.hub_items = int(nc.sum().item())
        if self.hub_items >= 1 << 32:
            raise ValueError(f"MSFEngine: {self.hub_items} hub items")
        if self.hub_rows:
            item_row = torch.repeat_interleave(
                torch.arange(self.hub_rows, device=dev), nc)
            first = torch.repeat_interleave(torch.cumsum(nc, 0) - nc, nc)
            item_chunk = torch.arange(self.hub_items, device=dev) - first
            self._hubrow = rows.to(U32)
            self._item_row = item_row.to(U32)
            self._item_chunk = item_chunk.to(U32)
        else:
            self._hubrow = torch.zeros(1, dtype=U32, device=dev)
            self._item_row = torch.zeros(1, dtype=U32, device=dev)
            self._item_chunk = torch.zeros(1, dtype=U32, device=dev)
        del dag, indeg, rows, nc
        self.phase_ms["adjacency"] = 1000.0 * (self._now() - t0)

        def vec(n=n1, dtype=U32):
            return torch.empty(n, dtype=dtype, device=dev)

        self._comp, self._parent, self._label = vec(), vec(), vec()
        self._best = vec(dtype=U64)
        self._deadrow = vec(dtype=U8)
        self._inforest = vec(m1, U8)
        self._hubext = vec(max(self.hub_rows, 1))
        self._meta = torch.zeros(ng.msf_meta_words(), dtype=U64, device=dev)
        self._out = torch.zeros(4, dtype=U64, device=dev)
        self._args = ng.msf_args(
            self.aptr, self._anbr, self._aeid, self._elo, self._ehi, self._w,
            self._comp, self._parent, self._best, self._deadrow,
            self._inforest, self._hubrow, self._hubext, self._item_row,
            self._item_chunk, self._meta, m, nv, self.hub_rows,
            self.hub_items, hub, self.dead)
        self._done = False
        self._total = self._nf = 0
        self._stats = self._fresh_stats()

    @staticmethod
    def _fresh_stats():
        return dict(rounds=0, scans=0, launches=0, host_reads=0, scanned=0,
                    per_round=[])

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    # -------- the host loop --------
    def _read_meta(self):
        """The blocking read of the meta record, one per round."""
        self._stats["host_reads"] += 1
        return self._meta.tolist()

    def solve(self):
        """Build the forest from scratch; returns its total weight."""
        from . import _native_gpu as ng
        st = self._stats = self._fresh_stats()
        t0 = self._now() if self.timed else 0.0
        s, a, nv = _stream(), self._args, self.part.nv
        ng.msf_init(s, a)
        st["launches"] += 1 if nv else 0
        total = nf = 0
        while self.m:
            if st["scans"] > MAX_ROUNDS:
                raise RuntimeError(
                    f"MSF does not terminate: {st['scans']} scans on "
                    f"{nv} vertices, per round {st['per_round']}")
            st["launches"] += ng.msf_scan(s, a, st["scans"] + 1)
            ng.msf_hook(s, a)
            ng.msf_flatten(s, a)
            st["launches"] += 2
            meta = self._read_meta()
            st["scans"] += 1
            if meta[ng.MSF_M_ERR]:
                raise RuntimeError(f"MSF hook: {meta[ng.MSF_M_ERR]} "
                                   f"components with a broken minimum edge")
            cwe, merged, scanned = (meta[ng.MSF_M_CWE], meta[ng.MSF_M_MERGED],
                                    meta[ng.MSF_M_SCANNED])
            st["scanned"] += scanned
            total, nf = meta[ng.MSF_M_TOTAL], meta[ng.MSF_M_NF]
            if merged == 0:
                break
            if not merged <= cwe <= nv or nf >= nv:
                raise RuntimeError(f"MSF round out of bounds: {cwe} "
                                   f"components with an edge, {merged} "
                                   f"hooks, {nf} forest edges, nv={nv}")
            st["rounds"] += 1
            st["per_round"].append((cwe, merged, scanned))
        if nv:
            # _parent is free now: the scratch of the maximum ids
            ng.msf_labels(s, nv, self._comp, self._parent, self._label)
            st["launches"] += 2
        if self.timed:
            self.phase_ms["solve"] = 1000.0 * (self._now() - t0)
        self._total, self._nf = int(total), int(nf)
        self._done = True
        return self._total

    # -------- results --------
    def _solved(self):
        if not self._done:
            self.solve()

    def total_weight(self):
        self._solved()
        return self._total

    def num_edges(self):
        """nf, the number of forest edges."""
        self._solved()
        return self._nf

    def num_components(self):
        return self.part.nv - self.num_edges()

    def in_forest(self):
        """Device bool[m]: the forest as a mask over the simple edges."""
        self._solved()
        return self._inforest[:self.m].view(torch.bool)

    def simple_edges(self):
        """Device (lo, hi, w) of all m simple edges in key order: int32
        holding u32 bits, int32 holding u32 bits, int32."""
        return self._elo[:self.m], self._ehi[:self.m], self._w[:self.m]

    def edges(self):
        """Device (lo, hi, w) of the forest in key order."""
        mask = self.in_forest()
        return tuple(torch.masked_select(t, mask)
                     for t in self.simple_edges())

    def labels(self):
        """Device int32[nv] (u32 bits): the largest vertex id of each
        vertex's component."""
        self._solved()
        return self._label[:self.part.nv]

    @property
    def stats(self):
        return dict(simple_edges=self.m, max_degree=self.max_degree,
                    hub_rows=self.hub_rows, hub_items=self.hub_items,
                    **self._stats)

    def check(self, mask=None):
        """Device check oracle (msf_check_*_kernel), the violations of:
        (a) a plain lock-free union over the forest edges only and one over
        all edges flatten to the same labels, and these equal labels();
        with nf == nv - components (counted again here) that makes the mask
        a spanning forest; its edge count and weight equal num_edges() and
        total_weight(); (b) every non-isolated vertex's minimum (w, e)
        entry is in the forest. Necessary, not sufficient for minimality
        (a spanning forest that keeps every vertex's lightest edge passes),
        so exactness rests on the tests against the CPU oracle. mask: a
        device u8[m] to judge instead of the engine's own forest (the
        tests' hook)."""
        from . import _native_gpu as ng
        self._solved()
        nv, dev = self.part.nv, self.device
        if mask is None:
            mask = self._inforest
        elif mask.dtype != U8 or mask.numel() < max(self.m, 1):
            raise ValueError("check(mask): need a device uint8[m] tensor")
        pf = torch.empty(max(nv, 1), dtype=U32, device=dev)
        pa = torch.empty(max(nv, 1), dtype=U32, device=dev)
        ng.msf_check(_stream(), nv, self.m, self.aptr, self._aeid, self._elo,
                     self._ehi, self._w, mask, self._label, pf, pa,
                     self._out)
        bad, count, roots, weight = self._out.tolist()
        return (bad + int(count != nv - roots) + int(count != self._nf) +
                int(weight != self._total))
