"""Batched personalised PageRank on one GPU (src/gpu/ppr.hip): K random
walks with restart at once, the K rank vectors kept vertex-major so that one
gathered source row serves every column. No reference equivalent; the
definition is in API.md.

The directed graph exactly as loaded: an entry u -> v is followed from u to
v, parallel entries and self-loops count. Column c has a non-empty seed set
S_c of distinct vertices, t_c = 1/|S_c| on S_c, and

    x_c^0 = t_c
    x_c^(i+1)[v] = (1 - d) t_c[v] + d * sum over u -> v of x_c^i[u] / outdeg(u)

A walk ends at a vertex without out-edges (mass leaks, column sums <= 1), the
convention PagerankEngine has. The columns run in batches of 64; a batch is
B = 16, 32 or 64 columns wide, the smallest that holds it, padding columns
have no teleport and stay zero. An iteration is one sweep launch (two with
hub rows). tol == 0 reads nothing on the host during the iterations; tol > 0
reads the 4-byte residual after every iteration and stops at the first one
<= tol.

Preparation (phase_ms["plan"]): the out-degrees, the static role lists by
in-degree — [0, PPR_GROUP] one lane group per row, up to LUX_PPR_HUB one
wave per row, longer rows as {vertex, chunk} items of LUX_PPR_HUB entries —
and the hub scratch.

Env knob: LUX_PPR_HUB (default the kernels' PPR_HUB, 64..2^20).
"""
import os
import time

import numpy as np
import torch

from .engine import GraphPart

U32, U64, F32 = torch.int32, torch.int64, torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _hub_items(deg, hub):
    """(items, number of items, rows, number of rows) of the rows longer
    than hub: flat u32 {vertex, chunk} pairs and {vertex, first item, items}
    triples, both in vertex order."""
    dev = deg.device
    hv = torch.nonzero(deg > hub, as_tuple=True)[0]
    nc = (deg[hv] + (hub - 1)) // hub
    first = torch.cumsum(nc, 0) - nc
    v = torch.repeat_interleave(hv, nc)
    c = torch.arange(v.numel(), device=dev) - torch.repeat_interleave(first, nc)
    items = torch.zeros(2 * max(v.numel(), 1), dtype=U32, device=dev)
    rows = torch.zeros(3 * max(hv.numel(), 1), dtype=U32, device=dev)
    if v.numel():
        items[0::2], items[1::2] = v.to(U32), c.to(U32)
        rows[0::3], rows[1::3], rows[2::3] = \
            hv.to(U32), first.to(U32), nc.to(U32)
    return items, int(v.numel()), rows, int(hv.numel())


def _seed_sets(seeds, nv):
    """seeds -> a list of lists of distinct vertex ids, one per column."""
    try:
        sets = [[int(s)] if isinstance(s, (int, np.integer))
                else [int(x) for x in s] for s in seeds]
    except (TypeError, ValueError):
        raise ValueError(f"seeds must be a list of vertex ids or lists of "
                         f"vertex ids, got {seeds!r}") from None
    if not sets:
        raise ValueError("seeds must name at least one column")
    for c, s in enumerate(sets):
        if not s or len(set(s)) != len(s) or not 0 <= min(s) <= max(s) < nv:
            raise ValueError(f"seeds[{c}] must be a non-empty set of distinct "
                             f"vertex ids in [0, {nv}), got {s[:8]}")
    return sets


class PPREngine:
    def __init__(self, part: GraphPart):
        if part.nparts != 1:
            raise ValueError(
                "PPREngine is single-rank: a sweep gathers the rows of every "
                f"in-neighbour on one device (got a GraphPart with "
                f"nparts={part.nparts})")
        from . import _native_gpu as ng
        hub = int(os.environ.get("LUX_PPR_HUB", ng.ppr_hub_default()))
        if not ng.ppr_hub_min() <= hub <= ng.ppr_hub_max():
            raise ValueError(f"LUX_PPR_HUB={hub} outside "
                             f"[{ng.ppr_hub_min()}, {ng.ppr_hub_max()}]")
        nv, ne = part.nv, part.ep
        if nv < 1:
            raise ValueError("PPREngine needs at least one vertex")
        self.part = part
        self.device = dev = part.device
        self.hub, self.group = hub, ng.ppr_group_limit()
        self.timed = False  # synchronise and clock run() (the app)
        self.phase_ms = dict(plan=0.0, run=0.0)

        t0 = self._now()
        self._outdeg = torch.zeros(nv, dtype=U32, device=dev)
        if ne:
            ng.hist_u32(_stream(), ne, part.col, self._outdeg)
        in_deg = part.row_ptr[1:] - part.row_ptr[:-1]
        self._grp = torch.nonzero(in_deg <= self.group,
                                  as_tuple=True)[0].to(U32)
        self._wav = torch.nonzero((in_deg > self.group) & (in_deg <= hub),
                                  as_tuple=True)[0].to(U32)
        self._n_grp, self._n_wav = self._grp.numel(), self._wav.numel()
        if not self._n_grp:  # never read; the pointers stay valid
            self._grp = torch.zeros(1, dtype=U32, device=dev)
        if not self._n_wav:
            self._wav = torch.zeros(1, dtype=U32, device=dev)
        self._hub_in, self._n_hub_in, self._hub_rows, self.hub_rows = \
            _hub_items(in_deg, hub)
        del in_deg
        self._scratch = torch.zeros(max(self._n_hub_in, 1) * ng.PPR_BATCH,
                                    dtype=F32, device=dev)
        self.phase_ms["plan"] = 1000.0 * (self._now() - t0)

        self._bad = torch.zeros(1, dtype=U64, device=dev)
        self._y = None        # the two state buffers of the last batch
        self._cur = 0         # which of them holds the last iteration
        self._args = self._keep = None
        self._ranks = None
        self._iterations = []
        self.residual_trace = []
        self.batch_ms = []
        self._stats = dict(launches=0, host_reads=0, width=0)

    def _now(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter()

    def _batch_args(self, sets, width, d32):
        """The lux_ppr_args of one batch and its per-column x^0."""
        from . import _native_gpu as ng
        nv, dev = self.part.nv, self.device
        sizes = np.array([len(s) for s in sets], np.int64)
        v = np.concatenate([np.asarray(s, np.int64) for s in sets])
        c = np.repeat(np.arange(len(sets), dtype=np.int64), sizes)
        order = np.lexsort((c, v))
        v, c = v[order], c[order]
        w = ((1.0 - d32) / sizes[c]).astype(np.float32)
        bits = np.zeros((nv + 31) // 32, np.uint32)
        np.bitwise_or.at(bits, v >> 5,
                         np.uint32(1) << (v & 31).astype(np.uint32))
        x0 = np.zeros(width, np.float32)
        x0[:len(sets)] = 1.0 / sizes

        def up(a, view=None):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(view) if view else a).to(dev)

        keep = (up(bits, np.int32), up(v.astype(np.uint32), np.int32),
                up(c.astype(np.uint32), np.int32), up(w), up(x0))
        args = ng.ppr_args(
            (self.part.row_ptr, self.part.col, self._outdeg, self._grp,
             self._wav, self._hub_in, self._hub_rows, self._scratch,
             keep[0], keep[1], keep[2], keep[3]),
            nv, self._n_grp, self._n_wav, self._n_hub_in, self.hub_rows,
            int(v.size), self.hub, width, d32)
        return args, keep

    # -------- the iteration --------
    def run(self, seeds, iters=20, tol=0.0, damping=0.85):
        """Iterate every column; returns ranks()."""
        from . import _native_gpu as ng
        nv, dev = self.part.nv, self.device
        sets = _seed_sets(seeds, nv)
        d32 = float(np.float32(damping)) if isinstance(
            damping, (int, float, np.floating)) else float("nan")
        if not 0.0 < d32 < 1.0:
            raise ValueError(f"damping must be a float in (0, 1), got "
                             f"{damping!r}")
        if not isinstance(iters, (int, np.integer)) or iters < 1:
            raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
        if not tol >= 0.0:
            raise ValueError(f"tol must be >= 0, got {tol!r}")
        K, W = len(sets), ng.PPR_BATCH
        t_run = self._now() if self.timed else 0.0
        s = _stream()
        self._ranks = torch.empty((nv, K), dtype=F32, device=dev)
        self._iterations, self.residual_trace, self.batch_ms = [], [], []
        st = self._stats = dict(launches=0, host_reads=0, width=0)
        for b in range(0, K, W):
            batch = sets[b:b + W]
            width = next(w for w in ng.PPR_WIDTHS if w >= len(batch))
            st["width"] = max(st["width"], width)
            t0 = self._now() if self.timed else 0.0
            a, keep = self._batch_args(batch, width, d32)
            if self._y is None or self._y[0].numel() != nv * width:
                self._y = None  # free before the new pair is allocated
                self._y = [torch.empty(nv * width, dtype=F32, device=dev)
                           for _ in range(2)]
            self._args, self._keep, cur = a, keep, 0
            res = torch.zeros(iters, dtype=F32, device=dev)
            ng.ppr_seed(s, a, self._y[0], keep[4])
            st["launches"] += 1
            done, trace = 0, []
            for it in range(iters):
                st["launches"] += ng.ppr_sweep(s, a, self._y[cur],
                                               self._y[1 - cur], res[it:])
                cur, done = 1 - cur, it + 1
                if tol > 0.0:
                    trace.append(float(res[it].item()))
                    st["host_reads"] += 1
                    if trace[-1] <= tol:
                        break
            if tol == 0.0:
                trace = res.tolist()  # once, after the last iteration
            ng.ppr_unscale(s, a, self._y[cur], self._ranks, K, b, len(batch))
            st["launches"] += 1
            self._cur = cur
            self._iterations.append(done)
            self.residual_trace.append(trace)
            if self.timed:
                self.batch_ms.append(1000.0 * (self._now() - t0))
        if self.timed:
            self.phase_ms["run"] = 1000.0 * (self._now() - t_run)
        return self._ranks

    def _ran(self):
        if self._ranks is None:
            raise ValueError("no result yet: call run(seeds) first")

    # -------- results --------
    def ranks(self):
        """Device f32[nv, K]: x, column c for seeds[c]."""
        self._ran()
        return self._ranks

    def iterations(self):
        """The iterations each batch ran."""
        self._ran()
        return list(self._iterations)

    def topk(self, k):
        """(values f32[K, k], vertices i64[K, k]), descending per column."""
        self._ran()
        return torch.topk(self._ranks.t(), min(int(k), self.part.nv), dim=1)

    def state(self):
        """Device f32[nv, width]: the stored form y = x / max(outdeg, 1) of
        the last batch after its last iteration (what check() examines)."""
        self._ran()
        return self._y[self._cur].view(self.part.nv, self._args.width)

    @property
    def stats(self):
        return dict(hub_rows=self.hub_rows, **self._stats)

    def check(self):
        """Device check (ppr_plain_kernel) of the last iteration of the last
        batch: one lane per (vertex, column) walks the row serially from the
        previous buffer, and the entries of state() further than
        (indeg + 6) * 2^-23 relative from its value are counted."""
        from . import _native_gpu as ng
        self._ran()
        self._bad.zero_()
        ng.ppr_check(_stream(), self._args, self._y[1 - self._cur],
                     self._y[self._cur], self._bad)
        return int(self._bad.item())
