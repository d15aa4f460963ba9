"""CF top-N recommendation on one GPU (src/gpu/cf_topn.hip): the n best
admissible candidates of an id range for every query vertex, by the fp32 dot
product of their factor rows. Scoring (MFMA) and selection are one kernel, so
no users x items score matrix exists. No reference equivalent; the definition
is in API.md.

    rec = CFTopN(part, eng.vectors())
    items, scores = rec.recommend(users, n=10)     # unseen items per user
    items, scores = rec.similar(items, n=10)       # item-item, self excluded
    items, scores = rec.topn(queries, c_lo, c_hi, n, excl_ptr, excl_adj)

Order: (score_i, i) precedes (score_j, j) iff score_i > score_j, or the scores
are equal and i < j. Row p of the result holds the first n admissible
candidates of queries[p] in that order, i32 items and f32 scores, padded with
-1 / -inf. The result is one fixed tensor: the same bits across runs and
across every work split.

Exclusion is a CSR over vertex ids (excl_ptr i64[nv+1], excl_adj u32) with
ASCENDING rows; repeated entries are allowed (a parallel edge of the graph
stays a repeated entry of the "seen" row, the lower bound does not mind).
The "seen" CSR of recommend() is built lazily, once: cf_topn_keys_kernel
emits (row << 32) | col for runs of at most LUX_TC_SORT_CHUNK CSC entries cut
at row boundaries, each run is sorted and its low words are the sorted rows.
Every m-sized tensor is one-dimensional and goes through the keys kernel,
sort, slices and element-wise ops only (the rules after BENCHLOG r11.1). Only
a graph with more entries than one chunk reads row boundaries on the host.

Queries given as a list, an array or a CPU tensor are range-checked here. A
device tensor is not read back: the kernel gives an id outside [0, nv) an
all-padding row, which check() counts. Apart from that, a call reads nothing
on the host; check() and stats["ms"] do.

Env knobs: LUX_CF_TOPN_SPLIT (force the number of candidate splits),
LUX_TC_SORT_CHUNK (keys per sort).
"""
import os

import numpy as np
import torch

from .engine import GraphPart
from .tc_engine import SORT_CHUNK_DEFAULT

U32, U64, F32 = torch.int32, torch.int64, torch.float32
MASK32 = 0xFFFFFFFF


def _stream():
    return torch.cuda.current_stream().cuda_stream


class CFTopN:
    def __init__(self, part: GraphPart, vectors):
        from . import _native_gpu as ng
        if part.nparts != 1:
            raise ValueError(
                "CFTopN is single-rank: the seen rows of a partition are "
                f"local (got a GraphPart with nparts={part.nparts})")
        if not (isinstance(vectors, torch.Tensor) and vectors.dtype == F32
                and vectors.dim() == 2 and vectors.shape[0] == part.nv
                and vectors.device == part.col.device):
            raise ValueError(
                f"vectors must be an f32 [nv={part.nv}, K] tensor on "
                f"{part.col.device}, got "
                f"{getattr(vectors, 'dtype', type(vectors))} "
                f"{tuple(getattr(vectors, 'shape', ()))} on "
                f"{getattr(vectors, 'device', None)}")
        if not 1 <= vectors.shape[1] <= ng.CF_TOPN_KMAX:
            raise ValueError(f"K={vectors.shape[1]} outside "
                             f"[1, {ng.CF_TOPN_KMAX}]")
        self.part = part
        self.device = part.col.device
        self.vectors = vectors.contiguous()
        self.K = int(vectors.shape[1])
        self._none = self._seen = self._ident = None
        self._last = None    # (args, tensors kept alive, items, scores)
        self._events = None
        self._stats = dict(splits=0, workgroups=0, launches=0, tiles=0)

    # -------- exclusion CSRs --------
    def _no_exclusion(self):
        if self._none is None:
            self._none = (torch.zeros(self.part.nv + 1, dtype=U64,
                                      device=self.device),
                          torch.zeros(1, dtype=U32, device=self.device), 0)
        return self._none

    def _identity(self):
        if self._ident is None:
            nv = self.part.nv
            self._ident = (torch.arange(nv + 1, dtype=U64, device=self.device),
                           torch.arange(nv, dtype=U32, device=self.device),
                           nv)
        return self._ident

    def seen(self):
        """(excl_ptr, excl_adj, entries): row v = the sources of v's CSC row,
        ascending, parallel edges repeated."""
        if self._seen is not None:
            return self._seen
        from . import _native_gpu as ng
        p, dev = self.part, self.device
        chunk = max(int(os.environ.get("LUX_TC_SORT_CHUNK",
                                       SORT_CHUNK_DEFAULT)), 1)
        adj = torch.empty(max(p.ep, 1), dtype=U32, device=dev)
        e0 = 0
        while e0 < p.ep:
            e1 = p.ep
            if e1 - e0 > chunk:  # the last row boundary within the chunk
                r = int(torch.searchsorted(
                    p.row_ptr, torch.tensor([e0 + chunk], dtype=U64,
                                            device=dev), right=True).item())
                e1 = int(p.row_ptr[r - 1].item())
                if e1 <= e0:     # a single row longer than the chunk
                    e1 = int(p.row_ptr[r].item())
            keys = torch.empty(e1 - e0, dtype=U64, device=dev)
            ng.cf_topn_keys(_stream(), p.vp, p.row_ptr, p.col, e0, e1, keys)
            adj[e0:e1] = torch.sort(keys).values & MASK32
            del keys
            e0 = e1
        self._seen = (p.row_ptr, adj, p.ep)
        return self._seen

    # -------- the calls --------
    def _query_ids(self, queries, lo, hi):
        """-> device i32[q]; host-side ids are checked against [lo, hi)."""
        if isinstance(queries, torch.Tensor) and queries.is_cuda:
            if queries.dtype not in (U32, U64) or queries.dim() != 1:
                raise ValueError("queries must be a one-dimensional int32 or "
                                 f"int64 tensor, got {queries.dtype} "
                                 f"{tuple(queries.shape)}")
            if queries.device != self.device:
                raise ValueError(f"queries are on {queries.device}, the "
                                 f"factors on {self.device}")
            ids = queries.to(U32).contiguous()
        else:
            try:
                host = np.asarray(queries.numpy() if isinstance(
                    queries, torch.Tensor) else queries)
                if host.dtype.kind not in "iu" or host.ndim != 1:
                    raise TypeError
                host = host.astype(np.int64)
            except (TypeError, ValueError):
                raise ValueError("queries must be a one-dimensional sequence "
                                 f"of vertex ids, got {queries!r}") from None
            if host.size and not lo <= host.min() <= host.max() < hi:
                raise ValueError(f"query ids must lie in [{lo}, {hi}), got "
                                 f"[{host.min()}, {host.max()}]")
            ids = torch.from_numpy(host.astype(np.int32)).to(self.device)
        if ids.numel() < 1:
            raise ValueError("queries must name at least one vertex")
        return ids

    @staticmethod
    def _check_n(n):
        from . import _native_gpu as ng
        if not isinstance(n, (int, np.integer)) or \
                not 1 <= n <= ng.CF_TOPN_NMAX:
            raise ValueError(f"n must be an integer in [1, "
                             f"{ng.CF_TOPN_NMAX}], got {n!r}")
        return int(n)

    def topn(self, queries, c_lo, c_hi, n, excl_ptr=None, excl_adj=None):
        """(items i32[q, n], scores f32[q, n]) on the device."""
        nv, dev = self.part.nv, self.device
        n = self._check_n(n)
        if not all(isinstance(c, (int, np.integer)) for c in (c_lo, c_hi)) \
                or not 0 <= c_lo < c_hi <= min(nv, 2 ** 31 - 1):
            raise ValueError(f"candidates must be a non-empty range within "
                             f"[0, {nv}), got [{c_lo!r}, {c_hi!r})")
        ids = self._query_ids(queries, 0, nv)
        if (excl_ptr is None) != (excl_adj is None):
            raise ValueError("excl_ptr and excl_adj go together")
        if excl_ptr is None:
            return self._run(ids, c_lo, c_hi, n, self._no_exclusion())
        for t, dt, name in ((excl_ptr, U64, "excl_ptr i64[nv+1]"),
                            (excl_adj, U32, "excl_adj u32 (as int32)")):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt
                    and t.dim() == 1 and t.device == dev
                    and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous "
                                 f"one-dimensional tensor on {dev}")
        if excl_ptr.numel() != nv + 1:
            raise ValueError(f"excl_ptr has {excl_ptr.numel()} entries, "
                             f"nv + 1 = {nv + 1}")
        n_excl = excl_adj.numel()
        if not n_excl:
            excl_adj = self._no_exclusion()[1]
        return self._run(ids, c_lo, c_hi, n, (excl_ptr, excl_adj, n_excl))

    def _run(self, ids, c_lo, c_hi, n, excl):
        from . import _native_gpu as ng
        nv, dev = self.part.nv, self.device
        excl_ptr, excl_adj, n_excl = excl
        force = os.environ.get("LUX_CF_TOPN_SPLIT")
        if force is not None and (not force.isdigit() or int(force) < 1):
            raise ValueError(f"LUX_CF_TOPN_SPLIT={force!r} must be an "
                             "integer >= 1")
        q, c_lo, c_hi = ids.numel(), int(c_lo), int(c_hi)
        S = ng.cf_topn_plan(q, c_hi - c_lo, n, int(force or 0))
        items = torch.empty((q, n), dtype=U32, device=dev)
        scores = torch.empty((q, n), dtype=F32, device=dev)
        pi = ps = None
        if S > 1:
            pi = torch.empty(S * q * n, dtype=U32, device=dev)
            ps = torch.empty(S * q * n, dtype=F32, device=dev)
        keep = (self.vectors, ids, excl_ptr, excl_adj, items, scores, pi, ps)
        a = ng.cf_topn_args(keep, n_excl, nv, self.K, q, n, c_lo, c_hi, S)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        launches = ng.cf_topn(_stream(), a)
        ev[1].record()
        self._events = ev
        self._last = (a, keep[:4], items, scores)
        tiles = -(-(c_hi - c_lo) // ng.CF_TOPN_TILE)
        self._stats = dict(splits=S, workgroups=-(-q // 64) * S,
                           launches=launches, tiles=tiles)
        return items, scores

    def _boundary(self):
        nu = self.part.n_users
        if nu is None:
            raise RuntimeError("recommend / similar need the bipartite "
                               "boundary: part.n_users is unset (load a "
                               "graph with -users / use the bipartite "
                               "builders)")
        return nu

    def recommend(self, users, n=10, exclude_seen=True):
        """The n best items of [n_users, nv) per user; with exclude_seen
        never an item of the user's own row of the graph."""
        nu, n = self._boundary(), self._check_n(n)
        ids = self._query_ids(users, 0, nu)
        excl = self.seen() if exclude_seen else self._no_exclusion()
        return self._run(ids, nu, self.part.nv, n, excl)

    def similar(self, items, n=10):
        """The n items of [n_users, nv) closest to each item, itself left
        out."""
        nu, n = self._boundary(), self._check_n(n)
        ids = self._query_ids(items, nu, self.part.nv)
        return self._run(ids, nu, self.part.nv, n, self._identity())

    # -------- results --------
    @property
    def stats(self):
        """splits, workgroups, launches and tiles of the last call; ms, its
        device time (reading it synchronises)."""
        ms = 0.0
        if self._events is not None:
            self._events[1].synchronize()
            ms = self._events[0].elapsed_time(self._events[1])
        return dict(ms=ms, **self._stats)

    def check(self, items=None, scores=None):
        """Device check (cf_topn_plain_kernel) of the last call, or of
        (items, scores) in its place: a wave per query recomputes every
        candidate's score as one serial fmaf chain with absdot = sum |u_k
        v_k| and counts returned items that are out of range, excluded or
        repeated, neighbours out of order, returned scores further than
        tol = 2 K 2^-24 absdot from the recomputed one, and admissible
        candidates left out whose score exceeds the last returned one by more
        than both tols. Necessary, not sufficient: a swap of two near-ties
        within tol passes."""
        from . import _native_gpu as ng
        if self._last is None:
            raise ValueError("no result yet: call recommend, similar or topn "
                             "first")
        a, _, own_items, own_scores = self._last
        if (items is None) != (scores is None):
            raise ValueError("items and scores go together")
        if items is None:
            items, scores = own_items, own_scores
        else:
            items = torch.as_tensor(items).to(self.device, U32).contiguous()
            scores = torch.as_tensor(scores).to(self.device, F32).contiguous()
            if items.shape != own_items.shape or scores.shape != items.shape:
                raise ValueError(f"items and scores must have the shape "
                                 f"{tuple(own_items.shape)} of the last call")
        bad = torch.zeros(a.q, dtype=U32, device=self.device)
        ng.cf_topn_check(_stream(), a, items, scores, bad)
        return int(bad.sum().item())
