"""Distributed push-model engine (SSSP, Connected Components).

The MI355X re-design of the reference's push pipeline
(push_app_task_impl, sssp_gpu.cu:335-522):
  - per-rank push CSR over ALL nv sources holding only edges into my
    partition (core/push_model.inl:321-324), built with device-wide scans;
  - adaptive per-partition frontier segments (dense bitmap / sparse queue,
    FrontierHeader-compatible) with majority-vote output format
    (sssp_gpu.cu:395-408), dense->sparse conversion and sparse-overflow
    fallback (sssp_gpu.cu:462-491) — ALL run as a device-predicated fixup
    chain (push.hip frontier_fixup), so the conversions never block the
    host;
  - pull fallback when the global frontier exceeds nv/16 (sssp_gpu.cu:414)
    or its out-edge volume dominates, served by the degree-binned pull
    kernels;
  - exchange: one batched RCCL p2p round per iteration over xGMI carrying
    only the USED frontier bytes, a label annex for sparse queues, and —
    only on dense iterations — the label slices. The reference instead
    re-reads whole zero-copy regions each iteration.

Latency hiding (reference: SLIDING_WINDOW=4 in-flight iterations,
sssp.cc:111-129): here each iteration has exactly ONE blocking D2H read —
the 32-byte-per-rank meta record produced on device and exchanged with the
payloads. Frontier counts, format decisions, conversion outcomes,
overflow flags and the push-vs-pull edge volume all ride that record, so
the r1 engine's 3-4 blocking reads per iteration are gone.
"""
import sys

import numpy as np
import torch

from . import _native_gpu as ng
from . import dist as dx
from .engine import GraphPart, run_pull
from .types import (DENSE_BITMAP, SPARSE_QUEUE, frontier_bytes,
                    frontier_capacity)

U8, U32, U64 = torch.uint8, torch.int32, torch.int64
INF_LABEL = 0xFFFFFFFF
SAT_LABEL = 0xFFFFFFFE  # largest finite label (push.hip sat_add_label)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _align16(x):
    return (x + 15) & ~15


def exchange_frontier_payloads(meta, verts_all, fq_all, new_seg, seg_off,
                               annex_all, new_annex, annex_off, labels,
                               labels_part, row_left_all, me):
    """Post the per-iteration payload exchange from a fresh meta table:
    frontier segments ship only their USED bytes, sparse queues ship a
    label annex, and ONLY dense ranks publish their label slice (sparse
    ranks' fresh labels ride the annex). One batched p2p round.

    Returns (work_handle, lab_n) — lab_n[q] > 0 iff rank q published its
    label slice. Factored out of PushEngine.step so the distributed
    byte-accounting is CPU-testable under gloo (tests/test_dist_cpu.py).
    """
    nparts = len(verts_all)
    used = [0] * nparts
    annex_n = [0] * nparts
    lab_n = [0] * nparts
    for q in range(nparts):
        if verts_all[q] == 0:
            continue
        if int(meta[q, 0]) == DENSE_BITMAP:
            used[q] = 8 + (verts_all[q] + 7) // 8
            lab_n[q] = verts_all[q]  # dense ranks publish labels
        else:
            used[q] = 8 + 4 * int(meta[q, 1])
            annex_n[q] = int(meta[q, 1])
    parts = [(fq_all,
              new_seg.narrow(0, 0, used[me]) if used[me] else None,
              used, seg_off),
             (annex_all,
              new_annex.narrow(0, 0, annex_n[me]) if annex_n[me] else None,
              annex_n, annex_off),
             (labels,
              labels_part if lab_n[me] else None,
              lab_n, row_left_all)]
    return dx.exchange_multi_async(parts, my_index=me), lab_n


class PushEngine:
    MODE_MIN = 1  # SSSP
    MODE_MAX = 2  # CC

    def __init__(self, part: GraphPart, mode, source=0, weighted=False,
                 delta=None):
        """weighted (MODE_MIN only): min-plus relaxation over part.weight
        (non-negative i32; ValueError on a negative one, agreed across
        ranks). Labels are exact shortest distances, saturating at
        0xFFFFFFFE; unreachable vertices keep INF. A label can improve in
        several iterations, so this mode uses neither the visited bitmap
        nor the pull kernels' settled-row skip.

        delta (weighted only; None or 0 = off): bucketed near-far schedule
        with bucket width delta. Only dirty vertices with label <= limit
        relax; the rest wait in a dirty bitmap until the limit advances to
        their bucket (see the "bucketed schedule" section below). Same
        labels, fewer relaxed edges, more iterations."""
        if delta is not None and delta < 0:
            raise ValueError("delta must be >= 0")
        if delta and not weighted:
            raise ValueError("delta (bucketed schedule) needs weighted=True")
        self.delta = int(delta or 0)
        self.part = part
        self.mode = mode
        self.is_min = mode == self.MODE_MIN
        self.weighted = bool(weighted)
        device = part.device
        self.device = device
        s = _stream()
        p = part
        if self.weighted:
            assert self.is_min, "weighted relaxation is MODE_MIN (SSSP) only"
            assert part.weight is not None, "weighted SSSP needs part.weight"
            # each rank checks its own slice; one all-reduce of the flag
            # makes every rank raise, or none
            neg = (part.weight.narrow(0, 0, p.ep) < 0).any().to(U32) \
                .reshape(1) if p.ep else torch.zeros(1, dtype=U32,
                                                     device=device)
            dx.all_reduce_sum_(neg)
            if int(neg.item()):
                raise ValueError("weighted SSSP needs non-negative edge "
                                 "weights")
        self._pull_mode = ng.PULL_MIN_W if self.weighted else (
            ng.PULL_MIN if self.is_min else ng.PULL_MAX)

        # pull bins (+ src-blocked CSC when nv is LLC-large) for the
        # dense fallback; the weighted one carries the weights per window
        if self.weighted:
            part.prepare_pull(weighted=True)
        else:
            part.prepare_pull()

        # ---- push CSR: all nv sources -> my-partition dsts ----
        deg_src = torch.zeros(p.nv, dtype=U32, device=device)
        ng.hist_u32(s, p.ep, p.col, deg_src)
        ends = torch.empty(p.nv, dtype=U64, device=device)
        partials = torch.empty(ng.scan_partials_size(p.nv), dtype=U64,
                               device=device)
        ng.scan_end_offsets(s, p.nv, deg_src, ends, partials)
        self.push_row_ptr = torch.empty(p.nv + 1, dtype=U64, device=device)
        ng.local_row_ptr(s, p.nv, 0, ends, self.push_row_ptr)
        cursor = self.push_row_ptr[:p.nv].clone()
        if self.weighted:
            # interleaved {global dst, weight} per out-edge (uint2[ep])
            self.push_col = None
            self.push_edge = torch.empty(2 * max(p.ep, 1), dtype=U32,
                                         device=device)
            ng.csr_scatter_w(s, p.ep, p.col, p.weight, p.row_ptr, p.vp,
                             p.row_left, cursor, self.push_edge)
        else:
            self.push_col = torch.empty(max(p.ep, 1), dtype=U32,
                                        device=device)
            ng.csr_scatter(s, p.ep, p.col, p.row_ptr, p.vp, p.row_left,
                           cursor, self.push_col)
        # global out-degrees (deg_src summed over ranks); keep only my
        # partition's slice — it prices the NEW frontier's out-edge volume
        # in the meta record (the exact push-vs-pull input)
        dx.all_reduce_sum_(deg_src)
        self.deg_part = deg_src.narrow(0, p.row_left, p.vp).clone() \
            if p.vp else torch.zeros(1, dtype=U32, device=device)
        torch.cuda.synchronize()
        del deg_src, ends, partials, cursor

        # ---- frontier buffers ----
        self.seg_bytes = [_align16(frontier_bytes(v)) for v in p.verts_all]
        self.seg_off = np.concatenate([[0], np.cumsum(self.seg_bytes)])
        self.capacity = frontier_capacity(p.vp)
        self.fq_all = torch.zeros(int(self.seg_off[-1]), dtype=U8,
                                  device=device)
        self.new_seg = torch.zeros(self.seg_bytes[p.p], dtype=U8,
                                   device=device)
        self.tmp_seg = torch.zeros_like(self.new_seg)
        # label annex: sparse queues travel with their final labels so
        # sparse iterations skip the O(nv) label slice exchange entirely
        caps = [frontier_capacity(v) for v in p.verts_all]
        self.annex_off = np.concatenate([[0], np.cumsum(caps)])
        self.fq_annex_all = torch.zeros(int(self.annex_off[-1]), dtype=U32,
                                        device=device)
        self.new_annex = torch.zeros(self.capacity, dtype=U32, device=device)
        # persistent zero header: zeroing via D2D copy (a python scalar
        # write does a pageable H2D that ABORTS hipGraph capture — and an
        # aborted capture can poison the stream)
        self._hdr_zero = torch.zeros(8, dtype=U8, device=device)
        # device meta record (u32[8]/rank: type,count,evol u64,overflow,..)
        self.meta_mine = torch.zeros(8, dtype=U32, device=device)
        self.meta_all = torch.zeros(8 * p.nparts, dtype=U32, device=device)

        # ---- edge-balanced scatter work items (push.hip expand+chunk):
        # push runs only while total frontier <= nv/16, so items are bounded
        # by nv/16 active vertices + ep/8192 extra chunks ----
        self.max_items = p.nv // 16 + p.ep // 8192 + 1024
        self.items = torch.empty(self.max_items * 2, dtype=U32,
                                 device=device)
        self.item_counter = torch.zeros(4, dtype=U32, device=device)
        # hop-SSSP (level-synchronous BFS) visited bitmap: push discovery
        # is a test-and-set against vp/8 bytes (L2-resident) instead of an
        # atomicMin against the 4*vp label array (push.hip BFS_BITS path);
        # rebuilt from labels after pull iterations. Weighted SSSP has no
        # one-shot discovery: no bitmap, label atomics only.
        self.visited = torch.empty((p.vp + 31) // 32, dtype=U32,
                                   device=device) \
            if self.is_min and not self.weighted else None
        self._bits_stale = True

        # ---- labels + frontier state ----
        self.labels = torch.empty(p.nv, dtype=U32, device=device)
        self.labels_part = torch.empty(p.vp, dtype=U32, device=device)
        self.snapshot = torch.empty_like(self.labels_part)
        # hipGraphs for the single-rank iteration bodies (pull / push
        # sparse-out / push dense-out): at world 1 every launch dimension
        # is static (frontier_expand_auto sizes itself from the segment
        # header on device), so a whole iteration replays as ONE graph
        # launch + one 32-byte meta read — removing the ~12-ctypes-call
        # host gap per iteration that made the python engine ~10% slower
        # than the native C++ runtime
        self._graphs = {}
        self._graph_uses = {}
        self._fq_init = None
        self.bucket_advances = 0
        self._seed_vols = {}
        if self.delta:
            # deferred set: one bit per local vertex, whole u64 words
            # (bucket_select stores them wave by wave)
            self.dirty = torch.zeros(2 * max((p.vp + 63) // 64, 1),
                                     dtype=U32, device=device)
            # device-resident limit: captured bodies replay across buckets
            self._limit_dev = torch.zeros(1, dtype=U32, device=device)
            # per-iteration preset of meta[6..7] (min deferred label,
            # deferred count), copied D2D like _hdr_zero
            self._meta67_init = torch.tensor([-1, 0], dtype=U32,
                                             device=device)
        self.reset(source)

    def reset(self, source=None):
        """(Re)initialise labels and the seed frontier
        (sssp_gpu.cu:733-744 / components_gpu.cu:733-740). Structures
        (CSRs, bins, buffers) are kept."""
        p = self.part
        if source is not None:
            self.source = source
        source = self.source
        if self.is_min:
            self.labels.fill_(-1)
            self.labels[source] = 0
        else:
            torch.arange(p.nv, dtype=U32, device=self.device,
                         out=self.labels)
        self.labels_part.copy_(self.labels.narrow(0, p.row_left, p.vp))
        self.labels_current = True

        if self._fq_init is None:
            fq_host = np.zeros(int(self.seg_off[-1]), np.uint8)
            meta0 = np.zeros((p.nparts, 8), np.uint32)
            for q in range(p.nparts):
                off = int(self.seg_off[q])
                hv = fq_host[off:off + 8].view(np.uint32)
                if self.is_min:
                    hv[0] = SPARSE_QUEUE
                    owner = (p.row_left_all[q] <= source
                             <= p.row_right_all[q]) if p.verts_all[q] \
                        else False
                    if owner:
                        hv[1] = 1
                        fq_host[off + 8:off + 12].view(np.uint32)[0] = source
                    meta0[q, 0] = SPARSE_QUEUE
                    meta0[q, 1] = hv[1]
                    # evol left 0: a 1-vertex seed frontier never flips the
                    # push-vs-pull decision
                else:
                    hv[0] = DENSE_BITMAP
                    hv[1] = p.verts_all[q]
                    nbytes = (p.verts_all[q] + 7) // 8
                    fq_host[off + 8:off + 8 + nbytes] = 0xFF
                    meta0[q, 0] = DENSE_BITMAP
                    meta0[q, 1] = p.verts_all[q]
            self._fq_init = (torch.from_numpy(fq_host).to(self.device),
                             meta0)
        self.fq_all.copy_(self._fq_init[0])
        self.fq_annex_all.zero_()  # seed labels are all 0 (SSSP source)
        self.meta_host = self._fq_init[1].copy()
        self.headers = [(int(self.meta_host[q, 0]),
                         int(self.meta_host[q, 1]))
                        for q in range(p.nparts)]
        self.iterations = 0
        self.stats = []
        self._bits_stale = True
        self.bucket_advances = 0
        if self.delta:
            # the seed is the active set (it sits in the segment); nothing
            # is deferred; snapshot == labels_part is the standing invariant
            self.dirty.zero_()
            self.snapshot.copy_(self.labels_part)
            self.meta_host[:, 6] = INF_LABEL
            self._set_limit(min(self.delta - 1, SAT_LABEL))

    # -------- helpers --------
    def _my_seg_i32(self):
        return self.new_seg.view(U32)

    def _sync_labels(self):
        """Catch-up all-gather of label slices (needed before a pull
        iteration or before reading the replicated labels) — slices go
        stale while sparse iterations skip the label exchange."""
        if self.labels_current:
            return
        p = self.part
        dx.all_gather_slices(self.labels, self.labels_part, p.verts_all,
                             p.row_left_all, my_index=p.p)
        self.labels_current = True

    def final_labels(self):
        """Replicated labels, synchronised (use after run())."""
        self._sync_labels()
        return self.labels

    def _scatter(self, s, new_dense, bits):
        """Chunk scatter over the expanded work items: the min-plus kernel
        on the interleaved CSR when weighted, else the hop / CC kernel."""
        p = self.part
        if self.weighted:
            ng.push_chunk_scatter_w(s, int(new_dense), self.items,
                                    self.item_counter, self.max_items,
                                    self.push_row_ptr, self.push_edge,
                                    self.labels, self.snapshot,
                                    self.labels_part, p.row_left,
                                    self.new_seg, self.capacity)
            return
        ng.push_chunk_scatter(s, int(self.is_min), int(new_dense),
                              self.items, self.item_counter,
                              self.max_items, self.push_row_ptr,
                              self.push_col, self.labels, self.snapshot,
                              self.labels_part, p.row_left,
                              self.new_seg, self.capacity,
                              visited_bits=bits)

    def _single_body(self, pull, new_dense):
        """One complete world-1 iteration body: compute + fixups + the
        device-side "exchange" (full-size self copies + meta). Every op
        has static shapes and fixed addresses -> hipGraph-capturable."""
        p = self.part
        s = _stream()
        self.snapshot.copy_(self.labels_part)
        self.new_seg[:8].copy_(self._hdr_zero)
        if pull:
            run_pull(p, self._pull_mode, self.labels, self.labels_part,
                     None, 0.0)
            counter = None
        else:
            self.item_counter.zero_()
            ng.frontier_expand_auto(s, p.vp, p.row_left, self.fq_all,
                                    self.fq_annex_all, self.labels,
                                    self.push_row_ptr, self.items,
                                    self.item_counter, self.max_items)
            bits = self.visited if self.visited is not None and p.vp > 0 \
                else None
            self._scatter(s, new_dense, bits)
            counter = self.item_counter
        if pull or new_dense:
            ng.build_bitmap(s, p.vp, self.snapshot, self.labels_part,
                            self.new_seg)
        ng.frontier_fixup(s, p.vp, p.row_left, self.capacity,
                          int(pull or new_dense), self.snapshot,
                          self.labels_part, self.deg_part, self.new_seg,
                          self.new_annex, self.tmp_seg, self.meta_mine,
                          counter, self.max_items)
        # world-1 "exchange": fixed-size self copies of the segment +
        # annex; the O(nv) label copy is device-predicated on the FINAL
        # type (sparse iterations skip it — the annex carries the queued
        # labels, exactly like the distributed label-skip)
        self.fq_all.copy_(self.new_seg)
        self.fq_annex_all[:self.capacity].copy_(self.new_annex)
        ng.publish_labels_guarded(s, p.vp, self.meta_mine,
                                  self.labels_part,
                                  self.labels.narrow(0, p.row_left, p.vp))

    def _run_single_body(self, pull, new_dense):
        key = ("pull",) if pull else ("push", bool(new_dense))
        self._run_captured(key,
                           lambda: self._single_body(pull, new_dense))

    def _run_captured(self, key, body):
        import os
        g = self._graphs.get(key)
        if g is not None:
            g.replay()
            return
        uses = self._graph_uses.get(key, 0) + 1
        self._graph_uses[key] = uses
        if (uses >= 2 and os.environ.get("LUX_HIPGRAPH", "1") == "1"
                and not os.environ.get("LUX_SYNC_CHECK")):
            try:
                torch.cuda.synchronize()
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg):
                    body()
                self._graphs[key] = cg
                cg.replay()  # capture records, doesn't run
                return
            except Exception as e:  # capture unsupported: stay eager
                print(f"[lux] push hipGraph capture disabled: {e}")
                os.environ["LUX_HIPGRAPH"] = "0"
                torch.cuda.synchronize()
        body()

    def _step_single(self):
        """World-1 fast path: replay the captured iteration graph, then
        ONE 32-byte meta read."""
        p = self.part
        mh = self.meta_host
        evol = int((mh[:, 2].astype(np.uint64)
                    | (mh[:, 3].astype(np.uint64) << np.uint64(32))).sum())
        overflow = bool(mh[:, 4].any())
        old_fq_size = int(mh[:, 1].sum())
        new_dense = int(mh[0, 0]) == DENSE_BITMAP
        pull = overflow or old_fq_size > p.nv // 16
        if overflow:
            print("[lux] frontier expand overflow: recovering with a "
                  "forced pull iteration", file=sys.stderr)
        if not pull:
            import os
            div = int(os.environ.get("LUX_PUSH_EVOL_DIV", "0") or 0)
            thresh = p.ne // div if div else (
                p.ne // 2 if self.visited is not None else p.ne // 8)
            if evol > thresh:
                pull = True
            elif (evol * p.ep // max(p.ne, 1)) // 16 > self.capacity:
                new_dense = True
        if pull and not self.labels_current:
            # catch up the replicated labels before the pull sweep (the
            # guarded publish skipped them on sparse iterations)
            self.labels.narrow(0, p.row_left, p.vp).copy_(self.labels_part)
            self.labels_current = True
        if not pull and self.visited is not None and p.vp > 0 \
                and self._bits_stale:
            ng.bits_from_labels(_stream(), p.vp, self.labels_part,
                                self.visited)
            self._bits_stale = False
        self._run_single_body(pull, new_dense)
        if pull:
            self._bits_stale = True
        mh = self.meta_mine.cpu().numpy().view(np.uint32).reshape(1, 8)
        self.meta_host = mh
        self.labels_current = int(mh[0, 0]) == DENSE_BITMAP
        self.headers = [(int(mh[0, 0]), int(mh[0, 1]))]
        self.iterations += 1
        self.stats.append(dict(iter=self.iterations,
                               old_frontier=old_fq_size,
                               pull_fallback=bool(pull),
                               out_dense=bool(mh[0, 0] == DENSE_BITMAP),
                               my_new=int(mh[0, 1])))
        return int(mh[0, 1])

    def step(self):
        """One push iteration. Returns the global new-frontier count
        (from the exchanged meta — no extra sync)."""
        p = self.part
        s = _stream()
        nparts = p.nparts
        ws = dx.world_size()
        if ws == 1 and nparts == 1:
            return self._step_single_bucketed() if self.delta \
                else self._step_single()
        if self.delta:
            return self._step_multi_bucketed()
        mh = self.meta_host  # (nparts, 8) u32 describing CURRENT frontier
        types = mh[:, 0]
        counts = mh[:, 1]
        evol = int((mh[:, 2].astype(np.uint64)
                    | (mh[:, 3].astype(np.uint64) << np.uint64(32))).sum())
        overflow = bool(mh[:, 4].any())
        old_fq_size = int(counts.sum())
        dense_votes = int((types == DENSE_BITMAP).sum())
        new_dense = dense_votes >= nparts - dense_votes
        self.snapshot.copy_(self.labels_part)
        # zero my new header (type patched by the device fixup chain)
        self.new_seg[:8].copy_(self._hdr_zero)

        pull_fallback = overflow or old_fq_size > p.nv // 16
        if overflow:
            print("[lux] frontier expand overflow: recovering with a "
                  "forced pull iteration", file=sys.stderr)
        if not pull_fallback:
            # second adaptivity axis (ours, not the reference's): the
            # vertex-count threshold misses RMAT's hub explosion — a 902K-
            # vertex frontier can cover ~half of all edges. The meta
            # record prices the frontier's out-edges exactly (global
            # out-degrees, accumulated at frontier build time); a dense
            # pull sweep (src-blocked LLC-resident gathers) is faster
            # beyond ~ne/8 edges. bitmap-BFS push touches vp/8 bytes of
            # visited bits instead of the label array, so it stays cheaper
            # up to much larger frontiers (~ne/2).
            import os
            div = int(os.environ.get("LUX_PUSH_EVOL_DIV", "0") or 0)
            thresh = p.ne // div if div else (
                p.ne // 2 if self.visited is not None else p.ne // 8)
            if evol > thresh:
                pull_fallback = True
            elif (evol * p.ep // max(p.ne, 1)) // 16 > self.capacity:
                # expected discoveries cannot fit the sparse queue: choose
                # the dense bitmap upfront instead of paying the sparse
                # append machinery + guaranteed overflow rebuild (the
                # reference always votes by input formats, sssp_gpu.cu:408)
                new_dense = True
        if pull_fallback:
            new_dense = True
            self._sync_labels()  # pull reads every vertex's label
            run_pull(p, self._pull_mode, self.labels, self.labels_part,
                     None, 0.0)
            self._bits_stale = True  # pull writes labels directly
            item_counter = None
        else:
            # expand all source segments into <=8192-edge work items;
            # sparse queues carry a label annex — expand repairs the
            # (possibly stale) replicated labels from it before the
            # scatter reads them
            self.item_counter.zero_()
            self._expand_segments(s, types, counts)
            bits = None
            if self.visited is not None and p.vp > 0:
                if self._bits_stale:
                    ng.bits_from_labels(s, p.vp, self.labels_part,
                                        self.visited)
                    self._bits_stale = False
                bits = self.visited
            self._scatter(s, new_dense, bits)
            item_counter = self.item_counter

        # ---- frontier fix-ups + meta, all device-side ----
        if new_dense:
            ng.build_bitmap(s, p.vp, self.snapshot, self.labels_part,
                            self.new_seg)
        ng.frontier_fixup(s, p.vp, p.row_left, self.capacity,
                          int(new_dense), self.snapshot, self.labels_part,
                          self.deg_part, self.new_seg, self.new_annex,
                          self.tmp_seg, self.meta_mine, item_counter,
                          self.max_items)

        mh = self._exchange()
        ntypes, ncounts = mh[:, 0], mh[:, 1]
        me = p.p
        self.iterations += 1
        # per-iteration trace row (reference -verbose parity,
        # sssp_gpu.cu:516-518: activeNodes + phase info per partition)
        my_new = int(ncounts[me])
        self.stats.append(dict(iter=self.iterations,
                               old_frontier=old_fq_size,
                               pull_fallback=bool(pull_fallback),
                               out_dense=bool(ntypes[me] == DENSE_BITMAP),
                               my_new=my_new))
        return int(ncounts.sum())

    def _expand_segments(self, s, types, counts):
        """Expand every source segment into work items (item_counter is
        zeroed by the caller)."""
        p = self.part
        # repair even at ws==1: sparse iterations skip the label
        # publish, so the replicated array is stale for exactly the
        # queued vertices — the annex carries their fresh labels
        repair = self.labels
        for q in range(p.nparts):
            typ, num = int(types[q]), int(counts[q])
            if p.verts_all[q] == 0:
                continue
            seg = self.fq_all.narrow(0, int(self.seg_off[q]),
                                     self.seg_bytes[q])
            if typ == DENSE_BITMAP:
                ng.frontier_expand(s, 1, p.row_left_all[q],
                                   p.verts_all[q], seg, None, None,
                                   self.push_row_ptr, self.items,
                                   self.item_counter, self.max_items)
            elif num:
                annex = self.fq_annex_all.narrow(
                    0, int(self.annex_off[q]), num)
                ng.frontier_expand(s, 0, 0, num, seg, annex, repair,
                                   self.push_row_ptr, self.items,
                                   self.item_counter, self.max_items)

    def _exchange(self):
        """Meta first (the ONE host read), then the payloads it sizes.
        Updates meta_host, headers and label freshness; returns the meta
        table."""
        p = self.part
        nparts = p.nparts
        dx.all_gather_slices(self.meta_all, self.meta_mine,
                             [8] * nparts, [8 * q for q in range(nparts)],
                             my_index=p.p)
        mh = self.meta_all.cpu().numpy().view(np.uint32).reshape(nparts, 8)
        self.meta_host = mh
        ntypes, ncounts = mh[:, 0], mh[:, 1]

        # payload exchange from the fresh meta: only USED bytes travel
        me = p.p
        h, _ = exchange_frontier_payloads(
            mh, p.verts_all, self.fq_all, self.new_seg,
            [int(o) for o in self.seg_off[:-1]], self.fq_annex_all,
            self.new_annex, [int(o) for o in self.annex_off[:-1]],
            self.labels, self.labels_part, p.row_left_all, me)
        h.wait()
        # slice q is fresh iff q published it now, or it was fresh before
        # and q changed nothing this iteration. Bucketed: a rank can change
        # labels and defer them all (new count 0), so only a published
        # slice counts; _sync_labels() before a pull does the catch-up
        self.labels_current = self._labels_fresh(self.labels_current, mh)

        self.headers = [(int(ntypes[q]), int(ncounts[q]))
                        for q in range(nparts)]
        return mh

    def _labels_fresh(self, was_fresh, mh):
        """Are all replicated label slices fresh after the exchange that
        meta table `mh` sized? Dense ranks published theirs."""
        p = self.part
        for q in range(p.nparts):
            if p.verts_all[q] == 0 or int(mh[q, 0]) == DENSE_BITMAP:
                continue
            if self.delta or not was_fresh or int(mh[q, 1]) != 0:
                return False
        return True

    # -------- bucketed schedule (near-far delta-stepping) --------
    # State: labels; `dirty`, the bitmap of vertices that improved since
    # they last relaxed their out-edges and lie beyond the limit (the
    # deferred set — the near ones are the active set and sit in the
    # frontier segment, so nothing is ever queued twice); `limit`, a global
    # u32 (near <=> label <= limit), device-resident so captured bodies
    # replay across buckets.
    #   relax   push: out-edges of the active set A, then
    #                 dirty = (dirty \ A) | changed
    #           pull: every edge (the plain rule applied to A), then
    #                 dirty = changed
    #   select  ng.bucket_select splits dirty into the next A (dense
    #           bitmap, finished by frontier_fixup(built_dense=1) as usual)
    #           and the deferred rest; meta[6] = min deferred label,
    #           meta[7] = deferred count
    #   advance A empty, deferred not: limit jumps to the end of the bucket
    #           holding the global min deferred label, select again. No
    #           edge is relaxed; counted in bucket_advances, not iterations
    # snapshot == labels_part holds between iterations: select refreshes
    # the snapshot where it saw a change, replacing the per-iteration copy.

    def _set_limit(self, limit):
        self.limit = int(limit)
        # U32 buffers are torch.int32: pass the same 32 bits
        self._limit_dev.fill_(self.limit - (1 << 32)
                              if self.limit >= 1 << 31 else self.limit)

    def _seed_volume(self):
        """Global out-degree of the source (stats only: the decision leaves
        the seed unpriced). Read once per source."""
        p = self.part
        cache = self._seed_vols
        if self.source not in cache:
            mine = p.vp > 0 and p.row_left <= self.source <= p.row_right
            v = self.deg_part.narrow(0, self.source - p.row_left, 1).to(U64) \
                if mine else torch.zeros(1, dtype=U64, device=self.device)
            dx.all_reduce_sum_(v)
            cache[self.source] = int(v.item()) & 0xFFFFFFFF
        return cache[self.source]

    def _bucket_decide(self):
        """(active count, its out-edge volume, overflow, pull) from the
        meta table of the current active set — the plain engine's rule."""
        import os
        p = self.part
        mh = self.meta_host
        evol = int((mh[:, 2].astype(np.uint64)
                    | (mh[:, 3].astype(np.uint64) << np.uint64(32))).sum())
        overflow = bool(mh[:, 4].any())
        active = int(mh[:, 1].sum())
        pull = overflow or active > p.nv // 16
        if overflow:
            print("[lux] frontier expand overflow: recovering with a "
                  "forced pull iteration", file=sys.stderr)
        if not pull:
            div = int(os.environ.get("LUX_PUSH_EVOL_DIV", "0") or 0)
            pull = evol > (p.ne // div if div else p.ne // 8)
        return active, evol, overflow, pull

    def needs_advance(self):
        """No near vertex left but deferred ones are (and no overflow
        pending: the forced pull comes first)."""
        mh = self.meta_host
        return bool(self.delta) and int(mh[:, 1].sum()) == 0 \
            and int(mh[:, 7].sum()) > 0 and not mh[:, 4].any()

    def _bucket_row(self, active, evol, pull, limit):
        mh = self.meta_host
        me = self.part.p if mh.shape[0] > 1 else 0
        if self.iterations == 1:
            evol = self._seed_volume()
        self.stats.append(dict(iter=self.iterations, old_frontier=active,
                               pull_fallback=bool(pull),
                               out_dense=bool(mh[me, 0] == DENSE_BITMAP),
                               my_new=int(mh[me, 1]), limit=limit,
                               volume=evol,
                               deferred=int(mh[:, 7].sum())))

    def _bucket_prologue(self):
        """Capturable per-iteration presets: zero my new header, reset the
        deferred min / count words of the meta record."""
        self.new_seg[:8].copy_(self._hdr_zero)
        self.meta_mine[6:8].copy_(self._meta67_init)

    def _bucket_select_fixup(self, s, replace, counter):
        p = self.part
        ng.bucket_select(s, p.vp, self.snapshot, self.labels_part,
                         self.dirty, self._limit_dev, replace, self.new_seg,
                         self.meta_mine)
        ng.frontier_fixup(s, p.vp, p.row_left, self.capacity, 1,
                          self.snapshot, self.labels_part, self.deg_part,
                          self.new_seg, self.new_annex, self.tmp_seg,
                          self.meta_mine, counter, self.max_items)

    def _bucket_body(self, kind):
        """World-1 bucketed body, kind = "pull" | "push" | "select" (the
        advance's reselect). Static shapes and addresses: capturable."""
        p = self.part
        s = _stream()
        self._bucket_prologue()
        counter = None
        if kind == "pull":
            run_pull(p, self._pull_mode, self.labels, self.labels_part,
                     None, 0.0)
        elif kind == "push":
            self.item_counter.zero_()
            ng.frontier_expand_auto(s, p.vp, p.row_left, self.fq_all,
                                    self.fq_annex_all, self.labels,
                                    self.push_row_ptr, self.items,
                                    self.item_counter, self.max_items)
            self._scatter(s, True, None)  # label atomics only, no enqueue
            counter = self.item_counter
        self._bucket_select_fixup(s, kind == "pull", counter)
        self.fq_all.copy_(self.new_seg)
        self.fq_annex_all[:self.capacity].copy_(self.new_annex)
        ng.publish_labels_guarded(s, p.vp, self.meta_mine,
                                  self.labels_part,
                                  self.labels.narrow(0, p.row_left, p.vp))

    def _run_bucket_single(self, kind):
        self._run_captured(("bucket", kind),
                           lambda: self._bucket_body(kind))
        mh = self.meta_mine.cpu().numpy().view(np.uint32).reshape(1, 8)
        self.meta_host = mh
        self.labels_current = int(mh[0, 0]) == DENSE_BITMAP
        self.headers = [(int(mh[0, 0]), int(mh[0, 1]))]

    def advance(self):
        """Bucket advance: move the limit to the end of the bucket that
        holds the global minimum deferred label and select again (select +
        fixup + the usual exchange, no relaxation). Every rank computes
        the same limit from the exchanged meta table."""
        p = self.part
        m = int(self.meta_host[:, 6].min())
        self._set_limit(min((m // self.delta + 1) * self.delta - 1,
                            SAT_LABEL))
        self.bucket_advances += 1
        if dx.world_size() == 1 and p.nparts == 1:
            self._run_bucket_single("select")
            return
        self._bucket_prologue()
        self._bucket_select_fixup(_stream(), False, None)
        self._exchange()

    def _step_single_bucketed(self):
        p = self.part
        if self.needs_advance():
            self.advance()
        active, evol, _, pull = self._bucket_decide()
        limit = self.limit
        if pull and not self.labels_current:
            self.labels.narrow(0, p.row_left, p.vp).copy_(self.labels_part)
            self.labels_current = True
        self._run_bucket_single("pull" if pull else "push")
        self.iterations += 1
        self._bucket_row(active, evol, pull, limit)
        return int(self.meta_host[0, 1])

    def _step_multi_bucketed(self):
        p = self.part
        s = _stream()
        if self.needs_advance():
            self.advance()
        mh = self.meta_host
        active, evol, _, pull = self._bucket_decide()
        limit = self.limit
        self._bucket_prologue()
        if pull:
            self._sync_labels()  # pull reads every vertex's label
            run_pull(p, self._pull_mode, self.labels, self.labels_part,
                     None, 0.0)
            counter = None
        else:
            self.item_counter.zero_()
            self._expand_segments(s, mh[:, 0], mh[:, 1])
            self._scatter(s, True, None)
            counter = self.item_counter
        self._bucket_select_fixup(s, pull, counter)
        mh = self._exchange()
        self.iterations += 1
        self._bucket_row(active, evol, pull, limit)
        return int(mh[:, 1].sum())

    def run(self, max_iters=None):
        """Iterate to convergence (every partition reports an empty new
        frontier; bucketed: and an empty deferred set)."""
        while True:
            total = self.step()
            if total == 0 and not self.meta_host[:, 4].any() \
                    and not (self.delta and self.meta_host[:, 7].any()):
                break  # overflow never terminates: forced pull recovers
            if max_iters and self.iterations >= max_iters:
                break
        self._sync_labels()
        return self.iterations

    def check(self):
        """Device check oracle; returns global violation count."""
        p = self.part
        self._sync_labels()
        mistakes = torch.zeros(1, dtype=U64, device=self.device)
        if self.weighted:
            ng.check_w(_stream(), p.vp, p.row_left, p.row_ptr, p.col,
                       p.weight, self.labels, self.source, mistakes)
        else:
            ng.check(_stream(), int(self.is_min), p.vp, p.row_left,
                     p.row_ptr, p.col, self.labels, mistakes)
        dx.all_reduce_sum_(mistakes)
        return int(mistakes.cpu().item())
