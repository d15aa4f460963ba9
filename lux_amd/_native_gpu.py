"""ctypes bindings for liblux_gpu.so (gfx950 HIP kernels).

All device pointers are passed as raw integers (torch `Tensor.data_ptr()`),
streams as `torch.cuda.current_stream().cuda_stream`. Dtype mapping:
u32 buffers <-> torch.int32, u64/E_ID <-> torch.int64, f32 <-> torch.float32
(bit-compatible; the native side interprets unsigned).

Every entry point raises if the library is missing — GPU paths must fail
loudly rather than fall back to eager/CPU silently.
"""
import ctypes
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_DIR, "liblux_gpu.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            raise RuntimeError(
                "liblux_gpu.so not built — run `python build.py --gpu` "
                "(the HIP extension is mandatory on GPU boxes; no fallback)")
        _lib = ctypes.CDLL(_PATH)
        _lib.lux_gpu_scan_partials_size.restype = ctypes.c_uint32
    return _lib


def dp(t):
    """torch tensor (or raw int device address) -> c_void_p."""
    if t is None:
        return ctypes.c_void_p(0)
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.data_ptr())


def _u64(x):
    return ctypes.c_uint64(int(x))


def _u32(x):
    return ctypes.c_uint32(int(x))


def rmat_edges(stream, seed, scale, ne, src, dst):
    lib().lux_gpu_rmat_edges(_u64(stream), _u64(seed), ctypes.c_int(scale),
                             _u64(ne), dp(src), dp(dst))


def rmat_edges_chunk(stream, seed, scale, e0, ne, src, dst):
    lib().lux_gpu_rmat_edges_chunk(_u64(stream), _u64(seed),
                                   ctypes.c_int(scale), _u64(e0), _u64(ne),
                                   dp(src), dp(dst))


def rmat_edges_folded(stream, seed, scale, nv, ne, src, dst):
    lib().lux_gpu_rmat_edges_folded(_u64(stream), _u64(seed),
                                    ctypes.c_int(scale), _u32(nv), _u64(ne),
                                    dp(src), dp(dst))


def rmat_edges_folded_chunk(stream, seed, scale, nv, e0, ne, src, dst):
    lib().lux_gpu_rmat_edges_folded_chunk(
        _u64(stream), _u64(seed), ctypes.c_int(scale), _u32(nv), _u64(e0),
        _u64(ne), dp(src), dp(dst))


def bipartite_edges_chunk(stream, seed, n_users, n_items, e0, ne, src, dst,
                          w):
    lib().lux_gpu_bipartite_edges_chunk(
        _u64(stream), _u64(seed), _u32(n_users), _u32(n_items), _u64(e0),
        _u64(ne), dp(src), dp(dst), dp(w))


def slice_scatter(stream, n, src, dst, w, rl, rr, cursor, out_col, out_w):
    lib().lux_gpu_slice_scatter(_u64(stream), _u64(n), dp(src), dp(dst),
                                dp(w), _u32(rl), _u32(rr), dp(cursor),
                                dp(out_col), dp(out_w))


def cf_iter(stream, n0, bin0, n1, bin1, n2, bin2, nbig, bin2v, row_ptr, col,
            w, oldv, newv, row_left, K):
    lib().lux_gpu_cf_iter(_u64(stream), _u32(n0), dp(bin0), _u32(n1),
                          dp(bin1), _u32(n2), dp(bin2), _u32(nbig), dp(bin2v),
                          dp(row_ptr), dp(col), dp(w), dp(oldv), dp(newv),
                          _u32(row_left), ctypes.c_int(K))


def bipartite_edges(stream, seed, n_users, n_items, ne, src, dst, w):
    lib().lux_gpu_bipartite_edges(_u64(stream), _u64(seed), _u32(n_users),
                                  _u32(n_items), _u64(ne), dp(src), dp(dst),
                                  dp(w))


def hist_u32(stream, n, ids, hist):
    lib().lux_gpu_hist_u32(_u64(stream), _u64(n), dp(ids), dp(hist))


def scan_partials_size(n):
    return int(lib().lux_gpu_scan_partials_size(_u64(n)))


def scan_end_offsets(stream, n, inp, out_end, partials):
    lib().lux_gpu_scan_end_offsets(_u64(stream), _u64(n), dp(inp),
                                   dp(out_end), dp(partials))


def u64_to_u32(stream, n, inp, out):
    lib().lux_gpu_u64_to_u32(_u64(stream), _u64(n), dp(inp), dp(out))


def edges_to_csc(stream, nv, ne, src, dst, w, col_end, out_src, out_w, hist,
                 cursor, partials):
    lib().lux_gpu_edges_to_csc(_u64(stream), _u32(nv), _u64(ne), dp(src),
                               dp(dst), dp(w), dp(col_end), dp(out_src),
                               dp(out_w), dp(hist), dp(cursor), dp(partials))


def local_row_ptr(stream, vp, col_left, col_end_slice, row_ptr_loc):
    lib().lux_gpu_local_row_ptr(_u64(stream), _u32(vp), _u64(col_left),
                                dp(col_end_slice), dp(row_ptr_loc))


def build_bins(stream, vp, row_ptr, bin0, bin1, bin2, bin2v, counters):
    lib().lux_gpu_build_bins(_u64(stream), _u32(vp), dp(row_ptr), dp(bin0),
                             dp(bin1), dp(bin2), dp(bin2v), dp(counters))


def csr_scatter(stream, ep, col, row_ptr_loc, vp, row_left, cursor,
                push_col):
    lib().lux_gpu_csr_scatter(_u64(stream), _u64(ep), dp(col),
                              dp(row_ptr_loc), _u32(vp), _u32(row_left),
                              dp(cursor), dp(push_col))


def build_bitmap(stream, vp, snapshot, new_labels, seg):
    lib().lux_gpu_build_bitmap(_u64(stream), _u32(vp), dp(snapshot),
                               dp(new_labels), dp(seg))


def d2s(stream, vp, row_left, dense_seg, sparse_seg):
    lib().lux_gpu_d2s(_u64(stream), _u32(vp), _u32(row_left), dp(dense_seg),
                      dp(sparse_seg))


def check(stream, is_min, vp, row_left, row_ptr_loc, col, labels, mistakes):
    lib().lux_gpu_check(_u64(stream), ctypes.c_int(is_min), _u32(vp),
                        _u32(row_left), dp(row_ptr_loc), dp(col), dp(labels),
                        dp(mistakes))


PULL_PR = 0
PULL_MIN = 1
PULL_MAX = 2


def pull_iter(stream, mode, n0, bin0, n1, bin1, n2, bin2, nbig, bin2v,
              row_ptr, col, oldv, newv, deg, row_left, init_rank,
              row_u32=0):
    lib().lux_gpu_pull_iter(_u64(stream), ctypes.c_int(mode), _u32(n0),
                            dp(bin0), _u32(n1), dp(bin1), _u32(n2), dp(bin2),
                            _u32(nbig), dp(bin2v), dp(row_ptr),
                            ctypes.c_int(row_u32), dp(col),
                            dp(oldv), dp(newv), dp(deg), _u32(row_left),
                            ctypes.c_float(init_rank))


def blocked_count(stream, ep, col, row_ptr_loc, vp, bounds, nb, counts,
                  lo=0, hi=0xFFFFFFFF):
    lib().lux_gpu_blocked_count(_u64(stream), _u64(ep), dp(col),
                                dp(row_ptr_loc), _u32(vp), dp(bounds),
                                ctypes.c_int(nb), _u32(lo), _u32(hi),
                                dp(counts))


def blocked_scatter(stream, ep, col, row_ptr_loc, vp, bounds, nb, cursor,
                    out_col, lo=0, hi=0xFFFFFFFF):
    lib().lux_gpu_blocked_scatter(_u64(stream), _u64(ep), dp(col),
                                  dp(row_ptr_loc), _u32(vp), dp(bounds),
                                  ctypes.c_int(nb), _u32(lo), _u32(hi),
                                  dp(cursor), dp(out_col))


PULL_MIN_W = 4  # weighted SSSP (min-plus); served by pull_iter_w


def pull_iter_w(stream, n0, bin0, n1, bin1, n2, bin2, nbig, bin2v, row_ptr,
                col, wgt, oldv, newv, row_left, row_u32=0):
    """Weighted SSSP dense sweep: wgt[j] is the weight of edge col[j]."""
    lib().lux_gpu_pull_iter_w(_u64(stream), _u32(n0), dp(bin0), _u32(n1),
                              dp(bin1), _u32(n2), dp(bin2), _u32(nbig),
                              dp(bin2v), dp(row_ptr), ctypes.c_int(row_u32),
                              dp(col), dp(wgt), dp(oldv), dp(newv),
                              _u32(row_left))


def blocked_scatter_w(stream, ep, col, weight, row_ptr_loc, vp, bounds, nb,
                      cursor, out_col, out_w, lo=0, hi=0xFFFFFFFF):
    lib().lux_gpu_blocked_scatter_w(_u64(stream), _u64(ep), dp(col),
                                    dp(weight), dp(row_ptr_loc), _u32(vp),
                                    dp(bounds), ctypes.c_int(nb), _u32(lo),
                                    _u32(hi), dp(cursor), dp(out_col),
                                    dp(out_w))


def hash_weights(stream, ep, col, row_ptr_loc, vp, row_left, seed, wmax,
                 weight):
    lib().lux_gpu_hash_weights(_u64(stream), _u64(ep), dp(col),
                               dp(row_ptr_loc), _u32(vp), _u32(row_left),
                               _u64(seed), _u32(wmax), dp(weight))


def csr_scatter_w(stream, ep, col, weight, row_ptr_loc, vp, row_left, cursor,
                  push_edge):
    lib().lux_gpu_csr_scatter_w(_u64(stream), _u64(ep), dp(col), dp(weight),
                                dp(row_ptr_loc), _u32(vp), _u32(row_left),
                                dp(cursor), dp(push_edge))


def push_chunk_scatter_w(stream, new_dense, items, counter, max_items,
                         push_row_ptr, push_edge, old_labels, snapshot,
                         new_labels, my_row_left, new_seg, capacity):
    lib().lux_gpu_push_chunk_scatter_w(
        _u64(stream), ctypes.c_int(new_dense), dp(items), dp(counter),
        _u32(max_items), dp(push_row_ptr), dp(push_edge), dp(old_labels),
        dp(snapshot), dp(new_labels), _u32(my_row_left), dp(new_seg),
        _u32(capacity))


def check_w(stream, vp, row_left, row_ptr_loc, col, weight, labels, source,
            mistakes):
    lib().lux_gpu_check_w(_u64(stream), _u32(vp), _u32(row_left),
                          dp(row_ptr_loc), dp(col), dp(weight), dp(labels),
                          _u32(source), dp(mistakes))


def bucket_select(stream, vp, snapshot, labels_part, dirty, limit, replace,
                  seg, meta):
    """Bucketed-schedule select pass (push.hip bucket_select_kernel). The
    kernel stores whole u64 words: dirty needs 2 * ceil(vp / 64) u32 words
    and seg 8 + 8 * ceil(vp / 64) bytes, checked here because a short
    buffer would be written past its end."""
    words = (int(vp) + 63) // 64
    if not isinstance(dirty, int) and dirty is not None:
        assert dirty.numel() * dirty.element_size() >= 8 * words, \
            "bucket_select: dirty shorter than 2 * ceil(vp / 64) u32 words"
    if not isinstance(seg, int) and seg is not None:
        assert seg.numel() * seg.element_size() >= 8 + 8 * words, \
            "bucket_select: seg shorter than 8 + 8 * ceil(vp / 64) bytes"
    lib().lux_gpu_bucket_select(_u64(stream), _u32(vp), dp(snapshot),
                                dp(labels_part), dp(dirty), dp(limit),
                                ctypes.c_int(int(bool(replace))), dp(seg),
                                dp(meta))


def pull_finish_pr(stream, vp, newv, deg, row_left, init_rank):
    lib().lux_gpu_pull_finish_pr(_u64(stream), _u32(vp), dp(newv), dp(deg),
                                 _u32(row_left), ctypes.c_float(init_rank))


def pull_active_flags(stream, vp, row_ptr, flags):
    lib().lux_gpu_pull_active_flags(_u64(stream), _u32(vp), dp(row_ptr),
                                    dp(flags))


def pull_active_list(stream, vp, flags, ends, active):
    lib().lux_gpu_pull_active_list(_u64(stream), _u32(vp), dp(flags),
                                   dp(ends), dp(active))


def pull_build_slots(stream, n, bin_, row_ptr, row_u32, ends, cidx, rng):
    lib().lux_gpu_pull_build_slots(_u64(stream), _u32(n), dp(bin_),
                                   dp(row_ptr), ctypes.c_int(row_u32),
                                   dp(ends), dp(cidx), dp(rng))


def pull_build_hub_slots(stream, n2, bin2, row_ptr, row_u32, ends, cidx,
                         rng):
    lib().lux_gpu_pull_build_hub_slots(_u64(stream), _u32(n2), dp(bin2),
                                       dp(row_ptr), ctypes.c_int(row_u32),
                                       dp(ends), dp(cidx), dp(rng))


def pull_slots_iter(stream, n0, cidx0, rng0, n1, cidx1, rng1, n2, cidx2,
                    rng2, col, oldv, acc):
    lib().lux_gpu_pull_slots_iter(_u64(stream), _u32(n0), dp(cidx0),
                                  dp(rng0), _u32(n1), dp(cidx1), dp(rng1),
                                  _u32(n2), dp(cidx2), dp(rng2), dp(col),
                                  dp(oldv), dp(acc))


def pull_slot_counts(stream, n, rng, cnt):
    lib().lux_gpu_pull_slot_counts(_u64(stream), _u32(n), dp(rng), dp(cnt))


def pull_stream_copy(stream, n0, rng0, off0, col, scol0):
    lib().lux_gpu_pull_stream_copy(_u64(stream), _u32(n0), dp(rng0),
                                   dp(off0), dp(col), dp(scol0))


def pull_stream_tile_counts(stream, n0, off0, cnt):
    lib().lux_gpu_pull_stream_tile_counts(_u64(stream), _u32(n0), dp(off0),
                                          dp(cnt))


def pull_stream_tile_fill(stream, n0, off0, ends, tile0):
    lib().lux_gpu_pull_stream_tile_fill(_u64(stream), _u32(n0), dp(off0),
                                        dp(ends), dp(tile0))


def pull_slots_stream_iter(stream, n0, cidx0, nt, tile0, off0, scol0, n1,
                           cidx1, rng1, n2, cidx2, rng2, col, oldv, acc):
    lib().lux_gpu_pull_slots_stream_iter(
        _u64(stream), _u32(n0), dp(cidx0), _u32(nt), dp(tile0), dp(off0),
        dp(scol0), _u32(n1), dp(cidx1), dp(rng1), _u32(n2), dp(cidx2),
        dp(rng2), dp(col), dp(oldv), dp(acc))


def pull_finish_pr_active(stream, na, active, acc, out, deg, row_left,
                          init_rank):
    lib().lux_gpu_pull_finish_pr_active(_u64(stream), _u32(na), dp(active),
                                        dp(acc), dp(out), dp(deg),
                                        _u32(row_left),
                                        ctypes.c_float(init_rank))


def pull_hot_col(stream, n, col, pos, hcol):
    lib().lux_gpu_pull_hot_col(_u64(stream), _u64(n), dp(col), dp(pos),
                               dp(hcol))


def pull_stream_copy_hot(stream, n0, rng0, off0, col, pos, scol0):
    lib().lux_gpu_pull_stream_copy_hot(_u64(stream), _u32(n0), dp(rng0),
                                       dp(off0), dp(col), dp(pos), dp(scol0))


def pull_hot_apos(stream, na, active, pos, deg, row_left, apos):
    lib().lux_gpu_pull_hot_apos(_u64(stream), _u32(na), dp(active), dp(pos),
                                dp(deg), _u32(row_left), dp(apos))


def pull_hot_scatter(stream, nv, pos, old, gold):
    lib().lux_gpu_pull_hot_scatter(_u64(stream), _u32(nv), dp(pos), dp(old),
                                   dp(gold))


def pull_finish_pr_active_hot(stream, na, active, apos, acc, out, gold, deg,
                              row_left, init_rank):
    lib().lux_gpu_pull_finish_pr_active_hot(
        _u64(stream), _u32(na), dp(active), dp(apos), dp(acc), dp(out),
        dp(gold), dp(deg), _u32(row_left), ctypes.c_float(init_rank))


def pull_slots_stream_hot_iter(stream, n0, cidx0, nt, tile0, off0, scol0, n1,
                               cidx1, rng1, n2, cidx2, rng2, col, gold, acc,
                               lo, hi, k):
    rc = lib().lux_gpu_pull_slots_stream_hot_iter(
        _u64(stream), _u32(n0), dp(cidx0), _u32(nt), dp(tile0), dp(off0),
        dp(scol0), _u32(n1), dp(cidx1), dp(rng1), _u32(n2), dp(cidx2),
        dp(rng2), dp(col), dp(gold), dp(acc), _u32(lo), _u32(hi),
        ctypes.c_int(k))
    if rc != 0:
        raise ValueError(f"pull_slots_stream_hot_iter: unsupported k={k}")


def pull_slots_stream_hot_wide_iter(stream, n0, cidx0, nt, tile0, off0,
                                    scol0, n1, cidx1, rng1, n2, cidx2, rng2,
                                    col, gold, acc, lo, hi, ks, kw,
                                    max_groups=0):
    """scol0 / col are the tensors themselves: their lengths set the role
    split. max_groups: 0 = eight workgroups per CU."""
    rc = lib().lux_gpu_pull_slots_stream_hot_wide_iter(
        _u64(stream), _u32(n0), dp(cidx0), _u32(nt), dp(tile0), dp(off0),
        dp(scol0), _u64(0 if scol0 is None else scol0.numel()), _u32(n1),
        dp(cidx1), dp(rng1), _u32(n2), dp(cidx2), dp(rng2), dp(col),
        _u64(col.numel()), dp(gold), dp(acc), _u32(lo), _u32(hi),
        ctypes.c_int(ks), ctypes.c_int(kw), _u32(max_groups))
    if rc == -1:
        raise ValueError("pull_slots_stream_hot_wide_iter: unsupported "
                         f"(ks, kw)=({ks}, {kw})")
    if rc != 0:
        raise RuntimeError("pull_slots_stream_hot_wide_iter: the runtime "
                           "refused the CU count or the LDS size")


def pull_fill_inactive_pr(stream, vp, row_ptr, out, deg, row_left,
                          init_rank):
    lib().lux_gpu_pull_fill_inactive_pr(_u64(stream), _u32(vp), dp(row_ptr),
                                        dp(out), dp(deg), _u32(row_left),
                                        ctypes.c_float(init_rank))


def cf_als_iter(stream, n0, bin0, n1, bin1, n2, bin2, nbig, bin2v, hubidx,
                gram_scratch, rhs_scratch, row_ptr, col, w, oldv, newv,
                row_left, K, oldv_bf=None):
    lib().lux_gpu_cf_als_iter(
        _u64(stream), _u32(n0), dp(bin0), _u32(n1), dp(bin1), _u32(n2),
        dp(bin2), _u32(nbig), dp(bin2v), dp(hubidx), dp(gram_scratch),
        dp(rhs_scratch), dp(row_ptr), dp(col), dp(w), dp(oldv), dp(oldv_bf),
        dp(newv), _u32(row_left), ctypes.c_int(K))


def frontier_expand(stream, old_dense, in_row_left, in_count, old_seg,
                    qlabels, labels_repair, push_row_ptr, items, counter,
                    max_items):
    lib().lux_gpu_frontier_expand(
        _u64(stream), ctypes.c_int(old_dense), _u32(in_row_left),
        _u32(in_count), dp(old_seg), dp(qlabels), dp(labels_repair),
        dp(push_row_ptr), dp(items), dp(counter), _u32(max_items))


def frontier_expand_auto(stream, verts, in_row_left, seg, qlabels,
                         labels_repair, push_row_ptr, items, counter,
                         max_items):
    lib().lux_gpu_frontier_expand_auto(
        _u64(stream), _u32(verts), _u32(in_row_left), dp(seg), dp(qlabels),
        dp(labels_repair), dp(push_row_ptr), dp(items), dp(counter),
        _u32(max_items))


def frontier_fixup(stream, vp, row_left, capacity, built_dense, snapshot,
                   labels_part, deg_part, new_seg, annex, tmp_seg, meta,
                   item_counter, max_items):
    """Device-predicated conversion chain + meta record (push.hip
    lux_gpu_frontier_fixup): zero host syncs."""
    lib().lux_gpu_frontier_fixup(
        _u64(stream), _u32(vp), _u32(row_left), _u32(capacity),
        ctypes.c_int(built_dense), dp(snapshot), dp(labels_part),
        dp(deg_part), dp(new_seg), dp(annex), dp(tmp_seg), dp(meta),
        dp(item_counter), _u32(max_items))


def push_chunk_scatter(stream, is_min, new_dense, items, counter, max_items,
                       push_row_ptr, push_col, old_labels, snapshot,
                       new_labels, my_row_left, new_seg, capacity,
                       visited_bits=None):
    lib().lux_gpu_push_chunk_scatter(
        _u64(stream), ctypes.c_int(is_min), ctypes.c_int(new_dense),
        dp(items), dp(counter), _u32(max_items), dp(push_row_ptr),
        dp(push_col), dp(old_labels), dp(snapshot), dp(new_labels),
        _u32(my_row_left), dp(new_seg), _u32(capacity), dp(visited_bits))


def publish_labels_guarded(stream, vp, meta, labels_part, labels_slice):
    lib().lux_gpu_publish_labels_guarded(_u64(stream), _u32(vp), dp(meta),
                                         dp(labels_part), dp(labels_slice))


def bits_from_labels(stream, vp, labels, bits):
    lib().lux_gpu_bits_from_labels(_u64(stream), _u32(vp), dp(labels),
                                   dp(bits))


def uf_union_star(stream, nv, star, parent):
    lib().lux_gpu_uf_union_star(_u64(stream), _u32(nv), dp(star), dp(parent))


def uf_flatten(stream, nv, parent, labels):
    lib().lux_gpu_uf_flatten(_u64(stream), _u32(nv), dp(parent), dp(labels))


def uf_union_binned(stream, n0, bin0, n1, bin1, n2, bin2, row_ptr, col,
                    row_left, parent, gbits=None):
    lib().lux_gpu_uf_union_binned(_u64(stream), _u32(n0), dp(bin0),
                                  _u32(n1), dp(bin1), _u32(n2), dp(bin2),
                                  dp(row_ptr), dp(col), _u32(row_left),
                                  dp(parent), dp(gbits))


def uf_union_kth(stream, vp, row_ptr, col, row_left, parent, k):
    lib().lux_gpu_uf_union_kth(_u64(stream), _u32(vp), dp(row_ptr), dp(col),
                               _u32(row_left), dp(parent), _u32(k))


def cc_giant_bits(stream, nv, labels, giant, bits):
    lib().lux_gpu_cc_giant_bits(_u64(stream), _u32(nv), dp(labels),
                                _u32(giant), dp(bits))


# ---- betweenness centrality (bc.hip) ----

def bc_init(stream, nv, source, depth, rec, sigma, delta):
    lib().lux_gpu_bc_init(_u64(stream), _u32(nv), _u32(source), dp(depth),
                          dp(rec), dp(sigma), dp(delta))


def bc_order_hist(stream, nv, depth, row_ptr, levels, cnt, hubrows):
    lib().lux_gpu_bc_order_hist(_u64(stream), _u32(nv), dp(depth),
                                dp(row_ptr), _u32(levels), dp(cnt),
                                dp(hubrows))


def bc_order_scatter(stream, nv, depth, row_ptr, levels, cursor, list_):
    lib().lux_gpu_bc_order_scatter(_u64(stream), _u32(nv), dp(depth),
                                   dp(row_ptr), _u32(levels), dp(cursor),
                                   dp(list_))


def bc_level(stream, forward, list_, o0, o1, o2, o3, row_ptr, adj, rec,
             sigma, delta, d, last, edges):
    """One level of the sigma (forward) or delta (backward) pass; o0..o3
    are the level's word offsets into the work list. `edges` is the address
    of one u64 counter."""
    lib().lux_gpu_bc_level(_u64(stream), ctypes.c_int(int(bool(forward))),
                           dp(list_), _u64(o0), _u64(o1), _u64(o2), _u64(o3),
                           dp(row_ptr), dp(adj), dp(rec), dp(sigma),
                           dp(delta), _u32(d), ctypes.c_int(int(bool(last))),
                           dp(edges))


def bc_check(stream, nv, source, in_ptr, in_adj, out_ptr, out_adj, depth,
             sigma, delta, rtol, out):
    lib().lux_gpu_bc_check(_u64(stream), _u32(nv), _u32(source), dp(in_ptr),
                           dp(in_adj), dp(out_ptr), dp(out_adj), dp(depth),
                           dp(sigma), dp(delta), ctypes.c_double(rtol),
                           dp(out))


# ---- triangle counting (tc.hip) ----

def tc_stage_max():
    """Largest staged-role cap (LDS entries) the kernels accept."""
    f = lib().lux_gpu_tc_stage_max
    f.restype = ctypes.c_uint32
    return int(f())


def tc_small_max():
    """Longest row (oriented arcs) the small role's kernel accepts."""
    f = lib().lux_gpu_tc_small_max
    f.restype = ctypes.c_uint32
    return int(f())


def tc_count_items(stream, role, optr, oadj, items, nitems, cap, counters,
                   pv=None):
    """Count one role's items (role 0 small, 1 staged, 2 hub) into counters
    (u64[2]: total, probes) and, with pv (u64[nv], rank-indexed), the
    per-vertex counts."""
    rc = lib().lux_gpu_tc_count_items(
        _u64(stream), ctypes.c_int(role), dp(optr), dp(oadj), dp(items),
        _u32(nitems), _u32(cap), dp(counters), dp(pv))
    if rc != 0:
        raise ValueError(f"tc_count_items: unsupported role={role} / "
                         f"cap={cap}")


def tc_count_plain(stream, nv, m, optr, oadj, counters, pv=None):
    lib().lux_gpu_tc_count_plain(_u64(stream), _u32(nv), _u64(m), dp(optr),
                                 dp(oadj), dp(counters), dp(pv))


# ---- k-core decomposition (kcore.hip) ----

def _kcore_const(name):
    f = getattr(lib(), name)
    f.restype = ctypes.c_uint32
    return int(f())


def kcore_hub_default():
    """KCORE_HUB: the longest row the row role takes when LUX_KCORE_HUB is
    unset."""
    return _kcore_const("lux_gpu_kcore_hub_default")


def kcore_fuse_default():
    """KCORE_FUSE: the tail kernel's round size when LUX_KCORE_FUSE is
    unset."""
    return _kcore_const("lux_gpu_kcore_fuse_default")


def kcore_fuse_max():
    return _kcore_const("lux_gpu_kcore_fuse_max")


def kcore_meta_words():
    return _kcore_const("lux_gpu_kcore_meta_words")


def kcore_adj_fill(stream, nv, m, optr, oadj, aptr, cursor, aadj):
    lib().lux_gpu_kcore_adj_fill(_u64(stream), _u32(nv), _u64(m), dp(optr),
                                 dp(oadj), dp(aptr), dp(cursor), dp(aadj))


def kcore_scan(stream, nv, aptr, deg, order, hubq, hubcap, meta, hub, k):
    lib().lux_gpu_kcore_scan(_u64(stream), _u32(nv), dp(aptr), dp(deg),
                             dp(order), dp(hubq), _u32(hubcap), dp(meta),
                             _u32(hub), ctypes.c_int(k))


def kcore_peel(stream, nv, aptr, aadj, deg, order, hubq, hubcap, meta, hub,
               k, head, tail, hubhead, hubtail):
    """One round: order[head:tail) and the hubq items [hubhead, hubtail)."""
    rc = lib().lux_gpu_kcore_peel(
        _u64(stream), _u32(nv), dp(aptr), dp(aadj), dp(deg), dp(order),
        dp(hubq), _u32(hubcap), dp(meta), _u32(hub), ctypes.c_int(k),
        _u32(head), _u32(tail), _u32(hubhead), _u32(hubtail))
    if rc != 0:
        raise ValueError(f"kcore_peel: bad round [{head}, {tail}) / "
                         f"[{hubhead}, {hubtail}), hub={hub}")


def kcore_tail(stream, nv, aptr, aadj, deg, order, hubq, hubcap, meta, hub,
               k, head, tail, hubtail, fuse):
    """Small rounds of the level from order[head:tail) on, one workgroup."""
    rc = lib().lux_gpu_kcore_tail(
        _u64(stream), _u32(nv), dp(aptr), dp(aadj), dp(deg), dp(order),
        dp(hubq), _u32(hubcap), dp(meta), _u32(hub), ctypes.c_int(k),
        _u32(head), _u32(tail), _u32(hubtail), _u32(fuse))
    if rc != 0:
        raise ValueError(f"kcore_tail: round [{head}, {tail}) does not "
                         f"qualify (fuse={fuse}, hub={hub})")


def kcore_check(stream, nv, aptr, aadj, core, bad):
    lib().lux_gpu_kcore_check(_u64(stream), _u32(nv), dp(aptr), dp(aadj),
                              dp(core), dp(bad))


# ---- strongly connected components (scc.hip) ----

class SccArgs(ctypes.Structure):
    """lux_scc_args: the graph in both directions and the per-vertex state."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "in_ptr", "in_col", "out_ptr", "out_col", "label", "in_cnt",
        "out_cnt", "colour", "mark", "stamp", "hubq", "meta")] + \
        [("nv", ctypes.c_uint32), ("hub", ctypes.c_uint32)]


class SccStep(ctypes.Structure):
    """lux_scc_step: one frontier step or trim round."""
    _fields_ = [("qr", ctypes.c_void_p), ("qw", ctypes.c_void_p)] + \
        [(n, ctypes.c_uint32) for n in ("qcap", "mw", "hr0", "hw0", "hcap")] + \
        [(n, ctypes.c_int) for n in ("mode", "dir", "cmode")] + \
        [("bit", ctypes.c_uint32), ("step", ctypes.c_uint32)]


SCC_TRIM, SCC_REACH, SCC_COLOUR = 0, 1, 2
SCC_F, SCC_B = 1, 2
# meta words
(SCC_M_TTAIL, SCC_M_RTAIL, SCC_M_CTAIL, SCC_M_HUBTAIL, SCC_M_FUSED,
 SCC_M_HEAD, SCC_M_DIED, SCC_M_MAXID, SCC_M_PIVOT) = range(9)


def _scc_const(name):
    f = getattr(lib(), name)
    f.restype = ctypes.c_uint32
    return int(f())


def scc_hub_default():
    """SCC_HUB: the longest row the row role takes when LUX_SCC_HUB is
    unset."""
    return _scc_const("lux_gpu_scc_hub_default")


def scc_fuse_default():
    """SCC_FUSE: the tail kernel's step size when LUX_SCC_FUSE is unset."""
    return _scc_const("lux_gpu_scc_fuse_default")


def scc_fuse_max():
    return _scc_const("lux_gpu_scc_fuse_max")


def scc_meta_words():
    return _scc_const("lux_gpu_scc_meta_words")


def scc_args(in_ptr, in_col, out_ptr, out_col, label, in_cnt, out_cnt,
             colour, mark, stamp, hubq, meta, nv, hub):
    return SccArgs(*(t.data_ptr() for t in (
        in_ptr, in_col, out_ptr, out_col, label, in_cnt, out_cnt, colour,
        mark, stamp, hubq, meta)), nv, hub)


def scc_step_desc(qr, qw, qcap, mw, hcap, mode, hr0=0, hw0=0, dir=0, cmode=0,
                  bit=0, step=0):
    """qr / qw: raw device addresses of the read and the write queue."""
    return SccStep(qr, qw, qcap, mw, hr0, hw0, hcap, mode, dir, cmode, bit,
                   step)


def scc_count(stream, a, st, items, nitems):
    """items: the static {vertex, chunk} list of the rows longer than hub."""
    lib().lux_gpu_scc_count(_u64(stream), ctypes.byref(a), ctypes.byref(st),
                            dp(items), _u32(nitems))


def scc_pivot(stream, a):
    lib().lux_gpu_scc_pivot(_u64(stream), ctypes.byref(a))


def scc_scan(stream, a, st, what):
    """what 0: colour = id and the first colour frontier; 1: the roots."""
    lib().lux_gpu_scc_scan(_u64(stream), ctypes.byref(a), ctypes.byref(st),
                           ctypes.c_int(what))


def scc_seed(stream, a, st, v, restart):
    lib().lux_gpu_scc_seed(_u64(stream), ctypes.byref(a), ctypes.byref(st),
                           _u32(v), ctypes.c_int(restart))


def scc_step(stream, a, st, head, tail, hubhead, hubtail, restart=0):
    """One step: st.qr[head:tail) and the hubq items [hubhead, hubtail)."""
    rc = lib().lux_gpu_scc_step(
        _u64(stream), ctypes.byref(a), ctypes.byref(st), _u32(head),
        _u32(tail), _u32(hubhead), _u32(hubtail), ctypes.c_int(restart))
    if rc != 0:
        raise ValueError(f"scc_step: bad step [{head}, {tail}) / "
                         f"[{hubhead}, {hubtail}), mode={st.mode}")


def scc_tail(stream, a, st, head, tail, hubtail, fuse, pingpong=0):
    """Small steps from st.qr[head:tail) on, one workgroup."""
    rc = lib().lux_gpu_scc_tail(
        _u64(stream), ctypes.byref(a), ctypes.byref(st), _u32(head),
        _u32(tail), _u32(hubtail), _u32(fuse), ctypes.c_int(pingpong))
    if rc != 0:
        raise ValueError(f"scc_tail: step [{head}, {tail}) does not qualify "
                         f"(fuse={fuse}, mode={st.mode})")


def scc_commit(stream, a, colour):
    lib().lux_gpu_scc_commit(_u64(stream), ctypes.byref(a),
                             ctypes.c_int(colour))


def scc_check_vertex(stream, nv, label, fwd, bwd, bad, what):
    lib().lux_gpu_scc_check_vertex(_u64(stream), _u32(nv), dp(label), dp(fwd),
                                   dp(bwd), dp(bad), ctypes.c_int(what))


def scc_check_sweep(stream, nv, in_ptr, in_col, out_ptr, out_col, label, fwd,
                    bwd, changed):
    lib().lux_gpu_scc_check_sweep(_u64(stream), _u32(nv), dp(in_ptr),
                                  dp(in_col), dp(out_ptr), dp(out_col),
                                  dp(label), dp(fwd), dp(bwd), dp(changed))


def scc_check_pairs(stream, nv, ne, in_ptr, in_col, out_ptr, out_col, label,
                    bad):
    lib().lux_gpu_scc_check_pairs(_u64(stream), _u32(nv), _u64(ne),
                                  dp(in_ptr), dp(in_col), dp(out_ptr),
                                  dp(out_col), dp(label), dp(bad))


# ---- minimum spanning forest (msf.hip) ----

class MsfArgs(ctypes.Structure):
    """lux_msf_args: the adjacency with edge ids, the simple edges, the
    static hub items and the state of a solve."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "aptr", "anbr", "aeid", "elo", "ehi", "w", "comp", "parent", "best",
        "dead", "inforest", "hubrow", "hubext", "item_row", "item_chunk",
        "meta")] + \
        [("m", ctypes.c_uint64), ("nv", ctypes.c_uint32),
         ("nhub", ctypes.c_uint32), ("nitems", ctypes.c_uint32),
         ("hub", ctypes.c_uint32), ("use_dead", ctypes.c_int)]


# meta words
(MSF_M_CWE, MSF_M_MERGED, MSF_M_SCANNED, MSF_M_TOTAL, MSF_M_NF,
 MSF_M_ERR) = range(6)


def _msf_const(name):
    f = getattr(lib(), name)
    f.restype = ctypes.c_uint32
    return int(f())


def msf_hub_default():
    """MSF_HUB: the longest row the row role takes when LUX_MSF_HUB is
    unset."""
    return _msf_const("lux_gpu_msf_hub_default")


def msf_meta_words():
    return _msf_const("lux_gpu_msf_meta_words")


def msf_args(aptr, anbr, aeid, elo, ehi, w, comp, parent, best, dead,
             inforest, hubrow, hubext, item_row, item_chunk, meta, m, nv,
             nhub, nitems, hub, use_dead):
    return MsfArgs(*(t.data_ptr() for t in (
        aptr, anbr, aeid, elo, ehi, w, comp, parent, best, dead, inforest,
        hubrow, hubext, item_row, item_chunk, meta)), m, nv, nhub, nitems,
        hub, int(bool(use_dead)))


def msf_weights(stream, nv, ne, row_ptr, col, weight, optr, oadj, w, err):
    """w (preset to INT32_MAX)[e] = the minimum weight over the CSC arcs of
    simple edge e; err counts arcs whose edge the DAG does not hold."""
    lib().lux_gpu_msf_weights(_u64(stream), _u32(nv), _u64(ne), dp(row_ptr),
                              dp(col), dp(weight), dp(optr), dp(oadj), dp(w),
                              dp(err))


def msf_adj_fill(stream, nv, m, optr, oadj, aptr, cursor, anbr, aeid, elo):
    lib().lux_gpu_msf_adj_fill(_u64(stream), _u32(nv), _u64(m), dp(optr),
                               dp(oadj), dp(aptr), dp(cursor), dp(anbr),
                               dp(aeid), dp(elo))


def msf_init(stream, a):
    lib().lux_gpu_msf_init(_u64(stream), ctypes.byref(a))


def msf_scan(stream, a, stamp):
    """Scan number stamp (1, 2, ...); returns the kernels launched."""
    rc = lib().lux_gpu_msf_scan(_u64(stream), ctypes.byref(a), _u32(stamp))
    if rc < 0:
        raise ValueError(f"msf_scan: bad arguments (stamp={stamp}, "
                         f"hub={a.hub}, m={a.m})")
    return rc


def msf_hook(stream, a):
    lib().lux_gpu_msf_hook(_u64(stream), ctypes.byref(a))


def msf_flatten(stream, a):
    lib().lux_gpu_msf_flatten(_u64(stream), ctypes.byref(a))


def msf_labels(stream, nv, comp, maxid, labels):
    lib().lux_gpu_msf_labels(_u64(stream), _u32(nv), dp(comp), dp(maxid),
                             dp(labels))


def msf_check(stream, nv, m, aptr, aeid, elo, ehi, w, mask, labels, pf, pa,
              out):
    """out u64[4]: violations, marked edges, vertices with label == id, the
    marked edges' weight."""
    lib().lux_gpu_msf_check(_u64(stream), _u32(nv), _u64(m), dp(aptr),
                            dp(aeid), dp(elo), dp(ehi), dp(w), dp(mask),
                            dp(labels), dp(pf), dp(pa), dp(out))


def msf_set_mark(stream, mask, m, e, value):
    """mask[e] = value on a u8[m] forest mask (the tests' corruption)."""
    rc = lib().lux_gpu_msf_set_mark(_u64(stream), dp(mask), _u64(m), _u64(e),
                                    ctypes.c_int(value))
    if rc != 0:
        raise ValueError(f"msf_set_mark: edge {e} outside [0, {m})")


# ---- greedy colouring / maximal independent set (colouring.hip) ----

class GcolArgs(ctypes.Structure):
    """lux_gcol_args: the predecessor / successor rows and the state of a
    solve."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "pptr", "padj", "sptr", "sadj", "colour", "pending", "order", "hubq",
        "rtail", "meta")] + \
        [("nv", ctypes.c_uint32), ("hubcap", ctypes.c_uint32),
         ("hub", ctypes.c_uint32)]


# meta words
GCOL_M_TAIL, GCOL_M_HUBTAIL, GCOL_M_FUSED, GCOL_M_HEAD = range(4)


def _gcol_const(name):
    f = getattr(lib(), name)
    f.restype = ctypes.c_uint32
    return int(f())


def gcol_hub_default():
    """GCOL_HUB: the longest row the row role takes when LUX_GCOL_HUB is
    unset."""
    return _gcol_const("lux_gpu_gcol_hub_default")


def gcol_fuse_default():
    """GCOL_FUSE: the tail kernel's round size when LUX_GCOL_FUSE is
    unset."""
    return _gcol_const("lux_gpu_gcol_fuse_default")


def gcol_fuse_max():
    return _gcol_const("lux_gpu_gcol_fuse_max")


def gcol_window_bits():
    """GCOL_WINDOW: the colours one pass of a select covers."""
    return _gcol_const("lux_gpu_gcol_window_bits")


def gcol_meta_words():
    return _gcol_const("lux_gpu_gcol_meta_words")


def gcol_args(pptr, padj, sptr, sadj, colour, pending, order, hubq, rtail,
              meta, nv, hubcap, hub):
    return GcolArgs(*(t.data_ptr() for t in (
        pptr, padj, sptr, sadj, colour, pending, order, hubq, rtail, meta)),
        nv, hubcap, hub)


def gcol_split_count(stream, nv, m, optr, oadj, rank, npred, nsucc):
    lib().lux_gpu_gcol_split_count(_u64(stream), _u32(nv), _u64(m), dp(optr),
                                   dp(oadj), dp(rank), dp(npred), dp(nsucc))


def gcol_split_fill(stream, nv, m, optr, oadj, rank, pptr, sptr, pcur, scur,
                    padj, sadj):
    lib().lux_gpu_gcol_split_fill(_u64(stream), _u32(nv), _u64(m), dp(optr),
                                  dp(oadj), dp(rank), dp(pptr), dp(sptr),
                                  dp(pcur), dp(scur), dp(padj), dp(sadj))


def gcol_seed(stream, a):
    lib().lux_gpu_gcol_seed(_u64(stream), ctypes.byref(a))


def gcol_step(stream, a, head, tail, hubhead, hubtail):
    """One round: order[head:tail) and the hubq items [hubhead, hubtail)."""
    rc = lib().lux_gpu_gcol_step(_u64(stream), ctypes.byref(a), _u32(head),
                                 _u32(tail), _u32(hubhead), _u32(hubtail))
    if rc != 0:
        raise ValueError(f"gcol_step: bad round [{head}, {tail}) / "
                         f"[{hubhead}, {hubtail}), hub={a.hub}")


def gcol_tail(stream, a, head, tail, hubtail, fuse, round0):
    """Small rounds from order[head:tail) on, one workgroup."""
    rc = lib().lux_gpu_gcol_tail(_u64(stream), ctypes.byref(a), _u32(head),
                                 _u32(tail), _u32(hubtail), _u32(fuse),
                                 _u32(round0))
    if rc != 0:
        raise ValueError(f"gcol_tail: round [{head}, {tail}) does not "
                         f"qualify (fuse={fuse}, hub={a.hub})")


def gcol_check(stream, nv, pptr, padj, sptr, sadj, colour, bad):
    lib().lux_gpu_gcol_check(_u64(stream), _u32(nv), dp(pptr), dp(padj),
                             dp(sptr), dp(sadj), dp(colour), dp(bad))
