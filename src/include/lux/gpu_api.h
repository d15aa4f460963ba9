// C ABI of liblux_gpu.so (gfx950 kernels). Consumed by the Python ctypes
// bindings (lux_amd/_native_gpu.py) and the native C++ runtime
// (src/runtime/). Pointers are device pointers; `stream` is a hipStream_t.
#pragma once
#include <cstdint>

#include "types.h"

// HIP vector type fwd-compat for non-HIP translation units
#ifndef __HIP_PLATFORM_AMD__
struct lux_uint2 { uint32_t x, y; };
#else
using lux_uint2 = uint2;
#endif

extern "C" {

// builder.hip
void lux_gpu_rmat_edges(uint64_t stream, uint64_t seed, int scale,
                        uint64_t ne, lux::V_ID* src, lux::V_ID* dst);
void lux_gpu_rmat_edges_folded(uint64_t stream, uint64_t seed, int scale,
                               lux::V_ID nv, uint64_t ne, lux::V_ID* src,
                               lux::V_ID* dst);
void lux_gpu_bipartite_edges(uint64_t stream, uint64_t seed,
                             lux::V_ID n_users, lux::V_ID n_items,
                             uint64_t ne, lux::V_ID* src, lux::V_ID* dst,
                             lux::WeightType* w);
void lux_gpu_hist_u32(uint64_t stream, uint64_t n, const lux::V_ID* ids,
                      uint32_t* hist);
void lux_gpu_rmat_edges_chunk(uint64_t stream, uint64_t seed, int scale,
                              uint64_t e0, uint64_t ne, lux::V_ID* src,
                              lux::V_ID* dst);
void lux_gpu_rmat_edges_folded_chunk(uint64_t stream, uint64_t seed,
                                     int scale, lux::V_ID nv, uint64_t e0,
                                     uint64_t ne, lux::V_ID* src,
                                     lux::V_ID* dst);
void lux_gpu_bipartite_edges_chunk(uint64_t stream, uint64_t seed,
                                   lux::V_ID n_users, lux::V_ID n_items,
                                   uint64_t e0, uint64_t ne, lux::V_ID* src,
                                   lux::V_ID* dst, lux::WeightType* w);
void lux_gpu_slice_scatter(uint64_t stream, uint64_t n, const lux::V_ID* src,
                           const lux::V_ID* dst, const lux::WeightType* w,
                           lux::V_ID rl, lux::V_ID rr,
                           unsigned long long* cursor, lux::V_ID* out_col,
                           lux::WeightType* out_w);
uint32_t lux_gpu_scan_partials_size(uint64_t n);
void lux_gpu_scan_end_offsets(uint64_t stream, uint64_t n,
                              const uint32_t* in, lux::E_ID* out_end,
                              unsigned long long* partials);
void lux_gpu_u64_to_u32(uint64_t stream, uint64_t n,
                        const unsigned long long* in, uint32_t* out);
void lux_gpu_edges_to_csc(uint64_t stream, uint32_t nv, uint64_t ne,
                          const lux::V_ID* src, const lux::V_ID* dst,
                          const lux::WeightType* w, lux::E_ID* col_end,
                          lux::V_ID* out_src, lux::WeightType* out_w,
                          uint32_t* hist, unsigned long long* cursor,
                          unsigned long long* partials);
void lux_gpu_local_row_ptr(uint64_t stream, uint32_t vp, lux::E_ID col_left,
                           const lux::E_ID* col_end_slice,
                           lux::E_ID* row_ptr_loc);
void lux_gpu_blocked_count(uint64_t stream, uint64_t ep, const lux::V_ID* col,
                           const lux::E_ID* row_ptr_loc, lux::V_ID vp,
                           const lux::V_ID* bounds, int nb, lux::V_ID lo,
                           lux::V_ID hi, uint32_t* counts);
void lux_gpu_blocked_scatter(uint64_t stream, uint64_t ep,
                             const lux::V_ID* col,
                             const lux::E_ID* row_ptr_loc, lux::V_ID vp,
                             const lux::V_ID* bounds, int nb, lux::V_ID lo,
                             lux::V_ID hi, unsigned long long* cursor,
                             lux::V_ID* out_col);
// weighted SSSP: blocked scatter moving col and its weight to one slot;
// endpoint-hash weights for synthetic graphs
void lux_gpu_blocked_scatter_w(uint64_t stream, uint64_t ep,
                               const lux::V_ID* col,
                               const lux::WeightType* weight,
                               const lux::E_ID* row_ptr_loc, lux::V_ID vp,
                               const lux::V_ID* bounds, int nb, lux::V_ID lo,
                               lux::V_ID hi, unsigned long long* cursor,
                               lux::V_ID* out_col, lux::WeightType* out_w);
void lux_gpu_hash_weights(uint64_t stream, uint64_t ep, const lux::V_ID* col,
                          const lux::E_ID* row_ptr_loc, lux::V_ID vp,
                          lux::V_ID row_left, uint64_t seed, uint32_t wmax,
                          lux::WeightType* weight);

// pull.hip
void lux_gpu_build_bins(uint64_t stream, uint32_t vp,
                        const lux::E_ID* row_ptr, lux::V_ID* bin0,
                        lux::V_ID* bin1, lux_uint2* bin2, lux::V_ID* bin2v,
                        uint32_t* counters);
void lux_gpu_pull_iter(uint64_t stream, int mode, uint32_t n0,
                       const lux::V_ID* bin0, uint32_t n1,
                       const lux::V_ID* bin1, uint32_t n2,
                       const lux_uint2* bin2, uint32_t nbig,
                       const lux::V_ID* bin2v, const void* row_ptr,
                       int row_u32, const lux::V_ID* col, const void* oldv,
                       void* newv, const lux::V_ID* deg, lux::V_ID row_left,
                       float init_rank);
// weighted SSSP dense sweep (min-plus, saturating; wgt indexed like col)
void lux_gpu_pull_iter_w(uint64_t stream, uint32_t n0, const lux::V_ID* bin0,
                         uint32_t n1, const lux::V_ID* bin1, uint32_t n2,
                         const lux_uint2* bin2, uint32_t nbig,
                         const lux::V_ID* bin2v, const void* row_ptr,
                         int row_u32, const lux::V_ID* col,
                         const lux::WeightType* wgt, const uint32_t* oldv,
                         uint32_t* newv, lux::V_ID row_left);
void lux_gpu_pull_finish_pr(uint64_t stream, lux::V_ID vp, float* newv,
                            const lux::V_ID* deg, lux::V_ID row_left,
                            float init_rank);
// slot path (PR_SUM): per-entry {compact row index, edge range} streams
// next to the bins, an accumulator over the rows with in-edges only, one
// launch per src window, epilogue straight into the replicated array
void lux_gpu_pull_active_flags(uint64_t stream, lux::V_ID vp,
                               const lux::E_ID* row_ptr, uint32_t* flags);
void lux_gpu_pull_active_list(uint64_t stream, lux::V_ID vp,
                              const uint32_t* flags, const lux::E_ID* ends,
                              lux::V_ID* active);
void lux_gpu_pull_build_slots(uint64_t stream, uint32_t n,
                              const lux::V_ID* bin, const void* row_ptr,
                              int row_u32, const lux::E_ID* ends,
                              lux::V_ID* cidx, lux_uint2* rng);
void lux_gpu_pull_build_hub_slots(uint64_t stream, uint32_t n2,
                                  const lux_uint2* bin2, const void* row_ptr,
                                  int row_u32, const lux::E_ID* ends,
                                  lux::V_ID* cidx, lux_uint2* rng);
void lux_gpu_pull_slots_iter(uint64_t stream, uint32_t n0,
                             const lux::V_ID* cidx0, const lux_uint2* rng0,
                             uint32_t n1, const lux::V_ID* cidx1,
                             const lux_uint2* rng1, uint32_t n2,
                             const lux::V_ID* cidx2, const lux_uint2* rng2,
                             const lux::V_ID* col, const float* oldv,
                             float* acc);
// stream role (thread bin as a contiguous edge stream, one wave per tile)
void lux_gpu_pull_slot_counts(uint64_t stream, uint32_t n,
                              const lux_uint2* rng, uint32_t* cnt);
void lux_gpu_pull_stream_copy(uint64_t stream, uint32_t n0,
                              const lux_uint2* rng0, const uint32_t* off0,
                              const lux::V_ID* col, lux::V_ID* scol0);
void lux_gpu_pull_stream_tile_counts(uint64_t stream, uint32_t n0,
                                     const uint32_t* off0, uint32_t* cnt);
void lux_gpu_pull_stream_tile_fill(uint64_t stream, uint32_t n0,
                                   const uint32_t* off0,
                                   const lux::E_ID* ends, uint32_t* tile0);
void lux_gpu_pull_slots_stream_iter(
    uint64_t stream, uint32_t n0, const lux::V_ID* cidx0, uint32_t nt,
    const uint32_t* tile0, const uint32_t* off0, const lux::V_ID* scol0,
    uint32_t n1, const lux::V_ID* cidx1, const lux_uint2* rng1, uint32_t n2,
    const lux::V_ID* cidx2, const lux_uint2* rng2, const lux::V_ID* col,
    const float* oldv, float* acc);
void lux_gpu_pull_finish_pr_active(uint64_t stream, lux::V_ID na,
                                   const lux::V_ID* active, const float* acc,
                                   float* out, const lux::V_ID* deg,
                                   lux::V_ID row_left, float init_rank);
// hot order: sources ranked by out-degree inside their src window (pos, a
// window-preserving permutation); column copies hold pos[col], the sweeps
// gather from gold[pos[v]] = old[v], the epilogue keeps gold current
void lux_gpu_pull_hot_col(uint64_t stream, uint64_t n, const lux::V_ID* col,
                          const lux::V_ID* pos, lux::V_ID* hcol);
void lux_gpu_pull_stream_copy_hot(uint64_t stream, uint32_t n0,
                                  const lux_uint2* rng0,
                                  const uint32_t* off0, const lux::V_ID* col,
                                  const lux::V_ID* pos, lux::V_ID* scol0);
void lux_gpu_pull_hot_apos(uint64_t stream, lux::V_ID na,
                           const lux::V_ID* active, const lux::V_ID* pos,
                           const lux::V_ID* deg, lux::V_ID row_left,
                           lux::V_ID* apos);
void lux_gpu_pull_hot_scatter(uint64_t stream, lux::V_ID nv,
                              const lux::V_ID* pos, const float* old,
                              float* gold);
void lux_gpu_pull_finish_pr_active_hot(uint64_t stream, lux::V_ID na,
                                       const lux::V_ID* active,
                                       const lux::V_ID* apos,
                                       const float* acc, float* out,
                                       float* gold, const lux::V_ID* deg,
                                       lux::V_ID row_left, float init_rank);
// hot-order stream sweep with the k hottest sources of the window [lo, hi)
// in LDS (k: 2048 / 4096, else -1 and no launch)
int lux_gpu_pull_slots_stream_hot_iter(
    uint64_t stream, uint32_t n0, const lux::V_ID* cidx0, uint32_t nt,
    const uint32_t* tile0, const uint32_t* off0, const lux::V_ID* scol0,
    uint32_t n1, const lux::V_ID* cidx1, const lux_uint2* rng1, uint32_t n2,
    const lux::V_ID* cidx2, const lux_uint2* rng2, const lux::V_ID* col,
    const float* gold, float* acc, lux::V_ID lo, lux::V_ID hi, int k);
// the same sweep by 1024-thread workgroups, two resident per CU: ks sources
// in LDS for the stream role, kw for the wave and chunk roles ((8192, 16384),
// else -1 and no launch; -2: the runtime refused the LDS size). ne0 / ne: entries of scol0 / col, the role split follows the roles'
// edge counts. max_groups: 0 = eight workgroups per CU, else the grid size.
int lux_gpu_pull_slots_stream_hot_wide_iter(
    uint64_t stream, uint32_t n0, const lux::V_ID* cidx0, uint32_t nt,
    const uint32_t* tile0, const uint32_t* off0, const lux::V_ID* scol0,
    uint64_t ne0, uint32_t n1, const lux::V_ID* cidx1, const lux_uint2* rng1,
    uint32_t n2, const lux::V_ID* cidx2, const lux_uint2* rng2,
    const lux::V_ID* col, uint64_t ne, const float* gold, float* acc,
    lux::V_ID lo, lux::V_ID hi, int ks, int kw, uint32_t max_groups);
void lux_gpu_pull_fill_inactive_pr(uint64_t stream, lux::V_ID vp,
                                   const lux::E_ID* row_ptr, float* out,
                                   const lux::V_ID* deg, lux::V_ID row_left,
                                   float init_rank);

// push.hip
void lux_gpu_csr_scatter(uint64_t stream, uint64_t ep, const lux::V_ID* col,
                         const lux::E_ID* row_ptr_loc, lux::V_ID vp,
                         lux::V_ID row_left, unsigned long long* cursor,
                         lux::V_ID* push_col);
void lux_gpu_frontier_expand(uint64_t stream, int old_dense,
                             lux::V_ID in_row_left, lux::V_ID in_count,
                             const uint8_t* old_seg,
                             const uint32_t* qlabels /*nullable*/,
                             uint32_t* labels_repair /*nullable*/,
                             const lux::E_ID* push_row_ptr,
                             lux_uint2* items, uint32_t* counter,
                             uint32_t max_items);
void lux_gpu_frontier_expand_auto(uint64_t stream, lux::V_ID verts,
                                  lux::V_ID in_row_left, const uint8_t* seg,
                                  const uint32_t* qlabels,
                                  uint32_t* labels_repair,
                                  const lux::E_ID* push_row_ptr,
                                  lux_uint2* items, uint32_t* counter,
                                  uint32_t max_items);
void lux_gpu_frontier_fixup(uint64_t stream, lux::V_ID vp,
                            lux::V_ID row_left, lux::V_ID capacity,
                            int built_dense, const uint32_t* snapshot,
                            const uint32_t* labels_part,
                            const uint32_t* deg_part, uint8_t* new_seg,
                            uint32_t* annex, uint8_t* tmp_seg,
                            uint32_t* meta,
                            const uint32_t* item_counter /*nullable*/,
                            uint32_t max_items);
void lux_gpu_push_chunk_scatter(uint64_t stream, int is_min, int new_dense,
                                const lux_uint2* items,
                                const uint32_t* counter, uint32_t max_items,
                                const lux::E_ID* push_row_ptr,
                                const lux::V_ID* push_col,
                                const uint32_t* old_labels,
                                const uint32_t* snapshot,
                                uint32_t* new_labels, lux::V_ID my_row_left,
                                uint8_t* new_seg, lux::V_ID capacity,
                                uint32_t* visited_bits /*nullable*/);
void lux_gpu_bits_from_labels(uint64_t stream, lux::V_ID vp,
                              const uint32_t* labels, uint32_t* bits);

void lux_gpu_build_bitmap(uint64_t stream, lux::V_ID vp,
                          const uint32_t* snapshot,
                          const uint32_t* new_labels, uint8_t* seg);
void lux_gpu_d2s(uint64_t stream, lux::V_ID vp, lux::V_ID row_left,
                 const uint8_t* dense_seg, uint8_t* sparse_seg);
void lux_gpu_publish_labels_guarded(uint64_t stream, lux::V_ID vp,
                                    const uint32_t* meta,
                                    const uint32_t* labels_part,
                                    uint32_t* labels_slice);
void lux_gpu_check(uint64_t stream, int is_min, lux::V_ID vp,
                   lux::V_ID row_left, const lux::E_ID* row_ptr_loc,
                   const lux::V_ID* col, const uint32_t* labels,
                   unsigned long long* mistakes);
// weighted SSSP (min-plus): push CSR of interleaved {dst, weight} edges,
// per-edge-candidate chunk scatter, weighted check oracle
void lux_gpu_csr_scatter_w(uint64_t stream, uint64_t ep, const lux::V_ID* col,
                           const lux::WeightType* weight,
                           const lux::E_ID* row_ptr_loc, lux::V_ID vp,
                           lux::V_ID row_left, unsigned long long* cursor,
                           lux_uint2* push_edge);
void lux_gpu_push_chunk_scatter_w(uint64_t stream, int new_dense,
                                  const lux_uint2* items,
                                  const uint32_t* counter, uint32_t max_items,
                                  const lux::E_ID* push_row_ptr,
                                  const lux_uint2* push_edge,
                                  const uint32_t* old_labels,
                                  const uint32_t* snapshot,
                                  uint32_t* new_labels, lux::V_ID my_row_left,
                                  uint8_t* new_seg, lux::V_ID capacity);
void lux_gpu_check_w(uint64_t stream, lux::V_ID vp, lux::V_ID row_left,
                     const lux::E_ID* row_ptr_loc, const lux::V_ID* col,
                     const lux::WeightType* weight, const uint32_t* labels,
                     lux::V_ID source, unsigned long long* mistakes);
// bucketed (near-far delta-stepping) schedule: the per-iteration O(vp)
// select pass — active bitmap into seg, deferred set into dirty, counts and
// the minimum deferred label into seg's header and meta[6..7]
void lux_gpu_bucket_select(uint64_t stream, lux::V_ID vp, uint32_t* snapshot,
                           const uint32_t* labels_part, uint32_t* dirty,
                           const uint32_t* limit, int replace, uint8_t* seg,
                           uint32_t* meta);

// cf.hip
void lux_gpu_cf_seed(uint64_t stream, uint64_t n, const float* oldv,
                     float* newv);
void lux_gpu_cf_iter(uint64_t stream, uint32_t n0, const lux::V_ID* bin0,
                     uint32_t n1, const lux::V_ID* bin1, uint32_t n2,
                     const lux_uint2* bin2, uint32_t nbig,
                     const lux::V_ID* bin2v, const lux::E_ID* row_ptr,
                     const lux::V_ID* col, const lux::WeightType* w,
                     const float* oldv, float* newv, lux::V_ID row_left,
                     int K);

// cc_uf.hip
void lux_gpu_count_diff(uint64_t stream, uint64_t n, const uint32_t* a,
                        const uint32_t* b, unsigned long long* out);
void lux_gpu_uf_union_binned(uint64_t stream, uint32_t n0,
                             const lux::V_ID* bin0, uint32_t n1,
                             const lux::V_ID* bin1, uint32_t n2,
                             const lux_uint2* bin2, const lux::E_ID* row_ptr,
                             const lux::V_ID* col, lux::V_ID row_left,
                             lux::V_ID* parent, const uint32_t* gbits);
void lux_gpu_uf_union_kth(uint64_t stream, lux::V_ID vp,
                          const lux::E_ID* row_ptr, const lux::V_ID* col,
                          lux::V_ID row_left, lux::V_ID* parent, uint32_t k);
void lux_gpu_cc_giant_bits(uint64_t stream, lux::V_ID nv,
                           const lux::V_ID* labels, lux::V_ID giant,
                           uint32_t* bits);
void lux_gpu_uf_union_star(uint64_t stream, lux::V_ID nv,
                           const lux::V_ID* star, lux::V_ID* parent);
void lux_gpu_uf_flatten(uint64_t stream, lux::V_ID nv, lux::V_ID* parent,
                        lux::V_ID* labels);

// cf_als.hip
// 1 <= K <= 128; anything else aborts on the host before any launch. K
// selects the hub scratch pitch KP (64 for K <= 64, 128 above):
// gram_scratch is f32[nbig * KP * KP] (upper triangle, rows/cols >= K stay
// zero), rhs_scratch f32[nbig * KP], both zeroed by the caller per sweep.
// oldv_bf (bf16 gather replica) is used for K <= 64 only.
void lux_gpu_cf_als_iter(uint64_t stream, uint32_t n0, const lux::V_ID* bin0,
                         uint32_t n1, const lux::V_ID* bin1, uint32_t n2,
                         const lux_uint2* bin2, uint32_t nbig,
                         const lux::V_ID* bin2v, const int* hubidx,
                         float* gram_scratch, float* rhs_scratch,
                         const lux::E_ID* row_ptr, const lux::V_ID* col,
                         const lux::WeightType* w, const float* oldv,
                         const uint16_t* oldv_bf /*nullable*/, float* newv,
                         lux::V_ID row_left, int K);

// bc.hip (betweenness centrality, single rank)
// Records: lux_uint2[nv] {depth, value}. Level order: a counting sort of the
// reached rows by key = depth*3 + degree bin into a u32 word list (a row id
// per thread/wave-bin row, a {row, chunk} pair per hub chunk); cnt and the
// scanned offsets are in words.
void lux_gpu_bc_init(uint64_t stream, lux::V_ID nv, lux::V_ID source,
                     const uint32_t* depth, lux_uint2* rec, float* sigma,
                     float* delta);
void lux_gpu_bc_order_hist(uint64_t stream, lux::V_ID nv,
                           const uint32_t* depth, const lux::E_ID* row_ptr,
                           uint32_t levels, uint32_t* cnt,
                           unsigned long long* hubrows);
void lux_gpu_bc_order_scatter(uint64_t stream, lux::V_ID nv,
                              const uint32_t* depth, const lux::E_ID* row_ptr,
                              uint32_t levels, unsigned long long* cursor,
                              uint32_t* list);
void lux_gpu_bc_level(uint64_t stream, int forward, const uint32_t* list,
                      uint64_t o0, uint64_t o1, uint64_t o2, uint64_t o3,
                      const lux::E_ID* row_ptr, const lux::V_ID* adj,
                      lux_uint2* rec, float* sigma, float* delta, uint32_t d,
                      int last, unsigned long long* edges);
void lux_gpu_bc_check(uint64_t stream, lux::V_ID nv, lux::V_ID source,
                      const lux::E_ID* in_ptr, const lux::V_ID* in_adj,
                      const lux::E_ID* out_ptr, const lux::V_ID* out_adj,
                      const uint32_t* depth, const float* sigma,
                      const float* delta, double rtol,
                      unsigned long long* out);

// tc.hip (triangle counting, single rank)
// optr u64[nv+1] / oadj u32[m]: the rank-relabelled, lo -> hi oriented
// simple graph, rows strictly ascending. items: u32 triples {row, first,
// last} (arc offsets inside the row), one list per role: 0 small (a wave per
// item, rows of at most small_max arcs; longer ones are skipped), 1 staged (a workgroup per item, the row in cap <= stage_max LDS
// entries), 2 hub (the same, searched in global memory). counters: u64[2]
// {total, probes}, added to. pv: u64[nv] rank-indexed per-vertex counts,
// added to; null counts the total alone.
uint32_t lux_gpu_tc_stage_max();
uint32_t lux_gpu_tc_small_max();
int lux_gpu_tc_count_items(uint64_t stream, int role, const lux::E_ID* optr,
                           const lux::V_ID* oadj, const uint32_t* items,
                           uint32_t nitems, uint32_t cap,
                           unsigned long long* counters,
                           unsigned long long* pv);
void lux_gpu_tc_count_plain(uint64_t stream, lux::V_ID nv, lux::E_ID m,
                            const lux::E_ID* optr, const lux::V_ID* oadj,
                            unsigned long long* counters,
                            unsigned long long* pv);

// kcore.hip (k-core decomposition by synchronous peeling, single rank)
// optr u64[nv+1] / oadj u32[m]: the id-order DAG of the simple graph (row u
// lists its neighbours > u). aptr u64[nv+1] / aadj u32[2m]: the full
// symmetric adjacency. deg i32[nv]: the current degree, the coreness at the
// end. order u32[nv] and hubq ({vertex, chunk} u32 pairs, hubcap of them):
// append-only lists, a round being order[head : tail) plus
// hubq[hubhead : hubtail). meta u32[meta_words]: [0] the order cursor, [1]
// the hubq cursor, [2] the scan's min{deg : deg > k} (0xFFFFFFFF: none),
// [3] rounds done and [4] first unprocessed entry of the last tail launch.
// hub: rows longer than this are peeled by hubq chunks of hub entries.
uint32_t lux_gpu_kcore_hub_default();
uint32_t lux_gpu_kcore_fuse_default();
uint32_t lux_gpu_kcore_fuse_max();
uint32_t lux_gpu_kcore_meta_words();
void lux_gpu_kcore_adj_fill(uint64_t stream, lux::V_ID nv, lux::E_ID m,
                            const lux::E_ID* optr, const lux::V_ID* oadj,
                            const lux::E_ID* aptr, uint32_t* cursor,
                            lux::V_ID* aadj);
void lux_gpu_kcore_scan(uint64_t stream, lux::V_ID nv, const lux::E_ID* aptr,
                        int* deg, lux::V_ID* order, uint32_t* hubq,
                        uint32_t hubcap, uint32_t* meta, uint32_t hub, int k);
int lux_gpu_kcore_peel(uint64_t stream, lux::V_ID nv, const lux::E_ID* aptr,
                       const lux::V_ID* aadj, int* deg, lux::V_ID* order,
                       uint32_t* hubq, uint32_t hubcap, uint32_t* meta,
                       uint32_t hub, int k, uint32_t head, uint32_t tail,
                       uint32_t hubhead, uint32_t hubtail);
int lux_gpu_kcore_tail(uint64_t stream, lux::V_ID nv, const lux::E_ID* aptr,
                       const lux::V_ID* aadj, int* deg, lux::V_ID* order,
                       uint32_t* hubq, uint32_t hubcap, uint32_t* meta,
                       uint32_t hub, int k, uint32_t head, uint32_t tail,
                       uint32_t hubtail, uint32_t fuse);
void lux_gpu_kcore_check(uint64_t stream, lux::V_ID nv, const lux::E_ID* aptr,
                         const lux::V_ID* aadj, const int* core,
                         unsigned long long* bad);

// scc.hip (strongly connected components: trim, forward-backward reach and
// colour propagation; single rank). lux_scc_args is the graph in both
// directions and the per-vertex state, lux_scc_step one frontier step or
// trim round: it reads qr[head : tail) and the hubq items
// [hr0 + hubhead, hr0 + hubtail), appends to qw at the cursor meta[mw]
// (below qcap) and to hubq from hw0 at the cursor meta[3] (below hcap).
// mode 0 trim / 1 reach / 2 colour; dir 0 along out-edges, 1 along in-edges;
// cmode: reach only inside the frontier vertex's colour; bit: the mark bit
// of the traversal; step: the colour step's stamp. meta u32[meta_words]:
// [0] trim, [1] reach, [2] colour queue cursors, [3] the hubq cursor, [4]
// steps done and [5] first unprocessed entry of the last tail launch, [6]
// died and [7] max id of the last commit, [8] the pivot.
struct lux_scc_args {
  const lux::E_ID* in_ptr;   // u64[nv+1]
  const lux::V_ID* in_col;   // u32[ne]
  const lux::E_ID* out_ptr;  // u64[nv+1]
  const lux::V_ID* out_col;  // u32[ne]
  uint32_t* label;           // u32[nv], 0xFFFFFFFF = alive
  int* in_cnt;               // i32[nv]
  int* out_cnt;              // i32[nv]
  uint32_t* colour;          // u32[nv]
  uint32_t* mark;            // u32[nv]
  uint32_t* stamp;           // u32[nv]
  uint32_t* hubq;            // u32 pairs
  uint32_t* meta;            // u32[meta_words]
  lux::V_ID nv;
  uint32_t hub;  // rows longer than this go through hubq
};
struct lux_scc_step {
  const lux::V_ID* qr;
  lux::V_ID* qw;
  uint32_t qcap, mw, hr0, hw0, hcap;
  int mode, dir, cmode;
  uint32_t bit, step;
};
uint32_t lux_gpu_scc_hub_default();
uint32_t lux_gpu_scc_fuse_default();
uint32_t lux_gpu_scc_fuse_max();
uint32_t lux_gpu_scc_meta_words();
void lux_gpu_scc_count(uint64_t stream, const lux_scc_args* a,
                       const lux_scc_step* st, const uint32_t* items,
                       uint32_t nitems);
void lux_gpu_scc_pivot(uint64_t stream, const lux_scc_args* a);
void lux_gpu_scc_scan(uint64_t stream, const lux_scc_args* a,
                      const lux_scc_step* st, int what);
void lux_gpu_scc_seed(uint64_t stream, const lux_scc_args* a,
                      const lux_scc_step* st, lux::V_ID v, int restart);
int lux_gpu_scc_step(uint64_t stream, const lux_scc_args* a,
                     const lux_scc_step* st, uint32_t head, uint32_t tail,
                     uint32_t hubhead, uint32_t hubtail, int restart);
int lux_gpu_scc_tail(uint64_t stream, const lux_scc_args* a,
                     const lux_scc_step* st, uint32_t head, uint32_t tail,
                     uint32_t hubtail, uint32_t fuse, int pingpong);
void lux_gpu_scc_commit(uint64_t stream, const lux_scc_args* a, int colour);
void lux_gpu_scc_check_vertex(uint64_t stream, lux::V_ID nv,
                              const uint32_t* label, uint32_t* fwd,
                              uint32_t* bwd, unsigned long long* bad,
                              int what);
void lux_gpu_scc_check_sweep(uint64_t stream, lux::V_ID nv,
                             const lux::E_ID* in_ptr, const lux::V_ID* in_col,
                             const lux::E_ID* out_ptr,
                             const lux::V_ID* out_col, const uint32_t* label,
                             uint32_t* fwd, uint32_t* bwd, uint32_t* changed);
void lux_gpu_scc_check_pairs(uint64_t stream, lux::V_ID nv, lux::E_ID ne,
                             const lux::E_ID* in_ptr, const lux::V_ID* in_col,
                             const lux::E_ID* out_ptr,
                             const lux::V_ID* out_col, const uint32_t* label,
                             unsigned long long* bad);

// msf.hip (minimum spanning forest by synchronous Boruvka rounds, single
// rank). optr / oadj: the id-order DAG of the simple graph; arc e of it is
// simple edge e = (elo[e], ehi[e]) with ehi = oadj, weight w[e] = the minimum
// over the edge's occurrences. aptr u64[nv+1] / anbr, aeid u32[2m]: the
// full symmetric adjacency, every entry with its edge id. hubrow: the rows
// longer than hub; item i is chunk item_chunk[i] (hub entries) of row
// hubrow[item_row[i]]. meta u64[meta_words]: [0] components with an edge,
// [1] hooks and [2] entries walked of the last scan / hook; [3] the total
// weight (i64 bits) and [4] the forest edges of the solve; [5] errors.
struct lux_msf_args {
  const lux::E_ID* aptr;       // u64[nv+1]
  const lux::V_ID* anbr;       // u32[2m]
  const uint32_t* aeid;        // u32[2m]
  const lux::V_ID* elo;        // u32[m]
  const lux::V_ID* ehi;        // u32[m]
  const int* w;                // i32[m]
  lux::V_ID* comp;             // u32[nv]
  lux::V_ID* parent;           // u32[nv]
  unsigned long long* best;    // u64[nv]
  uint8_t* dead;               // u8[nv]
  uint8_t* inforest;           // u8[m]
  const lux::V_ID* hubrow;     // u32[nhub]
  uint32_t* hubext;            // u32[nhub]
  const uint32_t* item_row;    // u32[nitems]
  const uint32_t* item_chunk;  // u32[nitems]
  unsigned long long* meta;    // u64[meta_words]
  lux::E_ID m;
  lux::V_ID nv;
  uint32_t nhub, nitems;
  uint32_t hub;  // rows longer than this are walked in chunks of hub entries
  int use_dead;  // 0: walk every row in every scan
};
uint32_t lux_gpu_msf_hub_default();
uint32_t lux_gpu_msf_meta_words();
void lux_gpu_msf_weights(uint64_t stream, lux::V_ID nv, lux::E_ID ne,
                         const lux::E_ID* row_ptr, const lux::V_ID* col,
                         const int* weight, const lux::E_ID* optr,
                         const lux::V_ID* oadj, int* w,
                         unsigned long long* err);
void lux_gpu_msf_adj_fill(uint64_t stream, lux::V_ID nv, lux::E_ID m,
                          const lux::E_ID* optr, const lux::V_ID* oadj,
                          const lux::E_ID* aptr, uint32_t* cursor,
                          lux::V_ID* anbr, uint32_t* aeid, lux::V_ID* elo);
void lux_gpu_msf_init(uint64_t stream, const lux_msf_args* a);
int lux_gpu_msf_scan(uint64_t stream, const lux_msf_args* a, uint32_t stamp);
void lux_gpu_msf_hook(uint64_t stream, const lux_msf_args* a);
void lux_gpu_msf_flatten(uint64_t stream, const lux_msf_args* a);
void lux_gpu_msf_labels(uint64_t stream, lux::V_ID nv, const lux::V_ID* comp,
                        lux::V_ID* maxid, lux::V_ID* labels);
void lux_gpu_msf_check(uint64_t stream, lux::V_ID nv, lux::E_ID m,
                       const lux::E_ID* aptr, const uint32_t* aeid,
                       const lux::V_ID* elo, const lux::V_ID* ehi,
                       const int* w, const uint8_t* mask,
                       const lux::V_ID* labels, lux::V_ID* pf, lux::V_ID* pa,
                       unsigned long long* out);
int lux_gpu_msf_set_mark(uint64_t stream, uint8_t* mask, lux::E_ID m,
                         lux::E_ID e, int value);

// colouring.hip (greedy colouring in a fixed priority order and the first
// maximal independent set, Jones-Plassmann rounds; single rank). optr / oadj:
// the id-order DAG of the simple graph; rank u32[nv]: a smaller rank
// precedes. pptr / padj: the predecessor rows, sptr / sadj: the successor
// rows, m entries each. lux_gcol_args is the split graph and the state of a
// solve. hubq items are {vertex, item}: item 0xFFFFFFFF selects the colour
// of a vertex whose predecessor row is longer than hub, item c notifies
// entries [c * hub, (c + 1) * hub) of a successor row longer than hub.
// meta u32[meta_words]: [0] the order cursor, [1] the hubq cursor, [2]
// rounds done and [3] first unprocessed entry of the last tail launch.
struct lux_gcol_args {
  const lux::E_ID* pptr;  // u64[nv+1]
  const lux::V_ID* padj;  // u32[m]
  const lux::E_ID* sptr;  // u64[nv+1]
  const lux::V_ID* sadj;  // u32[m]
  int* colour;            // i32[nv], -1 until coloured
  int* pending;           // i32[nv], the uncoloured predecessors
  lux::V_ID* order;       // u32[nv], append-only
  uint32_t* hubq;         // u32[2 * hubcap]
  uint32_t* rtail;        // u32[nv]: the order cursor after each fused round
  uint32_t* meta;         // u32[meta_words]
  lux::V_ID nv;
  uint32_t hubcap;  // items
  uint32_t hub;     // rows longer than this go through hubq
};
uint32_t lux_gpu_gcol_hub_default();
uint32_t lux_gpu_gcol_fuse_default();
uint32_t lux_gpu_gcol_fuse_max();
uint32_t lux_gpu_gcol_window_bits();
uint32_t lux_gpu_gcol_meta_words();
void lux_gpu_gcol_split_count(uint64_t stream, lux::V_ID nv, lux::E_ID m,
                              const lux::E_ID* optr, const lux::V_ID* oadj,
                              const uint32_t* rank, uint32_t* npred,
                              uint32_t* nsucc);
void lux_gpu_gcol_split_fill(uint64_t stream, lux::V_ID nv, lux::E_ID m,
                             const lux::E_ID* optr, const lux::V_ID* oadj,
                             const uint32_t* rank, const lux::E_ID* pptr,
                             const lux::E_ID* sptr, uint32_t* pcur,
                             uint32_t* scur, lux::V_ID* padj,
                             lux::V_ID* sadj);
void lux_gpu_gcol_seed(uint64_t stream, const lux_gcol_args* g);
int lux_gpu_gcol_step(uint64_t stream, const lux_gcol_args* g, uint32_t head,
                      uint32_t tail, uint32_t hubhead, uint32_t hubtail);
int lux_gpu_gcol_tail(uint64_t stream, const lux_gcol_args* g, uint32_t head,
                      uint32_t tail, uint32_t hubtail, uint32_t fuse,
                      uint32_t round0);
void lux_gpu_gcol_check(uint64_t stream, lux::V_ID nv, const lux::E_ID* pptr,
                        const lux::V_ID* padj, const lux::E_ID* sptr,
                        const lux::V_ID* sadj, const int* colour,
                        unsigned long long* bad);

}  // extern "C"
