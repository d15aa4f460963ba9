// Pull-model engine: degree-binned CSC gather kernels for gfx950.
//
// Replaces the reference's one-size block-scan CSC walk (pr_kernel,
// pagerank_gpu.cu:49-102; sssp_pull_kernel, sssp_gpu.cu:85-130) with a
// three-bin design shaped for CDNA4 and power-law graphs:
//   bin0 (deg <  T1): one thread per dst vertex, grid-stride.
//   bin1 (T1..T2):    one 64-lane wave per dst vertex; lanes stride the
//                     contiguous in-edge range (coalesced 256 B/instr col
//                     reads), shuffle-reduce, lane 0 writes.
//   bin2 (deg >= T2): hub vertices split into CHUNK_EDGES-edge chunks, one
//                     256-thread block per chunk, block-reduce + one global
//                     atomic per block (guideline: reduce first, atomic once).
// Bins are built once at init (degrees are static); per iteration we launch
// prep (bin2 only) + 3 bin kernels on one stream. The same machinery runs
// PageRank's float sum and SSSP/CC's u32 min/max dense fallback.
//
// PageRank additionally has a slot path (lux_gpu_pull_slots_iter): the
// same three role bodies in ONE launch per src window, fed by per-entry
// {compact row index, edge range} streams instead of row_ptr gathers, and
// accumulating into an array over the rows with in-edges only. Its thread
// bin can run as the stream role instead (lux_gpu_pull_slots_stream_iter):
// one wave per tile of consecutive slots, lane = edge, row sums out of LDS.
// In hot order (sources ranked by out-degree inside each src window) the
// same sweeps run on permuted column copies and a permuted rank table, and
// lux_gpu_pull_slots_stream_hot_iter keeps a window's hottest sources in LDS
// (lux_gpu_pull_slots_stream_hot_wide_iter: four to eight times as many, in
// 1024-thread workgroups).
#include "gpu_common.h"

namespace lux {

constexpr V_ID T1 = 32;
constexpr V_ID T2 = 2048;
constexpr V_ID CHUNK_EDGES = 8192;

enum PullMode { PR_SUM = 0, LAB_MIN = 1, LAB_MAX = 2, CF_SGD = 3,
                LAB_MIN_W = 4 };

// ---------------- bin building ----------------

// LDS-aggregated bin build: per-tile LDS counters, ONE global atomic per
// bin per tile (global-atomic contention on 3 words made the naive version
// ~250x slower at nv=2^27 — guideline 12: reduce first, atomic once).
__global__ void build_bins_kernel(V_ID vp, const E_ID* row_ptr,
                                  V_ID* bin0, V_ID* bin1, uint2* bin2,
                                  V_ID* bin2v, uint32_t* counters) {
  __shared__ uint32_t lcnt[4], lbase[4];
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t tile = (uint64_t)blockIdx.x * blockDim.x; tile < vp;
       tile += stride) {
    uint64_t v = tile + threadIdx.x;
    if (threadIdx.x < 4) lcnt[threadIdx.x] = 0;
    __syncthreads();
    int my_bin = -1;
    uint32_t lpos = 0, nchunks = 0, lpos_c = 0;
    if (v < vp) {
      E_ID deg = row_ptr[v + 1] - row_ptr[v];
      if (deg == 0) {
        // not binned: rows with no edges in this (block-)CSC are covered by
        // the seed/finish pass, so sweeps touch only active rows
      } else if (deg < T1) {
        my_bin = 0;
        lpos = atomicAdd(&lcnt[0], 1u);
      } else if (deg < T2) {
        my_bin = 1;
        lpos = atomicAdd(&lcnt[1], 1u);
      } else {
        my_bin = 3;
        lpos = atomicAdd(&lcnt[3], 1u);
        nchunks = (uint32_t)((deg + CHUNK_EDGES - 1) / CHUNK_EDGES);
        lpos_c = atomicAdd(&lcnt[2], nchunks);
      }
    }
    __syncthreads();
    if (threadIdx.x < 4)
      lbase[threadIdx.x] = lcnt[threadIdx.x]
                               ? atomicAdd(&counters[threadIdx.x],
                                           lcnt[threadIdx.x])
                               : 0;
    __syncthreads();
    if (my_bin == 0) bin0[lbase[0] + lpos] = (V_ID)v;
    else if (my_bin == 1) bin1[lbase[1] + lpos] = (V_ID)v;
    else if (my_bin == 3) {
      bin2v[lbase[3] + lpos] = (V_ID)v;
      uint32_t base = lbase[2] + lpos_c;
      for (uint32_t c = 0; c < nchunks; c++)
        bin2[base + c] = make_uint2((V_ID)v, c);
    }
    __syncthreads();
  }
}

// ---------------- per-mode value semantics ----------------

template <PullMode M> struct Val;
template <> struct Val<PR_SUM> {
  using T = float;
  static constexpr bool SKIP_SETTLED = false;
  static __device__ __forceinline__ T ident() { return 0.0f; }
  static __device__ __forceinline__ T map(T s) { return s; }
  static __device__ __forceinline__ T comb(T a, T b) { return a + b; }
  static __device__ __forceinline__ void atom(T* p, T v) { atomicAdd(p, v); }
  static __device__ __forceinline__ T reduce_wave(T v) {
    return wave_reduce_sum(v);
  }
};
template <> struct Val<LAB_MIN> {
  using T = uint32_t;
  // hop-SSSP (BFS) invariant: a finite label is the true depth and can
  // never improve under synchronized iterations — settled rows skip their
  // whole edge range (newv keeps the seeded own label). Only valid for the
  // +1 hop metric; LAB_MAX (CC) labels keep moving and never skip.
  static constexpr bool SKIP_SETTLED = true;
  static __device__ __forceinline__ T ident() { return INF_LABEL; }
  static __device__ __forceinline__ T map(T s) {
    return s == INF_LABEL ? INF_LABEL : s + 1;  // hop relaxation (+1)
  }
  static __device__ __forceinline__ T comb(T a, T b) { return a < b ? a : b; }
  static __device__ __forceinline__ void atom(T* p, T v) { atomicMin(p, v); }
  static __device__ __forceinline__ T reduce_wave(T v) {
    return wave_reduce_min(v);
  }
};
template <> struct Val<LAB_MAX> {
  using T = uint32_t;
  static constexpr bool SKIP_SETTLED = false;
  static __device__ __forceinline__ T ident() { return 0; }
  static __device__ __forceinline__ T map(T s) { return s; }
  static __device__ __forceinline__ T comb(T a, T b) { return a > b ? a : b; }
  static __device__ __forceinline__ void atom(T* p, T v) { atomicMax(p, v); }
  static __device__ __forceinline__ T reduce_wave(T v) {
    return wave_reduce_max(v);
  }
};

// Weighted SSSP (min-plus): every edge maps its source label with its own
// weight (mapw), labels keep improving over iterations, so no row is ever
// skipped as settled. Weights are non-negative i32; the sum saturates at
// 0xFFFFFFFE (a finite distance never becomes INF_LABEL or wraps).
template <> struct Val<LAB_MIN_W> {
  using T = uint32_t;
  static constexpr bool SKIP_SETTLED = false;
  static __device__ __forceinline__ T ident() { return INF_LABEL; }
  static __device__ __forceinline__ T mapw(T s, WeightType w) {
    if (s == INF_LABEL) return INF_LABEL;
    unsigned long long c = (unsigned long long)s + (uint32_t)w;
    return c > 0xFFFFFFFEull ? 0xFFFFFFFEu : (T)c;
  }
  static __device__ __forceinline__ T comb(T a, T b) { return a < b ? a : b; }
  static __device__ __forceinline__ void atom(T* p, T v) { atomicMin(p, v); }
  static __device__ __forceinline__ T reduce_wave(T v) {
    return wave_reduce_min(v);
  }
};

// Epilogue: PR computes (1-a)/nv + a*sum then stores /out_degree
// (pagerank_gpu.cu:97-100); labels fold the dst's own old label in.
template <PullMode M>
__device__ __forceinline__ typename Val<M>::T finish(
    typename Val<M>::T acc, typename Val<M>::T own, float init_rank,
    V_ID deg) {
  if (M == PR_SUM) {
    float pr = init_rank + PR_ALPHA * (float)acc;
    return deg != 0 ? pr / (float)deg : pr;
  }
  return Val<M>::comb(acc, own);
}

struct PullArgs {
  const void* row_ptr;   // RowT[vp+1], local 0-based: u64, or u32 for the
                         // blocked path (block-local offsets < 2^32 — half
                         // the per-row sweep traffic, NOTES_r2 item 1)
  const V_ID* col;       // u32[ep], local
  const void* oldv;      // full nv
  void* newv;            // vp
  const V_ID* deg;       // u32[nv] out-degrees (PR) or null
  V_ID row_left;
  float init_rank;
};

// Weighted sweeps: wgt[j] is the weight of edge col[j] (same edge index,
// for the plain CSC and for every src window of the blocked one).
struct PullArgsW : PullArgs {
  const WeightType* wgt;
};

// Hot-order sweeps with the window's K hottest sources in LDS: in hot order
// they are the K table entries from position lo on, copied by every
// workgroup once per launch; a gather whose index falls there never leaves
// the CU (PR_SUM slot sweeps only, see "hot order" below).
template <int K>
struct PullArgsHot : PullArgs {
  V_ID lo;  // first position of the src window
};
template <int K>
__device__ __forceinline__ float* hot_prefix() {
  __shared__ float hot[K];
  return hot;
}
template <int K>
__device__ __forceinline__ float hot_load(const float* oldv,
                                          const float* hot, V_ID lo,
                                          V_ID c) {
  // one flat load from a per-lane LDS-or-global address: no branch, so the
  // four gathers of a batch stay independent loads in flight together
  V_ID r = c - lo;
  const float* p = r < (V_ID)K ? hot + r : oldv + c;
  return *p;
}
// The wide sweep (pull_slots_stream_hot_wide_kernel) keeps its prefix in the
// workgroup's dynamic LDS: K sources from float offset OFF on, both fixed by
// the workgroup's role.
template <int K, int OFF>
struct PullArgsWide : PullArgs {
  V_ID lo;
};
__device__ __forceinline__ float* wide_lds() {
  extern __shared__ float wide_lds_[];
  return wide_lds_;
}

// Result store for the non-atomic bins. The iteration contract: newv is
// pre-seeded (PR: zeros; labels: the old label slice) before the sweep(s),
// every sweep — blocked or not — folds its partial in, and PR's epilogue
// runs once at the end (pull_finish_kernel). One writer per row per sweep,
// so the fold needs no atomics.
template <PullMode M>
__device__ __forceinline__ void store_result(typename Val<M>::T* slot,
                                             typename Val<M>::T acc) {
  *slot = Val<M>::comb(acc, *slot);
}

// Edge-range accumulation with a 4-deep software pipeline: the rolled
// col[j] -> oldv[col[j]] chain is two dependent loads with ONE iteration
// in flight (the dynamic trip count stops the compiler from unrolling);
// batching 4 col reads then 4 independent gathers quadruples the memory
// parallelism per lane (same fix as cf.hip cf_stage_tile).
template <PullMode M>
__device__ __forceinline__ typename Val<M>::T gather_range(
    const typename Val<M>::T* oldv, const V_ID* col, E_ID j, E_ID e,
    E_ID step) {
  using V = Val<M>;
  using T = typename V::T;
  T a0 = V::ident(), a1 = V::ident(), a2 = V::ident(), a3 = V::ident();
  for (; j + 3 * step < e; j += 4 * step) {
    V_ID c0 = col[j], c1 = col[j + step], c2 = col[j + 2 * step],
         c3 = col[j + 3 * step];
    a0 = V::comb(a0, V::map(oldv[c0]));
    a1 = V::comb(a1, V::map(oldv[c1]));
    a2 = V::comb(a2, V::map(oldv[c2]));
    a3 = V::comb(a3, V::map(oldv[c3]));
  }
  for (; j < e; j += step) a0 = V::comb(a0, V::map(oldv[col[j]]));
  return V::comb(V::comb(a0, a1), V::comb(a2, a3));
}

// gather_range with a per-edge weight: the same four-way pipeline, the
// weights of a batch fetched next to its col entries (both coalesced in
// the wave and chunk roles), then four independent label gathers.
template <PullMode M>
__device__ __forceinline__ typename Val<M>::T gather_range_w(
    const typename Val<M>::T* oldv, const V_ID* col, const WeightType* wgt,
    E_ID j, E_ID e, E_ID step) {
  using V = Val<M>;
  using T = typename V::T;
  T a0 = V::ident(), a1 = V::ident(), a2 = V::ident(), a3 = V::ident();
  for (; j + 3 * step < e; j += 4 * step) {
    V_ID c0 = col[j], c1 = col[j + step], c2 = col[j + 2 * step],
         c3 = col[j + 3 * step];
    WeightType w0 = wgt[j], w1 = wgt[j + step], w2 = wgt[j + 2 * step],
               w3 = wgt[j + 3 * step];
    a0 = V::comb(a0, V::mapw(oldv[c0], w0));
    a1 = V::comb(a1, V::mapw(oldv[c1], w1));
    a2 = V::comb(a2, V::mapw(oldv[c2], w2));
    a3 = V::comb(a3, V::mapw(oldv[c3], w3));
  }
  for (; j < e; j += step) a0 = V::comb(a0, V::mapw(oldv[col[j]], wgt[j]));
  return V::comb(V::comb(a0, a1), V::comb(a2, a3));
}

// What a role body calls for its edge range: picked by the args type, so
// the unweighted instantiations are the plain gather_range as before.
template <PullMode M>
__device__ __forceinline__ typename Val<M>::T gather_edges(
    const PullArgs& a, const typename Val<M>::T* oldv, E_ID j, E_ID e,
    E_ID step) {
  return gather_range<M>(oldv, a.col, j, e, step);
}
template <PullMode M>
__device__ __forceinline__ typename Val<M>::T gather_edges(
    const PullArgsW& a, const typename Val<M>::T* oldv, E_ID j, E_ID e,
    E_ID step) {
  return gather_range_w<M>(oldv, a.col, a.wgt, j, e, step);
}
// gather_range<PR_SUM> with the hot prefix served from LDS: same four-way
// pipeline, same association order, same values
template <int K>
__device__ __forceinline__ float gather_range_hot(const float* oldv,
                                                  const float* hot, V_ID lo,
                                                  const V_ID* col, E_ID j,
                                                  E_ID e, E_ID step) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (; j + 3 * step < e; j += 4 * step) {
    V_ID c0 = col[j], c1 = col[j + step], c2 = col[j + 2 * step],
         c3 = col[j + 3 * step];
    a0 = a0 + hot_load<K>(oldv, hot, lo, c0);
    a1 = a1 + hot_load<K>(oldv, hot, lo, c1);
    a2 = a2 + hot_load<K>(oldv, hot, lo, c2);
    a3 = a3 + hot_load<K>(oldv, hot, lo, c3);
  }
  for (; j < e; j += step) a0 = a0 + hot_load<K>(oldv, hot, lo, col[j]);
  return (a0 + a1) + (a2 + a3);
}
template <PullMode M, int K>
__device__ __forceinline__ float gather_edges(const PullArgsHot<K>& a,
                                              const float* oldv, E_ID j,
                                              E_ID e, E_ID step) {
  static_assert(M == PR_SUM, "hot prefix: float sums only");
  return gather_range_hot<K>(oldv, hot_prefix<K>(), a.lo, a.col, j, e, step);
}
template <PullMode M, int K, int OFF>
__device__ __forceinline__ float gather_edges(const PullArgsWide<K, OFF>& a,
                                              const float* oldv, E_ID j,
                                              E_ID e, E_ID step) {
  static_assert(M == PR_SUM, "hot prefix: float sums only");
  return gather_range_hot<K>(oldv, wide_lds() + OFF, a.lo, a.col, j, e, step);
}

// one gathered value, for the roles that do not go through gather_edges
__device__ __forceinline__ float old_load(const PullArgs&, const float* oldv,
                                          V_ID c) {
  return oldv[c];
}
template <int K>
__device__ __forceinline__ float old_load(const PullArgsHot<K>& a,
                                          const float* oldv, V_ID c) {
  return hot_load<K>(oldv, hot_prefix<K>(), a.lo, c);
}
template <int K, int OFF>
__device__ __forceinline__ float old_load(const PullArgsWide<K, OFF>& a,
                                          const float* oldv, V_ID c) {
  return hot_load<K>(oldv, wide_lds() + OFF, a.lo, c);
}

// ---- where a bin entry's output row and edge range come from ----
// The role bodies below are written once against these small sources.
// Table sources are the bin lists + a row_ptr table (every mode, RowT =
// u64 plain / u32 blocked). Slot sources (PR_SUM) carry, per entry, the
// compact output index and the edge range as two coalesced streams, so a
// sweep never gathers from a vp-wide row table (see "slot streams" below).
template <typename RowT>
struct TableRows {
  const V_ID* bin;
  const RowT* row_ptr;
  __device__ __forceinline__ V_ID row(uint64_t i) const { return bin[i]; }
  __device__ __forceinline__ void range(uint64_t, V_ID v, E_ID& b,
                                        E_ID& e) const {
    b = row_ptr[v];
    e = row_ptr[v + 1];
  }
};
template <typename RowT>
struct TableChunks {
  const uint2* bin2;
  const RowT* row_ptr;
  __device__ __forceinline__ V_ID row(uint64_t i, uint32_t& chunk) const {
    uint2 ent = bin2[i];
    chunk = ent.y;
    return ent.x;
  }
  __device__ __forceinline__ void range(uint64_t, V_ID v, uint32_t chunk,
                                        E_ID& b, E_ID& e) const {
    b = (E_ID)row_ptr[v] + (E_ID)chunk * CHUNK_EDGES;
    e = row_ptr[v + 1];
    if (e > b + CHUNK_EDGES) e = b + CHUNK_EDGES;
  }
};
struct SlotRows {
  const V_ID* cidx;  // compact row index (position in the active list)
  const uint2* rng;  // {begin, end} edge offsets; hub entries: one chunk
  __device__ __forceinline__ V_ID row(uint64_t i) const { return cidx[i]; }
  __device__ __forceinline__ V_ID row(uint64_t i, uint32_t&) const {
    return cidx[i];
  }
  __device__ __forceinline__ void range(uint64_t i, V_ID, E_ID& b,
                                        E_ID& e) const {
    uint2 r = rng[i];
    b = r.x;
    e = r.y;
  }
  __device__ __forceinline__ void range(uint64_t i, V_ID, uint32_t, E_ID& b,
                                        E_ID& e) const {
    range(i, 0, b, e);
  }
};

// ---- bin0 role: thread per vertex (block `blk` of `nblk`) ----
template <PullMode M, typename Src, typename Args>
__device__ __forceinline__ void pull_thread_role(uint32_t blk, uint32_t nblk,
                                                 uint32_t n0, const Src& src,
                                                 const Args& a) {
  using V = Val<M>;
  using T = typename V::T;
  const T* oldv = (const T*)a.oldv;
  T* newv = (T*)a.newv;
  uint64_t stride = (uint64_t)blockDim.x * nblk;
  for (uint64_t i = blk * (uint64_t)blockDim.x + threadIdx.x; i < n0;
       i += stride) {
    V_ID v = src.row(i);
    if (V::SKIP_SETTLED && oldv[a.row_left + v] != (T)INF_LABEL)
      continue;  // settled hop label: newv keeps the seed
    E_ID b, e;
    src.range(i, v, b, e);
    T acc = gather_edges<M>(a, oldv, b, e, 1);
    store_result<M>(&newv[v], acc);
  }
}

// ---- bin1 role: wave per vertex ----
template <PullMode M, typename Src, typename Args>
__device__ __forceinline__ void pull_wave_role(uint32_t blk, uint32_t nblk,
                                               uint32_t n1, const Src& src,
                                               const Args& a) {
  using V = Val<M>;
  using T = typename V::T;
  const T* oldv = (const T*)a.oldv;
  T* newv = (T*)a.newv;
  int lane = threadIdx.x & (WAVE - 1);
  uint64_t wave_id = ((uint64_t)blk * blockDim.x + threadIdx.x) / WAVE;
  uint64_t nwaves = ((uint64_t)nblk * blockDim.x) / WAVE;
  for (uint64_t i = wave_id; i < n1; i += nwaves) {
    V_ID v = src.row(i);
    if (V::SKIP_SETTLED && oldv[a.row_left + v] != (T)INF_LABEL)
      continue;
    E_ID b, e;
    src.range(i, v, b, e);
    T acc = gather_edges<M>(a, oldv, b + lane, e, WAVE);
    acc = V::reduce_wave(acc);
    if (lane == 0)
      store_result<M>(&newv[v], acc);
  }
}

// ---- bin2 role: chunk accumulation (hubs) ----
// Contains __syncthreads(): every thread of a workgroup must enter it
// together (the callers pick the role from blockIdx.x alone).
template <PullMode M, typename Src, typename Args>
__device__ __forceinline__ void pull_chunk_role(uint32_t blk, uint32_t nblk,
                                                uint32_t n2, const Src& src,
                                                const Args& a) {
  using V = Val<M>;
  using T = typename V::T;
  __shared__ T lds[BLOCK / WAVE];
  const T* oldv = (const T*)a.oldv;
  T* newv = (T*)a.newv;
  for (uint32_t i = blk; i < n2; i += nblk) {
    uint32_t chunk = 0;
    V_ID v = src.row(i, chunk);
    if (V::SKIP_SETTLED && oldv[a.row_left + v] != (T)INF_LABEL)
      continue;
    E_ID b, e;
    src.range(i, v, chunk, b, e);
    T acc = gather_edges<M>(a, oldv, b + threadIdx.x, e, blockDim.x);
    // block reduce (sum mode) or wave+lds fold (min/max)
    int lane = threadIdx.x & (WAVE - 1);
    int wid = threadIdx.x >> 6;
    acc = V::reduce_wave(acc);
    if (lane == 0) lds[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      acc = lds[0];
      for (int w = 1; w < (int)(blockDim.x / WAVE); w++)
        acc = V::comb(acc, lds[w]);
      V::atom(&newv[v], acc);
    }
    __syncthreads();
  }
}

template <PullMode M, typename RowT>
__global__ void pull_thread_kernel(uint32_t n0, const V_ID* bin0,
                                   PullArgs a) {
  pull_thread_role<M>(blockIdx.x, gridDim.x, n0,
                      TableRows<RowT>{bin0, (const RowT*)a.row_ptr}, a);
}

template <PullMode M, typename RowT>
__global__ void pull_wave_kernel(uint32_t n1, const V_ID* bin1, PullArgs a) {
  pull_wave_role<M>(blockIdx.x, gridDim.x, n1,
                    TableRows<RowT>{bin1, (const RowT*)a.row_ptr}, a);
}

template <PullMode M, typename RowT>
__global__ void pull_chunk_kernel(uint32_t n2, const uint2* bin2,
                                  PullArgs a) {
  pull_chunk_role<M>(blockIdx.x, gridDim.x, n2,
                     TableChunks<RowT>{bin2, (const RowT*)a.row_ptr}, a);
}

// Weighted twins of the three table kernels (LAB_MIN_W): same role bodies,
// PullArgsW carries the weight array.
template <typename RowT>
__global__ void pull_thread_w_kernel(uint32_t n0, const V_ID* bin0,
                                     PullArgsW a) {
  pull_thread_role<LAB_MIN_W>(blockIdx.x, gridDim.x, n0,
                              TableRows<RowT>{bin0, (const RowT*)a.row_ptr},
                              a);
}

template <typename RowT>
__global__ void pull_wave_w_kernel(uint32_t n1, const V_ID* bin1,
                                   PullArgsW a) {
  pull_wave_role<LAB_MIN_W>(blockIdx.x, gridDim.x, n1,
                            TableRows<RowT>{bin1, (const RowT*)a.row_ptr}, a);
}

template <typename RowT>
__global__ void pull_chunk_w_kernel(uint32_t n2, const uint2* bin2,
                                    PullArgsW a) {
  pull_chunk_role<LAB_MIN_W>(blockIdx.x, gridDim.x, n2,
                             TableChunks<RowT>{bin2, (const RowT*)a.row_ptr},
                             a);
}

// ---- slot streams: one launch per src window (PR_SUM) ----
// a.newv is the active-row accumulator acc[na]; a.row_ptr is unused. The
// three bins of one window touch disjoint rows, so they need no ordering:
// each workgroup takes its role from blockIdx.x — chunk blocks first, then
// wave, then thread, so the long-running work is dispatched first and the
// thread-bin blocks fill the wave-bin tail.
struct SlotBins {
  uint32_t n0, n1, n2;  // entries per bin (n2 = hub chunks)
  uint32_t g1, g2;      // workgroups of the wave / chunk roles
  const V_ID *cidx0, *cidx1, *cidx2;
  const uint2 *rng0, *rng1, *rng2;
};

template <PullMode M>
__global__ void __launch_bounds__(BLOCK)
    pull_slots_kernel(SlotBins s, PullArgs a) {
  uint32_t blk = blockIdx.x;
  if (blk < s.g2) {
    pull_chunk_role<M>(blk, s.g2, s.n2, SlotRows{s.cidx2, s.rng2}, a);
  } else if (blk < s.g2 + s.g1) {
    pull_wave_role<M>(blk - s.g2, s.g1, s.n1, SlotRows{s.cidx1, s.rng1}, a);
  } else {
    pull_thread_role<M>(blk - s.g2 - s.g1, gridDim.x - s.g2 - s.g1, s.n0,
                        SlotRows{s.cidx0, s.rng0}, a);
  }
}

// ---- stream role: the thread bin as one contiguous edge stream ----
// A thread-bin slot holds 3-4 edges on average, so thread-per-slot runs the
// rolled tail of gather_range: one dependent col -> oldv chain per lane, a
// fifth of the lanes active. Here one wave takes a TILE of consecutive
// thread-bin slots (at most 64 slots and TILE_EDGES edges), reads the tile's
// col entries from scol0 (the bin's edges copied contiguously in slot order)
// with lane = edge, gathers oldv for them as independent loads into the
// wave's LDS segment, and lane r then folds slot r's segment out of LDS in
// gather_range's step-1 association order (bit-identical sums).
constexpr uint32_t TILE_EDGES = 512;
constexpr uint32_t TILE_GROUP = WAVE;  // tiles never span a 64-slot group

struct SlotStream {
  uint32_t nt;            // tiles
  const uint32_t* tile0;  // u32[nt+1]: first slot of each tile, [nt] = n0
  const uint32_t* off0;   // u32[n0+1]: exclusive scan of the slots' degrees
  const V_ID* scol0;      // u32[off0[n0]]
};

// gather_range<PR_SUM>(.., step 1) over values already sitting in LDS
__device__ __forceinline__ float lds_range_sum(const float* v, uint32_t j,
                                               uint32_t e) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (; j + 3 < e; j += 4) {
    a0 = a0 + v[j];
    a1 = a1 + v[j + 1];
    a2 = a2 + v[j + 2];
    a3 = a3 + v[j + 3];
  }
  for (; j < e; j++) a0 = a0 + v[j];
  return (a0 + a1) + (a2 + a3);
}

// Wave-local throughout (no __syncthreads()): a wave's LDS accesses issue
// in order, the wavefront fence only keeps the compiler from moving them.
// NW waves per workgroup; vals: the workgroup's NW tile buffers.
template <PullMode M, uint32_t NW, typename Args>
__device__ __forceinline__ void pull_stream_tiles(uint32_t blk, uint32_t nblk,
                                                  const SlotStream& st,
                                                  const V_ID* cidx0,
                                                  const Args& a,
                                                  float (*vals)[TILE_EDGES]) {
  static_assert(M == PR_SUM, "stream role: float sums only");
  const float* oldv = (const float*)a.oldv;
  float* acc = (float*)a.newv;
  uint32_t lane = threadIdx.x & (WAVE - 1);
  uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* v = vals[wid];
  uint64_t nwaves = (uint64_t)nblk * NW;
  uint64_t t = (uint64_t)blk * NW + wid;
  if (t >= st.nt) return;
  uint32_t s0 = st.tile0[t], s1 = st.tile0[t + 1];
  uint32_t e0 = st.off0[s0], e1 = st.off0[s1];
  for (;;) {
    // the next tile's bounds are fetched under this tile's gathers
    uint64_t tn = t + nwaves;
    bool more = tn < st.nt;
    uint32_t s0n = 0, s1n = 0, e0n = 0, e1n = 0;
    if (more) {
      s0n = st.tile0[tn];
      s1n = st.tile0[tn + 1];
    }
    uint32_t rb = 0, re = 0;
    V_ID ci = 0;
    float prev = 0.0f;
    bool row = lane < s1 - s0;
    if (row) {
      rb = st.off0[s0 + lane] - e0;
      re = st.off0[s0 + lane + 1] - e0;
      ci = cidx0[s0 + lane];
      prev = acc[ci];  // one writer per row and sweep
    }
    // at most TILE_EDGES / (4 * WAVE) = 2 trips; 4 col loads, then 4
    // independent gathers per lane
    for (uint32_t base = e0 + lane; base < e1; base += 4 * WAVE) {
      uint32_t i0 = base, i1 = base + WAVE, i2 = base + 2 * WAVE,
               i3 = base + 3 * WAVE;
      bool p1 = i1 < e1, p2 = i2 < e1, p3 = i3 < e1;
      V_ID c0 = st.scol0[i0];
      V_ID c1 = p1 ? st.scol0[i1] : 0;
      V_ID c2 = p2 ? st.scol0[i2] : 0;
      V_ID c3 = p3 ? st.scol0[i3] : 0;
      float x0 = old_load(a, oldv, c0);
      float x1 = p1 ? old_load(a, oldv, c1) : 0.0f;
      float x2 = p2 ? old_load(a, oldv, c2) : 0.0f;
      float x3 = p3 ? old_load(a, oldv, c3) : 0.0f;
      v[i0 - e0] = x0;
      if (p1) v[i1 - e0] = x1;
      if (p2) v[i2 - e0] = x2;
      if (p3) v[i3 - e0] = x3;
    }
    if (more) {
      e0n = st.off0[s0n];
      e1n = st.off0[s1n];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (row) acc[ci] = Val<M>::comb(lds_range_sum(v, rb, re), prev);
    // the next tile's LDS writes stay behind these reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (!more) break;
    t = tn;
    s0 = s0n, s1 = s1n, e0 = e0n, e1 = e1n;
  }
}

template <PullMode M, typename Args>
__device__ __forceinline__ void pull_stream_role(uint32_t blk, uint32_t nblk,
                                                 const SlotStream& st,
                                                 const V_ID* cidx0,
                                                 const Args& a) {
  constexpr uint32_t NW = BLOCK / WAVE;
  __shared__ float vals[NW][TILE_EDGES];
  pull_stream_tiles<M, NW>(blk, nblk, st, cidx0, a, vals);
}

template <PullMode M>
__global__ void __launch_bounds__(BLOCK)
    pull_slots_stream_kernel(SlotBins s, SlotStream st, PullArgs a) {
  uint32_t blk = blockIdx.x;
  if (blk < s.g2) {
    pull_chunk_role<M>(blk, s.g2, s.n2, SlotRows{s.cidx2, s.rng2}, a);
  } else if (blk < s.g2 + s.g1) {
    pull_wave_role<M>(blk - s.g2, s.g1, s.n1, SlotRows{s.cidx1, s.rng1}, a);
  } else {
    pull_stream_role<M>(blk - s.g2 - s.g1, gridDim.x - s.g2 - s.g1, st,
                        s.cidx0, a);
  }
}

// pull_slots_stream_kernel on hot-ordered tables with the window's K hottest
// sources in LDS (a.oldv is gold; [a.lo, hi) the window's positions)
template <PullMode M, int K>
__global__ void __launch_bounds__(BLOCK)
    pull_slots_stream_hot_kernel(SlotBins s, SlotStream st, PullArgsHot<K> a,
                                 V_ID hi) {
  float* hot = hot_prefix<K>();
  const float* oldv = (const float*)a.oldv;
  for (uint32_t i = threadIdx.x; i < (uint32_t)K; i += BLOCK) {
    uint64_t p = (uint64_t)a.lo + i;
    hot[i] = p < hi ? oldv[p] : 0.0f;
  }
  __syncthreads();
  uint32_t blk = blockIdx.x;
  if (blk < s.g2) {
    pull_chunk_role<M>(blk, s.g2, s.n2, SlotRows{s.cidx2, s.rng2}, a);
  } else if (blk < s.g2 + s.g1) {
    pull_wave_role<M>(blk - s.g2, s.g1, s.n1, SlotRows{s.cidx1, s.rng1}, a);
  } else {
    pull_stream_role<M>(blk - s.g2 - s.g1, gridDim.x - s.g2 - s.g1, st,
                        s.cidx0, a);
  }
}

// ---- wide hot sweep: 1024-thread workgroups, two resident per CU ----
// Same three roles and the same row sums as pull_slots_stream_hot_kernel, but
// a workgroup is 16 waves, so one prefix copy serves four times the waves and
// can be four to eight times as long at the same 8 waves per SIMD. The grid
// is a few workgroups per CU (every workgroup copies its prefix once per
// launch) and the role loops grid-stride. One dynamic LDS allocation, laid out by role:
//   stream role:      16 tile buffers (32 KB) | prefix of KS sources
//   wave, chunk role: prefix of KW sources | 16 floats of reduction scratch
constexpr int WIDE_BLOCK = 1024;
constexpr uint32_t WIDE_NW = WIDE_BLOCK / WAVE;
constexpr uint32_t WIDE_Q = WIDE_BLOCK / BLOCK;  // 256-thread quarters
constexpr uint32_t WIDE_TILE_FLOATS = WIDE_NW * TILE_EDGES;
constexpr uint32_t WIDE_SCRATCH = WIDE_Q * (BLOCK / WAVE);
// Default grid per CU. Two workgroups are resident; with exactly those the
// fixed role split decides the launch's tail (13.75 ms per RMAT-27 iteration
// against 13.54 for the 256-thread kernel). Queued workgroups let dispatch
// even the roles out and cost one more prefix copy each: 4 per CU 13.42 ms,
// 8 per CU 13.12 ms (BENCHLOG r16.1).
constexpr uint32_t WIDE_GROUPS_PER_CU = 8;

template <int KS, int KW>
constexpr uint32_t wide_lds_bytes() {
  uint32_t s = WIDE_TILE_FLOATS + KS, w = KW + WIDE_SCRATCH;
  return 4 * (s > w ? s : w);
}

// pull_chunk_role for a 1024-thread workgroup: every 256-thread quarter takes
// its own chunk entry, strides it by 256 and folds its four waves in its own
// scratch, so a chunk's partial is the float pull_chunk_role gives. The trip
// count is the workgroup's: a quarter without an entry idles through the
// barriers.
template <int K, int OFF>
__device__ __forceinline__ void pull_chunk_role_wide(
    uint32_t blk, uint32_t nblk, uint32_t n2, const SlotRows& src,
    const PullArgsWide<K, OFF>& a, float* scratch) {
  using V = Val<PR_SUM>;
  const float* oldv = (const float*)a.oldv;
  float* newv = (float*)a.newv;
  uint32_t q = threadIdx.x / BLOCK, tq = threadIdx.x % BLOCK;
  uint32_t lane = tq & (WAVE - 1), wid = tq >> 6;
  float* lds = scratch + q * (BLOCK / WAVE);
  for (uint64_t base = (uint64_t)blk * WIDE_Q; base < n2;
       base += (uint64_t)nblk * WIDE_Q) {
    uint64_t i = base + q;
    bool work = i < n2;  // uniform in the quarter
    V_ID v = 0;
    if (work) {
      uint32_t chunk = 0;
      v = src.row(i, chunk);
      E_ID b, e;
      src.range(i, v, chunk, b, e);
      float acc = gather_edges<PR_SUM>(a, oldv, b + tq, e, BLOCK);
      acc = V::reduce_wave(acc);
      if (lane == 0) lds[wid] = acc;
    }
    __syncthreads();
    if (work && tq == 0) {
      float acc = lds[0];
      for (int w = 1; w < BLOCK / WAVE; w++) acc = V::comb(acc, lds[w]);
      V::atom(&newv[v], acc);
    }
    __syncthreads();
  }
}

template <int KS, int KW>
__global__ void __launch_bounds__(WIDE_BLOCK, 8)
    pull_slots_stream_hot_wide_kernel(SlotBins s, SlotStream st, PullArgs p,
                                      V_ID lo, V_ID hi) {
  uint32_t blk = blockIdx.x;
  bool stream = blk >= s.g2 + s.g1;
  float* hot = wide_lds() + (stream ? WIDE_TILE_FLOATS : 0);
  uint32_t k = stream ? KS : KW;
  const float* oldv = (const float*)p.oldv;
  for (uint32_t i = threadIdx.x; i < k; i += WIDE_BLOCK) {
    uint64_t pos = (uint64_t)lo + i;
    hot[i] = pos < hi ? oldv[pos] : 0.0f;
  }
  __syncthreads();
  if (blk < s.g2) {
    PullArgsWide<KW, 0> a{p, lo};
    pull_chunk_role_wide(blk, s.g2, s.n2, SlotRows{s.cidx2, s.rng2}, a,
                         wide_lds() + KW);
  } else if (!stream) {
    PullArgsWide<KW, 0> a{p, lo};
    pull_wave_role<PR_SUM>(blk - s.g2, s.g1, s.n1, SlotRows{s.cidx1, s.rng1},
                           a);
  } else {
    PullArgsWide<KS, WIDE_TILE_FLOATS> a{p, lo};
    pull_stream_tiles<PR_SUM, WIDE_NW>(
        blk - s.g2 - s.g1, gridDim.x - s.g2 - s.g1, st, s.cidx0, a,
        (float(*)[TILE_EDGES])wide_lds());
  }
}

// ---- slot / active-row builders (init time, once per graph) ----

// flags[v] = 1 when local row v has any in-edge in the partition
__global__ void pull_active_flags_kernel(V_ID vp, const E_ID* row_ptr,
                                         uint32_t* flags) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < vp;
       v += stride)
    flags[v] = row_ptr[v + 1] != row_ptr[v];
}

// ends = inclusive scan of flags: an active row's compact index is
// ends[v] - 1; scatter the ascending active list
__global__ void pull_active_list_kernel(V_ID vp, const uint32_t* flags,
                                        const E_ID* ends, V_ID* active) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < vp;
       v += stride)
    if (flags[v]) active[ends[v] - 1] = (V_ID)v;
}

template <typename RowT>
__global__ void pull_build_slots_kernel(uint32_t n, const V_ID* bin,
                                        const RowT* row_ptr, const E_ID* ends,
                                        V_ID* cidx, uint2* rng) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    V_ID v = bin[i];
    cidx[i] = (V_ID)(ends[v] - 1);
    rng[i] = make_uint2((uint32_t)row_ptr[v], (uint32_t)row_ptr[v + 1]);
  }
}

template <typename RowT>
__global__ void pull_build_hub_slots_kernel(uint32_t n2, const uint2* bin2,
                                            const RowT* row_ptr,
                                            const E_ID* ends, V_ID* cidx,
                                            uint2* rng) {
  TableChunks<RowT> t{bin2, row_ptr};
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n2;
       i += stride) {
    uint32_t chunk;
    V_ID v = t.row(i, chunk);
    E_ID b, e;
    t.range(i, v, chunk, b, e);
    cidx[i] = (V_ID)(ends[v] - 1);
    rng[i] = make_uint2((uint32_t)b, (uint32_t)e);
  }
}

// ---- stream-role builders (thread bin of one window) ----

// cnt[i] = edges of slot i; its scan is off0
__global__ void pull_slot_counts_kernel(uint32_t n, const uint2* rng,
                                        uint32_t* cnt) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint2 r = rng[i];
    cnt[i] = r.y - r.x;
  }
}

// scol0[off0[i] + j] = col[rng0[i].x + j]: the thread bin's edges made
// contiguous in slot order (wave-bin and hub rows sit between them in col)
__global__ void pull_stream_copy_kernel(uint32_t n0, const uint2* rng0,
                                        const uint32_t* off0,
                                        const V_ID* col, V_ID* scol0) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n0;
       i += stride) {
    uint2 r = rng0[i];
    uint32_t o = off0[i];
    for (uint32_t j = r.x; j < r.y; j++) scol0[o + (j - r.x)] = col[j];
  }
}

// ---- hot order: sources ranked by out-degree inside their src window ----
// pos[v] is a permutation of the vertex ids that maps every src window onto
// itself (out-degree descending, ties by id). The sweeps then run unchanged
// on column copies that hold pos[col[j]] and gather from gold, the rank
// array in that order (gold[pos[v]] = old[v]): a 128-byte line of gold holds
// 32 sources of like heat instead of one hot source and 31 cold ones, so the
// same L2 covers more of a window's gathers. Row sums read the same values
// in the same order as on the id-ordered tables.
constexpr V_ID HOT_NONE = 0xFFFFFFFFu;  // apos: row is never gathered

// hcol[j] = pos[col[j]]
__global__ void pull_hot_col_kernel(uint64_t n, const V_ID* col,
                                    const V_ID* pos, V_ID* hcol) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n;
       j += stride)
    hcol[j] = pos[col[j]];
}

// pull_stream_copy_kernel with pos applied on the way: the stream role's
// hot-ordered column copy straight from the id-ordered col
__global__ void pull_stream_copy_hot_kernel(uint32_t n0, const uint2* rng0,
                                            const uint32_t* off0,
                                            const V_ID* col, const V_ID* pos,
                                            V_ID* scol0) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n0;
       i += stride) {
    uint2 r = rng0[i];
    uint32_t o = off0[i];
    for (uint32_t j = r.x; j < r.y; j++) scol0[o + (j - r.x)] = pos[col[j]];
  }
}

// apos[i] = pos of active row i, or HOT_NONE when it has no out-edge (no
// col entry names it, so its gold cell is never read)
__global__ void pull_hot_apos_kernel(V_ID na, const V_ID* active,
                                     const V_ID* pos, const V_ID* deg,
                                     V_ID row_left, V_ID* apos) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < na;
       i += stride) {
    uint64_t g = (uint64_t)row_left + active[i];
    apos[i] = deg[g] != 0 ? pos[g] : HOT_NONE;
  }
}

// gold[pos[v]] = old[v] over all nv vertices
__global__ void pull_hot_scatter_kernel(V_ID nv, const V_ID* pos,
                                        const float* old, float* gold) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride)
    gold[pos[v]] = old[v];
}

// Greedy cut of the 64-slot group g into tiles of at most TILE_EDGES edges;
// returns the tile count and, with `out`, writes each tile's first slot.
// One slot is below T1 <= TILE_EDGES edges, so every cut makes progress.
__device__ __forceinline__ uint32_t cut_tile_group(uint64_t g, uint32_t n0,
                                                   const uint32_t* off0,
                                                   uint32_t* out) {
  uint64_t s = g * TILE_GROUP;
  uint64_t send = s + TILE_GROUP < n0 ? s + TILE_GROUP : n0;
  uint32_t begin = off0[s], nt = 1;
  if (out) out[0] = (uint32_t)s;
  for (uint64_t i = s; i < send; i++) {
    if (off0[i + 1] - begin > TILE_EDGES) {  // slot i opens the next tile
      begin = off0[i];
      if (out) out[nt] = (uint32_t)i;
      nt++;
    }
  }
  return nt;
}

__global__ void pull_stream_tile_counts_kernel(uint32_t n0,
                                               const uint32_t* off0,
                                               uint32_t* cnt) {
  uint64_t ngroups = ((uint64_t)n0 + TILE_GROUP - 1) / TILE_GROUP;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       g < ngroups; g += stride)
    cnt[g] = cut_tile_group(g, n0, off0, nullptr);
}

// ends = inclusive scan of the per-group tile counts
__global__ void pull_stream_tile_fill_kernel(uint32_t n0,
                                             const uint32_t* off0,
                                             const E_ID* ends,
                                             uint32_t* tile0) {
  uint64_t ngroups = ((uint64_t)n0 + TILE_GROUP - 1) / TILE_GROUP;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       g < ngroups; g += stride) {
    cut_tile_group(g, n0, off0, tile0 + (g ? ends[g - 1] : 0));
    if (g == ngroups - 1) tile0[ends[g]] = n0;
  }
}

template <PullMode M, typename RowT>
static void pull_iter(hipStream_t s, uint32_t n0, const V_ID* bin0,
                      uint32_t n1, const V_ID* bin1, uint32_t n2,
                      const uint2* bin2, uint32_t nbig, const V_ID* bin2v,
                      const PullArgs& a) {
  if (nbig) {
    hipLaunchKernelGGL((pull_chunk_kernel<M, RowT>),
                       dim3(n2 > MAX_GRID ? MAX_GRID : n2), dim3(BLOCK), 0, s,
                       n2, bin2, a);
  }
  if (n1)
    hipLaunchKernelGGL((pull_wave_kernel<M, RowT>),
                       dim3(grid_for((uint64_t)n1 * WAVE)), dim3(BLOCK), 0, s,
                       n1, bin1, a);
  if (n0)
    hipLaunchKernelGGL((pull_thread_kernel<M, RowT>), dim3(grid_for(n0)),
                       dim3(BLOCK), 0, s, n0, bin0, a);
}

template <typename RowT>
static void pull_iter_w(hipStream_t s, uint32_t n0, const V_ID* bin0,
                        uint32_t n1, const V_ID* bin1, uint32_t n2,
                        const uint2* bin2, uint32_t nbig,
                        const PullArgsW& a) {
  if (nbig)
    hipLaunchKernelGGL(pull_chunk_w_kernel<RowT>,
                       dim3(n2 > MAX_GRID ? MAX_GRID : n2), dim3(BLOCK), 0, s,
                       n2, bin2, a);
  if (n1)
    hipLaunchKernelGGL(pull_wave_w_kernel<RowT>,
                       dim3(grid_for((uint64_t)n1 * WAVE)), dim3(BLOCK), 0, s,
                       n1, bin1, a);
  if (n0)
    hipLaunchKernelGGL(pull_thread_w_kernel<RowT>, dim3(grid_for(n0)),
                       dim3(BLOCK), 0, s, n0, bin0, a);
}

// PR epilogue over the whole partition: pr = (1-a)/nv + a*sum, stored
// divided by out-degree (pagerank_gpu.cu:97-100, :255-259). Covers rows
// with no in-edges too (sum stays 0 from the seed).
__device__ __forceinline__ float finish_pr(float sum, V_ID d,
                                           float init_rank) {
  float pr = init_rank + PR_ALPHA * sum;
  return d != 0 ? pr / (float)d : pr;
}

__global__ void pull_finish_pr_kernel(V_ID vp, float* newv,
                                      const V_ID* deg, V_ID row_left,
                                      float init_rank) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < vp;
       v += stride)
    newv[v] = finish_pr(newv[v], deg[row_left + v], init_rank);
}

// PR epilogue over the active rows only, straight into the replicated rank
// array: out[row_left + active[i]] = finish(acc[i]). Rows outside `active`
// keep the constant pull_fill_inactive_pr_kernel gave them.
__global__ void pull_finish_pr_active_kernel(V_ID na, const V_ID* active,
                                             const float* acc, float* out,
                                             const V_ID* deg, V_ID row_left,
                                             float init_rank) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < na;
       i += stride) {
    uint64_t g = (uint64_t)row_left + active[i];
    out[g] = finish_pr(acc[i], deg[g], init_rank);
  }
}

// pull_finish_pr_active_kernel that also keeps the hot-ordered gather table
// current: the row's new value goes to out[] as before and to gold[apos[i]]
// (apos: coalesced stream next to active; rows nobody gathers skip the
// scattered store).
__global__ void pull_finish_pr_active_hot_kernel(
    V_ID na, const V_ID* active, const V_ID* apos, const float* acc,
    float* out, float* gold, const V_ID* deg, V_ID row_left,
    float init_rank) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < na;
       i += stride) {
    uint64_t g = (uint64_t)row_left + active[i];
    V_ID p = apos[i];
    float r = finish_pr(acc[i], deg[g], init_rank);
    out[g] = r;
    if (p != HOT_NONE) gold[p] = r;
  }
}

// Rows with no in-edge: their sum is 0 in every iteration, so the stored
// rank is the constant finish(0). Written once, not per iteration.
__global__ void pull_fill_inactive_pr_kernel(V_ID vp, const E_ID* row_ptr,
                                             float* out, const V_ID* deg,
                                             V_ID row_left,
                                             float init_rank) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < vp;
       v += stride) {
    if (row_ptr[v + 1] != row_ptr[v]) continue;
    uint64_t g = (uint64_t)row_left + v;
    out[g] = finish_pr(0.0f, deg[g], init_rank);
  }
}

}  // namespace lux

// ---------------- C ABI ----------------

using namespace lux;

extern "C" {

void lux_gpu_build_bins(uint64_t stream, uint32_t vp, const E_ID* row_ptr,
                        V_ID* bin0, V_ID* bin1, uint2* bin2, V_ID* bin2v,
                        uint32_t* counters /*pre-zeroed u32[4]*/) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(build_bins_kernel, dim3(grid_for(vp)), dim3(BLOCK), 0, s,
                     vp, row_ptr, bin0, bin1, bin2, bin2v, counters);
  LUX_POST_LAUNCH(stream);
}

// mode: 0 = PageRank float-sum, 1 = u32 min (SSSP dense), 2 = u32 max (CC).
// row_u32: row_ptr is u32[vp+1] (block-local offsets) instead of u64.
void lux_gpu_pull_iter(uint64_t stream, int mode, uint32_t n0,
                       const V_ID* bin0, uint32_t n1, const V_ID* bin1,
                       uint32_t n2, const uint2* bin2, uint32_t nbig,
                       const V_ID* bin2v, const void* row_ptr, int row_u32,
                       const V_ID* col, const void* oldv, void* newv,
                       const V_ID* deg, V_ID row_left, float init_rank) {
  hipStream_t s = (hipStream_t)stream;
  PullArgs a{row_ptr, col, oldv, newv, deg, row_left, init_rank};
#define LUX_PI(M_)                                                            do {                                                                          if (row_u32)                                                                  pull_iter<M_, uint32_t>(s, n0, bin0, n1, bin1, n2, bin2, nbig, bin2v,                               a);                                               else                                                                          pull_iter<M_, uint64_t>(s, n0, bin0, n1, bin1, n2, bin2, nbig, bin2v,                               a);                                             } while (0)
  switch (mode) {
    case 0: LUX_PI(PR_SUM); break;
    case 1: LUX_PI(LAB_MIN); break;
    case 2: LUX_PI(LAB_MAX); break;
  }
#undef LUX_PI
  LUX_POST_LAUNCH(stream);
}

// Weighted SSSP dense sweep (LAB_MIN_W): newv[v] = min(newv[v], min over
// in-edges j of sat(oldv[col[j]] + wgt[j])), INF sources skipped. wgt is
// indexed like col. Same bins, row tables and seed contract as
// lux_gpu_pull_iter's label modes; no settled-row skip.
void lux_gpu_pull_iter_w(uint64_t stream, uint32_t n0, const V_ID* bin0,
                         uint32_t n1, const V_ID* bin1, uint32_t n2,
                         const uint2* bin2, uint32_t nbig,
                         const V_ID* bin2v, const void* row_ptr, int row_u32,
                         const V_ID* col, const WeightType* wgt,
                         const uint32_t* oldv, uint32_t* newv,
                         V_ID row_left) {
  hipStream_t s = (hipStream_t)stream;
  (void)bin2v;
  PullArgsW a{{row_ptr, col, oldv, newv, nullptr, row_left, 0.0f}, wgt};
  if (row_u32)
    pull_iter_w<uint32_t>(s, n0, bin0, n1, bin1, n2, bin2, nbig, a);
  else
    pull_iter_w<uint64_t>(s, n0, bin0, n1, bin1, n2, bin2, nbig, a);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_pull_finish_pr(uint64_t stream, V_ID vp, float* newv,
                            const V_ID* deg, V_ID row_left,
                            float init_rank) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pull_finish_pr_kernel, dim3(grid_for(vp)), dim3(BLOCK),
                     0, s, vp, newv, deg, row_left, init_rank);
  LUX_POST_LAUNCH(stream);
}

// ---- slot path (PR_SUM): builders, merged sweep, active-row epilogue ----

void lux_gpu_pull_active_flags(uint64_t stream, V_ID vp, const E_ID* row_ptr,
                               uint32_t* flags) {
  hipLaunchKernelGGL(pull_active_flags_kernel, dim3(grid_for(vp)),
                     dim3(BLOCK), 0, (hipStream_t)stream, vp, row_ptr, flags);
  LUX_POST_LAUNCH(stream);
}

// ends: inclusive scan of flags (lux_gpu_scan_end_offsets); active: u32[na]
void lux_gpu_pull_active_list(uint64_t stream, V_ID vp, const uint32_t* flags,
                              const E_ID* ends, V_ID* active) {
  hipLaunchKernelGGL(pull_active_list_kernel, dim3(grid_for(vp)), dim3(BLOCK),
                     0, (hipStream_t)stream, vp, flags, ends, active);
  LUX_POST_LAUNCH(stream);
}

// One bin list (bin0 or bin1) -> compact indices + edge ranges. Offsets
// must fit u32 (always true for row_u32 tables; the caller checks ep for
// u64 ones).
void lux_gpu_pull_build_slots(uint64_t stream, uint32_t n, const V_ID* bin,
                              const void* row_ptr, int row_u32,
                              const E_ID* ends, V_ID* cidx, uint2* rng) {
  if (!n) return;
  hipStream_t s = (hipStream_t)stream;
  if (row_u32)
    hipLaunchKernelGGL(pull_build_slots_kernel<uint32_t>, dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, n, bin, (const uint32_t*)row_ptr,
                       ends, cidx, rng);
  else
    hipLaunchKernelGGL(pull_build_slots_kernel<uint64_t>, dim3(grid_for(n)),
                       dim3(BLOCK), 0, s, n, bin, (const uint64_t*)row_ptr,
                       ends, cidx, rng);
  LUX_POST_LAUNCH(stream);
}

// bin2 (row, chunk) entries -> compact index + that chunk's edge range
void lux_gpu_pull_build_hub_slots(uint64_t stream, uint32_t n2,
                                  const uint2* bin2, const void* row_ptr,
                                  int row_u32, const E_ID* ends, V_ID* cidx,
                                  uint2* rng) {
  if (!n2) return;
  hipStream_t s = (hipStream_t)stream;
  if (row_u32)
    hipLaunchKernelGGL(pull_build_hub_slots_kernel<uint32_t>,
                       dim3(grid_for(n2)), dim3(BLOCK), 0, s, n2, bin2,
                       (const uint32_t*)row_ptr, ends, cidx, rng);
  else
    hipLaunchKernelGGL(pull_build_hub_slots_kernel<uint64_t>,
                       dim3(grid_for(n2)), dim3(BLOCK), 0, s, n2, bin2,
                       (const uint64_t*)row_ptr, ends, cidx, rng);
  LUX_POST_LAUNCH(stream);
}

// One PR_SUM sweep of one src window (or the unblocked CSC) in ONE launch:
// acc[cidx] = acc[cidx] + sum over the slot's edges of oldv[col[j]].
void lux_gpu_pull_slots_iter(uint64_t stream, uint32_t n0, const V_ID* cidx0,
                             const uint2* rng0, uint32_t n1,
                             const V_ID* cidx1, const uint2* rng1,
                             uint32_t n2, const V_ID* cidx2,
                             const uint2* rng2, const V_ID* col,
                             const float* oldv, float* acc) {
  // per-role grids: what the three separate launches use
  uint32_t g2 = n2 ? (n2 > (uint32_t)MAX_GRID ? MAX_GRID : n2) : 0;
  uint32_t g1 = n1 ? grid_for((uint64_t)n1 * WAVE) : 0;
  uint32_t g0 = n0 ? grid_for(n0) : 0;
  if (g0 + g1 + g2 == 0) return;
  SlotBins sb{n0, n1, n2, g1, g2, cidx0, cidx1, cidx2, rng0, rng1, rng2};
  PullArgs a{nullptr, col, oldv, acc, nullptr, 0, 0.0f};
  hipLaunchKernelGGL(pull_slots_kernel<PR_SUM>, dim3(g0 + g1 + g2),
                     dim3(BLOCK), 0, (hipStream_t)stream, sb, a);
  LUX_POST_LAUNCH(stream);
}

// ---- stream role: builders and the sweep that runs it ----

// cnt[i] = rng[i].y - rng[i].x (u32[n]); scanned by the caller into off0
void lux_gpu_pull_slot_counts(uint64_t stream, uint32_t n, const uint2* rng,
                              uint32_t* cnt) {
  if (!n) return;
  hipLaunchKernelGGL(pull_slot_counts_kernel, dim3(grid_for(n)), dim3(BLOCK),
                     0, (hipStream_t)stream, n, rng, cnt);
  LUX_POST_LAUNCH(stream);
}

// off0: u32[n0+1] exclusive scan of the counts; scol0: u32[off0[n0]]
void lux_gpu_pull_stream_copy(uint64_t stream, uint32_t n0, const uint2* rng0,
                              const uint32_t* off0, const V_ID* col,
                              V_ID* scol0) {
  if (!n0) return;
  hipLaunchKernelGGL(pull_stream_copy_kernel, dim3(grid_for(n0)), dim3(BLOCK),
                     0, (hipStream_t)stream, n0, rng0, off0, col, scol0);
  LUX_POST_LAUNCH(stream);
}

// cnt: u32[ceil(n0 / 64)] tiles per 64-slot group
void lux_gpu_pull_stream_tile_counts(uint64_t stream, uint32_t n0,
                                     const uint32_t* off0, uint32_t* cnt) {
  if (!n0) return;
  uint64_t ngroups = ((uint64_t)n0 + TILE_GROUP - 1) / TILE_GROUP;
  hipLaunchKernelGGL(pull_stream_tile_counts_kernel, dim3(grid_for(ngroups)),
                     dim3(BLOCK), 0, (hipStream_t)stream, n0, off0, cnt);
  LUX_POST_LAUNCH(stream);
}

// ends: inclusive scan of cnt (nt = its last entry); tile0: u32[nt+1]
void lux_gpu_pull_stream_tile_fill(uint64_t stream, uint32_t n0,
                                   const uint32_t* off0, const E_ID* ends,
                                   uint32_t* tile0) {
  if (!n0) return;
  uint64_t ngroups = ((uint64_t)n0 + TILE_GROUP - 1) / TILE_GROUP;
  hipLaunchKernelGGL(pull_stream_tile_fill_kernel, dim3(grid_for(ngroups)),
                     dim3(BLOCK), 0, (hipStream_t)stream, n0, off0, ends,
                     tile0);
  LUX_POST_LAUNCH(stream);
}

// lux_gpu_pull_slots_iter with the thread bin run by the stream role: one
// wave per tile instead of one thread per slot. Same sums, bit for bit.
void lux_gpu_pull_slots_stream_iter(
    uint64_t stream, uint32_t n0, const V_ID* cidx0, uint32_t nt,
    const uint32_t* tile0, const uint32_t* off0, const V_ID* scol0,
    uint32_t n1, const V_ID* cidx1, const uint2* rng1, uint32_t n2,
    const V_ID* cidx2, const uint2* rng2, const V_ID* col, const float* oldv,
    float* acc) {
  uint32_t g2 = n2 ? (n2 > (uint32_t)MAX_GRID ? MAX_GRID : n2) : 0;
  uint32_t g1 = n1 ? grid_for((uint64_t)n1 * WAVE) : 0;
  uint32_t g0 = n0 && nt ? grid_for((uint64_t)nt * WAVE) : 0;
  if (g0 + g1 + g2 == 0) return;
  SlotBins sb{n0, n1, n2, g1, g2, cidx0, cidx1, cidx2, nullptr, rng1, rng2};
  SlotStream st{g0 ? nt : 0, tile0, off0, scol0};
  PullArgs a{nullptr, col, oldv, acc, nullptr, 0, 0.0f};
  hipLaunchKernelGGL(pull_slots_stream_kernel<PR_SUM>, dim3(g0 + g1 + g2),
                     dim3(BLOCK), 0, (hipStream_t)stream, sb, st, a);
  LUX_POST_LAUNCH(stream);
}

// lux_gpu_pull_slots_stream_iter on hot-ordered tables (scol0 / col hold
// positions, gold is the gather table in that order) with the k hottest
// sources of the window [lo, hi) kept in LDS; k: 2048 (16 KB with the stream
// role's tile buffer: still 8 workgroups per CU) or 4096 (6 per CU).
// Returns 0, or -1 for any other k (nothing is launched).
int lux_gpu_pull_slots_stream_hot_iter(
    uint64_t stream, uint32_t n0, const V_ID* cidx0, uint32_t nt,
    const uint32_t* tile0, const uint32_t* off0, const V_ID* scol0,
    uint32_t n1, const V_ID* cidx1, const uint2* rng1, uint32_t n2,
    const V_ID* cidx2, const uint2* rng2, const V_ID* col, const float* gold,
    float* acc, V_ID lo, V_ID hi, int k) {
  if (k != 2048 && k != 4096) return -1;
  uint32_t g2 = n2 ? (n2 > (uint32_t)MAX_GRID ? MAX_GRID : n2) : 0;
  uint32_t g1 = n1 ? grid_for((uint64_t)n1 * WAVE) : 0;
  uint32_t g0 = n0 && nt ? grid_for((uint64_t)nt * WAVE) : 0;
  if (g0 + g1 + g2 == 0) return 0;
  SlotBins sb{n0, n1, n2, g1, g2, cidx0, cidx1, cidx2, nullptr, rng1, rng2};
  SlotStream st{g0 ? nt : 0, tile0, off0, scol0};
#define LUX_HOT(K_)                                                           \
  do {                                                                        \
    PullArgsHot<K_> a{{nullptr, col, gold, acc, nullptr, 0, 0.0f}, lo};       \
    hipLaunchKernelGGL((pull_slots_stream_hot_kernel<PR_SUM, K_>),            \
                       dim3(g0 + g1 + g2), dim3(BLOCK), 0,                    \
                       (hipStream_t)stream, sb, st, a, hi);                   \
  } while (0)
  switch (k) {
    case 2048: LUX_HOT(2048); break;
    default: LUX_HOT(4096); break;
  }
#undef LUX_HOT
  LUX_POST_LAUNCH(stream);
  return 0;
}

// Workgroups per role for a grid of g: in proportion to the roles' edge
// counts, at least one for a role with work, none for a role without, and no
// more than the role has trips for (per[r] entries per workgroup and trip).
static void wide_split(uint32_t g, const uint64_t edges[3],
                       const uint64_t work[3], const uint32_t per[3],
                       uint32_t out[3]) {
  uint64_t tot = 0;
  uint32_t roles = 0, sum = 0;
  for (int r = 0; r < 3; r++)
    if (work[r]) tot += edges[r] ? edges[r] : 1, roles++;
  if (g < roles) g = roles;
  for (int r = 0; r < 3; r++) {
    uint64_t e = edges[r] ? edges[r] : 1;
    out[r] = work[r] ? (uint32_t)((double)g * (double)e / (double)tot) : 0;
    if (work[r] && !out[r]) out[r] = 1;
    sum += out[r];
  }
  while (sum != g) {  // rounding: give to / take from the largest share
    int big = 0;
    for (int r = 1; r < 3; r++)
      if (out[r] > out[big]) big = r;
    if (sum < g) out[big]++, sum++;
    else out[big]--, sum--;
  }
  for (int r = 0; r < 3; r++) {
    uint64_t cap = (work[r] + per[r] - 1) / per[r];
    if (out[r] > cap) out[r] = (uint32_t)cap;
  }
}

// lux_gpu_pull_slots_stream_hot_iter by 1024-thread workgroups with a prefix
// of ks sources in the stream role and kw in the wave and chunk roles
// (pull_slots_stream_hot_wide_kernel). ne0 / ne: entries of scol0 / col, for
// the role split. max_groups: 0 = WIDE_GROUPS_PER_CU workgroups per CU;
// else the grid (at least one workgroup per role with work). Returns 0, -1
// for a (ks, kw) that is not instantiated, or -2 if the runtime refuses the
// CU count or the LDS size (nothing is launched either way).
int lux_gpu_pull_slots_stream_hot_wide_iter(
    uint64_t stream, uint32_t n0, const V_ID* cidx0, uint32_t nt,
    const uint32_t* tile0, const uint32_t* off0, const V_ID* scol0,
    uint64_t ne0, uint32_t n1, const V_ID* cidx1, const uint2* rng1,
    uint32_t n2, const V_ID* cidx2, const uint2* rng2, const V_ID* col,
    uint64_t ne, const float* gold, float* acc, V_ID lo, V_ID hi, int ks,
    int kw, uint32_t max_groups) {
  // (4096, 8192) and (8192, 8192) were measured and are not built: 0.7 and
  // 0.6 ms per RMAT-27 iteration behind this pair (BENCHLOG r16.1)
  if (ks != 8192 || kw != 16384) return -1;
  uint32_t g = max_groups;
  if (!g) {
    static const uint32_t dflt = [] {
      int dev = 0, cus = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                dev) != hipSuccess)
        return 0u;
      return (uint32_t)(WIDE_GROUPS_PER_CU * cus);
    }();
    if (!dflt) return -2;
    g = dflt;
  }
  uint64_t work[3] = {n2, n1, n0 && nt ? nt : 0};
  uint64_t e2 = (uint64_t)n2 * CHUNK_EDGES, rest = ne > ne0 ? ne - ne0 : 0;
  if (e2 > rest) e2 = rest;
  uint64_t edges[3] = {e2, rest - e2, ne0};
  uint32_t per[3] = {WIDE_Q, WIDE_NW, WIDE_NW}, gr[3];
  if (!(work[0] | work[1] | work[2])) return 0;
  wide_split(g, edges, work, per, gr);
  uint32_t g2 = gr[0], g1 = gr[1], g0 = gr[2];
  SlotBins sb{n0, n1, n2, g1, g2, cidx0, cidx1, cidx2, nullptr, rng1, rng2};
  SlotStream st{g0 ? nt : 0, tile0, off0, scol0};
  PullArgs a{nullptr, col, gold, acc, nullptr, 0, 0.0f};
#define LUX_WIDE(KS_, KW_)                                                    \
  do {                                                                        \
    auto kern = pull_slots_stream_hot_wide_kernel<KS_, KW_>;                  \
    constexpr uint32_t bytes = wide_lds_bytes<KS_, KW_>();                    \
    static_assert(2 * bytes <= 160 * 1024, "two workgroups per CU");          \
    static const hipError_t raised = hipFuncSetAttribute(                     \
        (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,        \
        (int)bytes);                                                          \
    if (raised != hipSuccess) return -2;                                      \
    hipLaunchKernelGGL(kern, dim3(g0 + g1 + g2), dim3(WIDE_BLOCK), bytes,     \
                       (hipStream_t)stream, sb, st, a, lo, hi);               \
  } while (0)
  LUX_WIDE(8192, 16384);
#undef LUX_WIDE
  LUX_POST_LAUNCH(stream);
  return 0;
}

void lux_gpu_pull_finish_pr_active(uint64_t stream, V_ID na,
                                   const V_ID* active, const float* acc,
                                   float* out, const V_ID* deg, V_ID row_left,
                                   float init_rank) {
  if (!na) return;
  hipLaunchKernelGGL(pull_finish_pr_active_kernel, dim3(grid_for(na)),
                     dim3(BLOCK), 0, (hipStream_t)stream, na, active, acc,
                     out, deg, row_left, init_rank);
  LUX_POST_LAUNCH(stream);
}

// ---- hot order (sources by out-degree inside each src window) ----

// hcol[j] = pos[col[j]], j < n: one window's column copy in hot order
void lux_gpu_pull_hot_col(uint64_t stream, uint64_t n, const V_ID* col,
                          const V_ID* pos, V_ID* hcol) {
  if (!n) return;
  hipLaunchKernelGGL(pull_hot_col_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     (hipStream_t)stream, n, col, pos, hcol);
  LUX_POST_LAUNCH(stream);
}

// lux_gpu_pull_stream_copy with scol0 = pos[...] of the same col entries
void lux_gpu_pull_stream_copy_hot(uint64_t stream, uint32_t n0,
                                  const uint2* rng0, const uint32_t* off0,
                                  const V_ID* col, const V_ID* pos,
                                  V_ID* scol0) {
  if (!n0) return;
  hipLaunchKernelGGL(pull_stream_copy_hot_kernel, dim3(grid_for(n0)),
                     dim3(BLOCK), 0, (hipStream_t)stream, n0, rng0, off0, col,
                     pos, scol0);
  LUX_POST_LAUNCH(stream);
}

// apos: u32[na], pos of every active row (0xFFFFFFFF: out-degree 0)
void lux_gpu_pull_hot_apos(uint64_t stream, V_ID na, const V_ID* active,
                           const V_ID* pos, const V_ID* deg, V_ID row_left,
                           V_ID* apos) {
  if (!na) return;
  hipLaunchKernelGGL(pull_hot_apos_kernel, dim3(grid_for(na)), dim3(BLOCK), 0,
                     (hipStream_t)stream, na, active, pos, deg, row_left,
                     apos);
  LUX_POST_LAUNCH(stream);
}

// gold[pos[v]] = old[v], v < nv (pos: a permutation of 0..nv-1)
void lux_gpu_pull_hot_scatter(uint64_t stream, V_ID nv, const V_ID* pos,
                              const float* old, float* gold) {
  if (!nv) return;
  hipLaunchKernelGGL(pull_hot_scatter_kernel, dim3(grid_for(nv)), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, pos, old, gold);
  LUX_POST_LAUNCH(stream);
}

// lux_gpu_pull_finish_pr_active that also stores each row to gold[apos[i]]
void lux_gpu_pull_finish_pr_active_hot(uint64_t stream, V_ID na,
                                       const V_ID* active, const V_ID* apos,
                                       const float* acc, float* out,
                                       float* gold, const V_ID* deg,
                                       V_ID row_left, float init_rank) {
  if (!na) return;
  hipLaunchKernelGGL(pull_finish_pr_active_hot_kernel, dim3(grid_for(na)),
                     dim3(BLOCK), 0, (hipStream_t)stream, na, active, apos,
                     acc, out, gold, deg, row_left, init_rank);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_pull_fill_inactive_pr(uint64_t stream, V_ID vp,
                                   const E_ID* row_ptr, float* out,
                                   const V_ID* deg, V_ID row_left,
                                   float init_rank) {
  if (!vp) return;
  hipLaunchKernelGGL(pull_fill_inactive_pr_kernel, dim3(grid_for(vp)),
                     dim3(BLOCK), 0, (hipStream_t)stream, vp, row_ptr, out,
                     deg, row_left, init_rank);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
