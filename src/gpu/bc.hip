// Single-source betweenness centrality (Brandes dependency accumulation):
// level-ordered work lists and the sigma / delta accumulation kernels for
// gfx950. No reference equivalent.
//
// Definition (directed graph, source s, hop depths depth[] from the BFS):
//   sigma[s] = 1; for v at depth d > 0, sigma[v] = sum of sigma[u] over the
//   in-edges u->v with depth[u] == d-1;
//   for u at depth d, delta[u] = sum over the out-edges u->v with
//   depth[v] == d+1 of sigma[u]/sigma[v] * (1 + delta[v]).
// Every occurrence of a parallel edge is a term; a self-loop never passes
// the depth test; unreached vertices keep sigma = delta = 0; delta[s] is
// stored as 0. Values are fp32.
//
// Level order (lux_gpu_bc_order_hist / _scatter, run once over the CSC row
// table for the forward pass and once over the push CSR's for the backward
// pass): a counting sort of the reached rows by key = depth*3 + bin, bin
// from the row's degree with the pull kernels' thresholds. The list is u32
// words: a thread- or wave-bin row is one word (its id), a hub row is one
// {row, chunk} word pair per CHUNK_EDGES-edge chunk. Counts and offsets
// are in words.
//
// Accumulate (lux_gpu_bc_level): one launch per level and direction; each
// workgroup takes its role from blockIdx.x, chunk blocks first. Every edge
// costs one 8-byte gather of the neighbour's record {depth, value}: the
// value is sigma during the forward pass; the backward pass replaces it,
// level by level, with q = (1 + delta)/sigma, so level d computes
// delta[u] = sigma[u] * (sum of q[v] over depth d+1 out-neighbours). Rows
// of one level only ever store the value word of their own record, and a
// neighbour of the same level fails the depth test, so the stores race
// with no read that uses them.
#include "gpu_common.h"

namespace lux {

constexpr V_ID T1 = 32;
constexpr V_ID T2 = 2048;
constexpr V_ID CHUNK_EDGES = 8192;

// keys (3 * levels) the order kernels aggregate in LDS; deeper traversals
// spread over so many counters that plain global atomics do not contend
constexpr uint32_t ORDER_KEYS = 768;
constexpr int ORDER_ITEMS = 4;  // rows per thread and scatter tile

// ---------------- records ----------------

__global__ void bc_init_kernel(V_ID nv, V_ID source, const uint32_t* depth,
                               uint2* rec, float* sigma, float* delta) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    float s = v == source ? 1.0f : 0.0f;
    rec[v] = make_uint2(depth[v], __float_as_uint(s));
    sigma[v] = s;
    delta[v] = 0.0f;
  }
}

// ---------------- level order ----------------

// key and list words of row v; words == 0: the row is not listed (unreached,
// or deeper than the `levels` the BFS reported)
__device__ __forceinline__ uint32_t bc_row_words(uint32_t d, uint32_t levels,
                                                 E_ID deg, uint32_t& key,
                                                 uint32_t& nchunks) {
  nchunks = 0;
  key = 0;
  if (d >= levels) return 0;
  // degree-0 rows are listed too (thread bin): a leaf still publishes q
  uint32_t bin = deg < T1 ? 0 : (deg < T2 ? 1 : 2);
  key = d * 3 + bin;
  if (bin < 2) return 1;
  nchunks = (uint32_t)((deg + CHUNK_EDGES - 1) / CHUNK_EDGES);
  return 2 * nchunks;
}

template <bool LDS>
__global__ void bc_order_hist_kernel(V_ID nv, const uint32_t* depth,
                                     const E_ID* row_ptr, uint32_t levels,
                                     uint32_t* cnt,
                                     unsigned long long* hubrows) {
  __shared__ uint32_t lcnt[LDS ? ORDER_KEYS : 1];
  uint32_t nkeys = 3 * levels;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < nkeys; k += blockDim.x) lcnt[k] = 0;
    __syncthreads();
  }
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    uint32_t d = depth[v];
    if (d >= levels) continue;
    uint32_t key, nchunks;
    uint32_t words = bc_row_words(d, levels, row_ptr[v + 1] - row_ptr[v],
                                  key, nchunks);
    if (LDS) atomicAdd(&lcnt[key], words);
    else atomicAdd(&cnt[key], words);
    if (nchunks) atomicAdd(&hubrows[d], 1ull);
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nkeys; k += blockDim.x)
      if (lcnt[k]) atomicAdd(&cnt[k], lcnt[k]);
  }
}

// cursor[key] starts at the key's word offset; tiles of BLOCK * ORDER_ITEMS
// rows claim their ranges with one global atomic per key per tile
template <bool LDS>
__global__ void bc_order_scatter_kernel(V_ID nv, const uint32_t* depth,
                                        const E_ID* row_ptr, uint32_t levels,
                                        unsigned long long* cursor,
                                        uint32_t* list) {
  __shared__ uint32_t lcnt[LDS ? ORDER_KEYS : 1];
  __shared__ unsigned long long lbase[LDS ? ORDER_KEYS : 1];
  constexpr uint64_t TILE = (uint64_t)BLOCK * ORDER_ITEMS;
  uint32_t nkeys = 3 * levels;
  for (uint64_t tile = blockIdx.x * TILE; tile < nv;
       tile += (uint64_t)gridDim.x * TILE) {
    if (LDS) {
      for (uint32_t k = threadIdx.x; k < nkeys; k += blockDim.x) lcnt[k] = 0;
      __syncthreads();
    }
    uint32_t key[ORDER_ITEMS], words[ORDER_ITEMS], nchunks[ORDER_ITEMS];
    unsigned long long pos[ORDER_ITEMS];
#pragma unroll
    for (int i = 0; i < ORDER_ITEMS; i++) {
      uint64_t v = tile + (uint64_t)i * BLOCK + threadIdx.x;
      words[i] = 0;
      key[i] = 0;
      nchunks[i] = 0;
      pos[i] = 0;
      if (v < nv) {
        uint32_t d = depth[v];
        if (d < levels)
          words[i] = bc_row_words(d, levels, row_ptr[v + 1] - row_ptr[v],
                                  key[i], nchunks[i]);
      }
      if (words[i])
        pos[i] = LDS ? atomicAdd(&lcnt[key[i]], words[i])
                     : atomicAdd(&cursor[key[i]],
                                 (unsigned long long)words[i]);
    }
    if (LDS) {
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < nkeys; k += blockDim.x)
        if (lcnt[k])
          lbase[k] = atomicAdd(&cursor[k], (unsigned long long)lcnt[k]);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < ORDER_ITEMS; i++) {
      if (!words[i]) continue;
      V_ID v = (V_ID)(tile + (uint64_t)i * BLOCK + threadIdx.x);
      unsigned long long p = LDS ? lbase[key[i]] + pos[i] : pos[i];
      if (!nchunks[i]) {
        list[p] = v;
      } else {
        for (uint32_t c = 0; c < nchunks[i]; c++) {
          list[p + 2 * c] = v;
          list[p + 2 * c + 1] = c;
        }
      }
    }
    if (LDS) __syncthreads();
  }
}

// ---------------- accumulate ----------------

struct BcLevel {
  const uint32_t* list;     // level-ordered work list (words)
  uint64_t o0, o1, o2, o3;  // word offsets: thread, wave, chunk group, end
  uint32_t g1, g2;          // workgroups of the wave / chunk roles
  const E_ID* row_ptr;      // u64[nv+1]: CSC (forward) / push CSR (backward)
  const V_ID* adj;          // in-neighbours (forward) / out (backward)
  uint2* rec;               // {depth, value} per vertex
  float* sigma;
  float* delta;
  uint32_t d;               // the level
  uint32_t last;            // forward: d is the deepest level
  unsigned long long* edges;  // DAG edges of this level and direction
};

// gather_range's four-way pipeline over 8-byte records: four adjacency
// reads, then four independent record gathers; a neighbour counts iff its
// depth is the wanted one.
__device__ __forceinline__ float bc_gather(const uint2* rec, const V_ID* adj,
                                           E_ID j, E_ID e, E_ID step,
                                           uint32_t want, uint32_t& hits) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (; j + 3 * step < e; j += 4 * step) {
    V_ID c0 = adj[j], c1 = adj[j + step], c2 = adj[j + 2 * step],
         c3 = adj[j + 3 * step];
    uint2 r0 = rec[c0], r1 = rec[c1], r2 = rec[c2], r3 = rec[c3];
    bool h0 = r0.x == want, h1 = r1.x == want, h2 = r2.x == want,
         h3 = r3.x == want;
    a0 += h0 ? __uint_as_float(r0.y) : 0.0f;
    a1 += h1 ? __uint_as_float(r1.y) : 0.0f;
    a2 += h2 ? __uint_as_float(r2.y) : 0.0f;
    a3 += h3 ? __uint_as_float(r3.y) : 0.0f;
    hits += (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;
  }
  for (; j < e; j += step) {
    uint2 r = rec[adj[j]];
    bool h = r.x == want;
    a0 += h ? __uint_as_float(r.y) : 0.0f;
    hits += (uint32_t)h;
  }
  return (a0 + a1) + (a2 + a3);
}

// Row epilogue. Forward: sum is sigma; the record keeps it for the next
// level's gathers, except on the deepest level, whose records no forward
// level reads again: they take q = 1/sigma (delta = 0 there) for the
// backward pass. Backward: sum is the q total; the row reads its own sigma
// out of its record before q replaces it.
template <bool FWD>
__device__ __forceinline__ void bc_finish_row(const BcLevel& a, V_ID v,
                                              float sum) {
  if (FWD) {
    a.sigma[v] = sum;
    a.rec[v].y = __float_as_uint(a.last ? 1.0f / sum : sum);
  } else {
    float sig = __uint_as_float(a.rec[v].y);
    float dl = sig * sum;
    a.delta[v] = a.d == 0 ? 0.0f : dl;  // level 0 is the source alone
    a.rec[v].y = __float_as_uint((1.0f + dl) / sig);
  }
}

// one u64 atomic per workgroup for the level's DAG-edge count
__device__ __forceinline__ void bc_count_edges(const BcLevel& a,
                                               uint32_t hits) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long t = block_reduce_sum((unsigned long long)hits, lds);
  if (threadIdx.x == 0 && t) atomicAdd(a.edges, t);
}

template <bool FWD>
__global__ void __launch_bounds__(BLOCK) bc_level_kernel(BcLevel a) {
  const uint32_t want = FWD ? a.d - 1 : a.d + 1;
  uint32_t blk = blockIdx.x;
  uint32_t hits = 0;
  if (blk < a.g2) {
    // chunk role: one workgroup per {hub row, chunk}; partial sums meet in
    // the row's zeroed sigma (forward) / delta (backward) slot
    __shared__ float lds[BLOCK / WAVE];
    uint64_t n2 = (a.o3 - a.o2) / 2;
    for (uint64_t i = blk; i < n2; i += a.g2) {
      V_ID v = a.list[a.o2 + 2 * i];
      uint32_t chunk = a.list[a.o2 + 2 * i + 1];
      E_ID b = a.row_ptr[v] + (E_ID)chunk * CHUNK_EDGES;
      E_ID e = a.row_ptr[v + 1];
      if (e > b + CHUNK_EDGES) e = b + CHUNK_EDGES;
      float sum = bc_gather(a.rec, a.adj, b + threadIdx.x, e, blockDim.x,
                            want, hits);
      sum = block_reduce_sum(sum, lds);
      if (threadIdx.x == 0) atomicAdd(FWD ? &a.sigma[v] : &a.delta[v], sum);
      __syncthreads();
    }
  } else if (blk < a.g2 + a.g1) {
    // wave role: one wave per row
    int lane = threadIdx.x & (WAVE - 1);
    uint64_t n1 = a.o2 - a.o1;
    uint64_t wave_id = ((uint64_t)(blk - a.g2) * blockDim.x + threadIdx.x) /
                       WAVE;
    uint64_t nwaves = ((uint64_t)a.g1 * blockDim.x) / WAVE;
    for (uint64_t i = wave_id; i < n1; i += nwaves) {
      V_ID v = a.list[a.o1 + i];
      float sum = bc_gather(a.rec, a.adj, a.row_ptr[v] + lane,
                            a.row_ptr[v + 1], WAVE, want, hits);
      sum = wave_reduce_sum(sum);
      if (lane == 0) bc_finish_row<FWD>(a, v, sum);
    }
  } else {
    // thread role: one lane per row
    uint64_t n0 = a.o1 - a.o0;
    uint32_t b0 = blk - a.g2 - a.g1, g0 = gridDim.x - a.g2 - a.g1;
    uint64_t stride = (uint64_t)blockDim.x * g0;
    for (uint64_t i = b0 * (uint64_t)blockDim.x + threadIdx.x; i < n0;
         i += stride) {
      V_ID v = a.list[a.o0 + i];
      float sum = bc_gather(a.rec, a.adj, a.row_ptr[v], a.row_ptr[v + 1], 1,
                            want, hits);
      bc_finish_row<FWD>(a, v, sum);
    }
  }
  bc_count_edges(a, hits);
}

// hub rows of the level, after all their chunks: the entry of chunk 0 runs
// the row's epilogue on the accumulated sum
template <bool FWD>
__global__ void bc_hub_finish_kernel(BcLevel a) {
  uint64_t n2 = (a.o3 - a.o2) / 2;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n2;
       i += stride) {
    if (a.list[a.o2 + 2 * i + 1] != 0) continue;
    V_ID v = a.list[a.o2 + 2 * i];
    bc_finish_row<FWD>(a, v, FWD ? a.sigma[v] : a.delta[v]);
  }
}

// ---------------- check ----------------

// One plain thread per row, from the final arrays only: the forward sum
// over the in-edges and the backward sum over the out-edges, in fp64.
// out[0] counts rows where either misses its stored value by more than
// rtol (relative), or an unreached row is non-zero; out[1] counts reached
// rows whose sigma is not finite.
__global__ void bc_check_kernel(V_ID nv, V_ID source, const E_ID* in_ptr,
                                const V_ID* in_adj, const E_ID* out_ptr,
                                const V_ID* out_adj, const uint32_t* depth,
                                const float* sigma, const float* delta,
                                double rtol, unsigned long long* out) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    uint32_t d = depth[v];
    double sv = sigma[v], dv = delta[v];
    if (d == INF_LABEL) {
      if (sv != 0.0 || dv != 0.0) atomicAdd(&out[0], 1ull);
      continue;
    }
    if (!isfinite(sigma[v])) {
      atomicAdd(&out[1], 1ull);
      continue;
    }
    bool bad = false;
    double want_s = 0.0;
    if (v == source) {
      want_s = 1.0;
      bad = d != 0;
    } else {
      for (E_ID j = in_ptr[v]; j < in_ptr[v + 1]; j++) {
        V_ID u = in_adj[j];
        if (depth[u] != INF_LABEL && depth[u] + 1 == d) want_s += sigma[u];
      }
      if (!(want_s > 0.0)) bad = true;
    }
    if (!(fabs(sv - want_s) <= rtol * want_s)) bad = true;
    double want_d = 0.0;
    for (E_ID j = out_ptr[v]; j < out_ptr[v + 1]; j++) {
      V_ID w = out_adj[j];
      if (depth[w] == d + 1)
        want_d += sv / (double)sigma[w] * (1.0 + (double)delta[w]);
    }
    if (v == source) want_d = 0.0;
    if (!(fabs(dv - want_d) <= rtol * want_d)) bad = true;
    if (bad) atomicAdd(&out[0], 1ull);
  }
}

}  // namespace lux

using namespace lux;

extern "C" {

void lux_gpu_bc_init(uint64_t stream, V_ID nv, V_ID source,
                     const uint32_t* depth, uint2* rec, float* sigma,
                     float* delta) {
  if (!nv) return;
  hipLaunchKernelGGL(bc_init_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, source, depth, rec, sigma,
                     delta);
  LUX_POST_LAUNCH(stream);
}

// cnt: zeroed u32[3 * levels] (list words per key = depth*3 + bin);
// hubrows: zeroed u64[levels] (rows of the chunk bin per level)
void lux_gpu_bc_order_hist(uint64_t stream, V_ID nv, const uint32_t* depth,
                           const E_ID* row_ptr, uint32_t levels,
                           uint32_t* cnt, unsigned long long* hubrows) {
  if (!nv || !levels) return;
  hipStream_t s = (hipStream_t)stream;
  if (3 * (uint64_t)levels <= ORDER_KEYS)
    hipLaunchKernelGGL(bc_order_hist_kernel<true>, dim3(grid_for(nv)),
                       dim3(BLOCK), 0, s, nv, depth, row_ptr, levels, cnt,
                       hubrows);
  else
    hipLaunchKernelGGL(bc_order_hist_kernel<false>, dim3(grid_for(nv)),
                       dim3(BLOCK), 0, s, nv, depth, row_ptr, levels, cnt,
                       hubrows);
  LUX_POST_LAUNCH(stream);
}

// cursor: u64[3 * levels], each key's first word (the exclusive scan of
// cnt), consumed; list: u32[total words]
void lux_gpu_bc_order_scatter(uint64_t stream, V_ID nv, const uint32_t* depth,
                              const E_ID* row_ptr, uint32_t levels,
                              unsigned long long* cursor, uint32_t* list) {
  if (!nv || !levels) return;
  hipStream_t s = (hipStream_t)stream;
  int grid = grid_for(nv, BLOCK * ORDER_ITEMS);
  if (3 * (uint64_t)levels <= ORDER_KEYS)
    hipLaunchKernelGGL(bc_order_scatter_kernel<true>, dim3(grid), dim3(BLOCK),
                       0, s, nv, depth, row_ptr, levels, cursor, list);
  else
    hipLaunchKernelGGL(bc_order_scatter_kernel<false>, dim3(grid),
                       dim3(BLOCK), 0, s, nv, depth, row_ptr, levels, cursor,
                       list);
  LUX_POST_LAUNCH(stream);
}

// One level of one pass. o0..o3: the level's four word offsets into list
// (thread group, wave group, chunk group, end). forward: rows of depth d
// sum sigma over depth d-1 in-neighbours (row_ptr/adj = CSC); backward:
// q over depth d+1 out-neighbours (row_ptr/adj = push CSR). edges: one
// u64 counter, += the edges that passed the depth test.
void lux_gpu_bc_level(uint64_t stream, int forward, const uint32_t* list,
                      uint64_t o0, uint64_t o1, uint64_t o2, uint64_t o3,
                      const E_ID* row_ptr, const V_ID* adj, uint2* rec,
                      float* sigma, float* delta, uint32_t d, int last,
                      unsigned long long* edges) {
  uint64_t n0 = o1 - o0, n1 = o2 - o1, n2 = (o3 - o2) / 2;
  uint32_t g2 = n2 ? (uint32_t)(n2 > (uint64_t)MAX_GRID ? MAX_GRID : n2) : 0;
  uint32_t g1 = n1 ? grid_for(n1 * WAVE) : 0;
  uint32_t g0 = n0 ? grid_for(n0) : 0;
  if (g0 + g1 + g2 == 0) return;
  hipStream_t s = (hipStream_t)stream;
  BcLevel a{list, o0, o1, o2, o3, g1, g2, row_ptr, adj, rec, sigma, delta, d,
            (uint32_t)(last != 0), edges};
  if (forward) {
    hipLaunchKernelGGL(bc_level_kernel<true>, dim3(g0 + g1 + g2), dim3(BLOCK),
                       0, s, a);
    if (n2)
      hipLaunchKernelGGL(bc_hub_finish_kernel<true>, dim3(grid_for(n2)),
                         dim3(BLOCK), 0, s, a);
  } else {
    hipLaunchKernelGGL(bc_level_kernel<false>, dim3(g0 + g1 + g2),
                       dim3(BLOCK), 0, s, a);
    if (n2)
      hipLaunchKernelGGL(bc_hub_finish_kernel<false>, dim3(grid_for(n2)),
                         dim3(BLOCK), 0, s, a);
  }
  LUX_POST_LAUNCH(stream);
}

// out: zeroed u64[2] = {mismatching rows, reached rows with non-finite
// sigma}
void lux_gpu_bc_check(uint64_t stream, V_ID nv, V_ID source,
                      const E_ID* in_ptr, const V_ID* in_adj,
                      const E_ID* out_ptr, const V_ID* out_adj,
                      const uint32_t* depth, const float* sigma,
                      const float* delta, double rtol,
                      unsigned long long* out) {
  if (!nv) return;
  hipLaunchKernelGGL(bc_check_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, source, in_ptr, in_adj, out_ptr,
                     out_adj, depth, sigma, delta, rtol, out);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
