// Batched betweenness centrality: the Brandes sigma and delta passes of
// B = 16 / 32 / 64 sources in one level sweep, state kept vertex-major so
// that one gathered neighbour brings a whole row of columns and the edge
// list, the row lists and the launches are paid once per batch. No reference
// equivalent; the per-source definition is bc.hip's (API.md).
//
// State per batch (column c = source c of the batch, padding columns are
// unreached):
//   dep   u16 [nv][B]  hop depth, 0xFFFF where unreached; never changes
//   val   f32 [nv][B]  sigma during the forward pass; the backward pass
//                      replaces it, level by level, with q = (1 + delta) /
//                      sigma. The only array that is gathered.
//   delta f32 [nv][B]
// Every lane owns 4 consecutive columns: 8 bytes of dep, 16 bytes of val. A
// row belongs to a group of LPR = B / 4 lanes and a wave holds G = 64 / LPR
// groups, as in ppr.hip.
//
// Level lists (bcb_order_*): a row is listed at level d iff one of its
// columns has depth d, so a row has one entry per distinct depth. One lane
// group per row finds the distinct depths in ascending order (group minimum
// above the last one found). key = d * 3 + role; the list is u32 words, a
// group- or wave-role entry is one word, a hub row is one {row, chunk} pair
// per `hub` edges. Histogram, device scan, scatter; the forward lists take
// the roles from the in-degree, the backward lists from the out-degree.
//
// bcb_level_kernel<B, FWD>: one launch per level and pass, the role taken
// from blockIdx.x (group, wave, hub as in ppr_sweep_kernel). A lane's own
// mask is the columns of its row whose depth is d; the depth it accepts of a
// neighbour is d - 1 (forward, in-edges) or d + 1 (backward, out-edges) in
// the masked columns and BCB_NEVER elsewhere, so one packed compare per
// column does both tests. A lane with an empty mask gathers nothing.
//
// Why no read uses a value that is being written: dep never changes. A row
// stores only the columns of its own mask, i.e. entries (v, c) with
// dep[v][c] == d, and each row is listed once per level, so an entry has
// one writer. A gathered entry (u, c) is used only if dep[u][c] == d -+ 1,
// which no row of level d stores; an entry of the same level fails the
// test whatever bits it holds. The backward epilogue reads its own sigma
// before it overwrites it, in the one lane that owns the entry.
//
// No float atomics: hub items leave their partial vectors in scratch and
// bcb_hub_finish_kernel adds them in item order; the summation order of an
// entry depends on its role, B and hub alone, so two runs give the same
// bits. The only atomics are integers (list cursors, the DAG-edge counter).
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t BCB_GROUP = 8;       // longest group-role row
constexpr uint32_t BCB_HUB = 1024;      // default longest wave-role row
constexpr uint32_t BCB_HUB_MIN = 64;
constexpr uint32_t BCB_HUB_MAX = 1u << 20;
constexpr uint32_t BCB_MAX_LEVELS = 65534;
constexpr uint32_t BCB_UNREACHED = 0xFFFF;
constexpr uint32_t BCB_NEVER = 0xFFFE;  // no vertex has this depth
constexpr uint32_t BCB_ORDER_KEYS = 768;  // keys the order kernels keep in LDS
constexpr int BCB_MAX_GRID = 1 << 14;   // blocks per role
constexpr int BCB_NW = BLOCK / WAVE;

struct Dep4 {
  uint32_t c[4];
};

__device__ __forceinline__ Dep4 unpack(uint2 w) {
  return Dep4{{w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16}};
}

// Columns [4 * sub, 4 * sub + 4) of row u.
template <int B>
__device__ __forceinline__ uint2 dep_load(const uint16_t* dep, V_ID u,
                                          int sub) {
  return reinterpret_cast<const uint2*>(dep + (uint64_t)u * B)[sub];
}

template <int B>
__device__ __forceinline__ float4 val_load(const float* val, V_ID u, int sub) {
  return reinterpret_cast<const float4*>(val + (uint64_t)u * B)[sub];
}

__device__ __forceinline__ float4 f4_sum(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// ---------------- prepare ----------------

// One lane per (vertex, four columns): depth is the batch's i32 [k][nv]
// block of MSBFSEngine.depths(), -1 where unreached. Only a source has
// depth 0 in its own column: sigma = 1 there.
__global__ void __launch_bounds__(BLOCK)
bcb_prepare_kernel(V_ID nv, uint32_t B, uint32_t k, const int* depth,
                   uint2* dep, float4* val, float4* delta) {
  const uint32_t lpr = B / 4;
  const uint64_t n = (uint64_t)nv * lpr;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t v = i / lpr;
    const uint32_t c0 = 4 * (uint32_t)(i % lpr);
    uint32_t h[4];
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int d = c0 + j < k ? depth[(uint64_t)(c0 + j) * nv + v] : -1;
      h[j] = d < 0 || d >= (int)BCB_NEVER ? BCB_UNREACHED : (uint32_t)d;
      s[j] = d == 0 ? 1.0f : 0.0f;
    }
    dep[i] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    val[i] = make_float4(s[0], s[1], s[2], s[3]);
    delta[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// ---------------- level lists ----------------

// Calls emit(d) for every distinct depth d < levels of the row, ascending,
// in every lane of the row's group. w: this lane's four depths. The loop is
// wave-uniform: the shuffles stay inside a group, but every lane runs them.
template <int B, typename F>
__device__ __forceinline__ void bcb_row_depths(uint2 w, uint32_t levels,
                                               F emit) {
  constexpr int LPR = B / 4;
  const Dep4 x = unpack(w);
  uint32_t lb = 0;  // depths below lb are done
  for (;;) {
    uint32_t m = BCB_UNREACHED;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x.c[j] >= lb && x.c[j] < m) m = x.c[j];
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
      const uint32_t o = __shfl_xor(m, off, WAVE);
      m = o < m ? o : m;
    }
    const bool go = m < levels;
    if (!__any(go)) break;
    if (go) {
      emit(m);
      lb = m + 1;
    }
  }
}

// list words and key of a row of degree deg at depth d
__device__ __forceinline__ uint32_t bcb_words(uint32_t d, E_ID deg,
                                              uint32_t hub, uint32_t& key) {
  const uint32_t role = deg <= BCB_GROUP ? 0 : (deg <= hub ? 1 : 2);
  key = d * 3 + role;
  return role < 2 ? 1u : 2u * (uint32_t)((deg + hub - 1) / hub);
}

template <int B, bool LDS>
__global__ void __launch_bounds__(BLOCK)
bcb_order_hist_kernel(V_ID nv, const uint16_t* dep, const E_ID* row_ptr,
                      uint32_t levels, uint32_t hub, uint32_t* cnt,
                      unsigned long long* hubrows) {
  constexpr int LPR = B / 4, ROWS = BLOCK / LPR;
  __shared__ uint32_t lcnt[LDS ? BCB_ORDER_KEYS : 1];
  const uint32_t nkeys = 3 * levels;
  const int sub = threadIdx.x % LPR;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < nkeys; k += BLOCK) lcnt[k] = 0;
    __syncthreads();
  }
  // every lane of a block runs the same number of trips (wave-uniform loop
  // inside bcb_row_depths)
  for (uint64_t base = (uint64_t)blockIdx.x * ROWS; base < nv;
       base += (uint64_t)gridDim.x * ROWS) {
    const uint64_t v = base + threadIdx.x / LPR;
    const bool live = v < nv;
    const uint2 w = live ? dep_load<B>(dep, (V_ID)v, sub)
                         : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    const E_ID deg = live ? row_ptr[v + 1] - row_ptr[v] : 0;
    bcb_row_depths<B>(w, levels, [&](uint32_t d) {
      if (sub) return;
      uint32_t key;
      const uint32_t words = bcb_words(d, deg, hub, key);
      if (LDS) atomicAdd(&lcnt[key], words);
      else atomicAdd(&cnt[key], words);
      if (words > 1) atomicAdd(&hubrows[d], 1ull);
    });
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nkeys; k += BLOCK)
      if (lcnt[k]) atomicAdd(&cnt[k], lcnt[k]);
  }
}

// cursor[key] starts at the key's word offset. With the LDS table a tile of
// BLOCK / LPR rows counts its words per key, claims one range per key and
// then places its entries inside it; without it every entry claims its own.
// The order of the entries of a key is not fixed, and nothing depends on it.
template <int B, bool LDS>
__global__ void __launch_bounds__(BLOCK)
bcb_order_scatter_kernel(V_ID nv, const uint16_t* dep, const E_ID* row_ptr,
                         uint32_t levels, uint32_t hub,
                         unsigned long long* cursor, uint32_t* list,
                         uint64_t cap) {
  constexpr int LPR = B / 4, ROWS = BLOCK / LPR;
  __shared__ uint32_t lcnt[LDS ? BCB_ORDER_KEYS : 1];
  __shared__ unsigned long long lbase[LDS ? BCB_ORDER_KEYS : 1];
  const uint32_t nkeys = 3 * levels;
  const int sub = threadIdx.x % LPR;
  for (uint64_t base = (uint64_t)blockIdx.x * ROWS; base < nv;
       base += (uint64_t)gridDim.x * ROWS) {
    const uint64_t v = base + threadIdx.x / LPR;
    const bool live = v < nv;
    const uint2 w = live ? dep_load<B>(dep, (V_ID)v, sub)
                         : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    const E_ID deg = live ? row_ptr[v + 1] - row_ptr[v] : 0;
    if (LDS) {
      for (uint32_t k = threadIdx.x; k < nkeys; k += BLOCK) lcnt[k] = 0;
      __syncthreads();
      bcb_row_depths<B>(w, levels, [&](uint32_t d) {
        if (sub) return;
        uint32_t key;
        const uint32_t words = bcb_words(d, deg, hub, key);
        atomicAdd(&lcnt[key], words);
      });
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < nkeys; k += BLOCK) {
        if (lcnt[k])
          lbase[k] = atomicAdd(&cursor[k], (unsigned long long)lcnt[k]);
        lcnt[k] = 0;
      }
      __syncthreads();
    }
    bcb_row_depths<B>(w, levels, [&](uint32_t d) {
      if (sub) return;
      uint32_t key;
      const uint32_t words = bcb_words(d, deg, hub, key);
      const unsigned long long p =
          LDS ? lbase[key] + atomicAdd(&lcnt[key], words)
              : atomicAdd(&cursor[key], (unsigned long long)words);
      if (p + words > cap) return;  // cannot happen with the hist's table
      if (words == 1) {
        list[p] = (V_ID)v;
      } else {
        for (uint32_t c = 0; 2 * c < words; c++) {
          list[p + 2 * c] = (V_ID)v;
          list[p + 2 * c + 1] = c;
        }
      }
    });
    if (LDS) __syncthreads();  // lbase / lcnt are reused by the next tile
  }
}

// ---------------- the level sweep ----------------

struct BcbRow {
  uint2 want;     // per column: the neighbour depth that counts, or NEVER
  uint32_t mask;  // bit j: column 4 * sub + j of the row is at this level
};

// This lane's part of row v at level a.d.
template <int B, bool FWD>
__device__ __forceinline__ BcbRow bcb_row(const lux_bcb_level& a, V_ID v,
                                          int sub) {
  const Dep4 x = unpack(dep_load<B>(a.dep, v, sub));
  const uint32_t nb = FWD ? a.d - 1 : a.d + 1;
  uint32_t wt[4], mask = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const bool own = x.c[j] == a.d;
    mask |= (uint32_t)own << j;
    wt[j] = own ? nb : BCB_NEVER;
  }
  return BcbRow{make_uint2(wt[0] | (wt[1] << 16), wt[2] | (wt[3] << 16)),
                mask};
}

// acc += the columns of t whose depth in du is the wanted one
__device__ __forceinline__ void bcb_take(float4& acc, uint32_t& hits, uint2 du,
                                         float4 t, uint2 want) {
  const Dep4 x = unpack(du), w = unpack(want);
  const bool h0 = x.c[0] == w.c[0], h1 = x.c[1] == w.c[1],
             h2 = x.c[2] == w.c[2], h3 = x.c[3] == w.c[3];
  acc.x += h0 ? t.x : 0.0f;
  acc.y += h1 ? t.y : 0.0f;
  acc.z += h2 ? t.z : 0.0f;
  acc.w += h3 ? t.w : 0.0f;
  hits += (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;
}

// Row epilogue in the lane that holds the final sums of its four columns;
// stores the masked columns only.
template <int B, bool FWD>
__device__ __forceinline__ void bcb_finish_row(const lux_bcb_level& a, V_ID v,
                                               int sub, uint32_t mask,
                                               float4 s) {
  if (!mask) return;
  float* pv = a.val + (uint64_t)v * B + 4 * sub;
  const float sum[4] = {s.x, s.y, s.z, s.w};
  if (FWD) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((mask >> j) & 1) pv[j] = sum[j];
  } else {
    float* pd = a.delta + (uint64_t)v * B + 4 * sub;
    const float4 s4 = *reinterpret_cast<const float4*>(pv);  // still sigma
    const float sig[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((mask >> j) & 1) {
        const float dl = sig[j] * sum[j];
        pd[j] = dl;
        pv[j] = (1.0f + dl) / sig[j];
      }
  }
}

// Entries [b, end) of the adjacency, summed by the whole wave; the result is
// in every lane of every group. 64 neighbour ids come with one coalesced
// load; group g takes the ids g, g + G, ... and all LPR gathers of a load
// are in flight together. use: this lane gathers (its mask is not empty).
template <int B>
__device__ __forceinline__ float4 bcb_wave_row(const lux_bcb_level& a, E_ID b,
                                               E_ID end, int lane, uint2 want,
                                               bool use, uint32_t& hits) {
  constexpr int LPR = B / 4, G = WAVE / LPR;
  const int grp = lane / LPR, sub = lane % LPR;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (E_ID base = b; base < end; base += WAVE) {
    const E_ID x = base + lane;
    const V_ID nbr = x < end ? a.adj[x] : 0;
    const E_ID left = end - base;
    const int n = left < (E_ID)WAVE ? (int)left : WAVE;
    float4 t[LPR];
    uint2 du[LPR];
#pragma unroll
    for (int s = 0; s < LPR; s++) {
      const int j = s * G + grp;
      const V_ID u = __shfl(nbr, j, WAVE);
      const bool on = use && j < n;
      du[s] = on ? dep_load<B>(a.dep, u, sub)
                 : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
      t[s] = on ? val_load<B>(a.val, u, sub)
                : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int s = 0; s < LPR; s++) bcb_take(acc, hits, du[s], t[s], want);
  }
#pragma unroll
  for (int off = LPR; off < WAVE; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off, WAVE);
    acc.y += __shfl_xor(acc.y, off, WAVE);
    acc.z += __shfl_xor(acc.z, off, WAVE);
    acc.w += __shfl_xor(acc.w, off, WAVE);
  }
  return acc;
}

// Blocks [0, gb) run the group role, [gb, gb + wb) the wave role, the last
// hb the hub items.
template <int B, bool FWD>
__global__ void __launch_bounds__(BLOCK)
bcb_level_kernel(lux_bcb_level a, uint32_t gb, uint32_t wb, uint32_t hb) {
  constexpr int LPR = B / 4, G = WAVE / LPR;
  __shared__ float4 tile[BCB_NW][LPR];
  __shared__ unsigned long long ecnt[BCB_NW];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  const int sub = lane % LPR;
  const uint32_t b = blockIdx.x;
  // the leaf launch of the deepest level gathers nothing: its rows have no
  // deeper neighbour and only publish q = 1 / sigma
  const bool gather = !a.leaf;
  uint32_t hits = 0;
  if (b < gb) {
    const uint64_t n = a.o1 - a.o0;
    for (uint64_t i = (uint64_t)b * (BCB_NW * G) + threadIdx.x / LPR; i < n;
         i += (uint64_t)gb * (BCB_NW * G)) {
      const V_ID v = a.list[a.o0 + i];
      const BcbRow r = bcb_row<B, FWD>(a, v, sub);
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (r.mask && gather) {
        const E_ID end = a.row_ptr[v + 1];
        E_ID e = a.row_ptr[v];
        for (; e + 1 < end; e += 2) {
          const V_ID u0 = a.adj[e], u1 = a.adj[e + 1];
          const uint2 d0 = dep_load<B>(a.dep, u0, sub);
          const uint2 d1 = dep_load<B>(a.dep, u1, sub);
          const float4 t0 = val_load<B>(a.val, u0, sub);
          const float4 t1 = val_load<B>(a.val, u1, sub);
          bcb_take(acc, hits, d0, t0, r.want);
          bcb_take(acc, hits, d1, t1, r.want);
        }
        if (e < end) {
          const V_ID u = a.adj[e];
          bcb_take(acc, hits, dep_load<B>(a.dep, u, sub),
                   val_load<B>(a.val, u, sub), r.want);
        }
      }
      bcb_finish_row<B, FWD>(a, v, sub, r.mask, acc);
    }
  } else if (b < gb + wb) {
    const uint64_t n = a.o2 - a.o1;
    for (uint64_t i = (uint64_t)(b - gb) * BCB_NW + wid; i < n;
         i += (uint64_t)wb * BCB_NW) {
      const V_ID v = a.list[a.o1 + i];
      const BcbRow r = bcb_row<B, FWD>(a, v, sub);
      const E_ID r0 = a.row_ptr[v];
      const float4 acc = bcb_wave_row<B>(
          a, r0, gather ? a.row_ptr[v + 1] : r0, lane, r.want, r.mask != 0,
          hits);
      if (lane < LPR) bcb_finish_row<B, FWD>(a, v, sub, r.mask, acc);
    }
  } else {
    const uint64_t n = (a.o3 - a.o2) / 2;
    for (uint64_t i = b - gb - wb; i < n; i += hb) {
      const V_ID v = a.list[a.o2 + 2 * i];
      const uint32_t c = a.list[a.o2 + 2 * i + 1];
      const BcbRow r = bcb_row<B, FWD>(a, v, sub);
      const E_ID r0 = a.row_ptr[v] + (E_ID)c * a.hub;
      const E_ID rest = a.row_ptr[v + 1] - r0;
      const E_ID len = !gather ? 0 : (rest < a.hub ? rest : (E_ID)a.hub);
      const E_ID q = (len + BCB_NW * WAVE - 1) / (BCB_NW * WAVE) * WAVE;
      const E_ID w0 = (E_ID)wid * q < len ? (E_ID)wid * q : len;
      const E_ID w1 = w0 + q < len ? w0 + q : len;
      const float4 acc = bcb_wave_row<B>(a, r0 + w0, r0 + w1, lane, r.want,
                                         r.mask != 0, hits);
      if (lane < LPR) tile[wid][lane] = acc;
      __syncthreads();
      if (threadIdx.x < LPR) {
        float4 s = tile[0][threadIdx.x];
        for (int w = 1; w < BCB_NW; w++) s = f4_sum(s, tile[w][threadIdx.x]);
        reinterpret_cast<float4*>(a.scratch + i * B)[threadIdx.x] = s;
      }
      __syncthreads();  // tile is reused by the next item
    }
  }
  // the level's DAG edges: one integer atomic per workgroup
  const unsigned long long t =
      block_reduce_sum((unsigned long long)hits, ecnt);
  if (threadIdx.x == 0 && t) atomicAdd(a.edges, t);
}

// One lane group per hub row (the item of its chunk 0): the items' partial
// vectors in item order, then the epilogue.
template <int B, bool FWD>
__global__ void __launch_bounds__(BLOCK)
bcb_hub_finish_kernel(lux_bcb_level a) {
  constexpr int LPR = B / 4;
  const int sub = threadIdx.x % LPR;
  const uint64_t n = (a.o3 - a.o2) / 2;
  for (uint64_t i = (uint64_t)blockIdx.x * (BLOCK / LPR) + threadIdx.x / LPR;
       i < n; i += (uint64_t)gridDim.x * (BLOCK / LPR)) {
    if (a.list[a.o2 + 2 * i + 1] != 0) continue;
    const V_ID v = a.list[a.o2 + 2 * i];
    const E_ID deg = a.row_ptr[v + 1] - a.row_ptr[v];
    const uint64_t items = (deg + a.hub - 1) / a.hub;
    const float4* part = reinterpret_cast<const float4*>(a.scratch + i * B);
    float4 s = part[sub];
    for (uint64_t k = 1; k < items && i + k < n; k++)
      s = f4_sum(s, part[k * LPR + sub]);
    const BcbRow r = bcb_row<B, FWD>(a, v, sub);
    bcb_finish_row<B, FWD>(a, v, sub, r.mask, s);
  }
}

// ---------------- reduce ----------------

// bc[v] += the row sum of delta: one lane group per row, the four in-lane
// columns first, then an xor butterfly over the group (the same pairs in
// every lane, so every lane of the group ends with the same bits).
template <int B>
__global__ void __launch_bounds__(BLOCK)
bcb_reduce_kernel(V_ID nv, const float* delta, float* bc) {
  constexpr int LPR = B / 4, ROWS = BLOCK / LPR;
  const int sub = threadIdx.x % LPR;
  for (uint64_t base = (uint64_t)blockIdx.x * ROWS; base < nv;
       base += (uint64_t)gridDim.x * ROWS) {
    const uint64_t v = base + threadIdx.x / LPR;
    const float4 x = v < nv ? val_load<B>(delta, (V_ID)v, sub)
                            : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float s = (x.x + x.y) + (x.z + x.w);
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) s += __shfl_xor(s, off, WAVE);
    if (sub == 0 && v < nv) bc[v] += s;
  }
}

// ---------------- check ----------------

// One lane per (vertex, column), from the final arrays only and in fp64:
// the forward sum over the serial in-row and the backward sum over the
// serial out-row. No lists, roles, vectors or LDS. out[0] counts entries
// where either misses its stored value by more than rtol (relative), or an
// unreached entry is non-zero; out[1] counts reached entries whose sigma is
// not finite.
__global__ void __launch_bounds__(BLOCK)
bcb_plain_kernel(V_ID nv, uint32_t B, const E_ID* in_ptr, const V_ID* in_adj,
                 const E_ID* out_ptr, const V_ID* out_adj,
                 const uint16_t* dep, const float* sigma, const float* delta,
                 double rtol, unsigned long long* out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t n = (uint64_t)nv * B;
  unsigned long long bad = 0, nonfinite = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t v = i / B, c = i % B;
    const uint32_t d = dep[i];
    const double sv = sigma[i], dv = delta[i];
    if (d == BCB_UNREACHED) {
      if (sv != 0.0 || dv != 0.0) bad++;
      continue;
    }
    if (!isfinite(sigma[i])) {
      nonfinite++;
      continue;
    }
    bool wrong = false;
    double want_s = 0.0;
    if (d == 0) {
      want_s = 1.0;
    } else {
      for (E_ID j = in_ptr[v]; j < in_ptr[v + 1]; j++) {
        const uint64_t u = (uint64_t)in_adj[j] * B + c;
        if ((uint32_t)dep[u] + 1 == d) want_s += sigma[u];
      }
      if (!(want_s > 0.0)) wrong = true;
    }
    if (!(fabs(sv - want_s) <= rtol * want_s)) wrong = true;
    double want_d = 0.0;
    if (d != 0) {
      for (E_ID j = out_ptr[v]; j < out_ptr[v + 1]; j++) {
        const uint64_t w = (uint64_t)out_adj[j] * B + c;
        if ((uint32_t)dep[w] == d + 1)
          want_d += sv / (double)sigma[w] * (1.0 + (double)delta[w]);
      }
    }
    if (!(fabs(dv - want_d) <= rtol * want_d)) wrong = true;
    if (wrong) bad++;
  }
  bad = wave_reduce_sum(bad);
  nonfinite = wave_reduce_sum(nonfinite);
  if (lane == 0 && bad) atomicAdd(&out[0], bad);
  if (lane == 0 && nonfinite) atomicAdd(&out[1], nonfinite);
}

// ---------------- host side ----------------

__host__ bool bcb_width_ok(uint32_t w) { return w == 16 || w == 32 || w == 64; }

__host__ bool bcb_hub_ok(uint32_t hub) {
  return hub >= BCB_HUB_MIN && hub <= BCB_HUB_MAX;
}

__host__ uint32_t bcb_blocks(uint64_t work, uint32_t per_block) {
  const uint64_t g = (work + per_block - 1) / per_block;
  return (uint32_t)(g > (uint64_t)BCB_MAX_GRID ? BCB_MAX_GRID : g);
}

template <int B>
__host__ void bcb_order_hist(hipStream_t s, V_ID nv, const uint16_t* dep,
                             const E_ID* row_ptr, uint32_t levels,
                             uint32_t hub, uint32_t* cnt,
                             unsigned long long* hubrows) {
  const dim3 grid(grid_for(nv, BLOCK / (B / 4)));
  if (3 * levels <= BCB_ORDER_KEYS)
    hipLaunchKernelGGL((bcb_order_hist_kernel<B, true>), grid, dim3(BLOCK), 0,
                       s, nv, dep, row_ptr, levels, hub, cnt, hubrows);
  else
    hipLaunchKernelGGL((bcb_order_hist_kernel<B, false>), grid, dim3(BLOCK), 0,
                       s, nv, dep, row_ptr, levels, hub, cnt, hubrows);
}

template <int B>
__host__ void bcb_order_scatter(hipStream_t s, V_ID nv, const uint16_t* dep,
                                const E_ID* row_ptr, uint32_t levels,
                                uint32_t hub, unsigned long long* cursor,
                                uint32_t* list, uint64_t cap) {
  const dim3 grid(grid_for(nv, BLOCK / (B / 4)));
  if (3 * levels <= BCB_ORDER_KEYS)
    hipLaunchKernelGGL((bcb_order_scatter_kernel<B, true>), grid, dim3(BLOCK),
                       0, s, nv, dep, row_ptr, levels, hub, cursor, list, cap);
  else
    hipLaunchKernelGGL((bcb_order_scatter_kernel<B, false>), grid, dim3(BLOCK),
                       0, s, nv, dep, row_ptr, levels, hub, cursor, list, cap);
}

template <int B, bool FWD>
__host__ int bcb_level(hipStream_t s, const lux_bcb_level* a) {
  constexpr int LPR = B / 4;
  const uint64_t items = (a->o3 - a->o2) / 2;
  const uint32_t gb = bcb_blocks(a->o1 - a->o0, BLOCK / LPR);
  const uint32_t wb = bcb_blocks(a->o2 - a->o1, BCB_NW);
  const uint32_t hb = bcb_blocks(items, 1);
  if (gb + wb + hb == 0) return 0;
  hipLaunchKernelGGL((bcb_level_kernel<B, FWD>), dim3(gb + wb + hb),
                     dim3(BLOCK), 0, s, *a, gb, wb, hb);
  if (!items) return 1;
  hipLaunchKernelGGL((bcb_hub_finish_kernel<B, FWD>),
                     dim3(bcb_blocks(items, BLOCK / LPR)), dim3(BLOCK), 0, s,
                     *a);
  return 2;
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_bcb_group_limit() { return BCB_GROUP; }
uint32_t lux_gpu_bcb_hub_default() { return BCB_HUB; }
uint32_t lux_gpu_bcb_hub_min() { return BCB_HUB_MIN; }
uint32_t lux_gpu_bcb_hub_max() { return BCB_HUB_MAX; }
uint32_t lux_gpu_bcb_max_levels() { return BCB_MAX_LEVELS; }

int lux_gpu_bcb_prepare(uint64_t stream, V_ID nv, uint32_t width, uint32_t k,
                        const int* depth, uint16_t* dep, float* val,
                        float* delta) {
  if (!nv || !bcb_width_ok(width) || k < 1 || k > width || !depth || !dep ||
      !val || !delta)
    return -1;
  hipLaunchKernelGGL(bcb_prepare_kernel,
                     dim3(grid_for((uint64_t)nv * (width / 4))), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, width, k, depth,
                     reinterpret_cast<uint2*>(dep),
                     reinterpret_cast<float4*>(val),
                     reinterpret_cast<float4*>(delta));
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_bcb_order_hist(uint64_t stream, V_ID nv, uint32_t width,
                           const uint16_t* dep, const E_ID* row_ptr,
                           uint32_t levels, uint32_t hub, uint32_t* cnt,
                           unsigned long long* hubrows) {
  if (!nv || !bcb_width_ok(width) || !bcb_hub_ok(hub) || levels < 1 ||
      levels > BCB_MAX_LEVELS || !dep || !row_ptr || !cnt || !hubrows)
    return -1;
  const hipStream_t s = (hipStream_t)stream;
  if (width == 16)
    bcb_order_hist<16>(s, nv, dep, row_ptr, levels, hub, cnt, hubrows);
  else if (width == 32)
    bcb_order_hist<32>(s, nv, dep, row_ptr, levels, hub, cnt, hubrows);
  else
    bcb_order_hist<64>(s, nv, dep, row_ptr, levels, hub, cnt, hubrows);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_bcb_order_scatter(uint64_t stream, V_ID nv, uint32_t width,
                              const uint16_t* dep, const E_ID* row_ptr,
                              uint32_t levels, uint32_t hub,
                              unsigned long long* cursor, uint32_t* list,
                              uint64_t cap) {
  if (!nv || !bcb_width_ok(width) || !bcb_hub_ok(hub) || levels < 1 ||
      levels > BCB_MAX_LEVELS || !dep || !row_ptr || !cursor || !list)
    return -1;
  const hipStream_t s = (hipStream_t)stream;
  if (width == 16)
    bcb_order_scatter<16>(s, nv, dep, row_ptr, levels, hub, cursor, list, cap);
  else if (width == 32)
    bcb_order_scatter<32>(s, nv, dep, row_ptr, levels, hub, cursor, list, cap);
  else
    bcb_order_scatter<64>(s, nv, dep, row_ptr, levels, hub, cursor, list, cap);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_bcb_level(uint64_t stream, const lux_bcb_level* a, int forward) {
  if (!a || !a->nv || !bcb_width_ok(a->width) || !bcb_hub_ok(a->hub) ||
      !a->list || !a->row_ptr || !a->adj || !a->dep || !a->val || !a->delta ||
      !a->edges || a->o0 > a->o1 || a->o1 > a->o2 || a->o2 > a->o3 ||
      ((a->o3 - a->o2) & 1) || (a->o3 - a->o2) / 2 > a->scratch_items ||
      (a->o3 > a->o2 && !a->scratch) || a->d >= BCB_MAX_LEVELS ||
      (forward && (a->d < 1 || a->leaf)))
    return -1;
  const hipStream_t s = (hipStream_t)stream;
  int n;
  if (forward)
    n = a->width == 16   ? bcb_level<16, true>(s, a)
        : a->width == 32 ? bcb_level<32, true>(s, a)
                         : bcb_level<64, true>(s, a);
  else
    n = a->width == 16   ? bcb_level<16, false>(s, a)
        : a->width == 32 ? bcb_level<32, false>(s, a)
                         : bcb_level<64, false>(s, a);
  LUX_POST_LAUNCH(stream);
  return n;
}

int lux_gpu_bcb_reduce(uint64_t stream, V_ID nv, uint32_t width,
                       const float* delta, float* bc) {
  if (!nv || !bcb_width_ok(width) || !delta || !bc) return -1;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(grid_for(nv, BLOCK / (width / 4)));
  if (width == 16)
    hipLaunchKernelGGL(bcb_reduce_kernel<16>, grid, dim3(BLOCK), 0, s, nv,
                       delta, bc);
  else if (width == 32)
    hipLaunchKernelGGL(bcb_reduce_kernel<32>, grid, dim3(BLOCK), 0, s, nv,
                       delta, bc);
  else
    hipLaunchKernelGGL(bcb_reduce_kernel<64>, grid, dim3(BLOCK), 0, s, nv,
                       delta, bc);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_bcb_check(uint64_t stream, V_ID nv, uint32_t width,
                      const E_ID* in_ptr, const V_ID* in_adj,
                      const E_ID* out_ptr, const V_ID* out_adj,
                      const uint16_t* dep, const float* sigma,
                      const float* delta, double rtol,
                      unsigned long long* out) {
  if (!nv || !bcb_width_ok(width) || !in_ptr || !in_adj || !out_ptr ||
      !out_adj || !dep || !sigma || !delta || !out)
    return -1;
  hipLaunchKernelGGL(bcb_plain_kernel, dim3(grid_for((uint64_t)nv * width)),
                     dim3(BLOCK), 0, (hipStream_t)stream, nv, width, in_ptr,
                     in_adj, out_ptr, out_adj, dep, sigma, delta, rtol, out);
  LUX_POST_LAUNCH(stream);
  return 0;
}

}  // extern "C"
