// Minimum spanning forest by synchronous Boruvka rounds: simple-edge
// weights, adjacency with edge ids, per-component minimum-edge scan, hook,
// flatten, labels and a check oracle for gfx950. No reference equivalent.
//
// Input (lux_amd/msf_engine.py): the id-order DAG of tc_engine.orient, optr
// u64[nv+1] / oadj u32[m], row lo listing its neighbours hi > lo, strictly
// ascending: arc e of the DAG IS simple edge e, the edges ascending by
// (lo << 32) | hi. m < 2^32, so an edge id is a u32.
//   msf_weights_kernel   one lane per CSC arc src -> dst with src != dst:
//                        hi is searched in DAG row lo, and the arc's weight
//                        goes into w[e] by a signed atomicMin (w preset to
//                        INT32_MAX): the weight of {lo, hi} is the minimum
//                        over all its occurrences, in either direction.
//   msf_adj_fill_kernel  one lane per DAG arc e = (u, x): x into the front
//                        part of row u (its out-degree entries, in DAG
//                        order), u into row x behind x's own out-degree
//                        through a per-row cursor; each entry carries e in
//                        the parallel stream aeid, and elo[e] = u. Every
//                        index into anbr / aeid is 64-bit.
//
// State of a solve:
//   comp   u32[nv]  the component of v: a vertex c with comp[c] == c.
//   parent u32[nv]  parent[c] of a component c, written by the hook; only
//                   entries of current components are ever read, and those
//                   point at themselves until they hook, so nothing resets
//                   it between rounds.
//   best   u64[nv]  best[c] = the minimum key ((u32)w ^ 0x80000000) << 32 | e
//                   over the entries that leave component c; all-ones: none.
//                   The order (w, e) is strict, so the forest is unique.
//   dead   u8[nv]   a row that found no entry leaving its component is never
//                   walked again: components only merge.
//   meta   u64[8]   per scan: components with an edge, hooks, entries
//                   walked; per solve: total weight (i64), forest edges,
//                   errors (an index out of range: never).
//
// One round = three launches and one host read of meta:
//   msf_scan_kernel     both roles in one launch, picked from blockIdx.x.
//                       Row blocks: a wave per row of at most `hub` entries,
//                       lanes striding over it; hub blocks: one {hub row,
//                       chunk} item of the static list each, `hub` entries.
//                       The lanes keep the entries whose neighbour is in
//                       another component, the minimum key is reduced over
//                       the wave (and the workgroup), and one lane offers
//                       it to best[comp[v]]: a plain read first, the
//                       atomicMin only if the key is smaller. best only
//                       decreases, so a stale read costs an atomic, never a
//                       result; without it every row of the giant component
//                       would hit one address. A hub chunk that finds an
//                       outside entry stamps its row with the scan number;
//                       msf_hub_dead_kernel, one lane per hub row, then
//                       marks the rows no chunk stamped. No chunk waits for
//                       another.
//   msf_hook_kernel     one lane per component c with an edge: e gives
//                       (lo, hi), d is the component of the endpoint outside
//                       c. The order is strict, so the only cycles are pairs
//                       that chose the same e; of such a pair only the
//                       smaller id hooks. A hook sets parent[c] = d and
//                       inforest[e] and counts itself and w[e].
//   msf_flatten_kernel  one lane per vertex: walk parent from comp[v] to the
//                       root, read-only, store comp[v], reset best[v].
// Nothing here waits for another workgroup: no grid barrier, no cooperative
// launch, no spinning; every loop is bounded by nv or a row length.
//
// msf_check_*_kernel are the device oracle: a plain lock-free union-find and
// a per-vertex row walk that share no role, queue or key code with the
// above.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t MSF_HUB = 256;      // default longest row-role row
constexpr int MSF_MAX_GRID = 1 << 16;  // scan: blocks per role
constexpr unsigned long long MSF_INF = ~0ull;
enum { MM_CWE = 0, MM_MERGED = 1, MM_SCANNED = 2, MM_TOTAL = 3, MM_NF = 4,
       MM_ERR = 5, MM_WORDS = 8 };

using MsfArgs = lux_msf_args;

__device__ __forceinline__ unsigned long long msf_key(int w, uint32_t e) {
  return ((unsigned long long)((uint32_t)w ^ 0x80000000u) << 32) | e;
}

__device__ __forceinline__ unsigned long long msf_wave_min(
    unsigned long long v) {
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    unsigned long long o = __shfl_down(v, off, WAVE);
    v = o < v ? o : v;
  }
  return v;  // valid in lane 0
}

// The last row r with ptr[r] <= i, branch-free: ptr[r] <= i and the answer
// is in [r, r + len) throughout. Needs nv >= 1 and ptr[0] <= i.
__device__ __forceinline__ V_ID msf_row_of(const E_ID* ptr, V_ID nv, E_ID i) {
  V_ID r = 0;
  for (V_ID len = nv; len > 1;) {
    V_ID half = len >> 1;
    r += ptr[r + half] <= i ? half : 0;
    len -= half;
  }
  return r;
}

// The minimum key over the entries sub, sub + step, ... of
// anbr / aeid[b : b + n) whose neighbour lies outside component cv.
__device__ __forceinline__ unsigned long long msf_span(
    const MsfArgs& a, E_ID b, uint32_t n, uint32_t sub, uint32_t step,
    V_ID cv) {
  unsigned long long key = MSF_INF;
  for (uint32_t j = sub; j < n; j += step) {
    V_ID u = a.anbr[b + j];
    if (u >= a.nv || a.comp[u] == cv) continue;
    uint32_t e = a.aeid[b + j];
    if (e >= a.m) continue;
    unsigned long long k = msf_key(a.w[e], e);
    key = k < key ? k : key;
  }
  return key;
}

__device__ __forceinline__ void msf_offer(const MsfArgs& a, V_ID cv,
                                          unsigned long long key) {
  if (key < __hip_atomic_load(&a.best[cv], __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(&a.best[cv], key);
}

// ---------------- preparation ----------------

__global__ void __launch_bounds__(BLOCK) msf_weights_kernel(
    V_ID nv, E_ID ne, const E_ID* row_ptr, const V_ID* col, const int* weight,
    const E_ID* optr, const V_ID* oadj, int* w, unsigned long long* err) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < ne;
       i += stride) {
    V_ID dst = msf_row_of(row_ptr, nv, i);
    V_ID src = col[i];
    if (src == dst) continue;
    if (src >= nv) {
      atomicAdd(err, 1ull);
      continue;
    }
    V_ID lo = src < dst ? src : dst, hi = src ^ dst ^ lo;
    // the first entry >= hi of the ascending row lo
    E_ID b = optr[lo], e = optr[lo + 1];
    while (b < e) {
      E_ID mid = b + ((e - b) >> 1);
      if (oadj[mid] < hi) b = mid + 1;
      else e = mid;
    }
    if (b < optr[lo + 1] && oadj[b] == hi) atomicMin(&w[b], weight[i]);
    else atomicAdd(err, 1ull);
  }
}

__global__ void __launch_bounds__(BLOCK) msf_adj_fill_kernel(
    V_ID nv, E_ID m, const E_ID* optr, const V_ID* oadj, const E_ID* aptr,
    uint32_t* cursor, V_ID* anbr, uint32_t* aeid, V_ID* elo) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    V_ID u = msf_row_of(optr, nv, e);
    elo[e] = u;
    V_ID x = oadj[e];
    if (x >= nv) continue;
    E_ID iu = aptr[u] + (e - optr[u]);
    if (iu < aptr[u + 1]) {
      anbr[iu] = x;
      aeid[iu] = (uint32_t)e;
    }
    E_ID ix = aptr[x] + (optr[x + 1] - optr[x]) + atomicAdd(&cursor[x], 1u);
    if (ix < aptr[x + 1]) {
      anbr[ix] = u;
      aeid[ix] = (uint32_t)e;
    }
  }
}

__global__ void __launch_bounds__(BLOCK) msf_init_kernel(MsfArgs a) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < a.nv;
       v += stride) {
    a.comp[v] = (V_ID)v;
    a.parent[v] = (V_ID)v;
    a.best[v] = MSF_INF;
    a.dead[v] = 0;
  }
}

// ---------------- one round ----------------

__global__ void __launch_bounds__(BLOCK) msf_scan_kernel(MsfArgs a,
                                                         uint32_t row_blocks,
                                                         uint32_t stamp) {
  constexpr int NW = BLOCK / WAVE;
  __shared__ unsigned long long red[NW];
  __shared__ unsigned long long cnt[NW];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  unsigned long long walked = 0;  // counted in lane 0 of every wave
  if (blockIdx.x < row_blocks) {
    uint64_t step = (uint64_t)row_blocks * NW;
    for (uint64_t v = (uint64_t)blockIdx.x * NW + wid; v < a.nv; v += step) {
      if (a.use_dead && a.dead[v]) continue;
      E_ID b = a.aptr[v];
      uint64_t d = a.aptr[v + 1] - b;
      if (d > a.hub) continue;  // its chunks are in the item list
      V_ID cv = a.comp[v];
      unsigned long long key =
          msf_wave_min(msf_span(a, b, (uint32_t)d, lane, WAVE, cv));
      if (lane == 0) {
        walked += d;
        if (key != MSF_INF) msf_offer(a, cv, key);
        else if (a.use_dead) a.dead[v] = 1;
      }
    }
  } else {
    uint32_t nb = gridDim.x - row_blocks;
    for (uint64_t i = blockIdx.x - row_blocks; i < a.nitems; i += nb) {
      // everything up to the walk is the same in all lanes of the workgroup
      uint32_t hr = a.item_row[i];
      if (hr >= a.nhub) continue;
      V_ID v = a.hubrow[hr];
      if (v >= a.nv) continue;
      if (a.use_dead && a.dead[v]) continue;  // written after the scan only
      E_ID b = a.aptr[v];
      uint64_t d = a.aptr[v + 1] - b;
      uint64_t first = (uint64_t)a.item_chunk[i] * a.hub;
      if (first >= d) continue;
      uint32_t n = d - first < a.hub ? (uint32_t)(d - first) : a.hub;
      V_ID cv = a.comp[v];
      unsigned long long key =
          msf_wave_min(msf_span(a, b + first, n, threadIdx.x, BLOCK, cv));
      if (lane == 0) red[wid] = key;
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int k = 1; k < NW; k++) key = red[k] < key ? red[k] : key;
        walked += n;
        if (key != MSF_INF) {
          msf_offer(a, cv, key);
          __hip_atomic_store(&a.hubext[hr], stamp, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      __syncthreads();  // red is written again in the next trip
    }
  }
  if (lane == 0) cnt[wid] = walked;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < NW; k++) walked += cnt[k];
    if (walked) atomicAdd(&a.meta[MM_SCANNED], walked);
  }
}

// A hub row none of whose chunks found an outside entry in scan `stamp`.
__global__ void __launch_bounds__(BLOCK) msf_hub_dead_kernel(MsfArgs a,
                                                             uint32_t stamp) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t hr = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       hr < a.nhub; hr += stride) {
    V_ID v = a.hubrow[hr];
    if (v < a.nv && !a.dead[v] && a.hubext[hr] != stamp) a.dead[v] = 1;
  }
}

__global__ void __launch_bounds__(BLOCK) msf_hook_kernel(MsfArgs a) {
  __shared__ unsigned long long lds[4][BLOCK / WAVE];
  unsigned long long cwe = 0, merged = 0, tw = 0, err = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; c < a.nv;
       c += stride) {
    if (a.comp[c] != (V_ID)c) continue;
    unsigned long long key = a.best[c];
    if (key == MSF_INF) continue;
    cwe++;
    uint32_t e = (uint32_t)key;
    if (e >= a.m) {
      err++;
      continue;
    }
    V_ID lo = a.elo[e], hi = a.ehi[e];
    if (lo >= a.nv || hi >= a.nv) {
      err++;
      continue;
    }
    V_ID cl = a.comp[lo], ch = a.comp[hi];
    V_ID d = cl == (V_ID)c ? ch : cl;
    if ((cl != (V_ID)c && ch != (V_ID)c) || d == (V_ID)c || d >= a.nv) {
      err++;
      continue;
    }
    // both components chose e: only the smaller id hooks
    if (a.best[d] == key && (V_ID)c > d) continue;
    a.parent[c] = d;
    a.inforest[e] = 1;
    merged++;
    tw += (unsigned long long)(long long)a.w[e];  // i64, two's complement
  }
  cwe = block_reduce_sum(cwe, lds[0]);
  merged = block_reduce_sum(merged, lds[1]);
  tw = block_reduce_sum(tw, lds[2]);
  err = block_reduce_sum(err, lds[3]);
  if (threadIdx.x == 0) {
    if (cwe) atomicAdd(&a.meta[MM_CWE], cwe);
    if (merged) {
      atomicAdd(&a.meta[MM_MERGED], merged);
      atomicAdd(&a.meta[MM_NF], merged);
      atomicAdd(&a.meta[MM_TOTAL], tw);
    }
    if (err) atomicAdd(&a.meta[MM_ERR], err);
  }
}

__global__ void __launch_bounds__(BLOCK) msf_flatten_kernel(MsfArgs a) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < a.nv;
       v += stride) {
    V_ID r = a.comp[v];
    // hooks are acyclic; the bound only keeps a broken parent from looping
    for (V_ID hops = 0; hops < a.nv && r < a.nv; hops++) {
      V_ID p = a.parent[r];
      if (p == r || p >= a.nv) break;
      r = p;
    }
    a.comp[v] = r;
    a.best[v] = MSF_INF;
  }
}

// ---------------- labels ----------------

__global__ void __launch_bounds__(BLOCK) msf_maxid_kernel(V_ID nv,
                                                          const V_ID* comp,
                                                          V_ID* maxid) {
  // Vertices are taken in DESCENDING order, a wave at a time, so lane 0
  // holds the wave's largest id: a lane in lane 0's component has nothing
  // to add, and any other lane reads maxid first and skips the atomic when
  // its id is not larger (maxid only grows, so a stale read costs an
  // atomic, never a result). In ascending order with a bare atomicMax the
  // giant component's vertices all hit one address: 100 ms at RMAT-24.
  const int lane = threadIdx.x & (WAVE - 1);
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x - lane;
       i0 < nv; i0 += stride) {
    uint64_t i = i0 + lane;
    bool on = i < nv;
    V_ID v = on ? (V_ID)(nv - 1 - i) : 0;
    V_ID c = on ? comp[v] : nv;
    V_ID lead = __shfl(c, 0, WAVE);
    if (!on || c >= nv) continue;
    if (lane != 0 && c == lead) continue;
    if (__hip_atomic_load(&maxid[c], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT) < v)
      atomicMax(&maxid[c], v);
  }
}

__global__ void __launch_bounds__(BLOCK) msf_label_kernel(V_ID nv,
                                                          const V_ID* comp,
                                                          const V_ID* maxid,
                                                          V_ID* labels) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    V_ID c = comp[v];
    labels[v] = c < nv ? maxid[c] : (V_ID)v;
  }
}

// ---------------- check oracle ----------------

__device__ __forceinline__ V_ID msfc_load(const V_ID* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(BLOCK) msf_check_iota_kernel(V_ID nv,
                                                               V_ID* pf,
                                                               V_ID* pa) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    pf[v] = (V_ID)v;
    pa[v] = (V_ID)v;
  }
}

// Hooks only put a smaller root under a larger one, so a chain strictly
// increases and ends at the largest id it has reached.
__device__ __forceinline__ V_ID msfc_root(const V_ID* parent, V_ID v) {
  for (;;) {
    V_ID p = msfc_load(&parent[v]);
    if (p <= v) return v;
    v = p;
  }
}

// The root with path halving, for the union pass: only a non-root entry is
// rewritten, to one of its ancestors, so any interleaving keeps every chain
// increasing and inside its tree.
__device__ __forceinline__ V_ID msfc_find(V_ID* parent, V_ID v) {
  V_ID p = msfc_load(&parent[v]);
  V_ID gp = msfc_load(&parent[p]);
  while (p != gp) {
    __hip_atomic_store(&parent[v], gp, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    v = p;
    p = gp;
    gp = msfc_load(&parent[p]);
  }
  return p;
}

// One lane per edge: union its endpoints (only the marked edges if mask is
// given).
__global__ void __launch_bounds__(BLOCK) msf_check_union_kernel(
    E_ID m, V_ID nv, const V_ID* elo, const V_ID* ehi, const uint8_t* mask,
    V_ID* parent) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    if (mask && !mask[e]) continue;
    V_ID x = elo[e], y = ehi[e];
    if (x >= nv || y >= nv) continue;
    V_ID rx = msfc_find(parent, x), ry = msfc_find(parent, y);
    while (rx != ry) {
      V_ID lo = rx < ry ? rx : ry, hi = rx ^ ry ^ lo;
      V_ID old = atomicCAS(&parent[lo], lo, hi);
      if (old == lo) break;
      rx = msfc_find(parent, old);
      ry = msfc_find(parent, hi);
    }
  }
}

// out[0] += vertices whose root in either forest is not labels[v];
// out[2] += vertices with labels[v] == v (the components).
__global__ void __launch_bounds__(BLOCK) msf_check_labels_kernel(
    V_ID nv, const V_ID* pf, const V_ID* pa, const V_ID* labels,
    unsigned long long* out) {
  __shared__ unsigned long long lds[2][BLOCK / WAVE];
  unsigned long long bad = 0, roots = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    V_ID l = labels[v];
    bad += msfc_root(pf, (V_ID)v) != l;
    bad += msfc_root(pa, (V_ID)v) != l;
    roots += l == (V_ID)v;
  }
  bad = block_reduce_sum(bad, lds[0]);
  roots = block_reduce_sum(roots, lds[1]);
  if (threadIdx.x == 0) {
    if (bad) atomicAdd(&out[0], bad);
    if (roots) atomicAdd(&out[2], roots);
  }
}

// out[1] += marked edges, out[3] += their weights (i64).
__global__ void __launch_bounds__(BLOCK) msf_check_edges_kernel(
    E_ID m, const int* w, const uint8_t* mask, unsigned long long* out) {
  __shared__ unsigned long long lds[2][BLOCK / WAVE];
  unsigned long long n = 0, tw = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    if (!mask[e]) continue;
    n++;
    tw += (unsigned long long)(long long)w[e];
  }
  n = block_reduce_sum(n, lds[0]);
  tw = block_reduce_sum(tw, lds[1]);
  if (threadIdx.x == 0) {
    if (n) atomicAdd(&out[1], n);
    if (tw) atomicAdd(&out[3], tw);
  }
}

// out[0] += non-isolated vertices whose minimum (w, e) entry is not marked.
__global__ void __launch_bounds__(BLOCK) msf_check_min_kernel(
    V_ID nv, E_ID m, const E_ID* aptr, const uint32_t* aeid, const int* w,
    const uint8_t* mask, unsigned long long* out) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long bad = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    E_ID b = aptr[v], end = aptr[v + 1];
    if (b == end) continue;
    bool have = false;
    int bw = 0;
    uint32_t be = 0;
    for (E_ID j = b; j < end; j++) {
      uint32_t e = aeid[j];
      if (e >= m) continue;
      int we = w[e];
      if (!have || we < bw || (we == bw && e < be)) {
        have = true;
        bw = we;
        be = e;
      }
    }
    bad += !have || !mask[be];
  }
  bad = block_reduce_sum(bad, lds);
  if (threadIdx.x == 0 && bad) atomicAdd(&out[0], bad);
}

__global__ void msf_set_mark_kernel(uint8_t* mask, E_ID e, uint8_t value) {
  if (blockIdx.x == 0 && threadIdx.x == 0) mask[e] = value;
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_msf_hub_default() { return MSF_HUB; }
uint32_t lux_gpu_msf_meta_words() { return MM_WORDS; }

// w: i32[m] preset to INT32_MAX; err: one u64, added to (an arc whose
// simple edge is not in the DAG: never).
void lux_gpu_msf_weights(uint64_t stream, V_ID nv, E_ID ne,
                         const E_ID* row_ptr, const V_ID* col,
                         const int* weight, const E_ID* optr, const V_ID* oadj,
                         int* w, unsigned long long* err) {
  if (!nv || !ne) return;
  hipLaunchKernelGGL(msf_weights_kernel, dim3(grid_for(ne)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, ne, row_ptr, col, weight, optr,
                     oadj, w, err);
  LUX_POST_LAUNCH(stream);
}

// cursor: u32[nv], zeroed; anbr / aeid: u32[2m]; elo: u32[m].
void lux_gpu_msf_adj_fill(uint64_t stream, V_ID nv, E_ID m, const E_ID* optr,
                          const V_ID* oadj, const E_ID* aptr, uint32_t* cursor,
                          V_ID* anbr, uint32_t* aeid, V_ID* elo) {
  if (!nv || !m) return;
  hipLaunchKernelGGL(msf_adj_fill_kernel, dim3(grid_for(m)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, m, optr, oadj, aptr, cursor,
                     anbr, aeid, elo);
  LUX_POST_LAUNCH(stream);
}

// The state of a fresh solve: comp = parent = id, best = none, nothing dead,
// no forest edge, no stamp, meta zeroed.
void lux_gpu_msf_init(uint64_t stream, const lux_msf_args* a) {
  hipStream_t s = (hipStream_t)stream;
  LUX_CHECK_HIP(hipMemsetAsync(a->meta, 0, sizeof(uint64_t) * MM_WORDS, s));
  if (a->m) LUX_CHECK_HIP(hipMemsetAsync(a->inforest, 0, a->m, s));
  if (a->nhub)
    LUX_CHECK_HIP(hipMemsetAsync(a->hubext, 0, sizeof(uint32_t) * a->nhub, s));
  if (a->nv)
    hipLaunchKernelGGL(msf_init_kernel, dim3(grid_for(a->nv)), dim3(BLOCK), 0,
                       s, *a);
  LUX_POST_LAUNCH(stream);
}

// Scan number `stamp` (1, 2, ...): zeroes the per-scan words of meta, fills
// best and marks the rows that found nothing. Returns the kernels launched,
// -1 (and launches nothing) on arguments out of range.
int lux_gpu_msf_scan(uint64_t stream, const lux_msf_args* a, uint32_t stamp) {
  if (!a->hub || !stamp || a->m >> 32) return -1;
  if (!a->nv) return 0;
  hipStream_t s = (hipStream_t)stream;
  LUX_CHECK_HIP(hipMemsetAsync(a->meta, 0, sizeof(uint64_t) * 3, s));
  uint32_t rb = ceil_div_u32(a->nv, BLOCK / WAVE);
  if (rb > (uint32_t)MSF_MAX_GRID) rb = MSF_MAX_GRID;
  uint32_t hb = a->nitems > (uint32_t)MSF_MAX_GRID ? MSF_MAX_GRID : a->nitems;
  hipLaunchKernelGGL(msf_scan_kernel, dim3(rb + hb), dim3(BLOCK), 0, s, *a, rb,
                     stamp);
  int launched = 1;
  if (a->use_dead && a->nhub) {
    hipLaunchKernelGGL(msf_hub_dead_kernel, dim3(grid_for(a->nhub)),
                       dim3(BLOCK), 0, s, *a, stamp);
    launched++;
  }
  LUX_POST_LAUNCH(stream);
  return launched;
}

void lux_gpu_msf_hook(uint64_t stream, const lux_msf_args* a) {
  if (!a->nv) return;
  hipLaunchKernelGGL(msf_hook_kernel, dim3(grid_for(a->nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, *a);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_msf_flatten(uint64_t stream, const lux_msf_args* a) {
  if (!a->nv) return;
  hipLaunchKernelGGL(msf_flatten_kernel, dim3(grid_for(a->nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, *a);
  LUX_POST_LAUNCH(stream);
}

// labels[v] = the largest vertex id of comp[v]'s class; maxid: u32[nv]
// scratch. Two kernels.
void lux_gpu_msf_labels(uint64_t stream, V_ID nv, const V_ID* comp,
                        V_ID* maxid, V_ID* labels) {
  if (!nv) return;
  hipStream_t s = (hipStream_t)stream;
  LUX_CHECK_HIP(hipMemsetAsync(maxid, 0, sizeof(V_ID) * nv, s));
  hipLaunchKernelGGL(msf_maxid_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0, s,
                     nv, comp, maxid);
  hipLaunchKernelGGL(msf_label_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0, s,
                     nv, comp, maxid, labels);
  LUX_POST_LAUNCH(stream);
}

// The check oracle. mask: u8[m], the forest to judge; pf / pa: u32[nv]
// scratch; out: u64[4], zeroed here: [0] violations, [1] marked edges, [2]
// vertices with labels[v] == v, [3] the marked edges' weight (i64 bits).
void lux_gpu_msf_check(uint64_t stream, V_ID nv, E_ID m, const E_ID* aptr,
                       const uint32_t* aeid, const V_ID* elo, const V_ID* ehi,
                       const int* w, const uint8_t* mask, const V_ID* labels,
                       V_ID* pf, V_ID* pa, unsigned long long* out) {
  hipStream_t s = (hipStream_t)stream;
  LUX_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(uint64_t) * 4, s));
  if (!nv) return;
  hipLaunchKernelGGL(msf_check_iota_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0,
                     s, nv, pf, pa);
  if (m) {
    hipLaunchKernelGGL(msf_check_union_kernel, dim3(grid_for(m)), dim3(BLOCK),
                       0, s, m, nv, elo, ehi, mask, pf);
    hipLaunchKernelGGL(msf_check_union_kernel, dim3(grid_for(m)), dim3(BLOCK),
                       0, s, m, nv, elo, ehi, (const uint8_t*)nullptr, pa);
    hipLaunchKernelGGL(msf_check_edges_kernel, dim3(grid_for(m)), dim3(BLOCK),
                       0, s, m, w, mask, out);
    hipLaunchKernelGGL(msf_check_min_kernel, dim3(grid_for(nv)), dim3(BLOCK),
                       0, s, nv, m, aptr, aeid, w, mask, out);
  }
  hipLaunchKernelGGL(msf_check_labels_kernel, dim3(grid_for(nv)), dim3(BLOCK),
                     0, s, nv, pf, pa, labels, out);
  LUX_POST_LAUNCH(stream);
}

// mask[e] = value: the test hook that corrupts a copy of the forest mask.
int lux_gpu_msf_set_mark(uint64_t stream, uint8_t* mask, E_ID m, E_ID e,
                         int value) {
  if (e >= m) return -1;
  hipLaunchKernelGGL(msf_set_mark_kernel, dim3(1), dim3(WAVE), 0,
                     (hipStream_t)stream, mask, e, (uint8_t)(value != 0));
  LUX_POST_LAUNCH(stream);
  return 0;
}

}  // extern "C"
