// k-core decomposition by synchronous peeling: adjacency build, level scan,
// round peel, single-workgroup round fusion and a check oracle for gfx950.
// No reference equivalent.
//
// Input (lux_amd/kcore_engine.py): the id-order DAG of tc_engine.orient,
// optr u64[nv+1] / oadj u32[m], row u listing its neighbours > u.
// kcore_adj_fill_kernel turns it into the full symmetric adjacency aptr
// u64[nv+1] / aadj u32[2m]: one lane per arc (u, w), w into the front part
// of row u (its out-degree entries, in DAG order), u into row w behind w's
// own out-degree through a per-row cursor. Row order does not matter to
// the peel. Every index into aadj is 64-bit.
//
// State of a decomposition:
//   deg   i32[nv]  the current degree; signed, because concurrent
//                  decrements take a removed vertex transiently below k. A
//                  removed vertex rests at its coreness, so at the end deg
//                  is the answer.
//   order u32[nv]  append-only: every vertex exactly once, when it is found
//                  removable. A round is a range [head, tail) of it.
//   hubq  u32 pairs {v, chunk}, append-only: a row longer than `hub` is
//                  appended to order like any other and ALSO gives
//                  ceil(d / hub) chunk items here. The host sizes hubq
//                  from the degree array, so neither list can overflow;
//                  the appends are bounds-checked all the same.
//   meta  u32[8]   M_TAIL / M_HUBTAIL: the append cursors; M_MIN: the scan's
//                  minimum; M_FUSED / M_HEAD: what the tail kernel did.
//
// Level k (the host jumps k to the minimum alive degree, so every alive
// vertex has deg >= k when the level starts):
//   kcore_scan_kernel  one lane per vertex: deg == k is appended (a ballot
//                      and one atomic per wave), min{deg : deg > k} folded
//                      through wave and block into meta[M_MIN] (one atomic
//                      per block);
//   kcore_peel_kernel  one launch per round, the role from blockIdx.x: row
//                      blocks take order[head : tail), a wave per entry
//                      whose row is at most `hub` long, lanes striding
//                      over the row; hub blocks take one hubq item each.
//                      Both run kcore_visit on every neighbour: the
//                      decrement that takes deg from k + 1 to k appends the
//                      neighbour for the next round; a decrement that finds
//                      deg <= k hit a removed vertex and is put back;
//   kcore_tail_kernel  ONE workgroup (KCORE_TAIL_BLOCK threads) peels
//                      successive small rounds of the level (at most `fuse`
//                      entries, no hub item) with a workgroup barrier
//                      between them, so that a cascade (a path, a chain of
//                      shells) costs one launch and one host read, not one
//                      per round. It stops at an empty round (the level is
//                      done), or hands a round that is too large or has a
//                      hub row back to the host unprocessed. Every trip
//                      consumes at least one entry of order, which holds at
//                      most nv.
// Nothing here waits for another workgroup: no grid barrier, no spinning.
//
// kcore_check_kernel is the device oracle, a plain one-lane-per-vertex
// walk sharing nothing with the above.
#include "gpu_common.h"

namespace lux {

constexpr uint32_t KCORE_HUB = 1024;        // default longest row-role row
constexpr uint32_t KCORE_FUSE = 16;         // default tail-kernel round size
constexpr int KCORE_TAIL_BLOCK = 1024;      // tail kernel: 16 waves
constexpr int KCORE_SCAN_UNROLL = 4;        // scan: vertices per lane and trip
constexpr uint32_t KCORE_FUSE_MAX = 65536;  // what the tail kernel accepts
constexpr int KCORE_MAX_GRID = 1 << 16;     // peel: blocks per role
constexpr uint32_t KCORE_NONE = 0xFFFFFFFFu;
enum { M_TAIL = 0, M_HUBTAIL = 1, M_MIN = 2, M_FUSED = 3, M_HEAD = 4,
       M_WORDS = 8 };

struct KcArgs {
  const E_ID* aptr;  // u64[nv+1]
  const V_ID* aadj;  // u32[2m]
  int* deg;          // i32[nv]
  V_ID* order;       // u32[nv]
  uint32_t* hubq;    // u32[2 * hubcap]
  uint32_t* meta;    // u32[M_WORDS]
  V_ID nv;
  uint32_t hubcap;   // items
  uint32_t hub;      // rows longer than this go through hubq
  int k;
};

// Append the u of every lane with enq set to order (and its chunk items to
// hubq if its row is a hub row): one atomic on the cursor per wave. All
// lanes of the wave must call this together.
__device__ __forceinline__ void kcore_enqueue(const KcArgs& a, bool enq,
                                              V_ID u) {
  unsigned long long mask = __ballot(enq);
  if (!mask) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader)
    base = atomicAdd(&a.meta[M_TAIL], (uint32_t)__popcll(mask));
  base = __shfl(base, leader, WAVE);
  if (!enq) return;
  uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
  if (at < a.nv) a.order[at] = u;
  uint32_t d = (uint32_t)(a.aptr[u + 1] - a.aptr[u]);
  if (d > a.hub) {
    uint32_t nc = ceil_div_u32(d, a.hub);
    uint32_t h = atomicAdd(&a.meta[M_HUBTAIL], nc);
    for (uint32_t c = 0; c < nc && h + c < a.hubcap; c++) {
      a.hubq[2 * (uint64_t)(h + c)] = u;
      a.hubq[2 * (uint64_t)(h + c) + 1] = c;
    }
  }
}

// One neighbour u of a vertex removed at level k. Returns whether this
// decrement is the one that makes u removable. deg[u] <= k means u is
// removed already (it rests at its coreness, or below it while another
// lane's under-run is being put back): the pre-read skips it, and a
// decrement that still finds it (old <= k) is put back. An alive u has no
// pending put-back, so its count is exact and exactly one decrement sees
// k + 1.
__device__ __forceinline__ bool kcore_visit(const KcArgs& a, V_ID u) {
  if (__hip_atomic_load(&a.deg[u], __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT) <= a.k)
    return false;
  int old = atomicSub(&a.deg[u], 1);
  if (old == a.k + 1) return true;
  if (old <= a.k) atomicAdd(&a.deg[u], 1);
  return false;
}

// The entries sub, sub + step, ... of aadj[b : b + n), one per lane and
// trip; n is the same in every lane of a wave.
__device__ __forceinline__ void kcore_span(const KcArgs& a, E_ID b,
                                           uint32_t n, uint32_t sub,
                                           uint32_t step) {
  for (uint32_t j = sub; __any(j < n); j += step) {
    bool enq = false;
    V_ID u = 0;
    if (j < n) {
      u = a.aadj[b + j];
      enq = kcore_visit(a, u);
    }
    kcore_enqueue(a, enq, u);
  }
}

// ---------------- adjacency build ----------------

__global__ void __launch_bounds__(BLOCK) kcore_adj_fill_kernel(
    V_ID nv, E_ID m, const E_ID* optr, const V_ID* oadj, const E_ID* aptr,
    uint32_t* cursor, V_ID* aadj) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    // u = the last row with optr[u] <= e, branch-free: optr[u] <= e and
    // the answer is in [u, u + len) throughout
    V_ID u = 0;
    for (V_ID len = nv; len > 1;) {
      V_ID half = len >> 1;
      u += optr[u + half] <= e ? half : 0;
      len -= half;
    }
    V_ID w = oadj[e];
    if (w >= nv) continue;
    E_ID iu = aptr[u] + (e - optr[u]);
    if (iu < aptr[u + 1]) aadj[iu] = w;
    E_ID iw = aptr[w] + (optr[w + 1] - optr[w]) + atomicAdd(&cursor[w], 1u);
    if (iw < aptr[w + 1]) aadj[iw] = u;
  }
}

// ---------------- level scan ----------------

__global__ void __launch_bounds__(BLOCK) kcore_scan_kernel(KcArgs a) {
  __shared__ uint32_t red[BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  uint32_t mn = KCORE_NONE;
  // a wave takes KCORE_SCAN_UNROLL * 64 consecutive vertices per trip, the
  // loads issued together; -1 (below every k) stands for "past the end"
  constexpr int U = KCORE_SCAN_UNROLL;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x * U;
  for (uint64_t v0 = (blockIdx.x * (uint64_t)blockDim.x + wid * WAVE) * U;
       v0 < a.nv; v0 += stride) {
    int d[U];
#pragma unroll
    for (int j = 0; j < U; j++) {
      uint64_t v = v0 + j * WAVE + lane;
      d[j] = v < a.nv ? a.deg[v] : -1;
    }
#pragma unroll
    for (int j = 0; j < U; j++) {
      if (d[j] > a.k && (uint32_t)d[j] < mn) mn = (uint32_t)d[j];
      kcore_enqueue(a, d[j] == a.k, (V_ID)(v0 + j * WAVE + lane));
    }
  }
  mn = wave_reduce_min(mn);
  if (lane == 0) red[wid] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / WAVE; w++) mn = red[w] < mn ? red[w] : mn;
    if (mn != KCORE_NONE) atomicMin(&a.meta[M_MIN], mn);
  }
}

// ---------------- one round ----------------

__global__ void __launch_bounds__(BLOCK) kcore_peel_kernel(
    KcArgs a, uint32_t head, uint32_t tail, uint32_t hubhead,
    uint32_t hubtail, uint32_t row_blocks) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = BLOCK / WAVE;
  if (blockIdx.x < row_blocks) {
    uint64_t step = (uint64_t)row_blocks * NW;
    for (uint64_t i = head + (uint64_t)blockIdx.x * NW + wid; i < tail;
         i += step) {
      V_ID v = a.order[i];
      E_ID b = a.aptr[v];
      uint32_t d = (uint32_t)(a.aptr[v + 1] - b);
      if (d > a.hub) continue;  // its chunks are in hubq
      kcore_span(a, b, d, lane, WAVE);
    }
  } else {
    uint32_t nb = gridDim.x - row_blocks;
    for (uint64_t i = hubhead + (blockIdx.x - row_blocks); i < hubtail;
         i += nb) {
      V_ID v = a.hubq[2 * i];
      uint64_t first = (uint64_t)a.hubq[2 * i + 1] * a.hub;
      E_ID b = a.aptr[v];
      uint64_t d = a.aptr[v + 1] - b;
      uint32_t n = 0;
      if (first < d) n = d - first < a.hub ? (uint32_t)(d - first) : a.hub;
      kcore_span(a, b + first, n, threadIdx.x, BLOCK);
    }
  }
}

// ---------------- small-round fusion ----------------

// One workgroup. The host launches it on a round [head, tail) of at most
// fuse entries with no hub item pending (hubtail = the hubq cursor then).
__global__ void __launch_bounds__(KCORE_TAIL_BLOCK) kcore_tail_kernel(
    KcArgs a, uint32_t head, uint32_t tail, uint32_t hubtail,
    uint32_t fuse) {
  __shared__ uint32_t lds_tail, lds_hubtail;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = KCORE_TAIL_BLOCK / WAVE;
  uint32_t rounds = 0;
  for (;;) {
    for (uint32_t i = head + wid; i < tail; i += NW) {
      V_ID v = __hip_atomic_load(&a.order[i], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      E_ID b = a.aptr[v];
      uint32_t d = (uint32_t)(a.aptr[v + 1] - b);
      if (d > a.hub) d = 0;  // never: a hub row ends the loop below
      kcore_span(a, b, d, lane, WAVE);
    }
    rounds++;
    head = tail;
    __syncthreads();  // every wave's appends are counted in the cursors
    if (threadIdx.x == 0) {
      lds_tail = __hip_atomic_load(&a.meta[M_TAIL], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      lds_hubtail = __hip_atomic_load(&a.meta[M_HUBTAIL], __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    tail = lds_tail;
    // empty: the level is done; too large, a hub row, or a cursor past the
    // list: the host's
    if (tail <= head || tail - head > fuse || lds_hubtail != hubtail ||
        tail > a.nv)
      break;
  }
  if (threadIdx.x == 0) {
    a.meta[M_FUSED] = rounds;
    a.meta[M_HEAD] = head;
  }
}

// ---------------- check oracle ----------------

// Necessary conditions of a coreness array, per vertex v with c = core[v]:
// at least c neighbours of coreness >= c (v is in the c-core), fewer than
// c + 1 of coreness >= c + 1 (else v would be in the (c+1)-core), and
// 0 <= c <= degree. Not sufficient: the all-zero array passes on any graph.
__global__ void __launch_bounds__(BLOCK) kcore_check_kernel(
    V_ID nv, const E_ID* aptr, const V_ID* aadj, const int* core,
    unsigned long long* bad) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long mine = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    long long c = core[v];
    E_ID b = aptr[v], e = aptr[v + 1];
    long long ge = 0, gt = 0;
    for (E_ID j = b; j < e; j++) {
      long long cu = core[aadj[j]];
      ge += cu >= c;
      gt += cu >= c + 1;
    }
    mine += c < 0 || ge < c || gt >= c + 1 || c > (long long)(e - b);
  }
  mine = block_reduce_sum(mine, lds);
  if (threadIdx.x == 0 && mine) atomicAdd(bad, mine);
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_kcore_hub_default() { return KCORE_HUB; }
uint32_t lux_gpu_kcore_fuse_default() { return KCORE_FUSE; }
uint32_t lux_gpu_kcore_fuse_max() { return KCORE_FUSE_MAX; }
uint32_t lux_gpu_kcore_meta_words() { return M_WORDS; }

// optr / oadj: the id-order DAG (m arcs); aptr: u64[nv+1], the scanned
// full degrees; cursor: u32[nv], zeroed; aadj: u32[2m], filled.
void lux_gpu_kcore_adj_fill(uint64_t stream, V_ID nv, E_ID m,
                            const E_ID* optr, const V_ID* oadj,
                            const E_ID* aptr, uint32_t* cursor, V_ID* aadj) {
  if (!nv || !m) return;
  hipLaunchKernelGGL(kcore_adj_fill_kernel, dim3(grid_for(m)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, m, optr, oadj, aptr, cursor,
                     aadj);
  LUX_POST_LAUNCH(stream);
}

// Append every v with deg[v] == k; meta[M_MIN] = min{deg[v] : deg[v] > k},
// 0xFFFFFFFF if there is none.
void lux_gpu_kcore_scan(uint64_t stream, V_ID nv, const E_ID* aptr, int* deg,
                        V_ID* order, uint32_t* hubq, uint32_t hubcap,
                        uint32_t* meta, uint32_t hub, int k) {
  if (!nv) return;
  hipStream_t s = (hipStream_t)stream;
  LUX_CHECK_HIP(hipMemsetAsync(meta + M_MIN, 0xFF, sizeof(uint32_t), s));
  KcArgs a{aptr, nullptr, deg, order, hubq, meta, nv, hubcap, hub, k};
  int grid = grid_for(((uint64_t)nv + KCORE_SCAN_UNROLL - 1) /
                      KCORE_SCAN_UNROLL);
  hipLaunchKernelGGL(kcore_scan_kernel, dim3(grid), dim3(BLOCK), 0, s, a);
  LUX_POST_LAUNCH(stream);
}

// One round: order[head : tail) and hubq[hubhead : hubtail) (items), the
// cursors in meta standing at tail and hubtail. Returns -1 (and launches
// nothing) on cursors out of order or beyond the lists.
int lux_gpu_kcore_peel(uint64_t stream, V_ID nv, const E_ID* aptr,
                       const V_ID* aadj, int* deg, V_ID* order,
                       uint32_t* hubq, uint32_t hubcap, uint32_t* meta,
                       uint32_t hub, int k, uint32_t head, uint32_t tail,
                       uint32_t hubhead, uint32_t hubtail) {
  if (!hub) return -1;
  if (tail > nv || head > tail || hubtail > hubcap || hubhead > hubtail)
    return -1;
  const uint32_t n = tail - head, nh = hubtail - hubhead;
  if (!n && !nh) return 0;
  uint32_t rb = ceil_div_u32(n, BLOCK / WAVE);
  if (rb > (uint32_t)KCORE_MAX_GRID) rb = KCORE_MAX_GRID;
  uint32_t hb = nh > (uint32_t)KCORE_MAX_GRID ? KCORE_MAX_GRID : nh;
  KcArgs a{aptr, aadj, deg, order, hubq, meta, nv, hubcap, hub, k};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kcore_peel_kernel, dim3(rb + hb), dim3(BLOCK), 0, s, a,
                     head, tail, hubhead, hubtail, rb);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// Rounds of the current level from order[head : tail) on, in one workgroup,
// while they hold at most fuse entries and no hub item (hubtail: the hubq
// cursor at launch). Leaves meta[M_FUSED] = rounds done and meta[M_HEAD] =
// the first entry not processed. Returns -1 (and launches nothing) if the
// first round does not qualify.
int lux_gpu_kcore_tail(uint64_t stream, V_ID nv, const E_ID* aptr,
                       const V_ID* aadj, int* deg, V_ID* order,
                       uint32_t* hubq, uint32_t hubcap, uint32_t* meta,
                       uint32_t hub, int k, uint32_t head, uint32_t tail,
                       uint32_t hubtail, uint32_t fuse) {
  if (!hub || !fuse || fuse > KCORE_FUSE_MAX || tail > nv || head >= tail ||
      tail - head > fuse || hubtail > hubcap)
    return -1;
  KcArgs a{aptr, aadj, deg, order, hubq, meta, nv, hubcap, hub, k};
  hipLaunchKernelGGL(kcore_tail_kernel, dim3(1), dim3(KCORE_TAIL_BLOCK), 0,
                     (hipStream_t)stream, a, head, tail, hubtail, fuse);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// bad: one u64, added to: the vertices that violate a necessary condition.
void lux_gpu_kcore_check(uint64_t stream, V_ID nv, const E_ID* aptr,
                         const V_ID* aadj, const int* core,
                         unsigned long long* bad) {
  if (!nv) return;
  hipLaunchKernelGGL(kcore_check_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, aptr, aadj, core, bad);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
