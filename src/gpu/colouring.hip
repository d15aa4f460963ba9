// Greedy vertex colouring in a fixed priority order (and with it the
// lexicographically first maximal independent set) by the Jones-Plassmann
// schedule: predecessor / successor split, seed, round step, single-workgroup
// round fusion and a check oracle for gfx950. No reference equivalent.
//
// Definition (API.md): on the simple undirected graph, with a strict total
// order "precedes" on the vertices given as rank u32[nv] (a smaller rank
// precedes), pred(v) = the neighbours that precede v, succ(v) the others,
//   colour[v] = mex{colour[u] : u in pred(v)},
// the sequential greedy colouring in priority order; colour == 0 is the
// first maximal independent set. round[v] = 1 + max round over pred(v).
//
// Input (lux_amd/colouring_engine.py): the id-order DAG of tc_engine.orient,
// optr u64[nv+1] / oadj u32[m], row lo listing its neighbours hi > lo.
// gcol_split_count_kernel takes one lane per arc: the endpoint of smaller
// rank gains a successor, the other a predecessor. The host scans the two
// counts into pptr / sptr, and gcol_split_fill_kernel writes padj (row v =
// pred(v), read for colours) and sadj (row v = succ(v), walked to notify)
// through per-row cursors. Each holds m entries; row order does not matter.
// Every index into them is 64-bit.
//
// State of a solve:
//   colour  i32[nv]  -1 until coloured;
//   pending i32[nv]  the uncoloured predecessors, npred at the start;
//   order   u32[nv]  append-only: every vertex exactly once, when its last
//                    predecessor has notified. A round is a range
//                    [head, tail) of it;
//   hubq    u32 pairs {v, item}, append-only: a vertex whose predecessor
//                    row is longer than `hub` gives ONE item GCOL_SELECT, one
//                    whose successor row is longer than `hub` gives
//                    ceil(d / hub) chunk items 0, 1, ... The host sizes hubq
//                    from the two degree arrays, so neither list can
//                    overflow; the appends are bounds-checked all the same;
//   rtail   u32[nv]  rtail[r] = the order cursor at the end of round r + 1,
//                    written by the tail kernel for the rounds it fuses (the
//                    host knows the others);
//   meta    u32[8]   GM_TAIL / GM_HUBTAIL: the append cursors; GM_FUSED /
//                    GM_HEAD: what the tail kernel did.
//
//   gcol_seed_kernel  one lane per vertex: pending == 0 is appended (round 1);
//   gcol_step_kernel  one launch per round, the role from blockIdx.x. Row
//                     blocks take order[head : tail), a wave per entry v:
//                     select (if the predecessor row is at most `hub` long):
//                     the mex over padj row v through the wave's LDS bitmap
//                     window of GCOL_WINDOW bits: lanes atomicOr bit c - base
//                     for every neighbour colour c inside the window, lanes
//                     0..31 then inspect a word each and a ballot finds the
//                     first zero bit; a full window moves base on by
//                     GCOL_WINDOW and rescans the row. mex <= |pred(v)|, so
//                     |pred(v)| / GCOL_WINDOW + 1 passes are enough and the
//                     loop is bounded by that. Notify (if the successor row
//                     is at most `hub` long): a returning atomicSub on
//                     pending[u] for every u of sadj row v; the decrement that
//                     sees 1 appends u for the next round (exactly one does).
//                     Hub blocks take one hubq item each: GCOL_SELECT is the
//                     same select by the whole workgroup on one window, a
//                     chunk item notifies `hub` entries of a successor row.
//                     Every colour a select reads was written by an earlier
//                     launch: a vertex enters order only after all its
//                     predecessors have notified, and they notify in the
//                     round that colours them. Notifying does not need
//                     colour[v], so it runs in the same launch as the select.
//   gcol_tail_kernel  ONE workgroup (GCOL_TAIL_BLOCK threads) runs successive
//                     small rounds (at most `fuse` entries, no hub item) with
//                     a workgroup barrier between them, so a cascade (a path)
//                     costs one launch and one host read. The colours it
//                     reads were written before the previous __syncthreads.
//                     It stops at an empty round (done), or hands a round
//                     that is too large or has a hub item back unprocessed.
//                     Every trip consumes at least one entry of order.
// Nothing here waits for another workgroup: no grid barrier, no cooperative
// launch, no spinning.
//
// gcol_check_kernel is the device oracle, a plain one-lane-per-vertex walk
// sharing nothing with the above.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t GCOL_HUB = 1024;        // default longest row-role row
constexpr uint32_t GCOL_FUSE = 16;         // default tail-kernel round size
constexpr uint32_t GCOL_FUSE_MAX = 65536;  // what the tail kernel accepts
constexpr uint32_t GCOL_WINDOW = 1024;     // bits of a bitmap window
constexpr int GCOL_WORDS = GCOL_WINDOW / 32;  // one word per lane 0..31
constexpr int GCOL_TAIL_BLOCK = 1024;      // tail kernel: 16 waves
constexpr int GCOL_MAX_GRID = 1 << 16;     // step: blocks per role
constexpr uint32_t GCOL_SELECT = 0xFFFFFFFFu;  // hubq item: select, no chunk
enum { GM_TAIL = 0, GM_HUBTAIL = 1, GM_FUSED = 2, GM_HEAD = 3, GM_WORDS = 8 };
static_assert(GCOL_WORDS <= WAVE / 2 && GCOL_WORDS * 32 == (int)GCOL_WINDOW,
              "a window is one 32-bit word per lane of the lower half-wave");

using GcArgs = lux_gcol_args;  // the split graph and the state of a solve

// Colours and queue entries cross waves inside the tail kernel: agent-scope
// relaxed accesses, so that no wave works from a stale cached line.
__device__ __forceinline__ int gcol_colour_of(const GcArgs& a, V_ID u) {
  return __hip_atomic_load(&a.colour[u], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gcol_set_colour(const GcArgs& a, V_ID v,
                                                int c) {
  __hip_atomic_store(&a.colour[v], c, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Orders a wave's own LDS accesses (the hardware executes them in issue
// order; this keeps the compiler from moving them).
__device__ __forceinline__ void gcol_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Append the u of every lane with enq set to order, and its hub items to
// hubq: one atomic on the cursor per wave. All lanes of the wave must call
// this together.
__device__ __forceinline__ void gcol_enqueue(const GcArgs& a, bool enq,
                                             V_ID u) {
  unsigned long long mask = __ballot(enq);
  if (!mask) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader)
    base = atomicAdd(&a.meta[GM_TAIL], (uint32_t)__popcll(mask));
  base = __shfl(base, leader, WAVE);
  if (!enq) return;
  uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
  if (at < a.nv) a.order[at] = u;
  uint64_t dp = a.pptr[u + 1] - a.pptr[u];
  uint64_t ds = a.sptr[u + 1] - a.sptr[u];
  uint32_t sel = dp > a.hub ? 1u : 0u;
  uint32_t nc = ds > a.hub ? (uint32_t)((ds + a.hub - 1) / a.hub) : 0u;
  if (sel + nc) {
    uint32_t h = atomicAdd(&a.meta[GM_HUBTAIL], sel + nc);
    if (sel && h < a.hubcap) {
      a.hubq[2 * (uint64_t)h] = u;
      a.hubq[2 * (uint64_t)h + 1] = GCOL_SELECT;
    }
    h += sel;
    for (uint32_t c = 0; c < nc && h + c < a.hubcap; c++) {
      a.hubq[2 * (uint64_t)(h + c)] = u;
      a.hubq[2 * (uint64_t)(h + c) + 1] = c;
    }
  }
}

// The first zero bit of the window, as base + its index, or -1 if the
// window is full. Every lane of the calling wave gets the same answer.
__device__ __forceinline__ int gcol_first_zero(const uint32_t* win,
                                               uint32_t base) {
  const int lane = threadIdx.x & (WAVE - 1);
  uint32_t word = lane < GCOL_WORDS ? win[lane] : 0xFFFFFFFFu;
  unsigned long long open = __ballot(word != 0xFFFFFFFFu);
  if (!open) return -1;
  int l = __ffsll((long long)open) - 1;
  uint32_t w = __shfl(word, l, WAVE);
  return (int)(base + 32u * (uint32_t)l + (uint32_t)(__ffs((int)~w) - 1));
}

// Mark the colours of padj[b + sub], padj[b + sub + step], ... that fall in
// [base, base + GCOL_WINDOW).
__device__ __forceinline__ void gcol_mark(const GcArgs& a, uint32_t* win,
                                          E_ID b, uint32_t d, uint32_t base,
                                          uint32_t sub, uint32_t step) {
  for (uint32_t j = sub; j < d; j += step) {
    V_ID u = a.padj[b + j];
    if (u >= a.nv) continue;
    uint32_t off = (uint32_t)gcol_colour_of(a, u) - base;  // -1 wraps high
    if (off < GCOL_WINDOW) atomicOr(&win[off >> 5], 1u << (off & 31));
  }
}

// colour[v] by one wave; win: this wave's GCOL_WORDS words of LDS. d, the
// length of padj row v, is the same in every lane.
__device__ __forceinline__ void gcol_select_wave(const GcArgs& a, V_ID v,
                                                 E_ID b, uint32_t d,
                                                 uint32_t* win) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t passes = d / GCOL_WINDOW + 1;  // mex <= d
  int c = -1;
  for (uint32_t p = 0; p < passes && c < 0; p++) {
    const uint32_t base = p * GCOL_WINDOW;
    if (lane < GCOL_WORDS) win[lane] = 0;
    gcol_wave_sync();
    gcol_mark(a, win, b, d, base, lane, WAVE);
    gcol_wave_sync();
    c = gcol_first_zero(win, base);
    gcol_wave_sync();  // the next pass zeroes behind these reads
  }
  if (lane == 0) gcol_set_colour(a, v, c);
}

// colour[v] by the whole workgroup (all its threads call this together).
__device__ __forceinline__ void gcol_select_block(const GcArgs& a, V_ID v,
                                                  E_ID b, uint64_t d,
                                                  uint32_t* win) {
  const uint64_t passes = d / GCOL_WINDOW + 1;
  int c = -1;
  for (uint64_t p = 0; p < passes && c < 0; p++) {
    const uint32_t base = (uint32_t)(p * GCOL_WINDOW);
    if (threadIdx.x < GCOL_WORDS) win[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t j = threadIdx.x; j < d; j += blockDim.x) {
      V_ID u = a.padj[b + j];
      if (u >= a.nv) continue;
      uint32_t off = (uint32_t)gcol_colour_of(a, u) - base;
      if (off < GCOL_WINDOW) atomicOr(&win[off >> 5], 1u << (off & 31));
    }
    __syncthreads();
    c = gcol_first_zero(win, base);  // every wave finds the same
    __syncthreads();
  }
  if (threadIdx.x == 0) gcol_set_colour(a, v, c);
}

// Notify the entries sub, sub + step, ... of sadj[b : b + n); n is the same
// in every lane of a wave.
__device__ __forceinline__ void gcol_notify(const GcArgs& a, E_ID b,
                                            uint32_t n, uint32_t sub,
                                            uint32_t step) {
  for (uint32_t j = sub; __any(j < n); j += step) {
    bool enq = false;
    V_ID u = 0;
    if (j < n) {
      u = a.sadj[b + j];
      if (u < a.nv) enq = atomicSub(&a.pending[u], 1) == 1;
    }
    gcol_enqueue(a, enq, u);
  }
}

// One entry of a round by one wave: select and notify, each if its row is
// not a hub row.
__device__ __forceinline__ void gcol_entry(const GcArgs& a, V_ID v,
                                           uint32_t* win) {
  const int lane = threadIdx.x & (WAVE - 1);
  if (v >= a.nv) return;
  E_ID pb = a.pptr[v], sb = a.sptr[v];
  uint64_t dp = a.pptr[v + 1] - pb, ds = a.sptr[v + 1] - sb;
  if (dp <= a.hub) gcol_select_wave(a, v, pb, (uint32_t)dp, win);
  if (ds <= a.hub) gcol_notify(a, sb, (uint32_t)ds, lane, WAVE);
}

// ---------------- predecessor / successor split ----------------

// The row of DAG arc e: the last u with optr[u] <= e.
__device__ __forceinline__ V_ID gcol_arc_row(const E_ID* optr, V_ID nv,
                                             E_ID e) {
  V_ID u = 0;
  for (V_ID len = nv; len > 1;) {
    V_ID half = len >> 1;
    u += optr[u + half] <= e ? half : 0;
    len -= half;
  }
  return u;
}

__global__ void __launch_bounds__(BLOCK) gcol_split_count_kernel(
    V_ID nv, E_ID m, const E_ID* optr, const V_ID* oadj,
    const uint32_t* rank, uint32_t* npred, uint32_t* nsucc) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    V_ID lo = gcol_arc_row(optr, nv, e);
    V_ID hi = oadj[e];
    if (hi >= nv) continue;
    bool lo_first = rank[lo] < rank[hi];
    atomicAdd(&nsucc[lo_first ? lo : hi], 1u);
    atomicAdd(&npred[lo_first ? hi : lo], 1u);
  }
}

__global__ void __launch_bounds__(BLOCK) gcol_split_fill_kernel(
    V_ID nv, E_ID m, const E_ID* optr, const V_ID* oadj,
    const uint32_t* rank, const E_ID* pptr, const E_ID* sptr,
    uint32_t* pcur, uint32_t* scur, V_ID* padj, V_ID* sadj) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    V_ID lo = gcol_arc_row(optr, nv, e);
    V_ID hi = oadj[e];
    if (hi >= nv) continue;
    bool lo_first = rank[lo] < rank[hi];
    V_ID first = lo_first ? lo : hi, second = lo_first ? hi : lo;
    E_ID is = sptr[first] + atomicAdd(&scur[first], 1u);
    if (is < sptr[first + 1]) sadj[is] = second;
    E_ID ip = pptr[second] + atomicAdd(&pcur[second], 1u);
    if (ip < pptr[second + 1]) padj[ip] = first;
  }
}

// ---------------- round 1 ----------------

__global__ void __launch_bounds__(BLOCK) gcol_seed_kernel(GcArgs a) {
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  // whole waves trip together: the enqueue is a wave operation
  for (uint64_t v0 = blockIdx.x * (uint64_t)blockDim.x +
                     (threadIdx.x & ~(WAVE - 1));
       v0 < a.nv; v0 += stride) {
    uint64_t v = v0 + (threadIdx.x & (WAVE - 1));
    bool enq = v < a.nv && a.pending[v] == 0;
    gcol_enqueue(a, enq, (V_ID)v);
  }
}

// ---------------- one round ----------------

__global__ void __launch_bounds__(BLOCK) gcol_step_kernel(
    GcArgs a, uint32_t head, uint32_t tail, uint32_t hubhead,
    uint32_t hubtail, uint32_t row_blocks) {
  constexpr int NW = BLOCK / WAVE;
  __shared__ uint32_t win[NW * GCOL_WORDS];
  const int wid = threadIdx.x >> 6;
  if (blockIdx.x < row_blocks) {
    uint64_t step = (uint64_t)row_blocks * NW;
    for (uint64_t i = head + (uint64_t)blockIdx.x * NW + wid; i < tail;
         i += step)
      gcol_entry(a, a.order[i], win + wid * GCOL_WORDS);
  } else {
    uint32_t nb = gridDim.x - row_blocks;
    for (uint64_t i = hubhead + (blockIdx.x - row_blocks); i < hubtail;
         i += nb) {
      V_ID v = a.hubq[2 * i];
      uint32_t item = a.hubq[2 * i + 1];
      if (v >= a.nv) continue;  // uniform over the workgroup, like item
      if (item == GCOL_SELECT) {
        E_ID b = a.pptr[v];
        gcol_select_block(a, v, b, a.pptr[v + 1] - b, win);
      } else {
        uint64_t first = (uint64_t)item * a.hub;
        E_ID b = a.sptr[v];
        uint64_t d = a.sptr[v + 1] - b;
        uint32_t n = 0;
        if (first < d) n = d - first < a.hub ? (uint32_t)(d - first) : a.hub;
        gcol_notify(a, b + first, n, threadIdx.x, BLOCK);
      }
    }
  }
}

// ---------------- small-round fusion ----------------

// One workgroup. The host launches it on a round [head, tail) of at most
// fuse entries with no hub item pending (hubtail = the hubq cursor then);
// round0 = the rounds done before it.
__global__ void __launch_bounds__(GCOL_TAIL_BLOCK) gcol_tail_kernel(
    GcArgs a, uint32_t head, uint32_t tail, uint32_t hubtail, uint32_t fuse,
    uint32_t round0) {
  constexpr int NW = GCOL_TAIL_BLOCK / WAVE;
  __shared__ uint32_t win[NW * GCOL_WORDS];
  __shared__ uint32_t lds_tail, lds_hubtail;
  const int wid = threadIdx.x >> 6;
  uint32_t rounds = 0;
  for (;;) {
    for (uint32_t i = head + wid; i < tail; i += NW) {
      V_ID v = __hip_atomic_load(&a.order[i], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      gcol_entry(a, v, win + wid * GCOL_WORDS);
    }
    if (threadIdx.x == 0 && (uint64_t)round0 + rounds < a.nv)
      a.rtail[round0 + rounds] = tail;
    rounds++;
    head = tail;
    __syncthreads();  // every wave's colours and appends are out
    if (threadIdx.x == 0) {
      lds_tail = __hip_atomic_load(&a.meta[GM_TAIL], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
      lds_hubtail = __hip_atomic_load(&a.meta[GM_HUBTAIL], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    tail = lds_tail;
    // empty: done; too large, a hub item, or a cursor past the list: the
    // host's
    if (tail <= head || tail - head > fuse || lds_hubtail != hubtail ||
        tail > a.nv)
      break;
  }
  if (threadIdx.x == 0) {
    a.meta[GM_FUSED] = rounds;
    a.meta[GM_HEAD] = head;
  }
}

// ---------------- check oracle ----------------

// Necessary conditions of a greedy colouring, per vertex v with c =
// colour[v], over its full neighbourhood (both rows): 0 <= c <= |pred(v)|;
// no neighbour of colour c; if c > 0 a predecessor of colour c - 1 and a
// predecessor of colour 0 (class 0 is maximal). Not sufficient: a gap below
// c - 1 passes. Exactness rests on the CPU oracle.
__global__ void __launch_bounds__(BLOCK) gcol_check_kernel(
    V_ID nv, const E_ID* pptr, const V_ID* padj, const E_ID* sptr,
    const V_ID* sadj, const int* colour, unsigned long long* bad) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long mine = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    long long c = colour[v];
    E_ID pb = pptr[v], pe = pptr[v + 1];
    bool same = false, below = false, zero = false;
    bool wild = false;  // an entry that is no vertex
    for (E_ID j = pb; j < pe; j++) {
      V_ID u = padj[j];
      if (u >= nv) {
        wild = true;
        continue;
      }
      long long cu = colour[u];
      same |= cu == c;
      below |= cu == c - 1;
      zero |= cu == 0;
    }
    for (E_ID j = sptr[v]; j < sptr[v + 1]; j++) {
      V_ID u = sadj[j];
      if (u >= nv)
        wild = true;
      else
        same |= colour[u] == c;
    }
    mine += wild || c < 0 || c > (long long)(pe - pb) || same ||
            (c > 0 && (!below || !zero));
  }
  mine = block_reduce_sum(mine, lds);
  if (threadIdx.x == 0 && mine) atomicAdd(bad, mine);
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_gcol_hub_default() { return GCOL_HUB; }
uint32_t lux_gpu_gcol_fuse_default() { return GCOL_FUSE; }
uint32_t lux_gpu_gcol_fuse_max() { return GCOL_FUSE_MAX; }
uint32_t lux_gpu_gcol_window_bits() { return GCOL_WINDOW; }
uint32_t lux_gpu_gcol_meta_words() { return GM_WORDS; }

// optr / oadj: the id-order DAG (m arcs); rank: u32[nv]; npred / nsucc:
// u32[nv], zeroed, added to.
void lux_gpu_gcol_split_count(uint64_t stream, V_ID nv, E_ID m,
                              const E_ID* optr, const V_ID* oadj,
                              const uint32_t* rank, uint32_t* npred,
                              uint32_t* nsucc) {
  if (!nv || !m) return;
  hipLaunchKernelGGL(gcol_split_count_kernel, dim3(grid_for(m)), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, m, optr, oadj, rank, npred,
                     nsucc);
  LUX_POST_LAUNCH(stream);
}

// pptr / sptr: u64[nv+1], the scanned counts; pcur / scur: u32[nv], zeroed;
// padj / sadj: u32[m], filled.
void lux_gpu_gcol_split_fill(uint64_t stream, V_ID nv, E_ID m,
                             const E_ID* optr, const V_ID* oadj,
                             const uint32_t* rank, const E_ID* pptr,
                             const E_ID* sptr, uint32_t* pcur, uint32_t* scur,
                             V_ID* padj, V_ID* sadj) {
  if (!nv || !m) return;
  hipLaunchKernelGGL(gcol_split_fill_kernel, dim3(grid_for(m)), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, m, optr, oadj, rank, pptr,
                     sptr, pcur, scur, padj, sadj);
  LUX_POST_LAUNCH(stream);
}

// Append every v with pending[v] == 0 (round 1) and its hub items.
void lux_gpu_gcol_seed(uint64_t stream, const lux_gcol_args* g) {
  if (!g->nv) return;
  hipLaunchKernelGGL(gcol_seed_kernel, dim3(grid_for(g->nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, *g);
  LUX_POST_LAUNCH(stream);
}

// One round: order[head : tail) and hubq[hubhead : hubtail) (items), the
// cursors in meta standing at tail and hubtail. Returns -1 (and launches
// nothing) on cursors out of order or beyond the lists.
int lux_gpu_gcol_step(uint64_t stream, const lux_gcol_args* g, uint32_t head,
                      uint32_t tail, uint32_t hubhead, uint32_t hubtail) {
  if (!g->hub) return -1;
  if (tail > g->nv || head > tail || hubtail > g->hubcap || hubhead > hubtail)
    return -1;
  const uint32_t n = tail - head, nh = hubtail - hubhead;
  if (!n && !nh) return 0;
  uint32_t rb = ceil_div_u32(n, BLOCK / WAVE);
  if (rb > (uint32_t)GCOL_MAX_GRID) rb = GCOL_MAX_GRID;
  uint32_t hb = nh > (uint32_t)GCOL_MAX_GRID ? GCOL_MAX_GRID : nh;
  hipLaunchKernelGGL(gcol_step_kernel, dim3(rb + hb), dim3(BLOCK), 0,
                     (hipStream_t)stream, *g, head, tail, hubhead,
                     hubtail, rb);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// Rounds from order[head : tail) on, in one workgroup, while they hold at
// most fuse entries and no hub item (hubtail: the hubq cursor at launch);
// round0: the rounds done so far. Leaves meta[2] = rounds done, meta[3] =
// the first entry not processed, rtail[round0 + i] = the end of its i-th
// round. Returns -1 (and launches nothing) if the first round does not
// qualify.
int lux_gpu_gcol_tail(uint64_t stream, const lux_gcol_args* g, uint32_t head,
                      uint32_t tail, uint32_t hubtail, uint32_t fuse,
                      uint32_t round0) {
  if (!g->hub || !fuse || fuse > GCOL_FUSE_MAX || tail > g->nv ||
      head >= tail || tail - head > fuse || hubtail > g->hubcap ||
      round0 >= g->nv)
    return -1;
  hipLaunchKernelGGL(gcol_tail_kernel, dim3(1), dim3(GCOL_TAIL_BLOCK), 0,
                     (hipStream_t)stream, *g, head, tail, hubtail,
                     fuse, round0);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// bad: one u64, added to: the vertices that violate a necessary condition.
void lux_gpu_gcol_check(uint64_t stream, V_ID nv, const E_ID* pptr,
                        const V_ID* padj, const E_ID* sptr, const V_ID* sadj,
                        const int* colour, unsigned long long* bad) {
  if (!nv) return;
  hipLaunchKernelGGL(gcol_check_kernel, dim3(grid_for(nv)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, pptr, padj, sptr, sadj, colour,
                     bad);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
