// Triangle counting on a degree-oriented DAG: sorted-list intersection
// kernels for gfx950. No reference equivalent.
//
// Input (built by lux_amd/tc_engine.py: orient + build_items): the simple
// undirected graph, relabelled by rank and oriented lo -> hi.
//   optr u64[nv+1], oadj u32[m]; A(x) = oadj[optr[x] : optr[x+1]] is strictly
//   ascending and holds only ids > x.
// For every arc u -> v the kernels count |A(u) ∩ A(v)|: a triangle u < v < w
// is found exactly once, at its arc (u, v), when w of A(v) is found in A(u).
//
// Work items are u32 triples {u, first, last}: the arcs first..last-1 of row
// u (offsets inside the row). The host splits rows into items and groups the
// items by role; the role of a row comes from its out-degree d:
//   small  (d < TC_T1 <= 33):  tc_small_kernel, one wave per item, A(u) held
//                              one entry per lane and searched with
//                              cross-lane reads, four arcs at a time (16
//                              lanes each), no workgroup barrier, no LDS
//                              allocation;
//   staged (TC_T1 <= d <= cap): tc_item_kernel<true>, one workgroup per item,
//                              A(u) copied to LDS (cap entries of dynamic
//                              LDS), a wave per v, lanes striding over A(v);
//   hub    (d > cap):          tc_item_kernel<false>, the same body with the
//                              search in global memory.
// TC_T1, the item length and the default cap live in tc_engine.py; the
// kernels only see item lists and the cap.
//
// v sits at offset p of A(u) and every w of A(v) is > v, so the search
// window of the staged and hub roles is A(u)[p+1 : d); they take A(v) four
// 64-entry strides per trip and search the four keys of a lane in lockstep
// (tc_find4). tc_plain_kernel (one lane per arc, no items, no
// LDS) searches all of A(u) instead: it is the A/B baseline and the check
// oracle, and shares no search-window arithmetic with the role kernels.
//
// LDS banking of the staged search: the lanes of a wave search ascending
// w's in one window, so the first probes (the window's midpoints) read one
// address from every lane, which broadcasts; the lanes only spread over
// distinct dwords in the last steps, where ascending keys land on ascending
// (mostly distinct-bank) positions. The copy is therefore kept linear.
//
// PV (per-vertex counts) is a template flag on all bodies: a hit adds 1 to
// w, a wave (or 16-lane group, or plain lane) adds its per-v sum to v, and
// the item (or plain lane) sum goes to u; u64 atomics into a rank-indexed
// array. The total-only instantiations carry none of these.
#include "gpu_common.h"

namespace lux {

constexpr uint32_t TC_STAGE_MAX = 8192;  // LDS entries (32 KiB) at most
constexpr int TC_MAX_GRID = 1 << 18;     // item kernels: blocks per launch
constexpr int TC_GROUP = 16;             // small role: lanes per arc
constexpr uint32_t TC_SMALL_MAX = 32;    // small role: arcs per row at most
constexpr V_ID TC_PAD = 0xFFFFFFFFu;     // above every vertex id

struct TcArgs {
  const E_ID* optr;       // u64[nv+1]
  const V_ID* oadj;       // u32[m]
  const uint32_t* items;  // u32[3 * nitems]: {u, first, last}
  uint32_t nitems;
  uint32_t cap;           // staged role: LDS entries
  unsigned long long* total;
  unsigned long long* probes;  // elements of A(v) searched
  unsigned long long* pv;      // u64[nv], rank-indexed (PV only)
};

// is w in a[lo : hi) (ascending)?
__device__ __forceinline__ bool tc_find(const V_ID* a, uint32_t lo,
                                        uint32_t hi, V_ID w) {
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    V_ID x = a[mid];
    if (x == w) return true;
    if (x < w) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// Four keys per lane searched in lockstep in a[start : start + n), n >= 1
// and wave-uniform: a branch-free lower bound takes the same ceil(log2 n)
// steps for every key, so the four reads of a step are independent and in
// flight together (gather_range's four-way idiom, applied to the search).
// On exit the lower bound is b: a step that does not advance proves
// a[b + half - 1] >= w and leaves that element inside [b, b + len); if
// every step advanced, b + len is the window's end.
__device__ __forceinline__ void tc_find4(const V_ID* a, uint32_t start,
                                         uint32_t n, const V_ID (&w)[4],
                                         bool (&hit)[4]) {
  uint32_t b0 = start, b1 = start, b2 = start, b3 = start;
  for (uint32_t len = n; len > 1;) {
    uint32_t half = len >> 1;
    V_ID x0 = a[b0 + half - 1], x1 = a[b1 + half - 1],
         x2 = a[b2 + half - 1], x3 = a[b3 + half - 1];
    b0 += x0 < w[0] ? half : 0;
    b1 += x1 < w[1] ? half : 0;
    b2 += x2 < w[2] ? half : 0;
    b3 += x3 < w[3] ? half : 0;
    len -= half;
  }
  hit[0] = a[b0] == w[0];
  hit[1] = a[b1] == w[1];
  hit[2] = a[b2] == w[2];
  hit[3] = a[b3] == w[3];
}

// ---------------- staged / hub role ----------------

template <bool STAGE, bool PV>
__global__ void __launch_bounds__(BLOCK) tc_item_kernel(TcArgs a) {
  extern __shared__ V_ID tc_lds[];
  __shared__ unsigned long long red_hits[BLOCK / WAVE];
  __shared__ unsigned long long red_probes[BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = BLOCK / WAVE;
  unsigned long long block_hits = 0;   // thread 0
  unsigned long long wave_probes = 0;  // wave-uniform
  for (uint32_t i = blockIdx.x; i < a.nitems; i += gridDim.x) {
    V_ID u = a.items[3 * (uint64_t)i];
    uint32_t first = a.items[3 * (uint64_t)i + 1];
    uint32_t last = a.items[3 * (uint64_t)i + 2];
    E_ID ub = a.optr[u];
    uint32_t d = (uint32_t)(a.optr[u + 1] - ub);
    if (last > d) last = d;
    // a row longer than the LDS copy never belongs to this role: skip it
    // (the whole workgroup does) rather than write past the copy
    if (STAGE && d > a.cap) continue;
    const V_ID* au = a.oadj + ub;
    if (STAGE) {
      __syncthreads();  // the previous item's searches are done
      for (uint32_t k = threadIdx.x; k < d; k += BLOCK) tc_lds[k] = au[k];
      __syncthreads();
      au = tc_lds;
    }
    unsigned long long wave_hits = 0;  // wave-uniform
    for (uint32_t p = first + wid; p < last; p += NW) {
      V_ID v = au[p];
      E_ID vb = a.optr[v], ve = a.optr[v + 1];
      uint32_t vhits = 0;
      const uint32_t wn = d - (p + 1);  // window A(u)[p+1 : d)
      E_ID jb = vb;
      // four 64-entry strides of A(v) per trip: three full, the fourth
      // possibly short (its idle lanes search key 0 and are masked)
      for (; wn && jb + 3 * WAVE < ve; jb += 4 * WAVE) {
        E_ID j = jb + lane;
        bool ok3 = j + 3 * WAVE < ve;
        V_ID w[4] = {a.oadj[j], a.oadj[j + WAVE], a.oadj[j + 2 * WAVE],
                     ok3 ? a.oadj[j + 3 * WAVE] : 0};
        bool hit[4];
        tc_find4(au, p + 1, wn, w, hit);
        hit[3] = hit[3] && ok3;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (PV && hit[k]) atomicAdd(&a.pv[w[k]], 1ull);
          vhits += (uint32_t)__popcll(__ballot(hit[k]));
        }
      }
      for (; wn && jb < ve; jb += WAVE) {
        E_ID j = jb + lane;
        bool hit = false;
        if (j < ve) {
          V_ID w = a.oadj[j];
          hit = tc_find(au, p + 1, d, w);
          if (PV && hit) atomicAdd(&a.pv[w], 1ull);
        }
        vhits += (uint32_t)__popcll(__ballot(hit));
      }
      if (PV && vhits && lane == 0)
        atomicAdd(&a.pv[v], (unsigned long long)vhits);
      wave_hits += vhits;
      wave_probes += ve - vb;
    }
    if (lane == 0) red_hits[wid] = wave_hits;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long s = 0;
      for (int w = 0; w < NW; w++) s += red_hits[w];
      if (PV && s) atomicAdd(&a.pv[u], s);
      block_hits += s;
    }
    if (!STAGE) __syncthreads();  // red_hits is rewritten by the next item
  }
  if (lane == 0) red_probes[wid] = wave_probes;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < NW; w++) s += red_probes[w];
    if (block_hits) atomicAdd(a.total, block_hits);
    if (s) atomicAdd(a.probes, s);
  }
}

// ---------------- small role ----------------

// sum over the 16 lanes of a group, valid in every lane of the group
__device__ __forceinline__ uint32_t tc_group_sum(uint32_t v) {
  for (int off = TC_GROUP / 2; off > 0; off >>= 1)
    v += __shfl_xor(v, off, WAVE);
  return v;
}

// Four keys per lane searched in lockstep in the wave's copy of A(u): lane l
// holds A(u)[l] for l < d <= 32 and TC_PAD (above every id) otherwise, so
// the table is 32 ascending entries and every key takes the same five
// steps plus the final compare, each one cross-lane read. All lanes of the
// wave must be active. The whole row is searched: an entry <= v cannot
// equal a w of A(v).
__device__ __forceinline__ void tc_find4_wave(V_ID mine, const V_ID (&w)[4],
                                              bool (&hit)[4]) {
  uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
#pragma unroll
  for (uint32_t half = TC_SMALL_MAX / 2; half >= 1; half >>= 1) {
    V_ID x0 = __shfl(mine, (int)(b0 + half - 1), WAVE),
         x1 = __shfl(mine, (int)(b1 + half - 1), WAVE),
         x2 = __shfl(mine, (int)(b2 + half - 1), WAVE),
         x3 = __shfl(mine, (int)(b3 + half - 1), WAVE);
    b0 += x0 < w[0] ? half : 0;
    b1 += x1 < w[1] ? half : 0;
    b2 += x2 < w[2] ? half : 0;
    b3 += x3 < w[3] ? half : 0;
  }
  hit[0] = __shfl(mine, (int)b0, WAVE) == w[0];
  hit[1] = __shfl(mine, (int)b1, WAVE) == w[1];
  hit[2] = __shfl(mine, (int)b2, WAVE) == w[2];
  hit[3] = __shfl(mine, (int)b3, WAVE) == w[3];
}

template <bool PV>
__global__ void __launch_bounds__(BLOCK) tc_small_kernel(TcArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t grp = lane / TC_GROUP, sub = lane % TC_GROUP;
  constexpr uint32_t NG = WAVE / TC_GROUP;
  uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
  unsigned long long hits = 0, probes = 0;  // per lane
  for (uint64_t i = wave_id; i < a.nitems; i += nwaves) {
    V_ID u = a.items[3 * i];
    uint32_t first = a.items[3 * i + 1], last = a.items[3 * i + 2];
    E_ID ub = a.optr[u];
    uint32_t d = (uint32_t)(a.optr[u + 1] - ub);
    if (last > d) last = d;
    // a row longer than the register copy never belongs to this role: the
    // whole wave skips it
    if (d > TC_SMALL_MAX) continue;
    V_ID mine = (uint32_t)lane < d ? a.oadj[ub + lane] : TC_PAD;
    uint32_t item_hits = 0;  // per lane
    for (uint32_t pb = first; pb < last; pb += NG) {
      uint32_t p = pb + grp;
      bool valid = p < last;
      V_ID v = __shfl(mine, valid ? (int)p : 0, WAVE);
      E_ID vb = 0;
      uint32_t len = 0;
      if (valid) {
        vb = a.optr[v];
        len = (uint32_t)(a.optr[v + 1] - vb);
      }
      uint32_t cnt = 0;
      // four 16-entry strides of A(v) per trip; a lane past the end
      // searches key 0 (below every entry) and is masked
      for (uint32_t jo = sub; __any(jo < len); jo += 4 * TC_GROUP) {
        V_ID w[4];
        bool ok[4], hit[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          ok[k] = jo + k * TC_GROUP < len;
          w[k] = ok[k] ? a.oadj[vb + jo + k * TC_GROUP] : 0;
        }
        tc_find4_wave(mine, w, hit);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          bool h = hit[k] && ok[k];
          if (PV && h) atomicAdd(&a.pv[w[k]], 1ull);
          cnt += (uint32_t)h;
        }
      }
      if (PV) {
        uint32_t g = tc_group_sum(cnt);
        if (g && sub == 0) atomicAdd(&a.pv[v], (unsigned long long)g);
      }
      item_hits += cnt;
      if (sub == 0) probes += len;
    }
    if (PV) {
      uint32_t s = wave_reduce_sum(item_hits);
      if (s && lane == 0) atomicAdd(&a.pv[u], (unsigned long long)s);
    }
    hits += item_hits;
  }
  hits = wave_reduce_sum(hits);
  probes = wave_reduce_sum(probes);
  if (lane == 0) {
    if (hits) atomicAdd(a.total, hits);
    if (probes) atomicAdd(a.probes, probes);
  }
}

// ---------------- plain kernel ----------------

// One lane per arc: the arc's row by a search of optr, a sequential walk of
// A(v), every w searched in the whole of A(u).
template <bool PV>
__global__ void __launch_bounds__(BLOCK) tc_plain_kernel(
    V_ID nv, E_ID m, const E_ID* optr, const V_ID* oadj,
    unsigned long long* total, unsigned long long* probes,
    unsigned long long* pv) {
  __shared__ unsigned long long lds_h[BLOCK / WAVE];
  __shared__ unsigned long long lds_p[BLOCK / WAVE];
  unsigned long long hits = 0, walked = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    // u = the last row with optr[u] <= e
    V_ID lo = 0, hi = nv;
    while (hi - lo > 1) {
      V_ID mid = lo + (hi - lo) / 2;
      if (optr[mid] <= e) lo = mid;
      else hi = mid;
    }
    V_ID u = lo;
    E_ID ub = optr[u];
    uint32_t d = (uint32_t)(optr[u + 1] - ub);
    V_ID v = oadj[e];
    E_ID vb = optr[v], ve = optr[v + 1];
    unsigned long long cnt = 0;
    for (E_ID j = vb; j < ve; j++) {
      V_ID w = oadj[j];
      if (tc_find(oadj + ub, 0, d, w)) {
        cnt++;
        if (PV) atomicAdd(&pv[w], 1ull);
      }
    }
    if (PV && cnt) {
      atomicAdd(&pv[v], cnt);
      atomicAdd(&pv[u], cnt);
    }
    hits += cnt;
    walked += ve - vb;
  }
  hits = block_reduce_sum(hits, lds_h);
  walked = block_reduce_sum(walked, lds_p);
  if (threadIdx.x == 0) {
    if (hits) atomicAdd(total, hits);
    if (walked) atomicAdd(probes, walked);
  }
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_tc_stage_max() { return TC_STAGE_MAX; }
uint32_t lux_gpu_tc_small_max() { return TC_SMALL_MAX; }

// One role's items. role: 0 small, 1 staged (cap LDS entries, every listed
// row has at most cap arcs), 2 hub. counters: u64[2] = {total, probes},
// added to; pv: u64[nv] rank-indexed, added to, or null for the total alone.
// Returns -1 (and launches nothing) on a role or cap it does not know.
int lux_gpu_tc_count_items(uint64_t stream, int role, const E_ID* optr,
                           const V_ID* oadj, const uint32_t* items,
                           uint32_t nitems, uint32_t cap,
                           unsigned long long* counters,
                           unsigned long long* pv) {
  if (role < 0 || role > 2) return -1;
  if (role == 1 && (cap == 0 || cap > TC_STAGE_MAX)) return -1;
  if (!nitems) return 0;
  hipStream_t s = (hipStream_t)stream;
  TcArgs a{optr, oadj, items, nitems, cap, counters, counters + 1, pv};
  if (role == 0) {
    int grid = grid_for((uint64_t)nitems * WAVE);
    if (pv)
      hipLaunchKernelGGL(tc_small_kernel<true>, dim3(grid), dim3(BLOCK), 0, s,
                         a);
    else
      hipLaunchKernelGGL(tc_small_kernel<false>, dim3(grid), dim3(BLOCK), 0,
                         s, a);
  } else {
    int grid = nitems > (uint32_t)TC_MAX_GRID ? TC_MAX_GRID : (int)nitems;
    size_t lds = role == 1 ? (size_t)cap * sizeof(V_ID) : 0;
    if (role == 1) {
      if (pv)
        hipLaunchKernelGGL((tc_item_kernel<true, true>), dim3(grid),
                           dim3(BLOCK), lds, s, a);
      else
        hipLaunchKernelGGL((tc_item_kernel<true, false>), dim3(grid),
                           dim3(BLOCK), lds, s, a);
    } else {
      if (pv)
        hipLaunchKernelGGL((tc_item_kernel<false, true>), dim3(grid),
                           dim3(BLOCK), lds, s, a);
      else
        hipLaunchKernelGGL((tc_item_kernel<false, false>), dim3(grid),
                           dim3(BLOCK), lds, s, a);
    }
  }
  LUX_POST_LAUNCH(stream);
  return 0;
}

// The plain count over all m arcs; counters and pv as above.
void lux_gpu_tc_count_plain(uint64_t stream, V_ID nv, E_ID m,
                            const E_ID* optr, const V_ID* oadj,
                            unsigned long long* counters,
                            unsigned long long* pv) {
  if (!nv || !m) return;
  hipStream_t s = (hipStream_t)stream;
  if (pv)
    hipLaunchKernelGGL(tc_plain_kernel<true>, dim3(grid_for(m)), dim3(BLOCK),
                       0, s, nv, m, optr, oadj, counters, counters + 1, pv);
  else
    hipLaunchKernelGGL(tc_plain_kernel<false>, dim3(grid_for(m)), dim3(BLOCK),
                       0, s, nv, m, optr, oadj, counters, counters + 1, pv);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
