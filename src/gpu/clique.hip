// k-clique counting (3 <= k <= 8) on the degree-oriented DAG: LDS bit-matrix
// kernels for gfx950. No reference equivalent.
//
// Input (lux_amd/tc_engine.py orient): optr u64[nv+1], oadj u32[m];
// A(x) = oadj[optr[x] : optr[x+1]] is strictly ascending and holds only ids
// > x. A k-clique u < v1 < ... < v(k-1) is counted once, at its lowest vertex
// u, as a (k-1)-clique of the DAG induced on A(u). That DAG is a bit matrix
// in LDS: member i of the set owns row i, bit j of row i is set iff j > i and
// set[j] is in A(set[i]). A search is then ANDs and popcounts on LDS words;
// global memory is read only while the matrix is built.
//
// Work items are u32 pairs {u, p}, grouped on the host by the role the
// out-degree d of row u selects:
//   wave  (k-1 <= d <= 64):  cq_wave_kernel, one wave per row, the matrix is
//                            64 words in the wave's own LDS slice, one lane
//                            per first-level member, no workgroup barrier;
//   block (64 < d <= cap):   cq_block_kernel<.., false>, one workgroup per
//                            row, the d x ceil(d/64) matrix in dynamic LDS
//                            next to the staged row and (PV) one u64 counter
//                            per member; launched once per size class with
//                            that class's LDS size;
//   hub   (d > cap):         cq_block_kernel<.., true>, items are single arcs
//                            (u, v = A(u)[p]); the workgroup forms
//                            S = A(u) ∩ A(v) in LDS, builds the matrix on S
//                            and counts (k-2)-cliques there. An arc with
//                            |S| > cap is a spill: it is counted by the
//                            listless search of the plain kernel, the
//                            workgroup's lanes striding over its first level.
//
// Build: a wave per matrix row i; its lanes stride over A(set[i]),
// lower-bound each entry in set[i+1 : n) and OR the hit bits into row i
// (LDS atomicOr; a row has one owner). Rows are ascending, so the walk of
// A(set[i]) stops at the first 64-entry stride that starts above set[n-1].
//
// Count: a depth-first search that only touches LDS. The unit is a group of
// G lanes, G = the power of two >= words per row, at most 16 (one DPP row).
// Lane l of a group holds word l of the candidate set of every level, one
// u64 register per level (the recursion is a template on the vertices still
// to pick, so the stack is registers, at most 6). Descending to member j is
// cand & M[j][l]: rows hold only bits above j. A group finds the next member
// from a ballot of its non-empty words and a broadcast of each; the loop is
// group-uniform. The last level is a popcount. Groups take first-level
// members from an LDS counter, lowest (largest subtree) first. The wave role
// runs the same search with G = 1 and lane = first-level member.
//
// PV (per-vertex counts) is a template flag. Total-only: every lane sums its
// own leaf popcounts and the item is reduced once. PV: the leaf popcount is
// summed over the group with DPP row shifts and handed up the stack, lane 0
// adding each subtree's sum to its member's LDS counter; leaf members get +1
// each by a walk of the leaf word's bits. An item flushes its counters once,
// with u64 global atomics into the rank-indexed array, and adds its sum to u
// (and v in the hub role).
//
// cq_plain_kernel: one lane per arc (u, v1), a listless nested search: level
// t walks A(v(t-1)) and keeps an entry iff a binary search finds it in every
// earlier row. No candidate lists, no LDS, at most 7 row cursors. It is the
// A/B baseline, the spill path and the check oracle, and shares no bit
// arithmetic with the role kernels.
#include "gpu_common.h"

namespace lux {

constexpr uint32_t CQ_CAP_MAX = 1024;  // set members (matrix rows) at most
constexpr uint32_t CQ_WAVE_MAX = 64;   // wave role: arcs per row at most
constexpr int CQ_K_MIN = 3, CQ_K_MAX = 8;
constexpr int CQ_MAX_GRID = 1 << 16;   // block/hub role: blocks per launch
constexpr int CQ_NT_MAX = 1024;        // block/hub role: threads at most
constexpr V_ID CQ_PAD = 0xFFFFFFFFu;   // above every vertex id

typedef unsigned long long cq_u64;

struct CqArgs {
  const E_ID* optr;       // u64[nv+1]
  const V_ID* oadj;       // u32[m]
  const uint32_t* items;  // u32[2 * nitems]: {u, p}
  uint32_t nitems;
  uint32_t cap;           // block: the size class; hub: the cap
  cq_u64* counters;       // {total, set_ops, spills, built_bits}
  cq_u64* pv;             // u64[nv], rank-indexed (PV only)
};

// dynamic LDS of a workgroup whose set holds at most n members
__host__ __device__ constexpr size_t cq_lds_bytes(uint32_t n, bool pv) {
  return (size_t)n * (n / 64) * 8 + (pv ? (size_t)n * 8 : 0) + (size_t)n * 4;
}

// ---------------- the search ----------------

// sum over the G lanes of a group (G a power of two <= 16, wave-uniform),
// valid in every lane: DPP quad permutes, then the half-row and row mirrors
__device__ __forceinline__ uint32_t cq_group_sum(uint32_t v, uint32_t G) {
  if (G >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
  if (G >= 4) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
  if (G >= 8) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
  if (G >= 16) v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
  return v;
}

struct CqGroup {
  const cq_u64* M;  // LDS matrix, nw words per row
  cq_u64* cnt;      // LDS per-member counters (PV)
  uint32_t nw;      // words per row
  uint32_t G;       // lanes per group
  uint32_t l;       // this lane's word
  uint32_t base;    // the group's first lane in the wave
};

// The number of REM-cliques inside the candidate set whose word l this lane
// holds in `cand`. PV: the group's sum, valid in every lane; otherwise this
// lane's share. ops counts the words this lane evaluated.
template <int REM, bool PV>
__device__ __forceinline__ cq_u64 cq_dfs(const CqGroup& g, cq_u64 cand,
                                         uint32_t& ops) {
  const bool live = g.l < g.nw;
  if constexpr (REM == 1) {
    uint32_t c = (uint32_t)__popcll(cand);
    ops += live;
    if (PV) {
      for (cq_u64 x = cand; x; x &= x - 1)
        atomicAdd(&g.cnt[g.l * 64 + (uint32_t)__builtin_ctzll(x)], 1ull);
      c = cq_group_sum(c, g.G);
    }
    return c;
  } else {
    cq_u64 sum = 0;
    uint32_t nz = g.G == 1
        ? (uint32_t)(cand != 0)
        : (uint32_t)(__ballot(cand != 0) >> g.base) & ((1u << g.G) - 1);
    while (nz) {
      uint32_t w = (uint32_t)__builtin_ctz(nz);
      nz &= nz - 1;
      cq_u64 word = g.G == 1 ? cand : __shfl(cand, (int)(g.base + w), WAVE);
      while (word) {
        uint32_t j = w * 64 + (uint32_t)__builtin_ctzll(word);
        word &= word - 1;
        cq_u64 next = live ? cand & g.M[j * g.nw + g.l] : 0;
        ops += live;
        cq_u64 s = cq_dfs<REM - 1, PV>(g, next, ops);
        if (PV && s && g.l == 0) atomicAdd(&g.cnt[j], s);
        sum += s;
      }
    }
    return sum;
  }
}

// first position of set[lo : hi) that is >= w
__device__ __forceinline__ uint32_t cq_lower(const V_ID* set, uint32_t lo,
                                             uint32_t hi, V_ID w) {
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (set[mid] < w) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// is w in a[0 : n) (ascending)?
__device__ __forceinline__ bool cq_find(const V_ID* a, uint32_t n, V_ID w) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    V_ID x = a[mid];
    if (x == w) return true;
    if (x < w) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// ---------------- plain search ----------------

struct CqRow {
  const V_ID* p;
  uint32_t n;
};

// N keys searched in lockstep in a[0 : n), n >= 1: a branch-free lower
// bound takes the same steps for every key, so the N reads of a step are in
// flight together; hit[q] is and-ed with the outcome.
template <int N>
__device__ __forceinline__ void cq_find_n(const V_ID* a, uint32_t n,
                                          const V_ID (&w)[N],
                                          bool (&hit)[N]) {
  uint32_t b[N];
#pragma unroll
  for (int q = 0; q < N; q++) b[q] = 0;
  for (uint32_t len = n; len > 1;) {
    uint32_t half = len >> 1;
    V_ID x[N];
#pragma unroll
    for (int q = 0; q < N; q++) x[q] = a[b[q] + half - 1];
#pragma unroll
    for (int q = 0; q < N; q++) b[q] += x[q] < w[q] ? half : 0;
    len -= half;
  }
#pragma unroll
  for (int q = 0; q < N; q++) hit[q] = hit[q] && a[b[q]] == w[q];
}

constexpr int CQ_PLAIN_KEYS = 4;  // entries filtered per trip (16 at the
//                                   last level measured no faster, r28)

// T vertices are chosen and rows[0 .. T-1] are their rows. Walk
// rows[T-1][start::stride], keep an entry iff it is in every earlier row,
// and count the k-cliques through it. N entries are filtered per trip,
// their searches in lockstep, the latest (in a skewed graph the shortest,
// so the most selective) row first; above the last level the survivors are
// then descended into one after the other.
template <int K, int T, bool PV>
__device__ __forceinline__ cq_u64 cq_plain_level(const CqArgs& a,
                                                 CqRow (&rows)[CQ_K_MAX - 1],
                                                 uint32_t start,
                                                 uint32_t stride) {
  constexpr int N = CQ_PLAIN_KEYS;
  cq_u64 cnt = 0;
  const CqRow r = rows[T - 1];
  for (uint32_t i = start; i < r.n; i += N * stride) {
    V_ID w[N];
    bool ok[N];
    bool any = false;
#pragma unroll
    for (int q = 0; q < N; q++) {
      uint32_t idx = i + q * stride;
      ok[q] = idx < r.n;
      w[q] = ok[q] ? r.p[idx] : 0;  // key 0 is in no row
    }
#pragma unroll
    for (int t = T - 2; t >= 0; t--) {
      any = false;
#pragma unroll
      for (int q = 0; q < N; q++) any = any || ok[q];
      if (!any) break;
      if (rows[t].n) {
        cq_find_n<N>(rows[t].p, rows[t].n, w, ok);
      } else {
#pragma unroll
        for (int q = 0; q < N; q++) ok[q] = false;
      }
    }
    if constexpr (T == K - 1) {
#pragma unroll
      for (int q = 0; q < N; q++)
        if (ok[q]) {
          cnt++;
          if (PV) atomicAdd(&a.pv[w[q]], 1ull);
        }
    } else {
      static_assert(N == 4, "the survivor select below is written for 4");
#pragma unroll 1
      for (int q = 0; q < 4; q++) {
        bool okq = q == 0 ? ok[0] : q == 1 ? ok[1] : q == 2 ? ok[2] : ok[3];
        if (!okq) continue;
        V_ID wq = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
        E_ID wb = a.optr[wq];
        rows[T] = CqRow{a.oadj + wb, (uint32_t)(a.optr[wq + 1] - wb)};
        cq_u64 s = cq_plain_level<K, T + 1, PV>(a, rows, 0, 1);
        if (PV && s) atomicAdd(&a.pv[wq], s);
        cnt += s;
      }
    }
  }
  return cnt;
}

// the k-cliques through the arc (u, v), u's and v's own counts left to the
// caller; the first level is walked from `start` in steps of `stride`
template <int K, bool PV>
__device__ __forceinline__ cq_u64 cq_plain_arc(const CqArgs& a, V_ID u,
                                               V_ID v, uint32_t start,
                                               uint32_t stride) {
  CqRow rows[CQ_K_MAX - 1];
  E_ID ub = a.optr[u], vb = a.optr[v];
  rows[0] = CqRow{a.oadj + ub, (uint32_t)(a.optr[u + 1] - ub)};
  rows[1] = CqRow{a.oadj + vb, (uint32_t)(a.optr[v + 1] - vb)};
  return cq_plain_level<K, 2, PV>(a, rows, start, stride);
}

template <int K, bool PV>
__global__ void __launch_bounds__(BLOCK) cq_plain_kernel(CqArgs a, V_ID nv,
                                                         E_ID m) {
  __shared__ cq_u64 lds_h[BLOCK / WAVE];
  cq_u64 hits = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < m;
       e += stride) {
    // u = the last row with optr[u] <= e
    V_ID lo = 0, hi = nv;
    while (hi - lo > 1) {
      V_ID mid = lo + (hi - lo) / 2;
      if (a.optr[mid] <= e) lo = mid;
      else hi = mid;
    }
    V_ID u = lo, v = a.oadj[e];
    cq_u64 s = cq_plain_arc<K, PV>(a, u, v, 0, 1);
    if (PV && s) {
      atomicAdd(&a.pv[v], s);
      atomicAdd(&a.pv[u], s);
    }
    hits += s;
  }
  hits = block_reduce_sum(hits, lds_h);
  if (threadIdx.x == 0 && hits) atomicAdd(&a.counters[0], hits);
}

// ---------------- wave role ----------------

template <int K, bool PV>
__global__ void __launch_bounds__(BLOCK) cq_wave_kernel(CqArgs a) {
  constexpr int NW = BLOCK / WAVE;
  __shared__ cq_u64 s_m[NW][WAVE];
  __shared__ V_ID s_set[NW][WAVE];
  __shared__ cq_u64 s_cnt[PV ? NW : 1][WAVE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const uint32_t grp = lane / 16, sub = lane % 16;
  cq_u64* M = s_m[wid];
  V_ID* set = s_set[wid];
  cq_u64* cnt = s_cnt[PV ? wid : 0];
  const CqGroup g{M, cnt, 1, 1, 0, lane};
  uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
  cq_u64 hits = 0, ops_all = 0;  // per lane
  uint32_t ops = 0, bits = 0;       // ops: one item's, folded at the next
  for (uint64_t it = wave_id; it < a.nitems; it += nwaves) {
    ops_all += ops;
    ops = 0;
    V_ID u = a.items[2 * it];
    E_ID ub = a.optr[u];
    uint32_t d = (uint32_t)(a.optr[u + 1] - ub);
    // a row longer than the slice never belongs to this role: the whole
    // wave skips it
    if (d > CQ_WAVE_MAX || d < (uint32_t)K - 1) continue;
    V_ID mine = lane < d ? a.oadj[ub + lane] : CQ_PAD;
    set[lane] = mine;
    M[lane] = 0;
    if (PV) cnt[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const V_ID top = set[d - 1];
    // build: four rows per trip, 16 lanes striding over each A(set[i])
    for (uint32_t ib = 0; ib + 1 < d; ib += WAVE / 16) {
      uint32_t i = ib + grp;
      if (i + 1 >= d) continue;
      V_ID vi = set[i];
      E_ID vb = a.optr[vi];
      uint32_t len = (uint32_t)(a.optr[vi + 1] - vb);
      cq_u64 row = 0;
      for (uint32_t jo = sub; jo < len; jo += 16) {
        V_ID w = a.oadj[vb + jo];
        if (w > top) break;
        uint32_t pos = cq_lower(set, i + 1, d, w);
        if (pos < d && set[pos] == w) row |= 1ull << pos;
      }
      if (row) {
        atomicOr(&M[i], row);
        bits += (uint32_t)__popcll(row);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // count: lane j1 owns the subtree of first-level member j1
    cq_u64 s = 0;
    if (lane < d) {
      s = cq_dfs<K - 2, PV>(g, M[lane], ops);
      if (PV && s) atomicAdd(&cnt[lane], s);
    }
    hits += s;
    if (PV) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      cq_u64 c = cnt[lane];
      if (lane < d && c) atomicAdd(&a.pv[mine], c);
      cq_u64 tot = wave_reduce_sum(s);
      if (lane == 0 && tot) atomicAdd(&a.pv[u], tot);
    }
    // the next item rewrites the slice: every lane is past its reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  hits = wave_reduce_sum(hits);
  cq_u64 o = wave_reduce_sum(ops_all + ops),
         b = wave_reduce_sum((cq_u64)bits);
  if (lane == 0) {
    if (hits) atomicAdd(&a.counters[0], hits);
    if (o) atomicAdd(&a.counters[1], o);
    if (b) atomicAdd(&a.counters[3], b);
  }
}

// ---------------- block and hub roles ----------------

// blockDim.x is 256 or 1024; a.cap is the most members the LDS holds
template <int K, bool PV, bool HUB>
__global__ void __launch_bounds__(CQ_NT_MAX) cq_block_kernel(CqArgs a) {
  extern __shared__ cq_u64 cq_lds[];
  __shared__ cq_u64 s_red[3][CQ_NT_MAX / WAVE];
  __shared__ uint32_t s_wcnt[CQ_NT_MAX / WAVE];
  __shared__ uint32_t s_next;
  constexpr int R = HUB ? K - 2 : K - 1;  // clique size inside the matrix
  const uint32_t tid = threadIdx.x, NT = blockDim.x;
  const uint32_t lane = tid & (WAVE - 1), wid = tid >> 6, NW = NT / WAVE;
  const uint32_t cap = a.cap;
  cq_u64* M = cq_lds;
  cq_u64* cnt = M + (size_t)cap * (cap / 64);
  V_ID* set = (V_ID*)(cnt + (PV ? cap : 0));
  cq_u64 hits = 0, ops_all = 0;  // per lane; PV hits: group leaders only
  uint32_t ops = 0, bits = 0;       // ops: one item's, folded at the next
  cq_u64 spills = 0;                // thread 0
  for (uint32_t it = blockIdx.x; it < a.nitems; it += gridDim.x) {
    ops_all += ops;
    ops = 0;
    V_ID u = a.items[2 * (uint64_t)it];
    uint32_t p = a.items[2 * (uint64_t)it + 1];
    E_ID ub = a.optr[u];
    uint32_t d = (uint32_t)(a.optr[u + 1] - ub);
    const V_ID* au = a.oadj + ub;
    __syncthreads();  // the previous item is done with the LDS
    uint32_t n;       // members of the set, workgroup-uniform
    V_ID v = 0;
    if (!HUB) {
      // a row longer than the LDS copy never belongs to this launch: the
      // whole workgroup skips it rather than write past the copy
      if (d > cap) continue;
      n = d;
      for (uint32_t i = tid; i < d; i += NT) set[i] = au[i];
    } else {
      if (p >= d) continue;
      v = au[p];
      E_ID vb = a.optr[v];
      uint32_t lenv = (uint32_t)(a.optr[v + 1] - vb);
      const V_ID* av = a.oadj + vb;
      // S = A(u)[p+1 : d) ∩ A(v), ascending: an ordered compaction of the
      // hits, NT entries of A(v) per trip
      n = 0;
      for (uint32_t base = 0; base < lenv; base += NT) {
        uint32_t idx = base + tid;
        V_ID w = 0;
        bool hit = false;
        if (idx < lenv) {
          w = av[idx];
          hit = cq_find(au + p + 1, d - (p + 1), w);
        }
        cq_u64 bal = __ballot(hit);
        if (lane == 0) s_wcnt[wid] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = n, tot = 0;
        for (uint32_t k = 0; k < NW; k++) {
          uint32_t c = s_wcnt[k];
          off += k < wid ? c : 0;
          tot += c;
        }
        uint32_t pos = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        if (hit && pos < cap) set[pos] = w;
        n += tot;
        __syncthreads();
      }
      if (n > cap) {
        // spill: the listless search, lanes striding over A(v)
        cq_u64 s = cq_plain_arc<K, PV>(a, u, v, tid, NT);
        if (PV && s) {
          atomicAdd(&a.pv[v], s);
          atomicAdd(&a.pv[u], s);
        }
        hits += s;
        if (tid == 0) spills++;
        continue;
      }
    }
    if (n < (uint32_t)R) continue;
    if constexpr (R == 1) {
      // k = 3 in the hub role: every member of S closes one triangle
      __syncthreads();
      if (PV)
        for (uint32_t i = tid; i < n; i += NT) atomicAdd(&a.pv[set[i]], 1ull);
      if (tid == 0) {
        if (PV) {
          atomicAdd(&a.pv[u], (cq_u64)n);
          atomicAdd(&a.pv[v], (cq_u64)n);
        }
        hits += n;
      }
      continue;
    } else {
      const uint32_t nw = (n + 63) / 64;
      uint32_t G = 1;
      while (G < nw) G <<= 1;
      for (uint32_t i = tid; i < n * nw; i += NT) M[i] = 0;
      if (PV)
        for (uint32_t i = tid; i < n; i += NT) cnt[i] = 0;
      if (tid == 0) s_next = 0;
      __syncthreads();
      // build: a wave per row
      const V_ID top = set[n - 1];
      for (uint32_t i = wid; i + 1 < n; i += NW) {
        V_ID vi = set[i];
        E_ID vb = a.optr[vi], ve = a.optr[vi + 1];
        for (E_ID jb = vb; jb < ve; jb += WAVE) {
          if (a.oadj[jb] > top) break;  // wave-uniform
          E_ID j = jb + lane;
          if (j >= ve) continue;
          V_ID w = a.oadj[j];
          uint32_t pos = cq_lower(set, i + 1, n, w);
          if (pos < n && set[pos] == w) {
            atomicOr(&M[i * nw + pos / 64], 1ull << (pos % 64));
            bits++;
          }
        }
      }
      __syncthreads();
      // count: groups of G lanes take first-level members from s_next
      const CqGroup g{M, cnt, nw, G, lane & (G - 1), lane & ~(G - 1)};
      cq_u64 item = 0;
      for (;;) {
        uint32_t j1 = 0;
        if (g.l == 0) j1 = atomicAdd(&s_next, 1u);
        j1 = __shfl(j1, (int)g.base, WAVE);
        if (j1 + (uint32_t)R > n) break;  // too few members above j1
        cq_u64 c1 = g.l < nw ? M[j1 * nw + g.l] : 0;
        cq_u64 s = cq_dfs<R - 1, PV>(g, c1, ops);
        if (PV && s && g.l == 0) atomicAdd(&cnt[j1], s);
        item += (PV && g.l != 0) ? 0 : s;
      }
      hits += item;
      if (PV) {
        // flush: the members' counters, and the item's sum to u (and v)
        item = wave_reduce_sum(item);
        if (lane == 0) s_red[0][wid] = item;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += NT) {
          cq_u64 c = cnt[i];
          if (c) atomicAdd(&a.pv[set[i]], c);
        }
        if (tid == 0) {
          cq_u64 s = 0;
          for (uint32_t k = 0; k < NW; k++) s += s_red[0][k];
          if (s) {
            atomicAdd(&a.pv[u], s);
            if (HUB) atomicAdd(&a.pv[v], s);
          }
        }
      }
    }
  }
  __syncthreads();
  hits = wave_reduce_sum(hits);
  cq_u64 o = wave_reduce_sum(ops_all + ops),
         b = wave_reduce_sum((cq_u64)bits);
  if (lane == 0) {
    s_red[0][wid] = hits;
    s_red[1][wid] = o;
    s_red[2][wid] = b;
  }
  __syncthreads();
  if (tid == 0) {
    cq_u64 h = 0;
    o = b = 0;
    for (uint32_t k = 0; k < NW; k++) {
      h += s_red[0][k];
      o += s_red[1][k];
      b += s_red[2][k];
    }
    if (h) atomicAdd(&a.counters[0], h);
    if (o) atomicAdd(&a.counters[1], o);
    if (spills) atomicAdd(&a.counters[2], spills);
    if (b) atomicAdd(&a.counters[3], b);
  }
}

// ---------------- launchers ----------------

template <int K, bool PV>
__host__ int cq_launch_wave(hipStream_t s, const CqArgs& a) {
  int grid = grid_for((uint64_t)a.nitems * WAVE);
  hipLaunchKernelGGL((cq_wave_kernel<K, PV>), dim3(grid), dim3(BLOCK), 0, s,
                     a);
  return 0;
}

template <int K, bool PV, bool HUB>
__host__ int cq_launch_block(hipStream_t s, const CqArgs& a) {
  auto kern = cq_block_kernel<K, PV, HUB>;
  static const hipError_t raised = hipFuncSetAttribute(
      (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)cq_lds_bytes(CQ_CAP_MAX, PV));
  if (raised != hipSuccess) return -2;
  int grid = a.nitems > (uint32_t)CQ_MAX_GRID ? CQ_MAX_GRID : (int)a.nitems;
  // above 512 members one workgroup fills a CU's LDS: give it 16 waves
  int nt = a.cap > 512 ? CQ_NT_MAX : BLOCK;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), cq_lds_bytes(a.cap, PV), s,
                     a);
  return 0;
}

template <int K, bool PV>
__host__ int cq_launch_plain(hipStream_t s, const CqArgs& a, V_ID nv,
                             E_ID m) {
  hipLaunchKernelGGL((cq_plain_kernel<K, PV>), dim3(grid_for(m)), dim3(BLOCK),
                     0, s, a, nv, m);
  return 0;
}

template <int K>
__host__ int cq_launch_role(hipStream_t s, int role, const CqArgs& a) {
  const bool pv = a.pv != nullptr;
  if (role == 0)
    return pv ? cq_launch_wave<K, true>(s, a) : cq_launch_wave<K, false>(s, a);
  if (role == 1)
    return pv ? cq_launch_block<K, true, false>(s, a)
              : cq_launch_block<K, false, false>(s, a);
  return pv ? cq_launch_block<K, true, true>(s, a)
            : cq_launch_block<K, false, true>(s, a);
}

}  // namespace lux

using namespace lux;

#define CQ_SWITCH_K(k, call)     \
  switch (k) {                   \
    case 3: rc = call(3); break; \
    case 4: rc = call(4); break; \
    case 5: rc = call(5); break; \
    case 6: rc = call(6); break; \
    case 7: rc = call(7); break; \
    case 8: rc = call(8); break; \
    default: rc = -1;            \
  }

extern "C" {

uint32_t lux_gpu_clique_cap_max() { return CQ_CAP_MAX; }
uint32_t lux_gpu_clique_k_max() { return CQ_K_MAX; }
uint32_t lux_gpu_clique_wave_max() { return CQ_WAVE_MAX; }

// One role's items (u32 pairs {u, p}). role: 0 wave (rows of k-1 .. wave_max
// arcs; cap_or_class is not read), 1 block (cap_or_class = the size class:
// every listed row has at most that many arcs), 2 hub (p = the arc's offset
// in row u; cap_or_class = the cap, the most members of A(u) ∩ A(v) that
// are not a spill). Classes and caps are multiples of 64 in 64..cap_max.
// counters: u64[4] = {total, set_ops, spills, built_bits}, added to; pv:
// u64[nv] rank-indexed, added to, or null for the total alone. Returns -1
// (and launches nothing) on a role, k or cap it does not know, -2 when the
// dynamic-LDS limit cannot be raised.
int lux_gpu_clique_count_items(uint64_t stream, int role, int k,
                               const E_ID* optr, const V_ID* oadj,
                               const uint32_t* items, uint32_t nitems,
                               uint32_t cap_or_class,
                               unsigned long long* counters,
                               unsigned long long* pv) {
  if (role < 0 || role > 2 || k < CQ_K_MIN || k > CQ_K_MAX) return -1;
  if (role != 0 && (cap_or_class < 64 || cap_or_class > CQ_CAP_MAX ||
                    cap_or_class % 64))
    return -1;
  if (!nitems) return 0;
  hipStream_t s = (hipStream_t)stream;
  CqArgs a{optr, oadj, items, nitems, cap_or_class, counters, pv};
  int rc;
#define CQ_ROLE(K) cq_launch_role<K>(s, role, a)
  CQ_SWITCH_K(k, CQ_ROLE)
#undef CQ_ROLE
  if (rc == 0) LUX_POST_LAUNCH(stream);
  return rc;
}

// The plain count over all m arcs; counters and pv as above (only the total
// is added to). Returns -1 on a k it does not know.
int lux_gpu_clique_count_plain(uint64_t stream, int k, V_ID nv, E_ID m,
                               const E_ID* optr, const V_ID* oadj,
                               unsigned long long* counters,
                               unsigned long long* pv) {
  if (k < CQ_K_MIN || k > CQ_K_MAX) return -1;
  if (!nv || !m) return 0;
  hipStream_t s = (hipStream_t)stream;
  CqArgs a{optr, oadj, nullptr, 0, 0, counters, pv};
  int rc;
#define CQ_PLAIN(K)                              \
  (pv ? cq_launch_plain<K, true>(s, a, nv, m)    \
      : cq_launch_plain<K, false>(s, a, nv, m))
  CQ_SWITCH_K(k, CQ_PLAIN)
#undef CQ_PLAIN
  if (rc == 0) LUX_POST_LAUNCH(stream);
  return rc;
}

}  // extern "C"
