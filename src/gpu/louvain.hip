// Community detection by modularity optimisation (Louvain; Blondel et al.
// 2008), one colour class of a greedy colouring at a time: decide and apply
// kernels (group / wave / table / hub roles of a row's best community), a
// fused single-workgroup launch, check mode, the sweep statistics and the
// contraction kernels for gfx950. No reference equivalent.
//
// Definition (API.md): a level graph has a symmetric adjacency aptr / aadj
// with u32 weights aw, self[v] (twice the weight contracted inside v) and
// k[v] = self[v] + the row's weights; W = sum k < 2^32. A member v of the
// class with a neighbour computes a(c), the weight of its entries whose end
// lies in community c, from comm and tot as they stand when the class starts,
//   score(c) = a(c) * W - k[v] * (tot[c] - (c == A ? k[v] : 0)),  A = comm[v],
// and moves to the c != A of largest score (the smallest c among equals) iff
// that score is strictly larger than score(A).
//
// The score needs 65 signed bits: both products fit u64 (every factor is
// below 2^32), so a score is kept as two limbs, lo = a * W - k * tot modulo
// 2^64 and hi = -1 if that wrapped, else 0. Every role reduces (hi, lo, c)
// triples by "better": larger hi, then larger lo, then smaller c. A's own
// entries are summed apart (aA) and never compete, so the winner among the
// others moves iff it beats score(A).
//   group  deg <= 16: four rows per wave in 16-lane groups. A lane holds one
//          entry (c, w); a(c) comes from rotating the pairs round the group
//          with shuffles, aA from a butterfly sum, the best triple from a
//          butterfly over the group. Every lane fetches tot of its own c.
//   wave   17 <= deg <= 64: the same over all 64 lanes, one row per wave.
//   table  65 <= deg <= hub: one row per wave on the wave's quarter of the
//          workgroup's LDS table of (community, u32 weight sum), open
//          addressing with linear probing: an LDS atomicCAS claims the slot,
//          an atomicAdd accumulates. The scan that clears the used slots
//          fetches tot[c] from global memory and scores each of them.
//   hub    deg > hub: work items (vertex, p) for p < P = ceil(deg / (table /
//          2)), one workgroup each on the whole table. Item p owns the
//          communities with mix(c) % P == p; a share that does not fit is cut
//          into S = 2, 4, ... sub-passes by (mix(c) / P) % S. The item writes
//          its best triple to hubbest[item]; the item whose increment of
//          hubdone[row] sees P - 1 reduces the P triples in item order, sums
//          aA over the row and writes the decision.
//
// Decisions go to next[]; nothing a decide launch writes is read by another
// row of that launch. The apply kernel covers the class: comm[v] = next[v],
// tot[A] -= k[v], tot[c] += k[v] by u64 integer atomics (order-independent),
// and the movers are counted into meta. The fused launch is ONE workgroup
// looping over consecutive small classes: decide, fence + barrier, apply,
// fence + barrier; it reads comm, tot and next with agent-scope loads.
//
// Check mode: the decide body over all classes as one set, nothing written
// but meta[LVM_BAD], the rows that would move.
//
// Contraction: the relabel kernel turns every entry into the record
// (dense[comm[v]] << 32 | dense[comm[u]], w), or adds it to self' when both
// ends share a community; after a sort by key the heads kernel marks the first
// record of every run and counts the coarse degrees, and the run-reduce
// kernel sums each run with a segmented wave scan, one atomic per run and
// wave. The same two kernels build the level-0 rows from the arc records.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t LV_HUB = 1024;        // default longest table-role row
constexpr uint32_t LV_TABLE = 8192;      // default slots of the LDS table
constexpr uint32_t LV_TABLE_MIN = 64, LV_TABLE_MAX = 16384;
constexpr uint32_t LV_FUSE = 1024;       // default vertices of a fused launch
constexpr uint32_t LV_FUSE_MAX = 65536;
constexpr uint32_t LV_GROUP = 16;        // lanes of a group-role row
constexpr uint32_t LV_EMPTY = 0xFFFFFFFFu;  // a free slot; no community is -1
constexpr uint32_t LV_PROBES = 256;      // hub role: longest probe sequence
constexpr int LV_MAX_GRID = 1 << 16;     // blocks per role
constexpr int LV_NW = BLOCK / WAVE;
constexpr long long LV_SENT = 0x7FFFFFFFFFFFFFFFll;  // a record to drop
enum { LVM_MOVED = 0, LVM_IN = 1, LVM_SQ = 2, LVM_BAD = 3, LVM_WORDS = 4 };
enum { LVR_NONE = 0, LVR_GROUP = 1, LVR_WAVE = 2, LVR_TABLE = 3 };

using LvArgs = lux_louvain_args;

// A score in two limbs and its community; hi = -2 is "no candidate".
struct LvBest {
  unsigned long long lo;
  int hi;
  uint32_t c;
};
__device__ __forceinline__ LvBest lv_none() {
  return LvBest{0ull, -2, LV_EMPTY};
}
// a * W - kv * t; a, W, kv, t < 2^32.
__device__ __forceinline__ LvBest lv_score(uint32_t a, unsigned long long W,
                                           uint32_t kv, unsigned long long t,
                                           uint32_t c) {
  const unsigned long long p = a * W, q = kv * t;
  return LvBest{p - q, p < q ? -1 : 0, c};
}
__device__ __forceinline__ bool lv_better(const LvBest& x, const LvBest& y) {
  if (x.hi != y.hi) return x.hi > y.hi;
  if (x.lo != y.lo) return x.lo > y.lo;
  return x.c < y.c;
}
__device__ __forceinline__ LvBest lv_shfl_xor(const LvBest& x, int m) {
  LvBest o;
  uint32_t lo = __shfl_xor((uint32_t)x.lo, m, WAVE);
  uint32_t hi = __shfl_xor((uint32_t)(x.lo >> 32), m, WAVE);
  o.lo = ((unsigned long long)hi << 32) | lo;
  o.hi = __shfl_xor(x.hi, m, WAVE);
  o.c = __shfl_xor(x.c, m, WAVE);
  return o;
}
// The best over the W lanes (a power of two) around each lane, in all.
template <int W>
__device__ __forceinline__ LvBest lv_best_over(LvBest b) {
  for (int off = W / 2; off > 0; off >>= 1) {
    LvBest o = lv_shfl_xor(b, off);
    if (lv_better(o, b)) b = o;
  }
  return b;
}
template <int W>
__device__ __forceinline__ uint32_t lv_sum_over(uint32_t x) {
  for (int off = W / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

// comm, tot and next cross waves inside the fused launch: agent-scope
// relaxed accesses there (COH), plain loads elsewhere.
template <bool COH>
__device__ __forceinline__ uint32_t lv_comm_of(const LvArgs& a, V_ID u) {
  if (COH)
    return __hip_atomic_load(&a.comm[u], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  return a.comm[u];
}
template <bool COH>
__device__ __forceinline__ unsigned long long lv_tot_of(const LvArgs& a,
                                                        uint32_t c) {
  if (c >= a.nv) return 0;
  if (COH)
    return __hip_atomic_load(&a.tot[c], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  return a.tot[c];
}
__device__ __forceinline__ void lv_set_next(const LvArgs& a, V_ID v,
                                            uint32_t c) {
  __hip_atomic_store(&a.next[v], c, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Orders a wave's own LDS accesses.
__device__ __forceinline__ void lv_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lv_mix(uint32_t x) {  // murmur3 fmix32
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// The community v goes to: the best of the others if it beats score(A), the
// score of staying, else A.
template <bool COH>
__device__ __forceinline__ uint32_t lv_decide(const LvArgs& a, V_ID v,
                                              uint32_t A, uint32_t aA,
                                              const LvBest& best) {
  if (best.hi == -2) return A;
  const uint32_t kv = a.k[v];
  const LvBest own = lv_score(aA, a.W, kv, lv_tot_of<COH>(a, A) - kv, A);
  const bool wins = best.hi != own.hi ? best.hi > own.hi : best.lo > own.lo;
  return wins ? best.c : A;
}

// Group (W = 16) and wave (W = 64) role: the row of every W-lane group with
// `active` set, deg <= W; steps >= deg of every active group, the same in
// all lanes of the wave, which must call this together. Returns whether the
// group's row moves, in each of its lanes.
template <int W, bool COH, bool CHECK>
__device__ __forceinline__ bool lv_rotate(const LvArgs& a, bool active,
                                          V_ID v, E_ID b, uint32_t deg,
                                          uint32_t steps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t sub = lane & (W - 1);
  const int gbase = lane - (int)sub;
  bool have = active && sub < deg;
  V_ID u = have ? a.aadj[b + sub] : a.nv;
  if (u >= a.nv) have = false;
  const uint32_t c = have ? lv_comm_of<COH>(a, u) : LV_EMPTY;
  const uint32_t w = have ? a.aw[b + sub] : 0u;
  const uint32_t A = active ? lv_comm_of<COH>(a, v) : 0u;
  uint32_t sum = 0;
  for (uint32_t s = 0; s < steps; s++) {
    uint32_t idx = sub + s;  // sub, s < deg: one turn round the row
    if (idx >= deg) idx -= deg;
    const int src = gbase + (int)(idx & (W - 1));
    uint32_t oc = __shfl(c, src, WAVE);
    uint32_t ow = __shfl(w, src, WAVE);
    sum += (have && s < deg && oc == c) ? ow : 0u;
  }
  const uint32_t aA = lv_sum_over<W>(have && c == A ? w : 0u);
  const bool cand = have && c != A;
  LvBest mine = lv_none();
  if (cand) mine = lv_score(sum, a.W, a.k[v], lv_tot_of<COH>(a, c), c);
  const LvBest best = lv_best_over<W>(mine);
  if (!active) return false;
  const uint32_t to = lv_decide<COH>(a, v, A, aA, best);
  if (!CHECK && sub == 0) lv_set_next(a, v, to);
  return to != A;
}

// Add w to community c in the open-addressing table (mask + 1 slots) from
// slot h on; false if `limit` probes find neither c nor a free slot.
__device__ __forceinline__ bool lv_insert(uint32_t* keys, uint32_t* sums,
                                          uint32_t mask, uint32_t c,
                                          uint32_t w, uint32_t h,
                                          uint32_t limit) {
  h &= mask;
  for (uint32_t t = 0; t < limit; t++) {
    uint32_t prev = atomicCAS(&keys[h], LV_EMPTY, c);
    if (prev == LV_EMPTY || prev == c) {
      atomicAdd(&sums[h], w);
      return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

// Table role: row v (65 <= deg <= hub) by one wave on its nslots slots of
// LDS, all free at entry and at exit.
template <bool COH, bool CHECK>
__device__ __forceinline__ bool lv_table_row(const LvArgs& a, V_ID v, E_ID b,
                                             uint32_t deg, uint32_t* keys,
                                             uint32_t* sums,
                                             uint32_t nslots) {
  const int lane = threadIdx.x & (WAVE - 1);
  uint32_t n = 2 * WAVE;
  while (n < 2 * deg && n < nslots) n <<= 1;
  if (n < 2 * deg || n > nslots) return false;  // hub <= table / 8
  const uint32_t A = lv_comm_of<COH>(a, v);
  const uint32_t kv = a.k[v];
  for (uint32_t j = lane; j < deg; j += WAVE) {
    V_ID u = a.aadj[b + j];
    if (u >= a.nv) continue;
    uint32_t c = lv_comm_of<COH>(a, u);
    lv_insert(keys, sums, n - 1, c, a.aw[b + j], lv_mix(c), n);
  }
  lv_wave_sync();
  LvBest best = lv_none();
  uint32_t aA = 0;
  for (uint32_t s = lane; s < n; s += WAVE) {
    uint32_t c = keys[s];
    if (c == LV_EMPTY) continue;
    if (c == A) {
      aA = sums[s];
    } else {
      LvBest mine = lv_score(sums[s], a.W, kv, lv_tot_of<COH>(a, c), c);
      if (lv_better(mine, best)) best = mine;
    }
    keys[s] = LV_EMPTY;
    sums[s] = 0;
  }
  lv_wave_sync();
  best = lv_best_over<WAVE>(best);
  aA = lv_sum_over<WAVE>(aA);
  const uint32_t to = lv_decide<COH>(a, v, A, aA, best);
  if (!CHECK && lane == 0) lv_set_next(a, v, to);
  return to != A;
}

// The entries [lo, hi) of vorder by the waves of the row blocks; ch: this
// lane's count of rows that move (one lane per row).
template <bool COH, bool CHECK>
__device__ __forceinline__ void lv_rows(const LvArgs& a, uint32_t lo,
                                        uint32_t hi, uint32_t row_blocks,
                                        uint32_t* keys, uint32_t* sums,
                                        uint32_t nslots, uint32_t& ch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int g = lane / (int)LV_GROUP;
  const uint32_t sub = lane & (LV_GROUP - 1);
  constexpr uint32_t QUAD = WAVE / LV_GROUP;
  const uint64_t step = (uint64_t)row_blocks * LV_NW * QUAD;
  for (uint64_t q = lo + ((uint64_t)blockIdx.x * LV_NW + wid) * QUAD; q < hi;
       q += step) {
    const uint64_t i = q + g;
    V_ID v = i < hi ? a.vorder[i] : a.nv;
    uint32_t role = LVR_NONE, deg = 0;
    E_ID b = 0;
    if (v < a.nv) {
      b = a.aptr[v];
      uint64_t d = a.aptr[v + 1] - b;
      if (d > 0 && d <= a.hub) {
        deg = (uint32_t)d;
        role = deg <= LV_GROUP ? LVR_GROUP : deg <= WAVE ? LVR_WAVE
                                                         : LVR_TABLE;
      }
    }
    uint32_t steps = role == LVR_GROUP ? deg : 0u;
    for (int off = LV_GROUP; off < WAVE; off <<= 1) {
      uint32_t o = __shfl_xor(steps, off, WAVE);
      steps = o > steps ? o : steps;
    }
    if (steps) {
      bool c = lv_rotate<LV_GROUP, COH, CHECK>(a, role == LVR_GROUP, v, b,
                                               deg, steps);
      if (c && sub == 0) ch++;
    }
    for (int g2 = 0; g2 < (int)QUAD; g2++) {
      const int src = g2 * (int)LV_GROUP;
      uint32_t r = __shfl(role, src, WAVE);
      if (r != LVR_WAVE && r != LVR_TABLE) continue;  // uniform over the wave
      V_ID vv = __shfl(v, src, WAVE);
      uint32_t dd = __shfl(deg, src, WAVE);
      uint32_t blo = __shfl((uint32_t)b, src, WAVE);
      uint32_t bhi = __shfl((uint32_t)(b >> 32), src, WAVE);
      E_ID bb = ((E_ID)bhi << 32) | blo;
      bool c = r == LVR_WAVE
                   ? lv_rotate<WAVE, COH, CHECK>(a, true, vv, bb, dd, dd)
                   : lv_table_row<COH, CHECK>(a, vv, bb, dd, keys, sums,
                                              nslots);
      if (c && lane == 0) ch++;
    }
  }
}

// Hub role: item i = (v, p) of hub row `row` by the whole workgroup on the
// whole table, all free at entry and at exit. All threads call this together.
template <bool CHECK>
__device__ __forceinline__ void lv_hub_item(const LvArgs& a, uint64_t i,
                                            V_ID v, uint32_t p, uint32_t row,
                                            uint32_t* keys, uint32_t* sums,
                                            uint32_t& ch) {
  __shared__ uint32_t s_flag;  // go, then overflow, then last
  __shared__ LvBest s_red[LV_NW];
  __shared__ uint32_t s_sum[LV_NW];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const E_ID b = a.aptr[v];
  const uint64_t deg = a.aptr[v + 1] - b;
  const uint32_t half = a.table / 2;
  const uint32_t P = (uint32_t)((deg + half - 1) / half);
  if (threadIdx.x == 0)
    s_flag = (p < P && p <= i && i - p + P <= a.nitems && row < a.nhub &&
              deg > a.hub) ? 1u : 0u;
  __syncthreads();
  const bool go = s_flag != 0;
  __syncthreads();
  if (!go) return;
  const uint32_t A = lv_comm_of<false>(a, v);
  const uint32_t kv = a.k[v];
  const uint32_t mask = a.table - 1;
  const uint32_t limit = a.table < LV_PROBES ? a.table : LV_PROBES;
  LvBest best = lv_none();
  for (uint32_t S = 1; S != 0; S <<= 1) {
    best = lv_none();
    bool over = false;
    for (uint32_t s = 0; s < S && !over; s++) {
      if (threadIdx.x == 0) s_flag = 0;
      __syncthreads();
      for (uint64_t j = threadIdx.x; j < deg; j += BLOCK) {
        V_ID u = a.aadj[b + j];
        if (u >= a.nv) continue;
        uint32_t c = lv_comm_of<false>(a, u);
        uint32_t hh = lv_mix(c);
        if (c == A || hh % P != p || (hh / P) % S != s) continue;
        if (!lv_insert(keys, sums, mask, c, a.aw[b + j],
                       lv_mix(hh ^ 0x9E3779B9u), limit))
          s_flag = 1;
      }
      __syncthreads();
      over = s_flag != 0;
      for (uint32_t t = threadIdx.x; t <= mask; t += BLOCK) {
        uint32_t c = keys[t];
        if (c == LV_EMPTY) continue;
        if (!over) {
          LvBest mine = lv_score(sums[t], a.W, kv, lv_tot_of<false>(a, c), c);
          if (lv_better(mine, best)) best = mine;
        }
        keys[t] = LV_EMPTY;
        sums[t] = 0;
      }
      __syncthreads();
    }
    if (!over) break;
  }
  best = lv_best_over<WAVE>(best);
  if (lane == 0) s_red[wid] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < LV_NW; w++)
      if (lv_better(s_red[w], best)) best = s_red[w];
    unsigned long long* slot = a.hubbest + 3 * i;
    __hip_atomic_store(&slot[0], best.lo, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&slot[1], (unsigned long long)(long long)best.hi,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&slot[2], (unsigned long long)best.c, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    uint32_t last = atomicAdd(&a.hubdone[row], 1u) + 1 == P ? 1u : 0u;
    if (last) {
      __threadfence();
      atomicExch(&a.hubdone[row], 0u);
    }
    s_flag = last;
  }
  __syncthreads();
  const bool last = s_flag != 0;
  __syncthreads();
  if (!last) return;
  uint32_t aA = 0;  // the row's weight into A, over the whole row
  for (uint64_t j = threadIdx.x; j < deg; j += BLOCK) {
    V_ID u = a.aadj[b + j];
    if (u < a.nv && lv_comm_of<false>(a, u) == A) aA += a.aw[b + j];
  }
  aA = lv_sum_over<WAVE>(aA);
  if (lane == 0) s_sum[wid] = aA;
  __syncthreads();
  if (threadIdx.x == 0) {
    aA = 0;
    for (int w = 0; w < LV_NW; w++) aA += s_sum[w];
    best = lv_none();
    for (uint32_t t = 0; t < P; t++) {  // in item order
      const unsigned long long* slot = a.hubbest + 3 * (i - p + t);
      LvBest o;
      o.lo = __hip_atomic_load(&slot[0], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      o.hi = (int)(long long)__hip_atomic_load(&slot[1], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
      o.c = (uint32_t)__hip_atomic_load(&slot[2], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
      if (lv_better(o, best)) best = o;
    }
    const uint32_t to = lv_decide<false>(a, v, A, aA, best);
    if (!CHECK) lv_set_next(a, v, to);
    if (to != A) ch++;
  }
  __syncthreads();
}

// comm[v] = next[v] for the entries [lo, hi) of vorder, one thread each of
// `nthr` threads, this one `tid`; mv: this thread's movers.
template <bool COH>
__device__ __forceinline__ void lv_apply(const LvArgs& a, uint32_t lo,
                                         uint32_t hi, uint64_t tid,
                                         uint64_t nthr, uint32_t& mv) {
  for (uint64_t i = lo + tid; i < hi; i += nthr) {
    V_ID v = a.vorder[i];
    if (v >= a.nv) continue;
    uint32_t to = COH ? __hip_atomic_load(&a.next[v], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT)
                      : a.next[v];
    uint32_t A = lv_comm_of<COH>(a, v);
    if (to == A || to >= a.nv || A >= a.nv) continue;
    __hip_atomic_store(&a.comm[v], to, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long kv = a.k[v];
    atomicSub(&a.tot[A], kv);
    atomicAdd(&a.tot[to], kv);
    mv++;
  }
}

// Decide for classes [c0, c1): blocks below row_blocks take the rows, the
// others the hub items. FUSED: one workgroup, class after class, decide then
// apply; otherwise the classes are one set and only next[] is written.
// slots: the LDS table of this launch, a.table, or LV_TABLE_MIN for a launch
// without table-role rows and hub items.
template <bool FUSED, bool CHECK>
__global__ void __launch_bounds__(BLOCK) lv_class_kernel(
    LvArgs a, uint32_t c0, uint32_t c1, uint32_t row_blocks,
    uint32_t slots) {
  extern __shared__ uint32_t lv_lds[];
  uint32_t* keys = lv_lds;
  uint32_t* sums = lv_lds + slots;
  for (uint32_t t = threadIdx.x; t < slots; t += BLOCK) {
    keys[t] = LV_EMPTY;
    sums[t] = 0;
  }
  __syncthreads();
  const int wid = threadIdx.x >> 6;
  const uint32_t nslots = slots / LV_NW;
  uint32_t ch = 0, mv = 0;
  if (blockIdx.x < row_blocks) {
    uint32_t* wk = keys + wid * nslots;
    uint32_t* ws = sums + wid * nslots;
    if (FUSED) {
      for (uint32_t c = c0; c < c1; c++) {
        uint32_t lo = a.cptr[c], hi = a.cptr[c + 1];
        if (hi > a.nv) hi = a.nv;
        lv_rows<true, CHECK>(a, lo, hi, 1, wk, ws, nslots, ch);
        __threadfence();  // this class's decisions are out
        __syncthreads();
        lv_apply<true>(a, lo, hi, threadIdx.x, BLOCK, mv);
        __threadfence();  // and its moves
        __syncthreads();
      }
    } else {
      uint32_t lo = a.cptr[c0], hi = a.cptr[c1];
      if (hi > a.nv) hi = a.nv;
      lv_rows<false, CHECK>(a, lo, hi, row_blocks, wk, ws, nslots, ch);
    }
  } else {
    const uint32_t nb = gridDim.x - row_blocks;
    uint32_t end = a.hptr[c1];
    if (end > a.nitems) end = a.nitems;
    for (uint64_t i = (uint64_t)a.hptr[c0] + (blockIdx.x - row_blocks);
         i < end; i += nb) {
      V_ID v = a.hubv[i];
      if (v >= a.nv) continue;  // uniform over the workgroup
      lv_hub_item<CHECK>(a, i, v, a.hubp[i], a.hubr[i], keys, sums, ch);
    }
  }
  ch = wave_reduce_sum(ch);
  mv = wave_reduce_sum(mv);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (CHECK && ch) atomicAdd(&a.meta[LVM_BAD], (unsigned long long)ch);
    if (FUSED && mv) atomicAdd(&a.meta[LVM_MOVED], (unsigned long long)mv);
  }
}

// The apply launch of class c0.
__global__ void __launch_bounds__(BLOCK) lv_apply_kernel(LvArgs a,
                                                         uint32_t c0) {
  uint32_t lo = a.cptr[c0], hi = a.cptr[c0 + 1];
  if (hi > a.nv) hi = a.nv;
  uint32_t mv = 0;
  lv_apply<false>(a, lo, hi, blockIdx.x * (uint64_t)BLOCK + threadIdx.x,
                  (uint64_t)gridDim.x * BLOCK, mv);
  mv = wave_reduce_sum(mv);
  if ((threadIdx.x & (WAVE - 1)) == 0 && mv)
    atomicAdd(&a.meta[LVM_MOVED], (unsigned long long)mv);
}

// meta[LVM_IN] += self[v] + the weights of v's entries inside its community,
// meta[LVM_SQ] += tot[v]^2. A 16-lane group per vertex.
__global__ void __launch_bounds__(BLOCK) lv_stats_kernel(LvArgs a) {
  const uint32_t sub = threadIdx.x & (LV_GROUP - 1);
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x / LV_GROUP;
  unsigned long long in = 0, sq = 0;
  for (uint64_t v = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) /
                    LV_GROUP;
       v < a.nv; v += stride) {
    const E_ID b = a.aptr[v];
    const uint64_t deg = a.aptr[v + 1] - b;
    const uint32_t c = a.comm[v];
    if (sub == 0) {
      const unsigned long long t = a.tot[v];
      in += a.selfw[v];
      sq += t * t;
    }
    for (uint64_t j = sub; j < deg; j += LV_GROUP) {
      V_ID u = a.aadj[b + j];
      if (u < a.nv && a.comm[u] == c) in += a.aw[b + j];
    }
  }
  in = wave_reduce_sum(in);
  sq = wave_reduce_sum(sq);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (in) atomicAdd(&a.meta[LVM_IN], in);
    if (sq) atomicAdd(&a.meta[LVM_SQ], sq);
  }
}

// Contraction, step 1. dense[c]: the coarse id of community c. Entry e of
// row v becomes the record (dense[comm[v]] << 32 | dense[comm[u]], w), or
// LV_SENT with weight 0 if both ends share a community; self2 of the coarse
// vertex gains self[v] and those inside weights. A 16-lane group per vertex.
__global__ void __launch_bounds__(BLOCK) lv_relabel_kernel(
    LvArgs a, const uint32_t* dense, uint32_t n2, long long* keys,
    uint32_t* wrec, uint32_t* self2) {
  const uint32_t sub = threadIdx.x & (LV_GROUP - 1);
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x / LV_GROUP;
  for (uint64_t v = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) /
                    LV_GROUP;
       v < a.nv; v += stride) {
    const E_ID b = a.aptr[v];
    const uint64_t deg = a.aptr[v + 1] - b;
    const uint32_t cv = a.comm[v];
    const uint32_t c = cv < a.nv ? dense[cv] : n2;
    uint32_t inside = sub == 0 ? a.selfw[v] : 0u;
    for (uint64_t j = sub; j < deg; j += LV_GROUP) {
      V_ID u = a.aadj[b + j];
      const uint32_t cu = u < a.nv ? a.comm[u] : a.nv;
      const uint32_t d = cu < a.nv ? dense[cu] : n2;
      const uint32_t w = a.aw[b + j];
      const bool drop = c >= n2 || d >= n2 || c == d;
      if (c == d && c < n2) inside += w;
      keys[b + j] = drop ? LV_SENT : (long long)(((uint64_t)c << 32) | d);
      wrec[b + j] = drop ? 0u : w;
    }
    inside = lv_sum_over<LV_GROUP>(inside);
    if (sub == 0 && inside && c < n2) atomicAdd(&self2[c], inside);
  }
}

// Contraction, step 2, over the nrec records sorted by key: head[i] = 1 for
// the first record of every run of equal keys (0 for LV_SENT), and deg2 of
// the run's row gains one.
__global__ void __launch_bounds__(BLOCK) lv_heads_kernel(
    uint64_t nrec, const long long* keys, uint32_t n2, long long* head,
    uint32_t* deg2) {
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nrec;
       i += stride) {
    const long long key = keys[i];
    const uint32_t c = (uint32_t)((uint64_t)key >> 32);
    const bool h = key != LV_SENT && c < n2 && (i == 0 || keys[i - 1] != key);
    head[i] = h ? 1 : 0;
    if (h) atomicAdd(&deg2[c], 1u);
  }
}

// Contraction, step 3. pos[i]: the inclusive scan of head, so record i
// belongs to coarse entry pos[i] - 1 of nent. A wave takes 64 consecutive
// records; a segmented inclusive scan sums the weights of equal pos, and the
// last lane of each segment adds the sum to aw2[pos - 1] and to k2 of the
// row. The head lanes write aadj2.
__global__ void __launch_bounds__(BLOCK) lv_reduce_kernel(
    uint64_t nrec, const long long* keys, const uint32_t* wrec,
    const long long* pos, uint64_t nent, uint32_t n2, V_ID* aadj2,
    uint32_t* aw2, uint32_t* k2) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  const uint64_t rounds = (nrec + stride - 1) / stride;
  uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride) {
    long long key = i < nrec ? keys[i] : LV_SENT;
    const uint32_t c = (uint32_t)((uint64_t)key >> 32);
    uint64_t e = nent;  // no entry
    if (key != LV_SENT && c < n2) {
      long long p = pos[i];
      if (p >= 1 && (uint64_t)p <= nent) e = (uint64_t)p - 1;
    }
    uint32_t sum = e < nent ? wrec[i] : 0u;
    const uint32_t elo = (uint32_t)e, ehi = (uint32_t)(e >> 32);
    for (int off = 1; off < WAVE; off <<= 1) {
      uint32_t olo = __shfl_up(elo, off, WAVE);
      uint32_t ohi = __shfl_up(ehi, off, WAVE);
      uint32_t os = __shfl_up(sum, off, WAVE);
      if (lane >= off && olo == elo && ohi == ehi) sum += os;
    }
    uint32_t nlo = __shfl_down(elo, 1, WAVE);
    uint32_t nhi = __shfl_down(ehi, 1, WAVE);
    const bool tail = lane == WAVE - 1 || nlo != elo || nhi != ehi;
    if (e >= nent) continue;
    if (i == 0 || keys[i - 1] != key) aadj2[e] = (V_ID)(uint64_t)key;
    if (tail && sum) {
      atomicAdd(&aw2[e], sum);
      atomicAdd(&k2[c], sum);
    }
  }
}

// The longest row the table role takes: a wave's quarter of the table holds
// 2 * deg slots; never below the wave role's 64.
__host__ __forceinline__ uint32_t lv_row_limit(uint32_t hub, uint32_t table) {
  uint32_t t = hub < table / 8 ? hub : table / 8;
  return t < (uint32_t)WAVE ? (uint32_t)WAVE : t;
}

__host__ __forceinline__ bool lv_args_ok(const LvArgs* a) {
  const uint32_t t = a->table;
  return t >= LV_TABLE_MIN && t <= LV_TABLE_MAX && !(t & (t - 1)) &&
         a->hub >= (uint32_t)WAVE &&
         (a->hub == (uint32_t)WAVE || a->hub <= t / 8) &&
         a->W < (1ull << 32);
}

template <bool FUSED, bool CHECK>
__host__ int lv_launch(hipStream_t s, const LvArgs& a, uint32_t c0,
                       uint32_t c1, uint32_t grid, uint32_t row_blocks,
                       uint32_t maxdeg) {
  const bool bare = maxdeg <= (uint32_t)WAVE && grid == row_blocks;
  const uint32_t slots = bare ? LV_TABLE_MIN : a.table;
  auto kern = lv_class_kernel<FUSED, CHECK>;
  static const hipError_t raised = hipFuncSetAttribute(
      (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)(LV_TABLE_MAX * 2 * sizeof(uint32_t)));
  if (raised != hipSuccess) return -2;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK),
                     slots * 2 * sizeof(uint32_t), s, a, c0, c1, row_blocks,
                     slots);
  return 0;
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_louvain_hub_default() { return LV_HUB; }
uint32_t lux_gpu_louvain_table_default() { return LV_TABLE; }
uint32_t lux_gpu_louvain_table_min() { return LV_TABLE_MIN; }
uint32_t lux_gpu_louvain_table_max() { return LV_TABLE_MAX; }
uint32_t lux_gpu_louvain_fuse_default() { return LV_FUSE; }
uint32_t lux_gpu_louvain_fuse_max() { return LV_FUSE_MAX; }
uint32_t lux_gpu_louvain_meta_words() { return LVM_WORDS; }
uint32_t lux_gpu_louvain_row_limit(uint32_t hub, uint32_t table) {
  return lv_row_limit(hub, table);
}

// Classes [c0, c1) holding nrows entries of vorder, the longest of degree
// maxdeg, and nitems hub items. fused: one workgroup decides and applies them
// class after class (no hub item allowed); otherwise c1 == c0 + 1 and the
// class is decided by one launch and applied by a second. Returns -1 (and
// launches nothing) on bad arguments, -2 if the LDS limit cannot be raised.
int lux_gpu_louvain_classes(uint64_t stream, const lux_louvain_args* a,
                            uint32_t c0, uint32_t c1, uint32_t nrows,
                            uint32_t nitems, uint32_t maxdeg, int fused) {
  if (!lv_args_ok(a) || c0 >= c1 || c1 > a->ncls || nrows > a->nv ||
      nitems > a->nitems || (fused && (nitems || nrows > LV_FUSE_MAX)) ||
      (!fused && c1 != c0 + 1))
    return -1;
  if (!nrows && !nitems) return 0;
  int rc;
  if (fused) {
    rc = lv_launch<true, false>((hipStream_t)stream, *a, c0, c1, 1, 1,
                                maxdeg);
  } else {
    uint32_t rb = ceil_div_u32(nrows, WAVE / LV_GROUP * LV_NW);
    if (rb > (uint32_t)LV_MAX_GRID) rb = LV_MAX_GRID;
    uint32_t hb = nitems > (uint32_t)LV_MAX_GRID ? LV_MAX_GRID : nitems;
    rc = lv_launch<false, false>((hipStream_t)stream, *a, c0, c1, rb + hb,
                                 rb, maxdeg);
    if (rc == 0 && nrows)
      hipLaunchKernelGGL(lv_apply_kernel, dim3(grid_for(nrows)), dim3(BLOCK),
                         0, (hipStream_t)stream, *a, c0);
  }
  LUX_POST_LAUNCH(stream);
  return rc;
}

// meta[3] (added to): the rows with a neighbour that would move.
int lux_gpu_louvain_check(uint64_t stream, const lux_louvain_args* a) {
  if (!lv_args_ok(a)) return -1;
  if (!a->nv || !a->ncls) return 0;
  uint32_t rb = ceil_div_u32(a->nv, WAVE / LV_GROUP * LV_NW);
  if (rb > (uint32_t)LV_MAX_GRID) rb = LV_MAX_GRID;
  uint32_t hb = a->nitems > (uint32_t)LV_MAX_GRID ? LV_MAX_GRID : a->nitems;
  int rc = lv_launch<false, true>((hipStream_t)stream, *a, 0, a->ncls,
                                  rb + hb, rb, 0xFFFFFFFFu);
  LUX_POST_LAUNCH(stream);
  return rc;
}

// meta[1] += in, meta[2] += sum tot^2 of the level as it stands.
int lux_gpu_louvain_stats(uint64_t stream, const lux_louvain_args* a) {
  if (!lv_args_ok(a)) return -1;
  if (!a->nv) return 0;
  hipLaunchKernelGGL(lv_stats_kernel,
                     dim3(grid_for((uint64_t)a->nv * LV_GROUP)), dim3(BLOCK),
                     0, (hipStream_t)stream, *a);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// keys i64[entries], wrec u32[entries]: one record per adjacency entry of
// the level; self2 u32[n2], zeroed by the caller, added to.
int lux_gpu_louvain_relabel(uint64_t stream, const lux_louvain_args* a,
                            const uint32_t* dense, uint32_t n2,
                            long long* keys, uint32_t* wrec,
                            uint32_t* self2) {
  if (!lv_args_ok(a) || !n2) return -1;
  if (!a->nv) return 0;
  hipLaunchKernelGGL(lv_relabel_kernel,
                     dim3(grid_for((uint64_t)a->nv * LV_GROUP)), dim3(BLOCK),
                     0, (hipStream_t)stream, *a, dense, n2, keys, wrec,
                     self2);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// head i64[nrec] (written), deg2 u32[n2] (zeroed by the caller, added to).
void lux_gpu_louvain_heads(uint64_t stream, uint64_t nrec,
                           const long long* keys, uint32_t n2,
                           long long* head, uint32_t* deg2) {
  if (!nrec) return;
  hipLaunchKernelGGL(lv_heads_kernel, dim3(grid_for(nrec)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nrec, keys, n2, head, deg2);
  LUX_POST_LAUNCH(stream);
}

// aadj2 u32[nent] (written), aw2 u32[nent] (zeroed by the caller), k2
// u32[n2] (holding self2, added to).
void lux_gpu_louvain_reduce(uint64_t stream, uint64_t nrec,
                            const long long* keys, const uint32_t* wrec,
                            const long long* pos, uint64_t nent, uint32_t n2,
                            lux::V_ID* aadj2, uint32_t* aw2, uint32_t* k2) {
  if (!nrec || !nent) return;
  hipLaunchKernelGGL(lv_reduce_kernel, dim3(grid_for(nrec)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nrec, keys, wrec, pos, nent, n2,
                     aadj2, aw2, k2);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
