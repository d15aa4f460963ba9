// Community detection by semi-synchronous label propagation (Cordasco &
// Gargano): one colour class of a greedy colouring is updated at a time, so a
// parallel sweep equals the sequential pass in (colour, id) order. Class
// kernel (group / wave / table / hub roles of a row mode), check mode and the
// community statistics for gfx950. No reference equivalent.
//
// Definition (API.md): on the simple undirected graph, a sweep visits the
// vertices in (colour, id) order; a vertex v with deg > 0 and dirty[v] clears
// dirty[v], counts cnt(l) = |{u in N(v) : label[u] == l}| and, unless its own
// label reaches the maximum count, takes the smallest label that does and
// sets dirty[u] for every neighbour u.
//
// The mode of a row. Every role reduces the same packed key by maximum,
//   key = cnt << 33 | own << 32 | (0xFFFFFFFF - label),
// own marking the vertex's current label: the most frequent label wins, then
// the vertex's own label among ties, then the smallest label. A row changes
// iff the winning key has own clear.
//   group  deg <= 16: four rows per wave in 16-lane groups. A lane holds one
//          neighbour's label; cnt of it comes from rotating the labels round
//          the group with shuffles (deg steps), the key maximum from an
//          xor-butterfly inside the group.
//   wave   17 <= deg <= 64: the same over all 64 lanes, one row per wave.
//   table  65 <= deg <= hub: one row per wave on the wave's quarter of the
//          workgroup's LDS table (u32 label slots, u32 counts), open
//          addressing with linear probing: an LDS atomicCAS claims the slot,
//          an atomicAdd counts. The row uses n slots, n a power of two >=
//          2 * deg, and n <= table / 4 because hub <= table / 8 (the entry
//          point insists). The scan for the key maximum clears the used
//          slots behind it.
//   hub    deg > hub: work items (vertex, p) for p < P = ceil(deg / (table /
//          2)), one workgroup each on the whole table. Item p counts only the
//          labels with mix(label) % P == p, so every label is counted
//          completely in exactly one item, and the item maxima combine by a
//          64-bit atomicMax into hubkey[row]. The item whose returning
//          increment of hubdone[row] sees P - 1 is the last: it takes the
//          combined key, zeroes both words for the next sweep and applies the
//          update. Nobody of the same class reads label[v], so this is safe
//          inside the launch. P depends on deg alone. mix spreads labels
//          evenly only in expectation: an item whose share does not fit
//          (a probe sequence longer than LPA_PROBES, or a full table) clears
//          the table and starts again with its share cut into S = 2, 4, ...
//          sub-passes by (mix(label) / P) % S, which keeps the answer exact
//          for any row with no global scratch.
//
// A launch takes classes [c0, c1) of vorder (cptr: class offsets) and the
// hub items [hptr[c0], hptr[c1]). Row blocks give every wave quads of four
// consecutive entries; the group rows of a quad run together, its wave and
// table rows one after the other. The plain launch treats [c0, c1) as one
// set (the engine passes one class; the check mode all of them, it writes no
// label). The fused launch is ONE workgroup looping over its classes with a
// fence and a barrier between them; it reads labels and dirty flags with
// agent-scope loads. Nothing waits for another workgroup.
//
// Check mode: the same counting body, every vertex with deg > 0 regardless
// of dirty, nothing written but `bad`, the number of rows that would change.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t LPA_HUB = 1024;        // default longest table-role row
constexpr uint32_t LPA_TABLE = 8192;      // default slots of the LDS table
constexpr uint32_t LPA_TABLE_MIN = 64, LPA_TABLE_MAX = 16384;
constexpr uint32_t LPA_FUSE = 1024;       // default vertices of a fused launch
constexpr uint32_t LPA_FUSE_MAX = 65536;
constexpr uint32_t LPA_GROUP = 16;        // lanes of a group-role row
constexpr uint32_t LPA_EMPTY = 0xFFFFFFFFu;  // a free slot; no label is -1
constexpr uint32_t LPA_PROBES = 256;      // hub role: longest probe sequence
constexpr int LPA_MAX_GRID = 1 << 16;     // blocks per role
constexpr int LPA_NW = BLOCK / WAVE;
enum { LM_EVAL = 0, LM_CHANGED = 1, LM_WORDS = 8 };
enum { LR_NONE = 0, LR_GROUP = 1, LR_WAVE = 2, LR_TABLE = 3 };

using LpArgs = lux_lpa_args;

// Labels and dirty flags cross waves inside the fused launch: agent-scope
// relaxed loads there (COH), plain loads elsewhere.
template <bool COH>
__device__ __forceinline__ uint32_t lpa_label_of(const LpArgs& a, V_ID u) {
  if (COH)
    return (uint32_t)__hip_atomic_load(&a.label[u], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return (uint32_t)a.label[u];
}
template <bool COH>
__device__ __forceinline__ uint32_t lpa_dirty_of(const LpArgs& a, V_ID v) {
  if (COH)
    return __hip_atomic_load(&a.dirty[v], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  return a.dirty[v];
}
__device__ __forceinline__ void lpa_set_label(const LpArgs& a, V_ID v,
                                              uint32_t l) {
  __hip_atomic_store(&a.label[v], (int)l, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Orders a wave's own LDS accesses.
__device__ __forceinline__ void lpa_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lpa_mix(uint32_t x) {  // murmur3 fmix32
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ unsigned long long lpa_key(uint32_t cnt,
                                                      uint32_t label,
                                                      uint32_t own) {
  return ((unsigned long long)cnt << 33) |
         ((unsigned long long)(label == own ? 1u : 0u) << 32) |
         (unsigned long long)(0xFFFFFFFFu - label);
}
__device__ __forceinline__ bool lpa_changes(unsigned long long key) {
  return key != 0 && !((key >> 32) & 1);
}
__device__ __forceinline__ uint32_t lpa_key_label(unsigned long long key) {
  return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu);
}

__device__ __forceinline__ unsigned long long lpa_shfl64(
    unsigned long long x, int src) {
  uint32_t lo = __shfl((uint32_t)x, src, WAVE);
  uint32_t hi = __shfl((uint32_t)(x >> 32), src, WAVE);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long lpa_shfl_xor64(
    unsigned long long x, int m) {
  uint32_t lo = __shfl_xor((uint32_t)x, m, WAVE);
  uint32_t hi = __shfl_xor((uint32_t)(x >> 32), m, WAVE);
  return ((unsigned long long)hi << 32) | lo;
}
// The maximum over the W lanes (a power of two) around each lane, in all.
template <int W>
__device__ __forceinline__ unsigned long long lpa_max_over(
    unsigned long long k) {
  for (int off = W / 2; off > 0; off >>= 1) {
    unsigned long long o = lpa_shfl_xor64(k, off);
    k = o > k ? o : k;
  }
  return k;
}

// Count label L in the open-addressing table (mask + 1 slots) from slot h
// on; false if `limit` probes find neither L nor a free slot.
__device__ __forceinline__ bool lpa_insert(uint32_t* keys, uint32_t* cnts,
                                           uint32_t mask, uint32_t L,
                                           uint32_t h, uint32_t limit) {
  h &= mask;
  for (uint32_t t = 0; t < limit; t++) {
    uint32_t prev = atomicCAS(&keys[h], LPA_EMPTY, L);
    if (prev == LPA_EMPTY || prev == L) {
      atomicAdd(&cnts[h], 1u);
      return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

// Group (W = 16) and wave (W = 64) role: the row of every W-lane group with
// `active` set, deg <= W; steps >= deg of every active group, the same in
// all lanes of the wave, which must call this together. Returns whether the
// group's row changes, in each of its lanes.
template <int W, bool COH, bool CHECK>
__device__ __forceinline__ bool lpa_rotate(const LpArgs& a, bool active,
                                           V_ID v, E_ID b, uint32_t deg,
                                           uint32_t steps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t sub = lane & (W - 1);
  const int gbase = lane - (int)sub;
  bool have = active && sub < deg;
  V_ID u = have ? a.aadj[b + sub] : a.nv;
  if (u >= a.nv) have = false;
  const uint32_t L = have ? lpa_label_of<COH>(a, u) : LPA_EMPTY;
  const uint32_t own = active ? lpa_label_of<COH>(a, v) : 0;
  uint32_t cnt = 0;
  for (uint32_t s = 0; s < steps; s++) {
    uint32_t idx = sub + s;  // sub, s < deg: one turn round the row
    if (idx >= deg) idx -= deg;
    uint32_t o = __shfl(L, gbase + (int)(idx & (W - 1)), WAVE);
    cnt += (have && s < deg && o == L) ? 1u : 0u;
  }
  unsigned long long key = have ? lpa_key(cnt, L, own) : 0ull;
  key = lpa_max_over<W>(key);
  const bool changed = active && lpa_changes(key);
  if (!CHECK && changed) {
    if (sub == 0) lpa_set_label(a, v, lpa_key_label(key));
    if (have) a.dirty[u] = 1u;
  }
  return changed;
}

// Table role: row v (65 <= deg <= hub) by one wave on its nslots slots of
// LDS, all free at entry and at exit.
template <bool COH, bool CHECK>
__device__ __forceinline__ bool lpa_table_row(const LpArgs& a, V_ID v,
                                              E_ID b, uint32_t deg,
                                              uint32_t* keys, uint32_t* cnts,
                                              uint32_t nslots) {
  const int lane = threadIdx.x & (WAVE - 1);
  uint32_t n = 2 * WAVE;
  while (n < 2 * deg && n < nslots) n <<= 1;
  if (n < 2 * deg) return false;  // the entry point keeps hub <= table / 8
  const uint32_t own = lpa_label_of<COH>(a, v);
  for (uint32_t j = lane; j < deg; j += WAVE) {
    V_ID u = a.aadj[b + j];
    if (u >= a.nv) continue;
    uint32_t L = lpa_label_of<COH>(a, u);
    lpa_insert(keys, cnts, n - 1, L, lpa_mix(L), n);
  }
  lpa_wave_sync();
  unsigned long long key = 0;
  for (uint32_t s = lane; s < n; s += WAVE) {
    uint32_t k = keys[s];
    if (k == LPA_EMPTY) continue;
    unsigned long long mine = lpa_key(cnts[s], k, own);
    key = mine > key ? mine : key;
    keys[s] = LPA_EMPTY;
    cnts[s] = 0;
  }
  lpa_wave_sync();
  key = lpa_max_over<WAVE>(key);
  const bool changed = lpa_changes(key);
  if (!CHECK && changed) {
    if (lane == 0) lpa_set_label(a, v, lpa_key_label(key));
    for (uint32_t j = lane; j < deg; j += WAVE) {
      V_ID u = a.aadj[b + j];
      if (u < a.nv) a.dirty[u] = 1u;
    }
  }
  return changed;
}

// The entries [lo, hi) of vorder by the waves of the row blocks; ev / ch:
// this lane's counts of evaluated and changed rows (one lane per row).
template <bool COH, bool CHECK>
__device__ __forceinline__ void lpa_rows(const LpArgs& a, uint32_t lo,
                                         uint32_t hi, uint32_t row_blocks,
                                         uint32_t* keys, uint32_t* cnts,
                                         uint32_t nslots, uint32_t& ev,
                                         uint32_t& ch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int g = lane / (int)LPA_GROUP;
  const uint32_t sub = lane & (LPA_GROUP - 1);
  constexpr uint32_t QUAD = WAVE / LPA_GROUP;
  const uint64_t step = (uint64_t)row_blocks * LPA_NW * QUAD;
  for (uint64_t q = lo + ((uint64_t)blockIdx.x * LPA_NW + wid) * QUAD; q < hi;
       q += step) {
    const uint64_t i = q + g;
    V_ID v = i < hi ? a.vorder[i] : a.nv;
    uint32_t role = LR_NONE, deg = 0;
    E_ID b = 0;
    if (v < a.nv) {
      b = a.aptr[v];
      uint64_t d = a.aptr[v + 1] - b;
      if (d > 0 && d <= a.hub && (CHECK || lpa_dirty_of<COH>(a, v))) {
        deg = (uint32_t)d;
        role = deg <= LPA_GROUP ? LR_GROUP : deg <= WAVE ? LR_WAVE : LR_TABLE;
      }
    }
    if (role != LR_NONE && sub == 0) {
      ev++;
      if (!CHECK) a.dirty[v] = 0u;
    }
    uint32_t steps = role == LR_GROUP ? deg : 0u;
    for (int off = LPA_GROUP; off < WAVE; off <<= 1) {
      uint32_t o = __shfl_xor(steps, off, WAVE);
      steps = o > steps ? o : steps;
    }
    if (steps) {
      bool c = lpa_rotate<LPA_GROUP, COH, CHECK>(a, role == LR_GROUP, v, b,
                                                 deg, steps);
      if (c && sub == 0) ch++;
    }
    for (int g2 = 0; g2 < (int)QUAD; g2++) {
      const int src = g2 * (int)LPA_GROUP;
      uint32_t r = __shfl(role, src, WAVE);
      if (r != LR_WAVE && r != LR_TABLE) continue;  // uniform over the wave
      V_ID vv = __shfl(v, src, WAVE);
      uint32_t dd = __shfl(deg, src, WAVE);
      E_ID bb = lpa_shfl64(b, src);
      bool c = r == LR_WAVE
                   ? lpa_rotate<WAVE, COH, CHECK>(a, true, vv, bb, dd, dd)
                   : lpa_table_row<COH, CHECK>(a, vv, bb, dd, keys, cnts,
                                               nslots);
      if (c && lane == 0) ch++;
    }
  }
}

// Hub role: item (v, p) of hub row `row` by the whole workgroup on the whole
// table, all free at entry and at exit. All threads call this together.
template <bool CHECK>
__device__ __forceinline__ void lpa_hub_item(const LpArgs& a, V_ID v,
                                             uint32_t p, uint32_t row,
                                             uint32_t* keys, uint32_t* cnts,
                                             uint32_t& ev, uint32_t& ch) {
  __shared__ uint32_t s_flag;  // go, then overflow, then last
  __shared__ unsigned long long s_red[LPA_NW];
  __shared__ unsigned long long s_key;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const E_ID b = a.aptr[v];
  const uint64_t deg = a.aptr[v + 1] - b;
  const uint32_t half = a.table / 2;
  const uint32_t P = (uint32_t)((deg + half - 1) / half);
  if (threadIdx.x == 0)
    s_flag = (p < P && row < a.nhub && deg > a.hub &&
              (CHECK || a.dirty[v])) ? 1u : 0u;
  __syncthreads();
  const bool go = s_flag != 0;
  __syncthreads();
  if (!go) return;
  const uint32_t own = lpa_label_of<false>(a, v);
  const uint32_t mask = a.table - 1;
  const uint32_t limit = a.table < LPA_PROBES ? a.table : LPA_PROBES;
  unsigned long long key = 0;
  for (uint32_t S = 1; S != 0; S <<= 1) {
    key = 0;
    bool over = false;
    for (uint32_t s = 0; s < S && !over; s++) {
      if (threadIdx.x == 0) s_flag = 0;
      __syncthreads();
      for (uint64_t j = threadIdx.x; j < deg; j += BLOCK) {
        V_ID u = a.aadj[b + j];
        if (u >= a.nv) continue;
        uint32_t L = lpa_label_of<false>(a, u);
        uint32_t hh = lpa_mix(L);
        if (hh % P != p || (hh / P) % S != s) continue;
        if (!lpa_insert(keys, cnts, mask, L, lpa_mix(hh ^ 0x9E3779B9u),
                        limit))
          s_flag = 1;
      }
      __syncthreads();
      over = s_flag != 0;
      for (uint32_t t = threadIdx.x; t <= mask; t += BLOCK) {
        uint32_t k = keys[t];
        if (k == LPA_EMPTY) continue;
        unsigned long long mine = lpa_key(cnts[t], k, own);
        if (!over && mine > key) key = mine;
        keys[t] = LPA_EMPTY;
        cnts[t] = 0;
      }
      __syncthreads();
    }
    if (!over) break;
  }
  key = lpa_max_over<WAVE>(key);
  if (lane == 0) s_red[wid] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < LPA_NW; w++) key = s_red[w] > key ? s_red[w] : key;
    atomicMax(&a.hubkey[row], key);
    __threadfence();
    uint32_t last = atomicAdd(&a.hubdone[row], 1u) + 1 == P ? 1u : 0u;
    if (last) {
      __threadfence();
      s_key = atomicExch(&a.hubkey[row], 0ull);
      atomicExch(&a.hubdone[row], 0u);
    }
    s_flag = last;
  }
  __syncthreads();
  const bool last = s_flag != 0;
  key = s_key;
  __syncthreads();
  if (!last) return;
  const bool changed = lpa_changes(key);
  if (threadIdx.x == 0) {
    ev++;
    if (changed) ch++;
    if (!CHECK) a.dirty[v] = 0u;
    if (!CHECK && changed) lpa_set_label(a, v, lpa_key_label(key));
  }
  if (!CHECK && changed) {
    for (uint64_t j = threadIdx.x; j < deg; j += BLOCK) {
      V_ID u = a.aadj[b + j];
      if (u < a.nv) a.dirty[u] = 1u;
    }
  }
}

// Classes [c0, c1): blocks below row_blocks take the rows, the others the
// hub items. FUSED: one workgroup, class after class; otherwise the classes
// are one set. slots: the LDS table of this launch, a.table, or
// LPA_TABLE_MIN for a launch without table-role rows and hub items (more
// workgroups fit a CU then).
template <bool FUSED, bool CHECK>
__global__ void __launch_bounds__(BLOCK) lpa_class_kernel(
    LpArgs a, uint32_t c0, uint32_t c1, uint32_t row_blocks,
    uint32_t slots) {
  extern __shared__ uint32_t lpa_lds[];
  uint32_t* keys = lpa_lds;
  uint32_t* cnts = lpa_lds + slots;
  for (uint32_t t = threadIdx.x; t < slots; t += BLOCK) {
    keys[t] = LPA_EMPTY;
    cnts[t] = 0;
  }
  __syncthreads();
  const int wid = threadIdx.x >> 6;
  const uint32_t nslots = slots / LPA_NW;
  uint32_t ev = 0, ch = 0;
  if (blockIdx.x < row_blocks) {
    uint32_t* wk = keys + wid * nslots;
    uint32_t* wc = cnts + wid * nslots;
    if (FUSED) {
      for (uint32_t c = c0; c < c1; c++) {
        uint32_t lo = a.cptr[c], hi = a.cptr[c + 1];
        if (hi > a.nv) hi = a.nv;
        lpa_rows<true, CHECK>(a, lo, hi, row_blocks, wk, wc, nslots, ev, ch);
        __threadfence();  // this class's labels and flags are out
        __syncthreads();
      }
    } else {
      uint32_t lo = a.cptr[c0], hi = a.cptr[c1];
      if (hi > a.nv) hi = a.nv;
      lpa_rows<false, CHECK>(a, lo, hi, row_blocks, wk, wc, nslots, ev, ch);
    }
  } else {
    const uint32_t nb = gridDim.x - row_blocks;
    uint32_t end = a.hptr[c1];
    if (end > a.nitems) end = a.nitems;
    for (uint64_t i = (uint64_t)a.hptr[c0] + (blockIdx.x - row_blocks);
         i < end; i += nb) {
      V_ID v = a.hubv[i];
      if (v >= a.nv) continue;  // uniform over the workgroup
      lpa_hub_item<CHECK>(a, v, a.hubp[i], a.hubr[i], keys, cnts, ev, ch);
    }
  }
  ev = wave_reduce_sum(ev);
  ch = wave_reduce_sum(ch);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (CHECK) {
      if (ch) atomicAdd(a.bad, (unsigned long long)ch);
    } else {
      if (ev) atomicAdd(&a.meta[LM_EVAL], ev);
      if (ch) atomicAdd(&a.meta[LM_CHANGED], ch);
    }
  }
}

// sizes[l] += 1 and tot[l] += deg for l = label[v]; intra += the neighbours
// u > v of v with v's label. A 16-lane group per vertex.
__global__ void __launch_bounds__(BLOCK) lpa_stats_kernel(
    V_ID nv, const E_ID* aptr, const V_ID* aadj, const int* label,
    unsigned long long* sizes, unsigned long long* tot,
    unsigned long long* intra) {
  const uint32_t sub = threadIdx.x & (LPA_GROUP - 1);
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x / LPA_GROUP;
  unsigned long long mine = 0;
  for (uint64_t v = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) /
                    LPA_GROUP;
       v < nv; v += stride) {
    const E_ID b = aptr[v];
    const uint64_t deg = aptr[v + 1] - b;
    const uint32_t l = (uint32_t)label[v];
    if (l >= nv) continue;
    if (sub == 0) {
      atomicAdd(&sizes[l], 1ull);
      if (deg) atomicAdd(&tot[l], (unsigned long long)deg);
    }
    for (uint64_t j = sub; j < deg; j += LPA_GROUP) {
      V_ID u = aadj[b + j];
      if (u < nv && u > v && (uint32_t)label[u] == l) mine++;
    }
  }
  mine = wave_reduce_sum(mine);
  if ((threadIdx.x & (WAVE - 1)) == 0 && mine) atomicAdd(intra, mine);
}

// The longest row the table role takes: a wave's quarter of the table holds
// 2 * deg slots; never below the wave role's 64.
__host__ __forceinline__ uint32_t lpa_row_limit(uint32_t hub,
                                                uint32_t table) {
  uint32_t t = hub < table / 8 ? hub : table / 8;
  return t < (uint32_t)WAVE ? (uint32_t)WAVE : t;
}

__host__ __forceinline__ bool lpa_args_ok(const lux_lpa_args* a) {
  const uint32_t t = a->table;
  return t >= LPA_TABLE_MIN && t <= LPA_TABLE_MAX && !(t & (t - 1)) &&
         a->hub >= (uint32_t)WAVE &&
         (a->hub == (uint32_t)WAVE || a->hub <= t / 8);
}

template <bool FUSED, bool CHECK>
__host__ int lpa_launch(hipStream_t s, const lux_lpa_args& a, uint32_t c0,
                        uint32_t c1, uint32_t grid, uint32_t row_blocks,
                        uint32_t maxdeg) {
  const bool bare = maxdeg <= (uint32_t)WAVE && grid == row_blocks;
  const uint32_t slots = bare ? LPA_TABLE_MIN : a.table;
  auto kern = lpa_class_kernel<FUSED, CHECK>;
  static const hipError_t raised = hipFuncSetAttribute(
      (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)(LPA_TABLE_MAX * 2 * sizeof(uint32_t)));
  if (raised != hipSuccess) return -2;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(BLOCK),
                     slots * 2 * sizeof(uint32_t), s, a, c0, c1, row_blocks,
                     slots);
  return 0;
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_lpa_hub_default() { return LPA_HUB; }
uint32_t lux_gpu_lpa_table_default() { return LPA_TABLE; }
uint32_t lux_gpu_lpa_table_min() { return LPA_TABLE_MIN; }
uint32_t lux_gpu_lpa_table_max() { return LPA_TABLE_MAX; }
uint32_t lux_gpu_lpa_fuse_default() { return LPA_FUSE; }
uint32_t lux_gpu_lpa_fuse_max() { return LPA_FUSE_MAX; }
uint32_t lux_gpu_lpa_meta_words() { return LM_WORDS; }
uint32_t lux_gpu_lpa_row_limit(uint32_t hub, uint32_t table) {
  return lpa_row_limit(hub, table);
}

// Classes [c0, c1) holding nrows entries of vorder, the longest of degree
// maxdeg, and nitems hub items.
// fused: one workgroup runs them class after class (no hub item allowed);
// otherwise they are evaluated as one set, which is the definition only for
// c1 == c0 + 1. Returns -1 (and launches nothing) on bad arguments, -2 if
// the LDS limit cannot be raised.
int lux_gpu_lpa_classes(uint64_t stream, const lux_lpa_args* a, uint32_t c0,
                        uint32_t c1, uint32_t nrows, uint32_t nitems,
                        uint32_t maxdeg, int fused) {
  if (!lpa_args_ok(a) || c0 >= c1 || c1 > a->ncls || nrows > a->nv ||
      nitems > a->nitems || (fused && (nitems || nrows > LPA_FUSE_MAX)) ||
      (!fused && c1 != c0 + 1))
    return -1;
  if (!nrows && !nitems) return 0;
  int rc;
  if (fused) {
    rc = lpa_launch<true, false>((hipStream_t)stream, *a, c0, c1, 1, 1,
                                 maxdeg);
  } else {
    uint32_t rb = ceil_div_u32(nrows, WAVE / LPA_GROUP * LPA_NW);
    if (rb > (uint32_t)LPA_MAX_GRID) rb = LPA_MAX_GRID;
    uint32_t hb = nitems > (uint32_t)LPA_MAX_GRID ? LPA_MAX_GRID : nitems;
    rc = lpa_launch<false, false>((hipStream_t)stream, *a, c0, c1, rb + hb,
                                  rb, maxdeg);
  }
  LUX_POST_LAUNCH(stream);
  return rc;
}

// a->bad (one u64, added to): the vertices with deg > 0 whose own label
// does not reach the maximum count.
int lux_gpu_lpa_check(uint64_t stream, const lux_lpa_args* a) {
  if (!lpa_args_ok(a) || !a->bad) return -1;
  if (!a->nv || !a->ncls) return 0;
  uint32_t rb = ceil_div_u32(a->nv, WAVE / LPA_GROUP * LPA_NW);
  if (rb > (uint32_t)LPA_MAX_GRID) rb = LPA_MAX_GRID;
  uint32_t hb = a->nitems > (uint32_t)LPA_MAX_GRID ? LPA_MAX_GRID : a->nitems;
  int rc = lpa_launch<false, true>((hipStream_t)stream, *a, 0, a->ncls,
                                   rb + hb, rb, 0xFFFFFFFFu);
  LUX_POST_LAUNCH(stream);
  return rc;
}

// sizes, tot: u64[nv], intra: one u64; all zeroed by the caller, added to.
void lux_gpu_lpa_stats(uint64_t stream, lux::V_ID nv, const lux::E_ID* aptr,
                       const lux::V_ID* aadj, const int* label,
                       unsigned long long* sizes, unsigned long long* tot,
                       unsigned long long* intra) {
  if (!nv) return;
  hipLaunchKernelGGL(lpa_stats_kernel,
                     dim3(grid_for((uint64_t)nv * LPA_GROUP)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, aptr, aadj, label, sizes, tot,
                     intra);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
