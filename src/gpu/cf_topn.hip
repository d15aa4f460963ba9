// CF top-N recommendation on one GPU: for every query vertex the n best
// admissible candidates of an id range by the fp32 dot product of their factor
// rows, scoring (MFMA) and selection fused so that no score is ever written
// to memory. No reference equivalent; the definition is in API.md.
//
// Strict total order of a query's candidates: (s_i, i) precedes (s_j, j) iff
// s_i > s_j, or s_i == s_j and i < j. The result is the first n admissible
// candidates in that order, a fixed tensor whatever the work split.
//
// cf_topn_kernel<KP>, KP = 32 / 64 / 128 (K padded with zeros): a 256-thread
// workgroup owns 64 consecutive query positions (blockIdx.x) and one split
// of whole 64-item tiles of the candidate range (blockIdx.y); wave w owns
// queries 16w .. 16w + 15.
//   operands  v_mfma_f32_16x16x4_f32 with ITEMS as A and QUERIES as B. Lane
//             l = 16 g + m gives B[k = g][n = m], so the wave's query panel
//             is bq[t] = vec[query m][4 t + g], KP / 4 VGPRs loaded once and
//             held for the life of the workgroup. A[i = m][k = g] of item
//             block b comes from the LDS tile; the accumulator of a block
//             then holds, in lane l, the scores of items 4 g + r (r = 0..3)
//             of query m: a query's 16 scores of a block sit in 4 lanes x 4
//             registers (the D layout cf_als.hip's fragments use).
//   tiles     64 items x KP fp32, row pitch KP + 2 floats. A fragment read
//             is one ds_read_b32 per lane at word (16 b + m)(KP + 2) + 4 t
//             + g; KP is a multiple of 32, so a 32-lane group (m = 0..15,
//             g in {g0, g0 + 1}) reads banks 2 m + g + const mod 32: all 32
//             distinct. The pitch is even, so the staging stores are 8-byte
//             aligned: every thread moves KP / 16 16-byte pieces of the tile
//             (coalesced along the rows) as two ds_write_b64 each, and the
//             lanes of a row write consecutive 8-byte words. Tile t + 1's
//             global loads are issued into registers before tile t's MFMAs
//             and land under them (als_gram_range's prefetch under the
//             burst); the registers are the second buffer, one LDS tile
//             suffices. Rows past the split's end and columns past K are
//             zero-filled and such rows are never candidates.
//   select    every lane keeps its query's current n-th best entry as a
//             threshold in two registers. A score that does not precede it
//             costs one compare. The 16-lane groups g = 0..3 take turns (so
//             the four lanes of a query never touch its list at once, no
//             atomics). A passer is first searched in the query's ascending
//             exclusion row in global memory (branch-free lower bound, all
//             lanes at once, before the turns) and, if admissible, inserted
//             in its lane's turn into the query's sorted list in LDS; after
//             a turn every lane reloads its threshold.
//   output    list entries that were never filled are written as -1 / -inf.
//             With one split the lists are the result, otherwise they go to
//             part[s][q][n] and cf_topn_merge_kernel (a wave per query)
//             places every partial entry at its rank: the number of entries
//             of all S sorted partial lists that precede it, counted in LDS.
//
// A query id >= nv (the host checks ids it can see; a device tensor is not
// read back) loads nothing and yields an all-padding row.
//
// cf_topn_plain_kernel is the check: a wave per query position, a serial
// fmaf per candidate, no tiles, MFMA or lists. cf_topn_keys_kernel emits the
// (row << 32) | col keys of a range of CSC entries for the "seen" CSR.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr int TOPN_QB = 64;     // query positions per workgroup
constexpr int TOPN_TILE = 64;   // items per tile
constexpr int TOPN_NMAX = 64;   // longest list
constexpr int TOPN_LPITCH = TOPN_NMAX + 1;  // list row pitch in entries
constexpr int TOPN_MERGE_MAX = 2048;        // partial entries per query
constexpr uint32_t TOPN_NONE = 0x7fffffffu; // item of an unfilled entry
constexpr uint32_t TOPN_NINF = 0xff800000u; // -inf

typedef float topn_f32x4 __attribute__((ext_vector_type(4)));

// (s, i) precedes (t, j) in the strict total order.
__device__ __forceinline__ bool topn_before(float s, uint32_t i, float t,
                                            uint32_t j) {
  return s > t || (s == t && i < j);
}

// acc[j] without dynamic register indexing (which would go to scratch).
__device__ __forceinline__ float topn_pick(const topn_f32x4 acc[4], int j) {
  float s = acc[0][0];
#pragma unroll
  for (int b = 0; b < 4; b++)
#pragma unroll
    for (int r = 0; r < 4; r++) s = j == 4 * b + r ? acc[b][r] : s;
  return s;
}

// Is `item` in the ascending row adj[lo, lo + len)? Branch-free lower bound:
// adj[base] is the last entry <= item if there is one.
__device__ __forceinline__ bool topn_excluded(const uint32_t* adj,
                                              uint64_t lo, uint32_t len,
                                              uint32_t item) {
  if (!len) return false;
  uint64_t base = lo;
  while (len > 1) {
    const uint32_t half = len >> 1;
    base += adj[base + half] <= item ? half : 0;
    len -= half;
  }
  return adj[base] == item;
}

// The exclusion row of vertex u, clamped to the array.
__device__ __forceinline__ void topn_row(const lux_cf_topn_args& a, uint32_t u,
                                         uint64_t* lo, uint32_t* len) {
  uint64_t b = (uint64_t)a.excl_ptr[u], e = (uint64_t)a.excl_ptr[u + 1];
  e = e < a.n_excl ? e : a.n_excl;
  b = b < e ? b : e;
  *lo = b;
  const uint64_t l = e - b;
  *len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
}

template <int KP>
struct TopnLds {
  float S[TOPN_TILE * (KP + 2)];
  uint2 L[TOPN_QB * TOPN_LPITCH];  // {score bits, item}, best first
};

// The pieces of tile [c0, c0 + 64) this thread stages: piece c = tid + 256 j
// is columns [4 (c % (KP / 4)), + 4) of row c / (KP / 4).
template <int KP>
__device__ __forceinline__ void topn_tile_loads(const lux_cf_topn_args& a,
                                                uint32_t c0, uint32_t c_end,
                                                int tid, bool vec4,
                                                float4 st[KP / 16]) {
  constexpr int CPR = KP / 4;
#pragma unroll
  for (int j = 0; j < KP / 16; j++) {
    const int c = tid + BLOCK * j;
    const uint32_t item = c0 + (uint32_t)(c / CPR);
    const uint32_t k = 4u * (uint32_t)(c % CPR);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (item < c_end && k < a.K) {
      const float* p = a.vec + (uint64_t)item * a.K + k;
      if (vec4) {  // K % 4 == 0 and a 16-byte aligned base
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v.x = p[0];
        if (k + 1 < a.K) v.y = p[1];
        if (k + 2 < a.K) v.z = p[2];
        if (k + 3 < a.K) v.w = p[3];
      }
    }
    st[j] = v;
  }
}

template <int KP>
__global__ void __launch_bounds__(BLOCK)
cf_topn_kernel(lux_cf_topn_args a, int* __restrict__ dst_items,
               float* __restrict__ dst_scores, bool vec4) {
  constexpr int P = KP + 2, CPR = KP / 4, NT = KP / 4;
  __shared__ TopnLds<KP> lds;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid >> 6;
  const int m = lane & 15, g = lane >> 4;
  const uint32_t n = a.n;
  const int ql = 16 * wid + m;  // this lane's query, local
  const uint64_t qpos = (uint64_t)blockIdx.x * TOPN_QB + ql;
  uint2* const list = &lds.L[ql * TOPN_LPITCH];

  // the split's candidates [c0, c_end), whole tiles
  const uint64_t t0 = (uint64_t)blockIdx.y * a.tiles_per_split;
  const uint64_t first = a.c_lo + t0 * TOPN_TILE;
  const uint64_t last = first + (uint64_t)a.tiles_per_split * TOPN_TILE;
  const uint32_t c_end = last < a.c_hi ? (uint32_t)last : a.c_hi;
  uint32_t c0 = first < c_end ? (uint32_t)first : c_end;

  // the query panel, the exclusion row, the empty list
  uint32_t u = qpos < a.q ? a.queries[qpos] : a.nv;
  const bool live = u < a.nv;
  float bq[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const uint32_t k = 4u * t + g;
    bq[t] = live && k < a.K ? a.vec[(uint64_t)u * a.K + k] : 0.0f;
  }
  uint64_t e_lo = 0;
  uint32_t e_len = 0;
  if (live) topn_row(a, u, &e_lo, &e_len);
  for (uint32_t p = g; p < n; p += 4)
    list[p] = make_uint2(TOPN_NINF, TOPN_NONE);
  float ts = __uint_as_float(TOPN_NINF);  // the threshold: entry n - 1
  uint32_t ti = TOPN_NONE;
  __syncthreads();

  float4 st[KP / 16];
  if (c0 < c_end) topn_tile_loads<KP>(a, c0, c_end, tid, vec4, st);
  for (; c0 < c_end; c0 += TOPN_TILE) {
    // stage the prefetched tile
#pragma unroll
    for (int j = 0; j < KP / 16; j++) {
      const int c = tid + BLOCK * j;
      float* row = &lds.S[(c / CPR) * P + 4 * (c % CPR)];
      *reinterpret_cast<float2*>(row) = make_float2(st[j].x, st[j].y);
      *reinterpret_cast<float2*>(row + 2) = make_float2(st[j].z, st[j].w);
    }
    __syncthreads();
    // the next tile's loads land under the MFMAs; c_end - c0 > 64 is
    // workgroup-uniform
    if (c_end - c0 > TOPN_TILE)
      topn_tile_loads<KP>(a, c0 + TOPN_TILE, c_end, tid, vec4, st);
    topn_f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; b++) acc[b] = topn_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* frag = &lds.S[m * P + g];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      if (4u * t >= a.K) break;  // the remaining columns are zero
      float f[4];
#pragma unroll
      for (int b = 0; b < 4; b++) f[b] = frag[16 * b * P + 4 * t];
#pragma unroll
      for (int b = 0; b < 4; b++)
        acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[b], bq[t], acc[b], 0,
                                                      0, 0);
    }
    // selection: bit 4 b + r = item c0 + 16 b + 4 g + r may precede the
    // threshold (s >= ts is necessary) and is a candidate
    uint32_t mask = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t item = c0 + 16 * b + 4 * g + r;
        mask |= (acc[b][r] >= ts && item < c_end) ? 1u << (4 * b + r) : 0u;
      }
    if (!live) mask = 0;
    if (__any(mask != 0)) {
      // the exclusion searches of all four lanes of a query run at once;
      // only the list is taken in turns
      for (uint32_t rest = mask; rest; rest &= rest - 1) {
        const int j = __ffs(rest) - 1;
        const uint32_t item = c0 + 16 * (j >> 2) + 4 * g + (j & 3);
        if (!topn_before(topn_pick(acc, j), item, ts, ti) ||
            topn_excluded(a.excl_adj, e_lo, e_len, item))
          mask &= ~(1u << j);
      }
      for (int turn = 0; turn < 4; turn++) {
        if (g == turn) {
          while (mask) {
            const int j = __ffs(mask) - 1;
            mask &= mask - 1;
            const float s = topn_pick(acc, j);
            const uint32_t item = c0 + 16 * (j >> 2) + 4 * g + (j & 3);
            if (!topn_before(s, item, ts, ti)) continue;
            uint32_t p = n - 1;  // entry n - 1 falls off the end
            while (p > 0) {
              const uint2 o = list[p - 1];
              if (!topn_before(s, item, __uint_as_float(o.x), o.y)) break;
              list[p] = o;
              p--;
            }
            list[p] = make_uint2(__float_as_uint(s), item);
            const uint2 th = list[n - 1];
            ts = __uint_as_float(th.x);
            ti = th.y;
          }
        }
        // the other lanes of the query see the turn's list
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint2 th = list[n - 1];
        ts = __uint_as_float(th.x);
        ti = th.y;
      }
    }
    __syncthreads();  // tile consumed before the next stage overwrites
  }

  // lists -> dst[split][qpos][n]
  if (qpos < a.q) {
    const uint64_t o = ((uint64_t)blockIdx.y * a.q + qpos) * n;
    for (uint32_t p = g; p < n; p += 4) {
      const uint2 e = list[p];
      dst_items[o + p] = e.y == TOPN_NONE ? -1 : (int)e.y;
      dst_scores[o + p] = __uint_as_float(e.y == TOPN_NONE ? TOPN_NINF : e.x);
    }
  }
}

// A wave (one 64-thread workgroup) per query position: the S * n <=
// TOPN_MERGE_MAX partial entries are staged in LDS and every filled entry
// goes to its rank, the number of entries that precede it. The lists are
// sorted, so the count walks each list only up to its first entry that does
// not precede, and stops at n.
__global__ void __launch_bounds__(WAVE)
cf_topn_merge_kernel(lux_cf_topn_args a) {
  __shared__ uint2 E[TOPN_MERGE_MAX];  // {score bits, item}, item < 0 unfilled
  const int lane = threadIdx.x;
  const uint64_t qpos = blockIdx.x;
  const uint32_t n = a.n, S = a.splits, total = S * n;
  const uint64_t stride = (uint64_t)a.q * n;  // between the splits
  for (uint32_t e = lane; e < total; e += WAVE) {
    const uint64_t at = (uint64_t)(e / n) * stride + qpos * n + e % n;
    E[e] = make_uint2(__float_as_uint(a.part_scores[at]),
                      (uint32_t)a.part_items[at]);
  }
  __syncthreads();
  uint32_t filled = 0;
  for (uint32_t e = lane; e < total; e += WAVE) {
    const uint2 me = E[e];
    if ((int)me.y < 0) continue;
    filled++;
    const float s = __uint_as_float(me.x);
    uint32_t rank = 0;
    for (uint32_t t = 0; t < S && rank < n; t++)
      for (uint32_t p = 0; p < n; p++) {
        const uint2 o = E[t * n + p];
        if ((int)o.y < 0 || !topn_before(__uint_as_float(o.x), o.y, s, me.y))
          break;
        rank++;
      }
    if (rank < n) {
      a.out_items[qpos * n + rank] = (int)me.y;
      a.out_scores[qpos * n + rank] = s;
    }
  }
  for (int off = 1; off < WAVE; off <<= 1)
    filled += __shfl_xor(filled, off, WAVE);
  for (uint32_t p = filled + lane; p < n; p += WAVE) {
    a.out_items[qpos * n + p] = -1;
    a.out_scores[qpos * n + p] = __uint_as_float(TOPN_NINF);
  }
}

// The check. A wave per query position: lane j examines returned entry j,
// then the lanes stride over all candidates.
__global__ void __launch_bounds__(BLOCK)
cf_topn_plain_kernel(lux_cf_topn_args a, const int* __restrict__ items,
                     const float* __restrict__ scores, uint32_t* bad_out) {
  __shared__ int ret[BLOCK / WAVE][TOPN_NMAX];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  const uint64_t qpos = (uint64_t)blockIdx.x * (BLOCK / WAVE) + wid;
  if (qpos >= a.q) return;  // wave-uniform; no workgroup barrier below
  const uint32_t n = a.n, K = a.K;
  const uint32_t u = a.queries[qpos];
  uint32_t bad = 0;
  const bool have = (uint32_t)lane < n;
  const int item = have ? items[qpos * n + lane] : -1;
  const float score = have ? scores[qpos * n + lane]
                           : __uint_as_float(TOPN_NINF);
  ret[wid][lane] = item;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int* mine = ret[wid];
  if (u >= a.nv) {  // an id the engine could not see: the row must be empty
    bad = have && item != -1;
    bad = wave_reduce_sum(bad);
    if (lane == 0) bad_out[qpos] = bad;
    return;
  }
  const float* uv = a.vec + (uint64_t)u * K;
  uint64_t e_lo;
  uint32_t e_len;
  topn_row(a, u, &e_lo, &e_len);
  const float eps = 2.0f * (float)K * 0x1p-24f;

  // the returned entries
  const uint32_t cnt = (uint32_t)__popcll(__ballot(item >= 0));
  const int nxt_item = __shfl_down(item, 1, WAVE);
  const float nxt_score = __shfl_down(score, 1, WAVE);
  float tol = 0.0f;
  if (have && item < 0)
    bad += (uint32_t)lane < cnt || item != -1 ||
           __float_as_uint(score) != TOPN_NINF;  // padding comes last
  if (have && item >= 0) {
    const uint32_t i = (uint32_t)item;
    if (i < a.c_lo || i >= a.c_hi) {
      bad++;
    } else {
      const float* iv = a.vec + (uint64_t)i * K;
      float dot = 0.0f, absdot = 0.0f;
      for (uint32_t k = 0; k < K; k++) {
        dot = fmaf(uv[k], iv[k], dot);
        absdot += fabsf(uv[k] * iv[k]);
      }
      tol = eps * absdot;
      bad += !(fabsf(score - dot) <= tol);
      bad += topn_excluded(a.excl_adj, e_lo, e_len, i);
      for (int j = 0; j < lane; j++) bad += mine[j] == item;
      if ((uint32_t)lane + 1 < n && nxt_item >= 0)
        bad += !topn_before(score, i, nxt_score, (uint32_t)nxt_item);
    }
  }
  // the last returned entry bounds what may be left out; with a short list
  // nothing admissible may be
  const bool full = cnt == n;
  const float last = __shfl(score, (int)n - 1, WAVE);
  const float last_tol = __shfl(tol, (int)n - 1, WAVE);
  for (uint64_t c = (uint64_t)a.c_lo + lane; c < a.c_hi; c += WAVE) {
    const uint32_t i = (uint32_t)c;
    const float* iv = a.vec + (uint64_t)i * K;
    float dot = 0.0f, absdot = 0.0f;
    for (uint32_t k = 0; k < K; k++) {
      dot = fmaf(uv[k], iv[k], dot);
      absdot += fabsf(uv[k] * iv[k]);
    }
    if (full && !(dot > last + (eps * absdot + last_tol))) continue;
    if (topn_excluded(a.excl_adj, e_lo, e_len, i)) continue;
    bool returned = false;
    for (uint32_t j = 0; j < n; j++) returned |= mine[j] == (int)i;
    bad += !returned;
  }
  bad = wave_reduce_sum(bad);
  if (lane == 0) bad_out[qpos] = bad;
}

// One lane per CSC entry e of [e0, e1): out[e - e0] = (row << 32) | col.
__global__ void __launch_bounds__(BLOCK)
cf_topn_keys_kernel(V_ID nrows, const E_ID* __restrict__ row_ptr,
                    const V_ID* __restrict__ col, E_ID e0, E_ID e1,
                    unsigned long long* __restrict__ out) {
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = e0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < e1;
       e += stride) {
    // the last row with row_ptr[r] <= e, branch-free: the answer is in
    // [r, r + len) throughout
    V_ID r = 0;
    for (V_ID len = nrows; len > 1;) {
      const V_ID half = len >> 1;
      r += row_ptr[r + half] <= e ? half : 0;
      len -= half;
    }
    out[e - e0] = ((unsigned long long)r << 32) | col[e];
  }
}

__host__ uint32_t topn_tiles(const lux_cf_topn_args* a) {
  return (a->c_hi - a->c_lo + TOPN_TILE - 1) / TOPN_TILE;
}

__host__ bool topn_args_ok(const lux_cf_topn_args* a) {
  return a && a->vec && a->queries && a->excl_ptr && a->excl_adj &&
         a->out_items && a->out_scores && a->nv && a->K >= 1 &&
         a->K <= 128 && a->q >= 1 && a->n >= 1 && a->n <= TOPN_NMAX &&
         a->c_lo < a->c_hi && a->c_hi <= a->nv &&
         a->c_hi <= 0x7fffffffu;  // items are i32
}

__host__ uint32_t topn_cus() {
  static uint32_t cus = 0;  // the device property is read once
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || n < 1)
      n = 256;
    cus = (uint32_t)n;
  }
  return cus;
}

template <int KP>
__host__ void topn_launch(hipStream_t s, const lux_cf_topn_args* a, int* items,
                          float* scores, bool vec4) {
  hipLaunchKernelGGL(cf_topn_kernel<KP>,
                     dim3((a->q + TOPN_QB - 1) / TOPN_QB, a->splits),
                     dim3(BLOCK), 0, s, *a, items, scores, vec4);
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_cf_topn_plan(uint32_t q, uint32_t m, uint32_t n,
                              uint32_t force) {
  if (!q || !m || n < 1 || n > TOPN_NMAX) return 0;
  const uint32_t tiles = (m + TOPN_TILE - 1) / TOPN_TILE;
  const uint64_t wgs = ((uint64_t)q + TOPN_QB - 1) / TOPN_QB;
  const uint64_t want = 2ull * topn_cus();
  uint64_t s = force ? force : wgs >= want ? 1 : (want + wgs - 1) / wgs;
  if (s > tiles) s = tiles;
  if (s > TOPN_MERGE_MAX / n) s = TOPN_MERGE_MAX / n;  // the merge's LDS
  // no empty split: S = ceil(tiles / ceil(tiles / s))
  const uint32_t per = (uint32_t)((tiles + s - 1) / s);
  return (tiles + per - 1) / per;
}

int lux_gpu_cf_topn(uint64_t stream, const lux_cf_topn_args* a) {
  if (!topn_args_ok(a) || a->splits < 1 || a->splits > 65535) return -1;
  const uint32_t tiles = topn_tiles(a);
  if ((uint64_t)a->splits * a->tiles_per_split < tiles ||
      (uint64_t)(a->splits - 1) * a->tiles_per_split >= tiles)
    return -1;
  if (a->splits > 1 && (!a->part_items || !a->part_scores ||
                        a->splits * a->n > (uint32_t)TOPN_MERGE_MAX))
    return -1;
  if (((uint64_t)a->q + TOPN_QB - 1) / TOPN_QB > 0x7fffffffull) return -1;
  const hipStream_t s = (hipStream_t)stream;
  const bool vec4 = a->K % 4 == 0 && (uintptr_t)a->vec % 16 == 0;
  int* items = a->splits > 1 ? a->part_items : a->out_items;
  float* scores = a->splits > 1 ? a->part_scores : a->out_scores;
  if (a->K <= 32) topn_launch<32>(s, a, items, scores, vec4);
  else if (a->K <= 64) topn_launch<64>(s, a, items, scores, vec4);
  else topn_launch<128>(s, a, items, scores, vec4);
  int launches = 1;
  if (a->splits > 1) {
    hipLaunchKernelGGL(cf_topn_merge_kernel, dim3(a->q), dim3(WAVE), 0, s,
                       *a);
    launches = 2;
  }
  LUX_POST_LAUNCH(stream);
  return launches;
}

int lux_gpu_cf_topn_check(uint64_t stream, const lux_cf_topn_args* a,
                          const int* items, const float* scores,
                          uint32_t* bad) {
  if (!topn_args_ok(a) || !items || !scores || !bad) return -1;
  const uint64_t g = ((uint64_t)a->q + BLOCK / WAVE - 1) / (BLOCK / WAVE);
  if (g > 0x7fffffffull) return -1;
  hipLaunchKernelGGL(cf_topn_plain_kernel, dim3((uint32_t)g), dim3(BLOCK), 0,
                     (hipStream_t)stream, *a, items, scores, bad);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_cf_topn_keys(uint64_t stream, uint32_t nrows,
                         const lux::E_ID* row_ptr, const lux::V_ID* col,
                         uint64_t e0, uint64_t e1, unsigned long long* out) {
  if (!nrows || !row_ptr || !col || !out || e0 > e1) return -1;
  if (e0 == e1) return 0;
  hipLaunchKernelGGL(cf_topn_keys_kernel, dim3(grid_for(e1 - e0)),
                     dim3(BLOCK), 0, (hipStream_t)stream, nrows, row_ptr, col,
                     e0, e1, out);
  LUX_POST_LAUNCH(stream);
  return 0;
}

}  // extern "C"
