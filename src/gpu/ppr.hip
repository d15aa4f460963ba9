// Batched personalised PageRank (random walk with restart) on one GPU: K rank
// vectors kept vertex-major, so that one gathered source brings a whole row of
// B = 16 / 32 / 64 columns and the edge list is read once for B answers. No
// reference equivalent; the definition is in API.md.
//
// State: two f32 buffers [nv][B] in the stored form y = x / outdeg (x where
// outdeg == 0), as PageRank keeps it, so the gather needs no degree lookup.
// Every lane owns 4 consecutive columns and moves them as one 16-byte vector.
// A row therefore belongs to a group of LPR = B / 4 lanes (4, 8, 16) and a
// wave holds G = 64 / LPR groups (16, 8, 4).
//
// One sweep launch per iteration, three static role lists by in-degree:
//   group  in-degree 0..PPR_GROUP: one lane group per row, G rows per wave at
//          a time, the row walked serially two gathers at a time. No
//          cross-lane traffic.
//   wave   up to hub entries: one wave per row. 64 source ids come with one
//          coalesced load and reach the groups by cross-lane reads; group g
//          takes the ids g, g + G, ... of the 64, so every step gathers G
//          source rows and all LPR steps of a load are in flight together.
//          Each group keeps its partial vector; one xor-butterfly over the
//          groups ends the row.
//   hub    longer rows in {vertex, chunk} items of hub entries, a workgroup
//          per item: its four waves take a quarter each (a multiple of 64
//          entries) wave-role style, meet in an LDS [4][B] tile, and the item's
//          partial vector goes to scratch[item][B]. A second small launch
//          sums a row's items in item order.
// The lanes that hold a row's final sums run the epilogue: the teleport (a
// sparse list searched only by the rows whose bit is set), x = d * sum + t,
// the residual |x - y_old * max(outdeg, 1)| and the 16-byte store of y.
//
// No float atomics: the summation order of a row is a function of its role,
// B and hub alone, so two runs give the same bits. The residual is a maximum
// of non-negative floats, whose bit patterns order as u32: lane max, wave
// max, one vector atomicMax per wave.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t PPR_GROUP = 8;       // longest group-role row
constexpr uint32_t PPR_HUB = 1024;      // default longest wave-role row
constexpr uint32_t PPR_HUB_MIN = 64;
constexpr uint32_t PPR_HUB_MAX = 1u << 20;
constexpr int PPR_MAX_GRID = 1 << 14;   // blocks per role
constexpr int PPR_NW = BLOCK / WAVE;

__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// Columns [4 * sub, 4 * sub + 4) of row u.
template <int B>
__device__ __forceinline__ float4 row_load(const float* y, V_ID u, int sub) {
  return reinterpret_cast<const float4*>(y + (uint64_t)u * B)[sub];
}

// The teleport entries of row v that fall into this lane's four columns,
// each value[c] (tp_weight, or the seed kernel's per-column x^0).
__device__ __forceinline__ float4 teleport(const lux_ppr_args& a, V_ID v,
                                           int sub, const float* by_col) {
  float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if ((a.tp_bits[v >> 5] >> (v & 31)) & 1) {
    uint32_t lo = 0, hi = a.n_tp;  // the first entry with vertex >= v
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.tp_vertex[mid] < v) lo = mid + 1; else hi = mid;
    }
    for (; lo < a.n_tp && a.tp_vertex[lo] == v; lo++) {
      const uint32_t c = a.tp_col[lo];
      if ((int)(c >> 2) == sub) t[c & 3] = by_col ? by_col[c] : a.tp_weight[lo];
    }
  }
  return make_float4(t[0], t[1], t[2], t[3]);
}

// Row epilogue in the lane that holds the final sums of its four columns;
// returns max(res, the residual of these columns).
template <int B>
__device__ __forceinline__ float finish_row(const lux_ppr_args& a,
                                            const float* y_old, float* y_new,
                                            V_ID v, int sub, float4 s,
                                            float res) {
  const float4 t = teleport(a, v, sub, nullptr);
  const float d = a.damping;
  float4 x = make_float4(d * s.x + t.x, d * s.y + t.y, d * s.z + t.z,
                         d * s.w + t.w);
  const uint32_t deg = a.outdeg[v];
  const float scale = (float)(deg ? deg : 1u);
  const float4 o = row_load<B>(y_old, v, sub);
  res = fmaxf(res, fmaxf(fmaxf(fabsf(x.x - o.x * scale),
                               fabsf(x.y - o.y * scale)),
                         fmaxf(fabsf(x.z - o.z * scale),
                               fabsf(x.w - o.w * scale))));
  if (deg) x = make_float4(x.x / scale, x.y / scale, x.z / scale, x.w / scale);
  reinterpret_cast<float4*>(y_new + (uint64_t)v * B)[sub] = x;
  return res;
}

// Entries [b, end) of the edge list, summed by the whole wave; the result is
// in every lane of every group (the butterfly adds the same pairs in every
// group, and a + b == b + a).
template <int B>
__device__ __forceinline__ float4 wave_row(const float* y, const V_ID* col,
                                           E_ID b, E_ID end, int lane) {
  constexpr int LPR = B / 4, G = WAVE / LPR;
  const int grp = lane / LPR, sub = lane % LPR;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (E_ID base = b; base < end; base += WAVE) {
    const E_ID x = base + lane;
    const V_ID src = x < end ? col[x] : 0;
    const E_ID left = end - base;
    const int n = left < (E_ID)WAVE ? (int)left : WAVE;
    float4 t[LPR];
#pragma unroll
    for (int s = 0; s < LPR; s++) {
      const int j = s * G + grp;
      const V_ID u = __shfl(src, j, WAVE);
      t[s] = j < n ? row_load<B>(y, u, sub)
                   : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int s = 0; s < LPR; s++) acc = f4_add(acc, t[s]);
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

// Called by every lane of the wave.
__device__ __forceinline__ void publish_residual(float* residual, float res,
                                                 int lane) {
  const uint32_t m = wave_reduce_max(__float_as_uint(res));
  if (lane == 0 && m) atomicMax(reinterpret_cast<uint32_t*>(residual), m);
}

// Blocks [0, gb) run the group role, [gb, gb + wb) the wave role, the last
// hb the hub items.
template <int B>
__global__ void __launch_bounds__(BLOCK)
ppr_sweep_kernel(lux_ppr_args a, const float* __restrict__ y_old,
                 float* __restrict__ y_new, float* residual, uint32_t gb,
                 uint32_t wb, uint32_t hb) {
  constexpr int LPR = B / 4, G = WAVE / LPR;
  __shared__ float4 tile[PPR_NW][LPR];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  const int sub = lane % LPR;
  const uint32_t b = blockIdx.x;
  float res = 0.0f;
  if (b < gb) {
    for (uint64_t i = (uint64_t)b * (PPR_NW * G) + threadIdx.x / LPR;
         i < a.n_grp; i += (uint64_t)gb * (PPR_NW * G)) {
      const V_ID v = a.grp_in[i];
      const E_ID end = a.in_ptr[v + 1];
      E_ID e = a.in_ptr[v];
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (; e + 1 < end; e += 2) {
        const V_ID u0 = a.in_col[e], u1 = a.in_col[e + 1];
        const float4 t0 = row_load<B>(y_old, u0, sub);
        const float4 t1 = row_load<B>(y_old, u1, sub);
        acc = f4_add(f4_add(acc, t0), t1);
      }
      if (e < end) acc = f4_add(acc, row_load<B>(y_old, a.in_col[e], sub));
      res = finish_row<B>(a, y_old, y_new, v, sub, acc, res);
    }
  } else if (b < gb + wb) {
    for (uint64_t i = (uint64_t)(b - gb) * PPR_NW + wid; i < a.n_wav;
         i += (uint64_t)wb * PPR_NW) {
      const V_ID v = a.wav_in[i];
      const float4 acc =
          wave_row<B>(y_old, a.in_col, a.in_ptr[v], a.in_ptr[v + 1], lane);
      if (lane < LPR) res = finish_row<B>(a, y_old, y_new, v, sub, acc, res);
    }
  } else {
    for (uint64_t i = b - gb - wb; i < a.n_hub_in; i += hb) {
      const V_ID v = a.hub_in[2 * i];
      const uint32_t c = a.hub_in[2 * i + 1];
      const E_ID r0 = a.in_ptr[v] + (E_ID)c * a.hub;
      const E_ID rest = a.in_ptr[v + 1] - r0;
      const E_ID len = rest < a.hub ? rest : (E_ID)a.hub;
      const E_ID q = (len + PPR_NW * WAVE - 1) / (PPR_NW * WAVE) * WAVE;
      const E_ID w0 = (E_ID)wid * q < len ? (E_ID)wid * q : len;
      const E_ID w1 = w0 + q < len ? w0 + q : len;
      const float4 acc = wave_row<B>(y_old, a.in_col, r0 + w0, r0 + w1, lane);
      if (lane < LPR) tile[wid][lane] = acc;
      __syncthreads();
      if (threadIdx.x < LPR) {
        float4 s = tile[0][threadIdx.x];
        for (int w = 1; w < PPR_NW; w++) s = f4_add(s, tile[w][threadIdx.x]);
        reinterpret_cast<float4*>(a.scratch + i * B)[threadIdx.x] = s;
      }
      __syncthreads();  // tile is reused by the next item
    }
  }
  publish_residual(residual, res, lane);
}

// One lane group per hub row: the items' partial vectors in item order.
template <int B>
__global__ void __launch_bounds__(BLOCK)
ppr_hub_finish_kernel(lux_ppr_args a, const float* __restrict__ y_old,
                      float* __restrict__ y_new, float* residual) {
  constexpr int LPR = B / 4;
  const int lane = threadIdx.x & (WAVE - 1), sub = lane % LPR;
  float res = 0.0f;
  for (uint64_t r = (uint64_t)blockIdx.x * (BLOCK / LPR) + threadIdx.x / LPR;
       r < a.n_hub_rows; r += (uint64_t)gridDim.x * (BLOCK / LPR)) {
    const V_ID v = a.hub_rows[3 * r];
    const uint64_t first = a.hub_rows[3 * r + 1];
    const uint32_t n = a.hub_rows[3 * r + 2];
    const float4* part = reinterpret_cast<const float4*>(a.scratch + first * B);
    float4 s = part[sub];
    for (uint32_t k = 1; k < n; k++) s = f4_add(s, part[(uint64_t)k * LPR + sub]);
    res = finish_row<B>(a, y_old, y_new, v, sub, s, res);
  }
  publish_residual(residual, res, lane);
}

// One lane per (vertex, four columns): x^0 in stored form.
__global__ void __launch_bounds__(BLOCK)
ppr_seed_kernel(lux_ppr_args a, float* y, const float* col_x0) {
  const uint32_t lpr = a.width / 4;
  const uint64_t n = (uint64_t)a.nv * lpr;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * BLOCK) {
    const V_ID v = (V_ID)(i / lpr);
    float4 x = teleport(a, v, (int)(i % lpr), col_x0);
    const uint32_t deg = a.outdeg[v];
    if (deg) {
      const float s = (float)deg;
      x = make_float4(x.x / s, x.y / s, x.z / s, x.w / s);
    }
    reinterpret_cast<float4*>(y)[i] = x;
  }
}

// One lane per (vertex, column c < k) of the batch.
__global__ void __launch_bounds__(BLOCK)
ppr_unscale_kernel(lux_ppr_args a, const float* y, float* out, uint32_t ld,
                   uint32_t col0, uint32_t k) {
  const uint64_t n = (uint64_t)a.nv * k;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t v = i / k, c = i % k;
    const uint32_t deg = a.outdeg[v];
    out[v * ld + col0 + c] = y[v * a.width + c] * (float)(deg ? deg : 1u);
  }
}

// The check: one lane per (vertex, column), the row walked serially in entry
// order from y_old, no roles, no vectors, no cross-lane traffic.
__global__ void __launch_bounds__(BLOCK)
ppr_plain_kernel(lux_ppr_args a, const float* y_old, const float* y_new,
                 unsigned long long* bad_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t B = a.width;
  const uint64_t n = (uint64_t)a.nv * B;
  unsigned long long bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * BLOCK) {
    const V_ID v = (V_ID)(i / B);
    const uint32_t c = (uint32_t)(i % B);
    const E_ID e0 = a.in_ptr[v], end = a.in_ptr[v + 1];
    float sum = 0.0f;
    for (E_ID e = e0; e < end; e++) sum += y_old[(uint64_t)a.in_col[e] * B + c];
    const float4 t4 = teleport(a, v, (int)(c >> 2), nullptr);
    const float t = (c & 3) == 0 ? t4.x : (c & 3) == 1 ? t4.y
                  : (c & 3) == 2 ? t4.z : t4.w;
    float x = a.damping * sum + t;
    const uint32_t deg = a.outdeg[v];
    if (deg) x /= (float)deg;
    const float tol = (float)(end - e0 + 6) * 0x1p-23f * x + 1e-30f;
    if (!(fabsf(y_new[i] - x) <= tol)) bad++;
  }
  bad = wave_reduce_sum(bad);
  if (lane == 0 && bad) atomicAdd(bad_out, bad);
}

__host__ bool ppr_args_ok(const lux_ppr_args* a) {
  return a && a->nv && a->hub >= PPR_HUB_MIN && a->hub <= PPR_HUB_MAX &&
         (a->width == 16 || a->width == 32 || a->width == 64) &&
         a->n_grp <= a->nv && a->n_wav <= a->nv && a->n_hub_rows <= a->nv &&
         a->n_hub_rows <= a->n_hub_in && a->n_tp >= 1 && a->damping > 0.0f &&
         a->damping < 1.0f &&
         (uint64_t)a->n_grp + a->n_wav + a->n_hub_rows == a->nv;
}

__host__ uint32_t ppr_blocks(uint64_t work, uint32_t per_block) {
  uint64_t g = (work + per_block - 1) / per_block;
  return (uint32_t)(g > (uint64_t)PPR_MAX_GRID ? PPR_MAX_GRID : g);
}

template <int B>
__host__ int ppr_sweep(hipStream_t s, const lux_ppr_args* a,
                       const float* y_old, float* y_new, float* residual) {
  constexpr int LPR = B / 4;
  const uint32_t gb = ppr_blocks(a->n_grp, BLOCK / LPR);
  const uint32_t wb = ppr_blocks(a->n_wav, PPR_NW);
  const uint32_t hb = ppr_blocks(a->n_hub_in, 1);
  hipLaunchKernelGGL(ppr_sweep_kernel<B>, dim3(gb + wb + hb), dim3(BLOCK), 0,
                     s, *a, y_old, y_new, residual, gb, wb, hb);
  if (!a->n_hub_rows) return 1;
  hipLaunchKernelGGL(ppr_hub_finish_kernel<B>,
                     dim3(ppr_blocks(a->n_hub_rows, BLOCK / LPR)), dim3(BLOCK),
                     0, s, *a, y_old, y_new, residual);
  return 2;
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_ppr_group_limit() { return PPR_GROUP; }
uint32_t lux_gpu_ppr_hub_default() { return PPR_HUB; }
uint32_t lux_gpu_ppr_hub_min() { return PPR_HUB_MIN; }
uint32_t lux_gpu_ppr_hub_max() { return PPR_HUB_MAX; }

int lux_gpu_ppr_seed(uint64_t stream, const lux_ppr_args* a, float* y,
                     const float* col_x0) {
  if (!ppr_args_ok(a) || !y || !col_x0) return -1;
  hipLaunchKernelGGL(ppr_seed_kernel,
                     dim3(grid_for((uint64_t)a->nv * (a->width / 4))),
                     dim3(BLOCK), 0, (hipStream_t)stream, *a, y, col_x0);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_ppr_sweep(uint64_t stream, const lux_ppr_args* a,
                      const float* y_old, float* y_new, float* residual) {
  if (!ppr_args_ok(a) || !y_old || !y_new || y_old == y_new || !residual)
    return -1;
  const hipStream_t s = (hipStream_t)stream;
  const int n = a->width == 16   ? ppr_sweep<16>(s, a, y_old, y_new, residual)
                : a->width == 32 ? ppr_sweep<32>(s, a, y_old, y_new, residual)
                                 : ppr_sweep<64>(s, a, y_old, y_new, residual);
  LUX_POST_LAUNCH(stream);
  return n;
}

int lux_gpu_ppr_unscale(uint64_t stream, const lux_ppr_args* a, const float* y,
                        float* out, uint32_t ld, uint32_t col0, uint32_t k) {
  if (!ppr_args_ok(a) || !y || !out || k < 1 || k > a->width ||
      (uint64_t)col0 + k > ld)
    return -1;
  hipLaunchKernelGGL(ppr_unscale_kernel, dim3(grid_for((uint64_t)a->nv * k)),
                     dim3(BLOCK), 0, (hipStream_t)stream, *a, y, out, ld, col0,
                     k);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_ppr_check(uint64_t stream, const lux_ppr_args* a,
                      const float* y_old, const float* y_new,
                      unsigned long long* bad) {
  if (!ppr_args_ok(a) || !y_old || !y_new || !bad) return -1;
  hipLaunchKernelGGL(ppr_plain_kernel,
                     dim3(grid_for((uint64_t)a->nv * a->width)), dim3(BLOCK),
                     0, (hipStream_t)stream, *a, y_old, y_new, bad);
  LUX_POST_LAUNCH(stream);
  return 0;
}

}  // extern "C"
