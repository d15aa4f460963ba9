// Collaborative filtering — implicit-feedback ALS (Hu, Koren, Volinsky 2008)
// for K <= 64, all fp32 (gfx950).
//
// For a row v of the side being solved, with Y the factor rows of the whole
// other side and (y_e, w_e) v's CSC entries:
//     A_v = Y^T Y + alpha * sum_e w_e y_e y_e^T + reg I
//     b_v = sum_e (1 + alpha w_e) y_e
//     x_v = A_v^-1 b_v
// Unlike explicit ALS (cf_als.hip) every user/item pair enters the loss, which
// shows up as the dense term Y^T Y shared by all rows of a phase.
//
// Three pieces:
//   1. SIDE GRAM. The rows of one side are one contiguous n x K stream. Each
//      one-wave workgroup owns a contiguous slab of rows, stages 32-row tiles
//      in LDS (pitch 80: the 4 x 16 fragment read of a k-group lands on 64
//      distinct banks) and accumulates the 10 upper 16x16 tiles with
//      v_mfma_f32_16x16x4_f32; the next tile's loads fly under the MFMA burst.
//      Partial tiles go to scratch in accumulator layout; a second launch sums
//      them in workgroup order (16 runs of consecutive workgroups, then the 16
//      run totals in order) and mirrors the lower half. No atomics: the same
//      bits every run.
//   2. FUSED ROW SOLVE (deg < T2). One wave per row. The accumulators START
//      from the side Gram (C operand of the first MFMA), every staged source
//      row is scaled by sqrt(alpha w_e) on its way from registers to LDS, so
//      the weighted Gram is again S^T S and one fragment still serves as A of
//      its tile row and B of its tile column; b_v folds from the unscaled
//      register copy. Then the 64-row in-LDS Cholesky and two triangular
//      solves with the runtime reg.
//   3. HUB ROWS (deg >= T2). One wave per 8192-entry chunk writes the chunk's
//      weighted partial Gram (10 upper tiles) and rhs to ITS OWN scratch slot;
//      the hub solve sums a row's slots in chunk order, adds the side Gram and
//      reg, factors and solves. No atomics here either.
#include "gpu_common.h"

namespace lux {

constexpr int IALS_K = 64;       // max latent rank
constexpr int IALS_TILE = 32;    // rows staged per LDS tile
constexpr int IALS_SP = 80;      // stage pitch: 16 mod 64 banks
constexpr int IALS_GP = 65;      // Cholesky pitch (column walks)
constexpr int IALS_TB = 64;      // one wave per workgroup
constexpr int IALS_NT = 10;      // upper 16x16 tiles of the 4x4 grid
constexpr int IALS_TILE_F = IALS_NT * WAVE * 4;  // floats of 10 acc tiles
constexpr int IALS_SLOT_F = IALS_TILE_F + IALS_K;  // chunk slot: tiles + rhs
constexpr uint32_t IALS_GRAM_MAX_WG = 1024;
constexpr int IALS_RED_TB = 1024;  // reduce: 16 waves per tile
constexpr uint32_t IALS_CHUNK = 8192;  // entries per hub chunk (pull.hip)
constexpr float IALS_PIVOT_RTOL = 1e-5f;

using f32x4 = __attribute__((ext_vector_type(4))) float;

// tile t of the upper triangle sits at block row TI[t], block column TJ[t]
#define IALS_TI {0, 0, 0, 0, 1, 1, 1, 2, 2, 3}
#define IALS_TJ {0, 1, 2, 3, 1, 2, 3, 2, 3, 3}

__device__ __forceinline__ void ials_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Broadcast lane l's value (l is wave-uniform): one v_readlane, no LDS trip.
__device__ __forceinline__ float ials_lane(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// One k-group (4 staged rows starting at `base`) into the 10 accumulators.
// Fragment f[t] = S[k0 + (lane>>4)][16 t + (lane&15)] is operand A of tile row
// t and operand B of tile column t (gfx950 16x16x4 f32 lane maps).
__device__ __forceinline__ void ials_mfma_group(const float* base,
                                                f32x4 acc[IALS_NT]) {
  float f0 = base[0], f1 = base[16], f2 = base[32], f3 = base[48];
  acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0, f0, acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0, f1, acc[1], 0, 0, 0);
  acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0, f2, acc[2], 0, 0, 0);
  acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0, f3, acc[3], 0, 0, 0);
  acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1, f1, acc[4], 0, 0, 0);
  acc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1, f2, acc[5], 0, 0, 0);
  acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1, f3, acc[6], 0, 0, 0);
  acc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(f2, f2, acc[7], 0, 0, 0);
  acc[8] = __builtin_amdgcn_mfma_f32_16x16x4f32(f2, f3, acc[8], 0, 0, 0);
  acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(f3, f3, acc[9], 0, 0, 0);
}

// ============================== side Gram ==============================

// The slab is a flat stream of floats: element f of a tile is row f / K,
// column f % K, and lane `lane` owns f = j * 64 + lane for j = 0..31 (the
// first 32 K of them exist). Issue the whole tile's loads into registers;
// elements past the slab read as zero, so ragged tails are zero rows in LDS.
__device__ __forceinline__ void ials_tile_loads(const float* tab, uint64_t t,
                                                uint64_t e1, uint32_t tile_f,
                                                int lane,
                                                float tmp[IALS_TILE]) {
#pragma unroll
  for (int j = 0; j < IALS_TILE; j++) {
    uint32_t f = (uint32_t)j * WAVE + lane;
    tmp[j] = (f < tile_f && t + f < e1) ? tab[t + f] : 0.0f;
  }
}

// tab points at row `lo`; nelem = (hi - lo) * K floats; workgroup g owns rows
// [g * slab_rows, (g + 1) * slab_rows) and writes its 10 accumulator tiles to
// partial[g] as f32x4[10][64].
__global__ __launch_bounds__(IALS_TB) void cf_ials_side_gram_kernel(
    const float* tab, uint64_t nelem, int K, uint32_t slab_rows,
    float* partial) {
  __shared__ float S[IALS_TILE * IALS_SP];
  int lane = threadIdx.x;
  // columns >= K are never staged: zero once, they stay zero
  for (int i = lane; i < IALS_TILE * IALS_SP; i += IALS_TB) S[i] = 0.0f;
  uint64_t e0 = (uint64_t)blockIdx.x * slab_rows * (uint32_t)K;
  uint64_t e1 = e0 + (uint64_t)slab_rows * (uint32_t)K;
  if (e1 > nelem) e1 = nelem;
  uint32_t tile_f = IALS_TILE * (uint32_t)K;
  int q64 = WAVE / K, r64 = WAVE % K;  // how (row, col) moves per 64 floats
  int row0 = lane / K, col0 = lane % K;
  f32x4 acc[IALS_NT];
#pragma unroll
  for (int t = 0; t < IALS_NT; t++) acc[t] = {0, 0, 0, 0};
  float tmp[IALS_TILE];
  if (e0 < e1) ials_tile_loads(tab, e0, e1, tile_f, lane, tmp);
  const float* frag = &S[(lane >> 4) * IALS_SP + (lane & 15)];
  for (uint64_t t = e0; t < e1; t += tile_f) {
    int row = row0, col = col0;
#pragma unroll
    for (int j = 0; j < IALS_TILE; j++) {
      if (row < IALS_TILE) S[row * IALS_SP + col] = tmp[j];
      row += q64;
      col += r64;
      if (col >= K) {
        col -= K;
        row++;
      }
    }
    ials_lds_sync();
    // the next tile's loads land under this tile's 80 MFMAs
    if (t + tile_f < e1)
      ials_tile_loads(tab, t + tile_f, e1, tile_f, lane, tmp);
#pragma unroll
    for (int kk = 0; kk < IALS_TILE; kk += 4)
      ials_mfma_group(frag + kk * IALS_SP, acc);
    ials_lds_sync();  // tile consumed before the next stage overwrites it
  }
  f32x4* out = (f32x4*)partial + (uint64_t)blockIdx.x * IALS_NT * WAVE;
#pragma unroll
  for (int t = 0; t < IALS_NT; t++) out[t * WAVE + lane] = acc[t];
}

// Workgroup t sums tile t of the nwg partials: wave w takes the w-th run of
// consecutive workgroups in order, wave 0 then adds the 16 run totals in
// order. Writes the 64x64 matrix with the lower half mirrored (element (r, c)
// of a diagonal tile is written from its c >= r copy only, so the result is
// symmetric bit for bit).
__global__ __launch_bounds__(IALS_RED_TB) void cf_ials_side_gram_reduce_kernel(
    const float* partial, uint32_t nwg, float* out) {
  static constexpr int TI[IALS_NT] = IALS_TI;
  static constexpr int TJ[IALS_NT] = IALS_TJ;
  __shared__ f32x4 runs[IALS_RED_TB / WAVE][WAVE];
  int t = blockIdx.x;
  int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  uint32_t per = (nwg + IALS_RED_TB / WAVE - 1) / (IALS_RED_TB / WAVE);
  uint32_t b = (uint32_t)w * per, e = b + per;
  if (e > nwg) e = nwg;
  const f32x4* P = (const f32x4*)partial + (uint32_t)t * WAVE + lane;
  f32x4 s = {0, 0, 0, 0};
  for (uint32_t i = b; i < e; i++) s += P[(uint64_t)i * IALS_NT * WAVE];
  runs[w][lane] = s;
  __syncthreads();
  if (w) return;
  s = runs[0][lane];
  for (int k = 1; k < IALS_RED_TB / WAVE; k++) s += runs[k][lane];
  int row = TI[t] * 16 + (lane >> 4) * 4, gc = TJ[t] * 16 + (lane & 15);
#pragma unroll
  for (int reg = 0; reg < 4; reg++) {
    int gr = row + reg;
    if (gc >= gr) {
      out[gr * IALS_K + gc] = s[reg];
      out[gc * IALS_K + gr] = s[reg];
    }
  }
}

// ======================= weighted per-row Gram =======================

struct CFIalsArgs {
  const E_ID* row_ptr;  // u64[vp+1] local
  const V_ID* col;      // u32[ep]
  const WeightType* w;  // i32[ep], >= 0
  const float* oldv;    // f32[nv*K]
  float* newv;          // f32[vp*K]
  const float* gram;    // f32[64*64] unregularised side Gram
  float alpha;
  float reg;
  int K;
};

// The stage tile ALIASES the matrix: A_v sits in the accumulators until the
// last tile is consumed, so 16.6 KB per wave instead of 26.9 KB and LDS no
// longer caps the waves per CU below what the registers allow.
struct IalsLds {
  union {
    float S[IALS_TILE * IALS_SP];  // staged, scaled source rows (row = entry)
    float G[IALS_K * IALS_GP];     // A_v -> Cholesky factor (in place)
  };
};

// Issue the whole tile's source-row loads into registers (lane = dim).
__device__ __forceinline__ void ials_vec_loads(const CFIalsArgs& a,
                                               uint32_t mycol, int rem,
                                               int lane,
                                               float tmp[IALS_TILE]) {
#pragma unroll
  for (int r = 0; r < IALS_TILE; r++) {
    uint32_t src = (uint32_t)__builtin_amdgcn_readlane((int)mycol, r);
    tmp[r] = (r < rem && lane < a.K) ? a.oldv[(uint64_t)src * a.K + lane]
                                     : 0.0f;
  }
}

// acc += alpha * sum_e w_e y_e y_e^T and *rhs += sum_e (1 + alpha w_e) y_e
// over the entries [b, e). Lane r < 32 holds entry r's column and weight;
// staged row r is y_e * sqrt(alpha w_e), rows past the range are zero (their
// registers are zero), so the k-loop runs to the next multiple of 4.
__device__ __forceinline__ void ials_gram_range(const CFIalsArgs& a, E_ID b,
                                                E_ID e, int lane, float* S,
                                                f32x4 acc[IALS_NT],
                                                float* rhs) {
  if (b >= e) return;
  int rem = (int)(e - b < IALS_TILE ? e - b : (E_ID)IALS_TILE);
  uint32_t mycol = 0;
  float myw = 0.0f;
  if (lane < rem) {
    mycol = a.col[b + lane];
    myw = (float)a.w[b + lane];
  }
  float tmp[IALS_TILE];
  ials_vec_loads(a, mycol, rem, lane, tmp);
  float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
  const float* frag = &S[(lane >> 4) * IALS_SP + (lane & 15)];
  for (E_ID t = b; t < e; t += IALS_TILE) {
    float aw = a.alpha * myw;
    float sq = sqrtf(aw), cf = 1.0f + aw;
#pragma unroll
    for (int r = 0; r < IALS_TILE; r += 4) {
      float x0 = tmp[r], x1 = tmp[r + 1], x2 = tmp[r + 2], x3 = tmp[r + 3];
      S[r * IALS_SP + lane] = x0 * ials_lane(sq, r);
      S[(r + 1) * IALS_SP + lane] = x1 * ials_lane(sq, r + 1);
      S[(r + 2) * IALS_SP + lane] = x2 * ials_lane(sq, r + 2);
      S[(r + 3) * IALS_SP + lane] = x3 * ials_lane(sq, r + 3);
      r0 += ials_lane(cf, r) * x0;
      r1 += ials_lane(cf, r + 1) * x1;
      r2 += ials_lane(cf, r + 2) * x2;
      r3 += ials_lane(cf, r + 3) * x3;
    }
    int rem4 = (rem + 3) & ~3;
    // next tile's column/weight now, its vectors after the barrier
    E_ID t2 = t + IALS_TILE;
    bool more = t2 < e;
    uint32_t ncol = 0;
    float nw = 0.0f;
    if (more) {
      rem = (int)(e - t2 < IALS_TILE ? e - t2 : (E_ID)IALS_TILE);
      if (lane < rem) {
        ncol = a.col[t2 + lane];
        nw = (float)a.w[t2 + lane];
      }
    }
    ials_lds_sync();
    if (more) {  // these land under the MFMA burst
      myw = nw;
      mycol = ncol;
      ials_vec_loads(a, ncol, rem, lane, tmp);
    }
    for (int kk = 0; kk < rem4; kk += 4)
      ials_mfma_group(frag + kk * IALS_SP, acc);
    ials_lds_sync();  // tile consumed before the next stage overwrites it
  }
  *rhs += (r0 + r1) + (r2 + r3);
}

// The side Gram in accumulator layout (40 loads from a 16 KB matrix).
__device__ __forceinline__ void ials_load_base(const float* gram, int lane,
                                               f32x4 acc[IALS_NT]) {
  static constexpr int TI[IALS_NT] = IALS_TI;
  static constexpr int TJ[IALS_NT] = IALS_TJ;
  int row = (lane >> 4) * 4, col = lane & 15;
#pragma unroll
  for (int t = 0; t < IALS_NT; t++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++)
      acc[t][reg] = gram[(TI[t] * 16 + row + reg) * IALS_K + TJ[t] * 16 + col];
}

// Accumulators -> LDS matrix (lower half mirrored; 16x16x4 C/D map: row =
// (lane>>4)*4 + reg, col = lane&15), then reg on the diagonal of the K used
// dimensions and an identity diagonal on the rest.
__device__ __forceinline__ void ials_dump_gram(float* G, f32x4 acc[IALS_NT],
                                               int lane, int K, float reg_) {
  static constexpr int TI[IALS_NT] = IALS_TI;
  static constexpr int TJ[IALS_NT] = IALS_TJ;
  int row = (lane >> 4) * 4, col = lane & 15;
#pragma unroll
  for (int t = 0; t < IALS_NT; t++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      int gr = TI[t] * 16 + row + reg;
      int gc = TJ[t] * 16 + col;
      float v = acc[t][reg];
      G[gr * IALS_GP + gc] = v;
      if (TI[t] != TJ[t]) G[gc * IALS_GP + gr] = v;
    }
  }
  ials_lds_sync();
  G[lane * IALS_GP + lane] = lane < K ? G[lane * IALS_GP + lane] + reg_ : 1.0f;
  ials_lds_sync();
}

// In-place lower Cholesky (one wave, lane = row) with the project's pivot
// rule: a pivot at or below max(reg / 2, 1e-5 * the row's original diagonal)
// carries no information in fp32; it gets the -1 sentinel, a zeroed column and
// no step in the solves.
__device__ __forceinline__ void ials_cholesky64(float* G, int lane,
                                                float reg_) {
  float thr = fmaxf(reg_ * 0.5f, IALS_PIVOT_RTOL * G[lane * IALS_GP + lane]);
  for (int k = 0; k < IALS_K; k++) {
    float piv = G[k * IALS_GP + k];
    bool ok = piv > ials_lane(thr, k);
    float dkk = ok ? sqrtf(piv) : 1.0f;
    float lik = (lane > k && ok) ? G[lane * IALS_GP + k] / dkk : 0.0f;
    if (lane == k) G[k * IALS_GP + k] = ok ? dkk : -1.0f;
    if (lane > k) G[lane * IALS_GP + k] = lik;
    ials_lds_sync();
    for (int j = k + 1; j <= lane; j++)
      G[lane * IALS_GP + j] -= lik * G[j * IALS_GP + k];
    ials_lds_sync();
  }
}

// Solve L L^T x = r; r and the result live lane = dim in a register.
__device__ __forceinline__ float ials_solve64(const float* G, float r,
                                              int lane) {
  for (int k = 0; k < IALS_K; k++) {  // forward: L y = r
    float lkk = G[k * IALS_GP + k];
    float yk = lkk > 0.0f ? ials_lane(r, k) / lkk : 0.0f;
    if (lane == k) r = yk;
    else if (lane > k) r -= G[lane * IALS_GP + k] * yk;
  }
  for (int k = IALS_K - 1; k >= 0; k--) {  // backward: L^T x = y
    float lkk = G[k * IALS_GP + k];
    float xk = lkk > 0.0f ? ials_lane(r, k) / lkk : 0.0f;
    if (lane == k) r = xk;
    else if (lane < k) r -= G[k * IALS_GP + lane] * xk;
  }
  return r;
}

// ---- one wave per row: base + weighted Gram + solve (deg < T2 lists) ----
__global__ __launch_bounds__(IALS_TB) void cf_ials_solve_kernel(
    uint32_t n, const V_ID* binlist, CFIalsArgs a) {
  __shared__ IalsLds lds;
  int lane = threadIdx.x;
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    V_ID v = binlist[i];
    E_ID b = a.row_ptr[v], e = a.row_ptr[v + 1];
    f32x4 acc[IALS_NT];
    ials_load_base(a.gram, lane, acc);
    float rhs = 0.0f;
    ials_gram_range(a, b, e, lane, lds.S, acc, &rhs);
    ials_dump_gram(lds.G, acc, lane, a.K, a.reg);
    ials_cholesky64(lds.G, lane, a.reg);
    float x = ials_solve64(lds.G, rhs, lane);
    if (lane < a.K) a.newv[(uint64_t)v * a.K + lane] = x;
    ials_lds_sync();  // G reads done before the next row's dump
  }
}

// ---- hub rows: one wave per chunk, partial Gram + rhs into ITS slot ----
// chunks: uint2[n2] {row, chunk index}, sorted by (row, chunk index); entry i
// owns slot i = f32[IALS_SLOT_F]: the 10 tiles in accumulator layout (upper
// triangle of the tile grid), then the 64 rhs values.
constexpr int IALS_CHUNK_TB = 128;  // 2 independent waves per workgroup

__global__ __launch_bounds__(IALS_CHUNK_TB) void cf_ials_chunk_kernel(
    uint32_t n2, const uint2* chunks, float* slots, CFIalsArgs a) {
  __shared__ float S2[IALS_CHUNK_TB / WAVE][IALS_TILE * IALS_SP];
  float* S = S2[threadIdx.x >> 6];
  int lane = threadIdx.x & (WAVE - 1);
  uint32_t wave = blockIdx.x * (IALS_CHUNK_TB / WAVE) + (threadIdx.x >> 6);
  uint32_t nwaves = gridDim.x * (IALS_CHUNK_TB / WAVE);
  for (uint32_t i = wave; i < n2; i += nwaves) {
    uint2 ent = chunks[i];
    E_ID b = a.row_ptr[ent.x] + (E_ID)ent.y * IALS_CHUNK;
    E_ID e = a.row_ptr[ent.x + 1];
    if (e > b + IALS_CHUNK) e = b + IALS_CHUNK;
    f32x4 acc[IALS_NT];
#pragma unroll
    for (int t = 0; t < IALS_NT; t++) acc[t] = {0, 0, 0, 0};
    float rhs = 0.0f;
    ials_gram_range(a, b, e, lane, S, acc, &rhs);
    float* slot = slots + (uint64_t)i * IALS_SLOT_F;
#pragma unroll
    for (int t = 0; t < IALS_NT; t++) ((f32x4*)slot)[t * WAVE + lane] = acc[t];
    slot[IALS_TILE_F + lane] = rhs;
  }
}

// ---- hub rows: sum the row's slots in chunk order, add the base, solve ----
// first: u32[nbig+1], hub i of `hubs` owns slots [first[i], first[i+1]).
__global__ __launch_bounds__(IALS_TB) void cf_ials_hub_solve_kernel(
    uint32_t nbig, const V_ID* hubs, const uint32_t* first,
    const float* slots, CFIalsArgs a) {
  __shared__ float G[IALS_K * IALS_GP];
  int lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nbig; i += gridDim.x) {
    V_ID v = hubs[i];
    f32x4 acc[IALS_NT];
#pragma unroll
    for (int t = 0; t < IALS_NT; t++) acc[t] = {0, 0, 0, 0};
    float rhs = 0.0f;
    for (uint32_t c = first[i]; c < first[i + 1]; c++) {
      const float* slot = slots + (uint64_t)c * IALS_SLOT_F;
#pragma unroll
      for (int t = 0; t < IALS_NT; t++)
        acc[t] += ((const f32x4*)slot)[t * WAVE + lane];
      rhs += slot[IALS_TILE_F + lane];
    }
    f32x4 base[IALS_NT];
    ials_load_base(a.gram, lane, base);
#pragma unroll
    for (int t = 0; t < IALS_NT; t++) acc[t] += base[t];
    ials_dump_gram(G, acc, lane, a.K, a.reg);
    ials_cholesky64(G, lane, a.reg);
    float x = ials_solve64(G, rhs, lane);
    if (lane < a.K) a.newv[(uint64_t)v * a.K + lane] = x;
    ials_lds_sync();
  }
}

#undef IALS_TI
#undef IALS_TJ

// Rows per workgroup (a multiple of the 32-row tile) and the grid for a side
// of n rows: at most IALS_GRAM_MAX_WG workgroups, none of them empty.
static void ials_gram_plan(uint32_t n, uint32_t* slab_rows, uint32_t* nwg) {
  uint32_t per = (uint32_t)(((uint64_t)n + IALS_GRAM_MAX_WG - 1) /
                            IALS_GRAM_MAX_WG);
  uint32_t slab = ((per + IALS_TILE - 1) / IALS_TILE) * IALS_TILE;
  if (slab == 0) slab = IALS_TILE;
  *slab_rows = slab;
  *nwg = (uint32_t)(((uint64_t)n + slab - 1) / slab);
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_cf_ials_gram_wgs(uint32_t n) {
  uint32_t slab, nwg;
  ials_gram_plan(n, &slab, &nwg);
  return nwg;
}

uint32_t lux_gpu_cf_ials_gram_wg_floats(void) { return IALS_TILE_F; }

uint32_t lux_gpu_cf_ials_slot_floats(void) { return IALS_SLOT_F; }

int lux_gpu_cf_ials_side_gram(uint64_t stream, const float* table, V_ID lo,
                              V_ID hi, int K, float* scratch, float* out) {
  if (K < 1 || K > IALS_K || hi < lo || !table || !out) return -1;
  hipStream_t s = (hipStream_t)stream;
  uint32_t n = hi - lo, slab, nwg;
  ials_gram_plan(n, &slab, &nwg);
  if (nwg && !scratch) return -1;
  if (nwg)
    hipLaunchKernelGGL(cf_ials_side_gram_kernel, dim3(nwg), dim3(IALS_TB), 0,
                       s, table + (uint64_t)lo * K, (uint64_t)n * K, K, slab,
                       scratch);
  hipLaunchKernelGGL(cf_ials_side_gram_reduce_kernel, dim3(IALS_NT),
                     dim3(IALS_RED_TB), 0, s, scratch, nwg, out);
  LUX_POST_LAUNCH(stream);
  return nwg ? 2 : 1;
}

int lux_gpu_cf_ials_phase(uint64_t stream, uint32_t n0, const V_ID* bin0,
                          uint32_t n1, const V_ID* bin1, uint32_t n2,
                          const uint2* chunks, uint32_t nbig,
                          const V_ID* hubs, const uint32_t* hub_first,
                          float* slots, const E_ID* row_ptr, const V_ID* col,
                          const WeightType* w, const float* oldv, float* newv,
                          int K, const float* side_gram, float alpha,
                          float reg) {
  if (K < 1 || K > IALS_K || !(alpha > 0.0f) || !(reg > 0.0f) || !side_gram)
    return -1;
  if (nbig && (!n2 || !chunks || !hubs || !hub_first || !slots)) return -1;
  hipStream_t s = (hipStream_t)stream;
  CFIalsArgs a{row_ptr, col, w, oldv, newv, side_gram, alpha, reg, K};
  int launches = 0;
  if (nbig) {
    uint32_t gw = (n2 + 1) / 2;
    hipLaunchKernelGGL(cf_ials_chunk_kernel,
                       dim3(gw > MAX_GRID ? MAX_GRID : gw),
                       dim3(IALS_CHUNK_TB), 0, s, n2, chunks, slots, a);
    hipLaunchKernelGGL(cf_ials_hub_solve_kernel,
                       dim3(nbig > MAX_GRID ? MAX_GRID : nbig), dim3(IALS_TB),
                       0, s, nbig, hubs, hub_first, slots, a);
    launches += 2;
  }
  const V_ID* lists[2] = {bin1, bin0};
  uint32_t counts[2] = {n1, n0};
  for (int c = 0; c < 2; c++) {
    if (!counts[c]) continue;
    hipLaunchKernelGGL(cf_ials_solve_kernel,
                       dim3(counts[c] > MAX_GRID ? MAX_GRID : counts[c]),
                       dim3(IALS_TB), 0, s, counts[c], lists[c], a);
    launches++;
  }
  LUX_POST_LAUNCH(stream);
  return launches;
}

}  // extern "C"
