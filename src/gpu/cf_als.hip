// Collaborative filtering — ALS sweep with MFMA Gram accumulation (gfx950).
//
// A second CF optimizer beside the reference-parity SGD sweep (cf.hip;
// reference colfilter_gpu.cu:32-104). One ALS sweep solves, per dst vertex,
// the exact normal equations the SGD sweep only steps toward:
//     (S^T S + lambda I) d = S^T w
// where S (deg x K) stacks the OLD src vectors of v's in-edges and w the
// edge weights. This is the SGD fixed point (grad = S^T(w - S d) - lambda d
// = 0), so both optimizers share semantics; ALS just converges in far fewer
// sweeps. Data access per sweep is identical to the SGD sweep (gather src
// vectors over in-edges, publish my slice), so the distributed exchange
// (all-gather of vector slices) is unchanged.
//
// MI355X mapping: the Gram matrix G = S^T S is the dense hot loop —
// K^2 * deg MACs per vertex — and is exactly MFMA-shaped. One 64-lane wave
// owns one dst vertex, stages ALS_TILE-edge tiles of src vectors in LDS,
// and accumulates the upper-triangular 16x16 tiles of G (K <= 64 -> 4x4
// tile grid, 10 upper tiles) with v_mfma_f32_16x16x4_f32: per 4-edge group,
// fragment f[t] = S[e0 + (lane>>4)][t*16 + (lane&15)] serves as operand A of
// tile-row t AND operand B of tile-col t (A[i][k]=S[e0+k][16ti+i],
// B[k][j]=S[e0+k][16tj+j] per the gfx950 f32 MFMA lane maps), so 4 LDS reads
// feed 10 MFMAs. fp32-input MFMA runs at the fp32 vector rate on gfx950 but
// packs the 64x64 outer-product accumulation into 40 accumulator VGPRs with
// no cross-lane reduction — the vector formulation needs either 64 serial
// wave reduces per 4 edges or an LDS round-trip per rank-1 update.
// The 64x64 SPD solve (Cholesky + two triangular solves) runs in the same
// wave on the LDS copy of G — no global scratch for the common case.
// Hub vertices (deg >= T2, bin2 chunk lists from pull.hip) accumulate
// partial G/rhs into global scratch with atomics, then a second kernel
// solves per hub.
#include "gpu_common.h"

namespace lux {

constexpr int ALS_K = 64;        // max latent rank of the MFMA path
constexpr int ALS_ROW = 65;      // LDS row pitch (bank-conflict pad)
constexpr int ALS_TILE = 32;     // edges staged per LDS tile (32: half the
                                 // LDS per wave -> ~2x waves/CU; same
                                 // occupancy lesson as cf.hip TILE=32)
constexpr int ALS_TB = 64;       // one wave per workgroup

using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ void als_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

struct CFAlsArgs {
  const E_ID* row_ptr;   // u64[vp+1] local
  const V_ID* col;       // u32[ep]
  const WeightType* w;   // i32[ep]
  const float* oldv;     // f32[nv*K]
  const __bf16* oldv_bf; // bf16 gather replica (nullable): halves the
                         // per-edge gather bytes AND the LLC footprint of
                         // the hot src-vector table on the bf16 Gram path
  float* newv;           // f32[vp*K] (pre-seeded with old slice)
  V_ID row_left;
  int K;                 // <= 64 here, <= 128 in the wide kernels below
};

struct AlsGramLds {
  float S[ALS_TILE * ALS_ROW];  // staged src vectors, row = edge
  float W[ALS_TILE];            // staged edge weights
};

// bf16 Gram path (default): the fp32 MFMA formulation above runs at the
// 155 TF f32 matrix rate and IS the sweep's bound (measured r2: the gram
// chunk kernel ~14 ms/sweep ~= the f32-MFMA issue floor). bf16 inputs
// with fp32 accumulation move the Gram onto v_mfma_f32_16x16x32_bf16
// (2075 TF): one K=32 MFMA per 16x16 tile per 32-edge LDS tile — 10
// MFMAs per tile instead of 80 — and the rhs folds from registers, so
// the LDS image shrinks to a transposed bf16 [dim][edge] panel whose
// fragments are single ds_read_b128s. LUX_ALS_F32=1 restores the exact
// fp32 path.
constexpr int ALS_BPITCH = 40;  // bf16 row pitch: 80 B = b128-aligned;
                                // 16-lane b128 groups land on distinct
                                // 4-bank runs (20 dwords/row, 20*16%64
                                // spread) -> conflict-free reads

struct alignas(16) AlsGramLdsBf {
  __bf16 S[ALS_K * ALS_BPITCH];  // TRANSPOSED: row = dim, col = edge
  float W[ALS_TILE];
};

struct AlsLds {
  union {
    AlsGramLds g;               // staging (S/W), fp32 path
    AlsGramLdsBf gb;            // staging, bf16 path
  };
  float G[ALS_K * ALS_ROW];     // Gram -> Cholesky factor (in place)
};

// ---- Gram accumulation over one vertex's edge range [b, e) ----
// acc[10] are the upper tiles (ti<=tj) in order (0,0)(0,1)(0,2)(0,3)
// (1,1)(1,2)(1,3)(2,2)(2,3)(3,3); rhs is lane=dim.
//
// Tile-level software pipeline: the NEXT tile's src-vector loads issue into
// registers (tmp[ALS_TILE]) right before the CURRENT tile's MFMA burst
// (~80 x 32-cycle issue at ALS_TILE=32), so their ~LLC latency hides under
// the matrix work; one LDS buffer suffices (regs -> LDS at tile start).

// Issue the whole tile's vector loads into registers (all outstanding).
__device__ __forceinline__ void als_vec_loads(const CFAlsArgs& a,
                                              uint32_t mycol, int rem,
                                              int lane,
                                              float tmp[ALS_TILE]) {
#pragma unroll
  for (int r = 0; r < ALS_TILE; r++) {
    uint32_t src = __shfl(mycol, r, WAVE);
    tmp[r] = (r < rem && lane < a.K)
                 ? a.oldv[(uint64_t)src * a.K + lane]
                 : 0.0f;
  }
}

__device__ __forceinline__ void als_gram_range(const CFAlsArgs& a, E_ID b,
                                               E_ID e, int lane,
                                               AlsGramLds* lds,
                                               f32x4 acc[10], float* rhs) {
  if (b >= e) return;
  int rem = (int)(e - b < ALS_TILE ? e - b : (E_ID)ALS_TILE);
  uint32_t mycol = 0;
  float myw = 0.0f;
  if (lane < rem) {
    mycol = a.col[b + lane];
    myw = (float)a.w[b + lane];
  }
  float tmp[ALS_TILE];
  als_vec_loads(a, mycol, rem, lane, tmp);
  for (E_ID t = b; t < e; t += ALS_TILE) {
    // stage the (prefetched) current tile
    if (lane < ALS_TILE) lds->W[lane] = myw;
#pragma unroll
    for (int r = 0; r < ALS_TILE; r++)
      lds->S[r * ALS_ROW + lane] = tmp[r];
    int rem_cur = rem;
    // prefetch next tile's col/weight now, vectors after the rhs pass
    E_ID t2 = t + ALS_TILE;
    bool more = t2 < e;
    uint32_t ncol = 0;
    float nw = 0.0f;
    if (more) {
      rem = (int)(e - t2 < ALS_TILE ? e - t2 : (E_ID)ALS_TILE);
      if (lane < rem) {
        ncol = a.col[t2 + lane];
        nw = (float)a.w[t2 + lane];
      }
    }
    int rem4 = (rem_cur + 3) & ~3;
    als_lds_sync();
    // rhs += sum_r w_r * S[r][lane] (4 independent LDS-read chains)
    float r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    int rr = 0;
    for (; rr + 4 <= rem_cur; rr += 4) {
      r0 += lds->W[rr] * lds->S[rr * ALS_ROW + lane];
      r1 += lds->W[rr + 1] * lds->S[(rr + 1) * ALS_ROW + lane];
      r2 += lds->W[rr + 2] * lds->S[(rr + 2) * ALS_ROW + lane];
      r3 += lds->W[rr + 3] * lds->S[(rr + 3) * ALS_ROW + lane];
    }
    for (; rr < rem_cur; rr++)
      r0 += lds->W[rr] * lds->S[rr * ALS_ROW + lane];
    *rhs += ((r0 + r1) + (r2 + r3));
    // issue the next tile's vector loads; they land under the MFMA burst
    if (more) {
      myw = nw;
      als_vec_loads(a, ncol, rem, lane, tmp);
      mycol = ncol;
    }
    // MFMA over 4-edge groups
    int erow = lane >> 4, ecol = lane & 15;
    for (int kk = 0; kk < rem4; kk += 4) {
      const float* base = &lds->S[(kk + erow) * ALS_ROW + ecol];
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
    als_lds_sync();  // tile consumed before next stage overwrites
  }
}

// ---- bf16 Gram accumulation (v_mfma_f32_16x16x32_bf16) ----
// A/B lane map of the 16x16x32 family: lane holds 8 contiguous-k
// elements, i (or j) = lane&15, k = (lane>>4)*8 + e (verified on
// hardware by tests/test_gpu_cf.py bf16-vs-f32 equivalence). One
// fragment per 16-dim block serves as A of tile-row t AND B of
// tile-col t, exactly like the f32 path's shared fragment.
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// bf16-replica gathers, DWORD-shaped: each lane loads one dword = TWO
// adjacent dims of one staged edge row (sub-dword gathers measured 2.5x
// below dword gather throughput — BENCHLOG r2.4; this keeps the halved
// bytes AND full-rate loads). Lanes 0..31 cover row r's 32 dim-pairs,
// lanes 32..63 row r+1's; 16 passes stage a 32-edge tile. The pair is
// split into the transposed [dim][edge] bf16 panel with two b16 writes;
// rhs folds from the staged panel. Requires even K.
__device__ __forceinline__ void als_stage_tile_bf2(const CFAlsArgs& a,
                                                   uint32_t mycol, int rem,
                                                   int lane, float myw,
                                                   AlsGramLdsBf* lds,
                                                   uint32_t pair[16]) {
  const uint32_t* tab = (const uint32_t*)a.oldv_bf;
  int half = lane >> 5;        // which of the pass's two rows
  int m = lane & 31;           // dim pair index (dims 2m, 2m+1)
  int kp = a.K >> 1;
#pragma unroll
  for (int pass = 0; pass < 16; pass++) {
    int r = pass * 2 + half;
    uint32_t src = __shfl(mycol, r, WAVE);
    pair[pass] = (r < rem && m < kp)
                     ? tab[(uint64_t)src * kp + m]
                     : 0u;
  }
  if (lane < ALS_TILE) lds->W[lane] = myw;
#pragma unroll
  for (int pass = 0; pass < 16; pass++) {
    int r = pass * 2 + half;
    lds->S[(uint32_t)(2 * m) * ALS_BPITCH + r] =
        ((const __bf16*)&pair[pass])[0];
    lds->S[(uint32_t)(2 * m + 1) * ALS_BPITCH + r] =
        ((const __bf16*)&pair[pass])[1];
  }
}

__device__ __forceinline__ void als_gram_range_bf2(const CFAlsArgs& a,
                                                   E_ID b, E_ID e,
                                                   int lane,
                                                   AlsGramLdsBf* lds,
                                                   f32x4 acc[10],
                                                   float* rhs) {
  if (b >= e) return;
  int rem = (int)(e - b < ALS_TILE ? e - b : (E_ID)ALS_TILE);
  uint32_t mycol = 0;
  float myw = 0.0f;
  if (lane < rem) {
    mycol = a.col[b + lane];
    myw = (float)a.w[b + lane];
  }
  for (E_ID t = b; t < e; t += ALS_TILE) {
    uint32_t pair[16];
    als_stage_tile_bf2(a, mycol, rem, lane, myw, lds, pair);
    int rem_cur = rem;
    // prefetch next tile's col/weight
    E_ID t2 = t + ALS_TILE;
    bool more = t2 < e;
    uint32_t ncol = 0;
    float nw = 0.0f;
    if (more) {
      rem = (int)(e - t2 < ALS_TILE ? e - t2 : (E_ID)ALS_TILE);
      if (lane < rem) {
        ncol = a.col[t2 + lane];
        nw = (float)a.w[t2 + lane];
      }
    }
    als_lds_sync();
    // rhs += sum_r w_r * S[r][lane], from the staged bf16 panel
    if (lane < a.K) {
      const __bf16* row = &lds->S[(uint32_t)lane * ALS_BPITCH];
      float r0 = 0, r1 = 0;
      for (int r = 0; r + 2 <= rem_cur; r += 2) {
        r0 += lds->W[r] * (float)row[r];
        r1 += lds->W[r + 1] * (float)row[r + 1];
      }
      if (rem_cur & 1) r0 += lds->W[rem_cur - 1] * (float)row[rem_cur - 1];
      *rhs += r0 + r1;
    }
    bf16x8 f[4];
    int m = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
      f[ti] = *(const bf16x8*)&lds->S[(uint32_t)(16 * ti + m) * ALS_BPITCH +
                                      g * 8];
    if (more) {  // next tile's gathers land under the MFMA burst... the
      myw = nw;  // bf2 path stages lazily per tile, so just roll state
      mycol = ncol;
    }
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[0], acc[0], 0,
                                                     0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[1], acc[1], 0,
                                                     0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[2], acc[2], 0,
                                                     0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[3], acc[3], 0,
                                                     0, 0);
    acc[4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1], f[1], acc[4], 0,
                                                     0, 0);
    acc[5] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1], f[2], acc[5], 0,
                                                     0, 0);
    acc[6] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1], f[3], acc[6], 0,
                                                     0, 0);
    acc[7] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[2], f[2], acc[7], 0,
                                                     0, 0);
    acc[8] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[2], f[3], acc[8], 0,
                                                     0, 0);
    acc[9] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[3], f[3], acc[9], 0,
                                                     0, 0);
    als_lds_sync();
  }
}

__device__ __forceinline__ void als_gram_range_bf16(const CFAlsArgs& a,
                                                    E_ID b, E_ID e,
                                                    int lane,
                                                    AlsGramLdsBf* lds,
                                                    f32x4 acc[10],
                                                    float* rhs) {
  if (b >= e) return;
  int rem = (int)(e - b < ALS_TILE ? e - b : (E_ID)ALS_TILE);
  uint32_t mycol = 0;
  float myw = 0.0f;
  if (lane < rem) {
    mycol = a.col[b + lane];
    myw = (float)a.w[b + lane];
  }
  float tmp[ALS_TILE];
  als_vec_loads(a, mycol, rem, lane, tmp);
  for (E_ID t = b; t < e; t += ALS_TILE) {
    // rhs += sum_r w_r * S[r][lane] — straight from registers (lane=dim
    // holds S[r][lane] in tmp[r]); exact fp32
#pragma unroll
    for (int r = 0; r < ALS_TILE; r++)
      *rhs += __shfl(myw, r, WAVE) * tmp[r];
    // stage TRANSPOSED bf16: my row = dim `lane`, cols = edges (pairs
    // packed into dword stores)
    uint32_t* row32 = (uint32_t*)&lds->S[(uint32_t)lane * ALS_BPITCH];
#pragma unroll
    for (int w = 0; w < ALS_TILE / 2; w++) {
      union {
        __bf16 h[2];
        uint32_t u;
      } pk;
      pk.h[0] = (__bf16)tmp[2 * w];
      pk.h[1] = (__bf16)tmp[2 * w + 1];
      row32[w] = pk.u;
    }
    // prefetch next tile's col/weight, then its vectors (they land
    // under the MFMA burst)
    E_ID t2 = t + ALS_TILE;
    bool more = t2 < e;
    uint32_t ncol = 0;
    float nw = 0.0f;
    if (more) {
      rem = (int)(e - t2 < ALS_TILE ? e - t2 : (E_ID)ALS_TILE);
      if (lane < rem) {
        ncol = a.col[t2 + lane];
        nw = (float)a.w[t2 + lane];
      }
    }
    als_lds_sync();
    bf16x8 f[4];
    int m = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < 4; ti++)
      f[ti] = *(const bf16x8*)&lds->S[(uint32_t)(16 * ti + m) * ALS_BPITCH +
                                      g * 8];
    if (more) {
      myw = nw;
      als_vec_loads(a, ncol, rem, lane, tmp);
      mycol = ncol;
    }
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[0], acc[0], 0,
                                                     0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[1], acc[1], 0,
                                                     0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[2], acc[2], 0,
                                                     0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0], f[3], acc[3], 0,
                                                     0, 0);
    acc[4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1], f[1], acc[4], 0,
                                                     0, 0);
    acc[5] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1], f[2], acc[5], 0,
                                                     0, 0);
    acc[6] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1], f[3], acc[6], 0,
                                                     0, 0);
    acc[7] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[2], f[2], acc[7], 0,
                                                     0, 0);
    acc[8] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[2], f[3], acc[8], 0,
                                                     0, 0);
    acc[9] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[3], f[3], acc[9], 0,
                                                     0, 0);
    als_lds_sync();  // tile consumed before the next stage overwrites
  }
}

// Scatter MFMA accumulators into the LDS Gram (mirroring the lower half)
// using the 16x16x4 C/D lane map: element (row=(lane>>4)*4+reg, col=lane&15).
__device__ __forceinline__ void als_dump_gram(AlsLds* lds, f32x4 acc[10],
                                              int lane, int K) {
  static constexpr int TI[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
  static constexpr int TJ[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};
  int row = (lane >> 4) * 4, col = lane & 15;
#pragma unroll
  for (int tidx = 0; tidx < 10; tidx++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      int gr = TI[tidx] * 16 + row + reg;
      int gc = TJ[tidx] * 16 + col;
      float v = acc[tidx][reg];
      lds->G[gr * ALS_ROW + gc] = v;
      if (TI[tidx] != TJ[tidx]) lds->G[gc * ALS_ROW + gr] = v;
    }
  }
  als_lds_sync();
  // regularizer + identity padding for unused dims (keeps G SPD for K<64)
  lds->G[lane * ALS_ROW + lane] =
      lane < K ? lds->G[lane * ALS_ROW + lane] + CF_LAMBDA : 1.0f;
  als_lds_sync();
}

// In-place lower Cholesky of the 64x64 LDS matrix (one wave; lane = row).
// Semi-definite handling: a (near-)rank-deficient Gram — e.g. the parity
// init makes sweep 1's Gram rank-1 with entries ~deg/K, whose
// elimination cancels later pivots to rounding noise (negative under
// bf16 inputs at NetFlix-scale hub degrees; sqrt -> NaN, and a naive
// lambda floor instead explodes the degenerate directions' step, which
// overflowed the NEXT sweep's Gram to inf/NaN). Deficient pivots are
// marked with a -1 sentinel, their column is zeroed, and the solve
// takes NO step along those directions — the exact-arithmetic
// pseudoinverse behaviour on the deficient subspace.
//
// The test is RELATIVE to the row's original diagonal as well as absolute:
// an exactly deficient direction leaves pivot = lambda + rounding noise,
// and the noise scales with the diagonal (fp32 accumulation of deg terms
// plus 64 elimination steps, ~1e-6 * G_kk measured as a few e-3 on a
// 40K..200K-degree hub whose sources span < K dims). Once that exceeds
// lambda an absolute test passes pivots that are pure noise, the solve
// divides by them, and — the hub Gram being summed with atomics — the
// factors came out different from run to run (|item| 35 or 400 from the
// same input, the larger ones diverging in the next sweep). Pivots below
// ALS_PIVOT_RTOL * G_kk carry no information in fp32 and take no step.
constexpr float ALS_PIVOT_RTOL = 1e-5f;

__device__ __forceinline__ void wave_cholesky64(float* G, int lane) {
  // lane k keeps row k's threshold; k is wave-uniform, so the loop fetches
  // it with a readlane instead of a second LDS access per step
  float thr = fmaxf((float)CF_LAMBDA * 0.5f,
                    ALS_PIVOT_RTOL * G[lane * ALS_ROW + lane]);
  for (int k = 0; k < ALS_K; k++) {
    float piv = G[k * ALS_ROW + k];
    bool ok = piv > __int_as_float(__builtin_amdgcn_readlane(
                        __float_as_int(thr), k));
    float dkk = ok ? sqrtf(piv) : 1.0f;
    float lik = (lane > k && ok) ? G[lane * ALS_ROW + k] / dkk : 0.0f;
    if (lane == k) G[k * ALS_ROW + k] = ok ? dkk : -1.0f;
    if (lane > k) G[lane * ALS_ROW + k] = lik;
    als_lds_sync();
    for (int j = k + 1; j <= lane; j++)
      G[lane * ALS_ROW + j] -= lik * G[j * ALS_ROW + k];
    als_lds_sync();
  }
}

// Solve L L^T d = rhs; rhs/result live lane=dim in a register.
// Sentinel (-1) pivots contribute zero (see wave_cholesky64).
__device__ __forceinline__ float wave_spd_solve64(const float* G, float r,
                                                  int lane) {
  for (int k = 0; k < ALS_K; k++) {  // forward: L y = r
    float lkk = G[k * ALS_ROW + k];
    float yk = lkk > 0.0f ? __shfl(r, k, WAVE) / lkk : 0.0f;
    if (lane == k) r = yk;
    else if (lane > k) r -= G[lane * ALS_ROW + k] * yk;
  }
  for (int k = ALS_K - 1; k >= 0; k--) {  // backward: L^T d = y
    float lkk = G[k * ALS_ROW + k];
    float dk = lkk > 0.0f ? __shfl(r, k, WAVE) / lkk : 0.0f;
    if (lane == k) r = dk;
    else if (lane < k) r -= G[k * ALS_ROW + lane] * dk;
  }
  return r;
}

// ---- one wave per vertex: gram + solve fused (deg < T2 bin lists) ----
// MODE selects the Gram path at compile time (0 = exact fp32, 1 = bf16
// MFMA with fp32 gathers, 2 = bf16 MFMA with dword-pair bf16 gathers):
// a runtime branch would co-inline every path and the register
// allocator sizes for their union (measured: +40 VGPRs, occupancy 2->1,
// 10.5 -> 18 ms/sweep with the branch never taken).
template <int MODE>
__global__ __launch_bounds__(ALS_TB) void cf_als_solve_kernel(
    uint32_t n, const V_ID* binlist, CFAlsArgs a) {
  __shared__ AlsLds lds;
  int lane = threadIdx.x;
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    V_ID v = binlist[i];
    E_ID b = a.row_ptr[v], e = a.row_ptr[v + 1];
    f32x4 acc[10];
#pragma unroll
    for (int t = 0; t < 10; t++) acc[t] = {0, 0, 0, 0};
    float rhs = 0.0f;
    if (MODE == 2)
      als_gram_range_bf2(a, b, e, lane, &lds.gb, acc, &rhs);
    else if (MODE == 1)
      als_gram_range_bf16(a, b, e, lane, &lds.gb, acc, &rhs);
    else
      als_gram_range(a, b, e, lane, &lds.g, acc, &rhs);
    als_dump_gram(&lds, acc, lane, a.K);
    wave_cholesky64(lds.G, lane);
    float d = wave_spd_solve64(lds.G, rhs, lane);
    if (lane < a.K) a.newv[(uint64_t)v * a.K + lane] = d;
    als_lds_sync();  // G reads done before next vertex's MFMA dump
  }
}

// ---- hub path: chunk-parallel Gram into global scratch ----
// gram_scratch: f32[nbig * 64 * 64] (upper-triangular elements only),
// rhs_scratch: f32[nbig * 64]; both pre-zeroed by the engine each sweep.
constexpr int ALS_CHUNK_TB = 128;  // 2 independent waves per workgroup

template <int MODE>
__global__ __launch_bounds__(ALS_CHUNK_TB) void cf_als_gram_chunk_kernel(
    uint32_t n2, const uint2* bin2, V_ID chunk_edges, const int* hubidx,
    float* gram_scratch, float* rhs_scratch, CFAlsArgs a) {
  union StageLds {
    AlsGramLds g;
    AlsGramLdsBf gb;
  };
  __shared__ StageLds lds2[ALS_CHUNK_TB / WAVE];
  StageLds& lds = lds2[threadIdx.x >> 6];
  int lane = threadIdx.x & (WAVE - 1);
  uint32_t wave = (blockIdx.x * (ALS_CHUNK_TB / WAVE)) + (threadIdx.x >> 6);
  uint32_t nwaves = gridDim.x * (ALS_CHUNK_TB / WAVE);
  for (uint32_t i = wave; i < n2; i += nwaves) {
    uint2 ent = bin2[i];
    V_ID v = ent.x;
    E_ID b = a.row_ptr[v] + (E_ID)ent.y * chunk_edges;
    E_ID e = a.row_ptr[v + 1];
    if (e > b + chunk_edges) e = b + chunk_edges;
    f32x4 acc[10];
#pragma unroll
    for (int t = 0; t < 10; t++) acc[t] = {0, 0, 0, 0};
    float rhs = 0.0f;
    if (MODE == 2)
      als_gram_range_bf2(a, b, e, lane, &lds.gb, acc, &rhs);
    else if (MODE == 1)
      als_gram_range_bf16(a, b, e, lane, &lds.gb, acc, &rhs);
    else
      als_gram_range(a, b, e, lane, &lds.g, acc, &rhs);
    int idx = hubidx[v];
    float* Gg = gram_scratch + (uint64_t)idx * ALS_K * ALS_K;
    atomicAdd(&rhs_scratch[(uint64_t)idx * ALS_K + lane], rhs);
    static constexpr int TI[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
    static constexpr int TJ[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};
    int row = (lane >> 4) * 4, col = lane & 15;
#pragma unroll
    for (int tidx = 0; tidx < 10; tidx++) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        int gr = TI[tidx] * 16 + row + reg;
        int gc = TJ[tidx] * 16 + col;
        if (gc >= gr) atomicAdd(&Gg[gr * ALS_K + gc], acc[tidx][reg]);
      }
    }
  }
}

// ---- hub path: per-vertex solve from global scratch ----
__global__ __launch_bounds__(ALS_TB) void cf_als_hub_solve_kernel(
    uint32_t nbig, const V_ID* bin2v, const float* gram_scratch,
    const float* rhs_scratch, CFAlsArgs a) {
  __shared__ AlsLds lds;
  int lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nbig; i += gridDim.x) {
    V_ID v = bin2v[i];
    const float* Gg = gram_scratch + (uint64_t)i * ALS_K * ALS_K;
    for (int r = 0; r < ALS_K; r++) {
      float x = Gg[r * ALS_K + lane];
      lds.G[r * ALS_ROW + lane] = x;  // upper half valid (lane >= r)
    }
    als_lds_sync();
    for (int r = 0; r < ALS_K; r++)  // mirror upper -> lower
      if (lane > r) lds.G[lane * ALS_ROW + r] = lds.G[r * ALS_ROW + lane];
    als_lds_sync();
    lds.G[lane * ALS_ROW + lane] =
        lane < a.K ? lds.G[lane * ALS_ROW + lane] + CF_LAMBDA : 1.0f;
    float rhs = rhs_scratch[(uint64_t)i * ALS_K + lane];
    als_lds_sync();
    wave_cholesky64(lds.G, lane);
    float d = wave_spd_solve64(lds.G, rhs, lane);
    if (lane < a.K) a.newv[(uint64_t)v * a.K + lane] = d;
    als_lds_sync();
  }
}

// ======================== 64 < K <= 128 (wide path) ========================
// Separate kernels, launched only for K > 64; the kernels above are not
// parameterised over the rank and compile exactly as before.
//
// One 128-thread workgroup (two waves) owns one dst vertex: thread = dim =
// Cholesky row, so one edge's source vector is still one coalesced read
// (128 x 4 B = 512 B across the workgroup). The Gram is an 8x8 grid of
// 16x16 tiles, 36 of them on or above the diagonal, split 18/18 between
// the waves (72 accumulator registers each). Both waves run the SAME
// unrolled tile list over LOCAL block numbers 0..7; a wave-dependent block
// permutation (als2_blk) turns them into global 16-dim blocks, so no
// accumulator is ever indexed by a runtime value:
//   local tiles   the 10 upper tiles among blocks {0..3}, and
//                 (x, 4+x), (x, 4+(x+1)%4) for x = 0..3
//   wave 0        local == global: upper tiles of dims 0..63 plus two
//                 diagonals of the 4x4 cross panel
//   wave 1        local b -> b+4 (b < 4), (b-3)&3 (b >= 4): the tiles of
//                 dims 64..127 plus the cross panel's other two diagonals
//                 (as their transposes; the Gram is symmetric)
// Each wave reads all 8 fragments per k-step for its 18 MFMAs.
//
// LDS: the factor lives PACKED lower-triangular, L[i][j] at i(i+1)/2 + j,
// 129 rows (row 128 = rhs, see als2_factor): 33.5 KB instead of the 66 KB
// of a padded square, and the staging tile ALIASES it (the Gram sits in
// accumulators until the last tile is consumed) -> 34.5 KB static, so LDS
// admits 4 workgroups per CU (the Gram kernels' registers, ~250 VGPRs +
// accumulators at one wave per SIMD, allow 2; a tighter budget spills, and
// these kernels must not use scratch). Triangular numbers are a bijection mod 2^m,
// so the 32 lanes of a ds_read_b32 group walking one column (rows i0..i0+31,
// i0 a multiple of 32) hit 32 distinct banks; row reads are contiguous.
constexpr int ALS2_K = 128;       // KP: padded rank and hub scratch pitch
constexpr int ALS2_TB = 128;      // thread = dim = Cholesky row (2 waves)
constexpr int ALS2_NT = 18;       // tiles per wave
constexpr int ALS2_SPITCH = 144;  // fp32 stage pitch: 16 mod 32 banks, so a
                                  // fragment read (2 edge rows x 16 dims per
                                  // 32-lane group) is conflict-free
constexpr int ALS2_LSIZE = (ALS2_K + 1) * (ALS2_K + 2) / 2;

__host__ __device__ constexpr int als2_tri(int i) {
  return i * (i + 1) / 2;
}

__device__ __forceinline__ int als2_blk(int wv, int b) {
  return wv ? (b < 4 ? b + 4 : ((b - 3) & 3)) : b;
}

struct alignas(16) AlsWideStage {
  union {
    float S[ALS_TILE * ALS2_SPITCH];   // fp32: row = edge
    __bf16 Sb[ALS2_K * ALS_BPITCH];    // bf16, TRANSPOSED: row = dim
  };
};

struct AlsWideLds {
  union {
    AlsWideStage st;
    float L[ALS2_LSIZE];  // packed lower Gram -> factor; row 128 = rhs -> y
  };
  float thr[ALS2_K];      // per-row pivot thresholds
  float diag[ALS2_K];     // factor diagonal (-1 = deficient pivot)
};

#define ALS2_TILES_A {0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 0, 0, 1, 1, 2, 2, 3, 3}
#define ALS2_TILES_B {0, 1, 2, 3, 1, 2, 3, 2, 3, 3, 4, 5, 5, 6, 6, 7, 7, 4}

// Gram accumulation over edges [b, e) (workgroup-uniform). Same tile-level
// software pipeline as als_gram_range: the next tile's gathers issue into
// registers right before the current tile's MFMA burst. rhs folds from
// registers in exact fp32 in both modes (tid = dim holds S[r][tid]).
template <int MODE>
__device__ __forceinline__ void als2_gram_range(const CFAlsArgs& a, E_ID b,
                                                E_ID e, int tid,
                                                AlsWideStage* st,
                                                f32x4 acc[ALS2_NT],
                                                float* rhs) {
  static constexpr int TA[ALS2_NT] = ALS2_TILES_A;
  static constexpr int TB[ALS2_NT] = ALS2_TILES_B;
  if (b >= e) return;
  int lane = tid & (WAVE - 1);
  int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int rem = (int)(e - b < ALS_TILE ? e - b : (E_ID)ALS_TILE);
  uint32_t mycol = 0;
  float myw = 0.0f;
  if (lane < rem) {  // each wave keeps its own copy for the shuffles
    mycol = a.col[b + lane];
    myw = (float)a.w[b + lane];
  }
  float tmp[ALS_TILE];
  als_vec_loads(a, mycol, rem, tid, tmp);
  int m = lane & 15, g = lane >> 4;
  int fo[8];  // per-fragment LDS offsets of this wave's blocks
#pragma unroll
  for (int t = 0; t < 8; t++)
    fo[t] = MODE == 1 ? (16 * als2_blk(wv, t) + m) * ALS_BPITCH + g * 8
                      : g * ALS2_SPITCH + 16 * als2_blk(wv, t) + m;
  for (E_ID t = b; t < e; t += ALS_TILE) {
    float r0 = 0.0f, r1 = 0.0f;
#pragma unroll
    for (int r = 0; r < ALS_TILE; r += 2) {
      r0 += __shfl(myw, r, WAVE) * tmp[r];
      r1 += __shfl(myw, r + 1, WAVE) * tmp[r + 1];
    }
    *rhs += r0 + r1;
    int rem_cur = rem;
    if (MODE == 1) {
      uint32_t* row32 = (uint32_t*)&st->Sb[(uint32_t)tid * ALS_BPITCH];
#pragma unroll
      for (int w = 0; w < ALS_TILE / 2; w++) {
        union {
          __bf16 h[2];
          uint32_t u;
        } pk;
        pk.h[0] = (__bf16)tmp[2 * w];
        pk.h[1] = (__bf16)tmp[2 * w + 1];
        row32[w] = pk.u;
      }
    } else {
#pragma unroll
      for (int r = 0; r < ALS_TILE; r++)
        st->S[r * ALS2_SPITCH + tid] = tmp[r];
    }
    // prefetch next tile's col/weight, then its vectors
    E_ID t2 = t + ALS_TILE;
    bool more = t2 < e;
    uint32_t ncol = 0;
    float nw = 0.0f;
    if (more) {
      rem = (int)(e - t2 < ALS_TILE ? e - t2 : (E_ID)ALS_TILE);
      if (lane < rem) {
        ncol = a.col[t2 + lane];
        nw = (float)a.w[t2 + lane];
      }
    }
    __syncthreads();
    if (MODE == 1) {
      bf16x8 f[8];
#pragma unroll
      for (int i = 0; i < 8; i++) f[i] = *(const bf16x8*)&st->Sb[fo[i]];
      if (more) {
        myw = nw;
        als_vec_loads(a, ncol, rem, tid, tmp);
        mycol = ncol;
      }
#pragma unroll
      for (int i = 0; i < ALS2_NT; i++)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[TA[i]], f[TB[i]],
                                                         acc[i], 0, 0, 0);
    } else {
      if (more) {
        myw = nw;
        als_vec_loads(a, ncol, rem, tid, tmp);
        mycol = ncol;
      }
      int rem4 = (rem_cur + 3) & ~3;  // rows >= rem_cur are staged zeros
      for (int kk = 0; kk < rem4; kk += 4) {
        const float* base = &st->S[kk * ALS2_SPITCH];
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; i++) f[i] = base[fo[i]];
#pragma unroll
        for (int i = 0; i < ALS2_NT; i++)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[TA[i]], f[TB[i]],
                                                        acc[i], 0, 0, 0);
      }
    }
    __syncthreads();  // tile consumed before the next stage overwrites
  }
}

// In-place factor + solve of the packed 128-row system; every thread of the
// workgroup calls it. On entry L holds the lower triangle of G (regulariser
// and identity padding applied, thr[] set) and row 128 holds the rhs.
//
// Left-looking Cholesky: step k finishes COLUMN k,
//   L[i][k] = (G[i][k] - sum_{j<k} L[i][j] L[k][j]) / L[k][k],
// a read-only dot product per row (four independent chains) and ONE
// workgroup barrier per step, where the 64-row right-looking update would
// need two barriers and an LDS read-modify-write per element. Every thread
// folds the pivot's own sum of squares from the row-k values it reads
// anyway, so the pivot test needs no broadcast. Thread 0 has no column work
// after step 0 and carries the rhs as row 128: the same recurrence leaves
// y = L^-1 rhs there, which is the forward solve.
//
// The pivot rule is wave_cholesky64's: threshold max(lambda/2,
// ALS_PIVOT_RTOL * G_kk) from the diagonal BEFORE elimination; a deficient
// pivot gets the -1 sentinel, a zeroed column (y_k included) and no step in
// the backward solve. The factor diagonal goes to diag[] so step k never
// writes an element its own readers still need.
//
// The backward solve L^T d = y runs in wave 0 alone with two dims per lane
// (lane, lane + 64): pivots broadcast by shuffle, no barriers.
__device__ __forceinline__ void als2_factor_solve(AlsWideLds* lds, int tid,
                                                  const CFAlsArgs& a,
                                                  V_ID v) {
  float* L = lds->L;
  int row = tid == 0 ? ALS2_K : tid;
  float* Li = &L[als2_tri(row)];
  for (int k = 0; k < ALS2_K; k++) {
    if (row >= k) {
      const float* Lk = &L[als2_tri(k)];
      // 8 elements per trip, all 16 LDS reads issued before the first FMA:
      // the loop is latency-bound, not throughput-bound
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
      float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
      for (int j = 0; j < k; j += 8) {
        float kv[8], lv[8];
        if (j + 8 <= k) {
#pragma unroll
          for (int u = 0; u < 8; u++) kv[u] = Lk[j + u];
#pragma unroll
          for (int u = 0; u < 8; u++) lv[u] = Li[j + u];
        } else {  // ragged tail: elements at or past k count as zero
#pragma unroll
          for (int u = 0; u < 8; u++) kv[u] = j + u < k ? Lk[j + u] : 0.0f;
#pragma unroll
          for (int u = 0; u < 8; u++) lv[u] = j + u < k ? Li[j + u] : 0.0f;
        }
        d0 += kv[0] * kv[0] + kv[4] * kv[4];
        d1 += kv[1] * kv[1] + kv[5] * kv[5];
        d2 += kv[2] * kv[2] + kv[6] * kv[6];
        d3 += kv[3] * kv[3] + kv[7] * kv[7];
        s0 += lv[0] * kv[0] + lv[4] * kv[4];
        s1 += lv[1] * kv[1] + lv[5] * kv[5];
        s2 += lv[2] * kv[2] + lv[6] * kv[6];
        s3 += lv[3] * kv[3] + lv[7] * kv[7];
      }
      float piv = Lk[k] - ((d0 + d1) + (d2 + d3));
      bool ok = piv > lds->thr[k];
      float dkk = ok ? sqrtf(piv) : 1.0f;
      if (row > k)
        Li[k] = ok ? (Li[k] - ((s0 + s1) + (s2 + s3))) / dkk : 0.0f;
      if (tid == k) lds->diag[k] = ok ? dkk : -1.0f;
    }
    __syncthreads();
  }
  if (tid < WAVE) {
    const float* y = &L[als2_tri(ALS2_K)];
    float r0 = y[tid], r1 = y[tid + WAVE];
    for (int k = ALS2_K - 1; k >= WAVE; k--) {
      float lkk = lds->diag[k];
      float dk = lkk > 0.0f ? __shfl(r1, k - WAVE, WAVE) / lkk : 0.0f;
      const float* Lk = &L[als2_tri(k)];
      if (tid + WAVE == k) r1 = dk;
      else if (tid + WAVE < k) r1 -= Lk[tid + WAVE] * dk;
      r0 -= Lk[tid] * dk;
    }
    for (int k = WAVE - 1; k >= 0; k--) {
      float lkk = lds->diag[k];
      float dk = lkk > 0.0f ? __shfl(r0, k, WAVE) / lkk : 0.0f;
      if (tid == k) r0 = dk;
      else if (tid < k) r0 -= L[als2_tri(k) + tid] * dk;
    }
    if (tid < a.K) a.newv[(uint64_t)v * a.K + tid] = r0;
    if (tid + WAVE < a.K) a.newv[(uint64_t)v * a.K + tid + WAVE] = r1;
  }
  __syncthreads();  // L is free for the next vertex's stage / load
}

// Regulariser, identity padding for dims >= K, thresholds and the rhs row.
// Each thread touches only its own diagonal; the caller has made the
// triangle visible.
__device__ __forceinline__ void als2_finish_gram(AlsWideLds* lds, int tid,
                                                 int K, float rhs) {
  float d = tid < K ? lds->L[als2_tri(tid) + tid] + (float)CF_LAMBDA : 1.0f;
  lds->L[als2_tri(tid) + tid] = d;
  lds->thr[tid] = fmaxf((float)CF_LAMBDA * 0.5f, ALS_PIVOT_RTOL * d);
  lds->L[als2_tri(ALS2_K) + tid] = rhs;
  __syncthreads();
}

// ---- one workgroup per vertex: gram + solve fused (deg < T2 bin lists) ----
template <int MODE>
__global__ __launch_bounds__(ALS2_TB) void cf_als_wide_solve_kernel(
    uint32_t n, const V_ID* binlist, CFAlsArgs a) {
  static constexpr int TA[ALS2_NT] = ALS2_TILES_A;
  static constexpr int TB[ALS2_NT] = ALS2_TILES_B;
  __shared__ AlsWideLds lds;
  int tid = threadIdx.x;
  int lane = tid & (WAVE - 1);
  int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
    V_ID v = binlist[i];
    E_ID b = a.row_ptr[v], e = a.row_ptr[v + 1];
    f32x4 acc[ALS2_NT];
#pragma unroll
    for (int t = 0; t < ALS2_NT; t++) acc[t] = {0, 0, 0, 0};
    float rhs = 0.0f;
    als2_gram_range<MODE>(a, b, e, tid, &lds.st, acc, &rhs);
    // accumulators -> packed lower triangle (C/D map of both MFMA shapes:
    // row = (lane>>4)*4 + reg, col = lane&15); a diagonal tile keeps its
    // lower half only
    int row = (lane >> 4) * 4, col = lane & 15;
#pragma unroll
    for (int t = 0; t < ALS2_NT; t++) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        int gr = als2_blk(wv, TA[t]) * 16 + row + reg;
        int gc = als2_blk(wv, TB[t]) * 16 + col;
        int hi = gr > gc ? gr : gc, lo = gr > gc ? gc : gr;
        if (TA[t] != TB[t] || gr >= gc)
          lds.L[als2_tri(hi) + lo] = acc[t][reg];
      }
    }
    __syncthreads();
    als2_finish_gram(&lds, tid, a.K, rhs);
    als2_factor_solve(&lds, tid, a, v);
  }
}

// ---- hub path: one workgroup per 8192-edge chunk, Gram into scratch ----
// gram_scratch: f32[nbig * 128 * 128], upper triangle only, rows/cols >= K
// never touched (stay zero); rhs_scratch: f32[nbig * 128].
template <int MODE>
__global__ __launch_bounds__(ALS2_TB) void cf_als_wide_gram_chunk_kernel(
    uint32_t n2, const uint2* bin2, V_ID chunk_edges, const int* hubidx,
    float* gram_scratch, float* rhs_scratch, CFAlsArgs a) {
  static constexpr int TA[ALS2_NT] = ALS2_TILES_A;
  static constexpr int TB[ALS2_NT] = ALS2_TILES_B;
  __shared__ AlsWideStage st;
  int tid = threadIdx.x;
  int lane = tid & (WAVE - 1);
  int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (uint32_t i = blockIdx.x; i < n2; i += gridDim.x) {
    uint2 ent = bin2[i];
    V_ID v = ent.x;
    E_ID b = a.row_ptr[v] + (E_ID)ent.y * chunk_edges;
    E_ID e = a.row_ptr[v + 1];
    if (e > b + chunk_edges) e = b + chunk_edges;
    f32x4 acc[ALS2_NT];
#pragma unroll
    for (int t = 0; t < ALS2_NT; t++) acc[t] = {0, 0, 0, 0};
    float rhs = 0.0f;
    als2_gram_range<MODE>(a, b, e, tid, &st, acc, &rhs);
    int idx = hubidx[v];
    float* Gg = gram_scratch + (uint64_t)idx * ALS2_K * ALS2_K;
    if (tid < a.K) atomicAdd(&rhs_scratch[(uint64_t)idx * ALS2_K + tid], rhs);
    int row = (lane >> 4) * 4, col = lane & 15;
#pragma unroll
    for (int t = 0; t < ALS2_NT; t++) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        int gr = als2_blk(wv, TA[t]) * 16 + row + reg;
        int gc = als2_blk(wv, TB[t]) * 16 + col;
        int hi = gr > gc ? gr : gc, lo = gr > gc ? gc : gr;
        if ((TA[t] != TB[t] || gc >= gr) && hi < a.K)
          atomicAdd(&Gg[lo * ALS2_K + hi], acc[t][reg]);
      }
    }
  }
}

// ---- hub path: per-vertex solve from global scratch ----
__global__ __launch_bounds__(ALS2_TB) void cf_als_wide_hub_solve_kernel(
    uint32_t nbig, const V_ID* bin2v, const float* gram_scratch,
    const float* rhs_scratch, CFAlsArgs a) {
  __shared__ AlsWideLds lds;
  int tid = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nbig; i += gridDim.x) {
    V_ID v = bin2v[i];
    const float* Gg = gram_scratch + (uint64_t)i * ALS2_K * ALS2_K;
    // scratch row r, column tid (upper, tid >= r) -> packed L[tid][r]:
    // coalesced reads, each thread fills its own packed row
    for (int r = 0; r <= tid; r++)
      lds.L[als2_tri(tid) + r] = Gg[r * ALS2_K + tid];
    als2_finish_gram(&lds, tid, a.K,
                     rhs_scratch[(uint64_t)i * ALS2_K + tid]);
    als2_factor_solve(&lds, tid, a, v);
  }
}

#undef ALS2_TILES_A
#undef ALS2_TILES_B

}  // namespace lux

using namespace lux;

extern "C" {

// One ALS sweep over my partition. Reuses the pull.hip degree-bin lists;
// hubidx maps a hub vertex (local id) to its scratch slot [0, nbig).
// gram_scratch/rhs_scratch must be zeroed before each sweep when nbig > 0.
// K selects the scratch pitch KP: 64 for K <= 64 (gram nbig*64*64, rhs
// nbig*64), 128 for 64 < K <= 128 (gram nbig*128*128, rhs nbig*128). K < 1
// or K > 128 aborts before anything is launched.
void lux_gpu_cf_als_iter(uint64_t stream, uint32_t n0, const V_ID* bin0,
                         uint32_t n1, const V_ID* bin1, uint32_t n2,
                         const uint2* bin2, uint32_t nbig, const V_ID* bin2v,
                         const int* hubidx, float* gram_scratch,
                         float* rhs_scratch, const E_ID* row_ptr,
                         const V_ID* col, const WeightType* w,
                         const float* oldv,
                         const uint16_t* oldv_bf /*nullable*/, float* newv,
                         V_ID row_left, int K) {
  hipStream_t s = (hipStream_t)stream;
  if (K < 1 || K > ALS2_K) {
    fprintf(stderr, "lux_gpu_cf_als_iter: K = %d outside [1, %d]\n", K,
            ALS2_K);
    abort();
  }
  CFAlsArgs a{row_ptr, col, w, oldv, (const __bf16*)oldv_bf, newv, row_left,
              K};
  if (K > ALS_K) {
    // Wide path (KP = 128 scratch pitch). Same per-class defaults as below;
    // the bf16 gather replica (mode 2) is not extended past K = 64, so
    // oldv_bf is ignored here.
    a.oldv_bf = nullptr;
    bool f32 = getenv("LUX_ALS_F32") != nullptr;
    int mode = !f32 && getenv("LUX_ALS_BF16") ? 1 : 0;
    int chunk_mode = f32 ? 0 : 1;
    if (nbig) {
      dim3 grid(n2 > MAX_GRID ? MAX_GRID : n2);
      if (chunk_mode == 1)
        hipLaunchKernelGGL(cf_als_wide_gram_chunk_kernel<1>, grid,
                           dim3(ALS2_TB), 0, s, n2, bin2, (V_ID)8192, hubidx,
                           gram_scratch, rhs_scratch, a);
      else
        hipLaunchKernelGGL(cf_als_wide_gram_chunk_kernel<0>, grid,
                           dim3(ALS2_TB), 0, s, n2, bin2, (V_ID)8192, hubidx,
                           gram_scratch, rhs_scratch, a);
      hipLaunchKernelGGL(cf_als_wide_hub_solve_kernel,
                         dim3(nbig > MAX_GRID ? MAX_GRID : nbig),
                         dim3(ALS2_TB), 0, s, nbig, bin2v, gram_scratch,
                         rhs_scratch, a);
    }
    const V_ID* lists[2] = {bin1, bin0};
    uint32_t counts[2] = {n1, n0};
    for (int c = 0; c < 2; c++) {
      uint32_t n = counts[c];
      if (!n) continue;
      dim3 grid(n > MAX_GRID ? MAX_GRID : n);
      if (mode == 1)
        hipLaunchKernelGGL(cf_als_wide_solve_kernel<1>, grid, dim3(ALS2_TB),
                           0, s, n, lists[c], a);
      else
        hipLaunchKernelGGL(cf_als_wide_solve_kernel<0>, grid, dim3(ALS2_TB),
                           0, s, n, lists[c], a);
    }
    LUX_POST_LAUNCH(stream);
    return;
  }
  // Mode defaults are PER KERNEL CLASS. Fused per-row solves: exact fp32
  // Gram (16x16x4). bf16 Gram noise (~0.4% of ||G||) swamps sigma_min for
  // moderate-degree rows during alternation — measured: item factors jump
  // 0.32 -> 409 after one bf16 half-sweep and the feedback diverges to
  // 1e13 loss. Chunk/hub Gram (deg >= T2 = 2048): bf16 16x16x32 MFMA
  // stays the default — averaging over >= 2048 sources keeps ||G|| /
  // sigma_min well above the bf16 noise floor, and that is where the
  // NetFlix-shaped item volume (avg item degree ~5.7K) lives.
  // LUX_ALS_F32=1 forces fp32 everywhere; LUX_ALS_BF16=1 forces bf16 for
  // the fused solves too; mode 2 = dword-pair bf16 gathers (only when
  // the engine passed a bf16 replica; LUX_ALS_BF_GATHER experiment).
  int mode = getenv("LUX_ALS_F32")
                 ? 0
                 : (oldv_bf ? 2 : (getenv("LUX_ALS_BF16") ? 1 : 0));
  int chunk_mode = getenv("LUX_ALS_F32") ? 0 : (oldv_bf ? 2 : 1);
#define LUX_ALS_LAUNCH(K_, GRID_, N_, LIST_)                                  do {                                                                          if (mode == 2)                                                                hipLaunchKernelGGL(K_<2>, GRID_, dim3(ALS_TB), 0, s, N_, LIST_, a);       else if (mode == 1)                                                           hipLaunchKernelGGL(K_<1>, GRID_, dim3(ALS_TB), 0, s, N_, LIST_, a);       else                                                                          hipLaunchKernelGGL(K_<0>, GRID_, dim3(ALS_TB), 0, s, N_, LIST_, a);     } while (0)
  if (nbig) {
    uint32_t gw = (n2 + 1) / 2;
    dim3 grid(gw > MAX_GRID ? MAX_GRID : gw);
    int mode = chunk_mode;  // hub Gram keeps bf16 (see above)
    if (mode == 2)
      hipLaunchKernelGGL(cf_als_gram_chunk_kernel<2>, grid,
                         dim3(ALS_CHUNK_TB), 0, s, n2, bin2, (V_ID)8192,
                         hubidx, gram_scratch, rhs_scratch, a);
    else if (mode == 1)
      hipLaunchKernelGGL(cf_als_gram_chunk_kernel<1>, grid,
                         dim3(ALS_CHUNK_TB), 0, s, n2, bin2, (V_ID)8192,
                         hubidx, gram_scratch, rhs_scratch, a);
    else
      hipLaunchKernelGGL(cf_als_gram_chunk_kernel<0>, grid,
                         dim3(ALS_CHUNK_TB), 0, s, n2, bin2, (V_ID)8192,
                         hubidx, gram_scratch, rhs_scratch, a);
    hipLaunchKernelGGL(cf_als_hub_solve_kernel,
                       dim3(nbig > MAX_GRID ? MAX_GRID : nbig), dim3(ALS_TB),
                       0, s, nbig, bin2v, gram_scratch, rhs_scratch, a);
  }
  if (n1)
    LUX_ALS_LAUNCH(cf_als_solve_kernel, dim3(n1 > MAX_GRID ? MAX_GRID : n1),
                   n1, bin1);
  if (n0)
    LUX_ALS_LAUNCH(cf_als_solve_kernel, dim3(n0 > MAX_GRID ? MAX_GRID : n0),
                   n0, bin0);
#undef LUX_ALS_LAUNCH
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
