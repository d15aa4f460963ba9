// k-truss decomposition by decremental synchronous peeling: adjacency fill,
// edge classification, one intersection body in three modes (support, peel,
// check), level scan and single-workgroup round fusion for gfx950.
// No reference equivalent.
//
// Input (lux_amd/truss_engine.py): the id-order DAG of tc_engine.orient,
// optr u64[nv+1] / oadj u32[m]; DAG arc e IS edge e, the (lo << 32) | hi
// order of the definition. The engine sorts the 2m directed keys (a << 32) |
// b of both directions of every arc; truss_adj_fill_kernel turns a run of
// them into the full adjacency aptr u64[nv+1] / aadj u32[2m] / aeid u32[2m]
// (rows strictly ascending over the whole row; aeid the edge id of every
// entry, the lower bound of max(a, b) in DAG row min(a, b)) and elo u32[m],
// the row of every arc (ehi is oadj). Every index into aadj / aeid is
// 64-bit.
//
// The body: the triangles through edge e = {u, v} are N(u) & N(v). It
// ALWAYS iterates the shorter row S and searches the longer row L, so an
// edge costs min(d_u, d_v) lower bounds of log d_L steps. A hit at w gives
// the two other edges without another search: aeid of the iterated entry
// (the edge {s, w}) and aeid at the found position (the edge {l, w}); the
// searches therefore return positions (truss_lb4, the position-returning
// sibling of tc_find4). What happens at a hit is the mode (truss_hit):
//   SUPPORT  count it; the count is stored to sup[e] by the one wave that
//            owns the edge (no atomic), or added per chunk for a hub edge;
//   PEEL     decrement the surviving edges of the triangle, see below;
//   CHECK    count a = hits whose two edges have trussness >= t = truss[e]
//            and b = those where both have >= t + 1. A violation is
//            a < t - 2, b >= t - 1 or t outside [2, support + 2]:
//            necessary, NOT sufficient (exactness rests on the tests
//            against the CPU oracle).
//
// Three roles, from the two degrees of the edge (truss_role):
//   lane-held  d_L <= 64: a wave takes four list entries; their rows are
//              loaded together, L one entry per lane (padded with
//              0xFFFFFFFF, its edge ids in a second register), S one key
//              per lane, and each edge is a six-step lower bound through
//              __shfl plus two shuffles for the hit. No LDS, no barrier, no
//              dependent global read. (Four 16-lane groups, the tc_small
//              split, would each need their own table: a group cannot read
//              another register of the source lane with one shuffle, so
//              that split costs four shuffles per step; one edge at a time
//              over all 64 lanes costs one, and the four edges' loads are
//              still in flight together.)
//   wave       d_S <= hub: a wave per edge, lanes striding over S, four
//              keys per lane in a lockstep branch-free lower bound in
//              global memory;
//   hub        d_S > hub: ceil(d_S / hub) items {edge, chunk} in hubq, one
//              workgroup per item. The workgroup copies a fence table into
//              LDS, `fence` evenly spaced entries of L (the last entry of
//              every interval; the row itself if d_L <= fence): a key's
//              first log2(fence) steps run in LDS and only the last
//              ceil(log2(d_L / fence)) go to global memory, inside one
//              fence interval.
// For SUPPORT and CHECK truss_classify_kernel writes the lists once (lane
// edges from the front of one u32[m] list, wave edges from its back, hub
// items into their own hubq); for PEEL the role is taken when an edge is
// queued.
//
// State of a decomposition:
//   sup   i32[m]  the current support; signed, because concurrent
//                 decrements take a queued edge transiently below s. A
//                 removed edge rests at the level it left at.
//   order u32[m]  append-only: every edge exactly once, when it is found
//                 removable. A round is a range [head, tail) of it.
//   pos   u32[m]  the index of an edge in order, 0xFFFFFFFF before.
//   truss u32[m]  s + 2, written when the edge's round runs.
//   hubq  u32 pairs {edge, chunk}, append-only, filled when a hub edge is
//                 queued.
//   meta  u32[8]  TM_TAIL / TM_HUBTAIL: the append cursors; TM_MIN: the
//                 scan's minimum; TM_FUSED / TM_HEAD: what the tail kernel
//                 did; TM_LANE / TM_WAVE: the classification's counters.
//
// Level s (every alive edge has sup >= s when it starts): the scan appends
// every edge with sup == s and folds min{sup : sup > s}. A round [head,
// tail) writes truss[e] = s + 2 and handles each triangle (e, e1, e2):
//   pos[e1] < head or pos[e2] < head: it went in an earlier round, skip;
//   both in [head, tail): nothing is left to decrement;
//   exactly one, say e1, in [head, tail): e and e1 both find the triangle,
//     the smaller id of the two decrements e2, so it happens once;
//   neither (positions >= tail and "not queued" are indistinguishable on
//     purpose: an edge appended during this round is alive in it): e
//     decrements both.
// The decrement of x is a returning atomicSub: the one that returns s + 1
// appends x (wave-aggregated: a ballot, one atomic on the cursor per wave,
// then order[slot] = x and pos[x] = slot); one that returns <= s found x
// queued already and adds its unit back.
// Ownership: an alive, unqueued x has sup > s and no pending put-back, so
// its count is exact; the values it passes on the way down are distinct
// until s + 1, and a put-back only lifts a value <= s - 1 to at most s, so
// exactly one decrement ever returns s + 1. Every edge therefore enters
// order exactly once: order (u32[m]) and hubq (sized by the classification,
// which sums the same ceil(d_S / hub) over the same edges) cannot overflow
// and there is no double buffering; the appends are bounds-checked all the
// same. Edges of the round itself are never decremented.
//
// truss_tail_kernel: ONE workgroup peels successive small rounds of the
// level (at most `fuse` entries, no hub edge) behind __syncthreads, until a
// round is empty (the level is done) or is too large or holds a hub edge
// (handed back unprocessed). Every trip consumes at least one entry of
// order, which holds at most m. Nothing here waits for another workgroup:
// no grid barrier, no cooperative launch, no spinning.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t TRUSS_HUB = 1024;        // default longest wave-role S
constexpr uint32_t TRUSS_FUSE = 16;         // default tail-kernel round size
constexpr uint32_t TRUSS_FUSE_MAX = 65536;  // what the tail kernel accepts
constexpr uint32_t TRUSS_LANE_MAX = 64;     // lane-held: longest L
constexpr uint32_t TRUSS_FENCE = 1024;      // default fence entries
constexpr uint32_t TRUSS_FENCE_MAX = 2048;  // the LDS table: 8 KiB
constexpr int TRUSS_TAIL_BLOCK = 1024;      // tail kernel: 16 waves
constexpr int TRUSS_QUAD = 4;               // list entries per wave and trip
constexpr int TRUSS_MAX_GRID = 1 << 16;     // round: blocks per role
constexpr uint32_t TRUSS_NONE = 0xFFFFFFFFu;
enum { TM_TAIL = 0, TM_HUBTAIL = 1, TM_MIN = 2, TM_FUSED = 3, TM_HEAD = 4,
       TM_LANE = 5, TM_WAVE = 6, TM_WORDS = 8 };
enum { T_SUPPORT = 0, T_PEEL = 1, T_CHECK = 2 };
enum { R_NONE = 0, R_LANE = 1, R_WAVE = 2, R_HUB = 3 };

using TrArgs = lux_truss_args;

struct TrCount {
  uint32_t a, b;  // wave-uniform
};

__device__ __forceinline__ uint32_t uni(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}
__device__ __forceinline__ uint64_t uni(uint64_t x) {
  return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x);
}
__device__ __forceinline__ uint32_t ld_relaxed(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int truss_role(uint32_t dS, uint32_t dL,
                                          uint32_t hub) {
  if (dL <= TRUSS_LANE_MAX) return R_LANE;
  return dS <= hub ? R_WAVE : R_HUB;
}

// The two rows of edge e, the shorter first (ties: the lower endpoint).
struct TrRows {
  E_ID Sb, Lb;
  uint32_t dS, dL;
};
__device__ __forceinline__ TrRows truss_rows(const TrArgs& a, uint32_t e) {
  V_ID u = a.elo[e], v = a.ehi[e];
  E_ID ub = a.aptr[u], vb = a.aptr[v];
  uint32_t du = (uint32_t)(a.aptr[u + 1] - ub);
  uint32_t dv = (uint32_t)(a.aptr[v + 1] - vb);
  return du <= dv ? TrRows{ub, vb, du, dv} : TrRows{vb, ub, dv, du};
}

// Append the x of every lane with enq set to order (and its chunk items to
// hubq if it is a hub edge): one atomic on the cursor per wave. All lanes
// of the wave must call this together.
__device__ __forceinline__ void truss_enqueue(const TrArgs& a, bool enq,
                                              uint32_t x) {
  unsigned long long mask = __ballot(enq);
  if (!mask) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader)
    base = atomicAdd(&a.meta[TM_TAIL], (uint32_t)__popcll(mask));
  base = __shfl(base, leader, WAVE);
  if (!enq) return;
  uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
  if (at < a.m) {
    st_relaxed(&a.order[at], x);
    st_relaxed(&a.pos[x], at);
  }
  TrRows r = truss_rows(a, x);
  if (truss_role(r.dS, r.dL, a.hub) == R_HUB) {
    uint32_t nc = ceil_div_u32(r.dS, a.hub);
    uint32_t h = atomicAdd(&a.meta[TM_HUBTAIL], nc);
    for (uint32_t c = 0; c < nc && h + c < a.hubcap; c++) {
      a.hubq[2 * (uint64_t)(h + c)] = x;
      a.hubq[2 * (uint64_t)(h + c) + 1] = c;
    }
  }
}

// One decrement of an edge the round does not hold. Returns whether it is
// the one that makes x removable (see the ownership argument above).
__device__ __forceinline__ bool truss_dec(const TrArgs& a, uint32_t x) {
  int old = atomicSub(&a.sup[x], 1);
  if (old == a.s + 1) return true;
  if (old <= a.s) atomicAdd(&a.sup[x], 1);
  return false;
}

// One candidate triangle (e, e1, e2) per lane, real where hit is set. All
// lanes of the wave must call this together; e and t are wave-uniform.
template <int MODE>
__device__ __forceinline__ void truss_hit(const TrArgs& a, uint32_t e,
                                          uint32_t t, bool hit, uint32_t e1,
                                          uint32_t e2, TrCount& c) {
  hit = hit && e1 < a.m && e2 < a.m;
  if (MODE == T_SUPPORT) {
    c.a += (uint32_t)__popcll(__ballot(hit));
  } else if (MODE == T_CHECK) {
    bool ge = false, gt = false;
    if (hit) {
      uint32_t t1 = a.truss[e1], t2 = a.truss[e2];
      ge = t1 >= t && t2 >= t;
      gt = t1 > t && t2 > t;
    }
    c.a += (uint32_t)__popcll(__ballot(ge));
    c.b += (uint32_t)__popcll(__ballot(gt));
  } else {
    bool d1 = false, d2 = false;
    if (hit) {
      uint32_t p1 = ld_relaxed(&a.pos[e1]), p2 = ld_relaxed(&a.pos[e2]);
      if (p1 >= a.head && p2 >= a.head) {
        bool in1 = p1 < a.tail, in2 = p2 < a.tail;
        d1 = !in1 && (!in2 || e < e2);
        d2 = !in2 && (!in1 || e < e1);
      }
    }
    bool q1 = d1 && truss_dec(a, e1);
    truss_enqueue(a, q1, e1);
    bool q2 = d2 && truss_dec(a, e2);
    truss_enqueue(a, q2, e2);
  }
}

// Four keys per lane searched in lockstep in a[0 : n), n >= 1 and
// wave-uniform; p = the lower bound's position, in [0, n - 1]: a hit is
// a[p] == w (tc_find4's argument; this one returns where).
__device__ __forceinline__ void truss_lb4(const V_ID* a, uint32_t n,
                                          const V_ID (&w)[4],
                                          uint32_t (&p)[4]) {
  uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
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
  p[0] = b0; p[1] = b1; p[2] = b2; p[3] = b3;
}

// ---------------- lane-held role ----------------

// Lk / Le: L and its edge ids, entry `lane` of the row (Lk padded with
// TRUSS_NONE, above every id); Sk / Se: this lane's entry of S, real where
// sok. 64 ascending table entries: six steps and the final compare, each a
// cross-lane read. All lanes of the wave must be active.
template <int MODE>
__device__ __forceinline__ void truss_lane_edge(const TrArgs& a, uint32_t e,
                                                uint32_t t, V_ID Lk,
                                                uint32_t Le, V_ID Sk,
                                                uint32_t Se, bool sok,
                                                TrCount& c) {
  uint32_t b = 0;
#pragma unroll
  for (uint32_t half = TRUSS_LANE_MAX / 2; half >= 1; half >>= 1) {
    V_ID x = __shfl(Lk, (int)(b + half - 1), WAVE);
    b += x < Sk ? half : 0;
  }
  V_ID found = __shfl(Lk, (int)b, WAVE);
  uint32_t eL = __shfl(Le, (int)b, WAVE);
  truss_hit<MODE>(a, e, t, sok && found == Sk, Se, eL, c);
}

// ---------------- wave role ----------------

template <int MODE>
__device__ __forceinline__ void truss_wave_edge(const TrArgs& a, uint32_t e,
                                                uint32_t t, const TrRows& r,
                                                int lane, TrCount& c) {
  const V_ID* L = a.aadj + r.Lb;
  for (uint32_t j0 = 0; j0 < r.dS; j0 += 4 * WAVE) {
    V_ID w[4];
    uint32_t eS[4], p[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t j = j0 + k * WAVE + lane;
      ok[k] = j < r.dS;  // an idle lane searches key 0 and is masked
      w[k] = ok[k] ? a.aadj[r.Sb + j] : 0;
      eS[k] = ok[k] ? a.aeid[r.Sb + j] : 0;
    }
    truss_lb4(L, r.dL, w, p);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      bool hit = ok[k] && L[p[k]] == w[k];
      uint32_t eL = hit ? a.aeid[r.Lb + p[k]] : 0;
      truss_hit<MODE>(a, e, t, hit, eS[k], eL, c);
    }
  }
}

// ---------------- hub role ----------------

// The fence table of L: nf entries, entry i the last element of the
// interval [i * stride, min((i + 1) * stride, dL)). Called by the whole
// workgroup, between barriers.
__device__ __forceinline__ void truss_fence_fill(const V_ID* L, uint32_t dL,
                                                 uint32_t stride, uint32_t nf,
                                                 V_ID* fence) {
  for (uint32_t i = threadIdx.x; i < nf; i += BLOCK) {
    uint64_t last = (uint64_t)(i + 1) * stride;
    fence[i] = L[(last < dL ? last : dL) - 1];
  }
}

// S[first : first + n) against L through the fence table, by the whole
// workgroup. The lower bound in the table names the one interval that can
// hold the key; the second level runs `stride` lockstep steps in it, its
// reads clamped to the row's last element (>= every key that reached an
// interval, so a clamped read never advances the bound).
template <int MODE>
__device__ __forceinline__ void truss_hub_chunk(
    const TrArgs& a, uint32_t e, uint32_t t, const TrRows& r, uint64_t first,
    uint32_t n, const V_ID* fence, uint32_t nf, uint32_t stride,
    TrCount& c) {
  const V_ID* L = a.aadj + r.Lb;
  const uint32_t top = r.dL - 1;
  for (uint32_t j0 = 0; j0 < n; j0 += 4 * BLOCK) {
    V_ID w[4];
    uint32_t eS[4], p[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t j = j0 + k * BLOCK + threadIdx.x;
      ok[k] = j < n;
      w[k] = ok[k] ? a.aadj[r.Sb + first + j] : 0;
      eS[k] = ok[k] ? a.aeid[r.Sb + first + j] : 0;
    }
    truss_lb4(fence, nf, w, p);
    if (stride > 1) {
#pragma unroll
      for (int k = 0; k < 4; k++) p[k] *= stride;
      for (uint32_t len = stride; len > 1;) {
        uint32_t half = len >> 1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          uint32_t at = p[k] + half - 1;
          V_ID x = L[at < top ? at : top];
          p[k] += x < w[k] ? half : 0;
        }
        len -= half;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) p[k] = p[k] < top ? p[k] : top;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      bool hit = ok[k] && (stride > 1 ? L[p[k]] : fence[p[k]]) == w[k];
      uint32_t eL = hit ? a.aeid[r.Lb + p[k]] : 0;
      truss_hit<MODE>(a, e, t, hit, eS[k], eL, c);
    }
  }
}

__device__ __forceinline__ bool truss_violation(const TrArgs& a, uint32_t e,
                                                uint32_t t, const TrCount& c) {
  long long tt = t;
  return tt < 2 || tt > (long long)a.sup0[e] + 2 || (long long)c.a < tt - 2 ||
         (long long)c.b >= tt - 1;
}

// ---------------- a wave's share of a list ----------------

// list[i0 : min(i0 + 4, end)) by one wave: all four edges' rows are read
// first (lane-held role: the whole of both rows), then each edge runs in
// its role. A hub edge only gets its trussness here; its chunks are hubq
// items.
template <int MODE>
__device__ __forceinline__ void truss_quad(const TrArgs& a, uint64_t i0,
                                           uint64_t end, int lane,
                                           unsigned long long& bad) {
  uint32_t e[TRUSS_QUAD];
  int role[TRUSS_QUAD];
  TrRows r[TRUSS_QUAD];
  V_ID Lk[TRUSS_QUAD], Sk[TRUSS_QUAD];
  uint32_t Le[TRUSS_QUAD], Se[TRUSS_QUAD];
#pragma unroll
  for (int g = 0; g < TRUSS_QUAD; g++) {
    role[g] = R_NONE;
    r[g] = TrRows{0, 0, 0, 0};
    e[g] = TRUSS_NONE;
    Lk[g] = TRUSS_NONE;
    Sk[g] = Le[g] = Se[g] = 0;
    if (i0 + g >= end) continue;
    e[g] = uni(MODE == T_PEEL ? ld_relaxed(&a.order[i0 + g])
                              : a.order[i0 + g]);
    if (e[g] >= a.m) continue;
    TrRows q = truss_rows(a, e[g]);
    r[g] = TrRows{uni(q.Sb), uni(q.Lb), uni(q.dS), uni(q.dL)};
    if (!r[g].dS) continue;
    role[g] = truss_role(r[g].dS, r[g].dL, a.hub);
    if (role[g] == R_LANE) {
      if ((uint32_t)lane < r[g].dL) {
        Lk[g] = a.aadj[r[g].Lb + lane];
        Le[g] = a.aeid[r[g].Lb + lane];
      }
      if ((uint32_t)lane < r[g].dS) {
        Sk[g] = a.aadj[r[g].Sb + lane];
        Se[g] = a.aeid[r[g].Sb + lane];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < TRUSS_QUAD; g++) {
    if (role[g] == R_NONE) continue;
    const uint32_t t = MODE == T_CHECK ? uni(a.truss[e[g]]) : 0;
    TrCount c{0, 0};
    if (role[g] == R_LANE)
      truss_lane_edge<MODE>(a, e[g], t, Lk[g], Le[g], Sk[g], Se[g],
                            (uint32_t)lane < r[g].dS, c);
    else if (role[g] == R_WAVE)
      truss_wave_edge<MODE>(a, e[g], t, r[g], lane, c);
    if (lane == 0) {
      if (MODE == T_PEEL) a.truss[e[g]] = (uint32_t)(a.s + 2);
      if (MODE == T_SUPPORT && role[g] != R_HUB) a.sup[e[g]] = (int)c.a;
      if (MODE == T_CHECK && role[g] != R_HUB)
        bad += truss_violation(a, e[g], t, c);
    }
  }
}

// ---------------- adjacency fill ----------------

// keys[0 : n): a run of the sorted directed keys, the entries base.. of the
// adjacency. One lane per entry (x, y): aadj = y, aeid = the position of
// max(x, y) in DAG row min(x, y); the forward entry (x < y) also names the
// arc's row.
__global__ void __launch_bounds__(BLOCK) truss_adj_fill_kernel(
    V_ID nv, E_ID m, const E_ID* optr, const V_ID* oadj,
    const unsigned long long* keys, uint64_t n, uint64_t base, V_ID* aadj,
    uint32_t* aeid, V_ID* elo) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if (base + i >= 2 * m) continue;
    V_ID x = (V_ID)(keys[i] >> 32), y = (V_ID)keys[i];
    V_ID lo = x < y ? x : y, hi = x < y ? y : x;
    uint32_t id = TRUSS_NONE;
    if (hi < nv && lo != hi) {
      E_ID b = optr[lo], len = optr[lo + 1] - b;
      while (len > 1) {  // branch-free lower bound of hi in the DAG row
        E_ID half = len >> 1;
        b += oadj[b + half - 1] < hi ? half : 0;
        len -= half;
      }
      if (b < optr[lo + 1] && b < m && oadj[b] == hi) id = (uint32_t)b;
    }
    aadj[base + i] = y;
    aeid[base + i] = id;
    if (x < y && id != TRUSS_NONE) elo[id] = x;
  }
}

// ---------------- classification ----------------

// One lane per edge: its role, counted in meta[TM_LANE] / meta[TM_WAVE] /
// meta[TM_HUBTAIL] (items); with fill also listed: lane edges from the
// front of a.order, wave edges from its back, hub items in a.hubq. The
// engine runs it once to count and once to fill.
__global__ void __launch_bounds__(BLOCK) truss_classify_kernel(TrArgs a,
                                                               int fill) {
  const int lane = threadIdx.x & (WAVE - 1);
  const unsigned long long below = (1ull << lane) - 1;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  uint64_t e0 = blockIdx.x * (uint64_t)blockDim.x + (threadIdx.x & ~(WAVE - 1));
  for (; e0 < a.m; e0 += stride) {
    uint64_t e = e0 + lane;
    int role = R_NONE;
    uint32_t dS = 0;
    if (e < a.m) {
      TrRows r = truss_rows(a, (uint32_t)e);
      dS = r.dS;
      if (dS) role = truss_role(r.dS, r.dL, a.hub);
    }
#pragma unroll
    for (int which = R_LANE; which <= R_WAVE; which++) {
      unsigned long long mask = __ballot(role == which);
      if (!mask) continue;
      const int leader = __ffsll((long long)mask) - 1;
      uint32_t base = 0;
      if (lane == leader)
        base = atomicAdd(&a.meta[which == R_LANE ? TM_LANE : TM_WAVE],
                         (uint32_t)__popcll(mask));
      base = __shfl(base, leader, WAVE);
      uint32_t at = base + (uint32_t)__popcll(mask & below);
      if (fill && role == which && at < a.m)
        a.order[which == R_LANE ? at : a.m - 1 - at] = (uint32_t)e;
    }
    if (role == R_HUB) {
      uint32_t nc = ceil_div_u32(dS, a.hub);
      uint32_t h = atomicAdd(&a.meta[TM_HUBTAIL], nc);
      for (uint32_t c = 0; fill && c < nc && h + c < a.hubcap; c++) {
        a.hubq[2 * (uint64_t)(h + c)] = (uint32_t)e;
        a.hubq[2 * (uint64_t)(h + c) + 1] = c;
      }
    }
  }
}

// ---------------- level scan ----------------

__global__ void __launch_bounds__(BLOCK) truss_scan_kernel(TrArgs a) {
  __shared__ uint32_t red[BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  uint32_t mn = TRUSS_NONE;
  // a wave takes 4 * 64 consecutive edges per trip, the loads issued
  // together; -1 (below every s) stands for "past the end". A removed edge
  // rests at its level, below s.
  constexpr int U = 4;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x * U;
  for (uint64_t e0 = (blockIdx.x * (uint64_t)blockDim.x + wid * WAVE) * U;
       e0 < a.m; e0 += stride) {
    int d[U];
#pragma unroll
    for (int j = 0; j < U; j++) {
      uint64_t e = e0 + j * WAVE + lane;
      d[j] = e < a.m ? a.sup[e] : -1;
    }
#pragma unroll
    for (int j = 0; j < U; j++) {
      if (d[j] > a.s && (uint32_t)d[j] < mn) mn = (uint32_t)d[j];
      truss_enqueue(a, d[j] == a.s, (uint32_t)(e0 + j * WAVE + lane));
    }
  }
  mn = wave_reduce_min(mn);
  if (lane == 0) red[wid] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / WAVE; w++) mn = red[w] < mn ? red[w] : mn;
    if (mn != TRUSS_NONE) atomicMin(&a.meta[TM_MIN], mn);
  }
}

// ---------------- one list range and its hub items ----------------

// Row blocks take a.order[a.head : a.tail), a wave four entries per trip;
// hub blocks take one hubq item of [hubhead, hubtail) each. In CHECK mode
// the block that holds chunk 0 of a hub edge walks all its chunks, so that
// the two counts of the edge meet in one place.
template <int MODE>
__global__ void __launch_bounds__(BLOCK) truss_round_kernel(
    TrArgs a, uint32_t hubhead, uint32_t hubtail, uint32_t row_blocks) {
  __shared__ V_ID fence[TRUSS_FENCE_MAX];
  __shared__ uint32_t red[2][BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = BLOCK / WAVE;
  unsigned long long bad = 0;
  if (blockIdx.x < row_blocks) {
    uint64_t step = (uint64_t)row_blocks * NW * TRUSS_QUAD;
    for (uint64_t i = a.head + ((uint64_t)blockIdx.x * NW + wid) * TRUSS_QUAD;
         i < a.tail; i += step)
      truss_quad<MODE>(a, i, a.tail, lane, bad);
  } else {
    uint32_t nb = gridDim.x - row_blocks;
    for (uint64_t i = hubhead + (blockIdx.x - row_blocks); i < hubtail;
         i += nb) {
      uint32_t e = uni(a.hubq[2 * i]), chunk = uni(a.hubq[2 * i + 1]);
      if (e >= a.m || (MODE == T_CHECK && chunk != 0)) continue;
      TrRows q = truss_rows(a, e);
      const TrRows r{uni(q.Sb), uni(q.Lb), uni(q.dS), uni(q.dL)};
      if (!r.dS) continue;
      const uint32_t stride = ceil_div_u32(r.dL, a.fence);
      const uint32_t nf = ceil_div_u32(r.dL, stride);
      __syncthreads();  // the previous item's searches are done
      truss_fence_fill(a.aadj + r.Lb, r.dL, stride, nf, fence);
      __syncthreads();
      const uint32_t t = MODE == T_CHECK ? a.truss[e] : 0;
      const uint32_t last =
          MODE == T_CHECK ? ceil_div_u32(r.dS, a.hub) : chunk + 1;
      TrCount c{0, 0};
      for (uint32_t ch = chunk; ch < last; ch++) {
        uint64_t first = (uint64_t)ch * a.hub;
        if (first >= r.dS) break;
        uint32_t n = r.dS - first < a.hub ? (uint32_t)(r.dS - first) : a.hub;
        truss_hub_chunk<MODE>(a, e, t, r, first, n, fence, nf, stride, c);
      }
      if (MODE == T_SUPPORT && lane == 0 && c.a) atomicAdd(&a.sup[e], (int)c.a);
      if (MODE == T_CHECK) {
        if (lane == 0) {
          red[0][wid] = c.a;
          red[1][wid] = c.b;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          TrCount s{0, 0};
          for (int w = 0; w < NW; w++) {
            s.a += red[0][w];
            s.b += red[1][w];
          }
          bad += truss_violation(a, e, t, s);
        }
      }
    }
  }
  if (MODE == T_CHECK && lane == 0 && bad) atomicAdd(a.bad, bad);
}

// ---------------- small-round fusion ----------------

// One workgroup. The host launches it on a round [head, tail) of at most
// fuse entries with no hub item pending (hubtail = the hubq cursor then).
__global__ void __launch_bounds__(TRUSS_TAIL_BLOCK) truss_tail_kernel(
    TrArgs a, uint32_t hubtail, uint32_t fuse) {
  __shared__ uint32_t lds_tail, lds_hubtail;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = TRUSS_TAIL_BLOCK / WAVE;
  uint32_t rounds = 0;
  unsigned long long unused = 0;
  for (;;) {
    for (uint64_t i = a.head + (uint64_t)wid * TRUSS_QUAD; i < a.tail;
         i += NW * TRUSS_QUAD)
      truss_quad<T_PEEL>(a, i, a.tail, lane, unused);
    rounds++;
    a.head = a.tail;
    __syncthreads();  // every wave's appends are counted in the cursors
    if (threadIdx.x == 0) {
      lds_tail = ld_relaxed(&a.meta[TM_TAIL]);
      lds_hubtail = ld_relaxed(&a.meta[TM_HUBTAIL]);
    }
    __syncthreads();
    a.tail = lds_tail;
    // empty: the level is done; too large, a hub edge, or a cursor past the
    // list: the host's
    if (a.tail <= a.head || a.tail - a.head > fuse ||
        lds_hubtail != hubtail || a.tail > a.m)
      break;
  }
  if (threadIdx.x == 0) {
    a.meta[TM_FUSED] = rounds;
    a.meta[TM_HEAD] = a.head;
  }
}

template <int MODE>
static void truss_launch_round(hipStream_t s, const TrArgs& a,
                               uint32_t hubhead, uint32_t hubtail) {
  const uint32_t n = a.tail - a.head, nh = hubtail - hubhead;
  uint32_t rb = ceil_div_u32(ceil_div_u32(n, TRUSS_QUAD), BLOCK / WAVE);
  if (rb > (uint32_t)TRUSS_MAX_GRID) rb = TRUSS_MAX_GRID;
  uint32_t hb = nh > (uint32_t)TRUSS_MAX_GRID ? TRUSS_MAX_GRID : nh;
  hipLaunchKernelGGL(truss_round_kernel<MODE>, dim3(rb + hb), dim3(BLOCK), 0,
                     s, a, hubhead, hubtail, rb);
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_truss_hub_default() { return TRUSS_HUB; }
uint32_t lux_gpu_truss_fuse_default() { return TRUSS_FUSE; }
uint32_t lux_gpu_truss_fuse_max() { return TRUSS_FUSE_MAX; }
uint32_t lux_gpu_truss_fence_default() { return TRUSS_FENCE; }
uint32_t lux_gpu_truss_fence_max() { return TRUSS_FENCE_MAX; }
uint32_t lux_gpu_truss_meta_words() { return TM_WORDS; }

void lux_gpu_truss_adj_fill(uint64_t stream, V_ID nv, E_ID m,
                            const E_ID* optr, const V_ID* oadj,
                            const unsigned long long* keys, uint64_t n,
                            uint64_t base, V_ID* aadj, uint32_t* aeid,
                            V_ID* elo) {
  if (!nv || !m || !n || base + n > 2 * m) return;
  hipLaunchKernelGGL(truss_adj_fill_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     (hipStream_t)stream, nv, m, optr, oadj, keys, n, base,
                     aadj, aeid, elo);
  LUX_POST_LAUNCH(stream);
}

static bool truss_args_ok(const lux_truss_args* a) {
  return a->hub && a->fence && a->fence <= TRUSS_FENCE_MAX &&
         a->head <= a->tail && a->tail <= a->m;
}

int lux_gpu_truss_classify(uint64_t stream, const lux_truss_args* a,
                           int fill) {
  if (!truss_args_ok(a)) return -1;
  if (!a->m) return 0;
  hipLaunchKernelGGL(truss_classify_kernel, dim3(grid_for(a->m)), dim3(BLOCK),
                     0, (hipStream_t)stream, *a, fill);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_truss_scan(uint64_t stream, const lux_truss_args* a) {
  if (!truss_args_ok(a)) return -1;
  if (!a->m) return 0;
  hipStream_t s = (hipStream_t)stream;
  LUX_CHECK_HIP(hipMemsetAsync(a->meta + TM_MIN, 0xFF, sizeof(uint32_t), s));
  hipLaunchKernelGGL(truss_scan_kernel, dim3(grid_for(((uint64_t)a->m + 3) / 4)),
                     dim3(BLOCK), 0, s, *a);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_truss_round(uint64_t stream, const lux_truss_args* a, int mode,
                        uint32_t hubhead, uint32_t hubtail) {
  if (!truss_args_ok(a) || hubhead > hubtail || hubtail > a->hubcap ||
      mode < T_SUPPORT || mode > T_CHECK)
    return -1;
  if (a->head == a->tail && hubhead == hubtail) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (mode == T_SUPPORT) truss_launch_round<T_SUPPORT>(s, *a, hubhead, hubtail);
  else if (mode == T_PEEL) truss_launch_round<T_PEEL>(s, *a, hubhead, hubtail);
  else truss_launch_round<T_CHECK>(s, *a, hubhead, hubtail);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_truss_tail(uint64_t stream, const lux_truss_args* a,
                       uint32_t hubtail, uint32_t fuse) {
  if (!truss_args_ok(a) || !fuse || fuse > TRUSS_FUSE_MAX ||
      a->head >= a->tail || a->tail - a->head > fuse || hubtail > a->hubcap)
    return -1;
  hipLaunchKernelGGL(truss_tail_kernel, dim3(1), dim3(TRUSS_TAIL_BLOCK), 0,
                     (hipStream_t)stream, *a, hubtail, fuse);
  LUX_POST_LAUNCH(stream);
  return 0;
}

}  // extern "C"
