// Strongly connected components: trim, forward-backward reach and colour
// propagation with device-side queues, single-workgroup step fusion and a
// check oracle for gfx950. No reference equivalent.
//
// Input (lux_amd/scc_engine.py): the directed graph in both directions,
// in_ptr u64[nv+1] / in_col u32[ne] (row v: the sources of v's in-edges, the
// CSC as loaded) and out_ptr / out_col (row u: the targets of u's
// out-edges). Every edge index is 64-bit. Parallel edges count once per
// occurrence, self-loops never.
//
// State of a decomposition:
//   label   u32[nv]  the answer (largest id of the SCC); NONE = alive.
//   in_cnt / out_cnt i32[nv]  alive in- / out-neighbour occurrences of an
//                    alive vertex; signed, a vertex already claimed may be
//                    decremented below 0.
//   colour  u32[nv]  max-propagation value of a colour round.
//   mark    u32[nv]  bits: F / B = reached by the forward / backward
//                    traversal, T = claimed by trim (or dead).
//   stamp   u32[nv]  the last colour step that queued the vertex.
//   queues  u32      append-only lists of vertices; a frontier (or a trim
//                    round) is a range [head, tail) of one. Colour frontiers
//                    are double-buffered: a step reads one half and appends
//                    to the other.
//   hubq    u32 pairs {vertex, chunk}: a queued vertex whose row (the rows
//                    the mode walks) is longer than `hub` ALSO gives
//                    ceil(d / hub) chunk items here. Sized by the host from
//                    the degrees; all appends are bounds-checked.
//   meta    u32[S_WORDS]  cursors and results, see the enum.
//
// Kernels:
//   scc_count_kernel   alive-neighbour counts per alive row (a wave per
//                      row, 64 rows per wave and trip, so that the append of
//                      the zero-count rows — the first trim round — is one
//                      ballot and one atomic per wave); rows longer than
//                      hub are counted before it by scc_count_hub_kernel, a
//                      workgroup per chunk of a static item list;
//   scc_pivot_kernel   max in_cnt * out_cnt (u64), then the lowest id that
//                      has it; run after the trim so the counts are current;
//   scc_scan_kernel    one lane per vertex: colour[v] = v and the first
//                      colour frontier, or the roots of a colour round;
//   scc_step_kernel    one frontier step / trim round, the role from
//                      blockIdx.x: row blocks take queue[head : tail), a
//                      wave per entry, lanes striding over rows of at most
//                      `hub` entries; hub blocks take one hubq item each;
//   scc_tail_kernel    ONE workgroup runs successive small steps (at most
//                      `fuse` entries, no hub row) with a workgroup barrier
//                      between them, so a path or a cycle costs one launch.
//                      It stops at an empty step or hands a step that is too
//                      large or has a hub row back unprocessed;
//   scc_commit_kernel  F & B intersection (max id, labels) or label =
//                      colour of the reached; counts what died.
// Nothing here waits for another workgroup: no grid barrier, no spinning.
//
// scc_check_*_kernel are the device oracle: plain one-lane-per-vertex (or
// per-edge) sweeps sharing no queue or role code with the above.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

constexpr uint32_t SCC_HUB = 1024;        // default longest row-role row
constexpr uint32_t SCC_FUSE = 16;         // default tail-kernel step size
constexpr uint32_t SCC_FUSE_MAX = 65536;  // what the tail kernel accepts
constexpr int SCC_TAIL_BLOCK = 1024;      // tail kernel: 16 waves
constexpr int SCC_MAX_GRID = 1 << 16;     // step: blocks per role
constexpr int SCC_CHECK_REPS = 4;         // check sweep: passes per launch
constexpr uint32_t SCC_NONE = 0xFFFFFFFFu;
constexpr uint32_t SCC_F = 1, SCC_B = 2, SCC_T = 4;
enum { S_TTAIL = 0, S_RTAIL = 1, S_CTAIL = 2, S_HUBTAIL = 3, S_FUSED = 4,
       S_HEAD = 5, S_DIED = 6, S_MAXID = 7, S_PIVOT = 8,
       S_PROD = 10 /* u64: words 10 and 11 */, S_WORDS = 16 };
enum { SCC_TRIM = 0, SCC_REACH = 1, SCC_COLOUR = 2 };
enum { SCC_SCAN_INIT = 0, SCC_SCAN_ROOTS = 1 };

using SccArgs = lux_scc_args;
using SccStep = lux_scc_step;

template <typename T>
__device__ __forceinline__ T scc_ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void scc_st(T* p, T x) {
  __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t scc_chunks(const SccArgs& a, uint64_t d) {
  return d > a.hub ? (uint32_t)((d + a.hub - 1) / a.hub) : 0u;
}

// hubq items of a queued vertex: in-row chunks first, then out-row chunks,
// of the rows the mode walks.
__device__ __forceinline__ uint32_t scc_hub_items(const SccArgs& a,
                                                  const SccStep& st, V_ID w) {
  uint64_t din = a.in_ptr[w + 1] - a.in_ptr[w];
  uint64_t dout = a.out_ptr[w + 1] - a.out_ptr[w];
  if (st.mode == SCC_TRIM) return scc_chunks(a, din) + scc_chunks(a, dout);
  return scc_chunks(a, st.mode == SCC_REACH && st.dir ? din : dout);
}

// Append the w of every lane with enq set to st.qw (and its chunk items to
// hubq): one atomic on the cursor per wave. All lanes of the wave must call
// this together.
__device__ __forceinline__ void scc_enqueue(const SccArgs& a,
                                            const SccStep& st, bool enq,
                                            V_ID w) {
  unsigned long long mask = __ballot(enq);
  if (!mask) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader)
    base = atomicAdd(&a.meta[st.mw], (uint32_t)__popcll(mask));
  base = __shfl(base, leader, WAVE);
  if (!enq) return;
  uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
  if (at < st.qcap) st.qw[at] = w;
  uint32_t nc = scc_hub_items(a, st, w);
  if (nc) {
    uint32_t h = atomicAdd(&a.meta[S_HUBTAIL], nc);
    for (uint32_t c = 0; c < nc && h + c < st.hcap; c++) {
      a.hubq[2 * (uint64_t)(st.hw0 + h + c)] = w;
      a.hubq[2 * (uint64_t)(st.hw0 + h + c) + 1] = c;
    }
  }
}

// One neighbour w of the queue entry v (cv: v's colour where the mode uses
// it; inrow: w came from v's in-row). Returns whether this lane queues w.
//   trim:   the decrement that takes the counter to 0 claims w through the T
//           bit, so a vertex losing both counters in one round is queued
//           once. A dead w (its label is set) is skipped: its counters are
//           stale.
//   reach:  alive, of v's colour in colour mode, and this lane sets the bit.
//   colour: this lane raised colour[w], and is the first of the step to.
__device__ __forceinline__ bool scc_visit(const SccArgs& a, const SccStep& st,
                                          V_ID v, uint32_t cv, V_ID w,
                                          bool inrow) {
  if (w >= a.nv || scc_ld(&a.label[w]) != SCC_NONE) return false;
  if (st.mode == SCC_TRIM) {
    if (w == v) return false;
    int* cnt = inrow ? a.out_cnt : a.in_cnt;
    if (atomicSub(&cnt[w], 1) != 1) return false;
    return !(atomicOr(&a.mark[w], SCC_T) & SCC_T);
  }
  if (st.mode == SCC_REACH) {
    if (st.cmode && scc_ld(&a.colour[w]) != cv) return false;
    if (scc_ld(&a.mark[w]) & st.bit) return false;
    return !(atomicOr(&a.mark[w], st.bit) & st.bit);
  }
  if (scc_ld(&a.colour[w]) >= cv) return false;
  if (atomicMax(&a.colour[w], cv) >= cv) return false;
  return atomicMax(&a.stamp[w], st.step) < st.step;
}

// The entries sub, sub + step, ... of col[b : b + n), one per lane and
// trip; n is the same in every lane of a wave.
__device__ __forceinline__ void scc_span(const SccArgs& a, const SccStep& st,
                                         const V_ID* col, E_ID b, uint32_t n,
                                         uint32_t sub, uint32_t step, V_ID v,
                                         uint32_t cv, bool inrow) {
  for (uint32_t j = sub; __any(j < n); j += step) {
    bool enq = false;
    V_ID w = 0;
    if (j < n) {
      w = col[b + j];
      enq = scc_visit(a, st, v, cv, w, inrow);
    }
    scc_enqueue(a, st, enq, w);
  }
}

__device__ __forceinline__ uint32_t scc_entry_colour(const SccArgs& a,
                                                     const SccStep& st,
                                                     V_ID v) {
  if (st.mode == SCC_COLOUR || (st.mode == SCC_REACH && st.cmode))
    return scc_ld(&a.colour[v]);
  return 0;
}

// Row role: one wave takes the queue entry v and walks its rows of at most
// hub entries. A trimmed vertex gets its label here.
__device__ __forceinline__ void scc_entry(const SccArgs& a, const SccStep& st,
                                          V_ID v, int lane) {
  const bool trim = st.mode == SCC_TRIM;
  if (trim && lane == 0 && scc_ld(&a.label[v]) == SCC_NONE)
    scc_st(&a.label[v], (uint32_t)v);
  const uint32_t cv = scc_entry_colour(a, st, v);
  const bool wout = trim || st.mode == SCC_COLOUR || !st.dir;
  const bool win = trim || (st.mode == SCC_REACH && st.dir);
  if (wout) {
    E_ID b = a.out_ptr[v];
    uint64_t d = a.out_ptr[v + 1] - b;
    if (d <= a.hub)
      scc_span(a, st, a.out_col, b, (uint32_t)d, lane, WAVE, v, cv, false);
  }
  if (win) {
    E_ID b = a.in_ptr[v];
    uint64_t d = a.in_ptr[v + 1] - b;
    if (d <= a.hub)
      scc_span(a, st, a.in_col, b, (uint32_t)d, lane, WAVE, v, cv, true);
  }
}

// Hub role: one workgroup takes the hubq item i of the read half.
__device__ __forceinline__ void scc_hub_item(const SccArgs& a,
                                             const SccStep& st, uint64_t i) {
  V_ID v = a.hubq[2 * (st.hr0 + i)];
  uint32_t c = a.hubq[2 * (st.hr0 + i) + 1];
  if (v >= a.nv) return;
  bool inrow = st.mode == SCC_REACH && st.dir;
  if (st.mode == SCC_TRIM) {
    uint32_t nci = scc_chunks(a, a.in_ptr[v + 1] - a.in_ptr[v]);
    inrow = c < nci;
    if (!inrow) c -= nci;
  }
  const E_ID* ptr = inrow ? a.in_ptr : a.out_ptr;
  E_ID b = ptr[v];
  uint64_t d = ptr[v + 1] - b;
  uint64_t first = (uint64_t)c * a.hub;
  uint32_t n = 0;
  if (first < d) n = d - first < a.hub ? (uint32_t)(d - first) : a.hub;
  scc_span(a, st, inrow ? a.in_col : a.out_col, b + first, n, threadIdx.x,
           blockDim.x, v, scc_entry_colour(a, st, v), inrow);
}

// ---------------- counts and the first trim round ----------------

__device__ __forceinline__ int scc_count_row(const SccArgs& a,
                                             const E_ID* ptr, const V_ID* col,
                                             V_ID r, int lane) {
  int c = 0;
  for (E_ID j = ptr[r] + lane, e = ptr[r + 1]; j < e; j += WAVE) {
    V_ID u = col[j];
    c += u != r && u < a.nv && a.label[u] == SCC_NONE;
  }
  return __shfl(wave_reduce_sum(c), 0, WAVE);
}

// Hub rows of the count: one workgroup per {vertex, chunk} item of the
// static list (every row longer than hub, in-row chunks first, then out-row
// chunks, as in hubq), its alive entries added to the zeroed counter. Without
// it the wave that holds the 64 largest rows of an RMAT walks them alone.
__global__ void __launch_bounds__(BLOCK) scc_count_hub_kernel(
    SccArgs a, const uint32_t* items, uint32_t n) {
  __shared__ int lds[BLOCK / WAVE];
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    V_ID v = items[2 * (uint64_t)i];
    uint32_t c = items[2 * (uint64_t)i + 1];
    if (v >= a.nv || a.label[v] != SCC_NONE) continue;  // the whole block
    uint32_t nci = scc_chunks(a, a.in_ptr[v + 1] - a.in_ptr[v]);
    const bool inrow = c < nci;
    if (!inrow) c -= nci;
    const E_ID* ptr = inrow ? a.in_ptr : a.out_ptr;
    const V_ID* col = inrow ? a.in_col : a.out_col;
    E_ID b = ptr[v];
    uint64_t d = ptr[v + 1] - b;
    uint64_t first = (uint64_t)c * a.hub;
    uint32_t m = 0;
    if (first < d) m = d - first < a.hub ? (uint32_t)(d - first) : a.hub;
    int cnt = 0;
    for (uint32_t j = threadIdx.x; j < m; j += BLOCK) {
      V_ID u = col[b + first + j];
      cnt += u != v && u < a.nv && a.label[u] == SCC_NONE;
    }
    cnt = block_reduce_sum(cnt, lds);
    if (threadIdx.x == 0 && cnt)
      atomicAdd(inrow ? &a.in_cnt[v] : &a.out_cnt[v], cnt);
    __syncthreads();  // lds is written again in the next trip
  }
}

// st: the trim queue (append). Labels do not change here, so the counts are
// those of the alive subgraph at launch. Rows longer than hub have been
// counted by scc_count_hub_kernel; the others are walked here.
__global__ void __launch_bounds__(BLOCK) scc_count_kernel(SccArgs a,
                                                          SccStep st) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  uint64_t stride = (uint64_t)gridDim.x * (BLOCK / WAVE) * WAVE;
  for (uint64_t v0 = ((uint64_t)blockIdx.x * (BLOCK / WAVE) + wid) * WAVE;
       v0 < a.nv; v0 += stride) {
    uint64_t v = v0 + lane;
    bool alive = v < a.nv && a.label[v] == SCC_NONE;
    int ic = 0, oc = 0;
    for (unsigned long long todo = __ballot(alive); todo; todo &= todo - 1) {
      int j = __ffsll((long long)todo) - 1;
      V_ID r = (V_ID)(v0 + j);
      const bool hin = a.in_ptr[r + 1] - a.in_ptr[r] > a.hub;
      const bool hout = a.out_ptr[r + 1] - a.out_ptr[r] > a.hub;
      int ci = hin ? 0 : scc_count_row(a, a.in_ptr, a.in_col, r, lane);
      int co = hout ? 0 : scc_count_row(a, a.out_ptr, a.out_col, r, lane);
      if (lane == j) {
        ic = hin ? a.in_cnt[r] : ci;
        oc = hout ? a.out_cnt[r] : co;
      }
    }
    bool zero = alive && (ic == 0 || oc == 0);
    if (alive) {
      a.in_cnt[v] = ic;
      a.out_cnt[v] = oc;
      a.mark[v] = zero ? SCC_T : 0u;
    }
    scc_enqueue(a, st, zero, (V_ID)v);
  }
}

// pass 0: meta[S_PROD] (u64) = max in_cnt * out_cnt over the alive; pass 1:
// meta[S_PIVOT] = the lowest id that has it.
__global__ void __launch_bounds__(BLOCK) scc_pivot_kernel(SccArgs a,
                                                          int pass) {
  unsigned long long* prod = (unsigned long long*)(a.meta + S_PROD);
  unsigned long long best = pass ? *prod : 0ull;
  uint32_t low = SCC_NONE;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       v < a.nv; v += stride) {
    if (a.label[v] != SCC_NONE) continue;
    long long i = a.in_cnt[v], o = a.out_cnt[v];
    unsigned long long p = i > 0 && o > 0 ? (unsigned long long)(i * o) : 0;
    if (!pass)
      best = p > best ? p : best;
    else if (p == best && (uint32_t)v < low)
      low = (uint32_t)v;
  }
  if (!pass) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      unsigned long long o = __shfl_down(best, off, WAVE);
      best = o > best ? o : best;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && best) atomicMax(prod, best);
  } else {
    low = wave_reduce_min(low);
    if ((threadIdx.x & (WAVE - 1)) == 0 && low != SCC_NONE)
      atomicMin(&a.meta[S_PIVOT], low);
  }
}

// One lane per vertex. INIT: colour[v] = v, every alive v into st.qw (the
// first colour frontier). ROOTS: the alive v with colour[v] == v get st.bit
// and go into st.qw (the seeds of the backward traversal).
__global__ void __launch_bounds__(BLOCK) scc_scan_kernel(SccArgs a, SccStep st,
                                                         int what) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v0 = blockIdx.x * (uint64_t)blockDim.x; v0 < a.nv;
       v0 += stride) {
    uint64_t v = v0 + threadIdx.x;
    bool enq = v < a.nv && a.label[v] == SCC_NONE;
    if (enq && what == SCC_SCAN_INIT) a.colour[v] = (uint32_t)v;
    if (enq && what == SCC_SCAN_ROOTS) {
      enq = a.colour[v] == (uint32_t)v;
      if (enq) a.mark[v] |= st.bit;
    }
    scc_enqueue(a, st, enq, (V_ID)v);
  }
}

// One wave: the single vertex v gets st.bit and goes into st.qw.
__global__ void __launch_bounds__(WAVE) scc_seed_kernel(SccArgs a, SccStep st,
                                                        V_ID v) {
  bool enq = threadIdx.x == 0 && v < a.nv;
  if (enq) atomicOr(&a.mark[v], st.bit);
  scc_enqueue(a, st, enq, v);
}

// ---------------- one step ----------------

__global__ void __launch_bounds__(BLOCK) scc_step_kernel(
    SccArgs a, SccStep st, uint32_t head, uint32_t tail, uint32_t hubhead,
    uint32_t hubtail, uint32_t row_blocks) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = BLOCK / WAVE;
  if (blockIdx.x < row_blocks) {
    uint64_t step = (uint64_t)row_blocks * NW;
    for (uint64_t i = head + (uint64_t)blockIdx.x * NW + wid; i < tail;
         i += step) {
      V_ID v = st.qr[i];
      if (v < a.nv) scc_entry(a, st, v, lane);
    }
  } else {
    uint32_t nb = gridDim.x - row_blocks;
    for (uint64_t i = hubhead + (blockIdx.x - row_blocks); i < hubtail;
         i += nb)
      scc_hub_item(a, st, i);
  }
}

// ---------------- small-step fusion ----------------

// One workgroup. The host launches it on a step [head, tail) of st.qr of at
// most fuse entries with no hub item pending. Append mode (pingpong == 0):
// the next step is [tail, cursor) of the same list, hubtail the hubq cursor
// at launch. Ping-pong mode (colour): the next step is [0, cursor) of the
// other half, the cursors having been zero at launch; this kernel swaps the
// halves and zeroes the cursor between steps, and st.step counts up.
__global__ void __launch_bounds__(SCC_TAIL_BLOCK) scc_tail_kernel(
    SccArgs a, SccStep st, uint32_t head, uint32_t tail, uint32_t hubtail,
    uint32_t fuse, int pingpong) {
  __shared__ uint32_t lds_tail, lds_go;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  constexpr int NW = SCC_TAIL_BLOCK / WAVE;
  uint32_t steps = 0;
  for (;;) {
    for (uint32_t i = head + wid; i < tail; i += NW) {
      V_ID v = scc_ld(&st.qr[i]);
      if (v < a.nv) scc_entry(a, st, v, lane);
    }
    steps++;
    __syncthreads();  // every wave's appends are counted in the cursors
    if (threadIdx.x == 0) {
      uint32_t nt = scc_ld(&a.meta[st.mw]);
      uint32_t nh = scc_ld(&a.meta[S_HUBTAIL]);
      bool go;
      if (pingpong)
        go = nt > 0 && nt <= fuse && nt <= st.qcap && nh == 0;
      else
        go = nt > tail && nt - tail <= fuse && nt <= st.qcap && nh == hubtail;
      if (go && pingpong) scc_st(&a.meta[st.mw], 0u);
      lds_tail = nt;
      lds_go = go;
    }
    __syncthreads();
    if (pingpong) {
      head = 0;
      const V_ID* q = st.qr;
      st.qr = st.qw;
      st.qw = const_cast<V_ID*>(q);
      uint32_t h = st.hr0;
      st.hr0 = st.hw0;
      st.hw0 = h;
      st.step++;
    } else {
      head = tail;
    }
    tail = lds_tail;
    if (!lds_go) break;
  }
  if (threadIdx.x == 0) {
    a.meta[S_FUSED] = steps;
    a.meta[S_HEAD] = head;
  }
}

// ---------------- commit ----------------

// what 0: meta[S_MAXID] = the largest id with F and B, meta[S_DIED] their
// number; what 1: those vertices get label = meta[S_MAXID]; what 2 (colour
// round): every alive vertex with B gets label = colour, counted in
// meta[S_DIED]. Whoever dies also gets T.
__global__ void __launch_bounds__(BLOCK) scc_commit_kernel(SccArgs a,
                                                           int what) {
  __shared__ uint32_t lds[BLOCK / WAVE];
  const uint32_t top = what == 1 ? a.meta[S_MAXID] : 0;
  uint32_t died = 0, mx = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
       v < a.nv; v += stride) {
    if (a.label[v] != SCC_NONE) continue;
    uint32_t m = a.mark[v];
    if (what == 2) {
      if (!(m & SCC_B)) continue;
      a.label[v] = a.colour[v];
      a.mark[v] = m | SCC_T;
      died++;
    } else if ((m & (SCC_F | SCC_B)) == (SCC_F | SCC_B)) {
      if (what == 0) {
        died++;
        mx = (uint32_t)v > mx ? (uint32_t)v : mx;
      } else {
        a.label[v] = top;
        a.mark[v] = m | SCC_T;
      }
    }
  }
  if (what == 1) return;
  mx = wave_reduce_max(mx);
  if (what == 0 && (threadIdx.x & (WAVE - 1)) == 0 && mx)
    atomicMax(&a.meta[S_MAXID], mx);
  died = block_reduce_sum(died, lds);
  if (threadIdx.x == 0 && died) atomicAdd(&a.meta[S_DIED], died);
}

// ---------------- check oracle ----------------

// what 0: bad += label[v] < v, label[v] >= nv or label[label[v]] != label[v];
//         fwd[v] = bwd[v] = (label[v] == v).
// what 1: bad += !fwd[v] or !bwd[v].
__global__ void __launch_bounds__(BLOCK) scc_check_vertex_kernel(
    V_ID nv, const uint32_t* label, uint32_t* fwd, uint32_t* bwd,
    unsigned long long* bad, int what) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long mine = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; v < nv;
       v += stride) {
    if (what == 0) {
      uint32_t l = label[v];
      mine += l < v || l >= nv || label[l] != l;
      fwd[v] = bwd[v] = l == (uint32_t)v;
    } else {
      mine += !fwd[v] || !bwd[v];
    }
  }
  mine = block_reduce_sum(mine, lds);
  if (threadIdx.x == 0 && mine) atomicAdd(bad, mine);
}

// fwd[v] is set once an in-neighbour of v's label has it (v is reached from
// its root inside its class), bwd[v] once an out-neighbour of v's label has
// it (v reaches its root). Monotone, so any order of evaluation gives the
// same fixpoint; *changed is set if anything was.
__global__ void __launch_bounds__(BLOCK) scc_check_sweep_kernel(
    V_ID nv, const E_ID* in_ptr, const V_ID* in_col, const E_ID* out_ptr,
    const V_ID* out_col, const uint32_t* label, uint32_t* fwd, uint32_t* bwd,
    uint32_t* changed) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  bool any = false;
  for (int rep = 0; rep < SCC_CHECK_REPS; rep++) {
    for (uint64_t v = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
         v < nv; v += stride) {
      const uint32_t l = label[v];
      if (!scc_ld(&fwd[v])) {
        for (E_ID j = in_ptr[v], e = in_ptr[v + 1]; j < e; j++) {
          V_ID u = in_col[j];
          if (u < nv && label[u] == l && scc_ld(&fwd[u])) {
            scc_st(&fwd[v], 1u);
            any = true;
            break;
          }
        }
      }
      if (!scc_ld(&bwd[v])) {
        for (E_ID j = out_ptr[v], e = out_ptr[v + 1]; j < e; j++) {
          V_ID w = out_col[j];
          if (w < nv && label[w] == l && scc_ld(&bwd[w])) {
            scc_st(&bwd[v], 1u);
            any = true;
            break;
          }
        }
      }
    }
  }
  if (any) scc_st(changed, 1u);
}

// One lane per in-edge u -> v with label[u] != label[v]: bad++ if v -> u
// exists too (searched in the shorter of v's out-row and u's in-row).
__global__ void __launch_bounds__(BLOCK) scc_check_pairs_kernel(
    V_ID nv, E_ID ne, const E_ID* in_ptr, const V_ID* in_col,
    const E_ID* out_ptr, const V_ID* out_col, const uint32_t* label,
    unsigned long long* bad) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long mine = 0;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (E_ID e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < ne;
       e += stride) {
    // v = the last row with in_ptr[v] <= e
    V_ID v = 0;
    for (V_ID len = nv; len > 1;) {
      V_ID half = len >> 1;
      v += in_ptr[v + half] <= e ? half : 0;
      len -= half;
    }
    V_ID u = in_col[e];
    if (u >= nv || label[u] == label[v]) continue;
    E_ID ob = out_ptr[v], oe = out_ptr[v + 1];
    E_ID ib = in_ptr[u], ie = in_ptr[u + 1];
    bool found = false;
    if (oe - ob <= ie - ib) {
      for (E_ID j = ob; j < oe && !found; j++) found = out_col[j] == u;
    } else {
      for (E_ID j = ib; j < ie && !found; j++) found = in_col[j] == v;
    }
    mine += found;
  }
  mine = block_reduce_sum(mine, lds);
  if (threadIdx.x == 0 && mine) atomicAdd(bad, mine);
}

}  // namespace lux

using namespace lux;

namespace {
bool scc_step_ok(const SccArgs& a, const SccStep& st) {
  return a.hub && st.mode >= SCC_TRIM && st.mode <= SCC_COLOUR &&
         st.mw < S_WORDS && st.qr && st.qw;
}
void scc_zero(hipStream_t s, uint32_t* word, int n = 1) {
  LUX_CHECK_HIP(hipMemsetAsync(word, 0, n * sizeof(uint32_t), s));
}
}  // namespace

extern "C" {

uint32_t lux_gpu_scc_hub_default() { return SCC_HUB; }
uint32_t lux_gpu_scc_fuse_default() { return SCC_FUSE; }
uint32_t lux_gpu_scc_fuse_max() { return SCC_FUSE_MAX; }
uint32_t lux_gpu_scc_meta_words() { return S_WORDS; }

// Recount the alive subgraph and append its zero-count vertices to st.qw
// (the trim queue, cursor meta[st.mw]); the hubq cursor restarts at 0.
// items: the static list of nitems {vertex, chunk} pairs of every row longer
// than hub (in-row chunks first, then out-row chunks).
void lux_gpu_scc_count(uint64_t stream, const lux_scc_args* a,
                       const lux_scc_step* st, const uint32_t* items,
                       uint32_t nitems) {
  if (!a->nv) return;
  hipStream_t s = (hipStream_t)stream;
  scc_zero(s, a->meta + S_HUBTAIL);
  if (nitems) {
    LUX_CHECK_HIP(hipMemsetAsync(a->in_cnt, 0, sizeof(int) * (size_t)a->nv, s));
    LUX_CHECK_HIP(hipMemsetAsync(a->out_cnt, 0, sizeof(int) * (size_t)a->nv, s));
    uint32_t grid = nitems > (uint32_t)SCC_MAX_GRID ? SCC_MAX_GRID : nitems;
    hipLaunchKernelGGL(scc_count_hub_kernel, dim3(grid), dim3(BLOCK), 0, s, *a,
                       items, nitems);
  }
  // a wave per 64 vertices
  hipLaunchKernelGGL(scc_count_kernel, dim3(grid_for(a->nv)), dim3(BLOCK), 0,
                     s, *a, *st);
  LUX_POST_LAUNCH(stream);
}

// meta[S_PIVOT] = the alive vertex of maximum in_cnt * out_cnt, lowest id
// first; 0xFFFFFFFF if none has a positive product.
void lux_gpu_scc_pivot(uint64_t stream, const lux_scc_args* a) {
  if (!a->nv) return;
  hipStream_t s = (hipStream_t)stream;
  scc_zero(s, a->meta + S_PROD, 2);
  LUX_CHECK_HIP(hipMemsetAsync(a->meta + S_PIVOT, 0xFF, sizeof(uint32_t), s));
  for (int pass = 0; pass < 2; pass++)
    hipLaunchKernelGGL(scc_pivot_kernel, dim3(grid_for(a->nv)), dim3(BLOCK),
                       0, s, *a, pass);
  LUX_POST_LAUNCH(stream);
}

// what 0: colour[v] = v and every alive v into st.qw; what 1: the roots
// (colour[v] == v) get st.bit and go into st.qw. Both restart the cursors
// meta[st.mw] and the hubq one at 0.
void lux_gpu_scc_scan(uint64_t stream, const lux_scc_args* a,
                      const lux_scc_step* st, int what) {
  if (!a->nv) return;
  hipStream_t s = (hipStream_t)stream;
  scc_zero(s, a->meta + st->mw);
  scc_zero(s, a->meta + S_HUBTAIL);
  hipLaunchKernelGGL(scc_scan_kernel, dim3(grid_for(a->nv)), dim3(BLOCK), 0, s,
                     *a, *st, what);
  LUX_POST_LAUNCH(stream);
}

// The vertex v gets st.bit and is appended to st.qw; restart != 0 puts the
// cursors meta[st.mw] and the hubq one back to 0 first.
void lux_gpu_scc_seed(uint64_t stream, const lux_scc_args* a,
                      const lux_scc_step* st, V_ID v, int restart) {
  if (v >= a->nv) return;
  hipStream_t s = (hipStream_t)stream;
  if (restart) {
    scc_zero(s, a->meta + st->mw);
    scc_zero(s, a->meta + S_HUBTAIL);
  }
  hipLaunchKernelGGL(scc_seed_kernel, dim3(1), dim3(WAVE), 0, s, *a, *st, v);
  LUX_POST_LAUNCH(stream);
}

// One step: st.qr[head : tail) and the hubq items [hubhead, hubtail) of the
// read half. restart != 0 (colour: the write half is the other one) zeroes
// the cursors meta[st.mw] and the hubq one first. Returns -1 (and launches
// nothing) on cursors out of order or beyond the lists.
int lux_gpu_scc_step(uint64_t stream, const lux_scc_args* a,
                     const lux_scc_step* st, uint32_t head, uint32_t tail,
                     uint32_t hubhead, uint32_t hubtail, int restart) {
  if (!scc_step_ok(*a, *st) || tail > st->qcap || head > tail ||
      hubtail > st->hcap || hubhead > hubtail)
    return -1;
  const uint32_t n = tail - head, nh = hubtail - hubhead;
  hipStream_t s = (hipStream_t)stream;
  if (restart) {
    scc_zero(s, a->meta + st->mw);
    scc_zero(s, a->meta + S_HUBTAIL);
  }
  if (!n && !nh) return 0;
  uint32_t rb = ceil_div_u32(n, BLOCK / WAVE);
  if (rb > (uint32_t)SCC_MAX_GRID) rb = SCC_MAX_GRID;
  uint32_t hb = nh > (uint32_t)SCC_MAX_GRID ? SCC_MAX_GRID : nh;
  hipLaunchKernelGGL(scc_step_kernel, dim3(rb + hb), dim3(BLOCK), 0, s, *a,
                     *st, head, tail, hubhead, hubtail, rb);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// Steps from st.qr[head : tail) on, in one workgroup, while they hold at
// most fuse entries and no hub item. Leaves meta[S_FUSED] = steps done and
// meta[S_HEAD] = the first entry not processed (append mode). Returns -1
// (and launches nothing) if the first step does not qualify.
int lux_gpu_scc_tail(uint64_t stream, const lux_scc_args* a,
                     const lux_scc_step* st, uint32_t head, uint32_t tail,
                     uint32_t hubtail, uint32_t fuse, int pingpong) {
  if (!scc_step_ok(*a, *st) || !fuse || fuse > SCC_FUSE_MAX ||
      tail > st->qcap || head >= tail || tail - head > fuse ||
      hubtail > st->hcap)
    return -1;
  hipStream_t s = (hipStream_t)stream;
  if (pingpong) {
    scc_zero(s, a->meta + st->mw);
    scc_zero(s, a->meta + S_HUBTAIL);
  }
  hipLaunchKernelGGL(scc_tail_kernel, dim3(1), dim3(SCC_TAIL_BLOCK), 0, s, *a,
                     *st, head, tail, hubtail, fuse, pingpong);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// colour == 0: the vertices with F and B get the largest id among them
// (meta[S_MAXID]); colour != 0: the alive vertices with B get their colour.
// meta[S_DIED] = how many died.
void lux_gpu_scc_commit(uint64_t stream, const lux_scc_args* a, int colour) {
  if (!a->nv) return;
  hipStream_t s = (hipStream_t)stream;
  scc_zero(s, a->meta + S_DIED, 2);  // and S_MAXID
  int grid = grid_for(a->nv);
  if (colour) {
    hipLaunchKernelGGL(scc_commit_kernel, dim3(grid), dim3(BLOCK), 0, s, *a, 2);
  } else {
    hipLaunchKernelGGL(scc_commit_kernel, dim3(grid), dim3(BLOCK), 0, s, *a, 0);
    hipLaunchKernelGGL(scc_commit_kernel, dim3(grid), dim3(BLOCK), 0, s, *a, 1);
  }
  LUX_POST_LAUNCH(stream);
}

// what 0: range and idempotence of label, and fwd / bwd seeded at the
// roots; what 1: the vertices fwd or bwd never reached. bad is added to.
void lux_gpu_scc_check_vertex(uint64_t stream, V_ID nv, const uint32_t* label,
                              uint32_t* fwd, uint32_t* bwd,
                              unsigned long long* bad, int what) {
  if (!nv) return;
  hipLaunchKernelGGL(scc_check_vertex_kernel, dim3(grid_for(nv)), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, label, fwd, bwd, bad, what);
  LUX_POST_LAUNCH(stream);
}

// One launch of the reachability sweep; *changed is set if a flag was.
void lux_gpu_scc_check_sweep(uint64_t stream, V_ID nv, const E_ID* in_ptr,
                             const V_ID* in_col, const E_ID* out_ptr,
                             const V_ID* out_col, const uint32_t* label,
                             uint32_t* fwd, uint32_t* bwd, uint32_t* changed) {
  if (!nv) return;
  hipLaunchKernelGGL(scc_check_sweep_kernel, dim3(grid_for(nv)), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, in_ptr, in_col, out_ptr,
                     out_col, label, fwd, bwd, changed);
  LUX_POST_LAUNCH(stream);
}

// bad += the edges u -> v between different labels whose reverse exists.
void lux_gpu_scc_check_pairs(uint64_t stream, V_ID nv, E_ID ne,
                             const E_ID* in_ptr, const V_ID* in_col,
                             const E_ID* out_ptr, const V_ID* out_col,
                             const uint32_t* label, unsigned long long* bad) {
  if (!nv || !ne) return;
  hipLaunchKernelGGL(scc_check_pairs_kernel, dim3(grid_for(ne)), dim3(BLOCK),
                     0, (hipStream_t)stream, nv, ne, in_ptr, in_col, out_ptr,
                     out_col, label, bad);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
