// Bit-parallel multi-source BFS (MS-BFS, Then et al., VLDB 2014) on one GPU:
// every vertex carries one 64-bit word per state array, bit i belongs to
// source i of the batch, and one pass over an edge relaxes it for all 64
// sources with a single OR. No reference equivalent.
//
// State per vertex: seen (reached so far), front (reached at the last level),
// next (the level being discovered, zero between levels). A level is one
// traversal launch, pull or push, followed by the epilogue launch; the host
// reads the meta record once per level and picks the next direction from it.
//
//   pull  (CSC rows): next[v] = OR front[u] over the in-neighbours u, the
//         scan stopping once (acc | seen[v]) == active. Rows saturated before
//         the level (seen[v] == active) are not opened at all. Three static
//         role lists by in-degree: one lane per short row; one wave per row,
//         64 eight-byte gathers per step, a butterfly OR over the wave and
//         the exit test once per step; rows longer than hub in chunks of hub
//         entries, one workgroup per {vertex, chunk} item, OR-reduced through
//         LDS into one 64-bit atomic OR, a chunk skipping itself when
//         next[v] | seen[v] is already saturated.
//   push  (out-edge CSR): for every queued u and out-neighbour v,
//         w = front[u] & ~seen[v], and an atomic OR into next[v] only when
//         w != 0. The same three roles by out-degree, taken from the three
//         queues the epilogue wrote.
//   epilogue (all vertices): new = next & ~seen, seen |= new, front = new,
//         next = 0, the per-vertex sums, the optional depth rows, the queues
//         of the next level (one atomic per wave and role) and the meta
//         record. The 64 per-source counts are a bit-matrix column sum: a
//         wave whose 64 new words are all zero skips it, otherwise one ballot
//         per source bit, lane i keeps the count of bit i, 64 LDS counters
//         per workgroup and one global atomic per non-zero counter.
//
// Every accumulated value is an OR, an integer add, or is written by exactly
// one thread per vertex and level, so push and pull levels give identical
// bits. The meta record is written with vector atomics only.
#include "gpu_common.h"
#include "lux/gpu_api.h"

namespace lux {

typedef unsigned long long u64;

constexpr uint32_t MSBFS_HUB = 1024;      // default longest wave-role row
constexpr uint32_t MSBFS_HUB_MAX = 1u << 20;
constexpr uint32_t MSBFS_THREAD = 16;     // longest thread-role row
constexpr uint32_t MSBFS_PULL_DIV = 8;    // pull iff volume * div > ne
constexpr uint32_t MSBFS_BATCH = 64;      // sources per word
constexpr int MSBFS_MAX_GRID = 1 << 14;   // blocks per role
constexpr int MSBFS_NW = BLOCK / WAVE;

// meta record, u64 words, zeroed by the host before every level
enum {
  MM_FRONT,    // vertices with a new bit = the next frontier
  MM_VOLUME,   // sum of their out-degrees
  MM_PAIRS,    // new (source, vertex) pairs
  MM_NTHR,     // entries of qthr
  MM_NWAV,     // entries of qwav
  MM_NHUB,     // items of qhub
  MM_SCANNED,  // edge entries the traversal launch read
  MM_PAD,
  MM_SRC,      // 64 per-source counts of this level
  MM_WORDS = MM_SRC + MSBFS_BATCH
};

__device__ __forceinline__ u64 wave_or(u64 x) {
  for (int off = WAVE / 2; off > 0; off >>= 1) x |= __shfl_xor(x, off, WAVE);
  return x;  // in every lane
}

__device__ __forceinline__ void add_scanned(const lux_msbfs_args& a,
                                            u64 scanned) {
  scanned = wave_reduce_sum(scanned);
  if ((threadIdx.x & (WAVE - 1)) == 0 && scanned)
    atomicAdd(&a.meta[MM_SCANNED], scanned);
}

// Blocks [0, tb) run the thread role, [tb, tb + wb) the wave role, the last
// hb the hub items.
__global__ void __launch_bounds__(BLOCK)
msbfs_pull_kernel(lux_msbfs_args a, u64 active, uint32_t tb, uint32_t wb,
                  uint32_t hb) {
  __shared__ u64 part[MSBFS_NW];
  __shared__ u64 have_s;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x;
  u64 scanned = 0;
  if (b < tb) {
    for (uint64_t i = (uint64_t)b * BLOCK + threadIdx.x; i < a.n_thr_in;
         i += (uint64_t)tb * BLOCK) {
      const V_ID v = a.thr_in[i];
      const u64 s = a.seen[v];
      if (s == active) continue;
      const E_ID e0 = a.in_ptr[v], end = a.in_ptr[v + 1];
      E_ID e = e0;
      u64 acc = 0;
      while (e < end) {
        acc |= a.front[a.in_col[e++]];
        if ((acc | s) == active) break;
      }
      scanned += e - e0;
      if (acc) a.next[v] = acc;
    }
  } else if (b < tb + wb) {
    for (uint64_t i = (uint64_t)(b - tb) * MSBFS_NW + wid; i < a.n_wav_in;
         i += (uint64_t)wb * MSBFS_NW) {
      const V_ID v = a.wav_in[i];
      const u64 s = a.seen[v];
      if (s == active) continue;  // the whole wave
      const E_ID end = a.in_ptr[v + 1];
      u64 acc = 0;
      for (E_ID base = a.in_ptr[v]; base < end; base += WAVE) {
        const E_ID x = base + lane;
        acc |= wave_or(x < end ? a.front[a.in_col[x]] : 0ull);
        if (x < end) scanned++;
        if ((acc | s) == active) break;
      }
      if (lane == 0 && acc) a.next[v] = acc;
    }
  } else {
    for (uint64_t i = b - tb - wb; i < a.n_hub_in; i += hb) {
      const V_ID v = a.hub_in[2 * i];
      const uint32_t c = a.hub_in[2 * i + 1];
      const u64 s = a.seen[v];
      if (threadIdx.x == 0)
        have_s = __atomic_load_n(&a.next[v], __ATOMIC_RELAXED) | s;
      __syncthreads();
      if (have_s != active) {  // the whole workgroup
        const E_ID r0 = a.in_ptr[v] + (E_ID)c * a.hub;
        const E_ID rest = a.in_ptr[v + 1] - r0;
        const E_ID r1 = r0 + (rest < a.hub ? rest : (E_ID)a.hub);
        u64 acc = 0;
        for (E_ID x = r0 + threadIdx.x; x < r1; x += BLOCK) {
          acc |= a.front[a.in_col[x]];
          scanned++;
        }
        acc = wave_or(acc);
        if (lane == 0) part[wid] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
          acc = 0;
          for (int w = 0; w < MSBFS_NW; w++) acc |= part[w];
          acc &= ~s;
          if (acc) atomicOr(&a.next[v], acc);
        }
      }
      __syncthreads();  // part and have_s are reused by the next item
    }
  }
  add_scanned(a, scanned);
}

__device__ __forceinline__ void push_edge(const lux_msbfs_args& a, u64 f,
                                          E_ID x) {
  const V_ID v = a.out_col[x];
  const u64 w = f & ~a.seen[v];
  if (w) atomicOr(&a.next[v], w);
}

// The queues of this level: nthr entries of qthr, nwav of qwav, nhub items
// of qhub. The same block split as the pull kernel.
__global__ void __launch_bounds__(BLOCK)
msbfs_push_kernel(lux_msbfs_args a, uint32_t nthr, uint32_t nwav,
                  uint32_t nhub, uint32_t tb, uint32_t wb, uint32_t hb) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x;
  u64 scanned = 0;
  if (b < tb) {
    for (uint64_t i = (uint64_t)b * BLOCK + threadIdx.x; i < nthr;
         i += (uint64_t)tb * BLOCK) {
      const V_ID u = a.qthr[i];
      const u64 f = a.front[u];
      const E_ID e0 = a.out_ptr[u], end = a.out_ptr[u + 1];
      for (E_ID x = e0; x < end; x++) push_edge(a, f, x);
      scanned += end - e0;
    }
  } else if (b < tb + wb) {
    for (uint64_t i = (uint64_t)(b - tb) * MSBFS_NW + wid; i < nwav;
         i += (uint64_t)wb * MSBFS_NW) {
      const V_ID u = a.qwav[i];
      const u64 f = a.front[u];
      const E_ID end = a.out_ptr[u + 1];
      for (E_ID x = a.out_ptr[u] + lane; x < end; x += WAVE) {
        push_edge(a, f, x);
        scanned++;
      }
    }
  } else {
    for (uint64_t i = b - tb - wb; i < nhub; i += hb) {
      const V_ID u = a.qhub[2 * i];
      const uint32_t c = a.qhub[2 * i + 1];
      const u64 f = a.front[u];
      const E_ID r0 = a.out_ptr[u] + (E_ID)c * a.hub;
      const E_ID rest = a.out_ptr[u + 1] - r0;
      const E_ID r1 = r0 + (rest < a.hub ? rest : (E_ID)a.hub);
      for (E_ID x = r0 + threadIdx.x; x < r1; x += BLOCK) {
        push_edge(a, f, x);
        scanned++;
      }
    }
  }
  add_scanned(a, scanned);
}

// Append the lanes of `mask` to a queue whose tail is meta word `word`: one
// atomic per wave. Called by the whole wave.
__device__ __forceinline__ void wave_append(const lux_msbfs_args& a,
                                            V_ID* queue, int word, u64 mask,
                                            bool mine, V_ID v, int lane) {
  if (!mask) return;
  const int leader = __ffsll(mask) - 1;
  u64 pos = 0;
  if (lane == leader) pos = atomicAdd(&a.meta[word], (u64)__popcll(mask));
  pos = __shfl(pos, leader, WAVE);
  if (mine) queue[pos + __popcll(mask & ((1ull << lane) - 1))] = v;
}

// Level d just discovered; k sources in this batch; depth: the batch's rows
// of the depth matrix (k rows of nv), or null.
__global__ void __launch_bounds__(BLOCK)
msbfs_epilogue_kernel(lux_msbfs_args a, uint32_t d, uint32_t k, int* depth) {
  __shared__ uint32_t cnt[MSBFS_BATCH];
  const int lane = threadIdx.x & (WAVE - 1);
  if (threadIdx.x < MSBFS_BATCH) cnt[threadIdx.x] = 0;
  __syncthreads();
  uint32_t colsum = 0;  // of source bit `lane`
  u64 nfront = 0, volume = 0, pairs = 0;
  const uint64_t nvr = ((uint64_t)a.nv + BLOCK - 1) / BLOCK * BLOCK;
  for (uint64_t base = (uint64_t)blockIdx.x * BLOCK; base < nvr;
       base += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t v = base + threadIdx.x;
    u64 nw = 0;
    E_ID deg = 0;
    int role = 0;
    if (v < a.nv) {
      const u64 n = a.next[v];
      u64 s = 0;
      if (n) {
        a.next[v] = 0;
        s = a.seen[v];
        nw = n & ~s;
      }
      a.front[v] = nw;
      if (nw) {
        const uint32_t pc = __popcll(nw);
        a.seen[v] = s | nw;
        a.reach[v] += pc;
        a.dist_sum[v] += (u64)d * pc;
        if (d) a.harmonic[v] += (double)pc / (double)d;
        if (depth)
          for (u64 m = nw; m; m &= m - 1)
            depth[(uint64_t)(__ffsll(m) - 1) * a.nv + v] = (int)d;
        deg = a.out_ptr[v + 1] - a.out_ptr[v];
        role = deg == 0 ? 0 : deg <= a.thr ? 1 : deg <= a.hub ? 2 : 3;
        nfront++;
        volume += deg;
        pairs += pc;
      }
    }
    if (!__ballot(nw != 0)) continue;  // the whole wave
    for (uint32_t i = 0; i < k; i++) {
      const u64 col = __ballot((nw >> i) & 1);
      if (lane == (int)i) colsum += __popcll(col);
    }
    wave_append(a, a.qthr, MM_NTHR, __ballot(role == 1), role == 1, (V_ID)v,
                lane);
    wave_append(a, a.qwav, MM_NWAV, __ballot(role == 2), role == 2, (V_ID)v,
                lane);
    if (role == 3) {  // rare: one atomic per hub row
      const uint32_t nc = (uint32_t)((deg + a.hub - 1) / a.hub);
      const u64 pos = atomicAdd(&a.meta[MM_NHUB], (u64)nc);
      for (uint32_t c = 0; c < nc; c++) {
        a.qhub[2 * (pos + c)] = (V_ID)v;
        a.qhub[2 * (pos + c) + 1] = c;
      }
    }
  }
  if (colsum) atomicAdd(&cnt[lane], colsum);
  __syncthreads();
  if (threadIdx.x < MSBFS_BATCH && cnt[threadIdx.x])
    atomicAdd(&a.meta[MM_SRC + threadIdx.x], (u64)cnt[threadIdx.x]);
  nfront = wave_reduce_sum(nfront);
  volume = wave_reduce_sum(volume);
  pairs = wave_reduce_sum(pairs);
  if (lane == 0 && nfront) {
    atomicAdd(&a.meta[MM_FRONT], nfront);
    atomicAdd(&a.meta[MM_VOLUME], volume);
    atomicAdd(&a.meta[MM_PAIRS], pairs);
  }
}

__global__ void msbfs_seed_kernel(lux_msbfs_args a, const V_ID* sources,
                                  uint32_t k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k && sources[i] < a.nv) a.next[sources[i]] = 1ull << i;
}

// Necessary conditions on one batch, one wave per vertex v: lane i compares
// the sign of depth[i][v] with bit i of seen[v]; the wave of v < k checks
// source v; the lanes then walk v's in-edges.
__global__ void __launch_bounds__(BLOCK)
msbfs_check_kernel(lux_msbfs_args a, const u64* seen, const int* depth,
                   const V_ID* sources, uint32_t k, u64* bad_out) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x >> 6;
  u64 bad = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * MSBFS_NW + wid; v < a.nv;
       v += (uint64_t)gridDim.x * MSBFS_NW) {
    const u64 sv = seen[v];
    if (depth && lane < (int)k &&
        (depth[(uint64_t)lane * a.nv + v] >= 0) != (bool)((sv >> lane) & 1))
      bad++;
    if (v < k && lane == 0) {
      const V_ID s = sources[v];
      if (s >= a.nv || !((seen[s] >> v) & 1)) bad++;
      if (depth && s < a.nv && depth[v * a.nv + s] != 0) bad++;
    }
    const E_ID end = a.in_ptr[v + 1];
    for (E_ID x = a.in_ptr[v] + lane; x < end; x += WAVE) {
      const V_ID u = a.in_col[x];
      const u64 su = seen[u];
      if (su & ~sv) bad++;
      if (!depth) continue;
      for (u64 m = su; m; m &= m - 1) {
        const uint64_t row = (uint64_t)(__ffsll(m) - 1) * a.nv;
        const int du = depth[row + u], dv = depth[row + v];
        if (du >= 0 && (dv < 0 || dv > du + 1)) bad++;
      }
    }
  }
  bad = wave_reduce_sum(bad);
  if (lane == 0 && bad) atomicAdd(bad_out, bad);
}

__host__ bool msbfs_args_ok(const lux_msbfs_args* a) {
  return a && a->nv && a->hub >= 1 && a->hub <= MSBFS_HUB_MAX &&
         a->thr == (a->hub < MSBFS_THREAD ? a->hub : MSBFS_THREAD) &&
         a->n_thr_in <= a->nv && a->n_wav_in <= a->nv;
}

__host__ uint32_t msbfs_blocks(uint64_t work, uint32_t per_block) {
  uint64_t g = (work + per_block - 1) / per_block;
  return (uint32_t)(g > (uint64_t)MSBFS_MAX_GRID ? MSBFS_MAX_GRID : g);
}

}  // namespace lux

using namespace lux;

extern "C" {

uint32_t lux_gpu_msbfs_hub_default() { return MSBFS_HUB; }
uint32_t lux_gpu_msbfs_hub_max() { return MSBFS_HUB_MAX; }
uint32_t lux_gpu_msbfs_thread_limit() { return MSBFS_THREAD; }
uint32_t lux_gpu_msbfs_pull_div_default() { return MSBFS_PULL_DIV; }
uint32_t lux_gpu_msbfs_meta_words() { return MM_WORDS; }

// next[sources[i]] = 1 << i for i < k; the epilogue of level 0 does the rest.
int lux_gpu_msbfs_seed(uint64_t stream, const lux_msbfs_args* a,
                       const lux::V_ID* sources, uint32_t k) {
  if (!msbfs_args_ok(a) || !sources || k < 1 || k > MSBFS_BATCH) return -1;
  hipLaunchKernelGGL(msbfs_seed_kernel, dim3(1), dim3(MSBFS_BATCH), 0,
                     (hipStream_t)stream, *a, sources, k);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_msbfs_pull(uint64_t stream, const lux_msbfs_args* a,
                       unsigned long long active) {
  if (!msbfs_args_ok(a) || !active) return -1;
  const uint32_t tb = msbfs_blocks(a->n_thr_in, BLOCK);
  const uint32_t wb = msbfs_blocks(a->n_wav_in, MSBFS_NW);
  const uint32_t hb = msbfs_blocks(a->n_hub_in, 1);
  if (!(tb + wb + hb)) return 0;
  hipLaunchKernelGGL(msbfs_pull_kernel, dim3(tb + wb + hb), dim3(BLOCK), 0,
                     (hipStream_t)stream, *a, active, tb, wb, hb);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_msbfs_push(uint64_t stream, const lux_msbfs_args* a,
                       uint32_t nthr, uint32_t nwav, uint32_t nhub) {
  if (!msbfs_args_ok(a) || nthr > a->nv || nwav > a->nv ||
      nhub > a->hubcap_out)
    return -1;
  const uint32_t tb = msbfs_blocks(nthr, BLOCK);
  const uint32_t wb = msbfs_blocks(nwav, MSBFS_NW);
  const uint32_t hb = msbfs_blocks(nhub, 1);
  if (!(tb + wb + hb)) return 0;
  hipLaunchKernelGGL(msbfs_push_kernel, dim3(tb + wb + hb), dim3(BLOCK), 0,
                     (hipStream_t)stream, *a, nthr, nwav, nhub, tb, wb, hb);
  LUX_POST_LAUNCH(stream);
  return 0;
}

int lux_gpu_msbfs_epilogue(uint64_t stream, const lux_msbfs_args* a,
                           uint32_t d, uint32_t k, int* depth) {
  if (!msbfs_args_ok(a) || k < 1 || k > MSBFS_BATCH) return -1;
  hipLaunchKernelGGL(msbfs_epilogue_kernel, dim3(grid_for(a->nv)),
                     dim3(BLOCK), 0, (hipStream_t)stream, *a, d, k, depth);
  LUX_POST_LAUNCH(stream);
  return 0;
}

// bad (one u64, added to): the violations in one batch. seen: the batch's
// words; depth: its k rows of the depth matrix, or null.
int lux_gpu_msbfs_check(uint64_t stream, const lux_msbfs_args* a,
                        const unsigned long long* seen, const int* depth,
                        const lux::V_ID* sources, uint32_t k,
                        unsigned long long* bad) {
  if (!msbfs_args_ok(a) || !seen || !sources || !bad || k < 1 ||
      k > MSBFS_BATCH || k > a->nv)
    return -1;
  hipLaunchKernelGGL(msbfs_check_kernel,
                     dim3(msbfs_blocks(a->nv, MSBFS_NW)), dim3(BLOCK), 0,
                     (hipStream_t)stream, *a, seen, depth, sources, k, bad);
  LUX_POST_LAUNCH(stream);
  return 0;
}

}  // extern "C"
