// Push-model engine: frontier-driven scatter along out-edges, with the
// reference's adaptive dense-bitmap / sparse-queue frontier representation
// (FrontierHeader, core/graph.h:100-106) and first-improvement enqueue
// (process_edge_sparse, sssp_gpu.cu:63-82) re-validated on CDNA4 atomics.
//
// Structures per rank: a "push CSR" mapping EVERY source vertex to its
// out-edges that land in THIS rank's partition (the reference's
// push_row_ptr/push_col_idx of size nv per GPU, core/push_model.inl:321-324),
// built with a device-wide scan instead of the reference's serial
// single-thread prefix sum (sssp_gpu.cu:550-565).
//
// Per iteration the Python engine: snapshots labels, reads all P segment
// headers, picks push vs pull fallback (oldFqSize > nv/16, sssp_gpu.cu:414),
// launches one scatter per source segment, then bitmap/d2s fix-ups — all on
// one HIP stream; exchange is RCCL all-gather(v) (lux_amd/push_engine.py).
#include "gpu_common.h"

namespace lux {

// min (SSSP hop) / max (CC label) relaxation semantics.
template <bool IS_MIN> struct LabOp;
template <> struct LabOp<true> {
  static __device__ __forceinline__ uint32_t map(uint32_t src_label) {
    return src_label + 1;  // hop relaxation; sources in a frontier are finite
  }
  static __device__ __forceinline__ bool better(uint32_t a, uint32_t b) {
    return a < b;
  }
  static __device__ __forceinline__ uint32_t atom(uint32_t* p, uint32_t v) {
    return atomicMin(p, v);
  }
};
template <> struct LabOp<false> {
  static __device__ __forceinline__ uint32_t map(uint32_t src_label) {
    return src_label;  // CC propagates the label itself
  }
  static __device__ __forceinline__ bool better(uint32_t a, uint32_t b) {
    return a > b;
  }
  static __device__ __forceinline__ uint32_t atom(uint32_t* p, uint32_t v) {
    return atomicMax(p, v);
  }
};

// ---------------- push CSR build ----------------

__global__ void csr_scatter_kernel(uint64_t ep, const V_ID* col,
                                   const E_ID* row_ptr_loc, V_ID vp,
                                   V_ID row_left,
                                   unsigned long long* cursor,
                                   V_ID* push_col) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < ep;
       j += stride) {
    // binary search: dst row v with row_ptr[v] <= j < row_ptr[v+1]
    V_ID lo = 0, hi = vp - 1;
    while (lo < hi) {
      V_ID mid = (lo + hi + 1) >> 1;
      if (row_ptr_loc[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    V_ID src = col[j];
    unsigned long long pos = atomicAdd(&cursor[src], 1ull);
    push_col[pos] = lo + row_left;  // global dst id
  }
}

// ---------------- edge-balanced scatter (expand + chunk) ----------------
// The reference's kernel (sssp_gpu.cu:132-246) drains each
// 256-frontier-vertex group in ONE block, so a hub's whole out-edge range
// serializes there (measured with a faithful port: the 1-vertex first SSSP
// iteration from RMAT-27's root took 58 ms — one block walked ~4M edges
// while 255 CUs idled; the 902K-vertex second iteration 104 ms on its
// worst block). The MI355X design splits every active vertex's range into
// <=PUSH_CHUNK-edge work items first (LDS-aggregated append), then one
// grid covers all items — edge-balanced regardless of degree skew, and
// one launch per iteration instead of one per source segment.

constexpr V_ID PUSH_CHUNK = 8192;

// counter[0] = work items; counter[1] = low word of the segment's out-edge
// total (debug only — decisions use the exchanged u64 meta edge volume);
// counter[3] = overflow flag, set when items exceed max_items (VERDICT r1
// weak #6: silent truncation becomes a loud signal; the engine recovers
// with a forced pull iteration, which re-relaxes every edge).
// qlabels/labels_repair (nullable): sparse queues travel with a label
// annex so peers can skip the full label all-gather on sparse iterations;
// expand repairs the stale replicated labels[u] from the annex before the
// scatter reads them.
__global__ void frontier_expand_kernel(int old_dense, V_ID in_row_left,
                                       V_ID in_count,
                                       const uint8_t* old_seg,
                                       const uint32_t* qlabels,
                                       uint32_t* labels_repair,
                                       const E_ID* push_row_ptr,
                                       uint2* items, uint32_t* counter,
                                       uint32_t max_items) {
  __shared__ uint32_t lds_scan[BLOCK / WAVE + 1];
  __shared__ unsigned long long lds_red[BLOCK / WAVE];
  __shared__ uint32_t blk_base;
  const uint8_t* bitmap = old_seg + sizeof(FrontierHeader);
  const V_ID* queue = (const V_ID*)(old_seg + sizeof(FrontierHeader));
  for (V_ID blk = blockIdx.x * blockDim.x; blk < in_count;
       blk += blockDim.x * gridDim.x) {
    V_ID idx = blk + threadIdx.x;
    V_ID u = 0;
    uint32_t nch = 0;
    E_ID deg = 0;
    if (idx < in_count) {
      bool active;
      if (old_dense) {
        u = in_row_left + idx;
        active = (bitmap[idx >> 3] >> (idx & 7)) & 1;
      } else {
        u = queue[idx];
        active = true;
        if (labels_repair && qlabels) labels_repair[u] = qlabels[idx];
      }
      if (active) {
        deg = push_row_ptr[u + 1] - push_row_ptr[u];
        nch = (uint32_t)((deg + PUSH_CHUNK - 1) / PUSH_CHUNK);
      }
    }
    unsigned long long esum =
        block_reduce_sum((unsigned long long)deg, lds_red);
    uint32_t total;
    uint32_t ex = block_exscan<uint32_t, BLOCK>(nch, lds_scan, &total);
    if (threadIdx.x == 0) {
      blk_base = total ? atomicAdd(counter, total) : 0;
      if (esum) atomicAdd(&counter[1], (uint32_t)esum);
      if (total && blk_base + total > max_items) counter[3] = 1;
    }
    __syncthreads();
    for (uint32_t c = 0; c < nch; c++) {
      uint32_t pos = blk_base + ex + c;
      if (pos < max_items) items[pos] = make_uint2(u, c);
    }
    __syncthreads();
  }
}

// Device-sized expand: reads the segment's OWN header (type + count) so
// every launch dimension is static — the single-GPU engine captures the
// whole push iteration into a hipGraph and replays it (one launch + one
// 32 B meta read per iteration instead of ~12 ctypes calls; the same
// lever as the pull-body capture). Grid is fixed; the loop strides over
// whatever count the header holds.
__global__ void frontier_expand_auto_kernel(V_ID verts, V_ID in_row_left,
                                            const uint8_t* seg,
                                            const uint32_t* qlabels,
                                            uint32_t* labels_repair,
                                            const E_ID* push_row_ptr,
                                            uint2* items, uint32_t* counter,
                                            uint32_t max_items) {
  __shared__ uint32_t lds_scan[BLOCK / WAVE + 1];
  __shared__ unsigned long long lds_red[BLOCK / WAVE];
  __shared__ uint32_t blk_base;
  const FrontierHeader* h = (const FrontierHeader*)seg;
  int dense = h->type == FrontierHeader::DENSE_BITMAP;
  V_ID in_count = dense ? verts : h->numNodes;
  const uint8_t* bitmap = seg + sizeof(FrontierHeader);
  const V_ID* queue = (const V_ID*)(seg + sizeof(FrontierHeader));
  for (V_ID blk = blockIdx.x * blockDim.x; blk < in_count;
       blk += blockDim.x * gridDim.x) {
    V_ID idx = blk + threadIdx.x;
    V_ID u = 0;
    uint32_t nch = 0;
    E_ID deg = 0;
    if (idx < in_count) {
      bool active;
      if (dense) {
        u = in_row_left + idx;
        active = (bitmap[idx >> 3] >> (idx & 7)) & 1;
      } else {
        u = queue[idx];
        active = true;
        if (labels_repair && qlabels) labels_repair[u] = qlabels[idx];
      }
      if (active) {
        deg = push_row_ptr[u + 1] - push_row_ptr[u];
        nch = (uint32_t)((deg + PUSH_CHUNK - 1) / PUSH_CHUNK);
      }
    }
    unsigned long long esum =
        block_reduce_sum((unsigned long long)deg, lds_red);
    uint32_t total;
    uint32_t ex = block_exscan<uint32_t, BLOCK>(nch, lds_scan, &total);
    if (threadIdx.x == 0) {
      blk_base = total ? atomicAdd(counter, total) : 0;
      if (esum) atomicAdd(&counter[1], (uint32_t)esum);
      if (total && blk_base + total > max_items) counter[3] = 1;
    }
    __syncthreads();
    for (uint32_t c = 0; c < nch; c++) {
      uint32_t pos = blk_base + ex + c;
      if (pos < max_items) items[pos] = make_uint2(u, c);
    }
    __syncthreads();
  }
}

// BFS (IS_MIN) fast path: hop-SSSP is level-synchronous BFS — every vertex
// in an iteration's frontier carries the same depth, and a finite label is
// final (the settled-skip invariant in pull.hip). Discovery is therefore a
// one-shot test-and-set against a per-partition VISITED BITMAP (vp/8 bytes
// — ~2 MB at RMAT-27/8 ranks, 16.8 MB at 1 rank: L2/LLC-resident) instead
// of an atomicMin against the 4*vp-byte label array; the label is written
// once, on discovery. NOT valid for general min-plus relaxation (two
// frontier labels could race to a non-min value) — the engine enables it
// only for its single-source hop traversal; IS_MIN without a bitmap and
// CC (IS_MAX) keep the label-atomic path.
template <bool IS_MIN, bool NEW_DENSE, bool BFS_BITS>
__global__ void push_chunk_scatter_kernel(
    const uint2* items, const uint32_t* counter, uint32_t max_items,
    const E_ID* push_row_ptr, const V_ID* push_col,
    const uint32_t* old_labels, const uint32_t* snapshot,
    uint32_t* new_labels, V_ID my_row_left, uint8_t* new_seg,
    V_ID capacity, uint32_t* visited_bits) {
  using OP = LabOp<IS_MIN>;
  __shared__ uint32_t lds_scan[BLOCK / WAVE + 1];
  __shared__ uint32_t queue_base;
  V_ID* new_queue = nullptr;
  uint32_t* num_nodes = nullptr;
  if (!NEW_DENSE) {
    num_nodes = &((FrontierHeader*)new_seg)->numNodes;
    new_queue = (V_ID*)(new_seg + sizeof(FrontierHeader));
  }
  uint32_t n = *counter;
  if (n > max_items) n = max_items;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    uint2 it = items[i];
    V_ID u = it.x;
    uint32_t new_lab = OP::map(old_labels[u]);
    E_ID b = push_row_ptr[u] + (E_ID)it.y * PUSH_CHUNK;
    E_ID e = push_row_ptr[u + 1];
    if (e > b + PUSH_CHUNK) e = b + PUSH_CHUNK;
    uint32_t nstripes =
        (uint32_t)((e - b + blockDim.x - 1) / blockDim.x);
    // dense-output path: no block-wide scan per stripe, so 4 stripes are
    // processed per pass — 4 col loads then 4 dependent visited/label
    // line reads in flight (same MLP lever as pull.hip gather_range; the
    // hub-explosion iteration is LLC-random-line-bound)
    if (NEW_DENSE) {
      uint32_t s = 0;
      for (; s + 4 <= nstripes; s += 4) {
        E_ID k0 = b + (E_ID)s * blockDim.x + threadIdx.x;
        V_ID v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        bool p0 = k0 < e, p1 = k0 + blockDim.x < e,
             p2 = k0 + 2 * blockDim.x < e, p3 = k0 + 3 * blockDim.x < e;
        if (p0) v0 = push_col[k0];
        if (p1) v1 = push_col[k0 + blockDim.x];
        if (p2) v2 = push_col[k0 + 2 * blockDim.x];
        if (p3) v3 = push_col[k0 + 3 * blockDim.x];
#define LUX_PD_EDGE(P_, V_)                                                 \
        if (P_) {                                                           \
          V_ID lv = (V_) - my_row_left;                                     \
          if (BFS_BITS) {                                                   \
            uint32_t word = visited_bits[lv >> 5];                          \
            uint32_t bit = 1u << (lv & 31);                                 \
            if (!(word & bit)) {                                            \
              uint32_t old = atomicOr(&visited_bits[lv >> 5], bit);         \
              if (!(old & bit)) new_labels[lv] = new_lab;                   \
            }                                                               \
          } else {                                                          \
            uint32_t* slot = &new_labels[lv];                               \
            uint32_t cur = __hip_atomic_load(slot, __ATOMIC_RELAXED,        \
                                             __HIP_MEMORY_SCOPE_AGENT);     \
            if (OP::better(new_lab, cur)) OP::atom(slot, new_lab);          \
          }                                                                 \
        }
        LUX_PD_EDGE(p0, v0)
        LUX_PD_EDGE(p1, v1)
        LUX_PD_EDGE(p2, v2)
        LUX_PD_EDGE(p3, v3)
      }
      for (; s < nstripes; s++) {
        E_ID k = b + (E_ID)s * blockDim.x + threadIdx.x;
        if (k < e) {
          V_ID v = push_col[k];
          LUX_PD_EDGE(true, v)
        }
      }
#undef LUX_PD_EDGE
      continue;
    }
    for (uint32_t s = 0; s < nstripes; s++) {
      E_ID k = b + (E_ID)s * blockDim.x + threadIdx.x;
      uint32_t flag = 0;
      V_ID dstv = 0;
      if (k < e) {
        V_ID v = push_col[k];
        V_ID lv = v - my_row_left;
        if (BFS_BITS) {
          uint32_t word = visited_bits[lv >> 5];
          uint32_t bit = 1u << (lv & 31);
          if (!(word & bit)) {
            uint32_t old = atomicOr(&visited_bits[lv >> 5], bit);
            if (!(old & bit)) {  // this thread discovered v
              new_labels[lv] = new_lab;
              if (!NEW_DENSE) {
                flag = 1;
                dstv = v;
              }
            }
          }
        } else {
          uint32_t* slot = &new_labels[lv];
          uint32_t cur = __hip_atomic_load(slot, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
          if (OP::better(new_lab, cur)) {
            if (NEW_DENSE) {
              OP::atom(slot, new_lab);
            } else {
              // first-improvement enqueue (sssp_gpu.cu:63-82)
              uint32_t last = snapshot[lv];
              uint32_t act = OP::atom(slot, new_lab);
              if (act == last) {
                flag = 1;
                dstv = v;
              }
            }
          }
        }
      }
      if (!NEW_DENSE) {
        __syncthreads();
        uint32_t q_total;
        uint32_t q_off = block_exscan<uint32_t, BLOCK>(flag, lds_scan,
                                                       &q_total);
        if (threadIdx.x == 0 && q_total)
          queue_base = atomicAdd(num_nodes, q_total);
        __syncthreads();
        if (flag) {
          uint32_t pos = queue_base + q_off;
          if (pos < capacity) new_queue[pos] = dstv;
        }
        __syncthreads();
      }
    }
  }
}

// visited_bits[w] bit i <=> labels[32w+i] != INF (rebuilt after pull
// iterations, which write labels directly)
__global__ void bits_from_labels_kernel(V_ID vp, const uint32_t* labels,
                                        uint32_t* bits) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  V_ID nw = (vp + 31) / 32;
  for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < nw;
       w += stride) {
    uint32_t word = 0;
    V_ID base = (V_ID)w * 32;
    int n = vp - base < 32 ? (int)(vp - base) : 32;
    for (int i = 0; i < n; i++)
      if (labels[base + i] != INF_LABEL) word |= 1u << i;
    bits[w] = word;
  }
}

// ---------------- frontier representation fix-ups ----------------

// Build my dense output bitmap + count: bit v <=> snapshot[v]!=new[v]
// (bitmap_kernel, sssp_gpu.cu:248-281). guard (nullable): device-side
// predication for the fixup chain — run only when *guard == want, so the
// host never needs to read the frontier count mid-iteration.
__global__ void build_bitmap_kernel(V_ID vp, const uint32_t* snapshot,
                                    const uint32_t* new_labels,
                                    uint8_t* seg, const uint32_t* guard,
                                    uint32_t want) {
  if (guard && *guard != want) return;
  __shared__ uint32_t lds[BLOCK / WAVE];
  uint32_t* num_nodes = &((FrontierHeader*)seg)->numNodes;
  uint8_t* bitmap = seg + sizeof(FrontierHeader);
  V_ID nbytes = (vp + 7) / 8;
  uint32_t cnt = 0;
  for (V_ID i = blockIdx.x * blockDim.x + threadIdx.x; i < nbytes;
       i += blockDim.x * gridDim.x) {
    uint8_t byte = 0;
    for (int b = 0; b < 8; b++) {
      V_ID v = i * 8 + b;
      if (v < vp && snapshot[v] != new_labels[v]) {
        byte |= (1u << b);
        cnt++;
      }
    }
    bitmap[i] = byte;
  }
  cnt = block_reduce_sum(cnt, lds);
  if (threadIdx.x == 0 && cnt) atomicAdd(num_nodes, cnt);
}

// Dense bitmap -> sparse queue (convert_d2s_kernel, sssp_gpu.cu:283-315).
// Queue entries are GLOBAL vertex ids.
__global__ void d2s_kernel(V_ID vp, V_ID row_left, const uint8_t* dense_seg,
                           uint8_t* sparse_seg, const uint32_t* guard,
                           uint32_t want) {
  if (guard && *guard != want) return;
  __shared__ uint32_t lds[BLOCK / WAVE + 1];
  __shared__ uint32_t qbase;
  const uint8_t* bitmap = dense_seg + sizeof(FrontierHeader);
  uint32_t* num_nodes = &((FrontierHeader*)sparse_seg)->numNodes;
  V_ID* queue = (V_ID*)(sparse_seg + sizeof(FrontierHeader));
  for (V_ID blk = blockIdx.x * blockDim.x; blk < vp;
       blk += blockDim.x * gridDim.x) {
    V_ID v = blk + threadIdx.x;
    uint32_t flag = 0;
    if (v < vp) flag = (bitmap[v >> 3] >> (v & 7)) & 1;
    __syncthreads();
    uint32_t total;
    uint32_t off = block_exscan<uint32_t, BLOCK>(flag, lds, &total);
    if (threadIdx.x == 0 && total) qbase = atomicAdd(num_nodes, total);
    __syncthreads();
    if (flag) queue[qbase + off] = v + row_left;
    __syncthreads();
  }
}

// ---------------- device-side fixup chain (zero host syncs) ----------
// r1 read the frontier count 1-3x per iteration on the host to drive the
// dense<->sparse conversions (sssp_gpu.cu:462-491 reads headers in host
// task code, hidden there by Legion's 4-deep window). Here the whole
// decision chain runs on device, predicated on meta[5]; the single host
// read per iteration is the exchanged 8-word meta record.
//
// meta layout (u32[8] per rank): [0]=type [1]=count [2..3]=u64 out-edge
// volume of the new frontier (global out-degrees of its vertices — the
// engine's exact push-vs-pull input for the NEXT iteration) [4]=expand
// overflow flag [5]=fixup flag scratch (1=convert d2s, 2=rebuild dense)
// [6..7]=pad; the bucketed schedule keeps the minimum deferred label and
// the deferred count there (bucket_select_kernel) — nothing in this chain
// touches them.

__global__ void fixup_decide_kernel(int built_dense, V_ID capacity,
                                    uint8_t* new_seg, uint8_t* tmp_seg,
                                    uint32_t* meta) {
  FrontierHeader* h = (FrontierHeader*)new_seg;
  FrontierHeader* t = (FrontierHeader*)tmp_seg;
  uint32_t n = h->numNodes;
  uint32_t flag = 0;
  if (built_dense) {
    if (n < (uint32_t)capacity) {  // dense result fits sparse: convert
      flag = 1;
      t->type = FrontierHeader::SPARSE_QUEUE;
      t->numNodes = 0;
    } else {
      h->type = FrontierHeader::DENSE_BITMAP;
    }
  } else {
    if (n >= (uint32_t)capacity) {  // sparse overflow: rebuild as bitmap
      flag = 2;
      t->type = FrontierHeader::DENSE_BITMAP;
      t->numNodes = 0;
    } else {
      h->type = FrontierHeader::SPARSE_QUEUE;
    }
  }
  meta[5] = flag;
  *(unsigned long long*)(meta + 2) = 0ull;  // evol accumulator
}

// Copy the finished tmp segment back over new_seg (guarded; byte count
// depends on which conversion ran).
__global__ void seg_copy_kernel(V_ID vp, const uint8_t* tmp_seg,
                                uint8_t* new_seg, const uint32_t* meta) {
  uint32_t flag = meta[5];
  if (!flag) return;
  const FrontierHeader* t = (const FrontierHeader*)tmp_seg;
  uint32_t nbytes = (flag == 1)
                        ? (uint32_t)sizeof(FrontierHeader) + 4u * t->numNodes
                        : (uint32_t)sizeof(FrontierHeader) + (vp + 7) / 8;
  uint32_t nwords = (nbytes + 3) / 4;
  const uint32_t* src = (const uint32_t*)tmp_seg;
  uint32_t* dst = (uint32_t*)new_seg;
  uint32_t stride = blockDim.x * gridDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
       i += stride)
    dst[i] = src[i];
}

// Fill the label annex of a (final) sparse segment: annex[i] = my final
// label of queue[i]. Runs AFTER all conversions, so annex labels are the
// iteration-final values (enqueue-time labels could be stale for CC's
// atomicMax path: a later better update would not re-enqueue).
__global__ void annex_fill_kernel(V_ID row_left, const uint8_t* seg,
                                  const uint32_t* labels_part,
                                  uint32_t* annex) {
  const FrontierHeader* h = (const FrontierHeader*)seg;
  if (h->type != FrontierHeader::SPARSE_QUEUE) return;
  uint32_t n = h->numNodes;
  const V_ID* q = (const V_ID*)(seg + sizeof(FrontierHeader));
  uint32_t stride = blockDim.x * gridDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    annex[i] = labels_part[q[i] - row_left];
}

// Final meta record: type/count from the finished segment, out-edge
// volume from the GLOBAL out-degrees of the new frontier's vertices
// (deg_part = global out-degree slice of my partition), overflow from the
// expand counter.
__global__ void seg_meta_kernel(V_ID vp, V_ID row_left, const uint8_t* seg,
                                const uint32_t* deg_part,
                                const uint32_t* item_counter,
                                uint32_t max_items, uint32_t* meta) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  const FrontierHeader* h = (const FrontierHeader*)seg;
  uint32_t type = h->type, n = h->numNodes;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    meta[0] = type;
    meta[1] = n;
    meta[4] = item_counter
                  ? (item_counter[3] | (item_counter[0] > max_items ? 1u : 0u))
                  : 0u;
    meta[5] = 0;
  }
  unsigned long long acc = 0;
  uint32_t stride = blockDim.x * gridDim.x;
  if (type == FrontierHeader::DENSE_BITMAP) {
    const uint8_t* bm = seg + sizeof(FrontierHeader);
    for (V_ID v = blockIdx.x * blockDim.x + threadIdx.x; v < vp; v += stride)
      if ((bm[v >> 3] >> (v & 7)) & 1) acc += deg_part[v];
  } else {
    const V_ID* q = (const V_ID*)(seg + sizeof(FrontierHeader));
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
      acc += deg_part[q[i] - row_left];
  }
  acc = block_reduce_sum(acc, lds);
  if (threadIdx.x == 0 && acc)
    atomicAdd((unsigned long long*)(meta + 2), acc);
}

// World-1 publish: labels slice copy predicated on the FINAL segment
// type (sparse iterations skip the O(nv) copy — queued labels ride the
// annex and expand repairs them; the distributed engine makes the same
// decision from the exchanged meta). Runs inside the captured iteration
// graph, where the host cannot branch on the fixup outcome.
__global__ void publish_labels_guarded_kernel(V_ID vp, const uint32_t* meta,
                                              const uint32_t* labels_part,
                                              uint32_t* labels_slice) {
  if (meta[0] != FrontierHeader::DENSE_BITMAP) return;
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < vp;
       i += stride)
    labels_slice[i] = labels_part[i];
}

// Check oracles on device (check_kernel, sssp_gpu.cu:773-798 /
// components_gpu.cu:767-791): count violations over my pull-CSC partition.
template <bool IS_MIN>
__global__ void check_kernel(V_ID vp, V_ID row_left, const E_ID* row_ptr_loc,
                             const V_ID* col, const uint32_t* labels,
                             unsigned long long* mistakes) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long cnt = 0;
  for (V_ID v = blockIdx.x * blockDim.x + threadIdx.x; v < vp;
       v += blockDim.x * gridDim.x) {
    uint32_t lab = labels[row_left + v];
    for (E_ID j = row_ptr_loc[v]; j < row_ptr_loc[v + 1]; j++) {
      uint32_t sl = labels[col[j]];
      if (IS_MIN) {
        uint32_t cand = sl == INF_LABEL ? INF_LABEL : sl + 1;
        if (lab > cand) cnt++;
      } else {
        if (lab < sl) cnt++;
      }
    }
  }
  cnt = block_reduce_sum(cnt, lds);
  if (threadIdx.x == 0 && cnt) atomicAdd(mistakes, cnt);
}

// ---------------- weighted SSSP (min-plus) ----------------
// Edge weights are the graph's i32 weights read as non-negative integers
// (the engine rejects negative ones at construction). The candidate
// saturates at 0xFFFFFFFE: a finite distance never becomes INF_LABEL and
// never wraps. These kernels sit next to the hop/CC ones, which stay as
// they are: a vertex's label can improve in several iterations here, so
// neither the visited bitmap nor a settled-row skip applies.

__device__ __forceinline__ uint32_t sat_add_label(uint32_t lab, uint32_t w) {
  unsigned long long c = (unsigned long long)lab + w;
  return c > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)c;
}

// Push CSR with the weight riding next to its dst: one interleaved
// {global dst, weight} per out-edge at the claimed cursor position, so the
// two can never drift apart under the non-deterministic cursor order and
// the scatter fetches an edge with one coalesced 8-byte load per lane.
__global__ void csr_scatter_w_kernel(uint64_t ep, const V_ID* col,
                                     const WeightType* weight,
                                     const E_ID* row_ptr_loc, V_ID vp,
                                     V_ID row_left,
                                     unsigned long long* cursor,
                                     uint2* push_edge) {
  uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < ep;
       j += stride) {
    V_ID lo = 0, hi = vp - 1;
    while (lo < hi) {
      V_ID mid = (lo + hi + 1) >> 1;
      if (row_ptr_loc[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    V_ID src = col[j];
    unsigned long long pos = atomicAdd(&cursor[src], 1ull);
    push_edge[pos] = make_uint2(lo + row_left, (uint32_t)weight[j]);
  }
}

// push_chunk_scatter_kernel's min-plus twin: same work items, chunking,
// grid-stride over the device-side count and the same two output shapes,
// but every edge carries its own candidate sat(old_labels[u] + w).
template <bool NEW_DENSE>
__global__ void push_chunk_scatter_w_kernel(
    const uint2* items, const uint32_t* counter, uint32_t max_items,
    const E_ID* push_row_ptr, const uint2* push_edge,
    const uint32_t* old_labels, const uint32_t* snapshot,
    uint32_t* new_labels, V_ID my_row_left, uint8_t* new_seg,
    V_ID capacity) {
  __shared__ uint32_t lds_scan[BLOCK / WAVE + 1];
  __shared__ uint32_t queue_base;
  V_ID* new_queue = nullptr;
  uint32_t* num_nodes = nullptr;
  if (!NEW_DENSE) {
    num_nodes = &((FrontierHeader*)new_seg)->numNodes;
    new_queue = (V_ID*)(new_seg + sizeof(FrontierHeader));
  }
  uint32_t n = *counter;
  if (n > max_items) n = max_items;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    uint2 it = items[i];
    V_ID u = it.x;
    uint32_t src_lab = old_labels[u];  // start-of-iteration value (Jacobi)
    E_ID b = push_row_ptr[u] + (E_ID)it.y * PUSH_CHUNK;
    E_ID e = push_row_ptr[u + 1];
    if (e > b + PUSH_CHUNK) e = b + PUSH_CHUNK;
    uint32_t nstripes =
        (uint32_t)((e - b + blockDim.x - 1) / blockDim.x);
    if (NEW_DENSE) {
      // 4 stripes per pass: 4 edge loads, then 4 dependent label-line
      // reads in flight (as in the hop kernel's dense path)
      uint32_t s = 0;
      for (; s + 4 <= nstripes; s += 4) {
        E_ID k0 = b + (E_ID)s * blockDim.x + threadIdx.x;
        uint2 e0 = make_uint2(0, 0), e1 = e0, e2 = e0, e3 = e0;
        bool p0 = k0 < e, p1 = k0 + blockDim.x < e,
             p2 = k0 + 2 * blockDim.x < e, p3 = k0 + 3 * blockDim.x < e;
        if (p0) e0 = push_edge[k0];
        if (p1) e1 = push_edge[k0 + blockDim.x];
        if (p2) e2 = push_edge[k0 + 2 * blockDim.x];
        if (p3) e3 = push_edge[k0 + 3 * blockDim.x];
#define LUX_PDW_EDGE(P_, E_)                                                \
        if (P_) {                                                           \
          uint32_t cand = sat_add_label(src_lab, (E_).y);                   \
          uint32_t* slot = &new_labels[(E_).x - my_row_left];               \
          uint32_t cur = __hip_atomic_load(slot, __ATOMIC_RELAXED,          \
                                           __HIP_MEMORY_SCOPE_AGENT);       \
          if (cand < cur) atomicMin(slot, cand);                            \
        }
        LUX_PDW_EDGE(p0, e0)
        LUX_PDW_EDGE(p1, e1)
        LUX_PDW_EDGE(p2, e2)
        LUX_PDW_EDGE(p3, e3)
      }
      for (; s < nstripes; s++) {
        E_ID k = b + (E_ID)s * blockDim.x + threadIdx.x;
        if (k < e) {
          uint2 ed = push_edge[k];
          LUX_PDW_EDGE(true, ed)
        }
      }
#undef LUX_PDW_EDGE
      continue;
    }
    for (uint32_t s = 0; s < nstripes; s++) {
      E_ID k = b + (E_ID)s * blockDim.x + threadIdx.x;
      uint32_t flag = 0;
      V_ID dstv = 0;
      if (k < e) {
        uint2 ed = push_edge[k];
        V_ID lv = ed.x - my_row_left;
        uint32_t cand = sat_add_label(src_lab, ed.y);
        uint32_t* slot = &new_labels[lv];
        uint32_t cur = __hip_atomic_load(slot, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        if (cand < cur) {
          // first-improvement enqueue: labels only fall below the
          // snapshot, so exactly one atomicMin per improved vertex and
          // iteration returns the snapshot value
          uint32_t last = snapshot[lv];
          uint32_t act = atomicMin(slot, cand);
          if (act == last) {
            flag = 1;
            dstv = ed.x;
          }
        }
      }
      __syncthreads();
      uint32_t q_total;
      uint32_t q_off = block_exscan<uint32_t, BLOCK>(flag, lds_scan,
                                                     &q_total);
      if (threadIdx.x == 0 && q_total)
        queue_base = atomicAdd(num_nodes, q_total);
      __syncthreads();
      if (flag) {
        uint32_t pos = queue_base + q_off;
        if (pos < capacity) new_queue[pos] = dstv;
      }
      __syncthreads();
    }
  }
}

// Weighted check oracle over my pull-CSC partition: edges with
// label[v] > sat(label[u] + w) for a finite label[u], plus one if the
// source (counted by the rank that owns it) is not at distance 0.
__global__ void check_w_kernel(V_ID vp, V_ID row_left,
                               const E_ID* row_ptr_loc, const V_ID* col,
                               const WeightType* weight,
                               const uint32_t* labels, V_ID source,
                               unsigned long long* mistakes) {
  __shared__ unsigned long long lds[BLOCK / WAVE];
  unsigned long long cnt = 0;
  for (V_ID v = blockIdx.x * blockDim.x + threadIdx.x; v < vp;
       v += blockDim.x * gridDim.x) {
    uint32_t lab = labels[row_left + v];
    if (row_left + v == source && lab != 0) cnt++;
    for (E_ID j = row_ptr_loc[v]; j < row_ptr_loc[v + 1]; j++) {
      uint32_t sl = labels[col[j]];
      if (sl != INF_LABEL && lab > sat_add_label(sl, (uint32_t)weight[j]))
        cnt++;
    }
  }
  cnt = block_reduce_sum(cnt, lds);
  if (threadIdx.x == 0 && cnt) atomicAdd(mistakes, cnt);
}

// ---------------- bucketed schedule (near-far delta-stepping) ----------
// The one O(vp) pass of a bucketed iteration: it classifies every local
// vertex against the device-resident `limit` and replaces build_bitmap, the
// snapshot stream copy and any queue the scatter would have appended.
//
//   changed = snapshot[v] != label[v]
//   d       = changed | (replace ? 0 : dirty bit)   (pull: dirty = changed)
//   active  = d && label[v] <= *limit               -> seg's dense bitmap
//   dirty   = d && !active                          (the deferred set)
//   snapshot[v] = label[v]                          (standing invariant)
//
// One lane per vertex; a wave owns vertices [64w, 64w + 64) and forms its
// two words with __ballot: one u64 of dirty and one u64 of the bitmap (at
// seg + 8, 8-byte aligned), each stored by lane 0 — so dirty holds
// 2 * ceil(vp / 64) u32 words and the bitmap ceil(vp / 64) u64 words, and
// bits at and beyond vp are written 0. Counts and the minimum deferred
// label accumulate per lane over the grid-stride loop, then one block
// ladder and one atomic per block: active -> header numNodes, deferred ->
// meta[7], min deferred label -> meta[6] (the caller presets numNodes = 0,
// meta[6] = INF_LABEL, meta[7] = 0). With snapshot == labels everywhere the
// pass is the bucket advance's reselect.
__global__ void bucket_select_kernel(V_ID vp, uint32_t* snapshot,
                                     const uint32_t* labels_part,
                                     uint32_t* dirty, const uint32_t* limit_p,
                                     int replace, uint8_t* seg,
                                     uint32_t* meta) {
  __shared__ uint32_t lds_a[BLOCK / WAVE];
  __shared__ uint32_t lds_d[BLOCK / WAVE];
  __shared__ uint32_t lds_m[BLOCK / WAVE];
  const uint32_t limit = *limit_p;
  unsigned long long* dirty64 = (unsigned long long*)dirty;
  unsigned long long* bitmap64 =
      (unsigned long long*)(seg + sizeof(FrontierHeader));
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  uint32_t n_active = 0, n_defer = 0, min_defer = INF_LABEL;
  const uint64_t stride = (uint64_t)blockDim.x * gridDim.x;
  // block-uniform loop bound: every lane of a wave reaches the ballots
  for (uint64_t blk = (uint64_t)blockIdx.x * blockDim.x; blk < vp;
       blk += stride) {
    uint64_t v = blk + threadIdx.x;
    uint64_t wbase = blk + (uint64_t)wid * WAVE;  // wave-uniform
    if (wbase >= vp) continue;  // whole wave past the end: no word to own
    uint64_t word = wbase >> 6;
    bool in = v < vp;
    uint32_t snap = 0, lab = 0;
    if (in) {
      snap = snapshot[v];
      lab = labels_part[v];
    }
    bool d = in && snap != lab;
    if (d) snapshot[v] = lab;
    if (!replace) {
      unsigned long long old = dirty64[word];
      d = d || (in && ((old >> lane) & 1ull));
    }
    bool act = d && lab <= limit;
    bool def = d && !act;
    unsigned long long act_word = __ballot(act);
    unsigned long long def_word = __ballot(def);
    if (lane == 0) {
      bitmap64[word] = act_word;
      dirty64[word] = def_word;
    }
    n_active += act;
    if (def) {
      n_defer++;
      min_defer = lab < min_defer ? lab : min_defer;
    }
  }
  // block ladder (gpu_common.h shape): wave reduce, one LDS slot per wave,
  // wave 0 finishes, thread 0 issues the block's atomics
  n_active = wave_reduce_sum(n_active);
  n_defer = wave_reduce_sum(n_defer);
  min_defer = wave_reduce_min(min_defer);
  if (lane == 0) {
    lds_a[wid] = n_active;
    lds_d[wid] = n_defer;
    lds_m[wid] = min_defer;
  }
  __syncthreads();
  if (wid == 0) {
    bool has = lane < (int)(blockDim.x / WAVE);
    n_active = wave_reduce_sum(has ? lds_a[lane] : 0u);
    n_defer = wave_reduce_sum(has ? lds_d[lane] : 0u);
    min_defer = wave_reduce_min(has ? lds_m[lane] : INF_LABEL);
    if (lane == 0) {
      if (n_active) atomicAdd(&((FrontierHeader*)seg)->numNodes, n_active);
      if (n_defer) {
        atomicAdd(&meta[7], n_defer);
        atomicMin(&meta[6], min_defer);
      }
    }
  }
}

}  // namespace lux

// ---------------- C ABI ----------------

using namespace lux;

extern "C" {

void lux_gpu_csr_scatter(uint64_t stream, uint64_t ep, const V_ID* col,
                         const E_ID* row_ptr_loc, V_ID vp, V_ID row_left,
                         unsigned long long* cursor, V_ID* push_col) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(csr_scatter_kernel, dim3(grid_for(ep)), dim3(BLOCK), 0,
                     s, ep, col, row_ptr_loc, vp, row_left, cursor, push_col);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_frontier_expand(uint64_t stream, int old_dense,
                             V_ID in_row_left, V_ID in_count,
                             const uint8_t* old_seg,
                             const uint32_t* qlabels /*nullable*/,
                             uint32_t* labels_repair /*nullable*/,
                             const E_ID* push_row_ptr, uint2* items,
                             uint32_t* counter /*pre-zeroed u32[4]*/,
                             uint32_t max_items) {
  hipStream_t s = (hipStream_t)stream;
  if (in_count == 0) return;
  hipLaunchKernelGGL(frontier_expand_kernel, dim3(grid_for(in_count)),
                     dim3(BLOCK), 0, s, old_dense, in_row_left, in_count,
                     old_seg, qlabels, labels_repair, push_row_ptr, items,
                     counter, max_items);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_frontier_expand_auto(uint64_t stream, V_ID verts,
                                  V_ID in_row_left, const uint8_t* seg,
                                  const uint32_t* qlabels,
                                  uint32_t* labels_repair,
                                  const E_ID* push_row_ptr, uint2* items,
                                  uint32_t* counter, uint32_t max_items) {
  hipStream_t s = (hipStream_t)stream;
  if (verts == 0) return;
  hipLaunchKernelGGL(frontier_expand_auto_kernel, dim3(grid_for(verts)),
                     dim3(BLOCK), 0, s, verts, in_row_left, seg, qlabels,
                     labels_repair, push_row_ptr, items, counter, max_items);
  LUX_POST_LAUNCH(stream);
}

// Device-predicated frontier fix-up chain + meta record (see kernel
// comments above): decide -> (rebuild bitmap | convert d2s) -> copy back
// -> label annex -> meta. Replaces r1's host-read-driven conversion logic
// (push_engine.py r1 step: 3 blocking D2H reads per iteration -> 0; the
// engine reads only the exchanged meta once).
void lux_gpu_frontier_fixup(uint64_t stream, V_ID vp, V_ID row_left,
                            V_ID capacity, int built_dense,
                            const uint32_t* snapshot,
                            const uint32_t* labels_part,
                            const uint32_t* deg_part, uint8_t* new_seg,
                            uint32_t* annex, uint8_t* tmp_seg,
                            uint32_t* meta,
                            const uint32_t* item_counter /*nullable*/,
                            uint32_t max_items) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fixup_decide_kernel, dim3(1), dim3(1), 0, s,
                     built_dense, capacity, new_seg, tmp_seg, meta);
  if (vp > 0) {
    // sparse-overflow rebuild (flag 2)
    hipLaunchKernelGGL(build_bitmap_kernel, dim3(grid_for((vp + 7) / 8)),
                       dim3(BLOCK), 0, s, vp, snapshot, labels_part, tmp_seg,
                       meta + 5, 2u);
    // dense-fits-sparse conversion (flag 1)
    hipLaunchKernelGGL(d2s_kernel, dim3(grid_for(vp)), dim3(BLOCK), 0, s, vp,
                       row_left, new_seg, tmp_seg, meta + 5, 1u);
    hipLaunchKernelGGL(seg_copy_kernel,
                       dim3(grid_for((uint64_t)capacity + vp / 32 + 4)),
                       dim3(BLOCK), 0, s, vp, tmp_seg, new_seg, meta);
    hipLaunchKernelGGL(annex_fill_kernel, dim3(grid_for(capacity)),
                       dim3(BLOCK), 0, s, row_left, new_seg, labels_part,
                       annex);
  }
  hipLaunchKernelGGL(seg_meta_kernel, dim3(vp ? grid_for(vp) : 1),
                     dim3(BLOCK), 0, s, vp, row_left, new_seg, deg_part,
                     item_counter, max_items, meta);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_push_chunk_scatter(uint64_t stream, int is_min, int new_dense,
                                const uint2* items, const uint32_t* counter,
                                uint32_t max_items,
                                const E_ID* push_row_ptr,
                                const V_ID* push_col,
                                const uint32_t* old_labels,
                                const uint32_t* snapshot,
                                uint32_t* new_labels, V_ID my_row_left,
                                uint8_t* new_seg, V_ID capacity,
                                uint32_t* visited_bits /*nullable; IS_MIN
                                level-synchronous BFS fast path*/) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(MAX_GRID), blk(BLOCK);
  // grid-strided over the device-side item count: no host sync needed;
  // surplus blocks read the counter and exit
#define LUX_PCS(MIN_, DENSE_, BITS_)                                       \
  hipLaunchKernelGGL((push_chunk_scatter_kernel<MIN_, DENSE_, BITS_>),     \
                     grid, blk, 0, s, items, counter, max_items,           \
                     push_row_ptr, push_col, old_labels, snapshot,         \
                     new_labels, my_row_left, new_seg, capacity,           \
                     visited_bits)
  if (is_min && visited_bits) {
    if (new_dense) LUX_PCS(true, true, true);
    else LUX_PCS(true, false, true);
  } else if (is_min) {
    if (new_dense) LUX_PCS(true, true, false);
    else LUX_PCS(true, false, false);
  } else {
    if (new_dense) LUX_PCS(false, true, false);
    else LUX_PCS(false, false, false);
  }
#undef LUX_PCS
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_bits_from_labels(uint64_t stream, V_ID vp,
                              const uint32_t* labels, uint32_t* bits) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bits_from_labels_kernel,
                     dim3(grid_for((uint64_t)(vp + 31) / 32)), dim3(BLOCK),
                     0, s, vp, labels, bits);
  LUX_POST_LAUNCH(stream);
}


void lux_gpu_build_bitmap(uint64_t stream, V_ID vp, const uint32_t* snapshot,
                          const uint32_t* new_labels, uint8_t* seg) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(build_bitmap_kernel, dim3(grid_for((vp + 7) / 8)),
                     dim3(BLOCK), 0, s, vp, snapshot, new_labels, seg,
                     (const uint32_t*)nullptr, 0u);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_d2s(uint64_t stream, V_ID vp, V_ID row_left,
                 const uint8_t* dense_seg, uint8_t* sparse_seg) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(d2s_kernel, dim3(grid_for(vp)), dim3(BLOCK), 0, s, vp,
                     row_left, dense_seg, sparse_seg,
                     (const uint32_t*)nullptr, 0u);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_publish_labels_guarded(uint64_t stream, V_ID vp,
                                    const uint32_t* meta,
                                    const uint32_t* labels_part,
                                    uint32_t* labels_slice) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(publish_labels_guarded_kernel, dim3(grid_for(vp)),
                     dim3(BLOCK), 0, s, vp, meta, labels_part, labels_slice);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_check(uint64_t stream, int is_min, V_ID vp, V_ID row_left,
                   const E_ID* row_ptr_loc, const V_ID* col,
                   const uint32_t* labels, unsigned long long* mistakes) {
  hipStream_t s = (hipStream_t)stream;
  if (is_min)
    hipLaunchKernelGGL(check_kernel<true>, dim3(grid_for(vp)), dim3(BLOCK), 0,
                       s, vp, row_left, row_ptr_loc, col, labels, mistakes);
  else
    hipLaunchKernelGGL(check_kernel<false>, dim3(grid_for(vp)), dim3(BLOCK),
                       0, s, vp, row_left, row_ptr_loc, col, labels,
                       mistakes);
  LUX_POST_LAUNCH(stream);
}

// ---- weighted SSSP (min-plus) ----

// push_edge: uint2[ep] {global dst, weight}; cursor as lux_gpu_csr_scatter
void lux_gpu_csr_scatter_w(uint64_t stream, uint64_t ep, const V_ID* col,
                           const WeightType* weight, const E_ID* row_ptr_loc,
                           V_ID vp, V_ID row_left,
                           unsigned long long* cursor, uint2* push_edge) {
  hipStream_t s = (hipStream_t)stream;
  if (ep == 0 || vp == 0) return;
  hipLaunchKernelGGL(csr_scatter_w_kernel, dim3(grid_for(ep)), dim3(BLOCK), 0,
                     s, ep, col, weight, row_ptr_loc, vp, row_left, cursor,
                     push_edge);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_push_chunk_scatter_w(uint64_t stream, int new_dense,
                                  const uint2* items, const uint32_t* counter,
                                  uint32_t max_items,
                                  const E_ID* push_row_ptr,
                                  const uint2* push_edge,
                                  const uint32_t* old_labels,
                                  const uint32_t* snapshot,
                                  uint32_t* new_labels, V_ID my_row_left,
                                  uint8_t* new_seg, V_ID capacity) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(MAX_GRID), blk(BLOCK);
  if (new_dense)
    hipLaunchKernelGGL(push_chunk_scatter_w_kernel<true>, grid, blk, 0, s,
                       items, counter, max_items, push_row_ptr, push_edge,
                       old_labels, snapshot, new_labels, my_row_left, new_seg,
                       capacity);
  else
    hipLaunchKernelGGL(push_chunk_scatter_w_kernel<false>, grid, blk, 0, s,
                       items, counter, max_items, push_row_ptr, push_edge,
                       old_labels, snapshot, new_labels, my_row_left, new_seg,
                       capacity);
  LUX_POST_LAUNCH(stream);
}

void lux_gpu_check_w(uint64_t stream, V_ID vp, V_ID row_left,
                     const E_ID* row_ptr_loc, const V_ID* col,
                     const WeightType* weight, const uint32_t* labels,
                     V_ID source, unsigned long long* mistakes) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(check_w_kernel, dim3(grid_for(vp)), dim3(BLOCK), 0, s,
                     vp, row_left, row_ptr_loc, col, weight, labels, source,
                     mistakes);
  LUX_POST_LAUNCH(stream);
}

// ---- bucketed schedule ----

// dirty: u32[2 * ceil(vp / 64)] in/out; seg: header + ceil(vp / 64) u64
// bitmap words, numNodes preset to 0; meta[6] preset to INF_LABEL, meta[7]
// to 0; limit: one device-resident u32 (captured graphs replay across
// buckets). lux_gpu_frontier_fixup(built_dense = 1) finishes the segment.
void lux_gpu_bucket_select(uint64_t stream, V_ID vp, uint32_t* snapshot,
                           const uint32_t* labels_part, uint32_t* dirty,
                           const uint32_t* limit, int replace, uint8_t* seg,
                           uint32_t* meta) {
  hipStream_t s = (hipStream_t)stream;
  if (vp == 0) return;
  hipLaunchKernelGGL(bucket_select_kernel, dim3(grid_for(vp)), dim3(BLOCK), 0,
                     s, vp, snapshot, labels_part, dirty, limit, replace, seg,
                     meta);
  LUX_POST_LAUNCH(stream);
}

}  // extern "C"
