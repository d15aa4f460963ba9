// CPU reference engines for the four vertex programs.
//
// These are the golden-semantics implementations the GPU kernels are tested
// against, and the per-partition *_iter_part entry points are
// the compute step of the CPU multi-process path (gloo, world_size>1) that
// exercises the distributed exchange layer without a GPU.
//
// Semantics parity (reference file:line):
//  - PageRank: new_pr = (1-ALPHA)/nv + ALPHA * sum_{u in in(v)} old_pr[u],
//    stored divided by out-degree (pagerank_gpu.cu:97-100); initial value
//    rank/degree with rank = 1/nv, degree-0 stores rank (pagerank_gpu.cu:255-259).
//  - SSSP: unweighted hop relaxation label[dst] = min(label[dst],
//    label[src]+1) (sssp_gpu.cu:122,208,225); source = 0, rest INF.
//  - CC: label[dst] = max(label[dst], label[src]) along directed edges
//    (components_gpu.cu:122); init label[v] = v.
//  - CF: one SGD sweep per iteration over in-edges of each dst using OLD
//    vectors throughout: err = w - <src_vec, dst_vec>; acc += err*src_vec;
//    new = old + GAMMA*(acc - LAMBDA*old) (colfilter_gpu.cu:83-101). The
//    reference indexes the dst vector with a partition-local offset into a
//    full-length array (colfilter_gpu.cu:65 — a rowLeft>0 bug); we use the
//    intended old[dst].
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "lux/graph.h"
#include "lux/rmat.h"

namespace lux {

// ---------- PageRank (pull) ----------

void pagerank_init(V_ID nv, const V_ID* out_deg, float* pr) {
  float rank = 1.0f / nv;
  for (V_ID v = 0; v < nv; v++)
    pr[v] = out_deg[v] == 0 ? rank : rank / out_deg[v];
}

// One iteration over partition rows [row_left, row_right]; col_end/src are
// the partition slice (col_end global offsets, src indexed from col_left).
void pagerank_iter_part(V_ID nv, V_ID row_left, V_ID row_right,
                        E_ID col_left, const E_ID* col_end, const V_ID* src,
                        const V_ID* out_deg, const float* old_pr,
                        float* new_pr_part) {
  float init_rank = (1.0f - PR_ALPHA) / nv;
  for (V_ID v = row_left; v <= row_right; v++) {
    E_ID b = (v == row_left) ? col_left : col_end[v - 1 - row_left];
    E_ID e = col_end[v - row_left];
    float sum = 0.0f;
    for (E_ID i = b; i < e; i++) sum += old_pr[src[i - col_left]];
    float pr = init_rank + PR_ALPHA * sum;
    new_pr_part[v - row_left] = out_deg[v] == 0 ? pr : pr / out_deg[v];
  }
}

void out_degrees(V_ID nv, E_ID ne, const V_ID* src, V_ID* deg) {
  std::memset(deg, 0, sizeof(V_ID) * nv);
  for (E_ID e = 0; e < ne; e++) deg[src[e]]++;
}

// Whole-graph driver (tests/config-1 plumbing path).
void pagerank_cpu(const HostCSC& g, int iters, float* pr_out) {
  std::vector<V_ID> deg(g.nv);
  out_degrees(g.nv, g.ne, g.src.data(), deg.data());
  std::vector<float> oldp(g.nv), newp(g.nv);
  pagerank_init(g.nv, deg.data(), oldp.data());
  for (int it = 0; it < iters; it++) {
    pagerank_iter_part(g.nv, 0, g.nv - 1, 0, g.col_end.data(), g.src.data(),
                       deg.data(), oldp.data(), newp.data());
    std::swap(oldp, newp);
  }
  std::memcpy(pr_out, oldp.data(), sizeof(float) * g.nv);
}

// ---------- Label propagation core (SSSP min / CC max) ----------

// Dense pull relaxation of one partition: for every dst row, fold in-edge
// source labels. Returns number of labels that changed.
template <bool IS_MIN>
static V_ID label_iter_part(V_ID row_left, V_ID row_right, E_ID col_left,
                            const E_ID* col_end, const V_ID* src,
                            const V_ID* old_label, V_ID* new_label_part) {
  V_ID changed = 0;
  for (V_ID v = row_left; v <= row_right; v++) {
    E_ID b = (v == row_left) ? col_left : col_end[v - 1 - row_left];
    E_ID e = col_end[v - row_left];
    V_ID lab = old_label[v];
    for (E_ID i = b; i < e; i++) {
      V_ID sl = old_label[src[i - col_left]];
      if (IS_MIN) {
        V_ID cand = sl == INF_LABEL ? INF_LABEL : sl + 1;
        lab = std::min(lab, cand);
      } else {
        lab = std::max(lab, sl);
      }
    }
    if (lab != old_label[v]) changed++;
    new_label_part[v - row_left] = lab;
  }
  return changed;
}

V_ID sssp_iter_part(V_ID row_left, V_ID row_right, E_ID col_left,
                    const E_ID* col_end, const V_ID* src,
                    const V_ID* old_label, V_ID* new_label_part) {
  return label_iter_part<true>(row_left, row_right, col_left, col_end, src,
                               old_label, new_label_part);
}
V_ID cc_iter_part(V_ID row_left, V_ID row_right, E_ID col_left,
                  const E_ID* col_end, const V_ID* src, const V_ID* old_label,
                  V_ID* new_label_part) {
  return label_iter_part<false>(row_left, row_right, col_left, col_end, src,
                                old_label, new_label_part);
}

// Fixed-point drivers (converged results == what the push engine converges
// to; iteration count bounded by nv).
int sssp_cpu(const HostCSC& g, V_ID source, V_ID* label_out) {
  std::vector<V_ID> oldl(g.nv, INF_LABEL), newl(g.nv);
  oldl[source] = 0;
  int iters = 0;
  while (true) {
    V_ID changed = sssp_iter_part(0, g.nv - 1, 0, g.col_end.data(),
                                  g.src.data(), oldl.data(), newl.data());
    iters++;
    std::swap(oldl, newl);
    if (changed == 0) break;
  }
  std::memcpy(label_out, oldl.data(), sizeof(V_ID) * g.nv);
  return iters;
}

int cc_cpu(const HostCSC& g, V_ID* label_out) {
  std::vector<V_ID> oldl(g.nv), newl(g.nv);
  for (V_ID v = 0; v < g.nv; v++) oldl[v] = v;
  int iters = 0;
  while (true) {
    V_ID changed = cc_iter_part(0, g.nv - 1, 0, g.col_end.data(),
                                g.src.data(), oldl.data(), newl.data());
    iters++;
    std::swap(oldl, newl);
    if (changed == 0) break;
  }
  std::memcpy(label_out, oldl.data(), sizeof(V_ID) * g.nv);
  return iters;
}

// Check oracles, per the reference's CheckTask kernels
// (sssp_gpu.cu:773-798, components_gpu.cu:767-791): count violating edges.
E_ID sssp_check(const HostCSC& g, const V_ID* label) {
  E_ID mistakes = 0;
  for (V_ID v = 0; v < g.nv; v++) {
    for (E_ID i = g.row_begin(v); i < g.row_end(v); i++) {
      V_ID sl = label[g.src[i]];
      V_ID cand = sl == INF_LABEL ? INF_LABEL : sl + 1;
      if (label[v] > cand) mistakes++;
    }
  }
  return mistakes;
}
E_ID cc_check(const HostCSC& g, const V_ID* label) {
  E_ID mistakes = 0;
  for (V_ID v = 0; v < g.nv; v++)
    for (E_ID i = g.row_begin(v); i < g.row_end(v); i++)
      if (label[v] < label[g.src[i]]) mistakes++;
  return mistakes;
}

// ---------- Weighted SSSP (min-plus) ----------
// Weights are the graph's i32 weights read as non-negative integers.
// Relaxation saturates: cand = min(u64(label[u]) + w, 0xFFFFFFFE), so a
// finite distance never turns into INF_LABEL or wraps.

static inline V_ID sat_add_label(V_ID lab, WeightType w) {
  uint64_t c = (uint64_t)lab + (uint64_t)(uint32_t)w;
  return c > 0xFFFFFFFEull ? 0xFFFFFFFEu : (V_ID)c;
}

// weight[i] = edge_hash_weight(seed, src[i], dst of edge i, wmax)
void hash_weights(V_ID nv, const E_ID* col_end, const V_ID* src,
                  uint64_t seed, uint32_t wmax, WeightType* weight) {
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    E_ID e = col_end[v];
    for (E_ID i = b; i < e; i++)
      weight[i] = edge_hash_weight(seed, src[i], v, wmax);
    b = e;
  }
}

// Exact binary-heap Dijkstra (the CSC is turned into out-edge lists
// first). Returns -1 on a negative weight.
int sssp_weighted_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
                      const WeightType* weight, V_ID source,
                      V_ID* label_out) {
  for (E_ID i = 0; i < ne; i++)
    if (weight[i] < 0) return -1;
  std::vector<E_ID> out_ptr((size_t)nv + 1, 0);
  for (E_ID i = 0; i < ne; i++) out_ptr[src[i] + 1]++;
  for (V_ID v = 0; v < nv; v++) out_ptr[v + 1] += out_ptr[v];
  std::vector<V_ID> out_dst(ne);
  std::vector<WeightType> out_w(ne);
  {
    std::vector<E_ID> cur(out_ptr.begin(), out_ptr.end() - 1);
    E_ID b = 0;
    for (V_ID v = 0; v < nv; v++) {
      E_ID e = col_end[v];
      for (E_ID i = b; i < e; i++) {
        E_ID pos = cur[src[i]]++;
        out_dst[pos] = v;
        out_w[pos] = weight[i];
      }
      b = e;
    }
  }
  for (V_ID v = 0; v < nv; v++) label_out[v] = INF_LABEL;
  label_out[source] = 0;
  using Ent = std::pair<V_ID, V_ID>;  // (distance, vertex)
  std::priority_queue<Ent, std::vector<Ent>, std::greater<Ent>> heap;
  heap.push({0, source});
  while (!heap.empty()) {
    Ent top = heap.top();
    heap.pop();
    V_ID u = top.second;
    if (top.first != label_out[u]) continue;  // stale entry
    for (E_ID i = out_ptr[u]; i < out_ptr[u + 1]; i++) {
      V_ID cand = sat_add_label(top.first, out_w[i]);
      if (cand < label_out[out_dst[i]]) {
        label_out[out_dst[i]] = cand;
        heap.push({cand, out_dst[i]});
      }
    }
  }
  return 0;
}

// Edges with label[v] > sat(label[u] + w) where label[u] is finite, plus
// one if label[source] != 0 (the device check's invariant).
E_ID sssp_weighted_check(V_ID nv, const E_ID* col_end, const V_ID* src,
                         const WeightType* weight, const V_ID* label,
                         V_ID source) {
  E_ID mistakes = label[source] != 0 ? 1 : 0;
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    E_ID e = col_end[v];
    for (E_ID i = b; i < e; i++) {
      V_ID sl = label[src[i]];
      if (sl != INF_LABEL && label[v] > sat_add_label(sl, weight[i]))
        mistakes++;
    }
    b = e;
  }
  return mistakes;
}

// ---------- Betweenness centrality (single source, Brandes) ----------
// fp64 oracle of BCEngine (no reference equivalent). BFS over the out-edges
// in queue order; sigma grows along every edge into the next level (each
// occurrence of a parallel edge is a path, a self-loop never leads one level
// down); delta folds back in reverse queue order. Unreached vertices keep
// depth INF, sigma 0, delta 0; delta[source] is reported as 0.
void bc_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
            V_ID source, V_ID* depth, double* sigma, double* delta) {
  std::vector<E_ID> out_ptr((size_t)nv + 1, 0);
  for (E_ID i = 0; i < ne; i++) out_ptr[src[i] + 1]++;
  for (V_ID v = 0; v < nv; v++) out_ptr[v + 1] += out_ptr[v];
  std::vector<V_ID> out_dst(ne);
  {
    std::vector<E_ID> cur(out_ptr.begin(), out_ptr.end() - 1);
    E_ID b = 0;
    for (V_ID v = 0; v < nv; v++) {
      for (E_ID i = b; i < col_end[v]; i++) out_dst[cur[src[i]]++] = v;
      b = col_end[v];
    }
  }
  for (V_ID v = 0; v < nv; v++) {
    depth[v] = INF_LABEL;
    sigma[v] = 0.0;
    delta[v] = 0.0;
  }
  std::vector<V_ID> order;
  order.reserve(nv);
  depth[source] = 0;
  sigma[source] = 1.0;
  order.push_back(source);
  for (size_t head = 0; head < order.size(); head++) {
    V_ID u = order[head];
    for (E_ID i = out_ptr[u]; i < out_ptr[u + 1]; i++) {
      V_ID v = out_dst[i];
      if (depth[v] == INF_LABEL) {
        depth[v] = depth[u] + 1;
        order.push_back(v);
      }
      if (depth[v] == depth[u] + 1) sigma[v] += sigma[u];
    }
  }
  for (size_t k = order.size(); k-- > 0;) {
    V_ID u = order[k];
    double acc = 0.0;
    for (E_ID i = out_ptr[u]; i < out_ptr[u + 1]; i++) {
      V_ID v = out_dst[i];
      if (depth[v] == depth[u] + 1)
        acc += sigma[u] / sigma[v] * (1.0 + delta[v]);
    }
    delta[u] = acc;
  }
  delta[source] = 0.0;
}

// ---------- Triangle counting ----------
// Exact oracle of TCEngine (no reference equivalent), on the underlying
// simple undirected graph: {u,v} is an edge iff u != v and u->v or v->u
// occurs, so parallel edges collapse and self-loops vanish. Node-iterator
// counting on the sorted, deduplicated, id-oriented (lo -> hi) adjacency:
// for every arc u -> v, a merge of A(u) and A(v); each common w is the
// triangle u < v < w, counted once in *total and once for each corner.
void tc_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
            uint64_t* total, uint64_t* per_vertex) {
  std::vector<uint64_t> keys;
  keys.reserve(ne);
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    for (E_ID i = b; i < col_end[v]; i++) {
      V_ID s = src[i];
      if (s == v) continue;
      V_ID lo = std::min(s, v), hi = std::max(s, v);
      keys.push_back(((uint64_t)lo << 32) | hi);
    }
    b = col_end[v];
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  std::vector<E_ID> ptr((size_t)nv + 1, 0);
  std::vector<V_ID> adj(keys.size());
  for (size_t k = 0; k < keys.size(); k++) {
    ptr[(keys[k] >> 32) + 1]++;
    adj[k] = (V_ID)(keys[k] & 0xFFFFFFFFu);
  }
  for (V_ID v = 0; v < nv; v++) ptr[v + 1] += ptr[v];
  *total = 0;
  for (V_ID v = 0; v < nv; v++) per_vertex[v] = 0;
  for (V_ID u = 0; u < nv; u++) {
    for (E_ID k = ptr[u]; k < ptr[u + 1]; k++) {
      V_ID v = adj[k];
      E_ID i = k + 1, ie = ptr[u + 1];  // A(u) past v: every w is > v
      E_ID j = ptr[v], je = ptr[v + 1];
      while (i < ie && j < je) {
        if (adj[i] < adj[j]) i++;
        else if (adj[j] < adj[i]) j++;
        else {
          (*total)++;
          per_vertex[u]++;
          per_vertex[v]++;
          per_vertex[adj[i]]++;
          i++;
          j++;
        }
      }
    }
  }
}

// ---------- k-truss ----------
// Exact k-truss oracle (no reference equivalent), on the same simple
// undirected graph as tc_cpu. Edges are numbered in key order
// ((lo << 32) | hi, ascending). support[e] = triangles containing e;
// trussness[e] = the largest k whose k-truss (every edge in >= k - 2
// triangles inside it) contains e, 2 for an edge in no triangle.
// Sequential bucket-queue peeling on the full (both directions) adjacency:
// take an edge of minimum current support s, give it trussness s + 2, and
// take one off the other two edges of each triangle it still closes. No
// rounds, no recount, no orientation: nothing in common with a synchronous
// recompute-per-round peel.
// edges u32[2 * ne], support u32[ne] and trussness u32[ne] (may be null)
// are sized for the worst case; the return value m is the number filled.
E_ID truss_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
               V_ID* edges, uint32_t* support, uint32_t* trussness) {
  std::vector<uint64_t> keys;
  keys.reserve(ne);
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    for (E_ID i = b; i < col_end[v]; i++) {
      V_ID s = src[i];
      if (s == v) continue;
      V_ID lo = std::min(s, v), hi = std::max(s, v);
      keys.push_back(((uint64_t)lo << 32) | hi);
    }
    b = col_end[v];
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const E_ID m = keys.size();
  // full adjacency with edge ids; scanning the keys in order appends to
  // every vertex its lower neighbours (ascending) before its higher ones
  std::vector<E_ID> ptr((size_t)nv + 1, 0);
  for (E_ID e = 0; e < m; e++) {
    ptr[(keys[e] >> 32) + 1]++;
    ptr[(keys[e] & 0xFFFFFFFFu) + 1]++;
  }
  for (V_ID v = 0; v < nv; v++) ptr[v + 1] += ptr[v];
  std::vector<V_ID> nbr(2 * m);
  std::vector<E_ID> eid(2 * m);
  {
    std::vector<E_ID> fill(ptr.begin(), ptr.end() - 1);
    for (E_ID e = 0; e < m; e++) {
      V_ID lo = (V_ID)(keys[e] >> 32), hi = (V_ID)(keys[e] & 0xFFFFFFFFu);
      edges[2 * e] = lo;
      edges[2 * e + 1] = hi;
      nbr[fill[lo]] = hi;
      eid[fill[lo]++] = e;
      nbr[fill[hi]] = lo;
      eid[fill[hi]++] = e;
    }
  }
  // calls f(e1, e2) with the edges (lo, w), (hi, w) of every common
  // neighbour w of edge e's endpoints
  auto triangles_of = [&](E_ID e, auto&& f) {
    V_ID lo = edges[2 * e], hi = edges[2 * e + 1];
    E_ID i = ptr[lo], ie = ptr[lo + 1], j = ptr[hi], je = ptr[hi + 1];
    while (i < ie && j < je) {
      if (nbr[i] < nbr[j]) i++;
      else if (nbr[j] < nbr[i]) j++;
      else {
        f(eid[i], eid[j]);
        i++;
        j++;
      }
    }
  };
  uint32_t smax = 0;
  for (E_ID e = 0; e < m; e++) {
    uint32_t s = 0;
    triangles_of(e, [&](E_ID, E_ID) { s++; });
    support[e] = s;
    smax = std::max(smax, s);
  }
  if (!trussness || !m) return m;
  // bucket queue: order holds the edges ascending by current support,
  // bin[s] is where the edges of support s start, pos the inverse of order
  std::vector<uint32_t> cur(support, support + m);
  std::vector<E_ID> bin((size_t)smax + 2, 0), order(m), pos(m);
  for (E_ID e = 0; e < m; e++) bin[cur[e] + 1]++;
  for (uint32_t s = 0; s <= smax; s++) bin[s + 1] += bin[s];
  {
    std::vector<E_ID> fill(bin.begin(), bin.end() - 1);
    for (E_ID e = 0; e < m; e++) {
      pos[e] = fill[cur[e]]++;
      order[pos[e]] = e;
    }
  }
  std::vector<char> gone(m, 0);
  for (E_ID k = 0; k < m; k++) {
    E_ID e = order[k];
    uint32_t s = cur[e];
    trussness[e] = s + 2;
    gone[e] = 1;
    triangles_of(e, [&](E_ID e1, E_ID e2) {
      if (gone[e1] || gone[e2]) return;
      for (E_ID f : {e1, e2}) {
        if (cur[f] <= s) continue;
        // swap f with the first edge of its bin, then shrink the bin
        E_ID pf = pos[f], pw = std::max(bin[cur[f]], k + 1);
        E_ID w = order[pw];
        if (w != f) {
          order[pf] = w;
          pos[w] = pf;
          order[pw] = f;
          pos[f] = pw;
        }
        bin[cur[f]] = pw + 1;
        cur[f]--;
      }
    });
  }
  return m;
}

// ---------- k-core ----------
// Exact coreness oracle of KCoreEngine (no reference equivalent), on the
// same simple undirected graph as tc_cpu. coreness[v] = the largest k whose
// k-core (the largest subgraph in which every vertex has degree >= k)
// contains v; 0 for a vertex with no simple edge. Sequential
// Batagelj-Zaversnik bucket peel, O(m): vert holds the vertices ascending
// by current degree, bin[d] is where degree d starts, pos the inverse of
// vert; take the next vertex, fix its coreness at its current degree and
// move every neighbour of larger degree one bin down. No rounds, no queue.
void coreness_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
                  uint32_t* coreness) {
  std::vector<uint64_t> keys;
  keys.reserve(ne);
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    for (E_ID i = b; i < col_end[v]; i++) {
      V_ID s = src[i];
      if (s == v) continue;
      V_ID lo = std::min(s, v), hi = std::max(s, v);
      keys.push_back(((uint64_t)lo << 32) | hi);
    }
    b = col_end[v];
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const E_ID m = keys.size();
  std::vector<E_ID> ptr((size_t)nv + 1, 0);
  for (E_ID e = 0; e < m; e++) {
    ptr[(keys[e] >> 32) + 1]++;
    ptr[(keys[e] & 0xFFFFFFFFu) + 1]++;
  }
  for (V_ID v = 0; v < nv; v++) ptr[v + 1] += ptr[v];
  std::vector<V_ID> nbr(2 * m);
  {
    std::vector<E_ID> fill(ptr.begin(), ptr.end() - 1);
    for (E_ID e = 0; e < m; e++) {
      V_ID lo = (V_ID)(keys[e] >> 32), hi = (V_ID)(keys[e] & 0xFFFFFFFFu);
      nbr[fill[lo]++] = hi;
      nbr[fill[hi]++] = lo;
    }
  }
  uint32_t dmax = 0;
  for (V_ID v = 0; v < nv; v++) {
    coreness[v] = (uint32_t)(ptr[v + 1] - ptr[v]);  // the current degree
    dmax = std::max(dmax, coreness[v]);
  }
  std::vector<V_ID> bin((size_t)dmax + 2, 0), vert(nv), pos(nv);
  for (V_ID v = 0; v < nv; v++) bin[coreness[v] + 1]++;
  for (uint32_t d = 0; d <= dmax; d++) bin[d + 1] += bin[d];
  {
    std::vector<V_ID> fill(bin.begin(), bin.end() - 1);
    for (V_ID v = 0; v < nv; v++) {
      pos[v] = fill[coreness[v]]++;
      vert[pos[v]] = v;
    }
  }
  for (V_ID k = 0; k < nv; k++) {
    V_ID v = vert[k];
    for (E_ID i = ptr[v]; i < ptr[v + 1]; i++) {
      V_ID u = nbr[i];
      if (coreness[u] <= coreness[v]) continue;
      // swap u with the first vertex of its bin, then shrink the bin
      V_ID pu = pos[u], pw = bin[coreness[u]];
      V_ID w = vert[pw];
      if (w != u) {
        vert[pu] = w;
        pos[w] = pu;
        vert[pw] = u;
        pos[u] = pw;
      }
      bin[coreness[u]]++;
      coreness[u]--;
    }
  }
}

// ---------- greedy colouring ----------
// Exact oracle of ColouringEngine (no reference equivalent), on the same
// simple undirected graph as tc_cpu. A strict total order "v precedes u":
// order 0 (degree) deg[v] > deg[u], or equal and v < u; order 1 (id) v < u;
// order 2 (hash) h(v) < h(u), or equal and v < u, h(v) =
// splitmix64(seed ^ v) >> 1. colour[v] = the smallest colour no preceding
// neighbour has. One sequential pass in priority order: when v's turn comes
// its coloured neighbours are exactly its predecessors; stamp[c] == v + 1
// marks the colours they hold. No rounds, no queue. Returns -1 on an unknown
// order.
int greedy_colouring_cpu(V_ID nv, E_ID ne, const E_ID* col_end,
                         const V_ID* src, int order, uint64_t seed,
                         int32_t* colour) {
  if (order < 0 || order > 2) return -1;
  std::vector<uint64_t> keys;
  keys.reserve(ne);
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    for (E_ID i = b; i < col_end[v]; i++) {
      V_ID s = src[i];
      if (s == v) continue;
      V_ID lo = std::min(s, v), hi = std::max(s, v);
      keys.push_back(((uint64_t)lo << 32) | hi);
    }
    b = col_end[v];
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const E_ID m = keys.size();
  std::vector<E_ID> ptr((size_t)nv + 1, 0);
  for (E_ID e = 0; e < m; e++) {
    ptr[(keys[e] >> 32) + 1]++;
    ptr[(keys[e] & 0xFFFFFFFFu) + 1]++;
  }
  for (V_ID v = 0; v < nv; v++) ptr[v + 1] += ptr[v];
  std::vector<V_ID> nbr(2 * m);
  {
    std::vector<E_ID> fill(ptr.begin(), ptr.end() - 1);
    for (E_ID e = 0; e < m; e++) {
      V_ID lo = (V_ID)(keys[e] >> 32), hi = (V_ID)(keys[e] & 0xFFFFFFFFu);
      nbr[fill[lo]++] = hi;
      nbr[fill[hi]++] = lo;
    }
  }
  // the priority permutation: ascending (key, id)
  std::vector<uint64_t> key(nv, 0);
  for (V_ID v = 0; v < nv; v++) {
    if (order == 0) key[v] = ~(uint64_t)(ptr[v + 1] - ptr[v]);
    if (order == 2) key[v] = splitmix64(seed ^ (uint64_t)v) >> 1;
  }
  std::vector<V_ID> perm(nv);
  for (V_ID v = 0; v < nv; v++) perm[v] = v;
  std::sort(perm.begin(), perm.end(), [&](V_ID x, V_ID y) {
    return key[x] != key[y] ? key[x] < key[y] : x < y;
  });
  std::vector<V_ID> stamp((size_t)nv + 1, 0);
  for (V_ID v = 0; v < nv; v++) colour[v] = -1;
  for (V_ID k = 0; k < nv; k++) {
    V_ID v = perm[k];
    for (E_ID i = ptr[v]; i < ptr[v + 1]; i++) {
      int32_t c = colour[nbr[i]];
      if (c >= 0) stamp[c] = v + 1;
    }
    int32_t c = 0;
    while (stamp[c] == v + 1) c++;
    colour[v] = c;
  }
  return 0;
}

// ---------- strongly connected components ----------
// Exact oracle of SCCEngine (no reference equivalent), on the directed graph
// as loaded: row v of the CSC lists the sources u of the edges u -> v.
// label[v] = the largest vertex id of v's SCC. Tarjan's algorithm with an
// explicit call stack (no recursion: a path of thousands of vertices is a
// test). The search walks the CSC rows, i.e. the reversed graph, whose SCCs
// are the same. No trim, no pivot, no colouring.
void scc_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
             uint32_t* label) {
  (void)ne;
  constexpr uint32_t UNSEEN = 0xFFFFFFFFu;
  std::vector<uint32_t> index(nv, UNSEEN), low(nv, 0);
  std::vector<uint8_t> on_stack(nv, 0);
  std::vector<V_ID> stack, call;
  std::vector<E_ID> next(nv, 0);  // the next in-edge of a vertex on `call`
  uint32_t counter = 0;
  for (V_ID root = 0; root < nv; root++) {
    if (index[root] != UNSEEN) continue;
    call.push_back(root);
    while (!call.empty()) {
      V_ID v = call.back();
      if (index[v] == UNSEEN) {
        index[v] = low[v] = counter++;
        stack.push_back(v);
        on_stack[v] = 1;
        next[v] = v == 0 ? 0 : col_end[v - 1];
      }
      bool descended = false;
      while (next[v] < col_end[v]) {
        V_ID u = src[next[v]++];
        if (u >= nv) continue;
        if (index[u] == UNSEEN) {
          call.push_back(u);
          descended = true;
          break;
        }
        if (on_stack[u]) low[v] = std::min(low[v], index[u]);
      }
      if (descended) continue;
      call.pop_back();
      if (!call.empty()) {
        V_ID p = call.back();
        low[p] = std::min(low[p], low[v]);
      }
      if (low[v] != index[v]) continue;
      // v is the root of a component: the stack down to v
      size_t first = stack.size();
      V_ID top = 0;
      do {
        first--;
        top = std::max(top, stack[first]);
      } while (stack[first] != v);
      for (size_t i = first; i < stack.size(); i++) {
        label[stack[i]] = top;
        on_stack[stack[i]] = 0;
      }
      stack.resize(first);
    }
  }
}

// ---------- minimum spanning forest ----------
// Exact oracle of MSFEngine (no reference equivalent), on the simple
// undirected graph of tc_cpu. The weight of {lo, hi} is the minimum weight
// over all its occurrences in either direction: the (key, w) pairs are
// sorted and the first of each key kept, which also lists the edges
// ascending by key = (lo << 32) | hi, so the position is the edge id e.
// Kruskal over the strict order (w, e) with a union-find whose roots are
// the largest ids: label[v] = the largest vertex id of v's component.
// lo / hi / w / in_forest: room for ne entries; returns m. No rounds, no
// per-component search.
E_ID msf_cpu(V_ID nv, E_ID ne, const E_ID* col_end, const V_ID* src,
             const WeightType* weight, V_ID* lo, V_ID* hi, WeightType* w,
             uint8_t* in_forest, int64_t* total, uint32_t* label) {
  std::vector<std::pair<uint64_t, WeightType>> kw;
  kw.reserve(ne);
  E_ID b = 0;
  for (V_ID v = 0; v < nv; v++) {
    for (E_ID i = b; i < col_end[v]; i++) {
      V_ID s = src[i];
      if (s == v || s >= nv) continue;
      V_ID l = std::min(s, v), h = std::max(s, v);
      kw.emplace_back(((uint64_t)l << 32) | h, weight[i]);
    }
    b = col_end[v];
  }
  std::sort(kw.begin(), kw.end());
  E_ID m = 0;
  for (size_t i = 0; i < kw.size(); i++) {
    if (i && kw[i].first == kw[i - 1].first) continue;
    lo[m] = (V_ID)(kw[i].first >> 32);
    hi[m] = (V_ID)(kw[i].first & 0xFFFFFFFFu);
    w[m] = kw[i].second;
    in_forest[m] = 0;
    m++;
  }
  std::vector<E_ID> order(m);
  for (E_ID e = 0; e < m; e++) order[e] = e;
  std::sort(order.begin(), order.end(), [&](E_ID x, E_ID y) {
    return w[x] != w[y] ? w[x] < w[y] : x < y;
  });
  std::vector<V_ID> parent(nv);
  for (V_ID v = 0; v < nv; v++) parent[v] = v;
  auto find = [&](V_ID v) {
    while (parent[v] != v) {
      parent[v] = parent[parent[v]];
      v = parent[v];
    }
    return v;
  };
  int64_t sum = 0;
  for (E_ID k = 0; k < m; k++) {
    E_ID e = order[k];
    V_ID ra = find(lo[e]), rb = find(hi[e]);
    if (ra == rb) continue;
    parent[std::min(ra, rb)] = std::max(ra, rb);
    in_forest[e] = 1;
    sum += w[e];
  }
  *total = sum;
  for (V_ID v = 0; v < nv; v++) label[v] = find(v);
  return m;
}

// ---------- Collaborative filtering ----------

void cf_init(V_ID nv, int K, float* vec) {
  float v0 = std::sqrt(1.0f / K);  // reference init (colfilter_gpu.cu:260-264)
  for (uint64_t i = 0; i < (uint64_t)nv * K; i++) vec[i] = v0;
}

void cf_iter_part(V_ID row_left, V_ID row_right, E_ID col_left,
                  const E_ID* col_end, const V_ID* src, const WeightType* w,
                  int K, const float* old_vec, float* new_vec_part) {
  std::vector<float> acc(K);
  for (V_ID v = row_left; v <= row_right; v++) {
    E_ID b = (v == row_left) ? col_left : col_end[v - 1 - row_left];
    E_ID e = col_end[v - row_left];
    const float* dv = old_vec + (uint64_t)v * K;
    std::fill(acc.begin(), acc.end(), 0.0f);
    for (E_ID i = b; i < e; i++) {
      const float* sv = old_vec + (uint64_t)src[i - col_left] * K;
      float dot = 0.0f;
      for (int k = 0; k < K; k++) dot += sv[k] * dv[k];
      float err = (float)w[i - col_left] - dot;
      for (int k = 0; k < K; k++) acc[k] += err * sv[k];
    }
    float* nv_ = new_vec_part + (uint64_t)(v - row_left) * K;
    for (int k = 0; k < K; k++)
      nv_[k] = dv[k] + CF_GAMMA * (acc[k] - CF_LAMBDA * dv[k]);
  }
}

void cf_cpu(const HostCSC& g, int K, int iters, float* vec_out) {
  std::vector<float> oldv((uint64_t)g.nv * K), newv((uint64_t)g.nv * K);
  cf_init(g.nv, K, oldv.data());
  for (int it = 0; it < iters; it++) {
    cf_iter_part(0, g.nv - 1, 0, g.col_end.data(), g.src.data(),
                 g.weight.data(), K, oldv.data(), newv.data());
    std::swap(oldv, newv);
  }
  std::memcpy(vec_out, oldv.data(), sizeof(float) * (uint64_t)g.nv * K);
}

// CF training loss (for tests: loss must decrease over sweeps).
double cf_loss(const HostCSC& g, int K, const float* vec) {
  double loss = 0;
  for (V_ID v = 0; v < g.nv; v++) {
    const float* dv = vec + (uint64_t)v * K;
    for (E_ID i = g.row_begin(v); i < g.row_end(v); i++) {
      const float* sv = vec + (uint64_t)g.src[i] * K;
      float dot = 0.0f;
      for (int k = 0; k < K; k++) dot += sv[k] * dv[k];
      double err = (double)g.weight[i] - dot;
      loss += err * err;
    }
  }
  return loss;
}

}  // namespace lux
