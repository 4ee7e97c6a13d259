// Exact subgraph-isomorphism labels on the DEVICE: per (pattern, graph) pair the number of matches, the number of trials
// the search made, and -- without ever storing a match row -- the node and edge weights the matching loss is trained on
// (compute_nodeseq_subisoweights / compute_edgeseq_subisoweights as sums over matches).  The semantics are those of
// dmp_subiso.cpp, node order included: pattern nodes are placed in id order, a candidate for node k is a graph node of
// k's label that no earlier node uses, it is accepted when every pattern edge whose later endpoint is k has an image edge
// with its label, and a TRIAL is one candidate whose edge checks are evaluated.  Integers only: every sum is an integer
// atomic, so the result does not depend on the order of arrival and two runs are equal bit for bit.
//
// The image of a batch (dmp_subiso_image, built by subiso.py in vectorised numpy before the upload):
//   pattern  per node k its candidate range [cbeg, cend) in the graph's candidate list and tend = the end of the run of
//            pattern edges whose later endpoint is k (edges sorted by that endpoint, ties in edge order);
//   graph    the DISTINCT (src, dst, label) edges sorted, as a CSR by source of 64-bit keys dst << 32 | label code, the
//            nodes sorted by (label, id) (the candidate lists back to back) and, per original edge, its distinct entry.
// Parallel graph edges of one label are one entry: the search never walks duplicates, the edge weights are summed per
// entry and subiso_expand_k copies an entry's sum to every edge that shares it.
//
// Decomposition: a work item is (pair, image of pattern node 0).  A workgroup is ONE wave that takes up to 64 consecutive
// root candidates of one pair (a "chunk"; a heavy pair is many chunks), stages that pair's image in LDS once and lets
// every lane run its own iterative depth-first search: map, candidate cursors and the used-node bitmask are LDS columns
// of the lane ([depth][lane]: conflict free), edge lookups are binary searches in the source's CSR row in LDS.
// Divergence (cdna_hip_programming.md Guideline 5): the lanes of a wave share the pair, hence the LDS image and the
// loop bounds, but not the branch they are in.  The search is therefore ONE loop whose every trip does one step of the
// same shape in every lane (fetch the next candidate of the lane's depth; skip / test / descend / backtrack as
// predicated tails), so a wave runs one instruction stream and lanes differ only in the short edge-check loop (the
// number of pattern edges at the lane's depth) -- there is no per-lane recursion to serialise.  A lane that has finished
// idles until the wave's longest root is done; chunks are fine-grained enough (64 roots) for other waves to fill the CU.
// Atomics (Guideline 12): per lane in registers (count, trials), per workgroup in LDS (64-bit LDS adds of the weights),
// then one 64-bit global atomic per touched node / entry / pair and workgroup.
//
// Bounded by construction: every item carries a trial budget.  The one search loop makes at most
// (budget + 1) * (pn + 2) trips (a trip is a trial, a backtrack -- at most one per accepted trial -- or a skip of a used
// node -- at most pn - 1 per scanned list, one list per accepted trial), counted and capped; the edge-check loop is
// bounded by pm, the binary search by 12 halvings (2048 entries).  An item that needs a trial beyond its budget stops
// and clears its pair's `complete`; the outputs of such a pair are not used.  Everything read from the image is checked
// against the LDS capacities while it is staged: a value out of range makes the pair incomplete, never an access.
#include "dmp_common.h"

namespace {

using u64 = unsigned long long;
constexpr int kLanes = 64;                                     // one wave per workgroup
constexpr int kMaxPn = DMP_SUBISO_MAX_PN, kMaxPm = DMP_SUBISO_MAX_PM;
constexpr int kMaxGn = DMP_SUBISO_MAX_GN, kMaxGm = DMP_SUBISO_MAX_GM;
constexpr int kUsedWords = kMaxGn / 32;
constexpr int kChunksPerLaunch = 2048;                         // 131072 items: what the default budget is sized for
constexpr int kDesc = DMP_SUBISO_DESC_WORDS;
static_assert(kMaxGn % 32 == 0 && kMaxGm <= 4096 && kMaxGn <= 65535, "rowptr / candidates are staged as uint16, 12 halvings");

// dynamic LDS, 8-byte words first: ent [max_um] | nw [max_gn] uw [max_um] (weights only) | acc [2]
//   then 4-byte: used [16][64] | pe [64] pel [64] | tend cbeg cend [16] each | flags [2]
//   then 2-byte: rowptr [max_gn + 1] cand [max_gn] | map [16][64] pos [16][64]
__host__ __device__ inline size_t lds_bytes(int max_gn, int max_um, bool weights) {
  size_t b = 8 * ((size_t)max_um + (weights ? (size_t)max_gn + max_um : 0) + 2);
  b += 4 * ((size_t)kUsedWords * kLanes + 2 * kMaxPm + 3 * kMaxPn + 2);
  b += 2 * ((size_t)(max_gn + 1) + max_gn + 2 * kMaxPn * kLanes);
  return (b + 7) & ~(size_t)7;
}

__device__ __forceinline__ bool admitted(int pn, int pm, int gn, int um, int max_gn, int max_um) {
  return pn >= 0 && pn <= kMaxPn && pm >= 0 && pm <= kMaxPm && gn >= 0 && gn <= max_gn && max_gn <= kMaxGn && um >= 0 &&
         um <= max_um && max_um <= kMaxGm;
}

// every element of every output: counts (1 for an empty pattern), trials 0, complete = the pair is admitted, weights 0
__global__ __launch_bounds__(256) void subiso_init_k(dmp_subiso_image im, int64_t total, int64_t *counts, int64_t *trials,
                                                     uint8_t *complete, int64_t *node_w, int64_t *uw) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  if (idx < im.num_pairs) {
    const int32_t *d = im.desc + idx * kDesc;
    const bool ok = admitted(d[0], d[1], d[2], d[3], im.max_gn, im.max_um);
    counts[idx] = (ok && d[0] == 0) ? 1 : 0;
    trials[idx] = 0;
    complete[idx] = ok ? 1 : 0;
  }
  if (node_w && idx < im.total_gn) node_w[idx] = 0;
  if (uw && idx < im.total_um) uw[idx] = 0;
}

__global__ __launch_bounds__(256) void subiso_expand_k(dmp_subiso_image im, const int64_t *uw, int64_t *edge_w) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= im.total_gm) return;
  const int32_t u = im.g_inv[idx];
  edge_w[idx] = (u >= 0 && u < im.total_um) ? uw[u] : 0;
}

// the entry (mu -> mv, lab) in mu's CSR row, or -1: at most 12 halvings (um <= 4096)
__device__ __forceinline__ int find_entry(const u64 *ent, const uint16_t *rowptr, int mu, int mv, int lab) {
  int lo = rowptr[mu];
  const int end = rowptr[mu + 1];
  int hi = end;
  const u64 key = ((u64)(uint32_t)mv << 32) | (uint32_t)lab;
  for (int it = 0; it < 12 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if (ent[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < end && ent[lo] == key) ? lo : -1;
}

template <bool W>
__global__ __launch_bounds__(kLanes) void subiso_search_k(dmp_subiso_image im, int64_t chunk0, int64_t budget, int64_t *counts,
                                                          int64_t *trials, uint8_t *complete, int64_t *node_w, int64_t *uw_out) {
  extern __shared__ u64 smem[];
  const int lane = threadIdx.x;
  const int64_t c = chunk0 + blockIdx.x;
  if (c >= im.num_chunks) return;
  const int i = im.chunk_pair[c], root0 = im.chunk_root[c];
  if (i < 0 || i >= im.num_pairs) return;
  const int32_t *d = im.desc + (int64_t)i * kDesc;
  const int pn = d[0], pm = d[1], gn = d[2], um = d[3];
  const int64_t pno = d[4], peo = d[5], gno = d[6], uo = d[7];
  const int max_gn = im.max_gn, max_um = im.max_um;
  // uniform over the workgroup: every lane read the same words
  if (!(admitted(pn, pm, gn, um, max_gn, max_um) && pn >= 1 && gn >= 1 && root0 >= 0 && root0 < gn && pno >= 0 && pno + pn <= im.total_pn &&
        peo >= 0 && peo + pm <= im.total_pm && gno >= 0 && gno + gn <= im.total_gn && uo >= 0 && uo + um <= im.total_um)) {
    if (lane == 0) complete[i] = 0;
    return;
  }
  u64 *ent = smem;
  u64 *nw = ent + max_um;
  u64 *uw = nw + (W ? max_gn : 0);
  u64 *acc = uw + (W ? max_um : 0);
  uint32_t *used = reinterpret_cast<uint32_t *>(acc + 2);
  int32_t *pe = reinterpret_cast<int32_t *>(used + kUsedWords * kLanes);
  int32_t *pel = pe + kMaxPm;
  int32_t *tend = pel + kMaxPm, *cbeg = tend + kMaxPn, *cend = cbeg + kMaxPn;
  int32_t *flags = cend + kMaxPn;                              // [0] the image is bad, [1] a lane ran out of budget
  uint16_t *rowptr = reinterpret_cast<uint16_t *>(flags + 2);
  uint16_t *cand = rowptr + (max_gn + 1);
  uint16_t *map = cand + max_gn;                               // [depth][lane]
  uint16_t *pos = map + kMaxPn * kLanes;

  // ---- stage the pair's image, checking every value that will index LDS
  int bad = 0;
  if (lane < 2) { flags[lane] = 0; acc[lane] = 0; }
  for (int j = lane; j < um; j += kLanes) {
    const u64 e = (u64)im.g_ent[uo + j];
    bad |= (e >> 32) >= (u64)gn;
    ent[j] = e;
    if (W) uw[j] = 0;
  }
  for (int j = lane; j <= gn; j += kLanes) {
    const int64_t r = (int64_t)im.g_rowptr[gno + j] - uo;
    bad |= r < 0 || r > um;
    rowptr[j] = (uint16_t)r;
  }
  for (int j = lane; j < gn; j += kLanes) {
    const int v = im.g_cand[gno + j];
    bad |= v < 0 || v >= gn;
    cand[j] = (uint16_t)v;
    if (W) nw[j] = 0;
  }
  if (lane < pm) {
    const int e = im.p_ends[peo + lane];
    bad |= e < 0 || (e & 255) >= pn || (e >> 8) >= pn;
    pe[lane] = e;
    pel[lane] = im.p_elab[peo + lane];
  }
  if (lane < pn) {
    const int t = im.p_tend[pno + lane], b = im.p_cbeg[pno + lane], e = im.p_cend[pno + lane];
    bad |= t < 0 || t > pm || b < 0 || b > gn || e < 0 || e > gn;
    tend[lane] = t; cbeg[lane] = b; cend[lane] = e;
  }
  for (int k = 0; k < kMaxPn; ++k) map[k * kLanes + lane] = 0;  // a slot never placed reads as node 0: inside the graph
  for (int w = 0; w < kUsedWords; ++w) used[w * kLanes + lane] = 0;
  __syncthreads();
  if (bad) atomicOr(&flags[0], 1);
  __syncthreads();
  if (flags[0]) {
    if (lane == 0) complete[i] = 0;
    return;
  }

  // ---- the search: one step per trip, the same step shape in every lane
  const int root = cbeg[0] + root0 + lane;
  bool active = root < cend[0];
  bool over = false;
  u64 cnt = 0;
  int64_t tr = 0;
  int k = 0;
  pos[lane] = (uint16_t)(active ? root : 0);
  const int64_t max_steps = (budget + 1) * (pn + 2);
  for (int64_t step = 0; active && step < max_steps; ++step) {
    const int cur = pos[k * kLanes + lane];
    const int end = k == 0 ? root + 1 : cend[k];
    if (cur >= end) {                                           // this depth's list is spent: backtrack
      if (k == 0) { active = false; continue; }
      --k;
      const int v = map[k * kLanes + lane];
      used[(v >> 5) * kLanes + lane] &= ~(1u << (v & 31));
      continue;
    }
    pos[k * kLanes + lane] = (uint16_t)(cur + 1);
    const int v = cand[cur];
    if (used[(v >> 5) * kLanes + lane] >> (v & 31) & 1u) continue;
    if (tr >= budget) { over = true; break; }
    ++tr;
    map[k * kLanes + lane] = (uint16_t)v;
    bool good = true;
    const int t1 = tend[k];
    for (int e = k == 0 ? 0 : tend[k - 1]; e < t1 && e < kMaxPm; ++e) {
      const int se = pe[e];
      if (find_entry(ent, rowptr, map[(se & 255) * kLanes + lane], map[(se >> 8) * kLanes + lane], pel[e]) < 0) {
        good = false;
        break;
      }
    }
    if (!good) continue;
    if (k + 1 < pn) {                                           // descend
      used[(v >> 5) * kLanes + lane] |= 1u << (v & 31);
      ++k;
      pos[k * kLanes + lane] = (uint16_t)cbeg[k];
      continue;
    }
    ++cnt;                                                      // a match: the last node stays a candidate slot
    if (W) {
      for (int j = 0; j < pn; ++j) atomicAdd(&nw[map[j * kLanes + lane]], (u64)1);
      for (int e = 0; e < pm; ++e) {
        const int se = pe[e];
        const int at = find_entry(ent, rowptr, map[(se & 255) * kLanes + lane], map[(se >> 8) * kLanes + lane], pel[e]);
        if (at >= 0) atomicAdd(&uw[at], (u64)1);
      }
    }
  }
  if (active && !over) over = true;                             // the trip cap (never met: see the header) is a spent budget too

  // ---- per workgroup, then one global atomic per pair / touched node / touched entry
  if (cnt) atomicAdd(&acc[0], cnt);
  if (tr) atomicAdd(&acc[1], (u64)tr);
  if (over) atomicOr(&flags[1], 1);
  __syncthreads();
  if (lane == 0) {
    if (acc[0]) atomicAdd(reinterpret_cast<u64 *>(counts + i), acc[0]);
    if (acc[1]) atomicAdd(reinterpret_cast<u64 *>(trials + i), acc[1]);
    if (flags[1]) complete[i] = 0;
  }
  if (W) {
    if (node_w)
      for (int j = lane; j < gn; j += kLanes)
        if (nw[j]) atomicAdd(reinterpret_cast<u64 *>(node_w + gno + j), nw[j]);
    if (uw_out)
      for (int j = lane; j < um; j += kLanes)
        if (uw[j]) atomicAdd(reinterpret_cast<u64 *>(uw_out + uo + j), uw[j]);
  }
}

}  // namespace

using namespace dmp;

extern "C" {

int dmp_subiso_label_dev(const dmp_subiso_image *image, int64_t budget, int64_t *counts, int64_t *trials, uint8_t *complete,
                         int64_t *node_weights, int64_t *edge_weights, int64_t *workspace, void *stream) {
  if (!image) return DMP_ERR_BAD_ARG;
  const dmp_subiso_image im = *image;
  const int64_t lim = (int64_t)1 << 31;
  if (im.num_pairs < 0 || im.num_chunks < 0 || im.total_pn < 0 || im.total_pm < 0 || im.total_gn < 0 || im.total_gm < 0 ||
      im.total_um < 0 || im.total_um > im.total_gm || budget < 1 || budget > DMP_SUBISO_MAX_BUDGET)
    return DMP_ERR_BAD_ARG;
  if (im.num_pairs >= lim || im.total_pn >= lim || im.total_pm >= lim || im.total_gn >= lim || im.total_gm >= lim ||
      im.num_chunks >= lim || im.max_gn < 0 || im.max_gn > kMaxGn || im.max_um < 0 || im.max_um > kMaxGm)
    return DMP_ERR_UNSUPPORTED;
  if (im.num_pairs == 0) return DMP_OK;
  if (!im.desc || !counts || !trials || !complete || (edge_weights && !workspace) ||
      (im.num_chunks > 0 && (!im.chunk_pair || !im.chunk_root || !im.g_rowptr || !im.g_cand || !im.p_cbeg || !im.p_cend || !im.p_tend)) ||
      (im.total_um > 0 && !im.g_ent) || (im.total_pm > 0 && (!im.p_ends || !im.p_elab)) || (edge_weights && im.total_gm > 0 && !im.g_inv))
    return DMP_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  int64_t *uw = edge_weights ? workspace : nullptr;
  int64_t total = im.num_pairs;
  if (node_weights && im.total_gn > total) total = im.total_gn;
  if (uw && im.total_um > total) total = im.total_um;
  subiso_init_k<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(im, total, counts, trials, complete, node_weights, uw);
  const bool w = node_weights || uw;
  const size_t lds = lds_bytes(im.max_gn, im.max_um, w);      // at the limits 26.7 / 46.7 KiB: below the 64 KiB that need no opt-in
  for (int64_t c0 = 0; c0 < im.num_chunks; c0 += kChunksPerLaunch) {
    const int64_t nc = im.num_chunks - c0 < kChunksPerLaunch ? im.num_chunks - c0 : kChunksPerLaunch;
    if (w)
      subiso_search_k<true><<<(unsigned)nc, kLanes, lds, s>>>(im, c0, budget, counts, trials, complete, node_weights, uw);
    else
      subiso_search_k<false><<<(unsigned)nc, kLanes, lds, s>>>(im, c0, budget, counts, trials, complete, nullptr, nullptr);
  }
  if (edge_weights && im.total_gm > 0)
    subiso_expand_k<<<(unsigned)((im.total_gm + 255) / 256), 256, 0, s>>>(im, uw, edge_weights);
  return check_launch();
}

}  // extern "C"
