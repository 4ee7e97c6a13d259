// The ego-net permutation index of local relational pooling for a batched graph (gfx950), integer-exact:
// what SubgraphCountingMatching/dataset.py:1751-1797 + :1817-1860 enumerate per sample with itertools and scipy on the
// host, laid out as lrp.PermIndex wants it (slot / sizes / scale).
//
//   lrp_count_k   a thread per node: the node's distinct non-reversed out-neighbours in ascending order, each with the
//                 LAST edge that reaches it (insertion into the node's own CSR range of two scratch arrays: a list never
//                 outgrows the row it came from), the number of its permutations n! / (n - k)!, k = min(L - 1, n), and
//                 the pooling scale
//   (scan)        dmp_exclusive_scan_i64 over the counts: the first permutation of every node, the total behind them
//   lrp_fill_k    a thread per (permutation, row i of its L x L block): node by binary search over the offsets, the
//                 permutation unranked from its rank (itertools.permutations order = lexicographic in positions), then
//                 the L slots of row i -- the node on the diagonal, the edge perm[i] -> perm[j] looked up in perm[i]'s
//                 list elsewhere.  Consecutive threads write consecutive rows of L int64: coalesced.
//
// Every loop is bounded by L, by the neighbour cap or by a CSR row / 31 bisection steps; nothing depends on the order
// threads arrive in (the status word is only OR-ed into), so two runs give the same bits.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kCap = DMP_LRP_MAX_NEIGHBOURS;
constexpr int kMaxL = DMP_LRP_MAX_SEQ_LEN;
static_assert(kCap <= 32, "the unranking keeps the used positions in one 32-bit mask");

// n (n - 1) ... (n - k + 1); n <= 32, k <= 5: below 2^25
__device__ __forceinline__ uint32_t falling(int n, int k) {
  uint32_t r = 1;
  for (int i = 0; i < k; ++i) r *= (uint32_t)(n - i);
  return r;
}

__global__ __launch_bounds__(kBlock) void lrp_count_k(const int32_t *__restrict__ out_ptr, const int32_t *__restrict__ out_ent,
                                                      const int32_t *__restrict__ dst32, int64_t N, int L, int mean,
                                                      int32_t *nbr, int32_t *nbe, int32_t *__restrict__ ndist,
                                                      int64_t *__restrict__ sizes, float *__restrict__ scale,
                                                      unsigned long long *status) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= N) return;
  const int b = out_ptr[v], e = out_ptr[v + 1];
  int nd = 0;
  unsigned long long flags = 0;
  for (int q = b; q < e; ++q) {                       // ascending edge id: a later edge of a pair overwrites the earlier one
    const int ent = out_ent[q];
    if (ent & 1) continue;                            // is_reversed
    const int eid = ent >> 1, d = dst32[eid];
    if (d == (int)v) flags |= DMP_LRP_SELF_LOOP;
    int pos = 0;
    while (pos < nd && nbr[b + pos] < d) ++pos;
    if (pos < nd && nbr[b + pos] == d) {
      nbe[b + pos] = eid;
      continue;
    }
    if (nd == kCap) {                                 // the 33rd distinct neighbour: the node is left without permutations
      flags |= DMP_LRP_OVER_CAP;
      continue;
    }
    for (int s = nd; s > pos; --s) {                  // nd < (non-reversed edges seen so far) <= q - b: inside the row
      nbr[b + s] = nbr[b + s - 1];
      nbe[b + s] = nbe[b + s - 1];
    }
    nbr[b + pos] = d;
    nbe[b + pos] = eid;
    ++nd;
  }
  ndist[v] = nd;
  const int k = nd < L - 1 ? nd : L - 1;
  const int64_t cnt = (flags & DMP_LRP_OVER_CAP) ? 0 : (int64_t)falling(nd, k);
  sizes[v] = cnt;
  scale[v] = mean ? (cnt > 0 ? 1.0f / (float)cnt : 0.0f) : 1.0f;
  if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(kBlock) void lrp_fill_k(const int32_t *__restrict__ out_ptr, const int32_t *__restrict__ nbr,
                                                     const int32_t *__restrict__ nbe, const int32_t *__restrict__ ndist,
                                                     const int64_t *__restrict__ off, int64_t N, int64_t E, int L,
                                                     int64_t capacity, int64_t *__restrict__ slot, unsigned long long *status) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t total = off[N];
  if (row == 0 && total > capacity) atomicOr(status, (unsigned long long)DMP_LRP_DROPPED);
  if (row >= capacity * L) return;
  const int64_t p = row / L, zero = N + E;
  const int i = (int)(row - p * L);
  int64_t *__restrict__ o = slot + row * L;
  bool live = p < total;
  int perm[kMaxL];
  int len = 0;
  if (live) {
    int64_t lo = 0, hi = N;                           // off[lo] <= p < off[hi]; at most 31 halvings (N < 2^31)
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= p) lo = mid; else hi = mid;
    }
    const int v = (int)lo, nd = min(ndist[v], kCap), base = out_ptr[v];
    const int k = nd < L - 1 ? nd : L - 1;
    len = k + 1;
    live = i < len;
    if (live) {
      uint32_t r = (uint32_t)(p - off[lo]), block = falling(nd, k), used = 0;
      perm[0] = v;
#pragma unroll
      for (int t = 0; t < kMaxL - 1; ++t) {
        perm[t + 1] = 0;
        if (t < k) {
          block /= (uint32_t)(nd - t);                // permutations that share the first t + 1 positions
          uint32_t idx = r / block;
          r -= idx * block;
          int pos = 0;
          for (int c = 0; c < kCap; ++c) {            // the idx-th position not used yet (idx < nd - t: always found)
            if (!((used >> c) & 1u)) {
              if (idx == 0) { pos = c; break; }
              --idx;
            }
          }
          used |= 1u << pos;
          perm[t + 1] = nbr[base + pos];
        }
      }
    }
  }
  if (!live) {
    for (int j = 0; j < L; ++j) o[j] = zero;
    return;
  }
  int a = perm[0];
#pragma unroll
  for (int t = 1; t < kMaxL; ++t) a = (t == i) ? perm[t] : a;
  const int abase = out_ptr[a], and_ = min(ndist[a], kCap);
#pragma unroll
  for (int j = 0; j < kMaxL; ++j) {
    if (j >= L) break;
    int64_t val = zero;
    if (j == i) {
      val = a;
    } else if (j < len) {
      const int bnode = perm[j];
      for (int c = 0; c < and_; ++c) {                // a's list is ascending and short: a linear walk
        const int d = nbr[abase + c];
        if (d >= bnode) {
          if (d == bnode) val = N + (int64_t)nbe[abase + c];
          break;
        }
      }
    }
    o[j] = val;
  }
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

size_t dmp_lrp_workspace_words(int64_t N, int64_t E) {
  if (N < 0 || E < 0) return 0;
  return 2 * (size_t)E + (size_t)N + 8;
}

static bool lrp_shape_ok(int64_t N, int64_t E, int L) {
  return L >= 1 && L <= kMaxL && N + E + 1 < ((int64_t)1 << 31);
}

int dmp_lrp_count(const int32_t *out_ptr, const int32_t *out_ent, const int32_t *dst32, int64_t N, int64_t E, int L, int mean,
                  int32_t *ws, int64_t *sizes, float *scale, int64_t *status, void *stream) {
  if (N < 0 || E < 0 || !status) return DMP_ERR_BAD_ARG;
  if (!lrp_shape_ok(N, E, L)) return DMP_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipError_t err = hipMemsetAsync(status, 0, sizeof(int64_t), st);
  if (err != hipSuccess) { set_last_hip_error(err); return DMP_ERR_HIP; }
  if (N == 0) return DMP_OK;
  if (!out_ptr || !ws || !sizes || !scale || (E > 0 && (!out_ent || !dst32))) return DMP_ERR_BAD_ARG;
  int32_t *nbr = ws, *nbe = ws + E, *ndist = ws + 2 * E;
  lrp_count_k<<<(unsigned)((N + kBlock - 1) / kBlock), kBlock, 0, st>>>(out_ptr, out_ent, dst32, N, L, mean, nbr, nbe, ndist, sizes,
                                                                        scale, reinterpret_cast<unsigned long long *>(status));
  return check_launch();
}

int dmp_lrp_fill(const int32_t *out_ptr, const int32_t *ws, const int64_t *off, int64_t N, int64_t E, int L, int64_t capacity,
                 int64_t *slot, int64_t *status, void *stream) {
  if (N < 0 || E < 0 || capacity < 0 || !off || !status || (capacity > 0 && !slot)) return DMP_ERR_BAD_ARG;
  if (!lrp_shape_ok(N, E, L)) return DMP_ERR_UNSUPPORTED;
  if (N > 0 && (!out_ptr || !ws)) return DMP_ERR_BAD_ARG;
  const int64_t rows = capacity * L;
  const int64_t blocks = rows > 0 ? (rows + kBlock - 1) / kBlock : 1;      // one thread at least: it compares total and capacity
  if (capacity >= ((int64_t)1 << 40) || blocks >= ((int64_t)1 << 31)) return DMP_ERR_UNSUPPORTED;
  const int32_t *nbr = ws, *nbe = ws + E, *ndist = ws + 2 * E;
  lrp_fill_k<<<(unsigned)blocks, kBlock, 0, (hipStream_t)stream>>>(out_ptr, nbr, nbe, ndist, off, N, E, L, capacity, slot,
                                                                 reinterpret_cast<unsigned long long *>(status));
  return check_launch();
}

}  // extern "C"
