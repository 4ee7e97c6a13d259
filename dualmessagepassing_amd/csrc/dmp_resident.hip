// A batch assembled on the device from a resident dataset: dmp_collate_resident (include/dmp_hip.h).
//
// One workgroup per slot of the batch, one launch for both sides and the tail.  A slot's sizes and output offsets are
// differences / entries of the plan's prefix sums, which every lane of the workgroup reads at the same address (scalar
// loads): no search, no LDS.  A real slot streams its sample's rows out of the store (int32 / uint8 in, int64 / uint8 out,
// lane i on element i: coalesced both ways); an inert slot computes its ring.  The workgroups past the last slot zero the
// unused end of sub_flat, a fixed chunk each.  Every output element has exactly one writer.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kZeroChunk = kBlock * 16;      // int64 elements of sub_flat one trailing workgroup zeroes (32 KiB)

struct ResidentArgs {
  dmp_resident_side store[2];
  dmp_resident_batch out[2];
  const float *counts;
  const int32_t *subs;
  const int64_t *sub_ptr, *plan;
  float *o_counts, *o_weights;
  int64_t *sub_flat, *sample_ptr;
  int64_t slots, real, sub_capacity, sub_total;
};

__global__ __launch_bounds__(kBlock) void collate_resident_k(const ResidentArgs a) {
  const int64_t b = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t P = a.slots;
  if (b >= P) {                                  // the zeros behind the batch's rows
    const int64_t lo = a.sub_total + (b - P) * kZeroChunk;
    const int64_t hi = lo + kZeroChunk < a.sub_capacity ? lo + kZeroChunk : a.sub_capacity;
    for (int64_t i = lo + t; i < hi; i += kBlock) a.sub_flat[i] = 0;
    return;
  }
  const int64_t *label = a.plan, *sample = a.plan + 4, *prefix = a.plan + 4 + P;
  const bool real = b < a.real;
  const int64_t s = real ? sample[b] : 0;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const dmp_resident_side &S = a.store[side];
    const dmp_resident_batch &O = a.out[side];
    const int64_t *noff = prefix + (2 * side) * (P + 1), *eoff = prefix + (2 * side + 1) * (P + 1);
    const int64_t n0 = noff[b], e0 = eoff[b];
    const int n = (int)(noff[b + 1] - n0), e = (int)(eoff[b + 1] - e0);
    if (real) {
      const int64_t sn = S.node_ptr[s], se = S.edge_ptr[s];
      for (int i = t; i < n; i += kBlock) {
        O.nid[n0 + i] = i;
        O.vlabel[n0 + i] = S.vlabel[sn + i];
      }
      for (int j = t; j < e; j += kBlock) {
        O.src[e0 + j] = S.src[se + j];
        O.dst[e0 + j] = S.dst[se + j];
        O.eid[e0 + j] = S.eid[se + j];
        O.elabel[e0 + j] = S.elabel[se + j];
        O.rev[e0 + j] = S.rev[se + j];
      }
    } else {
      const int64_t vl = label[2 * side], el = label[2 * side + 1];
      const uint32_t un = n > 0 ? (uint32_t)n : 1u;
      for (int i = t; i < n; i += kBlock) {
        O.nid[n0 + i] = i;
        O.vlabel[n0 + i] = vl;
      }
      for (int j = t; j < e; j += kBlock) {
        const uint32_t u = (uint32_t)j % un, v = u + 1 == un ? 0u : u + 1;
        O.src[e0 + j] = u;
        O.dst[e0 + j] = v;
        O.eid[e0 + j] = j;
        O.elabel[e0 + j] = el;
        O.rev[e0 + j] = 0;
      }
    }
    if (t == 0) {
      O.num_nodes[b] = n;
      O.num_edges[b] = e;
    }
  }
  if (t == 0) {
    a.o_counts[b] = real ? a.counts[s] : 0.f;
    if (a.o_weights) a.o_weights[b] = real ? 1.f : 0.f;
  }
  if (a.sample_ptr) {                            // the tail; sub_flat may be NULL when its capacity is 0: nothing is stored to it then
    const int64_t *roff = prefix + 4 * (P + 1);
    const int64_t r0 = roff[b], r = roff[b + 1] - r0;
    if (t == 0) {
      a.sample_ptr[b] = r0;
      if (b == P - 1) a.sample_ptr[P] = roff[P];
    }
    if (real && r > 0) {
      const int64_t ss = a.sub_ptr[s];
      for (int64_t i = t; i < r; i += kBlock) a.sub_flat[r0 + i] = a.subs[ss + i];
    }
  }
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_collate_resident(const dmp_resident_side *store, const float *counts, const int32_t *subs, const int64_t *sub_ptr,
                         const int64_t *plan, int64_t slots, int64_t real, const dmp_resident_batch *out, float *o_counts,
                         float *o_weights, int64_t *sub_flat, int64_t sub_capacity, int64_t sub_total, int64_t *sample_ptr,
                         void *stream) {
  if (!store || !out || !plan || !counts || !o_counts || slots < 1 || real < 1 || real > slots) return DMP_ERR_BAD_ARG;
  if (sub_flat && !sample_ptr) return DMP_ERR_BAD_ARG;
  if (sample_ptr && (!sub_ptr || sub_total < 0 || sub_capacity < sub_total || (sub_total > 0 && !subs) || (sub_capacity > 0 && !sub_flat)))
    return DMP_ERR_BAD_ARG;
  if (slots > DMP_RESIDENT_MAX_SLOTS) return DMP_ERR_UNSUPPORTED;
  ResidentArgs a;
  for (int side = 0; side < 2; ++side) {
    if (!store[side].node_ptr || !store[side].edge_ptr || !out[side].num_nodes || !out[side].num_edges) return DMP_ERR_BAD_ARG;
    a.store[side] = store[side];
    a.out[side] = out[side];
  }
  a.counts = counts, a.subs = subs, a.sub_ptr = sub_ptr, a.plan = plan;
  a.o_counts = o_counts, a.o_weights = o_weights, a.sub_flat = sub_flat, a.sample_ptr = sample_ptr;
  a.slots = slots, a.real = real;
  a.sub_capacity = sample_ptr ? sub_capacity : 0, a.sub_total = sample_ptr ? sub_total : 0;
  const int64_t zero_blocks = (a.sub_capacity - a.sub_total + kZeroChunk - 1) / kZeroChunk;
  if (zero_blocks > (int64_t(1) << 30)) return DMP_ERR_UNSUPPORTED;
  collate_resident_k<<<dim3((unsigned)(slots + zero_blocks)), kBlock, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

}  // extern "C"
