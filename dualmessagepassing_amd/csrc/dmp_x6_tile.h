// A tile product on the bf16 matrix pipe ("bf16x6", dmp_mfma_common.h) and the scaffolding around it, for those of the kernels
// that keep a [32, K] operand tile as three bf16 planes in LDS and their [K, 32] panel slice as piece fragments in registers which compile to the same code through it:
// the k-group loop (one per fence placement: the two are two schedules), the accumulator block through a wave's scratch, the plain
// panel load, and the geometry of the two two-role edge MLP kernels (dmp_edgemlp.hip, dmp_l0mlp.hip).  gfx950 only.
#pragma once
#include "dmp_mfma_common.h"

namespace dmp {

// The fragment read of an image with padded rows: k-group g of this lane's row lies 4 g dwords behind `ar`, the mid and lo planes
// kPlaneDwords and 2 kPlaneDwords behind the hi plane (one ds_read_b128 each).
template <int kPlaneDwords>
struct PaddedRowRead {
  const uint32_t *ar;
  __device__ __forceinline__ void operator()(int g, Frag8 &hi, Frag8 &mid, Frag8 &lo) const {
    hi.v = *reinterpret_cast<const bf16x8 *>(ar + 4 * g);
    mid.v = *reinterpret_cast<const bf16x8 *>(ar + kPlaneDwords + 4 * g);
    lo.v = *reinterpret_cast<const bf16x8 *>(ar + 2 * kPlaneDwords + 4 * g);
  }
};

// acc += A B over G 16-deep k-groups: six piece MFMAs per group on the A fragments read(g, hi, mid, lo) fetches -- requested one
// group ahead -- and the panel fragment B[g], with the caller's actions (requests / staging of the neighbouring tiles) in their
// shadow.  "3 + 3": fence, three MFMAs, fence, action(2 g), fence, three MFMAs, fence, action(2 g + 1).  (edge_mlp_k.  The row
// waves of dmp_h1w.hip's two kernels run the same schedule from loops of their own: through this template they compiled to other
// registers; the cause is not established.)
template <int G, class Read, class Action>
__device__ __forceinline__ void x6_kgroups(Read &&read, const Split8 *B, f32x16 &acc, Action &&action) {
  Frag8 ah, am, al;
  read(0, ah, am, al);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    Frag8 nh = ah, nm = am, nl = al;
    if (g + 1 < G) read(g + 1, nh, nm, nl);
    const Split8 &bb = B[g];
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al.v, bb.hi.v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bb.lo.v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am.v, bb.mid.v, acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    action(2 * g);
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am.v, bb.hi.v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bb.mid.v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bb.hi.v, acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    action(2 * g + 1);
    ah = nh; am = nm; al = nl;
  }
}

// The other placement: a fence after EVERY MFMA, the group's kPer actions (16 over the tile: 2 at G = 8, 4 at G = 4) spread evenly
// behind its six MFMAs.  (typed_body; dmp_mfma.hip's pipelined step keeps its own copy: through this template its
// prologue's scalar instructions came out in another order.)
template <int G, class Read, class Action>
__device__ __forceinline__ void x6_kgroups_fenced(Read &&read, const Split8 *B, f32x16 &acc, Action &&action) {
  constexpr int kPer = 16 / G;
  Frag8 ah, am, al;
  read(0, ah, am, al);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    Frag8 nh = ah, nm = am, nl = al;
    if (g + 1 < G) read(g + 1, nh, nm, nl);
    const Split8 &bb = B[g];
    auto after = [&](int n) {                               // the actions due after the n-th MFMA of the group
#pragma unroll
      for (int q = 0; q < kPer; ++q)
        if (6 * (q + 1) / kPer == n) action(kPer * g + q);
      __builtin_amdgcn_sched_barrier(0);
    };
    __builtin_amdgcn_sched_barrier(0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al.v, bb.hi.v, acc, 0, 0, 0); after(1);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bb.lo.v, acc, 0, 0, 0); after(2);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am.v, bb.mid.v, acc, 0, 0, 0); after(3);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am.v, bb.hi.v, acc, 0, 0, 0); after(4);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bb.mid.v, acc, 0, 0, 0); after(5);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah.v, bb.hi.v, acc, 0, 0, 0); after(6);
    ah = nh; am = nm; al = nl;
  }
}

// The accumulator block through the wave's scratch: lane (li, h) holds rows (r & 3) + 8 (r >> 2) + 4 h of column li; read back as
// rows of 4 consecutive columns per lane (written and read by the same wave: LDS operations of one wave complete in order).
// (edge_mlp_k, l0_edge_mlp_k.  The other kernels with this loop keep it: through this function their store addresses were formed
// otherwise and the registers changed; the cause is not established.)
__device__ __forceinline__ void acc_to_scr(float *scr, const f32x16 &acc, int h, int li) {
#pragma unroll
  for (int r = 0; r < 16; ++r) scr[((r & 3) + 8 * (r >> 2) + 4 * h) * kScrStride + li] = acc[r];
}

// A plain panel slice as piece fragments: B6[g] = the 8 values at byte offsets first_offset + (8 g + j) step of rs_W.  32 values per
// round trip: with a few tiles per workgroup the panel's dependent round trips ARE the launch.  `in_flight` runs behind the first
// round's requests.
template <int G, class InFlight>
__device__ __forceinline__ void load_panel_x6(Split8 (&B6)[G], rsrc_t rs_W, uint32_t first_offset, uint32_t step, InFlight &&in_flight) {
  static_assert(G % 4 == 0, "rounds of 32 values");
  // The offsets hang off a value the optimiser cannot see through: otherwise it hoists the address computations out of the
  // caller's tile loop and keeps them live in registers across it.
  uint32_t off;
  asm volatile("v_mov_b32 %0, %1" : "=v"(off) : "v"(first_offset));
#pragma unroll
  for (int s0 = 0; s0 < 8 * G; s0 += 32) {
    float w0[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) w0[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_W, (int)off, (int)((s0 + j) * step), 0));
    if (s0 == 0) in_flight();
#pragma unroll
    for (int q = 0; q < 32; q += 8)
      split8(make_float4(w0[q], w0[q + 1], w0[q + 2], w0[q + 3]), make_float4(w0[q + 4], w0[q + 5], w0[q + 6], w0[q + 7]), B6[(s0 + q) / 8]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int G>
__device__ __forceinline__ void load_panel_x6(Split8 (&B6)[G], rsrc_t rs_W, uint32_t first_offset, uint32_t step) {
  load_panel_x6(B6, rs_W, first_offset, step, [] {});
}

// ---- the geometry the two two-role edge MLP kernels share (edge_mlp_k, l0_edge_mlp_k): a 512-thread workgroup at H = 128, the H1
// image as two buffers of three bf16 planes with padded rows, the per-row index arrays as rings of kMlpRing tiles.
constexpr int kMlpH = 128, kMlpThreads = 512;
constexpr int kMlpStride = (kMlpH + 8) / 2;          // dwords per image row: 128 bf16 + 8 of padding (68 = 4 mod 64: conflict-free ds_read_b128)
constexpr int kMlpPlane = kSub * kMlpStride;         // one bf16 plane of a 32-row tile
constexpr int kMlpTile = 3 * kMlpPlane;              // hi | mid | lo: 6528 dwords = 26112 bytes
constexpr int kMlpRing = 4;                          // tiles whose per-row indices (and l0's code images) are alive at once
constexpr int kMlpHalf = kMlpH / 2, kMlpGroups = kMlpHalf / 8;

}  // namespace dmp
