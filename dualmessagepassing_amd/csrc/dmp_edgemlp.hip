// A layer's edge MLP forward over the kept edges' class tiles as ONE launch (gfx950, H = 128, bf16x6):
//
//   H1[e]  = act(z[e] W_g + P[a_e, 0:H] - P[b_e, H:2H] + be)        (what dmp_edge_fwd_typed makes: mfma_typed<TEPI_EDGE>)
//   out[e] = R[e] + (H1[e] W2 + b2)                                 (what dmp_out_fwd_typed makes:  mfma_typed<TEPI_OUT>)
//
// As two launches the [Ek, H] activation H1 is written by the first and read back by the second.  Here a 512-thread workgroup
// (one per CU, persistent over a contiguous range of the class-sorted tile list) splits its eight waves into two ROLES around one
// LDS image of H1, as h1w_k (csrc/dmp_h1w.hip) does around its operands:
//
//   waves 0-3 ("first")   typed_body<TEPI_EDGE, 128, true> tile for tile: gather the rows of z by slot id, split them once into the
//                         three bf16 planes, six piece MFMAs per k-group against the class panel W_g = A' + c_g B' (registers,
//                         rebuilt at a class boundary of the range), epilogue act((acc + (P[a] - P[b])) + be).  The row goes to
//                         H1 by edge id (the backward needs it saved) AND, split into pieces, into a second double-buffered image;
//   waves 4-7 ("second")  typed_body<TEPI_OUT, 128, true> one tile behind, its operand tile being that image instead of rows staged
//                         from memory: plain panel W2 in registers, epilogue (acc + b2) + R[e], stored by edge id.  R (the layer's
//                         residual, z itself) is fetched again by row index: a row the same workgroup loaded a few tiles before.
//
// Same piece products in the same order, same epilogue order, and a row of a 32x32x16 MFMA chain depends on that row's operands
// only: H1 is bit-identical to dmp_edge_fwd_typed's and out to dmp_out_fwd_typed's on every kept row, whatever tile list the latter
// walks.  One barrier per tile (LDS traffic only); tile k's image is written between barriers k and k+1 and read between k+1 and
// k+2, so two buffers suffice; the per-row index arrays live in a ring of four (tile k+3's are written while tile k's are read).
#include "dmp_x6_tile.h"

namespace dmp {
namespace {

struct EdgeMlpArgs {
  const float *Z; int64_t ldz;                      // input rows [E, 128], gathered by slot id
  const float *W; int64_t ldw;                      // [128, ldw >= 256] = [A' | B']: B_g[k][j] = W[k][j] + c W[k][128 + j]
  const float *P; int64_t ldp; int64_t num_nodes;   // gathered table [N, >= 256]
  const float *bias1;                               // [128] or NULL
  const int32_t *selA, *selB;                       // [E] node ids of the added / subtracted P rows (-1: none)
  const float *W2; int64_t ldw2; int w2_transposed; // 0: B[k][j] = W2[k][j] ([in, out]); 1: B[k][j] = W2[j][k] (nn.Linear's [out, in])
  const float *bias2;                               // [128] or NULL
  const float *R; int64_t ldr;                      // residual rows [E, 128] or NULL
  float *H1; int64_t ldh;                           // saved activation rows [E, 128], scattered by edge id
  float *out; int64_t ldo;                          // output rows [E, 128], scattered by edge id
  int64_t E;
  const int32_t *slot_edge;                         // [tiles * 32] edge id per slot, -1 = padding
  const float *tile_scale;                          // [tiles] c_g of the tile's class
  const int32_t *num_tiles;                         // device scalar: tiles in use
  float slope;
};

// (the workgroup's geometry -- kMlpThreads, the image's kMlpStride / kMlpPlane / kMlpTile, kMlpRing -- is dmp_x6_tile.h's, shared with l0_edge_mlp_k)
constexpr int kImgOffH = 2 * kMlpTile * 4;          // the H1 image behind the z image (two buffers each)
constexpr int kScrOff = 4 * kMlpTile * 4;           // the eight waves' accumulator transposes
constexpr int kRowsOff = kScrOff + 8 * 32 * kScrStride * 4;
constexpr int kEdgeMlpLdsBytes = kRowsOff + 3 * kMlpRing * kSub * 4;   // 104448 + 36864 + 1536 = 142848

__global__ __launch_bounds__(kMlpThreads, 1) void edge_mlp_k(const EdgeMlpArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t *const zimg = reinterpret_cast<uint32_t *>(lds);
  uint32_t *const himg = reinterpret_cast<uint32_t *>(lds + kImgOffH);
  uint32_t *const rowA = reinterpret_cast<uint32_t *>(lds + kRowsOff);            // [kMlpRing][32] each: row INDICES (-1: none)
  uint32_t *const rowB = rowA + kMlpRing * kSub, *const rowC = rowB + kMlpRing * kSub;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool second = wave >= 4;
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5, cs = wave & 3;
  const int gtid = threadIdx.x & 255;                                             // thread of its role
  const int col = 32 * cs + li;
  float *const scr = reinterpret_cast<float *>(lds + kScrOff) + wave * (32 * kScrStride);
  const int lrow = lane >> 3, c4 = 32 * cs + (lane & 7) * 4;
  const uint32_t col4 = (uint32_t)c4 * 4u;
  constexpr uint32_t kRowBytes = kMlpH * 4u;
  constexpr uint32_t kNone = 0xFFFFFFFFu, kOOB = 0xFFFFF000u;

  // this workgroup's contiguous tile range (tiles are sorted by class)
  const int ntiles = __builtin_amdgcn_readfirstlane(*p.num_tiles);
  const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = (int)blockIdx.x * chunk;
  const int hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  const int mine = hi > lo ? hi - lo : 0;
  if (mine == 0) return;                                                          // (uniform per workgroup: before any barrier)

  Split8 B6[kMlpGroups];                    // the role's panel: fragment g = B[kMlpHalf h + 8 g .. + 7][col] as bf16 pieces
  f32x16 acc;
  // The tile's product on the bf16 pipe (x6_kgroups, the "3 + 3" schedule): the A fragments are those of the image row li (this
  // lane's 8 consecutive k = kMlpHalf h + 8 g ..), the caller's 16 actions are spread between the MFMAs.
  auto x6_tile = [&](const uint32_t *img, auto &&action) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    x6_kgroups<kMlpGroups>(PaddedRowRead<kMlpPlane>{img + li * kMlpStride + (kMlpHalf / 2) * h}, B6, acc, action);
  };

  if (!second) {
    // ==================================================================== the first Linear (waves 0-3): mfma_typed<TEPI_EDGE>
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias1) bias4 = *reinterpret_cast<const float4 *>(p.bias1 + c4);
    const float slope = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.slope)));
    const uint32_t rows4 = (uint32_t)(p.E * 4);
    const srsrc_t rs_Z = make_srsrc(p.Z, p.ldz, p.E);
    const srsrc_t rs_H1 = make_srsrc(p.H1, p.ldh, p.E);
    const srsrc_t rs_T = make_srsrc(p.P, p.ldp, p.num_nodes);
    const rsrc_t rs_idxA = make_rsrc(p.selA, rows4);
    const rsrc_t rs_idxB = make_rsrc(p.selB, rows4);
    const rsrc_t rs_slot = make_rsrc(p.slot_edge, (uint32_t)ntiles * (kSub * 4u));   // past the end: reads 0 (guarded below)
    const uint32_t colA = (uint32_t)(gtid & 31) * 16u;
    const int srow = gtid >> 5;                               // this thread stages rows srow + 8 m, float4 piece gtid % 32

    const rsrc_t rs_W = make_rsrc(p.W, (uint32_t)(kMlpH * p.ldw * 4));
    const uint32_t w_first = (uint32_t)((int64_t)kMlpHalf * h * p.ldw + col) * 4u;
    const uint32_t w_step = __builtin_amdgcn_readfirstlane((int)(p.ldw * 4));     // bytes from k to k+1
    auto load_panel = [&](float c) {                          // W_g = A' + c B' (the sum and its split as in typed_body)
      // (the offsets hang off values the optimiser cannot see through: otherwise it hoists the address computations out of the
      // tile loop and keeps them live in registers across it)
      uint32_t off, ws;
      asm volatile("v_mov_b32 %0, %1" : "=v"(off) : "v"(w_first));
      asm volatile("s_mov_b32 %0, %1" : "=s"(ws) : "s"(w_step));
      // 32 rows of both halves per round trip: while this role builds a panel the whole workgroup waits for it (the second role
      // stands at the barrier), so its dependent round trips are the launch's, not one of two workgroups'
#pragma unroll
      for (int s0 = 0; s0 < kMlpHalf; s0 += 32) {
        float w0[32], w1[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          w0[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_W, (int)off, (int)((s0 + j) * ws), 0));
          w1[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_W, (int)off + (int)kRowBytes, (int)((s0 + j) * ws), 0));
        }
#pragma unroll
        for (int q = 0; q < 32; q += 8) {
          float w[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) w[j] = w0[q + j] + c * w1[q + j];
          split8(make_float4(w[0], w[1], w[2], w[3]), make_float4(w[4], w[5], w[6], w[7]), B6[(s0 + q) / 8]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };

    // ---- prefetch: ids of tile k+3, rows of tile k+2 in registers, tile k+1 staged while tile k is computed
    int id_rows[kSubLoads];
    int id_own = -1, own_staged = -1;
    float4 pre[kSubLoads];
    uint32_t pre_a = 0, pre_b = 0;
    auto load_ids = [&](int k) {                              // ids of tile lo + k (-1 past the end)
      const bool ok = k < mine;
      const uint32_t so = (uint32_t)(lo + k) * (kSub * 4u);
#pragma unroll
      for (int m = 0; m < kSubLoads; ++m)
        id_rows[m] = ok ? (int)__builtin_amdgcn_raw_buffer_load_b32(rs_slot, (srow + 8 * m) * 4, (int)so, 0) : -1;
      if (gtid < kSub) id_own = ok ? (int)__builtin_amdgcn_raw_buffer_load_b32(rs_slot, gtid * 4, (int)so, 0) : -1;
    };
    auto load_row = [&](int m) { pre[m] = sbuf_load4(rs_Z, id_rows[m], colA); };   // id -1 (padding, past the end): zeros
    auto load_row_scalars = [&]() {
      if (gtid < kSub) {
        const uint32_t eo = id_own >= 0 ? (uint32_t)id_own * 4u : kOOB;
        pre_a = __builtin_amdgcn_raw_buffer_load_b32(rs_idxA, (int)eo, 0, 0);
        pre_b = __builtin_amdgcn_raw_buffer_load_b32(rs_idxB, (int)eo, 0, 0);
        own_staged = id_own;
      }
    };
    auto stage_row = [&](int buf, int m) {                    // registers -> the three planes of the z image
      uint2 ph, pm, pl;
      split_pair(pre[m].x, pre[m].y, ph.x, pm.x, pl.x);
      split_pair(pre[m].z, pre[m].w, ph.y, pm.y, pl.y);
      uint32_t *q = zimg + buf * kMlpTile + (srow + 8 * m) * kMlpStride + (gtid & 31) * 2;
      *reinterpret_cast<uint2 *>(q) = ph;
      *reinterpret_cast<uint2 *>(q + kMlpPlane) = pm;
      *reinterpret_cast<uint2 *>(q + 2 * kMlpPlane) = pl;
    };
    auto stage_scalars = [&](int par) {                       // per-row indices of the staged tile (threads < 32)
      if (gtid < kSub) {
        const bool ok = own_staged >= 0;
        rowA[par * kSub + gtid] = ok ? pre_a : kNone;         // the two gathered nodes
        rowB[par * kSub + gtid] = ok ? pre_b : kNone;
        rowC[par * kSub + gtid] = ok ? (uint32_t)own_staged : kNone;
      }
    };
    float4 g0[4], g1[4];
    auto fetch_operand = [&](int par, int k) {                // rows 8 k + lrow of the tile
      const int rr = 8 * k + lrow;
      g0[k] = sbuf_load4(rs_T, (int)rowA[par * kSub + rr], col4);
      g1[k] = sbuf_load4(rs_T, (int)rowB[par * kSub + rr], col4 + kRowBytes);
    };
    // One tile: the MFMAs of tile k (z image k & 1) with, in their shadow, the staging of tile k+1 into the other buffer, the row
    // requests of tile k+2 and the id requests of tile k+3 (typed_body's order).
    auto tile_step = [&](int k, int par) {
      const int buf = k & 1, nxt = (par + 1) & (kMlpRing - 1);
      x6_tile(zimg + buf * kMlpTile, [&](int i) {
        if (i < 4) {}                                         // (the epilogue operands: requested by the previous tile's epilogue)
        else if (i < 8) stage_row(buf ^ 1, i - 4);
        else if (i == 8) stage_scalars(nxt);
        else if (i < 13) load_row(i - 9);
        else if (i == 13) load_row_scalars();
        else if (i == 14) load_ids(k + 3);
      });
    };
    auto epilogue = [&](int k, int par) {
      uint32_t *const img = himg + (k & 1) * kMlpTile;
      const int nxt = (par + 1) & (kMlpRing - 1);
      acc_to_scr(scr, acc, h, li);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = 8 * q + lrow;
        float4 v = *reinterpret_cast<const float4 *>(&scr[rr * kScrStride + (lane & 7) * 4]);
        v.x = act_fwd((v.x + (g0[q].x - g1[q].x)) + bias4.x, slope);
        v.y = act_fwd((v.y + (g0[q].y - g1[q].y)) + bias4.y, slope);
        v.z = act_fwd((v.z + (g0[q].z - g1[q].z)) + bias4.z, slope);
        v.w = act_fwd((v.w + (g0[q].w - g1[q].w)) + bias4.w, slope);
        const uint32_t rc = rowC[par * kSub + rr];
        sbuf_store4(v, rs_H1, (int)rc, col4);                 // padding rows: dropped
        // ... and the same values as pieces into the H1 image (a padding row: zeros, as a row staged from memory would be)
        const bool pad = rc == kNone;
        uint2 ph, pm, pl;
        split_pair(pad ? 0.f : v.x, pad ? 0.f : v.y, ph.x, pm.x, pl.x);
        split_pair(pad ? 0.f : v.z, pad ? 0.f : v.w, ph.y, pm.y, pl.y);
        uint32_t *w = img + rr * kMlpStride + (c4 >> 1);
        *reinterpret_cast<uint2 *>(w) = ph;
        *reinterpret_cast<uint2 *>(w + kMlpPlane) = pm;
        *reinterpret_cast<uint2 *>(w + 2 * kMlpPlane) = pl;
        // this chunk's operand registers are free: request the NEXT tile's rows into them (its indices were staged during
        // this tile's MFMA phase, before the barrier); past the last tile they are out of range: zeros
        fetch_operand(nxt, q);
      }
    };

    load_ids(0);
#pragma unroll
    for (int m = 0; m < kSubLoads; ++m) load_row(m);          // tile 0
    load_row_scalars();
    load_ids(1);
    // the first class's panel is requested HERE, behind tile 0's rows and ahead of the wait for them: the two round trips run side by side
    float c_have = p.tile_scale[lo];
    load_panel(c_have);
#pragma unroll
    for (int m = 0; m < kSubLoads; ++m) stage_row(0, m);
    stage_scalars(0);
#pragma unroll
    for (int m = 0; m < kSubLoads; ++m) load_row(m);          // tile 1
    load_row_scalars();
    load_ids(2);
    lds_barrier();                                            // (barrier "start")
#pragma unroll
    for (int c = 0; c < 4; ++c) fetch_operand(0, c);          // tile 0's epilogue operands (later tiles: by the epilogue before)
    // The class structure of the range, 64 tiles at a time: lane l keeps the coefficient of tile 64 c + l, bit l of `starts`
    // says "tile 64 c + l begins a new class" (typed_body).
    int k = 0, par = 0;
    float sv = 0.f;
    unsigned long long starts = 0;
    while (k < mine) {
      if ((k & 63) == 0) {
        const float last = __shfl(sv, 63);
        sv = k + lane < mine ? p.tile_scale[lo + k + lane] : 0.f;
        float up = __shfl_up(sv, 1);
        if (lane == 0) up = k > 0 ? last : sv;
        starts = __ballot(k + lane < mine && __float_as_uint(sv) != __float_as_uint(up));
      }
      const float c = __shfl(sv, k & 63);
      if (__float_as_uint(c) != __float_as_uint(c_have)) {     // (wave-uniform) the range crosses into the next class
        load_panel(c);
        c_have = c;
      }
      do {
        tile_step(k, par);
        lds_barrier();           // (barrier k) tile k+1 is staged for everyone, everyone is done with tile k's z rows
        epilogue(k, par);
        ++k;
        par = (par + 1) & (kMlpRing - 1);
      } while (k < mine && (k & 63) != 0 && ((starts >> (k & 63)) & 1ull) == 0);
    }
    lds_barrier();               // (barrier `mine`) the last tile's H1 image is complete
  } else {
    // ==================================================================== the second Linear (waves 4-7): mfma_typed<TEPI_OUT>
    __builtin_amdgcn_s_setprio(1);                            // the later-dispatched half loses every arbitration otherwise
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias2) bias4 = *reinterpret_cast<const float4 *>(p.bias2 + c4);
    const srsrc_t rs_R = make_srsrc(p.R, p.R ? p.ldr : (int64_t)kMlpH, p.E);        // (no residual: zero records)
    const srsrc_t rs_O = make_srsrc(p.out, p.ldo, p.E);
    {                                                         // the plain panel W2, 32 values per round trip
      const rsrc_t rs_W = make_rsrc(p.W2, (uint32_t)(kMlpH * p.ldw2 * 4));
      const uint32_t w_first = (uint32_t)(p.w2_transposed ? (int64_t)col * p.ldw2 + kMlpHalf * h : (int64_t)kMlpHalf * h * p.ldw2 + col) * 4u;
      const uint32_t w_step = __builtin_amdgcn_readfirstlane((int)(p.w2_transposed ? 4 : p.ldw2 * 4));
      load_panel_x6(B6, rs_W, w_first, w_step);
    }
    float4 g1[4];
    auto fetch_residual = [&](int par, int q) {               // rows 8 q + lrow of the tile (a padding row, no residual: zeros)
      g1[q] = sbuf_load4(rs_R, (int)rowC[par * kSub + 8 * q + lrow], col4);
    };
    lds_barrier();                                            // (barrier "start") tile 0's row indices are staged
#pragma unroll
    for (int q = 0; q < 4; ++q) fetch_residual(0, q);
    lds_barrier();                                            // (barrier 0)
    int par = 0;
    for (int k = 0; k < mine; ++k) {
      lds_barrier();                                          // (barrier k+1) tile k's H1 image is complete
      x6_tile(himg + (k & 1) * kMlpTile, [&](int) {});
      acc_to_scr(scr, acc, h, li);
      const int nxt = (par + 1) & (kMlpRing - 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = 8 * q + lrow;
        float4 v = *reinterpret_cast<const float4 *>(&scr[rr * kScrStride + (lane & 7) * 4]);
        v.x = (v.x + bias4.x) + g1[q].x; v.y = (v.y + bias4.y) + g1[q].y;
        v.z = (v.z + bias4.z) + g1[q].z; v.w = (v.w + bias4.w) + g1[q].w;
        sbuf_store4(v, rs_O, (int)rowC[par * kSub + rr], col4);                   // padding rows: dropped
        fetch_residual(nxt, q);                               // tile k+1's rows (its indices were staged before barrier k)
      }
      par = nxt;
    }
  }
}

inline bool edge_mlp_lds_ready() {
  static bool done[kMaxDevices] = {};
  return opt_in_lds(reinterpret_cast<const void *>(&edge_mlp_k), kEdgeMlpLdsBytes, done);
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_edge_mlp_fwd(const float *Z, int64_t ldz, const float *W, int64_t ldw, const float *P, int64_t ldp, int64_t num_nodes,
                     const float *bias1, const int32_t *selA, const int32_t *selB, const float *W2, int64_t ldw2, int w2_in_out,
                     const float *bias2, const float *R, int64_t ldr, const int32_t *slot_edge, const float *tile_scale,
                     const int32_t *num_tiles, int64_t tiles_bound, int64_t E, int H, float slope, float *H1, int64_t ldh,
                     float *out, int64_t ldo, void *stream) {
  if (H != 128 || g_exact_fp32) return DMP_ERR_UNSUPPORTED;
  if (E < 0 || num_nodes < 0 || tiles_bound < 0) return DMP_ERR_BAD_ARG;
  if (!slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (E == 0 || tiles_bound == 0) return DMP_OK;
  if (!Z || !W || !P || !selA || !selB || !W2 || !slot_edge || !tile_scale || !num_tiles || !H1 || !out || ldz < H || ldw < 2 * H ||
      ldp < 2 * H || ldw2 < H || ldh < H || ldo < H || (R && ldr < H))
    return DMP_ERR_BAD_ARG;
  if (ldz % 4 || ldh % 4 || ldp % 4 || ldo % 4 || (R && ldr % 4) || !aligned16(Z) || !aligned16(H1) || !aligned16(P) || !aligned16(out) ||
      (R && !aligned16(R)) || (bias1 && !aligned16(bias1)) || (bias2 && !aligned16(bias2)))
    return DMP_ERR_UNSUPPORTED;
  const int64_t lim32 = ((int64_t)1 << 32) - 8192;
  if (!stride_ok(ldz) || !stride_ok(ldh) || !stride_ok(ldp) || !stride_ok(ldo) || (R && !stride_ok(ldr)) || E >= ((int64_t)1 << 30) ||
      num_nodes >= ((int64_t)1 << 31) || tiles_bound * kSub * 4 >= lim32 || (int64_t)H * ldw * 4 >= lim32 || (int64_t)H * ldw2 * 4 >= lim32 ||
      !fits4g(E, ldz) || !fits4g(E, ldh) || !fits4g(E, ldo) || (R && !fits4g(E, ldr)) || !fits4g(num_nodes, ldp))
    return DMP_ERR_UNSUPPORTED;                               // (arrays of 4 GiB and more: the two launches have the 64-bit row kernels)
  if (!edge_mlp_lds_ready()) return DMP_ERR_HIP;
  EdgeMlpArgs a{};
  a.Z = Z; a.ldz = ldz; a.W = W; a.ldw = ldw; a.P = P; a.ldp = ldp; a.num_nodes = num_nodes; a.bias1 = bias1; a.selA = selA; a.selB = selB;
  a.W2 = W2; a.ldw2 = ldw2; a.w2_transposed = w2_in_out ? 0 : 1; a.bias2 = bias2; a.R = R; a.ldr = R ? ldr : H;
  a.H1 = H1; a.ldh = ldh; a.out = out; a.ldo = ldo; a.E = E; a.slot_edge = slot_edge; a.tile_scale = tile_scale; a.num_tiles = num_tiles;
  a.slope = slope;
  edge_mlp_k<<<one_per_cu_blocks(tiles_bound), kMlpThreads, kEdgeMlpLdsBytes, (hipStream_t)stream>>>(a);
  return check_launch();
}

}  // extern "C"
