// The FIRST layer's edge MLP forward from the label codes as ONE launch (gfx950, H = 128, bf16x6):
//
//   H1[e]  = act(enc[e] MA + coef_e[e] (enc[e] MB) + P[a_e, 0:H] - P[b_e, H:2H] + be)     (what dmp_l0_edge_fwd_rows / _masked make)
//   out[e] = (e < r_rows ? R[e] : 0) + (H1[e] W2 + (e >= code_row0 ? codes[e] Wc : 0) + b2)   (what dmp_out_fwd_typed_codes makes)
//
// As launches of their own the [Ek, H] activation H1 is written by the first and read back by the second, and the code rows are
// fetched by both.  Here a 512-thread workgroup (one per CU, persistent over a contiguous range of the tile list) splits its
// eight waves into two ROLES around one LDS image of H1, as edge_mlp_k (csrc/dmp_edgemlp.hip) does for the inner layers:
//
//   waves 0-3 ("first")   the K-column product on the matrix pipe: a tile's operand rows are [enc | coef_e enc] laid out in four
//                         slots of kSlot columns -- (table 0, enc) (table 1, enc) (table 0, coef enc) (table 1, coef enc), a row
//                         filling the two slots of ITS embedding table (rows below row_split: table 0) and zeros in the others --
//                         against the stacked matrices [MA_0; MA_1; MB_0; MB_1] (registers, one panel for the launch): three
//                         16-deep k-groups of six piece MFMAs.  The tile list is in ascending row order, so the rows of a tile have
//                         different coefficients: the coefficient scales the operand row, not a class panel.  Epilogue
//                         act((acc + (P[a] - P[b])) + be); the row goes to H1 by edge id (the backward needs it saved) AND, split
//                         into pieces, into a double-buffered image;
//   waves 4-7 ("second")  typed_body<TEPI_OUT, 128, true, false, CODES> one tile behind, its operand tile being that image and its
//                         code rows the 16-wide piece image the first role staged from the SAME load (rows below code_row0: zeros):
//                         the same piece products in the same order, the same epilogue order -- out is bit-identical to
//                         dmp_out_fwd_typed_codes' on every kept row.
//
// One barrier per tile (LDS traffic only).  Tile k's operand image is written between barriers k-2 and k-1 and read between k-1 and k
// (two buffers); its H1 image is written between k and k+1 and read between k+1 and k+2 (two buffers); its row indices and its
// 16-wide code image are written between k-2 and k-1 and last read between k+1 and k+2, while tile k+3's are written: rings of four.
#include <type_traits>

#include "dmp_x6_tile.h"

namespace dmp {
namespace {

struct L0MlpArgs {
  const float *enc; int64_t lde; int K;             // packed label codes [E, lde >= K], columns >= K may hold anything
  const float *M; int64_t ldm; int tables;          // [tables * K, >= 256] = W_t [A | B] per embedding table
  int64_t row_split;                                // rows below it: table 0; the others: table 1 (one table: E)
  const float *P; int64_t ldp; int64_t num_nodes;   // gathered table [N, >= 256]
  const float *bias1;                               // [128] or NULL
  const float *coef_e;                              // [E] the row's coefficient
  const int32_t *selA, *selB;                       // [E] node ids of the added / subtracted P rows (-1: none)
  const float *W2; int64_t ldw2; int w2_transposed; // 0: B[k][j] = W2[k][j] ([in, out]); 1: B[k][j] = W2[j][k] (nn.Linear's [out, in])
  const float *bias2;                               // [128] or NULL
  const float *Wc; int64_t ldwc; int64_t code_row0; // [K, >= 128]: rows >= code_row0 take + enc[e, 0:K] Wc
  const float *R; int64_t ldr; int64_t r_rows;      // residual rows [r_rows, 128] (rows beyond: zeros) or NULL
  float *H1; int64_t ldh;                           // saved activation rows [E, 128], scattered by edge id
  float *out; int64_t ldo;                          // output rows [E, 128], scattered by edge id
  int64_t E;
  const int32_t *slot_edge;                         // [tiles * 32] edge id per slot, -1 = padding
  const int32_t *num_tiles;                         // device scalar: tiles in use
  float slope;
};

// (the workgroup's geometry and the H1 image's -- kMlpThreads, kMlpStride / kMlpPlane / kMlpTile, kMlpRing -- are dmp_x6_tile.h's, shared with edge_mlp_k)
constexpr int kSlot = 12;                           // code columns per operand slot: K <= kSlot
constexpr int kOpGroups = 4 * kSlot / 16;           // 16-deep k-groups of the first role's product (3)
constexpr int kOpStride = (4 * kSlot + 8) / 2;      // dwords per operand row: 48 bf16 + 8 of padding (28: rows of whole 16-byte pieces)
constexpr int kOpPlane = kSub * kOpStride;
constexpr int kOpTile = 3 * kOpPlane;               // 10752 bytes
constexpr int kCxPlane = kSub * 8;                  // the second role's code rows: 16 bf16 per row and plane
constexpr int kCxTile = 3 * kCxPlane;               // 3072 bytes
constexpr int kOpOff = 2 * kMlpTile * 4;            // behind the H1 image's two buffers
constexpr int kCxOff = kOpOff + 2 * kOpTile * 4;
constexpr int kScrOffL = kCxOff + kMlpRing * kCxTile * 4;
constexpr int kRowsOffL = kScrOffL + 8 * 32 * kScrStride * 4;
constexpr int kL0MlpLdsBytes = kRowsOffL + 3 * kMlpRing * kSub * 4;   // 52224 + 21504 + 12288 + 36864 + 1536 = 124416
static_assert(4 * kSlot % 16 == 0 && kOpStride % 4 == 0, "whole k-groups, 16-byte fragment reads");

__global__ __launch_bounds__(kMlpThreads, 1) void l0_edge_mlp_k(const L0MlpArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint32_t *const himg = reinterpret_cast<uint32_t *>(lds);
  uint32_t *const opimg = reinterpret_cast<uint32_t *>(lds + kOpOff);
  uint32_t *const cximg = reinterpret_cast<uint32_t *>(lds + kCxOff);
  uint32_t *const rowA = reinterpret_cast<uint32_t *>(lds + kRowsOffL);           // [kMlpRing][32] each: row INDICES (-1: none)
  uint32_t *const rowB = rowA + kMlpRing * kSub, *const rowC = rowB + kMlpRing * kSub;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool second = wave >= 4;
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5, cs = wave & 3;
  const int gtid = threadIdx.x & 255;                                             // thread of its role
  const int col = 32 * cs + li;
  float *const scr = reinterpret_cast<float *>(lds + kScrOffL) + wave * (32 * kScrStride);
  const int lrow = lane >> 3, c4 = 32 * cs + (lane & 7) * 4;
  const uint32_t col4 = (uint32_t)c4 * 4u;
  constexpr uint32_t kRowBytes = kMlpH * 4u;
  constexpr uint32_t kNone = 0xFFFFFFFFu, kOOB = 0xFFFFF000u;

  // this workgroup's contiguous tile range
  const int ntiles = __builtin_amdgcn_readfirstlane(*p.num_tiles);
  const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = (int)blockIdx.x * chunk;
  const int hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  const int mine = hi > lo ? hi - lo : 0;
  if (mine == 0) return;                                                          // (uniform per workgroup: before any barrier)

  Split8 B6[kMlpGroups];                    // the role's panel as bf16 pieces (the first role: kOpGroups fragments of it)
  f32x16 acc;
  // A tile's product on the bf16 pipe: per 16-deep k-group g six MFMAs on the three piece fragments of image row li (this lane's 8
  // consecutive k: `first` + `step` g dwords into the row, one ds_read_b128 per plane, requested one group ahead) and B6[g].
  auto x6_tile = [&](const uint32_t *ar, int plane, int step, auto groups) {
    constexpr int G = decltype(groups)::value;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    Frag8 ah, am, al;
    ah.v = *reinterpret_cast<const bf16x8 *>(ar);
    am.v = *reinterpret_cast<const bf16x8 *>(ar + plane);
    al.v = *reinterpret_cast<const bf16x8 *>(ar + 2 * plane);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      Frag8 nh = ah, nm = am, nl = al;
      if (g + 1 < G) {
        nh.v = *reinterpret_cast<const bf16x8 *>(ar + step * (g + 1));
        nm.v = *reinterpret_cast<const bf16x8 *>(ar + plane + step * (g + 1));
        nl.v = *reinterpret_cast<const bf16x8 *>(ar + 2 * plane + step * (g + 1));
      }
      __builtin_amdgcn_sched_barrier(0);
      acc = mfma_x6(ah, am, al, B6[g], acc);
      __builtin_amdgcn_sched_barrier(0);
      ah = nh; am = nm; al = nl;
    }
  };

  if (!second) {
    // ==================================================================== the K-column product (waves 0-3)
    const float4 bias4 = buf_load4(make_rsrc(p.bias1, p.bias1 ? kRowBytes : 0u), col4, 0);   // (no bias: zero records -> zeros, no branch)
    const float slope = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.slope)));
    const uint32_t rows4 = (uint32_t)(p.E * 4);
    const srsrc_t rs_enc = make_srsrc(p.enc, p.lde, p.E);
    const srsrc_t rs_H1 = make_srsrc(p.H1, p.ldh, p.E);
    const srsrc_t rs_T = make_srsrc(p.P, p.ldp, p.num_nodes);
    const rsrc_t rs_idxA = make_rsrc(p.selA, rows4);
    const rsrc_t rs_idxB = make_rsrc(p.selB, rows4);
    const rsrc_t rs_coef = make_rsrc(p.coef_e, rows4);
    const rsrc_t rs_slot = make_rsrc(p.slot_edge, (uint32_t)ntiles * (kSub * 4u));   // (its check covers the vector offset only: load_ids)
    // threads < 128 stage the code rows: codes 4 cq .. 4 cq + 3 of row crow (cq 3: beyond the kSlot columns, zeros); threads < 32 the
    // row's indices.  Every thread issues the same loads -- the others' at an offset beyond the descriptor: no memory access, no branch
    const int cq = gtid & 3, crow = (gtid >> 2) & (kSub - 1);
    const bool stager = gtid < 4 * kSub, owner = gtid < kSub;
    const bool cload = stager && 4 * cq < kSlot && 4 * cq < (int)p.lde;
    const uint32_t slot_c = stager ? (uint32_t)crow * 4u : kOOB, slot_o = owner ? (uint32_t)gtid * 4u : kOOB;
    const int K = __builtin_amdgcn_readfirstlane(p.K);

    auto load_panel = [&]() {              // fragment g: rows 16 g + 8 h .. + 7 of the stacked matrices [MA_0; MA_1; MB_0; MB_1], column col
      const rsrc_t rs_M = make_rsrc(p.M, (uint32_t)((int64_t)p.tables * K * p.ldm * 4));
      float w[kOpGroups][8];
#pragma unroll
      for (int g = 0; g < kOpGroups; ++g) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = 16 * g + 8 * h + j, s = k / kSlot, jj = k - s * kSlot, t = s & 1, half = s >> 1;
          const bool ok = jj < K && t < p.tables;                                  // (a slot's columns >= K, a table not there: zeros)
          const uint32_t off = ok ? (uint32_t)(((int64_t)(t * K + jj) * p.ldm + half * kMlpH + col) * 4) : kOOB;
          w[g][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_M, (int)off, 0, 0));
        }
      }
#pragma unroll
      for (int g = 0; g < kOpGroups; ++g)
        split8(make_float4(w[g][0], w[g][1], w[g][2], w[g][3]), make_float4(w[g][4], w[g][5], w[g][6], w[g][7]), B6[g]);
    };

    // ---- prefetch: ids of tile k+3, code rows and indices of tile k+2 in registers, tile k+1 staged while tile k is computed
    int id_c = -1, id_own = -1;             // the ids most recently requested: of row crow / of row gtid (-1: none)
    int id_data = -1, own_staged = -1;      // ... and those the registers below belong to
    float4 pre_c = make_float4(0.f, 0.f, 0.f, 0.f);
    float pre_cf = 0.f;
    uint32_t pre_a = 0, pre_b = 0;
    int raw_c = -1, raw_own = -1;           // as loaded, before load_data takes them
    bool ids_ok = false;
    auto load_ids = [&](int k) {                              // ids of tile lo + k
      // The tile's offset travels in the scalar operand, which the descriptor's range check does NOT cover: past this workgroup's
      // range the load is CLAMPED to its last tile (mine >= 1: in range) and load_data throws the value away.  The -1 of a tile past
      // the end and of the threads that stage nothing is selected THERE, a tile later: selected here, the compiler sinks the two loads
      // under `ok` -- a wave-uniform branch with a wait for every load in flight behind it, once per tile.
      ids_ok = k < mine;
      const uint32_t so = (uint32_t)(lo + (ids_ok ? k : mine - 1)) * (kSub * 4u);
      raw_c = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_slot, (int)slot_c, (int)so, 0);
      raw_own = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_slot, (int)slot_o, (int)so, 0);
    };
    auto load_data = [&]() {                                  // of the tile whose ids were requested last
      id_c = (ids_ok && stager) ? raw_c : -1;
      id_own = (ids_ok && owner) ? raw_own : -1;
      pre_c = sbuf_load4(rs_enc, cload ? id_c : -1, (uint32_t)cq * 16u);           // id -1 (padding, past the end): zeros
      pre_cf = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_coef, (int)(id_c >= 0 ? (uint32_t)id_c * 4u : kOOB), 0, 0));
      const uint32_t eo = id_own >= 0 ? (uint32_t)id_own * 4u : kOOB;
      pre_a = __builtin_amdgcn_raw_buffer_load_b32(rs_idxA, (int)eo, 0, 0);
      pre_b = __builtin_amdgcn_raw_buffer_load_b32(rs_idxB, (int)eo, 0, 0);
      id_data = id_c;
      own_staged = id_own;
    };
    auto stage = [&](int buf, int par) {                      // registers -> the operand image, the 16-wide code image, the row indices
      if (stager) {
        const int kc = K - 4 * cq;                            // (a row's padding columns may hold anything: zeros from here on)
        const float x0 = kc > 0 ? pre_c.x : 0.f, x1 = kc > 1 ? pre_c.y : 0.f, x2 = kc > 2 ? pre_c.z : 0.f, x3 = kc > 3 ? pre_c.w : 0.f;
        uint2 xh, xm, xl, yh, ym, yl;
        split_pair(x0, x1, xh.x, xm.x, xl.x);
        split_pair(x2, x3, xh.y, xm.y, xl.y);
        split_pair(pre_cf * x0, pre_cf * x1, yh.x, ym.x, yl.x);
        split_pair(pre_cf * x2, pre_cf * x3, yh.y, ym.y, yl.y);
        const uint2 zero = make_uint2(0u, 0u);
        const bool t1 = (int64_t)id_data >= p.row_split;      // the row's embedding table
        if (4 * cq < kSlot) {
          uint32_t *q = opimg + buf * kOpTile + crow * kOpStride + 2 * cq;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const bool mineslot = ((s & 1) != 0) == t1;
            const uint2 vh = (s >> 1) ? yh : xh, vm = (s >> 1) ? ym : xm, vl = (s >> 1) ? yl : xl;
            *reinterpret_cast<uint2 *>(q + (kSlot / 2) * s) = mineslot ? vh : zero;
            *reinterpret_cast<uint2 *>(q + (kSlot / 2) * s + kOpPlane) = mineslot ? vm : zero;
            *reinterpret_cast<uint2 *>(q + (kSlot / 2) * s + 2 * kOpPlane) = mineslot ? vl : zero;
          }
        }
        const bool cz = (int64_t)id_data >= p.code_row0;      // (id -1: its codes are zeros already)
        uint32_t *c = cximg + par * kCxTile + crow * 8 + 2 * cq;
        *reinterpret_cast<uint2 *>(c) = cz ? xh : zero;
        *reinterpret_cast<uint2 *>(c + kCxPlane) = cz ? xm : zero;
        *reinterpret_cast<uint2 *>(c + 2 * kCxPlane) = cz ? xl : zero;
      }
      if (owner) {
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
    load_data();                                              // tile 0
    load_ids(1);
    load_panel();                                             // behind tile 0's loads and ahead of the wait for them: one round trip
    stage(0, 0);
    load_data();                                              // tile 1
    load_ids(2);
    lds_barrier();                                            // (barrier "start")
#pragma unroll
    for (int c = 0; c < 4; ++c) fetch_operand(0, c);          // tile 0's epilogue operands (later tiles: by the epilogue before)
    for (int k = 0; k < mine; ++k) {
      const int par = k & (kMlpRing - 1);
      stage((k + 1) & 1, (par + 1) & (kMlpRing - 1));           // tile k+1 (past the end: zeros, no rows)
      load_data();                                            // tile k+2
      load_ids(k + 3);
      x6_tile(opimg + (k & 1) * kOpTile + li * kOpStride + 4 * h, kOpPlane, 8, std::integral_constant<int, kOpGroups>());
      lds_barrier();             // (barrier k) tile k+1 is staged for everyone, everyone is done with tile k's operand rows
      epilogue(k, par);
    }
    lds_barrier();               // (barrier `mine`) the last tile's H1 image is complete
  } else {
    // ==================================================================== the second Linear (waves 4-7): mfma_typed_codes
    __builtin_amdgcn_s_setprio(1);                            // the later-dispatched half loses every arbitration otherwise
    const float4 bias4 = buf_load4(make_rsrc(p.bias2, p.bias2 ? kRowBytes : 0u), col4, 0);   // (no bias: zero records -> zeros, no branch)
    const srsrc_t rs_R = make_srsrc(p.R, p.R ? p.ldr : (int64_t)kMlpH, p.r_rows);   // (no residual, rows >= r_rows: zero records)
    const srsrc_t rs_O = make_srsrc(p.out, p.ldo, p.E);
    Split8 BX;                                                // the codes k-group's panel fragment: BX[j] = Wc[8 h + j][col]
    {
      const rsrc_t rs_Wc = make_rsrc(p.Wc, (uint32_t)((int64_t)p.K * p.ldwc * 4));   // (rows >= K: beyond the range -> zeros)
      float w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        w[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_Wc, (int)(((int64_t)(8 * h + j) * p.ldwc + col) * 4), 0, 0));
      // the plain panel W2, 32 values per round trip
      const rsrc_t rs_W = make_rsrc(p.W2, (uint32_t)(kMlpH * p.ldw2 * 4));
      const uint32_t w_first = (uint32_t)(p.w2_transposed ? (int64_t)col * p.ldw2 + kMlpHalf * h : (int64_t)kMlpHalf * h * p.ldw2 + col) * 4u;
      const uint32_t w_step = __builtin_amdgcn_readfirstlane((int)(p.w2_transposed ? 4 : p.ldw2 * 4));
      load_panel_x6(B6, rs_W, w_first, w_step, [&] { split8(make_float4(w[0], w[1], w[2], w[3]), make_float4(w[4], w[5], w[6], w[7]), BX); });
    }
    float4 g1[4];
    auto fetch_residual = [&](int par, int q) {               // rows 8 q + lrow of the tile (padding, rows >= r_rows, no residual: zeros)
      g1[q] = sbuf_load4(rs_R, (int)rowC[par * kSub + 8 * q + lrow], col4);
    };
    lds_barrier();                                            // (barrier "start") tile 0's row indices are staged
#pragma unroll
    for (int q = 0; q < 4; ++q) fetch_residual(0, q);
    lds_barrier();                                            // (barrier 0)
    for (int k = 0; k < mine; ++k) {
      const int par = k & (kMlpRing - 1), nxt = (par + 1) & (kMlpRing - 1);
      lds_barrier();                                          // (barrier k+1) tile k's H1 image is complete
      x6_tile(himg + (k & 1) * kMlpTile + li * kMlpStride + (kMlpHalf / 2) * h, kMlpPlane, 4, std::integral_constant<int, kMlpGroups>());
      {                                                       // + codes Wc: one more 16-deep k-group (this lane: codes 8 h .. 8 h + 7 of row li)
        const uint32_t *c = cximg + par * kCxTile + li * 8 + 4 * h;
        Frag8 ch, cm, cl;
        ch.v = *reinterpret_cast<const bf16x8 *>(c);
        cm.v = *reinterpret_cast<const bf16x8 *>(c + kCxPlane);
        cl.v = *reinterpret_cast<const bf16x8 *>(c + 2 * kCxPlane);
        acc = mfma_x6(ch, cm, cl, BX, acc);
      }
      acc_to_scr(scr, acc, h, li);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = 8 * q + lrow;
        float4 v = *reinterpret_cast<const float4 *>(&scr[rr * kScrStride + (lane & 7) * 4]);
        v.x = (v.x + bias4.x) + g1[q].x; v.y = (v.y + bias4.y) + g1[q].y;
        v.z = (v.z + bias4.z) + g1[q].z; v.w = (v.w + bias4.w) + g1[q].w;
        sbuf_store4(v, rs_O, (int)rowC[par * kSub + rr], col4);                   // padding rows: dropped
        fetch_residual(nxt, q);                               // tile k+1's rows (its indices were staged before barrier k)
      }
    }
  }
}

inline bool l0_mlp_lds_ready() {
  static bool done[kMaxDevices] = {};
  return opt_in_lds(reinterpret_cast<const void *>(&l0_edge_mlp_k), kL0MlpLdsBytes, done);
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_l0_edge_mlp_max_codes(void) { return kSlot; }

int dmp_l0_edge_mlp_fwd(const float *enc, int64_t lde, int K, const float *M, int64_t ldm, int tables, int64_t row_split, const float *P,
                        int64_t ldp, int64_t num_nodes, const float *bias1, const float *coef_e, const int32_t *selA, const int32_t *selB,
                        float slope, const float *W2, int64_t ldw2, int w2_in_out, const float *bias2, const float *Wc, int64_t ldwc,
                        int64_t code_row0, const float *R, int64_t ldr, int64_t r_rows, const int32_t *slot_edge, const int32_t *num_tiles,
                        int64_t tiles_bound, int64_t E, int H, float *H1, int64_t ldh, float *out, int64_t ldo, void *stream) {
  if (H != 128 || g_exact_fp32) return DMP_ERR_UNSUPPORTED;
  if (E < 0 || num_nodes < 0 || tiles_bound < 0 || K < 1 || tables < 1 || row_split < 0 || code_row0 < 0 || code_row0 > E || r_rows < 0 || r_rows > E)
    return DMP_ERR_BAD_ARG;
  if (K > kSlot || tables > 2 || !slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (E == 0 || tiles_bound == 0) return DMP_OK;
  if (!enc || !M || !P || !coef_e || !selA || !selB || !W2 || !Wc || !slot_edge || !num_tiles || !H1 || !out || lde < K || ldm < 2 * H ||
      ldp < 2 * H || ldw2 < H || ldwc < H || ldh < H || ldo < H || (R && ldr < H))
    return DMP_ERR_BAD_ARG;
  if (lde % 4 || ldh % 4 || ldp % 4 || ldo % 4 || (R && ldr % 4) || !aligned16(enc) || !aligned16(H1) || !aligned16(P) || !aligned16(out) ||
      (R && !aligned16(R)) || (bias1 && !aligned16(bias1)) || (bias2 && !aligned16(bias2)))
    return DMP_ERR_UNSUPPORTED;
  const int64_t lim32 = ((int64_t)1 << 32) - 8192;
  if (!stride_ok(lde) || !stride_ok(ldh) || !stride_ok(ldp) || !stride_ok(ldo) || (R && !stride_ok(ldr)) || E >= ((int64_t)1 << 30) ||
      num_nodes >= ((int64_t)1 << 31) || tiles_bound * kSub * 4 >= lim32 || (int64_t)tables * K * ldm * 4 >= lim32 ||
      (int64_t)H * ldw2 * 4 >= lim32 || (int64_t)K * ldwc * 4 >= lim32 || !fits4g(E, lde) || !fits4g(E, ldh) || !fits4g(E, ldo) ||
      (R && !fits4g(r_rows, ldr)) || !fits4g(num_nodes, ldp))
    return DMP_ERR_UNSUPPORTED;                               // (arrays of 4 GiB and more: the launches of their own)
  if (!l0_mlp_lds_ready()) return DMP_ERR_HIP;
  L0MlpArgs a{};
  a.enc = enc; a.lde = lde; a.K = K; a.M = M; a.ldm = ldm; a.tables = tables; a.row_split = tables == 1 ? E : row_split;
  a.P = P; a.ldp = ldp; a.num_nodes = num_nodes; a.bias1 = bias1; a.coef_e = coef_e; a.selA = selA; a.selB = selB;
  a.W2 = W2; a.ldw2 = ldw2; a.w2_transposed = w2_in_out ? 0 : 1; a.bias2 = bias2; a.Wc = Wc; a.ldwc = ldwc; a.code_row0 = code_row0;
  a.R = R; a.ldr = R ? ldr : H; a.r_rows = R ? r_rows : 0; a.H1 = H1; a.ldh = ldh; a.out = out; a.ldo = ldo; a.E = E;
  a.slot_edge = slot_edge; a.num_tiles = num_tiles; a.slope = slope;
  l0_edge_mlp_k<<<one_per_cu_blocks(tiles_bound), kMlpThreads, kL0MlpLdsBytes, (hipStream_t)stream>>>(a);
  return check_launch();
}

}  // extern "C"
