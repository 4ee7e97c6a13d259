// The FIRST layer's NODE side from the label codes on the matrix pipe, ONE launch for every embedding table (gfx950, H = 128,
// bf16x6):
//
//   H1n[r]             = act([venc[r] | S0_in[r] | S0_out[r]] W_t[:, 0:H] + bn)
//   [P_dst | P_src][r] = [venc[r] | S0_in[r] | S0_out[r]] W_t[:, H:3H]
//
// for every KEPT node row r, t = the row's table (rows below row_split: table 0, as l0_edge_mlp_k takes its edge rows).  What
// dmp_l0_node_fwd (csrc/dmp_layer0.hip) makes with a v_readlane and a packed FMA per 128 outputs and code column, one launch per
// table, is here a [32, 48] x [48, 384] product per tile: the tile's code rows are split into bf16 pieces once by the staging
// threads, the packed matrix is three 16-deep k-groups -- [venc | S0_in | S0_out], each padded with zero rows to sixteen -- held as
// piece fragments in registers.  W_t's rows of S0 are zero outside the first H columns (the packing of dmp_l0_node_fwd), so the two
// projection blocks take the venc k-group alone: five fragments per table and wave, thirty piece MFMAs per tile and table.
//
// A 256-thread workgroup walks a contiguous range of the 32-row tiles of the kept nodes' list (dmp_kept_rows over ALL nodes,
// ascending; no list: the rows 0 .. N-1); wave cs owns the columns 32 cs .. 32 cs + 31 of each of the three H-wide output blocks.
// The list is ascending, so at most ONE tile holds rows of both tables: a wave masks its A fragments by the lane's row's table (a
// lane of an A fragment is a row) and runs the product of a table only where the tile has a row of it (wave-uniform, around MFMAs
// only).  The codes are small integers times a 0 / 1 gate, so up to magnitude 256 their mid and lo pieces are zeros; the kernel does
// NOT rely on it -- all six piece products run (they are ~2 % of the launch: it is bound by its stores).
//
// A dead node's H1n row stays unwritten; its P rows are written as ZEROS (the first layer's edge kernel gathers P through the plain
// selectors) by the workgroups past the tile range, from the row mask, as l0_node_fwd_k's fourth block row does.
//
// One barrier per tile (LDS traffic only): tile k's image and row ids are written before barrier k into buffer k & 1 and read after
// it; tile k+2's are written after barrier k+1, which every wave passes after its last read of tile k.  Loads: the ids of tile k+2
// and the code rows of tile k+1 are requested BEFORE tile k's stores (gfx9 counts loads and stores in one in-order counter), every
// load is issued by every thread at a clamped or out-of-range index and its result selected afterwards (no wave-uniform condition
// and no run-time column count around a load).
#include "dmp_mfma_common.h"

namespace dmp {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
__device__ i32x2 llvm_struct_buffer_load_v2i32(i32x4 rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.v2i32");
namespace {

struct L0NodeArgs {
  const float *venc; int64_t ldv; int VK;           // node codes [N, ldv], VK <= 16 in use (columns beyond: anything)
  const float *S0; int64_t lds; int K0, Kp;         // code sums [N, lds >= 2 Kp]: in-sums at column 0, out-sums at column Kp, K0 <= 16 each
  const float *W; int64_t ldw, wstride; int tables; // packed matrices [tables][VK + 2 K0 rows, ldw >= 384], `wstride` floats apart
  int64_t row_split;                                // rows below it: table 0, the others: table 1
  const float *bias; float slope;
  const uint32_t *rowmask;                          // bit r & 31 of word r >> 5: node r is kept; NULL: every node
  const int32_t *list, *count; int64_t list_bound;  // the kept nodes ascending, *count of them (NULL: rows 0 .. N-1)
  int64_t prefix;                                   // the list's first `prefix` entries are 0 .. prefix-1
  int64_t N;
  float *h1; int64_t ldh; float *P; int64_t ldp;
  int tile_blocks;                                  // workgroups 0 .. tile_blocks-1 walk tiles, the others zero the dead rows of P
};

constexpr int kHN = 128;
constexpr int kNGroups = 3;                         // k-groups: venc | S0_in | S0_out
constexpr int kNStride = (16 * kNGroups + 8) / 2;   // dwords per image row: 48 bf16 + 8 of padding (28: rows of whole 16-byte pieces)
constexpr int kNPlane = kSub * kNStride;
constexpr int kNTile = 3 * kNPlane;                 // hi | mid | lo: 10752 bytes
constexpr int kNScr = 32 * kScrStride;              // floats of a wave's accumulator scratch
constexpr uint32_t kOOBN = 0xFFFFF000u;
static_assert(kNStride % 4 == 0, "16-byte fragment reads");

__global__ __launch_bounds__(kGroupThreads, 2) void l0_node_mfma_k(const L0NodeArgs p) {
  __shared__ __attribute__((aligned(16))) uint32_t img[2 * kNTile];
  __shared__ __attribute__((aligned(16))) float scr_all[4 * kNScr];
  __shared__ int rowid[2 * kSub];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  if ((int)blockIdx.x >= p.tile_blocks) {
    // ---- a dead node's projections: zeros.  A wave per mask word: one load, then stores only
    if (!p.rowmask) return;
    const int nz = (int)gridDim.x - p.tile_blocks;
    const int64_t words = (p.N + 31) >> 5;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t wi = (int64_t)((int)blockIdx.x - p.tile_blocks) * 4 + wave; wi < words; wi += (int64_t)nz * 4) {
      uint32_t deadbits = ~p.rowmask[wi];
      deadbits = __builtin_amdgcn_readfirstlane(deadbits);
      while (deadbits) {
        const int b = __builtin_ctz(deadbits);
        deadbits &= deadbits - 1;
        const int64_t r = wi * 32 + b;
        if (r >= p.N) break;                                                       // (bits ascend: the rest lie past the end too)
        *reinterpret_cast<float4 *>(p.P + r * p.ldp + 4 * lane) = zero;            // 64 lanes x 4 = 2 H columns
      }
    }
    return;
  }
  const int cs = wave, col = 32 * cs + li;
  float *const scr = scr_all + wave * kNScr;
  const int lrow = lane >> 3, c4 = 32 * cs + (lane & 7) * 4;
  const uint32_t col4 = (uint32_t)c4 * 4u;
  constexpr uint32_t kRowBytes = kHN * 4u;

  // this workgroup's contiguous tile range
  const int cnt = __builtin_amdgcn_readfirstlane(p.count ? *p.count : (int)p.N);
  const int ntiles = (cnt + kSub - 1) / kSub;
  const int chunk = (ntiles + p.tile_blocks - 1) / p.tile_blocks;
  const int lo = (int)blockIdx.x * chunk;
  const int hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  const int mine = hi > lo ? hi - lo : 0;
  if (mine == 0) return;                                                           // (uniform per workgroup: before any barrier)

  const int VK = __builtin_amdgcn_readfirstlane(p.VK), K0 = __builtin_amdgcn_readfirstlane(p.K0);
  const int Kp = __builtin_amdgcn_readfirstlane(p.Kp);
  const int split = (int)(p.row_split < p.N ? p.row_split : p.N);
  const float slope = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.slope)));
  const float4 bias4 = buf_load4(make_rsrc(p.bias, p.bias ? kRowBytes : 0u), col4, 0);     // (no bias: zero records -> zeros, no branch)
  const srsrc_t rs_venc = make_srsrc(p.venc, p.ldv, p.N);
  const srsrc_t rs_S0 = make_srsrc(p.S0, p.lds, p.N);
  const srsrc_t rs_H1 = make_srsrc(p.h1, p.ldh, p.N);
  const srsrc_t rs_P = make_srsrc(p.P, p.ldp, p.N);
  const rsrc_t rs_list = make_rsrc(p.list, p.list ? (uint32_t)(p.list_bound * 4) : 0u);

  // ---- the panels: BW[t][0..2] = the k-groups of the first block (H1n), BW[t][3], BW[t][4] = the venc k-group of P_dst, P_src;
  // fragment element j of lane (li, h): packed row of code 8 h + j of the group, column `col` of the block
  Split8 BW[2][5];
  {
    const rsrc_t rs_W = make_rsrc(p.W, (uint32_t)(((int64_t)(p.tables - 1) * p.wstride + (int64_t)(VK + 2 * K0 - 1) * p.ldw + 3 * kHN) * 4));
#pragma unroll
    for (int t = 0; t < 2; ++t) {                                                  // (a table at a time: forty values in flight)
      float w[5][8];
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        const int g = f < 3 ? f : 0, blk = f < 3 ? 0 : f - 2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = 8 * h + j;
          const bool ok = t < p.tables && c < (g == 0 ? VK : K0);
          const int row = g == 0 ? c : VK + (g - 1) * K0 + c;
          const uint32_t off = ok ? (uint32_t)(((int64_t)t * p.wstride + (int64_t)row * p.ldw + blk * kHN + col) * 4) : kOOBN;
          w[f][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_W, (int)off, 0, 0));
        }
      }
#pragma unroll
      for (int f = 0; f < 5; ++f)
        split8(make_float4(w[f][0], w[f][1], w[f][2], w[f][3]), make_float4(w[f][4], w[f][5], w[f][6], w[f][7]), BW[t][f]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- staging: thread (srow, sc) of row srow loads two chunks of four codes: sc < 4 the venc chunk sc and the S0_out chunk sc,
  // sc >= 4 the S0_in chunk sc - 4 (its venc load is requested at row -1); a chunk past the columns in memory is requested at row -1
  // too: zeros, no memory access.  (One descriptor per load instruction: a per-lane choice of descriptor is a waterfall loop.)
  const int srow = threadIdx.x >> 3, sc = threadIdx.x & 7, sq = sc & 3;
  const bool first = sc < 4;
  const bool a_on = first && 4 * sq < (int)p.ldv, b_on = 4 * sq < Kp;
  const int a_lim = VK - 4 * sq, b_lim = K0 - 4 * sq;                              // columns of the chunk in use (beyond: anything in memory)
  const uint32_t b_off = (uint32_t)((first ? Kp : 0) + 4 * sq) * 4u;
  const bool listed = p.list != nullptr;
  const int prefix = (int)p.prefix;
  // (plain values handed from step to step, no state captured by reference: a choice between two captured variables becomes a
  // choice between two stack addresses)
  auto tile_pos = [=](int k) { return (lo + (k < mine ? k : mine - 1)) * kSub + srow; };   // of tile lo + k, clamped to this workgroup's last tile
  auto fetch_id = [=](int q) { return (int)__builtin_amdgcn_raw_buffer_load_b32(rs_list, (int)((uint32_t)q * 4u), 0, 0); };   // (no list: zero records)
  auto row_of = [=](int k, int q, int raw) {                                       // the row at position q of tile lo + k (-1: none)
    const int id = (listed && q >= prefix) ? raw : q;
    return (k < mine && q < cnt) ? id : -1;
  };
  int q_req = tile_pos(0), raw_id = fetch_id(q_req);
  int id_data = row_of(0, q_req, raw_id);                                          // tile 0
  float4 pre_a = sbuf_load4(rs_venc, a_on ? id_data : -1, (uint32_t)sq * 16u);
  float4 pre_b = sbuf_load4(rs_S0, b_on ? id_data : -1, b_off);
  q_req = tile_pos(1);
  raw_id = fetch_id(q_req);
  auto stage = [=](int buf, const float4 pre_a, const float4 pre_b, int id_data) {   // registers -> the image, the row ids
    uint2 ah, am, al, bh, bm, bl;
    split_pair(a_lim > 0 ? pre_a.x : 0.f, a_lim > 1 ? pre_a.y : 0.f, ah.x, am.x, al.x);
    split_pair(a_lim > 2 ? pre_a.z : 0.f, a_lim > 3 ? pre_a.w : 0.f, ah.y, am.y, al.y);
    split_pair(b_lim > 0 ? pre_b.x : 0.f, b_lim > 1 ? pre_b.y : 0.f, bh.x, bm.x, bl.x);
    split_pair(b_lim > 2 ? pre_b.z : 0.f, b_lim > 3 ? pre_b.w : 0.f, bh.y, bm.y, bl.y);
    uint32_t *const q = img + buf * kNTile + srow * kNStride + 2 * sq;
    uint32_t *const qb = q + (first ? 16 : 8);
    *reinterpret_cast<uint2 *>(qb) = bh;
    *reinterpret_cast<uint2 *>(qb + kNPlane) = bm;
    *reinterpret_cast<uint2 *>(qb + 2 * kNPlane) = bl;
    if (first) {
      *reinterpret_cast<uint2 *>(q) = ah;
      *reinterpret_cast<uint2 *>(q + kNPlane) = am;
      *reinterpret_cast<uint2 *>(q + 2 * kNPlane) = al;
    }
    if (sc == 0) rowid[buf * kSub + srow] = id_data;
  };

  for (int k = 0; k < mine; ++k) {
    const int buf = k & 1;
    stage(buf, pre_a, pre_b, id_data);                                             // tile k
    id_data = row_of(k + 1, q_req, raw_id);                                        // tile k+1 (past the end: nothing)
    pre_a = sbuf_load4(rs_venc, a_on ? id_data : -1, (uint32_t)sq * 16u);
    pre_b = sbuf_load4(rs_S0, b_on ? id_data : -1, b_off);
    q_req = tile_pos(k + 2);
    raw_id = fetch_id(q_req);
    lds_barrier();                                                                 // (barrier k) tile k is staged for everyone
    int ids[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ids[q] = rowid[buf * kSub + 8 * q + lrow];
    const int myid = rowid[buf * kSub + li];
    const bool in0 = myid >= 0 && myid < split, in1 = myid >= split;
    const bool has0 = __builtin_amdgcn_ballot_w64(in0) != 0, has1 = __builtin_amdgcn_ballot_w64(in1) != 0;
    // this lane's fragments: codes 8 h .. 8 h + 7 of every k-group of image row li
    const uint32_t *const ar = img + buf * kNTile + li * kNStride + 4 * h;
    Frag8 A[kNGroups][3];
#pragma unroll
    for (int g = 0; g < kNGroups; ++g) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) A[g][pl].v = *reinterpret_cast<const bf16x8 *>(ar + pl * kNPlane + 8 * g);
    }
    // ---- a block at a time: the product, then the block through this wave's scratch as rows of 4 consecutive columns per lane
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      auto product = [&](const Split8 *B, bool on) {                                // one table's rows: the others' fragments are zeros
#pragma unroll
        for (int g = 0; g < (b == 0 ? kNGroups : 1); ++g) {
          Frag8 M[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int d = 0; d < 4; ++d) M[pl].u[d] = on ? A[g][pl].u[d] : 0u;
          }
          acc = mfma_x6(M[0], M[1], M[2], B[b == 0 ? g : b + 2], acc);
        }
      };
      if (has0) product(BW[0], in0);                                               // (wave-uniform, around MFMAs only)
      if (has1) product(BW[1], in1);
#pragma unroll
      for (int r = 0; r < 16; ++r) scr[((r & 3) + 8 * (r >> 2) + 4 * h) * kScrStride + li] = acc[r];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 v = *reinterpret_cast<const float4 *>(&scr[(8 * q + lrow) * kScrStride + (lane & 7) * 4]);
        if (b == 0) {
          v.x = act_fwd(v.x + bias4.x, slope); v.y = act_fwd(v.y + bias4.y, slope);
          v.z = act_fwd(v.z + bias4.z, slope); v.w = act_fwd(v.w + bias4.w, slope);
          sbuf_store4(v, rs_H1, ids[q], col4);                                     // padding rows (-1): dropped
        } else {
          sbuf_store4(v, rs_P, ids[q], col4 + (uint32_t)(b - 1) * kRowBytes);
        }
      }
    }
  }
}


// ---- the BACKWARD's contraction over the kept node rows, ONE launch (what dmp_smallk_atb_jobs and dmp_smallk_atb_cols_* made in two):
//
//   X[h][table rows] = S0_h^T dPn                                     (h = in, out;  dPn = dXP[:, 0:H])
//   Y[b][table rows] = venc^T (block b of [dXP | dxn])                (b = 0 .. 2, and 3 with the residual)
//
// on v_mfma_f32_16x16x32_bf16 (bf16x6): the contraction index is the tile's 32 rows, the A operand the tile's code rows TRANSPOSED
// (sixteen codes of venc / S0_in / S0_out x 32 rows, staged as bf16 pieces by the forward's staging threads, one 2-byte store per
// piece), the B operand the fp32 rows of dXP / dxn: lane (j, kb) holds rows 8 kb .. 8 kb + 7 of the tile at the columns 2 j, 2 j + 1 of
// its wave's 32 (one 8-byte load per row and block: sixteen lanes cover a row's 128 bytes), split once per tile.  MFMA column j of
// N-tile u is therefore column 32 cs + 2 j + u of the block.  Only the block pairs that are asked for are formed: S0 against dPn alone.
// Tables: the list is ascending, so a workgroup's tiles are [table 0's] [at most one mixed tile] [table 1's]; the workgroup makes one
// PASS per table over its range with the rows of the other table masked out (row id -1: no memory access, zero pieces) and skips a
// tile without a row of the pass's table; X (and Y with a venc table per pass) goes out after each pass, Y of a single venc table
// after the last.  A workgroup's sums go out as partials [workgroup][...] for the layer's deferred reduction: no atomics, a fixed
// order, and a workgroup without tiles writes zeros.
struct L0NodeBwdArgs {
  const float *venc; int64_t ldv; int VK; int vtables;
  const float *S0; int64_t lds; int K0, Kp; int stables;
  int64_t row_split;
  const float *dXP; int64_t ldd; const float *dxn; int64_t ldx;   // dxn NULL: three blocks
  const int32_t *list, *count; int64_t list_bound, prefix, N;
  float *partX, *partY;                                           // [G][2][stables K0][H], [G][nblk][vtables VK][H]
};

constexpr int kTRow = 40;                            // halves per transposed image row: 32 tile rows + 8 of padding (16-byte fragments)
constexpr int kTPlane = 48 * kTRow;                  // 48 code columns
constexpr int kTTile = 3 * kTPlane;                  // hi | mid | lo: 11520 bytes

__global__ __launch_bounds__(kGroupThreads, 2) void l0_node_bwd_k(const L0NodeBwdArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned short timg[2 * kTTile];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, j = lane & 15, kb = lane >> 4;
  const int nblk = p.dxn ? 4 : 3;
  const int VK = __builtin_amdgcn_readfirstlane(p.VK), K0 = __builtin_amdgcn_readfirstlane(p.K0);
  const int Kp = __builtin_amdgcn_readfirstlane(p.Kp);
  const int cnt = __builtin_amdgcn_readfirstlane(p.count ? *p.count : (int)p.N);
  const int ntiles = (cnt + kSub - 1) / kSub;
  const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = (int)blockIdx.x * chunk;
  const int hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  const int mine = hi > lo ? hi - lo : 0;
  const int split = (int)(p.row_split < p.N ? p.row_split : p.N);
  const bool listed = p.list != nullptr;
  const int prefix = (int)p.prefix;
  const srsrc_t rs_venc = make_srsrc(p.venc, p.ldv, p.N);
  const srsrc_t rs_S0 = make_srsrc(p.S0, p.lds, p.N);
  const srsrc_t rs_D = make_srsrc(p.dXP, p.ldd, p.N);
  const srsrc_t rs_X = make_srsrc(p.dxn, p.dxn ? p.ldx : (int64_t)kHN, p.dxn ? p.N : 0);
  const rsrc_t rs_list = make_rsrc(p.list, p.list ? (uint32_t)(p.list_bound * 4) : 0u);
  const int srow = threadIdx.x >> 3, sc = threadIdx.x & 7, sq = sc & 3;
  const bool first = sc < 4;
  const bool a_on = first && 4 * sq < (int)p.ldv, b_on = 4 * sq < Kp;
  const int a_lim = VK - 4 * sq, b_lim = K0 - 4 * sq;
  const uint32_t b_off = (uint32_t)((first ? Kp : 0) + 4 * sq) * 4u;
  const uint32_t colb = (uint32_t)(32 * wave + 2 * j) * 4u;       // this lane's two columns of a block, in bytes
  const int TK = p.stables * K0, TVK = p.vtables * VK;
  float *const pX = p.partX + (int64_t)blockIdx.x * 2 * TK * kHN;
  float *const pY = p.partY + (int64_t)blockIdx.x * nblk * TVK * kHN;

  auto row_at = [=](int q, int raw, int pass) {                   // the row at list position q if it belongs to the pass's table, else -1
    const int id = (listed && q >= prefix) ? raw : q;
    const bool ok = q < cnt && id >= 0 && ((id >= split) == (pass == 1));
    return ok ? id : -1;
  };
  auto six = [&](f32x4 &c, const Frag8 &ah, const Frag8 &am, const Frag8 &al, const Split8 &bb) {   // the small terms first (mfma_x6's order)
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al.v, bb.hi.v, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah.v, bb.lo.v, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am.v, bb.mid.v, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am.v, bb.hi.v, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah.v, bb.mid.v, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah.v, bb.hi.v, c, 0, 0, 0);
  };
  // accumulator element r of lane (j, kb): code 4 kb + r, columns 2 j + u of the wave's 32
  auto emit = [=](float *base, int rows_k, const f32x4 &a0, const f32x4 &a1) {      // base: the [rows_k, H] block of the partial
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 4 * kb + r;
      if (m < rows_k) *reinterpret_cast<float2 *>(base + (int64_t)m * kHN + 32 * wave + 2 * j) = make_float2(a0[r], a1[r]);
    }
  };
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 Y[4][2];
#pragma unroll
  for (int b = 0; b < 4; ++b) { Y[b][0] = zero4; Y[b][1] = zero4; }
  const int passes = p.stables;
  int step = 0;                                                   // staged tiles so far: the image buffer alternates
  for (int pass = 0; pass < passes; ++pass) {
    f32x4 X[2][2] = {{zero4, zero4}, {zero4, zero4}};
    for (int k = 0; k < mine; ++k) {
      const int buf = step & 1;
      const int q0 = (lo + k) * kSub;
      // ---- this lane's eight rows of the tile (rows 8 kb .. 8 kb + 7), and the staging thread's row
      const u32x4 l0 = __builtin_amdgcn_raw_buffer_load_b128(rs_list, (int)((uint32_t)(q0 + 8 * kb) * 4u), 0, 0);
      const u32x4 l1 = __builtin_amdgcn_raw_buffer_load_b128(rs_list, (int)((uint32_t)(q0 + 8 * kb + 4) * 4u), 0, 0);
      const int sraw = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_list, (int)((uint32_t)(q0 + srow) * 4u), 0, 0);
      int rid[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) rid[s] = row_at(q0 + 8 * kb + s, (int)(s < 4 ? l0[s] : l1[s - 4]), pass);
      const int sid = row_at(q0 + srow, sraw, pass);
      bool any = false;
#pragma unroll
      for (int s = 0; s < 8; ++s) any = any || rid[s] >= 0;
      const bool has = __builtin_amdgcn_ballot_w64(any) != 0;     // (every wave sees all 32 rows: the same verdict in all four)
      if (!has) continue;                                         // (uniform per workgroup: no barrier is skipped by a part of it)
      // ---- the B rows, all in flight before anything waits
      i32x2 Bv[4][8];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
#pragma unroll
        for (int s = 0; s < 8; ++s) Bv[b][s] = llvm_struct_buffer_load_v2i32(rs_D, rid[s], (int)(colb + (uint32_t)b * (kHN * 4u)), 0, 0);
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) Bv[3][s] = llvm_struct_buffer_load_v2i32(rs_X, rid[s], (int)colb, 0, 0);      // (no residual: zero records)
      // ---- the code rows, transposed into the image as bf16 pieces
      const float4 ca = sbuf_load4(rs_venc, a_on ? sid : -1, (uint32_t)sq * 16u);
      const float4 cb = sbuf_load4(rs_S0, b_on ? sid : -1, b_off);
      {
        unsigned short *const t = timg + buf * kTTile + srow;
        const float av[4] = {a_lim > 0 ? ca.x : 0.f, a_lim > 1 ? ca.y : 0.f, a_lim > 2 ? ca.z : 0.f, a_lim > 3 ? ca.w : 0.f};
        const float bv[4] = {b_lim > 0 ? cb.x : 0.f, b_lim > 1 ? cb.y : 0.f, b_lim > 2 ? cb.z : 0.f, b_lim > 3 ? cb.w : 0.f};
        const int mb = (first ? 32 : 16) + 4 * sq;                // S0_out behind S0_in behind venc
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          uint32_t h2, m2, l2;
          split_pair(bv[e], bv[e + 1], h2, m2, l2);
          t[(mb + e) * kTRow] = (unsigned short)h2; t[(mb + e + 1) * kTRow] = (unsigned short)(h2 >> 16);
          t[kTPlane + (mb + e) * kTRow] = (unsigned short)m2; t[kTPlane + (mb + e + 1) * kTRow] = (unsigned short)(m2 >> 16);
          t[2 * kTPlane + (mb + e) * kTRow] = (unsigned short)l2; t[2 * kTPlane + (mb + e + 1) * kTRow] = (unsigned short)(l2 >> 16);
          if (first) {
            split_pair(av[e], av[e + 1], h2, m2, l2);
            const int ma = 4 * sq + e;
            t[ma * kTRow] = (unsigned short)h2; t[(ma + 1) * kTRow] = (unsigned short)(h2 >> 16);
            t[kTPlane + ma * kTRow] = (unsigned short)m2; t[kTPlane + (ma + 1) * kTRow] = (unsigned short)(m2 >> 16);
            t[2 * kTPlane + ma * kTRow] = (unsigned short)l2; t[2 * kTPlane + (ma + 1) * kTRow] = (unsigned short)(l2 >> 16);
          }
        }
      }
      lds_barrier();             // the image of this tile is complete; the other buffer's readers passed the barrier before
      // ---- this lane's A fragments: code 16 g + j of k-group g (venc | S0_in | S0_out), tile rows 8 kb .. 8 kb + 7
      Frag8 A[3][3];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          A[g][pl].v = *reinterpret_cast<const bf16x8 *>(timg + buf * kTTile + pl * kTPlane + (16 * g + j) * kTRow + 8 * kb);
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b == 3 && nblk == 3) break;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          Split8 B;
          split8(make_float4(__int_as_float(Bv[b][0][u]), __int_as_float(Bv[b][1][u]), __int_as_float(Bv[b][2][u]), __int_as_float(Bv[b][3][u])),
                 make_float4(__int_as_float(Bv[b][4][u]), __int_as_float(Bv[b][5][u]), __int_as_float(Bv[b][6][u]), __int_as_float(Bv[b][7][u])), B);
          six(Y[b][u], A[0][0], A[0][1], A[0][2], B);
          if (b == 0) {
            six(X[0][u], A[1][0], A[1][1], A[1][2], B);
            six(X[1][u], A[2][0], A[2][1], A[2][2], B);
          }
        }
      }
      ++step;                    // (only a staged tile turns the buffers: two staged tiles in a row never share one)
    }
    // ---- the pass's sums: X of its table; Y too where venc has a table per pass
    emit(pX + (int64_t)(0 * TK + pass * K0) * kHN, K0, X[0][0], X[0][1]);
    emit(pX + (int64_t)(1 * TK + pass * K0) * kHN, K0, X[1][0], X[1][1]);
    if (p.vtables == 2 || pass == passes - 1) {
      const int vt = p.vtables == 2 ? pass : 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (b < nblk) emit(pY + (int64_t)(b * TVK + vt * VK) * kHN, VK, Y[b][0], Y[b][1]);
        Y[b][0] = zero4; Y[b][1] = zero4;
      }
    }
  }
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_l0_node_fwd_mfma_max_codes(void) { return 16; }

int dmp_l0_node_fwd_mfma(const float *venc, int64_t ldv, int VK, const float *S0, int64_t lds, int K0, int Kp, const float *W, int64_t ldw,
                         int64_t wstride, int tables, int64_t row_split, const float *bias, float slope, const uint32_t *rowmask,
                         const int32_t *list, const int32_t *count, int64_t list_bound, int64_t prefix, int64_t N, int H, float *h1,
                         int64_t ldh, float *P, int64_t ldp, void *stream) {
  if (H != kHN || g_exact_fp32) return DMP_ERR_UNSUPPORTED;
  if (N < 0 || VK < 1 || K0 < 1 || Kp < K0 || tables < 1 || row_split < 0 || prefix < 0 || prefix > N ||
      (list && (!count || list_bound < 0 || prefix > list_bound)) || (!list && count))
    return DMP_ERR_BAD_ARG;
  if (VK > 16 || K0 > 16 || tables > 2 || !slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (N == 0) return DMP_OK;
  if (!venc || !S0 || !W || !h1 || !P || ldv < VK || lds < 2 * Kp || ldw < 3 * H || ldh < H || ldp < 2 * H || (tables > 1 && wstride <= 0))
    return DMP_ERR_BAD_ARG;
  if (ldv % 4 || lds % 4 || Kp % 4 || ldh % 4 || ldp % 4 || !aligned16(venc) || !aligned16(S0) || !aligned16(h1) || !aligned16(P) ||
      (bias && !aligned16(bias)) || (reinterpret_cast<uintptr_t>(W) & 3u))
    return DMP_ERR_UNSUPPORTED;
  const int64_t lim32 = ((int64_t)1 << 32) - 8192;
  if (!stride_ok(ldv) || !stride_ok(lds) || !stride_ok(ldh) || !stride_ok(ldp) || N >= ((int64_t)1 << 31) - 64 || !fits4g(N, ldv) ||
      !fits4g(N, lds) || !fits4g(N, ldh) || !fits4g(N, ldp) || (list && list_bound * 4 >= lim32) ||
      ((int64_t)(tables - 1) * wstride + (int64_t)(VK + 2 * K0) * ldw + 3 * H) * 4 >= lim32)
    return DMP_ERR_UNSUPPORTED;                                                    // (arrays the descriptors cannot address: the launches per table)
  L0NodeArgs a{};
  a.venc = venc; a.ldv = ldv; a.VK = VK; a.S0 = S0; a.lds = lds; a.K0 = K0; a.Kp = Kp; a.W = W; a.ldw = ldw; a.wstride = tables > 1 ? wstride : 0;
  a.tables = tables; a.row_split = tables == 1 ? N : row_split; a.bias = bias; a.slope = slope; a.rowmask = rowmask; a.list = list; a.count = count;
  a.list_bound = list ? list_bound : 0; a.prefix = list ? prefix : 0; a.N = N; a.h1 = h1; a.ldh = ldh; a.P = P; a.ldp = ldp;
  // a list holds at most min(list_bound, N) rows; two workgroups per CU, one round of resident waves
  const int64_t rows_bound = list ? (list_bound < N ? list_bound : N) : N;
  const int64_t tiles_bound = (rows_bound + kSub - 1) / kSub;
  const int64_t words = (N + 31) / 32;
  a.tile_blocks = (int)(tiles_bound < 512 ? (tiles_bound > 0 ? tiles_bound : 1) : 512);
  const int64_t zb = rowmask ? ((words + 3) / 4 < 1024 ? (words + 3) / 4 : 1024) : 0;
  l0_node_mfma_k<<<(unsigned)(a.tile_blocks + zb), kGroupThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

int64_t dmp_l0_node_codes_bwd_blocks(int64_t rows_bound) {
  const int64_t tiles = (rows_bound + kSub - 1) / kSub;
  return tiles < 256 ? (tiles > 0 ? tiles : 1) : 256;             // one workgroup per CU: each writes a partial of every sum
}

int dmp_l0_node_codes_bwd(const float *venc, int64_t ldv, int VK, int vtables, const float *S0, int64_t lds, int K0, int Kp, int stables,
                          int64_t row_split, const float *dXP, int64_t ldd, const float *dxn, int64_t ldx, const int32_t *list,
                          const int32_t *count, int64_t list_bound, int64_t prefix, int64_t N, int H, float *partX, float *partY,
                          void *stream) {
  if (H != kHN || g_exact_fp32) return DMP_ERR_UNSUPPORTED;
  if (N < 0 || VK < 1 || K0 < 1 || Kp < K0 || stables < 1 || vtables < 1 || row_split < 0 || prefix < 0 || prefix > N || !partX || !partY ||
      (list && (!count || list_bound < 0 || prefix > list_bound)) || (!list && count))
    return DMP_ERR_BAD_ARG;
  if (VK > 16 || K0 > 16 || stables > 2 || vtables > stables) return DMP_ERR_UNSUPPORTED;
  const int64_t rows_bound = list ? (list_bound < N ? list_bound : N) : N;
  const int64_t G = dmp_l0_node_codes_bwd_blocks(rows_bound);
  const int nblk = dxn ? 4 : 3;
  if (N == 0) {
    if (hipMemsetAsync(partX, 0, sizeof(float) * (size_t)(G * 2 * stables * K0 * H), (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(partY, 0, sizeof(float) * (size_t)(G * nblk * vtables * VK * H), (hipStream_t)stream) != hipSuccess)
      return DMP_ERR_HIP;
    return DMP_OK;
  }
  if (!venc || !S0 || !dXP || ldv < VK || lds < 2 * Kp || ldd < 3 * H || (dxn && ldx < H)) return DMP_ERR_BAD_ARG;
  if (ldv % 4 || lds % 4 || Kp % 4 || ldd % 2 || (dxn && ldx % 2) || !aligned16(venc) || !aligned16(S0) || !aligned16(list) ||
      (reinterpret_cast<uintptr_t>(dXP) & 7u) || (reinterpret_cast<uintptr_t>(dxn) & 7u) || (reinterpret_cast<uintptr_t>(partX) & 7u) ||
      (reinterpret_cast<uintptr_t>(partY) & 7u))
    return DMP_ERR_UNSUPPORTED;
  const int64_t lim32 = ((int64_t)1 << 32) - 8192;
  if (!stride_ok(ldv) || !stride_ok(lds) || !stride_ok(ldd) || (dxn && !stride_ok(ldx)) || N >= ((int64_t)1 << 31) - 64 || !fits4g(N, ldv) ||
      !fits4g(N, lds) || !fits4g(N, ldd) || (dxn && !fits4g(N, ldx)) || (list && list_bound * 4 >= lim32))
    return DMP_ERR_UNSUPPORTED;
  L0NodeBwdArgs a{};
  a.venc = venc; a.ldv = ldv; a.VK = VK; a.vtables = vtables; a.S0 = S0; a.lds = lds; a.K0 = K0; a.Kp = Kp; a.stables = stables;
  a.row_split = stables == 1 ? N : row_split; a.dXP = dXP; a.ldd = ldd; a.dxn = dxn; a.ldx = dxn ? ldx : H; a.list = list; a.count = count;
  a.list_bound = list ? list_bound : 0; a.prefix = list ? prefix : 0; a.N = N; a.partX = partX; a.partY = partY;
  l0_node_bwd_k<<<(unsigned)G, kGroupThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

}  // extern "C"
