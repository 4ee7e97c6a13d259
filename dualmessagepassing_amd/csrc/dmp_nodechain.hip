// The node side of a DMPNN layer over the tiles of the kept nodes as ONE launch per pass (gfx950, H = 128, bf16x6).
//
//   forward   H1n = act([x | S_in | S_out] [Wx0; Bn_in; Bn_out] + bn),  P_dst = x Wx1,  P_src = x Wx2,  xn = x + H1n W2^T + b2
//   backward  dPn = act'(H1n) (.) (dxn W2),  dS_in = dPn Bn_in^T,  dS_out = dPn Bn_out^T,  dx = dxn + [dPn | dP_dst | dP_src] Wx^T
//   (SubgraphCountingMatching/models/dmpnn.py:113,121,125,129-140 over the folded weights of dmp_fold.hip)
//
// Both are six [rows, 128] x [128, 128] products on row-local operands.  The tile kernels of dmp_typed.hip keep ONE weight panel
// in registers, so such a chain is three dependent launches with partial sums going through memory.  Here the ROWS stay put and
// the PANELS stream: a 256-thread workgroup (two per CU) owns a contiguous range of the tile list and walks it 2 tiles = 64
// rows at a time; the rows' current operand sits in LDS as three bf16 planes (the image of dmp_typed.hip, 52,224 bytes), the
// 64 x 128 fp32 result block in registers (wave w: tile w / 2, columns 64 (w & 1) ..: 2 x 16 accumulators per lane), and the
// six panels -- split into their bf16 pieces ONCE per step by dmp_node_chain_pack, in fragment order -- come from L2 through two
// 12 KiB LDS buffers, one k-group of a panel (16 k) per step, requested two steps ahead into a ring of two register sets.
// A workgroup still waits at most steps' end; the CU's two workgroups share no barrier, so one multiplies while the other
// waits (docs/HISTORY.md (pp)).
// A product's result that is the next product's operand (H1n, dPn) goes from the accumulators straight into the LDS image.
//
// Summation order is fixed (k-groups ascending inside a panel, panels in the order above; the column-sum partials through
// fixed trees), so a launch repeats bit for bit.
#include "dmp_mfma_common.h"

namespace dmp {
// one-dword forms of dmp_mfma_common.h's structured buffer access (the accumulator layout holds one column per lane)
__device__ int llvm_struct_buffer_load_i32(i32x4 rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.i32");
__device__ void llvm_struct_buffer_store_i32(int data, i32x4 rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.store.i32");
namespace {

constexpr int kChainTiles = 2;                                // tiles per pass of a workgroup (even): two waves per tile
constexpr int kChainThreads = 128 * kChainTiles;              // 256
constexpr int kChainRows = 32 * kChainTiles;                  // rows per pass of a workgroup: 64
constexpr int kChainStageRows = kChainThreads / 32;           // rows one staging sweep covers (32 float4 per row): 8 sweeps per pass
constexpr int kChainStrideD = 68;                             // dwords per image row: 128 bf16 + 8 of padding (dmp_typed.hip)
constexpr int kChainPlane = kChainRows * kChainStrideD;       // dwords per piece plane
constexpr int kChainImageBytes = 3 * kChainPlane * 4;         // 52,224
constexpr int kChainPanelBytes = 3 * 128 * 128 * 2;           // 98,304: [k-group 8][piece 3][column block 4][lane 64][8 bf16]
constexpr int kChainGroupBytes = kChainPanelBytes / 8;        // 12,288: one k-group
constexpr int kChainChunkGroups = kChainTiles / 2;            // k-groups per step: every thread fetches 3 x 16 bytes of them
constexpr int kChainChunkBytes = kChainChunkGroups * kChainGroupBytes;      // 12,288
constexpr int kChainSteps = 8 / kChainChunkGroups;            // steps per panel (even: a panel starts in buffer 0)
constexpr int kChainLdsBytes = kChainImageBytes + 2 * kChainChunkBytes + kChainRows * 4;   // 77,056: two workgroups in the CU's 163,840
constexpr int kChainBlocksPerCU = 163840 / kChainLdsBytes;    // 2
constexpr int kChainCUs = 256;
constexpr int kChainMaxBlocks = kChainCUs * kChainBlocksPerCU;      // every CU's share resident at once: 512
static_assert(kChainTiles % 2 == 0 && kChainSteps % 2 == 0 && kChainChunkBytes == 3 * kChainThreads * 16, "chunk = one 3 x 16-byte fetch per thread");
constexpr int kChainMaxPanels = 12;

__device__ __forceinline__ float sbuf_load1(srsrc_t r, int row, uint32_t col_bytes) {
  return __int_as_float(llvm_struct_buffer_load_i32(r, row, (int)col_bytes, 0, 0));
}
__device__ __forceinline__ void sbuf_store1(float v, srsrc_t r, int row, uint32_t col_bytes) {
  llvm_struct_buffer_store_i32(__float_as_int(v), r, row, (int)col_bytes, 0, 0);
}

// ---- the panels as bf16 pieces in fragment order: value j of lane (h, li) of column block cb, k-group g of panel p is
// B_p[64 h + 8 g + j][32 cb + li] (the k order of dmp_typed.hip's image reads), B_p[k][c] = W[k][c] or, transposed, W[c][k]
struct PackArgs {
  const float *W[kChainMaxPanels];
  int64_t ld[kChainMaxPanels];
  int transposed[kChainMaxPanels];
  uint32_t *out;
};
__global__ __launch_bounds__(256) void chain_pack_k(PackArgs p) {
  const int item = (int)blockIdx.x * 256 + (int)threadIdx.x;      // (g, cb, lane): 2048 per panel
  const int lane = item & 63, cb = (item >> 6) & 3, g = item >> 8;
  const int li = lane & 31, h = lane >> 5;
  const float *W = nullptr;
  int64_t ld = 0;
  int tr = 0;
#pragma unroll
  for (int j = 0; j < kChainMaxPanels; ++j)
    if (j == (int)blockIdx.y) { W = p.W[j]; ld = p.ld[j]; tr = p.transposed[j]; }
  const int k0 = 64 * h + 8 * g, c = 32 * cb + li;
  float w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = tr ? W[(int64_t)c * ld + k0 + j] : W[(int64_t)(k0 + j) * ld + c];
  Split8 s;
  split8(make_float4(w[0], w[1], w[2], w[3]), make_float4(w[4], w[5], w[6], w[7]), s);
  uint32_t *o = p.out + (size_t)blockIdx.y * (kChainPanelBytes / 4) + (size_t)g * 3072 + cb * 256 + lane * 4;
  *reinterpret_cast<uint4 *>(o) = make_uint4(s.hi.u[0], s.hi.u[1], s.hi.u[2], s.hi.u[3]);
  *reinterpret_cast<uint4 *>(o + 1024) = make_uint4(s.mid.u[0], s.mid.u[1], s.mid.u[2], s.mid.u[3]);
  *reinterpret_cast<uint4 *>(o + 2048) = make_uint4(s.lo.u[0], s.lo.u[1], s.lo.u[2], s.lo.u[3]);
}

struct ChainArgs {
  const float *A0, *A1, *A2;            // row operands: forward x, S_in, S_out; backward dxn, dP_dst, dP_src
  int64_t lda0, lda1, lda2;
  const float *X; int64_t ldx;          // backward: H1n (the saved activation)
  const float *Res; int64_t ldres;      // residual rows added to the last product (forward x, backward dxn) or NULL
  const float *bias1, *bias2;           // forward: bn, b2
  float *O0, *O1, *O2, *O3;             // forward P_dst, P_src, H1n, xn; backward dPn, dS_in, dS_out, dx
  int64_t ldo0, ldo1, ldo2, ldo3;
  float *partial, *partialA;            // backward: [grid, 128] column sums of dPn / of the fetched dxn rows
  const uint32_t *panels;               // dmp_node_chain_pack's output: the pass's panels in the order they are used
  int npanels;                          // 6; backward without dx: 3
  const int32_t *slot; const int32_t *num_tiles;
  int64_t rows;
  float slope;
};

template <bool BWD, bool FULL>
__global__ __launch_bounds__(kChainThreads, kChainBlocksPerCU) void node_chain_k(ChainArgs p) {
  extern __shared__ __attribute__((aligned(256))) unsigned char lds[];
  uint32_t *Aimg = reinterpret_cast<uint32_t *>(lds);
  unsigned char *Pb = lds + kChainImageBytes;
  int *ids_s = reinterpret_cast<int *>(lds + kChainImageBytes + 2 * kChainChunkBytes);

  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lane = t & 63, li = lane & 31, h = lane >> 5;
  const int rt = wave >> 1, ch = wave & 1;                    // this wave's tile of the pass and its 64-column half
  const int q = t & 31, r0 = t >> 5;                          // staging: float4 q of rows r0 + kChainStageRows m
  const float slope = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.slope)));
  const bool has_res = p.Res != nullptr;
  const int NC = __builtin_amdgcn_readfirstlane(p.npanels) * kChainSteps;      // chunks per pass
  constexpr bool full = FULL;                                 // backward: dx wanted (forward: always)

  const int ntiles = __builtin_amdgcn_readfirstlane(*p.num_tiles);
  const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = (int)blockIdx.x * chunk;
  const int hi = lo + chunk < ntiles ? lo + chunk : ntiles;
  if (hi <= lo) {
    if (BWD && t < 128) { p.partial[(int64_t)blockIdx.x * 128 + t] = 0.f; p.partialA[(int64_t)blockIdx.x * 128 + t] = 0.f; }
    return;
  }
  const rsrc_t rs_slot = make_rsrc(p.slot, (uint32_t)hi * (kSub * 4u));      // past this range's end: reads 0 (-> -1 below)
  const rsrc_t rs_pan = make_rsrc(p.panels, (uint32_t)NC * (uint32_t)kChainChunkBytes);
  const srsrc_t rs_A0 = make_srsrc(p.A0, p.lda0, p.rows), rs_A1 = make_srsrc(p.A1, p.lda1, p.rows), rs_A2 = make_srsrc(p.A2, p.lda2, p.rows);
  const srsrc_t rs_X = make_srsrc(p.X, p.X ? p.ldx : (int64_t)128, p.X ? p.rows : 0);
  const srsrc_t rs_Res = make_srsrc(p.Res, has_res ? p.ldres : (int64_t)128, has_res ? p.rows : 0);      // (none: zeros)
  const srsrc_t rs_O0 = make_srsrc(p.O0, p.ldo0, p.rows), rs_O1 = make_srsrc(p.O1, p.ldo1, p.rows), rs_O2 = make_srsrc(p.O2, p.ldo2, p.rows);
  const srsrc_t rs_O3 = make_srsrc(p.O3, p.O3 ? p.ldo3 : (int64_t)128, p.O3 ? p.rows : 0);

  int ids[8];
  float4 pre[8];
  auto load_ids = [&](int tile0) {                            // slots of the pass's tiles from tile0; past the range's end: -1
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int idx = tile0 * kSub + r0 + kChainStageRows * m;
      const int v = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_slot, idx * 4, 0, 0);
      ids[m] = idx < hi * kSub ? v : -1;
    }
  };
  auto load_rows = [&](srsrc_t rs) {                          // (id -1: zeros)
#pragma unroll
    for (int m = 0; m < 8; ++m) pre[m] = sbuf_load4(rs, ids[m], (uint32_t)q * 16u);
  };
  float4 csA = make_float4(0.f, 0.f, 0.f, 0.f);               // backward: this thread's 4 columns of the dxn rows it stages
  auto stage = [&](bool first) {                              // pre -> the image (split once, here); first: the pass's ids too
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int row = r0 + kChainStageRows * m;
      if (BWD && first) { csA.x += pre[m].x; csA.y += pre[m].y; csA.z += pre[m].z; csA.w += pre[m].w; }
      uint2 ph, pm, pl;
      split_pair(pre[m].x, pre[m].y, ph.x, pm.x, pl.x);
      split_pair(pre[m].z, pre[m].w, ph.y, pm.y, pl.y);
      uint32_t *d = Aimg + row * kChainStrideD + q * 2;
      *reinterpret_cast<uint2 *>(d) = ph;
      *reinterpret_cast<uint2 *>(d + kChainPlane) = pm;
      *reinterpret_cast<uint2 *>(d + 2 * kChainPlane) = pl;
      if (first && q == 0) ids_s[row] = ids[m];
    }
  };

  f32x16 acc[2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
  };
  // one panel = kChainSteps steps.  The chunks go through a ring of two register sets into the two LDS buffers: a step requests
  // the chunk TWO steps ahead (of this panel, the next one, or the next pass's first two) -- fenced, so that the request is issued
  // ahead of the step's MFMAs in every instantiation --, multiplies the current one (its k-groups x two column blocks x six piece
  // products), then stores the chunk requested a step earlier into the other buffer: the wait in front of that store leaves the
  // newest request in flight.  The CU's other workgroup, a phase apart, multiplies while this one waits -- but between two
  // waves of a SIMD the OLDER one wins every issue slot, so the workgroup that came second to a CU would run in the first one's
  // gaps only and finish a third later (docs/HISTORY.md (pp)).  The two therefore take the higher priority in turn, a product
  // each: workgroups b and b + kChainCUs share a CU when the grid fills the chip (a guess about placement that costs nothing
  // where it is wrong).
  uint4 pc[2][3];
  const int second = __builtin_amdgcn_readfirstlane((int)blockIdx.x / kChainCUs & 1);
  auto request = [&](int set, int c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_pan, (i * kChainThreads + t) * 16, c * kChainChunkBytes, 0);
      pc[set][i] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  auto product = [&](int pidx) {
#pragma unroll
    for (int cc = 0; cc < kChainSteps; ++cc) {
      const int c = kChainSteps * pidx + cc;
      const int nc = c + 2 >= NC ? c + 2 - NC : c + 2;
      if (cc == 0) {
        if ((pidx + second) & 1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      request(cc & 1, nc);
      __builtin_amdgcn_sched_barrier(0);
      const unsigned char *pb = Pb + (cc & 1) * kChainChunkBytes;
      const uint32_t *ar = Aimg + (32 * rt + li) * kChainStrideD + 32 * h;
#pragma unroll
      for (int gl = 0; gl < kChainChunkGroups; ++gl) {
        const int g = kChainChunkGroups * cc + gl;
        Split8 a;
        a.hi.v = *reinterpret_cast<const bf16x8 *>(ar + 4 * g);
        a.mid.v = *reinterpret_cast<const bf16x8 *>(ar + kChainPlane + 4 * g);
        a.lo.v = *reinterpret_cast<const bf16x8 *>(ar + 2 * kChainPlane + 4 * g);
#pragma unroll
        for (int cbl = 0; cbl < 2; ++cbl) {
          const unsigned char *bq = pb + gl * kChainGroupBytes + (2 * ch + cbl) * 1024 + lane * 16;
          Split8 b;
          b.hi.v = *reinterpret_cast<const bf16x8 *>(bq);
          b.mid.v = *reinterpret_cast<const bf16x8 *>(bq + 4096);
          b.lo.v = *reinterpret_cast<const bf16x8 *>(bq + 8192);
          acc[cbl] = mfma_x6(a, b, acc[cbl]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);                      // (the wait for the chunk stays behind the step's MFMAs)
      uint4 *pw = reinterpret_cast<uint4 *>(Pb + ((cc + 1) & 1) * kChainChunkBytes);
#pragma unroll
      for (int i = 0; i < 3; ++i) pw[i * kChainThreads + t] = pc[(cc + 1) & 1][i];
      lds_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  int rid[16];                                                // the ids of this lane's 16 accumulator rows
  auto store_acc = [&](srsrc_t rs) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sbuf_store1(acc[cb][r], rs, rid[r], (uint32_t)(64 * ch + 32 * cb + li) * 4u);
  };
  // the accumulators as the next product's operand: two neighbouring columns make a dword of each plane -- even lanes pack
  // the even accumulator rows, odd lanes the odd ones, with the neighbour's value of that row
  auto acc_to_image = [&]() {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float va = acc[cb][2 * i], vb = acc[cb][2 * i + 1];
        const float got = __shfl_xor((li & 1) ? va : vb, 1, 64);
        const float f0 = (li & 1) ? got : va, f1 = (li & 1) ? vb : got;
        const int r = 2 * i + (li & 1);
        const int row = 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h;
        uint32_t ph, pm, pl;
        split_pair(f0, f1, ph, pm, pl);
        uint32_t *d = Aimg + row * kChainStrideD + 32 * ch + 16 * cb + (li >> 1);
        d[0] = ph; d[kChainPlane] = pm; d[2 * kChainPlane] = pl;
      }
  };
  float colsum[2] = {0.f, 0.f};                               // backward: this lane's two columns of dPn

  // ---- prologue: the first pass's ids, then its rows; the first two chunks of the panels beside them (LDS, register set 1)
  load_ids(lo);
  load_rows(rs_A0);
  {
    uint4 *pw = reinterpret_cast<uint4 *>(Pb);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_pan, (i * kChainThreads + t) * 16, 0, 0);
      pw[i * kChainThreads + t] = make_uint4(v.x, v.y, v.z, v.w);
    }
    request(1, 1);
  }
  for (int g0 = lo; g0 < hi; g0 += kChainTiles) {
    stage(true);
    lds_barrier();
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int4 v = *reinterpret_cast<const int4 *>(&ids_s[32 * rt + 8 * qd + 4 * h]);
      rid[4 * qd] = v.x; rid[4 * qd + 1] = v.y; rid[4 * qd + 2] = v.z; rid[4 * qd + 3] = v.w;
    }
    if (!BWD) {
      load_rows(rs_A1);                                       // S_in, staged after the third product
      zero_acc(); product(0); store_acc(rs_O0);               // P_dst = x Wx1
      zero_acc(); product(1); store_acc(rs_O1);               // P_src = x Wx2
      zero_acc(); product(2);                                 // x Wx0
      stage(false); lds_barrier();
      load_rows(rs_A2);                                       // S_out
      product(3);                                             // + S_in Bn_in
      stage(false); lds_barrier();
      load_ids(g0 + kChainTiles);                                       // the next pass
      product(4);                                             // + S_out Bn_out
      load_rows(rs_A0);                                       // the next pass's x: requested ahead of this epilogue's stores
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const float b = p.bias1[64 * ch + 32 * cb + li];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = act_fwd(acc[cb][r] + b, slope);
      }
      float res[2][16];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) res[cb][r] = sbuf_load1(rs_Res, rid[r], (uint32_t)(64 * ch + 32 * cb + li) * 4u);
      store_acc(rs_O2);                                       // H1n
      acc_to_image();
      lds_barrier();
      zero_acc(); product(5);                                 // H1n W2^T
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const float b = p.bias2[64 * ch + 32 * cb + li];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = res[cb][r] + (acc[cb][r] + b);
      }
      store_acc(rs_O3);                                       // xn
    } else {
      float hv[2][16];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) hv[cb][r] = sbuf_load1(rs_X, rid[r], (uint32_t)(64 * ch + 32 * cb + li) * 4u);
      zero_acc(); product(0);                                 // dxn W2
      if (full) load_rows(rs_A1);                             // dP_dst: requested ahead of the stores
      else load_ids(g0 + kChainTiles);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[cb][r] = act_bwd(hv[cb][r], acc[cb][r], slope);     // (padding rows: activation 0, product 0 -> 0)
          colsum[cb] += acc[cb][r];
        }
      store_acc(rs_O0);                                       // dPn
      acc_to_image();
      lds_barrier();
      zero_acc(); product(1);
      if (!full) load_rows(rs_A0);                            // (no dx: the next pass's dxn)
      store_acc(rs_O1);                                       // dS_in = dPn Bn_in^T
      zero_acc(); product(2); store_acc(rs_O2);               // dS_out = dPn Bn_out^T
      if (full) {
        zero_acc(); product(3);                               // dPn Wx0^T
        stage(false); lds_barrier();
        load_rows(rs_A2);                                     // dP_src
        product(4);                                           // + dP_dst Wx1^T
        stage(false); lds_barrier();
        load_ids(g0 + kChainTiles);
        float res[2][16];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) res[cb][r] = sbuf_load1(rs_Res, rid[r], (uint32_t)(64 * ch + 32 * cb + li) * 4u);
        product(5);                                           // + dP_src Wx2^T
        load_rows(rs_A0);                                     // the next pass's dxn
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[cb][r] = res[cb][r] + acc[cb][r];
        store_acc(rs_O3);                                     // dx
      }
    }
  }
  if (BWD) {
    // column sums: the two half-waves of a lane's column, then the tiles' waves / the staging rows through LDS, in order
    float *red = reinterpret_cast<float *>(Pb);
    float *redA = red + kChainTiles * 128;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const float s = colsum[cb] + __shfl_xor(colsum[cb], 32, 64);
      if (h == 0) red[rt * 128 + 64 * ch + 32 * cb + li] = s;
    }
    *reinterpret_cast<float4 *>(&redA[r0 * 128 + q * 4]) = csA;
    lds_barrier();
    if (t < 128) {
      float s = red[t];
#pragma unroll
      for (int w = 1; w < kChainTiles; ++w) s += red[w * 128 + t];
      p.partial[(int64_t)blockIdx.x * 128 + t] = s;
      float sa = redA[t];
#pragma unroll
      for (int w = 1; w < kChainStageRows; ++w) sa += redA[w * 128 + t];
      p.partialA[(int64_t)blockIdx.x * 128 + t] = sa;
    }
  }
}

inline unsigned chain_blocks(int64_t tiles_bound) {
  const int64_t want = (tiles_bound + kChainTiles - 1) / kChainTiles;
  return (unsigned)(want < 1 ? 1 : (want > kChainMaxBlocks ? kChainMaxBlocks : want));
}

template <bool BWD, bool FULL>
inline bool chain_lds_ready() {
  static bool done[kMaxDevices] = {};
  return opt_in_lds(reinterpret_cast<const void *>(&node_chain_k<BWD, FULL>), kChainLdsBytes, done);
}

inline bool chain_rows_ok(const float *a, int64_t ld, int64_t rows) {
  return a && ld >= 128 && ld % 4 == 0 && aligned16(a) && stride_ok(ld) && fits4g(rows, ld);
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int64_t dmp_node_chain_blocks(int64_t tiles_bound) { return (int64_t)chain_blocks(tiles_bound); }
int64_t dmp_node_chain_panel_words(void) { return kChainPanelBytes / 4; }

int dmp_node_chain_pack(const dmp_chain_panel *panels, int num_panels, uint32_t *out, void *stream) {
  if (!panels || !out || num_panels < 1 || num_panels > kChainMaxPanels || !aligned16(out)) return DMP_ERR_BAD_ARG;
  PackArgs a{};
  for (int j = 0; j < num_panels; ++j) {
    if (!panels[j].W || panels[j].ld < 128) return DMP_ERR_BAD_ARG;
    a.W[j] = panels[j].W; a.ld[j] = panels[j].ld; a.transposed[j] = panels[j].transposed ? 1 : 0;
  }
  a.out = out;
  chain_pack_k<<<dim3(8, (unsigned)num_panels), 256, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

int dmp_node_chain_fwd(const float *x, int64_t ldx, const float *S, int64_t lds, const uint32_t *panels, const float *bn, const float *b2,
                       int residual, float slope, const int32_t *slot, const int32_t *num_tiles, int64_t tiles_bound, int64_t rows, int H,
                       float *H1n, int64_t ldh, float *P, int64_t ldp, float *xn, int64_t ldxn, void *stream) {
  if (H != 128 || g_exact_fp32) return DMP_ERR_UNSUPPORTED;
  if (rows < 0 || tiles_bound < 0) return DMP_ERR_BAD_ARG;
  if (!slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (rows == 0 || tiles_bound == 0) return DMP_OK;
  if (!panels || !bn || !b2 || !slot || !num_tiles || !aligned16(panels)) return DMP_ERR_BAD_ARG;
  if (!x || !S || !H1n || !P || !xn || ldx < H || lds < 2 * H || ldh < H || ldp < 2 * H || ldxn < H) return DMP_ERR_BAD_ARG;
  if (!chain_rows_ok(x, ldx, rows) || !chain_rows_ok(S, lds, rows) || !chain_rows_ok(H1n, ldh, rows) || !chain_rows_ok(P, ldp, rows) ||
      !chain_rows_ok(xn, ldxn, rows) || rows >= ((int64_t)1 << 30) || tiles_bound * kSub * 4 >= ((int64_t)1 << 32) - 8192)
    return DMP_ERR_UNSUPPORTED;
  if (!chain_lds_ready<false, true>()) return DMP_ERR_HIP;
  ChainArgs a{};
  a.A0 = x; a.lda0 = ldx; a.A1 = S; a.lda1 = lds; a.A2 = S + H; a.lda2 = lds;
  a.Res = residual ? x : nullptr; a.ldres = ldx; a.bias1 = bn; a.bias2 = b2;
  a.O0 = P; a.ldo0 = ldp; a.O1 = P + H; a.ldo1 = ldp; a.O2 = H1n; a.ldo2 = ldh; a.O3 = xn; a.ldo3 = ldxn;
  a.panels = panels; a.npanels = 6; a.slot = slot; a.num_tiles = num_tiles; a.rows = rows; a.slope = slope;
  node_chain_k<false, true><<<chain_blocks(tiles_bound), kChainThreads, kChainLdsBytes, (hipStream_t)stream>>>(a);
  return check_launch();
}

int dmp_node_chain_bwd(const float *dxn, int64_t ldd, const float *H1n, int64_t ldh, const float *dP, int64_t ldp, const uint32_t *panels,
                       int residual, float slope, const int32_t *slot, const int32_t *num_tiles, int64_t tiles_bound, int64_t rows, int H,
                       float *dPn, int64_t ldn, float *dS, int64_t lds, float *dx, int64_t ldx, float *partial, float *partial_rows,
                       void *stream) {
  if (H != 128 || g_exact_fp32) return DMP_ERR_UNSUPPORTED;
  if (rows < 0 || tiles_bound < 0) return DMP_ERR_BAD_ARG;
  if (!slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (!partial || !partial_rows) return DMP_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0 || tiles_bound == 0) {
    const size_t bytes = sizeof(float) * 128 * (size_t)chain_blocks(tiles_bound);
    if (hipMemsetAsync(partial, 0, bytes, st) != hipSuccess || hipMemsetAsync(partial_rows, 0, bytes, st) != hipSuccess) return DMP_ERR_HIP;
    return DMP_OK;
  }
  if (!panels || !slot || !num_tiles || !aligned16(panels)) return DMP_ERR_BAD_ARG;
  if (!dxn || !H1n || !dPn || !dS || ldd < H || ldh < H || ldn < H || lds < 2 * H || (dx && (!dP || ldp < 2 * H || ldx < H))) return DMP_ERR_BAD_ARG;
  if (!chain_rows_ok(dxn, ldd, rows) || !chain_rows_ok(H1n, ldh, rows) || !chain_rows_ok(dPn, ldn, rows) || !chain_rows_ok(dS, lds, rows) ||
      (dx && (!chain_rows_ok(dP, ldp, rows) || !chain_rows_ok(dx, ldx, rows))) || rows >= ((int64_t)1 << 30) ||
      tiles_bound * kSub * 4 >= ((int64_t)1 << 32) - 8192)
    return DMP_ERR_UNSUPPORTED;
  if (!(dx ? chain_lds_ready<true, true>() : chain_lds_ready<true, false>())) return DMP_ERR_HIP;
  ChainArgs a{};
  a.A0 = dxn; a.lda0 = ldd;
  a.A1 = dx ? dP : dxn; a.lda1 = dx ? ldp : ldd; a.A2 = dx ? dP + H : dxn; a.lda2 = a.lda1;      // (without dx: never read)
  a.X = H1n; a.ldx = ldh; a.Res = (dx && residual) ? dxn : nullptr; a.ldres = ldd;
  a.O0 = dPn; a.ldo0 = ldn; a.O1 = dS; a.ldo1 = lds; a.O2 = dS + H; a.ldo2 = lds; a.O3 = dx; a.ldo3 = ldx;
  a.partial = partial; a.partialA = partial_rows;
  a.panels = panels; a.npanels = dx ? 6 : 3; a.slot = slot; a.num_tiles = num_tiles; a.rows = rows; a.slope = slope;
  if (dx) node_chain_k<true, true><<<chain_blocks(tiles_bound), kChainThreads, kChainLdsBytes, st>>>(a);
  else node_chain_k<true, false><<<chain_blocks(tiles_bound), kChainThreads, kChainLdsBytes, st>>>(a);
  return check_launch();
}

}  // extern "C"
