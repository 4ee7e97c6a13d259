// The permutation product of an LRP / DMPLRP layer and its gradients WITHOUT the [P L L, in] matrix of gathered slot rows
// (lrp.py:66-73 / dmplrp.py:188-194: the einsum over the rows the two selection matrices pick).  gfx950.
//
//   out[p, :]  = sum_s row(slot[p, s]) W_s            row(t) = node_feat[t] (t < N), edge_feat[t - N] (t < N + E), else 0
//   dW_s       = sum_p row(slot[p, s])^T dOut[p]      W_s    = weight[:, :, s]   (weight [in, hid, L L], slot index innermost)
//   dTable[t]  = sum_{(p, s): slot[p, s] = t} dOut[p] W_s^T          (rows [0, N): d node_feat, rows [N, N + E): d edge_feat)
//
// Every kernel reads the feature rows in place; what is kept between them is [P, hid] and smaller.
//
// Panels.  A prologue (lrp_planes_k) splits the L L weight panels into their three bf16 planes once per launch, laid out so
// that a lane's MFMA fragment -- 8 consecutive k of one column -- is 16 consecutive bytes: [slot][plane][column][k].  The
// forward wants k = in, the table gradient k = hid: the entry asks for the orientation it needs.  The image (1.5 MB at L 4 and
// in = hid = 128) stays in L2; the tile kernels read their fragments from it.
//
// The tile kernel (lrp_tile_k) serves the forward and the table gradient: a workgroup owns 32 rows of the result (permutations
// / table rows), one wave per 32 columns; for every slot s that at least one of its rows fills it stages the 32 operand rows
// as bf16 planes in LDS -- split once by the staging thread -- and adds their product with panel s to ONE register tile per
// wave (six piece products, dmp_mfma_common.h "bf16x6": fp32-accurate).  The operand rows of the next filled slot are fetched
// while the MFMAs of this one run (two LDS images, one barrier per slot).  A slot none of the 32 rows fills is skipped: the
// permutations of a node are consecutive and share their empty slots.
//   forward         operand row r of slot s = row(slot[p0 + r, s])
//   table gradient  operand row r of slot s = sum of dOut[p] over the entries of key (t0 + r) L L + s of a CSR over those
//                   keys, in CSR order (ascending p; a row of kPoolLongRow entries or more: in contiguous shares, one per
//                   thread group, added in ascending share); a table row is written once, by one workgroup.
//
// The weight gradient (lrp_dw_k) is a gathered tall-skinny A^T B: workgroup (g, s) walks the g-th range of permutations 64 at
// a time, skips a group of 32 in which slot s is empty, stages the gathered rows and the dOut rows as fp32 in LDS, and every
// wave reads its fragments down the columns and splits them (as csrc/dmp_atb.hip does).  The per-range partials are added in
// ascending g by lrp_dw_reduce_k, which also writes the [in, hid, L L] layout.  No float atomics anywhere: two runs are
// bitwise equal.
#include "dmp_mfma_common.h"

namespace dmp {
namespace {

constexpr int kPoolRows = 32;                          // rows of a tile
constexpr int kPoolMaxL2 = DMP_LRP_MAX_SEQ_LEN * DMP_LRP_MAX_SEQ_LEN;
constexpr int kPoolIds = kPoolRows * kPoolMaxL2 + 1;   // slot ids / CSR offsets of a tile
constexpr int kPoolLongRow = 64;                       // entries of a (table row, slot) from which every thread group sums a share
constexpr int kDwMaxGroups = 16;                      // permutation ranges of the weight gradient
constexpr int kDwPermsPerGroup = 1024;                 // ... one per this many permutations

__host__ __device__ constexpr int pool_row_bytes(int K) { return 2 * K + 16; }     // an LDS row of one plane: 16 B of padding

// ---------------------------------------------------------------------------------------------------------------- the panels
// img[((s 3 + plane) NC + n) K + k] = plane of  transposed ? weight[n, k, s] : weight[k, n, s]
__global__ __launch_bounds__(kBlock) void lrp_planes_k(const float *__restrict__ weight, int IN, int HID, int L2, int transposed,
                                                       uint32_t *__restrict__ img) {
  const int K = transposed ? HID : IN, NC = transposed ? IN : HID, K2 = K / 2;
  const int64_t total = (int64_t)L2 * NC * K2;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int kp = (int)(idx % K2), n = (int)((idx / K2) % NC), s = (int)(idx / ((int64_t)K2 * NC));
  const int k = 2 * kp;
  const int64_t e0 = transposed ? ((int64_t)n * HID + k) * L2 + s : ((int64_t)k * HID + n) * L2 + s;
  const int64_t step = transposed ? (int64_t)L2 : (int64_t)HID * L2;       // to k + 1
  uint32_t h, m, l;
  split_pair(weight[e0], weight[e0 + step], h, m, l);
  const int64_t plane = (int64_t)NC * K2;                                  // 32-bit words of one plane of one slot
  uint32_t *o = img + ((int64_t)s * 3 * NC + n) * K2 + kp;
  o[0] = h;
  o[plane] = m;
  o[2 * plane] = l;
}

// ------------------------------------------------------------------------------------------------------------ the tile kernel
struct PoolTileArgs {
  const float *node, *edge;          // forward: the feature rows [N, K] / [E, K]
  const int64_t *slot;               // forward: [P L2]
  const int32_t *rowptr, *entp;      // table gradient: CSR over the keys t L2 + s ([R L2 + 1]) and the permutation of every entry
  const float *dout;                 // table gradient: [P, K]
  const uint32_t *img;               // the panels' planes, [L2][3][NC][K] bf16
  float *out;                        // forward: [P, NC]
  float *dnode, *dedge;              // table gradient: [N, NC] / [E, NC]
  int64_t rows;                      // rows of the result: P / N + E
  int N, E, L2;
};

template <int K, int NC, bool TABLE>
__global__ __launch_bounds__(64 * NC / 32) void lrp_tile_k(const PoolTileArgs a) {
  constexpr int T = 64 * NC / 32;                      // threads: one wave per 32 columns
  constexpr int C4 = K / 4;                            // float4 pieces of an operand row
  constexpr int RPP = T / C4;                          // rows staged per pass
  constexpr int NL = kPoolRows / RPP;                  // passes
  constexpr int RB = pool_row_bytes(K);
  constexpr int kPlane = kPoolRows * RB, kBuf = 3 * kPlane;
  __shared__ __attribute__((aligned(16))) unsigned char img_lds[2 * kBuf];
  __shared__ int ids[kPoolIds];
  __shared__ __attribute__((aligned(16))) float red[TABLE ? RPP * K : 4];      // the shares of a long row's sum
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, li = lane & 31, h = lane >> 5;
  const int srow = tid / C4, scol = tid % C4;
  const int L2 = a.L2;
  const int64_t r0 = (int64_t)blockIdx.x * kPoolRows;

  // ---- the tile's slot ids (forward: -1 = the zero row) / CSR offsets (table gradient: rows past the table are empty)
  if (!TABLE) {
    const int64_t first = r0 * L2, end = a.rows * L2;
    const int R = a.N + a.E;
    for (int i = tid; i < kPoolRows * L2; i += T) {
      const int64_t v = first + i < end ? a.slot[first + i] : -1;
      ids[i] = (v >= 0 && v < R) ? (int)v : -1;
    }
  } else {
    const int64_t first = r0 * L2, last = a.rows * L2;
    for (int i = tid; i <= kPoolRows * L2; i += T) ids[i] = a.rowptr[first + i < last ? first + i : last];
  }
  __syncthreads();
  unsigned long long mask = 0;                         // bit s: some row of the tile fills slot s (the same in every wave)
  for (int s = 0; s < L2; ++s) {
    const bool on = TABLE ? ids[li * L2 + s + 1] > ids[li * L2 + s] : ids[li * L2 + s] >= 0;
    if (__ballot(on) != 0ull) mask |= 1ull << s;
  }

  // table gradient: this thread's four columns of dOut summed over the CSR entries [j, e), in CSR order
  auto entry_sum = [&](int j, int e) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *col = a.dout + 4 * scol;
    for (; j + 8 <= e; j += 8) {                       // eight rows requested together (the loop is bound by their latency)
      int p[8];
      float4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = a.entp[j + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const float4 *>(col + (int64_t)p[u] * K);
#pragma unroll
      for (int u = 0; u < 8; ++u) { v.x += x[u].x; v.y += x[u].y; v.z += x[u].z; v.w += x[u].w; }
    }
    for (; j < e; ++j) {
      const float4 x = *reinterpret_cast<const float4 *>(col + (int64_t)a.entp[j] * K);
      v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
    }
    return v;
  };

  float4 pre[NL];
  auto fetch = [&](int s) {
#pragma unroll
    for (int m = 0; m < NL; ++m) {
      const int r = srow + RPP * m;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!TABLE) {
        const int t = ids[r * L2 + s];
        if (t >= 0) {
          const float *src = t < a.N ? a.node + (int64_t)t * K : a.edge + (int64_t)(t - a.N) * K;
          v = *reinterpret_cast<const float4 *>(src + 4 * scol);
        }
      } else {
        const int j = ids[r * L2 + s], e = ids[r * L2 + s + 1];
        if (e - j < kPoolLongRow) v = entry_sum(j, e);
      }
      pre[m] = v;
    }
    if (TABLE) {
      // a row with many entries (a hub's slot 0: every permutation of the node) is summed by ALL thread groups, group g the
      // g-th contiguous share of its entries, and the shares are added in ascending g by the row's own group: a fixed order.
      // The entry counts sit in LDS, so every thread sees the same long rows: the barriers are uniform.
      for (int r = 0; r < kPoolRows; ++r) {
        const int b = ids[r * L2 + s], e = ids[r * L2 + s + 1];
        if (e - b < kPoolLongRow) continue;
        const int q = (e - b + RPP - 1) / RPP;
        const int jb = min(b + srow * q, e), je = min(jb + q, e);
        *reinterpret_cast<float4 *>(&red[srow * K + 4 * scol]) = entry_sum(jb, je);
        __syncthreads();
        if (r % RPP == srow) {
          float4 t = *reinterpret_cast<const float4 *>(&red[4 * scol]);
#pragma unroll
          for (int g = 1; g < RPP; ++g) {
            const float4 x = *reinterpret_cast<const float4 *>(&red[g * K + 4 * scol]);
            t.x += x.x; t.y += x.y; t.z += x.z; t.w += x.w;
          }
#pragma unroll
          for (int m = 0; m < NL; ++m)
            if (srow + RPP * m == r) pre[m] = t;
        }
        __syncthreads();
      }
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int m = 0; m < NL; ++m) {
      uint2 ph, pm, pl;
      split_pair(pre[m].x, pre[m].y, ph.x, pm.x, pl.x);
      split_pair(pre[m].z, pre[m].w, ph.y, pm.y, pl.y);
      unsigned char *o = img_lds + buf * kBuf + (srow + RPP * m) * RB + 8 * scol;
      *reinterpret_cast<uint2 *>(o) = ph;
      *reinterpret_cast<uint2 *>(o + kPlane) = pm;
      *reinterpret_cast<uint2 *>(o + 2 * kPlane) = pl;
    }
  };

  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  if (mask != 0ull) {
    int s = __builtin_ctzll(mask);
    mask &= mask - 1;
    fetch(s);
    int buf = 0;
    for (;;) {
      stage(buf);
      lds_barrier();                                   // this slot's image is staged; everyone is done with the image before it
      const int cur = s;
      const bool more = mask != 0ull;
      if (more) {
        s = __builtin_ctzll(mask);
        mask &= mask - 1;
        fetch(s);
      }
      // fragments: A = LDS row li, k = 16 kg + 8 h ..; B = panel column 32 wave + li, the same k
      const unsigned char *arow = img_lds + buf * kBuf + li * RB + 16 * h;
      const uint32_t *bcol = a.img + ((int64_t)cur * 3 * NC + 32 * wave + li) * (K / 2) + 4 * h;
      constexpr int64_t kPanelPlane = (int64_t)NC * (K / 2);
#pragma unroll
      for (int kg = 0; kg < K / 16; ++kg) {
        Split8 fa, fb;
        fa.hi.v = *reinterpret_cast<const bf16x8 *>(arow + 32 * kg);
        fa.mid.v = *reinterpret_cast<const bf16x8 *>(arow + kPlane + 32 * kg);
        fa.lo.v = *reinterpret_cast<const bf16x8 *>(arow + 2 * kPlane + 32 * kg);
        fb.hi.v = *reinterpret_cast<const bf16x8 *>(bcol + 8 * kg);
        fb.mid.v = *reinterpret_cast<const bf16x8 *>(bcol + kPanelPlane + 8 * kg);
        fb.lo.v = *reinterpret_cast<const bf16x8 *>(bcol + 2 * kPanelPlane + 8 * kg);
        acc = mfma_x6(fa, fb, acc);
      }
      if (!more) break;
      buf ^= 1;
    }
  }

  // ---- accumulator g of lane (li, h): row (g & 3) + 8 (g >> 2) + 4 h, column 32 wave + li; every row is written once
  const int col = 32 * wave + li;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int64_t r = r0 + (g & 3) + 8 * (g >> 2) + 4 * h;
    if (r >= a.rows) continue;
    if (!TABLE) a.out[r * NC + col] = acc[g];
    else if (r < a.N) a.dnode[r * NC + col] = acc[g];
    else a.dedge[(r - a.N) * NC + col] = acc[g];
  }
}

// ------------------------------------------------------------------------------------------------------- the weight gradient
struct PoolDwArgs {
  const float *node, *edge;          // [N, IN] / [E, IN]
  const int64_t *slot;               // [P L2]
  const float *dout;                 // [P, HID]
  float *partial;                    // [gridDim.x][L2][IN][HID]
  int64_t P, chunk;                  // permutations of a range (a multiple of 64)
  int N, E, L2;
};

template <int IN, int HID>
__global__ __launch_bounds__(kBlock) void lrp_dw_k(const PoolDwArgs a) {
  constexpr int XS = IN + 4, DS = HID + 4;             // LDS row strides (floats): 16-byte rows, columns read conflict-free
  constexpr int CA = IN / 4, RA = kBlock / CA, NA = kPoolRows / RA;
  constexpr int CD = HID / 4, RD = kBlock / CD, ND = kPoolRows / RD;
  constexpr int NCB = HID / 32, WR = 4 / NCB, NB = (IN / 32) / WR;      // column blocks; waves down a column block; row blocks of a wave
  __shared__ __attribute__((aligned(16))) float X[kPoolRows * XS];
  __shared__ __attribute__((aligned(16))) float D[kPoolRows * DS];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, li = lane & 31, h = lane >> 5;
  const int s = blockIdx.y, L2 = a.L2, R = a.N + a.E;
  const int jb = wave % NCB, ib0 = wave / NCB;
  const int64_t begin = (int64_t)blockIdx.x * a.chunk;
  const int64_t end = begin + a.chunk < a.P ? begin + a.chunk : a.P;

  f32x16 acc[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[t][g] = 0.f;

  for (int64_t q0 = begin; q0 < end; q0 += 64) {
    // slot s of 64 permutations at a time: lane l holds permutation q0 + l's (every wave reads the same 64)
    int id = -1;
    if (q0 + lane < end) {
      const int64_t v = a.slot[(q0 + lane) * L2 + s];
      id = (v >= 0 && v < R) ? (int)v : -1;
    }
    const unsigned long long filled = __ballot(id >= 0);
    if (filled == 0ull) continue;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      if (((filled >> (32 * half)) & 0xFFFFFFFFull) == 0ull) continue;      // (uniform over the workgroup)
      const int64_t p0 = q0 + 32 * half;
      float4 pa[NA], pd[ND];
#pragma unroll
      for (int m = 0; m < NA; ++m) {
        const int r = tid / CA + RA * m;
        const int t = __shfl(id, 32 * half + r, kWave);
        pa[m] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0) {
          const float *src = t < a.N ? a.node + (int64_t)t * IN : a.edge + (int64_t)(t - a.N) * IN;
          pa[m] = *reinterpret_cast<const float4 *>(src + 4 * (tid % CA));
        }
      }
#pragma unroll
      for (int m = 0; m < ND; ++m) {
        const int64_t p = p0 + tid / CD + RD * m;
        pd[m] = p < end ? *reinterpret_cast<const float4 *>(a.dout + p * HID + 4 * (tid % CD)) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();                                 // everyone is done with the tile before
#pragma unroll
      for (int m = 0; m < NA; ++m) *reinterpret_cast<float4 *>(&X[(tid / CA + RA * m) * XS + 4 * (tid % CA)]) = pa[m];
#pragma unroll
      for (int m = 0; m < ND; ++m) *reinterpret_cast<float4 *>(&D[(tid / CD + RD * m) * DS + 4 * (tid % CD)]) = pd[m];
      __syncthreads();
      // the contraction over the tile's 32 permutations: two 16-deep k-groups; fragment element e of lane (li, h) = permutation 16 kg + 8 h + e
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        const float *dp = &D[(16 * kg + 8 * h) * DS + 32 * jb + li];
        Split8 fb;
        split8(make_float4(dp[0], dp[DS], dp[2 * DS], dp[3 * DS]), make_float4(dp[4 * DS], dp[5 * DS], dp[6 * DS], dp[7 * DS]), fb);
#pragma unroll
        for (int t = 0; t < NB; ++t) {
          const float *xp = &X[(16 * kg + 8 * h) * XS + 32 * (ib0 + WR * t) + li];
          Split8 fa;
          split8(make_float4(xp[0], xp[XS], xp[2 * XS], xp[3 * XS]), make_float4(xp[4 * XS], xp[5 * XS], xp[6 * XS], xp[7 * XS]), fa);
          acc[t] = mfma_x6(fa, fb, acc[t]);
        }
      }
    }
  }
  // accumulator (t, g): row (input column) 32 (ib0 + WR t) + (g & 3) + 8 (g >> 2) + 4 h, column (hidden) 32 jb + li
  float *out = a.partial + ((int64_t)blockIdx.x * L2 + s) * (IN * HID);
#pragma unroll
  for (int t = 0; t < NB; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g)
      out[(32 * (ib0 + WR * t) + (g & 3) + 8 * (g >> 2) + 4 * h) * HID + 32 * jb + li] = acc[t][g];
}

// dweight[(i HID + j) L2 + s] = sum_g partial[g][s][i][j], g ascending
__global__ __launch_bounds__(kBlock) void lrp_dw_reduce_k(const float *__restrict__ partial, int groups, int L2, int IH,
                                                          float *__restrict__ dweight) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (int64_t)L2 * IH) return;
  const int s = (int)(idx / IH), ij = (int)(idx % IH);
  float v = 0.f;
  for (int g = 0; g < groups; ++g) v += partial[((int64_t)g * L2 + s) * IH + ij];
  dweight[(int64_t)ij * L2 + s] = v;
}

inline int dw_groups(int64_t P) {
  const int64_t g = (P + kDwPermsPerGroup - 1) / kDwPermsPerGroup;
  return (int)(g < 1 ? 1 : (g > kDwMaxGroups ? kDwMaxGroups : g));
}
inline size_t plane_words(int in, int hid, int L2) { return (size_t)L2 * in * hid * 3 / 2; }

inline bool pool_shape_ok(int64_t P, int64_t N, int64_t E, int L) {
  const int64_t L2 = (int64_t)L * L;
  return P * L2 < ((int64_t)1 << 31) - 64 * L2 && (N + E + kPoolRows) * L2 + 1 < ((int64_t)1 << 31);
}

template <int K, int NC, bool TABLE>
void launch_tile(const PoolTileArgs &a, hipStream_t st) {
  const int64_t tiles = (a.rows + kPoolRows - 1) / kPoolRows;
  if (tiles > 0) hipLaunchKernelGGL((lrp_tile_k<K, NC, TABLE>), dim3((unsigned)tiles), dim3(64 * NC / 32), 0, st, a);
}

template <int IN, int HID>
void launch_dw(const PoolDwArgs &a, int groups, hipStream_t st) {
  hipLaunchKernelGGL((lrp_dw_k<IN, HID>), dim3((unsigned)groups, (unsigned)a.L2), dim3(kBlock), 0, st, a);
}

void launch_planes(const float *weight, int in, int hid, int L2, int transposed, uint32_t *img, hipStream_t st) {
  const int64_t total = (int64_t)L2 * in * hid / 2;
  hipLaunchKernelGGL(lrp_planes_k, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, weight, in, hid, L2, transposed, img);
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_lrp_pool_supported(int in, int hid, int L) {
  return (in == 64 || in == 128) && (hid == 64 || hid == 128) && L >= 1 && L <= DMP_LRP_MAX_SEQ_LEN;
}

size_t dmp_lrp_pool_workspace_words(int64_t P, int in, int hid, int L) {
  if (P < 0 || !dmp_lrp_pool_supported(in, hid, L)) return 0;
  return plane_words(in, hid, L * L) + (size_t)dw_groups(P) * L * L * in * hid;
}

int dmp_lrp_pool_fwd(const float *node_feat, const float *edge_feat, const float *weight, const int64_t *slot, int64_t P, int64_t N,
                     int64_t E, int in, int hid, int L, float *out, int32_t *ws, void *stream) {
  if (P < 0 || N < 0 || E < 0) return DMP_ERR_BAD_ARG;
  if (!dmp_lrp_pool_supported(in, hid, L) || !pool_shape_ok(P, N, E, L)) return DMP_ERR_UNSUPPORTED;
  if (P == 0) return DMP_OK;
  if (!weight || !slot || !out || !ws || (N > 0 && !node_feat) || (E > 0 && !edge_feat)) return DMP_ERR_BAD_ARG;
  if (!aligned16(node_feat) || !aligned16(edge_feat) || !aligned16(ws)) return DMP_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t *img = reinterpret_cast<uint32_t *>(ws);
  launch_planes(weight, in, hid, L * L, 0, img, st);
  PoolTileArgs a = {};
  a.node = node_feat; a.edge = edge_feat; a.slot = slot; a.img = img; a.out = out; a.rows = P;
  a.N = (int)N; a.E = (int)E; a.L2 = L * L;
  if (in == 64 && hid == 64) launch_tile<64, 64, false>(a, st);
  else if (in == 64) launch_tile<64, 128, false>(a, st);
  else if (hid == 64) launch_tile<128, 64, false>(a, st);
  else launch_tile<128, 128, false>(a, st);
  return check_launch();
}

int dmp_lrp_pool_bwd(const float *node_feat, const float *edge_feat, const float *weight, const int64_t *slot, const int32_t *rowptr,
                     const int32_t *entp, const float *dout, int64_t P, int64_t N, int64_t E, int in, int hid, int L, float *dnode,
                     float *dedge, float *dweight, int32_t *ws, void *stream) {
  if (P < 0 || N < 0 || E < 0) return DMP_ERR_BAD_ARG;
  if (!dmp_lrp_pool_supported(in, hid, L) || !pool_shape_ok(P, N, E, L)) return DMP_ERR_UNSUPPORTED;
  if (!dweight || (N > 0 && !dnode) || (E > 0 && !dedge)) return DMP_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int L2 = L * L;
  if (P == 0) {
    hipError_t e = hipMemsetAsync(dweight, 0, sizeof(float) * (size_t)in * hid * L2, st);
    if (e == hipSuccess && N > 0) e = hipMemsetAsync(dnode, 0, sizeof(float) * (size_t)N * in, st);
    if (e == hipSuccess && E > 0) e = hipMemsetAsync(dedge, 0, sizeof(float) * (size_t)E * in, st);
    if (e != hipSuccess) { set_last_hip_error(e); return DMP_ERR_HIP; }
    return DMP_OK;
  }
  if (!weight || !slot || !rowptr || !entp || !dout || !ws || (N > 0 && !node_feat) || (E > 0 && !edge_feat)) return DMP_ERR_BAD_ARG;
  if (!aligned16(node_feat) || !aligned16(edge_feat) || !aligned16(dout) || !aligned16(ws)) return DMP_ERR_BAD_ARG;
  uint32_t *img = reinterpret_cast<uint32_t *>(ws);
  float *partial = reinterpret_cast<float *>(ws) + plane_words(in, hid, L2);
  // ---- d node_feat / d edge_feat: rows [N + E, in] = staged dOut sums [., hid] times W_s^T (k = hid, columns = in)
  launch_planes(weight, in, hid, L2, 1, img, st);
  PoolTileArgs a = {};
  a.rowptr = rowptr; a.entp = entp; a.dout = dout; a.img = img; a.dnode = dnode; a.dedge = dedge; a.rows = N + E;
  a.N = (int)N; a.E = (int)E; a.L2 = L2;
  if (in == 64 && hid == 64) launch_tile<64, 64, true>(a, st);
  else if (in == 64) launch_tile<128, 64, true>(a, st);
  else if (hid == 64) launch_tile<64, 128, true>(a, st);
  else launch_tile<128, 128, true>(a, st);
  // ---- d weight
  const int groups = dw_groups(P);
  PoolDwArgs w = {};
  w.node = node_feat; w.edge = edge_feat; w.slot = slot; w.dout = dout; w.partial = partial; w.P = P;
  w.chunk = ((P + groups - 1) / groups + 63) / 64 * 64;
  w.N = (int)N; w.E = (int)E; w.L2 = L2;
  if (in == 64 && hid == 64) launch_dw<64, 64>(w, groups, st);
  else if (in == 64) launch_dw<64, 128>(w, groups, st);
  else if (hid == 64) launch_dw<128, 64>(w, groups, st);
  else launch_dw<128, 128>(w, groups, st);
  const int64_t total = (int64_t)L2 * in * hid;
  hipLaunchKernelGGL(lrp_dw_reduce_k, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, partial, groups, L2, in * hid, dweight);
  return check_launch();
}

}  // extern "C"
