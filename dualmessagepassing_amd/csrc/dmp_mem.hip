// Memory initialisation of the memory-attention heads and DIAMNet (SubgraphCountingMatching/models/pred.py:648-1328):
// every pair's padded rows pooled into M memory slots, the reference's per-pair Python loop (init_mem, pred.py:648-775)
// as one device-side pass.  Nothing is read back to the host, so a recorded training step can replay it.
//
// Per pair b (mask row [L], nonzero = live; rows x[b] [L, D]):
//   s = first live position, e = last live position (both 0 for a row with no live position: utils/dl.py:130-135);
//   n = e - s (memory-attention heads: the reference's slice ends AT e) or e - s + 1 (DIAMNet: pred.py:1188);
//   the segment is rows s .. s+n-1 as they are (masked interior rows included, each with its own mask bit);
//   circular: extended row p = segment row p mod n for p < n' = n + ceil((n+1)/2) - 1; otherwise n' = n;
//   n' <= M: slots 0 .. M-n'-1 are zero with mask 0, slot M-n'+q is extended row q with its mask bit;
//   n' >  M: stride = n' / M, k = n' - (M-1) stride, slot i pools extended rows i stride .. i stride + k - 1
//            (mean / sum / max per element; mask = OR of the window's bits; windows overlap when k > stride).
// Both cases are one form: slot i holds the window [q0_i, q0_i + k_i) of extended rows (k_i = 0 for an empty slot).
//
// Forward: grid (ceil(T M D/4 / 64), B), 4 waves per workgroup.  Lane j of every wave owns one (tensor, slot, 4-float
// column) item -- consecutive lanes take consecutive 16-byte columns of one row, so a wave step reads whole rows; wave r
// takes the window rows r, r+4, r+8, ... and the 4 partial results are combined in wave order through LDS (fixed order:
// bitwise reproducible).  s and e come from a scan of the pair's mask row by the workgroup.  T = 2 pools the key and the
// value memory of one MemDotAttention in the same launch (they share the mask, so they share the windows).
//
// Backward (gather form, no float atomics): one thread per (pair, row, 4-float column); segment row p is extended row p
// and, in circular mode, p + n; every window covering either position adds its share (mean dY/k, sum dY, max dY where the
// forward's first-maximum index is that extended position).  Rows outside the segment are written as zeros.
#include <climits>

#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kMemWaves = kBlock / kWave;   // row interleave of the forward

struct MemGeo {
  int s, n, np, stride, k;
};

__device__ __forceinline__ MemGeo mem_geo(int s, int n, int M, int circular) {
  MemGeo g;
  g.s = s;
  g.n = n;
  g.np = circular ? n + (n + 2) / 2 - 1 : n;
  g.stride = g.np > M ? g.np / M : 1;
  g.k = g.np > M ? g.np - (M - 1) * g.stride : 1;
  return g;
}

// the window of slot i: first extended row and row count
__device__ __forceinline__ void mem_window(const MemGeo &g, int M, int i, int &q0, int &kk) {
  if (g.np <= M) {
    q0 = i - (M - g.np);
    kk = q0 >= 0 ? 1 : 0;
  } else {
    q0 = i * g.stride;
    kk = g.k;
  }
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

struct MemFwdArgs {
  const float *X[2];
  int64_t ldx[2];
  float *Y[2];
  int32_t *arg[2];
  const uint8_t *mask;
  uint8_t *ymask;
  int32_t *seg;
  int64_t L;
  int D, M, T, mode, circular, inclusive;
};

__global__ __launch_bounds__(kBlock) void mem_init_fwd_kernel(MemFwdArgs a) {
  __shared__ int red_lo[kMemWaves], red_hi[kMemWaves];
  __shared__ float4 part[kMemWaves][kWave];
  __shared__ int4 part_q[kMemWaves][kWave];
  __shared__ int part_live[kMemWaves][kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t b = blockIdx.y;
  const uint8_t *mrow = a.mask + b * a.L;

  // s = first live position, e = last live position of the pair
  int lo = INT_MAX, hi = -1;
  for (int64_t l = tid; l < a.L; l += kBlock) {
    if (mrow[l]) {
      lo = min(lo, (int)l);
      hi = max(hi, (int)l);
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
  }
  if (lane == 0) { red_lo[wave] = lo; red_hi[wave] = hi; }
  __syncthreads();
  lo = red_lo[0];
  hi = red_hi[0];
#pragma unroll
  for (int w = 1; w < kMemWaves; ++w) { lo = min(lo, red_lo[w]); hi = max(hi, red_hi[w]); }
  const int s = hi < 0 ? 0 : lo, e = hi < 0 ? 0 : hi;
  const MemGeo g = mem_geo(s, a.inclusive ? e - s + 1 : e - s, a.M, a.circular);
  if (blockIdx.x == 0 && tid == 0) {
    a.seg[2 * b] = g.s;
    a.seg[2 * b + 1] = g.n;
  }

  const int D4 = a.D / 4;
  const int item = blockIdx.x * kWave + lane;
  const bool active = item < a.T * a.M * D4;
  const int c = active ? item % D4 : 0, ti = active ? item / D4 : 0;
  const int i = ti % a.M, t = ti / a.M;
  int q0, kk;
  mem_window(g, a.M, i, q0, kk);
  const float *X = a.X[t];
  const int64_t ldx = a.ldx[t];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int4 bq = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
  int live = 0;
  if (active) {
    if (a.mode == DMP_MEM_MAX) acc = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int j = wave; j < kk; j += kMemWaves) {
      const int q = q0 + j;
      const int row = g.s + (q < g.n ? q : q - g.n);      // q < n' < 2n
      const float4 v = ld4(X + (b * a.L + row) * ldx + 4 * c);
      live |= mrow[row];
      if (a.mode == DMP_MEM_MAX) {                         // first maximum in window order (F.max_pool1d)
        if (bq.x == INT_MAX || v.x > acc.x) { acc.x = v.x; bq.x = q; }
        if (bq.y == INT_MAX || v.y > acc.y) { acc.y = v.y; bq.y = q; }
        if (bq.z == INT_MAX || v.z > acc.z) { acc.z = v.z; bq.z = q; }
        if (bq.w == INT_MAX || v.w > acc.w) { acc.w = v.w; bq.w = q; }
      } else {
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
  }
  if (wave > 0) {
    part[wave][lane] = acc;
    part_q[wave][lane] = bq;
    part_live[wave][lane] = live;
  }
  __syncthreads();
  if (wave != 0 || !active) return;
#pragma unroll
  for (int w = 1; w < kMemWaves; ++w) {
    const float4 v = part[w][lane];
    const int4 vq = part_q[w][lane];
    live |= part_live[w][lane];
    if (a.mode == DMP_MEM_MAX) {
      if (vq.x != INT_MAX && (bq.x == INT_MAX || v.x > acc.x || (v.x == acc.x && vq.x < bq.x))) { acc.x = v.x; bq.x = vq.x; }
      if (vq.y != INT_MAX && (bq.y == INT_MAX || v.y > acc.y || (v.y == acc.y && vq.y < bq.y))) { acc.y = v.y; bq.y = vq.y; }
      if (vq.z != INT_MAX && (bq.z == INT_MAX || v.z > acc.z || (v.z == acc.z && vq.z < bq.z))) { acc.z = v.z; bq.z = vq.z; }
      if (vq.w != INT_MAX && (bq.w == INT_MAX || v.w > acc.w || (v.w == acc.w && vq.w < bq.w))) { acc.w = v.w; bq.w = vq.w; }
    } else {
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  if (kk == 0) {
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bq = make_int4(-1, -1, -1, -1);
  } else if (a.mode == DMP_MEM_MEAN) {
    const float f = (float)kk;
    acc.x /= f; acc.y /= f; acc.z /= f; acc.w /= f;
  }
  const int64_t o = (b * a.M + i) * a.D + 4 * c;
  *reinterpret_cast<float4 *>(a.Y[t] + o) = acc;
  if (a.mode == DMP_MEM_MAX) *reinterpret_cast<int4 *>(a.arg[t] + o) = bq;
  if (t == 0 && c == 0) a.ymask[b * a.M + i] = live ? 1 : 0;
}

struct MemBwdArgs {
  const float *dY[2];
  const int32_t *arg[2];
  float *dX[2];
  const int32_t *seg;
  int64_t B, L;
  int D, M, mode, circular;
};

__global__ __launch_bounds__(kBlock) void mem_init_bwd_kernel(MemBwdArgs a) {
  const int D4 = a.D / 4;
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int t = blockIdx.y;
  if (idx >= a.B * a.L * D4) return;
  const int c = (int)(idx % D4);
  const int64_t bl = idx / D4, b = bl / a.L;
  const int l = (int)(bl % a.L);
  const MemGeo g = mem_geo(a.seg[2 * b], a.seg[2 * b + 1], a.M, a.circular);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int p = l - g.s;
  if (p >= 0 && p < g.n) {
    const float *dY = a.dY[t] + b * a.M * a.D + 4 * c;
    const int32_t *arg = a.mode == DMP_MEM_MAX ? a.arg[t] + b * a.M * a.D + 4 * c : nullptr;
    for (int q = p; q < g.np; q += g.n) {                  // extended positions of this row: p, and p + n when circular
      if (g.np <= a.M) {
        const float4 d = ld4(dY + (a.M - g.np + q) * a.D);
        acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
        continue;
      }
      const int ilo = q - g.k + 1 <= 0 ? 0 : (q - g.k + g.stride) / g.stride;
      const int ihi = min(a.M - 1, q / g.stride);
      for (int i = ilo; i <= ihi; ++i) {
        const float4 d = ld4(dY + i * a.D);
        if (a.mode == DMP_MEM_MAX) {
          const int4 w = *reinterpret_cast<const int4 *>(arg + i * a.D);
          if (w.x == q) acc.x += d.x;
          if (w.y == q) acc.y += d.y;
          if (w.z == q) acc.z += d.z;
          if (w.w == q) acc.w += d.w;
        } else if (a.mode == DMP_MEM_MEAN) {
          const float f = (float)g.k;
          acc.x += d.x / f; acc.y += d.y / f; acc.z += d.z / f; acc.w += d.w / f;
        } else {
          acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
        }
      }
    }
  }
  *reinterpret_cast<float4 *>(a.dX[t] + bl * a.D + 4 * c) = acc;
}

bool mode_ok(int mode) { return mode == DMP_MEM_MEAN || mode == DMP_MEM_SUM || mode == DMP_MEM_MAX; }

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_mem_init_fwd(const float *X0, int64_t ldx0, const float *X1, int64_t ldx1, const uint8_t *mask, int64_t B, int64_t L, int D,
                     int M, int mode, int circular, int inclusive_end, float *Y0, float *Y1, uint8_t *ymask, int32_t *arg0,
                     int32_t *arg1, int32_t *seg, void *stream) {
  if (B < 0 || L < 1 || D < 4 || D % 4 || M < 1 || !mode_ok(mode)) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!X0 || !mask || !Y0 || !ymask || !seg || ldx0 < D || ldx0 % 4 || !aligned16(X0) || !aligned16(Y0)) return DMP_ERR_BAD_ARG;
  if (X1 && (!Y1 || ldx1 < D || ldx1 % 4 || !aligned16(X1) || !aligned16(Y1))) return DMP_ERR_BAD_ARG;
  if (mode == DMP_MEM_MAX && (!arg0 || !aligned16(arg0) || (X1 && (!arg1 || !aligned16(arg1))))) return DMP_ERR_BAD_ARG;
  if (L >= (int64_t)1 << 30 || B >= 65536 || (int64_t)M * D >= (int64_t)1 << 30) return DMP_ERR_UNSUPPORTED;
  MemFwdArgs a{{X0, X1 ? X1 : X0}, {ldx0, X1 ? ldx1 : ldx0}, {Y0, Y1}, {arg0, arg1}, mask, ymask, seg, L, D, M, X1 ? 2 : 1,
               mode, circular ? 1 : 0, inclusive_end ? 1 : 0};
  const int64_t items = (int64_t)a.T * M * (D / 4);
  hipLaunchKernelGGL(mem_init_fwd_kernel, dim3((unsigned)((items + kWave - 1) / kWave), (unsigned)B), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch();
}

int dmp_mem_init_bwd(const float *dY0, const float *dY1, const int32_t *arg0, const int32_t *arg1, const int32_t *seg, int64_t B,
                     int64_t L, int D, int M, int mode, int circular, float *dX0, float *dX1, void *stream) {
  if (B < 0 || L < 1 || D < 4 || D % 4 || M < 1 || !mode_ok(mode)) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!dY0 || !seg || !dX0 || !aligned16(dY0) || !aligned16(dX0)) return DMP_ERR_BAD_ARG;
  if (dY1 && (!dX1 || !aligned16(dY1) || !aligned16(dX1))) return DMP_ERR_BAD_ARG;
  if (mode == DMP_MEM_MAX && (!arg0 || !aligned16(arg0) || (dY1 && (!arg1 || !aligned16(arg1))))) return DMP_ERR_BAD_ARG;
  const int64_t n = B * L * (D / 4);
  if (L >= (int64_t)1 << 30 || (n + kBlock - 1) / kBlock >= ((int64_t)1 << 31)) return DMP_ERR_UNSUPPORTED;
  MemBwdArgs a{{dY0, dY1}, {arg0, arg1}, {dX0, dX1}, seg, B, L, D, M, mode, circular ? 1 : 0};
  hipLaunchKernelGGL(mem_init_bwd_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock), dY1 ? 2u : 1u), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
