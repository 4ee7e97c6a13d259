// The pooled prediction heads (SubgraphCountingMatching/models/pred.py:93-156 on per-graph sums, the node and the
// edge head of basemodel.py:1477-1498) as three launches for ALL heads: forward, backward over the rows, backward
// weight gradients.  The tensors are tiny ([B, 128..516], B = pairs per batch): the algebra is ~60 launches per
// step when done op by op, i.e. pure launch latency at the end of forward and the start of backward.
//
//   p = ps Wp^T + sp bp;  g = gs Wg^T + sg bg;  s = [pl, gl, 1/pl, 1/gl]
//   f = [p | g | g - p | g * p | s]  (4h + 4);  y1 = relu(f W1^T + b1);  y = [y1 | s] W2^T + b2
//
// h = input width = hidden width = 128 or 64.  fp32 MFMA products through LDS tiles (as csrc/dmp_fold.hip): 16 rows per
// workgroup, thread (r, cg) owns h / 16 consecutive columns of row r.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kThreads = 256, kRows = 16;
constexpr int kMaxHeads = DMP_HEADS_MAX;

// widths derived from the head's input = hidden width h (128, or the reference's shipped 64)
template <int kH> struct HeadGeom {
  static constexpr int kF = 4 * kH + 4, kYS = kH + 4;      // feature row [p | g | g - p | g * p | s], saved [y1 | s]
  static constexpr int kPad = kH + 4, kFPad = 4 * kH + 8;  // LDS row strides
  static constexpr int CW = kH / 16;                       // thread (r, cg) owns CW consecutive columns of row r
  static constexpr int NT = kH / 64, NKB = kH / 16;        // 16-column MFMA tiles per wave, k blocks of 16
};

__device__ __forceinline__ float4 ldg4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

struct Heads {
  dmp_head_weights w[kMaxHeads];
  dmp_head_io io[kMaxHeads];
  dmp_head_grads gr[kMaxHeads];
  int B;
  float slope;   // negative slope of the heads' activation (0 = ReLU; pred_act_func, pred.py:36)
};

// acc[CW] += A_lds[r][0..h-1] . op(W)[.., CW cg ..]   for one h-wide contraction; W element (j, k) at W[j * ldw + k]
//   wT = 1: out col j, contraction k: out[j] = sum_k a[k] W[j][k]     (x W^T, W in nn.Linear layout)
//   wT = 0: out col k, contraction j: out[k] = sum_j a[j] W[j][k]     (x W)
// A: the 16 operand rows in LDS (row i at A + i * lda, >= h values at stride 1, 16-byte aligned rows).
// The 16 x h product runs on the fp32 MFMA pipe (v_mfma_f32_16x16x4_f32: wave w owns output columns (h/4) w .. (h/4)(w+1) - 1):
// every lane requests its share of the whole h-deep weight panel in ONE batch of loads straight in the operand layout
// (one L2 round trip per product instead of one per 32-deep LDS slice), the A operand comes from LDS as float4 (lane
// (m, kq) takes k = 16 kb + 4 kq .. + 3, the weights follow the same order); the 16 x h result goes through Ws
// (>= 16 * kPad floats) into the (row r = tid / 16, CW columns cg) accumulators of the callers' epilogues.
template <int kH>
__device__ __forceinline__ void gemm_h(float (&acc)[kH / 16], const float *A, int lda, const float *W, int ldw, int wT, int wcol0,
                                       float *Ws, int tid, int cg) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  constexpr int kPad = HeadGeom<kH>::kPad, CW = HeadGeom<kH>::CW, NT = HeadGeom<kH>::NT, NKB = HeadGeom<kH>::NKB;
  const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  float4 bw[NT][NKB];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = wave * (16 * NT) + t * 16 + m;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int k = kb * 16 + 4 * kq;
      if (wT) {
        bw[t][kb] = ldg4(W + (int64_t)n * ldw + wcol0 + k);
      } else {
        const float *c = W + (int64_t)k * ldw + wcol0 + n;
        bw[t][kb] = make_float4(c[0], c[ldw], c[2 * (int64_t)ldw], c[3 * (int64_t)ldw]);
      }
    }
  }
  __syncthreads();                                          // the callers' operand rows are in LDS; Ws is free again
  f32x4 d[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) d[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const float4 a = *reinterpret_cast<const float4 *>(A + m * lda + kb * 16 + 4 * kq);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bw[t][kb].x, d[t], 0, 0, 0);
      d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bw[t][kb].y, d[t], 0, 0, 0);
      d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bw[t][kb].z, d[t], 0, 0, 0);
      d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bw[t][kb].w, d[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) Ws[(4 * kq + i) * kPad + wave * (16 * NT) + t * 16 + m] = d[t][i];
  __syncthreads();
  const int r = tid >> 4;
#pragma unroll
  for (int v = 0; v < CW / 4; ++v) {
    const float4 o = *reinterpret_cast<const float4 *>(&Ws[r * kPad + cg * CW + 4 * v]);
    acc[4 * v] += o.x; acc[4 * v + 1] += o.y; acc[4 * v + 2] += o.z; acc[4 * v + 3] += o.w;
  }
}

template <int kH>
__device__ __forceinline__ void stage_rows(float *As, const float *X, int64_t ldx, int i0, int B, int tid) {
  constexpr int kQ = kH / 4, kPass = kThreads / kQ;
#pragma unroll
  for (int m = 0; m < kRows / kPass; ++m) {
    const int row = tid / kQ + kPass * m, c4 = (tid % kQ) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i0 + row < B) a = ldg4(X + (int64_t)(i0 + row) * ldx + c4);
    *reinterpret_cast<float4 *>(&As[row * HeadGeom<kH>::kPad + c4]) = a;
  }
}

// CW consecutive floats of a thread's row: registers -> memory
template <int CW>
__device__ __forceinline__ void store_cw(float *o, const float (&v)[CW]) {
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) *reinterpret_cast<float4 *>(o + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

template <int kH>
__global__ __launch_bounds__(kThreads) void heads_fwd_k(const Heads t) {
  constexpr int kF = HeadGeom<kH>::kF, kYS = HeadGeom<kH>::kYS, kPad = HeadGeom<kH>::kPad, kFPad = HeadGeom<kH>::kFPad, CW = HeadGeom<kH>::CW;
  __shared__ float As[kRows * kPad];
  __shared__ float Fs[kRows * kFPad];
  __shared__ float Ws[16 * kPad];
  const dmp_head_weights &w = t.w[blockIdx.y];
  const dmp_head_io &io = t.io[blockIdx.y];
  const int tid = threadIdx.x, r = tid >> 4, cg = tid & 15, i0 = (int)blockIdx.x * kRows, b = i0 + r;
  const bool live = b < t.B;
  float p[CW], g[CW];
  // p = ps Wp^T + sp bp,  g = gs Wg^T + sg bg
#pragma unroll
  for (int e = 0; e < CW; ++e) { p[e] = 0.f; g[e] = 0.f; }
  stage_rows<kH>(As, io.ps, io.ld_ps, i0, t.B, tid);
  gemm_h<kH>(p, As, kPad, w.Wp, kH, 1, 0, Ws, tid, cg);
  __syncthreads();
  stage_rows<kH>(As, io.gs, io.ld_gs, i0, t.B, tid);
  gemm_h<kH>(g, As, kPad, w.Wg, kH, 1, 0, Ws, tid, cg);
#pragma unroll
  for (int e = 0; e < CW; ++e) {
    p[e] += io.scale_p * w.bp[cg * CW + e];
    g[e] += io.scale_g * w.bg[cg * CW + e];
  }
  // f = [p | g | g - p | g * p | s]
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) { s4[0] = io.pl[b]; s4[1] = io.gl[b]; s4[2] = 1.0f / s4[0]; s4[3] = 1.0f / s4[1]; }
#pragma unroll
  for (int e = 0; e < CW; ++e) {
    const int c = cg * CW + e;
    Fs[r * kFPad + c] = p[e];
    Fs[r * kFPad + kH + c] = g[e];
    Fs[r * kFPad + 2 * kH + c] = g[e] - p[e];
    Fs[r * kFPad + 3 * kH + c] = g[e] * p[e];
  }
  if (cg < 4) Fs[r * kFPad + 4 * kH + cg] = s4[cg];
  __syncthreads();
  if (live) {
    float *F = io.F + (int64_t)b * kF;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int v = 0; v < CW / 4; ++v)
        *reinterpret_cast<float4 *>(F + q * kH + cg * CW + 4 * v) = *reinterpret_cast<const float4 *>(&Fs[r * kFPad + q * kH + cg * CW + 4 * v]);
    if (cg < 4) F[4 * kH + cg] = s4[cg];
  }
  // y1 = act(f W1^T + b1): four h-wide contractions + the four scalars
  float y1[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) y1[e] = w.b1[cg * CW + e];
#pragma unroll 1
  for (int q = 0; q < 4; ++q) gemm_h<kH>(y1, Fs + q * kH, kFPad, w.W1, kF, 1, q * kH, Ws, tid, cg);
#pragma unroll
  for (int e = 0; e < CW; ++e) {
    const float *wr = w.W1 + (int64_t)(cg * CW + e) * kF + 4 * kH;
    y1[e] += s4[0] * wr[0] + s4[1] * wr[1] + s4[2] * wr[2] + s4[3] * wr[3];
    y1[e] = act_fwd(y1[e], t.slope);
  }
  // y = [y1 | s] W2^T + b2
  float part = 0.f;
#pragma unroll
  for (int e = 0; e < CW; ++e) part += y1[e] * w.W2[cg * CW + e];
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) part += __shfl_xor(part, off, 16);
  if (live) {
    float *ys = io.Y1S + (int64_t)b * kYS;
    store_cw<CW>(ys + cg * CW, y1);
    if (cg < 4) ys[kH + cg] = s4[cg];
    if (cg == 0)
      io.y[b] = part + s4[0] * w.W2[kH] + s4[1] * w.W2[kH + 1] + s4[2] * w.W2[kH + 2] + s4[3] * w.W2[kH + 3] + w.b2[0];
  }
}

// Backward over the rows: dy -> dy1 (activation mask) -> df = dy1 W1 -> dp, dg -> dps = dp Wp, dgs = dg Wg.
// Writes what the weight gradients need (dY1, dP, dG) and the input gradients.
template <int kH>
__global__ __launch_bounds__(kThreads) void heads_bwd_rows_k(const Heads t) {
  constexpr int kF = HeadGeom<kH>::kF, kYS = HeadGeom<kH>::kYS, kPad = HeadGeom<kH>::kPad, CW = HeadGeom<kH>::CW;
  __shared__ float As[kRows * kPad];
  __shared__ float Ws[16 * kPad];
  const dmp_head_weights &w = t.w[blockIdx.y];
  const dmp_head_io &io = t.io[blockIdx.y];
  const dmp_head_grads &gr = t.gr[blockIdx.y];
  const int tid = threadIdx.x, r = tid >> 4, cg = tid & 15, i0 = (int)blockIdx.x * kRows, b = i0 + r;
  const bool live = b < t.B;
  const float dy = live ? gr.dy[b] * (gr.dy_scale ? gr.dy_scale[b] : 1.0f) : 0.f;
  // dy1 = y1 > 0 ? dy W2 : slope * dy W2
  float d1[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) {
    const float y1 = live ? io.Y1S[(int64_t)b * kYS + cg * CW + e] : 0.f;
    d1[e] = act_bwd(y1, dy * w.W2[cg * CW + e], t.slope);
    As[r * kPad + cg * CW + e] = d1[e];
  }
  if (live) store_cw<CW>(gr.dY1 + (int64_t)b * kH + cg * CW, d1);
  // df blocks: [dfp | dfg | dfd | dfm] = dy1 W1[:, 0:4h]
  float df[4][CW];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int e = 0; e < CW; ++e) df[q][e] = 0.f;
    gemm_h<kH>(df[q], As, kPad, w.W1, kF, 0, q * kH, Ws, tid, cg);
  }
  float dp[CW], dg[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) {
    const float p = live ? io.F[(int64_t)b * kF + cg * CW + e] : 0.f;
    const float g = live ? io.F[(int64_t)b * kF + kH + cg * CW + e] : 0.f;
    dp[e] = (df[0][e] - df[2][e]) + df[3][e] * g;
    dg[e] = (df[1][e] + df[2][e]) + df[3][e] * p;
  }
  if (live) {
    store_cw<CW>(gr.dP + (int64_t)b * kH + cg * CW, dp);
    store_cw<CW>(gr.dG + (int64_t)b * kH + cg * CW, dg);
  }
  // input gradients: dps = dp Wp, dgs = dg Wg
  float out[CW];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < CW; ++e) { As[r * kPad + cg * CW + e] = dp[e]; out[e] = 0.f; }
  gemm_h<kH>(out, As, kPad, w.Wp, kH, 0, 0, Ws, tid, cg);
  if (live && gr.dps) store_cw<CW>(gr.dps + (int64_t)b * gr.ld_dps + cg * CW, out);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < CW; ++e) { As[r * kPad + cg * CW + e] = dg[e]; out[e] = 0.f; }
  gemm_h<kH>(out, As, kPad, w.Wg, kH, 0, 0, Ws, tid, cg);
  if (live && gr.dgs) store_cw<CW>(gr.dgs + (int64_t)b * gr.ld_dgs + cg * CW, out);
}

// Weight gradients: out[j, k] = sum_i dC[i, j] M[i, k]  (j < nj <= 128, k < ncols), bias[j] = bscale * sum_i dC[i, j].
// One workgroup per (job, 16 output rows, 16 output columns) on the fp32 MFMA pipe (v_mfma_f32_16x16x4_f32 contracts four
// batch rows per instruction): the four waves take interleaved groups of four batch rows, every lane requests its A / B
// operands of kSteps instructions in one batch straight in the operand layout, a batch ahead of the one being
// multiplied (B = 1024: four dependent L2 round trips per workgroup instead of sixteen staged 64-row chunks), and the
// four partial tiles meet in LDS.
struct WJob { const float *dC; const float *M; const float *row_scale; float *out; float *bias; int64_t ldc, ldm; int nj, ncols, ldo; float bscale; };
constexpr int kMaxWJobs = 4 * kMaxHeads;
struct WJobs { WJob job[kMaxWJobs]; int blk0[kMaxWJobs + 1]; int n; int B; };
constexpr int kColW = 16, kSteps = 16;

__global__ __launch_bounds__(kThreads) void heads_bwd_w_k(const WJobs t) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __shared__ float red[4 * 16 * 17];
  __shared__ float bred[4 * 64];
  int q = 0;
  while (q + 1 < t.n && (int)blockIdx.x >= t.blk0[q + 1]) ++q;
  const WJob &jb = t.job[q];
  const int kblocks = (jb.ncols + kColW - 1) / kColW;
  const int sub = (int)blockIdx.x - t.blk0[q];
  const int j0 = (sub / kblocks) * kRows, k0 = (sub % kblocks) * kColW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  const bool a_on = j0 + m < jb.nj, b_on = k0 + m < jb.ncols;
  const float *ap = jb.dC + j0 + m, *bp = jb.M + k0 + m;
  const int groups = (t.B + 3) / 4;                         // groups of four batch rows; wave w takes w, w + 4, ...
  float an[kSteps], sn[kSteps], bn[kSteps];
  auto fetch = [&](int g0) {
#pragma unroll
    for (int st = 0; st < kSteps; ++st) {
      const int64_t i = 4 * (int64_t)(g0 + wave + 4 * st) + kq;
      const bool in = i < t.B;
      an[st] = (in && a_on) ? ap[i * jb.ldc] : 0.f;
      sn[st] = (in && jb.row_scale) ? jb.row_scale[i] : 1.0f;
      bn[st] = (in && b_on) ? bp[i * jb.ldm] : 0.f;
    }
  };
  f32x4 d = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  fetch(0);
  for (int g0 = 0; g0 < groups; g0 += 4 * kSteps) {
    float a[kSteps], b[kSteps];
#pragma unroll
    for (int st = 0; st < kSteps; ++st) { a[st] = an[st] * sn[st]; b[st] = bn[st]; }
    if (g0 + 4 * kSteps < groups) fetch(g0 + 4 * kSteps);
#pragma unroll
    for (int st = 0; st < kSteps; ++st) {
      d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st], b[st], d, 0, 0, 0);
      bsum += a[st];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[(wave * 16 + 4 * kq + i) * 17 + m] = d[i];
  bred[wave * 64 + lane] = bsum;
  __syncthreads();
  const int jr = tid >> 4, kc = tid & 15;
  if (j0 + jr < jb.nj && k0 + kc < jb.ncols)
    jb.out[(int64_t)(j0 + jr) * jb.ldo + k0 + kc] =
        (red[(0 * 16 + jr) * 17 + kc] + red[(1 * 16 + jr) * 17 + kc]) + (red[(2 * 16 + jr) * 17 + kc] + red[(3 * 16 + jr) * 17 + kc]);
  if (jb.bias && k0 == 0 && tid < 16 && j0 + tid < jb.nj) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int c = 0; c < 4; ++c) sum += bred[w * 64 + c * 16 + tid];
    jb.bias[j0 + tid] = jb.bscale * sum;
  }
}

struct BlendArgs { const float *y[kMaxHeads]; const float *gl[kMaxHeads]; float *w[kMaxHeads]; float *out; int n, B; };
__global__ __launch_bounds__(kThreads) void heads_blend_k(const BlendArgs a) {
  const int b = (int)blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.B) return;
  float total = a.gl[0][b];
  for (int i = 1; i < a.n; ++i) total = total + a.gl[i][b];
  float out = 0.f;
  for (int i = 0; i < a.n; ++i) {
    const float w = a.gl[i][b] / total;
    a.w[i][b] = w;
    const float term = __fmul_rn(a.y[i][b], w);             // separate multiply and add, as the op-by-op blend rounds
    out = i == 0 ? term : __fadd_rn(out, term);
  }
  a.out[b] = out;
}

inline void add_wjob(WJobs &t, int &blocks, const float *dC, int64_t ldc, int nj, const float *row_scale, const float *M,
                     int64_t ldm, int ncols, float *out, int ldo, float *bias, float bscale) {
  WJob &j = t.job[t.n];
  j.dC = dC; j.ldc = ldc; j.nj = nj; j.row_scale = row_scale; j.M = M; j.ldm = ldm; j.ncols = ncols; j.out = out; j.ldo = ldo;
  j.bias = bias; j.bscale = bscale;
  t.blk0[t.n] = blocks;
  blocks += ((nj + kRows - 1) / kRows) * ((ncols + kColW - 1) / kColW);
  t.n += 1;
  t.blk0[t.n] = blocks;
}

inline bool ok16p(const void *q) { return q && (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

bool heads_valid(const dmp_head_weights *w, const dmp_head_io *io, int n, int B, int H) {
  const int kH = H;
  if (n < 1 || n > kMaxHeads || B < 0 || (H != 128 && H != 64) || !w || !io) return false;
  for (int i = 0; i < n; ++i) {
    if (!ok16p(w[i].Wp) || !ok16p(w[i].bp) || !ok16p(w[i].Wg) || !ok16p(w[i].bg) || !ok16p(w[i].W1) || !ok16p(w[i].b1) ||
        !ok16p(w[i].W2) || !w[i].b2)
      return false;
    if (!ok16p(io[i].ps) || !ok16p(io[i].gs) || !io[i].pl || !io[i].gl || !ok16p(io[i].F) || !ok16p(io[i].Y1S) || !io[i].y ||
        io[i].ld_ps < kH || io[i].ld_gs < kH || io[i].ld_ps % 4 || io[i].ld_gs % 4)
      return false;
  }
  return true;
}

// The count loss of a training step and its seed in ONE launch (train.py:624-628: bp_crit(leaky_relu(pred_c, slope), counts) with
// reduction 'mean', then loss.backward()): around a thousand numbers, five torch launches (criterion, mean, two fills, the
// criterion's backward).  One workgroup: loss[0] = mean_i crit(act(pred_i) - target_i), dpred[i] = d loss / d pred_i; fixed
// summation order (thread-strided partial sums, a tree over the threads): the same bits on every launch.
//   kind 0: MSE d^2      1: MAE |d|      2: smooth L1 (beta 1): d^2 / 2 inside |d| < 1, |d| - 1/2 outside
constexpr int kLossThreads = 1024;
__global__ __launch_bounds__(kLossThreads) void count_loss_k(const float *__restrict__ pred, const float *__restrict__ target, int64_t n,
                                                             int kind, float slope, float *__restrict__ loss, float *__restrict__ dpred) {
  __shared__ float red[kLossThreads];
  const float inv_n = 1.f / (float)n;
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kLossThreads) {
    const float p = pred[i];
    const float da = p > 0.f ? 1.f : slope;                  // leaky_relu'(p) (torch: the negative slope at p <= 0)
    const float d = p * da - target[i];
    float v, g;
    if (kind == 0) { v = d * d; g = 2.f * d; }
    else if (kind == 1) { v = fabsf(d); g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    else { const float a = fabsf(d); v = a < 1.f ? 0.5f * d * d : a - 0.5f; g = a < 1.f ? d : (d > 0.f ? 1.f : -1.f); }
    acc += v;
    dpred[i] = g * da * inv_n;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kLossThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] * inv_n;
}

// ------------------------------------------------------------------ the pooled last layer's per-graph algebra
// The turn-around of a step whose last layer hands out per-graph sums only (fused._pooled_outputs, _edge_out_bwd_lazy): the
// second level of the pooled sums (chunk -> graph), the [G, h] x [h, h] products with the second Linear's weight and the two
// parameter gradients, on arrays of a few thousand rows -- three launches on the tiles above instead of nine dependent ones
// (segment sums, library products, a row pass) of 5 .. 16 us each.  fp32 throughout.
constexpr int kWgGraphs = 32;     // graphs per workgroup of pool_wgrad_k: its rows in LDS -> one [h, h + 1] partial

// A thread's CW columns (from `col`) of one graph's second-level sum: the rows `gent[p] >> 1` of the chunk table, p =
// gptr[g] .. gptr[g + 1] - 1, added one by one from zero in that order -- the order and the bits of seg_sum_vec over the same
// CSR.  Four rows are requested together.  (An entry outside the table's V rows is left out, never read.)  `part2` (may be
// NULL; block-uniform): a second table of the same shape over the same CSR into `acc2`, its rows requested with the first's.
template <int CW>
__device__ __forceinline__ void chunk_sum(float (&acc)[CW], float (&acc2)[CW], const float *part, const float *part2, int64_t ld,
                                          int64_t V, const int32_t *gptr, const int32_t *gent, int64_t g, int col) {
  constexpr int U = 4;
#pragma unroll
  for (int e = 0; e < CW; ++e) { acc[e] = 0.f; acc2[e] = 0.f; }
  const int beg = gptr[g], end = gptr[g + 1];
  for (int p = beg; p < end; p += U) {
    float4 v[U][CW / 4], v2[U][CW / 4];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ok[u] = false;
      if (p + u < end) {
        const int64_t ch = gent[p + u] >> 1;
        ok[u] = ch >= 0 && ch < V;
        if (ok[u]) {
#pragma unroll
          for (int q = 0; q < CW / 4; ++q) v[u][q] = ldg4(part + ch * ld + col + 4 * q);
          if (part2) {
#pragma unroll
            for (int q = 0; q < CW / 4; ++q) v2[u][q] = ldg4(part2 + ch * ld + col + 4 * q);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (ok[u]) {
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) {
          acc[4 * q] += v[u][q].x; acc[4 * q + 1] += v[u][q].y; acc[4 * q + 2] += v[u][q].z; acc[4 * q + 3] += v[u][q].w;
        }
        if (part2) {
#pragma unroll
          for (int q = 0; q < CW / 4; ++q) {
            acc2[4 * q] += v2[u][q].x; acc2[4 * q + 1] += v2[u][q].y; acc2[4 * q + 2] += v2[u][q].z; acc2[4 * q + 3] += v2[u][q].w;
          }
        }
      }
    }
  }
}

struct PoolOut {
  const float *partH, *partZ, *partX, *gcnt, *W2, *b2;
  const int32_t *gptr, *gent, *ngptr, *ngent;
  float *es, *vs, *Q;
  int64_t ldh, V, Vn;
  int G, Gn, halves, eblocks;
};

// Forward.  Workgroups 0 .. eblocks - 1, 16 graphs each: Q = the non-flagged half of the chunk sums of g (.) H1, summed per
// graph;  es = sum of z's chunk sums + Q W2^T + gcnt[:, 0] b2.  The workgroups after them: vs = the node chunk sums per graph.
template <int kH>
__global__ __launch_bounds__(kThreads) void pool_out_k(const PoolOut a) {
  constexpr int kPad = HeadGeom<kH>::kPad, CW = HeadGeom<kH>::CW;
  __shared__ float As[kRows * kPad];
  __shared__ float Ws[16 * kPad];
  const int tid = threadIdx.x, r = tid >> 4, cg = tid & 15, col = cg * CW;
  float q[CW], zs[CW];
  if ((int)blockIdx.x >= a.eblocks) {
    const int64_t g = (int64_t)((int)blockIdx.x - a.eblocks) * kRows + r;
    if (g >= a.Gn) return;
    chunk_sum<CW>(q, zs, a.partX, nullptr, kH, a.Vn, a.ngptr, a.ngent, g, col);
    store_cw<CW>(a.vs + g * kH + col, q);
    return;
  }
  const int64_t g = (int64_t)blockIdx.x * kRows + r;
  const bool live = g < a.G;
#pragma unroll
  for (int e = 0; e < CW; ++e) { q[e] = 0.f; zs[e] = 0.f; }
  // (both tables' rows in one walk of the CSR: the residual term's loads do not wait behind the product)
  if (live) chunk_sum<CW>(q, zs, a.partH, a.partZ, a.ldh, a.V, a.gptr, a.gent, g, col);
  const float cnt = (live && a.b2) ? a.gcnt[g * a.halves] : 0.f;
  store_cw<CW>(&As[r * kPad + col], q);
  if (live && a.Q) store_cw<CW>(a.Q + g * kH + col, q);
  float es[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) es[e] = 0.f;
  gemm_h<kH>(es, As, kPad, a.W2, kH, 1, 0, Ws, tid, cg);
  if (!live) return;
  if (a.partZ) {
#pragma unroll
    for (int e = 0; e < CW; ++e) es[e] = zs[e] + es[e];
  }
  if (a.b2) {
#pragma unroll
    for (int e = 0; e < CW; ++e) es[e] += cnt * a.b2[col + e];
  }
  store_cw<CW>(a.es + g * kH + col, es);
}

// out = A op(W): a plain [rows, h] x [h, h] product, 16 rows per workgroup (wT as gemm_h's).
template <int kH>
__global__ __launch_bounds__(kThreads) void rows_gemm_k(const float *__restrict__ A, int64_t lda, int rows, const float *__restrict__ W, int wT,
                                                        float *__restrict__ out, int64_t ldo) {
  constexpr int kPad = HeadGeom<kH>::kPad, CW = HeadGeom<kH>::CW;
  __shared__ float As[kRows * kPad];
  __shared__ float Ws[16 * kPad];
  const int tid = threadIdx.x, r = tid >> 4, cg = tid & 15, i0 = (int)blockIdx.x * kRows;
  float acc[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) acc[e] = 0.f;
  stage_rows<kH>(As, A, lda, i0, rows, tid);
  gemm_h<kH>(acc, As, kPad, W, kH, wT, 0, Ws, tid, cg);
  if (i0 + r < rows) store_cw<CW>(out + (int64_t)(i0 + r) * ldo + cg * CW, acc);
}

struct PoolWgrad {
  const float *qc, *T, *gcnt;
  const int32_t *gptr, *gent;
  float *part, *Q;
  int64_t ldq, ldt, V;
  int G, halves;
};

// Backward, after pool_relu_bwd.  A workgroup owns kWgGraphs graphs: their Q rows (the non-flagged half of the chunk sums qc,
// per graph; thread (r, cg) sums h / 8 columns of row r) and T rows go to LDS, then  dW2 = T^T Q  (MFMA: A = T^T, the
// contraction runs over the graphs; wave w owns the output rows (h/4) w ..) and  db2 = sum_g gcnt[g, 0] T[g], graphs ascending.
// Its partial [h * h | h] is one row of `part`: no atomics, dmp_reduce_partials adds the workgroups' rows.
template <int kH>
__global__ __launch_bounds__(kThreads) void pool_wgrad_k(const PoolWgrad a) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  constexpr int CW = kH / 8, JT = kH / 64, KT = kH / 16;
  constexpr int kWPad = kH + 16;      // the MFMA operands are read down a column: the four rows of a k step in disjoint banks
  __shared__ float Ts[kWgGraphs * kWPad];
  __shared__ float Qs[kWgGraphs * kWPad];
  __shared__ float Cs[kWgGraphs];
  const int tid = threadIdx.x, r = tid >> 3, cg = tid & 7, col = cg * CW;
  const int lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  const int64_t g = (int64_t)blockIdx.x * kWgGraphs + r;
  const bool live = g < a.G;
  float q[CW], tv[CW], unused[CW];
#pragma unroll
  for (int e = 0; e < CW; ++e) { q[e] = 0.f; tv[e] = 0.f; }
  if (live) {
#pragma unroll
    for (int v = 0; v < CW / 4; ++v) {
      const float4 t4 = ldg4(a.T + g * a.ldt + col + 4 * v);
      tv[4 * v] = t4.x; tv[4 * v + 1] = t4.y; tv[4 * v + 2] = t4.z; tv[4 * v + 3] = t4.w;
    }
    if (cg == 0) Cs[r] = a.gcnt[g * a.halves];
    chunk_sum<CW>(q, unused, a.qc, nullptr, a.ldq, a.V, a.gptr, a.gent, g, col);
    if (a.Q) store_cw<CW>(a.Q + g * kH + col, q);
  } else if (cg == 0) {
    Cs[r] = 0.f;
  }
  store_cw<CW>(&Qs[r * kWPad + col], q);
  store_cw<CW>(&Ts[r * kWPad + col], tv);
  __syncthreads();
  f32x4 d[JT][KT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) d[jt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < kWgGraphs / 4; ++s) {
    const int row = (4 * s + kq) * kWPad;
    float av[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) av[jt] = Ts[row + (wave * JT + jt) * 16 + m];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const float b = Qs[row + kt * 16 + m];
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) d[jt][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[jt], b, d[jt][kt], 0, 0, 0);
    }
  }
  float *P = a.part + (int64_t)blockIdx.x * (kH * kH + kH);
#pragma unroll
  for (int jt = 0; jt < JT; ++jt)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) P[((wave * JT + jt) * 16 + 4 * kq + i) * kH + kt * 16 + m] = d[jt][kt][i];
  if (tid < kH) {
    float db = 0.f;
#pragma unroll
    for (int rr = 0; rr < kWgGraphs; ++rr) db += Cs[rr] * Ts[rr * kWPad + tid];
    P[kH * kH + tid] = db;
  }
}

inline bool pool_csr_ok(const int32_t *gptr, const int32_t *gent, int64_t V, int64_t G) {
  return gptr && (gent || V == 0) && V >= 0 && G >= 0 && G < ((int64_t)1 << 24) && V < ((int64_t)1 << 30);
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_heads_forward(const dmp_head_weights *w, const dmp_head_io *io, int num_heads, int B, int H, float slope,
                      void *stream) {
  if ((H != 128 && H != 64 && H > 0) || !slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (!heads_valid(w, io, num_heads, B, H)) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  Heads t;
  for (int i = 0; i < num_heads; ++i) { t.w[i] = w[i]; t.io[i] = io[i]; t.gr[i] = dmp_head_grads{}; }
  t.B = B; t.slope = slope;
  const dim3 grid((unsigned)((B + kRows - 1) / kRows), (unsigned)num_heads);
  if (H == 128) heads_fwd_k<128><<<grid, kThreads, 0, (hipStream_t)stream>>>(t);
  else heads_fwd_k<64><<<grid, kThreads, 0, (hipStream_t)stream>>>(t);
  return check_launch();
}

int dmp_heads_blend(const float *const *y, const float *const *gl, float *const *w, int num_heads, int B, float *out,
                    void *stream) {
  if (num_heads < 1 || num_heads > kMaxHeads || B < 0 || !y || !gl || !w) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!out) return DMP_ERR_BAD_ARG;
  BlendArgs a;
  for (int i = 0; i < num_heads; ++i) {
    if (!y[i] || !gl[i] || !w[i]) return DMP_ERR_BAD_ARG;
    a.y[i] = y[i]; a.gl[i] = gl[i]; a.w[i] = w[i];
  }
  a.out = out; a.n = num_heads; a.B = B;
  heads_blend_k<<<(unsigned)((B + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

int dmp_heads_backward(const dmp_head_weights *w, const dmp_head_io *io, const dmp_head_grads *g, int num_heads, int B,
                       int H, float slope, void *stream) {
  if ((H != 128 && H != 64 && H > 0) || !slope_ok(slope)) return DMP_ERR_UNSUPPORTED;
  if (!heads_valid(w, io, num_heads, B, H) || !g) return DMP_ERR_BAD_ARG;
  const int kH = H, kF = 4 * H + 4, kYS = H + 4;
  for (int i = 0; i < num_heads; ++i) {
    if (!g[i].dy || !ok16p(g[i].dY1) || !ok16p(g[i].dP) || !ok16p(g[i].dG) || (g[i].dps && (!ok16p(g[i].dps) || g[i].ld_dps % 4)) ||
        (g[i].dgs && (!ok16p(g[i].dgs) || g[i].ld_dgs % 4)) || !g[i].dWp || !g[i].dbp || !g[i].dWg || !g[i].dbg || !g[i].dW1 ||
        !g[i].db1 || !g[i].dW2 || !g[i].db2)
      return DMP_ERR_BAD_ARG;
  }
  if (B == 0) return DMP_OK;   // the caller zero-fills the weight gradients of an empty batch
  Heads t;
  WJobs wj;
  wj.n = 0; wj.B = B;
  int blocks = 0;
  for (int i = 0; i < num_heads; ++i) {
    t.w[i] = w[i]; t.io[i] = io[i]; t.gr[i] = g[i];
    add_wjob(wj, blocks, g[i].dY1, kH, kH, nullptr, io[i].F, kF, kF, g[i].dW1, kF, g[i].db1, 1.0f);
    add_wjob(wj, blocks, g[i].dP, kH, kH, nullptr, io[i].ps, io[i].ld_ps, kH, g[i].dWp, kH, g[i].dbp, io[i].scale_p);
    add_wjob(wj, blocks, g[i].dG, kH, kH, nullptr, io[i].gs, io[i].ld_gs, kH, g[i].dWg, kH, g[i].dbg, io[i].scale_g);
    add_wjob(wj, blocks, g[i].dy, 1, 1, g[i].dy_scale, io[i].Y1S, kYS, kYS, g[i].dW2, kYS, g[i].db2, 1.0f);
  }
  t.B = B; t.slope = slope;
  const dim3 grid((unsigned)((B + kRows - 1) / kRows), (unsigned)num_heads);
  if (H == 128) heads_bwd_rows_k<128><<<grid, kThreads, 0, (hipStream_t)stream>>>(t);
  else heads_bwd_rows_k<64><<<grid, kThreads, 0, (hipStream_t)stream>>>(t);
  int rc = check_launch();
  if (rc != DMP_OK) return rc;
  heads_bwd_w_k<<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(wj);
  return check_launch();
}

int dmp_count_loss(const float *pred, const float *target, int64_t n, int kind, float neg_slope, float *loss, float *dpred, void *stream) {
  if (n < 1 || kind < 0 || kind > 2 || !pred || !target || !loss || !dpred) return DMP_ERR_BAD_ARG;
  if (n > ((int64_t)1 << 22) || !(neg_slope >= 0.f && neg_slope <= 1.f)) return DMP_ERR_UNSUPPORTED;     // (one workgroup: a batch's counts)
  count_loss_k<<<1, kLossThreads, 0, (hipStream_t)stream>>>(pred, target, n, kind, neg_slope, loss, dpred);
  return check_launch();
}

int dmp_pool_out(const float *partH, const float *partZ, int64_t V, int halves, const int32_t *gptr, const int32_t *gent, int64_t G,
                 const float *gcnt, const float *W2, const float *b2, const float *partX, int64_t Vn, const int32_t *ngptr,
                 const int32_t *ngent, int64_t Gn, int H, float *es, float *vs, float *Q, void *stream) {
  if (H != 128 && H != 64) return DMP_ERR_UNSUPPORTED;
  if ((halves != 1 && halves != 2) || !pool_csr_ok(gptr, gent, V, G)) return DMP_ERR_BAD_ARG;
  if (G > 0 && (((V > 0 || partH) && !ok16p(partH)) || (partZ && !ok16p(partZ)) || !ok16p(W2) || (b2 && (!ok16p(b2) || !gcnt)) || !ok16p(es) || (Q && !ok16p(Q))))
    return DMP_ERR_BAD_ARG;
  if (!partX) Gn = 0;
  if (partX && (!pool_csr_ok(ngptr, ngent, Vn, Gn) || (Gn > 0 && (!ok16p(partX) || !ok16p(vs))))) return DMP_ERR_BAD_ARG;
  if (G == 0 && Gn == 0) return DMP_OK;
  PoolOut a;
  a.partH = partH; a.partZ = partZ; a.partX = partX; a.gcnt = gcnt; a.W2 = W2; a.b2 = b2;
  a.gptr = gptr; a.gent = gent; a.ngptr = ngptr; a.ngent = ngent; a.es = es; a.vs = vs; a.Q = Q;
  a.ldh = (int64_t)halves * H; a.V = V; a.Vn = Vn; a.G = (int)G; a.Gn = (int)Gn; a.halves = halves;
  a.eblocks = (int)((G + kRows - 1) / kRows);
  const unsigned grid = (unsigned)(a.eblocks + (Gn + kRows - 1) / kRows);
  if (H == 128) pool_out_k<128><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  else pool_out_k<64><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

int dmp_rows_gemm(const float *A, int64_t lda, int64_t rows, int H, const float *W, int w_out_in, float *out, int64_t ldo,
                  void *stream) {
  if (H != 128 && H != 64) return DMP_ERR_UNSUPPORTED;
  if (rows < 0 || rows >= ((int64_t)1 << 30) || lda < H || ldo < H || lda % 4 || ldo % 4) return DMP_ERR_BAD_ARG;
  if (rows == 0) return DMP_OK;
  if (!ok16p(A) || !ok16p(W) || !ok16p(out)) return DMP_ERR_BAD_ARG;
  const unsigned grid = (unsigned)((rows + kRows - 1) / kRows);
  if (H == 128) rows_gemm_k<128><<<grid, kThreads, 0, (hipStream_t)stream>>>(A, lda, (int)rows, W, w_out_in ? 1 : 0, out, ldo);
  else rows_gemm_k<64><<<grid, kThreads, 0, (hipStream_t)stream>>>(A, lda, (int)rows, W, w_out_in ? 1 : 0, out, ldo);
  return check_launch();
}

int64_t dmp_pool_wgrad_blocks(int64_t G) { return G > 0 ? (G + kWgGraphs - 1) / kWgGraphs : 0; }

int dmp_pool_wgrad(const float *qc, int64_t ldq, int64_t V, int halves, const int32_t *gptr, const int32_t *gent, int64_t G,
                   const float *T, int64_t ldt, const float *gcnt, int H, float *partial, float *Q, void *stream) {
  if (H != 128 && H != 64) return DMP_ERR_UNSUPPORTED;
  if ((halves != 1 && halves != 2) || !pool_csr_ok(gptr, gent, V, G) || ldt < H || ldt % 4 || ldq < H || ldq % 4) return DMP_ERR_BAD_ARG;
  if (G == 0) return DMP_OK;
  if (((V > 0 || qc) && !ok16p(qc)) || !ok16p(T) || !gcnt || !ok16p(partial) || (Q && !ok16p(Q))) return DMP_ERR_BAD_ARG;
  PoolWgrad a;
  a.qc = qc; a.T = T; a.gcnt = gcnt; a.gptr = gptr; a.gent = gent; a.part = partial; a.Q = Q;
  a.ldq = ldq; a.ldt = ldt; a.V = V; a.G = (int)G; a.halves = halves;
  const unsigned grid = (unsigned)dmp_pool_wgrad_blocks(G);
  if (H == 128) pool_wgrad_k<128><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  else pool_wgrad_k<64><<<grid, kThreads, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

}  // extern "C"
