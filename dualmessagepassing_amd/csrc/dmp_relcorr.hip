// CompGCN's relation-typed weights (UNC Model/CompGCN/src/model.py:117-264, comp_opt "corr") for the transform-then-
// aggregate form of dmp_relconv.hip.  The circular correlation corr(h, t)[k] = sum_i h[i] t[(i + k) mod I] is linear in
// h: corr(h, t) = h @ C(t) with C(t)[i, k] = t[(i + k) mod I].  An edge of type b carries the relation row t_b = T[b], so
// its message is h[src] @ W_b with W_b = C(t_b) @ in_weight; the self loop is one more block, C(loop_rel) @ loop_weight.
//
//   relcorr_fwd   Wcat[i, b P + o] = scale sum_k t_b[(i + k) mod I] W_b[k, o]         (o < H; zero for H <= o < P)
//   relcorr_bwd   dW_b[k, o]       = scale sum_i t_b[(i + k) mod I] dWcat[i, b P + o]   (dWin: summed over b < R, b ascending)
//                 dt_b[j]          = scale sum_i sum_o dWcat[i, b P + o] W_b[(j - i) mod I, o]
//
// with t_b = T[b], W_b = Win for b < R and t_R = loop_rel, W_R = Wloop.  The first two lines are one shape,
// out[r, o] = sum_s t[(r + s) mod I] M[s, o]: a workgroup owns kRows rows by 64 columns, a lane one column, and the four
// waves split the sum over s; the relation row sits in LDS twice over (t2[j] = t[j mod I]), so the wrap-around is an
// index and the kRows values a step needs are a window that slides by one LDS read.  dt_b is a circular convolution down
// every column: a lane owns a column and kRows consecutive j, the window of W rows slides by one global read per i.
// Every sum has a fixed order (ascending inside a wave, the waves' partials added 0..3, lanes by a fixed butterfly): no
// atomics, bitwise repeatable.  Plain fp32 FMAs -- at most 17 * 256^3 of them per launch.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kRows = 8;              // rows (fwd, dW) or j values (dt) a lane accumulates
constexpr int kCorrMaxDim = 256;      // I and H
constexpr int kCorrMaxBlocks = 17;    // R + 1
constexpr int kWaves = kBlock / kWave;

__host__ __device__ constexpr int t2_len(int I) { return 2 * I + 3 * kRows; }

// t2[j] = t[j mod I] for j < t2_len(I): every index r + s + u below (r < I + kRows, s + u < I + 2 kRows) stays inside
__device__ __forceinline__ void stage_row(float *t2, const float *__restrict__ t, int I) {
  for (int j = threadIdx.x; j < t2_len(I); j += kBlock) t2[j] = t[j % I];
}

// acc[rr] += sum_{s in [sb, se)} t2[r0 + rr + s] * M[s * ldm]   (M already points at this lane's column)
__device__ __forceinline__ void corr_rows(const float *t2, const float *__restrict__ M, int64_t ldm, bool col_on, int r0,
                                          int sb, int se, float (&acc)[kRows]) {
  float win[kRows];   // at step u of a batch the window value of row rr is win[(rr + u) % kRows]
#pragma unroll
  for (int rr = 0; rr < kRows - 1; ++rr) win[rr] = t2[r0 + sb + rr];
  for (int s = sb; s < se; s += kRows) {
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int ss = s + u;
      win[(kRows - 1 + u) % kRows] = t2[r0 + ss + kRows - 1];
      const float m = (col_on && ss < se) ? M[(int64_t)ss * ldm] : 0.f;
#pragma unroll
      for (int rr = 0; rr < kRows; ++rr) acc[rr] = fmaf(win[(rr + u) % kRows], m, acc[rr]);
    }
  }
}

// the four waves' partial tiles [kWaves][kRows][64] summed in wave order; out[(r0 + rr) * ldo + o] = scale * sum for o < H,
// zero for H <= o < P
__device__ __forceinline__ void reduce_store(float *red, const float (&acc)[kRows], float scale, float *__restrict__ out,
                                             int64_t ldo, int r0, int rows, int o0, int H, int P) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
  for (int rr = 0; rr < kRows; ++rr) red[(wave * kRows + rr) * kWave + lane] = acc[rr];
  __syncthreads();
  for (int e = threadIdx.x; e < kRows * kWave; e += kBlock) {
    const int rr = e / kWave, c = e % kWave;
    const int r = r0 + rr, o = o0 + c;
    if (r >= rows || o >= P) continue;
    float v = red[rr * kWave + c];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += red[(w * kRows + rr) * kWave + c];
    out[(int64_t)r * ldo + o] = o < H ? scale * v : 0.f;
  }
}

// grid (column tiles of P, row tiles of I, R + 1)
__global__ __launch_bounds__(kBlock) void relcorr_fwd_k(const float *__restrict__ T, const float *__restrict__ loop_rel,
                                                        const float *__restrict__ Win, const float *__restrict__ Wloop, int R,
                                                        int I, int H, int P, float scale, float *__restrict__ Wcat) {
  extern __shared__ float4 corr_lds[];
  float *t2 = reinterpret_cast<float *>(corr_lds);
  float *red = t2 + (t2_len(I) + 3) / 4 * 4;
  const int b = blockIdx.z, r0 = blockIdx.y * kRows, o0 = blockIdx.x * kWave;
  const int wave = threadIdx.x / kWave, o = o0 + threadIdx.x % kWave;
  stage_row(t2, b < R ? T + (int64_t)b * I : loop_rel, I);
  __syncthreads();
  const int chunk = (I + kWaves - 1) / kWaves;
  const int sb = min(I, wave * chunk), se = min(I, sb + chunk);
  const bool col_on = o < H;
  float acc[kRows];
#pragma unroll
  for (int rr = 0; rr < kRows; ++rr) acc[rr] = 0.f;
  corr_rows(t2, (b < R ? Win : Wloop) + (col_on ? o : 0), H, col_on, r0, sb, se, acc);
  reduce_store(red, acc, scale, Wcat + (int64_t)b * P, (int64_t)(R + 1) * P, r0, I, o0, H, P);
}

// dt_b[j0 .. j0 + kRows) for one b: lanes over the columns, the waves over column groups of 64 and then over parts of i
__device__ __forceinline__ void conv_cols(float *red, const float *__restrict__ dW, int64_t ldd, const float *__restrict__ W, int I,
                                          int H, int j0, float scale, float *__restrict__ dt) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int og = H <= kWave ? 1 : (H <= 2 * kWave ? 2 : kWaves);   // column groups; kWaves / og parts of the i range
  const int o = (wave % og) * kWave + lane, part = wave / og, parts = kWaves / og;
  const int chunk = (I + parts - 1) / parts;
  const int ib = min(I, part * chunk), ie = min(I, ib + chunk);
  const bool col_on = o < H;
  const float *Wc = W + (col_on ? o : 0), *dc = dW + (col_on ? o : 0);
  float acc[kRows], win[kRows];   // at step u the W value of j0 + jj is win[(jj - u) mod kRows]
#pragma unroll
  for (int jj = 0; jj < kRows; ++jj) acc[jj] = 0.f;
  int row = ((j0 - ib) % I + I) % I;   // (j0 - i) mod I, kept by decrement
#pragma unroll
  for (int jj = 1; jj < kRows; ++jj) win[jj] = col_on ? Wc[(int64_t)((row + jj) % I) * H] : 0.f;
  for (int i = ib; i < ie; i += kRows) {
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int ii = i + u;
      const bool on = col_on && ii < ie;     // (past the end of this wave's part: d is zero, the W row is not fetched)
      win[(kRows - u) % kRows] = on ? Wc[(int64_t)row * H] : 0.f;
      row = row == 0 ? I - 1 : row - 1;
      const float d = on ? dc[(int64_t)ii * ldd] : 0.f;
#pragma unroll
      for (int jj = 0; jj < kRows; ++jj) acc[jj] = fmaf(d, win[(jj - u + kRows) % kRows], acc[jj]);
    }
  }
#pragma unroll
  for (int jj = 0; jj < kRows; ++jj) {
    float v = acc[jj];
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    if (lane == 0) red[wave * kRows + jj] = v;
  }
  __syncthreads();
  if (threadIdx.x < kRows && j0 + (int)threadIdx.x < I) {
    float v = red[threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += red[w * kRows + threadIdx.x];
    dt[j0 + threadIdx.x] = scale * v;
  }
}

// grid x: first (R + 1) * jt blocks of dt (jt tiles of kRows j values), then 2 * ct * rt blocks of dWin / dWloop
__global__ __launch_bounds__(kBlock) void relcorr_bwd_k(const float *__restrict__ dWcat, const float *__restrict__ T,
                                                        const float *__restrict__ loop_rel, const float *__restrict__ Win,
                                                        const float *__restrict__ Wloop, int R, int I, int H, int P, float scale,
                                                        float *__restrict__ dT, float *__restrict__ dloop_rel,
                                                        float *__restrict__ dWin, float *__restrict__ dWloop) {
  extern __shared__ float4 corr_lds[];
  float *lds = reinterpret_cast<float *>(corr_lds);
  const int64_t ldd = (int64_t)(R + 1) * P;
  const int jt = (I + kRows - 1) / kRows, ct = (H + kWave - 1) / kWave;
  int blk = blockIdx.x;
  if (blk < (R + 1) * jt) {
    const int b = blk / jt, j0 = (blk % jt) * kRows;
    conv_cols(lds, dWcat + (int64_t)b * P, ldd, b < R ? Win : Wloop, I, H, j0, scale, b < R ? dT + (int64_t)b * I : dloop_rel);
    return;
  }
  blk -= (R + 1) * jt;
  const int is_loop = blk / (ct * jt);
  blk %= ct * jt;
  const int r0 = (blk / ct) * kRows, o0 = (blk % ct) * kWave;
  const int b0 = is_loop ? R : 0, nb = is_loop ? 1 : R;
  const int tl = (t2_len(I) + 3) / 4 * 4;
  float *red = lds + (int64_t)nb * tl;
  for (int b = 0; b < nb; ++b) stage_row(lds + b * tl, is_loop ? loop_rel : T + (int64_t)b * I, I);
  __syncthreads();
  const int wave = threadIdx.x / kWave, o = o0 + threadIdx.x % kWave;
  const int chunk = (I + kWaves - 1) / kWaves;
  const int sb = min(I, wave * chunk), se = min(I, sb + chunk);
  const bool col_on = o < H;
  float acc[kRows];
#pragma unroll
  for (int rr = 0; rr < kRows; ++rr) acc[rr] = 0.f;
  for (int b = 0; b < nb; ++b)
    corr_rows(lds + b * tl, dWcat + (int64_t)(b0 + b) * P + (col_on ? o : 0), ldd, col_on, r0, sb, se, acc);
  reduce_store(red, acc, scale, is_loop ? dWloop : dWin, H, r0, I, o0, H, H);
}

bool corr_shape_ok(int R, int I, int H, int P) {
  return R >= 1 && R + 1 <= kCorrMaxBlocks && I >= 4 && I <= kCorrMaxDim && H >= 4 && H <= kCorrMaxDim && P >= H && P % 4 == 0 &&
         P < H + 4;
}

size_t corr_lds_bytes(int rows, int I) { return sizeof(float) * ((size_t)rows * ((t2_len(I) + 3) / 4 * 4) + kWaves * kRows * kWave); }

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_relcorr_supported(int I, int H, int nblk) {
  return I >= 4 && I <= kCorrMaxDim && H >= 4 && H <= kCorrMaxDim && nblk >= 2 && nblk <= kCorrMaxBlocks;
}

int dmp_relcorr_weights_fwd(const float *T, const float *loop_rel, const float *Win, const float *Wloop, int R, int I, int H, int P,
                            float scale, float *Wcat, void *stream) {
  if (R < 1 || I < 1 || H < 1 || P < H || P % 4 != 0) return DMP_ERR_BAD_ARG;
  if (!corr_shape_ok(R, I, H, P)) return DMP_ERR_UNSUPPORTED;
  if (!T || !loop_rel || !Win || !Wloop || !Wcat) return DMP_ERR_BAD_ARG;
  const dim3 grid((P + kWave - 1) / kWave, (I + kRows - 1) / kRows, R + 1);
  hipLaunchKernelGGL(relcorr_fwd_k, grid, dim3(kBlock), corr_lds_bytes(1, I), static_cast<hipStream_t>(stream), T, loop_rel, Win, Wloop,
                     R, I, H, P, scale, Wcat);
  return check_launch();
}

int dmp_relcorr_weights_bwd(const float *dWcat, const float *T, const float *loop_rel, const float *Win, const float *Wloop, int R, int I,
                            int H, int P, float scale, float *dT, float *dloop_rel, float *dWin, float *dWloop, void *stream) {
  if (R < 1 || I < 1 || H < 1 || P < H || P % 4 != 0) return DMP_ERR_BAD_ARG;
  if (!corr_shape_ok(R, I, H, P)) return DMP_ERR_UNSUPPORTED;
  if (!dWcat || !T || !loop_rel || !Win || !Wloop || !dT || !dloop_rel || !dWin || !dWloop) return DMP_ERR_BAD_ARG;
  const int jt = (I + kRows - 1) / kRows, ct = (H + kWave - 1) / kWave;
  const dim3 grid((R + 1) * jt + 2 * ct * jt);
  hipLaunchKernelGGL(relcorr_bwd_k, grid, dim3(kBlock), corr_lds_bytes(R, I), static_cast<hipStream_t>(stream), dWcat, T, loop_rel, Win,
                     Wloop, R, I, H, P, scale, dT, dloop_rel, dWin, dWloop);
  return check_launch();
}

}  // extern "C"
