// The CNN rep-net layer of the edge-sequence models (SubgraphCountingMatching/models/cnn.py:13-172) on channels-last rows:
// X [B, L, H] -> Y [B, L', H], never the reference's [B, H, L] transposes.
//
// Geometry (stride 1, dilation 1): conv kernel k, padding p -> Lc = L + 2p - k + 1 conv rows; max-pool kernel pk, padding
// pp -> Lout = Lc + 2pp - pk + 1 rows.  conv[s] = b + sum_j W[:, :, j] x[s - p + j] (x outside [0, L) reads 0);
// pool[t] = max of act(conv[s]) over s in [t - pp, t - pp + pk) n [0, Lc) (the reference's -inf padding).
//
// Forward (dmp_cnn_fwd): grid (row tiles, B), 4 waves.  A workgroup computes kTM = 64 conv rows starting at S0 = T0 - pp
// and from them the kTM - (pk - 1) pool rows starting at T0: the pool halo of pk - 1 conv rows is recomputed by the
// neighbouring tile instead of going through HBM.  The GEMM (K = k H, k shifted row blocks of the X tile in LDS) runs on
// v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fma chain), B operand (the weight, Wt[j][i][o]) read through L2.  The
// epilogue writes act(conv + b) to LDS over the X tile, then per pool row: the window's first maximum, its offset and
// sign as one byte (arg, for the backward), the gate after the layer (max-pool of gate_in with the conv geometry, then
// the pool geometry), Y = pool * gate (apply_gate) + resid.  With pk = 1, pp = 0 and no activation the same kernel is a
// plain conv: the transposed conv of the backward (dX) is this kernel on the flipped, transposed weight.
//
// Backward, no float atomics (bitwise reproducible):
//   dmp_cnn_route_bwd  dC[s] = sum over the pool rows t whose window's maximum sits at s of dY[t] gate[t] act'(t)
//                      (gather form, t descending from s + pp);
//   dX                 dmp_cnn_fwd(dC, W2t, pad k - 1 - p), W2t[j][o][i] = W[o, i, k - 1 - j];
//   dmp_cnn_wgrad      split-K partials over row chunks: partial[c] = (dW as [k][o][i], db [H]) of kWgRows rows of
//                      (b, s); dmp_reduce_partials sums them in chunk order.
#include "dmp_common.h"

namespace dmp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTM = 64;         // conv rows per workgroup
constexpr int kMaxK = 8;
constexpr int kWgRows = 1024;   // rows of (b, s) per weight-gradient chunk
constexpr int kWgStage = 32;    // rows staged in LDS per step

struct CnnFwdArgs {
  const float *X, *Wt, *bias, *gate_in, *resid;
  float *Y, *gate_out;
  uint8_t *arg;
  int64_t L, Lc, Lout;
  int k, pad, pk, pp, act, apply_gate;
  float slope;
};

template <int H>
__global__ __launch_bounds__(kBlock) void cnn_fwd_kernel(CnnFwdArgs a) {
  constexpr int LD = H + 1;                      // odd stride: lanes reading one column of 32 rows hit 32 banks
  __shared__ float xs[(kTM + kMaxK - 1) * LD];
  __shared__ float gs[kTM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.y;
  const int TP = kTM - (a.pk - 1);
  const int64_t T0 = (int64_t)blockIdx.x * TP, S0 = T0 - a.pp, U0 = S0 - a.pad;
  const int xrows = kTM + a.k - 1;
  const float *Xb = a.X + b * a.L * H;

  // X rows U0 .. U0 + xrows - 1 (zero outside [0, L))
  for (int e = tid; e < xrows * (H / 4); e += kBlock) {
    const int r = e / (H / 4), c = (e % (H / 4)) * 4;
    const int64_t u = U0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u >= 0 && u < a.L) v = *reinterpret_cast<const float4 *>(Xb + u * H + c);
    float *d = xs + r * LD + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  // the gate after this layer for the pool rows of the tile
  if (a.gate_in && tid < TP) {
    const int64_t t = T0 + tid;
    float g = 0.f;
    if (t < a.Lout) {
      const float *gi = a.gate_in + b * a.L;
      g = -INFINITY;
      for (int q = 0; q < a.pk; ++q) {
        const int64_t s = t - a.pp + q;
        if (s < 0 || s >= a.Lc) continue;
        for (int j = 0; j < a.k; ++j) {
          const int64_t u = s - a.pad + j;
          if (u >= 0 && u < a.L) g = fmaxf(g, gi[u]);
        }
      }
      a.gate_out[b * a.Lout + t] = g;
    }
    gs[tid] = g;
  }
  __syncthreads();

  // MFMA tiles: H = 128 -> wave w owns columns 32w.. of both 32-row blocks; H = 64 -> one 32 x 32 tile per wave
  constexpr int NT = H == 128 ? 2 : 1;
  const int cb = H == 128 ? wave : (wave & 1);
  const int rb0 = H == 128 ? 0 : (wave >> 1);
  f32x16 acc[NT];
  for (int t = 0; t < NT; ++t)
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const int ar = lane & 31, ak = lane >> 5;
  const float *wcol = a.Wt + cb * 32 + ar;
  for (int j = 0; j < a.k; ++j) {
    const float *wj = wcol + (int64_t)j * H * H;
    const float *xj = xs + (j + ar) * LD + ak;
#pragma unroll 8
    for (int i0 = 0; i0 < H; i0 += 2) {
      const float bv = wj[(i0 + ak) * H];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float av = xj[(32 * (rb0 + t)) * LD + i0];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  __syncthreads();   // the X tile is overwritten by the conv rows below

  // act(conv + b) -> LDS; conv rows outside [0, Lc) are the pool's -inf padding
  const int col = cb * 32 + ar;
  const float bias = a.bias ? a.bias[col] : 0.f;
  for (int t = 0; t < NT; ++t) {
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * (rb0 + t) + (r & 3) + 8 * (r >> 2) + 4 * ak;
      const int64_t s = S0 + row;
      float v = acc[t][r] + bias;
      if (a.act) v = act_fwd(v, a.slope);
      xs[row * LD + col] = (s >= 0 && s < a.Lc) ? v : -INFINITY;
    }
  }
  __syncthreads();

  float *Yb = a.Y + b * a.Lout * H;
  for (int e = tid; e < TP * H; e += kBlock) {
    const int tl = e / H, c = e % H;
    const int64_t t = T0 + tl;
    if (t >= a.Lout) break;
    float best = xs[tl * LD + c];
    int bq = 0;
    for (int q = 1; q < a.pk; ++q) {
      const float v = xs[(tl + q) * LD + c];
      if (v > best) { best = v; bq = q; }
    }
    if (a.arg) a.arg[(b * a.Lout + t) * H + c] = (uint8_t)(bq | (best > 0.f ? 0x80 : 0));
    float y = best;
    if (a.gate_in && a.apply_gate) y *= gs[tl];
    if (a.resid) y += a.resid[(b * a.Lout + t) * H + c];
    Yb[t * H + c] = y;
  }
}

struct CnnRouteArgs {
  const float *dY, *gate;
  const uint8_t *arg;
  float *dC;
  int64_t B, Lc, Lout;
  int H, pk, pp;
  float slope;
};

__global__ __launch_bounds__(kBlock) void cnn_route_kernel(CnnRouteArgs a) {
  const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int H4 = a.H / 4;
  if (n >= a.B * a.Lc * H4) return;
  const int c = (int)(n % H4) * 4;
  const int64_t s = (n / H4) % a.Lc, b = n / H4 / a.Lc;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int q = 0; q < a.pk; ++q) {
    const int64_t t = s + a.pp - q;
    if (t < 0 || t >= a.Lout) continue;
    const int64_t o = (b * a.Lout + t) * a.H + c;
    const float g = a.gate ? a.gate[b * a.Lout + t] : 1.f;
    const float4 d = *reinterpret_cast<const float4 *>(a.dY + o);
    const uchar4 w = *reinterpret_cast<const uchar4 *>(a.arg + o);
    const float dv[4] = {d.x, d.y, d.z, d.w};
    const uint8_t wv[4] = {w.x, w.y, w.z, w.w};
    float r[4];
    for (int i = 0; i < 4; ++i) {
      const float x = dv[i] * g;
      r[i] = ((wv[i] & 0x7f) == q) ? ((wv[i] & 0x80) ? x : a.slope * x) : 0.f;
    }
    acc.x += r[0]; acc.y += r[1]; acc.z += r[2]; acc.w += r[3];
  }
  *reinterpret_cast<float4 *>(a.dC + (b * a.Lc + s) * a.H + c) = acc;
}

struct CnnWgradArgs {
  const float *dC, *X;
  float *partial;
  int64_t rows, L, Lc;
  int k, pad;
};

template <int H>
__global__ __launch_bounds__(kBlock) void cnn_wgrad_kernel(CnnWgradArgs a) {
  constexpr int LD = H + 4;
  __shared__ float ds[kWgStage * LD], xs[kWgStage * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kWgRows;
  const int64_t n1 = n0 + kWgRows < a.rows ? n0 + kWgRows : a.rows;
  constexpr int NT = H == 128 ? 4 : 1;          // output tiles [o block][i block] per wave
  const int ob = H == 128 ? wave : (wave & 1);
  const int ib0 = H == 128 ? 0 : (wave >> 1);
  f32x16 acc[NT];
  for (int t = 0; t < NT; ++t)
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;
  const int ar = lane & 31, ak = lane >> 5;
  for (int64_t m0 = n0; m0 < n1; m0 += kWgStage) {
    __syncthreads();
    for (int e = tid; e < kWgStage * (H / 4); e += kBlock) {
      const int r = e / (H / 4), c = (e % (H / 4)) * 4;
      const int64_t n = m0 + r;
      float4 dv = make_float4(0.f, 0.f, 0.f, 0.f), xv = dv;
      if (n < n1) {
        dv = *reinterpret_cast<const float4 *>(a.dC + n * H + c);
        const int64_t bb = n / a.Lc, s = n % a.Lc, u = s - a.pad + j;
        if (u >= 0 && u < a.L) xv = *reinterpret_cast<const float4 *>(a.X + (bb * a.L + u) * H + c);
      }
      *reinterpret_cast<float4 *>(ds + r * LD + c) = dv;
      *reinterpret_cast<float4 *>(xs + r * LD + c) = xv;
    }
    __syncthreads();
    if (j == 0 && tid < H)
      for (int r = 0; r < kWgStage; ++r) bsum += ds[r * LD + tid];
#pragma unroll 4
    for (int r = 0; r < kWgStage; r += 2) {
      const float av = ds[(r + ak) * LD + ob * 32 + ar];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bv = xs[(r + ak) * LD + (ib0 + t) * 32 + ar];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  float *P = a.partial + (int64_t)blockIdx.x * ((int64_t)a.k * H * H + H);
  float *Pj = P + (int64_t)j * H * H;
  for (int t = 0; t < NT; ++t)
    for (int r = 0; r < 16; ++r) {
      const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * ak, i = (ib0 + t) * 32 + ar;
      Pj[o * H + i] = acc[t][r];
    }
  if (j == 0 && tid < H) P[(int64_t)a.k * H * H + tid] = bsum;
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_cnn_fwd(const float *X, int64_t B, int64_t L, int H, const float *Wt, const float *bias, int k, int pad, int pk, int pp,
                int act, float slope, const float *gate_in, int apply_gate, const float *resid, float *Y, uint8_t *arg,
                float *gate_out, void *stream) {
  if (B < 0 || L < 1 || (H != 64 && H != 128) || k < 1 || k > kMaxK || pad < 0 || pad >= k || pk < 1 || pk > k || pp < 0 ||
      2 * pp > pk || !slope_ok(slope))
    return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!X || !Wt || !Y || !aligned16(X) || (gate_in && !gate_out)) return DMP_ERR_BAD_ARG;
  const int64_t Lc = L + 2 * pad - k + 1, Lout = Lc + 2 * pp - pk + 1;
  if (Lc < 1 || Lout < 1) return DMP_ERR_BAD_ARG;
  if (B >= 65536 || B * (L + 2 * kMaxK) * H >= ((int64_t)1 << 31) * 4) return DMP_ERR_UNSUPPORTED;
  CnnFwdArgs a{X, Wt, bias, gate_in, resid, Y, gate_out, arg, L, Lc, Lout, k, pad, pk, pp, act ? 1 : 0, apply_gate ? 1 : 0, slope};
  const int TP = kTM - (pk - 1);
  const dim3 grid((unsigned)((Lout + TP - 1) / TP), (unsigned)B);
  if (H == 128)
    hipLaunchKernelGGL(cnn_fwd_kernel<128>, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(cnn_fwd_kernel<64>, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

int dmp_cnn_route_bwd(const float *dY, const float *gate, const uint8_t *arg, int64_t B, int64_t Lc, int64_t Lout, int H, int pk,
                      int pp, float slope, float *dC, void *stream) {
  if (B < 0 || Lc < 1 || Lout < 1 || H < 4 || H % 4 || pk < 1 || pk > kMaxK || pp < 0 || !slope_ok(slope)) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!dY || !arg || !dC || !aligned16(dY) || !aligned16(dC) || ((uintptr_t)arg & 3u)) return DMP_ERR_BAD_ARG;
  const int64_t n = B * Lc * (H / 4);
  if ((n + kBlock - 1) / kBlock >= ((int64_t)1 << 31)) return DMP_ERR_UNSUPPORTED;
  CnnRouteArgs a{dY, gate, arg, dC, B, Lc, Lout, H, pk, pp, slope};
  hipLaunchKernelGGL(cnn_route_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch();
}

int64_t dmp_cnn_wgrad_chunks(int64_t rows) { return rows > 0 ? (rows + kWgRows - 1) / kWgRows : 0; }

int dmp_cnn_wgrad(const float *dC, const float *X, int64_t B, int64_t L, int64_t Lc, int H, int k, int pad, float *partial,
                  void *stream) {
  if (B < 0 || L < 1 || Lc < 1 || (H != 64 && H != 128) || k < 1 || k > kMaxK || pad < 0) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!dC || !X || !partial || !aligned16(dC) || !aligned16(X) || !aligned16(partial)) return DMP_ERR_BAD_ARG;
  const int64_t rows = B * Lc;
  CnnWgradArgs a{dC, X, partial, rows, L, Lc, k, pad};
  const dim3 grid((unsigned)dmp_cnn_wgrad_chunks(rows), (unsigned)k);
  if (H == 128)
    hipLaunchKernelGGL(cnn_wgrad_kernel<128>, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(cnn_wgrad_kernel<64>, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  return check_launch();
}

}  // extern "C"
