// Relational graph convolution (DGL 0.6 RelGraphConv, regularizer "basis") as transform-then-aggregate:
// the caller forms Y = x @ W_cat with one GEMM, W_cat = [W_0 | ... | W_{R-1} | loop_weight] (each block padded to P
// columns, the padding zero), and these kernels do the relation-typed gather-sum over the graph's CSRs.
//
//   relconv_fwd   out[v] = act(sum_{e: dst e = v} n_e Y[src e, t_e] + h_bias + Y[v, R])    over the in-CSR
//   relconv_bwd   g = dOut act'(out);  dY[u, r] = sum_{e: src e = u, t_e = r} n_e g[dst e],  dY[u, R] = g[u]
//                                                                                  over the out-CSR
//
// One G-lane group per row, each lane owning four columns of every block (float4).  The sums run in CSR order (ascending
// edge id), one accumulator per column: no float atomics, bitwise repeatable.  The backward keeps the R per-type partial
// rows of its source node in LDS (each lane touches only its own columns, so no barrier is needed) and writes them once.
// Edges whose type is outside [0, R) or whose other endpoint is outside [0, N) contribute nothing.
#include <algorithm>

#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kRelLdsBytes = 64 * 1024;   // LDS budget of one backward workgroup

__device__ __forceinline__ float4 ld4r(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4r(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }

// four columns c .. c + 3 of an [N, H] row (H need not be a multiple of 4): zero past H
__device__ __forceinline__ float4 ld_cols(const float *row, int c, int H) {
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = c + k < H ? row[c + k] : 0.f;
  return make_float4(v[0], v[1], v[2], v[3]);
}

// g = dOut * act'(out): act 0 none, 1 tanh (derivative 1 - out^2 on the saved output, torch's tanh_backward)
__device__ __forceinline__ float4 grad_cols(const float *dOut, const float *out, int64_t v, int c, int H, int act) {
  float4 d = ld_cols(dOut + v * H, c, H);
  if (act == 1) {
    const float4 y = ld_cols(out + v * H, c, H);
    d.x *= 1.f - y.x * y.x; d.y *= 1.f - y.y * y.y; d.z *= 1.f - y.z * y.z; d.w *= 1.f - y.w * y.w;
  }
  return d;
}

template <int G>
__global__ __launch_bounds__(kBlock) void relconv_fwd_k(
    const float *__restrict__ Y, const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_ent,
    const int32_t *__restrict__ src32, const int64_t *__restrict__ etype, const float *__restrict__ norm,
    const float *__restrict__ bias, int N, int R, int loop, int H, int P, int act, float *__restrict__ out) {
  constexpr int RPB = kBlock / G;
  const int row = xcd_remap(blockIdx.x, gridDim.x) * RPB + threadIdx.x / G;
  const int lane = threadIdx.x % G;
  if (row >= N) return;
  const int64_t ldy = (int64_t)(R + loop) * P;
  const int beg = in_ptr[row], end = in_ptr[row + 1];
  for (int c0 = 0; c0 < P; c0 += G * 4) {
    const int c = c0 + lane * 4;
    const bool on = c < P;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = beg; base < end; base += G) {
      const int cnt = min(G, end - base);
      int myu = -1, myt = 0;
      float myw = 0.f;
      if (lane < cnt) {
        const int e = in_ent[base + lane] >> 1;
        const int64_t t = etype[e];
        const int u = src32[e];
        if (t >= 0 && t < R && u >= 0 && u < N) {
          myu = u;
          myt = (int)t;
          myw = norm ? norm[e] : 1.f;
        }
      }
      for (int j = 0; j < cnt; ++j) {
        const int u = __shfl(myu, j, G), t = __shfl(myt, j, G);
        const float w = __shfl(myw, j, G);
        if (on && u >= 0) {
          const float4 y = ld4r(Y + (int64_t)u * ldy + (int64_t)t * P + c);
          acc.x += w * y.x; acc.y += w * y.y; acc.z += w * y.z; acc.w += w * y.w;
        }
      }
    }
    if (!on || c >= H) continue;
    // DGL's order: (agg + h_bias) + loop message, then the activation
    if (bias) {
      const float4 b = ld_cols(bias, c, H);
      acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
    }
    if (loop) {
      const float4 s = ld4r(Y + (int64_t)row * ldy + (int64_t)R * P + c);
      acc.x += s.x; acc.y += s.y; acc.z += s.z; acc.w += s.w;
    }
    float v[4] = {acc.x, acc.y, acc.z, acc.w};
    float *o = out + (int64_t)row * H;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < H) o[c + k] = act == 1 ? tanhf(v[k]) : v[k];
  }
}

template <int G>
__global__ __launch_bounds__(kBlock) void relconv_bwd_k(
    const float *__restrict__ dOut, const float *__restrict__ out, const int32_t *__restrict__ out_ptr,
    const int32_t *__restrict__ out_ent, const int32_t *__restrict__ dst32, const int64_t *__restrict__ etype,
    const float *__restrict__ norm, int N, int R, int loop, int H, int P, int act, float *__restrict__ dY) {
  extern __shared__ float4 rel_lds[];
  const int rpb = blockDim.x / G;
  const int gi = threadIdx.x / G, lane = threadIdx.x % G;
  const int row = blockIdx.x * rpb + gi;
  if (row >= N) return;                       // (no barrier below: every lane reads and writes its own LDS columns only)
  float *acc = reinterpret_cast<float *>(rel_lds) + (int64_t)gi * R * P;
  const int64_t ldy = (int64_t)(R + loop) * P;
  for (int t = 0; t < R; ++t)
    for (int c = lane * 4; c < P; c += G * 4) st4r(acc + t * P + c, make_float4(0.f, 0.f, 0.f, 0.f));
  const int beg = out_ptr[row], end = out_ptr[row + 1];
  for (int base = beg; base < end; base += G) {
    const int cnt = min(G, end - base);
    int myv = -1, myt = 0;
    float myw = 0.f;
    if (lane < cnt) {
      const int e = out_ent[base + lane] >> 1;
      const int64_t t = etype[e];
      const int v = dst32[e];
      if (t >= 0 && t < R && v >= 0 && v < N) {
        myv = v;
        myt = (int)t;
        myw = norm ? norm[e] : 1.f;
      }
    }
    for (int j = 0; j < cnt; ++j) {
      const int v = __shfl(myv, j, G), t = __shfl(myt, j, G);
      const float w = __shfl(myw, j, G);
      if (v < 0) continue;
      for (int c = lane * 4; c < P; c += G * 4) {
        const float4 g = grad_cols(dOut, out, v, c, H, act);
        float4 a = ld4r(acc + t * P + c);
        a.x += w * g.x; a.y += w * g.y; a.z += w * g.z; a.w += w * g.w;
        st4r(acc + t * P + c, a);
      }
    }
  }
  float *d = dY + (int64_t)row * ldy;
  for (int t = 0; t < R; ++t)
    for (int c = lane * 4; c < P; c += G * 4) st4r(d + t * P + c, ld4r(acc + t * P + c));
  if (loop)
    for (int c = lane * 4; c < P; c += G * 4) st4r(d + (int64_t)R * P + c, grad_cols(dOut, out, row, c, H, act));
}

// lanes per row: enough for one float4 per lane over P columns, at least 4, at most a wave
int lanes_for(int P) {
  int g = 4;
  while (g < kWave && g * 4 < P) g *= 2;
  return g;
}

bool shape_ok(int64_t N, int R, int H, int P, int loop, int act) {
  return N >= 0 && N < ((int64_t)1 << 31) && R >= 1 && H >= 1 && P >= H && P % 4 == 0 && (loop == 0 || loop == 1) &&
         (act == 0 || act == 1) && (int64_t)(R + loop) * P < ((int64_t)1 << 24);
}

bool lds_ok(int R, int P) { return (int64_t)R * P * 4 <= kRelLdsBytes; }

template <int G>
void launch_fwd(const float *Y, const int32_t *in_ptr, const int32_t *in_ent, const int32_t *src32, const int64_t *etype,
                const float *norm, const float *bias, int N, int R, int loop, int H, int P, int act, float *out, hipStream_t s) {
  constexpr int RPB = kBlock / G;
  hipLaunchKernelGGL(relconv_fwd_k<G>, dim3((N + RPB - 1) / RPB), dim3(kBlock), 0, s, Y, in_ptr, in_ent, src32, etype, norm, bias,
                     N, R, loop, H, P, act, out);
}

template <int G>
void launch_bwd(const float *dOut, const float *out, const int32_t *out_ptr, const int32_t *out_ent, const int32_t *dst32,
                const int64_t *etype, const float *norm, int N, int R, int loop, int H, int P, int act, float *dY, hipStream_t s) {
  const int64_t row_bytes = (int64_t)R * P * 4;
  const int rpb = (int)std::min<int64_t>(kBlock / G, kRelLdsBytes / row_bytes);
  hipLaunchKernelGGL(relconv_bwd_k<G>, dim3((N + rpb - 1) / rpb), dim3(rpb * G), (size_t)(rpb * row_bytes), s, dOut, out, out_ptr,
                     out_ent, dst32, etype, norm, N, R, loop, H, P, act, dY);
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_relconv_supported(int num_rels, int out_p) { return num_rels >= 1 && out_p >= 4 && out_p % 4 == 0 && lds_ok(num_rels, out_p); }

int dmp_relconv_fwd(const float *Y, const int32_t *in_ptr, const int32_t *in_ent, const int32_t *src32, const int64_t *etype,
                    const float *norm, const float *bias, int64_t N, int R, int loop, int H, int P, int act, float *out,
                    void *stream) {
  if (!shape_ok(N, R, H, P, loop, act)) return DMP_ERR_BAD_ARG;
  if (!lds_ok(R, P)) return DMP_ERR_UNSUPPORTED;
  if (N == 0) return DMP_OK;
  if (!Y || !in_ptr || !out || !aligned16(Y)) return DMP_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (lanes_for(P)) {
    case 4: launch_fwd<4>(Y, in_ptr, in_ent, src32, etype, norm, bias, (int)N, R, loop, H, P, act, out, s); break;
    case 8: launch_fwd<8>(Y, in_ptr, in_ent, src32, etype, norm, bias, (int)N, R, loop, H, P, act, out, s); break;
    case 16: launch_fwd<16>(Y, in_ptr, in_ent, src32, etype, norm, bias, (int)N, R, loop, H, P, act, out, s); break;
    case 32: launch_fwd<32>(Y, in_ptr, in_ent, src32, etype, norm, bias, (int)N, R, loop, H, P, act, out, s); break;
    default: launch_fwd<64>(Y, in_ptr, in_ent, src32, etype, norm, bias, (int)N, R, loop, H, P, act, out, s); break;
  }
  return check_launch();
}

int dmp_relconv_bwd(const float *dOut, const float *out, const int32_t *out_ptr, const int32_t *out_ent, const int32_t *dst32,
                    const int64_t *etype, const float *norm, int64_t N, int R, int loop, int H, int P, int act, float *dY,
                    void *stream) {
  if (!shape_ok(N, R, H, P, loop, act)) return DMP_ERR_BAD_ARG;
  if (!lds_ok(R, P)) return DMP_ERR_UNSUPPORTED;
  if (N == 0) return DMP_OK;
  if (!dOut || !out_ptr || !dY || (act == 1 && !out) || !aligned16(dY)) return DMP_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (lanes_for(P)) {
    case 4: launch_bwd<4>(dOut, out, out_ptr, out_ent, dst32, etype, norm, (int)N, R, loop, H, P, act, dY, s); break;
    case 8: launch_bwd<8>(dOut, out, out_ptr, out_ent, dst32, etype, norm, (int)N, R, loop, H, P, act, dY, s); break;
    case 16: launch_bwd<16>(dOut, out, out_ptr, out_ent, dst32, etype, norm, (int)N, R, loop, H, P, act, dY, s); break;
    case 32: launch_bwd<32>(dOut, out, out_ptr, out_ent, dst32, etype, norm, (int)N, R, loop, H, P, act, dY, s); break;
    default: launch_bwd<64>(dOut, out, out_ptr, out_ent, dst32, etype, norm, (int)N, R, loop, H, P, act, dY, s); break;
  }
  return check_launch();
}

}  // extern "C"
