// Transformer-XL relative-position attention without a causal mask: the core of `TXLAttn.forward`
// (SubgraphCountingMatching/models/txl.py:95-177) as the TXL rep-net runs it (`encoder_forward`: the attention mask is all ones).
//
//   per sequence n and head h, with m = k - q:
//   AC[i, j] = (Q_i + r_w_bias) . K_j                    BD[i, p] = (Q_i + r_r_bias) . R_p
//   S[i, j]  = scale * (AC[i, j] + shift(BD)[i, j])      P = softmax_j S        O = P V
//
// shift is the reference's `rel_shift`: BD padded with a zero column in front, read as [k + 1, q], first row dropped, read as
// [q, k].  Without the causal mask its wrap-around takes part, so in closed form
//   j - i <  m + 1:  shift(BD)[i, j] = BD[i, q - 1 - i + j]
//   j - i == m + 1:  0
//   j - i >  m + 1:  BD[i + 1, j - i - m - 2]            (the NEXT row's query)
// and its transpose, for the backward, with t = i + 1 + p - q:
//   t >= 0:  dBD[i, p] = dS[i, t];      t < 0 and i >= 1:  dBD[i, p] = dS[i - 1, t + k];      else 0  (BD[0, p < q - 1] is dropped).
//
// Shapes: q <= 64, q <= k <= 128, dh in {16, 32, 64, 128}; Q [N, q, nh, dh], K / V [N, k, nh, dh], R [k, nh, dh], biases [nh, dh].
// One workgroup (256 threads) owns one (sequence, head): the next row of the wrap is in the same tile.  No [N, q, k, nh] tensor
// reaches global memory: the forward keeps the row maximum and the row sum of exp, the backward recomputes S bit for bit.
//
// LDS map (floats; LDT = 132, LDC = DC + 4, DC = min(dh, 32) the chunk of the head width a pass stages):
//   T1 [q][LDT]   BD, then S, then P            (backward: later dBD)
//   T2 [q][LDT]   backward only: dP, then dS = scale * P * (dP - delta)
//   A0, A1 (, A2 backward) [q][LDC]             query-side chunks: Q + r_w_bias, Q + r_r_bias, dO, and the dQ halves
//   B0, B1 [k][LDC]                             key-side chunks: K, R, V
// Worst case (q 64, k 128): forward 87 KiB, backward 129 KiB of the CU's 160 KiB; q = k = 8 takes 8 / 13 KiB.
//
// Arithmetic: plain fp32 fmaf chains in a fixed order.  A thread of the 16 x 16 grid owns S[ty + 16 a, tx + 16 b]; the products
// against a tile give a thread one float4 of the chunk for each of its rows (P V, dS K, dBD R: rows ty + RP x, the tile read four
// columns at a time) or for four neighbouring columns of the tile (P^T dO, dS^T Qw, dBD^T Qr: one float4 of the tile per step).
//
// Backward: workgroup (g, h) walks the sequences g, g + G, ... of head h and keeps its own partial of dR and of the two bias
// gradients in global memory (the same thread adds to the same word every time); dmp_reduce_partials sums the G partials in
// a fixed order.  No float atomics: two runs are bitwise equal.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kTxlMaxQ = 64, kTxlMaxK = 128;
constexpr int kLdt = kTxlMaxK + 4;         // tile row stride: rows 4 banks apart
constexpr int kTxlGroups = 256;            // backward: workgroups in all (one per CU), shared out over the heads

struct TxlArgs {
  const float *Q, *K, *V, *R, *bw, *br;
  int64_t N;
  int q, k, nh, dh;
  float scale;
};

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// rows x DC floats of X (row stride ld) (+ bias[DC]) -> dst [rows][DC + 4]
template <int DC>
__device__ __forceinline__ void stage(float *dst, const float *__restrict__ X, int64_t ld, int rows, const float *__restrict__ bias) {
  constexpr int G = DC / 4, LDC = DC + 4;
  for (int e = threadIdx.x; e < rows * G; e += kBlock) {
    const int r = e / G, c = (e % G) * 4;
    float4 x = ld4(X + (int64_t)r * ld + c);
    if (bias) {
      const float4 b = ld4(bias + c);
      x.x += b.x; x.y += b.y; x.z += b.z; x.w += b.w;
    }
    st4(dst + r * LDC + c, x);
  }
}

// acc[a][b] += A[ia[a]] . B[jb[b]] over the DC columns of the chunk, ascending
template <int DC>
__device__ __forceinline__ void nt_acc(const float *A, const float *B, const int (&ia)[4], const int (&jb)[8], float (&acc)[4][8]) {
  constexpr int LDC = DC + 4;
#pragma unroll 2
  for (int d = 0; d < DC; d += 4) {
    float4 a[4], b[8];
#pragma unroll
    for (int x = 0; x < 4; ++x) a[x] = ld4(A + ia[x] * LDC + d);
#pragma unroll
    for (int y = 0; y < 8; ++y) b[y] = ld4(B + jb[y] * LDC + d);
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        float v = acc[x][y];
        v = fmaf(a[x].x, b[y].x, v);
        v = fmaf(a[x].y, b[y].y, v);
        v = fmaf(a[x].z, b[y].z, v);
        v = fmaf(a[x].w, b[y].w, v);
        acc[x][y] = v;
      }
  }
}

__device__ __forceinline__ void fma4(float4 &acc, float p, const float4 &v) {
  acc.x = fmaf(p, v.x, acc.x); acc.y = fmaf(p, v.y, acc.y); acc.z = fmaf(p, v.z, acc.z); acc.w = fmaf(p, v.w, acc.w);
}

// acc[x] = sum_{j < n} T[i[x], j] * B[j][c4 .. c4 + 4), j ascending, for the R rows i[x] (inside the tile); the rows of T are
// read four columns at a time
template <int DC, int R>
__device__ __forceinline__ void tile_rows_times(const float *T, const float *B, int n, const int (&i)[R], int c4, float4 (&acc)[R]) {
  constexpr int LDC = DC + 4;
#pragma unroll
  for (int x = 0; x < R; ++x) acc[x] = make_float4(0.f, 0.f, 0.f, 0.f);
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld4(B + (j + u) * LDC + c4);
#pragma unroll
    for (int x = 0; x < R; ++x) {
      const float4 p = ld4(T + i[x] * kLdt + j);
      fma4(acc[x], p.x, v[0]); fma4(acc[x], p.y, v[1]); fma4(acc[x], p.z, v[2]); fma4(acc[x], p.w, v[3]);
    }
  }
  for (; j < n; ++j) {
    const float4 v = ld4(B + j * LDC + c4);
#pragma unroll
    for (int x = 0; x < R; ++x) fma4(acc[x], T[i[x] * kLdt + j], v);
  }
}

// acc[u] = sum_{i < n} T[i, j0 + u] * A[i][c4 .. c4 + 4), i ascending, for the four columns j0 .. j0 + 3 of T (j0 % 4 == 0; a
// column past the tile's k reads the row's padding: its sum is not stored)
template <int DC> __device__ __forceinline__ void tile_cols_times(const float *T, const float *A, int n, int j0, int c4, float4 (&acc)[4]) {
  constexpr int LDC = DC + 4;
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = 0; i < n; ++i) {
    const float4 p = ld4(T + i * kLdt + j0);
    const float4 v = ld4(A + i * LDC + c4);
    fma4(acc[0], p.x, v); fma4(acc[1], p.y, v); fma4(acc[2], p.z, v); fma4(acc[3], p.w, v);
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {   // xor butterfly: both sides of a pair add the same two operands
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

struct Own {       // the 4 x 8 entries of a [q, k] tile that a thread of the 16 x 16 grid owns
  int i[4], j[8];    // true indices (may lie outside the tile)
  int ia[4], jb[8];  // clamped into the tile: operands of entries that are not stored
};
__device__ __forceinline__ Own own_entries(int q, int k) {
  Own o;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int a = 0; a < 4; ++a) { o.i[a] = ty + 16 * a; o.ia[a] = min(o.i[a], q - 1); }
#pragma unroll
  for (int b = 0; b < 8; ++b) { o.j[b] = tx + 16 * b; o.jb[b] = min(o.j[b], k - 1); }
  return o;
}

__device__ __forceinline__ void store_tile(float *T, const Own &o, int q, int k, const float (&acc)[4][8]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b)
      if (o.i[a] < q && o.j[b] < k) T[o.i[a] * kLdt + o.j[b]] = acc[a][b];
}

// S of sequence n, head h into T (every thread must call; ends behind a barrier)
template <int DC>
__device__ __forceinline__ void scores(const TxlArgs &a, int64_t n, int h, const Own &o, float *T, float *A0, float *A1, float *B0,
                                       float *B1) {
  const int q = a.q, k = a.k, dh = a.dh, m = k - q;
  const int64_t ld = (int64_t)a.nh * dh;
  const float *Qn = a.Q + n * q * ld + h * dh, *Kn = a.K + n * k * ld + h * dh, *Rh = a.R + h * dh;
  const float *bw = a.bw + h * dh, *br = a.br + h * dh;
  float ac[4][8], bd[4][8];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 8; ++y) ac[x][y] = bd[x][y] = 0.f;
  for (int c0 = 0; c0 < dh; c0 += DC) {
    __syncthreads();
    stage<DC>(A0, Qn + c0, ld, q, bw + c0);
    stage<DC>(A1, Qn + c0, ld, q, br + c0);
    stage<DC>(B0, Kn + c0, ld, k, nullptr);
    stage<DC>(B1, Rh + c0, ld, k, nullptr);
    __syncthreads();
    nt_acc<DC>(A0, B0, o.ia, o.jb, ac);
    nt_acc<DC>(A1, B1, o.ia, o.jb, bd);
  }
  store_tile(T, o, q, k, bd);
  __syncthreads();
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      const int i = o.i[x], j = o.j[y];
      float s = 0.f;
      if (i < q && j < k) {
        const int d = j - i;
        if (d < m + 1) s = T[i * kLdt + (q - 1 - i + j)];
        else if (d > m + 1) s = T[(i + 1) * kLdt + (d - m - 2)];
      }
      ac[x][y] = (ac[x][y] + s) * a.scale;
    }
  __syncthreads();
  store_tile(T, o, q, k, ac);
  __syncthreads();
}

template <int DC> __host__ __device__ constexpr int txl_lds_floats(int q, int k, int tiles, int abufs) {
  return tiles * q * kLdt + abufs * q * (DC + 4) + 2 * k * (DC + 4);
}

// ----------------------------------------------------------------------------- forward: grid N * nh
template <int DC>
__global__ void __launch_bounds__(kBlock) txl_fwd_k(TxlArgs a, float *__restrict__ O, float *__restrict__ rmax, float *__restrict__ rsum) {
  extern __shared__ float4 txl_lds[];
  constexpr int LDC = DC + 4, G = DC / 4, RP = kBlock / G, NR = kTxlMaxQ / RP;
  const int q = a.q, k = a.k, dh = a.dh;
  float *T = reinterpret_cast<float *>(txl_lds);
  float *A0 = T + q * kLdt, *A1 = A0 + q * LDC, *B0 = A1 + q * LDC, *B1 = B0 + k * LDC;
  const int h = (int)(blockIdx.x % a.nh);
  const int64_t n = blockIdx.x / a.nh;
  const int64_t ld = (int64_t)a.nh * dh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Own o = own_entries(q, k);
  scores<DC>(a, n, h, o, T, A0, A1, B0, B1);

  for (int i = wave; i < q; i += kBlock / kWave) {     // softmax of row i in place
    float *t = T + i * kLdt;
    const bool in0 = lane < k, in1 = lane + kWave < k;
    const float s0 = in0 ? t[lane] : -INFINITY, s1 = in1 ? t[lane + kWave] : -INFINITY;
    const float mx = wave_max(fmaxf(s0, s1));
    const float e0 = in0 ? expf(s0 - mx) : 0.f, e1 = in1 ? expf(s1 - mx) : 0.f;
    const float sum = wave_sum(e0 + e1);
    if (in0) t[lane] = e0 / sum;
    if (in1) t[lane + kWave] = e1 / sum;
    if (lane == 0) {
      const int64_t r = (n * a.nh + h) * q + i;
      rmax[r] = mx;
      rsum[r] = sum;
    }
  }

  const float *Vn = a.V + n * k * ld + h * dh;
  float *On = O + n * q * ld + h * dh;
  const int tx = threadIdx.x % G, ty = threadIdx.x / G;
  int rows[NR];                                        // the rows ty + RP x this thread owns, clamped into the tile
#pragma unroll
  for (int x = 0; x < NR; ++x) rows[x] = min(ty + RP * x, q - 1);
  for (int c0 = 0; c0 < dh; c0 += DC) {
    __syncthreads();
    stage<DC>(B0, Vn + c0, ld, k, nullptr);
    __syncthreads();
    float4 acc[NR];
    tile_rows_times<DC, NR>(T, B0, k, rows, tx * 4, acc);
#pragma unroll
    for (int x = 0; x < NR; ++x)
      if (ty + RP * x < q) st4(On + (int64_t)(ty + RP * x) * ld + c0 + tx * 4, acc[x]);
  }
}

// ----------------------------------------------------------------------------- backward: grid groups * nh
template <int DC>
__global__ void __launch_bounds__(kBlock) txl_bwd_k(TxlArgs a, const float *__restrict__ dO, const float *__restrict__ rmax,
                                                    const float *__restrict__ rsum, int groups, float *__restrict__ dQ,
                                                    float *__restrict__ dK, float *__restrict__ dV, float *__restrict__ partial) {
  extern __shared__ float4 txl_lds[];
  constexpr int LDC = DC + 4, G = DC / 4, RP = kBlock / G, NR = kTxlMaxQ / RP;
  const int q = a.q, k = a.k, dh = a.dh, nh = a.nh;
  float *T1 = reinterpret_cast<float *>(txl_lds), *T2 = T1 + q * kLdt;
  float *A0 = T2 + q * kLdt, *A1 = A0 + q * LDC, *A2 = A1 + q * LDC, *B0 = A2 + q * LDC, *B1 = B0 + k * LDC;
  const int h = (int)(blockIdx.x % nh), g = (int)(blockIdx.x / nh);
  const int64_t ld = (int64_t)nh * dh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = threadIdx.x % G, ty = threadIdx.x / G;
  const Own o = own_entries(q, k);
  int rows[NR];                                        // the rows ty + RP x this thread owns, clamped into the tile
#pragma unroll
  for (int x = 0; x < NR; ++x) rows[x] = min(ty + RP * x, q - 1);
  float *part = partial + (int64_t)g * (k + 2) * ld + h * dh;     // rows 0 .. k-1: dR, row k: d r_w_bias, row k + 1: d r_r_bias
  const float *bw = a.bw + h * dh, *br = a.br + h * dh;

  for (int64_t n = g; n < a.N; n += groups) {
    const bool first = n == g;
    const float *Qn = a.Q + n * q * ld + h * dh, *Kn = a.K + n * k * ld + h * dh, *Vn = a.V + n * k * ld + h * dh;
    const float *dOn = dO + n * q * ld + h * dh;
    scores<DC>(a, n, h, o, T1, A0, A1, B0, B1);

    for (int i = wave; i < q; i += kBlock / kWave) {   // P of row i in place, as the forward computed it
      float *t = T1 + i * kLdt;
      const int64_t r = (n * nh + h) * q + i;
      const float mx = rmax[r], sum = rsum[r];
      if (lane < k) t[lane] = expf(t[lane] - mx) / sum;
      if (lane + kWave < k) t[lane + kWave] = expf(t[lane + kWave] - mx) / sum;
    }

    {                                                  // dP = dO V^T -> T2
      float acc[4][8];
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 8; ++y) acc[x][y] = 0.f;
      for (int c0 = 0; c0 < dh; c0 += DC) {
        __syncthreads();
        stage<DC>(A0, dOn + c0, ld, q, nullptr);
        stage<DC>(B0, Vn + c0, ld, k, nullptr);
        __syncthreads();
        nt_acc<DC>(A0, B0, o.ia, o.jb, acc);
      }
      store_tile(T2, o, q, k, acc);
    }
    __syncthreads();

    for (int i = wave; i < q; i += kBlock / kWave) {   // dS = scale * P * (dP - sum_j P dP) in place of dP
      const float *p = T1 + i * kLdt;
      float *t = T2 + i * kLdt;
      const bool in0 = lane < k, in1 = lane + kWave < k;
      const float p0 = in0 ? p[lane] : 0.f, p1 = in1 ? p[lane + kWave] : 0.f;
      const float d0 = in0 ? t[lane] : 0.f, d1 = in1 ? t[lane + kWave] : 0.f;
      const float delta = wave_sum(fmaf(p1, d1, p0 * d0));
      if (in0) t[lane] = a.scale * (p0 * (d0 - delta));
      if (in1) t[lane + kWave] = a.scale * (p1 * (d1 - delta));
    }

    for (int c0 = 0; c0 < dh; c0 += DC) {              // dV = P^T dO,  dK = dS^T (Q + r_w_bias)
      __syncthreads();
      stage<DC>(A0, dOn + c0, ld, q, nullptr);
      stage<DC>(A1, Qn + c0, ld, q, bw + c0);
      __syncthreads();
      for (int j0 = 4 * ty; j0 < k; j0 += 4 * RP) {
        float4 gv[4], gk[4];
        tile_cols_times<DC>(T1, A0, q, j0, tx * 4, gv);
        tile_cols_times<DC>(T2, A1, q, j0, tx * 4, gk);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u < k) {
            const int64_t off = (n * k + j0 + u) * ld + h * dh + c0 + tx * 4;
            st4(dV + off, gv[u]);
            st4(dK + off, gk[u]);
          }
      }
    }
    __syncthreads();

    for (int e = threadIdx.x; e < q * k; e += kBlock) {   // dBD = shift^T(dS) -> T1
      const int i = e / k, p = e % k, t = i + 1 + p - q;
      float v = 0.f;
      if (t >= 0) v = T2[i * kLdt + t];
      else if (i >= 1) v = T2[(i - 1) * kLdt + t + k];
      T1[i * kLdt + p] = v;
    }

    for (int c0 = 0; c0 < dh; c0 += DC) {              // dR += dBD^T (Q + r_r_bias),  dQ = dS K + dBD R,  bias gradients
      __syncthreads();
      stage<DC>(A0, Qn + c0, ld, q, br + c0);
      stage<DC>(B0, Kn + c0, ld, k, nullptr);
      stage<DC>(B1, a.R + h * dh + c0, ld, k, nullptr);
      __syncthreads();
      for (int j0 = 4 * ty; j0 < k; j0 += 4 * RP) {
        float4 gr[4];
        tile_cols_times<DC>(T1, A0, q, j0, tx * 4, gr);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u < k) {
            float4 v = gr[u];
            float *pp = part + (int64_t)(j0 + u) * ld + c0 + tx * 4;
            if (!first) {
              const float4 w = ld4(pp);
              v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
            }
            st4(pp, v);
          }
      }
      {
        float4 gac[NR], gbd[NR];
        tile_rows_times<DC, NR>(T2, B0, k, rows, tx * 4, gac);
        tile_rows_times<DC, NR>(T1, B1, k, rows, tx * 4, gbd);
#pragma unroll
        for (int x = 0; x < NR; ++x) {
          const int i = ty + RP * x;
          if (i < q) {
            const float4 u = gac[x], v = gbd[x];
            st4(A1 + i * LDC + tx * 4, u);
            st4(A2 + i * LDC + tx * 4, v);
            st4(dQ + (n * q + i) * ld + h * dh + c0 + tx * 4, make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w));
          }
        }
      }
      __syncthreads();
      if (threadIdx.x < 2 * DC) {                      // column sums over the q rows, ascending
        const int which = threadIdx.x / DC, c = threadIdx.x % DC;
        const float *src = which ? A2 : A1;
        float s = 0.f;
        for (int i = 0; i < q; ++i) s += src[i * LDC + c];
        float *pp = part + (int64_t)(k + which) * ld + c0 + c;
        if (!first) s += *pp;
        *pp = s;
      }
    }
    __syncthreads();
  }
}

bool txl_shape_ok(int q, int k, int dh) {
  return q >= 1 && q <= kTxlMaxQ && k >= q && k <= kTxlMaxK && (dh == 16 || dh == 32 || dh == 64 || dh == 128);
}

int txl_groups(int64_t N, int nh) {
  const int64_t cap = kTxlGroups / nh > 0 ? kTxlGroups / nh : 1;
  return (int)(N < cap ? N : cap);
}

template <int DC>
int txl_fwd_launch(const TxlArgs &a, float *O, float *rmax, float *rsum, hipStream_t st) {
  static bool done[kMaxDevices] = {};
  constexpr int kMaxBytes = 4 * txl_lds_floats<DC>(kTxlMaxQ, kTxlMaxK, 1, 2);
  if (!opt_in_lds(reinterpret_cast<const void *>(&txl_fwd_k<DC>), kMaxBytes, done)) return DMP_ERR_HIP;
  const size_t bytes = sizeof(float) * (size_t)txl_lds_floats<DC>(a.q, a.k, 1, 2);
  txl_fwd_k<DC><<<(unsigned)(a.N * a.nh), kBlock, bytes, st>>>(a, O, rmax, rsum);
  return check_launch();
}

template <int DC>
int txl_bwd_launch(const TxlArgs &a, const float *dO, const float *rmax, const float *rsum, float *dQ, float *dK, float *dV,
                   float *partial, hipStream_t st) {
  static bool done[kMaxDevices] = {};
  constexpr int kMaxBytes = 4 * txl_lds_floats<DC>(kTxlMaxQ, kTxlMaxK, 2, 3);
  if (!opt_in_lds(reinterpret_cast<const void *>(&txl_bwd_k<DC>), kMaxBytes, done)) return DMP_ERR_HIP;
  const size_t bytes = sizeof(float) * (size_t)txl_lds_floats<DC>(a.q, a.k, 2, 3);
  const int groups = txl_groups(a.N, a.nh);
  txl_bwd_k<DC><<<(unsigned)(groups * a.nh), kBlock, bytes, st>>>(a, dO, rmax, rsum, groups, dQ, dK, dV, partial);
  return check_launch();
}

static_assert(4 * txl_lds_floats<32>(kTxlMaxQ, kTxlMaxK, 2, 3) <= 160 * 1024, "the backward's LDS exceeds a CU's 160 KiB");

int txl_check(const float *Q, const float *K, const float *V, const float *R, const float *bw, const float *br, int64_t N, int q, int k,
              int nh, int dh) {
  if (N < 0 || q < 1 || k < 1 || nh < 1 || dh < 1) return DMP_ERR_BAD_ARG;
  if (!txl_shape_ok(q, k, dh) || N * nh >= ((int64_t)1 << 31) || N * k * nh * dh >= ((int64_t)1 << 40)) return DMP_ERR_UNSUPPORTED;
  if (N == 0) return DMP_OK;
  if (!Q || !K || !V || !R || !bw || !br) return DMP_ERR_BAD_ARG;
  if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(R) || !aligned16(bw) || !aligned16(br)) return DMP_ERR_UNSUPPORTED;
  return DMP_OK;
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_txl_supported(int q, int k, int dh) { return txl_shape_ok(q, k, dh) ? 1 : 0; }

int64_t dmp_txl_bwd_groups(int64_t N, int nh) { return N < 1 || nh < 1 ? 0 : txl_groups(N, nh); }

int dmp_txl_attn_fwd(const float *Q, const float *K, const float *V, const float *R, const float *r_w_bias, const float *r_r_bias,
                     int64_t N, int q, int k, int nh, int dh, float scale, float *O, float *rowmax, float *rowsum, void *stream) {
  const int rc = txl_check(Q, K, V, R, r_w_bias, r_r_bias, N, q, k, nh, dh);
  if (rc != DMP_OK || N == 0) return rc;
  if (!O || !rowmax || !rowsum) return DMP_ERR_BAD_ARG;
  if (!aligned16(O)) return DMP_ERR_UNSUPPORTED;
  const TxlArgs a{Q, K, V, R, r_w_bias, r_r_bias, N, q, k, nh, dh, scale};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dh == 16 ? txl_fwd_launch<16>(a, O, rowmax, rowsum, st) : txl_fwd_launch<32>(a, O, rowmax, rowsum, st);
}

int dmp_txl_attn_bwd(const float *Q, const float *K, const float *V, const float *R, const float *r_w_bias, const float *r_r_bias,
                     const float *dO, const float *rowmax, const float *rowsum, int64_t N, int q, int k, int nh, int dh, float scale,
                     float *dQ, float *dK, float *dV, float *partial, void *stream) {
  const int rc = txl_check(Q, K, V, R, r_w_bias, r_r_bias, N, q, k, nh, dh);
  if (rc != DMP_OK || N == 0) return rc;
  if (!dO || !rowmax || !rowsum || !dQ || !dK || !dV || !partial) return DMP_ERR_BAD_ARG;
  if (!aligned16(dO) || !aligned16(dQ) || !aligned16(dK) || !aligned16(dV) || !aligned16(partial)) return DMP_ERR_UNSUPPORTED;
  const TxlArgs a{Q, K, V, R, r_w_bias, r_r_bias, N, q, k, nh, dh, scale};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dh == 16 ? txl_bwd_launch<16>(a, dO, rowmax, rowsum, dQ, dK, dV, partial, st)
                  : txl_bwd_launch<32>(a, dO, rowmax, rowsum, dQ, dK, dV, partial, st);
}

}  // extern "C"
