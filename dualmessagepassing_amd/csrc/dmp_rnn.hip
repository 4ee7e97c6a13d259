// The RNN rep-net layer of the edge-sequence models (SubgraphCountingMatching/models/rnn.py:13-52): one-layer nn.LSTM,
// nn.GRU or nn.RNN (tanh), uni- or bidirectional, batch first, on rows X [B, L, Hin].  Hd = hidden size per direction
// (32, 64 or 128), G gates (LSTM 4: i f g o, GRU 3: r z n, RNN 1), D directions.
//
// The input projection P [B, L, D, G Hd] = X W_ihᵀ + b is one GEMM on the host side (LSTM / RNN: b = b_ih + b_hh; GRU
// keeps b_hn out of P, it sits inside r * (W_hn h + b_hn)).  What is here is the time recurrence:
//
// Forward (dmp_rnn_fwd): grid (batch tiles of kS sequences, D), one workgroup runs all L steps of its tile in its
// direction (direction 1 walks the positions from L - 1 down).  Thread r < G Hd owns row r of W_hh in registers (Hd
// floats) for the whole launch; h_{t-1} of the tile sits in LDS.  Per step:
//   1. each row thread: pre = P[t, r] + W_hh[r] . h_{t-1} for the kS sequences (an fma chain in k order, h read as
//      float4 broadcasts), the gate's activation, -> LDS; P of the next step is prefetched into registers;
//   2. barrier; each (sequence, unit) item: the cell (LSTM c = f c + i g, h = o tanh c; GRU n = tanh(P_n + r hn),
//      h = n + z (h_{t-1} - n); RNN h = tanh(pre)), h -> the other LDS buffer, Y = h * gate (+ resid) into the
//      direction's half of [B, L, D Hd], h and the cell values the backward needs into H and S; barrier.
// The recurrence runs over every position, padding and gated holes included (their inputs are zero), as the module does.
//
// Backward (dmp_rnn_bwd): the same grid, the reverse-time recurrence in one launch.  Thread (g, k), g < G, k < Hd, owns
// column k of gate block g of W_hh (Hd floats).  Per step (latest time first):
//   1. each (sequence, unit) item: dh = dY gate + sum over g of the block partials of the step after (fixed g order)
//      (+ dh z for GRU); the cell's backward (LSTM carries dc) -> the pre-activation gradients dG into LDS and into
//      dG [B, L, D, NG Hd] (LSTM dGi dGf dGg dGo; GRU dGr dGz dGn d(W_hn h + b_hn); RNN dG); the next step's loads are
//      issued after the barrier;
//   2. barrier; each (g, k) thread: partial[g][k] = sum_j W_hh[g Hd + j][k] dG_rec[g Hd + j] (j in order); barrier.
// dX, dW_ih, dW_hh and the biases are GEMMs and column sums of dG on the host side.  No float atomics anywhere: two runs
// are bitwise equal.  The workgroups are independent: the batch is the only axis split across them.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kS = 4;   // sequences per workgroup

template <int CELL> struct CellInfo;
template <> struct CellInfo<0> { static constexpr int G = 4, NS = 5, NG = 4; };   // LSTM: saves i f g o c
template <> struct CellInfo<1> { static constexpr int G = 3, NS = 4, NG = 4; };   // GRU: saves r z n hn
template <> struct CellInfo<2> { static constexpr int G = 1, NS = 0, NG = 1; };   // RNN: h only

template <int CELL, int HD> constexpr int threads_of() { return ((CellInfo<CELL>::G * HD + 63) / 64) * 64; }

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

struct RnnFwdArgs {
  const float *P, *Whh, *bhn, *gate, *resid;
  float *Y, *H, *S;
  int64_t B;
  int L, D;
};

template <int CELL, int HD>
__global__ __launch_bounds__((threads_of<CELL, HD>())) void rnn_fwd_kernel(RnnFwdArgs a) {
  constexpr int G = CellInfo<CELL>::G, NS = CellInfo<CELL>::NS, GH = G * HD, NT = threads_of<CELL, HD>();
  constexpr int PW = (kS * HD + NT - 1) / NT;         // (sequence, unit) items per thread
  constexpr int GW = CELL == 1 ? 4 * HD : GH;         // GRU: r z hn P_n
  __shared__ __attribute__((aligned(16))) float hs[2][kS][HD];
  __shared__ float gs[kS][GW];
  __shared__ float cs[kS][HD];
  const int tid = threadIdx.x, d = blockIdx.y, D = a.D, L = a.L;
  const int64_t b0 = (int64_t)blockIdx.x * kS;
  const bool row = tid < GH;
  const int r = row ? tid : 0;

  float w[HD];
  {
    const float4 *wr = reinterpret_cast<const float4 *>(a.Whh + ((int64_t)d * GH + r) * HD);
#pragma unroll
    for (int k = 0; k < HD / 4; ++k) {
      const float4 v = wr[k];
      w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
  }
  const float bh = (CELL == 1 && row && r >= 2 * HD) ? a.bhn[d * HD + r - 2 * HD] : 0.f;
  for (int e = tid; e < kS * HD; e += NT) {
    (&hs[0][0][0])[e] = 0.f;
    (&cs[0][0])[e] = 0.f;
  }
  const int64_t ldp = (int64_t)D * GH, ldy = (int64_t)D * HD;
  auto pos = [&](int t) { return d == 0 ? t : L - 1 - t; };
  auto load_p = [&](float *pv, int t) {
    const int p = pos(t);
#pragma unroll
    for (int s = 0; s < kS; ++s) {
      const int64_t b = b0 + s;
      pv[s] = (row && b < a.B) ? a.P[(b * L + p) * ldp + (int64_t)d * GH + r] : 0.f;
    }
  };
  auto load_gr = [&](float *gv, float *rv, int t) {
    const int p = pos(t);
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int e = tid + i * NT, s = e / HD, j = e % HD;
      const int64_t b = b0 + s;
      const bool ok = e < kS * HD && b < a.B;
      gv[i] = (ok && a.gate) ? a.gate[b * L + p] : 1.f;
      rv[i] = (ok && a.resid) ? a.resid[(b * L + p) * ldy + (int64_t)d * HD + j] : 0.f;
    }
  };
  float pc[kS], gv[PW], rv[PW];
  load_p(pc, 0);
  load_gr(gv, rv, 0);
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const int p = pos(t), cur = t & 1;
    if (row) {
#pragma unroll
      for (int s = 0; s < kS; ++s) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < HD; k += 4) {
          const float4 hv = *reinterpret_cast<const float4 *>(&hs[cur][s][k]);
          acc = fmaf(w[k], hv.x, acc);
          acc = fmaf(w[k + 1], hv.y, acc);
          acc = fmaf(w[k + 2], hv.z, acc);
          acc = fmaf(w[k + 3], hv.w, acc);
        }
        if constexpr (CELL == 0) {
          const float v = pc[s] + acc;
          gs[s][r] = (r >= 2 * HD && r < 3 * HD) ? tanhf(v) : sigmoidf(v);
        } else if constexpr (CELL == 1) {
          if (r < 2 * HD) {
            gs[s][r] = sigmoidf(pc[s] + acc);
          } else {
            gs[s][r] = acc + bh;          // hn = W_hn h + b_hn
            gs[s][r + HD] = pc[s];           // P_n = W_in x + b_in
          }
        } else {
          gs[s][r] = tanhf(pc[s] + acc);
        }
      }
    }
    __syncthreads();
    if (t + 1 < L) load_p(pc, t + 1);
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int e = tid + i * NT;
      if (e >= kS * HD) break;
      const int s = e / HD, j = e % HD;
      float h, sv[NS > 0 ? NS : 1];
      if constexpr (CELL == 0) {
        const float ig = gs[s][j], fg = gs[s][HD + j], gg = gs[s][2 * HD + j], og = gs[s][3 * HD + j];
        const float c = fg * cs[s][j] + ig * gg;
        h = og * tanhf(c);
        cs[s][j] = c;
        sv[0] = ig; sv[1] = fg; sv[2] = gg; sv[3] = og; sv[4] = c;
      } else if constexpr (CELL == 1) {
        const float rg = gs[s][j], zg = gs[s][HD + j], hn = gs[s][2 * HD + j], pn = gs[s][3 * HD + j];
        const float n = tanhf(pn + rg * hn);
        h = n + zg * (hs[cur][s][j] - n);
        sv[0] = rg; sv[1] = zg; sv[2] = n; sv[3] = hn;
      } else {
        h = gs[s][j];
      }
      hs[cur ^ 1][s][j] = h;
      const int64_t b = b0 + s;
      if (b < a.B) {
        const int64_t o = (b * L + p) * ldy + (int64_t)d * HD + j;
        a.Y[o] = h * gv[i] + rv[i];
        a.H[o] = h;
        if constexpr (NS > 0) {
          float *so = a.S + ((b * L + p) * D + d) * (int64_t)(NS * HD) + j;
#pragma unroll
          for (int q = 0; q < NS; ++q) so[q * HD] = sv[q];
        }
      }
    }
    if (t + 1 < L) load_gr(gv, rv, t + 1);
    __syncthreads();
  }
}

struct RnnBwdArgs {
  const float *dY, *gate, *Whh, *H, *S;
  float *dG;
  int64_t B;
  int L, D;
};

template <int CELL, int HD>
__global__ __launch_bounds__((threads_of<CELL, HD>())) void rnn_bwd_kernel(RnnBwdArgs a) {
  constexpr int G = CellInfo<CELL>::G, NS = CellInfo<CELL>::NS, NG = CellInfo<CELL>::NG, GH = G * HD;
  constexpr int NT = threads_of<CELL, HD>(), PW = (kS * HD + NT - 1) / NT;
  constexpr int NV = CELL == 0 ? 8 : CELL == 1 ? 7 : 3;   // loads per item: dY gate, then the cell's values
  __shared__ __attribute__((aligned(16))) float dgs[kS][GH];   // the recurrent gradient vector of the step
  __shared__ float parts[kS][G][HD];
  __shared__ float carry[kS][HD];                               // LSTM dc, GRU dh z
  const int tid = threadIdx.x, d = blockIdx.y, D = a.D, L = a.L;
  const int64_t b0 = (int64_t)blockIdx.x * kS;
  const bool col = tid < GH;
  const int g = col ? tid / HD : 0, k = col ? tid % HD : 0;

  float w[HD];
  {
    const float *wc = a.Whh + ((int64_t)d * GH + g * HD) * HD + k;
#pragma unroll
    for (int j = 0; j < HD; ++j) w[j] = wc[(int64_t)j * HD];
  }
  for (int e = tid; e < kS * G * HD; e += NT) (&parts[0][0][0])[e] = 0.f;
  for (int e = tid; e < kS * HD; e += NT) (&carry[0][0])[e] = 0.f;
  const int64_t ldy = (int64_t)D * HD;
  auto pos = [&](int t) { return d == 0 ? t : L - 1 - t; };
  // v: dY, gate, then LSTM i f g o c c_prev / GRU r z n hn h_prev / RNN h
  auto load = [&](float (*v)[NV], int t) {
    const int p = pos(t);
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int e = tid + i * NT, s = e / HD, j = e % HD;
      const int64_t b = b0 + s;
      const bool ok = e < kS * HD && b < a.B;
#pragma unroll
      for (int q = 0; q < NV; ++q) v[i][q] = 0.f;
      if (!ok) continue;
      const int64_t o = (b * L + p) * ldy + (int64_t)d * HD + j;
      v[i][0] = a.dY[o];
      v[i][1] = a.gate ? a.gate[b * L + p] : 1.f;
      if constexpr (CELL == 2) {
        v[i][2] = a.H[o];
      } else {
        const float *so = a.S + ((b * L + p) * D + d) * (int64_t)(NS * HD) + j;
#pragma unroll
        for (int q = 0; q < NS; ++q) v[i][2 + q] = so[q * HD];
        if (t > 0) {
          const int pp = pos(t - 1);
          v[i][NV - 1] = CELL == 0 ? a.S[((b * L + pp) * D + d) * (int64_t)(NS * HD) + 4 * HD + j]
                                   : a.H[(b * L + pp) * ldy + (int64_t)d * HD + j];
        }
      }
    }
  };
  float v[PW][NV];
  load(v, L - 1);
  __syncthreads();

  for (int t = L - 1; t >= 0; --t) {
    const int p = pos(t);
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int e = tid + i * NT;
      if (e >= kS * HD) break;
      const int s = e / HD, j = e % HD;
      float dh = v[i][0] * v[i][1];
#pragma unroll
      for (int q = 0; q < G; ++q) dh += parts[s][q][j];
      float out[NG];
      if constexpr (CELL == 0) {
        const float ig = v[i][2], fg = v[i][3], gg = v[i][4], og = v[i][5], c = v[i][6], cp = v[i][7];
        const float tc = tanhf(c);
        const float dc = carry[s][j] + dh * og * (1.f - tc * tc);
        carry[s][j] = dc * fg;
        out[0] = dc * gg * ig * (1.f - ig);
        out[1] = dc * cp * fg * (1.f - fg);
        out[2] = dc * ig * (1.f - gg * gg);
        out[3] = dh * tc * og * (1.f - og);
#pragma unroll
        for (int q = 0; q < 4; ++q) dgs[s][q * HD + j] = out[q];
      } else if constexpr (CELL == 1) {
        dh += carry[s][j];
        const float rg = v[i][2], zg = v[i][3], n = v[i][4], hn = v[i][5], hp = v[i][6];
        carry[s][j] = dh * zg;
        const float dn = dh * (1.f - zg) * (1.f - n * n);
        out[0] = dn * hn * rg * (1.f - rg);
        out[1] = dh * (hp - n) * zg * (1.f - zg);
        out[2] = dn;
        out[3] = dn * rg;
        dgs[s][j] = out[0];
        dgs[s][HD + j] = out[1];
        dgs[s][2 * HD + j] = out[3];
      } else {
        const float h = v[i][2];
        out[0] = dh * (1.f - h * h);
        dgs[s][j] = out[0];
      }
      const int64_t b = b0 + s;
      if (b < a.B) {
        float *go = a.dG + ((b * L + p) * D + d) * (int64_t)(NG * HD) + j;
#pragma unroll
        for (int q = 0; q < NG; ++q) go[q * HD] = out[q];
      }
    }
    __syncthreads();
    if (t > 0) load(v, t - 1);
    if (col) {
#pragma unroll
      for (int s = 0; s < kS; ++s) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < HD; j += 4) {
          const float4 dv = *reinterpret_cast<const float4 *>(&dgs[s][g * HD + j]);
          acc = fmaf(w[j], dv.x, acc);
          acc = fmaf(w[j + 1], dv.y, acc);
          acc = fmaf(w[j + 2], dv.z, acc);
          acc = fmaf(w[j + 3], dv.w, acc);
        }
        parts[s][g][k] = acc;
      }
    }
    __syncthreads();
  }
}

template <template <int, int> class K, typename Args>
int launch(int cell, int Hd, dim3 grid, hipStream_t stream, const Args &a);

template <int CELL, int HD>
struct FwdK {
  static void go(dim3 grid, hipStream_t st, const RnnFwdArgs &a) {
    hipLaunchKernelGGL((rnn_fwd_kernel<CELL, HD>), grid, dim3(threads_of<CELL, HD>()), 0, st, a);
  }
};
template <int CELL, int HD>
struct BwdK {
  static void go(dim3 grid, hipStream_t st, const RnnBwdArgs &a) {
    hipLaunchKernelGGL((rnn_bwd_kernel<CELL, HD>), grid, dim3(threads_of<CELL, HD>()), 0, st, a);
  }
};

template <template <int, int> class K, int CELL, typename Args>
void launch_hd(int Hd, dim3 grid, hipStream_t st, const Args &a) {
  if (Hd == 32) K<CELL, 32>::go(grid, st, a);
  else if (Hd == 64) K<CELL, 64>::go(grid, st, a);
  else K<CELL, 128>::go(grid, st, a);
}

template <template <int, int> class K, typename Args>
int launch(int cell, int Hd, dim3 grid, hipStream_t st, const Args &a) {
  if (cell == 0) launch_hd<K, 0>(Hd, grid, st, a);
  else if (cell == 1) launch_hd<K, 1>(Hd, grid, st, a);
  else launch_hd<K, 2>(Hd, grid, st, a);
  return check_launch();
}

bool shape_ok(int64_t B, int64_t L, int D, int Hd, int cell) {
  return B >= 0 && L >= 1 && L < ((int64_t)1 << 31) && (D == 1 || D == 2) && (Hd == 32 || Hd == 64 || Hd == 128) && cell >= 0 &&
         cell <= 2;
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_rnn_fwd(const float *P, const float *Whh, const float *bhn, const float *gate, const float *resid, int64_t B, int64_t L,
                int D, int Hd, int cell, float *Y, float *H, float *S, void *stream) {
  if (!shape_ok(B, L, D, Hd, cell)) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!P || !Whh || !Y || !H || !aligned16(Whh) || (cell != 2 && !S) || (cell == 1 && !bhn)) return DMP_ERR_BAD_ARG;
  if ((B + kS - 1) / kS >= ((int64_t)1 << 31)) return DMP_ERR_UNSUPPORTED;
  RnnFwdArgs a{P, Whh, bhn, gate, resid, Y, H, S, B, (int)L, D};
  return launch<FwdK>(cell, Hd, dim3((unsigned)((B + kS - 1) / kS), (unsigned)D), static_cast<hipStream_t>(stream), a);
}

int dmp_rnn_bwd(const float *dY, const float *gate, const float *Whh, const float *H, const float *S, int64_t B, int64_t L, int D,
                int Hd, int cell, float *dG, void *stream) {
  if (!shape_ok(B, L, D, Hd, cell)) return DMP_ERR_BAD_ARG;
  if (B == 0) return DMP_OK;
  if (!dY || !Whh || !H || !dG || (cell != 2 && !S)) return DMP_ERR_BAD_ARG;
  if ((B + kS - 1) / kS >= ((int64_t)1 << 31)) return DMP_ERR_UNSUPPORTED;
  RnnBwdArgs a{dY, gate, Whh, H, S, dG, B, (int)L, D};
  return launch<BwdK>(cell, Hd, dim3((unsigned)((B + kS - 1) / kS), (unsigned)D), static_cast<hipStream_t>(stream), a);
}

}  // extern "C"
