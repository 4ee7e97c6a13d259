// What an evaluation batch leaves behind, on the device: dmp_eval_terms (include/dmp_hip.h).
//
// One workgroup of 16 waves walks the batch in chunks of 1024 pairs, one pair per thread.  Per chunk:
//   1. a thread's pair is real when pair_w says so; its result row = cursor + (real pairs before it): the wave's ballot
//      gives the count inside the wave, sixteen wave totals in LDS the count of the waves before it, a running total the
//      chunks before.  The thread writes pred_out / target_out of its row and adds its error terms to four fp64 partial
//      sums of its own;
//   2. per matching head, groups of G = min(64, pow2 >= Lc) lanes take the chunk's real pairs in turn: a lane adds the
//      |relu(pred) - float(w)| of its columns j = lane, lane + G, ... in fp32, a shuffle tree folds the G lane sums, lane 0
//      of the group writes err_out of the row.
// After the last chunk the partial sums are folded (a shuffle tree per wave, the sixteen wave sums in wave order by thread 0)
// and thread 0 adds them to sums[], raises the overflow word when cursor + real > cap, and advances the cursor.  Every order
// of summation is fixed by (n, Lc) alone: the same bits on every launch.  Rows at or beyond cap are never written.  No
// atomics: a pass's launches are ordered by their stream.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kEvalThreads = 1024;
constexpr int kEvalWaves = kEvalThreads / kWave;

struct EvalHead {
  const float *pred;
  const int64_t *w;
  float *err;
  int64_t ld;
  int Lc, G;      // G: lanes per row, a power of two in [1, 64]
};

// torch's relu: NaN stays NaN, everything else that is not positive gives +0
__device__ __forceinline__ float relu_t(float p) { return p > 0.f ? p : (p == p ? 0.f : p); }

__global__ __launch_bounds__(kEvalThreads) void eval_terms_k(const float *__restrict__ pred_c, const float *__restrict__ target,
                                                             const float *__restrict__ pair_w, int64_t n, EvalHead h0, EvalHead h1,
                                                             int64_t *cursor, int64_t cap, float *__restrict__ pred_out,
                                                             float *__restrict__ target_out, double *sums, int32_t *overflow) {
  __shared__ int wave_real[kEvalWaves];
  __shared__ int64_t srow[kEvalThreads];         // the chunk's result rows, -1 for an inert pair
  __shared__ double wave_sum[4][kEvalWaves];
  const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
  const int64_t row0 = *cursor;
  int64_t run = 0;                               // the real pairs of the chunks behind
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t base = 0; base < n; base += kEvalThreads) {
    const int64_t i = base + t;
    const bool real = i < n && (pair_w == nullptr || pair_w[i] != 0.f);
    const unsigned long long ballot = __ballot(real);
    if (lane == 0) wave_real[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kEvalWaves; ++w) {
      const int c = wave_real[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int64_t row = row0 + run + before + __popcll(ballot & ((1ull << lane) - 1ull));
    srow[t] = real ? row : -1;
    if (real) {
      const float p = relu_t(pred_c[i]), tg = target[i];
      if (row < cap) {
        pred_out[row] = p;
        target_out[row] = tg;
      }
      const double e = (double)(p - tg), a = fabs(e);        // the difference in fp32, as torch forms it, then widened
      acc[0] += 1.0;
      acc[1] += a;
      acc[2] += e * e;
      acc[3] += a < 1.0 ? 0.5 * e * e : a - 0.5;
    }
    __syncthreads();
    const int len = (int)(n - base < kEvalThreads ? n - base : kEvalThreads);
#pragma unroll
    for (int head = 0; head < 2; ++head) {
      const EvalHead &H = head == 0 ? h0 : h1;
      if (H.pred == nullptr) continue;           // block-uniform
      const int G = H.G, groups = kEvalThreads / G, group = t / G, sub = t % G;
      for (int r0 = 0; r0 < len; r0 += groups) { // block-uniform trip count: the shuffles below run converged
        const int r = r0 + group;
        const int64_t out_row = r < len ? srow[r] : -1;
        float v = 0.f;
        if (out_row >= 0) {
          const float *p = H.pred + (base + r) * H.ld;
          const int64_t *w = H.w + (base + r) * (int64_t)H.Lc;
          for (int j = sub; j < H.Lc; j += G) v += fabsf(relu_t(p[j]) - (float)w[j]);
        }
        for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_down(v, o, G);
        if (sub == 0 && out_row >= 0 && out_row < cap) H.err[out_row] = v;
      }
    }
    run += total;
    __syncthreads();                             // wave_real / srow are rewritten by the next chunk
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double v = acc[k];
    for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    if (lane == 0) wave_sum[k][wave] = v;
  }
  __syncthreads();
  if (t == 0) {
    for (int k = 0; k < 4; ++k) {
      double v = 0.0;
      for (int w = 0; w < kEvalWaves; ++w) v += wave_sum[k][w];
      sums[k] += v;
    }
    if (row0 + run > cap) *overflow = 1;
    *cursor = row0 + run;
  }
}

inline int group_width(int64_t Lc) {
  int g = 1;
  while (g < kWave && g < Lc) g <<= 1;
  return g;
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_eval_terms(const float *pred_c, const float *target, const float *pair_w, int64_t n, const float *pred_v, int64_t ld_v,
                   const int64_t *w_v, int64_t Lc_v, float *err_v, const float *pred_e, int64_t ld_e, const int64_t *w_e,
                   int64_t Lc_e, float *err_e, int64_t *cursor, int64_t cap, float *pred_out, float *target_out, double *sums,
                   int32_t *overflow, void *stream) {
  if (n < 0 || cap < 0 || !cursor || !sums || !overflow || (n > 0 && (!pred_c || !target)) || (cap > 0 && (!pred_out || !target_out)))
    return DMP_ERR_BAD_ARG;
  const float *pred[2] = {pred_v, pred_e};
  const int64_t *w[2] = {w_v, w_e};
  float *err[2] = {err_v, err_e};
  const int64_t ld[2] = {ld_v, ld_e}, Lc[2] = {Lc_v, Lc_e};
  EvalHead h[2];
  for (int k = 0; k < 2; ++k) {
    if (pred[k] && (Lc[k] < 1 || ld[k] < Lc[k] || !w[k] || (cap > 0 && !err[k]))) return DMP_ERR_BAD_ARG;
    if (pred[k] && Lc[k] > ((int64_t)1 << 30)) return DMP_ERR_UNSUPPORTED;
    h[k].pred = pred[k];
    h[k].w = w[k];
    h[k].err = err[k];
    h[k].ld = ld[k];
    h[k].Lc = pred[k] ? (int)Lc[k] : 0;
    h[k].G = pred[k] ? group_width(Lc[k]) : 1;
  }
  if (n > ((int64_t)1 << 22)) return DMP_ERR_UNSUPPORTED;      // (one workgroup: a batch's pairs)
  eval_terms_k<<<1, kEvalThreads, 0, (hipStream_t)stream>>>(pred_c, target, pair_w, n, h[0], h[1], cursor, cap, pred_out, target_out,
                                                            sums, overflow);
  return check_launch();
}

}  // extern "C"
