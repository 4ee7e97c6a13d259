// The matching loss and regulariser of a training step (train.py:627-649) with their gradient seeds, one call per term
// (node / edge), capacity-aware: pairs with pair_w == 0 and the front columns no real pair uses are left out, so the
// term of a padded batch is the term of its real pairs (see include/dmp_hip.h for the definition).
//
// A bandwidth-bound reduction over 17 bytes per element (pred 4, w 8, mask 1 read; dpred 4 written).  THREE launches per
// term, whatever the shape, no memset, no atomics:
//   1. match_ext_k     a wave per row: ext[i] = Lc - (first live column), 0 without one, -1 for an inert pair.
//   2. match_terms_k   a wave per (row, 1024-column chunk) task, four tasks per workgroup: every workgroup first folds
//                      ext[] into n (real pairs) and Lr (window length) -- integers, exact in any order --, then each wave
//                      reads its chunk (16-byte loads of pred where the rows allow them), writes dpred, and reduces its
//                      three sums with wave-64 shuffles: the regulariser's per-task sum for dpred_c goes to dc[task], the
//                      loss / reg sums of the four waves to one partial pair per workgroup (added in wave order).
//   3. match_final_k   one workgroup: the partial pairs in a fixed order (thread-strided, then a tree) -> terms[3];
//                      dpred_c[i] = the row's task sums in chunk order.
// Fixed summation order throughout: two launches on the same inputs give the same bits.
// Sized for a training batch: B up to a few thousand rows (every workgroup of the second launch reads all B extents, 4 B
// bytes from the L2: O(B x workgroups) beyond that), and the first launch reads a row whose start is not 16-byte aligned
// (Lc % 16 != 0) as single bytes, 16 per lane.  Larger B is computed correctly, not quickly.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kMatchCols = 1024;                    // columns of one wave task: 64 lanes x 4 columns x 4 rounds
constexpr int kMatchWaves = kBlock / kWave;         // tasks per workgroup
constexpr int kFinalThreads = 1024;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;                                         // lane 0 holds the sum
}

// crit(d) and crit'(d): kind 0 MSE, 1 MAE, 2 smooth L1 (beta 1) -- torch's formulas, sign(0) = 0
__device__ __forceinline__ void crit(int kind, float d, float &v, float &g) {
  if (kind == 0) { v = d * d; g = 2.f * d; }
  else if (kind == 1) { v = fabsf(d); g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
  else { const float a = fabsf(d); v = a < 1.f ? 0.5f * d * d : a - 0.5f; g = a < 1.f ? d : (d > 0.f ? 1.f : -1.f); }
}

// n = the number of real pairs, Lr = their largest extent, from ext[B] (every thread of the workgroup gets both)
template <int THREADS>
__device__ __forceinline__ void fold_ext(const int32_t *__restrict__ ext, int64_t B, int *sh, int &n, int &Lr) {
  int cnt = 0, mx = 0;
  for (int64_t i = threadIdx.x; i < B; i += THREADS) {
    const int e = ext[i];
    cnt += e >= 0 ? 1 : 0;
    mx = e > mx ? e : mx;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, kWave);
    const int other = __shfl_xor(mx, o, kWave);
    mx = other > mx ? other : mx;
  }
  constexpr int W = THREADS / kWave;
  if (threadIdx.x % kWave == 0) { sh[threadIdx.x / kWave] = cnt; sh[W + threadIdx.x / kWave] = mx; }
  __syncthreads();
  n = 0; Lr = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) { n += sh[k]; Lr = sh[W + k] > Lr ? sh[W + k] : Lr; }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void match_ext_k(const uint8_t *__restrict__ mask, const float *__restrict__ pair_w,
                                                      int64_t B, int Lc, int32_t *__restrict__ ext) {
  const int64_t row = blockIdx.x * (int64_t)kMatchWaves + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= B) return;                              // (no barrier below)
  if (pair_w && pair_w[row] == 0.f) {
    if (lane == 0) ext[row] = -1;
    return;
  }
  const uint8_t *m = mask + row * (int64_t)Lc;
  const bool vec = (reinterpret_cast<uintptr_t>(m) & 15u) == 0;
  int first = Lc;
  for (int base = 0; base < Lc; base += kWave * 16) {          // 16 columns per lane and round
    const int c = base + lane * 16;
    int mine = -1;
    if (c + 16 <= Lc && vec) {
      const uint4 q = *reinterpret_cast<const uint4 *>(m + c);
      const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 3; k >= 0; --k)
        if (word[k]) mine = 4 * k + (__ffs(word[k]) - 1) / 8;
    } else {
#pragma unroll
      for (int k = 15; k >= 0; --k)
        if (c + k < Lc && m[c + k]) mine = k;
    }
    const unsigned long long hit = __ballot(mine >= 0);
    if (hit) {
      const int src = __ffsll((long long)hit) - 1;
      first = __shfl(c + mine, src, kWave);
      break;
    }
  }
  if (lane == 0) ext[row] = Lc - first;
}

__global__ __launch_bounds__(kBlock) void match_terms_k(
    const float *__restrict__ pred, int64_t ldp, const int64_t *__restrict__ w, const uint8_t *__restrict__ mask,
    const float *__restrict__ pred_c, const float *__restrict__ coef, const int32_t *__restrict__ ext, int64_t B, int Lc,
    int chunks, int64_t tasks, int kind, int pred_vec, int in_vec, float *__restrict__ dpred, float *__restrict__ dc,
    float *__restrict__ partial) {
  __shared__ int sh_i[2 * kMatchWaves];
  __shared__ float sh_f[2 * kMatchWaves];
  int n, Lr;
  fold_ext<kBlock>(ext, B, sh_i, n, Lr);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int64_t task = blockIdx.x * (int64_t)kMatchWaves + wave;
  float s_loss = 0.f, s_reg = 0.f, s_dc = 0.f;
  if (task < tasks) {
    const int64_t row = task / chunks;
    const int c0 = (int)(task % chunks) * kMatchCols;
    const bool real = n > 0 && ext[row] >= 0;
    const int lo = Lc - Lr;                                     // first column of the window
    const float slope = coef[0], lw = coef[1], rw = coef[2];
    const float inv_n = n > 0 ? 1.f / (float)n : 0.f;
    const float c = pred_c[row];
    const float *prow = pred + row * ldp;
    const int64_t base = row * (int64_t)Lc;
    const bool out_vec = (base & 3) == 0;                       // dpred is 16-byte aligned: its rows are when Lc % 4 == 0 (or row 0)
#pragma unroll
    for (int r = 0; r < kMatchCols / (kWave * 4); ++r) {
      const int j = c0 + r * kWave * 4 + lane * 4;
      if (j >= Lc) continue;
      const bool full = j + 4 <= Lc;
      float x[4], g[4];
      if (!real || j + 4 <= lo) {                               // an inert pair, or in front of the window: exact zeros
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = 0.f;
      } else {
        if (full && pred_vec) {
          const float4 q = *reinterpret_cast<const float4 *>(prow + j);
          x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) x[k] = j + k < Lc ? prow[j + k] : 0.f;
        }
        // the four masks and weights of the group before any arithmetic (independent loads in flight); rows that start on
        // a multiple of four columns take them as one 4-byte and two 16-byte loads
        uint8_t mk[4];
        long long wk[4];
        if (full && out_vec && in_vec) {
          const uint32_t q = *reinterpret_cast<const uint32_t *>(mask + base + j);
          const longlong2 a = *reinterpret_cast<const longlong2 *>(w + base + j);
          const longlong2 b = *reinterpret_cast<const longlong2 *>(w + base + j + 2);
          mk[0] = q & 0xff; mk[1] = (q >> 8) & 0xff; mk[2] = (q >> 16) & 0xff; mk[3] = q >> 24;
          wk[0] = a.x; wk[1] = a.y; wk[2] = b.x; wk[3] = b.y;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            mk[k] = j + k < Lc ? mask[base + j + k] : 0;
            wk[k] = j + k < Lc ? (long long)w[base + j + k] : 0;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          g[k] = 0.f;
          if (j + k >= Lc || j + k < lo) continue;
          const bool live = mk[k] != 0;
          const float xv = live ? x[k] : 0.f;
          const float t = live ? (float)wk[k] : 0.f;
          const float da = xv > 0.f ? 1.f : slope;              // leaky_relu'(x) (torch: the slope at x <= 0)
          float v, gl, gr;
          crit(kind, xv * da - t, v, gl);
          s_loss += v;
          const float u = xv - c;
          const float rl = u > 0.f ? u : 0.f;
          crit(kind, rl, v, gr);
          s_reg += v;
          gr = u > 0.f ? gr : 0.f;                              // relu'(u)
          s_dc += gr;
          g[k] = (lw * (gl * da) + rw * gr) * inv_n;
        }
      }
      if (full && out_vec) {
        *reinterpret_cast<float4 *>(dpred + base + j) = make_float4(g[0], g[1], g[2], g[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (j + k < Lc) dpred[base + j + k] = g[k];
      }
    }
  }
  s_loss = wave_sum(s_loss);
  s_reg = wave_sum(s_reg);
  s_dc = wave_sum(s_dc);
  if (lane == 0) {
    if (task < tasks) dc[task] = s_dc;
    sh_f[wave] = s_loss;
    sh_f[kMatchWaves + wave] = s_reg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < kMatchWaves; ++k) { a += sh_f[k]; b += sh_f[kMatchWaves + k]; }
    partial[2 * (int64_t)blockIdx.x] = a;
    partial[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

__global__ __launch_bounds__(kFinalThreads) void match_final_k(const float *__restrict__ partial, int64_t groups,
                                                               const float *__restrict__ dc, int chunks,
                                                               const int32_t *__restrict__ ext, int64_t B,
                                                               const float *__restrict__ coef, float *__restrict__ terms,
                                                               float *__restrict__ dpred_c) {
  __shared__ int sh_i[2 * (kFinalThreads / kWave)];
  __shared__ float red[2][kFinalThreads];
  int n, Lr;
  fold_ext<kFinalThreads>(ext, B, sh_i, n, Lr);
  const float lw = coef[1], rw = coef[2];
  const float inv_n = n > 0 ? 1.f / (float)n : 0.f;
  float a = 0.f, b = 0.f;
  for (int64_t k = threadIdx.x; k < groups; k += kFinalThreads) { a += partial[2 * k]; b += partial[2 * k + 1]; }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int s = kFinalThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float loss = red[0][0] * inv_n, reg = red[1][0] * inv_n;
    terms[0] = loss;
    terms[1] = reg;
    terms[2] = lw * loss + rw * reg;
  }
  for (int64_t i = threadIdx.x; i < B; i += kFinalThreads) {
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += dc[i * chunks + k];
    dpred_c[i] = n > 0 && ext[i] >= 0 ? -(rw * s) * inv_n : 0.f;
  }
}

inline int64_t match_chunks(int64_t Lc) { return (Lc + kMatchCols - 1) / kMatchCols; }
inline int64_t match_groups(int64_t B, int64_t Lc) { return (B * match_chunks(Lc) + kMatchWaves - 1) / kMatchWaves; }

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int64_t dmp_match_loss_workspace_words(int64_t B, int64_t Lc) {
  if (B < 1 || Lc < 1 || Lc > ((int64_t)1 << 30) || B > (((int64_t)1 << 31) - 1) / Lc) return 0;
  return B + B * match_chunks(Lc) + 2 * match_groups(B, Lc);        // ext | dc | partial pairs
}

int dmp_match_loss(const float *pred, int64_t ldp, const int64_t *w, const uint8_t *mask, const float *pred_c,
                   const float *pair_w, const float *coef, int64_t B, int64_t Lc, int kind, float *terms, float *dpred,
                   float *dpred_c, void *workspace, void *stream) {
  if (B < 0 || Lc < 0 || kind < 0 || kind > 2 || ldp < Lc) return DMP_ERR_BAD_ARG;
  // (columns are 32-bit in the kernels, with room for one task past the row's end)
  if (B == 0 || Lc == 0 || Lc > ((int64_t)1 << 30) || B > (((int64_t)1 << 31) - 1) / Lc) return DMP_ERR_UNSUPPORTED;
  if (!pred || !w || !mask || !pred_c || !coef || !terms || !dpred || !dpred_c || !workspace || !aligned16(dpred))
    return DMP_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = match_chunks(Lc), tasks = B * chunks, groups = match_groups(B, Lc);
  int32_t *ext = static_cast<int32_t *>(workspace);
  float *dc = reinterpret_cast<float *>(ext + B);
  float *partial = dc + tasks;
  const int pred_vec = aligned16(pred) && ldp % 4 == 0 ? 1 : 0;
  const int in_vec = aligned16(w) && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0 ? 1 : 0;
  match_ext_k<<<(unsigned)((B + kMatchWaves - 1) / kMatchWaves), kBlock, 0, st>>>(mask, pair_w, B, (int)Lc, ext);
  int rc = check_launch();
  if (rc != DMP_OK) return rc;
  match_terms_k<<<(unsigned)groups, kBlock, 0, st>>>(pred, ldp, w, mask, pred_c, coef, ext, B, (int)Lc, (int)chunks, tasks,
                                                    kind, pred_vec, in_vec, dpred, dc, partial);
  rc = check_launch();
  if (rc != DMP_OK) return rc;
  match_final_k<<<1, kFinalThreads, 0, st>>>(partial, groups, dc, (int)chunks, ext, B, coef, terms, dpred_c);
  return check_launch();
}

}  // extern "C"
