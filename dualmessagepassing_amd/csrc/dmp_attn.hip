// Masked multi-head attention with sparsemax weights on padded batches: the core of the gated `DotAttention` of the
// attention prediction heads (SubgraphCountingMatching/models/pred.py:240-487, sparsemax utils/act.py:255-316).
//
//   s_ij = scale * q_i . k_j  (keys with kmask 0 excluded),  p_ij = max(0, s_ij - tau_i),  sum_j p_ij = 1,
//   o_i = sum_j p_ij v_j  (rows with qmask 0 written as zeros)
//
// A row whose keys are ALL masked gets the uniform weight 1 / Lk on every padded position and its scores get no
// gradient (the reference fills masked scores with -1e30 and blocks their gradient: pred.py:476-480).
//
// The [B, Lq, Lk, nh] score tensor never exists in HBM.  Layout: Q [B, Lq, nh * dh], K / V [B, Lk, nh * dh] row-major
// fp32; per row and head the forward keeps tau (fp32) and the support size |S| (int32; 0 = every key masked).
//
// Arithmetic: exact fp32 (fmaf chains, the fp32 vector rate = the fp32 MFMA rate on gfx950).  Lane mapping: lane
// (slot, sl) owns dims [sl * DS, sl * DS + DS) of key slot `slot` (DS = min(dh, 16), S = dh / DS lanes per key, 64 / S
// keys per wave step); a dot product is the lane's DS-deep fmaf chain plus a fixed xor butterfly over its S lanes, so
// every kernel below recomputes a score bit for bit the same (the support sets of forward and backward agree).
//
// tau: Michelot's fixed point from tau_0 = max - 1 (<= tau*):  S_k = {j : s_j > tau_k},
// tau_{k+1} = max + (sum_{S_k} (s_j - max) - 1) / |S_k|, until |S_k| stops changing; then tau = (sum_S s - 1) / |S|
// exactly as the reference's sort-based threshold.  Every iteration is one pass over the row's scores: held in LDS
// when Lk <= kCacheLk, recomputed from Q and K beyond that.
//
// Backward (no float atomics, fixed reduction orders -> bitwise reproducible):
//   rows kernel: per query row (4 rows per wave, 2 at dh >= 16), delta_i = mean_{j in S_i} dO_i . v_j (first pass over the keys), then
//                dQ_i = scale * sum_{j in S_i} (dO_i . v_j - delta_i) k_j (second pass);
//   keys kernel: per key tile, all query rows: dK_j = scale * sum_i dS_ij q_i, dV_j = sum_i p_ij dO_i; the 4 waves of a
//                workgroup take every 4th row and their partial sums are added in wave order.
#include "dmp_common.h"

namespace dmp {
namespace {

constexpr int kRowsPerWave = 4;        // query rows a wave carries through the forward / the rows kernel
constexpr int kCacheLk = 2048;         // scores kept in LDS up to this key count (4 waves x 4 rows x 2048 x 4 B = 128 KiB)
constexpr int kMaxIters = 64;          // Michelot iterations (each removes at least one key; a handful in practice)

template <int DH> struct Geo {
  static constexpr int DS = DH < 16 ? DH : 16;  // dims per lane
  static constexpr int S = DH / DS;             // lanes per key
  static constexpr int KPW = kWave / S;         // keys per wave step
};

template <int N> __device__ __forceinline__ void load_vec(float (&x)[N], const float *p) {
#pragma unroll
  for (int e = 0; e < N; e += 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p + e);
    x[e] = t.x; x[e + 1] = t.y; x[e + 2] = t.z; x[e + 3] = t.w;
  }
}

template <int N> __device__ __forceinline__ void zero_vec(float (&x)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) x[e] = 0.f;
}

// Cross-lane exchanges inside a row of 16 lanes on the VALU (DPP) instead of the LDS crossbar (ds_bpermute):
// quad_perm xor 1 / xor 2, and the mirrors i <-> 7 - i / i <-> 15 - i within 8 / 16 lanes.  After the quad steps every lane
// of a quad holds the same value, so a mirror step adds the same two operands (in swapped order) on both sides of the pair:
// every lane still ends with the same bits.
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
template <int CTRL> __device__ __forceinline__ float dpp(float a) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), CTRL, 0xF, 0xF, false));
}

// the S lanes of one key hold the partial sums of one dot product: fixed butterfly (every lane ends with the same bits)
template <int S> __device__ __forceinline__ float key_sum(float a) {
  if (S >= 2) a += dpp<kDppXor1>(a);
  if (S >= 4) a += dpp<kDppXor2>(a);
  return a;
}

// sum / max over the key slots of the wave (lanes with equal sl); fixed order
template <int S> __device__ __forceinline__ float slot_sum(float a) {
  if (S == 1) {
    a += dpp<kDppXor1>(a);
    a += dpp<kDppXor2>(a);
    a += dpp<kDppHalfMirror>(a);
    a += dpp<kDppMirror>(a);
    a += __shfl_xor(a, 16);
    return a + __shfl_xor(a, 32);
  }
#pragma unroll
  for (int o = S; o < kWave; o <<= 1) a += __shfl_xor(a, o);
  return a;
}
template <int S> __device__ __forceinline__ float slot_max(float a) {
  if (S == 1) {
    a = fmaxf(a, dpp<kDppXor1>(a));
    a = fmaxf(a, dpp<kDppXor2>(a));
    a = fmaxf(a, dpp<kDppHalfMirror>(a));
    a = fmaxf(a, dpp<kDppMirror>(a));
    a = fmaxf(a, __shfl_xor(a, 16));
    return fmaxf(a, __shfl_xor(a, 32));
  }
#pragma unroll
  for (int o = S; o < kWave; o <<= 1) a = fmaxf(a, __shfl_xor(a, o));
  return a;
}

template <int DS, int S> __device__ __forceinline__ float score(const float (&q)[DS], const float (&k)[DS], float scale) {
  float a = 0.f;
#pragma unroll
  for (int e = 0; e < DS; ++e) a = fmaf(q[e], k[e], a);
  return key_sum<S>(a) * scale;
}

struct AttnArgs {
  const float *Q, *K, *V;
  const uint8_t *qmask, *kmask;   // NULL = every row / key live
  int64_t B, Lq, Lk;
  int nh;
  float scale;
};

__device__ __forceinline__ bool live(const uint8_t *m, int64_t i) { return m == nullptr || m[i] != 0; }

// K / V rows of one key step, shared by the 4 waves of a workgroup: KPW rows x dh, row stride dh + 4 (conflict-free
// float4 reads of one row per lane)
template <int DH> struct Tile {
  static constexpr int LD = DH + 4, FLOATS = Geo<DH>::KPW * LD;
};

// rows j0 .. j0 + KPW - 1 of X (the pair and head's row 0; row stride ld) into t, zeros past Lk; one float4 per thread
template <int DH>
__device__ __forceinline__ void stage_tile(float *t, const float *X, int64_t ld, int64_t j0, int64_t Lk) {
  constexpr int N4 = Geo<DH>::KPW * DH / 4, LD = Tile<DH>::LD;
  const int tid = threadIdx.x;
  if (tid < N4) {
    const int key = tid * 4 / DH, col = tid * 4 % DH;
    const int64_t j = j0 + key;
    const float4 x = j < Lk ? *reinterpret_cast<const float4 *>(X + j * ld + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4 *>(t + key * LD + col) = x;
  }
}

// ----------------------------------------------------------------------------- forward
// one workgroup = 4 waves x R query rows of one (pair b, head h); wave-private rows: only wave-level reductions.  The key
// passes stage K / V through LDS tiles (one coalesced load per workgroup instead of one strided row per lane and wave).
template <int DH, bool CACHE>
__global__ void __launch_bounds__(kBlock) attn_fwd_kernel(AttnArgs a, float *__restrict__ O, float *__restrict__ tau_out,
                                                          int32_t *__restrict__ supp_out, int64_t tiles) {
  constexpr int DS = Geo<DH>::DS, S = Geo<DH>::S, KPW = Geo<DH>::KPW, R = kRowsPerWave;
  extern __shared__ float smem[];                        // K tile, V tile, CACHE: [4 waves][R][Lk] scores (-inf at masked keys)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane / S, sl = lane % S;
  const int64_t blk = blockIdx.x;
  const int64_t tile = blk % tiles;
  const int h = (int)((blk / tiles) % a.nh);
  const int64_t b = blk / tiles / a.nh;
  const int64_t ld = (int64_t)a.nh * DH;
  const int64_t i0 = tile * (4 * R) + wave * R;
  const int64_t Lk = a.Lk;
  const float *Kh = a.K + b * Lk * ld + h * DH, *Vh = a.V + b * Lk * ld + h * DH;
  const float *Kb = Kh + sl * DS;
  const uint8_t *km = a.kmask ? a.kmask + b * Lk : nullptr;
  constexpr int LD = Tile<DH>::LD;
  float *kt = smem, *vt = smem + Tile<DH>::FLOATS;
  float *cw = CACHE ? smem + 2 * Tile<DH>::FLOATS + (int64_t)wave * R * Lk : nullptr;

  float q[R][DS];
  bool rl[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = i0 + r;
    rl[r] = i < a.Lq && live(a.qmask, b * a.Lq + i);
    if (rl[r]) load_vec(q[r], a.Q + (b * a.Lq + i) * ld + h * DH + sl * DS);
    else zero_vec(q[r]);
  }

  float m[R], tau[R];
  int cnt[R];
  int nk = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) { m[r] = -INFINITY; tau[r] = 0.f; cnt[r] = 0; }

  {
    // pass A: scores, row maxima, live key count (every wave runs the key loops: they hold the workgroup's barriers)
    for (int64_t j0 = 0; j0 < Lk; j0 += KPW) {
      __syncthreads();
      stage_tile<DH>(kt, Kh, ld, j0, Lk);
      __syncthreads();
      const int64_t j = j0 + slot;
      const bool in = j < Lk, kv = in && live(km, j);
      float k[DS];
      load_vec(k, kt + slot * LD + sl * DS);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float s = score<DS, S>(q[r], k, a.scale);
        if (kv) m[r] = fmaxf(m[r], s);
        if (CACHE && in && sl == 0) cw[r * Lk + j] = kv ? s : -INFINITY;
      }
      nk += kv ? 1 : 0;                                   // (the S lanes of a key agree: no per-lane double count after slot_sum)
    }
#pragma unroll
    for (int r = 0; r < R; ++r) m[r] = slot_max<S>(m[r]);
    nk = (int)slot_sum<S>((float)nk);   // exact: integer counts far below 2^24
    if (CACHE) __builtin_amdgcn_wave_barrier();

    if (nk > 0) {
      // Michelot's fixed point, all R rows in step (the loop bound is wave-uniform)
      int prev[R];
      bool done[R];
#pragma unroll
      for (int r = 0; r < R; ++r) { tau[r] = m[r] - 1.f; prev[r] = -1; done[r] = !rl[r]; }
      for (int it = 0; it < kMaxIters; ++it) {
        float sum[R];
        float c[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { sum[r] = 0.f; c[r] = 0.f; }
        if (CACHE) {
          for (int64_t j = lane; j < Lk; j += kWave) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const float s = cw[r * Lk + j];
              if (s > tau[r]) { sum[r] += s - m[r]; c[r] += 1.f; }
            }
          }
#pragma unroll
          for (int r = 0; r < R; ++r) { sum[r] = slot_sum<1>(sum[r]); c[r] = slot_sum<1>(c[r]); }
        } else {
          for (int64_t j0 = 0; j0 < Lk; j0 += KPW) {
            const int64_t j = j0 + slot;
            const bool kv = j < Lk && live(km, j);
            float k[DS];
            if (j < Lk) load_vec(k, Kb + j * ld); else zero_vec(k);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const float s = score<DS, S>(q[r], k, a.scale);
              if (kv && s > tau[r]) { sum[r] += s - m[r]; c[r] += 1.f; }
            }
          }
#pragma unroll
          for (int r = 0; r < R; ++r) { sum[r] = slot_sum<S>(sum[r]); c[r] = slot_sum<S>(c[r]); }
        }
        bool all = true;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (done[r]) continue;
          const int ci = (int)c[r];
          tau[r] = m[r] + (sum[r] - 1.f) / c[r];
          cnt[r] = ci;
          done[r] = ci == prev[r];
          prev[r] = ci;
          all &= done[r];
        }
        if (all) break;
      }
    }
  }

  // pass C: o_i = sum_j p_ij v_j
  float acc[R][DS];
#pragma unroll
  for (int r = 0; r < R; ++r) zero_vec(acc[r]);
  {
    const float uni = 1.f / (float)Lk;
    for (int64_t j0 = 0; j0 < Lk; j0 += KPW) {
      __syncthreads();
      stage_tile<DH>(vt, Vh, ld, j0, Lk);
      if (!CACHE && nk > 0) stage_tile<DH>(kt, Kh, ld, j0, Lk);
      __syncthreads();
      const int64_t j = j0 + slot;
      const bool in = j < Lk, kv = in && live(km, j);
      float v[DS], k[DS];
      load_vec(v, vt + slot * LD + sl * DS);
      if (!CACHE && nk > 0) load_vec(k, kt + slot * LD + sl * DS);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float p;
        if (nk == 0) {
          p = in ? uni : 0.f;
        } else {
          const float s = CACHE ? (in ? cw[r * Lk + j] : -INFINITY) : score<DS, S>(q[r], k, a.scale);
          p = (kv && s > tau[r]) ? s - tau[r] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < DS; ++e) acc[r][e] = fmaf(p, v[e], acc[r][e]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = i0 + r;
#pragma unroll
    for (int e = 0; e < DS; ++e) acc[r][e] = slot_sum<S>(acc[r][e]);
    if (i >= a.Lq) continue;
    if (slot == 0) {
      float *o = O + (b * a.Lq + i) * ld + h * DH + sl * DS;
#pragma unroll
      for (int e = 0; e < DS; e += 4)
        *reinterpret_cast<float4 *>(o + e) = rl[r] ? make_float4(acc[r][e], acc[r][e + 1], acc[r][e + 2], acc[r][e + 3])
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane == 0) {
      const int64_t t = (b * a.Lq + i) * a.nh + h;
      tau_out[t] = rl[r] ? tau[r] : 0.f;
      supp_out[t] = (rl[r] && nk > 0) ? cnt[r] : 0;
    }
  }
}

// ----------------------------------------------------------------------------- backward, per query row: delta, dQ
template <int DH> constexpr int bwd_rows_per_wave() { return DH >= 16 ? 2 : 4; }

template <int DH>
__global__ void __launch_bounds__(kBlock) attn_bwd_rows_kernel(AttnArgs a, const float *__restrict__ dO,
                                                               const float *__restrict__ tau_in, const int32_t *__restrict__ supp,
                                                               float *__restrict__ delta_out, float *__restrict__ dQ, int64_t tiles) {
  constexpr int DS = Geo<DH>::DS, S = Geo<DH>::S, KPW = Geo<DH>::KPW, R = bwd_rows_per_wave<DH>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane / S, sl = lane % S;
  const int64_t blk = blockIdx.x;
  const int64_t tile = blk % tiles;
  const int h = (int)((blk / tiles) % a.nh);
  const int64_t b = blk / tiles / a.nh;
  const int64_t ld = (int64_t)a.nh * DH;
  const int64_t i0 = tile * (4 * R) + wave * R;
  const int64_t Lk = a.Lk;
  const float *Kh = a.K + b * Lk * ld + h * DH, *Vh = a.V + b * Lk * ld + h * DH;
  const uint8_t *km = a.kmask ? a.kmask + b * Lk : nullptr;
  constexpr int LD = Tile<DH>::LD;
  __shared__ __attribute__((aligned(16))) float kvt[2 * Tile<DH>::FLOATS];
  float *kt = kvt, *vt = kvt + Tile<DH>::FLOATS;

  float q[R][DS], g[R][DS], tau[R], cf[R];
  bool rl[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = i0 + r;
    const int64_t t = (b * a.Lq + i) * a.nh + h;
    // rows with a masked query or with every key masked send no gradient into the scores
    rl[r] = i < a.Lq && live(a.qmask, b * a.Lq + i) && supp[t] > 0;
    tau[r] = rl[r] ? tau_in[t] : 0.f;
    cf[r] = rl[r] ? (float)supp[t] : 1.f;
    if (rl[r]) {
      load_vec(q[r], a.Q + (b * a.Lq + i) * ld + h * DH + sl * DS);
      load_vec(g[r], dO + (b * a.Lq + i) * ld + h * DH + sl * DS);
    } else {
      zero_vec(q[r]);
      zero_vec(g[r]);
    }
  }
  float delta[R], acc[R][DS];
#pragma unroll
  for (int r = 0; r < R; ++r) { delta[r] = 0.f; zero_vec(acc[r]); }
  {
    // pass 1: delta_i = mean over the support of dO_i . v_j (every wave runs the key loops: they hold the barriers)
    for (int64_t j0 = 0; j0 < Lk; j0 += KPW) {
      __syncthreads();
      stage_tile<DH>(kt, Kh, ld, j0, Lk);
      stage_tile<DH>(vt, Vh, ld, j0, Lk);
      __syncthreads();
      const int64_t j = j0 + slot;
      const bool kv = j < Lk && live(km, j);
      float k[DS], v[DS];
      load_vec(k, kt + slot * LD + sl * DS);
      load_vec(v, vt + slot * LD + sl * DS);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float s = score<DS, S>(q[r], k, a.scale);
        const float dp = score<DS, S>(g[r], v, 1.f);
        if (kv && s > tau[r]) delta[r] += dp;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) delta[r] = slot_sum<S>(delta[r]) / cf[r];
    // pass 2: dQ_i = scale * sum_S (dp_ij - delta_i) k_j
    for (int64_t j0 = 0; j0 < Lk; j0 += KPW) {
      __syncthreads();
      stage_tile<DH>(kt, Kh, ld, j0, Lk);
      stage_tile<DH>(vt, Vh, ld, j0, Lk);
      __syncthreads();
      const int64_t j = j0 + slot;
      const bool kv = j < Lk && live(km, j);
      float k[DS], v[DS];
      load_vec(k, kt + slot * LD + sl * DS);
      load_vec(v, vt + slot * LD + sl * DS);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float s = score<DS, S>(q[r], k, a.scale);
        const float dp = score<DS, S>(g[r], v, 1.f);
        const float ds = (kv && s > tau[r]) ? dp - delta[r] : 0.f;
#pragma unroll
        for (int e = 0; e < DS; ++e) acc[r][e] = fmaf(ds, k[e], acc[r][e]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = i0 + r;
#pragma unroll
    for (int e = 0; e < DS; ++e) acc[r][e] = slot_sum<S>(acc[r][e]) * a.scale;
    if (i >= a.Lq) continue;
    if (slot == 0) {
      float *o = dQ + (b * a.Lq + i) * ld + h * DH + sl * DS;
#pragma unroll
      for (int e = 0; e < DS; e += 4)
        *reinterpret_cast<float4 *>(o + e) = rl[r] ? make_float4(acc[r][e], acc[r][e + 1], acc[r][e + 2], acc[r][e + 3])
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane == 0) delta_out[(b * a.Lq + i) * a.nh + h] = delta[r];
  }
}

// ----------------------------------------------------------------------------- backward, per key tile: dK, dV
// one workgroup = KPW keys of one (b, h); wave w takes the query rows w, w + 4, ...; the four partials are added in
// wave order through LDS
template <int DH>
__global__ void __launch_bounds__(kBlock) attn_bwd_keys_kernel(AttnArgs a, const float *__restrict__ dO,
                                                               const float *__restrict__ tau_in, const int32_t *__restrict__ supp,
                                                               const float *__restrict__ delta_in, float *__restrict__ dK,
                                                               float *__restrict__ dV, int64_t tiles) {
  constexpr int DS = Geo<DH>::DS, S = Geo<DH>::S, KPW = Geo<DH>::KPW;
  __shared__ float red[3][kWave * 2 * DS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane / S, sl = lane % S;
  const int64_t blk = blockIdx.x;
  const int64_t tile = blk % tiles;
  const int h = (int)((blk / tiles) % a.nh);
  const int64_t b = blk / tiles / a.nh;
  const int64_t ld = (int64_t)a.nh * DH;
  const int64_t Lk = a.Lk;
  const int64_t j = tile * KPW + slot;
  const bool in = j < Lk, kv = in && live(a.kmask, b * Lk + j);
  float k[DS], v[DS], gk[DS], gv[DS];
  if (in) {
    load_vec(k, a.K + (b * Lk + j) * ld + h * DH + sl * DS);
    load_vec(v, a.V + (b * Lk + j) * ld + h * DH + sl * DS);
  } else {
    zero_vec(k);
    zero_vec(v);
  }
  zero_vec(gk);
  zero_vec(gv);
  const float uni = 1.f / (float)Lk;
  for (int64_t i = wave; i < a.Lq; i += 4) {
    if (!live(a.qmask, b * a.Lq + i)) continue;
    const int64_t t = (b * a.Lq + i) * a.nh + h;
    const int c = supp[t];
    float g[DS];
    load_vec(g, dO + (b * a.Lq + i) * ld + h * DH + sl * DS);
    if (c == 0) {                            // every key masked: uniform weights, no score gradient
#pragma unroll
      for (int e = 0; e < DS; ++e) gv[e] = fmaf(uni, g[e], gv[e]);
      continue;
    }
    const float tau = tau_in[t], delta = delta_in[t];
    float q[DS];
    load_vec(q, a.Q + (b * a.Lq + i) * ld + h * DH + sl * DS);
    const float s = score<DS, S>(q, k, a.scale);
    const float dp = score<DS, S>(g, v, 1.f);
    const bool sup = kv && s > tau;
    const float p = sup ? s - tau : 0.f;
    const float ds = sup ? dp - delta : 0.f;
#pragma unroll
    for (int e = 0; e < DS; ++e) {
      gv[e] = fmaf(p, g[e], gv[e]);
      gk[e] = fmaf(ds, q[e], gk[e]);
    }
  }
  if (wave > 0) {
    float *w = red[wave - 1] + lane * 2 * DS;
#pragma unroll
    for (int e = 0; e < DS; ++e) { w[e] = gk[e]; w[DS + e] = gv[e]; }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const float *x = red[w] + lane * 2 * DS;
#pragma unroll
      for (int e = 0; e < DS; ++e) { gk[e] += x[e]; gv[e] += x[DS + e]; }
    }
    if (in) {
      float *ok = dK + (b * Lk + j) * ld + h * DH + sl * DS;
      float *ov = dV + (b * Lk + j) * ld + h * DH + sl * DS;
#pragma unroll
      for (int e = 0; e < DS; e += 4) {
        *reinterpret_cast<float4 *>(ok + e) = make_float4(gk[e] * a.scale, gk[e + 1] * a.scale, gk[e + 2] * a.scale, gk[e + 3] * a.scale);
        *reinterpret_cast<float4 *>(ov + e) = make_float4(gv[e], gv[e + 1], gv[e + 2], gv[e + 3]);
      }
    }
  }
}

bool dh_ok(int dh) { return dh == 4 || dh == 8 || dh == 16 || dh == 32 || dh == 64; }

bool args_ok(const AttnArgs &a, int dh) {
  if (!a.Q || !a.K || !a.V || a.B < 0 || a.Lq < 0 || a.Lk < 0 || a.nh < 1) return false;
  return aligned16(a.Q) && aligned16(a.K) && aligned16(a.V) && dh_ok(dh);
}

int64_t row_tiles(int64_t Lq, int rows_per_wave = kRowsPerWave) { return (Lq + 4 * rows_per_wave - 1) / (4 * rows_per_wave); }

template <int DH> int64_t key_tiles(int64_t Lk) { return (Lk + Geo<DH>::KPW - 1) / Geo<DH>::KPW; }

// the score cache goes above the 64 KiB default of dynamic LDS: opted in once per (kernel, device)
constexpr int kCacheBytes = 4 * kRowsPerWave * kCacheLk * 4;
template <int DH> constexpr int tile_bytes() { return 2 * Tile<DH>::FLOATS * 4; }
template <int DH> bool cache_lds_ready() {
  static bool done[kMaxDevices] = {};
  return opt_in_lds(reinterpret_cast<const void *>(&attn_fwd_kernel<DH, true>), kCacheBytes + tile_bytes<DH>(), done);
}

template <int DH>
int fwd_dh(const AttnArgs &a, float *O, float *tau, int32_t *supp, hipStream_t st) {
  const int64_t tiles = row_tiles(a.Lq);
  const int64_t nblk = tiles * a.nh * a.B;
  if (a.Lk <= kCacheLk) {
    const size_t lds = tile_bytes<DH>() + (size_t)4 * kRowsPerWave * a.Lk * sizeof(float);
    if (!cache_lds_ready<DH>()) return DMP_ERR_HIP;
    hipLaunchKernelGGL((attn_fwd_kernel<DH, true>), dim3((unsigned)nblk), dim3(kBlock), lds, st, a, O, tau, supp, tiles);
  } else {
    hipLaunchKernelGGL((attn_fwd_kernel<DH, false>), dim3((unsigned)nblk), dim3(kBlock), tile_bytes<DH>(), st, a, O, tau, supp, tiles);
  }
  return check_launch();
}

template <int DH>
int bwd_dh(const AttnArgs &a, const float *dO, const float *tau, const int32_t *supp, float *delta, float *dQ, float *dK, float *dV,
           hipStream_t st) {
  const int64_t rt = row_tiles(a.Lq, bwd_rows_per_wave<DH>()), kt = key_tiles<DH>(a.Lk);
  hipLaunchKernelGGL((attn_bwd_rows_kernel<DH>), dim3((unsigned)(rt * a.nh * a.B)), dim3(kBlock), 0, st, a, dO, tau, supp, delta, dQ, rt);
  const int rc = check_launch();
  if (rc != DMP_OK) return rc;
  hipLaunchKernelGGL((attn_bwd_keys_kernel<DH>), dim3((unsigned)(kt * a.nh * a.B)), dim3(kBlock), 0, st, a, dO, tau, supp, delta, dK,
                     dV, kt);
  return check_launch();
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_attn_supported_dh(int dh) { return dh_ok(dh) ? 1 : 0; }

int dmp_attn_fwd(const float *Q, const float *K, const float *V, const uint8_t *qmask, const uint8_t *kmask, int64_t B, int64_t Lq,
                 int64_t Lk, int nh, int dh, float scale, float *O, float *tau, int32_t *supp, void *stream) {
  AttnArgs a{Q, K, V, qmask, kmask, B, Lq, Lk, nh, scale};
  if (!dh_ok(dh)) return DMP_ERR_UNSUPPORTED;
  if (B == 0 || Lq == 0) return DMP_OK;
  if (!args_ok(a, dh) || !O || !tau || !supp || !aligned16(O) || Lk < 1) return DMP_ERR_BAD_ARG;
  if (row_tiles(Lq) * nh * B >= (int64_t)1 << 31) return DMP_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dh) {
    case 4: return fwd_dh<4>(a, O, tau, supp, st);
    case 8: return fwd_dh<8>(a, O, tau, supp, st);
    case 16: return fwd_dh<16>(a, O, tau, supp, st);
    case 32: return fwd_dh<32>(a, O, tau, supp, st);
    default: return fwd_dh<64>(a, O, tau, supp, st);
  }
}

int dmp_attn_bwd(const float *Q, const float *K, const float *V, const uint8_t *qmask, const uint8_t *kmask, const float *dO,
                 const float *tau, const int32_t *supp, int64_t B, int64_t Lq, int64_t Lk, int nh, int dh, float scale, float *delta,
                 float *dQ, float *dK, float *dV, void *stream) {
  AttnArgs a{Q, K, V, qmask, kmask, B, Lq, Lk, nh, scale};
  if (!dh_ok(dh)) return DMP_ERR_UNSUPPORTED;
  if (B == 0 || Lk == 0) return DMP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (Lq == 0) {   // no rows (the per-row arrays are empty and may be NULL): the key gradients are zero
    if (B < 0 || Lk < 0 || nh < 1 || !dK || !dV) return DMP_ERR_BAD_ARG;
    const size_t n = (size_t)(B * Lk * nh * dh) * sizeof(float);
    hipError_t e = hipMemsetAsync(dK, 0, n, st);
    if (e == hipSuccess) e = hipMemsetAsync(dV, 0, n, st);
    if (e != hipSuccess) { set_last_hip_error(e); return DMP_ERR_HIP; }
    return DMP_OK;
  }
  if (!args_ok(a, dh) || !dO || !tau || !supp || !delta || !dQ || !dK || !dV) return DMP_ERR_BAD_ARG;
  if (!aligned16(dO) || !aligned16(dQ) || !aligned16(dK) || !aligned16(dV)) return DMP_ERR_BAD_ARG;
  if (row_tiles(Lq, 2) * nh * B >= (int64_t)1 << 31 || (Lk + 63) * nh * B >= (int64_t)1 << 31) return DMP_ERR_UNSUPPORTED;
  switch (dh) {
    case 4: return bwd_dh<4>(a, dO, tau, supp, delta, dQ, dK, dV, st);
    case 8: return bwd_dh<8>(a, dO, tau, supp, delta, dQ, dK, dV, st);
    case 16: return bwd_dh<16>(a, dO, tau, supp, delta, dQ, dK, dV, st);
    case 32: return bwd_dh<32>(a, dO, tau, supp, delta, dQ, dK, dV, st);
    default: return bwd_dh<64>(a, dO, tau, supp, delta, dQ, dK, dV, st);
  }
}

}  // extern "C"
