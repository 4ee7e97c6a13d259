// Rank counts of a link predictor's decoder (unc_eval.py): for every query row i, how many candidates of a table score
// above / exactly at the score of the query's target,
//
//   score(i, c) = sum_h query[i, h] table[c, h],   t_i = score(i, target_i),
//   greater_i = #{c in C_i : score(i, c) > t_i},   equal_i = #{c in C_i : score(i, c) == t_i},
//   C_i = {c : c != target_i and c not in filt_i}                      (membership by INDEX, never by value)
//
// without the [Q, N] score matrix ever leaving the registers.
//
// Geometry.  A workgroup owns kRankQT = 128 query rows (32 per wave), staged once in LDS with the last k-group zero-padded
// there, and streams candidate tiles of kRankCT = 128 table rows past them, kRankKC = 32 columns at a time: the chunk of the
// next step is fetched into registers while the MFMAs of this one run, so one LDS buffer serves.  Each wave keeps four 32x32
// accumulators (its 32 queries against the tile's four groups of 32 candidates): five ds_read_b32 per four MFMAs.  Both LDS
// images are row-major with an ODD row stride, so the 32 rows a half-wave reads fall on 32 banks.  grid.y splits the
// candidate range when the query tiles alone would not fill the device.
//
// Arithmetic.  The exact f32-input MFMA (v_mfma_f32_32x32x2_f32): every score is a k-ascending fmaf chain, bit for bit the
// same whichever tile, column or workgroup computes it.  t_i comes out of the SAME routine: tile 0 of every workgroup is the
// gather of its 128 target rows, and a wave keeps the diagonal of its own group.  A candidate whose row equals the target's
// row therefore scores == t_i exactly.
//
// Counting.  The comparison runs on the accumulator registers; per-lane integer counters are butterfly-reduced over the 32
// lanes of a row at the end and added to the outputs with integer vector atomics (the entry zeroes the outputs first).
// Integer sums: the result does not depend on the order.  A NaN score compares false both ways.
//
// Filter, target, tail.  Per tile every lane (row lane & 31) builds a 128-bit exclusion mask of ITS row: the target's bit,
// the bits of the row's sorted filter list that fall into the tile (a cursor into the list, placed by one bisection at the
// workgroup's first candidate and advanced tile by tile), and the bits past N in the last tile.  A tile in which no row of
// the wave excludes anything -- the usual case -- takes the unmasked comparison; otherwise the masks are read across lanes.
#include "dmp_mfma_common.h"

namespace dmp {
namespace {

constexpr int kRankQT = 128;               // query rows of a workgroup
constexpr int kRankCT = 128;               // candidates of a tile
constexpr int kRankKC = 32;                // columns of a candidate tile in LDS at a time
constexpr int kRankCS = kRankKC + 1;       // its row stride (odd)
constexpr int kRankMaxH = 256;
constexpr int kRankLoads = kRankCT * kRankKC / kBlock;      // elements a thread stages per chunk (16)
constexpr int kRankRowStep = kBlock / kRankKC;              // rows between them (8)
constexpr int kRankMinTiles = 4;           // candidate tiles of a split at least
constexpr int kRankWantGroups = 2048;      // workgroups aimed at before the candidate range stops being split
constexpr int64_t kRankNoEntry = INT64_MAX;

__host__ __device__ constexpr int rank_qstride(int H) { return (H + kRankKC - 1) / kRankKC * kRankKC + 1; }
size_t rank_lds_bytes(int H) { return sizeof(float) * ((size_t)kRankQT * rank_qstride(H) + kRankCT * kRankCS + 2 * kRankQT); }

struct RankArgs {
  const float *query, *table;
  const int64_t *target, *filt_ptr, *filt_idx;
  int64_t nnz;
  int Q, N, H, tiles_per_split;
  int *greater, *equal;
};

// row of accumulator register g in a lane of half hi (the 32x32 C/D map; the column is lane & 31)
__device__ __forceinline__ int acc_row(int g, int hi) { return (g & 3) + 8 * (g >> 2) + 4 * hi; }

__device__ __forceinline__ void set_bit(uint32_t (&m)[4], int d) {
  const uint32_t b = 1u << (d & 31);
  const int w = d >> 5;
  m[0] |= w == 0 ? b : 0u;
  m[1] |= w == 1 ? b : 0u;
  m[2] |= w == 2 ? b : 0u;
  m[3] |= w == 3 ? b : 0u;
}

// (two waves per SIMD: left to itself the register allocator takes 305 registers and spills scalars for the 64 comparisons of a tile)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void rank_counts_k(RankArgs a) {
  extern __shared__ float4 rank_lds[];
  const int QS = rank_qstride(a.H);
  float *qs = reinterpret_cast<float *>(rank_lds);     // [kRankQT][QS]   the queries, columns H .. QS - 2 zero
  float *cs = qs + kRankQT * QS;                       // [kRankCT][kRankCS] one 32-column chunk of a candidate tile
  float *ts = cs + kRankCT * kRankCS;                  // [kRankQT]       the target scores
  int *tg = reinterpret_cast<int *>(ts + kRankQT);     // [kRankQT]       the target rows, clamped into the table
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, r = lane & 31, hi = lane >> 5;
  const int q0 = blockIdx.x * kRankQT;
  const int scol = tid % kRankKC, srow = tid / kRankKC;     // the element of a chunk this thread stages: (srow + 8 i, scol)
  const int ntiles = (a.N + kRankCT - 1) / kRankCT;
  const int tile_begin = blockIdx.y * a.tiles_per_split;
  const int ntl = min(a.tiles_per_split, ntiles - tile_begin);   // candidate tiles of this workgroup (>= 1 by the launch)
  const int c_begin = tile_begin * kRankCT;

  // ---- the queries and the targets of this workgroup
  for (int kc = 0; kc < QS - 1; kc += kRankKC) {
    const int col = kc + scol;
#pragma unroll 4
    for (int i = 0; i < kRankLoads; ++i) {
      const int row = srow + kRankRowStep * i, q = q0 + row;
      qs[row * QS + col] = (q < a.Q && col < a.H) ? a.query[(int64_t)q * a.H + col] : 0.f;
    }
  }
  if (tid < kRankQT) {
    const int q = q0 + tid;
    const int64_t t = q < a.Q ? a.target[q] : 0;
    tg[tid] = (int)(t < 0 ? 0 : (t >= a.N ? a.N - 1 : t));
  }
  // ---- this lane's row: its target and the cursor into its filter list
  const int myq = q0 + wave * 32 + r;
  int64_t tgt = -1, cur = 0, fend = 0, nxt = kRankNoEntry;
  if (myq < a.Q) {
    tgt = a.target[myq];
    if (a.filt_ptr) {
      int64_t lo = a.filt_ptr[myq], hiend = a.filt_ptr[myq + 1];
      lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
      hiend = hiend < lo ? lo : (hiend > a.nnz ? a.nnz : hiend);
      fend = hiend;
      while (lo < hiend) {                       // first entry >= c_begin
        const int64_t mid = lo + ((hiend - lo) >> 1);
        if (a.filt_idx[mid] < c_begin) lo = mid + 1; else hiend = mid;
      }
      cur = lo;
      if (cur < fend) nxt = a.filt_idx[cur];
    }
  }

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;
  float treg[16];
  int cg[16], ce[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) { treg[g] = 0.f; cg[g] = 0; ce[g] = 0; }

  // chunk (ti, kc): ti == 0 is the gather of the target rows, ti >= 1 candidate tile tile_begin + ti - 1
  float pf[kRankLoads];
  auto fetch = [&](int ti, int kc) {       // every load is issued unconditionally from a clamped address: no branch per element
    const int col = kc + scol;
    const bool col_on = col < a.H;
    const int colc = col_on ? col : 0;
    if (ti == 0) {
#pragma unroll
      for (int i = 0; i < kRankLoads; ++i) {
        const float v = a.table[(int64_t)tg[srow + kRankRowStep * i] * a.H + colc];
        pf[i] = col_on ? v : 0.f;
      }
    } else {
      const int c0 = c_begin + (ti - 1) * kRankCT;       // < N: the tile exists
      const float *base = a.table + (int64_t)c0 * a.H + colc;
#pragma unroll
      for (int i = 0; i < kRankLoads; ++i) {
        const int row = srow + kRankRowStep * i;
        const bool on = col_on && c0 + row < a.N;
        const float v = base[(on ? row : 0) * a.H];
        pf[i] = on ? v : 0.f;
      }
    }
  };
  __syncthreads();        // qs, tg written
  int ti = 0, kc = 0;
  fetch(0, 0);
  for (;;) {
    lds_barrier();        // every wave has read the previous chunk
#pragma unroll
    for (int i = 0; i < kRankLoads; ++i) cs[(srow + kRankRowStep * i) * kRankCS + scol] = pf[i];
    lds_barrier();
    int nti = ti, nkc = kc + kRankKC;
    if (nkc >= a.H) { nkc = 0; ++nti; }
    if (nti <= ntl) fetch(nti, nkc);
    const int kw = (min(kRankKC, a.H - kc) + 1) & ~1;       // the last k-group is zero-padded in LDS
    const float *qa = qs + (wave * 32 + r) * QS + kc + hi;
    const float *cb = cs + r * kRankCS + hi;
    // groups of four k-steps with their 20 operand reads issued ahead of the 16 MFMAs, then the steps that are left
    int k = 0;
    for (; k + 8 <= kw; k += 8) {
      float av[4], bv[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        av[u] = qa[k + 2 * u];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[u][j] = cb[j * 32 * kRankCS + k + 2 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][j], acc[j], 0, 0, 0);
    }
    for (; k < kw; k += 2) {
      const float av = qa[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cb[j * 32 * kRankCS + k], acc[j], 0, 0, 0);
    }
    if (nkc == 0) {       // the tile's scores are complete
      if (ti == 0) {
        // the target scores: the diagonal of this wave's own group
        const f32x16 d = wave == 0 ? acc[0] : (wave == 1 ? acc[1] : (wave == 2 ? acc[2] : acc[3]));
#pragma unroll
        for (int g = 0; g < 16; ++g)
          if (acc_row(g, hi) == r) ts[wave * 32 + r] = d[g];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int g = 0; g < 16; ++g) treg[g] = ts[wave * 32 + acc_row(g, hi)];
      } else {
        const int c0 = c_begin + (ti - 1) * kRankCT, cend = c0 + kRankCT;
        uint32_t m[4] = {0u, 0u, 0u, 0u};
        if (tgt >= c0 && tgt < cend) set_bit(m, (int)(tgt - c0));
        while (nxt < cend) {
          if (nxt >= c0) set_bit(m, (int)(nxt - c0));
          ++cur;
          nxt = cur < fend ? a.filt_idx[cur] : kRankNoEntry;
        }
        if (cend > a.N) {
          const int nv = a.N - c0;          // 1 .. kRankCT - 1 candidates of this tile exist
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int lo = nv - 32 * w;
            m[w] |= lo <= 0 ? 0xFFFFFFFFu : (lo >= 32 ? 0u : (0xFFFFFFFFu << lo));
          }
        }
        if (__ballot((m[0] | m[1] | m[2] | m[3]) != 0u) == 0ull) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
              const float s = acc[j][g];
              cg[g] += s > treg[g] ? 1 : 0;
              ce[g] += s == treg[g] ? 1 : 0;
            }
        } else {
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int owner = acc_row(g, hi);     // the lane that built this row's mask
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t mw = (uint32_t)__shfl((int)m[j], owner, kWave);
              const bool on = ((mw >> r) & 1u) == 0u;
              const float s = acc[j][g];
              cg[g] += (on && s > treg[g]) ? 1 : 0;
              ce[g] += (on && s == treg[g]) ? 1 : 0;
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;
    }
    if (nti > ntl) break;
    ti = nti;
    kc = nkc;
  }

  // ---- a row's 32 lanes (one half-wave) summed; lane g of the half adds register g's row
#pragma unroll
  for (int g = 0; g < 16; ++g) {
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
      cg[g] += __shfl_xor(cg[g], s, kWave);
      ce[g] += __shfl_xor(ce[g], s, kWave);
    }
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int q = q0 + wave * 32 + acc_row(g, hi);
    if (r == g && q < a.Q) {
      if (cg[g]) atomicAdd(a.greater + q, cg[g]);
      if (ce[g]) atomicAdd(a.equal + q, ce[g]);
    }
  }
}

constexpr int kRankMaxDevices = 64;
bool rank_lds_ready(int bytes) {
  static int have[kRankMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kRankMaxDevices) dev = 0;
  if (have[dev] >= bytes) return true;
  const int want = (int)rank_lds_bytes(kRankMaxH);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&rank_counts_k), hipFuncAttributeMaxDynamicSharedMemorySize, want);
  if (e != hipSuccess) { set_last_hip_error(e); return false; }
  have[dev] = want;
  return true;
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

int dmp_rank_supported(int H) { return H >= 1 && H <= kRankMaxH; }

int dmp_rank_counts(const float *query, const float *table, const int64_t *target, const int64_t *filt_ptr, const int64_t *filt_idx,
                    int64_t nnz, int64_t Q, int64_t N, int H, int32_t *greater, int32_t *equal, void *stream) {
  if (Q < 0 || N < 1 || H < 1 || nnz < 0) return DMP_ERR_BAD_ARG;
  if (!dmp_rank_supported(H) || N > (int64_t)INT32_MAX - 2 * kRankCT || Q > (int64_t)INT32_MAX - kRankQT) return DMP_ERR_UNSUPPORTED;
  if (Q == 0) return DMP_OK;
  if (!query || !table || !target || !greater || !equal) return DMP_ERR_BAD_ARG;
  if ((filt_ptr == nullptr) != (filt_idx == nullptr) && !(filt_ptr && nnz == 0)) return DMP_ERR_BAD_ARG;
  const size_t lds = rank_lds_bytes(H);
  if (!rank_lds_ready((int)lds)) return DMP_ERR_HIP;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(greater, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e == hipSuccess) e = hipMemsetAsync(equal, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e != hipSuccess) { set_last_hip_error(e); return DMP_ERR_HIP; }
  const int64_t qtiles = (Q + kRankQT - 1) / kRankQT, ntiles = (N + kRankCT - 1) / kRankCT;
  const int64_t want = (kRankWantGroups + qtiles - 1) / qtiles;          // splits wanted (>= 1)
  int64_t tps = (ntiles + want - 1) / want;
  if (tps < kRankMinTiles) tps = kRankMinTiles;
  const int64_t splits = (ntiles + tps - 1) / tps;                        // <= kRankWantGroups
  RankArgs a;
  a.query = query; a.table = table; a.target = target; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = filt_idx ? nnz : 0;
  a.Q = (int)Q; a.N = (int)N; a.H = H; a.tiles_per_split = (int)tps; a.greater = greater; a.equal = equal;
  hipLaunchKernelGGL(rank_counts_k, dim3((unsigned)qtiles, (unsigned)splits), dim3(kBlock), lds, st, a);
  return check_launch();
}

}  // extern "C"
