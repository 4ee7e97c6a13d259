// Rank counts against the candidates of the admitted node types (unc_eval.rank_counts_typed): dmp_rank_counts with
//
//   C_i = {c : c != target_i, c not in filt_i, bit cand_type[c] of allowed_i set},   considered_i = |C_i|,
//
// t_i the target's score whatever its type.  Two launches: the pre-pass below writes one word per candidate tile, the OR of
// 1 << type over its rows; the typed instantiation of dmp_rank_kernel.h walks only the tiles whose word meets the types its
// workgroup's rows admit.  Its own translation unit: the untyped kernel (dmp_rank.hip) keeps its code.
#include "dmp_rank_kernel.h"

namespace dmp {
namespace {

// one workgroup of kRankCT threads per candidate tile: a row's bit, OR-reduced over the wave, then over the waves in LDS
__global__ __launch_bounds__(kRankCT) void rank_tile_types_k(const uint8_t *cand_type, int N, uint64_t *tile_types, int64_t *status) {
  __shared__ uint64_t part[kRankCT / kWave];
  const int c = blockIdx.x * kRankCT + threadIdx.x, wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  uint64_t w = 0ull;
  if (c < N) {
    const int t = cand_type[c];
    w = 1ull << (t > kRankNoType ? kRankNoType : t);
  }
  uint32_t lo = (uint32_t)w, up = (uint32_t)(w >> 32);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, s, kWave);
    up |= (uint32_t)__shfl_xor((int)up, s, kWave);
  }
  if (lane == 0) part[wave] = ((uint64_t)up << 32) | lo;
  __syncthreads();
  if (threadIdx.x == 0) {
    w = 0ull;
#pragma unroll
    for (int i = 0; i < kRankCT / kWave; ++i) w |= part[i];
    tile_types[blockIdx.x] = w;
    if ((w >> kRankNoType) != 0ull && status) *status = DMP_RANK_BAD_TYPE;      // every writer stores the same value
  }
}

}  // namespace
}  // namespace dmp

using namespace dmp;

extern "C" {

size_t dmp_rank_typed_workspace_words(int64_t N) { return N < 1 ? 0 : (size_t)((N + kRankCT - 1) / kRankCT); }

int dmp_rank_counts_typed(const float *query, const float *table, const int64_t *target, const int64_t *filt_ptr, const int64_t *filt_idx,
                          int64_t nnz, const uint8_t *cand_type, const uint64_t *allowed, int64_t Q, int64_t N, int H, int32_t *greater,
                          int32_t *equal, int32_t *considered, uint64_t *tile_types, int64_t *status, void *stream) {
  if (Q < 0 || N < 1 || H < 1 || nnz < 0) return DMP_ERR_BAD_ARG;
  if (!dmp_rank_supported(H) || N > (int64_t)INT32_MAX - 2 * kRankCT || Q > (int64_t)INT32_MAX - kRankQT) return DMP_ERR_UNSUPPORTED;
  if (!cand_type || !allowed || !tile_types) return DMP_ERR_BAD_ARG;
  if (Q > 0 && (!query || !table || !target || !greater || !equal || !considered)) return DMP_ERR_BAD_ARG;
  if ((filt_ptr == nullptr) != (filt_idx == nullptr) && !(filt_ptr && nnz == 0)) return DMP_ERR_BAD_ARG;
  const size_t lds = rank_lds_bytes(H, true);
  static int have[kRankMaxDevices] = {};
  if (!rank_lds_ready(reinterpret_cast<const void *>(&rank_counts_k<RankTypedArgs>), (int)lds, (int)rank_lds_bytes(kRankMaxH, true), have)) return DMP_ERR_HIP;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = status ? hipMemsetAsync(status, 0, sizeof(int64_t), st) : hipSuccess;
  if (e == hipSuccess && Q > 0) e = hipMemsetAsync(greater, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e == hipSuccess && Q > 0) e = hipMemsetAsync(equal, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e == hipSuccess && Q > 0) e = hipMemsetAsync(considered, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e != hipSuccess) { set_last_hip_error(e); return DMP_ERR_HIP; }
  const int64_t ntiles = (N + kRankCT - 1) / kRankCT;
  hipLaunchKernelGGL(rank_tile_types_k, dim3((unsigned)ntiles), dim3(kRankCT), 0, st, cand_type, (int)N, tile_types, status);
  if (Q == 0) return check_launch();
  int64_t qtiles, tps, splits;
  rank_splits(Q, N, kRankWantGroupsTyped, qtiles, tps, splits);
  RankTypedArgs a;
  a.query = query; a.table = table; a.target = target; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = filt_idx ? nnz : 0;
  a.Q = (int)Q; a.N = (int)N; a.H = H; a.tiles_per_split = (int)tps; a.greater = greater; a.equal = equal;
  a.cand_type = cand_type; a.allowed = allowed; a.tile_types = tile_types; a.considered = considered;
  hipLaunchKernelGGL(rank_counts_k<RankTypedArgs>, dim3((unsigned)qtiles, (unsigned)splits), dim3(kBlock), lds, st, a);
  return check_launch();
}

}  // extern "C"
