// Rank counts of a link predictor's decoder (unc_eval.py): for every query row i, how many candidates of a table score
// above / exactly at the score of the query's target,
//
//   score(i, c) = sum_h query[i, h] table[c, h],   t_i = score(i, target_i),
//   greater_i = #{c in C_i : score(i, c) > t_i},   equal_i = #{c in C_i : score(i, c) == t_i},
//   C_i = {c : c != target_i and c not in filt_i}                      (membership by INDEX, never by value)
//
// without the [Q, N] score matrix ever leaving the registers.  The kernel, with its geometry, arithmetic and counting, is
// dmp_rank_kernel.h; this is its untyped instantiation (the one restricted by node type: dmp_rank_typed.hip).
#include "dmp_rank_kernel.h"

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
  const size_t lds = rank_lds_bytes(H, false);
  static int have[kRankMaxDevices] = {};
  if (!rank_lds_ready(reinterpret_cast<const void *>(&rank_counts_k<RankArgs>), (int)lds, (int)rank_lds_bytes(kRankMaxH, false), have)) return DMP_ERR_HIP;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(greater, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e == hipSuccess) e = hipMemsetAsync(equal, 0, sizeof(int32_t) * (size_t)Q, st);
  if (e != hipSuccess) { set_last_hip_error(e); return DMP_ERR_HIP; }
  int64_t qtiles, tps, splits;
  rank_splits(Q, N, kRankWantGroups, qtiles, tps, splits);
  RankArgs a;
  a.query = query; a.table = table; a.target = target; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = filt_idx ? nnz : 0;
  a.Q = (int)Q; a.N = (int)N; a.H = H; a.tiles_per_split = (int)tps; a.greater = greater; a.equal = equal;
  hipLaunchKernelGGL(rank_counts_k<RankArgs>, dim3((unsigned)qtiles, (unsigned)splits), dim3(kBlock), lds, st, a);
  return check_launch();
}

}  // extern "C"
