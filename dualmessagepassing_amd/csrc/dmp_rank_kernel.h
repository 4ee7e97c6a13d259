// The score-and-rank kernel: dmp_rank.hip instantiates it untyped (rank_counts_k<RankArgs>), dmp_rank_typed.hip with the
// candidates restricted by node type (rank_counts_k<RankTypedArgs>).  One translation unit per instantiation: the two do not
// share a register-allocation context, and the untyped one compiles to the instructions it had before the typed one existed.
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
//
// Types (kTyped).  tile_types[t] is the OR of 1 << type over the rows of candidate tile t (rank_tile_types_k, the pre-pass of
// dmp_rank_typed.hip; bit 63 stands for every code above 62, which nobody admits).  The workgroup ORs the `allowed` words of
// its 128 rows and walks only the tiles of its range whose word meets that union: the others are neither fetched nor
// multiplied, their filter entries are stepped over by the cursor, and a workgroup whose range holds no such tile leaves
// before it stages anything.  In a visited tile a row that does not admit every type present sets, in the SAME exclusion mask,
// all 128 bits when it admits none (the only case in a tile of one type), else the bits of the rows whose type it does not
// admit, read from the tile's 128 type bytes in LDS (staged only for a tile that straddles types).  considered_i is the sum
// over the visited tiles of 128 - popcount(mask_i): the lane that builds a row's mask counts it, no reduction.
#pragma once
#include <type_traits>

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
// ... of the typed kernel: most of its workgroups find no tile of an admitted type in their range and leave at once, and the
// ones that stay share the device the more evenly the shorter their ranges are (a range costs its start: the query rows
// and the gather tile).  PubMed's size, four types, one admitted: 0.47 of the untyped time at 2048, measured; see DESIGN.md §4.
constexpr int kRankWantGroupsTyped = 8192;
constexpr int64_t kRankNoEntry = INT64_MAX;
constexpr int kRankNoType = 63;            // the bit of a type code nobody admits (codes above 62, rows past N)
constexpr uint64_t kRankTypeBits = ~(1ull << kRankNoType);
constexpr int kRankTypedLds = 8 * kRankQT + kRankCT;      // bytes the typed kernel adds: a word per query row, the type bytes of a tile

__host__ __device__ constexpr int rank_qstride(int H) { return (H + kRankKC - 1) / kRankKC * kRankKC + 1; }
inline size_t rank_lds_bytes(int H, bool typed) {
  return sizeof(float) * ((size_t)kRankQT * rank_qstride(H) + kRankCT * kRankCS + 2 * kRankQT) + (typed ? kRankTypedLds : 0);
}

struct RankArgs {
  const float *query, *table;
  const int64_t *target, *filt_ptr, *filt_idx;
  int64_t nnz;
  int Q, N, H, tiles_per_split;
  int *greater, *equal;
};
struct RankTypedArgs : RankArgs {
  const uint8_t *cand_type;
  const uint64_t *allowed, *tile_types;
  int *considered;
};

// splits of the candidate range: tiles per workgroup of grid.y and how many of them
inline void rank_splits(int64_t Q, int64_t N, int want_groups, int64_t &qtiles, int64_t &tps, int64_t &splits) {
  qtiles = (Q + kRankQT - 1) / kRankQT;
  const int64_t ntiles = (N + kRankCT - 1) / kRankCT;
  const int64_t want = (want_groups + qtiles - 1) / qtiles;              // splits wanted (>= 1)
  tps = (ntiles + want - 1) / want;
  if (tps < kRankMinTiles) tps = kRankMinTiles;
  splits = (ntiles + tps - 1) / tps;                                      // <= want_groups
}

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

// A lane index that the optimiser must take as it finds it here: an address needed once in many tiles (the typed kernel's side
// paths) is then formed where it is used, not ahead of the loop and held -- or spilled -- across it.
__device__ __forceinline__ int formed_here(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// The next tile of a workgroup's range [tile_begin, tile_begin + ntl) whose word meets `un`, after the ones handed out
// (relative index), ntl when none is left: 64 tile words a load, one per lane, and the ballot of those that meet the union.
__device__ __forceinline__ int rank_next_tile(const uint64_t *tile_types, int tile_begin, int ntl, int lane, uint64_t un, int &vbase,
                                              uint64_t &vmap) {
  while (vmap == 0ull) {
    vbase += kWave;
    if (vbase >= ntl) return ntl;
    const int t = vbase + formed_here(lane);
    const uint64_t w = t < ntl ? tile_types[tile_begin + t] : 0ull;
    vmap = __ballot((w & un) != 0ull);
  }
  const int t = vbase + __builtin_ctzll(vmap);
  vmap &= vmap - 1;
  return t;
}

// (two waves per SIMD: left to itself the register allocator takes 305 registers and spills scalars for the 64 comparisons of a tile)
template <class Args>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void rank_counts_k(Args a) {
  constexpr bool kTyped = std::is_same<Args, RankTypedArgs>::value;
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
  const int myq = q0 + wave * 32 + r;                  // this lane's row

  // ---- (typed) the types this workgroup's rows admit, and the walk over the tiles of its range that hold one of them
  uint64_t *am = reinterpret_cast<uint64_t *>(tg + kRankQT);     // [kRankQT]      the types a row admits (bit kRankNoType clear)
  uint32_t *ty = reinterpret_cast<uint32_t *>(am + kRankQT);     // [kRankCT / 4]  the type bytes of a tile that straddles types
  uint64_t un = 0ull, vmap = 0ull, tw = 0ull, ntw = 0ull;
  int vbase = -kWave, cons = 0;
  if constexpr (kTyped) {
    if (tid < kRankQT) am[tid] = q0 + tid < a.Q ? (a.allowed[q0 + tid] & kRankTypeBits) : 0ull;
    __syncthreads();
    const uint64_t two = am[lane] | am[lane + kWave];       // every wave folds all 128 words: no second exchange
    uint32_t lo = (uint32_t)two, up = (uint32_t)(two >> 32);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      lo |= (uint32_t)__shfl_xor((int)lo, s, kWave);
      up |= (uint32_t)__shfl_xor((int)up, s, kWave);
    }
    un = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)up) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
  }
  int first = 1;
  if constexpr (kTyped) {
    first = rank_next_tile(a.tile_types, tile_begin, ntl, lane, un, vbase, vmap) + 1;
    if (first > ntl) return;        // nothing here that a row of this workgroup admits (uniform: un is the workgroup's)
  }

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
  // the target score of register g's row: kept in registers, or (typed, which has sixteen fewer to spare) re-read per tile
  auto tscore = [&](int g) -> float {
    if constexpr (kTyped) return ts[wave * 32 + acc_row(g, hi)]; else return treg[g];
  };

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
      if constexpr (kTyped) {
        if (kc == 0) ntw = a.tile_types[tile_begin + ti - 1];
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
    if constexpr (kTyped) {
      if (kc == 0 && ti >= 1 && (tw & (tw - 1)) != 0ull && tid < kRankCT / 4) {       // a tile that straddles types: its bytes, four a thread
        const int slot = formed_here(tid), c0 = c_begin + (ti - 1) * kRankCT + 4 * slot;
        uint32_t four = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t t = c0 + b < a.N ? a.cand_type[c0 + b] : (uint32_t)kRankNoType;
          four |= (t > kRankNoType ? kRankNoType : t) << (8 * b);
        }
        ty[slot] = four;
      }
    }
    lds_barrier();
    int nti = ti, nkc = kc + kRankKC;
    if (nkc >= a.H) {
      nkc = 0;
      if constexpr (kTyped) nti = ti == 0 ? first : rank_next_tile(a.tile_types, tile_begin, ntl, lane, un, vbase, vmap) + 1; else ++nti;
    }
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
        for (int g = 0; g < 16; ++g) treg[g] = ts[wave * 32 + acc_row(g, hi)];       // (dead in the typed kernel)
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
        if constexpr (kTyped) {
          const uint64_t amask = am[wave * 32 + r];
          if ((tw & ~amask) != 0ull) {        // a type is present here that this row does not admit
            if ((tw & amask) == 0ull) {
              m[0] = m[1] = m[2] = m[3] = 0xFFFFFFFFu;
            } else {
              const uint64_t refused = ~amask;          // bit kRankNoType is set
#pragma unroll
              for (int w = 0; w < 4; ++w) {
                uint32_t bits = 0u;
                for (int b = 0; b < 8; ++b) {
                  const uint32_t four = ty[8 * w + b];
#pragma unroll
                  for (int e = 0; e < 4; ++e) bits |= (uint32_t)((refused >> ((four >> (8 * e)) & 63u)) & 1ull) << (4 * b + e);
                }
                m[w] |= bits;
              }
            }
          }
          cons += kRankCT - (__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]));
        }
        if (__ballot((m[0] | m[1] | m[2] | m[3]) != 0u) == 0ull) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
              const float s = acc[j][g];
              cg[g] += s > tscore(g) ? 1 : 0;
              ce[g] += s == tscore(g) ? 1 : 0;
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
              cg[g] += (on && s > tscore(g)) ? 1 : 0;
              ce[g] += (on && s == tscore(g)) ? 1 : 0;
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
    if constexpr (kTyped) {
      if (nkc == 0) tw = ntw;
    }
  }

  int wq = q0 + wave * 32;      // the wave's first row
  if constexpr (kTyped) wq = q0 + formed_here(tid) / kWave * 32;
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
    const int q = wq + acc_row(g, hi);
    if (r == g && q < a.Q) {
      if (cg[g]) atomicAdd(a.greater + q, cg[g]);
      if (ce[g]) atomicAdd(a.equal + q, ce[g]);
    }
  }
  if constexpr (kTyped) {       // both halves of the wave built the row's mask: the lower one reports
    const int q = wq + r;
    if (hi == 0 && q < a.Q && cons) atomicAdd(a.considered + q, cons);
  }
}

constexpr int kRankMaxDevices = 64;
// raises the kernel's dynamic LDS limit once per device; `have`: the kernel's own [kRankMaxDevices] record
inline bool rank_lds_ready(const void *kernel, int bytes, int want, int *have) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kRankMaxDevices) dev = 0;
  if (have[dev] >= bytes) return true;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, want);
  if (e != hipSuccess) { set_last_hip_error(e); return false; }
  have[dev] = want;
  return true;
}

}  // namespace
}  // namespace dmp
