// bessx_k_infogram.hpp -- what the matrix-core Gram sweeps share (k_info_gram of bessx_k_info.hip and its three-weight
// form k_cxz_gram of bessx_k_coxzph.hip): the tile and slab split of a problem, what a lane's entry of an operand is and
// how its rows are loaded.  A unit that includes this gives a tile the same rows in the same order as every other.
#ifndef BESSX_K_INFOGRAM_HPP
#define BESSX_K_INFOGRAM_HPP
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int IG_JC = 4;           // tile slots a wave carries
constexpr int IG_WAVES = 4096;     // waves aimed at when the rows are split into slabs
constexpr int IG_SLABS_MAX = 256;  // at most this many slabs: workspace <= IG_SLABS_MAX * T * 256 doubles
constexpr int IG_RPS_MIN = 64;     // fewest rows per slab (a multiple of 16)

// tiles, tasks and the row split of a problem: a function of (n, M) alone
struct InfoSplit {
  int TI, T, tasks, slabs;
  long long rps;
};
inline InfoSplit ig_split(long long n, int M) {
  InfoSplit sp;
  sp.TI = (M + 15) / 16;
  sp.T = sp.TI * (sp.TI + 3) / 2;
  sp.tasks = 0;
  for (int I = 0; I < sp.TI; I++) sp.tasks += (I + 2 + IG_JC - 1) / IG_JC;
  const long long target = std::min<long long>(IG_SLABS_MAX, std::max<long long>(1, IG_WAVES / sp.tasks));
  long long rps = ((n + target - 1) / target + 15) / 16 * 16;
  sp.rps = std::max<long long>(rps, IG_RPS_MIN);
  sp.slabs = (int)((n + sp.rps - 1) / sp.rps);
  return sp;
}

enum { IG_ZERO = 0, IG_ONE = 1, IG_COL = 2, IG_G = 3 };  // what a lane's entry of an operand is

// entry `a` of z as an operand: its kind and, for a column of X, where it starts
template <typename T>
__device__ __forceinline__ int ig_entry(const T *src, long long cs, const int *__restrict__ cols, int M, int a,
                                        const T **ptr) {
  *ptr = src;
  if (a == 0) return IG_ONE;
  if (a >= M) return IG_ZERO;
  *ptr = src + (long long)cols[a - 1] * cs;
  return IG_COL;
}

// rows i0 .. i0 + E - 1 of an entry of z (exact zeros past n; only a column of X is read)
template <typename T, bool VEC, int E>
__device__ __forceinline__ void ig_rows(int kind, const T *cp, long long rs, long long i0, long long n, double *x) {
#pragma unroll
  for (int e = 0; e < E; e++) x[e] = (kind == IG_ONE && i0 + e < n) ? 1.0 : 0.0;
  if (kind == IG_COL) {
    if constexpr (VEC) {
      if (i0 + E <= n) {
        pr_unpack(*reinterpret_cast<const typename PrVec<T>::type *>(cp + i0), x);
        return;
      }
    }
#pragma unroll
    for (int e = 0; e < E; e++)
      if (i0 + e < n) x[e] = (double)cp[(i0 + e) * rs];
  }
}

}  // namespace

}  // namespace bessx

#endif  // BESSX_K_INFOGRAM_HPP
