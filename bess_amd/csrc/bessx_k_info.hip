// bessx_k_info.hip -- expected information and score of ONE model (identity, logistic or Poisson link) on a caller's
// DEVICE matrix, read where it lies, the support's columns only:
//     eta_i = sum_k X(i, cols[k]) * beta[k] + c          (the loops of bessx_k_xb.hpp, unchanged)
//     z_i   = (1, X(i, cols[0]), ..., X(i, cols[m - 1])),                M = m + 1 entries
//     I     = sum_i v_i z_i z_i^T   (M x M),      U = sum_i g_i z_i   (M)
//   link        mu_i                        v_i                       g_i
//   identity    eta_i                       w_i                       w_i (y_i - eta_i)
//   logistic    p_i = 1 / (1 + e^-eta_i)    w_i p_i (1 - p_i)         w_i (y_i - p_i)      (overflow-free, no clamp)
//   Poisson     e^eta_i                     w_i e^eta_i               w_i (y_i - e^eta_i)
// plus L = sum_i w_i f(eta_i, y_i) and sum_i w_i from launch_eval itself (bessx_k_eval.hip, R = 1): the same bits as
// bessx_eval_device.  Three steps:
//   1. eta pass: xb_launch with the store epilogue InfoStore writes v_i and g_i into two n-vectors of workspace.
//   2. k_info_gram: 16 x 16 tiles of D = A^T B on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  A = z, unweighted;
//      B = the M columns v_i z_i and, as one more tile column, g_i: one sweep over the rows gives I and U.  Tile row
//      It (16 entries of z) has It + 2 tile slots: slots 0 .. It are the tiles (It, J <= It) of I -- the lower triangle --
//      and slot It + 1 holds U (its column 0).  One wave = one task (tile row, run of up to IG_JC slots, row slab): it
//      loads its A operand once per step and feeds it to the run's tiles; waves are independent (no LDS, no barriers).
//      Lane (c = lane & 15, q = lane >> 4) supplies A[c][k = q] and B[k = q][c]; which row of X a k slot means is free as
//      long as A and B agree, so the lane takes E consecutive rows i0 = step + q * E .. + E - 1 of its column (one
//      16-byte load when the source allows: E = 2 doubles or 4 floats) and feeds element e to the e-th of E MFMAs.
//      Three access shapes, the same arithmetic in the same order: 16-byte loads (column-contiguous source, aligned
//      base and column stride); element loads at any strides; a row-contiguous source takes the element loads with
//      the 16 lanes of a k slot gathering the support's columns of one row (the shape of k_xb_gather).
//      Masking: the intercept entry is the constant 1 and is not read; rows >= n and tile entries >= M enter as exact
//      zeros in BOTH operands and are not read, so a NaN outside the n x m support view never reaches a sum.  Inside
//      the view 0 * NaN is NaN: a NaN in a support column of a row with v_i = 0 does propagate.
//      Every wave writes one partial per tile: part[(slab * T + tile) * 256 + reg * 64 + lane].
//   3. k_info_finish adds the slabs' partials of every tile entry in a fixed order (16 lanes per entry: lane l takes
//      slabs l, l + 16, ... in slab order, the 16 sums go through the DPP tree of pr_group_sum) and writes both
//      triangles of I from the lower one (bit-identical mirrors), then U.
// No floating-point atomics anywhere: the same call gives the same bits.  The slab count depends on (n, m) only.
#include "bessx_k_infogram.hpp"

namespace bessx {

namespace {

__device__ __forceinline__ double info_load(const void *p, int f32, long long off) {
  return f32 ? (double)static_cast<const float *>(p)[off] : static_cast<const double *>(p)[off];
}

// the epilogue of the eta pass: working weight and score weight of row i
struct InfoStore {
  static constexpr bool REDUCE = false, SKIPZ = false;
  EvalData d;
  int link;
  double *__restrict__ v;
  double *__restrict__ g;
  __device__ __forceinline__ void store(double eta, long long i, int) const {
    const double y = info_load(d.y, d.y_f32, i * d.yrs);
    const double w = d.w ? info_load(d.w, d.w_f32, i * d.ws) : 1.0;
    double vi, gi;
    if (link == PREDICT_LOGISTIC) {
      // t = e^-|eta| <= 1: p = 1 / (1 + t) or t / (1 + t), p (1 - p) = t / (1 + t)^2 -- nothing overflows and 1 - p is
      // never formed by a subtraction (comparisons, not fmax: a NaN eta stays a NaN)
      const double t = exp(-fabs(eta)), s = 1.0 + t;
      const double p = (eta >= 0.0 ? 1.0 : t) / s;
      vi = w * (t / (s * s));
      gi = w * (y - p);
    } else if (link == PREDICT_POISSON) {
      const double e = exp(eta);
      vi = w * e;
      gi = w * (y - e);
    } else {
      vi = w;
      gi = w * (y - eta);
    }
    v[i] = vi;
    g[i] = gi;
  }
};

}  // namespace

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) k_info_gram(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                   const int *__restrict__ cols, int M, const double *__restrict__ vw,
                                                   const double *__restrict__ gw, long long rps, int slabs, int T_tiles,
                                                   double *__restrict__ part) {
  constexpr int E = VEC ? PrVec<T>::N : 4;
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int s = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
  if (s >= slabs) return;  // (wave-uniform; the kernel has no barrier)
  int It = 0, run = (int)blockIdx.x;
  while (run >= (It + 2 + IG_JC - 1) / IG_JC) {
    run -= (It + 2 + IG_JC - 1) / IG_JC;
    It++;
  }
  const int slot0 = run * IG_JC, nJ = min(IG_JC, It + 2 - slot0);
  const T *pa;
  const int ka = ig_entry(src, cs, cols, M, 16 * It + c, &pa);
  const T *pb[IG_JC];
  int kb[IG_JC];
  bool need_g = false;
#pragma unroll
  for (int jj = 0; jj < IG_JC; jj++) {
    const int slot = slot0 + jj;
    pb[jj] = src;
    kb[jj] = IG_ZERO;
    if (jj < nJ) {
      if (slot <= It) {
        kb[jj] = ig_entry(src, cs, cols, M, 16 * slot + c, &pb[jj]);
      } else {
        kb[jj] = c == 0 ? IG_G : IG_ZERO;
        need_g = true;
      }
    }
  }
  d4 acc[IG_JC];
#pragma unroll
  for (int jj = 0; jj < IG_JC; jj++) acc[jj] = d4{0.0, 0.0, 0.0, 0.0};
  const long long r_end = min(n, ((long long)s + 1) * rps);
  for (long long rb = (long long)s * rps; rb < r_end; rb += 4 * E) {
    const long long i0 = rb + (long long)q * E;
    double vv[E], gg[E], xa[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      const bool in = i0 + e < n;
      vv[e] = in ? vw[i0 + e] : 0.0;
      gg[e] = (in && need_g) ? gw[i0 + e] : 0.0;
    }
    ig_rows<T, VEC, E>(ka, pa, rs, i0, n, xa);
#pragma unroll
    for (int jj = 0; jj < IG_JC; jj++) {
      if (jj < nJ) {  // (wave-uniform)
        double xb[E];
        if (slot0 + jj == It) {
#pragma unroll
          for (int e = 0; e < E; e++) xb[e] = xa[e];  // the diagonal tile: B's entry is A's
        } else {
          ig_rows<T, VEC, E>(kb[jj], pb[jj], rs, i0, n, xb);
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
          // (an entry past M, and the U slot's columns 1 .. 15, are exact zeros whatever v_i is)
          const double b = kb[jj] == IG_G ? gg[e] : (kb[jj] == IG_ZERO ? 0.0 : xb[e] * vv[e]);
          acc[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[e], b, acc[jj], 0, 0, 0);
        }
      }
    }
  }
  const long long t0 = (long long)It * (It + 3) / 2 + slot0;
#pragma unroll
  for (int jj = 0; jj < IG_JC; jj++) {
    if (jj < nJ) {
      double *o = part + ((long long)s * T_tiles + t0 + jj) * 256 + lane;
      o[0] = acc[jj].x;
      o[64] = acc[jj].y;
      o[128] = acc[jj].z;
      o[192] = acc[jj].w;
    }
  }
}

// block (tile, quarter): thread t = 16 * grp + lg sums entries e = 64 * quarter + 4 * grp .. + 3 of the tile over the
// slabs lg, lg + 16, ... in slab order; the 16 lanes of a group are then added by the DPP tree.  Entry e = 64 * reg +
// lane is D[row = (lane >> 4) + 4 * reg][col = lane & 15] of the tile (the C/D layout of the f64 MFMA).
__global__ void __launch_bounds__(256) k_info_finish(const double *__restrict__ part, int slabs, int T_tiles, int M,
                                                     double *__restrict__ info, long long ld,
                                                     double *__restrict__ score) {
  const int tile = (int)blockIdx.x, lg = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int e0 = (int)blockIdx.y * 64 + grp * 4;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = lg; s < slabs; s += 16) {
    const double *p = part + ((long long)s * T_tiles + tile) * 256 + e0;
    const d2 lo = *reinterpret_cast<const d2 *>(p), hi = *reinterpret_cast<const d2 *>(p + 2);
    sum[0] += lo.x;
    sum[1] += lo.y;
    sum[2] += hi.x;
    sum[3] += hi.y;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) sum[j] = pr_group_sum<16>(sum[j]);
  if (lg != 0) return;
  int It = 0;
  while ((It + 1) * (It + 4) / 2 <= tile) It++;
  const int slot = tile - It * (It + 3) / 2;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int e = e0 + j, reg = e >> 6, ln = e & 63;
    const int a = 16 * It + (ln >> 4) + 4 * reg, bl = ln & 15;
    if (a >= M) continue;
    if (slot > It) {
      if (bl == 0) score[a] = sum[j];
    } else {
      const int b = 16 * slot + bl;
      if (b <= a) {  // (b <= a < M) the lower triangle names the value, the upper one is its mirror
        info[(long long)a * ld + b] = sum[j];
        info[(long long)b * ld + a] = sum[j];
      }
    }
  }
}

// the split of a problem as the tests' bound needs it: rows per slab and slabs (a function of n and m alone)
void info_split(long long n, int m, long long *rows_per_slab, int *slabs) {
  const InfoSplit sp = ig_split(n, m + 1);
  *rows_per_slab = sp.rps;
  *slabs = sp.slabs;
}

// doubles of the tiles' partials: slabs * T * 256, at most IG_SLABS_MAX * T * 256 whatever n is
long long info_gram_workspace(long long n, int m) {
  const InfoSplit sp = ig_split(n, m + 1);
  return (long long)sp.slabs * sp.T * 256;
}

// doubles of workspace launch_info needs: v and g, the tiles' partials, and what launch_eval needs for R = 1
long long info_workspace(int f32, long long rs, long long cs, long long n, int m, int link, int weighted) {
  return 2 * ((n + 1) / 2 * 2) + info_gram_workspace(n, m) + eval_workspace(f32, rs, cs, n, m, 1, link, weighted);
}

template <typename T>
static hipError_t info_launch_gram(const T *src, long long rs, long long cs, long long n, const int *cols, int M,
                                   const double *vw, const double *gw, const InfoSplit &sp, double *part,
                                   hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const dim3 grid((unsigned)sp.tasks, (unsigned)((sp.slabs + 3) / 4));
  if (vec)
    hipLaunchKernelGGL((k_info_gram<T, true>), grid, dim3(256), 0, st, src, rs, cs, n, cols, M, vw, gw, sp.rps, sp.slabs,
                       sp.T, part);
  else
    hipLaunchKernelGGL((k_info_gram<T, false>), grid, dim3(256), 0, st, src, rs, cs, n, cols, M, vw, gw, sp.rps,
                       sp.slabs, sp.T, part);
  LAUNCH_CHECK();
  return hipSuccess;
}

// the Gram sweep and its finish alone (bessx_op_info_bench times these two): v, g are n doubles each, part
// slabs * T * 256 doubles, info (m + 1) x (m + 1) with leading dimension ld, score m + 1 doubles -- device memory
hipError_t launch_info_gram(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                            const double *vw, const double *gw, double *part, double *info, long long ld, double *score,
                            hipStream_t st) {
  if (!src || !vw || !gw || !part || !info || !score || n < 1 || n > 0x7fffffffLL || m < 0 || m + 1 > INFO_M_MAX ||
      (m > 0 && !cols) || rs < 0 || cs < 0 || ld < m + 1)
    return hipErrorInvalidValue;
  const int M = m + 1;
  const InfoSplit sp = ig_split(n, M);
  hipError_t e = f32 ? info_launch_gram(static_cast<const float *>(src), rs, cs, n, cols, M, vw, gw, sp, part, st)
                     : info_launch_gram(static_cast<const double *>(src), rs, cs, n, cols, M, vw, gw, sp, part, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_info_finish, dim3((unsigned)sp.T, 4), dim3(256), 0, st, part, sp.slabs, sp.T, M, info, ld, score);
  LAUNCH_CHECK();
  return hipSuccess;
}

// info (ld >= m + 1), score (m + 1) and res (3 doubles: L, the logistic link's count of correct labels, sum of the
// weights when d.w is given -- launch_eval's res for R = 1) are device memory; work: info_workspace(...) doubles.
// src, cols, B (m doubles), c (one double) as in launch_predict with R = 1.
hipError_t launch_info(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                       const double *B, const double *c, int link, const EvalData &d, double *work, double *res,
                       double *info, long long ld, double *score, hipStream_t st) {
  if (!src || !c || !d.y || !work || !res || !info || !score || n < 1 || n > 0x7fffffffLL || m < 0 ||
      m + 1 > INFO_M_MAX || (m > 0 && (!cols || !B)) || rs < 0 || cs < 0 || d.yrs < 0 || d.ws < 0 || ld < m + 1 ||
      link < PREDICT_IDENTITY || link > PREDICT_POISSON)
    return hipErrorInvalidValue;
  const InfoSplit sp = ig_split(n, m + 1);
  const long long nv = (n + 1) / 2 * 2;  // (the partials stay 16-byte aligned behind v and g)
  double *vw = work, *gw = work + nv, *part = work + 2 * nv, *ework = part + (long long)sp.slabs * sp.T * 256;
  const InfoStore epi{d, link, vw, gw};
  hipError_t e = f32 ? xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, c, 1, epi, st)
                     : xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, c, 1, epi, st);
  if (e != hipSuccess) return e;
  e = launch_info_gram(src, f32, rs, cs, n, cols, m, vw, gw, part, info, ld, score, st);
  if (e != hipSuccess) return e;
  EvalData d1 = d;
  d1.ycs = 0;
  return launch_eval(src, f32, rs, cs, n, cols, m, B, c, 1, link, d1, ework, res, st);
}

// the eta pass alone, ALWAYS k_xb_rows (never k_xb_gather, whose sums have another order): v_i and g_i are the same
// bits under every layout of X, which the robust covariance's cluster sums rely on (bessx_k_sandwich.hip)
template <typename T>
static hipError_t info_launch_vg_rows(const T *src, long long rs, long long cs, long long n, const int *cols, int m,
                                      const double *B, const double *c, const InfoStore &epi, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const long long rows_per_block = 64LL * PrVec<T>::N;
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block), 1);
  if (vec)
    hipLaunchKernelGGL((k_xb_rows<T, 1, true, InfoStore>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, c, 1, epi);
  else
    hipLaunchKernelGGL((k_xb_rows<T, 1, false, InfoStore>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, c, 1, epi);
  LAUNCH_CHECK();
  return hipSuccess;
}

// whether launch_info's own eta pass is k_xb_rows, i.e. its v and g are already those of launch_info_vg
bool info_eta_by_rows(long long rs, long long cs, int m) { return !(cs == 1 && rs != 1 && m > 0); }

hipError_t launch_info_vg(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                          const double *B, const double *c, int link, const EvalData &d, double *v, double *g,
                          hipStream_t st) {
  if (!src || !c || !d.y || !v || !g || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || rs < 0 ||
      cs < 0 || d.yrs < 0 || d.ws < 0 || link < PREDICT_IDENTITY || link > PREDICT_POISSON)
    return hipErrorInvalidValue;
  const InfoStore epi{d, link, v, g};
  return f32 ? info_launch_vg_rows(static_cast<const float *>(src), rs, cs, n, cols, m, B, c, epi, st)
             : info_launch_vg_rows(static_cast<const double *>(src), rs, cs, n, cols, m, B, c, epi, st);
}

}  // namespace bessx
