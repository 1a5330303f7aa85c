// bessx_k_sandwich.hip -- the "meat" of a robust (sandwich) covariance on a caller's DEVICE matrix, read where it lies
// (include/bessx.h section 2k):
//     B = sum_i u_i^2 z_i z_i^T                        without clusters
//     B = sum_g s_g s_g^T,   s_g = sum_{i in g} u_i z_i   with clusters of rows
// z_i = (1, X(i, cols[0]), ...) (intercept != 0) or (X(i, cols[0]), ...) (a dense source such as the Cox score
// residuals L), Ms entries; u_i a row scalar (null: ones).  Without clusters and with the intercept, B is one sweep of
// launch_info_gram (bessx_k_info.hip) over X in place with vw = u^2.  What is new here:
//   1. k_sw_sums: the segmented sums S(g, a) = sum_{i in g} u_i z_ia.  The host sorts the rows by label (stable: a
//      cluster's rows keep their original order) and cuts every cluster into RUNS of at most SW_RUN = 64 consecutive
//      rows of it; rptr[j] .. rptr[j + 1] are run j's positions in the sorted order, rowof[k] the row at position k (null:
//      the identity, labels already sorted).  One work item = (run j, entry a): acc = 0, then acc = fma(u_i, z_ia, acc)
//      over the run's rows in order -- a chain of at most 64 FMAs whose loads do not depend on one another.  A cluster
//      of one run writes S(g, a) itself (rdst[j] = g >= 0); a longer cluster writes the run's partial to P(-1 - rdst[j],
//      a) and k_sw_fold adds the cluster's partials in run order.  Additions behind S(g, a) for a cluster of r rows:
//      min(r, 64) + ceil(r / 64) - 1 (sandwich_sum_depth); the bits depend on the cluster's rows in their original
//      order and on u alone, not on the layout of X, n, the cluster's place or the other clusters.
//      Three access shapes, the same arithmetic in the same order:
//        16-byte loads: rowof is the identity and the source is column-contiguous with an aligned base and column
//          stride; lanes along runs, a lane walks its run's rows of a column with one 16-byte load per E = 2 (fp64) or
//          4 (fp32) rows (element loads up to the first aligned row and behind the last full group);
//        element loads at any strides: lanes along runs (coalesced-ish for a column-contiguous source whose runs are
//          short and neighbouring), the rows through rowof;
//        row-contiguous source (col_stride == 1): 16 lanes along the support's entries of one run, 16 runs per workgroup
//          -- the gather shape of k_xb_gather.
//      In the first two shapes a thread carries SW_AE = 4 entries, so u and rowof are read once per four columns.
//      Masking is k_info_gram's: the constant entry is not read, nothing outside the n x m view is read (a run's rows
//      are rows < n by construction, entries >= Ms have no work item), and a NaN inside the view propagates.
//   2. k_sw_u: u_i = g_i (HC0 / HC1), g_i / sqrt(1 - h_i) (HC2), g_i / (1 - h_i) (HC3) and u_i^2; no clamp.
//   3. launch_sandwich_gram: B from S by launch_info_gram on S as a dense G x (Ms - 1) matrix (columns 1 .. Ms - 1 of S
//      through an iota column list) with vw = ones and gw = S(:, 0): the sweep's "intercept" row is then the sum vector
//      sum_g S(g, a), its information block the entries (a, b >= 1) of B, its score B(0, a) for a >= 1 and sum_g S(g, 0)
//      at a = 0.  The one entry it does not give, B(0, 0) = sum_g S(g, 0)^2, is k_sw_sq: one workgroup, thread t adds
//      the squares g = t, t + 256, ... by FMA in that order, then a fixed LDS tree: ceil(G / 256) + 8 additions.  So
//      the sweep runs with Ms - 1 columns and Ms <= 1024 = INFO_M_MAX holds with no column lost.  k_sw_fix writes both
//      triangles of B (exact mirrors) and the sum vector.  A dense source without labels and without u (the Cox score
//      residuals L) takes the same route with x in the place of S: its first support column is copied to an n-vector
//      (k_sw_column) and the sweep reads the others in place -- no n x m copy.
// No floating-point atomics, no LDS besides k_sw_sq's tree: the same call gives the same bits.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int SW_RUN = 64;  // rows per run of a cluster
constexpr int SW_AE = 4;    // entries of z a thread carries when the lanes go along the runs

// rows k0 .. k1 - 1 (positions = rows: the identity order) of a column-contiguous column, 16-byte loads where aligned
template <typename T>
__device__ __forceinline__ double sw_run_vec(const T *__restrict__ cp, const double *__restrict__ u, long long k0,
                                             long long k1) {
  constexpr int E = PrVec<T>::N;
  double acc = 0.0;
  long long k = k0;
  for (; k < k1 && (k & (E - 1)); k++) acc = fma(u ? u[k] : 1.0, (double)cp[k], acc);
  for (; k + E <= k1; k += E) {
    double x[E];
    pr_unpack(*reinterpret_cast<const typename PrVec<T>::type *>(cp + k), x);
#pragma unroll
    for (int e = 0; e < E; e++) acc = fma(u ? u[k + e] : 1.0, x[e], acc);
  }
  for (; k < k1; k++) acc = fma(u ? u[k] : 1.0, (double)cp[k], acc);
  return acc;
}

__device__ __forceinline__ void sw_put(double v, int dst, int a, double *__restrict__ S, long long ldS,
                                       double *__restrict__ P, long long ldP) {
  if (dst >= 0)
    S[(long long)a * ldS + dst] = v;
  else
    P[(long long)a * ldP + (-1 - dst)] = v;
}

}  // namespace

// lanes along runs: block (256 runs, SW_AE entries)
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) k_sw_sums(const T *__restrict__ src, long long rs, long long cs,
                                                 const int *__restrict__ cols, int Ms, int icpt,
                                                 const double *__restrict__ u, const int *__restrict__ rowof,
                                                 const int *__restrict__ rptr, const int *__restrict__ rdst, int NR,
                                                 double *__restrict__ S, long long ldS, double *__restrict__ P,
                                                 long long ldP) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= NR) return;
  const int a0 = (int)blockIdx.y * SW_AE;
  const long long k0 = rptr[j], k1 = rptr[j + 1];
  const int dst = rdst[j];
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < SW_AE; q++) {
      const int a = a0 + q;
      if (a >= Ms) break;
      double acc = 0.0;
      if (icpt && a == 0) {
        for (long long k = k0; k < k1; k++) acc = fma(u ? u[k] : 1.0, 1.0, acc);
      } else {
        acc = sw_run_vec<T>(src + (long long)cols[a - icpt] * cs, u, k0, k1);
      }
      sw_put(acc, dst, a, S, ldS, P, ldP);
    }
  } else {
    const T *cp[SW_AE];
    int kind[SW_AE];  // 0: no entry, 1: the constant, 2: a column
    double acc[SW_AE];
#pragma unroll
    for (int q = 0; q < SW_AE; q++) {
      const int a = a0 + q;
      acc[q] = 0.0;
      cp[q] = src;
      kind[q] = a >= Ms ? 0 : ((icpt && a == 0) ? 1 : 2);
      if (kind[q] == 2) cp[q] = src + (long long)cols[a - icpt] * cs;
    }
    for (long long k = k0; k < k1; k++) {
      const long long i = rowof ? (long long)rowof[k] : k;
      const double ui = u ? u[i] : 1.0;
      double x[SW_AE];
#pragma unroll
      for (int q = 0; q < SW_AE; q++) x[q] = kind[q] == 2 ? (double)cp[q][i * rs] : 1.0;
#pragma unroll
      for (int q = 0; q < SW_AE; q++) acc[q] = fma(ui, x[q], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < SW_AE; q++)
      if (kind[q]) sw_put(acc[q], dst, a0 + q, S, ldS, P, ldP);
  }
}

// row-contiguous source: block (16 runs, 16 entries), the 16 lanes of a DPP row read 16 support entries of one row
template <typename T>
__global__ void __launch_bounds__(256) k_sw_sums_gather(const T *__restrict__ src, long long rs,
                                                        const int *__restrict__ cols, int Ms, int icpt,
                                                        const double *__restrict__ u, const int *__restrict__ rowof,
                                                        const int *__restrict__ rptr, const int *__restrict__ rdst,
                                                        int NR, double *__restrict__ S, long long ldS,
                                                        double *__restrict__ P, long long ldP) {
  const long long j = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int a = (int)blockIdx.y * 16 + (threadIdx.x & 15);
  if (j >= NR || a >= Ms) return;
  const bool one = icpt && a == 0;
  const long long col = one ? 0 : (long long)cols[a - icpt];
  const long long k0 = rptr[j], k1 = rptr[j + 1];
  double acc = 0.0;
  for (long long k = k0; k < k1; k++) {
    const long long i = rowof ? (long long)rowof[k] : k;
    const double x = one ? 1.0 : (double)src[i * rs + col];
    acc = fma(u ? u[i] : 1.0, x, acc);
  }
  sw_put(acc, rdst[j], a, S, ldS, P, ldP);
}

// the partials of a cluster of several runs, added in run order: block (long cluster, 256 entries)
__global__ void __launch_bounds__(256) k_sw_fold(const double *__restrict__ P, long long ldP,
                                                 const int *__restrict__ lptr, const int *__restrict__ lgrp, int Ms,
                                                 double *__restrict__ S, long long ldS) {
  const int l = (int)blockIdx.x, a = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (a >= Ms) return;
  const double *p = P + (long long)a * ldP;
  const int k1 = lptr[l + 1];
  int k = lptr[l];
  double acc = p[k];
  for (k++; k < k1; k++) acc += p[k];
  S[(long long)a * ldS + lgrp[l]] = acc;
}

// u and u^2 from the score weight g and the leverage h (null for HC0 / HC1)
__global__ void __launch_bounds__(256) k_sw_u(const double *__restrict__ g, const double *__restrict__ h, int kind,
                                              long long n, double *__restrict__ u, double *__restrict__ u2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double v = g[i];
  if (kind == SANDWICH_HC2) v = v / sqrt(1.0 - h[i]);
  if (kind == SANDWICH_HC3) v = v / (1.0 - h[i]);
  u[i] = v;
  u2[i] = v * v;
}

__global__ void __launch_bounds__(256) k_sw_fill(double *__restrict__ o, long long n, double v) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) o[i] = v;
}

// *out = sum_g s[g]^2: thread t takes g = t, t + 256, ... in that order, then the 256 sums through a fixed tree
__global__ void __launch_bounds__(256) k_sw_sq(const double *__restrict__ s, long long G, double *__restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (long long g = t; g < G; g += 256) acc = fma(s[g], s[g], acc);
  red[t] = acc;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) *out = red[0];
}

// B and the sum vector from the sweep over S: T (Ms x Ms, row 0 / column 0 = the sum vector, the rest B's entries),
// sc (Ms: sum_g S(g, 0), then B(0, a)), b00
__global__ void __launch_bounds__(256) k_sw_fix(const double *__restrict__ T, const double *__restrict__ sc,
                                                const double *__restrict__ b00, int Ms, double *__restrict__ B,
                                                long long ld, double *__restrict__ sums) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)Ms * Ms) return;
  const int a = (int)(e / Ms), b = (int)(e % Ms);
  double v;
  if (a == 0 && b == 0)
    v = *b00;
  else if (a == 0 || b == 0)
    v = sc[a + b];
  else
    v = T[(long long)a * Ms + b];
  B[(long long)a * ld + b] = v;
  if (b == 0) sums[a] = a == 0 ? sc[0] : T[(long long)a * Ms];
}

int sandwich_run_rows() { return SW_RUN; }

// additions behind S(g, a) for a cluster of r rows: the run's FMA chain, then its partials in run order
int sandwich_sum_depth(long long r) {
  if (r < 1) return 0;
  return (int)std::min<long long>(r, SW_RUN) + (int)((r + SW_RUN - 1) / SW_RUN) - 1;
}

// additions behind B(0, 0) = sum_g S(g, 0)^2
int sandwich_sq_depth(long long G) { return (int)((G + 255) / 256) + 8; }

// leading dimension of S (and of P) for G rows: its columns stay 16-byte aligned
long long sandwich_ld(long long G) { return (std::max<long long>(G, 1) + 1) / 2 * 2; }

// rows of P that are always enough for n rows in G clusters the longest of which has max_rows rows
long long sandwich_partial_rows(long long n, long long G, long long max_rows) {
  if (max_rows <= SW_RUN) return 0;
  return n / SW_RUN + std::min<long long>(G, n / (SW_RUN + 1));
}

template <typename T>
static hipError_t sw_launch_sums(const T *src, long long rs, long long cs, const int *cols, int Ms, int icpt,
                                 const double *u, const int *rowof, const int *rptr, const int *rdst, int NR, double *S,
                                 long long ldS, double *P, long long ldP, hipStream_t st) {
  if (cs == 1 && rs != 1 && Ms > icpt) {
    const dim3 grid((unsigned)((NR + 15) / 16), (unsigned)((Ms + 15) / 16));
    hipLaunchKernelGGL((k_sw_sums_gather<T>), grid, dim3(256), 0, st, src, rs, cols, Ms, icpt, u, rowof, rptr, rdst, NR, S,
                       ldS, P, ldP);
  } else {
    const long long per16 = 16 / (long long)sizeof(T);
    const bool vec = !rowof && rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
    const dim3 grid((unsigned)((NR + 255) / 256), (unsigned)((Ms + SW_AE - 1) / SW_AE));
    if (vec)
      hipLaunchKernelGGL((k_sw_sums<T, true>), grid, dim3(256), 0, st, src, rs, cs, cols, Ms, icpt, u, rowof, rptr, rdst,
                         NR, S, ldS, P, ldP);
    else
      hipLaunchKernelGGL((k_sw_sums<T, false>), grid, dim3(256), 0, st, src, rs, cs, cols, Ms, icpt, u, rowof, rptr,
                         rdst, NR, S, ldS, P, ldP);
  }
  LAUNCH_CHECK();
  return hipSuccess;
}

// S(g, a) for G clusters: rowof (n ints or null = identity), rptr (NR + 1), rdst (NR), lptr (NL + 1) / lgrp (NL) the
// partial rows and the cluster of every cluster of several runs; S: ldS * Ms doubles, P: ldP * Ms doubles (NL > 0).
hipError_t launch_sandwich_sums(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                                int icpt, const double *u, const int *rowof, const int *rptr, const int *rdst, int NR,
                                const int *lptr, const int *lgrp, int NL, double *S, long long ldS, double *P,
                                long long ldP, hipStream_t st) {
  const int Ms = m + (icpt ? 1 : 0);
  if (!src || !rptr || !rdst || !S || n < 1 || n > 0x7fffffffLL || m < 0 || Ms < 1 || Ms > INFO_M_MAX ||
      (m > 0 && !cols) || rs < 0 || cs < 0 || NR < 1 || NR > n || ldS < 1 || NL < 0 ||
      (NL > 0 && (!lptr || !lgrp || !P || ldP < 1)))
    return hipErrorInvalidValue;
  hipError_t e = f32 ? sw_launch_sums(static_cast<const float *>(src), rs, cs, cols, Ms, icpt ? 1 : 0, u, rowof, rptr,
                                      rdst, NR, S, ldS, P, ldP, st)
                     : sw_launch_sums(static_cast<const double *>(src), rs, cs, cols, Ms, icpt ? 1 : 0, u, rowof, rptr,
                                      rdst, NR, S, ldS, P, ldP, st);
  if (e != hipSuccess) return e;
  if (NL > 0) {
    hipLaunchKernelGGL(k_sw_fold, dim3((unsigned)NL, (unsigned)((Ms + 255) / 256)), dim3(256), 0, st, P, ldP, lptr, lgrp,
                       Ms, S, ldS);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

// u (n) and u2 (n) from g and, for HC2 / HC3, h
hipError_t launch_sandwich_u(const double *g, const double *h, int kind, long long n, double *u, double *u2,
                             hipStream_t st) {
  if (!g || !u || !u2 || n < 1 || kind < SANDWICH_HC0 || kind > SANDWICH_HC3 || (kind >= SANDWICH_HC2 && !h))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sw_u, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, h, kind, n, u, u2);
  LAUNCH_CHECK();
  return hipSuccess;
}

// doubles of work launch_sandwich_gram needs: ones, the sweep's partials, its (Ms x Ms + Ms) result and B(0, 0)
long long sandwich_gram_workspace(long long G, int Ms) {
  const long long Gv = (G + 1) / 2 * 2;
  return Gv + info_gram_workspace(G, Ms - 1) + ((long long)Ms * Ms + Ms + 2);
}

// o[i] = x(i, cols[0]) as a double (a dense source's first support column as the sweep's score weight)
template <typename T>
__global__ void __launch_bounds__(256) k_sw_column(const T *__restrict__ src, long long rs, long long cs,
                                                   const int *__restrict__ cols, long long n, double *__restrict__ o) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) o[i] = (double)src[i * rs + (long long)cols[0] * cs];
}

hipError_t launch_sandwich_column(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                  double *out, hipStream_t st) {
  if (!src || !cols || !out || n < 1 || rs < 0 || cs < 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (f32)
    hipLaunchKernelGGL((k_sw_column<float>), grid, dim3(256), 0, st, static_cast<const float *>(src), rs, cs, cols, n, out);
  else
    hipLaunchKernelGGL((k_sw_column<double>), grid, dim3(256), 0, st, static_cast<const double *>(src), rs, cs, cols, n,
                       out);
  LAUNCH_CHECK();
  return hipSuccess;
}

// B = sum_g y_g y_g^T (Ms x Ms, leading dimension ld) and the sum vector (Ms) for the G rows y_g = (gw[g], src(g,
// cols1[0]), ..., src(g, cols1[Ms - 2])): src is S itself (f32 = 0, rs = 1, cs = ldS, cols1 = 1 .. Ms - 1, gw = S(:, 0)) or
// a dense source read in place (cols1 = its support without the first column, gw = that column as G doubles)
hipError_t launch_sandwich_gram(const void *src, int f32, long long rs, long long cs, long long G, int Ms,
                                const int *cols1, const double *gw, double *work, double *B, long long ld, double *sums,
                                hipStream_t st) {
  if (!src || !gw || !work || !B || !sums || G < 1 || Ms < 1 || Ms > INFO_M_MAX || (Ms > 1 && !cols1) || rs < 0 ||
      cs < 0 || ld < Ms)
    return hipErrorInvalidValue;
  const long long Gv = (G + 1) / 2 * 2;
  double *ones = work, *part = work + Gv, *T = part + info_gram_workspace(G, Ms - 1), *sc = T + (long long)Ms * Ms,
         *b00 = sc + Ms;
  hipLaunchKernelGGL(k_sw_fill, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, ones, G, 1.0);
  LAUNCH_CHECK();
  hipError_t e = launch_info_gram(src, f32, rs, cs, G, cols1, Ms - 1, ones, gw, part, T, (long long)Ms, sc, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sw_sq, dim3(1), dim3(256), 0, st, gw, G, b00);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sw_fix, dim3((unsigned)(((long long)Ms * Ms + 255) / 256)), dim3(256), 0, st, T, sc, b00, Ms, B, ld,
                     sums);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
