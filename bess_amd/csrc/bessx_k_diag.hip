// bessx_k_diag.hip -- per-row diagnostics of ONE model (identity, logistic or Poisson link) on a caller's DEVICE
// matrix, read where it lies, the support's columns only (include/bessx.h section 2i):
//     leverage h_i = v_i sum_j t_ij^2,   t_ij = sum_{k <= j} R_jk z_ik,   z_i = (1, X(i, cols[0]), ...),  M = m + 1
// with R lower triangular, inverse(information) = R^T R, and the response, Pearson and deviance residuals, their
// standardised forms and Cook's distance.  Two steps:
//   1. eta pass: the loops of bessx_k_xb.hpp with the store epilogue DiagStore, which writes v_i (when a kind needs the
//      leverage) and the response, Pearson and deviance residuals of row i.  It is ALWAYS k_xb_rows (threads along
//      rows, 16-byte loads where the source allows, element loads at any strides otherwise -- the same arithmetic in
//      the same order), never k_xb_gather: the two add the support's products in different orders, and a row's
//      diagnostics are the same bits under every layout of X.  For a row-contiguous source with a scattered support
//      every element is a cache line of its own whichever kernel reads it.
//   2. k_diag_lev: T = Z R^T in 16 x 16 tiles on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  A = Z: lane (c = lane
//      & 15, q = lane >> 4) supplies A[slot c][k = q], entry 4 ks + q of z for k-step ks; B[k = q][c] = R[16 J + c][4 ks
//      + q] for output tile J, packed on the host in exactly that order (diag_pack_factor: one (tile, k-step) is 64
//      consecutive doubles, zeros above the diagonal and past M), so a B load is one 512-byte read.  Only the k-steps
//      ks < 4 (J + 1), those at or below the tile's diagonal, are issued.  One wave per workgroup (no LDS, no barrier).
//      Two access shapes, the same arithmetic in the same order:
//        16-byte loads (column-contiguous source, aligned base and column stride): the wave owns 16 E rows, E = 2 (fp64)
//          or 4 (fp32); slot c of the e-th of E row tiles is row c * E + e, so one load feeds E MFMAs that share one B
//          load.  Output tiles go in runs of DG_ACC / E; the wave re-reads its A operand per run (a column-contiguous
//          tile stays in cache).
//        element loads at any strides: the wave owns 16 rows, slot c is row c -- lanes along the rows of a
//          column-contiguous source; for a row-contiguous source the four lanes q of a slot read four neighbouring
//          support entries of one row, the gather of k_xb_gather turned to this operand.  There every element of a
//          scattered support is a cache line of its own and a re-read comes from memory again, so the run is
//          DG_ACC_EL = 16 tiles: up to M = 256 X is read exactly once.
//      Which row a slot means is free, the result lands on that row.  The wave keeps sum t^2 across runs: after a run
//      every lane adds the squares of its accumulators, tiles in ascending order, into s[e][reg] (row slot q + 4 reg of
//      row tile e);
//      at the end the 16 lanes of a DPP row, which hold the 16 columns of one row, are added by pr_group_sum<16>.
//      Addition depth of sum t^2: ceil(M / 16) + 4 (diag_sum_depth).  The epilogue multiplies by v_i and writes h_i,
//      the standardised residuals and Cook's distance.
// Masking: the intercept entry is the constant 1 and is not read; rows >= n and entries >= M of z enter as exact zeros
// and are not read.  No LDS, no barriers, no n x M intermediate, no floating-point atomics; a row's results depend on
// that row's values, R, the dispersion and M alone.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

// 16-byte loads: E = 2 (fp64) or 4 (fp32) row tiles x DG_ACC / E output tiles per run, DG_KU k-steps of loads in flight.
// Element loads: one row tile x DG_ACC_EL output tiles per run -- for a row-contiguous source every re-read of the A
// operand is a cache line per element from memory again, so the run is as long as the registers allow (M <= 256: one
// run, X is read once) -- and DG_KU_EL k-steps in flight.  The run lengths do not depend on M, and no result depends
// on them: a tile's k-steps are issued in ascending order and the tiles' squares are added in ascending order.
constexpr int DG_ACC = 8, DG_KU = 4, DG_ACC_EL = 16, DG_KU_EL = 2;

__device__ __forceinline__ double dg_load(const void *p, int f32, long long off) {
  return f32 ? (double)static_cast<const float *>(p)[off] : static_cast<const double *>(p)[off];
}

// y log y with 0 log 0 = 0 (a NaN stays a NaN)
__device__ __forceinline__ double dg_xlogx(double y) { return y == 0.0 ? 0.0 : y * log(y); }

// the epilogue of the eta pass: what row i contributes besides its leverage.  A null pointer is a vector nobody needs.
struct DiagStore {
  static constexpr bool REDUCE = false, SKIPZ = false;
  EvalData d;
  int link;
  double *__restrict__ v;
  double *__restrict__ resp;
  double *__restrict__ pear;
  double *__restrict__ dev;
  __device__ __forceinline__ void store(double eta, long long i, int) const {
    const double y = dg_load(d.y, d.y_f32, i * d.yrs);
    const double w = d.w ? dg_load(d.w, d.w_f32, i * d.ws) : 1.0;
    double mu, V, dd;
    if (link == PREDICT_LOGISTIC) {
      // (t, s, p and V as in InfoStore of bessx_k_info.hip; f as in EvLoss of bessx_k_eval.hip)
      const double t = exp(-fabs(eta)), s = 1.0 + t;
      mu = (eta >= 0.0 ? 1.0 : t) / s;
      V = t / (s * s);
      const double f = ((eta > 0.0 ? eta : 0.0) + log1p(t)) - y * eta;
      dd = 2.0 * ((f + dg_xlogx(y)) + dg_xlogx(1.0 - y));
    } else if (link == PREDICT_POISSON) {
      mu = exp(eta);
      V = mu;
      const double f = mu - y * eta;
      dd = 2.0 * ((f + dg_xlogx(y)) - y);
    } else {
      mu = eta;
      V = 1.0;
      const double e = y - eta;
      dd = e * e;
    }
    const double r = y - mu;
    if (v) v[i] = w * V;
    if (resp) resp[i] = r;
    if (pear) pear[i] = (sqrt(w) * r) / sqrt(V);
    if (dev) {
      const double sg = r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0);
      dev[i] = sg * sqrt(w * (dd < 0.0 ? 0.0 : dd));
    }
  }
};

}  // namespace

// the lane's E values of entry `a` of z (0: the intercept's 1, a >= M: nothing) for its rows i0 (+ e, or + 16 e for
// element loads); rows >= n are exact zeros and are not read
template <typename T, bool VEC, int E>
__device__ __forceinline__ void dg_entry(const T *__restrict__ src, long long rs, long long cs,
                                         const int *__restrict__ cols, int M, int a, long long i0, long long n,
                                         double *xa) {
  if (a == 0) {
#pragma unroll
    for (int e = 0; e < E; e++) xa[e] = (VEC ? i0 + e : i0 + 16 * e) < n ? 1.0 : 0.0;
    return;
  }
#pragma unroll
  for (int e = 0; e < E; e++) xa[e] = 0.0;
  if (a >= M) return;
  const T *cp = src + (long long)cols[a - 1] * cs;
  if constexpr (VEC) {
    if (i0 + E <= n) {
      pr_unpack(*reinterpret_cast<const typename PrVec<T>::type *>(cp + i0), xa);
    } else {
#pragma unroll
      for (int e = 0; e < E; e++)
        if (i0 + e < n) xa[e] = (double)cp[(i0 + e) * rs];
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; e++)
      if (i0 + 16 * e < n) xa[e] = (double)cp[(i0 + 16 * e) * rs];
  }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(64) k_diag_lev(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                 const int *__restrict__ cols, int M, const double *__restrict__ pk,
                                                 const double *__restrict__ vw, const double *__restrict__ rp,
                                                 const double *__restrict__ rd, double phi, double phiM,
                                                 double *__restrict__ o_h, double *__restrict__ o_sp,
                                                 double *__restrict__ o_sd, double *__restrict__ o_ck) {
  constexpr int E = VEC ? PrVec<T>::N : 1, JC = VEC ? DG_ACC / E : DG_ACC_EL, KU = VEC ? DG_KU : DG_KU_EL;
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const long long rb = (long long)blockIdx.x * (16 * E);  // one wave per workgroup: no LDS, no barrier
  const long long i0 = VEC ? rb + (long long)c * E : rb + c;  // the lane's first row as an A operand
  const int TI = (M + 15) / 16;
  double s[E][4];
#pragma unroll
  for (int e = 0; e < E; e++)
#pragma unroll
    for (int r = 0; r < 4; r++) s[e][r] = 0.0;
  for (int J0 = 0; J0 < TI; J0 += JC) {
    const int nJ = min(JC, TI - J0);
    d4 acc[E][JC];
#pragma unroll
    for (int e = 0; e < E; e++)
#pragma unroll
      for (int jj = 0; jj < JC; jj++) acc[e][jj] = d4{0.0, 0.0, 0.0, 0.0};
    const int ksteps = 4 * (J0 + nJ);  // (a multiple of KU, as is every tile's 4 (J + 1))
    for (int k0 = 0; k0 < ksteps; k0 += KU) {
      // the loads of KU k-steps are issued before their matrix instructions: the kernel is bound by load latency
      double xa[KU][E], b[KU][JC];
#pragma unroll
      for (int u = 0; u < KU; u++) dg_entry<T, VEC, E>(src, rs, cs, cols, M, 4 * (k0 + u) + q, i0, n, xa[u]);
#pragma unroll
      for (int jj = 0; jj < JC; jj++) {
        const int J = J0 + jj;
        if (jj < nJ && k0 < 4 * (J + 1)) {  // (wave-uniform)
#pragma unroll
          for (int u = 0; u < KU; u++) b[u][jj] = pk[((long long)2 * J * (J + 1) + k0 + u) * 64 + lane];
        }
      }
#pragma unroll
      for (int jj = 0; jj < JC; jj++) {
        if (jj < nJ && k0 < 4 * (J0 + jj + 1)) {
#pragma unroll
          for (int u = 0; u < KU; u++)  // (a tile's k-steps in ascending order)
#pragma unroll
            for (int e = 0; e < E; e++)
              acc[e][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u][e], b[u][jj], acc[e][jj], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < JC; jj++) {
      if (jj < nJ) {
#pragma unroll
        for (int e = 0; e < E; e++) {
          s[e][0] = fma(acc[e][jj].x, acc[e][jj].x, s[e][0]);
          s[e][1] = fma(acc[e][jj].y, acc[e][jj].y, s[e][1]);
          s[e][2] = fma(acc[e][jj].z, acc[e][jj].z, s[e][2]);
          s[e][3] = fma(acc[e][jj].w, acc[e][jj].w, s[e][3]);
        }
      }
    }
  }
  // register r of lane (c, q) is row slot q + 4 r, column c of a tile: the 16 lanes c of a DPP row hold one row's columns
#pragma unroll
  for (int e = 0; e < E; e++) {
#pragma unroll
    for (int r = 0; r < 4; r++) s[e][r] = pr_group_sum<16>(s[e][r]);
  }
  if (c >= 4) return;  // lane c < 4 of a DPP row writes the rows of register c
#pragma unroll
  for (int e = 0; e < E; e++) {
    const double st2 = c == 0 ? s[e][0] : (c == 1 ? s[e][1] : (c == 2 ? s[e][2] : s[e][3]));
    const int slot = q + 4 * c;
    const long long i = VEC ? rb + (long long)slot * E + e : rb + 16 * e + slot;
    if (i >= n) continue;
    const double h = vw[i] * st2;
    if (o_h) o_h[i] = h;
    const double om = 1.0 - h;
    if (o_sp || o_sd) {
      const double den = sqrt(phi * om);
      if (o_sp) o_sp[i] = rp[i] / den;
      if (o_sd) o_sd[i] = rd[i] / den;
    }
    if (o_ck) {
      const double p = rp[i];
      o_ck[i] = ((p * p) * h) / (phiM * (om * om));
    }
  }
}

// additions behind one row's sum of t^2: its tiles' squares in tile order, then 4 levels of the DPP tree
int diag_sum_depth(int m) { return (m + 1 + 15) / 16 + 4; }

// doubles of the packed factor of an M x M lower-triangular matrix
long long diag_factor_doubles(int m) {
  const long long TI = (m + 1 + 15) / 16;
  return 2 * TI * (TI + 1) * 64;
}

// the factor in the order the lanes consume it (host memory): (tile J, k-step ks < 4 (J + 1)) holds R[16 J + c][4 ks + q]
// at lane 16 q + c.  Entries above the diagonal and past M are zeros; the strict upper triangle of R is not read.
void diag_pack_factor(const double *R, long long ld, int m, double *pk) {
  const int M = m + 1, TI = (M + 15) / 16;
  for (int J = 0; J < TI; J++)
    for (int ks = 0; ks < 4 * (J + 1); ks++) {
      double *o = pk + ((long long)2 * J * (J + 1) + ks) * 64;
      for (int lane = 0; lane < 64; lane++) {
        const int j = 16 * J + (lane & 15), k = 4 * ks + (lane >> 4);
        o[lane] = (j < M && k <= j) ? R[(long long)j * ld + k] : 0.0;
      }
    }
}

template <typename T>
static hipError_t diag_launch_eta(const T *src, long long rs, long long cs, long long n, const int *cols, int m,
                                  const double *B, const double *c, const DiagStore &epi, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const long long rows_per_block = 64LL * PrVec<T>::N;
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block), 1);
  if (vec)
    hipLaunchKernelGGL((k_xb_rows<T, 1, true, DiagStore>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, c, 1, epi);
  else
    hipLaunchKernelGGL((k_xb_rows<T, 1, false, DiagStore>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, c, 1, epi);
  LAUNCH_CHECK();
  return hipSuccess;
}

// step 1 alone: v, resp, pear, dev are n doubles of device memory each or null (src, cols, B, c as in launch_predict
// with R = 1)
hipError_t launch_diag_eta(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                           const double *B, const double *c, int link, const EvalData &d, double *v, double *resp,
                           double *pear, double *dev, hipStream_t st) {
  if (!src || !c || !d.y || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || rs < 0 || cs < 0 ||
      d.yrs < 0 || d.ws < 0 || link < PREDICT_IDENTITY || link > PREDICT_POISSON)
    return hipErrorInvalidValue;
  const DiagStore epi{d, link, v, resp, pear, dev};
  return f32 ? diag_launch_eta(static_cast<const float *>(src), rs, cs, n, cols, m, B, c, epi, st)
             : diag_launch_eta(static_cast<const double *>(src), rs, cs, n, cols, m, B, c, epi, st);
}

template <typename T>
static hipError_t diag_launch_lev(const T *src, long long rs, long long cs, long long n, const int *cols, int M,
                                  const double *pk, const double *vw, const double *rp, const double *rd, double phi,
                                  double *o_h, double *o_sp, double *o_sd, double *o_ck, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const long long rows_per_block = vec ? 16LL * PrVec<T>::N : 16LL;
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block));
  const double phiM = phi * (double)M;
  if (vec)
    hipLaunchKernelGGL((k_diag_lev<T, true>), grid, dim3(64), 0, st, src, rs, cs, n, cols, M, pk, vw, rp, rd, phi, phiM,
                       o_h, o_sp, o_sd, o_ck);
  else
    hipLaunchKernelGGL((k_diag_lev<T, false>), grid, dim3(64), 0, st, src, rs, cs, n, cols, M, pk, vw, rp, rd, phi,
                       phiM, o_h, o_sp, o_sd, o_ck);
  LAUNCH_CHECK();
  return hipSuccess;
}

// step 2 alone: pk = diag_factor_doubles(m) doubles from diag_pack_factor, vw the n working weights, rp / rd the Pearson
// and deviance residuals (needed by o_sp and o_ck / by o_sd), o_*: n doubles each or null.  Device memory.
hipError_t launch_diag_lev(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                           const double *pk, const double *vw, const double *rp, const double *rd, double phi,
                           double *o_h, double *o_sp, double *o_sd, double *o_ck, hipStream_t st) {
  if (!src || !pk || !vw || n < 1 || n > 0x7fffffffLL || m < 0 || m + 1 > INFO_M_MAX || (m > 0 && !cols) || rs < 0 ||
      cs < 0 || ((o_sp || o_ck) && !rp) || (o_sd && !rd))
    return hipErrorInvalidValue;
  return f32 ? diag_launch_lev(static_cast<const float *>(src), rs, cs, n, cols, m + 1, pk, vw, rp, rd, phi, o_h, o_sp,
                               o_sd, o_ck, st)
             : diag_launch_lev(static_cast<const double *>(src), rs, cs, n, cols, m + 1, pk, vw, rp, rd, phi, o_h, o_sp,
                               o_sd, o_ck, st);
}

}  // namespace bessx
