// bessx_k_coxband.hip -- standard errors and pointwise confidence bands of the cumulative hazard and survival curves of ONE
// Cox model on a caller's DEVICE matrix (include/bessx.h section 2s; Tsiatis 1981, what survival::survfit gives for a
// Breslow baseline).  Positions, r(k), e, wd, S0, the risk-set means u and the accumulated means A_l = sum_{p <= l} dh_p u_p
// are those of bessx_k_coxinfo.hip / bessx_k_coxdiag.hip, H is the hazard scan of bessx_k_coxsurv.hip: all formed by those
// units' launchers as they are.  For a grid time tau with K(tau) the positions of time <= tau:
//     cumhaz(tau) = sum_K wd_k / S0_k      var0(tau) = sum_K wd_k / S0_k^2      drift(tau) = sum_K (wd_k / S0_k) u_k
//     V(tau | x)  = var0(tau) + sum_j (p_tau[j] - cumhaz(tau) t_j)^2,   t = R z,  p_tau = R drift(tau),  z = x[cols]
// with inverse(info) = R^T R, R lower triangular.  The sum of squares is formed DIRECTLY: its expansion |p|^2 - 2 H p.t +
// H^2 |t|^2 cancels for columns that are not centred (p_tau is about H R xbar there).  This unit adds:
//   k_cbd_dh2       var0's increment per position, k_cxd_dh with S0 squared: wd_p / S0(p)^2 under "order"; under "breslow"
//                   the thread of a tie group's first position adds wd_k / S0(p)^2 over the group in position order, every
//                   other position gets 0.  Its forward scan is launch_cox_prefix_scan (the k_cxs_scan_* kernels).
//   k_cbd_gather    (tau, c) -> the three prefix arrays at idx[tau], the end of the last event-carrying tie group with time
//                   <= tau, found by the host (-1: no event up to tau, exact zeros): c = 0 cumhaz, 1 var0, 2 + j drift_j.
//                   Those are the positions the baseline of bessx_k_coxsurv.hip reads: the same bits under "breslow".
//   k_cbd_band      t = Z R^T in 16 x 16 tiles on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), operand layout, packing
//                   (cox_diag_pack, tri) and both access shapes of k_diag_lev without its intercept entry: 16-byte loads
//                   (the wave owns 16 E rows, E = 2 fp64 / 4 fp32, slot c of row tile e is row c * E + e) or element
//                   loads at any strides (16 rows, slot c is row c).  Only the k-steps ks < 4 (J + 1) of tile J are issued.
//                   blockIdx.y walks chunks of CBD_TS / E grid times (16 / 8 / 4 for E = 1 / 2 / 4: the chunk is sized so
//                   that the accumulators of one chunk, 4 E doubles per time, stay in registers); a chunk recomputes t
//                   from the operand, which a column-contiguous tile serves from cache.  As the tiles of a run complete,
//                   every lane adds d^2, d = fma(-cumhaz_tau, t, p_tau[16 J + c]), per (row slot, time), tiles in
//                   ascending order; at the end the 16 lanes of a DPP row are added by pr_group_sum<16>, var0 is added,
//                   and lane c of the row writes register c & 3's row for the times = c >> 2 (mod 4).
//   k_cbd_band0     m = 0: V = var0, one thread per (row, time); the matrix-core kernel is not launched.
// Addition depth of the sum of squares: ceil(m / 16) + 4, then one addition of var0.  Entries >= m of z and rows >= n enter
// as exact zeros and are not read; the padding of p_tau is zeros.  No LDS, no barriers, no n x m or n x T intermediate, no
// floating-point atomics: a row's results depend on that row's values, its e and the T-sized inputs alone.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CBD_T = 256;
constexpr int CBD_TS = 16;                                // time slots x row tiles of one chunk: 4 * CBD_TS accumulators
constexpr int CBD_ACC = 8, CBD_KU = 4;                    // 16-byte loads: output tiles x row tiles per run, k-steps in flight
constexpr int CBD_ACC_EL = 8, CBD_KU_EL = 2;              // element loads

// what the epilogue writes: slab s of out holds element (i, j) at out[s * ss + i * rs + j * cs]; a negative slab is one
// nobody asked for (order: estimate, se, lower, upper)
struct CbdOut {
  double *out;
  long long ss, rs, cs;
  int slab[4];
  int kind, conf;  // BESSX_SURV_*, BESSX_BAND_*
  double zc;
};

// (a NaN stays a NaN: comparisons, not fmax / fmin)
__device__ __forceinline__ double cbd_floor0(double v) { return v < 0.0 ? 0.0 : v; }
__device__ __forceinline__ double cbd_ceil1(double v) { return v > 1.0 ? 1.0 : v; }

// the four numbers of (row i, time j) from H = cumhaz_j, V and e = e_i.  estimate is cxs_value's expression.
__device__ __forceinline__ void cbd_emit(double H, double V, double e, const CbdOut &o, long long i, long long j) {
  const double Lam = H * e;
  double est, se, lo, hi;
  if (H == 0.0) {  // before the first event: var0 and drift are exact zeros, every bound is the estimate (no 0 / 0)
    est = o.kind ? Lam : exp(-Lam);
    se = Lam;
    lo = hi = est;
  } else {
    const double sq = sqrt(V), seL = e * sq, w = o.zc * seL;
    if (o.kind) {
      est = Lam;
      se = seL;
      if (o.conf == 0) {
        lo = cbd_floor0(Lam - w);
        hi = Lam + w;
      } else {
        const double r = (o.zc * sq) / H;
        lo = Lam * exp(-r);
        hi = Lam * exp(r);
      }
    } else {
      est = exp(-Lam);
      se = est * seL;
      if (o.conf == 0) {
        const double ws = o.zc * se;
        lo = cbd_floor0(est - ws);
        hi = cbd_ceil1(est + ws);
      } else if (o.conf == 1) {
        lo = exp(-(Lam + w));
        hi = exp(-cbd_floor0(Lam - w));
      } else {
        const double r = (o.zc * sq) / H;
        lo = exp(-(Lam * exp(r)));
        hi = exp(-(Lam * exp(-r)));
      }
    }
  }
  double *p = o.out + i * o.rs + j * o.cs;
  if (o.slab[0] >= 0) p[o.slab[0] * o.ss] = est;
  if (o.slab[1] >= 0) p[o.slab[1] * o.ss] = se;
  if (o.slab[2] >= 0) p[o.slab[2] * o.ss] = lo;
  if (o.slab[3] >= 0) p[o.slab[3] * o.ss] = hi;
}

}  // namespace

__global__ void __launch_bounds__(CBD_T) k_cbd_dh2(const double *__restrict__ wd, const double *__restrict__ S0,
                                                   const int *__restrict__ first, const int *__restrict__ lastk,
                                                   long long n, double *__restrict__ dv) {
  const long long p = (long long)blockIdx.x * CBD_T + threadIdx.x;
  if (p >= n) return;
  if (!lastk) {
    dv[p] = wd[p] / (S0[p] * S0[p]);
    return;
  }
  double s = 0.0;
  if (first[p] == p) {
    const double S2 = S0[p] * S0[p];
    const long long end = lastk[p];
    for (long long k = p; k <= end; k++) s += wd[k] / S2;
  }
  dv[p] = s;
}

// out[tau * (m + 2) + c]; A may be null when m == 0 or no position is an event (drift is zeros then)
__global__ void __launch_bounds__(CBD_T) k_cbd_gather(const double *__restrict__ H, const double *__restrict__ V0,
                                                      const double *__restrict__ A, long long ldA,
                                                      const int *__restrict__ idx, int Tn, int m,
                                                      double *__restrict__ out) {
  const long long g = (long long)blockIdx.x * CBD_T + threadIdx.x, W = (long long)m + 2;
  if (g >= (long long)Tn * W) return;
  const int c = (int)(g % W);
  const long long k = idx[g / W];
  double v = 0.0;
  if (k >= 0) v = c == 0 ? H[k] : (c == 1 ? V0[k] : (A ? A[(long long)(c - 2) * ldA + k] : 0.0));
  out[g] = v;
}

// the lane's E values of entry `a` of z (a >= m: nothing) for its rows i0 (+ e, or + 16 e for element loads); rows >= n are
// exact zeros and are not read
template <typename T, bool VEC, int E>
__device__ __forceinline__ void cbd_entry(const T *__restrict__ src, long long rs, long long cs,
                                          const int *__restrict__ cols, int m, int a, long long i0, long long n,
                                          double *xa) {
#pragma unroll
  for (int e = 0; e < E; e++) xa[e] = 0.0;
  if (a >= m) return;
  const T *cp = src + (long long)cols[a] * cs;
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

// one wave per workgroup.  pk: cox_diag_pack(R, tri); P: Tn rows of ldP = 16 ceil(m / 16) doubles, p_tau with zeros behind
// entry m; hz, v0: Tn doubles; ex: n doubles in row order
template <typename T, bool VEC>
__global__ void __launch_bounds__(64) k_cbd_band(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                 const int *__restrict__ cols, int m, const double *__restrict__ pk,
                                                 const double *__restrict__ P, long long ldP,
                                                 const double *__restrict__ hz, const double *__restrict__ v0,
                                                 const double *__restrict__ ex, int Tn, const CbdOut o) {
  constexpr int E = VEC ? PrVec<T>::N : 1, JC = VEC ? CBD_ACC / E : CBD_ACC_EL, KU = VEC ? CBD_KU : CBD_KU_EL;
  constexpr int TC = CBD_TS / E;
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const long long rb = (long long)blockIdx.x * (16 * E);
  const long long i0 = VEC ? rb + (long long)c * E : rb + c;  // the lane's first row as an A operand
  const int j0 = (int)blockIdx.y * TC, nt = min(TC, Tn - j0);
  const int TI = (m + 15) / 16;
  double hc[TC];
  d4 s[E][TC];  // (x, y, z, w: registers 0 .. 3 of the tile, row slots q, q + 4, q + 8, q + 12)
#pragma unroll
  for (int t = 0; t < TC; t++) {
    hc[t] = t < nt ? hz[j0 + t] : 0.0;
#pragma unroll
    for (int e = 0; e < E; e++) s[e][t] = d4{0.0, 0.0, 0.0, 0.0};
  }
  for (int J0 = 0; J0 < TI; J0 += JC) {
    const int nJ = min(JC, TI - J0);
    d4 acc[E][JC];
#pragma unroll
    for (int e = 0; e < E; e++)
#pragma unroll
      for (int jj = 0; jj < JC; jj++) acc[e][jj] = d4{0.0, 0.0, 0.0, 0.0};
    const int ksteps = 4 * (J0 + nJ);  // (a multiple of KU, as is every tile's 4 (J + 1))
    for (int k0 = 0; k0 < ksteps; k0 += KU) {
      double xa[KU][E], b[KU][JC];
#pragma unroll
      for (int u = 0; u < KU; u++) cbd_entry<T, VEC, E>(src, rs, cs, cols, m, 4 * (k0 + u) + q, i0, n, xa[u]);
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
    // register r of lane (c, q) is row slot q + 4 r, column c of tile J: t_{16 J + c} of that row
#pragma unroll
    for (int jj = 0; jj < JC; jj++) {
      if (jj < nJ) {
        const double *pc = P + (long long)j0 * ldP + 16 * (J0 + jj) + c;
#pragma unroll
        for (int t = 0; t < TC; t++) {
          const double pv = t < nt ? pc[(long long)t * ldP] : 0.0;
#pragma unroll
          for (int e = 0; e < E; e++) {
            const double d0 = fma(-hc[t], acc[e][jj].x, pv), d1 = fma(-hc[t], acc[e][jj].y, pv);
            const double d2_ = fma(-hc[t], acc[e][jj].z, pv), d3 = fma(-hc[t], acc[e][jj].w, pv);
            s[e][t].x = fma(d0, d0, s[e][t].x);
            s[e][t].y = fma(d1, d1, s[e][t].y);
            s[e][t].z = fma(d2_, d2_, s[e][t].z);
            s[e][t].w = fma(d3, d3, s[e][t].w);
          }
        }
      }
    }
  }
  // the 16 lanes c of a DPP row hold one row's columns
#pragma unroll
  for (int e = 0; e < E; e++)
#pragma unroll
    for (int t = 0; t < TC; t++) {
      s[e][t].x = pr_group_sum<16>(s[e][t].x);
      s[e][t].y = pr_group_sum<16>(s[e][t].y);
      s[e][t].z = pr_group_sum<16>(s[e][t].z);
      s[e][t].w = pr_group_sum<16>(s[e][t].w);
    }
  // lane c of a DPP row writes the row of register c & 3 at the chunk's times = c >> 2 (mod 4)
  const int r = c & 3, slot = q + 4 * r;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const long long i = VEC ? rb + (long long)slot * E + e : rb + 16 * e + slot;
    const double ei = i < n ? ex[i] : 0.0;
#pragma unroll
    for (int u = 0; u < TC / 4; u++) {
      // (selects between registers: no indexing by a lane's value)
      double ss = 0.0, h = 0.0;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const int t = 4 * u + w;
        const double sr = r == 0 ? s[e][t].x : (r == 1 ? s[e][t].y : (r == 2 ? s[e][t].z : s[e][t].w));
        if ((c >> 2) == w) ss = sr, h = hc[t];
      }
      const int t = 4 * u + (c >> 2);
      if (i < n && t < nt) cbd_emit(h, ss + v0[j0 + t], ei, o, i, j0 + t);
    }
  }
}

__global__ void __launch_bounds__(CBD_T) k_cbd_band0(const double *__restrict__ hz, const double *__restrict__ v0,
                                                     const double *__restrict__ ex, long long n, int Tn, const CbdOut o) {
  const long long g = (long long)blockIdx.x * CBD_T + threadIdx.x;
  if (g >= n * Tn) return;
  const long long i = g / Tn, j = g % Tn;
  cbd_emit(hz[j], 0.0 + v0[j], ex[i], o, i, j);
}

// grid times per chunk of k_cbd_band for a source of this shape (tests and the workspace report it)
int cox_band_time_chunk(int f32, long long rs, long long cs, const void *src) {
  const long long per16 = f32 ? 4 : 2;
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  return vec ? CBD_TS / (int)per16 : CBD_TS;
}

// additions behind one V: the tiles' squares in tile order, 4 levels of the DPP tree, var0
int cox_band_sum_depth(int m) { return (m + 15) / 16 + 4 + 1; }

// dv[p] = var0's increment at position p (wd, S0, first = r(k), lastk (null: ties "order") as in launch_cox_diag_accum)
hipError_t launch_cox_band_dh2(const double *wd, const double *S0, const int *first, const int *lastk, long long n,
                               double *dv, hipStream_t st) {
  if (!wd || !S0 || !first || !dv || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cbd_dh2, dim3((unsigned)((n + CBD_T - 1) / CBD_T)), dim3(CBD_T), 0, st, wd, S0, first, lastk, n, dv);
  LAUNCH_CHECK();
  return hipSuccess;
}

// out[tau * (m + 2) + (0, 1, 2 + j)] = (H, V0, A(j, .)) at position idx[tau], zeros where idx[tau] < 0.  A null: drift zeros.
hipError_t launch_cox_band_gather(const double *H, const double *V0, const double *A, long long ldA, const int *idx,
                                  int Tn, int m, double *out, hipStream_t st) {
  if (!H || !V0 || !idx || !out || Tn < 1 || m < 0 || (A && ldA < 1)) return hipErrorInvalidValue;
  const long long cnt = (long long)Tn * (m + 2);
  hipLaunchKernelGGL(k_cbd_gather, dim3((unsigned)((cnt + CBD_T - 1) / CBD_T)), dim3(CBD_T), 0, st, H, V0, A, ldA, idx, Tn,
                     m, out);
  LAUNCH_CHECK();
  return hipSuccess;
}

template <typename T>
static hipError_t cbd_launch(const T *src, long long rs, long long cs, long long n, const int *cols, int m,
                             const double *pk, const double *P, long long ldP, const double *hz, const double *v0,
                             const double *ex, int Tn, const CbdOut &o, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const long long rows_per_block = vec ? 16LL * PrVec<T>::N : 16LL;
  const int tc = vec ? CBD_TS / PrVec<T>::N : CBD_TS;
  const unsigned chunks = (unsigned)((Tn + tc - 1) / tc);
  if (chunks > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block), chunks);
  if (vec)
    hipLaunchKernelGGL((k_cbd_band<T, true>), grid, dim3(64), 0, st, src, rs, cs, n, cols, m, pk, P, ldP, hz, v0, ex, Tn, o);
  else
    hipLaunchKernelGGL((k_cbd_band<T, false>), grid, dim3(64), 0, st, src, rs, cs, n, cols, m, pk, P, ldP, hz, v0, ex, Tn, o);
  LAUNCH_CHECK();
  return hipSuccess;
}

// the bands of n rows at Tn times: pk = cox_diag_pack_doubles(m, 1) doubles from cox_diag_pack (m > 0), P / ldP the rows
// p_tau (ldP = 16 ceil(m / 16), zeros behind entry m), hz / v0 the Tn values of cumhaz / var0, ex the n values of
// launch_cox_surv_ex.  slab[w] (w = estimate, se, lower, upper): which slab of out takes it, negative = not wanted; element
// (i, j) of slab s at out[s * oss + i * ors + j * ocs].  kind: BESSX_SURV_*; conf: 0 plain, 1 log, 2 log-log.  Device memory.
hipError_t launch_cox_band(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                           const double *pk, const double *P, long long ldP, const double *hz, const double *v0,
                           const double *ex, int Tn, int kind, int conf, double zc, const int *slab, double *out,
                           long long oss, long long ors, long long ocs, hipStream_t st) {
  if (!hz || !v0 || !ex || !slab || !out || n < 1 || n > 0x7fffffffLL || Tn < 1 || m < 0 || m + 1 > INFO_M_MAX ||
      (kind != 0 && kind != 1) || conf < 0 || conf > 2 || oss < 0 || ors < 0 || ocs < 0 ||
      (m > 0 && (!src || !cols || !pk || !P || ldP < 16LL * ((m + 15) / 16) || rs < 0 || cs < 0)))
    return hipErrorInvalidValue;
  const CbdOut o{out, oss, ors, ocs, {slab[0], slab[1], slab[2], slab[3]}, kind, conf, zc};
  if (m == 0) {
    const long long cnt = n * Tn;
    if ((cnt + CBD_T - 1) / CBD_T > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cbd_band0, dim3((unsigned)((cnt + CBD_T - 1) / CBD_T)), dim3(CBD_T), 0, st, hz, v0, ex, n, Tn, o);
    LAUNCH_CHECK();
    return hipSuccess;
  }
  return f32 ? cbd_launch(static_cast<const float *>(src), rs, cs, n, cols, m, pk, P, ldP, hz, v0, ex, Tn, o, st)
             : cbd_launch(static_cast<const double *>(src), rs, cs, n, cols, m, pk, P, ldP, hz, v0, ex, Tn, o, st);
}

}  // namespace bessx
