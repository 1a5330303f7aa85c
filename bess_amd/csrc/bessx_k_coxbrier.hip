// bessx_k_coxbrier.hip -- the IPCW Brier score of R Cox models at T times on a caller's DEVICE matrix: the fused
// reduction behind bessx_cox_brier_device.  With e(i, r) = exp(clamp(eta(i, r), +-30)), z = hg(r, j) * e(i, r),
//     term(i, j, r) = a_i exp(-z)^2             when time_i <= t_j      (the row has left the risk set)
//                   = b_j (-expm1(-z))^2        otherwise
//     BS(j, r)      = (1 / W) sum_i w_i term(i, j, r),
// a (n values) and b (T values) the inverse-probability-of-censoring weights, which the host forms.  No n x T element is
// ever stored.
//   predictor pass   the loops of bessx_k_xb.hpp with a store epilogue: e goes to an R x n array in ROW order (model r at
//                    e + r * n).  X is read once, the support's columns only.  (launch_cox_eval_eta's epilogue would
//                    also write eta, R x n doubles that nothing here reads, through a position map that is the identity.)
//   k_cxb_terms      grid (row slabs, models).  A workgroup owns a slab of CXB_ROWS = 1024 rows of ONE model: their e, time,
//                    w and w * a are read once into LDS (32 KiB), not once per time.  Its 256 threads form 256 / TJ row
//                    groups of TJ lanes, TJ the power of two that covers T (at most 256: the regrouping of k_cxs_curves, so
//                    T = 1 keeps every lane busy and T = 100 idles 28 of 128); a thread keeps hg, t and b of its time in
//                    registers, walks the rows of its group in ascending order (every LDS read is a broadcast within the
//                    group) and chunks of TJ times for T > 256.  Per element: one multiply for z, one compare, ONE
//                    transcendental (exp or expm1 -- lanes lie along the times, so for an ascending grid only the wave that
//                    holds a row's own time runs both sides of the branch), one square and one multiply-add into one of
//                    two sums, A = sum w a S^2 and Q = sum w q^2; b_j enters once per (slab, time): A + b_j Q.  The row
//                    groups' sums are added through LDS in ascending group order.
//   k_cxb_finish     bs(j, r) = (sum of the slabs' partials in ascending slab order) / W.
// fp64, no floating-point atomics, every sum in one fixed order; the grids depend on (n, T, R) alone: the same call gives
// the same bits.  Index arithmetic is in 64 bits.  Nothing is sized by n x T.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CXB_T = 256;      // threads per workgroup
constexpr int CXB_ROWS = 1024;  // rows per slab

struct CxbStore {
  static constexpr bool REDUCE = false, SKIPZ = true;
  long long n;
  double *__restrict__ ex;
  __device__ __forceinline__ void store(double v, long long i, int r) const {
    ex[(long long)r * n + i] = exp(clampv(v, 30.0));
  }
};

}  // namespace

// part[(slab * R + r) * T + j] = sum over the slab's rows of w_i term(i, j, r).  Thread t: time slot t & (TJ - 1), row
// group t >> tj_log2.
__global__ void __launch_bounds__(CXB_T) k_cxb_terms(const double *__restrict__ e, const double *__restrict__ time,
                                                     const double *__restrict__ w, const double *__restrict__ wa,
                                                     const double *__restrict__ hg, const double *__restrict__ tg,
                                                     const double *__restrict__ b, long long n, int T, int tj_log2,
                                                     double *__restrict__ part) {
  __shared__ double es[CXB_ROWS], ts[CXB_ROWS], ws[CXB_ROWS], as[CXB_ROWS];
  __shared__ double ra[CXB_T], rq[CXB_T];
  const int t = threadIdx.x, TJ = 1 << tj_log2, TR = CXB_T >> tj_log2, jt = t & (TJ - 1), rt = t >> tj_log2;
  const long long row0 = (long long)blockIdx.x * CXB_ROWS, r = blockIdx.y;
  const int rows = (int)(n - row0 < CXB_ROWS ? n - row0 : CXB_ROWS);
  const double *er = e + r * n + row0;
  for (int i = t; i < rows; i += CXB_T) {
    es[i] = er[i];
    ts[i] = time[row0 + i];
    ws[i] = w[row0 + i];
    as[i] = wa[row0 + i];
  }
  __syncthreads();
  const double *hr = hg + r * T;
  double *out = part + ((long long)blockIdx.x * gridDim.y + r) * T;
  for (long long j0 = 0; j0 < T; j0 += TJ) {  // (TR > 1 means TJ >= T: one trip, so the barriers below are uniform)
    const long long j = j0 + jt;
    const bool on = j < T;
    const double h = on ? hr[j] : 0.0, tj = on ? tg[j] : 0.0;
    double sa = 0.0, sq = 0.0;
    if (on)
      for (int i = rt; i < rows; i += TR) {
        const double nz = -(h * es[i]);
        if (ts[i] <= tj) {
          const double s = exp(nz);
          sa += as[i] * (s * s);
        } else {
          const double q = expm1(nz);  // (-q is 1 - S without the cancellation; only its square is used)
          sq += ws[i] * (q * q);
        }
      }
    if (TR > 1) {
      ra[t] = sa;
      rq[t] = sq;
      __syncthreads();
      if (rt == 0)
        for (int g = 1; g < TR; g++) {
          sa += ra[(g << tj_log2) + jt];
          sq += rq[(g << tj_log2) + jt];
        }
    }
    if (rt == 0 && on) out[j] = sa + b[j] * sq;
  }
}

// bs[j * R + r] = (sum_s part[s * R * T + r * T + j]) / W, the slabs in ascending order
__global__ void __launch_bounds__(CXB_T) k_cxb_finish(const double *__restrict__ part, long long slabs, long long RT,
                                                      int T, int R, double W, double *__restrict__ bs) {
  const long long q = (long long)blockIdx.x * CXB_T + threadIdx.x;
  if (q >= RT) return;
  double s = 0.0;
  for (long long k = 0; k < slabs; k++) s += part[k * RT + q];
  const long long r = q / T, j = q - r * T;
  bs[j * R + r] = s / W;
}

// the row split of k_cxb_terms, a function of n alone
void cox_brier_split(long long n, long long *rows_per_slab, long long *slabs) {
  *rows_per_slab = CXB_ROWS;
  *slabs = (n + CXB_ROWS - 1) / CXB_ROWS;
}

// the row groups of a workgroup of k_cxb_terms for T times: 256 / (the power of two that covers min(T, 256))
int cox_brier_row_groups(int T) {
  int lg = 0;
  while (lg < 8 && (1 << lg) < T) lg++;
  return CXB_T >> lg;
}

// doubles of device memory a bessx_cox_brier_device call holds: time, w and w * a (3 n), e (R n), the slabs' partials
// (slabs R T), hg and the result (2 R T), t and b (2 T).  Nothing n x T.
long long cox_brier_workspace(long long n, int T, int R) {
  long long rows, slabs;
  cox_brier_split(n, &rows, &slabs);
  return 3 * n + (long long)R * n + slabs * R * T + 2LL * R * T + 2LL * T;
}

// e[r * n + i] = exp(clamp(eta(i, r), +-30)); src, cols, B (m x R) as in launch_predict; zero: R device doubles of 0.0
hipError_t launch_cox_brier_ex(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *B, const double *zero, int R, double *ex, hipStream_t st) {
  if (!src || !zero || !ex || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || R < 1 || R > 65535 ||
      rs < 0 || cs < 0)
    return hipErrorInvalidValue;
  const CxbStore epi{n, ex};
  if (f32) return xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, zero, R, epi, st);
  return xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, zero, R, epi, st);
}

// bs[j * R + r] = BS(j, r) from e (R x n, launch_cox_brier_ex), time, w, wa = w * a (n each), hg (R x T), tg and b (T each);
// part: slabs * R * T doubles; W = sum of w > 0 (host).  only = 1 / 2 launches one of the two kernels alone.
hipError_t launch_cox_brier(const double *e, const double *time, const double *w, const double *wa, const double *hg,
                            const double *tg, const double *b, long long n, int T, int R, double W, double *part,
                            double *bs, int only, hipStream_t st) {
  if (!e || !time || !w || !wa || !hg || !tg || !b || !part || !bs || n < 1 || n > 0x7fffffffLL || T < 1 ||
      T > COX_BRIER_T_MAX || R < 1 || R > 65535 || !(W > 0.0))
    return hipErrorInvalidValue;
  long long rows, slabs;
  cox_brier_split(n, &rows, &slabs);
  if (only != 2) {
    int lg = 0;
    while (lg < 8 && (1 << lg) < T) lg++;
    hipLaunchKernelGGL(k_cxb_terms, dim3((unsigned)slabs, (unsigned)R), dim3(CXB_T), 0, st, e, time, w, wa, hg, tg, b, n,
                       T, lg, part);
    LAUNCH_CHECK();
  }
  if (only != 1) {
    const long long RT = (long long)R * T;
    hipLaunchKernelGGL(k_cxb_finish, dim3((unsigned)((RT + CXB_T - 1) / CXB_T)), dim3(CXB_T), 0, st, part, slabs, RT, T,
                       R, W, bs);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

}  // namespace bessx
