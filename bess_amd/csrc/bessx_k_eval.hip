// bessx_k_eval.hip -- held-out loss of R models on a caller's DEVICE matrix in one pass over the support's columns:
//     eta(i, r) = sum_k X(i, cols[k]) * B[k * R + r] + c[r],     L_r = sum_i w_i * f(eta(i, r), y(i, r))
// The loops that form eta are those of prediction (bessx_k_xb.hpp); this file supplies the epilogue that turns eta into
// the row's weighted loss term instead of storing it, and the second launch that adds the workgroups' partials.
//   identity   f = (y - eta)^2
//   logistic   f = max(eta, 0) + log1p(exp(-|eta|)) - y * eta  (negative log-likelihood, overflow-free, no clamp; any y
//              in [0, 1]);  second output A_r = sum_i w_i * [(eta > 0) == (y > 0.5)]
//   Poisson    f = exp(eta) - y * eta  (negative log-likelihood without the term in y alone)
// Reduction order: a workgroup adds its rows in a fixed order (k_xb_rows: a lane's rows in row order, the lanes by the
// DPP tree of pr_group_sum; k_xb_gather: a wave's rows by that tree, the four waves in wave order) and writes ONE
// partial per response; k_eval_finish adds the partials of a response in a fixed order (one wave per response: lane l
// takes blocks l, l + 64, ... in block order, then the lanes' sums go through the same DPP tree).  No floating-point
// atomics: the same call gives the same bits.  All sums are fp64.  n * m elements of X are read (none for m = 0), y and the weights
// are read where they lie (fp64 or fp32, any non-negative stride; a column stride of 0 shares one y between the models).
// A zero coefficient takes nothing from its column (Epi::SKIPZ), so with B holding the union of several supports a NaN
// in a column reaches exactly the models that use it, and only through the rows that hold it.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int EV_WCH = 4096;  // rows per workgroup of k_eval_wsum

__device__ __forceinline__ double ev_load(const void *p, int f32, long long off) {
  return f32 ? (double)static_cast<const float *>(p)[off] : static_cast<const double *>(p)[off];
}

struct EvLoss {
  static constexpr bool REDUCE = true, SKIPZ = true;
  EvalData d;
  int link, RS;  // RS: partials per workgroup = R (+ R for the logistic link's second output)
  int R;
  double *__restrict__ part;
  __device__ __forceinline__ void term(double eta, long long i, int r, double &s, double &a) const {
    const double y = ev_load(d.y, d.y_f32, i * d.yrs + (long long)r * d.ycs);
    const double w = d.w ? ev_load(d.w, d.w_f32, i * d.ws) : 1.0;
    double f;
    if (link == PREDICT_LOGISTIC) {
      // (comparisons, not fmax: a NaN eta stays a NaN through the log1p term)
      f = ((eta > 0.0 ? eta : 0.0) + log1p(exp(-fabs(eta)))) - y * eta;
      a += w * (((eta > 0.0) == (y > 0.5)) ? 1.0 : 0.0);
    } else if (link == PREDICT_POISSON) {
      f = exp(eta) - y * eta;
    } else {
      const double e = y - eta;
      f = e * e;
    }
    s += w * f;
  }
  __device__ __forceinline__ void put(long long blk, int r, double s, double a) const {
    part[blk * RS + r] = s;
    if (RS > R) part[blk * RS + R + r] = a;
  }
};

}  // namespace

// partial sums of the weights: workgroup b adds rows b * EV_WCH ... in a fixed order (a thread's rows in row order, the
// lanes by the DPP tree, the waves in wave order)
__global__ void __launch_bounds__(256) k_eval_wsum(const void *__restrict__ w, int f32, long long ws, long long n,
                                                   double *__restrict__ part) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * EV_WCH;
  double s = 0.0;
  for (int j = 0; j < EV_WCH / 256; j++) {
    const long long i = b0 + (long long)j * 256 + t;
    if (i < n) s += ev_load(w, f32, i * ws);
  }
  s = pr_group_sum<64>(s);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out[q] = sum over the blocks b of part[b * RS + q], q = blockIdx.x < RS, by one wave: lane l adds blocks l, l + 64, ...
// in that order, then the 64 lanes are added by the DPP tree of pr_group_sum -- a fixed order whose depth is nb / 64
__global__ void __launch_bounds__(64) k_eval_finish(const double *__restrict__ part, long long nb, int RS,
                                                    double *__restrict__ out) {
  const int q = blockIdx.x;
  double s = 0.0;
  for (long long b = threadIdx.x; b < nb; b += 64) s += part[b * RS + q];
  s = pr_group_sum<64>(s);
  if (threadIdx.x == 0) out[q] = s;
}

// k_eval_finish for other units (bessx_k_coxeval.hip): out[q] = sum_b part[b * RS + q], q < RS
hipError_t launch_eval_finish(const double *part, long long nb, int RS, double *out, hipStream_t st) {
  if (!part || !out || nb < 1 || RS < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)RS), dim3(64), 0, st, part, nb, RS, out);
  LAUNCH_CHECK();
  return hipSuccess;
}

template <typename T>
static long long ev_blocks(long long rs, long long cs, long long n, int m, int R) {
  const int rt = xb_tile(R);
  const long long rpb = rt == 1 ? xb_rows_per_block<T, 1>(rs, cs, m)
                                : (rt == 4 ? xb_rows_per_block<T, 4>(rs, cs, m) : xb_rows_per_block<T, 8>(rs, cs, m));
  return (n + rpb - 1) / rpb;
}

// doubles of workspace launch_eval needs for this problem
long long eval_workspace(int f32, long long rs, long long cs, long long n, int m, int R, int link, int weighted) {
  const long long nb = f32 ? ev_blocks<float>(rs, cs, n, m, R) : ev_blocks<double>(rs, cs, n, m, R);
  const long long RS = (long long)R * (link == PREDICT_LOGISTIC ? 2 : 1);
  return nb * RS + (weighted ? (n + EV_WCH - 1) / EV_WCH : 0);
}

// res[r] = L_r, (logistic) res[R + r] = A_r, res[2 * R] = sum of the weights (written only when d.w is given); res is a
// device array of 2 * R + 1 doubles, work one of eval_workspace(...) doubles.  src, cols, B, c as in launch_predict.
hipError_t launch_eval(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                       const double *B, const double *c, int R, int link, const EvalData &d, double *work, double *res,
                       hipStream_t st) {
  if (!src || !c || !d.y || !work || !res || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || R < 1 ||
      rs < 0 || cs < 0 || d.yrs < 0 || d.ycs < 0 || d.ws < 0 || link < PREDICT_IDENTITY || link > PREDICT_POISSON)
    return hipErrorInvalidValue;
  const long long nb = f32 ? ev_blocks<float>(rs, cs, n, m, R) : ev_blocks<double>(rs, cs, n, m, R);
  const int RS = R * (link == PREDICT_LOGISTIC ? 2 : 1);
  const EvLoss epi{d, link, RS, R, work};
  hipError_t e = f32 ? xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, c, R, epi, st)
                     : xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, c, R, epi, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)RS), dim3(64), 0, st, work, nb, RS, res);
  LAUNCH_CHECK();
  if (d.w) {
    double *wpart = work + nb * RS;
    const long long nbw = (n + EV_WCH - 1) / EV_WCH;
    hipLaunchKernelGGL(k_eval_wsum, dim3((unsigned)nbw), dim3(256), 0, st, d.w, d.w_f32, d.ws, n, wpart);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(64), 0, st, wpart, nbw, 1, res + 2 * (long long)R);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

}  // namespace bessx
