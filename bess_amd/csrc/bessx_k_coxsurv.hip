// bessx_k_coxsurv.hip -- Breslow baseline cumulative hazard and survival curves of ONE Cox model on a caller's DEVICE
// matrix.  Positions, pos and first are those of bessx_k_coxeval.hip, whose predictor pass (launch_cox_eval_eta) and
// risk-set sums (launch_cox_eval_suffix) the baseline reuses as they are.
//   baseline   h(k) = wd(k) / S(first[k]) (k_cxs_hazard), H(k) = sum_{l <= k} h(l) in place by a forward scan in the
//              two-launch fixed-order form of k_cxe_scan_tot / k_cxe_scan_apply (k_cxs_scan_tot / k_cxs_scan_apply: totals
//              of 1024-position blocks, then every block adds the totals of the blocks before it and rescans), and a
//              gather of H at the last position of every tie group that holds an event (k_cxs_gather).  The scan is
//              ADDITIONS ONLY in fp64, every term enters once, nothing is taken out again (the exclusive offset is
//              block_excl_256, never inclusive - own total): a term of 2^80 leaves the sums in front of it exact to their
//              own size.  No floating-point atomics: the same call gives the same bits.
//   curves     stage one: the loops of bessx_k_xb.hpp with a store epilogue, e_i = exp(clamp(eta_i, +-30)) in ROW order
//              (n doubles; X is read once, the support's columns only).  Stage two, k_cxs_curves, writes the n x T matrix
//              out(i, j) = exp(-(hg[j] * e_i)) or hg[j] * e_i exactly once, the lanes along whichever axis of out has
//              stride 1:
//                ALONG_T     (out_col_stride == 1, T > 1) a workgroup owns 256 rows, their e in LDS; its threads form
//                            256 / TJ row groups of TJ lanes, TJ the power of two that covers T (at most 256); a thread
//                            keeps its one or two hg of the current chunk of columns in registers and walks the rows.
//                ALONG_ROWS  (every other case) a workgroup owns 512 rows, a thread keeps the e of its two rows in
//                            registers and walks a chunk of 64 hg staged in LDS (blockIdx.y walks the chunks).
//              VEC: 16-byte stores where base and strides keep every pair aligned; otherwise element stores at any
//              strides -- the same arithmetic.  No register or LDS array is sized by T or n; index arithmetic is in 64
//              bits.  The round trip of e through memory is 1 / T of the output.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CXS_T = 256, CXS_E = 4, CXS_B = CXS_T * CXS_E;  // scan block: 1024 positions, as CXE_B
constexpr int CXS_ROWS = 256;                                  // rows per workgroup, ALONG_T
constexpr int CXS_HCH = 64;                                    // hg staged per workgroup, ALONG_ROWS

struct CxsStore {
  static constexpr bool REDUCE = false, SKIPZ = true;
  double *__restrict__ ex;
  __device__ __forceinline__ void store(double v, long long i, int) const { ex[i] = exp(clampv(v, 30.0)); }
};

// kind 0: the survival function, 1: the cumulative hazard (BESSX_SURV_* of include/bessx.h)
__device__ __forceinline__ double cxs_value(double hg, double e, int kind) {
  const double z = hg * e;
  return kind ? z : exp(-z);
}

}  // namespace

__global__ void __launch_bounds__(CXS_T) k_cxs_hazard(const double *__restrict__ wd, const double *__restrict__ S,
                                                      const int *__restrict__ first, long long n,
                                                      double *__restrict__ h) {
  const long long k = (long long)blockIdx.x * CXS_T + threadIdx.x;
  if (k < n) h[k] = wd[k] / S[first[k]];
}

// scr[b] = total of block b, positions in ascending order
__global__ void __launch_bounds__(CXS_T) k_cxs_scan_tot(const double *__restrict__ h, long long n,
                                                        double *__restrict__ scr) {
  __shared__ double sm[4];
  const long long k0 = (long long)blockIdx.x * CXS_B + (long long)threadIdx.x * CXS_E;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < CXS_E; q++)
    if (k0 + q < n) s += h[k0 + q];
  double bt;
  (void)block_excl_256(s, sm, &bt);
  if (threadIdx.x == 0) scr[blockIdx.x] = bt;
}

// h becomes H in place: a thread reads its four elements before it writes them, and no other thread touches them
__global__ void __launch_bounds__(CXS_T) k_cxs_scan_apply(double *__restrict__ h, long long n,
                                                          const double *__restrict__ scr) {
  __shared__ double sm[4];
  const long long k0 = (long long)blockIdx.x * CXS_B + (long long)threadIdx.x * CXS_E;
  double carry = 0.0;
  for (unsigned j = 0; j < blockIdx.x; j++) carry += scr[j];
  double x[CXS_E], tt = 0.0;
#pragma unroll
  for (int q = 0; q < CXS_E; q++) {
    x[q] = k0 + q < n ? h[k0 + q] : 0.0;
    tt += x[q];
  }
  double s = carry + block_excl_256(tt, sm, nullptr);
#pragma unroll
  for (int q = 0; q < CXS_E; q++)
    if (k0 + q < n) {
      s += x[q];
      h[k0 + q] = s;
    }
}

__global__ void __launch_bounds__(CXS_T) k_cxs_gather(const double *__restrict__ H, const int *__restrict__ ends, int J,
                                                      double *__restrict__ out) {
  const int g = (int)blockIdx.x * CXS_T + (int)threadIdx.x;
  if (g < J) out[g] = H[ends[g]];
}

// lanes along the columns of out (ocs == 1).  Thread t: column slot t & (TJ - 1), row group t >> tj_log2.
template <bool VEC>
__global__ void __launch_bounds__(CXS_T) k_cxs_curves(const double *__restrict__ e, const double *__restrict__ hg,
                                                      long long n, int T, int kind, int tj_log2,
                                                      double *__restrict__ out, long long ors) {
  constexpr int N = VEC ? 2 : 1;
  __shared__ double es[CXS_ROWS];
  const int t = threadIdx.x, TJ = 1 << tj_log2, TR = CXS_T >> tj_log2, jt = t & (TJ - 1), rt = t >> tj_log2;
  const long long row0 = (long long)blockIdx.x * CXS_ROWS;
  const int rows = (int)(n - row0 < CXS_ROWS ? n - row0 : CXS_ROWS);
  if (t < rows) es[t] = e[row0 + t];
  __syncthreads();
  for (long long j0 = 0; j0 < T; j0 += TJ * N) {
    const long long j = j0 + jt * N;
    if (j >= T) continue;
    double h[N];
#pragma unroll
    for (int q = 0; q < N; q++) h[q] = j + q < T ? hg[j + q] : 0.0;
    for (int r = rt; r < rows; r += TR) {
      const double ei = es[r];
      double *o = out + (row0 + r) * ors + j;
      if (VEC && j + 1 < T) {
        *reinterpret_cast<d2 *>(o) = d2{cxs_value(h[0], ei, kind), cxs_value(h[N - 1], ei, kind)};
      } else {
        o[0] = cxs_value(h[0], ei, kind);  // (VEC: the last column of an odd T)
      }
    }
  }
}

// lanes along the rows of out.  VEC (ors == 1): thread t owns rows row0 + 2 t, + 1; else rows row0 + t, + 256, any strides.
template <bool VEC>
__global__ void __launch_bounds__(CXS_T) k_cxs_curves_rows(const double *__restrict__ e, const double *__restrict__ hg,
                                                           long long n, int T, int kind, double *__restrict__ out,
                                                           long long ors, long long ocs) {
  __shared__ double hs[CXS_HCH];
  const int t = threadIdx.x;
  const int j0 = (int)blockIdx.y * CXS_HCH, jc = T - j0 < CXS_HCH ? T - j0 : CXS_HCH;
  if (t < jc) hs[t] = hg[j0 + t];
  __syncthreads();
  const long long row0 = (long long)blockIdx.x * (2 * CXS_T);
  const long long i0 = VEC ? row0 + 2 * t : row0 + t, i1 = VEC ? i0 + 1 : i0 + CXS_T;
  if (i0 >= n) return;
  const bool two = i1 < n;
  const double e0 = e[i0], e1 = two ? e[i1] : 0.0;
  for (int q = 0; q < jc; q++) {
    const double h = hs[q];  // (every lane reads the same word: a broadcast)
    const long long oc = (long long)(j0 + q) * ocs;
    if (VEC && two) {
      *reinterpret_cast<d2 *>(out + oc + i0) = d2{cxs_value(h, e0, kind), cxs_value(h, e1, kind)};
    } else {
      out[oc + i0 * ors] = cxs_value(h, e0, kind);
      if (two) out[oc + i1 * ors] = cxs_value(h, e1, kind);
    }
  }
}

// doubles of workspace launch_cox_baseline needs on top of cox_eval_workspace: the block totals of the forward scan
long long cox_surv_workspace(long long n) { return (n + CXS_B - 1) / CXS_B; }

// the baseline from S (n suffix sums in position order, launch_cox_eval_suffix): h (n doubles) receives H(k); hout[g] =
// H(ends[g]) for g < J.  wd, first as in launch_cox_eval_loglik (first required); scr: cox_surv_workspace(n) doubles.
hipError_t launch_cox_baseline(const double *S, const double *wd, const int *first, long long n, const int *ends, int J,
                               double *h, double *scr, double *hout, hipStream_t st) {
  if (!S || !wd || !first || !h || !scr || n < 1 || n > 0x7fffffffLL || J < 0 || J > n || (J > 0 && (!ends || !hout)))
    return hipErrorInvalidValue;
  const unsigned nb = (unsigned)((n + CXS_B - 1) / CXS_B);
  hipLaunchKernelGGL(k_cxs_hazard, dim3((unsigned)((n + CXS_T - 1) / CXS_T)), dim3(CXS_T), 0, st, wd, S, first, n, h);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cxs_scan_tot, dim3(nb), dim3(CXS_T), 0, st, h, n, scr);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cxs_scan_apply, dim3(nb), dim3(CXS_T), 0, st, h, n, scr);
  LAUNCH_CHECK();
  if (J > 0) {
    hipLaunchKernelGGL(k_cxs_gather, dim3((unsigned)((J + CXS_T - 1) / CXS_T)), dim3(CXS_T), 0, st, h, ends, J, hout);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

// the forward scan of launch_cox_baseline alone, for another increment (bessx_k_coxband.hip): h becomes its prefix sums in
// place; scr: cox_surv_workspace(n) doubles
hipError_t launch_cox_prefix_scan(double *h, long long n, double *scr, hipStream_t st) {
  if (!h || !scr || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  const unsigned nb = (unsigned)((n + CXS_B - 1) / CXS_B);
  hipLaunchKernelGGL(k_cxs_scan_tot, dim3(nb), dim3(CXS_T), 0, st, h, n, scr);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cxs_scan_apply, dim3(nb), dim3(CXS_T), 0, st, h, n, scr);
  LAUNCH_CHECK();
  return hipSuccess;
}

// curves, stage one: ex[i] = exp(clamp(eta_i, +-30)) in row order; src, cols, B as in launch_predict with R = 1; zero:
// one device double holding 0.0
hipError_t launch_cox_surv_ex(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                              const double *B, const double *zero, double *ex, hipStream_t st) {
  if (!src || !zero || !ex || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || rs < 0 || cs < 0)
    return hipErrorInvalidValue;
  const CxsStore epi{ex};
  if (f32) return xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, zero, 1, epi, st);
  return xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, zero, 1, epi, st);
}

// curves, stage two: out[i * ors + j * ocs] = kind ? hg[j] * ex[i] : exp(-(hg[j] * ex[i])) for i < n, j < T; ex, hg, out
// device memory
hipError_t launch_cox_surv_curves(const double *ex, const double *hg, long long n, int T, int kind, double *out,
                                  long long ors, long long ocs, hipStream_t st) {
  if (!ex || !hg || !out || n < 1 || n > 0x7fffffffLL || T < 1 || (kind != 0 && kind != 1) || ors < 0 || ocs < 0)
    return hipErrorInvalidValue;
  const bool al16 = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (T > 1 && ocs == 1) {
    const bool vec = al16 && ors % 2 == 0;
    int lg = 0;
    while (lg < 8 && ((long long)(vec ? 2 : 1) << lg) < T) lg++;
    const dim3 grid((unsigned)((n + CXS_ROWS - 1) / CXS_ROWS));
    if (vec)
      hipLaunchKernelGGL(k_cxs_curves<true>, grid, dim3(CXS_T), 0, st, ex, hg, n, T, kind, lg, out, ors);
    else
      hipLaunchKernelGGL(k_cxs_curves<false>, grid, dim3(CXS_T), 0, st, ex, hg, n, T, kind, lg, out, ors);
  } else {
    const unsigned chunks = (unsigned)((T + CXS_HCH - 1) / CXS_HCH);
    if (chunks > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 2 * CXS_T - 1) / (2 * CXS_T)), chunks);
    if (ors == 1 && al16 && (T == 1 || ocs % 2 == 0))
      hipLaunchKernelGGL(k_cxs_curves_rows<true>, grid, dim3(CXS_T), 0, st, ex, hg, n, T, kind, out, ors, ocs);
    else
      hipLaunchKernelGGL(k_cxs_curves_rows<false>, grid, dim3(CXS_T), 0, st, ex, hg, n, T, kind, out, ors, ocs);
  }
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
