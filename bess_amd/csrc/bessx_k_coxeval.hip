// bessx_k_coxeval.hip -- held-out Cox partial log-likelihood and Harrell's concordance of R models on a caller's DEVICE
// matrix.  Positions: k = 0 .. n - 1 is the rank of a row in the stable ascending order of the times (the host sorts and
// uploads pos[row]); first[k] is the smallest position with the time of position k.
//   1. predictor pass    the loops of bessx_k_xb.hpp with a store epilogue: eta(i, r) and exp(clamp(eta, +-30)) go to
//                        position pos[i] of two R x n position-major arrays.  X is read once, the support's columns only.
//   2. risk-set sums     S(k, r) = sum_{l >= k} e(l, r), in place over e, in the two-launch fixed-order form of
//                        k_scan3_tot / k_scan3_apply (bessx_k_cox.hip) with one grid row per model: totals of 1024-element
//                        blocks, then every block adds the totals of the blocks before it in scan order and rescans.
//   3. likelihood        wd(k) * (clamp(eta(k, r)) - log S(k or first[k], r)), wd = w * delta in position order: one
//                        partial per workgroup and model, added by k_eval_finish in a fixed order.  fp64, no
//                        floating-point atomics: the same call gives the same bits.
//   4. pair counts       all pairs of positions, tiled: a workgroup owns 1024 k-positions (4 per thread, in registers)
//                        and streams tiles of 1024 l-positions (eta and the tie-group index first[l]) through LDS.
//                        (k, l) is comparable when delta_k = 1 and first[l] > first[k] -- which also says l > k, so the
//                        diagonal tile needs no special case; kg[k] = first[k] for an event and INT_MAX otherwise folds
//                        delta in.  Counts are 32-bit per thread, 64-bit per workgroup, added with integer atomics (exact,
//                        order-free).  Tiles with l < k are not visited.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CXE_T = 256, CXE_E = 4, CXE_B = CXE_T * CXE_E;  // scan / reduction / pair tile: 1024 positions
constexpr int CXE_LSEG = 8;                                    // l-tiles per workgroup of k_cxe_pairs

struct CxStore {
  static constexpr bool REDUCE = false, SKIPZ = true;
  const int *__restrict__ pos;
  long long n;
  double *__restrict__ eta, *__restrict__ ex;
  __device__ __forceinline__ void store(double v, long long i, int r) const {
    const long long o = (long long)r * n + pos[i];
    eta[o] = v;
    ex[o] = exp(clampv(v, 30.0));
  }
};

}  // namespace

// scr[r * nb + b] = total of block b (scan order: from the last position down) of model r = blockIdx.y
__global__ void __launch_bounds__(CXE_T) k_cxe_scan_tot(const double *__restrict__ e, long long n,
                                                        double *__restrict__ scr) {
  __shared__ double sm[4];
  const double *in = e + (long long)blockIdx.y * n;
  const long long r0 = (long long)blockIdx.x * CXE_B + (long long)threadIdx.x * CXE_E;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < CXE_E; q++)
    if (r0 + q < n) s += in[n - 1 - (r0 + q)];
  double bt;
  (void)block_excl_256(s, sm, &bt);
  if (threadIdx.x == 0) scr[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = bt;
}

// e (R x n) becomes S in place: a thread reads its four elements before it writes them, and no other thread touches them
__global__ void __launch_bounds__(CXE_T) k_cxe_scan_apply(double *__restrict__ e, long long n,
                                                          const double *__restrict__ scr) {
  __shared__ double sm[4];
  double *io = e + (long long)blockIdx.y * n;
  const long long r0 = (long long)blockIdx.x * CXE_B + (long long)threadIdx.x * CXE_E;
  double carry = 0.0;
  for (unsigned j = 0; j < blockIdx.x; j++) carry += scr[(size_t)blockIdx.y * gridDim.x + j];
  double x[CXE_E], tt = 0.0;
#pragma unroll
  for (int q = 0; q < CXE_E; q++) {
    x[q] = r0 + q < n ? io[n - 1 - (r0 + q)] : 0.0;
    tt += x[q];
  }
  double bt;
  double s = carry + block_excl_256(tt, sm, &bt);
#pragma unroll
  for (int q = 0; q < CXE_E; q++)
    if (r0 + q < n) {
      s += x[q];
      io[n - 1 - (r0 + q)] = s;
    }
}

// part[b * R + r] = sum over the 1024 positions of block b of wd * (clamp(eta) - log S[k or first[k]]): a thread's four
// positions in position order, the lanes by the DPP tree of pr_group_sum, the waves in wave order
__global__ void __launch_bounds__(CXE_T) k_cxe_loglik(const double *__restrict__ eta, const double *__restrict__ S,
                                                      const double *__restrict__ wd, const int *__restrict__ first,
                                                      long long n, int R, double *__restrict__ part) {
  __shared__ double red[4];
  const int t = threadIdx.x, r = blockIdx.y;
  const long long k0 = (long long)blockIdx.x * CXE_B + (long long)t * CXE_E, o = (long long)r * n;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < CXE_E; q++) {
    const long long k = k0 + q;
    if (k < n) {
      const double a = clampv(eta[o + k], 30.0);
      s += wd[k] * (a - log(S[o + (first ? (long long)first[k] : k)]));
    }
  }
  s = pr_group_sum<64>(s);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) part[(long long)blockIdx.x * R + r] = ((red[0] + red[1]) + red[2]) + red[3];
}

// cnt[2 * r] += concordant, cnt[2 * r + 1] += discordant pairs (k, l) with k in k-tile blockIdx.x and l in the l-tiles
// of segment blockIdx.y, r = blockIdx.z.  (cnt is zeroed by the launcher.)
__global__ void __launch_bounds__(CXE_T) k_cxe_pairs(const double *__restrict__ eta, const int *__restrict__ kg,
                                                     const int *__restrict__ first, long long n,
                                                     unsigned long long *__restrict__ cnt) {
  const long long kt = blockIdx.x, lt0 = (long long)blockIdx.y * CXE_LSEG;
  if (lt0 + CXE_LSEG <= kt) return;  // (every l of this segment lies before the k-tile)
  __shared__ double le[CXE_B];
  __shared__ int lg[CXE_B];
  __shared__ unsigned long long wsum[2][4];
  const int t = threadIdx.x, r = blockIdx.z;
  const double *er = eta + (long long)r * n;
  double ek[CXE_E];
  int gk[CXE_E];
  unsigned conc[CXE_E], disc[CXE_E];
#pragma unroll
  for (int q = 0; q < CXE_E; q++) {
    const long long k = kt * CXE_B + (long long)q * CXE_T + t;
    ek[q] = k < n ? er[k] : 0.0;
    gk[q] = k < n ? kg[k] : 0x7fffffff;
    conc[q] = disc[q] = 0u;
  }
  const long long nlt = (n + CXE_B - 1) / CXE_B;
  const long long lt_lo = lt0 > kt ? lt0 : kt, lt_hi = lt0 + CXE_LSEG < nlt ? lt0 + CXE_LSEG : nlt;
  for (long long lt = lt_lo; lt < lt_hi; lt++) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CXE_E; q++) {
      const int j = q * CXE_T + t;
      const long long l = lt * CXE_B + j;
      le[j] = l < n ? er[l] : 0.0;
      lg[j] = l < n ? first[l] : -1;  // (-1 > kg never holds: a position past the end pairs with nothing)
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < CXE_B; j++) {
      const double el = le[j];  // (every lane reads the same word: a broadcast)
      const int gl = lg[j];
#pragma unroll
      for (int q = 0; q < CXE_E; q++) {
        const bool c = gl > gk[q];
        conc[q] += (unsigned)(c & (ek[q] > el));
        disc[q] += (unsigned)(c & (ek[q] < el));
      }
    }
  }
  // a thread has counted at most 4 * 8 * 1024 pairs per counter: 32 bits hold them; from here on 64
  unsigned long long c64 = 0, d64 = 0;
#pragma unroll
  for (int q = 0; q < CXE_E; q++) {
    c64 += conc[q];
    d64 += disc[q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c64 += __shfl_down(c64, o);
    d64 += __shfl_down(d64, o);
  }
  if ((t & 63) == 0) {
    wsum[0][t >> 6] = c64;
    wsum[1][t >> 6] = d64;
  }
  __syncthreads();
  if (t < 2) {
    const unsigned long long v = wsum[t][0] + wsum[t][1] + wsum[t][2] + wsum[t][3];
    if (v) atomicAdd(cnt + 2 * (long long)r + t, v);
  }
}

// doubles of workspace launch_cox_eval_loglik needs: the block totals of the scan, then the partials of the reduction
long long cox_eval_workspace(long long n, int R) { return 2 * ((n + CXE_B - 1) / CXE_B) * (long long)R; }

// stage 1: eta and ex (R x n, position-major) from src, cols, B as in launch_predict; pos[i] = position of row i (device);
// zero: R device doubles holding 0.0 (Cox has no intercept)
hipError_t launch_cox_eval_eta(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *B, const double *zero, int R, const int *pos, double *eta, double *ex,
                               hipStream_t st) {
  if (!src || !zero || !pos || !eta || !ex || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || R < 1 ||
      R > 65535 || rs < 0 || cs < 0)
    return hipErrorInvalidValue;
  const CxStore epi{pos, n, eta, ex};
  if (f32) return xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, zero, R, epi, st);
  return xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, zero, R, epi, st);
}

// stage 1 for ONE model, ALWAYS k_xb_rows (never k_xb_gather, whose sums have another order): eta and ex are the same bits
// under every layout of X, which the Cox score tests' layout-independent outputs rely on (bessx_k_coxaddscore.hip)
template <typename T>
static hipError_t cxe_launch_eta_rows(const T *src, long long rs, long long cs, long long n, const int *cols, int m,
                                      const double *B, const double *zero, const CxStore &epi, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const long long rows_per_block = 64LL * PrVec<T>::N;
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block), 1);
  if (vec)
    hipLaunchKernelGGL((k_xb_rows<T, 1, true, CxStore>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, zero, 1, epi);
  else
    hipLaunchKernelGGL((k_xb_rows<T, 1, false, CxStore>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, zero, 1, epi);
  LAUNCH_CHECK();
  return hipSuccess;
}

// whether launch_cox_eval_eta's own pass is k_xb_rows, i.e. its eta and ex are already those of launch_cox_eval_eta_rows
bool cox_eval_eta_by_rows(long long rs, long long cs, int m) { return !(cs == 1 && rs != 1 && m > 0); }

hipError_t launch_cox_eval_eta_rows(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                    int m, const double *B, const double *zero, const int *pos, double *eta, double *ex,
                                    hipStream_t st) {
  if (!src || !zero || !pos || !eta || !ex || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || rs < 0 ||
      cs < 0)
    return hipErrorInvalidValue;
  const CxStore epi{pos, n, eta, ex};
  if (f32) return cxe_launch_eta_rows(static_cast<const float *>(src), rs, cs, n, cols, m, B, zero, epi, st);
  return cxe_launch_eta_rows(static_cast<const double *>(src), rs, cs, n, cols, m, B, zero, epi, st);
}

// the first launch of stage 2 alone: scr[r * nb + b] = total of block b of row r of e (R x n), nb = ceil(n / 1024).  The
// risk-set means of bessx_k_coxinfo.hip follow it with an apply launch of their own.
hipError_t launch_cox_eval_scan_tot(const double *e, long long n, int R, double *scr, hipStream_t st) {
  if (!e || !scr || n < 1 || n > 0x7fffffffLL || R < 1 || R > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + CXE_B - 1) / CXE_B), (unsigned)R);
  hipLaunchKernelGGL(k_cxe_scan_tot, grid, dim3(CXE_T), 0, st, e, n, scr);
  LAUNCH_CHECK();
  return hipSuccess;
}

// stage 2 alone: ex (R x n, position-major) becomes S in place; scr: ceil(n / 1024) * R doubles (the first half of
// cox_eval_workspace).  The baseline hazard of bessx_k_coxsurv.hip starts from the same S.
hipError_t launch_cox_eval_suffix(double *ex, long long n, int R, double *scr, hipStream_t st) {
  if (hipError_t e = launch_cox_eval_scan_tot(ex, n, R, scr, st)) return e;
  const dim3 grid((unsigned)((n + CXE_B - 1) / CXE_B), (unsigned)R);
  hipLaunchKernelGGL(k_cxe_scan_apply, grid, dim3(CXE_T), 0, st, ex, n, scr);
  LAUNCH_CHECK();
  return hipSuccess;
}

// stages 2 and 3: ex becomes S in place; res[r] = loglik of model r.  wd: n doubles (w * delta in position order);
// first: n ints or null (ties = "order": the identity); work: cox_eval_workspace(n, R) doubles; all device memory.
hipError_t launch_cox_eval_loglik(const double *eta, double *ex, const double *wd, const int *first, long long n, int R,
                                  double *work, double *res, hipStream_t st) {
  if (!eta || !ex || !wd || !work || !res || n < 1 || n > 0x7fffffffLL || R < 1 || R > 65535)
    return hipErrorInvalidValue;
  const long long nb = (n + CXE_B - 1) / CXE_B;
  const dim3 grid((unsigned)nb, (unsigned)R);
  double *scr = work, *part = work + nb * R;
  if (hipError_t e = launch_cox_eval_suffix(ex, n, R, scr, st)) return e;
  hipLaunchKernelGGL(k_cxe_loglik, grid, dim3(CXE_T), 0, st, eta, ex, wd, first, n, R, part);
  LAUNCH_CHECK();
  return launch_eval_finish(part, nb, R, res, st);
}

// stage 4: cnt[2 * r], cnt[2 * r + 1] = concordant, discordant pairs of model r.  kg[k] = first[k] where position k is an
// event, INT_MAX elsewhere; first as above (required); cnt: 2 * R device words.
hipError_t launch_cox_eval_pairs(const double *eta, const int *kg, const int *first, long long n, int R,
                                 unsigned long long *cnt, hipStream_t st) {
  if (!eta || !kg || !first || !cnt || n < 1 || n > 0x7fffffffLL || R < 1 || R > 65535) return hipErrorInvalidValue;
  const long long nt = (n + CXE_B - 1) / CXE_B, nseg = (nt + CXE_LSEG - 1) / CXE_LSEG;
  if (nseg > 65535) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(cnt, 0, 2 * (size_t)R * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cxe_pairs, dim3((unsigned)nt, (unsigned)nseg, (unsigned)R), dim3(CXE_T), 0, st, eta, kg, first, n,
                     cnt);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
