// bessx_k_coxrmst.hip -- restricted mean and quantile survival times of ONE Cox model on a caller's DEVICE matrix
// (include/bessx.h section 2u).  No curve is stored: RMST is a sum over the steps of S(t | x_i) = exp(-(H0(t) e_i)), a
// quantile a search in a monotone step function.
//   stage one  launch_cox_surv_ex of bessx_k_coxsurv.hip as it is: e_i = exp(clamp(eta_i, +-30)) in ROW order (n doubles;
//              X is read once, the support's columns only).
//   RMST       the host hands over K segments (hs[k] >= 0 the baseline cumulative hazard on segment k, wd[k] > 0 its
//              width) and, per horizon j, cut[j] = the number of segments in front of it:
//                  out(i, j) = sum_{k < cut[j]} wd[k] * exp(-(hs[k] * e_i)).
//              The segments below the largest cut are split into PIECES that end at every distinct cut and after every
//              CXR_SL = 256 segments since the last end (cox_rmst_pieces: a function of K and the cuts alone), so no piece
//              straddles a cut.
//              k_cxr_partial: grid = pieces x row tiles.  A workgroup stages the (hs, wd) pairs of its piece in LDS; a
//              thread owns two rows (512 per tile) with their e in registers, walks the pairs in ascending order (every
//              lane reads the same word: a broadcast) and keeps ONE running sum per row,
//                  acc = fma(wd[k], exp(-(hs[k] * e)), acc)          acc = 0 in front of the first term,
//              the term being cxs_value's expression (kind 0).  THE FORM IS THE FUSED MULTIPLY-ADD: one rounding per
//              term, stated here because the bits depend on it.  The partial of (piece, row) goes to scratch, piece-major.
//              k_cxr_finish: a thread owns one row and keeps one running sum over the pieces in ascending order
//              (additions only, acc = 0 in front of the first -- a NaN row starts from its NaN e, so that even a horizon
//              of 0 tells); when the sum has taken in the last piece in front of a cut it is stored to every column
//              with that cut (colq / colj: the columns sorted by piece count, from the host), through the caller's
//              strides.  Every term enters exactly once; no floating-point atomics; the order is fixed by (K, cuts):
//              given e_i, the bits of a row depend neither on n, nor on where the row lies, nor on the layout or dtype
//              of X, nor on a repeat.  (e_i itself is stage one's: that pass adds the support's products in one order
//              for a row-contiguous X and in another for every other layout, whatever the dtype.)
//   scratch    pieces * rows doubles per launch pair, rows = the rows of one CHUNK: cox_rmst_chunk_rows(n, pieces) =
//              min(n, max(512, 2^24 / pieces rounded down to a multiple of 512)) -- at most 2^24 doubles (128 MiB)
//              unless pieces > 2^15 (then 512 * pieces).  The caller walks the chunks.  No n x K and no n x T temporary.
//   quantile   k_cxr_quantile: one thread per (row, level) does one binary search over hz (J non-decreasing values in
//              device memory) for g* = min{g : hz[g] * e_i >= c} -- the product one fp64 multiplication, compared as it
//              stands; multiplication by e_i > 0 is monotone, so the search is valid -- and stores ut[g*], +inf when
//              there is none (J = 0 included), NaN when e_i is a NaN (NaN >= c is false: it is tested first).
// Index arithmetic is in 64 bits; no register or LDS array is sized by K, T, J or n.
#include "bessx_kdev.hpp"

#include <vector>

namespace bessx {

namespace {

constexpr int CXR_T = 256;                 // threads of a workgroup
constexpr int CXR_SL = 256;                // segments of a piece at most (= CXR_T: one staged pair per thread)
constexpr int CXR_ROWS = 2 * CXR_T;        // rows of a tile of k_cxr_partial
constexpr long long CXR_SCRATCH = 1 << 24; // doubles of partials per chunk of rows, where the pieces allow

// the term: cxs_value(hs, e, 0) of bessx_k_coxsurv.hip
__device__ __forceinline__ double cxr_term(double hs, double e) {
  const double z = hs * e;
  return exp(-z);
}

}  // namespace

__global__ void __launch_bounds__(CXR_T) k_cxr_partial(const double *__restrict__ ex, long long nr,
                                                       const double *__restrict__ hs, const double *__restrict__ wd,
                                                       const int *__restrict__ pstart, double *__restrict__ part) {
  __shared__ double sh[CXR_SL], sw[CXR_SL];
  const int t = threadIdx.x;
  const long long p = blockIdx.x;
  const int k0 = pstart[p], len = pstart[p + 1] - k0;  // (1 <= len <= CXR_SL: cox_rmst_pieces)
  if (t < len) {
    sh[t] = hs[k0 + t];
    sw[t] = wd[k0 + t];
  }
  __syncthreads();
  const long long i0 = (long long)blockIdx.y * CXR_ROWS + t, i1 = i0 + CXR_T;
  if (i0 >= nr) return;
  const bool two = i1 < nr;
  const double e0 = ex[i0], e1 = two ? ex[i1] : 0.0;
  double a0 = 0.0, a1 = 0.0;
  for (int q = 0; q < len; q++) {
    const double h = sh[q], w = sw[q];
    a0 = fma(w, cxr_term(h, e0), a0);
    a1 = fma(w, cxr_term(h, e1), a1);
  }
  part[p * nr + i0] = a0;
  if (two) part[p * nr + i1] = a1;
}

// colq[s] ascending: the pieces in front of the cut of column colj[s]
__global__ void __launch_bounds__(CXR_T) k_cxr_finish(const double *__restrict__ ex, const double *__restrict__ part,
                                                      long long nr, int NP, const int *__restrict__ colq,
                                                      const int *__restrict__ colj, int T, double *__restrict__ out,
                                                      long long ors, long long ocs) {
  const long long i = (long long)blockIdx.x * CXR_T + threadIdx.x;
  if (i >= nr) return;
  const double e = ex[i];
  double acc = e == e ? 0.0 : e;
  double *o = out + i * ors;
  int s = 0;
  for (; s < T && colq[s] == 0; s++) o[(long long)colj[s] * ocs] = acc;
  for (int p = 0; p < NP && s < T; p++) {
    acc += part[(long long)p * nr + i];
    for (; s < T && colq[s] == p + 1; s++) o[(long long)colj[s] * ocs] = acc;
  }
}

__global__ void __launch_bounds__(CXR_T) k_cxr_quantile(const double *__restrict__ ex, long long n,
                                                        const double *__restrict__ hz, const double *__restrict__ ut,
                                                        int J, const double *__restrict__ c, int Q,
                                                        double *__restrict__ out, long long ors, long long ocs) {
  const long long id = (long long)blockIdx.x * CXR_T + threadIdx.x;
  if (id >= n * Q) return;
  const long long i = id / Q;
  const int j = (int)(id - i * Q);
  const double e = ex[i], lev = c[j];
  double r = e;  // (a NaN row)
  if (e == e) {
    int lo = 0, hi = J;  // the first g in [lo, hi] with hz[g] * e >= lev; hi = J: none
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (hz[mid] * e >= lev)
        hi = mid;
      else
        lo = mid + 1;
    }
    r = lo < J ? ut[lo] : __longlong_as_double(0x7ff0000000000000LL);
  }
  out[i * ors + (long long)j * ocs] = r;
}

int cox_rmst_slab() { return CXR_SL; }

// the pieces of the segments below the largest cut: pstart[0] = 0 < ... < pstart[NP] = that cut; qcut[j] = the pieces in
// front of cut[j].  cut: T >= 1 values, each >= 0.  pstart: room for max(cut) / cox_rmst_slab() + T + 1 values; qcut: T.
// Returns NP (0 when every cut is 0).
int cox_rmst_pieces(const int *cut, int T, int *pstart, int *qcut) {
  std::vector<int> ends(cut, cut + T);
  std::sort(ends.begin(), ends.end());
  ends.erase(std::unique(ends.begin(), ends.end()), ends.end());
  std::vector<int> qend(ends.size(), 0);  // pieces in front of the distinct cut
  int NP = 0;
  pstart[0] = 0;
  for (size_t c = 0; c < ends.size(); c++) {
    while (pstart[NP] < ends[c]) {
      pstart[NP + 1] = ends[c] - pstart[NP] > CXR_SL ? pstart[NP] + CXR_SL : ends[c];
      NP++;
    }
    qend[c] = NP;
  }
  for (int j = 0; j < T; j++) qcut[j] = qend[(size_t)(std::lower_bound(ends.begin(), ends.end(), cut[j]) - ends.begin())];
  return NP;
}

long long cox_rmst_chunk_rows(long long n, int NP) {
  long long rows = NP > 0 ? CXR_SCRATCH / NP / CXR_ROWS * CXR_ROWS : n;
  if (rows < CXR_ROWS) rows = CXR_ROWS;
  return rows < n ? rows : n;
}

// part[p * nr + i] = the partial of piece p < NP and row i < nr (ex: the e of these rows)
hipError_t launch_cox_rmst_partial(const double *ex, long long nr, const double *hs, const double *wd, const int *pstart,
                                   int NP, double *part, hipStream_t st) {
  if (!ex || !hs || !wd || !pstart || !part || nr < 1 || NP < 1) return hipErrorInvalidValue;
  const long long tiles = (nr + CXR_ROWS - 1) / CXR_ROWS;
  if (tiles > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxr_partial, dim3((unsigned)NP, (unsigned)tiles), dim3(CXR_T), 0, st, ex, nr, hs, wd, pstart, part);
  LAUNCH_CHECK();
  return hipSuccess;
}

// out[i * ors + colj[s] * ocs] = the sum of the first colq[s] pieces of row i, for i < nr and s < T (colq ascending)
hipError_t launch_cox_rmst_finish(const double *ex, const double *part, long long nr, int NP, const int *colq,
                                  const int *colj, int T, double *out, long long ors, long long ocs, hipStream_t st) {
  if (!ex || (NP > 0 && !part) || !colq || !colj || !out || nr < 1 || nr > 0x7fffffffLL || NP < 0 || T < 1 || ors < 0 ||
      ocs < 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxr_finish, dim3((unsigned)((nr + CXR_T - 1) / CXR_T)), dim3(CXR_T), 0, st, ex, part, nr, NP, colq,
                     colj, T, out, ors, ocs);
  LAUNCH_CHECK();
  return hipSuccess;
}

// out[i * ors + j * ocs] = ut[min{g : hz[g] * ex[i] >= c[j]}], +inf without such a g, NaN for a NaN ex[i]
hipError_t launch_cox_quantile(const double *ex, long long n, const double *hz, const double *ut, int J, const double *c,
                               int Q, double *out, long long ors, long long ocs, hipStream_t st) {
  if (!ex || !c || !out || n < 1 || n > 0x7fffffffLL || Q < 1 || J < 0 || (J > 0 && (!hz || !ut)) || ors < 0 || ocs < 0)
    return hipErrorInvalidValue;
  const long long blocks = (n * Q + CXR_T - 1) / CXR_T;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxr_quantile, dim3((unsigned)blocks), dim3(CXR_T), 0, st, ex, n, hz, ut, J, c, Q, out, ors, ocs);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
