// bessx_k_coxinfo.hip -- observed information and score of ONE Cox model on a caller's DEVICE matrix: the risk-set means.
// Positions, pos, first and the tie groups are those of bessx_k_coxeval.hip.  With e = exp(clamp(eta, +-30)), wd = w * status
// in position order, r(k) = k (ties "order") or first[k] ("breslow"), S0(k) = sum_{l >= r(k)} e_l and
// S1(k, c) = sum_{l >= r(k)} e_l x(l, c), u_k = S1(k) / S0(k):
//     info = sum_k wd_k sum_{l >= r(k)} (e_l / S0(k)) (x_l - u_k)(x_l - u_k)^T = G1 - G2,
//     G1 = sum_l v_l x_l x_l^T,  v_l = e_l H_l,  H_l = sum_{k : r(k) <= l} wd_k / S0(k)    (the cumulative hazard at l)
//     G2 = sum_{k : status_k = 1} wd_k u_k u_k^T,            score = sum_l g_l x_l,  g_l = wd_l - v_l.
// The predictor pass (launch_cox_eval_eta), S0 (launch_cox_eval_loglik / _suffix), H (launch_cox_baseline) and the two
// Gram sweeps (launch_info_gram, on X in place and on U) are the existing launchers; this unit adds what lies between:
//   k_cxi_gather_cols / _rows   W(c, k) = e_k * x(row_k, cols[c]), an m x n position-major array, one multiplication per
//                               element.  X's support is read once, fp64 or fp32 (widened in registers, exact), at any
//                               non-negative strides.  _rows serves a row-contiguous source (col_stride == 1): the 64
//                               lanes of a wave gather 64 support columns of one row, a 64 x 64 tile goes through LDS and
//                               is written with the lanes along the positions.  _cols serves every other source: a
//                               thread owns a position and walks a chunk of columns; it reads its column at permuted
//                               rows and writes with the lanes along the positions.
//   k_cxi_scan_emit             the apply launch of the two-launch fixed-order suffix scan (totals: k_cxe_scan_tot with
//                               one grid row per column) over W along k.  S1 is NOT written back: the thread that owns
//                               position p writes U(j, c) = S1(p, c) / S0(p) for the events j whose r(k_j) is p
//                               (jptr[p] <= j < jptr[p + 1]: one event under "order", every event of the tie group that
//                               starts at p under "breslow" -- a data set whose times are all equal has one thread per
//                               column write all of U's column).  U is J x m, column-contiguous, leading dimension ldU.
//   k_cxi_vg                    v and g in ROW order for the sweep over X: v_i = e(pos[i]) * H(last position of the tie
//                               group of pos[i]), g_i = wd(pos[i]) - v_i.
//   k_cxi_finish                info(a, b) = G1(a + 1, b + 1) - G2(a + 1, b + 1) (the sweeps carry an intercept entry that
//                               is dropped), score(a) = U1(a + 1), res[1] = U1(0) = sum_l g_l.  Both triangles of G1 and G2
//                               are exact mirrors, so those of info are.
// Additions only in every scan, one fixed order everywhere, no floating-point atomics: the same call gives the same bits.
// Block counts depend on (n, m, J) alone.  Index arithmetic is in 64 bits.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CXI_T = 256, CXI_E = 4, CXI_B = CXI_T * CXI_E;  // scan block: 1024 positions, as CXE_B
constexpr int CXI_TILE = 64;                                   // positions and columns per tile of k_cxi_gather_rows
constexpr int CXI_CCH = 32;                                    // columns per workgroup of k_cxi_gather_cols

}  // namespace

// thread = position k; blockIdx.y walks chunks of CXI_CCH support columns
template <typename T>
__global__ void __launch_bounds__(CXI_T) k_cxi_gather_cols(const T *__restrict__ src, long long rs, long long cs,
                                                           long long n, const int *__restrict__ cols, int m,
                                                           const int *__restrict__ rowof, const double *__restrict__ e,
                                                           double *__restrict__ W) {
  __shared__ long long co[CXI_CCH];
  const int c0 = (int)blockIdx.y * CXI_CCH, cc = min(CXI_CCH, m - c0);
  if ((int)threadIdx.x < cc) co[threadIdx.x] = (long long)cols[c0 + threadIdx.x] * cs;
  __syncthreads();
  const long long k = (long long)blockIdx.x * CXI_T + threadIdx.x;
  if (k >= n) return;
  const double ek = e[k];
  const T *row = src + (long long)rowof[k] * rs;
#pragma unroll 4
  for (int c = 0; c < cc; c++) W[(long long)(c0 + c) * n + k] = ek * (double)row[co[c]];
}

// block (tile of 64 positions, tile of 64 columns).  Read: wave w takes positions w, w + 4, ... of the tile, lane = column.
// Write: thread t takes position t & 63 and columns t >> 6, + 4, ...
template <typename T>
__global__ void __launch_bounds__(CXI_T) k_cxi_gather_rows(const T *__restrict__ src, long long rs, long long n,
                                                           const int *__restrict__ cols, int m,
                                                           const int *__restrict__ rowof, const double *__restrict__ e,
                                                           double *__restrict__ W) {
  __shared__ double tile[CXI_TILE][CXI_TILE + 1];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long k0 = (long long)blockIdx.x * CXI_TILE;
  const int c0 = (int)blockIdx.y * CXI_TILE;
  const bool cok = c0 + lane < m;
  const long long col = cok ? (long long)cols[c0 + lane] : 0;
  for (int kk = w; kk < CXI_TILE; kk += 4) {
    const long long k = k0 + kk;
    if (cok && k < n) tile[kk][lane] = e[k] * (double)src[(long long)rowof[k] * rs + col];
  }
  __syncthreads();
  const long long k = k0 + lane;
  if (k >= n) return;
  for (int c = w; c < CXI_TILE && c0 + c < m; c += 4) W[(long long)(c0 + c) * n + k] = tile[lane][c];
}

// column c = blockIdx.y of W (m x n): the suffix sums S1(p, c) in scan order (from the last position down), as
// k_cxe_scan_apply forms them, emitted as U(j, c) = S1(p, c) / S0[p] for jptr[p] <= j < jptr[p + 1]
__global__ void __launch_bounds__(CXI_T) k_cxi_scan_emit(const double *__restrict__ W, long long n,
                                                         const double *__restrict__ scr, const double *__restrict__ S0,
                                                         const int *__restrict__ jptr, double *__restrict__ U,
                                                         long long ldU) {
  __shared__ double sm[4];
  const double *in = W + (long long)blockIdx.y * n;
  double *out = U + (long long)blockIdx.y * ldU;
  const long long r0 = (long long)blockIdx.x * CXI_B + (long long)threadIdx.x * CXI_E;
  double carry = 0.0;
  for (unsigned j = 0; j < blockIdx.x; j++) carry += scr[(size_t)blockIdx.y * gridDim.x + j];
  double x[CXI_E], tt = 0.0;
#pragma unroll
  for (int q = 0; q < CXI_E; q++) {
    x[q] = r0 + q < n ? in[n - 1 - (r0 + q)] : 0.0;
    tt += x[q];
  }
  double s = carry + block_excl_256(tt, sm, nullptr);
#pragma unroll
  for (int q = 0; q < CXI_E; q++)
    if (r0 + q < n) {
      s += x[q];
      const long long p = n - 1 - (r0 + q);
      const int j0 = jptr[p], j1 = jptr[p + 1];
      if (j1 > j0) {
        const double u = s / S0[p];
        for (int j = j0; j < j1; j++) out[j] = u;
      }
    }
}

__global__ void __launch_bounds__(CXI_T) k_cxi_vg(const double *__restrict__ e, const double *__restrict__ H,
                                                  const int *__restrict__ lastk, const double *__restrict__ wd,
                                                  const int *__restrict__ pos, long long n, double *__restrict__ v,
                                                  double *__restrict__ g) {
  const long long i = (long long)blockIdx.x * CXI_T + threadIdx.x;
  if (i >= n) return;
  const int k = pos[i];
  const double vi = e[k] * H[lastk ? lastk[k] : k];
  v[i] = vi;
  g[i] = wd[k] - vi;
}

// G1, G2: (m + 1) x (m + 1) dense, U1: m + 1 (launch_info_gram's results); G2 null: no event, nothing is taken off
__global__ void __launch_bounds__(CXI_T) k_cxi_finish(const double *__restrict__ G1, const double *__restrict__ G2,
                                                      const double *__restrict__ U1, int m, double *__restrict__ info,
                                                      long long ld, double *__restrict__ score,
                                                      double *__restrict__ res) {
  const long long q = (long long)blockIdx.x * CXI_T + threadIdx.x, M = (long long)m + 1;
  if (q == 0) res[1] = U1[0];
  if (q >= (long long)m * m) return;
  const long long a = q / m, b = q % m, o = (a + 1) * M + b + 1;
  info[a * ld + b] = G2 ? G1[o] - G2[o] : G1[o];
  if (b == 0) score[a] = U1[a + 1];
}

// the leading dimension of U for J event rows: even, so that every column starts on a 16-byte boundary
long long cox_info_ldu(long long J) { return (J + 1) / 2 * 2; }

// W = e (n doubles, position order) times the support's columns of src, gathered into position order (m x n); rowof[k] =
// the row at position k.  Everything is device memory.
hipError_t launch_cox_info_gather(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                  int m, const int *rowof, const double *e, double *W, hipStream_t st) {
  if (!src || !cols || !rowof || !e || !W || n < 1 || n > 0x7fffffffLL || m < 1 || rs < 0 || cs < 0)
    return hipErrorInvalidValue;
  if (cs == 1 && rs != 1) {
    const dim3 grid((unsigned)((n + CXI_TILE - 1) / CXI_TILE), (unsigned)((m + CXI_TILE - 1) / CXI_TILE));
    if (f32)
      hipLaunchKernelGGL(k_cxi_gather_rows<float>, grid, dim3(CXI_T), 0, st, static_cast<const float *>(src), rs, n, cols,
                         m, rowof, e, W);
    else
      hipLaunchKernelGGL(k_cxi_gather_rows<double>, grid, dim3(CXI_T), 0, st, static_cast<const double *>(src), rs, n,
                         cols, m, rowof, e, W);
  } else {
    const dim3 grid((unsigned)((n + CXI_T - 1) / CXI_T), (unsigned)((m + CXI_CCH - 1) / CXI_CCH));
    if (f32)
      hipLaunchKernelGGL(k_cxi_gather_cols<float>, grid, dim3(CXI_T), 0, st, static_cast<const float *>(src), rs, cs, n,
                         cols, m, rowof, e, W);
    else
      hipLaunchKernelGGL(k_cxi_gather_cols<double>, grid, dim3(CXI_T), 0, st, static_cast<const double *>(src), rs, cs, n,
                         cols, m, rowof, e, W);
  }
  LAUNCH_CHECK();
  return hipSuccess;
}

// U (J x m, column c at U + c * ldU) from W (m x n) and S0 (n suffix sums in position order); jptr: n + 1 ints, ascending,
// jptr[n] = J; scr: ceil(n / 1024) * m doubles.  W is left as it is.
hipError_t launch_cox_info_means(const double *W, const double *S0, const int *jptr, long long n, int m, int J, double *scr,
                                 double *U, long long ldU, hipStream_t st) {
  if (!W || !S0 || !jptr || !scr || !U || n < 1 || n > 0x7fffffffLL || m < 1 || m > 65535 || J < 1 || J > n || ldU < J)
    return hipErrorInvalidValue;
  if (hipError_t e = launch_cox_eval_scan_tot(W, n, m, scr, st)) return e;
  const dim3 grid((unsigned)((n + CXI_B - 1) / CXI_B), (unsigned)m);
  hipLaunchKernelGGL(k_cxi_scan_emit, grid, dim3(CXI_T), 0, st, W, n, scr, S0, jptr, U, ldU);
  LAUNCH_CHECK();
  return hipSuccess;
}

// v, g (n doubles each, ROW order) from e, H, wd (position order); lastk[k] = the last position of k's tie group, or null
// (ties "order": the identity)
hipError_t launch_cox_info_vg(const double *e, const double *H, const int *lastk, const double *wd, const int *pos,
                              long long n, double *v, double *g, hipStream_t st) {
  if (!e || !H || !wd || !pos || !v || !g || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxi_vg, dim3((unsigned)((n + CXI_T - 1) / CXI_T)), dim3(CXI_T), 0, st, e, H, lastk, wd, pos, n, v,
                     g);
  LAUNCH_CHECK();
  return hipSuccess;
}

// info (m x m, leading dimension ld), score (m) and res[1] = the residual sum, from the two sweeps' results
hipError_t launch_cox_info_finish(const double *G1, const double *G2, const double *U1, int m, double *info, long long ld,
                                  double *score, double *res, hipStream_t st) {
  if (!G1 || !U1 || !info || !score || !res || m < 1 || ld < m) return hipErrorInvalidValue;
  const long long cnt = (long long)m * m;
  hipLaunchKernelGGL(k_cxi_finish, dim3((unsigned)((cnt + CXI_T - 1) / CXI_T)), dim3(CXI_T), 0, st, G1, G2, U1, m, info,
                     ld, score, res);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
