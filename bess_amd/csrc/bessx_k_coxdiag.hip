// bessx_k_coxdiag.hip -- per-row residuals and case influence of ONE Cox model on a caller's DEVICE matrix (include/bessx.h
// section 2j).  Positions, r(k), e, wd, S0, H, v, g, W and the risk-set means U are those of bessx_k_coxinfo.hip, formed by
// the launchers of that unit and of bessx_k_coxeval.hip / bessx_k_coxsurv.hip as they are.  With dh_p = sum_{k : r(k) = p}
// wd_k / S0(p), the hazard increment placed at position p, and A_l = sum_{p <= l} dh_p u_p (m values per position):
//     martingale    g_k = wd_k - v_k                                   (launch_cox_info_vg's g, already in row order)
//     deviance      sign(g_k) sqrt(2 max(v_k - wd_k + wd_k log(wd_k / v_k), 0)),  0 log 0 = 0, sign(0) = 0
//     score         L_k = g_k x_k - wd_k u_{r(k)} + e_k A_k             (n x m; its column sums are section 2h's score)
//     dfbeta        L_k C,  C = inverse(info)                           (n x m)
//     displacement  sum_j t_kj^2,  t_k = R L_k,  C = R^T R, R lower triangular
//     schoenfeld    x_{k_j} - u_{k_j} for the J rows with status = 1, in position order        (J x m)
// This unit adds:
//   k_cxd_dh          dh_p per position: wd_p / S0(p) under "order"; under "breslow" the thread of a tie group's first
//                     position adds wd_k / S0(p) over the group in position order, every other position gets 0.
//   k_cxd_incr        A(c, p) = U(jptr[p], c) * dh_p where an event has r(k) = p, else an exact 0 (U is not read there).
//                     A is m x n position-major like W, with an even leading dimension so that columns stay 16-byte aligned.
//   k_cxd_scan_tot / _apply
//                     the forward prefix sums of A along the positions, per column (blockIdx.y), in place: totals of
//                     1024-position blocks, then every block adds the totals of the blocks before it and rescans (the
//                     form of k_cxs_scan_tot / k_cxs_scan_apply).  Additions only, one fixed order.
//   k_cxd_form        L in place over A: L(c, k) = (g x - wd u) + e A with x = X(rowof[k], cols[c]), the exact element of
//                     X (widened if fp32), read by this kernel: the third pass over X's support after the predictor
//                     and the gather of W (launch_info_gram is not run; schoenfeld reads the J event rows once more).
//                     A thread owns a position and walks a chunk of columns; lanes along the positions for the
//                     writes.  For a row-contiguous X with a scattered support every element is a cache line of its own
//                     whichever way the lanes lie.  One kernel serves every layout: a row's L is the same arithmetic.
//   k_cxd_apply       T = L P^T in 16 x 16 tiles on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), operand layout and
//                     packing as k_diag_lev's 16-byte-load shape: the wave owns 32 positions, slot c of row tile e is
//                     position 2 c + e, lane (c, q) supplies entry 4 ks + q of L for k-step ks with one 16-byte load
//                     that feeds both row tiles; B[k = q][c] = P[16 J + c][4 ks + q] comes packed by cox_diag_pack in
//                     the order the lanes read it.  TRI (displacement, P = R): only the k-steps ks < 4 (J + 1) are
//                     issued; the squares are added per lane in ascending tile order, then across the 16 lanes of a
//                     DPP row; one double goes to row rowof[k].  Full (dfbeta, P = C): every k-step is issued and the
//                     tile is stored to out(rowof[k], 16 J + c).  Output tiles go in runs of four; the A operand is
//                     re-read per run (a column-contiguous tile stays in cache).
//   k_cxd_dev / k_cxd_perm / k_cxd_schoen
//                     the deviance residuals in row order, the permuted write of L into row order, and schoenfeld =
//                     x(evrow[j], cols[c]) - U(j, c): a gather of the J event rows' support entries, fp64 or fp32, any
//                     non-negative strides.
// Entries >= m of L and positions >= n enter as exact zeros and are not read.  No n x m intermediate besides W and A / L,
// no LDS in the apply kernel, no floating-point atomics: a row's dfbeta and displacement depend on that row's L and P
// alone, and the same call gives the same bits.  Block counts depend on (n, m, J) alone.  Index arithmetic is in 64 bits.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CXD_T = 256, CXD_E = 4, CXD_B = CXD_T * CXD_E;  // scan block: 1024 positions, as CXE_B
constexpr int CXD_CCH = 32;                                    // columns per workgroup of k_cxd_form / k_cxd_schoen
constexpr int CXD_JC = 4, CXD_KU = 4;                          // output tiles per run, k-steps of loads in flight

}  // namespace

__global__ void __launch_bounds__(CXD_T) k_cxd_dh(const double *__restrict__ wd, const double *__restrict__ S0,
                                                  const int *__restrict__ first, const int *__restrict__ lastk,
                                                  long long n, double *__restrict__ dh) {
  const long long p = (long long)blockIdx.x * CXD_T + threadIdx.x;
  if (p >= n) return;
  if (!lastk) {
    dh[p] = wd[p] / S0[p];
    return;
  }
  double s = 0.0;
  if (first[p] == p) {
    const double S = S0[p];
    const long long end = lastk[p];
    for (long long k = p; k <= end; k++) s += wd[k] / S;
  }
  dh[p] = s;
}

// thread = position p, blockIdx.y = column c.  U null: no event anywhere.
__global__ void __launch_bounds__(CXD_T) k_cxd_incr(const double *__restrict__ U, long long ldU,
                                                    const int *__restrict__ jptr, const double *__restrict__ dh,
                                                    long long n, double *__restrict__ A, long long ldA) {
  const long long p = (long long)blockIdx.x * CXD_T + threadIdx.x;
  if (p >= n) return;
  double a = 0.0;
  if (U) {
    const int j0 = jptr[p];
    if (jptr[p + 1] > j0) a = U[(long long)blockIdx.y * ldU + j0] * dh[p];
  }
  A[(long long)blockIdx.y * ldA + p] = a;
}

// scr[c * gridDim.x + b] = total of block b of column c = blockIdx.y, positions in ascending order
__global__ void __launch_bounds__(CXD_T) k_cxd_scan_tot(const double *__restrict__ A, long long ldA, long long n,
                                                        double *__restrict__ scr) {
  __shared__ double sm[4];
  const double *in = A + (long long)blockIdx.y * ldA;
  const long long k0 = (long long)blockIdx.x * CXD_B + (long long)threadIdx.x * CXD_E;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < CXD_E; q++)
    if (k0 + q < n) s += in[k0 + q];
  double bt;
  (void)block_excl_256(s, sm, &bt);
  if (threadIdx.x == 0) scr[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = bt;
}

// in place: a thread reads its four elements before it writes them, and no other thread touches them
__global__ void __launch_bounds__(CXD_T) k_cxd_scan_apply(double *__restrict__ A, long long ldA, long long n,
                                                          const double *__restrict__ scr) {
  __shared__ double sm[4];
  double *io = A + (long long)blockIdx.y * ldA;
  const long long k0 = (long long)blockIdx.x * CXD_B + (long long)threadIdx.x * CXD_E;
  double carry = 0.0;
  for (unsigned j = 0; j < blockIdx.x; j++) carry += scr[(size_t)blockIdx.y * gridDim.x + j];
  double x[CXD_E], tt = 0.0;
#pragma unroll
  for (int q = 0; q < CXD_E; q++) {
    x[q] = k0 + q < n ? io[k0 + q] : 0.0;
    tt += x[q];
  }
  double s = carry + block_excl_256(tt, sm, nullptr);
#pragma unroll
  for (int q = 0; q < CXD_E; q++)
    if (k0 + q < n) {
      s += x[q];
      io[k0 + q] = s;
    }
}

// thread = position k; blockIdx.y walks chunks of CXD_CCH support columns.  g is in ROW order; evj[k] = the event index of
// position k or -1; U may be null when no position is an event.
template <typename T>
__global__ void __launch_bounds__(CXD_T) k_cxd_form(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                    const int *__restrict__ cols, int m, const int *__restrict__ rowof,
                                                    const double *__restrict__ g, const double *__restrict__ wd,
                                                    const double *__restrict__ e, const int *__restrict__ evj,
                                                    const double *__restrict__ U, long long ldU,
                                                    double *__restrict__ A, long long ldA) {
  __shared__ long long co[CXD_CCH];
  const int c0 = (int)blockIdx.y * CXD_CCH, cc = min(CXD_CCH, m - c0);
  if ((int)threadIdx.x < cc) co[threadIdx.x] = (long long)cols[c0 + threadIdx.x] * cs;
  __syncthreads();
  const long long k = (long long)blockIdx.x * CXD_T + threadIdx.x;
  if (k >= n) return;
  const int i = rowof[k], j = evj[k];
  const double gk = g[i], wk = wd[k], ek = e[k];
  const T *row = src + (long long)i * rs;
#pragma unroll 4
  for (int c = 0; c < cc; c++) {
    const long long o = (long long)(c0 + c) * ldA + k;
    double t = gk * (double)row[co[c]];
    if (j >= 0) t -= wk * U[(long long)(c0 + c) * ldU + j];
    A[o] = t + ek * A[o];
  }
}

// one wave per workgroup: 32 positions.  pk: cox_diag_pack's order.  TRI: out is n doubles (row order); else out(row, j) at
// out[j * ldo + row].
template <bool TRI>
__global__ void __launch_bounds__(64) k_cxd_apply(const double *__restrict__ L, long long ldL, long long n, int m,
                                                  const double *__restrict__ pk, const int *__restrict__ rowof,
                                                  double *__restrict__ out, long long ldo) {
  constexpr int E = 2, JC = CXD_JC, KU = CXD_KU;
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const long long rb = (long long)blockIdx.x * (16 * E);
  const long long i0 = rb + (long long)c * E;  // the lane's first position as an A operand
  const int TI = (m + 15) / 16;
  double s[E][4];
#pragma unroll
  for (int e = 0; e < E; e++)
#pragma unroll
    for (int r = 0; r < 4; r++) s[e][r] = 0.0;
  // register r of lane (c, q) is row slot q + 4 r, column c of a tile; slot sl of row tile e is position rb + sl * E + e
  int orow[E][4];
  if (!TRI) {
#pragma unroll
    for (int e = 0; e < E; e++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long long k = rb + (long long)(q + 4 * r) * E + e;
        orow[e][r] = k < n ? rowof[k] : -1;
      }
  }
  for (int J0 = 0; J0 < TI; J0 += JC) {
    const int nJ = min(JC, TI - J0);
    d4 acc[E][JC];
#pragma unroll
    for (int e = 0; e < E; e++)
#pragma unroll
      for (int jj = 0; jj < JC; jj++) acc[e][jj] = d4{0.0, 0.0, 0.0, 0.0};
    const int ksteps = TRI ? 4 * (J0 + nJ) : 4 * TI;  // (a multiple of KU)
    for (int k0 = 0; k0 < ksteps; k0 += KU) {
      double xa[KU][E], b[KU][JC];
#pragma unroll
      for (int u = 0; u < KU; u++) {
        const int a = 4 * (k0 + u) + q;
        xa[u][0] = xa[u][1] = 0.0;
        if (a < m) {
          const double *cp = L + (long long)a * ldL;
          if (i0 + E <= n) {
            pr_unpack(*reinterpret_cast<const d2 *>(cp + i0), xa[u]);
          } else if (i0 < n) {
            xa[u][0] = cp[i0];
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < JC; jj++) {
        const int J = J0 + jj;
        if (jj < nJ && (!TRI || k0 < 4 * (J + 1))) {  // (wave-uniform)
          const long long base = TRI ? (long long)2 * J * (J + 1) + k0 : (long long)J * 4 * TI + k0;
#pragma unroll
          for (int u = 0; u < KU; u++) b[u][jj] = pk[(base + u) * 64 + lane];
        }
      }
#pragma unroll
      for (int jj = 0; jj < JC; jj++) {
        if (jj < nJ && (!TRI || k0 < 4 * (J0 + jj + 1))) {
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
        if (TRI) {
#pragma unroll
          for (int e = 0; e < E; e++) {
            s[e][0] = fma(acc[e][jj].x, acc[e][jj].x, s[e][0]);
            s[e][1] = fma(acc[e][jj].y, acc[e][jj].y, s[e][1]);
            s[e][2] = fma(acc[e][jj].z, acc[e][jj].z, s[e][2]);
            s[e][3] = fma(acc[e][jj].w, acc[e][jj].w, s[e][3]);
          }
        } else {
          const int j = 16 * (J0 + jj) + c;
          if (j < m) {
            double *oc = out + (long long)j * ldo;
#pragma unroll
            for (int e = 0; e < E; e++) {
              if (orow[e][0] >= 0) oc[orow[e][0]] = acc[e][jj].x;
              if (orow[e][1] >= 0) oc[orow[e][1]] = acc[e][jj].y;
              if (orow[e][2] >= 0) oc[orow[e][2]] = acc[e][jj].z;
              if (orow[e][3] >= 0) oc[orow[e][3]] = acc[e][jj].w;
            }
          }
        }
      }
    }
  }
  if (!TRI) return;
#pragma unroll
  for (int e = 0; e < E; e++) {
#pragma unroll
    for (int r = 0; r < 4; r++) s[e][r] = pr_group_sum<16>(s[e][r]);
  }
  if (c >= 4) return;  // lane c < 4 of a DPP row writes the positions of register c
#pragma unroll
  for (int e = 0; e < E; e++) {
    const double st2 = c == 0 ? s[e][0] : (c == 1 ? s[e][1] : (c == 2 ? s[e][2] : s[e][3]));
    const long long k = rb + (long long)(q + 4 * c) * E + e;
    if (k < n) out[rowof[k]] = st2;
  }
}

// thread = row i: v, g in row order, wd in position order
__global__ void __launch_bounds__(CXD_T) k_cxd_dev(const double *__restrict__ v, const double *__restrict__ g,
                                                   const double *__restrict__ wd, const int *__restrict__ pos,
                                                   long long n, double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * CXD_T + threadIdx.x;
  if (i >= n) return;
  const double w = wd[pos[i]], vi = v[i], gi = g[i];
  const double dd = (vi - w) + (w == 0.0 ? 0.0 : w * log(w / vi));
  const double sg = gi > 0.0 ? 1.0 : (gi < 0.0 ? -1.0 : 0.0);
  out[i] = sg * sqrt(2.0 * (dd < 0.0 ? 0.0 : dd));
}

// out(rowof[k], c) = L(c, k); thread = position k, blockIdx.y = column c
__global__ void __launch_bounds__(CXD_T) k_cxd_perm(const double *__restrict__ L, long long ldL, long long n,
                                                    const int *__restrict__ rowof, double *__restrict__ out,
                                                    long long ldo) {
  const long long k = (long long)blockIdx.x * CXD_T + threadIdx.x;
  if (k < n) out[(long long)blockIdx.y * ldo + rowof[k]] = L[(long long)blockIdx.y * ldL + k];
}

// thread = event j; blockIdx.y walks chunks of CXD_CCH support columns
template <typename T>
__global__ void __launch_bounds__(CXD_T) k_cxd_schoen(const T *__restrict__ src, long long rs, long long cs,
                                                      const int *__restrict__ cols, int m,
                                                      const int *__restrict__ evrow, int J,
                                                      const double *__restrict__ U, long long ldU,
                                                      double *__restrict__ out, long long ldo) {
  __shared__ long long co[CXD_CCH];
  const int c0 = (int)blockIdx.y * CXD_CCH, cc = min(CXD_CCH, m - c0);
  if ((int)threadIdx.x < cc) co[threadIdx.x] = (long long)cols[c0 + threadIdx.x] * cs;
  __syncthreads();
  const long long j = (long long)blockIdx.x * CXD_T + threadIdx.x;
  if (j >= J) return;
  const T *row = src + (long long)evrow[j] * rs;
#pragma unroll 4
  for (int c = 0; c < cc; c++)
    out[(long long)(c0 + c) * ldo + j] = (double)row[co[c]] - U[(long long)(c0 + c) * ldU + j];
}

// the leading dimension of A / L for n positions: even, so that every column starts on a 16-byte boundary
long long cox_diag_lda(long long n) { return (n + 1) / 2 * 2; }

// additions behind one entry of dfbeta (the k-steps of one tile, a 4-term sum each) and behind one row's displacement (its
// tiles' squares in tile order, then 4 levels of the DPP tree); functions of m alone
int cox_diag_dot_depth(int m) { return (m + 3) / 4 + 4; }
int cox_diag_sum_depth(int m) { return (m + 15) / 16 + 4; }

// doubles of the packed P (m x m): tri = the lower triangle only, k-steps ks < 4 (J + 1) of tile J; else every k-step
long long cox_diag_pack_doubles(int m, int tri) {
  const long long TI = (m + 15) / 16;
  return tri ? 2 * TI * (TI + 1) * 64 : TI * 4 * TI * 64;
}

// P in the order the lanes consume it (host memory): (tile J, k-step ks) holds P[16 J + c][4 ks + q] at lane 16 q + c.
// Entries past m are zeros; tri: entries above the diagonal are zeros and the strict upper triangle of P is not read.
void cox_diag_pack(const double *P, long long ld, int m, int tri, double *pk) {
  const int TI = (m + 15) / 16;
  for (int J = 0; J < TI; J++) {
    const int KS = tri ? 4 * (J + 1) : 4 * TI;
    for (int ks = 0; ks < KS; ks++) {
      double *o = pk + ((tri ? (long long)2 * J * (J + 1) : (long long)J * 4 * TI) + ks) * 64;
      for (int lane = 0; lane < 64; lane++) {
        const int j = 16 * J + (lane & 15), k = 4 * ks + (lane >> 4);
        o[lane] = (j < m && k < m && (!tri || k <= j)) ? P[(long long)j * ld + k] : 0.0;
      }
    }
  }
}

// A (m x n position-major, leading dimension ldA) becomes the accumulated means: U (J x m, leading dimension ldU; null when
// J = 0), jptr, S0, wd, first = r(k), lastk (null: ties "order") as in bessx_k_coxinfo.hip; dh: n doubles; scr: ceil(n / 1024)
// * m doubles.  Device memory.
hipError_t launch_cox_diag_accum(const double *U, long long ldU, const int *jptr, const double *wd, const double *S0,
                                 const int *first, const int *lastk, long long n, int m, double *dh, double *scr,
                                 double *A, long long ldA, hipStream_t st) {
  if (!wd || !S0 || !first || !dh || !scr || !A || n < 1 || n > 0x7fffffffLL || m < 1 || m > 65535 || ldA < n ||
      (U && (!jptr || ldU < 1)))
    return hipErrorInvalidValue;
  const unsigned nt = (unsigned)((n + CXD_T - 1) / CXD_T), nb = (unsigned)((n + CXD_B - 1) / CXD_B);
  hipLaunchKernelGGL(k_cxd_dh, dim3(nt), dim3(CXD_T), 0, st, wd, S0, first, lastk, n, dh);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cxd_incr, dim3(nt, (unsigned)m), dim3(CXD_T), 0, st, U, ldU, jptr, dh, n, A, ldA);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cxd_scan_tot, dim3(nb, (unsigned)m), dim3(CXD_T), 0, st, A, ldA, n, scr);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cxd_scan_apply, dim3(nb, (unsigned)m), dim3(CXD_T), 0, st, A, ldA, n, scr);
  LAUNCH_CHECK();
  return hipSuccess;
}

// L in place over A: g in ROW order, wd, e in position order, evj[k] = event index of position k or -1
hipError_t launch_cox_diag_form(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                                const int *rowof, const double *g, const double *wd, const double *e, const int *evj,
                                const double *U, long long ldU, double *A, long long ldA, hipStream_t st) {
  if (!src || !cols || !rowof || !g || !wd || !e || !evj || !A || n < 1 || n > 0x7fffffffLL || m < 1 || rs < 0 ||
      cs < 0 || ldA < n)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + CXD_T - 1) / CXD_T), (unsigned)((m + CXD_CCH - 1) / CXD_CCH));
  if (f32)
    hipLaunchKernelGGL(k_cxd_form<float>, grid, dim3(CXD_T), 0, st, static_cast<const float *>(src), rs, cs, n, cols, m,
                       rowof, g, wd, e, evj, U, ldU, A, ldA);
  else
    hipLaunchKernelGGL(k_cxd_form<double>, grid, dim3(CXD_T), 0, st, static_cast<const double *>(src), rs, cs, n, cols,
                       m, rowof, g, wd, e, evj, U, ldU, A, ldA);
  LAUNCH_CHECK();
  return hipSuccess;
}

// out = L P^T: tri: out[rowof[k]] = sum_j t_kj^2 (n doubles); else out[j * ldo + rowof[k]] = t_kj.  L: base and ldL keep
// every column 16-byte aligned (cox_diag_lda).  pk: cox_diag_pack_doubles(m, tri) doubles from cox_diag_pack.
hipError_t launch_cox_diag_apply(const double *L, long long ldL, long long n, int m, const double *pk, int tri,
                                 const int *rowof, double *out, long long ldo, hipStream_t st) {
  if (!L || !pk || !rowof || !out || n < 1 || n > 0x7fffffffLL || m < 1 || m + 1 > INFO_M_MAX || ldL < n || ldL % 2 ||
      (reinterpret_cast<uintptr_t>(L) & 15) || (!tri && ldo < n))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 31) / 32));
  if (tri)
    hipLaunchKernelGGL(k_cxd_apply<true>, grid, dim3(64), 0, st, L, ldL, n, m, pk, rowof, out, ldo);
  else
    hipLaunchKernelGGL(k_cxd_apply<false>, grid, dim3(64), 0, st, L, ldL, n, m, pk, rowof, out, ldo);
  LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_cox_diag_deviance(const double *v, const double *g, const double *wd, const int *pos, long long n,
                                    double *out, hipStream_t st) {
  if (!v || !g || !wd || !pos || !out || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxd_dev, dim3((unsigned)((n + CXD_T - 1) / CXD_T)), dim3(CXD_T), 0, st, v, g, wd, pos, n, out);
  LAUNCH_CHECK();
  return hipSuccess;
}

hipError_t launch_cox_diag_perm(const double *L, long long ldL, long long n, int m, const int *rowof, double *out,
                                long long ldo, hipStream_t st) {
  if (!L || !rowof || !out || n < 1 || n > 0x7fffffffLL || m < 1 || m > 65535 || ldL < n || ldo < n)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cxd_perm, dim3((unsigned)((n + CXD_T - 1) / CXD_T), (unsigned)m), dim3(CXD_T), 0, st, L, ldL, n,
                     rowof, out, ldo);
  LAUNCH_CHECK();
  return hipSuccess;
}

// out(j, c) = x(evrow[j], cols[c]) - U(j, c) for the J event rows in position order (column c at out + c * ldo)
hipError_t launch_cox_diag_schoenfeld(const void *src, int f32, long long rs, long long cs, const int *cols, int m,
                                      const int *evrow, int J, const double *U, long long ldU, double *out,
                                      long long ldo, hipStream_t st) {
  if (!src || !cols || !evrow || !U || !out || m < 1 || J < 1 || rs < 0 || cs < 0 || ldU < J || ldo < J)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((J + CXD_T - 1) / CXD_T), (unsigned)((m + CXD_CCH - 1) / CXD_CCH));
  if (f32)
    hipLaunchKernelGGL(k_cxd_schoen<float>, grid, dim3(CXD_T), 0, st, static_cast<const float *>(src), rs, cs, cols, m,
                       evrow, J, U, ldU, out, ldo);
  else
    hipLaunchKernelGGL(k_cxd_schoen<double>, grid, dim3(CXD_T), 0, st, static_cast<const double *>(src), rs, cs, cols, m,
                       evrow, J, U, ldU, out, ldo);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
