// bessx_k_coxaddscore.hip -- Rao score tests of candidate columns against ONE Cox model on a caller's DEVICE matrix, read
// where it lies (include/bessx.h section 2m).  Positions, r(k), e, wd, S0, H, v, g are those of bessx_k_coxinfo.hip, dh and
// A_l = sum_{p <= l} dh_p u_p those of bessx_k_coxdiag.hip, all formed by the launchers of those units as they are.  For a
// candidate column j, row j of the score and of the observed information of the model extended by j at coefficient 0:
//     u_j = sum_l g_l x_lj                                  c_j = sum_l x_lj (v_l x_l - e_l A_l)   (m entries)
//     d_j = sum_l v_l x_lj^2                                t_j = sum_p (dh_p / S0(p)) (sum_{l >= p} e_l x_lj)^2
// (the information's diagonal entry is d_j - t_j).  u, c and d are X_J^T P for the panel P with the ROW-order rows
// (v_i, v_i x_i - e_i A_pos(i), g_i, zeros): k_cas_pack writes it in k_as_pack's [tile][row][16] layout and
// launch_addscore_blocks (k_as_cross, k_as_finish, k_as_stat of bessx_k_addscore.hip, unchanged) does the rest, the factor
// packed with a zero row and column for the panel's column 0, which is v and feeds d's side sum only.
// No risk-set mean of a candidate is formed.  With a_l = e_l x_lj, cc_p = dh_p / S0(p), Cc_l = sum_{p <= l} cc_p:
//     t_j = sum_l a_l (a_l Cc_l + 2 P_l),   P_l = sum_{l' < l} Cc_l' a_l'
// and over slabs of positions, with Q_s the same recurrence started at P = 0, A_s = sum a_l, B_s = sum Cc_l a_l:
//     t_j = sum_s Q_s + 2 sum_s A_s (sum_{s' < s} B_s').
// This unit adds:
//   k_cas_pack        the panel.  Thread (row i, panel column pc): pc = 0: v_i; 1 .. m: fma(v_i, x, -(e_p * A(pc - 1, p))) with
//                     p = pos[i] and x = X(i, cols[pc - 1]) read in place (fp64 or fp32, any non-negative strides); m + 1:
//                     g_i; above, and rows >= n: exact zeros.
//   k_cas_cc          cc_p per position (k_cxd_dh's dh_p, the same operations, then one division by S0(p)).
//   k_cas_scan_tot / _apply
//                     the forward prefix sums Cc of cc in place: totals of 1024-position blocks, then every block adds the
//                     totals before it and rescans (the form of k_cxd_scan_tot / _apply).  Additions only, one fixed order.
//   k_cas_quad        one wave per (64 candidates, position slab); lane = candidate.  The lane walks the slab's positions in
//                     order:  a = e_l * x;  Q = fma(a, fma(a, Cc_l, P + P), Q);  P = fma(Cc_l, a, P);  A += a  -- explicit
//                     operations, so the bits do not hang on the compiler's contraction choice -- and writes Q_s, A_s, B_s =
//                     P.  Two load shapes, ONE arithmetic: DIRECT (col_stride <= row_stride, a row-contiguous X): the 64 lanes
//                     read 64 candidates of row rowof[l], batches of CAS_U positions in flight.  STAGED (a column-contiguous
//                     X): tiles of CAS_TL positions x 64 candidates go through LDS; the loads have the lanes along the
//                     positions (32 positions x 2 candidates per instruction: contiguous where the caller's rows are in
//                     time order), the tile row stride of 65 doubles keeps both the 8-byte stores (16-lane groups) and the
//                     reads (lane = candidate) conflict-free.  Positions past the slab and candidates past the block are
//                     neither read nor entered into the arithmetic.
//   k_cas_quad_fin    thread = candidate: t = (t + Q_s) then fma(A_s + A_s, carry, t), carry += B_s, slabs in ascending order.
// Candidates go in section 2l's blocks; the slab split is a function of (n, q, block) alone; partials are 3 * slabs * block
// doubles whatever p is.  No floating-point atomics: the same call gives the same bits, and every layout of the same
// values gives the same bits.  A NaN in a candidate column reaches that candidate's sums only.  Index arithmetic in 64 bits.
#include <algorithm>

#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CAS_T = 256, CAS_E = 4, CAS_B = CAS_T * CAS_E;  // scan block: 1024 positions, as CXD_B
constexpr int CAS_W = 64;                                      // candidates per workgroup of k_cas_quad (one wave)
constexpr int CAS_TL = 32;                                     // positions per LDS tile (STAGED)
constexpr int CAS_LD = CAS_W + 1;                              // tile row stride in doubles
constexpr int CAS_U = 8;                                       // positions in flight per lane (DIRECT)
constexpr int CAS_WGS = 2048;                                  // workgroups aimed at per block of candidates
constexpr int CAS_SLABS_MAX = 2048;
constexpr int CAS_BLOCK = 2048;                                // AS_BLOCK of bessx_k_addscore.hip

struct CasSplit {
  int CB, groups, slabs;  // candidates per block (a multiple of 16), 64-candidate groups of a block, position slabs
  long long rps;          // positions per slab (a multiple of CAS_TL)
};
inline CasSplit cas_split(long long n, int q, int block) {
  CasSplit sp;
  const int blk = block > 0 ? block : CAS_BLOCK;
  sp.CB = (std::min(q, blk) + 15) / 16 * 16;
  sp.groups = (sp.CB + CAS_W - 1) / CAS_W;
  const long long target =
      std::min<long long>(CAS_SLABS_MAX, std::max<long long>(1, (CAS_WGS + sp.groups - 1) / sp.groups));
  sp.rps = ((n + target - 1) / target + CAS_TL - 1) / CAS_TL * CAS_TL;
  sp.slabs = (int)((n + sp.rps - 1) / sp.rps);
  return sp;
}

// one step of a candidate's recurrence at a position with weight e and accumulated cc = C
__device__ __forceinline__ void cas_step(double e, double C, double x, double &Q, double &P, double &A) {
  const double a = __dmul_rn(e, x);
  Q = fma(a, fma(a, C, __dadd_rn(P, P)), Q);
  P = fma(C, a, P);
  A = __dadd_rn(A, a);
}

}  // namespace

// thread (row i = 16 blockIdx.x + (t >> 4), panel column pc = 16 blockIdx.y + (t & 15)); vw, gw in ROW order, e in position
// order, A m x n position-major (null when m = 0)
template <typename T>
__global__ void __launch_bounds__(256) k_cas_pack(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                  long long n_pad, const int *__restrict__ cols, int m,
                                                  const double *__restrict__ vw, const double *__restrict__ gw,
                                                  const double *__restrict__ e, const int *__restrict__ pos,
                                                  const double *__restrict__ A, long long ldA, double *__restrict__ P) {
  const int c = threadIdx.x & 15, t = (int)blockIdx.y, pc = 16 * t + c;
  const long long i = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= n_pad) return;
  double o = 0.0;
  if (i < n) {
    if (pc == 0) {
      o = vw[i];
    } else if (pc <= m) {
      const long long p = pos[i];
      const double x = (double)src[i * rs + (long long)cols[pc - 1] * cs];
      o = fma(vw[i], x, -__dmul_rn(e[p], A[(long long)(pc - 1) * ldA + p]));
    } else if (pc == m + 1) {
      o = gw[i];
    }
  }
  P[((long long)t * n_pad + i) * 16 + c] = o;
}

// cc_p = dh_p / S0(p): dh_p by the operations of k_cxd_dh (lastk null: ties "order")
__global__ void __launch_bounds__(CAS_T) k_cas_cc(const double *__restrict__ wd, const double *__restrict__ S0,
                                                  const int *__restrict__ first, const int *__restrict__ lastk,
                                                  long long n, double *__restrict__ cc) {
  const long long p = (long long)blockIdx.x * CAS_T + threadIdx.x;
  if (p >= n) return;
  const double S = S0[p];
  double s = 0.0;
  if (!lastk) {
    s = wd[p] / S;
  } else if (first[p] == p) {
    const long long end = lastk[p];
    for (long long k = p; k <= end; k++) s += wd[k] / S;
  }
  cc[p] = s / S;
}

// scr[b] = total of block b, positions in ascending order
__global__ void __launch_bounds__(CAS_T) k_cas_scan_tot(const double *__restrict__ in, long long n,
                                                        double *__restrict__ scr) {
  __shared__ double sm[4];
  const long long k0 = (long long)blockIdx.x * CAS_B + (long long)threadIdx.x * CAS_E;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < CAS_E; q++)
    if (k0 + q < n) s += in[k0 + q];
  double bt;
  (void)block_excl_256(s, sm, &bt);
  if (threadIdx.x == 0) scr[blockIdx.x] = bt;
}

// in place: a thread reads its four elements before it writes them, and no other thread touches them
__global__ void __launch_bounds__(CAS_T) k_cas_scan_apply(double *__restrict__ io, long long n,
                                                          const double *__restrict__ scr) {
  __shared__ double sm[4];
  const long long k0 = (long long)blockIdx.x * CAS_B + (long long)threadIdx.x * CAS_E;
  double carry = 0.0;
  for (unsigned j = 0; j < blockIdx.x; j++) carry += scr[j];
  double x[CAS_E], tt = 0.0;
#pragma unroll
  for (int q = 0; q < CAS_E; q++) {
    x[q] = k0 + q < n ? io[k0 + q] : 0.0;
    tt += x[q];
  }
  double s = carry + block_excl_256(tt, sm, nullptr);
#pragma unroll
  for (int q = 0; q < CAS_E; q++)
    if (k0 + q < n) {
      s += x[q];
      io[k0 + q] = s;
    }
}

// grid (64-candidate groups of the block, slabs); one wave.  part[(slab * 3 + k) * CB + jl], k = 0: Q, 1: A, 2: B.
template <typename T, bool STAGED, bool LIST>
__global__ void __launch_bounds__(CAS_W) k_cas_quad(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                    const int *__restrict__ cand, int j0, int qb,
                                                    const int *__restrict__ rowof, const double *__restrict__ e,
                                                    const double *__restrict__ Cc, long long rps, int CB,
                                                    double *__restrict__ part) {
  const int lane = threadIdx.x, jl = (int)blockIdx.x * CAS_W + lane;
  const bool valid = jl < qb;
  const long long l_begin = (long long)blockIdx.y * rps, l_end = min(n, l_begin + rps);
  const long long colo = valid ? (long long)(LIST ? cand[j0 + jl] : j0 + jl) * cs : 0;
  double Q = 0.0, P = 0.0, A = 0.0;
  if constexpr (STAGED) {
    __shared__ double tile[CAS_TL * CAS_LD];
    __shared__ long long co[CAS_W];
    co[lane] = valid ? colo : -1;
    __syncthreads();
    const int pl = lane & (CAS_TL - 1), h = lane / CAS_TL;  // the lane's position of the tile; which of 2 candidates
    for (long long l0 = l_begin; l0 < l_end; l0 += CAS_TL) {
      const int cnt = (int)min((long long)CAS_TL, l_end - l0);
      const bool rok = pl < cnt;
      const T *row = src + (rok ? (long long)rowof[l0 + pl] * rs : 0);
      double x[CAS_W / 2];
#pragma unroll
      for (int cc2 = 0; cc2 < CAS_W / 2; cc2++) {
        const long long o = co[2 * cc2 + h];
        x[cc2] = (rok && o >= 0) ? (double)row[o] : 0.0;
      }
#pragma unroll
      for (int cc2 = 0; cc2 < CAS_W / 2; cc2++) tile[pl * CAS_LD + 2 * cc2 + h] = x[cc2];
      __syncthreads();
      if (valid) {
        for (int k = 0; k < cnt; k++) cas_step(e[l0 + k], Cc[l0 + k], tile[k * CAS_LD + lane], Q, P, A);
      }
      __syncthreads();
    }
  } else {
    if (valid) {
      const T *cp = src + colo;
      long long l0 = l_begin;
      for (; l0 + CAS_U <= l_end; l0 += CAS_U) {  // whole batches: the loads go out unguarded, all before the first use
        T x[CAS_U];
#pragma unroll
        for (int k = 0; k < CAS_U; k++) x[k] = cp[(long long)rowof[l0 + k] * rs];
#pragma unroll
        for (int k = 0; k < CAS_U; k++) cas_step(e[l0 + k], Cc[l0 + k], (double)x[k], Q, P, A);
      }
      for (; l0 < l_end; l0++) cas_step(e[l0], Cc[l0], (double)cp[(long long)rowof[l0] * rs], Q, P, A);
    }
  }
  if (!valid) return;
  double *o = part + (long long)blockIdx.y * 3 * CB + jl;
  o[0] = Q;
  o[CB] = A;
  o[2 * (long long)CB] = P;
}

// thread = candidate of the block: the slabs in ascending order with the carry of B
__global__ void __launch_bounds__(256) k_cas_quad_fin(const double *__restrict__ part, int slabs, int CB, int j0, int qb,
                                                      double *__restrict__ t_out) {
  const int jl = (int)blockIdx.x * 256 + threadIdx.x;
  if (jl >= qb) return;
  double t = 0.0, carry = 0.0;
  for (int s = 0; s < slabs; s++) {
    const double *p = part + (long long)s * 3 * CB + jl;
    const double Qs = p[0], As = p[CB], Bs = p[2 * (long long)CB];
    t = __dadd_rn(t, Qs);
    t = fma(__dadd_rn(As, As), carry, t);
    carry = __dadd_rn(carry, Bs);
  }
  t_out[j0 + jl] = t;
}

// how the risk-set term of a call is split (a function of n, q and the block asked for alone): doubles of the partials,
// positions per slab, slabs, and the longest chain of additions behind one t_j
void cox_addscore_split(long long n, int q, int block, long long *part_doubles, long long *rows_per_slab, int *slabs,
                        int *t_depth) {
  const CasSplit sp = cas_split(n, q, block);
  *part_doubles = 3LL * sp.slabs * sp.CB;
  *rows_per_slab = sp.rps;
  *slabs = sp.slabs;
  // P_l: at most rps additions in a slab and `slabs` of the carry; on top of it Q: rps in a slab, 2 per slab at the finish
  *t_depth = (int)std::min<long long>(0x7fffffffLL, 2 * sp.rps + 3LL * sp.slabs);
}

// the panel of section 2m: P = panel_doubles of addscore_split(n, m, q, block) doubles.  vw, gw: ROW order; e: position
// order; pos[row] = position; A: m x n position-major, leading dimension ldA (null when m = 0).  Device memory.
hipError_t launch_cox_addscore_pack(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                    int m, int q, int block, const double *vw, const double *gw, const double *e,
                                    const int *pos, const double *A, long long ldA, double *P, hipStream_t st) {
  if (!src || !vw || !gw || !e || !pos || !P || n < 1 || n > 0x7fffffffLL || m < 0 || m + 1 > INFO_M_MAX ||
      (m > 0 && (!cols || !A || ldA < n)) || rs < 0 || cs < 0 || q < 1 || block < 0 || block % 16)
    return hipErrorInvalidValue;
  long long panel = 0, blk = 0, rps = 0;
  int slabs = 0, cb = 0, depth = 0;
  addscore_split(n, m, q, block, &panel, &blk, &rps, &slabs, &cb, &depth);
  const int TP = (m + 2 + 15) / 16;
  const long long n_pad = panel / (16LL * TP);
  const dim3 grid((unsigned)(n_pad / 16), (unsigned)TP);
  if (f32)
    hipLaunchKernelGGL(k_cas_pack<float>, grid, dim3(256), 0, st, static_cast<const float *>(src), rs, cs, n, n_pad, cols,
                       m, vw, gw, e, pos, A, ldA, P);
  else
    hipLaunchKernelGGL(k_cas_pack<double>, grid, dim3(256), 0, st, static_cast<const double *>(src), rs, cs, n, n_pad,
                       cols, m, vw, gw, e, pos, A, ldA, P);
  LAUNCH_CHECK();
  return hipSuccess;
}

// Cc (n doubles) from wd, S0, first = r(k), lastk (null: ties "order"); scr: ceil(n / 1024) doubles.  Device memory.
hipError_t launch_cox_addscore_cc(const double *wd, const double *S0, const int *first, const int *lastk, long long n,
                                  double *scr, double *Cc, hipStream_t st) {
  if (!wd || !S0 || !first || !scr || !Cc || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  const unsigned nt = (unsigned)((n + CAS_T - 1) / CAS_T), nb = (unsigned)((n + CAS_B - 1) / CAS_B);
  hipLaunchKernelGGL(k_cas_cc, dim3(nt), dim3(CAS_T), 0, st, wd, S0, first, lastk, n, Cc);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cas_scan_tot, dim3(nb), dim3(CAS_T), 0, st, Cc, n, scr);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cas_scan_apply, dim3(nb), dim3(CAS_T), 0, st, Cc, n, scr);
  LAUNCH_CHECK();
  return hipSuccess;
}

template <typename T>
static hipError_t cas_launch_quad(const T *src, long long rs, long long cs, long long n, const int *cand, int j0, int qb,
                                  const int *rowof, const double *e, const double *Cc, const CasSplit &sp, double *part,
                                  hipStream_t st) {
  const dim3 grid((unsigned)((qb + CAS_W - 1) / CAS_W), (unsigned)sp.slabs);
  const bool staged = cs > rs;
#define CAS_QUAD(S, L)                                                                                                 \
  hipLaunchKernelGGL((k_cas_quad<T, S, L>), grid, dim3(CAS_W), 0, st, src, rs, cs, n, cand, j0, qb, rowof, e, Cc, sp.rps, \
                     sp.CB, part)
  if (staged && cand)
    CAS_QUAD(true, true);
  else if (staged)
    CAS_QUAD(true, false);
  else if (cand)
    CAS_QUAD(false, true);
  else
    CAS_QUAD(false, false);
#undef CAS_QUAD
  LAUNCH_CHECK();
  return hipSuccess;
}

// t (q doubles) for every block of candidates: cand = q ascending column numbers (device) or null = columns 0 .. q - 1;
// part = part_doubles of cox_addscore_split.  only: 0 = both kernels, 1 = k_cas_quad, 2 = k_cas_quad_fin alone
// (bessx_op_cox_addscore_bench's stages).  Device memory.
hipError_t launch_cox_addscore_quad(const void *src, int f32, long long rs, long long cs, long long n, const int *cand,
                                    int q, int block, const int *rowof, const double *e, const double *Cc, double *part,
                                    double *t, int only, hipStream_t st) {
  if (!src || !rowof || !e || !Cc || !part || !t || n < 1 || n > 0x7fffffffLL || rs < 0 || cs < 0 || q < 1 ||
      block < 0 || block % 16)
    return hipErrorInvalidValue;
  const CasSplit sp = cas_split(n, q, block);
  for (int j0 = 0; j0 < q; j0 += sp.CB) {
    const int qb = std::min(sp.CB, q - j0);
    if (only == 0 || only == 1) {
      hipError_t er = f32 ? cas_launch_quad(static_cast<const float *>(src), rs, cs, n, cand, j0, qb, rowof, e, Cc, sp, part, st)
                          : cas_launch_quad(static_cast<const double *>(src), rs, cs, n, cand, j0, qb, rowof, e, Cc, sp, part, st);
      if (er != hipSuccess) return er;
    }
    if (only == 0 || only == 2) {
      hipLaunchKernelGGL(k_cas_quad_fin, dim3((unsigned)((qb + 255) / 256)), dim3(256), 0, st, part, sp.slabs, sp.CB, j0,
                         qb, t);
      LAUNCH_CHECK();
    }
  }
  return hipSuccess;
}

}  // namespace bessx
