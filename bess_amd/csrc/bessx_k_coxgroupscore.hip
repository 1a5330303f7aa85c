// bessx_k_coxgroupscore.hip -- Rao score tests of GROUPS of candidate columns against ONE Cox model on a caller's DEVICE
// matrix, read where it lies (include/bessx.h section 2o).  Positions, r(k), e, wd, S0, H, v, g, dh, A are those of
// bessx_k_coxinfo.hip and bessx_k_coxdiag.hip; the panel, u and the rows of C are section 2m's (launch_cox_addscore_pack,
// launch_addscore_blocks); the band of D = X_J^T diag(v) X_J, T_C = C Rx^T, the band of S and the extraction are section
// 2n's (launch_groupscore_gram with v in row order, launch_groupscore_sband, launch_groupscore_extract), all unchanged.
// This unit adds the one term that has no kernel, the d x d risk-set term of a tested group with columns J:
//     T = sum_p cc_p s_p s_p^T,     s_p = sum_{l >= p} e_l x_{l,J},     cc_p = dh_p / S0(p) >= 0
// (its diagonal is section 2m's t_j; the information's block of the group is (D - T) - S).  T is a Gram matrix of the
// SUFFIX-SUMMED operand with non-negative weights, so it is k_gs_gram's band with another operand: the tested columns of
// a block are tiled 16 per tile whatever the group boundaries are, band width w, upper triangle, mirrored by
// k_gs_extract.  Positions are cut into slabs; within slab s, s_p = s_loc,p + c_s with s_loc the suffix sum inside the
// slab and c_s = sum_{s' > s} A_s', A_s = sum_{l in s} e_l x_l, hence
//     T = sum_s ( Q_s + c_s B_s^T + B_s c_s^T + sigma_s c_s c_s^T ),
//     Q_s = sum_{p in s} cc_p s_loc,p s_loc,p^T,   B_s = sum_{p in s} cc_p s_loc,p,   sigma_s = sum_{p in s} cc_p.
//   k_cgs_cc       cc_p per position: k_cas_cc's operations (dh_p as k_cxd_dh forms it, then one division by S0(p)),
//                  NOT scanned.
//   k_cgs_band     one wave per (tile row t, position slab); four waves = four neighbouring tile rows per workgroup, no
//                  LDS, no barrier, no coupling between waves.  The wave walks its slab from the last chunk of CGS_CH = 32
//                  positions to the first.  Lane (c = lane & 15, q = lane >> 4) holds the CGS_E = 8 consecutive positions
//                  l0 + 8 q .. l0 + 8 q + 7 of column 16 (t + k) + c for its own tile (k = 0) and for the w neighbour
//                  tiles it loads itself: a = e_l * x with x read at row rowof[l] of X in place (element loads at any
//                  strides; on a row-contiguous X the 16 lanes of a k slot read neighbouring columns of one row).  The
//                  running local suffix sum of a column is a scan of the lane's eight values from the last to the first,
//                  a scan of the four k-lanes' totals (three lane exchanges) and the carry from the chunks behind, every
//                  lane of a column forming the same carry.  Step g of a chunk feeds A[m = c][k = q] = s_loc of the own
//                  tile and B[k = q][n = c] = cc (.) s_loc of tile t + k to v_mfma_f64_16x16x4_f64.  A chunk that lies
//                  wholly inside the slab is loaded without guards (a lane past the list reads the list's last column
//                  and is then set to zero); positions >= n and list entries >= qb enter as exact zeros and are not read.
//                  Entry (m, n) of tile (t, t + k) is sum_p s_p[16 t + m] * (cc_p s_p[16 (t + k) + n]): above the diagonal
//                  always (earlier column) x (cc later column), and a column's suffix sums are formed from that column
//                  alone, so the bits depend neither on where a block starts nor on the layout.  Written per slab and
//                  tile row: the NT band tiles of Q_s, and for the own tile A_s (the final carry), B_s (the lanes' fma
//                  sums, the four k-lanes added in descending order) and sigma_s.
//   k_cgs_finish   block = band tile (t, t + k), thread = entry (j, j'): the slabs in DESCENDING order with the carries
//                  c_j, c_j' of its two columns: acc += Q_s; acc = fma(c_j, B_s[j'], acc); acc = fma(B_s[j], c_j', acc);
//                  acc = fma(sigma_s * c_j, c_j', acc); c += A_s.  One fixed order, explicit operations.
// The slab split is a function of n alone, so every candidate_block gives the same bits.  No floating-point atomics.
// Index arithmetic in 64 bits.
#include <algorithm>

#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int CGS_E = 8;               // consecutive positions per lane and chunk
constexpr int CGS_CH = 4 * CGS_E;      // positions per chunk: 4 k-lanes x CGS_E
constexpr int CGS_SLABS_MAX = 32;      // at most this many position slabs
constexpr int CGS_NT_MAX = 5;          // GS_NT_MAX of bessx_k_groupscore.hip
constexpr int CGS_T = 256;
constexpr int CGS_VEC = 48;            // doubles per (slab, tile row) of the vectors: A (16), B (16), sigma (1), padding

}  // namespace

// cc_p = dh_p / S0(p) by k_cas_cc's operations (lastk null: ties "order")
__global__ void __launch_bounds__(CGS_T) k_cgs_cc(const double *__restrict__ wd, const double *__restrict__ S0,
                                                  const int *__restrict__ first, const int *__restrict__ lastk,
                                                  long long n, double *__restrict__ cc) {
  const long long p = (long long)blockIdx.x * CGS_T + threadIdx.x;
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

// grid (ceil(trb / 4), slabs); wave w of a workgroup is tile row 4 blockIdx.x + w.  cand: the block's qb list entries.
// qpart[((slab * trb + t) * NT + k) * 256 + reg * 64 + lane], vpart[(slab * trb + t) * CGS_VEC + {c, 16 + c, 32}]
template <typename T, int NT>
__global__ void __launch_bounds__(256) k_cgs_band(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                  const int *__restrict__ cand, int qb, const int *__restrict__ rowof,
                                                  const double *__restrict__ e, const double *__restrict__ ccw,
                                                  long long rps, int trb, double *__restrict__ qpart,
                                                  double *__restrict__ vpart) {
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int tr = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), slab = (int)blockIdx.y;
  if (tr >= trb) return;  // (wave-uniform; the kernel has no barrier)
  const int nk = min(NT, trb - tr);
  const T *pc[NT];
  bool valid[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) {
    const int jl = 16 * (tr + k) + c;
    valid[k] = k < nk && jl < qb;
    pc[k] = src + (long long)cand[min(jl, qb - 1)] * cs;  // (a lane past the list points at the list's last column)
  }
  const long long l_begin = (long long)slab * rps, l_end = min(n, l_begin + rps);
  const int nch = (int)((l_end - l_begin + CGS_CH - 1) / CGS_CH);
  d4 acc[NT];
  double carry[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) acc[k] = d4{0.0, 0.0, 0.0, 0.0}, carry[k] = 0.0;
  double Bl = 0.0, sg = 0.0;
  for (int ch = nch - 1; ch >= 0; ch--) {
    const long long i0 = l_begin + (long long)ch * CGS_CH + q * CGS_E;
    double ev[CGS_E], cv[CGS_E], x[NT][CGS_E];
    if (l_begin + (long long)(ch + 1) * CGS_CH <= l_end) {  // (wave-uniform) the whole chunk lies inside the slab
      long long ro[CGS_E];
#pragma unroll
      for (int j = 0; j < CGS_E; j++) {
        ro[j] = (long long)rowof[i0 + j] * rs;
        ev[j] = e[i0 + j];
        cv[j] = ccw[i0 + j];
      }
#pragma unroll
      for (int k = 0; k < NT; k++)
        if (k < nk) {
#pragma unroll
          for (int j = 0; j < CGS_E; j++) x[k][j] = (double)pc[k][ro[j]];
        }
#pragma unroll
      for (int k = 0; k < NT; k++)
#pragma unroll
        for (int j = 0; j < CGS_E; j++) x[k][j] = valid[k] ? x[k][j] : 0.0;
    } else {
#pragma unroll
      for (int j = 0; j < CGS_E; j++) {
        const bool in = i0 + j < l_end;
        const long long ro = in ? (long long)rowof[i0 + j] * rs : 0;
        ev[j] = in ? e[i0 + j] : 0.0;
        cv[j] = in ? ccw[i0 + j] : 0.0;
#pragma unroll
        for (int k = 0; k < NT; k++) x[k][j] = (in && valid[k]) ? (double)pc[k][ro] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < CGS_E; j++) sg = __dadd_rn(sg, cv[j]);
    // the local suffix sums of every tile's column: the lane's eight values from the last to the first, the totals of the
    // k-lanes behind it, the carry of the chunks behind
#pragma unroll
    for (int k = 0; k < NT; k++) {
      if (k < nk) {  // (wave-uniform: the lane exchanges below are made by whole waves)
        double ls[CGS_E];
        ls[CGS_E - 1] = __dmul_rn(ev[CGS_E - 1], x[k][CGS_E - 1]);
#pragma unroll
        for (int j = CGS_E - 2; j >= 0; j--) ls[j] = __dadd_rn(ls[j + 1], __dmul_rn(ev[j], x[k][j]));
        const double t0 = __shfl(ls[0], c), t1 = __shfl(ls[0], c + 16), t2 = __shfl(ls[0], c + 32),
                     t3 = __shfl(ls[0], c + 48);
        const double b3 = carry[k], b2 = __dadd_rn(b3, t3), b1 = __dadd_rn(b2, t2), b0 = __dadd_rn(b1, t1);
        const double base = q == 3 ? b3 : (q == 2 ? b2 : (q == 1 ? b1 : b0));
        carry[k] = __dadd_rn(b0, t0);
#pragma unroll
        for (int j = 0; j < CGS_E; j++) x[k][j] = __dadd_rn(base, ls[j]);  // (x now holds s_loc)
      }
    }
#pragma unroll
    for (int j = 0; j < CGS_E; j++) Bl = fma(cv[j], x[0][j], Bl);
#pragma unroll
    for (int j = 0; j < CGS_E; j++)
#pragma unroll
      for (int k = 0; k < NT; k++)
        if (k < nk)  // (wave-uniform)
          acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[0][j], __dmul_rn(cv[j], x[k][j]), acc[k], 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < NT; k++) {
    if (k < nk) {
      double *o = qpart + (((long long)slab * trb + tr) * NT + k) * 256 + lane;
      o[0] = acc[k].x;
      o[64] = acc[k].y;
      o[128] = acc[k].z;
      o[192] = acc[k].w;
    }
  }
  // the four k-lanes of a column, the lane of the last positions first
  const double B3 = __shfl(Bl, c + 48), B2 = __shfl(Bl, c + 32), B1 = __shfl(Bl, c + 16), B0 = __shfl(Bl, c);
  const double S3 = __shfl(sg, 48), S2 = __shfl(sg, 32), S1 = __shfl(sg, 16), S0 = __shfl(sg, 0);
  if (q == 0) {
    double *o = vpart + ((long long)slab * trb + tr) * CGS_VEC;
    o[c] = carry[0];
    o[16 + c] = __dadd_rn(__dadd_rn(__dadd_rn(B3, B2), B1), B0);
    if (c == 0) o[32] = __dadd_rn(__dadd_rn(__dadd_rn(S3, S2), S1), S0);
  }
}

// block = band tile (t, t + k); thread = register r (threadIdx.x >> 6) of lane (c, q): entry (j = 16 t + 4 r + q, j' = 16
// (t + k) + c).  The slabs in descending order.
__global__ void __launch_bounds__(256) k_cgs_finish(const double *__restrict__ qpart, const double *__restrict__ vpart,
                                                    int slabs, int trb, int NT, double *__restrict__ band) {
  const int tr = (int)blockIdx.x / NT, k = (int)blockIdx.x % NT;
  if (tr + k >= trb) return;
  const int lane = threadIdx.x & 63, cj2 = lane & 15, mj = 4 * (int)(threadIdx.x >> 6) + (lane >> 4);
  double acc = 0.0, c1 = 0.0, c2 = 0.0;
  for (int sl = slabs - 1; sl >= 0; sl--) {
    const double *v1 = vpart + ((long long)sl * trb + tr) * CGS_VEC, *v2 = vpart + ((long long)sl * trb + tr + k) * CGS_VEC;
    const double Q = qpart[(((long long)sl * trb + tr) * NT + k) * 256 + threadIdx.x];
    const double A1 = v1[mj], B1 = v1[16 + mj], A2 = v2[cj2], B2 = v2[16 + cj2], sig = v1[32];
    acc = __dadd_rn(acc, Q);
    acc = fma(c1, B2, acc);
    acc = fma(B1, c2, acc);
    acc = fma(__dmul_rn(sig, c1), c2, acc);
    c1 = __dadd_rn(c1, A1);
    c2 = __dadd_rn(c2, A2);
  }
  band[(long long)blockIdx.x * 256 + threadIdx.x] = acc;
}

// the position split of k_cgs_band, a function of n alone, and the longest chain of roundings behind an entry of T: a
// local suffix sum takes at most 4 additions of the carry per chunk, 3 of the k-lanes' totals, 8 inside the lane (twice:
// both factors); the matrix instructions add rows_per_slab products; B_s adds rows_per_slab / 4 + 3; the carry of A_s adds
// `slabs` on each side; the finish makes at most 6 roundings per slab; the products cc s, s s', sigma c: 4
void cox_groupscore_rows(long long n, long long *rows_per_slab, int *slabs, int *t_depth) {
  const long long rps = ((n + CGS_SLABS_MAX - 1) / CGS_SLABS_MAX + CGS_CH - 1) / CGS_CH * CGS_CH;
  const int sl = (int)((n + rps - 1) / rps);
  *rows_per_slab = rps;
  *slabs = sl;
  *t_depth = (int)std::min<long long>(0x7fffffffLL, 2 * (rps / 8 + 11) + rps + rps / 4 + 3 + 2LL * sl + 6LL * sl + 4);
}

// doubles of this unit's workspace for blocks of at most qmax columns: the slabs' band tiles of Q, their vectors, the
// band of T
long long cox_groupscore_doubles(long long n, int qmax, int band) {
  long long rps = 0;
  int slabs = 0, depth = 0;
  cox_groupscore_rows(n, &rps, &slabs, &depth);
  const long long trb = (qmax + 15) / 16, NT = band + 1;
  return (slabs + 1) * trb * NT * 256 + (long long)slabs * trb * CGS_VEC;
}

// cc (n doubles, position order) from wd, S0, first = r(k), lastk (null: ties "order").  Device memory.
hipError_t launch_cox_groupscore_cc(const double *wd, const double *S0, const int *first, const int *lastk, long long n,
                                    double *cc, hipStream_t st) {
  if (!wd || !S0 || !first || !cc || n < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cgs_cc, dim3((unsigned)((n + CGS_T - 1) / CGS_T)), dim3(CGS_T), 0, st, wd, S0, first, lastk, n, cc);
  LAUNCH_CHECK();
  return hipSuccess;
}

template <typename T>
static hipError_t cgs_launch_band(const T *src, long long rs, long long cs, long long n, const int *cand, int qb, int NT,
                                  const int *rowof, const double *e, const double *cc, long long rps, int slabs,
                                  double *qpart, double *vpart, hipStream_t st) {
  const int trb = (qb + 15) / 16;
  const dim3 grid((unsigned)((trb + 3) / 4), (unsigned)slabs);
#define CGS_BAND(N)                                                                                                    \
  hipLaunchKernelGGL((k_cgs_band<T, N>), grid, dim3(256), 0, st, src, rs, cs, n, cand, qb, rowof, e, cc, rps, trb, qpart, \
                     vpart)
  switch (NT) {
    case 1: CGS_BAND(1); break;
    case 2: CGS_BAND(2); break;
    case 3: CGS_BAND(3); break;
    case 4: CGS_BAND(4); break;
    default: CGS_BAND(5); break;
  }
#undef CGS_BAND
  LAUNCH_CHECK();
  return hipSuccess;
}

// the band of T for one block of candidates: cand = the block's qb ascending columns (device), band = w, rowof[position]
// = row, e and cc in position order, work = cox_groupscore_doubles' workspace (the slabs' tiles first, then their
// vectors, then the band of T: *bandT points at it).  only: 0 = both kernels, 1 = k_cgs_band, 2 = k_cgs_finish alone
// (bessx_op_cox_groupscore_bench's stages).  Device memory.
hipError_t launch_cox_groupscore_tband(const void *src, int f32, long long rs, long long cs, long long n, const int *cand,
                                       int qb, int band, const int *rowof, const double *e, const double *cc, double *work,
                                       int only, double **bandT, hipStream_t st) {
  if (!src || !cand || !rowof || !e || !cc || !work || n < 1 || n > 0x7fffffffLL || rs < 0 || cs < 0 || qb < 1 ||
      band < 0 || band + 1 > CGS_NT_MAX)
    return hipErrorInvalidValue;
  long long rps = 0;
  int slabs = 0, depth = 0;
  cox_groupscore_rows(n, &rps, &slabs, &depth);
  const int NT = band + 1, trb = (qb + 15) / 16;
  double *qpart = work, *vpart = qpart + (long long)slabs * trb * NT * 256, *bt = vpart + (long long)slabs * trb * CGS_VEC;
  if (bandT) *bandT = bt;
  if (only == 0 || only == 1) {
    hipError_t er =
        f32 ? cgs_launch_band(static_cast<const float *>(src), rs, cs, n, cand, qb, NT, rowof, e, cc, rps, slabs, qpart, vpart, st)
            : cgs_launch_band(static_cast<const double *>(src), rs, cs, n, cand, qb, NT, rowof, e, cc, rps, slabs, qpart, vpart, st);
    if (er != hipSuccess) return er;
  }
  if (only == 0 || only == 2) {
    hipLaunchKernelGGL(k_cgs_finish, dim3((unsigned)(trb * NT)), dim3(256), 0, st, qpart, vpart, slabs, trb, NT, bt);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

}  // namespace bessx
