// bessx_k_addscore.hip -- Rao score tests of candidate columns against ONE fitted model (identity, logistic or Poisson
// link) on a caller's DEVICE matrix, read where it lies (include/bessx.h section 2l).  With v_i, g_i of
// bessx_k_info.hip (launch_info_vg: the same bits under every layout), z_i = (1, X(i, cols[0]), ...), M = m + 1, and for
// every candidate column j of a list (or of all p columns):
//     u_j = sum_i g_i x_ij,      c_j = sum_i v_i x_ij z_i  (M entries),      d_j = sum_i v_i x_ij^2
//     s_j = || R c_j ||^2,       a_j = c_j . r             (R lower triangular, inverse(info) = R^T R; r = inverse(info) U)
// Four kernels:
//   1. k_as_pack writes the right-hand panel P once: n_pad x Mp, Mp = 16 ceil((M + 1) / 16), n_pad = n rounded up to
//      AS_CH rows; its columns are v_i z_i (column 0 is v_i itself), then g_i, then exact zeros, and rows >= n are exact
//      zeros.  Layout [tile][row][16]: the 16 columns of a tile of one row are 128 consecutive bytes, a chunk of AS_CH
//      rows of one tile AS_CH * 128 consecutive bytes.  This is the one place where the support is gathered from X: lane
//      (c = lane & 15, q = lane >> 4) takes E consecutive rows of support entry 16 t + c (one 16-byte load where the
//      source allows, E = 2 doubles or 4 floats; element loads at any strides otherwise -- for a row-contiguous source
//      the 16 lanes gather the support's entries of one row).
//   2. k_as_cross: D = X_J^T P in 16 x 16 tiles on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  A workgroup is four
//      waves = four candidate tile rows (16 candidates each) x one run of up to AS_JC panel tiles x one row slab.  The
//      workgroup streams the run's tiles of P through LDS in chunks of AS_CH rows, double-buffered with one barrier per
//      chunk: the next chunk's 16-byte global loads are issued before the matrix instructions of the current one and
//      stored to the other buffer after them.  P is so read from L2 once per FOUR tile rows, and every B operand is one
//      conflict-free 512-byte LDS read.  The A operand is read from X in place: lane (c, q) supplies A[c][k = q], E
//      consecutive rows of candidate 16 tr + c per k group (which row a k slot means is free as long as A and B agree:
//      the chunk is stored to LDS in the order the k slots consume it).  E depends on the element type alone, so the
//      arithmetic and its order are the same under every layout: 16-byte loads down a column-contiguous source, element
//      loads otherwise, where on a row-contiguous source the 16 lanes of a k slot read 16 neighbouring columns of one
//      row; both are issued one chunk ahead.  A list entry of -1 is the constant column 1.  The lanes that hold the A operand also form d_j's partials, fma(v_i, x * x, .) in row order (run 0 only:
//      v_i is column 0 of P, read from the LDS image); the four k lanes of a candidate are added in lane order.
//      Masking: rows >= n and candidates >= q enter as exact zeros and are not read; panel columns > M are exact zeros
//      in P.  A NaN outside the n x p view never reaches a sum; inside the view it propagates.
//      Every wave writes one partial per tile, part[((slab * TRB + tr) * TP + tile) * 256 + reg * 64 + lane], and 16
//      partials of d.
//   3. k_as_finish adds the slabs' partials in a fixed order (lane l takes slabs l, l + 16, ..., then the DPP tree of
//      pr_group_sum) and writes the block's rows of C (leading dimension Mp, the u column and the zero padding
//      included), u, d and, on request, the caller's C.
//   4. k_as_stat: T = C Rx^T in 16 x 16 tiles on the matrix cores, Rx = R with r appended as row M (diag_pack_factor's
//      packing for M + 1 rows; only the k-steps at or below each tile's diagonal).  One wave per candidate tile row;
//      the squares of columns < M are added per candidate, tiles in ascending order, then the DPP tree: s_j.  Column M
//      of T is a_j, a matrix-core dot product in ascending k-steps.
// Candidates are processed in blocks of at most `block` (a multiple of 16): partials and the block's C are bounded
// whatever p is.  The row split is a function of (n, M, q, block) alone.  No floating-point atomics: the same call gives
// the same bits.
#include <vector>

#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int AS_JC = 8;           // panel tiles a workgroup carries
constexpr int AS_CH = 32;          // rows per LDS chunk
constexpr int AS_WGS = 1024;       // workgroups aimed at when the rows are split into slabs
constexpr int AS_SLABS_MAX = 64;   // at most this many slabs
constexpr int AS_BLOCK = 2048;     // candidates per block unless the caller asks for fewer
constexpr int AS_ACC = 16;         // output tiles per run of k_as_stat

struct AsSplit {
  int TP, runs, TRB, block, slabs;
  long long rps, n_pad;
};
inline AsSplit as_split(long long n, int M, int q, int block) {
  AsSplit sp;
  sp.TP = (M + 1 + 15) / 16;
  sp.runs = (sp.TP + AS_JC - 1) / AS_JC;
  sp.block = block > 0 ? block : AS_BLOCK;
  sp.TRB = (std::min(q, sp.block) + 15) / 16;
  sp.n_pad = (n + AS_CH - 1) / AS_CH * AS_CH;
  const long long wgs = (long long)((sp.TRB + 3) / 4) * sp.runs;
  const long long target = std::min<long long>(AS_SLABS_MAX, std::max<long long>(1, (AS_WGS + wgs - 1) / wgs));
  sp.rps = ((n + target - 1) / target + AS_CH - 1) / AS_CH * AS_CH;
  sp.slabs = (int)((n + sp.rps - 1) / sp.rps);
  return sp;
}

// the lane's E rows i0 .. i0 + E - 1 of one column (exact zeros past n, which are not read)
template <typename T, bool VEC, int E>
__device__ __forceinline__ void as_rows(const T *cp, long long rs, long long i0, long long n, double *x) {
#pragma unroll
  for (int e = 0; e < E; e++) x[e] = 0.0;
  if constexpr (VEC) {
    if (i0 + E <= n) {
      pr_unpack(*reinterpret_cast<const typename PrVec<T>::type *>(cp + i0), x);
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < E; e++)
    if (i0 + e < n) x[e] = (double)cp[(i0 + e) * rs];
}

}  // namespace

// one wave per (panel tile, 4 E rows); grid (ceil(n_pad / (4 E * 4)), TP), four waves per workgroup along the rows
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) k_as_pack(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                 long long n_pad, const int *__restrict__ cols, int M,
                                                 const double *__restrict__ vw, const double *__restrict__ gw,
                                                 double *__restrict__ P) {
  constexpr int E = PrVec<T>::N;
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int t = (int)blockIdx.y, pc = 16 * t + c;
  const long long i0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (4 * E) + (long long)q * E;
  if (i0 >= n_pad) return;  // (n_pad is a multiple of E: a lane's rows are all inside or all outside)
  double x[E];
  if (pc >= 1 && pc < M) {
    as_rows<T, VEC, E>(src + (long long)cols[pc - 1] * cs, rs, i0, n, x);
  } else {
#pragma unroll
    for (int e = 0; e < E; e++) x[e] = 1.0;
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
    const long long i = i0 + e;
    double o = 0.0;
    if (i < n) {
      if (pc == 0)
        o = vw[i];
      else if (pc < M)
        o = x[e] * vw[i];
      else if (pc == M)
        o = gw[i];
    }
    P[((long long)t * n_pad + i) * 16 + c] = o;
  }
}

template <typename T, bool VEC, bool LIST>
__global__ void __launch_bounds__(256) k_as_cross(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                  long long n_pad, const int *__restrict__ cand, int j0, int qb,
                                                  const double *__restrict__ P, int TP, int runs, long long rps, int TRB,
                                                  double *__restrict__ part, double *__restrict__ dpart) {
  constexpr int E = PrVec<T>::N, G = AS_CH / (4 * E);  // k groups per chunk: a group is 4 k slots x E rows
  __shared__ double lds[2][AS_JC][AS_CH * 16];
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, q = lane >> 4, w = tid >> 6;
  const int run = (int)blockIdx.x % runs, tr = ((int)blockIdx.x / runs) * 4 + w, slab = (int)blockIdx.y;
  const int slot0 = run * AS_JC, nJ = min(AS_JC, TP - slot0);
  const bool active = tr < TRB;              // (wave-uniform; an inactive wave still loads P and meets the barriers)
  const int jl = 16 * tr + c;
  const bool valid = active && jl < qb;      // the lane's candidate exists
  const T *pa = src;
  bool ones = false;  // (a list entry of -1 is the constant column: the intercept's own score)
  if (valid) {
    const int col = LIST ? cand[j0 + jl] : j0 + jl;
    ones = LIST && col < 0;
    if (!ones) pa = src + (long long)col * cs;
  }
  // where this thread's 16 bytes of a chunk go: row r of the chunk is k slot (r / E) % 4 of MFMA (r / (4 E), r % E)
  const int r = tid >> 3, cp2 = (tid & 7) * 2;
  const int lds_at = ((((r / (4 * E)) * E + (r % E)) * 4) + ((r / E) & 3)) * 16 + cp2;
  const long long r_begin = (long long)slab * rps, r_end = min(n_pad, r_begin + rps);
  const int nch = (int)((r_end - r_begin) / AS_CH);
  d4 acc[AS_JC];
#pragma unroll
  for (int jj = 0; jj < AS_JC; jj++) acc[jj] = d4{0.0, 0.0, 0.0, 0.0};
  double dacc = 0.0;
  d2 pre[AS_JC];
  double xa[G][E], xn[G][E];
  // the lane's rows of chunk i0 as the A operand (exact zeros for a lane without a candidate and past n)
  auto load_a = [&](long long i0, double (*x)[E]) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      const long long i = i0 + g * (4 * E) + q * E;
      if (valid && !ones) {
        as_rows<T, VEC, E>(pa, rs, i, n, x[g]);
      } else {
#pragma unroll
        for (int e = 0; e < E; e++) x[g][e] = (ones && i + e < n) ? 1.0 : 0.0;
      }
    }
  };
#pragma unroll
  for (int jj = 0; jj < AS_JC; jj++)
    if (jj < nJ) {
      pre[jj] = *reinterpret_cast<const d2 *>(P + ((long long)(slot0 + jj) * n_pad + r_begin) * 16 + 2 * tid);
      *reinterpret_cast<d2 *>(&lds[0][jj][lds_at]) = pre[jj];
    }
  if (active) load_a(r_begin, xa);
  __syncthreads();
  for (int ch = 0; ch < nch; ch++) {
    const long long i0 = r_begin + (long long)ch * AS_CH;
    const int cur = ch & 1;
    if (ch + 1 < nch) {  // the next chunk's loads, of P and of the A operand, go out before this chunk's matrix work
#pragma unroll
      for (int jj = 0; jj < AS_JC; jj++)
        if (jj < nJ)
          pre[jj] = *reinterpret_cast<const d2 *>(P + ((long long)(slot0 + jj) * n_pad + i0 + AS_CH) * 16 + 2 * tid);
      if (active) load_a(i0 + AS_CH, xn);
    }
    if (active) {
      if (run == 0) {  // (column 0 of the panel's tile 0 is v_i, an exact zero past n)
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
          for (int e = 0; e < E; e++) dacc = fma(lds[cur][0][(g * E + e) * 64 + 16 * q], xa[g][e] * xa[g][e], dacc);
      }
#pragma unroll
      for (int g = 0; g < G; g++)
#pragma unroll
        for (int e = 0; e < E; e++)
#pragma unroll
          for (int jj = 0; jj < AS_JC; jj++)
            if (jj < nJ)
              acc[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[g][e], lds[cur][jj][(g * E + e) * 64 + lane], acc[jj], 0,
                                                             0, 0);
    }
    if (ch + 1 < nch) {
#pragma unroll
      for (int jj = 0; jj < AS_JC; jj++)
        if (jj < nJ) *reinterpret_cast<d2 *>(&lds[cur ^ 1][jj][lds_at]) = pre[jj];
      if (active) {
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
          for (int e = 0; e < E; e++) xa[g][e] = xn[g][e];
      }
    }
    __syncthreads();
  }
  if (!active) return;
#pragma unroll
  for (int jj = 0; jj < AS_JC; jj++) {
    if (jj < nJ) {
      double *o = part + (((long long)slab * TRB + tr) * TP + slot0 + jj) * 256 + lane;
      o[0] = acc[jj].x;
      o[64] = acc[jj].y;
      o[128] = acc[jj].z;
      o[192] = acc[jj].w;
    }
  }
  if (run == 0) {
    const double d1 = __shfl(dacc, c + 16), d2v = __shfl(dacc, c + 32), d3 = __shfl(dacc, c + 48);
    if (q == 0) dpart[((long long)slab * TRB + tr) * 16 + c] = ((dacc + d1) + d2v) + d3;
  }
}

// block (tile row * TP + tile, quarter): thread t = 16 * grp + lg sums entries e = 64 * quarter + 4 * grp .. + 3 of the
// tile over the slabs lg, lg + 16, ... in slab order; the 16 lanes of a group are then added by the DPP tree.  Entry e =
// 64 * reg + lane is D[candidate (lane >> 4) + 4 * reg][panel column lane & 15] of the tile.  The blocks of tile 0,
// quarter 0 add d's partials as well (group = candidate).
__global__ void __launch_bounds__(256) k_as_finish(const double *__restrict__ part, const double *__restrict__ dpart,
                                                   int slabs, int TRB, int TP, int M, int j0, int qb,
                                                   double *__restrict__ Cb, double *__restrict__ u,
                                                   double *__restrict__ d, double *__restrict__ Cout, long long ldc) {
  const int tr = (int)blockIdx.x / TP, tile = (int)blockIdx.x % TP, lg = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int e0 = (int)blockIdx.y * 64 + grp * 4, Mp = 16 * TP;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int s = lg; s < slabs; s += 16) {
    const double *p = part + (((long long)s * TRB + tr) * TP + tile) * 256 + e0;
    const d2 lo = *reinterpret_cast<const d2 *>(p), hi = *reinterpret_cast<const d2 *>(p + 2);
    sum[0] += lo.x;
    sum[1] += lo.y;
    sum[2] += hi.x;
    sum[3] += hi.y;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) sum[j] = pr_group_sum<16>(sum[j]);
  double ds = 0.0;
  const bool with_d = tile == 0 && blockIdx.y == 0;  // (block-uniform)
  if (with_d) {
    for (int s = lg; s < slabs; s += 16) ds += dpart[((long long)s * TRB + tr) * 16 + grp];
    ds = pr_group_sum<16>(ds);
  }
  if (lg != 0) return;
  if (with_d && 16 * tr + grp < qb) d[j0 + 16 * tr + grp] = ds;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int e = e0 + j, reg = e >> 6, ln = e & 63;
    const int jl = 16 * tr + (ln >> 4) + 4 * reg, pc = 16 * tile + (ln & 15);
    Cb[(long long)jl * Mp + pc] = sum[j];  // (rows past qb and columns past M are sums of exact zeros)
    if (jl < qb) {
      if (pc == M) u[j0 + jl] = sum[j];
      if (pc < M && Cout) Cout[(long long)(j0 + jl) * ldc + pc] = sum[j];
    }
  }
}

// one wave per tile row of 16 candidates: the element-load shape of k_diag_lev with the rows of Cb as its operand
__global__ void __launch_bounds__(64) k_as_stat(const double *__restrict__ Cb, int Mp, int M, int j0, int qb,
                                                const double *__restrict__ pk, double *__restrict__ o_s,
                                                double *__restrict__ o_a) {
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const int TI = Mp / 16, JM = M / 16, cM = M % 16;  // column M of T, the dot product with r, is column cM of tile JM
  const double *row = Cb + ((long long)blockIdx.x * 16 + c) * Mp;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int J0 = 0; J0 < TI; J0 += AS_ACC) {
    const int nJ = min(AS_ACC, TI - J0);
    d4 acc[AS_ACC];
#pragma unroll
    for (int jj = 0; jj < AS_ACC; jj++) acc[jj] = d4{0.0, 0.0, 0.0, 0.0};
    const int ksteps = 4 * (J0 + nJ);
    for (int k0 = 0; k0 < ksteps; k0 += 2) {
      double xa[2], b[2][AS_ACC];
#pragma unroll
      for (int uu = 0; uu < 2; uu++) {
        const int k = 4 * (k0 + uu) + q;
        xa[uu] = k < M ? row[k] : 0.0;  // (column M of Cb is u_j and is not an entry of c_j)
      }
#pragma unroll
      for (int jj = 0; jj < AS_ACC; jj++) {
        const int J = J0 + jj;
        if (jj < nJ && k0 < 4 * (J + 1)) {  // (wave-uniform)
#pragma unroll
          for (int uu = 0; uu < 2; uu++) b[uu][jj] = pk[((long long)2 * J * (J + 1) + k0 + uu) * 64 + lane];
        }
      }
#pragma unroll
      for (int jj = 0; jj < AS_ACC; jj++) {
        if (jj < nJ && k0 < 4 * (J0 + jj + 1)) {
#pragma unroll
          for (int uu = 0; uu < 2; uu++)  // (a tile's k-steps in ascending order)
            acc[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[uu], b[uu][jj], acc[jj], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < AS_ACC; jj++) {
      if (jj < nJ) {
        d4 t = acc[jj];
        if (J0 + jj == JM && c == cM) {  // register r of lane (c, q) is candidate q + 4 r, column 16 J + c
          a[0] = t.x, a[1] = t.y, a[2] = t.z, a[3] = t.w;
          t = d4{0.0, 0.0, 0.0, 0.0};
        }
        s[0] = fma(t.x, t.x, s[0]);
        s[1] = fma(t.y, t.y, s[1]);
        s[2] = fma(t.z, t.z, s[2]);
        s[3] = fma(t.w, t.w, s[3]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) s[r] = pr_group_sum<16>(s[r]);
  const int jb = (int)blockIdx.x * 16 + q;
  if (c == cM) {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (jb + 4 * r < qb) o_a[j0 + jb + 4 * r] = a[r];
  }
  if (c < 4) {  // lane c < 4 of a DPP row writes the candidate of register c
    const double st2 = c == 0 ? s[0] : (c == 1 ? s[1] : (c == 2 ? s[2] : s[3]));
    if (jb + 4 * c < qb) o_s[j0 + jb + 4 * c] = st2;
  }
}

// how a call is split (a function of n, m, q and the block asked for alone) and what it needs besides v and g
void addscore_split(long long n, int m, int q, int block, long long *panel_doubles, long long *block_doubles,
                    long long *rows_per_slab, int *slabs, int *cand_block, int *stat_depth) {
  const AsSplit sp = as_split(n, m + 1, q, block);
  *panel_doubles = (long long)sp.TP * sp.n_pad * 16;
  // the partials of C and d, the block's rows of C, and the packed factor of M + 1 rows
  *block_doubles = (long long)sp.slabs * sp.TRB * ((long long)sp.TP * 256 + 16) + (long long)sp.TRB * 16 * sp.TP * 16 +
                   diag_factor_doubles(m + 1);
  *rows_per_slab = sp.rps;
  *slabs = sp.slabs;
  *cand_block = std::min(sp.block, sp.TRB * 16);
  *stat_depth = sp.TP + 4;  // a candidate's squares: its tiles in ascending order, then 4 levels of the DPP tree
}

// the factor R (lower triangular, (m + 1) x (m + 1), host) with r (m + 1 values) appended as row m + 1, in the order
// k_as_stat's lanes consume it: pk holds diag_factor_doubles(m + 1) doubles
void addscore_pack_factor(const double *R, long long ld, const double *r, int m, double *pk) {
  const int M = m + 1, M1 = M + 1;
  std::vector<double> ext((size_t)M1 * M1, 0.0);
  for (int j = 0; j < M; j++)
    for (int k = 0; k <= j; k++) ext[(size_t)j * M1 + k] = R[(long long)j * ld + k];
  for (int k = 0; k < M; k++) ext[(size_t)M * M1 + k] = r[k];
  diag_pack_factor(ext.data(), M1, m + 1, pk);
}

template <typename T>
static hipError_t as_launch_pack(const T *src, long long rs, long long cs, long long n, const int *cols, int M,
                                 const double *vw, const double *gw, const AsSplit &sp, double *P, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const long long rows_per_block = 16LL * PrVec<T>::N;
  const dim3 grid((unsigned)((sp.n_pad + rows_per_block - 1) / rows_per_block), (unsigned)sp.TP);
  if (vec)
    hipLaunchKernelGGL((k_as_pack<T, true>), grid, dim3(256), 0, st, src, rs, cs, n, sp.n_pad, cols, M, vw, gw, P);
  else
    hipLaunchKernelGGL((k_as_pack<T, false>), grid, dim3(256), 0, st, src, rs, cs, n, sp.n_pad, cols, M, vw, gw, P);
  LAUNCH_CHECK();
  return hipSuccess;
}

template <typename T>
static hipError_t as_launch_cross(const T *src, long long rs, long long cs, long long n, const int *cand, int j0, int qb,
                                  const double *P, const AsSplit &sp, double *part, double *dpart, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const int trb = (qb + 15) / 16;  // (tile rows of THIS block; the partials keep the stride sp.TRB)
  const dim3 grid((unsigned)(((trb + 3) / 4) * sp.runs), (unsigned)sp.slabs);
#define AS_CROSS(V, L)                                                                                                 \
  hipLaunchKernelGGL((k_as_cross<T, V, L>), grid, dim3(256), 0, st, src, rs, cs, n, sp.n_pad, cand, j0, qb, P, sp.TP,   \
                     sp.runs, sp.rps, sp.TRB, part, dpart)
  if (vec && cand)
    AS_CROSS(true, true);
  else if (vec)
    AS_CROSS(true, false);
  else if (cand)
    AS_CROSS(false, true);
  else
    AS_CROSS(false, false);
#undef AS_CROSS
  LAUNCH_CHECK();
  return hipSuccess;
}

// step 2 alone: P = panel_doubles doubles, from the n-vectors v and g
hipError_t launch_addscore_pack(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                                int q, int block, const double *vw, const double *gw, double *P, hipStream_t st) {
  if (!src || !vw || !gw || !P || n < 1 || n > 0x7fffffffLL || m < 0 || m + 1 > INFO_M_MAX || (m > 0 && !cols) ||
      rs < 0 || cs < 0 || q < 1 || block < 0 || block % 16)
    return hipErrorInvalidValue;
  const AsSplit sp = as_split(n, m + 1, q, block);
  return f32 ? as_launch_pack(static_cast<const float *>(src), rs, cs, n, cols, m + 1, vw, gw, sp, P, st)
             : as_launch_pack(static_cast<const double *>(src), rs, cs, n, cols, m + 1, vw, gw, sp, P, st);
}

// steps 3 to 5 for every block of candidates: cand = q ascending column numbers (device) or null = columns 0 .. q - 1;
// work = block_doubles doubles; pk = the packed factor already inside work's tail when with_stat (see addscore_split:
// the last diag_factor_doubles(m + 1) doubles of work); u, d, s, a: q doubles each; Cout: q x ldc or null.  Device
// memory.  only: 0 = all steps, 1 = cross, 2 = finish, 3 = statistic alone (bessx_op_addscore_bench's stages).
hipError_t launch_addscore_blocks(const void *src, int f32, long long rs, long long cs, long long n, int m, const int *cand,
                                  int q, int block, const double *P, double *work, int with_stat, double *u, double *d,
                                  double *s, double *a, double *Cout, long long ldc, int only, hipStream_t st) {
  if (!src || !P || !work || !u || !d || n < 1 || n > 0x7fffffffLL || m < 0 || m + 1 > INFO_M_MAX || rs < 0 || cs < 0 ||
      q < 1 || block < 0 || block % 16 || (with_stat && (!s || !a)) || (Cout && ldc < m + 1))
    return hipErrorInvalidValue;
  const int M = m + 1;
  const AsSplit sp = as_split(n, M, q, block);
  double *part = work, *dpart = part + (long long)sp.slabs * sp.TRB * sp.TP * 256;
  double *Cb = dpart + (long long)sp.slabs * sp.TRB * 16, *pk = Cb + (long long)sp.TRB * 16 * sp.TP * 16;
  const int step = sp.TRB * 16;
  for (int j0 = 0; j0 < q; j0 += step) {
    const int qb = std::min(step, q - j0), trb = (qb + 15) / 16;
    if (only == 0 || only == 1) {
      hipError_t e = f32 ? as_launch_cross(static_cast<const float *>(src), rs, cs, n, cand, j0, qb, P, sp, part, dpart, st)
                         : as_launch_cross(static_cast<const double *>(src), rs, cs, n, cand, j0, qb, P, sp, part, dpart, st);
      if (e != hipSuccess) return e;
    }
    if (only == 0 || only == 2) {
      hipLaunchKernelGGL(k_as_finish, dim3((unsigned)(trb * sp.TP), 4), dim3(256), 0, st, part, dpart, sp.slabs, sp.TRB,
                         sp.TP, M, j0, qb, Cb, u, d, Cout, ldc);
      LAUNCH_CHECK();
    }
    if (with_stat && (only == 0 || only == 3)) {
      hipLaunchKernelGGL(k_as_stat, dim3((unsigned)trb), dim3(64), 0, st, Cb, 16 * sp.TP, M, j0, qb, pk, s, a);
      LAUNCH_CHECK();
    }
  }
  return hipSuccess;
}

}  // namespace bessx
