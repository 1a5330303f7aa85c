// bessx_k_groupscore.hip -- Rao score tests of GROUPS of candidate columns against ONE fitted model (identity, logistic or
// Poisson link) on a caller's DEVICE matrix, read where it lies (include/bessx.h section 2n).  v, g, the panel P, u_j and
// the rows c_j of C are section 2l's, formed by the launchers of bessx_k_info.hip and bessx_k_addscore.hip as they are
// (launch_info_vg, launch_addscore_pack, launch_addscore_blocks: k_as_pack, k_as_cross, k_as_finish unchanged).  For a
// tested group with columns J (d = |J| <= 64) this unit adds the two d x d blocks
//     D = X_J^T diag(v) X_J                 S = (C_J R^T) (C_J R^T)^T                and a = C_J r.
// The tested columns of a block of candidates are tiled in their ascending order, 16 per tile, whatever the group
// boundaries are; a group of width d that starts in tile t ends in tile t + w at the latest, w = (d_max + 14) / 16 <= 4,
// so only the band tiles (t, t), ..., (t, t + w) of the block's Gram matrix are formed, NT = w + 1 per tile row.
//   k_gs_gram     the band of D on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  One wave per (tile row t, row slab);
//                 four waves = four neighbouring tile rows per workgroup, no LDS, no barrier.  Lane (c = lane & 15, q =
//                 lane >> 4) holds E consecutive rows of column 16 t + c per k group (E = 2 doubles or 4 floats: one
//                 16-byte load down an aligned column-contiguous source, element loads at any strides otherwise, where on
//                 a row-contiguous source the 16 lanes of a k slot read the list's neighbouring columns of one row).  That
//                 IS the A operand A[m = c][k = q]; the B operand B[k = q][n = c] of tile t + k is v_i times the same
//                 kind of load of column 16 (t + k) + c.  The diagonal tile multiplies the wave's own registers; the
//                 neighbouring tiles are loaded by the same wave the same way (a second read that the waves of the
//                 neighbouring tile rows, resident at the same time, have just made or are about to make).  The next
//                 chunk of GS_CH rows is loaded before the matrix instructions of the current one, without a guard where
//                 the whole chunk lies inside the view (a lane past the list reads the list's last column and is then
//                 set to zero), so that all of a chunk's loads are in flight together.  E depends on the
//                 element type alone: the arithmetic and its order are the same under every layout.  Rows >= n and
//                 list entries >= qb enter as exact zeros and are not read.  Entry (m, n) of tile (t, t + k) is
//                 sum_i x_i[16 t + m] * (v_i x_i[16 (t + k) + n]): above the diagonal always (earlier column) x (v x later
//                 column), whatever tile the pair falls into, so the bits do not depend on where a block starts.
//   k_gs_sum      adds the slabs' partials of every band tile in ascending slab order.
//   k_gs_t        T = C Rx^T per tile row of 16 candidates, k_as_stat's loop (diag_pack_factor's packing of R with r
//                 appended as row M, only the k-steps at or below each tile's diagonal), written out as rows of Mp doubles;
//                 column M of T is a_j.
//   k_gs_sband    the band tiles T_t T_{t+k}^T on the matrix cores over the columns < M of T in ascending k-steps; one wave
//                 per band tile, both operands 16-byte loads of rows of T (a block's T is a few MB and stays in cache).
//   k_gs_extract  copies every group's d x d block out of the band tiles: the upper triangle, mirrored.
// No floating-point atomics: the same call gives the same bits.  Index arithmetic in 64 bits.
#include <algorithm>

#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

constexpr int GS_CH = 32;          // rows per chunk of k_gs_gram (AS_CH of bessx_k_addscore.hip)
constexpr int GS_SLABS_MAX = 32;   // at most this many row slabs
constexpr int GS_NT_MAX = 5;       // band tiles per tile row at the widest group (64 columns from offset 15)
constexpr int GS_ACC = 16;         // output tiles per run of k_gs_t (AS_ACC)

// the lane's E rows i0 .. i0 + E - 1 of one column (exact zeros past n, which are not read)
template <typename T, bool VEC, int E>
__device__ __forceinline__ void gs_rows(const T *cp, long long rs, long long i0, long long n, double *x) {
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

// the same E rows where all of them lie inside the view: no guard, so that a chunk's loads all go out before the first
// of them is waited for
template <typename T, bool VEC, int E>
__device__ __forceinline__ void gs_rows_inside(const T *cp, long long rs, long long i0, double *x) {
  if constexpr (VEC) {
    pr_unpack(*reinterpret_cast<const typename PrVec<T>::type *>(cp + i0), x);
  } else {
#pragma unroll
    for (int e = 0; e < E; e++) x[e] = (double)cp[(i0 + e) * rs];
  }
}

}  // namespace

// grid (ceil(trb / 4), slabs); wave w of a workgroup is tile row 4 blockIdx.x + w.  cand: the block's qb list entries.
// part[((slab * trb + t) * NT + k) * 256 + reg * 64 + lane]
template <typename T, bool VEC, int NT>
__global__ void __launch_bounds__(256) k_gs_gram(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                 const int *__restrict__ cand, int qb, const double *__restrict__ vw,
                                                 long long rps, int trb, double *__restrict__ part) {
  constexpr int E = PrVec<T>::N, G = GS_CH / (4 * E);  // k groups per chunk: a group is 4 k slots x E rows
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
  const long long r_begin = (long long)slab * rps, r_end = min(n, r_begin + rps);
  const int nch = (int)((r_end - r_begin + GS_CH - 1) / GS_CH);
  d4 acc[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) acc[k] = d4{0.0, 0.0, 0.0, 0.0};
  double xa[NT][G][E], xn[NT][G][E], va[G][E], vn[G][E];
  auto load = [&](long long i0, double (*x)[G][E], double (*v)[E]) {
    if (i0 + GS_CH <= n) {  // (wave-uniform) the whole chunk lies inside the view: unguarded loads, then the column mask
#pragma unroll
      for (int g = 0; g < G; g++) {
        const long long i = i0 + g * (4 * E) + q * E;
#pragma unroll
        for (int e = 0; e < E; e++) v[g][e] = vw[i + e];
#pragma unroll
        for (int k = 0; k < NT; k++)
          if (k < nk) gs_rows_inside<T, VEC, E>(pc[k], rs, i, x[k][g]);
      }
#pragma unroll
      for (int k = 0; k < NT; k++)
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
          for (int e = 0; e < E; e++) x[k][g][e] = valid[k] ? x[k][g][e] : 0.0;
      return;
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      const long long i = i0 + g * (4 * E) + q * E;
#pragma unroll
      for (int e = 0; e < E; e++) v[g][e] = i + e < n ? vw[i + e] : 0.0;
#pragma unroll
      for (int k = 0; k < NT; k++) {
        if (valid[k]) {
          gs_rows<T, VEC, E>(pc[k], rs, i, n, x[k][g]);
        } else {
#pragma unroll
          for (int e = 0; e < E; e++) x[k][g][e] = 0.0;
        }
      }
    }
  };
  if (nch > 0) load(r_begin, xa, va);
  for (int ch = 0; ch < nch; ch++) {
    if (ch + 1 < nch) load(r_begin + (long long)(ch + 1) * GS_CH, xn, vn);
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
      for (int e = 0; e < E; e++)
#pragma unroll
        for (int k = 0; k < NT; k++)
          if (k < nk)  // (wave-uniform)
            acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[0][g][e], __dmul_rn(va[g][e], xa[k][g][e]), acc[k], 0, 0, 0);
    if (ch + 1 < nch) {
#pragma unroll
      for (int g = 0; g < G; g++)
#pragma unroll
        for (int e = 0; e < E; e++) {
          va[g][e] = vn[g][e];
#pragma unroll
          for (int k = 0; k < NT; k++) xa[k][g][e] = xn[k][g][e];
        }
    }
  }
#pragma unroll
  for (int k = 0; k < NT; k++) {
    if (k < nk) {
      double *o = part + (((long long)slab * trb + tr) * NT + k) * 256 + lane;
      o[0] = acc[k].x;
      o[64] = acc[k].y;
      o[128] = acc[k].z;
      o[192] = acc[k].w;
    }
  }
}

// block = band tile (t, t + k), thread = entry: the slabs in ascending order
__global__ void __launch_bounds__(256) k_gs_sum(const double *__restrict__ part, int slabs, int trb, int NT,
                                                double *__restrict__ band) {
  const int tr = (int)blockIdx.x / NT, k = (int)blockIdx.x % NT;
  if (tr + k >= trb) return;
  double s = 0.0;
  for (int sl = 0; sl < slabs; sl++) s += part[(((long long)sl * trb + tr) * NT + k) * 256 + threadIdx.x];
  band[(long long)blockIdx.x * 256 + threadIdx.x] = s;
}

// one wave per tile row of 16 candidates: k_as_stat's products, written out.  Cb, Tb: rows of Mp doubles.
__global__ void __launch_bounds__(64) k_gs_t(const double *__restrict__ Cb, int Mp, int M, int qb,
                                             const double *__restrict__ pk, double *__restrict__ Tb,
                                             double *__restrict__ o_a) {
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const int TI = Mp / 16, JM = M / 16, cM = M % 16;  // column M of T, the dot product with r, is column cM of tile JM
  const double *row = Cb + ((long long)blockIdx.x * 16 + c) * Mp;
  const int jb = (int)blockIdx.x * 16 + q;
  for (int J0 = 0; J0 < TI; J0 += GS_ACC) {
    const int nJ = min(GS_ACC, TI - J0);
    d4 acc[GS_ACC];
#pragma unroll
    for (int jj = 0; jj < GS_ACC; jj++) acc[jj] = d4{0.0, 0.0, 0.0, 0.0};
    const int ksteps = 4 * (J0 + nJ);
    for (int k0 = 0; k0 < ksteps; k0 += 2) {
      double xa[2], b[2][GS_ACC];
#pragma unroll
      for (int uu = 0; uu < 2; uu++) {
        const int k = 4 * (k0 + uu) + q;
        xa[uu] = k < M ? row[k] : 0.0;
      }
#pragma unroll
      for (int jj = 0; jj < GS_ACC; jj++) {
        const int J = J0 + jj;
        if (jj < nJ && k0 < 4 * (J + 1)) {  // (wave-uniform)
#pragma unroll
          for (int uu = 0; uu < 2; uu++) b[uu][jj] = pk[((long long)2 * J * (J + 1) + k0 + uu) * 64 + lane];
        }
      }
#pragma unroll
      for (int jj = 0; jj < GS_ACC; jj++) {
        if (jj < nJ && k0 < 4 * (J0 + jj + 1)) {
#pragma unroll
          for (int uu = 0; uu < 2; uu++)  // (a tile's k-steps in ascending order)
            acc[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[uu], b[uu][jj], acc[jj], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < GS_ACC; jj++) {
      if (jj < nJ) {  // register r of lane (c, q) is candidate q + 4 r, column 16 J + c
        const d4 t = acc[jj];
        const double tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int r = 0; r < 4; r++) {
          Tb[((long long)blockIdx.x * 16 + q + 4 * r) * Mp + 16 * (J0 + jj) + c] = tv[r];
          if (J0 + jj == JM && c == cM && jb + 4 * r < qb) o_a[jb + 4 * r] = tv[r];
        }
      }
    }
  }
}

// one wave per band tile (t, t + k): lane (c, q) takes columns 8 s + 2 q and + 1 of T's rows 16 t + c and 16 (t + k) + c
__global__ void __launch_bounds__(64) k_gs_sband(const double *__restrict__ Tb, int Mp, int M, int trb, int NT,
                                                 double *__restrict__ band) {
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const int tr = (int)blockIdx.x / NT, k = (int)blockIdx.x % NT;
  if (tr + k >= trb) return;
  const double *ra = Tb + ((long long)tr * 16 + c) * Mp, *rb = Tb + ((long long)(tr + k) * 16 + c) * Mp;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < M; k0 += 8) {  // (M <= Mp - 1 and Mp is a multiple of 16: the loads stay inside the row)
    const int kk = k0 + 2 * q;
    d2 a = *reinterpret_cast<const d2 *>(ra + kk), b = *reinterpret_cast<const d2 *>(rb + kk);
    if (kk >= M) a.x = 0.0, b.x = 0.0;  // (column M of T is a_j and is not an entry of the product)
    if (kk + 1 >= M) a.y = 0.0, b.y = 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, acc, 0, 0, 0);
  }
  double *o = band + (long long)blockIdx.x * 256 + lane;
  o[0] = acc.x;
  o[64] = acc.y;
  o[128] = acc.z;
  o[192] = acc.w;
}

// block = tested group g0 + blockIdx.x of the block of candidates that starts at list position lpos[g0].  Entry (i, j),
// i <= j, of the group's block is entry (li & 15, lj & 15) of band tile (li >> 4, lj >> 4): register (li & 15) >> 2 of
// lane 16 ((li & 15) & 3) + (lj & 15).  Written to (i, j) and (j, i).
__global__ void __launch_bounds__(256) k_gs_extract(const double *__restrict__ band, int NT, const int *__restrict__ lpos,
                                                    const long long *__restrict__ offs, int g0,
                                                    double *__restrict__ out) {
  const int g = g0 + (int)blockIdx.x, lo = lpos[g] - lpos[g0], d = lpos[g + 1] - lpos[g];
  double *o = out + offs[g];
  for (int e = threadIdx.x; e < d * d; e += 256) {
    const int i = e / d, j = e % d;
    if (i > j) continue;
    const int li = lo + i, lj = lo + j, t = li >> 4, k = (lj >> 4) - t, mm = li & 15, cc = lj & 15;
    const double v = band[((long long)t * NT + k) * 256 + (mm >> 2) * 64 + (mm & 3) * 16 + cc];
    o[(long long)i * d + j] = v;
    o[(long long)j * d + i] = v;
  }
}

// the band width w of a widest tested group of dmax columns
int groupscore_band(int dmax) { return (dmax + 14) / 16; }

// the row split of k_gs_gram, a function of n alone
void groupscore_rows(long long n, long long *rows_per_slab, int *slabs) {
  const long long rps = ((n + GS_SLABS_MAX - 1) / GS_SLABS_MAX + GS_CH - 1) / GS_CH * GS_CH;
  *rows_per_slab = rps;
  *slabs = (int)((n + rps - 1) / rps);
}

// the cut of the tested groups (widths d[0 .. nt - 1], each <= block) into blocks of at most `block` columns that hold
// whole groups: first[b] = the first group of block b, first[blocks] = nt; returns the number of blocks
int groupscore_cut(const int *d, int nt, int block, int *first) {
  int nb = 0, cnt = 0;
  for (int g = 0; g < nt; g++) {
    if (g == 0 || cnt + d[g] > block) {
      first[nb++] = g;
      cnt = 0;
    }
    cnt += d[g];
  }
  first[nb] = nt;
  return nb;
}

// doubles of this unit's own workspace for blocks of at most qmax columns: the partials and the band of D, the band of
// S, the block's rows of C and of T, and LAST the packed factor (diag_factor_doubles(m + 1) doubles)
long long groupscore_doubles(long long n, int m, int qmax, int band) {
  long long rps = 0;
  int slabs = 0;
  groupscore_rows(n, &rps, &slabs);
  const long long trb = (qmax + 15) / 16, NT = band + 1, Mp = 16LL * ((m + 2 + 15) / 16);
  return (slabs + 2) * trb * NT * 256 + 2 * trb * 16 * Mp + diag_factor_doubles(m + 1);
}

template <typename T>
static hipError_t gs_launch_gram(const T *src, long long rs, long long cs, long long n, const int *cand, int qb, int NT,
                                 const double *vw, long long rps, int slabs, double *part, hipStream_t st) {
  const long long per16 = 16 / (long long)sizeof(T);
  const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
  const int trb = (qb + 15) / 16;
  const dim3 grid((unsigned)((trb + 3) / 4), (unsigned)slabs);
#define GS_GRAM(V, N)                                                                                                  \
  hipLaunchKernelGGL((k_gs_gram<T, V, N>), grid, dim3(256), 0, st, src, rs, cs, n, cand, qb, vw, rps, trb, part)
#define GS_GRAM_NT(V)                                                                                                  \
  switch (NT) {                                                                                                        \
    case 1: GS_GRAM(V, 1); break;                                                                                      \
    case 2: GS_GRAM(V, 2); break;                                                                                      \
    case 3: GS_GRAM(V, 3); break;                                                                                      \
    case 4: GS_GRAM(V, 4); break;                                                                                      \
    default: GS_GRAM(V, 5); break;                                                                                     \
  }
  if (vec) {
    GS_GRAM_NT(true)
  } else {
    GS_GRAM_NT(false)
  }
#undef GS_GRAM_NT
#undef GS_GRAM
  LAUNCH_CHECK();
  return hipSuccess;
}

// the band of D for one block of candidates: cand = the block's qb ascending columns (device), band = w, vw = the n row
// weights, work = groupscore_doubles' workspace (the partials first, then the band of D).  only: 0 = both kernels, 1 =
// k_gs_gram, 2 = k_gs_sum alone (bessx_op_groupscore_bench's stages).  Device memory.
hipError_t launch_groupscore_gram(const void *src, int f32, long long rs, long long cs, long long n, const int *cand,
                                  int qb, int band, const double *vw, double *work, int only, hipStream_t st) {
  if (!src || !cand || !vw || !work || n < 1 || n > 0x7fffffffLL || rs < 0 || cs < 0 || qb < 1 || band < 0 ||
      band + 1 > GS_NT_MAX)
    return hipErrorInvalidValue;
  long long rps = 0;
  int slabs = 0;
  groupscore_rows(n, &rps, &slabs);
  const int NT = band + 1, trb = (qb + 15) / 16;
  double *part = work, *bandD = work + (long long)slabs * trb * NT * 256;
  if (only == 0 || only == 1) {
    hipError_t e = f32 ? gs_launch_gram(static_cast<const float *>(src), rs, cs, n, cand, qb, NT, vw, rps, slabs, part, st)
                       : gs_launch_gram(static_cast<const double *>(src), rs, cs, n, cand, qb, NT, vw, rps, slabs, part, st);
    if (e != hipSuccess) return e;
  }
  if (only == 0 || only == 2) {
    hipLaunchKernelGGL(k_gs_sum, dim3((unsigned)(trb * NT)), dim3(256), 0, st, part, slabs, trb, NT, bandD);
    LAUNCH_CHECK();
  }
  return hipSuccess;
}

// the band of S and a for one block: Cb = the block's rows of C (16 ceil(qb / 16) rows of Mp doubles, Mp = 16 ceil((m +
// 2) / 16); rows past qb and columns >= m + 1 zeros), pk = addscore_pack_factor's packing, Tb = as many doubles as Cb,
// bandS = ceil(qb / 16) * (band + 1) * 256 doubles, a = qb doubles.  Device memory.
hipError_t launch_groupscore_sband(const double *Cb, int m, int qb, int band, const double *pk, double *Tb, double *bandS,
                                   double *a, hipStream_t st) {
  if (!Cb || !pk || !Tb || !bandS || !a || m < 0 || m + 1 > INFO_M_MAX || qb < 1 || band < 0 || band + 1 > GS_NT_MAX)
    return hipErrorInvalidValue;
  const int M = m + 1, Mp = 16 * ((M + 1 + 15) / 16), trb = (qb + 15) / 16, NT = band + 1;
  hipLaunchKernelGGL(k_gs_t, dim3((unsigned)trb), dim3(64), 0, st, Cb, Mp, M, qb, pk, Tb, a);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gs_sband, dim3((unsigned)(trb * NT)), dim3(64), 0, st, Tb, Mp, M, trb, NT, bandS);
  LAUNCH_CHECK();
  return hipSuccess;
}

// every group g0 .. g0 + ng - 1 of one block out of a band (of D or of S) into out + offs[g]; lpos: the list position of
// every tested group's first column (and the list's length last), offs: where its block starts.  Device memory.
hipError_t launch_groupscore_extract(const double *bandT, int band, const int *lpos, const long long *offs, int g0, int ng,
                                     double *out, hipStream_t st) {
  if (!bandT || !lpos || !offs || !out || g0 < 0 || ng < 1 || band < 0 || band + 1 > GS_NT_MAX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gs_extract, dim3((unsigned)ng), dim3(256), 0, st, bandT, band + 1, lpos, offs, g0, out);
  LAUNCH_CHECK();
  return hipSuccess;
}

}  // namespace bessx
