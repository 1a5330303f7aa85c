// bessx_k_xb.hpp -- the one copy of the loops that form eta = X[:, cols] B + c on a caller's DEVICE matrix, shared by
// prediction (bessx_k_predict.hip: the epilogue stores link(eta)) and evaluation (bessx_k_eval.hip: the epilogue turns
// eta into a weighted loss term and reduces it over the workgroup's rows).  X is fp64 or fp32 with arbitrary
// non-negative element strides and is read where it lies, only the m support columns of it: n * m elements instead of
// n * p.  fp32 is widened in registers (exact).  Two kernels:
//   k_xb_rows     threads along rows.  A workgroup owns 64 * N rows (N = elements of a 16-byte load); its four
//                 waves split every chunk of 64 support columns between them and their partial sums are added in
//                 wave order through LDS.  B is staged in LDS chunk by chunk.  VEC: column-contiguous source with an
//                 aligned base and column stride, one 16-byte load per column; otherwise element loads at any strides
//                 (coalesced when row_stride == 1) -- the same arithmetic in the same order.
//   k_xb_gather   row-contiguous source (col_stride == 1): the support is split across the lanes of a wave (LPR = 64)
//                 or of a quarter wave (LPR = 16, short supports); a lane keeps its columns' rows of B in registers
//                 while the wave walks its rows, and the lanes' partial sums are added by a DPP tree (+ three
//                 additions in lane order for LPR = 64).
// Both take RT responses per workgroup (blockIdx.y walks the tiles of a wide R) and loop over the support in chunks: no
// LDS or register array is sized by m or R.  Every sum has a fixed order and there are no atomics: a call repeats bit for
// bit.  Index arithmetic is in 64 bits.  Columns outside the support are not read.
//
// The epilogue Epi (passed by value) is one of two kinds:
//   Epi::REDUCE == false   epi.store(eta, i, r) for every row i < n and response r < R.
//   Epi::REDUCE == true    epi.term(eta, i, r, s, a) adds row i's terms of response r to s (and a); the kernel adds the
//                          workgroup's rows in a fixed order and calls epi.put(blockIdx.x, r, s, a) once per response:
//                          one partial per workgroup and response, to be added in a fixed order by a second launch.
//   Epi::SKIPZ == true     a coefficient that is exactly zero takes nothing from its column: a NaN or inf there does
//                          not reach that response (x * 0 would be NaN).  The sums are the same bits otherwise.
#ifndef BESSX_K_XB_HPP
#define BESSX_K_XB_HPP
#include "bessx_kdev.hpp"

namespace bessx {

namespace {

constexpr int PR_CH = 64;  // support columns staged per chunk of k_xb_rows
constexpr int PR_KPL = 2;  // support columns per lane and chunk of k_xb_gather

template <typename T>
struct PrVec;
template <>
struct PrVec<double> {
  static constexpr int N = 2;  // elements per 16-byte load
  typedef d2 type;
};
template <>
struct PrVec<float> {
  static constexpr int N = 4;
  typedef float4 type;
};

__device__ inline void pr_unpack(const d2 &v, double *o) {
  o[0] = v.x;
  o[1] = v.y;
}
__device__ inline void pr_unpack(const float4 &v, double *o) {
  o[0] = (double)v.x;
  o[1] = (double)v.y;
  o[2] = (double)v.z;
  o[3] = (double)v.w;
}

// sum over the LPR lanes of a lane group, the same bits in every lane of the group: four symmetric DPP exchanges inside
// each row of 16 lanes, then (LPR = 64) the four rows in lane order
template <int LPR>
__device__ __forceinline__ double pr_group_sum(double v) {
#pragma unroll
  for (int st = 0; st < 4; st++) v += dpp_f64(v, st);
  if (LPR == 64) v = ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
  return v;
}

// x as it enters x * b (see Epi::SKIPZ)
template <bool SKIPZ>
__device__ __forceinline__ double pr_x_for(double x, double b) {
  return (SKIPZ && b == 0.0) ? 0.0 : x;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// threads along rows: block (row block, response tile).  Lane l of every wave owns rows (blockIdx.x * 64 + l) * N ..
// + N - 1; wave w takes columns w, w + 4, ... of each chunk, four of them in flight per step.  REDUCE: wave 0, which
// holds the finished eta of all the block's rows, adds a lane's N rows in row order and the 64 lanes by pr_group_sum.
// ------------------------------------------------------------------------------------------
template <typename T, int RT, bool VEC, typename Epi>
__global__ void __launch_bounds__(256) k_xb_rows(const T *__restrict__ src, long long rs, long long cs, long long n,
                                                 const int *__restrict__ cols, int m, const double *__restrict__ B,
                                                 const double *__restrict__ c, int R, const Epi epi) {
  constexpr int N = PrVec<T>::N;
  typedef typename PrVec<T>::type V;
  __shared__ double Bs[PR_CH * RT];
  __shared__ int Cs[PR_CH];
  __shared__ double red[3][N * RT][64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const long long i0 = ((long long)blockIdx.x * 64 + lane) * N;
  const int r0 = (int)blockIdx.y * RT;
  double acc[N][RT];
#pragma unroll
  for (int e = 0; e < N; e++)
#pragma unroll
    for (int r = 0; r < RT; r++) acc[e][r] = 0.0;
  for (int k0 = 0; k0 < m; k0 += PR_CH) {
    const int kc = min(PR_CH, m - k0);
    __syncthreads();
    for (int q = t; q < kc * RT; q += 256) {
      const int j = q / RT, r = q % RT;
      Bs[q] = (r0 + r < R) ? B[(long long)(k0 + j) * R + r0 + r] : 0.0;
    }
    if (t < kc) Cs[t] = cols[k0 + t];
    __syncthreads();
    for (int j0 = w; j0 < kc; j0 += 16) {
      double x[4][N];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = j0 + 4 * u;
#pragma unroll
        for (int e = 0; e < N; e++) x[u][e] = 0.0;
        if (j < kc) {  // (wave-uniform; a column past the chunk is not read: its NaN must not reach the sum)
          const T *cp = src + (long long)Cs[j] * cs;
          if (VEC && i0 + N <= n) {
            pr_unpack(*reinterpret_cast<const V *>(cp + i0), x[u]);
          } else {
#pragma unroll
            for (int e = 0; e < N; e++)
              if (i0 + e < n) x[u][e] = (double)cp[(i0 + e) * rs];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = j0 + 4 * u;
        if (j < kc) {
#pragma unroll
          for (int r = 0; r < RT; r++) {
            const double b = Bs[j * RT + r];
#pragma unroll
            for (int e = 0; e < N; e++) acc[e][r] += pr_x_for<Epi::SKIPZ>(x[u][e], b) * b;
          }
        }
      }
    }
  }
  if (w > 0) {
#pragma unroll
    for (int e = 0; e < N; e++)
#pragma unroll
      for (int r = 0; r < RT; r++) red[w - 1][e * RT + r][lane] = acc[e][r];
  }
  __syncthreads();
  if (w == 0) {
    if constexpr (Epi::REDUCE) {
#pragma unroll
      for (int r = 0; r < RT; r++) {
        double s = 0.0, a = 0.0;
#pragma unroll
        for (int e = 0; e < N; e++) {
          const long long i = i0 + e;
          if (i < n && r0 + r < R) {
            const int q = e * RT + r;
            const double eta = (((acc[e][r] + red[0][q][lane]) + red[1][q][lane]) + red[2][q][lane]) + c[r0 + r];
            epi.term(eta, i, r0 + r, s, a);
          }
        }
        s = pr_group_sum<64>(s);
        a = pr_group_sum<64>(a);
        if (lane == 0 && r0 + r < R) epi.put((long long)blockIdx.x, r0 + r, s, a);
      }
    } else {
#pragma unroll
      for (int e = 0; e < N; e++) {
        const long long i = i0 + e;
#pragma unroll
        for (int r = 0; r < RT; r++) {
          if (i < n && r0 + r < R) {
            const int a = e * RT + r;
            const double eta = (((acc[e][r] + red[0][a][lane]) + red[1][a][lane]) + red[2][a][lane]) + c[r0 + r];
            epi.store(eta, i, r0 + r);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// row-contiguous source: block (row block, response tile), no LDS for the sums of eta.  A wave owns 64 / RT rows and
// works on G = 64 / LPR of them at a time, one per lane group, in S = LPR / RT steps.  Lane lg of a group gathers columns
// k0 + lg and k0 + LPR + lg of the chunk for its group's row; lane lg of group g keeps the finished sum of row
// (lg / RT) * G + g, response lg % RT, so the wave's 64 results are one register.  REDUCE: per response, the wave's rows
// are added by pr_group_sum over the lanes that hold it and the four waves in wave order through LDS.
// ------------------------------------------------------------------------------------------
template <typename T, int RT, int LPR, typename Epi>
__global__ void __launch_bounds__(256) k_xb_gather(const T *__restrict__ src, long long rs, long long n,
                                                   const int *__restrict__ cols, int m, const double *__restrict__ B,
                                                   const double *__restrict__ c, int R, const Epi epi) {
  constexpr int G = 64 / LPR, S = LPR / RT, RPW = 64 / RT;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, g = lane / LPR, lg = lane % LPR;
  const long long row0 = ((long long)blockIdx.x * 4 + w) * RPW;
  const int r0 = (int)blockIdx.y * RT;
  double eta = 0.0;
  for (int k0 = 0; k0 < m; k0 += LPR * PR_KPL) {
    long long col[PR_KPL];
    bool ok[PR_KPL];
    double b[PR_KPL][RT];
#pragma unroll
    for (int u = 0; u < PR_KPL; u++) {
      const int k = k0 + u * LPR + lg;
      ok[u] = k < m;
      col[u] = ok[u] ? (long long)cols[k] : 0;
#pragma unroll
      for (int r = 0; r < RT; r++) b[u][r] = (ok[u] && r0 + r < R) ? B[(long long)k * R + r0 + r] : 0.0;
    }
#pragma unroll 2
    for (int s = 0; s < S; s++) {
      const long long i = row0 + s * G + g;
      double x[PR_KPL];
#pragma unroll
      for (int u = 0; u < PR_KPL; u++) x[u] = (ok[u] && i < n) ? (double)src[i * rs + col[u]] : 0.0;
#pragma unroll
      for (int r = 0; r < RT; r++) {
        double part = pr_x_for<Epi::SKIPZ>(x[0], b[0][r]) * b[0][r];
#pragma unroll
        for (int u = 1; u < PR_KPL; u++) part += pr_x_for<Epi::SKIPZ>(x[u], b[u][r]) * b[u][r];
        part = pr_group_sum<LPR>(part);
        if (lg == s * RT + r) eta += part;
      }
    }
  }
  const long long i = row0 + (lg / RT) * G + g;
  const int r = r0 + lg % RT;
  if constexpr (Epi::REDUCE) {
    __shared__ double wsum[2][4][RT];
    double s = 0.0, a = 0.0;
    if (i < n && r < R) epi.term(eta + c[r], i, r, s, a);
#pragma unroll
    for (int q = 0; q < RT; q++) {
      const bool mine = lg % RT == q;
      const double sq = pr_group_sum<64>(mine ? s : 0.0), aq = pr_group_sum<64>(mine ? a : 0.0);
      if (lane == 0) {
        wsum[0][w][q] = sq;
        wsum[1][w][q] = aq;
      }
    }
    __syncthreads();
    if (t < RT && r0 + t < R)
      epi.put((long long)blockIdx.x, r0 + t, ((wsum[0][0][t] + wsum[0][1][t]) + wsum[0][2][t]) + wsum[0][3][t],
              ((wsum[1][0][t] + wsum[1][1][t]) + wsum[1][2][t]) + wsum[1][3][t]);
  } else {
    if (i < n && r < R) epi.store(eta + c[r], i, r);
  }
}

// rows of the source one workgroup of the kernel that xb_launch_rt picks takes: the grid's x extent is
// ceil(n / xb_rows_per_block), which is also the number of partials per response a REDUCE epilogue writes
template <typename T, int RT>
static long long xb_rows_per_block(long long rs, long long cs, int m) {
  return (cs == 1 && rs != 1 && m > 0) ? 4LL * (64 / RT) : 64LL * PrVec<T>::N;
}

template <typename T, int RT, typename Epi>
static hipError_t xb_launch_rt(const T *src, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *B, const double *c, int R, const Epi &epi, hipStream_t st) {
  const unsigned tiles = (unsigned)((R + RT - 1) / RT);
  if (tiles > 65535) return hipErrorInvalidValue;
  const long long rows_per_block = xb_rows_per_block<T, RT>(rs, cs, m);
  const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block), tiles);
  if (cs == 1 && rs != 1 && m > 0) {
    if (m <= 16 * PR_KPL)
      hipLaunchKernelGGL((k_xb_gather<T, RT, 16, Epi>), grid, dim3(256), 0, st, src, rs, n, cols, m, B, c, R, epi);
    else
      hipLaunchKernelGGL((k_xb_gather<T, RT, 64, Epi>), grid, dim3(256), 0, st, src, rs, n, cols, m, B, c, R, epi);
  } else {
    const long long per16 = 16 / (long long)sizeof(T);
    const bool vec = rs == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && cs % per16 == 0;
    if (vec)
      hipLaunchKernelGGL((k_xb_rows<T, RT, true, Epi>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, c, R, epi);
    else
      hipLaunchKernelGGL((k_xb_rows<T, RT, false, Epi>), grid, dim3(256), 0, st, src, rs, cs, n, cols, m, B, c, R, epi);
  }
  LAUNCH_CHECK();
  return hipSuccess;
}

// the response tile for R responses: 1, 4 or 8
static inline int xb_tile(int R) { return R == 1 ? 1 : (R <= 4 ? 4 : 8); }

template <typename T, typename Epi>
static hipError_t xb_launch(const T *src, long long rs, long long cs, long long n, const int *cols, int m,
                            const double *B, const double *c, int R, const Epi &epi, hipStream_t st) {
  if (R == 1) return xb_launch_rt<T, 1>(src, rs, cs, n, cols, m, B, c, R, epi, st);
  if (R <= 4) return xb_launch_rt<T, 4>(src, rs, cs, n, cols, m, B, c, R, epi, st);
  return xb_launch_rt<T, 8>(src, rs, cs, n, cols, m, B, c, R, epi, st);
}

}  // namespace bessx
#endif  // BESSX_K_XB_HPP
