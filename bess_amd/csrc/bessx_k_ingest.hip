// bessx_k_ingest.hip -- device ingest: fill the session's zero-padded column-major fp64 matrix from a caller's DEVICE
// matrix of fp64 or fp32 elements with arbitrary non-negative element strides (+ launcher).  Three kernels:
//   k_ingest_col   column-contiguous source, aligned: streaming copy, 16-byte loads and stores
//   k_ingest_tr    row-contiguous source: 64 x 64 tiles transposed through LDS, optional row order
//   k_ingest_any   everything else (odd bases / strides, views with two non-unit strides, a row order on a
//                  column-contiguous source): element loads, 16-byte stores along the destination column
// Every kernel writes rows n..ld-1 of its columns as zeros, widens fp32 in registers (exact), raises *nan_flag when it
// meets a NaN (plain store of a constant) and does its index arithmetic in 64 bits.  ld is a multiple of 128.
#include "bessx_kdev.hpp"

namespace bessx {

namespace {

constexpr int ING_ITER = 4;  // independent 16-byte loads per thread of the streaming kernels

template <typename T>
struct IngVec;
template <>
struct IngVec<double> {
  static constexpr int N = 2;  // elements per 16-byte load
  typedef d2 type;
};
template <>
struct IngVec<float> {
  static constexpr int N = 4;
  typedef float4 type;
};

__device__ inline void ing_unpack(const d2 &v, double *o) {
  o[0] = v.x;
  o[1] = v.y;
}
__device__ inline void ing_unpack(const float4 &v, double *o) {
  o[0] = (double)v.x;
  o[1] = (double)v.y;
  o[2] = (double)v.z;
  o[3] = (double)v.w;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// column-contiguous, aligned (base and col_stride * sizeof(T) multiples of 16): block (j, chunk) streams
// 256 * N * ING_ITER rows of column j; a thread moves N consecutive rows per step: one 16-byte load, N/2 16-byte stores
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_ingest_col(const T *__restrict__ src, long long cs, long long n,
                                                    double *__restrict__ X, long long ld,
                                                    unsigned *__restrict__ nan_flag) {
  constexpr int N = IngVec<T>::N;
  typedef typename IngVec<T>::type V;
  const long long j = blockIdx.x;
  const T *c = src + j * cs;
  double *o = X + j * ld;
  const long long base = (long long)blockIdx.y * (256LL * N * ING_ITER) + (long long)threadIdx.x * N;
  double v[ING_ITER][N];
#pragma unroll
  for (int u = 0; u < ING_ITER; u++) {
    const long long i0 = base + (long long)u * (256 * N);
    if (i0 + N <= n) {
      ing_unpack(*reinterpret_cast<const V *>(c + i0), v[u]);
    } else {
#pragma unroll
      for (int e = 0; e < N; e++) v[u][e] = (i0 + e < n) ? (double)c[i0 + e] : 0.0;
    }
  }
  bool bad = false;
#pragma unroll
  for (int u = 0; u < ING_ITER; u++) {
    const long long i0 = base + (long long)u * (256 * N);
    if (i0 < ld) {  // ld is a multiple of 128 and N divides it: i0 < ld means i0 + N <= ld
#pragma unroll
      for (int e = 0; e < N; e += 2) {
        bad |= (v[u][e] != v[u][e]) | (v[u][e + 1] != v[u][e + 1]);
        d2 w;
        w.x = v[u][e];
        w.y = v[u][e + 1];
        *reinterpret_cast<d2 *>(o + i0 + e) = w;
      }
    }
  }
  if (bad) *nan_flag = 1u;
}

// ------------------------------------------------------------------------------------------
// any strides: block (j, chunk), a thread moves two consecutive destination rows per step with element loads
// (coalesced 8- / 4-byte loads when row_stride == 1) and one 16-byte store
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_ingest_any(const T *__restrict__ src, long long rs, long long cs,
                                                    const int *__restrict__ order, long long n,
                                                    double *__restrict__ X, long long ld,
                                                    unsigned *__restrict__ nan_flag) {
  const long long j = blockIdx.x;
  const T *c = src + j * cs;
  double *o = X + j * ld;
  const long long base = (long long)blockIdx.y * (512LL * ING_ITER) + (long long)threadIdx.x * 2;
  double v[ING_ITER][2];
#pragma unroll
  for (int u = 0; u < ING_ITER; u++) {
    const long long i0 = base + (long long)u * 512;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const long long i = i0 + e;
      double x = 0.0;
      if (i < n) {
        const long long r = order ? (long long)order[i] : i;
        x = (double)c[r * rs];
      }
      v[u][e] = x;
    }
  }
  bool bad = false;
#pragma unroll
  for (int u = 0; u < ING_ITER; u++) {
    const long long i0 = base + (long long)u * 512;
    if (i0 < ld) {
      bad |= (v[u][0] != v[u][0]) | (v[u][1] != v[u][1]);
      d2 w;
      w.x = v[u][0];
      w.y = v[u][1];
      *reinterpret_cast<d2 *>(o + i0) = w;
    }
  }
  if (bad) *nan_flag = 1u;
}

// ------------------------------------------------------------------------------------------
// row-contiguous (col_stride == 1): one 64 x 64 tile per block.
//   load   a lane takes N = 16 / sizeof(T) consecutive columns of one source row (one 16-byte load when `wide`: base and
//          row_stride * sizeof(T) multiples of 16); a wave instruction covers whole 512-byte (fp64) / 256-byte (fp32)
//          row segments
//   LDS    the tile as doubles, column j contiguous over rows: element (i, j) at j * 64 + ((i + 2 * (j / N)) & 63).
//          The rotation is even, so rows (2q, 2q+1) stay one aligned 16-byte slot.
//          store side: ds_write_b64 is served in groups of 16 contiguous lanes over 32 banks; a group is 8 column
//          groups x 2 rows, whose 8-byte slots (i + di + 2 * jl) mod 16 are all different: no conflict.
//          read side: a lane reads rows (2q, 2q+1) of column j with one ds_read_b128; a half wave reads the 32 slots
//          of one column, and every 16-lane service group of that instruction hits 16 different slots mod 16.
//   store  a lane writes two consecutive rows of a destination column (16 bytes); a half wave covers 512 contiguous bytes.
// Rows n..ld-1 arrive as zeros through the same path (the row tiles cover ld, a multiple of 64).
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_ingest_tr(const T *__restrict__ src, long long rs,
                                                   const int *__restrict__ order, long long n, long long p,
                                                   double *__restrict__ X, long long ld, int wide,
                                                   unsigned *__restrict__ nan_flag) {
  constexpr int N = IngVec<T>::N;
  typedef typename IngVec<T>::type V;
  constexpr int LPR = 64 / N;          // lanes per tile row
  constexpr int RPP = 2 * (256 / (2 * LPR));  // tile rows per pass
  constexpr int PASSES = 64 / RPP;
  __shared__ __attribute__((aligned(16))) double tile[64 * 64];
  const long long bj = (long long)blockIdx.x * 64, bi = (long long)blockIdx.y * 64;
  const int t = threadIdx.x;
  const int jl = t & 7, di = (t >> 3) & 1, jh = (t >> 4) & (LPR / 8 - 1);
  const int jq = jh * 8 + jl;                 // column group of this lane: columns jq * N .. jq * N + N - 1
  const int r0 = (t / (2 * LPR)) * 2 + di;    // tile row of this lane in pass 0
  const long long j0 = bj + (long long)jq * N;
  double v[PASSES][N];
#pragma unroll
  for (int u = 0; u < PASSES; u++) {
    const long long i = bi + r0 + u * RPP;
#pragma unroll
    for (int e = 0; e < N; e++) v[u][e] = 0.0;
    if (i < n && j0 < p) {
      const long long r = order ? (long long)order[i] : i;
      const T *q = src + r * rs + j0;
      if (wide && j0 + N <= p) {
        ing_unpack(*reinterpret_cast<const V *>(q), v[u]);
      } else {
#pragma unroll
        for (int e = 0; e < N; e++)
          if (j0 + e < p) v[u][e] = (double)q[e];
      }
    }
  }
  bool bad = false;
#pragma unroll
  for (int u = 0; u < PASSES; u++) {
    const int i = r0 + u * RPP;
#pragma unroll
    for (int e = 0; e < N; e++) {
      bad |= v[u][e] != v[u][e];
      tile[(jq * N + e) * 64 + ((i + 2 * jq) & 63)] = v[u][e];
    }
  }
  if (bad) *nan_flag = 1u;
  __syncthreads();
  const int q2 = t & 31;  // rows 2 * q2, 2 * q2 + 1
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int jt = (t >> 5) + u * 8;
    const long long j = bj + jt;
    const d2 w = *reinterpret_cast<const d2 *>(&tile[jt * 64 + ((2 * q2 + 2 * (jt / N)) & 63)]);
    if (j < p) *reinterpret_cast<d2 *>(X + j * ld + bi + 2 * q2) = w;
  }
}

template <typename T>
static hipError_t launch_ingest_t(const T *src, long long rs, long long cs, const int *order, long long n,
                                  long long p, double *X, long long ld, unsigned *nan_flag, hipStream_t st) {
  const bool base16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const long long per16 = 16 / (long long)sizeof(T);
  if (rs == 1 && !order && base16 && cs % per16 == 0) {
    const long long rows_per_block = 256LL * IngVec<T>::N * ING_ITER;
    const long long gy = (ld + rows_per_block - 1) / rows_per_block;
    if (gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ingest_col<T>, dim3((unsigned)p, (unsigned)gy), dim3(256), 0, st, src, cs, n, X, ld, nan_flag);
  } else if (cs == 1 && rs != 1) {
    if (ld / 64 > 65535) return hipErrorInvalidValue;
    const int wide = base16 && rs % per16 == 0;
    hipLaunchKernelGGL(k_ingest_tr<T>, dim3((unsigned)((p + 63) / 64), (unsigned)(ld / 64)), dim3(256), 0, st, src, rs,
                       order, n, p, X, ld, wide, nan_flag);
  } else {
    const long long rows_per_block = 512LL * ING_ITER;
    const long long gy = (ld + rows_per_block - 1) / rows_per_block;
    if (gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ingest_any<T>, dim3((unsigned)p, (unsigned)gy), dim3(256), 0, st, src, rs, cs, order, n, X, ld,
                       nan_flag);
  }
  LAUNCH_CHECK();
  return hipSuccess;
}

// X[0..ld) x [0..p) <- src (n x p, element (i, j) at src[order[i] * rs + j * cs]); order may be null (identity).
// ld: multiple of 128, >= n.  *nan_flag is only ever set, never cleared: the caller zeroes it.
hipError_t launch_ingest(const void *src, int f32, long long rs, long long cs, const int *order, long long n,
                         long long p, double *X, long long ld, unsigned *nan_flag, hipStream_t st) {
  if (!src || !X || !nan_flag || n < 1 || p < 1 || ld < n || ld % 128 != 0 || rs < 0 || cs < 0 || p > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (f32) return launch_ingest_t(static_cast<const float *>(src), rs, cs, order, n, p, X, ld, nan_flag, st);
  return launch_ingest_t(static_cast<const double *>(src), rs, cs, order, n, p, X, ld, nan_flag, st);
}

}  // namespace bessx
