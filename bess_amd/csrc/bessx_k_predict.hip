// bessx_k_predict.hip -- prediction on a caller's DEVICE matrix: eta = X[:, cols] B + c for R responses, plus the link
// (+ launcher).  The loops that form eta are those of bessx_k_xb.hpp (k_xb_rows / k_xb_gather: in-place reads of the m
// support columns at any strides, fp32 widened in registers, fixed summation order); this file supplies the epilogue
// that stores link(eta).  A NaN in a support column of a row reaches that row's outputs; the other columns are not read.
#include "bessx_k_xb.hpp"

namespace bessx {

namespace {

// what bess_base.predict computes from eta on the host: the comparisons keep a NaN a NaN (fmin / fmax would drop it)
struct PrStore {
  static constexpr bool REDUCE = false, SKIPZ = false;
  int link;
  double *__restrict__ out, *__restrict__ out2;
  long long ors, ocs;
  __device__ __forceinline__ void store(double eta, long long i, int r) const {
    const long long off = i * ors + (long long)r * ocs;
    if (link == PREDICT_LOGISTIC) {
      const double cl = eta > 25.0 ? 25.0 : (eta < -25.0 ? -25.0 : eta);
      const double e = exp(cl);
      out[off] = e / (e + 1.0);
      out2[off] = eta > 0.0 ? 1.0 : 0.0;
    } else if (link == PREDICT_POISSON) {
      out[off] = exp(eta);
    } else {
      out[off] = eta;
    }
  }
};

}  // namespace

// out[i * ors + r * ocs] = link(sum_k src(i, cols[k]) * B[k * R + r] + c[r]) for i < n, r < R; cols (m, ascending, device),
// B (m x R row-major, device), c (R, device).  PREDICT_LOGISTIC: out = e / (e + 1) with e = exp(clip(eta, -25, 25)) and
// out2 (same strides) = (eta > 0); PREDICT_POISSON: out = exp(eta).  m = 0 reads no byte of src.
hipError_t launch_predict(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                          const double *B, const double *c, int R, int link, double *out, long long ors, long long ocs,
                          double *out2, hipStream_t st) {
  if (!src || !c || !out || n < 1 || n > 0x7fffffffLL || m < 0 || (m > 0 && (!cols || !B)) || R < 1 || rs < 0 || cs < 0 ||
      ors < 0 || ocs < 0 || link < PREDICT_IDENTITY || link > PREDICT_POISSON || (link == PREDICT_LOGISTIC && !out2))
    return hipErrorInvalidValue;
  const PrStore epi{link, out, out2, ors, ocs};
  if (f32) return xb_launch(static_cast<const float *>(src), rs, cs, n, cols, m, B, c, R, epi, st);
  return xb_launch(static_cast<const double *>(src), rs, cs, n, cols, m, B, c, R, epi, st);
}

}  // namespace bessx
