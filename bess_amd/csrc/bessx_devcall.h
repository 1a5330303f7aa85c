#ifndef BESSX_DEVCALL_H
#define BESSX_DEVCALL_H
// bessx_devcall.h -- what the entry points that take a caller's X in GPU memory share (include/bessx.h sections 2c to 2r,
// in bessx_abi.cpp): a view of the call's arguments with its checks, the scope one call runs in,
// the copy of staged results to the caller's host memory, and the timing of the single-kernel benches.
#include "bessx_host.h"

#include <climits>

namespace bessx {

static_assert((int)BESSX_LINK_IDENTITY == (int)PREDICT_IDENTITY && (int)BESSX_LINK_LOGISTIC == (int)PREDICT_LOGISTIC &&
                  (int)BESSX_LINK_POISSON == (int)PREDICT_POISSON, "link codes of the launcher");

// ---- the arguments of a call ----------------------------------------------------------------------------------------
// The public input structs share field names: each converts once to the view of its side, which the checks and the
// staging helpers take.

// x, the model(s) and the data of a GLM call.  One model: R = 1, one column of y, coef0 points into the input struct.
struct GlmCall {
  const void *x;
  int x_dtype;
  long long rs, cs;
  int n, p;
  const int *cols;
  int m;
  const double *beta, *coef0;  // m x R, R
  int R, link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_rs, y_cs;
  int y_cols;
  const double *w_host;
  const void *w_dev;
  int w_dtype;
  long long w_stride;
  hipStream_t stream;
  int f32() const { return x_dtype == BESSX_F32; }
};

template <class In>  // bessx_info_input and the structs that begin like it
GlmCall glm_call(const In *in) {
  return GlmCall{in->x,           in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,     in->p,        in->cols,
                 in->m,           in->beta,    &in->coef0,       1,                in->link,  in->y_host,   in->y_dev,
                 in->y_dtype,     in->y_stride, 0,               1,                in->weight_host,          in->weight_dev,
                 in->weight_dtype, in->weight_stride, static_cast<hipStream_t>(in->stream)};
}
inline GlmCall glm_call(const bessx_eval_input *in) {
  return GlmCall{in->x,        in->x_dtype,      in->x_row_stride,  in->x_col_stride, in->n,    in->p,      in->cols,
                 in->m,        in->B,            in->coef0,         in->R,            in->link, in->y_host, in->y_dev,
                 in->y_dtype,  in->y_row_stride, in->y_col_stride,  in->y_cols,       in->weight_host,      in->weight_dev,
                 in->weight_dtype, in->weight_stride, static_cast<hipStream_t>(in->stream)};
}

// x, the model(s) and the data of a Cox call (time, status and weight in host memory; null where a call has none)
struct CoxCall {
  const void *x;
  int x_dtype;
  long long rs, cs;
  int n, p;
  const int *cols;
  int m;
  const double *beta;  // m x R
  int R;
  const double *time, *status, *weight;
  int ties;
  hipStream_t stream;
  int f32() const { return x_dtype == BESSX_F32; }
};

template <class In>  // bessx_cox_info_input and the structs that begin like it
CoxCall cox_call(const In *in) {
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,      in->p,    in->cols, in->m,
                 in->beta, 1,        in->time,         in->status,       in->weight, in->ties, static_cast<hipStream_t>(in->stream)};
}
inline CoxCall cox_call(const bessx_cox_eval_input *in) {
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,      in->p,    in->cols, in->m,
                 in->B, in->R,       in->time,         in->status,       in->weight, in->ties, static_cast<hipStream_t>(in->stream)};
}
inline CoxCall cox_call(const bessx_cox_baseline_input *in) {  // (Breslow's estimator: ties = 1)
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,      in->p, in->cols, in->m,
                 in->B, 1,           in->time,         in->status,       in->weight, 1,     static_cast<hipStream_t>(in->stream)};
}
inline CoxCall cox_call(const bessx_cox_survival_input *in) {
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,   in->p, in->cols, in->m,
                 in->B, 1,           nullptr,          nullptr,          nullptr, 1,     static_cast<hipStream_t>(in->stream)};
}
inline CoxCall cox_call(const bessx_cox_survtime_input *in) {
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,   in->p, in->cols, in->m,
                 in->B, 1,           nullptr,          nullptr,          nullptr, 1,     static_cast<hipStream_t>(in->stream)};
}
inline CoxCall cox_call(const bessx_cox_brier_input *in) {  // (no status: row_a and time_b carry what it decides)
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,   in->p,      in->cols, in->m,
                 in->B, in->R,       in->time,         nullptr,          in->weight, 1,       static_cast<hipStream_t>(in->stream)};
}

// ---- the checks that need no device: they report under the entry point's name ------------------------------------------
// the shape and the support of a model
inline int predict_check_model(const char *who, int n, int p, const int *cols, int m, int R, int link) {
  const std::string w(who);
  if (n < 1 || p < 1) return fail(BESSX_ERR_ARG, w + ": empty matrix");
  if (R < 1) return fail(BESSX_ERR_ARG, w + ": R must be at least 1");
  if (link != BESSX_LINK_IDENTITY && link != BESSX_LINK_LOGISTIC && link != BESSX_LINK_POISSON)
    return fail(BESSX_ERR_ARG, w + ": unknown link");
  if (m < 0 || m > p) return fail(BESSX_ERR_ARG, w + ": m must lie in [0, p]");
  if (m > 0 && !cols) return fail(BESSX_ERR_ARG, w + ": null argument (cols)");
  for (int k = 0; k < m; k++) {
    if (cols[k] < 0 || cols[k] >= p) return fail(BESSX_ERR_ARG, w + ": column number out of range");
    if (k > 0 && cols[k] <= cols[k - 1]) return fail(BESSX_ERR_ARG, w + ": cols must be ascending and distinct");
  }
  return 0;
}

// the kernels of bessx_k_info.hip and what builds on them hold one row of the (m + 1)-square in a block
inline int check_m_max(const std::string &w, int m) {
  if (m + 1 > INFO_M_MAX)
    return fail(BESSX_ERR_UNSUPPORTED, w + ": m + 1 must be at most " + std::to_string(INFO_M_MAX));
  return 0;
}

// x, strides, the support, the coefficients (named B and not tested for finiteness when a call takes several models)
inline int check_x_model(const std::string &w, const void *x, int x_dtype, bool strides_ok, int n, int p, const int *cols,
                         int m, const double *beta, int R, int link, bool one_model) {
  if (x_dtype != BESSX_F64 && x_dtype != BESSX_F32)
    return fail(BESSX_ERR_ARG, w + ": x: dtype must be BESSX_F64 or BESSX_F32");
  if (!strides_ok) return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  if (int rc = predict_check_model(w.c_str(), n, p, cols, m, R, link)) return rc;
  if (m > 0 && !beta) return fail(BESSX_ERR_ARG, w + (one_model ? ": null argument (beta)" : ": null argument (B)"));
  if (one_model)
    for (int k = 0; k < m; k++)
      if (!std::isfinite(beta[k])) return fail(BESSX_ERR_ARG, w + ": beta must be finite");
  return 0;
}

inline int glm_check(const char *who, const GlmCall &c, bool one_model) {
  const std::string w(who);
  if (!c.x || !c.coef0) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = check_x_model(w, c.x, c.x_dtype, c.rs >= 0 && c.cs >= 0 && c.y_rs >= 0 && c.y_cs >= 0 && c.w_stride >= 0,
                             c.n, c.p, c.cols, c.m, c.beta, c.R, c.link, one_model))
    return rc;
  if (one_model && !std::isfinite(*c.coef0)) return fail(BESSX_ERR_ARG, w + ": coef0 must be finite");
  if ((c.y_host != nullptr) == (c.y_dev != nullptr))
    return fail(BESSX_ERR_ARG, w + ": give y as a host pointer or as a device view (one of the two)");
  if (c.y_dev && c.y_dtype != BESSX_F64 && c.y_dtype != BESSX_F32)
    return fail(BESSX_ERR_ARG, w + ": y: dtype must be BESSX_F64 or BESSX_F32");
  if (c.y_cols != 1 && c.y_cols != c.R) return fail(BESSX_ERR_ARG, w + ": y_cols must be 1 or R");
  if (c.w_host && c.w_dev)
    return fail(BESSX_ERR_ARG, w + ": give weight as a host pointer or as a device vector, not both");
  if (c.w_dev && c.w_dtype != BESSX_F64 && c.w_dtype != BESSX_F32)
    return fail(BESSX_ERR_ARG, w + ": weight: dtype must be BESSX_F64 or BESSX_F32");
  return 0;
}

// x and the model of a Cox call; with rows: ties, time and status as well (*events: rows with status 1)
inline int cox_check(const char *who, const CoxCall &c, bool one_model, bool rows = true, int *events = nullptr) {
  const std::string w(who);
  if (!c.x || (rows && (!c.time || !c.status))) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = check_x_model(w, c.x, c.x_dtype, c.rs >= 0 && c.cs >= 0, c.n, c.p, c.cols, c.m, c.beta, c.R,
                             BESSX_LINK_IDENTITY, one_model))
    return rc;
  if (!rows) return 0;
  if (c.ties != 0 && c.ties != 1) return fail(BESSX_ERR_ARG, w + ": ties must be 0 (order) or 1 (breslow)");
  int ev = 0;
  for (int i = 0; i < c.n; i++) {
    if (std::isnan(c.time[i])) return fail(BESSX_ERR_ARG, w + ": time holds a NaN");
    if (c.status[i] != 0.0 && c.status[i] != 1.0) return fail(BESSX_ERR_ARG, w + ": status must be 0 or 1");
    ev += c.status[i] != 0.0;
  }
  if (events) *events = ev;
  return 0;
}

// ---- the checks that ask the runtime ----------------------------------------------------------------------------------
// `what` (an n x cols view) is device memory of device dev, the one that owns x; `subject`: how the second message names
// it when that is not `what`
inline int check_on_device(const char *who, const char *what, const void *data, int dtype, long long rs, long long cs,
                           long long n, long long cols, int dev, const char *subject = nullptr) {
  const std::string w(who);
  int od = -1;
  if (int rc = check_device_matrix((w + ": " + what).c_str(), data, dtype, rs, cs, n, cols, &od)) return rc;
  if (od != dev) return fail(BESSX_ERR_ARG, w + ": " + (subject ? subject : what) + " is not on the device that owns x");
  return 0;
}

// a device is there and x is a view of its memory (*dev: which); y and weight, where given as device views, lie on it
inline int cox_check_device(const char *who, const CoxCall &c, int *dev) {
  if (int rc = need_device()) return rc;
  return check_device_matrix((std::string(who) + ": x").c_str(), c.x, c.x_dtype, c.rs, c.cs, c.n, c.p, dev);
}
inline int glm_check_device(const char *who, const GlmCall &c, int *dev) {
  if (int rc = need_device()) return rc;
  if (int rc = check_device_matrix((std::string(who) + ": x").c_str(), c.x, c.x_dtype, c.rs, c.cs, c.n, c.p, dev)) return rc;
  if (c.y_dev)
    if (int rc = check_on_device(who, "y", c.y_dev, c.y_dtype, c.y_rs, c.y_cols == 1 ? 0 : c.y_cs, c.n, c.y_cols, *dev))
      return rc;
  if (c.w_dev)
    if (int rc = check_on_device(who, "weight", c.w_dev, c.w_dtype, c.w_stride, 0, c.n, 1, *dev)) return rc;
  return 0;
}

// ---- the scope of one call --------------------------------------------------------------------------------------------
// What a call owns while it runs: device memory and events (sc), its host staging vectors, and the private stream.
struct DevCall {
  Owner sc;
  std::vector<double> h, pk;  // results on their way to the caller; a packed factor on its way to the device
  hipStream_t st = nullptr;
};

// Runs body(DevCall &) on device dev with a non-blocking stream of its own that waits for everything the caller has
// queued on `caller` so far.  THE INVARIANT: everything queued on the private stream is complete before any buffer of the
// call is freed, on every return path -- a body that succeeds has synchronised the stream itself, after a body that
// fails the stream is synchronised here, and only then do sc, h and pk go.  Host data that the body's copies read and
// that lives outside the DevCall (a time order, a plan of groups or clusters) is declared by the entry point BEFORE this
// call, so that it outlives it.
template <class Body>
int dev_call(int dev, hipStream_t caller, Body &&body) {
  HIPX(hipSetDevice(dev));
  hipStream_t st = nullptr;
  HIPX(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int rc;
  {
    DevCall dc;
    dc.st = st;
    rc = [&]() -> int {
      hipEvent_t ev = nullptr;
      HIPX(dc.sc.event(&ev, hipEventDisableTiming));
      HIPX(hipEventRecord(ev, caller));
      HIPX(hipStreamWaitEvent(st, ev, 0));
      return body(dc);
    }();
    if (rc) (void)hipStreamSynchronize(st);
  }
  (void)hipStreamDestroy(st);
  return rc;
}

// cnt runs of len staged doubles to the caller's host memory, run j at dst + j * ld (a vector: cnt = 1)
inline void copy_out(const double *src, size_t len, size_t cnt, double *dst, long long ld) {
  for (size_t j = 0; j < cnt; j++) std::copy(src + j * len, src + (j + 1) * len, dst + (long long)j * ld);
}

// ---- staging helpers both sides use -----------------------------------------------------------------------------------
// the model in one device allocation of `sc`: cols, then B, then coef0 (queued on st; the host arrays must outlive it)
inline int predict_upload_model(Owner &sc, const int *cols, int m, const double *B, const double *coef0, int R,
                                hipStream_t st, int **cols_d, double **B_d, double **c_d) {
  HIPX(sc.alloc(B_d, (size_t)m * R + (size_t)R));
  HIPX(sc.alloc(cols_d, (size_t)m));
  *c_d = *B_d + (size_t)m * R;
  if (m > 0) {
    HIPX(hipMemcpyAsync(*cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(hipMemcpyAsync(*B_d, B, (size_t)m * R * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIPX(hipMemcpyAsync(*c_d, coef0, (size_t)R * sizeof(double), hipMemcpyHostToDevice, st));
  return 0;
}

// ---- the timing of the bessx_op_*_bench functions ---------------------------------------------------------------------
// Two events of `sc`; run: one warm-up launch, then `repeats` launches between the events on the null stream.  launch()
// returns 0 or the code of a failure it has reported.
struct BenchTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int init(Owner &sc) {
    HIPX(sc.event(&e0));
    HIPX(sc.event(&e1));
    return 0;
  }
  template <class Launch>
  int run(int repeats, float *ms, Launch &&launch) {
    if (int rc = launch()) return rc;
    HIPX(hipEventRecord(e0, nullptr));
    for (int i = 0; i < repeats; i++)
      if (int rc = launch()) return rc;
    HIPX(hipEventRecord(e1, nullptr));
    HIPX(hipEventSynchronize(e1));
    HIPX(hipEventElapsedTime(ms, e0, e1));
    return 0;
  }
};

}  // namespace bessx

#endif  // BESSX_DEVCALL_H
