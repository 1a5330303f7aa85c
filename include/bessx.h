/* include/bessx.h -- C ABI of libbessx.so, the MI355X-native PDAS best-subset solver.
 *
 * This is the drop-in boundary for the hot path of Mamba413/bess (reference paths are
 * relative to /root/reference).  Plain pointers and sizes only; no C++/torch types.
 * Every entry point returns 0 (BESSX_OK) or an error code; bessx_last_error() gives the
 * message for the calling thread.  The library never falls back to a CPU path: if no
 * HIP device is usable every compute entry point fails with BESSX_ERR_HIP.
 *
 * Layers (each cites the reference interface it replaces):
 *   1. bessx_pywrap_bess      <- pywrap_bess, src/bess.h:35-51 (what SWIG binds, python/src/bess.i:17-30)
 *   2. bessx_session_*        <- bessCpp, src/bess.h:20-33: Data + Algorithm* + Metric* set-up
 *                                (src/bess.cpp:61-165) kept resident on the GPU, then
 *                                sequential_path / gs_path / pgs_path (src/path.h:22-44)
 *   3. bessx_session_fit      <- Algorithm::fit + the update_* setters, src/Algorithm.h:77-171
 *   4. bessx_op_*             <- single Eigen call sites of the hot loop;
 *                                exported so that every HIP kernel can be parity-tested alone.
 */
#ifndef BESSX_H
#define BESSX_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  BESSX_OK = 0,
  BESSX_ERR_ARG = 1,         /* invalid argument (the reference would crash or read out of bounds) */
  BESSX_ERR_HIP = 2,         /* HIP runtime / device failure, or no device */
  BESSX_ERR_UNSUPPORTED = 3, /* valid for the reference, not built here (see bessx_problem: screening with groups / Poisson) */
  BESSX_ERR_NUMERIC = 4      /* non-finite pivot in a k x k solve */
};

const char *bessx_last_error(void);

/* Device / build information: writes a NUL-terminated description (device name, CU count,
 * code-object arch) into buf.  Fails with BESSX_ERR_HIP when no GPU is visible. */
int bessx_device_info(char *buf, int buf_len);

/* ---------------------------------------------------------------------------------------
 * 1. Drop-in for pywrap_bess (src/bess.h:35-51, src/bess.cpp:218-281).
 *    Identical argument list (bool -> int).  x is row-major x_row * x_col.  Writes
 *    beta_out[0..x_col), *coef0_out, *train_loss_out, *ic_out exactly like the reference
 *    (src/bess.cpp:277-280); additionally fills the slots the reference leaves
 *    uninitialised: *nullloss_out (Data::get_nullloss, src/Data.h:120-130: |y|^2 / n of the
 *    normalised response for data_type 1, else 2 log 2 * sum(weight)),
 *    A_out[0..k) = selected support, *l_out = PDAS iterations of the selected candidate;
 *    aic/bic/gic_out are set to 0.
 *    Differences, all documented in INTEGRATION.md: is_cv draws folds from a fixed-seed
 *    generator instead of std::random_device; invalid codes return BESSX_ERR_ARG instead of
 *    dereferencing a null Algorithm* (src/bess.cpp:93-116).
 * ------------------------------------------------------------------------------------- */
int bessx_pywrap_bess(double *x, int x_row, int x_col, double *y, int y_len, int data_type, double *weight,
                      int weight_len, int is_normal, int algorithm_type, int model_type, int max_iter,
                      int exchange_num, int path_type, int is_warm_start, int ic_type, int is_cv, int K, int *gindex,
                      int gindex_len, double *state, int state_len, int *sequence, int sequence_len,
                      double *lambda_sequence, int lambda_sequence_len, int s_min, int s_max, int K_max,
                      double epsilon, double lambda_min, double lambda_max, int n_lambda, int is_screening,
                      int screening_size, int powell_path, int *always_select, int always_select_len, double tao,
                      double *beta_out, int beta_out_len, double *coef0_out, int coef0_out_len,
                      double *train_loss_out, int train_loss_out_len, double *ic_out, int ic_out_len,
                      double *nullloss_out, double *aic_out, int aic_out_len, double *bic_out, int bic_out_len,
                      double *gic_out, int gic_out_len, int *A_out, int A_out_len, int *l_out);

/* ---------------------------------------------------------------------------------------
 * 1b. Drop-in for bessCpp (src/bess.h:20-33, src/bess.cpp:37-214), the C++ entry the R package binds
 *     (R/src/RcppExports.cpp:10-48).  Same 30 arguments with Eigen objects unpacked into pointer + length
 *     (bool -> int); x is COLUMN-major n x p, as Eigen::MatrixXd and R matrices are.  The outputs are the named
 *     entries of the list the R build returns (src/path.cpp:116-123 sequential, :376-380 golden section,
 *     + screening_A, src/bess.cpp:207), flattened:
 *       sequential_path: candidate q = j * sequence_len + i for lambda j and size i -- beta_all = lambda_len blocks of
 *         p x sequence_len (column-major), coef0_all / train_loss_all = lambda_len blocks of sequence_len, ic_all =
 *         sequence_len x lambda_len column-major;  n_all = sequence_len * lambda_len.
 *       gs_path / pgs_path: candidate q = evaluation order (every new golden-section point, then every improvement
 *         of the final sweep; Powell: the best point of every line search and the final re-fit); n_all = count.
 *     All coefficients are de-normalised like the R build's (src/path.cpp:76-110, :330-373).  R/src/bess_amd_shim.cpp
 *     is the Rcpp wrapper around this function.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  double *beta;            /* p (caller-allocated) */
  double coef0, train_loss, ic, lambda;
  int all_capacity;        /* in: candidates the *_all arrays can hold (beta_all: p * all_capacity doubles) */
  int n_all;               /* out: candidates the path produced (written: min(n_all, all_capacity)) */
  double *beta_all, *coef0_all, *train_loss_all, *ic_all; /* caller-allocated, any may be NULL */
  int *screening_A;        /* screening_size entries (0-based original columns) when is_screening, may be NULL */
} bessx_r_result;

int bessx_bessCpp(const double *x, int n, int p, const double *y, int data_type, const double *weight, int is_normal,
                  int algorithm_type, int model_type, int max_iter, int exchange_num, int path_type,
                  int is_warm_start, int ic_type, int is_cv, int K, const double *state, int state_len,
                  const int *sequence, int sequence_len, const double *lambda_seq, int lambda_len, int s_min, int s_max,
                  int K_max, double epsilon, double lambda_min, double lambda_max, int nlambda, int is_screening,
                  int screening_size, int powell_path, const int *g_index, int g_index_len, const int *always_select,
                  int always_select_len, double tao, bessx_r_result *res);

/* ---------------------------------------------------------------------------------------
 * 2. Session: the state bessCpp builds (src/bess.cpp:61-165), resident in HBM.
 * ------------------------------------------------------------------------------------- */
typedef struct bessx_session bessx_session;

typedef struct {
  int n, p;
  const double *x;   /* host pointer */
  int x_col_major;   /* 0: row-major n x p (NumPy / pywrap_bess); 1: column-major (R / bessCpp MatrixXd) */
  const double *y;   /* n; for Cox: status, rows already sorted by time (python/bess/linear.py:257-263) */
  const double *weight; /* n, or NULL for all ones */
  int data_type;     /* 1 centre x,y + scale; 2 centre x + scale; 3 scale only (src/Data.h:79-93) */
  int is_normal;
  int model_type;    /* 1 LM, 2 logistic, 3 Poisson, 4 Cox (src/bess.cpp:95-111) */
  int algorithm_type;/* 1 PDAS, 5 L0L2 (same code path, lambda from the path); 2/3 need groups of size 1 */
  int max_iter;      /* PDAS iterations per fit (Algorithm::max_iter) */
  int is_warm_start;
  const int *always_select; /* indices kept in every active set (Algorithm::always_select), may be NULL */
  int always_select_len;
  int device;        /* HIP device ordinal, or -1 for the current device */
  const int *group_index; /* Data::g_index (src/Data.h:59-67): first column of every group, ascending from 0; NULL or
                             length p = every column its own group.  With groups, sparsity levels and always_select
                             count / name GROUPS.  Any group width the session's capacity (max_sparsity) holds -- up to 16 columns
                             a register-resident block per group, wider ones a tiled path; Cox: at most 256 columns per
                             group.  Cox with real groups needs algorithm_type 2 / 3
                             (the group branch of GroupPdasCox::get_A, src/Algorithm.h:1497-1568). */
  int group_index_len;
  int is_screening;   /* sure independence screening before the path (screening(), src/screening.cpp:26-105; called at
                         src/bess.cpp:57-61): keep the screening_size columns with the largest squared marginal
                         coefficient on the raw data plus always_select.  LM, logistic and Cox; with groups of
                         size > 1 (any width) screening_size and always_select count / name GROUPS, the marginal fit
                         is the model's fit on the whole group, and the coefficients are written to the columns they
                         belong to -- the reference misplaces them in this case, src/bess.cpp:195-198.  Poisson is
                         refused (the reference's poisson_fit is undefined behaviour there, src/poisson.cpp:113), and so
                         is a logistic group at least as wide as the sample (logit_fit's n <= p branch returns n
                         coefficients of which screening() reads the last g_size: out of bounds).
                         The session then lives on the kept columns: sparsity levels, traces,
                         bessx_session_fit and bessx_session_get_normalization index them 0..screening_size-1
                         (bessx_session_get_screening gives the map); every bessx_path_result is written in the
                         ORIGINAL column numbering, like src/bess.cpp:186-209. */
  int screening_size;
  int score_mode;     /* how the LM score pass X^T r of get_A is evaluated: 0 = automatic
                         (environment variable BESSX_SCORE_MODE, else covariance updates when they apply),
                         1 = streaming: every PDAS iteration reads X once, 2 = covariance updates: cached Gram
                         columns X^T x_a, X is read only when a new column enters.  Same results either way up to
                         summation order. */
  int max_sparsity;   /* largest number of active COLUMNS any fit of this session will be asked for (sparsity level x
                         largest group size); sizes the k x k work space.  0 = default: min(p, 2046).  Up to 16382;
                         levels beyond 254 use the blocked Cholesky in global memory.  bessx_pywrap_bess derives it
                         from sequence / s_max, so the reference's default sequence 1..min(p, n / log n)
                         (python/bess/linear.py:285-287) runs as it is. */
} bessx_problem;

int bessx_session_create(bessx_session **out, const bessx_problem *prob);
void bessx_session_destroy(bessx_session *s);

/* ---------------------------------------------------------------------------------------
 * 2b. X already in GPU memory.  The design matrix is read where it lies -- it never crosses the bus -- by one
 *     ingest kernel (bessx_k_ingest.hip) that leaves in the session exactly (bit for bit) the matrix that
 *     bessx_session_create uploads for the same values; everything after it is the same code.
 *     A matrix is (data, dtype, row_stride, col_stride): element (i, j) at data[i * row_stride + j * col_stride],
 *     strides in ELEMENTS, non-negative; dtype BESSX_F64 or BESSX_F32 (widened exactly).  Column-contiguous
 *     (row_stride 1) and row-contiguous (col_stride 1, a C-contiguous torch tensor) sources run at streaming rate;
 *     any other view is correct, not fast.
 *     row_order (host, n entries, a permutation of 0..n-1; NULL = identity): session row i is row row_order[i] of x.
 *     It applies to x ONLY: y and weight are given in the session's row order.  (The Cox estimators sort rows by
 *     time this way without a second copy of X.)
 *     y and weight are n values each: a host pointer (*_host) or a device vector (*_dev, *_dtype, *_stride); give one
 *     of the two for y; weight may be all NULL (= ones).  They are copied to the host once.
 *     stream: the HIP stream (hipStream_t) on which the caller produced the data, NULL = the null stream.  The library
 *     orders its reads after the work queued on that stream so far (event + stream wait) and has finished reading
 *     the caller's memory when the call returns: the caller's buffers are never written, never referenced afterwards,
 *     and may be freed or overwritten at once.  Peak device memory is therefore the caller's X plus the session's own
 *     padded fp64 copy (with screening: plus the kept columns).
 *     Every device pointer must be device memory (hipPointerGetAttributes) of the session's device and hold the
 *     whole view: otherwise BESSX_ERR_ARG, not a fault.  A NaN in x: BESSX_ERR_ARG, message "There is NAN value in X"
 *     (the kernel raises a device flag; X is not read back).
 * ------------------------------------------------------------------------------------- */
enum { BESSX_F64 = 0, BESSX_F32 = 1 };
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_stride;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  const int *row_order;
  void *stream;
} bessx_device_input;
/* bessx_session_create with the data of `in`: prob->x / y / weight / x_col_major are ignored; prob->device == -1
 * means the device that owns in->x.  Screening works (wide-group marginal fits run on column-offset views of in->x). */
int bessx_session_create_device(bessx_session **out, const bessx_problem *prob, const bessx_device_input *in);
/* bessx_pywrap_bess for data in GPU memory (section 2b): the x, x_row, x_col triple becomes the descriptor plus the
 * shape; y and weight come from the descriptor.  Everything after session creation is shared with bessx_pywrap_bess.
 * *x_nan_out (may be NULL) is set to 1 when the call fails because x holds a NaN, else 0. */
int bessx_pywrap_bess_device(const bessx_device_input *in, int x_row, int x_col, int data_type, int is_normal,
                             int algorithm_type, int model_type, int max_iter, int exchange_num, int path_type,
                             int is_warm_start, int ic_type, int is_cv, int K, int *gindex, int gindex_len,
                             double *state, int state_len, int *sequence, int sequence_len, double *lambda_sequence,
                             int lambda_sequence_len, int s_min, int s_max, int K_max, double epsilon,
                             double lambda_min, double lambda_max, int n_lambda, int is_screening, int screening_size,
                             int powell_path, int *always_select, int always_select_len, double tao, double *beta_out,
                             int beta_out_len, double *coef0_out, int coef0_out_len, double *train_loss_out,
                             int train_loss_out_len, double *ic_out, int ic_out_len, double *nullloss_out,
                             double *aic_out, int aic_out_len, double *bic_out, int bic_out_len, double *gic_out,
                             int gic_out_len, int *A_out, int A_out_len, int *l_out, int *x_nan_out);
/* ---------------------------------------------------------------------------------------
 * 2c. Prediction on an X already in GPU memory (bessx_k_predict.hip).  Stateless: a model is (cols, B, coef0), no
 *     session is needed, and the device is the one that owns x.  For row i and response r
 *         eta(i, r) = sum_k x(i, cols[k]) * B[k * R + r] + coef0[r]
 *     is formed from the m support columns alone -- n * m elements of x are read where they lie, not n * p; no fp64 copy
 *     of x is made, and x is never written.  x is a matrix as in section 2b (dtype, element strides, non-negative).
 *     cols: m >= 0 column numbers, ascending, distinct, in [0, p) (the union of the supports; m = 0 reads no byte of x
 *     and every row gets coef0); B: m x R row-major; coef0: R values; all three in HOST memory.  R >= 1.
 *     link            out                                              out2
 *     _IDENTITY       eta                                              NULL (ignored)
 *     _LOGISTIC       e / (e + 1), e = exp(clip(eta, -25, 25))         labels: 1.0 where eta > 0, else 0.0 (required)
 *     _POISSON        exp(eta)                                         NULL (ignored)
 *     out (and out2) hold element (i, r) at [i * out_row_stride + r * out_col_stride], strides in elements, non-negative
 *     and non-zero along every axis longer than 1.  out_on_device != 0: they are device memory of x's device, checked
 *     like the inputs of section 2b (hipPointerGetAttributes, the whole view inside its allocation): a wrong pointer is
 *     BESSX_ERR_ARG, not a fault.  Otherwise they are host memory: the library stages the n * R results through a
 *     device buffer of its own and copies them back.
 *     stream: as in section 2b.  Reads of x and writes of out are ordered after the work queued on `stream` so far; when
 *     the call returns the kernel has finished, and x is not referenced afterwards.
 *     Every sum has a fixed order (no floating-point atomics): the same call gives the same bits.  A NaN in a support
 *     column of a row reaches that row's outputs and is no error; columns outside the support are not read.
 *     Argument errors (BESSX_ERR_ARG with a message) are found before any device call; without a GPU a call with valid
 *     arguments returns BESSX_ERR_HIP.
 * ------------------------------------------------------------------------------------- */
enum { BESSX_LINK_IDENTITY = 0, BESSX_LINK_LOGISTIC = 1, BESSX_LINK_POISSON = 2 };
int bessx_predict_device(const void *x, int x_dtype, long long x_row_stride, long long x_col_stride, int n, int p,
                         const int *cols, int m, const double *B, const double *coef0, int R, int link, double *out,
                         long long out_row_stride, long long out_col_stride, double *out2, int out_on_device,
                         void *stream);
/* ---------------------------------------------------------------------------------------
 * 2d. Held-out loss on an X already in GPU memory (bessx_k_eval.hip).  Stateless like section 2c, and the same model:
 *     with eta(i, r) as there,
 *         loss[r] = sum_i w_i * f(eta(i, r), y(i, r))
 *     in ONE pass over the m support columns (n * m elements of x read where they lie, x never written, no fp64 copy of
 *     it; m = 0 reads no byte of x) -- the n x R predictions are never stored.
 *     link         f(eta, y)                                           aux[r]
 *     _IDENTITY    (y - eta)^2                                         ignored (may be NULL)
 *     _LOGISTIC    max(eta, 0) + log1p(exp(-|eta|)) - y * eta          sum_i w_i * [(eta > 0) == (y > 0.5)]: the weighted
 *                  (negative log-likelihood, overflow-free, no        count of correct labels, label rule of section 2c
 *                  clamp; any y in [0, 1])                              (required)
 *     _POISSON     exp(eta) - y * eta  (negative log-likelihood        ignored (may be NULL)
 *                  without the term in y alone)
 *     x, n, p, cols, m, B, coef0, R, link: as in section 2c (cols / B / coef0 in HOST memory, same checks).
 *     y: element (i, r) at [i * y_row_stride + r * y_col_stride], strides in elements, non-negative.  y_cols = 1: one
 *     column shared by all R models (y_col_stride is ignored); y_cols = R: one column per model.  Give y_host (fp64) or
 *     y_dev (device memory, y_dtype BESSX_F64 / BESSX_F32), not both.
 *     weight: n values, weight_host (fp64, contiguous) or weight_dev (weight_dtype, weight_stride), or both NULL = ones.
 *     stream: as in section 2b.  The reads are ordered after the work queued on `stream` so far; when the call returns
 *     the caller's buffers are no longer referenced.
 *     Outputs (host): loss[R]; aux[R] for the logistic link; *sum_w = sum_i w_i (exactly n without weights).
 *     Every sum is fp64 and has a fixed order -- a workgroup adds its rows in a fixed order and writes one partial per
 *     response, a second launch adds the partials in a fixed order; no floating-point atomics: the same call gives the same
 *     bits.  A coefficient that is exactly zero takes nothing from its column, so with B holding the union of several
 *     supports a NaN or inf in a column reaches exactly the models that use the column, through the rows that hold it; one
 *     in y or a weight reaches the losses that row belongs to.  None of it is an error; columns outside the support are
 *     not read.
 *     Every device pointer is checked as in section 2b (a wrong pointer or a view past its allocation: BESSX_ERR_ARG, not
 *     a fault).  Argument errors are found before any device call; without a GPU a call with valid arguments returns
 *     BESSX_ERR_HIP.  The call's device buffers are released before it returns (counters 38 / 39 are back at their
 *     earlier values; 40 has grown by the call's requests).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  const double *coef0;
  int R, link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_row_stride, y_col_stride;
  int y_cols;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  void *stream;
} bessx_eval_input;
int bessx_eval_device(const bessx_eval_input *in, double *loss, double *aux, double *sum_w);
/* ---------------------------------------------------------------------------------------
 * 2e. Held-out Cox partial log-likelihood and Harrell's concordance on an X already in GPU memory
 *     (bessx_k_coxeval.hip).  Stateless like sections 2c / 2d and the same model (cols, B, R), without an intercept:
 *         eta(i, r) = sum_k x(i, cols[k]) * B[k * R + r]
 *     (a coefficient that is exactly zero takes nothing from its column).  time, status (0 or 1) and weight (may be NULL =
 *     ones) are n values each in HOST memory.  The library sorts the rows itself: pi = std::stable_sort of the row
 *     numbers by time, ascending, equal times in row order; position k holds row pi(k), first(k) is the smallest
 *     position with the time of position k.  With a(k, r) = clamp(eta(pi(k), r), -30, 30), e = exp(a):
 *         ties = 0 ("order", the reference's loglik_cox):  S(k, r) = sum_{l >= k} e(l, r)
 *         ties = 1 ("breslow"):                             S(k, r) = sum_{l >= first(k)} e(l, r)
 *         loglik[r] = sum_k w_k status_k (a(k, r) - log S(k, r))        (weights on the terms, risk sets unweighted)
 *     want_pairs != 0: a pair of positions k < l is comparable when status_k = 1 and time_k < time_l strictly;
 *     *comparable = their number (the data alone decides it), and per model pairs[3 r], pairs[3 r + 1], pairs[3 r + 2] =
 *     the comparable pairs with eta_k > eta_l (concordant), eta_k < eta_l (discordant), neither (tied_risk: equal or
 *     NaN), from the unclamped eta, unweighted, exact 64-bit integers.  want_pairs == 0: pairs may be NULL, *comparable
 *     is still written, and the O(n^2) pair kernel is not launched.
 *     x is read once, the support's columns only, where it lies; every floating-point sum has a fixed order (the same call
 *     gives the same bits); the pair counts are added with integer atomics (exact in any order).  A NaN in a support
 *     column makes the loglik of exactly the models that use the column NaN.  None of it is an error.
 *     Argument errors (BESSX_ERR_ARG: the messages of section 2d for cols / strides / dtype; a NaN in time; a status
 *     other than 0 or 1; ties outside {0, 1}) are found before any device call; without a GPU a call with valid arguments
 *     returns BESSX_ERR_HIP.  Scratch memory (two R x n arrays of doubles and five n-vectors) is released before the call
 *     returns.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  int R;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  int want_pairs;
  void *stream;
} bessx_cox_eval_input;
int bessx_eval_cox_device(const bessx_cox_eval_input *in, double *loglik, long long *pairs, long long *comparable);
/* ---------------------------------------------------------------------------------------
 * 2f. Breslow baseline cumulative hazard and survival curves of ONE Cox model (R = 1, no intercept) on an X already in
 *     GPU memory (bessx_k_coxsurv.hip).  Stateless like sections 2c to 2e.  x is described by dtype, element strides, n and
 *     p; cols is ascending and distinct, m >= 0, in HOST memory; B holds m values in HOST memory; a coefficient that is
 *     exactly zero takes nothing from its column; stream is as in section 2b.  eta_i = sum_k x(i, cols[k]) * B[k].
 *
 *     bessx_cox_baseline_device: the Breslow estimator on the rows the model was fitted to.  time, status (0 or 1) and
 *     weight (may be NULL = ones; otherwise every weight >= 0) are n values each in HOST memory.  Positions, pi and
 *     first(k) are those of section 2e (the host sorts with std::stable_sort).  With a(k) = clamp(eta(pi(k)), -30, 30),
 *     e = exp(a):
 *         S(k) = sum_{l >= first(k)} e(l)        (the risk set is unweighted, as in "breslow" of section 2e)
 *         h(k) = w_k status_k / S(k),            H(k) = sum_{l <= k} h(l)
 *     Outputs (host): *n_times = J, the number of distinct times that carry at least one row with status = 1 (the data
 *     alone decide it; J = 0, every row censored, is valid); times[g], those times, ascending; cumhaz[g] = H(last position
 *     with time times[g]).  The caller sizes times / cumhaz for n entries.  H is an fp64 prefix sum of additions only, in
 *     a fixed order, every term entering once (no floating-point atomics: the same call gives the same bits).
 *     Argument errors besides those of section 2e for x / cols / B: a NaN in time; a status other than 0 or 1; a
 *     negative or NaN weight.
 *
 *     bessx_cox_survival_device: with e_i = exp(clamp(eta_i, -30, 30)) and hg (T >= 1 doubles in HOST memory: the
 *     baseline cumulative hazard at the T requested times -- the caller does the step-function lookup),
 *         kind = BESSX_SURV_SURVIVAL:  out(i, j) = exp(-(hg[j] * e_i))
 *         kind = BESSX_SURV_CUMHAZ:    out(i, j) = hg[j] * e_i
 *     out holds element (i, j) at [i * out_row_stride + j * out_col_stride] and is handled exactly as in section 2c:
 *     out_on_device != 0: device memory of x's device, checked as there; otherwise host memory, staged through a device
 *     buffer of the library's own.  The n x T matrix is written exactly once, at streaming rate when out_col_stride == 1
 *     or out_row_stride == 1 (16-byte stores where the base and the other stride allow); any other strides are correct, not
 *     fast -- the same arithmetic.  A NaN or negative hg[j] is BESSX_ERR_ARG.  hg[j] = 0 gives exactly 1.0 (_CUMHAZ:
 *     exactly 0.0) for every row whose support columns are finite.  A NaN in a support column of row i reaches the T
 *     outputs of row i and nothing else; columns outside the support are not read; x is never written.
 *
 *     Every device pointer is checked as in section 2b (a wrong pointer or a view past its allocation: BESSX_ERR_ARG, not
 *     a fault).  Argument errors are found before any device call; without a GPU a call with valid arguments returns
 *     BESSX_ERR_HIP.  Scratch memory (baseline: that of section 2e with R = 1 plus 2 J values; curves: n + T doubles, and
 *     n * T more for a host out) is released before the call returns: counters 38 / 39 are back at their earlier values.
 * ------------------------------------------------------------------------------------- */
enum { BESSX_SURV_SURVIVAL = 0, BESSX_SURV_CUMHAZ = 1 };
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  const double *time;
  const double *status;
  const double *weight;
  void *stream;
} bessx_cox_baseline_input;
int bessx_cox_baseline_device(const bessx_cox_baseline_input *in, int *n_times, double *times, double *cumhaz);
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  const double *hg;
  int T;
  int kind;
  long long out_row_stride, out_col_stride;
  int out_on_device;
  void *stream;
} bessx_cox_survival_input;
int bessx_cox_survival_device(const bessx_cox_survival_input *in, double *out);
/* ---------------------------------------------------------------------------------------
 * 2g. Expected information and score of ONE model on an X already in GPU memory (bessx_k_info.hip): what a coefficient
 *     table (standard errors, Wald z, p-values) is made of.  Stateless like sections 2c to 2f.  x, n, p, cols, m, link,
 *     y, weight, stream: as in section 2d with R = 1 and one column of y (beta: m values, coef0: one value, HOST memory,
 *     all finite).  With eta_i = sum_k x(i, cols[k]) * beta[k] + coef0 -- the loops of sections 2c / 2d, except that a
 *     zero coefficient is multiplied like any other -- and z_i = (1, x(i, cols[0]), ..., x(i, cols[m - 1])):
 *         info  = sum_i v_i z_i z_i^T      (m + 1) x (m + 1), entry (j, k) at [j * info_ld + k], info_ld >= m + 1;
 *                                          both triangles are written and are bit-identical mirrors
 *         score = sum_i g_i z_i            m + 1 values (intercept first)
 *     link         v_i                                   g_i
 *     _IDENTITY    w_i                                   w_i (y_i - eta_i)
 *     _LOGISTIC    w_i p_i (1 - p_i)                     w_i (y_i - p_i),   p_i = 1 / (1 + exp(-eta_i)), evaluated from
 *                                                        exp(-|eta_i|): no overflow, no clamp
 *     _POISSON     w_i exp(eta_i)                        w_i (y_i - exp(eta_i))
 *     *loss and *sum_w are those of section 2d for the same arguments, bit for bit (for the identity link *loss is the
 *     weighted residual sum of squares).  This is the UNPENALISED expected information on the original scale of x: a
 *     model fitted with a ridge penalty lambda > 0 has score != 0, and the inverse of info is then not its covariance.
 *     The support's columns are read in place -- no gathered copy of x[:, cols] is made -- and accumulated in 16 x 16
 *     tiles on the fp64 matrix cores, the lower triangle only; the rows are split into slabs whose number depends on
 *     (n, m) alone, every slab writes one partial per tile and a second launch adds them in slab order: no
 *     floating-point atomics, the same call gives the same bits.  Rows past n, columns outside the support and the
 *     padding of the last tile are not read.  A NaN INSIDE the support view is no error and propagates by IEEE rules:
 *     it makes eta_i NaN, so for the identity link row j and column j of info (its own entry of z) and every entry of
 *     score are NaN, and for the other links, where v_i depends on eta_i, every entry of info as well -- also when
 *     w_i = 0, since 0 * NaN is NaN.
 *     info and score are device memory of x's device when out_on_device != 0 (checked as in section 2c), else host
 *     memory.  loss and sum_w are host memory.  m + 1 <= 1024: a larger m is BESSX_ERR_UNSUPPORTED, with every other
 *     argument error (BESSX_ERR_ARG, the messages of section 2d; a non-finite beta or coef0) found before any device
 *     call.  Scratch memory (bessx_info_workspace doubles, the model, host y / weight) is released before the call
 *     returns: counters 38 / 39 are back at their earlier values.
 *     bessx_info_workspace needs no device: the doubles of scratch memory of such a call and how its rows are split.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  double coef0;
  int link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_stride;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  double *info;
  long long info_ld;
  double *score;
  int out_on_device;
  void *stream;
} bessx_info_input;
int bessx_info_device(const bessx_info_input *in, double *loss, double *sum_w);
int bessx_info_workspace(int x_dtype, long long x_row_stride, long long x_col_stride, int n, int m, int link,
                         int weighted, long long *doubles, long long *rows_per_slab, int *slabs);
/* ---------------------------------------------------------------------------------------
 * 2h. Observed information and score of ONE Cox model on an X already in GPU memory (bessx_k_coxinfo.hip): the Cox
 *     counterpart of section 2g.  Stateless like sections 2c to 2g.  x, n, p, cols, m, time, status, weight, ties,
 *     stream: as in section 2e with R = 1; beta: m finite values in HOST memory; no intercept.  Positions, pi, first(k):
 *     section 2e.  With eta_i = sum_c x(i, cols[c]) * beta[c] (a zero coefficient takes nothing from its column),
 *     e = exp(clamp(eta, -30, 30)), wd_k = w_k status_k, r(k) = k (ties = 0) or first(k) (ties = 1), x_l the m support
 *     entries of the row at position l,
 *         S0(k) = sum_{l >= r(k)} e_l,    S1(k) = sum_{l >= r(k)} e_l x_l,    u_k = S1(k) / S0(k)
 *         loglik = sum_k wd_k (clamp(eta_k) - log S0(k))              bit for bit section 2e's with want_pairs = 0
 *         score  = sum_k wd_k (x_k - u_k)                             m values
 *         info   = sum_k wd_k sum_{l >= r(k)} (e_l / S0(k)) (x_l - u_k)(x_l - u_k)^T
 *                                          m x m, entry (j, k) at [j * info_ld + k], info_ld >= m; both triangles are
 *                                          written and are bit-identical mirrors
 *     (weights on the event terms only, risk sets unweighted).  info is the negative Hessian of loglik in beta wherever
 *     no clamp is active; where one is, info is this formula and not a derivative.  It is computed as
 *         H_l = sum_{k : r(k) <= l} wd_k / S0(k),   v_l = e_l H_l,   g_l = wd_l - v_l      (g: the martingale residuals)
 *         score = sum_l g_l x_l,     info = G1 - G2,     G1 = sum_l v_l x_l x_l^T,     G2 = sum_{k : status_k = 1} wd_k u_k u_k^T
 *     G1 and score are one sweep of section 2g's matrix-core kernel over x in place; G2 is a second sweep over the J x m
 *     matrix of the u_k of the J rows with status = 1.  *residual_sum = sum_l g_l, which is 0 up to rounding (with m = 0,
 *     where no sweep is launched, it is returned as 0).  *n_events = sum_k wd_k (host, in position order).
 *     info = G1 - G2 is a DIFFERENCE: for columns far from centred both terms are much larger than info and digits are
 *     lost in proportion (the form R's survival::coxph uses as well); centre such columns before the call.
 *     Passes over the support of x: three (predictor, the gather of e_l x_l into position order, G1); no gathered copy of
 *     x[:, cols] in row order is made.  Every scan is additions only in a fixed order, there are no floating-point
 *     atomics, and block and slab counts depend on (n, m, J) alone: the same call gives the same bits.
 *     Scratch memory: about (m + 5) n + J m doubles plus the two sweeps' partials (bessx_cox_info_workspace states it;
 *     3.4 GB at n = 200 000, m = 1023, J = n), released before the call returns: counters 38 / 39 are back at their
 *     earlier values.  A NaN INSIDE the support view is no error and propagates by IEEE rules; rows past n and columns
 *     outside the support are not read.
 *     info and score are device memory of x's device when out_on_device != 0 (checked as in section 2c), else host
 *     memory; loglik, n_events, residual_sum are host memory.  m = 0 is valid: nothing of x is read, info and score are
 *     not touched and loglik is the null model's.  m + 1 <= 1024 (the sweeps carry an intercept entry): a larger m is
 *     BESSX_ERR_UNSUPPORTED, with every other argument error (BESSX_ERR_ARG, the messages of sections 2e / 2g) found
 *     before any device call.
 *     bessx_cox_info_workspace needs no device: for n rows, m columns and J event rows, the doubles of scratch memory and
 *     the row splits of the two sweeps: rows_per_slab[0], slabs[0] of G1 over n rows and rows_per_slab[1], slabs[1] of
 *     G2 over J rows (0, 0 for a sweep that is not launched).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  double *info;
  long long info_ld;
  double *score;
  int out_on_device;
  void *stream;
} bessx_cox_info_input;
int bessx_cox_info_device(const bessx_cox_info_input *in, double *loglik, double *n_events, double *residual_sum);
int bessx_cox_info_workspace(int n, int m, int n_event_rows, long long *doubles, long long *rows_per_slab, int *slabs);
/* ---------------------------------------------------------------------------------------
 * 2i. Per-row diagnostics of ONE model on an X already in GPU memory (bessx_k_diag.hip): which rows drive the fit.
 *     Stateless like sections 2c to 2h.  x, n, p, cols, m, beta, coef0, link, y, weight, stream: as in section 2g.
 *     eta_i, mu_i (identity: eta_i; logistic: p_i; Poisson: exp(eta_i)) and v_i are those of section 2g, the logistic
 *     ones from t = exp(-|eta_i|) without overflow or clamp; w_i = 1 without weights; z_i = (1, x(i, cols[0]), ...),
 *     M = m + 1; phi = dispersion; factor = R, an M x M lower-triangular matrix in HOST memory, entry (j, k) at
 *     [j * factor_ld + k], factor_ld >= M, with inverse(info) = R^T R for the info of section 2g.  Its strict upper
 *     triangle is never read.  One bit of `kinds` per kind, in this order (bit 0 first):
 *         BESSX_DIAG_LEVERAGE      h_i = v_i * sum_j t_ij^2,   t_ij = sum_{k <= j} R_jk z_ik
 *         BESSX_DIAG_RESPONSE      y_i - mu_i
 *         BESSX_DIAG_PEARSON       rp_i = sqrt(w_i) (y_i - mu_i) / sqrt(V_i)
 *         BESSX_DIAG_DEVIANCE      rd_i = sign(y_i - mu_i) * sqrt(w_i * max(d_i, 0)),   sign(0) = 0
 *         BESSX_DIAG_STD_PEARSON   rp_i / sqrt(phi (1 - h_i))
 *         BESSX_DIAG_STD_DEVIANCE  rd_i / sqrt(phi (1 - h_i))
 *         BESSX_DIAG_COOKS         rp_i^2 h_i / (phi M (1 - h_i)^2)
 *     link         V_i                                   d_i                                       (0 log 0 = 0)
 *     _IDENTITY    1                                     (y_i - eta_i)^2
 *     _LOGISTIC    t / (1 + t)^2 = p_i (1 - p_i)         2 [f(eta_i, y_i) + y_i log y_i + (1 - y_i) log(1 - y_i)]
 *     _POISSON     exp(eta_i)                            2 [f(eta_i, y_i) + y_i log y_i - y_i]
 *     with f the loss term of section 2d.  There is no clamp besides max(d_i, 0): h_i = 1, an underflowed V_i or a NaN
 *     inside the support view give what IEEE arithmetic gives.  A row of weight 0 has h_i = 0 and residuals 0 where
 *     the other factor is finite.  Rows past n, columns outside the support and the padding of the last tile are not
 *     read; m = 0 is valid (z = (1)) and reads nothing of x.
 *     out receives the K requested kinds in ascending bit order, kind slot s at out + s * out_ld, out_ld >= n: device
 *     memory of x's device when out_on_device != 0 (checked as in section 2c), else host memory.
 *     Two steps.  The predictor pass writes the residuals (and v_i); it is the whole call when no kind needs the
 *     leverage, and factor may then be null.  It always runs the threads-along-rows loop of sections 2c / 2d, also for a
 *     row-contiguous x, so that eta_i is the same bits under every layout of x (for a row-contiguous x, sections 2c to
 *     2g add the support's products in another order).  The second step forms T = Z R^T in 16 x 16 tiles on the fp64
 *     matrix cores from x in place, only the steps at or below each tile's diagonal, squares and adds per row in a
 *     fixed order and writes h_i and the kinds derived from it; the factor is uploaded once per call, packed in the
 *     order the lanes read it.  Nothing n x M is stored anywhere and there are no floating-point atomics.  A row's
 *     results depend on that row's values, R, phi and M alone: they are the same bits wherever the row lies in x,
 *     whatever n is, and under every layout of the same dtype.
 *     m + 1 <= 1024: a larger m is BESSX_ERR_UNSUPPORTED.  Every argument error is found before any device call
 *     (BESSX_ERR_ARG: the messages of sections 2d / 2g; kinds zero or with unknown bits; a kind that needs the leverage
 *     with a null factor; a dispersion that is not finite and positive when a kind uses it; a non-finite entry in the
 *     lower triangle of the factor).  Scratch memory (bessx_diag_workspace doubles, the model, host y / weight, a K x n
 *     staging buffer for a host out) is released before the call returns: counters 38 / 39 are back at their earlier
 *     values.  bessx_diag_workspace needs no device: the doubles of v, of the residual vectors that are needed but not
 *     requested, and of the packed factor.
 * ------------------------------------------------------------------------------------- */
enum {
  BESSX_DIAG_LEVERAGE = 1,
  BESSX_DIAG_RESPONSE = 2,
  BESSX_DIAG_PEARSON = 4,
  BESSX_DIAG_DEVIANCE = 8,
  BESSX_DIAG_STD_PEARSON = 16,
  BESSX_DIAG_STD_DEVIANCE = 32,
  BESSX_DIAG_COOKS = 64
};
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  double coef0;
  int link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_stride;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  const double *factor;
  long long factor_ld;
  double dispersion;
  unsigned kinds;
  double *out;
  long long out_ld;
  int out_on_device;
  void *stream;
} bessx_diag_input;
int bessx_diag_device(const bessx_diag_input *in);
int bessx_diag_workspace(int n, int m, unsigned kinds, long long *doubles);
/* ---------------------------------------------------------------------------------------
 * 2j. Residuals, dfbeta and case influence of ONE Cox model on an X already in GPU memory (bessx_k_coxdiag.hip): the Cox
 *     counterpart of section 2i.  Stateless like sections 2c to 2i.  x, n, p, cols, m, beta, time, status, weight, ties,
 *     stream and the notation (positions k, r(k), e, wd, S0, u_k, H, v, g): section 2h.  Weights act on the event terms
 *     only.  With dh_p = sum_{k : r(k) = p} wd_k / S0(p), the hazard increment at position p, and the m-vector
 *     A_l = sum_{p <= l} dh_p u_p (a forward prefix sum of a quantity that comes from the suffix scan), one bit of
 *     `kinds` per kind:
 *         BESSX_COX_DIAG_MARTINGALE    g_k = wd_k - v_k                                                          n
 *         BESSX_COX_DIAG_DEVIANCE      sign(g_k) sqrt(2 max(v_k - wd_k + wd_k log(wd_k / v_k), 0))               n
 *                                      (0 log 0 = 0, sign(0) = 0)
 *         BESSX_COX_DIAG_SCORE         L_k = g_k x_k - wd_k u_{r(k)} + e_k A_k                                   n x m
 *                                      = wd_k (x_k - u_k) - e_k sum_{j : r(j) <= k} (wd_j / S0(j)) (x_k - u_j); its
 *                                      column sums are section 2h's score
 *         BESSX_COX_DIAG_DFBETA        L_k C,  C = cinv = inverse(info), symmetric                               n x m
 *         BESSX_COX_DIAG_DISPLACEMENT  L_k^T C L_k = sum_j t_kj^2,  t_k = R L_k,  R = factor, C = R^T R          n
 *         BESSX_COX_DIAG_SCHOENFELD    x_{k_j} - u_{k_j} for the J rows with status = 1, in POSITION order       J x m
 *     Results are in ROW order except schoenfeld.  factor (lower triangular, its strict upper triangle is never read) and
 *     cinv are m x m in HOST memory, entry (j, k) at [j * ld + k], ld >= m; each is needed only by its kind.
 *     out_rows receives the requested n-vector kinds (martingale, deviance, displacement) in ascending bit order, slot
 *     s at out_rows + s * out_rows_ld, ld >= n; out_score and out_dfbeta hold column c at + c * ld, ld >= n;
 *     out_schoenfeld holds column c at + c * ld, ld >= J.  They are device memory of x's device when out_on_device != 0
 *     (checked as in section 2c), else host memory.  event_rows (HOST memory, J ints, may be null) receives the row of
 *     every schoenfeld row; *n_event_rows = J.  J is the number of rows with status = 1, which the caller counts to
 *     size out_schoenfeld.
 *     Apart from the clamp of eta and the max(., 0) of the deviance there is no clamp; a NaN inside the support view
 *     propagates by IEEE rules.  m = 0 is valid: martingale and deviance are the null model's, displacement is 0, the
 *     matrix kinds are empty and nothing of x is read.  J = 0 is valid: v = g = 0, L = 0, schoenfeld has no rows.
 *     The predictor pass, S0, H, W = e x, the means U, v and g are section 2h's launches as they are.  New: the
 *     increments dh_p u_p and their forward scan per column (two launches, additions only, fixed order), L formed in
 *     place over A from the exact elements of x (the third pass over the support of x: predictor, the gather of W, this
 *     one; schoenfeld reads the J event rows once more), and L P^T in 16 x 16 tiles on the fp64 matrix cores with P = R
 *     (only the k-steps at or below each tile's diagonal, squares added per row in a fixed order) or P = C (every
 *     k-step, tiles stored).  No n x m intermediate besides W and A / L, no floating-point atomics: the same call
 *     gives the same bits, and a row's dfbeta and displacement depend on that row's L and P alone.
 *     Scratch memory (bessx_cox_diag_workspace; no device needed): about (2 m + 6) n + J m doubles when score, dfbeta,
 *     displacement or schoenfeld is asked for, n-vectors only when just martingale / deviance are (then no gather, no
 *     U and no A are formed); released before the call returns: counters 38 / 39 are back at their earlier values.
 *     m + 1 <= 1024 as in section 2h: a larger m is BESSX_ERR_UNSUPPORTED.  Every argument error is found before any
 *     device call (BESSX_ERR_ARG: the messages of sections 2e / 2g / 2h; kinds zero or with unknown bits; a requested
 *     kind whose output, factor or cinv pointer is null; a non-finite entry in the read part of factor / cinv).
 * ------------------------------------------------------------------------------------- */
enum {
  BESSX_COX_DIAG_MARTINGALE = 1,
  BESSX_COX_DIAG_DEVIANCE = 2,
  BESSX_COX_DIAG_SCORE = 4,
  BESSX_COX_DIAG_DFBETA = 8,
  BESSX_COX_DIAG_DISPLACEMENT = 16,
  BESSX_COX_DIAG_SCHOENFELD = 32
};
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  const double *factor;
  long long factor_ld;
  const double *cinv;
  long long cinv_ld;
  unsigned kinds;
  double *out_rows;
  long long out_rows_ld;
  double *out_score;
  long long out_score_ld;
  double *out_dfbeta;
  long long out_dfbeta_ld;
  double *out_schoenfeld;
  long long out_schoenfeld_ld;
  int *event_rows;
  int out_on_device;
  void *stream;
} bessx_cox_diag_input;
int bessx_cox_diag_device(const bessx_cox_diag_input *in, int *n_event_rows);
int bessx_cox_diag_workspace(int n, int m, int n_event_rows, unsigned kinds, long long *doubles);
/* ---------------------------------------------------------------------------------------
 * 2k. The "meat" of a robust (Huber-White sandwich) or cluster-robust covariance on an X already in GPU memory
 *     (bessx_k_sandwich.hip).  Stateless like sections 2c to 2j.  Notation of section 2g: z_i = (1, x(i, cols[0]), ...),
 *     M = m + 1, v_i and g_i the working and score weights of the link, info = sum_i v_i z_i z_i^T.  With weights
 *     g_i = w_i (y_i - mu_i), so the meat carries w_i^2: the ESTIMATING-FUNCTION convention (weights are part of the
 *     estimating equation, not frequencies).
 *         row scalar   BESSX_HC0, BESSX_HC1: u_i = g_i;  BESSX_HC2: u_i = g_i / sqrt(1 - h_i);  BESSX_HC3: u_i = g_i /
 *                      (1 - h_i), with h_i the leverage of section 2i from the same factor R (inverse(info) = R^T R).
 *                      No clamp: h_i = 1 gives what IEEE arithmetic gives.
 *         meat         B = sum_i u_i^2 z_i z_i^T without clusters;  with cluster labels (n integers, any values, any
 *                      order) B = sum_g s_g s_g^T, s_g = sum_{i in g} u_i z_i.  M x M, entry (j, k) at [j * meat_ld + k],
 *                      both triangles written, exact mirrors.
 *     The covariance c * inverse(info) B inverse(info) and its scale factor c are the host's business (capi.py:
 *     sandwich_table); BESSX_HC0 and BESSX_HC1 give the same B.  Cluster labels with BESSX_HC2 / BESSX_HC3 are
 *     BESSX_ERR_ARG (the block-leverage corrections are not built).  A row or a cluster of weight 0 is a row / a cluster.
 *
 *     bessx_meat_device is the generic primitive: B and sums = sum_g s_g (without clusters sum_i u_i z_i) for a source
 *     matrix x (as in section 2c), a support cols, intercept != 0 (z has the leading 1) or 0 (z_i = x(i, cols), M = m >=
 *     1: a dense source such as the Cox score residuals L of section 2j), an optional u (n doubles with unit stride, host
 *     or device; both null = ones) and optional labels (host int64, or a device vector of BESSX_I64 / BESSX_I32 with an
 *     element stride, which is copied to the host; stride 0: one element is read and stands for every row).  *n_clusters = G, or 0 without labels.
 *     bessx_sandwich_device is the GLM route in one call, with no host round trip between the predictor pass and the
 *     meat: the arguments of section 2g plus kind, the factor R (HOST, as in section 2i; needed by BESSX_HC2 / _HC3
 *     only) and the labels.  info, score, *loss and *sum_w are section 2g's for the same arguments, bit for bit.
 *
 *     How: the host sorts the rows by label (std::stable_sort: a cluster's rows keep their order) and cuts every cluster
 *     into runs of at most 64 rows.  One kernel forms S(g, a) = sum_{i in g} u_i z_ia (G x M, column-contiguous) from x
 *     in place: a run is a chain of FMAs in row order, a cluster of several runs adds its runs' partial sums in run
 *     order -- min(r, 64) + ceil(r / 64) - 1 additions for a cluster of r rows, so the bits of S(g, :) depend on the
 *     cluster's rows in their original order and on u alone (not on the layout of x, on n, on where the cluster lies
 *     or on the other clusters).  Three access shapes with the same arithmetic: 16-byte loads (labels already sorted,
 *     column-contiguous aligned source), element loads at any strides, and a row-contiguous source with lanes across
 *     the support.  u and v come from a predictor pass with threads along rows under every layout.  B is then section
 *     2g's matrix-core sweep over S (columns 1 .. M - 1, with S(:, 0) as the score weight) plus one fixed-order sum for
 *     B(0, 0) (ceil(G / 256) + 8 additions); without clusters it is that sweep over x in place with u_i^2 as the
 *     working weight (intercept == 0 without clusters: the sweep runs over x in place with column cols[0], copied to an
 *     n-vector, as the score weight; only with a u is every row its own cluster and S = u x an n x m copy).  No
 *     floating-point atomics: the same call gives the same bits.  The constant entry is not read, nothing outside the
 *     n x m view is read, a NaN inside it propagates.  m + intercept <= 1024, else BESSX_ERR_UNSUPPORTED; every
 *     argument error is found before any device call.  Outputs are device memory of x's device when out_on_device != 0.
 *     bessx_sandwich_workspace needs no device: the doubles of device scratch of a bessx_sandwich_device call (an upper
 *     bound for n_clusters clusters the longest of which has max_cluster_rows rows; n_clusters = 0: no labels), the row
 *     split of the sweep over x (section 2g's for (n, m)) and of the sweep over S (that of (n_clusters, m); 0, 0 without
 *     labels), the additions behind an entry of S for a cluster of max_cluster_rows rows, and those behind B(0, 0).
 * ------------------------------------------------------------------------------------- */
enum { BESSX_HC0 = 0, BESSX_HC1 = 1, BESSX_HC2 = 2, BESSX_HC3 = 3 };
enum { BESSX_I64 = 0, BESSX_I32 = 1 };
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  int intercept;
  const double *u_host;
  const double *u_dev;
  const long long *cluster_host;
  const void *cluster_dev;
  int cluster_dtype;
  long long cluster_stride;
  double *meat;
  long long meat_ld;
  double *sums;
  int out_on_device;
  void *stream;
} bessx_meat_input;
int bessx_meat_device(const bessx_meat_input *in, int *n_clusters);
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  double coef0;
  int link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_stride;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  int kind;
  const double *factor;
  long long factor_ld;
  const long long *cluster_host;
  const void *cluster_dev;
  int cluster_dtype;
  long long cluster_stride;
  double *info;
  long long info_ld;
  double *score;
  double *meat;
  long long meat_ld;
  int out_on_device;
  void *stream;
} bessx_sandwich_input;
int bessx_sandwich_device(const bessx_sandwich_input *in, double *loss, double *sum_w, int *n_clusters);
int bessx_sandwich_workspace(int x_dtype, long long x_row_stride, long long x_col_stride, int n, int m, int link,
                             int weighted, int kind, int n_clusters, int max_cluster_rows, long long *doubles,
                             long long *rows_per_slab, int *slabs, long long *cluster_rows_per_slab, int *cluster_slabs,
                             int *sum_depth, int *sq_depth);
/* ---------------------------------------------------------------------------------------
 * 2l. Rao score tests of candidate columns against ONE fitted model on an X already in GPU memory
 *     (bessx_k_addscore.hip): did the selection leave out a column that matters?  Stateless like sections 2c to 2k.  x,
 *     n, p, cols, m, beta, coef0, link, y, weight, stream, info, info_ld, score, loss, sum_w: section 2g (info and score
 *     are HOST memory here); v_i, g_i, z_i, M = m + 1 as there.  Candidates: q ascending distinct column numbers in HOST
 *     memory, or null = all p columns (q = p).  factor = R, M x M lower triangular in HOST memory as in section 2i
 *     (inverse(info) = R^T R; its strict upper triangle is never read), and r = R^T (R score) = inverse(info) score,
 *     formed on the host in fp64.  For candidate j with column x_j:
 *         u_j = sum_i g_i x_ij                 raw score
 *         c_j = sum_i v_i x_ij z_i             cross information, M entries; cross[j * cross_ld + k], cross_ld >= M
 *         d_j = sum_i v_i x_ij^2               curvature
 *         s_j = || R c_j ||^2                  curvature explained by the support
 *         a_j = c_j . r                        shift of the score (0 at the unpenalised optimum)
 *     The score statistic is (u_j - a_j)^2 / (dispersion (d_j - s_j)): the two subtractions, which can cancel, are left
 *     to the caller's fp64 host code.  A candidate that is in the support has d_j - s_j = rounding noise.  factor null:
 *     s and a are not formed (and may be null); cross null: c_j is not returned.  u, d, s, a (q values each) and cross
 *     are device memory of x's device when out_on_device != 0 (checked as in section 2c), else host memory.
 *     Steps: the row weights v, g by the threads-along-rows predictor pass (the same bits under every layout of x);
 *     info, score, loss and sum_w by section 2g's launches (the same bits as bessx_info_device); the panel P = (v_i z_i,
 *     g_i, zeros) of n x Mp doubles, Mp = 16 ceil((M + 1) / 16), written once -- the one place where the support is
 *     gathered; X_J^T P in 16 x 16 tiles on the fp64 matrix cores with the candidates read from x in place and P shared
 *     by four candidate tile rows through double-buffered LDS; a fixed-order addition of the row slabs' partials; and
 *     C Rx^T on the matrix cores (Rx = R with r appended as one more row, only the steps at or below each tile's
 *     diagonal) whose squares are added per candidate in a fixed order.  No floating-point atomics: the same call gives
 *     the same bits, and u, d, s, a, cross are the same bits under every layout of the same element type.  Rows past n,
 *     columns that are neither in the support nor candidates and the padding of tiles are not read; a NaN inside the
 *     view propagates by IEEE rules.  No x-sized temporary is made: candidates are processed in blocks of
 *     candidate_block columns (0 = the library's choice, else a positive multiple of 16), so scratch memory is 2 n + n_pad
 *     Mp doubles plus a block workspace that does not depend on p.
 *     bessx_addscore_workspace needs no device: *doubles of scratch memory in all, the row split (*rows_per_slab,
 *     *slabs: a function of n, m, q and candidate_block alone), the *block of candidates used, the *block_doubles of it
 *     that do not depend on p, and *sum_depth, the additions behind one s_j.  An entry of u, c or d is a chain of at
 *     most rows_per_slab + ceil(slabs / 16) + 4 additions.
 *     m + 1 <= 1024: a larger m is BESSX_ERR_UNSUPPORTED; q >= 1; n <= 2^31 - 1.  Every argument error is found before any
 *     device call (BESSX_ERR_ARG: the messages of sections 2d / 2g / 2i; candidates not ascending and distinct or not
 *     columns of x; q != p without a list; a candidate_block that is not a multiple of 16).  Scratch memory is released
 *     before the call returns.  Tests of groups of columns with more than one degree of freedom: section 2n.  Cox
 *     models: section 2m.  Out of scope: any correction for selection.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  double coef0;
  int link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_stride;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  const double *factor;
  long long factor_ld;
  const int *candidates;
  int q;
  int candidate_block;
  double *info;
  long long info_ld;
  double *score;
  double *u;
  double *d;
  double *s;
  double *a;
  double *cross;
  long long cross_ld;
  int out_on_device;
  void *stream;
} bessx_addscore_input;
int bessx_addscore_device(const bessx_addscore_input *in, double *loss, double *sum_w);
int bessx_addscore_workspace(int n, int m, int q, int candidate_block, long long *doubles, long long *rows_per_slab,
                             int *slabs, int *block, long long *block_doubles, int *sum_depth);
/* ---------------------------------------------------------------------------------------
 * 2m. Rao score tests of candidate columns against ONE Cox model on an X already in GPU memory
 *     (bessx_k_coxaddscore.hip): section 2l's question for the model of section 2h.  Stateless like sections 2c to 2l.
 *     x, n, p, cols, m, beta, time, status, weight, ties, stream, loglik, n_events, residual_sum and the definitions of
 *     positions l, r(k), e, wd, S0, H, v, g: section 2h; info (m x m, info_ld >= m) and score are HOST memory here and,
 *     with loglik, n_events and residual_sum, bit for bit those of bessx_cox_info_device for the same arguments.
 *     candidates, q, candidate_block, out_on_device: section 2l.  factor = R, m x m lower triangular in HOST memory
 *     (inverse(info) = R^T R; its strict upper triangle is never read), r = R^T (R score).  With dh_p = sum_{k : r(k) = p}
 *     wd_k / S0(p), u_p = S1(p) / S0(p) the risk-set mean over the support and A_l = sum_{p <= l} dh_p u_p (section 2j), for
 *     candidate j with entries x_lj at position l -- row j of the score and of the observed information of the model
 *     extended by column j at coefficient 0:
 *         u_j = sum_l g_l x_lj                                   raw score
 *         c_j = sum_l x_lj (v_l x_l - e_l A_l)                   cross information with the support, m entries
 *         d_j = sum_l v_l x_lj^2                                 first curvature term
 *         t_j = sum_p (dh_p / S0(p)) (sum_{l >= p} e_l x_lj)^2   risk-set term: the information's diagonal entry is d_j - t_j
 *         s_j = || R c_j ||^2,   a_j = c_j . r
 *     The score statistic is (u_j - a_j)^2 / ((d_j - t_j) - s_j), chi-square with 1 degree of freedom, dispersion 1; the
 *     subtractions, which can cancel, are left to the caller's fp64 host code (d - t loses digits for columns far from
 *     centred: section 2h's G1 - G2 caveat).  u, d, t, s, a: q values each; cross: q rows of m + 1 values, cross[j *
 *     cross_ld] = sum_l v_l x_lj (the panel's weight column, not part of the statistic) followed by the m entries of c_j,
 *     cross_ld >= m + 1; null: not returned.  factor null: s and a are not formed (and may be null).  m = 0 is the test of
 *     every column against the null model: s = a = 0 and the factor is not read.  No event at all: every output is 0.
 *     Steps: section 2h's launches for info, score and loglik; where x is row-contiguous the predictor pass is repeated with
 *     threads along rows, so that e and everything after it are the same bits under every layout; section 2j's A; the
 *     panel P = (v_i, v_i x_i - e_i A_pos(i), g_i, zeros) in section 2l's layout, from which section 2l's kernels form u,
 *     c, d on the fp64 matrix cores and s, a from the factor packed with a zero row and column in front; and t by one
 *     streaming pass over the candidate columns: with a_l = e_l x_lj and Cc_l = sum_{p <= l} dh_p / S0(p),
 *     t_j = sum_l a_l (a_l Cc_l + 2 sum_{l' < l} Cc_l' a_l'), a recurrence per candidate over slabs of positions whose
 *     three partial numbers per slab are added in ascending order with a carry.  No n x q temporary, no risk-set mean of a
 *     candidate, no floating-point atomics: the same call gives the same bits, and u, d, t, s, a, cross are the same bits
 *     under every layout of the same element type.  A NaN inside a candidate column reaches that candidate only.
 *     bessx_cox_addscore_workspace needs no device: *doubles of scratch memory in all for J = n_event_rows, the
 *     *block_doubles of it that do not depend on p, the row split of the matrix-core pass (rows_per_slab[0], slabs[0])
 *     and of the risk-set pass (rows_per_slab[1], slabs[1]) -- functions of n, m, q and candidate_block alone --, the
 *     *block of candidates used, *sum_depth = the additions behind one s_j, chain[0] = the longest chain of additions
 *     behind an entry of u, c, d (rows_per_slab[0] + ceil(slabs[0] / 16) + 4) and chain[1] behind a t_j.
 *     m + 1 <= 1024: a larger m is BESSX_ERR_UNSUPPORTED; q >= 1; n <= 2^31 - 1.  Every argument error is found before any
 *     device call (BESSX_ERR_ARG: the messages of sections 2e / 2h / 2l).  Scratch memory is released before the call
 *     returns.  Tests of groups of columns with more than one degree of freedom: section 2o.  Out of scope: Efron ties,
 *     strata, any correction for selection.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  const double *factor;
  long long factor_ld;
  const int *candidates;
  int q;
  int candidate_block;
  double *info;
  long long info_ld;
  double *score;
  double *u;
  double *d;
  double *t;
  double *s;
  double *a;
  double *cross;
  long long cross_ld;
  int out_on_device;
  void *stream;
} bessx_cox_addscore_input;
int bessx_cox_addscore_device(const bessx_cox_addscore_input *in, double *loglik, double *n_events, double *residual_sum);
int bessx_cox_addscore_workspace(int n, int m, int n_event_rows, int q, int candidate_block, long long *doubles,
                                 long long *block_doubles, long long *rows_per_slab, int *slabs, int *block,
                                 int *sum_depth, int *chain);
/* ---------------------------------------------------------------------------------------
 * 2n. Rao score tests of GROUPS of candidate columns against ONE fitted model on an X already in GPU memory
 *     (bessx_k_groupscore.hip): did the selection leave out a group -- a dummy-coded factor, a spline basis -- that
 *     matters?  Stateless like sections 2c to 2m.  x, n, p, cols, m, beta, coef0, link, y, weight, stream, info, info_ld,
 *     score, loss, sum_w, factor = R, r, v_i, g_i, z_i, M = m + 1: section 2l.  The p columns are partitioned into
 *     n_groups contiguous groups by group_starts (HOST memory): ascending distinct start columns, group_starts[0] = 0,
 *     group g = columns group_starts[g] .. group_starts[g + 1] - 1, the last group ends at p - 1.  groups: n_tested
 *     ascending distinct group numbers in HOST memory, or null = all groups (n_tested is then not read).  For a tested
 *     group with columns J, d = |J|:
 *         u_g = X_J^T g                        raw score, d values
 *         C_g = X_J^T diag(v) Z                cross information, d x M (not returned)
 *         a_g = C_g r                          shift of the score, d values
 *         D_g = X_J^T diag(v) X_J              curvature, d x d
 *         S_g = (C_g R^T) (C_g R^T)^T          curvature explained by the support, d x d; its diagonal is section 2l's s_j
 *     The score statistic is (u_g - a_g)^T inverse(D_g - S_g) (u_g - a_g) / dispersion, chi-square with d degrees of
 *     freedom: the subtractions, which can cancel, the d x d Cholesky factor and the quadratic form are left to the
 *     caller's fp64 host code.  u and a hold one value per tested column, the tested groups' columns one after another
 *     in ascending order; D and S hold the blocks one after another, block t row-major d x d at offsets[t] doubles, and
 *     every block is exactly symmetric (the upper triangle is formed and mirrored).  offsets (n_tested + 1 values, the
 *     last one the length of D and of S) is always HOST memory; u, a, D, S are device memory of x's device when
 *     out_on_device != 0, else host memory.  factor null: S and a are not formed (and may be null).
 *     Steps: v, g, info, score, loss, sum_w, the panel P, u and the rows of C exactly as in section 2l, by its launches;
 *     the tested columns of a block are tiled 16 per tile in ascending order whatever the group boundaries are, and for
 *     every tile row t the band tiles (t, t) .. (t, t + w) of X^T diag(v) X are formed on the fp64 matrix cores with both
 *     operands read from x in place, w = (widest tested group + 14) / 16 the furthest tile a group reaches beyond the one
 *     it starts in; the row slabs' partials are added in ascending order; T = C Rx^T as in section 2l, written out, its
 *     column M being a; the band tiles T_t T_{t+k}^T on the matrix cores over the columns < M in ascending steps; and a
 *     copy of every group's block out of the two bands.  Above the diagonal an entry of D is always sum_i x_ij (v_i
 *     x_ij') with j < j'.  No floating-point atomics: the same call gives the same bits, and u, a, D, S are the same bits
 *     under every layout of the same element type.  Rows past n, columns outside the support and the tested groups and
 *     the padding of tiles are not read; a NaN inside the view propagates by IEEE rules.  Blocks of candidates hold whole
 *     groups: a block is closed when the next tested group would take it past candidate_block columns (0 = the
 *     library's choice, else a positive multiple of 16), a function of (group_starts, groups, candidate_block) alone;
 *     scratch memory is 2 n + n_pad Mp doubles plus a block workspace that does not depend on p.  The row split of u and
 *     C is section 2l's for the block's number of columns; that of D is a function of n alone.
 *     bessx_groupscore_workspace needs no device: *doubles of scratch memory in all, the *block_doubles of it that do
 *     not depend on p, the row split of u and C for the block with the longest chain (rows_per_slab[0], slabs[0]) and
 *     of D (rows_per_slab[1], slabs[1]), *n_blocks and, where block_first is not null, the first tested group of every
 *     block followed by n_tested (n_blocks + 1 values; room for n_tested + 1), the *band width w, and the longest chains
 *     of additions: depth[0] behind an entry of u or C (rows_per_slab[0] + ceil(slabs[0] / 16) + 4), depth[1] behind an
 *     entry of the score that r is formed from, depth[2] behind an entry of D (rows_per_slab[1] + slabs[1]), depth[3]
 *     behind an entry of S (Mp).
 *     A tested group of more than 64 columns is BESSX_ERR_UNSUPPORTED (the message names the group), as is m + 1 > 1024;
 *     n <= 2^31 - 1.  Every argument error is found before any device call (BESSX_ERR_ARG: the messages of sections 2d /
 *     2g / 2i / 2l; group_starts not ascending from 0 or not columns of x; groups not ascending and distinct or out of
 *     range; a candidate_block that is not a multiple of 16 or is below the widest tested group rounded up to 16).
 *     Scratch memory is released before the call returns.  Cox models: section 2o.  Out of scope: any correction for
 *     selection.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  double coef0;
  int link;
  const double *y_host;
  const void *y_dev;
  int y_dtype;
  long long y_stride;
  const double *weight_host;
  const void *weight_dev;
  int weight_dtype;
  long long weight_stride;
  const double *factor;
  long long factor_ld;
  const int *group_starts;
  int n_groups;
  const int *groups;
  int n_tested;
  int candidate_block;
  double *info;
  long long info_ld;
  double *score;
  double *u;
  double *a;
  double *D;
  double *S;
  long long *offsets;
  int out_on_device;
  void *stream;
} bessx_groupscore_input;
int bessx_groupscore_device(const bessx_groupscore_input *in, double *loss, double *sum_w);
int bessx_groupscore_workspace(int n, int p, int m, const int *group_starts, int n_groups, const int *groups,
                               int n_tested, int candidate_block, long long *doubles, long long *block_doubles,
                               long long *rows_per_slab, int *slabs, int *n_blocks, int *block_first, int *band,
                               int *depth);
/* ---------------------------------------------------------------------------------------
 * 2o. Rao score tests of GROUPS of candidate columns against ONE Cox model on an X already in GPU memory
 *     (bessx_k_coxgroupscore.hip): section 2n's question for the model of section 2h.  Stateless like sections 2c to 2n.
 *     x, n, p, cols, m, beta, time, status, weight, ties, stream, info, info_ld, score, loglik, n_events, residual_sum,
 *     factor = R (m x m, HOST memory), r, the positions l, e, S0, v, g, dh, A: section 2m; group_starts, n_groups, groups,
 *     n_tested, candidate_block, offsets, out_on_device and the layout of u, a and of the blocks: section 2n.  With
 *     cc_p = dh_p / S0(p) and s_p = sum_{l >= p} e_l x_{l,J} (positions in time order), for a tested group with columns J,
 *     d = |J| -- the rows J of the score and the block of the observed information of the model extended by the group at
 *     coefficient 0:
 *         u_g = X_J^T g                        raw score, d values
 *         C_g = X_J^T P                        cross information with the support, d x (m + 1) (not returned); P = section
 *                                              2m's panel, rows (v_i, v_i x_i - e_i A_pos(i))
 *         a_g = C_g r                          shift of the score, d values
 *         D_g = X_J^T diag(v) X_J              first curvature term, d x d; its diagonal is section 2m's d_j
 *         T_g = sum_p cc_p s_p s_p^T           risk-set term, d x d; its diagonal is section 2m's t_j
 *         S_g = (C_g R^T) (C_g R^T)^T          curvature explained by the support, d x d; its diagonal is section 2m's s_j
 *     The information's block is (D_g - T_g) - S_g and the score statistic (u_g - a_g)^T inverse((D_g - T_g) - S_g) (u_g -
 *     a_g), chi-square with d degrees of freedom, dispersion 1: the subtractions, which can cancel (D - T loses digits
 *     for columns far from centred, section 2h's caveat), the Cholesky factor and the quadratic form are left to the
 *     caller's fp64 host code.  factor null: S and a are not formed (and may be null).  m = 0 is the test against the null
 *     model: S = 0, a = 0 and the factor is not read.
 *     Steps: sections 2h's, 2j's and 2m's launches for info, score, loglik, e, S0, v, g, A and the panel, unchanged;
 *     section 2n's launches for u, the rows of C, the band of D (v in row order), T_C = C Rx^T with section 2m's zero row
 *     and column in the factor, the band of S, a and the extraction, unchanged; and the band of T by this section's
 *     kernels: the tested columns of a block tiled 16 per tile as in section 2n, one wave per (tile row, slab of
 *     positions) walking its slab from the last position to the first, reading row rowof[l] of x in place, keeping the
 *     running suffix sum of each of its columns inside the slab and feeding it, and cc times it, to the fp64 matrix
 *     cores for its own tile and the w neighbour tiles; per slab s it writes Q_s = sum cc_p s_loc s_loc^T (band), A_s =
 *     sum e_l x_l, B_s = sum cc_p s_loc,p and sigma_s = sum cc_p, and a finish kernel adds Q_s + c_s B_s^T + B_s c_s^T +
 *     sigma_s c_s c_s^T over the slabs in descending order with c_s = sum_{s' > s} A_s'.  No n x q temporary, no
 *     floating-point atomics: the same call gives the same bits, and u, a, D, T, S are the same bits under every layout
 *     of the same element type and under every candidate_block (the position split is a function of n alone).  Rows past
 *     n, columns outside the support and the tested groups and the padding of tiles are not read.
 *     bessx_cox_groupscore_workspace needs no device: *doubles of scratch memory in all for J = n_event_rows, the
 *     *block_doubles of it that do not depend on p, the row split of u and C (rows_per_slab[0], slabs[0]), of D
 *     (rows_per_slab[1], slabs[1]) and the position split of T (rows_per_slab[2], slabs[2]), *n_blocks, block_first and
 *     *band as in section 2n, and the longest chains: depth[0] .. depth[3] as in section 2n (depth[1]: the score behind r,
 *     summed over the support as candidates) and depth[4] = t_depth, the roundings behind a term of an entry of T.
 *     A tested group of more than 64 columns is BESSX_ERR_UNSUPPORTED, as is m + 1 > 1024; n <= 2^31 - 1.  Every argument
 *     error is found before any device call (BESSX_ERR_ARG: the messages of sections 2h, 2m and 2n).  Scratch memory is
 *     released before the call returns.  Out of scope: Efron ties, strata, any correction for selection.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  const double *factor;
  long long factor_ld;
  const int *group_starts;
  int n_groups;
  const int *groups;
  int n_tested;
  int candidate_block;
  double *info;
  long long info_ld;
  double *score;
  double *u;
  double *a;
  double *D;
  double *T;
  double *S;
  long long *offsets;
  int out_on_device;
  void *stream;
} bessx_cox_groupscore_input;
int bessx_cox_groupscore_device(const bessx_cox_groupscore_input *in, double *loglik, double *n_events,
                                double *residual_sum);
int bessx_cox_groupscore_workspace(int n, int p, int m, int n_event_rows, const int *group_starts, int n_groups,
                                   const int *groups, int n_tested, int candidate_block, long long *doubles,
                                   long long *block_doubles, long long *rows_per_slab, int *slabs, int *n_blocks,
                                   int *block_first, int *band, int *depth);
/* ---------------------------------------------------------------------------------------
 * 2p. The time-dependent Brier score of R Cox models under inverse-probability-of-censoring weights (Graf et al. 1999)
 *     on an X already in GPU memory (bessx_k_coxbrier.hip): how good the curves of section 2f are, without storing one.
 *     Stateless like sections 2c to 2o.  x, n, p, cols, m, B (m x R, HOST memory), R, stream: section 2e; no intercept;
 *     eta(i, r) = sum_k x(i, cols[k]) * B[k * R + r], e(i, r) = exp(clamp(eta(i, r), -30, 30)).  hg: R x T doubles in HOST
 *     memory, MODEL-major (hg[r * T + j] = the baseline cumulative hazard of model r at times[j], >= 0: the caller does the
 *     step-function lookup); times: T >= 1 doubles (any order; no NaN); time (n), row_a (n, >= 0, finite), time_b (T, >= 0,
 *     finite) and weight (n, >= 0, or NULL = ones) in HOST memory.  With z = hg[r * T + j] * e(i, r):
 *         term(i, j, r) = row_a[i] * exp(-z)^2              when time[i] <= times[j]   (inclusive)
 *                       = time_b[j] * (-expm1(-z))^2        otherwise
 *         bs[j * R + r] = (1 / W) sum_i w_i term(i, j, r),  W = *sum_w = sum_i w_i (added on the host in row order)
 *     One transcendental per element; 1 - S is never formed by a rounded subtraction.  row_a and time_b are plain arrays:
 *     the entry point does not know how they were made (Kaplan-Meier weights of the censoring distribution, ones, or a
 *     training set's).  Every term is non-negative.  hg = 0 gives exactly (1 / W) sum over time[i] <= times[j] of w_i
 *     row_a[i].  A NaN in a support column makes the scores of exactly the models that use the column NaN.
 *     Steps: the predictor pass of section 2e's loops writes e as R x n in row order; one reduction kernel over (row slabs
 *     of 1024) x models forms every term in registers -- a slab's e, time, w and w * row_a are read once per workgroup, the
 *     lanes lie along the times -- and writes one partial per (slab, model, time); a second kernel adds the slabs in
 *     ascending order and divides by W.  No n x T element is stored; no floating-point atomics; the grids depend on (n, T,
 *     R) alone: the same call gives the same bits.
 *     bessx_cox_brier_workspace needs no device: *doubles of device memory in all (3 n + R n + slabs R T + 2 R T + 2 T), the
 *     row split, and *row_groups = the sums of row groups a workgroup adds for T times (a function of T alone).
 *     R <= 65535, T <= 2^20, n <= 2^31 - 1.  Argument errors (BESSX_ERR_ARG: the messages of section 2e for x / cols /
 *     strides / dtype; a null pointer; T < 1; a NaN in times or time; a negative or NaN hg / weight; a negative or
 *     non-finite row_a / time_b; weights that sum to 0) are found before any device call; without a GPU a call with valid
 *     arguments returns BESSX_ERR_HIP.  Scratch memory is released before the call returns.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  int R;
  const double *hg;
  const double *times;
  int T;
  const double *time;
  const double *row_a;
  const double *time_b;
  const double *weight;
  void *stream;
} bessx_cox_brier_input;
int bessx_cox_brier_device(const bessx_cox_brier_input *in, double *bs, double *sum_w);
int bessx_cox_brier_workspace(int n, int T, int R, long long *doubles, long long *rows_per_slab, long long *slabs,
                              int *row_groups);
/* ---------------------------------------------------------------------------------------
 * 2q. The censoring-robust rank measures of R Cox models on an X already in GPU memory (bessx_k_pairauc.hip): the
 *     numerators of the cumulative/dynamic AUC(t) at T times (Uno et al. 2007; Hung and Chiang 2010) and of Uno's C
 *     (Uno et al. 2011), as weighted counts of ordered pairs of rows.  Stateless like sections 2c to 2p.  x, n, p, cols,
 *     m, B (m x R, HOST memory), R, stream: section 2e; no intercept; eta(i, r) = sum_k x(i, cols[k]) * B[k * R + r].
 *     times: T >= 0 doubles in HOST memory, NON-DECREASING (repeats allowed; no NaN); time, status (0 or 1), row_a
 *     (>= 0, finite: status_i / G(time_i-) for an inverse-probability-of-censoring estimate G, or status itself) and
 *     weight (>= 0, finite, or NULL = ones): n doubles each in HOST memory.  With w_i the weights:
 *         greater[j * R + r] = sum over time_i <= times[j] < time_l of w_i row_a[i] w_l 1(eta_ir > eta_lr)
 *         equal  [j * R + r] = the same with 1(eta_ir = eta_lr)
 *         cases[j] = sum_{time_i <= times[j]} w_i row_a[i],      controls[j] = sum_{time_l > times[j]} w_l
 *     and, when want_uno is not 0 (tau: the truncation time; NaN = none),
 *         uno[3 r], uno[3 r + 1] = sum over status_i = 1, time_i < time_l (strictly), time_i < tau of
 *                                  w_i row_a[i]^2 w_l 1(eta_ir > eta_lr) / 1(eta_ir = eta_lr)
 *         uno[3 r + 2] = *uno_comparable = the same sum without the indicator (the same for every model).
 *     AUC(t_j) = (greater + equal / 2) / (cases * controls) and C = (uno[0] + uno[1] / 2) / uno[2] are the caller's: half
 *     credit for ties in eta is never applied here.  Any of greater / equal / cases / controls may be NULL when T = 0.
 *     Steps: the host sorts the rows by time (stable) and cuts the positions at the T cuts into tiles of at most 1024
 *     that straddle no cut; the predictor pass of section 2e's loops writes eta as R x n in that order; one kernel over
 *     (tiles x models) keeps a tile's eta in registers, streams the later tiles through LDS and adds w_l 1(.) into fp64
 *     accumulators per row, which it reduces in a fixed order into a slot of its own per (model, tile, segment of l); a
 *     second adds the tiles in order and a third the segments on the far side of every cut.  No atomics of any kind, no
 *     n x T and no n x n array; the grids depend on (n, the cuts, R) alone: the same call gives the same bits.  Work is
 *     O(n^2 R) comparisons (twice that with want_uno and T > 0).
 *     bessx_cox_auc_workspace needs no device: *doubles = an upper bound of the device memory of a call in doubles
 *     (R n + 3 n + 2 R tiles_max (T + 1) + 2 R (T + 1), plus the int tables), *tile_rows = 1024, *tiles_max = ceil(n /
 *     1024) + T.  R <= 65535, T <= 1024, n <= 2^31 - 1.  Argument errors (BESSX_ERR_ARG: the messages of section 2e for
 *     x / cols / strides / dtype; a null pointer; T < 0 or T > 1024; times that decrease or hold a NaN; a NaN in time; a
 *     status that is not 0 or 1; a negative or non-finite row_a / weight) are found before any device call; without a GPU
 *     a call with valid arguments returns BESSX_ERR_HIP.  Scratch memory is released before the call returns.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  int R;
  const double *times;
  int T;
  const double *time;
  const double *status;
  const double *row_a;
  const double *weight;
  double tau;
  int want_uno;
  void *stream;
} bessx_cox_auc_input;
int bessx_cox_auc_device(const bessx_cox_auc_input *in, double *greater, double *equal, double *cases, double *controls,
                         double *uno, double *uno_comparable);
int bessx_cox_auc_workspace(int n, int T, int R, long long *doubles, long long *tile_rows, long long *tiles_max);
/* ---------------------------------------------------------------------------------------
 * 2r. The numerators of the ROC AUC of R logistic models on an X already in GPU memory: section 2q's kernels with the
 *     rows cut once, between the classes.  y: n doubles in HOST memory, shared by the models (no NaN); a row is a case
 *     when y_i > 0.5 and a control otherwise.  weight: n doubles >= 0, finite, or NULL = ones.
 *         greater[r] = sum over cases i, controls l of w_i w_l 1(eta_ir > eta_lr),   equal[r]: 1(eta_ir = eta_lr)
 *         *pos_weight = sum of w over the cases,   *neg_weight = sum of w over the controls
 *     AUC = (greater + equal / 2) / (pos_weight * neg_weight) is the caller's.  The intercept moves no rank and is not
 *     taken.  Limits, errors and determinism as in section 2q (T = 1).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  int R;
  const double *y;
  const double *weight;
  void *stream;
} bessx_auc_input;
int bessx_auc_device(const bessx_auc_input *in, double *greater, double *equal, double *pos_weight, double *neg_weight);
/* ---------------------------------------------------------------------------------------
 * 2s. Standard errors and pointwise confidence bands of the cumulative hazard and survival curves of ONE Cox model on an X
 *     already in GPU memory (bessx_k_coxband.hip; Tsiatis 1981, what survival::survfit returns with a Breslow baseline).
 *     Stateless like sections 2c to 2r.  Notation of section 2h: positions k in the stable ascending order of time, r(k),
 *     e = exp(clamp(eta, -30, 30)), wd = w * status, S0_k, u_k = S1_k / S0_k; ties as there.
 *
 *     bessx_cox_hazard_var_device: on the rows the model was fitted to (x, n, p, cols, m, beta, time, status, weight, ties,
 *     stream: section 2h; every weight >= 0) and T >= 1 grid times in HOST memory (any order, repeats allowed, a NaN is
 *     BESSX_ERR_ARG), with K(tau) the positions of time <= tau:
 *         cumhaz[j]          = sum_{k in K} wd_k / S0_k
 *         var0[j]            = sum_{k in K} wd_k / S0_k^2
 *         drift[j * ld + c]  = sum_{k in K} (wd_k / S0_k) u_k[c]            (T x m, drift_ld >= m)
 *     in HOST memory, *n_events = sum of wd.  A grid time before the first time gives exact zeros.  The predictor pass,
 *     S0, the hazard scan (section 2f's launcher: under ties = 1 cumhaz is section 2f's baseline at the grid times, bit
 *     for bit), the gather of W, the means U and the accumulated means (section 2j) are the existing launches as they
 *     are.  New: var0's increment (section 2j's dh with S0 squared, same tie handling), its scan in section 2f's form, and
 *     one gather kernel that reads the three prefix arrays at the last position with time <= tau behind which nothing
 *     is added (the end of the last tie group that holds an event; the host finds it from its sorted times): T (m + 2)
 *     numbers cross the bus.  Additions only, one fixed order: the same call gives the same bits.  m = 0: drift
 *     has no columns and nothing of x beyond section 2h's reads is read.  m + 1 <= 1024 (BESSX_ERR_UNSUPPORTED beyond).
 *     Scratch (bessx_cox_hazard_var_workspace): about (m + 4) n doubles with an event, plus J m for J event rows.
 *
 *     bessx_cox_band_device: for ANY rows x (n x p as in section 2c, read in place, the support's columns only), with
 *     z = x(i, cols), e_i as above, Lambda = cumhaz[j] * e_i, factor = R (m x m lower triangular, HOST memory, element
 *     (j, k) at [j * factor_ld + k], inverse(info) = R^T R for section 2h's info; its strict upper triangle is never read),
 *     t = R z and p_j = R drift[j]:
 *         V(i, j)   = var0[j] + sum_c (p_j[c] - cumhaz[j] * t_c)^2      (= var0 + q^T inverse(info) q, q = drift - z cumhaz)
 *         se_L      = e_i * sqrt(V),    w = z_c * se_L,    r = z_c * sqrt(V) / cumhaz[j]
 *         kind _CUMHAZ:    estimate Lambda, se = se_L;  _PLAIN: max(Lambda - w, 0), Lambda + w;  _LOG: Lambda exp(-r),
 *                          Lambda exp(r);  _LOGLOG: BESSX_ERR_ARG
 *         kind _SURVIVAL:  estimate S = exp(-Lambda), se = S se_L;  _PLAIN: max(S - z_c se, 0), min(S + z_c se, 1);  _LOG:
 *                          exp(-(Lambda + w)), exp(-max(Lambda - w, 0));  _LOGLOG: exp(-Lambda exp(r)), exp(-Lambda exp(-r))
 *     Where cumhaz[j] == 0 (decided by that comparison, never 0 / 0) se is 0 and both bounds are the estimate.  estimate is
 *     section 2f's expression from section 2f's predictor pass: the same bits for the same hg.  The sum of squares is formed
 *     directly (additions of non-negative terms: its expansion cancels for columns that are not centred).  The host forms
 *     p_j in fp64 plain loops in a fixed order; the device forms t in 16 x 16 tiles on the fp64 matrix cores from x in place
 *     (section 2i's operand layout and access shapes, only the k-steps at or below a tile's diagonal) and, as each tile
 *     completes, adds the squares per (row, time) for a chunk of times (*time_chunk of the workspace call: 16 for element
 *     loads, 8 / 4 for 16-byte loads of fp64 / fp32); tiles in ascending order, then the 16 lanes of a DPP row, then var0.
 *     No n x m or n x T intermediate, no floating-point atomics: V(i, .) depends on row i's values and the T-sized inputs
 *     alone, whatever the layout, the row's position or n.  m = 0: V = var0 and the matrix-core kernel is not launched.
 *     what: a non-empty set of BESSX_BAND_ESTIMATE / _SE / _LOWER / _UPPER; out holds K = |what| slabs in that order,
 *     element (i, j) of slab s at [s * out_slab_stride + i * out_row_stride + j * out_col_stride], device memory of x's
 *     device when out_on_device != 0 (every slab checked as in section 2c), else host memory staged through a device
 *     buffer.  z_c >= 0 finite (the normal quantile of the level).  A NaN in a support column of row i reaches the outputs
 *     of row i and nothing else.  Argument errors (BESSX_ERR_ARG: those of section 2f for x / cols / beta / out; a
 *     non-finite or negative cumhaz / var0, a non-finite drift or factor, an unknown kind / conf_type / what, _LOGLOG with
 *     _CUMHAZ) are found before any device call.  m + 1 <= 1024, T <= 65535 (BESSX_ERR_UNSUPPORTED beyond).  Out of scope:
 *     Efron ties, strata, bands simultaneous over time, robust-covariance bands, more than one model per call.
 * ------------------------------------------------------------------------------------- */
enum { BESSX_BAND_PLAIN = 0, BESSX_BAND_LOG = 1, BESSX_BAND_LOGLOG = 2 };
enum { BESSX_BAND_ESTIMATE = 1, BESSX_BAND_SE = 2, BESSX_BAND_LOWER = 4, BESSX_BAND_UPPER = 8 };
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  const double *times;
  int T;
  void *stream;
} bessx_cox_hazard_var_input;
int bessx_cox_hazard_var_device(const bessx_cox_hazard_var_input *in, double *cumhaz, double *var0, double *drift,
                                long long drift_ld, double *n_events);
int bessx_cox_hazard_var_workspace(int n, int m, int n_event_rows, int T, long long *doubles);
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *cumhaz;
  const double *var0;
  const double *drift;
  long long drift_ld;
  int T;
  const double *factor;
  long long factor_ld;
  int kind;
  int conf_type;
  double z_c;
  unsigned what;
  long long out_slab_stride, out_row_stride, out_col_stride;
  int out_on_device;
  void *stream;
} bessx_cox_band_input;
int bessx_cox_band_device(const bessx_cox_band_input *in, double *out);
int bessx_cox_band_workspace(int x_dtype, long long x_row_stride, long long x_col_stride, int n, int m, int T, unsigned what,
                             int out_on_device, long long *doubles, int *time_chunk);
/* ---------------------------------------------------------------------------------------
 * 2t. The test of the proportional-hazards assumption of ONE Cox model on an X already in GPU memory
 *     (bessx_k_coxzph.hip; Grambsch and Therneau 1994 in the exact form survival::cox.zph has used since 3.0, not the
 *     constant-variance approximation).  Stateless like sections 2c to 2s.  x, n, p, cols, m, beta, time, status, weight,
 *     ties, stream: exactly as in section 2h (the vectors in HOST memory); positions, r(k), e, wd, S0, u_k: sections 2e and
 *     2h.  gt: the time transform per row, n doubles in HOST memory, read at the rows with status = 1 only (finite there:
 *     else BESSX_ERR_ARG) and already centred by the caller; g_k its value at position k.  For q = 0, 1, 2
 *         h^q_k = wd_k g_k^q / S0(k),   H^q_l = sum_{k : r(k) <= l} h^q_k,   v^q_l = e_l H^q_l,   a^q_l = wd_l g_l^q - v^q_l
 *         info_q  = G1^q - G2^q,   G1^q = sum_l v^q_l x_l x_l^T,   G2^q = sum_{k : status_k = 1} wd_k g_k^q u_k u_k^T
 *         score_q = sum_l a^q_l x_l        ( = sum_k wd_k g_k^q (x_k - u_k): for q = 1 the g-weighted sum of the Schoenfeld
 *                                            residuals of section 2j )
 *     with wd_k g_k^2 formed as (wd_k g_k) g_k.  info_q = sum_k wd_k g_k^q Var_k(x), the information weighted by g^q.
 *     info0, score0 and loglik are section 2h's info, score and loglik BIT FOR BIT, and where gt is 1 at every event so
 *     are info1, info2 and score1.  The score test of theta = 0 in beta(t) = beta + theta g(t) follows on the host
 *     (score0 taken as 0): D = info2 - info1 inverse(info0) info1, global = score1^T inverse(D) score1 on m degrees of
 *     freedom, and per column score1_j^2 / D_jj on one.  g may be negative: the q = 1 sums are not sums of non-negative
 *     terms, and info_q is a DIFFERENCE as in section 2h.
 *     The predictor pass, the S0 scan, the gather of e x and the means u_k are section 2h's launches, unchanged.  The
 *     three H^q are three runs of section 2f's forward scan.  G1^q for q = 0, 1, 2 is ONE sweep of the matrix-core Gram
 *     over x in place that carries the three weight pairs (the loads and the unweighted operand are shared; each weight
 *     has its own accumulators and gets the bits section 2g's sweep gives with that weight alone), G2^q a second such
 *     sweep over the J x m matrix of the u_k.  No floating-point atomics; block and slab counts depend on (n, m, J)
 *     alone: the same call gives the same bits.
 *     info0, info1, info2: m x m each, entry (j, k) at [j * info_ld + k], info_ld >= m shared by the three, both triangles
 *     written as bit-identical mirrors; score0, score1: m values each.  They are device memory of x's device when
 *     out_on_device != 0 (checked as in section 2c), else host memory; loglik and n_events (= sum_k wd_k) are host
 *     memory.  m = 0 is valid: nothing of x is read, the outputs are untouched and loglik is the null model's.  Without an
 *     event row the matrices and vectors are exact zeros.  m + 1 <= 1024: a larger m is BESSX_ERR_UNSUPPORTED, with every
 *     other argument error (BESSX_ERR_ARG, the messages of sections 2e / 2h) found before any device call.  A NaN INSIDE
 *     the support view is no error and propagates; nothing outside the view is read.  Scratch memory (section 2h's plus
 *     10 n + 3 J doubles and the partials of the two three-weight sweeps: about (m + 15) n + J m doubles plus partials,
 *     bessx_cox_zph_workspace states it) is released before the call returns: counters 38 / 39 are back at their
 *     earlier values.
 *     bessx_cox_zph_workspace needs no device: the doubles of scratch memory and the row splits of the two sweeps as in
 *     bessx_cox_info_workspace (rows_per_slab[0], slabs[0] over n rows, [1] over J rows; 0, 0 for a sweep not launched).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *beta;
  const double *time;
  const double *status;
  const double *weight;
  int ties;
  const double *gt;
  double *info0, *info1, *info2;
  long long info_ld;
  double *score0, *score1;
  int out_on_device;
  void *stream;
} bessx_cox_zph_input;
int bessx_cox_zph_device(const bessx_cox_zph_input *in, double *loglik, double *n_events);
int bessx_cox_zph_workspace(int n, int m, int n_event_rows, long long *doubles, long long *rows_per_slab, int *slabs);
/* ---------------------------------------------------------------------------------------
 * 2u. Restricted mean survival times (RMST) and quantile survival times of ONE Cox model on an X already in GPU memory
 *     (bessx_k_coxrmst.hip): one number per row and horizon / level, and no curve is stored.  Stateless like sections 2c
 *     to 2t.  x, dtype, strides, n, p, cols, m, B, stream: exactly as in section 2f; e_i = exp(clamp(eta_i, -30, 30)) is
 *     that section's predictor pass, unchanged, and ONE such pass serves both parts.  S(t | x_i) = exp(-(H0(t) * e_i)),
 *     every value of it the element bessx_cox_survival_device would write.
 *
 *     RMST.  S is a step function, so RMST_i(tau) = integral_0^tau S(t | x_i) dt is a finite sum, and as in section 2f
 *     the caller does the step-function lookup: hs, wd (K values each, HOST memory) are the baseline cumulative hazard
 *     on, and the width of, the K segments between consecutive breakpoints (0, the baseline's times, the horizons), and
 *     cut (T values, HOST memory) the number of segments in front of each horizon:
 *         rmst(i, j) = sum_{k < cut[j]} wd[k] * exp(-(hs[k] * e_i))
 *     K >= 0 (K = 0: hs and wd may be NULL), 0 <= cut[j] <= K in any order, repeats allowed; cut[j] = 0 gives exactly 0.0.
 *     Each term is formed as fma(wd[k], exp(-(hs[k] * e_i)), acc): one rounding per term.  The segments below the largest
 *     cut are split into pieces that end at every distinct cut and after every 256 segments; a piece is summed in
 *     ascending order from 0, and a row's pieces are added in ascending order from 0: ADDITIONS ONLY in fp64, in an order
 *     fixed by (K, cut) alone, every term entering once, no floating-point atomics.  Given e_i, the bits of a row depend
 *     neither on n, nor on the row's position, nor on the layout or dtype of x, nor on a repeat of the call; two horizons
 *     with the same cut get the same bits, and along ascending cuts a row never decreases.  e_i is section 2f's: its
 *     predictor pass adds the support's products in one order for a row-contiguous x (x_col_stride = 1) and in another
 *     for every other layout, so equal widened values give equal bits within each of the two kinds of layout, for either
 *     dtype, and across them where m <= 1.
 *
 *     Quantiles.  hz, ut (J >= 0 values each, HOST memory): the baseline's cumulative hazards (non-negative and
 *     non-decreasing) and its times; c (Q levels > 0, HOST memory).  With g* = min{ g : fl(hz[g] * e_i) >= c[j] } -- the
 *     product one fp64 multiplication, compared as it stands, found by one binary search per (i, j) over hz in device
 *     memory (multiplication by e_i > 0 is monotone) --
 *         quant(i, j) = ut[g*],     +inf when there is no such g (J = 0 included).
 *     For the q-quantile of the survival time the caller passes c = -log1p(-q): quant is then the first baseline time at
 *     which S(t | x_i) <= 1 - q.  (survival::survfit averages two times where S equals 1 - q exactly; this does not.)
 *
 *     Either part may be absent (T = 0 with rmst NULL; Q = 0 with quant NULL); both absent is BESSX_ERR_ARG.  rmst holds
 *     element (i, j) at [i * rmst_row_stride + j * rmst_col_stride], quant at [i * quant_row_stride + j *
 *     quant_col_stride], and both are handled exactly as out is in section 2f: out_on_device != 0: device memory of x's
 *     device, checked as there; otherwise host memory, staged through a device buffer of the library's own.
 *     A NaN in a support column of row i gives NaN in every output of row i (a horizon with cut 0 included) and nowhere
 *     else; columns outside the support are not read; x is never written.
 *     BESSX_ERR_ARG with text, found before any device call, besides those of section 2f for x / cols / B: a NaN or
 *     negative hs; a wd that is NaN or not positive; a cut outside [0, K]; an hz that decreases, is negative or NaN; a c
 *     that is NaN or not positive; a NaN in ut; a negative stride, or a zero stride along an axis longer than 1; a
 *     negative count or a NULL array with a positive count.  Without a GPU a call with valid arguments returns
 *     BESSX_ERR_HIP.
 *     Scratch memory: n doubles of e; the K' = max(cut) used segments twice, the pieces' starts and 2 T column entries;
 *     the partials, NP * rows doubles with NP <= K' / 256 + T the number of pieces and rows = min(n, max(512, 2^24 / NP
 *     rounded down to a multiple of 512)) the rows taken at a time (at most 2^24 doubles = 128 MiB while NP <= 2^15);
 *     2 J + Q doubles for the quantiles; n * T and n * Q more for host outputs.  There is no n x K and no n x T
 *     temporary.  All of it is released before the call returns: counters 38 / 39 are back at their earlier values.
 *     Measured on an MI355X: n = 200 000, m = 150, K = 139 806, T = 1, Q = 5, fp64 row-major: 27.0 ms
 *     per call to device outputs, of which the partial kernel 17.8 ms (1 572 G terms/s, bound by the fp64 exp).
 *     bessx_cox_survtime_workspace needs no device: *slab = 256, and for the given cuts *pieces = NP, *rows_per_chunk and
 *     *doubles = the doubles of device scratch of a call with device outputs (the quantile part's not included).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void *x;
  int x_dtype;
  long long x_row_stride, x_col_stride;
  int n, p;
  const int *cols;
  int m;
  const double *B;
  const double *hs;
  const double *wd;
  int K;
  const int *cut;
  int T;
  const double *hz;
  const double *ut;
  int J;
  const double *c;
  int Q;
  long long rmst_row_stride, rmst_col_stride;
  long long quant_row_stride, quant_col_stride;
  int out_on_device;
  void *stream;
} bessx_cox_survtime_input;
int bessx_cox_survtime_device(const bessx_cox_survtime_input *in, double *rmst, double *quant);
int bessx_cox_survtime_workspace(int n, const int *cut, int T, int *slab, int *pieces, long long *rows_per_chunk,
                                 long long *doubles);
/* screening_A of src/screening.cpp:68: original column of every kept column (ascending).  Returns the number of
 * kept columns (= p when the session was created without screening, map = identity); writes min(count, cap). */
int bessx_session_get_screening(const bessx_session *s, int *columns, int cap);
/* Screening with groups of size > 1: the kept ORIGINAL group numbers (ascending) = screening_A of the
 * reference for that case; 0 when the session was not screened by groups.  Returns the count, writes min(count, cap). */
int bessx_session_get_screening_groups(const bessx_session *s, int *groups, int cap);
/* coef_norm of src/screening.cpp:60-64 as max_k saw it: one marginal-fit score per ranked unit (original column, or
 * original group when screening by groups), read-only.  DBL_MAX for an always_select unit, +inf for an all-zero LM
 * column, 0.0 for a degenerate logistic / Cox unit; a group wider than the one-block kernels take carries the score
 * of its sub-session fit.  Returns the number of ranked units (0 for a session created without screening), writes
 * min(count, cap).  Costs session creation one device-to-host copy of that many doubles. */
int bessx_session_get_screening_scores(const bessx_session *s, double *scores, int cap);
/* 1 = streaming score pass, 2 = covariance updates: what bessx_problem.score_mode resolved to for this session. */
int bessx_session_score_mode(const bessx_session *s);
/* Diagnostics of the covariance form since the session was created: which = 0 fits that ran chained behind their
 * predecessor, 1 conjugate-gradient solves handed to the Cholesky kernel, 2 passes over X (32-column panel groups),
 * 3 chained fits queued; 4-6 always 0 (background fills and the maintained inverse of round 2: measured, removed);
 * 7 rounds in which the fold fits of cross-validation ran side by side (one fit context per fold), 8 fills that served
 * several parked folds at once, 9 PDAS iterations redone with the exact tie rule, 10 times the Gram column cache was
 * started over since the last path call started, 11 times bessx_session_set_cv had to give the per-fold fit contexts up
 * (allocation or launch failure: the fold fits then run one after another -- slower, same results), 12 fold contexts
 * alive now (K when the fold fits of a CV evaluation run side by side, else 0), 13 fills of a parked fit that went
 * through the fill hook (bessx_session_set_fill_hook), 14 sequential paths run as chunk chains side by side
 * (BESSX_KPATH_CHAINS), 15 candidates re-fitted by their stitching, 16 fills of the shared cache
 * during the chunk phase, 17 chains of the last such path, 18 paths whose stitch gave up (a chunk's refit did not meet its
 * own chain within its budget: the rest of the path was walked as one chain, and the automatic choice of this session is
 * one chain from then on), 19 device nanoseconds of the last all-rows group_XTX pass inside a path call (LM; kernel timing
 * on), 20 / 21 retired, always 0 (chunk phases run as merged launches on one stream and the chains of such phases the
 * host had to finish: measured slower than a stream per chain and removed), 22-24 microseconds the
 * chunked paths spent in their coarse chain / chunk phase / stitch (host clock, summed); round 6: 25 / 26 timed panel
 * launches of ONE 32-column group and their nanoseconds, 27 / 28 the same for launches of TWO groups (one read of X each;
 * reset with bessx_session_score_pass_stats), 29 multi-chain launches of the chunk chains' shared passes over X
 * (fall-through launches included), 30 vector sets those launches served (kernel timing on), 31 batches launched before
 * every chain had arrived (the 50 ms timeout), 32 streams with a hardware queue of their own the PROCESS has created so
 * far (they are recycled across sessions); bessx_session_sequential_path_multi: 33 responses run through the merged
 * engine, 34 responses or parts of responses the host finished through the ordinary path (takeovers, and every response
 * of a path the engine does not apply to), 35 union fills served during merged runs of responses; 36 bytes of X
 * uploaded from host memory, 37 bytes of X ingested from device memory (source bytes, n * p * element size; a
 * session of bessx_session_create_device reports 0 for 36); 38 / 39 bytes of device / pinned host memory the library
 * holds right now in the whole PROCESS (every session, context and drop-in call: what its allocations handed out and
 * have not given back -- back at its earlier value once a session is destroyed), 40 allocation requests the library has
 * made in the process so far (device buffers, pinned buffers, events).  -1 for an unknown id.  s may be NULL for 38-40
 * (they belong to the process). */
long long bessx_session_counter(const bessx_session *s, int which);

/* Metric::set_cv_train_test_mask + cal_cv_group_XTX (src/Metric.h:49-129).  fold_id[i] in [0,K)
 * gives the test fold of row i; fold_id == NULL draws a permutation from mt19937(seed) and cuts
 * it into K contiguous chunks exactly as src/Metric.h:66-78 does. */
int bessx_session_set_cv(bessx_session *s, int K, const int *fold_id, unsigned seed);
/* The test fold of every row as bessx_session_set_cv fixed it (given or drawn): fold_id[0..n).  Lets a caller hand
 * the very same folds to another implementation (the tests feed them to the oracle). */
int bessx_session_get_cv_folds(const bessx_session *s, int *fold_id);

/* Results of a path run.  All pointers are caller-allocated; any of the *_all pointers may be
 * NULL to skip that output.  Candidates are stored in evaluation order. */
typedef struct {
  double *beta;       /* p: best model, de-normalised (src/path.cpp:76-131, :330-388) */
  double coef0, train_loss, ic, lambda;
  int best_T0, best_iters;
  int capacity;       /* candidate slots available in the arrays below */
  int n_candidates;   /* out: candidates evaluated (may exceed capacity; extra ones are not stored) */
  int *cand_T0;       /* capacity */
  double *cand_lambda;/* capacity */
  int *cand_iters;    /* capacity: PDAS iterations (Algorithm::l) of the full-data fit */
  double *cand_train_loss, *cand_ic, *cand_coef0; /* capacity each; coef0 and beta are de-normalised
                                                     like beta_all / coef0_all of the R build */
  int *cand_support;  /* capacity * max_T0 (row per candidate, ascending, -1 padded) */
  double *cand_beta;  /* capacity * max_T0: coefficients matching cand_support */
  int max_T0;         /* row length of cand_support / cand_beta */
  double device_seconds; /* out: wall time of the path on the device side (host clock around the loop) */
  long long n_fits, n_pdas_iters; /* out: Algorithm::fit calls (incl. CV folds) and get_A calls */
} bessx_path_result;

/* sequential_path (src/path.cpp:25-132): sizes x lambdas in snake order, warm-start chain. */
int bessx_session_sequential_path(bessx_session *s, const int *sequence, int sequence_len,
                                  const double *lambda_seq, int lambda_len, int ic_type, int is_cv,
                                  bessx_path_result *res);
/* sequential_path as ONE LINK of a longer warm-start chain (src/path.cpp:60-64: candidate i starts from candidate
 * i-1's model) that several processes walk in pieces -- the k-path chunks of a multi-GPU run (bess_amd/dist.py,
 * StitchedKPath).  in: the model the first candidate starts from = Algorithm::update_beta_init / update_coef0_init
 * (src/Algorithm.h:85-93) with the predecessor's Algorithm::get_beta / get_coef0 (:97-111), NORMALISED scale, column
 * indices of the session; keep_caches != 0: the call continues the job of the previous path call on this session (the
 * cached Gram columns and score sums depend on the data only and stay), 0: it starts cold like every path call.
 * stop_support / stop_beta (optional): candidates the caller already holds for this very sequence, laid out like
 * cand_support / cand_beta of a bessx_path_result (row i = candidate i in evaluation order, stop_row_len entries, -1 / 0
 * padded, caller's column numbering, de-normalised coefficients).  The path stops after the first candidate i whose
 * support equals row i (and whose coefficients agree within stop_rtol when stop_beta is given): from there on the
 * chain the caller holds IS this chain -- same model, hence the same successors.  That candidate is stored;
 * stopped_at = i, or -1 when the whole sequence was walked.  The best model of the result is the best of the
 * candidates evaluated.  out: last_* = the model the NEXT candidate of the chain would start from (normalised;
 * last_len entries, min(last_len, last_cap) written).  Not offered under CV with an initial model (the folds' chains
 * would have to be handed over as well). */
typedef struct {
  const int *init_idx;
  const double *init_val;
  int init_len;
  double init_coef0;
  int keep_caches;
  const int *stop_support;
  const double *stop_beta; /* may be NULL: supports only */
  int stop_rows, stop_row_len;
  double stop_rtol;
  int stopped_at;          /* out */
  int *last_idx;           /* caller-allocated, last_cap entries; may be NULL */
  double *last_val;
  int last_cap;
  int last_len;            /* out */
  double last_coef0;       /* out */
  /* optional LEAD fits (round 6): sparsity levels (ascending, below the link's first) of a warm-start chain that is run
   * on this session IN FRONT of the link, from init_* -- every rank of a multi-GPU k-path walks the same coarse levels
   * the one-GPU path walks (a few fits whose fills bring nearly every Gram column the link will ask for) instead of
   * starting cold at its chunk: no communication, and the link starts from the last lead model.  Their candidates are
   * not returned; NULL / 0: none.  LM only. */
  const int *lead_levels;
  int lead_len;
} bessx_path_chain;
int bessx_session_sequential_path_chain(bessx_session *s, const int *sequence, int sequence_len,
                                        const double *lambda_seq, int lambda_len, int ic_type, int is_cv,
                                        bessx_path_chain *chain, bessx_path_result *res);

/* Many responses against this session's design (LM, model_type 1; bessx_multi.cpp).
 * bessx_session_set_responses: R extra responses, Y n x R, column-major if col_major else row-major.  Each column is
 * prepared exactly like the session's y (weights, data_type centring; src/Data.h:79-93, k_y_prepare).  Replaces any
 * earlier set.  The session's own y is not changed.  BESSX_ERR_ARG for R < 1 or a NaN in Y; BESSX_ERR_UNSUPPORTED
 * for model_type != 1.
 * bessx_session_sequential_path_multi: sequential_path (same arguments and meaning) once per response set by
 * bessx_session_set_responses: res[0..R) in column order, each filled exactly as bessx_session_sequential_path fills its
 * result for a session created with that column as y.  Where the merged-launch engine applies (covariance score mode
 * with a cache that holds every column, one lambda, warm start, ascending levels of at most the k_sel_cgr range, singleton
 * groups) the responses run in batches of up to 256 as chains of ONE merged run that share the Gram column cache and
 * its fills; a response the device stops (tie, Cholesky handoff, ...) is finished on the host through
 * bessx_session_sequential_path_chain from its last recorded model.  Elsewhere the responses run one after another
 * through the ordinary path.  Same results either way.  The session's own response, X^T y and y.y are restored before
 * the call returns.  BESSX_ERR_UNSUPPORTED for is_cv != 0, model_type != 1 and a screening session; BESSX_ERR_ARG before
 * bessx_session_set_responses.  A response whose own path fails (e.g. a constant column: the error code its single-
 * response session returns) fails the whole call with that code; res[] is then incomplete and no response's result may
 * be used.  Counters 33-35 (bessx_session_counter). */
int bessx_session_set_responses(bessx_session *s, const double *Y, int R, int col_major);
/* The same for Y (n x R) in device memory, described like X in bessx_device_input (dtype, element strides, the
 * caller's stream; same ordering and lifetime rules).  Same preparation and results as bessx_session_set_responses. */
int bessx_session_set_responses_device(bessx_session *s, const void *Y, int dtype, long long row_stride,
                                       long long col_stride, int R, void *stream);
int bessx_session_sequential_path_multi(bessx_session *s, const int *sequence, int sequence_len,
                                        const double *lambda_seq, int lambda_len, int ic_type, int is_cv,
                                        bessx_path_result *res);

/* gs_path (src/path.cpp:134-389): integer golden section on [s_min, s_max] then exhaustive sweep. */
int bessx_session_gs_path(bessx_session *s, int s_min, int s_max, int ic_type, int is_cv, bessx_path_result *res);

/* pgs_path (src/path.cpp:1138-1309): Powell search over (s, log lambda) for the L0L2 / bsrr types; line searches
 * by golden section (powell_path 1, n_lambda forced to 100) or on the lambda grid (powell_path 2).  lambda_min /
 * lambda_max are floored at 1e-5 as bessCpp does (src/bess.cpp:176-177).  Candidates = the best point of every
 * line search plus the final re-fit; res->lambda receives the chosen lambda. */
int bessx_session_pgs_path(bessx_session *s, int s_min, int s_max, double lambda_min, double lambda_max, int n_lambda,
                           int powell_path, int ic_type, int is_cv, bessx_path_result *res);

/* Optional trace of every PDAS iteration of every fit of the LAST path run, same layout as the
 * oracle's (oracle/bess_oracle.h): which = 0 geta_meta(int x4: l, T0, train_n, offset) 1 a_flat(int)
 * 2 beta_flat(double) 3 coef0_calls(double) 4 loss_calls(double) 5 ic_calls(double). */
int bessx_session_trace_enable(bessx_session *s, int on);
int bessx_session_trace_size(bessx_session *s, int which);
int bessx_session_trace_copy_int(bessx_session *s, int which, int *out);
int bessx_session_trace_copy_double(bessx_session *s, int which, double *out);

/* Normalisation results (Data::x_mean / x_norm / y_mean, src/Data.h:26-29). */
int bessx_session_get_normalization(bessx_session *s, double *x_mean, double *x_norm, double *y_mean);

/* Timing of the dominant kernel (the X^T r score pass, K1) accumulated since the last reset:
 * HIP events recorded on the session's stream around every launch.  Used by bench.py for the
 * roofline line.  seconds = sum of launch durations, launches = count, bytes = algorithmic
 * bytes (8 * n * p per launch; doubled accumulators read the same bytes). */
int bessx_session_score_pass_stats(bessx_session *s, int reset, double *seconds, long long *launches,
                                   double *algorithmic_bytes);
int bessx_session_enable_kernel_timing(bessx_session *s, int on);
/* Steps of the restricted fits' inner iterations taken since the last reset: IRLS solves of the logistic / Poisson
 * fits (src/Algorithm.h:1148-1204, 1273-1322), Newton steps of the Cox fit (:1377-1490); 0 for LM.  A statistic for
 * bench.py (time per step of the chain between two passes over X). */
int bessx_session_submodel_steps(bessx_session *s, int reset, long long *steps);

/* ---------------------------------------------------------------------------------------
 * 3. One Algorithm::fit (src/Algorithm.h:113-171) on the resident data.
 *    fold = -1: all rows; else the training rows of that CV fold (update_train_mask +
 *    update_group_XTX, src/Metric.h:182-183).  init_* is the warm start (update_beta_init /
 *    update_coef0_init) as a sparse vector of COLUMNS.  Outputs: support[W] ascending, beta[W] with
 *    W = bessx_session_fit_width(s, T0): T0 for singleton groups; with groups of size > 1 (T0 counts groups,
 *    Algorithm::fit returns the columns of the selected groups) the widest T0 groups' column count -- entries beyond
 *    the selected columns are -1 / 0.  coef0,
 *    iters (Algorithm::l), train_loss = the family's train_loss on ALL rows (src/Metric.h:145,266,
 *    426,565), test_loss = the family's CV test loss on the fold's test rows (0 when fold < 0).
 * ------------------------------------------------------------------------------------- */
/* Forget everything a previous fit left on the device beyond the data (score sums, cached Gram columns, fold
 * warm starts): the state a path call starts from (a bessCpp call starts from nothing).  A caller that builds its own
 * path out of bessx_session_fit (bess_amd/dist.py) calls this first, so that a repeated path does not reuse work. */
int bessx_session_reset_caches(bessx_session *s);
int bessx_session_fit_width(const bessx_session *s, int T0); /* -1: T0 outside [1, number of groups] */
int bessx_session_fit(bessx_session *s, int T0, double lambda, int fold, const int *init_idx,
                      const double *init_val, int init_len, double init_coef0, int *support, double *beta,
                      double *coef0, int *iters, double *train_loss, double *test_loss);

/* One evaluation of a cross-validated candidate restricted to SOME folds: Metric::test_loss (src/Metric.h:150-195) for
 * the folds listed (ascending), preceded -- want_full != 0 -- by the full-data Algorithm::fit the path runs before it
 * (src/path.cpp:58, :171).  What one rank of a fold-sharded CV path owns (bess_amd.dist.FoldShardedCV): the fold fits
 * take the library's own route (LM covariance form: the chains side by side on their own streams, one fill of the
 * shared Gram column caches for all parked folds), and start from the session's own per-fold warm starts
 * (cv_initial_model_param.row(k), :177-188; cleared by every path call and by bessx_session_reset_caches).  init_* /
 * init_coef0 = update_beta_init / update_coef0_init as the path sets them before the candidate (the full-data chain's
 * previous model; the fold fits read coef0_init, and beta_init when the session was created without warm start).
 * Outputs: want_full + n_folds records in the order [full,] folds[0], folds[1], ...; record r = support / beta
 * [r * W .. (r+1) * W) with W = bessx_session_fit_width(s, T0), coef0[r], iters[r], train_loss[r], test_loss[r]
 * (0 for the full-data fit) -- the fields of bessx_session_fit. */
int bessx_session_cv_eval(bessx_session *s, int T0, double lambda, int want_full, const int *init_idx,
                          const double *init_val, int init_len, double init_coef0, const int *folds, int n_folds,
                          int *support, double *beta, double *coef0, int *iters, double *train_loss, double *test_loss);

/* Cooperative prefill of the Gram column cache (LM, covariance form of the score pass, all rows; not on sessions with
 * CV folds): several sessions that hold the SAME data -- the ranks of a multi-GPU k-path -- share the passes over X that
 * each of their cold starts would repeat.  Every rank lists the same columns (begin: the cache is started over and slot
 * i goes to cols[i], so slot numbers agree across ranks), forms the Gram columns X^T x_c of ITS groups of 32 (compute),
 * hands the p x 32 blocks out (export; group g = 32 * p doubles, column after column) and takes the others' in (import),
 * then fills the slot-indexed Gram between cached columns once (end).  A path call that follows with
 * bessx_path_chain.keep_caches finds the columns cached.  Cache contents only -- no result depends on it; the blocks
 * are bit-identical to what the rank would have formed itself.  bessx_session_marginal_scores: the sacrifice scores of
 * get_A at beta = 0 (src/Algorithm.h:1109-1123), what the first PDAS iteration of a cold fit ranks -- the list is
 * their top M.  *_on_device: the buffer is device memory of this session's device (else host memory). */
int bessx_session_marginal_scores(bessx_session *s, double *bd /* p */);
int bessx_session_cov_prefill_begin(bessx_session *s, const int *cols, int ncols /* multiple of 32, distinct */);
/* A second list on top of the cache as it is (after a prefill, after fits): the columns -- none of them cached yet --
 * take the next free slots in list order; identical on every rank whose session has done identical work so far. */
int bessx_session_cov_prefill_extend(bessx_session *s, const int *cols, int ncols);
/* bd[p]: the sacrifice scores the last fit's last PDAS iteration ranked; slot_of[p]: cache slot of every column, -1 =
 * not cached.  Either may be NULL.  What a caller needs to choose the next columns worth caching. */
int bessx_session_cov_state(bessx_session *s, double *bd, int *slot_of);
int bessx_session_cov_prefill_compute(bessx_session *s, int g0, int ngroups);
int bessx_session_cov_prefill_export(bessx_session *s, int g0, int ngroups, double *dst, int dst_on_device);
int bessx_session_cov_prefill_import(bessx_session *s, int g0, int ngroups, const double *src, int src_on_device);
int bessx_session_cov_prefill_end(bessx_session *s);
/* Diagnostic, read-only: the Gram columns X^T diag(m_r) x_c that row set r (0 = all rows, k + 1 = the training rows of
 * fold k) holds cached right now, on sessions with and without CV folds, whichever way the folds' caches are filled.
 * cached[i] = 1 if cols[i] is in THAT row set's cache (its own slot map: row set 0's where the folds share their fills);
 * then dst[i * p .. (i + 1) * p) is the column, all p entries, as bessx_session_cov_prefill_export lays a block out.
 * The entries of dst for uncached columns are left as they are.  Waits for the session's streams; changes no state and
 * queues nothing.  BESSX_ERR_UNSUPPORTED outside the covariance form of the LM score pass, BESSX_ERR_ARG for a row set
 * the session does not have or a column outside 0 .. p-1. */
int bessx_session_cov_cache_columns(bessx_session *s, int row_set, const int *cols, int ncols, double *dst, int *cached);
/* Diagnostic, read-only: the score state in device memory.  LM sessions with singleton groups, both forms of the score
 * pass; BESSX_ERR_UNSUPPORTED otherwise.  ctx < 0: the session's own state; ctx >= 0: fold context ctx of the
 * side-by-side CV chains (BESSX_ERR_ARG where the session has none).  Waits for the session's and the fold contexts'
 * streams and copies; allocates nothing, queues nothing and changes no host bookkeeping, so a fit chained ahead on the
 * device stays as it is.  head[BESSX_SCORE_STATE_HEAD]:
 *    0..8  the control block: done, l, T0, k_cur, d_fresh, info, cov_miss, fast_same, serial
 *    9     row set of the fit that block describes (0 = all rows, k + 1 = training rows of fold k; -1: not recorded)
 *   10     row set of the score kernel that wrote cov_bmm last (-1: bd was re-scored since, or never)
 *   11..15 score_mode (1 streaming, 2 covariance), U, nrb (row blocks of 128 U rows of the streaming pass), n, p
 *   16     layout of `sums`: 1 = d itself, p doubles (covariance form); 0 = the nrb x p row-block partials, row block
 *          after row block, as the streaming pass leaves them
 *   17     1 if the host has a record of the fit the block describes (then head[9] and *lambda are that fit's)
 *   18     1 if the session keeps membership flags (inA; covariance form), else inA is returned as zeros
 *   19     1 if the block describes a fit chained ahead on the device that no call has asked for yet
 * *lambda: the ridge parameter of that fit.  A_cur, b_cur: the first k_cur entries are written (buffers of p entries
 * always suffice); beta_dense, inA, bd: p entries; sums: p or nrb * p doubles (head[16]); r: the n residuals m o (y - X b)
 * the streaming pass read; cov_bmm: 3 * ceil(p / 32) doubles -- per block of 32 columns the smallest score inside the
 * active set (DBL_MAX if none) and the largest outside it (-1 if none), interleaved, then the lowest column attaining
 * each maximum (2147483647 if none).  Every array pointer may be NULL. */
#define BESSX_SCORE_STATE_HEAD 20
int bessx_session_score_state(bessx_session *s, int ctx, int *head, double *lambda, int *A_cur, double *b_cur,
                              double *beta_dense, unsigned char *inA, double *bd, double *sums, double *r, double *cov_bmm);
/* How the Gram fills of the CV row sets run.  out[0]: 1 = shared (one unmasked pass over a fold-major copy of X, every
 * fold padded to whole row slabs, serves all K + 1 row sets), 0 = one masked pass per row set (also: no folds).
 * out[1]: row slabs per fold, out[2]: rows per slab, out[3]: rows of the copy = K * out[1] * out[2]; 0 unless shared. */
int bessx_session_cv_fill_geometry(const bessx_session *s, int *out /* 4 */);

/* How many chunk chains bessx_session_sequential_path may run side by side (bessx_kchunks.cpp):
 * 0 = automatic, 1 = one chain, 2..8 = that many where the path qualifies.  The initial value is BESSX_KPATH_CHAINS (else
 * 0).  The candidates returned are the same for every setting. */
int bessx_session_set_kpath_chains(bessx_session *s, int chains);

/* Shared WIDE fills inside a fit that several sessions run identically (the pilot fit of a multi-GPU k-path: same data,
 * same cache, deterministic kernels -- every rank's fit parks at the same PDAS iteration on the same missing columns).
 * With a hook set, a fit of the all-rows row set that parks on missing Gram columns does not form them privately (one
 * pass over X for 32-64 columns, repeated on every rank): the library lists the missing columns followed by the
 * uncached columns the CURRENT sacrifice scores rank highest, `width` columns in all (a multiple of 32; the same list on
 * every rank), hands them slots as bessx_session_cov_prefill_extend does, and calls hook(user, n_groups) -- the caller
 * forms its share of the groups, exchanges the blocks and closes the list (cov_prefill_compute / export / import /
 * end); the fit then goes on.  A non-zero return fails the fit with BESSX_ERR_ARG.  hook = NULL: private fills. */
typedef int (*bessx_fill_hook)(void *user, int n_groups);
int bessx_session_set_fill_hook(bessx_session *s, bessx_fill_hook hook, void *user, int width);

/* Test hook: queue a host function on the session's stream that sleeps for `milliseconds` (negative: that many
 * MICROseconds) -- everything queued behind it waits, as behind a wedged kernel (tests/test_deadline_gpu.py: the waits of the host give up at
 * BESSX_WAIT_TIMEOUT_S instead of spinning for ever). */
int bessx_session_debug_block_stream(bessx_session *s, int milliseconds);

/* ---------------------------------------------------------------------------------------
 * 4. Single-kernel entry points (host buffers in, host buffers out; each call uploads,
 *    launches on the current device and synchronises).  They exist for parity tests.
 * ------------------------------------------------------------------------------------- */
/* K1: out[j] = sum_i x[i,j] * v[i]  (X^T v; src/Algorithm.h:1109,1236,1341).  x column-major, ld >= n.
 * If v2 != NULL also out2[j] = sum_i x[i,j]^2 * v2[i] (K2; src/Algorithm.h:1240-1246). */
int bessx_op_xtv(const double *x, int n, int p, int ld, const double *v, const double *v2, double *out,
                 double *out2);
/* K1 / K2 for nc <= 8 vectors in ONE pass over X (the multi-chain score pass of chunk chains, k_xtv_mc): v, v2 are
 * nc x n (row c = chain c), out, out2 nc x p.  Bitwise the sums of nc bessx_op_xtv calls. */
int bessx_op_xtv_multi(const double *x, int n, int p, int ld, const double *v, const double *v2, int nc, double *out,
                       double *out2);
/* K4: max_k (src/utilities.cpp:179-188): the k largest scores, indices ascending, ties -> lower index. */
int bessx_op_topk(const double *score, int len, int k, int *out_idx);
/* timing of the top-k kernel (k_topk) on synthetic chi-square scores; `variant` is reserved (one kernel exists) */
int bessx_op_topk_bench(int len, int k, int variant, int repeats, double *avg_us);
/* timing of the register-resident Cholesky solve (k_chol) for an m x m system, 1 <= m <= 254 */
int bessx_op_chol_bench(int m, int repeats, double *avg_us);
/* K6: out (m x m, column-major, full symmetric) = X_A^T diag(w) X_A for the m columns cols[] of x;
 * w may be NULL (src/Algorithm.h:1134,1171,1199,1299). */
int bessx_op_gram(const double *x, int n, int p, int ld, const int *cols, int m, const double *w, double *out);
/* K7: solve the SPD system a * sol = b (a m x m column-major), Cholesky in one workgroup
 * (stands in for ColPivHouseholderQR / LDLT solves, src/Algorithm.h:1134,1171,1199,1299,1473). */
int bessx_op_chol_solve(const double *a, int m, const double *b, double *sol);
/* K11: Normalize / Normalize3 / Normalize4 + add_weight (src/normalize.cpp:20-85, src/Data.h:70-77)
 * on a column-major copy of x; returns the transformed x, y and the statistics. */
int bessx_op_normalize(double *x, int n, int p, double *y, const double *weight, int data_type, int is_normal,
                       int add_weight, double *x_mean, double *x_norm, double *y_mean);
/* Tuning aid for K1: run geometry variant `variant` of the score pass `repeats` times on an n x p matrix
 * generated on the device and report algorithmic GB/s (8*n*p bytes per launch) and the mean launch time. */
int bessx_op_xtv_bench(int n, int p, int variant, int repeats, double *gbps, double *avg_ms);
/* ... and the multi-chain score pass: nc vector sets per launch (two != 0: with the second accumulator); GB/s counts the
 * 8*n*p bytes of X once per launch. */
int bessx_op_xtv_multi_bench(int n, int p, int nc, int two, int repeats, double *gbps, double *avg_ms);
/* The same for the one-pass Cox score kernel (k_cox_score1p, 8*n*p bytes per launch); variant 1 = the one the solver runs
 * (wave map of round 4), 0 = round 3; 10 + nc (nc = 1..4) = the multi-chain kernel k_cox_score1p_mc with nc vector sets. */
int bessx_op_cox_score_bench(int n, int p, int variant, int repeats, double *gbps, double *avg_ms);
/* The Cox solver's state pass alone (k_cox_eta, the risk-set scans k_scan3_tot / k_scan3_apply, k_cox_loss) for the model
 * (cols[m], b[m]) as a session runs it: x column-major n x p with the rows in time order, padded to the session's row
 * stride; status n; weight n or NULL (ones); mask n (1 = training row, 0 = test row of a CV fold) or NULL.  Every output is
 * n doubles and may be NULL: e = exp(clamp(x b, +-30)), theta = weight * e * mask, s0 = suffix sums of theta, rs0 = 1 / s0
 * (0 where s0 is 0), s_all = suffix sums of e, s_test = suffix sums of e * (1 - mask) (written only with a mask);
 * loss[0] = sum_i w_i delta_i log(e_i / s_all_i), loss[1] = the same over the test rows with s_test, each added over the
 * workgroups in workgroup order as the session does. */
int bessx_op_cox_state(const double *x, int n, int p, const double *status, const double *weight, const double *mask,
                       const int *cols, int m, const double *b, double *e, double *theta, double *s0, double *rs0,
                       double *s_all, double *s_test, double *loss);
/* ... followed by the score pass and the sacrifice scores bd[p] (GroupPdasCox::get_A, src/Algorithm.h:1569-1640) with ridge
 * lambda.  form 0: two passes over X (block totals, k_cox_carry, k_cox_colscan, k_cox_score); form 1: one pass
 * (k_cox_score1p, k_cox_score_1p), what a session runs by default. */
int bessx_op_cox_score(const double *x, int n, int p, const double *status, const double *weight, const double *mask,
                       const int *cols, int m, const double *b, double lambda, int form, double *bd);
/* ... and the one-pass form for nc (1..6) coefficient vectors on the same columns in ONE pass over X (k_cox_score1p_mc):
 * b is nc x m, bd nc x p, row c = chain c.  Bitwise the scores of nc calls of bessx_op_cox_score with form 1. */
int bessx_op_cox_score_multi(const double *x, int n, int p, const double *status, const double *weight,
                             const double *mask, const int *cols, int m, const double *b, int nc, double lambda,
                             double *bd);
/* The front half of get_A of the logistic (family 2) and Poisson (family 3) solver alone (k_glm_eta_gh through
 * launch_glm_eta_gh, as a session calls it) for the model (cols[m], b[m], coef0); m may be 0.  x column-major n x p, padded
 * to the session's row stride; y n; weight n or NULL (ones); mask n (1 = training row, 0 = test row of a CV fold) or NULL.
 * g, h: n doubles each (may be NULL); loss[0] = the train_loss summands over all rows, loss[1] = the held-out summands over
 * the rows with mask 0, the per-block pairs added in block order as the session does; the Poisson sums of log j are formed
 * by the session's own code.  bd (p doubles, or NULL): the score pass on (g, h) and the sacrifice scores with ridge lambda,
 * queued as the head of a PDAS iteration queues them (src/Algorithm.h:1223-1257, :1338-1361). */
int bessx_op_glm_gh(int family, const double *x, int n, int p, const double *y, const double *weight, const double *mask,
                    const int *cols, int m, const double *b, double coef0, double lambda, double *g, double *h,
                    double *loss, double *bd);
/* One IRLS step of the restricted fit (src/Algorithm.h:1148-1204, :1273-1322) from the iterate bcur[T0 + 1] (intercept
 * first) on the design [1, X_cols], 1 <= T0 <= 254, through the solver's own launchers.  route 1: the fused step
 * (k_irls_gram + k_gram_reduce, T0 + 2 <= 128); route 0: the five-launch step (k_glm_irls_prep + the Gram kernel); route -1:
 * whichever a session takes for this T0; *route_taken (may be NULL) says which ran.  t: the step's number (0: no floor, no
 * Poisson log-likelihood), wfloor: the 0.001 floor of the logistic weights for t >= 1.  rows_per_slab: 0 = the solver's
 * slab height; otherwise a multiple of 64 that replaces it (fused step only; a test override, no session sets it).
 * gram: (T0 + 2) x (T0 + 2), column-major, full symmetric = [1, X_A, z]^T diag(W w mask) [1, X_A, z]; *ll: the step's
 * log-likelihood, its slab or block terms added in the order of the convergence test; wv, z (n doubles each, may be NULL):
 * written by route 0 only; bnext[T0 + 1] (may be NULL): the solve with ridge 2 lambda off the intercept, without the
 * convergence test.  "A session" is a session in its default state: route -1 applies the rule by the number of tile rows
 * alone (a session also leaves the fused step when a test hook turns it off or its work space is too small for the
 * slabs), and the pivoted fallback solve is always queued behind the solve (a session queues it once a solve of its chain
 * has stood back). */
int bessx_op_glm_irls(int family, int route, int t, int wfloor, double lambda, int rows_per_slab, const double *x, int n,
                      int p, const double *y, const double *weight, const double *mask, const int *cols, int T0,
                      const double *bcur, double *gram, double *ll, double *wv, double *z, double *bnext,
                      int *route_taken);
/* The group-selection kernels alone, through the launchers a grouped fit calls (launch_group_moments, then
 * launch_group_score three times on the same inputs: eig_mode 0 = diagonalise, 1 = diagonalise and store, 2 = load what 1
 * stored).  p columns in N groups, gidx[N] their first columns (gidx[0] = 0, ascending; group g ends where g + 1 starts, the
 * last one at p), s_g their widths.  w1, w2: n row weights each or NULL (ones / no X^T w2 pass: dcol is then left as given).
 * mblk (out, sum of s_g^2 doubles, zero-filled first): block g, column-major s_g x s_g, = X_g^T diag(w1) X_g as the moment
 * kernels leave it (no division, no ridge).  dcol (p doubles, IN and out): X^T w2 where w2 is given.  The score reads
 * M_g = mblk_g (/ n_t with lm) + 2 lambda I and d = dcol (lm: the sum over the nrb rows of part[nrb x p], / n_t) - 2 lambda
 * beta_dense, and gives bd_g = |sqrtm(M_g) beta_g + sqrtm(M_g)^-1 d_g|^2 / s_g; bd (out) is 3 x N, row m = eig_mode m.  always:
 * N flags or NULL; a flagged group scores DBL_MAX.  Work space as a session sizes it: sum of s_g^2 and 2 p doubles.
 * cshift > 0 (the first column of some group g0): x holds only the columns from cshift on, n x (p - cshift), and only the
 * groups g0 .. N - 1 are launched, with gidx, mblk, dcol and bd still indexed globally -- the panel form of the Cox group
 * branch; the blocks and scores of the groups before g0 stay zero. */
int bessx_op_group_scores(const double *x, int n, int p, int cshift, const int *gidx, int N, const double *w1,
                          const double *w2, const double *beta_dense, int lm, double n_t, double lambda,
                          const unsigned char *always, const double *part, int nrb, double *mblk, double *dcol,
                          double *bd);
/* Grouped LM screening alone: launch_group_moments(..., NULL, yw, ...) and launch_group_lsq_score.  score[N] =
 * |(X_g^T X_g)^-1 X_g^T yw|^2 / s_g; a column that depends exactly on the ones before it is dropped, an all-zero column
 * gives HUGE_VAL, a flagged group (always, N flags or NULL) DBL_MAX. */
int bessx_op_group_lsq(const double *x, int n, int p, const int *gidx, int N, const double *yw,
                       const unsigned char *always, double *score);
/* The geometry bessx_op_glm_irls and a session use for sparsity level T0 (1 .. 254) on n rows; needs no device.  out[0] =
 * the padded row count, out[1] = tile rows of the step's Gram, out[2] = 64-row chunks per group of the fused kernel's
 * instance for that many tile rows (0 beyond 8 tile rows: the five-launch step), out[3] = the solver's rows per slab. */
int bessx_op_glm_irls_geometry(int T0, int n, int *out);
/* Device-to-device streaming copy rate in GB/s (read+write bytes / time): the measured HBM ceiling
 * quoted next to the spec peak in bench.py. */
int bessx_op_stream_copy_gbps(long long bytes, int repeats, double *gbps);
/* The ingest kernel alone (section 2b): x is a DEVICE matrix (dtype, element strides), row_order a host permutation or
 * NULL, ld a multiple of 128 >= n.  out (host, ld * p doubles) receives the padded column-major image, *nan_flag 1 if
 * the kernel met a NaN, else 0. */
int bessx_op_ingest(const void *x, int dtype, long long row_stride, long long col_stride, const int *row_order, int n,
                    int p, long long ld, void *stream, double *out, int *nan_flag);
/* The same launch timed with device events: one warm-up, then `repeats` launches; *avg_ms per launch and *gbps of
 * bytes read (n * p * element size) plus bytes written (ld * p * 8). */
int bessx_op_ingest_bench(const void *x, int dtype, long long row_stride, long long col_stride, const int *row_order,
                          int n, int p, long long ld, int repeats, double *avg_ms, double *gbps);
/* The prediction kernel of section 2c timed with device events on the device matrix x: one warm-up, then `repeats`
 * launches for the support cols (host, m ascending distinct columns) and R responses, with coefficients of the library's
 * own and results in a device buffer of its own.  *avg_ms per launch; *gbps counts the bytes the result needs,
 * n * m * element size read plus n * R * 8 written (a row-contiguous x moves more than that: whole sectors). */
int bessx_op_predict_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                           const int *cols, int m, int R, int link, int repeats, double *avg_ms, double *gbps);
/* The evaluation kernels of section 2d (the fused pass and the addition of its partials) timed the same way: y (n x
 * y_cols, y_cols = 1 or R, column by column), weights and coefficients of the library's own.  *gbps counts
 * n * m * element size + n * 8 * (y_cols + 1) bytes. */
int bessx_op_eval_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                        const int *cols, int m, int R, int link, int y_cols, int repeats, double *avg_ms, double *gbps);
/* The three stages of section 2e timed with device events, each in a loop of its own (one warm-up, then `repeats`
 * launches): stage_ms[0] the predictor pass, [1] the risk-set scan and the likelihood reduction, [2] the pair counts
 * (0 when want_pairs == 0).  Times (distinct, every second row an event) and coefficients of the library's own. */
int bessx_op_cox_eval_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int R, int ties, int want_pairs, int repeats, double *stage_ms);
/* The kernels of section 2f timed the same way for an n x T result of the given kind, row-major (out_col_major == 0) or
 * column-major, in a device buffer of the library's own: stage_ms[0] the predictor pass that stores exp(clamp(eta)) in row
 * order, [1] k_cxs_curves, [2] the baseline's own kernels (hazard terms, forward scan, gather) behind a predictor pass and
 * a risk-set scan that are not timed (they are stages 0 and 1 of bessx_op_cox_eval_bench).  Times, coefficients and hg
 * of the library's own. */
int bessx_op_cox_surv_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int T, int kind, int out_col_major, int repeats, double *stage_ms);
/* The Gram sweep of section 2g and the addition of its partials (k_info_gram, k_info_finish) timed the same way, from
 * working weights of the library's own (v_i = 1 / 4, g_i alternating in sign): *avg_ms per pair of launches, *tflops =
 * 2 n (m + 1) (m + 2) useful floating-point operations (both triangles and the score) per second / 1e12. */
int bessx_op_info_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                        const int *cols, int m, int repeats, double *avg_ms, double *tflops);
/* The matrix-core kernel of section 2i alone (k_diag_lev, every kind it writes) timed the same way, from a factor, working
 * weights and residuals of the library's own: *avg_ms per launch, *tflops = n * Mpad^2 floating-point operations per
 * second / 1e12 with Mpad = 16 ceil((m + 1) / 16) (two per multiply-add of the lower triangle's tiles), *bytes = what the
 * launch must move: n m item + 7 n 8 + the packed factor once. */
int bessx_op_diag_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                        const int *cols, int m, int repeats, double *avg_ms, double *tflops, double *bytes);
/* The new kernels of section 2h timed the same way (every second row an event, distinct times or, ties = 1, groups of
 * four equal times): stage_ms[0] the gather of e_l x_l into position order, [1] the column-wise suffix scan that emits
 * the risk-set means U, [2] every launch of a bessx_cox_info_device call on device data, stages 0 and 1 included
 * (predictor pass, S0, loglik, gather, H, v and g, the sweep over x, the means, the sweep over U, the finish).
 * *bytes = what stages 0 and 1 must move: n m (item + 8) + n m 8 + J m 8.  m >= 1. */
int bessx_op_cox_info_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int ties, int repeats, double *stage_ms, double *bytes);
/* The new kernels of section 2j timed the same way on the same data, with a P of the library's own: stage_ms[0] the
 * increments and their forward scan (A), [1] A and the forming of L over it, [2] L R^T with the displacement epilogue,
 * [3] L C with the dfbeta epilogue.  *bytes = what stages 1 to 3 must move: n m (item + 5 * 8) + 2 J m 8.  m >= 1. */
int bessx_op_cox_diag_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int ties, int repeats, double *stage_ms, double *bytes);
/* The cluster-sum kernel of section 2k alone (and the addition of the partials of clusters longer than a run) timed the
 * same way for the intercept and the support cols, a u of the library's own and n host labels.  *bytes = what the
 * algorithm needs: the support and u once, S once (the kernel's re-reads of u, the row order and the run table per four
 * entries are not counted). */
int bessx_op_sandwich_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, const long long *cluster, int repeats, double *avg_ms,
                            double *bytes);
/* The four kernels of section 2l timed the same way, from row weights and a factor of the library's own, each over
 * every block of candidates: stage_ms[0] the pack of the panel, [1] the cross product on the matrix cores, [2] the
 * addition of the partials, [3] the statistic kernel.  candidates / q / candidate_block as in section 2l. */
int bessx_op_addscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, const int *candidates, int q, int candidate_block, int repeats,
                            double *stage_ms);
/* The kernels of section 2m timed the same way, from n-vectors, an A and a factor of the library's own, each over every
 * block of candidates: stage_ms[0] the pack of the panel, [1] the cross product on the matrix cores, [2] the streaming
 * pass of the risk-set term, [3] the addition of its slabs, [4] the addition of the cross partials, [5] the statistic
 * kernel.  sorted != 0: the rows are in time order already; else a scattered order.  *bytes = what stage 2 needs: the
 * candidate columns once.  m >= 0. */
int bessx_op_cox_addscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                                const int *cols, int m, const int *candidates, int q, int candidate_block, int sorted,
                                int repeats, double *stage_ms, double *bytes);
/* The steps of section 2n timed the same way, from row weights and a factor of the library's own, each over every block
 * of candidates: stage_ms[0] the pack of the panel, [1] section 2l's cross product, [2] the addition of its partials,
 * [3] the Gram band on the matrix cores, [4] the addition of its partials, [5] T, the band of S and a, [6] the copy of
 * the groups' blocks of D and S.  group_starts / n_groups / groups / n_tested / candidate_block as in section 2n. */
int bessx_op_groupscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                              const int *cols, int m, const int *group_starts, int n_groups, const int *groups,
                              int n_tested, int candidate_block, int repeats, double *stage_ms);
/* The steps of section 2o timed the same way, from n-vectors, an A and a factor of the library's own (those of
 * bessx_op_cox_addscore_bench, with a constant cc): stage_ms[0] .. [6] as bessx_op_groupscore_bench with section 2m's
 * pack, [7] the band of the risk-set term T on the matrix cores, [8] the addition of its slabs and the copy of the
 * groups' blocks of T.  sorted != 0: the rows are in time order already; else a scattered order.  *bytes = what stage 7
 * needs: the tested columns once. */
int bessx_op_cox_groupscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                                  const int *cols, int m, const int *group_starts, int n_groups, const int *groups,
                                  int n_tested, int candidate_block, int sorted, int repeats, double *stage_ms,
                                  double *bytes);
/* The kernels of section 2s' band call timed the same way for an n x T result of the outputs `what` (K row-major slabs), from
 * a model, a factor and T-sized inputs of the library's own: stage_ms[0] the predictor pass that stores exp(clip(eta)),
 * stage_ms[1] k_cbd_band (k_cbd_band0 for m = 0) with the survival / log-log epilogue. */
int bessx_op_cox_band_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int T, unsigned what, int repeats, double *stage_ms);
/* The kernels of section 2u timed the same way for K segments, T horizons (cuts spread evenly over the segments), J
 * baseline times and Q levels, from a B, segments, a baseline and levels of the library's own; the outputs are row-major
 * device buffers: stage_ms[0] the predictor pass that stores e, [1] k_cxr_partial over every chunk of rows (n * K terms),
 * [2] k_cxr_finish over every chunk, [3] k_cxr_quantile (n * Q searches). */
int bessx_op_cox_rmst_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int K, int T, int J, int Q, int repeats, double *stage_ms);
/* Section 2t's sweep over x for three row-weight pairs of the library's own, device events with one warm-up, `repeats`
 * single timings each way, alternating: fused_ms[i] one launch of the three-weight sweep with its finish, separate_ms[i]
 * three back-to-back launches of section 2g's one-weight sweep with its finish on the same data. */
int bessx_op_cox_zph_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                           const int *cols, int m, int repeats, double *fused_ms, double *separate_ms);
/* The kernels of section 2p timed the same way for R models and T times, from a B, time, weights and an hg of the
 * library's own (distinct times, T ascending times across their range): stage_ms[0] the predictor pass that stores e
 * (R x n, row order), [1] the reduction kernel k_cxb_terms (n * T * R elements), [2] the addition of its slabs. */
int bessx_op_cox_brier_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                             const int *cols, int m, int R, int T, int repeats, double *stage_ms);
/* The kernels of sections 2q and 2r timed the same way for R models and T >= 1 cuts, from a B, times, a status and
 * weights of the library's own (distinct times, T ascending cuts across their range): stage_ms[0] the predictor pass
 * that stores eta (R x n, position order), [1] the pair kernel k_pa_pairs in AUC mode, [2] its two finish kernels, [3]
 * the pair kernel in Uno mode; *pairs = the pairs (k, l) stage 1 compares per launch, all models together. */
int bessx_op_pairauc_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                           const int *cols, int m, int R, int T, int repeats, double *stage_ms, double *pairs);

/* ---------------------------------------------------------------------------------------
 * 5. A communicator for hosts without torch.distributed (round 6): the ONE collective the sharded paths need -- an
 *    all-gather of small fp64 records (the IC / CV curve, 8 B per candidate; the k-chunks' last models; the fold fits'
 *    records: SURVEY 8e) -- on RCCL directly.  One process per GPU; rank 0 calls bessx_comm_unique_id and the host hands
 *    the 128 bytes to the other ranks by whatever it has (a file, MPI, a socket); every rank then calls bessx_comm_init
 *    (collective: returns when all `world` ranks have called it).  RCCL is loaded when the first of these functions is
 *    called (BESSX_ERR_UNSUPPORTED when it cannot be).  bess_amd.dist.BessxComm is the Python face of it.
 * ------------------------------------------------------------------------------------- */
#define BESSX_COMM_ID_BYTES 128
typedef struct bessx_comm bessx_comm;
int bessx_comm_unique_id(unsigned char *id /* BESSX_COMM_ID_BYTES */);
int bessx_comm_init(bessx_comm **out, int rank, int world, const unsigned char *id, int device);
int bessx_comm_rank(const bessx_comm *c);
int bessx_comm_world(const bessx_comm *c);
/* every rank's `count` doubles to every rank: recv[r * count .. (r + 1) * count) = rank r's send; host buffers */
int bessx_comm_allgather_f64(bessx_comm *c, const double *send, int count, double *recv);
void bessx_comm_destroy(bessx_comm *c);

#ifdef __cplusplus
}
#endif
#endif /* BESSX_H */
