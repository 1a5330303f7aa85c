// bessx_abi.cpp -- the drop-in entry points bessx_pywrap_bess / bessx_bessCpp (src/bess.h:20-51) and the single-kernel ops
#include "bessx_devcall.h"

extern "C" {

// ----------------------------------------------------------------------------------------------
// pywrap_bess drop-in (src/bess.cpp:218-281 -> bessCpp :37-214)
// ----------------------------------------------------------------------------------------------
// the body of bessx_pywrap_bess and bessx_pywrap_bess_device: din null = x, y, weight on the host; else the data of din
static int pywrap_impl(const bessx_device_input *din, double *x, int x_row, int x_col, double *y, int y_len,
                       int data_type, double *weight,
                      int weight_len, int is_normal, int algorithm_type, int model_type, int max_iter,
                      int exchange_num, int path_type, int is_warm_start, int ic_type, int is_cv, int K, int *gindex,
                      int gindex_len, double *state, int state_len, int *sequence, int sequence_len,
                      double *lambda_sequence, int lambda_sequence_len, int s_min, int s_max, int K_max,
                      double epsilon, double lambda_min, double lambda_max, int n_lambda, int is_screening,
                      int screening_size, int powell_path, int *always_select, int always_select_len, double tao,
                      double *beta_out, int beta_out_len, double *coef0_out, int coef0_out_len,
                      double *train_loss_out, int train_loss_out_len, double *ic_out, int ic_out_len,
                      double *nullloss_out, double *aic_out, int aic_out_len, double *bic_out, int bic_out_len,
                      double *gic_out, int gic_out_len, int *A_out, int A_out_len, int *l_out) {
  (void)exchange_num; (void)state; (void)state_len; (void)K_max; (void)epsilon;
  (void)tao;  // dead on the live reference paths
  (void)coef0_out_len; (void)train_loss_out_len; (void)ic_out_len;
  if ((!din && (!x || !y)) || !beta_out || !coef0_out || !train_loss_out || !ic_out) return fail(BESSX_ERR_ARG, "null argument");
  if (!din && (y_len != x_row || (weight && weight_len != x_row))) return fail(BESSX_ERR_ARG, "length of y / weight != rows of x");
  if (beta_out_len < x_col) return fail(BESSX_ERR_ARG, "beta_out too short");
  if (!gindex || gindex_len < 1 || gindex_len > x_col) return fail(BESSX_ERR_ARG, "bad group index");
  bessx_problem pb;
  std::memset(&pb, 0, sizeof(pb));
  pb.n = x_row;
  pb.p = x_col;
  pb.x = x;
  pb.x_col_major = 0;
  pb.y = y;
  pb.weight = weight;
  pb.data_type = data_type;
  pb.is_normal = is_normal;
  pb.model_type = model_type;
  pb.algorithm_type = algorithm_type;
  pb.max_iter = max_iter;
  pb.is_warm_start = is_warm_start;
  pb.always_select = always_select;
  pb.always_select_len = always_select_len;
  pb.device = -1;
  pb.group_index = gindex;
  pb.group_index_len = gindex_len;
  pb.is_screening = is_screening ? 1 : 0;
  pb.screening_size = screening_size;
  {
    // the work space is sized for the largest active set the path can ask for (levels count groups)
    long top = path_type == 1 ? 0 : s_max;
    if (path_type == 1)
      for (int i = 0; i < sequence_len; i++) top = std::max<long>(top, sequence ? sequence[i] : 0);
    long gmax = 1;
    for (int g = 0; g < gindex_len; g++)
      gmax = std::max<long>(gmax, (g + 1 < gindex_len ? gindex[g + 1] : x_col) - gindex[g]);
    pb.max_sparsity = (int)std::min<long>(std::min<long>(top * gmax, x_col), T0_HARD);
  }
  bessx_session *s = nullptr;
  if (int rc = din ? bessx_session_create_device(&s, &pb, din) : bessx_session_create(&s, &pb)) return rc;
  int rc = 0;
  if (is_cv) rc = bessx_session_set_cv(s, K, nullptr, 123u);
  bessx_path_result res;
  std::memset(&res, 0, sizeof(res));
  res.beta = beta_out;
  if (rc == 0) {
    if (path_type == 1)
      rc = bessx_session_sequential_path(s, sequence, sequence_len, lambda_sequence, lambda_sequence_len, ic_type,
                                         is_cv, &res);
    else if (algorithm_type == 5 || algorithm_type == 3)  // src/bess.cpp:174-180
      rc = bessx_session_pgs_path(s, s_min, s_max, lambda_min, lambda_max, n_lambda, powell_path, ic_type, is_cv, &res);
    else
      rc = bessx_session_gs_path(s, s_min, s_max, ic_type, is_cv, &res);
  }
  if (rc == 0) {
    *coef0_out = res.coef0;
    *train_loss_out = res.train_loss;
    *ic_out = res.ic;
    if (nullloss_out) *nullloss_out = s->nullloss;
    if (aic_out && aic_out_len > 0) aic_out[0] = 0.0;
    if (bic_out && bic_out_len > 0) bic_out[0] = 0.0;
    if (gic_out && gic_out_len > 0) gic_out[0] = 0.0;
    if (A_out) {
      int k = 0;
      for (int j = 0; j < x_col && k < A_out_len; j++)
        if (beta_out[j] != 0.0) A_out[k++] = j;
      for (; k < A_out_len; k++) A_out[k] = -1;
    }
    if (l_out) *l_out = res.best_iters;
  }
  std::string keep = g_err;
  bessx_session_destroy(s);
  g_err = keep;
  return rc;
}

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
                      double *gic_out, int gic_out_len, int *A_out, int A_out_len, int *l_out) {
  return pywrap_impl(nullptr, x, x_row, x_col, y, y_len, data_type, weight, weight_len, is_normal, algorithm_type,
                     model_type, max_iter, exchange_num, path_type, is_warm_start, ic_type, is_cv, K, gindex, gindex_len,
                     state, state_len, sequence, sequence_len, lambda_sequence, lambda_sequence_len, s_min, s_max, K_max,
                     epsilon, lambda_min, lambda_max, n_lambda, is_screening, screening_size, powell_path, always_select,
                     always_select_len, tao, beta_out, beta_out_len, coef0_out, coef0_out_len, train_loss_out,
                     train_loss_out_len, ic_out, ic_out_len, nullloss_out, aic_out, aic_out_len, bic_out, bic_out_len,
                     gic_out, gic_out_len, A_out, A_out_len, l_out);
}

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
                             int gic_out_len, int *A_out, int A_out_len, int *l_out, int *x_nan_out) {
  if (x_nan_out) *x_nan_out = 0;
  if (!in) return fail(BESSX_ERR_ARG, "null argument");
  const int rc = pywrap_impl(in, nullptr, x_row, x_col, nullptr, x_row, data_type, nullptr, x_row, is_normal,
                             algorithm_type, model_type, max_iter, exchange_num, path_type, is_warm_start, ic_type, is_cv,
                             K, gindex, gindex_len, state, state_len, sequence, sequence_len, lambda_sequence,
                             lambda_sequence_len, s_min, s_max, K_max, epsilon, lambda_min, lambda_max, n_lambda,
                             is_screening, screening_size, powell_path, always_select, always_select_len, tao, beta_out,
                             beta_out_len, coef0_out, coef0_out_len, train_loss_out, train_loss_out_len, ic_out,
                             ic_out_len, nullloss_out, aic_out, aic_out_len, bic_out, bic_out_len, gic_out, gic_out_len,
                             A_out, A_out_len, l_out);
  if (rc == BESSX_ERR_ARG && x_nan_out && g_err == "There is NAN value in X") *x_nan_out = 1;
  return rc;
}

// ----------------------------------------------------------------------------------------------
// bessCpp drop-in for the R package (src/bess.h:20-33; R/src/RcppExports.cpp:10-48): see include/bessx.h 1b
// ----------------------------------------------------------------------------------------------
int bessx_bessCpp(const double *x, int n, int p, const double *y, int data_type, const double *weight, int is_normal,
                  int algorithm_type, int model_type, int max_iter, int exchange_num, int path_type,
                  int is_warm_start, int ic_type, int is_cv, int K, const double *state, int state_len,
                  const int *sequence, int sequence_len, const double *lambda_seq, int lambda_len, int s_min, int s_max,
                  int K_max, double epsilon, double lambda_min, double lambda_max, int nlambda, int is_screening,
                  int screening_size, int powell_path, const int *g_index, int g_index_len, const int *always_select,
                  int always_select_len, double tao, bessx_r_result *res) {
  (void)exchange_num; (void)state; (void)state_len; (void)K_max; (void)epsilon; (void)tao;  // dead in the reference too
  if (!x || !y || !res || !res->beta) return fail(BESSX_ERR_ARG, "bessCpp: null argument");
  if (!g_index || g_index_len < 1 || g_index_len > p) return fail(BESSX_ERR_ARG, "bessCpp: bad group index");
  const bool seqp = path_type == 1;
  const bool powell = !seqp && (algorithm_type == 5 || algorithm_type == 3);  // src/bess.cpp:174-180
  if (seqp && (!sequence || sequence_len < 1 || !lambda_seq || lambda_len < 1))
    return fail(BESSX_ERR_ARG, "bessCpp: empty sequence / lambda_seq");
  bessx_problem pb;
  std::memset(&pb, 0, sizeof(pb));
  pb.n = n;
  pb.p = p;
  pb.x = x;
  pb.x_col_major = 1;
  pb.y = y;
  pb.weight = weight;
  pb.data_type = data_type;
  pb.is_normal = is_normal;
  pb.model_type = model_type;
  pb.algorithm_type = algorithm_type;
  pb.max_iter = max_iter;
  pb.is_warm_start = is_warm_start;
  pb.always_select = always_select;
  pb.always_select_len = always_select_len;
  pb.device = -1;
  pb.group_index = g_index;
  pb.group_index_len = g_index_len;
  pb.is_screening = is_screening ? 1 : 0;
  pb.screening_size = screening_size;
  long gmax = 1, top = seqp ? 0 : s_max;
  for (int g = 0; g < g_index_len; g++) gmax = std::max<long>(gmax, (g + 1 < g_index_len ? g_index[g + 1] : p) - g_index[g]);
  if (seqp)
    for (int i = 0; i < sequence_len; i++) top = std::max<long>(top, sequence[i]);
  pb.max_sparsity = (int)std::min<long>(std::min<long>(top * gmax, p), T0_HARD);
  bessx_session *s = nullptr;
  if (int rc = bessx_session_create(&s, &pb)) return rc;
  auto done = [&](int rc) {
    std::string keep = g_err;
    bessx_session_destroy(s);
    g_err = keep;
    return rc;
  };
  if (is_cv)
    if (int rc = bessx_session_set_cv(s, K, nullptr, 123u)) return done(rc);
  const int cap = seqp ? sequence_len * lambda_len : (powell ? 128 : 2 * (s_max - s_min + 1) + 64);
  const int maxT = (int)std::max<long>(1, std::min<long>(p, std::max<long>(top, 1) * gmax));
  std::vector<double> c_ic((size_t)cap), c_loss((size_t)cap), c_c0((size_t)cap), c_beta((size_t)cap * maxT);
  std::vector<int> c_sup((size_t)cap * maxT, -1), c_T0((size_t)cap);
  std::vector<double> c_lam((size_t)cap);
  bessx_path_result r;
  std::memset(&r, 0, sizeof(r));
  r.beta = res->beta;
  r.capacity = cap;
  r.max_T0 = maxT;
  r.cand_T0 = c_T0.data();
  r.cand_lambda = c_lam.data();
  r.cand_ic = c_ic.data();
  r.cand_train_loss = c_loss.data();
  r.cand_coef0 = c_c0.data();
  r.cand_beta = c_beta.data();
  r.cand_support = c_sup.data();
  int rc = seqp     ? bessx_session_sequential_path(s, sequence, sequence_len, lambda_seq, lambda_len, ic_type, is_cv, &r)
           : powell ? bessx_session_pgs_path(s, s_min, s_max, lambda_min, lambda_max, nlambda, powell_path, ic_type,
                                             is_cv, &r)
                    : bessx_session_gs_path(s, s_min, s_max, ic_type, is_cv, &r);
  if (rc) return done(rc);
  if (is_screening && res->screening_A) {
    // screening_A of src/screening.cpp:68: kept columns, or kept GROUPS when the groups have more than one column
    if (bessx_session_get_screening_groups(s, res->screening_A, screening_size) == 0)
      bessx_session_get_screening(s, res->screening_A, screening_size);
  }
  res->coef0 = r.coef0;
  res->train_loss = r.train_loss;
  res->ic = r.ic;
  res->lambda = r.lambda;
  const int nc = std::min(r.n_candidates, cap);
  res->n_all = nc;
  // candidates arrive in evaluation order; the sequential path's order is the snake of src/path.cpp:50
  std::vector<int> where((size_t)nc);
  if (seqp) {
    int c = 0;
    for (int i = 0; i < sequence_len; i++) {
      const int step = (i % 2 == 0) ? 1 : -1;
      for (int j = (i % 2 == 0) ? 0 : lambda_len - 1; j < lambda_len && j >= 0 && c < nc; j += step)
        where[c++] = j * sequence_len + i;
    }
  } else {
    for (int c = 0; c < nc; c++) where[c] = c;
  }
  const int wr = std::min(nc, res->all_capacity);
  if (res->beta_all) std::fill(res->beta_all, res->beta_all + (size_t)p * std::max(res->all_capacity, 0), 0.0);
  for (int c = 0; c < nc; c++) {
    const int q = where[c];
    if (q >= wr) continue;
    if (res->coef0_all) res->coef0_all[q] = c_c0[c];
    if (res->train_loss_all) res->train_loss_all[q] = c_loss[c];
    if (res->ic_all) res->ic_all[q] = c_ic[c];
    if (res->beta_all)
      for (int t = 0; t < maxT && c_sup[(size_t)c * maxT + t] >= 0; t++)
        res->beta_all[(size_t)q * p + c_sup[(size_t)c * maxT + t]] = c_beta[(size_t)c * maxT + t];
  }
  return done(BESSX_OK);
}

// ----------------------------------------------------------------------------------------------
// single-kernel entry points for parity tests
// ----------------------------------------------------------------------------------------------
int bessx_op_xtv(const double *x, int n, int p, int ld, const double *v, const double *v2, double *out,
                 double *out2) {
  if (int rc = need_device()) return rc;
  if (!x || !v || !out || n < 1 || p < 1 || ld < n) return fail(BESSX_ERR_ARG, "op_xtv: bad arguments");
  Owner sc;
  const int U = n >= 4096 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1));
  double *dX, *dv, *dv2 = nullptr, *part, *part2 = nullptr, *dout;
  long ldd;
  if (int rc = upload_padded(sc, x, n, p, ld, U, &dX, &ldd)) return rc;
  if (int rc = upload_vec_padded(sc, v, n, ldd, &dv)) return rc;
  if (v2)
    if (int rc = upload_vec_padded(sc, v2, n, ldd, &dv2)) return rc;
  int nrb = (int)(ldd / (128L * U));
  HIPX(sc.alloc(&part, (size_t)nrb * p));
  HIPX(sc.alloc(&part2, (size_t)nrb * p));
  HIPX(sc.alloc(&dout, (size_t)p));
  HIPX(launch_xtv(dX, ldd, p, U, dv, dv2, part, part2, nullptr, 0, nullptr));
  HIPX(launch_part_sum(part, nrb, p, dout, nullptr));
  HIPX(hipMemcpy(out, dout, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  if (v2 && out2) {
    HIPX(launch_part_sum(part2, nrb, p, dout, nullptr));
    HIPX(hipMemcpy(out2, dout, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  }
  return BESSX_OK;
}

// the same sums for nc vectors at once by the multi-chain kernel (k_xtv_mc: one pass over X): row c of v / v2 / out / out2
// belongs to chain c.  Bitwise the results of nc calls of bessx_op_xtv (tests/test_ops_gpu.py).
int bessx_op_xtv_multi(const double *x, int n, int p, int ld, const double *v, const double *v2, int nc, double *out,
                       double *out2) {
  if (int rc = need_device()) return rc;
  if (!x || !v || !out || n < 1 || p < 1 || ld < n || nc < 1 || nc > XTV_MC_MAX || (v2 && !out2))
    return fail(BESSX_ERR_ARG, "op_xtv_multi: bad arguments");
  Owner sc;
  const int U = n >= 4096 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1));
  double *dX, *dout;
  long ldd;
  if (int rc = upload_padded(sc, x, n, p, ld, U, &dX, &ldd)) return rc;
  const int nrb = (int)(ldd / (128L * U));
  XtvMc a = {};
  a.nc = nc;
  for (int c = 0; c < nc; c++) {
    double *dv, *dv2 = nullptr, *part, *part2 = nullptr;
    if (int rc = upload_vec_padded(sc, v + (size_t)c * n, n, ldd, &dv)) return rc;
    if (v2)
      if (int rc = upload_vec_padded(sc, v2 + (size_t)c * n, n, ldd, &dv2)) return rc;
    HIPX(sc.alloc(&part, (size_t)nrb * p));
    HIPX(sc.alloc(&part2, (size_t)nrb * p));
    a.v[c] = dv;
    a.v2[c] = dv2;
    a.part[c] = part;
    a.part2[c] = part2;
    a.ctrl[c] = nullptr;
    a.slot[c] = 0;
  }
  HIPX(sc.alloc(&dout, (size_t)p));
  HIPX(launch_xtv_mc(dX, ldd, p, U, a, v2 != nullptr, nullptr));
  for (int c = 0; c < nc; c++) {
    HIPX(launch_part_sum(a.part[c], nrb, p, dout, nullptr));
    HIPX(hipMemcpy(out + (size_t)c * p, dout, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
    if (v2) {
      HIPX(launch_part_sum(a.part2[c], nrb, p, dout, nullptr));
      HIPX(hipMemcpy(out2 + (size_t)c * p, dout, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  return BESSX_OK;
}

int bessx_op_topk(const double *score, int len, int k, int *out_idx) {
  if (int rc = need_device()) return rc;
  if (!score || !out_idx || len < 1 || k < 0 || k > len) return fail(BESSX_ERR_ARG, "op_topk: bad arguments");
  if (k == 0) return BESSX_OK;
  if (!topk_supported(len, k)) return fail(BESSX_ERR_UNSUPPORTED, "op_topk: len / k combination needs a third level");
  Owner sc;
  double *ds;
  int *dout, *dcand;
  HIPX(sc.alloc(&ds, (size_t)len));
  HIPX(sc.alloc(&dout, (size_t)k));
  int *dtie;
  HIPX(sc.alloc(&dcand, (size_t)32768));
  HIPX(sc.alloc(&dtie, (size_t)3 * len + 8));
  HIPX(hipMemset(dtie, 0, 8 * sizeof(int)));
  HIPX(hipMemcpy(ds, score, (size_t)len * sizeof(double), hipMemcpyHostToDevice));
  const TopkTie tie = {dtie, dtie + 8};
  HIPX(launch_topk(ds, len, k, dout, dcand, nullptr, 0, nullptr, nullptr, nullptr, &tie));
  HIPX(hipMemcpy(out_idx, dout, (size_t)k * sizeof(int), hipMemcpyDeviceToHost));
  return BESSX_OK;
}

int bessx_op_topk_bench(int len, int k, int variant, int repeats, double *avg_us) {
  if (int rc = need_device()) return rc;
  if (len < 1 || k < 1 || k > len || repeats < 1 || !avg_us) return fail(BESSX_ERR_ARG, "op_topk_bench: bad arguments");
  if (!topk_supported(len, k)) return fail(BESSX_ERR_UNSUPPORTED, "op_topk_bench: len / k combination needs a third level");
  Owner sc;
  double *ds;
  int *dout, *dcand;
  HIPX(sc.alloc(&ds, (size_t)len));
  HIPX(sc.alloc(&dout, (size_t)k));
  HIPX(sc.alloc(&dcand, (size_t)32768));
  std::vector<double> h((size_t)len);
  std::mt19937_64 g(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  for (auto &v : h) {
    const double z = nd(g);
    v = z * z;
  }
  HIPX(hipMemcpy(ds, h.data(), (size_t)len * sizeof(double), hipMemcpyHostToDevice));
  topk_set_variant(variant);
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  hipError_t e = launch_topk(ds, len, k, dout, dcand, nullptr, 0, nullptr);
  if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
  for (int i = 0; i < repeats && e == hipSuccess; i++) e = launch_topk(ds, len, k, dout, dcand, nullptr, 0, nullptr);
  if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  topk_set_variant(1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  HIPX(e);
  *avg_us = 1e3 * (double)ms / repeats;
  return BESSX_OK;
}

int bessx_op_gram(const double *x, int n, int p, int ld, const int *cols, int m, const double *w, double *out) {
  if (int rc = need_device()) return rc;
  if (!x || !cols || !out || n < 1 || p < 1 || ld < n || m < 1 || m > T0_CAP) return fail(BESSX_ERR_ARG, "op_gram: bad arguments");
  for (int i = 0; i < m; i++)
    if (cols[i] < 0 || cols[i] >= p) return fail(BESSX_ERR_ARG, "op_gram: column index out of range");
  Owner sc;
  const int U = 1;
  HIPX(gram_lds_prepare());
  double *dX, *dw = nullptr, *daux, *gpart, *Gt;
  long ldd;
  if (int rc = upload_padded(sc, x, n, p, ld, U, &dX, &ldd)) return rc;
  if (w)
    if (int rc = upload_vec_padded(sc, w, n, ldd, &dw)) return rc;
  HIPX(sc.alloc(&daux, (size_t)ldd * 3));
  HIPX(hipMemset(daux, 0, (size_t)ldd * 3 * sizeof(double)));
  const int mt = (m + 15) / 16, mp = mt * 16, ntiles = mt * (mt + 1) / 2;
  std::vector<int> hc(mp, -1);
  std::copy(cols, cols + m, hc.begin());
  int *dcols;
  HIPX(sc.alloc(&dcols, (size_t)mp));
  HIPX(hipMemcpy(dcols, hc.data(), (size_t)mp * sizeof(int), hipMemcpyHostToDevice));
  std::vector<GramTask> tasks;
  build_gram_tasks(mt, tasks);
  GramTask *dt;
  HIPX(sc.alloc(&dt, tasks.size()));
  HIPX(hipMemcpy(dt, tasks.data(), tasks.size() * sizeof(GramTask), hipMemcpyHostToDevice));
  bessx_session fake;
  fake.ld = ldd;
  int rps, nslab;
  gram_geometry(&fake, (int)tasks.size(), &rps, &nslab);
  HIPX(sc.alloc(&gpart, (size_t)nslab * ntiles * 256));
  HIPX(sc.alloc(&Gt, (size_t)ntiles * 256));
  HIPX(launch_gram(dX, daux, ldd, dcols, dw, rps, dt, (int)tasks.size(), nslab, gpart, ntiles, Gt, nullptr, 0, 0,
                   nullptr, 0));
  std::vector<double> ht((size_t)ntiles * 256);
  HIPX(hipMemcpy(ht.data(), Gt, ht.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int I = 0; I < mt; I++)
    for (int J = 0; J <= I; J++) {
      int t = I * (I + 1) / 2 + J;
      for (int lane = 0; lane < 64; lane++)
        for (int r = 0; r < 4; r++) {
          int row = I * 16 + (lane >> 4) + 4 * r, col = J * 16 + (lane & 15);
          if (row < m && col < m) {
            double v = ht[(size_t)t * 256 + lane * 4 + r];
            out[(size_t)col * m + row] = v;
            if (I != J) out[(size_t)row * m + col] = v;
          }
        }
    }
  return BESSX_OK;
}

int bessx_op_chol_solve(const double *a, int m, const double *b, double *sol) {
  if (int rc = need_device()) return rc;
  if (!a || !b || !sol || m < 1 || m > T0_CAP) return fail(BESSX_ERR_ARG, "op_chol_solve: need 1 <= m <= 2046");
  Owner sc;
  const int mt = (m + 1 + 15) / 16, ntiles = mt * (mt + 1) / 2;
  std::vector<double> ht((size_t)ntiles * 256, 0.0);
  for (int I = 0; I < mt; I++)
    for (int J = 0; J <= I; J++) {
      int t = I * (I + 1) / 2 + J;
      for (int lane = 0; lane < 64; lane++)
        for (int r = 0; r < 4; r++) {
          int row = I * 16 + (lane >> 4) + 4 * r, col = J * 16 + (lane & 15);
          if (row < m && col < m) ht[(size_t)t * 256 + lane * 4 + r] = a[(size_t)col * m + row];
        }
    }
  double *Gt, *drhs, *dsol;
  int *dinfo;
  HIPX(sc.alloc(&Gt, ht.size()));
  HIPX(sc.alloc(&drhs, (size_t)m));
  HIPX(sc.alloc(&dsol, (size_t)m));
  HIPX(sc.alloc(&dinfo, 1));
  HIPX(hipMemset(dinfo, 0, sizeof(int)));
  HIPX(hipMemcpy(Gt, ht.data(), ht.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(drhs, b, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
  if (mt <= 16) {
    double *dfb;
    HIPX(sc.alloc(&dfb, CHOL_FB_DOUBLES));
    CholFuse fbz = {};
    fbz.fb_work = dfb;  // (a singular / indefinite matrix goes to the pivoted solve, like in the fits)
    HIPX(launch_chol(Gt, m, mt, 0.0, 0, drhs, nullptr, dsol, dinfo, nullptr, 0, 0, nullptr, &fbz));
    HIPX(launch_sym_fallback(Gt, m, mt, 0.0, 0, drhs, nullptr, dsol, dinfo, nullptr, 0, nullptr, &fbz));
  } else {
    double *rd, *zz;
    HIPX(sc.alloc(&rd, (size_t)mt * 16));
    HIPX(sc.alloc(&zz, (size_t)mt * 16));
    HIPX(launch_chol_big(Gt, m, mt, 0.0, 0, drhs, nullptr, dsol, dinfo, rd, zz, nullptr, 0, 0, nullptr));
  }
  HIPX(hipMemcpy(sol, dsol, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
  int info = 0;
  HIPX(hipMemcpy(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost));
  if (info) return fail(BESSX_ERR_NUMERIC, "op_chol_solve: non-finite solution");
  return BESSX_OK;
}

int bessx_op_chol_bench(int m, int repeats, double *avg_us) {
  if (int rc = need_device()) return rc;
  if (m < 1 || m > T0_FAST || repeats < 1 || !avg_us) return fail(BESSX_ERR_ARG, "op_chol_bench: need 1 <= m <= 254");
  Owner sc;
  const int mt = (m + 1 + 15) / 16, ntiles = mt * (mt + 1) / 2;
  // a well conditioned matrix: 4 I + small symmetric off-diagonal entries
  std::vector<double> ht((size_t)ntiles * 256, 0.0);
  for (int I = 0; I < mt; I++)
    for (int J = 0; J <= I; J++) {
      int t = I * (I + 1) / 2 + J;
      for (int lane = 0; lane < 64; lane++)
        for (int r = 0; r < 4; r++) {
          int row = I * 16 + (lane >> 4) + 4 * r, col = J * 16 + (lane & 15);
          if (row < m && col < m)
            ht[(size_t)t * 256 + lane * 4 + r] = row == col ? 4.0 : 0.01 * std::cos(0.37 * (row + 1) * (col + 1));
        }
    }
  double *Gt, *drhs, *dsol;
  int *dinfo;
  HIPX(sc.alloc(&Gt, ht.size()));
  HIPX(sc.alloc(&drhs, (size_t)m));
  HIPX(sc.alloc(&dsol, (size_t)m));
  HIPX(sc.alloc(&dinfo, 1));
  HIPX(hipMemset(dinfo, 0, sizeof(int)));
  HIPX(hipMemcpy(Gt, ht.data(), ht.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(launch_fill(drhs, m, 1.0, nullptr));
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  hipError_t e = launch_chol(Gt, m, mt, 0.0, 0, drhs, nullptr, dsol, dinfo, nullptr, 0, 0, nullptr);
  if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
  for (int i = 0; i < repeats && e == hipSuccess; i++)
    e = launch_chol(Gt, m, mt, 0.0, 0, drhs, nullptr, dsol, dinfo, nullptr, 0, 0, nullptr);
  if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  HIPX(e);
  *avg_us = 1e3 * (double)ms / repeats;
  return BESSX_OK;
}

int bessx_op_normalize(double *x, int n, int p, double *y, const double *weight, int data_type, int is_normal,
                       int add_weight, double *x_mean, double *x_norm, double *y_mean) {
  if (int rc = need_device()) return rc;
  if (!x || !y || !weight || n < 1 || p < 1) return fail(BESSX_ERR_ARG, "op_normalize: bad arguments");
  Owner sc;
  double *dX, *dy, *dw, *dm, *dn, *dym;
  long ldd;
  if (int rc = upload_padded(sc, x, n, p, n, 1, &dX, &ldd)) return rc;
  if (int rc = upload_vec_padded(sc, y, n, ldd, &dy)) return rc;
  if (int rc = upload_vec_padded(sc, weight, n, ldd, &dw)) return rc;
  HIPX(sc.alloc(&dm, (size_t)p));
  HIPX(sc.alloc(&dn, (size_t)p));
  HIPX(sc.alloc(&dym, 1));
  HIPX(hipMemset(dm, 0, (size_t)p * sizeof(double)));
  HIPX(hipMemset(dn, 0, (size_t)p * sizeof(double)));
  HIPX(launch_normalize(dX, ldd, n, p, dy, dw, data_type, is_normal, add_weight, dm, dn, dym, nullptr));
  HIPX(hipMemcpy2D(x, (size_t)n * sizeof(double), dX, (size_t)ldd * sizeof(double), (size_t)n * sizeof(double),
                   (size_t)p, hipMemcpyDeviceToHost));
  HIPX(hipMemcpy(y, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (x_mean) HIPX(hipMemcpy(x_mean, dm, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  if (x_norm) HIPX(hipMemcpy(x_norm, dn, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  if (y_mean) HIPX(hipMemcpy(y_mean, dym, sizeof(double), hipMemcpyDeviceToHost));
  return BESSX_OK;
}

int bessx_op_xtv_bench(int n, int p, int variant, int repeats, double *gbps, double *avg_ms) {
  if (int rc = need_device()) return rc;
  if (n < 1 || p < 1 || repeats < 1 || !gbps) return fail(BESSX_ERR_ARG, "op_xtv_bench: bad arguments");
  Owner sc;
  const long ld = ((long)n + 1023) / 1024 * 1024;  // valid for every variant (multiple of 128*U)
  double *dX, *dv, *part;
  HIPX(sc.alloc(&dX, (size_t)ld * p));
  HIPX(sc.alloc(&dv, (size_t)ld));
  HIPX(sc.alloc(&part, (size_t)(ld / 128) * p));
  HIPX(launch_fill(dX, ld * (long)p, 1.0, nullptr));
  HIPX(launch_fill(dv, ld, 0.5, nullptr));
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  HIPX(launch_xtv_variant(variant, dX, ld, p, dv, part, nullptr));
  HIPX(hipEventRecord(e0, nullptr));
  for (int i = 0; i < repeats; i++) HIPX(launch_xtv_variant(variant, dX, ld, p, dv, part, nullptr));
  HIPX(hipEventRecord(e1, nullptr));
  HIPX(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPX(hipEventElapsedTime(&ms, e0, e1));
  *gbps = 8.0 * (double)n * (double)p * repeats / ((double)ms * 1e-3) / 1e9;
  if (avg_ms) *avg_ms = ms / repeats;
  return BESSX_OK;
}

int bessx_op_xtv_multi_bench(int n, int p, int nc, int two, int repeats, double *gbps, double *avg_ms) {
  if (int rc = need_device()) return rc;
  if (n < 1 || p < 1 || repeats < 1 || !gbps || nc < 1 || nc > XTV_MC_MAX) return fail(BESSX_ERR_ARG, "op_xtv_multi_bench: bad arguments");
  Owner sc;
  const long ld = ((long)n + 1023) / 1024 * 1024;
  double *dX, *dv, *part;
  HIPX(sc.alloc(&dX, (size_t)ld * p));
  HIPX(sc.alloc(&dv, (size_t)ld * 2 * nc));
  HIPX(sc.alloc(&part, (size_t)(ld / 1024) * p * 2 * nc));
  HIPX(launch_fill(dX, ld * (long)p, 1.0, nullptr));
  HIPX(launch_fill(dv, ld * 2 * nc, 0.5, nullptr));
  XtvMc a = {};
  a.nc = nc;
  for (int c = 0; c < nc; c++) {
    a.v[c] = dv + (size_t)(2 * c) * ld;
    a.v2[c] = two ? dv + (size_t)(2 * c + 1) * ld : nullptr;
    a.part[c] = part + (size_t)(2 * c) * (ld / 1024) * p;
    a.part2[c] = part + (size_t)(2 * c + 1) * (ld / 1024) * p;
  }
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  HIPX(launch_xtv_mc(dX, ld, p, 8, a, two != 0, nullptr));
  HIPX(hipEventRecord(e0, nullptr));
  for (int i = 0; i < repeats; i++) HIPX(launch_xtv_mc(dX, ld, p, 8, a, two != 0, nullptr));
  HIPX(hipEventRecord(e1, nullptr));
  HIPX(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPX(hipEventElapsedTime(&ms, e0, e1));
  *gbps = 8.0 * (double)n * (double)p * repeats / ((double)ms * 1e-3) / 1e9;
  if (avg_ms) *avg_ms = ms / repeats;
  return BESSX_OK;
}

int bessx_op_cox_score_bench(int n, int p, int variant, int repeats, double *gbps, double *avg_ms) {
  if (int rc = need_device()) return rc;
  if (n < 1 || p < 1 || repeats < 1 || !gbps) return fail(BESSX_ERR_ARG, "op_cox_score_bench: bad arguments");
  Owner sc;
  const long ld = ((long)n + 1023) / 1024 * 1024;
  const int nrb = (int)(ld / 1024);
  double *dX, *vec, *out;
  HIPX(sc.alloc(&dX, (size_t)ld * p));
  HIPX(sc.alloc(&vec, (size_t)ld * 4));
  HIPX(sc.alloc(&out, (size_t)5 * nrb * p + nrb));
  HIPX(launch_fill(dX, ld * (long)p, 1.0, nullptr));
  HIPX(launch_fill(vec, ld * 4, 0.5, nullptr));
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  // variant 1 (what the solver runs): consecutive waves take consecutive column groups of one row block; 0 (round 3):
  // the row blocks of one column group
  // variant 10 + nc: the multi-chain kernel (k_cox_score1p_mc) with nc chains' vector sets per launch
  const int mc = (variant >= 11 && variant <= 10 + COX_MC_MAX) ? variant - 10 : 0;
  if (!mc && (variant < 0 || variant > 1)) return fail(BESSX_ERR_ARG, "op_cox_score_bench: variant 0, 1 or 11..16");
  if (mc) {
    double *vecs, *outs;
    HIPX(sc.alloc(&vecs, (size_t)ld * 4 * mc));
    HIPX(sc.alloc(&outs, ((size_t)5 * nrb * p + nrb) * mc));
    HIPX(launch_fill(vecs, ld * 4 * mc, 0.5, nullptr));
    CoxMc a = {};
    a.nc = mc;
    for (int c = 0; c < mc; c++) {
      a.TH[c] = vecs + (size_t)(4 * c) * ld;
      a.CU[c] = vecs + (size_t)(4 * c + 1) * ld;
      a.CV[c] = vecs + (size_t)(4 * c + 2) * ld;
      a.C2[c] = vecs + (size_t)(4 * c + 3) * ld;
      a.out[c] = outs + ((size_t)5 * nrb * p + nrb) * c;
    }
    HIPX(launch_cox_score1p_mc(dX, ld, p, 8, nrb, a, nullptr));
    HIPX(hipEventRecord(e0, nullptr));
    for (int i = 0; i < repeats; i++) HIPX(launch_cox_score1p_mc(dX, ld, p, 8, nrb, a, nullptr));
    HIPX(hipEventRecord(e1, nullptr));
    HIPX(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPX(hipEventElapsedTime(&ms, e0, e1));
    *gbps = 8.0 * (double)n * (double)p * repeats / ((double)ms * 1e-3) / 1e9;
    if (avg_ms) *avg_ms = ms / repeats;
    return BESSX_OK;
  }
  cox_score_set_variant(variant);
  CoxBufs cb = {};
  cb.one_pass = 1;
  cb.TH = vec;
  cb.CU = vec + ld;
  cb.CV = vec + 2 * ld;
  cb.C2 = vec + 3 * ld;
  HIPX(launch_cox_score_pass(dX, ld, p, 8, nrb, cb, out, nullptr, nullptr, 0, nullptr));
  HIPX(hipEventRecord(e0, nullptr));
  for (int i = 0; i < repeats; i++) HIPX(launch_cox_score_pass(dX, ld, p, 8, nrb, cb, out, nullptr, nullptr, 0, nullptr));
  HIPX(hipEventRecord(e1, nullptr));
  HIPX(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPX(hipEventElapsedTime(&ms, e0, e1));
  *gbps = 8.0 * (double)n * (double)p * repeats / ((double)ms * 1e-3) / 1e9;
  if (avg_ms) *avg_ms = ms / repeats;
  cox_score_set_variant(1);
  return BESSX_OK;
}

// ---- the Cox solver's state pass and score passes alone (tests/test_cox_ops_gpu.py) ------------------------------
namespace {

// what a session holds of a Cox problem, for one coefficient vector: X padded to the session's row stride, status,
// weights (ones without), the row mask, an open FitCtrl (l = 0 = the `when` of the state pass) and the state vectors
struct CoxOpState {
  int U = 1, nrb = 0, nsse = 0;
  long ld = 0;
  double *X = nullptr, *y = nullptr, *w = nullptr, *mask = nullptr, *b = nullptr, *stats = nullptr;
  int *cols = nullptr;
  FitCtrl *ctrl = nullptr;
  CoxBufs cb = {};
};

int cox_op_check(const char *who, const double *x, int n, int p, const double *status, const int *cols, int m,
                 const double *b) {
  if (!x || !status || n < 1 || p < 1 || m < 0 || m > p || (m > 0 && (!cols || !b)))
    return fail(BESSX_ERR_ARG, std::string(who) + ": bad arguments");
  for (int a = 0; a < m; a++)
    if (cols[a] < 0 || cols[a] >= p) return fail(BESSX_ERR_ARG, std::string(who) + ": column index out of range");
  return 0;
}

// uploads the problem (dX given: X is shared with an earlier state of the same call) and runs launch_cox_state
int cox_op_state(Owner &sc, const double *x, int n, int p, const double *status, const double *weight,
                 const double *mask, const int *cols, int m, const double *b, int one_pass, double *dX, CoxOpState *o) {
  o->U = n >= 4096 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1));  // the session's row stride (bessx_session.cpp)
  if (dX) {
    o->X = dX;
    o->ld = ((long)n + 128L * o->U - 1) / (128L * o->U) * (128L * o->U);
  } else if (int rc = upload_padded(sc, x, n, p, n, o->U, &o->X, &o->ld)) {
    return rc;
  }
  const long ld = o->ld;
  o->nrb = (int)(ld / (128L * o->U));
  o->nsse = (int)((ld + 255) / 256);
  if (int rc = upload_vec_padded(sc, status, n, ld, &o->y)) return rc;
  std::vector<double> ones((size_t)n, 1.0);
  if (int rc = upload_vec_padded(sc, weight ? weight : ones.data(), n, ld, &o->w)) return rc;
  if (mask)
    if (int rc = upload_vec_padded(sc, mask, n, ld, &o->mask)) return rc;
  HIPX(sc.zeros(&o->cols, (size_t)m));
  HIPX(sc.zeros(&o->b, (size_t)m));
  if (m > 0) {
    HIPX(hipMemcpy(o->cols, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    HIPX(hipMemcpy(o->b, b, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
  }
  FitCtrl hc = {};
  hc.k_cur = m;
  HIPX(sc.alloc(&o->ctrl, 1));
  HIPX(hipMemcpy(o->ctrl, &hc, sizeof(FitCtrl), hipMemcpyHostToDevice));
  HIPX(sc.zeros(&o->stats, (size_t)2 * o->nsse));
  CoxBufs &c = o->cb;
  double **vec[] = {&c.E, &c.TH, &c.ET, &c.S0, &c.RS0, &c.SALL, &c.STEST, &c.EW, &c.WD, &c.C1, &c.CU, &c.CV, &c.C2};
  for (double **v : vec) HIPX(sc.zeros(v, (size_t)ld));
  HIPX(sc.zeros(&c.SCR, cox_scan_scratch_doubles(ld, 0)));
  c.one_pass = one_pass;
  HIPX(launch_cox_state(o->X, ld, n, o->y, o->w, o->mask, o->ctrl, 0, o->cols, o->b, c, o->stats, nullptr));
  return 0;
}

// bd (p, host) of the state o: launch_cox_score_pass unless the pass has run already (part given), then launch_cox_score
int cox_op_bd(Owner &sc, const CoxOpState &o, int p, const int *cols, int m, const double *b, double lambda,
              double *part, double *bd) {
  double *part2 = nullptr, *beta, *dbd;
  if (!part) {
    HIPX(sc.zeros(&part, cox_score_part_doubles(o.nrb, p, o.cb.one_pass)));
    if (!o.cb.one_pass) HIPX(sc.zeros(&part2, cox_score_part_doubles(o.nrb, p, 0)));
    HIPX(launch_cox_score_pass(o.X, o.ld, p, o.U, o.nrb, o.cb, part, part2, nullptr, 0, nullptr));
  }
  std::vector<double> hb((size_t)p, 0.0);
  for (int a = 0; a < m; a++) hb[cols[a]] = b[a];
  HIPX(sc.alloc(&beta, (size_t)p));
  HIPX(sc.alloc(&dbd, (size_t)p));
  HIPX(hipMemcpy(beta, hb.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice));
  HIPX(launch_cox_score(part, part2, o.nrb, p, beta, lambda, nullptr, dbd, nullptr, 0, nullptr));
  HIPX(hipMemcpy(bd, dbd, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

int bessx_op_cox_state(const double *x, int n, int p, const double *status, const double *weight, const double *mask,
                       const int *cols, int m, const double *b, double *e, double *theta, double *s0, double *rs0,
                       double *s_all, double *s_test, double *loss) {
  if (int rc = need_device()) return rc;
  if (int rc = cox_op_check("op_cox_state", x, n, p, status, cols, m, b)) return rc;
  Owner sc;
  CoxOpState o;
  if (int rc = cox_op_state(sc, x, n, p, status, weight, mask, cols, m, b, 0, nullptr, &o)) return rc;
  const std::pair<double *, const double *> outs[] = {{e, o.cb.E},        {theta, o.cb.TH},    {s0, o.cb.S0},
                                                      {rs0, o.cb.RS0},    {s_all, o.cb.SALL},  {s_test, mask ? o.cb.STEST : nullptr}};
  for (const auto &pr : outs)
    if (pr.first && pr.second) HIPX(hipMemcpy(pr.first, pr.second, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (loss) {  // added over the blocks in block order, as the session does (finish_fit)
    std::vector<double> part((size_t)2 * o.nsse);
    HIPX(hipMemcpy(part.data(), o.stats, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    double tr = 0.0, te = 0.0;
    for (int blk = 0; blk < o.nsse; blk++) {
      tr += part[2 * blk];
      te += part[2 * blk + 1];
    }
    loss[0] = tr;
    loss[1] = te;
  }
  return BESSX_OK;
}

int bessx_op_cox_score(const double *x, int n, int p, const double *status, const double *weight, const double *mask,
                       const int *cols, int m, const double *b, double lambda, int form, double *bd) {
  if (int rc = need_device()) return rc;
  if (int rc = cox_op_check("op_cox_score", x, n, p, status, cols, m, b)) return rc;
  if (!bd || (form != 0 && form != 1)) return fail(BESSX_ERR_ARG, "op_cox_score: form 0 (two passes) or 1 (one pass)");
  Owner sc;
  CoxOpState o;
  if (int rc = cox_op_state(sc, x, n, p, status, weight, mask, cols, m, b, form, nullptr, &o)) return rc;
  return cox_op_bd(sc, o, p, cols, m, b, lambda, nullptr, bd);
}

int bessx_op_cox_score_multi(const double *x, int n, int p, const double *status, const double *weight,
                             const double *mask, const int *cols, int m, const double *b, int nc, double lambda,
                             double *bd) {
  if (int rc = need_device()) return rc;
  if (nc < 1 || nc > COX_MC_MAX || !bd) return fail(BESSX_ERR_ARG, "op_cox_score_multi: 1 <= nc <= 6");
  if (int rc = cox_op_check("op_cox_score_multi", x, n, p, status, cols, m, b)) return rc;  // b: nc x m, row c = chain c
  Owner sc;
  std::vector<CoxOpState> o((size_t)nc);
  CoxMc a = {};
  a.nc = nc;
  for (int c = 0; c < nc; c++) {
    if (int rc = cox_op_state(sc, x, n, p, status, weight, mask, cols, m, m ? b + (size_t)c * m : b, 1, c ? o[0].X : nullptr, &o[c]))
      return rc;
    a.TH[c] = o[c].cb.TH;
    a.CU[c] = o[c].cb.CU;
    a.CV[c] = o[c].cb.CV;
    a.C2[c] = o[c].cb.C2;
    HIPX(sc.zeros(&a.out[c], cox_score_part_doubles(o[c].nrb, p, 1)));
  }
  HIPX(launch_cox_score1p_mc(o[0].X, o[0].ld, p, o[0].U, o[0].nrb, a, nullptr));
  for (int c = 0; c < nc; c++)
    if (int rc = cox_op_bd(sc, o[c], p, cols, m, m ? b + (size_t)c * m : b, lambda, a.out[c], bd + (size_t)c * p)) return rc;
  return BESSX_OK;
}

namespace {

// the log-likelihood of an IRLS step from its slab / block terms, added as irls_check_body<NT> adds them: thread i takes
// the terms i, i + NT, ... in order, wave_sum folds the 64 lanes of a wave (xor 32, 16, ..., 1), the waves follow in order
double irls_ll_sum(const std::vector<double> &part, int NT) {
  std::vector<double> th((size_t)NT, 0.0);
  for (size_t b = 0; b < part.size(); b++) th[b % NT] += part[b];
  double s = 0.0;
  for (int wv = 0; wv < NT / 64; wv++) {
    double *v = th.data() + 64 * wv, nx[64];
    for (int o = 32; o >= 1; o >>= 1) {
      for (int l = 0; l < 64; l++) nx[l] = v[l] + v[l ^ o];
      std::copy(nx, nx + 64, v);
    }
    s += v[0];
  }
  return s;
}

int glm_op_check(const char *who, int family, const double *x, int n, int p, const double *y, const int *cols, int m,
                 const double *b) {
  if (family != 2 && family != 3) return fail(BESSX_ERR_ARG, std::string(who) + ": family 2 (logistic) or 3 (Poisson)");
  if (!x || !y || n < 1 || p < 1 || m < 0 || m > p || (m > 0 && (!cols || !b)))
    return fail(BESSX_ERR_ARG, std::string(who) + ": bad arguments");
  for (int a = 0; a < m; a++)
    if (cols[a] < 0 || cols[a] >= p) return fail(BESSX_ERR_ARG, std::string(who) + ": column index out of range");
  return 0;
}

// X, y, weights (ones without) and the fold mask (none without) as a session holds them
struct GlmOpData {
  int U = 1, nrb = 0, nsse = 0;
  long ld = 0;
  double *X = nullptr, *y = nullptr, *w = nullptr, *mask = nullptr;
};

int glm_op_upload(Owner &sc, const double *x, int n, int p, const double *y, const double *weight, const double *mask,
                  GlmOpData *o) {
  o->U = n >= 4096 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1));  // the session's row stride (bessx_session.cpp)
  if (int rc = upload_padded(sc, x, n, p, n, o->U, &o->X, &o->ld)) return rc;
  o->nrb = (int)(o->ld / (128L * o->U));
  o->nsse = (int)((o->ld + 255) / 256);
  if (int rc = upload_vec_padded(sc, y, n, o->ld, &o->y)) return rc;
  std::vector<double> ones((size_t)n, 1.0);
  if (int rc = upload_vec_padded(sc, weight ? weight : ones.data(), n, o->ld, &o->w)) return rc;
  if (mask)
    if (int rc = upload_vec_padded(sc, mask, n, o->ld, &o->mask)) return rc;
  return 0;
}

}  // namespace

int bessx_op_glm_gh(int family, const double *x, int n, int p, const double *y, const double *weight, const double *mask,
                    const int *cols, int m, const double *b, double coef0, double lambda, double *g, double *h,
                    double *loss, double *bd) {
  if (int rc = need_device()) return rc;
  if (int rc = glm_op_check("op_glm_gh", family, x, n, p, y, cols, m, b)) return rc;
  Owner sc;
  GlmOpData o;
  if (int rc = glm_op_upload(sc, x, n, p, y, weight, mask, &o)) return rc;
  const long ld = o.ld;
  std::vector<double> lf((size_t)ld, 0.0);
  if (family == 3) poisson_logfact(y, n, lf.data());
  double *dlf, *db, *dg, *dh, *stats;
  int *dcols;
  FitCtrl *ctrl;
  HIPX(sc.alloc(&dlf, (size_t)ld));
  HIPX(hipMemcpy(dlf, lf.data(), (size_t)ld * sizeof(double), hipMemcpyHostToDevice));
  HIPX(sc.zeros(&dcols, (size_t)m));
  HIPX(sc.zeros(&db, (size_t)m));
  if (m > 0) {
    HIPX(hipMemcpy(dcols, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    HIPX(hipMemcpy(db, b, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
  }
  FitCtrl hc = {};  // l = 0: the pass at the start of a fit (when = 0), and slot 1 of the score pass behind it
  hc.k_cur = m;
  hc.coef0 = coef0;
  HIPX(sc.alloc(&ctrl, 1));
  HIPX(hipMemcpy(ctrl, &hc, sizeof(FitCtrl), hipMemcpyHostToDevice));
  HIPX(sc.zeros(&dg, (size_t)ld));
  HIPX(sc.zeros(&dh, (size_t)ld));
  HIPX(sc.zeros(&stats, (size_t)2 * o.nsse));
  HIPX(launch_glm_eta_gh(family, o.X, ld, n, o.y, o.w, o.mask, dlf, ctrl, 0, dcols, db, dg, dh, stats, nullptr));
  if (g) HIPX(hipMemcpy(g, dg, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (h) HIPX(hipMemcpy(h, dh, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (loss) {  // added over the blocks in block order, as the session does (finish_fit)
    std::vector<double> part((size_t)2 * o.nsse);
    HIPX(hipMemcpy(part.data(), stats, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    double tr = 0.0, te = 0.0;
    for (int blk = 0; blk < o.nsse; blk++) {
      tr += part[2 * blk];
      te += part[2 * blk + 1];
    }
    loss[0] = tr;
    loss[1] = te;
  }
  if (bd) {  // the score pass on (g, h) and the sacrifice scores, as enqueue_glm_head queues them
    double *part, *part2, *beta, *dbd;
    HIPX(sc.alloc(&part, (size_t)o.nrb * p));
    HIPX(sc.alloc(&part2, (size_t)o.nrb * p));
    HIPX(sc.alloc(&beta, (size_t)p));
    HIPX(sc.alloc(&dbd, (size_t)p));
    std::vector<double> hb((size_t)p, 0.0);
    for (int a = 0; a < m; a++) hb[cols[a]] = b[a];
    HIPX(hipMemcpy(beta, hb.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice));
    int n_train = n;
    if (mask) {
      n_train = 0;
      for (int i = 0; i < n; i++) n_train += mask[i] != 0.0;
    }
    HIPX(launch_xtv(o.X, ld, p, o.U, dg, dh, part, part2, ctrl, 1, nullptr));
    HIPX(launch_score(part, part2, o.nrb, p, beta, nullptr, (double)n_train, lambda, 1, nullptr, dbd, ctrl, 1, nullptr));
    HIPX(hipMemcpy(bd, dbd, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  }
  return BESSX_OK;
}

namespace {

// first column, width and block offset (sum of s^2) of every group, as a session holds them, on the device: gd, gd + N,
// gd + 2 N (N + 1 offsets)
struct GroupOpLayout {
  int smax = 1;
  std::vector<int> sz, off;
  int *gd = nullptr;
};

int group_op_layout(const char *who, Owner &sc, const int *gidx, int N, int p, GroupOpLayout *o) {
  if (!gidx || N < 1 || p < 1 || N > p || gidx[0] != 0) return fail(BESSX_ERR_ARG, std::string(who) + ": bad group starts");
  o->sz.resize((size_t)N);
  o->off.assign((size_t)N + 1, 0);
  long long tot = 0;
  for (int g = 0; g < N; g++) {
    const int hi = g + 1 < N ? gidx[g + 1] : p;
    if (hi <= gidx[g] || hi > p) return fail(BESSX_ERR_ARG, std::string(who) + ": group starts must ascend below p");
    o->sz[g] = hi - gidx[g];
    tot += (long long)o->sz[g] * o->sz[g];
    if (tot > INT_MAX) return fail(BESSX_ERR_ARG, std::string(who) + ": the group blocks exceed 2^31 entries");
    o->off[g + 1] = (int)tot;
    o->smax = std::max(o->smax, o->sz[g]);
  }
  HIPX(sc.alloc(&o->gd, (size_t)3 * N + 1));
  HIPX(hipMemcpy(o->gd, gidx, (size_t)N * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(o->gd + N, o->sz.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(o->gd + 2 * N, o->off.data(), ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

int upload_flags(Owner &sc, const unsigned char *always, int N, unsigned char **d) {
  *d = nullptr;
  if (!always) return 0;
  HIPX(sc.alloc(d, (size_t)N));
  HIPX(hipMemcpy(*d, always, (size_t)N, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

int bessx_op_group_scores(const double *x, int n, int p, int cshift, const int *gidx, int N, const double *w1,
                          const double *w2, const double *beta_dense, int lm, double n_t, double lambda,
                          const unsigned char *always, const double *part, int nrb, double *mblk, double *dcol,
                          double *bd) {
  if (int rc = need_device()) return rc;
  if (!x || n < 1 || !beta_dense || !mblk || !dcol || !bd || cshift < 0 || cshift >= p)
    return fail(BESSX_ERR_ARG, "op_group_scores: bad arguments");
  if (lm && (!part || nrb < 1 || !(n_t > 0.0))) return fail(BESSX_ERR_ARG, "op_group_scores: lm needs part, nrb >= 1 and n_t > 0");
  Owner sc;
  GroupOpLayout L;
  if (int rc = group_op_layout("op_group_scores", sc, gidx, N, p, &L)) return rc;
  int g0 = 0;  // the panel: the groups from global column cshift on
  while (g0 < N && gidx[g0] != cshift) g0++;
  if (g0 == N) return fail(BESSX_ERR_ARG, "op_group_scores: cshift is not the first column of a group");
  const int Np = N - g0;
  const size_t tot = (size_t)L.off[N];
  double *dX, *dw1 = nullptr, *dw2 = nullptr, *dbeta, *dpart = nullptr, *dm, *dd, *dbd, *work, *zwork, *ev, *el;
  unsigned char *dal;
  long ld;
  if (int rc = upload_padded(sc, x, n, p - cshift, n, 1, &dX, &ld)) return rc;
  if (w1)
    if (int rc = upload_vec_padded(sc, w1, n, ld, &dw1)) return rc;
  if (w2)
    if (int rc = upload_vec_padded(sc, w2, n, ld, &dw2)) return rc;
  if (int rc = upload_flags(sc, always, N, &dal)) return rc;
  HIPX(sc.alloc(&dbeta, (size_t)p));
  HIPX(hipMemcpy(dbeta, beta_dense, (size_t)p * sizeof(double), hipMemcpyHostToDevice));
  if (lm) {
    HIPX(sc.alloc(&dpart, (size_t)nrb * p));
    HIPX(hipMemcpy(dpart, part, (size_t)nrb * p * sizeof(double), hipMemcpyHostToDevice));
  }
  HIPX(sc.zeros(&dm, tot));
  HIPX(sc.alloc(&dd, (size_t)p));
  HIPX(hipMemcpy(dd, dcol, (size_t)p * sizeof(double), hipMemcpyHostToDevice));
  HIPX(sc.zeros(&dbd, (size_t)3 * N));
  HIPX(sc.zeros(&work, tot));  // sized as the session sizes them: sum of s^2, 2 p
  HIPX(sc.zeros(&zwork, (size_t)2 * p));
  HIPX(sc.zeros(&ev, tot));
  HIPX(sc.zeros(&el, (size_t)p));
  const int *gi = L.gd + g0, *gs = L.gd + N + g0, *go = L.gd + 2 * N + g0;
  HIPX(launch_group_moments(L.smax, dX, ld, n, dw1, dw2, Np, gi, gs, go, dm, dd, nullptr, cshift));
  for (int mode = 0; mode < 3; mode++)
    HIPX(launch_group_score(Np, gi, gs, go, dm, dd, dpart, nrb, p, lm, n_t, lambda, dbeta, dal ? dal + g0 : nullptr,
                            dbd + (size_t)mode * N + g0, nullptr, L.smax, work, zwork, nullptr, 0, mode, ev, el));
  HIPX(hipDeviceSynchronize());
  HIPX(hipMemcpy(mblk, dm, tot * sizeof(double), hipMemcpyDeviceToHost));
  HIPX(hipMemcpy(dcol, dd, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
  HIPX(hipMemcpy(bd, dbd, (size_t)3 * N * sizeof(double), hipMemcpyDeviceToHost));
  return BESSX_OK;
}

int bessx_op_group_lsq(const double *x, int n, int p, const int *gidx, int N, const double *yw,
                       const unsigned char *always, double *score) {
  if (int rc = need_device()) return rc;
  if (!x || n < 1 || !yw || !score) return fail(BESSX_ERR_ARG, "op_group_lsq: bad arguments");
  Owner sc;
  GroupOpLayout L;
  if (int rc = group_op_layout("op_group_lsq", sc, gidx, N, p, &L)) return rc;
  const size_t tot = (size_t)L.off[N];
  double *dX, *dyw, *dm, *dd, *work, *zwork, *ds;
  unsigned char *dal;
  long ld;
  if (int rc = upload_padded(sc, x, n, p, n, 1, &dX, &ld)) return rc;
  if (int rc = upload_vec_padded(sc, yw, n, ld, &dyw)) return rc;
  if (int rc = upload_flags(sc, always, N, &dal)) return rc;
  HIPX(sc.zeros(&dm, tot));
  HIPX(sc.zeros(&dd, (size_t)p));
  HIPX(sc.zeros(&work, tot));
  HIPX(sc.zeros(&zwork, (size_t)p));
  HIPX(sc.zeros(&ds, (size_t)N));
  HIPX(launch_group_moments(L.smax, dX, ld, n, nullptr, dyw, N, L.gd, L.gd + N, L.gd + 2 * N, dm, dd, nullptr));
  HIPX(launch_group_lsq_score(N, L.gd, L.gd + N, L.gd + 2 * N, dm, dd, dal, work, zwork, ds, nullptr));
  HIPX(hipDeviceSynchronize());
  HIPX(hipMemcpy(score, ds, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return BESSX_OK;
}

int bessx_op_glm_irls_geometry(int T0, int n, int *out) {
  if (T0 < 1 || T0 > T0_FAST || n < 1 || !out) return fail(BESSX_ERR_ARG, "op_glm_irls_geometry: bad arguments");
  const int U = n >= 4096 ? 8 : (n >= 2048 ? 4 : (n >= 1024 ? 2 : 1));
  const long ld = ((long)n + 128L * U - 1) / (128L * U) * (128L * U);
  const int mt = (T0 + 2 + 15) / 16;
  out[0] = (int)ld;
  out[1] = mt;
  out[2] = irls_gram_chunks(mt);
  out[3] = irls_gram_slab_rows(mt, ld);
  return BESSX_OK;
}

int bessx_op_glm_irls(int family, int route, int t, int wfloor, double lambda, int rows_per_slab, const double *x, int n,
                      int p, const double *y, const double *weight, const double *mask, const int *cols, int T0,
                      const double *bcur, double *gram, double *ll, double *wv, double *z, double *bnext,
                      int *route_taken) {
  if (int rc = need_device()) return rc;
  if (int rc = glm_op_check("op_glm_irls", family, x, n, p, y, cols, T0, bcur)) return rc;
  if (T0 < 1 || T0 > T0_FAST || !bcur || !gram || route < -1 || route > 1 || t < 0 || rows_per_slab < 0 ||
      rows_per_slab % 64 != 0)
    return fail(BESSX_ERR_ARG, "op_glm_irls: bad arguments");
  const int mt = (T0 + 2 + 15) / 16, mp = mt * 16, ntiles = mt * (mt + 1) / 2;  // glm_geometry
  // route -1: the rule of enqueue_glm_irls_step (the fused step up to 8 tile rows, the five-launch step beyond)
  const bool fused = route == 1 || (route == -1 && irls_gram_applies(mt));
  if (fused && !irls_gram_applies(mt)) return fail(BESSX_ERR_UNSUPPORTED, "op_glm_irls: the fused step takes at most 8 tile rows");
  if (!fused && rows_per_slab != 0) return fail(BESSX_ERR_ARG, "op_glm_irls: rows_per_slab belongs to the fused step");
  Owner sc;
  GlmOpData o;
  if (int rc = glm_op_upload(sc, x, n, p, y, weight, mask, &o)) return rc;
  const long ld = o.ld;
  HIPX(gram_lds_prepare());
  double *aux, *db, *Gt, *gpart, *llpart, *Wv = nullptr, *dfb;
  int *A_new, *A_cur, *gcols;
  FitCtrl *ctrl;
  {  // aux: column 0 zeros, column 1 ones on the data rows, column 2 the working response
    std::vector<double> ha((size_t)ld * 3, 0.0);
    std::fill(ha.begin() + ld, ha.begin() + ld + n, 1.0);
    HIPX(sc.alloc(&aux, ha.size()));
    HIPX(hipMemcpy(aux, ha.data(), ha.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  HIPX(sc.alloc(&A_new, (size_t)T0));
  HIPX(sc.zeros(&A_cur, (size_t)T0));
  HIPX(sc.alloc(&gcols, (size_t)mp + 16));
  HIPX(hipMemcpy(A_new, cols, (size_t)T0 * sizeof(int), hipMemcpyHostToDevice));
  HIPX(sc.zeros(&db, (size_t)mp + 16));
  HIPX(hipMemcpy(db, bcur, (size_t)(T0 + 1) * sizeof(double), hipMemcpyHostToDevice));
  FitCtrl hc = {};  // slot 1 of a fit, IRLS step t of its sub-model fit still to do
  hc.T0 = T0;
  hc.irls_steps = t;
  HIPX(sc.alloc(&ctrl, 1));
  HIPX(hipMemcpy(ctrl, &hc, sizeof(FitCtrl), hipMemcpyHostToDevice));
  HIPX(sc.alloc(&Gt, (size_t)ntiles * 256));
  HIPX(sc.alloc(&dfb, CHOL_FB_DOUBLES));
  const int slot = 1;
  HIPX(launch_gram_cols(A_new, T0, mp, 1, 1, gcols, ctrl, slot, A_cur, family == 2 ? 1 : 0, nullptr));
  std::vector<double> hll;
  if (fused) {
    const int rows = rows_per_slab ? rows_per_slab : irls_gram_slab_rows(mt, ld);
    const int ns = (int)((ld + rows - 1) / rows);
    HIPX(sc.alloc(&gpart, (size_t)ns * ntiles * 256));
    HIPX(sc.alloc(&llpart, (size_t)ns));
    HIPX(launch_irls_gram(family, o.X, aux, ld, n, gcols, o.y, o.w, o.mask, ns, mt, gpart, ntiles, ctrl, slot, t, T0, db,
                          llpart, nullptr, wfloor, rows_per_slab));
    HIPX(launch_gram_reduce(gpart, ns, ntiles, Gt, ctrl, slot, 1, nullptr));
    hll.resize((size_t)ns);
  } else {
    std::vector<GramTask> tasks;
    build_gram_tasks(mt, tasks);
    GramTask *dt;
    HIPX(sc.alloc(&dt, tasks.size()));
    HIPX(hipMemcpy(dt, tasks.data(), tasks.size() * sizeof(GramTask), hipMemcpyHostToDevice));
    bessx_session fake;
    fake.ld = ld;
    int rps, nslab;
    gram_geometry(&fake, (int)tasks.size(), &rps, &nslab, ntiles);
    HIPX(sc.alloc(&gpart, (size_t)nslab * ntiles * 256));
    HIPX(sc.alloc(&llpart, (size_t)o.nsse));
    HIPX(sc.zeros(&Wv, (size_t)ld));
    HIPX(launch_glm_irls_prep(family, o.X, ld, n, o.y, o.w, o.mask, ctrl, slot, t, A_new, T0, db, Wv, aux + 2 * ld, llpart,
                              nullptr, wfloor));
    HIPX(launch_gram(o.X, aux, ld, gcols, Wv, rps, dt, (int)tasks.size(), nslab, gpart, ntiles, Gt, ctrl, slot, 1, nullptr));
    hll.resize((size_t)o.nsse);
  }
  HIPX(hipMemcpy(hll.data(), llpart, hll.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (ll) *ll = irls_ll_sum(hll, fused ? 512 : 256);  // (the test rides in k_chol, 512 threads, or is k_glm_irls_check, 256)
  if (route_taken) *route_taken = fused ? 1 : 0;
  if (!fused) {
    if (wv) HIPX(hipMemcpy(wv, Wv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (z) HIPX(hipMemcpy(z, aux + 2 * ld, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  }
  {  // rows and columns 0 .. T0 of the tiles are [1, X_A]; the working response is Gram column mp - 1
    std::vector<double> ht((size_t)ntiles * 256);
    HIPX(hipMemcpy(ht.data(), Gt, ht.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int M = T0 + 2;
    auto pos = [&](int rc) { return rc <= T0 ? rc : (rc == mp - 1 ? T0 + 1 : -1); };
    for (int I = 0; I < mt; I++)
      for (int J = 0; J <= I; J++) {
        const int tl = I * (I + 1) / 2 + J;
        for (int lane = 0; lane < 64; lane++)
          for (int r = 0; r < 4; r++) {
            const int row = pos(I * 16 + (lane >> 4) + 4 * r), col = pos(J * 16 + (lane & 15));
            if (row < 0 || col < 0) continue;
            const double v = ht[(size_t)tl * 256 + lane * 4 + r];
            gram[(size_t)col * M + row] = v;
            if (I != J) gram[(size_t)row * M + col] = v;
          }
      }
  }
  if (bnext) {  // the solve of the step as the session queues it, without the convergence test at its head
    CholFuse fbz = {};
    fbz.fb_work = dfb;
    HIPX(launch_chol(Gt, T0 + 1, mt, 2.0 * lambda, 1, nullptr, nullptr, db, &ctrl->info, ctrl, slot, 1, nullptr, &fbz));
    // (a chain whose k_chol stood back carries the pivoted solve behind it: glm_fallback)
    HIPX(launch_sym_fallback(Gt, T0 + 1, mt, 2.0 * lambda, 1, nullptr, nullptr, db, &ctrl->info, ctrl, slot, nullptr, &fbz));
    HIPX(hipMemcpy(bnext, db, (size_t)(T0 + 1) * sizeof(double), hipMemcpyDeviceToHost));
    HIPX(hipMemcpy(&hc, ctrl, sizeof(FitCtrl), hipMemcpyDeviceToHost));
    if (hc.info) return fail(BESSX_ERR_NUMERIC, "op_glm_irls: the solve of the step gave up (singular system?)");
  }
  return BESSX_OK;
}

int bessx_op_stream_copy_gbps(long long bytes, int repeats, double *gbps) {
  if (int rc = need_device()) return rc;
  if (bytes < (1 << 20) || repeats < 1 || !gbps) return fail(BESSX_ERR_ARG, "op_stream_copy: bad arguments");
  Owner sc;
  double *a, *b;
  size_t n = (size_t)bytes / 16 * 2;
  HIPX(sc.alloc(&a, n));
  HIPX(sc.alloc(&b, n));
  HIPX(hipMemset(a, 1, n * sizeof(double)));
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  HIPX(launch_copy(a, b, (long)n, nullptr));
  HIPX(hipEventRecord(e0, nullptr));
  for (int i = 0; i < repeats; i++) HIPX(launch_copy(a, b, (long)n, nullptr));
  HIPX(hipEventRecord(e1, nullptr));
  HIPX(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPX(hipEventElapsedTime(&ms, e0, e1));
  *gbps = 2.0 * (double)n * 8.0 * repeats / ((double)ms * 1e-3) / 1e9;
  return BESSX_OK;
}

// the ingest kernel alone on a caller's device matrix (tests/test_device_input_gpu.py)
static int op_ingest_prepare(const void *x, int dtype, long long rs, long long cs, const int *row_order, int n, int p,
                             long long ld, Owner &sc, double **dst, unsigned **flag, int **order_d) {
  if (int rc = need_device()) return rc;
  if (ld < n || ld % 128 != 0) return fail(BESSX_ERR_ARG, "op_ingest: ld must be a multiple of 128, at least n");
  int dev = -1;
  if (int rc = check_device_matrix("op_ingest: x", x, dtype, rs, cs, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  *order_d = nullptr;
  if (row_order) {
    for (int i = 0; i < n; i++)
      if (row_order[i] < 0 || row_order[i] >= n) return fail(BESSX_ERR_ARG, "op_ingest: row_order entry out of range");
    HIPX(sc.alloc(order_d, (size_t)n));
    HIPX(hipMemcpy(*order_d, row_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  }
  HIPX(sc.alloc(dst, (size_t)ld * p));
  HIPX(sc.alloc(flag, 1));
  return 0;
}

int bessx_op_ingest(const void *x, int dtype, long long row_stride, long long col_stride, const int *row_order, int n,
                    int p, long long ld, void *stream, double *out, int *nan_flag) {
  if (!out || !nan_flag) return fail(BESSX_ERR_ARG, "op_ingest: null argument");
  Owner sc;
  double *dst = nullptr;
  unsigned *flag = nullptr;
  int *od = nullptr;
  if (int rc = op_ingest_prepare(x, dtype, row_stride, col_stride, row_order, n, p, ld, sc, &dst, &flag, &od)) return rc;
  HIPX(hipMemset(dst, 0xff, (size_t)ld * p * sizeof(double)));  // the kernel itself must write every padding row
  hipStream_t st = nullptr;
  HIPX(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int rc = ingest_enqueue(x, dtype == BESSX_F32, row_stride, col_stride, od, n, p, dst, ld, flag,
                          static_cast<hipStream_t>(stream), st);
  unsigned h = 0;
  if (rc == 0) {
    hipError_t e = hipMemcpyAsync(out, dst, (size_t)ld * p * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h, flag, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = fail(BESSX_ERR_HIP, std::string("op_ingest: ") + hipGetErrorString(e));
  }
  (void)hipStreamDestroy(st);
  *nan_flag = h ? 1 : 0;
  return rc;
}

int bessx_op_ingest_bench(const void *x, int dtype, long long row_stride, long long col_stride, const int *row_order,
                          int n, int p, long long ld, int repeats, double *avg_ms, double *gbps) {
  if (repeats < 1 || !avg_ms || !gbps) return fail(BESSX_ERR_ARG, "op_ingest_bench: bad arguments");
  Owner sc;
  double *dst = nullptr;
  unsigned *flag = nullptr;
  int *od = nullptr;
  if (int rc = op_ingest_prepare(x, dtype, row_stride, col_stride, row_order, n, p, ld, sc, &dst, &flag, &od)) return rc;
  HIPX(hipMemset(flag, 0, sizeof(unsigned)));
  HIPX(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  const int f32 = dtype == BESSX_F32;
  HIPX(launch_ingest(x, f32, row_stride, col_stride, od, n, p, dst, ld, flag, nullptr));
  HIPX(hipEventRecord(e0, nullptr));
  for (int i = 0; i < repeats; i++) HIPX(launch_ingest(x, f32, row_stride, col_stride, od, n, p, dst, ld, flag, nullptr));
  HIPX(hipEventRecord(e1, nullptr));
  HIPX(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPX(hipEventElapsedTime(&ms, e0, e1));
  const double bytes = (double)n * (double)p * (f32 ? 4.0 : 8.0) + (double)ld * (double)p * 8.0;
  *avg_ms = ms / repeats;
  *gbps = bytes * repeats / ((double)ms * 1e-3) / 1e9;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// prediction on a caller's device matrix (include/bessx.h section 2c)
// ----------------------------------------------------------------------------------------------
static int predict_run(Owner &sc, std::vector<double> &tmp, const void *x, int f32, long long rs, long long cs, int n,
                       const int *cols, int m, const double *B, const double *coef0, int R, int link, double *out,
                       long long ors, long long ocs, double *out2, int out_on_device, hipStream_t st) {
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *stage = nullptr;
  if (int rc = predict_upload_model(sc, cols, m, B, coef0, R, st, &cols_d, &B_d, &c_d)) return rc;
  const bool two = link == BESSX_LINK_LOGISTIC;
  const size_t cnt = (size_t)n * R;
  if (out_on_device) {
    HIPX(launch_predict(x, f32, rs, cs, n, cols_d, m, B_d, c_d, R, link, out, ors, ocs, out2, st));
    HIPX(hipStreamSynchronize(st));
    return 0;
  }
  HIPX(sc.alloc(&stage, cnt * (two ? 2 : 1)));
  HIPX(launch_predict(x, f32, rs, cs, n, cols_d, m, B_d, c_d, R, link, stage, R, 1, two ? stage + cnt : nullptr, st));
  const bool dense = ocs == 1 && ors == R;  // (R == 1: any ocs addresses the same elements)
  double *h1 = out, *h2 = out2;
  if (!(dense || (R == 1 && ors == 1))) {
    tmp.resize(cnt * (two ? 2 : 1));
    h1 = tmp.data();
    h2 = tmp.data() + cnt;
  }
  HIPX(hipMemcpyAsync(h1, stage, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  if (two) HIPX(hipMemcpyAsync(h2, stage + cnt, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  if (!tmp.empty()) {
    for (long long i = 0; i < n; i++)
      for (long long r = 0; r < R; r++) {
        out[i * ors + r * ocs] = h1[i * R + r];
        if (two) out2[i * ors + r * ocs] = h2[i * R + r];
      }
  }
  return 0;
}

extern "C" {

int bessx_predict_device(const void *x, int x_dtype, long long x_row_stride, long long x_col_stride, int n, int p,
                         const int *cols, int m, const double *B, const double *coef0, int R, int link, double *out,
                         long long out_row_stride, long long out_col_stride, double *out2, int out_on_device,
                         void *stream) {
  if (!x || !coef0 || !out) return fail(BESSX_ERR_ARG, "predict_device: null argument");
  if (int rc = check_x_model("predict_device", x, x_dtype,
                             x_row_stride >= 0 && x_col_stride >= 0 && out_row_stride >= 0 && out_col_stride >= 0, n, p,
                             cols, m, B, R, link, false))
    return rc;
  if (link == BESSX_LINK_LOGISTIC && !out2) return fail(BESSX_ERR_ARG, "predict_device: the logistic link needs out2");
  if ((n > 1 && out_row_stride == 0) || (R > 1 && out_col_stride == 0))
    return fail(BESSX_ERR_ARG, "predict_device: out: a zero stride along an axis longer than 1");
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("predict_device: x", x, x_dtype, x_row_stride, x_col_stride, n, p, &dev)) return rc;
  if (out_on_device) {
    if (int rc = check_on_device("predict_device", "out", out, BESSX_F64, out_row_stride, out_col_stride, n, R, dev))
      return rc;
    if (link == BESSX_LINK_LOGISTIC)
      if (int rc = check_on_device("predict_device", "out2", out2, BESSX_F64, out_row_stride, out_col_stride, n, R, dev))
        return rc;
  }
  return dev_call(dev, static_cast<hipStream_t>(stream), [&](DevCall &dc) {
    return predict_run(dc.sc, dc.h, x, x_dtype == BESSX_F32, x_row_stride, x_col_stride, n, cols, m, B, coef0, R, link, out,
                       out_row_stride, out_col_stride, out2, out_on_device, dc.st);
  });
}

int bessx_op_predict_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                           const int *cols, int m, int R, int link, int repeats, double *avg_ms, double *gbps) {
  if (!x || repeats < 1 || !avg_ms || !gbps) return fail(BESSX_ERR_ARG, "op_predict_bench: bad arguments");
  if (int rc = predict_check_model("op_predict_bench", n, p, cols, m, R, link)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_predict_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  std::vector<double> B((size_t)m * R), c0((size_t)R, 0.25);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *out = nullptr;
  if (int rc = predict_upload_model(sc, cols, m, B.data(), c0.data(), R, nullptr, &cols_d, &B_d, &c_d)) return rc;
  const size_t cnt = (size_t)n * R;
  HIPX(sc.alloc(&out, 2 * cnt));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  float ms = 0.f;
  if (int rc = bt.run(repeats, &ms, [&]() -> int {
        HIPX(launch_predict(x, f32, row_stride, col_stride, n, cols_d, m, B_d, c_d, R, link, out, R, 1, out + cnt, nullptr));
        return 0;
      }))
    return rc;
  const double bytes = (double)n * (double)m * (f32 ? 4.0 : 8.0) + (double)cnt * 8.0;
  *avg_ms = ms / repeats;
  *gbps = bytes * repeats / ((double)ms * 1e-3) / 1e9;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// held-out loss on a caller's device matrix (include/bessx.h section 2d)
// ----------------------------------------------------------------------------------------------
// everything about the call that needs no device
static int eval_check_args(const char *who, const GlmCall &c, const double *loss, const double *aux, const double *sum_w) {
  const std::string w(who);
  if (!loss || !sum_w) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = glm_check(who, c, false)) return rc;
  if (c.link == BESSX_LINK_LOGISTIC && !aux) return fail(BESSX_ERR_ARG, w + ": the logistic link needs aux");
  return 0;
}

// y and the weights as the kernel reads them: the caller's device memory where it lies, host data through a buffer of `sc`
static int eval_stage_data(Owner &sc, const GlmCall &c, hipStream_t st, EvalData *d) {
  const long long n = c.n;
  const long long ycs = c.y_cols == 1 ? 0 : c.y_cs;
  *d = EvalData{nullptr, 0, c.y_rs, ycs, nullptr, 0, 0};
  if (c.y_dev) {
    d->y = c.y_dev;
    d->y_f32 = c.y_dtype == BESSX_F32;
  } else {
    const size_t span = (size_t)((n - 1) * c.y_rs + (c.y_cols - 1) * ycs + 1);
    double *yd = nullptr;
    HIPX(sc.alloc(&yd, span));
    HIPX(hipMemcpyAsync(yd, c.y_host, span * sizeof(double), hipMemcpyHostToDevice, st));
    d->y = yd;
  }
  if (c.w_dev) {
    d->w = c.w_dev;
    d->w_f32 = c.w_dtype == BESSX_F32;
    d->ws = c.w_stride;
  } else if (c.w_host) {
    double *wd = nullptr;
    HIPX(sc.alloc(&wd, (size_t)n));
    HIPX(hipMemcpyAsync(wd, c.w_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    d->w = wd;
    d->ws = 1;
  }
  return 0;
}

static int eval_run(Owner &sc, std::vector<double> &h, const GlmCall &c, double *loss, double *aux, double *sum_w,
                    hipStream_t st) {
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *work = nullptr, *res = nullptr;
  const int R = c.R, f32 = c.f32();
  if (int rc = predict_upload_model(sc, c.cols, c.m, c.beta, c.coef0, R, st, &cols_d, &B_d, &c_d)) return rc;
  EvalData d;
  if (int rc = eval_stage_data(sc, c, st, &d)) return rc;
  const long long nwork = eval_workspace(f32, c.rs, c.cs, c.n, c.m, R, c.link, d.w != nullptr);
  HIPX(sc.alloc(&work, (size_t)nwork));
  HIPX(sc.alloc(&res, 2 * (size_t)R + 1));
  HIPX(launch_eval(c.x, f32, c.rs, c.cs, c.n, cols_d, c.m, B_d, c_d, R, c.link, d, work, res, st));
  h.resize(2 * (size_t)R + 1);
  HIPX(hipMemcpyAsync(h.data(), res, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  std::copy(h.begin(), h.begin() + R, loss);
  if (c.link == BESSX_LINK_LOGISTIC) std::copy(h.begin() + R, h.begin() + 2 * R, aux);
  *sum_w = d.w ? h[2 * (size_t)R] : (double)c.n;
  return 0;
}

extern "C" {

int bessx_eval_device(const bessx_eval_input *in, double *loss, double *aux, double *sum_w) {
  if (!in) return fail(BESSX_ERR_ARG, "eval_device: null argument");
  const GlmCall c = glm_call(in);
  if (int rc = eval_check_args("eval_device", c, loss, aux, sum_w)) return rc;
  int dev = -1;
  if (int rc = glm_check_device("eval_device", c, &dev)) return rc;
  return dev_call(dev, c.stream, [&](DevCall &dc) { return eval_run(dc.sc, dc.h, c, loss, aux, sum_w, dc.st); });
}

int bessx_op_eval_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                        const int *cols, int m, int R, int link, int y_cols, int repeats, double *avg_ms,
                        double *gbps) {
  if (!x || repeats < 1 || !avg_ms || !gbps) return fail(BESSX_ERR_ARG, "op_eval_bench: bad arguments");
  if (int rc = predict_check_model("op_eval_bench", n, p, cols, m, R, link)) return rc;
  if (y_cols != 1 && y_cols != R) return fail(BESSX_ERR_ARG, "op_eval_bench: y_cols must be 1 or R");
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_eval_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  std::vector<double> B((size_t)m * R), c0((size_t)R, 0.25), y((size_t)n * y_cols), wt((size_t)n, 1.0);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (size_t q = 0; q < y.size(); q++) y[q] = (double)(q % 2);
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *y_d = nullptr, *w_d = nullptr, *work = nullptr, *res = nullptr;
  if (int rc = predict_upload_model(sc, cols, m, B.data(), c0.data(), R, nullptr, &cols_d, &B_d, &c_d)) return rc;
  HIPX(sc.alloc(&y_d, y.size()));
  HIPX(sc.alloc(&w_d, wt.size()));
  HIPX(hipMemcpy(y_d, y.data(), y.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(w_d, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice));
  const int f32 = dtype == BESSX_F32;
  const EvalData d{y_d, 0, 1, y_cols == 1 ? 0 : (long long)n, w_d, 0, 1};  // (y column by column)
  HIPX(sc.alloc(&work, (size_t)eval_workspace(f32, row_stride, col_stride, n, m, R, link, 1)));
  HIPX(sc.alloc(&res, 2 * (size_t)R + 1));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  float ms = 0.f;
  if (int rc = bt.run(repeats, &ms, [&]() -> int {
        HIPX(launch_eval(x, f32, row_stride, col_stride, n, cols_d, m, B_d, c_d, R, link, d, work, res, nullptr));
        return 0;
      }))
    return rc;
  const double bytes = (double)n * (double)m * (f32 ? 4.0 : 8.0) + (double)n * 8.0 * (y_cols + 1.0);
  *avg_ms = ms / repeats;
  *gbps = bytes * repeats / ((double)ms * 1e-3) / 1e9;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// held-out Cox partial likelihood and concordance on a caller's device matrix (include/bessx.h section 2e)
// ----------------------------------------------------------------------------------------------
namespace {

// the host side of the time order: everything the kernels need about time, status and weight
struct CoxOrder {
  std::vector<int> pos, first, kg;  // pos[row] = position; first[k]; kg[k] = first[k] for an event, INT_MAX otherwise
  std::vector<double> wd;           // w * status in position order
  long long comparable = 0;
};

void cox_order(const double *time, const double *status, const double *weight, int n, CoxOrder *o) {
  std::vector<int> idx((size_t)n);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [time](int a, int b) { return time[a] < time[b]; });
  o->pos.resize((size_t)n);
  o->first.resize((size_t)n);
  o->kg.resize((size_t)n);
  o->wd.resize((size_t)n);
  for (int k = 0; k < n; k++) {
    const int i = idx[(size_t)k];
    o->pos[(size_t)i] = k;
    o->first[(size_t)k] = (k > 0 && time[idx[(size_t)k - 1]] == time[i]) ? o->first[(size_t)k - 1] : k;
    o->kg[(size_t)k] = status[i] != 0.0 ? o->first[(size_t)k] : INT_MAX;
    o->wd[(size_t)k] = (weight ? weight[i] : 1.0) * status[i];
  }
  // an event at position k is comparable with every position behind its tie group
  o->comparable = 0;
  for (int k = n - 1, end = n; k >= 0; k--) {  // end: first position with a later time than position k
    if (k < n - 1 && o->first[(size_t)k + 1] != o->first[(size_t)k]) end = k + 1;
    if (o->kg[(size_t)k] != INT_MAX) o->comparable += n - end;
  }
}

int cox_eval_check_args(const char *who, const CoxCall &c, const bessx_cox_eval_input *in, const double *loglik,
                        const long long *pairs, const long long *comparable) {
  const std::string w(who);
  if (!loglik || !comparable) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = cox_check(who, c, false)) return rc;
  if (in->R > 65535) return fail(BESSX_ERR_ARG, w + ": R must be at most 65535");
  if (in->want_pairs && !pairs) return fail(BESSX_ERR_ARG, w + ": want_pairs needs pairs");
  return 0;
}

// the device side of one problem: buffers of `sc`, uploads queued on st (the vectors of `o` must outlive them)
struct CoxDev {
  int *cols = nullptr, *pos = nullptr, *first = nullptr, *kg = nullptr;
  double *B = nullptr, *zero = nullptr, *wd = nullptr, *eta = nullptr, *ex = nullptr, *work = nullptr, *res = nullptr;
  unsigned long long *cnt = nullptr;
};

int cox_eval_stage(Owner &sc, const CoxOrder &o, const int *cols, int m, const double *B, int R, int n, int need_first,
                   int want_pairs, hipStream_t st, CoxDev *d) {
  const size_t N = (size_t)n;
  HIPX(sc.alloc(&d->B, (size_t)m * R + (size_t)R));
  HIPX(sc.alloc(&d->cols, (size_t)m));
  d->zero = d->B + (size_t)m * R;
  HIPX(hipMemsetAsync(d->zero, 0, (size_t)R * sizeof(double), st));
  if (m > 0) {
    HIPX(hipMemcpyAsync(d->cols, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(hipMemcpyAsync(d->B, B, (size_t)m * R * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIPX(sc.alloc(&d->pos, N));
  HIPX(hipMemcpyAsync(d->pos, o.pos.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(sc.alloc(&d->wd, N));
  HIPX(hipMemcpyAsync(d->wd, o.wd.data(), N * sizeof(double), hipMemcpyHostToDevice, st));
  if (need_first || want_pairs) {
    HIPX(sc.alloc(&d->first, N));
    HIPX(hipMemcpyAsync(d->first, o.first.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (want_pairs) {
    HIPX(sc.alloc(&d->kg, N));
    HIPX(hipMemcpyAsync(d->kg, o.kg.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&d->cnt, 2 * (size_t)R));
  }
  HIPX(sc.alloc(&d->eta, N * R));
  HIPX(sc.alloc(&d->ex, N * R));
  HIPX(sc.alloc(&d->work, (size_t)cox_eval_workspace(n, R)));
  HIPX(sc.alloc(&d->res, (size_t)R));
  return 0;
}

int cox_eval_run(Owner &sc, const CoxOrder &o, std::vector<double> &hl, std::vector<unsigned long long> &hc,
                 const bessx_cox_eval_input *in, double *loglik, long long *pairs, hipStream_t st) {
  const int R = in->R, n = in->n, f32 = in->x_dtype == BESSX_F32;
  CoxDev d;
  if (int rc = cox_eval_stage(sc, o, in->cols, in->m, in->B, R, n, in->ties == 1, in->want_pairs, st, &d)) return rc;
  HIPX(launch_cox_eval_eta(in->x, f32, in->x_row_stride, in->x_col_stride, n, d.cols, in->m, d.B, d.zero, R, d.pos,
                           d.eta, d.ex, st));
  HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, in->ties == 1 ? d.first : nullptr, n, R, d.work, d.res, st));
  hl.resize((size_t)R);
  HIPX(hipMemcpyAsync(hl.data(), d.res, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
  if (in->want_pairs) {
    HIPX(launch_cox_eval_pairs(d.eta, d.kg, d.first, n, R, d.cnt, st));
    hc.resize(2 * (size_t)R);
    HIPX(hipMemcpyAsync(hc.data(), d.cnt, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  std::copy(hl.begin(), hl.end(), loglik);
  if (in->want_pairs)
    for (int r = 0; r < R; r++) {
      const long long c = (long long)hc[2 * (size_t)r], dd = (long long)hc[2 * (size_t)r + 1];
      pairs[3 * r] = c;
      pairs[3 * r + 1] = dd;
      pairs[3 * r + 2] = o.comparable - c - dd;
    }
  return 0;
}

}  // namespace

extern "C" {

int bessx_eval_cox_device(const bessx_cox_eval_input *in, double *loglik, long long *pairs, long long *comparable) {
  if (!in) return fail(BESSX_ERR_ARG, "eval_cox_device: null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_eval_check_args("eval_cox_device", c, in, loglik, pairs, comparable)) return rc;
  int dev = -1;
  if (int rc = cox_check_device("eval_cox_device", c, &dev)) return rc;
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  std::vector<unsigned long long> hc;
  const int rc = dev_call(dev, c.stream,
                          [&](DevCall &dc) { return cox_eval_run(dc.sc, o, dc.h, hc, in, loglik, pairs, dc.st); });
  if (!rc) *comparable = o.comparable;
  return rc;
}

int bessx_op_cox_eval_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int R, int ties, int want_pairs, int repeats, double *stage_ms) {
  if (!x || repeats < 1 || !stage_ms) return fail(BESSX_ERR_ARG, "op_cox_eval_bench: bad arguments");
  if (int rc = predict_check_model("op_cox_eval_bench", n, p, cols, m, R, BESSX_LINK_IDENTITY)) return rc;
  if (R > 65535) return fail(BESSX_ERR_ARG, "op_cox_eval_bench: R must be at most 65535");
  if (ties != 0 && ties != 1) return fail(BESSX_ERR_ARG, "op_cox_eval_bench: ties must be 0 (order) or 1 (breslow)");
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_eval_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m * R), time((size_t)n), status((size_t)n);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int i = 0; i < n; i++) {  // distinct times in an order that is not the rows'
    time[(size_t)i] = (double)(((long long)i * 7919) % n) + (double)i / (2.0 * n);
    status[(size_t)i] = (double)(i % 2);
  }
  CoxOrder o;
  cox_order(time.data(), status.data(), nullptr, n, &o);
  Owner sc;
  CoxDev d;
  if (int rc = cox_eval_stage(sc, o, cols, m, B.data(), R, n, ties == 1, want_pairs, nullptr, &d)) return rc;
  HIPX(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  const int f32 = dtype == BESSX_F32;
  double *keep = nullptr;  // the scan works in place: every timed launch of stage 2 starts from a fresh copy of ex
  HIPX(sc.alloc(&keep, (size_t)n * R));
  for (int stage = 0; stage < 3; stage++) {
    stage_ms[stage] = 0.0;
    if (stage == 2 && !want_pairs) break;
    float total = 0.f;
    for (int i = -1; i < repeats; i++) {  // (i = -1: the warm-up)
      if (stage == 1)
        HIPX(hipMemcpyAsync(d.ex, keep, (size_t)n * R * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
      HIPX(hipEventRecord(e0, nullptr));
      if (stage == 0)
        HIPX(launch_cox_eval_eta(x, f32, row_stride, col_stride, n, d.cols, m, d.B, d.zero, R, d.pos, d.eta, d.ex, nullptr));
      else if (stage == 1)
        HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, ties == 1 ? d.first : nullptr, n, R, d.work, d.res, nullptr));
      else
        HIPX(launch_cox_eval_pairs(d.eta, d.kg, d.first, n, R, d.cnt, nullptr));
      HIPX(hipEventRecord(e1, nullptr));
      HIPX(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) total += ms;
    }
    stage_ms[stage] = total / repeats;
    if (stage == 0) HIPX(hipMemcpy(keep, d.ex, (size_t)n * R * sizeof(double), hipMemcpyDeviceToDevice));
  }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// Breslow baseline hazard and survival curves on a caller's device matrix (include/bessx.h section 2f)
// ----------------------------------------------------------------------------------------------
static_assert((int)BESSX_SURV_SURVIVAL == 0 && (int)BESSX_SURV_CUMHAZ == 1, "kind codes of launch_cox_surv_curves");

namespace {

const double kCoxZero = 0.0;  // Cox has no intercept: the coef0 of predict_upload_model

// the tie groups that hold an event: their times (ascending) and last positions
void cox_event_groups(const CoxOrder &o, const double *time, int n, std::vector<double> *times, std::vector<int> *ends) {
  std::vector<double> tpos((size_t)n);
  for (int i = 0; i < n; i++) tpos[(size_t)o.pos[(size_t)i]] = time[i];
  times->clear();
  ends->clear();
  bool event = false;
  for (int k = 0; k < n; k++) {
    event = event || o.kg[(size_t)k] != INT_MAX;
    if (k == n - 1 || o.first[(size_t)k + 1] != o.first[(size_t)k]) {  // (position k ends its group)
      if (event) {
        times->push_back(tpos[(size_t)k]);
        ends->push_back(k);
      }
      event = false;
    }
  }
}

int cox_baseline_run(Owner &sc, const CoxOrder &o, const std::vector<int> &ends, std::vector<double> &hh,
                     const bessx_cox_baseline_input *in, double *cumhaz, hipStream_t st) {
  const int n = in->n, J = (int)ends.size(), f32 = in->x_dtype == BESSX_F32;
  CoxDev d;
  if (int rc = cox_eval_stage(sc, o, in->cols, in->m, in->B, 1, n, 1, 0, st, &d)) return rc;
  int *ends_d = nullptr;
  double *scr = nullptr, *hout = nullptr;
  HIPX(sc.alloc(&ends_d, (size_t)J));
  HIPX(sc.alloc(&hout, (size_t)J));
  HIPX(sc.alloc(&scr, (size_t)cox_surv_workspace(n)));
  HIPX(hipMemcpyAsync(ends_d, ends.data(), (size_t)J * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(launch_cox_eval_eta(in->x, f32, in->x_row_stride, in->x_col_stride, n, d.cols, in->m, d.B, d.zero, 1, d.pos, d.eta,
                           d.ex, st));
  HIPX(launch_cox_eval_suffix(d.ex, n, 1, d.work, st));
  // (eta has served: its n doubles hold h, then H)
  HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, ends_d, J, d.eta, scr, hout, st));
  hh.resize((size_t)J);
  HIPX(hipMemcpyAsync(hh.data(), hout, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  std::copy(hh.begin(), hh.end(), cumhaz);
  return 0;
}

int cox_survival_run(Owner &sc, std::vector<double> &tmp, const bessx_cox_survival_input *in, double *out,
                     hipStream_t st) {
  const int n = in->n, T = in->T, f32 = in->x_dtype == BESSX_F32;
  int *cols_d = nullptr;
  double *B_d = nullptr, *zero_d = nullptr, *ex = nullptr, *hg_d = nullptr, *stage = nullptr;
  if (int rc = predict_upload_model(sc, in->cols, in->m, in->B, &kCoxZero, 1, st, &cols_d, &B_d, &zero_d)) return rc;
  HIPX(sc.alloc(&ex, (size_t)n));
  HIPX(sc.alloc(&hg_d, (size_t)T));
  HIPX(hipMemcpyAsync(hg_d, in->hg, (size_t)T * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(launch_cox_surv_ex(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, in->m, B_d, zero_d, ex, st));
  if (in->out_on_device) {
    HIPX(launch_cox_surv_curves(ex, hg_d, n, T, in->kind, out, in->out_row_stride, in->out_col_stride, st));
    HIPX(hipStreamSynchronize(st));
    return 0;
  }
  const size_t cnt = (size_t)n * (size_t)T;
  HIPX(sc.alloc(&stage, cnt));
  HIPX(launch_cox_surv_curves(ex, hg_d, n, T, in->kind, stage, T, 1, st));
  const long long ors = in->out_row_stride, ocs = in->out_col_stride;
  const bool dense = (T == 1 || ocs == 1) && (n == 1 || ors == T);
  double *h = out;
  if (!dense) {
    tmp.resize(cnt);
    h = tmp.data();
  }
  HIPX(hipMemcpyAsync(h, stage, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  if (!dense)
    for (long long i = 0; i < n; i++)
      for (long long j = 0; j < T; j++) out[i * ors + j * ocs] = h[i * T + j];
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_baseline_device(const bessx_cox_baseline_input *in, int *n_times, double *times, double *cumhaz) {
  const std::string w("cox_baseline_device");
  if (!in || !n_times || !times || !cumhaz) return fail(BESSX_ERR_ARG, w + ": null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_check("cox_baseline_device", c, false)) return rc;
  if (in->weight)
    for (int i = 0; i < in->n; i++)
      if (!(in->weight[i] >= 0.0)) return fail(BESSX_ERR_ARG, w + ": weight must be non-negative");
  int dev = -1;
  if (int rc = cox_check_device("cox_baseline_device", c, &dev)) return rc;
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  std::vector<double> gt;
  std::vector<int> ends;
  cox_event_groups(o, in->time, in->n, &gt, &ends);
  int rc = 0;
  if (!ends.empty())
    rc = dev_call(dev, c.stream, [&](DevCall &dc) { return cox_baseline_run(dc.sc, o, ends, dc.h, in, cumhaz, dc.st); });
  if (!rc) {
    *n_times = (int)ends.size();
    std::copy(gt.begin(), gt.end(), times);
  }
  return rc;
}

int bessx_cox_survival_device(const bessx_cox_survival_input *in, double *out) {
  const std::string w("cox_survival_device");
  if (!in || !out) return fail(BESSX_ERR_ARG, w + ": null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_check("cox_survival_device", c, false, false)) return rc;
  if (in->T < 1 || !in->hg) return fail(BESSX_ERR_ARG, w + ": hg needs T >= 1 values");
  for (int j = 0; j < in->T; j++)
    if (!(in->hg[j] >= 0.0)) return fail(BESSX_ERR_ARG, w + ": hg must be non-negative");
  if (in->kind != BESSX_SURV_SURVIVAL && in->kind != BESSX_SURV_CUMHAZ)
    return fail(BESSX_ERR_ARG, w + ": kind must be BESSX_SURV_SURVIVAL or BESSX_SURV_CUMHAZ");
  if (in->out_row_stride < 0 || in->out_col_stride < 0) return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  if ((in->n > 1 && in->out_row_stride == 0) || (in->T > 1 && in->out_col_stride == 0))
    return fail(BESSX_ERR_ARG, w + ": out: a zero stride along an axis longer than 1");
  int dev = -1;
  if (int rc = cox_check_device("cox_survival_device", c, &dev)) return rc;
  if (in->out_on_device)
    if (int rc = check_on_device("cox_survival_device", "out", out, BESSX_F64, in->out_row_stride, in->out_col_stride, in->n,
                                 in->T, dev))
      return rc;
  return dev_call(dev, c.stream, [&](DevCall &dc) { return cox_survival_run(dc.sc, dc.h, in, out, dc.st); });
}

int bessx_op_cox_surv_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int T, int kind, int out_col_major, int repeats, double *stage_ms) {
  if (repeats < 1 || !stage_ms || T < 1 || (kind != BESSX_SURV_SURVIVAL && kind != BESSX_SURV_CUMHAZ))
    return fail(BESSX_ERR_ARG, "op_cox_surv_bench: bad arguments");
  if (!x) return fail(BESSX_ERR_ARG, "op_cox_surv_bench: null argument");
  if (int rc = check_x_model("op_cox_surv_bench", x, dtype, row_stride >= 0 && col_stride >= 0, n, p, cols, m, &kCoxZero, 1,
                             BESSX_LINK_IDENTITY, false))
    return rc;  // (B is the library's own)
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_surv_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m), time((size_t)n), status((size_t)n), hg((size_t)T);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int i = 0; i < n; i++) {  // distinct times in an order that is not the rows'
    time[(size_t)i] = (double)(((long long)i * 7919) % n) + (double)i / (2.0 * n);
    status[(size_t)i] = (double)(i % 2);
  }
  for (int j = 0; j < T; j++) hg[(size_t)j] = (j + 1.0) / T;
  CoxOrder o;
  cox_order(time.data(), status.data(), nullptr, n, &o);
  std::vector<double> gt;
  std::vector<int> ends;
  cox_event_groups(o, time.data(), n, &gt, &ends);
  const int J = (int)ends.size();
  Owner sc;
  CoxDev d;
  if (int rc = cox_eval_stage(sc, o, cols, m, B.data(), 1, n, 1, 0, nullptr, &d)) return rc;
  int *ends_d = nullptr;
  double *scr = nullptr, *hout = nullptr, *ex = nullptr, *hg_d = nullptr, *out = nullptr;
  HIPX(sc.alloc(&ends_d, (size_t)J));
  HIPX(sc.alloc(&hout, (size_t)J));
  HIPX(sc.alloc(&scr, (size_t)cox_surv_workspace(n)));
  HIPX(sc.alloc(&ex, (size_t)n));
  HIPX(sc.alloc(&hg_d, (size_t)T));
  HIPX(sc.alloc(&out, (size_t)n * (size_t)T));
  HIPX(hipMemcpy(ends_d, ends.data(), (size_t)J * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(hg_d, hg.data(), (size_t)T * sizeof(double), hipMemcpyHostToDevice));
  const int f32 = dtype == BESSX_F32;
  // the baseline's own kernels start from S: one predictor pass and suffix scan outside the timed loops
  HIPX(launch_cox_eval_eta(x, f32, row_stride, col_stride, n, d.cols, m, d.B, d.zero, 1, d.pos, d.eta, d.ex, nullptr));
  HIPX(launch_cox_eval_suffix(d.ex, n, 1, d.work, nullptr));
  HIPX(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  const long long ors = out_col_major ? 1 : T, ocs = out_col_major ? n : 1;
  for (int stage = 0; stage < 3; stage++) {
    float total = 0.f;
    for (int i = -1; i < repeats; i++) {  // (i = -1: the warm-up)
      HIPX(hipEventRecord(e0, nullptr));
      if (stage == 0)
        HIPX(launch_cox_surv_ex(x, f32, row_stride, col_stride, n, d.cols, m, d.B, d.zero, ex, nullptr));
      else if (stage == 1)
        HIPX(launch_cox_surv_curves(ex, hg_d, n, T, kind, out, ors, ocs, nullptr));
      else
        HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, ends_d, J, d.eta, scr, hout, nullptr));
      HIPX(hipEventRecord(e1, nullptr));
      HIPX(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) total += ms;
    }
    stage_ms[stage] = total / repeats;
  }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// Restricted mean and quantile survival times on a caller's device matrix (include/bessx.h section 2u)
// ----------------------------------------------------------------------------------------------
namespace {

// the host side of the RMST part: the pieces of the used segments, and the columns sorted by the pieces in front of them
struct RmstPlan {
  int Kc = 0, NP = 0;  // segments below the largest cut; pieces
  std::vector<int> pstart, colq, colj;
};

void rmst_plan(const int *cut, int T, RmstPlan *pl) {
  pl->Kc = T > 0 ? *std::max_element(cut, cut + T) : 0;
  pl->pstart.assign((size_t)(pl->Kc / cox_rmst_slab() + T + 1), 0);
  std::vector<int> q((size_t)T);
  pl->NP = T > 0 ? cox_rmst_pieces(cut, T, pl->pstart.data(), q.data()) : 0;
  pl->colj.resize((size_t)T);
  std::iota(pl->colj.begin(), pl->colj.end(), 0);
  std::stable_sort(pl->colj.begin(), pl->colj.end(), [&](int a, int b) { return q[(size_t)a] < q[(size_t)b]; });
  pl->colq.resize((size_t)T);
  for (int s = 0; s < T; s++) pl->colq[(size_t)s] = q[(size_t)pl->colj[(size_t)s]];
}

// its device side: buffers of `sc`, uploads queued on st (the plan and hs / wd must outlive them)
struct RmstDev {
  double *hs = nullptr, *wd = nullptr, *part = nullptr;
  int *pstart = nullptr, *colq = nullptr, *colj = nullptr;
  long long rows = 0;  // rows per launch pair
};

int rmst_stage(Owner &sc, const RmstPlan &pl, const double *hs, const double *wd, int T, long long n, hipStream_t st,
               RmstDev *d) {
  const size_t Kc = (size_t)pl.Kc, NP = (size_t)pl.NP;
  d->rows = cox_rmst_chunk_rows(n, pl.NP);
  HIPX(sc.alloc(&d->hs, 2 * Kc));
  d->wd = d->hs + Kc;
  HIPX(sc.alloc(&d->pstart, NP + 1 + 2 * (size_t)T));
  d->colq = d->pstart + NP + 1;
  d->colj = d->colq + T;
  HIPX(sc.alloc(&d->part, NP * (size_t)d->rows));
  if (Kc > 0) {
    HIPX(hipMemcpyAsync(d->hs, hs, Kc * sizeof(double), hipMemcpyHostToDevice, st));
    HIPX(hipMemcpyAsync(d->wd, wd, Kc * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIPX(hipMemcpyAsync(d->pstart, pl.pstart.data(), (NP + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->colq, pl.colq.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->colj, pl.colj.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
  return 0;
}

// the launch pairs of every chunk of rows, in order on st (the partials of a chunk are read before the next overwrites
// them); only = 1 / 2: the partial / the finish kernels alone
int rmst_launch(const RmstPlan &pl, const RmstDev &d, const double *ex, long long n, int T, double *out, long long ors,
                long long ocs, hipStream_t st, int only = 0) {
  for (long long row0 = 0; row0 < n; row0 += d.rows) {
    const long long nr = std::min(d.rows, n - row0);
    if (pl.NP > 0 && only != 2) HIPX(launch_cox_rmst_partial(ex + row0, nr, d.hs, d.wd, d.pstart, pl.NP, d.part, st));
    if (only != 1)
      HIPX(launch_cox_rmst_finish(ex + row0, d.part, nr, pl.NP, d.colq, d.colj, T, out + row0 * ors, ors, ocs, st));
  }
  return 0;
}

// an n x T row-major staged result to the caller's host memory at its strides (tmp: the call's host vector)
int survtime_to_host(std::vector<double> &tmp, const double *stage, long long n, long long T, double *out, long long ors,
                     long long ocs, hipStream_t st) {
  const size_t cnt = (size_t)n * (size_t)T;
  const bool dense = (T == 1 || ocs == 1) && (n == 1 || ors == T);
  double *h = out;
  if (!dense) {
    tmp.resize(cnt);
    h = tmp.data();
  }
  HIPX(hipMemcpyAsync(h, stage, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  if (!dense)
    for (long long i = 0; i < n; i++)
      for (long long j = 0; j < T; j++) out[i * ors + j * ocs] = h[i * T + j];
  return 0;
}

int cox_survtime_run(DevCall &dc, const bessx_cox_survtime_input *in, const RmstPlan &pl, double *rmst, double *quant) {
  Owner &sc = dc.sc;
  hipStream_t st = dc.st;
  const int n = in->n, T = in->T, Q = in->Q, J = in->J, f32 = in->x_dtype == BESSX_F32;
  const bool dev_out = in->out_on_device != 0;
  int *cols_d = nullptr;
  double *B_d = nullptr, *zero_d = nullptr, *ex = nullptr, *rm = rmst, *qu = quant;
  if (int rc = predict_upload_model(sc, in->cols, in->m, in->B, &kCoxZero, 1, st, &cols_d, &B_d, &zero_d)) return rc;
  HIPX(sc.alloc(&ex, (size_t)n));
  HIPX(launch_cox_surv_ex(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, in->m, B_d, zero_d, ex, st));
  if (T > 0) {
    RmstDev d;
    if (int rc = rmst_stage(sc, pl, in->hs, in->wd, T, n, st, &d)) return rc;
    if (!dev_out) HIPX(sc.alloc(&rm, (size_t)n * (size_t)T));
    if (int rc = rmst_launch(pl, d, ex, n, T, rm, dev_out ? in->rmst_row_stride : T, dev_out ? in->rmst_col_stride : 1, st))
      return rc;
  }
  if (Q > 0) {
    double *hz_d = nullptr, *c_d = nullptr;
    HIPX(sc.alloc(&hz_d, 2 * (size_t)J));
    HIPX(sc.alloc(&c_d, (size_t)Q));
    if (J > 0) {
      HIPX(hipMemcpyAsync(hz_d, in->hz, (size_t)J * sizeof(double), hipMemcpyHostToDevice, st));
      HIPX(hipMemcpyAsync(hz_d + J, in->ut, (size_t)J * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPX(hipMemcpyAsync(c_d, in->c, (size_t)Q * sizeof(double), hipMemcpyHostToDevice, st));
    if (!dev_out) HIPX(sc.alloc(&qu, (size_t)n * (size_t)Q));
    HIPX(launch_cox_quantile(ex, n, J > 0 ? hz_d : nullptr, J > 0 ? hz_d + J : nullptr, J, c_d, Q, qu,
                             dev_out ? in->quant_row_stride : Q, dev_out ? in->quant_col_stride : 1, st));
  }
  if (dev_out) {
    HIPX(hipStreamSynchronize(st));
    return 0;
  }
  if (T > 0)
    if (int rc = survtime_to_host(dc.h, rm, n, T, rmst, in->rmst_row_stride, in->rmst_col_stride, st)) return rc;
  if (Q > 0)
    if (int rc = survtime_to_host(dc.h, qu, n, Q, quant, in->quant_row_stride, in->quant_col_stride, st)) return rc;
  return 0;
}

int survtime_check_strides(const std::string &w, const char *what, int n, int cols, long long rs, long long cs) {
  if (rs < 0 || cs < 0) return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  if ((n > 1 && rs == 0) || (cols > 1 && cs == 0))
    return fail(BESSX_ERR_ARG, w + ": " + what + ": a zero stride along an axis longer than 1");
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_survtime_device(const bessx_cox_survtime_input *in, double *rmst, double *quant) {
  const std::string w("cox_survtime_device");
  if (!in) return fail(BESSX_ERR_ARG, w + ": null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_check("cox_survtime_device", c, false, false)) return rc;
  const int T = in->T, Q = in->Q, K = in->K, J = in->J;
  if (T < 0 || Q < 0 || K < 0 || J < 0) return fail(BESSX_ERR_ARG, w + ": T, Q, K and J must be non-negative");
  if (T == 0 && Q == 0) return fail(BESSX_ERR_ARG, w + ": nothing to compute (T = 0 and Q = 0)");
  if ((T > 0) != (rmst != nullptr)) return fail(BESSX_ERR_ARG, w + ": rmst goes with T >= 1, and is NULL with T = 0");
  if ((Q > 0) != (quant != nullptr)) return fail(BESSX_ERR_ARG, w + ": quant goes with Q >= 1, and is NULL with Q = 0");
  if (T > 0) {
    if (!in->cut || (K > 0 && (!in->hs || !in->wd))) return fail(BESSX_ERR_ARG, w + ": null argument (hs, wd or cut)");
    for (int k = 0; k < K; k++) {
      if (!(in->hs[k] >= 0.0)) return fail(BESSX_ERR_ARG, w + ": hs must be non-negative");
      if (!(in->wd[k] > 0.0)) return fail(BESSX_ERR_ARG, w + ": wd must be positive");
    }
    for (int j = 0; j < T; j++)
      if (in->cut[j] < 0 || in->cut[j] > K) return fail(BESSX_ERR_ARG, w + ": cut must lie in [0, K]");
    if (int rc = survtime_check_strides(w, "rmst", in->n, T, in->rmst_row_stride, in->rmst_col_stride)) return rc;
  }
  if (Q > 0) {
    if (!in->c || (J > 0 && (!in->hz || !in->ut))) return fail(BESSX_ERR_ARG, w + ": null argument (hz, ut or c)");
    for (int g = 0; g < J; g++) {
      if (!(in->hz[g] >= 0.0)) return fail(BESSX_ERR_ARG, w + ": hz must be non-negative");
      if (g > 0 && in->hz[g] < in->hz[g - 1]) return fail(BESSX_ERR_ARG, w + ": hz must be non-decreasing");
      if (std::isnan(in->ut[g])) return fail(BESSX_ERR_ARG, w + ": ut holds a NaN");
    }
    for (int j = 0; j < Q; j++)
      if (!(in->c[j] > 0.0)) return fail(BESSX_ERR_ARG, w + ": c must be positive");
    if (int rc = survtime_check_strides(w, "quant", in->n, Q, in->quant_row_stride, in->quant_col_stride)) return rc;
  }
  int dev = -1;
  if (int rc = cox_check_device("cox_survtime_device", c, &dev)) return rc;
  if (in->out_on_device) {
    if (T > 0)
      if (int rc = check_on_device("cox_survtime_device", "rmst", rmst, BESSX_F64, in->rmst_row_stride,
                                   in->rmst_col_stride, in->n, T, dev))
        return rc;
    if (Q > 0)
      if (int rc = check_on_device("cox_survtime_device", "quant", quant, BESSX_F64, in->quant_row_stride,
                                   in->quant_col_stride, in->n, Q, dev))
        return rc;
  }
  RmstPlan pl;  // (declared before dev_call: the uploads of the call read it)
  rmst_plan(in->cut, T, &pl);
  return dev_call(dev, c.stream, [&](DevCall &dc) { return cox_survtime_run(dc, in, pl, rmst, quant); });
}

int bessx_cox_survtime_workspace(int n, const int *cut, int T, int *slab, int *pieces, long long *rows_per_chunk,
                                 long long *doubles) {
  const std::string w("cox_survtime_workspace");
  if (!slab || !pieces || !rows_per_chunk || !doubles || (T > 0 && !cut)) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (n < 1 || T < 0) return fail(BESSX_ERR_ARG, w + ": n must be at least 1 and T non-negative");
  for (int j = 0; j < T; j++)
    if (cut[j] < 0) return fail(BESSX_ERR_ARG, w + ": cut must be non-negative");
  RmstPlan pl;
  rmst_plan(cut, T, &pl);
  *slab = cox_rmst_slab();
  *pieces = pl.NP;
  *rows_per_chunk = T > 0 ? cox_rmst_chunk_rows(n, pl.NP) : 0;
  *doubles = n;
  if (T > 0) *doubles += 2LL * pl.Kc + (long long)pl.NP * *rows_per_chunk + (pl.NP + 1 + 2LL * T + 1) / 2;
  return BESSX_OK;
}

int bessx_op_cox_rmst_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int K, int T, int J, int Q, int repeats, double *stage_ms) {
  if (repeats < 1 || !stage_ms || K < 1 || T < 1 || J < 1 || Q < 1)
    return fail(BESSX_ERR_ARG, "op_cox_rmst_bench: bad arguments");
  if (!x) return fail(BESSX_ERR_ARG, "op_cox_rmst_bench: null argument");
  if (int rc = check_x_model("op_cox_rmst_bench", x, dtype, row_stride >= 0 && col_stride >= 0, n, p, cols, m, &kCoxZero, 1,
                             BESSX_LINK_IDENTITY, false))
    return rc;  // (B is the library's own)
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_rmst_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m), hs((size_t)K), wd((size_t)K), hzut(2 * (size_t)J), lev((size_t)Q);
  std::vector<int> cut((size_t)T);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int k = 0; k < K; k++) {  // a cumulative hazard that reaches 3 over a span of 1
    hs[(size_t)k] = 3.0 * k / K;
    wd[(size_t)k] = 1.0 / K;
  }
  for (int j = 0; j < T; j++) cut[(size_t)j] = (int)((long long)K * (j + 1) / T);
  for (int g = 0; g < J; g++) {
    hzut[(size_t)g] = 3.0 * (g + 1) / J;
    hzut[(size_t)J + g] = g + 1.0;
  }
  for (int j = 0; j < Q; j++) lev[(size_t)j] = -std::log1p(-(j + 1.0) / (Q + 1.0));
  RmstPlan pl;
  rmst_plan(cut.data(), T, &pl);
  Owner sc;
  int *cols_d = nullptr;
  double *B_d = nullptr, *zero_d = nullptr, *ex = nullptr, *hz_d = nullptr, *c_d = nullptr, *rm = nullptr, *qu = nullptr;
  if (int rc = predict_upload_model(sc, cols, m, B.data(), &kCoxZero, 1, nullptr, &cols_d, &B_d, &zero_d)) return rc;
  RmstDev d;
  if (int rc = rmst_stage(sc, pl, hs.data(), wd.data(), T, n, nullptr, &d)) return rc;
  HIPX(sc.alloc(&ex, (size_t)n));
  HIPX(sc.alloc(&hz_d, 2 * (size_t)J));
  HIPX(sc.alloc(&c_d, (size_t)Q));
  HIPX(sc.alloc(&rm, (size_t)n * (size_t)T));
  HIPX(sc.alloc(&qu, (size_t)n * (size_t)Q));
  HIPX(hipMemcpy(hz_d, hzut.data(), 2 * (size_t)J * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(c_d, lev.data(), (size_t)Q * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  const int f32 = dtype == BESSX_F32;
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  for (int stage = 0; stage < 4; stage++) {
    float total = 0.f;
    for (int i = -1; i < repeats; i++) {  // (i = -1: the warm-up)
      HIPX(hipEventRecord(e0, nullptr));
      if (stage == 0) {
        HIPX(launch_cox_surv_ex(x, f32, row_stride, col_stride, n, cols_d, m, B_d, zero_d, ex, nullptr));
      } else if (stage == 3) {
        HIPX(launch_cox_quantile(ex, n, hz_d, hz_d + J, J, c_d, Q, qu, Q, 1, nullptr));
      } else if (int rc = rmst_launch(pl, d, ex, n, T, rm, T, 1, nullptr, stage)) {
        return rc;
      }
      HIPX(hipEventRecord(e1, nullptr));
      HIPX(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) total += ms;
    }
    stage_ms[stage] = total / repeats;
  }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// IPCW Brier score of R Cox models at T times on a caller's device matrix (include/bessx.h section 2p)
// ----------------------------------------------------------------------------------------------
namespace {

// the device side of one problem: buffers of `sc`, uploads queued on st (the host arrays must outlive them)
struct BrierDev {
  int *cols = nullptr;
  double *B = nullptr, *zero = nullptr, *ex = nullptr, *time = nullptr, *w = nullptr, *wa = nullptr, *hg = nullptr,
         *tg = nullptr, *b = nullptr, *part = nullptr, *bs = nullptr;
};

// w, wa: n host values each (w = ones without weights, wa = w * row_a)
int cox_brier_stage(Owner &sc, const int *cols, int m, const double *B, int R, int n, int T, const double *time,
                    const double *w, const double *wa, const double *hg, const double *tg, const double *b, hipStream_t st,
                    BrierDev *d) {
  const size_t N = (size_t)n, RT = (size_t)R * (size_t)T;
  long long rows, slabs;
  cox_brier_split(n, &rows, &slabs);
  HIPX(sc.alloc(&d->B, (size_t)m * R + (size_t)R));
  HIPX(sc.alloc(&d->cols, (size_t)m));
  d->zero = d->B + (size_t)m * R;
  HIPX(hipMemsetAsync(d->zero, 0, (size_t)R * sizeof(double), st));
  if (m > 0) {
    HIPX(hipMemcpyAsync(d->cols, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(hipMemcpyAsync(d->B, B, (size_t)m * R * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIPX(sc.alloc(&d->time, 3 * N));  // time, w, wa
  d->w = d->time + N;
  d->wa = d->w + N;
  HIPX(hipMemcpyAsync(d->time, time, N * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->w, w, N * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->wa, wa, N * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(sc.alloc(&d->hg, 2 * RT + 2 * (size_t)T));  // hg, the result, t, b
  d->bs = d->hg + RT;
  d->tg = d->bs + RT;
  d->b = d->tg + T;
  HIPX(hipMemcpyAsync(d->hg, hg, RT * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->tg, tg, (size_t)T * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->b, b, (size_t)T * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(sc.alloc(&d->ex, N * (size_t)R));
  HIPX(sc.alloc(&d->part, (size_t)slabs * RT));
  return 0;
}

int cox_brier_run(Owner &sc, std::vector<double> &h, const std::vector<double> &w, const std::vector<double> &wa, double W,
                  const bessx_cox_brier_input *in, double *bs, hipStream_t st) {
  const int n = in->n, T = in->T, R = in->R, f32 = in->x_dtype == BESSX_F32;
  BrierDev d;
  if (int rc = cox_brier_stage(sc, in->cols, in->m, in->B, R, n, T, in->time, w.data(), wa.data(), in->hg, in->times,
                               in->time_b, st, &d))
    return rc;
  HIPX(launch_cox_brier_ex(in->x, f32, in->x_row_stride, in->x_col_stride, n, d.cols, in->m, d.B, d.zero, R, d.ex, st));
  HIPX(launch_cox_brier(d.ex, d.time, d.w, d.wa, d.hg, d.tg, d.b, n, T, R, W, d.part, d.bs, 0, st));
  h.resize((size_t)R * (size_t)T);
  HIPX(hipMemcpyAsync(h.data(), d.bs, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  std::copy(h.begin(), h.end(), bs);
  return 0;
}

int cox_brier_check_sizes(const std::string &w, int R, int T) {
  if (R > 65535) return fail(BESSX_ERR_ARG, w + ": R must be at most 65535");
  if (T < 1) return fail(BESSX_ERR_ARG, w + ": T must be at least 1");
  if (T > COX_BRIER_T_MAX) return fail(BESSX_ERR_ARG, w + ": T must be at most " + std::to_string(COX_BRIER_T_MAX));
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_brier_workspace(int n, int T, int R, long long *doubles, long long *rows_per_slab, long long *slabs,
                              int *row_groups) {
  const std::string w("cox_brier_workspace");
  if (!doubles || !rows_per_slab || !slabs || !row_groups) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (n < 1 || R < 1) return fail(BESSX_ERR_ARG, w + ": n and R must be at least 1");
  if (int rc = cox_brier_check_sizes(w, R, T)) return rc;
  *doubles = cox_brier_workspace(n, T, R);
  cox_brier_split(n, rows_per_slab, slabs);
  *row_groups = cox_brier_row_groups(T);
  return BESSX_OK;
}

int bessx_cox_brier_device(const bessx_cox_brier_input *in, double *bs, double *sum_w) {
  const std::string w("cox_brier_device");
  if (!in || !bs || !sum_w) return fail(BESSX_ERR_ARG, w + ": null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_check("cox_brier_device", c, false, false)) return rc;
  if (int rc = cox_brier_check_sizes(w, in->R, in->T)) return rc;
  if (!in->hg || !in->times || !in->time || !in->row_a || !in->time_b) return fail(BESSX_ERR_ARG, w + ": null argument");
  const int n = in->n, T = in->T;
  for (int j = 0; j < T; j++) {
    if (std::isnan(in->times[j])) return fail(BESSX_ERR_ARG, w + ": times holds a NaN");
    if (!(in->time_b[j] >= 0.0) || !std::isfinite(in->time_b[j]))
      return fail(BESSX_ERR_ARG, w + ": time_b must be non-negative and finite");
  }
  for (size_t q = 0; q < (size_t)in->R * (size_t)T; q++)
    if (!(in->hg[q] >= 0.0)) return fail(BESSX_ERR_ARG, w + ": hg must be non-negative");
  std::vector<double> wv((size_t)n), wa((size_t)n);
  double W = 0.0;
  for (int i = 0; i < n; i++) {
    if (std::isnan(in->time[i])) return fail(BESSX_ERR_ARG, w + ": time holds a NaN");
    if (!(in->row_a[i] >= 0.0) || !std::isfinite(in->row_a[i]))
      return fail(BESSX_ERR_ARG, w + ": row_a must be non-negative and finite");
    const double wi = in->weight ? in->weight[i] : 1.0;
    if (!(wi >= 0.0)) return fail(BESSX_ERR_ARG, w + ": weight must be non-negative");
    wv[(size_t)i] = wi;
    wa[(size_t)i] = wi * in->row_a[i];
    W += wi;
  }
  if (!(W > 0.0) || !std::isfinite(W)) return fail(BESSX_ERR_ARG, w + ": the weights must have a positive, finite sum");
  int dev = -1;
  if (int rc = cox_check_device("cox_brier_device", c, &dev)) return rc;
  const int rc = dev_call(dev, c.stream, [&](DevCall &dc) { return cox_brier_run(dc.sc, dc.h, wv, wa, W, in, bs, dc.st); });
  if (!rc) *sum_w = W;
  return rc;
}

int bessx_op_cox_brier_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                             const int *cols, int m, int R, int T, int repeats, double *stage_ms) {
  const std::string w("op_cox_brier_bench");
  if (repeats < 1 || !stage_ms) return fail(BESSX_ERR_ARG, w + ": bad arguments");
  if (!x) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = predict_check_model("op_cox_brier_bench", n, p, cols, m, R, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = cox_brier_check_sizes(w, R, T)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_brier_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m * R), time((size_t)n), wv((size_t)n, 1.0), wa((size_t)n), hg((size_t)R * T), tg((size_t)T),
      b((size_t)T);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int i = 0; i < n; i++) {  // distinct times in an order that is not the rows'
    time[(size_t)i] = (double)(((long long)i * 7919) % n) + (double)i / (2.0 * n);
    wa[(size_t)i] = (double)(i % 2);
  }
  for (int j = 0; j < T; j++) {
    tg[(size_t)j] = (j + 0.5) * (double)n / T;
    b[(size_t)j] = 1.0 + (double)j / T;
    for (int r = 0; r < R; r++) hg[(size_t)r * T + j] = (j + 1.0) / T * (1.0 + (double)r / R);
  }
  Owner sc;
  BrierDev d;
  if (int rc = cox_brier_stage(sc, cols, m, B.data(), R, n, T, time.data(), wv.data(), wa.data(), hg.data(), tg.data(),
                               b.data(), nullptr, &d))
    return rc;
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  for (int stage = 0; stage < 3; stage++) {
    float ms = 0.f;
    if (int rc = bt.run(repeats, &ms, [&]() -> int {
          if (stage == 0)
            HIPX(launch_cox_brier_ex(x, f32, row_stride, col_stride, n, d.cols, m, d.B, d.zero, R, d.ex, nullptr));
          else
            HIPX(launch_cox_brier(d.ex, d.time, d.w, d.wa, d.hg, d.tg, d.b, n, T, R, (double)n, d.part, d.bs, stage, nullptr));
          return 0;
        }))
      return rc;
    stage_ms[stage] = ms / repeats;
  }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// weighted pair counts on a caller's device matrix: AUC(t) and Uno's C of R Cox models (include/bessx.h section 2q), the
// ROC AUC of R logistic models (section 2r)
// ----------------------------------------------------------------------------------------------
namespace {

// the host side: the order of the rows, the tiles between the cuts, the weights in position order, and the sums that
// need no pair (all fp64, in position order)
struct PairPlan {
  std::vector<int> pos, first, kg, tstart, tseg, tnext, last, from;
  std::vector<double> cw, lw, cw2, cases, controls;
  double comparable = 0.0, pairs = 0.0;  // pairs: (k, l) the AUC mode compares, per model
  int NT = 0, S = 1;
};

// times: T non-decreasing values; row_a, weight: null = status, ones; tau: NaN = no truncation
void pair_plan(const double *time, const double *status, const double *row_a, const double *weight, int n,
               const double *times, int T, double tau, PairPlan *o) {
  const size_t N = (size_t)n;
  std::vector<int> idx(N);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [time](int a, int b) { return time[a] < time[b]; });
  o->pos.resize(N);
  o->first.resize(N);
  o->kg.resize(N);
  o->cw.resize(N);
  o->lw.resize(N);
  o->cw2.resize(N);
  std::vector<double> ts(N);
  for (int k = 0; k < n; k++) {
    const int i = idx[(size_t)k];
    const double w = weight ? weight[i] : 1.0, a = row_a ? row_a[i] : status[i];
    const bool ev = status[i] != 0.0;
    ts[(size_t)k] = time[i];
    o->pos[(size_t)i] = k;
    o->first[(size_t)k] = (k > 0 && ts[(size_t)k - 1] == time[i]) ? o->first[(size_t)k - 1] : k;
    o->kg[(size_t)k] = ev ? o->first[(size_t)k] : INT_MAX;
    o->cw[(size_t)k] = w * a;
    o->lw[(size_t)k] = w;
    o->cw2[(size_t)k] = (ev && !(time[i] >= tau)) ? (w * a) * a : 0.0;
  }
  // the segments: bnd[J] = rows with time <= times[J - 1]
  const int S = T + 1;
  std::vector<int> bnd((size_t)S + 1);
  bnd[0] = 0;
  for (int j = 0; j < T; j++) bnd[(size_t)j + 1] = (int)(std::upper_bound(ts.begin(), ts.end(), times[j]) - ts.begin());
  bnd[(size_t)S] = n;
  o->S = S;
  o->tstart.clear();
  o->tseg.clear();
  o->last.assign((size_t)S, -1);
  o->from.assign((size_t)S, 0);
  for (int s = 0; s < S; s++) {
    for (int p = bnd[(size_t)s]; p < bnd[(size_t)s + 1]; p += PAIRAUC_TILE) {
      o->tstart.push_back(p);
      o->tseg.push_back(s);
    }
    if (s < T) {  // entry j = s of k_pa_cut: the tiles of the segments <= j against the segments from j + 1 on
      o->last[(size_t)s] = (int)o->tseg.size() - 1;
      o->from[(size_t)s] = s + 1;
    }
  }
  o->NT = (int)o->tseg.size();
  o->tstart.push_back(n);
  o->last[(size_t)T] = o->NT - 1;  // entry T: everything (Uno's C)
  o->tnext.resize((size_t)o->NT);
  for (int t = o->NT - 1, nx = o->NT; t >= 0; t--) {
    if (t < o->NT - 1 && o->tseg[(size_t)t + 1] != o->tseg[(size_t)t]) nx = t + 1;
    o->tnext[(size_t)t] = nx;
  }
  // the sums without a pair
  std::vector<double> pc(N + 1), sl(N + 1);
  pc[0] = 0.0;
  for (size_t k = 0; k < N; k++) pc[k + 1] = pc[k] + o->cw[k];
  sl[N] = 0.0;
  for (size_t k = N; k-- > 0;) sl[k] = sl[k + 1] + o->lw[k];
  o->cases.resize((size_t)T);
  o->controls.resize((size_t)T);
  for (int j = 0; j < T; j++) {
    o->cases[(size_t)j] = pc[(size_t)bnd[(size_t)j + 1]];
    o->controls[(size_t)j] = sl[(size_t)bnd[(size_t)j + 1]];
  }
  o->comparable = 0.0;
  for (int k = n - 1, end = n; k >= 0; k--) {  // end: first position with a later time than position k
    if (k < n - 1 && o->first[(size_t)k + 1] != o->first[(size_t)k]) end = k + 1;
    o->comparable += o->cw2[(size_t)k] * sl[(size_t)end];
  }
  o->pairs = 0.0;
  for (int t = 0; t < o->NT; t++)
    o->pairs += (double)(o->tstart[(size_t)t + 1] - o->tstart[(size_t)t]) *
                (double)(n - (o->tnext[(size_t)t] < o->NT ? o->tstart[(size_t)o->tnext[(size_t)t]] : n));
}

// the device side of one problem: buffers of `sc`, uploads queued on st (the vectors of the plan must outlive them)
struct PairDev {
  int *cols = nullptr, *pos = nullptr, *first = nullptr, *kg = nullptr, *tstart = nullptr, *tseg = nullptr,
      *tnext = nullptr, *last = nullptr, *from = nullptr;
  double *B = nullptr, *zero = nullptr, *cw = nullptr, *lw = nullptr, *cw2 = nullptr, *eta = nullptr, *part = nullptr,
         *og = nullptr, *oe = nullptr;
};

template <class V>
int pair_upload(Owner &sc, V **dst, const std::vector<V> &src, hipStream_t st) {
  HIPX(sc.alloc(dst, src.size()));
  HIPX(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice, st));
  return 0;
}

int pairauc_stage(Owner &sc, const PairPlan &o, const int *cols, int m, const double *B, int R, int n, int uno,
                  hipStream_t st, PairDev *d) {
  HIPX(sc.alloc(&d->B, (size_t)m * R + (size_t)R));
  HIPX(sc.alloc(&d->cols, (size_t)m));
  d->zero = d->B + (size_t)m * R;
  HIPX(hipMemsetAsync(d->zero, 0, (size_t)R * sizeof(double), st));
  if (m > 0) {
    HIPX(hipMemcpyAsync(d->cols, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(hipMemcpyAsync(d->B, B, (size_t)m * R * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (int rc = pair_upload(sc, &d->pos, o.pos, st)) return rc;
  if (int rc = pair_upload(sc, &d->tstart, o.tstart, st)) return rc;
  if (int rc = pair_upload(sc, &d->tseg, o.tseg, st)) return rc;
  if (int rc = pair_upload(sc, &d->tnext, o.tnext, st)) return rc;
  if (int rc = pair_upload(sc, &d->last, o.last, st)) return rc;
  if (int rc = pair_upload(sc, &d->from, o.from, st)) return rc;
  if (int rc = pair_upload(sc, &d->cw, o.cw, st)) return rc;
  if (int rc = pair_upload(sc, &d->lw, o.lw, st)) return rc;
  if (uno) {
    if (int rc = pair_upload(sc, &d->first, o.first, st)) return rc;
    if (int rc = pair_upload(sc, &d->kg, o.kg, st)) return rc;
    if (int rc = pair_upload(sc, &d->cw2, o.cw2, st)) return rc;
  }
  HIPX(sc.alloc(&d->eta, (size_t)n * R));
  HIPX(sc.alloc(&d->part, 2 * (size_t)R * (size_t)o.NT * (size_t)o.S));
  HIPX(sc.alloc(&d->og, 2 * (size_t)o.S * R));
  d->oe = d->og + (size_t)o.S * R;
  return 0;
}

// res: (T + 1) * R greater then (T + 1) * R equal, entry T of each = Uno's sums (when uno)
int pairauc_run(Owner &sc, std::vector<double> &h, const PairPlan &o, const bessx_cox_auc_input *in, hipStream_t st) {
  const int n = in->n, T = in->T, R = in->R, f32 = in->x_dtype == BESSX_F32, uno = in->want_uno != 0;
  PairDev d;
  if (int rc = pairauc_stage(sc, o, in->cols, in->m, in->B, R, n, uno, st, &d)) return rc;
  HIPX(launch_pairauc_eta(in->x, f32, in->x_row_stride, in->x_col_stride, n, d.cols, in->m, d.B, d.zero, R, d.pos, d.eta,
                          st));
  if (T > 0)
    HIPX(launch_pairauc(d.eta, d.cw, d.lw, nullptr, nullptr, d.tstart, d.tseg, d.tnext, n, o.NT, o.S, R, 0, d.last, d.from,
                        T, d.part, d.og, d.oe, 0, st));
  if (uno)  // (the partials are free again: the stream has finished with them)
    HIPX(launch_pairauc(d.eta, d.cw2, d.lw, d.kg, d.first, d.tstart, d.tseg, d.tnext, n, o.NT, o.S, R, 1, d.last + T,
                        d.from + T, 1, d.part, d.og + (size_t)T * R, d.oe + (size_t)T * R, 0, st));
  h.assign(2 * (size_t)o.S * R, 0.0);
  HIPX(hipMemcpyAsync(h.data(), d.og, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  return 0;
}

int pairauc_check_sizes(const std::string &w, int R, int T) {
  if (R > 65535) return fail(BESSX_ERR_ARG, w + ": R must be at most 65535");
  if (T < 0) return fail(BESSX_ERR_ARG, w + ": T must not be negative");
  if (T > PAIRAUC_T_MAX) return fail(BESSX_ERR_ARG, w + ": T must be at most " + std::to_string(PAIRAUC_T_MAX));
  return 0;
}

inline CoxCall cox_call(const bessx_cox_auc_input *in) {
  return CoxCall{in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,      in->p, in->cols, in->m,
                 in->B, in->R,       in->time,         in->status,       in->weight, 1,     static_cast<hipStream_t>(in->stream)};
}

// the checks and the call of sections 2q and 2r; res as pairauc_run leaves it
int pairauc_call(const char *who, const bessx_cox_auc_input *in, PairPlan *o, std::vector<double> *res) {
  const std::string w(who);
  const CoxCall c = cox_call(in);
  if (int rc = cox_check(who, c, false)) return rc;
  if (int rc = pairauc_check_sizes(w, in->R, in->T)) return rc;
  if (in->T > 0 && !in->times) return fail(BESSX_ERR_ARG, w + ": null argument");
  for (int j = 0; j < in->T; j++) {
    if (std::isnan(in->times[j])) return fail(BESSX_ERR_ARG, w + ": times holds a NaN");
    if (j > 0 && in->times[j] < in->times[j - 1]) return fail(BESSX_ERR_ARG, w + ": times must not decrease");
  }
  for (int i = 0; i < in->n; i++) {
    if (in->row_a && (!(in->row_a[i] >= 0.0) || !std::isfinite(in->row_a[i])))
      return fail(BESSX_ERR_ARG, w + ": row_a must be non-negative and finite");
    if (in->weight && (!(in->weight[i] >= 0.0) || !std::isfinite(in->weight[i])))
      return fail(BESSX_ERR_ARG, w + ": weight must be non-negative and finite");
  }
  int dev = -1;
  if (int rc = cox_check_device(who, c, &dev)) return rc;
  pair_plan(in->time, in->status, in->row_a, in->weight, in->n, in->times, in->T, in->tau, o);
  return dev_call(dev, c.stream, [&](DevCall &dc) {
    if (int rc = pairauc_run(dc.sc, dc.h, *o, in, dc.st)) return rc;
    *res = dc.h;
    return 0;
  });
}

}  // namespace

extern "C" {

int bessx_cox_auc_workspace(int n, int T, int R, long long *doubles, long long *tile_rows, long long *tiles_max) {
  const std::string w("cox_auc_workspace");
  if (!doubles || !tile_rows || !tiles_max) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (n < 1 || R < 1) return fail(BESSX_ERR_ARG, w + ": n and R must be at least 1");
  if (int rc = pairauc_check_sizes(w, R, T)) return rc;
  *doubles = pairauc_workspace(n, T, R);
  *tile_rows = PAIRAUC_TILE;
  *tiles_max = pairauc_tiles_max(n, T);
  return BESSX_OK;
}

int bessx_cox_auc_device(const bessx_cox_auc_input *in, double *greater, double *equal, double *cases, double *controls,
                         double *uno, double *uno_comparable) {
  const std::string w("cox_auc_device");
  if (!in) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (in->T > 0 && (!greater || !equal || !cases || !controls)) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (in->want_uno && (!uno || !uno_comparable)) return fail(BESSX_ERR_ARG, w + ": want_uno needs uno and uno_comparable");
  PairPlan o;
  std::vector<double> res;
  if (int rc = pairauc_call("cox_auc_device", in, &o, &res)) return rc;
  const size_t T = (size_t)in->T, R = (size_t)in->R, SR = (T + 1) * R;
  std::copy(res.begin(), res.begin() + (long long)(T * R), greater);
  std::copy(res.begin() + (long long)SR, res.begin() + (long long)(SR + T * R), equal);
  std::copy(o.cases.begin(), o.cases.end(), cases);
  std::copy(o.controls.begin(), o.controls.end(), controls);
  if (in->want_uno) {
    for (size_t r = 0; r < R; r++) {
      uno[3 * r] = res[T * R + r];
      uno[3 * r + 1] = res[SR + T * R + r];
      uno[3 * r + 2] = o.comparable;
    }
    *uno_comparable = o.comparable;
  }
  return BESSX_OK;
}

int bessx_auc_device(const bessx_auc_input *in, double *greater, double *equal, double *pos_weight, double *neg_weight) {
  const std::string w("auc_device");
  if (!in || !greater || !equal || !pos_weight || !neg_weight) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (in->n < 1 || in->p < 1) return fail(BESSX_ERR_ARG, w + ": empty matrix");
  if (!in->y) return fail(BESSX_ERR_ARG, w + ": null argument");
  // the classes as times: a case leaves at 0, a control at 1, and the one cut lies at 0
  std::vector<double> cls((size_t)in->n), ones((size_t)in->n, 1.0);
  for (int i = 0; i < in->n; i++) {
    if (std::isnan(in->y[i])) return fail(BESSX_ERR_ARG, w + ": y holds a NaN");
    cls[(size_t)i] = in->y[i] > 0.5 ? 0.0 : 1.0;
  }
  const double cut = 0.0;
  const bessx_cox_auc_input c{in->x,      in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,      in->p,
                              in->cols,   in->m,       in->B,            in->R,            &cut,       1,
                              cls.data(), ones.data(), nullptr,          in->weight,       std::nan(""), 0,
                              in->stream};
  PairPlan o;
  std::vector<double> res;
  if (int rc = pairauc_call("auc_device", &c, &o, &res)) return rc;
  const size_t R = (size_t)in->R;
  std::copy(res.begin(), res.begin() + (long long)R, greater);
  std::copy(res.begin() + 2 * (long long)R, res.begin() + 3 * (long long)R, equal);
  *pos_weight = o.cases[0];
  *neg_weight = o.controls[0];
  return BESSX_OK;
}

int bessx_op_pairauc_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                           const int *cols, int m, int R, int T, int repeats, double *stage_ms, double *pairs) {
  const std::string w("op_pairauc_bench");
  if (repeats < 1 || !stage_ms || !pairs) return fail(BESSX_ERR_ARG, w + ": bad arguments");
  if (!x) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = predict_check_model("op_pairauc_bench", n, p, cols, m, R, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = pairauc_check_sizes(w, R, T)) return rc;
  if (T < 1) return fail(BESSX_ERR_ARG, w + ": T must be at least 1");
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_pairauc_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m * R), time((size_t)n), status((size_t)n), tg((size_t)T);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int i = 0; i < n; i++) {  // distinct times in an order that is not the rows'
    time[(size_t)i] = (double)(((long long)i * 7919) % n) + (double)i / (2.0 * n);
    status[(size_t)i] = (double)(i % 2);
  }
  for (int j = 0; j < T; j++) tg[(size_t)j] = (j + 0.5) * (double)n / T;
  PairPlan o;
  pair_plan(time.data(), status.data(), nullptr, nullptr, n, tg.data(), T, std::nan(""), &o);
  Owner sc;
  PairDev d;
  if (int rc = pairauc_stage(sc, o, cols, m, B.data(), R, n, 1, nullptr, &d)) return rc;
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  for (int stage = 0; stage < 4; stage++) {
    float ms = 0.f;
    if (int rc = bt.run(repeats, &ms, [&]() -> int {
          if (stage == 0)
            HIPX(launch_pairauc_eta(x, f32, row_stride, col_stride, n, d.cols, m, d.B, d.zero, R, d.pos, d.eta, nullptr));
          else if (stage < 3)
            HIPX(launch_pairauc(d.eta, d.cw, d.lw, nullptr, nullptr, d.tstart, d.tseg, d.tnext, n, o.NT, o.S, R, 0, d.last,
                                d.from, T, d.part, d.og, d.oe, stage, nullptr));
          else
            HIPX(launch_pairauc(d.eta, d.cw2, d.lw, d.kg, d.first, d.tstart, d.tseg, d.tnext, n, o.NT, o.S, R, 1,
                                d.last + T, d.from + T, 1, d.part, d.og + (size_t)T * R, d.oe + (size_t)T * R, 1, nullptr));
          return 0;
        }))
      return rc;
    stage_ms[stage] = ms / repeats;
  }
  *pairs = o.pairs * R;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// expected information and score of one model on a caller's device matrix (include/bessx.h section 2g)
// ----------------------------------------------------------------------------------------------
namespace {

// everything about a call that returns info and score which needs no device
int info_check_args(const char *who, const GlmCall &c, const double *info, long long info_ld, const double *score,
                    const double *loss, const double *sum_w) {
  const std::string w(who);
  if (!loss || !sum_w || !info || !score) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = glm_check(who, c, true)) return rc;
  if (info_ld < (long long)c.m + 1) return fail(BESSX_ERR_ARG, w + ": info_ld must be at least m + 1");
  return check_m_max(w, c.m);
}

int info_run(Owner &sc, std::vector<double> &h, const GlmCall &c, const bessx_info_input *in, double *loss, double *sum_w,
             hipStream_t st) {
  const int f32 = c.f32(), m = c.m;
  const size_t M = (size_t)m + 1;
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *work = nullptr, *res = nullptr, *stage = nullptr;
  if (int rc = predict_upload_model(sc, c.cols, m, c.beta, c.coef0, 1, st, &cols_d, &B_d, &c_d)) return rc;
  EvalData d;
  if (int rc = eval_stage_data(sc, c, st, &d)) return rc;
  HIPX(sc.alloc(&work, (size_t)info_workspace(f32, c.rs, c.cs, c.n, m, c.link, d.w != nullptr)));
  HIPX(sc.alloc(&res, 3));
  double *info_d = in->info, *score_d = in->score;
  long long ld = in->info_ld;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&stage, M * M + M));
    info_d = stage;
    score_d = stage + M * M;
    ld = (long long)M;
  }
  HIPX(launch_info(c.x, f32, c.rs, c.cs, c.n, cols_d, m, B_d, c_d, c.link, d, work, res, info_d, ld, score_d, st));
  h.resize(3 + (in->out_on_device ? 0 : M * M + M));
  HIPX(hipMemcpyAsync(h.data(), res, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (!in->out_on_device)
    HIPX(hipMemcpyAsync(h.data() + 3, stage, (M * M + M) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  *loss = h[0];
  *sum_w = d.w ? h[2] : (double)c.n;
  if (!in->out_on_device) {
    copy_out(h.data() + 3, M, M, in->info, in->info_ld);
    copy_out(h.data() + 3 + M * M, M, 1, in->score, 0);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_info_workspace(int x_dtype, long long x_row_stride, long long x_col_stride, int n, int m, int link,
                         int weighted, long long *doubles, long long *rows_per_slab, int *slabs) {
  if (!doubles || !rows_per_slab || !slabs) return fail(BESSX_ERR_ARG, "info_workspace: null argument");
  if (x_dtype != BESSX_F64 && x_dtype != BESSX_F32)
    return fail(BESSX_ERR_ARG, "info_workspace: x: dtype must be BESSX_F64 or BESSX_F32");
  if (x_row_stride < 0 || x_col_stride < 0) return fail(BESSX_ERR_ARG, "info_workspace: strides must be non-negative");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "info_workspace: empty matrix");
  if (link != BESSX_LINK_IDENTITY && link != BESSX_LINK_LOGISTIC && link != BESSX_LINK_POISSON)
    return fail(BESSX_ERR_ARG, "info_workspace: unknown link");
  if (int rc = check_m_max("info_workspace", m)) return rc;
  *doubles = info_workspace(x_dtype == BESSX_F32, x_row_stride, x_col_stride, n, m, link, weighted != 0);
  info_split(n, m, rows_per_slab, slabs);
  return BESSX_OK;
}

int bessx_info_device(const bessx_info_input *in, double *loss, double *sum_w) {
  if (!in) return fail(BESSX_ERR_ARG, "info_device: null argument");
  const GlmCall c = glm_call(in);
  if (int rc = info_check_args("info_device", c, in->info, in->info_ld, in->score, loss, sum_w)) return rc;
  int dev = -1;
  if (int rc = glm_check_device("info_device", c, &dev)) return rc;
  if (in->out_on_device) {
    const int M = in->m + 1;
    if (int rc = check_on_device("info_device", "info", in->info, BESSX_F64, in->info_ld, 1, M, M, dev)) return rc;
    if (int rc = check_on_device("info_device", "score", in->score, BESSX_F64, 1, 0, M, 1, dev)) return rc;
  }
  return dev_call(dev, c.stream, [&](DevCall &dc) { return info_run(dc.sc, dc.h, c, in, loss, sum_w, dc.st); });
}

int bessx_op_info_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                        const int *cols, int m, int repeats, double *avg_ms, double *tflops) {
  if (!x || repeats < 1 || !avg_ms || !tflops) return fail(BESSX_ERR_ARG, "op_info_bench: bad arguments");
  if (int rc = predict_check_model("op_info_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_info_bench", m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_info_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t M = (size_t)m + 1;
  std::vector<double> v((size_t)n, 0.25), g((size_t)n);
  for (size_t i = 0; i < g.size(); i++) g[i] = (i % 2) ? -0.5 : 0.5;
  int *cols_d = nullptr;
  double *v_d = nullptr, *g_d = nullptr, *part = nullptr, *out = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&v_d, v.size()));
  HIPX(sc.alloc(&g_d, g.size()));
  HIPX(sc.alloc(&part, (size_t)info_gram_workspace(n, m)));
  HIPX(sc.alloc(&out, M * M + M));
  if (m > 0) HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(v_d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(g_d, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  float ms = 0.f;
  if (int rc = bt.run(repeats, &ms, [&]() -> int {
        HIPX(launch_info_gram(x, f32, row_stride, col_stride, n, cols_d, m, v_d, g_d, part, out, (long long)M, out + M * M,
                              nullptr));
        return 0;
      }))
    return rc;
  *avg_ms = ms / repeats;
  *tflops = 2.0 * (double)n * (double)M * (double)(M + 1) * repeats / ((double)ms * 1e-3) / 1e12;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// per-row diagnostics of one model on a caller's device matrix (include/bessx.h section 2i)
// ----------------------------------------------------------------------------------------------
namespace {

constexpr unsigned kDiagAll = 0x7f;
constexpr unsigned kDiagLev = BESSX_DIAG_LEVERAGE | BESSX_DIAG_STD_PEARSON | BESSX_DIAG_STD_DEVIANCE | BESSX_DIAG_COOKS;
constexpr unsigned kDiagPhi = BESSX_DIAG_STD_PEARSON | BESSX_DIAG_STD_DEVIANCE | BESSX_DIAG_COOKS;

// which n-vectors of workspace a set of kinds needs: v, the Pearson and the deviance residual when they are needed
// but not requested
void diag_needs(unsigned kinds, bool *v, bool *pear, bool *dev) {
  *v = (kinds & kDiagLev) != 0;
  *pear = (kinds & (BESSX_DIAG_STD_PEARSON | BESSX_DIAG_COOKS)) && !(kinds & BESSX_DIAG_PEARSON);
  *dev = (kinds & BESSX_DIAG_STD_DEVIANCE) && !(kinds & BESSX_DIAG_DEVIANCE);
}

int diag_count(unsigned kinds) {
  int K = 0;
  for (unsigned b = 1; b <= kDiagAll; b <<= 1) K += (kinds & b) != 0;
  return K;
}

// everything about the call that needs no device
int diag_check_args(const char *who, const GlmCall &c, const bessx_diag_input *in) {
  const std::string w(who);
  if (!in->out) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = glm_check(who, c, true)) return rc;
  if (in->kinds == 0 || (in->kinds & ~kDiagAll)) return fail(BESSX_ERR_ARG, w + ": kinds must be a non-empty set of BESSX_DIAG_* bits");
  if (in->out_ld < (long long)in->n) return fail(BESSX_ERR_ARG, w + ": out_ld must be at least n");
  if (int rc = check_m_max(w, in->m)) return rc;
  if ((in->kinds & kDiagPhi) && !(std::isfinite(in->dispersion) && in->dispersion > 0.0))
    return fail(BESSX_ERR_ARG, w + ": dispersion must be finite and positive");
  if (in->kinds & kDiagLev) {
    if (!in->factor) return fail(BESSX_ERR_ARG, w + ": a kind that needs the leverage needs the factor");
    if (in->factor_ld < (long long)in->m + 1) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m + 1");
    for (long long j = 0; j <= in->m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  return 0;
}

long long diag_doubles(long long n, int m, unsigned kinds) {
  bool v, pear, dev;
  diag_needs(kinds, &v, &pear, &dev);
  const long long nv = (n + 1) / 2 * 2;
  return nv * ((int)v + (int)pear + (int)dev) + (v ? diag_factor_doubles(m) : 0);
}

int diag_run(Owner &sc, std::vector<double> &pk, std::vector<double> &h, const GlmCall &c, const bessx_diag_input *in,
             hipStream_t st) {
  const int f32 = in->x_dtype == BESSX_F32, m = in->m, K = diag_count(in->kinds);
  const long long n = in->n, nv = (n + 1) / 2 * 2;
  const unsigned kinds = in->kinds;
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *work = nullptr, *stage = nullptr;
  if (int rc = predict_upload_model(sc, in->cols, m, in->beta, &in->coef0, 1, st, &cols_d, &B_d, &c_d)) return rc;
  EvalData d;
  if (int rc = eval_stage_data(sc, c, st, &d)) return rc;
  bool need_v, tmp_pear, tmp_dev;
  diag_needs(kinds, &need_v, &tmp_pear, &tmp_dev);
  HIPX(sc.alloc(&work, (size_t)diag_doubles(n, m, kinds)));
  double *out_d = in->out;
  long long ld = in->out_ld;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&stage, (size_t)K * (size_t)n));
    out_d = stage;
    ld = n;
  }
  double *slot[7];
  int s = 0;
  for (int b = 0; b < 7; b++) slot[b] = (kinds & (1u << b)) ? out_d + (long long)(s++) * ld : nullptr;
  double *wp = work;
  double *v_d = nullptr, *pear_d = slot[2], *dev_d = slot[3];
  if (need_v) v_d = wp, wp += nv;
  if (tmp_pear) pear_d = wp, wp += nv;
  if (tmp_dev) dev_d = wp, wp += nv;
  HIPX(launch_diag_eta(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, B_d, c_d, in->link, d, v_d, slot[1],
                       pear_d, dev_d, st));
  if (need_v) {
    pk.resize((size_t)diag_factor_doubles(m));
    diag_pack_factor(in->factor, in->factor_ld, m, pk.data());
    HIPX(hipMemcpyAsync(wp, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPX(launch_diag_lev(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, wp, v_d, pear_d, dev_d,
                         in->dispersion, slot[0], slot[4], slot[5], slot[6], st));
  }
  if (!in->out_on_device) {
    h.resize((size_t)K * (size_t)n);
    HIPX(hipMemcpyAsync(h.data(), stage, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) copy_out(h.data(), (size_t)n, (size_t)K, in->out, in->out_ld);
  return 0;
}

}  // namespace

extern "C" {

int bessx_diag_workspace(int n, int m, unsigned kinds, long long *doubles) {
  if (!doubles) return fail(BESSX_ERR_ARG, "diag_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "diag_workspace: empty matrix");
  if (kinds == 0 || (kinds & ~kDiagAll))
    return fail(BESSX_ERR_ARG, "diag_workspace: kinds must be a non-empty set of BESSX_DIAG_* bits");
  if (int rc = check_m_max("diag_workspace", m)) return rc;
  *doubles = diag_doubles(n, m, kinds);
  return BESSX_OK;
}

int bessx_diag_device(const bessx_diag_input *in) {
  if (!in) return fail(BESSX_ERR_ARG, "diag_device: null argument");
  const GlmCall c = glm_call(in);
  if (int rc = diag_check_args("diag_device", c, in)) return rc;
  int dev = -1;
  if (int rc = glm_check_device("diag_device", c, &dev)) return rc;
  if (in->out_on_device)
    if (int rc = check_on_device("diag_device", "out", in->out, BESSX_F64, in->out_ld, 1, diag_count(in->kinds), in->n, dev))
      return rc;
  return dev_call(dev, c.stream, [&](DevCall &dc) { return diag_run(dc.sc, dc.pk, dc.h, c, in, dc.st); });
}

int bessx_op_diag_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                        const int *cols, int m, int repeats, double *avg_ms, double *tflops, double *bytes) {
  if (!x || repeats < 1 || !avg_ms || !tflops || !bytes) return fail(BESSX_ERR_ARG, "op_diag_bench: bad arguments");
  if (int rc = predict_check_model("op_diag_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_diag_bench", m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_diag_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t M = (size_t)m + 1;
  // a factor of the library's own: the scaled identity plus a small lower triangle
  std::vector<double> R(M * M, 0.0), pk((size_t)diag_factor_doubles(m)), v((size_t)n, 0.25), r((size_t)n);
  for (size_t j = 0; j < M; j++)
    for (size_t k = 0; k <= j; k++) R[j * M + k] = (j == k ? 1.0 : 1.0 / 64.0) / std::sqrt((double)n);
  diag_pack_factor(R.data(), (long long)M, m, pk.data());
  for (size_t i = 0; i < r.size(); i++) r[i] = (i % 2) ? -0.5 : 0.5;
  int *cols_d = nullptr;
  double *pk_d = nullptr, *v_d = nullptr, *r_d = nullptr, *out = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&pk_d, pk.size()));
  HIPX(sc.alloc(&v_d, v.size()));
  HIPX(sc.alloc(&r_d, r.size()));
  HIPX(sc.alloc(&out, 4 * (size_t)n));
  if (m > 0) HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(pk_d, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(v_d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(r_d, r.data(), r.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  const size_t N = (size_t)n;
  float ms = 0.f;
  if (int rc = bt.run(repeats, &ms, [&]() -> int {
        HIPX(launch_diag_lev(x, f32, row_stride, col_stride, n, cols_d, m, pk_d, v_d, r_d, r_d, 1.0, out, out + N,
                             out + 2 * N, out + 3 * N, nullptr));
        return 0;
      }))
    return rc;
  const double Mpad = 16.0 * (double)((M + 15) / 16);
  *avg_ms = ms / repeats;
  *tflops = (double)n * Mpad * Mpad * repeats / ((double)ms * 1e-3) / 1e12;
  *bytes = (double)n * (double)m * (f32 ? 4.0 : 8.0) + 7.0 * 8.0 * (double)n + 8.0 * (double)pk.size();
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// observed information and score of one Cox model on a caller's device matrix (include/bessx.h section 2h)
// ----------------------------------------------------------------------------------------------
namespace {

// what the kernels of bessx_k_coxinfo.hip need about the order on top of CoxOrder
struct CoxInfoOrder {
  std::vector<int> rowof, lastk, jptr, iota;  // row at a position; last position of a tie group; events per r(k); 0 .. m-1
  std::vector<double> wdJ;                    // wd of the J event rows, in position order
  int J = 0;
  double n_events = 0.0;
};

// o->first becomes r(k): it stays first(k) for ties = 1 and becomes the identity for ties = 0
void cox_info_order(CoxOrder *o, int n, int m, int ties, CoxInfoOrder *x) {
  const size_t N = (size_t)n;
  x->rowof.resize(N);
  for (int i = 0; i < n; i++) x->rowof[(size_t)o->pos[(size_t)i]] = i;
  if (ties) {
    x->lastk.resize(N);
    for (int k = n - 1, end = n - 1; k >= 0; k--) {
      if (k < n - 1 && o->first[(size_t)k + 1] != o->first[(size_t)k]) end = k;
      x->lastk[(size_t)k] = end;
    }
  } else {
    std::iota(o->first.begin(), o->first.end(), 0);
  }
  x->jptr.assign(N + 1, 0);
  x->wdJ.clear();
  x->n_events = 0.0;
  for (int k = 0; k < n; k++) {
    x->n_events += o->wd[(size_t)k];
    if (o->kg[(size_t)k] != INT_MAX) {
      x->wdJ.push_back(o->wd[(size_t)k]);
      x->jptr[(size_t)o->first[(size_t)k] + 1]++;
    }
  }
  for (int k = 0; k < n; k++) x->jptr[(size_t)k + 1] += x->jptr[(size_t)k];
  x->J = (int)x->wdJ.size();
  x->iota.resize((size_t)m);
  std::iota(x->iota.begin(), x->iota.end(), 0);
}

// doubles of device scratch of one call (the arrays of CoxInfoDev that hold doubles)
long long cox_info_doubles(long long n, int m, long long J) {
  const long long nb = (n + 1023) / 1024, M = (long long)m + 1;
  long long d = 2 * n + cox_eval_workspace(n, 1) + 2 + (long long)m + 1;  // eta / H, e -> S0, the scans' totals, res, B
  if (m == 0) return d;
  d += 3 * n + (long long)m * n + nb * m + cox_surv_workspace(n);  // e, v, g, W and the totals of its scan and of H's
  d += info_gram_workspace(n, m) + 2 * (M * M + M);                 // the sweeps' partials and results
  if (J > 0) d += cox_info_ldu(J) * m + J + info_gram_workspace(J, m);
  return d;
}

struct CoxInfoDev {
  CoxDev d;  // (d.first holds r(k); d.eta holds H once the likelihood has been formed)
  int *rowof = nullptr, *lastk = nullptr, *jptr = nullptr, *iota = nullptr;
  double *e = nullptr, *W = nullptr, *scr = nullptr, *hs = nullptr, *v = nullptr, *g = nullptr, *wdJ = nullptr;
  double *U = nullptr, *part1 = nullptr, *part2 = nullptr, *G = nullptr, *res = nullptr;
  long long ldU = 0;
  int J = 0;
};

// buffers of `sc`, uploads queued on st (the vectors of o and x must outlive them)
int cox_info_stage(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const int *cols, int m, const double *beta, int n,
                   int ties, hipStream_t st, CoxInfoDev *c) {
  const size_t N = (size_t)n, M = (size_t)m + 1;
  if (int rc = cox_eval_stage(sc, o, cols, m, beta, 1, n, 1, 0, st, &c->d)) return rc;
  HIPX(sc.alloc(&c->res, 2));
  c->J = x.J;
  if (m == 0) return 0;
  HIPX(sc.alloc(&c->rowof, N));
  HIPX(hipMemcpyAsync(c->rowof, x.rowof.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
  if (ties) {
    HIPX(sc.alloc(&c->lastk, N));
    HIPX(hipMemcpyAsync(c->lastk, x.lastk.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
  }
  HIPX(sc.alloc(&c->e, N));
  HIPX(sc.alloc(&c->v, N));
  HIPX(sc.alloc(&c->g, N));
  HIPX(sc.alloc(&c->W, (size_t)m * N));
  HIPX(sc.alloc(&c->scr, (size_t)((n + 1023) / 1024) * (size_t)m));
  HIPX(sc.alloc(&c->hs, (size_t)cox_surv_workspace(n)));
  HIPX(sc.alloc(&c->part1, (size_t)info_gram_workspace(n, m)));
  HIPX(sc.alloc(&c->G, 2 * (M * M + M)));
  if (x.J > 0) {
    const size_t J = (size_t)x.J;
    c->ldU = cox_info_ldu(x.J);
    HIPX(sc.alloc(&c->jptr, N + 1));
    HIPX(hipMemcpyAsync(c->jptr, x.jptr.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&c->iota, (size_t)m));
    HIPX(hipMemcpyAsync(c->iota, x.iota.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&c->wdJ, J));
    HIPX(hipMemcpyAsync(c->wdJ, x.wdJ.data(), J * sizeof(double), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&c->U, (size_t)c->ldU * (size_t)m));
    HIPX(sc.alloc(&c->part2, (size_t)info_gram_workspace(x.J, m)));
  }
  return 0;
}

// the launches of one call in order; stage >= 0 (the bench): only the gather (0) or the risk-set means (1), which need
// the buffers as a full sequence has left them -- e and S0 are not overwritten by anything after the likelihood
int cox_info_launch(const void *x, int f32, long long rs, long long cs, int n, int m, int ties, const CoxInfoDev &c,
                    double *info, long long ld, double *score, hipStream_t st, int stage = -1) {
  const CoxDev &d = c.d;
  const size_t M = (size_t)m + 1;
  double *G1 = c.G, *U1 = c.G + M * M, *G2 = U1 + M, *U2 = G2 + M * M;
  if (stage < 0) {
    HIPX(launch_cox_eval_eta(x, f32, rs, cs, n, d.cols, m, d.B, d.zero, 1, d.pos, d.eta, d.ex, st));
    if (m > 0) HIPX(hipMemcpyAsync(c.e, d.ex, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, ties ? d.first : nullptr, n, 1, d.work, c.res, st));
    if (m == 0) return 0;
  }
  if (stage < 0 || stage == 0) HIPX(launch_cox_info_gather(x, f32, rs, cs, n, d.cols, m, c.rowof, c.e, c.W, st));
  if (stage < 0) {
    // (eta has served: its n doubles hold h, then H)
    HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, nullptr, 0, d.eta, c.hs, nullptr, st));
    HIPX(launch_cox_info_vg(c.e, d.eta, ties ? c.lastk : nullptr, d.wd, d.pos, n, c.v, c.g, st));
    HIPX(launch_info_gram(x, f32, rs, cs, n, d.cols, m, c.v, c.g, c.part1, G1, (long long)M, U1, st));
  }
  if (c.J > 0 && (stage < 0 || stage == 1))
    HIPX(launch_cox_info_means(c.W, d.ex, c.jptr, n, m, c.J, c.scr, c.U, c.ldU, st));
  if (stage < 0) {
    if (c.J > 0)
      HIPX(launch_info_gram(c.U, 0, 1, c.ldU, c.J, c.iota, m, c.wdJ, c.wdJ, c.part2, G2, (long long)M, U2, st));
    HIPX(launch_cox_info_finish(G1, c.J > 0 ? G2 : nullptr, U1, m, info, ld, score, c.res, st));
  }
  return 0;
}

// everything about a call that returns info and score which needs no device (*events: rows with status 1)
int cox_info_check_args(const char *who, const CoxCall &c, const double *info, long long info_ld, const double *score,
                        const double *loglik, const double *n_events, const double *residual_sum, int *events = nullptr) {
  const std::string w(who);
  if (!loglik || !n_events || !residual_sum) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = cox_check(who, c, true, true, events)) return rc;
  if (c.m > 0 && (!info || !score)) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (info_ld < (long long)c.m) return fail(BESSX_ERR_ARG, w + ": info_ld must be at least m");
  return check_m_max(w, c.m);
}

int cox_info_run(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, std::vector<double> &h,
                 const bessx_cox_info_input *in, double *loglik, double *residual_sum, hipStream_t st) {
  const int n = in->n, m = in->m, f32 = in->x_dtype == BESSX_F32;
  const size_t mm = (size_t)m * (size_t)m;
  CoxInfoDev c;
  if (int rc = cox_info_stage(sc, o, x, in->cols, m, in->beta, n, in->ties, st, &c)) return rc;
  HIPX(hipMemsetAsync(c.res, 0, 2 * sizeof(double), st));
  double *info_d = in->info, *score_d = in->score, *stage = nullptr;
  long long ld = in->info_ld;
  const bool staged = m > 0 && !in->out_on_device;
  if (staged) {
    HIPX(sc.alloc(&stage, mm + (size_t)m));
    info_d = stage;
    score_d = stage + mm;
    ld = m;
  }
  if (int rc = cox_info_launch(in->x, f32, in->x_row_stride, in->x_col_stride, n, m, in->ties, c, info_d, ld, score_d, st))
    return rc;
  h.resize(2 + (staged ? mm + (size_t)m : 0));
  HIPX(hipMemcpyAsync(h.data(), c.res, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (staged) HIPX(hipMemcpyAsync(h.data() + 2, stage, (mm + (size_t)m) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  *loglik = h[0];
  *residual_sum = h[1];
  if (staged) {
    copy_out(h.data() + 2, (size_t)m, (size_t)m, in->info, in->info_ld);
    copy_out(h.data() + 2 + mm, (size_t)m, 1, in->score, 0);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_info_workspace(int n, int m, int n_event_rows, long long *doubles, long long *rows_per_slab, int *slabs) {
  if (!doubles || !rows_per_slab || !slabs) return fail(BESSX_ERR_ARG, "cox_info_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "cox_info_workspace: empty matrix");
  if (n_event_rows < 0 || n_event_rows > n)
    return fail(BESSX_ERR_ARG, "cox_info_workspace: n_event_rows must lie in [0, n]");
  if (int rc = check_m_max("cox_info_workspace", m)) return rc;
  *doubles = cox_info_doubles(n, m, n_event_rows);
  rows_per_slab[0] = rows_per_slab[1] = 0;
  slabs[0] = slabs[1] = 0;
  if (m > 0) {
    info_split(n, m, &rows_per_slab[0], &slabs[0]);
    if (n_event_rows > 0) info_split(n_event_rows, m, &rows_per_slab[1], &slabs[1]);
  }
  return BESSX_OK;
}

int bessx_cox_info_device(const bessx_cox_info_input *in, double *loglik, double *n_events, double *residual_sum) {
  if (!in) return fail(BESSX_ERR_ARG, "cox_info_device: null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_info_check_args("cox_info_device", c, in->info, in->info_ld, in->score, loglik, n_events, residual_sum))
    return rc;
  int dev = -1;
  if (int rc = cox_check_device("cox_info_device", c, &dev)) return rc;
  if (in->out_on_device && in->m > 0) {
    if (int rc = check_on_device("cox_info_device", "info", in->info, BESSX_F64, in->info_ld, 1, in->m, in->m, dev)) return rc;
    if (int rc = check_on_device("cox_info_device", "score", in->score, BESSX_F64, 1, 0, in->m, 1, dev)) return rc;
  }
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  CoxInfoOrder x;
  cox_info_order(&o, in->n, in->m, in->ties, &x);
  const int rc = dev_call(dev, c.stream,
                          [&](DevCall &dc) { return cox_info_run(dc.sc, o, x, dc.h, in, loglik, residual_sum, dc.st); });
  if (!rc) *n_events = x.n_events;
  return rc;
}

int bessx_op_cox_info_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int ties, int repeats, double *stage_ms, double *bytes) {
  if (!x || repeats < 1 || !stage_ms || !bytes || m < 1) return fail(BESSX_ERR_ARG, "op_cox_info_bench: bad arguments");
  if (int rc = predict_check_model("op_cox_info_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (ties != 0 && ties != 1) return fail(BESSX_ERR_ARG, "op_cox_info_bench: ties must be 0 (order) or 1 (breslow)");
  if (int rc = check_m_max("op_cox_info_bench", m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_info_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m), time((size_t)n), status((size_t)n);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int i = 0; i < n; i++) {  // times in an order that is not the rows'; ties = 1: groups of four equal times
    const long long s = ((long long)i * 7919) % n;
    time[(size_t)i] = ties ? (double)(s / 4) : (double)s + (double)i / (2.0 * n);
    status[(size_t)i] = (double)(i % 2);
  }
  CoxOrder o;
  cox_order(time.data(), status.data(), nullptr, n, &o);
  CoxInfoOrder xo;
  cox_info_order(&o, n, m, ties, &xo);
  Owner sc;
  CoxInfoDev c;
  if (int rc = cox_info_stage(sc, o, xo, cols, m, B.data(), n, ties, nullptr, &c)) return rc;
  double *out = nullptr;
  HIPX(sc.alloc(&out, (size_t)m * m + (size_t)m));
  HIPX(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  const int f32 = dtype == BESSX_F32;
  for (int stage = 2; stage >= 0; stage--) {  // (the full sequence first: stages 0 and 1 start from what it leaves)
    float total = 0.f;
    for (int i = -1; i < repeats; i++) {  // (i = -1: the warm-up)
      HIPX(hipEventRecord(e0, nullptr));
      if (int rc = cox_info_launch(x, f32, row_stride, col_stride, n, m, ties, c, out, m, out + (size_t)m * m, nullptr,
                                   stage == 2 ? -1 : stage))
        return rc;
      HIPX(hipEventRecord(e1, nullptr));
      HIPX(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) total += ms;
    }
    stage_ms[stage] = total / repeats;
  }
  const double item = f32 ? 4.0 : 8.0;
  *bytes = (double)n * m * (item + 8.0) + (double)n * m * 8.0 + (double)c.J * m * 8.0;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// the proportional-hazards test of one Cox model on a caller's device matrix (include/bessx.h section 2t)
// ----------------------------------------------------------------------------------------------
namespace {

// doubles of device scratch of one call: section 2h's buffers (its v, g, partials and results stay unused), then gp, the
// three H^q, v^q and a^q, the partials and results of the three-weight sweeps and the event weights
long long cox_zph_doubles(long long n, int m, long long J) {
  long long d = cox_info_doubles(n, m, J);
  if (m == 0) return d;
  const long long M = (long long)m + 1;
  d += n + 3 * n + 6 * n + cox_zph_gram_workspace(n, m) + 6 * (M * M + M) + 3 * (long long)m * m + 2 * m;
  if (J > 0) d += 3 * J + cox_zph_gram_workspace(J, m);
  return d;
}

// everything about the call that needs no device
int cox_zph_check_args(const char *who, const CoxCall &c, const bessx_cox_zph_input *in, const double *loglik,
                       const double *n_events) {
  const std::string w(who);
  if (!loglik || !n_events || !in->gt) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = cox_check(who, c, true, true)) return rc;
  if (c.m > 0 && (!in->info0 || !in->info1 || !in->info2 || !in->score0 || !in->score1))
    return fail(BESSX_ERR_ARG, w + ": null argument");
  if (in->info_ld < (long long)c.m) return fail(BESSX_ERR_ARG, w + ": info_ld must be at least m");
  for (int i = 0; i < c.n; i++)
    if (c.status[i] != 0.0 && !std::isfinite(in->gt[i]))
      return fail(BESSX_ERR_ARG, w + ": gt must be finite at every row with status 1");
  return check_m_max(w, c.m);
}

// gp: gt in position order with an exact 0 at the positions without an event; cJ: c^q_j = wd g^q of the J event rows in
// position order, q = 0, 1, 2, J values each -- the products the kernels form ((wd * g) * g)
void cox_zph_order(const CoxOrder &o, const CoxInfoOrder &x, const double *gt, int n, std::vector<double> *gp,
                   std::vector<double> *cJ) {
  const size_t J = (size_t)x.J;
  gp->assign((size_t)n, 0.0);
  cJ->resize(3 * J);
  size_t j = 0;
  for (int k = 0; k < n; k++)
    if (o.kg[(size_t)k] != INT_MAX) {
      const double g = gt[x.rowof[(size_t)k]], c0 = o.wd[(size_t)k], c1 = c0 * g;
      (*gp)[(size_t)k] = g;
      (*cJ)[j] = c0;
      (*cJ)[J + j] = c1;
      (*cJ)[2 * J + j] = c1 * g;
      j++;
    }
}

int cox_zph_run(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const std::vector<double> &gp,
                const std::vector<double> &cJ, std::vector<double> &h, const bessx_cox_zph_input *in, double *loglik,
                hipStream_t st) {
  const int n = in->n, m = in->m, f32 = in->x_dtype == BESSX_F32, ties = in->ties;
  const long long rs = in->x_row_stride, cs = in->x_col_stride;
  const size_t N = (size_t)n, M = (size_t)m + 1, mm = (size_t)m * (size_t)m, gs = M * M + M, nout = 3 * mm + 2 * (size_t)m;
  CoxInfoDev c;
  if (int rc = cox_info_stage(sc, o, x, in->cols, m, in->beta, n, ties, st, &c)) return rc;
  const CoxDev &d = c.d;
  HIPX(hipMemsetAsync(c.res, 0, 2 * sizeof(double), st));
  // the predictor, e, S0 and the likelihood: section 2h's launches (the same bits)
  HIPX(launch_cox_eval_eta(in->x, f32, rs, cs, n, d.cols, m, d.B, d.zero, 1, d.pos, d.eta, d.ex, st));
  if (m > 0) HIPX(hipMemcpyAsync(c.e, d.ex, N * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, ties ? d.first : nullptr, n, 1, d.work, c.res, st));
  const bool staged = m > 0 && !in->out_on_device;
  double *stage = nullptr;
  if (m > 0) {
    double *gp_d = nullptr, *H = nullptr, *va = nullptr, *part = nullptr, *G = nullptr;
    HIPX(sc.alloc(&gp_d, N));
    HIPX(hipMemcpyAsync(gp_d, gp.data(), N * sizeof(double), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&H, 3 * N));
    HIPX(sc.alloc(&va, 6 * N));
    HIPX(sc.alloc(&part, (size_t)cox_zph_gram_workspace(n, m)));
    HIPX(sc.alloc(&G, 6 * gs));
    double *v = va, *a = va + 3 * N, *G1 = G, *G2 = G + 3 * gs;
    HIPX(launch_cox_info_gather(in->x, f32, rs, cs, n, d.cols, m, c.rowof, c.e, c.W, st));
    HIPX(launch_cox_zph_hazard(d.wd, gp_d, d.ex, d.first, n, H, H + N, H + 2 * N, st));
    for (int q = 0; q < 3; q++) HIPX(launch_cox_prefix_scan(H + (size_t)q * N, n, c.hs, st));
    HIPX(launch_cox_zph_vg(c.e, H, n, ties ? c.lastk : nullptr, d.wd, gp_d, d.pos, n, v, a, n, st));
    HIPX(launch_cox_zph_gram(in->x, f32, rs, cs, n, d.cols, m, v, a, n, part, G1, (long long)gs, st));
    if (c.J > 0) {
      const size_t J = (size_t)c.J;
      double *cJ_d = nullptr, *part2 = nullptr;
      HIPX(sc.alloc(&cJ_d, 3 * J));
      HIPX(hipMemcpyAsync(cJ_d, cJ.data(), 3 * J * sizeof(double), hipMemcpyHostToDevice, st));
      HIPX(sc.alloc(&part2, (size_t)cox_zph_gram_workspace(c.J, m)));
      HIPX(launch_cox_info_means(c.W, d.ex, c.jptr, n, m, c.J, c.scr, c.U, c.ldU, st));
      HIPX(launch_cox_zph_gram(c.U, 0, 1, c.ldU, c.J, c.iota, m, cJ_d, cJ_d, c.J, part2, G2, (long long)gs, st));
    }
    double *i0 = in->info0, *i1 = in->info1, *i2 = in->info2, *s0 = in->score0, *s1 = in->score1;
    long long ld = in->info_ld;
    if (staged) {
      HIPX(sc.alloc(&stage, nout));
      i0 = stage, i1 = stage + mm, i2 = stage + 2 * mm, s0 = stage + 3 * mm, s1 = s0 + m;
      ld = m;
    }
    HIPX(launch_cox_zph_finish(G1, c.J > 0 ? G2 : nullptr, (long long)gs, m, i0, i1, i2, ld, s0, s1, st));
  }
  h.resize(1 + (staged ? nout : 0));
  HIPX(hipMemcpyAsync(h.data(), c.res, sizeof(double), hipMemcpyDeviceToHost, st));
  if (staged) HIPX(hipMemcpyAsync(h.data() + 1, stage, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  *loglik = h[0];
  if (staged) {
    const double *r = h.data() + 1;
    copy_out(r, (size_t)m, (size_t)m, in->info0, in->info_ld);
    copy_out(r + mm, (size_t)m, (size_t)m, in->info1, in->info_ld);
    copy_out(r + 2 * mm, (size_t)m, (size_t)m, in->info2, in->info_ld);
    copy_out(r + 3 * mm, (size_t)m, 1, in->score0, 0);
    copy_out(r + 3 * mm + (size_t)m, (size_t)m, 1, in->score1, 0);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_zph_workspace(int n, int m, int n_event_rows, long long *doubles, long long *rows_per_slab, int *slabs) {
  if (!doubles || !rows_per_slab || !slabs) return fail(BESSX_ERR_ARG, "cox_zph_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "cox_zph_workspace: empty matrix");
  if (n_event_rows < 0 || n_event_rows > n)
    return fail(BESSX_ERR_ARG, "cox_zph_workspace: n_event_rows must lie in [0, n]");
  if (int rc = check_m_max("cox_zph_workspace", m)) return rc;
  *doubles = cox_zph_doubles(n, m, n_event_rows);
  rows_per_slab[0] = rows_per_slab[1] = 0;
  slabs[0] = slabs[1] = 0;
  if (m > 0) {
    info_split(n, m, &rows_per_slab[0], &slabs[0]);
    if (n_event_rows > 0) info_split(n_event_rows, m, &rows_per_slab[1], &slabs[1]);
  }
  return BESSX_OK;
}

int bessx_cox_zph_device(const bessx_cox_zph_input *in, double *loglik, double *n_events) {
  if (!in) return fail(BESSX_ERR_ARG, "cox_zph_device: null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_zph_check_args("cox_zph_device", c, in, loglik, n_events)) return rc;
  int dev = -1;
  if (int rc = cox_check_device("cox_zph_device", c, &dev)) return rc;
  if (in->out_on_device && in->m > 0) {
    const char *names[3] = {"info0", "info1", "info2"};
    double *const infos[3] = {in->info0, in->info1, in->info2};
    for (int q = 0; q < 3; q++)
      if (int rc = check_on_device("cox_zph_device", names[q], infos[q], BESSX_F64, in->info_ld, 1, in->m, in->m, dev))
        return rc;
    if (int rc = check_on_device("cox_zph_device", "score0", in->score0, BESSX_F64, 1, 0, in->m, 1, dev)) return rc;
    if (int rc = check_on_device("cox_zph_device", "score1", in->score1, BESSX_F64, 1, 0, in->m, 1, dev)) return rc;
  }
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  CoxInfoOrder x;
  cox_info_order(&o, in->n, in->m, in->ties, &x);
  std::vector<double> gp, cJ;
  cox_zph_order(o, x, in->gt, in->n, &gp, &cJ);
  const int rc = dev_call(dev, c.stream,
                          [&](DevCall &dc) { return cox_zph_run(dc.sc, o, x, gp, cJ, dc.h, in, loglik, dc.st); });
  if (!rc) *n_events = x.n_events;
  return rc;
}

int bessx_op_cox_zph_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                           const int *cols, int m, int repeats, double *fused_ms, double *separate_ms) {
  if (!x || repeats < 1 || !fused_ms || !separate_ms || m < 1) return fail(BESSX_ERR_ARG, "op_cox_zph_bench: bad arguments");
  if (int rc = predict_check_model("op_cox_zph_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_cox_zph_bench", m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_zph_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t N = (size_t)n, M = (size_t)m + 1, gs = M * M + M;
  std::vector<double> v(3 * N), g(3 * N);
  for (size_t q = 0; q < 3; q++)
    for (size_t i = 0; i < N; i++) {
      v[q * N + i] = 0.25 * (double)(q + 1);
      g[q * N + i] = ((i + q) % 2) ? -0.5 : 0.5;
    }
  int *cols_d = nullptr;
  double *v_d = nullptr, *g_d = nullptr, *part = nullptr, *out = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&v_d, v.size()));
  HIPX(sc.alloc(&g_d, g.size()));
  HIPX(sc.alloc(&part, (size_t)cox_zph_gram_workspace(n, m)));
  HIPX(sc.alloc(&out, 3 * gs));
  HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(v_d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(g_d, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  const int f32 = dtype == BESSX_F32;
  for (int i = -1; i < repeats; i++)  // (i = -1: the warm-up of both routes)
    for (int route = 0; route < 2; route++) {
      HIPX(hipEventRecord(e0, nullptr));
      if (route == 0) {
        HIPX(launch_cox_zph_gram(x, f32, row_stride, col_stride, n, cols_d, m, v_d, g_d, n, part, out, (long long)gs,
                                 nullptr));
      } else {
        for (size_t q = 0; q < 3; q++)
          HIPX(launch_info_gram(x, f32, row_stride, col_stride, n, cols_d, m, v_d + q * N, g_d + q * N, part,
                                out + q * gs, (long long)M, out + q * gs + M * M, nullptr));
      }
      HIPX(hipEventRecord(e1, nullptr));
      HIPX(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) (route == 0 ? fused_ms : separate_ms)[i] = (double)ms;
    }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// residuals, dfbeta and case influence of one Cox model on a caller's device matrix (include/bessx.h section 2j)
// ----------------------------------------------------------------------------------------------
namespace {

constexpr unsigned kCoxDiagAll = 63u;
constexpr unsigned kCoxDiagRows = BESSX_COX_DIAG_MARTINGALE | BESSX_COX_DIAG_DEVIANCE | BESSX_COX_DIAG_DISPLACEMENT;
constexpr unsigned kCoxDiagL = BESSX_COX_DIAG_SCORE | BESSX_COX_DIAG_DFBETA | BESSX_COX_DIAG_DISPLACEMENT;
constexpr unsigned kCoxDiagU = kCoxDiagL | BESSX_COX_DIAG_SCHOENFELD;

int cox_diag_rows_count(unsigned kinds) {
  return (int)((kinds & BESSX_COX_DIAG_MARTINGALE) != 0) + (int)((kinds & BESSX_COX_DIAG_DEVIANCE) != 0) +
         (int)((kinds & BESSX_COX_DIAG_DISPLACEMENT) != 0);
}

// doubles of device scratch of one call
long long cox_diag_doubles(long long n, int m, long long J, unsigned kinds) {
  const long long nb = (n + 1023) / 1024;
  // eta / H, e -> S0, the scans' totals, res, B; e, v, g; the totals of H's scan
  long long d = 2 * n + cox_eval_workspace(n, 1) + 2 + (long long)m + 1 + 3 * n + cox_surv_workspace(n);
  if (m == 0) return d;
  if ((kinds & kCoxDiagU) && J > 0) d += (long long)m * n + nb * m + cox_info_ldu(J) * m;  // W, its totals, U
  if (kinds & kCoxDiagL) d += cox_diag_lda(n) * m + n + nb * m;                             // A / L, dh, A's totals
  if (kinds & BESSX_COX_DIAG_DFBETA) d += cox_diag_pack_doubles(m, 0);
  if (kinds & BESSX_COX_DIAG_DISPLACEMENT) d += cox_diag_pack_doubles(m, 1);
  return d;
}

// what the kernels of bessx_k_coxdiag.hip need about the order on top of CoxInfoOrder
struct CoxDiagOrder {
  std::vector<int> evj, evrow;  // event index of a position or -1; row of an event, in position order
};

void cox_diag_order(const CoxOrder &o, const CoxInfoOrder &x, int n, CoxDiagOrder *y) {
  y->evj.assign((size_t)n, -1);
  y->evrow.clear();
  for (int k = 0; k < n; k++)
    if (o.kg[(size_t)k] != INT_MAX) {
      y->evj[(size_t)k] = (int)y->evrow.size();
      y->evrow.push_back(x.rowof[(size_t)k]);
    }
}

// everything about the call that needs no device; *J = rows with status 1
int cox_diag_check_args(const char *who, const CoxCall &c, const bessx_cox_diag_input *in, const int *n_event_rows,
                        int *J) {
  const std::string w(who);
  if (!n_event_rows) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = cox_check(who, c, true, true, J)) return rc;
  const int ev = *J;
  const unsigned kinds = in->kinds;
  if (kinds == 0 || (kinds & ~kCoxDiagAll))
    return fail(BESSX_ERR_ARG, w + ": kinds must be a non-empty set of BESSX_COX_DIAG_* bits");
  if (int rc = check_m_max(w, in->m)) return rc;
  const long long n = in->n, m = in->m;
  if (kinds & kCoxDiagRows) {
    if (!in->out_rows) return fail(BESSX_ERR_ARG, w + ": a requested kind needs out_rows");
    if (in->out_rows_ld < n) return fail(BESSX_ERR_ARG, w + ": out_rows_ld must be at least n");
  }
  if ((kinds & BESSX_COX_DIAG_SCORE) && m > 0) {
    if (!in->out_score) return fail(BESSX_ERR_ARG, w + ": score needs out_score");
    if (in->out_score_ld < n) return fail(BESSX_ERR_ARG, w + ": out_score_ld must be at least n");
  }
  if ((kinds & BESSX_COX_DIAG_DFBETA) && m > 0) {
    if (!in->out_dfbeta) return fail(BESSX_ERR_ARG, w + ": dfbeta needs out_dfbeta");
    if (in->out_dfbeta_ld < n) return fail(BESSX_ERR_ARG, w + ": out_dfbeta_ld must be at least n");
    if (!in->cinv) return fail(BESSX_ERR_ARG, w + ": dfbeta needs cinv");
    if (in->cinv_ld < m) return fail(BESSX_ERR_ARG, w + ": cinv_ld must be at least m");
    for (long long j = 0; j < m; j++)
      for (long long k = 0; k < m; k++)
        if (!std::isfinite(in->cinv[j * in->cinv_ld + k])) return fail(BESSX_ERR_ARG, w + ": cinv must be finite");
  }
  if ((kinds & BESSX_COX_DIAG_DISPLACEMENT) && m > 0) {
    if (!in->factor) return fail(BESSX_ERR_ARG, w + ": displacement needs the factor");
    if (in->factor_ld < m) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m");
    for (long long j = 0; j < m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  if ((kinds & BESSX_COX_DIAG_SCHOENFELD) && m > 0 && ev > 0) {
    if (!in->out_schoenfeld) return fail(BESSX_ERR_ARG, w + ": schoenfeld needs out_schoenfeld");
    if (in->out_schoenfeld_ld < ev) return fail(BESSX_ERR_ARG, w + ": out_schoenfeld_ld must be at least n_event_rows");
  }
  return 0;
}

struct CoxDiagDev {
  CoxDev d;  // (d.first holds r(k); d.eta holds H once the likelihood has been formed; d.ex holds S0)
  int *rowof = nullptr, *lastk = nullptr, *jptr = nullptr, *evj = nullptr, *evrow = nullptr;
  double *e = nullptr, *v = nullptr, *g = nullptr, *hs = nullptr, *res = nullptr;
  double *W = nullptr, *scr = nullptr, *U = nullptr, *A = nullptr, *dh = nullptr, *scrA = nullptr;
  double *pkR = nullptr, *pkC = nullptr;
  long long ldU = 0, ldA = 0;
  int J = 0;
  bool needU = false, needL = false;
};

// buffers of `sc`, uploads queued on st (the vectors of o, x and y must outlive them)
int cox_diag_stage(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const CoxDiagOrder &y, const int *cols, int m,
                   const double *beta, int n, int ties, unsigned kinds, hipStream_t st, CoxDiagDev *c) {
  const size_t N = (size_t)n;
  if (int rc = cox_eval_stage(sc, o, cols, m, beta, 1, n, 1, 0, st, &c->d)) return rc;
  HIPX(sc.alloc(&c->res, 2));
  c->J = x.J;
  c->needU = m > 0 && x.J > 0 && (kinds & kCoxDiagU);
  c->needL = m > 0 && (kinds & kCoxDiagL);
  HIPX(sc.alloc(&c->e, N));
  HIPX(sc.alloc(&c->v, N));
  HIPX(sc.alloc(&c->g, N));
  HIPX(sc.alloc(&c->hs, (size_t)cox_surv_workspace(n)));
  if (ties) {
    HIPX(sc.alloc(&c->lastk, N));
    HIPX(hipMemcpyAsync(c->lastk, x.lastk.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (c->needU || c->needL) {
    HIPX(sc.alloc(&c->rowof, N));
    HIPX(hipMemcpyAsync(c->rowof, x.rowof.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&c->jptr, N + 1));
    HIPX(hipMemcpyAsync(c->jptr, x.jptr.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  }
  const size_t nb = (size_t)((n + 1023) / 1024);
  if (c->needU) {
    c->ldU = cox_info_ldu(x.J);
    HIPX(sc.alloc(&c->W, (size_t)m * N));
    HIPX(sc.alloc(&c->scr, nb * (size_t)m));
    HIPX(sc.alloc(&c->U, (size_t)c->ldU * (size_t)m));
    HIPX(sc.alloc(&c->evrow, (size_t)x.J));
    HIPX(hipMemcpyAsync(c->evrow, y.evrow.data(), (size_t)x.J * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (c->needL) {
    c->ldA = cox_diag_lda(n);
    HIPX(sc.alloc(&c->A, (size_t)c->ldA * (size_t)m));
    HIPX(sc.alloc(&c->dh, N));
    HIPX(sc.alloc(&c->scrA, nb * (size_t)m));
    HIPX(sc.alloc(&c->evj, N));
    HIPX(hipMemcpyAsync(c->evj, y.evj.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
    if (kinds & BESSX_COX_DIAG_DFBETA) HIPX(sc.alloc(&c->pkC, (size_t)cox_diag_pack_doubles(m, 0)));
    if (kinds & BESSX_COX_DIAG_DISPLACEMENT) HIPX(sc.alloc(&c->pkR, (size_t)cox_diag_pack_doubles(m, 1)));
  }
  return 0;
}

// section 2h's launches up to v and g (row order), W and U -- the same launchers with the same arguments
int cox_diag_launch_base(const void *x, int f32, long long rs, long long cs, int n, int m, int ties, const CoxDiagDev &c,
                         hipStream_t st) {
  const CoxDev &d = c.d;
  HIPX(launch_cox_eval_eta(x, f32, rs, cs, n, d.cols, m, d.B, d.zero, 1, d.pos, d.eta, d.ex, st));
  HIPX(hipMemcpyAsync(c.e, d.ex, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, ties ? d.first : nullptr, n, 1, d.work, c.res, st));
  if (c.needU) HIPX(launch_cox_info_gather(x, f32, rs, cs, n, d.cols, m, c.rowof, c.e, c.W, st));
  HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, nullptr, 0, d.eta, c.hs, nullptr, st));  // (eta's n doubles hold H)
  HIPX(launch_cox_info_vg(c.e, d.eta, ties ? c.lastk : nullptr, d.wd, d.pos, n, c.v, c.g, st));
  if (c.needU) HIPX(launch_cox_info_means(c.W, d.ex, c.jptr, n, m, c.J, c.scr, c.U, c.ldU, st));
  return 0;
}

// A, then L in place over it
int cox_diag_launch_L(const void *x, int f32, long long rs, long long cs, int n, int m, int ties, const CoxDiagDev &c,
                      hipStream_t st, bool form = true) {
  const CoxDev &d = c.d;
  HIPX(launch_cox_diag_accum(c.U, c.ldU, c.jptr, d.wd, d.ex, d.first, ties ? c.lastk : nullptr, n, m, c.dh, c.scrA, c.A,
                             c.ldA, st));
  if (form)
    HIPX(launch_cox_diag_form(x, f32, rs, cs, n, d.cols, m, c.rowof, c.g, d.wd, c.e, c.evj, c.U, c.ldU, c.A, c.ldA, st));
  return 0;
}

int cox_diag_run(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const CoxDiagOrder &y, std::vector<double> &pk,
                 std::vector<double> &h, const bessx_cox_diag_input *in, hipStream_t st) {
  const int n = in->n, m = in->m, f32 = in->x_dtype == BESSX_F32, J = x.J;
  const unsigned kinds = in->kinds;
  const size_t N = (size_t)n;
  const long long rs = in->x_row_stride, cs = in->x_col_stride;
  CoxDiagDev c;
  if (int rc = cox_diag_stage(sc, o, x, y, in->cols, m, in->beta, n, in->ties, kinds, st, &c)) return rc;
  HIPX(hipMemsetAsync(c.res, 0, 2 * sizeof(double), st));
  const int K = cox_diag_rows_count(kinds);
  const bool w_score = m > 0 && (kinds & BESSX_COX_DIAG_SCORE), w_dfb = m > 0 && (kinds & BESSX_COX_DIAG_DFBETA);
  const bool w_sch = m > 0 && J > 0 && (kinds & BESSX_COX_DIAG_SCHOENFELD);
  double *rows_d = in->out_rows, *score_d = in->out_score, *dfb_d = in->out_dfbeta, *sch_d = in->out_schoenfeld;
  long long rows_ld = in->out_rows_ld, score_ld = in->out_score_ld, dfb_ld = in->out_dfbeta_ld,
            sch_ld = in->out_schoenfeld_ld;
  const size_t s_rows = (size_t)K * N, s_mat = (size_t)m * N, s_sch = (size_t)m * (size_t)J;
  size_t o_score = 0, o_dfb = 0, o_sch = 0, total = 0;
  if (!in->out_on_device) {
    total = s_rows;
    o_score = total, total += w_score ? s_mat : 0;
    o_dfb = total, total += w_dfb ? s_mat : 0;
    o_sch = total, total += w_sch ? s_sch : 0;
    double *stage = nullptr;
    HIPX(sc.alloc(&stage, total > 0 ? total : 1));
    rows_d = stage, rows_ld = n;
    score_d = stage + o_score, score_ld = n;
    dfb_d = stage + o_dfb, dfb_ld = n;
    sch_d = stage + o_sch, sch_ld = J;
  }
  int s = 0;
  double *mart = (kinds & BESSX_COX_DIAG_MARTINGALE) ? rows_d + (long long)(s++) * rows_ld : nullptr;
  double *devr = (kinds & BESSX_COX_DIAG_DEVIANCE) ? rows_d + (long long)(s++) * rows_ld : nullptr;
  double *disp = (kinds & BESSX_COX_DIAG_DISPLACEMENT) ? rows_d + (long long)(s++) * rows_ld : nullptr;
  if (int rc = cox_diag_launch_base(in->x, f32, rs, cs, n, m, in->ties, c, st)) return rc;
  if (mart) HIPX(hipMemcpyAsync(mart, c.g, N * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (devr) HIPX(launch_cox_diag_deviance(c.v, c.g, c.d.wd, c.d.pos, n, devr, st));
  if (disp && m == 0) HIPX(hipMemsetAsync(disp, 0, N * sizeof(double), st));
  if (c.needL) {
    if (int rc = cox_diag_launch_L(in->x, f32, rs, cs, n, m, in->ties, c, st)) return rc;
    if (w_score) HIPX(launch_cox_diag_perm(c.A, c.ldA, n, m, c.rowof, score_d, score_ld, st));
    const size_t nC = w_dfb ? (size_t)cox_diag_pack_doubles(m, 0) : 0, nR = disp ? (size_t)cox_diag_pack_doubles(m, 1) : 0;
    pk.resize(nC + nR);
    if (w_dfb) {
      cox_diag_pack(in->cinv, in->cinv_ld, m, 0, pk.data());
      HIPX(hipMemcpyAsync(c.pkC, pk.data(), nC * sizeof(double), hipMemcpyHostToDevice, st));
      HIPX(launch_cox_diag_apply(c.A, c.ldA, n, m, c.pkC, 0, c.rowof, dfb_d, dfb_ld, st));
    }
    if (disp) {
      cox_diag_pack(in->factor, in->factor_ld, m, 1, pk.data() + nC);
      HIPX(hipMemcpyAsync(c.pkR, pk.data() + nC, nR * sizeof(double), hipMemcpyHostToDevice, st));
      HIPX(launch_cox_diag_apply(c.A, c.ldA, n, m, c.pkR, 1, c.rowof, disp, n, st));
    }
  }
  if (w_sch)
    HIPX(launch_cox_diag_schoenfeld(in->x, f32, rs, cs, c.d.cols, m, c.evrow, J, c.U, c.ldU, sch_d, sch_ld, st));
  if (!in->out_on_device && total > 0) {
    h.resize(total);
    HIPX(hipMemcpyAsync(h.data(), rows_d, total * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) {
    copy_out(h.data(), N, (size_t)K, in->out_rows, in->out_rows_ld);
    if (w_score) copy_out(h.data() + o_score, N, (size_t)m, in->out_score, in->out_score_ld);
    if (w_dfb) copy_out(h.data() + o_dfb, N, (size_t)m, in->out_dfbeta, in->out_dfbeta_ld);
    if (w_sch) copy_out(h.data() + o_sch, (size_t)J, (size_t)m, in->out_schoenfeld, in->out_schoenfeld_ld);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_diag_workspace(int n, int m, int n_event_rows, unsigned kinds, long long *doubles) {
  if (!doubles) return fail(BESSX_ERR_ARG, "cox_diag_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "cox_diag_workspace: empty matrix");
  if (n_event_rows < 0 || n_event_rows > n)
    return fail(BESSX_ERR_ARG, "cox_diag_workspace: n_event_rows must lie in [0, n]");
  if (kinds == 0 || (kinds & ~kCoxDiagAll))
    return fail(BESSX_ERR_ARG, "cox_diag_workspace: kinds must be a non-empty set of BESSX_COX_DIAG_* bits");
  if (int rc = check_m_max("cox_diag_workspace", m)) return rc;
  *doubles = cox_diag_doubles(n, m, n_event_rows, kinds);
  return BESSX_OK;
}

int bessx_cox_diag_device(const bessx_cox_diag_input *in, int *n_event_rows) {
  if (!in) return fail(BESSX_ERR_ARG, "cox_diag_device: null argument");
  const CoxCall c = cox_call(in);
  int J = 0;
  if (int rc = cox_diag_check_args("cox_diag_device", c, in, n_event_rows, &J)) return rc;
  int dev = -1;
  if (int rc = cox_check_device("cox_diag_device", c, &dev)) return rc;
  if (in->out_on_device) {
    const unsigned kinds = in->kinds;
    struct {
      const char *what;
      double *p;
      long long ld;
      int cols, rows;
      bool on;
    } outs[] = {
        {"out_rows", in->out_rows, in->out_rows_ld, cox_diag_rows_count(kinds), in->n, (kinds & kCoxDiagRows) != 0},
        {"out_score", in->out_score, in->out_score_ld, in->m, in->n, in->m > 0 && (kinds & BESSX_COX_DIAG_SCORE)},
        {"out_dfbeta", in->out_dfbeta, in->out_dfbeta_ld, in->m, in->n, in->m > 0 && (kinds & BESSX_COX_DIAG_DFBETA)},
        {"out_schoenfeld", in->out_schoenfeld, in->out_schoenfeld_ld, in->m, J,
         in->m > 0 && J > 0 && (kinds & BESSX_COX_DIAG_SCHOENFELD)},
    };
    for (const auto &t : outs)
      if (t.on)
        if (int rc = check_on_device("cox_diag_device", t.what, t.p, BESSX_F64, t.ld, 1, t.cols, t.rows, dev)) return rc;
  }
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  CoxInfoOrder x;
  cox_info_order(&o, in->n, in->m, in->ties, &x);
  CoxDiagOrder y;
  cox_diag_order(o, x, in->n, &y);
  const int rc = dev_call(dev, c.stream,
                          [&](DevCall &dc) { return cox_diag_run(dc.sc, o, x, y, dc.pk, dc.h, in, dc.st); });
  if (!rc) {
    *n_event_rows = x.J;
    if (in->event_rows) std::copy(y.evrow.begin(), y.evrow.end(), in->event_rows);
  }
  return rc;
}

int bessx_op_cox_diag_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int ties, int repeats, double *stage_ms, double *bytes) {
  if (!x || repeats < 1 || !stage_ms || !bytes || m < 1) return fail(BESSX_ERR_ARG, "op_cox_diag_bench: bad arguments");
  if (int rc = predict_check_model("op_cox_diag_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (ties != 0 && ties != 1) return fail(BESSX_ERR_ARG, "op_cox_diag_bench: ties must be 0 (order) or 1 (breslow)");
  if (int rc = check_m_max("op_cox_diag_bench", m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_diag_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  std::vector<double> B((size_t)m), time((size_t)n), status((size_t)n);
  for (size_t q = 0; q < B.size(); q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (int i = 0; i < n; i++) {  // (the data of op_cox_info_bench)
    const long long s = ((long long)i * 7919) % n;
    time[(size_t)i] = ties ? (double)(s / 4) : (double)s + (double)i / (2.0 * n);
    status[(size_t)i] = (double)(i % 2);
  }
  CoxOrder o;
  cox_order(time.data(), status.data(), nullptr, n, &o);
  CoxInfoOrder xo;
  cox_info_order(&o, n, m, ties, &xo);
  CoxDiagOrder yo;
  cox_diag_order(o, xo, n, &yo);
  const unsigned kinds = kCoxDiagL;
  // a P of the library's own: the scaled identity plus a small symmetric remainder (its lower triangle serves as R)
  const size_t M = (size_t)m;
  std::vector<double> P(M * M), pk((size_t)(cox_diag_pack_doubles(m, 0) + cox_diag_pack_doubles(m, 1)));
  for (size_t j = 0; j < M; j++)
    for (size_t k = 0; k < M; k++) P[j * M + k] = (j == k ? 1.0 : 1.0 / 64.0) / std::sqrt((double)n);
  cox_diag_pack(P.data(), (long long)M, m, 0, pk.data());
  cox_diag_pack(P.data(), (long long)M, m, 1, pk.data() + cox_diag_pack_doubles(m, 0));
  Owner sc;
  CoxDiagDev c;
  if (int rc = cox_diag_stage(sc, o, xo, yo, cols, m, B.data(), n, ties, kinds, nullptr, &c)) return rc;
  double *out = nullptr;
  HIPX(sc.alloc(&out, (size_t)m * (size_t)n + (size_t)n));
  HIPX(hipMemcpy(c.pkC, pk.data(), (size_t)cox_diag_pack_doubles(m, 0) * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(c.pkR, pk.data() + cox_diag_pack_doubles(m, 0), (size_t)cox_diag_pack_doubles(m, 1) * sizeof(double),
                 hipMemcpyHostToDevice));
  HIPX(hipMemset(c.res, 0, 2 * sizeof(double)));
  const int f32 = dtype == BESSX_F32;
  if (int rc = cox_diag_launch_base(x, f32, row_stride, col_stride, n, m, ties, c, nullptr)) return rc;
  HIPX(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  HIPX(sc.event(&e0));
  HIPX(sc.event(&e1));
  for (int stage = 0; stage < 4; stage++) {  // (stage 1 leaves L for stages 2 and 3)
    float total = 0.f;
    for (int i = -1; i < repeats; i++) {  // (i = -1: the warm-up)
      HIPX(hipEventRecord(e0, nullptr));
      if (stage < 2) {
        if (int rc = cox_diag_launch_L(x, f32, row_stride, col_stride, n, m, ties, c, nullptr, stage == 1)) return rc;
      } else if (stage == 2) {
        HIPX(launch_cox_diag_apply(c.A, c.ldA, n, m, c.pkR, 1, c.rowof, out, n, nullptr));
      } else {
        HIPX(launch_cox_diag_apply(c.A, c.ldA, n, m, c.pkC, 0, c.rowof, out + n, n, nullptr));
      }
      HIPX(hipEventRecord(e1, nullptr));
      HIPX(hipEventSynchronize(e1));
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) total += ms;
    }
    stage_ms[stage] = total / repeats;
  }
  const double item = f32 ? 4.0 : 8.0;
  *bytes = (double)n * m * (item + 5.0 * 8.0) + 2.0 * (double)c.J * m * 8.0;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// the meat of a robust / cluster-robust covariance on a caller's device matrix (include/bessx.h section 2k)
// ----------------------------------------------------------------------------------------------
static_assert((int)BESSX_HC0 == (int)SANDWICH_HC0 && (int)BESSX_HC1 == (int)SANDWICH_HC1 &&
                  (int)BESSX_HC2 == (int)SANDWICH_HC2 && (int)BESSX_HC3 == (int)SANDWICH_HC3, "kind codes of the launcher");
namespace {

// the rows in cluster order, cut into runs (host side of bessx_k_sandwich.hip)
struct ClusterPlan {
  std::vector<int> rowof, rptr, rdst, lptr, lgrp, iota1;  // rowof is empty when the labels are already sorted
  int G = 0, NR = 0, NL = 0;
  long long max_rows = 0, prow = 0;  // longest cluster; rows of P in use
};

// lab null: every row is its own cluster
void cluster_plan(const long long *lab, int n, int Ms, ClusterPlan *c) {
  const int RUN = sandwich_run_rows();
  std::vector<int> cptr;
  cptr.push_back(0);
  if (lab) {
    bool sorted = true;
    for (int i = 1; i < n && sorted; i++) sorted = lab[i - 1] <= lab[i];
    if (!sorted) {
      c->rowof.resize((size_t)n);
      std::iota(c->rowof.begin(), c->rowof.end(), 0);
      std::stable_sort(c->rowof.begin(), c->rowof.end(), [lab](int a, int b) { return lab[a] < lab[b]; });
    }
    for (int k = 1; k < n; k++) {
      const long long a = lab[c->rowof.empty() ? k - 1 : c->rowof[(size_t)k - 1]];
      const long long b = lab[c->rowof.empty() ? k : c->rowof[(size_t)k]];
      if (a != b) cptr.push_back(k);
    }
    cptr.push_back(n);
  } else {
    cptr.resize((size_t)n + 1);
    std::iota(cptr.begin(), cptr.end(), 0);
  }
  c->G = (int)cptr.size() - 1;
  c->lptr.push_back(0);
  for (int g = 0; g < c->G; g++) {
    const int k0 = cptr[(size_t)g], k1 = cptr[(size_t)g + 1], len = k1 - k0;
    c->max_rows = std::max<long long>(c->max_rows, len);
    if (len <= RUN) {
      c->rptr.push_back(k0);
      c->rdst.push_back(g);
    } else {
      for (int k = k0; k < k1; k += RUN) {
        c->rptr.push_back(k);
        c->rdst.push_back(-1 - (int)c->prow++);
      }
      c->lptr.push_back((int)c->prow);
      c->lgrp.push_back(g);
    }
  }
  c->rptr.push_back(n);
  c->NR = (int)c->rdst.size();
  c->NL = (int)c->lgrp.size();
  c->iota1.resize((size_t)std::max(Ms - 1, 0));
  std::iota(c->iota1.begin(), c->iota1.end(), 1);
}

struct ClusterDev {
  int *rowof = nullptr, *rptr = nullptr, *rdst = nullptr, *lptr = nullptr, *lgrp = nullptr, *iota1 = nullptr;
  double *S = nullptr, *P = nullptr, *gwork = nullptr;
  long long ldS = 0, ldP = 0;
};

int cluster_stage(Owner &sc, const ClusterPlan &c, int Ms, hipStream_t st, ClusterDev *d) {
  auto up = [&](int **dst, const std::vector<int> &v) -> int {
    if (v.empty()) return 0;
    HIPX(sc.alloc(dst, v.size()));
    HIPX(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, st));
    return 0;
  };
  if (int rc = up(&d->rowof, c.rowof)) return rc;
  if (int rc = up(&d->rptr, c.rptr)) return rc;
  if (int rc = up(&d->rdst, c.rdst)) return rc;
  if (c.NL > 0) {
    if (int rc = up(&d->lptr, c.lptr)) return rc;
    if (int rc = up(&d->lgrp, c.lgrp)) return rc;
  }
  if (int rc = up(&d->iota1, c.iota1)) return rc;
  d->ldS = sandwich_ld(c.G);
  HIPX(sc.alloc(&d->S, (size_t)d->ldS * (size_t)Ms));
  if (c.NL > 0) {
    d->ldP = sandwich_ld(c.prow);
    HIPX(sc.alloc(&d->P, (size_t)d->ldP * (size_t)Ms));
  }
  HIPX(sc.alloc(&d->gwork, (size_t)sandwich_gram_workspace(c.G, Ms)));
  return 0;
}

// S, then B and the sum vector (device memory)
int cluster_launch(const void *x, int f32, long long rs, long long cs, int n, const int *cols_d, int m, int icpt,
                   const double *u_d, const ClusterPlan &c, const ClusterDev &d, double *B, long long ld, double *sums,
                   hipStream_t st) {
  const int Ms = m + (icpt ? 1 : 0);
  HIPX(launch_sandwich_sums(x, f32, rs, cs, n, cols_d, m, icpt, u_d, d.rowof, d.rptr, d.rdst, c.NR, d.lptr, d.lgrp, c.NL,
                            d.S, d.ldS, d.P, d.ldP, st));
  HIPX(launch_sandwich_gram(d.S, 0, 1, d.ldS, c.G, Ms, d.iota1, d.S, d.gwork, B, ld, sums, st));
  return 0;
}

// the labels on the host as int64 (a device vector is copied: n elements, or ONE when its stride is 0 -- the view is then
// known to hold one element only); nullptr without labels
int cluster_labels(const long long *host, const void *dev, int dtype, long long stride, int n, hipStream_t st,
                   std::vector<long long> &buf, const long long **out) {
  *out = host;
  if (!dev) return 0;
  buf.resize((size_t)n);
  const size_t cnt = stride == 0 ? 1 : (size_t)n, item = dtype == BESSX_I64 ? 8 : 4;
  const size_t pitch = (size_t)std::max<long long>(stride, 1) * item;
  if (dtype == BESSX_I64) {
    HIPX(hipMemcpy2DAsync(buf.data(), 8, dev, pitch, 8, cnt, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
  } else {
    std::vector<int> t(cnt);
    HIPX(hipMemcpy2DAsync(t.data(), 4, dev, pitch, 4, cnt, hipMemcpyDeviceToHost, st));
    HIPX(hipStreamSynchronize(st));
    for (size_t i = 0; i < cnt; i++) buf[i] = t[i];
  }
  if (stride == 0) std::fill(buf.begin(), buf.end(), buf[0]);
  *out = buf.data();
  return 0;
}

int cluster_check_args(const std::string &w, const long long *host, const void *dev, int dtype, long long stride) {
  if (host && dev) return fail(BESSX_ERR_ARG, w + ": give cluster as a host pointer or as a device vector, not both");
  if (dev && dtype != BESSX_I64 && dtype != BESSX_I32)
    return fail(BESSX_ERR_ARG, w + ": cluster: dtype must be BESSX_I64 or BESSX_I32");
  if (stride < 0) return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  return 0;
}

int cluster_check_device(const char *who, const void *dev, int dtype, long long stride, int n, int xdev) {
  if (!dev) return 0;
  return check_on_device(who, "cluster", dev, dtype == BESSX_I32 ? BESSX_F32 : BESSX_F64, stride, 0, n, 1, xdev);
}

int meat_check_args(const bessx_meat_input *in, const int *n_clusters) {
  const std::string w("meat_device");
  if (!in || !n_clusters) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (!in->x || !in->meat || !in->sums) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (in->x_dtype != BESSX_F64 && in->x_dtype != BESSX_F32)
    return fail(BESSX_ERR_ARG, w + ": x: dtype must be BESSX_F64 or BESSX_F32");
  if (in->x_row_stride < 0 || in->x_col_stride < 0) return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  if (int rc = predict_check_model("meat_device", in->n, in->p, in->cols, in->m, 1, BESSX_LINK_IDENTITY)) return rc;
  const long long Ms = (long long)in->m + (in->intercept ? 1 : 0);
  if (Ms < 1) return fail(BESSX_ERR_ARG, w + ": an empty support needs the intercept");
  if (in->u_host && in->u_dev) return fail(BESSX_ERR_ARG, w + ": give u as a host pointer or as a device vector, not both");
  if (int rc = cluster_check_args(w, in->cluster_host, in->cluster_dev, in->cluster_dtype, in->cluster_stride)) return rc;
  if (in->meat_ld < Ms) return fail(BESSX_ERR_ARG, w + ": meat_ld must be at least m + intercept");
  if (Ms > INFO_M_MAX)
    return fail(BESSX_ERR_UNSUPPORTED, w + ": m + intercept must be at most " + std::to_string(INFO_M_MAX));
  return 0;
}

int meat_run(Owner &sc, ClusterPlan &plan, std::vector<long long> &lbuf, std::vector<double> &h,
             const bessx_meat_input *in, int *n_clusters, hipStream_t st) {
  const int f32 = in->x_dtype == BESSX_F32, m = in->m, n = in->n, icpt = in->intercept ? 1 : 0, Ms = m + icpt;
  const size_t M = (size_t)Ms, nv = ((size_t)n + 1) / 2 * 2;
  const long long *lab = nullptr;
  if (int rc = cluster_labels(in->cluster_host, in->cluster_dev, in->cluster_dtype, in->cluster_stride, n, st, lbuf, &lab))
    return rc;
  int *cols_d = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  if (m > 0) HIPX(hipMemcpyAsync(cols_d, in->cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
  const double *u_d = in->u_dev;
  if (in->u_host) {
    double *t = nullptr;
    HIPX(sc.alloc(&t, nv));
    HIPX(hipMemcpyAsync(t, in->u_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    u_d = t;
  }
  double *stage = nullptr, *B = in->meat, *sums = in->sums;
  long long ld = in->meat_ld;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&stage, M * M + M));
    B = stage;
    sums = stage + M * M;
    ld = (long long)M;
  }
  if (!lab && icpt) {
    // one sweep over x in place: vw = u^2, gw = u (ones without u)
    double *w = nullptr;
    HIPX(sc.alloc(&w, 2 * nv + (size_t)info_gram_workspace(n, m)));
    if (u_d) {
      HIPX(launch_sandwich_u(u_d, nullptr, SANDWICH_HC0, n, w, w + nv, st));
    } else {
      std::vector<double> &ones = h;  // (h outlives the copy; it is resized for the results only after the sync below)
      ones.assign(nv, 1.0);
      HIPX(hipMemcpyAsync(w, ones.data(), nv * sizeof(double), hipMemcpyHostToDevice, st));
      HIPX(hipMemcpyAsync(w + nv, ones.data(), nv * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPX(launch_info_gram(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, w + nv, w, w + 2 * nv, B, ld,
                          sums, st));
    *n_clusters = 0;
  } else if (!lab && !u_d) {
    // a dense source as it is: column cols[0] is copied to an n-vector (the sweep's score weight), the sweep runs over
    // the other columns of x in place -- launch_sandwich_gram's use of the sweep, with x in the place of S
    double *w = nullptr;
    HIPX(sc.alloc(&w, nv + (size_t)sandwich_gram_workspace(n, Ms)));
    HIPX(launch_sandwich_column(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, w, st));
    HIPX(launch_sandwich_gram(in->x, f32, in->x_row_stride, in->x_col_stride, n, Ms, cols_d + 1, w, w + nv, B, ld, sums,
                              st));
    *n_clusters = 0;
  } else {
    cluster_plan(lab, n, Ms, &plan);
    ClusterDev d;
    if (int rc = cluster_stage(sc, plan, Ms, st, &d)) return rc;
    if (int rc = cluster_launch(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, icpt, u_d, plan, d, B, ld,
                                sums, st))
      return rc;
    *n_clusters = lab ? plan.G : 0;
  }
  if (!in->out_on_device) {
    HIPX(hipStreamSynchronize(st));
    h.resize(M * M + M);
    HIPX(hipMemcpyAsync(h.data(), stage, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) {
    copy_out(h.data(), M, M, in->meat, in->meat_ld);
    copy_out(h.data() + M * M, M, 1, in->sums, 0);
  }
  return 0;
}

int sandwich_check_args(const GlmCall &c, const bessx_sandwich_input *in, const double *loss, const double *sum_w) {
  const std::string w("sandwich_device");
  if (int rc = info_check_args("sandwich_device", c, in->info, in->info_ld, in->score, loss, sum_w)) return rc;
  if (!in->meat) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (in->meat_ld < (long long)in->m + 1) return fail(BESSX_ERR_ARG, w + ": meat_ld must be at least m + 1");
  if (in->kind < BESSX_HC0 || in->kind > BESSX_HC3) return fail(BESSX_ERR_ARG, w + ": kind must be one of BESSX_HC0 .. BESSX_HC3");
  if (int rc = cluster_check_args(w, in->cluster_host, in->cluster_dev, in->cluster_dtype, in->cluster_stride)) return rc;
  if ((in->cluster_host || in->cluster_dev) && in->kind >= BESSX_HC2)
    return fail(BESSX_ERR_ARG, w + ": cluster labels go with BESSX_HC0 or BESSX_HC1 only");
  if (in->kind >= BESSX_HC2) {
    if (!in->factor) return fail(BESSX_ERR_ARG, w + ": BESSX_HC2 and BESSX_HC3 need the factor");
    if (in->factor_ld < (long long)in->m + 1) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m + 1");
    for (long long j = 0; j <= in->m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  return 0;
}

// doubles of device scratch of a sandwich call besides the model and host y / weight (an upper bound when the labels
// are not known: G clusters, the longest of max_rows rows; G = 0: no labels)
long long sandwich_doubles(int f32, long long rs, long long cs, long long n, int m, int link, int weighted, int kind,
                           long long G, long long max_rows) {
  const long long nv = (n + 1) / 2 * 2, M = (long long)m + 1;
  long long d = info_workspace(f32, rs, cs, n, m, link, weighted) + 3 + 2 * nv + M;  // res, u, u^2, the sweep's score
  if (kind >= BESSX_HC2) d += nv + diag_factor_doubles(m);
  if (G > 0) {
    d += sandwich_ld(G) * M + sandwich_gram_workspace(G, (int)M);
    const long long pr = sandwich_partial_rows(n, G, max_rows);
    if (pr > 0) d += sandwich_ld(pr) * M;
  }
  return d;
}

int sandwich_run(Owner &sc, ClusterPlan &plan, std::vector<long long> &lbuf, std::vector<double> &pk,
                 std::vector<double> &h, const GlmCall &c, const bessx_sandwich_input *in, double *loss, double *sum_w,
                 int *n_clusters, hipStream_t st) {
  const int f32 = in->x_dtype == BESSX_F32, m = in->m, n = in->n, kind = in->kind;
  const long long rs = in->x_row_stride, cs = in->x_col_stride;
  const size_t M = (size_t)m + 1, nv = ((size_t)n + 1) / 2 * 2;
  const long long *lab = nullptr;
  if (int rc = cluster_labels(in->cluster_host, in->cluster_dev, in->cluster_dtype, in->cluster_stride, n, st, lbuf, &lab))
    return rc;
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *work = nullptr, *res = nullptr, *stage = nullptr, *uw = nullptr;
  if (int rc = predict_upload_model(sc, in->cols, m, in->beta, &in->coef0, 1, st, &cols_d, &B_d, &c_d)) return rc;
  EvalData d;
  if (int rc = eval_stage_data(sc, c, st, &d)) return rc;
  HIPX(sc.alloc(&work, (size_t)info_workspace(f32, rs, cs, n, m, in->link, d.w != nullptr)));
  HIPX(sc.alloc(&res, 3));
  HIPX(sc.alloc(&uw, 2 * nv + M));
  double *info_d = in->info, *score_d = in->score, *meat_d = in->meat;
  long long ld = in->info_ld, mld = in->meat_ld;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&stage, 2 * M * M + M));
    info_d = stage;
    score_d = stage + M * M;
    meat_d = score_d + M;
    ld = mld = (long long)M;
  }
  HIPX(launch_info(in->x, f32, rs, cs, n, cols_d, m, B_d, c_d, in->link, d, work, res, info_d, ld, score_d, st));
  // launch_info's work starts with v and g (nv doubles each) and the partials of its sweep, which have served
  double *v_d = work, *g_d = work + nv, *part = work + 2 * nv, *u_d = uw, *u2_d = uw + nv, *sc2 = uw + 2 * nv;
  // with labels u must be the same bits under every layout: the pass with threads along rows (without labels nothing
  // needs that, and on a row-contiguous x the second pass would cost as much as the first)
  if (lab && !info_eta_by_rows(rs, cs, m))
    HIPX(launch_info_vg(in->x, f32, rs, cs, n, cols_d, m, B_d, c_d, in->link, d, v_d, g_d, st));
  double *h_d = nullptr;
  if (kind >= BESSX_HC2) {
    double *pk_d = nullptr;
    pk.resize((size_t)diag_factor_doubles(m));
    diag_pack_factor(in->factor, in->factor_ld, m, pk.data());
    HIPX(sc.alloc(&h_d, nv));
    HIPX(sc.alloc(&pk_d, pk.size()));
    HIPX(hipMemcpyAsync(pk_d, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPX(launch_diag_lev(in->x, f32, rs, cs, n, cols_d, m, pk_d, v_d, nullptr, nullptr, 1.0, h_d, nullptr, nullptr,
                         nullptr, st));
  }
  HIPX(launch_sandwich_u(g_d, h_d, kind, n, u_d, u2_d, st));
  if (!lab) {
    HIPX(launch_info_gram(in->x, f32, rs, cs, n, cols_d, m, u2_d, g_d, part, meat_d, mld, sc2, st));
    *n_clusters = 0;
  } else {
    cluster_plan(lab, n, (int)M, &plan);
    ClusterDev cd;
    if (int rc = cluster_stage(sc, plan, (int)M, st, &cd)) return rc;
    if (int rc = cluster_launch(in->x, f32, rs, cs, n, cols_d, m, 1, u_d, plan, cd, meat_d, mld, sc2, st)) return rc;
    *n_clusters = plan.G;
  }
  h.resize(3 + (in->out_on_device ? 0 : 2 * M * M + M));
  HIPX(hipMemcpyAsync(h.data(), res, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (!in->out_on_device)
    HIPX(hipMemcpyAsync(h.data() + 3, stage, (2 * M * M + M) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  *loss = h[0];
  *sum_w = d.w ? h[2] : (double)n;
  if (!in->out_on_device) {
    const double *hi = h.data() + 3, *hs = hi + M * M, *hm = hs + M;
    copy_out(hi, M, M, in->info, in->info_ld);
    copy_out(hs, M, 1, in->score, 0);
    copy_out(hm, M, M, in->meat, in->meat_ld);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_sandwich_workspace(int x_dtype, long long x_row_stride, long long x_col_stride, int n, int m, int link,
                             int weighted, int kind, int n_clusters, int max_cluster_rows, long long *doubles,
                             long long *rows_per_slab, int *slabs, long long *cluster_rows_per_slab, int *cluster_slabs,
                             int *sum_depth, int *sq_depth) {
  if (!doubles || !rows_per_slab || !slabs || !cluster_rows_per_slab || !cluster_slabs || !sum_depth || !sq_depth)
    return fail(BESSX_ERR_ARG, "sandwich_workspace: null argument");
  if (x_dtype != BESSX_F64 && x_dtype != BESSX_F32)
    return fail(BESSX_ERR_ARG, "sandwich_workspace: x: dtype must be BESSX_F64 or BESSX_F32");
  if (x_row_stride < 0 || x_col_stride < 0)
    return fail(BESSX_ERR_ARG, "sandwich_workspace: strides must be non-negative");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "sandwich_workspace: empty matrix");
  if (link != BESSX_LINK_IDENTITY && link != BESSX_LINK_LOGISTIC && link != BESSX_LINK_POISSON)
    return fail(BESSX_ERR_ARG, "sandwich_workspace: unknown link");
  if (kind < BESSX_HC0 || kind > BESSX_HC3)
    return fail(BESSX_ERR_ARG, "sandwich_workspace: kind must be one of BESSX_HC0 .. BESSX_HC3");
  if (n_clusters < 0 || n_clusters > n || max_cluster_rows < 0 || max_cluster_rows > n ||
      (n_clusters > 0 && max_cluster_rows < 1))
    return fail(BESSX_ERR_ARG, "sandwich_workspace: n_clusters and max_cluster_rows must lie in [0, n]");
  if (int rc = check_m_max("sandwich_workspace", m)) return rc;
  *doubles = sandwich_doubles(x_dtype == BESSX_F32, x_row_stride, x_col_stride, n, m, link, weighted != 0, kind,
                              n_clusters, max_cluster_rows);
  info_split(n, m, rows_per_slab, slabs);
  *cluster_rows_per_slab = 0;
  *cluster_slabs = 0;
  if (n_clusters > 0) info_split(n_clusters, m, cluster_rows_per_slab, cluster_slabs);  // (the sweep's M is m + 1)
  *sum_depth = n_clusters > 0 ? sandwich_sum_depth(max_cluster_rows) : 0;
  *sq_depth = n_clusters > 0 ? sandwich_sq_depth(n_clusters) : 0;
  return BESSX_OK;
}

int bessx_meat_device(const bessx_meat_input *in, int *n_clusters) {
  if (int rc = meat_check_args(in, n_clusters)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("meat_device: x", in->x, in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,
                                   in->p, &dev))
    return rc;
  if (in->u_dev)
    if (int rc = check_on_device("meat_device", "u", in->u_dev, BESSX_F64, 1, 0, in->n, 1, dev)) return rc;
  if (int rc = cluster_check_device("meat_device", in->cluster_dev, in->cluster_dtype, in->cluster_stride, in->n, dev))
    return rc;
  if (in->out_on_device) {
    const int Ms = in->m + (in->intercept ? 1 : 0);
    if (int rc = check_on_device("meat_device", "meat", in->meat, BESSX_F64, in->meat_ld, 1, Ms, Ms, dev)) return rc;
    if (int rc = check_on_device("meat_device", "sums", in->sums, BESSX_F64, 1, 0, Ms, 1, dev)) return rc;
  }
  ClusterPlan plan;
  std::vector<long long> lbuf;
  return dev_call(dev, static_cast<hipStream_t>(in->stream),
                  [&](DevCall &dc) { return meat_run(dc.sc, plan, lbuf, dc.h, in, n_clusters, dc.st); });
}

int bessx_sandwich_device(const bessx_sandwich_input *in, double *loss, double *sum_w, int *n_clusters) {
  if (!in || !n_clusters) return fail(BESSX_ERR_ARG, "sandwich_device: null argument");
  const GlmCall c = glm_call(in);
  if (int rc = sandwich_check_args(c, in, loss, sum_w)) return rc;
  int dev = -1;
  if (int rc = glm_check_device("sandwich_device", c, &dev)) return rc;
  if (int rc = cluster_check_device("sandwich_device", in->cluster_dev, in->cluster_dtype, in->cluster_stride, in->n,
                                    dev))
    return rc;
  if (in->out_on_device) {
    const int M = in->m + 1;
    if (int rc = check_on_device("sandwich_device", "info", in->info, BESSX_F64, in->info_ld, 1, M, M, dev)) return rc;
    if (int rc = check_on_device("sandwich_device", "score", in->score, BESSX_F64, 1, 0, M, 1, dev)) return rc;
    if (int rc = check_on_device("sandwich_device", "meat", in->meat, BESSX_F64, in->meat_ld, 1, M, M, dev)) return rc;
  }
  ClusterPlan plan;
  std::vector<long long> lbuf;
  return dev_call(dev, c.stream, [&](DevCall &dc) {
    return sandwich_run(dc.sc, plan, lbuf, dc.pk, dc.h, c, in, loss, sum_w, n_clusters, dc.st);
  });
}

int bessx_op_sandwich_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, const long long *cluster, int repeats, double *avg_ms,
                            double *bytes) {
  if (!x || !cluster || repeats < 1 || !avg_ms || !bytes) return fail(BESSX_ERR_ARG, "op_sandwich_bench: bad arguments");
  if (int rc = predict_check_model("op_sandwich_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_sandwich_bench", m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_sandwich_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const int Ms = m + 1, f32 = dtype == BESSX_F32;
  ClusterPlan plan;
  cluster_plan(cluster, n, Ms, &plan);
  ClusterDev d;
  if (int rc = cluster_stage(sc, plan, Ms, nullptr, &d)) return rc;
  std::vector<double> u((size_t)n);
  for (size_t i = 0; i < u.size(); i++) u[i] = (i % 2) ? -0.5 : 0.5;
  int *cols_d = nullptr;
  double *u_d = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&u_d, u.size()));
  if (m > 0) HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(u_d, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  float ms = 0.f;
  if (int rc = bt.run(repeats, &ms, [&]() -> int {
        HIPX(launch_sandwich_sums(x, f32, row_stride, col_stride, n, cols_d, m, 1, u_d, d.rowof, d.rptr, d.rdst, plan.NR,
                                  d.lptr, d.lgrp, plan.NL, d.S, d.ldS, d.P, d.ldP, nullptr));
        return 0;
      }))
    return rc;
  *avg_ms = ms / repeats;
  // what the algorithm needs: the support and u once, S once
  *bytes = (double)n * m * (f32 ? 4.0 : 8.0) + 8.0 * (double)n + 8.0 * (double)Ms * (double)plan.G;
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// score tests of candidate columns against one model on a caller's device matrix (include/bessx.h section 2l)
// ----------------------------------------------------------------------------------------------
namespace {

int addscore_check_block(const std::string &w, int block) {
  if (block < 0 || block % 16) return fail(BESSX_ERR_ARG, w + ": candidate_block must be 0 or a positive multiple of 16");
  return 0;
}

// everything about the call that needs no device
int addscore_check_args(const char *who, const GlmCall &c, const bessx_addscore_input *in, const double *loss,
                        const double *sum_w) {
  const std::string w(who);
  if (int rc = info_check_args(who, c, in->info, in->info_ld, in->score, loss, sum_w)) return rc;
  if (!in->u || !in->d) return fail(BESSX_ERR_ARG, w + ": null argument (u, d)");
  if (in->factor && (!in->s || !in->a)) return fail(BESSX_ERR_ARG, w + ": null argument (s, a)");
  if (in->q < 1) return fail(BESSX_ERR_ARG, w + ": q must be at least 1");
  if (!in->candidates && in->q != in->p) return fail(BESSX_ERR_ARG, w + ": without a candidate list q must be p");
  if (in->candidates) {
    for (int j = 0; j < in->q; j++) {
      if (in->candidates[j] < 0 || in->candidates[j] >= in->p)
        return fail(BESSX_ERR_ARG, w + ": a candidate is not a column of x");
      if (j > 0 && in->candidates[j] <= in->candidates[j - 1])
        return fail(BESSX_ERR_ARG, w + ": candidates must be ascending and distinct");
    }
  }
  if (int rc = addscore_check_block(w, in->candidate_block)) return rc;
  if (in->cross && in->cross_ld < (long long)in->m + 1)
    return fail(BESSX_ERR_ARG, w + ": cross_ld must be at least m + 1");
  if (in->factor) {
    if (in->factor_ld < (long long)in->m + 1) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m + 1");
    for (long long j = 0; j <= in->m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  return 0;
}

int addscore_run(Owner &sc, std::vector<double> &pk, std::vector<double> &h, const GlmCall &c,
                 const bessx_addscore_input *in, double *loss, double *sum_w, hipStream_t st) {
  const int f32 = in->x_dtype == BESSX_F32, m = in->m, q = in->q, block = in->candidate_block;
  const long long n = in->n, nv = (n + 1) / 2 * 2;
  const size_t M = (size_t)m + 1, Q = (size_t)q;
  const bool with_stat = in->factor != nullptr, want_c = in->cross != nullptr;
  long long panel = 0, blk = 0, rps = 0;
  int slabs = 0, cb = 0, depth = 0;
  addscore_split(n, m, q, block, &panel, &blk, &rps, &slabs, &cb, &depth);
  int *cols_d = nullptr, *cand_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *iwork = nullptr, *res = nullptr, *istage = nullptr, *vg = nullptr, *P = nullptr,
         *work = nullptr, *ostage = nullptr;
  if (int rc = predict_upload_model(sc, in->cols, m, in->beta, &in->coef0, 1, st, &cols_d, &B_d, &c_d)) return rc;
  EvalData d;
  if (int rc = eval_stage_data(sc, c, st, &d)) return rc;
  // 1. info, score, loss and sum_w: launch_info as bessx_info_device runs it (the same bits)
  HIPX(sc.alloc(&iwork, (size_t)info_workspace(f32, in->x_row_stride, in->x_col_stride, in->n, m, in->link,
                                                d.w != nullptr)));
  HIPX(sc.alloc(&res, 3));
  HIPX(sc.alloc(&istage, M * M + M));
  HIPX(launch_info(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, B_d, c_d, in->link, d, iwork, res, istage,
                   (long long)M, istage + M * M, st));
  h.resize(3 + M * M + 2 * M);
  HIPX(hipMemcpyAsync(h.data(), res, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipMemcpyAsync(h.data() + 3, istage, (M * M + M) * sizeof(double), hipMemcpyDeviceToHost, st));
  // the row weights, always by rows: the same bits under every layout of x
  HIPX(sc.alloc(&vg, (size_t)(2 * nv)));
  HIPX(launch_info_vg(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, B_d, c_d, in->link, d, vg, vg + nv,
                      st));
  HIPX(sc.alloc(&P, (size_t)panel));
  HIPX(sc.alloc(&work, (size_t)blk));
  if (in->candidates) {
    HIPX(sc.alloc(&cand_d, Q));
    HIPX(hipMemcpyAsync(cand_d, in->candidates, Q * sizeof(int), hipMemcpyHostToDevice, st));
  }
  HIPX(launch_addscore_pack(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, q, block, vg, vg + nv, P, st));
  // the score behind r, summed by this section's own kernels over the list (constant column, support): the same bits
  // under every layout of x, which launch_info's score is not
  std::vector<int> cand0;
  double *u0 = nullptr;
  if (with_stat) {
    long long panel0 = 0, blk0 = 0, rps0 = 0;
    int slabs0 = 0, cb0 = 0, depth0 = 0, *cand0_d = nullptr;
    double *work0 = nullptr;
    addscore_split(n, m, (int)M, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
    cand0.assign(M, -1);
    std::copy(in->cols, in->cols + m, cand0.begin() + 1);
    HIPX(sc.alloc(&cand0_d, M));
    HIPX(sc.alloc(&work0, (size_t)blk0));
    HIPX(sc.alloc(&u0, 2 * M));
    HIPX(hipMemcpyAsync(cand0_d, cand0.data(), M * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(launch_addscore_blocks(in->x, f32, in->x_row_stride, in->x_col_stride, n, m, cand0_d, (int)M, 0, P, work0, 0, u0,
                                u0 + M, nullptr, nullptr, nullptr, 0, 0, st));
    HIPX(hipMemcpyAsync(h.data() + 3 + M * M + M, u0, M * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  *loss = h[0];
  *sum_w = d.w ? h[2] : (double)in->n;
  copy_out(h.data() + 3, M, M, in->info, in->info_ld);
  copy_out(h.data() + 3 + M * M, M, 1, in->score, 0);
  if (with_stat) {
    // r = inverse(info) U = R^T (R U), on the host in fp64
    const double *U0 = h.data() + 3 + M * M + M;
    std::vector<double> t(M, 0.0), r(M, 0.0);
    for (size_t j = 0; j < M; j++)
      for (size_t k = 0; k <= j; k++) t[j] += in->factor[j * in->factor_ld + k] * U0[k];
    for (size_t j = 0; j < M; j++)
      for (size_t k = 0; k <= j; k++) r[k] += in->factor[j * in->factor_ld + k] * t[j];
    pk.resize((size_t)diag_factor_doubles(m + 1));
    addscore_pack_factor(in->factor, in->factor_ld, r.data(), m, pk.data());
    HIPX(hipMemcpyAsync(work + blk - (long long)pk.size(), pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice,
                        st));
  }
  double *u = in->u, *dd = in->d, *s = in->s, *a = in->a, *C = in->cross;
  long long ldc = in->cross_ld;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&ostage, 4 * Q + (want_c ? Q * M : 0)));
    u = ostage, dd = ostage + Q, s = ostage + 2 * Q, a = ostage + 3 * Q;
    C = want_c ? ostage + 4 * Q : nullptr;
    ldc = (long long)M;
  }
  HIPX(launch_addscore_blocks(in->x, f32, in->x_row_stride, in->x_col_stride, n, m, cand_d, q, block, P, work,
                              with_stat ? 1 : 0, u, dd, s, a, C, ldc, 0, st));
  if (!in->out_on_device) {
    h.resize(4 * Q + (want_c ? Q * M : 0));
    HIPX(hipMemcpyAsync(h.data(), ostage, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) {
    std::copy(h.begin(), h.begin() + Q, in->u);
    std::copy(h.begin() + Q, h.begin() + 2 * Q, in->d);
    if (with_stat) {
      std::copy(h.begin() + 2 * Q, h.begin() + 3 * Q, in->s);
      std::copy(h.begin() + 3 * Q, h.begin() + 4 * Q, in->a);
    }
    if (want_c) copy_out(h.data() + 4 * Q, M, Q, in->cross, in->cross_ld);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_addscore_workspace(int n, int m, int q, int candidate_block, long long *doubles, long long *rows_per_slab,
                             int *slabs, int *block, long long *block_doubles, int *sum_depth) {
  if (!doubles || !rows_per_slab || !slabs || !block || !block_doubles || !sum_depth)
    return fail(BESSX_ERR_ARG, "addscore_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "addscore_workspace: empty matrix");
  if (q < 1) return fail(BESSX_ERR_ARG, "addscore_workspace: q must be at least 1");
  if (int rc = addscore_check_block("addscore_workspace", candidate_block)) return rc;
  if (int rc = check_m_max("addscore_workspace", m)) return rc;
  long long panel = 0;
  addscore_split(n, m, q, candidate_block, &panel, block_doubles, rows_per_slab, slabs, block, sum_depth);
  // (plus the block workspace of the score behind r, whose candidates are the constant column and the support)
  long long panel0 = 0, blk0 = 0, rps0 = 0;
  int slabs0 = 0, cb0 = 0, depth0 = 0;
  addscore_split(n, m, m + 1, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
  *block_doubles += blk0 + 2 * ((long long)m + 1);
  *doubles = 2 * (((long long)n + 1) / 2 * 2) + panel + *block_doubles;
  return BESSX_OK;
}

int bessx_addscore_device(const bessx_addscore_input *in, double *loss, double *sum_w) {
  if (!in) return fail(BESSX_ERR_ARG, "addscore_device: null argument");
  const GlmCall c = glm_call(in);
  if (int rc = addscore_check_args("addscore_device", c, in, loss, sum_w)) return rc;
  int dev = -1;
  if (int rc = glm_check_device("addscore_device", c, &dev)) return rc;
  if (in->out_on_device) {
    double *const vec[4] = {in->u, in->d, in->factor ? in->s : nullptr, in->factor ? in->a : nullptr};
    for (double *v : vec)
      if (v)
        if (int rc = check_on_device("addscore_device", "u, d, s, a", v, BESSX_F64, 1, 0, in->q, 1, dev, "an output"))
          return rc;
    if (in->cross)
      if (int rc = check_on_device("addscore_device", "cross", in->cross, BESSX_F64, in->cross_ld, 1, in->q, in->m + 1, dev))
        return rc;
  }
  return dev_call(dev, c.stream,
                  [&](DevCall &dc) { return addscore_run(dc.sc, dc.pk, dc.h, c, in, loss, sum_w, dc.st); });
}

int bessx_op_addscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, const int *candidates, int q, int candidate_block, int repeats,
                            double *stage_ms) {
  if (!x || repeats < 1 || !stage_ms || q < 1) return fail(BESSX_ERR_ARG, "op_addscore_bench: bad arguments");
  if (int rc = predict_check_model("op_addscore_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_addscore_bench", m)) return rc;
  if (int rc = addscore_check_block("op_addscore_bench", candidate_block)) return rc;
  if (!candidates && q != p) return fail(BESSX_ERR_ARG, "op_addscore_bench: without a candidate list q must be p");
  if (candidates)
    for (int j = 0; j < q; j++)
      if (candidates[j] < 0 || candidates[j] >= p || (j > 0 && candidates[j] <= candidates[j - 1]))
        return fail(BESSX_ERR_ARG, "op_addscore_bench: candidates must be ascending distinct columns of x");
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_addscore_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t M = (size_t)m + 1, Q = (size_t)q;
  long long panel = 0, blk = 0, rps = 0;
  int slabs = 0, cb = 0, depth = 0;
  addscore_split(n, m, q, candidate_block, &panel, &blk, &rps, &slabs, &cb, &depth);
  // row weights and a factor of the library's own: the scaled identity plus a small lower triangle
  std::vector<double> v((size_t)n, 0.25), g((size_t)n), R(M * M, 0.0), r(M, 1.0 / 128.0),
      pk((size_t)diag_factor_doubles(m + 1));
  for (size_t i = 0; i < g.size(); i++) g[i] = (i % 2) ? -0.5 : 0.5;
  for (size_t j = 0; j < M; j++)
    for (size_t k = 0; k <= j; k++) R[j * M + k] = (j == k ? 1.0 : 1.0 / 64.0) / std::sqrt((double)n);
  addscore_pack_factor(R.data(), (long long)M, r.data(), m, pk.data());
  int *cols_d = nullptr, *cand_d = nullptr;
  double *v_d = nullptr, *g_d = nullptr, *P = nullptr, *work = nullptr, *out = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&v_d, v.size()));
  HIPX(sc.alloc(&g_d, g.size()));
  HIPX(sc.alloc(&P, (size_t)panel));
  HIPX(sc.alloc(&work, (size_t)blk));
  HIPX(sc.alloc(&out, 4 * Q));
  if (m > 0) HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  if (candidates) {
    HIPX(sc.alloc(&cand_d, Q));
    HIPX(hipMemcpy(cand_d, candidates, Q * sizeof(int), hipMemcpyHostToDevice));
  }
  HIPX(hipMemcpy(v_d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(g_d, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(work + blk - (long long)pk.size(), pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  auto run = [&](int stage) -> int {
    if (stage == 0)
      HIPX(launch_addscore_pack(x, f32, row_stride, col_stride, n, cols_d, m, q, candidate_block, v_d, g_d, P, nullptr));
    else
      HIPX(launch_addscore_blocks(x, f32, row_stride, col_stride, n, m, cand_d, q, candidate_block, P, work, 1, out,
                                  out + Q, out + 2 * Q, out + 3 * Q, nullptr, 0, stage, nullptr));
    return 0;
  };
  // (stage 0 = pack, 1 = cross, 2 = finish, 3 = statistic; each over every block of candidates, in this order, so that
  // a later stage finds the earlier one's results of the last block)
  for (int stage = 0; stage < 4; stage++) {
    float ms = 0.f;
    if (int rc = bt.run(repeats, &ms, [&]() { return run(stage); })) return rc;
    stage_ms[stage] = ms / repeats;
  }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// score tests of candidate columns against one Cox model on a caller's device matrix (include/bessx.h section 2m)
// ----------------------------------------------------------------------------------------------
namespace {

// everything about the call that needs no device
int cox_addscore_check_args(const char *who, const CoxCall &c, const bessx_cox_addscore_input *in, const double *loglik,
                            const double *n_events, const double *residual_sum) {
  const std::string w(who);
  if (int rc = cox_info_check_args(who, c, in->info, in->info_ld, in->score, loglik, n_events, residual_sum)) return rc;
  if (!in->u || !in->d || !in->t) return fail(BESSX_ERR_ARG, w + ": null argument (u, d, t)");
  if (in->factor && (!in->s || !in->a)) return fail(BESSX_ERR_ARG, w + ": null argument (s, a)");
  if (in->q < 1) return fail(BESSX_ERR_ARG, w + ": q must be at least 1");
  if (!in->candidates && in->q != in->p) return fail(BESSX_ERR_ARG, w + ": without a candidate list q must be p");
  if (in->candidates) {
    for (int j = 0; j < in->q; j++) {
      if (in->candidates[j] < 0 || in->candidates[j] >= in->p)
        return fail(BESSX_ERR_ARG, w + ": a candidate is not a column of x");
      if (j > 0 && in->candidates[j] <= in->candidates[j - 1])
        return fail(BESSX_ERR_ARG, w + ": candidates must be ascending and distinct");
    }
  }
  if (int rc = addscore_check_block(w, in->candidate_block)) return rc;
  if (in->cross && in->cross_ld < (long long)in->m + 1)
    return fail(BESSX_ERR_ARG, w + ": cross_ld must be at least m + 1");
  if (in->factor && in->m > 0) {
    if (in->factor_ld < (long long)in->m) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m");
    for (long long j = 0; j < in->m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  return 0;
}

// doubles of device scratch of one call beyond section 2h's, and the part of them that does not depend on p
void cox_addscore_doubles(long long n, int m, long long J, int q, int block, long long *all, long long *blockpart) {
  const long long nb = (n + 1023) / 1024, M = (long long)m + 1;
  long long panel = 0, blk = 0, rps = 0, part = 0, rpsq = 0;
  int slabs = 0, cb = 0, depth = 0, slabsq = 0, tdepth = 0;
  addscore_split(n, m, q, block, &panel, &blk, &rps, &slabs, &cb, &depth);
  cox_addscore_split(n, q, block, &part, &rpsq, &slabsq, &tdepth);
  long long d = cox_info_doubles(n, m, J) + (long long)m * m + m + 2;
  if (m == 0) d += 3 * n + cox_surv_workspace(n);  // e, v, g and the totals of H's scan, which section 2h skips at m = 0
  if (m > 0) d += cox_diag_lda(n) * m + n + nb * m;  // A, dh, A's totals
  d += n + nb + panel + blk + part;                  // Cc and its totals, the panel, the block workspaces
  long long bp = blk + part;
  if (m > 0) {  // the score behind r: the support as candidates
    long long panel0 = 0, blk0 = 0, rps0 = 0;
    int slabs0 = 0, cb0 = 0, depth0 = 0;
    addscore_split(n, m, m, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
    d += blk0 + 2 * M;
    bp += blk0 + 2 * M;
  }
  *all = d;
  *blockpart = bp;
}

// steps 1 to 3 that sections 2m and 2o share: info, score, loglik and residual_sum by section 2h's launches (queued into h:
// loglik, residual_sum, then info and score), e, S0, v, g -- once more by rows where section 2h's predictor pass gathers
// -- and A (null when m = 0).  c, *A_out and *ldA_out are the caller's to use; sc and h must outlive what is queued on st
int cox_score_stage(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const void *xp, int f32, long long rs,
                    long long cs, int n, const int *cols, int m, const double *beta, int ties, std::vector<double> &h,
                    hipStream_t st, CoxInfoDev &c, double **A_out, long long *ldA_out) {
  const size_t N = (size_t)n, mm = (size_t)m * (size_t)m, nb = (size_t)((n + 1023) / 1024);
  // 1. info, score, loglik and residual_sum: section 2h's launches as bessx_cox_info_device runs them (the same bits)
  if (int rc = cox_info_stage(sc, o, x, cols, m, beta, n, ties, st, &c)) return rc;
  const CoxDev &d = c.d;
  HIPX(hipMemsetAsync(c.res, 0, 2 * sizeof(double), st));
  double *istage = nullptr, *res2 = nullptr;
  h.resize(2 + mm + 2 * (size_t)m);
  if (m > 0) {
    HIPX(sc.alloc(&istage, mm + (size_t)m));
    if (int rc = cox_info_launch(xp, f32, rs, cs, n, m, ties, c, istage, m, istage + mm, st)) return rc;
    HIPX(hipMemcpyAsync(h.data() + 2, istage, (mm + (size_t)m) * sizeof(double), hipMemcpyDeviceToHost, st));
  } else {
    // (section 2h stops after the likelihood at m = 0: the arrays behind v and g are this section's own)
    HIPX(sc.alloc(&c.rowof, N));
    HIPX(hipMemcpyAsync(c.rowof, x.rowof.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
    if (ties) {
      HIPX(sc.alloc(&c.lastk, N));
      HIPX(hipMemcpyAsync(c.lastk, x.lastk.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIPX(sc.alloc(&c.e, N));
    HIPX(sc.alloc(&c.v, N));
    HIPX(sc.alloc(&c.g, N));
    HIPX(sc.alloc(&c.hs, (size_t)cox_surv_workspace(n)));
    HIPX(launch_cox_eval_eta(xp, f32, rs, cs, n, d.cols, m, d.B, d.zero, 1, d.pos, d.eta, d.ex, st));
    HIPX(hipMemcpyAsync(c.e, d.ex, N * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, ties ? d.first : nullptr, n, 1, d.work, c.res, st));
    HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, nullptr, 0, d.eta, c.hs, nullptr, st));
    HIPX(launch_cox_info_vg(c.e, d.eta, ties ? c.lastk : nullptr, d.wd, d.pos, n, c.v, c.g, st));
  }
  HIPX(hipMemcpyAsync(h.data(), c.res, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  // 2. where section 2h's predictor pass is the gathering one, e and what follows it once more from the pass with threads
  // along rows: the same bits under every layout of x
  if (!cox_eval_eta_by_rows(rs, cs, m)) {
    HIPX(sc.alloc(&res2, 2));
    HIPX(launch_cox_eval_eta_rows(xp, f32, rs, cs, n, d.cols, m, d.B, d.zero, d.pos, d.eta, d.ex, st));
    HIPX(hipMemcpyAsync(c.e, d.ex, N * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPX(launch_cox_eval_loglik(d.eta, d.ex, d.wd, ties ? d.first : nullptr, n, 1, d.work, res2, st));
    HIPX(launch_cox_info_gather(xp, f32, rs, cs, n, d.cols, m, c.rowof, c.e, c.W, st));
    HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, nullptr, 0, d.eta, c.hs, nullptr, st));
    HIPX(launch_cox_info_vg(c.e, d.eta, ties ? c.lastk : nullptr, d.wd, d.pos, n, c.v, c.g, st));
    if (c.J > 0) HIPX(launch_cox_info_means(c.W, d.ex, c.jptr, n, m, c.J, c.scr, c.U, c.ldU, st));
  }
  // 3. A (section 2j's launches)
  double *A = nullptr, *dh = nullptr, *scrA = nullptr;
  const long long ldA = cox_diag_lda(n);
  if (m > 0) {
    HIPX(sc.alloc(&A, (size_t)ldA * (size_t)m));
    HIPX(sc.alloc(&dh, N));
    HIPX(sc.alloc(&scrA, nb * (size_t)m));
    HIPX(launch_cox_diag_accum(c.U, c.ldU, c.jptr, d.wd, d.ex, d.first, ties ? c.lastk : nullptr, n, m, dh, scrA, A, ldA,
                               st));
  }
  *A_out = A;
  *ldA_out = ldA;
  return 0;
}

int cox_addscore_run(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, std::vector<double> &pk, std::vector<double> &h,
                     const bessx_cox_addscore_input *in, double *loglik, double *residual_sum, hipStream_t st) {
  const int n = in->n, m = in->m, f32 = in->x_dtype == BESSX_F32, q = in->q, block = in->candidate_block;
  const int ties = in->ties;
  const long long rs = in->x_row_stride, cs = in->x_col_stride;
  const size_t N = (size_t)n, mm = (size_t)m * (size_t)m, M = (size_t)m + 1, Q = (size_t)q;
  const size_t nb = (size_t)((n + 1023) / 1024);
  const bool with_stat = in->factor != nullptr && m > 0, want_c = in->cross != nullptr;
  // 1. to 3. info, score, loglik and residual_sum (the same bits as bessx_cox_info_device), e, v, g by rows, A
  CoxInfoDev c;
  double *A = nullptr;
  long long ldA = 0;
  if (int rc = cox_score_stage(sc, o, x, in->x, f32, rs, cs, n, in->cols, m, in->beta, ties, h, st, c, &A, &ldA)) return rc;
  const CoxDev &d = c.d;
  double *Cc = nullptr, *scrC = nullptr;
  HIPX(sc.alloc(&Cc, N));
  HIPX(sc.alloc(&scrC, nb));
  HIPX(launch_cox_addscore_cc(d.wd, d.ex, d.first, ties ? c.lastk : nullptr, n, scrC, Cc, st));
  // 4. the panel
  long long panel = 0, blk = 0, rps = 0, part_d = 0, rpsq = 0;
  int slabs = 0, cb = 0, depth = 0, slabsq = 0, tdepth = 0;
  addscore_split(n, m, q, block, &panel, &blk, &rps, &slabs, &cb, &depth);
  cox_addscore_split(n, q, block, &part_d, &rpsq, &slabsq, &tdepth);
  int *cand_d = nullptr;
  double *P = nullptr, *work = nullptr, *part = nullptr, *ostage = nullptr;
  HIPX(sc.alloc(&P, (size_t)panel));
  HIPX(sc.alloc(&work, (size_t)blk));
  HIPX(sc.alloc(&part, (size_t)part_d));
  if (in->candidates) {
    HIPX(sc.alloc(&cand_d, Q));
    HIPX(hipMemcpyAsync(cand_d, in->candidates, Q * sizeof(int), hipMemcpyHostToDevice, st));
  }
  HIPX(launch_cox_addscore_pack(in->x, f32, rs, cs, n, d.cols, m, q, block, c.v, c.g, c.e, d.pos, A, ldA, P, st));
  // the score behind r, summed by section 2l's kernels over the support as candidates: the same bits under every
  // layout of x, which section 2h's score is not
  if (with_stat) {
    long long panel0 = 0, blk0 = 0, rps0 = 0;
    int slabs0 = 0, cb0 = 0, depth0 = 0;
    double *work0 = nullptr, *u0 = nullptr;
    addscore_split(n, m, m, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
    HIPX(sc.alloc(&work0, (size_t)blk0));
    HIPX(sc.alloc(&u0, 2 * M));
    HIPX(launch_addscore_blocks(in->x, f32, rs, cs, n, m, d.cols, m, 0, P, work0, 0, u0, u0 + M, nullptr, nullptr, nullptr,
                                0, 0, st));
    HIPX(hipMemcpyAsync(h.data() + 2 + mm + (size_t)m, u0, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  *loglik = h[0];
  *residual_sum = h[1];
  copy_out(h.data() + 2, (size_t)m, (size_t)m, in->info, in->info_ld);
  if (m > 0) copy_out(h.data() + 2 + mm, (size_t)m, 1, in->score, 0);
  if (with_stat) {
    // r = inverse(info) U = R^T (R U) on the host in fp64; the factor gets a zero row and column in front for the panel's
    // column 0 (v), whose cross product has no part in s and a
    const double *U0 = h.data() + 2 + mm + (size_t)m;
    std::vector<double> t((size_t)m, 0.0), Rx(M * M, 0.0), rx(M, 0.0);
    for (size_t j = 0; j < (size_t)m; j++)
      for (size_t k = 0; k <= j; k++) {
        const double f = in->factor[j * in->factor_ld + k];
        t[j] += f * U0[k];
        Rx[(j + 1) * M + k + 1] = f;
      }
    for (size_t j = 0; j < (size_t)m; j++)
      for (size_t k = 0; k <= j; k++) rx[k + 1] += in->factor[j * in->factor_ld + k] * t[j];
    pk.resize((size_t)diag_factor_doubles(m + 1));
    addscore_pack_factor(Rx.data(), (long long)M, rx.data(), m, pk.data());
    HIPX(hipMemcpyAsync(work + blk - (long long)pk.size(), pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice,
                        st));
  }
  // 5. u, c, d, s, a by section 2l's kernels; t by the streaming pass
  double *u = in->u, *dd = in->d, *tt = in->t, *s = in->s, *a = in->a, *C = in->cross;
  long long ldc = in->cross_ld;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&ostage, 5 * Q + (want_c ? Q * M : 0)));
    u = ostage, dd = ostage + Q, tt = ostage + 2 * Q, s = ostage + 3 * Q, a = ostage + 4 * Q;
    C = want_c ? ostage + 5 * Q : nullptr;
    ldc = (long long)M;
  }
  HIPX(launch_addscore_blocks(in->x, f32, rs, cs, n, m, cand_d, q, block, P, work, with_stat ? 1 : 0, u, dd, s, a, C, ldc,
                              0, st));
  HIPX(launch_cox_addscore_quad(in->x, f32, rs, cs, n, cand_d, q, block, c.rowof, c.e, Cc, part, tt, 0, st));
  const bool zero_sa = m == 0 && s && a;  // (the null model: nothing is explained by a support)
  if (zero_sa) {
    HIPX(hipMemsetAsync(s, 0, Q * sizeof(double), st));
    HIPX(hipMemsetAsync(a, 0, Q * sizeof(double), st));
  }
  if (!in->out_on_device) {
    h.resize(5 * Q + (want_c ? Q * M : 0));
    HIPX(hipMemcpyAsync(h.data(), ostage, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) {
    std::copy(h.begin(), h.begin() + Q, in->u);
    std::copy(h.begin() + Q, h.begin() + 2 * Q, in->d);
    std::copy(h.begin() + 2 * Q, h.begin() + 3 * Q, in->t);
    if ((with_stat || m == 0) && in->s && in->a) {
      std::copy(h.begin() + 3 * Q, h.begin() + 4 * Q, in->s);
      std::copy(h.begin() + 4 * Q, h.begin() + 5 * Q, in->a);
    }
    if (want_c) copy_out(h.data() + 5 * Q, M, Q, in->cross, in->cross_ld);
  }
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_addscore_workspace(int n, int m, int n_event_rows, int q, int candidate_block, long long *doubles,
                                 long long *block_doubles, long long *rows_per_slab, int *slabs, int *block,
                                 int *sum_depth, int *chain) {
  if (!doubles || !block_doubles || !rows_per_slab || !slabs || !block || !sum_depth || !chain)
    return fail(BESSX_ERR_ARG, "cox_addscore_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "cox_addscore_workspace: empty matrix");
  if (n_event_rows < 0 || n_event_rows > n)
    return fail(BESSX_ERR_ARG, "cox_addscore_workspace: n_event_rows must lie in [0, n]");
  if (q < 1) return fail(BESSX_ERR_ARG, "cox_addscore_workspace: q must be at least 1");
  if (int rc = addscore_check_block("cox_addscore_workspace", candidate_block)) return rc;
  if (int rc = check_m_max("cox_addscore_workspace", m)) return rc;
  long long panel = 0, blk = 0, part = 0;
  addscore_split(n, m, q, candidate_block, &panel, &blk, &rows_per_slab[0], &slabs[0], block, sum_depth);
  cox_addscore_split(n, q, candidate_block, &part, &rows_per_slab[1], &slabs[1], &chain[1]);
  chain[0] = (int)std::min<long long>(0x7fffffffLL, rows_per_slab[0] + (slabs[0] + 15) / 16 + 4);
  cox_addscore_doubles(n, m, n_event_rows, q, candidate_block, doubles, block_doubles);
  return BESSX_OK;
}

int bessx_cox_addscore_device(const bessx_cox_addscore_input *in, double *loglik, double *n_events,
                              double *residual_sum) {
  if (!in) return fail(BESSX_ERR_ARG, "cox_addscore_device: null argument");
  const CoxCall c = cox_call(in);
  if (int rc = cox_addscore_check_args("cox_addscore_device", c, in, loglik, n_events, residual_sum)) return rc;
  int dev = -1;
  if (int rc = cox_check_device("cox_addscore_device", c, &dev)) return rc;
  if (in->out_on_device) {
    const bool sa = in->factor || in->m == 0;
    double *const vec[5] = {in->u, in->d, in->t, sa ? in->s : nullptr, sa ? in->a : nullptr};
    for (double *v : vec)
      if (v)
        if (int rc = check_on_device("cox_addscore_device", "u, d, t, s, a", v, BESSX_F64, 1, 0, in->q, 1, dev, "an output"))
          return rc;
    if (in->cross)
      if (int rc = check_on_device("cox_addscore_device", "cross", in->cross, BESSX_F64, in->cross_ld, 1, in->q, in->m + 1,
                                   dev))
        return rc;
  }
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  CoxInfoOrder x;
  cox_info_order(&o, in->n, in->m, in->ties, &x);
  const int rc = dev_call(dev, c.stream, [&](DevCall &dc) {
    return cox_addscore_run(dc.sc, o, x, dc.pk, dc.h, in, loglik, residual_sum, dc.st);
  });
  if (!rc) *n_events = x.n_events;
  return rc;
}

int bessx_op_cox_addscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                                const int *cols, int m, const int *candidates, int q, int candidate_block, int sorted,
                                int repeats, double *stage_ms, double *bytes) {
  if (!x || repeats < 1 || !stage_ms || !bytes || q < 1) return fail(BESSX_ERR_ARG, "op_cox_addscore_bench: bad arguments");
  if (int rc = predict_check_model("op_cox_addscore_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_cox_addscore_bench", m)) return rc;
  if (int rc = addscore_check_block("op_cox_addscore_bench", candidate_block)) return rc;
  if (!candidates && q != p) return fail(BESSX_ERR_ARG, "op_cox_addscore_bench: without a candidate list q must be p");
  if (candidates)
    for (int j = 0; j < q; j++)
      if (candidates[j] < 0 || candidates[j] >= p || (j > 0 && candidates[j] <= candidates[j - 1]))
        return fail(BESSX_ERR_ARG, "op_cox_addscore_bench: candidates must be ascending distinct columns of x");
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_addscore_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t M = (size_t)m + 1, Q = (size_t)q, N = (size_t)n;
  long long panel = 0, blk = 0, rps = 0, part_d = 0, rpsq = 0;
  int slabs = 0, cb = 0, depth = 0, slabsq = 0, tdepth = 0;
  addscore_split(n, m, q, candidate_block, &panel, &blk, &rps, &slabs, &cb, &depth);
  cox_addscore_split(n, q, candidate_block, &part_d, &rpsq, &slabsq, &tdepth);
  // n-vectors, an A and a factor of the library's own; positions in a scattered order unless the rows are sorted
  const long long ldA = cox_diag_lda(n);
  std::vector<double> v(N, 0.25), g(N), e(N), Cc(N), Ah((size_t)ldA * (size_t)m, 1.0 / 64.0), R(M * M, 0.0),
      r(M, 1.0 / 128.0), pk((size_t)diag_factor_doubles(m + 1));
  std::vector<int> pos(N), rowof(N);
  for (size_t i = 0; i < N; i++) {
    g[i] = (i % 2) ? -0.5 : 0.5;
    e[i] = 1.0 + (double)(i % 7) / 8.0;
    Cc[i] = (double)(i + 1) / ((double)n * (double)n);
    pos[i] = sorted ? (int)i : (int)(((long long)i * 7919) % n);
    rowof[i] = pos[i];
  }
  for (size_t j = 1; j < M; j++)
    for (size_t k = 1; k <= j; k++) R[j * M + k] = (j == k ? 1.0 : 1.0 / 64.0) / std::sqrt((double)n);
  r[0] = 0.0;
  addscore_pack_factor(R.data(), (long long)M, r.data(), m, pk.data());
  int *cols_d = nullptr, *cand_d = nullptr, *pos_d = nullptr, *rowof_d = nullptr;
  double *v_d = nullptr, *g_d = nullptr, *e_d = nullptr, *Cc_d = nullptr, *A_d = nullptr, *P = nullptr, *work = nullptr,
         *part = nullptr, *out = nullptr;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&pos_d, N));
  HIPX(sc.alloc(&rowof_d, N));
  HIPX(sc.alloc(&v_d, N));
  HIPX(sc.alloc(&g_d, N));
  HIPX(sc.alloc(&e_d, N));
  HIPX(sc.alloc(&Cc_d, N));
  HIPX(sc.alloc(&A_d, Ah.size()));
  HIPX(sc.alloc(&P, (size_t)panel));
  HIPX(sc.alloc(&work, (size_t)blk));
  HIPX(sc.alloc(&part, (size_t)part_d));
  HIPX(sc.alloc(&out, 5 * Q));
  if (m > 0) {
    HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    HIPX(hipMemcpy(A_d, Ah.data(), Ah.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (candidates) {
    HIPX(sc.alloc(&cand_d, Q));
    HIPX(hipMemcpy(cand_d, candidates, Q * sizeof(int), hipMemcpyHostToDevice));
  }
  HIPX(hipMemcpy(pos_d, pos.data(), N * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(rowof_d, rowof.data(), N * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(v_d, v.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(g_d, g.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(e_d, e.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(Cc_d, Cc.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(work + blk - (long long)pk.size(), pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  const int f32 = dtype == BESSX_F32;
  auto run = [&](int stage) -> int {
    const int only = stage == 1 ? 1 : (stage == 4 ? 2 : 3);
    if (stage == 0)
      HIPX(launch_cox_addscore_pack(x, f32, row_stride, col_stride, n, cols_d, m, q, candidate_block, v_d, g_d, e_d, pos_d,
                                    m > 0 ? A_d : nullptr, ldA, P, nullptr));
    else if (stage == 2 || stage == 3)
      HIPX(launch_cox_addscore_quad(x, f32, row_stride, col_stride, n, cand_d, q, candidate_block, rowof_d, e_d, Cc_d,
                                    part, out + 4 * Q, stage - 1, nullptr));
    else
      HIPX(launch_addscore_blocks(x, f32, row_stride, col_stride, n, m, cand_d, q, candidate_block, P, work, 1, out, out + Q,
                                  out + 2 * Q, out + 3 * Q, nullptr, 0, only, nullptr));
    return 0;
  };
  // (each stage over every block of candidates, in an order in which a later stage finds the earlier one's results of
  // the last block)
  for (int stage = 0; stage < 6; stage++) {
    float ms = 0.f;
    if (int rc = bt.run(repeats, &ms, [&]() { return run(stage); })) return rc;
    stage_ms[stage] = ms / repeats;
  }
  *bytes = (double)n * (double)q * (f32 ? 4.0 : 8.0);
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// score tests of groups of candidate columns against one model on a caller's device matrix (include/bessx.h section 2n)
// ----------------------------------------------------------------------------------------------
namespace {

constexpr int GS_WIDTH_MAX = 64;   // columns of a tested group
constexpr int GS_BLOCK = 2048;     // candidates per block unless the caller asks for fewer (AS_BLOCK)

// the tested columns and how they are cut: everything about a call that follows from (starts, groups, candidate_block)
struct GsPlan {
  std::vector<int> cand, lpos, width, first;  // tested columns; list position of each tested group (+ q); widths; blocks
  std::vector<long long> offs;                // where each tested group's d x d block starts (+ the total)
  int nt = 0, q = 0, dmax = 0, band = 0, blocks = 0, qmax = 0, block = 0;
};

int groupscore_plan(const std::string &w, int p, const int *starts, int G, const int *groups, int n_tested, int block,
                    GsPlan *pl) {
  if (!starts || G < 1) return fail(BESSX_ERR_ARG, w + ": group_starts must hold at least one group");
  if (starts[0] != 0) return fail(BESSX_ERR_ARG, w + ": group_starts must begin with column 0");
  for (int g = 1; g < G; g++)
    if (starts[g] <= starts[g - 1]) return fail(BESSX_ERR_ARG, w + ": group_starts must be ascending and distinct");
  if (starts[G - 1] >= p) return fail(BESSX_ERR_ARG, w + ": a group start is not a column of x");
  pl->nt = groups ? n_tested : G;
  if (pl->nt < 1) return fail(BESSX_ERR_ARG, w + ": n_tested must be at least 1");
  if (groups)
    for (int t = 0; t < pl->nt; t++) {
      if (groups[t] < 0 || groups[t] >= G) return fail(BESSX_ERR_ARG, w + ": a tested group is not a group of the partition");
      if (t > 0 && groups[t] <= groups[t - 1]) return fail(BESSX_ERR_ARG, w + ": groups must be ascending and distinct");
    }
  if (int rc = addscore_check_block(w, block)) return rc;
  pl->block = block > 0 ? block : GS_BLOCK;
  pl->width.resize((size_t)pl->nt);
  pl->lpos.assign((size_t)pl->nt + 1, 0);
  pl->offs.assign((size_t)pl->nt + 1, 0);
  pl->cand.clear();
  for (int t = 0; t < pl->nt; t++) {
    const int g = groups ? groups[t] : t, c0 = starts[g], c1 = g + 1 < G ? starts[g + 1] : p, d = c1 - c0;
    if (d > GS_WIDTH_MAX)
      return fail(BESSX_ERR_UNSUPPORTED, w + ": group " + std::to_string(g) + " has " + std::to_string(d) +
                                             " columns; a tested group may have at most " + std::to_string(GS_WIDTH_MAX));
    pl->width[(size_t)t] = d;
    pl->dmax = std::max(pl->dmax, d);
    pl->lpos[(size_t)t + 1] = pl->lpos[(size_t)t] + d;
    pl->offs[(size_t)t + 1] = pl->offs[(size_t)t] + (long long)d * d;
    for (int c = c0; c < c1; c++) pl->cand.push_back(c);
  }
  pl->q = pl->lpos[(size_t)pl->nt];
  if (pl->block < (pl->dmax + 15) / 16 * 16)
    return fail(BESSX_ERR_ARG, w + ": candidate_block must be at least the widest tested group rounded up to 16 (" +
                                   std::to_string((pl->dmax + 15) / 16 * 16) + ")");
  pl->band = groupscore_band(pl->dmax);
  pl->first.assign((size_t)pl->nt + 1, 0);
  pl->blocks = groupscore_cut(pl->width.data(), pl->nt, pl->block, pl->first.data());
  pl->first.resize((size_t)pl->blocks + 1);
  for (int b = 0; b < pl->blocks; b++)
    pl->qmax = std::max(pl->qmax, pl->lpos[(size_t)pl->first[(size_t)b + 1]] - pl->lpos[(size_t)pl->first[(size_t)b]]);
  return 0;
}

// section 2l's block workspace for the blocks of a plan (the largest over the blocks) and the longest chain of additions
// behind an entry of u or C
void groupscore_cross_figures(long long n, int m, const GsPlan &pl, long long *work, long long *rps_max, int *slabs_at,
                              int *chain) {
  *work = 0, *rps_max = 0, *slabs_at = 0, *chain = 0;
  for (int b = 0; b < pl.blocks; b++) {
    const int qb = pl.lpos[(size_t)pl.first[(size_t)b + 1]] - pl.lpos[(size_t)pl.first[(size_t)b]];
    long long panel = 0, blk = 0, rps = 0;
    int slabs = 0, cb = 0, depth = 0;
    addscore_split(n, m, qb, pl.block, &panel, &blk, &rps, &slabs, &cb, &depth);
    *work = std::max(*work, blk);
    const int ch = (int)std::min<long long>(0x7fffffffLL, rps + (slabs + 15) / 16 + 4);
    if (ch > *chain) *chain = ch, *rps_max = rps, *slabs_at = slabs;
  }
}

// everything about the call that needs no device
int groupscore_check_args(const char *who, const GlmCall &c, const bessx_groupscore_input *in, const double *loss,
                          const double *sum_w, GsPlan *pl) {
  const std::string w(who);
  if (int rc = info_check_args(who, c, in->info, in->info_ld, in->score, loss, sum_w)) return rc;
  if (!in->u || !in->D || !in->offsets) return fail(BESSX_ERR_ARG, w + ": null argument (u, D, offsets)");
  if (in->factor && (!in->S || !in->a)) return fail(BESSX_ERR_ARG, w + ": null argument (S, a)");
  if (int rc = groupscore_plan(w, in->p, in->group_starts, in->n_groups, in->groups, in->n_tested, in->candidate_block, pl))
    return rc;
  if (in->factor) {
    if (in->factor_ld < (long long)in->m + 1) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m + 1");
    for (long long j = 0; j <= in->m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  return 0;
}

// the device arrays of the blocks' loop
struct GsDev {
  const void *x;
  int f32;
  long long rs, cs, n;
  int m;
  int *cand, *lpos;
  long long *offs;
  double *v, *P, *work_as, *work_gs, *dd;  // row weights, the panel, section 2l's and this section's block workspace
};

// stage: 0 = everything, else ONE step over every block (bessx_op_groupscore_bench): 1 = the cross product, 2 = the
// addition of its partials, 3 = the Gram band, 4 = the addition of its partials, 5 = T, the band of S and a, 6 = the
// extraction of D and S.  with_s: the factor is packed in work_gs's tail.  u, a: q doubles; D, S: offs[nt] doubles.
int groupscore_blocks(const GsPlan &pl, const GsDev &d, int with_s, double *u, double *a, double *D, double *S, int stage,
                      hipStream_t st) {
  const int M = d.m + 1, Mp = 16 * ((M + 1 + 15) / 16), NT = pl.band + 1;
  long long rps = 0;
  int slabs = 0;
  groupscore_rows(d.n, &rps, &slabs);
  const long long trm = (pl.qmax + 15) / 16;
  // groupscore_doubles' layout for the largest block: partials and band of D (launch_groupscore_gram puts a block's
  // band right behind that block's partials), band of S, the block's rows of C and of T, the packed factor
  double *bandS = d.work_gs + (slabs + 1) * trm * NT * 256, *Cb = bandS + trm * NT * 256, *Tb = Cb + trm * 16 * Mp,
         *pk = Tb + trm * 16 * Mp;
  for (int b = 0; b < pl.blocks; b++) {
    const int g0 = pl.first[(size_t)b], g1 = pl.first[(size_t)b + 1], j0 = pl.lpos[(size_t)g0], qb = pl.lpos[(size_t)g1] - j0;
    const long long trb = (qb + 15) / 16;
    // u and the block's rows of C (leading dimension Mp; what k_as_finish does not write stays zero)
    if (stage == 0 || stage == 1) HIPX(hipMemsetAsync(Cb, 0, (size_t)(trb * 16 * Mp) * sizeof(double), st));
    if (stage <= 2)
      HIPX(launch_addscore_blocks(d.x, d.f32, d.rs, d.cs, d.n, d.m, d.cand + j0, qb, pl.block, d.P, d.work_as, 0, u + j0, d.dd,
                                  nullptr, nullptr, Cb, (long long)Mp, stage, st));
    if (stage == 0 || stage == 3 || stage == 4)
      HIPX(launch_groupscore_gram(d.x, d.f32, d.rs, d.cs, d.n, d.cand + j0, qb, pl.band, d.v, d.work_gs,
                                  stage == 0 ? 0 : stage - 2, st));
    if (with_s && (stage == 0 || stage == 5))
      HIPX(launch_groupscore_sband(Cb, d.m, qb, pl.band, pk, Tb, bandS, a + j0, st));
    if (stage == 0 || stage == 6) {
      HIPX(launch_groupscore_extract(d.work_gs + (long long)slabs * trb * NT * 256, pl.band, d.lpos, d.offs, g0, g1 - g0, D,
                                     st));
      if (with_s) HIPX(launch_groupscore_extract(bandS, pl.band, d.lpos, d.offs, g0, g1 - g0, S, st));
    }
  }
  return 0;
}

// the lists of a plan in device memory
int groupscore_upload_plan(Owner &sc, const GsPlan &pl, hipStream_t st, GsDev *d) {
  HIPX(sc.alloc(&d->cand, (size_t)pl.q));
  HIPX(sc.alloc(&d->lpos, pl.lpos.size()));
  HIPX(sc.alloc(&d->offs, pl.offs.size()));
  HIPX(hipMemcpyAsync(d->cand, pl.cand.data(), (size_t)pl.q * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->lpos, pl.lpos.data(), pl.lpos.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(d->offs, pl.offs.data(), pl.offs.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  return 0;
}

int groupscore_run(Owner &sc, const GsPlan &pl, std::vector<double> &pk, std::vector<double> &h, const GlmCall &c,
                   const bessx_groupscore_input *in, double *loss, double *sum_w, hipStream_t st) {
  const int f32 = in->x_dtype == BESSX_F32, m = in->m;
  const long long n = in->n, nv = (n + 1) / 2 * 2;
  const size_t M = (size_t)m + 1, Q = (size_t)pl.q, TOT = (size_t)pl.offs[(size_t)pl.nt];
  const bool with_s = in->factor != nullptr;
  long long panel = 0, blk = 0, rps = 0, work_as = 0, rpsx = 0;
  int slabs = 0, cb = 0, depth = 0, slabsx = 0, chain = 0;
  addscore_split(n, m, pl.qmax, pl.block, &panel, &blk, &rps, &slabs, &cb, &depth);
  groupscore_cross_figures(n, m, pl, &work_as, &rpsx, &slabsx, &chain);
  const long long work_gs = groupscore_doubles(n, m, pl.qmax, pl.band);
  int *cols_d = nullptr;
  double *B_d = nullptr, *c_d = nullptr, *iwork = nullptr, *res = nullptr, *istage = nullptr, *vg = nullptr,
         *ostage = nullptr;
  GsDev d{};
  d.x = in->x, d.f32 = f32, d.rs = in->x_row_stride, d.cs = in->x_col_stride, d.n = n, d.m = m;
  if (int rc = predict_upload_model(sc, in->cols, m, in->beta, &in->coef0, 1, st, &cols_d, &B_d, &c_d)) return rc;
  EvalData ed;
  if (int rc = eval_stage_data(sc, c, st, &ed)) return rc;
  // 1. info, score, loss and sum_w: launch_info as bessx_info_device runs it (the same bits)
  HIPX(sc.alloc(&iwork, (size_t)info_workspace(f32, in->x_row_stride, in->x_col_stride, in->n, m, in->link,
                                                ed.w != nullptr)));
  HIPX(sc.alloc(&res, 3));
  HIPX(sc.alloc(&istage, M * M + M));
  HIPX(launch_info(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, B_d, c_d, in->link, ed, iwork, res, istage,
                   (long long)M, istage + M * M, st));
  h.resize(3 + M * M + 2 * M);
  HIPX(hipMemcpyAsync(h.data(), res, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipMemcpyAsync(h.data() + 3, istage, (M * M + M) * sizeof(double), hipMemcpyDeviceToHost, st));
  // 2. the row weights, always by rows, and section 2l's panel
  HIPX(sc.alloc(&vg, (size_t)(2 * nv)));
  HIPX(launch_info_vg(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, B_d, c_d, in->link, ed, vg, vg + nv,
                      st));
  d.v = vg;
  HIPX(sc.alloc(&d.P, (size_t)panel));
  HIPX(sc.alloc(&d.work_as, (size_t)work_as));
  HIPX(sc.alloc(&d.work_gs, (size_t)work_gs));
  HIPX(sc.alloc(&d.dd, (size_t)(pl.qmax + 15) / 16 * 16));
  if (int rc = groupscore_upload_plan(sc, pl, st, &d)) return rc;
  HIPX(launch_addscore_pack(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, pl.qmax, pl.block, vg, vg + nv,
                            d.P, st));
  // the score behind r, summed by section 2l's kernels over the list (constant column, support), as section 2l does
  std::vector<int> cand0;
  double *u0 = nullptr;
  if (with_s) {
    long long panel0 = 0, blk0 = 0, rps0 = 0;
    int slabs0 = 0, cb0 = 0, depth0 = 0, *cand0_d = nullptr;
    double *work0 = nullptr;
    addscore_split(n, m, (int)M, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
    cand0.assign(M, -1);
    std::copy(in->cols, in->cols + m, cand0.begin() + 1);
    HIPX(sc.alloc(&cand0_d, M));
    HIPX(sc.alloc(&work0, (size_t)blk0));
    HIPX(sc.alloc(&u0, 2 * M));
    HIPX(hipMemcpyAsync(cand0_d, cand0.data(), M * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(launch_addscore_blocks(in->x, f32, in->x_row_stride, in->x_col_stride, n, m, cand0_d, (int)M, 0, d.P, work0, 0, u0,
                                u0 + M, nullptr, nullptr, nullptr, 0, 0, st));
    HIPX(hipMemcpyAsync(h.data() + 3 + M * M + M, u0, M * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  *loss = h[0];
  *sum_w = ed.w ? h[2] : (double)in->n;
  copy_out(h.data() + 3, M, M, in->info, in->info_ld);
  copy_out(h.data() + 3 + M * M, M, 1, in->score, 0);
  if (with_s) {
    // r = inverse(info) U = R^T (R U), on the host in fp64
    const double *U0 = h.data() + 3 + M * M + M;
    std::vector<double> t(M, 0.0), r(M, 0.0);
    for (size_t j = 0; j < M; j++)
      for (size_t k = 0; k <= j; k++) t[j] += in->factor[j * in->factor_ld + k] * U0[k];
    for (size_t j = 0; j < M; j++)
      for (size_t k = 0; k <= j; k++) r[k] += in->factor[j * in->factor_ld + k] * t[j];
    pk.resize((size_t)diag_factor_doubles(m + 1));
    addscore_pack_factor(in->factor, in->factor_ld, r.data(), m, pk.data());
    HIPX(hipMemcpyAsync(d.work_gs + work_gs - (long long)pk.size(), pk.data(), pk.size() * sizeof(double),
                        hipMemcpyHostToDevice, st));
  }
  double *u = in->u, *a = in->a, *D = in->D, *S = in->S;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&ostage, 2 * Q + 2 * TOT));
    u = ostage, a = ostage + Q, D = ostage + 2 * Q, S = D + TOT;
  }
  if (int rc = groupscore_blocks(pl, d, with_s ? 1 : 0, u, a, D, S, 0, st)) return rc;
  if (!in->out_on_device) {
    h.resize(2 * Q + 2 * TOT);
    HIPX(hipMemcpyAsync(h.data(), ostage, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) {
    std::copy(h.begin(), h.begin() + Q, in->u);
    std::copy(h.begin() + 2 * Q, h.begin() + 2 * Q + TOT, in->D);
    if (with_s) {
      std::copy(h.begin() + Q, h.begin() + 2 * Q, in->a);
      std::copy(h.begin() + 2 * Q + TOT, h.begin() + 2 * Q + 2 * TOT, in->S);
    }
  }
  std::copy(pl.offs.begin(), pl.offs.end(), in->offsets);
  return 0;
}

}  // namespace

extern "C" {

int bessx_groupscore_workspace(int n, int p, int m, const int *group_starts, int n_groups, const int *groups,
                               int n_tested, int candidate_block, long long *doubles, long long *block_doubles,
                               long long *rows_per_slab, int *slabs, int *n_blocks, int *block_first, int *band,
                               int *depth) {
  if (!doubles || !block_doubles || !rows_per_slab || !slabs || !n_blocks || !band || !depth)
    return fail(BESSX_ERR_ARG, "groupscore_workspace: null argument");
  if (n < 1 || p < 1 || m < 0) return fail(BESSX_ERR_ARG, "groupscore_workspace: empty matrix");
  if (int rc = check_m_max("groupscore_workspace", m)) return rc;
  GsPlan pl;
  if (int rc = groupscore_plan("groupscore_workspace", p, group_starts, n_groups, groups, n_tested, candidate_block, &pl))
    return rc;
  long long panel = 0, blk = 0, rps = 0, work_as = 0;
  int sl = 0, cb = 0, dp = 0;
  addscore_split(n, m, pl.qmax, pl.block, &panel, &blk, &rps, &sl, &cb, &dp);
  groupscore_cross_figures(n, m, pl, &work_as, &rows_per_slab[0], &slabs[0], &depth[0]);
  groupscore_rows(n, &rows_per_slab[1], &slabs[1]);
  // (plus the block workspace of the score behind r, whose candidates are the constant column and the support)
  long long panel0 = 0, blk0 = 0, rps0 = 0;
  int slabs0 = 0, cb0 = 0, depth0 = 0;
  addscore_split(n, m, m + 1, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
  depth[1] = (int)std::min<long long>(0x7fffffffLL, rps0 + (slabs0 + 15) / 16 + 4);
  depth[2] = (int)std::min<long long>(0x7fffffffLL, rows_per_slab[1] + slabs[1]);
  depth[3] = 16 * ((m + 2 + 15) / 16);
  *block_doubles = work_as + groupscore_doubles(n, m, pl.qmax, pl.band) + (pl.qmax + 15) / 16 * 16 + blk0 +
                   2 * ((long long)m + 1);
  *doubles = 2 * (((long long)n + 1) / 2 * 2) + panel + *block_doubles;
  *n_blocks = pl.blocks;
  *band = pl.band;
  if (block_first) std::copy(pl.first.begin(), pl.first.end(), block_first);
  return BESSX_OK;
}

int bessx_groupscore_device(const bessx_groupscore_input *in, double *loss, double *sum_w) {
  if (!in) return fail(BESSX_ERR_ARG, "groupscore_device: null argument");
  const GlmCall c = glm_call(in);
  GsPlan pl;
  if (int rc = groupscore_check_args("groupscore_device", c, in, loss, sum_w, &pl)) return rc;
  int dev = -1;
  if (int rc = glm_check_device("groupscore_device", c, &dev)) return rc;
  if (in->out_on_device) {
    const long long tot = pl.offs[(size_t)pl.nt];
    double *const vec[4] = {in->u, in->factor ? in->a : nullptr, in->D, in->factor ? in->S : nullptr};
    const long long len[4] = {pl.q, pl.q, tot, tot};
    for (int k = 0; k < 4; k++) {
      if (!vec[k]) continue;
      if (len[k] > 0x7fffffffLL) return fail(BESSX_ERR_ARG, "groupscore_device: too many block entries for device output");
      if (int rc = check_on_device("groupscore_device", "u, a, D, S", vec[k], BESSX_F64, 1, 0, (int)len[k], 1, dev,
                                   "an output"))
        return rc;
    }
  }
  return dev_call(dev, c.stream,
                  [&](DevCall &dc) { return groupscore_run(dc.sc, pl, dc.pk, dc.h, c, in, loss, sum_w, dc.st); });
}

int bessx_op_groupscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                              const int *cols, int m, const int *group_starts, int n_groups, const int *groups,
                              int n_tested, int candidate_block, int repeats, double *stage_ms) {
  if (!x || repeats < 1 || !stage_ms) return fail(BESSX_ERR_ARG, "op_groupscore_bench: bad arguments");
  if (int rc = predict_check_model("op_groupscore_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_groupscore_bench", m)) return rc;
  GsPlan pl;
  if (int rc = groupscore_plan("op_groupscore_bench", p, group_starts, n_groups, groups, n_tested, candidate_block, &pl))
    return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_groupscore_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t M = (size_t)m + 1, Q = (size_t)pl.q, TOT = (size_t)pl.offs[(size_t)pl.nt];
  long long panel = 0, blk = 0, rps = 0, work_as = 0, rpsx = 0;
  int slabs = 0, cb = 0, depth = 0, slabsx = 0, chain = 0;
  addscore_split(n, m, pl.qmax, pl.block, &panel, &blk, &rps, &slabs, &cb, &depth);
  groupscore_cross_figures(n, m, pl, &work_as, &rpsx, &slabsx, &chain);
  const long long work_gs = groupscore_doubles(n, m, pl.qmax, pl.band);
  // row weights and a factor of the library's own, as bessx_op_addscore_bench has them
  std::vector<double> v((size_t)n, 0.25), g((size_t)n), R(M * M, 0.0), r(M, 1.0 / 128.0),
      pk((size_t)diag_factor_doubles(m + 1));
  for (size_t i = 0; i < g.size(); i++) g[i] = (i % 2) ? -0.5 : 0.5;
  for (size_t j = 0; j < M; j++)
    for (size_t k = 0; k <= j; k++) R[j * M + k] = (j == k ? 1.0 : 1.0 / 64.0) / std::sqrt((double)n);
  addscore_pack_factor(R.data(), (long long)M, r.data(), m, pk.data());
  int *cols_d = nullptr;
  double *g_d = nullptr, *out = nullptr;
  GsDev d{};
  d.x = x, d.f32 = dtype == BESSX_F32, d.rs = row_stride, d.cs = col_stride, d.n = n, d.m = m;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&d.v, v.size()));
  HIPX(sc.alloc(&g_d, g.size()));
  HIPX(sc.alloc(&d.P, (size_t)panel));
  HIPX(sc.alloc(&d.work_as, (size_t)work_as));
  HIPX(sc.alloc(&d.work_gs, (size_t)work_gs));
  HIPX(sc.alloc(&d.dd, (size_t)(pl.qmax + 15) / 16 * 16));
  HIPX(sc.alloc(&out, 2 * Q + 2 * TOT));
  if (int rc = groupscore_upload_plan(sc, pl, nullptr, &d)) return rc;
  if (m > 0) HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(d.v, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(g_d, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(d.work_gs + work_gs - (long long)pk.size(), pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  auto run = [&](int stage) -> int {
    if (stage == 0) {
      HIPX(launch_addscore_pack(x, d.f32, row_stride, col_stride, n, cols_d, m, pl.qmax, pl.block, d.v, g_d, d.P, nullptr));
      return 0;
    }
    return groupscore_blocks(pl, d, 1, out, out + Q, out + 2 * Q, out + 2 * Q + TOT, stage, nullptr);
  };
  // (stage 0 = pack, then groupscore_blocks' steps 1 .. 6, each over every block, in an order in which a later stage
  // finds the earlier one's results of the last block)
  for (int stage = 0; stage < 7; stage++) {
    float ms = 0.f;
    if (int rc = bt.run(repeats, &ms, [&]() { return run(stage); })) return rc;
    stage_ms[stage] = ms / repeats;
  }
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// score tests of groups of candidate columns against one Cox model on a caller's device matrix (include/bessx.h section 2o)
// ----------------------------------------------------------------------------------------------
namespace {

// everything about the call that needs no device
int cox_groupscore_check_args(const char *who, const CoxCall &c, const bessx_cox_groupscore_input *in,
                              const double *loglik, const double *n_events, const double *residual_sum, GsPlan *pl) {
  const std::string w(who);
  if (int rc = cox_info_check_args(who, c, in->info, in->info_ld, in->score, loglik, n_events, residual_sum)) return rc;
  if (!in->u || !in->D || !in->T || !in->offsets) return fail(BESSX_ERR_ARG, w + ": null argument (u, D, T, offsets)");
  if (in->factor && (!in->S || !in->a)) return fail(BESSX_ERR_ARG, w + ": null argument (S, a)");
  if (int rc = groupscore_plan(w, in->p, in->group_starts, in->n_groups, in->groups, in->n_tested, in->candidate_block, pl))
    return rc;
  if (in->factor && in->m > 0) {
    if (in->factor_ld < (long long)in->m) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m");
    for (long long j = 0; j < in->m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  return 0;
}

// doubles of device scratch of one call beyond section 2h's, and the part of them that does not depend on p
void cox_groupscore_figures(long long n, int m, long long J, const GsPlan &pl, long long *all, long long *blockpart) {
  const long long nb = (n + 1023) / 1024, M = (long long)m + 1;
  long long panel = 0, blk = 0, rps = 0, work_as = 0, rpsx = 0;
  int slabs = 0, cb = 0, depth = 0, slabsx = 0, chain = 0;
  addscore_split(n, m, pl.qmax, pl.block, &panel, &blk, &rps, &slabs, &cb, &depth);
  groupscore_cross_figures(n, m, pl, &work_as, &rpsx, &slabsx, &chain);
  long long d = cox_info_doubles(n, m, J) + (long long)m * m + m + 2;
  if (m == 0) d += 3 * n + cox_surv_workspace(n);  // e, v, g and the totals of H's scan, which section 2h skips at m = 0
  if (m > 0) d += cox_diag_lda(n) * m + n + nb * m;  // A, dh, A's totals
  long long bp = work_as + groupscore_doubles(n, m, pl.qmax, pl.band) + (pl.qmax + 15) / 16 * 16 +
                 cox_groupscore_doubles(n, pl.qmax, pl.band);
  if (m > 0) {  // the score behind r: the support as candidates
    long long panel0 = 0, blk0 = 0, rps0 = 0;
    int slabs0 = 0, cb0 = 0, depth0 = 0;
    addscore_split(n, m, m, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
    bp += blk0 + 2 * M;
  }
  *all = d + n + panel + bp;  // cc, the panel, the block workspaces
  *blockpart = bp;
}

// the device arrays of the risk-set term
struct CgsDev {
  int *rowof;
  double *e, *cc, *work;
};

// the band of T of every block and its groups' blocks.  stage: 0 = both kernels and the extraction, 1 = k_cgs_band, 2 =
// k_cgs_finish and the extraction (bessx_op_cox_groupscore_bench)
int cox_groupscore_tblocks(const GsPlan &pl, const GsDev &d, const CgsDev &t, double *T, int stage, hipStream_t st) {
  for (int b = 0; b < pl.blocks; b++) {
    const int g0 = pl.first[(size_t)b], g1 = pl.first[(size_t)b + 1], j0 = pl.lpos[(size_t)g0], qb = pl.lpos[(size_t)g1] - j0;
    double *bandT = nullptr;
    HIPX(launch_cox_groupscore_tband(d.x, d.f32, d.rs, d.cs, d.n, d.cand + j0, qb, pl.band, t.rowof, t.e, t.cc, t.work, stage,
                                     &bandT, st));
    if (stage == 0 || stage == 2) HIPX(launch_groupscore_extract(bandT, pl.band, d.lpos, d.offs, g0, g1 - g0, T, st));
  }
  return 0;
}

int cox_groupscore_run(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const GsPlan &pl, std::vector<double> &pk,
                       std::vector<double> &h, const bessx_cox_groupscore_input *in, double *loglik, double *residual_sum,
                       hipStream_t st) {
  const int n = in->n, m = in->m, f32 = in->x_dtype == BESSX_F32, ties = in->ties;
  const long long rs = in->x_row_stride, cs = in->x_col_stride;
  const size_t N = (size_t)n, mm = (size_t)m * (size_t)m, M = (size_t)m + 1, Q = (size_t)pl.q,
               TOT = (size_t)pl.offs[(size_t)pl.nt];
  const bool with_s = in->factor != nullptr && m > 0;
  // 1. to 3. info, score, loglik and residual_sum (the same bits as bessx_cox_info_device), e, v, g by rows, A: section
  // 2m's steps; then cc
  CoxInfoDev c;
  double *A = nullptr;
  long long ldA = 0;
  if (int rc = cox_score_stage(sc, o, x, in->x, f32, rs, cs, n, in->cols, m, in->beta, ties, h, st, c, &A, &ldA)) return rc;
  const CoxDev &cd = c.d;
  CgsDev t{};
  t.rowof = c.rowof, t.e = c.e;
  HIPX(sc.alloc(&t.cc, N));
  HIPX(launch_cox_groupscore_cc(cd.wd, cd.ex, cd.first, ties ? c.lastk : nullptr, n, t.cc, st));
  // 4. section 2m's panel and section 2n's block workspaces
  long long panel = 0, blk = 0, rps = 0, work_as = 0, rpsx = 0;
  int slabs = 0, cb = 0, depth = 0, slabsx = 0, chain = 0;
  addscore_split(n, m, pl.qmax, pl.block, &panel, &blk, &rps, &slabs, &cb, &depth);
  groupscore_cross_figures(n, m, pl, &work_as, &rpsx, &slabsx, &chain);
  const long long work_gs = groupscore_doubles(n, m, pl.qmax, pl.band);
  GsDev d{};
  d.x = in->x, d.f32 = f32, d.rs = rs, d.cs = cs, d.n = n, d.m = m, d.v = c.v;
  double *ostage = nullptr;
  HIPX(sc.alloc(&d.P, (size_t)panel));
  HIPX(sc.alloc(&d.work_as, (size_t)work_as));
  HIPX(sc.alloc(&d.work_gs, (size_t)work_gs));
  HIPX(sc.alloc(&d.dd, (size_t)(pl.qmax + 15) / 16 * 16));
  HIPX(sc.alloc(&t.work, (size_t)cox_groupscore_doubles(n, pl.qmax, pl.band)));
  if (int rc = groupscore_upload_plan(sc, pl, st, &d)) return rc;
  HIPX(launch_cox_addscore_pack(in->x, f32, rs, cs, n, cd.cols, m, pl.qmax, pl.block, c.v, c.g, c.e, cd.pos, A, ldA, d.P, st));
  // the score behind r, summed by section 2l's kernels over the support as candidates (section 2m's step)
  if (with_s) {
    long long panel0 = 0, blk0 = 0, rps0 = 0;
    int slabs0 = 0, cb0 = 0, depth0 = 0;
    double *work0 = nullptr, *u0 = nullptr;
    addscore_split(n, m, m, 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
    HIPX(sc.alloc(&work0, (size_t)blk0));
    HIPX(sc.alloc(&u0, 2 * M));
    HIPX(launch_addscore_blocks(in->x, f32, rs, cs, n, m, cd.cols, m, 0, d.P, work0, 0, u0, u0 + M, nullptr, nullptr, nullptr,
                                0, 0, st));
    HIPX(hipMemcpyAsync(h.data() + 2 + mm + (size_t)m, u0, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  *loglik = h[0];
  *residual_sum = h[1];
  copy_out(h.data() + 2, (size_t)m, (size_t)m, in->info, in->info_ld);
  if (m > 0) copy_out(h.data() + 2 + mm, (size_t)m, 1, in->score, 0);
  if (with_s) {
    // r = inverse(info) U = R^T (R U) on the host in fp64; the factor gets section 2m's zero row and column in front
    const double *U0 = h.data() + 2 + mm + (size_t)m;
    std::vector<double> tt((size_t)m, 0.0), Rx(M * M, 0.0), rx(M, 0.0);
    for (size_t j = 0; j < (size_t)m; j++)
      for (size_t k = 0; k <= j; k++) {
        const double f = in->factor[j * in->factor_ld + k];
        tt[j] += f * U0[k];
        Rx[(j + 1) * M + k + 1] = f;
      }
    for (size_t j = 0; j < (size_t)m; j++)
      for (size_t k = 0; k <= j; k++) rx[k + 1] += in->factor[j * in->factor_ld + k] * tt[j];
    pk.resize((size_t)diag_factor_doubles(m + 1));
    addscore_pack_factor(Rx.data(), (long long)M, rx.data(), m, pk.data());
    HIPX(hipMemcpyAsync(d.work_gs + work_gs - (long long)pk.size(), pk.data(), pk.size() * sizeof(double),
                        hipMemcpyHostToDevice, st));
  }
  // 5. u, C, D, S, a by sections 2l's and 2n's kernels; T by this section's
  double *u = in->u, *a = in->a, *D = in->D, *T = in->T, *S = in->S;
  if (!in->out_on_device) {
    HIPX(sc.alloc(&ostage, 2 * Q + 3 * TOT));
    u = ostage, a = ostage + Q, D = ostage + 2 * Q, T = D + TOT, S = T + TOT;
  }
  if (int rc = groupscore_blocks(pl, d, with_s ? 1 : 0, u, a, D, S, 0, st)) return rc;
  if (int rc = cox_groupscore_tblocks(pl, d, t, T, 0, st)) return rc;
  const bool zero_sa = m == 0 && S && a;  // (the null model: nothing is explained by a support)
  if (zero_sa) {
    HIPX(hipMemsetAsync(S, 0, TOT * sizeof(double), st));
    HIPX(hipMemsetAsync(a, 0, Q * sizeof(double), st));
  }
  if (!in->out_on_device) {
    h.resize(2 * Q + 3 * TOT);
    HIPX(hipMemcpyAsync(h.data(), ostage, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPX(hipStreamSynchronize(st));
  if (!in->out_on_device) {
    std::copy(h.begin(), h.begin() + Q, in->u);
    std::copy(h.begin() + 2 * Q, h.begin() + 2 * Q + TOT, in->D);
    std::copy(h.begin() + 2 * Q + TOT, h.begin() + 2 * Q + 2 * TOT, in->T);
    if ((with_s || m == 0) && in->S && in->a) {
      std::copy(h.begin() + Q, h.begin() + 2 * Q, in->a);
      std::copy(h.begin() + 2 * Q + 2 * TOT, h.begin() + 2 * Q + 3 * TOT, in->S);
    }
  }
  std::copy(pl.offs.begin(), pl.offs.end(), in->offsets);
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_groupscore_workspace(int n, int p, int m, int n_event_rows, const int *group_starts, int n_groups,
                                   const int *groups, int n_tested, int candidate_block, long long *doubles,
                                   long long *block_doubles, long long *rows_per_slab, int *slabs, int *n_blocks,
                                   int *block_first, int *band, int *depth) {
  if (!doubles || !block_doubles || !rows_per_slab || !slabs || !n_blocks || !band || !depth)
    return fail(BESSX_ERR_ARG, "cox_groupscore_workspace: null argument");
  if (n < 1 || p < 1 || m < 0) return fail(BESSX_ERR_ARG, "cox_groupscore_workspace: empty matrix");
  if (n_event_rows < 0 || n_event_rows > n)
    return fail(BESSX_ERR_ARG, "cox_groupscore_workspace: n_event_rows must lie in [0, n]");
  if (int rc = check_m_max("cox_groupscore_workspace", m)) return rc;
  GsPlan pl;
  if (int rc = groupscore_plan("cox_groupscore_workspace", p, group_starts, n_groups, groups, n_tested, candidate_block,
                               &pl))
    return rc;
  long long work_as = 0;
  groupscore_cross_figures(n, m, pl, &work_as, &rows_per_slab[0], &slabs[0], &depth[0]);
  groupscore_rows(n, &rows_per_slab[1], &slabs[1]);
  cox_groupscore_rows(n, &rows_per_slab[2], &slabs[2], &depth[4]);
  long long panel0 = 0, blk0 = 0, rps0 = 0;
  int slabs0 = 0, cb0 = 0, depth0 = 0;
  addscore_split(n, m, std::max(m, 1), 0, &panel0, &blk0, &rps0, &slabs0, &cb0, &depth0);
  depth[1] = (int)std::min<long long>(0x7fffffffLL, rps0 + (slabs0 + 15) / 16 + 4);
  depth[2] = (int)std::min<long long>(0x7fffffffLL, rows_per_slab[1] + slabs[1]);
  depth[3] = 16 * ((m + 2 + 15) / 16);
  cox_groupscore_figures(n, m, n_event_rows, pl, doubles, block_doubles);
  *n_blocks = pl.blocks;
  *band = pl.band;
  if (block_first) std::copy(pl.first.begin(), pl.first.end(), block_first);
  return BESSX_OK;
}

int bessx_cox_groupscore_device(const bessx_cox_groupscore_input *in, double *loglik, double *n_events,
                                double *residual_sum) {
  if (!in) return fail(BESSX_ERR_ARG, "cox_groupscore_device: null argument");
  const CoxCall c = cox_call(in);
  GsPlan pl;
  if (int rc = cox_groupscore_check_args("cox_groupscore_device", c, in, loglik, n_events, residual_sum, &pl)) return rc;
  int dev = -1;
  if (int rc = cox_check_device("cox_groupscore_device", c, &dev)) return rc;
  if (in->out_on_device) {
    const long long tot = pl.offs[(size_t)pl.nt];
    const bool sa = in->factor || in->m == 0;
    double *const vec[5] = {in->u, sa ? in->a : nullptr, in->D, in->T, sa ? in->S : nullptr};
    const long long len[5] = {pl.q, pl.q, tot, tot, tot};
    for (int k = 0; k < 5; k++) {
      if (!vec[k]) continue;
      if (len[k] > 0x7fffffffLL)
        return fail(BESSX_ERR_ARG, "cox_groupscore_device: too many block entries for device output");
      if (int rc = check_on_device("cox_groupscore_device", "u, a, D, T, S", vec[k], BESSX_F64, 1, 0, (int)len[k], 1, dev,
                                   "an output"))
        return rc;
    }
  }
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  CoxInfoOrder x;
  cox_info_order(&o, in->n, in->m, in->ties, &x);
  const int rc = dev_call(dev, c.stream, [&](DevCall &dc) {
    return cox_groupscore_run(dc.sc, o, x, pl, dc.pk, dc.h, in, loglik, residual_sum, dc.st);
  });
  if (!rc) *n_events = x.n_events;
  return rc;
}

int bessx_op_cox_groupscore_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                                  const int *cols, int m, const int *group_starts, int n_groups, const int *groups,
                                  int n_tested, int candidate_block, int sorted, int repeats, double *stage_ms,
                                  double *bytes) {
  if (!x || repeats < 1 || !stage_ms || !bytes) return fail(BESSX_ERR_ARG, "op_cox_groupscore_bench: bad arguments");
  if (int rc = predict_check_model("op_cox_groupscore_bench", n, p, cols, m, 1, BESSX_LINK_IDENTITY)) return rc;
  if (int rc = check_m_max("op_cox_groupscore_bench", m)) return rc;
  GsPlan pl;
  if (int rc = groupscore_plan("op_cox_groupscore_bench", p, group_starts, n_groups, groups, n_tested, candidate_block, &pl))
    return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_groupscore_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  Owner sc;
  const size_t M = (size_t)m + 1, Q = (size_t)pl.q, TOT = (size_t)pl.offs[(size_t)pl.nt], N = (size_t)n;
  long long panel = 0, blk = 0, rps = 0, work_as = 0, rpsx = 0;
  int slabs = 0, cb = 0, depth = 0, slabsx = 0, chain = 0;
  addscore_split(n, m, pl.qmax, pl.block, &panel, &blk, &rps, &slabs, &cb, &depth);
  groupscore_cross_figures(n, m, pl, &work_as, &rpsx, &slabsx, &chain);
  const long long work_gs = groupscore_doubles(n, m, pl.qmax, pl.band);
  // n-vectors, an A and a factor of the library's own, as bessx_op_cox_addscore_bench has them (cc is its Cc's increment)
  const long long ldA = cox_diag_lda(n);
  std::vector<double> v(N, 0.25), g(N), e(N), cc(N, 1.0 / ((double)n * (double)n)), Ah((size_t)ldA * (size_t)m, 1.0 / 64.0),
      R(M * M, 0.0), r(M, 1.0 / 128.0), pk((size_t)diag_factor_doubles(m + 1));
  std::vector<int> pos(N), rowof(N);
  for (size_t i = 0; i < N; i++) {
    g[i] = (i % 2) ? -0.5 : 0.5;
    e[i] = 1.0 + (double)(i % 7) / 8.0;
    pos[i] = sorted ? (int)i : (int)(((long long)i * 7919) % n);
    rowof[i] = pos[i];
  }
  for (size_t j = 1; j < M; j++)
    for (size_t k = 1; k <= j; k++) R[j * M + k] = (j == k ? 1.0 : 1.0 / 64.0) / std::sqrt((double)n);
  r[0] = 0.0;
  addscore_pack_factor(R.data(), (long long)M, r.data(), m, pk.data());
  int *cols_d = nullptr, *pos_d = nullptr;
  double *g_d = nullptr, *A_d = nullptr, *out = nullptr;
  GsDev d{};
  CgsDev t{};
  d.x = x, d.f32 = dtype == BESSX_F32, d.rs = row_stride, d.cs = col_stride, d.n = n, d.m = m;
  HIPX(sc.alloc(&cols_d, (size_t)m));
  HIPX(sc.alloc(&pos_d, N));
  HIPX(sc.alloc(&t.rowof, N));
  HIPX(sc.alloc(&d.v, N));
  HIPX(sc.alloc(&g_d, N));
  HIPX(sc.alloc(&t.e, N));
  HIPX(sc.alloc(&t.cc, N));
  HIPX(sc.alloc(&A_d, Ah.size()));
  HIPX(sc.alloc(&d.P, (size_t)panel));
  HIPX(sc.alloc(&d.work_as, (size_t)work_as));
  HIPX(sc.alloc(&d.work_gs, (size_t)work_gs));
  HIPX(sc.alloc(&d.dd, (size_t)(pl.qmax + 15) / 16 * 16));
  HIPX(sc.alloc(&t.work, (size_t)cox_groupscore_doubles(n, pl.qmax, pl.band)));
  HIPX(sc.alloc(&out, 2 * Q + 3 * TOT));
  if (int rc = groupscore_upload_plan(sc, pl, nullptr, &d)) return rc;
  if (m > 0) {
    HIPX(hipMemcpy(cols_d, cols, (size_t)m * sizeof(int), hipMemcpyHostToDevice));
    HIPX(hipMemcpy(A_d, Ah.data(), Ah.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  HIPX(hipMemcpy(pos_d, pos.data(), N * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(t.rowof, rowof.data(), N * sizeof(int), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(d.v, v.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(g_d, g.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(t.e, e.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(t.cc, cc.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipMemcpy(d.work_gs + work_gs - (long long)pk.size(), pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  auto run = [&](int stage) -> int {
    if (stage == 0) {
      HIPX(launch_cox_addscore_pack(x, d.f32, row_stride, col_stride, n, cols_d, m, pl.qmax, pl.block, d.v, g_d, t.e, pos_d,
                                    m > 0 ? A_d : nullptr, ldA, d.P, nullptr));
      return 0;
    }
    if (stage >= 7) return cox_groupscore_tblocks(pl, d, t, out + 2 * Q + TOT, stage - 6, nullptr);
    return groupscore_blocks(pl, d, m > 0 ? 1 : 0, out, out + Q, out + 2 * Q, out + 2 * Q + 2 * TOT, stage, nullptr);
  };
  // (stage 0 = pack, then groupscore_blocks' steps 1 .. 6, then the band of T and its finish with the extraction, each
  // over every block, in an order in which a later stage finds the earlier one's results of the last block)
  for (int stage = 0; stage < 9; stage++) {
    float ms = 0.f;
    if (int rc = bt.run(repeats, &ms, [&]() { return run(stage); })) return rc;
    stage_ms[stage] = ms / repeats;
  }
  *bytes = (double)n * (double)pl.q * (dtype == BESSX_F32 ? 4.0 : 8.0);
  return BESSX_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// standard errors and confidence bands of the curves of one Cox model on a caller's device matrix (include/bessx.h
// section 2s)
// ----------------------------------------------------------------------------------------------
static_assert((int)BESSX_BAND_PLAIN == 0 && (int)BESSX_BAND_LOG == 1 && (int)BESSX_BAND_LOGLOG == 2,
              "conf codes of launch_cox_band");

namespace {

constexpr unsigned kBandAll = BESSX_BAND_ESTIMATE | BESSX_BAND_SE | BESSX_BAND_LOWER | BESSX_BAND_UPPER;
constexpr int kBandTMax = 65535;

inline CoxCall cox_call(const bessx_cox_band_input *in) {
  return CoxCall{in->x,    in->x_dtype, in->x_row_stride, in->x_col_stride, in->n,   in->p, in->cols, in->m,
                 in->beta, 1,           nullptr,          nullptr,          nullptr, 1,     static_cast<hipStream_t>(in->stream)};
}

// doubles of device scratch of one bessx_cox_hazard_var_device call
long long cox_hazvar_doubles(long long n, int m, long long J, int T) {
  const long long nb = (n + 1023) / 1024;
  // eta / H, e -> S0, the scans' totals, B; var0's increment, the totals of the two forward scans, the gathered result
  long long d = 2 * n + cox_eval_workspace(n, 1) + 1 + (long long)m + 1 + n + cox_surv_workspace(n) + (long long)T * (m + 2);
  if (m == 0 || J == 0) return d;
  // e, W and its totals, U, A and its totals, dh
  return d + n + (long long)m * n + nb * m + cox_info_ldu(J) * m + cox_diag_lda(n) * m + nb * m + n;
}

// idx[j]: where the prefix arrays are read for times[j] -- the last position with time <= times[j] behind which nothing is
// added any more: the end of the last tie group (ties = 0: the last position) that holds an event, -1 when no event has
// time <= times[j].  Under ties = 1 these are the positions section 2f's baseline reads, so cumhaz has its bits.  (o.first
// holds r(k): cox_event_groups sees single positions under ties = 0.)
void cox_hazvar_index(const CoxOrder &o, const double *time, int n, const double *times, int T, std::vector<int> *idx) {
  std::vector<double> gt;
  std::vector<int> ends;
  cox_event_groups(o, time, n, &gt, &ends);
  idx->resize((size_t)T);
  for (int j = 0; j < T; j++) {
    const size_t g = (size_t)(std::upper_bound(gt.begin(), gt.end(), times[j]) - gt.begin());
    (*idx)[(size_t)j] = g > 0 ? ends[g - 1] : -1;
  }
}

int cox_hazvar_run(Owner &sc, const CoxOrder &o, const CoxInfoOrder &x, const std::vector<int> &idx, std::vector<double> &h,
                   const bessx_cox_hazard_var_input *in, double *cumhaz, double *var0, double *drift, long long ld,
                   hipStream_t st) {
  const int n = in->n, m = in->m, T = in->T, f32 = in->x_dtype == BESSX_F32, ties = in->ties;
  const size_t N = (size_t)n, nb = (size_t)((n + 1023) / 1024), W = (size_t)m + 2;
  const long long rs = in->x_row_stride, cs = in->x_col_stride;
  const bool means = m > 0;  // (the caller has seen to it that an event exists)
  CoxDev d;  // (d.first holds r(k); d.ex holds S0 and d.eta holds H once they have been formed)
  if (int rc = cox_eval_stage(sc, o, in->cols, m, in->beta, 1, n, 1, 0, st, &d)) return rc;
  int *lastk = nullptr, *rowof = nullptr, *jptr = nullptr, *idx_d = nullptr;
  double *hs = nullptr, *v0 = nullptr, *res = nullptr, *e = nullptr, *Wd = nullptr, *scr = nullptr, *U = nullptr,
         *A = nullptr, *dh = nullptr, *scrA = nullptr;
  HIPX(sc.alloc(&hs, (size_t)cox_surv_workspace(n)));
  HIPX(sc.alloc(&v0, N));
  HIPX(sc.alloc(&res, (size_t)T * W));
  HIPX(sc.alloc(&idx_d, (size_t)T));
  HIPX(hipMemcpyAsync(idx_d, idx.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
  if (ties) {
    HIPX(sc.alloc(&lastk, N));
    HIPX(hipMemcpyAsync(lastk, x.lastk.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
  }
  const long long ldU = cox_info_ldu(x.J), ldA = cox_diag_lda(n);
  if (means) {
    HIPX(sc.alloc(&rowof, N));
    HIPX(hipMemcpyAsync(rowof, x.rowof.data(), N * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&jptr, N + 1));
    HIPX(hipMemcpyAsync(jptr, x.jptr.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPX(sc.alloc(&e, N));
    HIPX(sc.alloc(&Wd, (size_t)m * N));
    HIPX(sc.alloc(&scr, nb * (size_t)m));
    HIPX(sc.alloc(&U, (size_t)ldU * (size_t)m));
    HIPX(sc.alloc(&A, (size_t)ldA * (size_t)m));
    HIPX(sc.alloc(&dh, N));
    HIPX(sc.alloc(&scrA, nb * (size_t)m));
  }
  // sections 2e / 2f / 2h / 2j's launchers as they are
  HIPX(launch_cox_eval_eta(in->x, f32, rs, cs, n, d.cols, m, d.B, d.zero, 1, d.pos, d.eta, d.ex, st));
  if (means) HIPX(hipMemcpyAsync(e, d.ex, N * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPX(launch_cox_eval_suffix(d.ex, n, 1, d.work, st));
  if (means) HIPX(launch_cox_info_gather(in->x, f32, rs, cs, n, d.cols, m, rowof, e, Wd, st));
  HIPX(launch_cox_baseline(d.ex, d.wd, d.first, n, nullptr, 0, d.eta, hs, nullptr, st));  // (eta's n doubles hold H)
  HIPX(launch_cox_band_dh2(d.wd, d.ex, d.first, ties ? lastk : nullptr, n, v0, st));
  HIPX(launch_cox_prefix_scan(v0, n, hs, st));
  if (means) {
    HIPX(launch_cox_info_means(Wd, d.ex, jptr, n, m, x.J, scr, U, ldU, st));
    HIPX(launch_cox_diag_accum(U, ldU, jptr, d.wd, d.ex, d.first, ties ? lastk : nullptr, n, m, dh, scrA, A, ldA, st));
  }
  HIPX(launch_cox_band_gather(d.eta, v0, A, ldA, idx_d, T, m, res, st));
  h.resize((size_t)T * W);
  HIPX(hipMemcpyAsync(h.data(), res, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  for (int j = 0; j < T; j++) {
    const double *r = h.data() + (size_t)j * W;
    cumhaz[j] = r[0];
    var0[j] = r[1];
    std::copy(r + 2, r + W, drift + (long long)j * ld);
  }
  return 0;
}

// everything about a band call that needs no device; slab[w]: the slab of out that takes output w, or -1
int cox_band_check_args(const std::string &w, const CoxCall &c, const bessx_cox_band_input *in, const double *out, int *slab) {
  if (!out) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = cox_check(w.c_str(), c, true, false)) return rc;
  if (int rc = check_m_max(w, in->m)) return rc;
  const int T = in->T, m = in->m;
  if (T < 1 || !in->cumhaz || !in->var0) return fail(BESSX_ERR_ARG, w + ": cumhaz and var0 need T >= 1 values");
  if (T > kBandTMax) return fail(BESSX_ERR_UNSUPPORTED, w + ": T must be at most " + std::to_string(kBandTMax));
  for (int j = 0; j < T; j++) {
    if (!(in->cumhaz[j] >= 0.0) || !std::isfinite(in->cumhaz[j]))
      return fail(BESSX_ERR_ARG, w + ": cumhaz must be finite and non-negative");
    if (!(in->var0[j] >= 0.0) || !std::isfinite(in->var0[j]))
      return fail(BESSX_ERR_ARG, w + ": var0 must be finite and non-negative");
  }
  if (m > 0) {
    if (!in->drift || !in->factor) return fail(BESSX_ERR_ARG, w + ": null argument (drift, factor)");
    if (in->drift_ld < m) return fail(BESSX_ERR_ARG, w + ": drift_ld must be at least m");
    if (in->factor_ld < m) return fail(BESSX_ERR_ARG, w + ": factor_ld must be at least m");
    for (long long j = 0; j < T; j++)
      for (long long k = 0; k < m; k++)
        if (!std::isfinite(in->drift[j * in->drift_ld + k])) return fail(BESSX_ERR_ARG, w + ": drift must be finite");
    for (long long j = 0; j < m; j++)
      for (long long k = 0; k <= j; k++)
        if (!std::isfinite(in->factor[j * in->factor_ld + k]))
          return fail(BESSX_ERR_ARG, w + ": the lower triangle of the factor must be finite");
  }
  if (in->kind != BESSX_SURV_SURVIVAL && in->kind != BESSX_SURV_CUMHAZ)
    return fail(BESSX_ERR_ARG, w + ": kind must be BESSX_SURV_SURVIVAL or BESSX_SURV_CUMHAZ");
  if (in->conf_type != BESSX_BAND_PLAIN && in->conf_type != BESSX_BAND_LOG && in->conf_type != BESSX_BAND_LOGLOG)
    return fail(BESSX_ERR_ARG, w + ": conf_type must be BESSX_BAND_PLAIN, _LOG or _LOGLOG");
  if (in->kind == BESSX_SURV_CUMHAZ && in->conf_type == BESSX_BAND_LOGLOG)
    return fail(BESSX_ERR_ARG, w + ": log-log bands are defined for the survival function, not for the cumulative hazard");
  if (in->what == 0 || (in->what & ~kBandAll))
    return fail(BESSX_ERR_ARG, w + ": what must be a non-empty set of BESSX_BAND_* bits");
  if (!(in->z_c >= 0.0) || !std::isfinite(in->z_c)) return fail(BESSX_ERR_ARG, w + ": z_c must be finite and non-negative");
  if (in->out_slab_stride < 0 || in->out_row_stride < 0 || in->out_col_stride < 0)
    return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  int K = 0;
  for (int q = 0; q < 4; q++) slab[q] = (in->what >> q) & 1u ? K++ : -1;
  if ((in->n > 1 && in->out_row_stride == 0) || (T > 1 && in->out_col_stride == 0) || (K > 1 && in->out_slab_stride == 0))
    return fail(BESSX_ERR_ARG, w + ": out: a zero stride along an axis longer than 1");
  return 0;
}

int cox_band_run(Owner &sc, std::vector<double> &pk, std::vector<double> &tmp, const bessx_cox_band_input *in,
                 const int *slab, double *out, hipStream_t st) {
  const int n = in->n, m = in->m, T = in->T, f32 = in->x_dtype == BESSX_F32;
  const size_t ldP = 16 * (((size_t)m + 15) / 16), nP = (size_t)T * ldP, nR = m > 0 ? (size_t)cox_diag_pack_doubles(m, 1) : 0;
  int K = 0;
  for (int q = 0; q < 4; q++) K += slab[q] >= 0;
  // one upload: cumhaz, var0, the rows p_j = R drift_j (zeros behind entry m), the packed factor
  pk.assign(2 * (size_t)T + nP + nR, 0.0);
  std::copy(in->cumhaz, in->cumhaz + T, pk.begin());
  std::copy(in->var0, in->var0 + T, pk.begin() + T);
  double *P = pk.data() + 2 * (size_t)T;
  for (long long j = 0; j < T; j++) {
    const double *dj = in->drift + j * in->drift_ld;
    for (long long a = 0; a < m; a++) {
      const double *Ra = in->factor + a * in->factor_ld;
      double s = 0.0;
      for (long long k = 0; k <= a; k++) s += Ra[k] * dj[k];
      P[(size_t)j * ldP + (size_t)a] = s;
    }
  }
  if (m > 0) cox_diag_pack(in->factor, in->factor_ld, m, 1, P + nP);
  int *cols_d = nullptr;
  double *B_d = nullptr, *zero_d = nullptr, *ex = nullptr, *up = nullptr, *stage = nullptr;
  if (int rc = predict_upload_model(sc, in->cols, m, in->beta, &kCoxZero, 1, st, &cols_d, &B_d, &zero_d)) return rc;
  HIPX(sc.alloc(&ex, (size_t)n));
  HIPX(sc.alloc(&up, pk.size()));
  HIPX(hipMemcpyAsync(up, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(launch_cox_surv_ex(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, B_d, zero_d, ex, st));
  const double *hz = up, *v0 = up + T, *Pd = up + 2 * (size_t)T, *pkd = Pd + nP;
  if (in->out_on_device) {
    HIPX(launch_cox_band(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, pkd, Pd, (long long)ldP, hz, v0, ex,
                         T, in->kind, in->conf_type, in->z_c, slab, out, in->out_slab_stride, in->out_row_stride,
                         in->out_col_stride, st));
    HIPX(hipStreamSynchronize(st));
    return 0;
  }
  const size_t one = (size_t)n * (size_t)T, cnt = one * (size_t)K;
  HIPX(sc.alloc(&stage, cnt));
  HIPX(launch_cox_band(in->x, f32, in->x_row_stride, in->x_col_stride, n, cols_d, m, pkd, Pd, (long long)ldP, hz, v0, ex, T,
                       in->kind, in->conf_type, in->z_c, slab, stage, (long long)one, T, 1, st));
  tmp.resize(cnt);
  HIPX(hipMemcpyAsync(tmp.data(), stage, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  for (long long s = 0; s < K; s++)
    for (long long i = 0; i < n; i++)
      for (long long j = 0; j < T; j++)
        out[s * in->out_slab_stride + i * in->out_row_stride + j * in->out_col_stride] = tmp[(size_t)s * one + i * T + j];
  return 0;
}

}  // namespace

extern "C" {

int bessx_cox_hazard_var_workspace(int n, int m, int n_event_rows, int T, long long *doubles) {
  if (!doubles) return fail(BESSX_ERR_ARG, "cox_hazard_var_workspace: null argument");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, "cox_hazard_var_workspace: empty matrix");
  if (n_event_rows < 0 || n_event_rows > n)
    return fail(BESSX_ERR_ARG, "cox_hazard_var_workspace: n_event_rows must lie in [0, n]");
  if (T < 1) return fail(BESSX_ERR_ARG, "cox_hazard_var_workspace: T must be at least 1");
  if (int rc = check_m_max("cox_hazard_var_workspace", m)) return rc;
  *doubles = n_event_rows > 0 ? cox_hazvar_doubles(n, m, n_event_rows, T) : 0;
  return BESSX_OK;
}

int bessx_cox_hazard_var_device(const bessx_cox_hazard_var_input *in, double *cumhaz, double *var0, double *drift,
                                long long drift_ld, double *n_events) {
  const std::string w("cox_hazard_var_device");
  if (!in || !cumhaz || !var0 || !n_events) return fail(BESSX_ERR_ARG, w + ": null argument");
  const CoxCall c = cox_call(in);
  int events = 0;
  if (int rc = cox_check("cox_hazard_var_device", c, true, true, &events)) return rc;
  if (int rc = check_m_max(w, in->m)) return rc;
  if (in->weight)
    for (int i = 0; i < in->n; i++)
      if (!(in->weight[i] >= 0.0)) return fail(BESSX_ERR_ARG, w + ": weight must be non-negative");
  if (in->T < 1 || !in->times) return fail(BESSX_ERR_ARG, w + ": times needs T >= 1 values");
  for (int j = 0; j < in->T; j++)
    if (std::isnan(in->times[j])) return fail(BESSX_ERR_ARG, w + ": times holds a NaN");
  if (in->m > 0 && !drift) return fail(BESSX_ERR_ARG, w + ": null argument (drift)");
  if (drift_ld < (long long)in->m) return fail(BESSX_ERR_ARG, w + ": drift_ld must be at least m");
  int dev = -1;
  if (int rc = cox_check_device("cox_hazard_var_device", c, &dev)) return rc;
  CoxOrder o;
  cox_order(in->time, in->status, in->weight, in->n, &o);
  CoxInfoOrder x;
  cox_info_order(&o, in->n, in->m, in->ties, &x);
  std::vector<int> idx;
  cox_hazvar_index(o, in->time, in->n, in->times, in->T, &idx);
  int rc = 0;
  if (events > 0) {
    rc = dev_call(dev, c.stream, [&](DevCall &dc) {
      return cox_hazvar_run(dc.sc, o, x, idx, dc.h, in, cumhaz, var0, drift, drift_ld, dc.st);
    });
  } else {  // every row censored: no increment anywhere
    for (int j = 0; j < in->T; j++) {
      cumhaz[j] = var0[j] = 0.0;
      if (in->m > 0) std::fill(drift + (long long)j * drift_ld, drift + (long long)j * drift_ld + in->m, 0.0);
    }
  }
  if (!rc) *n_events = x.n_events;
  return rc;
}

int bessx_cox_band_workspace(int x_dtype, long long x_row_stride, long long x_col_stride, int n, int m, int T, unsigned what,
                             int out_on_device, long long *doubles, int *time_chunk) {
  const std::string w("cox_band_workspace");
  if (!doubles || !time_chunk) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (x_dtype != BESSX_F64 && x_dtype != BESSX_F32) return fail(BESSX_ERR_ARG, w + ": x: dtype must be BESSX_F64 or BESSX_F32");
  if (x_row_stride < 0 || x_col_stride < 0) return fail(BESSX_ERR_ARG, w + ": strides must be non-negative");
  if (n < 1 || m < 0) return fail(BESSX_ERR_ARG, w + ": empty matrix");
  if (T < 1) return fail(BESSX_ERR_ARG, w + ": T must be at least 1");
  if (T > kBandTMax) return fail(BESSX_ERR_UNSUPPORTED, w + ": T must be at most " + std::to_string(kBandTMax));
  if (what == 0 || (what & ~kBandAll)) return fail(BESSX_ERR_ARG, w + ": what must be a non-empty set of BESSX_BAND_* bits");
  if (int rc = check_m_max(w, m)) return rc;
  int K = 0;
  for (int q = 0; q < 4; q++) K += (what >> q) & 1u;
  const long long ldP = 16 * (((long long)m + 15) / 16);
  *doubles = (long long)m + 1 + n + 2LL * T + (long long)T * ldP + (m > 0 ? cox_diag_pack_doubles(m, 1) : 0) +
             (out_on_device ? 0 : (long long)K * n * T);
  *time_chunk = cox_band_time_chunk(x_dtype == BESSX_F32, x_row_stride, x_col_stride, nullptr);  // (an aligned base)
  return BESSX_OK;
}

int bessx_cox_band_device(const bessx_cox_band_input *in, double *out) {
  const std::string w("cox_band_device");
  if (!in) return fail(BESSX_ERR_ARG, w + ": null argument");
  const CoxCall c = cox_call(in);
  int slab[4];
  if (int rc = cox_band_check_args(w, c, in, out, slab)) return rc;
  int dev = -1;
  if (int rc = cox_check_device("cox_band_device", c, &dev)) return rc;
  if (in->out_on_device)
    for (int q = 0; q < 4; q++)
      if (slab[q] >= 0)
        if (int rc = check_on_device("cox_band_device", "out", out + (long long)slab[q] * in->out_slab_stride, BESSX_F64,
                                     in->out_row_stride, in->out_col_stride, in->n, in->T, dev))
          return rc;
  return dev_call(dev, c.stream, [&](DevCall &dc) { return cox_band_run(dc.sc, dc.pk, dc.h, in, slab, out, dc.st); });
}

int bessx_op_cox_band_bench(const void *x, int dtype, long long row_stride, long long col_stride, int n, int p,
                            const int *cols, int m, int T, unsigned what, int repeats, double *stage_ms) {
  const std::string w("op_cox_band_bench");
  if (repeats < 1 || !stage_ms || T < 1 || T > kBandTMax || what == 0 || (what & ~kBandAll))
    return fail(BESSX_ERR_ARG, w + ": bad arguments");
  if (!x) return fail(BESSX_ERR_ARG, w + ": null argument");
  if (int rc = check_x_model(w, x, dtype, row_stride >= 0 && col_stride >= 0, n, p, cols, m, &kCoxZero, 1,
                             BESSX_LINK_IDENTITY, false))
    return rc;  // (beta is the library's own)
  if (int rc = check_m_max(w, m)) return rc;
  if (int rc = need_device()) return rc;
  int dev = -1;
  if (int rc = check_device_matrix("op_cox_band_bench: x", x, dtype, row_stride, col_stride, n, p, &dev)) return rc;
  HIPX(hipSetDevice(dev));
  // a model, a factor and T-sized inputs of the library's own: R = 0.2 I + a small lower triangle, drift = cumhaz * 0.1
  const size_t M = (size_t)m, ldP = 16 * ((M + 15) / 16), nP = (size_t)T * ldP, nR = m > 0 ? (size_t)cox_diag_pack_doubles(m, 1) : 0;
  std::vector<double> B(M), R(M * M, 0.0), up(2 * (size_t)T + nP + nR, 0.0);
  for (size_t q = 0; q < M; q++) B[q] = ((q % 7) - 3.0) / 64.0;
  for (size_t j = 0; j < M; j++)
    for (size_t k = 0; k <= j; k++) R[j * M + k] = j == k ? 0.2 : ((j + 3 * k) % 5 - 2.0) / (16.0 * (double)M);
  for (int j = 0; j < T; j++) {
    const double H = (j + 1.0) / T;
    up[(size_t)j] = H;
    up[(size_t)T + (size_t)j] = H * H / 50.0;
    for (size_t a = 0; a < M; a++) {
      double s = 0.0;
      for (size_t k = 0; k <= a; k++) s += R[a * M + k] * (0.1 * H);
      up[2 * (size_t)T + (size_t)j * ldP + a] = s;
    }
  }
  if (m > 0) cox_diag_pack(R.data(), m, m, 1, up.data() + 2 * (size_t)T + nP);
  Owner sc;
  int *cols_d = nullptr, slab[4], K = 0;
  for (int q = 0; q < 4; q++) slab[q] = (what >> q) & 1u ? K++ : -1;
  double *B_d = nullptr, *zero_d = nullptr, *ex = nullptr, *upd = nullptr, *out = nullptr;
  if (int rc = predict_upload_model(sc, cols, m, B.data(), &kCoxZero, 1, nullptr, &cols_d, &B_d, &zero_d)) return rc;
  HIPX(sc.alloc(&ex, (size_t)n));
  HIPX(sc.alloc(&upd, up.size()));
  HIPX(sc.alloc(&out, (size_t)K * (size_t)n * (size_t)T));
  HIPX(hipMemcpy(upd, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPX(hipDeviceSynchronize());
  const int f32 = dtype == BESSX_F32;
  BenchTimer bt;
  if (int rc = bt.init(sc)) return rc;
  for (int stage = 0; stage < 2; stage++) {
    float ms = 0.f;
    const int rc = bt.run(repeats, &ms, [&]() -> int {
      if (stage == 0)
        HIPX(launch_cox_surv_ex(x, f32, row_stride, col_stride, n, cols_d, m, B_d, zero_d, ex, nullptr));
      else
        HIPX(launch_cox_band(x, f32, row_stride, col_stride, n, cols_d, m, upd + 2 * (size_t)T + nP, upd + 2 * (size_t)T,
                             (long long)ldP, upd, upd + T, ex, T, BESSX_SURV_SURVIVAL, BESSX_BAND_LOGLOG, 1.96, slab, out,
                             (long long)n * T, T, 1, nullptr));
      return 0;
    });
    if (rc) return rc;
    stage_ms[stage] = ms / repeats;
  }
  return BESSX_OK;
}

}  // extern "C"
