// bessx_multi.cpp -- many responses against one design: bessx_session_set_responses / bessx_session_sequential_path_multi.
// The Gram columns X^T diag(m) x_a and the cache that holds them depend on X and the row set only; what depends on the
// response is X^T y and y.y.  So the sequential paths of R responses run as R chains of the merged-launch engine
// (bessx_kchunks.cpp: mc_engine) on ONE cache: every response walks the same levels, the chains are at the same level at
// every step, and a parked response's missing columns join one union fill with every other parked response's.
#include "bessx_host.h"

#include <chrono>
#include <cmath>
#include <cstring>

namespace bessx {

namespace {

constexpr int MULTI_BATCH = 256;  // responses per merged run (one workgroup each in the selection + solve launches)

// what a fit reads of its response besides X^T y (shared by pointer): y (residual passes), y.y (the loss of a solve),
// the mean (coef0) and the null loss -- on one session or context
void set_response(bessx_session *c, double *y, double yy, double mean, double null) {
  c->y = y;
  c->yy_h[0] = yy;
  c->y_mean_h = mean;
  c->nullloss = null;
}

// ... on the session and on every context that runs fits for it: the chunk chains' and the merged runs' contexts and the
// CV fold contexts are copies of the session made when they were created, and keep those fields of their own
void set_response_all(bessx_session *s, double *y, double yy, double mean, double null) {
  set_response(s, y, yy, mean, null);
  std::vector<bessx_session *> ctx;
  kchains_contexts(s, &ctx);
  for (bessx_session *c : ctx) set_response(c, y, yy, mean, null);
  for (bessx_session *c : s->fold_ctx) set_response(c, y, yy, mean, null);
}

// response r in the place of the session's own: the host's statistics always; device: its prepared column becomes the
// y of the session and of all its contexts, and X^T y / diag(X^T X) of the all-rows set are formed from it by
// prepare_rowset -- the bits a session created with that column as y holds
int install_response(bessx_session *s, int r, bool device) {
  double *yr = s->resp_y + (size_t)r * s->ld;
  if (!device) {
    set_response(s, yr, s->resp_yy[(size_t)r], s->resp_mean[(size_t)r], s->resp_null[(size_t)r]);
    return 0;
  }
  kchains_quiesce(s);  // (no context may still be running on the response it had)
  set_response_all(s, yr, s->resp_yy[(size_t)r], s->resp_mean[(size_t)r], s->resp_null[(size_t)r]);
  if (int rc = settle_device_chain(s)) return rc;
  for (auto &q : s->cache) q.valid = q.model_only = false;  // (the device state is another response's)
  s->dev_state_rs = -1;
  return prepare_rowset(s, 0, true);
}

// the session's own response back: y, y.y, mean, null loss and X^T y (copied back bit for bit)
int restore_response(bessx_session *s) {
  kchains_quiesce(s);
  set_response_all(s, s->own_y, s->own_yy, s->own_mean, s->own_null);
  if (int rc = settle_device_chain(s)) return rc;
  HIPX(hipMemcpyAsync(s->xty[0], s->own_xty, (size_t)s->p * sizeof(double), hipMemcpyDeviceToDevice, s->st));
  return reset_path_caches(s);
}

// does the merged engine serve this path?  Otherwise the responses run one after another through sequential_path.
bool multi_batched_applies(const bessx_session *s, const int *seq, int ns, int nl) {
  if (nl != 1 || !mc_engine_applies(s) || s->grouped || !s->warm_start || s->trace.on || s->cv_shared || !s->publish ||
      !s->chain || s->fill_hook || s->kch_owner || s->parent)
    return false;
  for (int i = 0; i < ns; i++)
    if (seq[i] < 1 || (i && seq[i] <= seq[i - 1])) return false;  // ascending levels: one warm-start chain per response
  const int top = seq[ns - 1];
  if (top > 254 || top > s->cap || !mc_applies(s->p, top)) return false;
  // the cache must hold every column: it is never started over under the chains
  if (s->cov_C < (s->p + 31) / 32 * 32 + COV_R || top + COV_R + s->cov_spec > s->cov_C) return false;
  return true;
}

// responses per merged run: MULTI_BATCH, or fewer where the free device memory does not hold that many chain contexts
int batch_size(const bessx_session *s, int R) {
  const size_t mt = (size_t)s->capA / 16;
  const size_t per = 8 * ((size_t)4 * s->ld + part_elems(s) + (size_t)8 * s->p + mt * (mt + 1) / 2 * 256 +
                          (size_t)3 * (s->max_iter + 2) * s->hist_stride + (size_t)8 * s->capA) +
                     (size_t)4 * s->res_bytes;
  size_t fr = 0, tot = 0;
  int want = std::min(R, MULTI_BATCH);
  if (hipMemGetInfo(&fr, &tot) == hipSuccess && per > 0) {
    const size_t fit = fr / 2 / per;
    want = (int)std::max<size_t>(1, std::min<size_t>((size_t)want, fit));
  }
  return want;
}

// the paths of responses r0 .. r0 + B - 1 as B chains of one merged run
int run_batch(bessx_session *s, const int *seq, int ns, double lambda, int ic_type, int r0, int B, bessx_path_result *res) {
  const int p = s->p, width = seq[ns - 1];
  hipStream_t st = s->st;
  auto t0 = std::chrono::steady_clock::now();
  // X^T y of every response of the batch: k_xtv_mc, up to XTV_MC_MAX responses per pass over X (k_xtv's bits)
  const size_t pe = part_elems(s);
  for (int b0 = 0; b0 < B; b0 += XTV_MC_MAX) {
    XtvMc a = {};
    a.nc = std::min(XTV_MC_MAX, B - b0);
    for (int c = 0; c < a.nc; c++) {
      a.v[c] = s->resp_y + (size_t)(r0 + b0 + c) * s->ld;
      a.part[c] = s->resp_part + (size_t)c * pe;
    }
    HIPX(launch_xtv_mc(s->X, s->ld, p, s->U, a, false, st));
    for (int c = 0; c < a.nc; c++)
      HIPX(launch_part_sum(a.part[c], s->nrb, p, s->resp_xty + (size_t)(b0 + c) * p, st));
  }
  if (int rc = mc_contexts(s, B)) return rc;
  std::vector<McJob> jobs((size_t)B);
  for (int b = 0; b < B; b++) {
    McJob &j = jobs[(size_t)b];
    j.c = mc_context(s, b);
    // (the context's solves read its response's y.y, cov_fuse_args; its residual passes its y)
    const int r = r0 + b;
    set_response(j.c, s->resp_y + (size_t)r * s->ld, s->resp_yy[(size_t)r], s->resp_mean[(size_t)r], s->resp_null[(size_t)r]);
    j.lo = 0;
    j.ncand = ns;
    j.rec0 = b * ns;
    j.xty = s->resp_xty + (size_t)b * p;
  }
  McRecords rec;
  std::vector<int> takeover;
  long long fills = 0;
  int rc = mc_engine(s, seq, ns, jobs, B * ns, lambda, width, rec, takeover, &fills);
  s->multi_fills += fills;
  if (rc) return rc;
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // ---- every response's candidates, as sequential_path stores them (the session stands in for the response)
  for (int b = 0; b < B; b++) {
    const int r = r0 + b;
    bessx_path_result *out = res + r;
    out->n_candidates = 0;
    if (int rc2 = install_response(s, r, false)) return rc2;
    const double yy = s->yy_h[0];
    std::vector<Candidate> grid;
    grid.reserve((size_t)ns);
    SparseVec last;
    double last_c0 = 0.0;
    long long iters = 0;
    for (int i = 0; i < ns; i++) {
      const size_t g = (size_t)b * ns + i;
      if (!rec.i[g * MC_REC_I + 3]) break;
      const int T0 = rec.i[g * MC_REC_I + 0];
      if (T0 != seq[i]) return fail(BESSX_ERR_NUMERIC, "internal error: response chain record out of order");
      Candidate cand;
      cand.T0 = T0;
      cand.lambda = lambda;
      cand.beta.idx.assign(rec.A.begin() + g * width, rec.A.begin() + g * width + T0);
      cand.beta.val.assign(rec.b.begin() + g * width, rec.b.begin() + g * width + T0);
      cand.coef0 = rec.d[g * MC_REC_D + 0];
      cand.iters = rec.i[g * MC_REC_I + 1];
      // the loss from the solved system with this response's y.y; a pass over its own y where those terms cancel
      double tr = yy - rec.d[g * MC_REC_D + 1] - lambda * rec.d[g * MC_REC_D + 2];
      if (!rec.i[g * MC_REC_I + 2] || !(tr > 1e-6 * yy))
        if (int rc2 = mc_sse_by_residual(s, st, cand.beta.idx.data(), cand.beta.val.data(), T0, cand.coef0, &tr))
          return rc2;
      s->sparsity_level = T0;
      s->lambda_level = lambda;
      s->beta = cand.beta;
      s->coef0 = cand.coef0;
      s->l = cand.iters;
      s->sse_train = tr;
      s->sse_test = 0.0;
      if (int rc2 = metric_train_loss(s, &cand.loss)) return rc2;
      if (int rc2 = metric_ic(s, ic_type, 0, &cand.ic)) return rc2;
      store_candidate(s, out, cand, false);
      iters += cand.iters;
      last = cand.beta;
      last_c0 = cand.coef0;
      grid.push_back(cand);
    }
    const int good = (int)grid.size();
    size_t best = 0;  // first minimum, as sequential_path picks it
    for (size_t q = 1; q < grid.size(); q++)
      if (grid[q].ic < grid[best].ic) best = q;
    if (good > 0) store_best(s, out, grid[best], false);
    if (good < ns) {
      // the device stopped this response (a tie at the selection boundary, a solve for the Cholesky kernel, a full
      // cache, out of iterations): the rest of its path through the proven code, warm from its last recorded model, with
      // the response installed and the caches kept
      if (!takeover[(size_t)b]) return fail(BESSX_ERR_NUMERIC, "internal error: response chain ended short of its path");
      s->multi_host++;
      if (int rc2 = install_response(s, r, true)) return rc2;
      const int rest_n = ns - good, w = out->max_T0;
      std::vector<int> T0v((size_t)rest_n), itv((size_t)rest_n), sup((size_t)rest_n * std::max(w, 1));
      std::vector<double> lamv((size_t)rest_n), lossv((size_t)rest_n), icv((size_t)rest_n), c0v((size_t)rest_n),
          bv((size_t)rest_n * std::max(w, 1)), best_beta((size_t)s->p_full);
      bessx_path_result rest = {};
      rest.beta = best_beta.data();
      rest.capacity = rest_n;
      rest.cand_T0 = T0v.data();
      rest.cand_lambda = lamv.data();
      rest.cand_iters = itv.data();
      rest.cand_train_loss = lossv.data();
      rest.cand_ic = icv.data();
      rest.cand_coef0 = c0v.data();
      rest.cand_support = w > 0 ? sup.data() : nullptr;
      rest.cand_beta = w > 0 ? bv.data() : nullptr;
      rest.max_T0 = w;
      bessx_path_chain ch = {};
      ch.init_idx = last.idx.data();
      ch.init_val = last.val.data();
      ch.init_len = (int)last.idx.size();
      ch.init_coef0 = last_c0;
      ch.keep_caches = 1;
      if (int rc2 = bessx_session_sequential_path_chain(s, seq + good, rest_n, &lambda, 1, ic_type, 0, &ch, &rest))
        return rc2;
      for (int i = 0; i < rest.n_candidates && i < rest_n; i++) {
        const int q = out->n_candidates++;
        if (q >= out->capacity) continue;
        if (out->cand_T0) out->cand_T0[q] = T0v[(size_t)i];
        if (out->cand_lambda) out->cand_lambda[q] = lamv[(size_t)i];
        if (out->cand_iters) out->cand_iters[q] = itv[(size_t)i];
        if (out->cand_train_loss) out->cand_train_loss[q] = lossv[(size_t)i];
        if (out->cand_ic) out->cand_ic[q] = icv[(size_t)i];
        if (out->cand_coef0) out->cand_coef0[q] = c0v[(size_t)i];
        for (int jj = 0; jj < w; jj++) {
          if (out->cand_support) out->cand_support[(size_t)q * w + jj] = sup[(size_t)i * w + jj];
          if (out->cand_beta) out->cand_beta[(size_t)q * w + jj] = bv[(size_t)i * w + jj];
        }
        iters += itv[(size_t)i];
      }
      if (good == 0 || rest.ic < grid[best].ic) {  // (ties: the earlier candidate, as the single path's first minimum)
        if (out->beta) std::copy(best_beta.begin(), best_beta.end(), out->beta);
        out->coef0 = rest.coef0;
        out->train_loss = rest.train_loss;
        out->ic = rest.ic;
        out->lambda = rest.lambda;
        out->best_T0 = rest.best_T0;
        out->best_iters = rest.best_iters;
      }
    }
    out->device_seconds = secs;
    out->n_fits = ns;
    out->n_pdas_iters = iters;
  }
  s->multi_batched += B;
  return 0;
}

}  // namespace

}  // namespace bessx

extern "C" {

int bessx_session_set_responses(bessx_session *s, const double *Y, int R, int col_major) {
  if (!s || !Y) return fail(BESSX_ERR_ARG, "set_responses: null session or Y");
  if (R < 1) return fail(BESSX_ERR_ARG, "set_responses: R must be at least 1");
  if (s->model_type != 1)
    return fail(BESSX_ERR_UNSUPPORTED, "set_responses: several responses exist for the linear model (model_type 1) only");
  const int n = s->n;
  const long ld = s->ld;
  std::vector<double> host((size_t)ld * R, 0.0);  // column-major, ld rows per column, rows n..ld zero
  for (int r = 0; r < R; r++)
    for (int i = 0; i < n; i++) {
      const double v = col_major ? Y[(size_t)r * n + i] : Y[(size_t)i * R + r];
      if (std::isnan(v)) return fail(BESSX_ERR_ARG, "set_responses: Y contains NaN");
      host[(size_t)r * ld + i] = v;
    }
  HIPX(hipSetDevice(s->device));
  if (int rc = settle_device_chain(s)) return rc;
  if (R != s->resp_R) {
    s->resp_R = 0;
    HIPX(s->own.regrow(&s->resp_y, (size_t)ld * R));
  }
  if (!s->resp_xty) HIPX(s->own.alloc(&s->resp_xty, (size_t)MULTI_BATCH * s->p));
  if (!s->resp_part) HIPX(s->own.alloc(&s->resp_part, (size_t)XTV_MC_MAX * part_elems(s)));
  if (!s->own_xty) HIPX(s->own.alloc(&s->own_xty, (size_t)s->p));
  Owner tmp;
  double *stats = nullptr;
  HIPX(tmp.alloc(&stats, (size_t)2 * R));
  std::vector<double> st2((size_t)2 * R);
  std::vector<double> w((size_t)n);
  hipError_t e = hipMemcpyAsync(s->resp_y, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, s->st);
  // k_y_prepare's centring and weights for every column, and y.y (one launch)
  if (e == hipSuccess)
    e = launch_y_prepare_multi(s->resp_y, n, ld, R, s->w, s->data_type, s->is_normal, s->model_type == 1, stats,
                               stats + R, s->st);
  if (e == hipSuccess) e = hipMemcpyAsync(st2.data(), stats, st2.size() * sizeof(double), hipMemcpyDeviceToHost, s->st);
  if (e == hipSuccess) e = hipMemcpyAsync(w.data(), s->w, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->st);
  if (e == hipSuccess) e = hipStreamSynchronize(s->st);
  if (e != hipSuccess) return fail(BESSX_ERR_HIP, std::string("set_responses: ") + hipGetErrorString(e));
  s->resp_mean.assign(st2.begin(), st2.begin() + R);
  s->resp_yy.assign(st2.begin() + R, st2.end());
  s->resp_null.assign((size_t)R, 0.0);
  for (int r = 0; r < R; r++) {
    // Data::get_nullloss (src/Data.h:120-130) of that response, as session creation forms it
    double acc = 0.0, wsum = 0.0;
    for (int i = 0; i < n; i++) {
      const double yi = host[(size_t)r * ld + i] - (s->data_type == 1 && s->is_normal ? s->resp_mean[(size_t)r] : 0.0);
      acc += w[(size_t)i] * yi * yi;
      wsum += w[(size_t)i];
    }
    s->resp_null[(size_t)r] = s->data_type == 1 ? acc / (double)n : 2.0 * std::log(2.0) * wsum;
  }
  s->resp_R = R;
  return BESSX_OK;
}

int bessx_session_set_responses_device(bessx_session *s, const void *Y, int dtype, long long row_stride,
                                       long long col_stride, int R, void *stream) {
  if (!s || !Y) return fail(BESSX_ERR_ARG, "set_responses: null session or Y");
  if (R < 1) return fail(BESSX_ERR_ARG, "set_responses: R must be at least 1");
  if (s->model_type != 1)
    return fail(BESSX_ERR_UNSUPPORTED, "set_responses: several responses exist for the linear model (model_type 1) only");
  int dev = -1;
  if (int rc = check_device_matrix("set_responses: device Y", Y, dtype, row_stride, col_stride, s->n, R, &dev)) return rc;
  if (dev != s->device) return fail(BESSX_ERR_ARG, "set_responses: device Y: memory of another device than the session's");
  HIPX(hipSetDevice(s->device));
  if (int rc = settle_device_chain(s)) return rc;
  // Y is n x R values: the ingest kernel makes them fp64 column-major, the host copy goes through the host entry
  const int n = s->n;
  const long long ld = ((long long)n + 127) / 128 * 128;
  Owner sc;
  double *d = nullptr;
  unsigned *flag = nullptr;
  HIPX(sc.alloc(&d, (size_t)ld * R));
  HIPX(sc.alloc(&flag, 1));
  std::vector<double> host((size_t)n * R);
  if (int rc = ingest_enqueue(Y, dtype == BESSX_F32, row_stride, col_stride, nullptr, n, R, d, ld, flag,
                              static_cast<hipStream_t>(stream), s->st))
    return rc;
  HIPX(hipMemcpy2DAsync(host.data(), (size_t)n * sizeof(double), d, (size_t)ld * sizeof(double),
                        (size_t)n * sizeof(double), (size_t)R, hipMemcpyDeviceToHost, s->st));
  HIPX(hipStreamSynchronize(s->st));
  return bessx_session_set_responses(s, host.data(), R, 1);
}

int bessx_session_sequential_path_multi(bessx_session *s, const int *sequence, int sequence_len,
                                        const double *lambda_seq, int lambda_len, int ic_type, int is_cv,
                                        bessx_path_result *res) {
  if (!s || !res) return fail(BESSX_ERR_ARG, "sequential_path_multi: null session or results");
  if (!sequence || sequence_len < 1 || !lambda_seq || lambda_len < 1)
    return fail(BESSX_ERR_ARG, "sequential_path: empty sequence");
  if (is_cv) return fail(BESSX_ERR_UNSUPPORTED, "sequential_path_multi: cross-validation is not offered (is_cv = 0)");
  if (s->model_type != 1) return fail(BESSX_ERR_UNSUPPORTED, "sequential_path_multi: linear model (model_type 1) only");
  if (!s->screen_map.empty()) return fail(BESSX_ERR_UNSUPPORTED, "sequential_path_multi: not for a screening session");
  if (s->resp_R < 1) return fail(BESSX_ERR_ARG, "sequential_path_multi: call bessx_session_set_responses first");
  HIPX(hipSetDevice(s->device));
  if (int rc = settle_device_chain(s)) return rc;
  // the session's own response, put back whatever happens
  s->own_y = s->y;
  s->own_yy = s->yy_h[0];
  s->own_mean = s->y_mean_h;
  s->own_null = s->nullloss;
  HIPX(hipMemcpyAsync(s->own_xty, s->xty[0], (size_t)s->p * sizeof(double), hipMemcpyDeviceToDevice, s->st));
  const int R = s->resp_R;
  int rc = 0;
  // (one response: the ordinary path, whose chunk chains beat one chain of the merged run -- configs[1], 11.3 against
  // 20.7 ms)
  if (R > 1 && multi_batched_applies(s, sequence, sequence_len, lambda_len)) {
    // one cold cache for every batch (its columns depend on X only), like a path call
    rc = reset_path_caches(s);
    if (rc == 0 && !s->fcols_wide) {
      // the fill list of a union fill: the missing columns of up to 256 supports (every column at most once) and the
      // speculative ones, padded to a group
      int *wide = nullptr;
      if (s->own.alloc(&wide, (size_t)(s->p + 31) / 32 * 32 + 4 * COV_R) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(BESSX_ERR_HIP, "sequential_path_multi: fill list");
      } else {
        s->own.release_one(s->cov_fcols);
        s->cov_fcols = wide;
        s->fcols_wide = true;
      }
    }
    const int B = batch_size(s, R);
    for (int r0 = 0; r0 < R && rc == 0; r0 += B)
      rc = run_batch(s, sequence, sequence_len, lambda_seq[0], ic_type, r0, std::min(B, R - r0), res);
  } else {
    // the engine does not apply: every response through the ordinary path, installed in turn (same results, slower)
    for (int r = 0; r < R && rc == 0; r++) {
      rc = install_response(s, r, true);
      if (rc == 0) rc = bessx_session_sequential_path(s, sequence, sequence_len, lambda_seq, lambda_len, ic_type, 0, res + r);
      if (rc == 0) s->multi_host++;
    }
  }
  if (rc) kchains_quiesce(s);
  const int rc2 = restore_response(s);
  return rc ? rc : rc2;
}

}  // extern "C"
