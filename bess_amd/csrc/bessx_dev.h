// bessx_dev.h -- internal interface between the HIP kernels (bessx_kernels.hip) and the host-side
// solver (bessx_session.cpp, bessx_fit.cpp, bessx_cv.cpp, bessx_paths.cpp, bessx_abi.cpp).  Not part of the C ABI (that is include/bessx.h).
#ifndef BESSX_DEV_H
#define BESSX_DEV_H

#include <hip/hip_runtime.h>

namespace bessx {

// Device-resident control block of one Algorithm::fit (src/Algorithm.h:113-171).  The host enqueues
// PDAS iteration "slots" speculatively; every kernel of slot s runs only if l == s-1 && !done, so
// slots issued after convergence fall through in a few microseconds without a host round trip.
struct FitCtrl {
  int done;        // active set repeated: Algorithm::fit returned
  int l;           // PDAS iterations committed so far (Algorithm::l)
  int T0;          // sparsity level of this fit
  int k_cur;       // support size of the current beta
  int irls_done;   // GLM sub-model fit converged (per PDAS iteration)
  int irls_steps;  // IRLS / Newton steps taken in the current PDAS iteration
  int info;        // non-zero: a k x k solve produced a non-finite value
  int same_prev;   // this slot's active set equals the previous iteration's: solve + residual skipped
  double coef0;    // current intercept
  double ll0;      // GLM: log-likelihood of the previous iterate
  int d_fresh;     // the score-pass partial sums in memory were computed from the CURRENT coefficients
  int irls_last;   // IRLS steps the last committed sub-model fit took (host sizes its next batch from it)
  // Cox Newton line search (src/Algorithm.h:1474-1481)
  int fast_same;   // covariance form: k_cov_d found the selection unchanged (consumed by the next k_topk)
  int ls_m;        // accepted exponent m (step 0.5^m)
  double ll1;      // partial log-likelihood at the trial point
  int gram_full;   // LM Gram cache: 1 = form the whole Gram this slot, 0 = only the rows of the new columns
  // covariance-update mode (LM): see the k_cov_* kernels
  int cov_nfill;   // length of the current fill list (a multiple of 32): missing + speculative columns
  int cov_stall;   // the new active set has uncached columns: the fit is parked (l = -1 - l) until the host has
                   // issued the fill
  int cov_groups;  // 32-column panel groups (passes over X) this fit has formed so far (host statistics)
  int cov_miss;    // internal error flag: an active column was not in the Gram column cache
  int cov_nmiss;   // columns of the requested set that are not cached (set by k_cov_need)
  int serial;      // which fit this block describes (set by k_fit_continue; the host checks it for chained fits)
  int sse_valid;   // sse_dot / sse_nrm belong to the current coefficients (set by the fused k_chol)
  double sse_dot;  // beta . X^T(m y) of the last solve
  double sse_nrm;  // |beta|^2 of the last solve
  unsigned long long snap_seq;  // sequence number of the last device snapshot of this block (deferred publication)
};
static_assert(sizeof(FitCtrl) <= 128, "the published control block is 128 bytes");

constexpr int GRAM_JC = 8;  // most tiles of one tile row handled by one wave of k_gram (runs of 8/4/2/1)
struct GramTask {
  int I, J0, nJ, pad_;
};

hipError_t launch_transpose_in(const double *src, int rows, int p, double *X, long ld, long r0, hipStream_t st);
// device ingest (bessx_k_ingest.hip): X (ld x p, ld a multiple of 128, rows n..ld zero) <- a device matrix of fp64 / fp32
// elements, element (i, j) at src[order[i] * rs + j * cs] (order: device, may be null); *nan_flag is set on a NaN
hipError_t launch_ingest(const void *src, int f32, long long rs, long long cs, const int *order, long long n,
                         long long p, double *X, long long ld, unsigned *nan_flag, hipStream_t st);
// device prediction (bessx_k_predict.hip): out[i * ors + r * ocs] = link(sum_k src(i, cols[k]) * B[k * R + r] + c[r]) on a
// device matrix like launch_ingest's; cols (m >= 0, ascending), B (m x R row-major) and c (R) are device arrays.  Only the
// m support columns are read.  PREDICT_LOGISTIC: out = pr, out2 (same strides) = labels; PREDICT_POISSON: out = exp(eta).
enum { PREDICT_IDENTITY = 0, PREDICT_LOGISTIC = 1, PREDICT_POISSON = 2 };  // = BESSX_LINK_* of include/bessx.h
hipError_t launch_predict(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                          const double *B, const double *c, int R, int link, double *out, long long ors, long long ocs,
                          double *out2, hipStream_t st);
// device evaluation (bessx_k_eval.hip): res[r] = sum_i w_i * f(eta(i, r), y(i, r)) with eta as in launch_predict, in one
// pass over the support's columns; PREDICT_LOGISTIC also res[R + r] = sum_i w_i * [(eta > 0) == (y > 0.5)]; with weights
// res[2 * R] = sum_i w_i.  y(i, r) at y[i * yrs + r * ycs] (ycs = 0: one y for every response), w_i at w[i * ws] (w null:
// ones); fp64 or fp32 device memory.  work: eval_workspace(...) doubles; res: 2 * R + 1 doubles; both device memory.
struct EvalData {
  const void *y;
  int y_f32;
  long long yrs, ycs;
  const void *w;
  int w_f32;
  long long ws;
};
long long eval_workspace(int f32, long long rs, long long cs, long long n, int m, int R, int link, int weighted);
hipError_t launch_eval(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                       const double *B, const double *c, int R, int link, const EvalData &d, double *work, double *res,
                       hipStream_t st);
hipError_t launch_eval_finish(const double *part, long long nb, int RS, double *out, hipStream_t st);
// device evaluation of Cox models (bessx_k_coxeval.hip), in positions k = rank of a row in the stable ascending order of
// the times.  _eta: eta and exp(clamp(eta, +-30)) of every row at its position pos[i], two R x n position-major arrays
// (src, cols, B as in launch_predict; zero: R doubles of 0.0).  _loglik: ex becomes the suffix sums S in place, then
// res[r] = sum_k wd[k] * (clamp(eta) - log S[first ? first[k] : k]); work: cox_eval_workspace(n, R) doubles.  _pairs:
// cnt[2 r], cnt[2 r + 1] = pairs (k, l) with first[l] > kg[k] and eta_k > eta_l, eta_k < eta_l (kg[k] = first[k] for an
// event, INT_MAX otherwise).  _suffix is the first half of _loglik: ex becomes S in place (scr: ceil(n / 1024) * R doubles).
// Everything is device memory.
long long cox_eval_workspace(long long n, int R);
hipError_t launch_cox_eval_eta(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *B, const double *zero, int R, const int *pos, double *eta, double *ex,
                               hipStream_t st);
// _eta_rows: _eta for R = 1, always with threads along rows: eta and ex are the same bits under every layout of x.
// cox_eval_eta_by_rows: whether _eta's own pass is that one.
bool cox_eval_eta_by_rows(long long rs, long long cs, int m);
hipError_t launch_cox_eval_eta_rows(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                    int m, const double *B, const double *zero, const int *pos, double *eta, double *ex,
                                    hipStream_t st);
hipError_t launch_cox_eval_scan_tot(const double *e, long long n, int R, double *scr, hipStream_t st);
hipError_t launch_cox_eval_suffix(double *ex, long long n, int R, double *scr, hipStream_t st);
hipError_t launch_cox_eval_loglik(const double *eta, double *ex, const double *wd, const int *first, long long n, int R,
                                  double *work, double *res, hipStream_t st);
hipError_t launch_cox_eval_pairs(const double *eta, const int *kg, const int *first, long long n, int R,
                                 unsigned long long *cnt, hipStream_t st);
// Breslow baseline and survival curves of one Cox model (bessx_k_coxsurv.hip).  _baseline: from S (launch_cox_eval_suffix,
// R = 1) h(k) = wd[k] / S[first[k]], H = its forward prefix sums in place over h, hout[g] = H[ends[g]] for g < J; scr:
// cox_surv_workspace(n) doubles.  _surv_ex: ex[i] = exp(clamp(eta_i, +-30)) in ROW order (src, cols, B as in launch_predict,
// R = 1; zero: a double of 0.0).  _surv_curves: out[i * ors + j * ocs] = exp(-(hg[j] * ex[i])) (kind 0) or hg[j] * ex[i]
// (kind 1), i < n, j < T.  Everything is device memory.
long long cox_surv_workspace(long long n);
hipError_t launch_cox_baseline(const double *S, const double *wd, const int *first, long long n, const int *ends, int J,
                               double *h, double *scr, double *hout, hipStream_t st);
hipError_t launch_cox_prefix_scan(double *h, long long n, double *scr, hipStream_t st);  // (_baseline's scan alone)
hipError_t launch_cox_surv_ex(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                              const double *B, const double *zero, double *ex, hipStream_t st);
hipError_t launch_cox_surv_curves(const double *ex, const double *hg, long long n, int T, int kind, double *out,
                                  long long ors, long long ocs, hipStream_t st);
// Restricted mean and quantile survival times of one Cox model (bessx_k_coxrmst.hip), from the ex of launch_cox_surv_ex.
// cox_rmst_pieces (host): the pieces of the segments below the largest of the T cuts -- they end at every distinct cut
// and after every cox_rmst_slab() segments -- pstart[0 .. NP] (room for max(cut) / cox_rmst_slab() + T + 1 values) and
// qcut[j] = the pieces in front of cut[j]; returns NP.  cox_rmst_chunk_rows: the rows one launch pair takes, so that its
// NP * rows doubles of partials stay bounded.  _partial: part[p * nr + i] = sum over the segments k of piece p, ascending,
// of wd[k] * exp(-(hs[k] * ex[i])) by fused multiply-add; _finish: out[i * ors + colj[s] * ocs] = the sum of the first
// colq[s] partials of row i (colq ascending, T entries).  _quantile: out[i * ors + j * ocs] = ut[first g with
// hz[g] * ex[i] >= c[j]], +inf without one, NaN for a NaN ex[i].  Everything but cut / pstart / qcut is device memory.
int cox_rmst_slab();
int cox_rmst_pieces(const int *cut, int T, int *pstart, int *qcut);
long long cox_rmst_chunk_rows(long long n, int NP);
hipError_t launch_cox_rmst_partial(const double *ex, long long nr, const double *hs, const double *wd, const int *pstart,
                                   int NP, double *part, hipStream_t st);
hipError_t launch_cox_rmst_finish(const double *ex, const double *part, long long nr, int NP, const int *colq,
                                  const int *colj, int T, double *out, long long ors, long long ocs, hipStream_t st);
hipError_t launch_cox_quantile(const double *ex, long long n, const double *hz, const double *ut, int J, const double *c,
                               int Q, double *out, long long ors, long long ocs, hipStream_t st);
// IPCW Brier score of R Cox models at T times (bessx_k_coxbrier.hip).  _ex: e[r * n + i] = exp(clamp(eta(i, r), +-30)) in
// ROW order (src, cols, B (m x R) as in launch_predict; zero: R doubles of 0.0).  launch_cox_brier: bs[j * R + r] = (1 / W)
// sum_i (time[i] <= tg[j] ? wa[i] exp(-z)^2 : b[j] w[i] expm1(-z)^2), z = hg[r * T + j] * e[r * n + i]; part: slabs * R * T
// doubles of the split (a function of n alone); only = 1 / 2 launches the term kernel / the addition of the slabs alone.
// _row_groups: the row groups whose sums a workgroup adds, a function of T alone.  _workspace: the doubles of device
// memory of a bessx_cox_brier_device call.  Everything else is device memory.
constexpr int COX_BRIER_T_MAX = 1 << 20;
void cox_brier_split(long long n, long long *rows_per_slab, long long *slabs);
int cox_brier_row_groups(int T);
long long cox_brier_workspace(long long n, int T, int R);
hipError_t launch_cox_brier_ex(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *B, const double *zero, int R, double *ex, hipStream_t st);
hipError_t launch_cox_brier(const double *e, const double *time, const double *w, const double *wa, const double *hg,
                            const double *tg, const double *b, long long n, int T, int R, double W, double *part,
                            double *bs, int only, hipStream_t st);
// weighted pair counts of R models (bessx_k_pairauc.hip): AUC(t), Uno's C, ROC AUC.  _eta: eta[r * n + pos[i]] =
// eta(i, r) (src, cols, B (m x R) as in launch_predict; zero: R doubles of 0.0).  launch_pairauc: the positions are cut
// into NT tiles of 1 .. PAIRAUC_TILE consecutive positions (tstart: NT + 1 ints, tstart[NT] = n; tseg[tile] < S: its
// segment, ascending; tnext[tile]: the first tile of a later segment, NT where there is none); the pair kernel writes
// part[((r * NT + kt) * S + b) * 2 + {0, 1}] = sum over k in tile kt, l in segment b of cw[k] lw[l] 1(eta_k > eta_l) /
// 1(eta_k = eta_l) for the segments after the tile's own (uno: from the tile's own on, and only where first[l] > kg[k]);
// the finish adds the tiles in order and writes og / oe[q * R + r] = sum_{kt <= last[q]} sum_{b >= from[q]} part (Q
// entries; last[q] < 0 gives 0).  part: 2 R NT S doubles; only = 1 / 2 launches the pair kernel / the finish alone.
// _tiles_max, _workspace: upper bounds of NT and of the doubles of device memory of a call.  Everything else is device memory.
constexpr int PAIRAUC_TILE = 1024, PAIRAUC_T_MAX = 1024;
long long pairauc_tiles_max(long long n, int T);
long long pairauc_workspace(long long n, int T, int R);
hipError_t launch_pairauc_eta(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                              const double *B, const double *zero, int R, const int *pos, double *eta, hipStream_t st);
hipError_t launch_pairauc(const double *eta, const double *cw, const double *lw, const int *kg, const int *first,
                          const int *tstart, const int *tseg, const int *tnext, long long n, int NT, int S, int R, int uno,
                          const int *last, const int *from, int Q, double *part, double *og, double *oe, int only,
                          hipStream_t st);
// expected information and score of one model (bessx_k_info.hip): with eta as in launch_predict (R = 1), v_i / g_i the
// working and score weights of the link and z_i = (1, x(i, cols[0]), ...), info = sum_i v_i z_i z_i^T ((m + 1) x (m + 1),
// leading dimension ld, both triangles, mirrors of each other) and score = sum_i g_i z_i (m + 1); res: launch_eval's
// three doubles for R = 1 (the same bits).  m + 1 <= INFO_M_MAX.  work: info_workspace(...) doubles.  launch_info_gram is
// the Gram sweep and its finish alone, from n-vectors v and g and part = info_gram_workspace(n, m) doubles.  The row
// split (info_split) is a function of n and m alone.  Everything is device memory.
constexpr int INFO_M_MAX = 1024;
void info_split(long long n, int m, long long *rows_per_slab, int *slabs);
long long info_gram_workspace(long long n, int m);
long long info_workspace(int f32, long long rs, long long cs, long long n, int m, int link, int weighted);
hipError_t launch_info_gram(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                            const double *vw, const double *gw, double *part, double *info, long long ld, double *score,
                            hipStream_t st);
hipError_t launch_info(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                       const double *B, const double *c, int link, const EvalData &d, double *work, double *res,
                       double *info, long long ld, double *score, hipStream_t st);
// launch_info_vg: the eta pass of launch_info alone, always with threads along rows: v and g (n doubles each) are the
// same bits under every layout of x.  info_eta_by_rows: whether launch_info's own pass is that one (its work then
// starts with exactly these v and g, each (n + 1) / 2 * 2 doubles).
bool info_eta_by_rows(long long rs, long long cs, int m);
hipError_t launch_info_vg(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                          const double *B, const double *c, int link, const EvalData &d, double *v, double *g,
                          hipStream_t st);
// the meat of a robust (sandwich) covariance (bessx_k_sandwich.hip).  _sums: S(g, a) = sum_{i in g} u_i z_ia, z_i = (1,
// x(i, cols[..])) (icpt) or (x(i, cols[..])), Ms = m + icpt entries, u null = ones, for clusters given as runs of at
// most sandwich_run_rows() rows: rowof (row at a sorted position; null: identity), rptr (NR + 1 run starts), rdst (NR:
// g >= 0, or -1 - row of P for a cluster of several runs), lptr (NL + 1) / lgrp (NL): the rows of P and the cluster of
// every such cluster.  S and P are column-contiguous with leading dimensions ldS / ldP (sandwich_ld).  _u: u and u^2
// from g and the leverage h.  _gram: B = sum_g y_g y_g^T (Ms x Ms, both triangles) and the sum vector for the rows y_g =
// (gw[g], src(g, cols1[..])), from one launch_info_gram sweep plus a fixed-order sum for B(0, 0): src = S with cols1 = 1 ..
// Ms - 1 and gw = S(:, 0), or a dense source in place with gw its first support column (_column copies it); work:
// sandwich_gram_workspace(G, Ms) doubles.  The depth functions count the additions behind an entry.  Device memory.
enum { SANDWICH_HC0 = 0, SANDWICH_HC1 = 1, SANDWICH_HC2 = 2, SANDWICH_HC3 = 3 };
int sandwich_run_rows();
int sandwich_sum_depth(long long rows);
int sandwich_sq_depth(long long G);
long long sandwich_ld(long long G);
long long sandwich_partial_rows(long long n, long long G, long long max_rows);
long long sandwich_gram_workspace(long long G, int Ms);
hipError_t launch_sandwich_sums(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                                int icpt, const double *u, const int *rowof, const int *rptr, const int *rdst, int NR,
                                const int *lptr, const int *lgrp, int NL, double *S, long long ldS, double *P,
                                long long ldP, hipStream_t st);
hipError_t launch_sandwich_u(const double *g, const double *h, int kind, long long n, double *u, double *u2,
                             hipStream_t st);
hipError_t launch_sandwich_column(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                  double *out, hipStream_t st);
hipError_t launch_sandwich_gram(const void *src, int f32, long long rs, long long cs, long long G, int Ms,
                                const int *cols1, const double *gw, double *work, double *B, long long ld, double *sums,
                                hipStream_t st);
// per-row diagnostics of one model (bessx_k_diag.hip).  _eta: the predictor pass (src, cols, B, c as in launch_predict,
// R = 1) whose epilogue writes, each to n doubles or nowhere (null): v_i as in launch_info, the response residual
// y_i - mu_i, the Pearson and the deviance residual.  _lev: h_i = v_i * sum_j t_ij^2 with T = Z R^T on the fp64 matrix
// cores, R lower triangular (m + 1) x (m + 1), given as pk = diag_factor_doubles(m) doubles in the order of
// diag_pack_factor (which runs on the host and never reads R's strict upper triangle); writes, each to n doubles or
// nowhere, h, rp / sqrt(phi (1 - h)), rd / sqrt(phi (1 - h)) and rp^2 h / (phi (m + 1) (1 - h)^2).  m + 1 <= INFO_M_MAX.
// diag_sum_depth: the additions behind one row's sum of t^2, a function of m alone.  Everything else is device memory.
int diag_sum_depth(int m);
long long diag_factor_doubles(int m);
void diag_pack_factor(const double *R, long long ld, int m, double *pk);
hipError_t launch_diag_eta(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                           const double *B, const double *c, int link, const EvalData &d, double *v, double *resp,
                           double *pear, double *dev, hipStream_t st);
hipError_t launch_diag_lev(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                           const double *pk, const double *vw, const double *rp, const double *rd, double phi,
                           double *o_h, double *o_sp, double *o_sd, double *o_ck, hipStream_t st);
// score tests of candidate columns against one model (bessx_k_addscore.hip).  addscore_split: for n rows, m support
// columns, q candidates and a candidate block asked for (0: the library's, else a multiple of 16), the doubles of the
// panel P and of the block workspace (partials, the block's rows of C, and LAST the packed factor:
// diag_factor_doubles(m + 1) doubles), the row split, the block used and the additions behind a candidate's sum of
// squares.  _pack_factor runs on the host: R ((m + 1) x (m + 1), lower triangular) with r appended as one more row.
// _pack writes P from the n-vectors v and g; _blocks runs cross, finish and (with_stat) the statistic kernel per block
// of candidates (cand: q ascending columns, -1 = the constant column, or null = 0 .. q - 1): u, d, s, a q doubles each, Cout q x ldc or null; only
// = 1 / 2 / 3 launches one of the three kernels alone.  m + 1 <= INFO_M_MAX.  Everything else is device memory.
void addscore_split(long long n, int m, int q, int block, long long *panel_doubles, long long *block_doubles,
                    long long *rows_per_slab, int *slabs, int *cand_block, int *stat_depth);
void addscore_pack_factor(const double *R, long long ld, const double *r, int m, double *pk);
hipError_t launch_addscore_pack(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                                int q, int block, const double *vw, const double *gw, double *P, hipStream_t st);
hipError_t launch_addscore_blocks(const void *src, int f32, long long rs, long long cs, long long n, int m, const int *cand,
                                  int q, int block, const double *P, double *work, int with_stat, double *u, double *d,
                                  double *s, double *a, double *Cout, long long ldc, int only, hipStream_t st);
// observed information and score of one Cox model (bessx_k_coxinfo.hip), the kernels between the predictor pass, the
// scans and the two launch_info_gram sweeps.  _gather: W(c, k) = e[k] * x(rowof[k], cols[c]), m x n position-major.
// _means: U(j, c) = S1(p, c) / S0[p] for jptr[p] <= j < jptr[p + 1], S1 the suffix sums of W along k (scr: ceil(n / 1024)
// * m doubles; U column-contiguous with leading dimension ldU >= J, cox_info_ldu(J) keeps its columns 16-byte aligned).
// _vg: v_i = e[pos[i]] * H[lastk[pos[i]]], g_i = wd[pos[i]] - v_i in ROW order (lastk null: the identity).  _finish:
// info = G1 - G2 without the sweeps' intercept entry (G2 null: no event), score, res[1] = sum of g.  Device memory.
long long cox_info_ldu(long long J);
hipError_t launch_cox_info_gather(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                  int m, const int *rowof, const double *e, double *W, hipStream_t st);
hipError_t launch_cox_info_means(const double *W, const double *S0, const int *jptr, long long n, int m, int J, double *scr,
                                 double *U, long long ldU, hipStream_t st);
hipError_t launch_cox_info_vg(const double *e, const double *H, const int *lastk, const double *wd, const int *pos,
                              long long n, double *v, double *g, hipStream_t st);
hipError_t launch_cox_info_finish(const double *G1, const double *G2, const double *U1, int m, double *info, long long ld,
                                  double *score, double *res, hipStream_t st);
// the proportional-hazards score test of one Cox model (bessx_k_coxzph.hip), on top of the arrays of bessx_k_coxinfo.hip.
// gp: the time transform in position order, an exact 0 where status is 0.  _hazard: h^q[k] = wd[k] gp[k]^q / S[first[k]],
// q = 0, 1, 2 (their forward scans are launch_cox_prefix_scan).  _vg: v^q_i = e[pos[i]] * H^q[lastk[pos[i]]] and a^q_i =
// wd gp^q - v^q_i in ROW order, weight q at + q * vs (H^q at + q * hs; lastk null: the identity).  _gram: launch_info_gram
// for the three weight pairs (vw + q * ws, gw + q * ws) in ONE sweep, each weight's results bit for bit launch_info_gram's
// with that weight alone: G + q * gs holds the (m + 1) x (m + 1) matrix (leading dimension m + 1), then the m + 1 score
// values; part: cox_zph_gram_workspace(n, m) doubles.  _finish: info_q = G1^q - G2^q without the intercept entry (G2
// null: no event), score0, score1.  Device memory.
long long cox_zph_gram_workspace(long long n, int m);
hipError_t launch_cox_zph_hazard(const double *wd, const double *gp, const double *S, const int *first, long long n,
                                 double *h0, double *h1, double *h2, hipStream_t st);
hipError_t launch_cox_zph_vg(const double *e, const double *H, long long hs, const int *lastk, const double *wd,
                             const double *gp, const int *pos, long long n, double *v, double *a, long long vs,
                             hipStream_t st);
hipError_t launch_cox_zph_gram(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                               const double *vw, const double *gw, long long ws, double *part, double *G, long long gs,
                               hipStream_t st);
hipError_t launch_cox_zph_finish(const double *G1, const double *G2, long long gs, int m, double *info0, double *info1,
                                 double *info2, long long ld, double *score0, double *score1, hipStream_t st);
// residuals and case influence of one Cox model (bessx_k_coxdiag.hip), on top of the arrays of bessx_k_coxinfo.hip.
// _accum: A(c, l) = sum_{p <= l} dh_p U(jptr[p], c), m x n position-major with leading dimension ldA = cox_diag_lda(n)
// (dh: n doubles, scr: ceil(n / 1024) * m doubles; U null: no event, A = 0).  _form: L(c, k) = g[rowof[k]] x(rowof[k],
// cols[c]) - wd[k] U(evj[k], c) + e[k] A(c, k) in place over A (evj[k] < 0: no event at k).  _apply: L P^T on the fp64
// matrix cores from pk = cox_diag_pack(P): tri: out[rowof[k]] = sum_j (P L_k)_j^2 with P lower triangular, else
// out[j * ldo + rowof[k]] = (P L_k)_j.  _deviance: the deviance residuals in row order from v, g (row order) and wd
// (position order).  _perm: out[c * ldo + rowof[k]] = L(c, k).  _schoenfeld: out[c * ldo + j] = x(evrow[j], cols[c]) -
// U(j, c).  cox_diag_pack runs on the host.  Everything else is device memory.
long long cox_diag_lda(long long n);
int cox_diag_dot_depth(int m);
int cox_diag_sum_depth(int m);
long long cox_diag_pack_doubles(int m, int tri);
void cox_diag_pack(const double *P, long long ld, int m, int tri, double *pk);
hipError_t launch_cox_diag_accum(const double *U, long long ldU, const int *jptr, const double *wd, const double *S0,
                                 const int *first, const int *lastk, long long n, int m, double *dh, double *scr,
                                 double *A, long long ldA, hipStream_t st);
hipError_t launch_cox_diag_form(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                                const int *rowof, const double *g, const double *wd, const double *e, const int *evj,
                                const double *U, long long ldU, double *A, long long ldA, hipStream_t st);
hipError_t launch_cox_diag_apply(const double *L, long long ldL, long long n, int m, const double *pk, int tri,
                                 const int *rowof, double *out, long long ldo, hipStream_t st);
hipError_t launch_cox_diag_deviance(const double *v, const double *g, const double *wd, const int *pos, long long n,
                                    double *out, hipStream_t st);
hipError_t launch_cox_diag_perm(const double *L, long long ldL, long long n, int m, const int *rowof, double *out,
                                long long ldo, hipStream_t st);
hipError_t launch_cox_diag_schoenfeld(const void *src, int f32, long long rs, long long cs, const int *cols, int m,
                                      const int *evrow, int J, const double *U, long long ldU, double *out,
                                      long long ldo, hipStream_t st);
// standard errors and bands of the curves of one Cox model (bessx_k_coxband.hip).  _dh2: dv[p] = sum_{k : r(k) = p} wd_k /
// S0(p)^2 (arguments of launch_cox_diag_accum).  _gather: out[tau * (m + 2) + (0, 1, 2 + j)] = (H, V0, A(j, .)) at position
// idx[tau], zeros for idx[tau] < 0 (A null: no drift).  launch_cox_band: the n x Tn results from pk = cox_diag_pack(R, tri),
// P (Tn rows p_tau = R drift_tau of ldP = 16 ceil(m / 16) doubles, zeros behind entry m), hz = cumhaz, v0 = var0, ex of
// launch_cox_surv_ex; slab[w] for w = estimate, se, lower, upper: the slab of out that takes it or negative; conf: 0 plain,
// 1 log, 2 log-log.  _time_chunk: grid times per workgroup for a source of this shape.  Device memory.
int cox_band_time_chunk(int f32, long long rs, long long cs, const void *src);
int cox_band_sum_depth(int m);
hipError_t launch_cox_band_dh2(const double *wd, const double *S0, const int *first, const int *lastk, long long n,
                               double *dv, hipStream_t st);
hipError_t launch_cox_band_gather(const double *H, const double *V0, const double *A, long long ldA, const int *idx,
                                  int Tn, int m, double *out, hipStream_t st);
hipError_t launch_cox_band(const void *src, int f32, long long rs, long long cs, long long n, const int *cols, int m,
                           const double *pk, const double *P, long long ldP, const double *hz, const double *v0,
                           const double *ex, int Tn, int kind, int conf, double zc, const int *slab, double *out,
                           long long oss, long long ors, long long ocs, hipStream_t st);
// score tests of candidate columns against one Cox model (bessx_k_coxaddscore.hip), on top of the arrays of
// bessx_k_coxinfo.hip and bessx_k_coxdiag.hip.  _pack: the panel (v_i, v_i x_i - e_pos(i) A_pos(i), g_i, zeros) in
// launch_addscore_pack's layout for the same m (launch_addscore_blocks takes it as it is: column 0 is v, where section
// 2l has the intercept's entry).  _cc: Cc_l = sum_{p <= l} dh_p / S0(p) (scr: ceil(n / 1024) doubles).  _quad: t_j = sum_p (dh_p /
// S0(p)) (sum_{l >= p} e_l x_lj)^2 per candidate, one pass over the candidate columns in blocks (cand: q ascending
// columns or null = 0 .. q - 1; part: cox_addscore_split's part_doubles; only = 1 / 2 launches one of the two kernels
// alone).  cox_addscore_split: a function of (n, q, block) alone; t_depth = the longest chain of additions behind a
// t_j.  Device memory.
void cox_addscore_split(long long n, int q, int block, long long *part_doubles, long long *rows_per_slab, int *slabs,
                        int *t_depth);
hipError_t launch_cox_addscore_pack(const void *src, int f32, long long rs, long long cs, long long n, const int *cols,
                                    int m, int q, int block, const double *vw, const double *gw, const double *e,
                                    const int *pos, const double *A, long long ldA, double *P, hipStream_t st);
hipError_t launch_cox_addscore_cc(const double *wd, const double *S0, const int *first, const int *lastk, long long n,
                                  double *scr, double *Cc, hipStream_t st);
hipError_t launch_cox_addscore_quad(const void *src, int f32, long long rs, long long cs, long long n, const int *cand,
                                    int q, int block, const int *rowof, const double *e, const double *Cc, double *part,
                                    double *t, int only, hipStream_t st);
// score tests of groups of candidate columns against one model (bessx_k_groupscore.hip), on top of launch_info_vg and
// the launchers of bessx_k_addscore.hip.  _band: w = the furthest tile a group of at most dmax columns reaches beyond the
// tile it starts in.  _rows: the row split of the Gram kernel, a function of n alone.  _cut: the tested groups (widths d,
// each <= block) in blocks of whole groups, first[b] = first group of block b, first[blocks] = nt (host; returns blocks).
// _doubles: this unit's workspace for blocks of at most qmax columns: partials and band of D, band of S, the block's rows
// of C and of T, and LAST the packed factor of addscore_pack_factor.  _gram: the band of D of one block (only = 1 / 2
// launches one of its two kernels alone); _sband: T = C Rx^T, the band of S and a; _extract: the groups' d x d blocks out
// of a band, upper triangle mirrored.  band + 1 <= 5.  Everything else is device memory.
int groupscore_band(int dmax);
void groupscore_rows(long long n, long long *rows_per_slab, int *slabs);
int groupscore_cut(const int *d, int nt, int block, int *first);
long long groupscore_doubles(long long n, int m, int qmax, int band);
hipError_t launch_groupscore_gram(const void *src, int f32, long long rs, long long cs, long long n, const int *cand,
                                  int qb, int band, const double *vw, double *work, int only, hipStream_t st);
hipError_t launch_groupscore_sband(const double *Cb, int m, int qb, int band, const double *pk, double *Tb, double *bandS,
                                   double *a, hipStream_t st);
hipError_t launch_groupscore_extract(const double *bandT, int band, const int *lpos, const long long *offs, int g0, int ng,
                                     double *out, hipStream_t st);
// score tests of groups of candidate columns against one Cox model (bessx_k_coxgroupscore.hip), on top of the launchers
// of bessx_k_coxaddscore.hip and bessx_k_groupscore.hip: the band of the risk-set term T = sum_p cc_p s_p s_p^T, s_p =
// sum_{l >= p} e_l x_l, cc_p = dh_p / S0(p).  _rows: the position split, a function of n alone, and the longest chain of
// roundings behind an entry of T.  _doubles: the workspace for blocks of at most qmax columns.  _cc: cc (not scanned).
// _tband: the band of one block in k_gs_extract's tile layout (only = 1 / 2 launches one of its two kernels alone; *bandT
// = where the band lies inside work).  band + 1 <= 5.  Device memory.
void cox_groupscore_rows(long long n, long long *rows_per_slab, int *slabs, int *t_depth);
long long cox_groupscore_doubles(long long n, int qmax, int band);
hipError_t launch_cox_groupscore_cc(const double *wd, const double *S0, const int *first, const int *lastk, long long n,
                                    double *cc, hipStream_t st);
hipError_t launch_cox_groupscore_tband(const void *src, int f32, long long rs, long long cs, long long n, const int *cand,
                                       int qb, int band, const int *rowof, const double *e, const double *cc, double *work,
                                       int only, double **bandT, hipStream_t st);
// k_y_prepare for R responses (columns of Y, stride ld, rows n..ld zero) in one launch, plus y.y of each
hipError_t launch_y_prepare_multi(double *Y, int n, long ld, int R, const double *w, int data_type, int is_normal,
                                  int add_weight, double *y_mean, double *yy, hipStream_t st);
hipError_t launch_normalize(double *X, long ld, int n, int p, double *y, const double *w, int data_type,
                            int is_normal, int add_weight, double *x_mean, double *x_norm, double *y_mean,
                            hipStream_t st);
hipError_t launch_xtv(const double *X, long ld, int p, int U, const double *v, const double *v2, double *part,
                      double *part2, const FitCtrl *ctrl, int slot, hipStream_t st);
hipError_t launch_xtv_variant(int variant, const double *X, long ld, int p, const double *v, double *part,
                              hipStream_t st);
// One pass over X for several chains' score vectors (k_xtv_mc): per chain the arguments of launch_xtv; ran (optional)
// receives the number of chains whose gate was open (0: the launch fell through).
constexpr int XTV_MC_MAX = 8;
struct XtvMc {
  const double *v[XTV_MC_MAX], *v2[XTV_MC_MAX];
  double *part[XTV_MC_MAX], *part2[XTV_MC_MAX];
  const FitCtrl *ctrl[XTV_MC_MAX];
  int slot[XTV_MC_MAX];
  int nc;
  int *ran;
};
hipError_t launch_xtv_mc(const double *X, long ld, int p, int U, const XtvMc &a, bool two, hipStream_t st);
hipError_t launch_score(const double *part, const double *part2, int nrb, int p, const double *beta_dense,
                        const double *xtx, double n_t, double lambda, int glm, const unsigned char *always,
                        double *bd, const FitCtrl *ctrl, int slot, hipStream_t st);
// What k_publish copies into the pinned result block; the last kernel of a batch of slots can do it itself (on = 1).
struct PubArgs {
  const unsigned char *dev;
  unsigned char *host;
  int ctrl_bytes;
  size_t off_sse;
  int n_sse;
  size_t off_b, off_a;
  int kcopy;
  unsigned long long *seq_host;
  unsigned long long seq;
  const int *count_ptr;
  int on;               // 1: publish now (copy dev -> host, release the sequence number);  2: only take a snapshot of
                        // the block into `snap` (device) -- the publication follows from there, off the critical path
  unsigned char *snap;  // device staging block (same offsets as dev; the cache's column count at snap_count_off)
  size_t snap_count_off;
};
// k_topk2 can end with the work of k_cov_need (covariance form of the LM fit) when the scores fit one chunk
struct TopkNeed {
  const double *bd;
  double *bd2;
  int p;
  int C;
  int *slot_of, *meta, *fcols;
  FitCtrl *ctrl;
  const int *A_cur;
  const double *bmm;  // per-block (min inside, max outside) scores left by k_cov_d, nbmm pairs
  int nbmm;
  const unsigned char *inA;  // membership flags of the current active set
  int inc1;                  // the scores are those on which the previous fit (one size smaller) ended: arg-max path
  int bmm_fresh;             // ... and bmm (block maxima + their columns) comes from the k_cov_d that made them
  // deferred publication of the PARENT fit's result block (pub.on = 1, pub.dev = its snapshot): done by a second
  // workgroup of this launch, concurrently with the selection -- the two system-scope round trips of a publication
  // are then not part of the chain's critical path
  PubArgs pub;
  // ... and this batch's own snapshot (snap.on = 2), taken right where a repeated active set is recorded, so that the
  // solve kernel behind this launch has nothing left to do
  PubArgs snap;
  // fused k_fit_continue(chained): this launch opens a fit chained behind fit `cont_parent` (cont_on = 1)
  int cont_on, cont_serial, cont_parent;
  // fused commit of a repeated active set (the record-and-stop branch of k_commit): commit_on = 1
  int commit_on;
  int no_restart;  // fold chains side by side: a full cache parks the fit (cov_stall = 4) instead of starting it over
  int *cm_A_cur;
  double *cm_b_cur, *cm_beta_dense;
  int *cm_hist;
  double *cm_hist_beta, *cm_hist_coef0;
  int cm_hist_stride;
  unsigned char *cm_inA;
};
bool topk_can_fuse_need(int len);
// exact std::nth_element semantics behind a tie at the selection boundary (k_topk_ties): flag = 2 ints (zeroed once:
// [0] raised by the selection kernels and cleared by k_topk_ties, [1] its heap-select branch was needed), work = 3 len ints
struct TopkTie {
  int *flag;
  int *work;
};
hipError_t launch_topk(const double *score, int len, int k, int *out, int *cand, const FitCtrl *ctrl, int slot,
                       hipStream_t st, const int *run_flag = nullptr, const TopkNeed *need = nullptr,
                       const TopkTie *tie = nullptr);
bool topk_supported(int len, int k);
void topk_set_variant(int v);  // test / benchmark hook: 0 = bit-by-bit search, 1 = radix search (default)
void gram_set_variant(int v);  // 1 = LDS-staged Gram kernel where it applies (default), 0 = k_gram throughout
bool gram_lds_applies(int ntiles, int tile_base);
hipError_t gram_lds_prepare();
// the IRLS step of the GLM fits in one pass over the active columns (k_irls_gram): up to 8 tile rows
bool irls_gram_applies(int mt);
int irls_gram_slab_rows(int mt, long ld);
int irls_gram_chunks(int mt);  // 64-row chunks per group of the instance that serves mt tile rows (0: none does)
hipError_t launch_irls_gram(int fam, const double *X, const double *aux, long ld, int n, const int *cols,
                            const double *y, const double *w, const double *mask, int nslab, int mt, double *part,
                            int ntiles, const FitCtrl *ctrl, int slot, int t, int T0, const double *bcur,
                            double *llpart, hipStream_t st, int wfloor = 1, int rows_override = 0);
hipError_t launch_gram_reduce(const double *part, int nslab, int ntiles, double *Gt, const FitCtrl *ctrl, int slot,
                              int gate_mode, hipStream_t st);
hipError_t launch_gram(const double *X, const double *aux, long ld, const int *cols, const double *w,
                       int rows_per_slab, const GramTask *tasks, int ntask, int nslab, double *part, int ntiles,
                       double *Gt, const FitCtrl *ctrl, int slot, int gate_mode, hipStream_t st, int tile_base = 0);
hipError_t launch_gram_lm_cached(const double *X, const double *aux, long ld, int *cols, const double *w,
                                 const int *A_new, int T0, int mt, const GramTask *tasks_full, int ntask_full,
                                 int rps_full, int nslab_full, const GramTask *tasks_inc, int ntask_inc, int rps_inc,
                                 int nslab_inc, double *part, double *Gt, double *Rt, int *src, double *gbuf0,
                                 double *gbuf1, int *Ac, int *meta, FitCtrl *ctrl, int slot, hipStream_t st);
// k_chol in the covariance mode of the LM fit: Gram gathered from the column cache, k_commit's work at the end
struct CholFuse {
  const double *G;
  const int *slot_of;
  int p;
  int T0;
  FitCtrl *ctrl;
  int *A_cur;
  double *b_cur, *beta_dense;
  int *hist;
  double *hist_beta, *hist_coef0;
  int hist_stride;
  unsigned char *inA;  // membership flags of the active set (repeated-set shortcut of k_cov_d)
  double yy;           // y.(m y) of the row set (loss from the solved system, k_cg)
  const double *d;     // X^T (m r) of the current coefficients (start value of entering columns, k_cg)
  const double *GS;    // slot-indexed Gram of the cached columns (CS x CS), or nullptr (k_cgr gathers from it)
  int CS;
  const double *zero;  // a word that holds 0.0 (what k_cgr reads for matrix columns outside its system)
  PubArgs pub;         // pub.on: this launch closes a batch of slots and publishes the result block (k_cg / k_cgr)
  double *fb_work;     // k_chol: work space of the pivoted fallback solve (256 x 256 + 1024 doubles), or nullptr
  const int *dep;      // k_cg / k_cgr: != 0 when exactly dependent columns are cached for the row set (CovCache meta[4])
};
constexpr size_t CHOL_FB_DOUBLES = 256 * 256 + 1024;
// the IRLS convergence test at the head of k_chol (otherwise its own launch, k_glm_irls_check): on = 1
struct IrlsChk {
  int on;
  FitCtrl *ctrl;
  int t, fam;
  const double *llpart;  // log-likelihood terms of the iterate the Gram was formed at, nblk of them
  int nblk, m;           // m = coefficients incl. the intercept
  double *bcur, *bprev;
};
hipError_t launch_chol(const double *Gt, int m, int mt, double ridge, int ridge_skip0, const double *rhs,
                       const int *rhs_gather, double *sol, int *info, const FitCtrl *ctrl, int slot, int gate_mode,
                       hipStream_t st, const CholFuse *fuse = nullptr, const IrlsChk *chk = nullptr);
// the pivoted solve behind a launch_chol whose kernel gave up (info = 2); fuse->fb_work is required
hipError_t launch_sym_fallback(const double *Gt, int m, int mt, double ridge, int ridge_skip0, const double *rhs,
                               const int *rhs_gather, double *sol, int *info, const FitCtrl *ctrl, int slot,
                               hipStream_t st, const CholFuse *fuse);
// tol: accepted relative residual |q - (G + ridge I) x| <= tol |q|; by_rows: systems of up to 208 unknowns use the
// row-dealt kernel (k_cgr), otherwise / beyond the tile-dealt one (k_cg)
hipError_t launch_cg(int m, int mt, double ridge, const double *rhs, const int *A_new, double *sol, const FitCtrl *ctrl,
                     int slot, const CholFuse *fuse, int maxit, hipStream_t st, double tol = 1e-13, bool by_rows = true);
// the selection of a covariance-form slot and the solve behind it in one launch (k_sel_cgr)
bool sel_cgr_applies(int len, int m);
hipError_t launch_sel_cgr(const double *score, int len, int k, int *A_new, const FitCtrl *ctrl, int slot,
                          const TopkNeed *need, double ridge, const double *rhs, double *sol, const CholFuse *fuse,
                          int maxit, hipStream_t st, double tol);
// ---------------------------------------------------------------------------------------------------------------
// Merged launches over many chains (round 5, bessx_kchunks.cpp: mc_engine; today the paths of many responses,
// bessx_multi.cpp -- the chunk chains of ONE path, which it was first built for, run faster on a stream and a host thread
// each: DESIGN_HISTORY.md).  The device runs about 2.5 single-workgroup kernels of different streams at a time
// (tools/probe/launch_rate.hip), so four chains on streams of their own get 2.4 x one chain's rate.  Here every
// chain is a workgroup (or a slice of the grid) of the SAME launch on ONE stream, and the sequencing the host did per
// chain -- which candidate, which PDAS iteration, is the fit over, open the next one -- lives in device memory:
//   k_mc_cov_d    (grid: column blocks x chains)  d and the sacrifice scores of every chain whose coefficients changed
//   k_mc_sel_cgr  (grid: chains)                  per chain: [record the finished candidate, open the next one,] the
//                                                 selection (repeated set / arg-max / full search + cache lookup), the
//                                                 solve, the commit -- the bodies of k_sel_cgr, gate by gate
// One pair of launches = one PDAS iteration WITH a solve for every chain; the confirming iteration of a candidate and the
// first selection of the next one ride in the same k_mc_sel_cgr.  The host queues pairs ahead, reads all chains' states
// back in one block (k_mc_status), serves parked chains with ONE union fill, and takes a chain over (the proven per-
// context path) where anything unusual turns up: a tie at the selection boundary, a solve that missed its target, a
// fit out of iterations, a loss that has to be recomputed.
// ---------------------------------------------------------------------------------------------------------------
struct McState {   // per chain, device memory: written by k_mc_sel_cgr / k_mc_resume only
  int cand;        // index within the chunk of the candidate being fitted
  int ncand;       // candidates of the chunk
  int need_d;      // the coefficients changed since the last score pass: k_mc_cov_d has work for this chain
  int finished;    // 1: every candidate recorded; 2: stopped, the host takes the chain over from candidate `cand`
  int parked;      // cov_stall of a parked fit (1 missing columns, 2 solve, 3 tie, 4 full cache); 0: running
  int resume;      // set with the wake-up after a fill: this slot's solve is still to run
  int prev_fresh;  // the previous candidate ended on a repeated set with fresh scores (arg-max start of the next one)
  int prev_T0;
  int solves;      // statistics: solves committed
  int why;         // finished == 2: 1 out of iterations, 2 info / cov_miss, 3 parked with a code the host does not serve
  int pad_[6];
};
static_assert(sizeof(McState) == 64, "McState is copied to the host in 64-byte records");
constexpr int MC_REC_I = 4;  // per candidate: T0, PDAS iterations, sse_valid, done
constexpr int MC_REC_D = 4;  // per candidate: coef0, sse_dot, sse_nrm, (unused)
struct McChain {   // one chain of a merged run: device memory, constant while the run lasts
  McState *state;
  const int *seq;  // the chunk's sparsity levels (device), state->ncand of them
  int width;       // row length of rec_A / rec_b (largest level of the path)
  int max_iter, p;
  // score pass from the cached Gram columns (the arguments of k_cov_d)
  const double *G, *xty, *xtx;
  double n_t, lambda;
  const unsigned char *always;
  double *d_out, *bd, *bmm;
  // selection and solve (the arguments of k_sel_cgr as enqueue_lm_slot_cov fills them; per candidate only the level and
  // the arg-max flags change)
  TopkNeed nd, nd1;  // nd1: the same with inc1 = bmm_fresh = 1 (arg-max start of a candidate one level up)
  CholFuse fz;       // (its T0 is not read: k_cgr's body takes the level from the size of the system)
  int *A_new;
  double *sol;
  double tol;
  int maxit;
  // per-candidate records
  int *rec_i;
  double *rec_d;
  int *rec_A;
  double *rec_b;
};
bool mc_applies(int p, int kmax);
hipError_t launch_mc_cov_d(const McChain *chains, int nchains, int p, hipStream_t st);
hipError_t launch_mc_sel_cgr(const McChain *chains, int nchains, int p, hipStream_t st);
// every chain's state and control block into pinned memory (192 bytes per chain), then the sequence number
hipError_t launch_mc_status(const McChain *chains, int nchains, unsigned char *host, unsigned long long *seq_host,
                            unsigned long long seq, hipStream_t st);
// after the fill that served it: wake the parked fit up (k_cov_resume) and mark its solve as due
hipError_t launch_mc_resume(const McChain *chains, int chain, hipStream_t st);
// stop a chain where it stands (the host takes it over)
hipError_t launch_mc_stop(const McChain *chains, int chain, hipStream_t st);
// launch_mc_resume for the chains chain[0..n) (device list) in one launch
hipError_t launch_mc_resume_list(const McChain *chains, const int *chain, int n, hipStream_t st);

hipError_t launch_chol_big(double *Gt, int m, int mt, double ridge, int ridge_skip0, const double *rhs,
                           const int *rhs_gather, double *sol, int *info, double *rdiag, double *z,
                           const FitCtrl *ctrl, int slot, int gate_mode, hipStream_t st);
hipError_t launch_fit_begin(FitCtrl *ctrl, int T0, int k_init, const int *init_idx, const double *init_val,
                            double coef0_init, int *A_cur, double *b_cur, double *beta_dense, int p, int *hist,
                            hipStream_t st, unsigned char *inA = nullptr, int serial = 0);
hipError_t launch_fit_continue(FitCtrl *ctrl, int T0, int *hist, hipStream_t st, int serial = 0, int chained = 0,
                               int parent = 0);
hipError_t launch_commit(FitCtrl *ctrl, int slot, int T0, const int *A_new, const double *sol, int has_intercept,
                         int wait_chain, int *A_cur, double *b_cur, double *beta_dense, int *hist, double *hist_beta,
                         double *hist_coef0, int hist_stride, hipStream_t st, unsigned char *inA = nullptr);
hipError_t launch_resid_lm(const double *X, long ld, int n, const double *y, const double *mask,
                           const FitCtrl *ctrl, int when, const int *A_cur, const double *b_cur, double *r,
                           double *sse, hipStream_t st, int mode = 0, int kc_given = 0, double c0_given = 0.0);
hipError_t launch_dot(const double *a, const double *b, long n, double *out, hipStream_t st);
hipError_t launch_glm_eta_gh(int fam, const double *X, long ld, int n, const double *y, const double *w,
                             const double *mask, const double *logfact, const FitCtrl *ctrl, int when,
                             const int *A_cur, const double *b_cur, double *g, double *h, double *stats,
                             hipStream_t st);
hipError_t launch_glm_irls_begin(const FitCtrl *ctrl, int slot, int fam, int m, double *bcur, double *bprev,
                                 hipStream_t st);
hipError_t launch_glm_irls_prep(int fam, const double *X, long ld, int n, const double *y, const double *w,
                                const double *mask, const FitCtrl *ctrl, int slot, int t, const int *A_new, int T0,
                                const double *bcur, double *Wv, double *z, double *llpart, hipStream_t st,
                                int wfloor = 1);
hipError_t launch_glm_irls_check(FitCtrl *ctrl, int slot, int t, int fam, const double *llpart, int nblk, int m,
                                 double *bcur, double *bprev, hipStream_t st);
// Cox (src/Algorithm.h:1370-1650, src/coxph.cpp:16-40)
struct CoxBufs {
  double *E, *TH, *ET, *S0, *RS0, *SALL, *STEST;      // state pass: exp(eta), w*exp*mask, test-row exp, scans
  double *EW, *WD;                                     // w*[delta!=0]*mask (get_A), w*delta*mask (fit)
  double *ETA0, *THF, *S0F, *RS0F, *VG, *WG1, *UD, *TH1, *S1;  // Newton work vectors
  double *M;                                           // n x k matrix S1/S0 (ld x 256)
  double *g, *u, *b0;                                  // k-vectors: gradient, Newton direction, iterate
  double *Gt2;                                         // second Gram (M^T diag(w delta) M) in tile layout
  double *llpart;
  double *SCR;                                         // block totals of the multi-block scans
  double *C1, *CU, *CV, *C2;                           // one-pass score: prefix sums of ew/S0, u, ew - u, ew/S0^2
  int one_pass;                                        // score pass reads X once (k_cox_score1p)
  int need_uv;                                         // CU / CV wanted although the score is not one-pass (groups)
  double *ldl_work;                                    // 256 x 256: dense copy for the LDL^T fallback of the Newton solve
  // one-pass Hessian of the Newton step (k_cox_hess): weights of the second Gram, its slab partials, per slab the
  // column totals of theta x, the slab carries and the vectors q_b
  int hess_fused;
  double *CW, *HP2, *HT, *CAR, *HQ;
  double fit_clamp;  // clamp of the linear predictor in the Newton step: 30 (src/Algorithm.h:1417-1422); cox_fit of the
                     // screening uses 50 (src/coxph.cpp:65-71)
};
// One pass over X for several chains' one-pass Cox scores (k_cox_score1p_mc): per chain the four n-vectors of
// launch_cox_score_pass (one_pass form) and its output planes; ran (optional) receives the number of open gates.
constexpr int COX_MC_MAX = 6;
struct CoxMc {
  const double *TH[COX_MC_MAX], *CU[COX_MC_MAX], *CV[COX_MC_MAX], *C2[COX_MC_MAX];
  double *out[COX_MC_MAX];
  const FitCtrl *ctrl[COX_MC_MAX];
  int slot[COX_MC_MAX];
  int nc;
  int *ran;
};
hipError_t launch_cox_score1p_mc(const double *X, long ld, int p, int U, int nrb, const CoxMc &a, hipStream_t st);
void cox_score_set_variant(int v);  // bench hook: the wave -> (column group, row block) map of k_cox_score1p (1 = default)
int cox_hess_slab_rows(long ld);
bool cox_hess_applies(int mt);
hipError_t cox_hess_prepare();
size_t cox_scan_scratch_doubles(long ld, int kmax);
size_t cox_score_part_doubles(int nrb, int p, int one_pass);  // per buffer of launch_cox_score_pass (part; part2: one_pass = 0)
hipError_t launch_cox_state(const double *X, long ld, int n, const double *y, const double *w, const double *mask,
                            const FitCtrl *ctrl, int when, const int *A_cur, const double *b_cur, CoxBufs cb,
                            double *stats, hipStream_t st);
hipError_t launch_cox_score_pass(const double *X, long ld, int p, int U, int nrb, CoxBufs cb, double *part,
                                 double *part2, const FitCtrl *ctrl, int slot, hipStream_t st);
hipError_t launch_cox_score(const double *part, const double *part2, int nrb, int p, const double *beta_dense,
                            double lambda, const unsigned char *always, double *bd, const FitCtrl *ctrl, int slot,
                            hipStream_t st);
hipError_t launch_cox_newton_begin(FitCtrl *ctrl, int slot, int k, CoxBufs cb, int *idcols, hipStream_t st);
hipError_t launch_cox_newton_step(const double *X, const double *aux, long ld, int n, const double *mask,
                                  FitCtrl *ctrl, int slot, int t, const int *A_new, int k, double lambda,
                                  const int *gcols, const int *idcols, int mt, const GramTask *tasks, int ntask,
                                  int rps, int nslab, double *gpart, int ntiles, double *Gt, CoxBufs cb,
                                  hipStream_t st, double *rdiag, double *zbig);
hipError_t launch_group_moments(int smax, const double *X, long ld, int n, const double *w1, const double *w2, int N,
                                const int *gidx, const int *gsz, const int *goff, double *mblk, double *dcol,
                                hipStream_t st, int cshift = 0);
hipError_t launch_iota(int *a, int n, hipStream_t st);
// screening with groups, LM: score_g = |argmin_b |y - X_g b||^2 / size(g) from the group moments
hipError_t launch_group_lsq_score(int N, const int *gidx, const int *gsz, const int *goff, const double *mblk,
                                  const double *dcol, const unsigned char *always, double *work, double *zwork,
                                  double *score, hipStream_t st);
// screening with groups, logistic: per-group IRLS (groups of at most 8 columns)
bool screen_logit_group_supported(int gmax);
size_t screen_logit_group_state_doubles(int N);
hipError_t launch_screen_logit_group(const double *X, long ld, int n, int N, const int *gidx, const int *gsz,
                                     const double *y, const double *w, double *state, int *done,
                                     const unsigned char *always, double *score, hipStream_t st);
// screening with groups, Cox: per-group damped Newton (groups of at most 4 columns)
bool screen_cox_group_supported(int gmax);
hipError_t launch_screen_cox_group(const double *X, long ld, int n, int N, const int *gidx, const int *gsz,
                                   const double *st_, const double *w, const unsigned char *always, double *score,
                                   hipStream_t st);
hipError_t launch_cox_group_moments(const double *X, long ld, int n, int p, CoxBufs cb, const int *allcols, int mcols,
                                    int smax, int N, const int *gidx_h, const int *gsz_h, const int *gidx,
                                    const int *gsz, const int *goff, long mblk_len, double *mblk, double *mblk2,
                                    double *dcol, hipStream_t st);
hipError_t launch_group_score(int N, const int *gidx, const int *gsz, const int *goff, const double *mblk,
                              const double *dcol, const double *part, int nrb, int p, int lm, double n_t,
                              double lambda, const double *beta_dense, const unsigned char *always, double *bd,
                              hipStream_t st, int smax = 1, double *work = nullptr, double *zwork = nullptr,
                              const FitCtrl *ctrl = nullptr, int slot = 0, int eig_mode = 0, double *eig_v = nullptr,
                              double *eig_l = nullptr);
constexpr int GRP_EIG_MAX = 16;  // widest group of the register-resident score kernel (GRP_MAX of bessx_kdev.hpp)
// find_ind on the device for groups of one width (k_group_expand)
hipError_t launch_group_expand(const int *G_sel, int T0, int gs, const int *gidx, int *cols, const FitCtrl *ctrl,
                               int slot, hipStream_t st);
hipError_t launch_commit_group(FitCtrl *ctrl, int slot, int T0, const int *G_new, int K, const int *cols,
                               const double *sol, int has_intercept, int wait_chain, int *A_cur, double *b_cur,
                               double *beta_dense, int *hist, double *hist_beta, double *hist_coef0, int hist_stride,
                               hipStream_t st);
hipError_t launch_screen_score_lm(const double *sxy, const double *sxx, int p, const unsigned char *always,
                                  double *score, hipStream_t st);
hipError_t launch_screen_logit(const double *X, long ld, int n, int p, const double *y, const double *w,
                               double *state, int *done, const unsigned char *always, double *score, hipStream_t st);
hipError_t launch_screen_cox(const double *X, long ld, int n, int p, const double *st_, const double *w,
                             const unsigned char *always, double *score, hipStream_t st);
hipError_t launch_gather_cols(const double *X, long ld, const int *A, int pnew, double *X2, hipStream_t st);
// covariance-update mode (LM)
hipError_t launch_cov_need(const int *list, int len, const double *bd, double *bd2, int p, int *slot_of, int *meta,
                           int C, int *fcols, FitCtrl *ctrl, int slot, const int *A_cur, hipStream_t st,
                           int no_restart = 0);
// spec: the lookup formed the masked score copy bd2 and `extras` holds its best columns (0: only the missing columns)
hipError_t launch_cov_publish_slots(const int *fcols, const int *slot_w, int *slot_of, const FitCtrl *ctrl, hipStream_t st);
hipError_t launch_cov_fill_list(int *fcols, const int *extras, const double *bd2, int *slot_of, int *meta,
                                FitCtrl *ctrl, int parked, hipStream_t st, int spec_max, int spec, int spec_min = 0);
hipError_t launch_cov_resume(FitCtrl *ctrl, hipStream_t st);
// the row sets of a cross-validation that share their fills (one launch reduces / compacts for all of them)
struct CovRowSets {
  int nr;
  double *G[9], *GS[9];
  const double *xtx[9];
  int ex_lo[9], ex_hi[9];  // slabs of the fold-major copy this row set leaves out (its own fold's rows)
};
hipError_t launch_cov_reduce_compact_sets(const double *part, int p, const int *fcols, const int *slot_of, int *meta,
                                          const CovRowSets &rs, int g0, int ngroups, int nslab, int CS,
                                          const FitCtrl *ctrl, int parked, hipStream_t st);
// Conjugate gradients for the LM systems of the covariance form beyond the register-resident solvers (bessx_cgbig.hip):
// one launch per step, every workgroup multiplies its 8 rows of the dense k x k copy of the cached Gram entries.
constexpr int CGB_MAX_K = 4096;  // the search direction lives in LDS (32 KB), 16 vector elements per thread in registers
struct CgbState {
  double rr[2];   // |r|^2 of the last two steps (by step parity)
  double qq;      // |q|^2
  int done_step;  // step at which the recurrence residual reached its target (0x7fffffff: not yet)
  int steps;      // steps taken
};
struct CgbWork {
  double *x, *q, *r[2], *p[2], *ap[2], *part_pq[2], *part_qq;
  CgbState *st;
};
size_t cgb_work_doubles(int kcap);  // work space (the dense matrix first) for systems of up to kcap unknowns
hipError_t launch_cg_big(const double *G, int p, const int *slot_of, const int *meta, const int *A_new, int k,
                         double ridge, const double *xty, const double *beta_dense, double *work, int kcap, double *sol,
                         FitCtrl *ctrl, int slot, int nsteps, double tol, double yy, hipStream_t st);
// one fill for several parked fits that share a slot map (k_cov_fill_union)
struct CovUnion {
  int nf;
  const int *list[8];  // the column sets that have to be cached when the fill is done
  int len[8];
  int on_restart[8];   // 1: this set is already cached -- it is listed only if the cache is started over
  // more sets than the 8 above (the merged run of many responses): dn of them, device arrays of their lists and
  // lengths, listed after the fixed ones (on_restart 0)
  int dn;
  const int *const *dlist;
  const int *dlen;
};
// restart: 0 keep the cache, 1 start it over, 2 decide on the device -- start over iff the columns the due lists miss
// (counted per list: an upper bound) do not fit the C-column cache; fill_ctrl->cov_nmiss tells which it was
hipError_t launch_cov_fill_union(const CovUnion &u, int restart, const int *extras, const double *bd2, int spec_max,
                                 int spec_min, int *slot_of, int *meta, int p, int *fcols, FitCtrl *fill_ctrl,
                                 hipStream_t st, int C = 0);
int cov_streamed_tiles_per_wave();
hipError_t launch_cov_panel(const double *X, const double *aux, long ld, int p, const double *mask, const int *fcols,
                            int g0, int ngroups, int rows_per_slab, int nslab, double *part, const FitCtrl *ctrl,
                            int parked, hipStream_t st);  // k_cov_panel_dp; ngroups 1..2
hipError_t cov_panel_prepare();
hipError_t launch_cov_reduce(const double *part, int p, const int *fcols, const int *slot_of, double *G, int g0,
                             int ngroups, int nslab, const FitCtrl *ctrl, int parked, hipStream_t st,
                             int ex_lo = 0, int ex_hi = 0);
hipError_t launch_rows_permute(const double *X, long ld, int p, const int *perm, long ldp, double *Xp, hipStream_t st);
hipError_t launch_cov_compact(const double *G, int p, const int *slot_of, const int *fcols, int g0, int ngroups,
                              double *GS, int CS, const FitCtrl *ctrl, int parked, hipStream_t st,
                              const double *xtx = nullptr, int *meta = nullptr);
// background (speculative) fill on a second stream
hipError_t launch_cov_d(const double *G, int p, const int *slot_of, const double *xty, const int *A_cur,
                        const double *b_cur, double *d_out, const double *beta_dense, const double *xtx, double n_t,
                        double lambda, const unsigned char *always, double *bd, const unsigned char *inA, double *bmm,
                        const FitCtrl *ctrl, int slot, hipStream_t st);
hipError_t launch_cov_gram(const double *G, int p, const int *slot_of, const int *A_new, int T0, int mt, double *Gt,
                           int *meta, const FitCtrl *ctrl, int slot, hipStream_t st);
hipError_t launch_publish(const unsigned char *dev, unsigned char *host, int ctrl_bytes, size_t off_sse, int n_sse,
                          size_t off_b, size_t off_a, int kcopy, unsigned long long *seq_host, unsigned long long seq,
                          hipStream_t st, const int *count_ptr = nullptr);
hipError_t launch_vec_mul(const double *a, const double *b, long n, double *out, hipStream_t st);
hipError_t launch_part_sum(const double *part, int nrb, int p, double *out, hipStream_t st);
hipError_t launch_fill(double *a, long n, double v, hipStream_t st);
hipError_t launch_gram_cols(const int *A_new, int T0, int mp, int intercept, int rhs_col, int *cols, FitCtrl *ctrl,
                            int slot, const int *A_cur, int allow_skip, hipStream_t st);
hipError_t launch_copy(const double *src, double *dst, long n, hipStream_t st);

}  // namespace bessx
#endif
