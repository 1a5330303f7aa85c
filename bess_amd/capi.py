"""ctypes binding of libbessx.so (the C ABI declared in include/bessx.h).

This is plumbing only: every function forwards to the HIP library.  There is no Python or
NumPy fallback -- if the library is missing or no GPU is visible the call raises.
"""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BESSX_LIB_PATH: development aid (an instrumented build of the same library, e.g. -DBESSX_KTRACE for tools/ktrace.py)
LIB_PATH = os.environ.get("BESSX_LIB_PATH") or os.path.join(_HERE, "libbessx.so")

_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)
_i = ctypes.c_int
_d = ctypes.c_double
_ll = ctypes.c_longlong
_vp = ctypes.c_void_p

# names every build of libbessx.so must export (checked by tests/test_abi.py against include/bessx.h)
SYMBOLS = [
    "bessx_last_error", "bessx_device_info", "bessx_pywrap_bess", "bessx_bessCpp", "bessx_session_create",
    "bessx_session_destroy", "bessx_session_set_cv", "bessx_session_get_cv_folds", "bessx_session_sequential_path", "bessx_session_gs_path",
    "bessx_session_pgs_path", "bessx_session_get_screening", "bessx_session_get_screening_groups", "bessx_session_get_screening_scores", "bessx_session_score_mode", "bessx_session_counter",
    "bessx_session_trace_enable", "bessx_session_trace_size", "bessx_session_trace_copy_int",
    "bessx_session_trace_copy_double", "bessx_session_get_normalization", "bessx_session_score_pass_stats",
    "bessx_session_enable_kernel_timing", "bessx_session_submodel_steps", "bessx_session_fit", "bessx_session_fit_width", "bessx_session_reset_caches",
    "bessx_session_sequential_path_chain", "bessx_session_cv_eval", "bessx_session_debug_block_stream",
    "bessx_session_set_fill_hook", "bessx_session_set_kpath_chains",
    "bessx_session_marginal_scores", "bessx_session_cov_prefill_begin", "bessx_session_cov_prefill_compute",
    "bessx_session_cov_prefill_export", "bessx_session_cov_prefill_import", "bessx_session_cov_prefill_end",
    "bessx_session_cov_prefill_extend", "bessx_session_cov_state", "bessx_session_cov_cache_columns",
    "bessx_session_score_state",
    "bessx_session_cv_fill_geometry", "bessx_op_xtv", "bessx_op_topk", "bessx_op_gram",
    "bessx_op_chol_solve", "bessx_op_topk_bench", "bessx_op_chol_bench", "bessx_op_normalize", "bessx_op_stream_copy_gbps", "bessx_op_xtv_bench", "bessx_op_cox_score_bench",
    "bessx_op_cox_state", "bessx_op_cox_score", "bessx_op_cox_score_multi", "bessx_op_glm_gh", "bessx_op_glm_irls", "bessx_op_glm_irls_geometry",
    "bessx_op_group_scores", "bessx_op_group_lsq",
    "bessx_op_xtv_multi", "bessx_op_xtv_multi_bench", "bessx_session_set_responses", "bessx_session_sequential_path_multi",
    "bessx_session_create_device", "bessx_session_set_responses_device", "bessx_pywrap_bess_device", "bessx_op_ingest",
    "bessx_op_ingest_bench", "bessx_predict_device", "bessx_op_predict_bench", "bessx_eval_device", "bessx_op_eval_bench",
    "bessx_eval_cox_device", "bessx_op_cox_eval_bench",
    "bessx_cox_baseline_device", "bessx_cox_survival_device", "bessx_op_cox_surv_bench",
    "bessx_cox_survtime_device", "bessx_cox_survtime_workspace", "bessx_op_cox_rmst_bench",
    "bessx_cox_hazard_var_device", "bessx_cox_hazard_var_workspace", "bessx_cox_band_device", "bessx_cox_band_workspace",
    "bessx_op_cox_band_bench",
    "bessx_cox_brier_device", "bessx_cox_brier_workspace", "bessx_op_cox_brier_bench",
    "bessx_cox_auc_device", "bessx_cox_auc_workspace", "bessx_auc_device", "bessx_op_pairauc_bench",
    "bessx_info_device", "bessx_info_workspace", "bessx_op_info_bench",
    "bessx_cox_info_device", "bessx_cox_info_workspace", "bessx_op_cox_info_bench",
    "bessx_cox_zph_device", "bessx_cox_zph_workspace", "bessx_op_cox_zph_bench",
    "bessx_diag_device", "bessx_diag_workspace", "bessx_op_diag_bench",
    "bessx_cox_diag_device", "bessx_cox_diag_workspace", "bessx_op_cox_diag_bench",
    "bessx_meat_device", "bessx_sandwich_device", "bessx_sandwich_workspace", "bessx_op_sandwich_bench",
    "bessx_addscore_device", "bessx_addscore_workspace", "bessx_op_addscore_bench",
    "bessx_cox_addscore_device", "bessx_cox_addscore_workspace", "bessx_op_cox_addscore_bench",
    "bessx_groupscore_device", "bessx_groupscore_workspace", "bessx_op_groupscore_bench",
    "bessx_cox_groupscore_device", "bessx_cox_groupscore_workspace", "bessx_op_cox_groupscore_bench",
    "bessx_comm_unique_id", "bessx_comm_init", "bessx_comm_rank", "bessx_comm_world", "bessx_comm_allgather_f64",
    "bessx_comm_destroy",
]


MAX_SPARSITY = 16382  # T0_HARD of bessx_host.h: the largest bessx_problem.max_sparsity


class BessxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libbessx error %d: %s" % (code, msg))
        self.code = code


class Problem(ctypes.Structure):
    _fields_ = [("n", _i), ("p", _i), ("x", _D), ("x_col_major", _i), ("y", _D), ("weight", _D), ("data_type", _i),
                ("is_normal", _i), ("model_type", _i), ("algorithm_type", _i), ("max_iter", _i),
                ("is_warm_start", _i), ("always_select", _I), ("always_select_len", _i), ("device", _i),
                ("group_index", _I), ("group_index_len", _i),
                ("is_screening", _i), ("screening_size", _i), ("score_mode", _i), ("max_sparsity", _i)]


class DeviceInput(ctypes.Structure):
    """bessx_device_input: X (and optionally y, weight) in GPU memory; strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("y_host", _D),
                ("y_dev", _vp), ("y_dtype", _i), ("y_stride", _ll), ("weight_host", _D), ("weight_dev", _vp),
                ("weight_dtype", _i), ("weight_stride", _ll), ("row_order", _I), ("stream", _vp)]


class EvalInput(ctypes.Structure):
    """bessx_eval_input: the model, X in GPU memory, y and weight in host or GPU memory; strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("coef0", _D), ("R", _i), ("link", _i), ("y_host", _D),
                ("y_dev", _vp), ("y_dtype", _i), ("y_row_stride", _ll), ("y_col_stride", _ll), ("y_cols", _i),
                ("weight_host", _D), ("weight_dev", _vp), ("weight_dtype", _i), ("weight_stride", _ll), ("stream", _vp)]


class CoxEvalInput(ctypes.Structure):
    """bessx_cox_eval_input: the model, X in GPU memory, time / status / weight in host memory; strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("R", _i), ("time", _D), ("status", _D), ("weight", _D),
                ("ties", _i), ("want_pairs", _i), ("stream", _vp)]


class CoxBaselineInput(ctypes.Structure):
    """bessx_cox_baseline_input: one Cox model, X in GPU memory, time / status / weight in host memory."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("time", _D), ("status", _D), ("weight", _D), ("stream", _vp)]


class CoxSurvivalInput(ctypes.Structure):
    """bessx_cox_survival_input: one Cox model, X in GPU memory, the baseline cumulative hazard at T times in host
    memory, and how out is laid out; strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("hg", _D), ("T", _i), ("kind", _i), ("out_row_stride", _ll),
                ("out_col_stride", _ll), ("out_on_device", _i), ("stream", _vp)]


class CoxSurvtimeInput(ctypes.Structure):
    """bessx_cox_survtime_input: one Cox model, X in GPU memory; the segments and cuts of the RMST part and the baseline
    and levels of the quantile part in host memory (either part absent: count 0, pointers NULL); how the two outputs are
    laid out, strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("hs", _D), ("wd", _D), ("K", _i), ("cut", _I), ("T", _i),
                ("hz", _D), ("ut", _D), ("J", _i), ("c", _D), ("Q", _i), ("rmst_row_stride", _ll),
                ("rmst_col_stride", _ll), ("quant_row_stride", _ll), ("quant_col_stride", _ll), ("out_on_device", _i),
                ("stream", _vp)]


class CoxHazardVarInput(ctypes.Structure):
    """bessx_cox_hazard_var_input: one Cox model, X in GPU memory, time / status / weight and the T grid times in host
    memory."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("time", _D), ("status", _D), ("weight", _D), ("ties", _i),
                ("times", _D), ("T", _i), ("stream", _vp)]


class CoxBandInput(ctypes.Structure):
    """bessx_cox_band_input: one Cox model, X in GPU memory, cumhaz / var0 / drift at T times and the factor of the
    inverse information in host memory, what is wanted and how out is laid out; strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("cumhaz", _D), ("var0", _D), ("drift", _D), ("drift_ld", _ll),
                ("T", _i), ("factor", _D), ("factor_ld", _ll), ("kind", _i), ("conf_type", _i), ("z_c", _d),
                ("what", ctypes.c_uint), ("out_slab_stride", _ll), ("out_row_stride", _ll), ("out_col_stride", _ll),
                ("out_on_device", _i), ("stream", _vp)]


class CoxBrierInput(ctypes.Structure):
    """bessx_cox_brier_input: R Cox models, X in GPU memory, the baseline cumulative hazards at T times (R x T,
    model-major), the times, and the rows' time / IPCW weights / case weights in host memory; strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("R", _i), ("hg", _D), ("times", _D), ("T", _i), ("time", _D),
                ("row_a", _D), ("time_b", _D), ("weight", _D), ("stream", _vp)]


class CoxAucInput(ctypes.Structure):
    """bessx_cox_auc_input: R Cox models, X in GPU memory, T non-decreasing times, and the rows' time / status / IPCW
    weights / case weights in host memory, the truncation time of Uno's C (NaN = none); strides in elements."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("R", _i), ("times", _D), ("T", _i), ("time", _D), ("status", _D),
                ("row_a", _D), ("weight", _D), ("tau", _d), ("want_uno", _i), ("stream", _vp)]


class AucInput(ctypes.Structure):
    """bessx_auc_input: R logistic models, X in GPU memory, y (shared by the models) and the weights in host memory."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("B", _D), ("R", _i), ("y", _D), ("weight", _D), ("stream", _vp)]


class InfoInput(ctypes.Structure):
    """bessx_info_input: one model, X in GPU memory, y and weight in host or GPU memory, where info and score go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("coef0", _d), ("link", _i), ("y_host", _D), ("y_dev", _vp),
                ("y_dtype", _i), ("y_stride", _ll), ("weight_host", _D), ("weight_dev", _vp), ("weight_dtype", _i),
                ("weight_stride", _ll), ("info", _vp), ("info_ld", _ll), ("score", _vp), ("out_on_device", _i),
                ("stream", _vp)]


class DiagInput(ctypes.Structure):
    """bessx_diag_input: one model, X in GPU memory, y and weight in host or GPU memory, the factor of the inverse
    information in host memory, which kinds are wanted and where they go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("coef0", _d), ("link", _i), ("y_host", _D), ("y_dev", _vp),
                ("y_dtype", _i), ("y_stride", _ll), ("weight_host", _D), ("weight_dev", _vp), ("weight_dtype", _i),
                ("weight_stride", _ll), ("factor", _D), ("factor_ld", _ll), ("dispersion", _d),
                ("kinds", ctypes.c_uint), ("out", _vp), ("out_ld", _ll), ("out_on_device", _i), ("stream", _vp)]


class CoxInfoInput(ctypes.Structure):
    """bessx_cox_info_input: one Cox model, X in GPU memory, time / status / weight in host memory, where info and score
    go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("time", _D), ("status", _D), ("weight", _D), ("ties", _i),
                ("info", _vp), ("info_ld", _ll), ("score", _vp), ("out_on_device", _i), ("stream", _vp)]


class CoxZphInput(ctypes.Structure):
    """bessx_cox_zph_input: bessx_cox_info_input's model and data, the time transform gt in host memory, and where the
    three weighted information matrices and the two score vectors go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("time", _D), ("status", _D), ("weight", _D), ("ties", _i),
                ("gt", _D), ("info0", _vp), ("info1", _vp), ("info2", _vp), ("info_ld", _ll), ("score0", _vp),
                ("score1", _vp), ("out_on_device", _i), ("stream", _vp)]


class CoxDiagInput(ctypes.Structure):
    """bessx_cox_diag_input: one Cox model, X in GPU memory, time / status / weight in host memory, the factor of the
    inverse information and the inverse itself in host memory, which kinds are wanted and where they go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("time", _D), ("status", _D), ("weight", _D), ("ties", _i),
                ("factor", _D), ("factor_ld", _ll), ("cinv", _D), ("cinv_ld", _ll), ("kinds", ctypes.c_uint),
                ("out_rows", _vp), ("out_rows_ld", _ll), ("out_score", _vp), ("out_score_ld", _ll),
                ("out_dfbeta", _vp), ("out_dfbeta_ld", _ll), ("out_schoenfeld", _vp), ("out_schoenfeld_ld", _ll),
                ("event_rows", _I), ("out_on_device", _i), ("stream", _vp)]


class MeatInput(ctypes.Structure):
    """bessx_meat_input: a source matrix in GPU memory, the support, an optional row scalar u and optional cluster
    labels in host or GPU memory, where the meat and the sum vector go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("intercept", _i), ("u_host", _D), ("u_dev", _vp),
                ("cluster_host", ctypes.POINTER(_ll)), ("cluster_dev", _vp), ("cluster_dtype", _i),
                ("cluster_stride", _ll), ("meat", _vp), ("meat_ld", _ll), ("sums", _vp), ("out_on_device", _i),
                ("stream", _vp)]


class SandwichInput(ctypes.Structure):
    """bessx_sandwich_input: bessx_info_input plus the kind HC0 .. HC3, the factor of the inverse information in host
    memory, optional cluster labels in host or GPU memory and where the meat goes."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("coef0", _d), ("link", _i), ("y_host", _D), ("y_dev", _vp),
                ("y_dtype", _i), ("y_stride", _ll), ("weight_host", _D), ("weight_dev", _vp), ("weight_dtype", _i),
                ("weight_stride", _ll), ("kind", _i), ("factor", _D), ("factor_ld", _ll),
                ("cluster_host", ctypes.POINTER(_ll)), ("cluster_dev", _vp), ("cluster_dtype", _i),
                ("cluster_stride", _ll), ("info", _vp), ("info_ld", _ll), ("score", _vp), ("meat", _vp),
                ("meat_ld", _ll), ("out_on_device", _i), ("stream", _vp)]


class AddscoreInput(ctypes.Structure):
    """bessx_addscore_input: bessx_info_input's model and data, the factor of the inverse information in host memory (or
    null), the candidate columns (or null = all), the candidate block, and where info, score, u, d, s, a and the cross
    information go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("coef0", _d), ("link", _i), ("y_host", _D), ("y_dev", _vp),
                ("y_dtype", _i), ("y_stride", _ll), ("weight_host", _D), ("weight_dev", _vp), ("weight_dtype", _i),
                ("weight_stride", _ll), ("factor", _D), ("factor_ld", _ll), ("candidates", _I), ("q", _i),
                ("candidate_block", _i), ("info", _D), ("info_ld", _ll), ("score", _D), ("u", _vp), ("d", _vp),
                ("s", _vp), ("a", _vp), ("cross", _vp), ("cross_ld", _ll), ("out_on_device", _i), ("stream", _vp)]


class CoxAddscoreInput(ctypes.Structure):
    """bessx_cox_addscore_input: bessx_cox_info_input's model and data, the factor of the inverse information in host
    memory (or null), the candidate columns (or null = all), the candidate block, and where info, score, u, d, t, s, a and
    the cross information go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("time", _D), ("status", _D), ("weight", _D), ("ties", _i),
                ("factor", _D), ("factor_ld", _ll), ("candidates", _I), ("q", _i), ("candidate_block", _i),
                ("info", _D), ("info_ld", _ll), ("score", _D), ("u", _vp), ("d", _vp), ("t", _vp), ("s", _vp),
                ("a", _vp), ("cross", _vp), ("cross_ld", _ll), ("out_on_device", _i), ("stream", _vp)]


class GroupscoreInput(ctypes.Structure):
    """bessx_groupscore_input: bessx_info_input's model and data, the factor of the inverse information in host memory (or
    null), the partition of the columns into contiguous groups, the tested groups (or null = all), the candidate block,
    and where info, score, u, a, the packed blocks D and S and their offsets go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("coef0", _d), ("link", _i), ("y_host", _D), ("y_dev", _vp),
                ("y_dtype", _i), ("y_stride", _ll), ("weight_host", _D), ("weight_dev", _vp), ("weight_dtype", _i),
                ("weight_stride", _ll), ("factor", _D), ("factor_ld", _ll), ("group_starts", _I), ("n_groups", _i),
                ("groups", _I), ("n_tested", _i), ("candidate_block", _i), ("info", _D), ("info_ld", _ll), ("score", _D),
                ("u", _vp), ("a", _vp), ("D", _vp), ("S", _vp), ("offsets", ctypes.POINTER(_ll)), ("out_on_device", _i),
                ("stream", _vp)]


class CoxGroupscoreInput(ctypes.Structure):
    """bessx_cox_groupscore_input: bessx_cox_addscore_input's model and data, the factor of the inverse information in host
    memory (or null), bessx_groupscore_input's partition, tested groups and candidate block, and where info, score, u, a,
    the packed blocks D, T and S and their offsets go."""
    _fields_ = [("x", _vp), ("x_dtype", _i), ("x_row_stride", _ll), ("x_col_stride", _ll), ("n", _i), ("p", _i),
                ("cols", _I), ("m", _i), ("beta", _D), ("time", _D), ("status", _D), ("weight", _D), ("ties", _i),
                ("factor", _D), ("factor_ld", _ll), ("group_starts", _I), ("n_groups", _i), ("groups", _I),
                ("n_tested", _i), ("candidate_block", _i), ("info", _D), ("info_ld", _ll), ("score", _D), ("u", _vp),
                ("a", _vp), ("D", _vp), ("T", _vp), ("S", _vp), ("offsets", ctypes.POINTER(_ll)), ("out_on_device", _i),
                ("stream", _vp)]


class RResult(ctypes.Structure):
    _fields_ = [("beta", _D), ("coef0", _d), ("train_loss", _d), ("ic", _d), ("lambda_", _d), ("all_capacity", _i),
                ("n_all", _i), ("beta_all", _D), ("coef0_all", _D), ("train_loss_all", _D), ("ic_all", _D),
                ("screening_A", _I)]


class PathResult(ctypes.Structure):
    _fields_ = [("beta", _D), ("coef0", _d), ("train_loss", _d), ("ic", _d), ("lambda_", _d), ("best_T0", _i),
                ("best_iters", _i), ("capacity", _i), ("n_candidates", _i), ("cand_T0", _I), ("cand_lambda", _D),
                ("cand_iters", _I), ("cand_train_loss", _D), ("cand_ic", _D), ("cand_coef0", _D),
                ("cand_support", _I), ("cand_beta", _D), ("max_T0", _i), ("device_seconds", _d), ("n_fits", _ll),
                ("n_pdas_iters", _ll)]


class PathChain(ctypes.Structure):
    _fields_ = [("init_idx", _I), ("init_val", _D), ("init_len", _i), ("init_coef0", _d), ("keep_caches", _i),
                ("stop_support", _I), ("stop_beta", _D), ("stop_rows", _i), ("stop_row_len", _i), ("stop_rtol", _d),
                ("stopped_at", _i), ("last_idx", _I), ("last_val", _D), ("last_cap", _i), ("last_len", _i),
                ("last_coef0", _d), ("lead_levels", _I), ("lead_len", _i)]


_lib = None


def lib():
    """Load libbessx.so; raises ImportError loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "bess_amd: %s is missing. Build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C bess_amd/csrc). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.bessx_last_error.restype = ctypes.c_char_p
        L.bessx_device_info.argtypes = [ctypes.c_char_p, _i]
        L.bessx_pywrap_bess.argtypes = (
            [_D, _i, _i, _D, _i, _i, _D, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _I, _i, _D, _i, _I, _i, _D, _i]
            + [_i, _i, _i, _d, _d, _d, _i, _i, _i, _i, _I, _i, _d]
            + [_D, _i, _D, _i, _D, _i, _D, _i, _D, _D, _i, _D, _i, _D, _i, _I, _i, _I])
        L.bessx_bessCpp.argtypes = ([_D, _i, _i, _D, _i, _D, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _D, _i, _I, _i, _D,
                                     _i, _i, _i, _i, _d, _d, _d, _i, _i, _i, _i, _I, _i, _I, _i, _d,
                                     ctypes.POINTER(RResult)])
        L.bessx_session_create.argtypes = [ctypes.POINTER(_vp), ctypes.POINTER(Problem)]
        L.bessx_session_destroy.argtypes = [_vp]
        L.bessx_session_destroy.restype = None
        L.bessx_session_counter.argtypes = [_vp, _i]
        L.bessx_session_counter.restype = ctypes.c_longlong
        L.bessx_session_score_mode.argtypes = [_vp]
        L.bessx_session_score_mode.restype = _i
        L.bessx_session_get_screening.argtypes = [_vp, _I, _i]
        L.bessx_session_get_screening.restype = _i
        L.bessx_session_get_screening_groups.argtypes = [_vp, _I, _i]
        L.bessx_session_get_screening_groups.restype = _i
        L.bessx_session_get_screening_scores.argtypes = [_vp, _D, _i]
        L.bessx_session_get_screening_scores.restype = _i
        L.bessx_session_set_cv.argtypes = [_vp, _i, _I, ctypes.c_uint]
        L.bessx_session_get_cv_folds.argtypes = [_vp, _I]
        L.bessx_session_sequential_path.argtypes = [_vp, _I, _i, _D, _i, _i, _i, ctypes.POINTER(PathResult)]
        L.bessx_session_set_responses.argtypes = [_vp, _D, _i, _i]
        L.bessx_session_sequential_path_multi.argtypes = [_vp, _I, _i, _D, _i, _i, _i, ctypes.POINTER(PathResult)]
        L.bessx_session_gs_path.argtypes = [_vp, _i, _i, _i, _i, ctypes.POINTER(PathResult)]
        L.bessx_session_pgs_path.argtypes = [_vp, _i, _i, _d, _d, _i, _i, _i, _i, ctypes.POINTER(PathResult)]
        L.bessx_session_trace_enable.argtypes = [_vp, _i]
        L.bessx_session_trace_size.argtypes = [_vp, _i]
        L.bessx_session_trace_copy_int.argtypes = [_vp, _i, _I]
        L.bessx_session_trace_copy_double.argtypes = [_vp, _i, _D]
        L.bessx_session_get_normalization.argtypes = [_vp, _D, _D, _D]
        L.bessx_session_score_pass_stats.argtypes = [_vp, _i, _D, ctypes.POINTER(_ll), _D]
        L.bessx_session_enable_kernel_timing.argtypes = [_vp, _i]
        L.bessx_session_submodel_steps.argtypes = [_vp, _i, ctypes.POINTER(_ll)]
        L.bessx_session_fit.argtypes = [_vp, _i, _d, _i, _I, _D, _i, _d, _I, _D, _D, _I, _D, _D]
        L.bessx_session_reset_caches.argtypes = [_vp]
        L.bessx_session_sequential_path_chain.argtypes = [_vp, _I, _i, _D, _i, _i, _i, ctypes.POINTER(PathChain),
                                                          ctypes.POINTER(PathResult)]
        L.bessx_session_cv_eval.argtypes = [_vp, _i, _d, _i, _I, _D, _i, _d, _I, _i, _I, _D, _D, _I, _D, _D]
        L.bessx_session_debug_block_stream.argtypes = [_vp, _i]
        L.bessx_session_marginal_scores.argtypes = [_vp, _D]
        L.bessx_session_cov_prefill_begin.argtypes = [_vp, _I, _i]
        L.bessx_session_cov_prefill_extend.argtypes = [_vp, _I, _i]
        L.bessx_session_cov_state.argtypes = [_vp, _D, _I]
        L.bessx_session_cov_cache_columns.argtypes = [_vp, _i, _I, _i, _D, _I]
        L.bessx_session_score_state.argtypes = [_vp, _i, _I, _D, _I, _D, _D, _vp, _D, _D, _D, _D]
        L.bessx_session_cv_fill_geometry.argtypes = [_vp, _I]
        L.bessx_session_cov_prefill_compute.argtypes = [_vp, _i, _i]
        L.bessx_session_cov_prefill_export.argtypes = [_vp, _i, _i, _vp, _i]
        L.bessx_session_cov_prefill_import.argtypes = [_vp, _i, _i, _vp, _i]
        L.bessx_session_cov_prefill_end.argtypes = [_vp]
        L.bessx_op_xtv.argtypes = [_D, _i, _i, _i, _D, _D, _D, _D]
        L.bessx_op_topk.argtypes = [_D, _i, _i, _I]
        L.bessx_op_gram.argtypes = [_D, _i, _i, _i, _I, _i, _D, _D]
        L.bessx_op_chol_solve.argtypes = [_D, _i, _D, _D]
        L.bessx_op_normalize.argtypes = [_D, _i, _i, _D, _D, _i, _i, _i, _D, _D, _D]
        L.bessx_op_stream_copy_gbps.argtypes = [_ll, _i, _D]
        L.bessx_op_xtv_bench.argtypes = [_i, _i, _i, _i, _D, _D]
        L.bessx_comm_unique_id.argtypes = [ctypes.c_char_p]
        L.bessx_comm_init.argtypes = [ctypes.POINTER(_vp), _i, _i, ctypes.c_char_p, _i]
        L.bessx_comm_rank.argtypes = [_vp]
        L.bessx_comm_world.argtypes = [_vp]
        L.bessx_comm_allgather_f64.argtypes = [_vp, _D, _i, _D]
        L.bessx_comm_destroy.argtypes = [_vp]
        L.bessx_comm_destroy.restype = None
        L.bessx_op_cox_state.argtypes = [_D, _i, _i, _D, _D, _D, _I, _i, _D, _D, _D, _D, _D, _D, _D, _D]
        L.bessx_op_cox_score.argtypes = [_D, _i, _i, _D, _D, _D, _I, _i, _D, _d, _i, _D]
        L.bessx_op_cox_score_multi.argtypes = [_D, _i, _i, _D, _D, _D, _I, _i, _D, _i, _d, _D]
        L.bessx_op_glm_gh.argtypes = [_i, _D, _i, _i, _D, _D, _D, _I, _i, _D, _d, _d, _D, _D, _D, _D]
        L.bessx_op_glm_irls.argtypes = [_i, _i, _i, _i, _d, _i, _D, _i, _i, _D, _D, _D, _I, _i, _D, _D, _D, _D, _D, _D, _I]
        L.bessx_op_glm_irls_geometry.argtypes = [_i, _i, _I]
        L.bessx_op_group_scores.argtypes = [_D, _i, _i, _i, _I, _i, _D, _D, _D, _i, _d, _d, _vp, _D, _i, _D, _D, _D]
        L.bessx_op_group_lsq.argtypes = [_D, _i, _i, _I, _i, _D, _vp, _D]
        L.bessx_op_xtv_multi.argtypes = [_D, _i, _i, _i, _D, _D, _i, _D, _D]
        L.bessx_op_xtv_multi_bench.argtypes = [_i, _i, _i, _i, _i, _D, _D]
        L.bessx_op_topk_bench.argtypes = [_i, _i, _i, _i, _D]
        L.bessx_op_chol_bench.argtypes = [_i, _i, _D]
        L.bessx_session_create_device.argtypes = [ctypes.POINTER(_vp), ctypes.POINTER(Problem),
                                                  ctypes.POINTER(DeviceInput)]
        L.bessx_session_set_responses_device.argtypes = [_vp, _vp, _i, _ll, _ll, _i, _vp]
        L.bessx_pywrap_bess_device.argtypes = (
            [ctypes.POINTER(DeviceInput), _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _I, _i, _D, _i, _I, _i, _D, _i]
            + [_i, _i, _i, _d, _d, _d, _i, _i, _i, _i, _I, _i, _d]
            + [_D, _i, _D, _i, _D, _i, _D, _i, _D, _D, _i, _D, _i, _D, _i, _I, _i, _I, _I])
        L.bessx_op_ingest.argtypes = [_vp, _i, _ll, _ll, _I, _i, _i, _ll, _vp, _D, _I]
        L.bessx_op_ingest_bench.argtypes = [_vp, _i, _ll, _ll, _I, _i, _i, _ll, _i, _D, _D]
        L.bessx_predict_device.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _D, _D, _i, _i, _vp, _ll, _ll, _vp, _i, _vp]
        L.bessx_op_predict_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _D, _D]
        L.bessx_eval_device.argtypes = [ctypes.POINTER(EvalInput), _D, _D, _D]
        L.bessx_op_eval_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _i, _D, _D]
        L.bessx_eval_cox_device.argtypes = [ctypes.POINTER(CoxEvalInput), _D, ctypes.POINTER(_ll), ctypes.POINTER(_ll)]
        L.bessx_op_cox_eval_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _i, _D]
        L.bessx_cox_baseline_device.argtypes = [ctypes.POINTER(CoxBaselineInput), _I, _D, _D]
        L.bessx_cox_survival_device.argtypes = [ctypes.POINTER(CoxSurvivalInput), _vp]
        L.bessx_op_cox_surv_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _i, _D]
        L.bessx_cox_survtime_device.argtypes = [ctypes.POINTER(CoxSurvtimeInput), _vp, _vp]
        L.bessx_cox_survtime_workspace.argtypes = [_i, _I, _i, _I, _I, ctypes.POINTER(_ll), ctypes.POINTER(_ll)]
        L.bessx_op_cox_rmst_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _i, _i, _D]
        L.bessx_cox_hazard_var_device.argtypes =[ctypes.POINTER(CoxHazardVarInput), _D, _D, _D, _ll, _D]
        L.bessx_cox_hazard_var_workspace.argtypes = [_i, _i, _i, _i, ctypes.POINTER(_ll)]
        L.bessx_cox_band_device.argtypes = [ctypes.POINTER(CoxBandInput), _vp]
        L.bessx_cox_band_workspace.argtypes = [_i, _ll, _ll, _i, _i, _i, ctypes.c_uint, _i, ctypes.POINTER(_ll), _I]
        L.bessx_op_cox_band_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, ctypes.c_uint, _i, _D]
        L.bessx_cox_brier_device.argtypes = [ctypes.POINTER(CoxBrierInput), _D, _D]
        L.bessx_cox_brier_workspace.argtypes = [_i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll), ctypes.POINTER(_ll),
                                                _I]
        L.bessx_op_cox_brier_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _D]
        L.bessx_cox_auc_device.argtypes = [ctypes.POINTER(CoxAucInput), _D, _D, _D, _D, _D, _D]
        L.bessx_cox_auc_workspace.argtypes = [_i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll), ctypes.POINTER(_ll)]
        L.bessx_auc_device.argtypes = [ctypes.POINTER(AucInput), _D, _D, _D, _D]
        L.bessx_op_pairauc_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _i, _D, _D]
        L.bessx_info_device.argtypes = [ctypes.POINTER(InfoInput), _D, _D]
        L.bessx_info_workspace.argtypes = [_i, _ll, _ll, _i, _i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll), _I]
        L.bessx_op_info_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _D, _D]
        L.bessx_cox_info_device.argtypes = [ctypes.POINTER(CoxInfoInput), _D, _D, _D]
        L.bessx_cox_info_workspace.argtypes = [_i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll), _I]
        L.bessx_op_cox_info_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _D, _D]
        L.bessx_cox_zph_device.argtypes = [ctypes.POINTER(CoxZphInput), _D, _D]
        L.bessx_cox_zph_workspace.argtypes = [_i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll), _I]
        L.bessx_op_cox_zph_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _D, _D]
        L.bessx_diag_device.argtypes = [ctypes.POINTER(DiagInput)]
        L.bessx_diag_workspace.argtypes = [_i, _i, ctypes.c_uint, ctypes.POINTER(_ll)]
        L.bessx_op_diag_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _D, _D, _D]
        L.bessx_cox_diag_device.argtypes = [ctypes.POINTER(CoxDiagInput), _I]
        L.bessx_cox_diag_workspace.argtypes = [_i, _i, _i, ctypes.c_uint, ctypes.POINTER(_ll)]
        L.bessx_op_cox_diag_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _i, _i, _D, _D]
        L.bessx_meat_device.argtypes = [ctypes.POINTER(MeatInput), _I]
        L.bessx_sandwich_device.argtypes = [ctypes.POINTER(SandwichInput), _D, _D, _I]
        L.bessx_sandwich_workspace.argtypes = [_i, _ll, _ll, _i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_ll),
                                               ctypes.POINTER(_ll), _I, ctypes.POINTER(_ll), _I, _I, _I]
        L.bessx_op_sandwich_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, ctypes.POINTER(_ll), _i, _D, _D]
        L.bessx_addscore_device.argtypes = [ctypes.POINTER(AddscoreInput), _D, _D]
        L.bessx_addscore_workspace.argtypes = [_i, _i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll), _I, _I,
                                               ctypes.POINTER(_ll), _I]
        L.bessx_op_addscore_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _I, _i, _i, _i, _D]
        L.bessx_cox_addscore_device.argtypes = [ctypes.POINTER(CoxAddscoreInput), _D, _D, _D]
        L.bessx_cox_addscore_workspace.argtypes = [_i, _i, _i, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll),
                                                   ctypes.POINTER(_ll), _I, _I, _I, _I]
        L.bessx_op_cox_addscore_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _I, _i, _i, _i, _i, _D, _D]
        L.bessx_groupscore_device.argtypes = [ctypes.POINTER(GroupscoreInput), _D, _D]
        L.bessx_groupscore_workspace.argtypes = [_i, _i, _i, _I, _i, _I, _i, _i, ctypes.POINTER(_ll), ctypes.POINTER(_ll),
                                                 ctypes.POINTER(_ll), _I, _I, _I, _I, _I]
        L.bessx_op_groupscore_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _I, _i, _I, _i, _i, _i, _D]
        L.bessx_cox_groupscore_device.argtypes = [ctypes.POINTER(CoxGroupscoreInput), _D, _D, _D]
        L.bessx_cox_groupscore_workspace.argtypes = [_i, _i, _i, _i, _I, _i, _I, _i, _i, ctypes.POINTER(_ll),
                                                     ctypes.POINTER(_ll), ctypes.POINTER(_ll), _I, _I, _I, _I, _I]
        L.bessx_op_cox_groupscore_bench.argtypes = [_vp, _i, _ll, _ll, _i, _i, _I, _i, _I, _i, _I, _i, _i, _i, _i, _D, _D]
        _lib = L
    return _lib


def last_error():
    """Text of the calling thread's last library error (bessx_last_error)."""
    return lib().bessx_last_error().decode("utf-8", "replace")


def _check(rc):
    if rc != 0:
        raise BessxError(rc, lib().bessx_last_error().decode("utf-8", "replace"))


def _dp(a):
    return a.ctypes.data_as(_D) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(_I) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


NAN_IN_X = "There is NAN value in X"


def _check_device_route(rc):
    """_check for the entry points that ingest X on the device: the kernel's NaN flag becomes the estimators' error."""
    if rc == 1 and last_error() == NAN_IN_X:
        raise ValueError(NAN_IN_X)
    _check(rc)


def is_device_array(a):
    """True for an object in GPU memory: anything that exposes __cuda_array_interface__ (torch ROCm tensors do)."""
    return hasattr(a, "__cuda_array_interface__")


class _DeviceArray:
    """Pointer, element type, shape and ELEMENT strides of a device array, from its __cuda_array_interface__.  Raises
    ValueError for what the ingest kernel does not take; makes no device call.  Keeps the object alive."""

    def __init__(self, a, what, ndim=None):
        cai = a.__cuda_array_interface__
        shape = tuple(int(v) for v in cai["shape"])
        if ndim is not None and len(shape) != ndim:
            raise ValueError("%s: a device array must be %d-D, got shape %s" % (what, ndim, shape))
        if len(shape) < 1 or len(shape) > 2:
            raise ValueError("%s: a device array must be 1-D or 2-D, got shape %s" % (what, shape))
        typestr = cai["typestr"]
        if typestr not in ("<f8", "<f4"):
            raise ValueError("%s: a device array must be float64 or float32 (typestr '<f8' or '<f4'), got %r"
                             % (what, typestr))
        item = 8 if typestr == "<f8" else 4
        if any(v < 1 for v in shape):
            raise ValueError("%s: empty device array, shape %s" % (what, shape))
        strides = cai.get("strides")
        if strides is None:  # C-contiguous
            strides, acc = [], item
            for v in reversed(shape):
                strides.insert(0, acc)
                acc *= v
        strides = tuple(int(v) for v in strides)
        if len(strides) != len(shape) or any(v < 0 or v % item for v in strides):
            raise ValueError("%s: byte strides of a device array must be non-negative multiples of the item size %d, "
                             "got %s" % (what, item, strides))
        self.obj, self.ptr, self.item = a, int(cai["data"][0]), item
        self.dtype = 0 if item == 8 else 1  # BESSX_F64 / BESSX_F32
        self.shape, self.strides = shape, tuple(v // item for v in strides)
        if not self.ptr:
            raise ValueError("%s: null device pointer" % what)

    @property
    def size(self):
        return int(np.prod(self.shape))

    def as_vector(self, what):
        """(ptr, dtype, stride) of a 1-D array or of a 2-D one with a single row or column."""
        if len(self.shape) == 1:
            return self.strides[0]
        if self.shape[1] == 1:
            return self.strides[0]
        if self.shape[0] == 1:
            return self.strides[1]
        raise ValueError("%s: expected a vector, got shape %s" % (what, self.shape))


def _device_input(x, y, weight, row_order, stream):
    """(DeviceInput, n, p, objects to keep alive) for x on the device; every check that needs no device is made here."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    keep = [dx]
    din = DeviceInput()
    din.x, din.x_dtype, din.x_row_stride, din.x_col_stride = dx.ptr, dx.dtype, dx.strides[0], dx.strides[1]
    if is_device_array(y):
        dy = _DeviceArray(y, "y")
        if dy.size != n:
            raise ValueError("X.shape(0) should be equal to y.size")
        din.y_dev, din.y_dtype, din.y_stride = dy.ptr, dy.dtype, dy.as_vector("y")
        keep.append(dy)
    else:
        yh = _f64(y).reshape(-1)
        if yh.size != n:
            raise ValueError("X.shape(0) should be equal to y.size")
        din.y_host = _dp(yh)
        keep.append(yh)
    if weight is not None:
        if is_device_array(weight):
            dw = _DeviceArray(weight, "weight")
            if dw.size != n:
                raise ValueError("X.shape(0) should be equal to weight.size")
            din.weight_dev, din.weight_dtype, din.weight_stride = dw.ptr, dw.dtype, dw.as_vector("weight")
            keep.append(dw)
        else:
            wh = _f64(weight).reshape(-1)
            if wh.size != n:
                raise ValueError("X.shape(0) should be equal to weight.size")
            din.weight_host = _dp(wh)
            keep.append(wh)
    if row_order is not None:
        ro = _i32(row_order).reshape(-1)
        if ro.size != n or (np.sort(ro) != np.arange(n)).any():
            raise ValueError("row_order must be a permutation of 0..n-1")
        din.row_order = _ip(ro)
        keep.append(ro)
    din.stream = int(stream) if stream else None
    return din, n, p, keep


def device_info():
    buf = ctypes.create_string_buffer(512)
    _check(lib().bessx_device_info(buf, 512))
    return buf.value.decode()


def pywrap_bess(x, y, data_type, weight, is_normal, algorithm_type, model_type, max_iter, exchange_num, path_type,
                is_warm_start, ic_type, is_cv, K, g_index, state, sequence, lambda_sequence, s_min, s_max, K_max,
                epsilon, lambda_min, lambda_max, n_lambda, is_screening, screening_size, powell_path, always_select,
                tao, beta_out_len, coef0_out_len=1, train_loss_out_len=1, ic_out_len=1, aic_out_len=1,
                bic_out_len=1, gic_out_len=1, A_out_len=None, row_order=None, stream=0):
    """Same 38 positional arguments and 10-tuple result as the reference's SWIG wrapper
    (python/src/bess.i:17-30, called at python/bess/linear.py:360-375):
    (beta, coef0, train_loss, ic, nullloss, aic, bic, gic, A_out, l_out).
    An x in GPU memory (is_device_array) is read where it lies (bessx_pywrap_bess_device): y and weight may then be
    device arrays too, row_order (a permutation: row i of the problem is row row_order[i] of x; x only) and stream
    (raw handle of the stream x was produced on) apply; ValueError("There is NAN value in X") for a NaN in x."""
    din = None
    if is_device_array(x):
        din, n, p, _keep = _device_input(x, y, weight, row_order, stream)
    else:
        x = _f64(x)
        n, p = x.shape
        y = _f64(y).reshape(-1)
        weight = _f64(weight)
    state = _f64(state)
    g_index = _i32(g_index)
    sequence = _i32(sequence)
    lambda_sequence = _f64(lambda_sequence)
    always_select = _i32(always_select)
    if A_out_len is None:
        A_out_len = p
    beta = np.zeros(beta_out_len)
    coef0, loss, ic, nullloss = np.zeros(coef0_out_len), np.zeros(train_loss_out_len), np.zeros(ic_out_len), np.zeros(1)
    aic, bic, gic = np.zeros(aic_out_len), np.zeros(bic_out_len), np.zeros(gic_out_len)
    a_out = np.zeros(A_out_len, dtype=np.int32)
    l_out = np.zeros(1, dtype=np.int32)
    if din is not None:
        x_nan = np.zeros(1, dtype=np.int32)
        rc = lib().bessx_pywrap_bess_device(
            ctypes.byref(din), n, p, data_type, int(is_normal), algorithm_type, model_type,
            max_iter, exchange_num, path_type, int(is_warm_start), ic_type, int(is_cv), K, _ip(g_index), g_index.size,
            _dp(state), state.size, _ip(sequence), sequence.size, _dp(lambda_sequence), lambda_sequence.size, s_min,
            s_max, K_max, epsilon, lambda_min, lambda_max, n_lambda, int(is_screening), screening_size, powell_path,
            _ip(always_select), always_select.size, tao, _dp(beta), beta.size, _dp(coef0), coef0.size, _dp(loss),
            loss.size, _dp(ic), ic.size, _dp(nullloss), _dp(aic), aic.size, _dp(bic), bic.size, _dp(gic), gic.size,
            _ip(a_out), a_out.size, _ip(l_out), _ip(x_nan))
        if x_nan[0]:
            raise ValueError(NAN_IN_X)
        _check(rc)
        return beta, coef0, loss, ic, float(nullloss[0]), aic, bic, gic, a_out, int(l_out[0])
    _check(lib().bessx_pywrap_bess(
        _dp(x), n, p, _dp(y), y.size, data_type, _dp(weight), weight.size, int(is_normal), algorithm_type, model_type,
        max_iter, exchange_num, path_type, int(is_warm_start), ic_type, int(is_cv), K, _ip(g_index), g_index.size,
        _dp(state), state.size, _ip(sequence), sequence.size, _dp(lambda_sequence), lambda_sequence.size, s_min, s_max,
        K_max, epsilon, lambda_min, lambda_max, n_lambda, int(is_screening), screening_size, powell_path,
        _ip(always_select), always_select.size, tao, _dp(beta), beta.size, _dp(coef0), coef0.size, _dp(loss),
        loss.size, _dp(ic), ic.size, _dp(nullloss), _dp(aic), aic.size, _dp(bic), bic.size, _dp(gic), gic.size,
        _ip(a_out), a_out.size, _ip(l_out)))
    return beta, coef0, loss, ic, float(nullloss[0]), aic, bic, gic, a_out, int(l_out[0])


def bessCpp(x, y, data_type, weight, is_normal, algorithm_type, model_type, max_iter, exchange_num, path_type,
            is_warm_start, ic_type, is_cv, K, state, sequence, lambda_seq, s_min, s_max, K_max, epsilon, lambda_min,
            lambda_max, nlambda, is_screening, screening_size, powell_path, g_index, always_select, tao):
    """The R-facing entry (src/bess.h:20-33) through the C ABI (bessx_bessCpp): same 30 arguments, x handed over
    column-major like an R matrix; returns the named entries of the list the R build returns."""
    x = np.asfortranarray(x, dtype=np.float64)
    n, p = x.shape
    y, weight, state, lambda_seq = _f64(y).reshape(-1), _f64(weight), _f64(state), _f64(lambda_seq)
    sequence, g_index, always_select = _i32(sequence), _i32(g_index), _i32(always_select)
    cap = sequence.size * lambda_seq.size if path_type == 1 else 2 * (s_max - s_min + 1) + 128
    beta = np.zeros(p)
    beta_all = np.zeros((p, cap), order="F")
    coef0_all, loss_all, ic_all = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    scr = np.zeros(max(screening_size, 1), dtype=np.int32)
    r = RResult()
    r.beta, r.all_capacity = _dp(beta), cap
    r.beta_all, r.coef0_all, r.train_loss_all, r.ic_all, r.screening_A = (_dp(beta_all), _dp(coef0_all), _dp(loss_all),
                                                                         _dp(ic_all), _ip(scr))
    _check(lib().bessx_bessCpp(_dp(x), n, p, _dp(y), data_type, _dp(weight), int(is_normal), algorithm_type, model_type,
                               max_iter, exchange_num, path_type, int(is_warm_start), ic_type, int(is_cv), K, _dp(state),
                               state.size, _ip(sequence), sequence.size, _dp(lambda_seq), lambda_seq.size, s_min, s_max,
                               K_max, epsilon, lambda_min, lambda_max, nlambda, int(is_screening), screening_size,
                               powell_path, _ip(g_index), g_index.size, _ip(always_select), always_select.size, tao,
                               ctypes.byref(r)))
    k = min(r.n_all, cap)
    out = {"beta": beta, "coef0": r.coef0, "train_loss": r.train_loss, "ic": r.ic, "lambda": r.lambda_,
           "beta_all": np.array(beta_all[:, :k]), "coef0_all": coef0_all[:k], "train_loss_all": loss_all[:k],
           "ic_all": ic_all[:k]}
    if path_type == 1:  # list over lambda of p x len(sequence); ic_all as the len(sequence) x len(lambda) matrix
        ns, nl = sequence.size, lambda_seq.size
        out["beta_all"] = [np.array(beta_all[:, j * ns:(j + 1) * ns]) for j in range(nl)]
        out["coef0_all"] = [coef0_all[j * ns:(j + 1) * ns] for j in range(nl)]
        out["train_loss_all"] = [loss_all[j * ns:(j + 1) * ns] for j in range(nl)]
        out["ic_all"] = ic_all[:ns * nl].reshape(nl, ns).T
    if is_screening:
        out["screening_A"] = scr[:screening_size].copy()
    return out


class Session:
    """The state bessCpp builds (Data + Algorithm + Metric, src/bess.cpp:61-165), resident in HBM.

    x in GPU memory (anything with __cuda_array_interface__: 2-D, float64 or float32, any non-negative strides) is read
    where it lies (bessx_session_create_device) and never crosses the bus; y and weight may then be device arrays or
    anything NumPy accepts.  stream: raw handle of the stream the data was produced on (0 = the null stream); row_order:
    a permutation, session row i is row row_order[i] of x (x only; y and weight are in session order).  The caller's
    arrays are free again when the constructor returns.  x_col_major is ignored for a device x (its strides say it)."""

    def __init__(self, x, y, weight=None, data_type=1, is_normal=True, model_type=1, algorithm_type=1, max_iter=20,
                 is_warm_start=True, always_select=(), x_col_major=False, device=-1, g_index=None,
                 is_screening=False, screening_size=0, score_mode=0, max_sparsity=0, stream=0, row_order=None):
        din = None
        if is_device_array(x):
            din, self.n, self.p, _keep = _device_input(x, y, weight, row_order, stream)
            x = y = w = None
        else:
            x = np.asfortranarray(x, dtype=np.float64) if x_col_major else _f64(x)
            self.n, self.p = x.shape
            y = _f64(y).reshape(-1)
            if y.size != self.n:
                raise ValueError("X.shape(0) should be equal to y.size")
            w = None if weight is None else _f64(weight)
        al = _i32(always_select)
        gi = None if g_index is None else _i32(g_index)
        self._gsize_max = 1
        if gi is not None and gi.size:
            self._gsize_max = int(np.max(np.diff(np.append(gi, self.p))))
        pb = Problem(self.n, self.p, _dp(x), int(x_col_major), _dp(y), _dp(w), data_type, int(is_normal), model_type,
                     algorithm_type, max_iter, int(is_warm_start), _ip(al), al.size, device, _ip(gi),
                     0 if gi is None else gi.size, int(is_screening), int(screening_size), int(score_mode),
                     int(max_sparsity))
        h = _vp()
        if din is not None:
            _check_device_route(lib().bessx_session_create_device(ctypes.byref(h), ctypes.byref(pb), ctypes.byref(din)))
        else:
            _check(lib().bessx_session_create(ctypes.byref(h), ctypes.byref(pb)))
        self._h = h
        self.K = 0
        self.is_warm_start = bool(is_warm_start)
        self.p_kept = lib().bessx_session_get_screening(h, None, 0)  # columns the session works on

    def score_mode(self):
        """1 = streaming score pass, 2 = covariance updates (what bessx_problem.score_mode = 0 resolved to)."""
        return int(lib().bessx_session_score_mode(self._h))

    def counters(self):
        """Diagnostics of the covariance form (bessx_session_counter)."""
        names = {0: "chained_fits", 1: "cg_fallbacks", 2: "passes_over_X", 3: "chained_queued", 7: "cv_side_by_side_rounds",
                 8: "cv_union_fills", 9: "tie_rescues", 10: "cache_restarts", 11: "cv_contexts_dropped",
                 12: "cv_fold_contexts", 13: "shared_wide_fills", 14: "kpath_chunked_paths", 15: "kpath_stitch_refits",
                 16: "kpath_chunk_fills", 17: "kpath_chains_last_path",
                 18: "kpath_stitch_giveups", 19: "group_XTX_ns",
                 22: "kpath_coarse_us",
                 23: "kpath_chunks_us", 24: "kpath_stitch_us", 25: "panel_launches_one_group",
                 26: "panel_ns_one_group", 27: "panel_launches_two_groups", 28: "panel_ns_two_groups",
                 29: "shared_pass_launches", 30: "shared_pass_chain_slots", 31: "shared_pass_partial_batches",
                 32: "own_queue_streams_created_by_the_process", 33: "multi_responses_batched",
                 34: "multi_responses_host", 35: "multi_union_fills", 36: "x_bytes_uploaded_from_host",
                 37: "x_bytes_ingested_on_device", 38: "live_device_bytes_of_the_process",
                 39: "live_pinned_bytes_of_the_process", 40: "allocation_requests_of_the_process"}  # (4-6, 20-21: mechanisms removed)
        return {n: int(lib().bessx_session_counter(self._h, i)) for i, n in names.items()}

    def screening(self):
        """screening_A: original column of every kept column."""
        a = np.zeros(self.p_kept, dtype=np.int32)
        lib().bessx_session_get_screening(self._h, _ip(a), a.size)
        return a

    def screening_groups(self):
        """Kept original group numbers after screening with groups of size > 1 (empty otherwise)."""
        n = lib().bessx_session_get_screening_groups(self._h, None, 0)
        a = np.zeros(max(n, 1), dtype=np.int32)
        lib().bessx_session_get_screening_groups(self._h, _ip(a), n)
        return a[:n]

    def screening_scores(self):
        """coef_norm as the selection saw it: one marginal-fit score per original column (per original group when
        screening by groups); DBL_MAX for always_select units; empty for a session created without screening."""
        n = lib().bessx_session_get_screening_scores(self._h, None, 0)
        a = np.zeros(max(n, 1))
        lib().bessx_session_get_screening_scores(self._h, _dp(a), n)
        return a[:n]

    def close(self):
        if getattr(self, "_h", None):
            lib().bessx_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_cv(self, K, fold_id=None, seed=123):
        f = None if fold_id is None else _i32(fold_id)
        _check(lib().bessx_session_set_cv(self._h, K, _ip(f), seed))
        self.K = K

    def cv_folds(self):
        """Test fold of every row as set_cv fixed it (given, or drawn from the seed)."""
        f = np.zeros(self.n, dtype=np.int32)
        _check(lib().bessx_session_get_cv_folds(self._h, _ip(f)))
        return f

    def trace_enable(self, on=True):
        _check(lib().bessx_session_trace_enable(self._h, int(on)))

    def enable_kernel_timing(self, on=True):
        _check(lib().bessx_session_enable_kernel_timing(self._h, int(on)))

    def score_pass_stats(self, reset=False):
        sec, nb, cnt = _d(0), _d(0), _ll(0)
        _check(lib().bessx_session_score_pass_stats(self._h, int(reset), ctypes.byref(sec), ctypes.byref(cnt),
                                                    ctypes.byref(nb)))
        return {"seconds": sec.value, "launches": cnt.value, "algorithmic_bytes": nb.value}

    def submodel_steps(self, reset=False):
        """IRLS / Newton steps of the restricted fits since the last reset (0 for LM)."""
        cnt = _ll(0)
        _check(lib().bessx_session_submodel_steps(self._h, int(reset), ctypes.byref(cnt)))
        return cnt.value

    def normalization(self):
        xm, xn, ym = np.zeros(self.p_kept), np.zeros(self.p_kept), _d(0)
        _check(lib().bessx_session_get_normalization(self._h, _dp(xm), _dp(xn), ctypes.byref(ym)))
        return xm, xn, ym.value

    def _result(self, res, capacity, max_T0):
        """Caller-allocated arrays of one bessx_path_result, bound into res."""
        beta = np.zeros(self.p)
        arr = {
            "cand_T0": np.zeros(capacity, dtype=np.int32), "cand_lambda": np.zeros(capacity),
            "cand_iters": np.zeros(capacity, dtype=np.int32), "cand_train_loss": np.zeros(capacity),
            "cand_ic": np.zeros(capacity), "cand_coef0": np.zeros(capacity),
            "cand_support": np.full((capacity, max_T0), -1, dtype=np.int32), "cand_beta": np.zeros((capacity, max_T0)),
        }
        res.beta = _dp(beta)
        res.capacity = capacity
        res.max_T0 = max_T0
        for k, v in arr.items():
            setattr(res, k, _ip(v) if v.dtype == np.int32 else _dp(v))
        return beta, arr

    def _run(self, call, capacity, max_T0):
        res = PathResult()
        beta, arr = self._result(res, capacity, max_T0)
        _check(call(ctypes.byref(res)))
        return self._collect(res, beta, arr, capacity)

    def _collect(self, res, beta, arr, capacity, trace=None):
        nc = min(res.n_candidates, capacity)
        out = {"beta": beta, "coef0": res.coef0, "train_loss": res.train_loss, "ic": res.ic, "lambda": res.lambda_,
               "best_T0": res.best_T0, "best_iters": res.best_iters, "n_candidates": res.n_candidates,
               "device_seconds": res.device_seconds, "n_fits": res.n_fits, "n_pdas_iters": res.n_pdas_iters}
        for k, v in arr.items():
            out[k] = v[:nc]
        out["trace"] = self._trace() if trace is None else trace
        return out

    def sequential_path(self, sequence, lambda_seq=(0.0,), ic_type=4, is_cv=False):
        seq = _i32(sequence)
        lam = _f64(lambda_seq)
        L = lib()
        return self._run(lambda r: L.bessx_session_sequential_path(self._h, _ip(seq), seq.size, _dp(lam), lam.size,
                                                                   ic_type, int(is_cv), r),
                         seq.size * lam.size, min(self.p, (int(seq.max()) if seq.size else 1) * self._gsize_max))

    def set_responses(self, Y, stream=0):
        """R extra responses for this session's design (bessx_session_set_responses): Y is n x R; every column is
        prepared like the session's own y.  Replaces an earlier set; the session's own y stays.  Y may be a device
        array (float64 / float32, any strides; stream: the stream it was produced on)."""
        if is_device_array(Y):
            dY = _DeviceArray(Y, "Y")
            shape = dY.shape if len(dY.shape) == 2 else (dY.shape[0], 1)
            strides = dY.strides if len(dY.shape) == 2 else (dY.strides[0], 0)
            if shape[0] != self.n:
                raise ValueError("Y must have shape (n, R) with n = %d rows" % self.n)
            rc = lib().bessx_session_set_responses_device(self._h, dY.ptr, dY.dtype, strides[0], strides[1], shape[1],
                                                          int(stream) if stream else None)
            if rc == 1 and "NaN" in last_error():
                raise ValueError("Y contains NaN")
            _check(rc)
            self._n_responses = shape[1]
            return
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y.reshape(-1, 1)
        if Y.ndim != 2 or Y.shape[0] != self.n:
            raise ValueError("Y must have shape (n, R) with n = %d rows" % self.n)
        if np.isnan(Y).any():
            raise ValueError("Y contains NaN")
        Yc = np.asfortranarray(Y)
        _check(lib().bessx_session_set_responses(self._h, _dp(Yc), Yc.shape[1], 1))
        self._n_responses = Yc.shape[1]

    def sequential_path_multi(self, sequence, lambda_seq=(0.0,), ic_type=4):
        """sequential_path once per response of set_responses (bessx_session_sequential_path_multi): a list with what
        sequential_path returns, one entry per column of Y."""
        R = getattr(self, "_n_responses", 0)
        if R < 1:
            raise ValueError("call set_responses first")
        seq, lam = _i32(sequence), _f64(lambda_seq)
        capacity = seq.size * lam.size
        max_T0 = min(self.p, (int(seq.max()) if seq.size else 1) * self._gsize_max)
        results = (PathResult * R)()
        bufs = [self._result(results[r], capacity, max_T0) for r in range(R)]
        _check(lib().bessx_session_sequential_path_multi(self._h, _ip(seq), seq.size, _dp(lam), lam.size, ic_type, 0,
                                                         results))
        trace = self._trace()
        out = []
        for r in range(R):
            o = self._collect(results[r], bufs[r][0], bufs[r][1], capacity, trace)
            out.append(o)
        return out

    def sequential_path_chain(self, sequence, lambda_seq=(0.0,), ic_type=4, is_cv=False, init_idx=(), init_val=(),
                              init_coef0=0.0, keep_caches=False, stop_support=None, stop_beta=None, stop_rtol=1e-9,
                              lead_levels=()):
        """sequential_path as one link of a longer warm-start chain (bessx_session_sequential_path_chain): starts from
        the given (normalised) model, optionally on the caches of the previous call, and stops after the first
        candidate that equals the caller's own row of stop_support / stop_beta.  Adds to the path result: stopped_at,
        last_idx / last_val / last_coef0 (the model the next candidate of the chain starts from)."""
        seq, lam = _i32(sequence), _f64(lambda_seq)
        ii, iv = _i32(init_idx), _f64(init_val)
        max_T0 = min(self.p, (int(seq.max()) if seq.size else 1) * self._gsize_max)
        ch = PathChain()
        ch.init_idx, ch.init_val, ch.init_len, ch.init_coef0 = _ip(ii), _dp(iv), ii.size, float(init_coef0)
        ch.keep_caches = int(bool(keep_caches))
        lead = _i32(lead_levels)  # (bessx_path_chain.lead_levels: a coarse warm-start chain in front of the link)
        ch.lead_levels, ch.lead_len = (_ip(lead), lead.size) if lead.size else (None, 0)
        ss = sb = None
        if stop_support is not None:
            ss = np.full((len(stop_support), max_T0), -1, dtype=np.int32)
            sb = np.zeros((len(stop_support), max_T0))
            for r, row in enumerate(stop_support):
                row = np.asarray(row)
                row = row[row >= 0]
                ss[r, :row.size] = row
                if stop_beta is not None:
                    sb[r, :row.size] = np.asarray(stop_beta[r])[:row.size]
            ch.stop_support, ch.stop_rows, ch.stop_row_len, ch.stop_rtol = _ip(ss), ss.shape[0], max_T0, float(stop_rtol)
            ch.stop_beta = _dp(sb) if stop_beta is not None else None
        li, lv = np.zeros(max_T0, dtype=np.int32), np.zeros(max_T0)
        ch.last_idx, ch.last_val, ch.last_cap = _ip(li), _dp(lv), max_T0
        L = lib()
        out = self._run(lambda r: L.bessx_session_sequential_path_chain(self._h, _ip(seq), seq.size, _dp(lam), lam.size,
                                                                        ic_type, int(is_cv), ctypes.byref(ch), r),
                        seq.size * lam.size, max_T0)
        n_last = min(ch.last_len, max_T0)
        out.update({"stopped_at": int(ch.stopped_at), "last_idx": li[:n_last].copy(), "last_val": lv[:n_last].copy(),
                    "last_coef0": float(ch.last_coef0)})
        return out

    def cv_eval(self, T0, lam=0.0, want_full=True, init_idx=(), init_val=(), init_coef0=0.0, folds=()):
        """One cross-validated candidate restricted to `folds` (ascending), the full-data fit in front when want_full
        (bessx_session_cv_eval).  Returns the list of fit records [full,] fold..., each like fit()'s."""
        ii, iv, fo = _i32(init_idx), _f64(init_val), _i32(folds)
        w = self.fit_width(T0)
        nrec = int(bool(want_full)) + fo.size
        sup, b = np.zeros((max(nrec, 1), w), dtype=np.int32), np.zeros((max(nrec, 1), w))
        c0, tr, te = np.zeros(max(nrec, 1)), np.zeros(max(nrec, 1)), np.zeros(max(nrec, 1))
        it = np.zeros(max(nrec, 1), dtype=np.int32)
        _check(lib().bessx_session_cv_eval(self._h, int(T0), float(lam), int(bool(want_full)), _ip(ii), _dp(iv), ii.size,
                                           float(init_coef0), _ip(fo), fo.size, _ip(sup), _dp(b), _dp(c0), _ip(it),
                                           _dp(tr), _dp(te)))
        recs = []
        for r in range(nrec):
            keep = sup[r] >= 0
            recs.append({"support": sup[r][keep], "beta": b[r][keep], "coef0": float(c0[r]), "iters": int(it[r]),
                         "train_loss": float(tr[r]), "test_loss": float(te[r])})
        return recs

    # ---- cooperative prefill of the Gram column cache (bessx_session_cov_prefill_*) ----
    def marginal_scores(self):
        bd = np.zeros(self.p_kept)
        _check(lib().bessx_session_marginal_scores(self._h, _dp(bd)))
        return bd

    def cov_prefill_begin(self, cols):
        c = _i32(cols)
        _check(lib().bessx_session_cov_prefill_begin(self._h, _ip(c), c.size))

    def cov_prefill_extend(self, cols):
        c = _i32(cols)
        _check(lib().bessx_session_cov_prefill_extend(self._h, _ip(c), c.size))

    def cov_state(self):
        """(scores of the last fit's last PDAS iteration, cache slot of every column or -1)."""
        bd, so = np.zeros(self.p_kept), np.zeros(self.p_kept, dtype=np.int32)
        _check(lib().bessx_session_cov_state(self._h, _dp(bd), _ip(so)))
        return bd, so

    def cov_cache_columns(self, row_set, cols):
        """(G, cached): the Gram columns row set `row_set` (0 = all rows, k + 1 = training rows of fold k) holds cached
        for `cols`, p x len(cols), and which of them it holds (bool); columns of G that are not cached are NaN.
        Read-only (bessx_session_cov_cache_columns)."""
        c = _i32(cols)
        out = np.full((c.size, self.p_kept), np.nan)
        hit = np.zeros(c.size, dtype=np.int32)
        _check(lib().bessx_session_cov_cache_columns(self._h, int(row_set), _ip(c), c.size, _dp(out), _ip(hit)))
        return out.T.copy(), hit.astype(bool)

    SCORE_STATE_HEAD = ("done", "l", "T0", "k_cur", "d_fresh", "info", "cov_miss", "fast_same", "serial", "row_set",
                        "bmm_owner", "score_mode", "U", "nrb", "n", "p", "sums_are_d", "known", "has_inA", "ahead")

    def score_state(self, ctx=-1):
        """The score state in device memory, read-only (bessx_session_score_state): the control block's fields and the
        host's record of the fit it describes (SCORE_STATE_HEAD, "lambda"), the model (A_cur, b_cur, beta_dense, inA), the
        scores bd, the sums they were formed from ("d": p values in the covariance form; "part": nrb x p row-block
        partials and "r": the residual the pass read, in the streaming form) and cov_bmm as (min inside, max outside,
        column of that max) per block of 32 columns.  ctx >= 0: fold context ctx of the side-by-side CV chains."""
        p, n = self.p_kept, self.n
        head, lam = np.zeros(len(self.SCORE_STATE_HEAD), dtype=np.int32), _d(0)
        _check(lib().bessx_session_score_state(self._h, int(ctx), _ip(head), ctypes.byref(lam), None, None, None, None,
                                               None, None, None, None))
        st = {k: int(v) for k, v in zip(self.SCORE_STATE_HEAD, head)}
        A, b, beta, bd = np.zeros(p, dtype=np.int32), np.zeros(p), np.zeros(p), np.zeros(p)
        inA, r = np.zeros(p, dtype=np.uint8), np.zeros(n)
        sums = np.zeros((1 if st["sums_are_d"] else st["nrb"]) * p)
        nb = (p + 31) // 32
        bmm = np.zeros(3 * nb)
        _check(lib().bessx_session_score_state(self._h, int(ctx), _ip(head), ctypes.byref(lam), _ip(A), _dp(b), _dp(beta),
                                               inA.ctypes.data_as(_vp), _dp(bd), _dp(sums), _dp(r), _dp(bmm)))
        st = {k: int(v) for k, v in zip(self.SCORE_STATE_HEAD, head)}
        k = max(0, min(st["k_cur"], p))
        st.update({"lambda": lam.value, "A_cur": A[:k].copy(), "b_cur": b[:k].copy(), "beta_dense": beta,
                   "inA": inA.astype(bool), "bd": bd, "r": r,
                   "bmm_min": bmm[0:2 * nb:2].copy(), "bmm_max": bmm[1:2 * nb:2].copy(), "bmm_arg": bmm[2 * nb:].copy()})
        st["d" if st["sums_are_d"] else "part"] = sums if st["sums_are_d"] else sums.reshape(st["nrb"], p)
        return st

    def cv_fill_geometry(self):
        """How the CV row sets' Gram fills run (bessx_session_cv_fill_geometry): shared fills or masked ones, and the
        geometry of the fold-major copy (0 unless shared)."""
        g = np.zeros(4, dtype=np.int32)
        _check(lib().bessx_session_cv_fill_geometry(self._h, _ip(g)))
        return {"shared": bool(g[0]), "cvp_nsl": int(g[1]), "cvp_rps": int(g[2]), "copy_rows": int(g[3])}

    def cov_prefill_compute(self, g0, ngroups):
        _check(lib().bessx_session_cov_prefill_compute(self._h, int(g0), int(ngroups)))

    def cov_prefill_export(self, g0, ngroups, device_ptr=None):
        """The p x 32 blocks of groups g0 .. g0+ngroups-1: into device memory at device_ptr, or returned as an array."""
        if device_ptr is not None:
            _check(lib().bessx_session_cov_prefill_export(self._h, int(g0), int(ngroups), _vp(int(device_ptr)), 1))
            return None
        out = np.empty(int(ngroups) * 32 * self.p_kept)
        _check(lib().bessx_session_cov_prefill_export(self._h, int(g0), int(ngroups), out.ctypes.data_as(_vp), 0))
        return out

    def cov_prefill_import(self, g0, ngroups, blocks=None, device_ptr=None):
        if device_ptr is not None:
            _check(lib().bessx_session_cov_prefill_import(self._h, int(g0), int(ngroups), _vp(int(device_ptr)), 1))
            return
        b = _f64(blocks)
        assert b.size == int(ngroups) * 32 * self.p_kept
        _check(lib().bessx_session_cov_prefill_import(self._h, int(g0), int(ngroups), b.ctypes.data_as(_vp), 0))

    def cov_prefill_end(self):
        _check(lib().bessx_session_cov_prefill_end(self._h))

    def set_kpath_chains(self, chains):
        """Chunk chains of sequential_path (bessx_session_set_kpath_chains): 0 automatic, 1 one chain, 2..8."""
        _check(lib().bessx_session_set_kpath_chains(self._h, int(chains)))

    _FILL_HOOK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int)

    def set_fill_hook(self, fn, width=0):
        """Shared wide fills inside a fit (bessx_session_set_fill_hook): while set, a parked fit of the all-rows row set
        lists `width` columns -- the missing ones, then the best uncached ones by the current scores -- and calls
        fn(n_groups), which forms its share, exchanges the blocks and closes the list (cov_prefill_compute / export /
        import / end).  fn = None: private fills again.  An exception in fn fails the fit and is re-raised by it."""
        self._hook_error = None
        if fn is None:
            _check(lib().bessx_session_set_fill_hook(self._h, ctypes.cast(None, self._FILL_HOOK), None, 0))
            self._hook_ref = None
            return

        def tramp(_user, ng):
            try:
                fn(int(ng))
                return 0
            except BaseException as e:  # (an exception must not cross the C frames)
                self._hook_error = e
                return 1

        ref = self._FILL_HOOK(tramp)
        _check(lib().bessx_session_set_fill_hook(self._h, ref, None, int(width)))
        self._hook_ref = ref  # (kept alive as long as the library may call it)

    def debug_block_stream(self, milliseconds):
        """Test hook: everything queued on the session's stream waits behind a host function that sleeps."""
        _check(lib().bessx_session_debug_block_stream(self._h, int(milliseconds)))

    def gs_path(self, s_min, s_max, ic_type=4, is_cv=False):
        L = lib()
        return self._run(lambda r: L.bessx_session_gs_path(self._h, s_min, s_max, ic_type, int(is_cv), r),
                         2 * (s_max - s_min + 1) + 64, min(self.p, max(s_max, 1) * self._gsize_max))

    def pgs_path(self, s_min, s_max, lambda_min, lambda_max, n_lambda=100, powell_path=1, ic_type=4, is_cv=False):
        L = lib()
        return self._run(lambda r: L.bessx_session_pgs_path(self._h, s_min, s_max, lambda_min, lambda_max, n_lambda,
                                                            powell_path, ic_type, int(is_cv), r), 128,
                         min(self.p, max(s_max, 1) * self._gsize_max))

    def fit(self, T0, lam=0.0, fold=-1, init_idx=(), init_val=(), init_coef0=0.0):
        ii, iv = _i32(init_idx), _f64(init_val)
        w = self.fit_width(T0)  # T0 columns, or the columns of the T0 widest groups (groups of size > 1)
        sup, b = np.zeros(w, dtype=np.int32), np.zeros(w)
        c0, tr, te, it = _d(0), _d(0), _d(0), _i(0)
        _check(lib().bessx_session_fit(self._h, T0, lam, fold, _ip(ii), _dp(iv), ii.size, init_coef0, _ip(sup),
                                       _dp(b), ctypes.byref(c0), ctypes.byref(it), ctypes.byref(tr),
                                       ctypes.byref(te)))
        keep = sup >= 0  # (with groups the selected columns may be fewer than the width)
        return {"support": sup[keep], "beta": b[keep], "coef0": c0.value, "iters": it.value, "train_loss": tr.value,
                "test_loss": te.value}

    def fit_width(self, T0):
        """Most columns a fit of sparsity level T0 returns (bessx_session_fit_width)."""
        w = int(lib().bessx_session_fit_width(self._h, int(T0)))
        if w < 0:
            raise BessxError(1, "sparsity level outside [1, number of groups]")
        return w

    def reset_caches(self):
        """Start cold, like a path call does (bessx_session_reset_caches)."""
        _check(lib().bessx_session_reset_caches(self._h))

    def _trace(self):
        L = lib()

        def geti(which):
            n = L.bessx_session_trace_size(self._h, which)
            a = np.zeros(max(n, 1), dtype=np.int32)
            _check(L.bessx_session_trace_copy_int(self._h, which, _ip(a)))
            return a[:n]

        def getd(which):
            n = L.bessx_session_trace_size(self._h, which)
            a = np.zeros(max(n, 1))
            _check(L.bessx_session_trace_copy_double(self._h, which, _dp(a)))
            return a[:n]

        meta = geti(0).reshape(-1, 4)
        if meta.shape[0] == 0:
            return None
        a_flat, beta_flat, coef0_calls = geti(1), getd(2), getd(3)
        fits = []
        for c, (l, T0, train_n, off) in enumerate(meta):
            if l == 1:
                fits.append({"T0": int(T0), "train_n": int(train_n), "iters": [], "betas": [], "coef0s": []})
            nxt = meta[c + 1][3] if c + 1 < len(meta) else a_flat.size
            fits[-1]["iters"].append(a_flat[off:nxt].copy())
            fits[-1]["betas"].append(beta_flat[off:nxt].copy())
            fits[-1]["coef0s"].append(float(coef0_calls[c]))
        return {"fits": fits, "loss_calls": getd(4), "ic_calls": getd(5)}


# ---- single-kernel entry points (parity tests) -------------------------------------------------
def op_xtv(x, v, v2=None):
    x = np.asfortranarray(x, dtype=np.float64)
    n, p = x.shape
    v = _f64(v)
    out, out2 = np.zeros(p), np.zeros(p)
    v2a = None if v2 is None else _f64(v2)
    _check(lib().bessx_op_xtv(_dp(x), n, p, n, _dp(v), _dp(v2a), _dp(out), _dp(out2)))
    return (out, out2) if v2 is not None else out


def op_xtv_multi(x, vs, v2s=None):
    """X^T v for the rows of vs (nc x n) in one pass over X; with v2s also X^2^T v2."""
    x = np.asfortranarray(x, dtype=np.float64)
    n, p = x.shape
    vs = np.ascontiguousarray(vs, dtype=np.float64)
    nc = vs.shape[0]
    out, out2 = np.zeros((nc, p)), np.zeros((nc, p))
    v2a = None if v2s is None else np.ascontiguousarray(v2s, dtype=np.float64)
    _check(lib().bessx_op_xtv_multi(_dp(x), n, p, n, _dp(vs), _dp(v2a), nc, _dp(out), _dp(out2)))
    return (out, out2) if v2s is not None else out


def _cox_op_args(x, status, weight, mask, cols, b):
    x = np.asfortranarray(x, dtype=np.float64)
    cols = _i32(cols).reshape(-1)
    return (x, _f64(status), None if weight is None else _f64(weight), None if mask is None else _f64(mask), cols,
            _f64(b))


def op_cox_state(x, status, cols, b, weight=None, mask=None):
    """The Cox state pass alone for the model (cols, b) on rows in time order (bessx_op_cox_state): a dict of
    e, theta, s0, rs0, s_all, s_test (n each; s_test None without a mask) and loss = (all rows, test rows)."""
    x, st, w, mk, cols, b = _cox_op_args(x, status, weight, mask, cols, b)
    n, p = x.shape
    out = {k: np.zeros(n) for k in ("e", "theta", "s0", "rs0", "s_all", "s_test")}
    loss = np.zeros(2)
    _check(lib().bessx_op_cox_state(_dp(x), n, p, _dp(st), _dp(w), _dp(mk), _ip(cols), cols.size, _dp(b),
                                    *[_dp(out[k]) for k in ("e", "theta", "s0", "rs0", "s_all", "s_test")], _dp(loss)))
    if mk is None:
        out["s_test"] = None
    out["loss"] = loss
    return out


def op_cox_score(x, status, cols, b, lam=0.0, form=1, weight=None, mask=None):
    """Cox sacrifice scores bd (p) of the model (cols, b); form 0 = two passes over X, 1 = one pass."""
    x, st, w, mk, cols, b = _cox_op_args(x, status, weight, mask, cols, b)
    n, p = x.shape
    bd = np.zeros(p)
    _check(lib().bessx_op_cox_score(_dp(x), n, p, _dp(st), _dp(w), _dp(mk), _ip(cols), cols.size, _dp(b), float(lam),
                                    int(form), _dp(bd)))
    return bd


def op_cox_score_multi(x, status, cols, bs, lam=0.0, weight=None, mask=None):
    """... of the nc models (cols, bs[c]) in one pass over X (k_cox_score1p_mc): nc x p."""
    x, st, w, mk, cols, bs = _cox_op_args(x, status, weight, mask, cols, bs)
    n, p = x.shape
    bs = np.ascontiguousarray(np.atleast_2d(bs))
    nc = bs.shape[0]
    bd = np.zeros((nc, p))
    _check(lib().bessx_op_cox_score_multi(_dp(x), n, p, _dp(st), _dp(w), _dp(mk), _ip(cols), cols.size, _dp(bs), nc,
                                          float(lam), _dp(bd)))
    return bd


def op_glm_gh(family, x, y, cols, b, coef0=0.0, lam=0.0, weight=None, mask=None, want_bd=True):
    """The logistic (family 2) / Poisson (3) gradient and curvature pass alone for the model (cols, b, coef0)
    (bessx_op_glm_gh): a dict of g, h (n each), loss = (all rows, test rows) and, with want_bd, the scores bd (p)."""
    x, y, w, mk, cols, b = _cox_op_args(x, y, weight, mask, cols, b)
    n, p = x.shape
    out = {"g": np.zeros(n), "h": np.zeros(n), "loss": np.zeros(2), "bd": np.zeros(p) if want_bd else None}
    _check(lib().bessx_op_glm_gh(int(family), _dp(x), n, p, _dp(y), _dp(w), _dp(mk), _ip(cols), cols.size, _dp(b),
                                 float(coef0), float(lam), _dp(out["g"]), _dp(out["h"]), _dp(out["loss"]), _dp(out["bd"])))
    return out


def op_glm_irls(family, x, y, cols, bcur, route=-1, t=0, wfloor=1, lam=0.0, rows_per_slab=0, weight=None, mask=None,
                want_bnext=True):
    """One IRLS step from the iterate bcur (intercept first) on [1, x[:, cols]] (bessx_op_glm_irls): a dict of gram
    ((T0 + 2)^2, the working response last), ll, bnext (T0 + 1; None without want_bnext: the step's system is not solved),
    route (the one that ran: 1 fused, 0 five launches) and, from route 0 only, wv and z (n each; None from the fused step)."""
    x, y, w, mk, cols, bcur = _cox_op_args(x, y, weight, mask, cols, bcur)
    n, p = x.shape
    T0 = cols.size
    assert bcur.size == T0 + 1
    gram = np.zeros((T0 + 2, T0 + 2), order="F")
    wv, z, bnext, ll, taken = np.zeros(n), np.zeros(n), (np.zeros(T0 + 1) if want_bnext else None), _d(0), _i(-1)
    _check(lib().bessx_op_glm_irls(int(family), int(route), int(t), int(wfloor), float(lam), int(rows_per_slab), _dp(x), n,
                                   p, _dp(y), _dp(w), _dp(mk), _ip(cols), T0, _dp(bcur), _dp(gram), ctypes.byref(ll),
                                   _dp(wv), _dp(z), _dp(bnext), ctypes.byref(taken)))
    five = taken.value == 0
    return {"gram": np.array(gram), "ll": ll.value, "bnext": bnext, "route": taken.value, "wv": wv if five else None,
            "z": z if five else None}


def _group_op_layout(gidx, p):
    gidx = _i32(gidx).reshape(-1)
    sizes = np.diff(np.concatenate([gidx, [p]])).astype(np.int64)
    return gidx, sizes, np.concatenate([[0], np.cumsum(sizes * sizes)])


def _flags(always, N):
    if always is None:
        return None, None
    fl = np.ascontiguousarray(always, dtype=np.uint8).reshape(-1)
    assert fl.size == N
    return fl, fl.ctypes.data_as(_vp)


def op_group_scores(x, gidx, beta_dense, w1=None, w2=None, lm=False, n_t=1.0, lam=0.0, always=None, part=None,
                    dcol=None, cshift=0, p=None):
    """The group moment and score kernels alone (bessx_op_group_scores): a dict of mblk (list of the N blocks, s x s
    each), mblk_flat, dcol (p; given as `dcol`, zeros without, and overwritten only where w2 is given) and bd (3 x N: row
    m = eig_mode m).  gidx: the groups' first columns; part: nrb x p (lm).  With cshift > 0, x holds the columns from
    cshift on only (p then has to be given) and the groups before that column are not launched."""
    x = np.asfortranarray(x, dtype=np.float64)
    n = x.shape[0]
    p = x.shape[1] + int(cshift) if p is None else int(p)
    assert x.shape[1] == p - int(cshift)
    gidx, sizes, off = _group_op_layout(gidx, p)
    N = gidx.size
    beta = _f64(beta_dense).reshape(-1)
    assert beta.size == p
    w1 = None if w1 is None else _f64(w1)
    w2 = None if w2 is None else _f64(w2)
    nrb = 0
    if part is not None:
        part = np.ascontiguousarray(np.atleast_2d(part), dtype=np.float64)
        assert part.shape[1] == p
        nrb = part.shape[0]
    dc = np.zeros(p) if dcol is None else np.array(dcol, dtype=np.float64).reshape(-1)
    assert dc.size == p
    flat, bd = np.zeros(max(int(off[-1]), 1)), np.zeros((3, N))
    fl, flp = _flags(always, N)
    _check(lib().bessx_op_group_scores(_dp(x), n, p, int(cshift), _ip(gidx), N, _dp(w1), _dp(w2), _dp(beta), int(bool(lm)),
                                       float(n_t), float(lam), flp, _dp(part), nrb, _dp(flat), _dp(dc), _dp(bd)))
    blocks = [flat[off[g]:off[g + 1]].reshape(sizes[g], sizes[g], order="F").copy() for g in range(N)]
    return {"mblk": blocks, "mblk_flat": flat[:int(off[-1])], "dcol": dc, "bd": bd}


def op_group_lsq(x, gidx, yw, always=None):
    """Grouped LM screening alone (bessx_op_group_lsq): score (N) = |(X_g^T X_g)^-1 X_g^T yw|^2 / s_g."""
    x = np.asfortranarray(x, dtype=np.float64)
    n, p = x.shape
    gidx, _, _ = _group_op_layout(gidx, p)
    yw = _f64(yw)
    assert yw.size == n
    score = np.zeros(gidx.size)
    fl, flp = _flags(always, gidx.size)
    _check(lib().bessx_op_group_lsq(_dp(x), n, p, _ip(gidx), gidx.size, _dp(yw), flp, _dp(score)))
    return score


def op_glm_irls_geometry(T0, n):
    """(padded rows, tile rows, chunks per group of the fused kernel or 0, the solver's rows per slab) of an IRLS step at
    sparsity level T0 on n rows (bessx_op_glm_irls_geometry; needs no device)."""
    out = np.zeros(4, dtype=np.int32)
    _check(lib().bessx_op_glm_irls_geometry(int(T0), int(n), _ip(out)))
    return tuple(int(v) for v in out)


def op_topk(score, k):
    score = _f64(score)
    out = np.zeros(max(k, 1), dtype=np.int32)
    _check(lib().bessx_op_topk(_dp(score), score.size, k, _ip(out)))
    return out[:k]


def op_gram(x, cols, w=None):
    x = np.asfortranarray(x, dtype=np.float64)
    n, p = x.shape
    cols = _i32(cols)
    wa = None if w is None else _f64(w)
    out = np.zeros((cols.size, cols.size), order="F")
    _check(lib().bessx_op_gram(_dp(x), n, p, n, _ip(cols), cols.size, _dp(wa), _dp(out)))
    return np.array(out)


def op_chol_solve(a, b):
    a = np.asfortranarray(a, dtype=np.float64)
    b = _f64(b)
    sol = np.zeros(b.size)
    _check(lib().bessx_op_chol_solve(_dp(a), b.size, _dp(b), _dp(sol)))
    return sol


def op_normalize(x, y, weight, data_type, is_normal=True, add_weight=False):
    x = np.array(x, dtype=np.float64, order="F")
    n, p = x.shape
    y = np.array(y, dtype=np.float64)
    w = _f64(weight)
    xm, xn, ym = np.zeros(p), np.zeros(p), _d(0)
    _check(lib().bessx_op_normalize(_dp(x), n, p, _dp(y), _dp(w), data_type, int(is_normal), int(add_weight),
                                    _dp(xm), _dp(xn), ctypes.byref(ym)))
    return x, y, xm, xn, ym.value


def op_stream_copy_gbps(nbytes=1 << 30, repeats=10):
    g = _d(0)
    _check(lib().bessx_op_stream_copy_gbps(nbytes, repeats, ctypes.byref(g)))
    return g.value


def _ingest_args(x, row_order):
    dx = _DeviceArray(x, "x")
    shape = dx.shape if len(dx.shape) == 2 else (dx.shape[0], 1)
    strides = dx.strides if len(dx.shape) == 2 else (dx.strides[0], 0)
    ro = None
    if row_order is not None:
        ro = _i32(row_order).reshape(-1)
        if ro.size != shape[0]:
            raise ValueError("row_order must have one entry per row")
    return dx, shape, strides, ro


def padded_rows(n):
    """Leading dimension of a session's matrix for n rows (bessx_session_create: row blocks of 128 * U)."""
    rb = 128 * (8 if n >= 4096 else (4 if n >= 2048 else (2 if n >= 1024 else 1)))
    return (n + rb - 1) // rb * rb


def op_ingest(x, row_order=None, ld=None, stream=0):
    """The ingest kernel alone on a device array x (n x p): (the zero-padded column-major fp64 image as an (ld, p)
    Fortran-ordered host array, NaN flag)."""
    dx, (n, p), (rs, cs), ro = _ingest_args(x, row_order)
    ld = padded_rows(n) if ld is None else int(ld)
    out = np.empty((ld, p), order="F")
    flag = np.zeros(1, dtype=np.int32)
    _check(lib().bessx_op_ingest(dx.ptr, dx.dtype, rs, cs, _ip(ro), n, p, ld, int(stream) if stream else None, _dp(out),
                                 _ip(flag)))
    return out, bool(flag[0])


def device_to_host(a, stream=0):
    """A device array (1-D or 2-D, float64 / float32) as a float64 host array of the same shape, through the ingest
    kernel -- for the n-value vectors (y, weight) of the estimators; no torch needed."""
    shape = _DeviceArray(a, "array").shape
    out, _ = op_ingest(a, ld=(shape[0] + 127) // 128 * 128, stream=stream)
    return np.ascontiguousarray(out[:shape[0]]).reshape(shape)


def op_ingest_bench(x, row_order=None, repeats=20):
    """(ms per launch, GB/s of bytes read + written) of the ingest kernel on the device array x, device events."""
    dx, (n, p), (rs, cs), ro = _ingest_args(x, row_order)
    ms, g = _d(0), _d(0)
    _check(lib().bessx_op_ingest_bench(dx.ptr, dx.dtype, rs, cs, _ip(ro), n, p, padded_rows(n), repeats,
                                       ctypes.byref(ms), ctypes.byref(g)))
    return ms.value, g.value


LINKS = {"identity": 0, "logistic": 1, "poisson": 2}  # BESSX_LINK_*


def _predict_model(dx, cols, B=None, coef0=None):
    """(cols int32, B float64 (m, R) or None, coef0 float64 (R,) or None) of a model for the device matrix dx, checked."""
    p = dx.shape[1]
    cols = _i32(cols).reshape(-1)
    if cols.size and (cols.min() < 0 or cols.max() >= p):
        raise ValueError("cols: column numbers must lie in [0, %d)" % p)
    if cols.size > 1 and (np.diff(cols) <= 0).any():
        raise ValueError("cols must be ascending and distinct")
    if B is None:
        return cols, None, None
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 1:
        B = B.reshape(-1, 1)
    if B.ndim != 2 or B.shape[0] != cols.size or B.shape[1] < 1:
        raise ValueError("B must have shape (len(cols), R) = (%d, R) with R >= 1, got %s" % (cols.size, B.shape))
    coef0 = _f64(coef0).reshape(-1)
    if coef0.size != B.shape[1]:
        raise ValueError("coef0 must have one entry per response (%d), got %d" % (B.shape[1], coef0.size))
    return cols, np.ascontiguousarray(B), coef0


def predict_device(x, cols, B, coef0, link="identity", out=None, stream=0):
    """Prediction on a device matrix x (n x p: float64 or float32, any non-negative strides) that is read where it lies
    (bessx_predict_device): link(x[:, cols] @ B + coef0) from the support columns alone.  cols: ascending distinct column
    numbers (may be empty); B: (len(cols), R) or (len(cols),); coef0: R values; link: "identity", "logistic" or "poisson".
    Returns the linear predictor (identity), (pr, labels) (logistic) or exp(eta) (poisson), each of shape (n,) when B is
    1-D, else (n, R).  out: a float64 device array of that shape to write into (for the logistic link a pair of them with
    equal strides); out=None allocates a torch tensor on x's device when x is a torch tensor (torch is looked up, never
    imported), and returns NumPy arrays for any other device object.  stream: raw handle of the stream x was produced
    on; the results are complete when the call returns."""
    dx = _DeviceArray(x, "x", 2)
    n = dx.shape[0]
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    one_d = np.ndim(B) == 1
    cols, B, coef0 = _predict_model(dx, cols, B, coef0)
    R = B.shape[1]
    shape = (n,) if one_d else (n, R)
    two = link == "logistic"
    outs = None
    if out is not None:
        outs = list(out) if two and isinstance(out, (tuple, list)) else [out]
        if two and len(outs) != 2:
            raise ValueError("out: the logistic link writes a pair (pr, labels)")
        douts = []
        for o in outs:
            if not is_device_array(o):
                raise ValueError("out must be a device array")
            do = _DeviceArray(o, "out")
            if do.item != 8:
                raise ValueError("out: a device array of float64 is needed (typestr '<f8')")
            if do.shape != shape and not (R == 1 and do.shape in ((n,), (n, 1))):
                raise ValueError("out must have shape %s, got %s" % (shape, do.shape))
            douts.append(do)
        if two and douts[0].strides != douts[1].strides:
            raise ValueError("out: pr and labels must have equal strides")
        st = douts[0].strides
        ors, ocs = st[0], (st[1] if len(st) == 2 else 1)
        ptrs, on_device, result = [d.ptr for d in douts], 1, outs
    else:
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(x, torch.Tensor):
            result = [torch.empty(shape, dtype=torch.float64, device=x.device) for _ in range(2 if two else 1)]
            ptrs, on_device = [int(t.data_ptr()) for t in result], 1
        else:
            result = [np.empty(shape) for _ in range(2 if two else 1)]
            ptrs, on_device = [int(a.ctypes.data) for a in result], 0
        ors, ocs = R, 1
    _check(lib().bessx_predict_device(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], n, dx.shape[1], _ip(cols),
                                      cols.size, _dp(B), _dp(coef0), R, LINKS[link], ptrs[0], ors, ocs,
                                      ptrs[1] if two else None, on_device, int(stream) if stream else None))
    return tuple(result) if two else result[0]


def op_predict_bench(x, cols, R=1, link="identity", repeats=20):
    """(ms per launch, GB/s of n * m * item bytes read + n * R * 8 written) of the prediction kernel on the device
    matrix x for the support cols and R responses, device events."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms, g = _d(0), _d(0)
    _check(lib().bessx_op_predict_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                        _ip(cols), cols.size, int(R), LINKS[link], repeats, ctypes.byref(ms),
                                        ctypes.byref(g)))
    return ms.value, g.value


def process_counters():
    """The ledger of the library's GPU resources in this process (bessx_session_counter 38-40, no session needed)."""
    L = lib()
    return {"live_device_bytes": int(L.bessx_session_counter(None, 38)),
            "live_pinned_bytes": int(L.bessx_session_counter(None, 39)),
            "allocation_requests": int(L.bessx_session_counter(None, 40))}


def _eval_y(y, n, R):
    """y of evaluate_device as (host array or None, _DeviceArray or None, row stride, column stride, y_cols), checked:
    n values (one column for every model) or an (n, R) array (one column per model)."""
    if is_device_array(y):
        dy = _DeviceArray(y, "y")
        shape, strides, host = dy.shape, dy.strides, None
    else:
        host = np.asarray(y, dtype=np.float64)
        if host.ndim < 1 or host.ndim > 2:
            raise ValueError("y must be 1-D or 2-D, got shape %s" % (host.shape,))
        host = np.ascontiguousarray(host)
        dy, shape, strides = None, host.shape, tuple(v // 8 for v in host.strides)
    if shape[0] != n:
        raise ValueError("X.shape(0) should be equal to y.shape(0): %d rows, y has shape %s" % (n, shape))
    y_cols = shape[1] if len(shape) == 2 else 1
    if y_cols != 1 and y_cols != R:
        raise ValueError("y must have 1 column or one per model (%d), got %d" % (R, y_cols))
    return host, dy, strides[0], (strides[1] if len(shape) == 2 else 0), y_cols


def _set_x(a, dx):
    """The fields of the device matrix, which every input struct begins with."""
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride = dx.ptr, dx.dtype, dx.strides[0], dx.strides[1]
    a.n, a.p = dx.shape


def _set_weight(a, weight, n):
    """weight (None = ones, else n values in a host or a device array) into the weight fields of a GLM input struct,
    checked; returns what must stay alive for the call."""
    if weight is None:
        return []
    if is_device_array(weight):
        dw = _DeviceArray(weight, "weight")
        if dw.size != n:
            raise ValueError("X.shape(0) should be equal to weight.size")
        a.weight_dev, a.weight_dtype, a.weight_stride = dw.ptr, dw.dtype, dw.as_vector("weight")
        return [dw]
    wh = _f64(weight).reshape(-1)
    if wh.size != n:
        raise ValueError("X.shape(0) should be equal to weight.size")
    a.weight_host = _dp(wh)
    return [wh]


def _glm_call(a, who, x, cols, beta, coef0, y, link, weight, stream):
    """The fields that the input structs of the one-model GLM entry points share -- x, cols / m / beta / coef0 / link, y,
    weight, stream -- filled into a, after every check of them that needs no device (`who` names the wrapper in the
    message about a 2-D beta).  Returns (n, p, cols, beta, coef0, what must stay alive for the call)."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    if np.ndim(beta) > 1:
        raise ValueError("beta must be 1-D: %s takes one model per call" % who)
    cols, B, c0 = _predict_model(dx, cols, np.asarray(beta, dtype=np.float64).reshape(-1), [coef0])
    if not (np.isfinite(B).all() and np.isfinite(c0).all()):
        raise ValueError("beta and coef0 must be finite")
    yh, dy, yrs, _, _ = _eval_y(y, n, 1)
    _set_x(a, dx)
    a.cols, a.m, a.beta, a.coef0, a.link = _ip(cols), cols.size, _dp(B), float(c0[0]), LINKS[link]
    a.y_stride = yrs
    if dy is not None:
        a.y_dev, a.y_dtype = dy.ptr, dy.dtype
    else:
        a.y_host = _dp(yh)
    keep = [dx, cols, B, yh, dy] + _set_weight(a, weight, n)
    a.stream = int(stream) if stream else None
    return n, p, cols, B.reshape(-1), float(c0[0]), keep


def evaluate_device(x, cols, B, coef0, y, link="identity", weight=None, stream=0):
    """Held-out loss of R models on a device matrix x (n x p: float64 or float32, any non-negative strides) in one pass
    over the support's columns (bessx_eval_device): with eta = x[:, cols] @ B + coef0,
        loss[r] = sum_i w_i * f(eta[i, r], y[i, r])
    f = (y - eta)^2 ("identity"), max(eta, 0) + log1p(exp(-|eta|)) - y * eta ("logistic") or exp(eta) - y * eta
    ("poisson").  cols, B, coef0 as in predict_device; y: n values shared by the models or (n, R), host or device array;
    weight: n values, host or device array, None = ones.  Returns {"loss": (R,), "sum_w": float} plus, for the logistic
    link, "correct": (R,), the weighted count of rows with (eta > 0) == (y > 0.5).  The n x R predictions are never
    stored, every sum has a fixed order (the same call gives the same bits), and only these numbers cross the bus.
    stream: raw handle of the stream x (and y, weight) were produced on."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    cols, B, coef0 = _predict_model(dx, cols, B, coef0)
    R = B.shape[1]
    yh, dy, yrs, ycs, y_cols = _eval_y(y, n, R)
    a = EvalInput()
    _set_x(a, dx)
    a.cols, a.m, a.B, a.coef0, a.R, a.link = _ip(cols), cols.size, _dp(B), _dp(coef0), R, LINKS[link]
    a.y_row_stride, a.y_col_stride, a.y_cols = yrs, ycs, y_cols
    if dy is not None:
        a.y_dev, a.y_dtype = dy.ptr, dy.dtype
    else:
        a.y_host = _dp(yh)
    keep = _set_weight(a, weight, n)  # (alive until the call has returned)
    a.stream = int(stream) if stream else None
    loss, aux, sw = np.zeros(R), np.zeros(R), _d(0)
    _check(lib().bessx_eval_device(ctypes.byref(a), _dp(loss), _dp(aux), ctypes.byref(sw)))
    out = {"loss": loss, "sum_w": sw.value}
    if link == "logistic":
        out["correct"] = aux
    return out


def candidate_models(result):
    """(cols, B, coef0) of the candidates a path stored (cand_support / cand_beta / cand_coef0 of the dict that
    Session.sequential_path / gs_path / pgs_path return): the union of their supports, ascending, and the m x R matrix of
    their de-normalised coefficients (zero where a candidate does not use a column).  They apply to raw X."""
    sup, beta = np.asarray(result["cand_support"]), np.asarray(result["cand_beta"], dtype=np.float64)
    coef0 = _f64(result["cand_coef0"]).reshape(-1)
    R = coef0.size
    if R < 1 or sup.shape[0] != R or beta.shape != sup.shape:
        raise ValueError("result holds no stored candidates (cand_support / cand_beta / cand_coef0)")
    cols = np.unique(sup[sup >= 0]).astype(np.int32)
    B = np.zeros((cols.size, R))
    for r in range(R):
        used = sup[r] >= 0
        B[np.searchsorted(cols, sup[r][used]), r] = beta[r][used]
    return cols, B, coef0


def evaluate_candidates(result, x, y, link="identity", weight=None, stream=0):
    """The train / validation split: the loss of every candidate of a path (fitted on the training rows) on held-out rows
    x, y in GPU memory, in ONE evaluate_device call over the union of the candidates' supports.  Returns (losses (R,),
    best) with best the index of the smallest loss, the lowest index on a tie (a NaN loss never wins)."""
    cols, B, coef0 = candidate_models(result)
    losses = evaluate_device(x, cols, B, coef0, y, link=link, weight=weight, stream=stream)["loss"]
    finite = np.where(np.isnan(losses), np.inf, losses)
    return losses, int(np.argmin(finite))


def op_eval_bench(x, cols, R=1, link="identity", y_cols=1, repeats=20):
    """(ms per launch, GB/s of n * m * item + n * 8 * (y_cols + 1) bytes) of the evaluation kernels on the device matrix
    x for the support cols and R models, device events."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms, g = _d(0), _d(0)
    _check(lib().bessx_op_eval_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                     _ip(cols), cols.size, int(R), LINKS[link], int(y_cols), repeats, ctypes.byref(ms),
                                     ctypes.byref(g)))
    return ms.value, g.value


INFO_M_MAX = 1024  # the largest m + 1 of information_device (INFO_M_MAX of bessx_dev.h)


def info_workspace(n, m, link="identity", weighted=False, dtype=np.float64, row_stride=None, col_stride=1):
    """(doubles of scratch memory, rows per slab, slabs) of an information_device call on an n-row matrix with a support
    of m columns (bessx_info_workspace; no device is needed).  The row split depends on (n, m) alone."""
    nd, rps, sl = _ll(0), _ll(0), _i(0)
    rs = int(row_stride) if row_stride is not None else max(int(m), 1)
    _check(lib().bessx_info_workspace(1 if np.dtype(dtype) == np.float32 else 0, rs, int(col_stride), int(n), int(m),
                                      LINKS[link], int(bool(weighted)), ctypes.byref(nd), ctypes.byref(rps),
                                      ctypes.byref(sl)))
    return nd.value, rps.value, sl.value


def information_device(x, cols, beta, coef0, y, link="identity", weight=None, stream=0):
    """Expected information and score of ONE model on a device matrix x (n x p: float64 or float32, any non-negative
    strides), read where it lies (bessx_info_device): with eta = x[:, cols] @ beta + coef0 and z_i = (1, x[i, cols]),
        info = sum_i v_i z_i z_i^T  ((m + 1, m + 1), both triangles, exact mirrors),   score = sum_i g_i z_i  (m + 1,)
    v = w, g = w (y - eta) ("identity"); v = w p (1 - p), g = w (y - p) ("logistic", p = 1 / (1 + exp(-eta)) without
    overflow or clamp); v = w exp(eta), g = w (y - exp(eta)) ("poisson").  cols: ascending distinct column numbers (may
    be empty: the intercept-only model reads no element of x); beta: len(cols) finite values; y: n values, weight: n
    non-negative values or None = ones, each a host or device array, float64 or float32, any stride.  Returns {"info",
    "score", "loss", "sum_w"}: loss and sum_w are evaluate_device's for the same arguments, bit for bit.  This is the
    UNPENALISED information on the original scale of x: a model fitted with lambda > 0 has score != 0.  No gathered copy
    of x[:, cols] is made, every sum has a fixed order (the same call gives the same bits), and a NaN inside the support
    view propagates (also from a row of weight 0).  len(cols) + 1 <= 1024.  stream: raw handle of the stream x (and y,
    weight) were produced on."""
    a = InfoInput()
    n, p, cols, beta, coef0, keep = _glm_call(a, "information_device", x, cols, beta, coef0, y, link, weight, stream)
    M = cols.size + 1
    info, score = np.empty((M, M)), np.empty(M)
    a.info, a.info_ld, a.score, a.out_on_device = info.ctypes.data, M, score.ctypes.data, 0
    loss, sw = _d(0), _d(0)
    _check(lib().bessx_info_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw)))
    return {"info": info, "score": score, "loss": loss.value, "sum_w": sw.value}


def op_info_bench(x, cols, repeats=20):
    """(ms per Gram sweep and finish, TFLOP/s of 2 n (m + 1) (m + 2) operations) of the information kernels on the device
    matrix x for the support cols, device events."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms, tf = _d(0), _d(0)
    _check(lib().bessx_op_info_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                     _ip(cols), cols.size, repeats, ctypes.byref(ms), ctypes.byref(tf)))
    return ms.value, tf.value


def _wald(info, score, coef, dispersion, dof):
    """The table of wald_table / cox_wald_table from an M x M information matrix, M = coef.size: cov = dispersion *
    D S^-1 D with D = diag(info)^(-1/2) and S = D info D Cholesky-factored; NaNs and positive_definite = False when a
    diagonal entry is <= 0 or not finite or S is not positive definite."""
    import math
    info = np.array(info, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64).reshape(-1)
    score = np.asarray(score, dtype=np.float64).reshape(-1)
    M = coef.size
    if info.shape != (M, M) or score.shape != (M,):
        raise ValueError("info must be (%d, %d) and score (%d,), got %s and %s" % (M, M, M, info.shape, score.shape))
    nan_v, nan_m = np.full(M, np.nan), np.full((M, M), np.nan)
    out = {"coef": coef, "se": nan_v, "z": nan_v.copy(), "p_value": nan_v.copy(), "cov": nan_m, "score": score,
           "dispersion": dispersion, "dof": dof, "cond": float("nan"), "positive_definite": False}
    dg = np.diag(info)
    if not (np.isfinite(info).all() and (dg > 0).all()):
        return out
    d = 1.0 / np.sqrt(dg)
    S = info * d[:, None] * d[None, :]
    S = 0.5 * (S + S.T)
    ev = np.linalg.eigvalsh(S)
    # (a factor can exist for a matrix that is singular to working precision: the smallest eigenvalue decides as well)
    if not (ev[0] > M * np.finfo(np.float64).eps * ev[-1]):
        out["cond"] = float("inf") if ev[0] <= 0 else float(ev[-1] / ev[0])
        return out
    try:
        Lc = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        out["cond"] = float(ev[-1] / ev[0])
        return out
    Li = np.linalg.solve(Lc, np.eye(M))
    cov = (Li.T @ Li) * d[:, None] * d[None, :] * dispersion
    se = np.sqrt(np.diag(cov))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = coef / se
    pv = np.array([math.erfc(abs(v) / math.sqrt(2.0)) if v == v else float("nan") for v in z])
    out.update(se=se, z=z, p_value=pv, cov=cov, cond=float(ev[-1] / ev[0]), positive_definite=True)
    return out


def wald_table(info, score, coef, link, loss, sum_w):
    """The coefficient table from an information matrix, on the host in fp64 NumPy.  info (M, M), score (M,), coef (M,)
    with the intercept first, as information_device orders them; link "identity", "logistic" or "poisson"; loss and
    sum_w as information_device returns them.  With D = diag(info)^(-1/2) and S = D info D (unit diagonal), S is
    Cholesky-factored and cov = D S^-1 D; for the identity link cov is multiplied by dispersion = loss / (sum_w - M)
    (the residual variance; NaN when sum_w - M <= 0), for the other links dispersion = 1.  Returns coef, se =
    sqrt(diag(cov)), z = coef / se, p_value = erfc(|z| / sqrt(2)) -- two-sided NORMAL, for the identity link too (the
    normal approximation, not Student's t) -- cov, score, dispersion, dof = sum_w - M, cond = the 2-norm condition number
    of S, and positive_definite.  When a diagonal entry of info is <= 0 or not finite, or S is not positive definite
    (duplicated columns, a separated logistic sample), se, z, p_value and cov are NaN and positive_definite is False:
    data decide that, so nothing is raised.  A score that is not near 0 says that coef is not the unpenalised optimum
    of its support (lambda > 0), and cov is then not its covariance."""
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    M = np.asarray(coef, dtype=np.float64).size
    dof = float(sum_w) - M
    if link == "identity":
        dispersion = float(loss) / dof if dof > 0 else float("nan")
    else:
        dispersion = 1.0
    return _wald(info, score, coef, dispersion, dof)


def cox_wald_table(info, score, coef, n_events):
    """wald_table for a Cox model: info (m, m), score (m,) and coef (m,) as cox_information_device orders them (no
    intercept), n_events = sum of w * status.  The dict of wald_table with dispersion = 1 and dof = n_events - m; an
    empty model (m = 0) gives empty arrays and positive_definite = True."""
    m = np.asarray(coef, dtype=np.float64).size
    if m == 0:
        z = np.zeros(0)
        return {"coef": z, "se": z.copy(), "z": z.copy(), "p_value": z.copy(), "cov": np.zeros((0, 0)), "score": z.copy(),
                "dispersion": 1.0, "dof": float(n_events), "cond": float("nan"), "positive_definite": True}
    return _wald(info, score, coef, 1.0, float(n_events) - m)


DIAG_KINDS = ("leverage", "response", "pearson", "deviance", "std_pearson", "std_deviance", "cooks")  # BESSX_DIAG_* bits
DIAG_LEVERAGE_KINDS = ("leverage", "std_pearson", "std_deviance", "cooks")  # the kinds that need the factor


def info_factor(info):
    """(R, positive_definite) for an M x M information matrix: R lower triangular with inv(info) = R^T R, from the
    scaled Cholesky factorisation of wald_table: D = diag(info)^(-1/2), S = D info D = L L^T, R = L^-1 D.  The tests are
    wald_table's: a diagonal entry <= 0 or not finite, a smallest eigenvalue of S that is not above M eps times the
    largest, or a failed factorisation give (an M x M matrix of NaN, False)."""
    info = np.array(info, dtype=np.float64)
    if info.ndim != 2 or info.shape[0] != info.shape[1] or info.shape[0] < 1:
        raise ValueError("info must be a square matrix, got shape %s" % (info.shape,))
    M = info.shape[0]
    bad = np.full((M, M), np.nan)
    dg = np.diag(info)
    if not (np.isfinite(info).all() and (dg > 0).all()):
        return bad, False
    d = 1.0 / np.sqrt(dg)
    S = info * d[:, None] * d[None, :]
    S = 0.5 * (S + S.T)
    ev = np.linalg.eigvalsh(S)
    if not (ev[0] > M * np.finfo(np.float64).eps * ev[-1]):
        return bad, False
    try:
        Lc = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return bad, False
    return np.tril(np.linalg.solve(Lc, np.eye(M))) * d[None, :], True


def _diag_mask(kinds):
    """(bit mask, names in ascending bit order) of an iterable of kind names (or one name)."""
    if isinstance(kinds, str):
        kinds = (kinds,)
    kinds = tuple(kinds)
    for k in kinds:
        if k not in DIAG_KINDS:
            raise ValueError("kinds must be taken from %s, got %r" % (list(DIAG_KINDS), k))
    if not kinds:
        raise ValueError("kinds must name at least one of %s" % (list(DIAG_KINDS),))
    names = tuple(k for k in DIAG_KINDS if k in kinds)
    return sum(1 << DIAG_KINDS.index(k) for k in names), names


def diag_workspace(n, m, kinds=DIAG_KINDS):
    """Doubles of scratch memory of a diagnostics_device call on n rows with a support of m columns
    (bessx_diag_workspace; no device is needed): v, the residual vectors that are needed but not requested, and the
    packed factor."""
    mask, _ = _diag_mask(kinds)
    nd = _ll(0)
    _check(lib().bessx_diag_workspace(int(n), int(m), mask, ctypes.byref(nd)))
    return nd.value


def diagnostics_device(x, cols, beta, coef0, y, factor=None, dispersion=1.0, link="identity", weight=None,
                       kinds=DIAG_KINDS, out=None, stream=0):
    """Per-row diagnostics of ONE model on a device matrix x (n x p: float64 or float32, any non-negative strides), read
    where it lies (bessx_diag_device).  With eta, mu, v as in information_device, z_i = (1, x[i, cols]), M = len(cols) + 1,
    w = 1 without weights, phi = dispersion and factor = R, lower triangular (M, M) with inv(info) = R^T R (info_factor):
        leverage      h_i = v_i * sum_j t_ij^2,  t_ij = sum_{k <= j} R_jk z_ik
        response      y_i - mu_i
        pearson       rp_i = sqrt(w_i) (y_i - mu_i) / sqrt(V_i)
        deviance      rd_i = sign(y_i - mu_i) sqrt(w_i max(d_i, 0)),  sign(0) = 0
        std_pearson   rp_i / sqrt(phi (1 - h_i))
        std_deviance  rd_i / sqrt(phi (1 - h_i))
        cooks         rp_i^2 h_i / (phi M (1 - h_i)^2)
    V = 1, d = (y - eta)^2 ("identity"); V = p (1 - p), d = 2 [f + y log y + (1 - y) log(1 - y)] ("logistic"); V =
    exp(eta), d = 2 [f + y log y - y] ("poisson"), f the loss term of evaluate_device and 0 log 0 = 0.  No clamp besides
    max(d, 0): h = 1 or a NaN inside the support give what IEEE arithmetic gives.  kinds: names from DIAG_KINDS; factor
    may be None when none of DIAG_LEVERAGE_KINDS is asked for (the matrix-core kernel is then not launched), and its
    strict upper triangle is never read.  Returns a dict from kind name to an (n,) vector: views of ONE (K, n) torch
    tensor on x's device when x is a torch tensor (torch is looked up, never imported), NumPy arrays for any other
    device object; out: a float64 device array of shape (K, n) with unit stride along n (its rows in DIAG_KINDS order)
    to write into instead, whose padding between rows is left untouched.  A row's numbers depend on that row's values,
    R, phi and M alone: the same bits wherever the row lies, whatever n is, under every layout of x.  No gathered copy
    of x[:, cols] and nothing n x M is stored.  len(cols) + 1 <= 1024.  stream: raw handle of the stream x (and y,
    weight) were produced on."""
    mask, names = _diag_mask(kinds)
    K = len(names)
    a = DiagInput()
    n, p, cols, beta, coef0, keep = _glm_call(a, "diagnostics_device", x, cols, beta, coef0, y, link, weight, stream)
    M = cols.size + 1
    if factor is not None:
        fh = _f64(factor)
        if fh.shape != (M, M):
            raise ValueError("factor must have shape (%d, %d), got %s" % (M, M, fh.shape))
        a.factor, a.factor_ld = _dp(fh), M
        keep.append(fh)
    a.dispersion, a.kinds = float(dispersion), mask
    if out is not None:
        if not is_device_array(out):
            raise ValueError("out must be a device array")
        do = _DeviceArray(out, "out", 2)
        if do.item != 8:
            raise ValueError("out: a device array of float64 is needed (typestr '<f8')")
        if do.shape != (K, n) or (n > 1 and do.strides[1] != 1) or (K > 1 and do.strides[0] < n):
            raise ValueError("out must have shape (%d, %d), unit stride along its rows and a row stride of at least %d"
                             % (K, n, n))
        result = [out[s] for s in range(K)]
        a.out, a.out_ld, a.out_on_device = do.ptr, (do.strides[0] if K > 1 else n), 1
    else:
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(x, torch.Tensor):
            buf = torch.empty((K, n), dtype=torch.float64, device=x.device)
            a.out, a.out_on_device = int(buf.data_ptr()), 1
        else:
            buf = np.empty((K, n))
            a.out, a.out_on_device = int(buf.ctypes.data), 0
        a.out_ld = n
        result = [buf[s] for s in range(K)]
    _check(lib().bessx_diag_device(ctypes.byref(a)))
    return dict(zip(names, result))


def op_diag_bench(x, cols, repeats=20):
    """(ms per launch, fp64 TFLOP/s over n * Mpad^2 operations, bytes the launch must move) of the leverage kernel
    k_diag_lev alone on the device matrix x for the support cols, device events."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms, tf, by = _d(0), _d(0), _d(0)
    _check(lib().bessx_op_diag_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                     _ip(cols), cols.size, repeats, ctypes.byref(ms), ctypes.byref(tf),
                                     ctypes.byref(by)))
    return ms.value, tf.value, by.value


def _candidates(candidates, p):
    """(int32 array or None, q) of a candidate list: None = all p columns, else ascending distinct columns of x."""
    if candidates is None:
        return None, p
    cand = np.asarray(candidates)
    if cand.ndim != 1 or cand.size < 1:
        raise ValueError("candidates must be a non-empty 1-D list of column numbers or None")
    if not np.issubdtype(cand.dtype, np.integer):
        raise ValueError("candidates must be integers")
    if cand.min() < 0 or cand.max() >= p:
        raise ValueError("candidates must be columns of X (0 .. %d)" % (p - 1))
    if (np.diff(cand) <= 0).any():
        raise ValueError("candidates must be ascending and distinct")
    return _i32(cand), int(cand.size)


def addscore_workspace(n, m, q, candidate_block=0):
    """What an addscore_device call on n rows with a support of m columns and q candidates needs and how it is split
    (bessx_addscore_workspace; no device is needed): {"doubles": scratch memory in all (2 n for v and g, the panel of
    n_pad x Mp, the block workspace), "rows_per_slab", "slabs": the row split, a function of (n, m, q, candidate_block)
    alone, "block": candidates per block, "block_doubles": the part of the scratch memory beyond v, g and the panel,
    which does not depend on p, "sum_depth": the additions behind one s_j}."""
    nd, rps, sl, bl, bd, dp = _ll(0), _ll(0), _i(0), _i(0), _ll(0), _i(0)
    _check(lib().bessx_addscore_workspace(int(n), int(m), int(q), int(candidate_block), ctypes.byref(nd),
                                          ctypes.byref(rps), ctypes.byref(sl), ctypes.byref(bl), ctypes.byref(bd),
                                          ctypes.byref(dp)))
    return {"doubles": nd.value, "rows_per_slab": rps.value, "slabs": sl.value, "block": bl.value,
            "block_doubles": bd.value, "sum_depth": dp.value}


def addscore_device(x, cols, beta, coef0, y, link="identity", weight=None, factor=None, candidates=None,
                    want_cross=False, stream=0, candidate_block=0):
    """The ingredients of the Rao score test of every candidate column against ONE model on a device matrix x (n x p:
    float64 or float32, any non-negative strides), read where it lies (bessx_addscore_device).  The model and v, g, z,
    M = len(cols) + 1, info, score, loss, sum_w are information_device's (the same bits).  candidates: None = all p
    columns, else ascending distinct column numbers.  factor: R, lower triangular (M, M) with inv(info) = R^T R; None =
    information_device and info_factor are called first (and when the information is not positive definite, s and a
    are NaN).  With r = inv(info) @ score, for candidate j
        u_j = sum_i g_i x_ij,   c_j = sum_i v_i x_ij z_i,   d_j = sum_i v_i x_ij^2,   s_j = |R c_j|^2,   a_j = c_j . r
    Returns {"columns", "u", "d", "s", "a", "info", "score", "loss", "sum_w", "positive_definite"} (NumPy, host) plus
    "cross" (q, M), the c_j, when want_cross.  The subtractions u - a and d - s are score_test_table's.  One pass over
    all candidate columns on the fp64 matrix cores; no x-sized temporary; candidates go in blocks of candidate_block (0
    = the library's choice; a multiple of 16), so scratch beyond the n x Mp panel does not depend on p (addscore_workspace).
    The same call gives the same bits, and every layout of the same values of one dtype gives the same bits.  Cox
    models: cox_addscore_device.  Groups of columns with more than one degree of freedom: groupscore_device.  Not corrected
    for selection.
    len(cols) + 1 <= 1024.  stream: raw handle of the stream x (and y, weight) were produced on."""
    a = AddscoreInput()
    n, p, cols, beta, coef0, keep = _glm_call(a, "addscore_device", x, cols, beta, coef0, y, link, weight, stream)
    cand, q = _candidates(candidates, p)
    M = cols.size + 1
    pd = True
    if factor is None:
        first = information_device(x, cols, beta, coef0, y, link=link, weight=weight, stream=stream)
        fh, pd = info_factor(first["info"])
    else:
        fh = _f64(factor)
        if fh.shape != (M, M):
            raise ValueError("factor must have shape (%d, %d), got %s" % (M, M, fh.shape))
    if pd:
        a.factor, a.factor_ld = _dp(fh), M
    a.candidates, a.q, a.candidate_block = _ip(cand), q, int(candidate_block)
    info, score = np.empty((M, M)), np.empty(M)
    out = np.full((4, q), np.nan)
    a.info, a.info_ld, a.score = _dp(info), M, _dp(score)
    a.u, a.d, a.s, a.a = (out[k].ctypes.data for k in range(4))
    cross = None
    if want_cross:
        cross = np.empty((q, M))
        a.cross, a.cross_ld = cross.ctypes.data, M
    a.out_on_device = 0
    loss, sw = _d(0), _d(0)
    _check(lib().bessx_addscore_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw)))
    got = {"columns": np.arange(p, dtype=np.int64) if cand is None else cand.astype(np.int64), "u": out[0], "d": out[1],
           "s": out[2], "a": out[3], "info": info, "score": score, "loss": loss.value, "sum_w": sw.value,
           "positive_definite": bool(pd), "support": cols.astype(np.int64)}
    if want_cross:
        got["cross"] = cross
    return got


def score_test_table(got, link):
    """The Rao score test of every candidate from what addscore_device (or the NumPy route) returns, on the host in
    fp64: adj = u - a, variance = d - s, statistic = adj^2 / (dispersion * variance) where variance is finite and > 0,
    else NaN; p_value = erfc(sqrt(statistic / 2)), chi-square with 1 degree of freedom.  dispersion is wald_table's:
    loss / (sum_w - M) for the identity link (NaN when sum_w - M <= 0), 1 otherwise.  A candidate that is in the model's
    support ("support" of got) has in_model = True and NaN for statistic and p_value: its variance is rounding noise.
    For the identity link the statistic is the F-to-enter numerator over the CURRENT model's residual variance.
    Returns {"columns", "score", "variance", "statistic", "p_value", "in_model", "dispersion"}.  Selection is not
    corrected for."""
    import math
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    u, a = np.asarray(got["u"], dtype=np.float64), np.asarray(got["a"], dtype=np.float64)
    d, s = np.asarray(got["d"], dtype=np.float64), np.asarray(got["s"], dtype=np.float64)
    columns = np.asarray(got["columns"], dtype=np.int64)
    M = np.asarray(got["score"]).size
    if link == "identity":
        dof = float(got["sum_w"]) - M
        dispersion = float(got["loss"]) / dof if dof > 0 else float("nan")
    else:
        dispersion = 1.0
    adj, var = u - a, d - s
    in_model = np.isin(columns, np.asarray(got.get("support", np.zeros(0)), dtype=np.int64))
    ok = np.isfinite(var) & (var > 0) & ~in_model
    stat = np.full(columns.size, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        stat[ok] = (adj[ok] * adj[ok]) / (dispersion * var[ok])
    pv = np.array([math.erfc(math.sqrt(v / 2.0)) if (v == v and v >= 0) else float("nan") for v in stat])
    return {"columns": columns, "score": adj, "variance": var, "statistic": stat, "p_value": pv, "in_model": in_model,
            "dispersion": dispersion}


def op_addscore_bench(x, cols, candidates=None, candidate_block=0, repeats=5):
    """ms per stage of the score-test kernels on the device matrix x for the support cols, device events, each over
    every block of candidates: {"pack", "cross", "finish", "statistic"} (bessx_op_addscore_bench)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    cand, q = _candidates(candidates, dx.shape[1])
    ms = (_d * 4)()
    _check(lib().bessx_op_addscore_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, _ip(cand), q, int(candidate_block), repeats, ms))
    return dict(zip(("pack", "cross", "finish", "statistic"), [float(v) for v in ms]))


GROUPSCORE_WIDTH_MAX = 64  # columns of a tested group (bessx_groupscore_device)


def _group_lists(group_starts, groups, p):
    """(int32 starts, int32 tested groups or None) as the library takes them.  Only the shapes and dtypes are checked
    here: what the lists must satisfy is the library's to say (BESSX_ERR_ARG / BESSX_ERR_UNSUPPORTED)."""
    gs = np.asarray(group_starts)
    if gs.ndim != 1 or gs.size < 1 or not np.issubdtype(gs.dtype, np.integer):
        raise ValueError("group_starts must be a non-empty 1-D list of integer column numbers")
    tg = None
    if groups is not None:
        tg = np.asarray(groups)
        if tg.ndim != 1 or tg.size < 1 or not np.issubdtype(tg.dtype, np.integer):
            raise ValueError("groups must be a non-empty 1-D list of integer group numbers or None")
        tg = _i32(tg)
    return _i32(gs), tg


def _group_columns(gs, tg, p):
    """(tested group numbers, widths, columns, group_of_column) of lists the library accepts, else None."""
    G = gs.size
    if gs[0] != 0 or (np.diff(gs) <= 0).any() or gs[-1] >= p:
        return None
    tested = np.arange(G, dtype=np.int64) if tg is None else tg.astype(np.int64)
    if tested.min() < 0 or tested.max() >= G or (np.diff(tested) <= 0).any():
        return None
    ends = np.append(gs[1:], p).astype(np.int64)
    width = ends[tested] - gs[tested]
    columns = np.concatenate([np.arange(gs[g], ends[g], dtype=np.int64) for g in tested])
    return tested, width, columns, np.repeat(tested, width)


def groupscore_workspace(n, p, m, group_starts, groups=None, candidate_block=0):
    """What a groupscore_device call on n rows and p columns with a support of m columns needs and how it is split
    (bessx_groupscore_workspace; no device is needed): {"doubles": scratch memory in all, "block_doubles": the part of it
    beyond v, g and the panel, which does not depend on p, "rows_per_slab", "slabs": the row split of u and C (section 2l's,
    for the block with the longest chain), "gram_rows_per_slab", "gram_slabs": the row split of D, a function of n alone,
    "blocks", "block_first": the first tested group of every block, then the number of tested groups -- a function of
    (group_starts, groups, candidate_block) alone --, "band": w, and the longest chains of additions "depth" (u, C),
    "score_depth" (the score behind r), "gram_depth" (D), "s_depth" (S)}."""
    gs, tg = _group_lists(group_starts, groups, p)
    nt = gs.size if tg is None else tg.size
    nd, bd, rps, sl, nb, first, band, dep = _ll(0), _ll(0), (_ll * 2)(), (_i * 2)(), _i(0), (_i * (nt + 1))(), _i(0), (_i * 4)()
    _check(lib().bessx_groupscore_workspace(int(n), int(p), int(m), _ip(gs), gs.size, _ip(tg), nt, int(candidate_block),
                                            ctypes.byref(nd), ctypes.byref(bd), rps, sl, ctypes.byref(nb), first,
                                            ctypes.byref(band), dep))
    return {"doubles": nd.value, "block_doubles": bd.value, "rows_per_slab": rps[0], "slabs": sl[0],
            "gram_rows_per_slab": rps[1], "gram_slabs": sl[1], "blocks": nb.value,
            "block_first": [int(first[k]) for k in range(nb.value + 1)], "band": band.value, "depth": dep[0],
            "score_depth": dep[1], "gram_depth": dep[2], "s_depth": dep[3]}


def groupscore_device(x, cols, beta, coef0, y, group_starts, groups=None, link="identity", weight=None, factor=None,
                      stream=0, candidate_block=0):
    """The ingredients of the Rao score test of every tested GROUP of columns against ONE model on a device matrix x
    (n x p: float64 or float32, any non-negative strides), read where it lies (bessx_groupscore_device).  The model and
    v, g, z, M, info, score, loss, sum_w, factor and r are addscore_device's.  group_starts: G ascending start columns
    with group_starts[0] = 0, group g = columns group_starts[g] .. group_starts[g + 1] - 1 (the last one ends at p - 1);
    groups: ascending distinct group numbers, None = all.  For a tested group with columns J, d = len(J) <= 64:
        u = X_J^T g,   C = X_J^T diag(v) Z,   a = C r,   D = X_J^T diag(v) X_J,   S = (C R^T)(C R^T)^T
    Returns {"columns", "group_of_column", "u", "a" (one value per tested column), "D", "S" (the d x d blocks one after
    another, row-major, block t at offsets[t], each exactly symmetric), "offsets" (len(groups) + 1), "info", "score",
    "loss", "sum_w", "positive_definite", "support"} (NumPy, host).  The subtractions u - a and D - S, the d x d
    Cholesky factor and the quadratic form are group_score_test_table's.  factor None: information_device and
    info_factor are called first (and when the information is not positive definite, S and a are NaN).  The band of
    X_J^T diag(v) X_J around the diagonal is formed on the fp64 matrix cores with x read in place; no x-sized temporary;
    blocks of candidate_block columns (0 = the library's choice; a multiple of 16, at least the widest tested group
    rounded up to 16) hold whole groups, so scratch beyond the n x Mp panel does not depend on p (groupscore_workspace).
    The same call gives the same bits, and every layout of the same values of one dtype gives the same bits.  A tested
    group wider than 64 columns is BessxError code 3.  Cox models: cox_groupscore_device.  Not corrected for selection.
    len(cols) + 1 <= 1024.  stream: raw handle of the stream x (and y, weight) were produced on."""
    a = GroupscoreInput()
    n, p, cols, beta, coef0, keep = _glm_call(a, "groupscore_device", x, cols, beta, coef0, y, link, weight, stream)
    gs, tg = _group_lists(group_starts, groups, p)
    nt = gs.size if tg is None else tg.size
    lists = _group_columns(gs, tg, p)
    ok = lists is not None and lists[1].max() <= GROUPSCORE_WIDTH_MAX  # (else the library refuses before it writes)
    q, tot = (int(lists[1].sum()), int((lists[1] * lists[1]).sum())) if ok else (1, 1)
    M = cols.size + 1
    pd = True
    if factor is None:
        first = information_device(x, cols, beta, coef0, y, link=link, weight=weight, stream=stream)
        fh, pd = info_factor(first["info"])
    else:
        fh = _f64(factor)
        if fh.shape != (M, M):
            raise ValueError("factor must have shape (%d, %d), got %s" % (M, M, fh.shape))
    if pd:
        a.factor, a.factor_ld = _dp(fh), M
    a.group_starts, a.n_groups, a.groups, a.n_tested = _ip(gs), gs.size, _ip(tg), nt
    a.candidate_block = int(candidate_block)
    info, score = np.empty((M, M)), np.empty(M)
    vec, blk, offsets = np.full((2, q), np.nan), np.full((2, tot), np.nan), np.zeros(nt + 1, dtype=np.int64)
    a.info, a.info_ld, a.score = _dp(info), M, _dp(score)
    a.u, a.a, a.D, a.S = vec[0].ctypes.data, vec[1].ctypes.data, blk[0].ctypes.data, blk[1].ctypes.data
    a.offsets = offsets.ctypes.data_as(ctypes.POINTER(_ll))
    a.out_on_device = 0
    loss, sw = _d(0), _d(0)
    _check(lib().bessx_groupscore_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw)))
    return {"columns": lists[2], "group_of_column": lists[3], "u": vec[0], "a": vec[1], "D": blk[0], "S": blk[1],
            "offsets": offsets, "info": info, "score": score, "loss": loss.value, "sum_w": sw.value,
            "positive_definite": bool(pd), "support": cols.astype(np.int64)}


def chi2_sf(x, df):
    """The upper tail of the chi-square distribution with df > 0 degrees of freedom at x: Q(df / 2, x / 2), the
    regularised upper incomplete gamma function, in fp64 with no dependence outside the standard library.  For an
    integer df up to 512 (and x / 2 <= 700, so that exp(-x / 2) is a normal number) the finite recurrence
    Q(a + 1, y) = Q(a, y) + y^a exp(-y) / Gamma(a + 1) is run from Q(1/2, y) = erfc(sqrt(y)) or Q(1, y) = exp(-y): sums of
    positive terms, so df = 1 and df = 2 are score_test_table's erfc and the exponential to the last bits.  Otherwise
    1 - the series of the lower function below y = a + 1 and the continued fraction (modified Lentz) above.  NaN for a
    NaN or negative x; 1 at 0; 0 at inf."""
    import math
    x, a = float(x), 0.5 * float(df)
    if not a > 0:
        raise ValueError("df must be positive")
    if x != x or x < 0:
        return float("nan")
    if x == 0:
        return 1.0
    if x == float("inf"):
        return 0.0
    y = 0.5 * x
    if float(df) == int(df) and df <= 512 and y <= 700.0:
        df = int(df)
        if df % 2:
            s, t, k, steps = math.erfc(math.sqrt(y)), 2.0 * math.sqrt(y / math.pi) * math.exp(-y), 1.5, (df - 1) // 2
        else:
            s = math.exp(-y)
            t, k, steps = y * s, 2.0, df // 2 - 1
        for _ in range(steps):  # t = y^(k - 1) exp(-y) / Gamma(k): the step from Q(k - 1, y) to Q(k, y)
            s += t
            t *= y / k
            k += 1.0
        return min(s, 1.0)
    front = math.exp(-y + a * math.log(y) - math.lgamma(a))
    if y < a + 1.0:
        term = total = 1.0 / a
        ak = a
        for _ in range(10000):
            ak += 1.0
            term *= y / ak
            total += term
            if term < total * 1e-17:
                break
        return min(max(1.0 - front * total, 0.0), 1.0)
    tiny = 1e-300
    b = y + 1.0 - a
    c, dd = 1.0 / tiny, 1.0 / b
    hh = dd
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        dd = an * dd + b
        dd = tiny if abs(dd) < tiny else dd
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        dd = 1.0 / dd
        de = dd * c
        hh *= de
        if abs(de - 1.0) < 1e-15:
            break
    return min(max(front * hh, 0.0), 1.0)


def group_score_test_table(got, link):
    """The Rao score test of every tested group from what groupscore_device (or the NumPy route) returns, on the host in
    fp64.  For a group with d columns: adj = u - a, V = D - S, statistic = adj^T inverse(V) adj / dispersion through the
    Cholesky factor of V scaled to unit diagonal, p_value = chi2_sf(statistic, d).  dispersion is score_test_table's:
    loss / (sum_w - M) for the identity link (NaN when sum_w - M <= 0), 1 otherwise.  A group with any column in the
    model's support ("support" of got) has in_model = True and NaN for statistic and p_value.  A group whose V has a
    diagonal entry that is not finite and positive, or whose scaled V has no Cholesky factor with positive pivots (a
    group that the support, or the rest of the group, reproduces) has NaN as well; nothing is raised.  Returns {"group",
    "first_column", "df" (one value per tested group), "score" (a list: the adjusted vector of each group), "statistic",
    "p_value", "in_model", "dispersion"}.  Selection is not corrected for."""
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    D, S = np.asarray(got["D"], dtype=np.float64), np.asarray(got["S"], dtype=np.float64)
    M = np.asarray(got["score"]).size
    if link == "identity":
        dof = float(got["sum_w"]) - M
        dispersion = float(got["loss"]) / dof if dof > 0 else float("nan")
    else:
        dispersion = 1.0
    return _group_score_table(got, lambda lo, hi: D[lo:hi] - S[lo:hi], dispersion)


def _group_score_table(got, v_of, dispersion):
    """The loop of group_score_test_table and cox_group_score_test_table: v_of(lo, hi) gives the d * d entries of a
    group's V from the packed blocks' entries lo .. hi - 1."""
    u, a = np.asarray(got["u"], dtype=np.float64), np.asarray(got["a"], dtype=np.float64)
    columns = np.asarray(got["columns"], dtype=np.int64)
    goc = np.asarray(got["group_of_column"], dtype=np.int64)
    offsets = np.asarray(got["offsets"], dtype=np.int64)
    nt = offsets.size - 1
    df = np.rint(np.sqrt(np.diff(offsets))).astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(df)])
    support = np.asarray(got.get("support", np.zeros(0)), dtype=np.int64)
    col_in = np.isin(columns, support)
    group, first = np.empty(nt, dtype=np.int64), np.empty(nt, dtype=np.int64)
    stat, pv, in_model, adjs = np.full(nt, np.nan), np.full(nt, np.nan), np.zeros(nt, dtype=bool), []
    adj_all = u - a
    for t in range(nt):
        j0, j1, d = int(pos[t]), int(pos[t + 1]), int(df[t])
        group[t], first[t] = goc[j0], columns[j0]
        adj = adj_all[j0:j1]
        adjs.append(adj)
        in_model[t] = bool(col_in[j0:j1].any())
        if in_model[t]:
            continue
        V = v_of(offsets[t], offsets[t + 1]).reshape(d, d)
        dg = np.diag(V)
        if not (np.isfinite(V).all() and np.isfinite(adj).all() and (dg > 0).all()):
            continue
        sc = 1.0 / np.sqrt(dg)
        try:
            L = np.linalg.cholesky((V * sc[:, None]) * sc[None, :])
        except np.linalg.LinAlgError:
            continue
        if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
            continue
        z, rhs = np.zeros(d), adj * sc
        for j in range(d):  # (forward substitution: the operations the tests' error bound is derived for)
            z[j] = (rhs[j] - L[j, :j] @ z[:j]) / L[j, j]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            stat[t] = float(z @ z) / dispersion
        if stat[t] == stat[t] and stat[t] >= 0:
            pv[t] = chi2_sf(stat[t], d)
    return {"group": group, "first_column": first, "df": df, "score": adjs, "statistic": stat, "p_value": pv,
            "in_model": in_model, "dispersion": dispersion}


def op_groupscore_bench(x, cols, group_starts, groups=None, candidate_block=0, repeats=5):
    """ms per step of the group score test on the device matrix x for the support cols, device events, each over every
    block of candidates: {"pack", "cross", "finish", "gram", "gram_sum", "s_band", "extract"}
    (bessx_op_groupscore_bench)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    gs, tg = _group_lists(group_starts, groups, dx.shape[1])
    ms = (_d * 7)()
    _check(lib().bessx_op_groupscore_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                           _ip(cols), cols.size, _ip(gs), gs.size, _ip(tg),
                                           gs.size if tg is None else tg.size, int(candidate_block), repeats, ms))
    return dict(zip(("pack", "cross", "finish", "gram", "gram_sum", "s_band", "extract"), [float(v) for v in ms]))


TIES = {"order": 0, "breslow": 1}  # bessx_cox_eval_input.ties


COV_TYPES = ("HC0", "HC1", "HC2", "HC3")  # BESSX_HC0 .. BESSX_HC3
SANDWICH_RUN = 64  # rows per run of a cluster's sum (SW_RUN of bessx_k_sandwich.hip)


def _cov_kind(kind):
    if kind not in COV_TYPES:
        raise ValueError("kind must be one of %s, got %r" % (list(COV_TYPES), kind))
    return COV_TYPES.index(kind)


def cluster_labels(cluster, n):
    """Cluster labels as the library takes them, checked without a device call: (host int64 array or None, device
    pointer or None, BESSX_I64 / BESSX_I32, element stride, the object to keep alive).  cluster: n integer labels, a host
    array or a device array (__cuda_array_interface__) of int64 or int32; any values, any order."""
    if is_device_array(cluster):
        cai = cluster.__cuda_array_interface__
        shape = tuple(int(v) for v in cai["shape"])
        typestr = cai["typestr"]
        if typestr not in ("<i8", "<i4"):
            raise ValueError("cluster: a device array must be int64 or int32 (typestr '<i8' or '<i4'), got %r" % typestr)
        item = 8 if typestr == "<i8" else 4
        size = int(np.prod(shape)) if shape else 1
        if size != n:
            raise ValueError("X.shape(0) should be equal to cluster.size")
        if len([v for v in shape if v != 1]) > 1:
            raise ValueError("cluster: expected a vector, got shape %s" % (shape,))
        strides = cai.get("strides")
        stride = 1
        if strides is not None:
            big = [int(st) for v, st in zip(shape, strides) if v != 1]
            stride = big[0] // item if big else 1
            if big and (big[0] < 0 or big[0] % item):
                raise ValueError("cluster: byte strides of a device array must be non-negative multiples of the item size")
        ptr = int(cai["data"][0])
        if not ptr:
            raise ValueError("cluster: null device pointer")
        return None, ptr, 0 if item == 8 else 1, stride, cluster
    a = np.asarray(cluster)
    if a.dtype.kind not in "iu":
        raise ValueError("cluster must hold integer labels, got dtype %s" % a.dtype)
    if a.dtype.kind == "u" and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise ValueError("cluster labels must fit int64")
    a = np.ascontiguousarray(a.reshape(-1), dtype=np.int64)
    if a.size != n:
        raise ValueError("X.shape(0) should be equal to cluster.size")
    return a, None, 0, 1, a


def _set_cluster(a, cluster, n, keep):
    if cluster is None:
        return
    host, ptr, dt, stride, obj = cluster_labels(cluster, n)
    keep.append(obj)
    if host is not None:
        a.cluster_host = host.ctypes.data_as(ctypes.POINTER(_ll))
    else:
        a.cluster_dev, a.cluster_dtype, a.cluster_stride = ptr, dt, stride


def sandwich_workspace(n, m, link="identity", weighted=False, kind="HC0", n_clusters=0, max_cluster_rows=0,
                       dtype=np.float64, row_stride=None, col_stride=1):
    """What a sandwich_device call on n rows with a support of m columns needs and how it adds, without a device
    (bessx_sandwich_workspace): a dict with
        doubles                 device scratch in doubles (an upper bound for n_clusters clusters the longest of which has
                                max_cluster_rows rows; n_clusters = 0: no cluster labels)
        rows_per_slab, slabs    the row split of the Gram sweeps over x (information_device's for (n, m))
        cluster_rows_per_slab, cluster_slabs   the split of the sweep over the n_clusters rows of S (0, 0 without labels)
        sum_depth               additions behind an entry of s_g for a cluster of max_cluster_rows rows: a chain of
                                min(r, 64) FMAs in row order, then the ceil(r / 64) runs in run order
        sq_depth                additions behind meat[0, 0] = sum_g s_g0^2 with labels: ceil(G / 256) + 8."""
    nd, rps, sl, crps, csl, sd, qd = _ll(0), _ll(0), _i(0), _ll(0), _i(0), _i(0), _i(0)
    rs = int(row_stride) if row_stride is not None else max(int(m), 1)
    _check(lib().bessx_sandwich_workspace(1 if np.dtype(dtype) == np.float32 else 0, rs, int(col_stride), int(n), int(m),
                                          LINKS[link], int(bool(weighted)), _cov_kind(kind), int(n_clusters),
                                          int(max_cluster_rows), ctypes.byref(nd), ctypes.byref(rps), ctypes.byref(sl),
                                          ctypes.byref(crps), ctypes.byref(csl), ctypes.byref(sd), ctypes.byref(qd)))
    return {"doubles": nd.value, "rows_per_slab": rps.value, "slabs": sl.value, "cluster_rows_per_slab": crps.value,
            "cluster_slabs": csl.value, "sum_depth": sd.value, "sq_depth": qd.value}


def meat_device(x, cols, u=None, cluster=None, intercept=True, stream=0):
    """The meat of a sandwich covariance from a device matrix x (n x p: float64 or float32, any non-negative strides),
    read where it lies (bessx_meat_device).  With z_i = (1, x[i, cols]) (intercept=True) or x[i, cols] (intercept=False,
    a dense source such as the Cox score residuals L; len(cols) >= 1), M entries, and a row scalar u (n float64 values,
    host or device with unit stride; None = ones):
        without cluster   meat = sum_i u_i^2 z_i z_i^T,            sums = sum_i u_i z_i
        with cluster      meat = sum_g s_g s_g^T,  s_g = sum_{i in g} u_i z_i,   sums = sum_g s_g
    cluster: n integer labels (any values, any order; a host array, or a device array of int64 / int32 that is copied
    to the host).  Returns {"meat" (M, M) with both triangles exact mirrors, "sums" (M,), "n_clusters": G or None}.  The
    rows are sorted by label on the host (stable); s_g is formed by one kernel from x in place -- a cluster of r rows
    is min(r, 64) + ceil(r / 64) - 1 additions in an order that depends on r alone, so its bits depend on the cluster's
    rows in their original order and on u, not on the layout of x or the other clusters -- and the meat is the
    matrix-core Gram sweep of information_device over the G x M sums (without cluster and with the intercept: over x in
    place, with u^2 as the working weight; without cluster and without the intercept the sweep runs over x in place
    as well, and only with a u is every row its own cluster, an n x M copy).
    No floating-point atomics: the same call gives the same bits.  A NaN inside the support view propagates, nothing
    outside it is read.  len(cols) + intercept <= 1024.  stream: raw handle of the stream x (and u) were produced on."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    cols, _, _ = _predict_model(dx, cols)
    icpt = 1 if intercept else 0
    M = cols.size + icpt
    if M < 1:
        raise ValueError("an empty support needs intercept=True")
    a = MeatInput()
    _set_x(a, dx)
    a.cols, a.m, a.intercept = _ip(cols), cols.size, icpt
    keep = [dx, cols]
    if u is not None:
        if is_device_array(u):
            du = _DeviceArray(u, "u")
            if du.size != n:
                raise ValueError("X.shape(0) should be equal to u.size")
            if du.item != 8 or (n > 1 and du.as_vector("u") != 1):
                raise ValueError("u: a device array of float64 with unit stride is needed")
            a.u_dev = du.ptr
            keep.append(du)
        else:
            uh = _f64(u).reshape(-1)
            if uh.size != n:
                raise ValueError("X.shape(0) should be equal to u.size")
            a.u_host = _dp(uh)
            keep.append(uh)
    _set_cluster(a, cluster, n, keep)
    meat, sums = np.empty((M, M)), np.empty(M)
    a.meat, a.meat_ld, a.sums, a.out_on_device = meat.ctypes.data, M, sums.ctypes.data, 0
    a.stream = int(stream) if stream else None
    G = _i(0)
    _check(lib().bessx_meat_device(ctypes.byref(a), ctypes.byref(G)))
    return {"meat": meat, "sums": sums, "n_clusters": G.value if cluster is not None else None}


def sandwich_device(x, cols, beta, coef0, y, link="identity", weight=None, kind="HC0", factor=None, cluster=None,
                    stream=0):
    """Information, score and the meat of the robust (Huber-White) or cluster-robust covariance of ONE model on a device
    matrix x, read where it lies, in one call (bessx_sandwich_device).  Notation of information_device: z_i = (1,
    x[i, cols]), M = len(cols) + 1, v_i and g_i the working and score weights of the link, info = sum_i v_i z_i z_i^T.
    With weights g_i = w_i (y_i - mu_i), so the meat carries w_i^2: the estimating-function convention.
        row scalar   "HC0", "HC1": u_i = g_i;  "HC2": u_i = g_i / sqrt(1 - h_i);  "HC3": u_i = g_i / (1 - h_i), with h_i
                     diagnostics_device's leverage from the same factor R (info_factor(info)[0]; needed by HC2 / HC3
                     only).  No clamp: h_i = 1 gives what IEEE arithmetic gives.
        meat         B = sum_i u_i^2 z_i z_i^T without cluster;  B = sum_g s_g s_g^T, s_g = sum_{i in g} u_i z_i with
                     cluster (n integer labels, any values, any order, host or device).  (M, M), exact mirrors.
    The covariance c * inv(info) B inv(info) and its scale factor c are sandwich_table's; "HC0" and "HC1" give the same
    meat.  cluster with "HC2" / "HC3" raises ValueError (the block-leverage corrections are not built).  Returns {"info",
    "score", "loss", "sum_w"} -- information_device's for the same arguments, bit for bit -- plus "meat" and
    "n_clusters" (G, or None without cluster).  A row or a cluster of weight 0 counts as a row / a cluster.  No gathered
    copy of x[:, cols] and no n x M score matrix: the scratch is n-vectors, the Gram partials and G * M doubles of
    cluster sums.  The same call gives the same bits, and with cluster the meat is the same bits under every layout of
    the same x.  A NaN inside the support view propagates.  len(cols) + 1 <= 1024."""
    k = _cov_kind(kind)
    if cluster is not None and k >= 2:
        raise ValueError("cluster goes with kind 'HC0' (CR0) or 'HC1' (CR1), got %r" % kind)
    a = SandwichInput()
    n, p, cols, beta, coef0, keep = _glm_call(a, "sandwich_device", x, cols, beta, coef0, y, link, weight, stream)
    M = cols.size + 1
    a.kind = k
    if k >= 2:
        if factor is None:
            raise ValueError("kind %r needs the factor (info_factor)" % kind)
        fh = _f64(factor)
        if fh.shape != (M, M):
            raise ValueError("factor must have shape (%d, %d), got %s" % (M, M, fh.shape))
        if not np.isfinite(np.tril(fh)).all():
            raise ValueError("the lower triangle of the factor must be finite")
        a.factor, a.factor_ld = _dp(fh), M
        keep.append(fh)
    _set_cluster(a, cluster, n, keep)
    info, score, meat = np.empty((M, M)), np.empty(M), np.empty((M, M))
    a.info, a.info_ld, a.score, a.meat, a.meat_ld = info.ctypes.data, M, score.ctypes.data, meat.ctypes.data, M
    a.out_on_device = 0
    loss, sw, G = _d(0), _d(0), _i(0)
    _check(lib().bessx_sandwich_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw), ctypes.byref(G)))
    return {"info": info, "score": score, "loss": loss.value, "sum_w": sw.value, "meat": meat,
            "n_clusters": G.value if cluster is not None else None}


def op_sandwich_bench(x, cols, cluster, repeats=20):
    """(ms per launch, bytes the algorithm needs: the support and u once, S once) of the cluster-sum kernel alone (and the addition of the partials of
    clusters longer than a run) on the device matrix x for the intercept and the support cols and n host labels,
    device events."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    lab, _, _, _, _ = cluster_labels(np.asarray(cluster), dx.shape[0])
    ms, by = _d(0), _d(0)
    _check(lib().bessx_op_sandwich_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, lab.ctypes.data_as(ctypes.POINTER(_ll)), repeats,
                                         ctypes.byref(ms), ctypes.byref(by)))
    return ms.value, by.value


def _sandwich(info, meat, score, coef, scale, cov_type, n_clusters, dof):
    """_wald's table with cov = scale * inv(info) meat inv(info), inv(info) = R^T R from info_factor."""
    import math
    coef = np.asarray(coef, dtype=np.float64).reshape(-1)
    M = coef.size
    meat = np.array(meat, dtype=np.float64)
    if meat.shape != (M, M):
        raise ValueError("meat must be (%d, %d), got %s" % (M, M, meat.shape))
    out = _wald(info, score, coef, 1.0, dof)  # (shapes, the NaN table, cond and positive_definite)
    out.update(cov_type=cov_type, n_clusters=n_clusters, scale=scale, meat=meat)
    if not out["positive_definite"]:
        return out
    R, _ = info_factor(info)
    A = R.T @ R
    cov = scale * (A @ meat @ A)
    cov = 0.5 * (cov + cov.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        se = np.sqrt(np.diag(cov))
        z = coef / se
    pv = np.array([math.erfc(abs(v) / math.sqrt(2.0)) if v == v else float("nan") for v in z])
    out.update(cov=cov, se=se, z=z, p_value=pv)
    return out


def sandwich_table(info, meat, score, coef, kind, n, n_clusters=None):
    """The coefficient table with a robust covariance, on the host in fp64 NumPy: wald_table's dict with
        cov = c * inv(info) meat inv(info)        (formed as (R^T R) meat (R^T R), R = info_factor(info)[0])
    and se, z, p_value from it; no dispersion factor, for the identity link too (dispersion = 1).  info, meat (M, M),
    score, coef (M,) as sandwich_device orders them (intercept first); n: the number of rows passed; n_clusters: G, the
    number of distinct labels, or None without clusters.  The scale factor c:
        "HC0", "HC2", "HC3"          c = 1
        "HC1", no clusters           c = n / (n - M)
        "HC0" with clusters (CR0)    c = 1
        "HC1" with clusters (CR1)    c = G / (G - 1) * (n - 1) / (n - M)
    Rows and clusters of weight 0 count in n and G.  A non-positive denominator (n <= M, G = 1) gives c = NaN and a NaN
    table; nothing is raised.  Adds cov_type, n_clusters, scale (= c) and meat; dof = n - M.  The NaN /
    positive_definite rules are wald_table's: an info that is not positive definite gives NaN tables and
    positive_definite = False.  n_clusters with "HC2" / "HC3" raises ValueError."""
    k = _cov_kind(kind)
    M = np.asarray(coef, dtype=np.float64).size
    n = int(n)
    if n_clusters is not None and k >= 2:
        raise ValueError("clusters go with kind 'HC0' (CR0) or 'HC1' (CR1), got %r" % kind)
    c = 1.0
    if k == 1:
        if n_clusters is None:
            c = n / (n - M) if n - M > 0 else float("nan")
        else:
            G = int(n_clusters)
            c = (G / (G - 1)) * ((n - 1) / (n - M)) if (G - 1 > 0 and n - M > 0) else float("nan")
    return _sandwich(info, meat, score, coef, c, kind, None if n_clusters is None else int(n_clusters), float(n - M))


def cox_sandwich_table(info, meat, score, coef, kind, n_clusters=None):
    """sandwich_table for a Cox model (Lin-Wei): info, meat (m, m), score, coef (m,) as cox_information_device orders
    them (no intercept), meat = sum_k L_k L_k^T or sum_g s_g s_g^T, s_g = sum_{k in g} L_k, from the score residuals L
    of cox_diagnostics_device (meat_device(L, iota, intercept=False)).  cov = c * inv(info) meat inv(info) with c = 1
    for "HC0" and c = G / (G - 1) for "HC1" with clusters (NaN for G = 1); "HC1" without clusters and "HC2" / "HC3"
    raise ValueError.  dispersion = 1 and dof = NaN (the events are not passed); an empty model gives empty arrays."""
    k = _cov_kind(kind)
    if k >= 2 or (k == 1 and n_clusters is None):
        raise ValueError("a Cox model takes kind 'HC0', or 'HC1' with clusters, got %r" % kind)
    m = np.asarray(coef, dtype=np.float64).size
    G = None if n_clusters is None else int(n_clusters)
    c = 1.0
    if k == 1:
        c = G / (G - 1) if G - 1 > 0 else float("nan")
    if m == 0:
        z = np.zeros(0)
        return {"coef": z, "se": z.copy(), "z": z.copy(), "p_value": z.copy(), "cov": np.zeros((0, 0)), "score": z.copy(),
                "dispersion": 1.0, "dof": float("nan"), "cond": float("nan"), "positive_definite": True,
                "cov_type": kind, "n_clusters": G, "scale": c, "meat": np.zeros((0, 0))}
    return _sandwich(info, meat, score, coef, c, kind, G, float("nan"))


def _survival_vector(a, n, what, stream=0, check_only=False):
    """time, status or weight of the Cox evaluation as n float64 host values; a device array is checked without a device
    call (check_only) or copied to the host with device_to_host."""
    if is_device_array(a):
        if _DeviceArray(a, what).size != n:
            raise ValueError("X.shape(0) should be equal to %s.size" % what)
        return None if check_only else np.ascontiguousarray(device_to_host(a, stream).reshape(-1))
    a = _f64(a).reshape(-1)
    if a.size != n:
        raise ValueError("X.shape(0) should be equal to %s.size" % what)
    return a


def _cox_data(a, time, status, weight, n, stream):
    """time, status (0 or 1) and weight (None = ones) of a Cox call -- n values each, host or device arrays -- as float64
    host arrays in the fields of a, checked; every shape is checked before anything is copied.  Returns {"time",
    "status"[, "weight"]}, which must stay alive for the call."""
    given = [("time", time), ("status", status)] + ([("weight", weight)] if weight is not None else [])
    for what, v in given:
        _survival_vector(v, n, what, check_only=True)
    host = {what: _survival_vector(v, n, what, stream) for what, v in given}
    if np.isnan(host["time"]).any():
        raise ValueError("There is NAN value in time")
    if not np.isin(host["status"], (0.0, 1.0)).all():
        raise ValueError("status should be 0 or 1")
    a.time, a.status, a.weight = _dp(host["time"]), _dp(host["status"]), _dp(host.get("weight"))
    return host


def evaluate_cox_device(x, cols, B, time, status, weight=None, ties="order", concordance=True, stream=0):
    """Held-out Cox partial log-likelihood and Harrell's concordance of R models on a device matrix x (n x p: float64 or
    float32, any non-negative strides), read once where it lies, the support's columns only (bessx_eval_cox_device).
    With eta = x[:, cols] @ B (no intercept; a zero coefficient takes nothing from its column), the rows in the stable
    ascending order of time and e = exp(clip(eta, -30, 30)):
        loglik[r] = sum_k w_k status_k (clip(eta_k) - log S_k),  S_k = sum of e over the rows at or after k in that order
    (ties="order", the quantity the fit reports as train_loss = -2 loglik) or over every row with time >= time_k
    (ties="breslow").  A pair k, l is comparable when status_k = 1 and time_k < time_l; it is concordant when eta_k > eta_l,
    discordant when eta_k < eta_l, tied_risk otherwise; c_index = (concordant + tied_risk / 2) / comparable (NaN without a
    comparable pair).  cols, B as in predict_device; time, status (0 or 1), weight (None = ones): n values each, host or
    device arrays (device arrays are copied to the host, n values).  Returns {"loglik": (R,), "comparable": int} plus,
    with concordance=True, "concordant", "discordant", "tied_risk" ((R,) int64, exact) and "c_index" (R,);
    concordance=False skips the O(n^2) pair kernel.  Every floating-point sum has a fixed order: the same call gives the
    same bits.  stream: raw handle of the stream x was produced on."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    if ties not in TIES:
        raise ValueError("ties must be one of %s, got %r" % (sorted(TIES), ties))
    B = np.asarray(B, dtype=np.float64)
    R = B.shape[1] if B.ndim == 2 else 1
    cols, B, _ = _predict_model(dx, cols, B, np.zeros(R))
    a = CoxEvalInput()
    _set_x(a, dx)
    a.cols, a.m, a.B, a.R = _ip(cols), cols.size, _dp(B), R
    host = _cox_data(a, time, status, weight, n, stream)  # (alive until the call has returned)
    a.ties, a.want_pairs, a.stream = TIES[ties], int(bool(concordance)), int(stream) if stream else None
    loglik, pairs, comp = np.zeros(R), np.zeros((R, 3), dtype=np.int64), _ll(0)
    _check(lib().bessx_eval_cox_device(ctypes.byref(a), _dp(loglik), pairs.ctypes.data_as(ctypes.POINTER(_ll)),
                                       ctypes.byref(comp)))
    out = {"loglik": loglik, "comparable": int(comp.value)}
    if concordance:
        out["concordant"], out["discordant"], out["tied_risk"] = (np.ascontiguousarray(pairs[:, j]) for j in range(3))
        out["c_index"] = c_index(out["concordant"], out["tied_risk"], out["comparable"])
    return out


def c_index(concordant, tied_risk, comparable):
    """(concordant + tied_risk / 2) / comparable in fp64; NaN without a comparable pair."""
    num = np.asarray(concordant, dtype=np.float64) + 0.5 * np.asarray(tied_risk, dtype=np.float64)
    return num / comparable if comparable > 0 else np.full(np.shape(num), np.nan)


def evaluate_cox_candidates(result, x, time, status, weight=None, ties="order", stream=0):
    """The train / validation split for Cox: the partial log-likelihood of every candidate of a path (fitted on the
    training rows) on held-out rows x, time, status, in ONE evaluate_cox_device call over the union of the candidates'
    supports (their coef0 is ignored: Cox has no intercept), without the pair counts.  Returns (loglik (R,), best) with
    best the index of the largest log-likelihood, the lowest index on a tie (a NaN never wins)."""
    cols, B, _ = candidate_models(result)
    ll = evaluate_cox_device(x, cols, B, time, status, weight=weight, ties=ties, concordance=False,
                             stream=stream)["loglik"]
    return ll, int(np.argmax(np.where(np.isnan(ll), -np.inf, ll)))


def op_cox_eval_bench(x, cols, R=1, ties="order", concordance=True, repeats=20):
    """Milliseconds per launch of the three stages of the Cox evaluation on the device matrix x for the support cols and
    R models, device events: (predictor pass, risk-set scan + likelihood reduction, pair counts -- 0.0 without
    concordance)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms = np.zeros(3)
    _check(lib().bessx_op_cox_eval_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, int(R), TIES[ties], int(bool(concordance)), repeats,
                                         _dp(ms)))
    return tuple(float(v) for v in ms)


SURV_KINDS = {"survival": 0, "cumhaz": 1}  # BESSX_SURV_*


def _cox_model(dx, cols, B):
    """(cols int32, B float64 (m,)) of one Cox model for the device matrix dx, checked."""
    B = np.asarray(B, dtype=np.float64)
    if B.ndim == 2 and B.shape[1] != 1:
        raise ValueError("B must hold one model (len(cols) values), got shape %s" % (B.shape,))
    cols, B, _ = _predict_model(dx, cols, B.reshape(-1), np.zeros(1))
    return cols, np.ascontiguousarray(B.reshape(-1))


def _cox_call(a, who, x, cols, beta, time, status, weight, ties, stream):
    """The fields that the input structs of the one-model Cox entry points share -- x, cols / m / beta, time / status /
    weight, ties, stream -- filled into a, after every check of them that needs no device (`who` names the wrapper in
    the message about a 2-D beta).  Returns (n, p, cols, beta, the host arrays of _cox_data): what must stay alive for the
    call."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    if ties not in TIES:
        raise ValueError("ties must be one of %s, got %r" % (sorted(TIES), ties))
    if np.ndim(beta) > 1:
        raise ValueError("beta must be 1-D: %s takes one model per call" % who)
    cols, B = _cox_model(dx, cols, np.asarray(beta, dtype=np.float64).reshape(-1))
    if not np.isfinite(B).all():
        raise ValueError("beta must be finite")
    host = _cox_data(a, time, status, weight, n, stream)
    _set_x(a, dx)
    a.cols, a.m, a.beta = _ip(cols), cols.size, _dp(B)
    a.ties, a.stream = TIES[ties], int(stream) if stream else None
    return n, p, cols, B, host


def cox_info_workspace(n, m, n_event_rows):
    """(doubles of scratch memory, (rows per slab, slabs) of the sweep over x, (rows per slab, slabs) of the sweep over the
    risk-set means) of a cox_information_device call on n rows with a support of m columns and n_event_rows rows of
    status 1 (bessx_cox_info_workspace; no device is needed).  A sweep that is not launched reports (0, 0)."""
    nd, rps, sl = _ll(0), (_ll * 2)(), (_i * 2)()
    _check(lib().bessx_cox_info_workspace(int(n), int(m), int(n_event_rows), ctypes.byref(nd), rps, sl))
    return nd.value, (int(rps[0]), int(sl[0])), (int(rps[1]), int(sl[1]))


def cox_information_device(x, cols, beta, time, status, weight=None, ties="order", stream=0):
    """Observed information and score of ONE Cox model on a device matrix x (n x p: float64 or float32, any non-negative
    strides), read where it lies (bessx_cox_info_device).  With the definitions of evaluate_cox_device -- eta =
    x[:, cols] @ beta, the rows in the stable ascending order of time, e = exp(clip(eta, -30, 30)), wd = w * status --
    r(k) = k (ties="order") or the first position with the time of k (ties="breslow"), S0_k = sum of e over the positions
    >= r(k), S1_k = sum of e * x[., cols] over them and u_k = S1_k / S0_k:
        loglik = sum_k wd_k (clip(eta_k) - log S0_k)         evaluate_cox_device's, bit for bit
        score  = sum_k wd_k (x_k - u_k)                                                             (m,)
        info   = sum_k wd_k sum_{l >= r(k)} (e_l / S0_k) (x_l - u_k)(x_l - u_k)^T      (m, m), both triangles exact mirrors
    info is the negative Hessian of loglik in beta wherever no clip is active; where one is, it is this formula and not a
    derivative.  It is formed as G1 - G2 = sum_l v_l x_l x_l^T - sum_events wd_k u_k u_k^T with v_l = e_l H_l, H the
    cumulative hazard, and score = sum_l g_l x_l with the martingale residuals g = wd - v: a DIFFERENCE, so columns far
    from centred lose digits in proportion to |G1| / |info| (survival::coxph uses the same form; centre such columns
    first).  cols: ascending distinct column numbers (may be empty: nothing of x is read, info is (0, 0) and loglik the
    null model's); beta: len(cols) finite values; time, status (0 or 1), weight (None = ones): n values each, host or
    device arrays (device arrays are copied to the host).  Returns {"info", "score", "loglik", "n_events" = sum of wd,
    "residual_sum" = sum of g, 0 up to rounding}.  x's support is read three times, no gathered copy of x[:, cols] in row
    order is made, every sum has a fixed order (the same call gives the same bits), and a NaN inside the support view
    propagates.  Scratch: about (m + 5) n + J m doubles for J event rows plus the sweeps' partials (cox_info_workspace:
    3.4 GB at n = 200 000, m = 1023, J = n).  len(cols) + 1 <= 1024.  stream: raw handle of the stream x was produced on."""
    a = CoxInfoInput()
    n, p, cols, B, host = _cox_call(a, "cox_information_device", x, cols, beta, time, status, weight, ties, stream)
    m = cols.size
    info, score = np.empty((m, m)), np.empty(m)
    a.info, a.info_ld, a.score, a.out_on_device = info.ctypes.data, m, score.ctypes.data, 0
    ll, ne, rs = _d(0), _d(0), _d(0)
    _check(lib().bessx_cox_info_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs)))
    return {"info": info, "score": score, "loglik": ll.value, "n_events": ne.value, "residual_sum": rs.value}


def op_cox_info_bench(x, cols, ties="order", repeats=20):
    """((ms of the gather of e * x into position order, ms of the column-wise suffix scan that emits the risk-set means,
    ms of every launch of a cox_information_device call), bytes the first two must move) on the device matrix x for the
    support cols (at least one column), device events."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms, nbytes = np.zeros(3), _d(0)
    _check(lib().bessx_op_cox_info_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, TIES[ties], repeats, _dp(ms), ctypes.byref(nbytes)))
    return tuple(float(v) for v in ms), nbytes.value


def cox_zph_workspace(n, m, n_event_rows):
    """(doubles of scratch memory, (rows per slab, slabs) of the sweep over x, (rows per slab, slabs) of the sweep over the
    risk-set means) of a cox_zph_device call, as cox_info_workspace states them for cox_information_device
    (bessx_cox_zph_workspace; no device is needed).  The two sweeps carry three weights each over the same row splits."""
    nd, rps, sl = _ll(0), (_ll * 2)(), (_i * 2)()
    _check(lib().bessx_cox_zph_workspace(int(n), int(m), int(n_event_rows), ctypes.byref(nd), rps, sl))
    return nd.value, (int(rps[0]), int(sl[0])), (int(rps[1]), int(sl[1]))


def cox_zph_device(x, cols, beta, time, status, gt, weight=None, ties="order", stream=0):
    """The ingredients of the proportional-hazards score test (Grambsch and Therneau, the exact form of survival::cox.zph)
    of ONE Cox model on a device matrix x, read where it lies (bessx_cox_zph_device).  Model, data and definitions are
    cox_information_device's; gt: the time transform per row (n values, host or device array; zph_transform makes it),
    read at the rows with status 1 only, finite there, already centred.  With Var_k(x) the weighted covariance of the
    support's columns over the risk set of event k and u_k their mean there, for q = 0, 1, 2
        info_q  = sum_k wd_k gt_k^q Var_k(x)          (m, m), both triangles exact mirrors
        score_q = sum_k wd_k gt_k^q (x_k - u_k)       (m,)   (q = 1: the gt-weighted sum of the Schoenfeld residuals)
    Returns {"info0", "info1", "info2", "score0", "score1", "loglik", "n_events"}; info0, score0 and loglik are
    cox_information_device's info, score and loglik bit for bit.  cox_zph_table turns them into the test.  The three
    matrices come from ONE sweep of the matrix-core Gram over x's support carrying three row weights, and one over the
    risk-set means; every sum has a fixed order (the same call gives the same bits); a NaN inside the support view
    propagates.  len(cols) + 1 <= 1024; cols may be empty (the matrices are (0, 0), loglik the null model's)."""
    a = CoxZphInput()
    n, p, cols, B, host = _cox_call(a, "cox_zph_device", x, cols, beta, time, status, weight, ties, stream)
    _survival_vector(gt, n, "gt", check_only=True)
    g = _survival_vector(gt, n, "gt", stream)
    if not np.isfinite(g[host["status"] != 0.0]).all():
        raise ValueError("gt must be finite at every row with status 1")
    m = cols.size
    out = {k: np.empty((m, m)) for k in ("info0", "info1", "info2")}
    out.update({k: np.empty(m) for k in ("score0", "score1")})
    a.gt, a.info_ld, a.out_on_device = _dp(g), m, 0
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    ll, ne = _d(0), _d(0)
    _check(lib().bessx_cox_zph_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne)))
    out.update(loglik=ll.value, n_events=ne.value)
    return out


def op_cox_zph_bench(x, cols, repeats=20):
    """(fused_ms (repeats,), separate_ms (repeats,)): single timings by device events, alternating, after one warm-up of
    each, of cox_zph_device's three-weight Gram sweep over the device matrix x for the support cols (with its finish)
    and of three back-to-back one-weight sweeps of information_device on the same data."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    fused, sep = np.zeros(repeats), np.zeros(repeats)
    _check(lib().bessx_op_cox_zph_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                        _ip(cols), cols.size, repeats, _dp(fused), _dp(sep)))
    return fused, sep


ZPH_TRANSFORMS = ("km", "rank", "identity", "log")


def zph_transform(time, status, weight=None, transform="km"):
    """(gt (n,), centre): the time transform g(t) of the proportional-hazards test at every row's time, centred, on the
    host in fp64.  transform: "identity" (t), "log" (log t; a non-positive time at a row with status 1 is a ValueError),
    "rank" (the mid-rank of t among the times of the rows with status 1: those below it plus half of those equal to it,
    plus one half), "km" (1 - S(t-), S the weighted Kaplan-Meier estimate of all rows, taken just before t -- what
    survival::cox.zph uses by default), an array of n values, or a callable applied to the times.  centre = the mean of g
    over the rows with status 1 weighted by wd = weight * status, summed in np.longdouble and rounded once (0 without
    such a row); gt = g - centre.  time, status, weight: n values each, host or device arrays (None = ones)."""
    n = _DeviceArray(time, "time").size if is_device_array(time) else np.size(time)
    time = _survival_vector(time, n, "time")
    status = _survival_vector(status, n, "status")
    w = np.ones(n) if weight is None else _survival_vector(weight, n, "weight")
    if np.isnan(time).any():
        raise ValueError("There is NAN value in time")
    if not np.isin(status, (0.0, 1.0)).all():
        raise ValueError("status should be 0 or 1")
    ev = status != 0.0
    if callable(transform):
        g = _f64(transform(time)).reshape(-1)
        if g.size != n:
            raise ValueError("transform must return n = %d values, got %d" % (n, g.size))
    elif not isinstance(transform, str):
        g = _survival_vector(transform, n, "transform").copy()
    elif transform == "identity":
        g = time.copy()
    elif transform == "log":
        if (time[ev] <= 0.0).any():
            raise ValueError('transform="log" needs positive times at the rows with status 1')
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.log(time)
    elif transform == "rank":
        te = np.sort(time[ev])
        g = 0.5 * (np.searchsorted(te, time, side="left") + np.searchsorted(te, time, side="right") + 1.0)
    elif transform == "km":
        u, S = _km_survival(time, status, w)
        Sl = np.concatenate([[1.0], S])  # (S just before u[i] is S at u[i - 1], and 1 before the first time)
        g = 1.0 - Sl[np.searchsorted(u, time, side="left")]
    else:
        raise ValueError("transform must be one of %s, an array of n values or a callable, got %r"
                         % (list(ZPH_TRANSFORMS), transform))
    if not np.isfinite(g[ev]).all():
        raise ValueError("the transform must be finite at every row with status 1")
    wd = (w * status)[ev].astype(np.longdouble)
    sw = wd.sum()
    centre = float((wd * g[ev].astype(np.longdouble)).sum() / sw) if sw > 0 else 0.0
    return g - centre, centre


def _scaled_factor(A):
    """(inverse(A), cond of the scaled matrix, positive definite) by _wald's scaled Cholesky factorisation and tests."""
    M = A.shape[0]
    dg = np.diag(A)
    if not (np.isfinite(A).all() and (dg > 0).all()):
        return None, float("nan"), False
    d = 1.0 / np.sqrt(dg)
    S = A * d[:, None] * d[None, :]
    S = 0.5 * (S + S.T)
    ev = np.linalg.eigvalsh(S)
    if not (ev[0] > M * np.finfo(np.float64).eps * ev[-1]):
        return None, float("inf") if ev[0] <= 0 else float(ev[-1] / ev[0]), False
    try:
        Lc = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None, float(ev[-1] / ev[0]), False
    Li = np.linalg.solve(Lc, np.eye(M))
    return (Li.T @ Li) * d[:, None] * d[None, :], float(ev[-1] / ev[0]), True


def cox_zph_table(got, centre=None):
    """The proportional-hazards test from cox_zph_device's dict (or the host route's), on the host in fp64 NumPy with
    the scaled Cholesky factorisations of wald_table: D = info2 - info1 inverse(info0) info1, the information about
    theta in beta(t) = beta + theta g(t) at theta = 0 with beta profiled out (score0 is taken as 0: the model is at its
    optimum).  Returns {"chisq": score1_j^2 / D_jj (m,), "p_value": chi2_sf(chisq, 1), "global_chisq": score1^T
    inverse(D) score1, "global_df": m, "global_p_value", "slope_var": diag(inverse(D)), "cond": the 2-norm condition
    number of the scaled D, "cond_info": that of the scaled info0, "positive_definite", "score0", "score1", "n_events",
    "gt_centre": centre}.  When info0 or D is not positive definite by wald_table's tests -- no event, every event with
    one value of g (D = 0 up to rounding: a diagonal entry of D not above sqrt(eps) times info2's counts as 0), duplicated
    columns -- the statistics are NaN and positive_definite is False: data decide
    that, so nothing is raised.  An empty model gives empty arrays, a global statistic of 0 and positive_definite True."""
    I0, I1, I2 = (np.array(got[k], dtype=np.float64) for k in ("info0", "info1", "info2"))
    s0, s1 = (np.asarray(got[k], dtype=np.float64).reshape(-1) for k in ("score0", "score1"))
    m = s1.size
    if I0.shape != (m, m) or I1.shape != (m, m) or I2.shape != (m, m) or s0.shape != (m,):
        raise ValueError("info0, info1, info2 must be (%d, %d) and score0, score1 (%d,)" % (m, m, m))
    nan_v = np.full(m, np.nan)
    out = {"chisq": nan_v, "p_value": nan_v.copy(), "global_chisq": float("nan"), "global_df": m,
           "global_p_value": float("nan"), "slope_var": nan_v.copy(), "cond": float("nan"), "cond_info": float("nan"),
           "positive_definite": False, "score0": s0, "score1": s1, "n_events": float(got.get("n_events", float("nan"))),
           "gt_centre": centre}
    if m == 0:
        out.update(global_chisq=0.0, global_p_value=1.0, positive_definite=True)
        return out
    C0, out["cond_info"], ok = _scaled_factor(I0)
    if not ok or not (np.isfinite(I1).all() and np.isfinite(I2).all() and np.isfinite(s1).all()):
        return out
    D = I2 - I1 @ C0 @ I1
    D = 0.5 * (D + D.T)
    # (D is a difference of matrices that are differences themselves: a diagonal entry that keeps less than sqrt(eps) of
    # info2's has lost half its digits and counts as 0, whatever its sign -- one event time, or one value of g)
    if not (np.diag(D) > np.sqrt(np.finfo(np.float64).eps) * np.abs(np.diag(I2))).all():
        return out
    Dinv, out["cond"], ok = _scaled_factor(D)
    if not ok:
        return out
    chisq = s1 * s1 / np.diag(D)
    gl = float(s1 @ Dinv @ s1)
    out.update(chisq=chisq, p_value=np.array([chi2_sf(v, 1) for v in chisq]), global_chisq=gl,
               global_p_value=chi2_sf(gl, m), slope_var=np.diag(Dinv).copy(), positive_definite=True)
    return out


def cox_addscore_workspace(n, m, n_event_rows, q, candidate_block=0):
    """What a cox_addscore_device call on n rows (n_event_rows of them with status 1) with a support of m columns and q
    candidates needs and how it is split (bessx_cox_addscore_workspace; no device is needed): {"doubles": scratch
    memory in all, "block_doubles": the part of it that does not depend on p, "rows_per_slab", "slabs": the row split of
    the matrix-core pass behind u, c, d, "quad_rows_per_slab", "quad_slabs": the position split of the streaming pass
    behind t -- functions of (n, m, q, candidate_block) alone --, "block": candidates per block, "sum_depth": the
    additions behind one s_j, "chain": the longest chain of additions behind an entry of u, c, d, "quad_chain": behind
    a t_j}."""
    nd, bd, rps, sl, bl, dp, ch = _ll(0), _ll(0), (_ll * 2)(), (_i * 2)(), _i(0), _i(0), (_i * 2)()
    _check(lib().bessx_cox_addscore_workspace(int(n), int(m), int(n_event_rows), int(q), int(candidate_block),
                                              ctypes.byref(nd), ctypes.byref(bd), rps, sl, ctypes.byref(bl),
                                              ctypes.byref(dp), ch))
    return {"doubles": nd.value, "block_doubles": bd.value, "rows_per_slab": int(rps[0]), "slabs": int(sl[0]),
            "quad_rows_per_slab": int(rps[1]), "quad_slabs": int(sl[1]), "block": bl.value, "sum_depth": dp.value,
            "chain": int(ch[0]), "quad_chain": int(ch[1])}


def cox_addscore_device(x, cols, beta, time, status, weight=None, ties="order", factor=None, candidates=None,
                        candidate_block=0, want_cross=False, stream=0):
    """The ingredients of the Rao score test of every candidate column against ONE Cox model on a device matrix x (n x p:
    float64 or float32, any non-negative strides), read where it lies (bessx_cox_addscore_device).  The model, the
    positions and e, wd, S0, v, g, info, score, loglik, n_events, residual_sum are cox_information_device's (the same
    bits).  candidates: None = all p columns, else ascending distinct column numbers.  factor: R, lower triangular (m,
    m) with inv(info) = R^T R; None = cox_information_device and info_factor are called first (and when the information
    is not positive definite, s and a are NaN).  With dh_p the hazard increment at position p, u_p the risk-set mean
    over the support, A_l = sum_{p <= l} dh_p u_p, r = inv(info) @ score, for candidate j
        u_j = sum_l g_l x_lj,   c_j = sum_l x_lj (v_l x_l - e_l A_l),   d_j = sum_l v_l x_lj^2,
        t_j = sum_p (dh_p / S0_p) (sum_{l >= p} e_l x_lj)^2,   s_j = |R c_j|^2,   a_j = c_j . r
    -- row j of the score and of the observed information of the model extended by column j at coefficient 0, whose
    diagonal entry is d_j - t_j.  Returns {"columns", "u", "d", "t", "s", "a", "info", "score", "loglik", "n_events",
    "residual_sum", "positive_definite", "support"} (NumPy, host) plus "cross" (q, m), the c_j, when want_cross.  The
    subtractions u - a and (d - t) - s are cox_score_test_table's; d - t loses digits for columns far from centred
    (cox_information_device's G1 - G2 caveat).  m = 0 is the test against the null model (s = a = 0).  u, c, d take one
    pass over the candidate columns on the fp64 matrix cores and t a second, streaming one; no n x q temporary and no
    risk-set mean of a candidate is formed; candidates go in blocks of candidate_block (0 = the library's choice; a
    multiple of 16), so scratch beyond the support-sized arrays and the panel does not depend on p
    (cox_addscore_workspace).  The same call gives the same bits, and every layout of the same values of one dtype
    gives the same bits.  Groups of columns with more than one degree of freedom: cox_groupscore_device.  Not for Efron
    ties or strata, not corrected for selection.  len(cols) + 1 <= 1024.  stream: raw handle of the stream x was produced on."""
    a = CoxAddscoreInput()
    n, p, cols, B, host = _cox_call(a, "cox_addscore_device", x, cols, beta, time, status, weight, ties, stream)
    cand, q = _candidates(candidates, p)
    m = cols.size
    pd = True
    fh = None
    if m == 0:
        pass
    elif factor is None:
        first = cox_information_device(x, cols, B, host["time"], host["status"], weight=host.get("weight"), ties=ties,
                                       stream=stream)
        fh, pd = info_factor(first["info"])
    else:
        fh = _f64(factor)
        if fh.shape != (m, m):
            raise ValueError("factor must have shape (%d, %d), got %s" % (m, m, fh.shape))
    if pd and m > 0:
        a.factor, a.factor_ld = _dp(fh), m
    a.candidates, a.q, a.candidate_block = _ip(cand), q, int(candidate_block)
    info, score = np.empty((m, m)), np.empty(m)
    out = np.full((5, q), np.nan)
    a.info, a.info_ld, a.score = _dp(info), m, _dp(score)
    a.u, a.d, a.t, a.s, a.a = (out[k].ctypes.data for k in range(5))
    cross = None
    if want_cross:
        cross = np.empty((q, m + 1))
        a.cross, a.cross_ld = cross.ctypes.data, m + 1
    a.out_on_device = 0
    ll, ne, rs = _d(0), _d(0), _d(0)
    _check(lib().bessx_cox_addscore_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs)))
    got = {"columns": np.arange(p, dtype=np.int64) if cand is None else cand.astype(np.int64), "u": out[0], "d": out[1],
           "t": out[2], "s": out[3], "a": out[4], "info": info, "score": score, "loglik": ll.value, "n_events": ne.value,
           "residual_sum": rs.value, "positive_definite": bool(pd), "support": cols.astype(np.int64)}
    if want_cross:
        got["cross"] = np.ascontiguousarray(cross[:, 1:])  # (column 0 is sum_l v_l x_lj: not an entry of c_j)
    return got


def cox_score_test_table(got):
    """The Rao score test of every candidate from what cox_addscore_device (or the NumPy route) returns, on the host in
    fp64: score = u - a, variance = (d - t) - s, statistic = score^2 / variance where variance is finite and > 0, else
    NaN; p_value = erfc(sqrt(statistic / 2)), chi-square with 1 degree of freedom; dispersion = 1.  A candidate that is
    in the model's support ("support" of got) has in_model = True and NaN for statistic and p_value: its variance is
    rounding noise.  When the information is not positive definite s and a are NaN and so is every statistic.  Returns
    {"columns", "score", "variance", "statistic", "p_value", "in_model", "dispersion"}.  Selection is not corrected
    for."""
    import math
    u, a = np.asarray(got["u"], dtype=np.float64), np.asarray(got["a"], dtype=np.float64)
    d, t = np.asarray(got["d"], dtype=np.float64), np.asarray(got["t"], dtype=np.float64)
    s = np.asarray(got["s"], dtype=np.float64)
    columns = np.asarray(got["columns"], dtype=np.int64)
    adj, var = u - a, (d - t) - s
    in_model = np.isin(columns, np.asarray(got.get("support", np.zeros(0)), dtype=np.int64))
    ok = np.isfinite(var) & (var > 0) & ~in_model
    stat = np.full(columns.size, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        stat[ok] = (adj[ok] * adj[ok]) / var[ok]
    pv = np.array([math.erfc(math.sqrt(v / 2.0)) if (v == v and v >= 0) else float("nan") for v in stat])
    return {"columns": columns, "score": adj, "variance": var, "statistic": stat, "p_value": pv, "in_model": in_model,
            "dispersion": 1.0}


def op_cox_addscore_bench(x, cols, candidates=None, candidate_block=0, sorted_rows=False, repeats=5):
    """(ms per stage, bytes the streaming pass needs) of the Cox score-test kernels on the device matrix x for the support
    cols, device events, each over every block of candidates: {"pack", "cross", "quad", "quad_finish", "finish",
    "statistic"} (bessx_op_cox_addscore_bench).  sorted_rows: the rows are taken to be in time order already; else a
    scattered order.  The bytes are the candidate columns read once."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    cand, q = _candidates(candidates, dx.shape[1])
    ms, nbytes = (_d * 6)(), _d(0)
    _check(lib().bessx_op_cox_addscore_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                             _ip(cols), cols.size, _ip(cand), q, int(candidate_block),
                                             1 if sorted_rows else 0, repeats, ms, ctypes.byref(nbytes)))
    return dict(zip(("pack", "cross", "quad", "quad_finish", "finish", "statistic"), [float(v) for v in ms])), nbytes.value


def cox_groupscore_workspace(n, p, m, n_event_rows, group_starts, groups=None, candidate_block=0):
    """What a cox_groupscore_device call on n rows (n_event_rows of them with status 1) and p columns with a support of m
    columns needs and how it is split (bessx_cox_groupscore_workspace; no device is needed): groupscore_workspace's dict
    ("doubles", "block_doubles", "rows_per_slab", "slabs", "gram_rows_per_slab", "gram_slabs", "blocks", "block_first",
    "band", "depth", "score_depth", "gram_depth", "s_depth") plus "t_rows_per_slab", "t_slabs": the position split of
    the risk-set term T, a function of n alone, and "t_depth": the roundings behind a term of an entry of T."""
    gs, tg = _group_lists(group_starts, groups, p)
    nt = gs.size if tg is None else tg.size
    nd, bd, rps, sl, nb, first, band, dep = _ll(0), _ll(0), (_ll * 3)(), (_i * 3)(), _i(0), (_i * (nt + 1))(), _i(0), (_i * 5)()
    _check(lib().bessx_cox_groupscore_workspace(int(n), int(p), int(m), int(n_event_rows), _ip(gs), gs.size, _ip(tg), nt,
                                                int(candidate_block), ctypes.byref(nd), ctypes.byref(bd), rps, sl,
                                                ctypes.byref(nb), first, ctypes.byref(band), dep))
    return {"doubles": nd.value, "block_doubles": bd.value, "rows_per_slab": rps[0], "slabs": sl[0],
            "gram_rows_per_slab": rps[1], "gram_slabs": sl[1], "t_rows_per_slab": rps[2], "t_slabs": sl[2],
            "blocks": nb.value, "block_first": [int(first[k]) for k in range(nb.value + 1)], "band": band.value,
            "depth": dep[0], "score_depth": dep[1], "gram_depth": dep[2], "s_depth": dep[3], "t_depth": dep[4]}


def cox_groupscore_device(x, cols, beta, time, status, group_starts, groups=None, weight=None, ties="order", factor=None,
                          stream=0, candidate_block=0):
    """The ingredients of the Rao score test of every tested GROUP of columns against ONE Cox model on a device matrix x
    (n x p: float64 or float32, any non-negative strides), read where it lies (bessx_cox_groupscore_device).  The model,
    the positions, e, S0, v, g, info, score, loglik, n_events, residual_sum, factor and r are cox_addscore_device's;
    group_starts, groups and candidate_block are groupscore_device's.  With P cox_addscore_device's panel (rows v_i x_i -
    e_i A_pos(i)), cc_p = dh_p / S0_p and s_p = sum_{l >= p} e_l x_{l,J} over the positions in time order, for a tested
    group with columns J, d = len(J) <= 64:
        u = X_J^T g,   C = X_J^T P,   a = C r,   D = X_J^T diag(v) X_J,   T = sum_p cc_p s_p s_p^T,   S = (C R^T)(C R^T)^T
    -- the rows J of the score and the block (D - T) - S of the observed information of the model extended by the group
    at coefficient 0.  Returns groupscore_device's dict with "T" added and "loglik", "n_events", "residual_sum" in place
    of "loss", "sum_w".  The subtractions, the d x d Cholesky factor and the quadratic form are
    cox_group_score_test_table's; D - T loses digits for columns far from centred.  m = 0 is the test against the null
    model (S = 0, a = 0).  factor None: cox_information_device and info_factor are called first (and when the information
    is not positive definite, S and a are NaN).  The band of T is formed on the fp64 matrix cores from running suffix
    sums with x read in place; no n x q temporary; scratch beyond the panel does not depend on p
    (cox_groupscore_workspace).  The same call gives the same bits, and every layout of the same values of one dtype and
    every candidate_block gives the same bits.  A tested group wider than 64 columns is BessxError code 3.  Not for Efron
    ties or strata, not corrected for selection.  len(cols) + 1 <= 1024.  stream: raw handle of the stream x was
    produced on."""
    a = CoxGroupscoreInput()
    n, p, cols, B, host = _cox_call(a, "cox_groupscore_device", x, cols, beta, time, status, weight, ties, stream)
    gs, tg = _group_lists(group_starts, groups, p)
    nt = gs.size if tg is None else tg.size
    lists = _group_columns(gs, tg, p)
    ok = lists is not None and lists[1].max() <= GROUPSCORE_WIDTH_MAX  # (else the library refuses before it writes)
    q, tot = (int(lists[1].sum()), int((lists[1] * lists[1]).sum())) if ok else (1, 1)
    m = cols.size
    pd, fh = True, None
    if m == 0:
        pass
    elif factor is None:
        first = cox_information_device(x, cols, B, host["time"], host["status"], weight=host.get("weight"), ties=ties,
                                       stream=stream)
        fh, pd = info_factor(first["info"])
    else:
        fh = _f64(factor)
        if fh.shape != (m, m):
            raise ValueError("factor must have shape (%d, %d), got %s" % (m, m, fh.shape))
    if pd and m > 0:
        a.factor, a.factor_ld = _dp(fh), m
    a.group_starts, a.n_groups, a.groups, a.n_tested = _ip(gs), gs.size, _ip(tg), nt
    a.candidate_block = int(candidate_block)
    info, score = np.empty((m, m)), np.empty(m)
    vec, blk, offsets = np.full((2, q), np.nan), np.full((3, tot), np.nan), np.zeros(nt + 1, dtype=np.int64)
    a.info, a.info_ld, a.score = _dp(info), m, _dp(score)
    a.u, a.a = vec[0].ctypes.data, vec[1].ctypes.data
    a.D, a.T, a.S = blk[0].ctypes.data, blk[1].ctypes.data, blk[2].ctypes.data
    a.offsets = offsets.ctypes.data_as(ctypes.POINTER(_ll))
    a.out_on_device = 0
    ll, ne, rs = _d(0), _d(0), _d(0)
    _check(lib().bessx_cox_groupscore_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs)))
    return {"columns": lists[2], "group_of_column": lists[3], "u": vec[0], "a": vec[1], "D": blk[0], "T": blk[1],
            "S": blk[2], "offsets": offsets, "info": info, "score": score, "loglik": ll.value, "n_events": ne.value,
            "residual_sum": rs.value, "positive_definite": bool(pd), "support": cols.astype(np.int64)}


def cox_group_score_test_table(got):
    """The Rao score test of every tested group from what cox_groupscore_device (or the NumPy route) returns, on the host
    in fp64: group_score_test_table's operations and NaN rules with V = (D - T) - S and dispersion 1.  Returns its dict.
    Selection is not corrected for."""
    D, T = np.asarray(got["D"], dtype=np.float64), np.asarray(got["T"], dtype=np.float64)
    S = np.asarray(got["S"], dtype=np.float64)
    return _group_score_table(got, lambda lo, hi: (D[lo:hi] - T[lo:hi]) - S[lo:hi], 1.0)


def op_cox_groupscore_bench(x, cols, group_starts, groups=None, candidate_block=0, sorted_rows=False, repeats=5):
    """(ms per step, bytes the band of T needs) of the Cox group score test on the device matrix x for the support cols,
    device events, each over every block of candidates: {"pack", "cross", "finish", "gram", "gram_sum", "s_band",
    "extract", "t_band", "t_finish"} (bessx_op_cox_groupscore_bench).  sorted_rows: the rows are taken to be in time
    order already; else a scattered order.  The bytes are the tested columns read once."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    gs, tg = _group_lists(group_starts, groups, dx.shape[1])
    ms, nbytes = (_d * 9)(), _d(0)
    _check(lib().bessx_op_cox_groupscore_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                               _ip(cols), cols.size, _ip(gs), gs.size, _ip(tg),
                                               gs.size if tg is None else tg.size, int(candidate_block),
                                               1 if sorted_rows else 0, repeats, ms, ctypes.byref(nbytes)))
    names = ("pack", "cross", "finish", "gram", "gram_sum", "s_band", "extract", "t_band", "t_finish")
    return dict(zip(names, [float(v) for v in ms])), nbytes.value


COX_DIAG_KINDS = ("martingale", "deviance", "score", "dfbeta", "displacement", "schoenfeld")  # BESSX_COX_DIAG_* bits
COX_DIAG_ROW_KINDS = ("martingale", "deviance", "displacement")  # the (n,) kinds, in the order of their slots


def _cox_diag_mask(kinds):
    """(bit mask, names in ascending bit order) of an iterable of kind names (or one name)."""
    if isinstance(kinds, str):
        kinds = (kinds,)
    kinds = tuple(kinds)
    for k in kinds:
        if k not in COX_DIAG_KINDS:
            raise ValueError("kinds must be taken from %s, got %r" % (list(COX_DIAG_KINDS), k))
    if not kinds:
        raise ValueError("kinds must name at least one of %s" % (list(COX_DIAG_KINDS),))
    names = tuple(k for k in COX_DIAG_KINDS if k in kinds)
    return sum(1 << COX_DIAG_KINDS.index(k) for k in names), names


def cox_diag_workspace(n, m, n_event_rows, kinds=COX_DIAG_KINDS):
    """Doubles of scratch memory of a cox_diagnostics_device call on n rows with a support of m columns and
    n_event_rows rows of status 1 (bessx_cox_diag_workspace; no device is needed): about (2 m + 6) n + J m when score,
    dfbeta, displacement or schoenfeld is asked for, n-vectors only for martingale / deviance alone."""
    mask, _ = _cox_diag_mask(kinds)
    nd = _ll(0)
    _check(lib().bessx_cox_diag_workspace(int(n), int(m), int(n_event_rows), mask, ctypes.byref(nd)))
    return nd.value


def cox_diagnostics_device(x, cols, beta, time, status, factor=None, cinv=None, weight=None, ties="order",
                           kinds=COX_DIAG_KINDS, stream=0):
    """Residuals, dfbeta and case influence of ONE Cox model on a device matrix x (n x p: float64 or float32, any
    non-negative strides), read where it lies (bessx_cox_diag_device).  With the quantities of cox_information_device
    (positions k in time order, r(k), e, wd = w * status, S0, u_k = S1_k / S0_k, H, v = e H, g = wd - v),
    dh_p = sum_{k: r(k) = p} wd_k / S0_p and A_l = sum_{p <= l} dh_p u_p:
        martingale    g_k = wd_k - v_k                                                              (n,)
        deviance      sign(g_k) sqrt(2 max(v_k - wd_k + wd_k log(wd_k / v_k), 0)), 0 log 0 = 0       (n,)
        score         L_k = g_k x_k - wd_k u_r(k) + e_k A_k; its column sums are the score           (n, m)
        dfbeta        L_k @ cinv, cinv = inv(info): the approximate change in beta without row k     (n, m)
        displacement  L_k^T cinv L_k = sum_j t_kj^2, t_k = factor @ L_k (info_factor's R)            (n,)
        schoenfeld    x_k - u_k for the J rows with status 1, in time (position) order               (J, m)
    Everything but schoenfeld is in row order.  factor (m, m) lower triangular with inv(info) = R^T R is needed by
    displacement, cinv (m, m) symmetric by dfbeta; both are host arrays.  time, status (0 or 1), weight (None = ones):
    n values each, host or device arrays (device arrays are copied to the host).  Returns a dict from kind name to its
    array plus "event_rows" (J,) int32, the row of every schoenfeld row, and "event_times" (J,): torch tensors on x's
    device when x is a torch tensor (torch is looked up, never imported; the (n,) kinds are views of one tensor, the
    matrices are (n, m) / (J, m) views with unit stride along n / J), NumPy arrays of the same layout for any other
    device object; event_rows and event_times are always NumPy.  No clamp besides the one of eta at +-30 and the
    max(., 0) of the deviance; a NaN inside the support propagates.  x's support is read three times (predictor, the
    gather of e x, the forming of L) plus the J event rows for schoenfeld; the same call gives the same bits.
    len(cols) + 1 <= 1024.  stream: raw handle of the stream x was produced on."""
    mask, names = _cox_diag_mask(kinds)
    a = CoxDiagInput()
    n, p, cols, B, host = _cox_call(a, "cox_diagnostics_device", x, cols, beta, time, status, weight, ties, stream)
    m = cols.size
    J = int(np.count_nonzero(host["status"]))
    a.kinds = mask
    keep = []
    for what, mat in (("factor", factor), ("cinv", cinv)):
        if mat is not None:
            mh = _f64(mat)
            if mh.shape != (m, m):
                raise ValueError("%s must have shape (%d, %d), got %s" % (what, m, m, mh.shape))
            setattr(a, what, _dp(mh))
            setattr(a, what + "_ld", max(m, 1))
            keep.append(mh)
    rows = [k for k in COX_DIAG_ROW_KINDS if k in names]
    torch = sys.modules.get("torch")
    on_torch = torch is not None and isinstance(x, torch.Tensor)

    def empty(r, c):  # (r, c) with unit stride along c
        if on_torch:
            t = torch.empty((r, c), dtype=torch.float64, device=x.device)
            return t, int(t.data_ptr())
        t = np.empty((r, c))
        return t, int(t.ctypes.data)

    out = {}
    a.out_on_device = 1 if on_torch else 0
    if rows:
        buf, a.out_rows = empty(len(rows), n)
        a.out_rows_ld = n
        out.update((k, buf[s]) for s, k in enumerate(rows))
    for k, cnt in (("score", n), ("dfbeta", n), ("schoenfeld", J)):
        if k in names:
            buf, ptr = empty(m, cnt)
            setattr(a, "out_" + k, ptr)
            setattr(a, "out_%s_ld" % k, max(cnt, 1))
            out[k] = buf.T
    ev = np.zeros(J, dtype=np.int32)
    a.event_rows = _ip(ev)
    nj = _i(0)
    _check(lib().bessx_cox_diag_device(ctypes.byref(a), ctypes.byref(nj)))
    assert nj.value == J
    out = {k: out[k] for k in names}
    out["event_rows"] = ev
    out["event_times"] = host["time"][ev]
    return out


def op_cox_diag_bench(x, cols, ties="order", repeats=20):
    """((ms of the increments and their forward scan, ms of those plus the forming of L, ms of L R^T with the
    displacement epilogue, ms of L C with the dfbeta epilogue), bytes the last three must move) on the device matrix x
    for the support cols (at least one column), device events; the data are op_cox_info_bench's."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    ms, nbytes = np.zeros(4), _d(0)
    _check(lib().bessx_op_cox_diag_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, TIES[ties], repeats, _dp(ms), ctypes.byref(nbytes)))
    return tuple(float(v) for v in ms), nbytes.value

def cox_baseline_device(x, cols, B, time, status, weight=None, stream=0):
    """The Breslow baseline cumulative hazard of one Cox model on the rows it was fitted to, x a device matrix (n x p:
    float64 or float32, any non-negative strides) read once where it lies, the support's columns only
    (bessx_cox_baseline_device).  With eta = x[:, cols] @ B, the rows in the stable ascending order of time,
    e = exp(clip(eta, -30, 30)) and S_k the sum of e over every row with time >= time_k:
        H0(t) = sum over the rows k with time_k <= t of w_k status_k / S_k.
    cols, B as in predict_device (one model); time, status (0 or 1), weight (None = ones, else >= 0): n values each, host or
    device arrays (device arrays are copied to the host).  Returns {"times": (J,) the distinct times that carry an event,
    ascending, "cumhaz": (J,) H0 at them, "n_events": sum of w * status}; J = 0 when every row is censored.  The prefix
    sum is fp64, additions only, in a fixed order: the same call gives the same bits."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    cols, B = _cox_model(dx, cols, B)
    a = CoxBaselineInput()
    host = _cox_data(a, time, status, weight, n, stream)
    if weight is not None and not (host["weight"] >= 0.0).all():
        raise ValueError("weight should be non-negative")
    _set_x(a, dx)
    a.cols, a.m, a.B = _ip(cols), cols.size, _dp(B)
    a.stream = int(stream) if stream else None
    J, times, cumhaz = _i(0), np.zeros(n), np.zeros(n)
    _check(lib().bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(J), _dp(times), _dp(cumhaz)))
    w = host.get("weight")
    return {"times": times[:J.value].copy(), "cumhaz": cumhaz[:J.value].copy(),
            "n_events": float(np.sum(host["status"] if w is None else w * host["status"]))}


def baseline_at(base_times, base_cumhaz, times):
    """The baseline cumulative hazard as a right-continuous step function, on the host: H0(t) = base_cumhaz at the last
    base_times <= t, 0 before the first.  base_times ascending; times in any order, repeats allowed; a NaN in times is a
    ValueError.  Returns an array of the shape of times."""
    base_times, base_cumhaz = _f64(base_times).reshape(-1), _f64(base_cumhaz).reshape(-1)
    if base_times.size != base_cumhaz.size:
        raise ValueError("base_times and base_cumhaz must have the same size, got %d and %d"
                         % (base_times.size, base_cumhaz.size))
    times = np.asarray(times, dtype=np.float64)
    if np.isnan(times).any():
        raise ValueError("There is NAN value in times")
    idx = np.searchsorted(base_times, times, side="right")
    return np.where(idx > 0, np.concatenate([[0.0], base_cumhaz])[idx], 0.0)


def cox_survival_device(x, cols, B, base_times, base_cumhaz, times=None, kind="survival", out=None, stream=0):
    """Survival curves of one Cox model for the rows of a device matrix x (n x p: float64 or float32, any non-negative
    strides), read once where it lies, the support's columns only (bessx_cox_survival_device): with eta = x[:, cols] @ B,
    e = exp(clip(eta, -30, 30)) and H0 = baseline_at(base_times, base_cumhaz, times),
        kind="survival":  S(t_j | x_i) = exp(-(H0(t_j) * e_i)),        kind="cumhaz":  H0(t_j) * e_i,
    an (n, T) matrix that is written exactly once.  base_times, base_cumhaz: what cox_baseline_device returned;
    times=None means the baseline's own times.  out: a float64 device array of shape (n, T) to write into, any strides;
    out=None allocates a torch tensor on x's device when x is a torch tensor (torch is looked up, never imported) and
    returns a NumPy array for any other device object.  stream: raw handle of the stream x was produced on; the result is
    complete when the call returns."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    if kind not in SURV_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(SURV_KINDS), kind))
    cols, B = _cox_model(dx, cols, B)
    grid = base_times if times is None else times
    if np.ndim(grid) > 1:
        raise ValueError("times must be 1-D")
    hg = np.ascontiguousarray(baseline_at(base_times, base_cumhaz, grid).reshape(-1))
    T = hg.size
    if T < 1:
        raise ValueError("times is empty: no curve to compute (a baseline without an event has no times of its own)")
    if not (hg >= 0.0).all():
        raise ValueError("base_cumhaz should be non-negative")
    if out is not None:
        if not is_device_array(out):
            raise ValueError("out must be a device array")
        do = _DeviceArray(out, "out")
        if do.item != 8:
            raise ValueError("out: a device array of float64 is needed (typestr '<f8')")
        if do.shape != (n, T):
            raise ValueError("out must have shape %s, got %s" % ((n, T), do.shape))
        ptr, ors, ocs, on_device, result = do.ptr, do.strides[0], do.strides[1], 1, out
    else:
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(x, torch.Tensor):
            result = torch.empty((n, T), dtype=torch.float64, device=x.device)
            ptr, on_device = int(result.data_ptr()), 1
        else:
            result = np.empty((n, T))
            ptr, on_device = int(result.ctypes.data), 0
        ors, ocs = T, 1
    a = CoxSurvivalInput()
    _set_x(a, dx)
    a.cols, a.m, a.B, a.hg, a.T, a.kind = _ip(cols), cols.size, _dp(B), _dp(hg), T, SURV_KINDS[kind]
    a.out_row_stride, a.out_col_stride, a.out_on_device = ors, ocs, on_device
    a.stream = int(stream) if stream else None
    _check(lib().bessx_cox_survival_device(ctypes.byref(a), ptr))
    return result


def rmst_segments(base_times, base_cumhaz, tau):
    """The step function S(t | x) = exp(-H0(t) e) cut into the segments that the restricted mean survival time
    RMST(tau) = integral_0^tau S(t | x) dt sums over, on the host: (hs, wd, cut) with
        RMST_i(tau[j]) = sum over k < cut[j] of wd[k] * exp(-(hs[k] * e_i)).
    The breakpoints are 0, every base time below max(tau) and every tau, merged in ascending order; segment k spans
    [a_k, b_k) with hs[k] = baseline_at(base_times, base_cumhaz, a_k) and wd[k] = b_k - a_k in fp64 (segments of zero
    width are dropped), and cut[j] is the number of segments that end at or before tau[j].  base_times ascending and
    non-negative (what cox_baseline_device returned); tau 1-D with at least one value, finite and >= 0, in any order,
    repeats allowed.  The curve keeps its last value beyond the last base time; tau = 0 gives cut = 0 (an RMST of exactly
    0.0); a baseline without an event gives the segments of hazard 0 (an RMST of exactly tau).  A NaN or negative or
    infinite tau, or a negative base time, is a ValueError.  Returns (hs float64 (K,), wd float64 (K,), cut int32 (T,))."""
    base_times, base_cumhaz = _f64(base_times).reshape(-1), _f64(base_cumhaz).reshape(-1)
    if base_times.size != base_cumhaz.size:
        raise ValueError("base_times and base_cumhaz must have the same size, got %d and %d"
                         % (base_times.size, base_cumhaz.size))
    tau = np.asarray(tau, dtype=np.float64)
    if tau.ndim != 1 or tau.size < 1:
        raise ValueError("tau must be 1-D with at least one value, got shape %s" % (tau.shape,))
    if np.isnan(tau).any():
        raise ValueError("There is NAN value in tau")
    if not (np.isfinite(tau) & (tau >= 0.0)).all():
        raise ValueError("tau should be finite and non-negative")
    if np.isnan(base_times).any():
        raise ValueError("There is NAN value in base_times")
    if (base_times < 0.0).any():
        raise ValueError("base_times should be non-negative")
    pts = np.unique(np.concatenate([[0.0], base_times[base_times < tau.max()], tau]))  # ascending and distinct
    hs = np.ascontiguousarray(baseline_at(base_times, base_cumhaz, pts[:-1]))
    wd = np.ascontiguousarray(pts[1:] - pts[:-1])
    return hs, wd, np.searchsorted(pts, tau).astype(np.int32)


def survival_levels(q):
    """The cumulative-hazard levels c = -log1p(-q) of the q-quantiles of the survival time (S(t) <= 1 - q exactly when
    H(t) >= c), in fp64; q 0-D or 1-D with every value in (0, 1), else a ValueError."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.size < 1:
        raise ValueError("q must be a number or 1-D with at least one value, got shape %s" % (q.shape,))
    if not ((q > 0.0) & (q < 1.0)).all():
        raise ValueError("q should lie strictly between 0 and 1")
    return -np.log1p(-q)


def _hazard_levels(q, hazard_levels):
    """The (Q,) levels c > 0 of a quantile request given as q or as hazard_levels (one of the two)."""
    if q is not None and hazard_levels is not None:
        raise ValueError("give q or hazard_levels, not both")
    if q is not None:
        return np.ascontiguousarray(survival_levels(q))
    c = np.atleast_1d(np.asarray(hazard_levels, dtype=np.float64))
    if c.ndim != 1 or c.size < 1:
        raise ValueError("hazard_levels must be a number or 1-D with at least one value, got shape %s" % (c.shape,))
    if not (c > 0.0).all():
        raise ValueError("hazard_levels should be positive")
    return np.ascontiguousarray(c)


def _quantile_baseline(base_times, base_cumhaz):
    """(ut, hz) of a quantile request, checked: the same size, no NaN, hz non-negative and non-decreasing."""
    ut, hz = _f64(base_times).reshape(-1), _f64(base_cumhaz).reshape(-1)
    if ut.size != hz.size:
        raise ValueError("base_times and base_cumhaz must have the same size, got %d and %d" % (ut.size, hz.size))
    if np.isnan(ut).any():
        raise ValueError("There is NAN value in base_times")
    if not (hz >= 0.0).all():
        raise ValueError("base_cumhaz should be non-negative")
    if (np.diff(hz) < 0.0).any():
        raise ValueError("base_cumhaz should be non-decreasing")
    return ut, hz


def _survtime_out(out, what, x, n, T):
    """(result, ptr, row stride, column stride, on_device) of an (n, T) output of cox_survival_times_device: out as in
    cox_survival_device."""
    if out is not None:
        if not is_device_array(out):
            raise ValueError("%s must be a device array" % what)
        do = _DeviceArray(out, what)
        if do.item != 8:
            raise ValueError("%s: a device array of float64 is needed (typestr '<f8')" % what)
        if do.shape != (n, T):
            raise ValueError("%s must have shape %s, got %s" % (what, (n, T), do.shape))
        return out, do.ptr, do.strides[0], do.strides[1], 1
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(x, torch.Tensor):
        result = torch.empty((n, T), dtype=torch.float64, device=x.device)
        return result, int(result.data_ptr()), T, 1, 1
    result = np.empty((n, T))
    return result, int(result.ctypes.data), T, 1, 0


def cox_survtime_workspace(n, cut):
    """What the RMST part of cox_survival_times_device needs for n rows and the cuts of rmst_segments
    (bessx_cox_survtime_workspace; no device): {"slab": the segments of a piece at most, "pieces", "rows_per_chunk",
    "doubles": the doubles of device scratch with device outputs}."""
    cut = _i32(np.asarray(cut).reshape(-1))
    slab, pieces, rows, doubles = _i(0), _i(0), _ll(0), _ll(0)
    _check(lib().bessx_cox_survtime_workspace(int(n), _ip(cut), cut.size, ctypes.byref(slab), ctypes.byref(pieces),
                                              ctypes.byref(rows), ctypes.byref(doubles)))
    return {"slab": slab.value, "pieces": pieces.value, "rows_per_chunk": rows.value, "doubles": doubles.value}


def cox_survival_times_device(x, cols, B, base_times, base_cumhaz, tau=None, q=None, hazard_levels=None, out_rmst=None,
                              out_quantile=None, stream=0):
    """One number per row and horizon / level from one Cox model, for the rows of a device matrix x (n x p: float64 or
    float32, any non-negative strides) read once where it lies, the support's columns only
    (bessx_cox_survtime_device).  No curve is stored.  With eta = x[:, cols] @ B, e = exp(clip(eta, -30, 30)), H0 the step
    function of baseline_at(base_times, base_cumhaz, .) and S(t | x_i) = exp(-(H0(t) * e_i)):
        tau (T,):  "rmst" (n, T), the restricted mean survival times integral_0^tau[j] S(t | x_i) dt, the finite sum
                   over the segments of rmst_segments(base_times, base_cumhaz, tau) (tau finite and >= 0, any order,
                   repeats allowed; tau = 0 gives exactly 0.0), in fp64 by additions only in a fixed order: the bits of a
                   row depend neither on n nor on where the row lies, and along ascending tau a row never decreases;
        q (Q,) in (0, 1), or hazard_levels (Q,) > 0 (one of the two):  "quantile" (n, Q), the first base time at which
                   base_cumhaz * e_i (one fp64 product) reaches the level c = -log1p(-q), that is at which
                   S(t | x_i) <= 1 - q; +inf when the curve never gets there (a baseline without an event included);
                   q = 0.5 is the median survival time.  (survival::survfit averages two times where S equals 1 - q
                   exactly; this does not.)
    At least one of tau, q and hazard_levels must be given; only the requested keys are returned.  A NaN in a support
    column of row i gives NaN in every output of row i and nowhere else.  base_times, base_cumhaz: what
    cox_baseline_device returned.  out_rmst / out_quantile: float64 device arrays of shape (n, T) / (n, Q) to write into,
    any strides; without them the results are torch tensors on x's device when x is a torch tensor (torch is looked up,
    never imported) and NumPy arrays for any other device object.  stream: raw handle of the stream x was produced on;
    the results are complete when the call returns."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    cols, B = _cox_model(dx, cols, B)
    want_q = q is not None or hazard_levels is not None
    if tau is None and not want_q:
        raise ValueError("nothing to compute: give tau, q or hazard_levels")
    parts = {}
    if tau is not None:
        hs, wd, cut = rmst_segments(base_times, base_cumhaz, tau)
        if not (hs >= 0.0).all():
            raise ValueError("base_cumhaz should be non-negative")
        parts["rmst"] = (hs, wd, cut) + _survtime_out(out_rmst, "out_rmst", x, n, cut.size)
    elif out_rmst is not None:
        raise ValueError("out_rmst goes with tau")
    if want_q:
        c = _hazard_levels(q, hazard_levels)
        ut, hz = _quantile_baseline(base_times, base_cumhaz)
        parts["quantile"] = (hz, ut, c) + _survtime_out(out_quantile, "out_quantile", x, n, c.size)
    elif out_quantile is not None:
        raise ValueError("out_quantile goes with q or hazard_levels")
    # one call serves both parts (one predictor pass) unless one result is device memory and the other a host array
    groups = [list(parts)] if len({v[-1] for v in parts.values()}) == 1 else [[k] for k in parts]
    for names in groups:
        a = CoxSurvtimeInput()
        _set_x(a, dx)
        a.cols, a.m, a.B = _ip(cols), cols.size, _dp(B)
        a.stream = int(stream) if stream else None
        rm_ptr = qu_ptr = None
        if "rmst" in names:
            hs, wd, cut, _, rm_ptr, a.rmst_row_stride, a.rmst_col_stride, a.out_on_device = parts["rmst"]
            a.hs, a.wd, a.K, a.cut, a.T = _dp(hs), _dp(wd), hs.size, _ip(cut), cut.size
        if "quantile" in names:
            hz, ut, c, _, qu_ptr, a.quant_row_stride, a.quant_col_stride, a.out_on_device = parts["quantile"]
            a.hz, a.ut, a.J, a.c, a.Q = _dp(hz), _dp(ut), hz.size, _dp(c), c.size
        _check(lib().bessx_cox_survtime_device(ctypes.byref(a), rm_ptr, qu_ptr))
    return {k: v[3] for k, v in parts.items()}


def op_cox_rmst_bench(x, cols, K=1000, T=100, J=1000, Q=5, repeats=20):
    """Milliseconds per launch of the device steps of cox_survival_times_device on the device matrix x for the support
    cols, device events, for K segments, T horizons, J base times and Q levels of the library's own: (predictor pass that
    stores exp(clip(eta)) in row order, k_cxr_partial over every chunk of rows, k_cxr_finish over every chunk,
    k_cxr_quantile)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    if min(int(K), int(T), int(J), int(Q)) < 1:
        raise ValueError("K, T, J and Q must be at least 1")
    ms = np.zeros(4)
    _check(lib().bessx_op_cox_rmst_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, int(K), int(T), int(J), int(Q), repeats, _dp(ms)))
    return tuple(float(v) for v in ms)


BAND_CONF = {"plain": 0, "log": 1, "log-log": 2}  # BESSX_BAND_PLAIN / _LOG / _LOGLOG
BAND_WHAT = ("estimate", "se", "lower", "upper")  # bits 1, 2, 4, 8 (BESSX_BAND_*), the order of the slabs


def normal_quantile(level):
    """z with P(|N(0, 1)| <= z) = level, on the host: the root of erfc(z / sqrt 2) = 1 - level by bisection on math.erfc
    (erfc is decreasing; the interval is halved until it holds no further double).  level must lie in (0, 1)."""
    import math
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie in (0, 1), got %r" % (level,))
    target, r2 = 1.0 - level, math.sqrt(2.0)
    lo, hi = 0.0, 40.0  # erfc(0) = 1 > target >= 2^-53 > erfc(40 / sqrt 2)
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            # the neighbouring doubles lo, hi bracket the root: the one whose erfc is nearer the target
            return lo if abs(math.erfc(lo / r2) - target) <= abs(math.erfc(hi / r2) - target) else hi
        if math.erfc(mid / r2) > target:
            lo = mid
        else:
            hi = mid


def _band_mask(what):
    """(bit mask, names in slab order) of an iterable of output names (or one name)."""
    if isinstance(what, str):
        what = (what,)
    what = tuple(what)
    for k in what:
        if k not in BAND_WHAT:
            raise ValueError("what must be drawn from %s, got %r" % (list(BAND_WHAT), k))
    if not what:
        raise ValueError("what is empty: nothing to compute")
    names = [k for k in BAND_WHAT if k in what]
    return sum(1 << BAND_WHAT.index(k) for k in names), names


def _band_kind(kind, conf_type):
    if kind not in SURV_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(SURV_KINDS), kind))
    if conf_type not in BAND_CONF:
        raise ValueError("conf_type must be one of %s, got %r" % (sorted(BAND_CONF), conf_type))
    if kind == "cumhaz" and conf_type == "log-log":
        raise ValueError("conf_type 'log-log' is defined for kind='survival', not for the cumulative hazard")


def _band_inputs(m, cumhaz, var0, drift, factor):
    """cumhaz (T,), var0 (T,), drift (T, m), factor (m, m) as contiguous float64 host arrays, checked."""
    cumhaz, var0 = _f64(cumhaz).reshape(-1), _f64(var0).reshape(-1)
    T = cumhaz.size
    if T < 1:
        raise ValueError("cumhaz is empty: no curve to compute")
    if var0.size != T:
        raise ValueError("cumhaz and var0 must have the same size, got %d and %d" % (T, var0.size))
    for what, v in (("cumhaz", cumhaz), ("var0", var0)):
        if not (np.isfinite(v).all() and (v >= 0.0).all()):
            raise ValueError("%s should be finite and non-negative" % what)
    drift = _f64(drift if drift is not None else np.zeros((T, 0)))
    if drift.shape != (T, m):
        raise ValueError("drift must have shape (%d, %d), got %s" % (T, m, drift.shape))
    if not np.isfinite(drift).all():
        raise ValueError("drift should be finite")
    factor = _f64(factor if factor is not None else np.zeros((0, 0)))
    if factor.shape != (m, m):
        raise ValueError("factor must have shape (%d, %d), got %s" % (m, m, factor.shape))
    if not np.isfinite(np.tril(factor)).all():
        raise ValueError("the lower triangle of factor should be finite (is the information positive definite?)")
    return cumhaz, var0, drift, factor


def cox_baseline_variance_device(x, cols, beta, time, status, times, weight=None, ties="breslow", stream=0):
    """What the variance of the curves of ONE Cox model needs from the rows it was fitted to, x a device matrix (n x p:
    float64 or float32, any non-negative strides) read where it lies (bessx_cox_hazard_var_device).  With the quantities
    of cox_information_device (positions k in time order, r(k), e, wd = w * status, S0_k, u_k = S1_k / S0_k) and K(t) the
    positions with time <= t, for every grid time t:
        cumhaz = sum_K wd_k / S0_k,     var0 = sum_K wd_k / S0_k^2,     drift = sum_K (wd_k / S0_k) u_k     (m values)
    times: T >= 1 values in any order, repeats allowed, a NaN is a ValueError; a time before the first gives exact zeros.
    weight: None = ones, else >= 0.  Returns {"times" (T,), "cumhaz" (T,), "var0" (T,), "drift" (T, m), "n_events"},
    NumPy arrays.  Under ties="breslow" cumhaz is baseline_at(cox_baseline_device(...), times) bit for bit.  Additions
    only, in a fixed order: the same call gives the same bits.  len(cols) + 1 <= 1024."""
    a = CoxHazardVarInput()
    n, p, cols, B, host = _cox_call(a, "cox_baseline_variance_device", x, cols, beta, time, status, weight, ties, stream)
    if weight is not None and not (host["weight"] >= 0.0).all():
        raise ValueError("weight should be non-negative")
    if np.ndim(times) > 1:
        raise ValueError("times must be 1-D")
    tg = _f64(times).reshape(-1)
    if tg.size < 1:
        raise ValueError("times is empty: no curve to compute")
    if np.isnan(tg).any():
        raise ValueError("There is NAN value in times")
    m, T = cols.size, tg.size
    a.times, a.T = _dp(tg), T
    cumhaz, var0, drift, ne = np.zeros(T), np.zeros(T), np.zeros((T, m)), _d(0)
    _check(lib().bessx_cox_hazard_var_device(ctypes.byref(a), _dp(cumhaz), _dp(var0), _dp(drift), max(m, 1),
                                             ctypes.byref(ne)))
    return {"times": tg.copy(), "cumhaz": cumhaz, "var0": var0, "drift": drift, "n_events": ne.value}


def cox_band_workspace(n, m, T, what=("estimate", "lower", "upper"), dtype=np.float64, row_stride=None, col_stride=1,
                       out_on_device=True):
    """(doubles of scratch memory, grid times per workgroup of the matrix-core kernel) of a cox_survival_band_device call
    on an n-row matrix of the given element type and strides (row_stride=None: dense row-major needs no number here,
    any value > 1 stands for it) with a support of m columns, T times and the outputs `what`
    (bessx_cox_band_workspace; no device is needed)."""
    mask, _ = _band_mask(what)
    nd, tc = _ll(0), _i(0)
    rs = 2 if row_stride is None else int(row_stride)
    _check(lib().bessx_cox_band_workspace(0 if np.dtype(dtype) == np.float64 else 1, rs, int(col_stride), int(n), int(m),
                                          int(T), mask, int(bool(out_on_device)), ctypes.byref(nd), ctypes.byref(tc)))
    return nd.value, tc.value


def cox_survival_band_device(x, cols, beta, cumhaz, var0, drift, factor, kind="survival", conf_type="log-log", level=0.95,
                             what=("estimate", "lower", "upper"), out=None, stream=0):
    """Curves of one Cox model with their standard errors and pointwise confidence bounds for the rows of a device
    matrix x (n x p: float64 or float32, any non-negative strides), read where it lies, the support's columns only
    (bessx_cox_band_device; Tsiatis 1981, survival::survfit's numbers for a Breslow baseline).  cumhaz, var0 (T,) and
    drift (T, m) are cox_baseline_variance_device's; factor (m, m) is info_factor's R for cox_information_device's info
    (inv(info) = R^T R).  With z = x[i, cols], e = exp(clip(z @ beta, -30, 30)), L = cumhaz * e, t = R z, p = R drift and
    z_c = normal_quantile(level):
        V = var0 + |p - cumhaz t|^2,   se_L = e sqrt(V),   r = z_c sqrt(V) / cumhaz
        kind="cumhaz":    estimate L, se se_L; plain: max(L - z_c se_L, 0), L + z_c se_L; log: L exp(-r), L exp(r)
        kind="survival":  estimate S = exp(-L), se S se_L; plain: S -+ z_c se clipped to [0, 1]; log: exp(-(L + z_c se_L)),
                          exp(-max(L - z_c se_L, 0)); log-log: exp(-L exp(r)), exp(-L exp(-r))
    Where cumhaz is 0 the se is 0 and the bounds are the estimate.  estimate has cox_survival_device's bits for the same
    baseline values.  what: a subset of ("estimate", "se", "lower", "upper").  Returns a dict from name to an (n, T) view
    of one (K, n, T) array, K = len(what), slabs in that order: out when given (a float64 device array of shape
    (K, n, T), any strides), else a torch tensor on x's device when x is a torch tensor (torch is looked up, never
    imported) and a NumPy array for any other device object.  The sum of squares is formed directly on the fp64 matrix
    cores' output, never by the expansion that cancels for columns that are not centred; no (n, m) or (n, T) temporary
    is made.  len(cols) + 1 <= 1024, T <= 65535.  stream: raw handle of the stream x was produced on."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    _band_kind(kind, conf_type)
    mask, names = _band_mask(what)
    zc = normal_quantile(level)
    if np.ndim(beta) > 1:
        raise ValueError("beta must be 1-D: cox_survival_band_device takes one model per call")
    cols, B = _cox_model(dx, cols, np.asarray(beta, dtype=np.float64).reshape(-1))
    if not np.isfinite(B).all():
        raise ValueError("beta must be finite")
    m = cols.size
    cumhaz, var0, drift, factor = _band_inputs(m, cumhaz, var0, drift, factor)
    T, K = cumhaz.size, len(names)
    if out is not None:
        if not is_device_array(out):
            raise ValueError("out must be a device array")
        cai = out.__cuda_array_interface__
        shape = tuple(int(v) for v in cai["shape"])
        if cai["typestr"] != "<f8":
            raise ValueError("out: a device array of float64 is needed (typestr '<f8')")
        if shape != (K, n, T):
            raise ValueError("out must have shape %s, got %s" % ((K, n, T), shape))
        st = cai.get("strides")
        st = (n * T, T, 1) if st is None else tuple(int(v) // 8 for v in st)
        if any(int(v) < 0 or int(v) % 8 for v in (cai.get("strides") or ())):
            raise ValueError("out: byte strides must be non-negative multiples of 8")
        ptr, on_device, result = int(cai["data"][0]), 1, out
    else:
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(x, torch.Tensor):
            result = torch.empty((K, n, T), dtype=torch.float64, device=x.device)
            ptr, on_device = int(result.data_ptr()), 1
        else:
            result = np.empty((K, n, T))
            ptr, on_device = int(result.ctypes.data), 0
        st = (n * T, T, 1)
    a = CoxBandInput()
    _set_x(a, dx)
    a.cols, a.m, a.beta = _ip(cols), m, _dp(B)
    a.cumhaz, a.var0, a.drift, a.drift_ld, a.T = _dp(cumhaz), _dp(var0), _dp(drift), max(m, 1), T
    a.factor, a.factor_ld = _dp(factor), max(m, 1)
    a.kind, a.conf_type, a.z_c, a.what = SURV_KINDS[kind], BAND_CONF[conf_type], zc, mask
    a.out_slab_stride, a.out_row_stride, a.out_col_stride, a.out_on_device = st[0], st[1], st[2], on_device
    a.stream = int(stream) if stream else None
    _check(lib().bessx_cox_band_device(ctypes.byref(a), ptr))
    return {k: result[s] for s, k in enumerate(names)}


def op_cox_band_bench(x, cols, T=100, what=("estimate", "lower", "upper"), repeats=20):
    """Milliseconds per launch of the two device steps of cox_survival_band_device on the device matrix x for the support
    cols, device events: (predictor pass that stores exp(clip(eta)) in row order, k_cbd_band writing the K = len(what)
    row-major (n, T) slabs with the survival / log-log epilogue)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    mask, _ = _band_mask(what)
    if int(T) < 1:
        raise ValueError("T must be at least 1")
    ms = np.zeros(2)
    _check(lib().bessx_op_cox_band_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, int(T), mask, repeats, _dp(ms)))
    return tuple(float(v) for v in ms)


def op_cox_surv_bench(x, cols, T=100, kind="survival", out_col_major=False, repeats=20):
    """Milliseconds per launch of the kernels behind cox_survival_device / cox_baseline_device on the device matrix x for
    the support cols, device events: (predictor pass that stores exp(clip(eta)) in row order, k_cxs_curves for an (n, T)
    result laid out row-major or column-major, the baseline's hazard terms + forward scan + gather)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    if kind not in SURV_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(SURV_KINDS), kind))
    if int(T) < 1:
        raise ValueError("T must be at least 1")
    ms = np.zeros(3)
    _check(lib().bessx_op_cox_surv_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                         _ip(cols), cols.size, int(T), SURV_KINDS[kind], int(bool(out_col_major)),
                                         repeats, _dp(ms)))
    return tuple(float(v) for v in ms)


def _km_steps(time, status, w, order=None):
    """The distinct times u (ascending) with, in fp64: cens_u / ev_u = the weight of the rows censored / with an event at u,
    after_u = the weight of the rows with a later time.  Sums in time order (np.cumsum).  order: the stable argsort of
    time, where the caller has it."""
    if order is None:
        order = np.argsort(time, kind="stable")
    t, d, w = time[order], status[order], w[order]
    new = np.ones(t.size, dtype=bool)
    new[1:] = t[1:] != t[:-1]
    starts = np.nonzero(new)[0]
    ev = np.add.reduceat(w * d, starts)
    cens = np.add.reduceat(w * (1.0 - d), starts)
    tail = np.concatenate([np.cumsum(w[::-1])[::-1], [0.0]])  # tail[k]: the weight from position k on
    return t[starts], cens, ev, tail[np.append(starts[1:], t.size)]


def _km_vectors(time, status, weight):
    time, status = _f64(time).reshape(-1), _f64(status).reshape(-1)
    n = time.size
    if n < 1 or status.size != n:
        raise ValueError("time and status must hold the same number (>= 1) of values")
    w = np.ones(n) if weight is None else _f64(weight).reshape(-1)
    if w.size != n:
        raise ValueError("time.size should be equal to weight.size")
    if np.isnan(time).any():
        raise ValueError("There is NAN value in time")
    if not np.isin(status, (0.0, 1.0)).all():
        raise ValueError("status should be 0 or 1")
    if not (w >= 0.0).all():
        raise ValueError("weight should be non-negative")
    return time, status, w


def censoring_km(time, status, weight=None):
    """The weighted Kaplan-Meier estimate G of the censoring distribution as a right-continuous step function: (times,
    G), the distinct times of the rows, ascending, and G at them; G = 1 before the first.  An event at a time leaves the
    risk set before a censoring at the same time: with d_u the weight of the rows censored at u and Y_u the weight of the
    rows with a later time plus d_u, G(t) = prod over u <= t of (1 - d_u / Y_u), each factor formed as (Y_u - d_u) / Y_u
    from the sum it is, without the subtraction.  Host arrays, fp64."""
    return _censoring_km(*_km_vectors(time, status, weight))


def _censoring_km(time, status, w, order=None):
    u, cens, _, after = _km_steps(time, status, w, order)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(cens > 0.0, after / (after + cens), 1.0)
    return u, np.cumprod(f)


def _step_at(u, G, t, left=False):
    """G(t) (left: G(t-)) of the right-continuous step function (u, G) that is 1 before u[0]."""
    idx = np.searchsorted(u, t, side="left" if left else "right")
    return np.concatenate([[1.0], G])[idx]


def ipcw_weights(time, status, times, weight=None, censoring="km"):
    """(row_a (n,), time_b (T,)) of the IPCW Brier score at the requested times.  censoring="km": a_i = status_i /
    G(time_i-) (0 where weight_i = 0 or status_i = 0) and b_j = 1 / G(times_j) with G = censoring_km of the same rows; a
    time with G(times_j) = 0 is a ValueError that names the largest admissible time.  censoring=None: a = status, b = 1
    (without censoring: the mean squared error of S against 1{time > t}).  censoring=(row_a, time_b): the caller's
    arrays, finite and >= 0, for example from a training set's G."""
    return _ipcw_weights(*_km_vectors(time, status, weight), times, censoring)


def _ipcw_weights(time, status, w, times, censoring, order=None):
    times = _f64(times).reshape(-1)
    if np.isnan(times).any():
        raise ValueError("There is NAN value in times")
    if censoring is None:
        return status.copy(), np.ones(times.size)
    if isinstance(censoring, str):
        if censoring != "km":
            raise ValueError("censoring must be 'km', None or a pair (row_a, time_b), got %r" % (censoring,))
        u, G = _censoring_km(time, status, w, order)
        Gt = _step_at(u, G, times)
        if (Gt <= 0.0).any():
            raise ValueError("the censoring estimate G reaches 0 at the last time %r: the largest admissible time is %r"
                             % (float(u[-1]), float(np.nextafter(u[-1], -np.inf))))
        a = np.where((status != 0.0) & (w > 0.0), 1.0, 0.0)
        a[a > 0.0] /= _step_at(u, G, time[a > 0.0], left=True)
        return a, 1.0 / Gt
    try:
        row_a, time_b = censoring
        row_a, time_b = _f64(row_a).reshape(-1), _f64(time_b).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("censoring must be 'km', None or a pair (row_a, time_b), got %r" % (censoring,)) from None
    if row_a.size != time.size or time_b.size != times.size:
        raise ValueError("censoring=(row_a, time_b) must hold n = %d and T = %d values, got %d and %d"
                         % (time.size, times.size, row_a.size, time_b.size))
    for what, v in (("row_a", row_a), ("time_b", time_b)):
        if not (np.isfinite(v) & (v >= 0.0)).all():
            raise ValueError("censoring: %s must be finite and non-negative" % what)
    return row_a, time_b


def _increasing(times):
    return times.size >= 2 and bool((np.diff(times) > 0.0).all())


def integrated_brier(times, bs):
    """The integrated Brier score: the trapezoid rule over the strictly increasing times (T >= 2), divided by
    times[-1] - times[0].  bs: (T,) or (T, R); returns a float or (R,)."""
    times, bs = _f64(times).reshape(-1), np.asarray(bs, dtype=np.float64)
    if times.size < 2:
        raise ValueError("the integrated Brier score needs at least 2 times, got %d" % times.size)
    if np.isnan(times).any():
        raise ValueError("There is NAN value in times")
    if not _increasing(times):
        raise ValueError("the integrated Brier score needs strictly increasing times")
    if bs.shape[0] != times.size or bs.ndim not in (1, 2):
        raise ValueError("bs must have shape (T,) or (T, R) with T = %d, got %s" % (times.size, bs.shape))
    dt = np.diff(times)
    area = np.sum((0.5 * dt).reshape((-1,) + (1,) * (bs.ndim - 1)) * (bs[1:] + bs[:-1]), axis=0)
    return area / (times[-1] - times[0])


def _km_survival(time, status, w, order=None):
    """The weighted Kaplan-Meier survival of the rows as a right-continuous step function (u, S): the distinct times,
    ascending, and S at them; S = 1 before the first.  Each factor is (Y_u - ev_u) / Y_u formed from the sums it is."""
    u, cens, ev, after = _km_steps(time, status, w, order)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(ev > 0.0, (after + cens) / (after + cens + ev), 1.0)
    return u, np.cumprod(f)


def brier_null(time, status, w, times, row_a, time_b, order=None):
    """(BS_null (T,), sum_w): the weighted Kaplan-Meier survival S^ of the rows put through the Brier formula,
    BS_null[j] = (S^(t_j)^2 sum_{time_i <= t_j} w_i a_i + (1 - S^(t_j))^2 b_j sum_{time_i > t_j} w_i) / W.  Host, fp64."""
    if order is None:
        order = np.argsort(time, kind="stable")
    S = _step_at(*_km_survival(time, status, w, order), times)
    ts = time[order]
    idx = np.searchsorted(ts, times, side="right")  # rows with time <= t_j
    cum_wa = np.concatenate([[0.0], np.cumsum((w * row_a)[order])])
    tail_w = np.concatenate([np.cumsum(w[order][::-1])[::-1], [0.0]])
    W = float(np.sum(w))
    return (S * S * cum_wa[idx] + (1.0 - S) ** 2 * time_b * tail_w[idx]) / W, W


def _brier_result(bs, times, time, status, w, row_a, time_b, order=None):
    """The dict of cox_brier_device / bess_base.brier_survival from bs (T, R): the null model, IPA and the integrals (NaN
    where the times are not at least 2 and strictly increasing)."""
    null, W = brier_null(time, status, w, times, row_a, time_b, order)
    with np.errstate(invalid="ignore", divide="ignore"):
        ipa = np.where(null[:, None] > 0.0, 1.0 - bs / null[:, None], np.nan)
    if _increasing(times):
        ibs, ibs_null = integrated_brier(times, bs), float(integrated_brier(times, null))
    else:
        ibs, ibs_null = np.full(bs.shape[1], np.nan), float("nan")
    return {"brier": bs, "null": null, "ipa": ipa, "ibs": ibs, "ibs_null": ibs_null, "row_a": row_a, "time_b": time_b,
            "sum_w": W}


def _brier_grid(hg, times, R):
    """(hg float64 (T, R), times float64 (T,)), checked."""
    if np.ndim(times) > 1:
        raise ValueError("times must be 1-D")
    times = _f64(times).reshape(-1)
    T = times.size
    if T < 1:
        raise ValueError("times is empty: no score to compute")
    if np.isnan(times).any():
        raise ValueError("There is NAN value in times")
    hg = np.asarray(hg, dtype=np.float64)
    if hg.ndim == 1 and R == 1:
        hg = hg.reshape(-1, 1)
    if hg.shape != (T, R):
        raise ValueError("hg must have shape (T, R) = (%d, %d), got %s" % (T, R, hg.shape))
    if not (hg >= 0.0).all():
        raise ValueError("hg should be non-negative")
    return hg, times


def cox_brier_workspace(n, T, R):
    """(doubles of device memory, rows per slab, slabs, row groups per workgroup) of a cox_brier_device call on n rows, T
    times and R models (bessx_cox_brier_workspace; needs no device).  Nothing in it is n x T."""
    d, rows, slabs, groups = _ll(0), _ll(0), _ll(0), _i(0)
    _check(lib().bessx_cox_brier_workspace(int(n), int(T), int(R), ctypes.byref(d), ctypes.byref(rows),
                                           ctypes.byref(slabs), ctypes.byref(groups)))
    return int(d.value), int(rows.value), int(slabs.value), int(groups.value)


def cox_brier_device(x, cols, B, hg, times, time, status, weight=None, censoring="km", stream=0):
    """The time-dependent Brier score of R Cox models under inverse-probability-of-censoring weights on a device matrix x
    (n x p: float64 or float32, any non-negative strides), read once where it lies, the support's columns only
    (bessx_cox_brier_device): with eta = x[:, cols] @ B (no intercept), e = exp(clip(eta, -30, 30)), z = hg[j, r] e_ir,
    S = exp(-z) and q = -expm1(-z),
        BS[j, r] = (1 / W) sum_i w_i (a_i S^2 if time_i <= times_j else b_j q^2),      W = sum_i w_i,
    in one fused reduction that never stores an n x T element.  hg: (T, R) (or (T,) for one model), the baseline
    cumulative hazard of every model at the times (baseline_at on what cox_baseline_device returned); time, status (0 or
    1), weight (None = ones, else >= 0): n values each, host or device arrays (device arrays are copied to the host).
    (a, b) = ipcw_weights(time, status, times, weight, censoring).  Returns {"brier": (T, R), "null": (T,) the Kaplan-Meier
    survival of the same rows put through the same formula, "ipa": (T, R) = 1 - brier / null (NaN where null is 0),
    "ibs": (R,) and "ibs_null": integrated_brier over the times (NaN unless they are at least 2 and strictly increasing),
    "row_a", "time_b", "sum_w"}.  Every sum has a fixed order: the same call gives the same bits."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    B = np.asarray(B, dtype=np.float64)
    R = B.shape[1] if B.ndim == 2 else 1
    cols, B, _ = _predict_model(dx, cols, B, np.zeros(R))
    hg, times = _brier_grid(hg, times, R)
    if not (isinstance(censoring, (str, tuple, list)) or censoring is None):
        raise ValueError("censoring must be 'km', None or a pair (row_a, time_b), got %r" % (censoring,))
    if isinstance(censoring, str) and censoring != "km":
        raise ValueError("censoring must be 'km', None or a pair (row_a, time_b), got %r" % (censoring,))

    class _Fields:
        pass

    host = _cox_data(_Fields(), time, status, weight, n, stream)
    w = host.get("weight")
    if w is not None and not (w >= 0.0).all():
        raise ValueError("weight should be non-negative")
    wv = np.ones(n) if w is None else w
    if not float(np.sum(wv)) > 0.0:
        raise ValueError("the weights sum to 0")
    order = np.argsort(host["time"], kind="stable")  # (once: the weights and the null model both walk the rows in it)
    row_a, time_b = _ipcw_weights(host["time"], host["status"], wv, times, censoring, order)
    row_a, time_b = np.ascontiguousarray(row_a), np.ascontiguousarray(time_b)
    hg_mt = np.ascontiguousarray(hg.T)  # model-major
    a = CoxBrierInput()
    _set_x(a, dx)
    a.cols, a.m, a.B, a.R = _ip(cols), cols.size, _dp(B), R
    a.hg, a.times, a.T = _dp(hg_mt), _dp(times), times.size
    a.time, a.row_a, a.time_b, a.weight = _dp(host["time"]), _dp(row_a), _dp(time_b), _dp(w)
    a.stream = int(stream) if stream else None
    bs, sum_w = np.zeros((times.size, R)), _d(0)
    _check(lib().bessx_cox_brier_device(ctypes.byref(a), _dp(bs), ctypes.byref(sum_w)))
    out = _brier_result(bs, times, host["time"], host["status"], wv, row_a, time_b, order)
    out["sum_w"] = sum_w.value
    return out


def cox_brier_candidates(result, x_train, time_train, status_train, x_val, time_val, status_val, times, weight_train=None,
                         weight_val=None, censoring="km", stream=0):
    """The train / validation split for the curves: for every candidate of a path, the Breslow baseline on the training
    rows (one cox_baseline_device call per candidate: that entry point takes one model), then ONE cox_brier_device call
    over the union of the supports on the validation rows.  times: at least 2, strictly increasing.  Returns (ibs (R,),
    best) with best the lowest index among the smallest integrated Brier scores (a NaN never wins)."""
    cols, B, _ = candidate_models(result)
    times = _f64(times).reshape(-1)
    if not _increasing(times):
        raise ValueError("the integrated Brier score needs at least 2 strictly increasing times")
    hg = np.zeros((times.size, B.shape[1]))
    for r in range(B.shape[1]):
        used = B[:, r] != 0.0
        base = cox_baseline_device(x_train, cols[used], B[used, r], time_train, status_train, weight=weight_train,
                                   stream=stream)
        hg[:, r] = baseline_at(base["times"], base["cumhaz"], times)
    ibs = cox_brier_device(x_val, cols, B, hg, times, time_val, status_val, weight=weight_val, censoring=censoring,
                           stream=stream)["ibs"]
    return ibs, int(np.argmin(np.where(np.isnan(ibs), np.inf, ibs)))


def op_cox_brier_bench(x, cols, R=1, T=100, repeats=20):
    """Milliseconds per launch of the kernels behind cox_brier_device on the device matrix x for the support cols, R
    models and T times, device events: (predictor pass that stores exp(clip(eta)) as R x n, the reduction kernel
    k_cxb_terms over n * T * R elements, the addition of its slabs)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    if int(T) < 1 or int(R) < 1:
        raise ValueError("T and R must be at least 1")
    ms = np.zeros(3)
    _check(lib().bessx_op_cox_brier_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                          _ip(cols), cols.size, int(R), int(T), repeats, _dp(ms)))
    return tuple(float(v) for v in ms)


PAIRAUC_T_MAX = 1024  # the most times of cox_auc_device (PAIRAUC_T_MAX of bessx_dev.h)


def cox_auc_workspace(n, T, R):
    """(an upper bound of the doubles of device memory, positions per tile, an upper bound of the tiles) of a
    cox_auc_device call on n rows, T times and R models (bessx_cox_auc_workspace; needs no device).  Nothing in it is
    n x T or n x n."""
    d, rows, tiles = _ll(0), _ll(0), _ll(0)
    _check(lib().bessx_cox_auc_workspace(int(n), int(T), int(R), ctypes.byref(d), ctypes.byref(rows),
                                         ctypes.byref(tiles)))
    return int(d.value), int(rows.value), int(tiles.value)


def _auc_times(times):
    """(times float64 (T,), the stable argsort of them), checked; None = no times."""
    if times is None:
        times = np.zeros(0)
    if np.ndim(times) > 1:
        raise ValueError("times must be 1-D")
    times = _f64(times).reshape(-1)
    if np.isnan(times).any():
        raise ValueError("There is NAN value in times")
    if times.size > PAIRAUC_T_MAX:
        raise ValueError("at most %d times per call, got %d" % (PAIRAUC_T_MAX, times.size))
    return times, np.argsort(times, kind="stable")


def _auc_row_a(time, status, w, censoring, order=None):
    """row_a (n,) of the AUC / Uno's C: censoring="km": status_i / G(time_i-) from these rows (ipcw_weights without the
    check of G at requested times: none is needed here); None: status; n values: the caller's; a pair (row_a, time_b) as
    the Brier score takes it: its row_a."""
    if censoring is None or isinstance(censoring, str):
        return _ipcw_weights(time, status, w, np.zeros(0), censoring, order)[0]
    bad = "censoring must be 'km', None, row_a (n values) or a pair (row_a, time_b), got %r" % (censoring,)
    if isinstance(censoring, (tuple, list)) and len(censoring) == 2 and np.ndim(censoring[0]) >= 1:
        censoring = censoring[0]
    try:
        row_a = _f64(censoring).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(bad) from None
    if row_a.size != time.size:
        raise ValueError("censoring: row_a must hold n = %d values, got %d" % (time.size, row_a.size))
    if not (np.isfinite(row_a) & (row_a >= 0.0)).all():
        raise ValueError("censoring: row_a must be finite and non-negative")
    return row_a


def _auc_tau(tau):
    """tau of Uno's C as a float (NaN = no truncation), checked."""
    if tau is None:
        return float("nan")
    tau = float(tau)
    if np.isnan(tau):
        raise ValueError("tau must not be NaN (None = no truncation)")
    return tau


def _pair_sums_host(eta, time, w, cw, times):
    """(greater, equal) (T, R) of the cumulative/dynamic AUC in fp64 NumPy: eta (n, R); cases time_i <= t_j carry cw_i,
    controls time_l > t_j carry w_l.  Per model one stable sort of eta, then per time one cumulative sum of the controls'
    weights in that order: the weight strictly below a row is the running sum at the start of its group of equal eta,
    the weight level with it the group's sum.  Sums of non-negative terms only, no subtraction; no n x T temporary."""
    n, R = eta.shape
    T = times.size
    g, e = np.zeros((T, R)), np.zeros((T, R))
    for r in range(R):
        oe = np.argsort(eta[:, r], kind="stable")
        es = eta[oe, r]
        new = np.ones(n, dtype=bool)
        new[1:] = es[1:] != es[:-1]
        starts = np.nonzero(new)[0]
        gid = np.cumsum(new) - 1
        ts, ws, cs = time[oe], w[oe], cw[oe]
        for j in range(T):
            case = ts <= times[j]
            v = np.where(case, 0.0, ws)
            below = np.concatenate([[0.0], np.cumsum(v)])[starts][gid]
            level = np.add.reduceat(v, starts)[gid]
            u = np.where(case, cs, 0.0)
            g[j, r], e[j, r] = np.sum(u * below), np.sum(u * level)
    return g, e


def _uno_sums_host(eta, time, w, cw2, order, block=512):
    """(concordant, tied (R,), comparable) of Uno's C in fp64 NumPy: the pairs status_k = 1 (cw2_k > 0 carries it),
    time_k < time_l, weight cw2_k w_l.  O(n^2 R) comparisons in blocks of `block` case rows against all rows: this is
    the route without a GPU, meant for modest n."""
    n, R = eta.shape
    ts, ws, c2 = time[order], w[order], cw2[order]
    tail = np.concatenate([np.cumsum(ws[::-1])[::-1], [0.0]])
    comparable = float(np.sum(c2 * tail[np.searchsorted(ts, ts, side="right")]))
    conc, tied = np.zeros(R), np.zeros(R)
    rows = np.nonzero(c2 > 0.0)[0]
    for r in range(R):
        es = eta[order, r]
        sc = st = 0.0
        for b0 in range(0, rows.size, block):
            k = rows[b0:b0 + block]
            later = ts[None, :] > ts[k, None]
            sc += float(np.sum(c2[k] * ((later & (es[k, None] > es[None, :])) @ ws)))
            st += float(np.sum(c2[k] * ((later & (es[k, None] == es[None, :])) @ ws)))
        conc[r], tied[r] = sc, st
    return conc, tied, comparable


def _case_control_sums(time, w, cw, times, order):
    """(cases (T,), controls (T,)): sum of cw over time <= t_j and of w over time > t_j, running sums in time order."""
    ts = time[order]
    idx = np.searchsorted(ts, times, side="right")
    return (np.concatenate([[0.0], np.cumsum(cw[order])])[idx],
            np.concatenate([np.cumsum(w[order][::-1])[::-1], [0.0]])[idx])


def _cox_auc_result(greater, equal, cases, controls, perm, times, time, status, w, row_a, uno, order=None):
    """The dict of cox_auc_device / bess_base.auc_survival from the sums at the SORTED times (rows j of greater, equal,
    cases, controls belong to times[perm[j]]) and uno = (concordant, tied, comparable): the quotients, the Kaplan-Meier
    drops and their mean, everything returned in the caller's order of times."""
    T, R = greater.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        den = cases * controls
        auc = np.where(den[:, None] > 0.0, (greater + 0.5 * equal) / den[:, None], np.nan)
    S = _step_at(*_km_survival(time, status, w, order), times[perm])
    drop = np.concatenate([[1.0], S])[:T] - S
    used = drop > 0.0
    if used.any():
        with np.errstate(invalid="ignore"):
            mean = np.sum(auc[used] * drop[used, None], axis=0) / np.sum(drop[used])
    else:
        mean = np.full(R, np.nan)
    back = np.empty(T, dtype=np.int64)
    back[perm] = np.arange(T)
    conc, tied, comp = uno
    comp = float(comp)
    return {"auc": auc[back], "greater": greater[back], "equal": equal[back], "cases": cases[back],
            "controls": controls[back], "km_drop": drop[back], "mean_auc": mean,
            "uno_c": (conc + 0.5 * tied) / comp if comp > 0.0 else np.full(R, np.nan), "uno_concordant": conc,
            "uno_tied": tied, "uno_comparable": comp, "row_a": row_a}


def _cox_auc_host(eta, times, time, status, w, censoring, tau):
    """cox_auc_device in fp64 NumPy from the linear predictors eta (n, R): bess_base.auc_survival for a NumPy X."""
    times, perm = _auc_times(times)
    tau = _auc_tau(tau)
    order = np.argsort(time, kind="stable")
    row_a = _auc_row_a(time, status, w, censoring, order)
    cw = w * row_a
    cw2 = np.where((status != 0.0) & ~(time >= tau), cw * row_a, 0.0)
    ts = times[perm]
    greater, equal = _pair_sums_host(eta, time, w, cw, ts)
    cases, controls = _case_control_sums(time, w, cw, ts, order)
    uno = _uno_sums_host(eta, time, w, cw2, order)
    return _cox_auc_result(greater, equal, cases, controls, perm, times, time, status, w, row_a, uno, order)


def cox_auc_device(x, cols, B, times, time, status, weight=None, censoring="km", tau=None, stream=0):
    """The censoring-robust rank measures of R Cox models on a device matrix x (n x p: float64 or float32, any
    non-negative strides), read once where it lies, the support's columns only (bessx_cox_auc_device).  With eta =
    x[:, cols] @ B (no intercept), w the weights (None = ones) and a = row_a, the inverse-probability-of-censoring
    weights of the rows (censoring="km": status_i / G(time_i-) with G = censoring_km of these rows; None: status; n
    values, or the pair (row_a, time_b) the Brier score takes: the caller's):
        cumulative/dynamic AUC at every t_j of times (any order, repeats allowed, at most 1024; None or empty: none):
            cases time_i <= t_j carry w_i a_i, controls time_l > t_j carry w_l,
            greater[j, r] = sum over cases and controls of w_i a_i w_l 1(eta_ir > eta_lr), equal[j, r]: 1(eta_ir = eta_lr),
            auc = (greater + equal / 2) / (cases * controls), NaN where there is no case or no control;
        mean_auc[r] = sum_j auc[j, r] d_j / sum_j d_j over the times in ascending order, d_j = S^(t_(j-1)) - S^(t_j) the
            drop of the weighted Kaplan-Meier survival of these rows (S^ = 1 before the first time), over the times with
            d_j > 0; NaN if one of those auc is NaN or no d_j is positive;
        Uno's C truncated at tau (None = not truncated): the pairs status_i = 1, time_i < time_l (strictly),
            time_i < tau carry w_i a_i^2 w_l; uno_c = (uno_concordant + uno_tied / 2) / uno_comparable, NaN without a pair.
    time, status (0 or 1), weight (>= 0): n values each, host or device arrays (device arrays are copied to the host).
    Returns {"auc", "greater", "equal": (T, R); "cases", "controls", "km_drop": (T,); "mean_auc", "uno_c",
    "uno_concordant", "uno_tied": (R,); "uno_comparable": float; "row_a": (n,)}, the time axis in the caller's order.
    One tiled pair kernel counts all of it in fp64 with no atomics and every sum in a fixed order: the same call gives the
    same bits; only T x R numbers cross the bus, nothing n x T is stored.  The work is O(n^2 R) comparisons."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    B = np.asarray(B, dtype=np.float64)
    R = B.shape[1] if B.ndim == 2 else 1
    cols, B, _ = _predict_model(dx, cols, B, np.zeros(R))
    times, perm = _auc_times(times)
    tau = _auc_tau(tau)
    if isinstance(censoring, str) and censoring != "km":
        raise ValueError("censoring must be 'km', None, row_a (n values) or a pair (row_a, time_b), got %r" % (censoring,))
    a = CoxAucInput()
    _set_x(a, dx)
    a.cols, a.m, a.B, a.R = _ip(cols), cols.size, _dp(B), R
    host = _cox_data(a, time, status, weight, n, stream)  # (alive until the call has returned)
    w = host.get("weight")
    if w is not None and not (w >= 0.0).all():
        raise ValueError("weight should be non-negative")
    wv = np.ones(n) if w is None else w
    order = np.argsort(host["time"], kind="stable")
    row_a = np.ascontiguousarray(_auc_row_a(host["time"], host["status"], wv, censoring, order))
    ts = np.ascontiguousarray(times[perm])
    T = ts.size
    a.times, a.T, a.row_a, a.tau, a.want_uno = _dp(ts), T, _dp(row_a), tau, 1
    a.stream = int(stream) if stream else None
    greater, equal, cases, controls = np.zeros((T, R)), np.zeros((T, R)), np.zeros(T), np.zeros(T)
    uno, comp = np.zeros((R, 3)), _d(0)
    _check(lib().bessx_cox_auc_device(ctypes.byref(a), _dp(greater), _dp(equal), _dp(cases), _dp(controls), _dp(uno),
                                      ctypes.byref(comp)))
    return _cox_auc_result(greater, equal, cases, controls, perm, times, host["time"], host["status"], wv, row_a,
                           (np.ascontiguousarray(uno[:, 0]), np.ascontiguousarray(uno[:, 1]), comp.value), order)


def _auc_y(y, n):
    """y of the ROC AUC as n float64 host values shared by the models, checked."""
    if np.ndim(y) > 1 and not (np.ndim(y) == 2 and np.shape(y)[1] == 1):
        raise ValueError("y must hold one value per row, shared by the models, got shape %s" % (np.shape(y),))
    y = _f64(y).reshape(-1)
    if y.size != n:
        raise ValueError("X.shape(0) should be equal to y.shape(0): %d rows, y has %d values" % (n, y.size))
    if np.isnan(y).any():
        raise ValueError("There is NAN value in y")
    return y


def _auc_weight(weight, n):
    if weight is None:
        return None
    w = _f64(weight).reshape(-1)
    if w.size != n:
        raise ValueError("X.shape(0) should be equal to weight.size")
    if not (np.isfinite(w) & (w >= 0.0)).all():
        raise ValueError("weight should be non-negative")
    return w


def _auc_result(greater, equal, pos, neg):
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = (greater + 0.5 * equal) / (pos * neg) if pos * neg > 0.0 else np.full(greater.shape, np.nan)
    return {"auc": auc, "greater": greater, "equal": equal, "pos_weight": float(pos), "neg_weight": float(neg)}


def _auc_host(eta, y, weight):
    """auc_device in fp64 NumPy from the linear predictors eta (n, R): bess_base.auc for a NumPy X."""
    n = eta.shape[0]
    y, w = _auc_y(y, n), _auc_weight(weight, n)
    w = np.ones(n) if w is None else w
    cls = np.where(y > 0.5, 0.0, 1.0)  # (the classes as times: the one cut lies at 0)
    cut = np.zeros(1)
    greater, equal = _pair_sums_host(eta, cls, w, w, cut)
    pos, neg = _case_control_sums(cls, w, w, cut, np.argsort(cls, kind="stable"))
    return _auc_result(greater[0], equal[0], pos[0], neg[0])


def auc_device(x, cols, B, y, weight=None, stream=0):
    """The ROC AUC of R logistic models on a device matrix x (n x p: float64 or float32, any non-negative strides), read
    once where it lies, the support's columns only (bessx_auc_device): with eta = x[:, cols] @ B (the intercept moves no
    rank and is not taken), cases y_i > 0.5 and controls y_l <= 0.5 (y: n values shared by the models, a host or device
    array; an (n, R) y is a ValueError), w the weights (None = ones, else >= 0):
        greater[r] = sum over cases and controls of w_i w_l 1(eta_ir > eta_lr), equal[r]: 1(eta_ir = eta_lr),
        auc = (greater + equal / 2) / (pos_weight * neg_weight), NaN when a class is empty.
    Returns {"auc", "greater", "equal": (R,); "pos_weight", "neg_weight": floats}.  The kernels of cox_auc_device with
    the rows cut once, between the classes: fp64, no atomics, the same call gives the same bits."""
    dx = _DeviceArray(x, "x", 2)
    n, p = dx.shape
    B = np.asarray(B, dtype=np.float64)
    R = B.shape[1] if B.ndim == 2 else 1
    cols, B, _ = _predict_model(dx, cols, B, np.zeros(R))
    if is_device_array(y):
        shape = _DeviceArray(y, "y").shape
        if len(shape) > 1 and not (len(shape) == 2 and shape[1] == 1):
            raise ValueError("y must hold one value per row, shared by the models, got shape %s" % (shape,))
        y = device_to_host(y, stream)
    if is_device_array(weight):
        weight = device_to_host(weight, stream)
    y, w = np.ascontiguousarray(_auc_y(y, n)), _auc_weight(weight, n)
    a = AucInput()
    _set_x(a, dx)
    a.cols, a.m, a.B, a.R, a.y, a.weight = _ip(cols), cols.size, _dp(B), R, _dp(y), _dp(w)
    a.stream = int(stream) if stream else None
    greater, equal, pos, neg = np.zeros(R), np.zeros(R), _d(0), _d(0)
    _check(lib().bessx_auc_device(ctypes.byref(a), _dp(greater), _dp(equal), ctypes.byref(pos), ctypes.byref(neg)))
    return _auc_result(greater, equal, pos.value, neg.value)


def _best_score(scores):
    """The lowest index of the largest score; a NaN never wins."""
    return int(np.argmax(np.where(np.isnan(scores), -np.inf, scores)))


def cox_auc_candidates(result, x, time, status, times=None, weight=None, censoring="km", tau=None, by="uno_c", stream=0):
    """The validation split by discrimination: Uno's C (by="uno_c") or the mean cumulative/dynamic AUC over `times`
    (by="mean_auc") of every candidate of a path on held-out rows x, time, status, in ONE cox_auc_device call over the
    union of the candidates' supports (their coef0 is ignored; no training-set baseline is needed).  Returns (scores (R,),
    best) with best the lowest index of the largest score (a NaN never wins)."""
    if by not in ("uno_c", "mean_auc"):
        raise ValueError("by must be 'uno_c' or 'mean_auc', got %r" % (by,))
    cols, B, _ = candidate_models(result)
    scores = cox_auc_device(x, cols, B, times, time, status, weight=weight, censoring=censoring, tau=tau,
                            stream=stream)[by]
    return scores, _best_score(scores)


def auc_candidates(result, x, y, weight=None, stream=0):
    """The validation split of a logistic path by ROC AUC: every candidate on held-out rows x, y in ONE auc_device call
    over the union of the candidates' supports (coef0 is taken from the path and ignored: it moves no rank).  Returns
    (auc (R,), best) with best the lowest index of the largest AUC (a NaN never wins)."""
    cols, B, _coef0 = candidate_models(result)
    scores = auc_device(x, cols, B, y, weight=weight, stream=stream)["auc"]
    return scores, _best_score(scores)


def op_pairauc_bench(x, cols, R=1, T=100, repeats=5):
    """Milliseconds per launch of the kernels behind cox_auc_device / auc_device on the device matrix x for the support
    cols, R models and T cuts, device events, and the pairs the AUC pair kernel compares per launch: ((predictor pass
    that stores eta in position order, the pair kernel in AUC mode, its two finish kernels, the pair kernel in Uno
    mode), pairs)."""
    dx = _DeviceArray(x, "x", 2)
    cols, _, _ = _predict_model(dx, cols)
    if int(T) < 1 or int(R) < 1:
        raise ValueError("T and R must be at least 1")
    ms, pairs = np.zeros(4), _d(0)
    _check(lib().bessx_op_pairauc_bench(dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], dx.shape[0], dx.shape[1],
                                        _ip(cols), cols.size, int(R), int(T), repeats, _dp(ms), ctypes.byref(pairs)))
    return tuple(float(v) for v in ms), float(pairs.value)


def op_chol_bench(m, repeats=200):
    us = _d(0)
    _check(lib().bessx_op_chol_bench(m, repeats, ctypes.byref(us)))
    return us.value


def op_topk_bench(length, k, variant=1, repeats=200):
    us = _d(0)
    _check(lib().bessx_op_topk_bench(length, k, variant, repeats, ctypes.byref(us)))
    return us.value


def op_xtv_multi_bench(n, p, nc, two=False, repeats=20):
    g, ms = _d(0), _d(0)
    _check(lib().bessx_op_xtv_multi_bench(n, p, nc, int(two), repeats, ctypes.byref(g), ctypes.byref(ms)))
    return g.value, ms.value


def op_xtv_bench(n, p, variant, repeats=20):
    g, ms = _d(0), _d(0)
    _check(lib().bessx_op_xtv_bench(n, p, variant, repeats, ctypes.byref(g), ctypes.byref(ms)))
    return g.value, ms.value
