"""Estimator classes with the reference's Python surface (names, keyword arguments, defaults,
error messages and result attributes of /root/reference python/bess/linear.py), implemented on
top of libbessx.so.  The argument marshalling that bess_base.fit performs before it calls
pywrap_bess (python/bess/linear.py:204-387) is restated here; all numerical work happens in
the HIP library through bess_amd.capi.pywrap_bess -- there is no NumPy solver in this file.
"""
import math
import sys

import numpy as np

from . import capi

_ALGORITHM_CODE = {"Pdas": 1, "GroupPdas": 2, "L0L2": 5}          # linear.py:144-152
_MODEL_CODE = {"Lm": 1, "Logistic": 2, "Poisson": 3, "Cox": 4}     # linear.py:154-164
_PATH_CODE = {"seq": 1, "pgs": 2}                                  # linear.py:166-190
_IC_CODE = {"aic": 1, "bic": 2, "gic": 3, "ebic": 4}               # linear.py:192-202
_DATA_TYPE = {"Lm": 1, "Logistic": 2, "Poisson": 2, "Cox": 3}      # linear.py:475,517,559,597


def _current_stream(a):
    """Raw handle of torch's current stream for a's device when a is a torch tensor (torch is looked up, never
    imported), else 0 (the null stream)."""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(a, torch.Tensor) and a.is_cuda:
        return int(torch.cuda.current_stream(a.device).cuda_stream)
    return 0


class bess_base:
    """Base estimator.  Parameters follow python/bess/linear.py:87-91:

    max_iter=20, exchange_num=0, is_warm_start=True, sequence=None, lambda_sequence=None, s_min=None,
    s_max=None, K_max=None, epsilon=0.0001, lambda_min=0, lambda_max=0, ic_type="ebic", is_cv=False, K=5,
    is_screening=False, screening_size=None, powell_path=1, always_select=[], tao=0.

    Attributes after fit(): beta, coef0, train_loss, ic.

    fit(X, y) also takes an X in GPU memory (a torch ROCm tensor, or anything with __cuda_array_interface__: float64
    or float32, any strides): the library reads it where it lies, on torch's current stream, and X never crosses the
    bus.  y and weight may be device arrays too (n values: they are copied to the host).  predict(X) takes such an X too: a kernel reads the support's
    columns of it in place, and the results are torch tensors on X's device when X is one (NumPy arrays otherwise).
    evaluate(X, y) / score(X, y) turn held-out data into loss, R^2, accuracy or deviance: for an X in GPU memory in one
    fused pass over the support's columns that brings back R numbers.
    linear_predictor(X) is X @ beta + coef0 for every family -- for Cox the risk score that predict() does not return --
    as NumPy for a NumPy X and on X's device for an X in GPU memory.  The Cox classes also have
    evaluate_survival(X, y, weight=None, ties="order"), with y = (time, status) as in fit: the partial log-likelihood of
    the fitted model on these rows (ties="order": the rows at or after a row in the stable time order are at risk, the
    quantity train_loss = -2 loglik reports; ties="breslow": every row with time >= the row's), deviance = -2 loglik,
    n_events, and Harrell's concordance from exact pair counts (comparable, concordant, discordant, tied_risk, c_index);
    concordance(X, y) is its c_index.  A device X is read once, in place, by capi.evaluate_cox_device.
    Predictions in time, Cox classes only: fit_baseline(X, y, weight=None) on the rows the model was fitted to sets
    baseline_times_ and baseline_cumhaz_ (the Breslow cumulative baseline hazard H0 at the distinct event times) and
    returns self; predict_survival(X, times=None, kind="survival") then gives the (n, T) matrix
    S(t | x) = exp(-H0(t) exp(eta)) (kind="cumhaz": H0(t) exp(eta)) at the times given (None: baseline_times_), H0 a
    right-continuous step function that is 0 before the first event.  For an X in GPU memory both read the support's
    columns in place (capi.cox_baseline_device / capi.cox_survival_device) and the curves are a tensor on X's device that
    is written once; a NumPy X is served in fp64 NumPy.  fit() does not call fit_baseline.
    predict_rmst(X, tau) and predict_quantile(X, q=0.5) give one number per row from those curves without storing them:
    the restricted mean survival time to each horizon tau (the integral of the step function S(t | x) over [0, tau]) and
    the q-quantile of the survival time (q = 0.5: the median; +inf where the curve stays above 1 - q).  For an X in GPU
    memory both are capi.cox_survival_times_device: one predictor pass, a sum over the steps, a binary search.
    brier_survival(X, y, times, weight=None, censoring="km") says how good those curves are on rows the model may not
    have seen: the time-dependent Brier score under inverse-probability-of-censoring weights, the Kaplan-Meier null
    model's, IPA = 1 - brier / null and the integrated scores.  For an X in GPU memory one fused reduction
    (capi.cox_brier_device) forms every term in registers: no curve is stored.
    auc_survival(X, y, times=None, weight=None, censoring="km", tau=None) (Cox) and auc(X, y, weight=None) (Logistic) say
    how well the model ranks such rows: the cumulative/dynamic AUC(t) with its Kaplan-Meier-weighted mean and Uno's C,
    and the ROC AUC.  For an X in GPU memory one tiled kernel counts the weighted pairs (capi.cox_auc_device /
    capi.auc_device); any other model type raises a ValueError that names it.
    inference(X, y, weight=None) is the coefficient table of the fitted model on these rows (Lm, Logistic, Poisson; None
    for Cox; a 2-D beta raises): coef (intercept first), se, z, p_value (two-sided normal), cov, score, dispersion, dof,
    cond, positive_definite and cols, from the unpenalised expected information sum_i v_i z_i z_i^T of the selected
    columns (capi.wald_table).  An X in GPU memory is read in place by capi.information_device -- the support's columns
    go through the fp64 matrix cores, no gathered copy is made and (m + 1)^2 + m + 3 numbers come back; a NumPy X is served
    in fp64 NumPy with the same definitions.  The table ignores that the columns were selected, and a model fitted with
    lambda > 0 reports score != 0: its se are those of the unpenalised problem at a point that is not its optimum.
    """

    def __init__(self, algorithm_type, model_type, path_type, max_iter=20, exchange_num=0, is_warm_start=True,
                 sequence=None, lambda_sequence=None, s_min=None, s_max=None, K_max=None, epsilon=0.0001,
                 lambda_min=0, lambda_max=0, ic_type="ebic", is_cv=False, K=5, is_screening=False,
                 screening_size=None, powell_path=1, always_select=[], tao=0.):
        self.algorithm_type, self.model_type, self.path_type = algorithm_type, model_type, path_type
        self.max_iter, self.exchange_num, self.is_warm_start = max_iter, exchange_num, is_warm_start
        self.sequence, self.lambda_sequence = sequence, lambda_sequence
        self.s_min, self.s_max, self.K_max, self.epsilon = s_min, s_max, K_max, epsilon
        self.lambda_min, self.lambda_max, self.n_lambda = lambda_min, lambda_max, 100
        self.ic_type, self.is_cv, self.K = ic_type, is_cv, K
        self.is_screening, self.screening_size, self.powell_path = is_screening, screening_size, powell_path
        self.always_select, self.tao = always_select, tao
        self.path_len = self.p = None
        self.data_type = _DATA_TYPE.get(model_type)
        self.beta = self.coef0 = self.train_loss = self.ic = None
        self._arg_check()

    def _arg_check(self):
        if self.algorithm_type not in _ALGORITHM_CODE:
            raise ValueError("algorithm_type should not be " + str(self.algorithm_type))
        if self.model_type not in _MODEL_CODE:
            raise ValueError("model_type should not be " + str(self.model_type))
        if self.path_type not in _PATH_CODE:
            raise ValueError("path_type should be \'seq\' or \'pgs\'")
        if self.ic_type not in _IC_CODE:
            raise ValueError("ic_type should be \"aic\", \"bic\", \"ebic\" or \"gic\"")
        self.algorithm_type_int = _ALGORITHM_CODE[self.algorithm_type]
        self.model_type_int = _MODEL_CODE[self.model_type]
        self.path_type_int = _PATH_CODE[self.path_type]
        self.ic_type_int = _IC_CODE[self.ic_type]

    @staticmethod
    def _group_starts(group, p):
        # python/bess/linear.py:238-253: first column of every (sorted) group label
        if group is None:
            raise ValueError("When you choose GroupPdas algorithm, the group information should be given")
        if len(group) != p:
            raise ValueError("The length of group should be equal to the number of variables")
        group = np.sort(np.asarray(group))
        return [int(np.argmax(group == g)) for g in sorted(set(group.tolist()))]

    def fit(self, X, y, is_weight=False, is_normal=True, weight=None, state=None, group=None):
        try:
            self._fit(X, y, is_weight, is_normal, weight, state, group)
        finally:
            self._Y_device = None  # (no reference to the caller's device array outlives the call)

    def _fit(self, X, y, is_weight, is_normal, weight, state, group):
        on_device = capi.is_device_array(X)
        self._stream, self._row_order, self._Y_device = (_current_stream(X) if on_device else 0), None, None
        if on_device:
            # X stays where it is: its NaN verdict comes from the ingest kernel's flag (capi raises the same message)
            n, p = capi._DeviceArray(X, "X", 2).shape
            if capi.is_device_array(y):
                if len(y.__cuda_array_interface__["shape"]) == 2 and self.model_type_int == 1:
                    self._Y_device = y
                y = capi.device_to_host(y, _current_stream(y))
            if weight is not None and capi.is_device_array(weight):
                weight = capi.device_to_host(weight, _current_stream(weight))
            y = np.asarray(y)
        else:
            X, y = np.asarray(X), np.asarray(y)
            if np.isnan(X).any():
                raise ValueError("There is NAN value in X")
            n, p = X.shape
        if np.isnan(y).any():
            raise ValueError("There is NAN value in y")
        self.p = p
        Y = None
        if self.model_type_int == 1 and y.ndim == 2 and y.shape[1] >= 2:
            # several responses against one design: every column is fitted (beta (p, R); coef0, train_loss, ic (R,))
            if y.shape[0] != n:
                raise ValueError("X.shape(0) should be equal to y.shape(0) (y has one column per response)")
            Y, y = y, y[:, 0]
        g_index = self._group_starts(group, p) if self.algorithm_type_int == 2 else range(p)
        if self.model_type_int == 4:
            # Cox: rows by ascending time, response becomes the status column (linear.py:257-263)
            order = y[:, 0].argsort()
            if on_device:
                self._row_order = order  # the ingest kernel reads the rows in this order: no sorted copy of X
            else:
                X = X[order]
            y = y[order][:, 1].reshape(-1)
        if n != y.size:
            raise ValueError("X.shape(0) should be equal to y.size")
        if is_weight:
            if weight is None:
                raise ValueError("When you choose is_weight is True, the parameter weight should be given")
            if n != np.asarray(weight).size:
                raise ValueError("X.shape(0) should be equal to weight.size")
        else:
            weight = np.ones(n)
        if state is None:
            state = np.ones(n)
        if self.path_type_int == 1:
            if self.sequence is None:
                self.sequence = [i + 1 for i in range(min(p, int(n / np.log(n))))]
            if self.lambda_sequence is None:
                self.lambda_sequence = [0]
            self.s_min = self.s_max = self.K_max = 0
            self.lambda_min = self.lambda_max = 0
            self.path_len = int(len(self.sequence))
        else:
            self.sequence, self.lambda_sequence = [1], [0]
            self.s_min = 1 if self.s_min is None else self.s_min
            self.s_max = p if self.s_max is None else self.s_max
            if self.K_max is None:
                self.K_max = int(math.log(p, 2 / (math.sqrt(5) - 1)))
            self.lambda_min = 0 if self.lambda_min is None else self.lambda_min
            self.lambda_max = 0 if self.lambda_max is None else self.lambda_max
            self.path_len = self.K_max + 2
        if self.is_screening:
            if self.screening_size:
                if self.screening_size < max(self.sequence):
                    raise ValueError("screening size should be more than max(sequence).")
            else:
                self.screening_size = max(p, int(n / np.log(n)))
        else:
            self.screening_size = 1
        # libbessx holds the k x k work space of a session in HBM for at most 16382 active columns
        # (include/bessx.h: bessx_problem.max_sparsity); the reference has no such bound (any T0 <= p)
        top = max(self.sequence) if self.path_type_int == 1 else self.s_max
        gsz = int(np.max(np.diff(list(g_index) + [p])))
        if min(p, top * gsz) > capi.MAX_SPARSITY:
            raise ValueError("bess_amd: sparsity levels up to %d active columns are supported, this path asks for %d "
                             "(shorten `sequence` / lower `s_max`)" % (capi.MAX_SPARSITY, min(p, top * gsz)))
        if Y is not None:
            self._fit_responses(X, Y, weight, is_normal, g_index, state, p, top, gsz)
            return
        result = capi.pywrap_bess(X, y, self.data_type, weight, is_normal, self.algorithm_type_int,
                                  self.model_type_int, self.max_iter, self.exchange_num, self.path_type_int,
                                  self.is_warm_start, self.ic_type_int, self.is_cv, self.K, g_index, state,
                                  self.sequence, self.lambda_sequence, self.s_min, self.s_max, self.K_max,
                                  self.epsilon, self.lambda_min, self.lambda_max, self.n_lambda, self.is_screening,
                                  self.screening_size, self.powell_path, self.always_select, self.tao, p, 1, 1, 1, 1,
                                  1, 1, p, row_order=self._row_order, stream=self._stream)
        self.beta, self.coef0, self.train_loss, self.ic = result[0], result[1], result[2], result[3]

    def _fit_responses(self, X, Y, weight, is_normal, g_index, state, p, top, gsz):
        """fit() of the Lm classes for a 2-D y: the sequential path without CV or screening runs every response on ONE
        session (capi.Session.sequential_path_multi: one design upload, one shared Gram column cache); everything else
        fits the columns one after another through pywrap_bess.  Same results as fitting each column alone."""
        R = Y.shape[1]
        beta, coef0, loss, ic = np.zeros((p, R)), np.zeros(R), np.zeros(R), np.zeros(R)
        if self.path_type_int == 1 and not self.is_cv and not self.is_screening:
            ses = capi.Session(X, Y[:, 0], weight=weight, data_type=self.data_type, is_normal=is_normal,
                               model_type=self.model_type_int, algorithm_type=self.algorithm_type_int,
                               max_iter=self.max_iter, is_warm_start=self.is_warm_start,
                               always_select=self.always_select, g_index=list(g_index),
                               max_sparsity=min(top * gsz, p, capi.MAX_SPARSITY), stream=self._stream)
            try:
                if self._Y_device is not None:
                    ses.set_responses(self._Y_device, stream=_current_stream(self._Y_device))
                else:
                    ses.set_responses(Y)
                res = ses.sequential_path_multi(self.sequence, self.lambda_sequence, self.ic_type_int)
            finally:
                ses.close()
            for r, o in enumerate(res):
                beta[:, r], coef0[r], loss[r], ic[r] = o["beta"], o["coef0"], o["train_loss"], o["ic"]
        else:
            for r in range(R):
                out = capi.pywrap_bess(X, np.ascontiguousarray(Y[:, r]), self.data_type, weight, is_normal,
                                       self.algorithm_type_int, self.model_type_int, self.max_iter, self.exchange_num,
                                       self.path_type_int, self.is_warm_start, self.ic_type_int, self.is_cv, self.K,
                                       g_index, state, self.sequence, self.lambda_sequence, self.s_min, self.s_max,
                                       self.K_max, self.epsilon, self.lambda_min, self.lambda_max, self.n_lambda,
                                       self.is_screening, self.screening_size, self.powell_path, self.always_select,
                                       self.tao, p, 1, 1, 1, 1, 1, 1, p, stream=self._stream)
                beta[:, r] = out[0]
                coef0[r], loss[r], ic[r] = (float(np.ravel(v)[0]) for v in out[1:4])
        self.beta, self.coef0, self.train_loss, self.ic = beta, coef0, loss, ic

    def _predict_device(self, X):
        """predict() for an X in GPU memory: only the support's columns of X are read, where they lie."""
        if capi._DeviceArray(X, "X", 2).shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        if self.model_type_int == 4:
            return None
        beta = np.asarray(self.beta, dtype=np.float64)
        multi = self.model_type_int == 1 and beta.ndim == 2  # (one column per response)
        cols = np.nonzero(beta.any(axis=1) if multi else beta)[0]  # the union of the supports
        coef0 = np.asarray(self.coef0, dtype=np.float64).reshape(-1)
        link = {1: "identity", 2: "logistic", 3: "poisson"}[self.model_type_int]
        res = capi.predict_device(X, cols, beta[cols], coef0, link=link, stream=_current_stream(X))
        if self.model_type_int == 2:
            return {"Y": res[1], "pr": res[0]}
        if self.model_type_int == 3:
            return {"lam": res}
        return res

    def predict(self, X):
        if capi.is_device_array(X):
            return self._predict_device(X)
        X = np.asarray(X)
        if X.shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        if self.model_type_int == 1 and np.ndim(self.beta) == 2:  # (one column per response)
            return np.dot(X, self.beta) + np.asarray(self.coef0)[None, :]
        eta = np.dot(X, self.beta) + np.ones(X.shape[0]) * self.coef0
        if self.model_type_int == 1:
            return eta
        if self.model_type_int == 2:
            label = np.zeros(eta.size)
            label[eta > 0] = 1
            e = np.exp(np.clip(eta, -25, 25))
            return {"Y": label, "pr": e / (e + 1)}
        if self.model_type_int == 3:
            return {"lam": np.exp(eta)}
        return None

    # ---- held-out evaluation ------------------------------------------------------------------------------------
    _LINK = {1: "identity", 2: "logistic", 3: "poisson"}

    def _model_arrays(self):
        """(beta, cols, coef0 (R,), multi): cols is the union of the supports, multi says that beta has a column per
        response (Lm fitted to a 2-D y)."""
        beta = np.asarray(self.beta, dtype=np.float64)
        multi = self.model_type_int == 1 and beta.ndim == 2
        cols = np.nonzero(beta.any(axis=1) if multi else beta)[0]
        return beta, cols, np.asarray(self.coef0, dtype=np.float64).reshape(-1), multi

    @staticmethod
    def _loss_host(link, eta, Y, w):
        """(L (R,), A (R,) or None) in fp64 NumPy, the formulas of bessx_eval_device: eta, Y (n, R) or Y (n, 1), w (n,)."""
        A = None
        if link == "identity":
            f = (Y - eta) ** 2
        elif link == "logistic":
            f = np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))) - Y * eta
            A = (w[:, None] * ((eta > 0) == (Y > 0.5))).sum(axis=0)
        else:
            f = np.exp(eta) - Y * eta
        return (w[:, None] * f).sum(axis=0), A

    def evaluate(self, X, y, weight=None):
        """How good the fitted model is on data it was not fitted to: a dict of numbers shaped like coef0.
        All families: loss = sum_i w_i f(eta_i, y_i) (f as in capi.evaluate_device) and n_eff = sum_i w_i.
        Lm: mse = loss / n_eff, r2 = 1 - loss / sum_i w_i (y_i - ybar_w)^2 (a 2-D y: per response).
        Logistic: deviance = 2 loss, accuracy = weighted share of rows with (eta > 0) == (y > 0.5).
        Poisson: deviance = 2 (loss + sum_i w_i (y_i log y_i - y_i)) with 0 log 0 = 0, d2 = 1 - deviance / null deviance.
        Cox: None.  An X in GPU memory is read in place on torch's current stream by one fused kernel pass over the
        support's columns, y and weight may be device arrays as well, and the kernel brings back R numbers (2 R for
        Logistic).  For Lm and Poisson the terms in y alone (ybar_w, the total sum of squares, y log y, the null
        deviance) are computed on the host, so a device y and weight are also copied to the host, n values each;
        Logistic copies neither.  A NumPy X is evaluated in fp64 NumPy with the same formulas."""
        on_device = capi.is_device_array(X)
        n, p = capi._DeviceArray(X, "X", 2).shape if on_device else np.asarray(X).shape
        if p != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        if self.model_type_int == 4:
            return None
        beta, cols, coef0, multi = self._model_arrays()
        R, link = coef0.size, self._LINK[self.model_type_int]
        # (every shape is checked before anything is copied: a bad call makes no device call)
        y_dev, w_dev = capi.is_device_array(y), weight is not None and capi.is_device_array(weight)
        if not y_dev:
            y = np.asarray(y, dtype=np.float64)
        yshape = capi._DeviceArray(y, "y").shape if y_dev else y.shape
        if len(yshape) not in (1, 2) or yshape[0] != n or (len(yshape) == 2 and yshape[1] not in (1, R)):
            raise ValueError("X.shape(0) should be equal to y.shape(0), and y needs 1 column or one per response: "
                             "%d rows, %d responses, y has shape %s" % (n, R, tuple(yshape)))
        if weight is not None:
            if not w_dev:
                weight = np.asarray(weight, dtype=np.float64).reshape(-1)
            if (capi._DeviceArray(weight, "weight").size if w_dev else weight.size) != n:
                raise ValueError("X.shape(0) should be equal to weight.size")
        # host copies only where the host uses them: the NumPy route, and the terms in y alone of Lm and Poisson
        Y = w = None
        if not on_device or link != "logistic":
            Y = (capi.device_to_host(y, _current_stream(y)) if y_dev else y).reshape(n, -1)
            if weight is None:
                w = np.ones(n)
            else:
                w = (capi.device_to_host(weight, _current_stream(weight)) if w_dev else weight).reshape(-1)
        if on_device:
            got = capi.evaluate_device(X, cols, beta[cols].reshape(cols.size, R), coef0, y, link=link, weight=weight,
                                       stream=_current_stream(X))
            L, A, sw = got["loss"], got.get("correct"), got["sum_w"]
        else:
            eta = np.dot(np.asarray(X, dtype=np.float64), beta.reshape(p, R)) + coef0[None, :]
            L, A = self._loss_host(link, eta, Y, w)
            sw = float(n) if weight is None else float(w.sum())
        out = {"loss": L, "n_eff": np.full(R, sw)}
        with np.errstate(divide="ignore", invalid="ignore"):
            if link == "identity":
                ybar = (w[:, None] * Y).sum(axis=0) / sw
                out["mse"] = L / sw
                out["r2"] = 1.0 - L / (w[:, None] * (Y - ybar[None, :]) ** 2).sum(axis=0)
            elif link == "logistic":
                out["deviance"] = 2.0 * L
                out["accuracy"] = A / sw
            else:
                ylogy = np.where(Y > 0, Y * np.log(np.where(Y > 0, Y, 1.0)), 0.0)
                ybar = (w[:, None] * Y).sum(axis=0) / sw
                out["deviance"] = 2.0 * (L + (w[:, None] * (ylogy - Y)).sum(axis=0))
                null = 2.0 * (w[:, None] * (ylogy - Y * np.log(ybar)[None, :] - (Y - ybar[None, :]))).sum(axis=0)
                out["d2"] = 1.0 - out["deviance"] / null
        if not multi:
            out = {k: float(v[0]) for k, v in out.items()}
        return out

    # ---- coefficient table ---------------------------------------------------------------------------------------
    @staticmethod
    def _information_host(link, Xs, beta, coef0, y, w):
        """information_device's quantities in fp64 NumPy: Xs (n, m) the support's columns, beta (m,), y (n,), w (n,)."""
        n = Xs.shape[0]
        eta = Xs @ beta + coef0
        if link == "identity":
            v, g, f = w.copy(), w * (y - eta), (y - eta) ** 2
        elif link == "logistic":
            t = np.exp(-np.abs(eta))
            p = np.where(eta >= 0, 1.0, t) / (1.0 + t)
            v, g = w * (t / ((1.0 + t) * (1.0 + t))), w * (y - p)
            f = np.maximum(eta, 0.0) + np.log1p(t) - y * eta
        else:
            e = np.exp(eta)
            v, g, f = w * e, w * (y - e), e - y * eta
        Z = np.column_stack([np.ones(n), Xs])
        info = Z.T @ (v[:, None] * Z)
        info = np.tril(info) + np.tril(info, -1).T  # (both triangles from the lower one, as the kernel writes them)
        return {"info": info, "score": Z.T @ g, "loss": float((w * f).sum()), "sum_w": float(w.sum())}

    @staticmethod
    def _labels_host(cluster):
        """Cluster labels as a host int64 vector (a device array is copied to the host)."""
        if capi.is_device_array(cluster):
            torch = sys.modules.get("torch")
            if torch is not None and isinstance(cluster, torch.Tensor):
                cluster = cluster.detach().cpu().numpy()
            elif hasattr(cluster, "get"):
                cluster = cluster.get()
            else:
                raise ValueError("cluster: a device array that is no torch tensor cannot be copied to the host here")
        return np.ascontiguousarray(np.asarray(cluster).reshape(-1), dtype=np.int64)

    @staticmethod
    def _cov_args(cov_type, cluster, n, allowed):
        """The checks of cov_type / cluster that inference() and inference_survival() share; no device call."""
        if cov_type != "model" and cov_type not in capi.COV_TYPES:
            raise ValueError("cov_type must be 'model' or one of %s, got %r" % (list(capi.COV_TYPES), cov_type))
        if cluster is not None:
            if cov_type == "model":
                raise ValueError("cluster needs a robust cov_type ('HC0' or 'HC1'), got cov_type='model'")
            capi.cluster_labels(cluster, n)  # (size and dtype)
        if cov_type != "model" and not allowed(cov_type, cluster is not None):
            raise ValueError("cov_type %r is not available %s cluster for this model"
                             % (cov_type, "with" if cluster is not None else "without"))

    @staticmethod
    def _meat_host(Y, labels):
        """sum_g s_g s_g^T (labels: host int64) or sum_i y_i y_i^T (labels None) for the rows y_i of Y (n, M); both
        triangles from the lower one.  Returns (meat, G or None)."""
        G = None
        if labels is not None:
            order = np.argsort(labels, kind="stable")
            ls = labels[order]
            starts = np.nonzero(np.concatenate([[True], ls[1:] != ls[:-1]]))[0]
            Y = np.add.reduceat(Y[order], starts, axis=0)
            G = int(starts.size)
        B = Y.T @ Y
        return np.tril(B) + np.tril(B, -1).T, G

    @classmethod
    def _sandwich_host(cls, link, Xs, beta, coef0, y, w, kind, R, labels):
        """sandwich_device's meat in fp64 NumPy with the same definitions: Xs (n, m) the support's columns, R the factor
        of info_factor (HC2 / HC3 only), labels host int64 or None.  Returns (meat, G or None)."""
        n, M = Xs.shape[0], Xs.shape[1] + 1
        eta = Xs @ beta + coef0
        if link == "identity":
            v, g = w.copy(), w * (y - eta)
        elif link == "logistic":
            t = np.exp(-np.abs(eta))
            p = np.where(eta >= 0, 1.0, t) / (1.0 + t)
            v, g = w * (t / ((1.0 + t) * (1.0 + t))), w * (y - p)
        else:
            e = np.exp(eta)
            v, g = w * e, w * (y - e)
        Z = np.column_stack([np.ones(n), Xs])
        u = g
        if kind in ("HC2", "HC3"):
            T = Z @ np.tril(R).T
            h = v * np.sum(T * T, axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                u = g / np.sqrt(1.0 - h) if kind == "HC2" else g / (1.0 - h)
        return cls._meat_host(u[:, None] * Z, labels)

    def inference(self, X, y, weight=None, cov_type="model", cluster=None):
        """Standard errors and Wald tests of the fitted model on the rows (X, y): capi.wald_table's dict -- coef
        (intercept first), se, z, p_value, cov, score, dispersion, dof, cond, positive_definite -- plus cols, the
        selected columns in the order of coef[1:].  The information is the unpenalised expected information
        sum_i v_i z_i z_i^T, z_i = (1, X[i, cols]), on the original scale of X (capi.information_device states v and the
        score weights g per family); for Lm cov = (loss / (n_eff - m - 1)) (Z^T W Z)^-1 and p_value is the normal
        approximation.  score = sum_i g_i z_i is 0 up to rounding at the unpenalised optimum of the support: a model
        fitted with lambda > 0 shows score != 0.  Selection is not corrected for.  An X in GPU memory is read in place on
        torch's current stream, the support's columns only, and y and weight may be device arrays too; a NumPy X is
        served in fp64 NumPy with the same definitions.  Cox: None.  A 2-D beta (Lm fitted to several responses) raises
        ValueError: one model per call.
        cov_type: "model" (the default: the model-based covariance above, dispersion * inv(info)) or "HC0", "HC1", "HC2",
        "HC3": the robust (Huber-White sandwich) covariance c * inv(info) B inv(info) of capi.sandwich_table -- B = sum_i
        u_i^2 z_i z_i^T with u_i = g_i (HC0, HC1), g_i / sqrt(1 - h_i) (HC2), g_i / (1 - h_i) (HC3), no dispersion factor
        -- and the dict gains cov_type, n_clusters, scale and meat.  cluster: n integer labels (host or device array, any
        values, any order) for the cluster-robust covariance B = sum_g s_g s_g^T, s_g = sum_{i in g} u_i z_i: "HC0" is CR0,
        "HC1" is CR1 with c = G / (G - 1) * (n - 1) / (n - M); with "HC2" / "HC3" or with "model" it raises ValueError.
        With weights g carries w, so B carries w^2 (the estimating-function convention), and a row or a cluster of weight
        0 counts in n and G.  An X in GPU memory takes capi.sandwich_device (after capi.information_device and
        capi.info_factor when the leverage is needed)."""
        on_device = capi.is_device_array(X)
        shape = capi._DeviceArray(X, "X", 2).shape if on_device else np.shape(X)
        if len(shape) != 2 or shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        n = shape[0]
        self._cov_args(cov_type, cluster, n, lambda k, cl: not (cl and k in ("HC2", "HC3")))
        if self.model_type_int == 4:
            return None
        beta, cols, coef0, multi = self._model_arrays()
        if multi:
            raise ValueError("inference() takes one model: this Lm was fitted to %d responses (a 2-D beta), which is "
                             "not supported" % beta.shape[1])
        link = self._LINK[self.model_type_int]
        y_dev, w_dev = capi.is_device_array(y), weight is not None and capi.is_device_array(weight)
        ysize = capi._DeviceArray(y, "y").size if y_dev else np.size(y)
        if ysize != n:
            raise ValueError("X.shape(0) should be equal to y.size")
        if weight is not None and (capi._DeviceArray(weight, "weight").size if w_dev else np.size(weight)) != n:
            raise ValueError("X.shape(0) should be equal to weight.size")
        if on_device:
            if not y_dev:
                y = np.asarray(y, dtype=np.float64).reshape(-1)
            st = _current_stream(X)
            if cov_type in ("model", "HC2", "HC3"):
                got = capi.information_device(X, cols, beta[cols], coef0[0], y, link=link, weight=weight, stream=st)
            if cov_type in ("HC2", "HC3"):
                R, pd = capi.info_factor(got["info"])
                if pd:
                    got = capi.sandwich_device(X, cols, beta[cols], coef0[0], y, link=link, weight=weight, kind=cov_type,
                                               factor=R, stream=st)
                else:
                    got.update(meat=np.full_like(got["info"], np.nan), n_clusters=None)
            elif cov_type != "model":
                got = capi.sandwich_device(X, cols, beta[cols], coef0[0], y, link=link, weight=weight, kind=cov_type,
                                           cluster=cluster, stream=st)
        else:
            yh = (capi.device_to_host(y, _current_stream(y)) if y_dev else np.asarray(y, dtype=np.float64)).reshape(-1)
            if weight is None:
                w = np.ones(n)
            else:
                w = (capi.device_to_host(weight, _current_stream(weight)) if w_dev
                     else np.asarray(weight, dtype=np.float64)).reshape(-1)
            Xs = np.asarray(X, dtype=np.float64)[:, cols]
            got = self._information_host(link, Xs, beta[cols], coef0[0], yh, w)
            if cov_type != "model":
                R, pd = capi.info_factor(got["info"]) if cov_type in ("HC2", "HC3") else (None, True)
                if pd:
                    labels = None if cluster is None else self._labels_host(cluster)
                    got["meat"], got["n_clusters"] = self._sandwich_host(link, Xs, beta[cols], coef0[0], yh, w, cov_type,
                                                                         R, labels)
                else:
                    got.update(meat=np.full_like(got["info"], np.nan), n_clusters=None)
        coef = np.concatenate([coef0[:1], beta[cols]])
        if cov_type == "model":
            out = capi.wald_table(got["info"], got["score"], coef, link, got["loss"], got["sum_w"])
        else:
            out = capi.sandwich_table(got["info"], got["meat"], got["score"], coef, cov_type, n, got["n_clusters"])
        out["cols"] = cols
        return out

    # ---- per-row diagnostics -------------------------------------------------------------------------------------
    @staticmethod
    def _diagnostics_host(link, Xs, beta, coef0, y, w, R, dispersion, kinds):
        """diagnostics_device's quantities in fp64 NumPy, the same definitions: Xs (n, m) the support's columns, beta
        (m,), y (n,), w (n,), R (M, M) lower triangular or None (no leverage kind).  T = Z R^T is formed column by
        column with elementwise operations over the rows, so a row's result does not depend on where the row lies."""
        n, M = Xs.shape[0], Xs.shape[1] + 1
        eta = np.zeros(n)
        for k in range(M - 1):
            eta = eta + Xs[:, k] * beta[k]
        eta = eta + coef0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            xlogx = lambda a: np.where(a == 0, 0.0, a * np.log(np.where(a == 0, 1.0, a)))  # noqa: E731
            if link == "identity":
                mu, V, d = eta, np.ones(n), (y - eta) * (y - eta)
            elif link == "logistic":
                t = np.exp(-np.abs(eta))
                s = 1.0 + t
                mu, V = np.where(eta >= 0, 1.0, t) / s, t / (s * s)
                f = (np.where(eta > 0, eta, 0.0) + np.log1p(t)) - y * eta
                d = 2.0 * ((f + xlogx(y)) + xlogx(1.0 - y))
            else:
                mu = np.exp(eta)
                V = mu
                d = 2.0 * (((mu - y * eta) + xlogx(y)) - y)
            r = y - mu
            out = {"response": r, "pearson": (np.sqrt(w) * r) / np.sqrt(V),
                   "deviance": np.sign(r) * np.sqrt(w * np.where(d < 0, 0.0, d))}
            if any(k in capi.DIAG_LEVERAGE_KINDS for k in kinds):
                Z = np.column_stack([np.ones(n), Xs])
                s2 = np.zeros(n)
                for j in range(M):
                    tj = np.zeros(n)
                    for k in range(j + 1):
                        tj = tj + R[j, k] * Z[:, k]
                    s2 = s2 + tj * tj
                h = (w * V) * s2
                om = 1.0 - h
                den = np.sqrt(dispersion * om)
                out.update(leverage=h, std_pearson=out["pearson"] / den, std_deviance=out["deviance"] / den,
                           cooks=((out["pearson"] * out["pearson"]) * h) / ((dispersion * M) * (om * om)))
        return {k: out[k] for k in capi.DIAG_KINDS if k in kinds}

    def diagnostics(self, X, y, weight=None, kinds=None):
        """Which rows drive the fit: a dict from kind name to an (n,) vector for the kinds asked for (None: all of
        capi.DIAG_KINDS -- leverage, response, pearson, deviance, std_pearson, std_deviance, cooks, as
        capi.diagnostics_device defines them), plus cols, dispersion and positive_definite.  The leverage is the diagonal
        of the hat matrix W^(1/2) Z (Z^T W Z)^-1 Z^T W^(1/2) with z_i = (1, X[i, cols]) and the working weights of
        inference(); the dispersion is inference()'s (loss / (n_eff - m - 1) for Lm, 1 otherwise).  An X in GPU memory is
        read in place on torch's current stream -- the information matrix by capi.information_device, its factor by
        capi.info_factor on the host, the rows by capi.diagnostics_device -- and the vectors are views of one tensor
        on X's device; y and weight may be device arrays too.  A NumPy X is served in fp64 NumPy with the same
        definitions.  When the information is not positive definite (or, for Lm, the dispersion is not positive) the
        kinds that need the leverage are filled with NaN, the three residuals are still computed and nothing is raised.
        Cox: None.  A 2-D beta (Lm fitted to several responses) raises ValueError: one model per call."""
        on_device = capi.is_device_array(X)
        shape = capi._DeviceArray(X, "X", 2).shape if on_device else np.shape(X)
        if len(shape) != 2 or shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        n = shape[0]
        if self.model_type_int == 4:
            return None
        beta, cols, coef0, multi = self._model_arrays()
        if multi:
            raise ValueError("diagnostics() takes one model: this Lm was fitted to %d responses (a 2-D beta), which is "
                             "not supported" % beta.shape[1])
        _, kinds = capi._diag_mask(capi.DIAG_KINDS if kinds is None else kinds)
        link = self._LINK[self.model_type_int]
        y_dev, w_dev = capi.is_device_array(y), weight is not None and capi.is_device_array(weight)
        ysize = capi._DeviceArray(y, "y").size if y_dev else np.size(y)
        if ysize != n:
            raise ValueError("X.shape(0) should be equal to y.size")
        if weight is not None and (capi._DeviceArray(weight, "weight").size if w_dev else np.size(weight)) != n:
            raise ValueError("X.shape(0) should be equal to weight.size")
        M = cols.size + 1
        lev = [k for k in kinds if k in capi.DIAG_LEVERAGE_KINDS]
        res = [k for k in kinds if k not in capi.DIAG_LEVERAGE_KINDS]
        if on_device:
            if not y_dev:
                y = np.asarray(y, dtype=np.float64).reshape(-1)
            st = _current_stream(X)
            got = capi.information_device(X, cols, beta[cols], coef0[0], y, link=link, weight=weight, stream=st)
        else:
            Xs = np.asarray(X, dtype=np.float64)[:, cols]
            yh = (capi.device_to_host(y, _current_stream(y)) if y_dev else np.asarray(y, dtype=np.float64)).reshape(-1)
            if weight is None:
                w = np.ones(n)
            else:
                w = (capi.device_to_host(weight, _current_stream(weight)) if w_dev
                     else np.asarray(weight, dtype=np.float64)).reshape(-1)
            got = self._information_host(link, Xs, beta[cols], coef0[0], yh, w)
        dof = float(got["sum_w"]) - M
        if link == "identity":
            dispersion = float(got["loss"]) / dof if dof > 0 else float("nan")
        else:
            dispersion = 1.0
        R, pd = capi.info_factor(got["info"])
        ok = pd and np.isfinite(dispersion) and dispersion > 0
        ask = kinds if ok else tuple(res)
        out = {}
        if ask:
            if on_device:
                out = capi.diagnostics_device(X, cols, beta[cols], coef0[0], y, factor=R if ok and lev else None,
                                              dispersion=dispersion if ok else 1.0, link=link, weight=weight, kinds=ask,
                                              stream=st)
            else:
                out = self._diagnostics_host(link, Xs, beta[cols], coef0[0], yh, w, R, dispersion, ask)
        if not ok:
            torch = sys.modules.get("torch")
            for k in lev:
                if on_device and torch is not None and isinstance(X, torch.Tensor):
                    out[k] = torch.full((n,), float("nan"), dtype=torch.float64, device=X.device)
                else:
                    out[k] = np.full(n, np.nan)
        out = {k: out[k] for k in kinds}
        out.update(cols=cols, dispersion=dispersion, positive_definite=bool(pd))
        return out

    # ---- score tests of the columns left out ---------------------------------------------------------------------
    @staticmethod
    def _score_tests_host(link, X, cols, beta, coef0, y, w, cand):
        """addscore_device's quantities in fp64 NumPy with the same definitions: X (n, p), cols the support, beta (m,),
        y (n,), w (n,), cand the candidate columns (int64) or None = all.  Matrix products over the n rows."""
        n, p = X.shape
        Xs = X[:, cols]
        eta = Xs @ beta + coef0
        if link == "identity":
            v, g, f = w.copy(), w * (y - eta), (y - eta) ** 2
        elif link == "logistic":
            t = np.exp(-np.abs(eta))
            pr = np.where(eta >= 0, 1.0, t) / (1.0 + t)
            v, g = w * (t / ((1.0 + t) * (1.0 + t))), w * (y - pr)
            f = np.maximum(eta, 0.0) + np.log1p(t) - y * eta
        else:
            e = np.exp(eta)
            v, g, f = w * e, w * (y - e), e - y * eta
        Z = np.column_stack([np.ones(n), Xs])
        P = v[:, None] * Z
        info = Z.T @ P
        info = np.tril(info) + np.tril(info, -1).T
        score = Z.T @ g
        columns = np.arange(p, dtype=np.int64) if cand is None else np.asarray(cand, dtype=np.int64)
        R, pd = capi.info_factor(info)
        q = columns.size
        u, d, C = np.empty(q), np.empty(q), np.empty((q, Z.shape[1]))
        for j0 in range(0, q, 2048):  # (in blocks: no X-sized temporary here either)
            XJ = X[:, columns[j0:j0 + 2048]]
            u[j0:j0 + 2048] = XJ.T @ g
            C[j0:j0 + 2048] = XJ.T @ P
            d[j0:j0 + 2048] = v @ (XJ * XJ)
        if pd:
            r = R.T @ (R @ score)
            T = C @ np.tril(R).T
            s, a = np.sum(T * T, axis=1), C @ r
        else:
            s, a = np.full(q, np.nan), np.full(q, np.nan)
        return {"columns": columns, "u": u, "d": d, "s": s, "a": a, "info": info, "score": score,
                "loss": float((w * f).sum()), "sum_w": float(w.sum()), "positive_definite": bool(pd),
                "support": np.asarray(cols, dtype=np.int64), "cross": C}

    def score_tests(self, X, y, weight=None, candidates=None):
        """Did the selection leave out a column that matters?  The Rao score test of every candidate column against the
        fitted model on the rows (X, y) -- R's add1(fit, scope, test = "Rao"); for Lm the F-to-enter statistic over the
        current model's residual variance -- without refitting anything: capi.score_test_table's dict -- columns, score
        (the adjusted score u - a), variance (d - s), statistic = score^2 / (dispersion * variance), p_value (chi-square,
        1 degree of freedom), in_model, dispersion -- plus cols, the model's support.  candidates: None = all p columns,
        else ascending distinct column numbers.  A candidate that is in the support has in_model = True and NaN for
        statistic and p_value; a candidate whose variance is not positive (a column that the support reproduces) has
        NaN as well.  The information and the dispersion are inference()'s.  An X in GPU memory is read in place on
        torch's current stream in one pass over the candidate columns on the fp64 matrix cores
        (capi.addscore_device), with no X-sized temporary, and y and weight may be device arrays too; a NumPy X is
        served in fp64 NumPy with the same definitions.  When the information is not positive definite statistic and
        p_value are NaN and nothing is raised.  Every column is tested on its own, one degree of freedom each: the test
        of a whole group of columns (a model fitted with group selection) is score_tests_groups.  Selection is not corrected
        for: the p-values are those of a test chosen before seeing the data.  Cox: None (score_tests_survival, which
        takes the (time, status) response and the tie rule, serves the Cox classes).  A 2-D beta (Lm fitted to several
        responses) raises ValueError."""
        on_device = capi.is_device_array(X)
        shape = capi._DeviceArray(X, "X", 2).shape if on_device else np.shape(X)
        if len(shape) != 2 or shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        n = shape[0]
        cand, _ = capi._candidates(candidates, self.p)
        if self.model_type_int == 4:
            return None
        beta, cols, coef0, multi = self._model_arrays()
        if multi:
            raise ValueError("score_tests() takes one model: this Lm was fitted to %d responses (a 2-D beta), which is "
                             "not supported" % beta.shape[1])
        link = self._LINK[self.model_type_int]
        y_dev, w_dev = capi.is_device_array(y), weight is not None and capi.is_device_array(weight)
        ysize = capi._DeviceArray(y, "y").size if y_dev else np.size(y)
        if ysize != n:
            raise ValueError("X.shape(0) should be equal to y.size")
        if weight is not None and (capi._DeviceArray(weight, "weight").size if w_dev else np.size(weight)) != n:
            raise ValueError("X.shape(0) should be equal to weight.size")
        if on_device:
            if not y_dev:
                y = np.asarray(y, dtype=np.float64).reshape(-1)
            got = capi.addscore_device(X, cols, beta[cols], coef0[0], y, link=link, weight=weight, candidates=cand,
                                       stream=_current_stream(X))
        else:
            yh = (capi.device_to_host(y, _current_stream(y)) if y_dev else np.asarray(y, dtype=np.float64)).reshape(-1)
            if weight is None:
                w = np.ones(n)
            else:
                w = (capi.device_to_host(weight, _current_stream(weight)) if w_dev
                     else np.asarray(weight, dtype=np.float64)).reshape(-1)
            got = self._score_tests_host(link, np.asarray(X, dtype=np.float64), cols, beta[cols], coef0[0], yh, w, cand)
        out = capi.score_test_table(got, link)
        out["cols"] = cols
        return out

    @staticmethod
    def _group_runs(group, p):
        """The start column of every run of equal labels in the length-p label vector fit() takes: labels must be
        non-decreasing, so that each group is one contiguous run."""
        g = np.asarray(group).reshape(-1)
        if g.size != p:
            raise ValueError("group should have one label per column of X (%d), got %d" % (p, g.size))
        if p > 1 and (np.diff(g) < 0).any():
            raise ValueError("group labels must be non-decreasing: every group is a contiguous run of columns")
        return np.concatenate([[0], np.flatnonzero(np.diff(g) != 0) + 1]).astype(np.int32)

    @staticmethod
    def _score_tests_groups_host(link, X, cols, beta, coef0, y, w, starts, groups):
        """groupscore_device's quantities in fp64 NumPy with the same definitions: X (n, p), cols the support, beta
        (m,), y (n,), w (n,), starts the groups' start columns, groups the tested group numbers or None = all.  Matrix
        products over the n rows; the tested columns go in blocks of at most 2 048 that hold whole groups."""
        n, p = X.shape
        Xs = X[:, cols]
        eta = Xs @ beta + coef0
        if link == "identity":
            v, g, f = w.copy(), w * (y - eta), (y - eta) ** 2
        elif link == "logistic":
            t = np.exp(-np.abs(eta))
            pr = np.where(eta >= 0, 1.0, t) / (1.0 + t)
            v, g = w * (t / ((1.0 + t) * (1.0 + t))), w * (y - pr)
            f = np.maximum(eta, 0.0) + np.log1p(t) - y * eta
        else:
            e = np.exp(eta)
            v, g, f = w * e, w * (y - e), e - y * eta
        Z = np.column_stack([np.ones(n), Xs])
        P = v[:, None] * Z
        info = Z.T @ P
        info = np.tril(info) + np.tril(info, -1).T
        score = Z.T @ g
        R, pd = capi.info_factor(info)
        lists = capi._group_columns(np.asarray(starts, dtype=np.int32), None if groups is None else
                                    np.asarray(groups, dtype=np.int32), p)
        if lists is None:
            raise ValueError("groups must be ascending distinct group numbers")
        tested, width, columns, goc = lists
        q, nt = columns.size, tested.size
        pos = np.concatenate([[0], np.cumsum(width)])
        offsets = np.concatenate([[0], np.cumsum(width * width)]).astype(np.int64)
        u, a = np.empty(q), np.full(q, np.nan)
        D, S = np.empty(int(offsets[-1])), np.full(int(offsets[-1]), np.nan)
        if pd:
            r, Rl = R.T @ (R @ score), np.tril(R)
        t0 = 0
        while t0 < nt:  # (a block: whole groups, at most 2 048 columns unless one group alone is wider)
            t1 = t0 + 1
            while t1 < nt and pos[t1 + 1] - pos[t0] <= 2048:
                t1 += 1
            j0 = int(pos[t0])
            XJ = X[:, columns[j0:int(pos[t1])]]
            u[j0:int(pos[t1])] = XJ.T @ g
            C = XJ.T @ P
            VX = v[:, None] * XJ
            if pd:
                a[j0:int(pos[t1])] = C @ r
                T = C @ Rl.T
            for t in range(t0, t1):
                k0, k1 = int(pos[t]) - j0, int(pos[t + 1]) - j0
                Dg = np.triu(XJ[:, k0:k1].T @ VX[:, k0:k1])
                D[offsets[t]:offsets[t + 1]] = (Dg + np.triu(Dg, 1).T).reshape(-1)
                if pd:
                    Sg = np.triu(T[k0:k1] @ T[k0:k1].T)
                    S[offsets[t]:offsets[t + 1]] = (Sg + np.triu(Sg, 1).T).reshape(-1)
            t0 = t1
        return {"columns": columns, "group_of_column": goc, "u": u, "a": a, "D": D, "S": S, "offsets": offsets,
                "info": info, "score": score, "loss": float((w * f).sum()), "sum_w": float(w.sum()),
                "positive_definite": bool(pd), "support": np.asarray(cols, dtype=np.int64)}

    def score_tests_groups(self, X, y, group, weight=None, groups=None):
        """Did the selection leave out a GROUP that matters?  The Rao score test of every group of columns -- a
        dummy-coded factor, a spline basis: the units fit(..., group=...) selects -- against the fitted model on the
        rows (X, y), d degrees of freedom for a group of d columns, without refitting anything:
        capi.group_score_test_table's dict -- group (the number of the group in the order of its columns), first_column,
        df, score (the adjusted score vector u - a of each group), statistic = score^T inverse(D - S) score / dispersion,
        p_value (chi-square, df degrees of freedom), in_model, dispersion -- plus cols, the model's support.  group: the
        length-p label vector fit() takes; labels must be non-decreasing, so that every group is a contiguous run of
        columns (ValueError otherwise).  groups: None = all groups, else ascending distinct group numbers (0 = the
        first run).  A group with a column in the support has in_model = True and NaN for statistic and p_value; a
        group whose D - S is not positive definite (one that the support, or the rest of the group, reproduces) has NaN
        as well.  The information and the dispersion are inference()'s.  An X in GPU memory is read in place on torch's
        current stream (capi.groupscore_device: a tested group may have at most 64 columns), with no X-sized temporary,
        and y and weight may be device arrays too; a NumPy X is served in fp64 NumPy with the same definitions.  When
        the information is not positive definite statistic and p_value are NaN and nothing is raised.  For Lm,
        statistic * dispersion is the drop in the residual sum of squares on adding the whole group.  Selection is not
        corrected for.  Cox: None (score_tests_groups_survival).  A 2-D beta (Lm fitted to several responses) raises ValueError."""
        on_device = capi.is_device_array(X)
        shape = capi._DeviceArray(X, "X", 2).shape if on_device else np.shape(X)
        if len(shape) != 2 or shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        n = shape[0]
        starts = self._group_runs(group, self.p)
        _, tg = capi._group_lists(starts, groups, self.p)
        if tg is not None and (tg.min() < 0 or tg.max() >= starts.size or (np.diff(tg) <= 0).any()):
            raise ValueError("groups must be ascending distinct group numbers (0 .. %d)" % (starts.size - 1))
        if self.model_type_int == 4:
            return None
        beta, cols, coef0, multi = self._model_arrays()
        if multi:
            raise ValueError("score_tests_groups() takes one model: this Lm was fitted to %d responses (a 2-D beta), "
                             "which is not supported" % beta.shape[1])
        link = self._LINK[self.model_type_int]
        y_dev, w_dev = capi.is_device_array(y), weight is not None and capi.is_device_array(weight)
        ysize = capi._DeviceArray(y, "y").size if y_dev else np.size(y)
        if ysize != n:
            raise ValueError("X.shape(0) should be equal to y.size")
        if weight is not None and (capi._DeviceArray(weight, "weight").size if w_dev else np.size(weight)) != n:
            raise ValueError("X.shape(0) should be equal to weight.size")
        if on_device:
            if not y_dev:
                y = np.asarray(y, dtype=np.float64).reshape(-1)
            got = capi.groupscore_device(X, cols, beta[cols], coef0[0], y, starts, groups=tg, link=link, weight=weight,
                                         stream=_current_stream(X))
        else:
            yh = (capi.device_to_host(y, _current_stream(y)) if y_dev else np.asarray(y, dtype=np.float64)).reshape(-1)
            if weight is None:
                w = np.ones(n)
            else:
                w = (capi.device_to_host(weight, _current_stream(weight)) if w_dev
                     else np.asarray(weight, dtype=np.float64)).reshape(-1)
            got = self._score_tests_groups_host(link, np.asarray(X, dtype=np.float64), cols, beta[cols], coef0[0], yh, w,
                                                starts, tg)
        out = capi.group_score_test_table(got, link)
        out["cols"] = cols
        return out

    def score(self, X, y, weight=None):
        """r2 (Lm), accuracy (Logistic) or d2 (Poisson) of evaluate(X, y, weight); None for Cox."""
        res = self.evaluate(X, y, weight)
        return None if res is None else res[{1: "r2", 2: "accuracy", 3: "d2"}[self.model_type_int]]

    # ---- Cox: risk score, held-out partial likelihood, concordance -------------------------------------------------
    def linear_predictor(self, X):
        """X @ beta + coef0 (a 2-D beta of Lm: one column per response).  A NumPy X gives NumPy; an X in GPU memory is
        read in place, the support's columns only, and gives a tensor on X's device (capi.predict_device, identity
        link)."""
        if capi.is_device_array(X):
            if capi._DeviceArray(X, "X", 2).shape[1] != self.p:
                raise ValueError("X.shape[1] should be " + str(self.p))
            beta, cols, coef0, _ = self._model_arrays()
            return capi.predict_device(X, cols, beta[cols], coef0, link="identity", stream=_current_stream(X))
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        return X @ self.beta + self.coef0

    @staticmethod
    def _survival_host(eta, time, status, w, ties, pairs=True):
        """(loglik, comparable, concordant, discordant) in fp64 NumPy with the definitions of capi.evaluate_cox_device:
        eta, time, status, w are n-vectors in row order.  pairs=False leaves the O(n^2) counts out (three zeros)."""
        n = eta.size
        order = np.argsort(time, kind="stable")
        eta, t, d = eta[order], time[order], status[order]
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))  # (comparisons: a NaN stays a NaN)
        S = np.cumsum(np.exp(a)[::-1])[::-1]
        if ties == "breslow":
            S = S[first]
        loglik = float(np.sum((w[order] * d) * (a - np.log(S))))
        kg = np.where(d != 0, first, np.iinfo(np.int64).max)
        comparable = concordant = discordant = 0
        for k0 in range(0, n if pairs else 0, 512):  # (k, l) is comparable when first[l] > kg[k]: l > k follows from it
            cmp = first[None, k0:] > kg[k0:k0 + 512, None]
            ek, el = eta[k0:k0 + 512, None], eta[None, k0:]
            comparable += int(cmp.sum())
            concordant += int((cmp & (ek > el)).sum())
            discordant += int((cmp & (ek < el)).sum())
        return loglik, comparable, concordant, discordant

    def _survival_x(self, X):
        """(on_device, n) of an X for the Cox methods, NumPy or in GPU memory; raises the message of predict()."""
        on_device = capi.is_device_array(X)
        shape = tuple(capi._DeviceArray(X, "X", 2).shape if on_device else np.asarray(X).shape)
        if len(shape) != 2 or shape[1] != self.p:
            raise ValueError("X.shape[1] should be " + str(self.p))
        return on_device, shape[0]

    def _survival_data(self, X, y, weight):
        """(on_device, n, time, status, w, weight) for the Cox methods: y (n, 2) and weight (n values or None) as host
        arrays -- device arrays are copied once every shape has been checked -- w = ones without weights."""
        on_device, n = self._survival_x(X)
        y_dev, w_dev = capi.is_device_array(y), weight is not None and capi.is_device_array(weight)
        if not y_dev:
            y = np.asarray(y, dtype=np.float64)
        yshape = capi._DeviceArray(y, "y").shape if y_dev else y.shape
        if tuple(yshape) != (n, 2):
            raise ValueError("y should have shape (X.shape(0), 2) = (%d, 2): time and status, got %s"
                             % (n, tuple(yshape)))
        if weight is not None:
            if not w_dev:
                weight = np.asarray(weight, dtype=np.float64).reshape(-1)
            if (capi._DeviceArray(weight, "weight").size if w_dev else weight.size) != n:
                raise ValueError("X.shape(0) should be equal to weight.size")
        if y_dev:
            y = capi.device_to_host(y, _current_stream(y))
        w = np.ones(n) if weight is None else (
            capi.device_to_host(weight, _current_stream(weight)).reshape(-1) if w_dev else weight)
        time, status = np.ascontiguousarray(y[:, 0]), np.ascontiguousarray(y[:, 1])
        if np.isnan(time).any():
            raise ValueError("There is NAN value in y")
        if not np.isin(status, (0.0, 1.0)).all():
            raise ValueError("status (y[:, 1]) should be 0 or 1")
        return on_device, n, time, status, w, weight

    def evaluate_survival(self, X, y, weight=None, ties="order"):
        """Cox only: the fitted model on rows it may not have seen.  y: (n, 2) time and status (0 or 1) as in fit;
        weight: n values or None.  Returns plain floats and ints: loglik, deviance = -2 loglik, n_events = sum w status,
        comparable, concordant, discordant, tied_risk, c_index (NaN without a comparable pair); the definitions are those
        of capi.evaluate_cox_device, which serves an X in GPU memory in one call on torch's current stream (y and weight
        may be device arrays: n values each are copied to the host).  A NumPy X is evaluated in fp64 NumPy."""
        if self.model_type_int != 4:
            raise ValueError("evaluate_survival is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.evaluate_cox_device(X, cols, beta[cols], time, status, weight=None if weight is None else w,
                                           ties=ties, stream=_current_stream(X))
            loglik, comparable = float(got["loglik"][0]), got["comparable"]
            concordant, discordant = int(got["concordant"][0]), int(got["discordant"][0])
        else:
            X = np.asarray(X, dtype=np.float64)
            eta = np.zeros(n)
            for j in cols:  # (column by column: a row's sum does not depend on where the row lies)
                eta += X[:, j] * beta[j]
            loglik, comparable, concordant, discordant = self._survival_host(eta, time, status, w, ties)
        tied = comparable - concordant - discordant
        return {"loglik": loglik, "deviance": -2.0 * loglik, "n_events": float(np.sum(w * status)),
                "comparable": comparable, "concordant": concordant, "discordant": discordant, "tied_risk": tied,
                "c_index": float(capi.c_index(concordant, tied, comparable))}

    def concordance(self, X, y):
        """Harrell's c_index of evaluate_survival(X, y) (Cox only)."""
        if self.model_type_int != 4:
            raise ValueError("concordance is for the Cox classes, this is a %s model" % self.model_type)
        return self.evaluate_survival(X, y)["c_index"]

    # ---- Cox: coefficient table -------------------------------------------------------------------------------------
    @staticmethod
    def _cox_information_host(Xs, beta, time, status, w, ties):
        """cox_information_device's quantities in fp64 NumPy, by the same decomposition (running sums, not the O(n^2)
        definition): Xs (n, m) the support's columns, beta (m,), time, status, w (n,) in row order."""
        n, m = Xs.shape
        eta = np.zeros(n)
        for c in range(m):  # (column by column: a row's sum does not depend on where the row lies)
            eta += Xs[:, c] * beta[c]
        order = np.argsort(time, kind="stable")
        x, eta, t, d = Xs[order], eta[order], time[order], status[order]
        wd = w[order] * d
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        starts = np.nonzero(new)[0]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        last = np.append(starts[1:] - 1, n - 1)[np.cumsum(new) - 1]
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))  # (comparisons: a NaN stays a NaN)
        e = np.exp(a)
        r = first if ties == "breslow" else np.arange(n)
        S0 = np.cumsum(e[::-1])[::-1][r]
        loglik = float(np.sum(wd * (a - np.log(S0))))
        H = np.cumsum(wd / S0)
        if ties == "breslow":
            H = H[last]
        v = e * H
        g = wd - v
        S1 = np.cumsum((e[:, None] * x)[::-1], axis=0)[::-1]
        ev = d != 0
        U = S1[r[ev]] / S0[ev][:, None]
        info = x.T @ (v[:, None] * x) - U.T @ (wd[ev][:, None] * U)
        info = np.tril(info) + np.tril(info, -1).T  # (both triangles from the lower one, as the kernel writes them)
        return {"info": info, "score": x.T @ g, "loglik": loglik, "n_events": float(np.sum(wd)),
                "residual_sum": float(np.sum(g)) if m > 0 else 0.0}

    @classmethod
    def _cox_sandwich_host(cls, L, labels):
        """The Lin-Wei meat from the score residuals L (n, m) in fp64 NumPy: sum_k L_k L_k^T, or sum_g s_g s_g^T with
        s_g = sum_{k in g} L_k (labels: host int64).  Returns (meat, G or None)."""
        return cls._meat_host(np.asarray(L, dtype=np.float64), labels)

    def inference_survival(self, X, y, weight=None, ties="order", cov_type="model", cluster=None):
        """Cox only: standard errors and Wald tests of the fitted model on the rows (X, y) -- capi.cox_wald_table's dict
        (coef, se, z, p_value, cov, score, dispersion = 1, dof = n_events - m, cond, positive_definite; no intercept) plus
        cols, the selected columns in the order of coef, loglik and residual_sum.  y: (n, 2) time and status as in fit;
        weight: n values or None; ties: "order" (the risk sets of the fit) or "breslow".  The information is the observed
        information of the partial likelihood, sum_k w_k status_k Var_k(x) with Var_k the e-weighted covariance of the
        support's columns over the risk set of k, on the original scale of X (capi.cox_information_device states it; where
        a linear predictor is clipped at +-30 it is that formula, not a derivative).  It is formed as a difference of two
        Gram matrices, so columns far from centred lose digits; score = sum_k w_k status_k (x_k - u_k) is 0 up to rounding
        at the unpenalised optimum of the support, and residual_sum, the sum of the martingale residuals, is 0 up to
        rounding always.  Selection is not corrected for.  An X in GPU memory is read in place on torch's current stream,
        the support's columns only (y and weight may be device arrays: n values each are copied to the host); a NumPy X is
        served in fp64 NumPy with the same decomposition.  inference() stays None for the Cox classes.
        cov_type: "model" (the default, inv(info)) or the Lin-Wei robust covariance c * inv(info) B inv(info) of
        capi.cox_sandwich_table, with L the score residuals of capi.cox_diagnostics_device (they carry the weights):
        "HC0": B = sum_k L_k L_k^T, or with cluster (n integer labels, host or device) B = sum_g s_g s_g^T, s_g = sum_{k
        in g} L_k, c = 1; "HC1" with cluster: c = G / (G - 1).  "HC1" without cluster, "HC2", "HC3" and cluster with
        "model" raise ValueError.  The dict then gains cov_type, n_clusters, scale and meat, and dof stays n_events - m.
        An X in GPU memory takes capi.cox_information_device, capi.cox_diagnostics_device(kinds=("score",)) and
        capi.meat_device on L where it lies."""
        if self.model_type_int != 4:
            raise ValueError("inference_survival is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        self._cov_args(cov_type, cluster, self._survival_x(X)[1], lambda k, cl: k == "HC0" or (k == "HC1" and cl))
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        m = cols.size
        wt = None if weight is None else w
        if on_device:
            st = _current_stream(X)
            got = capi.cox_information_device(X, cols, beta[cols], time, status, weight=wt, ties=ties, stream=st)
        else:
            Xs = np.asarray(X, dtype=np.float64)[:, cols]
            got = self._cox_information_host(Xs, beta[cols], time, status, w, ties)
        if cov_type != "model":
            meat, G, L = np.zeros((0, 0)), None, None
            if m > 0 and on_device:
                L = capi.cox_diagnostics_device(X, cols, beta[cols], time, status, weight=wt, ties=ties,
                                                kinds=("score",), stream=st)["score"]
                if capi.is_device_array(L):
                    got_m = capi.meat_device(L, np.arange(m), cluster=cluster, intercept=False, stream=st)
                    meat, G, L = got_m["meat"], got_m["n_clusters"], None
            elif m > 0:
                L = self._cox_diagnostics_host(Xs, beta[cols], time, status, w, ties, None, None, ("score",))["score"]
            if L is not None or (m == 0 and cluster is not None):  # (labels on the host: the NumPy sums, or G alone)
                labels = None if cluster is None else self._labels_host(cluster)
                if L is not None:
                    meat, G = self._cox_sandwich_host(L, labels)
                else:
                    G = int(np.unique(labels).size)
            out = capi.cox_sandwich_table(got["info"], meat, got["score"], beta[cols], cov_type, G)
            out["dof"] = float(got["n_events"]) - m
            out.update(cols=cols, loglik=float(got["loglik"]), residual_sum=float(got["residual_sum"]))
            return out
        out = capi.cox_wald_table(got["info"], got["score"], beta[cols], got["n_events"])
        out.update(cols=cols, loglik=float(got["loglik"]), residual_sum=float(got["residual_sum"]))
        return out

    # ---- Cox: the test of proportional hazards -----------------------------------------------------------------------
    @staticmethod
    def _cox_zph_host(Xs, beta, time, status, w, gt, ties):
        """cox_zph_device's quantities in fp64 NumPy, by the same decomposition as _cox_information_host with the event
        weights wd g^q, q = 0, 1, 2: Xs (n, m) the support's columns, gt (n,) the centred time transform (read at the
        rows with status 1), the other arguments in row order."""
        n, m = Xs.shape
        eta = np.zeros(n)
        for c in range(m):  # (column by column: a row's sum does not depend on where the row lies)
            eta += Xs[:, c] * beta[c]
        order = np.argsort(time, kind="stable")
        x, eta, t, d = Xs[order], eta[order], time[order], status[order]
        wd = w[order] * d
        g = np.where(d != 0, gt[order], 0.0)
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        starts = np.nonzero(new)[0]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        last = np.append(starts[1:] - 1, n - 1)[np.cumsum(new) - 1]
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))  # (comparisons: a NaN stays a NaN)
        e = np.exp(a)
        r = first if ties == "breslow" else np.arange(n)
        S0 = np.cumsum(e[::-1])[::-1][r]
        out = {"loglik": float(np.sum(wd * (a - np.log(S0)))), "n_events": float(np.sum(wd))}
        ev = d != 0
        U = np.cumsum((e[:, None] * x)[::-1], axis=0)[::-1][r[ev]] / S0[ev][:, None]
        c = wd
        for q in range(3):
            H = np.cumsum(c / S0)
            if ties == "breslow":
                H = H[last]
            v = e * H
            info = x.T @ (v[:, None] * x) - U.T @ (c[ev][:, None] * U)
            out["info%d" % q] = np.tril(info) + np.tril(info, -1).T
            if q < 2:
                out["score%d" % q] = x.T @ (c - v)
            c = c * g
        return out

    def proportional_hazards_test(self, X, y, weight=None, ties="order", transform="km", residuals=False):
        """Cox only: the test of the proportional-hazards assumption of the fitted model on the rows (X, y) -- the score
        test of theta_j = 0 in beta_j(t) = beta_j + theta_j g(t) for every selected column and of all of them together
        (Grambsch and Therneau 1994, in the exact form survival::cox.zph has used since 3.0: the information matrices
        weighted by g and g^2 are computed, not approximated by a constant variance).  y: (n, 2) time and status as in
        fit; weight: n values or None; ties: "order" or "breslow"; transform: "km" (the default), "rank", "identity",
        "log", an array of n values or a callable (capi.zph_transform; g is centred at its event-weighted mean).
        Returns capi.cox_zph_table's dict (chisq, p_value per column on 1 degree of freedom, global_chisq, global_df,
        global_p_value, slope_var, cond, cond_info, positive_definite, score0, score1, n_events) plus cols, the selected
        columns in the order of chisq, transform, gt_centre and loglik.  A small p_value says that the column's effect
        drifts with g(t).  The model is taken to be at its optimum (score0, returned, is treated as 0); selection is not
        corrected for.  An X in GPU memory is read in place on torch's current stream by capi.cox_zph_device, the
        support's columns only (y and weight may be device arrays: n values each are copied to the host); a NumPy X is
        served in fp64 NumPy with the same decomposition.
        residuals=True adds "time" (the J event times in time order) and "scaled_schoenfeld" (J, m): r_j inv(info0) *
        n_events + beta, the points survival::cox.zph plots against g(t), r the Schoenfeld residuals of
        diagnostics_survival (capi.cox_diagnostics_device(kinds=("schoenfeld",)) for an X in GPU memory, where the
        product is a matrix product on the device and the result lies there); NaN where info0 is not positive definite."""
        if self.model_type_int != 4:
            raise ValueError("proportional_hazards_test is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        m = cols.size
        wt = None if weight is None else w
        gt, centre = capi.zph_transform(time, status, wt, transform)
        if on_device:
            st = _current_stream(X)
            got = capi.cox_zph_device(X, cols, beta[cols], time, status, gt, weight=wt, ties=ties, stream=st)
        else:
            Xs = np.asarray(X, dtype=np.float64)[:, cols]
            got = self._cox_zph_host(Xs, beta[cols], time, status, w, gt, ties)
        out = capi.cox_zph_table(got, centre)
        out.update(cols=cols, transform=transform if isinstance(transform, str) else "user", loglik=float(got["loglik"]))
        if residuals:
            C = capi._scaled_factor(np.array(got["info0"], dtype=np.float64))[0] if m > 0 else np.zeros((0, 0))
            if C is None:
                C = np.full((m, m), np.nan)
            C = C * float(got["n_events"])
            if on_device:
                d = capi.cox_diagnostics_device(X, cols, beta[cols], time, status, weight=wt, ties=ties,
                                                kinds=("schoenfeld",), stream=st)
                r = d["schoenfeld"]
                if capi.is_device_array(r):
                    import torch
                    ss = r @ torch.as_tensor(C, device=r.device) + torch.as_tensor(beta[cols], device=r.device)
                else:
                    ss = np.asarray(r) @ C + beta[cols]
            else:
                d = self._cox_diagnostics_host(Xs, beta[cols], time, status, w, ties, None, None, ("schoenfeld",))
                ss = d["schoenfeld"] @ C + beta[cols]
            out.update(time=np.asarray(d["event_times"]), scaled_schoenfeld=ss)
        return out

    # ---- Cox: score tests of the columns left out ----------------------------------------------------------------------
    @staticmethod
    def _cox_score_terms(X, cols, beta, time, status, w, ties):
        """What the Cox score tests share, in fp64 NumPy by cox_addscore_device's decomposition: (got, order, e, v, g, cc,
        P) with got = _cox_information_host's dict, order the rows in time order, e, v, g in position order, cc = dh / S0
        per position and P the panel's support columns v x - e A (n, m)."""
        n, p = X.shape
        m = cols.size
        got = bess_base._cox_information_host(X[:, cols], beta, time, status, w, ties)
        eta = np.zeros(n)
        for c in range(m):  # (column by column: a row's sum does not depend on where the row lies)
            eta += X[:, cols[c]] * beta[c]
        order = np.argsort(time, kind="stable")
        eta, t, d = eta[order], time[order], status[order]
        wd = w[order] * d
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        starts = np.nonzero(new)[0]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        last = np.append(starts[1:] - 1, n - 1)[np.cumsum(new) - 1]
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))
        e = np.exp(a)
        breslow = ties == "breslow"
        r = first if breslow else np.arange(n)
        S0 = np.cumsum(e[::-1])[::-1][r]
        h = wd / S0
        H = np.cumsum(h)
        if breslow:
            H = H[last]
            dh = np.zeros(n)
            dh[starts] = np.add.reduceat(h, starts)
        else:
            dh = h
        v = e * H
        g = wd - v
        cc = dh / S0
        xs = X[order][:, cols]
        if m > 0:
            u = np.cumsum((e[:, None] * xs)[::-1], axis=0)[::-1][r] / S0[:, None]
            A = np.cumsum(dh[:, None] * u, axis=0)
            P = v[:, None] * xs - e[:, None] * A
        else:
            P = np.zeros((n, 0))
        return got, order, e, v, g, cc, P

    @staticmethod
    def _cox_score_tests_host(X, cols, beta, time, status, w, ties, cand):
        """cox_addscore_device's quantities in fp64 NumPy, by the same decomposition (running sums; no risk-set mean of a
        candidate): X (n, p), cols the support, beta (m,), time, status, w (n,) in row order, cand the candidate columns
        (int64) or None = all.  With a = e x_j and Cc the running sum of dh / S0, t_j = sum_l a_l (a_l Cc_l + 2 P_l), P
        the exclusive running sum of Cc a."""
        n, p = X.shape
        m = cols.size
        got, order, e, v, g, cc, P = bess_base._cox_score_terms(X, cols, beta, time, status, w, ties)
        Cc = np.cumsum(cc)
        columns = np.arange(p, dtype=np.int64) if cand is None else np.asarray(cand, dtype=np.int64)
        q = columns.size
        uu, dd, tt, C = np.empty(q), np.empty(q), np.empty(q), np.empty((q, m))
        for j0 in range(0, q, 2048):  # (in blocks: no X-sized temporary here either)
            XJ = X[:, columns[j0:j0 + 2048]][order]
            uu[j0:j0 + 2048] = XJ.T @ g
            C[j0:j0 + 2048] = XJ.T @ P
            dd[j0:j0 + 2048] = v @ (XJ * XJ)
            aj = e[:, None] * XJ
            ca = Cc[:, None] * aj
            Pl = np.cumsum(ca, axis=0) - ca
            tt[j0:j0 + 2048] = np.sum(aj * (aj * Cc[:, None] + 2.0 * Pl), axis=0)
        pd = True
        if m == 0:
            s, aa = np.zeros(q), np.zeros(q)
        else:
            R, pd = capi.info_factor(got["info"])
            if pd:
                rr = R.T @ (R @ got["score"])
                T = C @ np.tril(R).T
                s, aa = np.sum(T * T, axis=1), C @ rr
            else:
                s, aa = np.full(q, np.nan), np.full(q, np.nan)
        out = dict(got)
        out.update(columns=columns, u=uu, d=dd, t=tt, s=s, a=aa, cross=C, positive_definite=bool(pd),
                   support=np.asarray(cols, dtype=np.int64))
        return out

    def score_tests_survival(self, X, y, weight=None, ties="order", candidates=None):
        """Cox only: did the selection leave out a column that matters?  The Rao score test of every candidate column
        against the fitted model on the rows (X, y), without refitting anything: capi.cox_score_test_table's dict --
        columns, score (the adjusted score u - a), variance ((d - t) - s), statistic = score^2 / variance, p_value
        (chi-square, 1 degree of freedom), in_model, dispersion = 1 -- plus cols, the model's support, loglik and
        positive_definite.  y: (n, 2) time and status as in fit; weight: n values or None; ties: "order" (the risk sets
        of the fit) or "breslow"; candidates: None = all p columns, else ascending distinct column numbers.  score and
        variance are row j of the score and the Schur complement of the observed information of the partial likelihood
        of the model extended by column j at coefficient 0 (capi.cox_addscore_device states the sums).  A candidate in
        the support has in_model = True and NaN for statistic and p_value; a non-positive variance or an information
        that is not positive definite gives NaN and nothing is raised.  An X in GPU memory is read in place on torch's
        current stream, in one pass over the candidate columns on the fp64 matrix cores and one streaming pass for the
        risk-set term, with no n x p temporary (y and weight may be device arrays: n values each are copied to the
        host); a NumPy X is served in fp64 NumPy with the same decomposition.  Columns far from centred lose digits in
        d - t (inference_survival's caveat).  Selection is not corrected for.  score_tests() stays None for the Cox
        classes."""
        if self.model_type_int != 4:
            raise ValueError("score_tests_survival is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        self._survival_x(X)
        cand, _ = capi._candidates(candidates, self.p)
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.cox_addscore_device(X, cols, beta[cols], time, status, weight=None if weight is None else w,
                                           ties=ties, candidates=cand, stream=_current_stream(X))
        else:
            got = self._cox_score_tests_host(np.asarray(X, dtype=np.float64), cols, beta[cols], time, status, w, ties,
                                             cand)
        out = capi.cox_score_test_table(got)
        out.update(cols=cols, loglik=float(got["loglik"]), positive_definite=bool(got["positive_definite"]))
        return out

    # ---- Cox: score tests of the groups left out -----------------------------------------------------------------------
    @staticmethod
    def _cox_score_tests_groups_host(X, cols, beta, time, status, w, ties, starts, groups):
        """cox_groupscore_device's quantities in fp64 NumPy with the same decomposition: X (n, p), cols the support, beta
        (m,), time, status, w (n,) in row order, starts the groups' start columns, groups the tested group numbers or None
        = all.  u, C, D, S, a are matrix products over the n rows as in _score_tests_groups_host; T = sum_p cc_p s_p s_p^T
        from the suffix sums s of e x_J of a block.  The tested columns go in blocks of at most 2 048 that hold whole
        groups: no X-sized temporary."""
        n, p = X.shape
        m = cols.size
        got, order, e, v, g, cc, P = bess_base._cox_score_terms(X, cols, beta, time, status, w, ties)
        lists = capi._group_columns(np.asarray(starts, dtype=np.int32), None if groups is None else
                                    np.asarray(groups, dtype=np.int32), p)
        if lists is None:
            raise ValueError("groups must be ascending distinct group numbers")
        tested, width, columns, goc = lists
        q, nt = columns.size, tested.size
        pos = np.concatenate([[0], np.cumsum(width)])
        offsets = np.concatenate([[0], np.cumsum(width * width)]).astype(np.int64)
        tot = int(offsets[-1])
        pd = True
        if m == 0:
            a, S = np.zeros(q), np.zeros(tot)
        else:
            R, pd = capi.info_factor(got["info"])
            a, S = np.full(q, np.nan), np.full(tot, np.nan)
            if pd:
                r, Rl = R.T @ (R @ got["score"]), np.tril(R)
        u, D, T = np.empty(q), np.empty(tot), np.empty(tot)
        t0 = 0
        while t0 < nt:  # (a block: whole groups, at most 2 048 columns unless one group alone is wider)
            t1 = t0 + 1
            while t1 < nt and pos[t1 + 1] - pos[t0] <= 2048:
                t1 += 1
            j0, j1 = int(pos[t0]), int(pos[t1])
            XJ = X[:, columns[j0:j1]][order]
            u[j0:j1] = XJ.T @ g
            VX = v[:, None] * XJ
            sfx = np.cumsum((e[:, None] * XJ)[::-1], axis=0)[::-1]
            CS = cc[:, None] * sfx
            if m > 0 and pd:
                C = XJ.T @ P
                a[j0:j1] = C @ r
                TC = C @ Rl.T
            for t in range(t0, t1):
                k0, k1 = int(pos[t]) - j0, int(pos[t + 1]) - j0
                for out, blk in ((D, XJ[:, k0:k1].T @ VX[:, k0:k1]), (T, sfx[:, k0:k1].T @ CS[:, k0:k1])):
                    up = np.triu(blk)
                    out[offsets[t]:offsets[t + 1]] = (up + np.triu(up, 1).T).reshape(-1)
                if m > 0 and pd:
                    Sg = np.triu(TC[k0:k1] @ TC[k0:k1].T)
                    S[offsets[t]:offsets[t + 1]] = (Sg + np.triu(Sg, 1).T).reshape(-1)
            t0 = t1
        out = dict(got)
        out.update(columns=columns, group_of_column=goc, u=u, a=a, D=D, T=T, S=S, offsets=offsets,
                   positive_definite=bool(pd), support=np.asarray(cols, dtype=np.int64))
        return out

    def score_tests_groups_survival(self, X, y, group, weight=None, ties="order", groups=None):
        """Cox only: did the selection leave out a GROUP that matters?  The Rao score test of every group of columns --
        the units fit(..., group=...) selects -- against the fitted model on the rows (X, y), d degrees of freedom for a
        group of d columns, without refitting anything: capi.cox_group_score_test_table's dict -- group, first_column,
        df, score (the adjusted score vector u - a of each group), statistic = score^T inverse((D - T) - S) score,
        p_value (chi-square, df degrees of freedom), in_model, dispersion = 1 -- plus cols, the model's support, loglik
        and positive_definite.  y: (n, 2) time and status as in fit; weight: n values or None; ties: "order" (the risk
        sets of the fit) or "breslow"; group and groups as in score_tests_groups.  (D - T) - S is the Schur complement of
        the observed information of the partial likelihood of the model extended by the group at coefficient 0
        (capi.cox_groupscore_device states the sums).  A group with a column in the support has in_model = True and NaN
        for statistic and p_value; a group whose (D - T) - S is not positive definite, or an information that is not
        positive definite, gives NaN and nothing is raised.  An X in GPU memory is read in place on torch's current
        stream (a tested group may have at most 64 columns), with no n x p temporary (y and weight may be device arrays:
        n values each are copied to the host); a NumPy X is served in fp64 NumPy with the same definitions.  Columns far
        from centred lose digits in D - T (inference_survival's caveat).  Selection is not corrected for.
        score_tests_groups() and score_tests() stay None for the Cox classes."""
        if self.model_type_int != 4:
            raise ValueError("score_tests_groups_survival is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        self._survival_x(X)
        starts = self._group_runs(group, self.p)
        _, tg = capi._group_lists(starts, groups, self.p)
        if tg is not None and (tg.min() < 0 or tg.max() >= starts.size or (np.diff(tg) <= 0).any()):
            raise ValueError("groups must be ascending distinct group numbers (0 .. %d)" % (starts.size - 1))
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.cox_groupscore_device(X, cols, beta[cols], time, status, starts, groups=tg,
                                             weight=None if weight is None else w, ties=ties, stream=_current_stream(X))
        else:
            got = self._cox_score_tests_groups_host(np.asarray(X, dtype=np.float64), cols, beta[cols], time, status, w,
                                                    ties, starts, tg)
        out = capi.cox_group_score_test_table(got)
        out.update(cols=cols, loglik=float(got["loglik"]), positive_definite=bool(got["positive_definite"]))
        return out

    # ---- Cox: residuals, dfbeta and case influence -------------------------------------------------------------------
    @staticmethod
    def _cox_diagnostics_host(Xs, beta, time, status, w, ties, R, C, kinds):
        """cox_diagnostics_device's quantities in fp64 NumPy, by the same decomposition (running sums, not the O(n^2)
        definition): Xs (n, m) the support's columns, beta (m,), time, status, w (n,) in row order, R (m, m) lower
        triangular and C (m, m) as capi.cox_diagnostics_device takes them (needed by their kinds only)."""
        n, m = Xs.shape
        eta = np.zeros(n)
        for c in range(m):  # (column by column: a row's sum does not depend on where the row lies)
            eta += Xs[:, c] * beta[c]
        order = np.argsort(time, kind="stable")
        x, eta, t, d = Xs[order], eta[order], time[order], status[order]
        wd = w[order] * d
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        starts = np.nonzero(new)[0]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        last = np.append(starts[1:] - 1, n - 1)[np.cumsum(new) - 1]
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))  # (comparisons: a NaN stays a NaN)
        e = np.exp(a)
        breslow = ties == "breslow"
        r = first if breslow else np.arange(n)
        S0 = np.cumsum(e[::-1])[::-1][r]
        h = wd / S0
        H = np.cumsum(h)
        if breslow:
            H = H[last]
        v = e * H
        g = wd - v
        ev = d != 0

        def rows(z):  # position order -> row order
            out = np.empty_like(z)
            out[order] = z
            return out

        out = {"event_rows": order[ev].astype(np.int32), "event_times": t[ev]}
        if "martingale" in kinds:
            out["martingale"] = rows(g)
        if "deviance" in kinds:
            with np.errstate(divide="ignore", invalid="ignore"):
                dd = (v - wd) + np.where(wd == 0, 0.0, wd * np.log(np.where(wd == 0, 1.0, wd) / np.where(wd == 0, 1.0, v)))
            out["deviance"] = rows(np.sign(g) * np.sqrt(2.0 * np.where(dd < 0, 0.0, dd)))
        if m == 0:
            if "displacement" in kinds:
                out["displacement"] = np.zeros(n)
            for k in ("score", "dfbeta"):
                if k in kinds:
                    out[k] = np.zeros((n, 0))
            if "schoenfeld" in kinds:
                out["schoenfeld"] = np.zeros((int(ev.sum()), 0))
            return out
        u = np.cumsum((e[:, None] * x)[::-1], axis=0)[::-1][r] / S0[:, None]
        if "schoenfeld" in kinds:
            out["schoenfeld"] = x[ev] - u[ev]
        if any(k in kinds for k in ("score", "dfbeta", "displacement")):
            if breslow:
                dh = np.zeros(n)
                dh[starts] = np.add.reduceat(h, starts)
                has = np.zeros(n, dtype=bool)
                has[starts] = np.maximum.reduceat(d, starts) > 0
            else:
                dh, has = h, ev
            with np.errstate(invalid="ignore"):
                A = np.cumsum(np.where(has[:, None], dh[:, None] * u, 0.0), axis=0)
                L = (g[:, None] * x - np.where(ev[:, None], wd[:, None] * u, 0.0)) + e[:, None] * A
            if "score" in kinds:
                out["score"] = rows(L)
            if "dfbeta" in kinds:
                T = np.zeros((n, m))
                for c in range(m):
                    T = T + L[:, c, None] * C[c][None, :]
                out["dfbeta"] = rows(T)
            if "displacement" in kinds:
                s2 = np.zeros(n)
                for j in range(m):
                    tj = np.zeros(n)
                    for k in range(j + 1):
                        tj = tj + R[j, k] * L[:, k]
                    s2 = s2 + tj * tj
                out["displacement"] = rows(s2)
        return out

    def diagnostics_survival(self, X, y, weight=None, ties="order", kinds=None):
        """Cox only: which subjects the model fits badly and which move a coefficient, on the rows (X, y).  A dict with
        the kinds asked for (None: all of capi.COX_DIAG_KINDS, as capi.cox_diagnostics_device defines them) --
        martingale, deviance and displacement (n,), score and dfbeta (n, m) in row order, schoenfeld (J, m) for the J
        rows with status 1 in time order -- plus cols, event_rows and event_times (the row and time of every schoenfeld
        row), positive_definite, loglik and residual_sum.  y: (n, 2) time and status as in fit; weight: n values or
        None (on the event terms only); ties: "order" or "breslow".  dfbeta = score @ inv(info) approximates the change
        in beta when a row is dropped; displacement = score_k^T inv(info) score_k is the likelihood displacement, Cox's
        counterpart of Cook's distance.  An X in GPU memory is read in place on torch's current stream -- the
        information by capi.cox_information_device, its factor by capi.info_factor on the host, the rows by
        capi.cox_diagnostics_device -- and the results are tensors on X's device; a NumPy X is served in fp64 NumPy
        with the same decomposition.  When the information is not positive definite dfbeta and displacement are filled
        with NaN, the other kinds are still computed and nothing is raised.  diagnostics() stays None for the Cox
        classes."""
        if self.model_type_int != 4:
            raise ValueError("diagnostics_survival is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        _, kinds = capi._cox_diag_mask(capi.COX_DIAG_KINDS if kinds is None else kinds)
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        m = cols.size
        wt = None if weight is None else w
        if on_device:
            st = _current_stream(X)
            got = capi.cox_information_device(X, cols, beta[cols], time, status, weight=wt, ties=ties, stream=st)
        else:
            Xs = np.asarray(X, dtype=np.float64)[:, cols]
            got = self._cox_information_host(Xs, beta[cols], time, status, w, ties)
        if m > 0:
            R, pd = capi.info_factor(got["info"])
        else:
            R, pd = np.zeros((0, 0)), True
        C = R.T @ R
        need = [k for k in kinds if k in ("dfbeta", "displacement")]
        ask = kinds if pd else tuple(k for k in kinds if k not in need)
        out = {}
        if on_device:
            if ask:
                out = capi.cox_diagnostics_device(X, cols, beta[cols], time, status, factor=R if pd else None,
                                                  cinv=C if pd else None, weight=wt, ties=ties, kinds=ask, stream=st)
            else:
                ev = np.argsort(time, kind="stable")
                ev = ev[status[ev] != 0].astype(np.int32)
                out = {"event_rows": ev, "event_times": time[ev]}
        else:
            out = self._cox_diagnostics_host(Xs, beta[cols], time, status, w, ties, R, C, ask)
        if not pd:
            torch = sys.modules.get("torch")
            for k in need:
                shape = (n,) if k == "displacement" else (n, m)
                if on_device and torch is not None and isinstance(X, torch.Tensor):
                    out[k] = torch.full(shape, float("nan"), dtype=torch.float64, device=X.device)
                else:
                    out[k] = np.full(shape, np.nan)
        res = {k: out[k] for k in kinds}
        res.update(cols=cols, event_rows=out["event_rows"], event_times=out["event_times"], positive_definite=bool(pd),
                   loglik=float(got["loglik"]), residual_sum=float(got["residual_sum"]))
        return res

    # ---- Cox: baseline hazard and survival curves ------------------------------------------------------------------
    def _support_eta(self, X, cols, beta):
        """X[:, cols] @ beta[cols] for a NumPy X, column by column: a row's sum does not depend on where the row lies."""
        X = np.asarray(X, dtype=np.float64)
        eta = np.zeros(X.shape[0])
        for j in cols:
            eta += X[:, j] * beta[j]
        return eta

    @staticmethod
    def _baseline_host(eta, time, status, w):
        """(times, cumhaz) in fp64 NumPy with the definitions of capi.cox_baseline_device: eta, time, status, w are
        n-vectors in row order."""
        n = eta.size
        order = np.argsort(time, kind="stable")
        eta, t, d, w = eta[order], time[order], status[order], w[order]
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        starts = np.nonzero(new)[0]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))  # (comparisons: a NaN stays a NaN)
        S = np.cumsum(np.exp(a)[::-1])[::-1][first]
        H = np.cumsum((w * d) / S)
        ends = np.append(starts[1:] - 1, n - 1)
        event = np.maximum.reduceat(d, starts) > 0
        return t[ends][event], H[ends][event]

    def fit_baseline(self, X, y, weight=None):
        """Cox only, after fit(): the Breslow baseline cumulative hazard of the fitted model on the rows X, y (the rows
        it was fitted to), y = (time, status) as in fit, weight n values >= 0 or None.  Sets baseline_times_ (the distinct
        times that carry an event, ascending) and baseline_cumhaz_ (H0 at them; definitions: capi.cox_baseline_device) and
        returns self.  An X in GPU memory is read once, in place, on torch's current stream (y and weight may be device
        arrays: n values each are copied to the host); a NumPy X is served in fp64 NumPy.  fit() does not call this."""
        if self.model_type_int != 4:
            raise ValueError("fit_baseline is for the Cox classes, this is a %s model" % self.model_type)
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        if not (w >= 0.0).all():
            raise ValueError("weight should be non-negative")
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.cox_baseline_device(X, cols, beta[cols], time, status, weight=None if weight is None else w,
                                           stream=_current_stream(X))
            self.baseline_times_, self.baseline_cumhaz_ = got["times"], got["cumhaz"]
        else:
            self.baseline_times_, self.baseline_cumhaz_ = self._baseline_host(self._support_eta(X, cols, beta), time,
                                                                              status, w)
        return self

    def predict_survival(self, X, times=None, kind="survival"):
        """Cox only, after fit_baseline(): the (n, T) matrix S(t_j | x_i) = exp(-H0(t_j) exp(clip(eta_i, -30, 30)))
        (kind="survival") or the cumulative hazard H0(t_j) exp(clip(eta_i)) (kind="cumhaz") at the times given (any order,
        repeats allowed; None = baseline_times_), H0 the right-continuous step function of capi.baseline_at.  An X in GPU
        memory gives a tensor on X's device, written once by capi.cox_survival_device; a NumPy X gives NumPy."""
        if self.model_type_int != 4:
            raise ValueError("predict_survival is for the Cox classes, this is a %s model" % self.model_type)
        on_device, n = self._survival_x(X)
        if kind not in capi.SURV_KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(capi.SURV_KINDS), kind))
        if getattr(self, "baseline_times_", None) is None:
            raise ValueError("predict_survival needs the baseline hazard: call fit_baseline(X, y) first")
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            return capi.cox_survival_device(X, cols, beta[cols], self.baseline_times_, self.baseline_cumhaz_, times=times,
                                            kind=kind, stream=_current_stream(X))
        grid = self.baseline_times_ if times is None else times
        if np.ndim(grid) > 1:
            raise ValueError("times must be 1-D")
        hg = capi.baseline_at(self.baseline_times_, self.baseline_cumhaz_, grid).reshape(-1)
        if hg.size < 1:
            raise ValueError("times is empty: no curve to compute (a baseline without an event has no times of its own)")
        eta = self._support_eta(X, cols, beta)
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))
        z = np.exp(a)[:, None] * hg[None, :]
        return z if kind == "cumhaz" else np.exp(-z)

    # ---- Cox: restricted mean and quantile survival times ------------------------------------------------------------
    _SURVTIME_BLOCK = 1 << 23  # elements of the largest temporary of the NumPy routes: 64 MB of float64

    def _survtime_model(self, X, who):
        """(on_device, n, cols, beta) for predict_rmst / predict_quantile, with their checks."""
        if self.model_type_int != 4:
            raise ValueError("%s is for the Cox classes, this is a %s model" % (who, self.model_type))
        on_device, n = self._survival_x(X)
        if getattr(self, "baseline_times_", None) is None:
            raise ValueError("%s needs the baseline hazard: call fit_baseline(X, y) first" % who)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        return on_device, n, np.nonzero(beta)[0], beta

    def _support_e(self, X, cols, beta):
        eta = self._support_eta(X, cols, beta)
        return np.exp(np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta)))  # (a NaN stays a NaN)

    def predict_rmst(self, X, tau):
        """Cox only, after fit_baseline(): the restricted mean survival times RMST_i(tau_j) = integral_0^tau_j S(t | x_i) dt
        of the curves of predict_survival, S a step function and the integral therefore a finite sum over the segments of
        capi.rmst_segments (tau finite and >= 0, any order, repeats allowed; tau = 0 gives 0.0, a baseline without an
        event gives tau).  Returns (n, T), or (n,) for a tau that is a single number.  No curve is stored: an X in GPU
        memory is read once on torch's current stream by capi.cox_survival_times_device and gives a tensor on X's device;
        a NumPy X is served in fp64 NumPy with the same definitions, the segments summed in blocks."""
        on_device, n, cols, beta = self._survtime_model(X, "predict_rmst")
        single = np.ndim(tau) == 0
        tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
        if on_device:
            out = capi.cox_survival_times_device(X, cols, beta[cols], self.baseline_times_, self.baseline_cumhaz_, tau=tau,
                                                 stream=_current_stream(X))["rmst"]
            return out[:, 0] if single else out
        hs, wd, cut = capi.rmst_segments(self.baseline_times_, self.baseline_cumhaz_, tau)
        if not (hs >= 0.0).all():
            raise ValueError("base_cumhaz should be non-negative")
        e = self._support_e(X, cols, beta)
        out = np.empty((n, cut.size))
        acc = np.where(np.isnan(e), e, 0.0)  # one running sum per row over the segments in ascending order
        block = max(1, self._SURVTIME_BLOCK // max(n, 1))
        k = 0
        for j in np.argsort(cut, kind="stable"):
            while k < cut[j]:
                kk = min(int(cut[j]), k + block)
                acc = acc + np.exp(-(e[:, None] * hs[None, k:kk])) @ wd[k:kk]
                k = kk
            out[:, j] = acc
        return out[:, 0] if single else out

    def predict_quantile(self, X, q=0.5):
        """Cox only, after fit_baseline(): the q-quantiles of the survival time of every row, the first baseline time at
        which S(t | x_i) <= 1 - q, found as the first time at which baseline_cumhaz_ * exp(clip(eta_i)) (one fp64 product)
        reaches -log1p(-q); +inf where the curve never gets there.  q = 0.5 is the median survival time.  q in (0, 1), a
        number (the result is (n,)) or 1-D (the result is (n, Q)).  survival::survfit averages two times where S equals
        1 - q exactly; this does not.  An X in GPU memory is read once on torch's current stream by
        capi.cox_survival_times_device and gives a tensor on X's device; a NumPy X is served in fp64 NumPy."""
        on_device, n, cols, beta = self._survtime_model(X, "predict_quantile")
        single = np.ndim(q) == 0
        c = capi.survival_levels(q)
        if on_device:
            out = capi.cox_survival_times_device(X, cols, beta[cols], self.baseline_times_, self.baseline_cumhaz_,
                                                 hazard_levels=c, stream=_current_stream(X))["quantile"]
            return out[:, 0] if single else out
        ut, hz = capi._quantile_baseline(self.baseline_times_, self.baseline_cumhaz_)
        e = self._support_e(X, cols, beta)
        out = np.full((n, c.size), np.inf)
        rows = max(1, self._SURVTIME_BLOCK // max(hz.size, 1))
        for i0 in range(0, n if hz.size else 0, rows):
            z = e[i0:i0 + rows, None] * hz[None, :]
            for j in range(c.size):
                hit = z >= c[j]
                g = hit.argmax(axis=1)  # (hz non-decreasing and e > 0: the first True)
                out[i0:i0 + rows, j] = np.where(hit[np.arange(g.size), g], ut[g], np.inf)
        out[np.isnan(e)] = np.nan
        return out[:, 0] if single else out

    # ---- Cox: standard errors and confidence bands of the curves -----------------------------------------------------
    @staticmethod
    def _hazard_var_host(Xs, beta, time, status, w, ties, times):
        """(cumhaz (T,), var0 (T,), drift (T, m)) in fp64 NumPy with the definitions of
        capi.cox_baseline_variance_device, by the same decomposition (running sums): Xs (n, m) the support's columns,
        beta (m,), time, status, w (n,) in row order, times (T,)."""
        n, m = Xs.shape
        eta = np.zeros(n)
        for c in range(m):  # (column by column: a row's sum does not depend on where the row lies)
            eta += Xs[:, c] * beta[c]
        order = np.argsort(time, kind="stable")
        x, eta, t, d = Xs[order], eta[order], time[order], status[order]
        wd = w[order] * d
        new = np.ones(n, dtype=bool)
        new[1:] = t[1:] != t[:-1]
        first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))  # (comparisons: a NaN stays a NaN)
        e = np.exp(a)
        r = first if ties == "breslow" else np.arange(n)
        S0 = np.cumsum(e[::-1])[::-1][r]
        h = wd / S0
        H, V0 = np.cumsum(h), np.cumsum(wd / (S0 * S0))
        u = np.cumsum((e[:, None] * x)[::-1], axis=0)[::-1][r] / S0[:, None]
        A = np.cumsum(np.where((d != 0)[:, None], h[:, None] * u, 0.0), axis=0)
        idx = np.searchsorted(t, times, side="right") - 1
        at = lambda z: np.where((idx >= 0).reshape((-1,) + (1,) * (z.ndim - 1)), z[np.maximum(idx, 0)], 0.0)
        return at(H), at(V0), at(A)

    @staticmethod
    def _bands_host(Xs, beta, cumhaz, var0, drift, R, kind, conf_type, zc, names):
        """capi.cox_survival_band_device's numbers in fp64 NumPy with the same definitions: Xs (n, m) the support's
        columns; returns {name: (n, T)}.  The sum of squares is formed directly, one support column at a time."""
        n, m = Xs.shape
        eta = np.zeros(n)
        for c in range(m):
            eta += Xs[:, c] * beta[c]
        e = np.exp(np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta)))[:, None]
        H = cumhaz[None, :]
        V = np.zeros((n, cumhaz.size))
        for j in range(m):
            tj, pj = np.zeros(n), np.zeros(cumhaz.size)
            for k in range(j + 1):
                tj = tj + R[j, k] * Xs[:, k]
                pj = pj + R[j, k] * drift[:, k]
            dj = pj[None, :] - H * tj[:, None]
            V = V + dj * dj
        V = V + var0[None, :]
        floor0 = lambda z: np.where(z < 0.0, 0.0, z)  # (comparisons: a NaN stays a NaN)
        ceil1 = lambda z: np.where(z > 1.0, 1.0, z)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            L = H * e
            sq = np.sqrt(V)
            seL = e * sq
            wv = zc * seL
            r = (zc * sq) / H
            if kind == "cumhaz":
                est, se = L, seL
                lo, hi = (floor0(L - wv), L + wv) if conf_type == "plain" else (L * np.exp(-r), L * np.exp(r))
            else:
                est = np.exp(-L)
                se = est * seL
                if conf_type == "plain":
                    lo, hi = floor0(est - zc * se), ceil1(est + zc * se)
                elif conf_type == "log":
                    lo, hi = np.exp(-(L + wv)), np.exp(-floor0(L - wv))
                else:
                    lo, hi = np.exp(-(L * np.exp(r))), np.exp(-(L * np.exp(-r)))
        zero = np.broadcast_to(H == 0.0, est.shape)  # before the first event: no 0 / 0, the bounds are the estimate
        se, lo, hi = np.where(zero, L, se), np.where(zero, est, lo), np.where(zero, est, hi)
        return {k: v for k, v in (("estimate", est), ("se", se), ("lower", lo), ("upper", hi)) if k in names}

    def fit_survival_bands(self, X, y, times, weight=None, ties="breslow"):
        """Cox only, after fit(): what the standard errors and confidence bands of the fitted model's curves need from
        the rows X, y (the rows it was fitted to), y = (time, status) as in fit, weight n values >= 0 or None, at the
        grid `times` (any order, repeats allowed).  Runs the observed information (capi.cox_information_device), its
        factor (capi.info_factor) and capi.cox_baseline_variance_device, sets band_times_, band_cumhaz_, band_var0_ (T,),
        band_drift_ (T, m), band_factor_ (m, m), band_cols_ and returns self.  Raises ValueError when the information is
        not positive definite (collinear support columns, or too few events for the support).  An X in GPU memory is
        read in place on torch's current stream; a NumPy X is served in fp64 NumPy with the same definitions.  fit(),
        fit_baseline() and predict_survival() do not depend on this."""
        if self.model_type_int != 4:
            raise ValueError("fit_survival_bands is for the Cox classes, this is a %s model" % self.model_type)
        if ties not in capi.TIES:
            self._survival_x(X)
            raise ValueError("ties must be one of %s, got %r" % (sorted(capi.TIES), ties))
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        if not (w >= 0.0).all():
            raise ValueError("weight should be non-negative")
        if np.ndim(times) > 1:
            raise ValueError("times must be 1-D")
        tg = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        if tg.size < 1:
            raise ValueError("times is empty: no curve to compute")
        if np.isnan(tg).any():
            raise ValueError("There is NAN value in times")
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        m = cols.size
        wt = None if weight is None else w
        if on_device:
            st = _current_stream(X)
            info = capi.cox_information_device(X, cols, beta[cols], time, status, weight=wt, ties=ties, stream=st)["info"]
        else:
            Xs = np.asarray(X, dtype=np.float64)[:, cols]
            info = self._cox_information_host(Xs, beta[cols], time, status, w, ties)["info"]
        R, pd = capi.info_factor(info) if m > 0 else (np.zeros((0, 0)), True)
        if not pd:
            raise ValueError("fit_survival_bands: the observed information of the fitted model on these rows is not "
                             "positive definite (collinear support columns, or too few events): no standard errors")
        if on_device:
            got = capi.cox_baseline_variance_device(X, cols, beta[cols], time, status, tg, weight=wt, ties=ties, stream=st)
            cumhaz, var0, drift = got["cumhaz"], got["var0"], got["drift"]
        else:
            cumhaz, var0, drift = self._hazard_var_host(Xs, beta[cols], time, status, w, ties, tg)
        self.band_times_, self.band_cumhaz_, self.band_var0_, self.band_drift_ = tg.copy(), cumhaz, var0, drift
        self.band_factor_, self.band_cols_ = R, cols
        return self

    def predict_survival_bands(self, X, kind="survival", conf_type="log-log", level=0.95,
                               what=("estimate", "lower", "upper")):
        """Cox only, after fit_survival_bands(): the curves of the rows of X at band_times_ with their standard errors
        and pointwise confidence bounds.  kind "survival" or "cumhaz"; conf_type "plain", "log" or "log-log" (survival
        only); level in (0, 1); what a subset of ("estimate", "se", "lower", "upper").  Returns a dict from name to an
        (n, T) array (definitions: capi.cox_survival_band_device): views of one tensor on X's device for an X in GPU
        memory, read in place on torch's current stream, NumPy for a NumPy X."""
        if self.model_type_int != 4:
            raise ValueError("predict_survival_bands is for the Cox classes, this is a %s model" % self.model_type)
        on_device, n = self._survival_x(X)
        capi._band_kind(kind, conf_type)
        _, names = capi._band_mask(what)
        zc = capi.normal_quantile(level)
        if getattr(self, "band_times_", None) is None:
            raise ValueError("predict_survival_bands needs the variance terms: call fit_survival_bands(X, y, times) first")
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if not np.array_equal(cols, self.band_cols_):
            raise ValueError("the support has changed since fit_survival_bands: call it again")
        if on_device:
            return capi.cox_survival_band_device(X, cols, beta[cols], self.band_cumhaz_, self.band_var0_, self.band_drift_,
                                                 self.band_factor_, kind=kind, conf_type=conf_type, level=level,
                                                 what=names, stream=_current_stream(X))
        Xs = np.asarray(X, dtype=np.float64)[:, cols]
        return self._bands_host(Xs, beta[cols], self.band_cumhaz_, self.band_var0_, self.band_drift_, self.band_factor_,
                                kind, conf_type, zc, names)

    # ---- Cox: how good the curves are -------------------------------------------------------------------------------
    @staticmethod
    def _brier_host(eta, hg, times, time, w, row_a, time_b):
        """BS (T, R) in fp64 NumPy with the definitions of capi.cox_brier_device: eta (n, R), hg (T, R), the rest
        vectors.  One model at a time: no temporary beyond n x T."""
        T, R = hg.shape
        a = np.where(eta > 30.0, 30.0, np.where(eta < -30.0, -30.0, eta))
        left = time[:, None] <= times[None, :]
        wa, W = w * row_a, np.sum(w)
        bs = np.empty((T, R))
        for r in range(R):
            nz = -(np.exp(a[:, r])[:, None] * hg[None, :, r])
            s, q = np.exp(np.where(left, nz, 0.0)), np.expm1(np.where(left, 0.0, nz))  # (one of the two is used)
            sa = np.sum(np.where(left, wa[:, None] * (s * s), 0.0), axis=0)
            sq = np.sum(np.where(left, 0.0, w[:, None] * (q * q)), axis=0)
            bs[:, r] = (sa + time_b * sq) / W
        return bs

    def brier_survival(self, X, y, times, weight=None, censoring="km"):
        """Cox only, after fit_baseline(): the time-dependent Brier score of the fitted model's curves S(t | x) on the rows
        X, y (which it may not have seen) under inverse-probability-of-censoring weights, at the times given.  y = (time,
        status) as in fit, weight n values >= 0 or None, censoring "km" (Kaplan-Meier weights from these rows), None or
        a pair (row_a, time_b): capi.ipcw_weights.  Returns the dict of capi.cox_brier_device for the one model: "brier",
        "null", "ipa" (T,), "ibs", "ibs_null" (floats; NaN unless the times are at least 2 and strictly increasing),
        "row_a", "time_b", "sum_w".  An X in GPU memory is read once, in place, on torch's current stream, by a fused
        reduction that stores no curve; a NumPy X is served in fp64 NumPy."""
        if self.model_type_int != 4:
            raise ValueError("brier_survival is for the Cox classes, this is a %s model" % self.model_type)
        on_device, n = self._survival_x(X)
        if getattr(self, "baseline_times_", None) is None:
            raise ValueError("brier_survival needs the baseline hazard: call fit_baseline(X, y) first")
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        if not (w >= 0.0).all():
            raise ValueError("weight should be non-negative")
        if not float(np.sum(w)) > 0.0:
            raise ValueError("the weights sum to 0")
        if np.ndim(times) > 1:
            raise ValueError("times must be 1-D")
        hg = capi.baseline_at(self.baseline_times_, self.baseline_cumhaz_, times).reshape(-1, 1)
        hg, times = capi._brier_grid(hg, times, 1)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.cox_brier_device(X, cols, beta[cols], hg, times, time, status,
                                        weight=None if weight is None else w, censoring=censoring,
                                        stream=_current_stream(X))
        else:
            row_a, time_b = capi.ipcw_weights(time, status, times, w, censoring)
            eta = self._support_eta(X, cols, beta).reshape(-1, 1)
            got = capi._brier_result(self._brier_host(eta, hg, times, time, w, row_a, time_b), times, time, status, w,
                                     row_a, time_b)
        out = dict(got)
        out["brier"], out["ipa"] = got["brier"][:, 0], got["ipa"][:, 0]
        out["ibs"] = float(np.asarray(got["ibs"]).reshape(-1)[0])
        return out

    # ---- discrimination: AUC(t) and Uno's C (Cox), ROC AUC (Logistic) ------------------------------------------------
    def auc_survival(self, X, y, times=None, weight=None, censoring="km", tau=None):
        """Cox only: how well the fitted model ranks rows it may not have seen, robust to the censoring pattern: the
        cumulative/dynamic AUC at the times given (any order; None: none), its mean weighted by the drops of the rows'
        Kaplan-Meier survival, and Uno's C truncated at tau (None: not truncated).  y = (time, status) as in fit, weight n
        values >= 0 or None, censoring "km" (Kaplan-Meier weights from these rows), None, row_a (n values) or the pair
        (row_a, time_b) of brier_survival.  Returns the dict of capi.cox_auc_device for the one model: "auc", "greater",
        "equal", "cases", "controls", "km_drop" (T,), "mean_auc", "uno_c", "uno_concordant", "uno_tied",
        "uno_comparable" (floats), "row_a".  An X in GPU memory is read once, in place, on torch's current stream, by a
        tiled pair kernel; a NumPy X is served in fp64 NumPy (a sort, then running sums per time; Uno's C by blocks of
        pairs)."""
        if self.model_type_int != 4:
            raise ValueError("auc_survival is for the Cox classes, this is a %s model" % self.model_type)
        on_device, n, time, status, w, weight = self._survival_data(X, y, weight)
        if not (w >= 0.0).all():
            raise ValueError("weight should be non-negative")
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.cox_auc_device(X, cols, beta[cols], times, time, status, weight=None if weight is None else w,
                                      censoring=censoring, tau=tau, stream=_current_stream(X))
        else:
            got = capi._cox_auc_host(self._support_eta(X, cols, beta).reshape(-1, 1), times, time, status, w, censoring,
                                     tau)
        out = dict(got)
        for k in ("auc", "greater", "equal"):
            out[k] = got[k][:, 0]
        for k in ("mean_auc", "uno_c", "uno_concordant", "uno_tied"):
            out[k] = float(np.asarray(got[k]).reshape(-1)[0])
        return out

    def auc(self, X, y, weight=None):
        """Logistic only: the ROC AUC of the fitted model on rows it may not have seen -- the weighted share of (case,
        control) pairs that the linear predictor orders correctly, ties counting half; cases are y > 0.5.  weight: n
        values >= 0 or None.  Returns {"auc", "greater", "equal", "pos_weight", "neg_weight"} as floats (auc is NaN when
        a class is empty): capi.auc_device.  An X in GPU memory is read once, in place, on torch's current stream; a
        NumPy X is served in fp64 NumPy (a sort and a running sum)."""
        if self.model_type_int != 2:
            raise ValueError("auc is for the Logistic classes, this is a %s model" % self.model_type)
        on_device, n = self._survival_x(X)
        beta = np.asarray(self.beta, dtype=np.float64).reshape(-1)
        cols = np.nonzero(beta)[0]
        if on_device:
            got = capi.auc_device(X, cols, beta[cols], y, weight=weight, stream=_current_stream(X))
        else:
            got = capi._auc_host(self._support_eta(X, cols, beta).reshape(-1, 1), y, weight)
        return {k: float(np.asarray(v).reshape(-1)[0]) for k, v in got.items()}


def _make(name, algorithm_type, model_type):
    def __init__(self, max_iter=20, exchange_num=0, path_type="seq", is_warm_start=True, sequence=None,
                 lambda_sequence=None, s_min=None, s_max=None, K_max=None, epsilon=0.0001, lambda_min=None,
                 lambda_max=None, ic_type="ebic", is_cv=False, K=5, is_screening=False, screening_size=None,
                 powell_path=1, always_select=[], tao=0.):
        bess_base.__init__(self, algorithm_type=algorithm_type, model_type=model_type, path_type=path_type,
                           max_iter=max_iter, exchange_num=exchange_num, is_warm_start=is_warm_start,
                           sequence=sequence, lambda_sequence=lambda_sequence, s_min=s_min, s_max=s_max,
                           K_max=K_max, epsilon=epsilon, lambda_min=lambda_min, lambda_max=lambda_max,
                           ic_type=ic_type, is_cv=is_cv, K=K, is_screening=is_screening,
                           screening_size=screening_size, powell_path=powell_path, always_select=always_select,
                           tao=tao)

    doc = ("%s: %s best-subset selection for the %s model (counterpart of bess.linear.%s, "
           "python/bess/linear.py:433-921).\n" % (name, algorithm_type, model_type, name)) + bess_base.__doc__
    return type(name, (bess_base,), {"__init__": __init__, "__doc__": doc})


PdasLm = _make("PdasLm", "Pdas", "Lm")
PdasLogistic = _make("PdasLogistic", "Pdas", "Logistic")
PdasPoisson = _make("PdasPoisson", "Pdas", "Poisson")
PdasCox = _make("PdasCox", "Pdas", "Cox")
L0L2Lm = _make("L0L2Lm", "L0L2", "Lm")
L0L2Logistic = _make("L0L2Logistic", "L0L2", "Logistic")
L0L2Poisson = _make("L0L2Poisson", "L0L2", "Poisson")
L0L2Cox = _make("L0L2Cox", "L0L2", "Cox")
GroupPdasLm = _make("GroupPdasLm", "GroupPdas", "Lm")
GroupPdasLogistic = _make("GroupPdasLogistic", "GroupPdas", "Logistic")
GroupPdasPoisson = _make("GroupPdasPoisson", "GroupPdas", "Poisson")
GroupPdasCox = _make("GroupPdasCox", "GroupPdas", "Cox")
