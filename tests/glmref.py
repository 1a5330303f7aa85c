"""Extended-precision reference for the logistic and Poisson SOLVER kernels reached by bessx_op_glm_gh / bessx_op_glm_irls and
by Session.fit (k_glm_eta_gh, k_glm_irls_prep, stage (B) of k_irls_gram, and behind them k_xtv + k_score, the Gram kernels
and k_chol): pure NumPy in np.longdouble, no GPU, no oracle.  It restates the formulas AS THE KERNELS STATE THEM (family 2 =
logistic, 3 = Poisson; w_i = weight, ones without; m_i = 1 on the training rows of a CV fold, 0 on its test rows, ones
without a fold):

  get_A front half (k_glm_eta_gh), model (cols, b, coef0), eta_i = sum_a x_i,cols[a] b_a + coef0
    logistic (src/Algorithm.h:1223-1235)   e = exp(clamp(eta, +-30)), pr = e / (e + 1), g = w (y - pr) m, h = w pr (1 - pr) m
      train summand (src/Metric.h:266-290) w (y log pr + (1 - y) log(1 - pr))                     over ALL rows
      held-out summand (:338-351)          the same with the clamp at +-25                         over the rows with m = 0
    Poisson (:1338-1340)                   e = exp(eta) UN-clamped, g = (y - e) w m, h = e w m
      summand (:426-440, :489; src/poisson.cpp:15-45)  v = clamp(eta, +-30), (y v - exp(v) - sum_{j <= y} log j) w
                                           over all rows / over the rows with m = 0
    scores (:1238-1257, :1342-1361)        d_j = sum_i x_ij g_i - 2 lam beta_j, l2_j = sum_i x_ij^2 h_i + 2 lam,
                                           bd_j = (sqrt(l2_j) beta_j + d_j / sqrt(l2_j))^2
  IRLS step t (k_glm_irls_prep, k_irls_gram), iterate bcur on [1, X_A], eta_i = bcur_0 + sum_a x_i,A[a] bcur_{a+1}
    logistic (:1160-1166 for t = 0, :1177-1194 for t >= 1)   Pi = e / (1 + e) with the clamp at +-30, W = Pi (1 - Pi), raised
      to 0.001 only for t >= 1 and only with wfloor; z = eta + (y - Pi) / W with the UN-clamped eta;
      ll summand (y log Pi + (1 - y) log(1 - Pi)) w m
    Poisson (:1286-1314)   t = 0: e = exp(eta) as it is, NO ll summand; t >= 1: eta clamped to +-30, e = exp(eta) raised to
      0.001 (the kernels do this for every t >= 1, with or without wfloor), ll summand (y eta - e) w m; W = e,
      z = eta + (y - e) / e with the eta just described
    Wv = W w m;  Gram = [1, X_A, z]^T diag(Wv) [1, X_A, z];  bnext solves (Gram_AA + 2 lam diag(0, 1, ..., 1)) b = Gram_Az.

Bounds.  Every per-row bound is a FIRST-ORDER forward-error bound of the stated formula, evaluated in longdouble from the
reference's own values, so it carries the amplification that is really there and nothing else (u = 2^-53):
  eta      de = (m + 2) u sum_a |x_ia b_a| (+ |intercept|): gamma_m of the linear predictor, any order of summation
  e        relative re = de + 2 u (the clamp is 1-Lipschitz; 2 u for the device exp, as tests/coxevalref.py allows)
  pr       relative rp = (1 - pr) re + 2 u            (e + 1 and the division)
  1 - pr   relative rq = pr re + 2 u pr / (1 - pr) + u: the absolute error of pr, u pr, is u pr / (1 - pr) RELATIVE to 1 - pr --
           at eta = 30 that is 1.2e-3.  It goes into log(1 - pr), into W = pr (1 - pr) and, through 1 / W, into z.
  log      absolute error = relative error of its argument + 2 u |log|
  W floor  max(., 0.001) is 1-Lipschitz; a row whose W + dW stays under the floor has W = 0.001 exactly (dW = 0)
and so on through g, h, Wv, z and the summands (the code below is the statement).  A sum's bound is the sum of its rows'
bounds plus n u sum_i |term_i| (gamma_n, any order).  The Gram takes xprec's bound 32 sqrt(n) u |c_j|_Wv |c_k|_Wv (weighted
column norms) PLUS what the per-row bounds of Wv and z carry into it: sum_i dWv_i |c_ij c_ik|, and for the z row / column
sum_i Wv_i |c_ij| dz_i (the z-z entry: sum_i Wv_i (2 |z_i| dz_i + dz_i^2)).  bnext: xprec.assert_fit_close with the condition
number of the reference system, compared only where that is under COND_LIMIT (the bound says nothing beyond).  bd: the forward-error form of xprec.scores / coxsolveref.assert_scores_close with
M1_j = sum_i |x_ij g_i| + 2 lam |beta_j|, M2_j = sum_i x_ij^2 h_i + 2 lam and the rows' dg, dh carried along; l2 is a sum of
non-negative terms, so no column is ill-conditioned and NONE is left out.

Constants.  Each bound is c x (the first-order expression at c = 1).  c is not taken from any kernel: fp64 NumPy evaluating
the same formulas (the *_fp64 functions, the CPU stand-in) is measured against this reference on every case of this module
(tests/test_glm_reference.py), the maximum is stored as *_NUMPY_MAX and c is the next power of two at or above four times
that (the convention that gave coxsolveref.SCORE_C = 64 from 8.79); the factor four allows for a different but equally valid
order of evaluation.  The GPU has to fit inside the same constants.

The module also owns the seeded cases, so that the CPU and the GPU file use the same inputs."""
import numpy as np

import xprec

LD, U, EXTENDED = xprec.LD, xprec.U, xprec.EXTENDED
ld = xprec.ld
CLAMP, CLAMP_TEST, FLOOR = 30.0, 25.0, 0.001
LOGISTIC, POISSON = 2, 3

# fp64 NumPy under the first-order bounds at c = 1, maxima over all_gh_cases() and all_irls_cases(); measured by
# tests/test_glm_reference.py::test_fp64_numpy_sits_inside_every_bound_and_fixes_the_constants (it prints them)
# g, h: logistic, n = 1025, m = 1, wide; wv, z: logistic, T0 = 30, n = 1025, wide, t = 0 and t = 1 (a case of SOLVE_CASES)
ROW_NUMPY_MAX = {"g": 0.5349, "h": 0.5257, "wv": 0.6493, "z": 0.5345}
SUM_NUMPY_MAX = 0.4142    # the loss sums of op_glm_gh and the log-likelihood of an IRLS step (logistic, T0 = 110, n = 1, t = 0)
SCORE_NUMPY_MAX = 1.5943  # bd (logistic, n = 1, m = 1, wide)
ROW_C = {"g": 4.0, "h": 4.0, "wv": 4.0, "z": 4.0}  # 4 x the maxima, rounded up to powers of two
SUM_C = 2.0
SCORE_C = 8.0


def constant_from(measured):
    """The next power of two at or above four times the measured maximum."""
    return float(2.0 ** np.ceil(np.log2(4.0 * measured)))


# ---- the operations ---------------------------------------------------------------------------------------------------
def _wm(n, w, mask):
    return (np.ones(n, dtype=LD) if w is None else ld(w)), (np.ones(n, dtype=LD) if mask is None else ld(mask))


def _lin(X, cols, b, c0):
    """eta (longdouble) and its bound de = (m + 2) u (sum_a |x_ia b_a| + |c0|) (fp64)."""
    X64 = np.asarray(X, dtype=np.float64)
    n = X64.shape[0]
    cols = np.asarray(cols, dtype=int).reshape(-1)
    bl = ld(b).reshape(-1)
    XA = ld(X64[:, cols])
    eta = (XA @ bl if cols.size else np.zeros(n, dtype=LD)) + LD(c0)
    mag = (np.abs(XA) @ np.abs(bl) if cols.size else np.zeros(n, dtype=LD)) + abs(LD(c0))
    return eta, (cols.size + 2) * U * mag


def _logistic_row(eta, de, clamp):
    """pr, q = 1 - pr, their relative bounds rp, rq, and log pr, log q with their absolute bounds."""
    e = np.exp(np.clip(eta, LD(-clamp), LD(clamp)))
    re = de + 2 * U
    pr = e / (e + LD(1))
    q = LD(1) / (e + LD(1))  # 1 - pr without the cancellation: the reference value, not the kernels' formula
    rp = q * re + 2 * U
    rq = pr * re + 2 * U * pr / q + U
    lp, lq = np.log(pr), np.log(q)
    return {"pr": pr, "q": q, "rp": rp, "rq": rq, "lp": lp, "lq": lq, "dlp": rp + 2 * U * np.abs(lp),
            "dlq": rq + 2 * U * np.abs(lq)}


def _logistic_term(r, y, wl):
    """w (y log pr + (1 - y) log q) and its bound."""
    t = wl * (y * r["lp"] + (LD(1) - y) * r["lq"])
    dt = wl * (np.abs(y) * (r["dlp"] + U * np.abs(r["lp"])) + np.abs(LD(1) - y) * (r["dlq"] + U * np.abs(r["lq"])))
    return t, dt + 2 * U * np.abs(t)


def logfact(y):
    """sum_{j = 1 .. y} log j in longdouble, and the bound of the fp64 loop that forms it: (y + 2) u of the sum."""
    y = np.asarray(y, dtype=np.float64)
    top = int(y.max()) if y.size else 0
    cum = np.concatenate([[LD(0)], np.cumsum(np.log(ld(np.arange(1, top + 1))))]) if top >= 1 else np.zeros(1, dtype=LD)
    lf = cum[np.floor(np.maximum(y, 0)).astype(int)]
    return lf, (ld(y) + 2) * U * lf


def gh(family, X, y, w, mask, cols, b, coef0):
    """k_glm_eta_gh in longdouble: g, h, the summands t_all / t_test (zero outside their rows) and the sums loss_all /
    loss_test, each with its first-order bound at c = 1 (dg, dh, dt_all, dt_test; loss_all_bound, loss_test_bound)."""
    n = np.shape(X)[0]
    eta, de = _lin(X, cols, b, coef0)
    wl, ml = _wm(n, w, mask)
    yl = ld(y)
    test = (ml == 0) if mask is not None else np.zeros(n, dtype=bool)
    if family == LOGISTIC:
        r = _logistic_row(eta, de, CLAMP)
        g = wl * (yl - r["pr"]) * ml
        dg = wl * ml * (r["pr"] * r["rp"] + U * np.abs(yl - r["pr"])) + 2 * U * np.abs(g)
        h = wl * r["pr"] * r["q"] * ml
        dh = np.abs(h) * (r["rp"] + r["rq"] + 3 * U)
        t_all, dt_all = _logistic_term(r, yl, wl)
        t_te, dt_te = _logistic_term(_logistic_row(eta, de, CLAMP_TEST), yl, wl)
    else:
        e = np.exp(eta)
        re = de + 2 * U
        g = (yl - e) * wl * ml
        dg = wl * ml * (e * re + U * np.abs(yl - e)) + 2 * U * np.abs(g)
        h = e * wl * ml
        dh = np.abs(h) * (re + 2 * U)
        v = np.clip(eta, LD(-CLAMP), LD(CLAMP))
        ev = np.exp(v)
        lf, dlf = logfact(y)
        t_all = (yl * v - ev - lf) * wl
        dt_all = wl * (np.abs(yl) * de + ev * re + dlf + 2 * U * (np.abs(yl * v) + ev + lf)) + U * np.abs(t_all)
        t_te, dt_te = t_all, dt_all
    t_te, dt_te = np.where(test, t_te, LD(0)), np.where(test, dt_te, LD(0))
    out = {"family": family, "eta": eta, "de": de, "g": g, "dg": dg, "h": h, "dh": dh, "t_all": t_all, "dt_all": dt_all,
           "t_test": t_te, "dt_test": dt_te, "n": n}
    for k in ("all", "test"):
        t, dt = out["t_" + k], out["dt_" + k]
        out["loss_" + k] = t.sum()
        out["loss_%s_bound" % k] = float(dt.sum() + n * U * np.abs(t).sum())
    return out


def irls(family, X, y, w, mask, cols, bcur, t, wfloor):
    """One IRLS step's working weights and response in longdouble: W (before w and the mask), wv = W w m, z, the ll
    summands `term` and their sum ll, with the first-order bounds at c = 1 (dwv, dz, dterm, ll_bound); C = [1, X_A, z]."""
    X64 = np.asarray(X, dtype=np.float64)
    n = X64.shape[0]
    cols = np.asarray(cols, dtype=int).reshape(-1)
    bcur = np.asarray(bcur, dtype=np.float64).reshape(-1)
    assert bcur.size == cols.size + 1
    eta, de = _lin(X64, cols, bcur[1:], bcur[0])
    wl, ml = _wm(n, w, mask)
    yl = ld(y)
    if family == LOGISTIC:
        r = _logistic_row(eta, de, CLAMP)
        W = r["pr"] * r["q"]
        dW = W * (r["rp"] + r["rq"] + U)
        if t > 0 and wfloor:
            dW = np.where(W + dW < LD(FLOOR), LD(0), dW)
            W = np.maximum(W, LD(FLOOR))
        num = yl - r["pr"]
        dnum = r["pr"] * r["rp"] + U * np.abs(num)
        zeta = eta
        term, dterm = _logistic_term(r, yl, wl * ml)
        dterm = dterm + U * np.abs(term)
    else:
        if t == 0:
            zeta = eta
            W = np.exp(eta)
            dW = W * (de + 2 * U)
            term = dterm = np.zeros(n, dtype=LD)
        else:
            zeta = np.clip(eta, LD(-CLAMP), LD(CLAMP))
            W = np.exp(zeta)
            dW = W * (de + 2 * U)
            dW = np.where(W + dW < LD(FLOOR), LD(0), dW)
            W = np.maximum(W, LD(FLOOR))
            term = (yl * zeta - W) * wl * ml
            dterm = wl * ml * (np.abs(yl) * de + U * np.abs(yl * zeta) + dW + U * np.abs(yl * zeta - W)) + 2 * U * np.abs(term)
        num = yl - W
        dnum = dW + U * np.abs(num)
    ratio = num / W
    z = zeta + ratio
    dz = de + dnum / W + np.abs(ratio) * (dW / W + U) + U * np.abs(z)
    wv = W * wl * ml
    dwv = wl * ml * dW + 2 * U * wv
    C = np.concatenate([np.ones((n, 1), dtype=LD), ld(X64[:, cols]), z[:, None]], axis=1)
    return {"family": family, "eta": eta, "de": de, "W": W, "wv": wv, "dwv": dwv, "z": z, "dz": dz, "term": term,
            "dterm": dterm, "ll": term.sum(), "ll_bound": float(dterm.sum() + n * U * np.abs(term).sum()), "C": C, "n": n,
            "T0": int(cols.size)}


def gram(ref):
    """The step's Gram in longdouble, the weighted column norms |c_j|_Wv of xprec's bound, and what the per-row bounds of
    Wv and z carry into each entry at c = 1 (module docstring)."""
    C, wv = ref["C"], ref["wv"]
    G = C.T @ (wv[:, None] * C)
    aC = np.abs(C)
    norms = np.sqrt(np.einsum("ij,ij->j", C * wv[:, None], C).astype(np.float64))
    carried = (aC.T @ (ref["dwv"][:, None] * aC)).astype(np.float64)
    zc = (aC.T @ (wv * ref["dz"])).astype(np.float64)  # sum_i Wv_i |c_ij| dz_i
    last = C.shape[1] - 1
    carried[:last, last] += zc[:last]
    carried[last, :last] += zc[:last]
    carried[last, last] += 2 * zc[last] + float((wv * ref["dz"] * ref["dz"]).sum())
    return G, norms, carried


def next_iterate(ref, lam, rounds=4):
    """bnext of the reference Gram by mixed-precision refinement (fp64 solves, longdouble residuals) and cond_2 of the
    system (Gram_AA + 2 lam diag(0, 1, ..., 1))."""
    G = gram(ref)[0]
    m = ref["T0"] + 1
    A = G[:m, :m] + 2 * LD(lam) * np.diag(ld([0.0] + [1.0] * (m - 1)))
    q = G[:m, m]
    A64 = A.astype(np.float64)
    b = ld(np.linalg.solve(A64, q.astype(np.float64)))
    for _ in range(rounds):
        b = b + ld(np.linalg.solve(A64, (q - A @ b).astype(np.float64)))
    return b, xprec.cond(A64)


def scores(X, ref, cols, b, lam):
    """bd of get_A for all p columns in longdouble from the reference g, h, with the magnitude sums of the error model
    (dd, dl2 at c = 1: u M1 + sum_i |x_ij| dg_i and u M2 + sum_i x_ij^2 dh_i)."""
    X64 = np.asarray(X, dtype=np.float64)
    Xl = ld(X64)
    p = X64.shape[1]
    beta = np.zeros(p, dtype=LD)
    beta[np.asarray(cols, dtype=int).reshape(-1)] = ld(b).reshape(-1)
    d = Xl.T @ ref["g"] - 2 * LD(lam) * beta
    l2 = (Xl * Xl).T @ ref["h"] + 2 * LD(lam)
    aX = np.abs(Xl)
    dd = U * (aX.T @ np.abs(ref["g"]) + 2 * LD(lam) * np.abs(beta)) + aX.T @ ref["dg"]
    dl2 = U * ((Xl * Xl).T @ np.abs(ref["h"]) + 2 * LD(lam)) + (Xl * Xl).T @ ref["dh"]
    phi = np.sqrt(l2)
    t = phi * beta + d / phi
    return {"bd": t * t, "t": t, "phi": phi, "d": d, "l2": l2, "beta": beta, "dd": dd.astype(np.float64),
            "dl2": dl2.astype(np.float64)}


# ---- fp64 NumPy evaluating the kernels' formulas (the CPU stand-in, never the kernels) ------------------------------------
def _f64(n, w, mask):
    return (np.ones(n) if w is None else np.asarray(w, dtype=np.float64)), (np.ones(n) if mask is None else np.asarray(mask, dtype=np.float64))


def logfact_fp64(y):
    out = np.zeros(len(y))
    for i, yi in enumerate(np.asarray(y, dtype=np.float64)):
        t, j = 0.0, 1.0
        while j <= yi:
            t, j = t + np.log(j), j + 1.0
        out[i] = t
    return out


def gh_fp64(family, X, y, w, mask, cols, b, coef0, train_clamp=CLAMP, use_mask=True):
    """train_clamp / use_mask: the stand-in defects of tests/test_glm_reference.py."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    cols = np.asarray(cols, dtype=int).reshape(-1)
    y = np.asarray(y, dtype=np.float64)
    w, mk = _f64(n, w, mask)
    mm = mk if use_mask else np.ones(n)
    eta = (X[:, cols] @ np.asarray(b, dtype=np.float64).reshape(-1) if cols.size else np.zeros(n)) + coef0
    test = (mk == 0) if mask is not None else np.zeros(n, dtype=bool)
    if family == LOGISTIC:
        e = np.exp(np.clip(eta, -CLAMP, CLAMP))
        pr = e / (e + 1.0)
        g, h = w * (y - pr) * mm, w * pr * (1.0 - pr) * mm
        e1 = np.exp(np.clip(eta, -train_clamp, train_clamp))
        p1 = e1 / (e1 + 1.0)
        t_all = w * (y * np.log(p1) + (1.0 - y) * np.log(1.0 - p1))
        e2 = np.exp(np.clip(eta, -CLAMP_TEST, CLAMP_TEST))
        p2 = e2 / (e2 + 1.0)
        t_te = w * (y * np.log(p2) + (1.0 - y) * np.log(1.0 - p2))
    else:
        e = np.exp(eta)
        g, h = (y - e) * w * mm, e * w * mm
        v = np.clip(eta, -CLAMP, CLAMP)
        t_all = (y * v - np.exp(v) - logfact_fp64(y)) * w
        t_te = t_all
    return {"g": g, "h": h, "loss": np.array([t_all.sum(), t_te[test].sum()])}


def irls_fp64(family, X, y, w, mask, cols, bcur, t, wfloor, lam=0.0, floor_at_t0=False, use_mask=True, z_slot=None,
              drop_rows=None):
    """wv, z, ll, gram ((T0 + 2)^2) and bnext in fp64.  floor_at_t0, use_mask, z_slot (the working response written into
    Gram column z_slot of the padded tile instead of the last one) and drop_rows (row indices left out of the Gram) are
    the stand-in defects of tests/test_glm_reference.py."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    cols = np.asarray(cols, dtype=int).reshape(-1)
    y = np.asarray(y, dtype=np.float64)
    bcur = np.asarray(bcur, dtype=np.float64).reshape(-1)
    w, mk = _f64(n, w, mask)
    mm = mk if use_mask else np.ones(n)
    eta = X[:, cols] @ bcur[1:] + bcur[0]
    if family == LOGISTIC:
        e = np.exp(np.clip(eta, -CLAMP, CLAMP))
        Pi = e / (1.0 + e)
        term = (y * np.log(Pi) + (1.0 - y) * np.log(1.0 - Pi)) * w * mk
        W = Pi * (1.0 - Pi)
        if (t > 0 or floor_at_t0) and wfloor:
            W = np.where(W < FLOOR, FLOOR, W)
        z = eta + (y - Pi) / W
    else:
        if t == 0:
            e = np.exp(eta)
            if floor_at_t0:
                e = np.where(e < FLOOR, FLOOR, e)
            term = np.zeros(n)
        else:
            eta = np.clip(eta, -CLAMP, CLAMP)
            e = np.exp(eta)
            e = np.where(e < FLOOR, FLOOR, e)
            term = (y * eta - e) * w * mk
        W = e
        z = eta + (y - e) / e
    wv = W * w * mm
    T0 = cols.size
    mp = (T0 + 2 + 15) // 16 * 16
    P = np.zeros((n, mp))  # the padded tile: [1, X_A, zero columns ..., z]
    P[:, 0] = 1.0
    P[:, 1:T0 + 1] = X[:, cols]
    P[:, mp - 1 if z_slot is None else z_slot] = z
    keep = np.ones(n, dtype=bool)
    if drop_rows is not None:
        keep[np.asarray(drop_rows, dtype=int)] = False
    Gp = P[keep].T @ (wv[keep, None] * P[keep])
    idx = list(range(T0 + 1)) + [mp - 1]
    G = Gp[np.ix_(idx, idx)]
    m = T0 + 1
    A = G[:m, :m] + 2 * lam * np.diag([0.0] + [1.0] * (m - 1))
    with np.errstate(all="ignore"):
        try:
            bnext = np.linalg.solve(A, G[:m, m])
        except np.linalg.LinAlgError:
            bnext = np.full(m, np.nan)
    return {"wv": wv, "z": z, "ll": term.sum(), "gram": G, "bnext": bnext}


def scores_fp64(X, g, h, cols, b, lam):
    X = np.asarray(X, dtype=np.float64)
    beta = np.zeros(X.shape[1])
    beta[np.asarray(cols, dtype=int).reshape(-1)] = np.asarray(b, dtype=np.float64).reshape(-1)
    d = X.T @ g - 2 * lam * beta
    phi = np.sqrt((X * X).T @ h + 2 * lam)
    t = phi * beta + (1.0 / phi) * d
    return t * t


# ---- the assertion helpers: one per quantity, each returns the fraction of its bound that was used ----------------------------
def _frac(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))


def row_units(got, want, bound1):
    """max_i |got_i - want_i| / (the first-order bound at c = 1), and the row."""
    got = np.asarray(got, dtype=np.float64)
    f = _frac(np.abs(ld(got) - want), bound1)
    f = np.where(np.isfinite(got), f, np.inf)
    i = int(np.argmax(f)) if f.size else 0
    return (float(f[i]) if f.size else 0.0), i


def _assert_rows(got, ref, key, dkey, what):
    r, i = row_units(got, ref[key], ref[dkey])
    c = ROW_C[key]
    print("%s: %s at %.3f of its bound (c = %.3f of %g, row %d, eta %.3f)" % (what, key, r / c, r, c, i, float(ref["eta"][i])))
    assert r <= c, (what, key, i, float(np.asarray(got)[i]), float(ref[key][i]), r, c)
    return r / c


def assert_g_close(g, ref, what):
    return _assert_rows(g, ref, "g", "dg", what)


def assert_h_close(h, ref, what):
    return _assert_rows(h, ref, "h", "dh", what)


def assert_wv_close(wv, ref, what):
    return _assert_rows(wv, ref, "wv", "dwv", what)


def assert_z_close(z, ref, what):
    return _assert_rows(z, ref, "z", "dz", what)


def sum_units(got, want, bound1):
    return float(_frac(abs(LD(got) - want), bound1)) if np.isfinite(got) else np.inf


def _assert_sum(got, want, bound1, what):
    r = sum_units(got, want, bound1)
    print("%s: %.17g at %.3f of its bound (c = %.3f of %g)" % (what, float(got), r / SUM_C, r, SUM_C))
    assert r <= SUM_C, (what, float(got), float(want), r, SUM_C, bound1)
    return r / SUM_C


def assert_loss_close(loss, ref, what, test=False):
    k = "test" if test else "all"
    return _assert_sum(loss, ref["loss_" + k], ref["loss_%s_bound" % k], what + (" held-out loss" if test else " loss"))


def assert_ll_close(ll, ref, what):
    return _assert_sum(ll, ref["ll"], ref["ll_bound"], what + " ll")


def assert_gram_close(G, ref, what, against=None, factor=1.0):
    """Every entry of the (T0 + 2)^2 Gram within xprec.assert_gram_close's bound (weighted column norms) plus what Wv and z
    carry into it, of the reference (or of `against`, another result on the same input, with `factor` times the bound)."""
    Gr, norms, carried = gram(ref)
    G = np.asarray(G, dtype=np.float64)
    assert G.shape == Gr.shape and np.isfinite(G).all(), (what, G.shape)
    f = xprec.assert_gram_close(G, Gr if against is None else against, norms, norms, ref["n"], what,
                                extra=max(ROW_C["wv"], ROW_C["z"]) * carried, scale=factor)
    print("%s: Gram at %.3f of its bound" % (what, f))
    return f


# a bound of 4e-13 cond |b*| says something about the solve only while cond is small: the cases that are there to test the
# solve must stay under this (4e-9 |b*|); beside a saturated Poisson row at e^30 cond is 1e13 to 1e15 and bnext is not compared
COND_LIMIT = 1e4


def assert_bnext_close(b, ref, lam, what):
    """xprec.assert_fit_close with the condition number of the reference system, which has to be under COND_LIMIT."""
    br, cond = next_iterate(ref, lam)
    assert cond <= COND_LIMIT, (what, "the system is too ill-conditioned for its bound to test the solve", cond)
    assert np.isfinite(np.asarray(b)).all(), what
    f = xprec.assert_fit_close(b, br, cond, what + " bnext")
    print("%s: bnext at %.3f of its bound (cond %.3g)" % (what, f, cond))
    return f


def score_units(bd, sref):
    """max_j |bd_j - bd*_j| / (the forward-error model at c = 1), and the column."""
    phi, t = sref["phi"].astype(np.float64), np.abs(sref["t"].astype(np.float64))
    beta, d = np.abs(sref["beta"].astype(np.float64)), np.abs(sref["d"].astype(np.float64))
    dphi = sref["dl2"] / (2 * phi)
    dt = beta * dphi + sref["dd"] / phi + d * dphi / (phi * phi)
    allowed = 2 * t * dt + dt * dt + 4 * U * t * t
    bd = np.asarray(bd, dtype=np.float64)
    f = _frac(np.abs(ld(bd) - sref["bd"]), allowed)
    f = np.where(np.isfinite(bd), f, np.inf)
    j = int(np.argmax(f))
    return float(f[j]), j


def assert_scores_close(bd, sref, what):
    r, j = score_units(bd, sref)
    print("%s: bd at %.3f of its bound (c = %.3f of %g, column %d)" % (what, r / SCORE_C, r, SCORE_C, j))
    assert r <= SCORE_C, (what, j, float(np.asarray(bd)[j]), float(sref["bd"][j]), r, SCORE_C)
    return r / SCORE_C


# ---- seeded cases, one place for both files -----------------------------------------------------------------------------------
REGIMES = {"mild": 3.0, "wide": 12.0, "saturating": 12.0}
TARGETS = (40.0, -40.0, 30.1, -30.1, 29.9, -29.9, 25.1, -25.1, 24.9, -24.9)
TEMPLATE_T0 = (1, 14, 15, 30, 31, 46, 62, 78, 94, 110, 126)  # T0 + 2 on and just past every tile-row edge, mt = 1 .. 8
TEMPLATE_N = (1, 2, 63, 65, 129, 1025)
NCH_OF_MT = {1: 8, 2: 8, 3: 8, 4: 6, 5: 5, 6: 4, 7: 3, 8: 2}  # chunks per group of k_irls_gram's instances
SLAB_T0 = ((8, 14), (8, 46), (6, 62), (5, 78), (4, 94), (3, 110), (2, 126))
GH_N, GH_M = (1, 255, 257, 1025), (0, 1, 17)
# part (b) runs in two regimes: "saturating" puts the clamped rows on the chunk and slab edges; in "mild" every row pair
# carries a visible share of every Gram entry (beside a Poisson row at e^30 a dropped row pair is below the rounding)
SLAB_REGIMES = ("saturating", "mild")
# where bnext is compared: systems whose condition number stays under COND_LIMIT -- these for both families, and the
# saturating cases of part (c) for logistic (W <= 1 / 4 whatever eta is)
SOLVE_CASES = ((14, 129, "mild"), (30, 1025, "mild"), (30, 1025, "wide"), (127, 1025, "mild"))


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def special_rows(n, slab_rows=64):
    """Where the saturating regime puts its rows: the last row, the last row of a 64-row chunk, the first row of a slab
    (and the one before it), then the first rows -- as many as fit, each once."""
    want = [n - 1, 63, slab_rows, slab_rows - 1, 64, 0, 1, 2, 3, 4, 5, 6]
    rows = []
    for r in want:
        if 0 <= r < n and r not in rows:
            rows.append(r)
    return rows[:len(TARGETS)]


def _place(X, col, coef, eta, rows):
    """Move X[rows, col] so that eta (= ... + X[:, col] coef) takes the values of TARGETS on `rows`."""
    for r, target in zip(rows, TARGETS):
        X[r, col] += (target - eta[r]) / coef


def _response(family, eta, rng, rows):
    n = eta.size
    if family == LOGISTIC:
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-np.clip(eta, -30, 30)))).astype(np.float64)
        y[rows] = np.arange(len(rows)) % 2  # both outcomes on the saturated rows, whatever their sign
        if n > 1 and y.min() == y.max():
            y[0] = 1.0 - y[0]
    else:
        y = rng.poisson(np.exp(np.clip(eta, -3.0, 3.5))).astype(np.float64)
        if n > 2:
            y[n // 2], y[n // 3] = 61.0, 0.0
        if n > 5:
            y[n // 5] = 75.0
    return y


def _weights(n, rng):
    w = rng.uniform(0.5, 2.0, n)
    if n > 3:
        w[2::7] = 0.0
        w[n - 2] = w[n - 2] or 1.25  # (the last row pair carries weight: a dropped pair shows)
    return w


def _fold(n, rng):
    mk = (rng.uniform(size=n) >= 0.2).astype(np.float64)
    mk[0] = 1.0
    if n > 1:
        mk[n - 1] = 0.0
    if n > 2:
        mk[n - 2] = 1.0  # (the last row pair is not all test rows: a dropped pair shows)
    return mk


def irls_case(family, T0, n, regime, weighted=True, masked=True, slab_rows=64):
    """(X, y, w, mask, cols, bcur): a seeded design with p = T0 + 3 columns, cols a shuffled subset of T0 of them, an
    iterate whose linear predictor stays inside the regime's limit, and for "saturating" the rows of special_rows() moved
    to |eta| = 40, 30.1, 29.9, 25.1, 24.9 in both signs."""
    rng = _rng(family, T0, n, sorted(REGIMES).index(regime), int(weighted), int(masked))
    p = T0 + 3
    X = rng.standard_normal((n, p))
    cols = rng.permutation(p)[:T0].astype(np.int32)
    b = np.concatenate([[rng.uniform(-0.3, 0.3)], rng.uniform(0.5, 1.0, T0) * rng.choice([-1.0, 1.0], T0)])
    raw = X[:, cols] @ b[1:]
    b[1:] *= 0.95 * (REGIMES[regime] - 0.3) / max(np.abs(raw).max(), 1e-30)
    rows = []
    if regime == "saturating":
        rows = special_rows(n, slab_rows)
        _place(X, cols[0], b[1], X[:, cols] @ b[1:] + b[0], rows)
    eta = X[:, cols] @ b[1:] + b[0]
    y = _response(family, eta, rng, rows)
    return X, y, (_weights(n, rng) if weighted else None), (_fold(n, rng) if masked else None), cols, b


def gh_case(family, n, m, regime, weighted=True, masked=True):
    """(X, y, w, mask, cols, b, coef0) for op_glm_gh: p = 20 columns, m of them in the model (m = 0: the intercept alone)."""
    rng = _rng(family, n, m, sorted(REGIMES).index(regime), int(weighted), int(masked), 77)
    p = 20
    X = rng.standard_normal((n, p))
    cols = np.sort(rng.permutation(p)[:m]).astype(np.int32)
    b = rng.uniform(0.5, 1.0, m) * rng.choice([-1.0, 1.0], m)
    lim = REGIMES[regime]
    coef0 = float(rng.uniform(-0.3, 0.3)) if m else {"mild": 0.7, "wide": -9.5, "saturating": 30.1}[regime]
    rows = []
    if m:
        b *= 0.95 * (lim - 0.3) / max(np.abs(X[:, cols] @ b).max(), 1e-30)
        if regime == "saturating":
            rows = special_rows(n)
            _place(X, cols[0], b[0], X[:, cols] @ b + coef0, rows)
    eta = (X[:, cols] @ b if m else np.zeros(n)) + coef0
    y = _response(family, eta, rng, rows)
    return X, y, (_weights(n, rng) if weighted else None), (_fold(n, rng) if masked else None), cols, b, coef0


def template_cases():
    """(family, T0, n, regime, t, wfloor, weighted, masked) of part (a): every T0 of TEMPLATE_T0 at two row counts that
    walk through TEMPLATE_N, both families; t, wfloor, weights and mask alternate so that every value meets every tile-row
    edge, and T0 = 14 / 15 (the z column directly behind / one tile row past the last active column) take every n."""
    out = []
    for family in (LOGISTIC, POISSON):
        for k, T0 in enumerate(TEMPLATE_T0):
            ns = TEMPLATE_N if T0 in (14, 15) else (TEMPLATE_N[k % 6], TEMPLATE_N[(k + 3) % 6])
            for j, n in enumerate(ns):
                q = k + j
                regime = ("mild", "wide", "saturating")[q % 3]
                out.append((family, T0, n, regime, q % 2, (q // 2) % 2, q % 3 != 1, q % 4 < 2))
    return out


def slab_case_n(nch):
    """Row counts for rows_per_slab = (nch + 1) * 64: the first slab is a full group of nch chunks and a one-chunk group,
    the last slab is short and its last chunk ragged (12 data rows)."""
    return (nch + 1) * 64 + 12


def all_irls_cases():
    """name -> (family, (X, y, w, mask, cols, bcur), t, wfloor, lam) over everything the GPU file runs through op_glm_irls
    at op level (the production-geometry case n = 16400 included)."""
    out = {}
    for family, T0, n, regime, t, wfloor, weighted, masked in template_cases():
        out["a fam%d T0=%d n=%d %s t=%d floor=%d w=%d m=%d" % (family, T0, n, regime, t, wfloor, weighted, masked)] = (
            family, irls_case(family, T0, n, regime, weighted, masked), t, wfloor, 0.0)
    for family in (LOGISTIC, POISSON):
        for nch, T0 in SLAB_T0:
            rows = (nch + 1) * 64
            for n in ((slab_case_n(nch),) + ((1100,) if (nch, T0) == (8, 14) else ())):
                for regime in SLAB_REGIMES:
                    out["b fam%d T0=%d n=%d rows=%d %s" % (family, T0, n, rows, regime)] = (
                        family, irls_case(family, T0, n, regime, True, True, slab_rows=rows), 1, 1, 0.0)
        out["b fam%d T0=14 n=16400" % family] = (family, irls_case(family, 14, 16400, "saturating", True, True, slab_rows=128), 1, 1, 0.0)
        for T0, n in ((14, 129), (30, 1025), (127, 1025)):
            for t, wfloor in ((0, 1), (1, 1), (1, 0)):
                out["c fam%d T0=%d n=%d t=%d floor=%d" % (family, T0, n, t, wfloor)] = (
                    family, irls_case(family, T0, n, "saturating", True, True), t, wfloor, 0.05)
        for T0, n, regime in SOLVE_CASES:
            for t in (0, 1):
                out["s fam%d T0=%d n=%d %s t=%d" % (family, T0, n, regime, t)] = (
                    family, irls_case(family, T0, n, regime, True, True), t, 1, 0.05)
    return out


def all_gh_cases():
    """name -> (family, (X, y, w, mask, cols, b, coef0), lam) of part (d)."""
    out = {}
    for family in (LOGISTIC, POISSON):
        for n in GH_N:
            for m in GH_M:
                for k, regime in enumerate(("mild", "wide", "saturating")):
                    weighted, masked = (n + m + k) % 2 == 0, (n + m + k) % 3 != 0
                    out["d fam%d n=%d m=%d %s w=%d m=%d" % (family, n, m, regime, weighted, masked)] = (
                        family, gh_case(family, n, m, regime, weighted, masked), 0.05 if k else 0.0)
    return out


def wide_design(family, n=600, p=40, seed=9):
    """A design whose fitted linear predictor spans more than 6 units (column 0 carries outliers and signal), for Session.fit."""
    rng = _rng(seed, family)
    X = rng.standard_normal((n, p))
    X[::25, 0] *= 6.0
    if family == LOGISTIC:
        eta = 1.2 * X[:, 0] + 0.8 * X[:, 1] - 0.8 * X[:, 2]
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        eta = 0.3 * X[:, 0] + 0.3 * X[:, 1] - 0.3 * X[:, 2] + 0.5
        y = rng.poisson(np.exp(np.clip(eta, -10, 5))).astype(np.float64)
    return X, y
