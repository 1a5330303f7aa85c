"""Extended-precision reference for the marginal-fit scores of sure independence screening (the kernels k_screen_* of
bessx_k_glm.hip, the sub-session route of wide groups and the device-matrix route, all read back through
Session.screening_scores()): pure NumPy in np.longdouble, no GPU, no oracle.  It restates the OPERATIONS of the modelled
project (screening(), src/screening.cpp:26-105; logit_fit, src/logistic.cpp:60-160; cox_fit and loglik_cox,
src/coxph.cpp:16-109), not the kernels.  Everything runs on the raw data: uncentred, before normalisation.

  unit       one original column, or one original group of s columns X_g (n x s).  score = |b|^2 / s over the
             NON-intercept coefficients b of the unit's marginal fit (coef_norm, src/screening.cpp:60).
  LM         b = the least-squares coefficients of y on X_g (one column: x.y / x.x).  The weight does not enter: the
             modelled project solves against the raw y (src/screening.cpp:46) and the session hands the kernels ones.
  logistic   IRLS on V = [1, X_g] from zero.  eta = V b;  Pi = 1 / (1 + exp(-clamp(eta, 30)));  ll(b) = sum_i w_i (y_i log Pi_i
             + (1 - y_i) log(1 - Pi_i));  a solve is b' = (V^T W V)^-1 V^T W z with W0 = Pi (1 - Pi) (no floor), z = eta +
             (y - Pi) / W0 (eta NOT clamped here), W = W0 w.  b0 = 0, b1 = solve(b0); then at most 30 times: ll1 = ll(b1); stop
             when |ll0 - ll1| / (0.1 + |ll1|) < 1e-6; else b0 = b1, ll0 = ll1, b1 = solve(b0).  The result is b0: the iterate
             BEFORE the last solve.
  Cox        damped Newton from zero, ll0 = 1e5 (so the first step is always halved down to 1/32).  Rows are in time
             order.  At b0: theta = exp(clamp(X_g b0, 50)), S0_i = sum_{l >= i} theta_l, S1_u(i) = sum_{l >= i} theta_l x_lu,
             S2_uv(i) likewise; g_u = sum_i w_i d_i (x_iu - S1_u(i) / S0_i), I_uv = sum_i w_i d_i (S2_uv(i) / S0_i - S1_u S1_v /
             S0_i^2) (d = status; the weight is NOT in the risk-set sums); direction D = I^-1 g; b1 = b0 + 2^-m D, m = 1, raised
             while ll0 > ll(b1) and m < 5, with ll(b) = sum_i w_i d_i log(e_i / sum_{l >= i} e_l), e = exp(clamp(X_g b, 30)).
             Stop when |ll0 - ll1| / |0.1 + ll0| < 1e-5, at most 30 steps; else b0 = b1, ll0 = ll1.  The result is b0: the
             iterate BEFORE the last step.
  special    a non-finite result scores 0.0 (an all-zero or all-ones column of logistic / Cox: a singular system), except
             an all-zero LM column, which scores +inf; an always_select unit scores DBL_MAX.  (The modelled project's
             pivoted LDL^T sets the coefficient of a zero pivot to 0, src/logistic.cpp:130, so its all-ones column has
             the slope 0 and the same score 0.0; its Cox direction there is 0 / 0 like here.)

Discrete decisions.  The iterate depends on how many steps were taken, so every fit records `margin`: the smallest
relative distance |ratio - thr| / thr over its stopping decisions, and |ll0 - ll1| / max(|ll0|, |ll1|) over its halving
decisions whose outcome is kept (a halving decision that is followed at once by the stop discards b1 and needs none).  A
unit with margin < MARGIN is UNDECIDED: counted, not compared.

Forward-error model, in coefficient space (after coxsolveref's for the sacrifice scores):
    |b - b*| <= C u (|b*| + |H*^-1| M_g)        coefficient by coefficient
at the returned iterate, with M_g the gradient-side sums with every elementary product replaced by its absolute value and
|H*^-1| the inverse information with every entry replaced by its absolute value (1 / h for one column; entry by entry,
not a matrix norm, so that the bound does not depend on the units of the columns):
    LM        H = X_g^T X_g,                     M_g,u = sum_i |x_iu| (|y_i| + sum_v |x_iv| |b_v|)
    logistic  H = V^T W V (intercept included),  M_g,a = sum_i W_i |v_ia| (|z_i| + sum_c |v_ic| |b_c|)
    Cox       H = I,                             M_g,u = sum_i w_i d_i (|x_iu| + B1_u(i) / S0_i + A1_u(i) B0(i) / S0_i^2),  A1, B1, B0 =
              suffix sums of theta |x_u|, theta (1 + |eta|) |x_u|, theta (1 + |eta|): the quotient S1 / S0 with the relative
              error (1 + |eta_l|) u that the product x b and exp leave in every theta_l
(the logistic intercept is a coefficient of H and M_g: its error feeds the slopes).  With Db_u that bound, the score
|b|^2 / s moves by at most sum_u (2 |b_u| Db_u + Db_u^2) / s over the non-intercept coefficients: `unit_bound` at C = 1.
A unit whose bound at the family's constant exceeds ILL_REL x its score is ILL-CONDITIONED: counted, not compared (in
these cases only Cox noise columns: without an intercept a column of mean +-2 and scale 0.3 cancels in x - S1 / S0).
The model is first order and speaks of the last solve alone; what earlier iterates carry into it, and the steps that a
far outlier makes the damped Newton iteration take (column C_TAIL), are left to the measured constant.

The constants.  fp64 NumPy evaluating the same formulas (dtype = np.float64: the CPU stand-in, never the kernels) against
this reference over every case below; tests/test_screen_reference.py re-measures the maxima and asserts that the
constants are 4 x the maximum rounded up to a power of two (the factor four allows for a different but equally valid
order of summation, as for coxsolveref.SCORE_C).

The module also holds the seeded cases both test files use and the assert_* helpers, one per bound."""
import numpy as np

import xprec

LD, U, EXTENDED = xprec.LD, xprec.U, xprec.EXTENDED
DBL_MAX = float(np.finfo(np.float64).max)
MARGIN = 1e-6    # a discrete decision closer than this to its threshold is not held against the kernels
ILL_REL = 1e-10  # no compared unit has a bound above this, relative to its score

# largest |score - score*| / unit_bound of the fp64 stand-in over all_cases(family); measured and re-derived by
# tests/test_screen_reference.py::test_constants_are_the_rule_applied_to_the_measured_maxima
SCREEN_C_LM_NUMPY_MAX = 1.5717     # lm-single-n513-plain-gauss, column 1
SCREEN_C_LOGIT_NUMPY_MAX = 5.6779  # logistic-single-n1000-plain-rare, column 18
SCREEN_C_COX_NUMPY_MAX = 5.9962    # cox-single-n1000-plain-cens30, column 14 (the outlier column)
SCREEN_C_LM = 8.0      # 4 x 1.5717 = 6.3, rounded up to a power of two
SCREEN_C_LOGIT = 32.0  # 4 x 5.6779 = 22.7
SCREEN_C_COX = 32.0    # 4 x 5.9962 = 24.0


def constant_rule(measured_max):
    """4 x the measured maximum, rounded up to a power of two."""
    return float(2.0 ** np.ceil(np.log2(4.0 * measured_max)))


# ---- small dense algebra in any NumPy float type (np.linalg has no longdouble) -----------------------------------------
def solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting.  A singular system gives non-finite entries, not an error."""
    A, b = np.array(A), np.array(b)
    m = b.size
    with np.errstate(all="ignore"):
        for k in range(m):
            col = np.abs(A[k:, k])
            piv = k + (int(np.argmax(col)) if np.all(np.isfinite(col)) else 0)
            if piv != k:
                A[[k, piv]] = A[[piv, k]]
                b[[k, piv]] = b[[piv, k]]
            for i in range(k + 1, m):
                f = A[i, k] / A[k, k]
                A[i, k:] = A[i, k:] - f * A[k, k:]
                b[i] = b[i] - f * b[k]
        x = np.zeros(m, dtype=A.dtype)
        for k in range(m - 1, -1, -1):
            x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def abs_inverse(H):
    """|H^-1| entry by entry (float64 is enough for a factor of the bound); inf for a singular or non-finite H."""
    H = np.asarray(H, dtype=np.float64)
    try:
        if not np.all(np.isfinite(H)):
            raise np.linalg.LinAlgError
        return np.abs(np.linalg.inv(H))
    except np.linalg.LinAlgError:
        return np.full(H.shape, np.inf)


def coefficient_bound(b, H, Mg):
    """U x (|b*| + |H*^-1| M_g), coefficient by coefficient."""
    with np.errstate(all="ignore"):
        return U * (np.abs(np.asarray(b, dtype=np.float64)) + abs_inverse(H) @ np.asarray(Mg, dtype=np.float64))


def suffix(v, restart=None):
    """Suffix sums over the rows (axis 0), accumulated from the last row.  restart = R is the deliberately wrong form
    that forgets what it has summed every R rows counted from the last (a dropped carry between row steps)."""
    r = v[::-1]
    if restart is None:
        return np.cumsum(r, axis=0)[::-1]
    out = np.concatenate([np.cumsum(r[a:a + restart], axis=0) for a in range(0, r.shape[0], restart)], axis=0)
    return out[::-1]


def _clamp(v, c):
    return np.minimum(np.maximum(v, -c), c)


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), np.finfo(np.float64).tiny)


# ---- the marginal fits -------------------------------------------------------------------------------------------------
def _finish(fit, b, Db, s):
    """score and unit_bound (the bound at C = 1) from the non-intercept coefficients and their coefficient_bound."""
    with np.errstate(all="ignore"):
        sc = np.sum(b * b) / s
        ub = float(np.sum(2 * np.abs(b.astype(np.float64)) * Db + Db * Db) / s)
    fit["b"] = b
    fit["finite"] = bool(np.isfinite(sc))
    fit["score"] = sc if fit["finite"] else sc.dtype.type(0.0)
    fit["unit_bound"] = ub if fit["finite"] else 0.0
    return fit


def lm_fit(Xg, y, dtype=LD):
    Xg, y = np.asarray(Xg, dtype=dtype), np.asarray(y, dtype=dtype)
    s = Xg.shape[1]
    H, t = Xg.T @ Xg, Xg.T @ y
    if s == 1 and H[0, 0] == 0:
        return {"b": np.full(1, np.inf), "finite": False, "score": dtype(np.inf), "unit_bound": 0.0, "steps": 0,
                "margin": np.inf}
    b = solve(H, t)
    A = np.abs(Xg)
    Mg = A.T @ (np.abs(y) + A @ np.abs(b))
    return _finish({"steps": 0, "margin": np.inf}, b, coefficient_bound(b, H, Mg), s)


def logit_fit(Xg, y, w, dtype=LD, after_last=False, force_stop=None):
    """after_last: the deliberately wrong result b1.  force_stop = k: ignore the rule and stop at the k-th decision."""
    Xg, y, w = np.asarray(Xg, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(w, dtype=dtype)
    n, s = Xg.shape
    V = np.concatenate([np.ones((n, 1), dtype=dtype), Xg], axis=1)
    one = dtype(1.0)

    def parts(b):
        eta = V @ b
        e = np.exp(_clamp(eta, dtype(30.0)))
        Pi = e / (one + e)
        ll = np.sum((y * np.log(Pi) + (one - y) * np.log(one - Pi)) * w)
        W0 = Pi * (one - Pi)
        z = eta + (y - Pi) / W0
        return ll, W0 * w, z

    def step(W, z):
        VW = V * W[:, None]
        return solve(VW.T @ V, VW.T @ z)

    with np.errstate(all="ignore"):
        b0 = np.zeros(s + 1, dtype=dtype)
        ll0, W, z = parts(b0)
        b1 = step(W, z)
        margin, steps = np.inf, 0
        for j in range(30):
            ll1, W1, z1 = parts(b1)
            ratio = abs(ll0 - ll1) / (dtype(0.1) + abs(ll1))
            steps = j + 1
            stop = bool(ratio < 1e-6) if force_stop is None else steps == force_stop
            if np.isfinite(ratio):
                margin = min(margin, float(abs(ratio - dtype(1e-6)) / dtype(1e-6)))
            if stop:
                break
            b0, ll0, W, z = b1, ll1, W1, z1
            b1 = step(W, z)
        # the model at the returned iterate: the solve that produced it used (W, z) of the iterate before; the sums at the
        # iterate itself have the same magnitudes and need no second bookkeeping
        _, Wb, zb = parts(b0)
        A = np.abs(V)
        Mg = (A * Wb[:, None]).T @ (np.abs(zb) + A @ np.abs(b0))
        H = (V * Wb[:, None]).T @ V
        Db = coefficient_bound(b0, H, Mg)[1:]
    res = b1 if after_last else b0
    return _finish({"steps": steps, "margin": margin}, res[1:], Db, s)


def cox_fit(Xg, status, w, dtype=LD, newton_clamp=50.0, weight_in_risk=False, after_last=False, restart=None,
            force_stop=None):
    """newton_clamp = 30, weight_in_risk, after_last and restart = 256 are the deliberately wrong forms the CPU test holds
    the bounds against.  force_stop = k: ignore the rule and stop at the k-th decision."""
    Xg, d, w = np.asarray(Xg, dtype=dtype), np.asarray(status, dtype=dtype), np.asarray(w, dtype=dtype)
    n, s = Xg.shape
    wd = w * d
    rw = w if weight_in_risk else np.ones(n, dtype=dtype)

    def newton(b):
        eta = _clamp(Xg @ b, dtype(newton_clamp))
        th = np.exp(eta) * rw
        S0 = suffix(th, restart)
        q1 = suffix(Xg * th[:, None], restart) / S0[:, None]
        g = (Xg - q1).T @ wd
        I = np.zeros((s, s), dtype=dtype)
        for u in range(s):
            for v in range(u + 1):
                S2 = suffix(th * Xg[:, u] * Xg[:, v], restart)
                I[u, v] = I[v, u] = np.sum((S2 / S0 - q1[:, u] * q1[:, v]) * wd)
        # M_g: theta_l carries the relative error (1 + |eta_l|) u of its argument and of exp into both risk-set sums
        te = th * (1 + np.abs(eta))
        A1 = suffix(np.abs(Xg) * th[:, None], restart) / S0[:, None]
        B1 = suffix(np.abs(Xg) * te[:, None], restart) / S0[:, None]
        Mg = (np.abs(Xg) + B1 + A1 * (suffix(te, restart) / S0)[:, None]).T @ wd
        return g, I, Mg

    def loglik(b):
        e = np.exp(_clamp(Xg @ b, dtype(30.0)))
        return np.sum(np.log(e / suffix(e * rw, restart)) * wd)

    with np.errstate(all="ignore"):
        b0, b1 = np.zeros(s, dtype=dtype), np.zeros(s, dtype=dtype)
        ll0 = dtype(1e5)
        margin, steps = np.inf, 0
        for l in range(1, 31):
            g, I, _ = newton(b0)
            D = solve(I, g)
            m = 1
            b1 = b0 + dtype(0.5) * D
            ll1 = loglik(b1)
            halvings = []
            while True:
                if np.isfinite(ll1):
                    halvings.append(_rel(ll0, ll1))
                if not (ll0 > ll1 and m < 5):
                    break
                m += 1
                b1 = b0 + dtype(0.5) ** m * D
                ll1 = loglik(b1)
            if m == 5 and halvings:
                halvings.pop()  # (the fifth comparison decides nothing: m < 5 ends the loop either way)
            ratio = abs(ll0 - ll1) / abs(dtype(0.1) + ll0)
            steps = l
            stop = bool(ratio < 1e-5) if force_stop is None else steps == force_stop
            if np.isfinite(ratio):
                margin = min(margin, float(abs(ratio - dtype(1e-5)) / dtype(1e-5)))
            if stop:
                break
            if halvings:
                margin = min(margin, float(min(halvings)))
            b0, ll0 = b1, ll1
        _, Ib, Mg = newton(b0)
        Db = coefficient_bound(b0, Ib, Mg)
    return _finish({"steps": steps, "margin": margin}, b1 if after_last else b0, Db, s)


FAMILY_C = {"lm": lambda: SCREEN_C_LM, "logistic": lambda: SCREEN_C_LOGIT, "cox": lambda: SCREEN_C_COX}
MODEL_TYPE = {"lm": 1, "logistic": 2, "cox": 4}


def unit_slices(p, g_index):
    if g_index is None:
        return [slice(j, j + 1) for j in range(p)]
    gi = list(g_index) + [p]
    return [slice(gi[g], gi[g + 1]) for g in range(len(gi) - 1)]


def reference(case, dtype=LD, **wrong):
    """Every unit of a case fitted in `dtype`: dict of arrays over the units (score, unit_bound, margin, steps, finite,
    always).  **wrong goes to the family's fit (the deliberately wrong forms)."""
    X, y, fam = case["X"], case["y"], case["family"]
    n, p = X.shape
    w = np.ones(n) if case["weight"] is None else case["weight"]
    units = unit_slices(p, case["g_index"])
    out = {k: [] for k in ("score", "unit_bound", "margin", "steps", "finite")}
    for u, sl in enumerate(units):
        if u in case["always"]:
            f = {"score": DBL_MAX, "unit_bound": 0.0, "margin": np.inf, "steps": 0, "finite": True}
        elif fam == "lm":
            f = lm_fit(X[:, sl], y, dtype)
        elif fam == "logistic":
            f = logit_fit(X[:, sl], y, w, dtype, **wrong)
        else:
            f = cox_fit(X[:, sl], y, w, dtype, **wrong)
        for k in out:
            out[k].append(f[k])
    ref = {"score": np.array(out["score"], dtype=dtype), "unit_bound": np.array(out["unit_bound"], dtype=np.float64),
           "margin": np.array(out["margin"], dtype=np.float64), "steps": np.array(out["steps"]),
           "finite": np.array(out["finite"]), "family": fam, "name": case["name"]}
    ref["always"] = np.isin(np.arange(len(units)), case["always"])
    return ref


# ---- who is compared, and the bounds -------------------------------------------------------------------------------------
def undecided(ref):
    return ref["finite"] & ~ref["always"] & (ref["margin"] < MARGIN)


def ill_conditioned(ref, c=None):
    c = FAMILY_C[ref["family"]]() if c is None else c
    sc = ref["score"].astype(np.float64)
    with np.errstate(all="ignore"):
        return ref["finite"] & ~ref["always"] & np.isfinite(sc) & (c * ref["unit_bound"] > ILL_REL * sc)


def compared(ref, c=None):
    """The units held to the forward-error model: finite, not always_select, decided and well-conditioned."""
    sc = ref["score"].astype(np.float64)
    return ref["finite"] & ~ref["always"] & np.isfinite(sc) & ~undecided(ref) & ~ill_conditioned(ref, c)


def score_error_units(scores, ref, c=None):
    """max |score - score*| / unit_bound over the compared units.  Returns (ratio, unit); (0, -1) when none is compared."""
    keep = compared(ref, c)
    if not keep.any():
        return 0.0, -1
    got = np.asarray(scores, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.abs((got.astype(LD) - ref["score"].astype(LD)).astype(np.float64))
        ratio = err / np.maximum(ref["unit_bound"], 1e-300)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    ratio = np.where(keep, ratio, 0.0)
    j = int(np.argmax(ratio))
    return float(ratio[j]), j


def assert_scores_close(scores, ref, what, c=None):
    """|score - score*| <= C x unit_bound on every compared unit.  Returns the ratio at C = 1."""
    c = FAMILY_C[ref["family"]]() if c is None else c
    r, j = score_error_units(scores, ref, c)
    print("%s: scores at c = %.3f (unit %d), allowed %g; %d undecided, %d ill-conditioned of %d"
          % (what, r, j, c, int(undecided(ref).sum()), int(ill_conditioned(ref, c).sum()), ref["score"].size))
    assert r <= c, (what, j, r, c, float(np.asarray(scores)[j]), float(ref["score"][j]))
    return r


def assert_special_scores(scores, ref, case, what):
    """The values that are exact by definition: DBL_MAX for always_select, 0.0 for a degenerate logistic / Cox unit, +inf
    for an all-zero LM column, bitwise equal scores for the duplicated pair."""
    got = np.asarray(scores, dtype=np.float64)
    assert got.shape == ref["score"].shape, (what, got.shape)
    for u in np.nonzero(ref["always"])[0]:
        assert got[u] == DBL_MAX, (what, "always_select", u, got[u])
    for u in np.nonzero(~ref["finite"])[0]:
        want = np.inf if ref["family"] == "lm" else 0.0
        assert got[u] == want, (what, "degenerate unit", u, got[u], want)
    for a, b in case["equal_pairs"]:
        assert got[a].tobytes() == got[b].tobytes(), (what, "duplicated pair", a, b, got[a], got[b])
    for u in np.nonzero(ref["finite"] & ~ref["always"])[0]:
        assert np.isfinite(got[u]) and got[u] >= 0.0, (what, u, got[u])


def assert_caps(ref, case, what, c=None):
    """At most one undecided or ill-conditioned unit per case, none of them a special column.  Returns their number."""
    bad = undecided(ref) | ill_conditioned(ref, c)
    print("%s: %d undecided, %d ill-conditioned of %d units" % (what, int(undecided(ref).sum()),
                                                                 int(ill_conditioned(ref, c).sum()), bad.size))
    assert int(bad.sum()) <= 1, (what, np.nonzero(bad)[0], ref["margin"][bad])
    for u in case["special"]:
        assert not bad[u], (what, "special unit not compared", u)
    return int(bad.sum())


def kept(scores, k):
    """The k largest (ascending unit numbers), or None where the k-th and (k + 1)-th are closer than 1e-9 relative: a
    top-k that the bounds do not decide."""
    sc = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-sc, kind="stable")
    if k < sc.size:
        a, b = sc[order[k - 1]], sc[order[k]]
        if a == b or (np.isfinite(a) and abs(a - b) <= 1e-9 * abs(a)):
            return None
    return np.sort(order[:k])


# ---- the seeded cases ------------------------------------------------------------------------------------------------------
SINGLETON_N = (50, 64, 65, 255, 256, 257, 513, 1000)
GROUP_N = (50, 257, 1000)
P_SINGLE = 40
LOGIT_WIDTHS = (1, 2, 3, 5, 8, 9, 4, 20)
COX_WIDTHS = (1, 2, 3, 4, 5, 20)
# special columns of the singleton layout
C_BIG, C_SMALL, C_DUP_A, C_DUP_B, C_ZERO, C_ONES, C_ALWAYS, C_TAIL = 7, 8, 9, 10, 11, 12, 13, 14
SIGNAL = (0, 1, 2, 3, 4)


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _weights(n, kind, rng):
    if kind == "plain":
        return None
    w = rng.uniform(0.5, 2.0, n)
    if kind == "zeros":
        w[rng.permutation(n)[:n // 10]] = 0.0
    return w


def _columns(n, p, rng, special):
    """Scales 0.3-3, means in +-2; columns 0-4 carry the signal (returned as the linear predictor on standardised columns)."""
    Z = rng.standard_normal((n, p))
    X = Z * rng.uniform(0.3, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    eta = Z[:, :5] @ np.array([1.0, -0.8, 0.6, -0.5, 0.4])
    if special:
        X[:, C_BIG] *= 1e3
        X[:, C_SMALL] *= 1e-3
        X[:, C_DUP_B] = X[:, C_DUP_A]
        X[:, C_ZERO] = 0.0
        X[:, C_ONES] = 1.0
        X[:, C_TAIL] = Z[:, C_TAIL]
    return X, eta


def _response(family, kind, n, eta, rng):
    if family == "lm":
        return eta + 0.5 * rng.standard_normal(n)
    if family == "logistic":
        off = 0.0 if kind == "balanced" else -3.6
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(eta + off)))).astype(np.float64)
        if y.sum() < 2:  # (a rare response needs both classes)
            y[np.argsort(-eta)[:2]] = 1.0
        return y
    cens = {"cens30": 0.3, "cens90": 0.9, "tail": 0.3}[kind]
    st = (rng.uniform(size=n) >= cens).astype(np.float64)
    if kind == "tail":
        st[-70:] = 0.0
        st[0] = 1.0
    if st.sum() < 3:
        st[rng.permutation(n)[:3]] = 1.0
    return st


def _order_by_time(X, eta, rng):
    """Cox: rows in time order, the hazard following the signal."""
    t = rng.exponential(1.0, eta.size) / np.exp(0.7 * eta)
    o = np.argsort(t)
    return X[o], eta[o]


RESPONSES = {"lm": ("gauss",), "logistic": ("balanced", "rare"), "cox": ("cens30", "cens90")}


def _case(family, n, wkind, rkind, seed, groups=False):
    name = "%s-%s-n%d-%s-%s" % (family, "groups" if groups else "single", n, wkind, rkind)
    rng = _rng(seed, RESEED.get(name, 0), n, MODEL_TYPE[family], int(groups), ("plain", "weighted", "zeros").index(wkind),
               ("gauss", "balanced", "rare", "cens30", "cens90", "tail").index(rkind))
    if groups:
        widths = {"lm": LOGIT_WIDTHS, "logistic": LOGIT_WIDTHS, "cox": COX_WIDTHS}[family]
        sizes = [widths[i % len(widths)] for i in range(len(widths) + 1)]  # one cycle, then the always_select group
        p = int(sum(sizes))
        gi = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
        always, special, pairs = [len(sizes) - 1], [], []
    else:
        p, gi = P_SINGLE, None
        always, pairs = [C_ALWAYS], [(C_DUP_A, C_DUP_B)]
        special = [C_BIG, C_SMALL, C_DUP_A, C_DUP_B, C_ZERO, C_ONES, C_ALWAYS]
    X, eta = _columns(n, p, rng, not groups)
    if family == "cox":
        X, eta = _order_by_time(X, eta, rng)
    y = _response(family, rkind, n, eta, rng)
    if family == "cox" and not groups:
        # one far outlier in the first row, an event: the Newton steps overshoot there and the linear predictor passes
        # 30, so the two clamps of cox_fit (50 in the Newton sums, 30 in the log-likelihood) are told apart
        X[0, C_TAIL] = 200.0
        y[0] = 1.0
    nunits = p if gi is None else gi.size
    return {"name": name, "family": family,
            "X": np.ascontiguousarray(X), "y": y, "weight": _weights(n, wkind, rng), "g_index": gi, "always": always,
            "special": special, "equal_pairs": pairs, "screening_size": nunits // 2, "nunits": nunits}


SEED = 20261020
# cases drawn again (second entry of the seed) until the REFERENCE ALONE leaves at most one unit undecided or
# ill-conditioned; tests/test_screen_reference.py asserts the caps on every case
RESEED = {
    'logistic-single-n50-plain-balanced': 1,
    'logistic-single-n257-weighted-rare': 1,
    'logistic-single-n513-weighted-rare': 1,
    'logistic-single-n1000-plain-balanced': 1,
    'cox-single-n50-plain-cens90': 1,
    'cox-single-n50-weighted-cens30': 1,
    'cox-single-n64-plain-cens30': 2,
    'cox-single-n64-weighted-cens30': 3,
    'cox-single-n65-plain-cens30': 1,
    'cox-single-n65-weighted-cens30': 3,
    'cox-single-n65-weighted-cens90': 3,
    'cox-single-n255-plain-cens30': 5,
    'cox-single-n255-plain-cens90': 2,
    'cox-single-n255-weighted-cens30': 2,
    'cox-single-n255-weighted-cens90': 3,
    'cox-single-n256-plain-cens30': 4,
    'cox-single-n256-weighted-cens30': 4,
    'cox-single-n257-plain-cens30': 3,
    'cox-single-n257-weighted-cens30': 7,
    'cox-single-n257-weighted-cens90': 2,
    'cox-single-n257-zeros-cens30': 5,
    'cox-single-n513-plain-cens30': 20,
    'cox-single-n513-plain-cens90': 2,
    'cox-single-n513-weighted-cens90': 2,
    'cox-single-n1000-plain-cens30': 6,
    'cox-single-n1000-plain-cens90': 1,
    'cox-single-n1000-weighted-cens30': 24,
    'cox-single-n1000-weighted-cens90': 3,
    'cox-single-n1000-zeros-cens30': 12,
    'cox-single-n1000-zeros-cens90': 2,
    'cox-groups-n257-plain-cens30': 1,
}


def singleton_cases(family):
    out = []
    for n in SINGLETON_N:
        for wkind in ("plain", "weighted") + (("zeros",) if n in (257, 1000) and family != "lm" else ()):
            for rkind in RESPONSES[family]:
                out.append(_case(family, n, wkind, rkind, SEED))
    if family == "cox":
        out.append(_case(family, 257, "weighted", "tail", SEED))
    return out


def group_cases(family):
    return [_case(family, n, wkind, RESPONSES[family][0], SEED, groups=True) for n in GROUP_N
            for wkind in ("plain", "weighted")]


def all_cases(family):
    return singleton_cases(family) + (group_cases(family) if family != "lm" else [])


_REF = {}


def cached_reference(case):
    """One longdouble reference per case, shared by every test of the process and left unchanged."""
    if case["name"] not in _REF:
        _REF[case["name"]] = reference(case)
    return _REF[case["name"]]
