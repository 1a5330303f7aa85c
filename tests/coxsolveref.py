"""Extended-precision reference for the Cox SOLVER's state pass, risk-set scans, loss sums and sacrifice scores (the
kernels of bessx_k_cox.hip reached by bessx_op_cox_state / _score / _score_multi and by Session.fit): pure NumPy in
np.longdouble, no GPU, no oracle.  It restates the OPERATIONS (GroupPdasCox::get_A, src/Algorithm.h:1569-1640;
primary_model_fit, :1377-1490; loglik_cox, src/coxph.cpp:16-40; CoxMetric, src/Metric.h:565-568, 609), not the kernels.

Conventions.  Rows are in time order (row 0 = earliest time), delta_i = status, w_i = weight (ones without), mask_i = 1 on
the training rows of a CV fold and 0 on its test rows (ones without a fold).  A model is (cols, b): eta_i = sum_a
x_i,cols[a] b_a (no intercept), a_i = clamp(eta_i, -30, 30), e_i = exp(a_i).

  state pass    theta_i = w_i e_i mask_i               (get_A weights exp by w; the fit does not)
                S0_i    = sum_{l >= i} theta_l         risk-set sums of the training rows;  RS0_i = 1 / S0_i, and 0 where
                                                       S0_i = 0 (rows behind the last training row: an empty risk set)
                Sall_i  = sum_{l >= i} e_l             (the loss is formed on ALL rows, unweighted sums)
                Stest_i = sum_{l >= i} e_l (1 - mask_l)
                loss_all  = sum_i w_i delta_i log(e_i / Sall_i),   loss_test = the same over the rows with mask_i = 0 and Stest
  scores        ew_i = w_i [delta_i != 0] mask_i,  S1_j(i) = sum_{l >= i} theta_l x_lj,  S2_j(i) = sum_{l >= i} theta_l x_lj^2
                g_j = sum_i ew_i (x_ij - S1_j(i) / S0_i),   h_j = sum_i ew_i (S2_j(i) / S0_i - (S1_j(i) / S0_i)^2)
                l1_j = -g_j + 2 lam beta_j,  l2_j = h_j + 2 lam,  d_j = -l1_j / l2_j,  bd_j = |beta_j + d_j| sqrt(l2_j)
  Newton step   (on the training rows, theta = e mask WITHOUT w)   grad_u = sum_i w_i delta_i mask_i (x_iu - S1_u(i) / S0_i)
                + 2 lam b_u;   hess_uv = -sum_i w_i delta_i mask_i (S2_uv(i) / S0_i - S1_u(i) S1_v(i) / S0_i^2) + 2 lam [u = v]
                (the sign of the ridge is the reference's, :1471); the step is b - hess^-1 grad.

Forward-error model of the scores (after xprec.scores): M1_j and M2_j are g_j and h_j with every elementary product
replaced by its absolute value, M1_j = sum_i ew_i (|x_ij| + A1_j(i) / S0_i) + 2 lam |beta_j|, M2_j = sum_i ew_i (A2_j(i) / S0_i
+ (A1_j(i) / S0_i)^2) + 2 lam with A1, A2 the suffix sums of theta |x| and theta x^2.  An error of c u M1 in l1 and c u M2 in
l2 moves bd = |beta - l1 / l2| sqrt(l2) by at most
    c u [ sqrt(l2) (M1 / l2 + |l1| M2 / l2^2) + |beta + d| M2 / (2 sqrt(l2)) ] + 4 u bd
(4 u bd: the division, the sum, the square root and the product themselves).  score_error_units returns the error in
units of that expression at c = 1.  The expression is first order in the error of l2: where ILL_COND u M2_j >= l2_j (the
sum h_j has lost 53 - 10 = 43 bits to cancellation: every row of the column's risk sets holds almost the same value)
the perturbation reaches l2 itself, sqrt(l2) of a computed value may be anything including NaN, and the bound says
nothing: such columns are counted, not compared (only the absorbing models have them: the model's own column, which is
-40 on all but nine rows).  The one-pass form of the library exchanges the order of summation (sum_l u_l x_lj
with u_l = theta_l sum_{i <= l} ew_i / S0_i, and (loc + car)^2 expanded): the same elementary products, the same M1, M2.

SCORE_C.  fp64 NumPy evaluating the formulas above with running sums of the positive terms (scores_fp64: the CPU
stand-in, never the kernels) against this reference over every case of tests/test_cox_ops_gpu.py
(tests/test_coxsolve_reference.py measures it): SCORE_C_NUMPY_MAX.  SCORE_C = 4 x that, rounded up to a power of two; the
factor four allows for a different but equally valid order of summation.

The module also holds the seeded cases both test files use and the assert_* helpers, one per bound, so that the CPU file
can show each of them failing on a perturbed input."""
import os
import re

import numpy as np

import xprec

LD, U, EXTENDED = xprec.LD, xprec.U, xprec.EXTENDED
ld = xprec.ld
CLAMP = 30.0
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bess_amd", "csrc")

# fp64 NumPy (scores_fp64) under the forward-error model, maximum over score_cases() and absorbing_models(); measured by
# tests/test_coxsolve_reference.py::test_fp64_numpy_scores_stay_inside_the_model_and_fix_SCORE_C
SCORE_C_NUMPY_MAX = 8.7912  # n = 4100, p = 8, plain, three coefficients, lam = 0.05, column 0
SCORE_C = 64.0             # 4 x 8.7912 = 35.2, rounded up to a power of two
ILL_COND = 1024.0


def _constant(fname, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, fname)).read())
    assert m, "%s no longer states %s: re-derive the bounds of coxsolveref" % (fname, pattern)
    return m


_m = _constant("bessx_k_cox.hip", r"constexpr int SC_T = (\d+), SC_E = (\d+), SC_B = SC_T \* SC_E;")
SC_T, SC_E = int(_m.group(1)), int(_m.group(2))
SC_B, SC_W = SC_T * SC_E, SC_T // 64
COX_MC_MAX = int(_constant("bessx_dev.h", r"constexpr int COX_MC_MAX = (\d+);").group(1))


# ---- the operations ---------------------------------------------------------------------------------------------------
def _wm(n, w, mask):
    return (np.ones(n, dtype=LD) if w is None else ld(w)), (np.ones(n, dtype=LD) if mask is None else ld(mask))


def suffix(v):
    return np.cumsum(v[::-1], axis=0)[::-1]


def exact_suffix_sums(v):
    """Suffix sums of non-negative fp64 values, EXACT (integers over a common power of two), rounded once to longdouble."""
    v = np.asarray(v, dtype=np.float64)
    assert (v >= 0).all() and np.isfinite(v).all()
    out = np.zeros(v.size, dtype=LD)
    if not (v > 0).any():
        return out
    mant, ex = np.frexp(v)
    emin = int(ex[v > 0].min()) - 53
    acc = 0
    for i in range(v.size - 1, -1, -1):
        if v[i] > 0:
            acc += int(np.ldexp(mant[i], 53)) << (int(ex[i]) - 53 - emin)
        if acc:
            sh = max(acc.bit_length() - 64, 0)
            top = acc >> sh
            out[i] = np.ldexp(LD(top >> 32) * LD(4294967296.0) + LD(top & 0xFFFFFFFF), sh + emin)
    return out


def state(X, status, w, mask, cols, b):
    """The state pass in longdouble: a dict of eta, e, theta, S0, RS0, S_all, S_test (None without a mask), loss_all,
    loss_test, and what the bounds need: eta_abs = sum_a |x_ia b_a|, loss_abs = sum_i w_i delta_i |log(e_i / Sall_i)|
    (loss_test_abs likewise)."""
    X64 = np.asarray(X, dtype=np.float64)
    n = X64.shape[0]
    cols = np.asarray(cols, dtype=int).reshape(-1)
    bl = ld(b).reshape(-1)
    XA = ld(X64[:, cols])
    eta = XA @ bl if cols.size else np.zeros(n, dtype=LD)
    eta_abs = (np.abs(XA) @ np.abs(bl)).astype(np.float64) if cols.size else np.zeros(n)
    e = np.exp(np.clip(eta, LD(-CLAMP), LD(CLAMP)))
    wl, ml = _wm(n, w, mask)
    d = ld(status)
    theta = wl * e * ml
    S0 = suffix(theta)
    with np.errstate(divide="ignore"):
        RS0 = np.where(S0 != 0, LD(1) / np.where(S0 != 0, S0, LD(1)), LD(0))
    S_all = suffix(e)
    t_all = wl * d * np.log(e / S_all)
    out = {"eta": eta, "eta_abs": eta_abs, "e": e, "theta": theta, "S0": S0, "RS0": RS0, "S_all": S_all, "S_test": None,
           "loss_all": t_all.sum(), "loss_abs": float(np.abs(t_all).sum()), "loss_test": LD(0), "loss_test_abs": 0.0,
           "wd": (wl * d).astype(np.float64), "mask": ml.astype(np.float64), "m": int(cols.size)}
    if mask is not None:
        et = e * (LD(1) - ml)
        S_test = suffix(et)
        te = (ml == 0) & (d != 0)
        t_te = np.where(te, wl * d * np.log(np.where(te, e, LD(1)) / np.where(te, S_test, LD(1))), LD(0))
        out.update(S_test=S_test, loss_test=t_te.sum(), loss_test_abs=float(np.abs(t_te).sum()))
    return out


def score_sums(X, status, w, mask, cols, b):
    """g, h, M1, M2 without the ridge terms (longdouble / fp64), for every column; finish with scores_finish(lam)."""
    st = state(X, status, w, mask, cols, b)
    X64 = np.asarray(X, dtype=np.float64)
    n, p = X64.shape
    Xl = ld(X64)
    wl, ml = _wm(n, w, mask)
    ew = wl * (ld(status) != 0) * ml
    ev = ew != 0
    th = st["theta"][:, None]
    rs = st["RS0"][ev][:, None]
    q1 = suffix(th * Xl)[ev] * rs
    q2 = suffix(th * Xl * Xl)[ev] * rs
    a1 = suffix(th * np.abs(Xl))[ev] * rs
    e1 = ew[ev]
    beta = np.zeros(p, dtype=LD)
    beta[np.asarray(cols, dtype=int).reshape(-1)] = ld(b).reshape(-1)
    return {"g": e1 @ (Xl[ev] - q1), "h": e1 @ (q2 - q1 * q1), "beta": beta,
            "M1": (e1 @ (np.abs(Xl[ev]) + a1)).astype(np.float64), "M2": (e1 @ (q2 + a1 * a1)).astype(np.float64)}


def scores_finish(s, lam):
    lam = LD(lam)
    beta = s["beta"]
    l1, l2 = -s["g"] + 2 * lam * beta, s["h"] + 2 * lam
    d = -l1 / l2
    return {"d": d, "phi": np.sqrt(l2), "l1": l1, "l2": l2, "beta": beta, "bd": np.abs(beta + d) * np.sqrt(l2),
            "M1": s["M1"] + 2 * float(lam) * np.abs(beta.astype(np.float64)), "M2": s["M2"] + 2 * float(lam)}


def scores(X, status, w, mask, cols, b, lam):
    """d, phi = sqrt(l2), bd for all p columns in longdouble, with the magnitude sums M1, M2 of the error model."""
    return scores_finish(score_sums(X, status, w, mask, cols, b), lam)


def scores_fp64(X, status, w, mask, cols, b, lam):
    """fp64 NumPy evaluating the same formulas with running sums (the CPU stand-in for the kernels)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    cols = np.asarray(cols, dtype=int).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    mk = np.ones(n) if mask is None else np.asarray(mask, dtype=np.float64)
    eta = X[:, cols] @ b if cols.size else np.zeros(n)
    th = w * np.exp(np.clip(eta, -CLAMP, CLAMP)) * mk
    S0 = suffix(th)
    ew = w * (np.asarray(status) != 0) * mk
    ev = ew != 0
    q1 = suffix(th[:, None] * X)[ev] / S0[ev][:, None]
    q2 = suffix(th[:, None] * X * X)[ev] / S0[ev][:, None]
    g, h = ew[ev] @ (X[ev] - q1), ew[ev] @ (q2 - q1 * q1)
    beta = np.zeros(p)
    beta[cols] = b
    l1, l2 = -g + 2 * lam * beta, h + 2 * lam
    with np.errstate(invalid="ignore"):  # (an ill-conditioned column's l2 may come out negative)
        return np.abs(beta - l1 / l2) * np.sqrt(l2)


def newton_gradient_hessian(X, status, w, mask, cols, b, lam):
    """(grad, hess) of the restricted fit's Newton step at b on support cols, longdouble (formulas in the module
    docstring; theta without the weights, the training rows only)."""
    X64 = np.asarray(X, dtype=np.float64)
    n = X64.shape[0]
    cols = np.asarray(cols, dtype=int).reshape(-1)
    wl, ml = _wm(n, w, mask)
    XA, bl = ld(X64[:, cols]), ld(b).reshape(-1)
    th = np.exp(np.clip(XA @ bl, LD(-CLAMP), LD(CLAMP))) * ml
    S0 = suffix(th)
    wd = wl * ld(status) * ml
    ev = wd != 0
    rs = (LD(1) / S0[ev])[:, None]
    q1 = suffix(th[:, None] * XA)[ev] * rs
    grad = wd[ev] @ (XA[ev] - q1) + 2 * LD(lam) * bl
    k = cols.size
    hess = np.zeros((k, k), dtype=LD)
    for u in range(k):
        q2 = suffix((th * XA[:, u])[:, None] * XA)[ev] * rs
        hess[u] = -(wd[ev] @ (q2 - q1[:, [u]] * q1))
    return grad, hess + 2 * LD(lam) * np.eye(k, dtype=LD)


# ---- the bounds ---------------------------------------------------------------------------------------------------------
def scan_depth(n):
    """k of |S - S*| <= k u S*: the longest chain of additions any term goes through on its way into a scan output of
    k_scan3_tot / k_scan3_apply (SC_E elements per thread, SC_T threads = SC_W waves per block, ceil(n / SC_B) blocks;
    block_excl_256 in bessx_kdev.hpp), every term non-negative and entering exactly once:
      SC_E - 1   the thread's own total ((x0 + x1) + x2) + x3
      6          the shuffle scan across the 64 lanes (log2 64 steps)
      SC_W - 1   the totals of the waves before (off), or the block's total from its wave totals
      nb - 1     the carry: the totals of the blocks before, in block order
      2          off + exc, carry + offset
      SC_E       the thread adds its own elements one by one behind the offset."""
    nb = -(-int(n) // SC_B)
    return (SC_E - 1) + 6 + (SC_W - 1) + (nb - 1) + 2 + SC_E


def loss_depth(n):
    """Roundings per term of k_cox_loss relative to |w delta log(e / S)|: the product w delta (1), the allowance of 2 u for
    log itself (as tests/coxevalref.py), the product with the logarithm (1), the thread's two rows (1), the butterfly
    over 64 lanes (6), the two waves (1), the workgroups of 256 rows in workgroup order on the host (ceil(n / 256) - 1;
    the workgroups of the row padding add exact zeros)."""
    return 1 + 2 + 1 + 1 + 6 + 1 + (-(-int(n) // 256) - 1)


def e_rtol(ref):
    """Per row: (m + 2) u sum_a |x_ia b_a| + 4 u.  A relative error of exp is an absolute error of its argument (the clamp
    is 1-Lipschitz); 4 u covers exp itself."""
    return (ref["m"] + 2) * U * ref["eta_abs"] + 4 * U


def _frac(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return f


def assert_e_close(e, ref, what):
    """|E - e*| <= e_rtol e*.  Returns the largest fraction of the bound used."""
    err = np.abs((ld(e) - ref["e"]) / ref["e"]).astype(np.float64)
    f = _frac(err, e_rtol(ref))
    i = int(np.argmax(f))
    print("%s: E off by %.2f of its bound at row %d" % (what, f[i], i))
    assert np.isfinite(np.asarray(e)).all() and f[i] <= 1.0, (what, i, err[i], e_rtol(ref)[i])
    return float(f[i])


def assert_risk_sums_close(S, terms, what, recip=None):
    """S against the EXACT suffix sums S* of the terms the device itself returned (that isolates the scan):
    |S - S*| <= scan_depth(n) u S*; rows with an empty risk set (S* = 0) are exactly 0; recip, if given, is within
    (scan_depth(n) + 2) u of 1 / S* (the scan's bound and two more roundings) and exactly 0 where S* = 0.
    Returns the largest fraction of the bound used by (sums, reciprocals)."""
    S, terms = np.asarray(S, dtype=np.float64), np.asarray(terms, dtype=np.float64)
    n = S.size
    k = scan_depth(n)
    Sx = exact_suffix_sums(terms)
    empty = Sx == 0
    assert (S[empty] == 0.0).all(), (what, "a row with an empty risk set has a non-zero sum")
    assert np.isfinite(S).all(), what
    one = np.where(empty, LD(1), Sx)
    f = _frac(np.abs((ld(S) - Sx) / one).astype(np.float64), np.where(empty, 0.0, k * U))
    i = int(np.argmax(f))
    print("%s: risk-set sum off by %.3f of %d u at row %d" % (what, f[i], k, i))
    assert f[i] <= 1.0, (what, "S", i, float(S[i]), float(Sx[i]), f[i])
    fr = 0.0
    if recip is not None:
        recip = np.asarray(recip, dtype=np.float64)
        assert (recip[empty] == 0.0).all() and np.isfinite(recip).all(), (what, "reciprocal of an empty risk set")
        g = _frac(np.where(empty, 0.0, np.abs(ld(recip) * one - LD(1)).astype(np.float64)), np.where(empty, 0.0, (k + 2) * U))
        j = int(np.argmax(g))
        print("%s: reciprocal off by %.3f of %d u at row %d" % (what, g[j], k + 2, j))
        assert g[j] <= 1.0, (what, "1/S", j, float(recip[j]), g[j])
        fr = float(g[j])
    return float(f[i]), fr


def loss_bound(ref, test=False):
    """|loss - loss*| <= sum_i w_i delta_i [ loss_depth u |log(e_i / S_i)| + rho_i + (scan_depth u + max_{l >= i} rho_l) + u ]
    with rho = e_rtol: the reduction's own roundings relative to the magnitude sum, plus what E (rho_i), S (the scan's
    bound on top of the largest relative error of its terms) and the division (u) carry into the logarithm's argument."""
    n = ref["e"].size
    rho = e_rtol(ref)
    rhomax = np.maximum.accumulate(rho[::-1])[::-1]
    wd = ref["wd"]
    if test:
        wd = wd * (ref["mask"] == 0)
    carried = float((wd * (rho + scan_depth(n) * U + rhomax + U)).sum())
    return loss_depth(n) * U * (ref["loss_test_abs"] if test else ref["loss_abs"]) + carried


def assert_loss_close(loss, ref, what, test=False):
    """The loss sum within loss_bound.  Returns the fraction of the bound used."""
    want = ref["loss_test"] if test else ref["loss_all"]
    err, bound = float(abs(LD(loss) - want)), loss_bound(ref, test)
    f = float(_frac(np.float64(err), np.float64(bound)))
    print("%s: loss %.17g off by %.3e = %.3f of its bound" % (what, float(loss), err, f))
    assert np.isfinite(loss) and f <= 1.0, (what, float(loss), float(want), err, bound)
    return f


def score_error_units(bd, ref):
    """max_j |bd_j - bd*_j| in units of the forward-error model at c = 1 over the columns the model speaks about (module
    docstring).  Returns (ratio, column); score_ill_conditioned(ref) names the columns left out."""
    l1, l2 = np.abs(ref["l1"].astype(np.float64)), ref["l2"].astype(np.float64)
    t, bdr = np.abs((ref["beta"] + ref["d"]).astype(np.float64)), ref["bd"].astype(np.float64)
    r2 = np.sqrt(l2)
    allowed = U * (r2 * (ref["M1"] / l2 + l1 * ref["M2"] / (l2 * l2)) + t * ref["M2"] / (2 * r2) + 4 * bdr)
    ratio = np.abs((ld(bd) - ref["bd"]).astype(np.float64)) / np.maximum(allowed, 1e-300)
    ratio = np.where(np.isfinite(np.asarray(bd, dtype=np.float64)), ratio, np.inf)
    ratio = np.where(score_ill_conditioned(ref), 0.0, ratio)
    j = int(np.argmax(ratio))
    return float(ratio[j]), j


def score_ill_conditioned(ref):
    return ILL_COND * U * ref["M2"] >= ref["l2"].astype(np.float64)


def assert_scores_close(bd, ref, what, c=None):
    """|bd - bd*| <= SCORE_C x the forward-error model.  Returns the ratio at c = 1."""
    r, j = score_error_units(bd, ref)
    c = SCORE_C if c is None else c
    print("%s: scores at c = %.3f (column %d), allowed %g" % (what, r, j, c))
    assert r <= c, (what, j, r, c, float(np.asarray(bd)[j]), float(ref["bd"][j]))
    return r


# ---- a NumPy stand-in of the block scan, both forms of the thread offset ------------------------------------------------------
def scan_standin(v, form):
    """Suffix sums of v in fp64 with the geometry of k_scan3_apply (SC_E x 64 x SC_W per block, carry in block order) and
    the thread's exclusive offset formed as `form`: "sub" = inclusive - own total (the solver before this reference
    existed), "add" = the inclusive value of the lane before plus the totals of the waves before."""
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    nb = -(-n // SC_B)
    x = np.zeros(nb * SC_B)
    x[:n] = v[::-1]
    x = x.reshape(nb, SC_W, 64, SC_E)
    out = np.empty_like(x)
    carry = 0.0
    for blk in range(nb):
        xb = x[blk]
        tt = xb[..., 0].copy()
        for q in range(1, SC_E):
            tt = tt + xb[..., q]
        inc = tt.copy()
        o = 1
        while o < 64:
            inc[:, o:] = inc[:, o:] + inc[:, :-o].copy()
            o *= 2
        wt = inc[:, 63]
        off = np.zeros(SC_W)
        for wv in range(1, SC_W):
            off[wv] = off[wv - 1] + wt[wv - 1]
        if form == "sub":
            exc = off[:, None] + inc - tt
        else:
            exc = np.concatenate([off[:, None], off[:, None] + inc[:, :-1]], axis=1)
        s = carry + exc
        for q in range(SC_E):
            s = s + xb[..., q]
            out[blk, ..., q] = s
        carry = carry + (((wt[0] + wt[1]) + wt[2]) + wt[3] if SC_W == 4 else wt.sum())
    return out.reshape(-1)[:n][::-1].copy()


# ---- seeded cases, one place for both files -----------------------------------------------------------------------------------
STATE_N = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 4100)
STATE_P = 12
SCORE_N, SCORE_P, SCORE_LAM = (97, 1024, 1025, 4100), (1, 7, 8, 9, 33, 257), (0.0, 0.05)
ABSORB_N, ABSORB_AT = 1040, (4, 252, 256, 260, 1028)


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def cv_mask(n, rng):
    """A 0/1 row mask whose last training row is followed by min(3, n - 1) test rows (empty risk sets)."""
    mk = (rng.uniform(size=n) < 0.75).astype(np.float64)
    tail = min(3, n - 1)
    mk[n - tail:] = 0.0
    mk[n - tail - 1] = 1.0
    return mk


def zero_weights(n, rng):
    """Weights in (0.25, 1.75) with every fifth row (from row 1) and the last row exactly 0."""
    w = rng.uniform(0.25, 1.75, n)
    w[1::5] = 0.0
    w[n - 1] = 0.0
    return w


def state_cases(n):
    """name -> (X, status, w, mask, cols, b) for the state pass at n rows, STATE_P columns: unit weights (m = 1), weights
    with exact zeros (m = 2), a CV mask with trailing test rows (m = 9), all rows censored, only the last / only the first
    row an event, and a model whose linear predictor leaves +-30 on both sides (the clamp)."""
    rng = _rng(7, n)
    X = rng.standard_normal((n, STATE_P))
    st = (rng.uniform(size=n) < 0.6).astype(np.float64)
    only = lambda i: np.eye(1, n, i).reshape(-1)  # noqa: E731
    c9 = np.arange(9, dtype=np.int32)
    big = X.copy()
    big[:, 3] = np.linspace(-1.0, 1.0, n) if n > 1 else 1.0
    return {
        "unit m=1": (X, st, None, None, [5], [0.7]),
        "zero weights m=2": (X, st, zero_weights(n, rng), None, [2, 7], [0.5, -0.8]),
        "cv mask m=9": (X, st, rng.uniform(0.5, 2.0, n), cv_mask(n, rng), c9, rng.uniform(-0.5, 0.5, 9)),
        "all censored": (X, np.zeros(n), None, cv_mask(n, rng), [1, 4], [0.3, 0.3]),
        "last row the only event": (X, only(n - 1), None, None, [0], [-0.4]),
        "first row the only event": (X, only(0), zero_weights(n, rng) + only(0), cv_mask(n, rng) if n > 4 else None, [0], [1.1]),
        "clamp": (big, st, None, None, [3, 6], [45.0, 0.25]),
    }


def absorbing_models():
    """The pattern at which a scan that forms a thread's exclusive offset as inclusive - own total loses everything, in the
    SOLVER's scan order: suffix scan index r is row n - 1 - r, thread t of a block owns indices 4 t .. 4 t + 3.  Column r
    of X, read alone with coefficient 1 (model r: cols = [r], b = [1]), holds by scan index: -40 (clamped to -30) before
    index j0 + 3 and +40 (clamped to +30) AT j0 + 3, the last element of the SAME thread, N(0, 9) behind it; j0 in
    ABSORB_AT = lane 1 and lane 63 of the first wave, lanes 0 and 1 of the second wave, lane 1 of the second block.  The
    last column is a staircase in thread 2: -40 up to index 6, 0 at 7..10, +40 at 11.  Every row is an event, unit
    weights.  Returns (X, status, [(cols, b)] per model)."""
    n, R = ABSORB_N, len(ABSORB_AT) + 1
    rng = _rng(85)
    scan = 3.0 * rng.standard_normal((n, R))
    for r, j0 in enumerate(ABSORB_AT):
        scan[:j0 + 3, r] = -40.0
        scan[j0 + 3, r] = 40.0
    scan[:7, R - 1], scan[7:11, R - 1], scan[11, R - 1] = -40.0, 0.0, 40.0
    X = np.ascontiguousarray(scan[::-1])
    return X, np.ones(n), [(np.array([r], dtype=np.int32), np.array([1.0])) for r in range(R)]


def score_data(n, p):
    rng = _rng(11, n, p)
    X = rng.standard_normal((n, p))
    st = (rng.uniform(size=n) < 0.6).astype(np.float64)
    st[n // 2] = 1.0
    return X, st, rng.uniform(0.5, 2.0, n), cv_mask(n, rng)


def score_models(p):
    """The model with (up to) three non-zero coefficients and the all-zero model (no column: what a cold fit starts from)."""
    cols = np.unique(np.array([0, p // 2, p - 1], dtype=np.int32))
    return {"three": (cols, np.array([0.8, -0.6, 0.4])[:cols.size]), "zero": (np.zeros(0, dtype=np.int32), np.zeros(0))}


def score_cases(n, p):
    """name -> (X, status, w, mask, cols, b): plain, weighted, masked (with weights) x the two models."""
    X, st, w, mk = score_data(n, p)
    out = {}
    for vn, (ww, mm) in {"plain": (None, None), "weighted": (w, None), "masked": (w, mk)}.items():
        for mn, (cols, b) in score_models(p).items():
            out["%s %s" % (vn, mn)] = (X, st, ww, mm, cols, b)
    return out


def outlier_design(n=600, p=40, seed=3):
    """A Cox design with one column of outliers (column 0: N(0, 1) with every 25th row times 12) that carries signal, so
    that the fitted linear predictor spans more than +-12.  Rows sorted by time.  Returns (X, status)."""
    rng = _rng(seed)
    X = rng.standard_normal((n, p))
    X[::25, 0] *= 12.0
    eta = 1.5 * X[:, 0] + 0.8 * X[:, 1] - 0.8 * X[:, 2]
    time = -np.log(rng.uniform(size=n)) / np.exp(np.clip(eta, -30, 30))
    ctime = np.quantile(time, 0.8) * rng.uniform(0.5, 1.5, n)
    st = (time < ctime).astype(np.float64)
    order = np.argsort(np.minimum(time, ctime), kind="stable")
    return np.ascontiguousarray(X[order]), st[order]
