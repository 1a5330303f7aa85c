"""Extended-precision reference, exact pair counts and error bound for the held-out Cox partial log-likelihood and
Harrell's concordance of bessx_eval_cox_device / capi.evaluate_cox_device / bess_base.evaluate_survival (shared by
tests/test_cox_eval_api.py and tests/test_cox_eval_gpu.py, in the manner of tests/evalref.py).

Definitions.  pi is the stable ascending sort of time; position k holds row pi(k); first(k) is the smallest position with
the time of position k.  eta*(k, r) = sum_j x(pi(k), cols[j]) B[j, r] (no intercept), a* = clamp(eta*, -30, 30),
e* = exp(a*), S*(k) = sum_{l >= k} e*(l) ("order") or sum_{l >= first(k)} e*(l) ("breslow"),
t*(k) = a*(k) - log S*(k), loglik*_r = sum_k w_k delta_k t*(k, r): NumPy in np.longdouble on the host copy of the same
(widened) values.  (On x86 longdouble carries 64 significant bits; the reference's own error is 2^-11 of every figure
below and is not added.)

The bound is derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u), and eta*, Delta come from
evalref.eta_reference with c = 0: |eta_hat - eta*| <= Delta_k = gamma_{m+2} sum_j |x_kj| |B_jr|.

What the implementations compute, each floating-point operation counted once (the device kernels of
bessx_k_coxeval.hip and the NumPy route of bess_base.evaluate_survival have the same form, a - log S):

    a_hat  = clamp(eta_hat)              comparisons and selection: no rounding
    e_hat  = exp(a_hat)                  one exp, allowed 1 ulp = 2 u relative
    S_hat  = sum of e_hat over the risk set, at most n terms, ADDITIONS ONLY, every term entering exactly once, so
             n - 1 additions in some order.  NumPy: a running sum.  Device (k_cxe_scan_tot / k_cxe_scan_apply), in scan
             order = from the last position down, blocks of 1024, a thread owning four consecutive terms:
               S = carry + (off + exc) + x_0 [+ x_1 [+ x_2 [+ x_3]]]     added from the left, where
               carry = the totals of the blocks before, added in block order; a block's total = the four wave totals
                       added in wave order, a wave total = the last lane's inclusive scan
               off   = the totals of the waves before in this block, added in wave order
               exc   = the inclusive shuffle scan (six steps of +) of the thread totals ((x_0 + x_1) + x_2) + x_3 of
                       the wave, taken from the lane before; lane 0 has no exc and uses off alone
             No term is taken out again: there is no subtraction anywhere in S.  (inclusive - own total, the usual way
             to an exclusive offset, is NOT covered by item 3: a thread total of e^30 absorbs a running sum of a few
             e^-30 and the difference is 0, a relative error of 1 in S.  test_cox_eval_gpu.py constructs that case.)
    l_hat  = log(S_hat)                  one log
    t_hat  = a_hat - l_hat               one subtraction
    wd     = w * delta                   one multiplication (exact: delta is 0 or 1)
    loglik = sum_k wd_k * t_hat_k        one multiplication per term, n - 1 additions in some order

1. The clamp is 1-Lipschitz: |a_hat - a*| <= Delta_k.
2. e: exp(a_hat) = exp(a*) exp(a_hat - a*), and the computed exp carries a relative error of at most 2 u:
       rho_k <= expm1(Delta_k) (1 + 2 u) + 2 u.
3. S is a sum of at most n positive terms, each with relative error at most rhomax_k = max of rho over the risk set (from
   k under "order", from first(k) under "breslow"), added in any order with every term entering once and none removed
   (Higham, section 4.2: n - 1 additions, gamma_{n-1} relative to the sum of the magnitudes, which for positive terms is
   the sum itself; the forms listed above are such sums):
       sigma_k <= rhomax_k + gamma_{n-1} (1 + rhomax_k).
4. log S: |log(S* (1 + s))| with |s| <= sigma_k is at most -log(1 - sigma_k); log's own rounding is an ALLOWANCE of
   2 u |log S| (not a derived figure: the accuracy of the device's and of NumPy's log is documented as about 1 ulp), with
   |log S| taken at |log S*| - log(1 - sigma_k).
5. The subtraction: u |t|, with |t| taken at |t*| plus the errors of items 1 and 4.
6. The weighted sum: the product w delta, the product with t and n - 1 additions: gamma_{n+1} sum_k |w_k delta_k t_k|.

Together, as the issue of this feature states it, with tau_k the sum of items 1 to 5,

    |loglik_hat_r - loglik*_r| <= sum_k w_k delta_k tau_k + gamma_{n+1} sum_k |w_k delta_k t*_k|

(the product gamma_{n+1} tau_k, of second order in u, is dropped as in evalref).

The counts involve no rounding at all once the ORDER of every comparable pair's two eta_hat is the order of their eta*:
count_precondition() asserts, on EVERY comparable pair and every model, that either the two rows are identical on the
model's support (the kernels and the NumPy route form a row's sum in an order that does not depend on the row, so the two
eta_hat are the same bits: an exact tie) or |eta*_k - eta*_l| > Delta_k + Delta_l.  No pair is left out; inputs that
violate it are to be replaced.  The counts then EQUAL those of pair_counts(), an O(n^2) integer count on eta*."""
import numpy as np

import evalref

LD = np.longdouble
U = evalref.U
gamma = evalref.gamma


def time_order(time):
    """(order, first): the stable ascending sort of time and, per position, the smallest position with the same time."""
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    order = np.argsort(time, kind="stable")
    t = time[order]
    first = np.zeros(t.size, dtype=np.int64)
    for k in range(1, t.size):
        first[k] = first[k - 1] if t[k] == t[k - 1] else k
    return order, first


def loglik_reference(eta, delta, time, status, w, ties):
    """Reference and bound for one call: eta, delta (n, R) in row order from evalref.eta_reference (c = 0); time, status
    (n,); w (n,) or None; ties "order" / "breslow".  Returns {"loglik": (R,), "bound": (R,)} in longdouble."""
    n, R = eta.shape
    order, first = time_order(time)
    eta, delta = eta[order], delta[order]
    d = np.asarray(status).astype(LD).reshape(-1)[order]
    wl = (np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)[order]) * d
    a = np.clip(eta, LD(-30), LD(30))
    e = np.exp(a)
    S = np.cumsum(e[::-1], axis=0)[::-1]
    rho = np.expm1(delta) * (LD(1) + LD(2) * U) + LD(2) * U
    rhomax = np.maximum.accumulate(rho[::-1], axis=0)[::-1]
    if ties == "breslow":
        S, rhomax = S[first], rhomax[first]
    elif ties != "order":
        raise ValueError(ties)
    logS = np.log(S)
    t = a - logS
    sigma = rhomax + gamma(n - 1) * (LD(1) + rhomax)
    dlog = -np.log1p(-sigma)                                   # item 4, from S
    rlog = LD(2) * U * (np.abs(logS) + dlog)                   # item 4, the allowance for log itself
    rsub = U * (np.abs(t) + delta + dlog + rlog)               # item 5
    tau = delta + dlog + rlog + rsub
    W = wl[:, None]
    return {"loglik": (W * t).sum(axis=0),
            "bound": (np.abs(W) * tau).sum(axis=0) + gamma(n + 1) * np.abs(W * t).sum(axis=0)}


def pair_counts(eta, time, status):
    """The exact counts on eta* (n, R), O(n^2): {"comparable": int, "concordant" / "discordant" / "tied_risk": (R,) int64}.
    A pair of positions k < l is comparable when status_k = 1 and time_k < time_l."""
    n, R = eta.shape
    order, _ = time_order(time)
    eta, t = eta[order], np.asarray(time, dtype=np.float64).reshape(-1)[order]
    ev = np.asarray(status).reshape(-1)[order] != 0
    cmp = ev[:, None] & (t[:, None] < t[None, :])  # (the sort makes l > k follow from time_k < time_l)
    out = {"comparable": int(cmp.sum()), "concordant": np.zeros(R, dtype=np.int64),
           "discordant": np.zeros(R, dtype=np.int64)}
    for r in range(R):
        out["concordant"][r] = int((cmp & (eta[:, r][:, None] > eta[:, r][None, :])).sum())
        out["discordant"][r] = int((cmp & (eta[:, r][:, None] < eta[:, r][None, :])).sum())
    out["tied_risk"] = out["comparable"] - out["concordant"] - out["discordant"]
    return out


def count_precondition(vals, cols, B, eta, delta, time, status, what=""):
    """Assert, on EVERY comparable pair of every model: the rows are identical on the model's support, or
    |eta*_k - eta*_l| > Delta_k + Delta_l.  Returns the smallest gap / required gap over the pairs that are not identical
    rows (inf when there is none)."""
    n, R = eta.shape
    order, _ = time_order(time)
    Xs = np.asarray(vals)[:, np.asarray(cols, dtype=np.int64).reshape(-1)][order]
    B = np.asarray(B, dtype=np.float64).reshape(Xs.shape[1], R)
    eta, delta = eta[order], delta[order]
    t = np.asarray(time, dtype=np.float64).reshape(-1)[order]
    ev = np.asarray(status).reshape(-1)[order] != 0
    cmp = ev[:, None] & (t[:, None] < t[None, :])
    worst = np.inf
    for r in range(R):
        gap = np.abs(eta[:, r][:, None] - eta[:, r][None, :])
        need = delta[:, r][:, None] + delta[:, r][None, :]
        close = cmp & ~(gap > need)
        sup = B[:, r] != 0.0
        for k, l in zip(*np.nonzero(close)):
            assert np.array_equal(Xs[k, sup], Xs[l, sup]), (
                what, "model %d: positions %d and %d are neither identical rows nor separated: choose other inputs"
                % (r, k, l))
        far = cmp & ~close
        if far.any():
            with np.errstate(divide="ignore"):
                worst = min(worst, float((gap[far] / need[far]).min()))
    return worst


def within(got, ref):
    """Per model: is the computed loglik inside the bound of the reference?  (A NaN is never inside.)"""
    got = np.asarray(got).astype(LD).reshape(-1)
    return np.abs(got - ref["loglik"]) <= ref["bound"]


def check_loglik(got, ref, what=""):
    """Print the figures, then assert the bound for every model."""
    got = np.asarray(got).astype(LD).reshape(-1)
    err = np.abs(got - ref["loglik"])
    worst = int(np.argmax(err - ref["bound"]))
    print("%s: at the worst model err %.3e against bound %.3e (loglik %.6e)" % (
        what, float(err[worst]), float(ref["bound"][worst]), float(ref["loglik"][worst])))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (err <= ref["bound"]).all(), (what, worst, float(err[worst]), float(ref["bound"][worst]))


def check_counts(got, ref, what=""):
    """The four counts of a result dict of capi.evaluate_cox_device (arrays) or evaluate_survival (ints) EQUAL ref's."""
    assert int(got["comparable"]) == ref["comparable"], (what, got["comparable"], ref["comparable"])
    for k in ("concordant", "discordant", "tied_risk"):
        assert np.array_equal(np.asarray(got[k], dtype=np.int64).reshape(-1), ref[k]), (what, k, got[k], ref[k])
