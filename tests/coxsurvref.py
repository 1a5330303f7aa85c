"""Extended-precision reference and error bound for the Breslow baseline cumulative hazard and the survival curves of
bessx_cox_baseline_device / bessx_cox_survival_device, capi.cox_baseline_device / cox_survival_device and
bess_base.fit_baseline / predict_survival (shared by tests/test_cox_surv_api.py and tests/test_cox_surv_gpu.py, in the
manner of tests/coxevalref.py, whose items 1 to 3 are used as they stand).

Definitions.  Positions, pi and first(k) as in coxevalref.  eta*_i = sum_j x(i, cols[j]) B[j], a* = clamp(eta*, -30, 30),
e* = exp(a*), S*(k) = sum_{l >= first(k)} e*(l) (the "breslow" risk set), h*(k) = w_k status_k / S*(k),
H*(k) = sum_{l <= k} h*(l); times = the distinct times that carry a row with status 1, H0*(g) = H* at the last position
with time times[g].  Curves: z*(i, j) = hg_j e*_i, survival exp(-z*), cumulative hazard z*.  NumPy in np.longdouble on the
host copy of the same (widened) values; the reference's own error is 2^-11 of every figure below and is not added.

The bound is derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u); Delta_i, rho_i and sigma_k are those of
coxevalref: |eta_hat - eta*| <= Delta_i, e_hat = e* (1 + r) with |r| <= rho_i = expm1(Delta_i) (1 + 2 u) + 2 u, and
S_hat = S* (1 + s) with |s| <= sigma_k = rhomax_k + gamma_{n-1} (1 + rhomax_k), rhomax_k the largest rho over the risk
set from first(k).  What the implementations compute on top of S_hat, each floating-point operation counted once (the
kernels of bessx_k_coxsurv.hip and the NumPy route of bess_base have the same form):

    wd     = w * status                 exact: status is 0 or 1
    h_hat  = wd / S_hat                 one division: h_hat = h* (1 + d) / (1 + s), |d| <= u, so
                                        |h_hat - h*| <= tau_k h*,  tau_k = (sigma_k + u) / (1 - sigma_k)
    H_hat  = sum of h_hat over the positions up to k: at most n NON-NEGATIVE terms, ADDITIONS ONLY, every term entering
             exactly once and none taken out again, so at most n - 1 additions in some order (Higham, section 4.2):
             gamma_{n-1} relative to the sum of the terms.  NumPy: a running sum.  Device (k_cxs_scan_tot /
             k_cxs_scan_apply): H = carry + (off + exc) + x_0 [+ x_1 [+ x_2 [+ x_3]]] in ascending position order, the form
             coxevalref lists for S.  (inclusive - own total is NOT such a sum: a term of 2^80 absorbs what came before it
             and the difference is 0.  test_cox_surv_gpu.py constructs that case.)
             |H_hat(k) - H*(k)| <= bH(k) = sum_{l <= k} tau_l h*(l) + gamma_{n-1} sum_{l <= k} (1 + tau_l) h*(l)
    z_hat  = hg_hat * e_hat             one multiplication; hg_hat = hg* + b with |b| <= bH (0 where hg is given data):
             |z_hat - z*| <= dz = e* (bH + hg* (rho_i + u))          (= z* (bH / H0* + rho_i + u); products of two
                                                                      of the small figures are dropped as in evalref)
    kind "cumhaz":    the bound is dz
    kind "survival":  exp(-z_hat) = exp(-z*) exp(z* - z_hat), the negation is exact and the computed exp carries a
             relative error of at most 2 u (1 ulp, the allowance of coxevalref item 2):
             |S_hat - S*| <= S* (expm1(dz) (1 + 2 u) + 2 u)

Gradual underflow.  The model fl(x) = x (1 + d), |d| <= u, and the "1 ulp = 2 u relative" of exp hold for results of at
least 2^-1022.  Below that fp64 is spaced TINY = 2^-1074 apart, so a rounding is an ABSOLUTE error of at most TINY / 2
and 1 ulp is TINY, however small the value: a survival of 1e-323 (z* about 743, which a fitted model reaches for its
highest risks at the last times) is correctly rounded with an error of up to 2.5e-324, which is 25% of it.  So the
product, unless it is an exact 0, carries TINY / 2 on top (dz = e* (bH + hg* (rho_i + u)) + TINY / 2), and the ulp of the computed exp is the
larger of the two statements.  With y = exp(-z_hat) <= S* (1 + expm1(dz)) the exact exp of the computed argument:
             |S_hat - S*| <= S* expm1(dz) + max(2 u S* (1 + expm1(dz)), TINY)
which is the line above wherever 2 u S* (1 + expm1(dz)) >= TINY, that is for every S* from 2^-1021 up.

hg = 0 gives z_hat = 0 and exp(-0) = 1 exactly: the bound is 2 u there and the tests ask for equality on top of it.

So that a loose bound cannot hide a failure, check_baseline and check_curves also assert, unless told that the case is
adversarial, that the bound itself is at most 1e-9 relative for H0 and for the cumulative hazard, and at most 1e-9
absolute for survival (with n <= 5000 and |eta| <= 5 the derivation gives about 1e-12).

self_check() holds baseline_reference to an independent O(n J) statement of the definition (for every event time the
rows with status 1 and time <= it, each over the sum of e over the rows with time >= its own) at n <= 200."""
import numpy as np

import coxevalref
import evalref

LD = np.longdouble
U = evalref.U
gamma = evalref.gamma
BOUND_CAP = 1e-9
TINY = LD(2.0) ** -1074  # the spacing of fp64 below 2^-1022


def _rho(delta):
    return np.expm1(delta) * (LD(1) + LD(2) * U) + LD(2) * U


def baseline_reference(eta, delta, time, status, w):
    """Reference and bound for one model: eta, delta (n,) or (n, 1) in row order from evalref.eta_reference (c = 0); time,
    status (n,); w (n,) or None.  Returns {"times": (J,) float64, "cumhaz": (J,) and "bound": (J,) longdouble}."""
    eta, delta = np.asarray(eta, dtype=LD).reshape(-1), np.asarray(delta, dtype=LD).reshape(-1)
    n = eta.size
    order, first = coxevalref.time_order(time)
    t = np.asarray(time, dtype=np.float64).reshape(-1)[order]
    eta, delta = eta[order], delta[order]
    d = np.asarray(status).astype(LD).reshape(-1)[order]
    wd = (np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)[order]) * d
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    S = np.cumsum(e[::-1])[::-1][first]
    rhomax = np.maximum.accumulate(_rho(delta)[::-1])[::-1][first]
    sigma = rhomax + gamma(n - 1) * (LD(1) + rhomax)
    tau = (sigma + U) / (LD(1) - sigma)
    h = wd / S
    H = np.cumsum(h)
    bH = np.cumsum(tau * h) + gamma(n - 1) * np.cumsum((LD(1) + tau) * h)
    ends = np.append(np.nonzero(first[1:] != first[:-1])[0], n - 1)
    event = np.array([bool((d[first[k]:k + 1] != 0).any()) for k in ends], dtype=bool)
    ends = ends[event]
    return {"times": t[ends].copy(), "cumhaz": H[ends], "bound": bH[ends]}


def brute_force_baseline(eta, time, status, w):
    """The definition stated row by row, O(n J), longdouble: (times, cumhaz)."""
    eta = np.asarray(eta, dtype=LD).reshape(-1)
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    status = np.asarray(status, dtype=np.float64).reshape(-1)
    w = np.ones(eta.size, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    times = np.unique(time[status != 0])
    cumhaz = np.zeros(times.size, dtype=LD)
    for g, tg in enumerate(times):
        for i in np.nonzero((status != 0) & (time <= tg))[0]:
            cumhaz[g] += w[i] / e[time >= time[i]].sum()
    return times, cumhaz


def curve_reference(eta, delta, hg, kind, hg_bound=None):
    """Reference and bound of the (n, T) curves: eta, delta (n,) or (n, 1) in row order; hg (T,) the baseline cumulative
    hazard at the requested times as the implementation is given it, or the exact one together with hg_bound (T,), the
    bound of what the implementation uses in its place.  Returns {"value": (n, T), "bound": (n, T)} in longdouble."""
    eta, delta = np.asarray(eta, dtype=LD).reshape(-1), np.asarray(delta, dtype=LD).reshape(-1)
    hg = np.asarray(hg).astype(LD).reshape(-1)
    bH = np.zeros(hg.size, dtype=LD) if hg_bound is None else np.asarray(hg_bound).astype(LD).reshape(-1)
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    z = e[:, None] * hg[None, :]
    dz = e[:, None] * (bH[None, :] + hg[None, :] * (_rho(delta) + U)[:, None]) + np.where(z > 0, TINY / LD(2), LD(0))
    if kind == "cumhaz":
        return {"value": z, "bound": dz, "kind": kind}
    if kind != "survival":
        raise ValueError(kind)
    s = np.exp(-z)
    grow = np.expm1(dz)
    return {"value": s, "bound": s * grow + np.maximum(LD(2) * U * s * (LD(1) + grow), TINY), "kind": kind}


def check_baseline(times, cumhaz, ref, what="", ordinary=True):
    """Print the figures, then assert: the times are the reference's bit for bit, every cumhaz is inside its bound, and
    (ordinary cases) the bound itself is at most 1e-9 of the value."""
    times, got = np.asarray(times, dtype=np.float64), np.asarray(cumhaz).astype(LD).reshape(-1)
    assert times.shape == ref["times"].shape and np.array_equal(times.view(np.int64), ref["times"].view(np.int64)), what
    if got.size == 0:
        print("%s: no event, nothing to compare" % what)
        return
    err = np.abs(got - ref["cumhaz"])
    worst = int(np.argmax(err - ref["bound"]))
    rel = ref["bound"] / np.where(ref["cumhaz"] > 0, ref["cumhaz"], LD(1))
    print("%s: J = %d, at the worst time err %.3e against bound %.3e (H0 %.6e); largest relative bound %.3e" % (
        what, got.size, float(err[worst]), float(ref["bound"][worst]), float(ref["cumhaz"][worst]), float(rel.max())))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (err <= ref["bound"]).all(), (what, worst, float(err[worst]), float(ref["bound"][worst]))
    if ordinary:
        assert float(rel.max()) <= BOUND_CAP, (what, "the bound is too loose for an ordinary case", float(rel.max()))


def check_curves(got, ref, what="", ordinary=True, rows=None):
    """Print the figures, then assert the bound for every element (of the rows given: a boolean mask, default all), and
    (ordinary cases) that the bound itself is at most 1e-9: absolute for survival, relative for the cumulative hazard."""
    got = np.asarray(got).astype(LD)
    assert got.shape == ref["value"].shape, (what, got.shape, ref["value"].shape)
    val, bnd = ref["value"], ref["bound"]
    if rows is not None:
        got, val, bnd = got[rows], val[rows], bnd[rows]
    err = np.abs(got - val)
    cap = bnd if ref["kind"] == "survival" else bnd / np.where(val > 0, val, LD(1))
    worst = np.unravel_index(int(np.argmax(err - bnd)), err.shape)
    print("%s: %s, at the worst element err %.3e against bound %.3e (value %.6e); largest bound %.3e" % (
        what, ref["kind"], float(err[worst]), float(bnd[worst]), float(val[worst]), float(cap.max())))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (err <= bnd).all(), (what, worst, float(err[worst]), float(bnd[worst]))
    if ordinary:
        assert float(cap.max()) <= BOUND_CAP, (what, "the bound is too loose for an ordinary case", float(cap.max()))


def self_check(seed=0):
    """baseline_reference against brute_force_baseline on small problems with ties, weights (some zero) and censoring."""
    rng = np.random.default_rng(seed)
    for n, weighted in ((1, False), (2, True), (37, False), (200, True)):
        eta = rng.normal(0.0, 1.5, n).astype(LD)
        time = np.round(rng.exponential(1.0, n), 1)  # (many ties)
        status = (rng.uniform(size=n) < 0.6).astype(np.float64)
        w = None
        if weighted:
            w = rng.integers(0, 9, n) / 4.0
        ref = baseline_reference(eta, np.zeros(n, dtype=LD), time, status, w)
        times, cumhaz = brute_force_baseline(eta, time, status, w)
        assert np.array_equal(ref["times"], times), (n, weighted)
        tol = LD(n + 2) * LD(2.0) ** -61 * np.maximum(cumhaz, LD(1e-300))
        assert (np.abs(ref["cumhaz"] - cumhaz) <= tol).all(), (n, weighted, ref["cumhaz"], cumhaz)
    return True
