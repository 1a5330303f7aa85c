"""Extended-precision reference and error bounds for bessx_cox_hazard_var_device / bessx_cox_band_device,
capi.cox_baseline_variance_device / cox_survival_band_device and bess_base.fit_survival_bands / predict_survival_bands
(shared by tests/test_cox_band_api.py and tests/test_cox_band_gpu.py), built on tests/coxinforef.py and
tests/coxdiagref.py, whose notation and items 1 to 6 and 13 it uses.

Definitions (position order; r(k), e*, wd, S0*, u*_k = S1*(k) / S0*(k): coxinforef).  For a grid time tau let K(tau) be
the positions with time <= tau:
    cumhaz*(tau) = sum_K wd_k / S0*(k)     var0*(tau) = sum_K wd_k / S0*(k)^2     drift*(tau) = sum_K (wd_k / S0*(k)) u*_k
hazard_var_reference states them by the EXPLICIT risk-set definition: for every event position k it re-sums its risk set
{l >= r(k)} for S0 and S1 (no scans, no running sums) and then adds the terms of K(tau) for every tau.  For a row with
z = x[cols], e*_x = exp(clamp(z . beta)), R the lower-triangular fp64 matrix both routes are given (DATA, like coxdiagref's
R), t* = tril(R) z and p*_tau = tril(R) drift(tau):
    V* = var0 + sum_j (p*_j - cumhaz t*_j)^2,   L* = cumhaz e*_x,   seL* = e*_x sqrt(V*),   w* = z_c seL*,
    r* = z_c sqrt(V*) / cumhaz
    cumhaz:    estimate L*, se seL*; plain max(L* - w*, 0), L* + w*; log L* exp(-+ r*)
    survival:  estimate S* = exp(-L*), se S* seL*; plain clamp(S* -+ z_c S* seL*, 0, 1); log exp(-(L* + w*)),
               exp(-max(L* - w*, 0)); log-log exp(-L* exp(+- r*))
    cumhaz = 0: se = 0 and both bounds are the estimate.
NumPy in np.longdouble on the host copy of the same (widened) values; the reference's own error is 2^-11 of every figure
below and is not added.  self_check() holds hazard_var_reference to the running-sum decomposition of coxinforef /
coxdiagref, and V to var0 + q^T (R^T R) q with q = drift - z cumhaz.

The bounds are derived, not measured.  u = 2^-53, gamma_k as in evalref; rho_l, rho, sigma, tau, eta_H, rw, sig1, ru, a_kc:
coxinforef items 1 to 6; rinc, rA, Abar: coxdiagref item 13.  A fused multiply-add has fewer roundings than the two
operations the bounds count.  Weights are non-negative.

B1. cumhaz is H of coxinforef item 3 at the last position of K(tau): |H_hat - H*| <= eta_H H*.
B2. var0.  S0_hat^2 (1 r) and the division (1 r): an increment is within tau2 = (1 + u) / ((1 - sigma)^2 (1 - u)) - 1 of
    wd / S0*^2; the tie group's additions and the scan are additions of non-negative terms only, at most n - 1 of them in
    some order: |var0_hat - var0*| <= eta_V var0*, eta_V = tau2 + gamma_{n-1} (1 + tau2).
B3. drift is A of coxdiagref item 13 at the last position of K(tau): |drift_hat_c - drift*_c| <= rA Abar_c(tau),
    Abar_c = sum_K h*_k a_kc.
B4. t_j = sum_{c <= j} R_jc z_c with z exact: a dot product with an addition chain of depth `dot` (device: ceil(m / 4)
    k-steps of four products plus 4, host: m), products rounded at most once: dt_j = gamma_{dot+1} (|R| |z|)_j.
    p_j = sum_{c <= j} R_jc drift_hat_c in plain fp64 loops, depth m, from a drift that is data (bD = 0) or carries B3's
    bound: dp_j = (1 + gamma_{m+1}) (|R| bD)_j + gamma_{m+1} (|R| |drift*|)_j.
B5. d_j = p_j - H t_j, a = H t: |a_hat - a*| <= e1 = H* dt + bH (|t*| + dt); the product (1 r) and the subtraction (1 r):
        dd_j = (1 + u) (dp_j + (1 + u) e1_j + u |a*_j|) + u (|p*_j| + |a*_j|).
    The difference may cancel (p is about H R xbar for columns that are not centred): dd is relative to |p| + |a|, not to
    |d|.  It enters V once, squared -- the expanded form would carry u (|p|^2 + H^2 |t|^2) instead.
B6. V = var0 + sum_j d_j^2: |d_hat^2 - d*^2| <= (2 |d*| + dd) dd, the squares (1 r, none when fused), an addition chain
    of depth `sum` (device: the tiles' squares per lane, 4 levels of the DPP tree, ceil(m / 16) + 4; host: m) and one
    addition of var0, non-negative terms only:
        bV = (1 + gamma_{sum+2}) (sum_j (2 |d*_j| + dd_j) dd_j + bV0) + gamma_{sum+2} V*.
B7. sq = sqrt(V) (1 r): bsq = (1 + u) min(sqrt(bV), bV / sqrt(V*)) + u sqrt(V*).  e_hat = e* (1 + r), |r| <= rho_i.
        L = H e (1 r):        bL   = e* (bH + H* (rho_i + u)) + TINY / 2                     (coxsurvref's dz)
        seL = e sq (1 r):     bseL = (1 + u) (e* (1 + rho_i) bsq + rho_i e* sq*) + u e* sq*
        w = z_c seL (1 r):    bw   = (1 + u) z_c bseL + u w*
        r = (z_c sq) / H:     bnum = (1 + u) z_c bsq + u z_c sq*,   br = (1 + u) (bnum + r* bH) / (H* - bH) + u r*
B8. exp is allowed 1 ulp = 2 u: for |x_hat - x*| <= bx, |exp_hat - exp(x*)| <= exp(x*) (expm1(bx) (1 + 2 u) + 2 u) =: exp(x*)
    rex(bx); for a survival-type value exp(-x) coxsurvref's statement with gradual underflow,
        bneg(x*, bx) = exp(-x*) expm1(bx) + max(2 u exp(-x*) (1 + expm1(bx)), TINY).
    A sum or difference of two computed values (1 r) carries (1 + u) (b1 + b2) + u |value*|; max(., 0) and the clamp to
    [0, 1] do not increase a distance to a reference that is clamped the same way.  A product g = L exp(+-r) (1 r):
        bg = (1 + u) (bL E* (1 + rex(br)) + L* E* rex(br)) + u L* E*,   E* = exp(+-r*).
    So: cumhaz estimate bL, se bseL, plain (1 + u) (bL + bw) + u |L* -+ w*|, log bg; survival estimate bneg(L*, bL), se
    (1 + u) (bS (seL* + bseL) + S* bseL) + u S* seL*, plain with ws = z_c se (1 r), bws = (1 + u) z_c bse + u ws*:
    (1 + u) (bS + bws) + u |S* -+ ws*|; log bneg(L* +- w*, (1 + u) (bL + bw) + u |L* +- w*|); log-log bneg(g*, bg).
    cumhaz = 0 (as data, or before the first event where the computed cumhaz is an exact 0 too): the bound is 0 for se
    and the bounds equal the estimate's bound.

So that a loose bound cannot hide a failure, every check also asserts, unless told that the case is adversarial, that the
bound itself is at most 1e-9: relative to the value for cumhaz, var0 and the cumulative-hazard outputs, relative to
Abar for drift (a sum of either sign), relative to V* for V, absolute for the survival outputs (which lie in [0, 1])."""
import numpy as np

import coxdiagref
import coxinforef
import evalref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
BOUND_CAP = 1e-9
TINY = LD(2.0) ** -1074
WHAT = ("estimate", "se", "lower", "upper")


def device_depths(m):
    """(dot, sum) of items B4 and B6 for a device call, as bessx_k_coxband.hip states them."""
    return (int(m) + 3) // 4 + 4, (int(m) + 15) // 16 + 4


def host_depths(m):
    """(dot, sum) of the NumPy route: running sums over m columns."""
    return max(int(m), 1), max(int(m), 1)


def hazard_var_reference(vals, cols, beta, time, status, w, ties, times):
    """Reference and bounds of step 1 by the explicit risk-set definition.  vals: the (widened) n x p values; cols, beta
    (m,); time, status (n,); w (n,) or None; ties; times (T,).  Returns longdouble arrays cumhaz, var0 (T,), drift (T, m),
    their bounds under *_bound, Abar (T, m) and n_events."""
    x, eta, delta, wd, d, order, first, last, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
    assert (wd >= 0).all(), "the bounds are derived for non-negative weights"
    n, m = x.shape
    one = LD(1)
    if ties not in ("order", "breslow"):
        raise ValueError(ties)
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    r = first if ties == "breslow" else np.arange(n)
    W, Wa = e[:, None] * x, e[:, None] * np.abs(x)
    h, v, hu, ha = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros((n, m), dtype=LD), np.zeros((n, m), dtype=LD)
    seen = {}
    for k in np.nonzero(d != 0)[0]:  # every event position re-sums its risk set
        rk = int(r[k])
        if rk not in seen:
            S0 = e[rk:].sum()
            seen[rk] = (S0, W[rk:].sum(axis=0) / S0, Wa[rk:].sum(axis=0) / S0)
        S0, u, a = seen[rk]
        h[k], v[k] = wd[k] / S0, wd[k] / (S0 * S0)
        hu[k], ha[k] = h[k] * u, h[k] * a
    t = np.asarray(time, dtype=np.float64).reshape(-1)[order]
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    cnt = np.searchsorted(t, times, side="right")
    cumhaz = np.array([h[:c].sum() for c in cnt], dtype=LD)
    var0 = np.array([v[:c].sum() for c in cnt], dtype=LD)
    drift = np.array([hu[:c].sum(axis=0) for c in cnt], dtype=LD).reshape(times.size, m)
    Abar = np.array([ha[:c].sum(axis=0) for c in cnt], dtype=LD).reshape(times.size, m)
    rho = (np.expm1(delta) * (one + LD(2) * U) + LD(2) * U).max()                     # coxinforef items 1 to 3, 6
    sigma = rho + gamma(n - 1) * (one + rho)
    tau = (sigma + U) / (one - sigma)
    eta_h = tau + gamma(n - 1) * (one + tau)
    tau2 = (one + U) / ((one - sigma) ** 2 * (one - U)) - one                          # B2
    eta_v = tau2 + gamma(n - 1) * (one + tau2)
    rw = (one + rho) * (one + U) - one
    sig1 = rw + gamma(n - 1) * (one + rw)
    ru = (one + sig1) * (one + U) / (one - sigma) - one
    rinc = (one + ru) * (one + eta_h) * (one + U) - one                               # coxdiagref item 13
    rA = rinc + (one + rinc) * gamma(n - 1)
    return {"cumhaz": cumhaz, "cumhaz_bound": eta_h * cumhaz, "var0": var0, "var0_bound": eta_v * var0, "drift": drift,
            "drift_bound": rA * Abar, "Abar": Abar, "n_events": wd.sum(), "rel": max(eta_h, eta_v, rA)}


def check_hazard_var(got, ref, what="", ordinary=True, factor=1):
    """Print the figures, then assert cumhaz, var0 and drift against their bounds (times `factor` when two computed
    results are compared) and, for ordinary cases, that the bounds are at most 1e-9 of their masses."""
    for k in ("cumhaz", "var0", "drift"):
        g = np.asarray(got[k]).astype(LD)
        assert g.shape == ref[k].shape, (what, k, g.shape, ref[k].shape)
        if g.size == 0:
            continue
        err, bnd = np.abs(g - ref[k]), factor * ref[k + "_bound"]
        worst = np.unravel_index(int(np.argmax(err - bnd)), err.shape)
        print("%s: %s err %.3e against bound %.3e (value %.6e)" % (what, k, float(err[worst]), float(bnd[worst]),
                                                                     float(ref[k][worst])))
        assert np.isfinite(np.asarray(g, dtype=np.float64)).all(), (what, k)
        assert (err <= bnd).all(), (what, k, worst, float(err[worst]), float(bnd[worst]))
        zero = ref[k + "_bound"] == 0  # (an exact zero: before the first time, or no event)
        assert (g[zero] == 0).all(), (what, k, "an exact zero is expected")
    print("%s: relative bound %.3e" % (what, float(ref["rel"])))
    if ordinary:
        assert float(ref["rel"]) <= BOUND_CAP, (what, "the bound is too loose for an ordinary case", float(ref["rel"]))


def _rex(bx):
    return np.expm1(bx) * (LD(1) + LD(2) * U) + LD(2) * U


def _bneg(x, bx):
    s, grow = np.exp(-x), np.expm1(bx)
    return s * grow + np.maximum(LD(2) * U * s * (LD(1) + grow), TINY)


def band_reference(vals, cols, beta, cumhaz, var0, drift, R, kind, conf_type, zc, depths, in_bounds=None):
    """Reference and bounds of step 2.  vals: the (widened) n x p values; cols, beta (m,); cumhaz, var0 (T,), drift (T, m),
    R (m, m): the fp64 data both routes are given -- or the exact longdouble values together with in_bounds = (bH, bV0, bD),
    the bounds of what the implementation uses in their place.  depths = (dot, sum).  Returns longdouble (n, T) arrays:
    V, V_bound and every output of WHAT with its bound under name + "_bound"."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    m = cols.size
    one, two = LD(1), LD(2)
    eta, delta = evalref.eta_reference(vals, cols, np.asarray(beta, dtype=np.float64).reshape(m, 1), [0.0])
    eta, delta = eta[:, 0].astype(LD), delta[:, 0].astype(LD)
    n = eta.size
    e = np.exp(np.clip(eta, LD(-30), LD(30)))[:, None]
    rho = (np.expm1(delta) * (one + two * U) + two * U)[:, None]
    H, V0 = np.asarray(cumhaz).astype(LD).reshape(1, -1), np.asarray(var0).astype(LD).reshape(1, -1)
    T = H.size
    D = np.asarray(drift).astype(LD).reshape(T, m)
    if in_bounds is None:
        bH, bV0, bD = np.zeros((1, T), dtype=LD), np.zeros((1, T), dtype=LD), np.zeros((T, m), dtype=LD)
    else:
        bH, bV0, bD = (np.asarray(b).astype(LD) for b in in_bounds)
        bH, bV0, bD = bH.reshape(1, T), bV0.reshape(1, T), bD.reshape(T, m)
    dot, sdepth = depths
    z = np.asarray(vals)[:, cols].astype(LD)
    Rl = np.tril(np.asarray(R, dtype=np.float64).reshape(m, m)).astype(LD)
    aR = np.abs(Rl)
    gd, gm, gs = gamma(dot + 1), gamma(m + 1), gamma(sdepth + 2)
    S, bS2 = np.zeros((n, T), dtype=LD), np.zeros((n, T), dtype=LD)
    for j in range(m):                                                               # B4 to B6, one column at a time
        tj, dtj = (z @ Rl[j])[:, None], (gd * (np.abs(z) @ aR[j]))[:, None]
        pj, dpj = (D @ Rl[j])[None, :], ((one + gm) * (bD @ aR[j]) + gm * (np.abs(D) @ aR[j]))[None, :]
        a = H * tj
        e1 = H * dtj + bH * (np.abs(tj) + dtj)
        dd = (one + U) * (dpj + (one + U) * e1 + U * np.abs(a)) + U * (np.abs(pj) + np.abs(a))
        dj = pj - a
        S += dj * dj
        bS2 += (two * np.abs(dj) + dd) * dd
    V = V0 + S
    bV = (one + gs) * (bS2 + bV0) + gs * V
    sq = np.sqrt(V)                                                                  # B7
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = np.where(sq > 0, bV / np.where(sq > 0, sq, one), np.inf)
    bsq = (one + U) * np.minimum(np.sqrt(bV), quot) + U * sq
    L = H * e
    bL = e * (bH + H * (rho + U)) + np.where(L > 0, TINY / two, LD(0))
    seL = e * sq
    bseL = (one + U) * (e * (one + rho) * bsq + rho * e * sq) + U * seL
    w = zc * seL
    bw = (one + U) * zc * bseL + U * w
    pos = np.broadcast_to(H > 0, L.shape)
    Hs = np.where(H > 0, H, one)
    assert (bH < Hs)[H > 0].all(), "cumhaz is not separated from zero by its bound"
    r = zc * sq / Hs
    bnum = (one + U) * zc * bsq + U * zc * sq
    br = (one + U) * (bnum + r * bH) / (Hs - bH) + U * r

    def prod(sign):  # L exp(sign r) and its bound
        E = np.exp(sign * r)
        return L * E, (one + U) * (bL * E * (one + _rex(br)) + L * E * _rex(br)) + U * L * E

    def pm(a, ba, b, bb, sign):  # a + sign b of two computed values
        v = a + sign * b
        return v, (one + U) * (ba + bb) + U * np.abs(v)

    out = {"V": V, "V_bound": bV, "kind": kind}
    if kind == "cumhaz":
        est, best, se, bse = L, bL, seL, bseL
        if conf_type == "plain":
            lo, blo = pm(L, bL, w, bw, -1)
            lo = np.where(lo < 0, LD(0), lo)
            hi, bhi = pm(L, bL, w, bw, +1)
        elif conf_type == "log":
            (lo, blo), (hi, bhi) = prod(-1), prod(+1)
        else:
            raise ValueError(conf_type)
    elif kind == "survival":
        est, best = np.exp(-L), _bneg(L, bL)
        se = est * seL
        bse = (one + U) * (best * (seL + bseL) + est * bseL) + U * se
        if conf_type == "plain":
            ws = zc * se
            bws = (one + U) * zc * bse + U * ws
            lo, blo = pm(est, best, ws, bws, -1)
            hi, bhi = pm(est, best, ws, bws, +1)
            lo, hi = np.where(lo < 0, LD(0), lo), np.where(hi > 1, LD(1), hi)
        elif conf_type == "log":
            a, ba = pm(L, bL, w, bw, +1)
            lo, blo = np.exp(-a), _bneg(a, ba)
            a, ba = pm(L, bL, w, bw, -1)
            a = np.where(a < 0, LD(0), a)
            hi, bhi = np.exp(-a), _bneg(a, ba)
        elif conf_type == "log-log":
            g, bg = prod(+1)
            lo, blo = np.exp(-g), _bneg(g, bg)
            g, bg = prod(-1)
            hi, bhi = np.exp(-g), _bneg(g, bg)
        else:
            raise ValueError(conf_type)
    else:
        raise ValueError(kind)
    zero = LD(0)
    out.update(estimate=est, estimate_bound=best, se=np.where(pos, se, zero), se_bound=np.where(pos, bse, zero),
               lower=np.where(pos, lo, est), lower_bound=np.where(pos, blo, best), upper=np.where(pos, hi, est),
               upper_bound=np.where(pos, bhi, best))
    return out


def check_bands(got, ref, names, what="", ordinary=True, rows=None, factor=1):
    """Print the figures, then assert every output of `names` (got: a dict of (n, T) arrays) against its bound, for the
    rows given (a boolean mask, default all); ordinary cases: the bound of V is at most 1e-9 of V and the bound of every
    output at most 1e-9 (absolute for survival, relative for the cumulative hazard)."""
    sel = slice(None) if rows is None else rows
    V, bV = ref["V"][sel], ref["V_bound"][sel]
    relV = float((bV / np.where(V > 0, V, LD(1))).max())
    print("%s: largest bound of V relative to V %.3e" % (what, relV))
    if ordinary:
        assert relV <= BOUND_CAP, (what, "the bound of V is too loose for an ordinary case", relV)
    for k in names:
        g = np.asarray(got[k]).astype(LD)
        assert g.shape == ref[k].shape, (what, k, g.shape, ref[k].shape)
        g, val, bnd = g[sel], ref[k][sel], factor * ref[k + "_bound"][sel]
        err = np.abs(g - val)
        cap = bnd if ref["kind"] == "survival" else bnd / np.where(val > 0, val, LD(1))
        worst = np.unravel_index(int(np.argmax(err - bnd)), err.shape)
        print("%s: %s %s err %.3e against bound %.3e (value %.6e); largest bound %.3e" % (
            what, ref["kind"], k, float(err[worst]), float(bnd[worst]), float(val[worst]), float(cap.max())))
        assert np.isfinite(np.asarray(g, dtype=np.float64)).all(), (what, k)
        assert (err <= bnd).all(), (what, k, worst, float(err[worst]), float(bnd[worst]))
        if ordinary:
            assert float(cap.max()) <= factor * BOUND_CAP, (what, k, "the bound is too loose for an ordinary case",
                                                            float(cap.max()))


def self_check(seed=0):
    """hazard_var_reference against the running-sum decomposition of coxinforef / coxdiagref, and V against
    var0 + q^T (R^T R) q, on small problems with ties, weights (some zero) and censoring."""
    rng = np.random.default_rng(seed)
    for n, m, weighted, ties in ((1, 1, False, "breslow"), (2, 0, True, "order"), (37, 3, False, "breslow"),
                                 (200, 5, True, "order"), (150, 4, True, "breslow")):
        X = rng.standard_normal((n, m + 2))
        cols = np.arange(m, dtype=np.int64)
        beta = rng.normal(0.0, 0.5, m)
        time = np.round(rng.exponential(1.0, n), 1)  # (many ties)
        status = (rng.uniform(size=n) < 0.6).astype(np.float64)
        status[0] = 1.0
        w = rng.integers(0, 9, n) / 4.0 if weighted else None
        times = np.concatenate([[time.min() - 1.0, time.max() + 1.0], rng.choice(time, 5), rng.uniform(0, 2, 5)])
        ref = hazard_var_reference(X, cols, beta, time, status, w, ties, times)
        x, eta, delta, wd, d, order, first, last, _ = coxinforef._ordered(X, cols, beta, time, status, w)
        dec = coxinforef._decomposition(x, eta, wd, d, first, last, ties)
        Hrun = np.cumsum(wd / dec["S0"])
        Vrun = np.cumsum(wd / (dec["S0"] * dec["S0"]))
        Arun = np.cumsum((wd / dec["S0"])[:, None] * dec["u"], axis=0)
        idx = np.searchsorted(time[order], times, side="right") - 1
        tol = LD(n + 4) * LD(2.0) ** -60
        for got, run in ((ref["cumhaz"], Hrun), (ref["var0"], Vrun), (ref["drift"], Arun)):
            want = np.where((idx >= 0).reshape((-1,) + (1,) * (run.ndim - 1)), run[np.maximum(idx, 0)], LD(0))
            scale = np.abs(want) + (ref["Abar"] if run.ndim == 2 else LD(0)) + LD(1e-300)
            assert (np.abs(got - want) <= tol * scale).all(), (n, m, ties)
        if m == 0:
            continue
        R = np.tril(rng.standard_normal((m, m))) + 2.0 * np.eye(m)
        b = band_reference(X, cols, beta, ref["cumhaz"], ref["var0"], ref["drift"], R, "survival", "log-log", 1.96,
                           host_depths(m), in_bounds=(0 * ref["cumhaz"], 0 * ref["var0"], 0 * ref["drift"]))
        C = R.astype(LD).T @ R.astype(LD)
        q = ref["drift"][None, :, :] - X[:, None, :m].astype(LD) * ref["cumhaz"][None, :, None]
        V = ref["var0"][None, :] + np.einsum("itj,jk,itk->it", q, C, q)
        mass = ref["var0"][None, :] + np.einsum("itj,jk,itk->it", np.abs(q), np.abs(C), np.abs(q))
        assert (np.abs(b["V"] - V) <= LD(8 * m * m) * LD(2.0) ** -60 * (mass + LD(1e-300))).all(), (n, m, ties)
    return True
