"""Extended-precision reference and error bounds for bessx_cox_diag_device / capi.cox_diagnostics_device /
bess_base.diagnostics_survival (shared by tests/test_cox_diag_api.py and tests/test_cox_diag_gpu.py), built on
tests/coxinforef.py, whose notation and items 1 to 6 it continues.

Definitions (position order; r(k), e*, wd, S0*, u*_k = S1*(k) / S0*(k), H*, v*, g*: coxinforef).  With h*_k = wd_k / S0*(k),
    A*_l = sum_{k : r(k) <= l} h*_k u*_k          (= sum_{p <= l} dh_p u_p with dh_p = sum_{k : r(k) = p} h_k)
    martingale   g*_k
    deviance     sign(g*_k) sqrt(2 max(v*_k - wd_k + wd_k log(wd_k / v*_k), 0)),  0 log 0 = 0, sign(0) = 0
    score        L*_k = g*_k x_k - wd_k u*_k + e*_k A*_k
    dfbeta       L*_k C                           (C: the fp64 matrix both routes are given)
    displacement sum_j t*_kj^2,  t*_k = tril(R) L*_k    (R: the fp64 matrix both routes are given)
    schoenfeld   x_k - u*_k for the rows with status = 1, position order
C and R are DATA: dfbeta and displacement are tested with the same C and R passed to the code under test, so the
conditioning of the information matrix does not enter.  self_check() holds the decomposition of L, at n <= 300, to
    L_k = wd_k (x_k - u_k) - e_k sum_{j : r(j) <= k} (wd_j / S0(j)) (x_k - u_j)
with every u_j summed directly, sum_k L_k to coxinforef's score, sum_k g_k to its residual and displacement to
L C L^T with a longdouble inverse.

The bounds are derived, not measured.  u = 2^-53, gamma_k as in evalref, "(1 r)" one rounding; a fused multiply-add has
fewer roundings than the two operations the bounds count.  rho_l, sigma, tau, eta_H, rv_l, dg_l, ru and a_kc are
coxinforef's items 1 to 6.

11. martingale: |g_hat - g*| <= dg_l (item 4).
12. deviance.  t1 = v_hat - wd (1 r): e1 = rv v* + u (|v* - wd| + rv v*).  q = wd / v_hat (1 r) is within rq = (rv + u) /
    (1 - rv) of wd / v*, so log moves by at most dl = rq / (1 - rq) and carries 1 ulp = 2 u of its own: el = dl + 2 u
    (|log*| + dl).  t2 = wd * log (1 r): e2 = wd el (1 + u) + u wd |log*|.  dd = t1 + t2 (1 r): bdd = (e1 + e2) (1 + u) +
    u |dd*|.  a = 2 max(dd, 0) (exact doubling; max does not increase a distance as dd* >= 0): ba = 2 bdd.  The square
    root (1 r): bs = (1 + u) min(sqrt(ba), ba / sqrt(a*)) + u sqrt(a*).  Where |g*| > dg the sign is that of g* and the
    bound is bs; in the neighbourhood of g = 0 (|g*| <= dg) either sign may come out and the bound is the absolute
    term 2 sqrt(a*) + bs.
13. A.  dh is h (item 3, relative tau) or a sum of a tie group's h, additions only: relative eta_H covers both.  An
    increment dh_hat u_hat (1 r) is within dh* a_pc rinc of dh* u*, rinc = (1 + ru) (1 + eta_H) (1 + u) - 1; A is a sum
    of at most n increments, n - 1 additions in some order whatever the blocks of the scan are:
        |A_hat_lc - A*_lc| <= rA Abar_lc,   Abar_lc = sum_{k : r(k) <= l} h*_k a_kc,   rA = rinc + (1 + rinc) gamma_{n-1}.
14. L is a sum of three terms.  g_hat x (1 r): |x| dg (1 + u) + u |g* x|.  wd u_hat (1 r): wd a (ru (1 + u) + u).
    e_hat A_hat (1 r): e* Abar ((1 + rho_l) (1 + rA) (1 + u) - 1).  Two additions:
        bL_kc = (1 + gamma_2) (sum of the three) + gamma_2 mass_kc,   mass_kc = |g*_k x_kc| + wd_k a_kc + e*_k Abar_kc.
    The bound is relative to mass, not to |L|: L is a difference.  Self-check: max bL / mass < coxinforef.REL_CEILING for
    every input a test uses (asserted), so a bound cannot grow until it hides a failure.
15. dfbeta_kj = sum_c L_hat_kc C_cj, a dot product of length m with an addition chain of depth `dot` (the device's matrix
    instruction adds four products per k-step: ceil(m / 4) steps plus 4 for the additions inside a step, stated by
    device_depths(); host: m), products rounded at most once:
        |dfbeta_hat - dfbeta*| <= (1 + gamma_{dot+1}) sum_c |C_cj| bL_kc + gamma_{dot+1} sum_c |C_cj L*_kc|.
16. displacement: t_kj = sum_{c <= j} R_jc L_hat_kc as item 15: delta_kj = (1 + gamma_{dot+1}) sum_c |R_jc| bL_kc +
    gamma_{dot+1} sum_c |R_jc L*_kc|; |t_hat^2 - t*^2| <= (2 |t*| + delta) delta; the squares (1 r, none when fused) and
    `sum` additions (device: the tiles' squares per lane, then 4 levels of the DPP tree, ceil(m / 16) + 4; host: m):
        |S_hat - S*| <= (1 + gamma_{sum+1}) sum_j (2 |t*_kj| + delta_kj) delta_kj + gamma_{sum+1} S*.
17. schoenfeld = x - u_hat (1 r): a ru (1 + u) + u |x - u*|.
18. Sums the tests take of the results in fp64 NumPy over n terms add gamma_n of the summed magnitudes; the tests state
    them where they use them."""
import numpy as np

import coxinforef
import evalref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = coxinforef.REL_CEILING
KINDS = ("martingale", "deviance", "score", "dfbeta", "displacement", "schoenfeld")


def device_depths(m):
    """(dot, sum) of items 15 and 16 for a device call: functions of m alone, as bessx_k_coxdiag.hip states them."""
    return (int(m) + 3) // 4 + 4, (int(m) + 15) // 16 + 4


def host_depths(m):
    """(dot, sum) of the NumPy route: running sums over m columns."""
    return max(int(m), 1), max(int(m), 1)


def _accumulated(dec, wd, last, ties, weight_by=None):
    """A (n, m) of a decomposition: sum over {k : r(k) <= l} of h_k * z_k, z = u (or weight_by)."""
    z = dec["u"] if weight_by is None else weight_by
    h = wd / dec["S0"]
    A = np.cumsum(h[:, None] * z, axis=0)
    return A[last] if ties == "breslow" else A


def _xlogy(w, v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w == 0, LD(0), w * np.log(np.where(w == 0, LD(1), w) / np.where(w == 0, LD(1), v)))


def cox_diag_reference(vals, cols, beta, time, status, w, ties, R, C, depths):
    """Reference and bounds of one call.  vals: the (widened) n x p values; cols, beta (m,); time, status (n,); w (n,) or
    None; ties; R, C (m, m) fp64 or None (then displacement / dfbeta are left out); depths = (dot, sum).  Returns a dict
    of longdouble arrays in ROW order (schoenfeld in position order), each kind k with its bound under k + "_bound", plus
    event_rows, event_times, rel (the largest bL / mass), wd (row order) and m."""
    x, eta, delta, wd, d, order, first, last, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
    assert (wd >= 0).all(), "the bounds are derived for non-negative weights"
    n, m = x.shape
    dot, sdepth = depths
    dec = coxinforef._decomposition(x, eta, wd, d, first, last, ties)
    e, r, S0, v, g, u, ev = dec["e"], dec["r"], dec["S0"], dec["v"], dec["g"], dec["u"], dec["ev"]
    one = LD(1)
    rho_l = np.expm1(delta) * (one + LD(2) * U) + LD(2) * U                 # coxinforef items 1 to 4
    rho = rho_l.max()
    sigma = rho + gamma(n - 1) * (one + rho)
    tau = (sigma + U) / (one - sigma)
    eta_h = tau + gamma(n - 1) * (one + tau)
    rv = (one + rho_l) * (one + eta_h) * (one + U) - one
    dg = rv * v + U * (np.abs(g) + rv * v)

    def rows(z):
        out = np.empty_like(z)
        out[order] = z
        return out

    out = {"m": m, "event_rows": order[ev], "event_times": np.asarray(time, dtype=np.float64)[order][ev],
           "wd": rows(wd), "martingale": rows(g), "martingale_bound": rows(dg)}                            # item 11
    lg = _xlogy(wd, v) / np.where(wd == 0, one, wd)                                                         # item 12
    dd = (v - wd) + wd * lg
    dd = np.where(dd < 0, LD(0), dd)
    e1 = rv * v + U * (np.abs(v - wd) + rv * v)
    rq = (rv + U) / (one - rv)
    dl = rq / (one - rq)
    el = dl + LD(2) * U * (np.abs(lg) + dl)
    e2 = wd * el * (one + U) + U * wd * np.abs(lg)
    bdd = (e1 + e2) * (one + U) + U * dd
    a_, ba = LD(2) * dd, LD(2) * bdd
    sa = np.sqrt(a_)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = np.where(sa > 0, ba / np.where(sa > 0, sa, one), np.inf)
    bs = (one + U) * np.minimum(np.sqrt(ba), quot) + U * sa
    out["deviance"] = rows(np.sign(g) * sa)
    out["deviance_bound"] = rows(np.where(np.abs(g) > dg, bs, LD(2) * sa + bs))
    if m == 0:
        z = np.zeros((n, 0), dtype=LD)
        out.update(score=z, score_bound=z, dfbeta=z, dfbeta_bound=z, displacement=np.zeros(n, dtype=LD),
                   displacement_bound=np.zeros(n, dtype=LD), schoenfeld=np.zeros((int(ev.sum()), 0), dtype=LD),
                   schoenfeld_bound=np.zeros((int(ev.sum()), 0), dtype=LD), rel=LD(0), mass=z)
        return out
    ax = np.abs(x)
    rw = (one + rho) * (one + U) - one                                                                      # item 6
    sig1 = rw + gamma(n - 1) * (one + rw)
    ru = (one + sig1) * (one + U) / (one - sigma) - one
    a = np.cumsum((e[:, None] * ax)[::-1], axis=0)[::-1][r] / S0[:, None]
    A = _accumulated(dec, wd, last, ties)                                                                   # item 13
    Abar = _accumulated(dec, wd, last, ties, weight_by=a)
    rinc = (one + ru) * (one + eta_h) * (one + U) - one
    rA = rinc + (one + rinc) * gamma(n - 1)
    L = g[:, None] * x - wd[:, None] * u + e[:, None] * A                                                   # item 14
    t1 = ax * dg[:, None] * (one + U) + U * np.abs(g[:, None] * x)
    t2 = wd[:, None] * a * (ru * (one + U) + U)
    t3 = e[:, None] * Abar * ((one + rho_l[:, None]) * (one + rA) * (one + U) - one)
    mass = np.abs(g[:, None] * x) + wd[:, None] * a + e[:, None] * Abar
    bL = (one + gamma(2)) * (t1 + t2 + t3) + gamma(2) * mass
    pos = mass > 0
    rel = (bL[pos] / mass[pos]).max() if pos.any() else LD(0)
    assert rel < REL_CEILING, ("the derived bound exceeds its ceiling: choose other inputs", float(rel))
    out.update(score=rows(L), score_bound=rows(bL), rel=rel, mass=rows(mass))
    out["schoenfeld"] = x[ev] - u[ev]                                                                       # item 17
    out["schoenfeld_bound"] = a[ev] * (ru * (one + U) + U) + U * np.abs(out["schoenfeld"])
    aL = np.abs(L)
    if C is not None:                                                                                       # item 15
        Cl = np.asarray(C, dtype=np.float64).astype(LD)
        gd = gamma(dot + 1)
        out["dfbeta"] = rows(L @ Cl)
        out["dfbeta_bound"] = rows((one + gd) * (bL @ np.abs(Cl)) + gd * (aL @ np.abs(Cl)))
    if R is not None:                                                                                       # item 16
        Rl = np.tril(np.asarray(R, dtype=np.float64)).astype(LD)
        gd, gs = gamma(dot + 1), gamma(sdepth + 1)
        T = L @ Rl.T
        dt = (one + gd) * (bL @ np.abs(Rl).T) + gd * (aL @ np.abs(Rl).T)
        S = (T * T).sum(axis=1)
        out["displacement"] = rows(S)
        out["displacement_bound"] = rows((one + gs) * ((LD(2) * np.abs(T) + dt) * dt).sum(axis=1) + gs * S)
    return out


def check_cox_diag(got, ref, kinds, what="", factor=1):
    """Print the figures, then assert every kind of `kinds` against its bound (times `factor`: the sum of two routes'
    bounds when two computed results are compared)."""
    for k in kinds:
        gk = np.asarray(got[k]).astype(LD)
        rk, bk = ref[k], ref[k + "_bound"] * LD(factor)
        assert gk.shape == rk.shape, (what, k, gk.shape, rk.shape)
        if gk.size == 0:
            continue
        err = np.abs(gk - rk)
        wi = np.unravel_index(int(np.argmax(err - bk)), err.shape)
        print("%s: %s err %.3e against bound %.3e at %s (value %.3e)" % (what, k, float(err[wi]), float(bk[wi]), wi,
                                                                       float(rk[wi])))
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), (what, k)
        assert (err <= bk).all(), (what, k, wi, float(err[wi]), float(bk[wi]))
    er = np.asarray(got["event_rows"]).astype(np.int64)
    assert np.array_equal(er, ref["event_rows"]), (what, "event_rows")
    assert np.array_equal(np.asarray(got["event_times"], dtype=np.float64), ref["event_times"]), (what, "event_times")


def direct_score_residuals(x, eta, wd, d, first, ties):
    """L by the O(n^2) definition, position order, longdouble."""
    n, m = x.shape
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    r = first if ties == "breslow" else np.arange(n)
    S0 = np.array([e[r[j]:].sum() for j in range(n)], dtype=LD)
    uu = np.array([(e[r[j]:, None] * x[r[j]:]).sum(axis=0) / S0[j] for j in range(n)], dtype=LD).reshape(n, m)
    L = np.zeros((n, m), dtype=LD)
    for k in range(n):
        L[k] = wd[k] * (x[k] - uu[k])
        for j in range(n):
            if r[j] <= k and wd[j] != 0:
                L[k] -= e[k] * (wd[j] / S0[j]) * (x[k] - uu[j])
    return L


def self_check(seed=0):
    """The decomposition of L against the direct definition, its column sums against coxinforef's score, sum g against
    its residual and displacement against L C L^T with a longdouble inverse; both ties values, weights (some zero),
    censoring and heavy ties, at n <= 300."""
    import inforef
    rng = np.random.default_rng(seed)
    for n, m, weighted in ((1, 2, False), (2, 3, True), (37, 4, False), (300, 5, True)):
        vals = rng.standard_normal((n, m + 2))
        cols = np.arange(1, m + 1)
        beta = rng.standard_normal(m) / np.sqrt(m)
        time = np.round(rng.exponential(1.0, n), 1)  # (many ties)
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0 if weighted else None
        for ties in ("order", "breslow"):
            x, eta, _, wd, d, order, first, last, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
            dec = coxinforef._decomposition(x, eta, wd, d, first, last, ties)
            Ld = direct_score_residuals(x, eta, wd, d, first, ties)
            tol = LD(n + 8) * LD(2.0) ** -58
            if n >= 37:
                Cl = inforef.ld_inverse_spd(dec["info"])
                # a lower-triangular R with C = R^T R: from the Cholesky factor of the reversed matrix
                P = np.eye(m)[::-1]
                Lc = np.linalg.cholesky(P @ Cl.astype(np.float64) @ P)
                Rf = (P @ Lc @ P).T
                assert np.allclose(np.triu(Rf, 1), 0)
                Cf = Rf.T @ Rf
                ref = cox_diag_reference(vals, cols, beta, time, status, w, ties, Rf, Cf, host_depths(m))
            else:
                ref = cox_diag_reference(vals, cols, beta, time, status, w, ties, None, None, host_depths(m))
            L = ref["score"][order]
            scale = (np.abs(x) * (wd + dec["v"])[:, None]).sum() + LD(1e-300)
            assert np.abs(L - Ld).max() <= tol * scale, (n, ties, float(np.abs(L - Ld).max()))
            assert np.abs(L.sum(axis=0) - dec["score"]).max() <= tol * scale, (n, ties)
            assert abs(ref["martingale"].sum() - dec["residual"]) <= tol * (wd.sum() + LD(1e-300)), (n, ties)
            if n >= 37:
                disp = np.einsum("kc,cj,kj->k", L, Cf.astype(LD), L)
                assert np.abs(ref["displacement"][order] - disp).max() <= tol * (np.abs(disp).max() + LD(1e-300)) * m, \
                    (n, ties)
                # and C is the inverse of the information up to fp64 rounding of the factor
                assert np.abs(Cf.astype(LD) - Cl).max() <= LD(1e-10) * np.abs(Cl).max(), (n, ties)
    return True
