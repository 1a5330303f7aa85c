"""Extended-precision reference and error bounds for bessx_cox_info_device / capi.cox_information_device /
bess_base.inference_survival (shared by tests/test_cox_info_api.py and tests/test_cox_info_gpu.py, in the manner of
tests/inforef.py and tests/coxsurvref.py).

Definitions.  Positions, pi and first(k) as in coxevalref; last(k) is the last position with the time of position k.
eta*_l = sum_c x(pi(l), cols[c]) beta[c] (no intercept), a* = clamp(eta*, -30, 30), e* = exp(a*), wd_k = w_k status_k,
r(k) = k ("order") or first(k) ("breslow"), x_l the m support entries of the row at position l,

    S0*(k) = sum_{l >= r(k)} e*_l,    S1*(k) = sum_{l >= r(k)} e*_l x_l,    u*_k = S1*(k) / S0*(k),
    H*_l   = sum_{k : r(k) <= l} wd_k / S0*(k)     (a prefix sum of h* = wd / S0*, taken at last(l) under "breslow"),
    v* = e* H*,    g* = wd - v*,
    score* = sum_l g*_l x_l,    info* = G1* - G2*,    G1* = sum_l v*_l x_l x_l^T,    G2* = sum_{k : status_k = 1} wd_k u*_k u*_k^T,
    residual* = sum_l g*_l,     loglik*: coxevalref.loglik_reference.

NumPy in np.longdouble on the host copy of the same (widened) values; eta* and the per-row Delta come from
evalref.eta_reference.  self_check() holds this decomposition, at n <= 300, to the direct O(n^2) definition
    info = sum_k wd_k sum_{l >= r(k)} (e_l / S0(k)) (x_l - u_k)(x_l - u_k)^T,    score = sum_k wd_k (x_k - u_k)
and to a central difference of the reference score in beta: the decomposition is the negative Hessian.

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).  The weights must be non-negative (the
sums of items 2 and 3 are then sums of non-negative terms); the reference asserts it.  Operations as built
(bessx_k_coxinfo.hip and the launchers it reuses; bess_base._cox_information_host does the same operations in fp64
NumPy with running sums and matrix products):

1. e.  |eta_hat - eta*| <= Delta_l, the clamp is 1-Lipschitz and exp is allowed 1 ulp (coxevalref items 1 and 2):
       e_hat = e* (1 + r),  |r| <= rho_l = expm1(Delta_l) (1 + 2 u) + 2 u;      rho = the largest rho_l.
2. S0 is a sum of at most n positive terms, additions only, every term entering once: n - 1 additions in some order
   whatever the blocks of the scan are (coxevalref item 3), so the scan's depth is n - 1:
       S0_hat = S0* (1 + s),  |s| <= sigma = rho + gamma_{n-1} (1 + rho).
3. h = wd / S0 (one division): |h_hat - h*| <= tau h*, tau = (sigma + u) / (1 - sigma) (coxsurvref).  H is a sum of at
   most n non-negative h, additions only (the forward scan of bessx_k_coxsurv.hip; NumPy: a running sum):
       H_hat = H* (1 + t),  |t| <= eta_H = tau + gamma_{n-1} (1 + tau).
4. v = e H (one multiplication):  v_hat = v* (1 + q),  |q| <= rv_l = (1 + rho_l) (1 + eta_H) (1 + u) - 1.
   g = wd - v (one subtraction):  |g_hat - g*| <= dg_l = rv_l v*_l + u (|g*_l| + rv_l v*_l).
5. The sweep over x (launch_info_gram; inforef item 3): an entry of G1 is sum_l a_l b_l with a = x_lj exact,
   b = x_lk v_hat_l (one rounding), the product inside the matrix instruction (at most one) and an addition chain of
   length depth1, any order (Higham, section 4.2):
       |G1_jk - G1*_jk|      <= b1_jk = sum_l v*_l |x_lj x_lk| (rv_l + (1 + rv_l) gamma_{depth1 + 2})
       |score_j - score*_j|  <= sum_l |x_lj| (dg_l + (|g*_l| + dg_l) gamma_{depth1 + 1})
       |residual - residual*| <= sum_l (dg_l + (|g*_l| + dg_l) gamma_{depth1 + 1})      (the sweep's intercept entry)
   depth1 = rows_per_slab + ceil(slabs / 16) + 4 of the sweep over n rows on the device, n on the host.
6. The risk-set means.  W_lc = e_l x_lc (one multiplication): relative rw = (1 + rho) (1 + u) - 1 of |e*_l x_lc|.
   S1 is a sum of at most n such terms of either sign, additions only, n - 1 additions in some order:
       |S1_hat(k, c) - S1*(k, c)| <= sig1 A_kc,   sig1 = rw + gamma_{n-1} (1 + rw),   A_kc = sum_{l >= r(k)} e*_l |x_lc|.
   u = S1 / S0 (one division, d): u_hat = (S1* + dS1) / S0* (1 + d) / (1 + s).  With a_kc = A_kc / S0*(k) >= |u*_kc|,
       |u_hat_kc - u*_kc| <= |u*| |(1 + d) / (1 + s) - 1| + (|dS1| / S0*) (1 + u) / (1 - sigma)
                          <= a_kc ru,   ru = (1 + sig1) (1 + u) / (1 - sigma) - 1,    and |u_hat_kc| <= a_kc (1 + ru).
7. The sweep over U: an entry of G2 is sum_k a_k b_k over the J event rows with a = u_hat_kj exact, b = u_hat_kk wd_k
   (one rounding), the product in the instruction, an addition chain of length depth2 (the split of a sweep over J
   rows; J on the host):
       |u_hat_kj u_hat_kk - u*_kj u*_kk| <= a_kj a_kk ((1 + ru)^2 - 1)
       |G2_jk - G2*_jk| <= b2_jk = sum_k wd_k a_kj a_kk ((1 + ru)^2 - 1 + (1 + ru)^2 gamma_{depth2 + 2}).
8. info = G1 - G2, one subtraction:  |info_jk - info*_jk| <= (b1_jk + b2_jk) (1 + u) + u |info*_jk|.
   This is where digits go: b1 and b2 are relative to mass_jk = sum_l v*_l |x_lj x_lk| + sum_k wd_k a_kj a_kk, which for
   columns far from centred is much larger than |info*_jk|.
9. Self-check: the bound of item 8 as a multiple of mass_jk must stay below REL_CEILING = 1e-9 for every input a test
   uses; cox_information_reference asserts it, so a bound cannot grow quietly until it hides a failure.
10. Standard errors (inforef item 5, no dispersion): with D* = diag(info*)^(-1/2) and S* = D* info* D*, the computed
   matrix is S* + E with |E_jk| <= r = max_jk bound_jk / sqrt(info*_jj info*_kk) -- relative to the diagonal of info*
   itself, so the cancellation factor mass / info* of item 8 is in it -- and
       |se - se*| / se* <= cond(S*) (M r + 8 M^2 u),   M = m,
   while cond(S*) < 1e6 and cond(S*) (M r + 8 M^2 u) < 0.1, which se_reference asserts."""
import numpy as np

import coxevalref
import evalref
import inforef

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = inforef.REL_CEILING
COND_CEILING = inforef.COND_CEILING


def _sweep_depth(rps, slabs):
    return int(rps) + (int(slabs) + 15) // 16 + 4 if slabs else 1


def device_depths(capi, n, m, n_event_rows):
    """(depth1, depth2) of items 5 and 7 for a device call: the splits are the library's own figures."""
    _, s1, s2 = capi.cox_info_workspace(n, m, n_event_rows)
    return _sweep_depth(*s1), _sweep_depth(*s2)


def host_depths(n, n_event_rows):
    """(depth1, depth2) of the NumPy route: matrix products over n and over J rows."""
    return int(n), max(int(n_event_rows), 1)


def _ordered(vals, cols, beta, time, status, w):
    """Everything in position order, longdouble: x (n, m), eta, delta (n,), wd, d, order, first, last."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, m = np.asarray(vals).shape[0], cols.size
    eta, delta = evalref.eta_reference(vals, cols, np.asarray(beta, dtype=np.float64).reshape(m, 1), [0.0])
    order, first = coxevalref.time_order(time)
    last = np.zeros(n, dtype=np.int64)
    for k in range(n - 1, -1, -1):
        last[k] = k if (k == n - 1 or first[k + 1] != first[k]) else last[k + 1]
    d = np.asarray(status).astype(LD).reshape(-1)[order]
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)[order]
    x = np.ascontiguousarray(np.asarray(vals)[:, cols].astype(LD)[order])
    return x, eta[order, 0], delta[order, 0], wl * d, d, order, first, last, (eta, delta)


def _decomposition(x, eta, wd, d, first, last, ties):
    """The decomposition in longdouble: dict of e, S0, H, v, g, u (n, m), G1, G2, info, score, residual."""
    n, m = x.shape
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    r = first if ties == "breslow" else np.arange(n)
    if ties not in ("order", "breslow"):
        raise ValueError(ties)
    S0 = np.cumsum(e[::-1])[::-1][r]
    H = np.cumsum(wd / S0)
    if ties == "breslow":
        H = H[last]
    v = e * H
    g = wd - v
    u = np.cumsum((e[:, None] * x)[::-1], axis=0)[::-1][r] / S0[:, None]
    ev = d != 0
    xt = np.ascontiguousarray(x.T)
    ut = np.ascontiguousarray(u[ev].T)
    G1 = np.einsum("ji,ki->jk", xt * v[None, :], xt)
    G2 = np.einsum("ji,ki->jk", ut * wd[ev][None, :], ut)
    info = G1 - G2
    info = np.tril(info) + np.tril(info, -1).T
    return {"e": e, "r": r, "S0": S0, "H": H, "v": v, "g": g, "u": u, "ev": ev, "G1": G1, "G2": G2, "info": info,
            "score": xt @ g, "residual": g.sum()}


def cox_information_reference(vals, cols, beta, time, status, w, ties, depths):
    """Reference and bounds of one call.  vals: the (widened) n x p values; cols, beta (m,); time, status (n,); w (n,)
    or None; ties "order" / "breslow"; depths = (depth1, depth2) of items 5 and 7.  Returns longdouble arrays: info,
    info_bound (m, m), score, score_bound (m,), residual, residual_bound, rel (the largest info_bound / mass), n_events,
    J, plus coxevalref's loglik reference under "loglik"."""
    x, eta, delta, wd, d, order, first, last, (eta_rows, delta_rows) = _ordered(vals, cols, beta, time, status, w)
    assert (wd >= 0).all(), "the bounds are derived for non-negative weights"
    n, m = x.shape
    depth1, depth2 = depths
    dec = _decomposition(x, eta, wd, d, first, last, ties)
    e, r, S0, v, g, ev = dec["e"], dec["r"], dec["S0"], dec["v"], dec["g"], dec["ev"]
    one = LD(1)
    rho_l = np.expm1(delta) * (one + LD(2) * U) + LD(2) * U                 # item 1
    rho = rho_l.max()
    sigma = rho + gamma(n - 1) * (one + rho)                                 # item 2
    tau = (sigma + U) / (one - sigma)                                        # item 3
    eta_h = tau + gamma(n - 1) * (one + tau)
    rv = (one + rho_l) * (one + eta_h) * (one + U) - one                     # item 4
    dg = rv * v + U * (np.abs(g) + rv * v)
    # (the bounds are sums of non-negative terms: fp64 BLAS forms them to a relative gamma_n, far inside the 2^-20 by
    # which they are enlarged here)
    up = one + LD(2.0) ** -20
    ax = np.abs(x)
    axt = np.ascontiguousarray(ax.T).astype(np.float64)
    mass1 = ((axt * v.astype(np.float64)[None, :]) @ axt.T).astype(LD)
    b1 = ((axt * (v * (rv + (one + rv) * gamma(depth1 + 2))).astype(np.float64)[None, :]) @ axt.T).astype(LD) * up  # item 5
    sterm = dg + (np.abs(g) + dg) * gamma(depth1 + 1)
    score_bound = ax.T @ sterm
    rw = (one + rho) * (one + U) - one                                       # item 6
    sig1 = rw + gamma(n - 1) * (one + rw)
    ru = (one + sig1) * (one + U) / (one - sigma) - one
    a = np.cumsum((e[:, None] * ax)[::-1], axis=0)[::-1][r] / S0[:, None]
    aet = np.ascontiguousarray(a[ev].T).astype(np.float64)
    mass2 = ((aet * wd[ev].astype(np.float64)[None, :]) @ aet.T).astype(LD)
    b2 = mass2 * ((one + ru) ** 2 - one + (one + ru) ** 2 * gamma(depth2 + 2)) * up   # item 7
    info_bound = (b1 + b2) * (one + U) + U * np.abs(dec["info"])             # item 8
    mass = mass1 + mass2
    pos = mass > 0
    rel = (info_bound[pos] / mass[pos]).max() if pos.any() else LD(0)        # item 9
    assert rel < REL_CEILING, ("the derived bound exceeds its ceiling: choose other inputs", float(rel))
    return {"info": dec["info"], "info_bound": info_bound, "score": dec["score"], "score_bound": score_bound,
            "residual": dec["residual"], "residual_bound": sterm.sum(), "rel": rel, "mass": mass, "m": m,
            "n_events": wd.sum(), "J": int(ev.sum()),
            "loglik": coxevalref.loglik_reference(eta_rows, delta_rows, time, status, w, ties)}


def check_cox_information(got, ref, what=""):
    """Print the figures, then assert info, score, residual_sum and loglik against their bounds."""
    gi, gs = np.asarray(got["info"]).astype(LD), np.asarray(got["score"]).astype(LD)
    m = ref["m"]
    assert gi.shape == (m, m) and gs.shape == (m,), (what, gi.shape, gs.shape)
    er, el = abs(LD(got["residual_sum"]) - ref["residual"]), abs(LD(got["loglik"]) - ref["loglik"]["loglik"][0])
    if m:
        ei, es = np.abs(gi - ref["info"]), np.abs(gs - ref["score"])
        wi = np.unravel_index(int(np.argmax(ei - ref["info_bound"])), ei.shape)
        ws = int(np.argmax(es - ref["score_bound"]))
        print("%s: info err %.3e against bound %.3e at %s (bound / mass %.3e); score err %.3e against bound %.3e at %d; "
              "residual_sum %.3e err %.3e against bound %.3e; loglik err %.3e against bound %.3e" % (
                  what, float(ei[wi]), float(ref["info_bound"][wi]), wi, float(ref["rel"]), float(es[ws]),
                  float(ref["score_bound"][ws]), ws, float(got["residual_sum"]), float(er), float(ref["residual_bound"]),
                  float(el), float(ref["loglik"]["bound"][0])))
        assert np.isfinite(np.asarray(got["info"])).all() and np.isfinite(np.asarray(got["score"])).all(), what
        assert (ei <= ref["info_bound"]).all(), (what, wi, float(ei[wi]), float(ref["info_bound"][wi]))
        assert (es <= ref["score_bound"]).all(), (what, ws, float(es[ws]), float(ref["score_bound"][ws]))
        assert er <= ref["residual_bound"], (what, float(er), float(ref["residual_bound"]))
    else:
        assert got["residual_sum"] == 0.0, what
    assert el <= ref["loglik"]["bound"][0], (what, float(el), float(ref["loglik"]["bound"][0]))
    assert float(got["n_events"]) == float(ref["n_events"]), what  # (weights in eighths: the sum is exact)


def se_reference(ref):
    """(se*, cov*, relative bound on se, cond(S*)) of a reference from cox_information_reference.  Asserts item 10's
    preconditions: cond(S*) < 1e6 and cond(S*) (M r + 8 M^2 u) < 0.1."""
    I, M = ref["info"], ref["m"]
    dg = np.diag(I)
    assert (dg > 0).all(), "the reference matrix has a non-positive diagonal entry"
    d = LD(1) / np.sqrt(dg)
    S = I * d[:, None] * d[None, :]
    ev = np.linalg.eigvalsh(S.astype(np.float64))
    cond = float(ev[-1] / ev[0])
    assert 0 < cond < COND_CEILING, ("cond(S*) is too large for the se bound: choose other inputs", cond)
    r = (ref["info_bound"] * d[:, None] * d[None, :]).max()
    rel = LD(cond) * (LD(M) * r + LD(8 * M * M) * U)
    assert rel < LD(0.1), float(rel)
    cov = inforef.ld_inverse_spd(S) * d[:, None] * d[None, :]
    return np.sqrt(np.diag(cov)), cov, rel, cond


def direct_definition(x, eta, wd, d, first, ties):
    """info and score by the O(n^2) definition, position order, longdouble."""
    n, m = x.shape
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    info, score = np.zeros((m, m), dtype=LD), np.zeros(m, dtype=LD)
    for k in range(n):
        if d[k] == 0:
            continue
        lo = first[k] if ties == "breslow" else k
        S0 = e[lo:].sum()
        uk = (e[lo:, None] * x[lo:]).sum(axis=0) / S0
        xc = x[lo:] - uk[None, :]
        info += wd[k] * ((e[lo:, None] * xc).T @ xc) / S0
        score += wd[k] * (x[k] - uk)
    return info, score


def self_check(seed=0):
    """The decomposition against the direct definition and against a central difference of the reference score in beta,
    for both ties values, with weights (some zero), censoring and heavy ties, at n <= 300."""
    rng = np.random.default_rng(seed)
    for n, m, weighted in ((1, 2, False), (2, 3, True), (37, 4, False), (300, 5, True)):
        vals = rng.standard_normal((n, m + 2))
        cols = np.arange(1, m + 1)
        beta = rng.standard_normal(m) / np.sqrt(m)
        time = np.round(rng.exponential(1.0, n), 1)  # (many ties)
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0 if weighted else None
        for ties in ("order", "breslow"):
            x, eta, _, wd, d, _, first, last, _ = _ordered(vals, cols, beta, time, status, w)
            dec = _decomposition(x, eta, wd, d, first, last, ties)
            info, score = direct_definition(x, eta, wd, d, first, ties)
            scale = np.abs(dec["G1"]).max() + LD(1e-300)
            assert np.abs(dec["info"] - info).max() <= LD(n + 8) * LD(2.0) ** -58 * scale, (n, ties)
            sscale = (np.abs(x) * wd[:, None]).sum() + LD(1e-300)
            assert np.abs(dec["score"] - score).max() <= LD(n + 8) * LD(2.0) ** -58 * sscale, (n, ties)
            assert abs(dec["residual"]) <= LD(n + 8) * LD(2.0) ** -58 * (wd.sum() + LD(1e-300)), (n, ties)
            h = LD(1e-6)
            for j in range(m):
                sc = []
                for sgn in (1, -1):
                    bj = np.asarray(beta, dtype=LD).copy()
                    bj[j] += sgn * h
                    sc.append(_decomposition(x, x @ bj, wd, d, first, last, ties)["score"])
                hess = (sc[0] - sc[1]) / (LD(2) * h)
                assert np.abs(hess + dec["info"][:, j]).max() <= LD(1e-9) * (scale + LD(1)), (n, ties, j)
    return True
