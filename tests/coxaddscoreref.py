"""Extended-precision reference and error bounds for bessx_cox_addscore_device / capi.cox_addscore_device /
bess_base.score_tests_survival (shared by tests/test_cox_addscore_api.py and tests/test_cox_addscore_gpu.py, in the manner
of tests/coxinforef.py and tests/addscoreref.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values, by the explicit risk-set definition and
NOT by the library's decomposition.  Positions, r(k), e*, wd, S0* as in coxinforef.  For every event k (status 1) the
e*-weighted mean and second moments over its risk set {l >= r(k)}, for the support columns x and the candidates z
together (suffix sums in longdouble; self_check() holds them to plain O(n^2) loops at n <= 300):

    E_k[f] = sum_{l >= r(k)} e*_l f_l / S0*(k),
    u*_j = sum_k wd_k (z_kj - E_k[z_j]),            c*_j = sum_k wd_k (E_k[z_j x] - E_k[z_j] E_k[x])     (m entries)
    d*_j = sum_k wd_k E_k[z_j^2],                   t*_j = sum_k wd_k E_k[z_j]^2,      var_j = sum_k wd_k Var_k(z_j) = d* - t*

-- row j of the score and of the observed information of the model extended by column j at coefficient 0 -- and with
the fp64 factor R the call was given (taken as exact), s*_j = |R c*_j|^2, a*_j = c*_j . r*, r* = R^T (R score*).

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).  Weights are non-negative.  rho_l, rho,
sigma, tau, eta_H, rv_l, dg_l, ru are items 1 to 6 of coxinforef, unchanged (row_terms() repeats their formulas).

A. u_j and d_j are addscoreref's step 3 with v, g of the Cox model and `chain` = the longest addition chain the library
   reports for an entry of u, c, d (n for the NumPy route):
       |u_j - u*_j| <= sum_l |z_lj| (dg_l + (|g*_l| + dg_l) gamma_{chain + 1})
       |d_j - d*_j| <= sum_l v*_l z_lj^2 (rv_l + (1 + rv_l) gamma_{chain + 3})
B. The panel entry P_lc = v_l x_lc - e_l A_lc.  dh_p is a sum of at most n quotients wd / S0 (relative tau each):
   relative tdh = tau + gamma_{n-1} (1 + tau).  With a_pc = E_p[|x_c|] >= |u*_pc| (coxinforef item 6: |u_hat - u*| <=
   a_pc ru), the increment dh_p u_pc (one rounding) is off by at most dh*_p a_pc rA1, rA1 = (1 + tdh)(1 + ru)(1 + u) - 1,
   and the forward scan adds at most n terms of either sign:
       |A_lc - A*_lc| <= bA_lc = AA_lc (rA1 + (1 + rA1) gamma_{n-1}),     AA_lc = sum_{p <= l} dh*_p a_pc >= |A*_lc|.
   The device forms fma(v, x, -(e A)): the product e A is rounded, then the fma; NumPy rounds v x as well, so v's
   relative error is taken as rv'_l = (1 + rv_l)(1 + u) - 1 for both routes.  With M1 = v*_l |x_lc|, M2 = e*_l AA_lc:
       err_in = M1 rv'_l + M2 ((1 + rho_l)(1 + u) - 1) + e*_l (1 + rho_l)(1 + u) bA_lc
       |P_lc - P*_lc| <= bP_lc = err_in + u (M1 + M2 + err_in).
   c_jc = sum_l z_lj P_lc on the matrix cores (or in BLAS), an addition chain of length `chain`, any order:
       |c_jc - c*_jc| <= bC_jc = sum_l |z_lj| (bP_lc + (M1 + M2 + bP_lc) gamma_{chain + 2});   mass_jc = sum_l |z_lj| (M1 + M2).
C. t_j = sum_l a_l (a_l Cc_l + 2 sum_{l' < l} Cc_l' a_l') with a = e z (one rounding: relative ra = (1 + rho)(1 + u) - 1) and
   Cc the forward sum of cc_p = dh_p / S0(p) >= 0 (relative tcc = (1 + tdh)(1 + u) / (1 - sigma) - 1; the scan adds at most
   n non-negative terms: rCc = tcc + gamma_{n-1} (1 + tcc)).  Expanded, every term is a product of two a and one Cc that
   passes through at most quad_chain + 8 further roundings (quad_chain is the library's figure: the recurrence within a
   slab of positions, the slab sums A, B and the carry, the ascending addition of the slabs; 2 n for the NumPy route):
       |t_j - t*_j| <= T_j ((1 + ra)^2 (1 + rCc) (1 + gamma_{quad_chain + 8}) - 1),
       T_j = sum_l |a*_l| (|a*_l| Cc*_l + 2 sum_{l' < l} Cc*_l' |a*_l'|)       (the mass of t_j).
D. s and a are addscoreref's step 4 with M = m: forward bounds through R from bC, the score behind r being the u-type
   bound of the support columns at the depth `score_chain`.
E. Self-check, asserted here so that a bound cannot grow quietly until it hides a failure: bu, bC, bd, bt stay below
   REL_CEILING = 1e-9 of their masses (sum |z| (|g*| ...), mass_jc, d*, T_j) on every input a test uses.
F. The statistic, by interval arithmetic in longdouble: adj in (u* - a*) +- (bu + ba), variance in ((d* - t*) - s*) +-
   (bd + bt + bs), gamma_8 for the fp64 operations of cox_score_test_table, dispersion exactly 1.  It is asserted only
   where variance* >= d* / 16; statistic_reference() asserts that EVERY candidate outside the support and outside an
   explicit `planted` list meets that condition, so no case is left out silently."""
import numpy as np

import addscoreref
import coxinforef
import evalref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = addscoreref.REL_CEILING
UP = addscoreref.UP


def device_depths(capi, n, m, n_event_rows, q, block=0):
    """{"chain", "score_chain", "sum_depth", "quad_chain"} of a device call: the splits are the library's own figures."""
    ws = capi.cox_addscore_workspace(n, m, n_event_rows, q, block)
    w0 = capi.cox_addscore_workspace(n, m, n_event_rows, max(m, 1), 0)
    return {"chain": ws["chain"], "score_chain": w0["chain"], "sum_depth": ws["sum_depth"], "quad_chain": ws["quad_chain"]}


def host_depths(n):
    """The NumPy route: matrix products and running sums over n rows."""
    return {"chain": int(n), "score_chain": int(n), "sum_depth": int(n), "quad_chain": 2 * int(n)}


def _sfx(a):
    return np.cumsum(a[::-1], axis=0)[::-1]


def row_terms(x, eta, delta, wd, d, first, last, ties):
    """coxinforef's decomposition and items 1 to 6 in position order (longdouble)."""
    n = eta.shape[0]
    dec = coxinforef._decomposition(x, eta, wd, d, first, last, ties)
    one = LD(1)
    rho_l = np.expm1(delta) * (one + LD(2) * U) + LD(2) * U
    rho = rho_l.max()
    sigma = rho + gamma(n - 1) * (one + rho)
    tau = (sigma + U) / (one - sigma)
    eta_h = tau + gamma(n - 1) * (one + tau)
    rv = (one + rho_l) * (one + eta_h) * (one + U) - one
    dg = rv * dec["v"] + U * (np.abs(dec["g"]) + rv * dec["v"])
    rw = (one + rho) * (one + U) - one
    sig1 = rw + gamma(n - 1) * (one + rw)
    ru = (one + sig1) * (one + U) / (one - sigma) - one
    dec.update(rho_l=rho_l, rho=rho, sigma=sigma, tau=tau, rv=rv, dg=dg, ru=ru)
    return dec


def cox_addscore_reference(vals, cols, beta, time, status, w, ties, R, candidates, depths):
    """Reference and bounds of one call.  vals: the (widened) n x p values; cols, beta (m,); time, status (n,); w (n,) or
    None; R: the fp64 factor (m, m) the call is given, or None (then no s, a; m = 0: s = a = 0); candidates: column
    numbers or None = all; depths: device_depths() or host_depths().  Returns longdouble arrays u, C, d, t, s, a, var
    with bounds bu, bC, bd, bt, bs, ba."""
    vals = np.asarray(vals)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, p = vals.shape
    x, eta, delta, wd, d, order, first, last, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
    assert (wd >= 0).all(), "the bounds are derived for non-negative weights"
    m = x.shape[1]
    J = np.arange(p) if candidates is None else np.asarray(candidates, dtype=np.int64)
    q = J.size
    rt = row_terms(x, eta, delta, wd, d, first, last, ties)
    e, r, S0, v, g, ev = rt["e"], rt["r"], rt["S0"], rt["v"], rt["g"], rt["ev"]
    Z = np.ascontiguousarray(vals[:, J].astype(LD)[order])
    one = LD(1)
    # the explicit risk-set definition, event by event
    evk = np.nonzero(ev)[0]
    rk, wk, S0k = r[evk], wd[evk], S0[evk]
    mz = _sfx(e[:, None] * Z)[rk] / S0k[:, None]
    m2 = _sfx(e[:, None] * Z * Z)[rk] / S0k[:, None]
    mx = rt["u"][evk]
    u = (wk[:, None] * (Z[evk] - mz)).sum(axis=0)
    dd = (wk[:, None] * m2).sum(axis=0)
    tt = (wk[:, None] * mz * mz).sum(axis=0)
    var_c = (wk[:, None] * (m2 - mz * mz)).sum(axis=0)
    C = np.zeros((q, m), dtype=LD)
    for j in range(q if m else 0):
        cj = _sfx((e * Z[:, j])[:, None] * x)[rk] / S0k[:, None] - mz[:, j, None] * mx
        C[j] = (wk[:, None] * cj).sum(axis=0)
    Us = (wk[:, None] * (x[evk] - mx)).sum(axis=0)
    # the bounds
    chain, qchain = int(depths["chain"]), int(depths["quad_chain"])
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    AZ = np.abs(Z).astype(np.float64)
    rv, dg, rho_l, rho, sigma, tau, ru = rt["rv"], rt["dg"], rt["rho_l"], rt["rho"], rt["sigma"], rt["tau"], rt["ru"]
    bu = (AZ.T @ f(dg + (np.abs(g) + dg) * gamma(chain + 1))).astype(LD) * LD(UP)                    # A
    mass_u = (AZ.T @ f(np.abs(g) + v)).astype(LD)
    bd = ((AZ * AZ).T @ f(v * (rv + (one + rv) * gamma(chain + 3)))).astype(LD) * LD(UP)
    S0pos = _sfx(e)
    dh = np.zeros(n, dtype=LD)
    np.add.at(dh, r, wd / S0)
    tdh = tau + gamma(n - 1) * (one + tau)
    ax = np.abs(x)
    apc = _sfx(e[:, None] * ax) / S0pos[:, None] if m else np.zeros((n, 0), dtype=LD)               # B
    AA = np.cumsum(dh[:, None] * apc, axis=0)
    rA1 = (one + tdh) * (one + ru) * (one + U) - one
    bA = AA * (rA1 + (one + rA1) * gamma(n - 1))
    rvp = (one + rv) * (one + U) - one
    M1, M2 = v[:, None] * ax, e[:, None] * AA
    err_in = M1 * rvp[:, None] + M2 * ((one + rho_l) * (one + U) - one)[:, None] + \
        (e * (one + rho_l) * (one + U))[:, None] * bA
    bP = err_in + U * (M1 + M2 + err_in)
    mass = (AZ.T @ f(M1 + M2)).astype(LD)
    bC = (AZ.T @ f(bP + (M1 + M2 + bP) * gamma(chain + 2))).astype(LD) * LD(UP)
    ra = (one + rho) * (one + U) - one                                                               # C
    tcc = (one + tdh) * (one + U) / (one - sigma) - one
    rCc = tcc + gamma(n - 1) * (one + tcc)
    Cc = np.cumsum(dh / S0pos)
    az = f(e)[:, None] * AZ
    ca = f(Cc)[:, None] * az
    T = ((az * (az * f(Cc)[:, None] + 2.0 * (np.cumsum(ca, axis=0) - ca))).sum(axis=0)).astype(LD) * LD(UP)
    bt = T * ((one + ra) ** 2 * (one + rCc) * (one + gamma(qchain + 8)) - one)
    # E
    for name, b, ms in (("u", bu, mass_u), ("C", bC, mass), ("d", bd, dd), ("t", bt, T)):
        pos = ms > 0
        assert (b[~pos] == 0).all(), ("a bound without a mass", name)
        rel = (b[pos] / ms[pos]).max() if pos.any() else LD(0)
        assert rel < REL_CEILING, ("the derived bound on %s exceeds its ceiling: choose other inputs" % name, float(rel))
    out = {"u": u, "bu": bu, "C": C, "bC": bC, "d": dd, "bd": bd, "t": tt, "bt": bt, "var_centred": var_c, "score": Us,
           "m": m, "columns": J, "cols": cols, "n_events": wd.sum(), "J": int(ev.sum()), "T": T}
    if m == 0:
        z = np.zeros(q, dtype=LD)
        out.update(s=z, bs=z.copy(), a=z.copy(), ba=z.copy())
    elif R is not None:                                                                              # D
        sdepth, cs = int(depths["sum_depth"]), int(depths["score_chain"])
        bU = (ax.astype(np.float64).T @ f(dg + (np.abs(g) + dg) * gamma(cs + 1))).astype(LD) * LD(UP)
        Rl = np.tril(np.asarray(R, dtype=np.float64)).astype(LD)
        aR = np.abs(np.tril(np.asarray(R, dtype=np.float64)))
        tR = np.einsum("jk,ak->ja", C, np.ascontiguousarray(Rl))
        btR = ((f(bC) @ aR.T) + float(gamma(m + 3)) * (f(np.abs(C) + bC) @ aR.T)).astype(LD) * LD(UP)
        s = (tR * tR).sum(axis=1)
        bs = (btR * (LD(2) * np.abs(tR) + btR)).sum(axis=1) + gamma(sdepth + 2) * ((np.abs(tR) + btR) ** 2).sum(axis=1)
        rr = Rl.T @ (Rl @ Us)
        AtA = aR.T @ aR
        br = ((AtA @ f(bU)) + float(gamma(2 * m + 2)) * (AtA @ f(np.abs(Us) + bU))).astype(LD) * LD(UP)
        a = C @ rr
        ba = (bC @ np.abs(rr) + np.abs(C) @ br + bC @ br + gamma(m + 3) * ((np.abs(C) + bC) @ (np.abs(rr) + br)))
        dp = dd > 0
        assert (bs[~dp] == 0).all() and (not dp.any() or (bs[dp] / dd[dp]).max() < REL_CEILING), "bound on s"
        out.update(s=s, bs=bs, a=a, ba=ba, r=rr)
    return out


def check_vectors(got, ref, what="", cross=True):
    """Print the figures, then assert u, d, t (and cross, s, a where both sides have them) against their bounds."""
    names = [("u", "bu"), ("d", "bd"), ("t", "bt")] + ([("s", "bs"), ("a", "ba")] if "s" in ref else [])
    if cross and "cross" in got:
        names.append(("cross", "bC"))
    line = []
    for k, b in names:
        gv = np.asarray(got[k]).astype(LD)
        rv = ref["C"] if k == "cross" else ref[k]
        assert gv.shape == rv.shape, (what, k, gv.shape, rv.shape)
        if gv.size == 0:
            continue
        err = np.abs(gv - rv)
        wi = np.unravel_index(int(np.argmax(err - ref[b])), err.shape)
        line.append("%s err %.2e bound %.2e" % (k, float(err[wi]), float(ref[b][wi])))
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), (what, k)
        assert (err <= ref[b]).all(), (what, k, wi, float(err[wi]), float(ref[b][wi]))
    print("%s: %s" % (what, "; ".join(line)))


def statistic_reference(ref, planted=()):
    """Step F, with the keys of addscoreref.statistic_reference (so that addscoreref.check_table serves): adj, var, stat,
    lo, hi, ok, in_model, dispersion, ratio, badj, bvar, planted.  Asserts that every candidate outside the support and
    outside `planted` has variance* >= d* / 16, and that d* - t* is the centred second moment."""
    adj, var = ref["u"] - ref["a"], (ref["d"] - ref["t"]) - ref["s"]
    badj, bvar = ref["bu"] + ref["ba"], ref["bd"] + ref["bt"] + ref["bs"]
    assert (np.abs((ref["d"] - ref["t"]) - ref["var_centred"]) <= LD(2.0) ** -50 * (ref["d"] + LD(1e-300))).all()
    in_model = np.isin(ref["columns"], ref["cols"])
    is_planted = np.isin(ref["columns"], np.asarray(planted, dtype=np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ref["d"] > 0, var / ref["d"], LD(0))
    ok = ~in_model & ~is_planted
    assert (ratio[ok] >= LD(1) / 16).all(), ("a candidate is nearly collinear with the support: plant it explicitly",
                                            float(ratio[ok].min()))
    assert (var[ok] - bvar[ok] > 0).all()
    lo_adj = np.maximum(np.abs(adj) - badj, LD(0))
    hi_adj = np.abs(adj) + badj
    g8 = gamma(8)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(ok, lo_adj * lo_adj / (var + bvar) * (LD(1) - g8), LD(0))
        hi = np.where(ok, hi_adj * hi_adj / (var - bvar) * (LD(1) + g8), LD(0))
        stat = np.where(ok, adj * adj / var, LD(0))
    return {"adj": adj, "var": var, "stat": stat, "lo": lo, "hi": hi, "ok": ok, "in_model": in_model,
            "dispersion": LD(1), "ratio": ratio, "badj": badj, "bvar": bvar, "planted": is_planted}


check_table = addscoreref.check_table


def self_check(seed=0):
    """The event-by-event reference against coxinforef's O(n^2) direct definition of the model extended by one candidate
    at coefficient 0 (its last score entry, last row and last diagonal entry), for both ties values, with weights (some
    zero), censoring and heavy ties, at n <= 300."""
    rng = np.random.default_rng(seed)
    for n, m, weighted in ((1, 0, False), (2, 1, True), (37, 3, False), (300, 4, True)):
        p = m + 3
        vals = rng.standard_normal((n, p))
        cols = np.arange(1, m + 1)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        time = np.round(rng.exponential(1.0, n), 1)
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0 if weighted else None
        for ties in ("order", "breslow"):
            ref = cox_addscore_reference(vals, cols, beta, time, status, w, ties, None, None, host_depths(n))
            x, eta, _, wd, d, order, first, _, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
            for j in range(p):
                xe = np.concatenate([x, vals[:, j].astype(LD)[order][:, None]], axis=1)
                info, score = coxinforef.direct_definition(xe, eta, wd, d, first, ties)
                tol = LD(n + 8) * LD(2.0) ** -58
                assert abs(score[m] - ref["u"][j]) <= tol * ((np.abs(xe[:, m]) * wd).sum() * 2 + LD(1e-300)), (n, ties, j)
                assert abs(info[m, m] - (ref["d"][j] - ref["t"][j])) <= tol * (ref["d"][j] + ref["T"][j] + LD(1e-300))
                if m:
                    sc = np.abs(ref["C"][j]).max() + ref["d"][j] + LD(1e-300)
                    assert np.abs(info[m, :m] - ref["C"][j]).max() <= tol * 64 * sc, (n, ties, j)
    return True
