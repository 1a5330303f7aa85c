"""Extended-precision reference and error bounds for bessx_cox_zph_device / capi.cox_zph_device / capi.cox_zph_table /
bess_base.proportional_hazards_test (shared by tests/test_cox_zph_api.py and tests/test_cox_zph_gpu.py), built on
tests/coxinforef.py, whose notation and items 1 to 10 it continues.

Definitions (position order; r(k), first, last, e*, wd, S0*, u*_k: coxinforef).  g_k = the caller's centred time transform
at position k, read where status is 1 (0 elsewhere).  For q = 0, 1, 2, with c^q_k = wd_k g_k^q,

    h^q*_k = c^q_k / S0*(k),   H^q*_l = sum_{k : r(k) <= l} h^q*_k   (a prefix sum, taken at last(l) under "breslow"),
    v^q* = e* H^q*,            a^q* = c^q - v^q*,
    G1^q* = sum_l v^q*_l x_l x_l^T,   G2^q* = sum_{k : status_k = 1} c^q_k u*_k u*_k^T,   I_q* = G1^q* - G2^q*,
    s^q*  = sum_l a^q*_l x_l,
    D* = I_2* - I_1* inverse(I_0*) I_1*,   global* = s^1*^T inverse(D*) s^1*,   chisq*_j = (s^1*_j)^2 / D*_jj.

NumPy in np.longdouble on the host copy of the same (widened) values.  self_check() holds the decomposition, at n <= 300,
to the direct O(n^2) definitions I_q = sum_k c^q_k sum_{l >= r(k)} (e_l / S0(k)) (x_l - u_k)(x_l - u_k)^T and s^q = sum_k
c^q_k (x_k - u_k), and checks that g + const leaves D unchanged and moves s^1 by const * s^0.

The bounds are derived, not measured; u = 2^-53.  g changes sign, so for q = 1 nothing is a sum of non-negative terms:
every bound is relative to the sum of the ABSOLUTE values, written with a bar: cb^q_k = wd_k |g_k|^q, hb^q = cb^q / S0*,
Hb^q its prefix sum (at last(l) under "breslow"), vb^q = e* Hb^q.  rho_l, rho, sigma, rw, sig1, ru and a_kc are
coxinforef's items 1, 2 and 6, unchanged.  Operations as built (bessx_k_coxzph.hip and the launchers it reuses;
bess_base._cox_zph_host does the same operations in fp64 NumPy with running sums and matrix products):

Z3. c^0 = wd is exact, c^1 = wd g one product, c^2 = c^1 g a second: c_hat = c (1 + k), |k| <= kc_q = (1 + u)^q - 1.
    h = c / S0 (one division): |h_hat - h*| <= tau_q hb,  tau_q = (1 + kc_q) (1 + u) / (1 - sigma) - 1 (q = 0: item 3's
    tau).  H is a sum of at most n terms of either sign, additions only, n - 1 additions in some order:
        |H_hat - H*| <= eta_q Hb,   eta_q = tau_q + gamma_{n-1} (1 + tau_q).
Z4. v = e H (one multiplication): |v_hat - v*| <= dv_l = rv_l vb_l,  rv_l = (1 + rho_l) (1 + eta_q) (1 + u) - 1 (|H*| <=
    Hb).  a = c - v (one subtraction): |a_hat - a*| <= da_l = kc_q cb_l + dv_l + u (|a*_l| + kc_q cb_l + dv_l).  (The
    device forms a as one fused multiply-add, c - e H with the product unrounded: fewer roundings, the same bound.)
Z5. The sweep over x, item 5 with |v*| <= vb:
        |G1_jk - G1*_jk| <= b1_jk = sum_l vb_l |x_lj x_lk| (rv_l + (1 + rv_l) gamma_{depth1 + 2})
        |s_j - s*_j|      <= sum_l |x_lj| (da_l + (|a*_l| + da_l) gamma_{depth1 + 1}).
Z7. The sweep over U, item 7 with the weight c_hat in place of wd:
        |G2_jk - G2*_jk| <= b2_jk = sum_k cb_k a_kj a_kk ((1 + ru)^2 (1 + kc_q) (1 + gamma_{depth2 + 2}) - 1).
Z8. I_q = G1 - G2, one subtraction: |I_jk - I*_jk| <= (b1 + b2) (1 + u) + u |I*_jk|, relative to mass_jk = sum_l vb_l
    |x_lj x_lk| + sum_k cb_k a_kj a_kk.
Z9. Self-check: the bound of Z8 as a multiple of mass_jk stays below REL_CEILING = 1e-9 for q = 0, 1, 2 and every input
    a test uses; cox_zph_reference asserts it.
Z10. The statistics, in the manner of item 10.  Scale by d = diag(I_0*)^(-1/2): A_q = d I_q* d, y = d s^1*, M = m.  The
    computed A_q differ from these by dA_q with ||dA_q||_2 <= eps_q = M r_q + 8 M^2 u, r_q = max_jk bound^q_jk d_j d_k (the
    second term: the host's fp64 linear algebra).  With k0 = cond(A_0) >= ||inverse(A_0)|| (A_0 has a unit diagonal),
    a_1 = ||A_1||_2, a_2 = ||A_2||_2:
        ||inverse(A_0 + dA_0) - inverse(A_0)|| <= di = k0^2 eps_0 / (1 - k0 eps_0)
        ||dDt|| <= eD = eps_2 + a_1^2 di + (2 a_1 eps_1 + eps_1^2) (k0 + di) + 8 M^2 u (a_2 + a_1^2 k0),  Dt = d D* d.
    chisq_j = s_j^2 / D_jj with |ds_j| from Z5 and |dD_jj| / D*_jj <= rD_j = eD / Dt_jj:
        |chisq_hat_j - chisq*_j| <= ((|s*_j| + ds_j)^2 / (1 - rD_j) - s*_j^2) / D*_jj + 4 u chisq*_j.
    With t = diag(Dt)^(-1/2), SD = t Dt t (unit diagonal), kD = cond(SD), rD = max_j rD_j >= ||t dDt t||, z = t y,
    dz_j = t_j d_j ds_j:  dI = kD^2 rD / (1 - kD rD),
        |global_hat - global*| <= (2 ||z|| ||dz|| + ||dz||^2) (kD + dI) + ||z||^2 (dI + 8 M^2 u kD).
    The bound is conditional on k0 < 1e6, kD < 1e6, k0 eps_0 < 0.1 and kD rD < 0.1, which table_reference ASSERTS."""
import numpy as np

import coxevalref
import coxinforef
import evalref
import inforef

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = coxinforef.REL_CEILING
COND_CEILING = coxinforef.COND_CEILING


def device_depths(capi, n, m, n_event_rows):
    """(depth1, depth2) of Z5 and Z7 for a device call: the splits are the library's own figures."""
    _, s1, s2 = capi.cox_zph_workspace(n, m, n_event_rows)
    return coxinforef._sweep_depth(*s1), coxinforef._sweep_depth(*s2)


host_depths = coxinforef.host_depths


def _g_ordered(gt, d, order):
    return np.where(d != 0, np.asarray(gt, dtype=np.float64).astype(LD).reshape(-1)[order], LD(0))


def _sym_gram(at, wv):
    """at diag(wv) at^T in longdouble, the lower triangle computed (in row blocks) and mirrored"""
    m = at.shape[0]
    G = np.zeros((m, m), dtype=LD)
    step = max(16, (m + 7) // 8)
    for lo in range(0, m, step):
        hi = min(lo + step, m)
        G[lo:hi, :hi] = np.einsum("ji,ki->jk", at[lo:hi] * wv[None, :], at[:hi])
    return np.tril(G) + np.tril(G, -1).T


def _decomposition(x, eta, wd, d, g, first, last, ties):
    """The decomposition in longdouble: e, r, S0, ev, u, and per q the lists c, H, Hb, v, vb, a, G1, G2, info, score."""
    n, m = x.shape
    if ties not in ("order", "breslow"):
        raise ValueError(ties)
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    r = first if ties == "breslow" else np.arange(n)
    S0 = np.cumsum(e[::-1])[::-1][r]
    u = np.cumsum((e[:, None] * x)[::-1], axis=0)[::-1][r] / S0[:, None]
    ev = d != 0
    xt = np.ascontiguousarray(x.T)
    ut = np.ascontiguousarray(u[ev].T)
    out = {"e": e, "r": r, "S0": S0, "u": u, "ev": ev}
    for name in ("c", "H", "Hb", "v", "vb", "a", "G1", "G2", "info", "score"):
        out[name] = []
    for q in range(3):
        c = wd * g ** q
        H, Hb = np.cumsum(c / S0), np.cumsum(np.abs(c) / S0)
        if ties == "breslow":
            H, Hb = H[last], Hb[last]
        v = e * H
        G1, G2 = _sym_gram(xt, v), _sym_gram(ut, c[ev])
        info = G1 - G2
        for name, val in (("c", c), ("H", H), ("Hb", Hb), ("v", v), ("vb", e * Hb), ("a", c - v), ("G1", G1), ("G2", G2),
                          ("info", info), ("score", xt @ (c - v))):
            out[name].append(val)
    return out


def cox_zph_reference(vals, cols, beta, time, status, w, gt, ties, depths):
    """Reference and bounds of one call.  vals: the (widened) n x p values; cols, beta (m,); time, status, gt (n,); w
    (n,) or None; depths = (depth1, depth2) of Z5 and Z7.  Returns longdouble arrays: "info" and "info_bound" (lists of
    three (m, m)), "score" and "score_bound" (lists of three (m,); the third is not an output), rel (the largest
    info_bound / mass over the three), n_events, J, m, plus coxevalref's loglik reference under "loglik"."""
    x, eta, delta, wd, d, order, first, last, (eta_rows, delta_rows) = coxinforef._ordered(vals, cols, beta, time, status, w)
    assert (wd >= 0).all(), "the bounds are derived for non-negative weights"
    g = _g_ordered(gt, d, order)
    n, m = x.shape
    depth1, depth2 = depths
    dec = _decomposition(x, eta, wd, d, g, first, last, ties)
    e, r, S0, ev = dec["e"], dec["r"], dec["S0"], dec["ev"]
    one = LD(1)
    rho_l = np.expm1(delta) * (one + LD(2) * U) + LD(2) * U                 # item 1
    rho = rho_l.max()
    sigma = rho + gamma(n - 1) * (one + rho)                                 # item 2
    rw = (one + rho) * (one + U) - one                                       # item 6
    sig1 = rw + gamma(n - 1) * (one + rw)
    ru = (one + sig1) * (one + U) / (one - sigma) - one
    up = one + LD(2.0) ** -20  # (the bounds are sums of non-negative terms formed in fp64: enlarged as in coxinforef)
    ax = np.abs(x)
    axt = np.ascontiguousarray(ax.T).astype(np.float64)
    ab = np.cumsum((e[:, None] * ax)[::-1], axis=0)[::-1][r] / S0[:, None]
    aet = np.ascontiguousarray(ab[ev].T).astype(np.float64)
    ref = {"info": dec["info"], "score": dec["score"], "info_bound": [], "score_bound": [], "mass": [], "m": m,
           "n_events": wd.sum(), "J": int(ev.sum()), "rel": LD(0),
           "loglik": coxevalref.loglik_reference(eta_rows, delta_rows, time, status, w, ties)}
    for q in range(3):
        cb, vb, a = np.abs(dec["c"][q]), dec["vb"][q], dec["a"][q]
        kc = (one + U) ** q - one                                            # Z3
        tau = (one + kc) * (one + U) / (one - sigma) - one
        eta_q = tau + gamma(n - 1) * (one + tau)
        rv = (one + rho_l) * (one + eta_q) * (one + U) - one                 # Z4
        dv = rv * vb
        da = kc * cb + dv + U * (np.abs(a) + kc * cb + dv)
        mass1 = ((axt * vb.astype(np.float64)[None, :]) @ axt.T).astype(LD)
        b1 = ((axt * (vb * (rv + (one + rv) * gamma(depth1 + 2))).astype(np.float64)[None, :]) @ axt.T).astype(LD) * up
        sterm = da + (np.abs(a) + da) * gamma(depth1 + 1)                    # Z5
        mass2 = ((aet * cb[ev].astype(np.float64)[None, :]) @ aet.T).astype(LD)
        b2 = mass2 * ((one + ru) ** 2 * (one + kc) * (one + gamma(depth2 + 2)) - one) * up   # Z7
        bound = (b1 + b2) * (one + U) + U * np.abs(dec["info"][q])           # Z8
        mass = mass1 + mass2
        pos = mass > 0
        rel = (bound[pos] / mass[pos]).max() if pos.any() else LD(0)         # Z9
        assert rel < REL_CEILING, ("the derived bound exceeds its ceiling: choose other inputs", q, float(rel))
        ref["rel"] = max(ref["rel"], rel)
        ref["info_bound"].append(bound)
        ref["score_bound"].append(ax.T @ sterm)
        ref["mass"].append(mass)
    return ref


def check_cox_zph(got, ref, what=""):
    """Print the figures, then assert the three matrices, the two vectors, loglik and n_events against their bounds."""
    m = ref["m"]
    el = abs(LD(got["loglik"]) - ref["loglik"]["loglik"][0])
    line = []
    for q in range(3):
        gi = np.asarray(got["info%d" % q]).astype(LD)
        assert gi.shape == (m, m), (what, q, gi.shape)
        if m:
            ei = np.abs(gi - ref["info"][q])
            wi = np.unravel_index(int(np.argmax(ei - ref["info_bound"][q])), ei.shape)
            line.append("info%d err %.3e against bound %.3e at %s" % (q, float(ei[wi]), float(ref["info_bound"][q][wi]), wi))
    for q in range(2):
        gs = np.asarray(got["score%d" % q]).astype(LD)
        assert gs.shape == (m,), (what, q, gs.shape)
        if m:
            es = np.abs(gs - ref["score"][q])
            ws = int(np.argmax(es - ref["score_bound"][q]))
            line.append("score%d err %.3e against bound %.3e at %d" % (q, float(es[ws]), float(ref["score_bound"][q][ws]), ws))
    print("%s: %s; bound / mass %.3e; loglik err %.3e against bound %.3e" % (
        what, "; ".join(line), float(ref["rel"]), float(el), float(ref["loglik"]["bound"][0])))
    for q in range(3):
        gi = np.asarray(got["info%d" % q])
        assert np.isfinite(gi).all() and np.array_equal(gi, gi.T), (what, q)
        ei = np.abs(gi.astype(LD) - ref["info"][q])
        assert (ei <= ref["info_bound"][q]).all(), (what, q, float((ei - ref["info_bound"][q]).max()))
    for q in range(2):
        gs = np.asarray(got["score%d" % q])
        assert np.isfinite(gs).all(), (what, q)
        es = np.abs(gs.astype(LD) - ref["score"][q])
        assert (es <= ref["score_bound"][q]).all(), (what, q, float((es - ref["score_bound"][q]).max()))
    assert el <= ref["loglik"]["bound"][0], (what, float(el), float(ref["loglik"]["bound"][0]))
    assert float(got["n_events"]) == float(ref["n_events"]), what  # (weights in eighths: the sum is exact)


def _norm2(A):
    return LD(np.linalg.norm(np.asarray(A, dtype=np.float64), 2)) * (LD(1) + LD(2.0) ** -20)


def table_reference(ref):
    """The statistics of a reference from cox_zph_reference and their bounds (Z10): dict of chisq, chisq_bound (m,),
    global_chisq, global_bound, slope_var, cond_info, cond, D.  Asserts Z10's preconditions."""
    I0, I1, I2, s, M = ref["info"][0], ref["info"][1], ref["info"][2], ref["score"][1], ref["m"]
    one = LD(1)
    dg = np.diag(I0)
    assert M >= 1 and (dg > 0).all(), "the reference information has a non-positive diagonal entry"
    d = one / np.sqrt(dg)
    sc = d[:, None] * d[None, :]
    A0, A1, A2 = I0 * sc, I1 * sc, I2 * sc
    ev0 = np.linalg.eigvalsh(A0.astype(np.float64))
    k0 = float(ev0[-1] / ev0[0])
    assert 0 < k0 < COND_CEILING, ("cond of the scaled I_0 is too large: choose other inputs", k0)
    X0 = inforef.ld_inverse_spd(A0)
    Dt = A2 - A1 @ X0 @ A1
    Dt = (Dt + Dt.T) / LD(2)
    dd = np.diag(Dt)
    assert (dd > 0).all(), "the reference D has a non-positive diagonal entry"
    t = one / np.sqrt(dd)
    SD = Dt * t[:, None] * t[None, :]
    evD = np.linalg.eigvalsh(SD.astype(np.float64))
    kD = float(evD[-1] / evD[0])
    assert 0 < kD < COND_CEILING, ("cond of the scaled D is too large: choose other inputs", kD)
    host = LD(8 * M * M) * U
    eps = [LD(M) * (ref["info_bound"][q] * sc).max() + host for q in range(3)]
    k0l, kDl = LD(k0) * (one + LD(2.0) ** -20), LD(kD) * (one + LD(2.0) ** -20)
    assert k0l * eps[0] < LD(0.1), float(k0l * eps[0])
    a1, a2 = _norm2(A1), _norm2(A2)
    di = k0l ** 2 * eps[0] / (one - k0l * eps[0])
    eD = eps[2] + a1 ** 2 * di + (LD(2) * a1 * eps[1] + eps[1] ** 2) * (k0l + di) + host * (a2 + a1 ** 2 * k0l)
    rDj = eD / dd
    rD = rDj.max()
    assert kDl * rD < LD(0.1), float(kDl * rD)
    Dfull = Dt / sc
    Djj = np.diag(Dfull)
    ds = ref["score_bound"][1]
    chisq = s * s / Djj
    chisq_bound = ((np.abs(s) + ds) ** 2 / (one - rDj) - s * s) / Djj + LD(4) * U * chisq
    z, dz = t * d * s, t * d * ds
    XD = inforef.ld_inverse_spd(SD)
    gl = z @ XD @ z
    nz, ndz = np.sqrt((z * z).sum()), np.sqrt((dz * dz).sum())
    dI = kDl ** 2 * rD / (one - kDl * rD)
    gb = (LD(2) * nz * ndz + ndz ** 2) * (kDl + dI) + nz ** 2 * (dI + host * kDl)
    slope_var = np.diag(XD) * (t * d) ** 2
    return {"chisq": chisq, "chisq_bound": chisq_bound, "global_chisq": gl, "global_bound": gb, "slope_var": slope_var,
            "cond_info": k0, "cond": kD, "D": Dfull, "diag_ratio": float((Djj / np.diag(I2)).min())}


def check_table(tab, tref, what=""):
    """Print the figures, then assert capi.cox_zph_table's statistics against table_reference's bounds."""
    ec = np.abs(np.asarray(tab["chisq"]).astype(LD) - tref["chisq"])
    eg = abs(LD(tab["global_chisq"]) - tref["global_chisq"])
    j = int(np.argmax(ec - tref["chisq_bound"]))
    print("%s: cond(I_0) %.3e cond(D) %.3e; chisq err %.3e against bound %.3e at %d; global %.6e err %.3e against bound "
          "%.3e" % (what, tref["cond_info"], tref["cond"], float(ec[j]), float(tref["chisq_bound"][j]), j,
                    float(tref["global_chisq"]), float(eg), float(tref["global_bound"])))
    assert tab["positive_definite"], what
    assert (ec <= tref["chisq_bound"]).all(), (what, j, float(ec[j]), float(tref["chisq_bound"][j]))
    assert eg <= tref["global_bound"], (what, float(eg), float(tref["global_bound"]))


def direct_definition(x, eta, wd, d, g, first, ties):
    """I_q and s^q, q = 0, 1, 2, by the O(n^2) definitions, position order, longdouble."""
    n, m = x.shape
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    info, score = np.zeros((3, m, m), dtype=LD), np.zeros((3, m), dtype=LD)
    for k in range(n):
        if d[k] == 0:
            continue
        lo = first[k] if ties == "breslow" else k
        S0 = e[lo:].sum()
        uk = (e[lo:, None] * x[lo:]).sum(axis=0) / S0
        xc = x[lo:] - uk[None, :]
        var = ((e[lo:, None] * xc).T @ xc) / S0
        for q in range(3):
            info[q] += wd[k] * g[k] ** q * var
            score[q] += wd[k] * g[k] ** q * (x[k] - uk)
    return info, score


def _schur(dec):
    I0, I1, I2 = dec["info"]
    return I2 - I1 @ np.linalg.solve(I0.astype(np.float64), I1.astype(np.float64)).astype(LD)


def self_check(seed=0):
    """The decomposition against the direct definitions, for both ties values, with weights (some zero), censoring and
    heavy ties, at n <= 300; and the shift of g by a constant: D stays, s^1 moves by const * s^0."""
    rng = np.random.default_rng(seed)
    for n, m, weighted in ((1, 2, False), (2, 3, True), (37, 4, False), (300, 5, True)):
        vals = rng.standard_normal((n, m + 2))
        cols = np.arange(1, m + 1)
        beta = rng.standard_normal(m) / np.sqrt(m)
        time = np.round(rng.exponential(1.0, n), 1)  # (many ties)
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0 if weighted else None
        gt = rng.standard_normal(n)
        for ties in ("order", "breslow"):
            x, eta, _, wd, d, order, first, last, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
            g = _g_ordered(gt, d, order)
            dec = _decomposition(x, eta, wd, d, g, first, last, ties)
            info, score = direct_definition(x, eta, wd, d, g, first, ties)
            tol = LD(n + 8) * LD(2.0) ** -58
            for q in range(3):
                scale = np.abs(np.einsum("ji,ki->jk", x.T * dec["vb"][q][None, :], x.T)).max() + LD(1e-300)
                assert np.abs(dec["info"][q] - info[q]).max() <= tol * scale, (n, ties, q)
                sscale = (np.abs(x) * np.abs(dec["c"][q])[:, None]).sum() + LD(1e-300)
                assert np.abs(dec["score"][q] - score[q]).max() <= tol * sscale, (n, ties, q)
            if n >= 37:
                cst = LD(0.75)
                dec2 = _decomposition(x, eta, wd, d, np.where(d != 0, g + cst, LD(0)), first, last, ties)
                D1, D2 = _schur(dec), _schur(dec2)
                assert np.abs(D1 - D2).max() <= LD(1e-10) * np.abs(dec2["info"][2]).max(), (n, ties)
                sscale = (np.abs(x) * wd[:, None]).sum() * (LD(1) + np.abs(g).max())
                assert np.abs(dec2["score"][1] - dec["score"][1] - cst * dec["score"][0]).max() <= tol * sscale, (n, ties)
    return True
