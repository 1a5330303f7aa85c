"""Extended-precision reference and error bounds for bessx_groupscore_device / bess_base.score_tests_groups (shared by
tests/test_groupscore_api.py and tests/test_groupscore_gpu.py, in the manner of tests/addscoreref.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values.  v*, g*, rf_i (relative error of v_i),
dg_i (absolute error of g_i) and Z are addscoreref.row_terms(), unchanged.  For every tested group with columns J,
d = |J|:

    u* = X_J^T g*,   C* = X_J^T diag(v*) Z,   a* = C* r*,   D* = X_J^T diag(v*) X_J,   S* = (C* R^T)(C* R^T)^T.

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).

1. u and C: step 3 of addscoreref.py with the depth the library reports for its own split (depth; n for NumPy).
2. D.  The right-hand operand v_hat_i x_ij' is rounded once, the product is formed inside the matrix instruction (at most
   one rounding) and a wave adds the rows of its slab, then the slabs are added in ascending order: gram_depth =
   gram_rows_per_slab + gram_slabs additions (n for the NumPy route, a matrix product over n rows):
       |D_jj' - D*_jj'| <= sum_i v*_i |x_ij x_ij'| (rf_i + (1 + rf_i) gamma_{gram_depth + 2})
3. S and a are FORWARD bounds through the fp64 factor R the call was given (taken as exact).  t_ja = sum_{k <= a} R_ak
   c_jk from the computed c, bt_ja as in addscoreref.py; S_jj' = sum_a t_ja t_j'a, a product over M terms on the matrix
   cores in s_depth additions (n for NumPy: never fewer than M):
       bS_jj' = sum_a (bt_ja |t*_j'a| + |t*_ja| bt_j'a + bt_ja bt_j'a)
                + gamma_{s_depth + 2} sum_a (|t*_ja| + bt_ja)(|t*_j'a| + bt_j'a)
   ba as in addscoreref.py, with the score behind r summed at score_depth.
4. Self-check, asserted here so that a bound cannot grow quietly until it hides a failure: bC relative to its mass, and
   bD_jj' and bS_jj' relative to sqrt(D*_jj D*_j'j'), all stay below REL_CEILING = 1e-9.
5. The statistic q = alpha^T V^-1 alpha, alpha = u - a, V = D - S, by a first-order-plus-remainder perturbation bound.
   Scale to unit diagonal with s_j = 1 / sqrt(V*_jj): A = s V* s, b = s alpha*, x = A^-1 b, q* = b^T x.  The computed
   side has A + E and b + delta with |E_jj'| <= e_jj' = s_j s_j' (bD + bS)_jj' + gamma_3 |A_jj'| (the table's own scaling:
   two roundings per entry) plus a symmetric perturbation of 2-norm at most e_host = d ||A||_F gamma_{4 d + 4} for the
   table's fp64 Cholesky factor and forward substitution: L_hat L_hat^T = A + dA with |dA| <= gamma_{d+1} |L||L^T|, (L +
   dL) z = b with |dL| <= gamma_d |L|, so z^T z = b^T (A + E')^-1 b with |E'| <= gamma_{3 d + 2} |L||L^T| and || |L||L^T| ||_2
   <= d ||A||_2 (Higham, Accuracy and Stability, thms 8.5, 10.3, eq. 10.7); the sum z^T z and the division by the
   dispersion are gamma_{d + 8} relative.  |delta_j| <= f_j = s_j (bu + ba)_j + gamma_2 |b_j|.  With eps = ||e||_F +
   e_host >= ||E||_2, phi = ||f||_2, nu = 1 / lambda_min(A), nu' = nu / (1 - eps nu), and from
       (A + E)^-1 = A^-1 - A^-1 E A^-1 + A^-1 E A^-1 E (A + E)^-1:
       |q - q*| <= 2 f^T |x| + |x|^T e |x| + e_host |x|^2                                     (first order)
                   + eps^2 nu nu' |x| |b| + 2 phi eps nu nu' |b| + phi^2 nu'                  (remainder)
   It is valid where eps nu < 1/2 and is asserted only where lambda_min(A) >= 1/16; statistic_reference() asserts that
   EVERY tested group outside the support and outside an explicit `planted` list meets that condition, so no case is
   left out silently, and that the bound itself stays below 1e-9 max(1, q* / phi*).  The dispersion is addscoreref's
   (identity link: evalref's loss bound over sum_w - M; else exactly 1).  Planted
   groups are held to the bounds on u, a, D and S and to "NaN, or finite and >= 0"."""
import numpy as np

import addscoreref
import evalref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = addscoreref.REL_CEILING
UP = addscoreref.UP
LAMBDA_MIN = LD(1) / 16
EIG_SLACK = 1e-12  # lambda_min is taken from an fp64 eigenvalue routine: its error on a d <= 64 unit-diagonal matrix


def device_depths(capi, n, p, m, starts, groups=None, block=0):
    """The chains of additions of a device call, the library's own figures."""
    ws = capi.groupscore_workspace(n, p, m, starts, groups, block)
    return {"depth": int(ws["depth"]), "score": int(ws["score_depth"]), "gram": int(ws["gram_depth"]),
            "s": int(ws["s_depth"])}


def host_depths(n):
    """The NumPy route: every sum is a matrix product over n rows (or over M <= n entries)."""
    return {"depth": n, "score": n, "gram": n, "s": n}


def tested_columns(starts, groups, p):
    starts = np.asarray(starts, dtype=np.int64)
    tested = np.arange(starts.size) if groups is None else np.asarray(groups, dtype=np.int64)
    ends = np.append(starts[1:], p)
    return tested, [np.arange(starts[g], ends[g]) for g in tested]


def chol_solve(A, b):
    """x = A^-1 b in longdouble for a small symmetric positive definite A (np.linalg has no longdouble)."""
    d = A.shape[0]
    L = np.zeros((d, d), dtype=LD)
    for j in range(d):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        assert piv > 0, "the reference matrix is not positive definite"
        L[j, j] = np.sqrt(piv)
        if j + 1 < d:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    z = np.zeros(d, dtype=LD)
    for j in range(d):
        z[j] = (b[j] - L[j, :j] @ z[:j]) / L[j, j]
    x = np.zeros(d, dtype=LD)
    for j in range(d - 1, -1, -1):
        x[j] = (z[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def groupscore_reference(vals, cols, beta, c, y, w, link, R, starts, groups, depths):
    """Reference and bounds of one call.  vals: the (widened) n x p values; R: the fp64 factor the call is given, or None
    (then no S, a); starts / groups: the partition and the tested groups (None = all); depths: device_depths() or
    host_depths().  Returns longdouble u, a (per tested column), lists D, S of d x d blocks, with bounds bu, ba, bD, bS,
    plus what statistic_reference() needs."""
    vals = np.asarray(vals)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, p = vals.shape
    M = cols.size + 1
    tested, glist = tested_columns(starts, groups, p)
    J = np.concatenate(glist)
    pos = np.concatenate([[0], np.cumsum([g.size for g in glist])])
    rt = addscoreref.row_terms(vals, cols, beta, c, y, w, link)
    v, g, rf, dg, Zt = rt["v"], rt["g"], rt["rf"], rt["dg"], rt["Zt"]
    depth, gdepth = depths["depth"], depths["gram"]
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    Xt = np.ascontiguousarray(vals[:, J].astype(LD).T)  # (q, n)
    Pt = np.ascontiguousarray(Zt * v[None, :])
    C = np.einsum("ji,ki->jk", Xt, Pt)
    u, Us = Xt @ g, Zt @ g
    AX, AZ = np.abs(Xt).astype(np.float64), np.abs(Zt).astype(np.float64)
    mass = ((AX * f(v)[None, :]) @ AZ.T).astype(LD)
    bC = ((AX * f(v * (rf + (LD(1) + rf) * gamma(depth + 2)))[None, :]) @ AZ.T).astype(LD) * LD(UP)
    bu = (AX @ f(dg + (np.abs(g) + dg) * gamma(depth + 1))).astype(LD) * LD(UP)
    bU = (AZ @ f(dg + (np.abs(g) + dg) * gamma(depths["score"] + 1))).astype(LD) * LD(UP)
    posm = mass > 0
    rel = (bC[posm] / mass[posm]).max() if posm.any() else LD(0)
    assert rel < REL_CEILING, ("the derived bound on C exceeds its ceiling: choose other inputs", float(rel))
    wD = f(v * (rf + (LD(1) + rf) * gamma(gdepth + 2)))
    D, bD = [], []
    for t in range(len(glist)):
        Xg, Ag = Xt[pos[t]:pos[t + 1]], AX[pos[t]:pos[t + 1]]
        Dg = np.einsum("ji,ki->jk", Xg * v[None, :], Xg)
        bg = ((Ag * wD[None, :]) @ Ag.T).astype(LD) * LD(UP)
        sc = np.sqrt(np.outer(np.diag(Dg), np.diag(Dg)))
        assert ((bg == 0) | (bg < REL_CEILING * sc)).all(), "bound on D"
        D.append(Dg)
        bD.append(bg)
    out = {"u": u, "bu": bu, "C": C, "bC": bC, "D": D, "bD": bD, "score": Us, "bscore": bU, "loss": rt["loss"], "M": M,
           "link": link, "columns": J, "cols": cols, "rel": rel, "tested": tested, "groups": glist, "pos": pos}
    if R is not None:
        Rl = np.tril(np.asarray(R, dtype=np.float64)).astype(LD)
        aR = np.abs(np.tril(np.asarray(R, dtype=np.float64)))
        T = np.einsum("jk,ak->ja", C, np.ascontiguousarray(Rl))
        bt = ((f(bC) @ aR.T) + float(gamma(M + 2)) * (f(np.abs(C) + bC) @ aR.T)).astype(LD) * LD(UP)
        r = Rl.T @ (Rl @ Us)
        AtA = aR.T @ aR
        br = ((AtA @ f(bU)) + float(gamma(2 * M + 2)) * (AtA @ f(np.abs(Us) + bU))).astype(LD) * LD(UP)
        a = C @ r
        ba = (bC @ np.abs(r) + np.abs(C) @ br + bC @ br + gamma(M + 2) * ((np.abs(C) + bC) @ (np.abs(r) + br)))
        gs = gamma(depths["s"] + 2)
        S, bS = [], []
        for t in range(len(glist)):
            Tg, Bg = T[pos[t]:pos[t + 1]], bt[pos[t]:pos[t + 1]]
            aT = np.abs(Tg)
            Sg = Tg @ Tg.T
            bg = Bg @ aT.T + aT @ Bg.T + Bg @ Bg.T + gs * ((aT + Bg) @ (aT + Bg).T)
            sc = np.sqrt(np.outer(np.diag(D[t]), np.diag(D[t])))
            assert ((bg == 0) | (bg < REL_CEILING * sc)).all(), "bound on S"
            S.append(Sg)
            bS.append(bg)
        out.update(S=S, bS=bS, a=a, ba=ba, r=r)
    return out


def _blocks(flat, offsets):
    offsets = np.asarray(offsets, dtype=np.int64)
    d = np.rint(np.sqrt(np.diff(offsets))).astype(np.int64)
    return [np.asarray(flat[offsets[t]:offsets[t + 1]]).reshape(d[t], d[t]) for t in range(d.size)]


def check_blocks(got, ref, what=""):
    """Print the figures, then assert u, a and every block of D and S against their bounds, the offsets, and that every
    returned block equals its transpose exactly."""
    names = [("u", "bu")] + ([("a", "ba")] if "a" in ref else [])
    line = []
    assert np.array_equal(np.asarray(got["columns"]), ref["columns"]), what
    want = np.concatenate([[0], np.cumsum([g.size ** 2 for g in ref["groups"]])])
    assert np.array_equal(np.asarray(got["offsets"]), want), what
    for k, b in names:
        gv = np.asarray(got[k]).astype(LD)
        err = np.abs(gv - ref[k])
        wi = int(np.argmax(err - ref[b]))
        line.append("%s err %.2e bound %.2e" % (k, float(err[wi]), float(ref[b][wi])))
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), (what, k)
        assert (err <= ref[b]).all(), (what, k, wi, float(err[wi]), float(ref[b][wi]))
    for k, b in [("D", "bD")] + ([("S", "bS")] if "S" in ref else []):
        worst = (-np.inf, 0.0, 0.0, -1)
        for t, blk in enumerate(_blocks(got[k], got["offsets"])):
            assert np.array_equal(blk, blk.T), (what, k, t, "a returned block is not symmetric")
            assert np.isfinite(blk).all(), (what, k, t)
            err = np.abs(blk.astype(LD) - ref[k][t])
            wi = np.unravel_index(int(np.argmax(err - ref[b][t])), err.shape)
            if float(err[wi] - ref[b][t][wi]) > worst[0]:
                worst = (float(err[wi] - ref[b][t][wi]), float(err[wi]), float(ref[b][t][wi]), t)
            assert (err <= ref[b][t]).all(), (what, k, t, wi, float(err[wi]), float(ref[b][t][wi]))
        line.append("%s err %.2e bound %.2e (group %d)" % (k, worst[1], worst[2], worst[3]))
    print("%s: %s" % (what, "; ".join(line)))


def statistic_reference(ref, planted=()):
    """Step 5.  planted: tested group numbers left out of the statistic's check.  Returns per tested group: stat (the
    reference), lo, hi (the interval a computed statistic must lie in), ok (where it is asserted), in_model, lam
    (lambda_min of the scaled V*), bound (on the statistic), dispersion.  Asserts that every tested group outside the
    support and outside `planted` has lambda_min >= 1/16 and a bound below 1e-9 max(1, stat*)."""
    nt = len(ref["groups"])
    if ref["link"] == "identity":
        L = ref["loss"]
        dof = L["sum_w"] - LD(ref["M"])
        assert dof > 0
        phi, bphi = L["loss"][0] / dof, (L["bound"][0] + gamma(2) * L["loss"][0]) / dof
    else:
        phi, bphi = LD(1), LD(0)
    assert phi - bphi > 0
    in_model = np.array([bool(np.isin(g, ref["cols"]).any()) for g in ref["groups"]])
    is_planted = np.isin(ref["tested"], np.asarray(planted, dtype=np.int64))
    ok = ~in_model & ~is_planted
    stat, lo, hi = np.zeros(nt, dtype=LD), np.zeros(nt, dtype=LD), np.zeros(nt, dtype=LD)
    lam, bound = np.zeros(nt), np.zeros(nt, dtype=LD)
    alpha, balpha = ref["u"] - ref["a"], ref["bu"] + ref["ba"]
    for t in range(nt):
        if not ok[t]:
            continue
        j0, j1 = ref["pos"][t], ref["pos"][t + 1]
        d = j1 - j0
        V, bV = ref["D"][t] - ref["S"][t], ref["bD"][t] + ref["bS"][t]
        assert (np.diag(V) > 0).all(), ("a tested group has a column that the support reproduces: plant it", t)
        s = LD(1) / np.sqrt(np.diag(V))
        A, b = V * np.outer(s, s), alpha[j0:j1] * s
        lam[t] = float(np.linalg.eigvalsh(A.astype(np.float64))[0]) - EIG_SLACK
        assert lam[t] >= float(LAMBDA_MIN), ("a tested group is nearly collinear (with the support or within itself): "
                                             "plant it explicitly", int(ref["tested"][t]), lam[t])
        x = chol_solve(A, b)
        q = b @ x
        e = bV * np.outer(s, s) + gamma(3) * np.abs(A)
        fb = balpha[j0:j1] * s + gamma(2) * np.abs(b)
        e_host = LD(d) * np.sqrt((A * A).sum()) * LD(UP) * gamma(4 * d + 4)
        g8 = gamma(d + 8)
        eps, ph, nu = np.sqrt((e * e).sum()) + e_host, np.sqrt(fb @ fb), LD(1) / LD(lam[t])
        assert eps * nu < LD(0.5)
        nu2 = nu / (LD(1) - eps * nu)
        nx, nb = np.sqrt(x @ x), np.sqrt(b @ b)
        ax = np.abs(x)
        first = LD(2) * (fb @ ax) + ax @ e @ ax + e_host * nx * nx
        rem = eps * eps * nu * nu2 * nx * nb + LD(2) * ph * eps * nu * nu2 * nb + ph * ph * nu2
        bq = first + rem
        stat[t] = q / phi
        lo[t] = max(q - bq, LD(0)) / (phi + bphi) * (LD(1) - g8)
        hi[t] = (q + bq) / (phi - bphi) * (LD(1) + g8)
        bound[t] = max(hi[t] - stat[t], stat[t] - lo[t])
        assert bound[t] < LD(1e-9) * max(LD(1), stat[t]), ("the statistic's bound is vacuous", t, float(bound[t]))
    return {"stat": stat, "lo": lo, "hi": hi, "ok": ok, "in_model": in_model, "planted": is_planted, "lam": lam,
            "bound": bound, "dispersion": phi}


def check_table(table, st, what=""):
    """Print the figures, then assert a group_score_test_table against statistic_reference: in_model and its NaNs, the
    interval wherever ok, and for planted groups NaN or finite and >= 0."""
    stat = np.asarray(table["statistic"]).astype(LD)
    ok, im = st["ok"], st["in_model"]
    assert np.array_equal(np.asarray(table["in_model"]), im), what
    assert np.isnan(table["statistic"][im]).all() and np.isnan(table["p_value"][im]).all(), what
    err = np.abs(stat[ok] - st["stat"][ok])
    print("%s: %d groups asserted, smallest lambda_min %.3f, largest |stat - stat*| %.3e, largest bound %.3e" % (
        what, int(ok.sum()), float(st["lam"][ok].min()) if ok.any() else float("nan"),
        float(err.max()) if ok.any() else 0.0, float(st["bound"][ok].max()) if ok.any() else 0.0))
    assert np.isfinite(table["statistic"][ok]).all(), what
    assert ((stat[ok] >= st["lo"][ok]) & (stat[ok] <= st["hi"][ok])).all(), what
    pl = table["statistic"][st["planted"] & ~im]
    assert (np.isnan(pl) | (np.isfinite(pl) & (pl >= 0))).all(), what
    pv = table["p_value"][ok]
    assert ((pv >= 0) & (pv <= 1)).all(), what
    assert abs(LD(table["dispersion"]) - st["dispersion"]) <= LD(1e-9) * st["dispersion"], what


def rss_drop_reference(vals, cols, y, w, gcols):
    """The drop in the weighted residual sum of squares on adding the columns gcols to the model (intercept, cols), by
    longdouble normal equations: for the identity link AT THE FITTED OPTIMUM it equals statistic * dispersion."""
    vals = np.asarray(vals)
    n = vals.shape[0]
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    yl = np.asarray(y).astype(LD).reshape(-1)

    def rss(cc):
        Z = np.concatenate([np.ones((n, 1), dtype=LD), vals[:, cc].astype(LD)], axis=1)
        ZW = Z * wl[:, None]
        coef = chol_solve(ZW.T @ Z, ZW.T @ yl)
        res = yl - Z @ coef
        return (wl * res) @ res

    cols = np.asarray(cols, dtype=np.int64)
    return rss(cols) - rss(np.concatenate([cols, np.asarray(gcols, dtype=np.int64)]))
