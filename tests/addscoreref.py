"""Extended-precision reference and error bounds for bessx_addscore_device / bess_base.score_tests (shared by
tests/test_addscore_api.py and tests/test_addscore_gpu.py, in the manner of tests/inforef.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values.  eta* and its per-row bound Delta_i
come from evalref.eta_reference; v*, g* and the row factors rf_i (relative error of v_i) and dg_i (absolute error of g_i)
are steps 1 and 2 of tests/inforef.py, unchanged (row_terms() repeats their formulas).  With z_i = (1, x(i, cols[..])),
M = m + 1, and for every candidate column j:

    u*_j = sum_i g*_i x_ij,    c*_j = sum_i v*_i x_ij z_i,    d*_j = sum_i v*_i x_ij^2.

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).

3. Sums (step 3 of inforef.py for these operands).  On the device the right-hand operand v_hat_i z_ik is rounded once
   when the panel is written, the product is formed inside the matrix instruction (at most one rounding) and a wave adds
   the rows of its slab -- rows_per_slab terms, however the instruction orders the four products of an issue; the
   finish kernel adds ceil(slabs / 16) partials per lane in slab order and then 4 levels of the DPP tree:
       depth_device = rows_per_slab + ceil(slabs / 16) + 4            (device_depth(): the split is the library's)
   d_j: a lane adds its rows_per_slab / 4 rows by fma(v, x * x, .) -- x * x is one more rounding --, the four k lanes of
   a candidate are 3 more additions, then the same finish: never more than depth_device.  The NumPy route is a matrix
   product over n rows, P = v * Z and x * x rounded once each: depth_host = n.
       |C_jk - C*_jk| <= sum_i v*_i |x_ij z_ik| (rf_i + (1 + rf_i) gamma_{depth + 2})
       |u_j  - u*_j | <= sum_i |x_ij| (dg_i + (|g*_i| + dg_i) gamma_{depth + 1})
       |d_j  - d*_j | <= sum_i v*_i x_ij^2 (rf_i + (1 + rf_i) gamma_{depth + 3})
4. s and a are FORWARD bounds through the fp64 factor R the call was given (taken as exact):  t_ja = sum_{k <= a} R_ak
   c_jk, an M-term product on the matrix cores (or in BLAS) from the computed c:
       bt_ja = sum_k |R_ak| bC_jk + gamma_{M + 2} sum_k |R_ak| (|c*_jk| + bC_jk)
   s_j = sum_a t_ja^2 by fma at the depth the statistic kernel reports (sum_depth = tiles + 4; n for NumPy):
       bs_j = sum_a bt_ja (2 |t*_ja| + bt_ja) + gamma_{sum_depth + 2} sum_a (|t*_ja| + bt_ja)^2
   r = R^T (R U) is formed on the host in fp64 from a score U that the device sums in the order of step 3 over the
   constant column and the support (depth_score; it differs from the returned score by rounding only), so with bU the
   u-type bound of that score
       br = |R|^T |R| bU + gamma_{2 M + 2} |R|^T |R| (|U*| + bU)
       ba_j = sum_k (bC_jk |r*_k| + |c*_jk| br_k + bC_jk br_k) + gamma_{M + 2} sum_k (|c*_jk| + bC_jk) (|r*_k| + br_k)
5. Self-check, asserted here so that a bound cannot grow quietly until it hides a failure: the bound on C relative to
   sum_i v*_i |x_ij z_ik|, the bound on d relative to d* and the bound on s relative to d* all stay below REL_CEILING =
   1e-9 (where d* = 0 -- a column that is zero on every row of positive weight -- the bounds must be 0 as well).
6. The statistic, by interval arithmetic in longdouble: adj in adj* +- (bu + ba), variance in var* +- (bd + bs),
   dispersion in phi* +- bphi (identity link: evalref's loss bound over sum_w - M; else exactly 1), and gamma_8 for the
   five fp64 operations of score_test_table.  It is asserted only where var* >= d* / 16; statistic_reference() asserts
   that EVERY candidate outside the support and outside an explicit `planted` list meets that condition, so no case is
   left out silently.  Planted near-collinear columns are held to the bounds on d and s and to "NaN or finite and >= 0"."""
import numpy as np

import evalref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = LD(1e-9)
UP = 1.0 + 2.0 ** -20  # the fp64 BLAS sums of non-negative terms behind the bounds are enlarged by this


def device_depths(capi, n, m, q, block=0):
    """(depth of an entry of u, C, d; depth of the score behind r; depth of a sum of squares) of a device call: the split
    is the library's own figure."""
    ws = capi.addscore_workspace(n, m, q, block)
    w0 = capi.addscore_workspace(n, m, m + 1, 0)
    return (int(ws["rows_per_slab"]) + (int(ws["slabs"]) + 15) // 16 + 4,
            int(w0["rows_per_slab"]) + (int(w0["slabs"]) + 15) // 16 + 4, int(ws["sum_depth"]))


def row_terms(vals, cols, beta, c, y, w, link):
    """Steps 1 and 2 of inforef.py: longdouble v*, g*, rf, dg (n,), Z^T (M, n) contiguous, and evalref's loss reference."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, m = np.asarray(vals).shape[0], cols.size
    eta, delta = evalref.eta_reference(vals, cols, np.asarray(beta, dtype=np.float64).reshape(m, 1), [c])
    loss = evalref.loss_reference(eta, delta, y, w, link)
    eta, delta = eta[:, 0], delta[:, 0]
    yl = np.asarray(y).astype(LD).reshape(-1)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    grow = np.exp(delta)
    if link == "identity":
        mu, v, rf, dmu = eta, wl.copy(), np.zeros(n, dtype=LD), delta
    elif link == "logistic":
        mu = LD(1) / (LD(1) + np.exp(-eta))
        v = wl * mu * (LD(1) / (LD(1) + np.exp(eta)))
        rf = np.expm1(delta) + grow * gamma(7)
        dmu = mu * (np.expm1(delta) + grow * gamma(4))
    elif link == "poisson":
        mu = np.exp(eta)
        v = wl * mu
        rf = np.expm1(delta) + grow * gamma(3)
        dmu = mu * (np.expm1(delta) + grow * gamma(2))
    else:
        raise ValueError(link)
    g = wl * (yl - mu)
    dg = wl * (dmu + gamma(2) * (np.abs(yl - mu) + dmu))
    Zt = np.ascontiguousarray(np.concatenate([np.ones((n, 1), dtype=LD), np.asarray(vals)[:, cols].astype(LD)], axis=1).T)
    return {"v": v, "g": g, "rf": rf, "dg": dg, "Zt": Zt, "loss": loss}


def addscore_reference(vals, cols, beta, c, y, w, link, R, candidates, depth, depth_score, sum_depth):
    """Reference and bounds of one call.  vals: the (widened) n x p values; R: the fp64 factor the call is given, or None
    (then no s, a); candidates: column numbers or None = all; the three depths of steps 3 and 4.  Returns longdouble
    arrays u, C, d, s, a with bounds bu, bC, bd, bs, ba, plus score U*, "loss" (evalref) and M."""
    vals = np.asarray(vals)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, p = vals.shape
    M = cols.size + 1
    J = np.arange(p) if candidates is None else np.asarray(candidates, dtype=np.int64)
    rt = row_terms(vals, cols, beta, c, y, w, link)
    v, g, rf, dg, Zt = rt["v"], rt["g"], rt["rf"], rt["dg"], rt["Zt"]
    Xt = np.ascontiguousarray(vals[:, J].astype(LD).T)  # (q, n)
    Pt = np.ascontiguousarray(Zt * v[None, :])
    C = np.einsum("ji,ki->jk", Xt, Pt)
    u, d, Us = Xt @ g, (Xt * Xt) @ v, Zt @ g
    AX, AZ = np.abs(Xt).astype(np.float64), np.abs(Zt).astype(np.float64)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    mass = ((AX * f(v)[None, :]) @ AZ.T).astype(LD)
    bC = ((AX * f(v * (rf + (LD(1) + rf) * gamma(depth + 2)))[None, :]) @ AZ.T).astype(LD) * LD(UP)
    bu = (AX @ f(dg + (np.abs(g) + dg) * gamma(depth + 1))).astype(LD) * LD(UP)
    bd = ((AX * AX) @ f(v * (rf + (LD(1) + rf) * gamma(depth + 3)))).astype(LD) * LD(UP)
    bU = (AZ @ f(dg + (np.abs(g) + dg) * gamma(depth_score + 1))).astype(LD) * LD(UP)
    pos = mass > 0
    rel = (bC[pos] / mass[pos]).max() if pos.any() else LD(0)
    assert rel < REL_CEILING, ("the derived bound on C exceeds its ceiling: choose other inputs", float(rel))
    dp = d > 0
    assert (bd[~dp] == 0).all() and (not dp.any() or (bd[dp] / d[dp]).max() < REL_CEILING), "bound on d"
    out = {"u": u, "bu": bu, "C": C, "bC": bC, "d": d, "bd": bd, "score": Us, "bscore": bU, "loss": rt["loss"], "M": M,
           "link": link, "columns": J, "cols": cols, "rel": rel}
    if R is not None:
        Rl = np.tril(np.asarray(R, dtype=np.float64)).astype(LD)
        aR = np.abs(np.tril(np.asarray(R, dtype=np.float64)))
        t = np.einsum("jk,ak->ja", C, np.ascontiguousarray(Rl))
        bt = ((f(bC) @ aR.T) + float(gamma(M + 2)) * (f(np.abs(C) + bC) @ aR.T)).astype(LD) * LD(UP)
        s = (t * t).sum(axis=1)
        bs = (bt * (LD(2) * np.abs(t) + bt)).sum(axis=1) + gamma(sum_depth + 2) * ((np.abs(t) + bt) ** 2).sum(axis=1)
        r = Rl.T @ (Rl @ Us)
        AtA = aR.T @ aR
        br = ((AtA @ f(bU)) + float(gamma(2 * M + 2)) * (AtA @ f(np.abs(Us) + bU))).astype(LD) * LD(UP)
        a = C @ r
        ba = (bC @ np.abs(r) + np.abs(C) @ br + bC @ br + gamma(M + 2) * ((np.abs(C) + bC) @ (np.abs(r) + br)))
        assert (bs[~dp] == 0).all() and (not dp.any() or (bs[dp] / d[dp]).max() < REL_CEILING), "bound on s"
        out.update(s=s, bs=bs, a=a, ba=ba, r=r)
    return out


def check_vectors(got, ref, what="", cross=True):
    """Print the figures, then assert u, d (and C, s, a where both sides have them) against their bounds."""
    names = [("u", "bu"), ("d", "bd")] + ([("s", "bs"), ("a", "ba")] if "s" in ref else [])
    if cross and "cross" in got:
        names.append(("cross", "bC"))
    line = []
    for k, b in names:
        gv = np.asarray(got[k]).astype(LD)
        rv = ref["C"] if k == "cross" else ref[k]
        assert gv.shape == rv.shape, (what, k, gv.shape, rv.shape)
        err = np.abs(gv - rv)
        wi = np.unravel_index(int(np.argmax(err - ref[b])), err.shape)
        line.append("%s err %.2e bound %.2e" % (k, float(err[wi]), float(ref[b][wi])))
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), (what, k)
        assert (err <= ref[b]).all(), (what, k, wi, float(err[wi]), float(ref[b][wi]))
    print("%s: %s" % (what, "; ".join(line)))


def statistic_reference(ref, sum_w_minus_M=None, planted=()):
    """Step 6.  Returns dict: adj, var, stat (reference), lo, hi (the interval a computed statistic must lie in), ok
    (where it is asserted), in_model, dispersion, ratio = var* / d*.  Asserts that every candidate outside the support
    and outside `planted` has var* >= d* / 16."""
    adj, var = ref["u"] - ref["a"], ref["d"] - ref["s"]
    badj, bvar = ref["bu"] + ref["ba"], ref["bd"] + ref["bs"]
    if ref["link"] == "identity":
        L = ref["loss"]
        dof = L["sum_w"] - LD(ref["M"])
        assert dof > 0
        phi, bphi = L["loss"][0] / dof, (L["bound"][0] + gamma(2) * L["loss"][0]) / dof
    else:
        phi, bphi = LD(1), LD(0)
    in_model = np.isin(ref["columns"], ref["cols"])
    is_planted = np.isin(ref["columns"], np.asarray(planted, dtype=np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ref["d"] > 0, var / ref["d"], LD(0))
    ok = ~in_model & ~is_planted
    assert (ratio[ok] >= LD(1) / 16).all(), ("a candidate is nearly collinear with the support: plant it explicitly",
                                            float(ratio[ok].min()))
    assert (var[ok] - bvar[ok] > 0).all() and phi - bphi > 0
    lo_adj = np.maximum(np.abs(adj) - badj, LD(0))
    hi_adj = np.abs(adj) + badj
    g8 = gamma(8)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(ok, lo_adj * lo_adj / ((phi + bphi) * (var + bvar)) * (LD(1) - g8), LD(0))
        hi = np.where(ok, hi_adj * hi_adj / ((phi - bphi) * (var - bvar)) * (LD(1) + g8), LD(0))
        stat = np.where(ok, adj * adj / (phi * var), LD(0))
    return {"adj": adj, "var": var, "stat": stat, "lo": lo, "hi": hi, "ok": ok, "in_model": in_model,
            "dispersion": phi, "ratio": ratio, "badj": badj, "bvar": bvar, "planted": is_planted}


def check_table(table, st, what=""):
    """Print the figures, then assert a score_test_table against statistic_reference: in_model and its NaNs, the
    interval wherever ok, and for planted columns NaN or finite and >= 0."""
    stat = np.asarray(table["statistic"]).astype(LD)
    ok, im = st["ok"], st["in_model"]
    assert np.array_equal(np.asarray(table["in_model"]), im), what
    assert np.isnan(table["statistic"][im]).all() and np.isnan(table["p_value"][im]).all(), what
    width = (st["hi"][ok] - st["lo"][ok]) / np.maximum(st["stat"][ok], LD(1e-300))
    err = np.abs(stat[ok] - st["stat"][ok])
    print("%s: %d candidates asserted, smallest var*/d* %.3f, largest |stat - stat*| %.3e, widest interval %.3e relative" % (
        what, int(ok.sum()), float(st["ratio"][ok].min()) if ok.any() else float("nan"),
        float(err.max()) if ok.any() else 0.0, float(width.max()) if ok.any() else 0.0))
    assert np.isfinite(table["statistic"][ok]).all(), what
    assert ((stat[ok] >= st["lo"][ok]) & (stat[ok] <= st["hi"][ok])).all(), what
    pl = table["statistic"][st["planted"] & ~im]
    assert (np.isnan(pl) | (np.isfinite(pl) & (pl >= 0))).all(), what
    pv = table["p_value"][ok]
    assert ((pv >= 0) & (pv <= 1)).all(), what
    assert abs(LD(table["dispersion"]) - st["dispersion"]) <= LD(1e-9) * st["dispersion"], what
