"""Extended-precision reference and error bounds for bessx_cox_groupscore_device / capi.cox_groupscore_device /
bess_base.score_tests_groups_survival (shared by tests/test_cox_groupscore_api.py and tests/test_cox_groupscore_gpu.py, in
the manner of tests/coxaddscoreref.py and tests/groupscoreref.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values, EVENT BY EVENT and NOT by the library's
decomposition.  Positions, r(k), e*, wd, S0* as in coxinforef.  The positions are walked from the last to the first with
the running sums over the risk set {l >= p} of e*, e* z, e* x, e* z x^T and, per tested group J, e* z_J z_J^T (x the
support's columns, z the tested columns).  At the head p of a risk set, with W = sum of wd_k over the events k with
r(k) = p, mean E[.] = (running sum) / S0*:
    u*  = sum_k wd_k z_k - sum_p W E[z]              C* += W (E[z x^T] - E[z] E[x]^T)            (q x m)
    D*_J += W E[z_J z_J^T]        T*_J += W E[z_J] E[z_J]^T        V*_J += W Cov(z_J) = D*_J - T*_J (checked)
and with the fp64 factor R the call was given (taken as exact): r* = R^T (R score*), a* = C* r*, S*_J = (C*_J R^T)(C*_J
R^T)^T.  self_check() holds all of it to coxinforef.direct_definition's O(n^2) loops on the model extended by a group, at
n <= 40.

The bounds are derived; u = 2^-53, gamma_k = k u / (1 - k u); weights are non-negative.  rho_l, rho, sigma, tau, rv_l,
dg_l, ru are coxaddscoreref.row_terms() (items 1 to 6 of coxinforef).
A. u and C: coxaddscoreref's items A and B at the depth the library reports for its split (n for NumPy).
B. D: groupscoreref's item 2 with v of the Cox model:
       |D_jj' - D*_jj'| <= sum_l v*_l |z_lj z_lj'| (rv_l + (1 + rv_l) gamma_{gram_depth + 2}).
C. T_jj' = sum_p cc_p s_p[j] s_p[j'].  Every elementary term cc_p a_l a_l' (l, l' >= p, a = e z) carries the relative
   error ra = (1 + rho)(1 + u) - 1 of each a and tcc = (1 + tdh)(1 + u) / (1 - sigma) - 1 of cc (coxaddscoreref item C,
   without a scan of cc) and passes through at most t_depth further roundings (the library's figure for its slabs, the
   carries and the finish; 3 n + 8 for the NumPy route: two suffix sums and a matrix product):
       |T_jj' - T*_jj'| <= mass_jj' ((1 + ra)^2 (1 + tcc)(1 + gamma_{t_depth}) - 1),
       mass_jj' = sum_p cc*_p |s|_j(p) |s|_j'(p),   |s| the suffix sums of |e* z|.
D. S and a: FORWARD bounds through the fp64 factor from bC (groupscoreref item 3 with M = m, coxaddscoreref item D), the
   score behind r at the depth score_depth.
E. Each of these is multiplied by a CONSTANT (C_U, C_A, C_D, C_T, C_S below): four times the largest ratio error / bound
   that fp64 NumPy (bess_base._cox_score_tests_groups_host, depths host_depths(n)) needs on cases(), rounded up to a
   power of two, with no floor.  tests/test_cox_groupscore_api.py measures the maxima and asserts that the constants follow
   from them; the measured value stands next to each constant.
F. Self-check: the bounds of u, a, D, T, S stay below REL_CEILING = 1e-9 of their masses (D and S: of sqrt(D*_jj D*_j'j')).
G. The statistic: groupscoreref.statistic_reference() (its item 5) with D := D* - T*, bD := bD + bT and dispersion 1:
   valid where the reference's V scaled to unit diagonal has lambda_min >= 1/16, which it asserts for every tested group
   outside the support and outside an explicit `planted` list, as it asserts bound < 1e-9 max(1, statistic).  The
   half-widths of its interval are multiplied by C_STAT, fixed the same way."""
import numpy as np

import coxaddscoreref
import coxinforef
import evalref
import groupscoreref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = coxaddscoreref.REL_CEILING
UP = coxaddscoreref.UP

# largest error / derived bound of fp64 NumPy over cases(), measured by tests/test_cox_groupscore_api.py::
# test_fp64_numpy_fixes_the_constants (it prints them), and the constants that follow (constant_from)
U_NUMPY_MAX = 0.01742
A_NUMPY_MAX = 0.002624
D_NUMPY_MAX = 0.03747
T_NUMPY_MAX = 0.009044
S_NUMPY_MAX = 0.006424
STAT_NUMPY_MAX = 0.0409   # (against the interval that the five constants below give)
C_U = 0.125        # 4 x 0.01742 = 0.06968, rounded up to a power of two
C_A = 0.015625     # 4 x 0.002624 = 0.0105, rounded up to a power of two
C_D = 0.25         # 4 x 0.03747 = 0.1499, rounded up to a power of two
C_T = 0.0625       # 4 x 0.009044 = 0.03618, rounded up to a power of two
C_S = 0.03125      # 4 x 0.006424 = 0.0257, rounded up to a power of two
C_STAT = 0.25      # 4 x 0.0409 = 0.1636, rounded up to a power of two


def constant_from(measured):
    """The next power of two at or above four times the measured maximum."""
    return float(2.0 ** np.ceil(np.log2(4.0 * measured)))


def device_depths(capi, n, p, m, n_event_rows, starts, groups=None, block=0):
    """The chains of additions of a device call, the library's own figures."""
    ws = capi.cox_groupscore_workspace(n, p, m, n_event_rows, starts, groups, block)
    return {"depth": int(ws["depth"]), "score": int(ws["score_depth"]), "gram": int(ws["gram_depth"]),
            "s": int(ws["s_depth"]), "t": int(ws["t_depth"])}


def host_depths(n):
    """The NumPy route: matrix products and running sums over n rows."""
    return {"depth": int(n), "score": int(n), "gram": int(n), "s": int(n), "t": 3 * int(n) + 8}


def _sfx(a):
    return np.cumsum(a[::-1], axis=0)[::-1]


def event_moments(e, r, ev, wd, x, Z, pos):
    """The event-by-event risk-set moments (module docstring): u, C, lists D, T, V per tested group and the support's
    score, all longdouble.  pos: the list position of every tested group's first column (+ q)."""
    n, q = Z.shape
    m = x.shape[1]
    W = np.zeros(n, dtype=LD)
    np.add.at(W, r[ev], wd[ev])
    nt = len(pos) - 1
    S0, S1z, S1x, S2x = LD(0), np.zeros(q, dtype=LD), np.zeros(m, dtype=LD), np.zeros((q, m), dtype=LD)
    S2 = [np.zeros((pos[t + 1] - pos[t],) * 2, dtype=LD) for t in range(nt)]
    u = (wd[ev][:, None] * Z[ev]).sum(axis=0)
    us = (wd[ev][:, None] * x[ev]).sum(axis=0)
    C = np.zeros((q, m), dtype=LD)
    D, T, V = [np.zeros_like(s) for s in S2], [np.zeros_like(s) for s in S2], [np.zeros_like(s) for s in S2]
    for l in range(n - 1, -1, -1):
        ez = e[l] * Z[l]
        S0 = S0 + e[l]
        S1z += ez
        S1x += e[l] * x[l]
        if m:
            S2x += np.outer(ez, x[l])
        for t in range(nt):
            S2[t] += np.outer(ez[pos[t]:pos[t + 1]], Z[l, pos[t]:pos[t + 1]])
        if W[l] == 0:
            continue
        mz, mx = S1z / S0, S1x / S0
        u -= W[l] * mz
        us -= W[l] * mx
        if m:
            C += W[l] * (S2x / S0 - np.outer(mz, mx))
        for t in range(nt):
            mg = mz[pos[t]:pos[t + 1]]
            second, outer = S2[t] / S0, np.outer(mg, mg)
            D[t] += W[l] * second
            T[t] += W[l] * outer
            V[t] += W[l] * (second - outer)
    return u, C, D, T, V, us


def cox_groupscore_reference(vals, cols, beta, time, status, w, ties, R, starts, groups, depths):
    """Reference and bounds of one call.  vals: the (widened) n x p values; R: the fp64 factor (m, m) the call is given, or
    None (then no S, a; m = 0: S = a = 0); starts / groups: the partition and the tested groups (None = all); depths:
    device_depths() or host_depths().  Returns longdouble u, a (per tested column), lists D, T, S of d x d blocks, with
    bounds bu, ba, bD, bT, bS (the constants of item E included), plus what statistic_reference() needs."""
    vals = np.asarray(vals)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, p = vals.shape
    tested, glist = groupscoreref.tested_columns(starts, groups, p)
    J = np.concatenate(glist)
    pos = np.concatenate([[0], np.cumsum([g.size for g in glist])]).astype(np.int64)
    nt = len(glist)
    x, eta, delta, wd, d, order, first, last, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
    assert (wd >= 0).all(), "the bounds are derived for non-negative weights"
    m = x.shape[1]
    rt = coxaddscoreref.row_terms(x, eta, delta, wd, d, first, last, ties)
    e, r, S0, v, g, ev = rt["e"], rt["r"], rt["S0"], rt["v"], rt["g"], rt["ev"]
    Z = np.ascontiguousarray(vals[:, J].astype(LD)[order])
    u, C, D, T, V, Us = event_moments(e, r, ev, wd, x, Z, pos)
    one = LD(1)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    AZ = np.abs(Z).astype(np.float64)
    rv, dg, rho_l, rho, sigma, tau, ru = rt["rv"], rt["dg"], rt["rho_l"], rt["rho"], rt["sigma"], rt["tau"], rt["ru"]
    depth, gdepth, tdepth = int(depths["depth"]), int(depths["gram"]), int(depths["t"])
    bu = (AZ.T @ f(dg + (np.abs(g) + dg) * gamma(depth + 1))).astype(LD) * LD(UP) * LD(C_U)                  # A
    mass_u = (AZ.T @ f(np.abs(g) + v)).astype(LD)
    S0pos = _sfx(e)
    dh = np.zeros(n, dtype=LD)
    np.add.at(dh, r, wd / S0)
    tdh = tau + gamma(n - 1) * (one + tau)
    ax = np.abs(x)
    apc = _sfx(e[:, None] * ax) / S0pos[:, None] if m else np.zeros((n, 0), dtype=LD)
    AA = np.cumsum(dh[:, None] * apc, axis=0)
    rA1 = (one + tdh) * (one + ru) * (one + U) - one
    bA = AA * (rA1 + (one + rA1) * gamma(n - 1))
    rvp = (one + rv) * (one + U) - one
    M1, M2 = v[:, None] * ax, e[:, None] * AA
    err_in = M1 * rvp[:, None] + M2 * ((one + rho_l) * (one + U) - one)[:, None] + \
        (e * (one + rho_l) * (one + U))[:, None] * bA
    bP = err_in + U * (M1 + M2 + err_in)
    mass_c = (AZ.T @ f(M1 + M2)).astype(LD)
    bC = (AZ.T @ f(bP + (M1 + M2 + bP) * gamma(depth + 2))).astype(LD) * LD(UP)
    wD = f(v * (rv + (one + rv) * gamma(gdepth + 2)))                                                        # B
    ra = (one + rho) * (one + U) - one                                                                       # C
    tcc = (one + tdh) * (one + U) / (one - sigma) - one
    relT = (one + ra) ** 2 * (one + tcc) * (one + gamma(tdepth)) - one
    cc = f(dh / S0pos)
    sabs = _sfx(f(e)[:, None] * AZ)
    bD, bT, massT = [], [], []
    for t in range(nt):
        Ag, sg = AZ[:, pos[t]:pos[t + 1]], sabs[:, pos[t]:pos[t + 1]]
        bg = ((Ag * wD[:, None]).T @ Ag).astype(LD) * LD(UP) * LD(C_D)
        mt = ((sg * cc[:, None]).T @ sg).astype(LD) * LD(UP)
        sc = np.sqrt(np.outer(np.diag(D[t]), np.diag(D[t])))
        assert ((bg == 0) | (bg < REL_CEILING * sc)).all(), "bound on D"                                    # F
        assert (relT * LD(C_T) < REL_CEILING), ("bound on T", float(relT))
        assert (np.abs(V[t] - (D[t] - T[t])) <= LD(2.0) ** -50 * (sc + LD(1e-300))).all()
        bD.append(bg)
        bT.append(mt * relT * LD(C_T))
        massT.append(mt)
    for name, b, ms in (("u", bu, mass_u), ("C", bC, mass_c)):
        ok = ms > 0
        assert (b[~ok] == 0).all(), ("a bound without a mass", name)
        rel = (b[ok] / ms[ok]).max() if ok.any() else LD(0)
        assert rel < REL_CEILING, ("the derived bound on %s exceeds its ceiling: choose other inputs" % name, float(rel))
    out = {"u": u, "bu": bu, "C": C, "bC": bC, "D": D, "bD": bD, "T": T, "bT": bT, "massT": massT, "score": Us, "m": m,
           "columns": J, "cols": cols, "tested": tested, "groups": glist, "pos": pos, "link": "cox", "M": m,
           "n_events": wd.sum(), "J": int(ev.sum())}
    if m == 0:
        z = np.zeros(J.size, dtype=LD)
        zs = [np.zeros((g.size, g.size), dtype=LD) for g in glist]
        out.update(a=z, ba=z.copy(), S=zs, bS=[s.copy() for s in zs])
    elif R is not None:                                                                                      # D
        cs = int(depths["score"])
        bU = (ax.astype(np.float64).T @ f(dg + (np.abs(g) + dg) * gamma(cs + 1))).astype(LD) * LD(UP)
        Rl = np.tril(np.asarray(R, dtype=np.float64)).astype(LD)
        aR = np.abs(np.tril(np.asarray(R, dtype=np.float64)))
        TC = np.einsum("jk,ak->ja", C, np.ascontiguousarray(Rl))
        bt = ((f(bC) @ aR.T) + float(gamma(m + 3)) * (f(np.abs(C) + bC) @ aR.T)).astype(LD) * LD(UP)
        rr = Rl.T @ (Rl @ Us)
        AtA = aR.T @ aR
        br = ((AtA @ f(bU)) + float(gamma(2 * m + 2)) * (AtA @ f(np.abs(Us) + bU))).astype(LD) * LD(UP)
        a = C @ rr
        ba = (bC @ np.abs(rr) + np.abs(C) @ br + bC @ br + gamma(m + 3) * ((np.abs(C) + bC) @ (np.abs(rr) + br))) * LD(C_A)
        mass_a = mass_c @ np.abs(rr)
        ok = mass_a > 0
        assert (ba[~ok] == 0).all() and (not ok.any() or (ba[ok] / mass_a[ok]).max() < REL_CEILING), "bound on a"
        gs = gamma(int(depths["s"]) + 2)
        S, bS = [], []
        for t in range(nt):
            Tg, Bg = TC[pos[t]:pos[t + 1]], bt[pos[t]:pos[t + 1]]
            aT = np.abs(Tg)
            bg = (Bg @ aT.T + aT @ Bg.T + Bg @ Bg.T + gs * ((aT + Bg) @ (aT + Bg).T)) * LD(C_S)
            sc = np.sqrt(np.outer(np.diag(D[t]), np.diag(D[t])))
            assert ((bg == 0) | (bg < REL_CEILING * sc)).all(), "bound on S"
            S.append(Tg @ Tg.T)
            bS.append(bg)
        out.update(S=S, bS=bS, a=a, ba=ba, r=rr)
    return out


def ratios(got, ref):
    """The largest error / bound of u, a and of the entries of D, T, S (0 where the bound is 0 and so is the error)."""
    def worst(err, b):
        err, b = np.asarray(err, dtype=LD), np.asarray(b, dtype=LD)
        assert (err[b == 0] == 0).all()
        return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    out = {"u": worst(np.abs(np.asarray(got["u"]).astype(LD) - ref["u"]), ref["bu"])}
    if "a" in ref:
        out["a"] = worst(np.abs(np.asarray(got["a"]).astype(LD) - ref["a"]), ref["ba"])
    for k in ("D", "T") + (("S",) if "S" in ref else ()):
        blocks = groupscoreref._blocks(got[k], got["offsets"])
        out[k] = max(worst(np.abs(blk.astype(LD) - ref[k][t]), ref["b" + k][t]) for t, blk in enumerate(blocks))
    return out


def check_blocks(got, ref, what=""):
    """Print the figures, then assert u, a and every block of D, T and S against their bounds, the offsets, and that every
    returned block equals its transpose exactly."""
    groupscoreref.check_blocks(got, ref, what)
    worst = (-np.inf, 0.0, 0.0, -1)
    for t, blk in enumerate(groupscoreref._blocks(got["T"], got["offsets"])):
        assert np.array_equal(blk, blk.T), (what, "T", t, "a returned block is not symmetric")
        assert np.isfinite(blk).all(), (what, "T", t)
        err = np.abs(blk.astype(LD) - ref["T"][t])
        wi = np.unravel_index(int(np.argmax(err - ref["bT"][t])), err.shape)
        if float(err[wi] - ref["bT"][t][wi]) > worst[0]:
            worst = (float(err[wi] - ref["bT"][t][wi]), float(err[wi]), float(ref["bT"][t][wi]), t)
        assert (err <= ref["bT"][t]).all(), (what, "T", t, wi, float(err[wi]), float(ref["bT"][t][wi]))
    print("%s: T err %.2e bound %.2e (group %d)" % (what, worst[1], worst[2], worst[3]))


def statistic_reference(ref, planted=()):
    """Item G: groupscoreref.statistic_reference on V = (D - T) - S, the half-widths of its interval times C_STAT."""
    view = dict(ref)
    view["D"] = [d - t for d, t in zip(ref["D"], ref["T"])]
    view["bD"] = [bd + bt for bd, bt in zip(ref["bD"], ref["bT"])]
    st = groupscoreref.statistic_reference(view, planted)
    st["lo"] = np.maximum(st["stat"] - LD(C_STAT) * (st["stat"] - st["lo"]), LD(0))
    st["hi"] = st["stat"] + LD(C_STAT) * (st["hi"] - st["stat"])
    st["bound"] = st["bound"] * LD(C_STAT)
    return st


check_table = groupscoreref.check_table


def lambda_min(ref):
    """lambda_min of the reference's V scaled to unit diagonal, per tested group (NaN where a diagonal entry is <= 0)."""
    out = np.full(len(ref["groups"]), np.nan)
    for t in range(out.size):
        V = (ref["D"][t] - ref["T"][t]) - ref["S"][t]
        dg = np.diag(V)
        if (dg > 0).all():
            s = LD(1) / np.sqrt(dg)
            out[t] = float(np.linalg.eigvalsh((V * np.outer(s, s)).astype(np.float64))[0])
    return out


def case(n, m, widths, weighted=True, all_tied=False, dtype=np.float64, support_group=None, collinear=None):
    """One seeded problem: standard-normal columns in groups of the given widths, times on a grid of eighths (real tie
    groups) or all equal, censoring, weights in eighths with zeros.  support_group: the group that is the model's
    support (its width must be m), else m scattered columns; collinear: a group (width >= 3) whose third column is the
    sum of its first two."""
    widths = np.asarray(widths, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(np.int64)
    p = int(widths.sum())
    rng = np.random.default_rng(11 * n + 5 * m + int(weighted) + (3 if dtype == np.float32 else 0))
    X = rng.standard_normal((n, p)).astype(dtype)
    if collinear is not None:
        c0 = int(starts[collinear])
        X[:, c0 + 2] = X[:, c0] + X[:, c0 + 1]
    if support_group is not None:
        assert widths[support_group] == m
        cols = np.arange(starts[support_group], starts[support_group] + m)
    else:
        cols = np.sort(rng.choice(p, m, replace=False))
    beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
    beta = np.where(beta == 0, 0.1, beta)
    time = np.ceil(rng.exponential(np.exp(-(X[:, cols].astype(np.float64) @ beta))) * 8) / 8
    if all_tied:
        time[:] = 1.0
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    wv = rng.integers(0, 17, n) / 8.0 if weighted else None
    return dict(X=X, cols=cols.astype(np.int32), beta=beta, time=time, status=status, w=wv, starts=starts, widths=widths)


CPU_WIDTHS = [5, 1, 3, 17, 2, 16, 33, 1, 4]  # p = 82; group 2 is the support of m = 3, group 8 is collinear
CPU_SHAPES = [(31, 0), (37, 3), (127, 3), (1025, 3), (4097, 3)]


def cases():
    """The seeded CPU cases the constants are fixed on: (name, case, ties)."""
    out = []
    for n, m in CPU_SHAPES:
        for ties in ("order", "breslow"):
            for weighted in (False, True):
                cs = case(n, m, CPU_WIDTHS, weighted, support_group=2 if m else None, collinear=8)
                out.append(("n%d-m%d-%s-%s" % (n, m, ties, "w" if weighted else "1"), cs, ties))
    out.append(("all-tied", case(127, 3, CPU_WIDTHS, True, all_tied=True, support_group=2, collinear=8), "breslow"))
    return out


def self_check(seed=0):
    """The event-by-event reference against coxinforef's O(n^2) direct definition of the model extended by one GROUP at
    coefficient 0 (its last d score entries, its cross rows and its trailing d x d block), for both ties values, with
    weights (some zero), censoring and heavy ties, at n <= 40."""
    rng = np.random.default_rng(seed)
    for n, m, weighted in ((1, 0, False), (2, 1, True), (23, 0, True), (40, 3, True), (37, 2, False)):
        widths = [2, 1, 4, 3]
        p = sum(widths)
        vals = rng.standard_normal((n, p))
        cols = np.arange(3, 3 + m)  # (inside the 4-wide group)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        time = np.round(rng.exponential(1.0, n), 1)
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0 if weighted else None
        starts = np.concatenate([[0], np.cumsum(widths)[:-1]])
        for ties in ("order", "breslow"):
            ref = cox_groupscore_reference(vals, cols, beta, time, status, w, ties, None, starts, None, host_depths(n))
            x, eta, _, wd, d, order, first, _, _ = coxinforef._ordered(vals, cols, beta, time, status, w)
            tol = LD(n + 8) * LD(2.0) ** -56
            for t, gc in enumerate(ref["groups"]):
                xe = np.concatenate([x, vals[:, gc].astype(LD)[order]], axis=1)
                info, score = coxinforef.direct_definition(xe, eta, wd, d, first, ties)
                j0, j1 = ref["pos"][t], ref["pos"][t + 1]
                sc = np.abs(ref["D"][t]).max() + np.abs(ref["T"][t]).max() + LD(1e-300)
                assert np.abs(score[m:] - ref["u"][j0:j1]).max() <= tol * ((np.abs(xe[:, m:]) * wd[:, None]).sum() * 2 + LD(1e-300))
                assert np.abs(info[m:, m:] - (ref["D"][t] - ref["T"][t])).max() <= tol * sc, (n, ties, t)
                if m:
                    assert np.abs(info[m:, :m] - ref["C"][j0:j1]).max() <= tol * 64 * (np.abs(ref["C"][j0:j1]).max() + sc)
    return True


# the problems of tests/test_cox_groupscore_gpu.py: tests/test_groupscore_gpu.py's 27 widths (p = 406: a group starts at
# every offset of a 16-column tile, groups straddle one, two and four tile boundaries, the 64-wide one starts at offset 15)
GPU_WIDTHS = np.array([31, 5, 3, 17, 31, 1, 17, 33, 5, 64, 16, 1, 3, 15, 31, 15, 5, 1, 5, 31, 15, 3, 17, 1, 5, 2, 33])
GPU_STARTS = np.concatenate([[0], np.cumsum(GPU_WIDTHS)[:-1]])
GPU_P = int(GPU_WIDTHS.sum())
GPU_SUPPORT_GROUP = {3: 2, 31: 4}  # m -> the group that is the model's support (m = 0: the null model)
GPU_COLLINEAR = 8                  # a group whose third column is the sum of its first two
# (n, m, ties, all_tied): n = 37 one short slab past a 32-position chunk, 1025 one position past the 1024-position scan
# block, 4097 twenty-six position slabs
GPU_CASES = [(37, 3, "order", False), (37, 31, "breslow", False), (1025, 0, "breslow", False), (1025, 31, "order", False),
             (1025, 3, "breslow", True), (4097, 3, "breslow", False), (4097, 31, "order", False)]


def gpu_problem(dt, n, m, all_tied=False):
    """One model per (dtype, n, m, all_tied), the same logical values under every layout."""
    return case(n, m, GPU_WIDTHS, True, all_tied=all_tied, dtype=np.float32 if dt == "f32" else np.float64,
                support_group=GPU_SUPPORT_GROUP.get(m), collinear=GPU_COLLINEAR)
