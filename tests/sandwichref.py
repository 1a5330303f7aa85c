"""Extended-precision reference and error bounds for bessx_meat_device / bessx_sandwich_device, bess_base.inference(...,
cov_type=...) and capi.sandwich_table (shared by tests/test_sandwich_api.py and tests/test_sandwich_gpu.py, in the manner
of tests/inforef.py and tests/diagref.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values.

    z_i = (1, x(i, cols[..])),  u*_i = g*_i (HC0, HC1),  g*_i / sqrt(1 - h*_i) (HC2),  g*_i / (1 - h*_i) (HC3)
    S*(g, a) = sum_{i in g} u*_i z_ia,      B* = sum_g S*(g, :)^T S*(g, :)      (every row its own g without labels)

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u); "(1 r)" marks one rounding.

1. g*_i and dg_i >= |g_hat_i - g*_i| are those of tests/inforef.py step 2, formula for formula (row_scalars below
   repeats them because inforef returns sums only); h*_i and bh_i >= |h_hat_i - h*_i| are those of tests/diagref.py
   steps 1 - 4 (diagref.diagnostics_reference, the factor R being fp64 DATA).
2. u.  HC0 / HC1: bu = dg.  With om = 1 - h (1 r): bom = bh + u (|om*| + bh) (diagref step 9); om_lo = om* - bom > 0 is
   asserted (no row has h* within its bound of 1).
       HC3  u = g / om (1 r):    bu = (1 + u) (dg / om_lo + |g*| bom / (om* om_lo)) + u |g* / om*|
       HC2  s = sqrt(om) (1 r):  bs = (1 + u) bom / sqrt(om*) + u sqrt(om*)  (|sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b)),
            u = g / s (1 r):     bu = (1 + u) (dg / s_lo + |g*| bs / (s* s_lo)) + u |g* / s*|,   s_lo = s* - bs > 0
3. S(g, a): every term u_hat_i z_ia goes through at most `sum_depth` roundings (device: the FMA chain of its run, whose
   products are exact, then the runs in run order -- the figure capi.sandwich_workspace reports for the longest cluster;
   host: the product (1 r) and the cluster's rows in order), and any order of that length obeys gamma_depth:
       bS(g, a) = sum_{i in g} |z_ia| (bu_i + (|u*_i| + bu_i) gamma_{sum_depth + 1})
4. B from S, clustered: an entry is sum_g a_g b_g with a = S_hat(g, a) and b = S_hat(g, b) times a working weight of 1 (at
   most 1 r), the product inside the matrix instruction and `gram_depth` additions (inforef step 3 for the G rows of S
   and the split capi.sandwich_workspace reports; B(0, a) comes from the sweep's score column, B(0, 0) from a chain of
   ceil(G / 256) FMAs and an 8-level tree: gram_depth is the largest of the three; host: G):
       bB(a, b) = sum_g [bS_ga |S*_gb| + |S*_ga| bS_gb + bS_ga bS_gb + (|S*_ga| + bS_ga)(|S*_gb| + bS_gb) gamma_{gram_depth + 3}]
   and the sum vector sum_g S(g, a):  bsum(a) = sum_g [bS_ga + (|S*_ga| + bS_ga) gamma_{gram_depth + 3}].
5. B without labels (device: the sweep over x with the working weight u2 = u_hat u_hat (1 r), b = z_ib u2 (1 r); host: the
   two factors u_hat z_ia, u_hat z_ib (1 r each) and a product of depth n):  bu2_i = (1 + u) bu_i (2 |u*_i| + bu_i) + u u*_i^2,
       bB(a, b) = sum_i |z_ia z_ib| (bu2_i + (u*_i^2 + bu2_i) gamma_{gram_depth + 3})
   with gram_depth = inforef.device_depth(n, m) or n; the sum vector: sum_i |z_ia| (bu_i + (|u*_i| + bu_i) gamma_{gram_depth + 3}).
6. Self-check (a condition on the INPUTS, so that a bound cannot quietly grow until it hides a failure): bB(a, b) <=
   ceiling * sum |.| |.| of the terms it bounds, ceiling = 1e-9 (inforef's) for HC0 / HC1 and 1e-9 / min(1 - h*)^2 for
   HC2 / HC3, where the row scalar magnifies its own error by up to 1 / (1 - h).
7. The covariance (covariance_reference): sandwich_table is given fp64 roundings of a longdouble info and B.  In the scaled
   variables of inforef step 5 (D = diag(info)^(-1/2), S = D info D, P = S^-1, C = D B D): cov = D P C P D.  The computed P
   has ||dP||_2 <= eps ||P||_2 with eps = 2 cond(S) (M u + 8 M^2 u) (the rounding of info to fp64, then inforef step 5's
   factorisation error, the factor 2 for the second order; cond(S) eps < 0.1 asserted), so
       |d(P C P)_jj| <= (2 eps + eps^2) ||P||_2^2 ||C||_2
   plus the rounding of B and of the two matrix products, the scalings by D and the symmetrisation:
   gamma_{2 M + 10} (|P| |C| |P|)_jj.  se = sqrt(cov_jj):  bse = bcov / se* + u se*.  For a table made from a COMPUTED
   info and meat, inforef's relative entry bound r of info joins eps (M (u + r) in place of M u) and the meat's entrywise
   bound bB enters linearly: (|P| D bB D |P|)_jj + (2 eps + eps^2) ||P||_2^2 ||D bB D||_2."""
import numpy as np

import diagref
import evalref
import inforef

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
CEILING = LD(1e-9)


def row_scalars(vals, cols, beta, c, y, w, link, kind="HC0", R=None, host=False):
    """Steps 1 and 2: {"Z" (n, M), "u", "bu", "g", "dg" (n,), "h", "bh" (n,) or None} in longdouble."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, m = np.asarray(vals).shape[0], cols.size
    eta, delta = evalref.eta_reference(vals, cols, np.asarray(beta, dtype=np.float64).reshape(m, 1), [c])
    eta, delta = eta[:, 0], delta[:, 0]
    yl = np.asarray(y).astype(LD).reshape(-1)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    grow, one = np.exp(delta), LD(1)
    if link == "identity":
        mu, dmu = eta, delta
    elif link == "logistic":
        mu = one / (one + np.exp(-eta))
        dmu = mu * (np.expm1(delta) + grow * gamma(4))
    elif link == "poisson":
        mu = np.exp(eta)
        dmu = mu * (np.expm1(delta) + grow * gamma(2))
    else:
        raise ValueError(link)
    g = wl * (yl - mu)
    dg = wl * (dmu + gamma(2) * (np.abs(yl - mu) + dmu))
    Z = np.concatenate([np.ones((n, 1), dtype=LD), np.asarray(vals)[:, cols].astype(LD)], axis=1)
    out = {"Z": Z, "g": g, "dg": dg, "h": None, "bh": None, "kind": kind}
    if kind in ("HC0", "HC1"):
        out.update(u=g, bu=dg)
        return out
    d = diagref.diagnostics_reference(vals, cols, beta, c, y, w, link, R, 1.0, diagref.sum_depth(m + 1, host=host))
    h, bh = d["ref"]["leverage"], d["bound"]["leverage"]
    om = one - h
    bom = bh + U * (np.abs(om) + bh)
    om_lo = om - bom
    assert (om_lo > 0).all(), "a row has h* within its bound of 1: choose other inputs"
    if kind == "HC3":
        u = g / om
        bu = (one + U) * (dg / om_lo + np.abs(g) * bom / (om * om_lo)) + U * np.abs(u)
    else:
        s = np.sqrt(om)
        bs = (one + U) * bom / s + U * s
        s_lo = s - bs
        assert (s_lo > 0).all()
        u = g / s
        bu = (one + U) * (dg / s_lo + np.abs(g) * bs / (s * s_lo)) + U * np.abs(u)
    out.update(u=u, bu=bu, h=h, bh=bh)
    return out


def _segments(labels, n):
    """(order, starts) of the stable sort of the rows by label; labels None: every row its own cluster."""
    if labels is None:
        return np.arange(n), np.arange(n)
    labels = np.asarray(labels).reshape(-1)
    order = np.argsort(labels, kind="stable")
    ls = labels[order]
    return order, np.nonzero(np.concatenate([[True], ls[1:] != ls[:-1]]))[0]


def _f64_nonneg_product(A, B):
    """A^T B for non-negative longdouble arrays through fp64 BLAS, enlarged by 2^-20 (far more than its gamma_n)."""
    return (A.astype(np.float64).T @ B.astype(np.float64)).astype(LD) * (LD(1) + LD(2.0) ** -20)


def _ceiling(rs):
    if rs["h"] is None:
        return CEILING
    return CEILING / (LD(1) - rs["h"].max()) ** 2


def rows_reference(Y, bY_in, labels, sum_depth, gram_depth, ceiling=CEILING):
    """Steps 3 and 4 for rows Y* (n, M) of which the code under test holds values within bY_in (n, M) entrywise (the Cox
    score residuals L with coxdiagref's bound; u z with |z| bu).  Returns longdouble {"S", "S_bound" (G, M) in the order
    of the sorted distinct labels, "meat", "meat_bound" (M, M), "sums", "sums_bound" (M,), "G"}."""
    Y, bY_in = np.asarray(Y).astype(LD), np.asarray(bY_in).astype(LD)
    order, starts = _segments(labels, Y.shape[0])
    bY = (bY_in + (np.abs(Y) + bY_in) * gamma(sum_depth + 1))[order]
    Y = Y[order]
    S = np.add.reduceat(Y, starts, axis=0)
    bS = np.add.reduceat(bY, starts, axis=0)
    A, gd = np.abs(S), gamma(gram_depth + 3)
    meat = S.T @ S
    meat = np.tril(meat) + np.tril(meat, -1).T
    cross = _f64_nonneg_product(bS, A)
    bB = cross + cross.T + _f64_nonneg_product(bS, bS) + _f64_nonneg_product(A + bS, A + bS) * gd
    T = np.add.reduceat(np.abs(Y), starts, axis=0)
    mass = _f64_nonneg_product(T, T)
    pos = mass > 0
    assert (bB[pos] <= ceiling * mass[pos]).all(), ("the derived bound exceeds its ceiling: choose other inputs",
                                                   float((bB[pos] / mass[pos]).max()))
    return {"S": S, "S_bound": bS, "meat": meat, "meat_bound": bB, "sums": S.sum(axis=0),
            "sums_bound": (bS + (A + bS) * gd).sum(axis=0), "G": int(starts.size)}


def clustered_reference(Z, u, bu, labels, sum_depth, gram_depth, ceiling=CEILING):
    """rows_reference for the rows u_i z_i: Z (n, M) exact and a row scalar u with bound bu (None, None: ones, exact)."""
    Z = np.asarray(Z).astype(LD)
    n = Z.shape[0]
    u = np.ones(n, dtype=LD) if u is None else np.asarray(u).astype(LD)
    bu = np.zeros(n, dtype=LD) if bu is None else np.asarray(bu).astype(LD)
    return rows_reference(u[:, None] * Z, np.abs(Z) * bu[:, None], labels, sum_depth, gram_depth, ceiling)


def unclustered_reference(Z, u, bu, gram_depth, ceiling=CEILING):
    """Step 5.  Returns longdouble {"meat", "meat_bound", "sums", "sums_bound"}."""
    Z = np.asarray(Z).astype(LD)
    n = Z.shape[0]
    u = np.ones(n, dtype=LD) if u is None else np.asarray(u).astype(LD)
    bu = np.zeros(n, dtype=LD) if bu is None else np.asarray(bu).astype(LD)
    gd = gamma(gram_depth + 3)
    u2 = u * u
    bu2 = (LD(1) + U) * bu * (LD(2) * np.abs(u) + bu) + U * u2
    Zt = np.ascontiguousarray(Z.T)
    meat = np.einsum("ji,ki->jk", Zt * u2[None, :], Zt)
    meat = np.tril(meat) + np.tril(meat, -1).T
    A = np.abs(Z)
    bB = _f64_nonneg_product(A * (bu2 + (u2 + bu2) * gd)[:, None], A)
    mass = _f64_nonneg_product(A * u2[:, None], A)
    pos = mass > 0
    assert (bB[pos] <= ceiling * mass[pos]).all(), ("the derived bound exceeds its ceiling: choose other inputs",
                                                   float((bB[pos] / mass[pos]).max()))
    return {"meat": meat, "meat_bound": bB, "sums": Zt @ u, "sums_bound": A.T @ (bu + (np.abs(u) + bu) * gd), "G": None}


def device_depths(capi, n, m, labels=None, intercept=True):
    """(sum_depth, gram_depth) of a device call on n rows and a support of m columns: the library's own figures."""
    if labels is None and intercept:
        return 0, inforef.device_depth(capi, n, m)
    if labels is None:
        G, longest = n, 1
    else:
        _, cnt = np.unique(np.asarray(labels), return_counts=True)
        G, longest = int(cnt.size), int(cnt.max())
    ms = m if intercept else m - 1  # (the support of a call whose z has m + 1 entries)
    ws = capi.sandwich_workspace(max(n, 1), ms, n_clusters=G, max_cluster_rows=longest)
    gram = int(ws["cluster_rows_per_slab"]) + (int(ws["cluster_slabs"]) + 15) // 16 + 4
    return int(ws["sum_depth"]), max(gram + 1, int(ws["sq_depth"]))


def host_depths(n, labels=None):
    """(sum_depth, gram_depth) of the fp64 NumPy route."""
    if labels is None:
        return 1, n
    _, cnt = np.unique(np.asarray(labels), return_counts=True)
    return int(cnt.max()) + 1, int(cnt.size)


def meat_reference(vals, cols, beta, c, y, w, link, kind, R, labels, depths, host=False):
    """Reference and bounds of one sandwich call: clustered_reference / unclustered_reference on the row scalars of
    steps 1 and 2; depths = (sum_depth, gram_depth).  Adds "rows" (row_scalars' dict)."""
    rs = row_scalars(vals, cols, beta, c, y, w, link, kind, R, host=host)
    if labels is None:
        out = unclustered_reference(rs["Z"], rs["u"], rs["bu"], depths[1], _ceiling(rs))
    else:
        out = clustered_reference(rs["Z"], rs["u"], rs["bu"], labels, depths[0], depths[1], _ceiling(rs))
    out["rows"] = rs
    return out


def add_bounds(a, b):
    """The bound of a comparison of two routes that are each within their own bound of the same reference."""
    return {k: (a[k] + b[k] if k.endswith("_bound") else a[k]) for k in a if k in b and k != "rows"}


def check_meat(got, ref, what="", factor=1):
    """Print the figures, then assert meat (and sums when got has them) against the bounds and meat == meat.T."""
    gm = np.asarray(got["meat"]).astype(LD)
    em, bm = np.abs(gm - ref["meat"]), LD(factor) * ref["meat_bound"]
    wi = np.unravel_index(int(np.argmax(em - bm)), em.shape)
    msg = "%s: meat err %.3e against bound %.3e at %s" % (what, float(em[wi]), float(bm[wi]), wi)
    ok_s = True
    if got.get("sums") is not None:
        es, bs = np.abs(np.asarray(got["sums"]).astype(LD) - ref["sums"]), LD(factor) * ref["sums_bound"]
        ws = int(np.argmax(es - bs))
        msg += "; sums err %.3e against bound %.3e at %d" % (float(es[ws]), float(bs[ws]), ws)
        ok_s = bool((es <= bs).all())
    print(msg)
    assert np.isfinite(np.asarray(got["meat"], dtype=np.float64)).all(), what
    assert np.array_equal(np.asarray(got["meat"]), np.asarray(got["meat"]).T), what
    assert (em <= bm).all(), (what, wi, float(em[wi]), float(bm[wi]))
    assert ok_s, what


def covariance_reference(info, meat, scale=1, info_rel=0, meat_bound=None):
    """Step 7 for longdouble info and meat (M, M): (cov*, se*, bound on cov's diagonal, bound on se, cond(S*)).  info_rel,
    meat_bound: for a table made from a COMPUTED info and meat, inforef's relative entry bound of info (it joins the
    rounding of info in eps) and the entrywise bound of meat (the covariance is linear in it: |A*| bB |A*|, A* =
    inv(info*), enlarged by (1 + eps)^2 for the computed A)."""
    info, meat = np.asarray(info).astype(LD), np.asarray(meat).astype(LD)
    M = info.shape[0]
    d = LD(1) / np.sqrt(np.diag(info))
    S = info * d[:, None] * d[None, :]
    ev = np.linalg.eigvalsh(S.astype(np.float64))
    cond = float(ev[-1] / ev[0])
    assert cond < inforef.COND_CEILING, cond
    P = inforef.ld_inverse_spd(S)
    C = meat * d[:, None] * d[None, :]
    cov = LD(scale) * (P @ C @ P) * d[:, None] * d[None, :]
    eps = LD(2) * LD(cond) * (LD(M) * (U + LD(info_rel)) + LD(8 * M * M) * U)
    assert LD(cond) * eps < LD(0.1)
    nP = LD(np.linalg.norm(P.astype(np.float64), 2)) * (LD(1) + LD(2.0) ** -20)
    nC = LD(np.linalg.norm(C.astype(np.float64), 2)) * (LD(1) + LD(2.0) ** -20)
    chain = np.diag(np.abs(P) @ np.abs(C) @ np.abs(P))
    inner = (LD(2) * eps + eps * eps) * nP * nP * nC + gamma(2 * M + 10) * chain
    if meat_bound is not None:
        bC = np.asarray(meat_bound).astype(LD) * d[:, None] * d[None, :]
        nbC = LD(np.linalg.norm(bC.astype(np.float64), 2)) * (LD(1) + LD(2.0) ** -20)
        inner = inner + np.diag(np.abs(P) @ bC @ np.abs(P)) + (LD(2) * eps + eps * eps) * nP * nP * nbC
    bdiag = abs(LD(scale)) * d * d * inner
    se = np.sqrt(np.diag(cov))
    return cov, se, bdiag, bdiag / se + U * se, cond
