"""Extended-precision reference and error bounds for bessx_diag_device / bess_base.diagnostics (shared by
tests/test_diag_api.py and tests/test_diag_gpu.py, in the manner of tests/inforef.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values; eta* and its per-row bound Delta_i come
from evalref.eta_reference (any order of an m-term dot product plus one addition, so the analysis does not depend on
which of the loops of bessx_k_xb.hpp formed eta).  The factor R and the dispersion phi are fp64 DATA: the reference uses
exactly the numbers the code under test is given.

    z_i = (1, x(i, cols[0]), ...),   t*_ij = sum_{k <= j} R_jk z_ik,   S*_i = sum_j t*_ij^2,   h*_i = v*_i S*_i

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u); "(1 r)" marks one rounding.

1. rf_i (relative error of v_i and, without the weight, of V_i) and dmu_i (|mu_hat - mu*|) are those of tests/inforef.py
   steps 1 and 2, formula for formula.
2. t: an at most M-term dot product inside the matrix instruction, whatever order it adds in, and (host route) the same
   products added column by column:                    |t_hat_ij - t*_ij| <= e_ij = gamma_{M+1} a_ij,  a_ij = sum_k |R_jk z_ik|
3. S: every square (1 r, none when fused) and `depth` additions in a fixed order (device: the tiles' squares per lane,
   then 4 levels of the DPP tree: depth = ceil(M / 16) + 4, capi-independent and stated by sum_depth(); host: M):
       |S_hat - S*| <= bS = (1 + gamma_{depth+1}) sum_j e_ij (2 |t*_ij| + e_ij) + gamma_{depth+1} S*
4. h = v_hat * S_hat (1 r):    |h_hat - h*| <= bh = (1 + u) (v* (1 + rf) bS + rf h*) + u h*
5. response r = y - mu_hat (1 r):                      br = dmu + u (|r*| + dmu)
6. pearson = (sqrt(w) (1 r) * r (1 r)) / sqrt(V_hat) (1 r) (1 r), V_hat = V* (1 + eps), |eps| <= rf: the factor that
   multiplies sqrt(w) r_hat / sqrt(V*) lies within theta = (1 + u)^3 / ((1 - u) sqrt(1 - rf)) - 1 of 1:
       brp = sqrt(w / V*) (br (1 + theta) + |r*| theta)
7. unit deviance d.  f is the loss term of tests/evalref.py; its derivative in eta is mu - y, and between eta* and
   eta_hat mu stays within dmu of mu*, so |f(eta_hat) - f(eta*)| <= (|y - mu*| + dmu) Delta; its own roundings are
   evalref's q (logistic: u (4 log 2 + 2 e + 2 s + 2 |y| |eta|), Poisson: u (3 e + 2 |y| |eta|), magnitudes at |eta*| +
   Delta).  A = y log y: log 1 ulp = 2 u, the product (1 r): gamma_4 |A*|.  B = (1 - y) log(1 - y) (logistic): 1 - y
   (1 r) moves the logarithm by at most u / (1 - u): gamma_4 |B*| + 2 u |1 - y|; B = -y (Poisson) is exact.  Two
   additions (1 r each), the factor 2 is exact:
       bd = 2 ((1 + gamma_2) (df + dA + dB) + gamma_2 (|f*| + |A*| + |B*|))
   identity: e = y - eta_hat (1 r): be = Delta + u (|e*| + Delta); d = e e (1 r): bd = (1 + u) be (2 |e*| + be) + u d*.
   max(., 0) does not increase a distance (d* >= 0).
8. deviance residual: a = w * max(d, 0) (1 r): ba = (1 + u) w bd + u a*; the square root: |sqrt(a_hat) - sqrt(a*)| <=
   sqrt(|a_hat - a*|), and <= |a_hat - a*| / sqrt(a*) away from 0 (the quotient form, since sqrt(a_hat) + sqrt(a*) >=
   sqrt(a*)); its own (1 r):          brd = (1 + u) min(sqrt(ba), ba / sqrt(a*)) + u sqrt(a*)
   The sign is that of y - mu_hat, which is the sign of y - mu* as no row has |y - mu*| <= dmu (asserted).
9. om = 1 - h (1 r): bom = bh + u (|om*| + bh);  P = phi * om (1 r): bP = (1 + u) phi bom + u P*;  den = sqrt(P) (1 r):
   bden = (1 + u) bP / sqrt(P*) + u den*  (quotient form; P* > bP is asserted: no row has h within its bound of 1).
   A quotient x / den (1 r), den_lo = den* - bden:
       b(x / den) = (1 + u) (bx / den_lo + |x*| bden / (den* den_lo)) + u |x* / den*|
10. cooks = ((rp rp) (1 r) h) (1 r) / ((phi M) (1 r) (om om) (1 r)) (1 r) (1 r):
       bN = (1 + gamma_2) (brp (2 |rp*| + brp) (h* + bh) + rp*^2 bh) + gamma_2 N*
       bD = (1 + gamma_3) phi M bom (2 |om*| + bom) + gamma_3 D*,     D_lo = D* - bD > 0
       bck = (1 + u) (bN / D_lo + N* bD / (D* D_lo)) + u N* / D*

Self-checks, asserted here so that a bound cannot quietly grow until it hides a failure (conditions on the INPUTS):
    bh_i / (v*_i sum_j a_ij^2) < REL_CEILING = 1e-9 (inforef's ceiling);   bh_i <= 1e-6 h*_i wherever h*_i > 0;
    no row has |y_i - mu*_i| <= dmu_i."""
import numpy as np

import evalref
import inforef

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
KINDS = ("leverage", "response", "pearson", "deviance", "std_pearson", "std_deviance", "cooks")


def sum_depth(M, host=False):
    """The additions behind one row's sum of t^2 (step 3): the device's ceil(M / 16) + 4, the NumPy route's M."""
    return M if host else (M + 15) // 16 + 4


def _xlogx(a):
    return np.where(a == 0, LD(0), a * np.log(np.where(a == 0, LD(1), a)))


def geometry(vals, cols, R):
    """What steps 2 and 3 need of (vals, cols, R) alone, so that the links, responses and weights of one design share
    it: S* (n,), E = sum_j e_ij (2 |t*_ij| + e_ij) (n,) and A2 = sum_j a_ij^2 (n,).  (|Z| |R|^T is a sum of non-negative
    terms: fp64 BLAS forms it to a relative gamma_M, far inside the 2^-20 by which it is enlarged.)"""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, M = np.asarray(vals).shape[0], cols.size + 1
    Rl = np.tril(np.asarray(R, dtype=np.float64)).astype(LD)
    Z = np.concatenate([np.ones((n, 1), dtype=LD), np.asarray(vals)[:, cols].astype(LD)], axis=1)
    Rt = np.ascontiguousarray(Rl.T)
    T = np.empty((n, M), dtype=LD)
    for j0 in range(0, M, 32):  # (R is lower triangular: columns j0 .. j1 - 1 of T take entries k < j1 of z only)
        j1 = min(M, j0 + 32)
        T[:, j0:j1] = np.ascontiguousarray(Z[:, :j1]) @ np.ascontiguousarray(Rt[:j1, j0:j1])
    Aabs = (np.abs(Z).astype(np.float64) @ np.abs(Rt).astype(np.float64)).astype(LD) * (LD(1) + LD(2.0) ** -20)
    e_t = gamma(M + 1) * Aabs
    return {"S": (T * T).sum(axis=1), "E": (e_t * (LD(2) * np.abs(T) + e_t)).sum(axis=1), "A2": (Aabs * Aabs).sum(axis=1)}


def diagnostics_reference(vals, cols, beta, c, y, w, link, R, phi, depth, geom=None, factor_rel=0, phi_rel=0):
    """Reference and bounds of one call.  vals: the (widened) n x p values; cols, beta (m,), c; y (n,), w (n,) or None;
    R (M, M) fp64, lower triangle used; phi; depth: sum_depth(M); geom: geometry(vals, cols, R) when the caller shares
    it.  factor_rel, phi_rel: for a code under test that used ANOTHER factor and dispersion than R and phi, how far
    z^T R^T R z and the dispersion may lie from these, relatively (added to bh, bP and bD; 0: the same numbers).
    Returns {"ref": {kind: (n,) longdouble}, "bound": {kind: (n,) longdouble}, "h_sum_bound": sum of the leverage
    bounds}."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, m = np.asarray(vals).shape[0], cols.size
    M = m + 1
    eta, delta = evalref.eta_reference(vals, cols, np.asarray(beta, dtype=np.float64).reshape(m, 1), [c])
    eta, delta = eta[:, 0], delta[:, 0]
    yl = np.asarray(y).astype(LD).reshape(-1)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    grow, mag = np.exp(delta), np.abs(eta) + delta
    one = LD(1)
    if link == "identity":
        mu, V, rf, dmu = eta, np.ones(n, dtype=LD), np.zeros(n, dtype=LD), delta
        es = np.abs(yl - eta)
        d = (yl - eta) ** 2
        be = delta + U * (es + delta)
        bd = (one + U) * be * (LD(2) * es + be) + U * d
    elif link == "logistic":
        mu = one / (one + np.exp(-eta))
        V = mu * (one / (one + np.exp(eta)))
        rf = np.expm1(delta) + grow * gamma(7)
        dmu = mu * (np.expm1(delta) + grow * gamma(4))
        e = np.exp(-np.abs(eta))
        f = np.maximum(eta, LD(0)) + np.log1p(e) - yl * eta
        s = np.maximum(eta, LD(0)) + delta + np.log1p(e)
        q = U * (LD(4) * evalref.LOG2 + LD(2) * e + LD(2) * s + LD(2) * np.abs(yl) * mag)
        A, B = _xlogx(yl), _xlogx(one - yl)
        dB = gamma(4) * np.abs(B) + LD(2) * U * np.abs(one - yl)
    elif link == "poisson":
        mu = np.exp(eta)
        V = mu
        rf = np.expm1(delta) + grow * gamma(3)
        dmu = mu * (np.expm1(delta) + grow * gamma(2))
        f = mu - yl * eta
        q = U * (LD(3) * np.exp(eta + delta) + LD(2) * np.abs(yl) * mag)
        A, B = _xlogx(yl), -yl
        dB = np.zeros(n, dtype=LD)
    else:
        raise ValueError(link)
    r = yl - mu
    assert not (np.abs(r) <= dmu).any(), "a row has |y - mu*| <= dmu (its sign could flip): choose other inputs"
    if link != "identity":
        df = (np.abs(r) + dmu) * delta + q
        d = LD(2) * ((f + A) + B)
        bd = LD(2) * ((one + gamma(2)) * (df + gamma(4) * np.abs(A) + dB) + gamma(2) * (np.abs(f) + np.abs(A) + np.abs(B)))
        d = np.maximum(d, LD(0))
    v = wl * V
    # steps 2 - 4
    if geom is None:
        geom = geometry(vals, cols, R)
    S = geom["S"]
    bS = (one + gamma(depth + 1)) * geom["E"] + gamma(depth + 1) * S
    h = v * S
    bh = (one + U) * (v * (one + rf) * bS + rf * h) + U * h + LD(factor_rel) * h
    mass = v * geom["A2"]
    pos = mass > 0
    rel = (bh[pos] / mass[pos]).max() if pos.any() else LD(0)
    assert rel < inforef.REL_CEILING, ("the derived leverage bound exceeds its ceiling: choose other inputs", float(rel))
    hp = h > 0
    assert (bh[hp] <= LD(1e-6) * h[hp]).all(), "the leverage bound exceeds 1e-6 h*: choose other inputs"
    # steps 5, 6, 8
    br = dmu + U * (np.abs(r) + dmu)
    theta = (one + U) ** 3 / ((one - U) * np.sqrt(one - rf)) - one
    scale = np.sqrt(wl / V)
    rp = scale * r
    brp = scale * (br * (one + theta) + np.abs(r) * theta)
    a = wl * d
    ba = (one + U) * wl * bd + U * a
    sa = np.sqrt(a)
    quot = np.where(a > 0, ba / np.where(a > 0, sa, one), np.sqrt(ba))
    rd = np.sign(r) * sa
    brd = (one + U) * np.minimum(np.sqrt(ba), quot) + U * sa
    # steps 9, 10
    phi = LD(phi)
    om = one - h
    bom = bh + U * (np.abs(om) + bh)
    P = phi * om
    bP = (one + U) * phi * bom + (U + LD(phi_rel)) * np.abs(P)
    assert (P > bP).all(), "a row has h* within its bound of 1: choose other inputs"
    den = np.sqrt(P)
    bden = (one + U) * bP / den + U * den
    den_lo = den - bden
    assert (den_lo > 0).all()

    def quotient(x, bx):
        return (one + U) * (bx / den_lo + np.abs(x) * bden / (den * den_lo)) + U * np.abs(x / den)

    N = rp * rp * h
    bN = (one + gamma(2)) * (brp * (LD(2) * np.abs(rp) + brp) * (h + bh) + rp * rp * bh) + gamma(2) * N
    D = phi * LD(M) * om * om
    bD = (one + gamma(3)) * phi * LD(M) * bom * (LD(2) * np.abs(om) + bom) + (gamma(3) + LD(phi_rel)) * D
    D_lo = D - bD
    assert (D_lo > 0).all()
    bck = (one + U) * (bN / D_lo + N * bD / (D * D_lo)) + U * N / D
    ref = {"leverage": h, "response": r, "pearson": rp, "deviance": rd, "std_pearson": rp / den,
           "std_deviance": rd / den, "cooks": N / D}
    bound = {"leverage": bh, "response": br, "pearson": brp, "deviance": brd, "std_pearson": quotient(rp, brp),
             "std_deviance": quotient(rd, brd), "cooks": bck}
    return {"ref": ref, "bound": bound, "h_sum_bound": bh.sum(), "M": M}


def check_diagnostics(got, ref, what="", factor=1):
    """Print every kind's worst error against its bound, then assert; got: {kind: (n,) array} (any subset of KINDS);
    factor: 2 when two routes that are each within their bound are compared."""
    worst = []
    for k in KINDS:
        if k not in got:
            continue
        g = np.asarray(got[k]).astype(LD)
        err, b = np.abs(g - ref["ref"][k]), LD(factor) * ref["bound"][k]
        with np.errstate(divide="ignore", invalid="ignore"):  # (the row that uses most of its bound)
            i = int(np.argmax(np.where(b > 0, err / b, np.where(err > 0, np.inf, 0))))
        worst.append((k, i, float(err[i]), float(b[i]), bool(np.isfinite(np.asarray(got[k], dtype=np.float64)).all()),
                      bool((err <= b).all())))
    print("%s: %s" % (what, "; ".join("%s err %.3e against bound %.3e at %d" % (w[0], w[2], w[3], w[1])
                                      for w in worst)))
    for k, i, e, b, finite, ok in worst:
        assert finite, (what, k, "not finite")
        assert ok, (what, k, i, e, b)
