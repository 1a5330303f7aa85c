"""Extended-precision reference and error bounds for the weighted pair counts of bessx_cox_auc_device / bessx_auc_device,
capi.cox_auc_device / auc_device and bess_base.auc_survival / auc (shared by tests/test_pairauc_api.py and
tests/test_pairauc_gpu.py).

Definitions (w_i >= 0 the weights, a_i the inverse-probability-of-censoring weight of row i, h(x, y) = 1(x > y)).
    AUC(t_j):  cases time_i <= t_j carrying w_i a_i, controls time_l > t_j carrying w_l;
               greater[j, r] = sum_cases sum_controls w_i a_i w_l h(eta_ir, eta_lr), equal[j, r]: 1(eta_ir = eta_lr);
               cases[j] = sum w_i a_i 1(time_i <= t_j), controls[j] = sum w_l 1(time_l > t_j);
               auc = (greater + equal / 2) / (cases controls), NaN where a factor is 0.
    mean_auc:  sum_j auc[j] d_j / sum_j d_j over the times ascending, d_j = S^(t_(j-1)) - S^(t_j), S^ the weighted
               Kaplan-Meier survival of the rows, over the times with d_j > 0; NaN if one of those auc is NaN or none is.
    Uno's C:   pairs status_i = 1, time_i < time_l (strictly), time_i < tau carrying w_i a_i^2 w_l: concordant, tied,
               comparable; uno_c = (concordant + tied / 2) / comparable, NaN without a pair.
    ROC AUC:   cases y > 0.5, controls y <= 0.5, both carrying w.
The reference works straight from these, O(n^2) in np.longdouble, ONE requested time at a time: a matrix of cases x
controls per time.  It is not the segment matrix of the kernel and not the sort of the NumPy route.  a (row_a) is DATA
here: the fp64 values the implementation used (checked on their own with coxbrierref.check_ipcw).

Inputs that make every comparison decidable (exact_problem): X entries are integers / 8 in [-4, 4], B entries integers
/ 4, m <= 16: every partial sum of eta is a multiple of 1/32 below 2^9, exactly representable in fp32 products and fp64
sums, so eta is the SAME number in any order of summation, under every layout, and for an fp32 X; ties in eta are exact.

Two kinds of comparison.
    EXACT    censoring=None (a = status) and weights None or integers / 8: every term w a w, w a^2 w is a multiple of
             1/64 and every sum stays far below 2^53 / 64: fp64 sums are exact in any order, so the sums must EQUAL the
             reference.  (Logistic: weight=None only, every term an integer.)
    BOUNDED  otherwise: every numerator is a sum of non-negative terms.  With u = 2^-53: the inner sum over l adds at
             most n terms (n u), the products w a (or w a a) and their product with the inner sum round 3 times (3 u),
             the outer sum over k adds at most n terms (n u) and the cells of the segment matrix at most T + 1 more
             ((T + 1) u): relative error at most (2 n + T + 8) u = rel_bound(n, T), in any order of summation.  The
             same bound holds for cases, controls and comparable (fewer operations).  rel_bound is asserted below 1e-9.
    Quotients, to first order in quantities below 1e-9 (the neglected squares are below 1e-18 u^-1 u = far below u):
             auc    = (g + e / 2) / (cases controls): numerator rel (one addition, + u), two factors rel, one product
                      (u), one division (u):                              3 rel + 3 u  -> auc_rel = 3 rel + 4 u
             uno_c  = (c + t / 2) / comparable:                            2 rel + 2 u  -> uno_rel = 2 rel + 3 u
             mean   = sum_j auc_j d_j / sum_j d_j with d (km_drop) taken as DATA (>= 0): a product (u) and at most T
                      additions (T u) above, T additions below, a division: auc_rel + (2 T + 3) u.
             km_drop is held to the longdouble Kaplan-Meier estimate absolutely: S^ is a product of at most K factors
             (Y - ev) / Y, each from two sums of at most n non-negative weights, an addition and a division (2 gamma_n +
             3 u), S^ <= 1, and a drop is a difference of two of them (u): 2 K (2 gamma_n + 3 u) + u = km_bound(K, n).

self_check() holds the vectorised reference to a plain double loop over pairs at small n."""
import numpy as np

import coxevalref
import evalref

LD = np.longdouble
U = evalref.U
gamma = evalref.gamma
REL_CEILING = LD(1e-9)
TILE = 1024  # PAIRAUC_TILE of bessx_dev.h


def _ld(a):
    return np.asarray(a).astype(LD)


def exact_problem(n, m, R, P=24, seed=0, nmax=None):
    """X (n x P) with entries integers / 8 in [-4, 4], m ascending support columns, B (m, R) with entries integers / 4 in
    [-2, 2]; the first n rows of a draw of nmax rows, so that problems of different n share their leading rows."""
    rng = np.random.default_rng(1000 + seed + 7 * m)
    X = (rng.integers(-32, 33, (nmax or n, P)) / 8.0)[:n]
    cols = np.sort(rng.choice(P, m, replace=False)).astype(np.int32)
    B = rng.integers(-8, 9, (m, 3))[:, :R] / 4.0
    return X, cols, B


def survival_data(n, ties=False, seed=0, nmax=None):
    """(time, status): continuous times in an order that is not the rows' (ties: 20 distinct values, events and
    censorings sharing them), about 60% events; the first n of nmax draws."""
    rng = np.random.default_rng(2000 + seed)
    time = rng.exponential(1.0, nmax or n)[:n] + 0.05
    if ties:
        time = np.ceil(rng.uniform(0.0, 20.0, nmax or n))[:n] / 4.0
    status = (rng.uniform(size=nmax or n) < 0.6).astype(np.float64)[:n]
    return time, status


def weights(n, kind, nmax=None):
    """None ("none"), integers / 8 in [1/8, 2] ("eighths"), the same with every third row at 0 ("zeros")."""
    if kind == "none":
        return None
    w = np.random.default_rng(5).integers(1, 17, nmax or n)[:n] / 8.0
    if kind == "zeros":
        w[::3] = 0.0
        w[0] = 1.0
    return w


def eta_exact(vals, cols, B):
    """eta (n, R) in longdouble; asserts that it is exactly representable in fp64 (so every route holds the same)."""
    eta, delta = evalref.eta_reference(vals, cols, B, np.zeros(np.shape(B)[1]))
    assert np.array_equal(eta, np.asarray(eta, dtype=np.float64).astype(LD))
    assert np.array_equal(eta * 32, np.round(eta * 32)) and (np.abs(eta) < 2.0 ** 9).all()
    return eta


def rel_bound(n, T):
    b = LD(2 * n + T + 8) * U
    assert b < REL_CEILING
    return b


def auc_rel(n, T):
    return LD(3) * rel_bound(n, T) + LD(4) * U


def uno_rel(n):
    return LD(2) * rel_bound(n, 0) + LD(3) * U


def km_bound(K, n):
    return LD(2 * K) * (LD(2) * gamma(n) + LD(3) * U) + U


def pair_sums(eta, time, cw, lw, t):
    """(greater, equal (R,), cases, controls) at ONE time t: cases time <= t carrying cw, controls time > t carrying lw."""
    eta, cw, lw = _ld(eta), _ld(cw), _ld(lw)
    case = np.asarray(time) <= t
    ck, wl = cw[case], lw[~case]
    g, e = np.zeros(eta.shape[1], dtype=LD), np.zeros(eta.shape[1], dtype=LD)
    for r in range(eta.shape[1]):
        ek, el = eta[case, r], eta[~case, r]
        g[r] = (ck * np.where(ek[:, None] > el[None, :], wl[None, :], LD(0)).sum(axis=1)).sum()
        e[r] = (ck * np.where(ek[:, None] == el[None, :], wl[None, :], LD(0)).sum(axis=1)).sum()
    return g, e, ck.sum(), wl.sum()


def km_survival(time, status, w, times):
    """(S^ at the times, the number of event times): the weighted Kaplan-Meier survival by its definition, longdouble."""
    time, status = np.asarray(time, dtype=np.float64), np.asarray(status, dtype=np.float64)
    wl = _ld(w)
    ev_times = np.unique(time[(status != 0) & (np.asarray(w) > 0)])
    f = np.array([LD(1) - wl[(time == v) & (status != 0)].sum() / wl[time >= v].sum() for v in ev_times], dtype=LD)
    S = np.array([np.prod(f[ev_times <= t]) if f.size else LD(1) for t in times], dtype=LD)
    return S, ev_times.size


def cox_auc_reference(eta, times, time, status, w, row_a, tau):
    """The whole dict of capi.cox_auc_device in longdouble (the time axis in the order of `times`), except mean_auc,
    which mean_auc_reference forms from the implementation's km_drop; plus "km_drop" by the definition and "K"."""
    eta = _ld(eta)
    n, R = eta.shape
    time, status = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(status, dtype=np.float64).reshape(-1)
    times = np.asarray([] if times is None else times, dtype=np.float64).reshape(-1)
    T = times.size
    wl = np.ones(n, dtype=LD) if w is None else _ld(w).reshape(-1)
    a = _ld(row_a).reshape(-1)
    out = {k: np.zeros((T, R), dtype=LD) for k in ("greater", "equal")}
    out.update({k: np.zeros(T, dtype=LD) for k in ("cases", "controls")})
    for j, t in enumerate(times):
        out["greater"][j], out["equal"][j], out["cases"][j], out["controls"][j] = pair_sums(eta, time, wl * a, wl, t)
    den = out["cases"] * out["controls"]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["auc"] = np.where(den[:, None] > 0, (out["greater"] + out["equal"] / 2) / np.where(den > 0, den, 1)[:, None],
                              LD(np.nan))
    order = np.argsort(times, kind="stable")
    S, K = km_survival(time, status, wl, times[order])
    drop = np.zeros(T, dtype=LD)
    drop[order] = np.concatenate([[LD(1)], S])[:T] - S
    out["km_drop"], out["K"] = drop, K
    # Uno's C: blocks of case rows against every row
    c2 = np.where((status != 0) & ~(time >= (np.nan if tau is None else tau)), wl * a * a, LD(0))
    conc, tied, comp = np.zeros(R, dtype=LD), np.zeros(R, dtype=LD), LD(0)
    rows = np.nonzero(c2 > 0)[0]
    for b0 in range(0, rows.size, 256):
        k = rows[b0:b0 + 256]
        later = time[None, :] > time[k, None]
        comp += (c2[k] * np.where(later, wl[None, :], LD(0)).sum(axis=1)).sum()
        for r in range(R):
            gt = later & (eta[k, r][:, None] > eta[None, :, r])
            eq = later & (eta[k, r][:, None] == eta[None, :, r])
            conc[r] += (c2[k] * np.where(gt, wl[None, :], LD(0)).sum(axis=1)).sum()
            tied[r] += (c2[k] * np.where(eq, wl[None, :], LD(0)).sum(axis=1)).sum()
    out["uno_concordant"], out["uno_tied"], out["uno_comparable"] = conc, tied, comp
    out["uno_c"] = (conc + tied / 2) / comp if comp > 0 else np.full(R, LD(np.nan))
    return out


def mean_auc_reference(auc, drop, times):
    """mean_auc (R,) in longdouble from the reference's auc (T, R) and the implementation's km_drop (T,), as data."""
    d = _ld(drop)
    used = d > 0
    if not used.any():
        return np.full(auc.shape[1], LD(np.nan))
    return (auc[used] * d[used, None]).sum(axis=0) / d[used].sum()


def auc_reference(eta, y, w):
    """{"greater", "equal", "auc": (R,), "pos_weight", "neg_weight"} of the ROC AUC in longdouble."""
    eta = _ld(eta)
    n = eta.shape[0]
    wl = np.ones(n, dtype=LD) if w is None else _ld(w).reshape(-1)
    cls = np.where(np.asarray(y, dtype=np.float64).reshape(-1) > 0.5, 0.0, 1.0)
    g, e, pos, neg = pair_sums(eta, cls, wl, wl, 0.0)
    auc = (g + e / 2) / (pos * neg) if pos * neg > 0 else np.full(eta.shape[1], LD(np.nan))
    return {"greater": g, "equal": e, "auc": auc, "pos_weight": pos, "neg_weight": neg}


SUMS = ("greater", "equal", "cases", "controls", "uno_concordant", "uno_tied", "uno_comparable")


def _cmp(got, ref, rel, what, exact):
    got, ref = _ld(got), _ld(ref)
    if got.size == ref.size and got.ndim < ref.ndim:  # (the estimators return one model's column as a vector or a float)
        got = got.reshape(ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", got, ref)
    err = np.where(nan, LD(0), np.abs(got - ref))
    bnd = np.where(nan, LD(0), LD(0) if exact else rel * np.abs(ref))
    print("%s: largest err %.3e, its bound %.3e%s" % (what, float(err.max(initial=0)), float(bnd.max(initial=0)),
                                                    " (exact)" if exact else ""))
    assert (err <= bnd).all(), (what, float((err - bnd).max()), got, ref)


def check_cox_auc(got, ref, n, exact, what=""):
    """Every entry of a result dict of cox_auc_device / _cox_auc_host / auc_survival against the reference: the sums
    EQUAL it (exact) or lie within rel_bound, the quotients within their propagated bounds, km_drop within km_bound,
    mean_auc against the reference's auc weighted by the result's own km_drop.  Prints error against bound."""
    T = int(np.size(got["km_drop"]))
    rel = rel_bound(n, T)
    for k in SUMS:
        _cmp(got[k], ref[k], rel, what + " " + k, exact)
    _cmp(got["auc"], ref["auc"], auc_rel(n, T), what + " auc", False)
    _cmp(got["uno_c"], ref["uno_c"], uno_rel(n), what + " uno_c", False)
    err = np.abs(_ld(got["km_drop"]) - ref["km_drop"])
    assert (err <= km_bound(ref["K"], n)).all(), (what, "km_drop", float(err.max(initial=0)))
    assert (np.asarray(got["km_drop"]) >= 0).all()
    mean = mean_auc_reference(ref["auc"], got["km_drop"], None)
    _cmp(np.reshape(got["mean_auc"], -1), mean, auc_rel(n, T) + LD(2 * T + 3) * U, what + " mean_auc", False)


def check_auc(got, ref, n, exact, what=""):
    rel = rel_bound(n, 1)
    for k in ("greater", "equal", "pos_weight", "neg_weight"):
        _cmp(got[k], ref[k], rel, what + " " + k, exact)
    _cmp(got["auc"], ref["auc"], auc_rel(n, 1), what + " auc", False)


def brute_force(eta, time, status, w, a, t, tau):
    """greater, equal at t and Uno's three sums for ONE model by a double loop over the pairs, longdouble."""
    n = len(time)
    g = e = c = d = comp = LD(0)
    for i in range(n):
        for l in range(n):
            if time[i] <= t < time[l]:
                g += w[i] * a[i] * w[l] * (eta[i] > eta[l])
                e += w[i] * a[i] * w[l] * (eta[i] == eta[l])
            if status[i] == 1 and time[i] < time[l] and (tau is None or time[i] < tau):
                v = w[i] * a[i] * a[i] * w[l]
                comp += v
                c += v * (eta[i] > eta[l])
                d += v * (eta[i] == eta[l])
    return g, e, c, d, comp


def self_check(seed=0):
    rng = np.random.default_rng(seed)
    for n, tau in ((1, None), (2, None), (23, 1.0), (40, None)):
        eta = _ld(rng.integers(-4, 5, (n, 2)) / 4.0)
        time = np.round(rng.exponential(1.0, n), 1) + 0.1
        status = (rng.uniform(size=n) < 0.6).astype(np.float64)
        w = _ld(rng.integers(0, 9, n) / 4.0)
        a = _ld(status * rng.uniform(1.0, 2.0, n))
        times = np.array([0.05, np.median(time), time.max()])
        ref = cox_auc_reference(eta, times, time, status, w, a, tau)
        for j, t in enumerate(times):
            for r in range(2):
                g, e, c, d, comp = brute_force(eta[:, r], time, status, w, a, t, tau)
                tol = LD(8 * n + 8) * LD(2.0) ** -63
                assert abs(ref["greater"][j, r] - g) <= tol * max(g, 1) and abs(ref["equal"][j, r] - e) <= tol * max(e, 1)
                assert abs(ref["uno_concordant"][r] - c) <= tol * max(c, 1) and abs(ref["uno_tied"][r] - d) <= tol * max(d, 1)
                assert abs(ref["uno_comparable"] - comp) <= tol * max(comp, 1)
        order, first = coxevalref.time_order(time)  # Uno's pair set is Harrell's: unit weights count the same pairs
        one = cox_auc_reference(eta, None, time, status, None, status, None)
        cnt = coxevalref.pair_counts(eta, time, status)
        assert int(one["uno_comparable"]) == cnt["comparable"]
        assert np.array_equal(one["uno_concordant"].astype(np.int64), cnt["concordant"])
        assert np.array_equal(one["uno_tied"].astype(np.int64), cnt["tied_risk"])
    return True
