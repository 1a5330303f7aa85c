"""CPU: the NumPy route of bess_base.fit_survival_bands / predict_survival_bands against the longdouble reference of
tests/coxbandref.py (explicit risk sets, derived bounds), the delta-method gradient by finite differences, the normal
quantile, and every argument error that needs no device."""
import numpy as np
import pytest

import coxbandref
import evalref
from bess_amd import capi, linear

LD = np.longdouble
P = 12
_CACHE = {}


def test_the_reference_agrees_with_the_running_sum_decomposition_and_the_quadratic_form():
    assert coxbandref.self_check()


def _problem(n=157, m=4, tied=False, seed=5):
    rng = np.random.default_rng(seed + m)
    X = rng.standard_normal((n, P))
    cols = np.sort(rng.choice(P, m, replace=False))
    beta = np.zeros(P)
    beta[cols] = rng.normal(0.0, 0.6, m)
    time = rng.exponential(1.0, n)
    if tied:
        time = np.ceil(time * 6.0) / 6.0
    status = (rng.uniform(size=n) < 0.65).astype(np.float64)
    return X, cols, beta, time, status


def _weights(n, kind):
    if kind == "none":
        return None
    w = np.random.default_rng(5).integers(1, 17, n) / 8.0
    if kind == "zeros":
        w[::3] = 0.0
    return w


def _grid(time):
    """before the first time, at, between and after the times, unsorted, with repeats"""
    s = np.sort(time)
    return np.array([s[40], s[0] - 0.5, 0.5 * (s[10] + s[11]), s[-1] + 1.0, s[40], s[0], s[-1], s[3], 0.5 * (s[90] + s[91])])


def _estimator(X, beta):
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = X.shape[1], beta.copy(), 0.0
    return est


def _fitted(key, tied, wk, ties, m=4):
    k = (key, tied, wk, ties, m)
    if k not in _CACHE:
        X, cols, beta, time, status = _problem(m=m, tied=tied)
        w = _weights(X.shape[0], wk)
        est = _estimator(X, beta)
        assert est.fit_survival_bands(X, np.column_stack([time, status]), _grid(time), weight=w, ties=ties) is est
        ref = coxbandref.hazard_var_reference(X, cols, beta[cols], time, status, w, ties, _grid(time))
        _CACHE[k] = (X, cols, beta, time, status, w, est, ref)
    return _CACHE[k]


@pytest.mark.parametrize("ties", ["order", "breslow"])
@pytest.mark.parametrize("wk", ["none", "random", "zeros"])
@pytest.mark.parametrize("tied", [False, True])
def test_fit_survival_bands_against_the_explicit_risk_set_reference(tied, wk, ties):
    X, cols, beta, time, status, w, est, ref = _fitted("fit", tied, wk, ties)
    got = {"cumhaz": est.band_cumhaz_, "var0": est.band_var0_, "drift": est.band_drift_}
    coxbandref.check_hazard_var(got, ref, "numpy route tied=%s w=%s %s" % (tied, wk, ties))
    assert np.array_equal(est.band_times_, _grid(time)) and est.band_factor_.shape == (4, 4)
    assert est.band_cumhaz_[1] == 0.0 and est.band_var0_[1] == 0.0 and (est.band_drift_[1] == 0.0).all()
    assert est.band_cumhaz_[0] == est.band_cumhaz_[4]  # (a repeated grid time)
    if tied:  # a grid time at a tied time takes the whole tie group under both rules
        at = np.sort(time)[40]
        assert abs(float(ref["cumhaz"][0]) - float(ref["cumhaz"][4])) == 0.0 and (time == at).sum() > 1


@pytest.mark.parametrize("kind,conf", [("survival", "plain"), ("survival", "log"), ("survival", "log-log"),
                                       ("cumhaz", "plain"), ("cumhaz", "log")])
@pytest.mark.parametrize("ties", ["order", "breslow"])
def test_predict_survival_bands_every_kind_and_conf_type(kind, conf, ties):
    for tied, wk in ((False, "none"), (True, "random"), (True, "zeros")):
        X, cols, beta, time, status, w, est, href = _fitted("fit", tied, wk, ties)
        Xn = np.random.default_rng(9).standard_normal((33, P))  # (any rows: not the training rows)
        got = est.predict_survival_bands(Xn, kind=kind, conf_type=conf, level=0.9, what=coxbandref.WHAT)
        assert list(got) == list(coxbandref.WHAT) and all(v.shape == (33, 9) for v in got.values())
        zc = capi.normal_quantile(0.9)
        # (1) the formulas alone: the estimator's own cumhaz / var0 / drift / factor as data
        ref = coxbandref.band_reference(Xn, cols, beta[cols], est.band_cumhaz_, est.band_var0_, est.band_drift_,
                                        est.band_factor_, kind, conf, zc, coxbandref.host_depths(4))
        coxbandref.check_bands(got, ref, coxbandref.WHAT, "%s %s %s, inputs as data" % (kind, conf, ties))
        # (2) end to end: the explicit-risk-set values with the bounds of what the estimator holds in their place
        ref = coxbandref.band_reference(Xn, cols, beta[cols], href["cumhaz"], href["var0"], href["drift"],
                                        est.band_factor_, kind, conf, zc, coxbandref.host_depths(4),
                                        in_bounds=(href["cumhaz_bound"], href["var0_bound"], href["drift_bound"]))
        coxbandref.check_bands(got, ref, coxbandref.WHAT, "%s %s %s, end to end" % (kind, conf, ties))
        # where cumhaz = 0 the bounds equal the estimate and se is 0
        z = est.band_cumhaz_ == 0.0
        assert z.any()
        assert (got["estimate"][:, z] == (1.0 if kind == "survival" else 0.0)).all() and (got["se"][:, z] == 0.0).all()
        assert np.array_equal(got["lower"][:, z], got["estimate"][:, z])
        assert np.array_equal(got["upper"][:, z], got["estimate"][:, z])
        assert (got["lower"] <= got["estimate"]).all() and (got["estimate"] <= got["upper"]).all()
        assert (got["se"] >= 0.0).all() and (got["lower"] >= 0.0).all()
        if kind == "survival":
            assert (got["upper"] <= 1.0).all()
        # estimate is predict_survival's for the same baseline values
        est.baseline_times_, est.baseline_cumhaz_ = np.arange(9.0), est.band_cumhaz_
        assert np.array_equal(got["estimate"], est.predict_survival(Xn, times=np.arange(9.0), kind=kind))
        some = est.predict_survival_bands(Xn, kind=kind, conf_type=conf, level=0.9, what=("upper", "se"))
        assert list(some) == ["se", "upper"] and np.array_equal(some["upper"], got["upper"])


def test_without_a_support_the_variance_is_nelson_aalens():
    X, cols, beta, time, status = _problem(m=0)
    w = _weights(X.shape[0], "random")
    grid = _grid(time)
    est = _estimator(X, np.zeros(P))
    est.fit_survival_bands(X, np.column_stack([time, status]), grid, weight=w, ties="breslow")
    assert est.band_drift_.shape == (9, 0) and est.band_factor_.shape == (0, 0)
    tl, wl, dl = time.astype(LD), w.astype(LD), status.astype(LD)
    Y = np.array([(tl >= t).sum() for t in tl], dtype=LD)  # the size of each row's risk set
    na = np.array([(wl * dl / Y ** 2)[time <= g].sum() for g in grid], dtype=LD)
    ch = np.array([(wl * dl / Y)[time <= g].sum() for g in grid], dtype=LD)
    tol = LD(2 * X.shape[0] + 8) * evalref.U
    assert (np.abs(est.band_var0_.astype(LD) - na) <= tol * na).all()
    assert (np.abs(est.band_cumhaz_.astype(LD) - ch) <= tol * ch).all()
    got = est.predict_survival_bands(X[:5], kind="cumhaz", conf_type="plain", what=("estimate", "se"))
    assert (np.abs(got["se"].astype(LD) - np.sqrt(na)[None, :]) <= LD(4) * evalref.U * np.sqrt(na)[None, :] + tol * np.sqrt(na)).all()
    assert np.array_equal(got["estimate"], np.broadcast_to(est.band_cumhaz_, (5, 9)))


def test_the_delta_method_term_is_the_gradient_of_the_cumulative_hazard_in_beta():
    """-e_x (drift - z cumhaz) against the central finite difference of the reference's Lambda(tau | x) in beta, in
    longdouble.  Tolerance, stated below: the truncation term of a central difference, h^2 / 6 times the largest third
    derivative -- every derivative of Lambda = cumhaz(beta) exp(z . beta) in beta_c brings a factor of at most D = 2 max|x_c|
    (a difference of a covariate and a risk-set mean, or z_c itself) and the product rule at most 16 such terms: 16 D^3
    Lambda -- plus the rounding term of the longdouble reference, 2^-60 Lambda / h."""
    X, cols, beta, time, status = _problem(m=3, tied=True)
    w = _weights(X.shape[0], "random")
    grid = _grid(time)[[0, 2, 3, 8]]
    b = beta[cols]
    ref = coxbandref.hazard_var_reference(X, cols, b, time, status, w, "breslow", grid)
    xs = np.random.default_rng(3).standard_normal((6, P))
    z = xs[:, cols].astype(LD)
    e = np.exp(z @ b.astype(LD))
    grad = -e[:, None, None] * (ref["drift"][None, :, :] - z[:, None, :] * ref["cumhaz"][None, :, None])

    def lam(bb):
        r = coxbandref.hazard_var_reference(X, cols, bb, time, status, w, "breslow", grid)
        return r["cumhaz"][None, :] * np.exp(z @ bb.astype(LD))[:, None]

    h = 2.0 ** -17  # (the reference takes fp64 coefficients: beta +- h is exact)
    D = LD(2.0 * max(np.abs(X[:, cols]).max(), np.abs(xs[:, cols]).max()))
    for c in range(3):
        up, dn = b.copy(), b.copy()
        up[c] += h
        dn[c] -= h
        assert up[c] - b[c] == h and b[c] - dn[c] == h
        fd = (lam(up) - lam(dn)) / LD(2 * h)
        tol = (LD(h) ** 2 / 6 * 16 * D ** 3 + LD(2.0) ** -60 / LD(h)) * np.maximum(lam(up), lam(dn))
        err = np.abs(fd - grad[:, :, c])
        print("column %d: largest |fd - grad| %.3e against tol %.3e, |grad| up to %.3e" % (
            c, float(err.max()), float(tol[np.unravel_index(int(np.argmax(err)), err.shape)]), float(np.abs(grad[:, :, c]).max())))
        assert (err <= tol).all() and float(np.abs(grad[:, :, c]).max()) > 1e3 * float(tol.max())


def test_normal_quantile():
    q = capi.normal_quantile(0.95)
    assert abs(q - 1.959963984540054) <= np.spacing(1.959963984540054)
    levels = [1e-6, 0.01, 0.5, 0.8, 0.9, 0.95, 0.99, 0.999, 1 - 1e-9]
    qs = [capi.normal_quantile(v) for v in levels]
    assert all(a < b for a, b in zip(qs, qs[1:])) and qs[0] > 0
    assert abs(capi.normal_quantile(0.6826894921370859) - 1.0) < 1e-14
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            capi.normal_quantile(bad)


def test_argument_errors_need_no_device():
    X, cols, beta, time, status, w, est, _ = _fitted("fit", False, "none", "breslow")
    y = np.column_stack([time, status])
    with pytest.raises(ValueError, match="kind"):
        est.predict_survival_bands(X, kind="hazard")
    with pytest.raises(ValueError, match="conf_type"):
        est.predict_survival_bands(X, conf_type="arcsine")
    with pytest.raises(ValueError, match="log-log"):
        est.predict_survival_bands(X, kind="cumhaz", conf_type="log-log")
    with pytest.raises(ValueError, match="what"):
        est.predict_survival_bands(X, what=("estimate", "median"))
    with pytest.raises(ValueError, match="what"):
        est.predict_survival_bands(X, what=())
    with pytest.raises(ValueError, match="level"):
        est.predict_survival_bands(X, level=1.0)
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be %d" % P):
        est.predict_survival_bands(X[:, :P - 1])
    with pytest.raises(ValueError, match="ties"):
        est.fit_survival_bands(X, y, [1.0], ties="efron")
    with pytest.raises(ValueError, match="NAN"):
        est.fit_survival_bands(X, y, [1.0, np.nan])
    with pytest.raises(ValueError, match="empty"):
        est.fit_survival_bands(X, y, [])
    with pytest.raises(ValueError, match="1-D"):
        est.fit_survival_bands(X, y, [[1.0]])
    with pytest.raises(ValueError, match="non-negative"):
        est.fit_survival_bands(X, y, [1.0], weight=-np.ones(X.shape[0]))
    fresh = _estimator(X, beta)
    with pytest.raises(ValueError, match="fit_survival_bands"):
        fresh.predict_survival_bands(X)
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = P, beta, 0.0
    with pytest.raises(ValueError, match="Cox"):
        lm.fit_survival_bands(X, y, [1.0])
    with pytest.raises(ValueError, match="Cox"):
        lm.predict_survival_bands(X)
    dup = X.copy()
    dup[:, cols[1]] = dup[:, cols[0]]  # two identical support columns: the information is singular
    with pytest.raises(ValueError, match="positive definite"):
        _estimator(dup, beta).fit_survival_bands(dup, y, [1.0])
    moved = _estimator(X, beta)
    moved.__dict__.update({k: v for k, v in est.__dict__.items() if k.startswith("band_")})
    moved.beta[cols[0]] = 0.0
    with pytest.raises(ValueError, match="support has changed"):
        moved.predict_survival_bands(X)


def test_the_capi_checks_of_the_band_inputs_come_before_any_device_work():
    class Fake:  # a device array by its interface alone: nothing dereferences the pointer before the checks are through
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (4096, False), "version": 2}

    x = Fake((10, 5))
    cols, beta = [1, 3], [0.5, -0.25]
    H, V0, D, R = np.array([0.0, 0.5]), np.array([0.0, 0.1]), np.zeros((2, 2)), np.eye(2)
    call = lambda **kw: capi.cox_survival_band_device(x, cols, beta, kw.pop("H", H), kw.pop("V0", V0), kw.pop("D", D),
                                                      kw.pop("R", R), **kw)
    for kw, msg in (({"kind": "hazard"}, "kind"), ({"conf_type": "x"}, "conf_type"),
                    ({"kind": "cumhaz", "conf_type": "log-log"}, "log-log"), ({"what": ("lower", "mean")}, "what"),
                    ({"what": ()}, "what"), ({"level": 0.0}, "level"), ({"H": np.array([0.0, -1.0])}, "cumhaz"),
                    ({"H": np.array([0.0, np.inf])}, "cumhaz"), ({"V0": np.array([np.nan, 0.1])}, "var0"),
                    ({"V0": np.array([0.1])}, "same size"), ({"D": np.zeros((2, 3))}, "drift"),
                    ({"D": np.full((2, 2), np.inf)}, "drift"), ({"R": np.eye(3)}, "factor"),
                    ({"R": np.full((2, 2), np.nan)}, "factor"), ({"H": np.array([]), "V0": np.array([])}, "empty"),
                    ({"out": np.zeros((3, 10, 2))}, "device array"), ({"out": Fake((3, 10, 3))}, "shape"),
                    ({"out": Fake((3, 10, 2), "<f4")}, "float64")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="1-D"):
        capi.cox_survival_band_device(x, cols, np.zeros((2, 2)), H, V0, D, R)
    t, s = np.arange(10.0), np.ones(10)
    for kw, msg in (({"times": [1.0, np.nan]}, "NAN"), ({"times": []}, "empty"), ({"times": [[1.0]]}, "1-D"),
                    ({"times": [1.0], "ties": "efron"}, "ties"), ({"times": [1.0], "weight": -s}, "non-negative")):
        with pytest.raises(ValueError, match=msg):
            capi.cox_baseline_variance_device(x, cols, beta, t, s, **kw)
    nd, tc = capi.cox_band_workspace(1000, 5, 10)
    assert tc == 16 and nd >= 1000 + 2 * 10 + 10 * 16
    assert capi.cox_band_workspace(1000, 5, 10, row_stride=1, col_stride=1000)[1] == 8
    assert capi.cox_band_workspace(1000, 5, 10, dtype=np.float32, row_stride=1, col_stride=1000)[1] == 4
    with pytest.raises(capi.BessxError) as e:
        capi.cox_band_workspace(1000, 1024, 10)
    assert e.value.code == 3  # BESSX_ERR_UNSUPPORTED: m + 1 > 1024
