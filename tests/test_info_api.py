"""Coefficient tables without a GPU: bess_base.inference on a NumPy X (bess_base._information_host, fp64 NumPy) and
capi.wald_table against the longdouble reference and the derived bounds of tests/inforef.py; the data-dependent failure
modes of wald_table; and the argument checks of bessx_info_device, which are made before any device call."""
import ctypes

import numpy as np
import pytest

import inforef
from bess_amd import capi, linear

LD = np.longdouble
LINKS = ["identity", "logistic", "poisson"]
N, P = 300, 40


def _est(link, beta, coef0):
    est = {"identity": linear.PdasLm, "logistic": linear.PdasLogistic, "poisson": linear.PdasPoisson}[link]()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, coef0
    return est


_CASES = {}


def _case(link, weighted):
    """A model on N rows with a support of 6 of P columns, its responses, weights (multiples of 1/8 with zeros), the
    longdouble reference at depth_host = N, and the table of the NumPy route -- computed once and shared."""
    key = (link, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(11 + 3 * LINKS.index(link) + weighted)
        X = rng.standard_normal((N, P))
        cols = np.sort(rng.choice(P, 6, replace=False))
        beta = np.zeros(P)
        beta[cols] = rng.standard_normal(6) * 0.5
        coef0 = 0.3
        eta = X @ beta + coef0
        y = {"identity": eta + rng.standard_normal(N),
             "logistic": (rng.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(float),
             "poisson": rng.poisson(np.exp(eta)).astype(float)}[link]
        w = rng.integers(0, 17, N) / 8.0 if weighted else None
        ref = inforef.information_reference(X, cols, beta[cols], coef0, y, w, link, depth=N)
        table = _est(link, beta, coef0).inference(X, y, weight=w)
        _CASES[key] = dict(X=X, cols=cols, beta=beta, coef0=coef0, y=y, w=w, ref=ref, table=table)
    return _CASES[key]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("link", LINKS)
def test_numpy_route_is_within_the_bounds_of_the_reference(link, weighted):
    cs = _case(link, weighted)
    ref, tb = cs["ref"], cs["table"]
    got = linear.bess_base._information_host(link, cs["X"][:, cs["cols"]], cs["beta"][cs["cols"]], cs["coef0"], cs["y"],
                                             np.ones(N) if cs["w"] is None else cs["w"])
    inforef.check_information(got, ref, "%s weighted=%s" % (link, weighted))
    assert np.array_equal(got["info"], got["info"].T)
    assert abs(LD(got["loss"]) - ref["loss"]["loss"][0]) <= ref["loss"]["bound"][0]
    assert got["sum_w"] == float(ref["loss"]["sum_w"])
    se, cov, rel, cond = inforef.se_reference(ref)
    print("cond(S*) %.3e, se bound %.3e, se err %.3e" % (cond, float(rel), float(np.abs(tb["se"] - se).max() / se.min())))
    assert rel < 1e-3
    assert tb["positive_definite"] and np.array_equal(tb["cols"], cs["cols"])
    assert (np.abs(tb["se"].astype(LD) - se) <= rel * se).all()
    assert np.array_equal(tb["coef"], np.concatenate([[cs["coef0"]], cs["beta"][cs["cols"]]]))
    assert np.allclose(tb["z"], tb["coef"] / tb["se"], rtol=1e-15)
    # the two-sided normal tail, against its continued definition at a known point: P(|Z| > 1.959964) = 0.05
    assert abs(capi.wald_table(np.eye(1), [0.0], [1.959963984540054], "logistic", 0.0, 10.0)["p_value"][0] - 0.05) < 1e-12
    assert tb["dispersion"] == (got["loss"] / (got["sum_w"] - 7) if link == "identity" else 1.0)
    assert abs(tb["cond"] - cond) <= 1e-6 * cond


def test_unpenalised_lm_fit_has_zero_score_and_the_textbook_covariance():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, P))
    cols = np.array([3, 17, 29])
    y = X[:, cols] @ np.array([1.0, -2.0, 0.5]) + 0.7 + rng.standard_normal(N)
    Z = np.column_stack([np.ones(N), X[:, cols]])
    sol = np.linalg.lstsq(Z, y, rcond=None)[0]
    beta = np.zeros(P)
    beta[cols] = sol[1:]
    tb = _est("identity", beta, sol[0]).inference(X, y)
    ref = inforef.information_reference(X, cols, sol[1:], sol[0], y, None, "identity", depth=N)
    # the least-squares solution is the optimum up to its own rounding: the exact score at it is not 0 but small; what
    # the table reports is within the score bound of that exact value, and the exact value is itself below the bound of
    # a solve that is backward stable (|U*| <= gamma_{N + 8} sum_i |z_ij| (|y_i| + |z_i| |coef|))
    assert (np.abs(tb["score"].astype(LD) - ref["score"]) <= ref["score_bound"]).all()
    optimum = inforef.gamma(N + 8) * (np.abs(Z).T @ (np.abs(y) + np.abs(Z) @ np.abs(sol)))
    assert (np.abs(tb["score"]) <= ref["score_bound"].astype(np.float64) + optimum).all(), tb["score"]
    se, cov, rel, _ = inforef.se_reference(ref)
    assert (np.abs(tb["cov"].astype(LD) - cov) <= 2 * rel * np.sqrt(np.outer(np.diag(cov), np.diag(cov)))).all()
    sigma2 = ref["loss"]["loss"][0] / LD(N - 4)
    assert abs(LD(tb["dispersion"]) - sigma2) <= ref["loss"]["bound"][0] / LD(N - 4) + 4 * inforef.U * sigma2


def test_duplicated_support_column_is_not_positive_definite():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((N, 5))
    X[:, 3] = X[:, 1]
    beta = np.array([0.0, 0.5, 0.0, 0.5, -1.0])
    y = X @ beta + rng.standard_normal(N)
    tb = _est("identity", beta, 0.1).inference(X, y)
    assert tb["positive_definite"] is False
    for k in ("se", "z", "p_value", "cov"):
        assert np.isnan(tb[k]).all(), k
    assert np.isfinite(tb["score"]).all() and np.array_equal(tb["cols"], [1, 3, 4])


def test_separated_logistic_sample_is_not_positive_definite():
    # a fit that ran off along the separating direction: |eta| > 745, so every p (1 - p) underflows to 0
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N, 5))
    X[:, 2] = np.where(X[:, 2] >= 0, X[:, 2] + 1.0, X[:, 2] - 1.0)
    y = (X[:, 2] > 0).astype(float)
    beta = np.array([0.0, 0.0, 800.0, 0.0, 0.0])
    tb = _est("logistic", beta, 0.0).inference(X, y)
    assert tb["positive_definite"] is False and np.isnan(tb["se"]).all() and np.isnan(tb["cov"]).all()
    assert tb["dispersion"] == 1.0 and np.isfinite(tb["score"]).all()


def test_dispersion_is_nan_without_residual_degrees_of_freedom():
    rng = np.random.default_rng(8)
    X = rng.standard_normal((3, 4))
    beta = np.array([0.5, 0.0, -0.5, 0.0])
    tb = _est("identity", beta, 0.0).inference(X, rng.standard_normal(3))  # sum_w = 3 = m + 1
    assert np.isnan(tb["dispersion"]) and tb["dof"] == 0.0 and np.isnan(tb["se"]).all()
    tb = capi.wald_table(np.eye(2), np.zeros(2), np.ones(2), "identity", 1.0, 1.5)
    assert np.isnan(tb["dispersion"]) and tb["dof"] == -0.5
    assert capi.wald_table(np.eye(2), np.zeros(2), np.ones(2), "poisson", 1.0, 1.5)["dispersion"] == 1.0


def test_cox_returns_none_and_a_two_dimensional_beta_raises():
    X = np.zeros((10, 4))
    cox = linear.PdasCox()
    cox.p, cox.beta, cox.coef0 = 4, np.array([1.0, 0, 0, 0]), 0.0
    assert cox.inference(X, np.zeros((10, 2))) is None
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = 4, np.ones((4, 2)), np.zeros(2)
    with pytest.raises(ValueError, match="not supported"):
        lm.inference(X, np.zeros(10))


def test_bad_shapes_raise_the_existing_messages():
    est = _est("identity", np.array([1.0, 0.0, 2.0]), 0.0)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        est.inference(np.zeros((10, 4)), np.zeros(10))
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to y.size"):
        est.inference(np.zeros((10, 3)), np.zeros(9))
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to weight.size"):
        est.inference(np.zeros((10, 3)), np.zeros(10), weight=np.ones(11))
    with pytest.raises(ValueError):
        capi.wald_table(np.eye(3), np.zeros(2), np.zeros(3), "identity", 1.0, 10.0)
    with pytest.raises(ValueError, match="link must be one of"):
        capi.wald_table(np.eye(1), np.zeros(1), np.zeros(1), "cox", 1.0, 10.0)


def test_row_split_is_a_function_of_n_and_m_alone():
    for n, m in ((1, 0), (127, 15), (4097, 200), (50000, 200), (2 ** 31 - 1, 1023)):
        a = capi.info_workspace(n, m)
        assert a[1:] == capi.info_workspace(n, m, link="logistic", weighted=True, dtype=np.float32, row_stride=1,
                                            col_stride=n)[1:]
        rps, slabs = a[1], a[2]
        assert rps % 16 == 0 and (slabs - 1) * rps < n <= slabs * rps and slabs <= 256
    # the partials do not grow with n once the slab count is capped
    M, T = 201, 13 * 16 // 2
    assert capi.info_workspace(10 ** 8, 200)[0] - 2 * 10 ** 8 <= 256 * T * 256 + 10 ** 8 // 64
    with pytest.raises(capi.BessxError) as e:
        capi.info_workspace(127, 1024)
    assert e.value.code == 3


def _input(n=8, p=4, cols=(1, 2), beta=(0.5, -0.5)):
    a = capi.InfoInput()
    keep = dict(cols=np.asarray(cols, dtype=np.int32), beta=np.asarray(beta, dtype=np.float64), y=np.zeros(n),
                info=np.zeros((len(cols) + 1) ** 2), score=np.zeros(len(cols) + 1))
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 0x1000, 0, p, 1, n, p
    a.cols, a.m, a.beta, a.coef0, a.link = capi._ip(keep["cols"]), len(cols), capi._dp(keep["beta"]), 0.1, 0
    a.y_host, a.y_stride = capi._dp(keep["y"]), 1
    a.info, a.info_ld, a.score = keep["info"].ctypes.data, len(cols) + 1, keep["score"].ctypes.data
    return a, keep


def _call(a):
    loss, sw = ctypes.c_double(0), ctypes.c_double(0)
    rc = capi.lib().bessx_info_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw))
    return rc, capi.last_error()


def test_abi_argument_checks_need_no_gpu():
    lib = capi.lib()
    assert lib.bessx_info_device(None, None, None) == 1 and "null" in capi.last_error()
    checks = [
        (lambda a: setattr(a, "x_dtype", 7), 1, "dtype must be BESSX_F64 or BESSX_F32"),
        (lambda a: setattr(a, "x_row_stride", -1), 1, "strides must be non-negative"),
        (lambda a: setattr(a, "y_stride", -1), 1, "strides must be non-negative"),
        (lambda a: setattr(a, "link", 3), 1, "unknown link"),
        (lambda a: setattr(a, "n", 0), 1, "empty matrix"),
        (lambda a: setattr(a, "m", 5), 1, "m must lie in [0, p]"),
        (lambda a: setattr(a, "beta", None), 1, "null argument (beta)"),
        (lambda a: setattr(a, "coef0", float("inf")), 1, "coef0 must be finite"),
        (lambda a: setattr(a, "y_host", None), 1, "give y as a host pointer or as a device view"),
        (lambda a: setattr(a, "y_dev", 0x2000), 1, "give y as a host pointer or as a device view"),
        (lambda a: (setattr(a, "weight_dev", 0x2000), setattr(a, "weight_dtype", 5)), 1, "weight: dtype must be"),
        (lambda a: setattr(a, "info_ld", 2), 1, "info_ld must be at least m + 1"),
        (lambda a: setattr(a, "info", None), 1, "null argument"),
    ]
    for change, code, text in checks:
        a, keep = _input()
        change(a)
        rc, msg = _call(a)
        assert rc == code and text in msg, (rc, msg, text)
    for cols, text in (((2, 1), "cols must be ascending and distinct"), ((1, 1), "cols must be ascending and distinct"),
                       ((1, 4), "column number out of range")):
        a, keep = _input(cols=cols)
        rc, msg = _call(a)
        assert rc == 1 and text in msg, (rc, msg)
    a, keep = _input(beta=(0.5, float("nan")))
    rc, msg = _call(a)
    assert rc == 1 and "beta must be finite" in msg
    # m + 1 = 1025: unsupported, said before the device is touched (the x pointer above is not a device pointer)
    a, keep = _input(p=2000, cols=tuple(range(1024)), beta=(0.0,) * 1024)
    rc, msg = _call(a)
    assert rc == 3 and "m + 1 must be at most 1024" in msg
    assert lib.bessx_op_info_bench(None, 0, 1, 1, 1, 1, None, 0, 1, None, None) == 1


def test_python_checks_are_made_before_any_device_call():
    class Fake:  # a device array by its interface only: any device call on it would fail
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3,
                                             "strides": None}
    x = Fake((10, 4))
    with pytest.raises(ValueError, match="cols must be ascending and distinct"):
        capi.information_device(x, [2, 1], [0.1, 0.2], 0.0, np.zeros(10))
    with pytest.raises(ValueError, match="one model per call"):
        capi.information_device(x, [1, 2], np.zeros((2, 2)), 0.0, np.zeros(10))
    with pytest.raises(ValueError, match="beta and coef0 must be finite"):
        capi.information_device(x, [1, 2], [0.1, np.nan], 0.0, np.zeros(10))
    with pytest.raises(ValueError, match="link must be one of"):
        capi.information_device(x, [1], [0.1], 0.0, np.zeros(10), link="cox")
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to y.shape\(0\)"):
        capi.information_device(x, [1], [0.1], 0.0, np.zeros(9))
    est = _est("identity", np.array([1.0, 0.0, 2.0]), 0.0)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        est.inference(x, np.zeros(10))
