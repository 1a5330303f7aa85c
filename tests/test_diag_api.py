"""Row diagnostics without a GPU: bess_base.diagnostics on a NumPy X (bess_base._diagnostics_host, fp64 NumPy) against
the longdouble reference and the derived bounds of tests/diagref.py; capi.info_factor; the data-dependent failure
mode; and the argument checks of bessx_diag_device, which are made before any device call."""
import ctypes
import os

import numpy as np
import pytest

import diagref
import inforef
from bess_amd import capi, linear

LD = np.longdouble
LINKS = ["identity", "logistic", "poisson"]
N, P = 300, 40
NEW = ["bessx_diag_device", "bessx_diag_workspace", "bessx_op_diag_bench"]


def _est(link, beta, coef0):
    est = {"identity": linear.PdasLm, "logistic": linear.PdasLogistic, "poisson": linear.PdasPoisson}[link]()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, coef0
    return est


_CASES = {}


def _case(link, weighted):
    """A model on N rows with a support of 6 of P columns, responses, weights (multiples of 1/8 with zeros), what the
    NumPy route returns, the factor it used and the longdouble reference for that factor -- computed once, shared."""
    key = (link, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(31 + 3 * LINKS.index(link) + weighted)
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
        got = _est(link, beta, coef0).diagnostics(X, y, weight=w)
        info = linear.bess_base._information_host(link, X[:, cols], beta[cols], coef0, y, np.ones(N) if w is None else w)
        R, pd = capi.info_factor(info["info"])
        assert pd
        iref = inforef.information_reference(X, cols, beta[cols], coef0, y, w, link, depth=N)
        ref = diagref.diagnostics_reference(X, cols, beta[cols], coef0, y, w, link, R, got["dispersion"],
                                            diagref.sum_depth(7, host=True))
        _CASES[key] = dict(X=X, cols=cols, beta=beta, coef0=coef0, y=y, w=w, got=got, R=R, info=info, iref=iref, ref=ref)
    return _CASES[key]


def test_symbols_are_exported_declared_and_listed():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bessx.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and ("int %s(" % name) in header, name
    assert "bessx_diag_input;" in header and capi.DIAG_KINDS == diagref.KINDS
    for bit, kind in enumerate(capi.DIAG_KINDS):
        assert "BESSX_DIAG_%s = %d" % (kind.upper(), 1 << bit) in header


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("link", LINKS)
def test_numpy_route_is_within_the_bounds_of_the_reference(link, weighted):
    cs = _case(link, weighted)
    got, ref = cs["got"], cs["ref"]
    assert got["positive_definite"] is True and np.array_equal(got["cols"], cs["cols"])
    assert list(got)[:7] == list(capi.DIAG_KINDS)
    diagref.check_diagnostics(got, ref, "%s weighted=%s" % (link, weighted))
    # the trace identity: sum_i h_i = trace(R I R^T) = M up to the error of the factor, which comes from the same rows.
    # With S* = D I* D, the factor inverts a matrix within eps = M r + 8 M^2 u of S* in the 2-norm (inforef step 5), so
    # |trace(S_hat^-1 (S* - S_hat))| <= M ||S_hat^-1|| eps <= 2 M cond(S*) eps <= 2 M rel, rel = se_reference's figure;
    # likewise z^T (C_hat - C*) z <= 2 rel z^T C* z, and h* <= 1 for the exact inverse.
    _, _, rel, cond = inforef.se_reference(cs["iref"])
    M = 7
    h = got["leverage"].astype(LD)
    tb = ref["h_sum_bound"] + LD(2 * M) * rel
    print("sum h - M = %.3e against bound %.3e (cond(S*) %.3e); max h %.6f" % (float(h.sum() - M), float(tb), cond,
                                                                              float(h.max())))
    assert abs(h.sum() - LD(M)) <= tb
    assert (h >= 0).all() and (h <= LD(1) + LD(2) * rel + ref["bound"]["leverage"]).all()
    if weighted:
        zero = cs["w"] == 0
        assert zero.any()
        for k in ("leverage", "pearson", "deviance", "std_pearson", "std_deviance", "cooks"):
            assert (got[k][zero] == 0).all(), k
    sub = _est(link, cs["beta"], cs["coef0"]).diagnostics(cs["X"], cs["y"], weight=cs["w"], kinds=["cooks", "response"])
    assert list(sub) == ["response", "cooks", "cols", "dispersion", "positive_definite"]
    assert np.array_equal(sub["cooks"], got["cooks"]) and np.array_equal(sub["response"], got["response"])


def test_a_rows_result_does_not_depend_on_where_the_row_lies():
    cs = _case("poisson", True)
    perm = np.random.default_rng(3).permutation(N)
    R, w = cs["R"], cs["w"]
    a = linear.bess_base._diagnostics_host("poisson", cs["X"][:, cs["cols"]], cs["beta"][cs["cols"]], cs["coef0"], cs["y"],
                                           w, R, 1.0, capi.DIAG_KINDS)
    b = linear.bess_base._diagnostics_host("poisson", cs["X"][perm][:, cs["cols"]], cs["beta"][cs["cols"]], cs["coef0"],
                                           cs["y"][perm], w[perm], R, 1.0, capi.DIAG_KINDS)
    c = linear.bess_base._diagnostics_host("poisson", cs["X"][:17, cs["cols"]], cs["beta"][cs["cols"]], cs["coef0"],
                                           cs["y"][:17], w[:17], R, 1.0, capi.DIAG_KINDS)
    for k in capi.DIAG_KINDS:
        assert np.array_equal(a[k][perm], b[k]) and np.array_equal(a[k][:17], c[k]), k


@pytest.mark.parametrize("link", LINKS)
def test_info_factor_reproduces_the_covariance_of_wald_table(link):
    cs = _case(link, True)
    R, info = cs["R"], cs["info"]
    M = R.shape[0]
    assert np.array_equal(R, np.tril(R)) and (np.diag(R) > 0).all()
    tb = capi.wald_table(info["info"], info["score"], np.zeros(M), link, info["loss"], info["sum_w"])
    C = tb["cov"] / tb["dispersion"]
    # both are the inverse of the same scaled matrix from the same factor: they differ by the backward error of the
    # products and solves, 8 M^2 u in the 2-norm of the scaled matrix (inforef step 5), times its condition number
    tol = 2 * tb["cond"] * 8 * M * M * float(inforef.U) * np.sqrt(np.outer(np.diag(C), np.diag(C)))
    err = np.abs(R.T @ R - C)
    print("%s: R^T R - cov / dispersion: worst %.3e of its bound" % (link, float((err / tol).max())))
    assert (err <= tol).all()
    with pytest.raises(ValueError, match="square"):
        capi.info_factor(np.zeros((2, 3)))


def test_a_singular_information_gives_nan_leverage_kinds_and_finite_residuals():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((N, 5))
    X[:, 3] = X[:, 1]
    beta = np.array([0.0, 0.5, 0.0, 0.5, -1.0])
    y = X @ beta + rng.standard_normal(N)
    R, pd = capi.info_factor(np.ones((3, 3)))
    assert pd is False and np.isnan(R).all() and R.shape == (3, 3)
    assert capi.info_factor(np.diag([1.0, 0.0]))[1] is False and capi.info_factor(np.diag([1.0, np.inf]))[1] is False
    got = _est("identity", beta, 0.1).diagnostics(X, y)
    assert got["positive_definite"] is False and np.array_equal(got["cols"], [1, 3, 4])
    for k in capi.DIAG_LEVERAGE_KINDS:
        assert got[k].shape == (N,) and np.isnan(got[k]).all(), k
    for k in ("response", "pearson", "deviance"):
        assert got[k].shape == (N,) and np.isfinite(got[k]).all(), k
    assert np.array_equal(got["response"], y - (X[:, 1] * 0.5 + X[:, 3] * 0.5 + X[:, 4] * -1.0 + 0.1))
    only = _est("identity", beta, 0.1).diagnostics(X, y, kinds=["leverage"])
    assert np.isnan(only["leverage"]).all() and "response" not in only


def test_cox_returns_none_and_a_two_dimensional_beta_raises():
    X = np.zeros((10, 4))
    cox = linear.PdasCox()
    cox.p, cox.beta, cox.coef0 = 4, np.array([1.0, 0, 0, 0]), 0.0
    assert cox.diagnostics(X, np.zeros((10, 2))) is None
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = 4, np.ones((4, 2)), np.zeros(2)
    with pytest.raises(ValueError, match="not supported"):
        lm.diagnostics(X, np.zeros(10))


def test_bad_shapes_and_kinds_raise():
    est = _est("identity", np.array([1.0, 0.0, 2.0]), 0.0)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        est.diagnostics(np.zeros((10, 4)), np.zeros(10))
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to y.size"):
        est.diagnostics(np.zeros((10, 3)), np.zeros(9))
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to weight.size"):
        est.diagnostics(np.zeros((10, 3)), np.zeros(10), weight=np.ones(11))
    with pytest.raises(ValueError, match="kinds must be taken from"):
        est.diagnostics(np.zeros((10, 3)), np.zeros(10), kinds=["dfbeta"])
    with pytest.raises(ValueError, match="at least one"):
        est.diagnostics(np.zeros((10, 3)), np.zeros(10), kinds=[])


def test_workspace_needs_no_device_and_counts_what_the_kinds_need():
    n, m = 4097, 200
    nv, TI = 4098, 13
    pk = 2 * TI * (TI + 1) * 64
    assert capi.diag_workspace(n, m) == nv + pk  # v and the packed factor: pearson and deviance are requested
    assert capi.diag_workspace(n, m, ["response", "pearson", "deviance"]) == 0
    assert capi.diag_workspace(n, m, ["leverage"]) == nv + pk
    assert capi.diag_workspace(n, m, ["cooks"]) == 2 * nv + pk
    assert capi.diag_workspace(n, m, ["std_deviance", "std_pearson"]) == 3 * nv + pk
    assert capi.diag_workspace(n, m, ["std_deviance", "deviance"]) == nv + pk
    assert capi.diag_workspace(1, 0, ["leverage"]) == 2 + 2 * 2 * 64
    with pytest.raises(capi.BessxError) as e:
        capi.diag_workspace(127, 1024)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    lib = capi.lib()
    nd = ctypes.c_longlong(0)
    assert lib.bessx_diag_workspace(10, 2, 0, ctypes.byref(nd)) == 1 and "kinds" in capi.last_error()
    assert lib.bessx_diag_workspace(10, 2, 128, ctypes.byref(nd)) == 1 and "kinds" in capi.last_error()
    assert lib.bessx_diag_workspace(0, 2, 1, ctypes.byref(nd)) == 1 and lib.bessx_diag_workspace(10, 2, 1, None) == 1


def _input(n=8, p=4, cols=(1, 2), beta=(0.5, -0.5), kinds=0x7f):
    a = capi.DiagInput()
    M = len(cols) + 1
    keep = dict(cols=np.asarray(cols, dtype=np.int32), beta=np.asarray(beta, dtype=np.float64), y=np.zeros(n),
                factor=np.eye(M), out=np.zeros(7 * n))
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 0x1000, 0, p, 1, n, p
    a.cols, a.m, a.beta, a.coef0, a.link = capi._ip(keep["cols"]), len(cols), capi._dp(keep["beta"]), 0.1, 0
    a.y_host, a.y_stride = capi._dp(keep["y"]), 1
    a.factor, a.factor_ld, a.dispersion, a.kinds = capi._dp(keep["factor"]), M, 1.0, kinds
    a.out, a.out_ld, a.out_on_device = keep["out"].ctypes.data, n, 0
    return a, keep


def _call(a):
    rc = capi.lib().bessx_diag_device(ctypes.byref(a))
    return rc, capi.last_error()


def test_abi_argument_checks_need_no_gpu():
    lib = capi.lib()
    assert lib.bessx_diag_device(None) == 1 and "null" in capi.last_error()

    def poke(name, j, k, value):
        def change(a, keep):
            keep[name][j, k] = value
        return change

    checks = [
        (lambda a, keep: setattr(a, "x_dtype", 7), 1, "dtype must be BESSX_F64 or BESSX_F32"),
        (lambda a, keep: setattr(a, "x_row_stride", -1), 1, "strides must be non-negative"),
        (lambda a, keep: setattr(a, "y_stride", -1), 1, "strides must be non-negative"),
        (lambda a, keep: setattr(a, "link", 3), 1, "unknown link"),
        (lambda a, keep: setattr(a, "n", 0), 1, "empty matrix"),
        (lambda a, keep: setattr(a, "m", 5), 1, "m must lie in [0, p]"),
        (lambda a, keep: setattr(a, "beta", None), 1, "null argument (beta)"),
        (lambda a, keep: setattr(a, "coef0", float("inf")), 1, "coef0 must be finite"),
        (lambda a, keep: setattr(a, "y_host", None), 1, "give y as a host pointer or as a device view"),
        (lambda a, keep: setattr(a, "y_dev", 0x2000), 1, "give y as a host pointer or as a device view"),
        (lambda a, keep: (setattr(a, "weight_dev", 0x2000), setattr(a, "weight_dtype", 5)), 1, "weight: dtype must be"),
        (lambda a, keep: setattr(a, "out", None), 1, "null argument"),
        (lambda a, keep: setattr(a, "out_ld", 7), 1, "out_ld must be at least n"),
        (lambda a, keep: setattr(a, "kinds", 0), 1, "kinds must be a non-empty set"),
        (lambda a, keep: setattr(a, "kinds", 0x80), 1, "kinds must be a non-empty set"),
        (lambda a, keep: setattr(a, "factor", None), 1, "needs the factor"),
        (lambda a, keep: (setattr(a, "factor", None), setattr(a, "kinds", 0x20)), 1, "needs the factor"),
        (lambda a, keep: setattr(a, "factor_ld", 2), 1, "factor_ld must be at least m + 1"),
        (lambda a, keep: setattr(a, "dispersion", 0.0), 1, "dispersion must be finite and positive"),
        (lambda a, keep: setattr(a, "dispersion", -1.0), 1, "dispersion must be finite and positive"),
        (lambda a, keep: setattr(a, "dispersion", float("nan")), 1, "dispersion must be finite and positive"),
        (lambda a, keep: setattr(a, "dispersion", float("inf")), 1, "dispersion must be finite and positive"),
        (poke("factor", 2, 1, np.nan), 1, "lower triangle of the factor must be finite"),
        (poke("factor", 1, 1, np.inf), 1, "lower triangle of the factor must be finite"),
    ]
    for change, code, text in checks:
        a, keep = _input()
        change(a, keep)
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
    # what is not an error: a NaN in the strict upper triangle (never read), a null factor and any dispersion when no
    # kind uses them -- such calls get as far as the device (the x pointer above is not a device pointer: code 1 with the
    # pointer's message, or code 2 where no device is visible)
    for change in (poke("factor", 0, 2, np.nan),
                   lambda a, keep: (setattr(a, "factor", None), setattr(a, "dispersion", -1.0), setattr(a, "kinds", 0x0e)),
                   lambda a, keep: (setattr(a, "dispersion", float("nan")), setattr(a, "kinds", 0x0f))):
        a, keep = _input()
        change(a, keep)
        rc, msg = _call(a)
        assert (rc == 2 and "no HIP device" in msg) or (rc == 1 and "diag_device: x" in msg), (rc, msg)
    # m + 1 = 1025: unsupported, said before the device is touched
    a, keep = _input(p=2000, cols=tuple(range(1024)), beta=(0.0,) * 1024)
    rc, msg = _call(a)
    assert rc == 3 and "m + 1 must be at most 1024" in msg
    assert lib.bessx_op_diag_bench(None, 0, 1, 1, 1, 1, None, 0, 1, None, None, None) == 1


def test_python_checks_are_made_before_any_device_call():
    class Fake:  # a device array by its interface only: any device call on it would fail
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3,
                                             "strides": None}
    x = Fake((10, 4))
    with pytest.raises(ValueError, match="cols must be ascending and distinct"):
        capi.diagnostics_device(x, [2, 1], [0.1, 0.2], 0.0, np.zeros(10), factor=np.eye(3))
    with pytest.raises(ValueError, match="one model per call"):
        capi.diagnostics_device(x, [1, 2], np.zeros((2, 2)), 0.0, np.zeros(10), factor=np.eye(3))
    with pytest.raises(ValueError, match="beta and coef0 must be finite"):
        capi.diagnostics_device(x, [1, 2], [0.1, np.nan], 0.0, np.zeros(10), factor=np.eye(3))
    with pytest.raises(ValueError, match="link must be one of"):
        capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(10), factor=np.eye(2), link="cox")
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to y.shape\(0\)"):
        capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(9), factor=np.eye(2))
    with pytest.raises(ValueError, match="kinds must be taken from"):
        capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(10), factor=np.eye(2), kinds=["hat"])
    with pytest.raises(ValueError, match=r"factor must have shape \(2, 2\)"):
        capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(10), factor=np.eye(3))
    with pytest.raises(ValueError, match="out must be a device array"):
        capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(10), factor=np.eye(2), out=np.zeros((7, 10)))
    with pytest.raises(ValueError, match=r"out must have shape \(2, 10\)"):
        capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(10), kinds=["response", "pearson"], out=Fake((3, 10)))
    # the library's own checks, through the Python face: they raise before the fake pointer is looked at
    for kw, text in ((dict(factor=None), "needs the factor"), (dict(factor=np.eye(2), dispersion=0.0), "dispersion"),
                     (dict(factor=np.full((2, 2), np.nan)), "lower triangle of the factor")):
        with pytest.raises(capi.BessxError) as e:
            capi.diagnostics_device(x, [1], [0.1], 0.0, np.zeros(10), **kw)
        assert e.value.code == 1 and text in str(e.value)
    est = _est("identity", np.array([1.0, 0.0, 2.0]), 0.0)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        est.diagnostics(x, np.zeros(10))
