"""Cox coefficient tables without a GPU: bess_base.inference_survival on a NumPy X (bess_base._cox_information_host, fp64
NumPy) and capi.cox_wald_table against the longdouble reference and the derived bounds of tests/coxinforef.py; the
reference's own cross-check against the O(n^2) definition and a central difference; and the argument checks of
bessx_cox_info_device, which are made before any device call."""
import ctypes

import numpy as np
import pytest

import coxinforef
from bess_amd import capi, linear

LD = np.longdouble
N, P, M = 300, 40, 6


def _cox(beta):
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, 0.0
    return est


def test_symbols_are_exported():
    for name in ("bessx_cox_info_device", "bessx_cox_info_workspace", "bessx_op_cox_info_bench"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    for name in ("CoxInfoInput", "cox_information_device", "cox_info_workspace", "op_cox_info_bench", "cox_wald_table"):
        assert hasattr(capi, name)
    assert hasattr(linear.PdasCox, "inference_survival")


def test_the_reference_is_the_definition_and_the_hessian():
    assert coxinforef.self_check()


_CASES = {}


def _case(weighted):
    """A model on N rows with a support of M of P columns: standard-normal X, beta ~ N(0, 1 / M), about a third of the rows
    sharing a time, about 70 % events, weights in eighths with zeros -- computed once and shared."""
    if weighted not in _CASES:
        rng = np.random.default_rng(31 + weighted)
        X = rng.standard_normal((N, P))
        cols = np.sort(rng.choice(P, M, replace=False))
        beta = np.zeros(P)
        beta[cols] = rng.standard_normal(M) / np.sqrt(M)
        time = rng.integers(0, int(2.5 * N), N) / 8.0
        status = (rng.uniform(size=N) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, N) / 8.0 if weighted else None
        _CASES[weighted] = dict(X=X, cols=cols, beta=beta, y=np.column_stack([time, status]), time=time, status=status, w=w)
    return _CASES[weighted]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ties", ["order", "breslow"])
def test_numpy_route_is_within_the_bounds_of_the_reference(ties, weighted):
    cs = _case(weighted)
    shared = np.unique(cs["time"], return_counts=True)[1]
    assert 0.2 < shared[shared > 1].sum() / N < 0.5  # (about a third of the rows share a time)
    ref = coxinforef.cox_information_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["time"], cs["status"],
                                               cs["w"], ties, coxinforef.host_depths(N, int(cs["status"].sum())))
    got = linear.bess_base._cox_information_host(cs["X"][:, cs["cols"]], cs["beta"][cs["cols"]], cs["time"], cs["status"],
                                                 np.ones(N) if cs["w"] is None else cs["w"], ties)
    coxinforef.check_cox_information(got, ref, "%s weighted=%s" % (ties, weighted))
    assert np.array_equal(got["info"], got["info"].T)
    tb = _cox(cs["beta"]).inference_survival(cs["X"], cs["y"], weight=cs["w"], ties=ties)
    assert np.array_equal(tb["cols"], cs["cols"]) and np.array_equal(tb["coef"], cs["beta"][cs["cols"]])
    assert tb["loglik"] == got["loglik"] and tb["residual_sum"] == got["residual_sum"]
    assert np.array_equal(tb["score"], got["score"])
    assert tb["dispersion"] == 1.0 and tb["dof"] == got["n_events"] - M and tb["positive_definite"]
    ev = _cox(cs["beta"]).evaluate_survival(cs["X"], cs["y"], weight=cs["w"], ties=ties)
    assert abs(LD(ev["loglik"]) - ref["loglik"]["loglik"][0]) <= ref["loglik"]["bound"][0]
    se, cov, rel, cond = coxinforef.se_reference(ref)
    print("cond(S*) %.3e, se bound %.3e, se err %.3e" % (cond, float(rel), float(np.abs(tb["se"] - se).max() / se.min())))
    assert rel < 1e-3
    assert (np.abs(tb["se"].astype(LD) - se) <= rel * se).all()
    assert np.allclose(tb["z"], tb["coef"] / tb["se"], rtol=1e-15)
    assert abs(tb["cond"] - cond) <= 1e-6 * cond


def test_edge_data_on_the_numpy_route():
    cs = _case(True)
    X, cols, b = cs["X"], cs["cols"], cs["beta"][cs["cols"]]
    w = np.ones(N)
    host = linear.bess_base._cox_information_host
    # no event: exact zeros
    got = host(X[:, cols], b, cs["time"], np.zeros(N), w, "breslow")
    assert not got["info"].any() and not got["score"].any() and got["loglik"] == 0.0 and got["n_events"] == 0.0
    # every time tied; no ties, in reverse row order; an event only at the last position (its risk set is itself: u = x)
    for time, status in ((np.full(N, 2.0), cs["status"]), (np.arange(N, dtype=float)[::-1].copy(), cs["status"]),
                         (np.arange(N, dtype=float), np.eye(1, N, N - 1).reshape(-1))):
        for ties in ("order", "breslow"):
            ref = coxinforef.cox_information_reference(X, cols, b, time, status, None, ties,
                                                       coxinforef.host_depths(N, int(status.sum())))
            coxinforef.check_cox_information(host(X[:, cols], b, time, status, w, ties), ref, ties)
    # an empty model
    tb = _cox(np.zeros(P)).inference_survival(X, cs["y"])
    assert tb["coef"].size == 0 and tb["cov"].shape == (0, 0) and tb["cols"].size == 0 and tb["residual_sum"] == 0.0
    assert tb["loglik"] == _cox(np.zeros(P)).evaluate_survival(X, cs["y"])["loglik"]


def test_cox_wald_table():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((50, 4))
    info = A.T @ A
    tb = capi.cox_wald_table(info, np.zeros(4), np.arange(1.0, 5.0), 37.5)
    assert tb["se"].shape == tb["z"].shape == tb["p_value"].shape == tb["score"].shape == (4,) and tb["cov"].shape == (4, 4)
    assert tb["dispersion"] == 1.0 and tb["dof"] == 33.5 and tb["positive_definite"]
    assert np.allclose(tb["cov"], np.linalg.inv(info), rtol=1e-10) and np.allclose(tb["se"] ** 2, np.diag(tb["cov"]))
    same = capi.wald_table(info, np.zeros(4), np.arange(1.0, 5.0), "poisson", 0.0, 37.5 + 4)
    for k in ("se", "z", "p_value", "cov"):
        assert np.array_equal(tb[k], same[k]), k
    sing = info.copy()
    sing[:, 3] = sing[:, 1]
    sing[3, :] = sing[1, :]
    sing[3, 3] = sing[1, 1]
    for bad in (sing, np.where(np.eye(4) > 0, np.nan, info), np.zeros((4, 4))):
        tb = capi.cox_wald_table(bad, np.zeros(4), np.ones(4), 10.0)
        assert tb["positive_definite"] is False and tb["dof"] == 6.0
        for k in ("se", "z", "p_value", "cov"):
            assert np.isnan(tb[k]).all(), k
    with pytest.raises(ValueError):
        capi.cox_wald_table(np.eye(3), np.zeros(2), np.zeros(3), 10.0)
    # wald_table itself is as it was
    with pytest.raises(ValueError, match="link must be one of"):
        capi.wald_table(np.eye(1), np.zeros(1), np.zeros(1), "cox", 1.0, 10.0)


def test_other_families_raise_and_inference_stays_none_for_cox():
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = 4, np.array([1.0, 0, 0, 0]), 0.0
    with pytest.raises(ValueError, match="inference_survival is for the Cox classes, this is a Lm model"):
        lm.inference_survival(np.zeros((10, 4)), np.zeros((10, 2)))
    cox = _cox(np.array([1.0, 0, 0, 0]))
    assert cox.inference(np.zeros((10, 4)), np.zeros((10, 2))) is None
    with pytest.raises(ValueError, match="ties must be one of"):
        cox.inference_survival(np.zeros((10, 4)), np.zeros((10, 2)), ties="efron")
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 4"):
        cox.inference_survival(np.zeros((10, 5)), np.zeros((10, 2)))
    with pytest.raises(ValueError, match=r"y should have shape"):
        cox.inference_survival(np.zeros((10, 4)), np.zeros(10))
    with pytest.raises(ValueError, match=r"status \(y\[:, 1\]\) should be 0 or 1"):
        cox.inference_survival(np.zeros((10, 4)), np.full((10, 2), 2.0))


def test_workspace_needs_no_device_and_depends_on_the_counts_alone():
    for n, m, J in ((1, 1, 0), (1023, 15, 700), (4097, 150, 2800), (200000, 1023, 200000)):
        d, s1, s2 = capi.cox_info_workspace(n, m, J)
        assert s1 == capi.info_workspace(n, m)[1:]
        assert s2 == (capi.info_workspace(J, m)[1:] if J else (0, 0))
        assert d >= (m + 2) * n + J * m and d <= (m + 6) * n + (J + 1) * m + 2 * 256 * 256 * 2200 + 2 * (m + 2) ** 2 + 64
    assert capi.cox_info_workspace(200000, 1023, 200000)[0] * 8 < 3.5e9
    assert capi.cox_info_workspace(10, 0, 3)[1:] == ((0, 0), (0, 0))
    with pytest.raises(capi.BessxError) as e:
        capi.cox_info_workspace(127, 1024, 3)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    for bad in ((0, 1, 0), (5, -1, 0), (5, 1, 6)):
        with pytest.raises(capi.BessxError) as e:
            capi.cox_info_workspace(*bad)
        assert e.value.code == 1


def _input(n=8, p=4, cols=(1, 2), beta=(0.5, -0.5)):
    a = capi.CoxInfoInput()
    keep = dict(cols=np.asarray(cols, dtype=np.int32), beta=np.asarray(beta, dtype=np.float64),
                time=np.arange(n, dtype=np.float64), status=np.ones(n), info=np.zeros(len(cols) ** 2),
                score=np.zeros(len(cols)))
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 0x1000, 0, p, 1, n, p
    a.cols, a.m, a.beta = capi._ip(keep["cols"]), len(cols), capi._dp(keep["beta"])
    a.time, a.status, a.ties = capi._dp(keep["time"]), capi._dp(keep["status"]), 0
    a.info, a.info_ld, a.score = keep["info"].ctypes.data, len(cols), keep["score"].ctypes.data
    return a, keep


def _call(a):
    ll, ne, rs = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    rc = capi.lib().bessx_cox_info_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs))
    return rc, capi.last_error()


def test_abi_argument_checks_need_no_gpu():
    lib = capi.lib()
    assert lib.bessx_cox_info_device(None, None, None, None) == 1 and "null" in capi.last_error()

    def nan_time(a, keep):
        keep["time"][3] = np.nan

    def bad_status(a, keep):
        keep["status"][2] = 0.5

    checks = [
        (lambda a, k: setattr(a, "x", None), 1, "null argument"),
        (lambda a, k: setattr(a, "time", None), 1, "null argument"),
        (lambda a, k: setattr(a, "status", None), 1, "null argument"),
        (lambda a, k: setattr(a, "x_dtype", 7), 1, "dtype must be BESSX_F64 or BESSX_F32"),
        (lambda a, k: setattr(a, "x_row_stride", -1), 1, "strides must be non-negative"),
        (lambda a, k: setattr(a, "x_col_stride", -1), 1, "strides must be non-negative"),
        (lambda a, k: setattr(a, "n", 0), 1, "empty matrix"),
        (lambda a, k: setattr(a, "m", 5), 1, "m must lie in [0, p]"),
        (lambda a, k: setattr(a, "cols", None), 1, "null argument (cols)"),
        (lambda a, k: setattr(a, "beta", None), 1, "null argument (beta)"),
        (lambda a, k: setattr(a, "ties", 2), 1, "ties must be 0 (order) or 1 (breslow)"),
        (nan_time, 1, "time holds a NaN"),
        (bad_status, 1, "status must be 0 or 1"),
        (lambda a, k: setattr(a, "info_ld", 1), 1, "info_ld must be at least m"),
        (lambda a, k: setattr(a, "info", None), 1, "null argument"),
        (lambda a, k: setattr(a, "score", None), 1, "null argument"),
    ]
    for change, code, text in checks:
        a, keep = _input()
        change(a, keep)
        rc, msg = _call(a)
        assert rc == code and text in msg and msg.startswith("cox_info_device"), (rc, msg, text)
    for cols, text in (((2, 1), "cols must be ascending and distinct"), ((1, 1), "cols must be ascending and distinct"),
                       ((1, 4), "column number out of range")):
        a, keep = _input(cols=cols)
        rc, msg = _call(a)
        assert rc == 1 and text in msg, (rc, msg)
    a, keep = _input(beta=(0.5, float("inf")))
    rc, msg = _call(a)
    assert rc == 1 and "beta must be finite" in msg
    # m + 1 = 1025: unsupported, said before the device is touched (the x pointer above is not a device pointer)
    a, keep = _input(p=2000, cols=tuple(range(1024)), beta=(0.0,) * 1024)
    rc, msg = _call(a)
    assert rc == 3 and "m + 1 must be at most 1024" in msg
    assert lib.bessx_op_cox_info_bench(None, 0, 1, 1, 1, 1, None, 0, 0, 1, None, None) == 1
    assert lib.bessx_cox_info_workspace(8, 2, 3, None, None, None) == 1


def test_python_checks_are_made_before_any_device_call():
    class Fake:  # a device array by its interface only: any device call on it would fail
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3,
                                             "strides": None}
    x, t, s = Fake((10, 4)), np.arange(10.0), np.ones(10)
    with pytest.raises(ValueError, match="cols must be ascending and distinct"):
        capi.cox_information_device(x, [2, 1], [0.1, 0.2], t, s)
    with pytest.raises(ValueError, match="beta must be 1-D"):
        capi.cox_information_device(x, [1, 2], np.zeros((2, 2)), t, s)
    with pytest.raises(ValueError, match="beta must be finite"):
        capi.cox_information_device(x, [1, 2], [0.1, np.nan], t, s)
    with pytest.raises(ValueError, match="ties must be one of"):
        capi.cox_information_device(x, [1], [0.1], t, s, ties="efron")
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to time.size"):
        capi.cox_information_device(x, [1], [0.1], t[:9], s)
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to weight.size"):
        capi.cox_information_device(x, [1], [0.1], t, s, weight=np.ones(11))
    with pytest.raises(ValueError, match="There is NAN value in time"):
        capi.cox_information_device(x, [1], [0.1], np.where(t == 3, np.nan, t), s)
    with pytest.raises(ValueError, match="status should be 0 or 1"):
        capi.cox_information_device(x, [1], [0.1], t, s * 2)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        _cox(np.array([1.0, 0.0, 2.0])).inference_survival(x, np.zeros((10, 2)))
