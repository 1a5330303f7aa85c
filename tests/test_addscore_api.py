"""Score tests of the excluded columns without a GPU: bess_base.score_tests on a NumPy X
(bess_base._score_tests_host, fp64 NumPy) and capi.score_test_table against the longdouble reference and the derived
bounds of tests/addscoreref.py at depth n; score_test_table on hand-made inputs; bessx_addscore_workspace, which needs no
device; and the argument checks, which are made before any device call."""
import ctypes

import numpy as np
import pytest

import addscoreref
from bess_amd import capi, linear

LD = np.longdouble
LINKS = ["identity", "logistic", "poisson"]
N, P, SIGNAL = 300, 40, 23


def _est(link, beta, coef0):
    est = {"identity": linear.PdasLm, "logistic": linear.PdasLogistic, "poisson": linear.PdasPoisson}[link]()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, coef0
    return est


_CASES = {}


def _case(link, weighted):
    """A model on N rows with a support of 6 of P columns that leaves out the column SIGNAL the responses depend on;
    weights are multiples of 1/8 with zeros.  Computed once and shared."""
    key = (link, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(31 + 3 * LINKS.index(link) + weighted)
        X = rng.standard_normal((N, P))
        cols = np.sort(rng.choice(np.setdiff1d(np.arange(P), [SIGNAL]), 6, replace=False))
        beta = np.zeros(P)
        beta[cols] = rng.standard_normal(6) * 0.5
        coef0 = 0.3
        eta = X @ beta + coef0 + 0.9 * X[:, SIGNAL]
        y = {"identity": eta + rng.standard_normal(N),
             "logistic": (rng.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(float),
             "poisson": rng.poisson(np.exp(np.clip(eta, -5, 3))).astype(float)}[link]
        w = rng.integers(0, 17, N) / 8.0 if weighted else None
        _CASES[key] = dict(X=X, cols=cols, beta=beta, coef0=coef0, y=y, w=w)
    return _CASES[key]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("link", LINKS)
def test_numpy_route_is_within_the_bounds_of_the_reference(link, weighted):
    cs = _case(link, weighted)
    w = np.ones(N) if cs["w"] is None else cs["w"]
    got = linear.bess_base._score_tests_host(link, cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], w,
                                             None)
    assert got["positive_definite"]
    R, pd = capi.info_factor(got["info"])
    ref = addscoreref.addscore_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], cs["w"], link,
                                         R, None, depth=N, depth_score=N, sum_depth=N)
    addscoreref.check_vectors(got, ref, "%s weighted=%s" % (link, weighted))
    table = _est(link, cs["beta"], cs["coef0"]).score_tests(cs["X"], cs["y"], weight=cs["w"])
    st = addscoreref.statistic_reference(ref)
    addscoreref.check_table(table, st, "%s weighted=%s" % (link, weighted))
    assert np.array_equal(table["cols"], cs["cols"]) and np.array_equal(table["columns"], np.arange(P))
    assert int(np.nanargmin(table["p_value"])) == SIGNAL
    # a candidate list gives the same numbers for its columns
    cand = np.array([1, SIGNAL, int(cs["cols"][2]), P - 1])
    cand.sort()
    sub = _est(link, cs["beta"], cs["coef0"]).score_tests(cs["X"], cs["y"], weight=cs["w"], candidates=cand)
    assert np.array_equal(sub["columns"], cand) and np.array_equal(sub["in_model"], np.isin(cand, cs["cols"]))
    both = ~sub["in_model"]
    assert np.allclose(sub["statistic"][both], table["statistic"][cand][both], rtol=1e-10)


def test_identity_statistic_is_the_drop_of_the_residual_sum_of_squares():
    cs = _case("identity", False)
    table = _est("identity", cs["beta"], cs["coef0"]).score_tests(cs["X"], cs["y"])
    Z = np.column_stack([np.ones(N), cs["X"][:, cs["cols"]]])
    rss = lambda A: float(((cs["y"] - A @ np.linalg.lstsq(A, cs["y"], rcond=None)[0]) ** 2).sum())  # noqa: E731
    outside = np.setdiff1d(np.arange(P), cs["cols"])
    for j in (int(outside[0]), SIGNAL, int(outside[-1])):
        drop = rss(Z) - rss(np.column_stack([Z, cs["X"][:, j]]))
        assert abs(table["statistic"][j] * table["dispersion"] - drop) <= 1e-9 * max(drop, 1.0)


def test_score_test_table_on_hand_made_inputs():
    got = {"columns": np.array([0, 2, 3, 5, 7]), "u": np.array([3.0, 1.0, 2.0, 1.0, 4.0]),
           "a": np.array([1.0, 0.0, 0.0, 0.0, 0.0]), "d": np.array([8.0, 1.0, 1.0, np.inf, 2.0]),
           "s": np.array([4.0, 1.0, 2.0, 1.0, 1.0]), "score": np.zeros(3), "loss": 14.0, "sum_w": 10.0,
           "support": np.array([7, 9])}
    t = capi.score_test_table(got, "logistic")
    assert t["dispersion"] == 1.0
    assert np.array_equal(t["in_model"], [False, False, False, False, True])
    assert t["statistic"][0] == 1.0 and np.array_equal(t["score"], [2.0, 1.0, 2.0, 1.0, 4.0])
    assert np.array_equal(t["variance"][:3], [4.0, 0.0, -1.0])
    assert np.isnan(t["statistic"][1:]).all() and np.isnan(t["p_value"][1:]).all()  # variance 0, < 0, inf; in the model
    assert abs(t["p_value"][0] - 0.31731050786291415) < 1e-15  # P(chi2_1 > 1)
    t = capi.score_test_table(got, "identity")
    assert t["dispersion"] == 2.0 and t["statistic"][0] == 0.5
    got["sum_w"] = 3.0  # no residual degrees of freedom
    assert np.isnan(capi.score_test_table(got, "identity")["statistic"]).all()
    with pytest.raises(ValueError):
        capi.score_test_table(got, "cox")


def test_workspace_needs_no_device_and_its_block_bound_does_not_depend_on_p():
    n, m = 50000, 200
    small, big = capi.addscore_workspace(n, m, 10000), capi.addscore_workspace(n, m, 1000000)
    Mp = 16 * ((m + 2 + 15) // 16)
    for ws in (small, big):
        assert ws["block"] % 16 == 0 and 16 <= ws["block"] <= 2048
        assert ws["rows_per_slab"] % 16 == 0 and ws["slabs"] == -(-n // ws["rows_per_slab"])
        assert ws["sum_depth"] == Mp // 16 + 4
    assert small["block_doubles"] == big["block_doubles"] and small["doubles"] == big["doubles"]
    assert (small["rows_per_slab"], small["slabs"]) == (big["rows_per_slab"], big["slabs"])
    # scratch is v, g, the n x Mp panel (rows padded to 32) and the block bound (which holds the small pass behind r)
    panel = (n + 31) // 32 * 32 * Mp
    assert small["doubles"] == 2 * n + panel + small["block_doubles"]
    assert small["block_doubles"] * 8 < 128 << 20
    assert capi.addscore_workspace(n, m, 10000, 64)["block"] == 64
    assert capi.addscore_workspace(4097, 31, 600)["block"] == 608  # fewer candidates than a block: its tile rows
    for bad in (dict(n=0, m=1, q=1), dict(n=5, m=-1, q=1), dict(n=5, m=1, q=0), dict(n=5, m=1, q=4, candidate_block=24)):
        with pytest.raises(capi.BessxError) as e:
            capi.addscore_workspace(**bad)
        assert e.value.code == 1
    with pytest.raises(capi.BessxError) as e:
        capi.addscore_workspace(100, 1024, 10)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    assert capi.addscore_workspace(100, 1023, 10)["sum_depth"] == 65 + 4


def _raw_input(n=8, p=5, m=2, q=5):
    """A bessx_addscore_input whose pointers are host memory: good enough for the checks that come before any device
    call (the last of them is the question whether x is device memory)."""
    keep = dict(x=np.zeros((n, p)), cols=np.arange(m, dtype=np.int32), beta=np.zeros(max(m, 1)), y=np.zeros(n),
                info=np.zeros((m + 1, m + 1)), score=np.zeros(m + 1), out=np.zeros((4, q)), factor=np.eye(m + 1))
    a = capi.AddscoreInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = keep["x"].ctypes.data, 0, p, 1, n, p
    a.cols, a.m, a.beta, a.coef0, a.link = capi._ip(keep["cols"]), m, capi._dp(keep["beta"]), 0.0, 0
    a.y_host, a.y_stride = capi._dp(keep["y"]), 1
    a.factor, a.factor_ld, a.q = capi._dp(keep["factor"]), m + 1, q
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), m + 1, capi._dp(keep["score"])
    a.u, a.d, a.s, a.a = (keep["out"][k].ctypes.data for k in range(4))
    return a, keep


def _raw_call(a):
    loss, sw = ctypes.c_double(0), ctypes.c_double(0)
    return capi.lib().bessx_addscore_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw))


def test_argument_errors_of_the_library_come_before_any_device_call():
    L = capi.lib()
    cases = []
    a, k1 = _raw_input()
    a.q = 0
    cases.append((a, b"q must be at least 1"))
    a, k2 = _raw_input()
    a.q = 3
    cases.append((a, b"without a candidate list q must be p"))
    a, k3 = _raw_input(q=3)
    c3 = np.array([0, 3, 2], dtype=np.int32)
    a.candidates = capi._ip(c3)
    cases.append((a, b"ascending and distinct"))
    a, k4 = _raw_input(q=3)
    c4 = np.array([0, 2, 2], dtype=np.int32)
    a.candidates = capi._ip(c4)
    cases.append((a, b"ascending and distinct"))
    a, k5 = _raw_input(q=3)
    c5 = np.array([0, 2, 5], dtype=np.int32)
    a.candidates = capi._ip(c5)
    cases.append((a, b"not a column of x"))
    a, k6 = _raw_input()
    a.candidate_block = 40
    cases.append((a, b"multiple of 16"))
    a, k7 = _raw_input()
    a.s = None
    cases.append((a, b"null argument (s, a)"))
    a, k8 = _raw_input()
    k8["factor"][1, 0] = np.nan
    cases.append((a, b"lower triangle of the factor must be finite"))
    a, k9 = _raw_input()
    a.u = None
    cases.append((a, b"null argument (u, d)"))
    a, k10 = _raw_input()
    k10["cross"] = np.zeros((5, 3))
    a.cross, a.cross_ld = k10["cross"].ctypes.data, 2
    cases.append((a, b"cross_ld must be at least m + 1"))
    for a, msg in cases:
        assert _raw_call(a) == 1 and msg in L.bessx_last_error(), msg
    assert L.bessx_addscore_device(None, None, None) == 1
    # every check passed: the next answer is about the device (none here) or about x not being device memory
    a, k11 = _raw_input()
    assert _raw_call(a) in (1, 2) and b"candidate" not in L.bessx_last_error()


def test_argument_errors_of_the_estimator():
    cs = _case("identity", False)
    est = _est("identity", cs["beta"], cs["coef0"])
    X, y = cs["X"], cs["y"]
    for cand in ([3, 2], [2, 2], [0, P], [-1, 2], [], [[1, 2]], [0.5, 2.0]):
        with pytest.raises(ValueError):
            est.score_tests(X, y, candidates=cand)
    with pytest.raises(ValueError, match="y.size"):
        est.score_tests(X, y[:-1])
    with pytest.raises(ValueError, match="weight.size"):
        est.score_tests(X, y, weight=np.ones(N + 1))
    with pytest.raises(ValueError, match="X.shape"):
        est.score_tests(X[:, :-1], y)
    multi = _est("identity", np.zeros((P, 2)), np.zeros(2))
    multi.beta[3, 0] = multi.beta[4, 1] = 1.0
    with pytest.raises(ValueError, match="one model"):
        multi.score_tests(X, np.column_stack([y, y]))
    cox = linear.PdasCox()
    cox.p, cox.beta, cox.coef0 = P, cs["beta"], 0.0
    assert cox.score_tests(X, np.column_stack([np.abs(y) + 1, np.ones(N)])) is None


def test_a_singular_information_gives_nan_and_raises_nothing():
    cs = _case("logistic", False)
    X = cs["X"].copy()
    X[:, 5] = X[:, 4]
    beta = np.zeros(P)
    beta[[4, 5]] = 0.3
    t = _est("logistic", beta, 0.1).score_tests(X, cs["y"])
    assert np.isnan(t["statistic"]).all() and np.isnan(t["p_value"]).all()
    assert np.array_equal(np.nonzero(t["in_model"])[0], [4, 5])
