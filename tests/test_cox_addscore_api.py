"""Cox score tests of the excluded columns without a GPU: the NumPy route of bess_base.score_tests_survival against the
longdouble reference of tests/coxaddscoreref.py (the explicit risk-set definition) within its derived bounds,
capi.cox_score_test_table on hand-made inputs, bessx_cox_addscore_workspace, and the argument errors that the library
finds before any device call."""
import ctypes

import numpy as np
import pytest

import coxaddscoreref
from bess_amd import capi, linear

# (n, p, m, candidates: None = all / "scattered" = 37 of p / "support")
SHAPES = [(31, 40, 0, None), (33, 40, 1, None), (127, 70, 15, None), (203, 70, 16, "scattered"), (1025, 70, 31, None),
          (4097, 50, 5, None), (203, 70, 5, "support")]


def _case(n, p, m, weighted, all_tied=False):
    """Standard-normal columns, times rounded to eighths (real tie groups), censoring, weights in eighths with zeros."""
    rng = np.random.default_rng(7 * n + 3 * m + int(weighted))
    X = rng.standard_normal((n, p))
    cols = np.sort(rng.choice(p, m, replace=False))
    beta = np.zeros(p)
    beta[cols] = rng.standard_normal(m) / np.sqrt(max(m, 1))
    beta[cols] = np.where(beta[cols] == 0, 0.1, beta[cols])
    time = np.ceil(rng.exponential(np.exp(-(X @ beta))) * 8) / 8
    if all_tied:
        time[:] = 1.0
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    w = rng.integers(0, 17, n) / 8.0 if weighted else None
    return dict(X=X, cols=cols, beta=beta, y=np.column_stack([time, status]), w=w)


def _cand(kind, cs, p):
    if kind is None:
        return None
    if kind == "support":
        return cs["cols"].astype(np.int64)
    return np.sort(np.random.default_rng(p).choice(p, 37, replace=False))


def _est(cs):
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = cs["X"].shape[1], cs["beta"], 0.0
    return est


def test_the_reference_is_the_direct_risk_set_definition():
    assert coxaddscoreref.self_check()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ties", ["order", "breslow"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-p%d-m%d-%s" % s)
def test_numpy_route_is_within_the_bounds_of_the_reference(shape, ties, weighted):
    n, p, m, kind = shape
    cs = _case(n, p, m, weighted)
    cand = _cand(kind, cs, p)
    cols, b = cs["cols"], cs["beta"][cs["cols"]]
    w = np.ones(n) if cs["w"] is None else cs["w"]
    got = linear.bess_base._cox_score_tests_host(cs["X"], cols, b, cs["y"][:, 0], cs["y"][:, 1], w, ties, cand)
    R = None
    if m:
        R, pd = capi.info_factor(got["info"])
        assert pd
    ref = coxaddscoreref.cox_addscore_reference(cs["X"], cols, b, cs["y"][:, 0], cs["y"][:, 1], cs["w"], ties, R, cand,
                                                coxaddscoreref.host_depths(n))
    what = "numpy n=%d m=%d %s" % (n, m, ties)
    coxaddscoreref.check_vectors(got, ref, what)
    st = coxaddscoreref.statistic_reference(ref)
    table = _est(cs).score_tests_survival(cs["X"], cs["y"], weight=cs["w"], ties=ties, candidates=cand)
    coxaddscoreref.check_table(table, st, what)
    assert np.array_equal(table["cols"], cols) and table["dispersion"] == 1.0
    if kind == "support":
        assert table["in_model"].all() and np.isnan(table["statistic"]).all()
        LD = coxaddscoreref.LD
        assert (np.abs(table["variance"].astype(LD) - st["var"]) <= st["bvar"] + LD(2.0) ** -50 * ref["d"]).all()
        assert (np.abs(table["variance"]).astype(LD) <= LD(1e-9) * ref["d"]).all()  # (rounding noise)


def test_all_times_equal():
    n, p, m = 127, 40, 3
    cs = _case(n, p, m, True, all_tied=True)
    cols, b = cs["cols"], cs["beta"][cs["cols"]]
    for ties in ("order", "breslow"):
        got = linear.bess_base._cox_score_tests_host(cs["X"], cols, b, cs["y"][:, 0], cs["y"][:, 1], cs["w"], ties, None)
        R, pd = capi.info_factor(got["info"])
        assert pd
        ref = coxaddscoreref.cox_addscore_reference(cs["X"], cols, b, cs["y"][:, 0], cs["y"][:, 1], cs["w"], ties, R,
                                                    None, coxaddscoreref.host_depths(n))
        coxaddscoreref.check_vectors(got, ref, "all tied " + ties)
        coxaddscoreref.check_table(capi.cox_score_test_table(got), coxaddscoreref.statistic_reference(ref), "all tied")


def test_no_event_gives_zeros_and_a_nan_table():
    cs = _case(50, 12, 2, False)
    cs["y"][:, 1] = 0.0
    t = _est(cs).score_tests_survival(cs["X"], cs["y"])
    assert (t["score"][~t["in_model"]] == 0).all() or np.isnan(t["score"]).all()
    assert np.isnan(t["statistic"]).all() and np.isnan(t["p_value"]).all() and not t["positive_definite"]


def test_cox_score_test_table_on_hand_made_inputs():
    got = {"columns": np.array([0, 2, 3, 5, 6]), "support": np.array([2]), "u": np.array([3.0, 1.0, -2.0, 1.0, 1.0]),
           "a": np.array([1.0, 1.0, 0.0, 0.0, 0.0]), "d": np.array([9.0, 4.0, 6.0, 2.0, np.nan]),
           "t": np.array([3.0, 1.0, 1.0, 1.0, 0.0]), "s": np.array([2.0, 3.0, 1.0, 1.0, 0.0])}
    t = capi.cox_score_test_table(got)
    assert np.array_equal(t["columns"], got["columns"]) and t["dispersion"] == 1.0
    assert np.array_equal(t["score"], [2.0, 0.0, -2.0, 1.0, 1.0])
    assert np.array_equal(t["variance"][:4], [4.0, 0.0, 4.0, 0.0]) and np.isnan(t["variance"][4])
    assert np.array_equal(t["in_model"], [False, True, False, False, False])
    assert t["statistic"][0] == 1.0 and t["statistic"][2] == 1.0
    assert np.isnan(t["statistic"][[1, 3, 4]]).all() and np.isnan(t["p_value"][[1, 3, 4]]).all()  # in model, var 0, NaN
    import math
    assert t["p_value"][0] == math.erfc(math.sqrt(0.5))
    nan_sa = dict(got, s=np.full(5, np.nan), a=np.full(5, np.nan))  # an information that is not positive definite
    assert np.isnan(capi.cox_score_test_table(nan_sa)["statistic"]).all()
    with pytest.raises(ValueError):
        capi.score_test_table(got, "cox")


def test_workspace_needs_no_device_and_its_block_bound_does_not_depend_on_p():
    n, m, J = 200000, 150, 100000
    small, big = capi.cox_addscore_workspace(n, m, J, 10000), capi.cox_addscore_workspace(n, m, J, 1000000)
    for ws in (small, big):
        assert ws["block"] % 16 == 0 and 16 <= ws["block"] <= 2048
        assert ws["slabs"] == -(-n // ws["rows_per_slab"]) and ws["quad_slabs"] == -(-n // ws["quad_rows_per_slab"])
        assert ws["quad_rows_per_slab"] % 32 == 0
        assert ws["chain"] == ws["rows_per_slab"] + (ws["slabs"] + 15) // 16 + 4
        assert ws["quad_chain"] == 2 * ws["quad_rows_per_slab"] + 3 * ws["quad_slabs"]
    assert small["block_doubles"] == big["block_doubles"] and small["doubles"] == big["doubles"]
    assert small["block_doubles"] * 8 < 128 << 20
    # nothing is n x q: the whole scratch at configs[4]'s shape is a small part of one n x 2048 block of temporaries
    assert capi.cox_addscore_workspace(n, m, J, 20000)["doubles"] < n * 2048
    assert capi.cox_addscore_workspace(n, m, J, 10000, 64)["block"] == 64
    assert capi.cox_addscore_workspace(4097, 5, 3000, 50, 16)["quad_slabs"] > 1
    for bad in (dict(n=0, m=1, n_event_rows=0, q=1), dict(n=5, m=-1, n_event_rows=1, q=1),
                dict(n=5, m=1, n_event_rows=6, q=1), dict(n=5, m=1, n_event_rows=1, q=0),
                dict(n=5, m=1, n_event_rows=1, q=4, candidate_block=24)):
        with pytest.raises(capi.BessxError) as e:
            capi.cox_addscore_workspace(**bad)
        assert e.value.code == 1
    with pytest.raises(capi.BessxError) as e:
        capi.cox_addscore_workspace(100, 1024, 10, 10)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    assert capi.cox_addscore_workspace(100, 1023, 10, 10)["sum_depth"] == 65 + 4


def _raw_input(n=8, p=5, m=2, q=5):
    """A bessx_cox_addscore_input whose pointers are host memory: good enough for the checks that come before any
    device call (the last of them is the question whether x is device memory)."""
    keep = dict(x=np.zeros((n, p)), cols=np.arange(m, dtype=np.int32), beta=np.zeros(max(m, 1)),
                time=np.arange(n, dtype=np.float64), status=np.ones(n), info=np.zeros((m, m)), score=np.zeros(m),
                out=np.zeros((5, q)), factor=np.eye(m))
    a = capi.CoxAddscoreInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = keep["x"].ctypes.data, 0, p, 1, n, p
    a.cols, a.m, a.beta = capi._ip(keep["cols"]), m, capi._dp(keep["beta"])
    a.time, a.status, a.ties = capi._dp(keep["time"]), capi._dp(keep["status"]), 0
    a.factor, a.factor_ld, a.q = capi._dp(keep["factor"]), m, q
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), m, capi._dp(keep["score"])
    a.u, a.d, a.t, a.s, a.a = (keep["out"][k].ctypes.data for k in range(5))
    return a, keep


def _raw_call(a):
    ll, ne, rs = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    return capi.lib().bessx_cox_addscore_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs))


def test_argument_errors_of_the_library_come_before_any_device_call():
    L = capi.lib()
    cases, keep = [], []

    def case(msg, q=5, **change):
        a, k = _raw_input(q=q)
        keep.append(k)
        for name, v in change.items():
            if isinstance(v, np.ndarray):
                k[name + "_given"] = v
                v = capi._ip(v) if v.dtype == np.int32 else v.ctypes.data
            setattr(a, name, v)
        cases.append((a, k, msg))
        return a, k

    case(b"q must be at least 1", q=0)
    case(b"without a candidate list q must be p", q=3)
    case(b"ascending and distinct", q=3, candidates=np.array([0, 3, 2], dtype=np.int32))
    case(b"ascending and distinct", q=3, candidates=np.array([0, 2, 2], dtype=np.int32))
    case(b"not a column of x", q=3, candidates=np.array([0, 2, 5], dtype=np.int32))
    case(b"multiple of 16", candidate_block=40)
    case(b"ties must be 0 (order) or 1 (breslow)", ties=2)
    case(b"null argument (s, a)", s=None)
    case(b"null argument (u, d, t)", t=None)
    a, k = case(b"cross_ld must be at least m + 1", cross_ld=2)
    k["cross"] = np.zeros((5, 3))
    a.cross = k["cross"].ctypes.data
    a, k = case(b"status must be 0 or 1")
    k["status"][3] = 2.0
    a, k = case(b"time holds a NaN")
    k["time"][2] = np.nan
    a, k = case(b"lower triangle of the factor must be finite")
    k["factor"][1, 0] = np.nan
    for a, k, msg in cases:
        assert _raw_call(a) == 1 and msg in L.bessx_last_error(), msg
    assert L.bessx_cox_addscore_device(None, None, None, None) == 1
    # every check passed: the next answer is about the device (none here) or about x not being device memory
    a, k = _raw_input()
    assert _raw_call(a) in (1, 2) and b"candidate" not in L.bessx_last_error()


def test_argument_errors_of_the_estimator():
    cs = _case(60, 12, 2, False)
    est = _est(cs)
    X, y = cs["X"], cs["y"]
    for cand in ([3, 2], [2, 2], [0, 12], [-1, 2], [], [[1, 2]], [0.5, 2.0]):
        with pytest.raises(ValueError):
            est.score_tests_survival(X, y, candidates=cand)
    with pytest.raises(ValueError, match="ties"):
        est.score_tests_survival(X, y, ties="efron")
    with pytest.raises(ValueError, match="shape"):
        est.score_tests_survival(X, y[:-1])
    with pytest.raises(ValueError, match="weight.size"):
        est.score_tests_survival(X, y, weight=np.ones(61))
    with pytest.raises(ValueError, match="X.shape"):
        est.score_tests_survival(X[:, :-1], y)
    bad = y.copy()
    bad[3, 1] = 2.0
    with pytest.raises(ValueError, match="0 or 1"):
        est.score_tests_survival(X, bad)
    bad = y.copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError, match="NAN"):
        est.score_tests_survival(X, bad)
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = 12, cs["beta"], 0.0
    with pytest.raises(ValueError, match="Cox"):
        lm.score_tests_survival(X, y)
    assert est.score_tests(X, y) is None  # (unchanged: the Cox classes answer through score_tests_survival)
