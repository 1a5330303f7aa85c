"""The proportional-hazards test without a GPU: capi.zph_transform and capi.cox_zph_table on hand-computed cases,
bess_base.proportional_hazards_test on a NumPy X (bess_base._cox_zph_host, fp64 NumPy) against the longdouble reference
and the derived bounds of tests/coxzphref.py, the reference's own cross-check against the O(n^2) definitions, a simulated
drift, and the argument checks of bessx_cox_zph_device, which are made before any device call."""
import ctypes
import math

import numpy as np
import pytest

import coxzphref
from bess_amd import capi, linear

LD = np.longdouble
N, P, M = 300, 40, 6
OUT = ("info0", "info1", "info2", "score0", "score1")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _cox(beta):
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, 0.0
    return est


def test_symbols_are_exported_declared_and_listed():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bessx.h")).read()
    for name in ("bessx_cox_zph_device", "bessx_cox_zph_workspace", "bessx_op_cox_zph_bench"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and name + "(" in header
    assert "bessx_cox_zph_input" in header
    for name in ("CoxZphInput", "cox_zph_device", "cox_zph_workspace", "op_cox_zph_bench", "zph_transform", "cox_zph_table"):
        assert hasattr(capi, name)
    assert hasattr(linear.PdasCox, "proportional_hazards_test")


def test_the_reference_is_the_definition_and_shifting_g_moves_nothing_but_the_score():
    assert coxzphref.self_check()


# ---- zph_transform: ten rows with ties, censoring and zero weights, every value worked out by hand ------------------
T10 = np.array([1.0, 2, 2, 3, 4, 4, 5, 6, 7, 8])
S10 = np.array([1.0, 1, 0, 1, 1, 1, 0, 1, 0, 1])
W10 = np.array([1.0, 2, 1, 0, 1, 1, 1, 0.5, 1, 2])  # (row 3 is an event of weight 0)
# wd = w * status at the events (rows 0, 1, 3, 4, 5, 7, 9) = 1, 2, 0, 1, 1, 0.5, 2: sum 7.5


def test_transforms_and_their_centres_on_ten_rows():
    g, c = capi.zph_transform(T10, S10, W10, "identity")
    assert c == 32.0 / 7.5  # (1 + 4 + 0 + 4 + 4 + 3 + 16) / 7.5
    assert np.array_equal(g, T10 - c)
    g, c = capi.zph_transform(T10, S10, W10, "log")
    want = (2 * math.log(2) + 2 * math.log(4) + 0.5 * math.log(6) + 2 * math.log(8)) / 7.5
    assert abs(c - want) <= 4e-16 * want and np.array_equal(g, np.log(T10) - c)
    # the event times are 1, 2, 3, 4, 4, 6, 8: mid-ranks 1, 2, 3, 4.5, 4.5, 6, 7; a censored time lies between them
    g, c = capi.zph_transform(T10, S10, W10, "rank")
    rank = np.array([1.0, 2, 2, 3, 4.5, 4.5, 5.5, 6, 6.5, 7])
    assert c == 31.0 / 7.5 and np.array_equal(g, rank - c)  # (1 + 4 + 0 + 4.5 + 4.5 + 3 + 14) / 7.5
    # Kaplan-Meier of all rows with the weights: at risk 10.5, 9.5, 6.5, 6.5, 4.5, 3.5, 3, 2 at the times 1 .. 8; events of
    # weight 1, 2, 0, 2, -, 0.5, -, 2
    s1 = 9.5 / 10.5
    s2 = s1 * (7.5 / 9.5)
    s4 = s2 * (4.5 / 6.5)
    s6 = s4 * (3.0 / 3.5)
    km = 1.0 - np.array([1.0, s1, s1, s2, s2, s2, s4, s4, s6, s6])  # S just before each row's time
    g, c = capi.zph_transform(T10, S10, W10, "km")
    wd = np.array([1.0, 2, 0, 1, 1, 0.5, 2])
    want = float(np.sum(wd * km[S10 != 0])) / 7.5
    assert abs(c - want) <= 4e-16 and np.abs(g - (km - c)).max() <= 4e-16
    assert abs(float(np.sum((W10 * S10 * g)[S10 != 0]))) <= 1e-15  # centred at the wd-weighted mean of the events
    # without weights every event counts once
    g, c = capi.zph_transform(T10, S10, None, "identity")
    assert c == 28.0 / 7.0
    # an array and a callable
    g, c = capi.zph_transform(T10, S10, W10, T10 ** 2)
    g2, c2 = capi.zph_transform(T10, S10, W10, lambda t: t ** 2)
    assert c == c2 == (1 + 8 + 16 + 16 + 18 + 128) / 7.5 and np.array_equal(g, g2) and np.array_equal(g, T10 ** 2 - c)
    # no event: nothing to centre at
    g, c = capi.zph_transform(T10, np.zeros(10), None, "identity")
    assert c == 0.0 and np.array_equal(g, T10)


def test_transform_errors():
    with pytest.raises(ValueError, match='transform="log" needs positive times'):
        capi.zph_transform(T10 - 1.0, S10, None, "log")
    g, _ = capi.zph_transform(np.where(S10 == 0, 0.0, T10), S10, None, "log")  # (a censored row at time 0 is not read)
    assert np.isfinite(g[S10 != 0]).all()
    with pytest.raises(ValueError, match="transform must be one of"):
        capi.zph_transform(T10, S10, None, "sqrt")
    with pytest.raises(ValueError, match="finite at every row with status 1"):
        capi.zph_transform(T10, S10, None, np.where(T10 == 3, np.inf, T10))
    with pytest.raises(ValueError, match="status should be 0 or 1"):
        capi.zph_transform(T10, S10 * 2, None, "km")
    with pytest.raises(ValueError, match="There is NAN value in time"):
        capi.zph_transform(np.where(T10 == 3, np.nan, T10), S10, None, "km")
    with pytest.raises(ValueError, match=r"should be equal to weight.size"):
        capi.zph_transform(T10, S10, np.ones(9), "km")


# ---- cox_zph_table ---------------------------------------------------------------------------------------------------
def test_table_on_a_hand_built_two_by_two_case():
    got = {"info0": np.diag([2.0, 4.0]), "info1": np.array([[1.0, 0.5], [0.5, 1.0]]), "info2": np.diag([3.0, 5.0]),
           "score0": np.zeros(2), "score1": np.array([1.0, 2.0]), "n_events": 12.5}
    # info1 inverse(info0) info1 = [[0.5625, 0.375], [0.375, 0.375]], D = [[2.4375, -0.375], [-0.375, 4.625]],
    # det D = 11.1328125, score1^T inverse(D) score1 = (4.625 + 4 * 0.375 + 4 * 2.4375) / det
    tb = capi.cox_zph_table(got, centre=0.25)
    assert tb["positive_definite"] and tb["global_df"] == 2 and tb["gt_centre"] == 0.25 and tb["n_events"] == 12.5
    assert np.allclose(tb["chisq"], [1.0 / 2.4375, 4.0 / 4.625], rtol=1e-14, atol=0)
    assert abs(tb["global_chisq"] - 15.875 / 11.1328125) <= 1e-14
    assert np.allclose(tb["slope_var"], [4.625 / 11.1328125, 2.4375 / 11.1328125], rtol=1e-14, atol=0)
    assert tb["p_value"][0] == capi.chi2_sf(tb["chisq"][0], 1) and tb["global_p_value"] == capi.chi2_sf(tb["global_chisq"], 2)
    assert abs(tb["p_value"][1] - math.erfc(math.sqrt(0.5 * 4.0 / 4.625))) <= 1e-15
    assert abs(tb["cond_info"] - 1.0) <= 1e-15 and tb["cond"] > 1.0
    with pytest.raises(ValueError):
        capi.cox_zph_table(dict(got, info1=np.zeros((3, 3))))


def test_table_on_the_degenerate_cases():
    ok = {"info0": np.diag([2.0, 4.0]), "info1": np.array([[1.0, 0.5], [0.5, 1.0]]), "info2": np.diag([3.0, 5.0]),
          "score0": np.zeros(2), "score1": np.array([1.0, 2.0]), "n_events": 5.0}
    z = np.zeros((2, 2))
    sing = np.array([[2.0, 2.0], [2.0, 2.0]])
    cases = {"info0 is singular": dict(ok, info0=sing), "no event": dict(ok, info0=z, info1=z, info2=z, score1=np.zeros(2)),
             "every event shares one g": dict(ok, info1=z, info2=z, score1=np.zeros(2)),
             "D is indefinite": dict(ok, info2=np.diag([0.1, 5.0])), "a NaN": dict(ok, info1=np.full((2, 2), np.nan)),
             "D vanishes up to rounding": dict(ok, info1=np.diag([2.0, 4.0]), info2=np.diag([2.0 + 1e-15, 4.0]))}
    for name, got in cases.items():
        tb = capi.cox_zph_table(got)
        assert tb["positive_definite"] is False and tb["global_df"] == 2, name
        assert np.isnan(tb["chisq"]).all() and np.isnan(tb["p_value"]).all() and np.isnan(tb["slope_var"]).all(), name
        assert np.isnan(tb["global_chisq"]) and np.isnan(tb["global_p_value"]), name
    e = {k: np.zeros((0, 0)) if k.startswith("info") else np.zeros(0) for k in OUT}
    tb = capi.cox_zph_table(dict(e, n_events=3.0))
    assert tb["chisq"].shape == (0,) and tb["global_df"] == 0 and tb["global_chisq"] == 0.0 and tb["positive_definite"]


# ---- the NumPy route against the reference -----------------------------------------------------------------------------
_CASES = {}


def _case(weighted):
    """test_cox_info_api's model: N rows, a support of M of P columns, about a third of the rows sharing a time, about
    70 % events, weights in eighths with zeros -- computed once and shared."""
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


@pytest.mark.parametrize("transform", ["km", "rank", "identity"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ties", ["order", "breslow"])
def test_numpy_route_is_within_the_bounds_of_the_reference(ties, weighted, transform):
    cs = _case(weighted)
    b = cs["beta"][cs["cols"]]
    gt, centre = capi.zph_transform(cs["time"], cs["status"], cs["w"], transform)
    ref = coxzphref.cox_zph_reference(cs["X"], cs["cols"], b, cs["time"], cs["status"], cs["w"], gt, ties,
                                      coxzphref.host_depths(N, int(cs["status"].sum())))
    w1 = np.ones(N) if cs["w"] is None else cs["w"]
    got = linear.bess_base._cox_zph_host(cs["X"][:, cs["cols"]], b, cs["time"], cs["status"], w1, gt, ties)
    what = "%s weighted=%s %s" % (ties, weighted, transform)
    coxzphref.check_cox_zph(got, ref, what)
    info = linear.bess_base._cox_information_host(cs["X"][:, cs["cols"]], b, cs["time"], cs["status"], w1, ties)
    assert np.array_equal(got["info0"], info["info"]) and np.array_equal(got["score0"], info["score"])
    assert got["loglik"] == info["loglik"] and got["n_events"] == info["n_events"]
    tb = _cox(cs["beta"]).proportional_hazards_test(cs["X"], cs["y"], weight=cs["w"], ties=ties, transform=transform)
    assert np.array_equal(tb["cols"], cs["cols"]) and tb["transform"] == transform and tb["gt_centre"] == centre
    assert tb["loglik"] == got["loglik"] and np.array_equal(tb["score1"], got["score1"]) and tb["global_df"] == M
    coxzphref.check_table(tb, coxzphref.table_reference(ref), what)
    tref = coxzphref.table_reference(ref)
    assert (np.abs(tb["slope_var"].astype(LD) - tref["slope_var"]) <= LD(1e-9) * tref["slope_var"]).all()
    assert abs(tb["cond"] - tref["cond"]) <= 1e-6 * tref["cond"]
    assert abs(tb["cond_info"] - tref["cond_info"]) <= 1e-6 * tref["cond_info"]


def test_edge_data_and_residuals_on_the_numpy_route():
    cs = _case(True)
    X, cols, b = cs["X"], cs["cols"], cs["beta"][cs["cols"]]
    est = _cox(cs["beta"])
    # no event: exact zeros and the degenerate table
    tb = est.proportional_hazards_test(X, np.column_stack([cs["time"], np.zeros(N)]), ties="breslow")
    assert not tb["score1"].any() and not tb["positive_definite"] and np.isnan(tb["chisq"]).all() and tb["n_events"] == 0.0
    # every time tied: one value of g, which centring takes to 0
    tb = est.proportional_hazards_test(X, np.column_stack([np.full(N, 2.0), cs["status"]]), transform="identity")
    assert not tb["score1"].any() and not tb["positive_definite"] and np.isnan(tb["global_chisq"])
    # an empty model
    tb = _cox(np.zeros(P)).proportional_hazards_test(X, cs["y"], residuals=True)
    assert tb["chisq"].size == 0 and tb["cols"].size == 0 and tb["global_df"] == 0 and tb["positive_definite"]
    assert tb["scaled_schoenfeld"].shape == (int(cs["status"].sum()), 0)
    assert tb["loglik"] == _cox(np.zeros(P)).evaluate_survival(X, cs["y"])["loglik"]
    # the points of the plot: Schoenfeld residuals times inverse(info0) n_events, plus beta, in time order
    tb = est.proportional_hazards_test(X, cs["y"], weight=cs["w"], residuals=True)
    J = int(cs["status"].sum())
    d = linear.bess_base._cox_diagnostics_host(X[:, cols], b, cs["time"], cs["status"], cs["w"], "order", None, None,
                                               ("schoenfeld",))
    gt = capi.zph_transform(cs["time"], cs["status"], cs["w"], "km")[0]
    got = linear.bess_base._cox_zph_host(X[:, cols], b, cs["time"], cs["status"], cs["w"], gt, "order")
    want = d["schoenfeld"] @ (np.linalg.inv(got["info0"]) * got["n_events"]) + b
    assert tb["scaled_schoenfeld"].shape == (J, M) and np.allclose(tb["scaled_schoenfeld"], want, rtol=1e-10, atol=1e-10)
    assert np.array_equal(tb["time"], np.sort(cs["time"][cs["status"] != 0]))


def test_a_coefficient_that_changes_sign_is_found_and_a_null_column_is_not():
    """n = 2000, two columns: the first has coefficient +1 before the baseline's median time log 2 and -1 after it, the
    second none.  The model is fitted by Newton steps on the NumPy route; the longdouble reference itself gives a p-value
    below 1e-6 for the first column and above 0.01 for the second (seed 5 was chosen on the CPU for that)."""
    n, t0 = 2000, math.log(2.0)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 2))
    E = rng.exponential(1.0, n)
    r = np.exp(X[:, 0])
    time = np.where(E <= t0 * r, E / r, t0 + (E - t0 * r) * r)  # the cumulative hazard t e^x, then t0 e^x + (t - t0) e^-x
    cens = rng.exponential(4.0, n)
    status = (time <= cens).astype(np.float64)
    time = np.minimum(time, cens)
    y = np.column_stack([time, status])
    beta = np.zeros(2)
    for _ in range(8):
        got = linear.bess_base._cox_information_host(X, beta, time, status, np.ones(n), "order")
        beta = beta + np.linalg.solve(got["info"], got["score"])
    assert np.abs(got["score"]).max() < 1e-6 and (beta != 0).all()
    for transform in ("km", "identity"):
        tb = _cox(beta).proportional_hazards_test(X, y, transform=transform)
        gt = capi.zph_transform(time, status, None, transform)[0]
        ref = coxzphref.cox_zph_reference(X, [0, 1], beta, time, status, None, gt, "order",
                                          coxzphref.host_depths(n, int(status.sum())))
        tref = coxzphref.table_reference(ref)
        pref = [capi.chi2_sf(float(v), 1) for v in tref["chisq"]]
        print(transform, "chisq", tb["chisq"], "p", tb["p_value"], "reference p", pref, "global p", tb["global_p_value"])
        assert pref[0] < 1e-6 and pref[1] > 0.01  # the reference itself
        coxzphref.check_table(tb, tref, transform)
        assert tb["p_value"][0] < 1e-6 and tb["p_value"][1] > 0.01 and tb["global_p_value"] < 1e-6


def test_other_families_raise():
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = 4, np.array([1.0, 0, 0, 0]), 0.0
    with pytest.raises(ValueError, match="proportional_hazards_test is for the Cox classes, this is a Lm model"):
        lm.proportional_hazards_test(np.zeros((10, 4)), np.zeros((10, 2)))
    cox = _cox(np.array([1.0, 0, 0, 0]))
    with pytest.raises(ValueError, match="ties must be one of"):
        cox.proportional_hazards_test(np.zeros((10, 4)), np.zeros((10, 2)), ties="efron")
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 4"):
        cox.proportional_hazards_test(np.zeros((10, 5)), np.zeros((10, 2)))
    with pytest.raises(ValueError, match=r"status \(y\[:, 1\]\) should be 0 or 1"):
        cox.proportional_hazards_test(np.zeros((10, 4)), np.full((10, 2), 2.0))
    with pytest.raises(ValueError, match="transform must be one of"):
        cox.proportional_hazards_test(np.zeros((10, 4)), np.column_stack([np.arange(10.0), np.ones(10)]), transform="sqrt")


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_workspace_needs_no_device_and_is_what_the_buffers_add_up_to():
    """Scratch of a call = section 2h's (cox_info_workspace) plus, for m > 0: gp (n), three H (3 n), three v and three a
    (6 n), three weights' partials of the sweep over n rows, six (m + 1) x (m + 2) results, the staged outputs (3 m^2 +
    2 m), and with events three J-vectors of weights and three weights' partials of the sweep over J rows."""
    for n, m, J in ((1, 1, 0), (1023, 15, 700), (4097, 150, 2800), (200000, 150, 140000)):
        d, s1, s2 = capi.cox_zph_workspace(n, m, J)
        di, i1, i2 = capi.cox_info_workspace(n, m, J)
        assert (s1, s2) == (i1, i2)  # the same row splits: each weight's sums have section 2h's order
        T = ((m + 1 + 15) // 16) * ((m + 1 + 15) // 16 + 3) // 2  # tiles: TI (TI + 3) / 2
        part1 = s1[1] * T * 256
        part2 = s2[1] * T * 256
        want = di + 10 * n + 3 * part1 + 6 * (m + 1) * (m + 2) + 3 * m * m + 2 * m + (3 * J + 3 * part2 if J else 0)
        assert d == want, (n, m, J, d, want)
    # by hand: n = 1023, m = 15 is one tile row, T = 2 tiles; 1023 rows in slabs of 64 are 16 slabs, 700 in 11
    assert capi.cox_zph_workspace(1023, 15, 700)[1:] == ((64, 16), (64, 11))
    assert capi.cox_zph_workspace(10, 0, 3) == (capi.cox_info_workspace(10, 0, 3)[0], (0, 0), (0, 0))
    with pytest.raises(capi.BessxError) as e:
        capi.cox_zph_workspace(127, 1024, 3)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    for bad in ((0, 1, 0), (5, -1, 0), (5, 1, 6)):
        with pytest.raises(capi.BessxError) as e:
            capi.cox_zph_workspace(*bad)
        assert e.value.code == 1


def _input(n=8, p=4, cols=(1, 2), beta=(0.5, -0.5)):
    a = capi.CoxZphInput()
    m = len(cols)
    keep = dict(cols=np.asarray(cols, dtype=np.int32), beta=np.asarray(beta, dtype=np.float64),
                time=np.arange(n, dtype=np.float64), status=np.ones(n), gt=np.linspace(-1.0, 1.0, n),
                info0=np.zeros(m * m), info1=np.zeros(m * m), info2=np.zeros(m * m), score0=np.zeros(m), score1=np.zeros(m))
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 0x1000, 0, p, 1, n, p
    a.cols, a.m, a.beta = capi._ip(keep["cols"]), m, capi._dp(keep["beta"])
    a.time, a.status, a.ties, a.gt = capi._dp(keep["time"]), capi._dp(keep["status"]), 0, capi._dp(keep["gt"])
    for k in OUT:
        setattr(a, k, keep[k].ctypes.data)
    a.info_ld = m
    return a, keep


def _call(a):
    ll, ne = ctypes.c_double(0), ctypes.c_double(0)
    rc = capi.lib().bessx_cox_zph_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne))
    return rc, capi.last_error()


def test_abi_argument_checks_need_no_gpu():
    lib = capi.lib()
    assert lib.bessx_cox_zph_device(None, None, None) == 1 and "null" in capi.last_error()

    def change(key, i, v):
        def f(a, keep):
            keep[key][i] = v
        return f

    checks = [
        (lambda a, k: setattr(a, "x", None), 1, "null argument"),
        (lambda a, k: setattr(a, "time", None), 1, "null argument"),
        (lambda a, k: setattr(a, "status", None), 1, "null argument"),
        (lambda a, k: setattr(a, "gt", None), 1, "null argument"),
        (lambda a, k: setattr(a, "x_dtype", 7), 1, "dtype must be BESSX_F64 or BESSX_F32"),
        (lambda a, k: setattr(a, "x_row_stride", -1), 1, "strides must be non-negative"),
        (lambda a, k: setattr(a, "x_col_stride", -1), 1, "strides must be non-negative"),
        (lambda a, k: setattr(a, "n", 0), 1, "empty matrix"),
        (lambda a, k: setattr(a, "m", 5), 1, "m must lie in [0, p]"),
        (lambda a, k: setattr(a, "cols", None), 1, "null argument (cols)"),
        (lambda a, k: setattr(a, "beta", None), 1, "null argument (beta)"),
        (lambda a, k: setattr(a, "ties", 2), 1, "ties must be 0 (order) or 1 (breslow)"),
        (change("time", 3, np.nan), 1, "time holds a NaN"),
        (change("status", 2, 0.5), 1, "status must be 0 or 1"),
        (change("gt", 5, np.nan), 1, "gt must be finite at every row with status 1"),
        (change("gt", 0, np.inf), 1, "gt must be finite at every row with status 1"),
        (lambda a, k: setattr(a, "info_ld", 1), 1, "info_ld must be at least m"),
    ] + [(lambda a, k, name=name: setattr(a, name, None), 1, "null argument") for name in OUT]
    for chg, code, text in checks:
        a, keep = _input()
        chg(a, keep)
        rc, msg = _call(a)
        assert rc == code and text in msg and msg.startswith("cox_zph_device"), (rc, msg, text)
    for cols, text in (((2, 1), "cols must be ascending and distinct"), ((1, 4), "column number out of range")):
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
    assert lib.bessx_op_cox_zph_bench(None, 0, 1, 1, 1, 1, None, 0, 1, None, None) == 1
    assert lib.bessx_cox_zph_workspace(8, 2, 3, None, None, None) == 1


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_a_valid_call_without_a_gpu_is_a_hip_error_and_touches_nothing():
    a, keep = _input()
    keep["gt"][:] = np.nan  # (not read at rows without an event ...)
    keep["status"][:] = 0.0
    keep["status"][2], keep["gt"][2] = 1.0, 0.5  # (... and finite at the one event: the call is valid)
    before = capi.process_counters()
    rc, msg = _call(a)
    assert rc == 2, (rc, msg)  # BESSX_ERR_HIP
    assert not any(keep[k].any() for k in OUT) and capi.process_counters() == before


def test_python_checks_are_made_before_any_device_call():
    class Fake:  # a device array by its interface only: any device call on it would fail
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3,
                                             "strides": None}
    x, t, s, g = Fake((10, 4)), np.arange(10.0), np.ones(10), np.linspace(-1, 1, 10)
    with pytest.raises(ValueError, match="cols must be ascending and distinct"):
        capi.cox_zph_device(x, [2, 1], [0.1, 0.2], t, s, g)
    with pytest.raises(ValueError, match="beta must be 1-D"):
        capi.cox_zph_device(x, [1, 2], np.zeros((2, 2)), t, s, g)
    with pytest.raises(ValueError, match="ties must be one of"):
        capi.cox_zph_device(x, [1], [0.1], t, s, g, ties="efron")
    with pytest.raises(ValueError, match=r"X.shape\(0\) should be equal to gt.size"):
        capi.cox_zph_device(x, [1], [0.1], t, s, g[:9])
    with pytest.raises(ValueError, match="gt must be finite at every row with status 1"):
        capi.cox_zph_device(x, [1], [0.1], t, s, np.where(t == 3, np.nan, g))
    with pytest.raises(ValueError, match="status should be 0 or 1"):
        capi.cox_zph_device(x, [1], [0.1], t, s * 2, g)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        _cox(np.array([1.0, 0.0, 2.0])).proportional_hazards_test(x, np.zeros((10, 2)))
