"""The cumulative/dynamic AUC, Uno's C and the ROC AUC without a GPU: the fp64 NumPy route of bess_base.auc_survival /
auc (capi._cox_auc_host / _auc_host) against the longdouble reference of tests/pairaucref.py -- the sums EQUAL it where
every term lies on the 1/64 grid, and stay within the derived bound (2 n + T + 8) 2^-53 otherwise -- the argument
checks, and the workspace query.  Every check prints error against bound."""
import numpy as np
import pytest

import coxbrierref
import pairaucref
from bess_amd import capi, linear

LD = np.longdouble
P = 24
NMAX = 1025
_KEYS = {"auc", "greater", "equal", "cases", "controls", "km_drop", "mean_auc", "uno_c", "uno_concordant", "uno_tied",
         "uno_comparable", "row_a"}


def _est(cls, cols, beta):
    est = cls()
    est.p = P
    est.beta = np.zeros(P)
    est.beta[cols] = beta
    est.coef0 = 0.0
    return est


def _times(time, T, seed=0):
    """T requested times, NOT sorted, with a repeat: below the smallest row time, equal to row times, between them, at
    the largest row time."""
    u = np.unique(time)
    rng = np.random.default_rng(seed + T)
    if T == 0:
        return np.zeros(0)
    if T == 1:
        return np.array([u[u.size // 2]])
    t = np.concatenate([[0.5 * u[0], u[-1]], rng.choice(u, T // 2), rng.uniform(u[0], u[-1], T)])[:T]
    t[-1] = t[0] if T < 3 else t[2]
    return t[rng.permutation(T)] if T > 2 else t


def test_the_reference_agrees_with_a_double_loop_over_the_pairs():
    assert pairaucref.self_check()


@pytest.mark.parametrize("n", [1, 2, 300, 1025])
def test_the_numpy_route_of_auc_survival_against_the_reference(n):
    X, cols, B = pairaucref.exact_problem(n, 7, 1, P, nmax=NMAX)
    eta = pairaucref.eta_exact(X, cols, B)
    est = _est(linear.PdasCox, cols, B[:, 0])
    for ties in (False, True):
        time, status = pairaucref.survival_data(n, ties, nmax=NMAX)
        y = np.column_stack([time, status])
        for wk in ("none", "eighths", "zeros"):
            w = pairaucref.weights(n, wk, NMAX)
            for T in (0, 2, 9):
                times = _times(time, T)
                for censoring, tau in ((None, None), ("km", None), ("km", float(np.median(time)))):
                    what = "n=%d ties=%s w=%s T=%d censoring=%s tau=%s" % (n, ties, wk, T, censoring, tau)
                    got = est.auc_survival(X, y, times, weight=w, censoring=censoring, tau=tau)
                    assert set(got) == _KEYS and got["auc"].shape == (T,) and isinstance(got["uno_c"], float)
                    if censoring is None:
                        assert np.array_equal(got["row_a"], status)
                    else:
                        ip = coxbrierref.ipcw_reference(time, status, np.zeros(0), w)
                        coxbrierref.check_ipcw(got["row_a"], np.zeros(0), ip, n, what)
                    ref = pairaucref.cox_auc_reference(eta, times, time, status, w, got["row_a"], tau)
                    pairaucref.check_cox_auc(got, ref, n, censoring is None, what)


def test_times_without_cases_or_without_controls_give_nan_and_do_not_enter_the_mean():
    n = 300
    X, cols, B = pairaucref.exact_problem(n, 7, 1, P, nmax=NMAX)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    est = _est(linear.PdasCox, cols, B[:, 0])
    times = np.array([time.max(), np.median(time), 0.5 * time.min(), np.median(time)])
    got = est.auc_survival(X, np.column_stack([time, status]), times, censoring=None)
    assert np.isnan(got["auc"][[0, 2]]).all() and got["auc"][1] == got["auc"][3] and 0.0 < got["auc"][1] < 1.0
    assert got["controls"][0] == 0.0 and got["cases"][2] == 0.0
    assert got["km_drop"][2] == 0.0 and got["km_drop"][3] == 0.0 and got["km_drop"][1] > 0.0  # (the repeat drops nothing)
    if status[np.argmax(time)] == 1:  # the last drop belongs to a time without controls: the mean is NaN
        assert got["km_drop"][0] > 0.0 and np.isnan(got["mean_auc"])
    two = est.auc_survival(X, np.column_stack([time, status]), times[1:], censoring=None)
    # one time with a positive drop: the mean is its auc, times d and over d (two roundings)
    assert abs(two["mean_auc"] - two["auc"][0]) <= 2 * np.spacing(two["auc"][0])
    none = est.auc_survival(X, np.column_stack([time, status]))
    assert none["auc"].shape == (0,) and np.isnan(none["mean_auc"]) and 0.0 < none["uno_c"] < 1.0


def test_edge_rows_of_unos_c():
    n = 300
    X, cols, B = pairaucref.exact_problem(n, 7, 1, P, nmax=NMAX)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    est = _est(linear.PdasCox, cols, B[:, 0])
    t1 = np.array([np.median(time)])
    got = est.auc_survival(X, np.column_stack([time, np.zeros(n)]), t1)  # every row censored
    assert np.isnan(got["uno_c"]) and got["uno_comparable"] == 0.0 and np.isnan(got["auc"][0]) and not got["row_a"].any()
    got = est.auc_survival(X, np.column_stack([time, np.ones(n)]), t1)  # every row an event: G = 1, a = 1
    assert (got["row_a"] == 1.0).all() and got["uno_comparable"] == n * (n - 1) / 2
    y = np.column_stack([time, status])
    below = est.auc_survival(X, y, t1, tau=time[status == 1].min())  # tau at the first event: no pair is left
    assert np.isnan(below["uno_c"]) and below["uno_comparable"] == 0.0
    a, b = est.auc_survival(X, y, t1, tau=None), est.auc_survival(X, y, t1, tau=np.inf)
    for k in ("uno_c", "uno_concordant", "uno_tied", "uno_comparable"):
        assert a[k] == b[k], k
    given = np.random.default_rng(3).uniform(0.0, 2.0, n) * status
    for cens in (given, (given, np.ones(1))):
        got = est.auc_survival(X, y, t1, censoring=cens)
        assert np.array_equal(got["row_a"], given)


@pytest.mark.parametrize("n", [1, 2, 300, 1025])
def test_the_numpy_route_of_auc_against_the_reference(n):
    X, cols, B = pairaucref.exact_problem(n, 7, 1, P, nmax=NMAX)
    eta = pairaucref.eta_exact(X, cols, B)
    est = _est(linear.PdasLogistic, cols, B[:, 0])
    y = (np.random.default_rng(8).uniform(size=NMAX) < 0.4).astype(np.float64)[:n]
    for wk in ("none", "eighths", "zeros"):
        w = pairaucref.weights(n, wk, NMAX)
        got = est.auc(X, y, weight=w)
        assert set(got) == {"auc", "greater", "equal", "pos_weight", "neg_weight"}
        assert all(isinstance(v, float) for v in got.values())
        pairaucref.check_auc(got, pairaucref.auc_reference(eta, y, w), n, wk == "none", "n=%d w=%s" % (n, wk))
    assert np.isnan(est.auc(X, np.ones(n))["auc"]) and np.isnan(est.auc(X, np.zeros(n))["auc"])  # a class is empty
    if n >= 300:
        sep = (np.asarray(eta[:, 0], dtype=np.float64) > 0.0).astype(np.float64)
        assert est.auc(X, sep)["auc"] == 1.0 and est.auc(X, 1.0 - sep)["auc"] == 0.0  # perfectly separated
        flat = _est(linear.PdasLogistic, cols, np.zeros(7))
        assert flat.auc(X, y)["auc"] == 0.5 and flat.auc(X, y)["greater"] == 0.0  # every eta equal


def test_argument_checks():
    n = 50
    X, cols, B = pairaucref.exact_problem(n, 3, 1, P)
    time, status = pairaucref.survival_data(n)
    y = np.column_stack([time, status])
    cox, logit = _est(linear.PdasCox, cols, B[:, 0]), _est(linear.PdasLogistic, cols, B[:, 0])
    lm = _est(linear.PdasLm, cols, B[:, 0])
    with pytest.raises(ValueError, match="Logistic"):
        logit.auc_survival(X, y)
    with pytest.raises(ValueError, match="Cox"):
        cox.auc(X, status)
    with pytest.raises(ValueError, match="Lm"):
        lm.auc(X, status)
    with pytest.raises(ValueError, match="Lm"):
        lm.auc_survival(X, y)
    with pytest.raises(ValueError, match="shared by the models"):
        logit.auc(X, np.column_stack([status, status]))
    with pytest.raises(ValueError, match="y"):
        logit.auc(X, status[:-1])
    with pytest.raises(ValueError, match="NAN"):
        logit.auc(X, np.where(np.arange(n) == 3, np.nan, status))
    bad = y.copy()
    bad[4, 0] = np.nan
    with pytest.raises(ValueError, match="NAN"):
        cox.auc_survival(X, bad)
    with pytest.raises(ValueError, match="non-negative"):
        cox.auc_survival(X, y, weight=-np.ones(n))
    with pytest.raises(ValueError, match="non-negative"):
        logit.auc(X, status, weight=-np.ones(n))
    with pytest.raises(ValueError, match="censoring"):
        cox.auc_survival(X, y, censoring="kaplan")
    with pytest.raises(ValueError, match="censoring"):
        cox.auc_survival(X, y, censoring=np.ones(n - 1))
    with pytest.raises(ValueError, match="censoring"):
        cox.auc_survival(X, y, censoring=-np.ones(n))
    with pytest.raises(ValueError, match="NAN"):
        cox.auc_survival(X, y, times=[1.0, np.nan])
    with pytest.raises(ValueError, match="1-D"):
        cox.auc_survival(X, y, times=np.ones((2, 2)))
    with pytest.raises(ValueError, match="at most 1024"):
        cox.auc_survival(X, y, times=np.linspace(0.1, 1.0, 1025))
    with pytest.raises(ValueError, match="tau"):
        cox.auc_survival(X, y, tau=np.nan)
    with pytest.raises(ValueError, match="X.shape"):
        cox.auc_survival(X[:, :5], y)
    with pytest.raises(ValueError, match="by must be"):
        capi.cox_auc_candidates({}, None, time, status, by="harrell")


def test_the_workspace_query_needs_no_device():
    d, rows, tiles = capi.cox_auc_workspace(200000, 100, 150)
    assert rows == 1024 and tiles == 196 + 100
    assert d == 150 * 200000 + 3 * 200000 + 2 * 150 * tiles * 101 + 2 * 150 * 101 + (3 * 200000 + 3 * tiles + 205) // 2
    assert d * 8 < 1 << 30  # (nothing n x T x R: that alone would be 24 GB)
    assert capi.cox_auc_workspace(1, 0, 1)[1:] == (1024, 1)
    for n, T, R in ((0, 1, 1), (10, -1, 1), (10, 1025, 1), (10, 1, 0), (10, 1, 65536)):
        with pytest.raises(capi.BessxError):
            capi.cox_auc_workspace(n, T, R)


def test_against_scikit_survival_on_data_without_ties():
    metrics = pytest.importorskip("sksurv.metrics")
    n = 400
    rng = np.random.default_rng(4)
    eta = rng.standard_normal(n)  # (continuous: no ties in eta, none in time)
    time = rng.exponential(np.exp(-eta)) + 0.01
    cens = rng.exponential(2.0, n) + 0.01
    status = (time <= cens).astype(np.float64)
    obs = np.minimum(time, cens)
    sy = np.array(list(zip(status.astype(bool), obs)), dtype=[("e", bool), ("t", float)])
    times = np.quantile(obs, [0.2, 0.4, 0.6])
    got = capi._cox_auc_host(eta.reshape(-1, 1), times, obs, status, np.ones(n), "km", float(times[-1]))
    auc, mean = metrics.cumulative_dynamic_auc(sy, sy, eta, times)
    assert np.allclose(got["auc"][:, 0], auc, rtol=1e-10) and np.isclose(got["mean_auc"][0], mean, rtol=1e-10)
    assert np.isclose(got["uno_c"][0], metrics.concordance_index_ipcw(sy, sy, eta, tau=float(times[-1]))[0], rtol=1e-10)
