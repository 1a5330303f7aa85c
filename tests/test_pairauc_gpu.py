"""The cumulative/dynamic AUC, Uno's C and the ROC AUC on an X already in GPU memory (bessx_cox_auc_device,
bessx_auc_device, bess_amd/csrc/bessx_k_pairauc.hip) against the O(n^2) longdouble reference of tests/pairaucref.py.
X entries are integers / 8 and B entries integers / 4, so eta is the same number under every layout and ties in eta
are exact; with censoring=None the sums must EQUAL the reference, with Kaplan-Meier weights they stay within the derived
bound (2 n + T + 8) 2^-53 (asserted below 1e-9).  Every check prints error against bound.  The shapes are the smallest
that reach every path of the kernels as built: tiles of 1024 positions (n = 1, 2, 1023, 1024, 1025, two tiles plus one,
and 3073, where a k-tile meets l-tiles that are not its neighbours), cuts inside a tile and exactly on a tile's edge,
empty segments (repeated times, a time below every row, a time at the largest), T = 0, 1, 2, 100."""
import ctypes

import numpy as np
import pytest

import coxbrierref
import pairaucref
from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
P = 24
NMAX = 3073
LAYOUTS = ["f64 row-major", "f64 column-major", "f32 row-major", "strided"]
_KEYS = {"auc", "greater", "equal", "cases", "controls", "km_drop", "mean_auc", "uno_c", "uno_concordant", "uno_tied",
         "uno_comparable", "row_a"}
_REFS = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _view(vals, layout):
    """(the n x P device view of the values in the given layout, the widened values it holds)"""
    n, p = vals.shape
    if layout == "f64 row-major":
        return _dev(vals), vals
    if layout == "f64 column-major":
        F = np.full((p, (n + 3) // 4 * 4), np.nan)
        F[:, :n] = vals.T
        return _dev(F)[:, :n].T, vals
    if layout == "f32 row-major":
        v32 = vals.astype(np.float32)
        return _dev(v32), v32.astype(np.float64)
    S = np.full((2 * n, 3 * p), np.nan)  # both strides > 1
    S[::2, 1::3] = vals
    return _dev(S)[::2, 1::3], vals


def _problem(n, m=16, R=3):
    key = ("problem", n, m, R)
    if key not in _REFS:
        X, cols, B = pairaucref.exact_problem(n, m, R, P, nmax=NMAX)
        _REFS[key] = (X, cols, B, pairaucref.eta_exact(X, cols, B))
    return _REFS[key]


def _check(gpu, t, eta, cols, B, times, time, status, w, censoring, tau, what):
    """One cox_auc_device call against the reference, its row_a against the longdouble Kaplan-Meier weights; the same
    call again gives the same bits."""
    n = time.size
    got = gpu.cox_auc_device(t, cols, B, times, time, status, weight=w, censoring=censoring, tau=tau)
    T, R = np.size(times) if times is not None else 0, np.shape(B)[1]
    assert set(got) == _KEYS and got["auc"].shape == (T, R) and got["uno_c"].shape == (R,)
    if censoring is None:
        assert np.array_equal(got["row_a"], status)
    elif isinstance(censoring, str):
        ip = coxbrierref.ipcw_reference(time, status, np.zeros(0), w)
        coxbrierref.check_ipcw(got["row_a"], np.zeros(0), ip, n, what)
    ref = pairaucref.cox_auc_reference(eta, times, time, status, w, got["row_a"], tau)
    pairaucref.check_cox_auc(got, ref, n, censoring is None, what)
    again = gpu.cox_auc_device(t, cols, B, times, time, status, weight=w, censoring=censoring, tau=tau)
    for k in _KEYS:
        assert np.array_equal(_bits(again[k]), _bits(got[k])), (what, k)
    return got, ref


def _edge_times(time):
    """Two times: one whose cut lies inside a tile, one whose cut lies exactly on the first tile's edge (n > 1024)."""
    s = np.sort(time)
    return np.array([s[min(1023, s.size - 1)], s[s.size // 3]])


# ----------------------------------------------------------------------------------------------------------------
# the shapes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049, 3073])
def test_the_tile_edges_with_every_kind_of_weight_and_censoring(gpu, n):
    X, cols, B, eta = _problem(n)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    if n <= 2:
        status = np.ones(n)
    d, rows, tiles = gpu.cox_auc_workspace(n, 2, 3)
    assert rows == pairaucref.TILE and tiles == -(-n // 1024) + 2
    t = _dev(X)
    times = _edge_times(time)
    if n > 1024:
        assert (time <= times[0]).sum() == 1024  # the cut on the tile's edge
    given = np.random.default_rng(3).integers(0, 17, NMAX)[:n] / 8.0 * status
    for wk, censoring, tau in (("none", None, None), ("eighths", None, float(np.median(time))), ("eighths", "km", None),
                               ("zeros", "km", float(np.median(time))), ("none", "km", None), ("zeros", given, None)):
        got, _ = _check(gpu, t, eta, cols, B, times, time, status, pairaucref.weights(n, wk, NMAX), censoring, tau,
                        "n=%d w=%s censoring=%s tau=%s" % (n, wk, "given" if censoring is given else censoring, tau))
        if censoring is given:
            assert np.array_equal(got["row_a"], given)


@pytest.mark.parametrize("T", [0, 1, 2, 100])
def test_the_number_of_times_with_repeats_any_order_and_empty_segments(gpu, T):
    n = 1025
    X, cols, B, eta = _problem(n)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    s = np.sort(time)
    rng = np.random.default_rng(T)
    if T == 0:
        times = None
    elif T == 1:
        times = np.array([s[1023]])  # one cut, on the tile's edge: the second tile holds one row
    elif T == 2:
        times = np.array([s[700], s[100]])  # descending
    else:
        times = np.concatenate([[0.5 * s[0], s[-1], 2.0 * s[-1], s[1023], s[1023], s[0]], rng.choice(s[1:1000], 30),
                                rng.uniform(s[0], s[-1], 64)])[rng.permutation(100)]
    for w, censoring in ((pairaucref.weights(n, "eighths", NMAX), None), (pairaucref.weights(n, "zeros", NMAX), "km")):
        got, ref = _check(gpu, t := _dev(X), eta, cols, B, times, time, status, w, censoring, None,
                          "T=%d censoring=%s" % (T, censoring))
        if T == 100:
            below, above = times < s[0], times >= s[-1]
            assert below.sum() == 1 and above.sum() == 2
            assert np.isnan(got["auc"][below | above]).all() and not np.isnan(got["auc"][~(below | above)]).any()
            assert (got["cases"][below] == 0.0).all() and (got["controls"][above] == 0.0).all()
            rep = np.nonzero(times == s[1023])[0]
            assert rep.size == 2 and np.array_equal(_bits(got["auc"][rep[0]]), _bits(got["auc"][rep[1]]))
            assert sorted(got["km_drop"][rep] > 0.0) in ([False, True], [False, False])
    if T == 2:  # the caller's order: the same numbers as the ascending call, swapped
        up = gpu.cox_auc_device(t, cols, B, times[::-1], time, status, weight=w)
        for k in ("auc", "greater", "equal", "cases", "controls", "km_drop"):
            assert np.array_equal(_bits(up[k][::-1]), _bits(got[k])), k
        assert np.array_equal(_bits(up["mean_auc"]), _bits(got["mean_auc"]))


def test_cuts_on_both_tile_edges_of_three_tiles(gpu):
    n = 2049
    X, cols, B, eta = _problem(n)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    s = np.sort(time)
    times = np.array([s[1023], s[2047]])  # segments of 1024, 1024 and 1 rows: every tile is full or a single row
    _check(gpu, _dev(X), eta, cols, B, times, time, status, None, None, None, "cuts at 1024 and 2048")
    _check(gpu, _dev(X), eta, cols, B, times, time, status, pairaucref.weights(n, "eighths", NMAX), "km", None,
           "cuts at 1024 and 2048, km")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_of_x_every_support_size_and_one_or_three_models(gpu, layout):
    n = 1025
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    y = (np.random.default_rng(8).uniform(size=NMAX) < 0.4).astype(np.float64)[:n]
    times = _edge_times(time)
    for m, R in ((0, 1), (1, 3), (16, 1), (16, 3)):
        X, cols, B, _ = _problem(n, m, R)
        t, vals = _view(X, layout)
        assert tuple(t.shape) == (n, P)
        keep = t.clone()
        eta = pairaucref.eta_exact(vals, cols, B)
        before = gpu.process_counters()
        got, _ = _check(gpu, t, eta, cols, B, times, time, status, pairaucref.weights(n, "eighths", NMAX), None, None,
                        "%s m=%d R=%d" % (layout, m, R))
        lg = gpu.auc_device(t, cols, B, y)
        after = gpu.process_counters()
        assert after["live_device_bytes"] == before["live_device_bytes"]
        assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
        assert torch.equal(t, keep)  # x is never written
        pairaucref.check_auc(lg, pairaucref.auc_reference(eta, y, None), n, True, "%s m=%d R=%d logistic" % (layout, m, R))
        if m == 0:  # every eta is 0: nothing is greater, everything ties
            assert not got["greater"].any() and (got["auc"] == 0.5).all() and (got["uno_c"] == 0.5).all()
            assert lg["auc"].tolist() == [0.5]


# ----------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------
def test_heavy_ties_in_time_with_row_times_equal_to_the_requested_times(gpu):
    n = 1500
    X, cols, B, eta = _problem(n)
    time, status = pairaucref.survival_data(n, ties=True, nmax=NMAX)
    u = np.unique(time)
    assert u.size == 20 and all(((time == v) & (status == 1)).any() and ((time == v) & (status == 0)).any() for v in u)
    times = u[::2]  # every requested time IS a row time (inclusive: those rows are cases)
    t = _dev(X)
    for wk, censoring, tau in (("none", None, None), ("zeros", "km", None), ("eighths", "km", float(u[12]))):
        _check(gpu, t, eta, cols, B, times, time, status, pairaucref.weights(n, wk, NMAX), censoring, tau,
               "ties in time w=%s censoring=%s" % (wk, censoring))


def test_heavy_ties_in_eta_from_rows_identical_on_the_support(gpu):
    n = 1500
    X, cols, B, _ = _problem(n)
    X = X.copy()
    X[:, cols] = X[np.random.default_rng(6).integers(0, 5, n)][:, cols]  # five distinct rows on the support
    eta = pairaucref.eta_exact(X, cols, B)
    assert np.unique(np.asarray(eta[:, 0], dtype=np.float64)).size <= 5
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    t = _dev(X)
    got, _ = _check(gpu, t, eta, cols, B, _edge_times(time), time, status, pairaucref.weights(n, "eighths", NMAX), None,
                    None, "ties in eta")
    assert (got["equal"] > 0).all() and (got["uno_tied"] > 0).all()
    _check(gpu, t, eta, cols, B, _edge_times(time), time, status, None, "km", None, "ties in eta, km")
    y = (np.random.default_rng(8).uniform(size=NMAX) < 0.4).astype(np.float64)[:n]
    pairaucref.check_auc(gpu.auc_device(t, cols, B, y), pairaucref.auc_reference(eta, y, None), n, True, "ties in eta")


def test_edge_rows(gpu):
    n = 1025
    X, cols, B, eta = _problem(n)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    t, times = _dev(X), _edge_times(time)
    got, _ = _check(gpu, t, eta, cols, B, times, time, np.zeros(n), None, "km", None, "every row censored")
    assert np.isnan(got["uno_c"]).all() and got["uno_comparable"] == 0.0 and np.isnan(got["auc"]).all()
    got, _ = _check(gpu, t, eta, cols, B, times, time, np.ones(n), None, "km", None, "every row an event")
    assert (got["row_a"] == 1.0).all() and got["uno_comparable"] == n * (n - 1) / 2
    w = np.ones(n)
    w[np.argsort(time)[5]] = 0.0  # a zero-weight row among the first cases
    _check(gpu, t, eta, cols, B, times, time, status, w, None, None, "a zero-weight row")
    _check(gpu, t, eta, cols, B, times, time, status, w, "km", None, "a zero-weight row, km")
    got, _ = _check(gpu, t, eta, cols, B, times, time, status, None, "km", float(time[status == 1].min()),
                    "tau at the first event")
    assert np.isnan(got["uno_c"]).all() and got["uno_comparable"] == 0.0 and not got["uno_concordant"].any()
    a = gpu.cox_auc_device(t, cols, B, times, time, status, tau=None)
    b = gpu.cox_auc_device(t, cols, B, times, time, status, tau=np.inf)
    for k in _KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("n", [1, 2, 1023, 1025, 3073])
def test_the_roc_auc_of_logistic_models(gpu, n):
    X, cols, B, eta = _problem(n)
    t = _dev(X)
    y = (np.random.default_rng(8).uniform(size=NMAX) < 0.4).astype(np.float64)[:n]
    if n == 2:
        y = np.array([1.0, 0.0])
    for wk in ("none", "eighths", "zeros"):
        w = pairaucref.weights(n, wk, NMAX)
        got = gpu.auc_device(t, cols, B, y, weight=w)
        assert set(got) == {"auc", "greater", "equal", "pos_weight", "neg_weight"} and got["auc"].shape == (3,)
        pairaucref.check_auc(got, pairaucref.auc_reference(eta, y, w), n, wk == "none", "n=%d w=%s" % (n, wk))
        again = gpu.auc_device(t, cols, B, _dev(y), weight=None if w is None else _dev(w))  # device y and weight
        for k in got:
            assert np.array_equal(_bits(again[k]), _bits(got[k])), k
    for empty in (np.ones(n), np.zeros(n)):  # one class empty
        got = gpu.auc_device(t, cols, B, empty)
        assert np.isnan(got["auc"]).all() and not got["greater"].any() and got["pos_weight"] * got["neg_weight"] == 0.0
    if n >= 1023:
        sep = (np.asarray(eta[:, 1], dtype=np.float64) > 0.0).astype(np.float64)  # perfectly separated by model 1
        got = gpu.auc_device(t, cols, B, sep)
        assert got["auc"][1] == 1.0 and got["equal"][1] == 0.0 and 0.0 < got["auc"][0] < 1.0
        assert gpu.auc_device(t, cols, B, 1.0 - sep)["auc"][1] == 0.0
        flat = gpu.auc_device(t, cols, np.zeros_like(B), y)  # every eta equal
        assert flat["auc"].tolist() == [0.5] * 3 and not flat["greater"].any()
    with pytest.raises(ValueError, match="shared by the models"):
        gpu.auc_device(t, cols, B, np.column_stack([y] * 3))


def test_unos_c_with_unit_weights_and_no_censoring_weights_is_harrells_c(gpu):
    for n, ties in ((1025, False), (1500, True)):
        X, cols, B, eta = _problem(n)
        time, status = pairaucref.survival_data(n, ties, nmax=NMAX)
        t = _dev(X)
        uno = gpu.cox_auc_device(t, cols, B, None, time, status, censoring=None, tau=None)
        har = gpu.evaluate_cox_device(t, cols, B, time, status)
        assert uno["uno_comparable"] == har["comparable"]
        assert np.array_equal(uno["uno_concordant"], har["concordant"].astype(np.float64))
        assert np.array_equal(uno["uno_tied"], har["tied_risk"].astype(np.float64))
        assert np.array_equal(_bits(uno["uno_c"]), _bits(har["c_index"]))


# ----------------------------------------------------------------------------------------------------------------
# the C ABI, the estimators, a path
# ----------------------------------------------------------------------------------------------------------------
def test_c_abi_pointer_checks_limits_ledger_and_bench(gpu):
    n, T, R = 1025, 2, 3
    X, cols, B, eta = _problem(n)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    times = np.sort(_edge_times(time))
    t = _dev(X)
    lib = gpu.lib()
    before = gpu.process_counters()
    a = gpu.CoxAucInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = X.ctypes.data, 0, P, 1, n, P  # x: a host pointer
    a.cols, a.m, a.B, a.R = gpu._ip(cols), cols.size, gpu._dp(B), R
    a.times, a.T, a.time, a.status, a.tau, a.want_uno = gpu._dp(times), T, gpu._dp(time), gpu._dp(status), float("nan"), 1
    g, e, ca, co = np.full((T, R), -7.0), np.full((T, R), -7.0), np.full(T, -7.0), np.full(T, -7.0)
    uno, comp = np.full((R, 3), -7.0), ctypes.c_double(-7.0)

    def call():
        return lib.bessx_cox_auc_device(ctypes.byref(a), gpu._dp(g), gpu._dp(e), gpu._dp(ca), gpu._dp(co), gpu._dp(uno),
                                        ctypes.byref(comp))

    assert call() == 1 and b"x" in lib.bessx_last_error()
    a.x, a.x_row_stride = t.data_ptr(), 1 << 24  # a view that reaches past its allocation
    assert call() == 1
    a.x_row_stride = P
    assert lib.bessx_cox_auc_device(None, gpu._dp(g), gpu._dp(e), gpu._dp(ca), gpu._dp(co), gpu._dp(uno),
                                    ctypes.byref(comp)) == 1
    assert lib.bessx_cox_auc_device(ctypes.byref(a), None, gpu._dp(e), gpu._dp(ca), gpu._dp(co), gpu._dp(uno),
                                    ctypes.byref(comp)) == 1 and b"null" in lib.bessx_last_error()
    assert lib.bessx_cox_auc_device(ctypes.byref(a), gpu._dp(g), gpu._dp(e), gpu._dp(ca), gpu._dp(co), None,
                                    ctypes.byref(comp)) == 1
    for field, bad, good in (("time", None, gpu._dp(time)), ("status", None, gpu._dp(status)),
                             ("times", None, gpu._dp(times)), ("T", -1, T), ("T", 1025, T), ("R", 65536, R), ("R", 0, R),
                             ("n", 0, n), ("m", P + 1, cols.size)):
        setattr(a, field, bad)
        assert call() == 1, field
        setattr(a, field, good)
    down = np.ascontiguousarray(times[::-1])
    a.times = gpu._dp(down)
    assert call() == 1 and b"decrease" in lib.bessx_last_error()
    a.times = gpu._dp(times)
    assert (g == -7.0).all() and (uno == -7.0).all() and comp.value == -7.0  # nothing was written by a refused call
    assert call() == 0, gpu.last_error()
    ref = pairaucref.cox_auc_reference(eta, times, time, status, None, status, None)
    got = {"greater": g, "equal": e, "cases": ca, "controls": co, "uno_concordant": uno[:, 0], "uno_tied": uno[:, 1],
           "uno_comparable": comp.value}
    for k, v in got.items():
        assert np.array_equal(np.asarray(v).astype(LD), ref[k]), k
    assert (uno[:, 2] == comp.value).all()
    la = gpu.AucInput()
    la.x, la.x_dtype, la.x_row_stride, la.x_col_stride, la.n, la.p = t.data_ptr(), 0, P, 1, n, P
    la.cols, la.m, la.B, la.R = gpu._ip(cols), cols.size, gpu._dp(B), R
    lg, le, pw, nw = np.full(R, -7.0), np.full(R, -7.0), ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    args = (gpu._dp(lg), gpu._dp(le), ctypes.byref(pw), ctypes.byref(nw))
    assert lib.bessx_auc_device(ctypes.byref(la), *args) == 1 and (lg == -7.0).all()  # y is null
    la.y = gpu._dp(status)
    assert lib.bessx_auc_device(ctypes.byref(la), None, *args[1:]) == 1
    la.R = 65536
    assert lib.bessx_auc_device(ctypes.byref(la), *args) == 1
    la.R = R
    assert lib.bessx_auc_device(ctypes.byref(la), *args) == 0, gpu.last_error()
    want = pairaucref.auc_reference(eta, status, None)
    assert np.array_equal(lg.astype(LD), want["greater"]) and np.array_equal(le.astype(LD), want["equal"])
    assert pw.value == status.sum() and nw.value == n - status.sum()
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
    assert after["allocation_requests"] > before["allocation_requests"]
    for R_, T_ in ((1, 1), (3, 100)):
        ms, pairs = gpu.op_pairauc_bench(t, cols, R=R_, T=T_, repeats=2)
        assert len(ms) == 4 and all(v > 0 for v in ms) and 0 < pairs <= R_ * n * (n - 1) / 2
    assert gpu.process_counters()["live_device_bytes"] == before["live_device_bytes"]


def test_the_estimators_agree_with_the_capi_route(gpu):
    n = 1025
    X, cols, B, eta = _problem(n, 16, 1)
    time, status = pairaucref.survival_data(n, nmax=NMAX)
    y = np.column_stack([time, status])
    w = pairaucref.weights(n, "eighths", NMAX)
    times = _edge_times(time)
    Xd = _dev(X)
    cox = linear.PdasCox()
    cox.p, cox.beta, cox.coef0 = P, np.zeros(P), 0.0
    cox.beta[cols] = B[:, 0]
    for wt, censoring, tau in ((None, "km", None), (w, None, float(np.median(time)))):
        got = cox.auc_survival(Xd, _dev(y), times, weight=None if wt is None else _dev(wt), censoring=censoring, tau=tau)
        direct = gpu.cox_auc_device(Xd, cols, B, times, time, status, weight=wt, censoring=censoring, tau=tau)
        assert set(got) == _KEYS and got["auc"].shape == (2,) and isinstance(got["uno_c"], float)
        for k in _KEYS:
            assert np.array_equal(_bits(got[k]).reshape(-1), _bits(direct[k]).reshape(-1)), k
        host = cox.auc_survival(X, y, times, weight=wt, censoring=censoring, tau=tau)  # the NumPy route: the same reference
        ref = pairaucref.cox_auc_reference(eta, times, time, status, wt, got["row_a"], tau)
        pairaucref.check_cox_auc(got, ref, n, censoring is None, "estimator, device")
        pairaucref.check_cox_auc(host, ref, n, censoring is None, "estimator, numpy")
    lab = (np.random.default_rng(8).uniform(size=NMAX) < 0.4).astype(np.float64)[:n]
    logit = linear.PdasLogistic()
    logit.p, logit.beta, logit.coef0 = P, cox.beta, 0.7
    for wt in (None, w):
        got = logit.auc(Xd, _dev(lab), weight=None if wt is None else _dev(wt))
        direct = gpu.auc_device(Xd, cols, B, lab, weight=wt)
        for k in got:
            assert isinstance(got[k], float) and got[k] == np.asarray(direct[k]).reshape(-1)[0], k
        ref = pairaucref.auc_reference(eta, lab, wt)
        pairaucref.check_auc(got, ref, n, wt is None, "estimator, device")
        pairaucref.check_auc(logit.auc(X, lab, weight=wt), ref, n, wt is None, "estimator, numpy")
    with pytest.raises(ValueError, match="Logistic"):
        logit.auc_survival(Xd, y)
    with pytest.raises(ValueError, match="Cox"):
        cox.auc(Xd, lab)


def _candidates(result):
    """(cols, coefficients) of every stored candidate, ascending columns."""
    out = []
    for r in range(len(result["cand_coef0"])):
        sup = result["cand_support"][r]
        sup = sup[sup >= 0]
        order = np.argsort(sup)
        out.append((sup[order], result["cand_beta"][r][:sup.size][order]))
    return out


def _separated(e64, what):
    """The precondition of a comparison on coefficients that lie on no grid: the candidate's own predictor e64 (fp64,
    from predict_device) and the predictor of the call over the union of the supports differ by a few ulp at most, so
    they order every pair alike as long as no two rows are closer than 1e-9 (and none are equal)."""
    gaps = np.diff(np.sort(e64[:, 0]))
    assert (gaps > 1e-9).all() and np.abs(e64).max() < 1e3, (what, "two rows are too close: choose another seed")


def test_candidates_of_a_cox_path_are_chosen_by_unos_c_and_by_the_mean_auc_on_held_out_rows(gpu):
    X, obs, status, _, _ = synth.make_cox(700, 30, 3, seed=76)  # (rows in time order, as the session wants them)
    pick = np.random.default_rng(2).permutation(700)
    tr, va = np.sort(pick[:400]), np.sort(pick[400:])
    with gpu.Session(X[tr], status[tr], data_type=3, model_type=4) as s:
        result = s.sequential_path(np.arange(1, 6), ic_type=3)
    R, n, T = len(result["cand_coef0"]), va.size, 8
    assert R == 5
    Xv = _dev(X[va])
    times = np.quantile(obs[va], np.linspace(0.1, 0.8, T))
    cols, Bm, _ = gpu.candidate_models(result)
    full = gpu.cox_auc_device(Xv, cols, Bm, times, obs[va], status[va])
    for by in ("uno_c", "mean_auc"):
        scores, best = gpu.cox_auc_candidates(result, Xv, obs[va], status[va], times, by=by)
        assert isinstance(scores, np.ndarray) and scores.shape == (R,) and isinstance(best, int)
        assert np.array_equal(_bits(scores), _bits(full[by]))
        want = np.zeros(R, dtype=LD)
        for r, (c, beta) in enumerate(_candidates(result)):
            e64 = gpu.predict_device(Xv, c, beta, [0.0]).cpu().numpy().reshape(-1, 1)
            _separated(e64, "candidate %d" % r)
            ref = pairaucref.cox_auc_reference(e64, times, obs[va], status[va], None, full["row_a"], None)
            want[r] = ref["uno_c"][0] if by == "uno_c" else pairaucref.mean_auc_reference(ref["auc"], full["km_drop"], None)[0]
        rel = pairaucref.uno_rel(n) if by == "uno_c" else pairaucref.auc_rel(n, T) + LD(2 * T + 3) * pairaucref.U
        err = np.abs(scores.astype(LD) - want)
        print(by, scores, "largest err %.3e against bound %.3e" % (float(err.max()), float((rel * want).max())))
        assert (err <= rel * want).all()
        two = np.sort(want)[-2:]
        assert two[1] - two[0] > 100 * rel, "the two best candidates are too close for this seed"
        assert best == int(np.argmax(want))


def test_candidates_of_a_logistic_path_are_chosen_by_roc_auc_on_held_out_rows(gpu):
    X, y, _, _ = synth.make_logistic(700, 30, 3, seed=5)
    pick = np.random.default_rng(2).permutation(700)
    tr, va = np.sort(pick[:400]), np.sort(pick[400:])
    with gpu.Session(X[tr], y[tr], data_type=2, model_type=2) as s:
        result = s.sequential_path(np.arange(1, 6), ic_type=3)
    R, n = len(result["cand_coef0"]), va.size
    assert R == 5
    Xv = _dev(X[va])
    scores, best = gpu.auc_candidates(result, Xv, y[va])
    assert isinstance(scores, np.ndarray) and scores.shape == (R,) and isinstance(best, int)
    want = np.zeros(R, dtype=LD)
    for r, (c, beta) in enumerate(_candidates(result)):
        e64 = gpu.predict_device(Xv, c, beta, [0.0]).cpu().numpy().reshape(-1, 1)
        _separated(e64, "candidate %d" % r)
        want[r] = pairaucref.auc_reference(e64, y[va], None)["auc"][0]
    err, rel = np.abs(scores.astype(LD) - want), pairaucref.auc_rel(n, 1)
    print(scores, "largest err %.3e against bound %.3e" % (float(err.max()), float((rel * want).max())))
    assert (err <= rel * want).all()
    two = np.sort(want)[-2:]
    assert two[1] - two[0] > 100 * rel, "the two best candidates are too close for this seed"
    assert best == int(np.argmax(want))
