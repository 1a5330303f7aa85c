"""The IPCW Brier score of Cox models (bessx_cox_brier_device, capi.cox_brier_device / ipcw_weights / censoring_km /
integrated_brier / cox_brier_candidates, bess_base.brier_survival): what needs no GPU -- the entry points are exported,
declared and listed, bad arguments raise ValueError before the library is asked for a device, the C entries refuse to
compute without a GPU, the weights and the integral have their properties, and the NumPy route is inside the derived bound
(tests/coxbrierref.py) of the longdouble reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coxbrierref
import evalref
from bess_amd import capi, linear, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_cox_brier_device", "bessx_cox_brier_workspace", "bessx_op_cox_brier_bench")
LD = np.longdouble
U = evalref.U


class FakeDevice:
    """Stand-in for a device array: only the attribute capi looks at.  The pointer is never dereferenced."""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=1 << 20):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False),
                                         "strides": strides, "version": 3}


def _no_library():
    raise AssertionError("the library was asked before the argument check")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _fitted(cls=linear.PdasCox, p=5, baseline=True):
    est = cls()
    est.p = p
    est.beta = np.array([0.0, 1.5, 0.0, -2.0, 0.0])[:p]
    est.coef0 = 0.0 if cls is linear.PdasCox else 0.25
    if baseline:
        est.baseline_times_, est.baseline_cumhaz_ = np.array([1.0, 2.0]), np.array([0.25, 0.5])
    return est


def test_new_symbols_are_exported_declared_and_listed():
    assert all(n in capi.SYMBOLS for n in NEW)
    lib = os.path.join(ROOT, "bess_amd", "libbessx.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(bessx_\w+)\b", out))
    header = open(os.path.join(ROOT, "include", "bessx.h")).read()
    for n in NEW:
        assert n in exported, n
        assert re.search(r"\bint %s\(" % n, header), n
        assert getattr(capi.lib(), n).argtypes is not None, n
    assert "bessx_cox_brier_input" in header
    for f in ("CoxBrierInput", "censoring_km", "ipcw_weights", "cox_brier_device", "integrated_brier",
              "cox_brier_workspace", "op_cox_brier_bench", "cox_brier_candidates"):
        assert callable(getattr(capi, f)), f
    assert callable(linear.bess_base.brier_survival) and callable(linear.bess_base._brier_host)


def test_the_workspace_holds_nothing_n_by_t():
    doubles, rows, slabs, groups = capi.cox_brier_workspace(200000, 100, 150)
    assert (rows, slabs, groups) == (coxbrierref.SLAB_ROWS, 196, coxbrierref.row_groups(100)) and groups == 2
    assert doubles == 3 * 200000 + 150 * 200000 + 196 * 150 * 100 + 2 * 150 * 100 + 2 * 100
    assert doubles < 200000 * 100 * 2  # far below ONE model's n x T matrix times two, for all 150 models
    for T in (1, 2, 3, 100, 128, 129, 256, 4096):
        assert capi.cox_brier_workspace(5, T, 1)[3] == coxbrierref.row_groups(T)
    assert capi.cox_brier_workspace(2 ** 31 - 1, 4096, 1024)[2] == (2 ** 31 - 1 + 1023) // 1024
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0), (5, 1, 65536), (5, (1 << 20) + 1, 1)):
        with pytest.raises(capi.BessxError) as e:
            capi.cox_brier_workspace(*bad)
        assert e.value.code == 1


# ----------------------------------------------------------------------------------------------------------------
# the reference itself
# ----------------------------------------------------------------------------------------------------------------
def test_the_reference_agrees_with_the_brute_force_statement_and_the_identities():
    assert coxbrierref.self_check()


# ----------------------------------------------------------------------------------------------------------------
# the weights and the integral
# ----------------------------------------------------------------------------------------------------------------
def _survival_rows(n, seed, decimals=None, events=0.6):
    rng = np.random.default_rng(seed)
    time = rng.exponential(1.0, n) + 0.05
    if decimals is not None:
        time = np.round(time, decimals) + 0.1
    status = (rng.uniform(size=n) < events).astype(np.float64)
    return time, status


def _weights(n, kind):
    if kind == "none":
        return None
    w = np.random.default_rng(5).integers(1, 17, n) / 8.0
    if kind == "zeros":
        w[::3] = 0.0
    return w


def _grid(time, status, w, rng, extra=()):
    """Ascending times: before the first row time, equal to some row times, between them, and the last admissible one."""
    u = np.unique(time)
    last_censored = bool(((time == u[-1]) & (status == 0) & ((w if w is not None else 1.0) * np.ones(time.size) > 0)).any())
    last = np.nextafter(u[-1], -np.inf) if last_censored else u[-1]
    g = np.concatenate([[0.5 * u[0]], rng.choice(u[:-1], min(4, u.size - 1), replace=False),
                        rng.uniform(u[0], u[-1], 3), list(extra), [last]])
    g = np.unique(g[g <= last])
    return g, last, last_censored


@pytest.mark.parametrize("wk", ["none", "eighths", "zeros"])
@pytest.mark.parametrize("decimals", [None, 1])
def test_censoring_km_and_ipcw_weights_against_the_product_definition(decimals, wk):
    n = 257
    time, status = _survival_rows(n, 31, decimals)
    w = _weights(n, wk)
    times, last, last_censored = _grid(time, status, w, np.random.default_rng(2))
    ref = coxbrierref.ipcw_reference(time, status, times, w)
    a, b = capi.ipcw_weights(time, status, times, weight=w)
    coxbrierref.check_ipcw(a, b, ref, n, "ipcw n=%d decimals=%s w=%s" % (n, decimals, wk))
    assert (a[status == 0] == 0).all() and (w is None or (a[w == 0] == 0).all()) and (b >= 1.0).all()
    u, G = capi.censoring_km(time, status, weight=w)
    assert np.array_equal(u, np.unique(time)) and (np.diff(G) <= 0).all() and (G <= 1.0).all() and (G >= 0.0).all()
    assert (np.abs(G.astype(LD) - ref["G"][1]) <= coxbrierref.ipcw_bound(n, n) * ref["G"][1]).all()
    assert np.array_equal(1.0 / capi._step_at(u, G, times), b)
    # the IPCW identity on the fp64 weights: the two masses add up to W at every time
    wl = np.ones(n) if w is None else w
    for j, t in enumerate(times):
        tot = float(np.sum((wl * a)[time <= t]) + b[j] * np.sum(wl[time > t]))
        assert abs(tot - wl.sum()) <= float(coxbrierref.ipcw_bound(n, n)) * 4 * wl.sum(), (j, tot)
    if last_censored:
        assert G[-1] == 0.0
        with pytest.raises(ValueError, match=re.escape(repr(float(last)))):
            capi.ipcw_weights(time, status, [times[0], np.unique(time)[-1]], weight=w)
    a1, b1 = capi.ipcw_weights(time, status, times, weight=w, censoring=None)
    assert np.array_equal(a1, status) and np.array_equal(b1, np.ones(times.size))
    a2, b2 = capi.ipcw_weights(time, status, times, weight=w, censoring=(a, b))
    assert np.array_equal(a2, a) and np.array_equal(b2, b)


def test_g_reaches_zero_only_when_the_last_time_is_censored():
    time, status = np.array([1.0, 2.0, 3.0, 3.0]), np.array([1.0, 0.0, 1.0, 0.0])
    u, G = capi.censoring_km(time, status)
    assert np.array_equal(u, [1.0, 2.0, 3.0]) and np.array_equal(G, [1.0, 2.0 / 3.0, 0.0])  # (the event at 3 leaves first)
    a, b = capi.ipcw_weights(time, status, [0.5, 2.0, np.nextafter(3.0, 0.0)])
    assert np.array_equal(a, [1.0, 0.0, 1.5, 0.0]) and np.array_equal(b, [1.0, 1.5, 1.5])
    with pytest.raises(ValueError, match="largest admissible time is %s" % re.escape(repr(float(np.nextafter(3.0, 0.0))))):
        capi.ipcw_weights(time, status, [3.0])
    a, b = capi.ipcw_weights(time, np.array([1.0, 0.0, 1.0, 1.0]), [3.0, 99.0])  # the last time holds events only
    assert np.array_equal(b, [1.5, 1.5])


def test_integrated_brier_on_a_known_piecewise_linear_curve():
    t = np.array([1.0, 2.0, 4.0, 4.5])
    bs = np.array([0.0, 0.5, 0.25, 0.25])  # areas 0.25 + 0.75 + 0.125 = 1.125 over 3.5
    assert capi.integrated_brier(t, bs) == 1.125 / 3.5
    both = capi.integrated_brier(t, np.column_stack([bs, 2.0 * bs]))
    assert both.shape == (2,) and both[0] == 1.125 / 3.5 and both[1] == 2.25 / 3.5
    assert capi.integrated_brier([0.0, 8.0], [0.125, 0.125]) == 0.125  # a constant curve integrates to itself
    for bad, msg in (([1.0], "at least 2"), ([], "at least 2"), ([1.0, 1.0, 2.0], "strictly increasing"),
                     ([2.0, 1.0], "strictly increasing"), ([1.0, np.nan], "NAN")):
        with pytest.raises(ValueError, match=msg):
            capi.integrated_brier(bad, np.zeros(len(bad)))
    with pytest.raises(ValueError, match="bs must have shape"):
        capi.integrated_brier(t, np.zeros(3))


# ----------------------------------------------------------------------------------------------------------------
# the NumPy route against the longdouble reference
# ----------------------------------------------------------------------------------------------------------------
def _cox_problem(n, p, m, seed, decimals=None):
    X, obs, status, _, _ = synth.make_cox(n, p, 3, seed=seed)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    X, obs, status = np.ascontiguousarray(X[perm]), obs[perm], status[perm]
    if decimals is not None:
        obs = np.round(obs, decimals) + 0.1
    est = linear.PdasCox()
    est.p, est.coef0 = p, 0.0
    est.beta = np.zeros(p)
    est.beta[rng.choice(p, m, replace=False)] = rng.normal(0.0, 0.5, m)
    return est, X, obs, status


def _null_tolerance(n, k, time, times, w, a, b):
    """|BS_null - reference|: the Kaplan-Meier survival carries k factors of relative error 2 gamma_n + 3 u each, it enters
    squared, (1 - S)^2 moves by 2 (1 - S) S eps at most, and the two sums are gamma_n each: together at most
    (2 k (2 gamma_n + 3 u) + 4 gamma_n + 16 u) times the two masses over W."""
    wl = np.ones(n) if w is None else w
    mass = np.array([np.sum((wl * a)[time <= t]) + b[j] * np.sum(wl[time > t]) for j, t in enumerate(times)]) / wl.sum()
    g = evalref.gamma(n)
    return (LD(2 * k) * (2 * g + 3 * U) + 4 * g + 16 * U) * mass.astype(LD)


@pytest.mark.parametrize("wk", ["none", "eighths", "zeros"])
@pytest.mark.parametrize("decimals", [None, 1])
@pytest.mark.parametrize("censoring", ["km", None, "given"])
def test_numpy_route_is_inside_the_bound(censoring, decimals, wk, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)  # (a NumPy X never touches the library)
    n = 513
    est, X, time, status = _cox_problem(n, 16, 3, seed=84, decimals=decimals)
    w = _weights(n, wk)
    y = np.column_stack([time, status])
    cols = np.nonzero(est.beta)[0]
    eta, delta = evalref.eta_reference(X, cols, est.beta[cols].reshape(-1, 1), [0.0])
    assert float(np.abs(eta).max()) <= 5.0
    est.fit_baseline(X, y, weight=w)
    # (times equal to row times are in the grid: some row has time_i == t_j, and with decimals many do)
    times, last, last_censored = _grid(time, status, w, np.random.default_rng(1), extra=est.baseline_times_[:3])
    assert np.isin(times, time).sum() >= 3 and times[0] < time.min() and times[-1] == last
    if decimals is not None:
        assert np.unique(time).size < 0.9 * n
    cens = censoring
    if censoring == "given":
        cens = (np.random.default_rng(3).uniform(0.0, 2.0, n) * status, np.linspace(1.0, 3.0, times.size))
    what = "numpy n=%d censoring=%s decimals=%s w=%s" % (n, censoring, decimals, wk)
    got = est.brier_survival(X, y, times, weight=w, censoring=cens)
    assert set(got) == {"brier", "null", "ipa", "ibs", "ibs_null", "row_a", "time_b", "sum_w"}
    T = times.size
    assert got["brier"].shape == (T,) and got["null"].shape == (T,) and got["ipa"].shape == (T,)
    assert isinstance(got["ibs"], float) and isinstance(got["ibs_null"], float)
    assert got["sum_w"] == (n if w is None else float(w.sum()))
    a, b = got["row_a"], got["time_b"]
    if censoring == "km":
        coxbrierref.check_ipcw(a, b, coxbrierref.ipcw_reference(time, status, times, w), n, what)
    elif censoring is None:
        assert np.array_equal(a, status) and np.array_equal(b, np.ones(T))
    else:
        assert np.array_equal(a, cens[0]) and np.array_equal(b, cens[1])
    hg = capi.baseline_at(est.baseline_times_, est.baseline_cumhaz_, times).reshape(-1, 1)
    assert hg[0, 0] == 0.0 and hg[-1, 0] > 0.0
    ref = coxbrierref.brier_reference(eta, delta, hg, times, time, w, a, b, n, what)
    coxbrierref.check_brier(got["brier"].reshape(-1, 1), ref, what)
    # the bound is not slack: a relative change of 1e-9 falls outside
    exact = ref["value"][:, 0].astype(np.float64)
    assert (np.abs((exact * (1 + 1e-9)).astype(LD) - ref["value"][:, 0]) > ref["bound"][:, 0])[exact > 0].all()
    # hg = 0 at the first time: the weighted fraction that has left, exactly
    wl = np.ones(n) if w is None else w
    assert got["brier"][0] == float(np.sum((wl * a)[time <= times[0]]) / wl.sum()) == 0.0
    null = coxbrierref.null_reference(time, status, w, times, a, b)
    k = int(np.unique(time[status != 0]).size)
    assert (np.abs(got["null"].astype(LD) - null) <= _null_tolerance(n, k, time, times, w, a, b)).all(), what
    with np.errstate(invalid="ignore", divide="ignore"):
        ipa = np.where(got["null"] > 0, 1.0 - got["brier"] / got["null"], np.nan)
    assert np.array_equal(got["ipa"], ipa, equal_nan=True) and np.isnan(got["ipa"][0]) and got["null"][0] == 0.0
    assert got["ibs"] == float(capi.integrated_brier(times, got["brier"]))
    assert got["ibs_null"] == float(capi.integrated_brier(times, got["null"]))
    assert 0.0 < got["ibs"] < 1.0 and 0.0 < got["ibs_null"] < 1.0
    # one time, and times in any order with repeats: the same scores (each inside its bound), no integral
    for pick in ([3], [2, 0, 2]):
        sub = est.brier_survival(X, y, times[pick], weight=w,
                                 censoring=cens if censoring != "given" else (cens[0], cens[1][pick]))
        assert sub["brier"].shape == (len(pick),) and np.isnan(sub["ibs"]) and np.isnan(sub["ibs_null"])
        assert (np.abs(sub["brier"].astype(LD) - ref["value"][pick, 0]) <= ref["bound"][pick, 0]).all()


def test_the_known_answer(monkeypatch):
    """Times (1, 2, 3, 4), every row an event, no support column and H0(2.5) = log 2: S = 1 / 2 for every row, two rows
    have left and two have not, so BS = (2 * 1/4 + 2 * 1/4) / 4 = 1/4; G = 1 throughout."""
    monkeypatch.setattr(capi, "lib", _no_library)
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = 3, np.zeros(3), 0.0
    est.baseline_times_, est.baseline_cumhaz_ = np.array([2.0]), np.array([np.log(2.0)])
    y = np.column_stack([[1.0, 2.0, 3.0, 4.0], np.ones(4)])
    got = est.brier_survival(np.zeros((4, 3)), y, [0.5, 2.5])
    assert np.array_equal(got["row_a"], np.ones(4)) and np.array_equal(got["time_b"], np.ones(2))
    assert got["brier"][0] == 0.0 and abs(got["brier"][1] - 0.25) <= 4 * float(U)
    # the null model: S^(2.5) = 1/2 as well, so IPA = 0 to rounding
    assert abs(got["null"][1] - 0.25) <= 4 * float(U) and abs(got["ipa"][1]) <= 32 * float(U)
    assert abs(got["ibs"] - 0.125) <= 4 * float(U)


# ----------------------------------------------------------------------------------------------------------------
# the candidates' rule
# ----------------------------------------------------------------------------------------------------------------
def test_cox_brier_candidates_takes_the_lowest_index_among_the_smallest_and_a_nan_never_wins(monkeypatch):
    result = {"cand_support": np.array([[1, -1], [1, 3], [0, 3], [2, -1]]),
              "cand_beta": np.array([[0.5, 0.0], [0.25, -1.0], [2.0, 1.0], [1.0, 0.0]]), "cand_coef0": np.zeros(4)}
    calls = {"baseline": [], "brier": 0}

    def baseline(x, cols, B, time, status, weight=None, stream=0):
        calls["baseline"].append((list(cols), list(B)))
        return {"times": np.array([1.0, 2.0]), "cumhaz": np.array([0.5, 1.0]) * len(calls["baseline"]), "n_events": 2.0}

    def brier(fab):
        def f(x, cols, B, hg, times, time, status, weight=None, censoring="km", stream=0):
            calls["brier"] += 1
            assert x == "val" and list(cols) == [0, 1, 2, 3] and B.shape == (4, 4) and hg.shape == (3, 4)
            assert np.array_equal(hg[:, 2], [0.0, 1.5, 3.0]) and censoring is None and weight == "wv"
            return {"ibs": np.array(fab)}
        return f

    monkeypatch.setattr(capi, "lib", _no_library)
    monkeypatch.setattr(capi, "cox_baseline_device", baseline)
    for fab, best in (([0.3, 0.2, 0.2, 0.25], 1), ([np.nan, 0.4, 0.1, 0.1], 2), ([np.nan, np.nan, np.nan, 0.5], 3),
                      ([0.1, 0.1, 0.1, 0.1], 0)):
        monkeypatch.setattr(capi, "cox_brier_device", brier(fab))
        calls["baseline"] = []
        ibs, got = capi.cox_brier_candidates(result, "train", "tt", "st", "val", "tv", "sv", [0.5, 1.0, 2.5],
                                             weight_train="wt", weight_val="wv", censoring=None)
        assert got == best and np.array_equal(ibs, fab, equal_nan=True)
        assert calls["baseline"] == [([1], [0.5]), ([1, 3], [0.25, -1.0]), ([0, 3], [2.0, 1.0]), ([2], [1.0])]
    assert calls["brier"] == 4  # ONE call per path
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            capi.cox_brier_candidates(result, "train", "tt", "st", "val", "tv", "sv", bad)


# ----------------------------------------------------------------------------------------------------------------
# argument errors, before the library is asked for anything
# ----------------------------------------------------------------------------------------------------------------
_Y = np.column_stack([np.arange(1.0, 31.0), np.tile([1.0, 1.0, 0.0], 10)])
_NAN_Y = _Y.copy()
_NAN_Y[7, 0] = np.nan
BAD_EST = [
    (dict(times=[]), "empty"),
    (dict(times=np.zeros((2, 2))), "1-D"),
    (dict(times=[1.0, np.nan]), "NAN"),
    (dict(y=_NAN_Y), "NAN"),
    (dict(y=np.zeros(30)), r"\(30, 2\)"),
    (dict(y=np.column_stack([np.arange(30.0), np.full(30, 2.0)])), "0 or 1"),
    (dict(weight=np.ones(31)), r"weight\.size"),
    (dict(weight=np.where(np.arange(30) == 3, -1.0, 1.0)), "non-negative"),
    (dict(weight=np.zeros(30)), "sum to 0"),
    (dict(times=[1.0, 30.0]), "largest admissible time"),  # the last row is censored: G(30) = 0
    (dict(censoring="nelson"), "censoring"),
    (dict(censoring=3.5), "censoring"),
    (dict(censoring=(np.ones(30),)), "censoring"),
    (dict(censoring=(np.ones(29), np.ones(2))), "n = 30 and T = 2"),
    (dict(censoring=(np.ones(30), np.ones(3))), "n = 30 and T = 2"),
    (dict(censoring=(-np.ones(30), np.ones(2))), "row_a must be finite"),
    (dict(censoring=(np.ones(30), np.array([1.0, np.inf]))), "time_b must be finite"),
]


@pytest.mark.parametrize("kw,msg", BAD_EST)
def test_brier_survival_rejects_bad_arguments_before_any_device_call(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for X in (FakeDevice((30, 5)), np.zeros((30, 5))):
        args = dict(y=_Y, times=[1.5, 2.5])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            _fitted().brier_survival(X, **args)


def test_other_families_a_missing_baseline_a_negative_hazard_and_a_bad_x(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for X in (np.zeros((30, 5)), FakeDevice((30, 5))):
        for cls in (linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson):
            with pytest.raises(ValueError, match="Cox"):
                _fitted(cls).brier_survival(X, _Y, [1.5, 2.5])
        with pytest.raises(ValueError, match="brier_survival needs the baseline hazard: call fit_baseline"):
            _fitted(baseline=False).brier_survival(X, _Y, [1.5, 2.5])
        est = _fitted()
        est.baseline_cumhaz_ = np.array([0.25, -0.5])
        with pytest.raises(ValueError, match="non-negative"):
            est.brier_survival(X, _Y, [1.5, 2.5])
    for X in (np.zeros((30, 6)), FakeDevice((30, 6)), FakeDevice((30,)), np.zeros(30)):
        with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5|2-D"):
            _fitted().brier_survival(X, _Y, [1.5, 2.5])


BAD_CAPI = [
    (dict(times=[]), "empty"),
    (dict(times=[1.0, np.nan], hg=np.zeros((2, 2))), "NAN"),
    (dict(hg=np.zeros((3, 2))), r"hg must have shape \(T, R\) = \(2, 2\)"),
    (dict(hg=np.zeros((2, 3))), r"hg must have shape \(T, R\) = \(2, 2\)"),
    (dict(hg=np.zeros(2)), r"hg must have shape \(T, R\) = \(2, 2\)"),
    (dict(hg=np.array([[0.0, 0.1], [0.2, -0.1]])), "non-negative"),
    (dict(hg=np.array([[0.0, 0.1], [0.2, np.nan]])), "non-negative"),
    (dict(time=_NAN_Y[:, 0]), "NAN"),
    (dict(time=np.zeros(29)), r"time\.size"),
    (dict(status=np.full(30, 2.0)), "0 or 1"),
    (dict(status=FakeDevice((30,), "<i4")), "float64 or float32"),
    (dict(weight=np.full(30, -0.5)), "non-negative"),
    (dict(weight=np.zeros(30)), "sum to 0"),
    (dict(times=[1.0, 30.0]), "largest admissible time is %s" % re.escape(repr(float(np.nextafter(30.0, 0.0))))),
    (dict(censoring="breslow"), "censoring"),
    (dict(censoring=7), "censoring"),
    (dict(cols=[3, 1]), "ascending"),
    (dict(cols=[1, 5]), r"\[0, 5\)"),
    (dict(B=np.ones((3, 2))), "B must have shape"),
]


@pytest.mark.parametrize("kw,msg", BAD_CAPI)
def test_cox_brier_device_rejects_bad_arguments_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    args = dict(cols=[1, 3], B=np.ones((2, 2)), hg=np.full((2, 2), 0.25), times=[1.5, 2.5], time=_Y[:, 0], status=_Y[:, 1])
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        capi.cox_brier_device(FakeDevice((30, 5)), **args)


def test_bad_device_x_and_the_bench_wrapper(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for kw, msg in ((dict(shape=(30,)), "2-D"), (dict(shape=(30, 5), typestr="<i4"), "float64 or float32"),
                    (dict(shape=(30, 5), strides=(-40, 8)), "strides"), (dict(shape=(0, 5)), "empty"),
                    (dict(shape=(30, 5), ptr=0), "null")):
        with pytest.raises(ValueError, match=msg):
            capi.cox_brier_device(FakeDevice(**kw), [1], [1.0], [0.5], [1.5], _Y[:, 0], _Y[:, 1])
        with pytest.raises(ValueError, match=msg):
            capi.op_cox_brier_bench(FakeDevice(**kw), [1])
    for kw, msg in ((dict(cols=[3, 1]), "ascending"), (dict(T=0), "at least 1"), (dict(R=0), "at least 1")):
        args = dict(cols=[1, 3])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            capi.op_cox_brier_bench(FakeDevice((30, 5)), **args)


# ----------------------------------------------------------------------------------------------------------------
# the C entry point
# ----------------------------------------------------------------------------------------------------------------
def _brier_input(**over):
    """A valid bessx_cox_brier_input on a pointer that is never dereferenced, plus the arrays it refers to."""
    n, T, R = 30, 3, 2
    arrays = {"cols": np.asarray(over.pop("cols", [1, 3]), dtype=np.int32), "B": np.ones((2, R)),
              "hg": np.full((R, T), 0.25), "times": np.array([1.5, 0.5, 2.5]), "time": np.arange(1.0, n + 1.0),
              "row_a": np.ones(n), "time_b": np.ones(T), "weight": None}
    for k in list(over):
        if k.endswith("_values"):
            v = over.pop(k)
            arrays[k[:-7]] = None if v is None else np.asarray(v, dtype=np.float64)
    a = capi.CoxBrierInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1 << 20, 0, 5, 1, n, 5
    a.cols, a.m, a.B, a.R = capi._ip(arrays["cols"]), 2, capi._dp(arrays["B"]), R
    a.hg, a.times, a.T = capi._dp(arrays["hg"]), capi._dp(arrays["times"]), T
    a.time, a.row_a, a.time_b = capi._dp(arrays["time"]), capi._dp(arrays["row_a"]), capi._dp(arrays["time_b"])
    a.weight = capi._dp(arrays["weight"])
    for k, v in over.items():
        setattr(a, k, v)
    return a, arrays


def _with(name, index, value, base):
    v = np.array(base, dtype=np.float64)
    v.reshape(-1)[index] = value
    return {name + "_values": v}


def test_c_entry_checks_its_arguments_without_a_gpu():
    lib = capi.lib()
    bs, sw = np.zeros((3, 2)), ctypes.c_double(-7.0)
    t30, ones30 = np.arange(1.0, 31.0), np.ones(30)
    bad = [(dict(cols=[3, 1]), b"ascending"), (dict(cols=[1, 5]), b"out of range"), (dict(x_row_stride=-5), b"strides"),
           (dict(x=None), b"null"), (dict(B=None), b"null"), (dict(m=6), b"m must"), (dict(x_dtype=2), b"dtype"),
           (dict(n=0), b"empty"), (dict(R=0), b"R must"), (dict(R=65536), b"R must"), (dict(T=0), b"T must"),
           (dict(T=(1 << 20) + 1), b"T must"), (dict(hg=None), b"null"), (dict(times=None), b"null"),
           (dict(time=None), b"null"), (dict(row_a=None), b"null"), (dict(time_b=None), b"null"),
           (_with("times", 1, np.nan, [1.5, 0.5, 2.5]), b"times holds a NaN"),
           (_with("time", 7, np.nan, t30), b"time holds a NaN"),
           (_with("hg", 4, -0.25, np.full((2, 3), 0.25)), b"hg must be non-negative"),
           (_with("hg", 5, np.nan, np.full((2, 3), 0.25)), b"hg must be non-negative"),
           (_with("row_a", 3, -1.0, ones30), b"row_a must be non-negative"),
           (_with("row_a", 3, np.inf, ones30), b"row_a must be non-negative"),
           (_with("time_b", 2, -1.0, np.ones(3)), b"time_b must be non-negative"),
           (_with("time_b", 2, np.nan, np.ones(3)), b"time_b must be non-negative"),
           (_with("weight", 4, -1.0, ones30), b"weight must be non-negative"),
           (_with("weight", 4, np.nan, ones30), b"weight must be non-negative"),
           (dict(weight_values=np.zeros(30)), b"positive, finite sum")]
    for over, word in bad:
        a, keep = _brier_input(**dict(over))
        assert lib.bessx_cox_brier_device(ctypes.byref(a), capi._dp(bs), ctypes.byref(sw)) == 1, over
        assert word in lib.bessx_last_error(), (over, lib.bessx_last_error())
    a, keep = _brier_input()
    assert lib.bessx_cox_brier_device(None, capi._dp(bs), ctypes.byref(sw)) == 1
    assert lib.bessx_cox_brier_device(ctypes.byref(a), None, ctypes.byref(sw)) == 1
    assert lib.bessx_cox_brier_device(ctypes.byref(a), capi._dp(bs), None) == 1
    assert not bs.any() and sw.value == -7.0
    ms = np.zeros(3)
    cols = np.array([3, 1], dtype=np.int32)
    assert lib.bessx_op_cox_brier_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, 1, 10, 3,
                                        capi._dp(ms)) == 1
    assert b"ascending" in lib.bessx_last_error()
    cols = np.array([1, 3], dtype=np.int32)
    for R, T, rep in ((0, 10, 3), (1, 0, 3), (1, 10, 0)):
        assert lib.bessx_op_cox_brier_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, R, T, rep,
                                            capi._dp(ms)) == 1


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu_and_the_ledger_is_untouched():
    lib = capi.lib()
    before = capi.process_counters()
    a, keep = _brier_input()
    bs, sw = np.zeros((3, 2)), ctypes.c_double(-7.0)
    assert lib.bessx_cox_brier_device(ctypes.byref(a), capi._dp(bs), ctypes.byref(sw)) == 2  # BESSX_ERR_HIP
    assert not bs.any() and sw.value == -7.0
    for call in (lambda: _fitted().brier_survival(FakeDevice((30, 5)), _Y, [1.5, 2.5]),
                 lambda: capi.cox_brier_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], [0.25, 0.5], [1.5, 2.5], _Y[:, 0],
                                               _Y[:, 1]),
                 lambda: capi.op_cox_brier_bench(FakeDevice((30, 5)), [1, 3], R=2, T=4)):
        with pytest.raises(capi.BessxError) as e:
            call()
        assert e.value.code == 2
    assert capi.process_counters() == before


# ----------------------------------------------------------------------------------------------------------------
# another implementation, where one is installed
# ----------------------------------------------------------------------------------------------------------------
def test_against_scikit_survival_where_it_is_installed(monkeypatch):
    metrics = pytest.importorskip("sksurv.metrics")
    util = pytest.importorskip("sksurv.util")
    monkeypatch.setattr(capi, "lib", _no_library)
    n = 300
    est, X, time, status = _cox_problem(n, 16, 3, seed=84)
    y = np.column_stack([time, status])
    est.fit_baseline(X, y)
    times = np.quantile(time, [0.1, 0.3, 0.5, 0.7])
    got = est.brier_survival(X, y, times)
    surv = est.predict_survival(X, times=times)
    ys = util.Surv.from_arrays(status.astype(bool), time)
    _, bs = metrics.brier_score(ys, ys, surv, times)  # (censoring from the same rows on both sides)
    assert np.abs(bs - got["brier"]).max() <= 1e-10
    assert abs(metrics.integrated_brier_score(ys, ys, surv, times) - got["ibs"]) <= 1e-10
