"""Baseline hazard and survival curves of a Cox model (bessx_cox_baseline_device / bessx_cox_survival_device,
capi.cox_baseline_device / baseline_at / cox_survival_device, bess_base.fit_baseline / predict_survival): what needs no
GPU -- the entry points are exported, declared and listed, bad arguments raise ValueError before the library is asked for
a device, the C entries refuse to compute without a GPU and leave the ledger alone, the step function has its properties,
and the NumPy route is inside the derived bound (tests/coxsurvref.py) of the longdouble reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coxsurvref
import evalref
from bess_amd import capi, linear, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_cox_baseline_device", "bessx_cox_survival_device", "bessx_op_cox_surv_bench")
LD = np.longdouble


class FakeDevice:
    """Stand-in for a device array: only the attribute capi looks at.  The pointer is never dereferenced."""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=1 << 20):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False),
                                         "strides": strides, "version": 3}


def _no_library():
    raise AssertionError("the library was asked before the argument check")


def _fitted(cls=linear.PdasCox, p=5, baseline=True):
    est = cls()
    est.p = p
    est.beta = np.array([0.0, 1.5, 0.0, -2.0, 0.0])[:p]
    est.coef0 = 0.0 if cls is linear.PdasCox else 0.25
    if baseline:
        est.baseline_times_, est.baseline_cumhaz_ = np.array([1.0, 2.0]), np.array([0.25, 0.5])
    return est


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


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
    for word in ("bessx_cox_baseline_input", "bessx_cox_survival_input", "BESSX_SURV_SURVIVAL", "BESSX_SURV_CUMHAZ"):
        assert word in header, word
    for f in ("cox_baseline_device", "baseline_at", "cox_survival_device", "op_cox_surv_bench"):
        assert callable(getattr(capi, f))
    for f in ("fit_baseline", "predict_survival"):
        assert callable(getattr(linear.bess_base, f))


BAD_X = [
    (dict(shape=(30,)), "2-D"),
    (dict(shape=(30, 5, 2)), "2-D"),
    (dict(shape=(30, 5), typestr="<i4"), "float64 or float32"),
    (dict(shape=(30, 5), strides=(-40, 8)), "strides"),
    (dict(shape=(0, 5)), "empty"),
    (dict(shape=(30, 5), ptr=0), "null"),
    (dict(shape=(30, 6)), r"X\.shape\[1\] should be 5"),
]


@pytest.mark.parametrize("kw,msg", BAD_X)
def test_bad_device_x_raises_before_any_device_call(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted().fit_baseline(FakeDevice(**kw), np.zeros((30, 2)))
    with pytest.raises(ValueError, match=msg):
        _fitted().predict_survival(FakeDevice(**kw))
    if "X" not in msg:
        with pytest.raises(ValueError, match=msg):
            capi.cox_baseline_device(FakeDevice(**kw), [1], [1.0], np.arange(30.0), np.ones(30))
        with pytest.raises(ValueError, match=msg):
            capi.cox_survival_device(FakeDevice(**kw), [1], [1.0], [1.0], [0.5])


@pytest.mark.parametrize("shape", [(30,), (30, 5, 2), (30, 6), ()])
def test_a_numpy_x_of_the_wrong_shape_raises_the_existing_message(shape, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
        _fitted().fit_baseline(np.zeros(shape), np.zeros((30, 2)))
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
        _fitted().predict_survival(np.zeros(shape))


_NAN_TIME = np.column_stack([np.where(np.arange(30) == 7, np.nan, np.arange(30.0)), np.ones(30)])
BAD_DATA = [
    (dict(y=np.zeros(30)), r"\(30, 2\)"),
    (dict(y=np.zeros((29, 2))), r"\(30, 2\)"),
    (dict(y=FakeDevice((30,))), r"\(30, 2\)"),
    (dict(y=FakeDevice((30, 2), "<i8")), "float64 or float32"),
    (dict(y=np.zeros((30, 2)), weight=np.ones(31)), r"weight\.size"),
    (dict(y=np.zeros((30, 2)), weight=FakeDevice((29,))), r"weight\.size"),
    (dict(y=_NAN_TIME), "NAN"),
    (dict(y=np.column_stack([np.arange(30.0), np.full(30, 2.0)])), "0 or 1"),
    (dict(y=np.zeros((30, 2)), weight=np.where(np.arange(30) == 3, -1.0, 1.0)), "non-negative"),
    (dict(y=np.zeros((30, 2)), weight=np.where(np.arange(30) == 3, np.nan, 1.0)), "non-negative"),
]


@pytest.mark.parametrize("kw,msg", BAD_DATA)
def test_fit_baseline_rejects_bad_y_and_weight_before_any_device_call(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted().fit_baseline(FakeDevice((30, 5)), **kw)
    if not any(capi.is_device_array(v) for v in kw.values()):
        with pytest.raises(ValueError, match=msg):
            _fitted().fit_baseline(np.zeros((30, 5)), **kw)


BAD_VECTORS = [
    (dict(time=np.zeros(29)), r"time\.size"),
    (dict(time=FakeDevice((31,))), r"time\.size"),
    (dict(status=np.zeros(31)), r"status\.size"),
    (dict(status=FakeDevice((30,), "<i4")), "float64 or float32"),
    (dict(weight=np.ones(3)), r"weight\.size"),
    (dict(time=_NAN_TIME[:, 0]), "NAN"),
    (dict(status=np.full(30, 2.0)), "0 or 1"),
    (dict(weight=np.full(30, -0.5)), "non-negative"),
    (dict(cols=[3, 1]), "ascending"),
    (dict(cols=[1, 1]), "ascending"),
    (dict(cols=[1, 5]), r"\[0, 5\)"),
    (dict(B=[1.0, 2.0, 3.0]), "B must have shape"),
    (dict(B=np.ones((2, 2))), "one model"),
]


@pytest.mark.parametrize("kw,msg", BAD_VECTORS)
def test_cox_baseline_device_rejects_bad_arguments_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    args = dict(cols=[1, 3], B=[1.0, 2.0], time=np.arange(30.0), status=np.ones(30))
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        capi.cox_baseline_device(FakeDevice((30, 5)), **args)


BAD_CURVES = [
    (dict(cols=[3, 1]), "ascending"),
    (dict(cols=[-1, 2]), r"\[0, 5\)"),
    (dict(B=[1.0]), "B must have shape"),
    (dict(kind="hazard"), "kind"),
    (dict(times=[0.5, np.nan]), "NAN"),
    (dict(times=np.zeros((2, 2))), "1-D"),
    (dict(times=[]), "empty"),
    (dict(base_cumhaz=[0.25]), "same size"),
    (dict(base_cumhaz=[0.25, -0.5]), "non-negative"),
    (dict(out=np.zeros((30, 2))), "device array"),
    (dict(out=FakeDevice((30, 3))), r"out must have shape \(30, 2\)"),
    (dict(out=FakeDevice((2, 30))), r"out must have shape \(30, 2\)"),
    (dict(out=FakeDevice((30, 2), "<f4")), "float64"),
    (dict(out=FakeDevice((30, 2), strides=(16, -8))), "strides"),
    (dict(times=[0.5, 1.5, 2.5], out=FakeDevice((30, 2))), r"out must have shape \(30, 3\)"),
]


@pytest.mark.parametrize("kw,msg", BAD_CURVES)
def test_cox_survival_device_rejects_bad_arguments_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    args = dict(cols=[1, 3], B=[1.0, 2.0], base_times=[1.0, 2.0], base_cumhaz=[0.25, 0.5])
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        capi.cox_survival_device(FakeDevice((30, 5)), **args)
    if set(kw) <= {"kind", "times"}:  # (the estimator passes these on: the same error, for either kind of X)
        for X in (FakeDevice((30, 5)), np.zeros((30, 5))):
            with pytest.raises(ValueError, match=msg):
                _fitted().predict_survival(X, **kw)


def test_bench_wrapper_rejects_bad_arguments_before_the_library(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for kw, msg in ((dict(cols=[3, 1]), "ascending"), (dict(kind="hazard"), "kind"), (dict(T=0), "T must")):
        args = dict(cols=[1, 3])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            capi.op_cox_surv_bench(FakeDevice((30, 5)), **args)


def test_other_families_raise_and_curves_need_a_baseline(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for cls in (linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson):
        for X in (np.zeros((30, 5)), FakeDevice((30, 5))):
            with pytest.raises(ValueError, match="Cox"):
                _fitted(cls).fit_baseline(X, np.zeros((30, 2)))
            with pytest.raises(ValueError, match="Cox"):
                _fitted(cls).predict_survival(X)
    for X in (np.zeros((30, 5)), FakeDevice((30, 5))):
        with pytest.raises(ValueError, match="fit_baseline"):
            _fitted(baseline=False).predict_survival(X)


def _baseline_input(**over):
    """A valid bessx_cox_baseline_input on a pointer that is never dereferenced, plus the arrays it refers to."""
    cols = np.asarray(over.pop("cols", [1, 3]), dtype=np.int32)
    time = np.asarray(over.pop("time_values", np.arange(30.0)))
    status = np.asarray(over.pop("status_values", np.ones(30)))
    weight = over.pop("weight_values", None)
    weight = None if weight is None else np.asarray(weight, dtype=np.float64)
    B = np.array([1.0, 2.0])
    a = capi.CoxBaselineInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1 << 20, 0, 5, 1, 30, 5
    a.cols, a.m, a.B = capi._ip(cols), 2, capi._dp(B)
    a.time, a.status, a.weight = capi._dp(time), capi._dp(status), capi._dp(weight)
    for k, v in over.items():
        setattr(a, k, v)
    return a, (cols, B, time, status, weight)


def _survival_input(**over):
    cols = np.asarray(over.pop("cols", [1, 3]), dtype=np.int32)
    hg = np.asarray(over.pop("hg_values", [0.0, 0.25, 0.5]), dtype=np.float64)
    B = np.array([1.0, 2.0])
    a = capi.CoxSurvivalInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1 << 20, 0, 5, 1, 30, 5
    a.cols, a.m, a.B, a.hg, a.T, a.kind = capi._ip(cols), 2, capi._dp(B), capi._dp(hg), hg.size, 0
    a.out_row_stride, a.out_col_stride, a.out_on_device = hg.size, 1, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a, (cols, B, hg)


_COMMON_BAD = [(dict(cols=[3, 1]), b"ascending"), (dict(cols=[1, 1]), b"ascending"), (dict(cols=[1, 5]), b"out of range"),
               (dict(cols=[-1, 2]), b"out of range"), (dict(x_row_stride=-5), b"strides"),
               (dict(x_col_stride=-1), b"strides"), (dict(x=None), b"null"), (dict(B=None), b"null"),
               (dict(m=6), b"m must"), (dict(x_dtype=2), b"dtype"), (dict(n=0), b"empty")]


def test_c_entries_check_their_arguments_without_a_gpu():
    lib = capi.lib()
    J, times, cumhaz = ctypes.c_int(0), np.zeros(30), np.zeros(30)
    nan_time = np.arange(30.0)
    nan_time[7] = np.nan
    neg_w, nan_w = np.ones(30), np.ones(30)
    neg_w[4], nan_w[4] = -1.0, np.nan
    for bad, word in _COMMON_BAD + [(dict(time=None), b"null"), (dict(status=None), b"null"),
                                    (dict(time_values=nan_time), b"NaN"),
                                    (dict(status_values=np.full(30, 2.0)), b"status"),
                                    (dict(weight_values=neg_w), b"weight"), (dict(weight_values=nan_w), b"weight")]:
        a, keep = _baseline_input(**bad)
        assert lib.bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(J), capi._dp(times), capi._dp(cumhaz)) == 1, bad
        assert word in lib.bessx_last_error(), (bad, lib.bessx_last_error())
    a, keep = _baseline_input()
    assert lib.bessx_cox_baseline_device(None, ctypes.byref(J), capi._dp(times), capi._dp(cumhaz)) == 1
    assert lib.bessx_cox_baseline_device(ctypes.byref(a), None, capi._dp(times), capi._dp(cumhaz)) == 1
    assert lib.bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(J), None, capi._dp(cumhaz)) == 1
    out = np.zeros((30, 3))
    for bad, word in _COMMON_BAD + [(dict(hg=None), b"hg"), (dict(T=0), b"hg"),
                                    (dict(hg_values=[0.0, -0.25, 0.5]), b"non-negative"),
                                    (dict(hg_values=[0.0, np.nan, 0.5]), b"non-negative"), (dict(kind=2), b"kind"),
                                    (dict(kind=-1), b"kind"), (dict(out_row_stride=-3), b"strides"),
                                    (dict(out_col_stride=-1), b"strides"), (dict(out_row_stride=0), b"zero stride"),
                                    (dict(out_col_stride=0), b"zero stride")]:
        a, keep = _survival_input(**bad)
        assert lib.bessx_cox_survival_device(ctypes.byref(a), out.ctypes.data) == 1, bad
        assert word in lib.bessx_last_error(), (bad, lib.bessx_last_error())
    a, keep = _survival_input()
    assert lib.bessx_cox_survival_device(None, out.ctypes.data) == 1
    assert lib.bessx_cox_survival_device(ctypes.byref(a), None) == 1
    assert not out.any()
    ms = np.zeros(3)
    cols = np.array([3, 1], dtype=np.int32)
    assert lib.bessx_op_cox_surv_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, 10, 0, 0, 3,
                                       capi._dp(ms)) == 1
    assert b"ascending" in lib.bessx_last_error()
    cols = np.array([1, 3], dtype=np.int32)
    for T, kind in ((0, 0), (10, 2)):
        assert lib.bessx_op_cox_surv_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, T, kind, 0, 3,
                                           capi._dp(ms)) == 1


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu_and_the_ledger_is_untouched():
    lib = capi.lib()
    before = capi.process_counters()
    a, keep = _baseline_input()
    J, times, cumhaz = ctypes.c_int(-7), np.zeros(30), np.zeros(30)
    assert lib.bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(J), capi._dp(times), capi._dp(cumhaz)) == 2
    assert J.value == -7 and not times.any() and not cumhaz.any()
    a, keep = _survival_input()
    out = np.zeros((30, 3))
    assert lib.bessx_cox_survival_device(ctypes.byref(a), out.ctypes.data) == 2  # BESSX_ERR_HIP
    assert not out.any()
    y = np.column_stack([np.arange(30.0), np.ones(30)])
    for call in (lambda: _fitted().fit_baseline(FakeDevice((30, 5)), y),
                 lambda: _fitted().predict_survival(FakeDevice((30, 5))),
                 lambda: capi.cox_baseline_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], y[:, 0], y[:, 1]),
                 lambda: capi.cox_survival_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], [1.0], [0.5]),
                 lambda: capi.op_cox_surv_bench(FakeDevice((30, 5)), [1, 3], T=4)):
        with pytest.raises(capi.BessxError) as e:
            call()
        assert e.value.code == 2
    assert capi.process_counters() == before


# ----------------------------------------------------------------------------------------------------------------
# the step function
# ----------------------------------------------------------------------------------------------------------------
def test_baseline_at_is_the_right_continuous_step_function():
    bt, bh = np.array([1.0, 2.0, 3.5]), np.array([0.25, 0.75, 2.0])
    at = lambda t: capi.baseline_at(bt, bh, t)
    assert np.array_equal(at([0.0, 0.999, -5.0]), [0.0, 0.0, 0.0])                      # before the first time
    assert np.array_equal(at([1.0, 2.0, 3.5]), bh)                                      # at an event time: included
    assert np.array_equal(at([np.nextafter(1.0, 0.0), np.nextafter(2.0, 0.0)]), [0.0, 0.25])
    assert np.array_equal(at([1.5, 2.5, 3.4999]), [0.25, 0.75, 0.75])                   # between times
    assert np.array_equal(at([3.5001, 1e300, np.inf]), [2.0, 2.0, 2.0])                 # after the last
    assert np.array_equal(at([9.0, 0.5, 2.0, 1.0, 2.0, 2.0, 0.5]), [2.0, 0.0, 0.75, 0.25, 0.75, 0.75, 0.0])
    assert at(2.0).shape == () and float(at(2.0)) == 0.75
    assert at(np.array([[1.0, 2.0], [3.0, 4.0]])).shape == (2, 2)
    assert np.array_equal(capi.baseline_at([], [], [0.0, 1.0]), [0.0, 0.0])             # every row censored
    with pytest.raises(ValueError, match="NAN"):
        at([1.0, np.nan])
    with pytest.raises(ValueError, match="same size"):
        capi.baseline_at(bt, bh[:2], [1.0])


# ----------------------------------------------------------------------------------------------------------------
# the NumPy route against the longdouble reference
# ----------------------------------------------------------------------------------------------------------------
def test_the_reference_agrees_with_the_brute_force_statement_of_the_definition():
    assert coxsurvref.self_check()


def _cox_problem(n, p, m, seed, decimals=None):
    """make_cox rows in a shuffled order, m random support columns with N(0, 0.25) coefficients, weights that are
    multiples of 1/8 (some zero); decimals rounds the times into tie groups."""
    X, obs, status, _, _ = synth.make_cox(n, p, 3, seed=seed)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    X, obs, status = np.ascontiguousarray(X[perm]), obs[perm], status[perm]
    if decimals is not None:
        obs = np.round(obs, decimals)
    est = linear.PdasCox()
    est.p, est.coef0 = p, 0.0
    est.beta = np.zeros(p)
    est.beta[rng.choice(p, m, replace=False)] = rng.normal(0.0, 0.5, m)
    w = rng.integers(0, 17, n) / 8.0
    return est, X, obs, status, w


def _grid(bt, rng):
    """Times before, at, between and after the baseline's, unsorted and repeated."""
    lo, hi = (bt[0], bt[-1]) if bt.size else (1.0, 2.0)
    g = np.concatenate([[lo - 1.0, hi + 1.0], bt[:5], 0.5 * (bt[:-1] + bt[1:])[:5], rng.uniform(lo, hi, 7)])
    g = np.concatenate([g, g[:3]])
    return g[rng.permutation(g.size)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("decimals", [None, 1])
def test_numpy_route_is_inside_the_bound(decimals, weighted, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)  # (a NumPy X never touches the library)
    n = 513
    est, X, time, status, w = _cox_problem(n, 16, 3, seed=84, decimals=decimals)
    w = w if weighted else None
    cols = np.nonzero(est.beta)[0]
    eta, delta = evalref.eta_reference(X, cols, est.beta[cols].reshape(-1, 1), [0.0])
    assert float(np.abs(eta).max()) <= 5.0
    ref = coxsurvref.baseline_reference(eta, delta, time, status, w)
    what = "numpy n=%d decimals=%s weighted=%s" % (n, decimals, weighted)
    assert est.fit_baseline(X, np.column_stack([time, status]), weight=w) is est
    if decimals is not None:
        assert ref["times"].size < np.unique(time).size < 0.9 * n  # (ties, and times that carry no event)
    coxsurvref.check_baseline(est.baseline_times_, est.baseline_cumhaz_, ref, what)
    assert (np.diff(est.baseline_times_) > 0).all() and (np.diff(est.baseline_cumhaz_) >= 0).all()
    # the bound is not slack: a relative change of 1e-10 falls outside
    exact = ref["cumhaz"].astype(np.float64)
    pos = ref["cumhaz"] > 0
    assert (np.abs((exact * (1 + 1e-10)).astype(LD) - ref["cumhaz"]) > ref["bound"])[pos].all()
    # the curves: the estimator's H0 stands in for the exact one, within the baseline's bound
    grid = _grid(est.baseline_times_, np.random.default_rng(1))
    idx = np.searchsorted(ref["times"], grid, side="right")
    hg = np.concatenate([[LD(0)], ref["cumhaz"]])[idx]
    hb = np.concatenate([[LD(0)], ref["bound"]])[idx]
    for kind in ("survival", "cumhaz"):
        got = est.predict_survival(X, times=grid, kind=kind)
        assert isinstance(got, np.ndarray) and got.shape == (n, grid.size)
        coxsurvref.check_curves(got, coxsurvref.curve_reference(eta, delta, hg, kind, hg_bound=hb), what)
        assert (got[:, idx == 0] == (1.0 if kind == "survival" else 0.0)).all() and (idx == 0).any()
    own = est.predict_survival(X)
    assert own.shape == (n, est.baseline_times_.size)
    assert (np.diff(own, axis=1) <= 0).all() and (own >= 0).all() and (own <= 1).all()


def test_every_row_censored_is_not_an_error(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    est, X, time, status, w = _cox_problem(64, 16, 3, seed=84)
    est.fit_baseline(X, np.column_stack([time, np.zeros(64)]), weight=w)
    assert est.baseline_times_.shape == (0,) and est.baseline_cumhaz_.shape == (0,)
    coxsurvref.check_baseline(est.baseline_times_, est.baseline_cumhaz_,
                              coxsurvref.baseline_reference(np.zeros(64), np.zeros(64), time, np.zeros(64), w), "censored")
    assert np.array_equal(est.predict_survival(X, times=[0.5, 3.0]), np.ones((64, 2)))
    assert np.array_equal(est.predict_survival(X, times=[0.5, 3.0], kind="cumhaz"), np.zeros((64, 2)))
    with pytest.raises(ValueError, match="empty"):
        est.predict_survival(X)


def test_the_known_answer(monkeypatch):
    """times (1, 2, 2, 3), status (1, 1, 0, 1), no support column: e = 1 for every row, the risk sets hold 4, 3, 3, 1
    rows, so H0 = 1/4, 1/4 + 1/3, 1/4 + 1/3 + 1 at the times 1, 2, 3; S(2.5 | any x) = exp(-7/12), S(0.5) = 1 exactly."""
    monkeypatch.setattr(capi, "lib", _no_library)
    y = np.array([[1.0, 1.0], [2.0, 1.0], [2.0, 0.0], [3.0, 1.0]])
    X = np.random.default_rng(0).standard_normal((4, 3))
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = 3, np.zeros(3), 0.0
    est.fit_baseline(X, y)
    want = np.array([LD(1) / 4, LD(1) / 4 + LD(1) / 3, LD(1) / 4 + LD(1) / 3 + LD(1)])
    ref = coxsurvref.baseline_reference(np.zeros(4), np.zeros(4), y[:, 0], y[:, 1], None)
    assert np.array_equal(ref["times"], [1.0, 2.0, 3.0])
    assert (np.abs(ref["cumhaz"] - want) <= LD(2.0) ** -60).all()
    coxsurvref.check_baseline(est.baseline_times_, est.baseline_cumhaz_, ref, "known answer")
    got = est.predict_survival(X, times=[2.5, 0.5])
    cref = coxsurvref.curve_reference(np.zeros(4), np.zeros(4), [want[1], 0.0], "survival", hg_bound=[ref["bound"][1], 0.0])
    assert (np.abs(cref["value"][:, 0] - np.exp(-LD(7) / 12)) <= LD(2.0) ** -60).all()
    coxsurvref.check_curves(got, cref, "known answer")
    assert (got[:, 1] == 1.0).all()
    brute = coxsurvref.brute_force_baseline(np.zeros(4), y[:, 0], y[:, 1], None)
    assert np.array_equal(brute[0], [1.0, 2.0, 3.0]) and (np.abs(brute[1] - want) <= LD(2.0) ** -60).all()


def test_the_bound_holds_a_correctly_rounded_survival_below_the_normal_range(monkeypatch):
    """Below 2^-1022 fp64 is spaced 2^-1074 apart: the correctly rounded value of exp(-743.7) is off by up to a quarter
    of itself, far outside 2 u S*, and the bound carries the spacing there.  From 2^-1021 up it is the relative one."""
    monkeypatch.setattr(capi, "lib", _no_library)
    hg = np.concatenate([np.linspace(1.0, 700.0, 50), np.linspace(708.0, 760.0, 400)])
    cref = coxsurvref.curve_reference(np.zeros(2), np.zeros(2), hg, "survival")
    val, bnd = cref["value"][0], cref["bound"][0]
    rounded = val.astype(np.float64)
    assert (np.abs(rounded.astype(LD) - val) <= bnd).all()
    low = val < LD(2.0) ** -1022
    assert low.sum() > 100 and (np.abs(rounded.astype(LD) - val) > 4 * evalref.U * val)[low].any()
    assert (bnd[low] <= coxsurvref.TINY + LD(1e-12) * val[low]).all() and (bnd[low] >= coxsurvref.TINY).all()
    high = val >= LD(2.0) ** -1021
    grow = np.expm1(hg.astype(LD) * (coxsurvref._rho(LD(0)) + evalref.U))  # (dz: no error in eta or in hg)
    stated = val * (grow * (1 + 2 * evalref.U) + 2 * evalref.U)
    assert high.sum() >= 50 and (np.abs(bnd - stated)[high] <= LD(2.0) ** -60 * stated[high]).all()
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = 3, np.zeros(3), 0.0
    est.baseline_times_, est.baseline_cumhaz_ = np.arange(1.0, hg.size + 1.0), hg
    got = est.predict_survival(np.ones((2, 3)))
    coxsurvref.check_curves(got, cref, "numpy, subnormal range")
    assert (got[:, low] < 2.0 ** -1022).all() and (got == 0).any() and (got[:, -1] == 0).all()


def test_fit_leaves_no_baseline_behind():
    est = linear.PdasCox()
    assert not hasattr(est, "baseline_times_") and not hasattr(est, "baseline_cumhaz_")
