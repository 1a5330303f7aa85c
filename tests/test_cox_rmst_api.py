"""Restricted mean and quantile survival times (capi.rmst_segments, capi.cox_survival_times_device,
bess_base.predict_rmst / predict_quantile, bessx_cox_survtime_device of include/bessx.h section 2u): everything that needs
no GPU -- the segments, every argument error of the Python layers and of the C entry, the NumPy route against the
longdouble reference and derived bound of tests/coxrmstref.py, and the no-GPU behaviour."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coxrmstref
import evalref
from bess_amd import capi, linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_cox_survtime_device", "bessx_cox_survtime_workspace", "bessx_op_cox_rmst_bench")
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
    assert "bessx_cox_survtime_input" in header and " 2u. " in header
    for f in ("rmst_segments", "cox_survival_times_device", "op_cox_rmst_bench", "cox_survtime_workspace"):
        assert callable(getattr(capi, f))
    for f in ("predict_rmst", "predict_quantile"):
        assert callable(getattr(linear.bess_base, f))


# ----------------------------------------------------------------------------------------------------------------
# the segments
# ----------------------------------------------------------------------------------------------------------------
def test_rmst_segments_on_hand_made_baselines():
    bt, bh = np.array([1.0, 2.0, 4.0]), np.array([0.25, 0.5, 1.0])
    hs, wd, cut = capi.rmst_segments(bt, bh, [3.0])
    assert hs.tolist() == [0.0, 0.25, 0.5] and wd.tolist() == [1.0, 1.0, 1.0] and cut.tolist() == [3]
    assert hs.dtype == np.float64 and wd.dtype == np.float64 and cut.dtype == np.int32
    # ties of tau with event times, tau = 0, tau beyond the last time, unsorted and repeated
    hs, wd, cut = capi.rmst_segments(bt, bh, [2.0, 0.0, 7.0, 2.0, 4.0, 0.5])
    assert hs.tolist() == [0.0, 0.0, 0.25, 0.5, 1.0] and wd.tolist() == [0.5, 0.5, 1.0, 2.0, 3.0]
    assert cut.tolist() == [3, 0, 5, 3, 4, 1]
    # the base times at or beyond max(tau) make no segment; a base time of exactly 0 moves the first hazard
    hs, wd, cut = capi.rmst_segments([0.0, 1.0, 2.0], [0.125, 0.25, 0.5], [1.0])
    assert hs.tolist() == [0.125] and wd.tolist() == [1.0] and cut.tolist() == [1]
    hs, wd, cut = capi.rmst_segments(bt, bh, [0.0, 0.0])
    assert hs.size == 0 and wd.size == 0 and cut.tolist() == [0, 0]
    hs, wd, cut = capi.rmst_segments([], [], [2.5])  # J = 0: one segment (0, tau)
    assert hs.tolist() == [0.0] and wd.tolist() == [2.5] and cut.tolist() == [1]
    hs, wd, cut = capi.rmst_segments(bt, bh, [0.75])  # below the first event time
    assert hs.tolist() == [0.0] and wd.tolist() == [0.75] and cut.tolist() == [1]
    rng = np.random.default_rng(3)
    bt, bh = np.cumsum(rng.uniform(0.1, 1.0, 50)), np.cumsum(rng.uniform(0.0, 0.2, 50))
    tau = rng.uniform(0.0, bt[-1] + 3.0, 9)
    hs, wd, cut = capi.rmst_segments(bt, bh, tau)
    ends = np.cumsum(wd)
    assert (wd > 0).all() and (np.diff(hs) >= 0).all() and cut.max() == hs.size
    assert np.allclose(ends[cut - 1], tau, rtol=1e-14) and (hs == capi.baseline_at(bt, bh, ends - wd * 0.5)).all()


@pytest.mark.parametrize("kw,msg", [
    (dict(tau=[1.0, np.nan]), "NAN value in tau"), (dict(tau=[-1.0]), "non-negative"), (dict(tau=[np.inf]), "finite"),
    (dict(tau=[]), "at least one"), (dict(tau=[[1.0, 2.0]]), "1-D"), (dict(tau=3.0), "1-D"),
    (dict(base_times=[-1.0, 2.0]), "base_times should be non-negative"), (dict(base_cumhaz=[0.5]), "same size"),
    (dict(base_times=[np.nan, 2.0]), "NAN value in base_times"),
])
def test_rmst_segments_value_errors(kw, msg):
    args = dict(base_times=[1.0, 2.0], base_cumhaz=[0.25, 0.5], tau=[1.5])
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        capi.rmst_segments(**args)


@pytest.mark.parametrize("kw,msg", [
    (dict(), "nothing to compute"), (dict(q=[0.5], hazard_levels=[0.3]), "not both"), (dict(q=[0.0]), "between 0 and 1"),
    (dict(q=[1.0]), "between 0 and 1"), (dict(q=[np.nan]), "between 0 and 1"), (dict(q=[[0.5]]), "1-D"),
    (dict(hazard_levels=[0.0]), "positive"), (dict(hazard_levels=[np.nan]), "positive"), (dict(hazard_levels=[]), "at least"),
    (dict(tau=[-1.0]), "non-negative"), (dict(tau=[np.nan]), "NAN"), (dict(tau=[1.0], out_quantile=1), "out_quantile goes"),
    (dict(q=[0.5], out_rmst=1), "out_rmst goes"), (dict(tau=[1.0], out_rmst=np.zeros((30, 1))), "must be a device array"),
    (dict(tau=[1.0], out_rmst=FakeDevice((30, 2))), "must have shape"),
    (dict(q=[0.5], out_quantile=FakeDevice((30, 1), typestr="<f4")), "float64"),
    (dict(q=[0.5], base_cumhaz=[0.5, 0.25]), "non-decreasing"), (dict(q=[0.5], base_cumhaz=[-0.5, 0.25]), "non-negative"),
    (dict(tau=[3.0], base_cumhaz=[-0.5, 0.25]), "non-negative"), (dict(q=[0.5], base_times=[np.nan, 1.0]), "NAN"),
    (dict(tau=[1.0], cols=[3, 1]), "ascending|sorted|increasing"),
])
def test_cox_survival_times_device_rejects_bad_arguments_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    args = dict(x=FakeDevice((30, 5)), cols=[1, 3], B=[1.0, 2.0], base_times=[1.0, 2.0], base_cumhaz=[0.25, 0.5])
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        capi.cox_survival_times_device(**args)


def test_the_estimator_methods_check_before_any_device_call(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for cls in (linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson):
        for X in (np.zeros((30, 5)), FakeDevice((30, 5))):
            with pytest.raises(ValueError, match="predict_rmst is for the Cox classes"):
                _fitted(cls).predict_rmst(X, [1.0])
            with pytest.raises(ValueError, match="predict_quantile is for the Cox classes"):
                _fitted(cls).predict_quantile(X)
    for X in (np.zeros((30, 5)), FakeDevice((30, 5))):
        with pytest.raises(ValueError, match="predict_rmst needs the baseline hazard: call fit_baseline"):
            _fitted(baseline=False).predict_rmst(X, [1.0])
        with pytest.raises(ValueError, match="predict_quantile needs the baseline hazard: call fit_baseline"):
            _fitted(baseline=False).predict_quantile(X)
        with pytest.raises(ValueError, match="non-negative"):
            _fitted().predict_rmst(X, [-1.0])
        with pytest.raises(ValueError, match="NAN"):
            _fitted().predict_rmst(X, [np.nan])
        with pytest.raises(ValueError, match="between 0 and 1"):
            _fitted().predict_quantile(X, 1.0)
    for X in (np.zeros((30, 6)), FakeDevice((30, 6))):
        with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
            _fitted().predict_rmst(X, [1.0])
        with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
            _fitted().predict_quantile(X)


# ----------------------------------------------------------------------------------------------------------------
# the C entry without a device
# ----------------------------------------------------------------------------------------------------------------
def _input(**over):
    """A valid bessx_cox_survtime_input on a pointer that is never dereferenced, plus the arrays it refers to."""
    cols = np.asarray(over.pop("cols", [1, 3]), dtype=np.int32)
    hs = np.asarray(over.pop("hs_values", [0.0, 0.25, 0.5]), dtype=np.float64)
    wd = np.asarray(over.pop("wd_values", [1.0, 1.0, 0.5]), dtype=np.float64)
    cut = np.asarray(over.pop("cut_values", [3, 1]), dtype=np.int32)
    hz = np.asarray(over.pop("hz_values", [0.25, 0.5, 0.5]), dtype=np.float64)
    ut = np.asarray(over.pop("ut_values", [1.0, 2.0, 4.0]), dtype=np.float64)
    c = np.asarray(over.pop("c_values", [0.3, 0.7]), dtype=np.float64)
    B = np.array([1.0, 2.0])
    a = capi.CoxSurvtimeInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1 << 20, 0, 5, 1, 30, 5
    a.cols, a.m, a.B = capi._ip(cols), 2, capi._dp(B)
    a.hs, a.wd, a.K, a.cut, a.T = capi._dp(hs), capi._dp(wd), hs.size, capi._ip(cut), cut.size
    a.hz, a.ut, a.J, a.c, a.Q = capi._dp(hz), capi._dp(ut), hz.size, capi._dp(c), c.size
    a.rmst_row_stride, a.rmst_col_stride, a.quant_row_stride, a.quant_col_stride = cut.size, 1, c.size, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a, (cols, B, hs, wd, cut, hz, ut, c)


_BAD = [(dict(cols=[3, 1]), b"ascending"), (dict(cols=[1, 1]), b"ascending"), (dict(cols=[1, 5]), b"out of range"),
        (dict(x_row_stride=-5), b"strides"), (dict(x=None), b"null"), (dict(B=None), b"null"), (dict(m=6), b"m must"),
        (dict(x_dtype=2), b"dtype"), (dict(n=0), b"empty"),
        (dict(hs_values=[0.0, np.nan, 0.5]), b"hs must be non-negative"),
        (dict(hs_values=[0.0, -0.25, 0.5]), b"hs must be non-negative"),
        (dict(wd_values=[1.0, 0.0, 0.5]), b"wd must be positive"), (dict(wd_values=[1.0, np.nan, 0.5]), b"wd must be positive"),
        (dict(wd_values=[1.0, -1.0, 0.5]), b"wd must be positive"), (dict(cut_values=[4, 1]), b"cut must lie"),
        (dict(cut_values=[3, -1]), b"cut must lie"), (dict(hz_values=[0.5, 0.25, 0.5]), b"non-decreasing"),
        (dict(hz_values=[-0.5, 0.25, 0.5]), b"hz must be non-negative"),
        (dict(hz_values=[0.25, np.nan, 0.5]), b"hz must be non-negative"), (dict(c_values=[0.3, 0.0]), b"c must be positive"),
        (dict(c_values=[np.nan, 0.7]), b"c must be positive"), (dict(c_values=[-0.3, 0.7]), b"c must be positive"),
        (dict(ut_values=[1.0, np.nan, 4.0]), b"ut holds a NaN"), (dict(rmst_row_stride=-2), b"strides"),
        (dict(quant_col_stride=-1), b"strides"), (dict(rmst_row_stride=0), b"zero stride"),
        (dict(rmst_col_stride=0), b"zero stride"), (dict(quant_row_stride=0), b"zero stride"),
        (dict(quant_col_stride=0), b"zero stride"), (dict(hs=None), b"null"), (dict(wd=None), b"null"),
        (dict(cut=None), b"null"), (dict(hz=None), b"null"), (dict(ut=None), b"null"), (dict(c=None), b"null"),
        (dict(T=-1), b"non-negative"), (dict(Q=-1), b"non-negative"), (dict(K=-1), b"non-negative"),
        (dict(J=-1), b"non-negative")]


def test_the_c_entry_checks_its_arguments_without_a_gpu():
    lib = capi.lib()
    rm, qu = np.zeros((30, 2)), np.zeros((30, 2))
    for bad, word in _BAD:
        a, keep = _input(**bad)
        assert lib.bessx_cox_survtime_device(ctypes.byref(a), rm.ctypes.data, qu.ctypes.data) == 1, bad
        assert word in lib.bessx_last_error(), (bad, lib.bessx_last_error())
    a, keep = _input()
    assert lib.bessx_cox_survtime_device(None, rm.ctypes.data, qu.ctypes.data) == 1
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), None, qu.ctypes.data) == 1 and b"rmst" in lib.bessx_last_error()
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), rm.ctypes.data, None) == 1 and b"quant" in lib.bessx_last_error()
    a, keep = _input(T=0, Q=0)
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), None, None) == 1 and b"nothing" in lib.bessx_last_error()
    a, keep = _input(T=0)  # an absent part goes with a NULL pointer
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), rm.ctypes.data, qu.ctypes.data) == 1
    assert not rm.any() and not qu.any()
    ms = np.zeros(4)
    cols = np.array([1, 3], dtype=np.int32)
    for K, T, J, Q in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert lib.bessx_op_cox_rmst_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, K, T, J, Q, 3,
                                           capi._dp(ms)) == 1
    with pytest.raises(ValueError, match="at least 1"):
        capi.op_cox_rmst_bench(FakeDevice((30, 5)), [1, 3], T=0)


def test_the_workspace_states_the_pieces_and_the_bounded_scratch():
    w = capi.cox_survtime_workspace(1000, [0])
    SL = w["slab"]
    assert SL >= 2 and w["pieces"] == 0 and w["doubles"] >= 1000
    for cut, pieces in (([1], 1), ([SL - 1], 1), ([SL], 1), ([SL + 1], 2), ([3 * SL], 3), ([3 * SL, SL], 3),
                        ([3 * SL, SL + 1, SL + 1, 0], 4), ([5, 7, 5], 2), ([2 * SL + 1, 2 * SL], 3)):
        assert capi.cox_survtime_workspace(1000, cut)["pieces"] == pieces, cut
    big = capi.cox_survtime_workspace(200000, [139733])
    assert big["pieces"] == -(-139733 // SL) and big["rows_per_chunk"] % 512 == 0
    assert big["pieces"] * big["rows_per_chunk"] <= 1 << 24  # 128 MiB of partials, not n x K
    assert big["doubles"] <= 200000 + 2 * 139733 + (1 << 24) + big["pieces"] + 8
    small = capi.cox_survtime_workspace(1000, [139733])
    assert small["rows_per_chunk"] == 1000
    with pytest.raises(capi.BessxError):
        capi.cox_survtime_workspace(0, [1])
    with pytest.raises(capi.BessxError):
        capi.cox_survtime_workspace(10, [-1])


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu_and_the_ledger_is_untouched():
    lib = capi.lib()
    before = capi.process_counters()
    rm, qu = np.zeros((30, 2)), np.zeros((30, 2))
    a, keep = _input()
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), rm.ctypes.data, qu.ctypes.data) == 2  # BESSX_ERR_HIP
    a, keep = _input(T=0)
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), None, qu.ctypes.data) == 2
    a, keep = _input(Q=0, J=0, hz=None, ut=None, c=None)
    assert lib.bessx_cox_survtime_device(ctypes.byref(a), rm.ctypes.data, None) == 2
    assert not rm.any() and not qu.any()
    for call in (lambda: _fitted().predict_rmst(FakeDevice((30, 5)), [1.0, 3.0]),
                 lambda: _fitted().predict_quantile(FakeDevice((30, 5))),
                 lambda: capi.cox_survival_times_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], [1.0], [0.5], tau=[2.0],
                                                        q=[0.5]),
                 lambda: capi.op_cox_rmst_bench(FakeDevice((30, 5)), [1, 3])):
        with pytest.raises(capi.BessxError) as e:
            call()
        assert e.value.code == 2
    assert capi.process_counters() == before


# ----------------------------------------------------------------------------------------------------------------
# the NumPy route
# ----------------------------------------------------------------------------------------------------------------
def test_the_reference_agrees_with_the_independent_statement_of_the_definition():
    assert coxrmstref.self_check()


def _cox_problem(n, p, m, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    est = linear.PdasCox()
    est.p, est.coef0 = p, 0.0
    est.beta = np.zeros(p)
    cols = np.sort(rng.choice(p, m, replace=False))
    est.beta[cols] = rng.standard_normal(m) / np.sqrt(max(m, 1))
    time = rng.exponential(1.0, n)
    status = (rng.uniform(size=n) < 0.6).astype(np.float64)
    est.fit_baseline(X, np.column_stack([time, status]))
    eta, delta = evalref.eta_reference(X, cols, est.beta[cols].reshape(-1, 1), [0.0])
    return est, X, time, eta[:, 0], delta[:, 0]


@pytest.mark.parametrize("m", [0, 3])
def test_numpy_route_is_inside_the_bound(m, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    est, X, time, eta, delta = _cox_problem(700, 12, m, seed=5 + m)
    bt, bh = est.baseline_times_, est.baseline_cumhaz_
    tau = np.array([np.quantile(time, 0.5), 0.0, 1.5 * time.max(), bt[3], np.quantile(time, 0.1), bt[3], 0.5 * bt[0]])
    monkeypatch.setattr(linear.bess_base, "_SURVTIME_BLOCK", 700 * 37)  # several blocks of segments
    got = est.predict_rmst(X, tau)
    assert got.shape == (700, 7) and got.dtype == np.float64
    hs, wd, cut = capi.rmst_segments(bt, bh, tau)
    coxrmstref.check_rmst(got, coxrmstref.rmst_reference(eta, delta, hs, wd, cut), "numpy route, m=%d" % m)
    assert (got[:, 1] == 0.0).all() and (got[:, 6] == 0.5 * bt[0]).all()
    assert np.array_equal(got[:, 3], got[:, 5]) and (np.diff(got[:, np.argsort(tau, kind="stable")], axis=1) >= 0).all()
    one = est.predict_rmst(X, float(tau[0]))
    assert one.shape == (700,) and np.array_equal(one, est.predict_rmst(X, tau[:1])[:, 0])
    levels = np.array([0.1, 0.25, 0.5, 0.75, 0.9])
    monkeypatch.setattr(linear.bess_base, "_SURVTIME_BLOCK", bt.size * 64)  # several blocks of rows
    qt = est.predict_quantile(X, levels)
    assert qt.shape == (700, 5)
    ref = coxrmstref.quantile_reference(eta, delta, bh, capi.survival_levels(levels))
    coxrmstref.check_quantiles(qt, ref, bt, "numpy route, m=%d" % m)
    assert np.isfinite(qt).any() and (m == 0 or np.isinf(qt).any())  # (the +inf branch: rows that never reach 0.9)
    med = est.predict_quantile(X)
    assert med.shape == (700,) and np.array_equal(med, qt[:, 2])
    bad = X.copy()
    support = np.nonzero(est.beta)[0]
    if m:
        bad[17, support[0]] = np.nan
        bad[:, np.setdiff1d(np.arange(12), support)] = np.nan  # outside the support: not seen
        rn, qn = est.predict_rmst(bad, tau), est.predict_quantile(bad, levels)
        assert np.isnan(rn[17]).all() and np.isnan(qn[17]).all()
        keep = np.arange(700) != 17
        assert np.array_equal(rn[keep], got[keep]) and np.array_equal(qn[keep], qt[keep])


def test_the_known_answers(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    est = _fitted()
    est.beta = np.zeros(5)  # e = 1 for every row
    est.baseline_times_, est.baseline_cumhaz_ = np.arange(1.0, 9.0), np.arange(1.0, 9.0) / 8.0
    X = np.zeros((3, 5))
    got = est.predict_rmst(X, [2.0])
    want = 1.0 + float(np.exp(np.float64(-0.125)))
    assert np.allclose(got, want, rtol=1e-15)
    assert abs(float(capi.survival_levels(-np.expm1(-0.375))[0]) - 0.375) < 1e-15
    assert (est.predict_quantile(X, -np.expm1(-0.3)) == 3.0).all()  # hz[g] = (g + 1) / 8 first reaches 0.3 at ut[2]
    none = _fitted()
    none.beta = np.zeros(5)
    none.baseline_times_, none.baseline_cumhaz_ = np.zeros(0), np.zeros(0)  # J = 0
    assert (none.predict_rmst(X, [0.0, 2.5]) == [0.0, 2.5]).all() and np.isinf(none.predict_quantile(X)).all()
    assert (est.predict_quantile(X, -np.expm1(-2.0)) == np.inf).all()  # a level above hz[J - 1] = 1
