"""Held-out Cox evaluation (bessx_eval_cox_device, capi.evaluate_cox_device / evaluate_cox_candidates,
bess_base.linear_predictor / evaluate_survival / concordance): what needs no GPU -- the new entry points are exported,
declared and listed, bad arguments raise ValueError before the library is asked for a device, the C entry refuses to
compute without a GPU and leaves the ledger alone, and the NumPy route is inside the derived bound
(tests/coxevalref.py) of the longdouble reference with counts that equal the O(n^2) integer reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coxevalref
import evalref
from bess_amd import capi, linear, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_eval_cox_device", "bessx_op_cox_eval_bench")
LD = np.longdouble


class FakeDevice:
    """Stand-in for a device array: only the attribute capi looks at.  The pointer is never dereferenced."""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=1 << 20):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False),
                                         "strides": strides, "version": 3}


def _no_library():
    raise AssertionError("the library was asked before the argument check")


def _fitted(cls=linear.PdasCox, p=5):
    est = cls()
    est.p = p
    est.beta = np.array([0.0, 1.5, 0.0, -2.0, 0.0])[:p]
    est.coef0 = 0.0 if cls is linear.PdasCox else 0.25
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
    assert "bessx_cox_eval_input" in header
    for f in ("evaluate_cox_device", "evaluate_cox_candidates", "op_cox_eval_bench"):
        assert callable(getattr(capi, f))
    for f in ("linear_predictor", "evaluate_survival", "concordance"):
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
def test_estimator_rejects_bad_device_x_before_any_device_call(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted().evaluate_survival(FakeDevice(**kw), np.zeros((30, 2)))
    with pytest.raises(ValueError, match=msg):
        _fitted().concordance(FakeDevice(**kw), np.zeros((30, 2)))
    with pytest.raises(ValueError, match=msg):
        _fitted().linear_predictor(FakeDevice(**kw))


@pytest.mark.parametrize("shape", [(30,), (30, 5, 2), (30, 6), ()])
def test_estimator_rejects_a_numpy_x_of_the_wrong_shape_with_the_same_message(shape, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for call in (lambda X: _fitted().evaluate_survival(X, np.zeros((30, 2))),
                 lambda X: _fitted().concordance(X, np.zeros((30, 2))), lambda X: _fitted().linear_predictor(X)):
        with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
            call(np.zeros(shape))


BAD_DATA = [
    (dict(y=np.zeros(30)), r"\(30, 2\)"),
    (dict(y=np.zeros((29, 2))), r"\(30, 2\)"),
    (dict(y=np.zeros((30, 3))), r"\(30, 2\)"),
    (dict(y=FakeDevice((30,))), r"\(30, 2\)"),
    (dict(y=FakeDevice((30, 1))), r"\(30, 2\)"),
    (dict(y=FakeDevice((30, 2), "<i8")), "float64 or float32"),
    (dict(y=np.zeros((30, 2)), weight=np.ones(31)), r"weight\.size"),
    (dict(y=np.zeros((30, 2)), weight=FakeDevice((29,))), r"weight\.size"),
    (dict(y=FakeDevice((30, 2)), weight=FakeDevice((30,), "<i4")), "float64 or float32"),
    (dict(y=np.zeros((30, 2)), ties="efron"), "ties"),
    (dict(y=FakeDevice((30, 2)), ties="efron"), "ties"),
]


@pytest.mark.parametrize("kw,msg", BAD_DATA)
def test_evaluate_survival_rejects_bad_y_weight_and_ties_before_any_device_call(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted().evaluate_survival(FakeDevice((30, 5)), **kw)
    if not any(capi.is_device_array(v) for v in kw.values()):
        with pytest.raises(ValueError, match=msg):
            _fitted().evaluate_survival(np.zeros((30, 5)), **kw)


BAD_VECTORS = [
    (dict(time=np.zeros(29)), r"time\.size"),
    (dict(time=FakeDevice((31,))), r"time\.size"),
    (dict(status=np.zeros(31)), r"status\.size"),
    (dict(status=FakeDevice((30,), "<i4")), "float64 or float32"),
    (dict(weight=np.ones(3)), r"weight\.size"),
    (dict(weight=FakeDevice((29,))), r"weight\.size"),
    (dict(ties="efron"), "ties"),
    (dict(time=np.full(30, np.nan)), "NAN"),
    (dict(status=np.full(30, 2.0)), "0 or 1"),
]


@pytest.mark.parametrize("kw,msg", BAD_VECTORS)
def test_evaluate_cox_device_rejects_bad_vectors_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    args = dict(time=np.arange(30.0), status=np.ones(30))
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        capi.evaluate_cox_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], **args)


BAD_MODEL = [
    (dict(cols=[3, 1], B=[1.0, 2.0]), "ascending"),
    (dict(cols=[1, 1], B=[1.0, 2.0]), "ascending"),
    (dict(cols=[1, 5], B=[1.0, 2.0]), r"\[0, 5\)"),
    (dict(cols=[-1, 2], B=[1.0, 2.0]), r"\[0, 5\)"),
    (dict(cols=[1, 3], B=[1.0, 2.0, 3.0]), "B must have shape"),
    (dict(cols=[1, 3], B=np.ones((3, 2))), "B must have shape"),
]


@pytest.mark.parametrize("kw,msg", BAD_MODEL)
def test_evaluate_cox_device_rejects_bad_models_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        capi.evaluate_cox_device(FakeDevice((30, 5)), time=np.arange(30.0), status=np.ones(30), **kw)


@pytest.mark.parametrize("kw,msg", BAD_X[:6])
def test_evaluate_cox_device_rejects_bad_x_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        capi.evaluate_cox_device(FakeDevice(**kw), [1], [1.0], np.arange(30.0), np.ones(30))


def test_evaluate_cox_candidates_rejects_a_result_without_candidates(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    empty = {"cand_support": np.zeros((0, 3), dtype=np.int32), "cand_beta": np.zeros((0, 3)), "cand_coef0": np.zeros(0)}
    with pytest.raises(ValueError, match="no stored candidates"):
        capi.evaluate_cox_candidates(empty, FakeDevice((30, 5)), np.arange(30.0), np.ones(30))


def test_survival_methods_raise_on_estimators_that_are_not_cox(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    for cls in (linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson):
        for X in (np.zeros((30, 5)), FakeDevice((30, 5))):
            with pytest.raises(ValueError, match="Cox"):
                _fitted(cls).evaluate_survival(X, np.zeros((30, 2)))
            with pytest.raises(ValueError, match="Cox"):
                _fitted(cls).concordance(X, np.zeros((30, 2)))


def _c_input(**over):
    """A valid bessx_cox_eval_input on a pointer that is never dereferenced, plus the arrays it refers to."""
    cols = np.asarray(over.pop("cols", [1, 3]), dtype=np.int32)
    time = np.asarray(over.pop("time_values", np.arange(30.0)))
    status = np.asarray(over.pop("status_values", np.ones(30)))
    B = np.array([1.0, 2.0])
    a = capi.CoxEvalInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1 << 20, 0, 5, 1, 30, 5
    a.cols, a.m, a.B, a.R = capi._ip(cols), 2, capi._dp(B), 1
    a.time, a.status, a.ties, a.want_pairs = capi._dp(time), capi._dp(status), 0, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a, (cols, B, time, status)


def test_c_entry_checks_its_arguments_without_a_gpu():
    lib = capi.lib()
    ll, pairs, comp = np.zeros(1), np.zeros(3, dtype=np.int64), ctypes.c_longlong(0)
    pp = pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))

    def call(pairs=pp, **over):
        a, keep = _c_input(**over)
        return lib.bessx_eval_cox_device(ctypes.byref(a), capi._dp(ll), pairs, ctypes.byref(comp))

    nan_time = np.arange(30.0)
    nan_time[7] = np.nan
    for bad, word in [(dict(cols=[3, 1]), b"ascending"), (dict(cols=[1, 1]), b"ascending"),
                      (dict(cols=[1, 5]), b"out of range"), (dict(cols=[-1, 2]), b"out of range"),
                      (dict(x_row_stride=-5), b"strides"), (dict(x_col_stride=-1), b"strides"), (dict(x=None), b"null"),
                      (dict(time=None), b"null"), (dict(status=None), b"null"), (dict(B=None), b"null"),
                      (dict(R=0), b"R must"), (dict(R=70000), b"R must"), (dict(m=6), b"m must"),
                      (dict(x_dtype=2), b"dtype"), (dict(n=0), b"empty"), (dict(ties=2), b"ties"),
                      (dict(ties=-1), b"ties"), (dict(pairs=None), b"pairs"), (dict(time_values=nan_time), b"NaN"),
                      (dict(status_values=np.full(30, 0.5)), b"status")]:
        assert call(**bad) == 1, bad  # BESSX_ERR_ARG
        assert word in lib.bessx_last_error(), (bad, lib.bessx_last_error())
    assert lib.bessx_eval_cox_device(None, capi._dp(ll), pp, ctypes.byref(comp)) == 1
    ms = np.zeros(3)
    cols = np.array([3, 1], dtype=np.int32)
    assert lib.bessx_op_cox_eval_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, 1, 0, 1, 3,
                                       capi._dp(ms)) == 1
    assert b"ascending" in lib.bessx_last_error()
    cols = np.array([1, 3], dtype=np.int32)
    assert lib.bessx_op_cox_eval_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, 1, 5, 1, 3,
                                       capi._dp(ms)) == 1
    assert b"ties" in lib.bessx_last_error()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu_and_the_ledger_is_untouched():
    lib = capi.lib()
    before = capi.process_counters()
    a, keep = _c_input()
    ll, pairs, comp = np.zeros(1), np.zeros(3, dtype=np.int64), ctypes.c_longlong(0)
    rc = lib.bessx_eval_cox_device(ctypes.byref(a), capi._dp(ll), pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                   ctypes.byref(comp))
    assert rc == 2  # BESSX_ERR_HIP
    assert not ll.any() and not pairs.any() and comp.value == 0
    y = np.column_stack([np.arange(30.0), np.ones(30)])
    with pytest.raises(capi.BessxError) as e:
        _fitted().evaluate_survival(FakeDevice((30, 5)), y)
    assert e.value.code == 2
    with pytest.raises(capi.BessxError) as e:
        capi.evaluate_cox_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], y[:, 0], y[:, 1], concordance=False)
    assert e.value.code == 2
    with pytest.raises(capi.BessxError) as e:
        capi.op_cox_eval_bench(FakeDevice((30, 5)), [1, 3])
    assert e.value.code == 2
    assert capi.process_counters() == before


# ----------------------------------------------------------------------------------------------------------------
# the NumPy route against the longdouble reference
# ----------------------------------------------------------------------------------------------------------------
def _cox_problem(n, p, m, seed):
    """make_cox rows in a shuffled order (the estimator has to sort them), m random support columns with N(0, 0.25)
    coefficients, weights that are multiples of 1/8."""
    X, obs, status, _, _ = synth.make_cox(n, p, 3, seed=seed)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    X, obs, status = np.ascontiguousarray(X[perm]), obs[perm], status[perm]
    est = linear.PdasCox()
    est.p, est.coef0 = p, 0.0
    est.beta = np.zeros(p)
    est.beta[rng.choice(p, m, replace=False)] = rng.normal(0.0, 0.5, m)
    w = rng.integers(1, 17, n) / 8.0
    return est, X, obs, status, w


def _reference(est, X, time, status, w, ties):
    cols = np.nonzero(est.beta)[0]
    B = est.beta[cols].reshape(-1, 1)
    eta, delta = evalref.eta_reference(X, cols, B, [0.0])
    ref = coxevalref.loglik_reference(eta, delta, time, status, w, ties)
    gap = coxevalref.count_precondition(X, cols, B, eta, delta, time, status)
    return ref, coxevalref.pair_counts(eta, time, status), gap


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ties", ["order", "breslow"])
def test_numpy_route_is_inside_the_bound_and_its_counts_are_exact(ties, weighted, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)  # (a NumPy X never touches the library)
    n = 513
    est, X, time, status, w = _cox_problem(n, 16, 3, seed=84)
    w = w if weighted else None
    ref, counts, gap = _reference(est, X, time, status, w, ties)
    print("smallest gap / required gap %.3e" % gap)
    got = est.evaluate_survival(X, np.column_stack([time, status]), weight=w, ties=ties)
    coxevalref.check_loglik([got["loglik"]], ref, "numpy n=%d %s weighted=%s" % (n, ties, weighted))
    coxevalref.check_counts(got, counts)
    assert got["deviance"] == -2.0 * got["loglik"]
    assert got["n_events"] == float(np.sum((np.ones(n) if w is None else w) * status))  # (multiples of 1/8: exact)
    assert got["c_index"] == (counts["concordant"][0] + 0.5 * counts["tied_risk"][0]) / counts["comparable"]
    assert est.concordance(X, np.column_stack([time, status])) == got["c_index"]
    for k in ("loglik", "deviance", "n_events", "c_index"):
        assert type(got[k]) is float, k
    for k in ("comparable", "concordant", "discordant", "tied_risk"):
        assert type(got[k]) is int, k
    assert set(got) == {"loglik", "deviance", "n_events", "comparable", "concordant", "discordant", "tied_risk",
                        "c_index"}
    # the bound is not slack: a relative change of 1e-10 falls outside
    exact = ref["loglik"].astype(np.float64)
    assert coxevalref.within(exact, ref).all()
    assert not coxevalref.within(exact * (1 + 1e-10), ref).any()
    assert not coxevalref.within(np.full(1, np.nan), ref).any()


def test_a_hand_made_case_with_a_time_tie_and_identical_rows(monkeypatch):
    """One column, beta = log 2, so e = 2^x.  Rows as given (x, time, status):
        C (2, 2, 0)   A (1, 1, 1)   F (1, 5, 1)   B (0, 2, 1)   E (0, 4, 0)   D (1, 3, 1)
    The stable order by time is A, C, B, D, E, F (C stands before B among the rows, so the censored C keeps its place in
    front of the event B at the tied time 2).  e by position: 2, 4, 1, 2, 1, 2; suffix sums S: 12, 10, 6, 5, 3, 2.
    Events: A, B, D, F with a = log 2, 0, log 2, log 2.
        "order":    loglik = (log 2 - log 12) + (0 - log 6) + (log 2 - log 5) + (log 2 - log 2) = log(4 / 360) = -log 90
        "breslow":  B's risk set starts at C: S = 10 instead of 6:                 loglik = log(4 / 600) = -log 150
    Comparable pairs (an event against every row with a strictly later time), with x in brackets:
        A[1]: C[2] discordant, B[0] concordant, D[1] tied, E[0] concordant, F[1] tied
        B[0]: D[1] discordant, E[0] tied, F[1] discordant          (C has B's time: not comparable)
        D[1]: E[0] concordant, F[1] tied
    comparable 10, concordant 3, discordant 3, tied_risk 4 (A, D and F are identical rows: exact ties),
    c_index = (3 + 4 / 2) / 10 = 0.5.
    The closed forms hold for beta = log 2, the fitted beta is fl(log 2): |beta - log 2| <= u log 2.  The derivative of an
    event's term a_k - log S_k in beta is x_k - (the e-weighted mean of x over its risk set), two numbers in [0, 2], so at
    most 2 in magnitude: the longdouble reference lies within 2 (sum of w delta) u log 2 of the closed form, 8 u log 2
    for the four unweighted events and 10 u log 2 with B's weight doubled (the second order in u and the reference's own
    rounding, 2^-11 of this, are left out as in coxevalref).  This figure checks the reference against the hand
    calculation; the code under test is held to the reference's derived bound."""
    monkeypatch.setattr(capi, "lib", _no_library)
    X = np.array([[2.0], [1.0], [1.0], [0.0], [0.0], [1.0]])
    y = np.array([[2.0, 0.0], [1.0, 1.0], [5.0, 1.0], [2.0, 1.0], [4.0, 0.0], [3.0, 1.0]])
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = 1, np.array([np.log(2.0)]), 0.0
    eta, delta = evalref.eta_reference(X, [0], est.beta.reshape(1, 1), [0.0])
    want = {"order": -np.log(LD(90)), "breslow": -np.log(LD(150))}
    got = {}
    for ties in ("order", "breslow"):
        ref = coxevalref.loglik_reference(eta, delta, y[:, 0], y[:, 1], None, ties)
        assert abs(ref["loglik"][0] - want[ties]) <= 2 * 4 * evalref.U * np.log(LD(2))
        got[ties] = est.evaluate_survival(X, y, ties=ties)
        coxevalref.check_loglik([got[ties]["loglik"]], ref, "hand-made " + ties)
        assert (got[ties]["comparable"], got[ties]["concordant"], got[ties]["discordant"], got[ties]["tied_risk"]) == (
            10, 3, 3, 4)
        assert got[ties]["c_index"] == 0.5 and got[ties]["n_events"] == 4.0
    assert got["order"]["loglik"] != got["breslow"]["loglik"] and got["order"]["tied_risk"] >= 1
    coxevalref.count_precondition(X, [0], est.beta.reshape(1, 1), eta, delta, y[:, 0], y[:, 1])
    assert coxevalref.pair_counts(eta, y[:, 0], y[:, 1])["tied_risk"][0] == 4
    # weights multiply the terms only: doubling B's weight adds B's term once more
    w = np.array([1.0, 1.0, 1.0, 2.0, 1.0, 1.0])
    ref = coxevalref.loglik_reference(eta, delta, y[:, 0], y[:, 1], w, "order")
    assert abs(ref["loglik"][0] - (want["order"] - np.log(LD(6)))) <= 2 * 5 * evalref.U * np.log(LD(2))
    coxevalref.check_loglik([est.evaluate_survival(X, y, weight=w)["loglik"]], ref, "hand-made weighted")


def test_the_null_model_has_its_closed_form_and_a_c_index_of_one_half(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    n = 513
    est, X, time, status, _ = _cox_problem(n, 16, 3, seed=84)
    est.beta = np.zeros(16)
    eta, delta = evalref.eta_reference(X, [], np.zeros((0, 1)), [0.0])
    ref = coxevalref.loglik_reference(eta, delta, time, status, None, "order")
    d = status[np.argsort(time, kind="stable")]
    closed = -(d.astype(LD) * np.log((n - np.arange(n)).astype(LD))).sum()
    assert abs(ref["loglik"][0] - closed) <= ref["bound"][0]
    got = est.evaluate_survival(X, np.column_stack([time, status]))
    assert abs(LD(got["loglik"]) - closed) <= ref["bound"][0]
    assert got["c_index"] == 0.5 and got["concordant"] == got["discordant"] == 0
    assert got["tied_risk"] == got["comparable"] > 0


def test_no_event_and_a_single_row_are_not_errors(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    est, X, time, status, _ = _cox_problem(64, 16, 3, seed=84)
    cols = np.nonzero(est.beta)[0]
    eta, delta = evalref.eta_reference(X, cols, est.beta[cols].reshape(-1, 1), [0.0])
    ref = coxevalref.loglik_reference(eta, delta, time, np.zeros(64), None, "order")
    assert ref["loglik"][0] == 0 and ref["bound"][0] == 0  # (no event: no term)
    got = est.evaluate_survival(X, np.column_stack([time, np.zeros(64)]))
    coxevalref.check_loglik([got["loglik"]], ref, "no event")
    assert got["comparable"] == 0 and np.isnan(got["c_index"]) and got["n_events"] == 0.0
    ref = coxevalref.loglik_reference(eta[:1], delta[:1], [2.5], [1.0], None, "order")
    one = est.evaluate_survival(X[:1], np.array([[2.5, 1.0]]))
    coxevalref.check_loglik([one["loglik"]], ref, "one row")  # (a - log exp(a): zero but for the rounding)
    assert one["comparable"] == 0 and np.isnan(one["c_index"])


def test_linear_predictor_on_numpy_is_x_beta_plus_coef0_bit_for_bit():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 5))
    for cls in (linear.PdasCox, linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson):
        est = _fitted(cls)
        got = est.linear_predictor(X)
        assert isinstance(got, np.ndarray) and got.shape == (200,)
        assert np.array_equal(got, X @ est.beta + est.coef0)
    multi = linear.PdasLm()
    multi.p, multi.beta, multi.coef0 = 5, rng.standard_normal((5, 3)), rng.standard_normal(3)
    assert np.array_equal(multi.linear_predictor(X), X @ multi.beta + multi.coef0)
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
        _fitted().linear_predictor(np.zeros((3, 6)))
