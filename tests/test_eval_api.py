"""Held-out evaluation (bessx_eval_device, capi.evaluate_device / evaluate_candidates, bess_base.evaluate / score): what
needs no GPU -- the new entry points are exported, declared and listed, bad device objects and bad models raise
ValueError before the library is asked for a device, Cox returns None, the C entry refuses to compute without a GPU and
leaves the ledger alone, and the NumPy host route is inside the derived bound (tests/evalref.py) of the longdouble
reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import evalref
from bess_amd import capi, linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_eval_device", "bessx_op_eval_bench")
LD = np.longdouble


class FakeDevice:
    """Stand-in for a device array: only the attribute capi looks at.  The pointer is never dereferenced."""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=1 << 20):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False),
                                         "strides": strides, "version": 3}


def _no_library():
    raise AssertionError("the library was asked before the argument check")


def _fitted(cls=linear.PdasLm, p=5):
    est = cls()
    est.p = p
    est.beta = np.array([0.0, 1.5, 0.0, -2.0, 0.0])[:p]
    est.coef0 = 0.25
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
    assert "bessx_eval_input" in header
    for f in ("evaluate_device", "evaluate_candidates"):
        assert callable(getattr(capi, f))
    for f in ("evaluate", "score"):
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


@pytest.mark.parametrize("cls", [linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson, linear.PdasCox])
@pytest.mark.parametrize("kw,msg", BAD_X)
def test_evaluate_rejects_bad_device_x_before_any_device_call(cls, kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted(cls).evaluate(FakeDevice(**kw), np.zeros(30))
    with pytest.raises(ValueError, match=msg):
        _fitted(cls).score(FakeDevice(**kw), np.zeros(30))


BAD_DATA = [
    (dict(y=np.zeros(29)), r"y\.shape"),
    (dict(y=FakeDevice((29,))), r"y\.shape"),
    (dict(y=np.zeros((30, 2))), "1 column or one per"),
    (dict(y=FakeDevice((30, 3))), "1 column or one per"),
    (dict(y=np.zeros((30, 1, 1))), r"y"),
    (dict(y=FakeDevice((30,), "<i8")), "float64 or float32"),
    (dict(y=np.zeros(30), weight=np.ones(31)), r"weight\.size"),
    (dict(y=np.zeros(30), weight=FakeDevice((29,))), r"weight\.size"),
    (dict(y=FakeDevice((30,)), weight=FakeDevice((30,), "<i4")), "float64 or float32"),
]


@pytest.mark.parametrize("cls", [linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson])
@pytest.mark.parametrize("kw,msg", BAD_DATA)
def test_evaluate_rejects_bad_y_and_weight_before_any_device_call(cls, kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted(cls).evaluate(FakeDevice((30, 5)), **kw)


@pytest.mark.parametrize("kw,msg", BAD_DATA)
def test_evaluate_device_rejects_bad_y_and_weight_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        capi.evaluate_device(FakeDevice((30, 5)), [1, 3], [1.0, 2.0], [0.0], **kw)


BAD_MODEL = [
    (dict(cols=[3, 1], B=[1.0, 2.0], coef0=[0.0]), "ascending"),
    (dict(cols=[1, 1], B=[1.0, 2.0], coef0=[0.0]), "ascending"),
    (dict(cols=[1, 5], B=[1.0, 2.0], coef0=[0.0]), r"\[0, 5\)"),
    (dict(cols=[-1, 2], B=[1.0, 2.0], coef0=[0.0]), r"\[0, 5\)"),
    (dict(cols=[1, 3], B=[1.0, 2.0, 3.0], coef0=[0.0]), "B must have shape"),
    (dict(cols=[1, 3], B=np.ones((2, 2)), coef0=[0.0]), "coef0"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], link="probit"), "link"),
]


@pytest.mark.parametrize("kw,msg", BAD_MODEL)
def test_evaluate_device_rejects_bad_models_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        capi.evaluate_device(FakeDevice((30, 5)), y=np.zeros(30), **kw)


@pytest.mark.parametrize("kw,msg", BAD_X[:6])
def test_evaluate_device_rejects_bad_x_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        capi.evaluate_device(FakeDevice(**kw), [1], [1.0], [0.0], np.zeros(30))


def test_evaluate_candidates_rejects_a_result_without_candidates(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    empty = {"cand_support": np.zeros((0, 3), dtype=np.int32), "cand_beta": np.zeros((0, 3)), "cand_coef0": np.zeros(0)}
    with pytest.raises(ValueError, match="no stored candidates"):
        capi.evaluate_candidates(empty, FakeDevice((30, 5)), np.zeros(30))


def test_candidate_models_builds_the_union_and_the_coefficient_matrix():
    res = {"cand_support": np.array([[3, -1, -1], [1, 3, -1], [0, 3, 4]], dtype=np.int32),
           "cand_beta": np.array([[2.0, 0, 0], [0.5, 1.5, 0], [-1.0, 1.0, 4.0]]), "cand_coef0": np.array([0.1, 0.2, 0.3])}
    cols, B, c = capi.candidate_models(res)
    assert np.array_equal(cols, [0, 1, 3, 4]) and cols.dtype == np.int32
    assert np.array_equal(B, [[0, 0, -1.0], [0, 0.5, 0], [2.0, 1.5, 1.0], [0, 0, 4.0]])
    assert np.array_equal(c, [0.1, 0.2, 0.3])


def test_cox_evaluate_and_score_are_none_without_a_device_call(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    cox = _fitted(linear.PdasCox)
    assert cox.evaluate(FakeDevice((30, 5)), np.zeros((30, 2))) is None
    assert cox.score(FakeDevice((30, 5)), np.zeros((30, 2))) is None
    assert cox.evaluate(np.zeros((30, 5)), np.zeros((30, 2))) is None


def _c_input(**over):
    """A valid bessx_eval_input on a pointer that is never dereferenced, plus the arrays it refers to."""
    cols = np.asarray(over.pop("cols", [1, 3]), dtype=np.int32)
    B, c0, y = np.array([1.0, 2.0]), np.array([0.5]), np.zeros(30)
    a = capi.EvalInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1 << 20, 0, 5, 1, 30, 5
    a.cols, a.m, a.B, a.coef0, a.R, a.link = capi._ip(cols), 2, capi._dp(B), capi._dp(c0), 1, 0
    a.y_host, a.y_row_stride, a.y_col_stride, a.y_cols = capi._dp(y), 1, 0, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a, (cols, B, c0, y)


def test_c_entry_checks_its_arguments_without_a_gpu():
    lib = capi.lib()
    loss, aux, sw = np.zeros(1), np.zeros(1), ctypes.c_double(0)

    def call(aux=aux, **over):
        a, keep = _c_input(**over)
        return lib.bessx_eval_device(ctypes.byref(a), capi._dp(loss), None if aux is None else capi._dp(aux),
                                     ctypes.byref(sw))

    for bad, word in [(dict(cols=[3, 1]), b"ascending"), (dict(cols=[1, 1]), b"ascending"),
                      (dict(cols=[1, 5]), b"out of range"), (dict(cols=[-1, 2]), b"out of range"),
                      (dict(x_row_stride=-5), b"strides"), (dict(y_row_stride=-1), b"strides"),
                      (dict(weight_stride=-1), b"strides"), (dict(x=None), b"null"), (dict(coef0=None), b"null"),
                      (dict(B=None), b"null"), (dict(R=0), b"R must"), (dict(link=3), b"link"), (dict(link=-1), b"link"),
                      (dict(link=1, aux=None), b"aux"), (dict(m=6), b"m must"), (dict(x_dtype=2), b"dtype"),
                      (dict(y_host=None), b"y as a host pointer"), (dict(y_dev=1 << 21), b"y as a host pointer"),
                      (dict(y_cols=2), b"y_cols"), (dict(y_cols=0), b"y_cols"),
                      (dict(y_host=None, y_dev=1 << 21, y_dtype=5), b"dtype"),
                      (dict(weight_dev=1 << 21, weight_dtype=7), b"dtype"), (dict(n=0), b"empty")]:
        assert call(**bad) == 1, bad  # BESSX_ERR_ARG
        assert word in lib.bessx_last_error(), (bad, lib.bessx_last_error())
    assert lib.bessx_eval_device(None, capi._dp(loss), capi._dp(aux), ctypes.byref(sw)) == 1
    ms, g = ctypes.c_double(0), ctypes.c_double(0)
    cols = np.array([3, 1], dtype=np.int32)
    assert lib.bessx_op_eval_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, 1, 0, 1, 3,
                                   ctypes.byref(ms), ctypes.byref(g)) == 1
    cols = np.array([1, 3], dtype=np.int32)
    assert lib.bessx_op_eval_bench(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, 4, 0, 2, 3,
                                   ctypes.byref(ms), ctypes.byref(g)) == 1
    assert b"y_cols" in lib.bessx_last_error()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu_and_the_ledger_is_untouched():
    lib = capi.lib()
    before = capi.process_counters()
    assert set(before) == {"live_device_bytes", "live_pinned_bytes", "allocation_requests"}
    a, keep = _c_input()
    loss, sw = np.zeros(1), ctypes.c_double(0)
    rc = lib.bessx_eval_device(ctypes.byref(a), capi._dp(loss), None, ctypes.byref(sw))
    assert rc == 2  # BESSX_ERR_HIP
    assert not loss.any() and sw.value == 0.0
    with pytest.raises(capi.BessxError) as e:
        _fitted(linear.PdasLm).evaluate(FakeDevice((30, 5)), np.zeros(30))
    assert e.value.code == 2
    with pytest.raises(capi.BessxError) as e:
        capi.op_eval_bench(FakeDevice((30, 5)), [1, 3])
    assert e.value.code == 2
    assert capi.process_counters() == before


# ----------------------------------------------------------------------------------------------------------------
# the NumPy host route against the longdouble reference
# ----------------------------------------------------------------------------------------------------------------
def _host_problem(cls, rng, n, p, m, R=1):
    X = rng.standard_normal((n, p))
    est = cls()
    est.p = p
    beta = np.zeros((p, R))
    for r in range(R):
        beta[rng.choice(p, m, replace=False), r] = rng.standard_normal(m) * 0.7
    est.beta, est.coef0 = (beta[:, 0], float(rng.standard_normal())) if R == 1 else (beta, rng.standard_normal(R))
    eta = X @ beta + np.reshape(est.coef0, (1, -1))
    if cls is linear.PdasLm:
        y = eta + rng.standard_normal((n, R))
    elif cls is linear.PdasLogistic:
        y = (rng.uniform(size=(n, R)) < 1 / (1 + np.exp(-eta))).astype(float)
    else:
        y = rng.poisson(np.exp(np.clip(eta, -5, 3))).astype(float)
    return est, X, (y[:, 0] if R == 1 else y)


LINK = {linear.PdasLm: "identity", linear.PdasLogistic: "logistic", linear.PdasPoisson: "poisson"}


def _reference_for(est, X, y, w):
    beta = np.asarray(est.beta).reshape(X.shape[1], -1)
    cols = np.nonzero(beta.any(axis=1))[0]
    eta, delta = evalref.eta_reference(X, cols, beta[cols], np.reshape(est.coef0, -1))
    return evalref.loss_reference(eta, delta, y, w, LINK[type(est)])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cls,R", [(linear.PdasLm, 1), (linear.PdasLm, 6), (linear.PdasLogistic, 1),
                                   (linear.PdasPoisson, 1)])
def test_host_route_is_inside_the_bound_of_the_longdouble_reference(cls, R, weighted, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)  # (a NumPy X never touches the library)
    rng = np.random.default_rng(11 + R + 100 * weighted)
    n = 4097
    est, X, y = _host_problem(cls, rng, n, 60, 9, R)
    w = rng.integers(1, 17, n) / 8.0 if weighted else None
    ref = _reference_for(est, X, y, w)
    got = est.evaluate(X, y, weight=w)
    evalref.check_loss(got["loss"], ref, "%s R=%d weighted=%s" % (cls.__name__, R, weighted))
    sw = np.asarray(got["n_eff"], dtype=LD).reshape(-1)
    assert (np.abs(sw - ref["sum_w"]) <= ref["sum_w_bound"]).all()
    if not weighted:
        assert (np.asarray(got["n_eff"]).reshape(-1) == n).all()
    shape = () if R == 1 else (R,)
    for k, v in got.items():
        assert np.shape(v) == shape, k
        assert isinstance(v, float) if R == 1 else isinstance(v, np.ndarray)
    L, S = np.asarray(got["loss"]).reshape(-1), np.asarray(got["n_eff"]).reshape(-1)
    if cls is linear.PdasLm:
        wl = np.ones(n) if w is None else w
        Y = np.reshape(y, (n, -1))
        ybar = (wl[:, None] * Y).sum(axis=0) / wl.sum()
        tss = (wl[:, None] * (Y - ybar) ** 2).sum(axis=0)
        assert np.allclose(np.reshape(got["mse"], -1), L / S, rtol=1e-14)
        assert np.allclose(np.reshape(got["r2"], -1), 1 - L / tss, rtol=1e-12)
        assert np.array_equal(np.reshape(est.score(X, y, weight=w), -1), np.reshape(got["r2"], -1))
    elif cls is linear.PdasLogistic:
        evalref.label_precondition(ref)
        assert got["deviance"] == 2.0 * got["loss"]
        assert got["accuracy"] == float(ref["correct"][0]) / float(ref["sum_w"])  # (weights are multiples of 1/8: exact)
        assert est.score(X, y, weight=w) == got["accuracy"]
    else:
        assert est.score(X, y, weight=w) == got["d2"]
        assert got["d2"] < 1.0 and got["deviance"] > 0.0


def test_r2_is_one_for_an_exact_fit_and_zero_for_the_mean():
    rng = np.random.default_rng(5)
    X = rng.integers(-4, 5, (64, 5)).astype(float)
    est = _fitted(linear.PdasLm)
    y = X @ est.beta + 0.25  # (small integers and quarters: exact in fp64)
    got = est.evaluate(X, y)
    assert got == {"loss": 0.0, "n_eff": 64.0, "mse": 0.0, "r2": 1.0}
    assert est.score(X, y) == 1.0
    flat = _fitted(linear.PdasLm)
    flat.beta, flat.coef0 = np.zeros(5), float(y.mean())
    assert abs(flat.score(X, y)) < 1e-14


def test_d2_and_accuracy_on_a_tiny_hand_computed_case():
    # one column, beta = log 2, no intercept: eta = (0, log 2, 2 log 2), mu = (1, 2, 4); y = (1, 1, 6)
    X = np.array([[0.0], [1.0], [2.0]])
    y = np.array([1.0, 1.0, 6.0])
    po = linear.PdasPoisson()
    po.p, po.beta, po.coef0 = 1, np.array([np.log(2.0)]), 0.0
    got = po.evaluate(X, y)
    l2, l6 = np.log(2.0), np.log(6.0)
    loss = (1 - 0) + (2 - l2) + (4 - 6 * 2 * l2)  # sum mu - y eta
    dev = 2 * ((0 - (1 - 1)) + (1 * np.log(1 / 2) - (1 - 2)) + (6 * np.log(6 / 4) - (6 - 4)))  # 2 sum y log(y/mu) - (y - mu)
    ybar = 8.0 / 3.0
    null = 2 * (2 * np.log(1 / ybar) + 6 * np.log(6 / ybar))
    assert np.isclose(got["loss"], loss, rtol=1e-14) and got["n_eff"] == 3.0
    assert np.isclose(got["deviance"], dev, rtol=1e-12) and np.isclose(got["d2"], 1 - dev / null, rtol=1e-12)
    assert np.isclose(got["deviance"], 2 * (loss + 6 * l6 - 8.0), rtol=1e-12)
    # a zero count: 0 log 0 = 0
    z = po.evaluate(X, np.array([0.0, 1.0, 6.0]))
    assert np.isfinite(z["deviance"]) and np.isclose(z["deviance"], 2 * ((1 - 0) + (2 - l2) + (4 - 12 * l2) + 6 * l6 - 7.0))
    # logistic: eta = (-1, 1, 3, -2) against y = (0, 1, 0, 1): two of four right; weights (1, 2, 1, 4): 3 of 8
    lo = linear.PdasLogistic()
    lo.p, lo.beta, lo.coef0 = 1, np.array([1.0]), 0.0
    Xl, yl = np.array([[-1.0], [1.0], [3.0], [-2.0]]), np.array([0.0, 1.0, 0.0, 1.0])
    got = lo.evaluate(Xl, yl)
    sp = lambda t: np.log1p(np.exp(t))  # noqa: E731
    assert got["accuracy"] == 0.5 and lo.score(Xl, yl) == 0.5
    assert np.isclose(got["loss"], sp(-1) + (sp(1) - 1) + sp(3) + (sp(-2) + 2), rtol=1e-14)
    assert got["deviance"] == 2 * got["loss"]
    assert lo.score(Xl, yl, weight=np.array([1.0, 2.0, 1.0, 4.0])) == 3.0 / 8.0


@pytest.mark.parametrize("link", ["identity", "logistic", "poisson"])
def test_the_bound_rejects_a_loss_perturbed_by_1e_minus_10(link):
    """Without this a slack bound would go unnoticed: at n = 4097 a relative change of 1e-10 must fall outside."""
    cls = {v: k for k, v in LINK.items()}[link]
    rng = np.random.default_rng(77)
    est, X, y = _host_problem(cls, rng, 4097, 60, 9)
    w = rng.integers(1, 17, 4097) / 8.0
    ref = _reference_for(est, X, y, w)
    exact = ref["loss"].astype(np.float64)
    assert evalref.within(exact, ref).all()
    assert not evalref.within(exact * (1 + 1e-10), ref).any()
    assert not evalref.within(exact * (1 - 1e-10), ref).any()
    assert not evalref.within(np.full(1, np.nan), ref).any()
