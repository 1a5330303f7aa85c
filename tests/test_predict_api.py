"""Prediction on an X already in GPU memory: what needs no GPU -- the new entry points are exported, declared and listed,
bad device objects and bad models raise ValueError before the library is asked for a device, host X never reaches the
library, and the C entry refuses to compute without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bess_amd import capi, linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_predict_device", "bessx_op_predict_bench")


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
    for name in ("BESSX_LINK_IDENTITY", "BESSX_LINK_LOGISTIC", "BESSX_LINK_POISSON"):
        assert name in header


BAD = [
    (dict(shape=(30,)), "2-D"),
    (dict(shape=(30, 5, 2)), "2-D"),
    (dict(shape=(30, 5), typestr="<i4"), "float64 or float32"),
    (dict(shape=(30, 5), strides=(-40, 8)), "strides"),
    (dict(shape=(0, 5)), "empty"),
    (dict(shape=(30, 5), ptr=0), "null"),
    (dict(shape=(30, 6)), r"X\.shape\[1\] should be 5"),
]


@pytest.mark.parametrize("cls", [linear.PdasLm, linear.PdasLogistic, linear.PdasPoisson, linear.PdasCox])
@pytest.mark.parametrize("kw,msg", BAD)
def test_predict_rejects_bad_device_objects_before_any_device_call(cls, kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        _fitted(cls).predict(FakeDevice(**kw))


def test_cox_predict_on_a_device_object_is_none_without_a_device_call(monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    assert _fitted(linear.PdasCox).predict(FakeDevice((30, 5))) is None


BAD_MODEL = [
    (dict(cols=[3, 1], B=[1.0, 2.0], coef0=[0.0]), "ascending"),
    (dict(cols=[1, 1], B=[1.0, 2.0], coef0=[0.0]), "ascending"),
    (dict(cols=[1, 5], B=[1.0, 2.0], coef0=[0.0]), r"\[0, 5\)"),
    (dict(cols=[-1, 2], B=[1.0, 2.0], coef0=[0.0]), r"\[0, 5\)"),
    (dict(cols=[1, 3], B=[1.0, 2.0, 3.0], coef0=[0.0]), "B must have shape"),
    (dict(cols=[1, 3], B=np.ones((3, 2)), coef0=[0.0, 0.0]), "B must have shape"),
    (dict(cols=[1, 3], B=np.ones((2, 2)), coef0=[0.0]), "coef0"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], link="probit"), "link"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], out=FakeDevice((29,))), "out must have shape"),
    (dict(cols=[1, 3], B=np.ones((2, 2)), coef0=[0.0, 0.0], out=FakeDevice((30, 3))), "out must have shape"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], out=FakeDevice((30,), "<f4")), "float64"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], out=FakeDevice((30,), "<i8")), "float64"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], out=np.zeros(30)), "device array"),
    (dict(cols=[1, 3], B=[1.0, 2.0], coef0=[0.0], link="logistic", out=FakeDevice((30,))), "pair"),
]


@pytest.mark.parametrize("kw,msg", BAD_MODEL)
def test_predict_device_rejects_bad_models_before_the_library(kw, msg, monkeypatch):
    monkeypatch.setattr(capi, "lib", _no_library)
    with pytest.raises(ValueError, match=msg):
        capi.predict_device(FakeDevice((30, 5)), **kw)


def test_host_x_never_reaches_the_library(monkeypatch):
    def no_device_route(*a, **k):
        raise AssertionError("a host X was sent to the device route")
    monkeypatch.setattr(capi, "lib", _no_library)
    monkeypatch.setattr(capi, "predict_device", no_device_route)  # (the entry exists, and host X does not take it)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((30, 5))
    lm = _fitted(linear.PdasLm)
    eta = X @ lm.beta + 0.25
    assert np.array_equal(lm.predict(X), np.dot(X, lm.beta) + np.ones(30) * 0.25)
    got = _fitted(linear.PdasLogistic).predict(X)
    e = np.exp(np.clip(eta, -25, 25))
    assert np.array_equal(got["Y"], (eta > 0).astype(float)) and np.array_equal(got["pr"], e / (e + 1))
    assert np.array_equal(_fitted(linear.PdasPoisson).predict(X)["lam"], np.exp(eta))
    assert _fitted(linear.PdasCox).predict(X) is None
    multi = _fitted(linear.PdasLm)
    multi.beta, multi.coef0 = rng.standard_normal((5, 3)), np.array([1.0, 2.0, 3.0])
    assert np.array_equal(multi.predict(X), np.dot(X, multi.beta) + multi.coef0[None, :])
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 5"):
        lm.predict(rng.standard_normal((30, 6)))


def test_c_entry_checks_its_arguments_without_a_gpu():
    lib = capi.lib()
    x = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below fails in the argument checks
    B, c0 = np.array([1.0, 2.0]), np.array([0.5])
    out = np.zeros(30)

    def call(cols, m=2, x=x, R=1, link=0, rs=5, cs=1, ors=1, ocs=1, out=out, out2=None, B=B, c0=c0):
        cols = np.asarray(cols, dtype=np.int32)
        return lib.bessx_predict_device(x, 0, rs, cs, 30, 5, capi._ip(cols), m, capi._dp(B), capi._dp(c0), R, link,
                                        None if out is None else out.ctypes.data, ors, ocs,
                                        None if out2 is None else out2.ctypes.data, 0, None)

    for bad, word in [(dict(cols=[3, 1]), b"ascending"), (dict(cols=[1, 1]), b"ascending"),
                      (dict(cols=[1, 5]), b"out of range"), (dict(cols=[-1, 2]), b"out of range"),
                      (dict(cols=[1, 3], rs=-5), b"strides"), (dict(cols=[1, 3], ors=-1), b"strides"),
                      (dict(cols=[1, 3], x=None), b"null"), (dict(cols=[1, 3], out=None), b"null"),
                      (dict(cols=[1, 3], c0=None), b"null"), (dict(cols=[1, 3], B=None), b"null"),
                      (dict(cols=[1, 3], R=0), b"R must"), (dict(cols=[1, 3], link=3), b"link"),
                      (dict(cols=[1, 3], link=-1), b"link"), (dict(cols=[1, 3], link=1), b"out2"),
                      (dict(cols=[1, 3], m=6), b"m must")]:
        assert call(**bad) == 1, bad  # BESSX_ERR_ARG
        assert word in lib.bessx_last_error(), (bad, lib.bessx_last_error())
    ms, g = ctypes.c_double(0), ctypes.c_double(0)
    cols = np.array([3, 1], dtype=np.int32)
    assert lib.bessx_op_predict_bench(x, 0, 5, 1, 30, 5, capi._ip(cols), 2, 1, 0, 3, ctypes.byref(ms),
                                      ctypes.byref(g)) == 1


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback_without_gpu():
    lib = capi.lib()
    cols = np.array([1, 3], dtype=np.int32)
    B, c0, out = np.array([1.0, 2.0]), np.array([0.5]), np.zeros(30)
    rc = lib.bessx_predict_device(ctypes.c_void_p(1 << 20), 0, 5, 1, 30, 5, capi._ip(cols), 2, capi._dp(B), capi._dp(c0),
                                  1, 0, out.ctypes.data, 1, 1, None, 0, None)
    assert rc == 2  # BESSX_ERR_HIP
    assert not out.any()
    with pytest.raises(capi.BessxError) as e:
        _fitted(linear.PdasLm).predict(FakeDevice((30, 5)))
    assert e.value.code == 2
