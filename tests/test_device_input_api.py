"""X already in GPU memory: what needs no GPU -- the new entry points are exported, declared and listed, and a device
object that the ingest kernel cannot take raises ValueError before the library is asked for a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from bess_amd import capi, linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_session_create_device", "bessx_session_set_responses_device", "bessx_pywrap_bess_device",
       "bessx_op_ingest", "bessx_op_ingest_bench")


class FakeDevice:
    """Stand-in for a device array: only the attribute capi looks at.  The pointer is never dereferenced."""

    def __init__(self, shape, typestr="<f8", strides=None, ptr=1 << 20):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False),
                                         "strides": strides, "version": 3}


def test_new_symbols_are_exported_declared_and_listed():
    assert all(n in capi.SYMBOLS for n in NEW)
    lib = os.path.join(ROOT, "bess_amd", "libbessx.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(bessx_\w+)\b", out))
    header = open(os.path.join(ROOT, "include", "bessx.h")).read()
    for n in NEW:
        assert n in exported, n
        assert re.search(r"\bint %s\(" % n, header), n
    assert "bessx_device_input" in header and "BESSX_F32" in header


BAD = [
    (dict(shape=(30,)), "2-D"),
    (dict(shape=(30, 5, 2)), "2-D"),
    (dict(shape=(30, 5), typestr="<i4"), "float64 or float32"),
    (dict(shape=(30, 5), typestr=">f8"), "float64 or float32"),
    (dict(shape=(30, 5), typestr="<f2"), "float64 or float32"),
    (dict(shape=(30, 5), strides=(-40, 8)), "strides"),
    (dict(shape=(30, 5), strides=(40, 4)), "strides"),
    (dict(shape=(30, 5), typestr="<f4", strides=(20, 6)), "strides"),
    (dict(shape=(0, 5)), "empty"),
    (dict(shape=(30, 5), ptr=0), "null"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_bad_device_objects_raise_before_any_device_call(kw, msg, monkeypatch):
    def no_library():
        raise AssertionError("the library was asked before the argument check")
    monkeypatch.setattr(capi, "lib", no_library)
    x = FakeDevice(**kw)
    y = np.zeros(30)
    with pytest.raises(ValueError, match=msg):
        capi.Session(x, y)
    with pytest.raises(ValueError, match=msg):
        capi.pywrap_bess(x, y, 1, np.ones(30), True, 1, 1, 20, 0, 1, True, 4, False, 5, range(5), np.ones(30), [1, 2],
                         [0.0], 0, 0, 0, 1e-4, 0, 0, 100, False, 1, 1, [], 0.0, 5)
    with pytest.raises(ValueError, match=msg):
        linear.PdasLm(sequence=[1, 2]).fit(x, y)


def test_row_counts_are_checked_before_any_device_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked before the argument check")
    monkeypatch.setattr(capi, "lib", no_library)
    x = FakeDevice((30, 5), "<f4")
    with pytest.raises(ValueError, match=r"X\.shape\(0\) should be equal to y\.size"):
        capi.Session(x, np.zeros(29))
    with pytest.raises(ValueError, match=r"X\.shape\(0\) should be equal to y\.size"):
        capi.Session(x, FakeDevice((31,)))
    with pytest.raises(ValueError, match=r"weight\.size"):
        capi.Session(x, np.zeros(30), weight=np.ones(7))
    with pytest.raises(ValueError, match="vector"):
        capi.Session(x, FakeDevice((15, 2)))
    with pytest.raises(ValueError, match="permutation"):
        capi.Session(x, np.zeros(30), row_order=np.zeros(30, dtype=np.int32))
    with pytest.raises(ValueError, match="permutation"):
        capi.Session(x, np.zeros(30), row_order=np.arange(29))
    with pytest.raises(ValueError, match=r"X\.shape\(0\) should be equal to y\.size"):
        linear.PdasLm(sequence=[1, 2]).fit(x, np.zeros(29))


def test_strides_become_element_strides():
    d = capi._DeviceArray(FakeDevice((30, 5), "<f4", strides=(40, 8)), "x", 2)
    assert (d.dtype, d.strides, d.shape) == (1, (10, 2), (30, 5))
    d = capi._DeviceArray(FakeDevice((30, 5)), "x", 2)  # strides None: C-contiguous
    assert (d.dtype, d.strides) == (0, (5, 1))
    assert capi.is_device_array(FakeDevice((3, 3))) and not capi.is_device_array(np.zeros((3, 3)))


def test_device_set_responses_checks_before_the_device(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked before the argument check")
    monkeypatch.setattr(capi, "lib", no_library)
    s = capi.Session.__new__(capi.Session)
    s.n = 10
    with pytest.raises(ValueError, match="shape"):
        s.set_responses(FakeDevice((9, 2)))
    with pytest.raises(ValueError, match="float64 or float32"):
        s.set_responses(FakeDevice((10, 2), "<i8"))


def test_c_entry_points_check_their_arguments_without_a_gpu():
    lib = capi.lib()
    assert lib.bessx_session_create_device(None, None, None) == 1  # BESSX_ERR_ARG
    assert b"null" in lib.bessx_last_error()
    assert lib.bessx_session_set_responses_device(None, None, 0, 1, 1, 1, None) == 1
    assert lib.bessx_op_ingest(None, 0, 1, 1, None, 1, 1, 128, None, None, None) == 1
