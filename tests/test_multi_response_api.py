"""Argument checks of the multi-response entry points that need no GPU: they raise before any device call."""
import os
import re
import subprocess

import numpy as np
import pytest

from bess_amd import capi, linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bessx_session_set_responses", "bessx_session_sequential_path_multi")


def test_row_count_of_a_2d_response_has_its_own_message():
    X = np.random.default_rng(0).standard_normal((30, 5))
    with pytest.raises(ValueError, match=r"y\.shape\(0\)"):
        linear.PdasLm(sequence=[1, 2]).fit(X, np.zeros((29, 3)))


def test_nan_in_a_2d_response():
    X = np.random.default_rng(0).standard_normal((30, 5))
    Y = np.zeros((30, 3))
    Y[4, 2] = np.nan
    with pytest.raises(ValueError, match="There is NAN value in y"):
        linear.PdasLm(sequence=[1, 2]).fit(X, Y)


@pytest.mark.parametrize("cls", [linear.PdasLogistic, linear.PdasPoisson])
def test_other_families_keep_rejecting_a_2d_response(cls):
    X = np.random.default_rng(0).standard_normal((30, 5))
    with pytest.raises(ValueError, match=r"X\.shape\(0\) should be equal to y\.size"):
        cls(sequence=[1, 2]).fit(X, np.zeros((30, 3)))


def test_set_responses_checks_before_the_device():
    s = capi.Session.__new__(capi.Session)  # (no device session: the checks come first)
    s.n = 10
    with pytest.raises(ValueError, match="NaN"):
        s.set_responses(np.full((10, 2), np.nan))
    with pytest.raises(ValueError, match="shape"):
        s.set_responses(np.zeros((9, 2)))
    with pytest.raises(ValueError, match="set_responses first"):
        s.sequential_path_multi([1, 2])


def test_new_symbols_are_exported_and_declared():
    assert all(n in capi.SYMBOLS for n in NEW)
    lib = os.path.join(ROOT, "bess_amd", "libbessx.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(bessx_\w+)\b", out))
    header = open(os.path.join(ROOT, "include", "bessx.h")).read()
    for n in NEW:
        assert n in exported, n
        assert re.search(r"\bint %s\(" % n, header), n
