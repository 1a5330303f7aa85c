"""The argument checks that the device-matrix entry points of the C ABI share (include/bessx.h sections 2c to 2o), as one
table: every entry point is fed the same bad inputs through its ctypes struct, and the return code and the whole text
of bessx_last_error are compared.  The checks are made before any device call, so nothing here needs a GPU: x is a
made-up pointer that is never read."""
import ctypes

import numpy as np
import pytest

from bess_amd import capi

N, P, M = 8, 4, 2
ARG, UNSUPPORTED = 1, 3
M_MAX = 1024  # INFO_M_MAX

_out = lambda: (ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0))


def _model(a, keep, n, p, cols, beta, name="beta"):
    keep["cols"], keep[name] = np.asarray(cols, dtype=np.int32), np.asarray(beta, dtype=np.float64)
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 0x1000, 0, p, 1, n, p
    a.cols, a.m = capi._ip(keep["cols"]), len(cols)
    setattr(a, name, capi._dp(keep[name]))


def _glm(cls, n, p, cols, beta):
    """A valid call of one of the structs that share bessx_info_input's model and data fields."""
    a, keep = cls(), {}
    _model(a, keep, n, p, cols, beta)
    keep["y"] = np.zeros(n)
    a.coef0, a.link, a.y_host, a.y_stride = 0.1, 0, capi._dp(keep["y"]), 1
    return a, keep


def _cox(cls, n, p, cols, beta, name="beta"):
    a, keep = cls(), {}
    _model(a, keep, n, p, cols, beta, name)
    keep["time"], keep["status"] = np.arange(n, dtype=np.float64), np.ones(n)
    a.time, a.status = capi._dp(keep["time"]), capi._dp(keep["status"])
    return a, keep


def _buf(keep, name, count):
    keep[name] = np.zeros(max(int(count), 1))
    return keep[name].ctypes.data


def _info_out(a, keep, M1):
    a.info, a.info_ld, a.score = _buf(keep, "info", M1 * M1), M1, _buf(keep, "score", M1)


def _groups(a, keep, p):
    keep["gs"] = np.arange(0, p, 2, dtype=np.int32)
    a.group_starts, a.n_groups = capi._ip(keep["gs"]), len(keep["gs"])
    keep["offs"] = np.zeros(len(keep["gs"]) + 1, dtype=np.int64)
    a.offsets = keep["offs"].ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    a.u, a.D = _buf(keep, "u", p), _buf(keep, "D", 4 * p)


def _eval(n, p, cols, beta):
    a, keep = capi.EvalInput(), {}
    _model(a, keep, n, p, cols, beta, "B")
    keep["c0"], keep["y"] = np.array([0.1]), np.zeros(n)
    a.coef0, a.R, a.link = capi._dp(keep["c0"]), 1, 0
    a.y_host, a.y_row_stride, a.y_col_stride, a.y_cols = capi._dp(keep["y"]), 1, 1, 1
    loss, aux, sw = _out()
    return a, keep, lambda: capi.lib().bessx_eval_device(ctypes.byref(a), loss, aux, sw)


def _info(n, p, cols, beta):
    a, keep = _glm(capi.InfoInput, n, p, cols, beta)
    _info_out(a, keep, len(cols) + 1)
    loss, sw, _ = _out()
    return a, keep, lambda: capi.lib().bessx_info_device(ctypes.byref(a), loss, sw)


def _diag(n, p, cols, beta):
    a, keep = _glm(capi.DiagInput, n, p, cols, beta)
    a.kinds, a.out, a.out_ld, a.dispersion = 2, _buf(keep, "out", n), n, 1.0  # (a kind that needs no factor)
    return a, keep, lambda: capi.lib().bessx_diag_device(ctypes.byref(a))


def _sandwich(n, p, cols, beta):
    a, keep = _glm(capi.SandwichInput, n, p, cols, beta)
    M1 = len(cols) + 1
    _info_out(a, keep, M1)
    a.kind, a.meat, a.meat_ld = 0, _buf(keep, "meat", M1 * M1), M1
    loss, sw, _ = _out()
    nc = ctypes.c_int(0)
    return a, keep, lambda: capi.lib().bessx_sandwich_device(ctypes.byref(a), loss, sw, ctypes.byref(nc))


def _addscore(n, p, cols, beta):
    a, keep = _glm(capi.AddscoreInput, n, p, cols, beta)
    M1 = len(cols) + 1
    keep["info"], keep["score"] = np.zeros(M1 * M1), np.zeros(M1)
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), M1, capi._dp(keep["score"])
    a.q, a.u, a.d = p, _buf(keep, "u", p), _buf(keep, "d", p)
    loss, sw, _ = _out()
    return a, keep, lambda: capi.lib().bessx_addscore_device(ctypes.byref(a), loss, sw)


def _groupscore(n, p, cols, beta):
    a, keep = _glm(capi.GroupscoreInput, n, p, cols, beta)
    M1 = len(cols) + 1
    keep["info"], keep["score"] = np.zeros(M1 * M1), np.zeros(M1)
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), M1, capi._dp(keep["score"])
    _groups(a, keep, p)
    loss, sw, _ = _out()
    return a, keep, lambda: capi.lib().bessx_groupscore_device(ctypes.byref(a), loss, sw)


def _meat(n, p, cols, beta):
    a, keep = capi.MeatInput(), {}
    keep["cols"] = np.asarray(cols, dtype=np.int32)
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 0x1000, 0, p, 1, n, p
    a.cols, a.m, a.intercept = capi._ip(keep["cols"]), len(cols), 1
    M1 = len(cols) + 1
    a.meat, a.meat_ld, a.sums = _buf(keep, "meat", M1 * M1), M1, _buf(keep, "sums", M1)
    nc = ctypes.c_int(0)
    return a, keep, lambda: capi.lib().bessx_meat_device(ctypes.byref(a), ctypes.byref(nc))


def _cox_eval(n, p, cols, beta):
    a, keep = _cox(capi.CoxEvalInput, n, p, cols, beta, "B")
    a.R = 1
    ll = ctypes.c_double(0)
    pairs, comp = (ctypes.c_longlong * 3)(), ctypes.c_longlong(0)
    return a, keep, lambda: capi.lib().bessx_eval_cox_device(ctypes.byref(a), ll, pairs, ctypes.byref(comp))


def _cox_baseline(n, p, cols, beta):
    a, keep = _cox(capi.CoxBaselineInput, n, p, cols, beta, "B")
    nt = ctypes.c_int(0)
    keep["t"], keep["h"] = np.zeros(n), np.zeros(n)
    return a, keep, lambda: capi.lib().bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(nt), capi._dp(keep["t"]),
                                                                 capi._dp(keep["h"]))


def _cox_survival(n, p, cols, beta):
    a, keep = capi.CoxSurvivalInput(), {}
    _model(a, keep, n, p, cols, beta, "B")
    keep["hg"], keep["out"] = np.array([0.5]), np.zeros(n)
    a.hg, a.T, a.kind, a.out_row_stride, a.out_col_stride = capi._dp(keep["hg"]), 1, 0, 1, 1
    return a, keep, lambda: capi.lib().bessx_cox_survival_device(ctypes.byref(a), keep["out"].ctypes.data)


def _cox_info(n, p, cols, beta):
    a, keep = _cox(capi.CoxInfoInput, n, p, cols, beta)
    _info_out(a, keep, len(cols))
    ll, ne, rs = _out()
    return a, keep, lambda: capi.lib().bessx_cox_info_device(ctypes.byref(a), ll, ne, rs)


def _cox_diag(n, p, cols, beta):
    a, keep = _cox(capi.CoxDiagInput, n, p, cols, beta)
    a.kinds, a.out_rows, a.out_rows_ld = 1, _buf(keep, "rows", n), n
    ne = ctypes.c_int(0)
    return a, keep, lambda: capi.lib().bessx_cox_diag_device(ctypes.byref(a), ctypes.byref(ne))


def _cox_addscore(n, p, cols, beta):
    a, keep = _cox(capi.CoxAddscoreInput, n, p, cols, beta)
    m = len(cols)
    keep["info"], keep["score"] = np.zeros(max(m * m, 1)), np.zeros(max(m, 1))
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), m, capi._dp(keep["score"])
    a.q, a.u, a.d, a.t = p, _buf(keep, "u", p), _buf(keep, "d", p), _buf(keep, "t", p)
    ll, ne, rs = _out()
    return a, keep, lambda: capi.lib().bessx_cox_addscore_device(ctypes.byref(a), ll, ne, rs)


def _cox_groupscore(n, p, cols, beta):
    a, keep = _cox(capi.CoxGroupscoreInput, n, p, cols, beta)
    m = len(cols)
    keep["info"], keep["score"] = np.zeros(max(m * m, 1)), np.zeros(max(m, 1))
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), m, capi._dp(keep["score"])
    _groups(a, keep, p)
    a.T = _buf(keep, "T", 4 * p)
    ll, ne, rs = _out()
    return a, keep, lambda: capi.lib().bessx_cox_groupscore_device(ctypes.byref(a), ll, ne, rs)


def _set(**kw):
    def change(a, keep):
        for k, v in kw.items():
            setattr(a, k, v)
    return change


def _nan_time(a, keep):
    keep["time"][3] = np.nan


def _half_status(a, keep):
    keep["status"][3] = 0.5


# name of the case -> (the one change to a valid call, return code, text behind "<who>: ")
X_AND_MODEL = {
    "x dtype 7": (_set(x_dtype=7), ARG, "x: dtype must be BESSX_F64 or BESSX_F32"),
    "negative x row stride": (_set(x_row_stride=-1), ARG, "strides must be non-negative"),
    "negative x column stride": (_set(x_col_stride=-1), ARG, "strides must be non-negative"),
}
Y_AND_WEIGHT = {
    "y as host and device": (_set(y_dev=0x2000), ARG,
                             "give y as a host pointer or as a device view (one of the two)"),
    "y as neither": (_set(y_host=None), ARG, "give y as a host pointer or as a device view (one of the two)"),
    "weight as both": (lambda a, keep: (keep.__setitem__("w", np.ones(N)), setattr(a, "weight_host", capi._dp(keep["w"])),
                                        setattr(a, "weight_dev", 0x2000)), ARG,
                       "give weight as a host pointer or as a device vector, not both"),
}
COX_DATA = {
    "ties 2": (_set(ties=2), ARG, "ties must be 0 (order) or 1 (breslow)"),
    "NaN time": (_nan_time, ARG, "time holds a NaN"),
    "status 0.5": (_half_status, ARG, "status must be 0 or 1"),
}
# bad supports and coefficients are separate calls: (cols, beta) -> code, text
COLS = [((1, 4), (0.5, -0.5), ARG, "column number out of range"),
        ((2, 1), (0.5, -0.5), ARG, "cols must be ascending and distinct"),
        ((1, 1), (0.5, -0.5), ARG, "cols must be ascending and distinct")]
FINITE = [((1, 2), (0.5, np.nan), ARG, "beta must be finite"), ((1, 2), (np.inf, 0.5), ARG, "beta must be finite")]

# who -> (maker, name of the coefficient field, the groups of shared cases that apply)
ENTRY = {
    "eval_device": (_eval, "B", ("glm",)),
    "info_device": (_info, "beta", ("glm", "finite", "coef0", "m_max")),
    "diag_device": (_diag, "beta", ("glm", "finite", "coef0", "m_max")),
    "sandwich_device": (_sandwich, "beta", ("glm", "finite", "coef0", "m_max")),
    "addscore_device": (_addscore, "beta", ("glm", "finite", "coef0", "m_max")),
    "groupscore_device": (_groupscore, "beta", ("glm", "finite", "coef0", "m_max")),
    "meat_device": (_meat, None, ()),
    "eval_cox_device": (_cox_eval, "B", ("cox",)),
    "cox_baseline_device": (_cox_baseline, "B", ("cox_rows",)),
    "cox_survival_device": (_cox_survival, "B", ()),
    "cox_info_device": (_cox_info, "beta", ("cox", "finite", "m_max")),
    "cox_diag_device": (_cox_diag, "beta", ("cox", "finite", "m_max")),
    "cox_addscore_device": (_cox_addscore, "beta", ("cox", "finite", "m_max")),
    "cox_groupscore_device": (_cox_groupscore, "beta", ("cox", "finite", "m_max")),
}


def _expect(who, call, code, text):
    rc = call()
    assert (rc, capi.last_error()) == (code, "%s: %s" % (who, text))


@pytest.mark.parametrize("who", sorted(ENTRY))
def test_shared_bad_inputs_give_the_same_code_and_text_under_every_entry_point(who):
    make, coef, groups = ENTRY[who]
    cases = dict(X_AND_MODEL)
    if "glm" in groups:
        cases.update(Y_AND_WEIGHT)
    if "cox" in groups:
        cases.update(COX_DATA)
    if "cox_rows" in groups:  # (the baseline has no ties argument: it is Breslow's)
        cases.update({k: v for k, v in COX_DATA.items() if k != "ties 2"})
    if "coef0" in groups:
        cases["infinite coef0"] = (_set(coef0=float("inf")), ARG, "coef0 must be finite")
        cases["NaN coef0"] = (_set(coef0=float("nan")), ARG, "coef0 must be finite")
    if coef:
        cases["null %s with m > 0" % coef] = (_set(**{coef: None}), ARG, "null argument (%s)" % coef)
    for name, (change, code, text) in cases.items():
        a, keep, call = make(N, P, (1, 2), (0.5, -0.5))
        change(a, keep)
        print(who, "|", name)
        _expect(who, call, code, text)
    for cols, beta, code, text in COLS + (FINITE if "finite" in groups else []):
        a, keep, call = make(N, P, cols, beta)
        _expect(who, call, code, text)
    if "m_max" in groups:  # m + 1 = 1025: said before the device is touched
        a, keep, call = make(N, 2000, tuple(range(M_MAX)), (0.0,) * M_MAX)
        _expect(who, call, UNSUPPORTED, "m + 1 must be at most %d" % M_MAX)


def test_predict_device_makes_the_model_checks_under_its_own_name():
    cols, B, c0, out = np.array([1, 2], dtype=np.int32), np.array([0.5, -0.5]), np.array([0.1]), np.zeros(N)

    def call(dtype=0, rs=P, cs=1, cols=cols, B=B):
        return lambda: capi.lib().bessx_predict_device(0x1000, dtype, rs, cs, N, P, capi._ip(cols), M, capi._dp(B),
                                                       capi._dp(c0), 1, 0, out.ctypes.data, 1, 1, None, 0, None)
    _expect("predict_device", call(dtype=7), ARG, "x: dtype must be BESSX_F64 or BESSX_F32")
    _expect("predict_device", call(rs=-1), ARG, "strides must be non-negative")
    _expect("predict_device", call(cs=-1), ARG, "strides must be non-negative")
    _expect("predict_device", call(cols=np.array([1, 4], dtype=np.int32)), ARG, "column number out of range")
    _expect("predict_device", call(cols=np.array([2, 1], dtype=np.int32)), ARG, "cols must be ascending and distinct")
    _expect("predict_device", call(B=None), ARG, "null argument (B)")


def test_a_valid_call_passes_every_check_that_needs_no_device():
    """The valid calls of the table really are valid: each gets as far as the first device call, which on a machine
    without a GPU is the library's own 'no device' error and on one with a GPU the rejection of the made-up pointer."""
    for who, (make, coef, groups) in sorted(ENTRY.items()):
        a, keep, call = make(N, P, (1, 2), (0.5, -0.5))
        rc, msg = call(), capi.last_error()
        assert (rc, msg) in ((2, "no HIP device visible: libbessx has no CPU path"),
                             (1, who + ": x: not a device pointer (hipPointerGetAttributes does not know it)"),
                             (1, who + ": x: not device memory (host or managed memory)")), (who, rc, msg)
