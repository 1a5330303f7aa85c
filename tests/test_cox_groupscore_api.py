"""Cox score tests of excluded GROUPS of columns without a GPU: the NumPy route of
bess_base.score_tests_groups_survival against the longdouble reference of tests/coxgroupscoreref.py (event-by-event
risk-set moments) within its bounds, the constants of those bounds, capi.cox_group_score_test_table,
bessx_cox_groupscore_workspace, and the argument errors that the library finds before any device call."""
import ctypes

import numpy as np
import pytest

import coxaddscoreref
import coxgroupscoreref as ref_
from bess_amd import capi, linear

LD = ref_.LD
_CACHE = {}


def _est(cs):
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = cs["X"].shape[1], np.zeros(cs["X"].shape[1]), 0.0
    est.beta[cs["cols"]] = cs["beta"]
    return est


def _labels(cs):
    return np.repeat(np.arange(cs["widths"].size), cs["widths"])


def _host(cs, ties, groups=None):
    n = cs["X"].shape[0]
    w = np.ones(n) if cs["w"] is None else cs["w"]
    return linear.bess_base._cox_score_tests_groups_host(cs["X"].astype(np.float64), cs["cols"].astype(np.int64), cs["beta"],
                                                         cs["time"], cs["status"], w, ties, cs["starts"], groups)


def _all():
    """(name, case, ties, NumPy route, reference) of every CPU case, computed once and left unchanged."""
    if not _CACHE:
        for name, cs, ties in ref_.cases():
            got = _host(cs, ties)
            R = None
            if cs["cols"].size:
                R, pd = capi.info_factor(got["info"])
                assert pd, name
            ref = ref_.cox_groupscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties, R,
                                                cs["starts"], None, ref_.host_depths(cs["X"].shape[0]))
            _CACHE[name] = (cs, ties, got, ref)
    return _CACHE


def _planted(cs, ref):
    """The collinear group always; below n = 1025 also every group whose reference V, scaled to unit diagonal, has
    lambda_min below 1/8 (too few events for its width)."""
    n = cs["X"].shape[0]
    lam = ref_.lambda_min(ref)
    out = {8}
    if n < 1025:
        out |= {int(t) for t in range(lam.size) if not lam[t] >= 0.125}
    return sorted(out)


def test_the_new_symbols_are_exported_declared_and_listed():
    L = capi.lib()
    header = open(capi.os.path.join(capi._HERE, "..", "include", "bessx.h")).read()
    for name in ("bessx_cox_groupscore_device", "bessx_cox_groupscore_workspace", "bessx_op_cox_groupscore_bench"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in header
    assert "bessx_cox_groupscore_input;" in header
    for name in ("CoxGroupscoreInput", "cox_groupscore_workspace", "cox_groupscore_device", "cox_group_score_test_table",
                 "op_cox_groupscore_bench"):
        assert hasattr(capi, name)
    assert hasattr(linear.bess_base, "score_tests_groups_survival")
    assert hasattr(linear.bess_base, "_cox_score_tests_groups_host")


def test_the_reference_is_the_direct_risk_set_definition():
    assert ref_.self_check()


def test_fp64_numpy_fixes_the_constants():
    worst = {"u": 0.0, "a": 0.0, "D": 0.0, "T": 0.0, "S": 0.0, "stat": 0.0}
    for name, (cs, ties, got, ref) in _all().items():
        r = ref_.ratios(got, ref)
        for k, v in r.items():
            worst[k] = max(worst[k], v)
        st = ref_.statistic_reference(ref, planted=_planted(cs, ref))
        table = capi.cox_group_score_test_table(got)
        ok = st["ok"]
        if ok.any():
            err = np.abs(table["statistic"][ok].astype(LD) - st["stat"][ok])
            worst["stat"] = max(worst["stat"], float((err / st["bound"][ok]).max()))
    consts = {"u": ref_.C_U, "a": ref_.C_A, "D": ref_.C_D, "T": ref_.C_T, "S": ref_.C_S, "stat": ref_.C_STAT}
    stored = {"u": ref_.U_NUMPY_MAX, "a": ref_.A_NUMPY_MAX, "D": ref_.D_NUMPY_MAX, "T": ref_.T_NUMPY_MAX,
              "S": ref_.S_NUMPY_MAX, "stat": ref_.STAT_NUMPY_MAX}
    # (the ratios are measured against bounds that already hold the constants: undo them)
    raw = {k: worst[k] * consts[k] for k in worst}
    print("fp64 NumPy needs, as a multiple of the derived bounds:", {k: "%.4g" % v for k, v in raw.items()})
    for k in raw:
        assert raw[k] <= stored[k] * (1 + 1e-3), (k, raw[k], stored[k])  # (stored to four significant digits)
        assert raw[k] >= stored[k] / 2, (k, "the stored maximum is stale", raw[k], stored[k])
        assert consts[k] == ref_.constant_from(stored[k]), k


@pytest.mark.parametrize("name", [c[0] for c in ref_.cases()])
def test_numpy_route_is_within_the_bounds_of_the_reference(name):
    cs, ties, got, ref = _all()[name]
    n = cs["X"].shape[0]
    ref_.check_blocks(got, ref, "numpy " + name)
    planted = _planted(cs, ref)
    if n >= 1025:
        assert planted == [8]  # only the support's group and the collinear group are left out
    st = ref_.statistic_reference(ref, planted=planted)
    table = _est(cs).score_tests_groups_survival(cs["X"].astype(np.float64),
                                                 np.column_stack([cs["time"], cs["status"]]), _labels(cs),
                                                 weight=cs["w"], ties=ties)
    ref_.check_table(table, st, "numpy " + name)
    assert table["dispersion"] == 1.0 and np.array_equal(table["cols"], cs["cols"])
    assert np.array_equal(table["df"], cs["widths"])
    if cs["cols"].size:  # a group touching the support: in_model and NaN
        assert table["in_model"][2] and np.isnan(table["statistic"][2]) and np.isnan(table["p_value"][2])
        assert table["in_model"].sum() == 1
    cl = table["statistic"][8]  # the planted collinear group: NaN, or finite and >= 0; nothing is raised
    assert np.isnan(cl) or (np.isfinite(cl) and cl >= 0)


@pytest.mark.parametrize("case", [c for c in ref_.GPU_CASES if c[0] >= 1025 and c[1] != 31 or c[:2] == (1025, 31)],
                         ids=lambda c: "n%d-m%d-%s%s" % (c[0], c[1], c[2], "-tied" if c[3] else ""))
def test_the_gpu_problems_leave_out_only_the_support_and_the_planted_group(case):
    """What tests/test_cox_groupscore_gpu.py may leave out of the statistic's comparison at n >= 1025: the support's
    group and the planted collinear group.  Every other group has lambda_min >= 1/16 (statistic_reference asserts it)."""
    n, m, ties, tied = case
    cs = ref_.gpu_problem("f64", n, m, tied)
    got = _host(cs, ties)
    R = capi.info_factor(got["info"])[0] if m else None
    ref = ref_.cox_groupscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties, R,
                                        cs["starts"], None, ref_.host_depths(n))
    st = ref_.statistic_reference(ref, planted=[ref_.GPU_COLLINEAR])
    assert int(st["ok"].sum()) == ref_.GPU_WIDTHS.size - 1 - (1 if m else 0)
    lam = st["lam"][st["ok"]]
    print("n=%d m=%d %s: smallest lambda_min %.3f" % (n, m, ties, lam.min()))
    assert lam.min() >= 1.0 / 16
    ref_.check_blocks(got, ref, "numpy, the GPU problem")
    ref_.check_table(capi.cox_group_score_test_table(got), st, "numpy, the GPU problem")


def test_a_collinear_group_gives_nan_and_a_subset_gives_the_same_values():
    cs, ties, got, ref = _all()["n1025-m3-breslow-w"]
    exact = dict(got)
    V = (got["D"] - got["T"]) - got["S"]
    o = got["offsets"]
    blk = V[o[8]:o[9]].reshape(4, 4).copy()
    blk[2, :], blk[:, 2] = blk[0, :] + blk[1, :], blk[:, 0] + blk[:, 1]
    blk[2, 2] = blk[0, 0] + blk[1, 1] + 2 * blk[0, 1] - 1e-3  # exactly singular and a little beyond: no Cholesky factor
    exact["D"], exact["T"], exact["S"] = V.copy(), np.zeros_like(V), np.zeros_like(V)
    exact["D"][o[8]:o[9]] = blk.reshape(-1)
    t = capi.cox_group_score_test_table(exact)
    assert np.isnan(t["statistic"][8]) and np.isnan(t["p_value"][8]) and np.isfinite(t["statistic"][[0, 1, 3]]).all()
    sub = _host(cs, ties, groups=np.array([1, 3, 6]))
    for k in ("u", "a"):
        pos = np.concatenate([[0], np.cumsum(cs["widths"])])
        assert np.allclose(sub[k], np.concatenate([got[k][pos[g]:pos[g + 1]] for g in (1, 3, 6)]), rtol=1e-12, atol=1e-12)


def test_singleton_groups_equal_the_column_table_within_both_bounds():
    cs = ref_.case(203, 3, np.ones(40, dtype=np.int64), True)
    n, p = cs["X"].shape
    y = np.column_stack([cs["time"], cs["status"]])
    est = _est(cs)
    for ties in ("order", "breslow"):
        tg = est.score_tests_groups_survival(cs["X"], y, np.arange(p), weight=cs["w"], ties=ties)
        tc = est.score_tests_survival(cs["X"], y, weight=cs["w"], ties=ties)
        got = _host(cs, ties)
        R, pd = capi.info_factor(got["info"])
        assert pd
        rg = ref_.cox_groupscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties, R,
                                           cs["starts"], None, ref_.host_depths(n))
        rc = coxaddscoreref.cox_addscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties,
                                                   R, None, coxaddscoreref.host_depths(n))
        sg, sc = ref_.statistic_reference(rg), coxaddscoreref.statistic_reference(rc)
        assert np.array_equal(tg["in_model"], tc["in_model"]) and np.array_equal(tg["first_column"], tc["columns"])
        ok = sg["ok"]
        assert np.array_equal(ok, sc["ok"])
        width = (sg["hi"] - sg["lo"]) + (sc["hi"] - sc["lo"])
        assert (np.abs(tg["statistic"][ok] - tc["statistic"][ok]).astype(LD) <= width[ok]).all()
        for k, b in (("u", "bu"), ("a", "ba")):  # the ingredients, entry by entry
            col = linear.bess_base._cox_score_tests_host(cs["X"], cs["cols"].astype(np.int64), cs["beta"], cs["time"],
                                                         cs["status"], np.ones(n) if cs["w"] is None else cs["w"], ties, None)
            assert (np.abs(got[k] - col[k]).astype(LD) <= rg[b] + rc[b]).all(), (ties, k)
        for k, kc, b, bc in (("D", "d", "bD", "bd"), ("T", "t", "bT", "bt"), ("S", "s", "bS", "bs")):
            bg = np.array([x[0, 0] for x in rg[b]])
            assert (np.abs(got[k] - col[kc]).astype(LD) <= bg + rc[bc]).all(), (ties, k)


def test_each_bound_helper_fails_on_a_value_perturbed_at_1e_9():
    cs, ties, got, ref = _all()["n127-m3-order-w"]
    ref_.check_blocks(got, ref, "unperturbed")
    o = got["offsets"]
    for k in ("u", "a", "D", "T", "S"):
        bad = {kk: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for kk, v in got.items()}
        if k in ("u", "a"):
            j = int(np.argmax(np.abs(bad[k])))
            bad[k][j] *= 1 + 1e-9
        else:  # a diagonal entry of the widest group (symmetry is kept)
            bad[k][o[6]] *= 1 + 1e-9
        with pytest.raises(AssertionError):
            ref_.check_blocks(bad, ref, "perturbed " + k)
    st = ref_.statistic_reference(ref, planted=_planted(cs, ref))
    table = capi.cox_group_score_test_table(got)
    ref_.check_table(table, st, "unperturbed")
    t = int(np.nonzero(st["ok"])[0][0])
    bad = dict(table, statistic=table["statistic"].copy())
    bad["statistic"][t] *= 1 + 1e-9
    assert st["stat"][t] >= 1e-3  # (else a relative 1e-9 would say nothing)
    with pytest.raises(AssertionError):
        ref_.check_table(bad, st, "perturbed statistic")


def test_cox_group_score_test_table_on_hand_made_inputs_and_the_shared_loop():
    got = {"columns": np.array([0, 1, 2, 3, 4]), "group_of_column": np.array([0, 0, 1, 2, 2]), "support": np.array([2]),
           "u": np.array([3.0, 1.0, 1.0, 2.0, 0.0]), "a": np.array([1.0, 1.0, 0.0, 0.0, 0.0]),
           "D": np.array([9.0, 0, 0, 4.0, 5.0, 8.0, 0, 0, 2.0]), "T": np.array([3.0, 0, 0, 1.0, 1.0, 2.0, 0, 0, 1.0]),
           "S": np.array([2.0, 0, 0, 2.0, 1.0, 2.0, 0, 0, 1.0]), "offsets": np.array([0, 4, 5, 9]), "score": np.zeros(1)}
    t = capi.cox_group_score_test_table(got)
    assert t["dispersion"] == 1.0 and np.array_equal(t["df"], [2, 1, 2]) and np.array_equal(t["group"], [0, 1, 2])
    assert t["statistic"][0] == 1.0 and np.array_equal(t["in_model"], [False, True, False])  # 2^2 / 4 + 0
    assert np.isnan(t["statistic"][1]) and np.isnan(t["statistic"][2])  # in the model; a zero diagonal entry of V
    assert t["p_value"][0] == capi.chi2_sf(1.0, 2)
    # the GLM table is unchanged by the shared loop: the same V through D - S gives the same statistic
    glm = dict(got, D=got["D"] - got["T"], loss=1.0, sum_w=10.0)
    assert capi.group_score_test_table(glm, "logistic")["statistic"][0] == 1.0


def test_workspace_needs_no_device_and_its_block_bound_does_not_depend_on_p():
    n, m, J = 200000, 150, 100000
    small = capi.cox_groupscore_workspace(n, 10000, m, J, np.arange(0, 10000, 5))
    big = capi.cox_groupscore_workspace(n, 1000000, m, J, np.arange(0, 1000000, 5))
    for ws in (small, big):
        assert ws["t_slabs"] == -(-n // ws["t_rows_per_slab"]) and ws["t_rows_per_slab"] % 32 == 0
        assert ws["t_slabs"] <= 32 and ws["band"] == 1
        rps, sl = ws["t_rows_per_slab"], ws["t_slabs"]
        assert ws["t_depth"] == 2 * (rps // 8 + 11) + rps + rps // 4 + 3 + 8 * sl + 4
    assert small["block_doubles"] == big["block_doubles"] and small["doubles"] == big["doubles"]
    assert small["doubles"] < n * 2048  # nothing is n x q
    # the split of T is a function of n alone
    a = capi.cox_groupscore_workspace(4097, 406, 3, 3000, np.arange(0, 406, 7), candidate_block=64)
    b = capi.cox_groupscore_workspace(4097, 50, 31, 100, [0], candidate_block=0)
    assert (a["t_rows_per_slab"], a["t_slabs"], a["t_depth"]) == (b["t_rows_per_slab"], b["t_slabs"], b["t_depth"])
    assert a["t_slabs"] >= 3
    assert capi.cox_groupscore_workspace(37, 10, 0, 5, [0])["t_slabs"] == 2
    for bad in (dict(n=0, p=5, m=1, n_event_rows=0), dict(n=5, p=5, m=-1, n_event_rows=1),
                dict(n=5, p=5, m=1, n_event_rows=6), dict(n=5, p=5, m=1, n_event_rows=1, candidate_block=24)):
        with pytest.raises(capi.BessxError) as e:
            capi.cox_groupscore_workspace(group_starts=[0], **bad)
        assert e.value.code == 1
    with pytest.raises(capi.BessxError) as e:
        capi.cox_groupscore_workspace(100, 10, 1024, 10, [0])
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    with pytest.raises(capi.BessxError) as e:
        capi.cox_groupscore_workspace(100, 200, 3, 10, [0, 3, 68])
    assert e.value.code == 3 and "group 1 has 65 columns" in str(e.value)


def _raw_input(n=8, p=6, m=2, starts=(0, 2, 3)):
    """A bessx_cox_groupscore_input whose pointers are host memory: good enough for the checks that come before any
    device call (the last of them is the question whether x is device memory)."""
    keep = dict(x=np.zeros((n, p)), cols=np.arange(m, dtype=np.int32), beta=np.zeros(max(m, 1)),
                time=np.arange(n, dtype=np.float64), status=np.ones(n), info=np.zeros((m, m)), score=np.zeros(m),
                vec=np.zeros((2, p)), blk=np.zeros((3, p * p)), factor=np.eye(m), starts=np.array(starts, dtype=np.int32),
                offsets=np.zeros(len(starts) + 1, dtype=np.int64))
    a = capi.CoxGroupscoreInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = keep["x"].ctypes.data, 0, p, 1, n, p
    a.cols, a.m, a.beta = capi._ip(keep["cols"]), m, capi._dp(keep["beta"])
    a.time, a.status, a.ties = capi._dp(keep["time"]), capi._dp(keep["status"]), 0
    a.factor, a.factor_ld = capi._dp(keep["factor"]), m
    a.group_starts, a.n_groups = capi._ip(keep["starts"]), len(starts)
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), m, capi._dp(keep["score"])
    a.u, a.a = keep["vec"][0].ctypes.data, keep["vec"][1].ctypes.data
    a.D, a.T, a.S = (keep["blk"][k].ctypes.data for k in range(3))
    a.offsets = keep["offsets"].ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    return a, keep


def _raw_call(a):
    ll, ne, rs = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    return capi.lib().bessx_cox_groupscore_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs))


def test_argument_errors_of_the_library_come_before_any_device_call():
    L = capi.lib()
    cases, keep = [], []

    def case(msg, code=1, **change):
        a, k = _raw_input()
        keep.append(k)
        for name, v in change.items():
            if isinstance(v, np.ndarray):
                k[name + "_given"] = v
                v = capi._ip(v) if v.dtype == np.int32 else v.ctypes.data
            setattr(a, name, v)
        cases.append((a, k, msg, code))
        return a, k

    case(b"group_starts must begin with column 0", group_starts=np.array([1, 2, 3], dtype=np.int32))
    case(b"group_starts must be ascending and distinct", group_starts=np.array([0, 3, 3], dtype=np.int32))
    case(b"a group start is not a column of x", group_starts=np.array([0, 3, 6], dtype=np.int32))
    case(b"groups must be ascending and distinct", groups=np.array([1, 0], dtype=np.int32), n_tested=2)
    case(b"not a group of the partition", groups=np.array([0, 3], dtype=np.int32), n_tested=2)
    case(b"n_tested must be at least 1", groups=np.array([0], dtype=np.int32), n_tested=0)
    case(b"multiple of 16", candidate_block=40)
    case(b"ties must be 0 (order) or 1 (breslow)", ties=2)
    case(b"null argument (S, a)", S=None)
    case(b"null argument (u, D, T, offsets)", T=None)
    a, k = case(b"status must be 0 or 1")
    k["status"][3] = 2.0
    a, k = case(b"time holds a NaN")
    k["time"][2] = np.nan
    a, k = case(b"lower triangle of the factor must be finite")
    k["factor"][1, 0] = np.nan
    for a, k, msg, code in cases:
        assert _raw_call(a) == code and msg in L.bessx_last_error(), msg
    assert L.bessx_cox_groupscore_device(None, None, None, None) == 1
    # a tested group of more than 64 columns: code 3 before anything is written
    a, k = _raw_input(p=70, starts=(0, 3))
    k["vec"][:], k["blk"][:] = 7.0, 7.0
    assert _raw_call(a) == 3 and b"group 1 has 67 columns" in L.bessx_last_error()
    assert (k["vec"] == 7.0).all() and (k["blk"] == 7.0).all() and (k["offsets"] == 0).all()
    # every check passed: the next answer is about the device (none here) or about x not being device memory
    a, k = _raw_input()
    rc, msg = _raw_call(a), L.bessx_last_error()
    assert rc == 2 or (rc == 1 and b"x: not device memory" in msg), msg


def test_argument_errors_of_the_estimator_and_what_stays_none():
    cs = ref_.case(60, 2, [3, 2, 4, 3], False, support_group=1)
    est = _est(cs)
    X, y, labels = cs["X"], np.column_stack([cs["time"], cs["status"]]), _labels(cs)
    with pytest.raises(ValueError, match="ties"):
        est.score_tests_groups_survival(X, y, labels, ties="efron")
    with pytest.raises(ValueError, match="shape"):
        est.score_tests_groups_survival(X, y[:-1], labels)
    with pytest.raises(ValueError, match="weight.size"):
        est.score_tests_groups_survival(X, y, labels, weight=np.ones(61))
    with pytest.raises(ValueError, match="X.shape"):
        est.score_tests_groups_survival(X[:, :-1], y, labels)
    with pytest.raises(ValueError, match="one label per column"):
        est.score_tests_groups_survival(X, y, labels[:-1])
    with pytest.raises(ValueError, match="non-decreasing"):
        est.score_tests_groups_survival(X, y, labels[::-1])
    for groups in ([1, 0], [0, 0], [0, 4], [-1], []):
        with pytest.raises(ValueError):
            est.score_tests_groups_survival(X, y, labels, groups=groups)
    lm = linear.PdasLm()
    lm.p, lm.beta, lm.coef0 = est.p, est.beta, 0.0
    with pytest.raises(ValueError, match="Cox"):
        lm.score_tests_groups_survival(X, y, labels)
    # unchanged: the Cox classes answer through the _survival methods
    assert est.score_tests_groups(X, y[:, 0], labels) is None and est.score_tests(X, y) is None
    sub = est.score_tests_groups_survival(X, y, labels, groups=[0, 3])
    full = est.score_tests_groups_survival(X, y, labels)
    assert np.array_equal(sub["group"], [0, 3]) and np.allclose(sub["statistic"], full["statistic"][[0, 3]], rtol=1e-9)
