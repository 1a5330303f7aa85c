"""Score tests of excluded GROUPS of columns without a GPU: bess_base.score_tests_groups on a NumPy X
(bess_base._score_tests_groups_host, fp64 NumPy) and capi.group_score_test_table against the longdouble reference and the
derived bounds of tests/groupscoreref.py at depth n; the residual-sum-of-squares identity; singletons against
score_tests; capi.chi2_sf; group_score_test_table on hand-made inputs; bessx_groupscore_workspace, which needs no device;
and the argument checks, which are made before any device call."""
import ctypes
import math

import numpy as np
import pytest

import groupscoreref
from bess_amd import capi, linear

LD = np.longdouble
LINKS = ["identity", "logistic", "poisson"]
N, P = 300, 40
WIDTHS = np.array([1, 2, 3, 5, 4, 1, 6, 8, 3, 7])
STARTS = np.concatenate([[0], np.cumsum(WIDTHS)[:-1]])  # 0 1 3 6 11 15 16 22 30 33
LABELS = np.repeat(np.arange(WIDTHS.size) * 3 + 2, WIDTHS)  # non-decreasing labels, not 0 .. G - 1
SUPPORT = np.array([1, 2, 11, 12, 13, 14])  # groups 1 and 4
SIGNAL = 6  # the left-out group the responses depend on: columns 16 .. 21


def _est(link, beta, coef0):
    est = {"identity": linear.PdasLm, "logistic": linear.PdasLogistic, "poisson": linear.PdasPoisson}[link]()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, coef0
    return est


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


_CASES = {}


def _case(link, weighted):
    """A model on N rows whose support is groups 1 and 4 and that leaves out the group SIGNAL the responses depend on;
    weights are multiples of 1/8 with zeros.  Computed once and shared."""
    key = (link, weighted)
    if key not in _CASES:
        rng = np.random.default_rng(57 + 3 * LINKS.index(link) + weighted)
        X = rng.standard_normal((N, P))
        beta = np.zeros(P)
        beta[SUPPORT] = rng.standard_normal(SUPPORT.size) * 0.5
        coef0 = 0.3
        sig = np.arange(STARTS[SIGNAL], STARTS[SIGNAL] + WIDTHS[SIGNAL])
        eta = X @ beta + coef0 + X[:, sig] @ (np.array([0.5, -0.4, 0.3, 0.4, -0.3, 0.5]))
        y = {"identity": eta + rng.standard_normal(N),
             "logistic": (rng.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(float),
             "poisson": rng.poisson(np.exp(np.clip(eta, -5, 3))).astype(float)}[link]
        w = rng.integers(0, 17, N) / 8.0 if weighted else None
        _CASES[key] = dict(X=X, cols=SUPPORT, beta=beta, coef0=coef0, y=y, w=w)
    return _CASES[key]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("link", LINKS)
def test_numpy_route_is_within_the_bounds_of_the_reference(link, weighted):
    cs = _case(link, weighted)
    what = "%s weighted=%s" % (link, weighted)
    w = np.ones(N) if cs["w"] is None else cs["w"]
    got = linear.bess_base._score_tests_groups_host(link, cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"],
                                                    w, STARTS, None)
    assert got["positive_definite"]
    R, pd = capi.info_factor(got["info"])
    ref = groupscoreref.groupscore_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], cs["w"],
                                             link, R, STARTS, None, groupscoreref.host_depths(N))
    groupscoreref.check_blocks(got, ref, what)
    est = _est(link, cs["beta"], cs["coef0"])
    table = est.score_tests_groups(cs["X"], cs["y"], LABELS, weight=cs["w"])
    st = groupscoreref.statistic_reference(ref)
    groupscoreref.check_table(table, st, what)
    assert np.array_equal(table["cols"], cs["cols"]) and np.array_equal(table["group"], np.arange(WIDTHS.size))
    assert np.array_equal(table["df"], WIDTHS) and np.array_equal(table["first_column"], STARTS)
    assert np.array_equal(np.nonzero(table["in_model"])[0], [1, 4])
    assert int(np.nanargmin(table["p_value"])) == SIGNAL
    # a subset of the groups gives the same numbers for its groups
    sub_groups = np.array([0, 1, SIGNAL, 9])
    sub = est.score_tests_groups(cs["X"], cs["y"], LABELS, weight=cs["w"], groups=sub_groups)
    assert np.array_equal(sub["group"], sub_groups) and np.array_equal(sub["in_model"], [False, True, False, False])
    both = ~sub["in_model"]
    assert np.allclose(sub["statistic"][both], table["statistic"][sub_groups][both], rtol=1e-10)
    assert np.allclose(sub["p_value"][both], table["p_value"][sub_groups][both], rtol=1e-8, atol=0)


def test_identity_statistic_is_the_drop_of_the_residual_sum_of_squares():
    cs = _case("identity", False)
    table = _est("identity", cs["beta"], cs["coef0"]).score_tests_groups(cs["X"], cs["y"], LABELS)
    Z = np.column_stack([np.ones(N), cs["X"][:, cs["cols"]]])
    rss = lambda A: float(((cs["y"] - A @ np.linalg.lstsq(A, cs["y"], rcond=None)[0]) ** 2).sum())  # noqa: E731
    for g in (2, SIGNAL, 7):  # widths 3, 6 and 8
        J = np.arange(STARTS[g], STARTS[g] + WIDTHS[g])
        drop = rss(Z) - rss(np.column_stack([Z, cs["X"][:, J]]))
        assert abs(table["statistic"][g] * table["dispersion"] - drop) <= 1e-9 * max(drop, 1.0)


@pytest.mark.parametrize("link", LINKS)
def test_a_partition_into_singletons_gives_the_statistics_of_score_tests(link):
    cs = _case(link, True)
    est = _est(link, cs["beta"], cs["coef0"])
    one = est.score_tests(cs["X"], cs["y"], weight=cs["w"])
    grp = est.score_tests_groups(cs["X"], cs["y"], np.arange(P), weight=cs["w"])
    assert np.array_equal(grp["in_model"], one["in_model"]) and np.array_equal(grp["df"], np.ones(P))
    out = ~one["in_model"]
    assert np.allclose(grp["statistic"][out], one["statistic"][out], rtol=1e-10, atol=0)
    assert np.allclose(grp["p_value"][out], one["p_value"][out], rtol=1e-8, atol=0)
    assert np.isnan(grp["statistic"][~out]).all()


def test_chi2_sf_closed_forms():
    xs = np.concatenate([np.logspace(-3, np.log10(500.0), 60), [0.5, 1.0, 2.0, 3.0, 4.0, 50.0]])
    for x in xs:
        e1, e2 = math.erfc(math.sqrt(x / 2)), math.exp(-x / 2)
        assert abs(capi.chi2_sf(x, 1) - e1) <= 1e-15 * e1, x
        assert abs(capi.chi2_sf(x, 2) - e2) <= 1e-15 * e2, x
    assert capi.chi2_sf(0.0, 5) == 1.0 and capi.chi2_sf(float("inf"), 5) == 0.0
    assert math.isnan(capi.chi2_sf(float("nan"), 3)) and math.isnan(capi.chi2_sf(-1.0, 3))
    with pytest.raises(ValueError):
        capi.chi2_sf(1.0, 0)
    # P(chi2_4 > x) = exp(-x / 2) (1 + x / 2); the series and the continued fraction agree with the recurrence
    assert abs(capi.chi2_sf(3.0, 4) - math.exp(-1.5) * 2.5) <= 1e-15
    for df in (1, 2, 3, 7, 16, 33, 64):
        for x in (0.01, 0.7, df * 0.5, df + 1.5, df * 2.0 + 2, df * 4.0 + 30):
            exact, general = capi.chi2_sf(x, df), capi.chi2_sf(x, df + 1e-12)  # (a non-integer df takes the general route)
            assert abs(general - exact) <= 1e-9 * exact + 1e-300, (df, x, exact, general)
    # monotone in x and in df
    assert capi.chi2_sf(5.0, 3) > capi.chi2_sf(6.0, 3) and capi.chi2_sf(5.0, 4) > capi.chi2_sf(5.0, 3)
    assert capi.chi2_sf(2000.0, 3) == pytest.approx(0.0, abs=1e-300) and 0 < capi.chi2_sf(10.0, 1000) <= 1.0


def test_chi2_sf_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    xs = np.logspace(-3, np.log10(500.0), 80)
    for df in range(1, 65):
        want = stats.chi2.sf(xs, df)
        got = np.array([capi.chi2_sf(x, df) for x in xs])
        assert np.allclose(got, want, rtol=1e-12, atol=1e-300), df
        got = np.array([capi.chi2_sf(x, df + 0.5) for x in xs])  # the series and the continued fraction
        assert np.allclose(got, stats.chi2.sf(xs, df + 0.5), rtol=1e-11, atol=1e-300), df


def test_group_score_test_table_on_hand_made_inputs():
    # groups of columns (0, 1), (4,), (6, 7), (9, 10): regular, regular, singular, in the model
    D = [np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([[5.0]]), np.array([[2.0, 2.0], [2.0, 2.0]]), np.eye(2)]
    S = [np.array([[2.0, 0.0], [0.0, 1.0]]), np.array([[1.0]]), np.zeros((2, 2)), np.zeros((2, 2))]
    got = {"columns": np.array([0, 1, 4, 6, 7, 9, 10]), "group_of_column": np.array([0, 0, 2, 3, 3, 5, 5]),
           "u": np.array([3.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0]), "a": np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
           "D": np.concatenate([b.reshape(-1) for b in D]), "S": np.concatenate([b.reshape(-1) for b in S]),
           "offsets": np.array([0, 4, 5, 9, 13]), "score": np.zeros(3), "loss": 14.0, "sum_w": 10.0,
           "support": np.array([10, 12])}
    t = capi.group_score_test_table(got, "logistic")
    assert t["dispersion"] == 1.0
    assert np.array_equal(t["group"], [0, 2, 3, 5]) and np.array_equal(t["first_column"], [0, 4, 6, 9])
    assert np.array_equal(t["df"], [2, 1, 2, 2]) and np.array_equal(t["in_model"], [False, False, False, True])
    assert np.array_equal(t["score"][0], [2.0, 1.0]) and np.array_equal(t["score"][1], [2.0])
    # V = [[2, 1], [1, 2]], adj = (2, 1): adj^T V^-1 adj = (2 * 4 - 2 * 2 + 2 * 1) / 3 = 2
    assert abs(t["statistic"][0] - 2.0) < 1e-14 and abs(t["p_value"][0] - math.exp(-1.0)) < 1e-14
    assert abs(t["statistic"][1] - 1.0) < 1e-15 and abs(t["p_value"][1] - 0.31731050786291415) < 1e-15
    assert np.isnan(t["statistic"][2:]).all() and np.isnan(t["p_value"][2:]).all()  # singular; in the model
    t = capi.group_score_test_table(got, "identity")
    assert t["dispersion"] == 2.0 and abs(t["statistic"][0] - 1.0) < 1e-14
    for bad in (np.nan, np.inf, -1.0):  # a diagonal entry of V that is not finite and positive
        g2 = dict(got, D=got["D"].copy())
        g2["D"][0] = bad
        assert np.isnan(capi.group_score_test_table(g2, "logistic")["statistic"][0])
    got["sum_w"] = 3.0  # no residual degrees of freedom
    assert np.isnan(capi.group_score_test_table(got, "identity")["statistic"]).all()
    with pytest.raises(ValueError):
        capi.group_score_test_table(got, "cox")


def test_workspace_needs_no_device_and_its_block_bound_does_not_depend_on_p():
    n, m = 50000, 200
    small = capi.groupscore_workspace(n, 10000, m, np.arange(0, 10000, 5))
    big = capi.groupscore_workspace(n, 1000000, m, np.arange(0, 1000000, 5))
    Mp = 16 * ((m + 2 + 15) // 16)
    for ws in (small, big):
        assert ws["band"] == 1 and ws["s_depth"] == Mp
        assert ws["gram_rows_per_slab"] % 32 == 0 and ws["gram_slabs"] == -(-n // ws["gram_rows_per_slab"]) <= 32
        assert ws["gram_depth"] == ws["gram_rows_per_slab"] + ws["gram_slabs"]
        assert ws["depth"] == ws["rows_per_slab"] + (ws["slabs"] + 15) // 16 + 4
        assert ws["block_first"][0] == 0 and ws["block_first"][1] == 2045 // 5
    assert small["block_doubles"] == big["block_doubles"] and small["doubles"] == big["doubles"]
    assert small["blocks"] == -(-10000 // 2045) and big["blocks"] == -(-1000000 // 2045)
    panel = (n + 31) // 32 * 32 * Mp
    assert small["doubles"] == 2 * n + panel + small["block_doubles"]
    assert small["block_doubles"] * 8 < 256 << 20
    # the cut is a function of (starts, groups, candidate_block): whole groups, at most candidate_block columns
    starts = np.concatenate([[0], np.cumsum([15, 16, 17, 31, 33, 64, 1, 2])[:-1]])
    ws = capi.groupscore_workspace(37, 179, 3, starts, candidate_block=64)
    assert ws["band"] == 4 and ws["block_first"] == [0, 3, 5, 6, 8] and ws["blocks"] == 4  # 48, 31 + 33, 64, 1 + 2
    assert capi.groupscore_workspace(37, 179, 3, starts, groups=[0, 1, 6, 7], candidate_block=32)["block_first"] == [0, 3, 4]
    assert capi.groupscore_workspace(37, 179, 3, starts, groups=[0, 1, 6, 7])["band"] == 1
    assert capi.groupscore_workspace(37, 179, 3, starts, groups=[6])["band"] == 0
    bad = [dict(n=0, p=5, m=1, group_starts=[0]), dict(n=5, p=5, m=-1, group_starts=[0]),
           dict(n=5, p=5, m=1, group_starts=[1, 2]), dict(n=5, p=5, m=1, group_starts=[0, 2, 2]),
           dict(n=5, p=5, m=1, group_starts=[0, 3, 2]), dict(n=5, p=5, m=1, group_starts=[0, 5]),
           dict(n=5, p=5, m=1, group_starts=[0, 2], groups=[1, 0]), dict(n=5, p=5, m=1, group_starts=[0, 2], groups=[1, 1]),
           dict(n=5, p=5, m=1, group_starts=[0, 2], groups=[2]), dict(n=5, p=5, m=1, group_starts=[0, 2], groups=[-1]),
           dict(n=5, p=5, m=1, group_starts=[0, 2], candidate_block=24),
           dict(n=5, p=40, m=1, group_starts=[0, 17], candidate_block=16)]  # (widths 17 and 23 need a block of 32)
    for kw in bad:
        with pytest.raises(capi.BessxError) as e:
            capi.groupscore_workspace(**kw)
        assert e.value.code == 1, kw
    assert capi.groupscore_workspace(5, 40, 1, [0, 17], groups=[0], candidate_block=32)["blocks"] == 1
    # the width limit: 64 columns are served, 65 are not, and the message names the group
    assert capi.groupscore_workspace(100, 131, 1, [0, 3, 67])["band"] == 4  # widths 3, 64, 64
    with pytest.raises(capi.BessxError) as e:
        capi.groupscore_workspace(100, 132, 1, [0, 3, 67])  # widths 3, 64, 65
    assert e.value.code == 3 and "group 2 has 65 columns" in str(e.value)
    assert capi.groupscore_workspace(100, 132, 1, [0, 3, 67], groups=[0, 1])["band"] == 4  # (the wide one is not tested)
    with pytest.raises(capi.BessxError) as e:
        capi.groupscore_workspace(100, 50, 1024, [0])
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    for kw in (dict(group_starts=[]), dict(group_starts=[[0]]), dict(group_starts=[0.0, 1.0]),
               dict(group_starts=[0], groups=[]), dict(group_starts=[0], groups=[0.5])):
        with pytest.raises(ValueError):
            capi.groupscore_workspace(5, 5, 1, **kw)


def _raw_input(n=8, p=6, m=2, starts=(0, 2, 3), groups=None):
    """A bessx_groupscore_input whose pointers are host memory: good enough for the checks that come before any device
    call (the last of them is the question whether x is device memory)."""
    keep = dict(x=np.zeros((n, p)), cols=np.arange(m, dtype=np.int32), beta=np.zeros(max(m, 1)), y=np.zeros(n),
                info=np.zeros((m + 1, m + 1)), score=np.zeros(m + 1), vec=np.zeros((2, p)), blk=np.zeros((2, p * p)),
                factor=np.eye(m + 1), starts=np.asarray(starts, dtype=np.int32), offsets=np.zeros(p + 1, dtype=np.int64),
                groups=None if groups is None else np.asarray(groups, dtype=np.int32))
    a = capi.GroupscoreInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = keep["x"].ctypes.data, 0, p, 1, n, p
    a.cols, a.m, a.beta, a.coef0, a.link = capi._ip(keep["cols"]), m, capi._dp(keep["beta"]), 0.0, 0
    a.y_host, a.y_stride = capi._dp(keep["y"]), 1
    a.factor, a.factor_ld = capi._dp(keep["factor"]), m + 1
    a.group_starts, a.n_groups = capi._ip(keep["starts"]), keep["starts"].size
    if groups is not None:
        a.groups, a.n_tested = capi._ip(keep["groups"]), keep["groups"].size
    a.info, a.info_ld, a.score = capi._dp(keep["info"]), m + 1, capi._dp(keep["score"])
    a.u, a.a = (keep["vec"][k].ctypes.data for k in range(2))
    a.D, a.S = (keep["blk"][k].ctypes.data for k in range(2))
    a.offsets = keep["offsets"].ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    return a, keep


def _raw_call(a):
    loss, sw = ctypes.c_double(0), ctypes.c_double(0)
    return capi.lib().bessx_groupscore_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw))


def test_argument_errors_of_the_library_come_before_any_device_call():
    L = capi.lib()
    cases, keeps = [], []

    def add(msg, code=1, edit=None, **kw):
        a, k = _raw_input(**kw)
        if edit:
            edit(a, k)
        cases.append((a, msg, code))
        keeps.append(k)

    add(b"must begin with column 0", starts=(1, 2))
    add(b"group_starts must be ascending and distinct", starts=(0, 3, 3))
    add(b"group_starts must be ascending and distinct", starts=(0, 3, 2))
    add(b"not a column of x", starts=(0, 6))
    add(b"groups must be ascending and distinct", groups=(1, 0))
    add(b"groups must be ascending and distinct", groups=(1, 1))
    add(b"not a group of the partition", groups=(0, 3))
    add(b"not a group of the partition", groups=(-1, 1))
    add(b"n_tested must be at least 1", groups=(0,), edit=lambda a, k: setattr(a, "n_tested", 0))
    add(b"at least one group", edit=lambda a, k: setattr(a, "n_groups", 0))
    add(b"multiple of 16", edit=lambda a, k: setattr(a, "candidate_block", 40))
    add(b"null argument (S, a)", edit=lambda a, k: setattr(a, "S", None))
    add(b"null argument (u, D, offsets)", edit=lambda a, k: setattr(a, "D", None))
    add(b"lower triangle of the factor must be finite", edit=lambda a, k: k["factor"].__setitem__((1, 0), np.nan))
    add(b"factor_ld must be at least m + 1", edit=lambda a, k: setattr(a, "factor_ld", 2))
    add(b"group 1 has 65 columns", code=3, p=70, starts=(0, 2, 67))
    add(b"candidate_block must be at least the widest tested group rounded up to 16 (32)", p=40, starts=(0, 17),
        edit=lambda a, k: setattr(a, "candidate_block", 16))
    for a, msg, code in cases:
        assert _raw_call(a) == code and msg in L.bessx_last_error(), msg
    assert L.bessx_groupscore_device(None, None, None) == 1
    # every check passed: the next answer is about the device (none here) or about x not being device memory
    a, k = _raw_input()
    rc = _raw_call(a)
    msg = L.bessx_last_error()
    assert rc in (1, 2) and not any(w in msg for w in (b"group_starts", b"tested", b"candidate_block", b"null"))
    if not _has_gpu():
        assert rc == 2
    assert L.bessx_op_groupscore_bench(None, 0, 1, 1, 1, 1, None, 0, None, 0, None, 0, 0, 1, None) == 1


def test_without_a_gpu_valid_arguments_are_refused_with_the_device_error():
    class Fake:  # a device array by its interface only: any device call on it would fail
        def __init__(self, shape, typestr="<f8"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3,
                                             "strides": None}
    x = Fake((10, 6))
    with pytest.raises(capi.BessxError) as e:
        capi.groupscore_device(x, [1, 2], [0.1, 0.2], 0.0, np.zeros(10), [0, 2, 3], factor=np.eye(3))
    assert e.value.code == 2 if not _has_gpu() else e.value.code in (1, 2)
    # what the library refuses it refuses first, with its own code
    with pytest.raises(capi.BessxError) as e:
        capi.groupscore_device(Fake((10, 70)), [1], [0.1], 0.0, np.zeros(10), [0, 2, 67], factor=np.eye(2))
    assert e.value.code == 3 and "group 1 has 65 columns" in str(e.value)
    with pytest.raises(capi.BessxError) as e:
        capi.groupscore_device(x, [1], [0.1], 0.0, np.zeros(10), [0, 3, 2], factor=np.eye(2))
    assert e.value.code == 1
    with pytest.raises(ValueError, match="one model per call"):
        capi.groupscore_device(x, [1, 2], np.zeros((2, 2)), 0.0, np.zeros(10), [0])
    with pytest.raises(ValueError, match="link must be one of"):
        capi.groupscore_device(x, [1], [0.1], 0.0, np.zeros(10), [0], link="cox")
    with pytest.raises(ValueError, match="factor must have shape"):
        capi.groupscore_device(x, [1], [0.1], 0.0, np.zeros(10), [0], factor=np.eye(3))
    est = _est("identity", np.array([1.0, 0.0, 2.0]), 0.0)
    with pytest.raises(ValueError, match=r"X.shape\[1\] should be 3"):
        est.score_tests_groups(x, np.zeros(10), [0, 0, 1])


def test_argument_errors_of_the_estimator():
    cs = _case("identity", False)
    est = _est("identity", cs["beta"], cs["coef0"])
    X, y = cs["X"], cs["y"]
    with pytest.raises(ValueError, match="non-decreasing"):
        est.score_tests_groups(X, y, np.concatenate([[1], np.zeros(P - 1)]))
    with pytest.raises(ValueError, match="one label per column"):
        est.score_tests_groups(X, y, np.zeros(P - 1))
    for groups in ([3, 2], [2, 2], [0, WIDTHS.size], [-1, 2], [], [[1, 2]], [0.5, 2.0]):
        with pytest.raises(ValueError):
            est.score_tests_groups(X, y, LABELS, groups=groups)
    with pytest.raises(ValueError, match="y.size"):
        est.score_tests_groups(X, y[:-1], LABELS)
    with pytest.raises(ValueError, match="weight.size"):
        est.score_tests_groups(X, y, LABELS, weight=np.ones(N + 1))
    with pytest.raises(ValueError, match="X.shape"):
        est.score_tests_groups(X[:, :-1], y, LABELS)
    multi = _est("identity", np.zeros((P, 2)), np.zeros(2))
    multi.beta[3, 0] = multi.beta[4, 1] = 1.0
    with pytest.raises(ValueError, match="one model"):
        multi.score_tests_groups(X, np.column_stack([y, y]), LABELS)
    cox = linear.PdasCox()
    cox.p, cox.beta, cox.coef0 = P, cs["beta"], 0.0
    assert cox.score_tests_groups(X, np.column_stack([np.abs(y) + 1, np.ones(N)]), LABELS) is None


def test_a_singular_block_or_information_gives_nan_and_raises_nothing():
    cs = _case("logistic", False)
    X = cs["X"].copy()
    X[:, 8] = X[:, 6] + X[:, 7]  # group 3 (columns 6 .. 10) reproduces one of its own columns
    X[:, 22] = X[:, 1]           # group 7 holds a copy of a support column
    t = _est("logistic", cs["beta"], cs["coef0"]).score_tests_groups(X, cs["y"], LABELS)
    for g in (3, 7):
        assert np.isnan(t["statistic"][g]) or (np.isfinite(t["statistic"][g]) and t["statistic"][g] >= 0)
    assert np.isfinite(t["statistic"][[0, 2, 5, 6, 8, 9]]).all()
    X[:, 2] = X[:, 1]  # the information itself is singular
    t = _est("logistic", cs["beta"], cs["coef0"]).score_tests_groups(X, cs["y"], LABELS)
    assert np.isnan(t["statistic"]).all() and np.isnan(t["p_value"]).all()
    assert np.array_equal(np.nonzero(t["in_model"])[0], [1, 4])
