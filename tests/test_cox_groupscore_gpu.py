"""Cox score tests of excluded GROUPS of columns on an X already in GPU memory (bessx_cox_groupscore_device,
bess_amd/csrc/bessx_k_coxgroupscore.hip) against the event-by-event longdouble reference of tests/coxgroupscoreref.py,
within its bounds (the addition depths are those of the split the library reports).  Shapes (coxgroupscoreref.GPU_CASES):
n = 37 (one short slab of positions past a 32-position chunk), n = 1025 (one position past the 1024-position scan block),
n = 4097 (26 position slabs: the carries and the cross terms of the finish); p = 406 columns in
tests/test_groupscore_gpu.py's 27 groups; supports of m = 0 (the null model), 3 and 31 columns, each a whole group; both
ties on a grid of eighths and one all-tied case; weights in eighths with zeros; candidate blocks of 64 and 128; the
layouts of tests/test_addscore_gpu.py, every element outside the view a NaN."""
import numpy as np
import pytest

import coxaddscoreref
import coxgroupscoreref as ref_
import groupscoreref
from bess_amd import linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
WIDTHS, STARTS, P = ref_.GPU_WIDTHS, ref_.GPU_STARTS, ref_.GPU_P
COLLINEAR = ref_.GPU_COLLINEAR
F32_CASES = [c for c in ref_.GPU_CASES if c[:2] in ((37, 3), (4097, 31))]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _embed(layout, vals):
    """(base host array that holds vals in the layout under test, NaN everywhere else; base tensor -> the n x p view)"""
    n, p = vals.shape
    if layout == "C":  # row-major
        return vals.copy(), (lambda t: t)
    if layout == "F":  # column-major with a padded leading dimension, NaN rows >= n
        b = np.full((p, (n + 3) // 4 * 4), np.nan, dtype=vals.dtype)
        b[:, :n] = vals.T
        return b, (lambda t: t[:, :n].T)
    if layout == "T":  # a transposed view that starts on an odd element
        b = np.full((p, n + 3), np.nan, dtype=vals.dtype)
        b[:, 1:1 + n] = vals.T
        return b, (lambda t: t[:, 1:1 + n].T)
    if layout == "two_strides":
        b = np.full((2 * n, 3 * p), np.nan, dtype=vals.dtype)
        b[::2, ::3] = vals
        return b, (lambda t: t[::2, ::3])
    if layout == "odd_offset":  # row-contiguous, first element at an odd offset
        b = np.full((n, p + 5), np.nan, dtype=vals.dtype)
        b[:, 3:3 + p] = vals
        return b, (lambda t: t[:, 3:3 + p])
    raise AssertionError(layout)


_PROBLEMS, _REFS, _TENSORS = {}, {}, {}


def _problem(dt, case):
    key = (dt,) + tuple(case)
    if key not in _PROBLEMS:
        n, m, ties, tied = case
        cs = ref_.gpu_problem(dt, n, m, tied)
        rng = np.random.default_rng(n + m)
        cs["R"] = np.tril(rng.standard_normal((m, m))) / np.sqrt(float(n) * max(m, 1)) if m else None
        cs["J"] = int((cs["status"] != 0).sum())
        _PROBLEMS[key] = cs
    return _PROBLEMS[key]


def _tensor(dt, layout, case):
    key = (dt, layout) + tuple(case)
    if key not in _TENSORS:
        if len(_TENSORS) > 24:
            _TENSORS.clear()
        base, view = _embed(layout, _problem(dt, case)["X"])
        _TENSORS[key] = view(_dev(base))
    return _TENSORS[key]


def _ref(gpu, dt, case, R="given"):
    """The reference of one call (all groups, the library's default blocks), computed once and left unchanged."""
    key = (dt,) + tuple(case) + (R if isinstance(R, str) else "own",)
    if key not in _REFS:
        n, m, ties, tied = case
        cs = _problem(dt, case)
        depths = ref_.device_depths(gpu, n, P, m, cs["J"], STARTS)
        _REFS[key] = ref_.cox_groupscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties,
                                                   cs["R"] if isinstance(R, str) else R, STARTS, None, depths)
    return _REFS[key]


def _call(gpu, dt, layout, case, **kw):
    cs = _problem(dt, case)
    kw.setdefault("factor", cs["R"])
    return gpu.cox_groupscore_device(_tensor(dt, layout, case), cs["cols"], cs["beta"], cs["time"], cs["status"], STARTS,
                                     weight=cs["w"], ties=case[2], **kw)


def _same_bits(a, b, what):
    for k in ("u", "a", "D", "T", "S", "offsets", "columns"):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_u_a_and_the_blocks_of_d_t_and_s_are_within_the_bounds(gpu, dt, layout):
    for case in (ref_.GPU_CASES if dt == "f64" else F32_CASES):
        n, m, ties, tied = case
        cs = _problem(dt, case)
        t = _tensor(dt, layout, case)
        assert tuple(t.shape) == (n, P)
        got = _call(gpu, dt, layout, case)
        what = "%s %s n=%d m=%d %s%s" % (dt, layout, n, m, ties, " all tied" if tied else "")
        assert got["u"].shape == (P,) and got["T"].shape == (int((WIDTHS * WIDTHS).sum()),)
        assert np.array_equal(got["group_of_column"], np.repeat(np.arange(WIDTHS.size), WIDTHS))
        ref_.check_blocks(got, _ref(gpu, dt, case), what)
        if m == 0:
            assert not got["a"].any() and not got["S"].any()
        # info, score and loglik are cox_information_device's, bit for bit
        inf = gpu.cox_information_device(t, cs["cols"], cs["beta"], cs["time"], cs["status"], weight=cs["w"], ties=ties)
        assert np.array_equal(got["info"], inf["info"]) and np.array_equal(got["score"], inf["score"]), what
        assert got["loglik"] == inf["loglik"] and got["n_events"] == inf["n_events"], what


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_same_call_same_bits_under_every_layout_repeat_and_candidate_block(gpu, dt):
    case = (4097, 31, "order", False)
    ws = gpu.cox_groupscore_workspace(4097, P, 31, _problem(dt, case)["J"], STARTS, candidate_block=64)
    assert ws["t_slabs"] >= 3 and ws["blocks"] > 2 and ws["band"] == 4  # the carry and the cross terms of the finish run
    first = None
    for li, layout in enumerate(LAYOUTS):
        a = _call(gpu, dt, layout, case)
        b = _call(gpu, dt, layout, case)
        c = _call(gpu, dt, layout, case, candidate_block=64 if li % 2 else 128)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d = _call(gpu, dt, layout, case, stream=s.cuda_stream)
        for other in (b, c, d):
            _same_bits(a, other, layout)
            assert np.array_equal(a["info"], other["info"]) and np.array_equal(a["score"], other["score"])
            assert a["loglik"] == other["loglik"]
        first = first or a
        _same_bits(a, first, layout)
        for k in ("D", "T", "S"):
            for blk in groupscoreref._blocks(a[k], a["offsets"]):
                assert np.array_equal(blk, blk.T), (layout, k)


@pytest.mark.parametrize("case", [(37, 3, "order", False), (4097, 3, "breslow", False)], ids=lambda c: "n%d-m%d" % c[:2])
def test_a_tested_subset_gives_the_same_bits_as_the_full_call(gpu, case):
    one = _call(gpu, "f64", "C", case)
    pos, off = np.concatenate([[0], np.cumsum(WIDTHS)]), one["offsets"]
    for groups, block, layout in (([0, 3, 9, 10, 26], 0, "odd_offset"), ([9], 64, "F"), (list(range(1, 27, 2)), 64, "T")):
        sub = _call(gpu, "f64", layout, case, groups=groups, candidate_block=block)
        assert np.array_equal(sub["columns"], np.concatenate([np.arange(STARTS[g], STARTS[g] + WIDTHS[g]) for g in groups]))
        for k in ("u", "a"):
            assert np.array_equal(sub[k], np.concatenate([one[k][pos[g]:pos[g + 1]] for g in groups])), (groups, k)
        for k in ("D", "T", "S"):
            assert np.array_equal(sub[k], np.concatenate([one[k][off[g]:off[g + 1]] for g in groups])), (groups, k)


@pytest.mark.parametrize("ties", ["order", "breslow"])
def test_singleton_groups_agree_with_the_column_call_within_both_bounds(gpu, ties):
    case = (1025, 31, "order", False)  # (the model's data; ties as parametrised)
    n, m = 1025, 31
    cs = _problem("f64", case)
    columns = np.arange(0, P, 7)
    t = _tensor("f64", "F", case)
    args = (t, cs["cols"], cs["beta"], cs["time"], cs["status"])
    grp = gpu.cox_groupscore_device(*args, np.arange(P), groups=columns, weight=cs["w"], ties=ties, factor=cs["R"])
    col = gpu.cox_addscore_device(*args, weight=cs["w"], ties=ties, factor=cs["R"], candidates=columns)
    assert np.array_equal(grp["columns"], col["columns"]) and np.array_equal(grp["offsets"], np.arange(columns.size + 1))
    rg = ref_.cox_groupscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties, cs["R"],
                                       np.arange(P), columns, ref_.device_depths(gpu, n, P, m, cs["J"], np.arange(P), columns))
    rc = coxaddscoreref.cox_addscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], ties,
                                               cs["R"], columns,
                                               coxaddscoreref.device_depths(gpu, n, m, cs["J"], columns.size))
    ref_.check_blocks(grp, rg, "singletons " + ties)
    coxaddscoreref.check_vectors(col, rc, "columns " + ties)
    for k, b in (("u", "bu"), ("a", "ba")):
        assert (np.abs(grp[k] - col[k]).astype(LD) <= rg[b] + rc[b]).all(), (ties, k)
    for k, kc, b, bc in (("D", "d", "bD", "bd"), ("T", "t", "bT", "bt"), ("S", "s", "bS", "bs")):
        bg = np.array([x[0, 0] for x in rg[b]])
        err = np.abs(grp[k] - col[kc]).astype(LD)
        print("%s %s: largest |group - column| %.3e, sum of the bounds there %.3e" % (
            ties, k, float(err.max()), float((bg + rc[bc])[int(np.argmax(err))])))
        assert (err <= bg + rc[bc]).all(), (ties, k)


@pytest.mark.parametrize("case", ref_.GPU_CASES, ids=lambda c: "n%d-m%d-%s%s" % (c[0], c[1], c[2], "-tied" if c[3] else ""))
def test_cox_group_score_test_table_is_within_the_bound_of_the_reference(gpu, case):
    n, m, ties, tied = case
    ci = ref_.GPU_CASES.index(case)
    dt = "f32" if case in F32_CASES and ci % 2 else "f64"
    layout = LAYOUTS[ci % 5]
    got = _call(gpu, dt, layout, case, factor=None)
    what = "%s %s n=%d m=%d %s" % (dt, layout, n, m, ties)
    assert got["positive_definite"], what
    R = gpu.info_factor(got["info"])[0] if m else None
    ref = _ref(gpu, dt, case, R=R) if m else _ref(gpu, dt, case)
    ref_.check_blocks(got, ref, what)
    table = gpu.cox_group_score_test_table(got)
    support = [ref_.GPU_SUPPORT_GROUP[m]] if m else []
    assert np.array_equal(np.nonzero(table["in_model"])[0], support), what
    assert np.array_equal(table["df"], WIDTHS) and np.array_equal(table["first_column"], STARTS), what
    assert table["dispersion"] == 1.0
    cl = table["statistic"][COLLINEAR]  # one column is the sum of two others: NaN, or finite and >= 0
    assert np.isnan(cl) or (np.isfinite(cl) and cl >= 0), what
    if n >= 1025:  # only the support's group and the planted collinear group are left out
        st = ref_.statistic_reference(ref, planted=[COLLINEAR])
        assert int(st["ok"].sum()) == WIDTHS.size - 1 - len(support)
        ref_.check_table(table, st, what)
    else:  # most wide groups are singular (d >= the number of events): NaN, or a value within its bound
        lam = ref_.lambda_min(ref)
        planted = [g for g in range(WIDTHS.size) if not lam[g] >= 0.125]
        st = ref_.statistic_reference(ref, planted=planted)
        ref_.check_table(table, st, what)
        assert st["ok"].sum() >= 5, what


def test_estimator_on_a_device_matrix_agrees_with_the_numpy_route(gpu):
    n, p = 400, 60
    widths = np.array([3, 1, 5, 2, 7, 4, 3, 6, 1, 8, 2, 5, 3, 4, 6])
    cs = ref_.case(n, 4, widths, True, support_group=5)
    labels = np.repeat(np.arange(widths.size) * 2, widths)
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = p, np.zeros(p), 0.0
    est.beta[cs["cols"]] = cs["beta"]
    y = np.column_stack([cs["time"], cs["status"]])
    Xd = _dev(cs["X"])
    for ties in ("order", "breslow"):
        dev = est.score_tests_groups_survival(Xd, _dev(y), labels, weight=_dev(cs["w"]), ties=ties)
        host = est.score_tests_groups_survival(cs["X"], y, labels, weight=cs["w"], ties=ties)
        assert np.array_equal(dev["cols"], cs["cols"]) and np.array_equal(dev["in_model"], host["in_model"])
        assert np.array_equal(dev["df"], widths) and dev["in_model"].sum() == 1
        args = (cs["cols"], cs["beta"], cs["time"], cs["status"])
        info_d = gpu.cox_information_device(Xd, *args, weight=cs["w"], ties=ties)["info"]
        info_h = linear.bess_base._cox_information_host(cs["X"][:, cs["cols"]], *args[1:], cs["w"], ties)["info"]
        J = int((cs["status"] != 0).sum())
        sts = []
        for info, depths, tb in ((info_d, ref_.device_depths(gpu, n, p, 4, J, cs["starts"]), dev),
                                 (info_h, ref_.host_depths(n), host)):
            R, pd = gpu.info_factor(info)
            assert pd
            ref = ref_.cox_groupscore_reference(cs["X"], *args, cs["w"], ties, R, cs["starts"], None, depths)
            st = ref_.statistic_reference(ref)
            ref_.check_table(tb, st, "estimator " + ties)
            sts.append(st)
        ok = sts[0]["ok"]
        width = (sts[0]["hi"] - sts[0]["lo"]) + (sts[1]["hi"] - sts[1]["lo"]) + np.abs(sts[0]["stat"] - sts[1]["stat"])
        assert (np.abs(dev["statistic"] - host["statistic"]).astype(LD)[ok] <= width[ok]).all()
        sub = est.score_tests_groups_survival(Xd, y, labels, weight=cs["w"], ties=ties, groups=[1, 4, 9])
        assert np.array_equal(sub["group"], [1, 4, 9])
        assert np.array_equal(sub["statistic"], dev["statistic"][[1, 4, 9]])
        assert est.score_tests_groups(Xd, y[:, 0], labels) is None


def test_a_group_wider_than_64_columns_is_refused_before_anything_is_written(gpu):
    case = (37, 3, "order", False)
    cs = _problem("f64", case)
    t = _tensor("f64", "C", case)
    args = (t, cs["cols"], cs["beta"], cs["time"], cs["status"])
    starts = np.array([0, 3, 67, 132])  # widths 3, 64, 65, 274
    got = gpu.cox_groupscore_device(*args, starts, groups=[0, 1], factor=cs["R"], weight=cs["w"])
    assert got["offsets"].tolist() == [0, 9, 9 + 64 * 64]
    ref = ref_.cox_groupscore_reference(cs["X"], cs["cols"], cs["beta"], cs["time"], cs["status"], cs["w"], "order", cs["R"],
                                        starts, [0, 1], ref_.device_depths(gpu, 37, P, 3, cs["J"], starts, [0, 1]))
    ref_.check_blocks(got, ref, "a group of 64 columns")
    with pytest.raises(gpu.BessxError) as e:
        gpu.cox_groupscore_device(*args, starts, groups=[1, 2], factor=cs["R"])
    assert e.value.code == 3 and "group 2 has 65 columns" in str(e.value)
    # the raw call: the outputs are untouched
    import ctypes
    a = gpu.CoxGroupscoreInput()
    dx = gpu._DeviceArray(t, "x", 2)
    keep = dict(cols=cs["cols"].astype(np.int32), starts=starts.astype(np.int32), groups=np.array([1, 2], dtype=np.int32),
                info=np.full((3, 3), 7.0), score=np.full(3, 7.0), vec=np.full((2, 129), 7.0), blk=np.full((3, 8321), 7.0),
                offsets=np.full(3, 7, dtype=np.int64))
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = dx.ptr, dx.dtype, dx.strides[0], dx.strides[1], 37, P
    a.cols, a.m, a.beta = gpu._ip(keep["cols"]), 3, gpu._dp(cs["beta"])
    a.time, a.status, a.ties = gpu._dp(cs["time"]), gpu._dp(cs["status"]), 0
    a.group_starts, a.n_groups, a.groups, a.n_tested = gpu._ip(keep["starts"]), 4, gpu._ip(keep["groups"]), 2
    a.info, a.info_ld, a.score = gpu._dp(keep["info"]), 3, gpu._dp(keep["score"])
    a.u, a.a = keep["vec"][0].ctypes.data, keep["vec"][1].ctypes.data
    a.D, a.T, a.S = (keep["blk"][k].ctypes.data for k in range(3))
    a.offsets = keep["offsets"].ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    out = [ctypes.c_double(7.0) for _ in range(3)]
    assert gpu.lib().bessx_cox_groupscore_device(ctypes.byref(a), *[ctypes.byref(o) for o in out]) == 3
    for k in ("info", "score", "vec", "blk", "offsets"):
        assert (keep[k] == 7).all(), k
    assert all(o.value == 7.0 for o in out)


def test_device_memory_is_given_back(gpu):
    case = (1025, 31, "order", False)
    before = gpu.process_counters()
    _call(gpu, "f64", "C", case, candidate_block=128)
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
