"""Score tests of excluded GROUPS of columns on an X already in GPU memory (bessx_groupscore_device,
bess_amd/csrc/bessx_k_groupscore.hip) against NumPy in np.longdouble on the host copy of the same values, within the
bounds derived in tests/groupscoreref.py (the addition depths are those of the split the library reports).  Shapes: n = 37
(one partial slab of the Gram kernel past a 32-row chunk) and n = 4097 (32 slabs, the last one short, one row past a
16-byte boundary); p = 406 columns in 27 groups whose widths are drawn from {1, 2, 3, 5, 15, 16, 17, 31, 33, 64} in an
order in which a group starts at every offset 0 .. 15 of a 16-column tile and groups straddle one, two and four tile
boundaries (the 64-wide one starts at offset 15: the widest band, five tiles); supports of m = 3 and m = 31 columns, each a
whole group (one and three panel tiles); candidate blocks of 64 and 128 columns, which cut the list at other group
boundaries and move every later group to another tile offset.  Layouts are those of tests/test_addscore_gpu.py, every
element outside the view a NaN.  Weights are multiples of 1/8 with zeros."""
import numpy as np
import pytest

import groupscoreref
from bess_amd import linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
LINKS = ["identity", "logistic", "poisson"]
WIDTHS = np.array([31, 5, 3, 17, 31, 1, 17, 33, 5, 64, 16, 1, 3, 15, 31, 15, 5, 1, 5, 31, 15, 3, 17, 1, 5, 2, 33])
STARTS = np.concatenate([[0], np.cumsum(WIDTHS)[:-1]])
P = int(WIDTHS.sum())  # 406
SUPPORT_GROUP = {3: 2, 31: 4}  # m -> the group that is the model's support
COLLINEAR, SIGNAL = 8, 16     # a group whose third column is the sum of its first two; the group y depends on
CASES = [(37, 3), (37, 31), (4097, 3), (4097, 31)]


def test_the_widths_cover_what_the_tiling_can_get_wrong():
    assert set(int(s) % 16 for s in STARTS) == set(range(16))
    assert set(int(w) for w in WIDTHS) == {1, 2, 3, 5, 15, 16, 17, 31, 33, 64}
    crossed = (STARTS + WIDTHS - 1) // 16 - STARTS // 16
    assert {1, 2, 4} <= set(int(c) for c in crossed) and STARTS[9] % 16 == 15 and WIDTHS[9] == 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _embed(layout, vals):
    """(base host array that holds vals in the layout under test, NaN everywhere else; base tensor -> the n x p view)"""
    n, p = vals.shape
    if layout == "C":  # row-major
        return vals.copy(), (lambda t: t)
    if layout == "F":  # column-major with a padded leading dimension: aligned columns (the 16-byte loads), NaN rows >= n
        b = np.full((p, (n + 3) // 4 * 4), np.nan, dtype=vals.dtype)
        b[:, :n] = vals.T
        return b, (lambda t: t[:, :n].T)
    if layout == "T":  # a transposed view that starts on an odd element: column-contiguous, element loads
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


def _gcols(g):
    return np.arange(STARTS[g], STARTS[g] + WIDTHS[g])


_PROBLEMS, _REFS, _TENSORS = {}, {}, {}


def _problem(dt, n, m):
    """One model per (dtype, n, m), the same logical values under every layout: the support is one whole group, the
    responses of the three families depend on the support and on the left-out group SIGNAL, the third column of the
    group COLLINEAR is the sum of its first two, weights have zeros among them, and R is a random well-scaled
    lower-triangular factor."""
    key = (dt, n, m)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + (7 if dt == "f32" else 0))
        vals = np.random.default_rng(n + m + (1 if dt == "f32" else 0)).standard_normal((n, P)).astype(DT[dt])
        cc = _gcols(COLLINEAR)
        vals[:, cc[2]] = vals[:, cc[0]] + vals[:, cc[1]]
        cols = _gcols(SUPPORT_GROUP[m]).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(m)
        c = 0.3
        extra = vals[:, _gcols(SIGNAL)].astype(np.float64) @ np.array([0.6, -0.5, 0.4, 0.5, -0.6])
        eta = vals[:, cols].astype(np.float64) @ beta + c
        ys = {"identity": eta + extra + rng.standard_normal(n),
              "logistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-(eta + extra)))).astype(float),
              "poisson": rng.poisson(np.exp(np.clip(eta + extra, -5, 3))).astype(float)}
        w = rng.integers(0, 17, n) / 8.0
        M = m + 1
        R = np.tril(rng.standard_normal((M, M))) / np.sqrt(float(n) * M)
        _PROBLEMS[key] = dict(vals=vals, cols=cols, beta=beta, c=c, ys=ys, w=w, R=R)
    return _PROBLEMS[key]


def _tensor(dt, layout, n, m):
    key = (dt, layout, n, m)
    if key not in _TENSORS:
        if len(_TENSORS) > 24:
            _TENSORS.clear()
        base, view = _embed(layout, _problem(dt, n, m)["vals"])
        _TENSORS[key] = view(_dev(base))
    return _TENSORS[key]


def _ref(gpu, dt, n, m, link, weighted=True, groups=None, block=0, R="given"):
    """The reference of one call, computed once and left unchanged."""
    key = (dt, n, m, link, weighted, None if groups is None else tuple(groups), block, R if isinstance(R, str) else "own")
    if key not in _REFS:
        pr = _problem(dt, n, m)
        depths = groupscoreref.device_depths(gpu, n, P, m, STARTS, groups, block)
        _REFS[key] = groupscoreref.groupscore_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], pr["ys"][link],
                                                        pr["w"] if weighted else None, link,
                                                        pr["R"] if isinstance(R, str) else R, STARTS, groups, depths)
    return _REFS[key]


def _call(gpu, dt, layout, n, m, link, **kw):
    pr = _problem(dt, n, m)
    kw.setdefault("weight", pr["w"])
    kw.setdefault("factor", pr["R"])
    return gpu.groupscore_device(_tensor(dt, layout, n, m), pr["cols"], pr["beta"], pr["c"], pr["ys"][link], STARTS,
                                 link=link, **kw)


def _same_bits(a, b, what):
    for k in ("u", "a", "D", "S", "offsets", "columns"):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_u_a_and_the_blocks_of_d_and_s_are_within_the_bounds(gpu, dt, layout):
    for ci, (n, m) in enumerate(CASES):
        link = LINKS[ci % 3]
        pr = _problem(dt, n, m)
        t = _tensor(dt, layout, n, m)
        assert tuple(t.shape) == (n, P)
        w = _dev(pr["w"]) if ci % 2 else pr["w"]
        got = _call(gpu, dt, layout, n, m, link, weight=w)
        what = "%s %s n=%d m=%d %s" % (dt, layout, n, m, link)
        assert got["u"].shape == (P,) and got["D"].shape == (int((WIDTHS * WIDTHS).sum()),)
        assert np.array_equal(got["group_of_column"], np.repeat(np.arange(WIDTHS.size), WIDTHS))
        groupscoreref.check_blocks(got, _ref(gpu, dt, n, m, link), what)
        # info, score, loss and sum_w are information_device's, bit for bit
        inf = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], pr["ys"][link], link=link, weight=w)
        assert np.array_equal(got["info"], inf["info"]) and np.array_equal(got["score"], inf["score"]), what
        assert got["loss"] == inf["loss"] and got["sum_w"] == inf["sum_w"], what


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_same_call_same_bits_and_every_layout_gives_the_same_bits(gpu, dt):
    n, m = 4097, 31
    pr = _problem(dt, n, m)
    y, w = _dev(pr["ys"]["poisson"]), _dev(pr["w"])
    torch.cuda.synchronize()
    first = None
    for layout in LAYOUTS:
        t = _tensor(dt, layout, n, m)
        args = (t, pr["cols"], pr["beta"], pr["c"], y, STARTS)
        a = gpu.groupscore_device(*args, link="poisson", weight=w, factor=pr["R"])
        b = gpu.groupscore_device(*args, link="poisson", weight=w, factor=pr["R"])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = gpu.groupscore_device(*args, link="poisson", weight=w, factor=pr["R"], stream=s.cuda_stream)
        for other in (b, c):
            _same_bits(a, other, layout)
            assert np.array_equal(a["info"], other["info"]) and np.array_equal(a["score"], other["score"])
            assert a["loss"] == other["loss"] and a["sum_w"] == other["sum_w"]
        first = first or a
        _same_bits(a, first, layout)
        for k in ("D", "S"):
            for blk in groupscoreref._blocks(a[k], a["offsets"]):
                assert np.array_equal(blk, blk.T), (layout, k)


@pytest.mark.parametrize("case", [(37, 3), (4097, 31)], ids=lambda c: "n%d-m%d" % c)
def test_blocks_cut_at_group_boundaries_and_subsets_give_the_same_bits(gpu, case):
    n, m = case
    one = _call(gpu, "f64", "C", n, m, "logistic")
    assert gpu.groupscore_workspace(n, P, m, STARTS)["blocks"] == 1
    for block, layout in ((64, "F"), (128, "C"), (64, "two_strides")):
        ws = gpu.groupscore_workspace(n, P, m, STARTS, candidate_block=block)
        assert ws["blocks"] > 2 and ws["band"] == 4
        width = np.diff(np.cumsum(np.concatenate([[0], WIDTHS]))[ws["block_first"]])
        assert (width <= block).all() and width.sum() == P
        _same_bits(one, _call(gpu, "f64", layout, n, m, "logistic", candidate_block=block), (block, layout))
    pos, off = np.concatenate([[0], np.cumsum(WIDTHS)]), one["offsets"]
    for groups, block in (([0, 3, 9, 10, 26], 0), ([1, 2, 5, 11, 12, 17], 0), ([9], 64), (list(range(1, 27, 2)), 64)):
        sub = _call(gpu, "f64", "odd_offset", n, m, "logistic", groups=groups, candidate_block=block)
        assert np.array_equal(sub["columns"], np.concatenate([_gcols(g) for g in groups]))
        assert np.array_equal(sub["group_of_column"], np.repeat(groups, WIDTHS[groups]))
        for k in ("u", "a"):
            assert np.array_equal(sub[k], np.concatenate([one[k][pos[g]:pos[g + 1]] for g in groups])), (groups, k)
        for k in ("D", "S"):
            assert np.array_equal(sub[k], np.concatenate([one[k][off[g]:off[g + 1]] for g in groups])), (groups, k)


def test_the_width_limit_and_the_block_limit(gpu):
    n, m = 37, 3
    pr = _problem("f64", n, m)
    t = _tensor("f64", "C", n, m)
    args = (t, pr["cols"], pr["beta"], pr["c"], pr["ys"]["identity"])
    starts = np.array([0, 3, 67, 132])  # widths 3, 64, 65, 274
    got = gpu.groupscore_device(*args, starts, groups=[0, 1], factor=pr["R"], weight=pr["w"])
    assert got["offsets"].tolist() == [0, 9, 9 + 64 * 64]
    ref = groupscoreref.groupscore_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], pr["ys"]["identity"], pr["w"],
                                             "identity", pr["R"], starts, [0, 1],
                                             groupscoreref.device_depths(gpu, n, P, m, starts, [0, 1]))
    groupscoreref.check_blocks(got, ref, "a group of 64 columns")
    with pytest.raises(gpu.BessxError) as e:
        gpu.groupscore_device(*args, starts, groups=[1, 2], factor=pr["R"])
    assert e.value.code == 3 and "group 2 has 65 columns" in str(e.value)
    with pytest.raises(gpu.BessxError) as e:
        gpu.groupscore_device(*args, starts, groups=[0, 1], factor=pr["R"], candidate_block=48)
    assert e.value.code == 1 and "candidate_block must be at least" in str(e.value)


def _planted(n, m):
    """The groups left out of the statistic's check, explicitly: the collinear one, and at n = 37 every group so wide
    that the few rows cannot hold lambda_min of its scaled D - S at 1/16."""
    return [COLLINEAR] + ([g for g in range(WIDTHS.size) if WIDTHS[g] > 5] if n == 37 else [])


@pytest.mark.parametrize("case", [(37, 3), (4097, 3), (4097, 31)], ids=lambda c: "n%d-m%d" % c)
def test_group_score_test_table_is_within_the_interval_of_the_reference(gpu, case):
    n, m = case
    ci = CASES.index(case)
    for li, link in enumerate(LINKS):
        dt = "f32" if (ci + li) % 3 == 2 else "f64"
        layout = LAYOUTS[(ci + 2 * li) % 5]
        got = _call(gpu, dt, layout, n, m, link, factor=None)
        what = "%s %s n=%d m=%d %s" % (dt, layout, n, m, link)
        assert got["positive_definite"], what
        R, pd = gpu.info_factor(got["info"])
        ref = _ref(gpu, dt, n, m, link, R=R)
        groupscoreref.check_blocks(got, ref, what)
        table = gpu.group_score_test_table(got, link)
        st = groupscoreref.statistic_reference(ref, planted=_planted(n, m))
        groupscoreref.check_table(table, st, what)
        assert np.array_equal(np.nonzero(table["in_model"])[0], [SUPPORT_GROUP[m]]), what
        assert np.array_equal(table["df"], WIDTHS) and np.array_equal(table["first_column"], STARTS), what
        cl = table["statistic"][COLLINEAR]  # one column is the sum of two others: NaN, or finite and >= 0
        assert np.isnan(cl) or (np.isfinite(cl) and cl >= 0), what
        if n == 4097:
            assert int(np.nanargmin(np.where(np.arange(WIDTHS.size) == COLLINEAR, np.nan, table["p_value"]))) == SIGNAL, what


def test_identity_statistic_times_dispersion_is_the_drop_of_a_longdouble_refit(gpu):
    """(u - a)^T (D - S)^-1 (u - a) = RSS_A - RSS_{A + group} for the identity link, whatever beta is.  Reference:
    weighted least squares refitted in longdouble for every asserted group.  Bound: the interval of groupscoreref for
    the statistic plus the refit's own cancellation error, 64 * 2^-64 * RSS_A * (condition of the normal equations, at
    most 256 here: two residual sums of squares of that size are subtracted in longdouble)."""
    n, m = 4097, 3
    pr = _problem("f64", n, m)
    y, w = pr["ys"]["identity"], pr["w"]
    got = _call(gpu, "f64", "F", n, m, "identity", factor=None)
    R, pd = gpu.info_factor(got["info"])
    assert pd
    ref = _ref(gpu, "f64", n, m, "identity", R=R)
    st = groupscoreref.statistic_reference(ref, planted=_planted(n, m))
    table = gpu.group_score_test_table(got, "identity")
    Z = np.concatenate([np.ones((n, 1), dtype=LD), pr["vals"][:, pr["cols"]].astype(LD)], axis=1)
    coef = groupscoreref.chol_solve((Z * w.astype(LD)[:, None]).T @ Z, (Z * w.astype(LD)[:, None]).T @ y.astype(LD))
    rss_a = (w.astype(LD) * (y.astype(LD) - Z @ coef) ** 2).sum()
    worst = 0.0
    for g in np.nonzero(st["ok"])[0][::3]:
        drop = groupscoreref.rss_drop_reference(pr["vals"], pr["cols"], y, w, _gcols(g))
        have = LD(table["statistic"][g]) * LD(table["dispersion"])
        phi = st["dispersion"]
        lo, hi = st["lo"][g] * phi * (1 - LD(1e-12)), st["hi"][g] * phi * (1 + LD(1e-12))
        allow = (hi - lo) + LD(64 * 256) * LD(2.0) ** -64 * rss_a
        worst = max(worst, float(abs(have - drop) / allow))
        assert abs(have - drop) <= allow, (g, float(have), float(drop), float(allow))
    print("largest |statistic * dispersion - drop| / allowance %.3e" % worst)


@pytest.mark.parametrize("name", ["PdasLm", "PdasLogistic", "PdasPoisson"])
def test_estimator_score_tests_groups_on_a_device_matrix_agree_with_the_numpy_route(gpu, name):
    n, p, k = 400, 60, 4
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p))
    truth = np.zeros(p)
    truth[rng.choice(p, k, replace=False)] = np.array([1.0, -1.0, 0.8, -0.8])
    eta = X @ truth + 0.2
    y = {"PdasLm": eta + rng.standard_normal(n), "PdasLogistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))) * 1.0,
         "PdasPoisson": rng.poisson(np.exp(eta)) * 1.0}[name]
    est = getattr(linear, name)(sequence=[2])  # two of the four true columns: the other two are left out
    Xd = _dev(X)
    est.fit(Xd, y)
    link = est._LINK[est.model_type_int]
    cols = np.nonzero(est.beta)[0]
    widths = np.array([3, 1, 5, 2, 7, 4, 3, 6, 1, 8, 2, 5, 3, 4, 6])
    starts, labels = np.concatenate([[0], np.cumsum(widths)[:-1]]), np.repeat(np.arange(widths.size) * 2, widths)
    assert widths.sum() == p
    dev, host = est.score_tests_groups(Xd, _dev(y), labels), est.score_tests_groups(X, y, labels)
    assert np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    assert np.array_equal(dev["in_model"], host["in_model"]) and np.array_equal(dev["df"], widths)
    b, c0 = est.beta[cols], float(np.ravel(est.coef0)[0])
    info_d = gpu.information_device(Xd, cols, b, c0, y, link=link)["info"]
    info_h = linear.bess_base._information_host(link, X[:, cols], b, c0, y, np.ones(n))["info"]
    sts = []
    for info, depths, tb in ((info_d, groupscoreref.device_depths(gpu, n, p, cols.size, starts), dev),
                             (info_h, groupscoreref.host_depths(n), host)):
        R, pd = gpu.info_factor(info)
        assert pd
        ref = groupscoreref.groupscore_reference(X, cols, b, c0, y, None, link, R, starts, None, depths)
        st = groupscoreref.statistic_reference(ref)
        groupscoreref.check_table(tb, st, name)
        sts.append(st)
    ok = sts[0]["ok"]
    width = (sts[0]["hi"] - sts[0]["lo"]) + (sts[1]["hi"] - sts[1]["lo"]) + np.abs(sts[0]["stat"] - sts[1]["stat"])
    assert (np.abs(sts[0]["stat"] - sts[1]["stat"])[ok] <= LD(1e-9) * sts[0]["stat"][ok] + LD(1e-12)).all()
    assert (np.abs(dev["statistic"] - host["statistic"]).astype(LD)[ok] <= width[ok]).all()
    group_of = np.repeat(np.arange(widths.size), widths)
    left_out = np.setdiff1d(group_of[np.nonzero(truth)[0]], group_of[cols])
    assert left_out.size >= 1 and int(np.nanargmin(dev["p_value"])) in left_out
    sub = est.score_tests_groups(Xd, y, labels, groups=left_out)
    assert np.array_equal(sub["group"], left_out)
    assert np.allclose(sub["statistic"], dev["statistic"][left_out], rtol=1e-9)


def test_a_nan_outside_the_view_is_never_read_and_one_inside_propagates(gpu):
    n, m = 37, 3
    pr = _problem("f64", n, m)
    groups = [0, 5, 9, 12, 20]
    tested = np.concatenate([_gcols(g) for g in groups])
    vals = pr["vals"].copy()
    other = np.setdiff1d(np.arange(P), np.concatenate([pr["cols"], tested]))
    vals[:, other] = np.nan  # columns that are neither in the support nor in a tested group
    ref = _ref(gpu, "f64", n, m, "logistic", groups=groups)
    args = (pr["cols"], pr["beta"], pr["c"], pr["ys"]["logistic"], STARTS)
    for layout in ("C", "F"):
        base, view = _embed(layout, vals)
        got = gpu.groupscore_device(view(_dev(base)), *args, groups=groups, link="logistic", weight=pr["w"],
                                    factor=pr["R"])
        groupscoreref.check_blocks(got, ref, "NaN outside " + layout)
        inside = pr["vals"].copy()
        inside[29, _gcols(9)[40]] = np.nan  # one column of the 64-wide group: its row and column of that group's blocks
        base, view = _embed(layout, inside)
        got = gpu.groupscore_device(view(_dev(base)), *args, groups=groups, link="logistic", weight=pr["w"],
                                    factor=pr["R"])
        j = int(WIDTHS[0] + WIDTHS[5] + 40)
        want = np.arange(tested.size) == j
        for k in ("u", "a"):
            assert np.array_equal(np.isnan(got[k]), want), (layout, k)
        for k in ("D", "S"):
            for ti, blk in enumerate(groupscoreref._blocks(got[k], got["offsets"])):
                bad = np.zeros(blk.shape, dtype=bool)
                if groups[ti] == 9:
                    bad[40, :] = bad[:, 40] = True
                assert np.array_equal(np.isnan(blk), bad), (layout, k, ti)


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    t = _tensor("f64", "C", n, m)
    y, w = pr["ys"]["logistic"], _dev(pr["w"])

    def call():
        gpu.groupscore_device(t, pr["cols"], pr["beta"], pr["c"], y, STARTS, link="logistic", weight=w, factor=pr["R"],
                              candidate_block=128)
        return gpu.process_counters()

    before = gpu.process_counters()
    first = call()
    second = call()
    third = call()
    for c in (first, second, third):
        assert c["live_device_bytes"] == before["live_device_bytes"]
        assert c["live_pinned_bytes"] == before["live_pinned_bytes"]
    added = second["allocation_requests"] - first["allocation_requests"]
    assert added > 0 and third["allocation_requests"] - second["allocation_requests"] == added
