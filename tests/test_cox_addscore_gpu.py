"""Cox score tests of the excluded columns on an X already in GPU memory (bessx_cox_addscore_device,
bess_amd/csrc/bessx_k_coxaddscore.hip) against NumPy in np.longdouble on the host copy of the same values, by the explicit
risk-set definition and within the bounds derived in tests/coxaddscoreref.py (the addition chains are those of the
splits the library reports).  Shapes are the smallest at which each mechanism can go wrong: the null model, one support
column, candidates that cross a block, a scattered list, one position past the 1024-position scan block, and several
position slabs so that the carry of the risk-set term is exercised.  Layouts are those of tests/test_addscore_gpu.py,
every element outside the view a NaN.  Times are rounded to eighths (real tie groups), weights are multiples of 1/8 with
zeros."""
import numpy as np
import pytest

import coxaddscoreref
import coxinforef
from bess_amd import linear
from test_addscore_gpu import LAYOUTS, _dev, _embed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
TIES = ["order", "breslow"]
# (n, p, m, candidates: None = all / "scattered" = 37 of p / "support", candidate_block)
CASES = [(31, 40, 0, None, 0), (33, 40, 1, None, 16), (127, 70, 15, None, 32), (203, 70, 16, "scattered", 0),
         (1025, 70, 31, None, 0), (4097, 50, 5, None, 16)]
ROUTES = [("f64", "F"), ("f64", "C"), ("f32", "C")]

_PROBLEMS, _REFS = {}, {}


def _problem(dt, n, p, m, all_tied=False):
    """One model per (dtype, n, p, m), the same logical values under every layout: standard-normal columns, a linear
    predictor with a standard deviation of about 1, times on a grid of eighths, censoring, weights with zeros."""
    key = (dt, n, p, m, all_tied)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + (7 if dt == "f32" else 0))
        vals = rng.standard_normal((n, p)).astype(DT[dt])
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        eta = vals[:, cols].astype(np.float64) @ beta
        time = np.ceil(rng.exponential(np.exp(-eta)) * 8) / 8
        if all_tied:
            time[:] = 2.0
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0
        _PROBLEMS[key] = dict(vals=vals, cols=cols, beta=beta, time=time, status=status, w=w)
    return _PROBLEMS[key]


def _tensor(layout, vals):
    base, view = _embed(layout, vals)
    return view(_dev(base))


def _cand(pr, p, kind):
    if kind is None:
        return None
    if kind == "support":
        return pr["cols"].astype(np.int64)
    return np.sort(np.random.default_rng(p).choice(p, 37, replace=False))


def _factor(gpu, t, pr, w, ties):
    """The factor a call is given: from the device information of the same model (None at m = 0)."""
    if pr["cols"].size == 0:
        return None
    info = gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=w, ties=ties)["info"]
    R, pd = gpu.info_factor(info)
    assert pd
    return R


def _ref(gpu, pr, w, ties, R, cand, block, key=None):
    if key is None or key not in _REFS:
        n, p = pr["vals"].shape
        q = p if cand is None else cand.size
        depths = coxaddscoreref.device_depths(gpu, n, pr["cols"].size, int(pr["status"].sum()), q, block)
        ref = coxaddscoreref.cox_addscore_reference(pr["vals"], pr["cols"], pr["beta"], pr["time"], pr["status"], w,
                                                    ties, R, cand, depths)
        if key is None:
            return ref
        _REFS[key] = ref
    return _REFS[key]


def _call(gpu, t, pr, w, ties, R, cand=None, block=0, **kw):
    return gpu.cox_addscore_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=w, ties=ties, factor=R,
                                   candidates=cand, candidate_block=block, want_cross=True, **kw)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-m%d-%s-b%d" % c)
def test_u_d_t_s_a_cross_and_the_table_are_within_the_bounds(gpu, case, ties, weighted):
    n, p, m, kind, block = case
    for dt, layout in ROUTES:
        pr = _problem(dt, n, p, m)
        w = pr["w"] if weighted else None
        cand = _cand(pr, p, kind)
        t = _tensor(layout, pr["vals"])
        R = _factor(gpu, _tensor("F", pr["vals"]), pr, w, ties)  # (one factor per dtype: the same reference serves F and C)
        ref = _ref(gpu, pr, w, ties, R, cand, block, key=(dt, case, ties, weighted))
        got = _call(gpu, t, pr, w, ties, R, cand, block)
        what = "%s %s %s %s w=%s" % (case, dt, layout, ties, weighted)
        coxaddscoreref.check_vectors(got, ref, what)
        coxaddscoreref.check_table(gpu.cox_score_test_table(got), coxaddscoreref.statistic_reference(ref), what)
        assert float(got["n_events"]) == float(ref["n_events"])


@pytest.mark.parametrize("ties", TIES)
def test_all_times_equal(gpu, ties):
    n, p, m = 127, 40, 3
    pr = _problem("f64", n, p, m, all_tied=True)
    for layout in ("F", "C"):
        t = _tensor(layout, pr["vals"])
        R = _factor(gpu, t, pr, pr["w"], ties)
        ref = _ref(gpu, pr, pr["w"], ties, R, None, 0)
        got = _call(gpu, t, pr, pr["w"], ties, R)
        coxaddscoreref.check_vectors(got, ref, "all tied " + layout + " " + ties)
        coxaddscoreref.check_table(gpu.cox_score_test_table(got), coxaddscoreref.statistic_reference(ref), "all tied")


def test_candidates_equal_to_the_support_have_noise_for_a_variance(gpu):
    n, p, m = 203, 70, 16
    pr = _problem("f64", n, p, m)
    cand = _cand(pr, p, "support")
    for layout in ("F", "C"):
        t = _tensor(layout, pr["vals"])
        R = _factor(gpu, t, pr, pr["w"], "breslow")
        ref = _ref(gpu, pr, pr["w"], "breslow", R, cand, 0)
        got = _call(gpu, t, pr, pr["w"], "breslow", R, cand)
        coxaddscoreref.check_vectors(got, ref, "support as candidates " + layout)
        st = coxaddscoreref.statistic_reference(ref)
        table = gpu.cox_score_test_table(got)
        coxaddscoreref.check_table(table, st, "support as candidates")
        assert table["in_model"].all() and np.isnan(table["statistic"]).all() and np.isnan(table["p_value"]).all()
        assert (np.abs(table["variance"].astype(LD) - st["var"]) <= st["bvar"] + LD(2.0) ** -50 * ref["d"]).all()
        assert (np.abs(table["variance"]).astype(LD) <= LD(1e-9) * ref["d"]).all()  # (rounding noise)


@pytest.mark.parametrize("ties", TIES)
def test_the_extended_model_of_section_2h_has_the_same_row(gpu, ties):
    """Independent of the new reference: cox_information_device on cols + [j] with a zero coefficient appended."""
    n, p, m = 1025, 70, 31
    pr = _problem("f64", n, p, m)
    t = _tensor("C", pr["vals"])
    w, J = pr["w"], int(pr["status"].sum())
    R = _factor(gpu, t, pr, w, ties)
    got = _call(gpu, t, pr, w, ties, R)
    ref = _ref(gpu, pr, w, ties, R, None, 0)
    free = np.setdiff1d(np.arange(p), pr["cols"])
    for j in free[[0, 7, 15, 23, -1]]:
        ext = np.sort(np.append(pr["cols"], j)).astype(np.int32)
        at = int(np.searchsorted(ext, j))
        b = np.insert(pr["beta"], at, 0.0)
        big = gpu.cox_information_device(t, ext, b, pr["time"], pr["status"], weight=w, ties=ties)
        rb = coxinforef.cox_information_reference(pr["vals"], ext, b, pr["time"], pr["status"], w, ties,
                                                  coxinforef.device_depths(gpu, n, m + 1, J))
        rest = np.delete(np.arange(m + 1), at)
        eu = abs(LD(big["score"][at]) - LD(got["u"][j]))
        ec = np.abs(big["info"][at, rest].astype(LD) - got["cross"][j].astype(LD))
        dv = LD(got["d"][j]) - LD(got["t"][j])
        ed = abs(LD(big["info"][at, at]) - dv)
        print("candidate %d: u %.2e (%.2e), c %.2e, d - t %.2e (%.2e)" % (
            j, float(eu), float(rb["score_bound"][at] + ref["bu"][j]), float(ec.max()), float(ed),
            float(rb["info_bound"][at, at] + ref["bd"][j] + ref["bt"][j])))
        assert eu <= rb["score_bound"][at] + ref["bu"][j]
        assert (ec <= rb["info_bound"][at, rest] + ref["bC"][j]).all()
        assert ed <= rb["info_bound"][at, at] + ref["bd"][j] + ref["bt"][j]


def test_same_call_same_bits_and_every_layout_gives_the_same_bits(gpu):
    n, p, m = 4097, 70, 31
    pr = _problem("f64", n, p, m)
    w = pr["w"]
    R = _factor(gpu, _tensor("F", pr["vals"]), pr, w, "breslow")
    first = None
    for layout in LAYOUTS:
        t = _tensor(layout, pr["vals"])
        a = _call(gpu, t, pr, w, "breslow", R)
        b = _call(gpu, t, pr, w, "breslow", R)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = _call(gpu, t, pr, w, "breslow", R, stream=s.cuda_stream)
        for other in (b, c):
            for k in ("u", "d", "t", "s", "a", "cross", "info", "score"):
                assert np.array_equal(a[k], other[k]), (layout, k)
            assert a["loglik"] == other["loglik"] and a["residual_sum"] == other["residual_sum"]
        one = gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=w, ties="breslow")
        assert np.array_equal(a["info"], one["info"]) and np.array_equal(a["score"], one["score"]), layout
        assert a["loglik"] == one["loglik"] and a["n_events"] == one["n_events"], layout
        assert a["residual_sum"] == one["residual_sum"], layout
        first = first or a
        for k in ("u", "d", "t", "s", "a", "cross"):
            assert np.array_equal(a[k], first[k]), (layout, k)


@pytest.mark.parametrize("layout", ["C", "F"])
def test_the_largest_support_and_one_past_it(gpu, layout):
    n, p, m = 127, 1040, 1023
    pr = _problem("f64", n, p, m)
    rng = np.random.default_rng(5)
    # (n < m: the information has no factor of its own; a random one, scaled so that s stays below d as a real one's does)
    R = np.tril(rng.standard_normal((m, m))) / (16.0 * np.sqrt(float(n) * m))
    cand = _cand(pr, p, "scattered")
    t = _tensor(layout, pr["vals"])
    ref = _ref(gpu, pr, pr["w"], "order", R, cand, 0, key=("largest",))
    got = _call(gpu, t, pr, pr["w"], "order", R, cand)
    coxaddscoreref.check_vectors(got, ref, "m + 1 = 1024 " + layout)
    with pytest.raises(gpu.BessxError) as e:
        gpu.cox_addscore_device(t, np.arange(1024), np.zeros(1024), pr["time"], pr["status"], factor=np.eye(1024))
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)


def test_a_nan_outside_the_view_is_never_read_and_one_inside_reaches_its_candidate_only(gpu):
    n, p, m = 127, 70, 15
    pr = _problem("f64", n, p, m)
    cand = np.sort(np.random.default_rng(2).choice(np.setdiff1d(np.arange(p), pr["cols"]), 20, replace=False))
    vals = pr["vals"].copy()
    other = np.setdiff1d(np.arange(p), np.concatenate([pr["cols"], cand]))
    vals[:, other] = np.nan  # columns that are neither in the support nor candidates
    R = _factor(gpu, _tensor("F", pr["vals"]), pr, pr["w"], "breslow")
    ref = _ref(gpu, pr, pr["w"], "breslow", R, cand, 0)
    for layout in ("C", "F"):
        got = _call(gpu, _tensor(layout, vals), pr, pr["w"], "breslow", R, cand)
        coxaddscoreref.check_vectors(got, ref, "NaN outside " + layout)
        inside = pr["vals"].copy()
        inside[77, cand[3]] = np.nan  # one candidate's column: that candidate alone is NaN
        got = _call(gpu, _tensor(layout, inside), pr, pr["w"], "breslow", R, cand)
        want = np.arange(cand.size) == 3
        for k in ("u", "d", "t", "s", "a"):
            assert np.array_equal(np.isnan(got[k]), want), (layout, k)
        assert np.array_equal(np.isnan(got["cross"]).any(axis=1), want), layout


def test_no_event_gives_zeros_and_a_nan_table(gpu):
    n, p, m = 127, 70, 15
    pr = dict(_problem("f64", n, p, m))
    pr["status"] = np.zeros(n)
    got = gpu.cox_addscore_device(_tensor("C", pr["vals"]), pr["cols"], pr["beta"], pr["time"], pr["status"],
                                  want_cross=True)
    for k in ("u", "d", "t", "cross"):
        assert (got[k] == 0).all(), k
    assert not got["positive_definite"] and np.isnan(got["s"]).all() and np.isnan(got["a"]).all()
    table = gpu.cox_score_test_table(got)
    assert np.isnan(table["statistic"]).all() and np.isnan(table["p_value"]).all()


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, p, m = 4097, 70, 31
    pr = _problem("f64", n, p, m)
    t = _tensor("C", pr["vals"])
    R = _factor(gpu, t, pr, pr["w"], "order")

    def call():
        got = _call(gpu, t, pr, pr["w"], "order", R)
        return got, gpu.process_counters()

    before = gpu.process_counters()
    (g1, first), (g2, second), (g3, third) = call(), call(), call()
    for c in (first, second, third):
        assert c["live_device_bytes"] == before["live_device_bytes"]
        assert c["live_pinned_bytes"] == before["live_pinned_bytes"]
    added = second["allocation_requests"] - first["allocation_requests"]
    assert added > 0 and third["allocation_requests"] - second["allocation_requests"] == added
    for k in ("u", "d", "t", "s", "a", "cross"):
        assert np.array_equal(g1[k], g2[k]) and np.array_equal(g2[k], g3[k]), k


@pytest.mark.parametrize("ties", TIES)
def test_estimator_score_tests_on_a_device_matrix_agree_with_the_numpy_route(gpu, ties):
    n, p, k = 400, 60, 4
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p))
    truth = np.zeros(p)
    truth[rng.choice(p, k, replace=False)] = np.array([1.0, -1.0, 0.8, -0.8])
    time = np.ceil(rng.exponential(np.exp(-X @ truth)) * 40) / 8.0  # (a grid: ties)
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    y = np.column_stack([time, status])
    w = rng.integers(1, 17, n) / 8.0
    est = linear.PdasCox(sequence=[2])  # two of the four true columns: the other two are left out
    Xd = _dev(X)
    est.fit(Xd, y)
    cols = np.nonzero(est.beta)[0]
    b = est.beta[cols]
    dev = est.score_tests_survival(Xd, _dev(y), weight=_dev(w), ties=ties)
    host = est.score_tests_survival(X, y, weight=w, ties=ties)
    assert np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    assert np.array_equal(dev["in_model"], host["in_model"]) and np.array_equal(dev["columns"], np.arange(p))
    info_d = gpu.cox_information_device(Xd, cols, b, time, status, weight=w, ties=ties)["info"]
    info_h = linear.bess_base._cox_information_host(X[:, cols], b, time, status, w, ties)["info"]
    J = int(status.sum())
    sts = []
    for info, depths, tb in ((info_d, coxaddscoreref.device_depths(gpu, n, cols.size, J, p), dev),
                             (info_h, coxaddscoreref.host_depths(n), host)):
        R, pd = gpu.info_factor(info)
        assert pd
        ref = coxaddscoreref.cox_addscore_reference(X, cols, b, time, status, w, ties, R, None, depths)
        st = coxaddscoreref.statistic_reference(ref)
        coxaddscoreref.check_table(tb, st, "estimator " + ties)
        sts.append(st)
    ok = sts[0]["ok"]
    width = (sts[0]["hi"] - sts[0]["lo"]) + (sts[1]["hi"] - sts[1]["lo"]) + np.abs(sts[0]["stat"] - sts[1]["stat"])
    assert (np.abs(dev["statistic"] - host["statistic"]).astype(LD)[ok] <= width[ok]).all()
    left_out = np.setdiff1d(np.nonzero(truth)[0], cols)
    assert left_out.size >= 1 and int(np.nanargmin(dev["p_value"])) in left_out
    sub = est.score_tests_survival(Xd, y, weight=w, ties=ties, candidates=left_out)
    assert np.array_equal(sub["columns"], left_out)
    assert np.allclose(sub["statistic"], dev["statistic"][left_out], rtol=1e-9)  # (another split: not the same bits)
