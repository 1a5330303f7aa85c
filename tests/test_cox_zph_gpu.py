"""The proportional-hazards test of a Cox model on an X already in GPU memory (bessx_cox_zph_device,
bess_amd/csrc/bessx_k_coxzph.hip) against NumPy in np.longdouble on the host copy of the same values, within the bounds
derived in tests/coxzphref.py (the addition depths are those of the row splits the library reports).  Shapes, layouts and
the generator are those of tests/test_cox_info_gpu.py: n = 1, 2, 1023, 1025 around the 1024-position scan block and 4097;
m + 1 = 2, 15, 16, 17 around one matrix-core tile, 32, 151, 1024 the largest, 1025 refused; every element outside the view
a NaN.  gt comes from capi.zph_transform; the transform, ties, weight and host / device vectors cycle across the cases."""
import ctypes

import numpy as np
import pytest

import coxzphref
from bess_amd import linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
TIES = ["order", "breslow"]
TRANSFORMS = ["km", "rank", "identity", np.log1p]  # (times start at 0: "log" itself is covered in test_cox_zph_api.py)
P = 400
NS, MS = (1, 2, 1023, 1025, 4097), (1, 14, 15, 16, 31, 150)
OUT = ("info0", "info1", "info2", "score0", "score1")


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


_VALS, _PROBLEMS, _REFS = {}, {}, {}


def _vals(dt, n, p=P):
    if (dt, n, p) not in _VALS:
        _VALS[(dt, n, p)] = np.random.default_rng(n + (1 if dt == "f32" else 0)).standard_normal((n, p)).astype(DT[dt])
    return _VALS[(dt, n, p)]


def _problem(dt, n, m, p=P):
    """test_cox_info_gpu's generator: beta ~ N(0, 1 / m), times on a grid of 2.5 n points (about a third of the rows share
    one), about 70 % events, weights in eighths with zeros."""
    key = (dt, n, m, p)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + (7 if dt == "f32" else 0))
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        time = rng.integers(0, int(2.5 * n) + 1, n) / 8.0
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0
        _PROBLEMS[key] = dict(vals=_vals(dt, n, p), cols=cols, beta=beta, time=time, status=status, w=w)
    return _PROBLEMS[key]


def _reference(gpu, vals, cols, beta, time, status, w, gt, ties):
    n, J = vals.shape[0], int(np.count_nonzero(status))
    return coxzphref.cox_zph_reference(vals, cols, beta, time, status, w, gt, ties,
                                       coxzphref.device_depths(gpu, n, len(cols), J))


def _case(gpu, dt, n, m, ties, weighted, ti, p=P):
    """(gt, centre, reference at the device's addition depths), once per distinct set of values"""
    key = (dt, n, m, ties, weighted, ti, p)
    if key not in _REFS:
        pr = _problem(dt, n, m, p)
        w = pr["w"] if weighted else None
        gt, centre = gpu.zph_transform(pr["time"], pr["status"], w, TRANSFORMS[ti])
        _REFS[key] = (gt, centre, _reference(gpu, pr["vals"], pr["cols"], pr["beta"], pr["time"], pr["status"], w, gt, ties))
    return _REFS[key]


def _forms(pr, gt, form, wi):
    """time, status, gt and weight as passed: host arrays (form 0) or device arrays (form 1: float64, a strided view,
    float32 for the status, which is exact); wi = 0 is no weight, 1 a host and 2 a device array."""
    t, s, g, w = pr["time"], pr["status"], gt, pr["w"]
    if form:
        t, s, g = _dev(np.column_stack([t, t]))[:, 1], _dev(s.astype(np.float32)), _dev(g)
    return t, s, g, [None, w, _dev(w)][wi]


def _same_as_information(gpu, got, t, pr, time, status, w, ties, what):
    info = gpu.cox_information_device(t, pr["cols"], pr["beta"], time, status, weight=w, ties=ties)
    assert np.array_equal(got["info0"], info["info"]) and np.array_equal(got["score0"], info["score"]), what
    assert got["loglik"] == info["loglik"] and got["n_events"] == info["n_events"], what  # the same bits


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_all_outputs_are_within_the_bounds_and_the_table_follows(gpu, dt, layout, n):
    base, view = _embed(layout, _vals(dt, n))
    t = view(_dev(base))
    assert tuple(t.shape) == (n, P)
    ni, li = NS.index(n), LAYOUTS.index(layout)
    for mi, m in enumerate(MS):
        pr = _problem(dt, n, m)
        ties, wi, form, ti = TIES[(mi + ni) % 2], (mi + 2 * ni) % 3, (mi + li) % 2, (mi + ni + li) % 4
        gt, centre, ref = _case(gpu, dt, n, m, ties, wi > 0, ti)
        time, status, g, w = _forms(pr, gt, form, wi)
        what = "%s %s n=%d m=%d %s w%d form%d transform%d" % (dt, layout, n, m, ties, wi, form, ti)
        got = gpu.cox_zph_device(t, pr["cols"], pr["beta"], time, status, g, weight=w, ties=ties)
        coxzphref.check_cox_zph(got, ref, what)
        _same_as_information(gpu, got, t, pr, time, status, w, ties, what)
        tab = gpu.cox_zph_table(got, centre)
        if n >= 1023:
            coxzphref.check_table(tab, coxzphref.table_reference(ref), what)
            assert tab["global_df"] == m and 0.0 <= tab["global_p_value"] <= 1.0
        else:  # one or two rows: D is zero or indefinite, the table says so and raises nothing
            assert not tab["positive_definite"] and np.isnan(tab["chisq"]).all() and np.isnan(tab["global_chisq"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_transform_of_one_repeats_the_information_bit_for_bit(gpu, dt, layout):
    n = 1025
    base, view = _embed(layout, _vals(dt, n))
    t = view(_dev(base))
    for mi, m in enumerate(MS):
        pr = _problem(dt, n, m)
        ties, w = TIES[mi % 2], (pr["w"] if mi % 3 else None)
        gt = np.where(pr["status"] != 0, 1.0, np.nan)  # (not read where status is 0)
        got = gpu.cox_zph_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], gt, weight=w, ties=ties)
        what = "%s %s m=%d" % (dt, layout, m)
        _same_as_information(gpu, got, t, pr, pr["time"], pr["status"], w, ties, what)
        assert np.array_equal(got["info1"], got["info0"]) and np.array_equal(got["info2"], got["info0"]), what
        assert np.array_equal(got["score1"], got["score0"]), what


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("layout", ["C", "F"])
def test_special_time_and_status_patterns(gpu, layout, ties):
    """Every time tied (one risk set under "breslow"; every event shares one g, so gt is 0 after centring, info1, info2
    and score1 are exact zeros and the table is the degenerate one); no ties at all; one event (at the last position:
    its risk set is itself); every event at one time among censored rows elsewhere; no event (exact zeros)."""
    n, m = 1025, 31
    pr = _problem("f64", n, m)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    rng = np.random.default_rng(9)
    perm = rng.permutation(n).astype(np.float64)
    last = np.zeros(n)
    last[int(np.argmax(perm))] = 1.0
    mid = (perm == 500.0).astype(np.float64)
    one_time = np.where(pr["status"] != 0, 500.0, perm)
    for name, time, status in (("all tied", np.full(n, 3.0), pr["status"]), ("no ties", perm, pr["status"]),
                               ("event at the last position", perm, last), ("one event", perm, mid),
                               ("every event at one time", one_time, pr["status"])):
        gt, centre = gpu.zph_transform(time, status, pr["w"], "identity")
        ref = _reference(gpu, pr["vals"], pr["cols"], pr["beta"], time, status, pr["w"], gt, ties)
        got = gpu.cox_zph_device(t, pr["cols"], pr["beta"], time, status, gt, weight=pr["w"], ties=ties)
        what = "%s %s %s" % (name, layout, ties)
        coxzphref.check_cox_zph(got, ref, what)
        _same_as_information(gpu, got, t, pr, time, status, pr["w"], ties, what)
        tab = gpu.cox_zph_table(got, centre)
        if name != "no ties":  # every event shares one g
            assert not got["info1"].any() and not got["info2"].any() and not got["score1"].any(), what
            assert not tab["positive_definite"] and np.isnan(tab["chisq"]).all(), what
        else:
            coxzphref.check_table(tab, coxzphref.table_reference(ref), what)
    got = gpu.cox_zph_device(t, pr["cols"], pr["beta"], pr["time"], np.zeros(n), np.full(n, np.nan), weight=pr["w"],
                             ties=ties)
    for k in OUT:
        assert got[k].shape == ((m, m) if k.startswith("info") else (m,)) and not got[k].any(), k
    assert got["loglik"] == 0.0 and got["n_events"] == 0.0
    tab = gpu.cox_zph_table(got)
    assert not tab["positive_definite"] and np.isnan(tab["global_chisq"]) and np.isnan(tab["p_value"]).all()


def test_the_empty_model_the_largest_support_and_one_past_it(gpu):
    n, p, m = 1025, 1100, 1023
    pr = _problem("f64", n, m, p)
    t = _dev(pr["vals"])
    gt, centre, ref = _case(gpu, "f64", n, m, "breslow", True, 0, p)
    got = gpu.cox_zph_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], gt, weight=pr["w"], ties="breslow")
    coxzphref.check_cox_zph(got, ref, "m + 1 = 1024")
    _same_as_information(gpu, got, t, pr, pr["time"], pr["status"], pr["w"], "breslow", "m + 1 = 1024")
    with pytest.raises(gpu.BessxError) as e:
        gpu.cox_zph_device(t, np.arange(1024), np.zeros(1024), pr["time"], pr["status"], gt)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    # m = 0 reads nothing of x: every element of the matrix may be a NaN
    nan = _dev(np.full((n, 5), np.nan))
    got = gpu.cox_zph_device(nan, [], [], pr["time"], pr["status"], gt, weight=pr["w"])
    null = gpu.evaluate_cox_device(nan, [], np.zeros((0, 1)), pr["time"], pr["status"], weight=pr["w"], concordance=False)
    assert all(got[k].shape == ((0, 0) if k.startswith("info") else (0,)) for k in OUT)
    assert got["loglik"] == null["loglik"][0] and np.isfinite(got["loglik"])
    assert got["n_events"] == float(np.sum(pr["w"] * pr["status"]))
    tab = gpu.cox_zph_table(got, centre)
    assert tab["chisq"].shape == (0,) and tab["global_df"] == 0 and tab["positive_definite"]


@pytest.mark.parametrize("layout", ["C", "F", "two_strides"])
def test_same_call_same_bits_also_on_a_second_stream(gpu, layout):
    n, m = 4097, 150
    pr = _problem("f64", n, m)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    gt = gpu.zph_transform(pr["time"], pr["status"], pr["w"], "km")[0]
    torch.cuda.synchronize()
    args = (t, pr["cols"], pr["beta"], pr["time"], pr["status"], gt)
    a = gpu.cox_zph_device(*args, weight=pr["w"], ties="breslow")
    b = gpu.cox_zph_device(*args, weight=pr["w"], ties="breslow")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = gpu.cox_zph_device(*args, weight=pr["w"], ties="breslow", stream=s.cuda_stream)
    for other in (b, c):
        assert all(np.array_equal(a[k], other[k]) for k in OUT)
        assert a["loglik"] == other["loglik"]


@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_nan_inside_the_support_propagates_and_one_outside_does_not(gpu, dt, layout):
    """The construction of test_cox_info_gpu: the row with the largest time holds a NaN in a support column and the
    smallest time is an event of weight 1, so every S0 and with it every h^q, v^q and a^q is NaN."""
    n, m, c = 1023, 31, 9
    pr = _problem(dt, n, m)
    time = np.random.default_rng(4).permutation(n).astype(np.float64)
    i = int(np.argmax(time))
    status, w = pr["status"].copy(), pr["w"].copy()
    status[int(np.argmin(time))], w[int(np.argmin(time))] = 1.0, 1.0
    gt = gpu.zph_transform(time, status, w, "rank")[0]
    vals = pr["vals"].copy()
    vals[i, pr["cols"][c]] = np.nan
    base, view = _embed(layout, vals)
    t = view(_dev(base))
    for ties in TIES:
        got = gpu.cox_zph_device(t, pr["cols"], pr["beta"], time, status, gt, weight=w, ties=ties)
        assert all(np.isnan(got[k]).all() for k in OUT), ties
        assert np.isnan(got["loglik"]) and got["n_events"] == float(np.sum(w * status))
        assert not gpu.cox_zph_table(got)["positive_definite"]
    # ... and a NaN in a column OUTSIDE the support, or in the padding of the layout, is never read
    vals = pr["vals"].copy()
    vals[:, np.setdiff1d(np.arange(P), pr["cols"])] = np.nan
    base, view = _embed(layout, vals)
    got = gpu.cox_zph_device(view(_dev(base)), pr["cols"], pr["beta"], time, status, gt, weight=w)
    ref = _reference(gpu, pr["vals"], pr["cols"], pr["beta"], time, status, w, gt, "order")
    coxzphref.check_cox_zph(got, ref, "NaN outside the support")


def test_outputs_in_device_memory_with_a_padded_leading_dimension(gpu):
    """The C entry with out_on_device = 1 and info_ld > m: the same bits as the host route, the padding untouched."""
    n, m, ld = 1025, 31, 40
    pr = _problem("f64", n, m)
    t = _dev(pr["vals"])
    gt = gpu.zph_transform(pr["time"], pr["status"], pr["w"], "km")[0]
    want = gpu.cox_zph_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], gt, weight=pr["w"], ties="breslow")
    out = {k: torch.full((m, ld) if k.startswith("info") else (m,), -7.0, dtype=torch.float64, device="cuda") for k in OUT}
    torch.cuda.synchronize()
    a = gpu.CoxZphInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = t.data_ptr(), 0, P, 1, n, P
    a.cols, a.m, a.beta = gpu._ip(pr["cols"]), m, gpu._dp(pr["beta"])
    a.time, a.status, a.weight, a.ties = gpu._dp(pr["time"]), gpu._dp(pr["status"]), gpu._dp(pr["w"]), 1
    a.gt, a.info_ld, a.out_on_device = gpu._dp(gt), ld, 1
    for k in OUT:
        setattr(a, k, out[k].data_ptr())
    ll, ne = ctypes.c_double(0), ctypes.c_double(0)
    rc = gpu.lib().bessx_cox_zph_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne))
    assert rc == 0, gpu.last_error()
    for k in OUT:
        got = out[k].cpu().numpy()
        if k.startswith("info"):
            assert np.array_equal(got[:, :m], want[k]) and (got[:, m:] == -7.0).all(), k
        else:
            assert np.array_equal(got, want[k]), k
    assert (ll.value, ne.value) == (want["loglik"], want["n_events"])
    host = np.zeros(m)
    a.score1 = host.ctypes.data
    assert gpu.lib().bessx_cox_zph_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne)) == 1
    assert "score1" in gpu.last_error()


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    t = _dev(pr["vals"])
    w = _dev(pr["w"])
    gt = gpu.zph_transform(pr["time"], pr["status"], pr["w"], "km")[0]

    def call():
        gpu.cox_zph_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], gt, weight=w, ties="breslow")
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
    assert first["allocation_requests"] - before["allocation_requests"] == added


@pytest.mark.parametrize("ties", TIES)
def test_estimator_on_a_device_matrix_agrees_with_the_numpy_route(gpu, ties):
    n, p, k = 600, 60, 4
    rng = np.random.default_rng(23)
    X = rng.standard_normal((n, p))
    truth = np.zeros(p)
    truth[rng.choice(p, k, replace=False)] = np.array([1.0, -1.0, 0.8, -0.8])
    time = np.ceil(rng.exponential(np.exp(-X @ truth)) * 40) / 8.0  # (a grid: ties)
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    y = np.column_stack([time, status])
    est = linear.PdasCox(sequence=list(range(1, 7)))
    Xd = _dev(X)
    est.fit(Xd, y)
    dev = est.proportional_hazards_test(Xd, _dev(y), ties=ties, residuals=True)
    host = est.proportional_hazards_test(X, y, ties=ties, residuals=True)
    cols = np.nonzero(est.beta)[0]
    m, J = cols.size, int(status.sum())
    assert m >= 1 and np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    assert dev["transform"] == host["transform"] == "km" and dev["gt_centre"] == host["gt_centre"]
    gt, centre = gpu.zph_transform(time, status, None, "km")
    assert centre == dev["gt_centre"]
    # one layer down, where the matrices are returned: each route is within its own bound of the reference
    ref_dev = _reference(gpu, X, cols, est.beta[cols], time, status, None, gt, ties)
    ref_host = coxzphref.cox_zph_reference(X, cols, est.beta[cols], time, status, None, gt, ties,
                                           coxzphref.host_depths(n, J))
    got_dev = gpu.cox_zph_device(Xd, cols, est.beta[cols], time, status, gt, ties=ties)
    got_host = linear.bess_base._cox_zph_host(X[:, cols], est.beta[cols], time, status, np.ones(n), gt, ties)
    coxzphref.check_cox_zph(got_dev, ref_dev, "device " + ties)
    coxzphref.check_cox_zph(got_host, ref_host, "numpy " + ties)
    assert np.array_equal(dev["score1"], got_dev["score1"]) and np.array_equal(host["score1"], got_host["score1"])
    assert dev["loglik"] == got_dev["loglik"]
    # the statistics: each route within its own bound of the reference, so the two agree within the sum of both
    td, th = coxzphref.table_reference(ref_dev), coxzphref.table_reference(ref_host)
    coxzphref.check_table(dev, td, "device table " + ties)
    coxzphref.check_table(host, th, "numpy table " + ties)
    assert (np.abs(dev["chisq"] - host["chisq"]).astype(LD) <= td["chisq_bound"] + th["chisq_bound"]).all()
    assert abs(LD(dev["global_chisq"]) - LD(host["global_chisq"])) <= td["global_bound"] + th["global_bound"]
    assert dev["global_df"] == host["global_df"] == m
    # the points of the plot: the Schoenfeld residuals times inverse(info0) n_events, plus beta
    ss = dev["scaled_schoenfeld"]
    assert gpu.is_device_array(ss) and tuple(ss.shape) == (J, m) and host["scaled_schoenfeld"].shape == (J, m)
    assert np.array_equal(dev["time"], host["time"]) and np.array_equal(dev["time"], np.sort(time[status != 0]))
    r = gpu.cox_diagnostics_device(Xd, cols, est.beta[cols], time, status, ties=ties, kinds=("schoenfeld",))["schoenfeld"]
    C = np.linalg.inv(got_dev["info0"]) * got_dev["n_events"]
    want = r.cpu().numpy() @ C + est.beta[cols]
    scale = np.abs(r.cpu().numpy()) @ np.abs(C) + np.abs(est.beta[cols])
    assert (np.abs(ss.cpu().numpy() - want) <= 1e-10 * scale).all()
    assert (np.abs(ss.cpu().numpy() - host["scaled_schoenfeld"]) <= 1e-8 * scale).all()
