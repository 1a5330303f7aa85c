"""Observed information and score of a Cox model on an X already in GPU memory (bessx_cox_info_device,
bess_amd/csrc/bessx_k_coxinfo.hip) against NumPy in np.longdouble on the host copy of the same values, within the bounds
derived in tests/coxinforef.py (the addition depths are those of the row splits the library reports).  Shapes: n = 1, 2,
1023, 1025 around the 1024-position scan block and 4097 for a carry over several blocks; m + 1 = 2, 15, 16, 17 around one
matrix-core tile, 32 = two tiles, 151 = ten with a ragged last one, 1024 the largest, 1025 refused.  Layouts are those of
tests/test_info_gpu.py, every element outside the view a NaN.  About a third of the rows share a time, about 70 % are
events, weights are multiples of 1/8 with zeros, so their sum is exact.  ties, weight and host / device vectors cycle
across the cases."""
import numpy as np
import pytest

import coxinforef
from bess_amd import linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
TIES = ["order", "breslow"]
P = 400
NS, MS = (1, 2, 1023, 1025, 4097), (1, 14, 15, 16, 31, 150)


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
    """One model per (dtype, n, m), the same logical values under every layout: beta ~ N(0, 1 / m), times on a grid of
    2.5 n points (about a third of the rows share one), about 70 % events, weights in eighths with zeros."""
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


def _reference(gpu, vals, cols, beta, time, status, w, ties):
    n, J = vals.shape[0], int(np.count_nonzero(status))
    return coxinforef.cox_information_reference(vals, cols, beta, time, status, w, ties,
                                                coxinforef.device_depths(gpu, n, len(cols), J))


def _ref(gpu, dt, n, m, ties, weighted, p=P):
    """coxinforef.cox_information_reference at the device's addition depths, once per distinct set of values"""
    key = (dt, n, m, ties, weighted, p)
    if key not in _REFS:
        pr = _problem(dt, n, m, p)
        _REFS[key] = _reference(gpu, pr["vals"], pr["cols"], pr["beta"], pr["time"], pr["status"],
                                pr["w"] if weighted else None, ties)
    return _REFS[key]


def _forms(pr, form, wi):
    """time, status and weight as passed: host arrays (form 0) or device arrays (form 1: float64, a strided view, float32
    for the status, which is exact); wi = 0 is no weight, 1 a host and 2 a device array."""
    t, s, w = pr["time"], pr["status"], pr["w"]
    if form:
        t, s = _dev(np.column_stack([t, t]))[:, 1], _dev(s.astype(np.float32))
    return t, s, [None, w, _dev(w)][wi]


def _check(gpu, t, pr, time, status, w, ties, ref, what):
    got = gpu.cox_information_device(t, pr["cols"], pr["beta"], time, status, weight=w, ties=ties)
    coxinforef.check_cox_information(got, ref, what)
    assert np.array_equal(got["info"], got["info"].T), what
    ev = gpu.evaluate_cox_device(t, pr["cols"], pr["beta"], time, status, weight=w, ties=ties, concordance=False)
    assert got["loglik"] == ev["loglik"][0], what  # the same bits
    return got


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_information_score_and_loglik_are_within_the_bounds(gpu, dt, layout, n):
    base, view = _embed(layout, _vals(dt, n))
    t = view(_dev(base))
    assert tuple(t.shape) == (n, P)
    ni, li = NS.index(n), LAYOUTS.index(layout)
    for mi, m in enumerate(MS):
        pr = _problem(dt, n, m)
        ties, wi, form = TIES[(mi + ni) % 2], (mi + 2 * ni) % 3, (mi + li) % 2
        time, status, w = _forms(pr, form, wi)
        ref = _ref(gpu, dt, n, m, ties, wi > 0)
        _check(gpu, t, pr, time, status, w, ties, ref, "%s %s n=%d m=%d %s w%d form%d" % (dt, layout, n, m, ties, wi, form))


@pytest.mark.parametrize("ties", TIES)
@pytest.mark.parametrize("layout", ["C", "F"])
def test_special_time_and_status_patterns(gpu, layout, ties):
    """Every time tied (one risk set under "breslow": one thread per column writes all of U); no ties at all, in an order
    that is not the rows'; no event (info and score are exact zeros: v = e * 0 and no sweep over U); an event only at the
    last position (its risk set is itself: u = x, G1 and G2 cancel up to the bound)."""
    n, m = 1025, 31
    pr = _problem("f64", n, m)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    rng = np.random.default_rng(9)
    perm = rng.permutation(n).astype(np.float64)
    last = np.zeros(n)
    last[int(np.argmax(perm))] = 1.0
    for name, time, status in (("all tied", np.full(n, 3.0), pr["status"]), ("no ties", perm, pr["status"]),
                               ("event at the last position", perm, last)):
        ref = _reference(gpu, pr["vals"], pr["cols"], pr["beta"], time, status, pr["w"], ties)
        _check(gpu, t, pr, time, status, pr["w"], ties, ref, "%s %s %s" % (name, layout, ties))
    got = gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], np.zeros(n), weight=pr["w"], ties=ties)
    assert got["info"].shape == (m, m) and not got["info"].any() and not got["score"].any()
    assert got["loglik"] == 0.0 and got["n_events"] == 0.0 and got["residual_sum"] == 0.0


@pytest.mark.parametrize("layout", ["C", "F"])
def test_the_empty_model_the_largest_support_and_one_past_it(gpu, layout):
    n, p, m = 127, 1100, 1023
    pr = _problem("f64", n, m, p)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    ref = _ref(gpu, "f64", n, m, "breslow", True, p)
    _check(gpu, t, pr, pr["time"], pr["status"], pr["w"], "breslow", ref, "m + 1 = 1024 " + layout)
    with pytest.raises(gpu.BessxError) as e:
        gpu.cox_information_device(t, np.arange(1024), np.zeros(1024), pr["time"], pr["status"])
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    # m = 0 reads nothing of x: every element of the matrix may be a NaN
    nan = _dev(np.full((n, 5), np.nan))
    got = gpu.cox_information_device(nan, [], [], pr["time"], pr["status"], weight=pr["w"])
    null = gpu.evaluate_cox_device(nan, [], np.zeros((0, 1)), pr["time"], pr["status"], weight=pr["w"], concordance=False)
    assert got["info"].shape == (0, 0) and got["score"].shape == (0,) and got["residual_sum"] == 0.0
    assert got["loglik"] == null["loglik"][0] and np.isfinite(got["loglik"])
    assert got["n_events"] == float(np.sum(pr["w"] * pr["status"]))


@pytest.mark.parametrize("layout", ["C", "F", "two_strides"])
def test_same_call_same_bits_also_on_a_second_stream(gpu, layout):
    n, m = 4097, 150
    pr = _problem("f64", n, m)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    torch.cuda.synchronize()
    args = (t, pr["cols"], pr["beta"], pr["time"], pr["status"])
    a = gpu.cox_information_device(*args, weight=pr["w"], ties="breslow")
    b = gpu.cox_information_device(*args, weight=pr["w"], ties="breslow")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = gpu.cox_information_device(*args, weight=pr["w"], ties="breslow", stream=s.cuda_stream)
    for other in (b, c):
        assert np.array_equal(a["info"], other["info"]) and np.array_equal(a["score"], other["score"])
        assert a["loglik"] == other["loglik"] and a["residual_sum"] == other["residual_sum"]


@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_nan_inside_the_support_propagates_and_one_outside_does_not(gpu, dt, layout):
    """A NaN at x(i, cols[c]) makes eta_i and e_i NaN.  Here row i holds the largest time and the smallest time is an
    event of weight 1: e_i is in every risk set, so every S0 is NaN, the hazard is NaN from the first position on, and
    with it every v, every g, loglik, and every entry of info and score -- for either ties."""
    n, m, c = 1023, 31, 9
    pr = _problem(dt, n, m)
    time = np.random.default_rng(4).permutation(n).astype(np.float64)
    i = int(np.argmax(time))
    status, w = pr["status"].copy(), pr["w"].copy()
    status[int(np.argmin(time))], w[int(np.argmin(time))] = 1.0, 1.0
    vals = pr["vals"].copy()
    vals[i, pr["cols"][c]] = np.nan
    base, view = _embed(layout, vals)
    t = view(_dev(base))
    for ties in TIES:
        got = gpu.cox_information_device(t, pr["cols"], pr["beta"], time, status, weight=w, ties=ties)
        assert np.isnan(got["info"]).all() and np.isnan(got["score"]).all(), ties
        assert np.isnan(got["loglik"]) and np.isnan(got["residual_sum"]), ties
        assert got["n_events"] == float(np.sum(w * status))
    # ... and a NaN in a column OUTSIDE the support, or in the padding of the layout, is never read
    vals = pr["vals"].copy()
    vals[:, np.setdiff1d(np.arange(P), pr["cols"])] = np.nan
    base, view = _embed(layout, vals)
    got = gpu.cox_information_device(view(_dev(base)), pr["cols"], pr["beta"], time, status, weight=w)
    ref = _reference(gpu, pr["vals"], pr["cols"], pr["beta"], time, status, w, "order")
    coxinforef.check_cox_information(got, ref, "NaN outside the support")


@pytest.mark.parametrize("ties", TIES)
def test_estimator_inference_on_a_device_matrix_agrees_with_the_numpy_route(gpu, ties):
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
    dev, host = est.inference_survival(Xd, _dev(y), ties=ties), est.inference_survival(X, y, ties=ties)
    cols = np.nonzero(est.beta)[0]
    assert cols.size >= 1 and np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    J = int(status.sum())
    assert J > 4 * cols.size  # (the se bound is asked for where n_events > 4 m)
    # one layer down, where info itself is returned: each route is within its own bound of the reference, so the two
    # agree within the sum of the two bounds
    ref_dev = _reference(gpu, X, cols, est.beta[cols], time, status, None, ties)
    ref_host = coxinforef.cox_information_reference(X, cols, est.beta[cols], time, status, None, ties,
                                                    coxinforef.host_depths(n, J))
    got_dev = gpu.cox_information_device(Xd, cols, est.beta[cols], time, status, ties=ties)
    got_host = linear.bess_base._cox_information_host(X[:, cols], est.beta[cols], time, status, np.ones(n), ties)
    coxinforef.check_cox_information(got_dev, ref_dev, "device " + ties)
    coxinforef.check_cox_information(got_host, ref_host, "numpy " + ties)
    assert (np.abs(got_dev["info"] - got_host["info"]).astype(LD) <= ref_dev["info_bound"] + ref_host["info_bound"]).all()
    assert (np.abs(got_dev["score"] - got_host["score"]).astype(LD)
            <= ref_dev["score_bound"] + ref_host["score_bound"]).all()
    assert np.array_equal(dev["score"], got_dev["score"]) and np.array_equal(host["score"], got_host["score"])
    assert dev["loglik"] == got_dev["loglik"] and dev["residual_sum"] == got_dev["residual_sum"]
    # the standard errors, against the reference with the looser of the two routes' bounds
    ref = ref_dev if float(ref_dev["rel"]) >= float(ref_host["rel"]) else ref_host
    se, cov, rel, cond = coxinforef.se_reference(ref)
    print("%s: %d columns, cond(S*) %.3e, se bound %.3e, device - host %.3e" % (
        ties, cols.size, cond, float(rel), float(np.abs(dev["se"] - host["se"]).max())))
    assert rel < 1e-3 and dev["positive_definite"] and host["positive_definite"]
    for tb, r in ((dev, ref_dev), (host, ref_host)):
        rel_r = coxinforef.se_reference(r)[2]
        assert (np.abs(tb["se"].astype(LD) - se) <= rel_r * se).all()
    assert (np.abs(dev["se"] - host["se"]).astype(LD) <= 2 * rel * se).all()
    assert np.array_equal(dev["coef"], host["coef"]) and dev["dof"] == host["dof"] == J - cols.size
    assert dev["loglik"] == est.evaluate_survival(Xd, y, ties=ties)["loglik"]


def test_info_and_score_in_device_memory_with_a_padded_leading_dimension(gpu):
    """The C entry with out_on_device = 1 and info_ld > m: the same bits as the host route, the padding untouched."""
    import ctypes
    n, m, ld = 1025, 31, 40
    pr = _problem("f64", n, m)
    t = _dev(pr["vals"])
    want = gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=pr["w"], ties="breslow")
    info = torch.full((m, ld), -7.0, dtype=torch.float64, device="cuda")
    score = torch.full((m,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a = gpu.CoxInfoInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = t.data_ptr(), 0, P, 1, n, P
    a.cols, a.m, a.beta = gpu._ip(pr["cols"]), m, gpu._dp(pr["beta"])
    a.time, a.status, a.weight, a.ties = gpu._dp(pr["time"]), gpu._dp(pr["status"]), gpu._dp(pr["w"]), 1
    a.info, a.info_ld, a.score, a.out_on_device = info.data_ptr(), ld, score.data_ptr(), 1
    ll, ne, rs = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    rc = gpu.lib().bessx_cox_info_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs))
    assert rc == 0, gpu.last_error()
    got = info.cpu().numpy()
    assert np.array_equal(got[:, :m], want["info"]) and (got[:, m:] == -7.0).all()
    assert np.array_equal(score.cpu().numpy(), want["score"])
    assert (ll.value, ne.value, rs.value) == (want["loglik"], want["n_events"], want["residual_sum"])
    a.info_ld = m - 1
    assert gpu.lib().bessx_cox_info_device(ctypes.byref(a), ctypes.byref(ll), ctypes.byref(ne), ctypes.byref(rs)) == 1
    assert "info_ld must be at least m" in gpu.last_error()


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    t = _dev(pr["vals"])
    w = _dev(pr["w"])

    def call():
        gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=w, ties="breslow")
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
