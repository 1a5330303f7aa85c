"""Expected information and score on an X already in GPU memory (bessx_info_device, bess_amd/csrc/bessx_k_info.hip)
against NumPy in np.longdouble on the host copy of the same values, within the bounds derived in tests/inforef.py (the
addition depth is that of the row split the library reports).  Shapes: one row, a partial slab, just past a slab and a
16-byte boundary; m + 1 = 15, 16, 17 around one matrix-core tile, 32 = two tiles, 201 = thirteen with a ragged last one,
1024 the largest, 1025 refused.  Layouts are those of tests/test_eval_gpu.py, every element outside the view a NaN.
Weights are multiples of 1/8 with zeros, so their sum is exact.  Two routes that are each within their bound of the
reference agree within twice the bound."""
import numpy as np
import pytest

import inforef
from bess_amd import linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
LINKS = ["identity", "logistic", "poisson"]
P = 600
NS, MS = (1, 127, 4097), (0, 1, 14, 15, 16, 31, 200)


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
    """One model per (dtype, n, m), the same logical values under every layout: a linear predictor with a standard
    deviation of about 1, the responses of the three families and weights with zeros among them."""
    key = (dt, n, m, p)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + (7 if dt == "f32" else 0))
        vals = _vals(dt, n, p)
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        c = 0.3
        eta = vals[:, cols].astype(np.float64) @ beta + c
        ys = {"identity": eta + rng.standard_normal(n),
              "logistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float),
              "poisson": rng.poisson(np.exp(np.clip(eta, -5, 3))).astype(float)}
        w = rng.integers(0, 17, n) / 8.0
        _PROBLEMS[key] = dict(vals=vals, cols=cols, beta=beta, c=c, ys=ys, w=w)
    return _PROBLEMS[key]


def _ref(gpu, dt, n, m, link, y32, weighted, p=P):
    """inforef.information_reference at the device's addition depth, once per distinct set of values"""
    key = (dt, n, m, link, y32, weighted, p)
    if key not in _REFS:
        pr = _problem(dt, n, m, p)
        y = pr["ys"][link].astype(np.float32) if y32 else pr["ys"][link]
        _REFS[key] = inforef.information_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], y,
                                                   pr["w"] if weighted else None, link, inforef.device_depth(gpu, n, m))
    return _REFS[key]


def _forms(pr, link, fi, wi):
    """y and weight as passed: host array, float64 device array, strided device view, float32 device array; wi = 0 is
    no weight.  Returns (y, weight, y is float32)."""
    y, w = pr["ys"][link], pr["w"]
    ys = [y, _dev(y), _dev(np.column_stack([y, y]))[:, 1], _dev(y.astype(np.float32))]
    ws = [None, w, _dev(w), _dev(np.column_stack([w, w, w]))[:, 2], _dev(w.astype(np.float32))]
    return ys[fi], ws[wi], fi == 3


def _check(gpu, t, pr, link, y, w, ref, what):
    got = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w)
    M = pr["cols"].size + 1
    assert got["info"].shape == (M, M) and got["score"].shape == (M,)
    inforef.check_information(got, ref, what)
    assert np.array_equal(got["info"], got["info"].T), what
    assert abs(LD(got["info"][0, 0]) - ref["sum_v"]) <= ref["info_bound"][0, 0], what
    L = ref["loss"]
    assert abs(LD(got["loss"]) - L["loss"][0]) <= L["bound"][0], what
    assert got["sum_w"] == float(L["sum_w"]), what
    ev = gpu.evaluate_device(t, pr["cols"], pr["beta"], [pr["c"]], y, link=link, weight=w)
    assert got["loss"] == ev["loss"][0] and got["sum_w"] == ev["sum_w"], what  # the same bits
    return got


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_information_score_and_loss_are_within_the_bounds(gpu, dt, layout, n):
    base, view = _embed(layout, _vals(dt, n))
    t = view(_dev(base))
    assert tuple(t.shape) == (n, P)
    ni = NS.index(n)
    for mi, m in enumerate(MS):
        pr = _problem(dt, n, m)
        for li, link in enumerate(LINKS):
            fi, wi = (mi + li) % 4, (mi + 2 * li + ni) % 5
            y, w, y32 = _forms(pr, link, fi, wi)
            ref = _ref(gpu, dt, n, m, link, y32, wi > 0)
            _check(gpu, t, pr, link, y, w, ref, "%s %s n=%d m=%d %s y%d w%d" % (dt, layout, n, m, link, fi, wi))


@pytest.mark.parametrize("layout", ["C", "F"])
def test_the_largest_support_and_one_past_it(gpu, layout):
    n, p, m = 127, 1100, 1023
    pr = _problem("f64", n, m, p)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    ref = _ref(gpu, "f64", n, m, "logistic", False, True, p)
    _check(gpu, t, pr, "logistic", pr["ys"]["logistic"], pr["w"], ref, "m + 1 = 1024 " + layout)
    with pytest.raises(gpu.BessxError) as e:
        gpu.information_device(t, np.arange(1024), np.zeros(1024), 0.0, pr["ys"]["logistic"], link="logistic")
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)


@pytest.mark.parametrize("layout", ["C", "F", "two_strides"])
def test_same_call_same_bits_also_on_a_second_stream(gpu, layout):
    n, m = 4097, 200
    pr = _problem("f64", n, m)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    y, w = _dev(pr["ys"]["poisson"]), _dev(pr["w"])
    torch.cuda.synchronize()
    a = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w)
    b = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w, stream=s.cuda_stream)
    for other in (b, c):
        assert np.array_equal(a["info"], other["info"]) and np.array_equal(a["score"], other["score"])
        assert a["loss"] == other["loss"] and a["sum_w"] == other["sum_w"]


@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_nan_inside_the_support_reaches_what_the_definitions_say(gpu, dt, layout):
    """A NaN at x(i, cols[k]) is entry j = k + 1 of z_i and makes eta_i NaN (a zero coefficient is multiplied like any
    other).  From the definitions: identity, v_i = w_i stays finite, so info is NaN exactly in row j and column j
    (v_i z_ij z_il for every l) and finite elsewhere -- info[0, 0] = sum v_i included -- while g_i = w_i (y_i - eta_i) is
    NaN and with it every entry of score; logistic and Poisson, v_i is NaN as well, so every entry of info and score is
    NaN.  A weight of 0 in that row changes nothing: 0 * NaN is NaN.  The loss is NaN in every case."""
    n, m, i, k = 127, 31, 77, 9
    pr = _problem(dt, n, m)
    vals = pr["vals"].copy()
    vals[i, pr["cols"][k]] = np.nan
    base, view = _embed(layout, vals)
    t = view(_dev(base))
    w = pr["w"].copy()
    for wi in (1.0, 0.0):
        w[i] = wi
        for link in LINKS:
            got = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], pr["ys"][link], link=link, weight=w)
            want = np.zeros((m + 1, m + 1), dtype=bool)
            if link == "identity":
                want[k + 1, :] = want[:, k + 1] = True
            else:
                want[:] = True
            assert np.array_equal(np.isnan(got["info"]), want), (link, wi)
            assert np.isnan(got["score"]).all() and np.isnan(got["loss"]), (link, wi)
            assert got["sum_w"] == float(w.sum())
    # ... and a NaN in a column OUTSIDE the support, or in a row past n, is never read
    vals = pr["vals"].copy()
    outside = np.setdiff1d(np.arange(P), pr["cols"])
    vals[:, outside] = np.nan
    base, view = _embed(layout, vals)
    got = gpu.information_device(view(_dev(base)), pr["cols"], pr["beta"], pr["c"], pr["ys"]["logistic"], link="logistic")
    ref = _ref(gpu, dt, n, m, "logistic", False, False)
    inforef.check_information(got, ref, "NaN outside the support")


@pytest.mark.parametrize("name", ["PdasLm", "PdasLogistic", "PdasPoisson"])
def test_estimator_inference_on_a_device_matrix_agrees_with_the_numpy_route(gpu, name):
    n, p, k = 400, 60, 4
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p))
    truth = np.zeros(p)
    truth[rng.choice(p, k, replace=False)] = np.array([1.0, -1.0, 0.8, -0.8])
    eta = X @ truth + 0.2
    y = {"PdasLm": eta + rng.standard_normal(n), "PdasLogistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))) * 1.0,
         "PdasPoisson": rng.poisson(np.exp(eta)) * 1.0}[name]
    est = getattr(linear, name)(sequence=list(range(1, 7)))
    Xd = _dev(X)
    est.fit(Xd, y)
    dev, host = est.inference(Xd, _dev(y)), est.inference(X, y)
    link = est._LINK[est.model_type_int]
    cols = np.nonzero(est.beta)[0]
    assert np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    ref = inforef.information_reference(X, cols, est.beta[cols], float(np.ravel(est.coef0)[0]), y, None, link,
                                        max(n, inforef.device_depth(gpu, n, cols.size)))
    se, cov, rel, cond = inforef.se_reference(ref)
    print("%s: %d columns, cond(S*) %.3e, se bound %.3e, device - host %.3e" % (
        name, cols.size, cond, float(rel), float(np.abs(dev["se"] - host["se"]).max())))
    assert rel < 1e-3 and dev["positive_definite"] and host["positive_definite"]
    for tb in (dev, host):
        assert (np.abs(tb["se"].astype(LD) - se) <= rel * se).all()
    assert (np.abs(dev["se"] - host["se"]).astype(LD) <= 2 * rel * se).all()
    assert np.array_equal(dev["coef"], host["coef"]) and dev["dof"] == host["dof"] == n - cols.size - 1


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    t = _dev(pr["vals"])
    y, w = pr["ys"]["logistic"], _dev(pr["w"])

    def call():
        gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link="logistic", weight=w)
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
