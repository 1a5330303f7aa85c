"""Score tests of the excluded columns on an X already in GPU memory (bessx_addscore_device,
bess_amd/csrc/bessx_k_addscore.hip) against NumPy in np.longdouble on the host copy of the same values, within the bounds
derived in tests/addscoreref.py (the addition depths are those of the split the library reports).  Shapes: one row, a
partial slab, just past a slab and a 16-byte boundary; 1, 15, 16, 17 and 600 candidates; a scattered list and the support
itself; m + 2 panel columns around one matrix-core tile (m = 14 fills it, m = 15 starts a second), two tiles, thirteen,
the largest (m + 1 = 1024) and one past it; a candidate block of 64 so that 600 candidates cross blocks.  Layouts are
those of tests/test_info_gpu.py, every element outside the view a NaN.  Weights are multiples of 1/8 with zeros."""
import numpy as np
import pytest

import addscoreref
import inforef
from bess_amd import linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
LINKS = ["identity", "logistic", "poisson"]
P = 600
# (n, p, m, candidates: None = all / "scattered" = 37 of p / "support", candidate_block)
DEV_CASES = [(1, 1, 0, None, 0), (1, 17, 15, None, 0), (127, 15, 14, None, 0), (127, 16, 15, None, 0),
             (127, 17, 16, None, 0), (127, P, 30, None, 0), (127, P, 200, "support", 0), (4097, P, 0, None, 0),
             (4097, P, 14, None, 0), (4097, P, 31, None, 64), (4097, P, 200, "scattered", 0), (4097, P, 16, "support", 0)]
TABLE_SHAPES = [(127, 0), (127, 14), (127, 16), (4097, 15), (4097, 31), (4097, 200), (1000, 200)]


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


_PROBLEMS, _REFS, _TENSORS = {}, {}, {}


def _problem(dt, n, m, p=P, signal=False):
    """One model per (dtype, n, m, p), the same logical values under every layout: a linear predictor with a standard
    deviation of about 1, the responses of the three families, weights with zeros among them and a random well-scaled
    lower-triangular factor.  signal: the responses also depend on one excluded column (`sig`), and one more excluded
    column (`planted`, m >= 1) is the first support column plus 2^-10 noise."""
    key = (dt, n, m, p, signal)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + (7 if dt == "f32" else 0) + (3 if signal else 0))
        vals = np.random.default_rng(n + m + (1 if dt == "f32" else 0)).standard_normal((n, p)).astype(DT[dt])
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        c = 0.3
        sig = planted = None
        extra = 0.0
        if signal:
            free = np.setdiff1d(np.arange(p), cols)
            sig = int(free[len(free) // 2])
            extra = 1.2 * vals[:, sig].astype(np.float64)
            if m >= 1:
                planted = int(free[len(free) // 3])
                vals[:, planted] = vals[:, cols[0]] + DT[dt](2.0 ** -10) * rng.standard_normal(n).astype(DT[dt])
        eta = vals[:, cols].astype(np.float64) @ beta + c
        ys = {"identity": eta + extra + rng.standard_normal(n),
              "logistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-(eta + extra)))).astype(float),
              "poisson": rng.poisson(np.exp(np.clip(eta + extra, -5, 3))).astype(float)}
        w = rng.integers(0, 17, n) / 8.0
        M = m + 1
        R = np.tril(rng.standard_normal((M, M))) / np.sqrt(float(n) * M)
        _PROBLEMS[key] = dict(vals=vals, cols=cols, beta=beta, c=c, ys=ys, w=w, R=R, sig=sig, planted=planted)
    return _PROBLEMS[key]


def _tensor(dt, layout, n, m, p, signal=False):
    key = (dt, layout, n, m, p, signal)
    if key not in _TENSORS:
        if len(_TENSORS) > 24:
            _TENSORS.clear()
        base, view = _embed(layout, _problem(dt, n, m, p, signal)["vals"])
        _TENSORS[key] = view(_dev(base))
    return _TENSORS[key]


def _cand(pr, p, kind):
    if kind is None:
        return None
    if kind == "support":
        return pr["cols"].astype(np.int64)
    return np.sort(np.random.default_rng(p).choice(p, 37, replace=False))


def _forms(pr, link, fi, wi):
    """y and weight as passed: host array, float64 device array, strided device view, float32 device array; wi = 0 is
    no weight.  Returns (y, weight, y as the kernels see it, w as they see it)."""
    y, w = pr["ys"][link], pr["w"]
    ys = [y, _dev(y), _dev(np.column_stack([y, y]))[:, 1], _dev(y.astype(np.float32))]
    ws = [None, w, _dev(w), _dev(np.column_stack([w, w, w]))[:, 2], _dev(w.astype(np.float32))]
    return ys[fi], ws[wi], (y.astype(np.float32) if fi == 3 else y), (None if wi == 0 else w)


def _ref(gpu, dt, case, link, yv, wv, y32, signal=False, R="given"):
    n, p, m, kind, block = case
    key = (dt, case, link, y32, wv is not None, signal, R if isinstance(R, str) else "own")
    if key not in _REFS:
        pr = _problem(dt, n, m, p, signal)
        cand = _cand(pr, p, kind)
        q = p if cand is None else cand.size
        depth, depth_score, sum_depth = addscoreref.device_depths(gpu, n, m, q, block)
        _REFS[key] = addscoreref.addscore_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], yv, wv, link,
                                                    pr["R"] if isinstance(R, str) else R, cand, depth, depth_score,
                                                    sum_depth)
    return _REFS[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_u_d_s_a_and_the_cross_information_are_within_the_bounds(gpu, dt, layout):
    for ci, case in enumerate(DEV_CASES):
        n, p, m, kind, block = case
        pr = _problem(dt, n, m, p)
        t = _tensor(dt, layout, n, m, p)
        assert tuple(t.shape) == (n, p)
        link = LINKS[ci % 3]
        fi, wi = ci % 4, (ci + ci // 3) % 5
        y, w, yv, wv = _forms(pr, link, fi, wi)
        ref = _ref(gpu, dt, case, link, yv, wv, fi == 3)
        cand = _cand(pr, p, kind)
        got = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w, factor=pr["R"],
                                  candidates=cand, want_cross=True, candidate_block=block)
        what = "%s %s n=%d p=%d m=%d %s %s y%d w%d" % (dt, layout, n, p, m, kind, link, fi, wi)
        q = p if cand is None else cand.size
        assert got["cross"].shape == (q, m + 1) and got["u"].shape == (q,)
        assert np.array_equal(got["columns"], np.arange(p) if cand is None else cand)
        addscoreref.check_vectors(got, ref, what)
        # info, score, loss and sum_w are information_device's, bit for bit
        inf = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w)
        assert np.array_equal(got["info"], inf["info"]) and np.array_equal(got["score"], inf["score"]), what
        assert got["loss"] == inf["loss"] and got["sum_w"] == inf["sum_w"], what
        if kind == "support" and m > 0:  # the support as candidates: u is the score, C is the information
            assert (np.abs(got["u"].astype(LD) - ref["score"][1:]) <= ref["bu"]).all(), what
        # want_cross=False and factor flag: nothing else changes
        if ci in (5, 9):
            again = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w, factor=pr["R"],
                                        candidates=cand, candidate_block=block)
            assert "cross" not in again
            for k in ("u", "d", "s", "a"):
                assert np.array_equal(again[k], got[k]), (what, k)


@pytest.mark.parametrize("layout", ["C", "F"])
def test_the_largest_support_and_one_past_it(gpu, layout):
    n, p, m = 127, 1040, 1023
    case = (n, p, m, "scattered", 0)
    pr = _problem("f64", n, m, p)
    t = _tensor("f64", layout, n, m, p)
    y, w = pr["ys"]["logistic"], pr["w"]
    ref = _ref(gpu, "f64", case, "logistic", y, w, False)
    got = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="logistic", weight=w, factor=pr["R"],
                              candidates=_cand(pr, p, "scattered"), want_cross=True)
    addscoreref.check_vectors(got, ref, "m + 1 = 1024 " + layout)
    everything = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="logistic", weight=w, factor=pr["R"])
    sel = _cand(pr, p, "scattered")
    for k in ("u", "d", "s", "a"):  # all 1040 candidates (another row split): the listed ones agree to rounding
        assert np.allclose(everything[k][sel], got[k], rtol=1e-10, atol=1e-12 * np.abs(got[k]).max()), k
    with pytest.raises(gpu.BessxError) as e:
        gpu.addscore_device(t, np.arange(1024), np.zeros(1024), 0.0, y, link="logistic", factor=np.eye(1025))
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)


def test_same_call_same_bits_and_every_layout_gives_the_same_bits(gpu):
    n, p, m = 4097, P, 31
    pr = _problem("f64", n, m, p)
    y, w = _dev(pr["ys"]["poisson"]), _dev(pr["w"])
    torch.cuda.synchronize()
    first = None
    for layout in LAYOUTS:
        t = _tensor("f64", layout, n, m, p)
        a = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w, factor=pr["R"],
                                want_cross=True)
        b = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w, factor=pr["R"],
                                want_cross=True)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w, factor=pr["R"],
                                    want_cross=True, stream=s.cuda_stream)
        for other in (b, c):
            for k in ("u", "d", "s", "a", "cross", "info", "score"):
                assert np.array_equal(a[k], other[k]), (layout, k)
            assert a["loss"] == other["loss"] and a["sum_w"] == other["sum_w"]
        first = first or a
        for k in ("u", "d", "s", "a", "cross"):
            assert np.array_equal(a[k], first[k]), (layout, k)


@pytest.mark.parametrize("shape", TABLE_SHAPES, ids=lambda s: "n%d-m%d" % s)
def test_score_test_table_is_within_the_interval_of_the_reference(gpu, shape):
    n, m = shape
    si = TABLE_SHAPES.index(shape)
    for li, link in enumerate(LINKS):
        dt = "f32" if (si + li) % 4 == 3 else "f64"
        layout = LAYOUTS[(si + 2 * li) % 5]
        pr = _problem(dt, n, m, P, signal=True)
        t = _tensor(dt, layout, n, m, P, signal=True)
        fi, wi = (si + li) % 4, (si + 2 * li) % 5
        y, w, yv, wv = _forms(pr, link, fi, wi)
        got = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w)
        what = "%s %s n=%d m=%d %s y%d w%d" % (dt, layout, n, m, link, fi, wi)
        assert got["positive_definite"], what
        R, pd = gpu.info_factor(got["info"])
        ref = _ref(gpu, dt, (n, P, m, None, 0), link, yv, wv, fi == 3, signal=True, R=R)
        addscoreref.check_vectors(got, ref, what)
        table = gpu.score_test_table(got, link)
        planted = [] if pr["planted"] is None else [pr["planted"]]
        st = addscoreref.statistic_reference(ref, planted=planted)
        addscoreref.check_table(table, st, what)
        assert np.array_equal(np.nonzero(table["in_model"])[0], pr["cols"]), what
        assert int(np.nanargmin(table["p_value"])) == pr["sig"], what
        for j in planted:  # x_j = x_a + 2^-10 noise: variance* / d* is about 2^-20
            assert st["ratio"][j] < 1e-4, what


def test_identity_statistic_times_dispersion_is_the_drop_of_a_longdouble_refit(gpu):
    """(u - a)^2 / (d - s) = RSS_A - RSS_{A + j} for the identity link, whatever beta is: both sides only see the part
    of x_j and of y that is orthogonal to the support.  Reference: weighted least squares refitted in longdouble for
    every candidate.  Bound: the interval of addscoreref for adj^2 / variance plus the refit's own cancellation error,
    64 * 2^-64 * RSS_A (two residual sums of squares of that size are subtracted in longdouble)."""
    n, m = 127, 14
    pr = _problem("f64", n, m, P, signal=True)
    t = _tensor("f64", "F", n, m, P, signal=True)
    y, w = pr["ys"]["identity"], pr["w"]
    got = gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="identity", weight=w)
    R, pd = gpu.info_factor(got["info"])
    assert pd
    ref = _ref(gpu, "f64", (n, P, m, None, 0), "identity", y, w, False, signal=True, R=R)
    st = addscoreref.statistic_reference(ref, planted=[pr["planted"]])
    table = gpu.score_test_table(got, "identity")
    X, yl, wl = pr["vals"].astype(LD), y.astype(LD), w.astype(LD)
    Z = np.concatenate([np.ones((n, 1), dtype=LD), X[:, pr["cols"]]], axis=1)

    def rss(A):
        Aw = A * wl[:, None]
        b = inforef.ld_inverse_spd(A.T @ Aw) @ (Aw.T @ yl)
        return (wl * (yl - A @ b) ** 2).sum()

    rss_a = rss(Z)
    worst = 0.0
    for j in np.nonzero(st["ok"])[0]:
        drop = rss_a - rss(np.concatenate([Z, X[:, j:j + 1]], axis=1))
        have = LD(table["statistic"][j]) * LD(table["dispersion"])
        phi = st["dispersion"]
        lo, hi = st["lo"][j] * phi * (1 - LD(1e-12)), st["hi"][j] * phi * (1 + LD(1e-12))
        allow = (hi - lo) + LD(64) * LD(2.0) ** -64 * rss_a
        worst = max(worst, float(abs(have - drop) / allow))
        assert abs(have - drop) <= allow, (j, float(have), float(drop), float(allow))
    print("%d candidates, largest |statistic * dispersion - drop| / allowance %.3e" % (int(st["ok"].sum()), worst))


@pytest.mark.parametrize("name", ["PdasLm", "PdasLogistic", "PdasPoisson"])
def test_estimator_score_tests_on_a_device_matrix_agree_with_the_numpy_route(gpu, name):
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
    dev, host = est.score_tests(Xd, _dev(y)), est.score_tests(X, y)
    assert np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    assert np.array_equal(dev["in_model"], host["in_model"]) and np.array_equal(dev["columns"], np.arange(p))
    b, c0 = est.beta[cols], float(np.ravel(est.coef0)[0])
    info_d = gpu.information_device(Xd, cols, b, c0, y, link=link)["info"]
    info_h = linear.bess_base._information_host(link, X[:, cols], b, c0, y, np.ones(n))["info"]
    sts = []
    for info, depths, tb in ((info_d, addscoreref.device_depths(gpu, n, cols.size, p), dev), (info_h, (n, n, n), host)):
        R, pd = gpu.info_factor(info)
        assert pd
        ref = addscoreref.addscore_reference(X, cols, b, c0, y, None, link, R, None, *depths)
        st = addscoreref.statistic_reference(ref)
        addscoreref.check_table(tb, st, name)
        sts.append(st)
    ok = sts[0]["ok"]
    width = (sts[0]["hi"] - sts[0]["lo"]) + (sts[1]["hi"] - sts[1]["lo"]) + np.abs(sts[0]["stat"] - sts[1]["stat"])
    assert (np.abs(sts[0]["stat"] - sts[1]["stat"])[ok] <= LD(1e-9) * sts[0]["stat"][ok] + LD(1e-12)).all()
    assert (np.abs(dev["statistic"] - host["statistic"]).astype(LD)[ok] <= width[ok]).all()
    left_out = np.setdiff1d(np.nonzero(truth)[0], cols)
    assert left_out.size >= 1 and int(np.nanargmin(dev["p_value"])) in left_out
    assert dev["p_value"][left_out].max() < 1e-3
    sub = est.score_tests(Xd, y, candidates=left_out)
    assert np.array_equal(sub["columns"], left_out)
    assert np.allclose(sub["statistic"], dev["statistic"][left_out], rtol=1e-9)  # (another row split: not the same bits)


def test_a_nan_outside_the_view_is_never_read_and_one_inside_propagates(gpu):
    n, p, m = 127, P, 16
    pr = _problem("f64", n, m, p)
    cand = np.sort(np.random.default_rng(2).choice(np.setdiff1d(np.arange(p), pr["cols"]), 20, replace=False))
    vals = pr["vals"].copy()
    other = np.setdiff1d(np.arange(p), np.concatenate([pr["cols"], cand]))
    vals[:, other] = np.nan  # columns that are neither in the support nor candidates
    ref = addscoreref.addscore_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], pr["ys"]["logistic"], pr["w"],
                                         "logistic", pr["R"], cand, *addscoreref.device_depths(gpu, n, m, cand.size))
    for layout in ("C", "F"):
        base, view = _embed(layout, vals)
        got = gpu.addscore_device(view(_dev(base)), pr["cols"], pr["beta"], pr["c"], pr["ys"]["logistic"], link="logistic",
                                  weight=pr["w"], factor=pr["R"], candidates=cand, want_cross=True)
        addscoreref.check_vectors(got, ref, "NaN outside " + layout)
        inside = pr["vals"].copy()
        inside[77, cand[3]] = np.nan  # one candidate's column: that candidate alone is NaN
        base, view = _embed(layout, inside)
        got = gpu.addscore_device(view(_dev(base)), pr["cols"], pr["beta"], pr["c"], pr["ys"]["logistic"], link="logistic",
                                  weight=pr["w"], factor=pr["R"], candidates=cand)
        want = np.arange(cand.size) == 3
        for k in ("u", "d", "s", "a"):
            assert np.array_equal(np.isnan(got[k]), want), (layout, k)


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    t = _tensor("f64", "C", n, m, P)
    y, w = pr["ys"]["logistic"], _dev(pr["w"])

    def call():
        gpu.addscore_device(t, pr["cols"], pr["beta"], pr["c"], y, link="logistic", weight=w, factor=pr["R"])
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
