"""Held-out evaluation on an X already in GPU memory (bessx_eval_device, bess_amd/csrc/bessx_k_eval.hip) against NumPy in
np.longdouble on the host copy of the same values.  The bound is derived in tests/evalref.py; `correct` is compared
exactly after evalref.label_precondition has held on every row of every case (weights are multiples of 1/8, so sums of
weights are exact in fp64).  Where two routes are compared with each other (device against host NumPy) each is within its
bound of the exact value, so they agree within twice that bound.

Resource accounting: counters 38 / 39 (live bytes) are back at their earlier values after a call.  Counter 40 counts the
allocation REQUESTS of the process so far and only grows; the test pins what a call adds to it (the same for every
call of the same kind), which is what shows that the call's buffers came from the library's owner type."""
import ctypes

import numpy as np
import pytest

import evalref
from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
LINKS = ["identity", "logistic", "poisson"]
P = 600
NS, MS, RS = (1, 127, 4097), (0, 1, 7, 200, P), (1, 3, 5, 256)


def _cases(n):
    """Every m at R = 5; every R at n = 1 and 127 with every m, and at n = 4097 with m = 7 and 200 (the longdouble
    reference of the full cross product would take minutes), plus the corners (m = 0, R = 1), (m = 1, R = 256) and
    (m = p, R = 256) at n = 4097."""
    out = [(m, R) for m in MS for R in RS if R == 5 or n <= 127 or m in (7, 200)]
    return out + ([(0, 1), (1, 256), (P, 256)] if n == 4097 else [])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _embed(layout, vals):
    """(base host array that holds vals in the layout under test, NaN everywhere else; base tensor -> the n x p view)"""
    n, p = vals.shape
    if layout == "C":  # row-major
        return vals.copy(), (lambda t: t)
    if layout == "F":  # column-major with a padded leading dimension: aligned columns (the 16-byte loads)
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


_PROBLEMS, _REFS = {}, {}


def _loss_ref(key, pr, yref, w, link):
    """evalref.loss_reference, computed once per distinct set of values (the layouts share them)"""
    if key not in _REFS:
        _REFS[key] = evalref.loss_reference(pr["eta"], pr["delta"], yref, w, link)
    return _REFS[key]


def _problem(dt, n, m, R):
    """One problem per (dtype, n, m, R), the same logical values under every layout: the design, a model whose linear
    predictor has a standard deviation of about 1.5 (exp stays finite), the responses of the three families (shared and
    per model), weights, and the longdouble eta* / Delta -- the expensive part of the reference, computed once."""
    key = (dt, n, m, R)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + R + (7 if dt == "f32" else 0))
        if (dt, n) not in _PROBLEMS:
            _PROBLEMS[(dt, n)] = np.random.default_rng(n + (1 if dt == "f32" else 0)).standard_normal((n, P)).astype(DT[dt])
        vals = _PROBLEMS[(dt, n)]
        cols = np.sort(rng.choice(P, m, replace=False)).astype(np.int32)
        B = rng.standard_normal((m, R)) * (1.5 / np.sqrt(max(m, 1)))
        B[rng.uniform(size=(m, R)) < 0.2] = 0.0  # (models that do not use every column of the union)
        c = rng.standard_normal(R) * 0.5 + 0.3
        eta, delta = evalref.eta_reference(vals, cols, B, c)
        e64 = eta.astype(np.float64)
        ys = {"identity": e64 + rng.standard_normal((n, R)),
              "logistic": np.where(rng.uniform(size=(n, R)) < 0.1, rng.choice([0.25, 0.75], (n, R)),
                                   (rng.uniform(size=(n, R)) < 1 / (1 + np.exp(-e64))).astype(float)),
              "poisson": rng.poisson(np.exp(np.clip(e64, -5, 3))).astype(float)}
        w = rng.integers(1, 17, n) / 8.0
        _PROBLEMS[key] = dict(vals=vals, cols=cols, B=B, c=c, eta=eta, delta=delta, ys=ys, w=w)
    return _PROBLEMS[key]


def _y_forms(pr, link, mode):
    """(y as passed, y of the reference) for one column shared by the models or one per model, alternating between
    host arrays, float64 device arrays (row-major and a strided view) and float32 device arrays over the cases."""
    Y = pr["ys"][link]
    R = Y.shape[1]
    if mode == "shared":
        y = Y[:, 0].copy()
        forms = [y, _dev(y), _dev(np.column_stack([y, y]))[:, 1], _dev(y.astype(np.float32))]
    else:
        forms = [Y, _dev(Y), _dev(np.asfortranarray(Y).T.copy()).T, _dev(Y.astype(np.float32))]
        y = Y
    return forms, y, R


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_losses_are_within_the_bound_and_correct_counts_are_exact(gpu, dt, layout):
    ncalls = 0
    for n in NS:
        base, view = _embed(layout, _problem(dt, n, 0, 5)["vals"])
        t = view(_dev(base))
        assert tuple(t.shape) == (n, P)
        for k, (m, R) in enumerate(_cases(n)):
            pr = _problem(dt, n, m, R)
            wforms = [None, pr["w"], _dev(pr["w"]), _dev(pr["w"].astype(np.float32))]
            for li, link in enumerate(LINKS):
                for mi, mode in enumerate(("shared", "per_model")):
                    yforms, yref, _ = _y_forms(pr, link, mode)
                    for wi in range(3):  # weights: none, host, device
                        wgiven = wforms[wi] if wi < 2 else wforms[2 + (k + li) % 2]
                        fi = (k + li + mi + wi) % 4
                        y = yforms[fi]
                        yr = yref.astype(np.float32) if fi == 3 else yref  # (float32 on the device: the rounded values)
                        what = "%s %s n=%d m=%d R=%d %s %s w=%d" % (dt, layout, n, m, R, link, mode, wi)
                        ref = _loss_ref((dt, n, m, R, link, mode, wi > 0, fi == 3), pr, yr,
                                        None if wi == 0 else pr["w"], link)
                        got = gpu.evaluate_device(t, pr["cols"], pr["B"], pr["c"], y, link=link, weight=wgiven)
                        ncalls += 1
                        assert isinstance(got["loss"], np.ndarray) and got["loss"].shape == (R,)
                        evalref.check_loss(got["loss"], ref, what)
                        assert got["sum_w"] == (float(n) if wi == 0 else float(ref["sum_w"])), what
                        if link == "logistic":
                            evalref.label_precondition(ref, what)
                            assert np.array_equal(got["correct"].astype(LD), ref["correct"]), what
                        else:
                            assert "correct" not in got
                        if m == 0:  # the closed form: every row has eta = c
                            assert np.array_equal(pr["eta"].astype(np.float64), np.broadcast_to(pr["c"], (n, R)))
    print("%s %s: %d calls" % (dt, layout, ncalls))


def _bits(a):
    return np.ascontiguousarray(_host(a)).view(np.int64 if _host(a).dtype.itemsize == 8 else np.int32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("link", LINKS)
def test_the_same_call_twice_gives_the_same_bits_and_nothing_is_written(gpu, layout, link):
    n, m, R = 4097, 200, 256
    pr = _problem("f64", n, m, R)
    base, view = _embed(layout, pr["vals"])
    tb = _dev(base)
    t = view(tb)
    y, w = _dev(pr["ys"][link]), _dev(pr["w"])
    x0, y0, w0 = _bits(tb).copy(), _bits(y).copy(), _bits(w).copy()
    a = gpu.evaluate_device(t, pr["cols"], pr["B"], pr["c"], y, link=link, weight=w)
    b = gpu.evaluate_device(t, pr["cols"], pr["B"], pr["c"], y, link=link, weight=w)
    for k in a:
        assert np.array_equal(_bits(np.atleast_1d(a[k])), _bits(np.atleast_1d(b[k]))), k
    assert np.array_equal(_bits(tb), x0) and np.array_equal(_bits(y), y0) and np.array_equal(_bits(w), w0)


def test_a_call_on_a_side_stream_sees_the_work_queued_there_before_it(gpu):
    n, m, R = 4097, 200, 5
    pr = _problem("f64", n, m, R)
    src, y = _dev(pr["vals"]), _dev(pr["ys"]["identity"])
    want = gpu.evaluate_device(src, pr["cols"], pr["B"], pr["c"], y)
    Xd = torch.zeros_like(src)
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(40):  # tens of milliseconds of work in front of the copy
            a = a @ a
            a = a / a.abs().max()
        Xd.copy_(src)
        got = gpu.evaluate_device(Xd, pr["cols"], pr["B"], pr["c"], y, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got["loss"]), _bits(want["loss"]))


@pytest.mark.parametrize("layout", ["C", "F", "two_strides"])
@pytest.mark.parametrize("link", LINKS)
def test_a_nan_reaches_exactly_the_models_that_use_its_column(gpu, layout, link):
    n, m, R = 4097, 200, 256
    pr = _problem("f64", n, m, R)
    y = pr["ys"][link]
    clean = gpu.evaluate_device(_embed_dev(layout, pr["vals"]), pr["cols"], pr["B"], pr["c"], y, link=link)
    assert np.isfinite(clean["loss"]).all()
    k = 57
    uses = pr["B"][k] != 0.0
    assert uses.any() and not uses.all()
    vals = pr["vals"].copy()
    vals[1234, pr["cols"][k]] = np.nan
    got = gpu.evaluate_device(_embed_dev(layout, vals), pr["cols"], pr["B"], pr["c"], y, link=link)
    assert np.array_equal(np.isnan(got["loss"]), uses)
    assert np.array_equal(_bits(got["loss"][~uses]), _bits(clean["loss"][~uses]))
    # ... and an inf likewise stays with them
    vals[1234, pr["cols"][k]] = np.inf
    got = gpu.evaluate_device(_embed_dev(layout, vals), pr["cols"], pr["B"], pr["c"], y, link=link)
    assert np.array_equal(~np.isfinite(got["loss"]), uses)
    # a NaN in every column outside the support changes nothing
    vals = pr["vals"].copy()
    outside = np.setdiff1d(np.arange(P), pr["cols"])
    vals[:, outside] = np.nan
    got = gpu.evaluate_device(_embed_dev(layout, vals), pr["cols"], pr["B"], pr["c"], y, link=link)
    assert np.array_equal(_bits(got["loss"]), _bits(clean["loss"]))
    # a NaN in y (per model) or in a weight stays with its model / reaches every model
    Y = y.copy()
    Y[77, 3] = np.nan
    got = gpu.evaluate_device(_embed_dev(layout, pr["vals"]), pr["cols"], pr["B"], pr["c"], Y, link=link)
    assert np.array_equal(np.isnan(got["loss"]), np.arange(R) == 3)
    w = pr["w"].copy()
    w[5] = np.nan
    got = gpu.evaluate_device(_embed_dev(layout, pr["vals"]), pr["cols"], pr["B"], pr["c"], y, link=link, weight=w)
    assert np.isnan(got["loss"]).all() and np.isnan(got["sum_w"])


def _embed_dev(layout, vals):
    base, view = _embed(layout, vals)
    return view(_dev(base))


def _c_call(gpu, x, n, p, y_dev=None, y_host=None, w_dev=None, xrs=None, yrs=1, ws=1):
    cols, B, c0 = np.array([1, 3], dtype=np.int32), np.array([1.0, 2.0]), np.array([0.5])
    a = gpu.EvalInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = x, 0, (p if xrs is None else xrs), 1, n, p
    a.cols, a.m, a.B, a.coef0, a.R, a.link = gpu._ip(cols), 2, gpu._dp(B), gpu._dp(c0), 1, 0
    a.y_row_stride, a.y_col_stride, a.y_cols = yrs, 0, 1
    if y_dev is not None:
        a.y_dev, a.y_dtype = y_dev, 0
    else:
        a.y_host = gpu._dp(y_host)
    if w_dev is not None:
        a.weight_dev, a.weight_dtype, a.weight_stride = w_dev, 0, ws
    loss, sw = np.full(1, -7.0), ctypes.c_double(-7.0)
    rc = gpu.lib().bessx_eval_device(ctypes.byref(a), gpu._dp(loss), None, ctypes.byref(sw))
    assert rc == 0 or (loss[0] == -7.0 and sw.value == -7.0)  # (a refused call writes nothing)
    return rc, gpu.last_error()


def test_bad_device_pointers_are_argument_errors_not_faults(gpu):
    n, p = 64, 5
    X = torch.randn((n, p), dtype=torch.float64, device="cuda")
    y, w = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.ones(n, dtype=torch.float64, device="cuda")
    yh, far = np.zeros(n), 1 << 26  # (a stride that leaves any allocation: torch hands out parts of larger blocks)
    assert _c_call(gpu, X.data_ptr(), n, p, y_host=yh)[0] == 0
    assert _c_call(gpu, X.data_ptr(), n, p, y_dev=y.data_ptr(), w_dev=w.data_ptr())[0] == 0
    host = np.zeros((n, p))
    for rc, msg in [
        _c_call(gpu, host.ctypes.data, n, p, y_host=yh),                                # x: a host pointer
        _c_call(gpu, X.data_ptr(), n, p, y_dev=yh.ctypes.data),                         # y: a host pointer
        _c_call(gpu, X.data_ptr(), n, p, y_host=yh, w_dev=yh.ctypes.data),              # weight: a host pointer
        _c_call(gpu, X.data_ptr(), n, p, y_host=yh, xrs=far),                           # x: reaches past its allocation
        _c_call(gpu, X.data_ptr(), n, p, y_dev=y.data_ptr(), yrs=far),                  # y: likewise
        _c_call(gpu, X.data_ptr(), n, p, y_host=yh, w_dev=w.data_ptr(), ws=far),        # weight: likewise
    ]:
        assert rc == 1, msg  # BESSX_ERR_ARG
        assert "device" in msg, msg


def test_live_bytes_return_and_requests_grow_by_a_fixed_count(gpu):
    pr = _problem("f64", 4097, 200, 5)
    t, y, w = _dev(pr["vals"]), _dev(pr["ys"]["logistic"]), _dev(pr["w"])
    call = lambda **kw: gpu.evaluate_device(t, pr["cols"], pr["B"], pr["c"], y, link="logistic", **kw)  # noqa: E731
    call(weight=w)
    before = gpu.process_counters()
    call(weight=w)
    mid = gpu.process_counters()
    call(weight=w)
    after = gpu.process_counters()
    for k in ("live_device_bytes", "live_pinned_bytes"):
        assert before[k] == mid[k] == after[k], k
    step = mid["allocation_requests"] - before["allocation_requests"]
    assert step > 0 and after["allocation_requests"] - mid["allocation_requests"] == step
    ms, gbps = gpu.op_eval_bench(t, pr["cols"], R=5, link="logistic", repeats=2)
    assert ms > 0 and gbps > 0
    assert gpu.process_counters()["live_device_bytes"] == before["live_device_bytes"]


# ----------------------------------------------------------------------------------------------------------------
# the path workflow: fit on the training rows, choose the candidate on validation rows in GPU memory
# ----------------------------------------------------------------------------------------------------------------
def _split_reference(result, Xv, yv, link):
    refs = []
    for r in range(len(result["cand_coef0"])):
        sup = result["cand_support"][r]
        sup = sup[sup >= 0]
        order = np.argsort(sup)
        eta, delta = evalref.eta_reference(Xv, sup[order], result["cand_beta"][r][:sup.size][order],
                                           [result["cand_coef0"][r]])
        refs.append(evalref.loss_reference(eta, delta, yv, None, link))
    return (np.array([float(f["loss"][0]) for f in refs], dtype=LD), np.array([f["bound"][0] for f in refs], dtype=LD),
            refs)


def _split_case(family):
    """Training rows, validation rows and the link.  Checked on the CPU for these seeds: the two smallest reference
    losses on the validation rows are further apart than the sum of their bounds."""
    if family == "lm":
        X, y, _, _ = synth.make_lm(3000, 200, 8, seed=301)
        return X[:2000], y[:2000], X[2000:], y[2000:], "identity", 1
    X, y, _, _ = synth.make_logistic(3000, 120, 5, seed=302)
    return X[:2000], y[:2000], X[2000:], y[2000:], "logistic", 2


@pytest.mark.parametrize("family", ["lm", "logistic"])
@pytest.mark.parametrize("dev_dtype", ["f64", "f32"])
def test_candidates_of_a_path_are_chosen_on_validation_rows_in_gpu_memory(gpu, family, dev_dtype):
    Xt, yt, Xv, yv, link, model = _split_case(family)
    if dev_dtype == "f32":
        Xv = Xv.astype(np.float32)
    kw = {} if model == 1 else dict(data_type=2, model_type=2)
    with gpu.Session(Xt, yt, **kw) as s:
        result = s.sequential_path(np.arange(1, 21), ic_type=3)
    R = len(result["cand_coef0"])
    assert R == 20
    want, bound, refs = _split_reference(result, Xv, yv, link)
    losses, best = gpu.evaluate_candidates(result, _dev(Xv), _dev(yv), link=link)
    assert isinstance(losses, np.ndarray) and losses.shape == (R,) and isinstance(best, int)
    err = np.abs(losses.astype(LD) - want)
    print("%s %s: max err / bound %.3e" % (family, dev_dtype, float((err / bound).max())))
    assert (err <= bound).all()
    two = np.argsort(want)[:2]
    assert want[two[1]] - want[two[0]] > bound[two[0]] + bound[two[1]], "choose another seed"
    assert best == int(two[0])
    # the same numbers as R separate calls over each candidate's own support would give, within both bounds
    sup = result["cand_support"][best]
    sup = sup[sup >= 0]
    order = np.argsort(sup)
    one = gpu.evaluate_device(_dev(Xv), sup[order], result["cand_beta"][best][:sup.size][order],
                              [result["cand_coef0"][best]], yv, link=link)
    assert abs(LD(one["loss"][0]) - LD(losses[best])) <= 2 * bound[best]


# ----------------------------------------------------------------------------------------------------------------
# the estimators
# ----------------------------------------------------------------------------------------------------------------
def _est_reference(est, X, y, w, link):
    beta = np.asarray(est.beta).reshape(X.shape[1], -1)
    cols = np.nonzero(beta.any(axis=1))[0]
    eta, delta = evalref.eta_reference(X, cols, beta[cols], np.reshape(est.coef0, -1))
    return evalref.loss_reference(eta, delta, y, w, link)


def _plain(v):
    return isinstance(v, float) or (isinstance(v, np.ndarray) and v.dtype == np.float64)


def _compare_routes(est, Xh, yh, wh, link, derived):
    """evaluate on the device X (y and weight on the device too) against the host route on the same values."""
    ref = _est_reference(est, Xh, yh, wh, link)
    host = est.evaluate(Xh, yh, weight=wh)
    dev = est.evaluate(_dev(Xh), _dev(yh), weight=None if wh is None else _dev(wh))
    assert set(dev) == set(host)
    assert all(_plain(v) for v in dev.values()), {k: type(v) for k, v in dev.items()}
    L_h, L_d = np.reshape(host["loss"], -1).astype(LD), np.reshape(dev["loss"], -1).astype(LD)
    print("%s: max |dev - host| / bound %.3e" % (type(est).__name__, float((np.abs(L_d - L_h) / ref["bound"]).max())))
    assert (np.abs(L_d - L_h) <= 2 * ref["bound"]).all()
    assert evalref.within(dev["loss"], ref).all() and evalref.within(host["loss"], ref).all()
    assert np.array_equal(np.reshape(dev["n_eff"], -1), np.reshape(host["n_eff"], -1))
    # the derived figures divide the loss by a term in y alone, computed by the same host code on both routes
    for name, scale in derived.items():
        d, h = np.reshape(dev[name], -1).astype(LD), np.reshape(host[name], -1).astype(LD)
        assert (np.abs(d - h) <= 2 * ref["bound"] * scale(host) * (1 + 1e-9)).all(), name
    score_d = est.score(_dev(Xh), yh, weight=wh)  # (a host y with a device X)
    assert _plain(score_d)
    return dev, host, ref, score_d


def _tss(est, Y, w):
    Y = np.reshape(Y, (len(Y), -1))
    w = np.ones(len(Y)) if w is None else w
    ybar = (w[:, None] * Y).sum(axis=0) / w.sum()
    return (w[:, None] * (Y - ybar) ** 2).sum(axis=0)


@pytest.mark.parametrize("weighted", [False, True])
def test_lm_estimators_evaluate_on_the_device_like_on_the_host(gpu, weighted):
    rng = np.random.default_rng(90)
    X, y, _, _ = synth.make_lm(3000, 80, 6, seed=91)
    w = rng.integers(1, 17, 1000) / 8.0 if weighted else None
    est = linear.PdasLm(sequence=list(range(1, 11)))
    est.fit(_dev(X[:2000]), y[:2000])
    Xv, yv = X[2000:], y[2000:]
    tss = _tss(est, yv, w)
    dev, host, ref, score = _compare_routes(est, Xv, yv, w, "identity",
                                            {"mse": lambda h: 1.0 / h["n_eff"], "r2": lambda h: 1.0 / tss})
    assert score == est.evaluate(_dev(Xv), yv, weight=w)["r2"] and 0.5 < score <= 1.0
    # 8 responses against one design
    Y = np.column_stack([y + 0.1 * k * rng.standard_normal(3000) for k in range(8)])
    multi = linear.PdasLm(sequence=list(range(1, 11)))
    multi.fit(_dev(X[:2000]), Y[:2000])
    Yv = Y[2000:]
    tss = _tss(multi, Yv, w)
    dev, host, ref, score = _compare_routes(multi, Xv, Yv, w, "identity",
                                            {"mse": lambda h: 1.0 / h["n_eff"], "r2": lambda h: 1.0 / tss})
    assert dev["loss"].shape == (8,) and score.shape == (8,)


@pytest.mark.parametrize("weighted", [False, True])
def test_logistic_and_poisson_estimators_evaluate_on_the_device_like_on_the_host(gpu, weighted):
    rng = np.random.default_rng(92)
    w = rng.integers(1, 17, 500) / 8.0 if weighted else None
    X, y, _, _ = synth.make_logistic(1500, 40, 4, seed=74)
    est = linear.PdasLogistic(sequence=list(range(1, 7)))
    est.fit(_dev(X[:1000]), y[:1000])
    dev, host, ref, score = _compare_routes(est, X[1000:], y[1000:], w, "logistic", {"deviance": lambda h: 2.0})
    evalref.label_precondition(ref)
    assert dev["accuracy"] == host["accuracy"] == float(ref["correct"][0]) / float(ref["sum_w"]) == score
    assert score > 0.6

    X, y, _, _ = synth.make_poisson(1500, 40, 4, seed=75)
    est = linear.PdasPoisson(sequence=list(range(1, 7)))
    est.fit(_dev(X[:1000]), y[:1000])
    yv = y[1000:]
    wl = np.ones(500) if w is None else w
    ybar = (wl * yv).sum() / wl.sum()
    ylogy = np.where(yv > 0, yv * np.log(np.where(yv > 0, yv, 1.0)), 0.0)
    null = 2.0 * (wl * (ylogy - yv * np.log(ybar) - (yv - ybar))).sum()
    dev, host, ref, score = _compare_routes(est, X[1000:], yv, w, "poisson",
                                            {"deviance": lambda h: 2.0, "d2": lambda h: 2.0 / null})
    assert score == dev["d2"]


def test_cox_estimator_evaluates_to_none_for_a_device_x(gpu):
    X, obs, status, _, _ = synth.make_cox(400, 30, 3, seed=76)
    est = linear.PdasCox(sequence=[1, 2, 3])
    est.fit(_dev(X), np.column_stack([obs, status]))
    assert est.evaluate(_dev(X), np.column_stack([obs, status])) is None
    assert est.score(_dev(X), np.column_stack([obs, status])) is None
